"""The solve of one round's ILP (py/freddie_cluster.py run_ilp :347-592 with K = 2) behind a narrow interface: a plain callable
``solve(model, settings) -> (status, x, e)``.  The backend here is HiGHS through scipy.optimize.milp; where a Gurobi licence exists a
backend for it is another callable of the same shape.  Optimal solutions of equal cost may differ between solvers: HiGHS breaks ties
its own way, so the isoforms of a round can differ from Gurobi's where the optimum is not unique.

With K = 2 (isoform 0 is the garbage isoform, isoform 1 the round's) the reference's model is, over the remaining reps ("columns")
and the informative segments:
  x_i  binary   rep i is in the round's isoform (R2I[i][1]; R2I[i][0] = 1 - x_i)
  e_j  binary   segment j is in the isoform: the OR of the x_i over the reps that cover it (E2I_C1, a max constraint :440-445)
                    e_j >= x_i for every support entry, e_j <= sum of those x_i (no entry: e_j = 0)
  o_ij in [0,1] rep i is in, j is in, and C[i][j] = 1: a correction (OBJ_C1 :530-534), cost 1;  o_ij >= x_i + e_j - 1
  G_g  = sum of len_j e_j over the group's segments (GAPI_C1 :474-481), and per (column, gap of length l) the two big-M rows
                    (1 - epsilon) G_g - offset - (1 - x_i) MAX_LG <= l   (:482-489)
                    (1 + epsilon) G_g + offset + (1 - x_i) MAX_LG >= l   (:490-497)
  x_a + x_b <= 1 per incompatible pair (:505-511);  the garbage cost on 1 - x_i (:544).
``model`` = cluster_prep.round_model() of the problem plus ``garbage`` (a cost per column) and ``max_lg`` (the tint's summed segment
lengths).  The relative recycle model needs E2I_min and the reference's preprocess_ilp() sets no garbage cost for it: refused.

With K = 2 the model is a function of the chosen column set S alone: e = the OR of the chosen reps' I rows on the informative segments,
cost = sum over S of popcount(C_c & e) + the others' garbage costs, S without an incompatible pair, every gap row of a member holding.
greedy_incumbent() is a seeded greedy over exactly that (the definition the GPU's fclu_round_incumbents reproduces bit for bit); an
incumbent in ``model["incumbent"]`` = (cost, x) gives solve_round() an objective cutoff and, under settings["incumbent"] == "fallback",
the answer when the solve ends without a proven optimum (status INCUMBENT).  exact_small() enumerates all 2^R column sets of a problem
of at most 24 columns (the definition the GPU's fclu_round_exact reproduces bit for bit): a proven optimum with no matrix and no solver."""
import numpy as np

OPTIMAL, NO_SOLUTION, INCUMBENT = "OPTIMAL", "NO_SOLUTION", "INCUMBENT"
RECYCLE_MODELS = ("constant", "exons", "introns")
INCUMBENT_MODES = ("off", "cutoff", "fallback")


def check_settings(settings):
    if settings["recycle_model"] not in RECYCLE_MODELS:
        raise ValueError("recycle model %r: the solve supports %s (relative needs E2I_min and has no garbage cost in the reference either)"
                         % (settings["recycle_model"], ", ".join(RECYCLE_MODELS)))
    if settings.get("incumbent", "off") not in INCUMBENT_MODES:
        raise ValueError("incumbent mode %r: one of %s" % (settings["incumbent"], ", ".join(INCUMBENT_MODES)))


def build_rows(model, settings):
    """(cost, A as (data, rows, cols), lower, upper, upper bounds of the variables, constant of the objective): variables are the R
    columns' x, then the e of inf_seg, then one o per correction term."""
    R, inf_seg = model["n_cols"], model["inf_seg"]
    E = len(inf_seg)
    e_of = {j: R + k for k, j in enumerate(inf_seg)}
    terms = [(c, j) for c, segs in enumerate(model["corrections"]) for j in segs]
    n = R + E + len(terms)
    cost = np.zeros(n)
    cost[:R] = -np.asarray(model["garbage"], float)
    cost[R + E:] = 1.0
    ub = np.ones(n)
    data, rows, cols, lo, hi = [], [], [], [], []

    def row(entries, lower, upper):
        r = len(lo)
        for col, v in entries:
            data.append(v); rows.append(r); cols.append(col)
        lo.append(lower); hi.append(upper)

    for k, support in enumerate(model["support"]):
        if not support:
            ub[R + k] = 0.0
            continue
        for c in support:
            row([(R + k, 1.0), (c, -1.0)], 0.0, np.inf)
        row([(R + k, 1.0)] + [(c, -1.0) for c in support], -np.inf, 0.0)
    for t, (c, j) in enumerate(terms):
        row([(R + E + t, 1.0), (c, -1.0), (e_of[j], -1.0)], -1.0, np.inf)
    eps, off, big = settings["epsilon"], settings["offset"], model["max_lg"]
    for c, g, l in model["gap_rows"]:
        segs = model["group_segs"][g]
        row([(e_of[j], (1.0 - eps) * ln) for j, ln in segs] + [(c, float(big))], -np.inf, l + off + big)
        row([(e_of[j], (1.0 + eps) * ln) for j, ln in segs] + [(c, -float(big))], l - off - big, np.inf)
    for a, b in model["pairs"]:
        row([(a, 1.0), (b, 1.0)], -np.inf, 1.0)
    return cost, (data, rows, cols), np.array(lo), np.array(hi), ub, float(sum(model["garbage"]))


def garbage2(garbage):
    """Twice the garbage costs as ints; costs are multiples of 0.5 (and not negative), anything else is refused."""
    out = []
    for c, g in enumerate(garbage):
        g2 = int(round(2 * g))
        if g2 != 2 * g or g2 < 0 or g2 > 0x7fffffff:
            raise ValueError("garbage cost %r of column %d is not a multiple of 0.5 in [0, 2^30)" % (g, c))
        out.append(g2)
    return out


def _bits(x):
    while x:
        b = x & -x
        yield b.bit_length() - 1
        x ^= b


def greedy_incumbent(model, settings, max_seeds=64):
    """The seeded greedy incumbent of one round_model() dict (with ``garbage`` and ``max_lg``): dict(cost2, cost, start, members, x, e,
    grow_steps, repair_steps), or None when no start ends feasible.  Rows are Python ints over the segment numbers (only informative
    segments ever carry a bit).

    Starts: n = min(R, max_seeds); start k < n is {k * R // n}, start n is the empty set.
    Grow: with E = the OR of the members' I rows and cnt[j] = the members with C = 1 at j, every column outside S that conflicts with no
        member has N = I_c & ~E and delta2 = 2 * (popcount(C_c & (E | N)) + sum of cnt[j] over N) - g2_c; the smallest delta2 (then the
        smallest column) is added while it is negative.
    Repair: G_g = the group's lengths summed over the segments in E; a member's row (g, l) is violated when lo_f * G_g - offset > l or
        hi_f * G_g + offset < l (doubles, one rounded multiply and one rounded add; no tolerance, so whatever passes here passes the
        model's rows); while a member has a violated row the one with the most (then the smallest column) leaves and E is recomputed.
    Score: cost2 = the non-members' g2 + 2 * the members' popcount(C_c & E); the smallest cost2 wins, then the earliest start.  The
        model gives the rows of a column OUTSIDE the set a slack of max_lg and no more, so a gap longer than the tint can still need
        segments in E: a start with such a row violated -- the same test with offset + max_lg (one exact integer) for offset -- is
        not feasible and has no cost2.  (The empty set is feasible unless a gap is longer than offset + max_lg.)"""
    if max_seeds < 1:
        raise ValueError("max_seeds is %r: at least 1" % (max_seeds,))
    R = model["n_cols"]
    g2 = garbage2(model["garbage"])
    if len(g2) != R:
        raise ValueError("%d garbage costs for %d columns" % (len(g2), R))
    rows_i, rows_c, conf = [0] * R, [0] * R, [0] * R
    for j, support in zip(model["inf_seg"], model["support"]):
        for c in support:
            rows_i[c] |= 1 << j
    for c, segs in enumerate(model["corrections"]):
        for j in segs:
            rows_c[c] |= 1 << j
    for a, b in model["pairs"]:
        conf[a] |= 1 << b
        conf[b] |= 1 << a
    col_rows = [[] for _ in range(R)]
    for c, g, l in model["gap_rows"]:
        col_rows[c].append((g, l))
    lo_f, hi_f, offset = 1.0 - settings["epsilon"], 1.0 + settings["epsilon"], settings["offset"]
    out_offset = offset + int(model["max_lg"])
    n = min(R, max_seeds)
    best = None
    for k in range(n + 1):
        members, E, blocked, cnt, grow_steps, repair_steps = 0, 0, 0, {}, 0, 0

        def add(c):
            nonlocal members, E, blocked
            members |= 1 << c
            blocked |= conf[c]
            E |= rows_i[c]
            for j in _bits(rows_c[c]):
                cnt[j] = cnt.get(j, 0) + 1

        if k < n:
            add(k * R // n)
        for _ in range(R):
            pick = None
            for c in range(R):
                if (members | blocked) >> c & 1:
                    continue
                N = rows_i[c] & ~E
                d2 = 2 * (bin(rows_c[c] & (E | N)).count("1") + sum(cnt.get(j, 0) for j in _bits(N))) - g2[c]
                if pick is None or d2 < pick[0]:
                    pick = (d2, c)
            if pick is None or pick[0] >= 0:
                break
            add(pick[1])
            grow_steps += 1
        def violated(c, off):
            bad = 0
            for g, l in col_rows[c]:
                G = sum(ln for j, ln in model["group_segs"][g] if E >> j & 1)
                if lo_f * G - off > l or hi_f * G + off < l:
                    bad += 1
            return bad

        while members:
            worst = None
            for c in _bits(members):
                bad = violated(c, offset)
                if bad and (worst is None or bad > worst[0]):
                    worst = (bad, c)
            if worst is None:
                break
            members ^= 1 << worst[1]
            repair_steps += 1
            E = 0
            for c in _bits(members):
                E |= rows_i[c]
        if any(violated(c, out_offset) for c in range(R) if not members >> c & 1):
            continue
        cost2 = sum(g2[c] for c in range(R) if not members >> c & 1) + 2 * sum(bin(rows_c[c] & E).count("1") for c in _bits(members))
        if best is None or cost2 < best["cost2"]:
            best = dict(cost2=cost2, cost=cost2 / 2.0, start=k, members=list(_bits(members)), grow_steps=grow_steps, repair_steps=repair_steps,
                        x=[members >> c & 1 for c in range(R)], e=[E >> j & 1 for j in model["inf_seg"]])
    return best


EXACT_MAX_COLS = 24
_POPC16 = None


def _popcounts(v):
    """popcount of every element of an int64 array of values below 2^32."""
    global _POPC16
    if _POPC16 is None:
        t = np.zeros(1 << 16, np.int64)
        for b in range(16):
            t += (np.arange(1 << 16) >> b) & 1
        _POPC16 = t
    return _POPC16[v & 0xffff] + _POPC16[v >> 16]


def exact_small(model, settings, chunk=1 << 16):
    """The proven optimum of one round_model() dict (with ``garbage`` and ``max_lg``) of at most 24 columns by enumeration -- the
    definition the GPU's fclu_round_exact reproduces bit for bit: dict(cost2, cost, mask, members, x, e), or None when no subset is
    feasible.  e = the OR of the members' support (as solve_round()'s fallback computes it).

    Search: all subsets S of the R columns as masks 0 .. 2^R - 1, bit c = column c, over the transposed model: per informative segment
        the mask of its support and the mask of the columns with C = 1 there, per column the mask of the columns it conflicts with.
    Feasible (the yardstick's test, tests/round_util.py subset_cost): no pair of model["pairs"] inside S, and every gap row (c, g, l)
        holds: with G = the summed lengths of group g's segments whose support meets S and slack = 0 when c is in S, else max_lg, the row
        is violated when (1.0 - eps) * G - offset - slack > l + 1e-9 or (1.0 + eps) * G + offset + slack < l - 1e-9, in doubles, these
        operations in this order, none fused.  greedy_incumbent()'s test has no tolerance, because an incumbent must be feasible for
        everybody; a proven optimum must not exclude what the model admits: eps 0.15, offset 20, G = 200, l = 250 holds with equality
        in rationals, and in doubles 1.15 * 200 + 20 is below 250.
    Cost: cost2 = the g2 of the columns outside S + 2 * the sum over S of popcount(C_c & e).  The smallest cost2 wins, then the smallest
        mask as an integer.
    The masks are evaluated ``chunk`` at a time as numpy arrays (R = 12 is one chunk and takes milliseconds)."""
    R = model["n_cols"]
    if R > EXACT_MAX_COLS:
        raise ValueError("%d columns: exact_small takes %d at the most" % (R, EXACT_MAX_COLS))
    g2 = garbage2(model["garbage"])
    if len(g2) != R:
        raise ValueError("%d garbage costs for %d columns" % (len(g2), R))
    sup_of = {}
    sup, corr, conf = [], [0] * len(model["inf_seg"]), [0] * R
    for j, support in zip(model["inf_seg"], model["support"]):
        sup.append(sum(1 << c for c in support))
        sup_of[j] = sup[-1]
    place = {j: k for k, j in enumerate(model["inf_seg"])}
    for c, segs in enumerate(model["corrections"]):
        for j in segs:
            corr[place[j]] |= 1 << c
    for a, b in model["pairs"]:
        conf[a] |= 1 << b
        conf[b] |= 1 << a
    lo_f, hi_f, offset, max_lg = 1.0 - settings["epsilon"], 1.0 + settings["epsilon"], float(settings["offset"]), float(int(model["max_lg"]))
    used = sorted(set(g for _, g, _ in model["gap_rows"]))
    best = None
    for m0 in range(0, 1 << R, chunk):
        S = np.arange(m0, min(m0 + chunk, 1 << R), dtype=np.int64)
        ok = np.ones(S.size, bool)
        for c in range(R):
            if conf[c]:
                ok &= ~(((S >> c) & 1).astype(bool) & ((S & conf[c]) != 0))
        G = {}
        for g in used:
            total = np.zeros(S.size, np.int64)
            for j, ln in model["group_segs"][g]:
                total += np.where((S & sup_of.get(j, 0)) != 0, ln, 0)
            G[g] = total.astype(np.float64)
        for c, g, l in model["gap_rows"]:
            slack = np.where((S >> c) & 1, 0.0, max_lg)
            a = lo_f * G[g]
            a = a - offset
            a = a - slack
            b = hi_f * G[g]
            b = b + offset
            b = b + slack
            ok &= ~((a > float(l) + 1e-9) | (b < float(l) - 1e-9))
        if not ok.any():
            continue
        cost2 = np.zeros(S.size, np.int64)
        for c in range(R):
            cost2 += np.where((S >> c) & 1, 0, g2[c])
        for s_mask, c_mask in zip(sup, corr):
            if c_mask:
                cost2 += 2 * np.where((S & s_mask) != 0, _popcounts(S & c_mask), 0)
        key = np.where(ok, (cost2 << EXACT_MAX_COLS) | S, np.int64(1) << 62)
        k = int(key.min())
        if best is None or k < best:
            best = k
    if best is None:
        return None
    cost2, mask = best >> EXACT_MAX_COLS, best & ((1 << EXACT_MAX_COLS) - 1)
    x = [mask >> c & 1 for c in range(R)]
    return dict(cost2=cost2, cost=cost2 / 2.0, mask=mask, members=list(_bits(mask)), x=x,
                e=[int(any(x[c] for c in support)) for support in model["support"]])


def solve_round(model, settings):
    """(status, x, e): status OPTIMAL only for a proven optimum within timeout minutes (anything else is NO_SOLUTION, as :591-592),
    x a 0 / 1 per column, e a 0 / 1 per informative segment (beside model['inf_seg']).  The relative gap is 0: costs are multiples of
    0.5 and a relative gap would accept a worse isoform.  model["incumbent"] = (cost, x) of a feasible column set, when there is one,
    adds the row objective <= cost + 0.25 (the incumbent and every optimum stay feasible); under settings["incumbent"] == "fallback" a
    solve without a proven optimum returns (INCUMBENT, the incumbent's x, its e = the OR of the members' support)."""
    from scipy.optimize import Bounds, LinearConstraint, milp
    from scipy.sparse import csr_matrix
    check_settings(settings)
    R, E = model["n_cols"], len(model["inf_seg"])
    if R == 0:
        return OPTIMAL, [], [0] * E
    cost, (data, rows, cols), lo, hi, ub, _ = build_rows(model, settings)
    n = cost.size
    integrality = np.zeros(n)
    integrality[:R + E] = 1
    constraints = [LinearConstraint(csr_matrix((data, (rows, cols)), shape=(lo.size, n)), lo, hi)] if lo.size else []
    incumbent = model.get("incumbent")
    if incumbent is not None:                                # cost . v + sum(garbage) <= the incumbent's cost + 0.25
        constraints.append(LinearConstraint(csr_matrix(cost.reshape(1, n)), -np.inf, incumbent[0] + 0.25 - float(sum(model["garbage"]))))
    res = milp(cost, integrality=integrality, bounds=Bounds(np.zeros(n), ub), constraints=constraints,
               options=dict(time_limit=settings["timeout"] * 60, mip_rel_gap=0.0, disp=False))
    if res.status != 0 or res.x is None:
        if incumbent is not None and settings.get("incumbent", "off") == "fallback":
            x = [int(v) for v in incumbent[1]]
            return INCUMBENT, x, [int(any(x[c] for c in support)) for support in model["support"]]
        return NO_SOLUTION, None, None
    return OPTIMAL, [int(v > 0.5) for v in res.x[:R]], [int(v > 0.5) for v in res.x[R:R + E]]


def round_cost(model, x, e):
    """The objective's value of a solution: the chosen reps' corrections and the others' garbage costs."""
    on = {j for j, v in zip(model["inf_seg"], e) if v}
    return (sum(g for g, v in zip(model["garbage"], x) if not v) +
            sum(1 for c, segs in enumerate(model["corrections"]) if x[c] for j in segs if j in on))
