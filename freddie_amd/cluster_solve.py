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


BNB_MAX_COLS = 64
BNB_DEPTH = 6             # columns fixed by the task number: 64 tasks a problem.  On the cluster-many workload nearly every prefix is dropped at once
                          # (a problem of 60 columns counts a few hundred nodes), so 12 columns only add 4 096 one-node tasks a problem
BNB_NODE_CAP = 1024       # nodes a task may count: what keeps the longest launch under 50 ms at 64 columns while 98 % of the problems are still
                          # proved (profiles/cluster_bnb.txt; 4 096 proves them all but a launch takes longer than 50 ms)
BNB_WIDE_MAX_COLS = 1024  # exact_bnb_wide(): column sets of up to 16 words of 64 bits
_BNB_NONE = 1 << 62       # "no bound": no cost2 reaches it


def _popc(x):
    return bin(x).count("1")


def bnb_tables(model, settings, max_cols=BNB_MAX_COLS, who="exact_bnb"):
    """The transposed tables of exact_small() as Python ints of up to max_cols bits (bit c = column c): sup[k] and corr[k] per informative
    segment, conf[c] and g2[c] per column; the gap rows (column, group, l) and per group its segments as (support mask, length)."""
    R = model["n_cols"]
    if R > max_cols:
        raise ValueError("%d columns: %s takes %d at the most" % (R, who, max_cols))
    g2 = garbage2(model["garbage"])
    if len(g2) != R:
        raise ValueError("%d garbage costs for %d columns" % (len(g2), R))
    sup, corr, conf = [], [0] * len(model["inf_seg"]), [0] * R
    for support in model["support"]:
        sup.append(sum(1 << c for c in support))
    place = {j: k for k, j in enumerate(model["inf_seg"])}
    for c, segs in enumerate(model["corrections"]):
        for j in segs:
            if j in place:
                corr[place[j]] |= 1 << c
    for a, b in model["pairs"]:
        conf[a] |= 1 << b
        conf[b] |= 1 << a
    ccol = [sum(1 << k for k in range(len(sup)) if corr[k] >> c & 1) for c in range(R)]       # the same tables by column: bit k = segment k
    icol = [sum(1 << k for k in range(len(sup)) if sup[k] >> c & 1) for c in range(R)]
    gsegs = [[(sup[place[j]] if j in place else 0, ln) for j, ln in segs] for segs in model["group_segs"]]
    return dict(R=R, g2=g2, sup=sup, corr=corr, conf=conf, ccol=ccol, icol=icol, rows=list(model["gap_rows"]), gsegs=gsegs,
                lo_f=1.0 - settings["epsilon"], hi_f=1.0 + settings["epsilon"], offset=float(settings["offset"]), max_lg=float(int(model["max_lg"])))


def _bnb_pruned(tb, S, d, best2, weak):
    """A node (columns 0 .. d - 1 fixed, S of them in) is dropped: its lower bound exceeds best2, or a member's row is violated from below."""
    g2, ccol = tb["g2"], tb["ccol"]
    e_in = blocked = 0
    for c in _bits(S):
        e_in |= tb["icol"][c]
        blocked |= tb["conf"][c]
    lb = 0
    for c in range(d):
        lb += 2 * _popc(ccol[c] & e_in) if S >> c & 1 else g2[c]
    if not weak:
        for c in range(d, tb["R"]):
            lb += g2[c] if blocked >> c & 1 else min(g2[c], 2 * _popc(ccol[c] & e_in))
    if lb > best2:
        return True
    for c, g, l in tb["rows"]:
        if S >> c & 1:
            G = sum(ln for m, ln in tb["gsegs"][g] if m & S)
            a = tb["lo_f"] * G
            a = a - tb["offset"]
            if a > float(l) + 1e-9:
                return True
    return False


def _bnb_leaf(tb, S):
    """cost2 of the full column set S, or None when it is not feasible: exact_small()'s test and cost."""
    for c in _bits(S):
        if tb["conf"][c] & S:
            return None
    for c, g, l in tb["rows"]:
        G = float(sum(ln for m, ln in tb["gsegs"][g] if m & S))
        slack = 0.0 if S >> c & 1 else tb["max_lg"]
        a = tb["lo_f"] * G
        a = a - tb["offset"]
        a = a - slack
        b = tb["hi_f"] * G
        b = b + tb["offset"]
        b = b + slack
        if a > float(l) + 1e-9 or b < float(l) - 1e-9:
            return None
    cost2 = sum(tb["g2"][c] for c in range(tb["R"]) if not S >> c & 1)
    for s_mask, c_mask in zip(tb["sup"], tb["corr"]):
        if s_mask & S:
            cost2 += 2 * _popc(c_mask & S)
    return cost2


def bnb_prefix_task(tb, P, L, best2=None, node_cap=BNB_NODE_CAP, weak=False):
    """The task on the prefix (P, L) -- the columns 0 .. L - 1 are fixed and P is the set of them that are in -- of exact_bnb()'s and
    exact_bnb_wide()'s docstrings: (cost2, mask, nodes, capped, open); cost2 -1 and mask 0 when it found no leaf.  best2: where the task's
    best cost starts (None: no bound; a leaf of equal cost is still taken).  open: the open children (prefix, length) of a capped task, by
    ascending level, at the top level the include child first; empty when the task is not capped."""
    R, conf = tb["R"], tb["conf"]
    best2, mask, have, nodes = (_BNB_NONE if best2 is None else best2), 0, False, 1
    S = P

    def leaf(S):
        nonlocal best2, mask, have
        cost2 = _bnb_leaf(tb, S)
        if cost2 is not None and (cost2 < best2 or (cost2 == best2 and (not have or S < mask))):
            best2, mask, have = cost2, S, True

    dead = any(conf[c] & S for c in _bits(S))
    if not dead and L == R:
        leaf(S)
    capped, opened = False, []
    if not dead and L < R and not _bnb_pruned(tb, S, L, best2, weak):
        d, tried_in, tried_out = L, 0, 0                     # the stack: frame d is S's low d bits and two bits of progress
        while True:
            bit = 1 << d
            Sd = S & (bit - 1)
            if tried_out & bit:                              # both children done: pop
                if d == L:
                    break
                d -= 1
                continue
            if not tried_in & bit:
                tried_in |= bit
                if conf[d] & Sd:
                    continue
                child, inc = Sd | bit, True
            else:
                tried_out |= bit
                child, inc = Sd, False
            if nodes >= node_cap:
                capped = True
                if inc:                                      # the child was not evaluated: its progress bit is taken back
                    tried_in &= ~bit
                else:
                    tried_out &= ~bit
                opened = bnb_open_children(conf, S, tried_in, tried_out, L, d)
                break
            nodes += 1
            if d + 1 == R:
                leaf(child)
            elif not _bnb_pruned(tb, child, d + 1, best2, weak):
                S, d = child, d + 1
                tried_in &= ~(1 << d)
                tried_out &= ~(1 << d)
    return (best2 if have else -1), (mask if have else 0), nodes, capped, opened


def bnb_open_children(conf, S, tried_in, tried_out, L, d):
    """The open children of a task on a prefix of length L that was capped at level d, from its frame after the roll-back: the subtrees
    its walk has not entered, as prefixes (set, length)."""
    out = []
    for j in range(L, d + 1):
        Sj = S & ((1 << j) - 1)
        if j == d and not tried_in >> j & 1:
            if not conf[j] & Sj:
                out.append((Sj | 1 << j, j + 1))
            out.append((Sj, j + 1))
        elif not tried_out >> j & 1:
            out.append((Sj, j + 1))
    return out


def bnb_task(tb, t, D, ub2=None, node_cap=BNB_NODE_CAP, weak=False):
    """Task t of a problem's 2^D (exact_bnb()'s docstring): (cost2, mask, nodes, capped); cost2 -1 and mask 0 when it found no leaf.  It
    is bnb_prefix_task() on the prefix (t, D)."""
    return bnb_prefix_task(tb, t, D, ub2, node_cap, weak)[:4]


def exact_bnb(model, settings, ub2=None, depth=BNB_DEPTH, node_cap=BNB_NODE_CAP, weak=False):
    """A depth-first branch and bound over the column sets of one round_model() dict (with ``garbage`` and ``max_lg``) of at most 64
    columns -- the definition the GPU's fclu_round_bnb reproduces exactly, node counts included: dict(status, cost2, cost, mask, members,
    x, e, nodes, capped).  Where it ends "optimal" the (cost2, mask) is exact_small()'s: the smallest cost2, then the smallest mask.

    Tables: bnb_tables(), those of exact_small() as 64-bit masks (bit c = column c): sup[k], corr[k] per informative segment, conf[c], g2[c].
    Node: columns 0 .. d - 1 are fixed and S is the set of those fixed in.  With e_in = the segments whose support meets S and blocked = the
        OR of conf[c] over S,
            LB2 = the g2 of the columns fixed out + 2 * the sum over S of |C_c & e_in|
                  + over the columns c >= d: g2_c when c is blocked, else min(g2_c, 2 * |C_c & e_in|).
        (e only grows, so a member's corrections only grow; a blocked column ends outside S; a free one ends outside, g2_c, or inside with
        at least its corrections on e_in.)  ``weak`` leaves the last line out (profiles only; the device has the full bound).
    Pruned: LB2 > best2 (strict: every set of optimal cost is still reached, so the tie rule holds; best2 starts at ub2 when one is given
        and falls with the task's own leaves), or a row (c, g, l) of a member c of S is violated from below already -- with G = the summed
        lengths of group g's segments whose support meets S, lo_f * G - offset > l + 1e-9 in doubles, one rounded multiply, one rounded
        subtraction and one rounded addition, none fused (G only grows).
    Leaf: a node at depth R; exact_small()'s whole test (pairs, every row, the slack of the columns outside, the tolerance) and its cost2.
        A leaf replaces the task's best when its cost2 is smaller, or equal and the task has none yet or a larger mask.
    Tasks: D = min(R, depth); task t of 2^D fixes columns 0 .. D - 1, bit c of t = column c is in.  A task with a pair inside its prefix
        counts one node and is dead.  Otherwise the prefix counts one node: at D = R it is a leaf; else it is tested by the pruning rules
        and searched depth first over the columns D .. R - 1 with an explicit stack of at most R - D frames.  At column d the include child
        comes first, when conf[d] & S == 0 (else there is none and nothing is counted), then the exclude child.  Before a child is
        evaluated the task's count is compared with node_cap: where it has reached it the task stops and is capped (its best leaf so far
        still counts); else the child counts one node.  Tasks share nothing, so a task depends on (model, ub2, t, node_cap) alone.
    Result: "optimal" -- no task capped and a leaf exists (at cost2 <= ub2 when one is given): the lexicographic minimum of (cost2, mask)
        over the tasks; "infeasible" -- no task capped, no leaf, no ub2; "unproven" -- a task was capped (cost2 and mask the best found,
        or None), or a ub2 was given and no leaf is at or under it.  nodes = the tasks' counts summed, capped = the capped tasks."""
    return _bnb_search(bnb_tables(model, settings), model, ub2, depth, node_cap, weak)


def bnb_pass_bound(ub2, best):
    """The bound every task of a pass starts at: the smaller of ub2 and the best (cost2, mask) of the passes before, either may be None."""
    return ub2 if best is None else best[0] if ub2 is None else min(ub2, best[0])


def bnb_pass(tb, tasks, bound, node_cap, weak=False):
    """One pass of exact_bnb_wide(): the tasks (prefix, length), each started at bound.  dict(best = the smallest (cost2, mask) or None,
    nodes, capped, opened = the capped tasks' open children, stats = the pass's entry of pass_stats)."""
    best, nodes, capped, opened = None, 0, 0, []
    for P, L in tasks:
        cost2, mask, n, cap, children = bnb_prefix_task(tb, P, L, bound, node_cap, weak)
        nodes += n
        capped += cap
        opened += children
        if cost2 >= 0 and (best is None or (cost2, mask) < best):
            best = (cost2, mask)
    return dict(best=best, nodes=nodes, capped=capped, opened=opened,
                stats=dict(tasks=len(tasks), nodes=nodes, capped=capped, min_len=min(L for _, L in tasks), max_len=max(L for _, L in tasks)))


def _bnb_search(tb, model, ub2, depth, node_cap, weak, passes=1, max_tasks=None):
    """exact_bnb()'s body on the tables tb: every task, the passes of exact_bnb_wide(), and the result rule."""
    R = tb["R"]
    if depth < 0 or node_cap < 1:
        raise ValueError("depth %r, node_cap %r: at least 0 and 1" % (depth, node_cap))
    if passes < 1 or (max_tasks is not None and max_tasks < 1):
        raise ValueError("passes %r, max_tasks %r: at least 1" % (passes, max_tasks))
    D = min(R, depth)
    best, nodes, capped, stats = None, 0, 0, []
    tasks = [(t, D) for t in range(1 << D)]
    for k in range(passes):
        one = bnb_pass(tb, tasks, bnb_pass_bound(ub2, best), node_cap, weak)
        nodes, capped = nodes + one["nodes"], one["capped"]
        if one["best"] is not None and (best is None or one["best"] < best):
            best = one["best"]
        stats.append(one["stats"])
        tasks = one["opened"]
        if not tasks or (max_tasks is not None and len(tasks) > max_tasks):
            break
    status = "unproven" if capped or (best is None and ub2 is not None) else "optimal" if best is not None else "infeasible"
    out = dict(status=status, cost2=None, cost=None, mask=None, members=None, x=None, e=None, nodes=nodes, capped=capped)
    if best is not None:
        cost2, mask = best
        x = [mask >> c & 1 for c in range(R)]
        out.update(cost2=cost2, cost=cost2 / 2.0, mask=mask, members=list(_bits(mask)), x=x,
                   e=[int(any(x[c] for c in support)) for support in model["support"]])
    out["pass_stats"] = stats
    return out


def bnb_wide_node_cap(R):
    """The default node_cap of exact_bnb_wide() and Context.round_bnb_wide() at R columns, from profiles/cluster_bnb_wide.txt (DESIGN.md
    section 8).  A task cannot reach a leaf in fewer than R - D nodes and one task of a problem walks nearly all of its nodes, so the cap
    has to grow with R; a lone task's nodes run one after the other, about 2.6 us each at 123 columns, 4.3 at 245 and 6.8 at 490, so the
    cap is also what the longest launch takes.  Up to 64 columns BNB_NODE_CAP, so that the two searches agree; up to 128 columns 4 096,
    which proves every problem of the workload (10 ms); up to 256 columns 8 192, the largest power of two under 50 ms there (35 ms; it
    proves 4 of 80, 16 384 proves 64 and takes 69 ms); beyond 256 columns 4 096 again: nothing was proven at 8 192 or 16 384 nodes, and
    8 192 take 56 ms at 490 columns."""
    return BNB_NODE_CAP if R <= BNB_MAX_COLS else 8192 if 128 < R <= 256 else 4096


def exact_bnb_wide(model, settings, ub2=None, depth=BNB_DEPTH, node_cap=None, passes=1, max_tasks=None):
    """exact_bnb() for a model of at most BNB_WIDE_MAX_COLS = 1024 columns -- the definition the GPU's fclu_round_bnb_wide and
    fclu_round_bnb_wide_passes reproduce exactly, node counts included.  exact_bnb()'s docstring holds word for word (tables, node, bound
    LB2, lower-side row test, leaf, tasks, cap, result rule, node counts); a mask is a Python integer of up to 1024 bits and the smallest
    mask is the smaller integer.  On a model of at most 64 columns and with one pass the two return equal dicts (exact_bnb()'s has the one-pass pass_stats too).
    node_cap None = bnb_wide_node_cap(R).

    Passes: a capped task is not abandoned.  A task is a prefix (P, L): the columns 0 .. L - 1 are fixed, P of them in (bnb_prefix_task();
        exact_bnb()'s task t is the prefix (t, D)).  It is dead on a pair inside P, counting one node; a leaf at L = R; else it is tested by
        the pruning rules, the rows always among them, and searched depth first over the columns L .. R - 1.  Its best starts at the pass's
        bound and a leaf of equal cost is still taken.
    Open children: where a task's count has reached node_cap before a child at level d is evaluated, that child's progress bit is taken
        back.  With Sj = the low j bits of S, the open children are, at the levels j = L .. d - 1, the exclude child (Sj, j + 1) where
        tried_out bit j is clear; at j = d, where tried_in bit d is clear, the include child (Sj | bit j, j + 1) when conf[j] & Sj == 0 and
        the exclude child (Sj, j + 1), and where only tried_out bit d is clear the exclude child alone.  The subtrees of the task's prefix
        are exactly those its walk has finished, those under the open children and the nodes on the stack, which are no leaves.
    Pass 1 is the 2^D tasks, bounded by ub2.  Pass k + 1 is the open children of pass k's capped tasks; each of them starts at B = the
        smaller of ub2 and the best cost2 of every task of the passes before, and at nothing else.  The search ends when no task is open,
        after ``passes`` passes, or when the next pass would hold more than max_tasks tasks (None: no limit): the problem is then not
        continued and stays as it is.  No order among a pass's tasks enters: minima and sums only.
    Result: the lexicographic minimum of (cost2, mask) over all tasks of all passes; nodes = all counts summed; capped = the tasks still
        open at the end, that is the capped tasks of the last pass that ran; the status by exact_bnb()'s rule with those.  pass_stats: a
        dict(tasks, nodes, capped, min_len, max_len) a pass that ran (the prefix lengths' range).
    Why an "optimal" end is exact_small()'s (cost2, mask): pruning is strict (LB2 > best2) and every best2 used is at least the optimal
        cost2 c* (it is ub2, which the result rule only trusts when a leaf is at or under it, or a leaf's cost), so no node above a set of
        cost c* is ever dropped by the bound, and the row test drops only nodes without a feasible leaf.  Every set of cost c* therefore
        lies in a finished subtree or under an open child; with no task open all were reached as leaves, each was taken unless the task
        held an equal-cost smaller mask, and the minimum over the tasks is the smallest cost2, then the smallest mask."""
    tb = bnb_tables(model, settings, BNB_WIDE_MAX_COLS, "exact_bnb_wide")
    return _bnb_search(tb, model, ub2, depth, bnb_wide_node_cap(tb["R"]) if node_cap is None else node_cap, False, passes, max_tasks)


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
