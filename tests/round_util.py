"""Yardsticks of the round models (fclu_round_models) and of the solver: a plain restatement of the arrays from a tint dict -- lists
and sets, nothing like the kernels -- and a brute-force solver that enumerates the subsets of the remaining reps and evaluates each
from the reference's definitions (py/freddie_cluster.py:347-572, K = 2), with no matrix and no solver."""
import random


def informative_segs(tint, remaining):
    """:331-344 restated: segment j (1 <= j <= M - 2) is dropped when the columns j - 1, j, j + 1 hold one value each, the same one."""
    M = len(tint["segs"])
    I = tint["ilp_data"]["I"]
    content = [set(I[i][j] for i in remaining) for j in range(M)]
    out = [True] * M
    for j in range(1, M - 1):
        if len(content[j]) == 1 and content[j - 1] == content[j] == content[j + 1]:
            out[j] = False
    return out


def rep_gaps(tint, i):
    return list(tint["reads"][tint["read_reps"][i][0]]["gaps"].items())


def restate(tint, incomp, remaining):
    """The model arrays of one problem in the shape of cluster_prep.round_model(); refused: None, or the smallest offending column."""
    M = len(tint["segs"])
    I, C = tint["ilp_data"]["I"], tint["ilp_data"]["C"]
    remaining = list(remaining)
    inf = informative_segs(tint, remaining)
    inf_seg = [j for j in range(M) if inf[j]]
    col = {rid: c for c, rid in enumerate(remaining)}
    keys = sorted(set(k for i in remaining for k, _ in rep_gaps(tint, i)))
    bad = [c for c, i in enumerate(remaining) for (j1, j2), _ in rep_gaps(tint, i) if not (inf[j1 % M] and inf[j2 % M])]
    words = [0] * max((M + 31) // 32, 1)
    for j in inf_seg:
        words[j // 32] |= 1 << (j % 32)
    return dict(
        refused=min(bad) if bad else None, n_cols=len(remaining), words=words, inf_seg=inf_seg,
        support=[[c for c, i in enumerate(remaining) if I[i][j] == 1] for j in inf_seg],
        corrections=[[j for j in inf_seg if C[i][j] == 1] for i in remaining],
        pairs=[(col[a], col[b]) for a, b in incomp if a in col and b in col],
        groups=keys,
        group_segs=[[(j, tint["segs"][j][2]) for j in range(j1 + 1, j2) if inf[j]] for j1, j2 in keys],
        gap_rows=[(c, keys.index(k), l) for c, i in enumerate(remaining) for k, l in rep_gaps(tint, i)])


def garbage_costs(tint, remaining, recycle_model):
    """Per remaining rep, what the reference's three garbage-cost formulas mean (:186-194, :314-322) for rows held as lists."""
    I, C = tint["ilp_data"]["I"], tint["ilp_data"]["C"]
    out = []
    for i in remaining:
        n = len(tint["read_reps"][i])
        if recycle_model == "constant":
            out.append(n * 3)
        elif recycle_model == "exons":
            out.append(n * max(sum(I[i]) - 0.5, 1))
        elif recycle_model == "introns":
            out.append(n * max(sum(C[i]) - 0.5, 1))
        else:
            raise ValueError(recycle_model)
    return out


def subset_cost(tint, incomp, remaining, chosen, settings):
    """Cost of putting exactly the columns `chosen` (a set) into the round's isoform, or None when that is infeasible.  E = the OR of
    the chosen reps' rows on informative segments (E2I_C1: the max over the isoform's reads, :440-445); every chosen rep pays one per
    informative segment with C = 1 and E = 1 (:522-535); every other rep pays its garbage cost (:544)."""
    M = len(tint["segs"])
    I, C = tint["ilp_data"]["I"], tint["ilp_data"]["C"]
    remaining = list(remaining)
    inf = informative_segs(tint, remaining)
    chosen_rids = [remaining[c] for c in sorted(chosen)]
    inside = set(chosen_rids)
    if any(a in inside and b in inside for a, b in incomp):
        return None
    E = [1 if inf[j] and any(I[i][j] == 1 for i in chosen_rids) else 0 for j in range(M)]
    eps, off = settings["epsilon"], settings["offset"]
    max_lg = sum(s[2] for s in tint["segs"])
    for i in remaining:                                      # (:482-497: a rep outside the isoform gets MAX_ISOFORM_LG of slack, no more)
        slack = 0 if i in inside else max_lg
        for (j1, j2), l in rep_gaps(tint, i):
            L = sum(tint["segs"][j][2] for j in range(j1 + 1, j2) if E[j])
            if (1.0 - eps) * L - off - slack > l + 1e-9 or (1.0 + eps) * L + off + slack < l - 1e-9:
                return None
    garbage = garbage_costs(tint, remaining, settings["recycle_model"])
    cost = sum(g for c, g in enumerate(garbage) if c not in chosen)
    cost += sum(1 for i in chosen_rids for j in range(M) if inf[j] and C[i][j] == 1 and E[j])
    return cost


def brute_force(tint, incomp, remaining, settings):
    """(optimal cost, one optimal subset of columns) over all 2^R subsets, R <= 12; None when no subset is feasible (a gap longer than
    offset + MAX_ISOFORM_LG makes the reference's model infeasible whatever the rep is assigned to)."""
    R = len(remaining)
    assert R <= 12
    best = None
    for mask in range(1 << R):
        chosen = set(c for c in range(R) if mask >> c & 1)
        cost = subset_cost(tint, incomp, remaining, chosen, settings)
        if cost is not None and (best is None or cost < best[0]):
            best = (cost, chosen)
    return best


# ---- crafted tints in read_segment()'s shape ---------------------------------------------------------------------------------
def make_tint(tid, rows, gaps=None, polys=None, seg_lens=None, members=None):
    """rows: label lists (0 / 1 / 2), one a rep; gaps: {rep: {(j1, j2): l}}; polys: {rep: {key: (length, gap)}}; members: reads a rep."""
    M = len(rows[0])
    seg_lens = seg_lens or [10 + 3 * (j % 7) for j in range(M)]
    pos = [100]
    for l in seg_lens:
        pos.append(pos[-1] + l)
    reads, read_reps = [], []
    for i, row in enumerate(rows):
        read_reps.append([])
        for _ in range((members or {}).get(i, 1)):
            read_reps[-1].append(len(reads))
            reads.append(dict(id=len(reads), name="r%d_%d" % (tid, len(reads)), chr="chr1", strand="+", tint=tid, data=list(row),
                              gaps=dict((gaps or {}).get(i, {})), softclip={}, poly_tail=dict((polys or {}).get(i, {}))))
    return dict(id=tid, chr="chr1", segs=[(s, e, e - s) for s, e in zip(pos[:-1], pos[1:])], reads=reads, read_reps=read_reps)


def random_rows(rng, n, M, n_patterns=3, flip=0.05, two=0.3, const_runs=True):
    """Noisy copies of a few patterns with constant stretches (uninformative runs) and 0 -> 2 swaps (C differs where I does not)."""
    pats = []
    for _ in range(n_patterns):
        p = [1 if rng.random() < 0.6 else 0 for _ in range(M)]
        pats.append(p)
    if const_runs and M >= 6:
        a = rng.randrange(M - 4); b = min(M, a + rng.randrange(3, max(4, M // 2)))
        v = rng.randrange(2)
        for p in pats:
            p[a:b] = [v] * (b - a)
    rows = []
    for _ in range(n):
        p = pats[rng.randrange(n_patterns)]
        row = [(1 - v) if rng.random() < flip and not const_runs else v for v in p]
        lo, hi = sorted((rng.randrange(M), rng.randrange(M)))
        if rng.random() < 0.5:
            row = [v if lo <= j <= hi else 0 for j, v in enumerate(row)]
        rows.append([2 if v == 0 and rng.random() < two else v for v in row])
    return rows


def random_gaps(rng, rows, p=0.4, tails=True):
    """Internal gaps between covered segments and poly tails, as read_segment() accepts them (0 <= j1 < j2 < M)."""
    M = len(rows[0])
    gaps, polys = {}, {}
    for i, row in enumerate(rows):
        ones = [j for j, v in enumerate(row) if v == 1]
        g = {}
        for _ in range(rng.randrange(0, 4) if rng.random() < p else 0):
            if len(ones) >= 2:
                a, b = sorted(rng.sample(ones, 2))
                g[(a, b)] = rng.randrange(0, 200)
        if g:
            gaps[i] = g
        if tails and rng.random() < 0.3:
            polys[i] = {rng.choice(["SA", "ST", "EA", "ET"]): (rng.randrange(5, 40), rng.randrange(0, 100))}
    return gaps, polys
