"""Built cases for the first two stages of the clustering library (freddie_amd/csrc/freddie_cluster.hip): the pairwise compatibility
graph (k_compat<RANK>) and its pruning (k_prune_lds; k_prune_edges; k_deg1 + k_prune), at the kernels' own edges, with a vectorised
numpy / scipy model of both that is fast where oracle/cluster_oracle.py (a Python pair loop) is not.

  compat_model(rows, first, last, tail)   py/freddie_cluster.py:219-234 for all pairs at once: "bits of a read in [f, l]" from per-row
                                          prefix sums, `same` from rows @ rows.T (a read's bits lie inside its own [first, last] --
                                          the library's check_rows refuses anything else -- so a & b has no bit outside the overlap)
  prune_model(A) -> (A', passes)          :240-255 with scipy.sparse: (S @ S).multiply(S) counts common neighbours on the edges

Both take a named one-rule MUTATION (the style of tests/scoring_model.py).  A case names the mutations it is there to catch and
tests/test_compat_cases_host.py shows that each changes the case's matrix: the proof that the case's answer turns on that rule.

The cases are tints: (rows bool [N, M], first, last, tail), in the row order the case wants -- fclu_compat_graph does not ask for
unique or sorted rows.  pack() makes the dict cluster_prep.pack_structures() makes.
  R  the rule, pair by pair: overlap start / length / diff / same on a grid around the 32-bit word edges; adjacent and apart spans;
     the nine tail combinations; reads that cover nothing
  W  row widths: 65 rows (two tile rows, one off-diagonal tile and its transpose) at n_seg around 32, 64, kRankWords * 32 and kMaxWords * 32
  P  pruning gadgets made of fully covered reads (an edge iff the spans meet; S and E tails take edges out), each on its own segments, at
     chosen rows of a tint of 130, 1 100, 4 096, 4 097 or 4 161 rows
Tail codes: 0 'N', 1 'S', 2 'E'."""
import functools
from types import SimpleNamespace

import numpy as np

TN, TS, TE = 0, 1, 2

COMPAT_MUTATIONS = ("o_ge_3", "diff_le_3", "short_diff_le_1", "no_same", "no_tail_rule", "tail_N_is_a_category", "mask_f_minus_1",
                    "mask_l_plus_1", "middle_words_skipped")
PRUNE_MUTATIONS = ("deg1_row_end_only", "common_only_below_4096", "neighbours_from_4096_kept", "remainder_batch_kept",
                   "sequential_removal", "no_pass")
CHUNK = 4096           # columns of one 64-word chunk of an adjacency row (k_prune_edges' work item, k_prune's z0 step)
RANK_WORDS = 207       # kRankWords
MAX_WORDS = 300        # kMaxWords
PRUNE_LDS_WORDS = 7808  # kPruneLdsWords


# ---- the model -----------------------------------------------------------------------------------------------------------------
def compat_model(rows, first, last, tail, mutation=None):
    """Boolean N x N compatibility matrix."""
    assert mutation is None or mutation in COMPAT_MUTATIONS, mutation
    rows = np.asarray(rows, bool)
    n, M = rows.shape
    first, last, tail = (np.asarray(x, np.int32) for x in (first, last, tail))
    P = np.zeros((n, M + 1), np.int32)                      # P[i, s] = bits of row i in front of segment s
    np.cumsum(rows, axis=1, out=P[:, 1:])
    f = np.maximum(first[:, None], first[None, :])
    l = np.minimum(last[:, None], last[None, :])
    o = l - f + 1
    ok = (o >= 1) & (f >= 0)                                # (f < 0: neither read covers anything; their slices are empty, :228-230)
    lo = np.clip(f - (1 if mutation == "mask_f_minus_1" else 0), 0, M)
    hi = np.clip(l + 1 + (1 if mutation == "mask_l_plus_1" else 0), 0, M)
    in_a = np.take_along_axis(P, hi, 1) - np.take_along_axis(P, lo, 1)       # bits of row i in the overlap with row j
    in_b = in_a.T                                                            # (f and l are symmetric)
    R = rows.astype(np.float32)
    same = (R @ R.T).astype(np.int32)                       # exact: counts stay below 2^24
    if mutation == "middle_words_skipped":                  # only the overlap's first and last word are summed
        W = (M + 31) // 32
        assert n * n * (W + 1) <= 1 << 26, "middle_words_skipped is for the small tints"
        cum = np.zeros((W + 1, n, n), np.int32)
        for w in range(W):
            Rw = R[:, 32 * w:32 * w + 32]
            cum[w + 1] = cum[w] + (Rw @ Rw.T).astype(np.int32)
        wf, wl = np.clip(f, 0, M - 1) >> 5, np.clip(l, 0, M - 1) >> 5
        ii, jj = np.indices((n, n))
        mid = np.where(wl > wf + 1, cum[wl, ii, jj] - cum[np.minimum(wf + 1, W), ii, jj], 0)
        same = same - mid
    diff = in_a + in_b - 2 * same
    if mutation == "tail_N_is_a_category":
        clash = tail[:, None] != tail[None, :]
    elif mutation == "no_tail_rule":
        clash = np.zeros((n, n), bool)
    else:
        clash = (tail[:, None] != 0) & (tail[None, :] != 0) & (tail[:, None] != tail[None, :])
    long_ok = (o >= 3 if mutation == "o_ge_3" else o > 3) & (diff <= 3 if mutation == "diff_le_3" else diff < 3)
    short_ok = (o < 3 if mutation == "o_ge_3" else o <= 3) & (diff <= 1 if mutation == "short_diff_le_1" else diff == 0)
    edge = ok & ~clash & (long_ok | short_ok)
    if mutation != "no_same":
        edge &= same >= 1
    edge[np.arange(n), np.arange(n)] = False
    return edge


def _one_pass(A, mutation):
    """One pass of :243-252 on a boolean matrix: the matrix behind it."""
    from scipy.sparse import csr_matrix
    n = A.shape[0]
    S = csr_matrix(A.astype(np.int32))
    deg = np.asarray(A.sum(1)).ravel()
    if mutation == "common_only_below_4096":
        common = (S[:, :CHUNK] @ S[:CHUNK, :]).multiply(S)
    else:
        common = (S @ S).multiply(S)
    keep = np.zeros((n, n), bool)
    cr, ccol = common.nonzero()
    keep[cr, ccol] = True
    r, c = np.nonzero(A)
    excused = deg[r] == 1
    if mutation != "deg1_row_end_only":
        excused = excused | (deg[c] == 1)
    keep[r[excused], c[excused]] = True
    if mutation == "neighbours_from_4096_kept":
        keep[:, CHUNK:] = True
    if mutation == "remainder_batch_kept":                   # of a row's neighbours inside one chunk, four at a time: the last count % 4
        for row in np.unique(r):
            nb = c[r == row]
            for q in np.unique(nb // CHUNK):
                part = nb[nb // CHUNK == q]
                if len(part) % 4:
                    keep[row, part[-(len(part) % 4):]] = True
    return A & keep


def _sequential_pass(A):
    """The pass with every removal seen by the edges behind it (the reference collects a pass' edges first, :252)."""
    A = A.copy()
    r, c = np.nonzero(np.triu(A))
    for i, j in zip(r.tolist(), c.tolist()):
        if A[i].sum() == 1 or A[j].sum() == 1 or (A[i] & A[j]).any():
            continue
        A[i, j] = A[j, i] = False
    return A


def prune_model(A, mutation=None):
    """(the matrix at the pruning's fixed point, the passes that removed something)."""
    assert mutation is None or mutation in PRUNE_MUTATIONS, mutation
    A = np.asarray(A, bool)
    if mutation == "no_pass":
        return A.copy(), 0
    passes = 0
    while passes < 16:
        B = _sequential_pass(A) if mutation == "sequential_removal" else _one_pass(A, mutation)
        if np.array_equal(A, B):
            break
        A = B
        passes += 1
    return A, passes


# ---- tints and batches ---------------------------------------------------------------------------------------------------------
def make_tint(name, group, n_seg, reads, mutations=(), **meta):
    """reads: [(first, last, tail, covered segments)] in row order."""
    n = len(reads)
    rows = np.zeros((n, n_seg), bool)
    for i, (_, _, _, cov) in enumerate(reads):
        if len(cov):
            rows[i, np.asarray(cov, np.int64)] = True
    return SimpleNamespace(name=name, group=group, n=n, n_seg=n_seg, words=max((n_seg + 31) // 32, 1), rows=rows, first=np.array([r[0] for r in reads], np.int32),
                           last=np.array([r[1] for r in reads], np.int32), tail=np.array([r[2] for r in reads], np.uint8),
                           mutations=tuple(mutations), **meta)


def pack(tints):
    """The dict of cluster_prep.pack_structures() for a list of tints."""
    T = len(tints)
    row_off = np.zeros(T + 1, np.int64); bits_off = np.zeros(T + 1, np.int64); adj_off = np.zeros(T + 1, np.int64)
    bits = []
    for t, x in enumerate(tints):
        W = max((x.n_seg + 31) // 32, 1)
        row_off[t + 1] = row_off[t] + x.n
        bits_off[t + 1] = bits_off[t] + x.n * W
        adj_off[t + 1] = adj_off[t] + x.n * ((x.n + 63) // 64)
        padded = np.zeros((x.n, W * 32), np.uint8)
        padded[:, :x.n_seg] = x.rows
        bits.append(np.packbits(padded, axis=1, bitorder="little").view(np.uint32).reshape(-1))
    return dict(n_tint=T, row_off=row_off, n_seg=np.array([x.n_seg for x in tints], np.int32), bits_off=bits_off, bits=np.concatenate(bits),
                first=np.concatenate([x.first for x in tints]), last=np.concatenate([x.last for x in tints]),
                tail=np.concatenate([x.tail for x in tints]), adj_off=adj_off)


def structures(x):
    """The tint as cluster_oracle.compat_edges() takes it: [((row tuple, (first, last, tail letter)), [row index])]."""
    return [((tuple(int(v) for v in x.rows[i]), (int(x.first[i]), int(x.last[i]), "NSE"[x.tail[i]])), [i]) for i in range(x.n)]


# ---- group R: the rule, pair by pair ---------------------------------------------------------------------------------------------
R_SEG = 200
R_STARTS = (0, 1, 30, 31, 32, 33, 62, 63, 64, 95, 96)
R_LENGTHS = (1, 2, 3, 4, 5, 31, 32, 33, 64, 65, 97)
R_DIFFS = (0, 1, 2, 3, 4)
R_SAME = ("none", "one", "many")
R_TINTS = 8
R_RULE_MUTATIONS = ("o_ge_3", "diff_le_3", "short_diff_le_1", "no_same", "mask_f_minus_1", "mask_l_plus_1", "middle_words_skipped")


def rule_pair(f, o, diff, same, turn=0):
    """Two reads whose overlap is [f, f + o - 1]: a reaches three segments to its left (and covers them: bits just outside the
    overlap, in its first word unless f is a word's first bit), b three to its right.  `diff` positions of the overlap are covered by
    exactly one of them: taken, from position `turn` on, from the overlap's two ends and the two sides of every word edge inside it.
    same: both cover every other position / one of them / none.  None when the overlap has no room for that."""
    l = f + o - 1
    edges = [p for k in range(f // 32 + 1, l // 32 + 1) for p in (32 * k - 1, 32 * k) if f <= p <= l]
    cand = list(dict.fromkeys([f, l] + edges))
    cand = cand[turn % len(cand):] + cand[:turn % len(cand)]
    cand += [p for p in range(f, l + 1) if p not in cand]
    if diff > o or (same == "one" and o - diff < 1):
        return None
    differing = cand[:diff]
    rest = [p for p in range(f, l + 1) if p not in differing]
    both = rest if same == "many" else rest[len(rest) // 2:len(rest) // 2 + 1] if same == "one" else []
    a_cov = list(range(max(f - 3, 0), f)) + both
    b_cov = list(range(l + 1, l + 4)) + both
    for k, p in enumerate(sorted(differing)):
        # (the overlap's first position stays with b, whose first segment it is, and its last with a)
        (b_cov if p == f or (p != l and k % 2) else a_cov).append(p)
    return (max(f - 3, 0), l, TN, sorted(a_cov)), (f, l + 3, TN, sorted(b_cov))


def rule_grid():
    """[(f, o, diff, same, a, b)] over the whole grid."""
    out = []
    for f in R_STARTS:
        for o in R_LENGTHS:
            for diff in R_DIFFS:
                for same in R_SAME:
                    pair = rule_pair(f, o, diff, same, turn=len(out))
                    if pair is not None:
                        out.append((f, o, diff, same) + pair)
    return out


def special_tint():
    """Adjacent spans and spans apart; the nine tail combinations on a pair the rule accepts and on one it refuses; reads that cover
    nothing, as find_segment_read() writes them: (first, last) = (-1, M - 1)."""
    M = R_SEG
    reads, what = [], {}
    full = lambda a, b: list(range(a, b + 1))
    what["adjacent"] = (len(reads), len(reads) + 1); reads += [(10, 40, TN, full(10, 40)), (41, 70, TN, full(41, 70))]
    what["apart"] = (len(reads), len(reads) + 1); reads += [(80, 95, TN, full(80, 95)), (97, 120, TN, full(97, 120))]
    what["tails"] = []
    for accept in (True, False):
        for ta in (TN, TS, TE):
            for tb in (TN, TS, TE):
                # (preprocess_ilp puts an S read's first at 0 and an E read's last at M - 1, :293-300; the rule compares the letters only)
                s = 128 + 2 * len(what["tails"])
                a = (s - 8, s + 6, ta, full(s - 8, s + 6))
                hole = [] if accept else [s + 1, s + 2, s + 3]
                b = (s, s + 12, tb, [p for p in full(s, s + 12) if p not in hole])
                what["tails"].append((len(reads), len(reads) + 1, ta, tb, accept))
                reads += [a, b]
    what["empty"] = (len(reads), len(reads) + 1, len(reads) + 2)
    reads += [(-1, M - 1, TN, []), (-1, M - 1, TS, []), (0, M - 1, TN, full(0, M - 1))]
    return make_tint("R-special", "R", M, reads, ("no_tail_rule", "tail_N_is_a_category"), what=what)


@functools.lru_cache(maxsize=None)
def group_r():
    grid = rule_grid()
    tints = []
    for t in range(R_TINTS):
        mine = grid[t::R_TINTS]
        reads = [r for g in mine for r in g[4:]]
        tints.append(make_tint("R-grid-%d" % t, "R", R_SEG, reads, R_RULE_MUTATIONS, grid=[g[:4] for g in mine]))
    return tints + [special_tint()]


# ---- group W: row widths -------------------------------------------------------------------------------------------------------------
W_SEGS = (1, 31, 32, 33, 64, 65, 6623, 6624, 6625, 9599, 9600)
W_ROWS = 65


def width_tint(M):
    """65 rows of M segments: a fully covered row; reads inside the first and inside the last word; fully covered rows with one, two and
    three holes in the first, a middle and the last word, as far as the word has the positions (diff 1, 2, 3 against the full row over
    every word); the rest seeded
    sub-ranges of a few patterns.  Row 64 -- the second tile row -- is a fully covered row with one hole in the last word."""
    rng = np.random.default_rng(7000 + M)
    W = (M + 31) // 32
    full = list(range(M))
    reads = [(0, M - 1, TN, full)]
    lw0 = 32 * (W - 1)
    reads.append((lw0, M - 1, TN, list(range(lw0, M))))                       # overlap with the full row: the last word only
    reads.append((0, min(31, M - 1), TN, list(range(0, min(32, M)))))          # the first word only
    holes = []
    for w in sorted({0, W // 2, W - 1}):
        inside = [p for p in range(32 * w, min(32 * w + 32, M)) if p > 0]
        picks = list(dict.fromkeys([inside[0], inside[len(inside) // 2], inside[-1]])) if inside else []
        for k in (1, 2, 3):
            if k <= len(picks):
                holes.append((w, tuple(picks[:k])))
                reads.append((0, M - 1, TN, [p for p in full if p not in picks[:k]]))
    pats = rng.random((4, M)) < 0.6
    while len(reads) < W_ROWS - 1:
        a = int(rng.integers(0, M)); b = int(rng.integers(a, M))
        row = np.zeros(M, bool)
        row[a:b + 1] = pats[rng.integers(0, 4), a:b + 1] ^ (rng.random(b - a + 1) < 0.02)
        cov = np.flatnonzero(row)
        reads.append((int(cov[0]), int(cov[-1]), int(rng.integers(0, 3)) if rng.random() < 0.2 else TN, cov.tolist()) if len(cov)
                     else (-1, M - 1, TN, []))
    last_hole = M - 2 if M >= 3 else None
    reads.append((0, M - 1, TN, [p for p in full if p != last_hole]))
    muts = (("diff_le_3",) if holes else ()) + (("middle_words_skipped",) if W >= 3 else ())
    return make_tint("W-%d" % M, "W", M, reads, muts, holes=holes)


@functools.lru_cache(maxsize=None)
def group_w():
    return [width_tint(M) for M in W_SEGS]


# ---- group P: pruning gadgets ----------------------------------------------------------------------------------------------------------
# A gadget: (width in segments, [(lo, hi, tail)] fully covered reads on segments lo .. hi of the gadget's own range).
def g_path(n):
    return 2 * n + 1, [(2 * i, 2 * i + 2, TN) for i in range(n)]


def g_star(m):
    """node 0 the hub, then m leaves"""
    return m, [(0, m - 1, TN)] + [(i, i, TN) for i in range(m)]


def g_clique(n):
    return 2 * n - 1, [(i, n - 1 + i, TN) for i in range(n)]


def g_k2m(m):
    """Two hubs over the same span, one with an S tail and one with an E tail (no edge between them), and m leaves without a tail under
    both: no triangle, every degree at least 2."""
    return m, [(0, m - 1, TS), (0, m - 1, TE)] + [(i, i, TN) for i in range(m)]


def g_triangle_pendant():
    """node 0 the pendant of node 1; 1, 2, 3 the triangle"""
    return 6, [(0, 1, TN), (0, 3, TN), (2, 4, TN), (3, 5, TN)]


def g_hub(d, paired=False):
    """node 0: a hub of degree d; node 1: its one removable neighbour x (x's other neighbour, node 2, does not touch the hub); nodes
    3 ..: d - 1 neighbours that stay -- leaves (degree 1), or with `paired` two to a segment (a triangle with the hub)."""
    leaves = [((i // 2) * 2 if paired and (i // 2) * 2 + 1 < d - 1 else i) for i in range(d - 1)]
    return d + 1, [(0, d - 1, TN), (d - 1, d, TN), (d, d, TN)] + [(s, s, TN) for s in leaves]


HUB_DEGREES = (1, 2, 3, 4, 5, 8, 9)


class _Placer:
    """Rows of a tint handed out to gadgets; take() reserves what it returns."""

    def __init__(self, n):
        self.n, self.items, self.taken, self.info = n, [], set(), []

    def take(self, count=1, lo=0, hi=None, step=1, base=0):
        """`count` free rows of base .. hi - 1, ascending: the first free ones at or after lo (modulo hi), `step` apart; what finds no
        room before hi is the first free rows from base on."""
        hi = self.n if hi is None else hi
        out, r = [], max(lo % hi, base)
        while len(out) < count and r < hi:
            if r in self.taken:
                r += 1
            else:
                out.append(r); self.taken.add(r); r += step
        rest = [v for v in range(base, hi) if v not in self.taken][:count - len(out)]
        assert len(out) + len(rest) == count, "no room in rows %d .. %d" % (base, hi)
        self.taken |= set(rest)
        return sorted(out + rest)

    def put(self, kind, gadget, rows, **meta):
        width, nodes = gadget
        assert len(rows) == len(nodes) and len(set(rows)) == len(rows) and set(rows) <= self.taken, (kind, rows)
        self.items.append((width, nodes, rows))
        self.info.append(dict(kind=kind, rows=list(rows), **meta))

    def tint(self, name, mutations):
        seg, reads = 0, [None] * self.n
        for width, nodes, rows in self.items:
            for (lo, hi, tail), r in zip(nodes, rows):
                assert reads[r] is None
                reads[r] = (seg + lo, seg + hi, tail, list(range(seg + lo, seg + hi + 1)))
            seg += width
        for r in range(self.n):                               # the rest: isolated reads, a segment each
            if reads[r] is None:
                reads[r] = (seg, seg, TN, [seg]); seg += 1
        return make_tint(name, "P", seg, reads, mutations, gadgets=self.info)


TOP_ROWS = 12          # the last rows below CHUNK, kept for the nodes that want a high row in a tint that has too few


def prune_tint(n, removing=True):
    """The gadgets at chosen rows of a tint of n rows.  The rows from CHUNK on are `high` (the tint's last rows when it has none that
    far: the same gadgets, inside one chunk).  removing=False: stars and cliques only -- a tint no pass removes anything from."""
    pl = _Placer(n)
    below = min(n, CHUNK)
    high = iter(pl.take(min(n - CHUNK, 16), lo=CHUNK, base=CHUNK) if n > CHUNK else [])
    top = iter(pl.take(TOP_ROWS, lo=below - TOP_ROWS, hi=below, base=below - TOP_ROWS))

    def hi_row():                                             # a row from CHUNK on while there are any, else one of the last below it
        r = next(high, None)
        return next(top) if r is None else r

    low = lambda count=1, **kw: pl.take(count, hi=below - TOP_ROWS, **kw)
    if not removing:
        for m in (1, 2, 5, 9):
            pl.put("star", g_star(m), low(m + 1, lo=3), expect="kept")
        for k in (3, 4, 7):
            pl.put("clique", g_clique(k), low(k, lo=70, step=5), expect="kept")
        pl.put("clique", g_clique(3), low(2, lo=500) + [hi_row()], expect="kept")
        return pl.tint("P-still-%d" % n, ())
    # --- across the chunk edge (the first one has the first high row: the only one of a tint of CHUNK + 1 rows)
    r, c = low(2, lo=5, step=70)
    pl.put("q2_triangle", g_clique(3), [r, c, hi_row()], expect="kept")                   # (r, c): common neighbour at a high row only
    pl.put("high_c_low_common", g_clique(3), low(2, lo=11, step=130) + [hi_row()], expect="kept")      # nodes r, k, c
    pl.put("high_c_high_common", g_clique(3), low(1, lo=17) + [hi_row(), hi_row()], expect="kept")      # r's neighbours: high rows only
    pl.put("high_c_leaf", g_star(2), low(2, lo=23, step=64) + [hi_row()], expect="kept")
    p1, r, p2 = low(3, lo=29, step=200)
    pl.put("high_c_removed", g_path(4), [p1, r, hi_row(), p2], expect="interior")          # c = node 2: its neighbours are low rows only
    pl.put("star_high_leaves", g_star(3), low(1, lo=37) + [hi_row(), hi_row(), hi_row()], expect="kept")
    nb = low(7, lo=41, step=max(below // 8, 1)) + [hi_row(), hi_row()]                     # a hub of degree 9 over many words, x last
    pl.put("hub", g_hub(9), low(1, lo=43) + [nb[-1]] + low(1, lo=47) + nb[:-1], degree=9, x="last", placement="across", paired=False,
           expect="x")
    # --- the plain gadgets
    for k in (2, 3, 4, 5, 6):
        pl.put("path", g_path(k), low(k, lo=50 + 3 * k, step=1 if k % 2 else 67), expect="interior")
    pl.put("star", g_star(5), low(6, lo=90), expect="kept")
    pl.put("star_hub_last", g_star(4), list(reversed(low(5, lo=100, step=3))), expect="kept")
    pl.put("clique", g_clique(5), low(5, lo=110, step=2), expect="kept")
    pl.put("k2m", g_k2m(3), low(5, lo=60), expect="none")
    pl.put("triangle_pendant", g_triangle_pendant(), low(4, lo=64), expect="kept")
    # --- hub rows: degree 1 .. 9, one removable neighbour, first or last among the row's neighbours, in one word or over several
    big = n >= 1000
    k = 0
    for placement in (("spread", "word") if big else ("spread",)):
        for x_at in (("first", "last") if big else ("alternate",)):
            for d in HUB_DEGREES:
                where = x_at if x_at != "alternate" else ("first", "last")[k % 2]
                paired = big and d in (5, 9) and placement == "word"
                if placement == "word":
                    word = 2 + k % 14
                    nb = pl.take(d, lo=64 * word, hi=64 * word + 64, base=64 * word)
                else:
                    nb = low(d, lo=7 + 3 * k, step=max((below - 60) // 10, 1))
                x = nb[0] if where == "first" else nb[-1]
                hub, y = low(1, lo=128 % n)[0], low(1, lo=(300 + 7 * k) % (n - 40))[0]
                pl.put("hub", g_hub(d, paired), [hub, x, y] + [v for v in nb if v != x], degree=d, x=where, placement=placement,
                       paired=paired, expect="x" if d > 1 else "kept")
                k += 1
    muts = ["deg1_row_end_only", "remainder_batch_kept", "sequential_removal", "no_pass"]
    if n > CHUNK:
        muts.append("common_only_below_4096")
    if n - CHUNK >= 8:
        muts.append("neighbours_from_4096_kept")
    return pl.tint("P-%d" % n, muts)


P_SIZES = (130, 1100, 4096, 4097, 4161)


@functools.lru_cache(maxsize=None)
def group_p():
    return [prune_tint(n) for n in P_SIZES] + [prune_tint(4161, removing=False)]


# ---- names, models, batches ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _by_name():
    return {x.name: x for x in group_r() + group_w() + group_p()}


def all_tints():
    return list(_by_name().values())


def tint(name):
    return _by_name()[name]


@functools.lru_cache(maxsize=None)
def model_of(name):
    """(raw matrix, pruned matrix, passes) of a tint by the model; computed once."""
    x = tint(name)
    raw = compat_model(x.rows, x.first, x.last, x.tail)
    pruned, passes = prune_model(raw)
    return raw, pruned, passes


def batches():
    """{batch name: [tint names]}: what the device tests run, each as one call."""
    b = {"R": [x.name for x in group_r()]}
    for M in W_SEGS:
        b["W-%d" % M] = ["W-%d" % M]
    b["W-6624+6625"] = ["W-6624", "W-6625"]                                  # one batch: the masked form takes both
    for n in (4096, 4097, 4161):
        b["P-%d" % n] = ["P-%d" % n]
    b["P-small"] = ["P-130"]
    b["P-mid"] = ["P-1100"]
    b["P-mixed"] = ["P-130", "P-4161", "P-1100"]                             # n_chunks < max_chunks; an in_lds tint beside large ones
    b["P-still+removing"] = ["P-still-4161", "P-1100"]                       # pass states 0 and 1 in one batch
    b["P-still"] = ["P-still-4161"]
    b["P-still+small"] = ["P-still-4161", "P-130"]                           # one pass that removes nothing: the answer is the matrix' second
                                                                             # copy, where k_prune_lds must have left the small tint's too
    return b
