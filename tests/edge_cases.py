"""Hand-built partitions for the kernels around the scoring stage -- k_smooth, k_peaks_edges, k_fix, k_segments, k_refine,
k_label_cols, k_label_reads -- at the sizes where their code takes another branch.  Built on util.hand() / util.junction_reads() /
util.flat_top(): counts are placed position by position, so a case says which tile, block, word or chunk edge it sits on.
tests/test_edge_cases_host.py runs every case through the CPU oracle and asserts that it reaches the edge it is named after;
tests/test_gpu_front_edges.py and tests/test_gpu_tail_edges.py run the same cases on the device.

A case is (partitions, params); a case's oracles are computed once (oracles()) and shared by every test."""
import functools

import numpy as np

import util

TILE = 512             # kSmoothTile (csrc/seg_common.h)
REF_CAP = 1024         # kRefCap
LABEL_STAGE = 1024     # kLabelStage
S0 = 1000              # genomic start of the interval under test

SIGMAS = {"sigma5": 5.0, "sigma3": 3.0, "sigma2.5": 2.5, "sigma0.1": 0.1}
RADIUS = {"sigma5": 20, "sigma3": 12, "sigma2.5": 10, "sigma0.1": 0}      # int(4 * sigma + 0.5)
SMOOTH_R = {"sigma5": 20, "sigma3": 12, "sigma2.5": 0, "sigma0.1": 0}     # the k_smooth instance (census word smooth_r)
PLATEAU_SIGMAS = ("sigma5", "sigma3", "sigma2.5")


def single(length, positions, weights, odd_first=False):
    """[interval of `length` positions, sink] with the counts given, optionally behind an interval of 37 positions (the tiles of the
    interval under test then start at an odd bit of the flag words and share their first and last word)."""
    iv = (S0, S0 + length - 1)
    sink = (iv[1] + 200, iv[1] + 299)
    reads, w = util.junction_reads(iv, positions, weights, sink)
    ivs = ([(S0 - 100, S0 - 64)] if odd_first else []) + [iv, sink]
    return util.hand(ivs, reads, w)


# ---- plateaus (k_smooth's tiles, tile_defer, k_peaks_edges) -------------------------------------------------------------------
# name -> (first position, length) of the plateau, in an interval of PLATEAU_LEN positions (tiles start at 0, 512, 1024, ...)
PLATEAU_LEN = 2300
PLATEAUS = {
    "inside-tile": (100, 7), "cross-511-512": (509, 6), "start-511": (511, 5), "start-512": (512, 5), "start-tile-0": (1024, 4),
    "end-511": (505, 7), "longer-than-512": (300, 600), "longer-than-1024": (300, 1300), "to-last-position": (2200, 100),
}


def plateau_part(name, r, odd_first=False):
    p, n = PLATEAUS[name]
    pos, w = util.flat_top(p - r, n + 2 * r)
    if name == "to-last-position":
        pos = [q for q in pos if q < PLATEAU_LEN]          # (the reflection at the interval's end keeps the signal level)
        w = w[:len(pos)]
    return single(PLATEAU_LEN, pos, w, odd_first)


def twin_part(sigma, odd_first=False):
    """Two-position plateaus three positions apart, so that one thread's four positions hold two plateau starts (mid0 and mid1 of
    k_smooth).  Counts that are symmetric about the middle of a pair of positions give that pair bit-identical smoothed values
    whatever the filter (the taps' pair sums are the same numbers); with period 3 every such pair is a plateau of its own.  Under
    sigma 3 and 2.5 the pairs that hold the counts (w w 0 w w 0 ...) are the maxima; under sigma 5 the filter, cut off at four sigma,
    passes that period with the opposite sign, and the empty pairs of 0 0 w 0 0 w ... are.  Radius 0 (sigma 0.1): the counts
    themselves, plateaus of two and of three positions."""
    pos, w = [], []
    if sigma == "sigma0.1":
        for q in range(60, 460, 7):
            pos += [q, q + 1, q + 3, q + 4, q + 5]; w += [5] * 5
    elif sigma == "sigma5":
        pos = list(range(62, 460, 3)); w = [40] * len(pos)
    else:
        for q in range(60, 460, 3):
            pos += [q, q + 1]; w += [40, 40]
    return single(PLATEAU_LEN, pos, w, odd_first)


def plateau_midpoint(name):
    p, n = PLATEAUS[name]
    return (p + p + n - 1) // 2


def plateau_case(sigma, odd_first):
    r = RADIUS[sigma]
    names = list(PLATEAUS) + ["twins"]
    parts = [plateau_part(n, r, odd_first) for n in PLATEAUS] + [twin_part(sigma, odd_first)]
    return names, parts, dict(sigma=SIGMAS[sigma])


def twins_in_one_quad(o, k):
    """Quads (four positions from a multiple of four: one thread of k_smooth) of interval k that hold two plateau starts, with the
    plateaus' midpoints."""
    quads = {}
    for i, m in plateau_starts(o["Y"][o["pos_off"][k]:o["pos_off"][k + 1]]):
        quads.setdefault(i // 4, []).append(m)
    return [v for v in quads.values() if len(v) >= 2]


def plateau_starts(y):
    """Positions i of a signal where a plateau that counts as a peak starts (rise, level, ..., fall), with its midpoint."""
    out = []
    n = len(y)
    for i in range(1, n - 1):
        if y[i - 1] < y[i] and y[i + 1] == y[i]:
            ia = i + 1
            while ia < n - 1 and y[ia] == y[i]:
                ia += 1
            if y[ia] < y[i]:
                out.append((i, (i + ia - 1) // 2))
    return out


# ---- interval lengths around the radius, the quad and the tile (reflect_index, a partial last quad, load_counts' fast branch) ----
def short_lengths(r):
    """(An interval of one position is refused on upload, as the reference's read_split asserts start < end: one_position_case().)"""
    return [2, 3, 4, 5, r - 1, r, r + 1, 511, 512, 513, 1023, 1025]


def one_position_case():
    iv, sink = (S0, S0), (S0 + 200, S0 + 299)
    return ["len-1"], [util.hand([iv, sink], [[(sink[0] + 5, sink[0] + 50), (sink[0] + 60, sink[1])]])], {}


def length_case(sigma):
    r = RADIUS[sigma]
    names, parts = [], []
    for L in short_lengths(r):
        # (an exon needs start < end, so no first exon ends on position 0: the ends are counted here, and every rep's start is position 0)
        pos = sorted({q for q in (1, L - 2, L - 1) if 0 < q < L})
        names.append("len-%d" % L)
        parts.append(single(L, pos, [7 + 2 * i for i in range(len(pos))]))
    return names, parts, dict(sigma=SIGMAS[sigma], ignore_ends=False)


# ---- k_fix / k_segments: candidates per interval against the block size ------------------------------------------------------
STEP = 45              # light junctions (weight 3) every STEP positions: each a candidate of its own under sigma 5
COUNTS = [63, 64, 65, 255, 256, 257, 300, 1100]
WIDTH_LEN = {64: 0, 256: 20000, 1024: 70000}            # interval length at least this -> iv_threads (<= 16 384: 64, <= 65 536: 256)
WIDTH_MPS = (1000, 5, 50, 100)
WIDTH_PARAMS = dict(min_read_support_outside=1000, variance_factor=1.0)


def heavy_ranks(n, layout):
    """Ranks (= candidate indices: candidate 0 is the interval's first position) of the heavy junctions among n candidates.
    "a": gaps of 1, 63, 64, 65, 130 and 257 candidates between consecutive ones as far as n allows, the rest every 40.
    "b": 7, 60 and 200 (then every 40) -- candidates 64 .. 191, two whole 64-candidate chunks, hold none, and the first oversized gap under
    max_problem_size 5, (0, 7), puts its anchor on candidate 4: the window 4 - 5 .. 4 + 4 starts at index -1 (the wraparound).
    "refuse": 5 -- under max_problem_size 5 the window of (0, 5) starts at -2, the sink's peak: the reference's assert."""
    if layout == "refuse":
        return [5]
    if layout == "b":
        return [r for r in (7, 60, 200) if r < n - 2] + list(range(240, n - 2, 40))
    out, c = [], 1
    for gap in (1, 63, 64, 65, 130, 257):
        out.append(c)
        if c + gap >= n - 2:
            return out
        c += gap
    out.append(c)
    while c + 40 < n - 2:
        c += 40; out.append(c)
    return out


def spike_ranks(n, layout):
    """A junction of weight 25 in the middle of every gap of four candidates and more between consecutive heavy ones (the interval's
    first position and the sink, candidate n - 2, included): not fixed, but enough for refinement to add its position (the light
    ones' 3 are not) -- which it does only if k_segments hands k_refine the segment with the right previous chosen candidate, however
    many 64-candidate chunks or block-sized steps back that one lies, in a slot of its own."""
    marks = [0] + heavy_ranks(n, layout) + [n - 2]
    return [(a + b) // 2 for a, b in zip(marks, marks[1:]) if b - a >= 4]


def width_part(n_cand, threads, layout="a"):
    """One interval of n_cand candidates -- its two ends, n_cand - 3 junctions and the sink, a stretch at its end --, as long as makes
    the host choose `threads` for k_fix / k_segments (the batch holds only such intervals: their length is the average)."""
    nj = n_cand - 3
    length = max(STEP * (nj + 1) + 150, WIDTH_LEN[threads])
    heavy = set(heavy_ranks(n_cand, layout))
    spikes = set() if layout == "refuse" else set(spike_ranks(n_cand, layout))
    pos = [STEP * (i + 1) for i in range(nj)]
    w = [400 if i + 1 in heavy else 25 if i + 1 in spikes else 3 for i in range(nj)]
    iv = (S0, S0 + length - 1)
    reads, w = util.junction_reads(iv, pos, w, (iv[1] - 99, iv[1]))
    return util.hand([iv], reads, w)


def width_case(threads, mps):
    counts = [n for n in COUNTS if threads != 64 or n <= 300]         # (1 100 candidates 45 apart do not fit 16 384 positions)
    names = ["cand-%d-%s" % (n, lay) for n in counts for lay in "ab"]
    return names, [width_part(n, threads, lay) for n in counts for lay in "ab"], dict(WIDTH_PARAMS, max_problem_size=mps)


def refusal_case(threads):
    return ["refuse-65"], [width_part(65, threads, "refuse")], dict(WIDTH_PARAMS, max_problem_size=5)


# ---- k_segments' inner-sum test and k_refine's two paths ---------------------------------------------------------------------
INNER_LENS = [41, 42, 200, 1024, 1025, 1100, 512 * 66 + 100]
INNER_P0 = [300, 492, 1004, 297]       # P0 + 20 on a block edge (320), a tile edge (512), both (1024), neither
INNER_D = (-2, -1, 0, 1, 2)
TAIL_PARAMS = dict(min_read_support_outside=1000, variance_factor=1.0)      # (the heavy junctions are fixed, a spike of 25 is not)


def segment_part(P0, length, inner, weights, heavy=400):
    """[interval, sink]: heavy junctions on positions P0 and P0 + length of the interval -- consecutive chosen candidates, the segment
    (P0, P0 + length] --, and the counts `weights` on the positions `inner` (relative to P0)."""
    return single(P0 + length + 60, [P0, P0 + length] + [P0 + q for q in inner], [heavy, heavy] + list(weights))


def inner_variants(length, side):
    """name -> (positions relative to P0, weights): a spike of 25 on the first (side a) / last (side b) inner position, P0 + 20 /
    P0 + length - 21, and up to two positions either way; 19 there with 1 on its neighbour outside; 19 alone."""
    edge, out = (20, -1) if side == "a" else (length - 21, 1)
    v = {"w25-d%+d" % d: ([edge - out * d], [25]) for d in INNER_D}
    v["split-19-1"] = ([edge, edge + out], [19, 1])
    v["w19"] = ([edge], [19])
    return v


def inner_case(length):
    names, parts = [], []
    for P0 in INNER_P0:
        for side in "ab":
            for n, (pos, w) in inner_variants(length, side).items():
                names.append("P0-%d-%s-%s" % (P0, side, n)); parts.append(segment_part(P0, length, pos, w))
    return names, parts, dict(TAIL_PARAMS)


REFINE_SIGMAS = {"sigma5": 5.0, "sigma50": 50.0, "sigma0.1": 0.1}


def refine_case(sigma):
    P0 = 700
    shapes = {
        "tie-1500": (1500, [745, 755], [25, 25]),                       # two equal clusters 10 apart, the segment in global memory
        "tie-900": (900, [445, 455], [25, 25]),                         # ... in LDS
        "flat-3200": (3200,) + tuple(util.flat_top(400, 2400)),         # a plateau's midpoint inside the refinement (either half: global)
        "flat-900": (900,) + tuple(util.flat_top(80, 740)),
        "apart-19": (1500, [600, 619, 900, 919], [30, 31, 31, 30]), "apart-20": (1500, [600, 620, 900, 920], [30, 31, 31, 30]),
        "apart-21": (1500, [600, 621, 900, 921], [30, 31, 31, 30]),
        "apart-20-lds": (900, [300, 320, 600, 620], [30, 31, 31, 30]),
        "len-1025": (1025, [22, 500, 1002], [30, 31, 30]), "len-1024": (1024, [22, 500, 1001], [30, 31, 30]),   # kRefCap and one more
    }
    names = list(shapes)
    return names, [segment_part(P0, L, pos, w, heavy=4000) for L, pos, w in shapes.values()], dict(TAIL_PARAMS, sigma=REFINE_SIGMAS[sigma])


def refined(o, k=0):
    """(previous chosen position, position) of every position refinement added to interval k, from the oracle's result."""
    c = o["cands"][o["cand_off"][k]:o["cand_off"][k + 1]]
    chosen = c[o["finalc"][o["finalc_off"][k]:o["finalc_off"][k + 1]]]
    fy = o["final_y"][o["final_off"][k]:o["final_off"][k + 1]]
    return [(int(chosen[np.searchsorted(chosen, y) - 1]), int(chosen[np.searchsorted(chosen, y)]), int(y)) for y in fy if y not in set(chosen.tolist())]


# ---- labels ------------------------------------------------------------------------------------------------------------------
LABEL_COLS = [1023, 1024, 1025, 2201]
LABEL_REPS = [1, 63, 64, 65, 257]
LABEL_PARAMS = dict(sigma=3.0, variance_factor=0.01, min_read_support_outside=1000)


def label_part(S, n_reps, seed):
    """Two intervals whose final positions are the ends of one rep's exons (30 positions an exon, a boundary on its positions 0 and
    14) and the intervals' own ends: S columns, the sentinel between the intervals among them.  The other n_reps - 1 reps are single
    exons (under ignore_ends they count nothing) placed against the columns' edges, and two-exon reads across the sentinel whose inner
    ends lie on boundaries that exist."""
    E = (S - 1) // 2 if S % 2 else S // 2               # 2E - 2 boundaries + 4 interval ends - 1; even S: one boundary on an interval's end
    E1 = E // 2
    a0, a1 = S0, S0 + 30 * E1 + (20 if S % 2 else -6)  # (even S: the last exon of the first interval ends on the interval's end)
    b0 = a1 + 500
    ex = [(a0 + 10 + 30 * i, a0 + 24 + 30 * i) for i in range(E1)] + [(b0 + 10 + 30 * i, b0 + 24 + 30 * i) for i in range(E - E1)]
    b1 = ex[-1][1] + 40
    bounds = sorted({a0, a1, b0, b1} | {x for e in ex for x in e} - {ex[0][0], ex[-1][1]})
    assert len(bounds) - 1 == S, (len(bounds) - 1, S)
    in_a = [g for g in bounds if g <= a1]
    rng = np.random.default_rng(seed)
    reads = []

    def col(c):                                         # (g0, g1) of column c; the sentinel is column len(in_a) - 1
        return bounds[c], bounds[c + 1]
    sent = len(in_a) - 1

    def add(x, y):                                      # a single exon, if it lies inside one interval
        if a0 <= x < y <= a1 or b0 <= x < y <= b1:
            reads.append([(x, y)])
    for i in (1, 2, 5):                                                               # across the sentinel, inner ends on boundaries
        reads.append([(in_a[-2 - 2 * i] - 3, ex[E1 - 1][1]), (ex[E1][0], ex[E1 + i][1] + 3)])
    edge_cols = [3, 15, 16, sent - 2, sent + 2, S - 4] + [c for c in (1023, 1024, 1040) if c < S - 3]
    for c in edge_cols:
        g0, g1 = col(c)
        add(g0 + 2, g0 + 6)                                                           # one exon inside one column
        for end in (g0 - 1, g0, g1 - 1, g1):                                          # ending on / starting from a column's edges
            add(bounds[c - 2] + 1, end)
            add(end, bounds[c + 3] - 1)
        for n in (1, 2, 3, 4, 5):                                                     # reaching n columns
            add(bounds[c] + 1, bounds[min(c + n - 1, S - 1)] + 1)
    while len(reads) < n_reps - 1:
        c = int(rng.integers(1, S - 6)); n = int(rng.integers(1, 7))
        add(bounds[c] + int(rng.integers(0, 14)), bounds[c + n - 1] + int(rng.integers(0, 14)))
    reads = [ex] + reads[:n_reps - 1]
    return util.hand([(a0, a1), (b0, b1)], reads, [60] + [1] * (len(reads) - 1))


def label_case(S, rate):
    return (["reps-%d" % r for r in LABEL_REPS], [label_part(S, r, 10 * S + r) for r in LABEL_REPS],
            dict(LABEL_PARAMS, threshold_rate=rate))


def twins0_case():
    return ["twins-2-3"], [twin_part("sigma0.1")], dict(sigma=0.1)


CASES = dict(twins0=twins0_case, one_position=one_position_case, width=width_case, refusal=refusal_case, inner=inner_case, refine=refine_case, label=label_case)


@functools.lru_cache(maxsize=None)
def case(kind, *key):
    """(names, partitions, params) of a case, built once."""
    if kind == "plateau":
        return plateau_case(*key)
    if kind == "length":
        return length_case(*key)
    if kind in CASES:
        return CASES[kind](*key)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def oracles(kind, *key):
    names, parts, params = case(kind, *key)
    return [util.run_oracle(p, params) for p in parts]


def run_on_gpu(kind, *key, iv_threads=None, smooth_r=None, label_packed=None):
    """One case on a fresh context (the switches are read by fseg_create): every tap against the case's oracles on the first run and
    on the replay, the smoothed signal bit-identical, the census words as given.  Returns the context's packed and byte labels."""
    from freddie_amd import _lib
    names, parts, params = case(kind, *key)
    want = oracles(kind, *key)
    ctx = _lib.Context(0)
    try:
        for run in ("first run", "replay"):
            if run == "first run":
                util.run_gpu(ctx, parts, params)
            else:
                ctx.run(); ctx.sync()
            census = ctx.paths()
            try:
                rep = util.compare_partitions(ctx, parts, want)
            except AssertionError as e:
                raise AssertionError("%s, %s (partitions: %s)" % (run, e, ", ".join("p%d %s" % x for x in enumerate(names)))) from None
            assert rep["y_identical"], "%s: smoothed signal not bit-identical (max err %g)" % (run, rep["max_y_err"])
            for word, v in (("iv_threads", iv_threads), ("smooth_r", smooth_r), ("label_packed", label_packed)):
                assert v is None or census[word] == v, (run, word, census[word], v)
        packed = ctx.results(packed=True)[3].copy()
        return ctx.download()[3], packed
    finally:
        ctx.close()
