"""Hand-built partitions for the variance threshold (S3a: mean(V) + vf * std(V) over a partition's Y > 0 values, in numpy's summation
order) at the sizes where its code takes another branch -- vsum_chunk's trees, k_thr_part's groups, words and chunk sums, and the
chunk path (k_scan_emit<values>, k_scan1 / k_scan2, k_voff, k_vplan, k_vsum_chunks, k_vsum_part).  Built on util.hand(): counts are
placed position by position, so a case says how many values its V holds and on which word, row, group or block they sit.
tests/test_threshold_cases_host.py runs every case through the CPU oracle and asserts that it reaches the edge it is named after,
that the oracle is numpy, and that a wrong summation order would change the threshold's bits; tests/test_gpu_threshold_edges.py
runs the same cases on the device both ways.

A case is (names, partitions, params); a case's oracles are computed once (oracles()) and shared by every test.

Group A (tree shapes): one partition per count m, every position flagged, so |V| = m.
Group B (which values reach V, in what order): flags on chosen single positions (sigma 0.1: radius 0, V is the counts themselves,
  so a lost, doubled or foreign value changes an integer sum), again under sigma 3 (runs of 25 real values over the same places).
  Two batches: "ends" counts the reads' own ends (ignore_ends off), the only way to flag a partition's first and last position;
  "nan" ignores them, the only way to a partition without a value (single-exon reads count nothing: threshold NaN).
Group C (limits): 2^20 positions (128 full chunks: k_thr_part's last chunk sum), one more (the host falls back to the chunk
  kernels), and more than 4 096 partitions (k_thr_part's workgroups take a second partition; k_vplan's carry, the grid loops of
  k_voff and k_vsum_chunks).

Not reachable at test size: k_scan2's second round needs more than 8 192 blocks of 8 192 positions (67 M positions)."""
import functools

import numpy as np

import util

CHUNK = 8192           # numpy's buffer and kScanBlock (csrc/seg_common.h): values per chunk, positions per scan block
GROUP = 2048           # positions of a wave's 64 flag words
MAX_CHUNKS = 128       # kThrPartMaxChunks
GRID = 4096            # workgroups of k_thr_part at most
S0 = 1000              # genomic start of every partition's first interval


def radius(sigma):
    return int(4 * sigma + 0.5)


# ---- a partition whose every position is flagged -------------------------------------------------------------------------------
def filled(L, seed, sigma=5.0, ends=True):
    """One interval of L positions with a count at most 2 r + 1 positions from the next (r: the filter's radius), the reads' ends
    counted (they start on the interval's first and end on its last position; `ends` off: not counted, the last junction within r of
    the interval's end instead): every position's smoothed value is positive, so |V| = L, real-valued.  Junctions come in pairs, a two-exon read [(0, a), (b, L - 1)] each, with weights 1 .. 60 drawn from
    `seed`; an interval of two or three positions holds one single-exon read (two equal values / a symmetric triple)."""
    r, rng = radius(sigma), np.random.default_rng(seed)
    iv = (S0, S0 + L - 1)
    if L < 4:
        return util.hand([iv], [[iv]], [int(rng.integers(1, 61))])
    q, junctions = int(rng.integers(1, min(r, L - 3) + 1)), []
    while q <= L - 2:
        junctions.append(q); q += int(rng.integers(max(1, r // 2), 2 * r + 2))
    if L - 1 - junctions[-1] > (2 * r + 1 if ends else r) or len(junctions) < 2:
        junctions.append(L - 2)
    junctions = sorted(set(junctions))
    if len(junctions) % 2:
        junctions.insert(-1, junctions[-2] if len(junctions) > 2 else junctions[0])       # (a position used twice: its counts add up)
        junctions.sort()
    pairs = list(zip(junctions[0::2], junctions[1::2]))
    reads = [[(S0, S0 + a), (S0 + b, iv[1])] if a < b else [(S0, S0 + a), (S0 + a + 1, iv[1])] for a, b in pairs]
    return util.hand([iv], reads, rng.integers(1, 61, len(reads)))


# Group A: m -> weight seed, the first of 0 .. 999 under which every wrong-order model that is not numpy's order by construction
# at that m (same_by_construction()) gives a threshold with other bits (found by search_seed()); no exception was needed.
# m = 2 is the smallest: the input format has no interval of one position (upload refuses it, as the reference's read_split asserts
# start < end), and a single positive position inside a longer interval needs radius 0, which group B runs.  Its two values are
# equal: std == 0, the threshold equals Y, and k_fix's strict > fixes nothing.
A_SEEDS = {
    2: 0, 7: 0, 8: 0, 9: 0, 15: 4, 16: 6, 17: 4, 63: 0, 64: 0, 65: 0, 127: 0, 128: 1, 129: 4, 135: 15, 136: 7, 137: 17,
    255: 7, 256: 2, 257: 0, 265: 1, 1023: 17, 1024: 0, 1025: 0, 4096: 1, 8184: 1, 8191: 10, 8192: 0, 8193: 31, 8199: 14, 8200: 0,
    8192 + 128: 7, 8192 + 129: 3, 16383: 14, 16384: 0, 16385: 8,
}
A_PARAMS = dict(sigma=5.0, variance_factor=9.99, ignore_ends=False)


def group_a():
    return ["m-%d" % m for m in A_SEEDS], [filled(m, s) for m, s in A_SEEDS.items()], dict(A_PARAMS)


# ---- flags on chosen single positions ------------------------------------------------------------------------------------------
class Layout:
    """Partitions of one interval each, one behind the other: batch position q of a partition's position i is known from the
    lengths alone.  add() takes flags as batch positions (`at`) or positions inside the partition (`rel`, negative: from its end)."""

    def __init__(self, ends, seed):
        self.ends, self.rng, self.pos = ends, np.random.default_rng(seed), 0
        self.names, self.parts, self.flags, self.starts = [], [], [], []

    def add(self, name, length, at=(), rel=()):
        f = sorted({q - self.pos for q in at} | {i % length for i in rel})
        assert length >= 2 and all(0 <= i < length for i in f) and len(f) != 1, (name, length, f)
        iv = (S0, S0 + length - 1)
        if not f:                                              # no junction: nothing is counted (ends ignored), the threshold is NaN
            assert not self.ends
            reads = [[iv]]
        elif self.ends:                                        # single-exon reads (a, b): a count on a and on b
            pairs = list(zip(f[0::2], f[1::2])) + ([(f[-2], f[-1])] if len(f) % 2 else [])
            reads = [[(S0 + a, S0 + b)] for a, b in pairs]
        else:                                                  # two-exon reads [(0, a), (b, L - 1)]: a count on a and on b
            assert f[0] >= 1 and f[-1] <= length - 2, (name, f)
            pairs = list(zip(f[0::2], f[1::2])) + ([(f[-2], f[-1])] if len(f) % 2 else [])
            reads = [[(S0, S0 + a), (S0 + b, iv[1])] for a, b in pairs]
        self.names.append(name); self.parts.append(util.hand([iv], reads, self.rng.integers(1, 61, len(reads))))
        self.flags.append([self.pos + i for i in f]); self.starts.append(self.pos)
        self.pos += length
        return self

    def until(self, name, target, **kw):
        return self.add(name, target - self.pos, **kw)


ROWS = {8: [0, 3, 4, 9, 17, 18, 30, 31], 9: [0, 1, 5, 8, 13, 21, 22, 29, 31], 32: list(range(32))}


def row_flags(base, n):
    """Flags in exactly n rows of 64 of the group of 2 048 positions at batch position `base`: one or two a row, on changing
    columns, column 0 and 63 among them."""
    out = []
    for j, q in enumerate(ROWS[n]):
        out.append(base + 64 * q + (0 if j == 0 else 63 if j == 1 else (7 * j + 3 * q) % 64))
        if j % 3 == 2:
            out.append(base + 64 * q + (11 * j + 40) % 64)
    return sorted(set(out))


WORD_OFFSETS = (31, 32, 63, 64, 2047, 2048)


def group_b_ends():
    """ignore_ends off.  Every figure in a name is a batch position or a count of groups of 2 048 positions."""
    lay = Layout(True, 71)
    lay.add("first-last-45", 45, rel=(0, -1, 31, 32))                              # ends in the middle of word 1
    # starts in word 1 beside its neighbour's last flag; 31 / 32, 63 / 64, 2047 / 2048 from its word-aligned start (32)
    lay.add("word-shared-2110", 2110, at=[45] + [32 + d for d in WORD_OFFSETS], rel=(-1,))
    # the same offsets from a wave's 2 048 positions and from the blocks of 8 192 (k_scan_emit<values>); crosses two block edges
    at = [2 * GROUP + d for d in WORD_OFFSETS[:4]] + [CHUNK - 1, CHUNK] + [CHUNK + d for d in WORD_OFFSETS] + [2 * CHUNK - 1, 2 * CHUNK]
    lay.until("blocks-0-to-2", 2 * CHUNK + 7, at=at, rel=(0, -1))
    lay.until("fill-a", 3 * CHUNK - 1, rel=(0, 5, -1))
    lay.add("start-24575", 40, rel=(0, 1, -1))                                     # 8192 k - 1
    lay.until("fill-b", 4 * CHUNK, rel=(0, -2))
    lay.add("start-32768", 77, rel=(0, 33, -1))                                    # 8192 k
    lay.until("fill-c", 5 * CHUNK + 1, rel=(0, -1))
    lay.add("start-40961", 50, rel=(0, 30, 31, -1))                                # 8192 k + 1
    lay.until("fill-d", 6 * CHUNK, rel=(3, -1))
    for n in (8, 9, 32):                                                           # rows of 64 with a flag inside one group
        lay.add("rows-%d" % n, GROUP, at=row_flags(lay.pos, n))
    for g in (1, 7, 8, 9, 17):                                                     # groups a partition: waves with none, one, two
        at = [lay.pos + GROUP * k + d for k in range(g) for d in ((0, 1029, GROUP - 1) if k % 2 == 0 else (64 * k % GROUP + 5, GROUP - 1))]
        lay.add("groups-%d" % g, GROUP * g, at=at)
    lay.add("odd-start-33", 33, rel=(0, -1))                                       # the next partition's groups start in the middle of a word
    x = lay.pos - 33                                                               # (a multiple of 2 048; the partition's first word starts on x + 32)
    at = [x + GROUP * k + d for k in range(1, 8) for d in (0, 31, 32, GROUP - 1)] + [x + GROUP * 8, x + GROUP * 8 + 31]
    at += [x + 32 + GROUP * k + d for k in (1, 2, 7, 8) for d in (-1, 0)]
    lay.add("groups-9-unaligned", GROUP * 8 + 5, at=at, rel=(0, -1))               # 9 groups from its word-aligned start, the last of one word
    lay.add("last-101", 101, rel=(0, 64, -1))                                      # the batch ends on no multiple of 64
    assert lay.pos % 64 != 0
    return lay


def group_b_nan():
    """ignore_ends on: partitions without a junction (NaN) first, between two others, two in a row, and last."""
    lay = Layout(False, 72)
    lay.add("nan-first", 45)
    lay.add("after-nan-2100", 2100, at=[32 + d for d in WORD_OFFSETS], rel=(1, -2))
    lay.add("nan-between", 19)
    lay.until("blocks", 2 * CHUNK + 7, at=[CHUNK - 1, CHUNK] + [CHUNK + d for d in WORD_OFFSETS] + [2 * CHUNK - 1, 2 * CHUNK], rel=(1, -2))
    lay.add("nan-pair-0", 3000); lay.add("nan-pair-1", 64)
    lay.until("to-block-3", 3 * CHUNK, rel=(1, 2, -2))
    lay.add("rows-9", GROUP, at=[max(q, lay.pos + 1) for q in row_flags(lay.pos, 9)])  # (position 0 cannot be flagged here)
    lay.add("nan-last", 101)
    assert lay.pos % 64 != 0
    return lay


B_SIGMAS = {"sigma0.1": 0.1, "sigma3": 3.0}
B_LAYOUTS = {"ends": group_b_ends, "nan": group_b_nan}


@functools.lru_cache(maxsize=None)
def layout(which):
    return B_LAYOUTS[which]()


def group_b(which, sigma):
    lay = layout(which)
    return lay.names, lay.parts, dict(sigma=B_SIGMAS[sigma], ignore_ends=which != "ends")


# ---- limits ----------------------------------------------------------------------------------------------------------------------
C_BIG_PARAMS = dict(sigma=50.0, variance_factor=0.99, ignore_ends=True)
C_BIG = {"c1": (MAX_CHUNKS * CHUNK, 3), "c2": (MAX_CHUNKS * CHUNK + 1, 3)}        # name -> (positions, weight seed)


def group_c_big(which):
    L, seed = C_BIG[which]
    small = filled(300, 1, 50.0, ends=False)
    return ["small-300", "m-%d" % L], [small, filled(L, seed, 50.0, ends=False)], dict(C_BIG_PARAMS)


# C3: index -> (|V|, weight seed); every other partition is tiny.  Partition p and p + 4 096 are the same workgroup's in k_thr_part.
C3_PARTS = 4104
C3_NAMED = {2: (8191, 10), 2 + GRID: (129, 4), 3: (CHUNK + 300, 30), 3 + GRID: (500, 0), 5: (129, 4), 5 + GRID: (2 * CHUNK + 1, 8)}
C3_PARAMS = dict(sigma=5.0, variance_factor=9.99, ignore_ends=False)


def group_c_many():
    rng = np.random.default_rng(73)
    names, parts = [], []
    for p in range(C3_PARTS):
        if p in C3_NAMED:
            m, seed = C3_NAMED[p]
            names.append("m-%d" % m); parts.append(filled(m, seed))
            continue
        L = int(rng.integers(40, 61))
        iv = (S0, S0 + L - 1)
        a = int(rng.integers(0, L - 8)); b = int(rng.integers(a + 1, L))
        reads = [[(S0 + a, S0 + b)]] + ([[iv]] if p % 3 == 0 else [])
        names.append("tiny-%d" % p); parts.append(util.hand([iv], reads, rng.integers(1, 61, len(reads))))
    return names, parts, dict(C3_PARAMS)


CASES = dict(a=group_a, b=group_b, c_big=group_c_big, c_many=group_c_many)
ALL = [("a",)] + [("b", w, s) for w in B_LAYOUTS for s in B_SIGMAS] + [("c_big", "c1"), ("c_big", "c2"), ("c_many",)]


@functools.lru_cache(maxsize=None)
def case(kind, *key):
    """(names, partitions, params) of a case, built once."""
    return CASES[kind](*key)


@functools.lru_cache(maxsize=None)
def oracles(kind, *key):
    names, parts, params = case(kind, *key)
    return [util.run_oracle(p, params) for p in parts]


def values(o):
    return o["Y"][o["Y"] > 0]


# ---- numpy's summation order and four plausible mistakes, in plain Python ---------------------------------------------------------
def _leaf8(a):
    """A leaf of at most 128 values: from 0.0 left to right below 8, else eight accumulators and the len % 8 tail."""
    n = len(a)
    if n < 8:
        res = 0.0
        for x in a.tolist():
            res += x
        return res
    r = a[:8].copy()
    body = n - n % 8
    for i in range(8, body, 8):
        r += a[i:i + 8]
    r = r.tolist()
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for x in a[body:].tolist():
        res += x
    return res


def _ltr(a):
    res = 0.0
    for x in a.tolist():
        res += x
    return res


def _pairwise(a, leaf, rounded):
    n = len(a)
    if n <= 128:
        return leaf(a)
    n2 = n // 2
    if rounded:
        n2 -= n2 % 8
    return _pairwise(a[:n2], leaf, rounded) + _pairwise(a[n2:], leaf, rounded)


def _shape(n, rounded):
    """The recursion's tree over n values as nested leaf lengths."""
    if n <= 128:
        return n
    n2 = n // 2
    if rounded:
        n2 -= n2 % 8
    return (_shape(n2, rounded), _shape(n - n2, rounded))


def _sum(a, model):
    if model == "left-to-right":
        return _ltr(a)
    if model == "unchunked":
        return _pairwise(a, _leaf8, True)
    leaf = _ltr if model == "leaves-left-to-right" else _leaf8
    cs = [_pairwise(a[s:s + CHUNK], leaf, model != "halves-unrounded") for s in range(0, len(a), CHUNK)]
    if model == "chunks-right-to-left":
        cs.reverse()
    res = cs[0]
    for x in cs[1:]:
        res += x
    return res


UNSEPARATED = set()    # (m, model): no weight seed of 0 .. 999 gave that model a threshold with other bits at that count -- none so far
MODELS = ("left-to-right", "halves-unrounded", "leaves-left-to-right", "unchunked", "chunks-right-to-left")


def model_threshold(v, vf, model="numpy"):
    """mean(v) + vf * std(v) as numpy computes it, with every sum taken in the model's order."""
    n = float(len(v))
    mean = _sum(v, model) / n
    d = v - mean
    return float(mean + vf * np.sqrt(_sum(d * d, model) / n))


def same_by_construction(m, model):
    """Whether the model adds m values in numpy's own order (up to the commutativity of one addition)."""
    if model in ("left-to-right", "leaves-left-to-right"):
        return m < 8
    if model == "halves-unrounded":
        return all(_shape(min(CHUNK, m - s), True) == _shape(min(CHUNK, m - s), False) for s in range(0, m, CHUNK))
    if model == "unchunked":                           # (16 384 values halve into the two chunks)
        chain = _shape(min(CHUNK, m), True)
        for s in range(CHUNK, m, CHUNK):
            chain = (chain, _shape(min(CHUNK, m - s), True))
        return chain == _shape(m, True)
    return m <= 2 * CHUNK                              # chunks right to left: two chunk sums are one addition


def separated(v, vf, m=None):
    """The models whose order differs from numpy's at this count and whose threshold has other bits / the same bits."""
    want = model_threshold(v, vf)
    diff = [k for k in MODELS if not same_by_construction(len(v), k)]
    hit = [k for k in diff if model_threshold(v, vf, k) != want]
    return hit, [k for k in diff if k not in hit]


def search_seed(m, sigma=5.0, params=A_PARAMS, tries=1000):
    """The first weight seed under which filled(m, seed) separates every model (how the seeds of the tables above were found)."""
    best = (None, MODELS)
    for seed in range(tries):
        o = util.run_oracle(filled(m, seed, sigma, ends=not params.get("ignore_ends", True)), params, stop_after=1)
        missed = separated(values(o), params["variance_factor"])[1]
        if not missed:
            return seed, []
        if len(missed) < len(best[1]):
            best = (seed, missed)
    return best
