"""Hand-built batches for what k_thr_part carries from one step to the next: the partial chunk's leaf table
across the two passes and from one partition of a workgroup to its next, the first LDS_VALS values of V in LDS, the flag words a
wave keeps in registers, and the chunk sums of more chunks than one sweep holds.  Built on tests/threshold_cases.py (filled(): every
position of a partition is flagged, so |V| is the partition's length).

A batch has GRID + 32 partitions: partition k and k + GRID are walked by the same workgroup, one after the other, so a pair
(first, second) of counts sits at k and k + GRID and everything between is filler.  tests/test_threshold_chain_host.py shows on the
CPU that every pair reaches the edge it is there for and that a stale table, stale values or a dropped last LDS value would change the
second partition's threshold; tests/test_gpu_threshold_chain.py runs the batches on the device."""
import functools

import numpy as np

import threshold_cases as tc
import util

CHUNK, GROUP, GRID, S0 = tc.CHUNK, tc.GROUP, tc.GRID, tc.S0
KEEP_GROUPS = 8        # kThrKeepGroups (csrc/seg_common.h): flag words a lane keeps; a wave's further groups are read a second time
SWEEP_CHUNKS = 4       # kThrSweepChunks: chunks summed in one sweep
LDS_VALS = 8192        # kThrLdsVals: values of V that stay in LDS
BIG = 140000           # 69 groups of 2 048 positions: nine a wave (one more than kept), 18 chunks (five sweeps)

# the counts of a batch, and (first, second) pairs of them on one workgroup: every count after its neighbour and before it.
# "ends" counts the reads' ends (the only way to |V| = 2: an interval of two positions); "nan" ignores them (the only way to |V| = 0)
# and puts the empty partition before and behind every other count.
COUNTS = {
    "ends": [2, 7, 8, 9, 128, 129, LDS_VALS - 1, LDS_VALS, LDS_VALS + 1, 2 * CHUNK, 2 * CHUNK + 1, SWEEP_CHUNKS * CHUNK + 1, BIG],
    "nan": [0, 7, 8, 9, 128, 129, LDS_VALS - 1, LDS_VALS, LDS_VALS + 1, 2 * CHUNK, 2 * CHUNK + 1, SWEEP_CHUNKS * CHUNK + 1],
}
PARAMS = {"ends": dict(sigma=5.0, variance_factor=9.99, ignore_ends=False), "nan": dict(sigma=5.0, variance_factor=9.99, ignore_ends=True)}
# weight seeds of the counts threshold_cases.A_SEEDS does not have (search_seed(): every wrong-order model gives other bits; at BIG no
# seed of 0 .. 399 separates all five -- under 42 "chunks-right-to-left" alone keeps numpy's bits)
SEEDS = {SWEEP_CHUNKS * CHUNK + 1: 22, BIG: 42}
KINDS = list(COUNTS)


def pairs(kind):
    c = COUNTS[kind]
    if kind == "ends":
        fwd = [(c[i], c[(i + 1) % len(c)]) for i in range(len(c))]
        return fwd + [(b, a) for a, b in fwd]
    return [(0, m) for m in c[1:]] + [(m, 0) for m in c[1:]]


@functools.lru_cache(maxsize=None)
def partition(kind, m):
    """The partition of a count: the same object wherever the count stands, so its oracle is computed once."""
    if kind == "ends":
        return tc.filled(m, tc.A_SEEDS.get(m, SEEDS.get(m, 0)))
    return tc.filled(3 if m == 0 else m, 40 + m % 7, ends=False)      # (three positions, one single-exon read: nothing is counted)


@functools.lru_cache(maxsize=None)
def filler(kind, i):
    if kind == "ends":
        L = 40 + 7 * i
        iv = (S0, S0 + L - 1)
        return util.hand([iv], [[(S0 + 3 + i, S0 + L - 5)]] + ([[iv]] if i % 2 else []), [11 + i] + ([5] if i % 2 else []))
    return tc.filled(40 + 7 * i, 90 + i, ends=False)


@functools.lru_cache(maxsize=None)
def case(kind):
    """(names, partitions, params): the pairs at k and k + GRID, four filler partitions in turn everywhere else."""
    pr = pairs(kind)
    assert len(pr) <= 32
    named = {}
    for k, (a, b) in enumerate(pr):
        named[k], named[k + GRID] = a, b
    names, parts = [], []
    for p in range(GRID + 32):
        if p in named:
            names.append("m-%d" % named[p]); parts.append(partition(kind, named[p]))
        else:
            names.append("filler-%d" % (p % 4)); parts.append(filler(kind, p % 4))
    return names, parts, dict(PARAMS[kind])


@functools.lru_cache(maxsize=None)
def oracles(kind):
    names, parts, params = case(kind)
    done = {}
    for part in parts:
        if id(part) not in done:
            done[id(part)] = util.run_oracle(part, params)
    return [done[id(part)] for part in parts]


# ---- the chain's structure and what stale state would compute, in plain Python ------------------------------------------------------
def structure(n):
    """What the kernel derives from |V| = n: chunks, full chunks, the partial chunk's count, its leaves, sweeps."""
    nch, nfull = (n + CHUNK - 1) // CHUNK, n // CHUNK
    m_last = n - nfull * CHUNK

    def leaves(shape):
        return [shape] if isinstance(shape, int) else leaves(shape[0]) + leaves(shape[1])
    return dict(nch=nch, nfull=nfull, m_last=m_last, leaves=leaves(tc._shape(m_last, True)) if m_last else [],
                sweeps=(nch + SWEEP_CHUNKS - 1) // SWEEP_CHUNKS, in_lds=min(n, LDS_VALS))


def groups_per_wave(length, start=0):
    words = ((start + length + 31) >> 5) - (start >> 5)
    return ((words + 63) // 64 + 7) // 8


def _sum_shape(a, shape):
    if isinstance(shape, int):
        return tc._leaf8(a[:shape]), a[shape:]
    left, a = _sum_shape(a, shape[0])
    right, a = _sum_shape(a, shape[1])
    return left + right, a


def _threshold(v, vf, chunk_sum):
    n = float(len(v))

    def total(a):
        cs = [chunk_sum(a[s:s + CHUNK]) for s in range(0, len(a), CHUNK)]
        res = cs[0]
        for x in cs[1:]:
            res += x
        return res
    mean = total(v) / n
    d = v - mean
    return float(mean + vf * np.sqrt(total(d * d) / n))


def stale_table_threshold(v, m_before, vf, before=None):
    """The partial chunk summed with the leaf table of a chunk of m_before values.  What a longer table reads past the chunk's own
    values: where the chunk lies in LDS (|V| < LDS_VALS), the values the partition before left there (`before`: its V); else zeros."""
    def chunk_sum(a):
        if len(a) == CHUNK:
            return tc._pairwise(a, tc._leaf8, True)
        b = np.zeros(m_before)
        if before is not None and len(v) < LDS_VALS:
            b[:min(m_before, len(before))] = before[:m_before]
        b[:min(len(a), m_before)] = a[:m_before]
        return _sum_shape(b, tc._shape(m_before, True))[0]
    return _threshold(v, vf, chunk_sum)


def stale_values_threshold(v, before, vf, only_last=False):
    """The values in LDS still the previous partition's (only_last: the last of them alone -- its own value never arrived)."""
    w = v.copy()
    k = min(len(v), LDS_VALS)
    old = np.zeros(k)
    old[:min(k, len(before))] = before[:k]
    if only_last:
        w[k - 1] = old[k - 1]
    else:
        w[:k] = old
    return _threshold(w, vf, lambda a: tc._pairwise(a, tc._leaf8, True))
