"""The position compactions (k_pos_count, k_scan_emit<positions>: blocks of 32 768 positions, four flag words a thread, block sums
and sums of groups of 64 blocks) and the read ranges of the problems (k_prob_range: a workgroup's lanes staged in LDS) against
the CPU oracle, through the C-ABI: the smallest shapes at which they can go wrong.

An interval's first and last position are always candidates and final positions, so the intervals' lengths place flags exactly.
A wrong read range changes a DP's result: the ranges are checked through `chosen` and the `problems` rows."""
import functools

import numpy as np
import pytest

import util
from freddie_amd import _lib

pytestmark = pytest.mark.gpu

B = 32768              # kPosBlock (csrc/seg_common.h)
G = 64                 # kPosGroup
RANGE_BLOCK = 1024     # kRangeThreads: candidates per workgroup of k_prob_range
RANGE_STAGE = 4096     # kRangeStage: lanes it bisects in LDS
hand = util.hand


def layout(lengths, start=1000, gap=10):
    """Intervals of the given lengths, one behind the other: position q of the batch is known from the lengths alone."""
    ivs, s = [], start
    for n in lengths:
        ivs.append((s, s + n - 1)); s += n + gap
    return ivs


def end_reads(ivs, extra=()):
    """Reads near the two ends of every interval, nothing in between (an interval of a few positions gets one read over it)."""
    reads = []
    for a, b in ivs:
        if b - a < 900:
            reads.append([(a, b)])
            continue
        reads += [[(a + 5, a + 90), (a + 100, a + 400), (b - 400, b - 7)], [(a + 7, a + 95), (a + 100, a + 380), (b - 390, b - 3)],
                  [(a, a + 90), (a + 105, a + 400), (b - 400, b)]]
    return reads + list(extra)


def block_boundary():
    """Interval ends on position 767 (the last bit of a thread's fourth word; the next interval starts on the next thread's first
    bit), on the last position of block 0 and an interval start on the first position of block 1."""
    ivs = layout([768, B - 768, 1000, 4000])
    return [hand(ivs, end_reads(ivs))], {}


def empty_blocks(total):
    """One long interval with reads only near its ends: blocks, and threads' four words, without a flag.  total = 3 * B + 1: a last
    block of a single position; 2 * B + 77: a position count that is no multiple of 128."""
    ivs = layout([total])
    return [hand(ivs, end_reads(ivs))], {}


def two_groups():
    """Flags in the first and the last block of two neighbouring groups of the two-level sums (blocks 0, 63, 64, 127) and in the
    first block of a third (128); every block between holds none."""
    ivs = layout([63 * B + 600, B + 5, 63 * B, B + 93])
    pos = np.cumsum([0] + [b - a + 1 for a, b in ivs])
    assert [int(q // B) for q in pos[1:] - 1] == [63, 64, 127, 128] and 64 % G == 0 and pos[-1] > 2 * G * B
    return [hand(ivs, end_reads(ivs))], dict(ignore_ends=False)


def unstaged():
    """1 100 intervals of nine positions in one block: more than the emit kernel's LDS stage of 768 intervals."""
    ivs = [(1000 + 12 * k, 1000 + 12 * k + 8) for k in range(1100)]
    rng = np.random.default_rng(5)
    reads = []
    for _ in range(40):
        ks = np.sort(rng.choice(1100, 6, replace=False))
        reads.append([(ivs[k][0] + int(rng.integers(0, 4)), ivs[k][1] - int(rng.integers(0, 4))) for k in ks])
    return [hand(ivs, reads)], {}


def stage_boundary():
    """A partition of 5 000 reps (its lanes alone exceed the LDS stage: the bisections in device memory) between partitions that
    fit; the last workgroup's candidates lie in small partitions only."""
    big = util.make_partition(11, dedupe=False, n_reads=5000, n_exons=24, max_span=0)
    assert big.n_reps > RANGE_STAGE
    small = [util.make_partition(20 + i, n_reads=200, n_exons=60, rp=0.05) for i in range(12)]
    return [small[0], big] + small[1:], {}


def many_small():
    """96 partitions of eight reads: one workgroup's candidates span dozens of partitions."""
    return [util.make_partition(7000 + i, n_reads=8, n_exons=5 + i % 4, max_span=0) for i in range(96)], {}


def straddle():
    """More than 1 024 candidates, with a problem whose candidates lie on both sides of a 1 024-candidate boundary."""
    return [util.make_partition(31 + i, n_reads=300, n_exons=120, rp=0.05) for i in range(10)], {}


def odd_count():
    """A candidate count that is no multiple of 1 024: the last workgroup of k_prob_range is partly idle."""
    return [util.make_partition(41 + i, n_reads=250, n_exons=90, rp=0.05) for i in range(8)], {}


MULTI = {"FSEG_SCAN_SINGLE_MAX": "0"}        # block sums + group sums at any size (by default up to 512 blocks look back)
CASES = {
    "block-boundary": (block_boundary, [{}, MULTI]),
    "empty-blocks-single-position": (lambda: empty_blocks(3 * B + 1), [{}, MULTI]),
    "empty-blocks-odd-count": (lambda: empty_blocks(2 * B + 77), [{}, MULTI]),
    "two-groups": (two_groups, [MULTI]),
    "unstaged-intervals": (unstaged, [{}, MULTI]),
    "range-stage-boundary": (stage_boundary, [{}]),
    "range-many-small": (many_small, [{}]),
    "range-straddle": (straddle, [{}]),
    "range-odd-count": (odd_count, [{}]),
}
RUNS = [(name, i) for name, (_, envs) in CASES.items() for i in range(len(envs))]


@functools.lru_cache(maxsize=None)
def case(name):
    parts, params = CASES[name][0]()
    return parts, params, [util.run_oracle(p, params) for p in parts]


def candidate_problems(oracles):
    """(first, last) batch-wide candidate index of every DP problem of at least three candidates, and the candidate count."""
    spans, c0 = [], 0
    for o in oracles:
        n = o["prob_end"] - o["prob_start"] + 1
        first = c0 + o["cand_off"][o["prob_interval"]] + o["prob_start"]
        spans += [(int(a), int(a + m - 1)) for a, m in zip(first, n) if m >= 3]
        c0 += int(o["cand_off"][-1])
    return spans, c0


def block_lanes(parts, oracles):
    """Lanes (reads) of the partitions that every block of 1 024 candidates touches: what a workgroup of k_prob_range would stage."""
    ends = np.cumsum([int(o["cand_off"][-1]) for o in oracles])
    lanes = np.array([int(p.rep_weight.sum()) for p in parts])
    out = []
    for c0 in range(0, int(ends[-1]), RANGE_BLOCK):
        p0 = int(np.searchsorted(ends, c0, side="right")); p1 = int(np.searchsorted(ends, min(c0 + RANGE_BLOCK, ends[-1]) - 1, side="right"))
        out.append(int(lanes[p0:p1 + 1].sum()))
    return out


def flagged(oracles, key_off, key_y):
    """Batch-wide positions of the oracle's candidates (cand_off, cands) or final positions (final_off, final_y), ascending."""
    out, p0 = [], 0
    for o in oracles:
        po, off, y = o["pos_off"], o[key_off], o[key_y]
        for k in range(len(po) - 1):
            out.append(p0 + po[k] + np.asarray(y[off[k]:off[k + 1]], np.int64))
        p0 += int(po[-1])
    return np.concatenate(out)


def check_shape(name, parts, oracles):
    """The case is what its name says (the oracle's own figures, before anything runs on the device)."""
    spans, n_cand = candidate_problems(oracles)
    cand, final = flagged(oracles, "cand_off", "cands"), flagged(oracles, "final_off", "final_y")
    n_pos = sum(int(o["pos_off"][-1]) for o in oracles)
    if name == "block-boundary":
        for f in (cand, final):                 # a thread's last bit and the next one's first; a block's last position and the next one's first
            assert {767, 768, B - 1, B} <= set(f.tolist()) and n_pos > B
    if name.startswith("empty-blocks"):
        for f in (cand, final):                 # flags within 512 positions of the interval's ends only: the middle block and most threads hold none
            assert f[0] == 0 and f[-1] == n_pos - 1 and not ((f >= 512) & (f < n_pos - 512)).any() and n_pos > 2 * B
        assert n_pos % 128 != 0 and (name != "empty-blocks-single-position" or n_pos % B == 1)
    if name == "two-groups":
        for f in (cand, final):                 # the blocks that hold a flag at all
            assert sorted(set((f // B).tolist())) == [0, 63, 64, 127, 128]
    if name == "unstaged-intervals":
        assert len(parts[0].iv_start) > 768 and n_pos <= B
    if name.startswith("range"):
        assert spans, "no DP problem"
    if name == "range-straddle":
        assert n_cand > RANGE_BLOCK and any(a // RANGE_BLOCK != b // RANGE_BLOCK for a, b in spans), (n_cand, len(spans))
    if name == "range-odd-count":
        assert n_cand > RANGE_BLOCK and n_cand % RANGE_BLOCK != 0, n_cand
    if name == "range-many-small":
        assert len(parts) >= 64 and n_cand < RANGE_BLOCK * 2
    if name == "range-stage-boundary":
        lanes = block_lanes(parts, oracles)
        assert max(lanes) > RANGE_STAGE and min(lanes) <= RANGE_STAGE and len(lanes) >= 2, lanes
    elif name.startswith("range"):
        assert max(block_lanes(parts, oracles)) <= RANGE_STAGE


@pytest.mark.parametrize("name,env", RUNS, ids=["%s-%s" % (n, "multi" if CASES[n][1][i] else "default") for n, i in RUNS])
def test_compaction_edges(name, env, monkeypatch):
    monkeypatch.delenv("FSEG_SCAN_SINGLE_MAX", raising=False)
    for k, v in CASES[name][1][env].items():
        monkeypatch.setenv(k, v)
    parts, params, oracles = case(name)
    check_shape(name, parts, oracles)
    ctx = _lib.Context(0)
    try:
        util.run_gpu(ctx, parts, params)
        util.compare_partitions(ctx, parts, oracles)
        cand_y = ctx.tap("cand_y").copy(); final_pos = ctx.download()[1].copy()
        ctx.run(); ctx.sync()                                          # the replay (the captured launch)
        assert np.array_equal(ctx.tap("cand_y"), cand_y) and np.array_equal(ctx.download()[1], final_pos)
    finally:
        ctx.close()
