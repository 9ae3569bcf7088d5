"""S1 with packed 16-bit LDS counters (k_hist<16>) against the 32-bit instance and the CPU oracle, through the C-ABI: the smallest
shapes at which the packing can go wrong.  Every case runs under FSEG_HIST16=0 and =1, the census (the `paths` tap, word `hist16`)
says which instance ran, Y_raw is compared with == and every later tap through util.compare_partitions.

Position i of a chunk is half i & 1 of LDS word i >> 1, a chunk starts anywhere (p0 is the sum of the positions before it), and
the chunk's size is halved while the batch would have fewer than 512 chunks -- so a small batch runs chunks of 1 024 positions and
only a batch of 512 * kHistChunk16 positions runs them at full size (chunk_edges carries a filler partition for that)."""
import functools

import numpy as np
import pytest

import util
from freddie_amd import _lib

pytestmark = pytest.mark.gpu

K16 = 16384            # kHistChunk16 (csrc/seg_common.h)
ENDS = dict(ignore_ends=False)
hand, shifted = util.hand, util.shifted


# three exons a read: under ignore_ends the first exon's start and the last exon's end do not count, the four ends between do
A = [(1000, 1049), (1060, 1100), (1200, 1300)]       # ends at positions 49, 60, 100 (even), 200 of an interval that starts at 1000
B = [(1002, 1031), (1070, 1101), (1210, 1320)]       # ... 31, 70, 101 (odd: the other half of A's word), 210
C = [(1004, 1051), (1101, 1150), (1220, 1340)]       # a start on 101


def neighbours():
    """Positions 2k and 2k + 1 hit by different reads' ts / te, and the same shifted by one position (the pair in two words)."""
    reads = [A, B, C, A]
    return [hand([(1000, 1399)], reads), hand([(1000, 1399)], shifted(reads, 1))], {}


def bound(weight):
    """One rep of `weight` reads ends on an even position, another read on the odd position next to it."""
    return [hand([(1000, 1399)], [A, B], [weight, 1])], {}


def edge_reads(s, length, ivs):
    """Single-exon reads that end on position q - 1 and start on position q, for every q a multiple of 1 024 (the edge of a chunk
    whatever power of two its size), and reads over every whole interval (the partition's first and last position)."""
    reads = [[(a, b)] for a, b in ivs]
    pos = np.concatenate([np.arange(a, b + 1) for a, b in ivs])       # genomic coordinate of every position
    for q in range(1024, length, 1024):
        reads.append([(int(pos[q - 300]), int(pos[q - 1]))])
        reads.append([(int(pos[q]), int(pos[q + 200]))] if q + 200 < length else [(int(pos[q - 200]), int(pos[q]))])
    return reads


def chunk_edges():
    """Partitions of kHistChunk16 + 1 and 2 * kHistChunk16 - 1 positions (the second of three intervals, the middle one across the
    chunk boundary), and a filler that makes the batch large enough for chunks of full size."""
    a_iv = [(1000, 1000 + K16)]
    b_len = [10752, 11264, 2 * K16 - 1 - 22016]                       # interval boundaries half way between multiples of 1 024
    b_iv, s = [], 5000
    for n in b_len:
        b_iv.append((s, s + n - 1)); s += n + 50
    n_fill = 512 * K16 // 4
    f_iv = [(100 + i * (n_fill + 10), 100 + i * (n_fill + 10) + n_fill - 1) for i in range(4)]
    filler = [[(a + 5, a + 90), (a + 100, a + 400), (a + 1000, b - 7)] for a, b in f_iv] + [[(f_iv[0][0] + 7, f_iv[0][0] + 300)]]
    parts = [hand(a_iv, edge_reads(1000, K16 + 1, a_iv)), hand(b_iv, edge_reads(5000, 2 * K16 - 1, b_iv)), hand(f_iv, filler)]
    return parts, ENDS


def odd_start():
    """The first partition holds an odd number of positions: the second one's p0 is odd; hits on its first and last position."""
    first = hand([(1000, 1400)], [A, B])                              # 401 positions
    second = hand([(2000, 2399)], [[(2000, 2399)], shifted([A], 1000)[0], [(2000, 2100), (2150, 2399)]])
    return [first, second], ENDS


def uncached():
    """More than kHistIv (1 024) short intervals in one partition: the interval search in device memory."""
    ivs = [(1000 + 12 * k, 1000 + 12 * k + 8) for k in range(1100)]
    rng = np.random.default_rng(5)
    reads = []
    for _ in range(40):
        ks = np.sort(rng.choice(1100, 6, replace=False))
        reads.append([(ivs[k][0] + int(rng.integers(0, 4)), ivs[k][1] - int(rng.integers(0, 4))) for k in ks])
    return [hand(ivs, reads)], {}


def ends(ignore):
    one = [(1010, 1390)]
    return [hand([(1000, 1399)], [one, A, B, one, C])], dict(ignore_ends=ignore)


def many_small():
    """64 partitions of 8 reads and one without a hit (single-exon reads under ignore_ends)."""
    parts = [util.make_partition(7000 + i, n_reads=8, n_exons=5 + i % 4, max_span=0) for i in range(64)]
    parts.insert(31, hand([(1000, 1200)], [[(1010, 1190)], [(1020, 1180)]]))
    return parts, {}


CASES = {
    "neighbours": (neighbours, 1), "bound-65535": (lambda: bound(65535), 1), "bound-65536": (lambda: bound(65536), 0),
    "chunk-edges": (chunk_edges, 1), "odd-start": (odd_start, 1), "uncached-intervals": (uncached, 1),
    "ends-ignored": (lambda: ends(True), 1), "ends-counted": (lambda: ends(False), 1), "many-small": (many_small, 1),
}


@functools.lru_cache(maxsize=None)
def case(name):
    parts, params = CASES[name][0]()
    return parts, params, [util.run_oracle(p, params) for p in parts]


@pytest.mark.parametrize("hist16", ["0", "1"])
@pytest.mark.parametrize("name", list(CASES))
def test_packed_histogram(name, hist16, monkeypatch):
    monkeypatch.setenv("FSEG_HIST16", hist16)
    parts, params, oracles = case(name)
    ctx = _lib.Context(0)
    try:
        util.run_gpu(ctx, parts, params)
        # 1 asks for the packed instance and is ignored where a count could pass 65 535
        assert ctx.paths()["hist16"] == (CASES[name][1] if hist16 == "1" else 0), ctx.paths()
        y_raw = ctx.tap("y_raw").copy()
        util.compare_partitions(ctx, parts, oracles)
        if name.startswith("bound"):
            w = int(parts[0].rep_weight[0])
            assert y_raw[100] == w and y_raw[101] == 1 and y_raw[60] == w and y_raw[70] == 1, y_raw[[60, 70, 100, 101]]
        if name == "many-small":
            p0 = ctx.tap("pos_off")[sum(len(p.iv_start) for p in parts[:31])]
            assert not y_raw[p0:p0 + 201].any()
        ctx.run(); ctx.sync()                                          # the replay (the captured launch)
        assert np.array_equal(ctx.tap("y_raw"), y_raw)
    finally:
        ctx.close()


def test_default_is_packed(monkeypatch):
    monkeypatch.delenv("FSEG_HIST16", raising=False)
    parts, params, oracles = case("neighbours")
    ctx = _lib.Context(0)
    try:
        util.run_gpu(ctx, parts, params)
        assert ctx.paths()["hist16"] == 1
        util.compare_partitions(ctx, parts, oracles)
    finally:
        ctx.close()
