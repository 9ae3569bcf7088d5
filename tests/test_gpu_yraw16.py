"""The S1 histogram as uint16 in device memory (FSEG_YRAW16, wherever k_hist<16> counts) against the int32 one and the CPU oracle,
through the C-ABI: the smallest shapes at which the narrow array can go wrong.  Every case runs under FSEG_YRAW16=1 and =0; the census
(the `paths` tap, word `yraw16`) says which width ran, Y_raw is compared with == between the two settings and against the oracle,
every later tap goes through util.compare_partitions, and a replay must leave the same Y_raw.

k_hist<16, uint16_t> copies its LDS words out sixteen bytes at a time; the sixteen-byte groups at a chunk's two ends, which may
hold a neighbouring chunk's positions (another workgroup's), leave as 2-byte stores.  A small batch runs chunks of 1 024 positions
(the chunk size is halved while the batch has fewer than 512 chunks), so chunk edges lie at every multiple of 1 024 positions of a
partition and p0, a chunk's first position in the batch, is whatever the partitions before it add up to.  The readers (k_smooth,
k_segments, k_refine) must zero-extend: 65 535 read as a signed short is -1.

An interval of one position is refused on upload (start < end, as the reference asserts: test_gpu_front_edges), and an exon needs
start < end as well, so the shortest interval and the shortest partition here have two positions.  With ignore_ends=False every
read counts, so the partitions without any hit are a batch of their own (the same sizes, the ends ignored), run on the context
that has just held the counted batch: freshly allocated memory is zero anyway."""
import functools

import numpy as np
import pytest

import edge_cases as ec
import util
from freddie_amd import _lib

pytestmark = pytest.mark.gpu

ENDS = dict(ignore_ends=False)
hand, shifted = util.hand, util.shifted

# test_gpu_hist_packed's reads: under ignore_ends A counts on positions 49, 60, 100 (even), 200 of an interval that starts at 1000,
# B on 31, 70, 101 (odd: the other half of A's word), 210
A = [(1000, 1049), (1060, 1100), (1200, 1300)]
B = [(1002, 1031), (1070, 1101), (1210, 1320)]


def shared_word(first_len):
    """A first partition of first_len positions (odd: the second one's p0 is odd, and its first position shares a 32-bit word with
    the first one's last), counts on both of those positions, and inside the second partition counts on q - 1 and q for every
    multiple q of 1 024: the two sides of every chunk edge.  Every weight differs from its neighbour's."""
    e = 1000 + first_len - 1
    first = hand([(1000, e)], [[(1000, e)], [(1003, e)]], [3, 4])                  # 3 on position 0, 7 on the last, 4 on 3
    s, L = 2000, 3100
    reads, weights = [[(s, s + L - 1)], [(s, s + 10)]], [5, 6]                     # 11 on position 0, 5 on the last, 6 on 10
    for j, q in enumerate(range(1024, L, 1024)):
        reads += [[(s + q - 300, s + q - 1)], [(s + q, s + q + 20)]]
        weights += [20 + j, 30 + j]
    return [first, hand([(s, s + L - 1)], reads, weights)], ENDS


# (in this order the partitions' first positions take every one of the eight places of a sixteen-byte group, and so do their ends)
SIZES = (7, 2, 15, 9, 17, 1025, 3, 1023, 1031, 8)


def heads_and_tails(params):
    """Ten partitions of one interval each, a read over the whole of it and one from its second position to its last: under
    ignore_ends=False counts on every partition's first, second and last position; under ignore_ends=True no hit anywhere."""
    parts, s = [], 1000
    for i, n in enumerate(SIZES):
        reads, weights = [[(s, s + n - 1)]], [3 + i]
        if n >= 3:
            reads.append([(s + 1, s + n - 1)]); weights.append(40 + i)
        parts.append(hand([(s, s + n - 1)], reads, weights))
        s += n + 100
    return parts, params


def bound(w_even, w_odd):
    """One rep of w_even reads ends on an even position (100), one of w_odd reads on the odd position next to it (101)."""
    return [hand([(1000, 1399)], [A, B], [w_even, w_odd])], {}


REFLECT_LENGTHS = (2, 5, 13, 20, 21, 41, 1024 + 3)
SIGMAS = {"sigma5": (5.0, 20), "sigma3": (3.0, 12), "sigma2.5": (2.5, 0)}          # sigma, the k_smooth instance (census word smooth_r)


def reflect(sigma):
    """One partition whose intervals are shorter than, as long as and just longer than the radius 20 (reflect_index; one reflection;
    load_counts' fast branch and its left halo), and one of two tiles and three positions, each with counts on and next to both ends."""
    ivs, reads, weights, s = [], [], [], 1000
    for i, n in enumerate(REFLECT_LENGTHS):
        ivs.append((s, s + n - 1))
        for d in range(3):
            if s + d < s + n - 1 - d:
                reads.append([(s + d, s + n - 1 - d)]); weights.append(7 + 5 * d + i)
        s += n + 37
    return [hand(ivs, reads, weights)], dict(ENDS, sigma=SIGMAS[sigma][0])


INNER_LENGTHS = (200, 1024, 1025, 1100, 42, 41)
INNER_VARIANTS = ("w25-d+0", "w25-d-1", "w25-d+1", "split-19-1", "w19")


def consumers(seed):
    """What k_segments and k_refine read: sixteen generated partitions of a few dozen reads (counts up to a few dozen; every segment
    between chosen neighbours more than 40 positions apart has inner counts that add up to less than 20), one without a hit, and ten
    of edge_cases' hand-built segments between two heavy junctions -- 25, or 19, or 19 + 1 across the edge, on and next to the first
    and the last inner position -- so that refine_segmentation's `sum(i_vals) < 20` is true of some segments and false of others."""
    parts = [util.make_partition(9000 + 16 * seed + i, n_reads=24 + 4 * (i % 5), n_exons=10 + i % 7) for i in range(16)]
    parts.insert(5, hand([(1000, 1200)], [[(1010, 1190)], [(1020, 1180)]]))
    P0, length = ec.INNER_P0[seed % 4] + seed // 4, INNER_LENGTHS[seed]
    for side in "ab":
        v = ec.inner_variants(length, side)
        parts += [ec.segment_part(P0, length, *v[n]) for n in INNER_VARIANTS]
    return parts, dict(ec.TAIL_PARAMS)


CASES = {
    "shared-word-odd": (lambda: shared_word(401), 1), "shared-word-even": (lambda: shared_word(400), 1),
    "heads-and-tails": (lambda: heads_and_tails(ENDS), 1), "heads-and-tails-no-hit": (lambda: heads_and_tails({}), 1),
    "unsigned-even": (lambda: bound(65535, 1), 1), "unsigned-odd": (lambda: bound(1, 65535), 1), "wide-65536": (lambda: bound(65536, 1), 0),
}
CASES.update({"reflect-" + k: (functools.partial(reflect, k), 1) for k in SIGMAS})
CASES.update({"consumers-%d" % seed: (functools.partial(consumers, seed), 1) for seed in range(6)})


@functools.lru_cache(maxsize=None)
def case(name):
    parts, params = CASES[name][0]()
    return parts, params, [util.run_oracle(p, params) for p in parts]


def check_run(ctx, name, yraw16):
    """One upload and run of the case on ctx, checked; the replay as well.  Returns Y_raw."""
    parts, params, oracles = case(name)
    packed = CASES[name][1]
    util.run_gpu(ctx, parts, params)
    census = ctx.paths()
    # 1 asks for uint16 and is ignored where the counters are not packed (a count could pass 65 535)
    assert census["hist16"] == packed and census["yraw16"] == (packed if yraw16 == "1" else 0), census
    y_raw = ctx.tap("y_raw").copy()
    assert y_raw.dtype == np.int32 and len(y_raw) == ctx.tap("pos_off")[-1]
    util.compare_partitions(ctx, parts, oracles)
    ctx.run(); ctx.sync()                                              # the replay (the captured launch)
    assert np.array_equal(ctx.tap("y_raw"), y_raw)
    return y_raw


def both_widths(name, monkeypatch):
    """The case under FSEG_YRAW16=1 and =0, a fresh context each (fseg_create reads the switch): the same Y_raw."""
    out = {}
    for yraw16 in ("1", "0"):
        monkeypatch.setenv("FSEG_YRAW16", yraw16)
        ctx = _lib.Context(0)
        try:
            out[yraw16] = check_run(ctx, name, yraw16)
            if name.startswith("reflect-"):
                assert ctx.paths()["smooth_r"] == SIGMAS[name[len("reflect-"):]][1], ctx.paths()
        finally:
            ctx.close()
    assert np.array_equal(out["1"], out["0"]), np.flatnonzero(out["1"] != out["0"])[:8]
    return out["1"]


@pytest.mark.parametrize("first_len", [401, 400])
def test_two_chunks_share_a_word(first_len, monkeypatch):
    y = both_widths("shared-word-odd" if first_len & 1 else "shared-word-even", monkeypatch)
    assert y[first_len - 1] == 7 and y[first_len] == 11, y[first_len - 2:first_len + 2]
    for j, q in enumerate((1024, 2048, 3072)):
        assert y[first_len + q - 1] == 20 + j and y[first_len + q] == 30 + j, (q, y[first_len + q - 2:first_len + q + 2])


def test_heads_and_tails(monkeypatch):
    y = both_widths("heads-and-tails", monkeypatch)
    p0 = np.cumsum((0,) + SIZES)
    assert len(set(int(p) & 7 for p in p0[:-1])) == 8 and len(set(int(p) & 7 for p in p0[1:])) == 8
    for i, n in enumerate(SIZES):
        first, last = (3 + i, 43 + 2 * i) if n >= 3 else (3 + i, 3 + i)
        assert y[p0[i]] == first and y[p0[i + 1] - 1] == last, (n, y[p0[i]:p0[i + 1]][:4], y[p0[i]:p0[i + 1]][-4:])


@pytest.mark.parametrize("yraw16", ["1", "0"])
def test_partitions_without_a_hit(yraw16, monkeypatch):
    """On a context whose histogram has just held heads-and-tails' counts on the very same positions: zeros must be written."""
    monkeypatch.setenv("FSEG_YRAW16", yraw16)
    ctx = _lib.Context(0)
    try:
        assert check_run(ctx, "heads-and-tails", yraw16).any()
        assert not check_run(ctx, "heads-and-tails-no-hit", yraw16).any()
    finally:
        ctx.close()


@pytest.mark.parametrize("name,even,odd", [("unsigned-even", 65535, 1), ("unsigned-odd", 1, 65535), ("wide-65536", 65536, 1)])
def test_counts_are_unsigned(name, even, odd, monkeypatch):
    """65 535 on one half of a word and 1 on the other, either way round, must come back as they are -- thresholds, candidates and
    finals (compare_partitions) are the oracle's only if the readers zero-extend; one read more and the batch is int32 throughout."""
    y = both_widths(name, monkeypatch)
    assert y[100] == even and y[101] == odd and y[60] == even and y[70] == odd, y[[60, 70, 100, 101]]


@pytest.mark.parametrize("sigma", list(SIGMAS))
def test_short_intervals_reflect(sigma, monkeypatch):
    both_widths("reflect-" + sigma, monkeypatch)


@pytest.mark.parametrize("seed", range(6))
def test_consumers(seed, monkeypatch):
    y = both_widths("consumers-%d" % seed, monkeypatch)
    parts, _, oracles = case("consumers-%d" % seed)
    added = [bool(ec.refined(o)) for o in oracles[17:]]                # the hand-built segments: refinement adds a position to some
    assert any(added) and not all(added), added
    p0 = sum(int((p.iv_end - p.iv_start + 1).sum()) for p in parts[:5])
    assert not y[p0:p0 + 201].any()


@pytest.mark.parametrize("yraw16", ["1", "0"])
def test_width_follows_the_batch(yraw16, monkeypatch):
    """One context: a packed batch, one whose count passes 65 535 (int32 whatever the switch says), the packed one again."""
    monkeypatch.setenv("FSEG_YRAW16", yraw16)
    ctx = _lib.Context(0)
    try:
        first = check_run(ctx, "shared-word-odd", yraw16)
        wide = check_run(ctx, "wide-65536", yraw16)
        assert wide[100] == 65536 and wide[101] == 1
        assert np.array_equal(check_run(ctx, "shared-word-odd", yraw16), first)
    finally:
        ctx.close()


def test_default_is_narrow(monkeypatch):
    monkeypatch.delenv("FSEG_YRAW16", raising=False)
    monkeypatch.delenv("FSEG_HIST16", raising=False)
    ctx = _lib.Context(0)
    try:
        check_run(ctx, "shared-word-odd", "1")
    finally:
        ctx.close()
