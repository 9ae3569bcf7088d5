"""S4 and S6 by candidates -- k_fix_cand and k_segments_cand (csrc/seg_problems.hip, seg_tail.hip), a thread per candidate, chosen under
FSEG_IV_CAND=1 wherever iv_threads is 64 -- at the sizes where their code takes another branch.  A workgroup owns OWN consecutive
candidates of the batch and stages HALO in front of them (kIvCandOwn, kIvCandHalo: read from seg_common.h, so the shapes follow the
code); the batches here put intervals of chosen sizes at chosen places of the batch's candidate list, filler intervals of two and three
candidates between them:

  boundary   intervals of 2, 3, 50 and 64 candidates that start 1, N / 2 and N - 1 candidates in front of a multiple of OWN (and one on
             it), a heavy junction behind the split: its problem's size is the distance to a flag that only the halo holds
  long50 / long1000   short against long: 50 | 51 candidates under max_problem_size 50, 64 | 65 under 1000; two long intervals in one
             owned run, one whose candidate 0 is the run's first candidate, one whose candidate 0 is its last
  width      edge_cases' width intervals (63 .. 300 candidates, and 1 100: more than two owned runs) across the runs' edges
  lookback   layout "a" with the candidate behind a gap of 63 / 64 / 65 chosen candidates as the first owned one of a run -- the
             predecessor inside the halo, on its first candidate, one beyond it -- and 1 100 candidates with gaps of 130 and 257
  inner      edge_cases' inner-sum cases behind enough filler for iv_threads 64, under both histogram widths
  ends       candidate counts of a multiple of OWN, of one more, and the smallest batch there is

Every batch is checked as edge_cases.run_on_gpu checks its own (run_case: the census word iv_cand beside the others): every tap against
the CPU oracle on the first run and on the replay.
test_shapes_reach_their_edges needs no device: it shows by the oracle's cand_off that the batches have the shapes named here."""
import functools
import os
import re

import numpy as np
import pytest

import edge_cases as ec
import lane_cases as lc
import util
from freddie_amd import synth

gpu = pytest.mark.gpu

_SRC = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "freddie_amd", "csrc", "seg_common.h")).read()
OWN, HALO = map(int, re.search(r"constexpr int kIvCandOwn = (\d+), kIvCandHalo = (\d+)", _SRC).groups())
FROM = int(re.search(r"constexpr long long kIvCandFrom = (\d+)", _SRC).group(1))
STEP = ec.STEP


# ---- builders: candidate counts are known by construction (and checked against the oracle by the host test) ----------------------
def interval_part(n_cand, heavy=(), spikes=()):
    """[interval of n_cand >= 3 candidates, sink of 3]: its two ends and n_cand - 2 junctions STEP apart, of weight 400 (ranks
    `heavy`), 25 (`spikes`) or 3."""
    nj = n_cand - 2
    assert nj >= 1
    w = [400 if i + 1 in heavy else 25 if i + 1 in spikes else 3 for i in range(nj)]
    return ec.single(STEP * (nj + 1) + 40, [STEP * (i + 1) for i in range(nj)], w)


def small_part(kinds, weights=(3, 400, 30)):
    """A partition of intervals of two (no junction) and three (one junction) candidates, `kinds` in order, and the sink (3)."""
    ivs, s = [], ec.S0
    for n in kinds:
        ivs.append((s, s + (59 if n == 2 else 99)))
        s = ivs[-1][1] + 101
    sink = (s + 100, s + 199)
    reads, w = [], []
    for i, (iv, n) in enumerate(zip(ivs, kinds)):
        if n == 3:
            r, ww = util.junction_reads(iv, [50], [weights[i % len(weights)]], sink)
            reads += r; w += ww
    return util.hand(ivs + [sink], reads, w)


@functools.lru_cache(maxsize=None)
def filler(n):
    """n candidates in intervals of two and three (about as many of each) and the sink."""
    rest = n - 3
    b = max(1, rest // 5)
    b += (b - rest) % 2
    assert rest >= 3 and 3 * b <= rest, n
    a = (rest - 3 * b) // 2
    kinds = [3, 2] * min(a, b) + [3] * (b - min(a, b)) + [2] * (a - min(a, b))
    return small_part(tuple(kinds))


class Layout:
    """Partitions in batch order with the candidate index each starts at; place(part, at) fills up to candidate `at` first."""

    def __init__(self):
        self.names, self.parts, self.n, self.k, self.marks = [], [], 0, 0, {}

    def add(self, name, part, n_cand, n_iv, mark=None):
        if mark:
            self.marks[mark] = (self.k, self.n)              # (batch interval, batch candidate) of the partition's first interval
        self.names.append(name); self.parts.append(part); self.n += n_cand; self.k += n_iv

    def fill(self, n):
        if n:
            p = filler(n)
            self.add("fill-%d" % n, p, n, len(p.iv_start))

    def place(self, name, part, n_cand, n_iv, at):
        while at - self.n < 8 and at != self.n:
            at += OWN
        self.fill(at - self.n)
        self.add(name, part, n_cand, n_iv, mark=name)

    def next_multiple(self, room=8):
        return (self.n + room + OWN - 1) // OWN * OWN


def splits(N):
    return sorted({1, N // 2, N - 1} - {0})


def boundary_layout():
    L = Layout()
    for N in (2, 3, 50, 64):
        for s in splits(N):
            if N == 2:
                part, nc, ni = small_part((2, 3)), 8, 3
            else:
                h = min(N - 2, max(s, N // 2))              # a heavy junction behind the split (N - 1 in front: the last candidate is)
                part, nc, ni = interval_part(N, heavy={h}), N + 3, 2
            L.place("N%d-s%d" % (N, s), part, nc, ni, L.next_multiple(s + 8) - s)
    L.place("N50-s0", interval_part(50, heavy={30}), 53, 2, L.next_multiple())
    L.fill(40)
    return L, dict(ec.WIDTH_PARAMS, max_problem_size=1000)


def long_layout(mps):
    short_n, long_n = (50, 51) if mps == 50 else (64, 65)
    L = Layout()
    L.fill(100)
    L.add("short", interval_part(short_n), short_n + 3, 2, mark="short")
    L.fill(20)
    L.add("long", interval_part(long_n), long_n + 3, 2, mark="long")
    m = L.next_multiple()
    L.place("long-first-owned", interval_part(long_n), long_n + 3, 2, m)
    L.place("long-pair-a", interval_part(long_n), long_n + 3, 2, m + 100)
    L.place("long-pair-b", interval_part(long_n + 2), long_n + 5, 2, m + 200)
    L.place("long-last-owned", interval_part(long_n), long_n + 3, 2, m + 2 * OWN - 1)
    L.fill(30)
    return L, dict(ec.WIDTH_PARAMS, max_problem_size=mps)


WIDTH_COUNTS = [n for n in ec.COUNTS if n <= 300] + [1100]


def width_layout(mps):
    L = Layout()
    for n in WIDTH_COUNTS:
        for lay in "ab":
            # (an interval of n candidates: its ends, n - 3 junctions and the sink's peak)
            L.place("cand-%d-%s" % (n, lay), ec.width_part(n, 64, lay), n, 1, L.next_multiple(n // 3 + 8) - n // 3)
    L.fill(50)
    return L, dict(ec.WIDTH_PARAMS, max_problem_size=mps)


LOOKBACK_RANKS = {63: 65, 64: 129, 65: 194}            # gap -> the rank of layout "a" behind it (heavy_ranks: 1, 2, 65, 129, 194, 324, 581)


def lookback_layout():
    L = Layout()
    for gap, rank in LOOKBACK_RANKS.items():
        L.place("gap-%d" % gap, ec.width_part(300, 64, "a"), 300, 1, L.next_multiple(rank + 8) - rank)
    L.place("gaps-130-257", ec.width_part(1100, 64, "a"), 1100, 1, L.next_multiple(8) - 5)
    L.fill(30)
    return L, dict(ec.WIDTH_PARAMS, max_problem_size=1000)


def inner_layout(length):
    names, parts, params = ec.inner_case(length)
    L = Layout()
    L.fill(OWN - 7)
    for n, p in zip(names, parts):
        L.add(n, p, 0, 2)                                 # (candidate counts not tracked: the spikes may add candidates)
    f = filler(1003)                                      # 400 intervals: the batch's average interval stays far below 16 384 positions
    L.add("fill-1003", f, 1003, len(f.iv_start))
    return L, params


def ends_layout(extra):
    L = Layout()
    L.fill(2 * OWN + extra)
    return L, dict(ec.WIDTH_PARAMS)


def smallest_layout():
    """One interval, two candidates: a read that covers it as one exon counts nothing under ignore_ends."""
    L = Layout()
    L.add("one-interval", lc.single([ec.S0], [ec.S0 + 199]), 2, 1)
    return L, dict(ec.WIDTH_PARAMS)


LAYOUTS = dict(boundary=boundary_layout, long=long_layout, width=width_layout, lookback=lookback_layout, inner=inner_layout,
               ends=ends_layout, smallest=smallest_layout)


@functools.lru_cache(maxsize=None)
def layout(kind, *key):
    return LAYOUTS[kind](*key)


def iv_cand_case(kind, *key):
    L, params = layout(kind, *key)
    return L.names, L.parts, params


ec.CASES["iv_cand"] = iv_cand_case                     # edge_cases.case / oracles / run_on_gpu take the batches by this name


def batch_cand_off(kind, *key):
    """cand_off of the whole batch (and every candidate's fixed / chosen flag) from the partitions' oracles."""
    off, fixed, chosen = [0], [], []
    for o in ec.oracles("iv_cand", kind, *key):
        assert o["error"] == 0, o["errmsg"]
        n = int(o["cand_off"][-1])
        fx, ch = np.zeros(n, bool), np.zeros(n, bool)
        for k in range(len(o["cand_off"]) - 1):
            fx[o["cand_off"][k] + o["fixed"][o["fixed_off"][k]:o["fixed_off"][k + 1]]] = True
            ch[o["cand_off"][k] + o["finalc"][o["finalc_off"][k]:o["finalc_off"][k + 1]]] = True
        off += (off[-1] + o["cand_off"][1:]).tolist()
        fixed.append(fx); chosen.append(ch)
    return np.array(off), np.concatenate(fixed), np.concatenate(chosen)


# ---- the host's view: the batches have the shapes they are named after -------------------------------------------------------------
def test_shapes_reach_their_edges():
    # boundary: every named interval has its N candidates, starts s in front of a multiple of OWN, and the candidate behind the split
    # that is fixed has its previous fixed candidate in front of the split
    L, _ = layout("boundary")
    off, fixed, _ = batch_cand_off("boundary")
    assert off[-1] == L.n
    for name, (k, g) in L.marks.items():
        N, s = (int(x[1:]) for x in name.split("-"))
        assert off[k] == g and off[k + 1] - off[k] == N and (g + s) % OWN == 0, (name, off[k], g)
        if N > 2 and 0 < s < N - 1:
            right = [c for c in range(s, N) if fixed[g + c]]
            assert right and not fixed[g + 1:g + s].any(), name      # its problem reaches back to candidate 0, in the halo
    # short against long
    for mps, (short_n, long_n) in ((50, (50, 51)), (1000, (64, 65))):
        L, _ = layout("long", mps)
        off, _, _ = batch_cand_off("long", mps)
        k, g = L.marks["short"]; assert off[k] == g and off[k + 1] - g == short_n
        k, g = L.marks["long"]; assert off[k] == g and off[k + 1] - g == long_n
        k, g = L.marks["long-first-owned"]; assert off[k] == g and g % OWN == 0 and off[k + 1] - g == long_n
        k, g = L.marks["long-last-owned"]; assert off[k] == g and g % OWN == OWN - 1 and off[k + 1] - g == long_n
        (ka, ga), (kb, gb) = L.marks["long-pair-a"], L.marks["long-pair-b"]
        assert off[ka] == ga and off[kb] == gb and ga // OWN == gb // OWN and off[ka + 1] - ga > min(mps, 64) and off[kb + 1] - gb > min(mps, 64)
    # width: every interval lies across an edge of the owned runs, the 1 100 across more than two runs
    L, _ = layout("width", 1000)
    off, _, _ = batch_cand_off("width", 1000)
    for name, (k, g) in L.marks.items():
        n = int(name.split("-")[1])
        assert off[k] == g and off[k + 1] - g == n and g // OWN < (g + n - 1) // OWN, name
        if n == 1100:
            assert (g + n - 1) // OWN - g // OWN >= 2
    # lookback: the chosen candidate behind a gap of 63 / 64 / 65 is the first owned candidate of a run; 130 and 257 occur
    L, _ = layout("lookback")
    off, _, chosen = batch_cand_off("lookback")
    for gap, rank in LOOKBACK_RANKS.items():
        k, g = L.marks["gap-%d" % gap]
        assert off[k] == g and (g + rank) % OWN == 0 and chosen[g + rank] and chosen[g + rank - gap] and not chosen[g + rank - gap + 1:g + rank].any()
    k, g = L.marks["gaps-130-257"]
    gaps = np.diff(np.flatnonzero(chosen[g:off[k + 1]]))
    assert {63, 64, 65, 130, 257} <= set(gaps.tolist())
    # ends
    for extra in (0, 1):
        off, _, _ = batch_cand_off("ends", extra)
        assert off[-1] % OWN == extra and off[-1] > OWN
    off, _, _ = batch_cand_off("smallest")
    assert off.tolist() == [0, 2]


# ---- the device ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def cand_on(monkeypatch):
    monkeypatch.setenv("FSEG_IV_CAND", "1")
    monkeypatch.delenv("FSEG_YRAW16", raising=False)
    return monkeypatch


def run_case(*key, iv_cand=1, **words):
    """edge_cases.run_on_gpu with the census word iv_cand beside the others: the batch on a fresh context (fseg_create reads the
    switches), every tap against the oracles on the first run and on the replay, the smoothed signal bit-identical."""
    from freddie_amd import _lib
    names, parts, params = ec.case("iv_cand", *key)
    want = ec.oracles("iv_cand", *key)
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
            for word, v in dict(words, iv_cand=iv_cand, iv_threads=64).items():
                assert census[word] == v, (run, word, census[word], v)
    finally:
        ctx.close()


def census_of(parts, params):
    from freddie_amd import _lib
    ctx = _lib.Context(0)
    try:
        util.run_gpu(ctx, parts, params)
        return ctx.paths()
    finally:
        ctx.close()


@gpu
def test_intervals_across_the_owned_runs_edges(cand_on):
    run_case("boundary", smooth_r=20)


@gpu
@pytest.mark.parametrize("mps", [50, 1000])
def test_short_against_long(cand_on, mps):
    run_case("long", mps, smooth_r=20)


@gpu
@pytest.mark.parametrize("mps", ec.WIDTH_MPS)
def test_width_cases_across_the_runs(cand_on, mps):
    run_case("width", mps, smooth_r=20)


@gpu
def test_look_back_inside_on_and_beyond_the_halo(cand_on):
    run_case("lookback", smooth_r=20)


@gpu
@pytest.mark.parametrize("yraw16", ["0", "1"])
@pytest.mark.parametrize("length", [41, 1025, 512 * 66 + 100])
def test_inner_sums_of_both_instances(cand_on, length, yraw16):
    cand_on.setenv("FSEG_YRAW16", yraw16)
    run_case("inner", length, yraw16=int(yraw16))


@gpu
def test_refusal_keeps_its_code(monkeypatch):
    from freddie_amd import _lib
    names, parts, params = ec.case("refusal", 64)
    codes = {}
    for sw in ("0", "1"):
        monkeypatch.setenv("FSEG_IV_CAND", sw)
        ctx = _lib.Context(0)
        try:
            with pytest.raises(_lib.SegError, match="break_large_problems") as e:
                util.run_gpu(ctx, parts, params)
                ctx.download()
            codes[sw] = (e.value.code, str(e.value))
        finally:
            ctx.close()
    assert codes["1"] == codes["0"] and codes["1"][0] == _lib.ERR_INPUT, codes


@gpu
@pytest.mark.parametrize("which", ["multiple", "multiple+1", "smallest"])
def test_ends_of_the_candidate_list(cand_on, which):
    if which == "smallest":
        run_case("smallest")
    else:
        run_case("ends", 0 if which == "multiple" else 1)


@functools.lru_cache(maxsize=None)
def config4_small():
    kw = dict(synth.WORKLOADS["config4"]); kw.pop("n_partitions")
    parts = [util.make_partition(i, **kw) for i in range(64)]
    return parts, [util.run_oracle(p) for p in parts]


@gpu
def test_a_real_shape_small(monkeypatch):
    """64 partitions of the config4 generator: against the oracle under FSEG_IV_CAND=1, and tap for tap against FSEG_IV_CAND=0."""
    from freddie_amd import _lib
    parts, want = config4_small()
    taps = {}
    for sw in ("1", "0"):
        monkeypatch.setenv("FSEG_IV_CAND", sw)
        ctx = _lib.Context(0)
        try:
            util.run_gpu(ctx, parts)
            census = ctx.paths()
            assert census["iv_cand"] == int(sw) and census["iv_threads"] == 64, census
            if sw == "1":
                util.compare_partitions(ctx, parts, want)
            taps[sw] = {k: ctx.tap(k).copy() for k in ("fixed", "chosen", "problems", "final_y")}
        finally:
            ctx.close()
    for k in taps["1"]:
        assert np.array_equal(taps["1"][k], taps["0"][k]), k


@gpu
def test_census(monkeypatch):
    names, parts, params = ec.case("iv_cand", "ends", 1)
    monkeypatch.setenv("FSEG_IV_CAND", "1")
    census = census_of(parts, params)
    assert census["iv_cand"] == 1 and census["iv_threads"] == 64, census
    # a batch of long intervals (iv_threads 256) keeps the kernels by intervals whatever the switch says
    wn, wparts, wparams = ec.case("width", 256, 1000)
    census = census_of(wparts[:2], wparams)
    assert census["iv_cand"] == 0 and census["iv_threads"] == 256, census
    # the switch unset: the size rule
    monkeypatch.delenv("FSEG_IV_CAND")
    census = census_of(parts, params)
    K = sum(len(p.iv_start) for p in parts)
    assert census["iv_cand"] == int(K >= FROM) and census["iv_threads"] == 64, census
    if FROM > 1:
        one = parts[:1]
        census = census_of(one, params)
        assert census["iv_cand"] == int(len(one[0].iv_start) >= FROM), census
