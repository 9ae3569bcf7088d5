"""The hand-built cases of tests/edge_cases.py under the CPU oracle alone: every case reaches the edge it is named after (candidate
counts, plateau midpoints, segment lengths, column counts, both outcomes of every boundary sweep), and the reference raises only
where a refusal is the case.  What tests/test_gpu_front_edges.py and tests/test_gpu_tail_edges.py compare the device with."""
import math

import numpy as np
import pytest

import edge_cases as ec


def interval(o, k, what="cands", off="cand_off"):
    return o[what][o[off][k]:o[off][k + 1]]


def chosen(o, k=0):
    return interval(o, k)[interval(o, k, "finalc", "finalc_off")]


@pytest.mark.parametrize("odd_first", [False, True])
@pytest.mark.parametrize("sigma", ec.PLATEAU_SIGMAS)
def test_plateaus_lie_where_they_are_named(sigma, odd_first):
    names, parts, _ = ec.case("plateau", sigma, odd_first)
    k = int(odd_first)
    for name, part, o in zip(names, parts, ec.oracles("plateau", sigma, odd_first)):
        assert o["error"] == 0, (name, o["errmsg"])
        assert (o["pos_off"][k] & 31 != 0) == odd_first and part.iv_end[k] - part.iv_start[k] + 1 == ec.PLATEAU_LEN
        c, y = interval(o, k), interval(o, k, "Y", "pos_off")
        if name == "twins":
            twins = ec.twins_in_one_quad(o, k)
            assert twins and all(m in c for pair in twins for m in pair), name
            continue
        p, n = ec.PLATEAUS[name]
        assert (y[p:p + n] == y[p]).all() and y[p - 1] < y[p], name
        if name == "to-last-position":
            assert p + n == len(y) and list(c) == [0, len(y) - 1]             # level up to the last position: no peak (scipy)
        else:
            assert y[p + n] < y[p] and list(c) == [0, ec.plateau_midpoint(name), len(y) - 1], (name, c)
    at = {n: ec.PLATEAUS[n] for n in ec.PLATEAUS}
    assert at["cross-511-512"][0] < 511 < 512 < sum(at["cross-511-512"]) and sum(at["end-511"]) - 1 == 511
    assert at["longer-than-512"][1] > 512 and at["longer-than-1024"][1] > 1024 + 512 - at["longer-than-1024"][0] % 512   # past a whole tile


def test_radius_zero_twins():
    o = ec.oracles("twins0")[0]
    twins = ec.twins_in_one_quad(o, 0)
    assert o["error"] == 0 and twins and all(m in interval(o, 0) for pair in twins for m in pair)


@pytest.mark.parametrize("sigma", ec.PLATEAU_SIGMAS)
def test_interval_lengths(sigma):
    names, parts, _ = ec.case("length", sigma)
    r = ec.RADIUS[sigma]
    assert [int(p.iv_end[0] - p.iv_start[0] + 1) for p in parts] == [2, 3, 4, 5, r - 1, r, r + 1, 511, 512, 513, 1023, 1025]
    for name, part, o in zip(names, parts, ec.oracles("length", sigma)):
        L = int(part.iv_end[0] - part.iv_start[0] + 1)
        assert o["error"] == 0, (name, o["errmsg"])
        raw = interval(o, 0, "Y_raw", "pos_off")
        assert sorted(np.flatnonzero(raw)) == sorted({q for q in (0, 1, L - 2, L - 1) if 0 <= q < L}), name    # (ends counted: 0 is every rep's start)
        assert {0, L - 1} <= set(interval(o, 0).tolist())


@pytest.mark.parametrize("threads", [64, 256, 1024])
def test_candidate_counts_gaps_and_block_sizes(threads):
    names, parts, _ = ec.case("width", threads, 1000)
    gaps, empty_chunk, back = set(), False, {}
    for name, part, o in zip(names, parts, ec.oracles("width", threads, 1000)):
        n = int(name.split("-")[1])
        L = int(part.iv_end[0] - part.iv_start[0] + 1)
        assert o["error"] == 0 and len(part.iv_start) == 1 and len(o["cands"]) == n, (name, o["errmsg"], len(o["cands"]))
        assert (64 if L <= 16384 else 256 if L <= 65536 else 1024) == threads           # the host's rule for the block size
        fc = o["finalc"]
        assert np.array_equal(fc, o["fixed"])                                           # the DP adds nothing
        gaps |= set(np.diff(fc).tolist())
        # positions refinement adds: every spike's, and only if k_segments names the right previous chosen candidate for its segment
        c = o["cands"]
        added = ec.refined(o)
        assert sorted(y for _, _, y in added) == [ec.STEP * r for r in ec.spike_ranks(n, name[-1])], (name, added)
        for a, b, y in added:                        # how far back the previous chosen candidate lies: in chunks of 64, in steps of the block
            ra, rb = int(np.searchsorted(c, a)), int(np.searchsorted(c, b))
            back.setdefault(n, set()).add((rb // 64 - ra // 64, rb // threads - ra // threads))
        if n <= 256:                                                                    # (the one-wave path of k_segments at 64 threads)
            empty_chunk |= any(not ((fc >= u) & (fc < u + 64)).any() and (fc < u).any() and (fc >= u + 64).any() for u in range(0, n, 64))
    assert {1, 63, 64, 65} <= gaps and empty_chunk
    for n in (255, 256, 257):                        # refined segments whose previous chosen candidate is in the same chunk, one back, more back
        assert {0, 1} <= {ch for ch, _ in back[n]} and max(ch for ch, _ in back[n]) >= 2, (n, back[n])
    for n in ec.COUNTS:
        # ... in an earlier step of the multi-wave loop (not 257 at 256 threads: candidate 256 is the interval's end, 49 behind the sink)
        if n in back and threads + 1 < n and (threads > 64 or n > 256):
            assert any(st >= 1 for _, st in back[n]), (n, back[n])
    if threads > 64:
        assert 130 in gaps and max(gaps) > 256 and any(n.startswith("cand-1100") for n in names)
    assert [n for n in ec.COUNTS if n > threads] or threads == 1024                     # more candidates than threads
    for mps in (5, 50, 100):
        for name, o, o0 in zip(names, ec.oracles("width", threads, mps), ec.oracles("width", threads, 1000)):
            assert o["error"] == 0, (name, mps, o["errmsg"])
            assert len(o["fixed"]) >= len(o0["fixed"]) and (mps > 5 or len(o["fixed"]) > len(o0["fixed"]))
    # layout b under max_problem_size 5: the first oversized pair is (0, 7); its anchor's window starts at index -1
    size = 8; cnt = math.ceil(size / 5)
    assert int(0 + 1 * (size / cnt)) - 5 == -1 and ec.heavy_ranks(300, "b")[0] == 7
    o = ec.oracles("refusal", threads)[0]
    assert o["error"] != 0 and "negative anchor" in o["errmsg"]


@pytest.mark.parametrize("length", ec.INNER_LENS)
def test_inner_sum_sweeps_straddle_the_edge(length):
    names, parts, _ = ec.case("inner", length)
    got = {}
    for name, part, o in zip(names, parts, ec.oracles("inner", length)):
        P0 = int(name.split("-")[1])
        assert o["error"] == 0, (name, o["errmsg"])
        assert list(chosen(o)) == [0, P0, P0 + length, P0 + length + 59], (name, chosen(o))
        got[name] = [y - P0 for a, b, y in ec.refined(o) if (a, b) == (P0, P0 + length)]
    for P0 in ec.INNER_P0:
        for side in "ab":
            sweep = [bool(got["P0-%d-%s-w25-d%+d" % (P0, side, d)]) for d in ec.INNER_D]
            assert True in sweep and False in sweep, (P0, side, sweep)
            edge = 20 if side == "a" else length - 21
            assert got["P0-%d-%s-w25-d+0" % (P0, side)] == [edge] and not got["P0-%d-%s-w25-d-1" % (P0, side)]
            assert not got["P0-%d-%s-split-19-1" % (P0, side)] and not got["P0-%d-%s-w19" % (P0, side)]
    assert [(P0 + 20) % 16 == 0 for P0 in ec.INNER_P0] == [True, True, True, False]
    assert [(P0 + 20) % 512 == 0 for P0 in ec.INNER_P0] == [False, True, True, False]
    if length == max(ec.INNER_LENS):
        assert all(((P0 + length - 21) >> 9) - ((P0 + 20) >> 9) > 64 for P0 in ec.INNER_P0)      # k_segments leaves the sum to k_refine


@pytest.mark.parametrize("sigma", list(ec.REFINE_SIGMAS))
def test_refinement_reaches_both_paths(sigma):
    names, parts, _ = ec.case("refine", sigma)
    added = {}
    for name, o in zip(names, ec.oracles("refine", sigma)):
        assert o["error"] == 0, (name, o["errmsg"])
        added[name] = ec.refined(o)
        assert added[name], name
    lens = {n: {b - a for a, b, _ in v} for n, v in added.items()}
    if sigma != "sigma50":                           # (under radius 200 the heavy junctions' candidates lie elsewhere)
        assert lens["len-1025"] == {1025} and lens["len-1024"] == {1024} and len(added["len-1025"]) == 3 and len(added["len-1024"]) == 3
    for n in ("tie-1500", "flat-3200", "apart-19", "apart-20", "apart-21"):
        assert min(lens[n]) > ec.REF_CAP, (n, lens[n])                                   # scratch in global memory
    for n in ("tie-900", "flat-900", "apart-20-lds"):
        assert max(lens[n]) <= ec.REF_CAP, (n, lens[n])
    assert len(added["tie-1500"]) == 1 and len(added["tie-900"]) == 1                   # two equal clusters 10 apart: one peak
    if sigma != "sigma50":
        assert len(added["apart-19"]) == 2 and len(added["apart-20"]) == 4 and len(added["apart-21"]) == 4      # distance = 20


@pytest.mark.parametrize("rate", [0.9, 1.0])
@pytest.mark.parametrize("S", ec.LABEL_COLS)
def test_label_partitions_have_the_columns_and_reads(S, rate):
    names, parts, _ = ec.case("label", S, rate)
    for n_reps, part, o in zip(ec.LABEL_REPS, parts, ec.oracles("label", S, rate)):
        assert o["error"] == 0, (n_reps, o["errmsg"])
        fp = o["final_pos"]
        assert len(fp) - 1 == S and part.n_reps == n_reps and o["labels"].shape == (n_reps, S)
        if n_reps < 63:
            continue
        sent = int(o["final_off"][1]) - 1                                                # the sentinel column between the intervals
        first, last = part.ex_ts[part.rep_exon_off[:-1]], part.ex_te[part.rep_exon_off[1:] - 1]
        lo, hi = np.searchsorted(fp, first, "right") - 1, np.searchsorted(fp, last, "right") - 1
        single = np.diff(part.rep_exon_off) == 1
        assert {1, 2, 3, 4, 5} <= set((hi - lo + 1)[single].tolist())                    # columns a read reaches
        assert ((lo < sent) & (hi > sent))[1:].any()                                     # a read across the sentinel (rep 0 is the backbone)
        inner = fp[1:-1]
        for d in (-1, 0):                                                                # reads ending on g - 1 and on g, starting on them
            assert np.isin(last[single] - d, inner).any() and np.isin(first[single] - d, inner).any()
    assert (S <= ec.LABEL_STAGE) == (S in (1023, 1024))                              # the column table in LDS / in global memory
    assert (S % 16 != 0) == (S != 1024)                                              # rows share packed words unless S is a multiple of 16
    assert set(np.unique(ec.oracles("label", S, rate)[-1]["labels"]).tolist()) == {0, 1, 2}
