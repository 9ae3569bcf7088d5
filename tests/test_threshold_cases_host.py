"""The hand-built cases of tests/threshold_cases.py under the CPU oracle alone: every case reaches the count or the offsets it is
named after, the oracle's threshold is numpy's bit for bit, and every wrong summation order that differs from numpy's at that count
gives a threshold with other bits.  What tests/test_gpu_threshold_edges.py compares the device with."""
import warnings

import numpy as np
import pytest

import threshold_cases as tc
import util

CHUNK, GROUP = tc.CHUNK, tc.GROUP
FILLED = [("a",), ("c_big", "c1"), ("c_big", "c2"), ("c_many",)]         # the cases whose partitions are named after |V|


def numpy_threshold(v, vf):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                        # (mean of an empty slice: NaN, as the reference computes it)
        return float(v.mean() + vf * v.std())


def same_bits(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def named_count(name):
    return int(name.split("-")[1]) if name.startswith("m-") else None


@pytest.mark.parametrize("key", tc.ALL, ids=["-".join(k) for k in tc.ALL])
def test_the_oracle_is_numpy(key):
    names, parts, params = tc.case(*key)
    vf = dict(util.DEFAULTS, **params)["variance_factor"]
    for name, o in zip(names, tc.oracles(*key)):
        assert o["error"] == 0, (name, o["errmsg"])
        v = tc.values(o)
        assert o["n_vals"] == len(v)
        assert same_bits(o["threshold"], numpy_threshold(v, vf)), (name, o["threshold"], numpy_threshold(v, vf))
        if len(v) and len(v) <= 2 * CHUNK + 1:                 # ... and so is the plain-Python model the wrong orders are variants of
            assert tc.model_threshold(v, vf) == o["threshold"], name


@pytest.mark.parametrize("key", FILLED, ids=["-".join(k) for k in FILLED])
def test_counts_are_the_ones_named(key):
    names, parts, params = tc.case(*key)
    for name, part, o in zip(names, parts, tc.oracles(*key)):
        m = named_count(name)
        if m is not None:
            assert len(tc.values(o)) == m == int(o["pos_off"][-1]) and len(part.iv_start) == 1, (name, len(tc.values(o)))
        assert int(part.rep_weight.min()) >= 1 and int(part.rep_weight.max()) <= 60, name


def test_group_a_holds_every_tree_shape():
    names, parts, params = tc.case("a")
    ms = [named_count(n) for n in names]
    assert ms == sorted(ms) and len(ms) < 64                   # fewer than 64 partitions: the default takes the chunk kernels
    want = [2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 135, 136, 137, 255, 256, 257, 265, 1023, 1024, 1025, 4096, 8184, 8191,
            8192, 8193, 8199, 8200, 8192 + 128, 8192 + 129, 16383, 16384, 16385]
    assert ms == want
    o = tc.oracles("a")[0]                                     # two equal values: std == 0, the threshold is that value, nothing exceeds it
    y = o["Y"]
    assert y[0] == y[1] == o["threshold"] and np.array_equal(o["fixed"], [0, 1])         # (an interval's ends are fixed by rule, not by value)
    # the shapes the counts stand for (vsum_chunk): a lone leaf below 8, leaves with and without a tail, the general tree with a last
    # leaf of one to seven values as a chunk of its own, the perfect tree, two and three chunks
    last = {m: m - (m - 1) // CHUNK * CHUNK for m in ms}
    assert {last[8193], last[8199], last[8200], last[16385]} == {1, 7, 8, 1} and last[8192] == CHUNK and last[16384] == CHUNK
    # counts above 128 whose halves the rounding to a multiple of 8 moves somewhere in the recursion (129, 257, 1025 halve evenly)
    assert [m for m in ms if m > 128 and not tc.same_by_construction(m, "halves-unrounded")] == [135, 136, 137, 255, 265, 1023, 8184, 8191, 16383]
    assert [m for m in ms if not tc.same_by_construction(m, "chunks-right-to-left")] == [16385]


@pytest.mark.parametrize("key", FILLED, ids=["-".join(k) for k in FILLED])
def test_a_wrong_order_changes_the_threshold(key):
    """left to right; halves not rounded to a multiple of 8; leaves left to right; no chunks of 8 192; chunk sums right to left."""
    names, parts, params = tc.case(*key)
    for name, o in zip(names, tc.oracles(*key)):
        m = named_count(name)
        if m is None:
            continue
        hit, missed = tc.separated(tc.values(o), params["variance_factor"])
        assert set(missed) == {k for k in tc.MODELS if (m, k) in tc.UNSEPARATED}, (name, missed)
        for k in tc.MODELS:                                    # what agrees with numpy by construction: every order below 8 values, ...
            if tc.same_by_construction(m, k):
                assert tc.model_threshold(tc.values(o), params["variance_factor"], k) == o["threshold"], (name, k)
    assert tc.same_by_construction(7, "left-to-right") and not tc.same_by_construction(8, "left-to-right")
    assert tc.same_by_construction(256, "halves-unrounded") and not tc.same_by_construction(265, "halves-unrounded")
    assert tc.same_by_construction(2 * CHUNK, "unchunked") and not tc.same_by_construction(2 * CHUNK - 1, "unchunked")


# ---- group B: the flags sit where the names say ----------------------------------------------------------------------------------
def flagged(which, sigma):
    """Batch positions with Y > 0 per partition, from the oracles, and the layout."""
    lay = tc.layout(which)
    return lay, {n: (np.flatnonzero(o["Y"] > 0) + s).tolist() for n, o, s in zip(lay.names, tc.oracles("b", which, sigma), lay.starts)}


@pytest.mark.parametrize("which", list(tc.B_LAYOUTS))
def test_group_b_flags_are_the_ones_placed(which):
    lay, got = flagged(which, "sigma0.1")
    assert [got[n] for n in lay.names] == lay.flags            # radius 0: the counts' own positions
    for n, o in zip(lay.names, tc.oracles("b", which, "sigma0.1")):
        v = tc.values(o)
        assert np.array_equal(v, np.round(v)) and (len(v) == 0 or v.min() >= 1), n          # integers: any order gives the same first sum
    lay, got = flagged(which, "sigma3")
    for n, f, s, part in zip(lay.names, lay.flags, lay.starts, lay.parts):                 # radius 12: runs of 25, cut at the partition's ends
        e = s + int(part.iv_end[0] - part.iv_start[0])
        assert got[n] == sorted({q for x in f for q in range(max(s, x - 12), min(e, x + 12) + 1)}), n
    assert sum(int(p.iv_end[0] - p.iv_start[0]) + 1 for p in lay.parts) == lay.pos and lay.pos % 64 != 0


def test_group_b_offsets_with_the_reads_ends_counted():
    lay, got = flagged("ends", "sigma0.1")
    start = dict(zip(lay.names, lay.starts))
    end = {n: s + int(p.iv_end[0] - p.iv_start[0]) for n, s, p in zip(lay.names, lay.starts, lay.parts)}
    a, b = "first-last-45", "word-shared-2110"
    # first and last position flagged, the partition ending and the next one starting inside one flag word
    assert got[a][0] == start[a] and got[a][-1] == end[a] and got[b][0] == start[b] == end[a] + 1 and got[b][-1] == end[b]
    assert end[a] >> 5 == start[b] >> 5 and end[a] % 32 not in (0, 31) and end[b] % 32 not in (0, 31)
    w0 = start[b] >> 5 << 5                                                                # k_thr_part's groups start on the partition's first word
    assert w0 < start[b] and {w0 + d for d in tc.WORD_OFFSETS} <= set(got[b])
    c = "blocks-0-to-2"                                                                # k_scan_emit<values>: waves of 2 048, blocks of 8 192
    assert {2 * GROUP + d for d in tc.WORD_OFFSETS[:4]} | {CHUNK + d for d in tc.WORD_OFFSETS} | {CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK} <= set(got[c])
    assert start[c] < CHUNK and end[c] > 2 * CHUNK
    # partitions that start one before, on and one after a block of 8 192, with flags in the block before them (what k_voff counts)
    for n, r in (("start-24575", CHUNK - 1), ("start-32768", 0), ("start-40961", 1)):
        before = lay.names[lay.names.index(n) - 1]
        assert start[n] % CHUNK == r and got[n][0] == start[n] and got[before], n
        in_block = [q for q in got[before] if q >= start[n] // CHUNK * CHUNK]
        assert (len(in_block) > 0) == (r != 0), (n, in_block)
    for n in (8, 9, 32):                                                                   # rounds of eight flagged rows: one, two, four
        s, f = start["rows-%d" % n], got["rows-%d" % n]
        assert s % GROUP == 0 and end["rows-%d" % n] - s == GROUP - 1 and len({(q - s) // 64 for q in f}) == n
        assert {(q - s) % 64 for q in f} >= {0, 63}
    for g in (1, 7, 8, 9, 17):                                                             # groups of 64 words a wave: ceil(g / 8)
        n = "groups-%d" % g
        s, e = start[n], end[n]
        assert (((e + 32) >> 5) - (s >> 5) + 63) // 64 == g and {(q - s) // GROUP for q in got[n]} == set(range(g)), n
    gpw = {g: (g + 7) // 8 for g in (1, 7, 8, 9, 17)}
    idle = {g: sum(1 for w in range(8) if w * gpw[g] >= g) for g in gpw}
    assert gpw == {1: 1, 7: 1, 8: 1, 9: 2, 17: 3} and idle == {1: 7, 7: 1, 8: 0, 9: 3, 17: 2}
    n = "groups-9-unaligned"
    s, e = start[n], end[n]
    words = ((e + 32) >> 5) - (s >> 5)
    assert s % 32 == 1 and (words + 63) // 64 == 9 and words % 64 == 1 and got[n][0] == s and got[n][-1] == e
    w0 = s >> 5 << 5
    assert {w0 + GROUP * k + d for k in (1, 2, 7, 8) for d in (-1, 0)} <= set(got[n])         # its own groups' edges, and the batch's waves'
    assert {q for k in range(1, 9) for q in (w0 - 32 + GROUP * k, w0 - 32 + GROUP * k + 31)} <= set(got[n])
    assert (end["last-101"] + 1) % 64 != 0 and got["last-101"][-1] == end["last-101"] == lay.pos - 1


def test_group_b_partitions_without_a_value():
    lay, got = flagged("nan", "sigma0.1")
    for sigma in tc.B_SIGMAS:
        nan = [n for n, o in zip(lay.names, tc.oracles("b", "nan", sigma)) if np.isnan(o["threshold"])]
        assert nan == [n for n in lay.names if n.startswith("nan")] == ["nan-first", "nan-between", "nan-pair-0", "nan-pair-1", "nan-last"]
        assert all(len(tc.values(o)) == 0 for n, o in zip(lay.names, tc.oracles("b", "nan", sigma)) if n in nan)
    i = {n: k for k, n in enumerate(lay.names)}
    assert i["nan-first"] == 0 and i["nan-last"] == len(lay.names) - 1 and 0 < i["nan-between"] < i["nan-pair-0"] == i["nan-pair-1"] - 1
    assert all(got[lay.names[k + d]] for k in (i["nan-between"],) for d in (-1, 1))        # between two partitions that have values
    assert {CHUNK + d for d in tc.WORD_OFFSETS} <= set(got["blocks"]) and len({(q - lay.starts[i["rows-9"]]) // 64 for q in got["rows-9"]}) == 9


# ---- group C ---------------------------------------------------------------------------------------------------------------------
def test_group_c_limits():
    for which, extra in (("c1", 0), ("c2", 1)):
        names, parts, _ = tc.case("c_big", which)
        L = int(parts[1].iv_end[0] - parts[1].iv_start[0]) + 1
        assert L == tc.MAX_CHUNKS * CHUNK + extra == 2 ** 20 + extra and len(parts) == 2 and names[0] == "small-300"
        assert (L + CHUNK - 1) // CHUNK == tc.MAX_CHUNKS + extra                          # c1: the last of k_thr_part's 128 chunk sums, a full chunk
    names, parts, _ = tc.case("c_many")
    assert len(parts) == tc.C3_PARTS > tc.GRID + 4 and len(parts) > 16 * 256              # k_vplan: more than 256 partitions
    count = {p: len(tc.values(tc.oracles("c_many")[p])) for p in tc.C3_NAMED}
    assert count == {p: m for p, (m, _) in tc.C3_NAMED.items()}
    assert count[2] == 8191 and count[2 + tc.GRID] == 129                                # one workgroup: the general tree, then one leaf and a value
    assert count[3] > CHUNK and count[3 + tc.GRID] <= CHUNK                              # two chunks, then one
    assert count[5] <= CHUNK and count[5 + tc.GRID] > 2 * CHUNK                          # one chunk, then three
    n_chunks = sum((len(tc.values(o)) + CHUNK - 1) // CHUNK for o in tc.oracles("c_many"))
    assert n_chunks > 4096 and len(parts) + 1 > 2048                                     # the grids of k_vsum_chunks (4 096) and k_voff (2 048) loop
    tiny = [int(o["pos_off"][-1]) for n, o in zip(names, tc.oracles("c_many")) if n.startswith("tiny")]
    assert len(tiny) >= 4096 and 40 <= min(tiny) and max(tiny) <= 60
