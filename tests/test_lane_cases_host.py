"""tests/lane_cases.py on the CPU: every batch reaches the edge it is named after -- shown from its inputs: tile and block counts, where
the largest last position sits in sorted order, exon totals per tile, which chunk has a lane on which bound --, every mutation a batch
names changes that batch's expected arrays and every mutation has such a batch, the validation restatement agrees with the oracle's
error where the oracle has the rule (:666-668), and the oracle accepts the accepted half of group V."""
import numpy as np
import pytest

import lane_cases as lc
import util


def parts_of(name):
    return lc.batch(name)[0]


def tiles(p):
    return -(-p.n_reps // lc.TILE)


# ---- every case reaches its edge -----------------------------------------------------------------------------------------------------
def test_rep_counts_sit_on_the_sorts_sizes():
    for n in lc.N_SIZES:
        (p,), _ = lc.batch("N-%d" % n)
        assert p.n_reps == n and lc.model_batch([p])["lane_sort"] == 0
    assert {1, 2, lc.SORT_MAX - 1, lc.SORT_MAX} <= set(lc.N_SIZES)
    # powers of two of the bitonic network, one rep to either side; whole tiles, one rep to either side
    assert all({n - 1, n, n + 1} <= set(lc.N_SIZES) for n in (64, 256, 512)) and {1023, 1025, 2047} <= set(lc.N_SIZES)
    allp = parts_of("N-all")
    assert sorted(p.n_reps for p in allp) == sorted(lc.N_SIZES)
    assert all(tiles(a) != tiles(b) for a, b in zip(allp, allp[1:]))
    assert lc.model_batch(allp)["lane_sort"] == 0
    big = parts_of("N-all+2049")
    assert max(p.n_reps for p in big) == lc.SORT_MAX + 1 and sum(p.n_reps <= lc.SORT_MAX for p in big) == 16
    assert big[0].n_reps <= lc.SORT_MAX and big[-1].n_reps <= lc.SORT_MAX              # small partitions on both sides of the large one
    assert lc.model_batch(big)["lane_sort"] == 1
    # ties on the first position in the partitions of more than one tile
    assert all(len(np.unique(lc.firsts(p))) < p.n_reps for p in allp if p.n_reps > 256)


def test_order_cases():
    parts = lc.order_partitions()
    for how in ("sorted", "reverse", "shuffled"):
        p = parts["T-" + how]
        first = lc.firsts(p)
        srt = np.sort(first)
        # runs of ties across the edge of tile 0 and across key 512 of the network of 1 024
        assert p.n_reps == 700 and (srt[250:261] == srt[250]).all() and srt[249] < srt[250] < srt[261]
        assert (srt[505:521] == srt[505]).all() and srt[504] < srt[505] < srt[521]
        d = np.diff(first.astype(np.int64))
        assert {"sorted": (d >= 0).all(), "reverse": (d <= 0).all(), "shuffled": (d > 0).any() and (d < 0).any()}[how]
    # reverse input: the tied reps arrive in falling order of nothing but their index -- rep order is still the rule
    one = parts["T-one-first"]
    assert len(np.unique(lc.firsts(one))) == 1 and len(np.unique(lc.lasts(one))) == one.n_reps
    assert np.array_equal(lc.sorted_order(one), np.arange(one.n_reps))
    assert lc.firsts(parts["T-2^30"]).min() > 2 ** 30 and parts["T-2^30"].iv_start[0] > 2 ** 30
    p = parts["T-2e9"]
    assert p.iv_start[0] >= 1_999_999_000 and p.iv_end[-1] < 2 ** 31 - 1 and lc.firsts(p).min() >= 2_000_000_000
    assert ((lc.firsts(p).astype(np.int64) ^ 0x80000000) >> 28 == 0xF).all()          # the biased key's top four bits are set
    pw = parts_of("T-partition-word")
    lo = [int(lc.firsts(p).min()) for p in pw]
    hi = [int(lc.firsts(p).max()) for p in pw]
    assert any(hi[i + 1] < lo[i] for i in range(len(pw) - 1)) and any(lo[i + 1] > hi[i] for i in range(len(pw) - 1))


@pytest.mark.parametrize("n", lc.M_SIZES)
def test_running_maximum_cases(n):
    parts = parts_of("M-%d" % n)
    blocks = -(-n // lc.TILE)
    assert blocks == {300: 2, 2049: 9, 16385: 65, 16640: 65}[n]
    assert (blocks > lc.SCAN) == (n > 16384)                       # k_lane_block_scan's second trip
    if n == 16640:
        assert parts[1].n_reps == 16384 and tiles(parts[1]) == lc.SCAN
        parts = parts[:1] + parts[2:]
    for p, where in zip(parts, lc.M_WHERE):
        assert p.n_reps == n
        last = lc.lasts(p)[lc.sorted_order(p)].astype(np.int64)
        assert len(np.unique(lc.firsts(p))) == n                   # no ties: the order is the first positions' alone
        assert not np.array_equal(lc.sorted_order(p), np.arange(n))
        if where == "rising":
            assert (np.diff(last) > 0).all()
        elif where == "falling":
            assert (np.diff(last) < 0).all()
        else:
            j = n - 1 if where == "last" else where
            assert int(np.argmax(last)) == j and (np.delete(last, j) < last[j] - 40).all()
            # the value must survive every wave, tile, block and trip behind it
            assert (np.maximum.accumulate(last)[j:] == last[j]).all()


def test_weight_cases():
    parts = parts_of("W")
    assert (parts[0].rep_weight == 1).all()
    for p, j in zip(parts[1:5], (0, 599, 255, 256)):
        w = p.rep_weight[lc.sorted_order(p)]
        assert w[j] == lc.W_HEAVY and w.sum() == lc.W_HEAVY + 599
    assert parts[5].rep_weight.min() == 2 and parts[5].rep_weight.max() == 5
    assert all(tiles(p) == 3 for p in parts)
    m = lc.model_batch(parts)
    assert np.array_equal(np.diff(m["part_lane_off"]), [p.rep_weight.sum() for p in parts])
    assert m["hist16"] == 0                                        # a position can count 70 005: the 32-bit counters


def test_exon_stream_cases():
    parts = parts_of("X")

    def tile_totals(p):
        ne = np.diff(p.rep_exon_off)[lc.sorted_order(p)]
        return [int(ne[i:i + lc.TILE].sum()) for i in range(0, p.n_reps, lc.TILE)], ne
    for p, t in zip(parts, lc.X_TOTALS):
        assert p.n_reps == lc.TILE and tile_totals(p)[0] == [t]
    tot, ne = tile_totals(parts[5])
    before = int(ne[:255].sum())
    assert ne[255] == 40 and before < lc.LEX < before + 40 and tot[0] == 4120          # a rep across exon 4 096 of its tile's piece
    tot, ne = tile_totals(parts[6])
    assert sorted(ne)[-2:] == [4097, 9000] and len(tot) == 1 and tot[0] > 3 * lc.LEX
    assert (np.diff(parts[7].rep_exon_off) == 1).all() and parts[7].n_reps > lc.TILE
    assert parts[8].rep_weight.max() > 1 and tile_totals(parts[8])[0][0] > lc.LEX
    assert not np.array_equal(lc.sorted_order(parts[0]), np.arange(lc.TILE))


def test_partition_and_block_counts():
    for n in lc.B_COUNTS:
        assert len(parts_of("B-%d" % n)) == n
    # end_bit of the radix sort: 33 + the bits of n_part beyond the first
    assert {2 ** k for k in (0, 1, 2, 3, 8)} | {2 ** k + 1 for k in (1, 2, 3, 8)} <= set(lc.B_COUNTS) | {3}
    assert len({(p.n_reps, int(p.iv_start[0])) for p in lc.TINY}) == 7 and {p.n_reps for p in lc.TINY} == {1, 2, 3}
    parts = parts_of("B-%d" % lc.B_LARGE)
    assert len(parts) == lc.GRID + 1 + 300
    assert len(parts) > lc.GRID                                    # k_lanes' loop over partitions: a second trip
    assert sum(tiles(p) for p in parts) > lc.GRID                  # every loop over rep blocks: a second trip
    assert len({id(p) for p in parts}) == 7


@pytest.mark.parametrize("name,chunk", [("H-1024", lc.CHUNK_MIN), ("H-full", lc.CHUNK16)])
def test_histogram_range_cases(name, chunk):
    parts = parts_of(name)
    assert lc.chunk_size(parts) == chunk
    p = parts[1]
    q0, n, glo, ghi = lc.chunks(p, chunk)
    m = lc.model_partition(p)
    rows = lc.model_ranges(p, m, chunk)
    start, pmax = m["start"], m["pmax"]
    ivs = list(zip(p.iv_start.tolist(), p.iv_end.tolist()))
    assert len(q0) == 9 and n[-1] < chunk and (n[:-1] == chunk).all()
    assert ivs[0][0] < glo[1] and ghi[1] < ivs[0][1]               # chunk 1: in the middle of the first interval
    assert glo[3] == ivs[1][0]                                     # chunk 3: starts on an interval's first position
    assert glo[4] < ivs[1][1] < ivs[2][0] < ghi[4]                 # chunk 4: spans a gap
    assert glo[0] == ivs[0][0] and ghi[8] == ivs[2][1]             # the partition's first and last chunk
    on = {}
    for c in range(9):
        llo, lhi = int(rows[c, 2]), int(rows[c, 3])
        on[c] = (llo > 0 and pmax[llo - 1] == glo[c] - 1, llo < len(pmax) and pmax[llo] == glo[c],
                 lhi > 0 and start[lhi - 1] == ghi[c], lhi < len(start) and start[lhi] == ghi[c] + 1)
    assert on[1] == (True, True, True, True) and on[4] == (True, True, True, True)
    assert on[0][2:] == (True, True) and on[8][:2] == (True, True)
    assert on[3][2:] == (True, True) and start[int(rows[3, 2])] == glo[3] and pmax[int(rows[3, 2]) - 1] == ivs[0][1]
    assert rows[lc.H_EMPTY_CHUNK, 2] == rows[lc.H_EMPTY_CHUNK, 3] and 0 < rows[lc.H_EMPTY_CHUNK, 2] < len(start)
    assert all(rows[c, 2] < rows[c, 3] for c in lc.H_BOUND_CHUNKS)


def test_chunking_follows_the_counters_width():
    small = parts_of("N-3")
    assert lc.chunk_size(small) == lc.CHUNK_MIN and lc.hist_packed(small)
    assert lc.chunk_size(parts_of("B-%d" % lc.B_LARGE)) == 4096
    heavy = [lc.single([1000, 1010], [1020, 1030], weights=[65536, 1])]
    light = [lc.single([1000, 1010], [1020, 1030], weights=[65535, 1])]
    assert not lc.hist_packed(heavy) and lc.hist_packed(light)
    assert lc.chunk_size(light + [lc.filler()]) == lc.CHUNK16 and lc.chunk_size(heavy + [lc.filler()]) == lc.CHUNK32


# ---- every mutation is seen ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lc.SEES))
def test_named_mutations_change_the_expected_arrays(name):
    parts = parts_of(name)
    want = lc.model_batch(parts)
    for mut in lc.SEES[name]:
        assert lc.differs(want, lc.model_batch(parts, mut)), (name, mut)


def test_every_mutation_has_a_batch():
    seen = {m for muts in lc.SEES.values() for m in muts}
    assert seen == set(lc.MUTATIONS) - {"key_unsigned"}
    assert set(lc.SEES) <= set(lc.BATCHES)
    # where each carry of the maximum is looked at: only the 65-block partitions see a trip's carry lost
    for name in ("M-300", "M-2049"):
        parts = parts_of(name)
        assert not lc.differs(lc.model_batch(parts), lc.model_batch(parts, "pmax_reset_16384"))


def test_unsigned_keys_differ_only_below_zero():
    """The bias of the sort key (first ^ 0x80000000) gives signed order.  Every built position is a genomic coordinate, at least 0, and
    there an unbiased unsigned key sorts alike -- at 2^30 and at 2 000 000 000 too; it is a negative position that would tell."""
    for name in ("T-order", "T-2e9", "T-partition-word"):
        parts = parts_of(name)
        assert not lc.differs(lc.model_batch(parts), lc.model_batch(parts, "key_unsigned"))
    below = [lc.single([-50, 20, -10], [-40, 30, 5])]
    assert lc.differs(lc.model_batch(below), lc.model_batch(below, "key_unsigned"))


def test_the_model_is_the_one_the_suite_already_states():
    """util.lanes_range (k_prob_range's rule on the host) over the same partitions."""
    for p in parts_of("T-order") + parts_of("W")[-1:]:
        m = lc.model_partition(p)
        lanes, lo, n = util.lanes_range(p, int(p.iv_start[0]) + 100, int(p.iv_start[0]) + 900)
        assert np.array_equal(m["start"], lc.firsts(p)[lanes]) and np.array_equal(m["pmax"], np.maximum.accumulate(lc.lasts(p)[lanes]))
        assert lo == np.searchsorted(m["pmax"], int(p.iv_start[0]) + 100, "left")


# ---- validation --------------------------------------------------------------------------------------------------------------------------
def test_the_oracle_accepts_the_accepted_half():
    parts = parts_of("V-accepted")
    assert lc.verdict(parts) is None
    for o in lc.oracles("V-accepted"):
        assert o["error"] == 0, o["errmsg"]
    (s0, e0), (s2, e2) = lc.V_IVS[0], lc.V_IVS[2]
    ex = lambda p: list(zip(p.ex_ts.tolist(), p.ex_te.tolist()))      # noqa: E731
    assert (s0, s0 + 9) in ex(parts[0]) and (e0 - 9, e0) in ex(parts[0]) and (s0, e0) in ex(parts[0])
    assert (1100, 1200) in ex(parts[1]) and (1200, 1300) in ex(parts[1])
    assert parts[2].ex_te.max() <= e0 and parts[3].ex_ts.min() >= s2 and (s2, e2) in ex(parts[3])
    assert lc.firsts(parts[4])[0] > s2 and lc.firsts(parts[4])[1] == s2              # the binary search ends on the last interval


@pytest.mark.parametrize("name", list(lc.REFUSALS))
def test_refusals_against_the_oracle(name):
    rule = lc.REFUSALS[name][0]
    for where in lc.PLACES:
        big, r = lc.place(where)
        good, bad = lc.v_base(big), lc.refused(name, where)
        assert lc.verdict(good) is None
        assert lc.verdict(bad) == (rule, r), (name, where)
        assert lc.offenders(bad) == {rule: r}                         # one rule, one rep: nothing else about the batch changed
        r0 = 0
        for g, b in zip(good, bad):
            hit = r0 <= r < r0 + b.n_reps
            o = util.run_oracle(b, lc.ENDS, stop_after=1)
            # the oracle has :666-668 only
            assert (o["error"] != 0) == (hit and rule == "interval"), (name, where, o["errmsg"])
            if not hit:
                assert all(np.array_equal(getattr(g, f), getattr(b, f)) for f in ("ex_ts", "ex_te", "rep_exon_off"))
            r0 += b.n_reps
    assert [lc.place(w)[1] for w in lc.PLACES[:4]] == [0, lc.TILE - 1, lc.TILE, sum(p.n_reps for p in lc.v_base(False)) - 1]
    assert lc.v_base(False)[0].n_reps == 300                        # reps 255 and 256: the last of one block, the first of the next
    assert lc.v_base(True)[1].n_reps == lc.SORT_MAX + 1


def test_reversed_exons_stay_inside_their_interval():
    """What the module docstring of lane_cases promises about ts > te."""
    for where in lc.PLACES:
        for p in lc.refused("ts>te", where):
            rev = p.ex_ts > p.ex_te
            for ts, te in zip(p.ex_ts[rev], p.ex_te[rev]):
                assert any(s <= te < ts <= e for s, e in zip(p.iv_start, p.iv_end))


def test_two_bad_reps():
    want = {"interval@20+ends@310": ("interval", 20), "ends@320+interval@5": ("interval", 5), "order@257+order@300": ("order", 257)}
    for name, edits in lc.PAIRS.items():
        bad = lc.spoiled(lc.v_base(False), edits)
        assert lc.verdict(bad) == want[name]
        assert len({r // lc.TILE if r < 300 else 2 + (r - 300) // lc.TILE for r in edits}) == 2        # two rep blocks
    assert lc.offenders(lc.spoiled(lc.v_base(False), lc.PAIRS["interval@20+ends@310"])) == {"interval": 20, "ends": 310}
