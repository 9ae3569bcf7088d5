"""--decide gpu (fiso_isoforms: k_iso_exons + k_iso_correct): exons, strand and corrected boundaries from one device call,
against the reference's GTFs, the CPU oracle on random jobs, hand-built cases at every decision's edge (the oracle's answer
asserted beside the device's and beside the expected one), the library's refusals, and the command line."""
import copy
import ctypes
import os

import numpy as np
import pytest

import isoforms_util as iu
from freddie_amd import isoforms
from oracle import isoforms_oracle
from test_host_mirror import input_dir

pytestmark = pytest.mark.gpu
FAR = 1000000                                            # a read boundary that votes for nothing


@pytest.fixture(scope="module")
def ctx():
    c = isoforms.Context(0)
    yield c
    c.close()


def limits():
    out = (ctypes.c_int32 * 4)()
    assert isoforms.load().fiso_isoforms_limits(ctypes.byref(out)) == 0
    return list(out)


def make_job(tint, pos, iso_reads):
    """(isoforms, segments, reads) of one tint; iso_reads: per isoform a list of (data, tail, starts, ends)."""
    segs = list(zip(pos[:-1], pos[1:]))
    isos, reads = {}, {}
    rid = 0
    for iid, rs in enumerate(iso_reads):
        key = ("c", tint, 0, iid)
        isos[key] = dict(rids=set())
        for data, tail, starts, ends in rs:
            assert len(data) == len(segs)
            reads[rid] = dict(rid=rid, rname="r%d" % rid, chrom="c", strand="+", tint=tint, pid=0, tail=tail, iid=iid, data=data,
                              starts=tuple(starts), ends=tuple(ends))
            isos[key]["rids"].add(rid)
            rid += 1
    return isos, {("c", tint): segs}, reads


def oracle_of(jobs, m, w):
    for isos, segments, reads in jobs:
        isoforms_oracle.isoforms_cons(isos, segments, reads)
        isoforms_oracle.correct_boundaries("starts", isos, reads, m, w)
        isoforms_oracle.correct_boundaries("ends", isos, reads, m, w)
    return [iso for isos, _, _ in jobs for iso in isos.values()]


def decide(ctx, jobs, m, w):
    """The isoform dicts as the device call leaves them (asserted equal to the oracle's: 'starts', 'ends', 'strand', and which
    isoforms have none of them) and the call's result arrays."""
    dev = copy.deepcopy(jobs)
    res = isoforms.decide_gpu_batch(isoforms.isoforms_input(dev), m, w, ctx)
    got = [iso for isos, _, _ in dev for iso in isos.values()]
    want = oracle_of(copy.deepcopy(jobs), m, w)
    assert got == want
    return got, res


def exons(iso):
    return list(zip(iso["starts"], iso["ends"])) if "starts" in iso else None


def plain(data, n=3, tail="N"):
    return [(data, tail, [FAR], [FAR + 1])] * n


# ---- goldens ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", iu.names())
def test_gtf_matches_reference_and_the_host_path(ctx, name, tmp_path):
    doc, ctsv, split_tsv, _, _ = iu.write_case(name, tmp_path, input_dir)
    for m, w in iu.settings():
        text = {}
        for decide_ in ("gpu", "host"):
            recs = isoforms.run_consensus_batch([[doc["contig"], doc["tint_id"], ctsv, split_tsv, m, w]], ctx, verbose=False, decide=decide_)
            recs.sort()
            text[decide_] = "".join(r + "\n" for _, r in recs)
        assert text["gpu"] == doc["gtf"]["%g,%d" % (m, w)], (name, m, w)
        assert text["gpu"] == text["host"], (name, m, w)


# ---- random jobs ------------------------------------------------------------------------------------------------------------
SETTINGS = [(0.5, 8), (0.7, 3), (1.0, 20), (0.5, 0)]


@pytest.mark.parametrize("per", ["1", "3", "tile+1"])
@pytest.mark.parametrize("n_segs", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024])
def test_random_jobs_match_the_oracle(ctx, n_segs, per):
    per = limits()[1] + 1 if per == "tile+1" else int(per)
    job = iu.random_job(7 * n_segs + per, 3, per, n_segs)
    cons = copy.deepcopy(job)
    isoforms_oracle.isoforms_cons(*cons)                             # (the settings change the correction only)
    n_with = 0
    for m, w in SETTINGS:
        dev = copy.deepcopy(job)
        isoforms.decide_gpu_batch(isoforms.isoforms_input([dev]), m, w, ctx)
        want = copy.deepcopy(cons)
        isoforms_oracle.correct_boundaries("starts", want[0], want[2], m, w)
        isoforms_oracle.correct_boundaries("ends", want[0], want[2], m, w)
        assert dev[0] == want[0], (n_segs, per, m, w)
        n_with = sum("starts" in i for i in dev[0].values())
    if per > 250:
        assert n_with == 2                                           # (the case is not empty: both full isoforms have exons)


def test_random_jobs_in_one_batch(ctx):
    """Tints of different row lengths in one call, isoforms with and without exons next to each other."""
    jobs = [iu.random_job(1, 40, 60, 50), iu.random_job(2, 5, 300, 300), iu.random_job(3, 300, 4, 9), iu.random_job(4, 2, 3, 1),
            iu.random_job(5, 6, 40, 130)]
    for m, w in ((0.5, 8), (0.6, 20)):
        got, res = decide(ctx, jobs, m, w)
        assert sum("starts" in i for i in got) > 100 and sum("starts" not in i for i in got) > 5


# ---- counts -----------------------------------------------------------------------------------------------------------------
def test_cons_2_against_cons_3(ctx):
    got, res = decide(ctx, [make_job(1, [100, 200], [plain("1", 2), plain("1", 3)])], 0.5, 8)
    assert exons(got[0]) is None and exons(got[1]) == [(100, 200)]
    assert res["n_exon"].tolist() == [0, 1] and res["seg_first"].tolist() == [0, 0] and res["seg_last"].tolist() == [0, 0]


def test_half_of_the_coverage_is_no_majority(ctx):
    pos = [100, 200, 300, 400]
    got, _ = decide(ctx, [make_job(1, pos, [plain("111") + plain("101"), plain("111") + plain("101", 2)])], 0.5, 0)
    assert exons(got[0]) == [(100, 200), (300, 400)]                 # segment 1: cons 3, cov 6
    assert exons(got[1]) == [(100, 400)]                             # segment 1: cons 3, cov 5


# ---- tails and skipped reads ------------------------------------------------------------------------------------------------
def test_an_s_read_spans_every_segment(ctx):
    pos = [10, 20, 30, 40, 50]
    got, res = decide(ctx, [make_job(1, pos, [plain("0110") + plain("0001", tail="S"), plain("0110") + plain("0001", tail="E")])], 0.5, 0)
    assert exons(got[0]) == [(40, 50)] and got[0]["strand"] == "-"   # the S reads cover segments 1, 2: 3 of 6
    assert exons(got[1]) == [(20, 50)] and got[1]["strand"] == "+"
    assert res["tails"].tolist() == [[3, 3, 0], [3, 0, 3]]


def test_a_read_without_a_1_is_out_of_tails_and_cov_but_counts_in_n(ctx):
    near = [("11", "N", [103], [FAR])] * 3
    skipped = [("00", "S", [FAR], [FAR])] * 3 + [("2X", "S", [FAR], [FAR])]
    got, res = decide(ctx, [make_job(1, [100, 200, 300], [near + skipped[:3], near + skipped[:3] + skipped[3:]])], 0.5, 8)
    assert exons(got[0]) == [(103, 300)] and got[0]["strand"] == "+"  # cov 3, not 6; tails S 0; 3 of N = 6 reaches 0.5
    assert exons(got[1]) == [(100, 300)]                              # 3 of N = 7 does not
    assert res["tails"].tolist() == [[3, 0, 0], [3, 0, 0]]
    got, _ = decide(ctx, [make_job(1, [100, 200, 300], [near + skipped[:3]])], 0.6, 8)
    assert exons(got[0]) == [(100, 300)]                              # 3 of 6 < 0.6 (3 of 3 would have passed)


def test_strand_needs_more_s_than_e(ctx):
    one = lambda t: ("1", t, [FAR], [FAR])
    got, _ = decide(ctx, [make_job(1, [5, 9], [[one("S"), one("E"), one("N")], [one("S"), one("S"), one("E")],
                                              [one("E"), one("E"), one("S")], [one("N")] * 3])], 0.5, 0)
    assert [g["strand"] for g in got] == ["+", "-", "+", "+"]


# ---- exon runs --------------------------------------------------------------------------------------------------------------
def test_runs_at_the_first_and_last_segment(ctx):
    pos = [10, 20, 30, 40, 50, 60]
    got, res = decide(ctx, [make_job(1, pos, [plain("10001"), plain("11111"), plain("01110")])], 0.5, 0)
    assert exons(got[0]) == [(10, 20), (50, 60)] and exons(got[1]) == [(10, 60)] and exons(got[2]) == [(20, 50)]
    assert res["exon_off"].tolist() == [0, 3, 6, 9] and res["n_exon"].tolist() == [2, 1, 1]
    assert res["seg_first"].tolist() == [0, 4, 0, 0, 0, 0, 1, 0, 0] and res["seg_last"].tolist() == [0, 4, 0, 4, 0, 0, 3, 0, 0]


def test_runs_across_word_and_thread_group_borders(ctx):
    M = 300
    pos = list(range(1000, 1000 + 10 * (M + 1), 10))
    data = "".join("1" if 60 <= j <= 70 or 250 <= j <= 260 or j == 127 or j == 128 else "0" for j in range(M))
    got, res = decide(ctx, [make_job(1, pos, [plain(data)])], 0.5, 0)
    assert exons(got[0]) == [(pos[60], pos[71]), (pos[127], pos[129]), (pos[250], pos[261])]
    assert res["seg_first"][:3].tolist() == [60, 127, 250] and res["seg_last"][:3].tolist() == [70, 128, 260]


@pytest.mark.parametrize("M", [1023, 1024])
def test_alternating_flags_fill_every_slot(ctx, M):
    pos = list(range(0, 3 * (M + 1), 3))
    data = ("10" * 512)[:M]
    got, res = decide(ctx, [make_job(1, pos, [plain("01" * 2 + "0" * (M - 4)), plain(data), plain("0" * (M - 1) + "1")])], 0.5, 0)
    cap = (M + 1) // 2
    assert cap == 512 and res["exon_off"].tolist() == [0, cap, 2 * cap, 3 * cap]
    assert res["n_exon"].tolist() == [2, 512, 1]
    assert exons(got[1]) == [(pos[j], pos[j + 1]) for j in range(0, M, 2)][:512]
    assert res["seg_first"][cap:2 * cap].tolist() == list(range(0, 1024, 2)) and exons(got[2]) == [(pos[M - 1], pos[M])]


# ---- votes ------------------------------------------------------------------------------------------------------------------
def voters(n, offsets, b=1000, e=2000):
    """n reads of an isoform of one segment b .. e; read k's start boundaries lie at b + x for x in offsets[k] (none: far)."""
    return [("1", "N", [b + x for x in offsets[k]] if k < len(offsets) and offsets[k] else [FAR], [FAR]) for k in range(n)]


def test_a_vote_share_equal_to_the_threshold_passes_and_one_short_does_not(ctx):
    """v / N == threshold exactly.  An isoform with an exon has at least three reads, so 1 of 2 is taken as 2 of 4: the same
    double, 0.5."""
    cases = [(0.5, 4, 2), (0.5, 6, 3), (0.6, 5, 3), (1.0, 3, 3), (1.0, 7, 7)]
    for m, n, v in cases:
        got, _ = decide(ctx, [make_job(1, [1000, 2000], [voters(n, [[3]] * v), voters(n, [[3]] * (v - 1)), voters(n, [[-4]] * v)])], m, 8)
        assert [exons(g) for g in got] == [[(1003, 2000)], [(1000, 2000)], [(996, 2000)]], (m, n, v)


def test_the_larger_of_two_passing_offsets_wins(ctx):
    got, _ = decide(ctx, [make_job(1, [1000, 2000], [voters(4, [[2], [2], [-3], [-3]]), voters(6, [[-5]] * 4 + [[1]] * 2),
                                                   voters(6, [[-5]] * 3 + [[1]] * 3), voters(3, [[1, 4]] * 3)])], 0.5, 8)
    assert [exons(g)[0][0] for g in got] == [1002, 995, 1001, 1004]


def test_a_read_that_votes_twice_for_one_offset(ctx):
    """v > N: two of a read's boundaries at the same offset both count (:131-136 loops over every boundary)."""
    got, _ = decide(ctx, [make_job(1, [1000, 2000], [voters(3, [[2, 2]]), voters(3, [[2]])])], 0.6, 8)
    assert [exons(g)[0][0] for g in got] == [1002, 1000]             # 2 of 3 reaches 0.6, 1 of 3 does not
    got, _ = decide(ctx, [make_job(1, [1000, 2000], [voters(3, [[2, 2], [2, 2], [2, 2]])])], 1.0, 8)
    assert exons(got[0])[0][0] == 1002                               # 6 of 3


@pytest.mark.parametrize("w", [1, 8, 20])
def test_the_window_is_closed(ctx, w):
    iso = [voters(3, [[x]] * 3) for x in (w, -w, w + 1, -w - 1)]
    ends = [[("1", "N", [FAR], [2000 + x])] * 3 for x in (w, -w, w + 1, -w - 1)]
    got, _ = decide(ctx, [make_job(1, [1000, 2000], iso + ends)], 1.0, w)
    assert [exons(g)[0][0] for g in got[:4]] == [1000 + w, 1000 - w, 1000, 1000]
    assert [exons(g)[0][1] for g in got[4:]] == [2000 + w, 2000 - w, 2000, 2000]


# ---- boundary geometry ------------------------------------------------------------------------------------------------------
def test_one_read_boundary_votes_for_two_isoform_boundaries(ctx):
    pos = [1000, 1005, 1010, 1020]
    got, _ = decide(ctx, [make_job(1, pos, [[("101", "N", [1007], [1015])] * 3])], 1.0, 20)
    assert exons(got[0]) == [(1007, 1015), (1007, 1015)]             # starts 1000 and 1010 both see 1007; ends 1005 and 1020 both 1015


def test_positions_at_the_ends_of_int32(ctx):
    lo, hi = -2 ** 31, 2 ** 31 - 1
    a = make_job(1, [lo + 5, lo + 30], [[("1", "N", [lo], [lo + 12])] * 3])
    b = make_job(2, [hi - 40, hi - 3], [[("1", "N", [hi - 20], [hi])] * 3])
    got, _ = decide(ctx, [a, b], 1.0, 20)
    assert exons(got[0]) == [(lo, lo + 12)] and exons(got[1]) == [(hi - 20, hi)]
    got, _ = decide(ctx, [a, b], 1.0, 4)
    assert exons(got[0]) == [(lo + 5, lo + 30)] and exons(got[1]) == [(hi - 40, hi)]


def test_more_exons_than_the_boundary_tile_and_more_votes_than_one_pass(ctx):
    n_ex = limits()[2] + 1
    M = 2 * n_ex - 1
    pos = list(range(5000, 5000 + 50 * (M + 1), 50))
    data = ("10" * n_ex)[:M]
    starts = [pos[j] + 2 for j in range(0, M, 2)]
    ends = [pos[j + 1] - 3 for j in range(0, M, 2)]
    reads = [(data, "N", starts, ends)] * 3                          # 3 x 257 member boundaries a side
    many = [("1" + "0" * (M - 1), "N", [pos[0] - 1], [pos[1] + 1])] * 300   # 300 reads of one boundary
    got, res = decide(ctx, [make_job(1, pos, [reads, many])], 1.0, 8)
    assert res["n_exon"].tolist() == [n_ex, 1]
    assert exons(got[0]) == list(zip(starts, ends)) and exons(got[1]) == [(pos[0] - 1, pos[1] + 1)]


# ---- isoform sizes ----------------------------------------------------------------------------------------------------------
def test_an_isoform_without_exons_between_two_with(ctx):
    pos = [10, 20, 30, 40, 50]
    job = make_job(1, pos, [[("1010", "N", [11, 31], [21, 41])] * 3, plain("1111", 2), []] + [[("0101", "S", [22], [FAR])] * 3])
    got, res = decide(ctx, [job], 1.0, 3)
    assert exons(got[0]) == [(11, 21), (31, 41)] and exons(got[1]) is None and exons(got[2]) is None and exons(got[3]) == [(22, 30), (40, 50)]
    assert res["n_exon"].tolist() == [2, 0, 0, 2] and res["strand"].tolist() == [ord("+"), 0, 0, ord("-")]
    assert res["exon_off"].tolist() == [0, 2, 4, 6, 8]
    assert res["start"].tolist() == [11, 31, 0, 0, 0, 0, 22, 40] and res["end"].tolist() == [21, 41, 0, 0, 0, 0, 30, 50]
    assert res["tails"].tolist() == [[3, 0, 0], [2, 0, 0], [0, 0, 0], [0, 3, 0]]


def test_a_call_of_isoforms_without_reads(ctx):
    got, res = decide(ctx, [make_job(1, [10, 20, 30], [[], []])], 0.5, 8)
    assert [exons(g) for g in got] == [None, None] and res["n_exon"].tolist() == [0, 0] and res["tails"].tolist() == [[0, 0, 0]] * 2


# ---- refusals ---------------------------------------------------------------------------------------------------------------
ARGS = ("tint_pos_off", "pos", "iso_tint", "iso_read_off", "read_bits_off", "bits", "tail", "read_b_off", "read_start", "read_end")


def base_input():
    inp = isoforms.isoforms_input([iu.random_job(3, 4, 5, 70), iu.random_job(4, 3, 4, 9)])
    return {k: np.array(inp[k]) for k in ARGS}


def call(ctx, a, m=0.5, w=8):
    return ctx.isoforms(*[a[k] for k in ARGS], m, w)


def _bad(a, what):
    if what == "tint_pos_off start":
        a["tint_pos_off"][0] = 1
    elif what == "iso_read_off monotone":
        a["iso_read_off"][2] = a["iso_read_off"][1] - 1
    elif what == "read_b_off monotone":
        a["read_b_off"][3] = a["read_b_off"][2] - 1
    elif what == "read_bits_off start":
        a["read_bits_off"] += 1
    elif what == "read_bits_off advance":
        a["read_bits_off"][4:] += 1
    elif what == "bit beyond M":
        a["bits"][int(a["read_bits_off"][2]) + 1] |= np.uint64(1 << 6)          # a row of 70 segments: bit 70
    elif what == "tail":
        a["tail"][5] = 3
    elif what == "iso_tint high":
        a["iso_tint"][1] = 2
    elif what == "iso_tint negative":
        a["iso_tint"][1] = -1
    elif what == "positions":
        a["pos"][4] = a["pos"][3]
    return a


@pytest.mark.parametrize("what,named", [
    ("tint_pos_off start", "tint_pos_off"), ("iso_read_off monotone", "iso_read_off"), ("read_b_off monotone", "read_b_off"),
    ("read_bits_off start", "read_bits_off"), ("read_bits_off advance", "read_bits_off does not advance by 2 words at read 3"),
    ("bit beyond M", "read 2: a bit is set beyond segment 69"), ("tail", "read 5: tail 3"), ("iso_tint high", "iso_tint[1] = 2"),
    ("iso_tint negative", "iso_tint[1] = -1"), ("positions", "tint 0: positions are not strictly ascending at 4")])
def test_malformed_input_is_refused_by_name(ctx, what, named):
    good = base_input()
    want = call(ctx, good)
    with pytest.raises(isoforms.IsoformsError) as e:
        call(ctx, _bad(base_input(), what))
    assert e.value.code == 1 and named in str(e.value), str(e.value)
    again = call(ctx, good)                                          # the context is as usable as before
    assert all(np.array_equal(want[k], again[k]) for k in want) and want["n_exon"].sum() > 0


@pytest.mark.parametrize("m,w,named", [(0.5, -1, "window -1"), (0.5, 21, "window 21"), (0.49, 8, "majority_threshold 0.49"),
                                       (1.01, 8, "majority_threshold 1.01"), (float("nan"), 8, "majority_threshold")])
def test_settings_out_of_range_are_refused(ctx, m, w, named):
    good = base_input()
    with pytest.raises(isoforms.IsoformsError) as e:
        call(ctx, good, m, w)
    assert e.value.code == 1 and named in str(e.value), str(e.value)
    assert call(ctx, good)["n_exon"].sum() > 0


def test_results_need_a_successful_call():
    c = isoforms.Context(0)
    try:
        L, out = isoforms.load(), isoforms.FisoIsoformsOut()
        assert L.fiso_isoforms_results(c._h, ctypes.byref(out)) == 1
        assert "no successful fiso_isoforms call" in L.fiso_last_error(c._h).decode()
        good = base_input()
        call(c, good)
        assert L.fiso_isoforms_results(c._h, ctypes.byref(out)) == 0 and out.n_iso == 7
        with pytest.raises(isoforms.IsoformsError):
            call(c, good, 0.5, 21)
        assert L.fiso_isoforms_results(c._h, ctypes.byref(out)) == 1      # the refused call is the last one
        assert call(c, good)["n_exon"].sum() > 0
    finally:
        c.close()


def test_a_row_of_1025_segments_is_unsupported(ctx):
    assert limits() == [1024, 256, 256, 0]
    M = limits()[0] + 1
    job = make_job(1, list(range(0, 2 * (M + 1), 2)), [plain("1" * M), plain("0" * (M - 1) + "1")])
    small = make_job(2, [10, 20], [plain("1")])
    inp = isoforms.isoforms_input([small, job])
    with pytest.raises(isoforms.IsoformsError) as e:
        call(ctx, inp)
    assert e.value.code == isoforms.FISO_ERR_UNSUPPORTED == 3 and "isoform 1 has 1025 segments" in str(e.value)
    got, _ = decide(ctx, [small], 0.5, 8)
    assert exons(got[0]) == [(10, 20)]


# ---- command line -----------------------------------------------------------------------------------------------------------
def run_main(tmp_path, sdir, cdir, decide_, extra=()):
    out = str(tmp_path / ("out_%s.gtf" % decide_))
    isoforms.main(["-s", sdir, "-c", cdir, "-m", "0.7", "-w", "3", "-o", out, "--decide", decide_] + list(extra))
    return open(out, "rb").read()


def test_cli_gives_the_same_bytes_either_way(tmp_path):
    names = ["g1_retention", "g_refine", "g_sigma12", "e_plateau_touch"]
    cdir = str(tmp_path / "cluster"); sdir = str(tmp_path / "split")
    for name in names:
        doc = iu.load(name)
        d, contig, tid = input_dir(name, tmp_path)
        os.makedirs(os.path.join(cdir, contig), exist_ok=True); os.makedirs(os.path.join(sdir, contig), exist_ok=True)
        open(os.path.join(cdir, contig, "cluster_%s_%d.tsv" % (contig, tid)), "w").write(doc["cluster_tsv"])
        src = os.path.join(d, contig, "split_%s_%d.tsv" % (contig, tid))
        open(os.path.join(sdir, contig, "split_%s_%d.tsv" % (contig, tid)), "wb").write(open(src, "rb").read())
    before = dict(isoforms.decide_stats)
    gpu = run_main(tmp_path, sdir, cdir, "gpu", ["--batch-tints", "2"])
    assert isoforms.decide_stats["gpu_batches"] - before["gpu_batches"] == 2 and isoforms.decide_stats["fallback_batches"] == before["fallback_batches"]
    host = run_main(tmp_path, sdir, cdir, "host", ["--batch-tints", "2"])
    assert gpu == host and gpu.count(b"\ttranscript\t") >= 4


def test_cli_sends_a_tint_of_1025_segments_to_the_host_path(tmp_path):
    M = 1025
    pos = list(range(100, 100 + 7 * (M + 1), 7))
    cdir = tmp_path / "cluster" / "chr1"; sdir = tmp_path / "split" / "chr1"
    cdir.mkdir(parents=True); sdir.mkdir(parents=True)
    rows = ["1" * 600 + "0" * 425, "1" * 600 + "0" * 424 + "1", "0" * 300 + "1" * 725]
    clines = ["#chr1\t0\t" + ",".join(map(str, pos))]
    slines = ["#chr1\t0"]
    for rid in range(9):
        data = rows[rid % 3]
        clines.append("\t".join([str(rid), "r%d" % rid, "chr1", "+", "0", "0", "NSE"[rid % 3], "0", data]))
        first, last = data.index("1"), M - 1 - data[::-1].index("1")
        slines.append("\t".join([str(rid), "r%d" % rid, "chr1", "+", "0", "%d-%d:x" % (pos[first] + 2, pos[last + 1] - 1)]))
    (cdir / "cluster_chr1_0.tsv").write_text("\n".join(clines) + "\n")
    (sdir / "split_chr1_0.tsv").write_text("\n".join(slines) + "\n")
    before = dict(isoforms.decide_stats)
    gpu = run_main(tmp_path, str(tmp_path / "split"), str(tmp_path / "cluster"), "gpu")
    assert isoforms.decide_stats["fallback_batches"] - before["fallback_batches"] == 1
    assert isoforms.decide_stats["gpu_batches"] == before["gpu_batches"]
    host = run_main(tmp_path, str(tmp_path / "split"), str(tmp_path / "cluster"), "host")
    assert gpu == host and b"\texon\t" in gpu


# ---- the default path -------------------------------------------------------------------------------------------------------
def test_the_default_makes_no_fiso_isoforms_call(ctx, tmp_path, monkeypatch):
    L = isoforms.load()
    real, calls = L.fiso_isoforms, []

    def counting(*a):
        calls.append(1)
        return real(*a)

    monkeypatch.setattr(L, "fiso_isoforms", counting)
    name = iu.names()[0]
    doc, ctsv, split_tsv, _, _ = iu.write_case(name, tmp_path, input_dir)
    args = [[doc["contig"], doc["tint_id"], ctsv, split_tsv, 0.5, 8]]
    isoforms.run_consensus_batch(args, ctx, verbose=False)
    assert calls == []
    assert isoforms.parse_args(["-s", "s", "-c", "c"]).decide == "host"
    isoforms.run_consensus_batch(args, ctx, verbose=False, decide="gpu")
    assert calls == [1]                                              # (the wrapper does see the call when it is made)
