"""Host side of --decide gpu (freddie_amd/isoforms.py), no GPU needed: the label bits, the arrays built for the one
device call, and the command line."""
import numpy as np
import pytest

import isoforms_util as iu
from freddie_amd import isoforms


@pytest.mark.parametrize("M", [1, 63, 64, 65, 128, 129])
def test_pack_label_bits_against_a_loop(M):
    rng = np.random.default_rng(M)
    rows = rng.choice(np.frombuffer(b"012X-", np.uint8), size=(7, M), p=[0.3, 0.4, 0.1, 0.1, 0.1])
    rows[0] = ord("1"); rows[1] = ord("0"); rows[2] = ord("X")
    rows[3, -1] = ord("1"); rows[4, -1] = ord("2")
    got = isoforms.pack_label_bits(rows, M)
    W = (M + 63) // 64
    assert got.shape == (7, W) and got.dtype == np.dtype("<u8")
    for r in range(7):
        want = [0] * W
        for j in range(M):
            if chr(rows[r, j]) == "1":
                want[j // 64] |= 1 << (j % 64)
        assert [int(x) for x in got[r]] == want, (M, r)
    assert {"X", "-", "2"} <= {chr(c) for c in rows.reshape(-1)} or M < 8
    # a flat buffer of the same bytes packs the same
    assert np.array_equal(isoforms.pack_label_bits(rows.reshape(-1), M), got)


def test_pack_label_bits_of_no_rows_and_no_columns():
    assert isoforms.pack_label_bits(np.zeros(0, np.uint8), 5).shape == (0, 1)
    assert isoforms.pack_label_bits(np.zeros((3, 0), np.uint8), 0).shape == (3, 0)


def test_the_argument_builder_on_random_jobs():
    jobs = [iu.random_job(1, 5, 4, 70), iu.random_job(2, 3, 6, 9), iu.random_job(3, 2, 3, 64)]
    inp = isoforms.isoforms_input(jobs)
    isos = [(j, key) for j, (isoforms_, _, _) in enumerate(jobs) for key in isoforms_]
    assert len(inp["isos"]) == len(isos) == 10
    assert all(inp["isos"][i] is jobs[j][0][key] for i, (j, key) in enumerate(isos))
    # tints: one a job here, M + 1 positions each
    assert inp["tint_pos_off"].tolist() == [0, 71, 81, 146]
    for t, (_, segments, _) in enumerate(jobs):
        segs = next(iter(segments.values()))
        assert inp["pos"][inp["tint_pos_off"][t]:inp["tint_pos_off"][t + 1]].tolist() == [s for s, _ in segs] + [segs[-1][1]]
    assert inp["iso_tint"].tolist() == [0] * 5 + [1] * 3 + [2] * 2
    # reads: grouped by isoform, an isoform's in sorted(rids) order; N counts them all
    want_rids = [(j, rid) for j, key in isos for rid in sorted(jobs[j][0][key]["rids"])]
    assert inp["rids"] == want_rids
    assert inp["N"].tolist() == [len(jobs[j][0][key]["rids"]) for j, key in isos]
    assert inp["iso_read_off"].tolist() == np.concatenate([[0], np.cumsum(inp["N"])]).tolist()
    R = len(want_rids)
    W = np.repeat([(70 + 63) // 64] * 5 + [1] * 3 + [1] * 2, inp["N"])
    assert inp["read_bits_off"].tolist() == np.concatenate([[0], np.cumsum(W)]).tolist()
    assert len(inp["bits"]) == inp["read_bits_off"][-1] and inp["bits"].dtype == np.uint64
    assert len(inp["tail"]) == R
    b = 0
    for r, (j, rid) in enumerate(want_rids):
        read = jobs[j][2][rid]
        M = len(read["data"])
        o = int(inp["read_bits_off"][r])
        word = [int(x) for x in inp["bits"][o:o + (M + 63) // 64]]
        assert [(word[k // 64] >> (k % 64)) & 1 for k in range(M)] == [int(c == "1") for c in read["data"]]
        assert inp["tail"][r] == {"N": 0, "S": 1, "E": 2}[read["tail"]]
        assert inp["read_b_off"][r] == b
        n = len(read["starts"])
        assert inp["read_start"][b:b + n].tolist() == list(read["starts"]) and inp["read_end"][b:b + n].tolist() == list(read["ends"])
        b += n
    assert inp["read_b_off"][R] == b and inp["missing"] == []


def test_the_builder_notes_reads_without_boundaries_and_keeps_the_host_asserts():
    isos, segments, reads = iu.random_job(5, 3, 4, 12)
    rid = sorted(isos[("c", 5, 0, 1)]["rids"])[1]
    del reads[rid]["starts"], reads[rid]["ends"]
    inp = isoforms.isoforms_input([(isos, segments, reads)])
    assert inp["missing"] == [(1, rid)]
    r = inp["rids"].index((0, rid))
    assert inp["read_b_off"][r] == inp["read_b_off"][r + 1]
    reads[rid]["data"] += "0"
    with pytest.raises(AssertionError):
        isoforms.isoforms_input_rows([(isos, segments, reads)])
    reads[rid]["data"] = reads[rid]["data"][:-1]
    reads[rid]["tail"] = "Q"
    with pytest.raises(KeyError):
        isoforms.isoforms_input_rows([(isos, segments, reads)])


def test_parse_args_accepts_decide():
    base = ["-s", "s", "-c", "c"]
    assert isoforms.parse_args(base).decide == "host"
    assert isoforms.parse_args(base + ["--decide", "gpu"]).decide == "gpu"
    assert isoforms.parse_args(base + ["--decide", "host"]).decide == "host"
    with pytest.raises(SystemExit):
        isoforms.parse_args(base + ["--decide", "cpu"])
    assert {"fiso_isoforms", "fiso_isoforms_results", "fiso_isoforms_limits"} <= set(isoforms.EXPORTS)
    assert set(isoforms.decide_stats) == {"gpu_batches", "fallback_batches"}
