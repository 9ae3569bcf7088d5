"""Differential test of the oracle against the reference's own results on generated inputs: the reference's smoothed signal,
final positions, labels and output bytes were recorded by tests/golden/make_live_golden.py (tests/golden/live/); the inputs are
regenerated here from the recorded generator arguments."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_live_golden as live  # noqa: E402
import util  # noqa: E402
from freddie_amd import pack, synth  # noqa: E402


def recorded(name, d):
    """The reference's recorded arrays of a case, once the case's input TSVs written under ``d`` are the ones it read."""
    _, _, rec = live.load(name)
    live.write_inputs(name, d)
    assert live.inputs_digest(d) == str(rec["inputs_sha256"]), "the generator no longer writes the inputs the fixture was minted from"
    return rec


def oracle_vs_recorded(name, d):
    """(the oracle's result on the case's partition, the reference's recorded arrays)."""
    gen, run, _ = live.load(name)
    rec = recorded(name, d)
    g = synth.generate(live.CASES[name][0], with_seq=False, **gen)
    part = pack.pack_partition(g.iv_start, g.iv_end, g.read_exon_off, g.ex_ts, g.ex_te)
    o = util.run_oracle(part, dict(run, ignore_ends=True))
    assert o["error"] == 0, o["errmsg"]
    assert part.n_reps == len(rec["labels"])
    return o, rec


@pytest.mark.parametrize("seed", [101, 102, 103])
def test_oracle_vs_live_reference(tmp_path, seed):
    o, rec = oracle_vs_recorded("seed%d" % seed, str(tmp_path))
    assert np.array_equal(rec["Y"], o["Y"])
    assert np.array_equal(rec["final_positions"], o["final_pos"])
    assert np.array_equal(np.asarray(o["labels"]), rec["labels"])


def test_oracle_vs_live_reference_threshold_rate_one(tmp_path):
    """threshold_rate == 1 (the CLI's upper bound): long segments get h == 1, low == 0, so a read without coverage
    is ambiguous ('2') there -- the lo < 0 paths of the kernels."""
    o, rec = oracle_vs_recorded("threshold_rate_one", str(tmp_path))
    assert live.CASES["threshold_rate_one"][2]["threshold_rate"] == 1.0
    assert np.array_equal(rec["final_positions"], o["final_pos"])
    assert np.array_equal(np.asarray(o["labels"]), rec["labels"])
    assert np.count_nonzero(rec["labels"] == 2) > 0


def test_oracle_vs_live_reference_large_problems(tmp_path):
    """max_problem_size = 100: DP problems with up to ~110 candidates (the default 50 keeps them <= 60)."""
    o, rec = oracle_vs_recorded("large_problems", str(tmp_path))
    assert live.CASES["large_problems"][2]["max_problem_size"] == 100
    assert int((np.asarray(o["prob_end"]) - np.asarray(o["prob_start"]) + 1).max()) > 60
    assert np.array_equal(rec["final_positions"], o["final_pos"])
    assert np.array_equal(np.asarray(o["labels"]), rec["labels"])


@pytest.mark.parametrize("seed", [31, 33])
def test_native_writer_vs_live_reference_on_crafted_poly_clips(tmp_path, seed):
    """The native writer's gaps / poly-A annotation (:370-472; one pass for both letters since round 6) against the reference's own
    run_segment() output bytes on soft clips crafted to hold competing poly-A / poly-T runs (ties, lengths 19 / 20, impurities, both
    strands).  Labels and final positions are the reference's."""
    from freddie_amd import _host
    from test_host_native import paths
    d = str(tmp_path / "in")
    rec = recorded("poly_clips%d" % seed, d)
    want = rec["segment_tsv"].tobytes()
    assert sum(want.count(k) for k in (b"SA_", b"ST_", b"EA_", b"ET_")) >= 25
    labels, fp = rec["labels"], rec["final_positions"]
    sp, rp = paths(d, "chrS", seed)
    hb = _host.HostBatch([sp], [rp], n_threads=2)
    try:
        out = str(tmp_path / "got.tsv")
        hb.write(np.array([0, len(fp)]), fp, np.array([0, labels.size]), (labels + 48).astype(np.uint8).ravel(), [out], n_threads=2)
        assert open(out, "rb").read() == want
    finally:
        hb.close()
