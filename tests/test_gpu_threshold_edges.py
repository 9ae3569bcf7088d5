"""The variance threshold at its edges, on the device, both ways: a workgroup per partition (k_thr_part) and the batch-wide
compaction with a workgroup per chunk (k_scan_emit<values>, k_voff, k_vplan, k_vsum_chunks, k_vsum_part; with FSEG_SCAN_SINGLE_MAX=0
behind k_scan1 / k_scan2, k_voff reading the block sums).  Cases: tests/threshold_cases.py -- vsum_chunk's tree shapes (group A),
flags on the words, rows, groups and blocks the compactions cut at (group B), 2^20 positions, one more, and more than 4 096
partitions (group C).  tests/test_threshold_cases_host.py proves on the CPU that every case reaches its edge.

Every tap against the CPU oracle on the first run and on the replay: thresholds bit-identical (NaN with NaN), `fixed` and everything
behind it equal, the smoothed signal bit-identical; the census says which path ran."""
import numpy as np
import pytest

import threshold_cases as tc
import util
from freddie_amd import _lib

pytestmark = pytest.mark.gpu

SETTINGS = {
    "part": {"FSEG_THR_PART": "1"},
    "chunks": {"FSEG_THR_PART": "0"},
    "chunks-scan3": {"FSEG_THR_PART": "0", "FSEG_SCAN_SINGLE_MAX": "0"},
    "default": {},
}
RUNS = [(key, s) for key in tc.ALL for s in ("part", "chunks", "chunks-scan3")] + [(("c_many",), "default")]


def expected_path(key, setting):
    if key == ("c_big", "c2"):
        return 0                                               # one position more than k_thr_part's 128 chunk sums hold
    if setting == "default":
        assert len(tc.case(*key)[1]) >= 64
        return 1
    return int(setting == "part")


def wrong_thresholds(ctx, names, want):
    thr = ctx.tap("threshold")
    assert len(thr) == len(want)
    return ["p%d %s (%r, oracle %r)" % (p, names[p], float(t), o["threshold"]) for p, (t, o) in enumerate(zip(thr, want))
            if not (t == o["threshold"] or (np.isnan(t) and np.isnan(o["threshold"])))][:40]


@pytest.mark.parametrize("key,setting", RUNS, ids=["%s-%s" % ("-".join(k), s) for k, s in RUNS])
def test_threshold_edges(key, setting, monkeypatch):
    for name in ("FSEG_THR_PART", "FSEG_SCAN_SINGLE_MAX"):
        monkeypatch.delenv(name, raising=False)
    for name, v in SETTINGS[setting].items():
        monkeypatch.setenv(name, v)
    names, parts, params = tc.case(*key)
    want = tc.oracles(*key)
    ctx = _lib.Context(0)                                      # (the switches are read by fseg_create)
    try:
        for run in ("first run", "replay"):
            if run == "first run":
                util.run_gpu(ctx, parts, params)
            else:
                ctx.run(); ctx.sync()
            wrong = wrong_thresholds(ctx, names, want)         # every partition's, so that a failure names all the edges it broke
            assert not wrong, "%s: thresholds differ from the oracle's: %s" % (run, ", ".join(wrong))
            try:
                rep = util.compare_partitions(ctx, parts, want)
            except AssertionError as e:
                raise AssertionError("%s, %s (partitions: %s)" % (run, e, ", ".join("p%d %s" % x for x in list(enumerate(names))[:64]))) from None
            assert rep["y_identical"], "%s: smoothed signal not bit-identical (max err %g)" % (run, rep["max_y_err"])
            assert ctx.paths()["thr_part"] == expected_path(key, setting), (run, ctx.paths()["thr_part"])
    finally:
        ctx.close()
