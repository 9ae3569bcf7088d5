"""What k_thr_part carries from step to step, on the device: the batches of
tests/threshold_chain_cases.py -- a workgroup walks two partitions of different shape one after the other (counts 0, 2, 7, 8, 9, 128,
129, 8 191 / 8 192 / 8 193 = the values kept in LDS less one, exactly and one more, 16 384, 16 385, one chunk more than a sweep holds,
and 140 000 = more flag groups a wave than it keeps words of), under the default and under FSEG_THR_PART=0 (the chunk kernels).  tests/test_threshold_chain_host.py proves on the CPU that a stale leaf table, stale values
or a dropped last LDS value would change the bits compared here.

Thresholds bit-identical with the CPU oracle (NaN with NaN) on the first run and on the replay, every other tap equal, the smoothed
signal bit-identical; the census says which kernel ran."""
import numpy as np
import pytest

import threshold_chain_cases as cc
import util
from freddie_amd import _lib

pytestmark = pytest.mark.gpu

SETTINGS = {
    "default": ({}, dict(thr_part=1)),
    "chunks": ({"FSEG_THR_PART": "0"}, dict(thr_part=0)),
}
RUNS = [(kind, s) for kind in cc.KINDS for s in SETTINGS]


def wrong_thresholds(ctx, names, want):
    thr = ctx.tap("threshold")
    assert len(thr) == len(want)
    return ["p%d %s (%r, oracle %r)" % (p, names[p], float(t), o["threshold"]) for p, (t, o) in enumerate(zip(thr, want))
            if not (t == o["threshold"] or (np.isnan(t) and np.isnan(o["threshold"])))][:40]


@pytest.mark.parametrize("kind,setting", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_threshold_chain(kind, setting, monkeypatch):
    for name in ("FSEG_THR_PART", "FSEG_SCAN_SINGLE_MAX"):
        monkeypatch.delenv(name, raising=False)
    env, census = SETTINGS[setting]
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    names, parts, params = cc.case(kind)
    want = cc.oracles(kind)
    ctx = _lib.Context(0)                                      # (the switches are read by fseg_create)
    try:
        for run in ("first run", "replay"):
            if run == "first run":
                util.run_gpu(ctx, parts, params)
            else:
                ctx.run(); ctx.sync()
            wrong = wrong_thresholds(ctx, names, want)         # every partition's, so that a failure names all the edges it broke
            assert not wrong, "%s: thresholds differ from the oracle's: %s" % (run, ", ".join(wrong))
            rep = util.compare_partitions(ctx, parts, want)
            assert rep["y_identical"], "%s: smoothed signal not bit-identical (max err %g)" % (run, rep["max_y_err"])
            got = ctx.paths()
            assert {k: got[k] for k in census} == census, (run, got)
    finally:
        ctx.close()
