"""k_label_reads on the device: the batches of tests/label_cases.py, every tap against the CPU oracle on the first run and on the
replay -- under the default (the column table and the units' exons read from LDS where they fit) and with the label launch capped at
one and at three workgroups (FSEG_LABEL_GRID), so that one workgroup walks units of different partitions and shapes in turn over
what the unit before it staged.  The census word label_packed says which arena the kernel wrote."""
import numpy as np
import pytest

import label_cases as lc
import util

pytestmark = pytest.mark.gpu

SWITCHES = {
    "default": {},
    "grid-1": {"FSEG_LABEL_GRID": "1"},
    "grid-3": {"FSEG_LABEL_GRID": "3"},
}


@pytest.mark.parametrize("switch", list(SWITCHES))
@pytest.mark.parametrize("name", list(lc.BATCHES))
def test_labels_against_the_oracle(name, switch, monkeypatch):
    from freddie_amd import _lib
    env = SWITCHES[switch]
    for k in ("FSEG_LABEL_GRID", "FSEG_LABEL_BYTES"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    names, parts, params = lc.batch(name)
    want = lc.oracles(name)
    packed = name != "bytes"
    ctx = _lib.Context(0)                                            # (the switches are read by fseg_create)
    try:
        for run in ("first run", "replay"):
            if run == "first run":
                util.run_gpu(ctx, parts, params)
            else:
                ctx.run(); ctx.sync()
            census = ctx.paths()
            assert census["label_packed"] == int(packed), (run, census)
            try:
                util.compare_partitions(ctx, parts, want)
            except AssertionError as e:
                raise AssertionError("%s, %s (partitions: %s)" % (run, e, ", ".join("p%d %s" % x for x in enumerate(names)))) from None
        labels = np.concatenate([o["labels"].ravel() for o in want]) + ord("0")
        assert np.array_equal(ctx.results(packed=True)[3], util.pack_labels(labels))
        assert np.array_equal(ctx.download()[3], labels)
    finally:
        ctx.close()
