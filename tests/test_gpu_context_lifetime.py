"""A context closed in every state its destructor has to cope with (``-m gpu``): fresh, parameters only, uploaded, a run enqueued and
not waited for, a live graph, profiling events in use, annotate's arenas allocated, side streams used by a run that forked.  After
every close a new context must still compute the oracle's results, and so must 32 contexts made, run and closed in a row.  One
process, no timing, no memory accounting (the device is shared): what a wrong order of release does is fault or corrupt a later run."""
import numpy as np
import pytest

import annotate_util as au
import util
from freddie_amd import _host, _lib, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small():
    parts = [util.make_partition(93000 + i, n_reads=60, n_exons=40) for i in range(2)]
    return parts, [util.run_oracle(p) for p in parts]


def _run_and_compare(small):
    ctx = _lib.Context(0)
    try:
        util.run_gpu(ctx, small[0])
        assert util.compare_partitions(ctx, *small)["y_identical"]
    finally:
        ctx.close()


def _set_params(ctx):
    ctx.set_params(**util.DEFAULTS, **util.param_tables(util.DEFAULTS))


def _fresh(ctx, small, tmp_path):
    pass


def _params_only(ctx, small, tmp_path):
    _set_params(ctx)


def _uploaded(ctx, small, tmp_path):
    from freddie_amd import pack
    _set_params(ctx)
    ctx.upload(**pack.concat_batch(small[0]))


def _run_in_flight(ctx, small, tmp_path):
    _uploaded(ctx, small, tmp_path)
    ctx.run()                                    # (no sync: the close has to wait for it)


def _graph_alive(ctx, small, tmp_path):
    util.run_gpu(ctx, small[0])
    ctx.run(); ctx.sync()                        # a small batch keeps to one stream: the replay is a graph
    assert util.compare_partitions(ctx, *small)["y_identical"]
    ctx.run()                                    # ... and one more launch of it in flight


def _profiling(ctx, small, tmp_path):
    ctx.set_profiling(True)
    util.run_gpu(ctx, small[0])
    ctx.run(); ctx.sync()                        # two graphs with the scoring stage's events between them
    ms = ctx.stage_ms()
    assert ms["graph_pre"] > 0 and ms["graph_post"] > 0, ms


def _annotated(ctx, small, tmp_path):
    d = str(tmp_path / "in")
    fp, rows = au.cigar_partition(d)
    rows[3] = 0                                  # (read 3's CIGAR ends short of its goal: a status, not what this test is about)
    hb = _host.HostBatch(*[[p] for p in au.case_paths(d, "c", 9)])
    try:
        _set_params(ctx)
        ctx.upload(**hb.arrays())
        ann = ctx.annotate(hb.read_arrays(), labels=(np.array([0, len(fp)]), fp, np.array([0, rows.size]), au.pack2(rows)))
        assert len(ann["tail"]) == 8
    finally:
        hb.close()


def _forked(ctx, small, tmp_path):
    kw = dict(synth.WORKLOADS["config4"]); kw.pop("n_partitions")
    util.run_gpu(ctx, [util.make_partition(93100 + i, **kw) for i in range(70)])
    ctx.run(); ctx.sync()                        # the list sizes are known now: alone on the device, the scoring stage takes a plan
    assert ctx.paths()["plan"] == 1


STATES = [_fresh, _params_only, _uploaded, _run_in_flight, _graph_alive, _profiling, _annotated, _forked]


@pytest.mark.parametrize("state", STATES, ids=[f.__name__[1:] for f in STATES])
def test_close_in_every_state_then_a_new_context_is_right(state, small, tmp_path):
    ctx = _lib.Context(0)
    try:
        state(ctx, small, tmp_path)
    finally:
        ctx.close()
    _run_and_compare(small)


def test_32_contexts_made_run_and_closed_in_a_row(small):
    for _ in range(32):
        _run_and_compare(small)
