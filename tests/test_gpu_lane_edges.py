"""The built cases of tests/lane_cases.py on the device: fseg_upload's preparation (k_prep_reps; k_lanes with its sort in LDS; the radix
sort with k_lane_blocks / k_lane_block_scan / k_lane_emit; lex_copy_tile; k_hist_ranges) against the numpy model, with ==.  Every batch
runs under the default and under FSEG_GLOBAL_SORT=1 -- the flag is read by fseg_create, so each switch set has a context of its own,
made after the variable is set -- and on the first run and on a replay the taps lane_start, lane_pmax, lane_exons, lane_stream,
exon_stream and hist_ranges must equal the model's arrays, hist_ranges' p0 and n the chunking tests/test_lane_cases_host.py computes
from seg_common.h's constants, and the census words lane_sort and hist16 what the batch and the switch decide.  Every batch then
goes through util.compare_partitions against the oracle (under ignore_ends=False, so that single-exon reps count), which consumes
the lists: a lane range that hides a read loses its counts.  That includes B-65837, the batch of 65 837 partitions: the oracle runs
on its seven distinct partitions, the device run takes 0.1 s and the comparison's Python loop 1.7 s (measured on an MI355X machine).

Group V: accepted batches run like the others; refused ones must come back as FSEG_ERR_INPUT with the rule's message and the rep the
validation model names, exactly, and the context then takes a good batch (lane_cases' docstring: these are status returns)."""
import numpy as np
import pytest

import lane_cases as lc
import util
from freddie_amd import _lib

pytestmark = pytest.mark.gpu

SWITCHES = {"default": None, "global-sort": "1"}
ERR_INPUT = 3            # FSEG_ERR_INPUT (include/freddie_seg.h)


@pytest.fixture(scope="module", params=list(SWITCHES))
def lane_ctx(request):
    mp = pytest.MonkeyPatch()
    for k in ("FSEG_GLOBAL_SORT", "FSEG_HIST16", "FSEG_YRAW16"):
        mp.delenv(k, raising=False)
    if SWITCHES[request.param]:
        mp.setenv("FSEG_GLOBAL_SORT", SWITCHES[request.param])
    ctx = _lib.Context(0)
    yield ctx, SWITCHES[request.param] is not None
    ctx.close()
    mp.undo()


def assert_taps(ctx, forced, want, what):
    for k in lc.TAPS:
        got = ctx.tap(k)
        assert got.shape == want[k].shape, "%s: %s has shape %r, the model %r" % (what, k, got.shape, want[k].shape)
        bad = np.flatnonzero((got != want[k]).reshape(len(got), -1).any(axis=1)) if len(got) else []
        assert not len(bad), "%s: %s differs in %d rows, first %d: %r, model %r" % (what, k, len(bad), bad[0], got[bad[0]], want[k][bad[0]])
    census = ctx.paths()
    assert census["lane_sort"] == (1 if forced else want["lane_sort"]), (what, census)
    assert census["hist16"] == want["hist16"], (what, census)


def check_batch(ctx, forced, name):
    parts, params = lc.batch(name)
    want = lc.model_batch(parts)
    util.run_gpu(ctx, parts, params)
    assert_taps(ctx, forced, want, name + ", first run")
    util.compare_partitions(ctx, parts, lc.oracles(name))
    ctx.run(); ctx.sync()
    assert_taps(ctx, forced, want, name + ", replay")
    return want


@pytest.mark.parametrize("name", lc.BATCHES)
def test_lane_batches(lane_ctx, name):
    ctx, forced = lane_ctx
    want = check_batch(ctx, forced, name)
    # what the names promise about the path, literally
    if name in ("N-all+2049", "M-2049", "M-16385", "M-16640"):
        assert want["lane_sort"] == 1
    if name.startswith("N-") and name != "N-all+2049" or name in ("M-300", "W", "X", "H-1024", "H-full") or name.startswith("B-"):
        assert want["lane_sort"] == 0 and ctx.paths()["lane_sort"] == int(forced)
    if name == "W":
        assert want["hist16"] == 0
    if name == "H-full":
        assert want["chunk"] == lc.CHUNK16
    if name == "B-%d" % lc.B_LARGE:
        assert want["chunk"] == 4096 and len(want["hist_ranges"]) == lc.B_LARGE


@pytest.mark.parametrize("name", list(lc.REFUSALS))
def test_refused_batches_name_the_rule_and_the_rep(lane_ctx, name):
    ctx, forced = lane_ctx
    for where in lc.PLACES:
        bad = lc.refused(name, where)
        rule, rep = lc.verdict(bad)
        assert rule == lc.REFUSALS[name][0]
        with pytest.raises(_lib.SegError) as e:
            util.run_gpu(ctx, bad, lc.ENDS)
        assert e.value.code == ERR_INPUT and str(e.value).endswith("(%d): %s" % (ERR_INPUT, lc.MESSAGES[rule] % rep)), (where, str(e.value))
        check_batch(ctx, forced, "V-base")


@pytest.mark.parametrize("name", list(lc.PAIRS))
def test_the_smaller_of_two_bad_reps_is_named(lane_ctx, name):
    ctx, forced = lane_ctx
    bad = lc.spoiled(lc.v_base(False), lc.PAIRS[name])
    rule, rep = lc.verdict(bad)
    assert rep == min(lc.PAIRS[name])
    with pytest.raises(_lib.SegError) as e:
        util.run_gpu(ctx, bad, lc.ENDS)
    assert e.value.code == ERR_INPUT and str(e.value).endswith("(%d): %s" % (ERR_INPUT, lc.MESSAGES[rule] % rep)), str(e.value)
    check_batch(ctx, forced, "V-base")
