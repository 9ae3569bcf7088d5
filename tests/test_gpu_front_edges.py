"""S2-S4 at their edges, on the device: k_smooth's three instances and k_peaks_edges on plateaus laid over tile edges and on
intervals around the radius, the quad and the tile; k_fix and k_segments with 63 .. 1 100 candidates per interval under each of
their three block sizes.  The cases are tests/edge_cases.py's (tests/test_edge_cases_host.py shows by the oracle alone that they
reach the edges they are named after); every tap is compared with the CPU oracle on the first run and on the replay, and the
census says which instance and which block size ran."""
import pytest

import edge_cases as ec
import util
from freddie_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("odd_first", [False, True], ids=["aligned", "behind-37"])
@pytest.mark.parametrize("sigma", ec.PLATEAU_SIGMAS)
def test_plateaus_over_tile_edges(sigma, odd_first):
    ec.run_on_gpu("plateau", sigma, odd_first, smooth_r=ec.SMOOTH_R[sigma], iv_threads=64)


def test_plateaus_of_two_and_three_positions_under_radius_zero():
    ec.run_on_gpu("twins0", smooth_r=0, iv_threads=64)


@pytest.mark.parametrize("sigma", ec.PLATEAU_SIGMAS)
def test_interval_lengths_around_radius_quad_and_tile(sigma):
    ec.run_on_gpu("length", sigma, smooth_r=ec.SMOOTH_R[sigma], iv_threads=64)


def test_interval_of_one_position_is_refused():
    """start == end: read_split's assert (:140) in the reference, FSEG_ERR_INPUT on upload here."""
    names, parts, params = ec.case("one_position")
    ctx = _lib.Context(0)
    try:
        with pytest.raises(_lib.SegError, match="start >= end"):
            util.run_gpu(ctx, parts, params)
    finally:
        ctx.close()


@pytest.mark.parametrize("mps", ec.WIDTH_MPS)
@pytest.mark.parametrize("threads", [64, 256, 1024])
def test_candidates_per_interval_against_the_block_size(threads, mps):
    ec.run_on_gpu("width", threads, mps, iv_threads=threads, smooth_r=20)


@pytest.mark.parametrize("threads", [64, 256, 1024])
def test_negative_anchor_is_refused(threads):
    """break_large_problems takes the sink's peak through index -2: the reference would add a negative index (as x_mps4: a refusal)."""
    names, parts, params = ec.case("refusal", threads)
    assert ec.oracles("refusal", threads)[0]["error"] != 0
    ctx = _lib.Context(0)
    try:
        with pytest.raises(_lib.SegError, match="break_large_problems") as e:
            util.run_gpu(ctx, parts, params)
            ctx.download()
        assert e.value.code == _lib.ERR_INPUT
    finally:
        ctx.close()
