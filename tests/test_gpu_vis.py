"""Segmentation-visualisation script on the GPU: the drop-in CLI (py/freddie_segment_vis.py) in a child process against what
the reference script wrote for the fixture inputs (tests/golden/vis/) and against a literal statement of the script
(tests/vis_util.py) -- pickle bytes, stdout, exit status, no output file on error -- and
the library (include/freddie_vis.h) against the vectorised numpy statement on a seeded fuzz and on the chromosome-wide case of
tools/vis_bench.py; malformed input gives a status."""
import ctypes
import hashlib
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import vis_util as vu
from freddie_amd import segment_vis as sv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = vu.cases()
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vis_ctx():
    ctx = sv.Context(0)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_cli_matches_the_script(name, tmp_path):
    p = vu.write_inputs(CASES[name], tmp_path)
    stdout, exc, blob = vu.literal_main(p, sv)
    out = tmp_path / "vis.pickle"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "py", "freddie_segment_vis.py"), "-s", p["split"], "-g", p["segment"],
                        "-a", p["gtf"], "-o", str(out)], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.stdout == stdout, r.stderr
    if exc is None:
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == blob
    else:
        assert r.returncode != 0 and r.stderr.strip().splitlines()[-1].startswith(exc), r.stderr
        assert not out.exists()


@pytest.mark.parametrize("name", vu.names())
def test_cli_matches_the_reference(name, tmp_path):
    """What the reference script wrote for the fixture inputs (tests/golden/vis/): pickle bytes (the typed structure where the
    interpreter's pickle protocol differs from the one that minted them), stdout, exception, no output on error."""
    doc = vu.load(name)
    p = vu.write_inputs(vu.fixture_inputs(name, tmp_path / "in"), tmp_path)
    out = tmp_path / "vis.pickle"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "py", "freddie_segment_vis.py"), "-s", p["split"], "-g", p["segment"],
                        "-a", p["gtf"], "-o", str(out)], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.stdout == doc["stdout"], r.stderr
    if doc["exception"] is None:
        assert r.returncode == 0, r.stderr
        blob = out.read_bytes()
        assert vu.typed(pickle.loads(blob)) == doc["pickle"]
        if doc["protocol"] == pickle.DEFAULT_PROTOCOL:
            assert hashlib.sha256(blob).hexdigest() == doc["pickle_sha256"]
    else:
        assert r.returncode != 0 and r.stderr.strip().splitlines()[-1].startswith(doc["exception"]), r.stderr
        assert not out.exists()


def check(ctx, bounds, obj_chrom, iv_off, iv):
    want, bad = vu.restate(bounds, obj_chrom, iv_off, iv)
    assert bad is None
    flag_off, seg, cls = ctx.classify(bounds, obj_chrom, iv_off, iv)
    assert np.array_equal(flag_off, want[0])
    assert np.array_equal(seg, want[1])
    assert np.array_equal(cls, want[2])
    return flag_off, seg, cls


def test_fuzz_against_the_restatement(vis_ctx):
    rng = np.random.default_rng(2024)
    bounds, obj_chrom, iv_off, iv = vu.fuzz_batch(rng, 100_000)
    flag_off, seg, cls = check(vis_ctx, bounds, obj_chrom, iv_off, iv)
    assert len(seg) > 100_000 and np.all(np.bincount(cls, minlength=3) > 1000)
    # the literal statement on a sample of the small-coordinate objects
    for o in rng.choice(np.flatnonzero(obj_chrom == 0), 200, replace=False):
        ivs = [tuple(x) for x in iv[iv_off[o]:iv_off[o + 1]].tolist()]
        B = bounds[0]
        got = dict(zip(seg[flag_off[o]:flag_off[o + 1]].tolist(), cls[flag_off[o]:flag_off[o + 1]].tolist()))
        assert got == vu.literal_data(ivs, list(zip(B[:-1], B[1:])))


def test_chromosome_wide_case_against_the_restatement(vis_ctx):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import vis_bench
    reads, tx, bounds = vis_bench.make_case(4000)               # the benchmarked case itself: 2 M reads, 20 000 transcripts
    s_pos = {"chrS": set(bounds)}
    sv.switch_to_nearest(s_pos, s_pos)
    segs = sv.get_seg_track(s_pos, s_pos)
    plan = sv.Plan(segs, {"chrS": {t["tid"]: t for t in tx}}, {"chrS": reads})
    check(vis_ctx, *plan.arrays(segs))


def test_first_object_without_position_is_reported(vis_ctx):
    with pytest.raises(sv.EmptyObject) as e:
        vis_ctx.classify([[0, 10, 20]], [0, 0, 0, 0], [0, 1, 3, 3, 4], [(1, 2), (5, 5), (9, 3), (4, 5)])
    assert e.value.index == 1
    flag_off, seg, cls = vis_ctx.classify([[0, 10, 20]], [0], [0, 1], [(1, 2)])
    assert flag_off.tolist() == [0, 1] and seg.tolist() == [0] and cls.tolist() == [2]      # 1 of 10: 0.1, not below it


def test_malformed_input_gives_a_status(vis_ctx):
    L, h = vis_ctx._L, vis_ctx._h
    bad = ctypes.c_int64(0)

    def call(bound_off, bounds, obj_chrom, iv_off, iv):
        arrs = [np.ascontiguousarray(a, t) for a, t in ((bound_off, np.int64), (bounds, np.int32), (obj_chrom, np.int32),
                                                        (iv_off, np.int64), (iv, np.int32))]
        return L.fvis_classify(h, len(bound_off) - 1, arrs[0].ctypes.data, arrs[1].ctypes.data, len(obj_chrom), arrs[2].ctypes.data,
                               arrs[3].ctypes.data, arrs[4].ctypes.data, ctypes.byref(bad))

    assert call([0, 3], [0, 10, 10], [0], [0, 1], [1, 2]) == 3 and bad.value == 0          # not strictly ascending
    assert call([0, 2, 4], [0, 5, 9, 3], [1], [0, 1], [1, 2]) == 3 and bad.value == 1
    assert call([0, 3], [0, 10, 20], [1], [0, 1], [1, 2]) == 1                             # chromosome index out of range
    assert call([0, 3], [0, 10, 20], [-1], [0, 1], [1, 2]) == 1
    assert call([0, 3], [0, 10, 20], [0, 0], [0, 2, 1], [1, 2, 3, 4]) == 1                 # offsets not monotone
    assert call([1, 3], [0, 10, 20], [0], [0, 1], [1, 2]) == 1                             # offsets not starting at 0
    assert call([0, 3], [0, 10, 20], [0], [0, 1], [5, 5]) == 4 and bad.value == 0          # no position
    assert L.fvis_classify(h, 1, None, None, 0, None, None, None, ctypes.byref(bad)) == 1
    assert "offsets" in L.fvis_last_error(h).decode() or "null" in L.fvis_last_error(h).decode()
    flag_off, seg, cls = vis_ctx.classify([[0, 10, 20]], [0], [0, 1], [(3, 15)])            # the context still works
    assert seg.tolist() == [0, 1] and cls.tolist() == [2, 2]


def test_source_hash_matches_the_tree():
    from freddie_amd import build
    assert sv.load().fvis_source_hash().decode() == sv.source_hash() == build.embedded_hash(sv.VIS_SO)
