"""fseg_annotate on the GPU: per-read unaligned gaps, clips and poly tails against the reference's segment TSV bytes (goldens) and
against the Python mirror of get_unaligned_gaps_and_polyA() (crafted poly clips, label rows that no segmentation produces)."""
import re

import numpy as np
import pytest

import annotate_util as au
import goldens
from freddie_amd import _host, _lib, segment, synth
from test_host_mirror import NAMES, input_dir
from test_host_native import craft_poly_clips

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _open(names, tmp_path, n_threads=2):
    sps, rps, gs = [], [], []
    for n in names:
        d, contig, tid = input_dir(n, tmp_path)
        sp, rp = au.case_paths(d, contig, tid)
        sps.append(sp); rps.append(rp); gs.append(goldens.load(n))
    return _host.HostBatch(sps, rps, n_threads=n_threads), gs


def _run_annotate_write(ctx, hb, g, tmp_path, n_out):
    ctx.set_params(**goldens.params_of(g), **goldens.tables_of(g))
    ctx.upload(**hb.arrays())
    ctx.run()
    ann = ctx.annotate(hb.read_arrays(n_threads=2))
    res = ctx.results(packed=True)
    outs = [str(tmp_path / ("out%d.tsv" % i)) for i in range(n_out)]
    hb.write_annotated(*res, ann, outs, n_threads=2)
    return [open(o, "rb").read() for o in outs]


@pytest.mark.parametrize("name", NAMES)
def test_goldens_end_to_end(name, ctx, tmp_path):
    hb, (g,) = _open([name], tmp_path)
    try:
        assert _run_annotate_write(ctx, hb, g, tmp_path, 1)[0] == g["segment_tsv"].tobytes()
    finally:
        hb.close()


def _same_params(names):
    ref = goldens.load("g1_dense")
    key = lambda g: (sorted(goldens.params_of(g).items()), [v.tolist() for v in goldens.tables_of(g).values()])     # noqa: E731
    return [n for n in names if key(goldens.load(n)) == key(ref)]


@pytest.mark.parametrize("label_bytes", [False, True])
def test_several_goldens_as_one_batch(label_bytes, tmp_path, monkeypatch):
    names = _same_params(NAMES)
    assert len(names) >= 3 and "g1_dense" in names
    if label_bytes:
        monkeypatch.setenv("FSEG_LABEL_BYTES", "1")
    c = _lib.Context(0)
    hb, gs = _open(names, tmp_path, n_threads=3)
    try:
        got = _run_annotate_write(c, hb, gs[0], tmp_path, len(names))
        assert c.paths()["label_packed"] == (0 if label_bytes else 1)
        for n, b, g in zip(names, got, gs):
            assert b == g["segment_tsv"].tobytes(), n
    finally:
        hb.close()
        c.close()


@pytest.mark.parametrize("seed", [31, 32])
def test_crafted_poly_clips_match_the_mirror(seed, ctx, tmp_path):
    import util
    d = str(tmp_path / "in")
    synth.generate(seed, write_dir=d, n_reads=240, n_exons=30, rp=0.1)
    craft_poly_clips(d, "chrS", seed, seed)
    tint = segment._load_partition(d, "chrS", seed)
    sp, rp = au.case_paths(d, "chrS", seed)
    hb = _host.HostBatch([sp], [rp])
    try:
        util.run_gpu(ctx, [segment.pack_tint(tint)])
        pfo, fp, lo, lab = ctx.download()
        got = {k: v.copy() for k, v in ctx.annotate(hb.read_arrays()).items()}
        want, raised = au.mirror_annotation(tint, fp, (lab - 48).reshape(-1, len(fp) - 1))
        assert not any(raised)
        au.assert_annotation_equal(got, want)
        assert all((got["polys"][:, 0] == k).sum() >= 3 for k in range(4)), np.bincount(got["polys"][:, 0], minlength=4)
        # the same through segment_batch(gaps="gpu"): the token strings of the mirror
        t2 = segment._load_partition(d, "chrS", seed)
        p = util.DEFAULTS
        segment.segment_batch([t2], p["sigma"], util.param_tables(p)["h_table"], p["threshold_rate"], p["variance_factor"], p["max_problem_size"],
                              p["min_read_support_outside"], p["ignore_ends"], ctx=ctx, gaps="gpu")
        assert [list(r["gaps"]) for r in t2["reads"]] == [list(r["gaps"]) for r in tint["reads"]]
    finally:
        hb.close()


def _override(ctx, hb, tint, fp, rows):
    """Annotates the label rows `rows` (one per rep) and checks them against the mirror: equal arrays, or -- when the mirror raises on
    a read -- FSEG_ERR_INPUT naming the smallest such read, after which the rows of the raising reads' reps are cleared and the call
    is made again.  Returns how many reads raised."""
    S = len(fp) - 1
    n_raised = 0
    for _ in range(len(rows) + 1):
        want, raised = au.mirror_annotation(tint, fp, rows)
        labels = (np.array([0, len(fp)]), fp, np.array([0, rows.size]), au.pack2(rows))
        bad = [i for i, e in enumerate(raised) if e is not None]
        if not bad:
            au.assert_annotation_equal(ctx.annotate(hb.read_arrays(), labels=labels), want)
            return n_raised
        n_raised += len(bad)
        with pytest.raises(_lib.SegError) as ei:
            ctx.annotate(hb.read_arrays(), labels=labels)
        assert ei.value.code == _lib.ERR_INPUT
        m = re.search(r"partition 0, read (\d+): .*\(:\d+", str(ei.value))
        assert m and int(m.group(1)) == bad[0], (str(ei.value), bad[0], raised[bad[0]])
        rows = rows.copy()
        for ri, (_, ridxs) in enumerate(tint["read_reps"]):
            if set(ridxs) & set(bad):
                rows[ri] = 0
    raise AssertionError("the rows kept raising")


def test_label_rows_no_segmentation_produces(ctx, tmp_path):
    name = "g1_dense"
    g = goldens.load(name)
    d, contig, tid = input_dir(name, tmp_path)
    tint = segment._load_partition(d, contig, tid)
    sp, rp = au.case_paths(d, contig, tid)
    hb = _host.HostBatch([sp], [rp])
    try:
        ctx.set_params(**goldens.params_of(g), **goldens.tables_of(g))
        ctx.upload(**hb.arrays())
        fp = g["final_positions"]
        R, S = g["labels"].shape
        assert S >= 6
        hand = [np.zeros(S, np.uint8), np.ones(S, np.uint8), np.eye(1, S, 0, dtype=np.uint8)[0], np.eye(1, S, S - 1, dtype=np.uint8)[0],
                (np.arange(S) % 2 == 0).astype(np.uint8), np.where(np.arange(S) % 3 == 0, 1, 2).astype(np.uint8)]
        n_raised = 0
        for row in hand:
            n_raised += _override(ctx, hb, tint, fp, np.tile(row, (R, 1)))
        rng = np.random.default_rng(5)
        n_rows = 0
        while n_rows < 200:                              # a random row per rep and call
            density = rng.choice([0.05, 0.3, 0.6, 0.9])
            rows = np.where(rng.random((R, S)) < density, 1, rng.integers(0, 3, (R, S))).astype(np.uint8)
            rows[:, rng.integers(0, S)] = 1
            n_raised += _override(ctx, hb, tint, fp, rows)
            n_rows += R
        print("reads on which the mirror raised:", n_raised)
        # the context is usable afterwards: the golden's own run and annotation
        assert _run_annotate_write(ctx, hb, g, tmp_path, 1)[0] == g["segment_tsv"].tobytes()
    finally:
        hb.close()


def test_argument_errors_name_the_read(ctx, tmp_path):
    name = "g_tiny"
    g = goldens.load(name)
    hb, _ = _open([name], tmp_path)
    try:
        ctx.set_params(**goldens.params_of(g), **goldens.tables_of(g))
        ctx.upload(**hb.arrays())
        ctx.run()
        good = {k: v.copy() for k, v in hb.read_arrays().items()}
        n = len(good["read_part"])
        assert n >= 4

        def bad(key, idx, value, match):
            a = dict(good)
            a[key] = good[key].copy()
            a[key][idx] = value
            with pytest.raises(_lib.SegError, match=match) as ei:
                ctx.annotate(a)
            assert ei.value.code == _lib.ERR_ARG
        bad("seq_off", 3, good["seq_off"][2] - 16, r"read 2: seq_off does not ascend")
        bad("read_q_off", 2, good["read_q_off"][1] - 1, r"read 1: read_q_off does not ascend")
        bad("read_rep", 3, len(g["rep_weight"]), r"read 3: rep %d is beyond the %d reps of partition 0" % (len(g["rep_weight"]), len(g["rep_weight"])))
        bad("read_part", 1, 1, r"read 1: partition 1 is outside the batch")
        bad("read_q_off", 2, good["read_q_off"][2] + 1, r"read 1: read_q_off spans \d+ exons, its rep has \d+")
        bad("strand", 2, ord("x"), r"read 2: strand is neither")
        ann = ctx.annotate(good)                         # and the context still annotates
        assert len(ann["tail"]) == n
    finally:
        hb.close()


def test_cli_annotate_gpu_gives_the_recorded_hashes(tmp_path):
    """py/freddie_segment.py --annotate gpu on the inputs of tests/golden/g5_cli_hashes.json: every output hashes to what the
    reference CLI wrote, from the TSVs (first pass, which also writes the side-cars) and from the side-cars (second pass)."""
    import hashlib
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    doc = json.load(open(os.path.join(goldens.GOLDEN_DIR, "g5_cli_hashes.json")))
    gen = doc["generator"]
    d = str(tmp_path / "in")
    for i in range(gen["n_partitions"]):
        synth.generate(i, n_reads=gen["n_reads"], n_exons=gen["n_exons"], rp=gen["rp"], write_dir=d)
    for mode in ("write", "auto"):
        out = str(tmp_path / mode)
        cmd = [sys.executable, os.path.join(root, "py", "freddie_segment.py"), "-s", d, "-o", out, "--gpus", "1", "-t", "4",
               "--batch-reads", "20000", "--annotate", "gpu", "--sidecar", mode]
        res = subprocess.run(cmd, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-2000:]
        bad = [f for f, want in doc["outputs"].items()
               if hashlib.sha256(open(os.path.join(out, "chrS", f), "rb").read()).hexdigest() != want]
        assert not bad, "%s: %d of %d outputs differ from the reference, e.g. %s" % (mode, len(bad), len(doc["outputs"]), bad[:3])
    assert any(f.endswith(".fsc") for f in os.listdir(os.path.join(d, "chrS")))


def test_cigar_threading_and_poly_windows_by_hand(ctx, tmp_path):
    """annotate_util.cigar_partition(): I / D / X / = ops, a goal inside an I-then-M pair, a CIGAR that ends short of the goal (a status,
    no fault), windows of 19 / 20 / 21 letters, purity exactly 17 / 20, an A and a T run of equal purity, a '-' read whose window
    reaches index 0 -- against the mirror, and against the tokens worked out by hand."""
    d = str(tmp_path / "in")
    fp, rows = au.cigar_partition(d)
    tint = segment._load_partition(d, "c", 9)
    assert len(tint["read_reps"]) == len(rows) == 8
    sp, rp = au.case_paths(d, "c", 9)
    hb = _host.HostBatch([sp], [rp])
    try:
        util_params = dict(sigma=5.0, threshold_rate=0.9, variance_factor=3.0, max_problem_size=50, min_read_support_outside=3, ignore_ends=True)
        import util
        ctx.set_params(**util_params, **util.param_tables(util_params))
        ctx.upload(**hb.arrays())
        assert _override(ctx, hb, tint, fp, rows) == 1            # read 3: forward_thread_cigar's CIGAR runs out (:293)
        rows[3] = 0
        ann = ctx.annotate(hb.read_arrays(), labels=(np.array([0, len(fp)]), fp, np.array([0, rows.size]), au.pack2(rows)))
        assert [segment.annotation_tokens(ann, r) for r in range(8)] == [
            ["1-4:50", "ESC:19", "SA_20:0", "SSC:0"], ["0-2:53", "EA_20:0", "ESC:20", "SA_21:0", "SSC:0"],
            ["2-4:0", "EA_30:0", "ESC:30", "SSC:0", "ST_25:0"], [], ["ESC:25", "ET_22:0", "SA_20:21", "SSC:0"],
            ["0-2:5", "2-4:10", "ESC:5", "SSC:5"], ["1-3:10", "ESC:8", "SSC:10"], []]
    finally:
        hb.close()


def _same(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), "%s %s" % (what, k)
        else:
            assert a[k] == b[k], "%s %s" % (what, k)


@pytest.mark.parametrize("name", ["g1_retention", "g_weights_ends", "g3_ont"])
def test_seam_to_the_clustering_stage_without_files(name, ctx, tmp_path):
    """segment -> annotate -> arrays_from_segmentation against read_segment_arrays() on the TSVs the same run wrote: the arrays, the
    rep grouping, the partitions with their pair lists and the models of round 0 (every partition with all of its reps); no solver."""
    from freddie_amd import cluster_prep
    hb, (g,) = _open([name], tmp_path)
    cctx = cluster_prep.Context(0)
    try:
        ctx.set_params(**goldens.params_of(g), **goldens.tables_of(g))
        ctx.upload(**hb.arrays())
        ctx.run()
        ann = ctx.annotate(hb.read_arrays())
        res = ctx.results(packed=True)
        out = str(tmp_path / "segment_x_1.tsv")
        hb.write_annotated(*res, ann, [out])
        want = cluster_prep.read_segment_arrays([out], mirror=False)
        assert not want.declined
        got = cluster_prep.arrays_from_segmentation(hb, res, ann)
        au.assert_segment_arrays_equal(got, want, name)
        _same(cctx.group_reads(got), cctx.group_reads(want), "groups")
        want.a = au.gaps_by_j1(want.a)                   # (round_gaps() lists a rep's gaps in its dict's order)
        sides = []
        for arrays in (got, want):
            groups, prep, arr = cctx.partition_segment(arrays, 1000)
            tints = cluster_prep.tints_from_arrays(arrays, groups, prep, arr, dict(recycle_model="constant"))
            cctx.round_setup(*cluster_prep.round_gaps(tints))
            n_parts = int(arr["tint_part_off"][-1])
            rem = [list(p[0]) for t in tints for p in t["partitions"]]
            assert len(rem) == n_parts
            sides.append((groups, prep, arr, cctx.round_models(list(range(n_parts)), rem)))
        for k, what in enumerate(("groups", "prep", "partitions", "round models")):
            _same(sides[0][k], sides[1][k], what)
        want.close()
    finally:
        hb.close()
        cctx.close()
