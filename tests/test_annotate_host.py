"""The host side of the device annotation (no GPU): fhost_write_annotated formats an annotation that is GIVEN -- here made by the
Python mirror on the goldens' labels -- into the reference's segment TSV bytes, and HostBatch.read_arrays() hands the per-read
arrays over in fseg_reads' layout, from TSVs and from side-cars alike."""
import numpy as np
import pytest

import annotate_util as au
import goldens
from freddie_amd import _host, segment, synth
from test_host_mirror import NAMES, input_dir
from test_host_native import craft_poly_clips


def _write_annotated(sp, rp, final_positions, labels, ann, out, sidecar=None):
    hb = _host.HostBatch([sp], [rp], n_threads=2, sidecar_paths=sidecar)
    try:
        F = len(final_positions)
        hb.write_annotated(np.array([0, F]), final_positions, np.array([0, np.asarray(labels).size]), au.pack2(labels), ann, [out], n_threads=2)
    finally:
        hb.close()
    return open(out, "rb").read()


@pytest.mark.parametrize("name", NAMES)
def test_annotated_writer_gives_the_reference_bytes(name, tmp_path):
    g = goldens.load(name)
    d, contig, tid = input_dir(name, tmp_path)
    tint = segment._load_partition(d, contig, tid)
    ann, raised = au.mirror_annotation(tint, g["final_positions"], g["labels"])
    assert not any(raised)
    sp, rp = au.case_paths(d, contig, tid)
    assert _write_annotated(sp, rp, g["final_positions"], g["labels"], ann, str(tmp_path / "out.tsv")) == g["segment_tsv"].tobytes()


def test_annotated_writer_does_not_depend_on_the_order_of_a_reads_gaps(tmp_path):
    name = "g3_ont"
    g = goldens.load(name)
    d, contig, tid = input_dir(name, tmp_path)
    tint = segment._load_partition(d, contig, tid)
    ann, _ = au.mirror_annotation(tint, g["final_positions"], g["labels"])
    gaps = ann["gaps"].copy()
    for r in range(len(ann["tail"])):
        a, b = ann["gap_off"][r], ann["gap_off"][r + 1]
        gaps[a:b] = gaps[a:b][::-1]
    assert not np.array_equal(gaps, ann["gaps"])
    sp, rp = au.case_paths(d, contig, tid)
    assert _write_annotated(sp, rp, g["final_positions"], g["labels"], dict(ann, gaps=gaps), str(tmp_path / "out.tsv")) == g["segment_tsv"].tobytes()


@pytest.mark.parametrize("seed", [31, 32])
def test_annotated_writer_on_crafted_poly_clips(seed, tmp_path):
    import util
    d = str(tmp_path / "in")
    synth.generate(seed, write_dir=d, n_reads=240, n_exons=30, rp=0.1)
    craft_poly_clips(d, "chrS", seed, seed)
    tint = segment._load_partition(d, "chrS", seed)
    o = util.run_oracle(segment.pack_tint(tint))
    assert o["error"] == 0
    ann, raised = au.mirror_annotation(tint, o["final_pos"], o["labels"])
    assert not any(raised)
    assert len(ann["polys"]) >= 25 and all((ann["polys"][:, 0] == k).sum() >= 3 for k in range(4))
    want = tmp_path / "want.tsv"
    segment.write_segment_tsv(tint, str(want))
    sp, rp = au.case_paths(d, "chrS", seed)
    assert _write_annotated(sp, rp, o["final_pos"], o["labels"], ann, str(tmp_path / "got.tsv")) == want.read_bytes()


def _check_read_arrays(ra, tint):
    part = segment.pack_tint(tint)
    n = len(tint["reads"])
    assert len(ra["read_part"]) == n and not ra["read_part"].any()
    assert np.array_equal(ra["read_rep"], part.read_rep)
    assert np.array_equal(ra["read_id"], [r["id"] for r in tint["reads"]])
    assert bytes(ra["strand"]).decode() == "".join(r["strand"] for r in tint["reads"])
    assert np.array_equal(ra["seq_len"], [r["length"] for r in tint["reads"]])
    assert np.array_equal(ra["read_q_off"], np.concatenate([[0], np.cumsum([len(r["intervals"]) for r in tint["reads"]])]))
    iv = [x for r in tint["reads"] for x in r["intervals"]]
    assert np.array_equal(ra["qs"], [x[2] for x in iv]) and np.array_equal(ra["qe"], [x[3] for x in iv])
    assert np.array_equal(ra["cig_off"], np.concatenate([[0], np.cumsum([len(x[4]) for x in iv])]))
    assert np.array_equal(ra["cig_len"], [ln for x in iv for ln, _ in x[4]])
    assert bytes(ra["cig_op"]).decode() == "".join(op for x in iv for _, op in x[4])
    assert not (ra["seq_off"] % 16).any() and (np.diff(ra["seq_off"]) >= ra["seq_len"]).all()
    for r, read in enumerate(tint["reads"]):
        b = np.frombuffer(read["seq"].encode(), np.uint8)
        want = np.where(b == ord("A"), 0, np.where(b == ord("T"), 1, 2))                      # the one-line restatement
        w = ra["seq_classes"][ra["seq_off"][r] // 16:ra["seq_off"][r + 1] // 16]
        got = ((w[:, None] >> (2 * np.arange(16, dtype=np.uint32))) & 3).ravel()
        assert np.array_equal(got[:len(b)], want) and not got[len(b):].any(), r


@pytest.mark.parametrize("name", ["e_one_rep", "g_tiny", "g1_dense", "g3_ont"])
def test_read_arrays_match_the_python_parser(name, tmp_path):
    d, contig, tid = input_dir(name, tmp_path)
    tint = segment._load_partition(d, contig, tid)
    sp, rp = au.case_paths(d, contig, tid)
    sc = sp[:-4] + ".fsc"
    hb = _host.HostBatch([sp], [rp], n_threads=2)
    a0 = {k: v.copy() for k, v in hb.read_arrays(n_threads=2).items()}
    hb.write_sidecars([sc]); hb.close()
    _check_read_arrays(a0, tint)
    hb = _host.HostBatch([sp], [rp], sidecar_paths=[sc])
    assert hb.n_from_sidecar == 1
    a1 = hb.read_arrays()
    for k in a0:
        assert np.array_equal(a0[k], a1[k]), k
    hb.close()


def test_read_arrays_class_codes_of_non_acgt_bytes(tmp_path):
    """The fixture of test_sidecar_keeps_non_acgt_bytes: N, lower case and IUPAC letters are class 2 from the TSV and from the
    side-car's exception list alike (a packed exception holds code 0, which would read as 'A')."""
    sp = tmp_path / "split_c_7.tsv"; rp = tmp_path / "reads_c_7.tsv"
    seqs = ["ACGTNNacgtRYKM" + "A" * 30 + "N" + "A" * 5 + "CCCC" * 30 + "t" * 25, "T" * 26 + "G" * 140 + "N", "n" + "ACGT" * 40]
    lines = ["#c\t7\t100-300\t3\n"]
    for i in range(3):
        lines.append("%d\tr%d\tc\t%s\t7\t120-180:40-100:60M\t200-260:100-160:60M\n" % (i, i, "+-"[i % 2]))
    sp.write_text("".join(lines))
    rp.write_text("".join("%d\tc\t7\t%s\n" % (i, s) for i, s in enumerate(seqs)))
    tint = segment.read_split(str(sp))[0]
    segment.read_sequence(tint, str(rp))
    sc = str(tmp_path / "split_c_7.fsc")
    hb = _host.HostBatch([str(sp)], [str(rp)])
    a0 = {k: v.copy() for k, v in hb.read_arrays().items()}
    hb.write_sidecars([sc]); hb.close()
    _check_read_arrays(a0, tint)
    hb = _host.HostBatch([str(sp)], [str(rp)], sidecar_paths=[sc])
    assert hb.n_from_sidecar == 1
    a1 = hb.read_arrays()
    for k in a0:
        assert np.array_equal(a0[k], a1[k]), k
    hb.close()
    assert np.array_equal(segment.read_arrays_from_tints([tint], [segment.pack_tint(tint)])["seq_classes"], a0["seq_classes"])


@pytest.mark.parametrize("name", NAMES)
def test_arrays_from_segmentation_equal_the_native_reader(name, tmp_path):
    """The in-memory seam: SegmentArrays built from the batch, the packed results and a (mirror-made) annotation equal what the
    native reader makes of the golden's segment TSV, field by field, every read's gaps in ascending j1 on both sides."""
    from freddie_amd import cluster_prep
    g = goldens.load(name)
    d, contig, tid = input_dir(name, tmp_path)
    tint = segment._load_partition(d, contig, tid)
    ann, _ = au.mirror_annotation(tint, g["final_positions"], g["labels"])
    tsv = tmp_path / ("segment_%s_%d.tsv" % (contig, tid))
    tsv.write_bytes(g["segment_tsv"].tobytes())
    want = cluster_prep.read_segment_arrays([str(tsv)], mirror=False)
    assert not want.declined
    sp, rp = au.case_paths(d, contig, tid)
    hb = _host.HostBatch([sp], [rp])
    try:
        F = len(g["final_positions"])
        got = cluster_prep.arrays_from_segmentation(hb, (np.array([0, F]), g["final_positions"], np.array([0, g["labels"].size]), au.pack2(g["labels"])), ann)
        au.assert_segment_arrays_equal(got, want, name)
    finally:
        hb.close()
        want.close()
