"""Shared by tests/test_annotate_host.py and tests/test_gpu_annotate.py: fseg_annot's arrays (include/freddie_seg.h) made from the
Python mirror of get_unaligned_gaps_and_polyA(), and the inputs of a golden case as a native batch."""
import os
import re

import numpy as np

import goldens
from freddie_amd import segment

_GAP = re.compile(r"^(\d+)-(\d+):(\d+)$")
_CLIP = re.compile(r"^([ES])SC:(\d+)$")
_POLY = re.compile(r"^([ES])([AT])_(\d+):(\d+)$")


def read_entries(tokens):
    """(gaps in j1 order, clips ESC then SSC, polys E keys then S keys, tail, key tokens) of one read's token strings."""
    gaps, clips, polys = [], [], []
    for t in sorted(tokens):                     # 'E' < 'S': the order of a TSV line
        m = _GAP.match(t)
        if m:
            gaps.append(tuple(int(x) for x in m.groups()))
            continue
        m = _CLIP.match(t)
        if m:
            clips.append((1 if m.group(1) == "E" else 0, int(m.group(2))))
            continue
        m = _POLY.match(t)
        assert m, t
        polys.append(((2 if m.group(1) == "E" else 0) + (1 if m.group(2) == "T" else 0), int(m.group(3)), int(m.group(4))))
    gaps.sort()
    tail = 0
    if len(polys) == 1 and polys[0][1] > 10:
        tail = 2 if polys[0][0] >= 2 else 1
    tok = [ln if ln > 10 else 0 for _, _, ln in gaps]
    tok += [0x80000000 | (0x40000000 if k >= 2 else 0) | (gap if gap > 10 else 0) for k, _, gap in polys]
    return gaps, clips, polys, tail, tok


def annotation_from_tokens(per_read_tokens):
    """fseg_annot's arrays by name from one iterable of token strings per read."""
    gap_off, clip_off, poly_off, tok_off = [0], [0], [0], [0]
    gaps, clips, polys, tail, tok = [], [], [], [], []
    for tokens in per_read_tokens:
        g, c, p, t, k = read_entries(tokens)
        gaps += g; clips += c; polys += p; tail.append(t); tok += k
        gap_off.append(len(gaps)); clip_off.append(len(clips)); poly_off.append(len(polys)); tok_off.append(len(tok))
    return dict(gap_off=np.array(gap_off, np.int64), gaps=np.array(gaps, np.int32).reshape(-1, 3),
                clip_off=np.array(clip_off, np.int64), clips=np.array(clips, np.int32).reshape(-1, 2),
                poly_off=np.array(poly_off, np.int64), polys=np.array(polys, np.int32).reshape(-1, 3),
                tail=np.array(tail, np.uint8), tok_off=np.array(tok_off, np.int64), tok=np.array(tok, np.uint32))


def mirror_annotation(tint, final_positions, labels):
    """Runs the mirror over a tint dict with the given final positions and per-rep label rows.  Returns (annotation arrays, [the
    exception a read raised or None])."""
    tint["final_positions"] = [int(x) for x in final_positions]
    tint["segs"] = list(zip(tint["final_positions"][:-1], tint["final_positions"][1:]))
    for ri, (_, ridxs) in enumerate(tint["read_reps"]):
        for ridx in ridxs:
            tint["reads"][ridx]["data"] = [int(x) for x in labels[ri]]
    raised, toks = [], []
    for read in tint["reads"]:
        try:
            segment.unaligned_gaps_and_polyA(read, tint["segs"])
            raised.append(None)
            toks.append(list(read["gaps"]))
        except (AssertionError, IndexError) as exc:
            raised.append(exc)
            toks.append([])
    return annotation_from_tokens(toks), raised


def assert_annotation_equal(got, want, what=""):
    for k in ("gap_off", "gaps", "clip_off", "clips", "poly_off", "polys", "tail", "tok_off", "tok"):
        assert np.array_equal(np.asarray(got[k]).reshape(np.asarray(want[k]).shape) if np.asarray(got[k]).size == np.asarray(want[k]).size
                              else got[k], want[k]), "%s %s" % (what, k)


def case_paths(d, contig, tid):
    return (os.path.join(d, contig, "split_%s_%d.tsv" % (contig, tid)), os.path.join(d, contig, "reads_%s_%d.tsv" % (contig, tid)))


def pack2(labels):
    """Label values 0 / 1 / 2 (flat) at two bits each, four to a byte (fseg_results_packed's layout)."""
    v = np.asarray(labels, np.uint8).ravel() & 3
    v = np.concatenate([v, np.zeros(-len(v) % 4, np.uint8)]).reshape(-1, 4)
    return (v[:, 0] | (v[:, 1] << 2) | (v[:, 2] << 4) | (v[:, 3] << 6)).astype(np.uint8)


def cigar_partition(d):
    """A hand-written partition for the CIGAR threading and the poly windows: writes split_c_9.tsv / reads_c_9.tsv under d/c and
    returns (final positions, one label row per read = rep).  Read by read:
      0  50M5I50M and a second exon; start clip of exactly 20 A (found), end clip of 19 A (too short)
      1  48M5I252M: the goal 150 falls inside the I-then-M pair, so the insertion is clipped to 2 (:294); start clip of 21 letters with
         one mismatch; end clip of 20 letters with purity exactly 17 / 20 = 0.85
      2  '-', 50=5X45M10D40M and a second exon that starts where the gap ends; its end window reaches index 0 of the stored sequence
      3  a CIGAR (100M) that ends 200 short of the goal: a status, never a fault
      4  start clip with an A run and a T run of equal purity (the A run wins), end clip with a T run
      5  '-', three exons under alternating labels: every boundary is a gap; clips shorter than 20
      6  exons that do not reach the segment boundaries: the slack branch at a read end and at a gap
      7  no label 1 at all"""
    import os
    fp = [100, 150, 200, 250, 300, 350, 400]
    body = lambda n, k: ("CGGC" * (n // 4 + 1))[k % 4:][:n]     # noqa: E731  (no A, no T)
    reads = [
        ("+", "100-200:20-125:50M5I50M\t250-400:125-275:150M", "A" * 20, 255, "A" * 19, [1, 1, 0, 0, 1, 1]),
        ("+", "100-400:21-326:48M5I252M", "A" * 10 + "C" + "A" * 10, 305, "A" * 5 + "C" + "A" * 4 + "C" + "A" * 4 + "C" + "A" * 4, [1, 0, 1, 1, 1, 1]),
        ("-", "100-250:25-165:50=5X45M10D40M\t300-400:165-265:100M", "T" * 30, 240, "A" * 25, [1, 1, 1, 0, 1, 1]),
        ("+", "101-400:10-200:100M", "G" * 10, 190, "C" * 12, [1, 1, 1, 0, 0, 1]),
        ("+", "100-398:41-339:298M", "A" * 20 + "G" + "T" * 20, 298, "T" * 22 + "CCC", [1, 1, 1, 1, 1, 1]),
        ("-", "100-150:5-55:50M\t200-250:60-110:50M\t300-350:120-170:50M", "TTTTT", 165, "AAAAA", [1, 0, 1, 0, 1, 0]),
        ("+", "120-180:10-70:60M\t220-380:70-230:160M", "A" * 10, 220, "T" * 8, [1, 1, 0, 1, 1, 1]),
        ("+", "100-300:0-200:200M", "", 200, "A" * 30, [0, 0, 2, 0, 0, 0]),
    ]
    os.makedirs(os.path.join(d, "c"), exist_ok=True)
    with open(os.path.join(d, "c", "split_c_9.tsv"), "w") as f:
        f.write("#c\t9\t100-400\t%d\n" % len(reads))
        for i, r in enumerate(reads):
            f.write("%d\tr%d\tc\t%s\t9\t%s\n" % (i, i, r[0], r[1]))
    with open(os.path.join(d, "c", "reads_c_9.tsv"), "w") as f:
        for i, r in enumerate(reads):
            f.write("%d\tc\t9\t%s\n" % (i, r[2] + body(r[3], i) + r[4]))
    return np.array(fp, np.int32), np.array([r[5] for r in reads], np.uint8)


def gaps_by_j1(a):
    """The arrays of a SegmentArrays with every read's gaps (and the gap part of its key tokens) in ascending j1."""
    a = dict(a)
    gaps, tok = np.array(a["gaps"]).reshape(-1, 3).copy(), np.array(a["tok"]).copy()
    for r in range(len(a["tail"])):
        g0, g1, t0 = int(a["gap_off"][r]), int(a["gap_off"][r + 1]), int(a["tok_off"][r])
        order = np.argsort(gaps[g0:g1, 0], kind="stable")
        gaps[g0:g1] = gaps[g0:g1][order]
        tok[t0:t0 + g1 - g0] = tok[t0:t0 + g1 - g0][order]
    a["gaps"], a["tok"] = gaps, tok
    return a


def assert_segment_arrays_equal(got, want, what=""):
    g, w = gaps_by_j1(got.a), gaps_by_j1(want.a)
    assert sorted(g) == sorted(w), what
    for k in w:
        assert np.array_equal(np.asarray(g[k]).reshape(np.asarray(w[k]).shape) if np.asarray(g[k]).size == np.asarray(w[k]).size else g[k], w[k]), "%s %s" % (what, k)
    assert [list(x) for x in got.strings()] == [list(x) for x in want.strings()], what
    assert np.array_equal(got.file_tint_off, want.file_tint_off), what
