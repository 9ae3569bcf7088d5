"""Helpers of the segmentation-visualisation tests: the fixtures the reference script wrote (tests/golden/vis/, minted by
tests/golden/make_vis_golden.py) and their inputs, crafted input cases, a literal statement of the script's main()
(py/freddie_segment_vis.py:224-247, get_data() :199-222 as its definition reads), the pickle as type-tagged JSON, and a
vectorised numpy statement of get_data() for whole batches."""
import glob
import gzip
import hashlib
import io
import json
import os
import pathlib
import pickle
import random

import numpy as np

VIS_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vis")
# segmentation goldens (tests/golden/<name>.npz) whose segment TSV, with its split TSV regenerated, is a fixture input
GOLDEN_SOURCES = ["g_tiny", "e_single_exon", "e_plateau_touch", "e_tau9999_len107", "b_sigma50", "g1_retention"]


def names(errors=None):
    """Fixture names; errors=True / False: only the cases on which the reference failed / succeeded."""
    out = sorted(os.path.basename(p)[:-8] for p in glob.glob(os.path.join(VIS_DIR, "*.json.gz")))
    return [n for n in out if errors is None or n.startswith("x_") == errors]


def load(name):
    with gzip.open(os.path.join(VIS_DIR, name + ".json.gz")) as f:
        return json.loads(f.read())


def gtf_around(chrom, bounds, rng, n_tx=12):
    """Transcripts on a segmentation's boundaries: exons starting and ending on, next to and between boundaries, minus-strand
    ones in descending order, one upstream of the first boundary, a duplicated id, a chromosome without reads."""
    out = ["#!genome-build test\n"]
    b = sorted(bounds)
    for t in range(n_tx):
        pos = b[rng.randrange(len(b))] + rng.choice([0, 0, 1, -1, 3])
        exons = []
        for _ in range(rng.randint(1, 5)):
            s = pos + rng.randint(0, 30)
            e = s + rng.randint(1, 200)
            if rng.random() < 0.4:
                e = max(s + 1, min(b, key=lambda x: abs(x - e)))
            exons.append((s, e))
            pos = e + rng.randint(5, 120)
        strand = "-" if t % 3 == 0 else "+"
        if strand == "-":
            exons = exons[::-1]
        gid, tid = ens("G", 100 + t // 2), ens("T", 1000 + t)
        out.append(gtf_line(chrom, min(x for x, _ in exons), max(y for _, y in exons), gid, tid, strand, kind="transcript"))
        out.extend(gtf_line(chrom, s, e, gid, tid, strand) for s, e in exons)
    out.append(gtf_line(chrom, max(1, b[0] - 40), max(2, b[0] - 10), ens("G", 9), ens("T", 9)))      # upstream of the first boundary
    out.append(gtf_line(chrom, b[-1] - 5, b[-1] + 50, ens("G", 100), ens("T", 1000)))              # a duplicate id: appended
    out.append(gtf_line("chrOther", 10, 20, ens("G", 1), ens("T", 1)))                              # a chromosome without reads
    return "".join(out)


def golden_case(name, d):
    """dict(split, segment, gtf) of the segmentation golden ``name``: its stored segment TSV, its split TSV regenerated under
    ``d`` (test_host_mirror.input_dir()), a GTF crafted around its boundaries (seeded by the name)."""
    import goldens
    from test_host_mirror import input_dir
    g = goldens.load(name)
    dd, contig, tid = input_dir(name, pathlib.Path(str(d)))
    split = open(os.path.join(dd, contig, "split_%s_%d.tsv" % (contig, tid))).read()
    seg = g["segment_tsv"].tobytes().decode()
    bounds = [int(x) for x in seg.split("\n")[0].split("\t")[2].split(",")]
    rng = random.Random(int(hashlib.sha256(name.encode()).hexdigest()[:8], 16))
    return dict(split=split, segment=seg, gtf=gtf_around(contig, bounds, rng))


def fixture_inputs(name, d):
    """The input texts of fixture ``name``: stored, or (s_* cases) rebuilt from the golden and checked against the split
    TSV the reference read."""
    doc = load(name)
    if "source" not in doc:
        return doc
    case = golden_case(doc["source"], d)
    assert hashlib.sha256(case["split"].encode()).hexdigest() == doc["split_sha256"], \
        "the generator no longer writes the split TSV the fixture was minted from"
    assert case["gtf"] == doc["gtf"]
    return case


def write_inputs(doc, d):
    paths = {k: os.path.join(str(d), k + ".txt") for k in ("split", "segment", "gtf")}
    for k, p in paths.items():
        with open(p, "w") as f:
            f.write(doc[k])
    return paths


def typed(x):
    """A pickled value as JSON that keeps tuple / list and int / str apart."""
    if isinstance(x, dict):
        return ["d", [[typed(k), typed(v)] for k, v in x.items()]]
    if isinstance(x, tuple):
        return ["t", [typed(v) for v in x]]
    if isinstance(x, list):
        return ["l", [typed(v) for v in x]]
    if isinstance(x, bool) or not isinstance(x, (int, str)):
        raise TypeError(type(x))
    return ["i" if isinstance(x, int) else "s", x]


def untyped(x):
    """The inverse of typed()."""
    tag, v = x
    if tag == "d":
        return {untyped(a): untyped(b) for a, b in v}
    if tag in ("t", "l"):
        items = [untyped(a) for a in v]
        return tuple(items) if tag == "t" else items
    return v


def recorded_data(doc):
    """The 'data' dicts of the reference's pickle in main()'s order (per chromosome of the split TSV: its reads, then its
    transcripts)."""
    _, transcripts, reads = untyped(doc["pickle"])
    out = []
    for chrom, rs in reads.items():
        out.extend(r["data"] for r in rs)
        out.extend(t["data"] for t in transcripts[chrom].values())
    return out


def literal_data(intervals, segs):
    """get_data() as its definition reads: the positions of the object, then per segment the flag test and the covered share."""
    locs = set()
    for s, e in intervals:
        locs.update(range(s, e))
    if not locs:
        raise ValueError("no position")                  # (min() of the empty set in the script)
    out = {}
    for j, (a, b) in enumerate(segs):
        if not any(a <= s <= b or s <= a <= e for s, e in intervals):
            continue
        c = len(locs.intersection(range(a, b))) / (b - a)
        out[j] = 1 if c > 0.9 else (0 if c < 0.1 else 2)
    return out


def restate(bounds, obj_chrom, iv_off, iv):
    """((flag_off, seg, cls), None) of a batch in the layout of fvis_classify(), with numpy over the whole batch: intervals
    sorted by (object, start); flagged ranges [searchsorted(B[1:], s), searchsorted(B[:-1], max(s, e), right) - 1] minus
    what an earlier interval of the object flagged; covered positions from the union of [s, e).  (None, index of the first
    object that covers no position) when there is one."""
    obj_chrom = np.asarray(obj_chrom, np.int64)
    iv_off = np.asarray(iv_off, np.int64)
    iv = np.asarray(iv, np.int64).reshape(-1, 2)
    n = len(obj_chrom)
    obj = np.repeat(np.arange(n, dtype=np.int64), np.diff(iv_off))
    order = np.lexsort((iv[:, 0], obj))
    obj, s, e = obj[order], iv[order, 0], iv[order, 1]
    ch = obj_chrom[obj]
    lo = np.zeros(len(s), np.int64)
    hi = np.full(len(s), -1, np.int64)
    for c, B in enumerate(bounds):
        B = np.asarray(B, np.int64)
        m = ch == c
        if len(B) < 2 or not m.any():
            continue
        lo[m] = np.searchsorted(B[1:], s[m], "left")
        hi[m] = np.searchsorted(B[:-1], np.maximum(s[m], e[m]), "right") - 1
    K = np.int64(1) << np.int64(34)                       # per-object offsets turn running maxima into segmented ones
    base = obj * K

    def excl_max(v, floor):
        run = np.maximum.accumulate(v + base)
        prev = np.concatenate([[np.iinfo(np.int64).min // 2], run[:-1]])
        return np.maximum(prev - base, floor)

    first = np.maximum(lo, excl_max(hi, -1) + 1)
    cnt = np.maximum(hi - first + 1, 0)
    ps = np.maximum(s, excl_max(e, np.int64(-2 ** 40)))
    ln = np.maximum(e - ps, 0)
    tot = np.zeros(n, np.int64)
    np.add.at(tot, obj, ln)
    empty = np.flatnonzero(tot == 0)
    if len(empty):
        return None, int(empty[0])
    csum = np.concatenate([[0], np.cumsum(ln)])
    cum = csum[:-1] - csum[iv_off[obj]]
    flag_off = np.zeros(n + 1, np.int64)
    per_obj = np.zeros(n, np.int64)
    np.add.at(per_obj, obj, cnt)
    np.cumsum(per_obj, out=flag_off[1:])
    q = np.repeat(np.arange(len(s)), cnt)
    start = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    j = first[q] + (np.arange(len(q)) - start[q])
    o = obj[q]
    bound_off = np.concatenate([[0], np.cumsum([len(b) for b in bounds])]).astype(np.int64)
    flat = np.concatenate([np.asarray(b, np.int64) for b in bounds]) if bounds else np.zeros(0, np.int64)
    b0 = flat[bound_off[obj_chrom[o]] + j]
    b1 = flat[bound_off[obj_chrom[o]] + j + 1]
    key = ps + base                                       # ascending: objects in order, piece starts non-decreasing

    def below(x):
        k = np.searchsorted(key, x + o * K, "right") - 1
        ok = (k >= 0) & (obj[np.maximum(k, 0)] == o)
        k = np.maximum(k, 0)
        return np.where(ok, cum[k] + np.clip(x - ps[k], 0, ln[k]), 0)

    cov = below(b1) - below(b0)
    nn = b1 - b0
    cls = np.where(10 * cov > 9 * nn, 1, np.where(10 * cov < nn, 0, 2)).astype(np.int8)
    return (flag_off, j.astype(np.int32), cls), None


def fuzz_batch(rng, n_obj, n_chrom=4):
    """Random boundaries (one chromosome spanning the whole int32 range) and objects with random, adversarial intervals:
    overlapping, unsorted, zero-length, reversed, on boundaries, outside the boundaries, a few objects with hundreds of
    intervals; every object covers at least one position."""
    bounds = []
    for c in range(n_chrom):
        if c == n_chrom - 1:
            B = np.unique(np.concatenate([[-2 ** 31, 2 ** 31 - 1, 0], rng.integers(-2 ** 31, 2 ** 31 - 1, 50)]))
        else:
            B = np.unique(rng.integers(0, 20000 * (c + 1), rng.integers(1, 3000)))
        bounds.append(B.astype(np.int64))
    obj_chrom = rng.integers(0, n_chrom, n_obj)
    n_iv = rng.integers(1, 9, n_obj)
    big = rng.random(n_obj) < 0.002
    n_iv[big] = rng.integers(64, 400, int(big.sum()))
    iv_off = np.concatenate([[0], np.cumsum(n_iv)]).astype(np.int64)
    Q = int(iv_off[-1])
    oc = np.repeat(obj_chrom, n_iv)
    hi_b = np.array([int(b[-1]) for b in bounds])[oc]
    lo_b = np.array([int(b[0]) for b in bounds])[oc]
    span = (hi_b - lo_b).astype(np.float64)
    s = (lo_b + rng.random(Q) * span * 1.02 - span * 0.01).astype(np.int64)
    on_b = rng.random(Q) < 0.3
    s[on_b] = [bounds[c][rng.integers(0, len(bounds[c]))] for c in oc[on_b]]
    length = np.where(rng.random(Q) < 0.1, -rng.integers(0, 50, Q), rng.integers(0, 2000, Q))
    length = np.where(rng.random(Q) < 0.05, (span * rng.random(Q)).astype(np.int64), length)
    iv = np.stack([np.clip(s, -2 ** 31, 2 ** 31 - 1), np.clip(s + length, -2 ** 31, 2 ** 31 - 1)], 1)
    f = iv_off[:-1]
    s0 = np.minimum(iv[f, 0], 2 ** 31 - 2)
    bad = iv[f, 0] >= iv[f, 1]
    iv[f[bad], 0] = s0[bad]
    iv[f[bad], 1] = s0[bad] + 1
    return [b.tolist() for b in bounds], obj_chrom, iv_off, iv


# ---------------------------------------------------------------------------------------------------------------
def gtf_line(chrom, s, e, gid, tid, strand="+", kind="exon"):
    return "\t".join([chrom, "test", kind, str(s), str(e), ".", strand, ".",
                      'gene_id "%s"; transcript_id "%s"; gene_name "G";' % (gid, tid)]) + "\n"


def ens(kind, n):
    return "ENS%s%011d" % (kind, n)


def read_line(rid, name, chrom, strand, tint, ivs):
    return "\t".join([str(rid), name, chrom, strand, tint] + ["%d-%d:0-10:10M" % (s, e) for s, e in ivs]) + "\n"


def cases():
    """{name: dict(split, segment, gtf)} (texts).  'x_' cases are the ones the script fails on."""
    out = {}
    # several tints and chromosomes in one segment file; a boundary at 0; positions 3 apart (the lower one dropped), exactly
    # 5 apart (dropped too: only a gap above 5 keeps it) and 6 apart (kept); single-character chromosome / strand / tint
    # strings (one shared object each in CPython: the pickle refers back to them)
    seg = ("#1\t1\t0,10,20,40,43,60,65,71,100\n"
           "0\ta\t1\t+\t1\t101\n"
           "#1\t12\t100,120,130\n"
           "#chr2\t3\t5,15,25,35,45\n")
    split = "".join([
        "# a comment line\n",
        read_line(0, "r0", "1", "+", "1", [(0, 10), (10, 19)]),                  # 10 of 10, then 9 of 10 = 0.9 exactly: class 2
        read_line(1, "r1_x", "1", "-", "1", [(40, 59), (12, 13)]),               # descending; 1 of 10 = 0.1 exactly: class 2
        read_line(2, "r2", "1", "+", "1", [(20, 40), (25, 30), (22, 45)]),       # overlapping
        read_line(3, "3_r", "1", "+", "12", [(50, 50), (60, 55), (101, 120)]),   # zero-length and reversed; ends on a boundary
        read_line(4, "r4", "1", "+", "1", [(10, 10), (30, 31)]),                 # a zero-length interval on a boundary
        read_line(5, "r5", "chr2", "+", "3", [(0, 3), (44, 46)]),                # upstream of the first boundary
        read_line(6, "r6", "chr2", "-", "3", [(15, 35)]),
        read_line(7, "r7", "chr2", "+", "3", [(7, 25), (200, 201)]),             # 18 of 20 = 0.9; past the last boundary
        read_line(8, "r8", "1", "+", "1", [(99, 100), (100, 101)]),
        read_line(9, "r9", "1", "+", "1", [(71, 76), (90, 130)]),
    ])
    gtf = "".join([
        "#!genome-build test\n",
        gtf_line("1", 20, 40, ens("G", 1), ens("T", 1)),
        gtf_line("1", 41, 60, ens("G", 1), ens("T", 1)),
        gtf_line("chr2", 30, 34, ens("G", 2), ens("T", 2), "-"),                 # minus strand: descending exons
        gtf_line("chr2", 5, 15, ens("G", 2), ens("T", 2), "-"),
        gtf_line("chr2", 10, 11, ens("G", 3), ens("T", 1)),                      # the same transcript id on another chromosome
        gtf_line("1", 90, 130, ens("G", 1), ens("T", 1)),                        # the duplicate id: appended to the first
        gtf_line("1", 1, 30, ens("G", 4), ens("T", 4), kind="CDS"),
        gtf_line("3", 1, 30, ens("G", 5), ens("T", 5)),                          # a chromosome without reads: no 'data'
    ])
    out["c_edges"] = dict(split=split, segment=seg, gtf=gtf)

    # more than 500 reads (several progress lines) on two chromosomes, random intervals in every shape
    rng = random.Random(11)
    bounds = sorted(set(rng.sample(range(1, 3000), 150)))
    seg = "#chrA\t0\t%s\n#chrB\t1\t%s\n" % (",".join(map(str, bounds)), ",".join(map(str, bounds[::3])))
    lines, gl = [], []
    for rid in range(1300):
        chrom = "chrA" if rid % 3 else "chrB"
        ivs = []
        for _ in range(rng.randint(1, 6)):
            s = rng.choice([rng.randrange(0, 3100), rng.choice(bounds)])
            e = max(0, s + rng.choice([rng.randint(1, 300), rng.randint(-20, 0), rng.choice(bounds) - s]))
            ivs.append((s, e))
        if all(s >= e for s, e in ivs):
            ivs.append((ivs[0][0], ivs[0][0] + 1))
        lines.append(read_line(rid, "rand_%d_%d" % (rid // 7, rid), chrom, "+-"[rid % 2], str(rid // 100), ivs))
    for t in range(700):
        chrom = "chrA" if t % 2 else "chrB"
        s = rng.randrange(1, 3000)
        for _ in range(rng.randint(1, 4)):
            gl.append(gtf_line(chrom, s, s + rng.randint(1, 100), ens("G", t // 3), ens("T", t)))
            s += rng.randint(101, 400)
    out["c_random"] = dict(split="".join(lines), segment=seg, gtf="".join(gl))

    base = out["c_edges"]
    out["x_versioned_id"] = dict(base, gtf=base["gtf"] + gtf_line("1", 5, 9, ens("G", 7) + ".3", ens("T", 7) + ".1"))
    out["x_chrom_not_in_gtf"] = dict(base, gtf="".join(l for l in base["gtf"].splitlines(True) if not l.startswith("chr2\t")))
    out["x_chrom_not_in_segments"] = dict(base, segment="".join(l for l in base["segment"].splitlines(True) if not l.startswith("#chr2")))
    out["x_read_without_position"] = dict(base, split=base["split"] + read_line(10, "r10", "1", "+", "1", [(30, 30), (50, 40)]) +
                                          read_line(11, "r11", "1", "+", "1", [(1, 2)]))
    out["x_read_without_interval"] = dict(base, split=base["split"] + "12\tr12\t1\t+\t1\n")
    out["x_transcript_without_position"] = dict(base, gtf=base["gtf"] + gtf_line("1", 70, 70, ens("G", 8), ens("T", 8)))
    P = 2 ** 60                        # float64 rounds the weighted mean of P+130, P+134 to P+256: 2 below P+254
    out["x_annotation_assert"] = dict(base, gtf=base["gtf"] + gtf_line("chr9", P + 130, P + 134, ens("G", 9), ens("T", 90)) +
                                      gtf_line("chr9", P + 254, P + 400, ens("G", 9), ens("T", 91)))
    return out


def literal_main(paths, sv):
    """The script's main() with get_data() as literal_data(): (stdout, exception class name or None, pickle bytes or None).
    ``sv``: the module whose readers to use (freddie_amd.segment_vis)."""
    out = io.StringIO()
    try:
        transcripts = sv.read_annotation_gtf(paths["gtf"])
        sv.get_annotation_positions(transcripts)
        s_pos = sv.get_segmentation_position(paths["segment"])
        sv.switch_to_nearest(s_pos, s_pos)
        segs = sv.get_seg_track(s_pos, s_pos)
        reads = sv.get_reads(paths["split"])
        for chrom, rs in reads.items():
            for idx, r in enumerate(rs):
                if idx % 500 == 0:
                    out.write("Chrom {}: Read {}/{}\n".format(chrom, idx, len(rs)))
                r["data"] = literal_data(r["intervals"], segs[chrom]["segs"])
            for idx, t in enumerate(transcripts[chrom].values()):
                if idx % 500 == 0:
                    out.write("Chrom {}: Transcript {}/{}\n".format(chrom, idx, len(transcripts[chrom])))
                t["data"] = literal_data(t["intervals"], segs[chrom]["segs"])
        return out.getvalue(), None, pickle.dumps((segs, transcripts, reads))
    except Exception as e:                                      # noqa: BLE001 -- the script's exception is the result
        return out.getvalue(), type(e).__name__, None
