"""Host side of the segmentation-visualisation script: the same interface as the reference's ``py/freddie_segment_vis.py``
(CLI flags, split TSV + segment TSV + annotation GTF in, one pickle out), with get_data() -- which segments every read and
annotated transcript flags, and how much of each it covers -- done by the gfx950 library behind ``include/freddie_vis.h``
for every object of every chromosome in one call.  There is no CPU implementation of that loop in this package.

Reference map (file:line of vpc-ccg/freddie ``py/freddie_segment_vis.py``):
  parse_args :8-34 / main :224-247          -> parse_args(), main()
  read_annotation_gtf :36-57                -> read_annotation_gtf()
  get_annotation_positions :59-92           -> get_annotation_positions()   (result unused by main; its assert can fire)
  get_segmentation_position :94-104         -> get_segmentation_position()
  switch_to_nearest :106-113                -> switch_to_nearest()
  get_seg_track :129-172                    -> get_seg_track()
  get_reads :174-197                        -> get_reads()
  get_data :199-222                         -> the library (fvis_classify); data_dicts() builds the dicts
The pickle holds the same objects as the reference's, shared the same way (a transcript's ``tid`` key and value are one
string; strings the readers cut out of a line are new objects, as there), so the bytes are the same.
"""
import argparse
import ctypes
import os
import pickle
import re
import sys

import numpy as np

from . import build as _build

VIS_SO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfreddie_vis.so")
VIS_SRC = [os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "freddie_vis.hip")]
VIS_HEADER = os.path.join(_build.INCLUDE, "freddie_vis.h")
EXPORTS = ["fvis_abi_version", "fvis_create", "fvis_destroy", "fvis_last_error", "fvis_source_hash", "fvis_classify", "fvis_results",
           "fvis_last_kernel_ms"]
FVIS_ERR_BOUNDS, FVIS_ERR_EMPTY = 3, 4
_lib = None
_I32 = (-2 ** 31, 2 ** 31 - 1)


class VisError(RuntimeError):
    pass


def command():
    return ["hipcc", "-O3", "--offload-arch=gfx950", "-shared", "-fPIC", "-I", _build.INCLUDE, "-o", VIS_SO] + VIS_SRC


def source_hash():
    """The hash a current libfreddie_vis.so carries (fvis_source_hash())."""
    return _build.source_hash(VIS_SRC + [VIS_HEADER], command())


def build(force=False, verbose=False):
    _build.build_stamped(VIS_SO, command(), VIS_SRC + [VIS_HEADER], force, verbose)
    return VIS_SO


def load():
    global _lib
    if _lib is not None:
        return _lib
    so = os.environ.get("FVIS_LIB") or VIS_SO          # (FVIS_LIB: a variant build, tools/ only)
    if not os.path.exists(so):
        raise VisError("%s not found: build it first (freddie_amd.segment_vis.build()); there is no CPU fallback" % so)
    L = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    L.fvis_abi_version.restype = ctypes.c_int
    L.fvis_create.restype = ctypes.c_int
    L.fvis_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.fvis_destroy.restype = None
    L.fvis_destroy.argtypes = [vp]
    L.fvis_last_error.restype = ctypes.c_char_p
    L.fvis_last_error.argtypes = [vp]
    L.fvis_source_hash.restype = ctypes.c_char_p
    L.fvis_source_hash.argtypes = []
    L.fvis_classify.restype = ctypes.c_int
    L.fvis_classify.argtypes = [vp, ctypes.c_int32, vp, vp, ctypes.c_int64, vp, vp, vp, ctypes.POINTER(ctypes.c_int64)]
    L.fvis_results.restype = ctypes.c_int
    L.fvis_results.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.fvis_last_kernel_ms.restype = ctypes.c_int
    L.fvis_last_kernel_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    _lib = L
    return L


def _ptr(a):
    return a.ctypes.data if a.size else None


def _int32(a, what):
    a = np.asarray(a, np.int64)
    if a.size and (a.min() < _I32[0] or a.max() > _I32[1]):
        raise VisError("%s: coordinates outside int32" % what)
    return np.ascontiguousarray(a, np.int32)


class EmptyObject(VisError):
    """An object whose intervals cover no position; ``index`` is its place in the call."""
    def __init__(self, index, msg):
        super().__init__(msg)
        self.index = index


class Context:
    def __init__(self, device=0):
        self._L = load()
        h = ctypes.c_void_p()
        if self._L.fvis_create(int(device), ctypes.byref(h)) != 0:
            raise VisError("fvis_create: " + self._L.fvis_last_error(None).decode())
        self._h = h
        self.kernel_ms = 0.0

    def classify(self, bounds, obj_chrom, iv_off, iv):
        """bounds: one ascending boundary list per chromosome; obj_chrom (n_obj), iv_off (n_obj + 1) and iv ((n, 2) of (s, e))
        describe the objects.  Returns (flag_off, seg, cls), copies of the library's results."""
        bound_off = np.zeros(len(bounds) + 1, np.int64)
        np.cumsum([len(b) for b in bounds], out=bound_off[1:])
        flat = _int32(np.concatenate([np.asarray(b, np.int64) for b in bounds]) if bounds else np.zeros(0, np.int64), "boundaries")
        oc = np.ascontiguousarray(obj_chrom, np.int32)
        io = np.ascontiguousarray(iv_off, np.int64)
        ivs = _int32(np.asarray(iv, np.int64).reshape(-1, 2), "intervals")
        bad = ctypes.c_int64(-1)
        rc = self._L.fvis_classify(self._h, len(bounds), bound_off.ctypes.data, _ptr(flat), len(oc), _ptr(oc), io.ctypes.data, _ptr(ivs),
                                   ctypes.byref(bad))
        if rc != 0:
            msg = "fvis_classify: " + self._L.fvis_last_error(self._h).decode()
            raise EmptyObject(bad.value, msg) if rc == FVIS_ERR_EMPTY else VisError(msg)
        v = ctypes.c_float()
        self._L.fvis_last_kernel_ms(self._h, ctypes.byref(v))
        self.kernel_ms = v.value
        fo, sg, cl = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._L.fvis_results(self._h, ctypes.byref(fo), ctypes.byref(sg), ctypes.byref(cl))
        flag_off = np.ctypeslib.as_array(ctypes.cast(fo, ctypes.POINTER(ctypes.c_int64)), (len(oc) + 1,)).copy()
        T = int(flag_off[-1])
        seg = np.ctypeslib.as_array(ctypes.cast(sg, ctypes.POINTER(ctypes.c_int32)), (T,)).copy() if T else np.zeros(0, np.int32)
        cls = np.ctypeslib.as_array(ctypes.cast(cl, ctypes.POINTER(ctypes.c_int8)), (T,)).copy() if T else np.zeros(0, np.int8)
        return flag_off, seg, cls

    def close(self):
        if getattr(self, "_h", None):
            self._L.fvis_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Outputs pickle file for vis purposes")
    ap.add_argument("-s", "--split-tsv", type=str, required=True, help="Freddie split TSV file")
    ap.add_argument("-g", "--segment-tsv", type=str, required=True, help="Freddie segment TSV file")
    ap.add_argument("-a", "--annotation-gtf", type=str, required=True, help="Annotation GTF file path")
    ap.add_argument("-o", "--output", type=str, default="vis_segmentation.pickle",
                    help="Output path. Default: vis_segmentation.pickle")
    ap.add_argument("--device", type=int, default=0, help="GPU ordinal")
    return ap.parse_args(argv)


_GID = re.compile(r'gene_id \"(?P<gid>ENSG\d{11})\"')
_TID = re.compile(r'transcript_id \"(?P<tid>ENST\d{11})\"')


def read_annotation_gtf(annotation_gtf):
    """{chrom: {tid: {'tid', 'gid', 'intervals'}}} of the exon lines (:36-57).  Only unversioned Ensembl ids match: another id
    raises AttributeError, as the reference's .group() on a failed search."""
    out = dict()
    with open(annotation_gtf) as f:
        for line in f:
            if line[0] == "#":
                continue
            cols = line.split("\t")
            if cols[2] != "exon":
                continue
            chrom = cols[0]
            transcripts = out.setdefault(chrom, dict())
            gid = _GID.search(cols[8]).group("gid")
            tid = _TID.search(cols[8]).group("tid")
            t = transcripts.get(tid)
            if t is None:
                t = transcripts[tid] = dict(tid=tid, gid=gid, intervals=list())
            t["intervals"].append((int(cols[3]), int(cols[4])))
    return out


def get_annotation_positions(cid_to_transcripts, w=5):
    """{chrom: positions}: exon ends closer than w merged into their count-weighted mean (:59-92).  main() does not use the
    result, but its closing assert is part of the script's behaviour."""
    out = dict()
    for chrom, transcripts in cid_to_transcripts.items():
        count = dict()
        for t in transcripts.values():
            for s, e in t["intervals"]:
                count[s] = count.get(s, 0) + 1
                count[e] = count.get(e, 0) + 1
        positions = sorted(count)
        groups, cur = [], []
        for a, b in zip(positions[:-1], positions[1:]):       # runs of neighbours closer than w
            if b - a < w:
                if not cur:
                    cur.append(a)
                cur.append(b)
            elif cur:
                groups.append(cur)
                cur = []
        if cur:
            groups.append(cur)
        final = set(count)
        for g in groups:
            final.difference_update(g)
            final.add(int(round(np.average(g, weights=[count[p] for p in g]))))
        final = sorted(final)
        for a, b in zip(final[:-1], final[1:]):
            assert b - a >= w
        out[chrom] = final
    return out


def get_segmentation_position(segment_tsv):
    """{chrom: set of boundaries} from the '#' header lines, of any number of tints and chromosomes (:94-104)."""
    out = dict()
    with open(segment_tsv) as f:
        for line in f:
            if line[0] != "#":
                continue
            cols = line[1:].rstrip().split("\t")
            out.setdefault(cols[0], set()).update(int(x) for x in cols[2].split(","))
    return out


def switch_to_nearest(cid_to_s_pos, cid_to_a_pos, w=5):
    """In place: each chromosome's sorted positions, those less than w + 1 below their successor dropped, then each moved to
    the nearest of cid_to_a_pos within w (:106-113).  main() passes the same dict twice: every position is its own nearest."""
    for chrom in cid_to_s_pos:
        pos = sorted(cid_to_s_pos[chrom])
        pos = [a for a, b in zip(pos[:-1], pos[1:]) if b - a > w] + [pos[-1]]
        cid_to_s_pos[chrom] = pos
        near = set(cid_to_a_pos[chrom])
        for i, p in enumerate(pos):
            hits = [(abs(x - p), x) for x in range(p - w, p + w + 1) if x in near]
            if hits:
                pos[i] = min(hits)[1]


def get_seg_track(cid_to_s_pos, cid_to_a_pos):
    """{chrom: {'segs': consecutive pairs of the sorted positions with 0 added, 'track': marks}} (:129-172).  A position's
    type is 1 (segmentation), 2 (annotation) or 3 (both; 0 is always 3); a mark is written only for a segment ending on an
    annotation-only position, so with the same dict passed twice the track is empty."""
    out = dict()
    for chrom in cid_to_s_pos:
        kind = {0: 3}
        for p in cid_to_s_pos[chrom] + cid_to_a_pos[chrom]:
            kind[p] = 0
        for p in cid_to_s_pos[chrom]:
            kind[p] |= 1
        for p in cid_to_a_pos[chrom]:
            kind[p] |= 2
        items = sorted(kind.items())
        entry = out[chrom] = dict(segs=list(), track=list())
        for (p1, t1), (p2, t2) in zip(items[:-1], items[1:]):
            entry["segs"].append((p1, p2))
            if t2 == 2:
                entry["track"].append("-" if t1 == 2 else "<")
            elif t1 == 2:
                entry["track"].append(">")
    return out


def get_reads(split_tsv):
    """{chrom: [read]} in file order (:174-197); a read's interval is the 's-e' before the first ':' of each field from the
    sixth on."""
    out = dict()
    with open(split_tsv) as f:
        for line in f:
            if line[0] == "#":
                continue
            cols = line.rstrip().split("\t")
            read = dict(rid=int(cols[0]), name=cols[1], tid=cols[1].split("_")[0], strand=cols[3], tint=cols[4], intervals=list())
            for field in cols[5:]:
                se = field.split(":")[0].split("-")
                read["intervals"].append((int(se[0]), int(se[1])))
            out.setdefault(cols[2], list()).append(read)
    return out


# ---------------------------------------------------------------------------------------------------------------
class Plan:
    """The objects main() classifies, in its order (per chromosome of the split TSV: its reads, then its transcripts), and
    where the reference stops with a KeyError: ``stop`` = (number of objects before it, chromosome, chromosome's kind)."""

    def __init__(self, cid_to_segs, cid_to_transcripts, cid_to_reads):
        self.chroms, self.groups, self.objects, self.stop = [], [], [], None
        self._spans = []                                     # (chromosome's index, objects) of the call, in order
        for chrom, reads in cid_to_reads.items():
            self.groups.append((chrom, "Read", reads))
            if chrom not in cid_to_segs:                     # get_data(..., segs=cid_to_segs[chrom]['segs']) of its first read
                self.stop = (len(self.objects), chrom, "Read")
                return
            self.chroms.append(chrom)
            self._add(reads)
            if chrom not in cid_to_transcripts:             # cid_to_transcripts[chrom].values() before its loop
                self.stop = (len(self.objects), chrom, None)
                return
            transcripts = list(cid_to_transcripts[chrom].values())
            self.groups.append((chrom, "Transcript", transcripts))
            self._add(transcripts)

    def _add(self, objs):
        self._spans.append((len(self.chroms) - 1, len(objs)))
        self.objects.extend(objs)

    def object_chroms(self):
        """The chromosome of every object, in order."""
        return [self.chroms[c] for c, n in self._spans for _ in range(n)]

    def arrays(self, cid_to_segs):
        """(boundary lists, obj_chrom, iv_off, iv) of the objects, for Context.classify()."""
        bounds = []
        for c in self.chroms:
            segs = cid_to_segs[c]["segs"]
            bounds.append([s for s, _ in segs] + [segs[-1][1]] if segs else [])
        obj_chrom = np.repeat(np.array([c for c, _ in self._spans], np.int32), [n for _, n in self._spans])
        iv_off = np.zeros(len(self.objects) + 1, np.int64)
        np.cumsum(np.fromiter((len(o["intervals"]) for o in self.objects), np.int64, len(self.objects)), out=iv_off[1:])
        try:
            iv = np.fromiter((x for o in self.objects for ab in o["intervals"] for x in ab), np.int64, int(iv_off[-1]) * 2)
        except OverflowError:
            raise VisError("intervals: coordinates outside int32") from None
        return bounds, obj_chrom, iv_off, iv.reshape(-1, 2)


def classify_plan(plan, cid_to_segs, ctx):
    """(flag_off, seg, cls) of the plan's objects, or the EmptyObject error of the first that covers no position."""
    if not plan.objects:
        return np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int8)
    return ctx.classify(*plan.arrays(cid_to_segs))


def data_dicts(flag_off, seg, cls):
    """get_data()'s dict {segment index: class} per object, ascending."""
    segs, classes, off = seg.tolist(), cls.tolist(), flag_off.tolist()
    return [dict(zip(segs[a:b], classes[a:b])) for a, b in zip(off[:-1], off[1:])]


def attach(plan, flag_off, seg, cls, failed=None, out=None):
    """main()'s loop (:232-243): the progress lines and each object's 'data', in the reference's order, up to the object the
    reference fails on (``failed``: its index, from the library) or the plan's KeyError; then that error."""
    out = out or sys.stdout
    datas = data_dicts(flag_off, seg, cls) if failed is None else None
    k = 0
    lines = []
    for chrom, kind, objs in plan.groups:
        for idx, obj in enumerate(objs):
            if idx % 500 == 0:
                lines.append("Chrom {}: {} {}/{}\n".format(chrom, kind, idx, len(objs)))
            if plan.stop is not None and plan.stop[0] == k and plan.stop[2] == kind:
                out.write("".join(lines))
                raise KeyError(chrom)
            if failed is not None and k == failed:
                out.write("".join(lines))
                min(set())                                   # the reference's ValueError, with its message
            if datas is not None:
                obj["data"] = datas[k]
            k += 1
    out.write("".join(lines))
    if plan.stop is not None:
        raise KeyError(plan.stop[1])


def compute(split_tsv, segment_tsv, annotation_gtf, device=0, ctx=None):
    """The library's results for main()'s objects without the dicts: dict(plan=Plan (its ``objects`` are the reads' and
    transcripts' dicts in classification order), flag_off, seg (ascending segment indices per object), cls (0 / 1 / 2),
    kernel_ms, and the readers' dicts).  Fails where main() fails, with the same exception class and nothing written: the
    readers' errors and the annotation assert, ValueError for the first object that covers no position, KeyError for a
    chromosome of the split TSV missing from the segment TSV or the GTF."""
    cid_to_transcripts = read_annotation_gtf(annotation_gtf)
    get_annotation_positions(cid_to_transcripts)
    cid_to_s_pos = get_segmentation_position(segment_tsv)
    switch_to_nearest(cid_to_s_pos, cid_to_s_pos)
    cid_to_segs = get_seg_track(cid_to_s_pos, cid_to_s_pos)
    cid_to_reads = get_reads(split_tsv)
    plan = Plan(cid_to_segs, cid_to_transcripts, cid_to_reads)
    own = ctx is None and bool(plan.objects)
    ctx = Context(device) if own else ctx
    try:
        try:
            flag_off, seg, cls = classify_plan(plan, cid_to_segs, ctx)
        except EmptyObject as e:                            # every object of the call comes before the plan's stop
            raise ValueError("object %d (main()'s order) covers no position" % e.index) from e
    finally:
        if own:
            ctx.close()
    if plan.stop is not None:
        raise KeyError(plan.stop[1])
    return dict(plan=plan, flag_off=flag_off, seg=seg, cls=cls, kernel_ms=ctx.kernel_ms if ctx is not None else 0.0,
                cid_to_segs=cid_to_segs, cid_to_transcripts=cid_to_transcripts, cid_to_reads=cid_to_reads)


def write_pickle(path, cid_to_segs, cid_to_transcripts, cid_to_reads):
    with open(path, "wb+") as f:
        pickle.dump((cid_to_segs, cid_to_transcripts, cid_to_reads), f)


def main(argv=None):
    args = parse_args(argv)
    cid_to_transcripts = read_annotation_gtf(args.annotation_gtf)
    get_annotation_positions(cid_to_transcripts)
    cid_to_s_pos = get_segmentation_position(args.segment_tsv)
    switch_to_nearest(cid_to_s_pos, cid_to_s_pos)
    cid_to_segs = get_seg_track(cid_to_s_pos, cid_to_s_pos)
    cid_to_reads = get_reads(args.split_tsv)
    plan = Plan(cid_to_segs, cid_to_transcripts, cid_to_reads)
    failed = None
    flag_off = seg = cls = None
    if plan.objects:
        ctx = Context(args.device)
        try:
            flag_off, seg, cls = classify_plan(plan, cid_to_segs, ctx)
        except EmptyObject as e:
            failed = e.index
        finally:
            ctx.close()
    else:
        flag_off, seg, cls = classify_plan(plan, cid_to_segs, None)
    attach(plan, flag_off, seg, cls, failed)
    write_pickle(args.output, cid_to_segs, cid_to_transcripts, cid_to_reads)


if __name__ == "__main__":
    main()
