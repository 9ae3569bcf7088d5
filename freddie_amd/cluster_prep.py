"""Pre-ILP work of the clustering stage: the host-side mirror of the reference's
``py/freddie_cluster.py`` up to (not including) the ILP, with the two quadratic loops of ``partition_reads`` done by
the gfx950 library behind ``include/freddie_cluster.h``.

Reference map (file:line of vpc-ccg/freddie ``py/freddie_cluster.py``):
  read_segment :119-172        -> read_segment()          segment_*.tsv -> tint dicts (reads, read_reps by structure key)
  find_segment_read :175-183   -> find_segment_read()
  preprocess_ilp :277-328      -> preprocess_ilp()        I / C / FL / garbage_cost, poly-tail categories
  split_list_evenly :112-116   -> split_list_evenly()
  partition_reads :196-274     -> partition_reads(), partition_reads_batch()
       unique structures :203-215 (host); pairwise compatibility :217-234, edge pruning :240-255, connected components
       :256-257, even split and incompatible pairs :258-274 (GPU: Context.partition, flat arrays)
  preprocess_ilp + partition_reads on tints that are not preprocessed yet -> pack_labels(), preprocess_ilp_batch(),
       cluster_arrays_batch(): I / C / FL, the dedupe and everything behind it in one device call (Context.partition_labels)
  segment_*.tsv files -> arrays without a Python loop over reads: read_segment_arrays() (the native reader of libfreddie_host.so),
       Context.group_reads() / Context.partition_segment() (read_reps :154-164 on the GPU, then all of the above),
       cluster_files_batch(), tints_from_arrays() (back to the dicts, for code that wants them)
  informative_segs :331-344 and the model run_ilp builds :397-535 -> Context.round_setup() / Context.round_models() (GPU: one call per
       round of many partitions), round_gaps(), round_model(); the solve is freddie_amd/cluster_solve.py, the loop freddie_amd/cluster.py
  run_ilp's read-out :601-635 -> Context.round_readout() (GPU: the isoforms of a round's accepted column sets, behind round_models() in
       either form; fetch=False leaves the models on the device), readout_isoform(), and readout_mirror() / readout_words(), the numpy
       restatement of the kernels' word arithmetic (tests, tools/readout_host_check.py)
There is no CPU implementation of the quadratic
loops in this package: without the HIP library partition_reads() raises.  FCLU_HOST_PARTITIONS=1 keeps :256-274 on the
host, behind the GPU's graph (adjacency_matrix + _components + _partitions_from_graph): for A/B runs and timings.
"""
import ctypes
import os
import re
from math import ceil

import numpy as np

from . import build as _build
from . import cluster_solve

# ---------------------------------------------------------------------------------------------------------------
# segment_*.tsv -> tint dict   (read_segment :119-172)
# ---------------------------------------------------------------------------------------------------------------
_CHR = r"[0-9A-Za-z!#$%&+./:;?@^_|~-][0-9A-Za-z!#$%&*+./:;=?@^_|~-]*"
_HEADER = re.compile(r"#(" + _CHR + r")\t([0-9]+)\t([0-9]+(?:,[0-9]+)*)\n$")
_INTERNAL = r"(\d+)-(\d+):(\d+),"
_SOFTCLIP = r"([ES]SC):(\d+),"
_POLY = r"([ES][AT])_(\d+):(\d+),"
_READ = re.compile(r"([0-9]+)\t([!-?A-~]{1,254})\t(" + _CHR + r")\t([+-])\t([0-9]+)\t([012]+)\t((?:" + _INTERNAL + "|" +
                   _SOFTCLIP + "|" + _POLY + r")*)\n$")
_INTERNAL_RE, _SOFTCLIP_RE, _POLY_RE = re.compile(_INTERNAL), re.compile(_SOFTCLIP), re.compile(_POLY)


def read_segment(segment_tsv):
    """{tint id: tint}; tint = id, chr, segs [(start, end, length)], reads [...], read_reps [[read index, ...], ...]
    where reads with the same structure key (labels with 2 -> 0, large internal gaps, large poly tails) share a rep."""
    tints = dict()
    keys = dict()
    for line in open(segment_tsv):
        if line[0] == "#":
            m = _HEADER.match(line)
            pos = [int(x) for x in m.group(3).split(",")]
            assert all(a < b for a, b in zip(pos[:-1], pos[1:])), pos
            tid = int(m.group(2))
            assert tid not in tints, "Transcriptional interval with id {} is repeated!".format(tid)
            tints[tid] = dict(id=tid, chr=m.group(1), segs=[(s, e, e - s) for s, e in zip(pos[:-1], pos[1:])],
                              read_reps=list(), reads=list())
            keys[tid] = dict()
            continue
        m = _READ.match(line)
        rid, name, chrom, strand, cid, data, gaps = m.group(1, 2, 3, 4, 5, 6, 7)
        internal = _INTERNAL_RE.findall(gaps)
        poly = _POLY_RE.findall(gaps)
        read = dict(id=int(rid), name=name, chr=chrom, strand=strand, tint=int(cid), data=[int(d) for d in data],
                    gaps={(int(a), int(b)): int(c) for a, b, c in internal},
                    softclip={k: int(v) for k, v in _SOFTCLIP_RE.findall(gaps)},
                    poly_tail={k: (int(a), int(b)) for k, a, b in poly})
        key = data.replace("2", "0")
        key += "".join(".{}".format(c if int(c) > 10 else 0) for _, _, c in internal)
        key += "".join(".{}{}".format(k[0], b if int(b) > 10 else 0) for k, _, b in poly)
        tint = tints[read["tint"]]
        tint["reads"].append(read)
        reps = keys[read["tint"]]
        if key not in reps:
            reps[key] = len(tint["read_reps"])
            tint["read_reps"].append(list())
        tint["read_reps"][reps[key]].append(len(tint["reads"]) - 1)
        assert len(read["data"]) == len(tint["segs"]), (read["data"], tint["segs"])
        assert read["chr"] == tint["chr"]
        assert all(0 <= a < b < len(read["data"]) for a, b in read["gaps"].keys())
    return tints


def find_segment_read(M, i):
    """(first, last) segment of row i holding a 1; (-1, len - 1) when there is none (:175-183)."""
    row = M[i]
    first, last = -1, len(row) - 1
    for j, v in enumerate(row):
        if v == 1:
            if first == -1:
                first = j
            last = j
    return (first, last)


def garbage_cost_introns(C):
    return max(sum(C.values()) - 0.5, 1)


def garbage_cost_exons(I):
    return max(sum(I.values()) - 0.5, 1)


def preprocess_ilp(tint, ilp_settings):
    """tint['ilp_data'] = I (label % 2), C (0-labels strictly inside the read's span), FL (first, last), garbage_cost;
    sets poly_tail_category on every read and the tail pseudo-gaps (-1, first) / (last, M) on the reps (:277-328)."""
    read_reps = tint["read_reps"]
    M = len(tint["segs"])
    I, C, FL = dict(), dict(), dict()
    for i, members in enumerate(read_reps):
        read = tint["reads"][members[0]]
        I[i] = [v % 2 for v in read["data"][:M]]
        C[i] = [0] * M
        lo, hi = find_segment_read(I, i)
        read["poly_tail_category"] = "N"
        if len(read["poly_tail"]) == 1:
            key = next(iter(read["poly_tail"]))
            length, gap = read["poly_tail"][key]
            if key in ("SA", "ST") and length > 10:
                read["poly_tail_category"] = "S"
                read["gaps"][(-1, lo)] = gap
                lo = 0
            elif key in ("EA", "ET") and length > 10:
                read["poly_tail_category"] = "E"
                read["gaps"][(hi, M)] = gap
                hi = M - 1
        FL[i] = (lo, hi)
        for j in range(M):
            C[i][j] = 1 if (lo <= j <= hi and read["data"][j] == 0) else 0
        for ridx in members:
            tint["reads"][ridx]["poly_tail_category"] = read["poly_tail_category"]
            tint["reads"][ridx]["gaps"] = read["gaps"]
    garbage_cost = {}
    for i in range(len(read_reps)):
        if ilp_settings["recycle_model"] == "exons":
            garbage_cost[i] = len(read_reps[i]) * garbage_cost_exons(I=I[i])      # a list: raises like the reference (:314)
        elif ilp_settings["recycle_model"] == "introns":
            garbage_cost[i] = len(read_reps[i]) * garbage_cost_introns(C=C[i])  # a list: raises like the reference (:316)
        elif ilp_settings["recycle_model"] == "constant":
            garbage_cost[i] = len(read_reps[i]) * 3
    tint["ilp_data"] = dict(FL=FL, I=I, C=C, garbage_cost=garbage_cost)


def split_list_evenly(l, m):
    p = ceil(len(l) / m)
    s = ceil(len(l) / p)
    for idx in range(0, p * s, s):
        yield l[idx:idx + s]


# ---------------------------------------------------------------------------------------------------------------
# the C-ABI (include/freddie_cluster.h)
# ---------------------------------------------------------------------------------------------------------------
CLUSTER_SO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfreddie_cluster.so")
CLUSTER_SRC = [os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "freddie_cluster.hip")]
CLUSTER_HEADERS = [os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", n) for n in ("clu_incumbent.h", "clu_exact.h", "clu_bnb.h", "clu_bnb_wide.h", "clu_readout.h", "clu_plan.h")]
EXPORTS = ["fclu_abi_version", "fclu_create", "fclu_destroy", "fclu_last_error", "fclu_compat_graph", "fclu_last_timing",
           "fclu_last_paths",
           "fclu_partition", "fclu_partition_adj", "fclu_partition_results", "fclu_partition_timing",
           "fclu_preprocess", "fclu_preprocess_results", "fclu_partition_reads", "fclu_preprocess_timing",
           "fclu_group_reads", "fclu_partition_segment", "fclu_group_results", "fclu_group_timing",
           "fclu_round_setup", "fclu_round_models", "fclu_round_results", "fclu_round_timing",
           "fclu_round_incumbents", "fclu_round_incumbent_results", "fclu_round_incumbent_timing",
           "fclu_round_exact", "fclu_round_exact_results", "fclu_round_exact_timing",
           "fclu_round_bnb", "fclu_round_bnb_results", "fclu_round_bnb_timing",
           "fclu_round_bnb_wide", "fclu_round_bnb_wide_results", "fclu_round_bnb_wide_timing",
           "fclu_round_bnb_wide_passes", "fclu_round_bnb_wide_pass_stats",
           "fclu_round_models_resident", "fclu_round_readout", "fclu_round_readout_results", "fclu_round_readout_timing"]
ERR_UNSUPPORTED = 3
_lib = None


class ClusterError(RuntimeError):
    """code: the library's return value (FCLU_ERR_*), or None when the error is this module's own."""

    def __init__(self, message, code=None):
        RuntimeError.__init__(self, message)
        self.code = code


class _Batch(ctypes.Structure):
    _fields_ = [("n_tint", ctypes.c_int32), ("row_off", ctypes.c_void_p), ("n_seg", ctypes.c_void_p),
                ("bits_off", ctypes.c_void_p), ("bits", ctypes.c_void_p), ("first", ctypes.c_void_p),
                ("last", ctypes.c_void_p), ("tail", ctypes.c_void_p), ("adj_off", ctypes.c_void_p)]


class _Parts(ctypes.Structure):
    _fields_ = [("n_tint", ctypes.c_int32), ("n_rows", ctypes.c_int64), ("n_part", ctypes.c_int64), ("n_rids", ctypes.c_int64),
                ("n_pairs", ctypes.c_int64), ("tint_part_off", ctypes.c_void_p), ("part_node_off", ctypes.c_void_p),
                ("part_nodes", ctypes.c_void_p), ("part_rid_off", ctypes.c_void_p), ("part_rids", ctypes.c_void_p),
                ("part_pair_off", ctypes.c_void_p), ("pairs", ctypes.c_void_p), ("label", ctypes.c_void_p)]


class _Reads(ctypes.Structure):
    _fields_ = [("n_tint", ctypes.c_int32), ("rep_off", ctypes.c_void_p), ("n_seg", ctypes.c_void_p), ("lab_off", ctypes.c_void_p),
                ("labels", ctypes.c_void_p), ("tail", ctypes.c_void_p)]


class _Prep(ctypes.Structure):
    _fields_ = [("n_tint", ctypes.c_int32), ("n_reps", ctypes.c_int64), ("n_rows", ctypes.c_int64)] + [
        (name, ctypes.c_void_p) for name in ("row_off", "bits_off", "adj_off", "rep_bits_off", "i_bits", "c_bits", "first", "last",
                                             "raw_first", "raw_last", "rep_node", "node_rep", "mem_off", "mem", "bits",
                                             "node_first", "node_last", "node_tail")]


class _Segment(ctypes.Structure):
    _fields_ = [("n_tint", ctypes.c_int32), ("read_off", ctypes.c_void_p), ("n_seg", ctypes.c_void_p), ("lab_off", ctypes.c_void_p),
                ("labels", ctypes.c_void_p), ("tok_off", ctypes.c_void_p), ("tok", ctypes.c_void_p), ("tail", ctypes.c_void_p)]


class _Groups(ctypes.Structure):
    _fields_ = [("n_tint", ctypes.c_int32), ("n_reads", ctypes.c_int64), ("n_reps", ctypes.c_int64)] + [
        (name, ctypes.c_void_p) for name in ("rep_off", "read_rep", "rep_mem_off", "rep_mem", "rep_first")]


class _RoundBatch(ctypes.Structure):
    _fields_ = [("n_prob", ctypes.c_int32), ("part", ctypes.c_void_p), ("rid_off", ctypes.c_void_p), ("rids", ctypes.c_void_p)]


_ROUND_COUNTS = ("n_cols", "n_inf", "n_sup", "n_corr", "n_pairs", "n_grp", "n_grp_seg", "n_gap_rows")
_ROUND_ARRAYS = ("refused", "inf_bits_off", "inf_bits", "inf_off", "inf_seg", "sup_off", "sup_cols", "col_off", "corr_off", "corr_seg", "pair_off",
                 "pairs", "grp_off", "grp", "grp_seg_off", "grp_seg", "grp_len", "row_off", "rows")


class _Rounds(ctypes.Structure):
    _fields_ = [("n_prob", ctypes.c_int32)] + [(n, ctypes.c_int64) for n in _ROUND_COUNTS] + [(n, ctypes.c_void_p) for n in _ROUND_ARRAYS]


_PATHS = ("compat_form", "tiles", "lds_tints", "pass_kernel", "edge_chunks", "passes_enqueued", "passes_ran")     # FCLU_PATH_*


class _Incumbents(ctypes.Structure):
    _fields_ = [("n_prob", ctypes.c_int32), ("n_mem", ctypes.c_int64)] + [
        (n, ctypes.c_void_p) for n in ("cost2", "start", "grow_steps", "repair_steps", "mem_off", "mem")]


class _Exact(ctypes.Structure):
    _fields_ = [("n_prob", ctypes.c_int32), ("cost2", ctypes.c_void_p), ("mask", ctypes.c_void_p), ("n_taken", ctypes.c_int64),
                ("n_masks", ctypes.c_int64), ("n_launches", ctypes.c_int64)]


class _Bnb(ctypes.Structure):
    _fields_ = [("n_prob", ctypes.c_int32)] + [(n, ctypes.c_void_p) for n in ("status", "cost2", "mask", "nodes", "capped")] + [
        (n, ctypes.c_int64) for n in ("n_taken", "n_launches", "nodes_total")]


class _Readout(ctypes.Structure):
    _fields_ = [("n_prob", ctypes.c_int32)] + [(n, ctypes.c_int64) for n in ("n_sets", "n_mem", "n_exon_bytes", "n_corr_bytes", "n_e")] + [
        (n, ctypes.c_void_p) for n in ("exon_off", "exons", "mem_off", "corr_off", "corr", "e_off", "e")]


_READOUT_PATHS = ("sets", "members", "stores")     # FCLU_PATH_READOUT_*, behind the graph's words
STORE_WIDE, STORE_BYTES = 1, 2                     # FCLU_STORE_*


BNB_STATUS = {0: "optimal", 1: "infeasible", 2: "unproven", -2: None}     # FCLU_BNB_*


def build(force=False, verbose=False):
    """hipcc -> libfreddie_cluster.so (in-tree; cross-compiles without a GPU)."""
    cmd = ["hipcc", "-O3", "--offload-arch=gfx950", "-shared", "-fPIC", "-I", _build.INCLUDE, "-o", CLUSTER_SO] + CLUSTER_SRC
    _build.build_stamped(CLUSTER_SO, cmd, CLUSTER_SRC + CLUSTER_HEADERS + [os.path.join(_build.INCLUDE, "freddie_cluster.h")], force, verbose)
    return CLUSTER_SO


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(CLUSTER_SO):
        raise ClusterError("%s not found: build it first (freddie_amd.cluster_prep.build()); there is no CPU fallback" % CLUSTER_SO)
    L = ctypes.CDLL(CLUSTER_SO)
    vp = ctypes.c_void_p
    L.fclu_abi_version.restype = ctypes.c_int
    L.fclu_create.restype = ctypes.c_int
    L.fclu_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.fclu_destroy.restype = None
    L.fclu_destroy.argtypes = [vp]
    L.fclu_last_error.restype = ctypes.c_char_p
    L.fclu_last_error.argtypes = [vp]
    L.fclu_compat_graph.restype = ctypes.c_int
    L.fclu_compat_graph.argtypes = [vp, ctypes.POINTER(_Batch), ctypes.c_int32, vp, vp]
    L.fclu_last_timing.restype = ctypes.c_int
    L.fclu_last_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    L.fclu_last_paths.restype = ctypes.c_int
    L.fclu_last_paths.argtypes = [vp, vp, ctypes.c_int32]
    L.fclu_partition.restype = ctypes.c_int
    L.fclu_partition.argtypes = [vp, ctypes.POINTER(_Batch), vp, vp, ctypes.c_int32]
    L.fclu_partition_adj.restype = ctypes.c_int
    L.fclu_partition_adj.argtypes = [vp, ctypes.c_int32, vp, vp, vp, vp, vp, ctypes.c_int32]
    L.fclu_partition_results.restype = ctypes.c_int
    L.fclu_partition_results.argtypes = [vp, ctypes.POINTER(_Parts)]
    L.fclu_partition_timing.restype = ctypes.c_int
    L.fclu_partition_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    L.fclu_preprocess.restype = ctypes.c_int
    L.fclu_preprocess.argtypes = [vp, ctypes.POINTER(_Reads)]
    L.fclu_preprocess_results.restype = ctypes.c_int
    L.fclu_preprocess_results.argtypes = [vp, ctypes.POINTER(_Prep)]
    L.fclu_partition_reads.restype = ctypes.c_int
    L.fclu_partition_reads.argtypes = [vp, ctypes.POINTER(_Reads), ctypes.c_int32]
    L.fclu_preprocess_timing.restype = ctypes.c_int
    L.fclu_preprocess_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    L.fclu_group_reads.restype = ctypes.c_int
    L.fclu_group_reads.argtypes = [vp, ctypes.POINTER(_Segment)]
    L.fclu_partition_segment.restype = ctypes.c_int
    L.fclu_partition_segment.argtypes = [vp, ctypes.POINTER(_Segment), ctypes.c_int32]
    L.fclu_group_results.restype = ctypes.c_int
    L.fclu_group_results.argtypes = [vp, ctypes.POINTER(_Groups)]
    L.fclu_group_timing.restype = ctypes.c_int
    L.fclu_group_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    L.fclu_round_setup.restype = ctypes.c_int
    L.fclu_round_setup.argtypes = [vp, vp, vp, vp, vp]
    L.fclu_round_models.restype = ctypes.c_int
    L.fclu_round_models.argtypes = [vp, ctypes.POINTER(_RoundBatch)]
    L.fclu_round_results.restype = ctypes.c_int
    L.fclu_round_results.argtypes = [vp, ctypes.POINTER(_Rounds)]
    L.fclu_round_timing.restype = ctypes.c_int
    L.fclu_round_timing.argtypes = [vp] + [ctypes.POINTER(ctypes.c_float)] * 3
    L.fclu_round_incumbents.restype = ctypes.c_int
    L.fclu_round_incumbents.argtypes = [vp, vp, ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.c_int32]
    L.fclu_round_incumbent_results.restype = ctypes.c_int
    L.fclu_round_incumbent_results.argtypes = [vp, ctypes.POINTER(_Incumbents)]
    L.fclu_round_incumbent_timing.restype = ctypes.c_int
    L.fclu_round_incumbent_timing.argtypes = [vp] + [ctypes.POINTER(ctypes.c_float)] * 3
    L.fclu_round_exact.restype = ctypes.c_int
    L.fclu_round_exact.argtypes = [vp, vp, ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64]
    L.fclu_round_exact_results.restype = ctypes.c_int
    L.fclu_round_exact_results.argtypes = [vp, ctypes.POINTER(_Exact)]
    L.fclu_round_exact_timing.restype = ctypes.c_int
    L.fclu_round_exact_timing.argtypes = [vp] + [ctypes.POINTER(ctypes.c_float)] * 3
    L.fclu_round_bnb.restype = ctypes.c_int
    L.fclu_round_bnb.argtypes = [vp, vp, vp, ctypes.c_double, ctypes.c_double] + [ctypes.c_int32] * 5 + [ctypes.c_int64]
    L.fclu_round_bnb_results.restype = ctypes.c_int
    L.fclu_round_bnb_results.argtypes = [vp, ctypes.POINTER(_Bnb)]
    L.fclu_round_bnb_timing.restype = ctypes.c_int
    L.fclu_round_bnb_timing.argtypes = [vp] + [ctypes.POINTER(ctypes.c_float)] * 3
    L.fclu_round_bnb_wide.restype = ctypes.c_int
    L.fclu_round_bnb_wide.argtypes = [vp, vp, vp, ctypes.c_double, ctypes.c_double] + [ctypes.c_int32] * 5 + [ctypes.c_int64]
    L.fclu_round_bnb_wide_results.restype = ctypes.c_int
    L.fclu_round_bnb_wide_results.argtypes = [vp, ctypes.POINTER(_Bnb)]
    L.fclu_round_bnb_wide_passes.restype = ctypes.c_int
    L.fclu_round_bnb_wide_passes.argtypes = [vp, vp, vp, ctypes.c_double, ctypes.c_double] + [ctypes.c_int32] * 5 + [ctypes.c_int64, ctypes.c_int32]
    L.fclu_round_bnb_wide_pass_stats.restype = ctypes.c_int
    L.fclu_round_bnb_wide_pass_stats.argtypes = [vp, vp, ctypes.c_int32]
    L.fclu_round_bnb_wide_timing.restype = ctypes.c_int
    L.fclu_round_bnb_wide_timing.argtypes = [vp] + [ctypes.POINTER(ctypes.c_float)] * 3
    L.fclu_round_models_resident.restype = ctypes.c_int
    L.fclu_round_models_resident.argtypes = [vp, ctypes.POINTER(_RoundBatch)]
    L.fclu_round_readout.restype = ctypes.c_int
    L.fclu_round_readout.argtypes = [vp, vp, vp]
    L.fclu_round_readout_results.restype = ctypes.c_int
    L.fclu_round_readout_results.argtypes = [vp, ctypes.POINTER(_Readout)]
    L.fclu_round_readout_timing.restype = ctypes.c_int
    L.fclu_round_readout_timing.argtypes = [vp] + [ctypes.POINTER(ctypes.c_float)] * 2
    _lib = L
    return L


def _copy_out(ptr, n, dtype):
    """numpy copy of n items behind a pointer of the library (its buffers live only until the context's next call)."""
    dtype = np.dtype(dtype)
    if n == 0:
        return np.zeros(0, dtype)
    return np.frombuffer((ctypes.c_char * (n * dtype.itemsize)).from_address(ptr), dtype, n).copy()


class Context:
    """One GPU context of the clustering pre-ILP library."""

    def __init__(self, device=0):
        self._L = load()
        h = ctypes.c_void_p()
        rc = self._L.fclu_create(int(device), ctypes.byref(h))
        if rc != 0:
            raise ClusterError("fclu_create: " + self._L.fclu_last_error(None).decode())
        self._h = h

    @staticmethod
    def _batch(packed):
        b = _Batch(n_tint=packed["n_tint"])
        keep = []
        for name, dt in (("row_off", np.int64), ("n_seg", np.int32), ("bits_off", np.int64), ("bits", np.uint32),
                         ("first", np.int32), ("last", np.int32), ("tail", np.uint8), ("adj_off", np.int64)):
            a = np.ascontiguousarray(packed[name], dt)
            keep.append(a)
            setattr(b, name, a.ctypes.data if a.size else None)
        return b, keep

    def compat_graph(self, packed, prune=True):
        """packed: pack_structures() of a batch.  Returns (adj uint64[adj_off[-1]], rounds int32[n_tint])."""
        b, keep = self._batch(packed)
        adj = np.zeros(max(int(packed["adj_off"][-1]), 1), np.uint64)
        rounds = np.zeros(packed["n_tint"], np.int32)
        rc = self._L.fclu_compat_graph(self._h, ctypes.byref(b), 1 if prune else 0, adj.ctypes.data, rounds.ctypes.data)
        if rc != 0:
            raise ClusterError("fclu_compat_graph: " + self._L.fclu_last_error(self._h).decode(), rc)
        return adj[:int(packed["adj_off"][-1])], rounds

    def _partition_arrays(self, what, rc):
        if rc != 0:
            raise ClusterError(what + ": " + self._L.fclu_last_error(self._h).decode(), rc)
        p = _Parts()
        rc = self._L.fclu_partition_results(self._h, ctypes.byref(p))
        if rc != 0:
            raise ClusterError("fclu_partition_results: " + self._L.fclu_last_error(self._h).decode(), rc)
        P = int(p.n_part)
        return dict(tint_part_off=_copy_out(p.tint_part_off, p.n_tint + 1, np.int64),
                    part_node_off=_copy_out(p.part_node_off, P + 1, np.int64), part_nodes=_copy_out(p.part_nodes, int(p.n_rows), np.int32),
                    part_rid_off=_copy_out(p.part_rid_off, P + 1, np.int64), part_rids=_copy_out(p.part_rids, int(p.n_rids), np.int32),
                    part_pair_off=_copy_out(p.part_pair_off, P + 1, np.int64),
                    pairs=_copy_out(p.pairs, 2 * int(p.n_pairs), np.int32).reshape(-1, 2), label=_copy_out(p.label, int(p.n_rows), np.int32))

    @staticmethod
    def _members(members):
        mem_off = np.ascontiguousarray(members["mem_off"], np.int64)
        mem = np.ascontiguousarray(members["mem"], np.int32)
        return mem_off, mem

    def partition(self, packed, members, maximum_ilp_size):
        """partition_reads() behind the dedupe for a batch, on the device: packed = pack_structures(), members = pack_members().
        Returns numpy arrays (include/freddie_cluster.h, fclu_parts): tint_part_off [T+1]; per partition part_node_off /
        part_rid_off / part_pair_off [P+1] into part_nodes (node indices local to the tint), part_rids and pairs (int32 [n, 2]);
        label (the smallest node of each unique read's component)."""
        b, keep = self._batch(packed)
        mem_off, mem = self._members(members)
        if mem_off.size != int(packed["row_off"][-1]) + 1:
            raise ClusterError("partition: mem_off has %d entries for %d rows" % (mem_off.size, int(packed["row_off"][-1])))
        rc = self._L.fclu_partition(self._h, ctypes.byref(b), mem_off.ctypes.data, mem.ctypes.data if mem.size else None,
                                    int(maximum_ilp_size))
        return self._partition_arrays("fclu_partition", rc)

    def partition_adj(self, row_off, adj_off, adj, members, maximum_ilp_size):
        """The same behind a graph of the caller's: adj in the layout compat_graph() returns (symmetric, empty diagonal)."""
        row_off = np.ascontiguousarray(row_off, np.int64)
        adj_off = np.ascontiguousarray(adj_off, np.int64)
        adj = np.ascontiguousarray(adj, np.uint64)
        mem_off, mem = self._members(members)
        if row_off.size < 2 or adj_off.size != row_off.size or adj.size != int(adj_off[-1]) or mem_off.size != int(row_off[-1]) + 1:
            raise ClusterError("partition_adj: array lengths do not match (row_off, adj_off: T + 1; adj: adj_off[-1]; mem_off: rows + 1)")
        rc = self._L.fclu_partition_adj(self._h, row_off.size - 1, row_off.ctypes.data, adj_off.ctypes.data, adj.ctypes.data if adj.size else None,
                                        mem_off.ctypes.data, mem.ctypes.data if mem.size else None, int(maximum_ilp_size))
        return self._partition_arrays("fclu_partition_adj", rc)

    @staticmethod
    def _reads(packed):
        r = _Reads(n_tint=packed["n_tint"])
        keep = []
        for name, dt in (("rep_off", np.int64), ("n_seg", np.int32), ("lab_off", np.int64), ("labels", np.uint32), ("tail", np.uint8)):
            a = np.ascontiguousarray(packed[name], dt)
            keep.append(a)
            setattr(r, name, a.ctypes.data if a.size else None)
        return r, keep

    def _prep_arrays(self):
        p = _Prep()
        rc = self._L.fclu_preprocess_results(self._h, ctypes.byref(p))
        if rc != 0:
            raise ClusterError("fclu_preprocess_results: " + self._L.fclu_last_error(self._h).decode(), rc)
        T, N, R = p.n_tint, int(p.n_reps), int(p.n_rows)
        out = dict(n_tint=T, n_reps=N, n_rows=R)
        for name in ("row_off", "bits_off", "adj_off", "rep_bits_off"):
            out[name] = _copy_out(getattr(p, name), T + 1, np.int64)
        n_rbits, n_bits = int(out["rep_bits_off"][-1]), int(out["bits_off"][-1])
        for name, n, dt in (("i_bits", n_rbits, np.uint32), ("c_bits", n_rbits, np.uint32), ("first", N, np.int32), ("last", N, np.int32),
                            ("raw_first", N, np.int32), ("raw_last", N, np.int32), ("rep_node", N, np.int32), ("node_rep", R, np.int32),
                            ("mem_off", R + 1, np.int64), ("mem", N, np.int32), ("bits", n_bits, np.uint32), ("node_first", R, np.int32),
                            ("node_last", R, np.int32), ("node_tail", R, np.uint8)):
            out[name] = _copy_out(getattr(p, name), n, dt)
        return out

    def preprocess(self, packed):
        """preprocess_ilp() per rep and the dedupe of a batch, on the device: packed = pack_labels().  Returns numpy arrays named as
        in include/freddie_cluster.h, fclu_prep (prep_structures() / prep_members() give pack_structures() / pack_members())."""
        r, keep = self._reads(packed)
        rc = self._L.fclu_preprocess(self._h, ctypes.byref(r))
        if rc != 0:
            raise ClusterError("fclu_preprocess: " + self._L.fclu_last_error(self._h).decode(), rc)
        return self._prep_arrays()

    def partition_labels(self, packed, maximum_ilp_size):
        """From label rows to tint['partitions'] of a batch in one device call: (preprocess() arrays, partition() arrays)."""
        r, keep = self._reads(packed)
        rc = self._L.fclu_partition_reads(self._h, ctypes.byref(r), int(maximum_ilp_size))
        parts = self._partition_arrays("fclu_partition_reads", rc)
        return self._prep_arrays(), parts

    @staticmethod
    def _segment(arrays):
        a = arrays.a if isinstance(arrays, SegmentArrays) else arrays
        g = _Segment(n_tint=int(a["n_tint"]))
        keep = []
        for name, dt in (("read_off", np.int64), ("n_seg", np.int32), ("lab_off", np.int64), ("labels", np.uint32), ("tok_off", np.int64),
                         ("tok", np.uint32), ("tail", np.uint8)):
            x = np.ascontiguousarray(a[name], dt)
            keep.append(x)
            setattr(g, name, x.ctypes.data if x.size else None)
        if keep[0].size != g.n_tint + 1 or keep[1].size != g.n_tint or keep[2].size != g.n_tint + 1 or g.n_tint < 0:
            raise ClusterError("group_reads: read_off / lab_off need n_tint + 1 entries, n_seg n_tint")
        n = int(keep[0][-1]) if g.n_tint else 0
        if n > 0 and (keep[4].size != n + 1 or keep[6].size != n or keep[3].size != int(keep[2][-1]) or
                      keep[5].size != max(int(keep[4][-1]), 0)):
            raise ClusterError("group_reads: array lengths do not match (tok_off: reads + 1; tail: reads; labels: lab_off[-1]; tok: tok_off[-1])")
        return g, keep

    def _group_arrays(self):
        g = _Groups()
        rc = self._L.fclu_group_results(self._h, ctypes.byref(g))
        if rc != 0:
            raise ClusterError("fclu_group_results: " + self._L.fclu_last_error(self._h).decode(), rc)
        T, N, R = g.n_tint, int(g.n_reads), int(g.n_reps)
        return dict(n_tint=T, n_reads=N, n_reps=R, rep_off=_copy_out(g.rep_off, T + 1, np.int64), read_rep=_copy_out(g.read_rep, N, np.int32),
                    rep_mem_off=_copy_out(g.rep_mem_off, R + 1, np.int64), rep_mem=_copy_out(g.rep_mem, N, np.int32),
                    rep_first=_copy_out(g.rep_first, R, np.int32))

    def group_reads(self, arrays):
        """read_segment()'s rep grouping of a batch on the device: arrays = read_segment_arrays() (or a dict of the fclu_segment
        arrays).  Returns numpy arrays named as in include/freddie_cluster.h, fclu_groups."""
        g, keep = self._segment(arrays)
        rc = self._L.fclu_group_reads(self._h, ctypes.byref(g))
        if rc != 0:
            raise ClusterError("fclu_group_reads: " + self._L.fclu_last_error(self._h).decode(), rc)
        return self._group_arrays()

    def partition_segment(self, arrays, maximum_ilp_size):
        """From all reads' rows and token streams to tint['partitions'] of a batch in one device call:
        (group_reads() arrays, preprocess() arrays of the reps, partition() arrays)."""
        g, keep = self._segment(arrays)
        rc = self._L.fclu_partition_segment(self._h, ctypes.byref(g), int(maximum_ilp_size))
        parts = self._partition_arrays("fclu_partition_segment", rc)
        return self._group_arrays(), self._prep_arrays(), parts

    def round_setup(self, gap_off, gaps, seg_off, seg_len):
        """Once per batch, behind partition_labels() / partition_segment() on this context: the reps' gap triples (j1, j2, l) (CSR by the
        batch's reps, round_gaps()) and the segments' lengths (CSR by tint)."""
        gap_off = np.ascontiguousarray(gap_off, np.int64)
        gaps = np.ascontiguousarray(gaps, np.int32).reshape(-1)
        seg_off = np.ascontiguousarray(seg_off, np.int64)
        seg_len = np.ascontiguousarray(seg_len, np.int32)
        if gap_off.size == 0 or seg_off.size == 0 or gaps.size != 3 * int(gap_off[-1]) or seg_len.size != int(seg_off[-1]):
            raise ClusterError("round_setup: array lengths do not match (gaps: 3 x gap_off[-1]; seg_len: seg_off[-1])")
        rc = self._L.fclu_round_setup(self._h, gap_off.ctypes.data, gaps.ctypes.data if gaps.size else None, seg_off.ctypes.data,
                                      seg_len.ctypes.data if seg_len.size else None)
        if rc != 0:
            raise ClusterError("fclu_round_setup: " + self._L.fclu_last_error(self._h).decode(), rc)

    def round_models(self, parts, remaining, fetch=True):
        """The ILP models of one round of many partitions, one device call (include/freddie_cluster.h, fclu_rounds): parts = partition
        ids numbered through the batch, remaining = per problem the remaining rep ids (local to the tint) in the caller's order.
        Returns the flat numpy arrays, pairs as [n, 2], grp as [n, 2], rows as [n, 3] (column, group, l); round_model() cuts one
        problem out.  refused[p] >= 0: the reference raises on problem p (a gap with an uninformative endpoint, :467-468), the value is
        the smallest offending column and the problem has no model.
        fetch=False (fclu_round_models_resident): the models stay on the device, where round_incumbents(), round_exact(), round_bnb() and
        round_readout() find them; only n_prob, the counts, refused, col_off, inf_bits_off and inf_bits come back, under resident=True,
        and round_model() refuses such a result."""
        part = np.ascontiguousarray(parts, np.int64)
        if len(remaining) != part.size:
            raise ClusterError("round_models: %d partitions, %d remaining lists" % (part.size, len(remaining)))
        rid_off = np.zeros(part.size + 1, np.int64)
        np.cumsum([len(r) for r in remaining], out=rid_off[1:])
        rids = np.fromiter((i for r in remaining for i in r), np.int32, int(rid_off[-1]))
        b = _RoundBatch(n_prob=part.size, part=part.ctypes.data if part.size else None, rid_off=rid_off.ctypes.data,
                        rids=rids.ctypes.data if rids.size else None)
        rc = (self._L.fclu_round_models if fetch else self._L.fclu_round_models_resident)(self._h, ctypes.byref(b))
        if rc != 0:
            raise ClusterError("fclu_round_models: " + self._L.fclu_last_error(self._h).decode(), rc)
        r = _Rounds()
        rc = self._L.fclu_round_results(self._h, ctypes.byref(r))
        if rc != 0:
            raise ClusterError("fclu_round_results: " + self._L.fclu_last_error(self._h).decode(), rc)
        P = r.n_prob
        out = dict(n_prob=P)
        for n in _ROUND_COUNTS:
            out[n] = int(getattr(r, n))
        if not fetch:
            out["resident"] = True
            out["inf_bits_off"], out["col_off"] = _copy_out(r.inf_bits_off, P + 1, np.int64), _copy_out(r.col_off, P + 1, np.int64)
            out["refused"], out["inf_bits"] = _copy_out(r.refused, P, np.int32), _copy_out(r.inf_bits, int(out["inf_bits_off"][-1]), np.uint32)
            return out
        for n in ("inf_bits_off", "inf_off", "col_off", "pair_off", "grp_off", "row_off"):
            out[n] = _copy_out(getattr(r, n), P + 1, np.int64)
        for n, cnt, dt in (("refused", P, np.int32), ("inf_bits", int(out["inf_bits_off"][-1]), np.uint32), ("inf_seg", out["n_inf"], np.int32),
                           ("sup_off", out["n_inf"] + 1, np.int64), ("sup_cols", out["n_sup"], np.int32), ("corr_off", out["n_cols"] + 1, np.int64),
                           ("corr_seg", out["n_corr"], np.int32), ("pairs", 2 * out["n_pairs"], np.int32), ("grp", 2 * out["n_grp"], np.int32),
                           ("grp_seg_off", out["n_grp"] + 1, np.int64), ("grp_seg", out["n_grp_seg"], np.int32),
                           ("grp_len", out["n_grp_seg"], np.int32), ("rows", 3 * out["n_gap_rows"], np.int32)):
            out[n] = _copy_out(getattr(r, n), cnt, dt)
        out["pairs"] = out["pairs"].reshape(-1, 2); out["grp"] = out["grp"].reshape(-1, 2); out["rows"] = out["rows"].reshape(-1, 3)
        return out

    def _garbage2(self, what, garbage):
        """Twice the garbage costs of the last round_models() call's columns as int32 (multiples of 0.5, as cluster_solve.garbage2()),
        and that call's col_off."""
        g = np.asarray(garbage, np.float64).reshape(-1)
        g2 = np.rint(2.0 * g)
        if g.size and not (np.isfinite(g).all() and (g2 == 2.0 * g).all() and (g2 >= 0).all() and (g2 < 2.0 ** 31).all()):
            bad = int(np.flatnonzero(~(np.isfinite(g) & (g2 == 2.0 * g) & (g2 >= 0) & (g2 < 2.0 ** 31)))[0])
            raise ClusterError("%s: garbage cost %r of column %d is not a multiple of 0.5 in [0, 2^30)" % (what, float(g[bad]), bad))
        r = _Rounds()
        rc = self._L.fclu_round_results(self._h, ctypes.byref(r))
        if rc != 0:
            raise ClusterError("%s: " % what + self._L.fclu_last_error(self._h).decode(), rc)
        if g.size != int(r.n_cols):
            raise ClusterError("%s: %d garbage costs for the %d columns of the last round_models() call" % (what, g.size, int(r.n_cols)))
        return np.ascontiguousarray(g2, np.int32), _copy_out(r.col_off, r.n_prob + 1, np.int64)

    def round_incumbents(self, garbage, epsilon, offset, max_seeds=64):
        """Greedy incumbents of the problems of the last round_models() call, one device call (include/freddie_cluster.h,
        fclu_incumbents; the definition is cluster_solve.greedy_incumbent()): garbage = the garbage cost of every column of that batch,
        problem by problem (multiples of 0.5).  Returns numpy arrays: cost2 (twice the cost; -1 for a refused problem), start,
        grow_steps, repair_steps per problem, mem_off / mem (the members, as columns, ascending) and col_off; round_incumbent() cuts
        one problem out."""
        g2, col_off = self._garbage2("round_incumbents", garbage)
        rc = self._L.fclu_round_incumbents(self._h, g2.ctypes.data if g2.size else None, 1.0 - float(epsilon), 1.0 + float(epsilon), int(offset),
                                           int(max_seeds))
        if rc != 0:
            raise ClusterError("fclu_round_incumbents: " + self._L.fclu_last_error(self._h).decode(), rc)
        i = _Incumbents()
        rc = self._L.fclu_round_incumbent_results(self._h, ctypes.byref(i))
        if rc != 0:
            raise ClusterError("fclu_round_incumbent_results: " + self._L.fclu_last_error(self._h).decode(), rc)
        P = i.n_prob
        return dict(n_prob=P, col_off=col_off, cost2=_copy_out(i.cost2, P, np.int64), start=_copy_out(i.start, P, np.int32),
                    grow_steps=_copy_out(i.grow_steps, P, np.int32), repair_steps=_copy_out(i.repair_steps, P, np.int32),
                    mem_off=_copy_out(i.mem_off, P + 1, np.int64), mem=_copy_out(i.mem, int(i.n_mem), np.int32))

    def _times(self, entry, *names):
        """What a *_timing entry point hands out, a float for each name."""
        v = [ctypes.c_float() for _ in names]
        entry(self._h, *[ctypes.byref(x) for x in v])
        return {n: x.value for n, x in zip(names, v)}

    def round_incumbent_timing(self):
        return self._times(self._L.fclu_round_incumbent_timing, "conflict_ms", "starts_ms", "pick_ms")

    def round_exact(self, garbage, epsilon, offset, max_cols, max_masks):
        """The proven optimum of every small problem of the last round_models() call by enumeration, one device call
        (include/freddie_cluster.h, fclu_exact; the definition is cluster_solve.exact_small()): garbage as round_incumbents'; a problem
        is taken when it has a model, at most max_cols (<= 24) columns and 2^columns fits what is left of max_masks, in ascending
        (columns, problem).  Returns numpy arrays cost2 (twice the cost; -1: no feasible subset; -2: not taken or refused) and mask (bit c
        = column c) per problem, col_off, and n_taken, n_masks, n_launches; round_exact_solution() cuts one problem out."""
        g2, col_off = self._garbage2("round_exact", garbage)
        rc = self._L.fclu_round_exact(self._h, g2.ctypes.data if g2.size else None, 1.0 - float(epsilon), 1.0 + float(epsilon), int(offset),
                                      int(max_cols), int(max_masks))
        if rc != 0:
            raise ClusterError("fclu_round_exact: " + self._L.fclu_last_error(self._h).decode(), rc)
        x = _Exact()
        rc = self._L.fclu_round_exact_results(self._h, ctypes.byref(x))
        if rc != 0:
            raise ClusterError("fclu_round_exact_results: " + self._L.fclu_last_error(self._h).decode(), rc)
        P = x.n_prob
        return dict(n_prob=P, col_off=col_off, cost2=_copy_out(x.cost2, P, np.int64), mask=_copy_out(x.mask, P, np.uint32),
                    n_taken=int(x.n_taken), n_masks=int(x.n_masks), n_launches=int(x.n_launches))

    def round_exact_timing(self):
        return self._times(self._L.fclu_round_exact_timing, "prep_ms", "search_ms", "longest_launch_ms")

    def round_bnb(self, garbage, ub2, epsilon, offset, min_cols, max_cols, max_nodes, depth=cluster_solve.BNB_DEPTH, node_cap=cluster_solve.BNB_NODE_CAP):
        """A branch and bound over every problem of min_cols .. max_cols (<= 64) columns of the last round_models() call, one device call
        (include/freddie_cluster.h, fclu_bnb; the definition is cluster_solve.exact_bnb()): garbage as round_incumbents'; ub2 = per problem
        twice the cost of a known feasible set, or a negative number (e.g. round_incumbents()' cost2); a problem is taken in ascending
        (columns, problem) while 2^min(columns, depth) * node_cap fits what is left of max_nodes.  Returns numpy arrays status (0 optimal,
        1 infeasible, 2 unproven, -2 not taken or refused), cost2 (-1: no set found), mask (uint64, bit c = column c), nodes and capped per
        problem, col_off, and n_taken, n_launches, nodes_total; round_bnb_solution() cuts one problem out."""
        g2, col_off = self._garbage2("round_bnb", garbage)
        out = self._round_search("round_bnb", g2, col_off, ub2, epsilon, offset, min_cols, max_cols, max_nodes, depth, node_cap, 1)
        out["mask"] = out["mask"].reshape(-1)
        return out

    def _round_search(self, name, g2, col_off, ub2, epsilon, offset, min_cols, max_cols, max_nodes, depth, node_cap, words, passes=None):
        """round_bnb() and round_bnb_wide() behind their own arguments: the entry points fclu_<name> / fclu_<name>_results, the resolved
        depth and node_cap, and the words of a problem's mask (fclu_bnb_wide has fclu_bnb's layout, so _Bnb reads both); mask comes
        back as a (problems, words) array.  passes: not None = through fclu_<name>_passes."""
        ub = np.ascontiguousarray(np.asarray(ub2, np.int64).reshape(-1))
        if ub.size != col_off.size - 1:
            raise ClusterError("%s: %d bounds for the %d problems of the last round_models() call" % (name, ub.size, col_off.size - 1))
        entry, more = ("fclu_" + name, ()) if passes is None else ("fclu_%s_passes" % name, (int(passes),))
        rc = getattr(self._L, entry)(self._h, g2.ctypes.data if g2.size else None, ub.ctypes.data if ub.size else None, 1.0 - float(epsilon),
                                     1.0 + float(epsilon), int(offset), int(min_cols), int(max_cols), int(depth), int(node_cap), int(max_nodes), *more)
        if rc != 0:
            raise ClusterError("%s: " % entry + self._L.fclu_last_error(self._h).decode(), rc)
        b = _Bnb()
        rc = getattr(self._L, "fclu_%s_results" % name)(self._h, ctypes.byref(b))
        if rc != 0:
            raise ClusterError("fclu_%s_results: " % name + self._L.fclu_last_error(self._h).decode(), rc)
        P = b.n_prob
        return dict(n_prob=P, col_off=col_off, status=_copy_out(b.status, P, np.int32), cost2=_copy_out(b.cost2, P, np.int64),
                    mask=_copy_out(b.mask, P * words, np.uint64).reshape(P, words), nodes=_copy_out(b.nodes, P, np.int64),
                    capped=_copy_out(b.capped, P, np.int32), n_taken=int(b.n_taken), n_launches=int(b.n_launches), nodes_total=int(b.nodes_total))

    def round_bnb_timing(self):
        return self._times(self._L.fclu_round_bnb_timing, "prep_ms", "search_ms", "longest_launch_ms")

    def round_bnb_wide(self, garbage, ub2, epsilon, offset, min_cols, max_cols, max_nodes, depth=None, node_cap=None, passes=1):
        """round_bnb() for the problems of min_cols .. max_cols (<= 1024) columns whose tables fit (bnb_wide_lds_bytes), one device call
        (include/freddie_cluster.h, fclu_bnb_wide; the definition is cluster_solve.exact_bnb_wide()).  depth None = cluster_solve.BNB_DEPTH;
        node_cap None = cluster_solve.bnb_wide_node_cap(R) of the round's largest problem of min_cols .. max_cols columns (a call has one
        cap: the measured defaults are per size, and the largest problem is the one that decides a launch's time).  Returns round_bnb()'s dict with mask as a (problems, 16) uint64 array,
        low word first, and the depth and node_cap used; round_bnb_wide_solution() cuts one problem out.  passes > 1: the capped tasks' open
        subtrees are run as tasks of further passes (fclu_round_bnb_wide_passes; cluster_solve.exact_bnb_wide(passes=...)); capped then
        counts the tasks still open, and round_bnb_wide_pass_stats() has a row a pass.  passes == 1 makes fclu_round_bnb_wide's call."""
        depth = cluster_solve.BNB_DEPTH if depth is None else depth
        g2, col_off = self._garbage2("round_bnb_wide", garbage)
        if node_cap is None:
            cols = np.diff(col_off)
            cols = cols[(cols >= int(min_cols)) & (cols <= int(max_cols))]
            node_cap = cluster_solve.bnb_wide_node_cap(int(cols.max()) if cols.size else int(max_cols))
        out = self._round_search("round_bnb_wide", g2, col_off, ub2, epsilon, offset, min_cols, max_cols, max_nodes, depth, node_cap, BNB_WIDE_WORDS,
                                 None if int(passes) == 1 else passes)
        out.update(depth=int(depth), node_cap=int(node_cap), passes=int(passes))
        return out

    def round_bnb_wide_pass_stats(self):
        """The passes of the last round_bnb_wide() call that ran: a list of dict(tasks, nodes, capped, launches, problems)."""
        rows = np.zeros((BNB_WIDE_MAX_PASSES, 5), np.int64)
        rc = self._L.fclu_round_bnb_wide_pass_stats(self._h, rows.ctypes.data, BNB_WIDE_MAX_PASSES)
        if rc != 0:
            raise ClusterError("fclu_round_bnb_wide_pass_stats: " + self._L.fclu_last_error(self._h).decode(), rc)
        return [dict(zip(("tasks", "nodes", "capped", "launches", "problems"), map(int, row))) for row in rows if row[0] > 0]

    def round_bnb_wide_timing(self):
        return self._times(self._L.fclu_round_bnb_wide_timing, "prep_ms", "search_ms", "longest_launch_ms")

    def round_readout(self, sets):
        """The isoforms of the last round_models() call's problems (either form) from their accepted column sets, one device call
        (include/freddie_cluster.h, fclu_readout; the definition is cluster.read_out()): sets = per problem the accepted columns, ascending,
        or an empty list for "no isoform this round".  Returns numpy arrays: exons (uint8 0 / 1, M_t a problem with a set) under exon_off;
        corr (ASCII bytes, M_t a member, in set order; member k of problem p starts at corr_off[p] + k * M_t); e (the exon values at the
        informative segments) under e_off; mem_off; and n_sets, n_mem.  readout_isoform() cuts one problem out."""
        r = _Rounds()
        rc = self._L.fclu_round_results(self._h, ctypes.byref(r))
        if rc != 0:
            raise ClusterError("round_readout: " + self._L.fclu_last_error(self._h).decode(), rc)
        if len(sets) != r.n_prob:
            raise ClusterError("round_readout: %d sets for the %d problems of the last round_models() call" % (len(sets), r.n_prob))
        sel_off = np.zeros(len(sets) + 1, np.int64)
        np.cumsum([len(x) for x in sets], out=sel_off[1:])
        sel = np.fromiter((c for x in sets for c in x), np.int32, int(sel_off[-1]))
        rc = self._L.fclu_round_readout(self._h, sel_off.ctypes.data, sel.ctypes.data if sel.size else None)
        if rc != 0:
            raise ClusterError("fclu_round_readout: " + self._L.fclu_last_error(self._h).decode(), rc)
        o = _Readout()
        rc = self._L.fclu_round_readout_results(self._h, ctypes.byref(o))
        if rc != 0:
            raise ClusterError("fclu_round_readout_results: " + self._L.fclu_last_error(self._h).decode(), rc)
        P = o.n_prob
        if P != len(sets):
            raise ClusterError("round_readout: %d sets for the %d problems of the last round_models() call" % (len(sets), P))
        return dict(n_prob=P, n_sets=int(o.n_sets), n_mem=int(o.n_mem), exon_off=_copy_out(o.exon_off, P + 1, np.int64),
                    exons=_copy_out(o.exons, int(o.n_exon_bytes), np.uint8), mem_off=_copy_out(o.mem_off, P + 1, np.int64),
                    corr_off=_copy_out(o.corr_off, P + 1, np.int64), corr=_copy_out(o.corr, int(o.n_corr_bytes), np.uint8),
                    e_off=_copy_out(o.e_off, P + 1, np.int64), e=_copy_out(o.e, int(o.n_e), np.uint8), sel=sel)

    def round_readout_timing(self):
        return self._times(self._L.fclu_round_readout_timing, "exons_ms", "corr_ms")

    def readout_paths(self):
        """The launch census of the last round_readout() call (include/freddie_cluster.h, FCLU_PATH_READOUT_*): sets (problems with a
        set), members, wide_stores / byte_stores (some lane stores 16 bytes at once / some byte is stored alone, as the host predicts
        it from the rows' addresses; the kernel reports nothing)."""
        v = np.zeros(len(_PATHS) + len(_READOUT_PATHS), np.int32)
        rc = self._L.fclu_last_paths(self._h, v.ctypes.data, v.size)
        if rc != 0:
            raise ClusterError("fclu_last_paths: bad arguments", rc)
        sets, members, stores = v[len(_PATHS):].tolist()
        return dict(sets=sets, members=members, wide_stores=bool(stores & STORE_WIDE), byte_stores=bool(stores & STORE_BYTES))

    def round_timing(self):
        return self._times(self._L.fclu_round_timing, "count_ms", "gaps_ms", "fill_ms")

    def group_timing(self):
        return self._times(self._L.fclu_group_timing, "keys_ms", "dedupe_ms")

    def preprocess_timing(self):
        return self._times(self._L.fclu_preprocess_timing, "rows_ms", "dedupe_ms")

    def partition_timing(self):
        return self._times(self._L.fclu_partition_timing, "components_ms", "pairs_ms")

    def last_timing(self):
        return self._times(self._L.fclu_last_timing, "compat_ms", "prune_ms")

    def last_paths(self):
        """The launch census of the last call that built a graph (include/freddie_cluster.h, fclu_last_paths): compat_form "rank" /
        "masked", tiles, lds_tints, pass_kernel None / "edge_walk" / "or_of_rows", edge_chunks, passes_enqueued, passes_ran."""
        v = np.zeros(len(_PATHS), np.int32)
        rc = self._L.fclu_last_paths(self._h, v.ctypes.data, v.size)
        if rc != 0:
            raise ClusterError("fclu_last_paths: bad arguments", rc)
        out = dict(zip(_PATHS, v.tolist()))
        out["compat_form"] = (None, "rank", "masked")[out["compat_form"]]
        out["pass_kernel"] = (None, "edge_walk", "or_of_rows")[out["pass_kernel"]]
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._L.fclu_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------------------------
# a round's models (run_ilp :347-535 up to the solver): the inputs of Context.round_setup() and one problem of Context.round_models()
# ---------------------------------------------------------------------------------------------------------------
def round_gaps(tints):
    """(gap_off, gaps [n, 3], seg_off, seg_len) of preprocessed tints for Context.round_setup(): per rep the (j1, j2, l) of its first
    read's gaps dict, pseudo-gaps included, in the dict's order."""
    gap_off, gaps, seg_off, seg_len = [0], [], [0], []
    for tint in tints:
        for members in tint["read_reps"]:
            gaps.extend((j1, j2, l) for (j1, j2), l in tint["reads"][members[0]]["gaps"].items())
            gap_off.append(len(gaps))
        seg_len.extend(s[2] for s in tint["segs"])
        seg_off.append(len(seg_len))
    return (np.array(gap_off, np.int64), np.array(gaps, np.int32).reshape(-1, 3), np.array(seg_off, np.int64), np.array(seg_len, np.int32))


def round_model(arr, p):
    """Problem p of Context.round_models() as plain lists, or None when it was refused: informative (bit row as a list of 0 / 1 is the
    caller's, from inf_bits), inf_seg, support (per informative segment its columns), corrections (per column its segments), pairs,
    groups [(j1, j2)], group_segs (per group [(j, length)]), gap_rows [(column, group, l)]."""
    if isinstance(arr, dict) and arr.get("resident"):
        raise ClusterError("round_model: the models of this round_models(fetch=False) call stayed on the device; problem %d has none on the host" % p)
    if arr["refused"][p] >= 0:
        return None
    i0, i1 = int(arr["inf_off"][p]), int(arr["inf_off"][p + 1])
    c0, c1 = int(arr["col_off"][p]), int(arr["col_off"][p + 1])
    g0, g1 = int(arr["grp_off"][p]), int(arr["grp_off"][p + 1])
    so, co, go = arr["sup_off"].tolist(), arr["corr_off"], arr["grp_seg_off"]
    sup, corr, gs, gl = arr["sup_cols"], arr["corr_seg"], arr["grp_seg"], arr["grp_len"]
    return dict(n_cols=c1 - c0, words=arr["inf_bits"][int(arr["inf_bits_off"][p]):int(arr["inf_bits_off"][p + 1])].tolist(),
                inf_seg=arr["inf_seg"][i0:i1].tolist(),
                support=[sup[so[k]:so[k + 1]].tolist() for k in range(i0, i1)],
                corrections=[corr[int(co[c]):int(co[c + 1])].tolist() for c in range(c0, c1)],
                pairs=[tuple(x) for x in arr["pairs"][int(arr["pair_off"][p]):int(arr["pair_off"][p + 1])].tolist()],
                groups=[tuple(x) for x in arr["grp"][g0:g1].tolist()],
                group_segs=[list(zip(gs[int(go[g]):int(go[g + 1])].tolist(), gl[int(go[g]):int(go[g + 1])].tolist())) for g in range(g0, g1)],
                gap_rows=[tuple(x) for x in arr["rows"][int(arr["row_off"][p]):int(arr["row_off"][p + 1])].tolist()])


def readout_isoform(out, p, remaining):
    """Problem p of Context.round_readout() as cluster.read_out() returns it and the solver's e: (dict(exons, rid_to_corrections), e), or
    None when the problem had no set.  remaining: the problem's rep ids in its column order."""
    a, b = int(out["exon_off"][p]), int(out["exon_off"][p + 1])
    m0, m1 = int(out["mem_off"][p]), int(out["mem_off"][p + 1])
    if m0 == m1:
        return None
    M, c0 = b - a, int(out["corr_off"][p])
    text = out["corr"][c0:c0 + (m1 - m0) * M].tobytes().decode("ascii")
    members = out["sel"][m0:m1].tolist()
    return (dict(exons=out["exons"][a:b].tolist(), rid_to_corrections={remaining[c]: list(text[k * M:(k + 1) * M]) for k, c in enumerate(members)}),
            out["e"][int(out["e_off"][p]):int(out["e_off"][p + 1])].tolist())


def readout_words(I, C, labels, inf, members, M, rule=None):
    """One problem: I, C = uint32 [R, W] bit rows of its columns, labels = uint32 [R, LW] label rows (two bits a label), inf = uint32 [W],
    members = the accepted columns.  Returns (exon words uint32 [W], corrections uint8 [len(members), M]).  rule names the one step left
    out (the tests' mutations): "first_member" (the uninformative value from the first member instead of column 0), "x_without_exon"
    ('X' wherever C is 1), "no_dash" ('-' dropped), "label2_as_0", "no_tail_mask" (the last word's bits behind M kept)."""
    W = I.shape[1]
    valid = np.full(W, 0xffffffff, np.uint32)
    for w in range(W):                                       # ro_valid
        n = min(max(M - 32 * w, 0), 32)
        valid[w] = 0xffffffff if n >= 32 else (1 << n) - 1
    if rule == "no_tail_mask":
        valid[:] = 0xffffffff
    member_or = np.bitwise_or.reduce(I[members], axis=0) if len(members) else np.zeros(W, np.uint32)
    base = I[members[0]] if rule == "first_member" else I[0]
    inf = inf & valid
    ex = ((member_or & inf) | (base & ~inf)) & valid         # ro_exon_word
    j = np.arange(M)
    bit = lambda words: (words[..., j >> 5] >> (j & 31).astype(np.uint32)) & 1
    corr = np.zeros((len(members), M), np.uint8)
    for k, c in enumerate(members):                          # ro_corr_byte
        code = (labels[c][j >> 4] >> (2 * (j & 15)).astype(np.uint32)) & 3
        if rule == "label2_as_0":
            code = np.where(code == 2, 0, code)
        row = (ord("0") + code).astype(np.uint8)
        x = (bit(C[c]) & (1 if rule == "x_without_exon" else bit(ex))) == 1
        on = bit(inf) == 1
        if rule == "no_dash":
            row[x] = ord("X")
        else:
            row[x & on] = ord("X")
            row[~on] = ord("-")
        corr[k] = row
    return ex, corr


def _pack_bits(rows, M):
    W = max((M + 31) // 32, 1)
    a = np.zeros((len(rows), W * 32), np.uint8)
    if M and len(rows):
        a[:, :M] = np.asarray(rows, np.uint8).reshape(len(rows), M)
    return np.packbits(a, axis=1, bitorder="little").view(np.uint32).reshape(len(rows), W)


def readout_rows(tint, remaining):
    """(I, C, labels) of a problem's columns as readout_words() wants them, from a preprocessed tint dict."""
    M = len(tint["segs"])
    I, C = tint["ilp_data"]["I"], tint["ilp_data"]["C"]
    LW = max((M + 15) // 16, 1)
    labels = np.zeros((len(remaining), LW), np.uint32)
    for c, i in enumerate(remaining):
        data = tint["reads"][tint["read_reps"][i][0]]["data"]
        for j in range(M):
            labels[c, j >> 4] |= np.uint32((data[j] & 3) << (2 * (j & 15)))
    return _pack_bits([I[i] for i in remaining], M), _pack_bits([C[i] for i in remaining], M), labels


def readout_mirror(tints, problems, sets, informative, rule=None):
    """What Context.round_readout() returns, in numpy: the word arithmetic of freddie_amd/csrc/clu_readout.h on packed rows, so that the
    kernels' code and this agree word by word (tools/readout_host_check.py) and this and cluster.read_out() agree on every case the tests
    name.  problems = [(tint index, remaining rep ids)], sets = per problem the accepted columns, informative = per problem the 0 / 1
    list of its segments (inf_bits unpacked).  rule: one step of readout_words() left out (tests)."""
    exons, corr, e, exon_off, corr_off, e_off, mem_off, sel = [], [], [], [0], [0], [0], [0], []
    for (t, remaining), members, inf in zip(problems, sets, informative):
        members = list(members)
        if members:
            M = len(tints[t]["segs"])
            I, C, labels = readout_rows(tints[t], remaining)
            inf_w = _pack_bits([inf], M)[0]
            ex, rows = readout_words(I, C, labels, inf_w, members, M, rule)
            j = np.arange(M)
            row = ((ex[j >> 5] >> (j & 31).astype(np.uint32)) & 1).astype(np.uint8)
            exons.append(row); corr.append(rows.reshape(-1)); e.append(row[np.flatnonzero(np.asarray(inf[:M]))])
            sel.extend(members)
        exon_off.append(exon_off[-1] + (len(exons[-1]) if members else 0))
        corr_off.append(corr_off[-1] + (len(corr[-1]) if members else 0))
        e_off.append(e_off[-1] + (len(e[-1]) if members else 0))
        mem_off.append(len(sel))
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return dict(n_prob=len(problems), n_sets=len(exons), n_mem=len(sel), exon_off=np.array(exon_off, np.int64), exons=cat(exons),
                mem_off=np.array(mem_off, np.int64), corr_off=np.array(corr_off, np.int64), corr=cat(corr), e_off=np.array(e_off, np.int64),
                e=cat(e), sel=np.array(sel, np.int32))


def round_incumbent(arr, p):
    """Problem p of Context.round_incumbents(): (cost, x) -- the cost and a 0 / 1 per column -- or None when the problem was refused."""
    if arr["cost2"][p] < 0:
        return None
    x = [0] * int(arr["col_off"][p + 1] - arr["col_off"][p])
    for c in arr["mem"][int(arr["mem_off"][p]):int(arr["mem_off"][p + 1])].tolist():
        x[c] = 1
    return int(arr["cost2"][p]) / 2.0, x


def round_exact_solution(arr, p):
    """Problem p of Context.round_exact(): (cost, x) -- the proven optimum's cost and a 0 / 1 per column --, "infeasible" when no subset
    of the columns is feasible, or None when the problem was not taken."""
    cost2 = int(arr["cost2"][p])
    if cost2 == -1:
        return "infeasible"
    if cost2 < 0:
        return None
    mask = int(arr["mask"][p])
    return cost2 / 2.0, [mask >> c & 1 for c in range(int(arr["col_off"][p + 1] - arr["col_off"][p]))]


def round_bnb_solution(arr, p):
    """Problem p of Context.round_bnb(): (cost, x) -- a proven optimum's cost and a 0 / 1 per column --, "infeasible" when no subset of
    the columns is feasible, ("unproven", cost, x) -- the best set the search found before a task ran into its node cap --,
    ("unproven", None, None) when it found none, or None when the problem was not taken."""
    status = BNB_STATUS[int(arr["status"][p])]
    if status is None or status == "infeasible":
        return status
    cost2, mask = int(arr["cost2"][p]), int(arr["mask"][p])
    found = (cost2 / 2.0, [mask >> c & 1 for c in range(int(arr["col_off"][p + 1] - arr["col_off"][p]))]) if cost2 >= 0 else (None, None)
    return found if status == "optimal" else ("unproven",) + found


BNB_WIDE_WORDS = 16           # words of a set of Context.round_bnb_wide() (FCLU_BNB_WIDE_WORDS)
BNB_WIDE_MAX_PASSES = 16      # passes of one Context.round_bnb_wide() call at the most
BNB_WIDE_MAX_PASS_TASKS = 1 << 16   # a problem whose next pass would hold more tasks is not continued (exact_bnb_wide()'s max_tasks)
BNB_WIDE_LDS_BYTES = 160 * 1024
BNB_WIDE_WAVES = 8


def bnb_wide_lds_bytes(R, E):
    """The LDS fclu_round_bnb_wide needs for a problem of R columns and E informative segments (bw_lds_bytes of csrc/clu_bnb_wide.h, the
    same formula): it is taken only when this is at most BNB_WIDE_LDS_BYTES."""
    W, EW = max(1, (R + 63) // 64), (E + 63) // 64
    return (8 * 2 * R * EW + 4 * R + 8 * BNB_WIDE_WAVES * (9 * W + 2 * EW) + 15) & ~15


def wide_mask(words):
    """A set of Context.round_bnb_wide() (16 words, low word first) as one Python integer, bit c = column c."""
    return sum(int(w) << (64 * i) for i, w in enumerate(words))


def round_bnb_wide_solution(arr, p):
    """Problem p of Context.round_bnb_wide(), by round_bnb_solution()'s convention; x is a list of R zeros and ones."""
    status = BNB_STATUS[int(arr["status"][p])]
    if status is None or status == "infeasible":
        return status
    cost2, mask = int(arr["cost2"][p]), wide_mask(arr["mask"][p])
    found = (cost2 / 2.0, [mask >> c & 1 for c in range(int(arr["col_off"][p + 1] - arr["col_off"][p]))]) if cost2 >= 0 else (None, None)
    return found if status == "optimal" else ("unproven",) + found


# ---------------------------------------------------------------------------------------------------------------
# partition_reads (:196-274)
# ---------------------------------------------------------------------------------------------------------------
_TAIL_CODE = {"N": 0, "S": 1, "E": 2}


def unique_structures(tint):
    """[(structure, [rep ids])] in first-occurrence order: reps with the same I row, first/last and tail category (:203-215)."""
    reads, read_reps = tint["reads"], tint["read_reps"]
    I, FL = tint["ilp_data"]["I"], tint["ilp_data"]["FL"]
    seen = dict()
    for i in sorted(I.keys()):
        d = (tuple(I[i]), (FL[i][0], FL[i][1], reads[read_reps[i][0]]["poly_tail_category"]))
        seen.setdefault(d, []).append(i)
    return list(seen.items())


def pack_structures(unique_per_tint):
    """Flat arrays of include/freddie_cluster.h for a list of unique_structures() results."""
    T = len(unique_per_tint)
    row_off = np.zeros(T + 1, np.int64); bits_off = np.zeros(T + 1, np.int64); adj_off = np.zeros(T + 1, np.int64)
    n_seg = np.zeros(T, np.int32)
    bits, first, last, tail = [], [], [], []
    for t, uniq in enumerate(unique_per_tint):
        n = len(uniq)
        M = len(uniq[0][0][0]) if n else 0
        W = max((M + 31) // 32, 1)
        n_seg[t] = M
        row_off[t + 1] = row_off[t] + n
        bits_off[t + 1] = bits_off[t] + n * W
        adj_off[t + 1] = adj_off[t] + n * ((n + 63) // 64)
        if n:
            rows = np.zeros((n, W * 32), np.uint8)
            if M:
                rows[:, :M] = np.array([u[0][0] for u in uniq], np.uint8).reshape(n, M)
            bits.append(np.packbits(rows, axis=1, bitorder="little").view(np.uint32).reshape(-1))
            first.extend(u[0][1][0] for u in uniq)
            last.extend(u[0][1][1] for u in uniq)
            tail.extend(_TAIL_CODE[u[0][1][2]] for u in uniq)
    return dict(n_tint=T, row_off=row_off, n_seg=n_seg, bits_off=bits_off,
                bits=np.concatenate(bits) if bits else np.zeros(0, np.uint32), first=np.array(first, np.int32),
                last=np.array(last, np.int32), tail=np.array(tail, np.uint8), adj_off=adj_off)


def pack_members(unique_per_tint):
    """dict(mem_off int64[rows + 1], mem int32): the rep ids of every unique row of the batch, rows in pack_structures() order."""
    counts = [len(u[1]) for uniq in unique_per_tint for u in uniq]
    mem_off = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=mem_off[1:])
    mem = np.fromiter((rid for uniq in unique_per_tint for u in uniq for rid in u[1]), np.int32, int(mem_off[-1]))
    return dict(mem_off=mem_off, mem=mem)


def adjacency_matrix(adj, packed, t):
    """Boolean N_t x N_t matrix of tint t from the packed result."""
    n = int(packed["row_off"][t + 1] - packed["row_off"][t])
    aw = (n + 63) // 64
    words = adj[int(packed["adj_off"][t]):int(packed["adj_off"][t + 1])].reshape(n, aw) if n else np.zeros((0, 0), np.uint64)
    return np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool) if n else np.zeros((0, 0), bool)


def _components(A):
    """Connected components as sorted lists, ordered by their smallest node (networkx yields them in node order, :257)."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    n = A.shape[0]
    if n == 0:
        return []
    _, lab = connected_components(csr_matrix(A), directed=False)
    order = np.argsort(lab, kind="stable")
    groups = np.split(order, np.flatnonzero(np.diff(lab[order])) + 1)
    return sorted((g.tolist() for g in groups), key=lambda g: g[0])


def _partitions_from_graph(unique, A, maximum_ilp_size, verbose):
    parts = []
    for comp in _components(A):
        for c in split_list_evenly(comp, maximum_ilp_size):
            if verbose:
                print(len(c), c[:10])                       # the reference prints this line (:262)
            rids, incomp = [], []
            for idx, i in enumerate(c):
                rids.extend(unique[i][1])
                for j in c[idx + 1:]:
                    if A[i, j]:
                        continue
                    for rid_1 in unique[i][1]:
                        for rid_2 in unique[j][1]:
                            incomp.append((rid_1, rid_2))
            parts.append((rids, incomp))
    return parts


# ---------------------------------------------------------------------------------------------------------------
# the front on the device: label rows in, preprocess_ilp() + the dedupe (+ everything behind it) out
# ---------------------------------------------------------------------------------------------------------------
def tail_categories(tint):
    """uint8 per rep: 0 'N', 1 'S', 2 'E' -- the category preprocess_ilp() gives the rep's first read (:291-300)."""
    reads = tint["reads"]
    out = np.zeros(len(tint["read_reps"]), np.uint8)
    for i, members in enumerate(tint["read_reps"]):
        pt = reads[members[0]]["poly_tail"]
        if len(pt) == 1:
            (key, (length, _)), = pt.items()
            if length > 10:
                out[i] = 1 if key in ("SA", "ST") else 2 if key in ("EA", "ET") else 0
    return out


def pack_labels(tints):
    """The fclu_reads arrays (include/freddie_cluster.h) of read_segment() tints: a rep's row is its first read's labels, two bits
    a label, sixteen labels a uint32 word."""
    T = len(tints)
    rep_off = np.zeros(T + 1, np.int64); lab_off = np.zeros(T + 1, np.int64)
    n_seg = np.zeros(T, np.int32)
    labels, tails = [], []
    for t, tint in enumerate(tints):
        reads, reps = tint["reads"], tint["read_reps"]
        n, M = len(reps), len(tint["segs"])
        LW = max((M + 15) // 16, 1)
        n_seg[t] = M
        rep_off[t + 1] = rep_off[t] + n
        lab_off[t + 1] = lab_off[t] + n * LW
        if n:
            codes = np.zeros((n, LW * 16), np.uint8)
            if M:
                raw = b"".join(bytes(reads[m[0]]["data"][:M]) for m in reps)        # (labels are small ints: one C loop a row)
                codes[:, :M] = np.frombuffer(raw, np.uint8).reshape(n, M) & 3
            q = codes.reshape(n, LW * 4, 4)                                          # four labels a byte, the first in the low bits;
            by = q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)
            labels.append(np.ascontiguousarray(by).view("<u4").astype(np.uint32, copy=False).reshape(-1))   # words: little-endian
            tails.append(tail_categories(tint))
    return dict(n_tint=T, rep_off=rep_off, n_seg=n_seg, lab_off=lab_off,
                labels=np.concatenate(labels) if labels else np.zeros(0, np.uint32),
                tail=np.concatenate(tails) if tails else np.zeros(0, np.uint8))


def prep_structures(prep, n_seg):
    """pack_structures() of the batch's unique rows, from Context.preprocess() arrays."""
    return dict(n_tint=prep["n_tint"], row_off=prep["row_off"], n_seg=np.asarray(n_seg, np.int32), bits_off=prep["bits_off"],
                bits=prep["bits"], first=prep["node_first"], last=prep["node_last"], tail=prep["node_tail"], adj_off=prep["adj_off"])


def prep_members(prep):
    """pack_members() of the batch's unique rows, from Context.preprocess() arrays."""
    return dict(mem_off=prep["mem_off"], mem=prep["mem"])


def _ilp_data_from_prep(tints, packed, prep, ilp_settings):
    """Leaves every tint as preprocess_ilp() leaves it, from the device's per-rep arrays."""
    for t, tint in enumerate(tints):
        r0, r1 = int(packed["rep_off"][t]), int(packed["rep_off"][t + 1])
        n, M = r1 - r0, int(packed["n_seg"][t])
        W = max((M + 31) // 32, 1)
        b0 = int(prep["rep_bits_off"][t])
        rows = {}
        for name in ("i_bits", "c_bits"):
            words = prep[name][b0:b0 + n * W].reshape(n, W)
            rows[name] = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :M].tolist() if n else []
        first, last = prep["first"][r0:r1].tolist(), prep["last"][r0:r1].tolist()
        raw_first, raw_last = prep["raw_first"][r0:r1].tolist(), prep["raw_last"][r0:r1].tolist()
        tail = packed["tail"][r0:r1].tolist()
        reads, read_reps = tint["reads"], tint["read_reps"]
        I, C, FL = dict(), dict(), dict()
        for i, members in enumerate(read_reps):
            read = reads[members[0]]
            I[i], C[i], FL[i] = rows["i_bits"][i], rows["c_bits"][i], (first[i], last[i])
            cat = "NSE"[tail[i]]
            if cat == "S":
                read["gaps"][(-1, raw_first[i])] = next(iter(read["poly_tail"].values()))[1]
            elif cat == "E":
                read["gaps"][(raw_last[i], M)] = next(iter(read["poly_tail"].values()))[1]
            for ridx in members:
                reads[ridx]["poly_tail_category"] = cat
                reads[ridx]["gaps"] = read["gaps"]
        garbage_cost = {}
        for i in range(len(read_reps)):
            if ilp_settings["recycle_model"] == "exons":
                garbage_cost[i] = len(read_reps[i]) * garbage_cost_exons(I=I[i])      # a list: raises like the reference (:314)
            elif ilp_settings["recycle_model"] == "introns":
                garbage_cost[i] = len(read_reps[i]) * garbage_cost_introns(C=C[i])  # a list: raises like the reference (:316)
            elif ilp_settings["recycle_model"] == "constant":
                garbage_cost[i] = len(read_reps[i]) * 3
        tint["ilp_data"] = dict(FL=FL, I=I, C=C, garbage_cost=garbage_cost)


def preprocess_ilp_batch(tints, ilp_settings, ctx):
    """preprocess_ilp() of several read_segment() tints with one device call: every tint is left as preprocess_ilp() leaves it."""
    packed = pack_labels(tints)
    _ilp_data_from_prep(tints, packed, ctx.preprocess(packed), ilp_settings)


def cluster_arrays_batch(tints, maximum_ilp_size, ctx):
    """From read_segment() tints that are not preprocessed to the flat arrays of Context.partition(), one device call:
    (pack_labels() arrays, Context.preprocess() arrays, partition arrays)."""
    packed = pack_labels(tints)
    prep, parts = ctx.partition_labels(packed, maximum_ilp_size)
    return packed, prep, parts


def partition_arrays_batch(tints, maximum_ilp_size, ctx):
    """partition_reads() of several preprocessed tints as the flat arrays of Context.partition(): one device call."""
    uniq = [unique_structures(t) for t in tints]
    return ctx.partition(pack_structures(uniq), pack_members(uniq), maximum_ilp_size)


def _partitions_from_arrays(arr, t, verbose):
    """tint['partitions'] of tint t of the batch: [(rep ids, [(rid_1, rid_2), ...]), ...]."""
    parts = []
    node_off, rid_off, pair_off = arr["part_node_off"], arr["part_rid_off"], arr["part_pair_off"]
    for q in range(int(arr["tint_part_off"][t]), int(arr["tint_part_off"][t + 1])):
        if verbose:
            c = arr["part_nodes"][node_off[q]:node_off[q + 1]].tolist()
            print(len(c), c[:10])                           # the reference prints this line (:262)
        pairs = arr["pairs"][pair_off[q]:pair_off[q + 1]]
        parts.append((arr["part_rids"][rid_off[q]:rid_off[q + 1]].tolist(), list(zip(pairs[:, 0].tolist(), pairs[:, 1].tolist()))))
    return parts


def _partition_reads_host_tail(tints, maximum_ilp_size, ctx, verbose):
    uniq = [unique_structures(t) for t in tints]
    packed = pack_structures(uniq)
    adj, _ = ctx.compat_graph(packed, prune=True)
    for t, tint in enumerate(tints):
        tint["partitions"] = _partitions_from_graph(uniq[t], adjacency_matrix(adj, packed, t), maximum_ilp_size, verbose)


def partition_reads_batch(tints, maximum_ilp_size, ctx, verbose=True, ilp_settings=None):
    """partition_reads() of several tints with one device call; sets tint['partitions'] on each.  A batch whose pair list the
    library refuses as too large for one call goes tint by tint.  Tints without 'ilp_data' (straight from read_segment()) are
    preprocessed by the same call (cluster_arrays_batch) and left as preprocess_ilp(tint, ilp_settings) leaves them; ilp_settings
    defaults to the constant recycle model."""
    if os.environ.get("FCLU_HOST_PARTITIONS", "0") == "1":
        return _partition_reads_host_tail(tints, maximum_ilp_size, ctx, verbose)
    fresh = [t for t in tints if "ilp_data" not in t]
    if fresh and len(fresh) != len(tints):                               # a mixed batch: each kind its own way
        done = [t for t in tints if "ilp_data" in t]
        partition_reads_batch(fresh, maximum_ilp_size, ctx, verbose, ilp_settings)
        return partition_reads_batch(done, maximum_ilp_size, ctx, verbose, ilp_settings)
    try:
        if fresh:
            packed, prep, arr = cluster_arrays_batch(tints, maximum_ilp_size, ctx)
            _ilp_data_from_prep(tints, packed, prep, ilp_settings or dict(recycle_model="constant"))
        else:
            arr = partition_arrays_batch(tints, maximum_ilp_size, ctx)
    except ClusterError as e:
        if e.code != ERR_UNSUPPORTED or len(tints) < 2:
            raise
        for tint in tints:
            partition_reads_batch([tint], maximum_ilp_size, ctx, verbose, ilp_settings)
        return
    for t, tint in enumerate(tints):
        tint["partitions"] = _partitions_from_arrays(arr, t, verbose)


def partition_reads(tint, maximum_ilp_size, ctx=None, verbose=True):
    """Reference-shaped entry (:196): tint['partitions'] = [(rep ids, [(incompatible rep pair), ...]), ...]."""
    own = ctx is None
    ctx = ctx or Context(0)
    try:
        partition_reads_batch([tint], maximum_ilp_size, ctx, verbose)
    finally:
        if own:
            ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# segment_*.tsv in, arrays out: the native reader (include/freddie_host.h, fhost_read_segment) and the rep grouping on the device
# ---------------------------------------------------------------------------------------------------------------
class _HostSegments(ctypes.Structure):
    _fields_ = [("owner", ctypes.c_void_p), ("n_file", ctypes.c_int32), ("n_tint", ctypes.c_int32), ("n_read", ctypes.c_int64)] + [
        (name, ctypes.c_void_p) for name in ("file_declined", "file_line", "file_reason", "file_map", "file_tint_off", "tint_id", "tint_file",
                                             "tint_chr_off", "tint_chr_len", "n_seg", "pos_off", "pos", "read_off", "lab_off", "rid", "strand",
                                             "name_off", "name_len", "chr_off", "chr_len", "labels", "tail", "gap_off", "gaps", "clip_off",
                                             "clips", "poly_off", "polys", "tok_off", "tok")]


_CLIP_KEYS = ("SSC", "ESC")
_POLY_KEYS = ("SA", "ST", "EA", "ET")
# (name, dtype, what it is counted by, columns): the arrays of a batch; offsets are listed with what they index
_PER_TINT = (("tint_id", np.int64), ("n_seg", np.int32))
_PER_READ = (("rid", np.int64), ("strand", np.uint8), ("tail", np.uint8))
_CSR = (("pos_off", "pos", np.int64, 1, "tint"), ("read_off", None, None, 0, "tint"), ("lab_off", "labels", np.uint32, 1, "tint"),
        ("gap_off", "gaps", np.int32, 3, "read"), ("clip_off", "clips", np.int32, 2, "read"), ("poly_off", "polys", np.int32, 3, "read"),
        ("tok_off", "tok", np.uint32, 1, "read"))


def _view(ptr, n, dtype):
    dtype = np.dtype(dtype)
    if n == 0 or not ptr:
        return np.zeros(0, dtype)
    return np.frombuffer((ctypes.c_char * (int(n) * dtype.itemsize)).from_address(ptr), dtype, int(n))


def _ints(values, dtype, cols=1):
    """An integer array of the given dtype; a wider one (in the end Python objects) for the numbers of a file the reader declined."""
    for dt in (dtype, np.int64, object):
        try:
            a = np.array(values, dt)
            if dt is object or a.size == 0 or (a.astype(object) == np.array(values, object)).all():
                return a.reshape(-1, cols) if cols > 1 else a.reshape(-1)
        except OverflowError:
            pass


def _pack_codes(codes):
    """uint8 label codes [rows, 16 * LW] -> uint32 words, two bits a label (pack_labels()' packing): four labels a byte, the first
    in the low bits; words little-endian."""
    q = codes.reshape(codes.shape[0], -1, 4)
    by = q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)
    return np.ascontiguousarray(by).view("<u4").astype(np.uint32, copy=False).reshape(-1)


def _chunk_from_tints(tints):
    """The arrays of one file from the mirror's dicts (a file the reader declined).  Its token streams are the mirror's own rep
    numbers, one token a read: the grouping they give is the mirror's, whatever made the reader decline (a leading zero or a
    repeated key is in the mirror's rep key as written, not in its dicts)."""
    a = dict(n_tint=len(tints), tint_chr=[t["chr"] for t in tints], read_name=[], read_chr=[])
    a["tint_id"] = _ints([t["id"] for t in tints], np.int64)
    a["n_seg"] = np.array([len(t["segs"]) for t in tints], np.int32)
    pos, pos_off, read_off, lab_off, labels = [], [0], [0], [0], []
    rid, strand, tail, gaps, clips, polys, tok = [], [], [], [], [], [], []
    gap_off, clip_off, poly_off = [0], [0], [0]
    for t in tints:
        if t["segs"]:
            pos.extend([t["segs"][0][0]] + [s[1] for s in t["segs"]])
        pos_off.append(len(pos))
        reads, M = t["reads"], len(t["segs"])
        LW = max((M + 15) // 16, 1)
        rep_of = {r: i for i, members in enumerate(t["read_reps"]) for r in members}
        codes = np.zeros((len(reads), LW * 16), np.uint8)
        for i, r in enumerate(reads):
            codes[i, :M] = r["data"]
            rid.append(r["id"]); strand.append(ord(r["strand"]))
            a["read_name"].append(r["name"]); a["read_chr"].append(r["chr"])
            pt = r["poly_tail"]
            cat = 0
            if len(pt) == 1:
                (key, (length, _)), = pt.items()
                if length > 10:
                    cat = 1 if key in ("SA", "ST") else 2
            tail.append(cat)
            gaps.extend([k[0], k[1], v] for k, v in r["gaps"].items()); gap_off.append(len(gaps))
            clips.extend([_CLIP_KEYS.index(k), v] for k, v in r["softclip"].items()); clip_off.append(len(clips))
            polys.extend([_POLY_KEYS.index(k), v[0], v[1]] for k, v in pt.items()); poly_off.append(len(polys))
            tok.append(rep_of[i])
        labels.append(_pack_codes(codes))
        read_off.append(len(rid)); lab_off.append(lab_off[-1] + len(reads) * LW)
    a.update(pos=_ints(pos, np.int64), pos_off=np.array(pos_off, np.int64), read_off=np.array(read_off, np.int64),
             lab_off=np.array(lab_off, np.int64), labels=np.concatenate(labels) if labels else np.zeros(0, np.uint32),
             rid=_ints(rid, np.int64), strand=np.array(strand, np.uint8), tail=np.array(tail, np.uint8),
             gap_off=np.array(gap_off, np.int64), gaps=_ints(gaps, np.int32, 3), clip_off=np.array(clip_off, np.int64),
             clips=_ints(clips, np.int32, 2), poly_off=np.array(poly_off, np.int64), polys=_ints(polys, np.int32, 3),
             tok_off=np.arange(len(rid) + 1, dtype=np.int64), tok=np.array(tok, np.uint32))
    return a


def _slice_chunk(a, t0, t1):
    """Tints t0 .. t1 of a batch's arrays as a batch of their own (copies)."""
    r0, r1 = int(a["read_off"][t0]), int(a["read_off"][t1])
    out = dict(n_tint=t1 - t0, tint_chr=a["tint_chr"][t0:t1], read_name=a["read_name"][r0:r1], read_chr=a["read_chr"][r0:r1])
    for name, _ in _PER_TINT:
        out[name] = a[name][t0:t1].copy()
    for name, _ in _PER_READ:
        out[name] = a[name][r0:r1].copy()
    for off, data, _, _, by in _CSR:
        i0, i1 = (t0, t1) if by == "tint" else (r0, r1)
        o = a[off][i0:i1 + 1]
        out[off] = o - o[0]
        if data:
            out[data] = a[data][int(o[0]):int(o[-1])].copy()
    return out


def _concat_chunks(chunks):
    out = dict(n_tint=sum(c["n_tint"] for c in chunks))
    for name in ("tint_chr", "read_name", "read_chr"):
        out[name] = [x for c in chunks for x in c[name]]
    for name, dt in _PER_TINT + _PER_READ:
        out[name] = np.concatenate([c[name] for c in chunks]) if chunks else np.zeros(0, dt)
    for off, data, dt, cols, _ in _CSR:
        offs, base = [np.zeros(1, np.int64)], 0
        for c in chunks:
            offs.append(c[off][1:] + base)
            base += int(c[off][-1])
        out[off] = np.concatenate(offs)
        if data:
            empty = np.zeros((0, cols) if cols > 1 else 0, dt)
            out[data] = np.concatenate([c[data] for c in chunks] or [empty])
    return out


class SegmentArrays:
    """A batch of segment_*.tsv files as flat arrays (include/freddie_host.h, fhost_segments): ``a`` maps the header's names to numpy
    arrays -- views of the native result, valid until close(), when no file was declined; copies otherwise, the declined files'
    parts made from the mirror's read_segment() (mirror=False: left out).  gaps / clips / polys have a row an entry.  file_tint_off: the tints of file f;
    declined: [(path, line, reason)].  Tint contigs, read names and read contigs (views into the mapped files): strings()."""

    def __init__(self, paths, threads=1, mirror=True):
        from . import _host
        self._L = _host.load()
        self.paths = [str(p) for p in paths]
        self._s = _HostSegments()
        self._strings = None
        self.declined = []
        if not self.paths:
            self.a = _concat_chunks([])
            self.file_tint_off = np.zeros(1, np.int64)
            return
        rc = self._L.fhost_read_segment(_host._c_strings(self.paths), len(self.paths), int(threads), ctypes.byref(self._s))
        if rc != 0:
            raise ClusterError("fhost_read_segment: out of memory or bad arguments (%d)" % rc)
        s, F, T, N = self._s, len(self.paths), self._s.n_tint, int(self._s.n_read)
        a = dict(n_tint=T)
        for name, dt in _PER_TINT:
            a[name] = _view(getattr(s, name), T, dt)
        for name, dt in _PER_READ:
            a[name] = _view(getattr(s, name), N, dt)
        for off, data, dt, cols, by in _CSR:
            a[off] = _view(getattr(s, off), (T if by == "tint" else N) + 1, np.int64)
            if data:
                x = _view(getattr(s, data), int(a[off][-1]) * cols, dt)
                a[data] = x.reshape(-1, cols) if cols > 1 else x
        self.a = a
        self.file_tint_off = _view(s.file_tint_off, F + 1, np.int64)
        declined = _view(s.file_declined, F, np.int32)
        if declined.any():
            lines = _view(s.file_line, F, np.int64).tolist()
            reasons = ctypes.cast(s.file_reason, ctypes.POINTER(ctypes.c_char_p))
            self.declined = [(self.paths[f], lines[f], reasons[f].decode()) for f in np.flatnonzero(declined).tolist()]
            if mirror:
                self._mix_in_the_mirror(declined)

    def _native_strings(self):
        s, T, N = self._s, self._s.n_tint, int(self._s.n_read)
        maps = _view(s.file_map, len(self.paths), np.uint64).tolist()
        tfile = _view(s.tint_file, T, np.int32).tolist()
        at = ctypes.string_at
        tint_chr = [at(maps[f] + o, n).decode() for f, o, n in zip(tfile, _view(s.tint_chr_off, T, np.int64).tolist(), _view(s.tint_chr_len, T, np.int32).tolist())]
        base = np.repeat(np.array([maps[f] for f in tfile], np.uint64), np.diff(_view(s.read_off, T + 1, np.int64))).tolist() if T else []
        name = [at(b + o, n).decode() for b, o, n in zip(base, _view(s.name_off, N, np.int64).tolist(), _view(s.name_len, N, np.int32).tolist())]
        chrom = [at(b + o, n).decode() for b, o, n in zip(base, _view(s.chr_off, N, np.int64).tolist(), _view(s.chr_len, N, np.int32).tolist())]
        return tint_chr, name, chrom

    def _mix_in_the_mirror(self, declined):
        """The declined files go through read_segment() (which raises what it always raised on a malformed one)."""
        native = dict(self.a)
        native["tint_chr"], native["read_name"], native["read_chr"] = self._native_strings()
        chunks = []
        for f, path in enumerate(self.paths):
            if declined[f]:
                chunks.append(_chunk_from_tints(list(read_segment(path).values())))
            else:
                chunks.append(_slice_chunk(native, int(self.file_tint_off[f]), int(self.file_tint_off[f + 1])))
        self.a = _concat_chunks(chunks)
        self._strings = (self.a.pop("tint_chr"), self.a.pop("read_name"), self.a.pop("read_chr"))
        self.file_tint_off = np.concatenate([[0], np.cumsum([c["n_tint"] for c in chunks])]).astype(np.int64)
        self.close()

    def strings(self):
        """(tint contigs, read names, read contigs) as lists of str."""
        if self._strings is None:
            self._strings = self._native_strings()
        return self._strings

    def close(self):
        if getattr(self, "_s", None) is not None and self._s.owner:
            self._L.fhost_segments_free(ctypes.byref(self._s))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def read_segment_arrays(paths, threads=1, mirror=True):
    """segment_*.tsv files as a SegmentArrays: parsed natively on `threads` threads, no per-read Python; a file the reader declines
    goes through read_segment().  mirror=False: the native result alone -- a declined file has no tints in the arrays and is only
    listed in .declined (path, line, reason)."""
    return SegmentArrays(paths, threads, mirror)


def arrays_from_segmentation(host_batch, results, annotation):
    """The SegmentArrays read_segment_arrays() would make of the segment TSVs of a batch, built in memory from the segmentation
    stage: host_batch = the loaded _host.HostBatch, results = (part_final_off, final_pos, label_off, labels2) of
    Context.results(packed=True), annotation = the arrays of _lib.Context.annotate().  Context.partition_segment, tints_from_arrays,
    round_gaps and cluster.cluster_tints take it unchanged.
    A read's gaps come in ascending j1 (a TSV line has them in string order).  Nothing downstream depends on that order: the rep
    grouping compares the key tokens of reads with equal label rows, and equal rows have equal j1 lists in either order."""
    pfo, fp, lo, l2 = (np.asarray(results[0], np.int64), np.asarray(results[1], np.int32), np.asarray(results[2], np.int64),
                       np.asarray(results[3], np.uint8))
    ra = host_batch.read_arrays()
    tint_id, tint_chr, read_name, read_chr = host_batch.names()
    T, N = len(pfo) - 1, len(ra["read_part"])
    read_off = np.zeros(T + 1, np.int64)
    np.cumsum(np.bincount(ra["read_part"], minlength=T), out=read_off[1:])
    n_seg = np.maximum(np.diff(pfo) - 1, 0).astype(np.int32)
    lab_off, labels = np.zeros(T + 1, np.int64), []
    for t in range(T):
        M, n_r = int(n_seg[t]), int(read_off[t + 1] - read_off[t])
        LW = max((M + 15) // 16, 1)
        g = np.arange(int(lo[t]), int(lo[t + 1]), dtype=np.int64)
        rows = ((l2[g >> 2] >> (2 * (g & 3)).astype(np.uint8)) & 3).reshape(-1, M) if M else np.zeros((0, 0), np.uint8)
        codes = np.zeros((n_r, LW * 16), np.uint8)
        if M and n_r:
            codes[:, :M] = rows[ra["read_rep"][read_off[t]:read_off[t + 1]]]
        labels.append(_pack_codes(codes))
        lab_off[t + 1] = lab_off[t] + n_r * LW
    a = dict(n_tint=T, tint_id=tint_id, n_seg=n_seg, pos_off=pfo.copy(), pos=fp[:int(pfo[-1])].astype(np.int64), read_off=read_off,
             lab_off=lab_off, labels=np.concatenate(labels) if labels else np.zeros(0, np.uint32), rid=ra["read_id"].copy(),
             strand=ra["strand"].copy(), tail=np.array(annotation["tail"], np.uint8))
    for off, data, dt, cols in (("gap_off", "gaps", np.int32, 3), ("clip_off", "clips", np.int32, 2), ("poly_off", "polys", np.int32, 3),
                                ("tok_off", "tok", np.uint32, 1)):
        a[off] = np.array(annotation[off], np.int64)
        x = np.array(annotation[data], dt)
        a[data] = x.reshape(-1, cols) if cols > 1 else x.reshape(-1)
    if len(a["tail"]) != N or len(a["gap_off"]) != N + 1:
        raise ClusterError("arrays_from_segmentation: the annotation is not of this batch's reads")
    out = SegmentArrays.__new__(SegmentArrays)
    out._L, out._s, out.paths, out.declined = None, None, [], []
    out.a = a
    out.file_tint_off = np.arange(T + 1, dtype=np.int64)          # (a partition is what a segment TSV holds)
    out._strings = (tint_chr, read_name, read_chr)
    return out


def cluster_files_batch(paths, maximum_ilp_size, ctx, ilp_settings=None, threads=8):
    """segment_*.tsv files in, (read_segment_arrays(), Context.group_reads() arrays, Context.preprocess() arrays of the reps,
    Context.partition() arrays) out: the native reader and one device call.  With ilp_settings the groups carry garbage_cost per rep
    (the constant model; the reference's other two models raise, :314-316)."""
    arrays = read_segment_arrays(paths, threads)
    groups, prep, arr = ctx.partition_segment(arrays, maximum_ilp_size)
    if ilp_settings is not None:
        counts = np.diff(groups["rep_mem_off"])
        if ilp_settings["recycle_model"] == "constant":
            groups["garbage_cost"] = counts * 3
        elif ilp_settings["recycle_model"] in ("exons", "introns"):
            garbage_cost_exons(I=[])                                     # a list: raises like the reference (:314, :316)
    return arrays, groups, prep, arr


def tints_from_arrays(arrays, groups, prep=None, arr=None, ilp_settings=None):
    """The tint dicts of a batch, in batch order, exactly as read_segment() leaves them; with prep / arr (Context.partition_segment)
    as preprocess_ilp(tint, ilp_settings) + partition_reads() leave them.  The in-process seam to code that wants dicts."""
    a = arrays.a
    tint_chr, read_name, read_chr = arrays.strings()
    T = a["n_tint"]
    tid, n_seg, pos, pos_off = a["tint_id"].tolist(), a["n_seg"].tolist(), a["pos"].tolist(), a["pos_off"].tolist()
    read_off, lab_off = a["read_off"].tolist(), a["lab_off"].tolist()
    rid, strand = a["rid"].tolist(), a["strand"].tolist()
    gap_off, clip_off, poly_off = a["gap_off"].tolist(), a["clip_off"].tolist(), a["poly_off"].tolist()
    gaps, clips, polys = a["gaps"].tolist(), a["clips"].tolist(), a["polys"].tolist()
    rep_off, mem_off, mem = groups["rep_off"].tolist(), groups["rep_mem_off"].tolist(), groups["rep_mem"].tolist()
    tints = []
    for t in range(T):
        p = pos[pos_off[t]:pos_off[t + 1]]
        r0, r1, M = read_off[t], read_off[t + 1], n_seg[t]
        LW = max((M + 15) // 16, 1)
        words = np.ascontiguousarray(a["labels"][lab_off[t]:lab_off[t + 1]], np.uint32).reshape(r1 - r0, LW)
        data = ((words[:, :, None] >> (2 * np.arange(16, dtype=np.uint32))[None, None, :]) & 3).reshape(r1 - r0, LW * 16)[:, :M].tolist()
        reads = []
        for i, r in enumerate(range(r0, r1)):
            reads.append(dict(id=rid[r], name=read_name[r], chr=read_chr[r], strand=chr(strand[r]), tint=tid[t], data=data[i],
                              gaps={(g[0], g[1]): g[2] for g in gaps[gap_off[r]:gap_off[r + 1]]},
                              softclip={_CLIP_KEYS[c[0]]: c[1] for c in clips[clip_off[r]:clip_off[r + 1]]},
                              poly_tail={_POLY_KEYS[q[0]]: (q[1], q[2]) for q in polys[poly_off[r]:poly_off[r + 1]]}))
        read_reps = [mem[mem_off[q]:mem_off[q + 1]] for q in range(rep_off[t], rep_off[t + 1])]
        tints.append(dict(id=tid[t], chr=tint_chr[t], segs=[(s, e, e - s) for s, e in zip(p[:-1], p[1:])], read_reps=read_reps, reads=reads))
    if prep is not None:
        first = groups["rep_first"].astype(np.int64) + np.repeat(a["read_off"][:-1], np.diff(groups["rep_off"]))
        packed = dict(rep_off=groups["rep_off"], n_seg=a["n_seg"], tail=a["tail"][first])
        _ilp_data_from_prep(tints, packed, prep, ilp_settings or dict(recycle_model="constant"))
    if arr is not None:
        for t, tint in enumerate(tints):
            tint["partitions"] = _partitions_from_arrays(arr, t, False)
    return tints
