#!/usr/bin/env python3
"""Measurement of row N3 (clustering pre-ILP graph work) on MI355X: pairwise compatibility + pruning of a batch of
synthetic preprocessed tints through include/freddie_cluster.h.

    python bench.py --full --workload cluster-many|cluster-big [--steps K] [--no-cpu-baseline]     (with the CPU baseline)
    python tools/cluster_bench.py [--workload many|big] [--steps K]                          (GPU side only)
    python tools/cluster_bench.py --partitions [--workload many|big] [--steps K] [--host-sample N]
                       (the whole of partition_reads() behind the dedupe on the device against the host tail it replaces)
    python tools/cluster_bench.py --front [--workload many|big] [--steps K]
                       (label rows in: the host front preprocess_ilp + unique_structures + pack_structures + pack_members, then
                        Context.partition, against the one call Context.partition_labels; the new kernels' event times)
    python tools/cluster_bench.py --files [--workload many|big] [--steps K] [--baseline-steps K] [--threads N]
                       (segment_*.tsv files in: the native reader, the rep grouping and the whole cluster_files_batch, against
                        read_segment + pack_labels + Context.partition_labels on the same files)
    python tools/cluster_bench.py --incumbents [--workload many|big] [--steps K] [--host-sample N] [--solve-budget S] [--max-seeds N] [--out FILE]
    python tools/cluster_bench.py --exact [--max-ilp K] [--exact-small N] [--exact-masks M] [--steps K] [--host-sample N] [--solve-budget S] [--out FILE]
                       (per problem size N = 8, 12, 16, 20, 24: Context.round_exact on every partition's first N reps -- the call, the kernels,
                        the longest launch, masks per second -- against HiGHS on a sample of the same problems; profiles/cluster_exact.txt)
    python tools/cluster_bench.py --wide [--sizes 128,256,1000] [--tints 40] [--wide-node-caps A,B] [--wide-passes A,B] [--loop-runs R] [--steps K] [--host-sample N] [--out FILE] [--append]
                       (per maximum_ilp_size: Context.round_bnb_wide on the first round's problems of 65 .. min(N, 1024) columns by column class --
                        taken, proven, unproven, nodes, ms a call, the longest launch --, HiGHS on a sample of the same problems, and optionally
                        the whole loop with and without --exact-wide; profiles/cluster_bnb_wide.txt)
    python tools/cluster_bench.py --bnb [--exact-bnb N] [--bnb-nodes M] [--bnb-depth D] [--bnb-node-cap C] [--steps K] [--host-sample N] [--solve-budget S] [--out FILE]
                       (per maximum_ilp_size N = 32, 48, 64: Context.round_bnb on the first round's problems of 25 .. N columns -- taken, proved,
                        capped, nodes, the call, the longest launch, nodes per second -- against HiGHS with 1 and 16 workers on a sample of
                        the same problems, and the weak bound's node count from the mirror; profiles/cluster_bnb.txt)
    python tools/cluster_bench.py --rounds [--workload many|big] [--steps K] [--host-sample N] [--solve-budget S] [--out FILE]
                       (the first round of every partition: Context.round_models against the plain-Python build of the same arrays as
                        the reference does it, the kernels' event times, and -- apart -- what HiGHS takes on the same round; the
                        result also goes to profiles/cluster_rounds.txt)

    python tools/cluster_bench.py --device-rounds [--sizes 24,64,1000] [--runs K] [--threads N] [--max-rounds R] [--tints N] [--out FILE] [--append]
                       (per maximum_ilp_size: the whole cluster_tints loop under --exact-small 24 --exact-bnb 64 with N solver workers, with
                        device_rounds off and on in turn, K runs each: wall time in total and per round, bytes copied to numpy, round_model()
                        builds, solver jobs, the read-out's kernel time, and whether both settings left the same tints;
                        profiles/cluster_device_rounds.txt)

One JSON line: read pairs tested per second of the CALL (packed host arrays in -> pruned adjacency in host memory: copies,
kernels and the pruning loop's host round trips all inside), the kernel times as detail, and the bound of the compatibility
kernel.  That kernel works on bit rows staged in LDS, so bytes do not describe it (a byte roofline credited it with more
than the bus can move); its bound is integer VALU work: per pair and 32-segment word of the pair's overlap 2 logic ops +
2 popcounts + 2 adds (py/freddie_cluster.py:229,232 as bit rows), against 256 CUs x 64 lanes x 2.4 GHz lane-ops/s.  The CPU baseline (the oracle's Python
restatement on a bounded sample of the same tints) is bench.py's leg: this file never touches oracle/.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cluster_util as cu  # noqa: E402
from freddie_amd import cluster_prep  # noqa: E402

WORKLOADS = {"many": dict(n_tints=400, n_reps=500, n_segs=300), "big": dict(n_tints=1, n_reps=20000, n_segs=2000)}


def overlap_words(packed):
    """sum over unordered pairs with a non-empty overlap [max f, min l] of the 32-segment words that overlap spans."""
    total = 0
    for t in range(packed["n_tint"]):
        a, b = int(packed["row_off"][t]), int(packed["row_off"][t + 1])
        f = packed["first"][a:b].astype(np.int64); l = packed["last"][a:b].astype(np.int64)
        for i0 in range(0, b - a, 2048):
            lo = np.maximum(f[i0:i0 + 2048, None], f[None, :]); hi = np.minimum(l[i0:i0 + 2048, None], l[None, :])
            w = (hi >> 5) - (lo >> 5) + 1
            total += int(w[(hi >= lo) & (lo >= 0)].sum())
        own = (l >> 5) - (f >> 5) + 1
        total -= int(own[(l >= f) & (f >= 0)].sum())              # the diagonal
    return total // 2


def run(workload="many", steps=5, cpu_baseline=None):
    """Returns the result dict.  cpu_baseline: a callable(unique structures per tint) -> dict supplied by bench.py (the
    only place besides the tests that may use the oracle), or None."""
    w = WORKLOADS[workload]
    tints = [cu.random_tint(1000 + t, w["n_reps"], w["n_segs"], n_isoforms=8) for t in range(w["n_tints"])]
    uniq = [cluster_prep.unique_structures(t) for t in tints]
    packed = cluster_prep.pack_structures(uniq)
    n_pairs = sum(len(u) * (len(u) - 1) // 2 for u in uniq)
    words = overlap_words(packed)
    ctx = cluster_prep.Context(0)
    ctx.compat_graph(packed)                                     # warm-up
    compat, prune, wall = [], [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        adj, rounds = ctx.compat_graph(packed)
        wall.append(time.perf_counter() - t0)
        tm = ctx.last_timing()
        compat.append(tm["compat_ms"]); prune.append(tm["prune_ms"])
    ctx.close()
    compat_ms, prune_ms = float(np.mean(compat)), float(np.mean(prune))
    wall_ms = float(np.median(wall)) * 1e3
    lane_ops = 6 * words
    peak = 256 * 64 * 2.4                                          # G lane-ops/s
    out = {
        "metric": "read pairs tested/sec (compatibility graph + pruning, whole call: host arrays in, adjacency out)",
        "value": n_pairs / (wall_ms * 1e-3),
        "unit": "pairs/s", "n_gpus": 1, "steps": steps, "higher_is_better": True, "dtype": "u32", "data": "synthetic",
        "config": {"workload": "cluster-" + workload, **w, "unique_reads": int(packed["row_off"][-1]),
                   "pairs": n_pairs, "prune_passes_max": int(rounds.max())},
        "call_wall_ms": wall_ms, "kernel_ms": {"compat": compat_ms, "prune": prune_ms},
        "value_kernels_only": n_pairs / ((compat_ms + prune_ms) * 1e-3),
        "roofline": {"kernel": "k_compat", "bound": "valu (integer: and / xor / popcount over bit rows in LDS)",
                     "achieved": lane_ops / (compat_ms * 1e-3) / 1e9, "peak": peak, "unit": "G lane-op/s",
                     "frac": lane_ops / (compat_ms * 1e-3) / 1e9 / peak, "traffic": None,
                     "algorithmic_lane_ops_per_launch": lane_ops, "overlap_words": words},
    }
    if cpu_baseline is not None:
        out["cpu_baseline"] = cpu_baseline(uniq)
    return out


def run_partitions(workload="many", steps=5, maximum_ilp_size=1000, host_sample=20):
    """Context.partition() of the workload (graph, components, even split, members, incompatible pairs: packed arrays in,
    flat arrays out) and, on the first host_sample tints, partition_reads_batch() both ways: the device path and, through
    FCLU_HOST_PARTITIONS=1, the host tail behind the same device graph (adjacency_matrix + scipy components + the Python pair
    loop).  Both of those end in tint['partitions'] as Python lists, so they share the cost of building the lists."""
    w = WORKLOADS[workload]
    tints = [cu.random_tint(1000 + t, w["n_reps"], w["n_segs"], n_isoforms=8) for t in range(w["n_tints"])]
    uniq = [cluster_prep.unique_structures(t) for t in tints]
    packed, members = cluster_prep.pack_structures(uniq), cluster_prep.pack_members(uniq)
    ctx = cluster_prep.Context(0)
    arr = ctx.partition(packed, members, maximum_ilp_size)       # warm-up
    comp, pairs, graph, wall = [], [], [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        arr = ctx.partition(packed, members, maximum_ilp_size)
        wall.append(time.perf_counter() - t0)
        tm, tg = ctx.partition_timing(), ctx.last_timing()
        comp.append(tm["components_ms"]); pairs.append(tm["pairs_ms"]); graph.append(tg["compat_ms"] + tg["prune_ms"])
    sample = tints[:host_sample]

    def reads_batch(host):
        if host:
            os.environ["FCLU_HOST_PARTITIONS"] = "1"
        else:
            os.environ.pop("FCLU_HOST_PARTITIONS", None)
        try:
            t0 = time.perf_counter()
            cluster_prep.partition_reads_batch(sample, maximum_ilp_size, ctx, verbose=False)
            dt = time.perf_counter() - t0
        finally:
            os.environ.pop("FCLU_HOST_PARTITIONS", None)
        return dt, [t["partitions"] for t in sample]

    reads_batch(False)                                           # warm-up of the sample's shapes
    dev_s, dev_parts = reads_batch(False)
    host_s, host_parts = reads_batch(True)
    t0 = time.perf_counter()
    ctx.partition(cluster_prep.pack_structures(uniq[:host_sample]), cluster_prep.pack_members(uniq[:host_sample]), maximum_ilp_size)
    arrays_sample_s = time.perf_counter() - t0
    ctx.close()
    return {
        "metric": "partition_reads() behind the dedupe: device arrays against the host tail", "unit": "ms", "data": "synthetic",
        "config": {"workload": "cluster-" + workload, **w, "maximum_ilp_size": maximum_ilp_size, "steps": steps,
                   "unique_reads": int(packed["row_off"][-1]), "partitions": int(arr["tint_part_off"][-1]), "incompatible_pairs": int(len(arr["pairs"]))},
        "whole_batch": {"partition_call_wall_ms": float(np.median(wall)) * 1e3,
                        "kernel_ms": {"graph (compat + prune)": float(np.mean(graph)), "components": float(np.mean(comp)),
                                      "pairs (count + emit + members)": float(np.mean(pairs))}},
        "sample": {"tints": len(sample), "identical_partitions": dev_parts == host_parts,
                   "partition_call_wall_ms": arrays_sample_s * 1e3,
                   "partition_reads_batch_device_ms": dev_s * 1e3, "partition_reads_batch_host_tail_ms": host_s * 1e3},
    }


def run_front(workload="many", steps=5, maximum_ilp_size=1000, dup=0.1):
    """The workload rebuilt as label rows (tests/front_util.labels_from_preprocessed: label = I, a fifth of the zeros written as 2,
    a share `dup` of the reps copies of earlier reps), then three things timed on the same tints:
      host front   preprocess_ilp + unique_structures + pack_structures + pack_members, as they stand (pure Python), on deep copies;
      present path host front + Context.partition;
      one call     pack_labels + Context.partition_labels (and the call alone, and its kernels' event times).
    Every timed region ends in a finished device call or is host work; medians over `steps` after one warm-up."""
    import copy
    import front_util as fu
    w = WORKLOADS[workload]
    base = [cu.random_tint(1000 + t, w["n_reps"], w["n_segs"], n_isoforms=8) for t in range(w["n_tints"])]
    tints = [fu.labels_from_preprocessed(b, seed=b["id"], twos=0.2, dup=dup) for b in base]
    del base
    ctx = cluster_prep.Context(0)
    settings = dict(recycle_model="constant")

    def host_front():
        work = copy.deepcopy(tints)
        t0 = time.perf_counter()
        for t in work:
            cluster_prep.preprocess_ilp(t, settings)
        t1 = time.perf_counter()
        uniq = [cluster_prep.unique_structures(t) for t in work]
        t2 = time.perf_counter()
        packed, members = cluster_prep.pack_structures(uniq), cluster_prep.pack_members(uniq)
        t3 = time.perf_counter()
        return (packed, members), dict(preprocess_ilp=t1 - t0, unique_structures=t2 - t1, pack=t3 - t2, total=t3 - t0)

    (packed, members), _ = host_front()
    labels = cluster_prep.pack_labels(tints)
    want = ctx.partition(packed, members, maximum_ilp_size)                    # warm-up of both paths, and the results compared
    prep, got = ctx.partition_labels(labels, maximum_ilp_size)
    same = all(np.array_equal(want[k], got[k]) for k in want) and np.array_equal(prep["bits"], packed["bits"]) and \
        np.array_equal(prep["mem"], members["mem"]) and np.array_equal(prep["mem_off"], members["mem_off"])
    front, part, pack_l, call, rows, dedupe = [], [], [], [], [], []
    for _ in range(steps):                                                     # the two paths alternate
        (packed, members), hf = host_front()
        front.append(hf)
        t0 = time.perf_counter()
        ctx.partition(packed, members, maximum_ilp_size)
        part.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        labels = cluster_prep.pack_labels(tints)
        t1 = time.perf_counter()
        ctx.partition_labels(labels, maximum_ilp_size)
        t2 = time.perf_counter()
        pack_l.append(t1 - t0); call.append(t2 - t1)
        tm = ctx.preprocess_timing()
        rows.append(tm["rows_ms"]); dedupe.append(tm["dedupe_ms"])
    ctx.close()
    med = lambda xs: float(np.median(xs)) * 1e3
    n_reps, n_rows = int(prep["n_reps"]), int(prep["n_rows"])
    host_ms = {k: med([f[k] for f in front]) for k in front[0]}
    present, one_call = host_ms["total"] + med(part), med(pack_l) + med(call)
    return {
        "metric": "the front of partition_reads(): host front + Context.partition against one Context.partition_labels call", "unit": "ms",
        "data": "synthetic", "config": {"workload": "cluster-" + workload, **w, "maximum_ilp_size": maximum_ilp_size, "steps": steps,
                                         "reps": n_reps, "unique_rows": n_rows, "share_of_reps_collapsed": 1.0 - n_rows / max(n_reps, 1),
                                         "duplicates_drawn": dup, "label_2_share_of_zeros": 0.2},
        "identical_results": bool(same),
        "host_front_ms": host_ms, "partition_call_ms": med(part), "present_path_ms": present,
        "pack_labels_ms": med(pack_l), "partition_labels_call_ms": med(call), "one_call_path_ms": one_call,
        "kernel_ms": {"rows (k_rows)": float(np.median(rows)), "dedupe (sorts, scans, k_leader, k_nodes, k_mem_off)": float(np.median(dedupe))},
        "one_call_not_slower": bool(one_call <= present), "call_alone_not_slower": bool(med(call) <= host_ms["total"] + med(part)),
        "spread_ms": {"present_path": [min(f["total"] + p for f, p in zip(front, part)) * 1e3, max(f["total"] + p for f, p in zip(front, part)) * 1e3],
                      "one_call_path": [min(a + b for a, b in zip(pack_l, call)) * 1e3, max(a + b for a, b in zip(pack_l, call)) * 1e3]},
    }


def write_segment_files(workload, directory, seed=7, gaps=True):
    """The workload as segment_<contig>_<tint>.tsv files, a tint a file: rows are noisy sub-ranges of a few isoform patterns (as
    cluster_util.random_tint draws them), a fifth of the zeros written as 2, every structure written as one to three reads whose 2s
    and small gaps differ (so they share a rep), one internal gap a read and a poly tail on a quarter of them.  gaps=False: the same
    reads without gaps and tails (the random draws are the same), for a loop that must reach its end: with them some first-round problem
    has a gap that ends on an uninformative segment, where the reference asserts and the loop raises."""
    w = WORKLOADS[workload]
    M, n = w["n_segs"], w["n_reps"]
    rng = np.random.default_rng(seed)
    header_pos = ",".join(str(100 + 50 * j) for j in range(M + 1))
    paths, n_reads = [], 0
    for t in range(w["n_tints"]):
        iso = rng.random((8, M)) < 0.6
        a = rng.integers(0, M, n); b = rng.integers(a, M)
        col = np.arange(M)[None, :]
        rows = (iso[rng.integers(0, 8, n)] ^ (rng.random((n, M)) < 0.03)) & (col >= a[:, None]) & (col <= b[:, None])
        copies = rng.integers(1, 4, n)
        g1 = rng.integers(0, M - 1, n); l1 = rng.choice([4, 9, 15, 60], n)
        poly = rng.integers(0, 16, n)
        lines = ["#ctg%d\t%d\t%s\n" % (t % 7, t, header_pos)]
        rid = 0
        for c in range(3):
            idx = np.flatnonzero(copies > c)
            text = np.where(rows[idx], 49, np.where(rng.random((len(idx), M)) < 0.2, 50, 48)).astype(np.uint8)
            small = rng.integers(0, 11, len(idx))
            for k, i in enumerate(idx.tolist()):
                gap_text = "%d-%d:%d," % (g1[i], g1[i] + 1, l1[i] if l1[i] > 10 else small[k])
                if poly[i] < 4:
                    gap_text += "%s_%d:%d," % (("SA", "ST", "EA", "ET")[poly[i]], 8 + 3 * (i % 5), (i % 3) * 9)
                lines.append("%d\tread%d_%d\tctg%d\t%s\t%d\t%s\t%s\n" % (rid, i, c, t % 7, "+-"[i & 1], t, text[k].tobytes().decode(), gap_text if gaps else ""))
                rid += 1
        n_reads += rid
        path = os.path.join(directory, "segment_ctg%d_%d.tsv" % (t % 7, t))
        with open(path, "w") as f:
            f.write("".join(lines))
        paths.append(path)
    return paths, n_reads


def run_files(workload="many", steps=5, baseline_steps=1, maximum_ilp_size=1000, threads=16):
    """segment_*.tsv files of the workload in a temporary directory, then on the same files, medians after one warm-up:
      native read   read_segment_arrays;  group  Context.group_reads (with fclu_group_timing's kernel times);
      whole         cluster_files_batch: reader + one device call, arrays out;
      baseline      the path without them: read_segment + pack_labels (with tail_categories) + Context.partition_labels."""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        paths, n_reads = write_segment_files(workload, d)
        n_bytes = sum(os.path.getsize(p) for p in paths)
        ctx = cluster_prep.Context(0)
        arrays, groups, prep, arr = cluster_prep.cluster_files_batch(paths, maximum_ilp_size, ctx, threads=threads)      # warm-up
        read, group, whole, keys, dedupe = [], [], [], [], []
        for _ in range(steps):
            t0 = time.perf_counter()
            a = cluster_prep.read_segment_arrays(paths, threads)
            t1 = time.perf_counter()
            ctx.group_reads(a)
            t2 = time.perf_counter()
            tm = ctx.group_timing()
            a.close()
            t3 = time.perf_counter()
            cluster_prep.cluster_files_batch(paths, maximum_ilp_size, ctx, threads=threads)[0].close()
            t4 = time.perf_counter()
            read.append(t1 - t0); group.append(t2 - t1); whole.append(t4 - t3); keys.append(tm["keys_ms"]); dedupe.append(tm["dedupe_ms"])
        base, same = [], True
        for _ in range(baseline_steps):
            t0 = time.perf_counter()
            tints = [t for p in paths for t in cluster_prep.read_segment(p).values()]
            t1 = time.perf_counter()
            packed = cluster_prep.pack_labels(tints)
            t2 = time.perf_counter()
            prep0, arr0 = ctx.partition_labels(packed, maximum_ilp_size)
            t3 = time.perf_counter()
            base.append(dict(read_segment=t1 - t0, pack_labels=t2 - t1, partition_labels=t3 - t2, total=t3 - t0))
            same = same and all(np.array_equal(prep0[k], prep[k]) for k in prep0) and all(np.array_equal(arr0[k], arr[k]) for k in arr0)
            del tints
        ctx.close()
        declined = len(arrays.declined)
        arrays.close()
    med = lambda xs: float(np.median(xs)) * 1e3
    base_ms = {k: med([b[k] for b in base]) for k in base[0]} if base else None
    return {
        "metric": "segment TSVs in, partitions out: native reader + one device call against read_segment + pack_labels + partition_labels",
        "unit": "ms", "data": "synthetic",
        "config": {"workload": "cluster-" + workload, **WORKLOADS[workload], "files": len(paths), "bytes": n_bytes, "reads": n_reads,
                   "reps": int(groups["n_reps"]), "unique_rows": int(prep["n_rows"]), "maximum_ilp_size": maximum_ilp_size, "steps": steps,
                   "baseline_steps": baseline_steps, "threads": threads, "files_declined": declined},
        "native_read_ms": med(read), "group_reads_call_ms": med(group),
        "kernel_ms": {"keys (k_gkeys)": float(np.median(keys)), "dedupe (sorts, scans, k_gleader, k_greps, k_mem_off)": float(np.median(dedupe))},
        "cluster_files_batch_ms": med(whole), "baseline_ms": base_ms,
        "identical_results": bool(same) if base else None,
        "whole_path_faster_than_baseline": bool(med(whole) < base_ms["total"]) if base else None,
        "spread_ms": {"native_read": [min(read) * 1e3, max(read) * 1e3], "cluster_files_batch": [min(whole) * 1e3, max(whole) * 1e3]},
    }


def python_round(tint, remaining_rids, incomp_rids):
    """The arrays of one problem in plain Python, as the reference gets at them inside run_ilp(): informative_segs() (:331-344, with its
    early break), the transposes the model loops walk (:429-439, :519-535), the pair filter with `in` on the LIST remaining_rids
    (:500-502), the gap keys and their segments (:462-481)."""
    M = len(tint["segs"])
    I, C = tint["ilp_data"]["I"], tint["ilp_data"]["C"]
    seg_content = [set() for _ in range(M)]
    informative = [True for _ in range(M)]
    for j in range(M):
        for i in remaining_rids:
            seg_content[j].add(I[i][j])
            if seg_content[j] == {0, 1}:
                break
    for j in range(1, M - 1):
        if len(seg_content[j]) == 1 and (seg_content[j - 1] == seg_content[j] == seg_content[j + 1]):
            informative[j] = False
    support = [[c for c, i in enumerate(remaining_rids) if I[i][j] == 1] for j in range(M) if informative[j]]
    corrections = [[j for j in range(M) if informative[j] and C[i][j] > 0] for i in remaining_rids]
    pairs = [(i1, i2) for (i1, i2) in incomp_rids if i1 in remaining_rids and i2 in remaining_rids]
    groups = dict()
    for i in remaining_rids:
        for (j1, j2), l in tint["reads"][tint["read_reps"][i][0]]["gaps"].items():
            if (j1, j2) not in groups:
                groups[(j1, j2)] = [(j, tint["segs"][j][2]) for j in range(j1 + 1, j2) if informative[j]]
    return informative, support, corrections, pairs, groups


def run_rounds(workload="many", steps=5, host_sample=4, solve_budget=120.0, maximum_ilp_size=1000, threads=16):
    """The workload's segment_*.tsv files staged as the stage does (cluster.stage_files), then the FIRST round, every partition active:
      device    Context.round_models on all problems (medians over `steps` after a warm-up; fclu_round_timing's kernel split), and on
                the problems of the first `host_sample` tints alone;
      baseline  python_round() on those same `host_sample` tints' problems (the pair filter is quadratic: a sample, not the batch);
      solve     apart from both: cluster_solve.solve_round (HiGHS) on the sample's problems, smallest first, until `solve_budget`
                seconds are spent -- the model build is not the solve."""
    import tempfile
    from freddie_amd import cluster, cluster_solve
    with tempfile.TemporaryDirectory() as d:
        paths, n_reads = write_segment_files(workload, d)
        ctx = cluster_prep.Context(0)
        settings = cluster.ilp_settings(max_ilp=maximum_ilp_size)
        t0 = time.perf_counter()
        tints, part0, _ = cluster.stage_files(paths, settings, ctx, threads)
        stage_s = time.perf_counter() - t0
    problems = [(t, q, list(rids)) for t, tint in enumerate(tints) for q, (rids, _) in enumerate(tint["partitions"])]
    sample = [p for p in problems if p[0] < host_sample]
    call = lambda ps: ctx.round_models([part0[t] + q for t, q, _ in ps], [rem for _, _, rem in ps])
    arr = call(problems)                                                          # warm-up
    all_s, kern, sample_s = [], [], []
    for _ in range(steps):
        t0 = time.perf_counter(); arr = call(problems); all_s.append(time.perf_counter() - t0)
        kern.append(ctx.round_timing())
        t0 = time.perf_counter(); sarr = call(sample); sample_s.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    py = [python_round(tints[t], rem, tints[t]["partitions"][q][1]) for t, q, rem in sample]
    python_s = time.perf_counter() - t0
    same = True
    for p, (informative, support, corrections, pairs, groups) in enumerate(py):
        m = cluster_prep.round_model(sarr, p)
        if m is None:                                                             # (a problem the reference asserts on, :467-468: no model)
            continue
        col = {rid: c for c, rid in enumerate(sample[p][2])}
        same = same and m["inf_seg"] == [j for j, v in enumerate(informative) if v] and m["support"] == support and \
            m["corrections"] == corrections and m["pairs"] == [(col[a], col[b]) for a, b in pairs] and m["groups"] == sorted(groups) and \
            m["group_segs"] == [groups[k] for k in sorted(groups)]
    solved, spent, statuses = [], 0.0, {}
    order = sorted(range(len(sample)), key=lambda p: len(sample[p][2]))
    for p in order:
        if spent >= solve_budget:
            break
        t, q, rem = sample[p]
        model = cluster_prep.round_model(sarr, p)
        if model is None:
            continue
        costs = cluster.garbage_costs(tints[t], "constant")
        model["garbage"] = [costs[i] for i in rem]; model["max_lg"] = sum(s[2] for s in tints[t]["segs"])
        t0 = time.perf_counter()
        status = cluster_solve.solve_round(model, settings)[0]
        dt = time.perf_counter() - t0
        spent += dt
        solved.append((len(rem), dt)); statuses[status] = statuses.get(status, 0) + 1
        print("solved %d reps in %.2f s: %s" % (len(rem), dt, status), file=sys.stderr, flush=True)
    ctx.close()
    med = lambda xs: float(np.median(xs)) * 1e3
    return {
        "metric": "first round of every partition: Context.round_models against the plain-Python build of the same arrays", "unit": "ms",
        "data": "synthetic",
        "config": {"workload": "cluster-" + workload, **WORKLOADS[workload], "reads": n_reads, "reps": sum(len(t["read_reps"]) for t in tints),
                   "problems": len(problems), "columns": int(arr["n_cols"]), "pairs_kept": int(arr["n_pairs"]), "support_entries": int(arr["n_sup"]),
                   "correction_terms": int(arr["n_corr"]), "gap_rows": int(arr["n_gap_rows"]), "gap_groups": int(arr["n_grp"]),
                   "refused_problems": int((arr["refused"] >= 0).sum()), "maximum_ilp_size": maximum_ilp_size, "steps": steps,
                   "host_sample_tints": host_sample, "sample_problems": len(sample), "sample_refused": int((sarr["refused"] >= 0).sum()), "sample_columns": int(sarr["n_cols"])},
        "stage_files_s": stage_s,
        "round_models_call_ms": med(all_s), "kernel_ms": {k: float(np.median([x[k] for x in kern])) for k in kern[0]},
        "sample_round_models_call_ms": med(sample_s), "sample_python_ms": python_s * 1e3, "identical_results": bool(same),
        "sample_python_over_device": python_s / max(float(np.median(sample_s)), 1e-9),
        "highs": {"problems_solved": len(solved), "of_sample_problems": len(sample), "seconds": spent, "statuses": statuses,
                  "largest_solved_reps": max([n for n, _ in solved] or [0]), "slowest_s": max([x for _, x in solved] or [0.0])},
        "spread_ms": {"round_models_call": [min(all_s) * 1e3, max(all_s) * 1e3]},
    }


def run_incumbents(workload="many", steps=5, host_sample=2, solve_budget=300.0, maximum_ilp_size=1000, threads=16, max_seeds=64):
    """The workload staged as run_rounds() stages it, then the FIRST round, every partition active:
      device   Context.round_models then Context.round_incumbents on all problems (medians over `steps` after a warm-up; the kernel
               splits of fclu_round_timing and fclu_round_incumbent_timing side by side), and the share of problems with a model whose
               incumbent is not empty;
      solve    on the solvable problems of the first `host_sample` tints (run_rounds()' sample), smallest first, until `solve_budget`
               seconds are spent: HiGHS without and with the incumbent as a cutoff, and incumbent cost / HiGHS optimum.
    What was not taken is None."""
    import tempfile
    from freddie_amd import cluster, cluster_solve
    with tempfile.TemporaryDirectory() as d:
        paths, n_reads = write_segment_files(workload, d)
        ctx = cluster_prep.Context(0)
        settings = cluster.ilp_settings(max_ilp=maximum_ilp_size)
        tints, part0, _ = cluster.stage_files(paths, settings, ctx, threads)
    costs = [cluster.garbage_costs(t, "constant") for t in tints]
    problems = [(t, q, list(rids)) for t, tint in enumerate(tints) for q, (rids, _) in enumerate(tint["partitions"])]
    sample = [p for p in problems if p[0] < host_sample]

    def call(ps):
        t0 = time.perf_counter()
        arr = ctx.round_models([part0[t] + q for t, q, _ in ps], [rem for _, _, rem in ps])
        t1 = time.perf_counter()
        inc = ctx.round_incumbents([costs[t][i] for t, _, rem in ps for i in rem], settings["epsilon"], settings["offset"], max_seeds)
        return arr, inc, t1 - t0, time.perf_counter() - t1

    call(problems)                                                                # warm-up
    models_s, inc_s, kern_models, kern_inc = [], [], [], []
    for _ in range(steps):
        arr, inc, a, b = call(problems)
        models_s.append(a); inc_s.append(b)
        kern_models.append(ctx.round_timing()); kern_inc.append(ctx.round_incumbent_timing())
    with_model = int((arr["refused"] < 0).sum())
    no_start = int(((inc["cost2"] < 0) & (arr["refused"] < 0)).sum())
    sizes = np.diff(inc["mem_off"])
    nonempty = int((sizes > 0).sum())
    sarr, sinc, _, _ = call(sample)
    rows, spent = [], 0.0
    for p in sorted(range(len(sample)), key=lambda p: len(sample[p][2])):
        t, q, rem = sample[p]
        model = cluster_prep.round_model(sarr, p)
        if model is None or spent >= solve_budget:
            continue
        model["garbage"] = [costs[t][i] for i in rem]; model["max_lg"] = sum(s[2] for s in tints[t]["segs"])
        incumbent = cluster_prep.round_incumbent(sinc, p)
        row = {"reps": len(rem), "incumbent_cost": incumbent[0] if incumbent else None, "incumbent_members": int(sum(incumbent[1])) if incumbent else None}
        for name, with_cutoff in (("plain", False), ("cutoff", True)):
            m = dict(model)
            if with_cutoff and incumbent is not None:
                m["incumbent"] = incumbent
            t0 = time.perf_counter()
            status, x, e = cluster_solve.solve_round(m, settings)
            dt = time.perf_counter() - t0
            spent += dt
            row[name + "_s"], row[name + "_status"] = dt, status
            row[name + "_cost"] = cluster_solve.round_cost(model, x, e) if status == cluster_solve.OPTIMAL else None
            print("%s: %d reps in %.2f s: %s" % (name, len(rem), dt, status), file=sys.stderr, flush=True)
        row["incumbent_over_optimum"] = incumbent[0] / row["plain_cost"] if incumbent and row["plain_cost"] else None
        rows.append(row)
    ctx.close()
    med = lambda xs: float(np.median(xs)) * 1e3
    kmed = lambda ks: {k: float(np.median([x[k] for x in ks])) for k in ks[0]}
    return {
        "metric": "first round of every partition: Context.round_incumbents behind Context.round_models; HiGHS with and without the cutoff on the sample",
        "unit": "ms", "data": "synthetic", "source_hash": _build_hash(),
        "config": {"workload": "cluster-" + workload, **WORKLOADS[workload], "reads": n_reads, "problems": len(problems), "columns": int(arr["n_cols"]),
                   "pairs_kept": int(arr["n_pairs"]), "gap_rows": int(arr["n_gap_rows"]), "refused_problems": len(problems) - with_model,
                   "max_seeds": max_seeds, "steps": steps, "host_sample_tints": host_sample, "sample_problems": len(sample), "solve_budget_s": solve_budget},
        "round_models_call_ms": med(models_s), "round_models_kernel_ms": kmed(kern_models),
        "round_incumbents_call_ms": med(inc_s), "round_incumbents_kernel_ms": kmed(kern_inc),
        "round_incumbents_kernel_ms_total": float(np.median([sum(k.values()) for k in kern_inc])),
        "round_models_kernel_ms_total": float(np.median([sum(k.values()) for k in kern_models])),
        "problems_with_a_model": with_model, "without_a_feasible_start": no_start, "incumbent_not_empty": nonempty,
        "share_not_empty": nonempty / with_model if with_model else None,
        "mean_members_over_columns": float(sizes.sum()) / max(int(np.diff(arr["col_off"])[arr["refused"] < 0].sum()), 1),
        "sample": rows or None, "sample_solve_seconds": spent,
        "spread_ms": {"round_incumbents_call": [min(inc_s) * 1e3, max(inc_s) * 1e3]},
    }


EXACT_LAUNCH_MASKS = 1 << 24     # kExactLaunchMasks of freddie_amd/csrc/freddie_cluster.hip: the masks one search launch evaluates at the most


def run_exact(workload="many", steps=3, maximum_ilp_size=24, sizes=(8, 12, 16, 20, 24), max_masks=1 << 30, host_sample=24, solve_budget=120.0, threads=16):
    """The workload staged with a small maximum_ilp_size (thousands of small partitions with incompatible pairs), then per N of `sizes`
    the round whose problems are every partition's first N reps (a later round's shape: at most N columns, most of them exactly N):
      models   Context.round_models on these problems (median call time: what a round costs today on the device);
      exact    Context.round_exact with max_cols = N and the budget max_masks (medians over `steps` after a warm-up): the call, the
               kernels from fclu_round_exact_timing (prep, all search launches, the longest launch), problems taken, masks, launches,
               masks per second of the call and of the search kernels;
      HiGHS    cluster_solve.solve_round on `host_sample` of the taken problems, evenly spread, within solve_budget / len(sizes) seconds:
               the mean per problem, extrapolated to the taken problems, and whether the costs agree with the exact ones.
    What was not taken is None."""
    import tempfile
    from freddie_amd import cluster, cluster_solve
    with tempfile.TemporaryDirectory() as d:
        paths, n_reads = write_segment_files(workload, d)
        ctx = cluster_prep.Context(0)
        settings = cluster.ilp_settings(max_ilp=maximum_ilp_size)
        tints, part0, _ = cluster.stage_files(paths, settings, ctx, threads)
    costs = [cluster.garbage_costs(t, "constant") for t in tints]
    med = lambda xs: float(np.median(xs))
    rows = []
    for N in sizes:
        problems = [(t, q, list(rids)[:N]) for t, tint in enumerate(tints) for q, (rids, _) in enumerate(tint["partitions"])]
        garbage = [costs[t][i] for t, _, rem in problems for i in rem]
        models_s = []
        for _ in range(steps + 1):
            t0 = time.perf_counter()
            arr = ctx.round_models([part0[t] + q for t, q, _ in problems], [rem for _, _, rem in problems])
            models_s.append(time.perf_counter() - t0)
        models_kernel_ms = sum(ctx.round_timing().values())
        got = ctx.round_exact(garbage, settings["epsilon"], settings["offset"], N, max_masks)      # warm-up
        call_s, kern = [], []
        for _ in range(steps):
            t0 = time.perf_counter()
            got = ctx.round_exact(garbage, settings["epsilon"], settings["offset"], N, max_masks)
            call_s.append(time.perf_counter() - t0)
            kern.append(ctx.round_exact_timing())
        taken = np.flatnonzero(got["cost2"] != -2)
        row = {"N": N, "problems": len(problems), "with_a_model": int((arr["refused"] < 0).sum()), "columns": int(arr["n_cols"]), "pairs_kept": int(arr["n_pairs"]),
               "gap_rows": int(arr["n_gap_rows"]), "informative_segments": int(arr["n_inf"]),
               "round_models_call_ms": med(models_s[1:]) * 1e3, "round_models_kernel_ms": models_kernel_ms,
               "taken": got["n_taken"], "masks": got["n_masks"], "launches": got["n_launches"], "infeasible": int((got["cost2"] == -1).sum()),
               "round_exact_call_ms": med(call_s) * 1e3, "round_exact_call_spread_ms": [min(call_s) * 1e3, max(call_s) * 1e3],
               "kernel_ms": {k: med([x[k] for x in kern]) for k in kern[0]},
               "masks_per_s_call": got["n_masks"] / med(call_s),
               "masks_per_s_search_kernels": got["n_masks"] / max(med([x["search_ms"] for x in kern]) * 1e-3, 1e-9)}
        sample = taken[np.linspace(0, len(taken) - 1, min(host_sample, len(taken))).astype(int)].tolist() if len(taken) else []
        spent, solved, agree = 0.0, [], 0
        for p in sample:
            if spent >= solve_budget / len(sizes):
                break
            t, q, rem = problems[p]
            model = cluster_prep.round_model(arr, p)
            model["garbage"] = [costs[t][i] for i in rem]; model["max_lg"] = sum(s[2] for s in tints[t]["segs"])
            t0 = time.perf_counter()
            status, x, e = cluster_solve.solve_round(model, settings)
            dt = time.perf_counter() - t0
            spent += dt
            solved.append(dt)
            exact = cluster_prep.round_exact_solution(got, p)
            agree += (status != cluster_solve.OPTIMAL and exact == "infeasible") or \
                (status == cluster_solve.OPTIMAL and exact != "infeasible" and abs(cluster_solve.round_cost(model, x, e) - exact[0]) < 0.25)
        mean_s = float(np.mean(solved)) if solved else None
        row["highs"] = {"problems_solved": len(solved), "seconds": spent, "mean_s": mean_s, "slowest_s": max(solved or [0.0]), "costs_agree": int(agree),
                        "extrapolated_to_taken_s": mean_s * got["n_taken"] if solved else None,
                        "extrapolated_over_16_workers_s": mean_s * got["n_taken"] / 16 if solved else None}
        row["exact_call_faster_than_highs_on_the_taken"] = bool(med(call_s) < mean_s * got["n_taken"] / 16) if solved else None
        print("N = %d: %d taken, %d masks, call %.2f ms, longest launch %.2f ms; HiGHS mean %s s" %
              (N, got["n_taken"], got["n_masks"], row["round_exact_call_ms"], row["kernel_ms"]["longest_launch_ms"], mean_s), file=sys.stderr, flush=True)
        rows.append(row)
    ctx.close()
    return {
        "metric": "a round's small problems: Context.round_exact (enumeration on the device) against HiGHS (cluster_solve.solve_round) on a sample of the same problems",
        "unit": "ms", "data": "synthetic", "source_hash": _build_hash(),
        "config": {"workload": "cluster-" + workload, **WORKLOADS[workload], "reads": n_reads, "maximum_ilp_size": maximum_ilp_size, "max_masks": max_masks,
                   "steps": steps, "host_sample": host_sample, "solve_budget_s": solve_budget, "launch_bound_masks": EXACT_LAUNCH_MASKS,
                   "problems_of_N": "every partition's first N reps"},
        "longest_launch_ms": max(r["kernel_ms"]["longest_launch_ms"] for r in rows),
        "sizes": rows,
    }


BNB_LAUNCH_NODES = 1 << 24       # kBnbLaunchNodes of freddie_amd/csrc/freddie_cluster.hip: the task-nodes of budget one search launch holds


def _solve_timed(job):
    from freddie_amd import cluster_solve
    model, settings = job
    t0 = time.perf_counter()
    status, x, e = cluster_solve.solve_round(model, settings)
    return status, (cluster_solve.round_cost(model, x, e) if status == cluster_solve.OPTIMAL else None), time.perf_counter() - t0


def run_bnb(workload="many", steps=3, sizes=(32, 48, 64), min_cols=25, max_nodes=None, depth=None, node_cap=None, host_sample=16, solve_budget=240.0,
            weak_budget=90.0, threads=16):
    """Per N of `sizes` the workload is staged with maximum_ilp_size = N and the FIRST round of every partition is the batch:
      device   Context.round_models, Context.round_incumbents (the bounds) and Context.round_bnb with min_cols .. N columns (medians over
               `steps` after a warm-up): problems taken, proved (optimal or infeasible), unproven with and without a set, capped tasks,
               nodes, the call, the kernels of fclu_round_bnb_timing (tables, all search launches, the longest launch), nodes per second;
      sample   `host_sample` of the taken problems, evenly spread, as a round of their own: the three device calls timed together, then
               HiGHS (cluster_solve.solve_round) on the same problems with 1 worker, one after the other until solve_budget / len(sizes)
               seconds are spent, and on those it got through with 16 workers (wall time of a pool); the feature's path on them = the
               device calls + HiGHS with 16 workers on the unproven ones, each with the incumbent cluster_tints() would hand it;
      weak     the mirror (cluster_solve.bnb_task) with the weak bound on the sample's first problems, task by task, until weak_budget /
               len(sizes) seconds are spent: its nodes and capped tasks beside the device's on the same tasks.
    What was not taken is None."""
    import tempfile
    from multiprocessing import Pool
    from freddie_amd import cluster, cluster_solve
    depth = cluster_solve.BNB_DEPTH if depth is None else depth
    node_cap = cluster_solve.BNB_NODE_CAP if node_cap is None else node_cap
    max_nodes = cluster.BNB_NODES if max_nodes is None else max_nodes
    pool = Pool(16)                                              # before the device is opened: the workers never touch it
    med = lambda xs: float(np.median(xs))
    rows = []
    ctx = cluster_prep.Context(0)
    for N in sizes:
        with tempfile.TemporaryDirectory() as d:
            paths, n_reads = write_segment_files(workload, d)
            settings = cluster.ilp_settings(max_ilp=N)
            tints, part0, _ = cluster.stage_files(paths, settings, ctx, threads)
        costs = [cluster.garbage_costs(t, "constant") for t in tints]
        problems = [(t, q, list(rids)) for t, tint in enumerate(tints) for q, (rids, _) in enumerate(tint["partitions"])]

        def device(ps):
            t0 = time.perf_counter()
            arr = ctx.round_models([part0[t] + q for t, q, _ in ps], [rem for _, _, rem in ps])
            garbage = [costs[t][i] for t, _, rem in ps for i in rem]
            inc = ctx.round_incumbents(garbage, settings["epsilon"], settings["offset"])
            t1 = time.perf_counter()
            got = ctx.round_bnb(garbage, inc["cost2"], settings["epsilon"], settings["offset"], min_cols, N, max_nodes, depth, node_cap)
            return arr, inc, got, t1 - t0, time.perf_counter() - t1

        device(problems)                                                          # warm-up
        call_s, kern = [], []
        for _ in range(steps):
            arr, inc, got, _, b = device(problems)
            call_s.append(b)
            kern.append(ctx.round_bnb_timing())
        status = got["status"]
        taken = np.flatnonzero(status != -2)
        cols = np.diff(got["col_off"])
        row = {"N": N, "problems": len(problems), "with_a_model": int((arr["refused"] < 0).sum()), "of_min_cols_to_N_columns": int(((cols >= min_cols) & (cols <= N)).sum()),
               "informative_segments": int(arr["n_inf"]), "gap_rows": int(arr["n_gap_rows"]), "pairs_kept": int(arr["n_pairs"]),
               "taken": got["n_taken"], "taken_columns": [int(cols[taken].min()), int(cols[taken].max())] if len(taken) else None,
               "proved": int(((status == 0) | (status == 1)).sum()), "infeasible": int((status == 1).sum()),
               "unproven_with_a_set": int(((status == 2) & (got["cost2"] >= 0)).sum()), "unproven_without_a_set": int(((status == 2) & (got["cost2"] < 0)).sum()),
               "capped_tasks": int(got["capped"].sum()), "nodes": got["nodes_total"], "launches": got["n_launches"],
               "round_bnb_call_ms": med(call_s) * 1e3, "round_bnb_call_spread_ms": [min(call_s) * 1e3, max(call_s) * 1e3],
               "kernel_ms": {k: med([x[k] for x in kern]) for k in kern[0]},
               "nodes_per_s_call": got["nodes_total"] / med(call_s),
               "nodes_per_s_search_kernels": got["nodes_total"] / max(med([x["search_ms"] for x in kern]) * 1e-3, 1e-9)}
        pick = taken[np.linspace(0, len(taken) - 1, min(host_sample, len(taken))).astype(int)].tolist() if len(taken) else []
        sample = [problems[p] for p in pick]
        if sample:
            device(sample)
            sarr, sinc, sgot, a, b = device(sample)
            jobs, spent = [], 0.0
            for p, (t, q, rem) in enumerate(sample):
                model = cluster_prep.round_model(sarr, p)
                model["garbage"] = [costs[t][i] for i in rem]; model["max_lg"] = sum(s[2] for s in tints[t]["segs"])
                jobs.append(model)
            serial = []
            for model in jobs:                                                    # 1 worker
                if spent >= solve_budget / len(sizes):
                    break
                serial.append(_solve_timed((model, settings)))
                spent += serial[-1][2]
            done = len(serial)
            t0 = time.perf_counter()
            pool.map(_solve_timed, [(m, settings) for m in jobs[:done]], chunksize=1)
            pool16_s = time.perf_counter() - t0
            later, agree = [], 0
            for p in range(done):
                found = cluster_prep.round_bnb_solution(sgot, p)
                if found is not None and found != "infeasible" and found[0] != "unproven":
                    agree += serial[p][0] == cluster_solve.OPTIMAL and abs(serial[p][1] - found[0]) < 0.25
                elif found == "infeasible":
                    agree += serial[p][0] != cluster_solve.OPTIMAL
                else:
                    m = dict(jobs[p])
                    greedy = cluster_prep.round_incumbent(sinc, p)
                    if found is not None and found[1] is not None:
                        m["incumbent"] = tuple(found[1:]) if greedy is None or found[1] < greedy[0] else greedy
                    later.append((m, settings))
            t0 = time.perf_counter()
            if later:
                pool.map(_solve_timed, later, chunksize=1)
            later_s = time.perf_counter() - t0
            sstat = sgot["status"][:done]
            row["sample"] = {"problems": len(sample), "solved_by_highs": done, "columns": [len(rem) for _, _, rem in sample[:done]],
                             "models_and_incumbents_call_ms": a * 1e3, "round_bnb_call_ms": b * 1e3, "proved": int(((sstat == 0) | (sstat == 1)).sum()),
                             "unproven": int((sstat == 2).sum()), "nodes": int(sgot["nodes"][:done].sum()),
                             "highs_1_worker_s": spent, "highs_1_worker_slowest_s": max([x[2] for x in serial] or [0.0]), "highs_16_workers_s": pool16_s,
                             "highs_statuses": {s: sum(1 for x in serial if x[0] == s) for s in set(x[0] for x in serial)},
                             "proved_costs_agree_with_highs": int(agree), "later_solves_16_workers_s": later_s,
                             "bnb_path_s": b + later_s, "bnb_path_faster_than_16_workers": bool(b + later_s < pool16_s)}
            weak_nodes = weak_capped = strong_nodes = strong_capped = tasks = 0
            t0 = time.perf_counter()
            complete, out_of_time = 0, False
            for p in range(done):
                tb = cluster_solve.bnb_tables(jobs[p], settings)
                D = min(tb["R"], depth)
                ub2 = None if sinc["cost2"][p] < 0 else int(sinc["cost2"][p])
                for t in range(1 << D):
                    if time.perf_counter() - t0 > weak_budget / len(sizes):
                        out_of_time = True
                        break
                    w = cluster_solve.bnb_task(tb, t, D, ub2, node_cap, weak=True)
                    s = cluster_solve.bnb_task(tb, t, D, ub2, node_cap)
                    weak_nodes += w[2]; weak_capped += w[3]; strong_nodes += s[2]; strong_capped += s[3]; tasks += 1
                if out_of_time:
                    break
                complete += 1
            row["weak_bound_mirror"] = {"problems_complete": complete, "tasks": tasks, "weak_nodes": weak_nodes, "weak_capped_tasks": weak_capped,
                                        "full_bound_nodes_same_tasks": strong_nodes, "full_bound_capped_tasks": strong_capped}
        print("N = %d: %d taken, %d proved, %d nodes, call %.2f ms, longest launch %.2f ms; sample %s" %
              (N, got["n_taken"], row["proved"], got["nodes_total"], row["round_bnb_call_ms"], row["kernel_ms"]["longest_launch_ms"], row.get("sample")),
              file=sys.stderr, flush=True)
        rows.append(row)
    ctx.close()
    pool.close()
    pool.join()
    return {
        "metric": "a round's problems of 25 to N columns: Context.round_bnb (branch and bound on the device) against HiGHS (cluster_solve.solve_round) on a sample of the same problems",
        "unit": "ms", "data": "synthetic", "source_hash": _build_hash(),
        "config": {"workload": "cluster-" + workload, **WORKLOADS[workload], "min_cols": min_cols, "max_nodes": max_nodes, "depth": depth, "node_cap": node_cap,
                   "steps": steps, "host_sample": host_sample, "solve_budget_s": solve_budget, "weak_budget_s": weak_budget, "launch_bound_task_nodes": BNB_LAUNCH_NODES,
                   "problems_of_N": "every partition's first round under maximum_ilp_size N"},
        "longest_launch_ms": max(r["kernel_ms"]["longest_launch_ms"] for r in rows),
        "sizes": rows,
    }


def _compare_rounds(base, wide):
    """Two loops' on_round records, keyed (tint, partition, round) -> (status, cost, remaining, x), partition by partition up to the first
    round in which they differ (behind it the remaining reps differ and the rounds are other problems): how many partitions agree to the
    end, and what the first difference is -- the same status and cost with another set (an optimum that is not unique), another cost, or
    another status -- with up to five examples of each of the last two."""
    parts = sorted(set(k[:2] for k in base) | set(k[:2] for k in wide))
    out = {"partitions": len(parts), "same_to_the_end": 0, "rounds_compared_equal": 0, "first_difference": {"same_cost_other_set": 0, "other_cost": 0, "other_status": 0,
                                                                                                             "one_loop_has_no_such_round": 0}, "examples": []}
    for part in parts:
        r = 0
        while True:
            a, b = base.get(part + (r,)), wide.get(part + (r,))
            if a is None and b is None:
                out["same_to_the_end"] += 1
                break
            if a is None or b is None:
                kind = "one_loop_has_no_such_round"
            elif a == b:
                out["rounds_compared_equal"] += 1
                r += 1
                continue
            elif a[0] != b[0]:
                kind = "other_status"
            elif a[1] != b[1]:
                kind = "other_cost"
            else:
                kind = "same_cost_other_set"
            out["first_difference"][kind] += 1
            if kind != "same_cost_other_set" and len(out["examples"]) < 10:
                out["examples"].append({"tint": part[0], "partition": part[1], "round": r, "columns": None if a is None else len(a[2]),
                                        "without": None if a is None else list(a[:2]), "with": None if b is None else list(b[:2])})
            break
    return out


WIDE_CLASSES = ((65, 128), (129, 256), (257, 512), (513, 1024))


def run_wide(workload="many", steps=3, sizes=(128, 256, 1000), n_tints=40, max_nodes=None, depth=None, node_caps=None, host_sample=32, threads=16,
             loop_runs=0, exact_cols=24, bnb_cols=64, passes_list=(1,)):
    """Per N of `sizes` the workload's first n_tints files, written without gaps, are staged with maximum_ilp_size = N and the FIRST round
    of every partition is the batch:
      device   Context.round_models, Context.round_incumbents (the bounds) and Context.round_bnb_wide with 65 .. min(N, 1024) columns, once
               per node cap of `node_caps` (default: cluster_solve.bnb_wide_node_cap(N); medians over `steps` after a warm-up): per column
               class 65-128, 129-256, 257-512, 513-1024 the problems of that size, those whose tables do not fit, taken, proven and unproven;
               nodes, capped tasks, the call, the kernels of fclu_round_bnb_wide_timing (tables, all search launches, the longest launch);
      solver   HiGHS (cluster_solve.solve_round) with `threads` workers on `host_sample` of the taken problems, evenly spread: wall time of
               the pool, and the share of them the search proved at the default cap;
      loop     loop_runs > 0: the whole cluster_tints() loop under exact_cols / bnb_cols with and without wide_cols = min(N, 1024), in turn,
               loop_runs times each: seconds, solver jobs, and whether tints and logs are the same.
      passes   passes_list (--wide-passes A,B,...): every node cap is run once per number of passes (Context.round_bnb_wide(passes=...)),
               with the rows of round_bnb_wide_pass_stats() -- a pass's tasks, nodes, capped tasks, launches, problems -- and the loop
               once per number of passes (wide_passes) beside the loop without wide_cols."""
    import hashlib
    import tempfile
    from multiprocessing import Pool
    from freddie_amd import cluster, cluster_solve
    depth = cluster_solve.BNB_DEPTH if depth is None else depth
    max_nodes = cluster.WIDE_NODES if max_nodes is None else max_nodes
    pool = Pool(threads)                                         # before the device is opened: the workers never touch it
    med = lambda xs: float(np.median(xs))
    rows = []
    ctx = cluster_prep.Context(0)
    with tempfile.TemporaryDirectory() as d:
        paths, n_reads = write_segment_files(workload, d, gaps=False)
        paths = paths[:n_tints] if n_tints else paths
        for N in sizes:
            top = min(N, cluster_solve.BNB_WIDE_MAX_COLS)
            settings = cluster.ilp_settings(max_ilp=N)
            tints, part0, _ = cluster.stage_files(paths, settings, ctx, threads)
            costs = [cluster.garbage_costs(t, "constant") for t in tints]
            problems = [(t, q, list(rids)) for t, tint in enumerate(tints) for q, (rids, _) in enumerate(tint["partitions"])]
            row = {"N": N, "problems": len(problems), "caps": []}
            for node_cap, passes in ((c, k) for c in (node_caps or (cluster_solve.bnb_wide_node_cap(top),)) for k in passes_list):
                def device(ps):
                    arr = ctx.round_models([part0[t] + q for t, q, _ in ps], [rem for _, _, rem in ps])
                    garbage = [costs[t][i] for t, _, rem in ps for i in rem]
                    inc = ctx.round_incumbents(garbage, settings["epsilon"], settings["offset"])
                    t1 = time.perf_counter()
                    got = ctx.round_bnb_wide(garbage, inc["cost2"], settings["epsilon"], settings["offset"], 65, top, max_nodes, depth, node_cap,
                                             **({"passes": passes} if passes > 1 else {}))
                    return arr, inc, got, time.perf_counter() - t1

                device(problems)                                                  # warm-up
                call_s, kern = [], []
                for _ in range(steps):
                    arr, inc, got, b = device(problems)
                    call_s.append(b)
                    kern.append(ctx.round_bnb_wide_timing())
                status, cols = got["status"], np.diff(got["col_off"])
                n_inf = np.diff(arr["inf_off"])
                fits = np.array([cluster_prep.bnb_wide_lds_bytes(int(r), int(e)) <= cluster_prep.BNB_WIDE_LDS_BYTES for r, e in zip(cols, n_inf)], bool)
                classes = {}
                for lo, hi in WIDE_CLASSES:
                    sel = (cols >= lo) & (cols <= hi) & (arr["refused"] < 0)
                    classes["%d-%d" % (lo, hi)] = {"problems": int(sel.sum()), "tables_do_not_fit": int((sel & ~fits).sum()), "taken": int((sel & (status != -2)).sum()),
                                                   "proven": int((sel & ((status == 0) | (status == 1))).sum()), "unproven": int((sel & (status == 2)).sum()),
                                                   "nodes": int(got["nodes"][sel].sum()), "capped_tasks": int(got["capped"][sel].sum()),
                                                   "informative_segments_range": [int(n_inf[sel].min()), int(n_inf[sel].max())] if sel.any() else None}
                row["caps"].append({"node_cap": node_cap, "depth": depth, "passes": passes, "pass_rows": ctx.round_bnb_wide_pass_stats(),
                                    "proven": int(((status == 0) | (status == 1)).sum()), "taken": got["n_taken"], "launches": got["n_launches"], "nodes": got["nodes_total"],
                                    "classes": classes, "round_bnb_wide_call_ms": med(call_s) * 1e3, "call_spread_ms": [min(call_s) * 1e3, max(call_s) * 1e3],
                                    "kernel_ms": {k: med([x[k] for x in kern]) for k in kern[0]}})
                print("N = %d cap %d passes %d: %s" % (N, node_cap, passes, json.dumps(row["caps"][-1])), file=sys.stderr, flush=True)
            taken = np.flatnonzero(status != -2)
            pick = taken[np.linspace(0, len(taken) - 1, min(host_sample, len(taken))).astype(int)].tolist() if len(taken) and host_sample else []
            if pick:
                jobs = []
                for p in pick:
                    t, q, rem = problems[p]
                    model = cluster_prep.round_model(arr, p)
                    model["garbage"] = [costs[t][i] for i in rem]; model["max_lg"] = sum(s[2] for s in tints[t]["segs"])
                    jobs.append((model, settings))
                t0 = time.perf_counter()
                solved = pool.map(_solve_timed, jobs, chunksize=1)
                row["solver"] = {"problems": len(pick), "columns": [int(cols[p]) for p in pick], "workers": threads, "wall_s": time.perf_counter() - t0,
                                 "solve_s_sum": sum(x[2] for x in solved), "solve_s_longest": max(x[2] for x in solved),
                                 "statuses": {k: sum(1 for x in solved if x[0] == k) for k in set(x[0] for x in solved)},
                                 "proven_by_the_search_at_the_last_cap": int(sum(1 for p in pick if status[p] in (0, 1)))}
                print("N = %d solver: %s" % (N, json.dumps(row["solver"])), file=sys.stderr, flush=True)
            del tints
            loops, records = [], {}
            for run_no in range(loop_runs):
                for wide_cols, passes in [(0, 1)] + [(top, k) for k in passes_list]:
                    ls = cluster.ilp_settings(max_ilp=N, exact_cols=exact_cols, bnb_cols=bnb_cols, wide_cols=wide_cols, wide_passes=passes)
                    tints, part0, _ = cluster.stage_files(paths, ls, ctx, threads)
                    jobs_n = [0]

                    class CountingPool:
                        def map(self, fn, items, chunksize=1):
                            jobs_n[0] += len(items)
                            return pool.map(fn, items, chunksize=chunksize)

                    record = {}
                    keep = lambda r: record.__setitem__((r["tint"]["id"], r["partition"], r["round"]),
                                                        (r["status"], r["cost"], tuple(r["remaining"]), None if r["x"] is None else tuple(r["x"])))
                    t0 = time.perf_counter()
                    logs = cluster.cluster_tints(tints, part0, ctx, ls, pool=CountingPool(), on_round=keep)
                    t1 = time.perf_counter()
                    digest = hashlib.sha256(repr([(t["id"], t["isoforms"], t["garbage_rids"]) for t in tints]).encode() + repr(logs).encode()).hexdigest()[:16]
                    loops.append({"wide_cols": wide_cols, "wide_passes": passes, "run": run_no, "loop_s": t1 - t0, "solver_jobs": jobs_n[0], "digest": digest,
                                  "rounds": len(record), "statuses": {k: sum(1 for v in record.values() if v[0] == k) for k in set(v[0] for v in record.values())}})
                    records[(run_no, wide_cols, passes)] = record
                    print("N = %d loop: %s" % (N, json.dumps(loops[-1])), file=sys.stderr, flush=True)
                    del tints
            if loops:
                row["loop"] = {"runs": loops, "same_tints_and_logs": len(set(r["digest"] for r in loops)) == 1,
                               "round_for_round": [_compare_rounds(records[(k, 0, 1)], records[(k, top, passes_list[-1])]) for k in range(loop_runs)]}
            rows.append(row)
    ctx.close()
    pool.close()
    pool.join()
    return {"metric": "a round's problems of 65 to min(N, 1024) columns: Context.round_bnb_wide against HiGHS on a sample of the same problems, and the whole loop",
            "unit": "ms", "data": "synthetic", "source_hash": _build_hash(),
            "config": {"workload": "cluster-" + workload, **WORKLOADS[workload], "files_taken": len(paths), "reads_written": n_reads, "gaps": "left out", "max_nodes": max_nodes,
                       "steps": steps, "host_sample": host_sample, "solver_workers": threads, "loop_runs": loop_runs, "exact_cols": exact_cols, "bnb_cols": bnb_cols},
            "sizes": rows}


class _RoundClock:
    """A context that notes when each round starts (its first round_models call) and what the read-out's kernels took."""

    def __init__(self, ctx, device):
        self.ctx, self.device, self.marks, self.readout_ms, self.calls, self.bytes = ctx, device, [], [], dict(models=0, readout=0), 0

    def __getattr__(self, name):
        return getattr(self.ctx, name)

    def round_models(self, parts, remaining, fetch=True):
        if not (self.device and fetch):
            self.marks.append(time.perf_counter())
            print("  round %d: %d problems" % (len(self.marks) - 1, len(parts)), file=sys.stderr, flush=True)
        self.calls["models"] += 1
        return self._count(self.ctx.round_models(parts, remaining, fetch) if self.device else self.ctx.round_models(parts, remaining))

    def _count(self, arrays):
        self.bytes += sum(a.nbytes for a in arrays.values() if isinstance(a, np.ndarray))
        return arrays

    def round_incumbents(self, *args, **kw):
        return self._count(self.ctx.round_incumbents(*args, **kw))

    def round_exact(self, *args, **kw):
        return self._count(self.ctx.round_exact(*args, **kw))

    def round_bnb(self, *args, **kw):
        return self._count(self.ctx.round_bnb(*args, **kw))

    def round_readout(self, sets):
        out = self._count(self.ctx.round_readout(sets))
        self.calls["readout"] += 1
        self.readout_ms.append(sum(self.ctx.round_readout_timing().values()))
        return out


def run_device_rounds(workload="many", sizes=(24, 64, 1000), runs=3, threads=16, max_rounds=30, exact_cols=24, bnb_cols=64, n_tints=None):
    """The workload's segment_*.tsv files staged afresh for every run (cluster.stage_files, timed apart), then the whole cluster_tints()
    loop to its end under exact_cols / bnb_cols with `threads` solver workers, device_rounds off and on in turn, `runs` times each.  The
    yardstick is the flag-off run: the same binary on the path the flag leaves alone.  n_tints: the workload's first so many files only."""
    import hashlib
    import tempfile
    from multiprocessing import Pool
    from freddie_amd import cluster
    pool = Pool(threads)                                      # before the GPU is opened: the workers never touch it
    rows = []
    try:
        with tempfile.TemporaryDirectory() as d:
            paths, n_reads = write_segment_files(workload, d, gaps=False)
            paths = paths[:n_tints] if n_tints else paths
            ctx = cluster_prep.Context(0)
            for size in sizes:
                per = {False: [], True: []}
                for run_no in range(runs):
                    for flag in (False, True):
                        settings = cluster.ilp_settings(max_ilp=size, max_rounds=max_rounds, exact_cols=exact_cols, bnb_cols=bnb_cols, device_rounds=flag)
                        t0 = time.perf_counter()
                        tints, part0, _ = cluster.stage_files(paths, settings, ctx, threads)
                        stage_s = time.perf_counter() - t0
                        clock, built, jobs = _RoundClock(ctx, flag), [0], [0]

                        def counting(arr, p):
                            built[0] += 1
                            return cluster_prep.round_model(arr, p)

                        class CountingPool:
                            def map(self, fn, items, chunksize=1):
                                jobs[0] += len(items)
                                return pool.map(fn, items, chunksize=chunksize)

                        t0 = time.perf_counter()
                        logs = cluster.cluster_tints(tints, part0, clock, settings, pool=CountingPool(), round_model=counting)
                        t1 = time.perf_counter()
                        marks = clock.marks + [t1]
                        digest = hashlib.sha256(repr([(t["id"], t["isoforms"], t["garbage_rids"]) for t in tints]).encode() + repr(logs).encode()).hexdigest()[:16]
                        per[flag].append(dict(total_s=t1 - t0, stage_files_s=stage_s, rounds=len(clock.marks), round_s=[b - a for a, b in zip(marks[:-1], marks[1:])],
                                              round_models_calls=clock.calls["models"], round_readout_calls=clock.calls["readout"],
                                              bytes_copied=clock.bytes, round_model_builds=built[0], solver_jobs=jobs[0],
                                              problem_rounds=sum(len(l) for l in logs), isoforms=sum(len(t["isoforms"]) for t in tints),
                                              readout_kernel_ms=float(sum(clock.readout_ms)), readout_kernel_ms_longest=max(clock.readout_ms or [0.0]),
                                              digest=digest))
                        print("max_ilp %d run %d device_rounds=%s: %.2f s, %d rounds, %d builds, %d solver jobs" %
                              (size, run_no, flag, t1 - t0, len(clock.marks), built[0], jobs[0]), file=sys.stderr, flush=True)
                        del tints
                summary = {}
                for flag in (False, True):
                    tot = [r["total_s"] for r in per[flag]]
                    summary["on" if flag else "off"] = dict(
                        total_s_median=float(np.median(tot)), total_s_range=[min(tot), max(tot)], runs=per[flag],
                        round_s_median=[float(np.median(x)) for x in zip(*[r["round_s"] for r in per[flag]])] if len(set(r["rounds"] for r in per[flag])) == 1 else None,
                        bytes_copied_per_round=float(np.median([r["bytes_copied"] / max(r["rounds"], 1) for r in per[flag]])))
                off, on = summary["off"], summary["on"]
                spread = max(off["total_s_range"][1] - off["total_s_range"][0], on["total_s_range"][1] - on["total_s_range"][0])
                rows.append(dict(maximum_ilp_size=size, off=off, on=on, saved_s=off["total_s_median"] - on["total_s_median"], run_to_run_range_s=spread,
                                 faster_by_more_than_the_range=bool(off["total_s_median"] - on["total_s_median"] > spread),
                                 same_tints_and_logs=bool(len(set(r["digest"] for f in (False, True) for r in per[f])) == 1)))
            ctx.close()
    finally:
        pool.close()
        pool.join()
    return {
        "metric": "the whole cluster_tints loop with device_rounds off (the yardstick: the unchanged path of the same binary) and on", "unit": "s",
        "data": "synthetic", "source_hash": _build_hash(),
        "config": {"workload": "cluster-" + workload, **WORKLOADS[workload], "files_taken": len(paths), "reads_written": n_reads, "exact_cols": exact_cols, "bnb_cols": bnb_cols, "solver_workers": threads,
                   "max_rounds": max_rounds, "runs": runs,
                   "gaps": "left out (write_segment_files(gaps=False)): with them the first round holds problems the reference asserts on, and the loop raises",
                   "order": "off, on, off, on, ...: every run stages the files afresh; the first run of a size grows the buffers"},
        "sizes": rows,
    }


def _build_hash():
    from freddie_amd import build as _b
    return _b.embedded_hash(cluster_prep.CLUSTER_SO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="many", choices=sorted(WORKLOADS))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--partitions", action="store_true", help="measure Context.partition() against the host tail (FCLU_HOST_PARTITIONS=1)")
    ap.add_argument("--host-sample", type=int, default=None, help="--partitions: tints the two partition_reads_batch() runs take (default 20; --rounds 4, --incumbents 2, --exact 24, "
                                                                  "--bnb 16, --wide 32)")
    ap.add_argument("--front", action="store_true", help="measure the host front + Context.partition against Context.partition_labels")
    ap.add_argument("--files", action="store_true", help="measure the native segment TSV reader + Context.partition_segment against read_segment + partition_labels")
    ap.add_argument("--baseline-steps", type=int, default=1, help="--files: runs of the Python baseline (it takes seconds a run)")
    ap.add_argument("--threads", type=int, default=16, help="--files: threads of the native reader")
    ap.add_argument("--rounds", action="store_true", help="measure Context.round_models on the first round against the plain-Python build; HiGHS apart")
    ap.add_argument("--solve-budget", type=float, default=120.0, help="--rounds: seconds of HiGHS solves on the sample's problems")
    ap.add_argument("--incumbents", action="store_true", help="measure Context.round_incumbents on the first round; HiGHS with and without the cutoff on the --rounds sample")
    ap.add_argument("--max-seeds", type=int, default=64, help="--incumbents: seeded starts a problem")
    ap.add_argument("--out", default=None, help="--rounds / --incumbents: where the result is written too (profiles/cluster_rounds.txt, profiles/cluster_incumbents.txt)")
    ap.add_argument("--exact", action="store_true", help="measure Context.round_exact per problem size against HiGHS on a sample of the same problems")
    ap.add_argument("--max-ilp", type=int, default=24, help="--exact: maximum_ilp_size the workload is staged with")
    ap.add_argument("--exact-small", type=int, default=None, help="--exact: one N instead of 8, 12, 16, 20, 24")
    ap.add_argument("--exact-masks", type=int, default=1 << 30, help="--exact: the mask budget of a call")
    ap.add_argument("--bnb", action="store_true", help="measure Context.round_bnb under maximum_ilp_size 32, 48 and 64 against HiGHS on a sample of the same problems")
    ap.add_argument("--exact-bnb", type=int, default=None, help="--bnb: one N instead of 32, 48, 64")
    ap.add_argument("--bnb-nodes", type=int, default=None, help="--bnb: the node budget of a call (default: cluster.BNB_NODES)")
    ap.add_argument("--bnb-depth", type=int, default=None, help="--bnb: columns the task number fixes (default: cluster_solve.BNB_DEPTH)")
    ap.add_argument("--bnb-node-cap", type=int, default=None, help="--bnb: nodes a task may count (default: cluster_solve.BNB_NODE_CAP)")
    ap.add_argument("--weak-budget", type=float, default=90.0, help="--bnb: seconds of the weak-bound mirror on the sample")
    ap.add_argument("--device-rounds", action="store_true", help="measure the whole cluster_tints loop with device_rounds off and on (profiles/cluster_device_rounds.txt)")
    ap.add_argument("--sizes", default=None, help="--device-rounds: the maximum_ilp_size values (default 24,64,1000; --wide: 128,256,1000)")
    ap.add_argument("--runs", type=int, default=3, help="--device-rounds: runs of each setting")
    ap.add_argument("--max-rounds", type=int, default=30, help="--device-rounds: the loop's max_rounds")
    ap.add_argument("--tints", type=int, default=None, help="--device-rounds: the workload's first N files only (default: all)")
    ap.add_argument("--append", action="store_true", help="--device-rounds: add the result to --out instead of replacing it (a size a call, each under its own time limit)")
    ap.add_argument("--wide", action="store_true", help="measure Context.round_bnb_wide under maximum_ilp_size 128, 256 and 1000 (--sizes) on the first --tints files "
                                                         "(default 40) against HiGHS on a sample of the same problems (profiles/cluster_bnb_wide.txt)")
    ap.add_argument("--wide-node-caps", default=None, help="--wide: node caps to run, comma separated (default: cluster_solve.bnb_wide_node_cap(N))")
    ap.add_argument("--wide-passes", default=None, help="--wide: numbers of passes to run every node cap (and the loop) with, comma separated (default: 1; "
                                                        "profiles/cluster_bnb_wide_passes.txt)")
    ap.add_argument("--loop-runs", type=int, default=0, help="--wide: runs of the whole loop with and without --exact-wide (default: none)")
    args = ap.parse_args()
    sample = lambda default: default if args.host_sample is None else args.host_sample
    if args.wide:
        args.sizes = args.sizes or "128,256,1000"
        sizes = tuple(int(v) for v in args.sizes.split(","))
        caps = tuple(int(v) for v in args.wide_node_caps.split(",")) if args.wide_node_caps else None
        passes = tuple(int(v) for v in args.wide_passes.split(",")) if args.wide_passes else (1,)
        res = run_wide(args.workload, args.steps, sizes, args.tints or 40, node_caps=caps, host_sample=sample(32),
                       threads=args.threads, loop_runs=args.loop_runs, passes_list=passes)
        default_out = "cluster_bnb_wide_passes.txt" if args.wide_passes else "cluster_bnb_wide.txt"
        with open(args.out or os.path.join(ROOT, "profiles", default_out), "a" if args.append else "w") as f:
            f.write("tools/cluster_bench.py --wide --workload %s --steps %d --sizes %s --wide-node-caps %s%s --loop-runs %d  (libfreddie_cluster.so source hash %s)\n" %
                    (args.workload, args.steps, ",".join(map(str, sizes)), args.wide_node_caps, " --wide-passes %s" % args.wide_passes if args.wide_passes else "",
                     args.loop_runs, res["source_hash"]))
            f.write(json.dumps(res, indent=1) + "\n")
        print(json.dumps(res))
    elif args.device_rounds:
        args.sizes = args.sizes or "24,64,1000"
        sizes = tuple(int(v) for v in args.sizes.split(","))
        res = run_device_rounds(args.workload, sizes, args.runs, args.threads, args.max_rounds, n_tints=args.tints)
        with open(args.out or os.path.join(ROOT, "profiles", "cluster_device_rounds.txt"), "a" if args.append else "w") as f:
            f.write("tools/cluster_bench.py --device-rounds --workload %s --sizes %s --runs %d --threads %d --max-rounds %d%s  (libfreddie_cluster.so source hash %s)\n" %
                    (args.workload, args.sizes, args.runs, args.threads, args.max_rounds, " --tints %d" % args.tints if args.tints else "", res["source_hash"]))
            f.write(json.dumps(res, indent=1) + "\n")
        print(json.dumps({k: v for k, v in res.items() if k != "sizes"}))
        for row in res["sizes"]:
            print(json.dumps({k: (v if not isinstance(v, dict) else {a: b for a, b in v.items() if a != "runs"}) for k, v in row.items()}))
    elif args.bnb:
        res = run_bnb(args.workload, args.steps, (args.exact_bnb,) if args.exact_bnb is not None else (32, 48, 64), max_nodes=args.bnb_nodes, depth=args.bnb_depth,
                      node_cap=args.bnb_node_cap, host_sample=sample(16),
                      solve_budget=args.solve_budget if args.solve_budget != 120.0 else 240.0, weak_budget=args.weak_budget, threads=args.threads)
        with open(args.out or os.path.join(ROOT, "profiles", "cluster_bnb.txt"), "w") as f:
            f.write("tools/cluster_bench.py --bnb --workload %s --steps %d  (libfreddie_cluster.so source hash %s)\n" % (args.workload, args.steps, res["source_hash"]))
            f.write(json.dumps(res, indent=1) + "\n")
        print(json.dumps(res))
    elif args.exact:
        res = run_exact(args.workload, args.steps, args.max_ilp, (args.exact_small,) if args.exact_small is not None else (8, 12, 16, 20, 24), args.exact_masks,
                        host_sample=sample(24), solve_budget=args.solve_budget, threads=args.threads)
        with open(args.out or os.path.join(ROOT, "profiles", "cluster_exact.txt"), "w") as f:
            f.write("tools/cluster_bench.py --exact --workload %s --steps %d --max-ilp %d --exact-masks %d  (libfreddie_cluster.so source hash %s)\n" %
                    (args.workload, args.steps, args.max_ilp, args.exact_masks, res["source_hash"]))
            f.write(json.dumps(res, indent=1) + "\n")
        print(json.dumps(res))
    elif args.incumbents:
        res = run_incumbents(args.workload, args.steps, host_sample=sample(2),
                             solve_budget=args.solve_budget if args.solve_budget != 120.0 else 300.0, threads=args.threads, max_seeds=args.max_seeds)
        with open(args.out or os.path.join(ROOT, "profiles", "cluster_incumbents.txt"), "w") as f:
            f.write("tools/cluster_bench.py --incumbents --workload %s --steps %d  (libfreddie_cluster.so source hash %s)\n" % (args.workload, args.steps, res["source_hash"]))
            f.write(json.dumps(res, indent=1) + "\n")
        print(json.dumps(res))
    elif args.rounds:
        res = run_rounds(args.workload, args.steps, host_sample=sample(4),
                         solve_budget=args.solve_budget, threads=args.threads)
        with open(args.out or os.path.join(ROOT, "profiles", "cluster_rounds.txt"), "w") as f:
            f.write("tools/cluster_bench.py --rounds --workload %s --steps %d\n" % (args.workload, args.steps))
            f.write(json.dumps(res, indent=1) + "\n")
        print(json.dumps(res))
    elif args.files:
        print(json.dumps(run_files(args.workload, args.steps, args.baseline_steps, threads=args.threads)))
    elif args.front:
        print(json.dumps(run_front(args.workload, args.steps)))
    elif args.partitions:
        print(json.dumps(run_partitions(args.workload, args.steps, host_sample=sample(20))))
    else:
        print(json.dumps(run(args.workload, args.steps)))


if __name__ == "__main__":
    main()
