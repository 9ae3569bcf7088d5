#!/usr/bin/env python3
"""Chromosome-wide case of the segmentation-visualisation library (freddie_amd/segment_vis.py, include/freddie_vis.h): the
reads of freddie_amd.synth's config4 (4000 partitions x 500 reads, about 2 M) placed side by side on one chromosome, about
20 000 synthetic Ensembl-style transcripts over the same span, and as segment boundaries every exon boundary of every
partition (the positions the segmentation stage recovers on these inputs).  Prints kernel ms, call ms (fvis_classify() with
its copies), the host's array building and dict building, and the share of the whole spent building dicts.

Usage: python tools/vis_bench.py [--partitions 4000] [--repeat 3]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from freddie_amd import segment_vis as sv, synth  # noqa: E402

STRIDE = 200_000                           # chromosome span of a partition (a synthetic partition spans < 100 kb)


def make_case(n_part, n_tx=20_000, seed=3):
    w = dict(synth.WORKLOADS["config4"])
    w.pop("n_partitions")
    reads, bounds = [], set()
    for p in range(n_part):
        g = synth.generate(p, with_seq=False, **w)
        off = p * STRIDE
        s = g.ex_ts.astype(np.int64) + off
        e = g.ex_te.astype(np.int64) + off
        bounds.update(s.tolist()); bounds.update(e.tolist())
        ro = g.read_exon_off
        sl, el = s.tolist(), e.tolist()
        for r in range(len(ro) - 1):
            reads.append(dict(intervals=list(zip(sl[ro[r]:ro[r + 1]], el[ro[r]:ro[r + 1]]))))
    rng = np.random.default_rng(seed)
    span = n_part * STRIDE
    tx = []
    for t in range(n_tx):
        n_ex = int(rng.integers(1, 30))
        starts = np.sort(rng.integers(0, span - 10_000, 1))[0] + np.cumsum(rng.integers(50, 3000, n_ex))
        ivs = [(int(a), int(a + rng.integers(50, 400))) for a in starts]
        tx.append(dict(tid="ENST%011d" % t, intervals=ivs[::-1] if t % 2 else ivs))
    return reads, tx, sorted(bounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--partitions", type=int, default=4000)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    t0 = time.perf_counter()
    reads, tx, bounds = make_case(args.partitions)
    gen_s = time.perf_counter() - t0
    s_pos = {"chrS": set(bounds)}
    sv.switch_to_nearest(s_pos, s_pos)
    segs = sv.get_seg_track(s_pos, s_pos)
    plan = sv.Plan(segs, {"chrS": {t["tid"]: t for t in tx}}, {"chrS": reads})
    t0 = time.perf_counter()
    arrays = plan.arrays(segs)
    arr_ms = (time.perf_counter() - t0) * 1e3
    n_iv = int(arrays[2][-1])
    ctx = sv.Context(0)
    try:
        calls, kernels = [], []
        for _ in range(args.repeat + 1):
            t0 = time.perf_counter()
            flag_off, seg, cls = ctx.classify(*arrays)
            calls.append((time.perf_counter() - t0) * 1e3)
            kernels.append(ctx.kernel_ms)
    finally:
        ctx.close()
    t0 = time.perf_counter()
    datas = sv.data_dicts(flag_off, seg, cls)
    for o, d in zip(plan.objects, datas):
        o["data"] = d
    dict_ms = (time.perf_counter() - t0) * 1e3
    call_ms, kernel_ms = float(np.median(calls[1:])), float(np.median(kernels[1:]))
    total = arr_ms + call_ms + dict_ms
    print("case: %d reads + %d transcripts = %d objects, %d intervals, %d segments, %d flagged (object, segment) pairs "
          "(generated in %.1f s)" % (len(reads), len(tx), len(plan.objects), n_iv, len(segs["chrS"]["segs"]), len(seg), gen_s))
    print("kernel ms (median of %d, first call dropped): %.3f   [%s]" % (args.repeat, kernel_ms, ", ".join("%.3f" % k for k in kernels)))
    print("call ms   (fvis_classify with uploads and copies back): %.1f   [%s]" % (call_ms, ", ".join("%.1f" % c for c in calls)))
    print("host: object arrays %.1f ms, dict building %.1f ms" % (arr_ms, dict_ms))
    print("share of arrays + call + dicts spent building dicts: %.2f" % (dict_ms / total))
    cnt = np.bincount(cls, minlength=3)
    print("classes: 0: %d, 1: %d, 2: %d" % tuple(cnt))


if __name__ == "__main__":
    main()
