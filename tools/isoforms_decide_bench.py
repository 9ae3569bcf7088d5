#!/usr/bin/env python3
"""--decide host against --decide gpu on one synthetic batch of the shape tools/isoforms_bench.py uses (4 000 isoforms x 500
reads x 150 segments, 12 exons an isoform, 8 alignment intervals a read, window 8), in one session.

    python tools/isoforms_decide_bench.py [--runs 3] [--out profiles/isoforms_decide.txt]

host path  what run_consensus_batch() does between the readers and the GTF writer by default: Context.consensus (label bytes
           in, counts out), the per-isoform flags / exon runs / strand in Python, two Context.boundary_votes calls (votes out)
           and the per-boundary loops in Python -- the loops of isoforms_cons_batch() / correct_boundaries_batch() on arrays.
gpu path   pack_label_bits (timed apart as well: a producer that holds bits does not pay it) + one Context.isoforms call.
Both start from the label bytes and the reads' boundaries in host arrays and end with every isoform's strand and corrected
exons; the two results are compared.  Prints a text report (and writes it to --out) whose last line is one JSON document.
"""
import argparse
import json
import os
import sys
import time
from itertools import groupby

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from freddie_amd import isoforms  # noqa: E402


def make_batch(n_iso, per, M, n_exon, per_read, seed=11):
    """Labels that follow an isoform pattern of n_exon runs (5 % of the labels flipped, 2 % of the rest '2'), tails, positions,
    and per_read alignment intervals a read: boundaries of the isoform's exons, moved."""
    rng = np.random.default_rng(seed)
    R = n_iso * per
    pos = (1000 + 40 * np.arange(M + 1) + rng.integers(0, 5, M + 1)).astype(np.int32)
    cuts = np.sort(np.stack([rng.permutation(M - 1)[:2 * n_exon - 1] + 1 for _ in range(n_iso)]), axis=1)      # run borders
    edge = np.concatenate([np.zeros((n_iso, 1), np.int64), cuts, np.full((n_iso, 1), M)], axis=1)              # 2 n_exon + 1
    run_of = (np.arange(M)[None, :, None] >= edge[:, None, 1:]).sum(2)                                          # (n_iso, M)
    pat = (run_of % 2 == 0)
    lab = np.repeat(pat, per, axis=0)
    lab ^= rng.random((R, M)) < 0.05
    lab = np.where(lab, ord("1"), np.where(rng.random((R, M)) < 0.02, ord("2"), ord("0"))).astype(np.uint8)
    tail = rng.integers(0, 3, R).astype(np.uint8)
    ex_first, ex_last = edge[:, 0:-1:2], edge[:, 1::2] - 1                                                      # (n_iso, n_exon)
    pick = np.sort(rng.integers(0, n_exon, (R, per_read)), axis=1)
    iso = np.repeat(np.arange(n_iso), per)[:, None]
    # nine boundaries in ten lie 3 after an exon's start / 2 before its end, so that most corrections find their majority
    rs = (pos[ex_first[iso, pick]] + np.where(rng.random((R, per_read)) < 0.9, 3, rng.integers(-12, 13, (R, per_read)))).astype(np.int32)
    re_ = (pos[ex_last[iso, pick] + 1] + np.where(rng.random((R, per_read)) < 0.9, -2, rng.integers(-12, 13, (R, per_read)))).astype(np.int32)
    return dict(n_iso=n_iso, per=per, M=M, R=R, pos=pos, lab=lab, tail=tail, rs=rs.reshape(-1), re=re_.reshape(-1), per_read=per_read,
                iro=np.arange(n_iso + 1, dtype=np.int64) * per, rbo=np.arange(R + 1, dtype=np.int64) * per_read)


def host_path(ctx, b, m, w):
    """(strand, starts, ends) per isoform (None without an exon), seconds per part, bytes across PCIe."""
    n_iso, M, R = b["n_iso"], b["M"], b["R"]
    t = {}
    t0 = time.perf_counter()
    ctx.kernel_ms = 0.0
    seg_off, cons, cov, tails = ctx.consensus(b["iro"], np.full(n_iso, M), np.arange(R, dtype=np.int64) * M, b["lab"].reshape(-1), b["tail"])
    t["consensus_call"] = time.perf_counter() - t0
    k_ms = {"consensus": ctx.kernel_ms}
    t0 = time.perf_counter()
    pos = b["pos"].tolist()
    out = [None] * n_iso
    for i in range(n_iso):                                           # isoforms_cons_batch()'s loop
        x = cons[seg_off[i]:seg_off[i + 1]].tolist(); c = cov[seg_off[i]:seg_off[i + 1]].tolist()
        flags = [p / q > 0.5 if p >= 3 else False for p, q in zip(x, c)]
        if True not in flags:
            continue
        starts, ends = [], []
        for d, group in groupby(enumerate(flags), lambda e: e[1]):
            if d is not True:
                continue
            group = list(group)
            starts.append(pos[group[0][0]]); ends.append(pos[group[-1][0] + 1])
        out[i] = ["-" if tails[i][1] > tails[i][2] else "+", starts, ends]
    t["decide_exons_python"] = time.perf_counter() - t0
    nbytes = b["lab"].nbytes + R + 8 * R + 20 * n_iso + 8 * n_iso * M + 12 * n_iso
    t["votes_calls"] = t["decide_votes_python"] = 0.0
    k_ms["votes"] = 0.0
    for side, rb in ((1, b["rs"]), (2, b["re"])):                    # correct_boundaries_batch(), a side at a time
        t0 = time.perf_counter()
        isos = [i for i in range(n_iso) if out[i] is not None]
        iso_b_off = np.concatenate([[0], np.cumsum([len(out[i][side]) for i in isos])]).astype(np.int64)
        iso_bound = np.asarray([v for i in isos for v in out[i][side]], np.int32)
        assert len(isos) == n_iso                                    # (every isoform of this batch has exons: the reads stay as they are)
        t["decide_votes_python"] += time.perf_counter() - t0
        t0 = time.perf_counter()
        ctx.kernel_ms = 0.0
        votes = ctx.boundary_votes(b["iro"], iso_b_off, iso_bound, b["rbo"], rb, w)
        t["votes_calls"] += time.perf_counter() - t0
        k_ms["votes"] += ctx.kernel_ms
        nbytes += 16 * n_iso + iso_bound.nbytes + b["rbo"].nbytes + rb.nbytes + votes.nbytes
        t0 = time.perf_counter()
        for a, i in enumerate(isos):
            n = b["per"]
            for idx in range(iso_b_off[a + 1] - iso_b_off[a]):
                iso_s = out[i][side][idx]
                for k, v in enumerate(votes[iso_b_off[a] + idx].tolist()):
                    if v / n >= m:
                        out[i][side][idx] = (k - w) + iso_s
        t["decide_votes_python"] += time.perf_counter() - t0
    return out, t, k_ms, nbytes


def gpu_path(ctx, b, m, w):
    n_iso, M, R = b["n_iso"], b["M"], b["R"]
    W = (M + 63) // 64
    t = {}
    t0 = time.perf_counter()
    bits = isoforms.pack_label_bits(b["lab"], M)
    t["pack_label_bits"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    ctx.kernel_ms = 0.0
    res = ctx.isoforms([0, M + 1], b["pos"], np.zeros(n_iso, np.int32), b["iro"], np.arange(R + 1, dtype=np.int64) * W, bits.reshape(-1),
                       b["tail"], b["rbo"], b["rs"], b["re"], m, w)
    t["isoforms_call"] = time.perf_counter() - t0
    k_ms = {"k_iso_exons + k_iso_correct": ctx.kernel_ms}
    t0 = time.perf_counter()
    out = [None] * n_iso
    off, ne = res["exon_off"], res["n_exon"]
    for i in np.flatnonzero(ne).tolist():                            # what decide_gpu_batch() does with the arrays
        lo, hi = int(off[i]), int(off[i]) + int(ne[i])
        out[i] = [chr(res["strand"][i]), res["start"][lo:hi].tolist(), res["end"][lo:hi].tolist()]
    t["results_to_lists"] = time.perf_counter() - t0
    # across PCIe: bits, tails, both sides' boundaries, the per-isoform offsets and tints, the positions; the result block back
    nbytes = bits.nbytes + R + b["rs"].nbytes + b["re"].nbytes + 28 * n_iso + b["pos"].nbytes + sum(res[k].nbytes for k in res)
    return out, t, k_ms, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--isoforms", type=int, default=4000)
    ap.add_argument("--reads-per-isoform", type=int, default=500)
    ap.add_argument("--segments", type=int, default=150)
    ap.add_argument("--exons", type=int, default=12)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    m, w = 0.5, 8
    b = make_batch(a.isoforms, a.reads_per_isoform, a.segments, a.exons, 8)
    ctx = isoforms.Context(0)
    host_path(ctx, b, m, w); gpu_path(ctx, b, m, w)                   # warm-up: module load, first allocations
    runs = {"host": [], "gpu": []}
    for _ in range(a.runs):                                          # alternating, so that drift hits both alike
        for name, fn in (("host", host_path), ("gpu", gpu_path)):
            t0 = time.perf_counter()
            out, t, k_ms, nbytes = fn(ctx, b, m, w)
            runs[name].append(dict(wall_s=time.perf_counter() - t0, parts_s=t, kernel_ms=k_ms, pcie_bytes=int(nbytes), out=out))
    ctx.close()
    same = runs["host"][-1]["out"] == runs["gpu"][-1]["out"]
    n_exons = sum(len(o[1]) for o in runs["gpu"][-1]["out"] if o)
    lines = ["isoform decisions: --decide host against --decide gpu, %d isoforms x %d reads x %d segments, %d exons found, window %d, "
             "threshold %g, %d runs of each (alternating, after one warm-up of each)" % (a.isoforms, a.reads_per_isoform, a.segments, n_exons, w, m, a.runs),
             "results identical: %s" % same]
    doc = {"config": {"isoforms": a.isoforms, "reads": b["R"], "segments": a.segments, "exons_found": n_exons, "window": w, "threshold": m},
           "results_identical": same}
    for name in ("host", "gpu"):
        walls = [r["wall_s"] for r in runs[name]]
        lines.append("%-4s wall s: %s   min %.3f max %.3f spread %.3f   PCIe MB %.1f" %
                     (name, " ".join("%.3f" % v for v in walls), min(walls), max(walls), max(walls) - min(walls), runs[name][0]["pcie_bytes"] / 1e6))
        for key in runs[name][0]["parts_s"]:
            lines.append("       %-22s %s" % (key, " ".join("%.3f" % r["parts_s"][key] for r in runs[name])))
        for key in runs[name][0]["kernel_ms"]:
            lines.append("       kernel ms %-28s %s" % (key, " ".join("%.3f" % r["kernel_ms"][key] for r in runs[name])))
        doc[name] = {"wall_s": walls, "parts_s": [r["parts_s"] for r in runs[name]], "kernel_ms": [r["kernel_ms"] for r in runs[name]],
                     "pcie_bytes": runs[name][0]["pcie_bytes"]}
    hw, gw = doc["host"]["wall_s"], doc["gpu"]["wall_s"]
    spread = max(max(hw) - min(hw), max(gw) - min(gw))
    doc["gpu_faster_beyond_spread"] = bool(np.median(hw) - np.median(gw) > spread)
    doc["speedup_median"] = float(np.median(hw) / np.median(gw))
    lines.append("median host - median gpu = %.3f s against a spread (max - min, the wider of the two) of %.3f s: gpu faster beyond the "
                 "spread: %s   median host / median gpu = %.2f" %
                 (np.median(hw) - np.median(gw), spread, doc["gpu_faster_beyond_spread"], doc["speedup_median"]))
    lines.append(json.dumps(doc))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
