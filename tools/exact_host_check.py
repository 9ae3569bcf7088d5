#!/usr/bin/env python3
"""The kernels' per-thread code of the exact small-problem solve (freddie_amd/csrc/clu_exact.h) against the Python mirror
(cluster_solve.exact_small) without a GPU: builds tools/exact_host_check.cpp with the address and undefined-behaviour sanitizers, feeds
it problems as the device sees them (inf_seg, the support and correction lists, conflict pairs, gap groups and rows) and compares cost2
and mask.  The problems: the grid of the host tests (seeds 1 .. 40, with and without gaps and pairs, refused ones left out) under the
three recycle models, random ones up to 14 columns with other epsilons, offsets and a short MAX_ISOFORM_LG, and the epsilon 0.15
boundary rows; the slice sizes go from 1 mask up to the whole problem.

    python tools/exact_host_check.py [--cases N]
"""
import argparse
import os
import random
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import round_util as ru  # noqa: E402
from freddie_amd import cluster, cluster_prep, cluster_solve  # noqa: E402


def csr(lists):
    off = [0]
    for l in lists:
        off.append(off[-1] + len(l))
    return off + [v for l in lists for v in l]


def problem_text(model, settings, slice_masks):
    """One problem in the harness' input format, from the model's arrays."""
    out = [model["n_cols"], slice_masks, settings["offset"], model["max_lg"], (1.0 - settings["epsilon"]).hex(), (1.0 + settings["epsilon"]).hex()]
    out.append(len(model["inf_seg"]))
    out.extend(model["inf_seg"])
    out.extend(csr(model["support"]))
    out.extend(csr(model["corrections"]))
    out.extend(cluster_solve.garbage2(model["garbage"]))
    out.append(len(model["pairs"]))
    for a, b in model["pairs"]:
        out.extend((a, b))
    out.append(len(model["group_segs"]))
    out.extend(csr([[j for j, _ in segs] for segs in model["group_segs"]]))
    out.extend(ln for segs in model["group_segs"] for _, ln in segs)
    out.append(len(model["gap_rows"]))
    for c, g, l in model["gap_rows"]:
        out.extend((c, g, l))
    return " ".join(map(str, out))


def boundary_model(l):
    """Two columns over three segments; column 0 has a gap (0, 2) of length l whose group is segment 1, 200 long, covered by column 1."""
    return dict(n_cols=2, inf_seg=[0, 1, 2], support=[[0, 1], [1], [0, 1]], corrections=[[1], []], pairs=[], groups=[(0, 2)],
                group_segs=[[(1, 200)]], gap_rows=[(0, 0, l)], garbage=[50.0, 50.0], max_lg=400)


def cases(n_random):
    for seed in range(1, 41):                                # the grid
        n, M = 6 + seed % 7, 5 + seed % 9
        for with_gaps, with_pairs in ((False, False), (True, False), (False, True), (True, True)):
            rng = random.Random(seed)
            rows = ru.random_rows(rng, n, M, const_runs=seed % 2 == 0, flip=0.1)
            gaps, polys = ru.random_gaps(rng, rows, p=0.7) if with_gaps else ({}, {})
            tint = ru.make_tint(seed, rows, gaps, polys, members={i: rng.randrange(1, 4) for i in range(n)})
            cluster_prep.preprocess_ilp(tint, dict(recycle_model="constant"))
            incomp = [(a, b) for a in range(n) for b in range(a + 1, n) if rng.random() < 0.25] if with_pairs else []
            remaining = list(range(n))
            model = ru.restate(tint, incomp, remaining)
            if model["refused"] is not None:
                continue
            for recycle_model in cluster_solve.RECYCLE_MODELS:
                m = dict(model, garbage=ru.garbage_costs(tint, remaining, recycle_model), max_lg=sum(s[2] for s in tint["segs"]))
                yield m, cluster.ilp_settings(recycle_model), (1, 64, 256, 1000, 4096)[seed % 5]
    rng = random.Random(23)
    for k in range(n_random):
        n, M = rng.choice([1, 2, 3, 5, 9, 12, 14]), rng.choice([1, 3, 12, 31, 32, 33, 64, 65, 100])
        rows = ru.random_rows(rng, n, M, const_runs=k % 2 == 0, flip=0.1)
        gaps, polys = ru.random_gaps(rng, rows, p=0.7) if k % 3 else ({}, {})
        tint = ru.make_tint(k, rows, gaps, polys, members={i: rng.randrange(1, 4) for i in range(n)})
        cluster_prep.preprocess_ilp(tint, dict(recycle_model="constant"))
        incomp = [(a, b) for a in range(n) for b in range(a + 1, n) if rng.random() < (0.15 if k % 4 else 0.0)]
        remaining = list(range(n))
        rng.shuffle(remaining)
        remaining = remaining[:max(1, n - rng.randrange(3))]
        settings = cluster.ilp_settings(rng.choice(cluster_solve.RECYCLE_MODELS), epsilon=rng.choice([0.2, 0.0, 0.35, 0.15]), offset=rng.choice([20, 0, 3]))
        model = ru.restate(tint, incomp, remaining)
        if model["refused"] is not None:
            continue
        model["garbage"] = ru.garbage_costs(tint, remaining, settings["recycle_model"])
        model["max_lg"] = sum(s[2] for s in tint["segs"]) if k % 5 else 30        # (a short "tint": outside rows get violated too)
        yield model, settings, rng.choice([1, 7, 256, 4096])
    for l in (250, 251, 249):
        yield boundary_model(l), cluster.ilp_settings(epsilon=0.15), 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=200, help="random problems beside the grid")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "exact_host_check")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I", os.path.join(ROOT, "freddie_amd", "csrc"), os.path.join(ROOT, "tools", "exact_host_check.cpp"), "-o", exe])
        texts, want = [], []
        for model, settings, slice_masks in cases(args.cases):
            texts.append(problem_text(model, settings, slice_masks))
            m = cluster_solve.exact_small(model, settings)
            want.append([-1, 0] if m is None else [m["cost2"], m["mask"]])
        res = subprocess.run([exe], input="\n".join(texts) + "\n", capture_output=True, text=True)
        if res.returncode != 0:
            sys.exit("the harness failed:\n" + res.stderr[-4000:])
        got = [[int(v) for v in line.split()] for line in res.stdout.splitlines()]
        assert len(got) == len(want), (len(got), len(want))
        bad = [k for k, w in enumerate(want) if got[k] != w]
        for k in bad[:5]:
            print("case %d: got %r, the mirror %r" % (k, got[k], want[k]))
        print("%d problems: %d differ (%d optima not empty, %d without a feasible set)" %
              (len(want), len(bad), sum(1 for w in want if w[1]), sum(1 for w in want if w[0] < 0)))
        return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
