#!/usr/bin/env python3
"""The kernels' per-lane code of the branch and bound over a round's larger problems (freddie_amd/csrc/clu_bnb.h) against the Python
mirror (cluster_solve.bnb_task) without a GPU: builds tools/bnb_host_check.cpp with the address and undefined-behaviour sanitizers,
feeds it problems as the device sees them and compares every task's cost2, mask, node count and capped flag.  The problems: the grid of
the host tests (seeds 1 .. 40, with and without gaps and pairs, refused ones left out) under the three recycle models at depths 0 .. 12
with and without the greedy's bound; random ones of up to 40 columns at node_cap 256 with other epsilons, offsets and a short
MAX_ISOFORM_LG; two families of 33 and of 64 columns whose optimum lies at the columns from 32 on; the epsilon 0.15 boundary rows.

    python tools/bnb_host_check.py [--cases N]
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


def problem_text(model, settings, depth, node_cap, ub2):
    """One problem in the harness' input format, from the model's arrays."""
    out = [model["n_cols"], depth, node_cap, -1 if ub2 is None else ub2, settings["offset"], model["max_lg"], (1.0 - settings["epsilon"]).hex(),
           (1.0 + settings["epsilon"]).hex()]
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


def family_tint(tid, R, n_low, gaps=None, weight=None):
    """Two families of reps and two reps that tie them into one component: family A, reps 0 .. n_low - 1, is all ones with one 0 at a
    place of the rep's own (rep 0: none); family B, reps n_low .. R - 1, has three 0s in common and one of the rep's own (rep n_low:
    none).  Two reps of a family differ in at most 2 segments and are compatible, two of different families in at least 3 and are not.
    Reps R (one of B's 0s) and R + 1 (two of them) are compatible with each other, with A resp. B and with rep 0, so the partition is
    one; a problem leaves them out: remaining = range(R), with every cross pair in its pair list.  A rep of B stands for n_low + 1
    reads, so B as a whole is the optimum -- cost (R - n_low - 1) + 3 n_low under the constant model -- at the columns from n_low on.
    gaps: make_tint()'s, {rep: {(j1, j2): l}}; weight: the reads a rep of B stands for, n_low + 1 by default.
    Returns (tint as read_segment() leaves it, the cross pairs)."""
    n_high = R - n_low
    assert n_low >= 1 and n_high >= 1
    M = R + 6
    common = [1, 2, 3]
    rows = []
    for i in range(R):
        row = [1] * M
        if i >= n_low:
            for j in common:
                row[j] = 0
        if i not in (0, n_low):
            row[3 + i] = 0                                   # places 4 .. R + 2 < M - 1
        rows.append(row)
    for zeros in (common[:1], common[:2]):
        row = [1] * M
        for j in zeros:
            row[j] = 0
        rows.append(row)
    tint = ru.make_tint(tid, rows, gaps, members={i: n_low + 1 if weight is None else weight for i in range(n_low, R)})
    return tint, [(a, b) for a in range(n_low) for b in range(n_low, R)]


def family_model(R, n_low, recycle_model="constant"):
    """The problem of family_tint()'s reps 0 .. R - 1 as a model dict, with the tint (preprocessed) and the pairs: (model, tint, incomp)."""
    tint, incomp = family_tint(0, R, n_low)
    cluster_prep.preprocess_ilp(tint, dict(recycle_model="constant"))
    remaining = list(range(R))
    model = ru.restate(tint, incomp, remaining)
    assert model["refused"] is None
    model["garbage"] = ru.garbage_costs(tint, remaining, recycle_model)
    model["max_lg"] = sum(s[2] for s in tint["segs"])
    return model, tint, incomp


def greedy2(model, settings):
    inc = cluster_solve.greedy_incumbent(model, settings)
    return None if inc is None else inc["cost2"]


def cases(n_random):
    """(model, settings, depth, node_cap, ub2)"""
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
            for k, recycle_model in enumerate(cluster_solve.RECYCLE_MODELS):
                m = dict(model, garbage=ru.garbage_costs(tint, remaining, recycle_model), max_lg=sum(s[2] for s in tint["segs"]))
                settings = cluster.ilp_settings(recycle_model)
                yield m, settings, (0, 1, 2, 3, 12)[(seed + k) % 5], (1, 7, 4096)[(seed // 5 + k) % 3], greedy2(m, settings) if (seed + k) % 2 else None
    rng = random.Random(23)
    for k in range(n_random):
        n, M = rng.choice([1, 2, 5, 14, 25, 31, 32, 33, 40]), rng.choice([1, 3, 12, 31, 32, 33, 64, 65, 100])
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
        yield model, settings, rng.choice([0, 2, 5]), 256, greedy2(model, settings) if k % 2 else None
    settings = cluster.ilp_settings()
    for R, n_low in ((33, 32), (64, 32)):
        model = family_model(R, n_low)[0]
        yield model, settings, 4, 4096, greedy2(model, settings)
        yield model, settings, 3, 64, None
    for l in (250, 251, 671):
        yield boundary_model(l), cluster.ilp_settings(epsilon=0.15), 1, 4096, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=120, help="random problems beside the grid")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "bnb_host_check")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I", os.path.join(ROOT, "freddie_amd", "csrc"), os.path.join(ROOT, "tools", "bnb_host_check.cpp"), "-o", exe])
        texts, want, owner = [], [], []
        found = capped = 0
        for k, (model, settings, depth, node_cap, ub2) in enumerate(cases(args.cases)):
            texts.append(problem_text(model, settings, depth, node_cap, ub2))
            tb = cluster_solve.bnb_tables(model, settings)
            D = min(tb["R"], depth)
            for t in range(1 << D):
                cost2, mask, nodes, cap = cluster_solve.bnb_task(tb, t, D, ub2, node_cap)
                want.append([cost2, mask, nodes, int(cap)])
                owner.append((k, t))
                found += cost2 >= 0
                capped += cap
        res = subprocess.run([exe], input="\n".join(texts) + "\n", capture_output=True, text=True)
        if res.returncode != 0:
            sys.exit("the harness failed:\n" + res.stderr[-4000:])
        got = [[int(v) for v in line.split()] for line in res.stdout.splitlines()]
        assert len(got) == len(want), (len(got), len(want))
        bad = [i for i, w in enumerate(want) if got[i] != w]
        for i in bad[:5]:
            print("problem %d task %d: got %r, the mirror %r" % (owner[i] + (got[i], want[i])))
        print("%d problems, %d tasks: %d differ (%d tasks with a leaf, %d capped, %d nodes)" %
              (len(texts), len(want), len(bad), found, capped, sum(w[2] for w in want)))
        return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
