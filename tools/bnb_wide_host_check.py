#!/usr/bin/env python3
"""The kernels' per-lane code and task walk of the branch and bound over a round's problems of up to 1024 columns
(freddie_amd/csrc/clu_bnb_wide.h) against the Python mirror (cluster_solve.bnb_task on exact_bnb_wide()'s tables) without a GPU: builds
tools/bnb_wide_host_check.cpp with the address and undefined-behaviour sanitizers, feeds it problems as the device sees them and
compares every task's cost2, mask, node count and capped flag.  The problems: those of tools/bnb_host_check.py (the single-word sizes);
the families of 65, 128, 129 and 200 columns whose optimum lies at the upper columns; random ones of 65 .. 140 columns with gaps and
pairs, capped; the two-optima tie; 70 columns without an informative segment; the 300-column all-in problem at depth 0.

    python tools/bnb_wide_host_check.py [--cases N]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import round_util as ru  # noqa: E402
from bnb_host_check import cases as narrow_cases, family_model, family_tint, greedy2, problem_text  # noqa: E402
from freddie_amd import cluster, cluster_prep, cluster_solve  # noqa: E402


def random_model(seed, n, M, with_gaps, with_pairs, recycle_model="constant"):
    """A random problem of n columns over M segments, all columns remaining."""
    rng = random.Random(seed)
    rows = ru.random_rows(rng, n, M, const_runs=seed % 2 == 0, flip=0.1)
    gaps, polys = ru.random_gaps(rng, rows, p=0.7) if with_gaps else ({}, {})
    tint = ru.make_tint(seed, rows, gaps, polys, members={i: rng.randrange(1, 4) for i in range(n)})
    cluster_prep.preprocess_ilp(tint, dict(recycle_model="constant"))
    incomp = [(a, b) for a in range(n) for b in range(a + 1, n) if rng.random() < 0.25] if with_pairs else []
    remaining = list(range(n))
    model = ru.restate(tint, incomp, remaining)
    if model["refused"] is not None:
        return None
    model["garbage"] = ru.garbage_costs(tint, remaining, recycle_model)
    model["max_lg"] = sum(s[2] for s in tint["segs"])
    return model


def tie_tint(tid):
    """family_tint() of 128 reps, 64 a family, every rep one read: family A at the columns 0 .. 63 costs its 63 corrections and B's 64
    garbage costs, family B at the columns 64 .. 127 its 63 and A's 64.  Exactly two optimal sets; the smaller mask is A's."""
    return family_tint(tid, 128, 64, weight=1)[0]


def tie_model():
    tint, incomp = family_tint(0, 128, 64, weight=1)
    cluster_prep.preprocess_ilp(tint, dict(recycle_model="constant"))
    remaining = list(range(128))
    model = ru.restate(tint, incomp, remaining)
    assert model["refused"] is None
    model["garbage"] = ru.garbage_costs(tint, remaining, "constant")
    model["max_lg"] = sum(s[2] for s in tint["segs"])
    return model, tint, incomp


def bare_model(R):
    """R columns of garbage cost 1.5, no informative segment, no pair, no row: the empty table."""
    return dict(n_cols=R, inf_seg=[], support=[], corrections=[[]] * R, pairs=[], groups=[], group_segs=[], gap_rows=[], garbage=[1.5] * R, max_lg=0)


def all_in_model(R):
    """R reps of one pattern without gaps and pairs: the optimum is every column (the two end segments are the informative ones)."""
    tint = ru.make_tint(0, [[1, 0, 1, 1]] * R)
    cluster_prep.preprocess_ilp(tint, dict(recycle_model="constant"))
    model = ru.restate(tint, [], list(range(R)))
    assert model["refused"] is None
    model["garbage"] = ru.garbage_costs(tint, list(range(R)), "constant")
    model["max_lg"] = sum(s[2] for s in tint["segs"])
    return model


def cases(n_narrow):
    """(model, settings, depth, node_cap, ub2)"""
    for k, case in enumerate(narrow_cases(0)):
        if k % 3 == 0 or k >= n_narrow:                      # a third of the grid, and the families and boundary rows behind it
            yield case
    settings = cluster.ilp_settings()
    for R, n_low in ((65, 64), (65, 32), (128, 64), (129, 128), (200, 70)):
        model = family_model(R, n_low)[0]
        yield model, settings, 6, 4096, greedy2(model, settings)
    yield family_model(65, 32)[0], settings, 2, 40, None
    yield tie_model()[0], settings, 6, 4096, None
    yield bare_model(70), settings, 3, 50, None              # (no informative segment: a tint always has one, so this one is a model of its own)
    yield bare_model(70), settings, 0, 4096, 0
    for seed, n, M, depth, node_cap in ((1, 70, 12, 6, 300), (3, 65, 70, 3, 200), (5, 80, 12, 2, 100), (6, 130, 130, 4, 150), (7, 140, 30, 0, 500)):
        for with_gaps, with_pairs in ((False, False), (True, True)):
            model = random_model(seed, n, M, with_gaps, with_pairs, "exons" if seed % 2 else "constant")
            if model is not None:
                yield model, settings, depth, node_cap, greedy2(model, settings) if seed % 3 else None
    model = all_in_model(300)
    yield model, settings, 0, 4096, greedy2(model, settings)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=480, help="problems of the narrow check's grid a third of which is run")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "bnb_wide_host_check")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I", os.path.join(ROOT, "freddie_amd", "csrc"), os.path.join(ROOT, "tools", "bnb_wide_host_check.cpp"), "-o", exe])
        texts, want, owner = [], [], []
        found = capped = wide = 0
        for k, (model, settings, depth, node_cap, ub2) in enumerate(cases(args.cases)):
            texts.append(problem_text(model, settings, depth, node_cap, ub2))
            tb = cluster_solve.bnb_tables(model, settings, cluster_solve.BNB_WIDE_MAX_COLS, "exact_bnb_wide")
            wide += tb["R"] > 64
            D = min(tb["R"], depth)
            for t in range(1 << D):
                cost2, mask, nodes, cap = cluster_solve.bnb_task(tb, t, D, ub2, node_cap)
                want.append([cost2, nodes, int(cap), mask])
                owner.append((k, t))
                found += cost2 >= 0
                capped += cap
        res = subprocess.run([exe], input="\n".join(texts) + "\n", capture_output=True, text=True)
        if res.returncode != 0:
            sys.exit("the harness failed:\n" + res.stderr[-4000:])
        got = [[int(v) for v in line.split()[:3]] + [int(line.split()[3], 16)] for line in res.stdout.splitlines()]
        assert len(got) == len(want), (len(got), len(want))
        bad = [i for i, w in enumerate(want) if got[i] != w]
        for i in bad[:5]:
            print("problem %d task %d: got %r, the mirror %r" % (owner[i] + (got[i], want[i])))
        print("%d problems (%d of more than 64 columns), %d tasks: %d differ (%d tasks with a leaf, %d capped, %d nodes)" %
              (len(texts), wide, len(want), len(bad), found, capped, sum(w[1] for w in want)))
        return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
