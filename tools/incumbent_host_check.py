#!/usr/bin/env python3
"""The kernels' per-thread code of the greedy round incumbents (freddie_amd/csrc/clu_incumbent.h) against the Python mirror
(cluster_solve.greedy_incumbent) without a GPU: builds tools/incumbent_host_check.cpp with the address and undefined-behaviour
sanitizers, feeds it random and crafted problems as the device would see them (raw I / C rows, the informative row, conflict pairs, gap
groups and rows) and compares cost2, start, members and step counts, for the staged and the unstaged row path.

    python tools/incumbent_host_check.py [--cases N]
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


def words(row, W):
    out = [0] * W
    for j, v in enumerate(row):
        if v == 1:
            out[j // 32] |= 1 << (j % 32)
    return out


def problem_text(tint, remaining, model, settings, max_seeds):
    """One problem in the harness' input format, from the tint's raw rows and the model's arrays."""
    M = len(tint["segs"])
    W = max((M + 31) // 32, 1)
    I, C = tint["ilp_data"]["I"], tint["ilp_data"]["C"]
    out = [len(remaining), M, max_seeds, settings["offset"], model["max_lg"], (1.0 - settings["epsilon"]).hex(), (1.0 + settings["epsilon"]).hex()]
    for rows in (I, C):
        for i in remaining:
            out.extend(words(rows[i], W))
    out.extend(model["words"])
    out.extend(cluster_solve.garbage2(model["garbage"]))
    out.append(len(model["pairs"]))
    for a, b in model["pairs"]:
        out.extend((a, b))
    off = [0]
    for segs in model["group_segs"]:
        off.append(off[-1] + len(segs))
    out.append(len(model["groups"]))
    out.extend(off)
    out.extend(j for segs in model["group_segs"] for j, _ in segs)
    out.extend(ln for segs in model["group_segs"] for _, ln in segs)
    col_off = [0] * (len(remaining) + 1)
    for c, _, _ in model["gap_rows"]:
        col_off[c + 1] += 1
    for c in range(len(remaining)):
        col_off[c + 1] += col_off[c]
    out.extend(col_off)
    for c, g, l in model["gap_rows"]:                        # (already in column order)
        out.extend((c, g, l))
    return " ".join(map(str, out))


def cases(n_cases):
    rng = random.Random(17)
    for k in range(n_cases):
        n, M = rng.choice([1, 2, 5, 9, 33, 64, 65, 120]), rng.choice([1, 3, 12, 31, 32, 33, 64, 65, 100])
        rows = ru.random_rows(rng, n, M, const_runs=k % 2 == 0, flip=0.1)
        gaps, polys = ru.random_gaps(rng, rows, p=0.7) if k % 3 else ({}, {})
        tint = ru.make_tint(k, rows, gaps, polys, members={i: rng.randrange(1, 4) for i in range(n)})
        cluster_prep.preprocess_ilp(tint, dict(recycle_model="constant"))
        incomp = [(a, b) for a in range(n) for b in range(a + 1, n) if rng.random() < (0.15 if k % 4 else 0.0)]
        remaining = list(range(n))
        rng.shuffle(remaining)
        remaining = remaining[:max(1, n - rng.randrange(3))]
        settings = cluster.ilp_settings(rng.choice(cluster_solve.RECYCLE_MODELS), epsilon=rng.choice([0.2, 0.0, 0.35]), offset=rng.choice([20, 0, 3]))
        model = ru.restate(tint, incomp, remaining)
        if model["refused"] is not None:
            continue
        model["garbage"] = ru.garbage_costs(tint, remaining, settings["recycle_model"])
        model["max_lg"] = sum(s[2] for s in tint["segs"]) if k % 5 else 30        # (a short "tint": outside rows get violated too)
        yield tint, remaining, model, settings, rng.choice([1, 3, 64, 1000])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=300)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "incumbent_host_check")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I", os.path.join(ROOT, "freddie_amd", "csrc"), os.path.join(ROOT, "tools", "incumbent_host_check.cpp"), "-o", exe])
        texts, want = [], []
        for tint, remaining, model, settings, max_seeds in cases(args.cases):
            texts.append(problem_text(tint, remaining, model, settings, max_seeds))
            m = cluster_solve.greedy_incumbent(model, settings, max_seeds)
            want.append([-1, -1, 0, 0, 0] if m is None else [m["cost2"], m["start"], m["grow_steps"], m["repair_steps"], len(m["members"])] + m["members"])
        res = subprocess.run([exe], input="\n".join(texts) + "\n", capture_output=True, text=True)
        if res.returncode != 0:
            sys.exit("the harness failed:\n" + res.stderr[-4000:])
        got = [[int(v) for v in line.split()] for line in res.stdout.splitlines()]
        assert len(got) == 2 * len(want), (len(got), len(want))
        bad = [(k, path) for k, w in enumerate(want) for path in (0, 1) if got[2 * k + path] != w]
        for k, path in bad[:5]:
            print("case %d path %s: got %r, the mirror %r" % (k, "staged unstaged".split()[path], got[2 * k + path], want[k]))
        nonempty = sum(1 for w in want if w[4])
        repaired = sum(1 for w in want if w[3])
        none = sum(1 for w in want if w[0] < 0)
        print("%d problems, both paths: %d differ (%d incumbents not empty, %d with a repair step, %d without a feasible start)" %
              (len(want), len(bad), nonempty, repaired, none))
        return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
