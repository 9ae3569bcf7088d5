#!/usr/bin/env python3
"""The passes of the branch and bound over a round's problems of up to 1024 columns (freddie_amd/csrc/clu_bnb_wide.h: bw_task_from, the
roll-back of a capped task, bw_open_include / bw_open_count / bw_open_emit) against the Python mirror (cluster_solve.bnb_prefix_task on
exact_bnb_wide()'s tables) without a GPU: builds tools/bnb_passes_host_check.cpp with the address and undefined-behaviour sanitizers,
feeds it problems as the device sees them with a number of passes and a task limit, and compares every task of every pass: its prefix
length, cost2, mask, node count, capped flag and the number of its open children -- the records themselves are the next pass's tasks.
The problems: a sixth of tools/bnb_host_check.py's grid at caps of 1 .. 7 nodes; the families of 65, 70 and 129 columns and the
128-column tie at depth 2 and caps 40 and 300; random ones of 65 .. 140 columns with gaps and pairs; 70 columns without an informative
segment (E = 0), whose capped tasks leave prefixes of every length up to R.

    python tools/bnb_passes_host_check.py
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bnb_host_check import cases as narrow_cases, family_model, greedy2, problem_text  # noqa: E402
from bnb_wide_host_check import bare_model, random_model, tie_model  # noqa: E402
from freddie_amd import cluster, cluster_solve  # noqa: E402


def cases():
    """(model, settings, depth, node_cap, ub2, passes, max_tasks)"""
    for k, (model, settings, depth, node_cap, ub2) in enumerate(narrow_cases(0)):
        if k % 6 == 0:
            yield model, settings, min(depth, 3), (1, 2, 3, 7)[k // 6 % 4], ub2, 1 + k // 6 % 5, 4096
    settings = cluster.ilp_settings()
    for R, n_low in ((65, 32), (70, 6), (129, 128)):
        model = family_model(R, n_low)[0]
        for node_cap in (40, 300):
            yield model, settings, 2, node_cap, greedy2(model, settings), 6, 4096
    yield family_model(65, 32)[0], settings, 2, 40, None, 4, 4096
    model = tie_model()[0]
    yield model, settings, 2, 300, greedy2(model, settings), 6, 4096
    yield model, settings, 2, 40, None, 3, 4096
    yield bare_model(70), settings, 3, 50, None, 4, 4096      # (E = 0; every child is a leaf's ancestor, so the prefixes reach L = R)
    yield bare_model(70), settings, 0, 8, 0, 16, 4096
    yield bare_model(3), settings, 0, 2, None, 4, 2           # (a pass beyond max_tasks is not run)
    for seed, n, M, depth, node_cap in ((1, 70, 12, 3, 30), (3, 65, 70, 3, 20), (6, 130, 130, 2, 50)):
        for with_gaps, with_pairs in ((False, False), (True, True)):
            model = random_model(seed, n, M, with_gaps, with_pairs, "exons" if seed % 2 else "constant")
            if model is not None:
                yield model, settings, depth, node_cap, greedy2(model, settings), 5, 2048


def mirror_tasks(model, settings, depth, node_cap, ub2, passes, max_tasks):
    """Every task of every pass, in the order the harness runs them: [pass, L, cost2, nodes, capped, open children, mask]."""
    tb = cluster_solve.bnb_tables(model, settings, cluster_solve.BNB_WIDE_MAX_COLS, "exact_bnb_wide")
    D = min(tb["R"], depth)
    tasks, best, out = [(t, D) for t in range(1 << D)], None, []
    for k in range(1, passes + 1):
        bound = ub2 if best is None else best if ub2 is None else min(ub2, best)
        opened = []
        for P, L in tasks:
            cost2, mask, nodes, cap, children = cluster_solve.bnb_prefix_task(tb, P, L, bound, node_cap)
            out.append([k, L, cost2, nodes, int(cap), len(children), mask])
            opened += children
            if cost2 >= 0 and (best is None or cost2 < best):
                best = cost2
        if not opened or len(opened) > max_tasks:
            break
        tasks = opened
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "bnb_passes_host_check")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I", os.path.join(ROOT, "freddie_amd", "csrc"), os.path.join(ROOT, "tools", "bnb_passes_host_check.cpp"), "-o", exe])
        texts, want, owner = [], [], []
        for k, (model, settings, depth, node_cap, ub2, passes, max_tasks) in enumerate(cases()):
            texts.append("%d %d %s" % (passes, max_tasks, problem_text(model, settings, depth, node_cap, ub2)))
            rows = mirror_tasks(model, settings, depth, node_cap, ub2, passes, max_tasks)
            want += rows
            owner += [k] * len(rows)
        res = subprocess.run([exe], input="\n".join(texts) + "\n", capture_output=True, text=True)
        if res.returncode != 0:
            sys.exit("the harness failed:\n" + res.stderr[-4000:])
        got = [[int(v) for v in line.split()[:6]] + [int(line.split()[6], 16)] for line in res.stdout.splitlines()]
        assert len(got) == len(want), (len(got), len(want))
        bad = [i for i, w in enumerate(want) if got[i] != w]
        for i in bad[:5]:
            print("problem %d: got %r, the mirror %r" % (owner[i], got[i], want[i]))
        later = [w for w in want if w[0] > 1]
        model_R = {k: c[0]["n_cols"] for k, c in enumerate(cases())}
        print("%d problems, %d tasks (%d behind the first pass, %d of them with a prefix of L = R, %d with two or more open children): %d differ "
              "(%d capped, %d nodes)" % (len(texts), len(want), len(later), sum(w[1] == model_R[owner[i]] for i, w in enumerate(want) if w[0] > 1),
                                         sum(1 for w in want if w[5] >= 2), len(bad), sum(w[4] for w in want), sum(w[3] for w in want)))
        assert later and any(w[1] == model_R[owner[i]] for i, w in enumerate(want) if w[0] > 1), "the cases do not reach the passes or L = R"
        return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
