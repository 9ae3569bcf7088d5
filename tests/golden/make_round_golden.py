#!/usr/bin/env python3
"""Mint the fixtures of the clustering rounds by executing the REFERENCE's own source of informative_segs(), output_isoforms() and
cluster_tint() (vpc-ccg/freddie py/freddie_cluster.py:331-344, :639-691, :694-780), with read_segment(), preprocess_ilp() and
partition_reads() under them, all taken from its syntax tree as tests/golden/make_cluster_golden.py does.

gurobipy cannot be imported here, so run_ilp() in that namespace is a STAND-IN that replays recorded per-round solutions: it calls the
reference's informative_segs(), takes the round's solution (x per remaining rep, e per informative segment, or "no solution") from a
chooser, wraps the values in objects with Gurobi's getAttr(), and then executes the reference's OWN read-out statements (:594, :601-635,
lifted from run_ilp's syntax tree) on them.  The chooser at mint time is this project's HiGHS solve on the plain restatement of
tests/round_util.py; which solution it picks does not matter to the fixtures, which store it: the stored RESULTS -- the informative row of
every (tint, remaining set) and the cluster_*.tsv bytes of every (tint, recorded solutions) -- are the reference functions' own.
Inputs: the reference's segment_*.tsv bytes already stored in tests/golden/*.npz.  Build container only.

Usage: python tests/golden/make_round_golden.py
"""
import ast
import contextlib
import gzip
import io
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/py/freddie_cluster.py"
WANT_FUNCS = {"read_segment", "find_segment_read", "preprocess_ilp", "garbage_cost_introns", "garbage_cost_exons", "split_list_evenly",
              "partition_reads", "informative_segs", "output_isoforms", "cluster_tint"}
WANT_NAMES = {"tint_prog", "internal_gap_re", "softclip_gap_re", "poly_gap_re", "read_prog", "internal_gap_prog", "softclip_gap_prog",
              "poly_gap_prog"}
# (fixture, maximum_ilp_size, min_isoform_size, max_rounds, the round of partition 0 recorded as "no solution" or None)
CASES = [("e_one_rep", 1000, 3, 30, None), ("e_plateau_touch", 1000, 3, 30, None), ("e_plateau_touch", 1000, 1, 30, None),
         ("e_refine_tie", 1000, 3, 30, None), ("g_tiny", 1000, 2, 30, None), ("g_tiny", 7, 0, 3, None), ("g1_long", 1000, 3, 30, None),
         ("g1_long", 7, 2, 2, None), ("g_sigma12", 7, 3, 30, 1), ("g_sigma12", 1000, 1, 4, None), ("g1_retention", 7, 3, 30, None)]
SOLVE_SECONDS = 20


class Var:
    def __init__(self, value):
        self.value = float(value)

    def getAttr(self, _):
        return self.value


class FakeGRB:
    class Attr:
        X = "X"


def load_reference():
    tree = ast.parse(open(REF).read(), REF)
    keep, readout = [], None
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in WANT_FUNCS:
            keep.append(node)
        elif isinstance(node, ast.Assign) and all(isinstance(t, ast.Name) and t.id in WANT_NAMES for t in node.targets):
            keep.append(node)
        elif isinstance(node, ast.FunctionDef) and node.name == "run_ilp":
            for stmt in node.body:                           # `if ILP_ISOFORMS_STATUS != GRB.Status.OPTIMAL: ... else: <the read-out>`
                if isinstance(stmt, ast.If) and "ILP_ISOFORMS_STATUS" in ast.dump(stmt.test):
                    readout = [s for s in stmt.orelse if not (isinstance(s, ast.If) and "log_prefix" in ast.dump(s.test))]
    assert readout and len(readout) == 4                     # status = 'OPTIMAL' and the three loops of :602-635
    ns = {"__name__": "freddie_cluster_partial"}
    exec("import os\nimport re\nfrom math import ceil, floor\nfrom networkx.algorithms import components\nfrom networkx import Graph\n", ns)
    exec(compile(ast.Module(body=keep, type_ignores=[]), REF, "exec"), ns)
    assert WANT_FUNCS <= set(ns) and WANT_NAMES <= set(ns)
    return ns, compile(ast.Module(body=readout, type_ignores=[]), REF, "exec")


def install_stand_in(ns, readout, chooser, record):
    def run_ilp(tint, remaining_rids, incomp_rids, ilp_settings, log_prefix):
        M = len(tint["segs"])
        I, C = tint["ilp_data"]["I"], tint["ilp_data"]["C"]
        informative = ns["informative_segs"](tint, remaining_rids)
        status, x, e = chooser(tint, list(remaining_rids), incomp_rids, ilp_settings)
        record(dict(remaining=list(remaining_rids), informative="".join("1" if v else "0" for v in informative), status=status, x=x, e=e))
        isoforms = {k: dict() for k in range(1, ilp_settings["K"])}
        if status != "OPTIMAL":
            return 9, "NO_SOLUTION", isoforms
        inf_seg = [j for j in range(M) if informative[j]]
        e_of = dict(zip(inf_seg, e))
        x_of = dict(zip(remaining_rids, x))
        env = dict(ISOFORM_INDEX_START=1, ilp_settings=ilp_settings, M=M, informative=informative, I=I, C=C, tint=tint,
                   remaining_rids=remaining_rids, isoforms=isoforms, GRB=FakeGRB,
                   E2I={j: {1: Var(e_of[j])} for j in inf_seg},
                   R2I={i: {0: Var(1 - x_of[i]), 1: Var(x_of[i])} for i in remaining_rids},
                   OBJ={i: {j: {1: Var(x_of[i] and e_of[j])} for j in inf_seg if C[i][j] > 0} for i in remaining_rids})
        exec(readout, env)
        return 2, env["status"], isoforms
    ns["run_ilp"] = run_ilp


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import round_util as ru
    from freddie_amd import cluster, cluster_solve
    ns, readout = load_reference()
    out_dir = os.path.join(HERE, "rounds")
    os.makedirs(out_dir, exist_ok=True)
    docs = []
    for name, max_ilp, min_size, max_rounds, fail_round in CASES:
        tsv = np.load(os.path.join(HERE, name + ".npz"))["segment_tsv"].tobytes()
        rounds, seen = [], dict()

        def chooser(tint, remaining, incomp, settings):
            part = [p for p, (_, inc) in enumerate(tint["partitions"]) if inc is incomp][0]
            seen[part] = seen.get(part, -1) + 1
            rounds.append(dict(partition=part, round=seen[part]))
            if part == 0 and seen[part] == fail_round:
                return "NO_SOLUTION", None, None
            model = ru.restate(tint, incomp, remaining)
            assert model["refused"] is None
            model["garbage"] = [tint["ilp_data"]["garbage_cost"][i] for i in remaining]
            model["max_lg"] = sum(s[2] for s in tint["segs"])
            return cluster_solve.solve_round(model, dict(settings, timeout=SOLVE_SECONDS / 60.0))

        install_stand_in(ns, readout, chooser, lambda rec: rounds[-1].update(rec))
        settings = dict(recycle_model="constant", K=2, epsilon=0.2, offset=20, timeout=1, max_rounds=max_rounds, threads=1)
        with tempfile.TemporaryDirectory() as d:
            os.makedirs(os.path.join(d, "seg", "ctg"))
            os.makedirs(os.path.join(d, "out", "ctg"))
            tid = int(tsv.split(b"\n", 1)[0].split(b"\t")[1])
            open(os.path.join(d, "seg", "ctg", "segment_ctg_%d.tsv" % tid), "wb").write(tsv)
            with contextlib.redirect_stdout(io.StringIO()):
                ns["cluster_tint"]((os.path.join(d, "seg"), os.path.join(d, "out"), "ctg", tid, settings, min_size, max_ilp, None))
            text = open(os.path.join(d, "out", "ctg", "cluster_ctg_%d.tsv" % tid)).read()
        docs.append(dict(name=name, max_ilp=max_ilp, min_isoform_size=min_size, max_rounds=max_rounds, rounds=rounds, tsv=text))
        print(name, max_ilp, min_size, max_rounds, "rounds", len(rounds), "optimal", sum(r["status"] == "OPTIMAL" for r in rounds),
              "isoform lines", text.count("\nisoform_"), "bytes", len(text))
    with gzip.GzipFile(os.path.join(out_dir, "rounds.json.gz"), "wb", mtime=0) as fz:
        fz.write(json.dumps(docs, sort_keys=True, separators=(",", ":")).encode())


if __name__ == "__main__":
    main()
