"""The passes of the wide branch and bound on the GPU (fclu_round_bnb_wide_passes) against the Python mirror behind the library's rule of
which problems a pass continues (test_bnb_passes_host.device_passes on cluster_solve.bnb_pass), exactly: status, cost2, every mask word,
node count and open tasks of every problem, n_taken, nodes_total and every row of the pass statistics; and one pass against
fclu_round_bnb_wide word for word.  The grid in one call; families of 63 .. 129 columns and the 128-column tie, whose prefixes cross
the words and reach L = R; passes of more than 64 records of one problem; one task a launch; E = 1; a budget that continues the
first problems only; two rounds and a resident round; the refusals; what stays valid behind the call; the loop.

A problem whose next pass would hold more than 2^16 tasks is covered on the host only (test_bnb_passes_host.test_the_budget_rules):
its mirror alone would take minutes."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest

from freddie_amd import cluster, cluster_prep, cluster_solve
from test_bnb_passes_host import PassesContext, device_passes
from test_gpu_incumbents import flips_tint, grid_tints
from test_gpu_round_bnb import BIG, SETTINGS, STATUS, family, garbage_of, models_of
from test_gpu_round_bnb_wide import counted_tint, whole
from test_gpu_round_models import all_problems, stage

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

from bnb_host_check import family_tint  # noqa: E402
from bnb_wide_host_check import tie_tint  # noqa: E402

pytestmark = pytest.mark.gpu

WORDS = cluster_prep.BNB_WIDE_WORDS
KEYS = ("status", "cost2", "mask", "nodes", "capped")


@pytest.fixture(scope="module")
def ctx():
    c = cluster_prep.Context(0)
    yield c
    c.close()


def check(got, rows, want, want_rows, n_taken):
    assert got["n_prob"] == len(want) and got["n_taken"] == n_taken
    for p, w in enumerate(want):
        mine = (int(got["status"][p]), int(got["cost2"][p]), [int(v) for v in got["mask"][p]], int(got["nodes"][p]), int(got["capped"][p]))
        if w is None:
            assert mine == (-2, -1, [0] * WORDS, 0, 0), (p, mine)
            continue
        mask = w["mask"] or 0
        assert mine == (STATUS[w["status"]], -1 if w["mask"] is None else w["cost2"], [mask >> (64 * i) & (2 ** 64 - 1) for i in range(WORDS)], w["nodes"],
                        w["capped"]), (p, mine, w)
    assert got["nodes_total"] == sum(w["nodes"] for w in want if w is not None)
    assert [{k: r[k] for k in ("tasks", "nodes", "capped", "problems")} for r in rows] == [{k: r[k] for k in ("tasks", "nodes", "capped", "problems")} for r in want_rows]
    assert all(r["launches"] >= 1 for r in rows) and got["n_launches"] == sum(r["launches"] for r in rows)


def compare(ctx, tints, part0, problems, passes, settings=SETTINGS, bound=True, min_cols=1, max_cols=1024, depth=2, node_cap=40, max_nodes=BIG, resident=False):
    """One round on the device and through the mirror; bound: the device's greedy incumbents' cost2 bounds both.  passes = 1 goes through
    fclu_round_bnb_wide_passes too (Context.round_bnb_wide would make the single call)."""
    models = models_of(tints, problems, settings)
    ctx.round_models([part0[t] + q for t, q, _ in problems], [rem for _, _, rem in problems], fetch=not resident)
    garbage = garbage_of(tints, problems, settings)
    ub2 = ctx.round_incumbents(garbage, settings["epsilon"], settings["offset"])["cost2"] if bound else np.full(len(problems), -1, np.int64)
    g2, col_off = ctx._garbage2("round_bnb_wide", garbage)
    got = ctx._round_search("round_bnb_wide", g2, col_off, ub2, settings["epsilon"], settings["offset"], min_cols, max_cols, max_nodes, depth, node_cap, WORDS, passes)
    rows = ctx.round_bnb_wide_pass_stats()
    want, want_rows, n_taken = device_passes(models, settings, ub2, min_cols, max_cols, depth, node_cap, max_nodes, passes)
    check(got, rows, want, want_rows, n_taken)
    if passes == 1:                                          # the single call, word for word
        plain = ctx.round_bnb_wide(garbage, ub2, settings["epsilon"], settings["offset"], min_cols, max_cols, max_nodes, depth, node_cap)
        assert all(plain[k].tolist() == got[k].tolist() for k in KEYS)
        assert all(plain[k] == got[k] for k in ("n_prob", "n_taken", "n_launches", "nodes_total")) and ctx.round_bnb_wide_pass_stats() == rows
    return got, rows, want, want_rows


@pytest.mark.parametrize("depth,node_cap", [(0, 2), (0, 7), (3, 2), (3, 7)])
def test_the_grid(ctx, depth, node_cap):
    """Every partition of the 80 grid tints in one call with 1, 2 and 6 passes, bounded by the greedy: problems that end in the first
    pass beside ones that go on, refused problems left in; more passes never prove less."""
    tints = grid_tints()
    part0 = stage(ctx, tints)
    problems = all_problems(tints, lambda t, q, rids: rids[::-1] if t % 3 == 0 else rids)
    proven = []
    for passes in (1, 2, 6):
        got, rows, want, _ = compare(ctx, tints, part0, problems, passes, depth=depth, node_cap=node_cap)
        proven.append(sum(w is not None and w["status"] == "optimal" for w in want))
        assert min(passes, 2) <= len(rows) <= passes and any(w is None for w in want)
    assert proven[0] < proven[1] <= proven[2]


BOUNDARY_SHAPES = [(63, 31), (65, 32), (70, 6), (129, 64)]


@pytest.fixture(scope="module")
def boundary():
    return [family(t, R, n_low) for t, (R, n_low) in enumerate(BOUNDARY_SHAPES)] + [tie_tint(len(BOUNDARY_SHAPES))]


def boundary_problems():
    """The families' R reps (a staged partition has two more, which tie the families into one component) and the tie's 128."""
    return [(t, 0, list(range(R))) for t, (R, _) in enumerate(BOUNDARY_SHAPES)] + [(len(BOUNDARY_SHAPES), 0, list(range(128)))]


def test_word_boundaries_and_the_tie(ctx, boundary):
    """Families of 63, 65, 70 and 129 columns and the 128-column tie at depth 2 with 40 and 300 nodes a task: records of one, two and
    three words in one pass, prefixes on either side of the word boundaries, and the tie's lower set."""
    tints = boundary
    part0 = stage(ctx, tints)
    assert [len(t["partitions"]) for t in tints] == [1] * len(tints)
    problems = boundary_problems()
    got, rows, want, want_rows = compare(ctx, tints, part0, problems, 6, node_cap=40)
    assert len(rows) > 2 and any(r["min_len"] <= 63 and r["max_len"] >= 65 for r in want_rows[1:])           # prefixes on both sides of a word boundary in one pass
    assert want[-1]["status"] == "optimal" and want[-1]["mask"] == (1 << 64) - 1
    compare(ctx, tints, part0, problems, 6, node_cap=300, bound=False)
    _, _, once, _ = compare(ctx, tints, part0, problems, 1, node_cap=40)
    assert all(want[p]["nodes"] > once[p]["nodes"] for p in (0, 1, 3, 4))                                     # records of one, two and three words
    compare(ctx, tints, part0, [(t, q, rem[::-1]) for t, q, rem in problems], 4, node_cap=40)          # (the families at the other end)


def test_many_records_of_one_problem_and_prefixes_of_every_length(ctx, boundary, monkeypatch):
    """The problems of at most 72 columns without a bound, 40 nodes a task: passes of more than a thousand records of one problem --
    several items, and under FCLU_BNB_WIDE_ITEM=64 several turns of a workgroup's waves -- most of which end at their first node, and prefixes that reach L = R.  The
    node budget keeps a pass under 4 000 tasks."""
    tints = boundary
    part0 = stage(ctx, tints)
    problems = boundary_problems()
    got, rows, want, want_rows = compare(ctx, tints, part0, problems, 5, node_cap=40, bound=False, max_cols=72, max_nodes=40 * 4000)
    taken = [w for w in want if w is not None]
    assert len(taken) == 3 and max(r["tasks"] for r in rows) > 64 * 8
    assert any(r["max_len"] in (63, 65, 70) for r in want_rows[1:]) and sum(r["nodes"] for r in rows) < 40000
    for item in (64, 3):                                     # a workgroup's waves take eight turns; three records a workgroup
        monkeypatch.setenv("FCLU_BNB_WIDE_ITEM", str(item))
        again, _, _, _ = compare(ctx, tints, part0, problems, 5, node_cap=40, bound=False, max_cols=72, max_nodes=40 * 4000)
        assert all(again[k].tolist() == got[k].tolist() for k in KEYS)


def test_one_task_a_launch(ctx, boundary, monkeypatch):
    """FCLU_BNB_WIDE_SLICE=1: every task of every pass is a launch of its own; the results and the rows are the same but for the launches."""
    tints = boundary
    part0 = stage(ctx, tints)
    problems = boundary_problems()[1:3]
    plain, rows, _, _ = compare(ctx, tints, part0, problems, 3, node_cap=40)
    assert [r["launches"] for r in rows] == [1] * len(rows) and len(rows) == 3
    monkeypatch.setenv("FCLU_BNB_WIDE_SLICE", "1")
    sliced, srows, _, _ = compare(ctx, tints, part0, problems, 3, node_cap=40)
    assert [r["launches"] for r in srows] == [r["tasks"] for r in rows] and max(r["tasks"] for r in rows) > 8
    monkeypatch.setenv("FCLU_BNB_WIDE_SLICE", "11")
    some, _, _, _ = compare(ctx, tints, part0, problems, 3, node_cap=40)
    for k in KEYS:
        assert sliced[k].tolist() == plain[k].tolist() == some[k].tolist()


def test_one_informative_segment(ctx):
    """70 columns over exactly one informative segment (E = 1), 34 nodes a task."""
    tints = [counted_tint(0, 70, 1, [])]
    part0 = stage(ctx, tints)
    problems = whole(tints)
    assert [len(m["inf_seg"]) for m in models_of(tints, problems, SETTINGS)] == [1]
    got, rows, want, want_rows = compare(ctx, tints, part0, problems, 4, node_cap=34)
    assert want[0]["status"] == "optimal" and want[0]["mask"] == (1 << 70) - 1
    assert [r["max_len"] for r in want_rows[:3]] == [2, 36, 70]          # every pass takes the all-in chain 34 columns on: a prefix of L = R
    got, rows, want, _ = compare(ctx, tints, part0, problems, 4, node_cap=34, bound=False, max_nodes=34 * 2000)
    assert want[0]["status"] == "unproven" and len(rows) == 2            # (without a bound the third pass is beyond the budget)


def test_a_budget_that_continues_the_first_problems_only(ctx):
    """Problems of 70, 66 and 68 columns at depth 4 and 10 nodes a task, all taken by pass 1; the budget holds the second pass of the 66
    and the 68 columns and not the 70's, which stays as pass 1 left it -- in pass 3 too, where there would be room."""
    tints = [flips_tint(0, 70, 44), flips_tint(1, 66, 44), flips_tint(2, 68, 44)]
    part0 = stage(ctx, tints)
    problems = whole(tints)
    models = models_of(tints, problems, SETTINGS)
    none = np.full(3, -1, np.int64)
    second = [cluster_solve.exact_bnb_wide(m, SETTINGS, None, 4, 10, passes=2)["pass_stats"][1]["tasks"] for m in models]
    budget = max(3 * 160, 10 * (second[1] + second[2]))
    assert budget < 10 * sum(second)
    got, rows, want, _ = compare(ctx, tints, part0, problems, 3, depth=4, node_cap=10, bound=False, max_nodes=budget)
    assert got["n_taken"] == 3 and [r["problems"] for r in rows[:2]] == [3, 2] and all(r["problems"] <= 2 for r in rows[1:])
    one = device_passes(models, SETTINGS, none, 1, 1024, 4, 10, BIG, 1)[0]
    assert want[0] == one[0] and want[1] != one[1] and want[2] != one[2]


def test_two_rounds_a_resident_round_and_what_stays_valid(ctx, boundary):
    """Two rounds on one context, each followed by one behind a resident round; behind the call the round's own results and the
    incumbents' are where they were."""
    tints = grid_tints()[::8] + boundary[:3]
    part0 = stage(ctx, tints)
    for pick in (lambda t, q, rids: rids, lambda t, q, rids: rids[1::2][::-1]):
        problems = all_problems(tints, pick)
        arr = ctx.round_models([part0[t] + q for t, q, _ in problems], [rem for _, _, rem in problems])
        garbage = garbage_of(tints, problems, SETTINGS)
        inc = ctx.round_incumbents(garbage, SETTINGS["epsilon"], SETTINGS["offset"])
        got = ctx.round_bnb_wide(garbage, inc["cost2"], SETTINGS["epsilon"], SETTINGS["offset"], 1, 1024, BIG, 2, 7, passes=4)
        assert got["passes"] == 4
        want, want_rows, n_taken = device_passes(models_of(tints, problems, SETTINGS), SETTINGS, inc["cost2"], 1, 1024, 2, 7, BIG, 4)
        check(got, ctx.round_bnb_wide_pass_stats(), want, want_rows, n_taken)
        r = cluster_prep._Rounds()
        assert ctx._L.fclu_round_results(ctx._h, ctypes.byref(r)) == 0 and r.n_prob == len(problems)
        assert cluster_prep._copy_out(r.inf_seg, int(r.n_inf), np.int32).tolist() == arr["inf_seg"].tolist()
        assert cluster_prep._copy_out(r.rows, 3 * int(r.n_gap_rows), np.int32).tolist() == arr["rows"].reshape(-1).tolist()
        i = cluster_prep._Incumbents()
        assert ctx._L.fclu_round_incumbent_results(ctx._h, ctypes.byref(i)) == 0 and i.n_prob == len(problems)
        assert cluster_prep._copy_out(i.cost2, i.n_prob, np.int64).tolist() == inc["cost2"].tolist()
        assert cluster_prep._copy_out(i.mem, int(i.n_mem), np.int32).tolist() == inc["mem"].tolist()
        compare(ctx, tints, part0, problems, 3, resident=True, node_cap=7)


def test_refusals(ctx):
    """passes outside 1 .. 16 is refused on the host, before any launch, and the context stays usable."""
    tints = [flips_tint(0, 66, 44), flips_tint(1, 5, 12)]
    part0 = stage(ctx, tints)
    problems = whole(tints)
    compare(ctx, tints, part0, problems, 2)
    g2, ub2 = np.full(71, 6, np.int32), np.full(2, -1, np.int64)
    for passes in (0, 17, -1, 1 << 20):
        assert ctx._L.fclu_round_bnb_wide_passes(ctx._h, g2.ctypes.data, ub2.ctypes.data, 0.8, 1.2, 20, 1, 1024, 6, 64, BIG, passes) == 1     # FCLU_ERR_ARG
        assert b"passes" in ctx._L.fclu_last_error(ctx._h)
        rows = np.zeros((16, 5), np.int64)
        assert ctx._L.fclu_round_bnb_wide_pass_stats(ctx._h, rows.ctypes.data, 16) == 1                 # (a failed call leaves no result)
    for passes in (0, 17):
        with pytest.raises(cluster_prep.ClusterError, match="passes") as e:
            ctx.round_bnb_wide([3.0] * 71, [-1, -1], 0.2, 20, 1, 1024, BIG, passes=passes)
        assert e.value.code == 1
    assert ctx._L.fclu_round_bnb_wide_passes(ctx._h, g2.ctypes.data, ub2.ctypes.data, 0.8, 1.2, 20, 1, 1024, 6, 0, BIG, 2) == 1 and \
        b"node_cap" in ctx._L.fclu_last_error(ctx._h)
    assert ctx._L.fclu_round_bnb_wide_passes(ctx._h, g2.ctypes.data, ub2.ctypes.data, 0.8, 1.2, 20, 1, 1024, 6, 64, BIG, 16) == 0
    assert ctx._L.fclu_round_bnb_wide_pass_stats(ctx._h, None, 0) == 0 and ctx._L.fclu_round_bnb_wide_pass_stats(ctx._h, None, 3) == 1
    assert ctx._L.fclu_round_bnb_wide_pass_stats(ctx._h, None, -1) == 1
    compare(ctx, tints, part0, problems, 2)


class CappedContext:
    """The device context with round_bnb_wide() held to a small depth and node cap, so that the loop's searches need their passes."""

    def __init__(self, ctx, depth, node_cap):
        self._ctx, self.depth, self.node_cap, self.passes_seen, self.rows = ctx, depth, node_cap, [], []

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def round_bnb_wide(self, garbage, ub2, epsilon, offset, min_cols, max_cols, max_nodes, depth=None, node_cap=None, passes=1):
        self.passes_seen.append(passes)
        out = self._ctx.round_bnb_wide(garbage, ub2, epsilon, offset, min_cols, max_cols, max_nodes, self.depth, self.node_cap, passes)
        self.rows.append(self._ctx.round_bnb_wide_pass_stats())
        return out


def test_the_loop_with_three_passes_on_a_partition_of_70_reps(ctx, monkeypatch):
    """cluster_tints() under wide_cols = 128 and wide_passes = 3 on a staged tint whose one partition holds 72 reps, the searches held to
    depth 2 and 40 nodes a task: the records, the logs and the isoforms are those of the loop through the stand-in context whose
    round_bnb_wide() is the mirror, and the first round is proven by the passes, not by the first."""
    tints = [family_tint(0, 70, 6)[0]]
    part0 = stage(ctx, tints)
    assert len(tints[0]["partitions"]) == 1 and len(tints[0]["partitions"][0][0]) == 72
    host = copy.deepcopy(tints)
    settings = cluster.ilp_settings(min_isoform_size=2, wide_cols=128, wide_passes=3)
    runs = []
    for which, ts in (("device", tints), ("mirror", host)):
        c = CappedContext(ctx, 2, 40) if which == "device" else PassesContext(ts, part0, 2, 40)
        if which == "mirror":
            monkeypatch.setattr(cluster_prep, "round_model", lambda arr, p: arr.model(p))
        record, jobs = [], []
        logs = cluster.cluster_tints(ts, part0, c, settings, solve=lambda m, s: jobs.append(m["n_cols"]) or cluster_solve.solve_round(m, s),
                                     on_round=lambda r: record.append((r["partition"], r["round"], r["remaining"], r["status"], r["x"], r["e"], r["cost"])))
        runs.append((logs, record, jobs, [(t["isoforms"], t["garbage_rids"]) for t in ts]))
        if which == "device":
            assert set(c.passes_seen) == {3} and len(c.rows[0]) > 1 and c.rows[0][0]["capped"] > 0
    assert runs[0] == runs[1] and runs[0][1][0][3] == "OPTIMAL" and len(runs[0][1][0][4]) == 72
