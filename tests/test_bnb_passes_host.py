"""The passes of the wide branch and bound without a GPU: cluster_solve.exact_bnb_wide(passes=..., max_tasks=...) -- the definition of
fclu_round_bnb_wide_passes -- with one pass against the single search, with enough passes against exact_small(), with too few; that the
cases really split tasks; the measured task counts of a family; the tie under a bound that equals its optimum; the budget rules; the
settings and the flag; the loop through a stand-in context whose round_bnb_wide() is the mirror behind the library's rule of which
problems a pass continues (device_passes(), which the GPU tests hold the device to as well); and the kernels' code on the host."""
import os
import subprocess
import sys

import numpy as np
import pytest

from freddie_amd import cluster, cluster_prep, cluster_solve
from test_bnb_wide_host import WideContext, run_wide_loop
from test_incumbent_host import loop_tints
from test_round_host import model_of, small_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bnb_host_check import family_model, greedy2  # noqa: E402
from bnb_wide_host_check import bare_model, tie_model  # noqa: E402

ENOUGH = 10 ** 6
DEPTH_CAP = ((0, 1), (1, 2), (2, 3), (3, 7))


def single(model, settings, ub2, depth, node_cap):
    """The search as it was before the passes: every task of the 2^D once, by bnb_task(), and the result rule."""
    tb = cluster_solve.bnb_tables(model, settings, cluster_solve.BNB_WIDE_MAX_COLS, "exact_bnb_wide")
    D = min(tb["R"], depth)
    tasks = [cluster_solve.bnb_task(tb, t, D, ub2, node_cap) for t in range(1 << D)]
    found = [(c, m) for c, m, _, _ in tasks if c >= 0]
    capped = sum(cap for _, _, _, cap in tasks)
    status = "unproven" if capped or (not found and ub2 is not None) else "optimal" if found else "infeasible"
    return status, min(found) if found else None, sum(n for _, _, n, _ in tasks), capped


def grid():
    """(model, settings) of every unrefused grid case: small_case() of the seeds 1 .. 40, gaps and pairs on and off, all three recycle models."""
    for seed in range(1, 41):
        for with_gaps, with_pairs in ((False, False), (True, False), (False, True), (True, True)):
            tint, incomp = small_case(seed, 6 + seed % 7, 5 + seed % 9, with_gaps, with_pairs)
            for recycle in cluster_solve.RECYCLE_MODELS:
                settings = cluster.ilp_settings(recycle)
                model = model_of(tint, incomp, list(range(6 + seed % 7)), settings)
                if model["refused"] is None:
                    yield model, settings


@pytest.fixture(scope="module")
def grid_cases():
    """The grid with each case's exact_small() and greedy bound, computed once."""
    return [(model, settings, cluster_solve.exact_small(model, settings), greedy2(model, settings)) for model, settings in grid()]


def test_one_pass_is_the_single_search(grid_cases):
    """passes = 1 (and the default) returns the search of before on the grid and the families, key for key, and pass_stats has its one row."""
    n = 0
    for k, (model, settings, _, bound) in enumerate(grid_cases):
        depth, node_cap = DEPTH_CAP[k % 4]
        for ub2 in (None, bound):
            status, best, nodes, capped = single(model, settings, ub2, depth, node_cap)
            got = cluster_solve.exact_bnb_wide(model, settings, ub2, depth, node_cap, passes=1)
            assert got == cluster_solve.exact_bnb_wide(model, settings, ub2, depth, node_cap) == cluster_solve.exact_bnb(model, settings, ub2, depth, node_cap)
            assert (got["status"], got["nodes"], got["capped"]) == (status, nodes, capped)
            assert (None if got["mask"] is None else (got["cost2"], got["mask"])) == best
            assert got["pass_stats"] == [dict(tasks=1 << min(model["n_cols"], depth), nodes=nodes, capped=capped, min_len=min(model["n_cols"], depth),
                                              max_len=min(model["n_cols"], depth))]
            n += 1
    assert n > 700
    for R, n_low in ((33, 32), (65, 32), (129, 128)):
        model, settings = family_model(R, n_low)[0], cluster.ilp_settings()
        for ub2, depth, node_cap in ((greedy2(model, settings), 6, 4096), (None, 3, 64)):
            status, best, nodes, capped = single(model, settings, ub2, depth, node_cap)
            got = cluster_solve.exact_bnb_wide(model, settings, ub2, depth, node_cap, passes=1, max_tasks=1)
            assert (got["status"], got["cost2"], got["mask"], got["nodes"], got["capped"]) == (status, best and best[0], best and best[1], nodes, capped)


def test_enough_passes_reach_exact_small_and_too_few_do_not(grid_cases):
    """Every grid case, bounded by the greedy and not, at (depth, cap) = (0, 1), (1, 2), (2, 3) and (3, 7): with enough passes the search
    ends with exact_small()'s (cost2, mask) and the right status, no task open, the nodes the passes' sum; with one pass fewer than it
    took it is unproven with a set no cheaper than the optimum.  And the cases exercise the feature: more than half take more than one
    pass, some prefix has L = R."""
    runs = more = full_len = 0
    for model, settings, exact, bound in grid_cases:
        R = model["n_cols"]
        for ub2 in (None, bound):
            for depth, node_cap in DEPTH_CAP:
                got = cluster_solve.exact_bnb_wide(model, settings, ub2, depth, node_cap, passes=ENOUGH)
                stats = got["pass_stats"]
                assert got["capped"] == 0 and stats[-1]["capped"] == 0 and got["nodes"] == sum(s["nodes"] for s in stats)
                assert all(a["capped"] > 0 and b["tasks"] >= 1 and b["min_len"] > a["min_len"] for a, b in zip(stats, stats[1:]))
                if exact is None:                            # no subset is feasible
                    assert (got["status"], got["mask"]) == ("infeasible" if ub2 is None else "unproven", None)
                else:
                    assert ub2 is None or ub2 >= exact["cost2"]
                    assert (got["status"], got["cost2"], got["mask"], got["x"], got["e"]) == ("optimal", exact["cost2"], exact["mask"], exact["x"], exact["e"])
                runs += 1
                more += len(stats) > 1
                full_len += any(s["max_len"] == R for s in stats[1:])
                if len(stats) > 1:
                    few = cluster_solve.exact_bnb_wide(model, settings, ub2, depth, node_cap, passes=len(stats) - 1)
                    assert few["status"] == "unproven" and few["capped"] == stats[-2]["capped"] and few["pass_stats"] == stats[:-1]
                    assert few["mask"] is None or (exact is not None and (few["cost2"], few["mask"]) >= (exact["cost2"], exact["mask"]))
    assert runs > 3000 and 2 * more > runs and full_len


def test_a_task_is_split_at_its_top_level_with_both_children_open():
    """A task capped in front of an include child leaves that child and the exclude child of the same level, and the exclude children of
    the levels under it that it entered by their include child; capped in front of an exclude child, that child alone."""
    both = one = 0
    for model, settings in list(grid())[:60]:
        tb = cluster_solve.bnb_tables(model, settings, cluster_solve.BNB_WIDE_MAX_COLS)
        for node_cap in (1, 2, 3, 7):
            cost2, mask, nodes, capped, opened = cluster_solve.bnb_prefix_task(tb, 0, 0, None, node_cap)
            assert bool(opened) == capped and (not capped or nodes == node_cap)
            if capped:
                top = max(L for _, L in opened)
                at_top = [P for P, L in opened if L == top]
                assert len(at_top) in (1, 2) and all(P >> L == 0 for P, L in opened) and len(set(opened)) == len(opened)
                if len(at_top) == 2:
                    assert sorted(at_top) == [at_top[1], at_top[1] | 1 << (top - 1)] and at_top[0] == at_top[1] | 1 << (top - 1)
                both += len(at_top) == 2
                one += len(at_top) == 1
    assert both and one
    tb = cluster_solve.bnb_tables(bare_model(3), cluster.ilp_settings(), cluster_solve.BNB_WIDE_MAX_COLS)
    assert cluster_solve.bnb_prefix_task(tb, 0, 0, None, 1)[4] == [(1, 1), (0, 1)]
    assert cluster_solve.bnb_prefix_task(tb, 0, 0, None, 3)[4] == [(0, 1), (1, 2), (7, 3), (3, 3)]      # (the children at the top are leaves: L = R)
    assert cluster_solve.bnb_prefix_task(tb, 5, 3, None, 1) == (3, 5, 1, False, [])                       # a prefix of L = R is a leaf
    assert cluster_solve.bnb_task(tb, 1, 1, None, 2) == cluster_solve.bnb_prefix_task(tb, 1, 1, None, 2)[:4]


def test_the_measured_task_counts_of_a_family():
    """family_model(65, 32) at depth 2, 40 nodes a task, no bound: the passes hold 4, 124, 1 796 and 1 tasks and 6 883 nodes in all."""
    model, settings = family_model(65, 32)[0], cluster.ilp_settings()
    got = cluster_solve.exact_bnb_wide(model, settings, None, 2, 40, passes=4)
    assert [s["tasks"] for s in got["pass_stats"]] == [4, 124, 1796, 1] and got["nodes"] == 6883 and got["status"] == "unproven"
    assert got["pass_stats"][0] == dict(tasks=4, nodes=160, capped=4, min_len=2, max_len=2) and got["pass_stats"][2]["max_len"] == 65
    done = cluster_solve.exact_bnb_wide(model, settings, None, 2, 40, passes=16)
    want = cluster_solve.exact_bnb_wide(model, settings, None, 2, 1 << 20)
    assert want["capped"] == 0 and (done["status"], done["cost2"], done["mask"]) == ("optimal", want["cost2"], want["mask"]) and len(done["pass_stats"]) > 4


def test_the_lower_set_wins_the_tie_under_a_bound_that_equals_the_optimum():
    """tie_model(), 128 columns with two optimal sets, bounded by exactly their cost, 64 nodes a task: every pass starts at that bound, a
    leaf of equal cost is still taken, and the smaller mask -- the columns 0 .. 63 -- wins over the passes."""
    model, _, _ = tie_model()
    settings = cluster.ilp_settings()
    want = cluster_solve.exact_bnb_wide(model, settings, None, 6, 1 << 20)
    assert want["status"] == "optimal" and want["mask"] == (1 << 64) - 1
    got = cluster_solve.exact_bnb_wide(model, settings, want["cost2"], 2, 64, passes=ENOUGH)
    assert len(got["pass_stats"]) > 1 and (got["status"], got["cost2"], got["mask"], got["capped"]) == ("optimal", want["cost2"], (1 << 64) - 1, 0)
    assert cluster_solve.exact_bnb_wide(model, settings, want["cost2"] - 1, 2, 64, passes=ENOUGH)["status"] == "unproven"     # nothing is cheaper


def test_the_budget_rules():
    """max_tasks: a pass that would hold more tasks is not run and the problem stays as it is.  device_passes(): the first problem whose
    pass does not fit the node budget ends the taking for this and every later pass."""
    settings = cluster.ilp_settings()
    model = family_model(65, 32)[0]
    full = cluster_solve.exact_bnb_wide(model, settings, None, 2, 40, passes=3)
    for max_tasks, n in ((123, 1), (124, 2), (1795, 2), (1796, 3)):
        got = cluster_solve.exact_bnb_wide(model, settings, None, 2, 40, passes=3, max_tasks=max_tasks)
        assert got["pass_stats"] == full["pass_stats"][:n] and got["status"] == "unproven" and got["capped"] == full["pass_stats"][n - 1]["capped"]
    with pytest.raises(ValueError, match="at least 1"):
        cluster_solve.exact_bnb_wide(model, settings, None, 2, 40, passes=0)
    with pytest.raises(ValueError, match="at least 1"):
        cluster_solve.exact_bnb_wide(model, settings, None, 2, 40, passes=2, max_tasks=0)
    # three problems of 7, 6 and 8 columns at depth 1 and one node a task: a task leaves two children, so pass 2 holds 4 tasks each and pass 3 8
    models = [bare_model(R) for R in (7, 6, 8)]
    ub2 = [-1, -1, -1]
    every, rows, taken = device_passes(models, settings, ub2, 1, 64, 1, 1, 1 << 30, 2)
    assert taken == 3 and [r["tasks"] for r in rows] == [6, 12] and [r["problems"] for r in rows] == [3, 3]
    some, rows, taken = device_passes(models, settings, ub2, 1, 64, 1, 1, 8, 3)       # pass 2: the 6 and the 7 columns; pass 3: the 6 alone
    assert taken == 3 and [(r["tasks"], r["problems"]) for r in rows] == [(6, 3), (8, 2), (8, 1)]
    assert some[0] == every[0] and some[1]["nodes"] == 2 + 4 + 8 and some[2] != every[2] and some[2]["nodes"] == cluster_solve.exact_bnb_wide(models[2], settings, None, 1, 1)["nodes"] == 2
    assert device_passes(models, settings, ub2, 1, 64, 1, 1, 2, 3)[1:] == ([dict(tasks=2, nodes=2, capped=2, problems=1, min_len=1, max_len=1)], 1)
    lone, rows, taken = device_passes(models[:1], settings, ub2[:1], 1, 64, 1, 1, 1 << 30, 3, max_tasks=2)     # beyond max_tasks: not continued
    assert [r["tasks"] for r in rows] == [2] and lone[0]["capped"] == 2
    assert cluster_prep.BNB_WIDE_MAX_PASS_TASKS == 1 << 16 and cluster_prep.BNB_WIDE_MAX_PASSES == cluster.WIDE_MAX_PASSES == 16


def device_passes(models, settings, ub2, min_cols, max_cols, depth, node_cap, max_nodes, passes, max_tasks=cluster_prep.BNB_WIDE_MAX_PASS_TASKS):
    """fclu_round_bnb_wide_passes' rule (include/freddie_cluster.h) on the mirror: (per problem None (refused or not taken) or
    exact_bnb_wide()'s dict without the solution's lists; the rows of round_bnb_wide_pass_stats() without the launches, with the range of
    the pass's prefix lengths; problems taken).
    Pass 1 takes the problems with a model, inside the sizes, whose tables fit, in ascending (columns, problem) inside the budget; a later
    pass the problems of the pass before, in that order, that have 1 .. max_tasks open children, while the running total of children x
    node_cap stays inside the budget -- the first that does not fit ends the taking, for good."""
    fits = lambda m: cluster_prep.bnb_wide_lds_bytes(m["n_cols"], len(m["inf_seg"])) <= cluster_prep.BNB_WIDE_LDS_BYTES
    state, current, total = {}, [], 0
    for R, p in sorted((m["n_cols"], p) for p, m in enumerate(models) if m.get("refused") is None and min_cols <= m["n_cols"] <= max_cols and fits(m)):
        if total + (node_cap << min(R, depth)) > max_nodes:
            break
        total += node_cap << min(R, depth)
        tb = cluster_solve.bnb_tables(models[p], settings, cluster_solve.BNB_WIDE_MAX_COLS, "exact_bnb_wide")
        D = min(R, depth)
        state[p] = dict(tb=tb, ub2=None if ub2[p] < 0 else int(ub2[p]), tasks=[(t, D) for t in range(1 << D)], best=None, nodes=0, capped=0)
        current.append(p)
    n_taken, rows = len(current), []
    for k in range(passes):
        if k:
            cand, current, total = [p for p in current if 0 < len(state[p]["tasks"]) <= max_tasks], [], 0
            for p in cand:
                if total + len(state[p]["tasks"]) * node_cap > max_nodes:
                    break
                total += len(state[p]["tasks"]) * node_cap
                current.append(p)
        if not current:
            break
        row = dict(tasks=0, nodes=0, capped=0, problems=len(current), min_len=1 << 20, max_len=0)
        for p in current:
            s = state[p]
            one = cluster_solve.bnb_pass(s["tb"], s["tasks"], cluster_solve.bnb_pass_bound(s["ub2"], s["best"]), node_cap)
            if one["best"] is not None and (s["best"] is None or one["best"] < s["best"]):
                s["best"] = one["best"]
            row["tasks"] += len(s["tasks"])
            row["nodes"] += one["nodes"]
            row["capped"] += one["capped"]
            row["min_len"], row["max_len"] = min(row["min_len"], one["stats"]["min_len"]), max(row["max_len"], one["stats"]["max_len"])
            s["nodes"], s["capped"], s["tasks"] = s["nodes"] + one["nodes"], one["capped"], one["opened"]
        rows.append(row)
    want = [None] * len(models)
    for p, s in state.items():
        status = "unproven" if s["capped"] or (s["best"] is None and s["ub2"] is not None) else "optimal" if s["best"] is not None else "infeasible"
        want[p] = dict(status=status, cost2=s["best"] and s["best"][0], mask=s["best"] and s["best"][1], nodes=s["nodes"], capped=s["capped"])
    return want, rows, n_taken


def test_device_passes_is_the_mirror_where_nothing_is_cut():
    """With room for everything device_passes() gives each problem exact_bnb_wide(passes=...)'s result."""
    settings = cluster.ilp_settings()
    models = [family_model(65, 32)[0], bare_model(9), family_model(33, 32)[0]]
    ub2 = [greedy2(models[0], settings), -1, -1]
    for passes in (1, 2, 5):
        want, rows, taken = device_passes(models, settings, ub2, 1, 1024, 2, 25, 1 << 40, passes)
        assert taken == 3 and len(rows) <= passes
        for p, m in enumerate(models):
            one = cluster_solve.exact_bnb_wide(m, settings, None if ub2[p] < 0 else ub2[p], 2, 25, passes=passes, max_tasks=1 << 16)
            assert want[p] == {k: one[k] for k in ("status", "cost2", "mask", "nodes", "capped")}
        assert sum(r["nodes"] for r in rows) == sum(w["nodes"] for w in want)


def test_settings_and_cli_flag(tmp_path):
    settings = cluster.ilp_settings()
    assert settings["wide_passes"] == 1
    cluster.check_wide(settings)
    cluster.check_wide({})                                   # (settings from before the feature)
    for passes in (1, 2, 16):
        cluster.check_wide(cluster.ilp_settings(wide_cols=300, wide_passes=passes))
    for passes in (0, 17, -1, 2.5, None):
        with pytest.raises(ValueError, match="wide_passes"):
            cluster.check_wide(cluster.ilp_settings(wide_cols=300, wide_passes=passes))
    base = ["-s", str(tmp_path)]
    assert cluster.parse_args(base).wide_passes == 1
    for k in (1, 3, 16):
        assert cluster.parse_args(base + ["--exact-wide", "400", "--wide-passes", str(k)]).wide_passes == k
    for bad in ("0", "17", "-1", "x"):
        with pytest.raises(SystemExit):
            cluster.parse_args(base + ["--wide-passes", bad])


class PassesContext(WideContext):
    """WideContext whose round_bnb_wide() takes passes: device_passes() on the round's problems."""

    def round_bnb_wide(self, garbage, ub2, epsilon, offset, min_cols, max_cols, max_nodes, depth=None, node_cap=None, passes=1):
        self.wide_calls += 1
        self.wide_args.append((min_cols, max_cols, max_nodes, passes))
        col_off = np.cumsum([0] + [len(rem) for _, rem in self.problems])
        P = len(self.problems)
        models = []
        for p, (q, rem) in enumerate(self.problems):
            tint = self.tints[max(k for k in range(len(self.part0)) if self.part0[k] <= q)]
            models.append(dict(self.model(p), garbage=list(garbage[col_off[p]:col_off[p + 1]]), max_lg=sum(s[2] for s in tint["segs"]), refused=None))
        want, self.rows, _ = device_passes(models, dict(epsilon=epsilon, offset=offset), ub2, min_cols, max_cols, self.depth, self.node_cap, max_nodes, passes)
        status, cost2, mask = [-2] * P, [-1] * P, np.zeros((P, 16), np.uint64)
        for p, w in enumerate(want):
            if w is not None:
                status[p] = ("optimal", "infeasible", "unproven").index(w["status"])
                if w["mask"] is not None:
                    cost2[p] = w["cost2"]
                    for i in range(16):
                        mask[p, i] = w["mask"] >> (64 * i) & (2 ** 64 - 1)
                self.results.append((self.problems[p][0], tuple(self.problems[p][1]), w))
        return dict(n_prob=P, col_off=col_off, status=np.array(status, np.int32), cost2=np.array(cost2, np.int64), mask=mask)


def run_passes_loop(monkeypatch, depth, node_cap, settings):
    tints, part0 = loop_tints()
    ctx = PassesContext(tints, part0, depth, node_cap)
    monkeypatch.setattr(cluster_prep, "round_model", lambda arr, p: arr.model(p))
    record, jobs = [], []

    def solve(model, s):
        jobs.append((model["key"], model["n_cols"], model.get("incumbent")))
        return cluster_solve.solve_round(model, s)

    logs = cluster.cluster_tints(tints, part0, ctx, settings, solve=solve, on_round=record.append)
    return ctx, logs, record, jobs


def test_the_loop_hands_the_passes_on(monkeypatch):
    """wide_passes = 1 (and settings that do not know it) call round_bnb_wide() without the argument -- WideContext's has none -- and give
    the calls, logs and records of before.  With 4 nodes a task at depth 2 the single search leaves problems to the solver; wide_passes = 8
    proves them all on the stand-in, no solve job is made, and the records are those of the run with room to finish."""
    base = dict(min_isoform_size=2)
    plain = run_wide_loop(monkeypatch, 2, 4, cluster.ilp_settings(wide_cols=12, **base))
    one = run_wide_loop(monkeypatch, 2, 4, cluster.ilp_settings(wide_cols=12, wide_passes=1, **base))
    old = run_wide_loop(monkeypatch, 2, 4, {k: v for k, v in cluster.ilp_settings(wide_cols=12, **base).items() if k != "wide_passes"})
    for ctx, logs, record, jobs in (one, old):
        assert (ctx.wide_calls, ctx.wide_args, logs, jobs) == (plain[0].wide_calls, plain[0].wide_args, plain[1], plain[3]) and jobs
        assert [(r["status"], r["cost"], r["x"]) for r in record] == [(r["status"], r["cost"], r["x"]) for r in plain[2]]
    ctx, logs, record, jobs = run_passes_loop(monkeypatch, 2, 4, cluster.ilp_settings(wide_cols=12, wide_passes=8, **base))
    assert not jobs and ctx.wide_calls and set(ctx.wide_args) == {(1, 12, cluster.WIDE_NODES, 8)}
    assert all(w["status"] == "optimal" for _, _, w in ctx.results)
    roomy = run_wide_loop(monkeypatch, 12, 4096, cluster.ilp_settings(wide_cols=12, **base))
    assert not roomy[3] and logs == roomy[1]
    assert [(r["status"], r["cost"], r["x"], r["remaining"]) for r in record] == [(r["status"], r["cost"], r["x"], r["remaining"]) for r in roomy[2]]


def test_kernel_bodies_on_the_host():
    """The walk on a prefix, the roll-back and the open children (freddie_amd/csrc/clu_bnb_wide.h), compiled for the host with the address
    and undefined-behaviour sanitizers and run pass by pass, the lanes of a wave one after another, against the mirror: E = 0 and
    prefixes of L = R among the cases."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bnb_passes_host_check.py")], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and " 0 differ" in res.stdout, res.stdout + res.stderr
