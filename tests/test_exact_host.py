"""The exact small-problem solve without a GPU: the Python mirror (cluster_solve.exact_small, the definition the device reproduces)
against the brute force on the grid of small problems -- cost, infeasibility, the tie rule --, against the greedy incumbent, on the
epsilon 0.15 boundary row, its argument errors; the loop (cluster_tints) through a stand-in context whose round_exact() is the mirror;
the command line's flags; the kernels' per-thread code on the host."""
import os
import subprocess
import sys

import numpy as np
import pytest

import round_util as ru
from freddie_amd import cluster, cluster_prep, cluster_solve
from test_incumbent_host import FLAVOURS, MirrorContext, grid, loop_tints
from test_round_host import model_of, small_case


@pytest.mark.parametrize("recycle_model", cluster_solve.RECYCLE_MODELS)
def test_mirror_reaches_the_brute_force_cost_and_the_smallest_optimal_mask(recycle_model):
    """On the grid's 132 feasible cases: the cost is the smallest over the feasible subsets (round_util.subset_cost) and the mask the
    smallest among the optimal ones.  Cases with more than one optimal subset: constant 25, exons 17, introns 37."""
    settings = cluster.ilp_settings(recycle_model)
    cases = grid()
    assert len(cases) == 132
    ties = 0
    for tint, incomp, remaining, feasible in cases:
        model = model_of(tint, incomp, remaining, settings)
        garbage = model["garbage"]
        costs = {mask: corr + sum(g for c, g in enumerate(garbage) if not mask >> c & 1) for mask, corr in feasible.items()}
        best = min(costs.values())
        optimal = sorted(mask for mask, cost in costs.items() if cost == best)
        ties += len(optimal) > 1
        got = cluster_solve.exact_small(model, settings)
        assert got is not None and got["cost"] == best and got["cost2"] == 2 * best, (tint["id"], got, best)
        assert got["mask"] == optimal[0], (tint["id"], got["mask"], optimal)
        n = len(remaining)
        assert got["x"] == [got["mask"] >> c & 1 for c in range(n)] and got["members"] == [c for c in range(n) if got["x"][c]]
        assert got["e"] == [int(any(got["x"][c] for c in support)) for support in model["support"]]
        assert cluster_solve.round_cost(model, got["x"], got["e"]) == best
        assert ru.subset_cost(tint, incomp, remaining, set(got["members"]), settings) == best
    print("%s: %d of %d cases have more than one optimal subset" % (recycle_model, ties, len(cases)))
    assert ties >= 10


def test_mirror_has_no_result_exactly_where_the_brute_force_has_none():
    """The grid's 160 cases: 4 are refused, 24 have no feasible subset (feasibility does not depend on the recycle model)."""
    content = lambda tint, incomp: (tint["id"], repr([(r["data"], r["gaps"]) for r in tint["reads"]]), repr(incomp))   # (what feasibility depends on)
    kept = {content(t, inc) for t, inc, _, _ in grid()}
    refused = infeasible = 0
    for seed in range(1, 41):
        n, M = 6 + seed % 7, 5 + seed % 9
        for with_gaps, with_pairs in FLAVOURS:
            tint, incomp = small_case(seed, n, M, with_gaps, with_pairs)
            remaining = list(range(n))
            if ru.restate(tint, incomp, remaining)["refused"] is not None:
                refused += 1
                continue
            if content(tint, incomp) in kept:
                continue                                     # (a case of grid(): feasible, and checked above)
            brute = ru.brute_force(tint, incomp, remaining, cluster.ilp_settings())
            for recycle_model in cluster_solve.RECYCLE_MODELS:
                settings = cluster.ilp_settings(recycle_model)
                assert (cluster_solve.exact_small(model_of(tint, incomp, remaining, settings), settings) is None) == (brute is None)
            infeasible += brute is None
    assert (refused, infeasible) == (4, 24)


@pytest.mark.parametrize("recycle_model", cluster_solve.RECYCLE_MODELS)
def test_exact_is_never_worse_than_the_greedy(recycle_model):
    settings = cluster.ilp_settings(recycle_model)
    both = 0
    for seed in range(1, 41):
        n, M = 6 + seed % 7, 5 + seed % 9
        for with_gaps, with_pairs in FLAVOURS:
            tint, incomp = small_case(seed, n, M, with_gaps, with_pairs)
            remaining = list(range(n))
            model = model_of(tint, incomp, remaining, settings)
            if model["refused"] is not None:
                continue
            greedy, exact = cluster_solve.greedy_incumbent(model, settings), cluster_solve.exact_small(model, settings)
            if greedy is not None:
                assert exact is not None and exact["cost2"] <= greedy["cost2"]
                both += 1
    assert both >= 100


def boundary_model(l):
    """Two columns over three segments; column 0 has a gap (0, 2) of length l whose group is segment 1, 200 long, which only column 1
    covers.  {0, 1} costs one correction if column 0's row holds at G = 200; {0} alone never holds (20 < l); {1} costs column 0's garbage."""
    return dict(n_cols=2, inf_seg=[0, 1, 2], support=[[0, 1], [1], [0, 1]], corrections=[[1], []], pairs=[], groups=[(0, 2)],
                group_segs=[[(1, 200)]], gap_rows=[(0, 0, l)], garbage=[50.0, 50.0], max_lg=400)


def test_the_boundary_row_is_feasible():
    """epsilon 0.15, offset 20, G = 200: 1.15 x 200 + 20 = 250 in rationals and less in doubles; the model's tolerance admits l = 250."""
    assert 1.15 * 200 + 20 < 250
    settings = cluster.ilp_settings(epsilon=0.15)
    got = cluster_solve.exact_small(boundary_model(250), settings)
    assert (got["cost2"], got["mask"], got["members"], got["e"]) == (2, 3, [0, 1], [1, 1, 1])
    got = cluster_solve.exact_small(boundary_model(251), settings)
    assert (got["cost2"], got["mask"]) == (100, 2)
    assert cluster_solve.exact_small(boundary_model(250 + 20 + 400 + 1), settings) is None      # beyond the slack of a column outside, too


def test_mirror_arguments():
    tint, incomp = small_case(3, 8, 9, True, True)
    settings = cluster.ilp_settings()
    model = model_of(tint, incomp, list(range(8)), settings)
    with pytest.raises(ValueError, match="multiple of 0.5"):
        cluster_solve.exact_small(dict(model, garbage=[3.25] * 8), settings)
    with pytest.raises(ValueError, match="multiple of 0.5"):
        cluster_solve.exact_small(dict(model, garbage=[-1.0] * 8), settings)
    with pytest.raises(ValueError, match="8 columns"):
        cluster_solve.exact_small(dict(model, garbage=[3.0] * 7), settings)
    wide = dict(n_cols=25, inf_seg=[], support=[], corrections=[[]] * 25, pairs=[], groups=[], group_segs=[], gap_rows=[], garbage=[1.0] * 25, max_lg=0)
    with pytest.raises(ValueError, match="24 at the most"):
        cluster_solve.exact_small(wide, settings)
    empty = cluster_solve.exact_small(model_of(tint, incomp, [], settings), settings)
    assert (empty["cost2"], empty["mask"], empty["members"], empty["x"]) == (0, 0, [], [])
    small = cluster_solve.exact_small(model, settings, chunk=7)                   # (the chunks are an implementation detail)
    assert small == cluster_solve.exact_small(model, settings)
    with pytest.raises(ValueError, match="exact_cols"):
        cluster.check_exact(cluster.ilp_settings(exact_cols=25))
    with pytest.raises(ValueError, match="exact_masks"):
        cluster.check_exact(cluster.ilp_settings(exact_cols=3, exact_masks=0))


class ExactContext(MirrorContext):
    """MirrorContext with a round_exact() that is the mirror behind the library's rule of which problems are taken."""

    def __init__(self, tints, part0):
        MirrorContext.__init__(self, tints, part0)
        self.exact_calls, self.taken = 0, 0

    def round_exact(self, garbage, epsilon, offset, max_cols, max_masks):
        self.exact_calls += 1
        col_off = np.cumsum([0] + [len(rem) for _, rem in self.problems])
        assert len(garbage) == col_off[-1]
        cost2, mask, total = [-2] * len(self.problems), [0] * len(self.problems), 0
        for R, p in sorted((len(rem), p) for p, (_, rem) in enumerate(self.problems)):
            if R > max_cols or total + (1 << R) > max_masks:
                break
            total += 1 << R
            q = self.problems[p][0]
            tint = self.tints[max(k for k in range(len(self.part0)) if self.part0[k] <= q)]
            got = cluster_solve.exact_small(dict(self.model(p), garbage=list(garbage[col_off[p]:col_off[p + 1]]), max_lg=sum(s[2] for s in tint["segs"])),
                                            dict(epsilon=epsilon, offset=offset))
            cost2[p], mask[p] = (-1, 0) if got is None else (got["cost2"], got["mask"])
            self.taken += 1
        return dict(n_prob=len(cost2), col_off=col_off, cost2=np.array(cost2, np.int64), mask=np.array(mask, np.uint32))


def run_exact_loop(monkeypatch, tints, part0, solve, **settings):
    ctx = ExactContext(tints, part0)
    monkeypatch.setattr(cluster_prep, "round_model", lambda arr, p: arr.model(p))
    record = []
    logs = cluster.cluster_tints(tints, part0, ctx, cluster.ilp_settings(min_isoform_size=2, **settings), solve=solve, on_round=record.append)
    return ctx, logs, record


def solver_for_more_than(n_cols, calls):
    def solve(model, settings):
        assert model["n_cols"] > n_cols, "a model of %d columns reached the solver" % model["n_cols"]
        calls.append(model["n_cols"])
        return cluster_solve.solve_round(model, settings)
    return solve


def test_loop_solves_small_problems_without_the_solver(monkeypatch):
    """Partitions of 4 .. 6 reps: with exact_cols = 12 the solver is never called, with 4 only for the larger models, with 0 always and
    round_exact() never; every round's cost is the brute force's whichever way it was solved."""
    key = lambda r: (r["tint"]["id"], r["partition"], r["round"])
    costs = {}
    for exact_cols in (12, 4, 0):
        tints, part0 = loop_tints()
        calls = []
        ctx, logs, record = run_exact_loop(monkeypatch, tints, part0, solver_for_more_than(exact_cols, calls), exact_cols=exact_cols)
        assert record and all(l[0] == "OPTIMAL" for lines in logs for l in lines)
        rounds = len(set(r["round"] for r in record))
        if exact_cols == 12:
            assert not calls and ctx.exact_calls == rounds and ctx.taken == len(record)
        elif exact_cols == 4:
            assert calls and 0 < ctx.taken < len(record) and ctx.exact_calls == rounds
        else:
            assert ctx.exact_calls == 0 and len(calls) == len(record)
        for r in record:
            best = ru.brute_force(r["tint"], r["incomp"], r["remaining"], cluster.ilp_settings())
            assert best is not None and r["status"] == "OPTIMAL" and r["cost"] == best[0], (key(r), r["cost"], best)
            assert ru.subset_cost(r["tint"], r["incomp"], r["remaining"], set(c for c, v in enumerate(r["x"]) if v), cluster.ilp_settings()) == best[0]
        costs[exact_cols] = sorted((key(r), r["cost"]) for r in record if r["round"] == 0)
        assert any(t["isoforms"] for t in tints)
    assert costs[12] == costs[4] == costs[0]


def test_loop_budget_leaves_the_rest_to_the_solver(monkeypatch):
    """A budget of 2^4 + 2^4 masks admits two of the four 4-column problems of the first round and nothing larger."""
    tints, part0 = loop_tints()
    calls = []
    ctx, logs, record = run_exact_loop(monkeypatch, tints, part0, lambda m, s: calls.append(m["n_cols"]) or cluster_solve.solve_round(m, s),
                                       exact_cols=12, exact_masks=32, max_rounds=1)
    sizes = sorted(len(r["remaining"]) for r in record)
    assert ctx.taken == 2 and sorted(calls) == sizes[2:] and sizes[:2] == [4, 4]


def flips_tint(tid, n, M, gaps=None):
    """n reps, all ones, rep i > 0 with a 0 at one of the places 3, 8, ... in turn: a complete graph, one partition."""
    places = list(range(3, M - 3, 5))
    rows = []
    for i in range(n):
        row = [1] * M
        if i:
            row[places[(i - 1) % len(places)]] = 0
        rows.append(row)
    tint = ru.make_tint(tid, rows, gaps)
    cluster_prep.preprocess_ilp(tint, dict(recycle_model="constant"))
    tint["partitions"] = [(list(range(n)), [])]
    return tint


def test_loop_ends_an_infeasible_partition_as_no_solution(monkeypatch):
    """A gap of 500 > offset + MAX_ISOFORM_LG (20 + 213) breaks its rep's row inside and outside the isoform: no subset is feasible."""
    tints = [flips_tint(0, 8, 12, {3: {(2, 9): 500}}), flips_tint(1, 8, 12)]
    assert ru.brute_force(tints[0], [], list(range(8)), cluster.ilp_settings()) is None

    def solve(model, settings):
        raise AssertionError("the solver was called")

    ctx, logs, record = run_exact_loop(monkeypatch, tints, [0, 1], solve, exact_cols=8)
    assert [l[0] for l in logs[0]] == ["NO_SOLUTION"] and logs[0][0][2:] == (0, 0, 8)
    assert [r["status"] for r in record if r["tint"]["id"] == 0] == ["NO_SOLUTION"] and [r["cost"] for r in record if r["tint"]["id"] == 0] == [None]
    assert tints[0]["isoforms"] == [] and tints[0]["garbage_rids"] == list(range(8))
    assert logs[1] and all(l[0] == "OPTIMAL" for l in logs[1]) and tints[1]["isoforms"]


def test_round_exact_solution():
    arr = dict(col_off=np.array([0, 3, 5, 6]), cost2=np.array([7, -1, -2]), mask=np.array([5, 0, 0], np.uint32))
    assert cluster_prep.round_exact_solution(arr, 0) == (3.5, [1, 0, 1])
    assert cluster_prep.round_exact_solution(arr, 1) == "infeasible"
    assert cluster_prep.round_exact_solution(arr, 2) is None


def test_cli_flags(tmp_path):
    base = ["-s", str(tmp_path)]
    args = cluster.parse_args(base)
    assert args.exact_small == 0 and args.exact_masks == cluster.EXACT_MASKS
    for n in (0, 1, 12, 24):
        assert cluster.parse_args(base + ["--exact-small", str(n)]).exact_small == n
    assert cluster.parse_args(base + ["--exact-small", "8", "--exact-masks", "1000"]).exact_masks == 1000
    for bad in (["--exact-small", "25"], ["--exact-small", "-1"], ["--exact-small", "x"], ["--exact-masks", "0"]):
        with pytest.raises(SystemExit):
            cluster.parse_args(base + bad)
    settings = cluster.ilp_settings()
    assert settings["exact_cols"] == 0 and settings["exact_masks"] == cluster.EXACT_MASKS
    assert cluster.ilp_settings(exact_cols=12, exact_masks=5)["exact_cols"] == 12


def test_kernel_bodies_on_the_host():
    """What one thread of k_exact_prep / k_exact_search computes (freddie_amd/csrc/clu_exact.h), compiled for the host with the address
    and undefined-behaviour sanitizers and run over every mask of the grid's problems and of random ones, against the mirror."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, os.path.join(root, "tools", "exact_host_check.py"), "--cases", "60"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and " 0 differ" in res.stdout, res.stdout + res.stderr
