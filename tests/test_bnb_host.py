"""The branch and bound over a round's larger problems without a GPU: the Python mirror (cluster_solve.exact_bnb, the definition the
device reproduces) against the enumeration on the grid of small problems -- cost, mask, infeasibility, the tie rule --, against HiGHS at
28 columns, on built problems whose optimum lies beyond column 31, under a node cap, on the epsilon 0.15 boundary row; the loop
(cluster_tints) through a stand-in context whose round_bnb() is the mirror; the settings and the command line's flags; the kernels'
per-lane code on the host."""
import os
import subprocess
import sys

import numpy as np
import pytest

import round_util as ru
from freddie_amd import cluster, cluster_prep, cluster_solve
from test_exact_host import boundary_model
from test_incumbent_host import FLAVOURS, MirrorContext, grid, loop_tints
from test_round_host import model_of, small_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bnb_host_check import family_model  # noqa: E402

DEPTHS = (2, 3, 12)
NO_CAP = 1 << 13


@pytest.mark.parametrize("recycle_model", cluster_solve.RECYCLE_MODELS)
def test_mirror_equals_the_enumeration_on_the_grid(recycle_model):
    """Every non-refused case of the 40-seed grid at prefix depths 2, 3 and 12, without a bound and with the greedy's cost2: cost2 and
    mask are exact_small()'s, and "infeasible" stands exactly where the enumeration finds no set.  A task of at most 12 columns has fewer
    than 2^13 nodes, so no cap bites at NO_CAP."""
    settings = cluster.ilp_settings(recycle_model)
    solved = infeasible = 0
    for seed in range(1, 41):
        n, M = 6 + seed % 7, 5 + seed % 9
        for with_gaps, with_pairs in FLAVOURS:
            tint, incomp = small_case(seed, n, M, with_gaps, with_pairs)
            model = model_of(tint, incomp, list(range(n)), settings)
            if model["refused"] is not None:
                continue
            want = cluster_solve.exact_small(model, settings)
            greedy = cluster_solve.greedy_incumbent(model, settings)
            assert (want is None) == (greedy is None)
            for depth in DEPTHS:
                got = cluster_solve.exact_bnb(model, settings, depth=depth, node_cap=NO_CAP)
                assert got["capped"] == 0 and got["nodes"] >= 1 << min(n, depth)
                if want is None:
                    assert got["status"] == "infeasible" and got["mask"] is None and got["cost2"] is None, (seed, depth, got)
                    infeasible += 1
                    continue
                bounded = cluster_solve.exact_bnb(model, settings, ub2=greedy["cost2"], depth=depth, node_cap=NO_CAP)
                for g in (got, bounded):
                    assert g["status"] == "optimal" and (g["cost2"], g["mask"]) == (want["cost2"], want["mask"]), (seed, with_gaps, with_pairs, depth, g, want)
                    assert (g["x"], g["e"], g["members"], g["cost"]) == (want["x"], want["e"], want["members"], want["cost"])
                assert bounded["nodes"] <= got["nodes"]
                solved += 1
    assert (solved, infeasible) == (132 * len(DEPTHS), 24 * len(DEPTHS))


@pytest.mark.parametrize("recycle_model", cluster_solve.RECYCLE_MODELS)
def test_mirror_picks_the_smallest_optimal_mask(recycle_model):
    """The grid's feasible cases against the brute force's list of optimal subsets; at least 10 cases a model have more than one
    (constant 25, exons 17, introns 37, as test_exact_host counts them)."""
    settings = cluster.ilp_settings(recycle_model)
    ties = 0
    for tint, incomp, remaining, feasible in grid():
        model = model_of(tint, incomp, remaining, settings)
        costs = {mask: corr + sum(g for c, g in enumerate(model["garbage"]) if not mask >> c & 1) for mask, corr in feasible.items()}
        best = min(costs.values())
        optimal = sorted(mask for mask, cost in costs.items() if cost == best)
        ties += len(optimal) > 1
        got = cluster_solve.exact_bnb(model, settings, depth=3, node_cap=NO_CAP)
        assert (got["status"], got["cost"], got["mask"]) == ("optimal", best, optimal[0]), (tint["id"], got, optimal)
    assert ties >= 10


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_mirror_against_highs_at_28_columns(seed):
    """small_case(seed, 28, 12, gaps, pairs) under the default settings, bounded by the greedy, depth 12, node_cap 65 536: proven, at the
    cost HiGHS proves."""
    settings = cluster.ilp_settings()
    tint, incomp = small_case(seed, 28, 12, True, True)
    remaining = list(range(28))
    model = model_of(tint, incomp, remaining, settings)
    assert model["refused"] is None
    greedy = cluster_solve.greedy_incumbent(model, settings)
    got = cluster_solve.exact_bnb(model, settings, ub2=greedy["cost2"], depth=12, node_cap=65536)
    assert got["status"] == "optimal" and got["capped"] == 0
    status, x, e = cluster_solve.solve_round(model, settings)
    assert status == cluster_solve.OPTIMAL
    want = cluster_solve.round_cost(model, x, e)
    assert cluster_solve.round_cost(model, got["x"], got["e"]) == want == got["cost"]
    assert ru.subset_cost(tint, incomp, remaining, set(got["members"]), settings) == want


@pytest.mark.parametrize("R,n_low", [(33, 32), (64, 32)])
def test_the_optimum_beyond_column_31(R, n_low):
    """Two families, every cross pair incompatible; the one at the columns from 32 on is the cheaper: a mask cut to 32 bits is empty."""
    settings = cluster.ilp_settings()
    model, tint, incomp = family_model(R, n_low)
    want_mask = ((1 << R) - 1) ^ ((1 << n_low) - 1)
    want_cost = (R - n_low - 1) + 3 * n_low
    greedy = cluster_solve.greedy_incumbent(model, settings)
    for ub2, depth in ((greedy["cost2"], 12), (greedy["cost2"], 3)) + (((None, 12),) if R == 33 else ()):      # (unbounded, 64 columns take a minute here)
        got = cluster_solve.exact_bnb(model, settings, ub2=ub2, depth=depth, node_cap=1 << 20)
        assert (got["status"], got["mask"], got["cost"]) == ("optimal", want_mask, want_cost), (ub2, depth, got)
        assert got["mask"] & 0xffffffff == 0 and got["members"] == list(range(n_low, R))
    assert ru.subset_cost(tint, incomp, list(range(R)), set(range(n_low, R)), settings) == want_cost
    assert ru.subset_cost(tint, incomp, list(range(R)), set(range(n_low)), settings) > want_cost
    assert ru.subset_cost(tint, incomp, list(range(R)), {0, n_low}, settings) is None


def test_the_cap():
    """node_cap = 1 leaves every live prefix of a 12-column problem capped and without a leaf; a larger cap finds sets, all feasible,
    none better than the optimum; the counts respect the cap."""
    settings = cluster.ilp_settings()
    tint, incomp = small_case(5, 12, 12, True, True)
    remaining = list(range(12))
    model = model_of(tint, incomp, remaining, settings)
    want = cluster_solve.exact_small(model, settings)
    assert want["mask"] & 3 != 3                             # (the optimum is not the all-in prefix)
    got = cluster_solve.exact_bnb(model, settings, depth=2, node_cap=1)
    assert got["status"] == "unproven" and got["capped"] >= 1 and got["nodes"] == 4 and got["mask"] is None and got["cost2"] is None
    seen = set()
    for node_cap in (7, 11, 12, 40, 200):
        got = cluster_solve.exact_bnb(model, settings, depth=2, node_cap=node_cap)
        assert got["nodes"] <= 4 * node_cap
        if got["capped"]:
            assert got["status"] == "unproven"
        if got["mask"] is not None:
            assert ru.subset_cost(tint, incomp, remaining, set(got["members"]), settings) == got["cost"] >= want["cost"]
        seen.add((got["status"], got["mask"] is not None))
    assert ("unproven", True) in seen
    tb = cluster_solve.bnb_tables(model, settings)
    assert cluster_solve.bnb_task(tb, 0, 2, None, 1) == (-1, 0, 1, True)


def test_the_boundary_row():
    """test_exact_host's three boundary models through the search at depth 1."""
    settings = cluster.ilp_settings(epsilon=0.15)
    got = cluster_solve.exact_bnb(boundary_model(250), settings, depth=1)
    assert (got["status"], got["cost2"], got["mask"], got["members"], got["e"]) == ("optimal", 2, 3, [0, 1], [1, 1, 1])
    got = cluster_solve.exact_bnb(boundary_model(251), settings, depth=1)
    assert (got["status"], got["cost2"], got["mask"]) == ("optimal", 100, 2)
    got = cluster_solve.exact_bnb(boundary_model(250 + 20 + 400 + 1), settings, depth=1)
    assert (got["status"], got["cost2"], got["mask"]) == ("infeasible", None, None)


def test_mirror_arguments():
    settings = cluster.ilp_settings()
    tint, incomp = small_case(3, 8, 9, True, True)
    model = model_of(tint, incomp, list(range(8)), settings)
    with pytest.raises(ValueError, match="multiple of 0.5"):
        cluster_solve.exact_bnb(dict(model, garbage=[3.25] * 8), settings)
    with pytest.raises(ValueError, match="8 columns"):
        cluster_solve.exact_bnb(dict(model, garbage=[3.0] * 7), settings)
    with pytest.raises(ValueError, match="node_cap"):
        cluster_solve.exact_bnb(model, settings, node_cap=0)
    wide = dict(n_cols=65, inf_seg=[], support=[], corrections=[[]] * 65, pairs=[], groups=[], group_segs=[], gap_rows=[], garbage=[1.0] * 65, max_lg=0)
    with pytest.raises(ValueError, match="64 at the most"):
        cluster_solve.exact_bnb(wide, settings)
    empty = cluster_solve.exact_bnb(model_of(tint, incomp, [], settings), settings)
    assert (empty["status"], empty["cost2"], empty["mask"], empty["nodes"]) == ("optimal", 0, 0, 1)
    got = cluster_solve.exact_bnb(model, settings, ub2=0, depth=3)             # a bound nothing reaches
    assert got["status"] == "unproven" and got["mask"] is None and got["capped"] == 0


class BnbContext(MirrorContext):
    """MirrorContext with a round_bnb() that is the mirror behind the library's rule of which problems are taken."""

    def __init__(self, tints, part0, depth, node_cap):
        MirrorContext.__init__(self, tints, part0)
        self.depth, self.node_cap, self.bnb_calls, self.results = depth, node_cap, 0, []

    def round_bnb(self, garbage, ub2, epsilon, offset, min_cols, max_cols, max_nodes, depth=None, node_cap=None):
        self.bnb_calls += 1
        col_off = np.cumsum([0] + [len(rem) for _, rem in self.problems])
        assert len(garbage) == col_off[-1] and len(ub2) == len(self.problems)
        P = len(self.problems)
        status, cost2, mask, total = [-2] * P, [-1] * P, [0] * P, 0
        for R, p in sorted((len(rem), p) for p, (_, rem) in enumerate(self.problems) if min_cols <= len(rem) <= max_cols):
            if total + (self.node_cap << min(R, self.depth)) > max_nodes:
                break
            total += self.node_cap << min(R, self.depth)
            q = self.problems[p][0]
            tint = self.tints[max(k for k in range(len(self.part0)) if self.part0[k] <= q)]
            got = cluster_solve.exact_bnb(dict(self.model(p), garbage=list(garbage[col_off[p]:col_off[p + 1]]), max_lg=sum(s[2] for s in tint["segs"])),
                                          dict(epsilon=epsilon, offset=offset), None if ub2[p] < 0 else int(ub2[p]), self.depth, self.node_cap)
            status[p] = ("optimal", "infeasible", "unproven").index(got["status"])
            if got["mask"] is not None:
                cost2[p], mask[p] = got["cost2"], got["mask"]
            self.results.append((q, tuple(self.problems[p][1]), got))
        return dict(n_prob=P, col_off=col_off, status=np.array(status, np.int32), cost2=np.array(cost2, np.int64), mask=np.array(mask, np.uint64))


def run_bnb_loop(monkeypatch, depth, node_cap, settings):
    tints, part0 = loop_tints()
    ctx = BnbContext(tints, part0, depth, node_cap)
    monkeypatch.setattr(cluster_prep, "round_model", lambda arr, p: arr.model(p))
    record, jobs = [], []

    def solve(model, s):
        jobs.append((model["key"], model["n_cols"], model.get("incumbent")))
        return cluster_solve.solve_round(model, s)

    logs = cluster.cluster_tints(tints, part0, ctx, settings, solve=solve, on_round=record.append)
    return ctx, logs, record, jobs


def summary(record):
    return sorted((r["tint"]["id"], r["partition"], r["round"], r["status"], r["cost"], tuple(r["remaining"])) for r in record)


def test_loop_proved_problems_make_no_job_and_unproven_ones_carry_the_incumbent(monkeypatch):
    """Partitions of 4 .. 6 reps.  With room to finish, every problem is proven and the solver is never called; with 4 nodes a task
    behind a 2-column prefix some searches stop early: each of those makes one job, which carries the better of the search's set and the
    greedy's as its incumbent where the search had found one, and none where it had not (the incumbent mode is off)."""
    base = dict(min_isoform_size=2)
    ctx, logs, record, jobs = run_bnb_loop(monkeypatch, 12, 4096, cluster.ilp_settings(bnb_cols=12, **base))
    rounds = len(set(r["round"] for r in record))
    assert record and not jobs and ctx.bnb_calls == ctx.incumbent_calls == rounds
    assert all(got["status"] == "optimal" for _, _, got in ctx.results) and len(ctx.results) == len(record)
    for r in record:
        best = ru.brute_force(r["tint"], r["incomp"], r["remaining"], cluster.ilp_settings())
        assert r["status"] == "OPTIMAL" and r["cost"] == best[0]
    proven = summary(record)

    ctx, logs, record, jobs = run_bnb_loop(monkeypatch, 2, 4, cluster.ilp_settings(bnb_cols=12, **base))
    assert [s[:5] for s in summary(record) if s[2] == 0] == [s[:5] for s in proven if s[2] == 0]       # (later rounds may differ where HiGHS breaks a tie another way)
    by_status = {"optimal": 0, "unproven": 0}
    carried = bare = 0
    job_of = {(key, n): inc for key, n, inc in jobs}
    assert len(job_of) == len(jobs)
    keyed = {}
    for r in record:
        keyed[(ctx.part0[[t["id"] for t in ctx.tints].index(r["tint"]["id"])] + r["partition"], tuple(r["remaining"]))] = r
    for q, remaining, got in ctx.results:
        r = keyed[(q, remaining)]
        key = ((r["tint"]["id"], r["partition"], r["round"]), len(remaining))
        by_status[got["status"]] += 1
        if got["status"] == "optimal":
            assert key not in job_of and r["status"] == "OPTIMAL" and r["cost"] == got["cost"] and r["x"] == got["x"]
            continue
        assert key in job_of
        model = model_of(r["tint"], r["incomp"], list(remaining), cluster.ilp_settings())
        greedy = cluster_solve.greedy_incumbent(model, cluster.ilp_settings())
        if got["mask"] is None:
            assert job_of[key] is None
            bare += 1
        else:
            assert got["cost2"] <= greedy["cost2"]
            assert job_of[key] == ((got["cost"], got["x"]) if got["cost2"] < greedy["cost2"] else (greedy["cost"], greedy["x"]))
            carried += 1
        assert r["status"] == "OPTIMAL" and r["cost"] == ru.brute_force(r["tint"], r["incomp"], list(remaining), cluster.ilp_settings())[0]
    assert by_status["optimal"] and carried and bare and len(jobs) == by_status["unproven"]


def test_loop_without_the_feature_makes_no_call(monkeypatch):
    """bnb_cols = 0, and settings that do not know the feature at all: no round_bnb call, no incumbents call, the same records; a
    bnb_cols at or under exact_cols leaves the search nothing to take and makes no call either."""
    base = dict(min_isoform_size=2)
    ctx0, logs0, record0, jobs0 = run_bnb_loop(monkeypatch, 12, 4096, cluster.ilp_settings(bnb_cols=0, **base))
    assert ctx0.bnb_calls == 0 and ctx0.incumbent_calls == 0 and len(jobs0) == len(record0) > 0
    old = {k: v for k, v in cluster.ilp_settings(**base).items() if not k.startswith("bnb_")}
    ctx1, logs1, record1, jobs1 = run_bnb_loop(monkeypatch, 12, 4096, old)
    assert ctx1.bnb_calls == 0 and logs0 == logs1 and jobs0 == jobs1
    strip = lambda rec: [{k: v for k, v in r.items() if k != "tint"} for r in rec]
    assert strip(record0) == strip(record1)
    assert [r["tint"]["id"] for r in record0] == [r["tint"]["id"] for r in record1]
    ctx2, _, record2, jobs2 = run_bnb_loop(monkeypatch, 12, 4096, cluster.ilp_settings(bnb_cols=0, incumbent="cutoff", **base))
    assert ctx2.bnb_calls == 0 and ctx2.incumbent_calls > 0


def test_loop_shares_the_incumbents_call_and_respects_the_sizes(monkeypatch):
    """Under incumbent = cutoff the loop's own round_incumbents call serves the search too; min_cols is exact_cols + 1."""
    tints, part0 = loop_tints()
    seen = []

    class Ctx(BnbContext):
        def round_bnb(self, garbage, ub2, epsilon, offset, min_cols, max_cols, max_nodes, **kw):
            seen.append((min_cols, max_cols, max_nodes))
            return BnbContext.round_bnb(self, garbage, ub2, epsilon, offset, min_cols, max_cols, max_nodes)

        def round_exact(self, garbage, epsilon, offset, max_cols, max_masks):
            P = len(self.problems)
            col_off = np.cumsum([0] + [len(rem) for _, rem in self.problems])
            return dict(n_prob=P, col_off=col_off, cost2=np.full(P, -2, np.int64), mask=np.zeros(P, np.uint32))

    ctx = Ctx(tints, part0, 12, 4096)
    monkeypatch.setattr(cluster_prep, "round_model", lambda arr, p: arr.model(p))
    sizes = []
    settings = cluster.ilp_settings(min_isoform_size=2, incumbent="cutoff", exact_cols=4, bnb_cols=5, bnb_nodes=1 << 20, max_rounds=1)
    record = []
    cluster.cluster_tints(tints, part0, ctx, settings, solve=lambda m, s: sizes.append(m["n_cols"]) or cluster_solve.solve_round(m, s), on_round=record.append)
    assert seen == [(5, 5, 1 << 20)] and ctx.incumbent_calls == 1
    lens = sorted(len(r["remaining"]) for r in record)
    assert sorted(sizes) == [n for n in lens if n != 5] and 5 in lens and all(r["status"] == "OPTIMAL" for r in record)


def test_round_bnb_solution():
    arr = dict(col_off=np.array([0, 3, 5, 6, 40, 42]), status=np.array([0, 1, -2, 2, 2], np.int32), cost2=np.array([7, -1, -1, 9, -1]),
               mask=np.array([5, 0, 0, (1 << 33) | 1, 0], np.uint64))
    assert cluster_prep.round_bnb_solution(arr, 0) == (3.5, [1, 0, 1])
    assert cluster_prep.round_bnb_solution(arr, 1) == "infeasible"
    assert cluster_prep.round_bnb_solution(arr, 2) is None
    assert cluster_prep.round_bnb_solution(arr, 3) == ("unproven", 4.5, [1] + [0] * 32 + [1])
    assert cluster_prep.round_bnb_solution(arr, 4) == ("unproven", None, None)


def test_settings_and_cli_flags(tmp_path):
    settings = cluster.ilp_settings()
    assert settings["bnb_cols"] == 0 and settings["bnb_nodes"] == cluster.BNB_NODES
    cluster.check_bnb(settings)
    cluster.check_bnb(cluster.ilp_settings(bnb_cols=64, bnb_nodes=1))
    cluster.check_bnb({})                                    # (settings from before the feature)
    with pytest.raises(ValueError, match="bnb_cols"):
        cluster.check_bnb(cluster.ilp_settings(bnb_cols=65))
    with pytest.raises(ValueError, match="bnb_cols"):
        cluster.check_bnb(cluster.ilp_settings(bnb_cols=-1))
    with pytest.raises(ValueError, match="bnb_nodes"):
        cluster.check_bnb(cluster.ilp_settings(bnb_cols=30, bnb_nodes=0))
    base = ["-s", str(tmp_path)]
    args = cluster.parse_args(base)
    assert args.exact_bnb == 0 and args.bnb_nodes == cluster.BNB_NODES
    for n in (0, 1, 25, 64):
        assert cluster.parse_args(base + ["--exact-bnb", str(n)]).exact_bnb == n
    assert cluster.parse_args(base + ["--exact-bnb", "40", "--bnb-nodes", "1000"]).bnb_nodes == 1000
    for bad in (["--exact-bnb", "65"], ["--exact-bnb", "-1"], ["--exact-bnb", "x"], ["--bnb-nodes", "0"]):
        with pytest.raises(SystemExit):
            cluster.parse_args(base + bad)


def test_kernel_bodies_on_the_host():
    """What one lane of k_bnb_prep / k_bnb_search computes (freddie_amd/csrc/clu_bnb.h), compiled for the host with the address and
    undefined-behaviour sanitizers and run over every task of the grid's problems, of random ones of up to 40 columns at node_cap 256
    and of the built 33- and 64-column problems, against the mirror."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bnb_host_check.py"), "--cases", "40"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and " 0 differ" in res.stdout, res.stdout + res.stderr
