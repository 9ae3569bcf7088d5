"""The branch and bound over a round's larger problems on the GPU (fclu_round_bnb) against the Python mirror (cluster_solve.exact_bnb),
exactly: status, cost2, mask, node count and capped tasks of every problem, on the grid of small problems in one batch (refused problems
left in; R below, at and above the prefix depth; dead prefixes) and on built ones where the kernels can go wrong -- optima beyond
column 31, segment counts that more than one lane stages, a set every pair of which is in conflict, no pairs at all, a problem without a
feasible subset, the epsilon 0.15 boundary row, node caps of 1 and 7, the node budget, one task a launch, two rounds on one context --
then what stays valid behind the call, the refusals and the loop on files."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

import cluster_util as cu
import round_util as ru
from freddie_amd import cluster, cluster_prep, cluster_solve
from test_gpu_incumbents import flips_tint, grid_tints, star_tint
from test_gpu_round_models import all_problems, stage

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

from bnb_host_check import family_tint  # noqa: E402

pytestmark = pytest.mark.gpu

SETTINGS = cluster.ilp_settings()
BIG = 1 << 34
STATUS = {"optimal": 0, "infeasible": 1, "unproven": 2}


@pytest.fixture(scope="module")
def ctx():
    c = cluster_prep.Context(0)
    yield c
    c.close()


def models_of(tints, problems, settings):
    models = []
    for t, q, rem in problems:
        model = ru.restate(tints[t], tints[t]["partitions"][q][1], rem)
        model["garbage"] = ru.garbage_costs(tints[t], rem, settings["recycle_model"])
        model["max_lg"] = sum(s[2] for s in tints[t]["segs"])
        models.append(model)
    return models


def mirror(models, settings, ub2, min_cols, max_cols, depth, node_cap, max_nodes):
    """(per problem None (refused or not taken) or (status, cost2, mask, nodes, capped); problems taken), by the rule of
    include/freddie_cluster.h: ascending (columns, problem) while the running total of 2^D * node_cap stays inside the budget."""
    want, n_taken, total = [None] * len(models), 0, 0
    for R, p in sorted((m["n_cols"], p) for p, m in enumerate(models) if m["refused"] is None and min_cols <= m["n_cols"] <= max_cols):
        if total + (node_cap << min(R, depth)) > max_nodes:
            break
        n_taken, total = n_taken + 1, total + (node_cap << min(R, depth))
        got = cluster_solve.exact_bnb(models[p], settings, None if ub2[p] < 0 else int(ub2[p]), depth, node_cap)
        want[p] = (STATUS[got["status"]], -1 if got["mask"] is None else got["cost2"], got["mask"] or 0, got["nodes"], got["capped"])
    return want, n_taken


def garbage_of(tints, problems, settings):
    return [g for t, _, rem in problems for g in ru.garbage_costs(tints[t], rem, settings["recycle_model"])]


def check(got, want, n_taken, problems):
    assert got["n_prob"] == len(want) == len(problems)
    assert got["n_taken"] == n_taken
    for p, w in enumerate(want):
        mine = tuple(int(got[k][p]) for k in ("status", "cost2", "mask", "nodes", "capped"))
        solution = cluster_prep.round_bnb_solution(got, p)
        if w is None:
            assert mine == (-2, -1, 0, 0, 0) and solution is None, (p, mine)
            continue
        assert mine == w, (p, mine, w)
        x = [w[2] >> c & 1 for c in range(len(problems[p][2]))]
        if w[0] == 0:
            assert solution == (w[1] / 2.0, x)
        elif w[0] == 1:
            assert solution == "infeasible"
        else:
            assert solution == (("unproven", w[1] / 2.0, x) if w[1] >= 0 else ("unproven", None, None))
    assert got["nodes_total"] == sum(w[3] for w in want if w is not None)


def compare(ctx, tints, part0, problems, settings=SETTINGS, bound=True, min_cols=1, max_cols=64, depth=3, node_cap=4096, max_nodes=BIG):
    """One round on the device and through the mirror; bound: the device's greedy incumbents' cost2 bounds both."""
    models = models_of(tints, problems, settings)
    ctx.round_models([part0[t] + q for t, q, _ in problems], [rem for _, _, rem in problems])
    garbage = garbage_of(tints, problems, settings)
    ub2 = ctx.round_incumbents(garbage, settings["epsilon"], settings["offset"])["cost2"] if bound else np.full(len(problems), -1, np.int64)
    got = ctx.round_bnb(garbage, ub2, settings["epsilon"], settings["offset"], min_cols, max_cols, max_nodes, depth, node_cap)
    want, n_taken = mirror(models, settings, ub2, min_cols, max_cols, depth, node_cap, max_nodes)
    check(got, want, n_taken, problems)
    return got, want


@pytest.mark.parametrize("max_ilp", [1000, 3])
@pytest.mark.parametrize("recycle_model", cluster_solve.RECYCLE_MODELS)
def test_grid_in_one_batch(ctx, recycle_model, max_ilp):
    """Every partition of the 80 grid tints in ONE call at depth 3: problems of fewer, of 3 and of more columns than the prefix, refused
    ones (not taken), infeasible ones, prefixes with a pair inside (max_ilp 3 splits the components, which is where pairs come from),
    with the greedy's bound and without one."""
    tints = grid_tints()
    part0 = stage(ctx, tints, maximum_ilp_size=max_ilp)
    problems = all_problems(tints, lambda t, q, rids: rids[::-1] if t % 3 == 0 else rids)
    settings = cluster.ilp_settings(recycle_model)
    for bound in (True, False):
        got, want = compare(ctx, tints, part0, problems, settings, bound)
        taken = [w for w in want if w is not None]
        assert all(w[4] == 0 for w in taken) and sum(w[0] == 0 for w in taken) > len(want) // 2 and any(w[2] for w in taken)
        sizes = set(len(rem) for _, _, rem in problems)
        assert min(sizes) < 3 and 3 in sizes and 4 in sizes
        if max_ilp == 1000:
            assert any(w is None for w in want) and (bound or any(w is not None and w[0] == 1 for w in want))
        else:
            assert sum(len(inc) for tint in tints for _, inc in tint["partitions"]) > 0
    assert got["n_launches"] >= 1 and all(v >= 0 for v in ctx.round_bnb_timing().values())


def family(tid, R, n_low):
    return family_tint(tid, R, n_low)[0]


def test_optima_beyond_column_31(ctx):
    """Two families of reps, every cross pair incompatible, the cheaper one at the upper columns: R = 25, 32, 33, 63 and 64 at depth 12.
    At 33 columns the optimum is column 32 alone, at 64 the columns 32 .. 63: a mask cut to 32 bits would be empty."""
    shapes = [(25, 12), (32, 16), (33, 32), (63, 31), (64, 32)]
    tints = [family(t, R, n_low) for t, (R, n_low) in enumerate(shapes)]
    part0 = stage(ctx, tints)
    assert [len(t["partitions"]) for t in tints] == [1] * len(shapes)
    problems = [(t, 0, list(range(R))) for t, (R, _) in enumerate(shapes)]
    for t, (R, n_low) in enumerate(shapes):
        assert sorted(tints[t]["partitions"][0][0]) == list(range(R + 2))
        assert ru.restate(tints[t], tints[t]["partitions"][0][1], problems[t][2])["pairs"] == [(a, b) for a in range(n_low) for b in range(n_low, R)]
    got, want = compare(ctx, tints, part0, problems, depth=12)
    for (R, n_low), w in zip(shapes, want):
        assert w[0] == 0 and w[2] == ((1 << R) - 1) ^ ((1 << n_low) - 1) and w[1] == 2 * ((R - n_low - 1) + 3 * n_low)
    assert got["mask"].dtype == np.uint64 and int(got["mask"][2]) == 1 << 32 and int(got["mask"][4]) == 0xffffffff00000000
    compare(ctx, tints, part0, [(t, q, rem[::-1]) for t, q, rem in problems], depth=6, node_cap=512)      # (the families at the other end)


def test_28_columns_at_depth_12(ctx):
    """The rows and gaps of the host test's 28-column cases, partitioned on the device (whole, and in parts of at most 14 reps, which
    brings pairs), every partition a problem, 4 096 tasks each where it has 12 columns or more."""
    tints = []
    for seed in (1, 2, 3):
        rng = random.Random(seed)
        rows = ru.random_rows(rng, 28, 12, const_runs=seed % 2 == 0, flip=0.1)
        gaps, polys = ru.random_gaps(rng, rows, p=0.7)
        tints.append(ru.make_tint(seed, rows, gaps, polys, members={i: rng.randrange(1, 4) for i in range(28)}))
    for max_ilp in (1000, 14):
        part0 = stage(ctx, tints, maximum_ilp_size=max_ilp)
        got, want = compare(ctx, tints, part0, all_problems(tints, lambda t, q, rids: rids), depth=12, node_cap=65536)
        assert any(w is not None and w[0] == 0 and w[3] > 4096 for w in want)


@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 130])
def test_segment_counts(ctx, M):
    rng = random.Random(M)
    rows = ru.random_rows(rng, 10, M)
    tints = [ru.make_tint(7, rows, *ru.random_gaps(rng, rows), members={i: rng.randrange(1, 4) for i in range(10)}), flips_tint(1, 9, max(M, 8))]
    part0 = stage(ctx, tints)
    for recycle_model in ("constant", "introns"):
        got, want = compare(ctx, tints, part0, all_problems(tints, lambda t, q, rids: rids), cluster.ilp_settings(recycle_model))
        assert any(w is not None and w[0] == 0 for w in want)
    compare(ctx, tints, part0, all_problems(tints, lambda t, q, rids: rng.sample(rids, (len(rids) + 1) // 2)), bound=False)


def test_every_pair_in_conflict_and_no_pairs_at_all(ctx):
    """26 leaves of a star without its centre: every pair is in conflict, the optimum is one column, the smallest; 26 reps of one pattern
    and no pair: everything joins, and the bound proves it in a few hundred nodes."""
    tints = [star_tint(0, 26, 110), flips_tint(1, 26, 44)]
    part0 = stage(ctx, tints)
    assert [len(t["partitions"]) for t in tints] == [1, 1] and len(tints[0]["partitions"][0][1]) == 26 * 25 // 2 and tints[1]["partitions"][0][1] == []
    leaves = [r for r in tints[0]["partitions"][0][0] if r != 26]
    problems = [(0, 0, leaves[::-1]), (1, 0, list(tints[1]["partitions"][0][0]))]
    got, want = compare(ctx, tints, part0, problems)
    assert want[0][:3] == (0, 2 * 3 * 25, 1) and want[1][0] == 0 and want[1][2] == (1 << 26) - 1 and want[1][3] < 1000
    got, want = compare(ctx, tints, part0, problems, bound=False, depth=5)
    assert want[0][:3] == (0, 2 * 3 * 25, 1)


def test_a_gap_nothing_satisfies_and_the_boundary_row(ctx):
    """A gap of 500 > offset + MAX_ISOFORM_LG breaks its rep's row inside and outside the set: infeasible without a bound, and there is
    no incumbent to bound it.  epsilon 0.15, offset 20, G = 200: l = 250 holds by the model's tolerance alone, l = 251 does not."""
    lens = [10, 10, 10, 50, 50, 10, 10, 50, 50, 10, 10, 10]
    tints = [flips_tint(0, 8, 12, {3: {(2, 9): 500}}), flips_tint(1, 8, 12, {3: {(2, 9): 5}}), flips_tint(2, 8, 12, {0: {(2, 9): 250}}, lens),
             flips_tint(3, 8, 12, {0: {(2, 9): 251}}, lens)]
    part0 = stage(ctx, tints)
    problems = all_problems(tints, lambda t, q, rids: rids)
    for bound in (True, False):
        got, want = compare(ctx, tints, part0, problems, cluster.ilp_settings(epsilon=0.15), bound)
        assert [w[:3] for w in want[2:]] == [(0, 14, 0xff), (0, 20, 0xfe)] and want[0][:3] == (1, -1, 0) and want[1][0] == 0
    got, want = compare(ctx, tints, part0, problems, bound=False, depth=0)
    assert [w[:3] for w in want[2:]] == [(0, 14, 0xff), (0, 14, 0xff)]


@pytest.mark.parametrize("node_cap", [1, 7])
def test_node_caps(ctx, node_cap):
    """Every task stops at 1 resp. 7 nodes: capped tasks, unproven problems with and without a set, every count the mirror's."""
    tints = grid_tints()[::2]
    part0 = stage(ctx, tints)
    problems = all_problems(tints, lambda t, q, rids: rids)
    for bound in (True, False):
        got, want = compare(ctx, tints, part0, problems, bound=bound, depth=2, node_cap=node_cap)
        taken = [w for w in want if w is not None]
        assert any(w[0] == 2 and w[4] > 0 for w in taken) and all(w[3] <= 4 * node_cap for w in taken)
        assert any(w[0] == 0 for w in taken)                 # (problems of at most two columns are leaves at once)
        if node_cap == 7:
            assert any(w[0] == 2 and w[1] >= 0 for w in taken)


def test_the_budget(ctx):
    """Problems of 8, 3 and 5 columns at depth 4 and node_cap 10: 160, 80 and 160 nodes of budget, taken in ascending (columns, problem)."""
    tints = [flips_tint(0, 8, 12), flips_tint(1, 3, 12), flips_tint(2, 5, 12)]
    part0 = stage(ctx, tints)
    problems = all_problems(tints, lambda t, q, rids: rids)
    for budget, taken in ((240, 2), (399, 2), (400, 3), (239, 1), (80, 1), (79, 0), (1, 0)):
        got, want = compare(ctx, tints, part0, problems, depth=4, node_cap=10, max_nodes=budget)
        assert got["n_taken"] == taken
        assert [w is not None for w in want] == [taken >= 3, taken >= 1, taken >= 2]
    got, want = compare(ctx, tints, part0, problems, min_cols=4, max_cols=5)
    assert [w is not None for w in want] == [False, False, True]
    got, want = compare(ctx, tints, part0, problems, min_cols=0, max_cols=0)
    assert want == [None] * 3 and (got["n_taken"], got["n_launches"], got["nodes_total"]) == (0, 0, 0)


def test_one_task_a_launch(ctx, monkeypatch):
    """FCLU_BNB_SLICE=1: a 7-column problem at depth 5 is 32 launches, the problems beside it more; the results are the same."""
    tints = [flips_tint(0, 7, 44, {5: {(2, 9): 3}}), flips_tint(1, 3, 12), flips_tint(2, 9, 12)]
    part0 = stage(ctx, tints)
    problems = all_problems(tints, lambda t, q, rids: rids)
    plain, want = compare(ctx, tints, part0, problems, cluster.ilp_settings("exons"), depth=5)
    assert plain["n_launches"] == 1
    monkeypatch.setenv("FCLU_BNB_SLICE", "1")
    sliced, _ = compare(ctx, tints, part0, problems, cluster.ilp_settings("exons"), depth=5)
    assert sliced["n_launches"] == 8 + 32 + 32
    monkeypatch.setenv("FCLU_BNB_SLICE", "40")
    some, _ = compare(ctx, tints, part0, problems, cluster.ilp_settings("exons"), depth=5)
    assert 1 < some["n_launches"] < 8
    for k in ("status", "cost2", "mask", "nodes", "capped"):
        assert sliced[k].tolist() == plain[k].tolist() == some[k].tolist()


def test_two_rounds_and_what_stays_valid(ctx):
    """Two rounds on one context; behind the call the round's own results, the incumbents' and the exact call's are where they were."""
    tints = grid_tints()[::5]
    part0 = stage(ctx, tints)
    for pick in (lambda t, q, rids: rids, lambda t, q, rids: rids[1::2][::-1]):
        problems = all_problems(tints, pick)
        models = models_of(tints, problems, SETTINGS)
        arr = ctx.round_models([part0[t] + q for t, q, _ in problems], [rem for _, _, rem in problems])
        garbage = garbage_of(tints, problems, SETTINGS)
        inc = ctx.round_incumbents(garbage, SETTINGS["epsilon"], SETTINGS["offset"])
        exact = ctx.round_exact(garbage, SETTINGS["epsilon"], SETTINGS["offset"], 12, 1 << 40)
        got = ctx.round_bnb(garbage, inc["cost2"], SETTINGS["epsilon"], SETTINGS["offset"], 1, 64, BIG, 3, 4096)
        check(got, *mirror(models, SETTINGS, inc["cost2"], 1, 64, 3, 4096, BIG), problems)
        r = cluster_prep._Rounds()
        assert ctx._L.fclu_round_results(ctx._h, ctypes.byref(r)) == 0 and r.n_prob == len(problems)
        assert cluster_prep._copy_out(r.inf_seg, int(r.n_inf), np.int32).tolist() == arr["inf_seg"].tolist()
        assert cluster_prep._copy_out(r.sup_cols, int(r.n_sup), np.int32).tolist() == arr["sup_cols"].tolist()
        assert cluster_prep._copy_out(r.rows, 3 * int(r.n_gap_rows), np.int32).tolist() == arr["rows"].reshape(-1).tolist()
        assert cluster_prep._copy_out(r.refused, r.n_prob, np.int32).tolist() == arr["refused"].tolist()
        i = cluster_prep._Incumbents()
        assert ctx._L.fclu_round_incumbent_results(ctx._h, ctypes.byref(i)) == 0 and i.n_prob == len(problems)
        assert cluster_prep._copy_out(i.cost2, i.n_prob, np.int64).tolist() == inc["cost2"].tolist()
        assert cluster_prep._copy_out(i.mem, int(i.n_mem), np.int32).tolist() == inc["mem"].tolist()
        x = cluster_prep._Exact()
        assert ctx._L.fclu_round_exact_results(ctx._h, ctypes.byref(x)) == 0 and x.n_prob == len(problems)
        assert cluster_prep._copy_out(x.cost2, x.n_prob, np.int64).tolist() == exact["cost2"].tolist()
        assert cluster_prep._copy_out(x.mask, x.n_prob, np.uint32).tolist() == exact["mask"].tolist()
        for p in range(len(problems)):                       # the search and the enumeration agree problem for problem
            if got["status"][p] == 0:
                assert (int(got["cost2"][p]), int(got["mask"][p])) == (int(exact["cost2"][p]), int(exact["mask"][p]))


def test_refusals(ctx):
    fresh = cluster_prep.Context(0)
    try:
        with pytest.raises(cluster_prep.ClusterError) as e:
            fresh.round_bnb([], [], 0.2, 20, 1, 64, BIG)
        assert e.value.code == 1
        assert fresh._L.fclu_round_bnb(fresh._h, None, None, 0.8, 1.2, 20, 1, 64, 12, 4096, 1000) == 1                # FCLU_ERR_ARG
        assert b"fclu_round_models" in fresh._L.fclu_last_error(fresh._h)
        b = cluster_prep._Bnb()
        assert fresh._L.fclu_round_bnb_results(fresh._h, ctypes.byref(b)) == 1
    finally:
        fresh.close()
    tints = [flips_tint(0, 8, 12), flips_tint(1, 5, 12)]
    part0 = stage(ctx, tints)
    problems = all_problems(tints, lambda t, q, rids: rids)
    compare(ctx, tints, part0, problems)
    none = [-1, -1]
    for garbage, word in (([3.0] * 12 + [3.25], "multiple of 0.5"), ([3.0] * 12, "12 garbage costs"), ([3.0] * 12 + [-1.0], "multiple of 0.5")):
        with pytest.raises(cluster_prep.ClusterError, match=word):
            ctx.round_bnb(garbage, none, 0.2, 20, 1, 64, BIG)
    with pytest.raises(cluster_prep.ClusterError, match="3 bounds"):
        ctx.round_bnb([3.0] * 13, [-1] * 3, 0.2, 20, 1, 64, BIG)
    for min_cols, max_cols, depth, node_cap, max_nodes, word in ((1, 65, 12, 4096, BIG, "max_cols"), (-1, 64, 12, 4096, BIG, "min_cols"), (9, 8, 12, 4096, BIG, "min_cols"),
                                                                 (1, 64, 21, 4096, BIG, "depth"), (1, 64, -1, 4096, BIG, "depth"), (1, 64, 12, 0, BIG, "node_cap"),
                                                                 (1, 64, 12, 4096, 0, "max_nodes"), (1, 64, 12, 4096, -5, "max_nodes")):
        with pytest.raises(cluster_prep.ClusterError, match=word) as e:
            ctx.round_bnb([3.0] * 13, none, 0.2, 20, min_cols, max_cols, max_nodes, depth, node_cap)
        assert e.value.code == 1
    g2, ub2 = np.full(13, 6, np.int32), np.full(2, -1, np.int64)
    call = lambda g, u, offset=20, node_cap=4096, max_nodes=BIG: ctx._L.fclu_round_bnb(ctx._h, g, u, 0.8, 1.2, offset, 1, 64, 12, node_cap, max_nodes)
    assert call(g2.ctypes.data, ub2.ctypes.data, offset=-1) == 1
    assert call(None, ub2.ctypes.data) == 1 and b"g2 is null" in ctx._L.fclu_last_error(ctx._h)
    assert call(g2.ctypes.data, None) == 1 and b"ub2 is null" in ctx._L.fclu_last_error(ctx._h)
    g2[4] = -1
    assert call(g2.ctypes.data, ub2.ctypes.data) == 1 and b"g2[4]" in ctx._L.fclu_last_error(ctx._h)
    g2[4] = 6
    assert ctx._L.fclu_round_bnb(ctx._h, g2.ctypes.data, ub2.ctypes.data, 0.8, 1.2, 20, 1, 64, 0, 1 << 30, 1 << 62) == 0     # one task a problem: one a launch
    assert ctx._L.fclu_round_bnb(ctx._h, g2.ctypes.data, ub2.ctypes.data, float("nan"), 1.2, 20, 1, 64, 12, 4096, BIG) == 1
    compare(ctx, tints, part0, problems)                                                    # the context stays usable
    many = [flips_tint(t, 13, 12) for t in range(3)]
    part0 = stage(ctx, many)
    probs = all_problems(many, lambda t, q, rids: rids)
    ctx.round_models([part0[t] + q for t, q, _ in probs], [rem for _, _, rem in probs])
    with pytest.raises(cluster_prep.ClusterError, match="launches") as e:                     # 3 x 2^13 tasks, one a launch
        ctx.round_bnb([3.0] * 39, [-1] * 3, 0.2, 20, 1, 64, 1 << 62, 13, 1 << 30)
    assert e.value.code == cluster_prep.ERR_UNSUPPORTED
    part0 = stage(ctx, tints)
    compare(ctx, tints, part0, problems)
    host = cu.random_tint(3, 30, 20)
    cluster_prep.partition_reads_batch([host], 1000, ctx, verbose=False)                    # fclu_partition ends the rounds' source
    assert call(g2.ctypes.data, ub2.ctypes.data) == 1
    with pytest.raises(cluster_prep.ClusterError):
        ctx.round_bnb([3.0] * 13, none, 0.2, 20, 1, 64, BIG)
    part0 = stage(ctx, tints)
    compare(ctx, tints, part0, problems)


def test_the_loop_on_files(ctx, tmp_path):
    """cluster_files() under exact_cols = 12, bnb_cols = 32 on fixture files staged with max_ilp = 20: problems of 13 .. 20 columns go
    to the search.  Where a round has no unproven problem its costs are those of the run with bnb_cols = 0 (the tie rule may pick
    another optimal set than HiGHS, so later rounds can differ: the first round is compared); a proven problem never reaches the solver."""
    paths = []
    for name in ("e_plateau_touch", "g1_dense", "g1_retention"):
        paths.append(cu.segment_tsv_file(name, tmp_path))
    costs, solved = {}, {}
    for bnb_cols in (32, 0):
        record, calls = [], []

        def solve(model, settings):
            calls.append((model["key"], model["n_cols"], model.get("incumbent")))
            return cluster_solve.solve_round(model, settings)

        settings = cluster.ilp_settings(max_ilp=20, exact_cols=12, bnb_cols=bnb_cols, max_rounds=30 if bnb_cols else 1)
        out = list(cluster.cluster_files(paths, settings, ctx=ctx, solve=solve, on_round=record.append))
        assert len(out) == len(paths) and len(record) > 5
        costs[bnb_cols] = sorted((r["tint"]["id"], r["partition"], r["status"], r["cost"]) for r in record if r["round"] == 0)
        solved[bnb_cols] = calls
        if bnb_cols:
            big = [r for r in record if 12 < len(r["remaining"]) <= 32]
            assert big, "no problem of 13 .. 32 columns: the search had nothing to take"
            asked = set(key for key, _, _ in calls)
            proven = 0
            for r in big:
                model = ru.restate(r["tint"], r["incomp"], r["remaining"])
                model["garbage"] = ru.garbage_costs(r["tint"], r["remaining"], "constant")
                model["max_lg"] = sum(s[2] for s in r["tint"]["segs"])
                greedy = cluster_solve.greedy_incumbent(model, settings)
                want = cluster_solve.exact_bnb(model, settings, None if greedy is None else greedy["cost2"])
                key = (r["tint"]["id"], r["partition"], r["round"])
                if want["status"] == "optimal":
                    assert key not in asked and (r["status"], r["cost"], r["x"], r["e"]) == ("OPTIMAL", want["cost"], want["x"], want["e"])
                    proven += 1
                elif want["status"] == "infeasible":
                    assert key not in asked and r["status"] == "NO_SOLUTION"
                else:
                    assert key in asked
            assert proven
    assert solved[0] and costs[32] == costs[0]
