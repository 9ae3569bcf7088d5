"""The exact small-problem solve on the GPU (fclu_round_exact) against the Python mirror (cluster_solve.exact_small), exactly: cost2,
mask and taken or not of every problem, on the grid of small problems in one batch (refused problems left in) and on hand-built ones
where the kernels can go wrong -- one column, the column limit, segment counts around word boundaries, a set every pair of which is in
conflict, a tie between two columns, a problem without a feasible subset, the epsilon 0.15 boundary row, half-integer costs, the mask
budget, many slices and several launches, two rounds on one context -- then what stays valid behind the call, the refusals and the loop."""
import ctypes
import random

import numpy as np
import pytest

import cluster_util as cu
import round_util as ru
from freddie_amd import cluster, cluster_prep, cluster_solve
from test_gpu_incumbents import flips_tint, grid_tints, star_tint
from test_gpu_round_models import all_problems, stage

pytestmark = pytest.mark.gpu

SETTINGS = cluster.ilp_settings()
BIG = 1 << 40


@pytest.fixture(scope="module")
def ctx():
    c = cluster_prep.Context(0)
    yield c
    c.close()


def mirror(tints, problems, settings, max_cols, max_masks):
    """(per problem -2 (refused or not taken), (-1, 0) (no feasible subset) or (cost2, mask); problems taken; masks evaluated), by the
    rule of include/freddie_cluster.h: ascending (columns, problem) while the running total of 2^R stays inside the budget."""
    models = []
    for t, q, rem in problems:
        model = ru.restate(tints[t], tints[t]["partitions"][q][1], rem)
        model["garbage"] = ru.garbage_costs(tints[t], rem, settings["recycle_model"])
        model["max_lg"] = sum(s[2] for s in tints[t]["segs"])
        models.append(model)
    want, n_taken, n_masks = [-2] * len(problems), 0, 0
    for R, p in sorted((m["n_cols"], p) for p, m in enumerate(models) if m["refused"] is None and m["n_cols"] <= max_cols):
        if n_masks + (1 << R) > max_masks:
            break
        n_taken, n_masks = n_taken + 1, n_masks + (1 << R)
        got = cluster_solve.exact_small(models[p], settings)
        want[p] = (-1, 0) if got is None else (got["cost2"], got["mask"])
    return want, n_taken, n_masks


def garbage_of(tints, problems, settings):
    return [g for t, _, rem in problems for g in ru.garbage_costs(tints[t], rem, settings["recycle_model"])]


def device(ctx, tints, part0, problems, settings, max_cols, max_masks):
    arr = ctx.round_models([part0[t] + q for t, q, _ in problems], [rem for _, _, rem in problems])
    return arr, ctx.round_exact(garbage_of(tints, problems, settings), settings["epsilon"], settings["offset"], max_cols, max_masks)


def check(got, want, n_taken, n_masks, problems):
    assert got["n_prob"] == len(want) == len(problems)
    assert (got["n_taken"], got["n_masks"]) == (n_taken, n_masks)
    for p, w in enumerate(want):
        mine = (int(got["cost2"][p]), int(got["mask"][p]))
        solution = cluster_prep.round_exact_solution(got, p)
        if w == -2:
            assert mine == (-2, 0) and solution is None, (p, mine)
        elif w[0] == -1:
            assert mine == (-1, 0) and solution == "infeasible", (p, mine)
        else:
            assert mine == w, (p, mine, w)
            assert solution == (w[0] / 2.0, [w[1] >> c & 1 for c in range(len(problems[p][2]))])


def compare(ctx, tints, part0, problems, settings=SETTINGS, max_cols=12, max_masks=BIG):
    want, n_taken, n_masks = mirror(tints, problems, settings, max_cols, max_masks)
    arr, got = device(ctx, tints, part0, problems, settings, max_cols, max_masks)
    check(got, want, n_taken, n_masks, problems)
    return got, want


@pytest.mark.parametrize("max_ilp", [1000, 3])
@pytest.mark.parametrize("recycle_model", cluster_solve.RECYCLE_MODELS)
def test_grid_in_one_batch(ctx, recycle_model, max_ilp):
    """Every partition of the 80 grid tints in ONE call, the refused problems among them (-2), the infeasible ones (-1) and the rest the
    mirror's.  max_ilp 3 splits the components, which is where incompatible pairs come from; the reps weigh 1 .. 3 reads, so the costs
    under exons / introns are half-integers."""
    tints = grid_tints()
    part0 = stage(ctx, tints, maximum_ilp_size=max_ilp)
    problems = all_problems(tints, lambda t, q, rids: rids[::-1] if t % 3 == 0 else rids)
    got, want = compare(ctx, tints, part0, problems, cluster.ilp_settings(recycle_model))
    solved = [w for w in want if w != -2 and w[0] >= 0]
    assert len(solved) > len(want) // 2 and any(w[1] for w in solved)
    if max_ilp == 1000:
        assert any(w == -2 for w in want) and any(w != -2 and w[0] == -1 for w in want)
    else:
        assert sum(len(inc) for tint in tints for _, inc in tint["partitions"]) > 0
    if recycle_model != "constant":
        assert any(w[0] % 2 for w in solved)
    assert got["n_launches"] >= 1 and all(v >= 0 for v in ctx.round_exact_timing().values())


def test_one_column_the_column_limit_and_no_columns_allowed(ctx):
    """R = 1; R = max_cols is taken and R = max_cols + 1 is not, in one batch; max_cols = 0 takes nothing and launches nothing."""
    tints = [flips_tint(0, 1, 12), flips_tint(1, 5, 12), flips_tint(2, 6, 12), flips_tint(3, 4, 12)]
    part0 = stage(ctx, tints)
    assert [len(t["partitions"]) for t in tints] == [1] * 4
    problems = all_problems(tints, lambda t, q, rids: rids)
    got, want = compare(ctx, tints, part0, problems, max_cols=5)
    assert want[0] == (0, 1) and want[1] != -2 and want[2] == -2 and want[3] != -2
    got, want = compare(ctx, tints, part0, problems, max_cols=0)
    assert want == [-2] * 4 and (got["n_taken"], got["n_masks"], got["n_launches"]) == (0, 0, 0)
    got, want = compare(ctx, tints, part0, all_problems(tints, lambda t, q, rids: rids[:1]), max_cols=1)
    assert all(w == (0, 1) for w in want)
    got, want = compare(ctx, tints, part0, all_problems(tints, lambda t, q, rids: []), max_cols=3, max_masks=4)     # no column: the empty set, cost 0
    assert want == [(0, 0)] * 4 and (got["n_taken"], got["n_masks"]) == (4, 4)


@pytest.mark.parametrize("M", [1, 2, 31, 32, 33, 64, 65])
def test_segment_counts(ctx, M):
    rng = random.Random(M)
    rows = ru.random_rows(rng, 10, M)
    tints = [ru.make_tint(7, rows, *ru.random_gaps(rng, rows), members={i: rng.randrange(1, 4) for i in range(10)}), flips_tint(1, 9, max(M, 8))]
    part0 = stage(ctx, tints)
    for recycle_model in ("constant", "introns"):
        got, want = compare(ctx, tints, part0, all_problems(tints, lambda t, q, rids: rids), cluster.ilp_settings(recycle_model))
        assert any(w != -2 and w[0] >= 0 for w in want)
    compare(ctx, tints, part0, all_problems(tints, lambda t, q, rids: rng.sample(rids, (len(rids) + 1) // 2)))


def test_every_pair_in_conflict_and_the_tie(ctx):
    """The leaves of a star without its centre: every pair is in conflict, so the optimum is one column or none; every leaf costs the same,
    and the smallest mask -- column 0 whatever rep stands there -- wins.  Two leaves alone: {0} and {1} tie, {0} it is."""
    tints = [star_tint(0, 9), star_tint(1, 9)]
    part0 = stage(ctx, tints)
    assert [len(t["partitions"]) for t in tints] == [1, 1] and len(tints[0]["partitions"][0][1]) == 36
    problems = [(0, 0, [5, 3, 8, 0, 1, 2, 4, 7, 6]), (1, 0, list(range(10))[::-1])]
    got, want = compare(ctx, tints, part0, problems)
    assert want[0] == (2 * 3 * 8, 1) and bin(want[1][1]).count("1") == 2 and want[1][1] & 1
    two = [(0, 0, [5, 3])]
    got, want = compare(ctx, tints, part0, two)
    costs = [ru.subset_cost(tints[0], tints[0]["partitions"][0][1], [5, 3], chosen, SETTINGS) for chosen in ({0}, {1}, {0, 1})]
    assert costs[0] == costs[1] == want[0][0] / 2.0 and costs[2] is None and want[0][1] == 1
    got, want = compare(ctx, tints, part0, problems[:1], cluster.ilp_settings(offset=0, epsilon=0.0))


def test_a_gap_nothing_satisfies(ctx):
    """A gap of 500 > offset + MAX_ISOFORM_LG (20 + 213) breaks its rep's row inside and outside the set: -1, beside a feasible problem."""
    tints = [flips_tint(0, 8, 12, {3: {(2, 9): 500}}), flips_tint(1, 8, 12, {3: {(2, 9): 5}})]
    part0 = stage(ctx, tints)
    problems = all_problems(tints, lambda t, q, rids: rids)
    got, want = compare(ctx, tints, part0, problems)
    column = problems[1][2].index(3)                         # (a partition lists its reps node by node)
    assert want[0] == (-1, 0) and want[1][0] >= 0 and want[1][1] == 0xff ^ (1 << column)


def test_the_boundary_row(ctx):
    """epsilon 0.15, offset 20: the group of rep 0's gap (2, 9) is the segments 3, 4, 7, 8 of 50 each, 200 once every rep is in.  l = 250
    holds with equality in rationals and only by the model's tolerance in doubles: everything joins; l = 251 does not hold: rep 0 stays out."""
    lens = [10, 10, 10, 50, 50, 10, 10, 50, 50, 10, 10, 10]
    tints = [flips_tint(0, 8, 12, {0: {(2, 9): 250}}, lens), flips_tint(1, 8, 12, {0: {(2, 9): 251}}, lens)]
    part0 = stage(ctx, tints)
    settings = cluster.ilp_settings(epsilon=0.15)
    got, want = compare(ctx, tints, part0, all_problems(tints, lambda t, q, rids: rids), settings)
    assert want == [(14, 0xff), (20, 0xfe)]
    got, want = compare(ctx, tints, part0, all_problems(tints, lambda t, q, rids: rids))           # (epsilon 0.2: both hold)
    assert want == [(14, 0xff), (14, 0xff)]


def test_the_budget(ctx):
    """Problems of 8, 3 and 5 columns: a budget of 8 + 32 masks admits the two small ones, and so does every budget short of 8 + 32 + 256."""
    tints = [flips_tint(0, 8, 12), flips_tint(1, 3, 12), flips_tint(2, 5, 12)]
    part0 = stage(ctx, tints)
    problems = all_problems(tints, lambda t, q, rids: rids)
    for budget, taken, masks in ((40, 2, 40), (295, 2, 40), (296, 3, 296), (39, 1, 8), (7, 0, 0), (1, 0, 0)):
        got, want = compare(ctx, tints, part0, problems, max_masks=budget)
        assert (got["n_taken"], got["n_masks"]) == (taken, masks)
        assert [w != -2 for w in want] == [taken >= 3, taken >= 1, taken >= 2]


def test_many_slices_and_launches(ctx, monkeypatch):
    """A 12-column problem with 64 masks a workgroup and 1024 a launch: 64 slices, 4 launches, the same answer; small problems beside it."""
    tints = [flips_tint(0, 12, 44, {5: {(2, 9): 3}}), flips_tint(1, 3, 12)]
    part0 = stage(ctx, tints)
    problems = all_problems(tints, lambda t, q, rids: rids)
    plain, want = compare(ctx, tints, part0, problems, cluster.ilp_settings("exons"))
    assert plain["n_launches"] == 1 and want[0][1] not in (0, 0xfff)
    monkeypatch.setenv("FCLU_EXACT_SLICE", "64")
    sliced, _ = compare(ctx, tints, part0, problems, cluster.ilp_settings("exons"))
    assert sliced["n_launches"] > 1 and sliced["n_masks"] == 4096 + 8
    assert sliced["cost2"].tolist() == plain["cost2"].tolist() and sliced["mask"].tolist() == plain["mask"].tolist()


def test_two_rounds_and_what_stays_valid(ctx):
    """Two rounds on one context; behind the exact call the round's own results and the incumbents' are where they were."""
    tints = grid_tints()[::5]
    part0 = stage(ctx, tints)
    for pick in (lambda t, q, rids: rids, lambda t, q, rids: rids[1::2][::-1]):
        problems = all_problems(tints, pick)
        arr = ctx.round_models([part0[t] + q for t, q, _ in problems], [rem for _, _, rem in problems])
        garbage = garbage_of(tints, problems, SETTINGS)
        inc = ctx.round_incumbents(garbage, SETTINGS["epsilon"], SETTINGS["offset"])
        got = ctx.round_exact(garbage, SETTINGS["epsilon"], SETTINGS["offset"], 12, BIG)
        check(got, *mirror(tints, problems, SETTINGS, 12, BIG), problems)
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
        for p in range(len(problems)):                       # a proven optimum is never worse than the greedy's set
            if inc["cost2"][p] >= 0:
                assert 0 <= got["cost2"][p] <= inc["cost2"][p]


def test_refusals(ctx):
    fresh = cluster_prep.Context(0)
    try:
        with pytest.raises(cluster_prep.ClusterError) as e:
            fresh.round_exact([], 0.2, 20, 12, BIG)
        assert e.value.code == 1
        assert fresh._L.fclu_round_exact(fresh._h, None, 0.8, 1.2, 20, 12, 1000) == 1                # FCLU_ERR_ARG
        assert b"fclu_round_models" in fresh._L.fclu_last_error(fresh._h)
        x = cluster_prep._Exact()
        assert fresh._L.fclu_round_exact_results(fresh._h, ctypes.byref(x)) == 1
    finally:
        fresh.close()
    tints = [flips_tint(0, 8, 12), flips_tint(1, 5, 12)]
    part0 = stage(ctx, tints)
    problems = all_problems(tints, lambda t, q, rids: rids)
    compare(ctx, tints, part0, problems)
    for garbage, word in (([3.0] * 12 + [3.25], "multiple of 0.5"), ([3.0] * 12, "12 garbage costs"), ([3.0] * 12 + [-1.0], "multiple of 0.5")):
        with pytest.raises(cluster_prep.ClusterError, match=word):
            ctx.round_exact(garbage, 0.2, 20, 12, BIG)
    for max_cols, max_masks, word in ((25, BIG, "max_cols"), (-1, BIG, "max_cols"), (12, 0, "max_masks"), (12, -5, "max_masks")):
        with pytest.raises(cluster_prep.ClusterError, match=word) as e:
            ctx.round_exact([3.0] * 13, 0.2, 20, max_cols, max_masks)
        assert e.value.code == 1
    g2 = np.full(13, 6, np.int32)
    assert ctx._L.fclu_round_exact(ctx._h, g2.ctypes.data, 0.8, 1.2, -1, 12, 1000) == 1
    g2[4] = -1
    assert ctx._L.fclu_round_exact(ctx._h, g2.ctypes.data, 0.8, 1.2, 20, 12, 1000) == 1
    assert b"g2[4]" in ctx._L.fclu_last_error(ctx._h)
    g2[4] = 6
    compare(ctx, tints, part0, problems)                                                    # the context stays usable
    host = cu.random_tint(3, 30, 20)
    cluster_prep.partition_reads_batch([host], 1000, ctx, verbose=False)                    # fclu_partition ends the rounds' source
    assert ctx._L.fclu_round_exact(ctx._h, g2.ctypes.data, 0.8, 1.2, 20, 12, 1000) == 1
    with pytest.raises(cluster_prep.ClusterError):
        ctx.round_exact([3.0] * 13, 0.2, 20, 12, BIG)
    part0 = stage(ctx, tints)
    compare(ctx, tints, part0, problems)


def test_the_loop_on_files(ctx, tmp_path):
    """cluster_files() with exact_cols = 12 on fixture files staged with max_ilp = 7: no problem is larger, so the solver is never called;
    every round's cost is the mirror's for that round's remaining reps, and the first rounds' costs are those of the plain run (later
    rounds may differ where HiGHS breaks a tie another way, so the plain run stops behind its first)."""
    paths = []
    for name in ("e_plateau_touch", "g1_dense", "g1_retention"):
        paths.append(cu.segment_tsv_file(name, tmp_path))

    def solve(model, settings):
        assert model["n_cols"] > 12, "a model of %d columns reached the solver" % model["n_cols"]
        return cluster_solve.solve_round(model, settings)

    costs = {}
    for exact_cols in (12, 0):
        record = []
        settings = cluster.ilp_settings(max_ilp=7, exact_cols=exact_cols, max_rounds=30 if exact_cols else 1)
        out = list(cluster.cluster_files(paths, settings, ctx=ctx, solve=solve if exact_cols else cluster_solve.solve_round, on_round=record.append))
        assert len(out) == len(paths) and len(record) > 20
        costs[exact_cols] = sorted((r["tint"]["id"], r["partition"], r["status"], r["cost"]) for r in record if r["round"] == 0)
        if exact_cols:
            assert any(r["incomp"] for r in record) and any(r["round"] > 0 for r in record)
            for r in record:
                model = ru.restate(r["tint"], r["incomp"], r["remaining"])
                model["garbage"] = ru.garbage_costs(r["tint"], r["remaining"], "constant")
                model["max_lg"] = sum(s[2] for s in r["tint"]["segs"])
                want = cluster_solve.exact_small(model, settings)
                assert (r["status"], r["cost"]) == (("NO_SOLUTION", None) if want is None else ("OPTIMAL", want["cost"]))
                if want is not None:
                    assert r["x"] == want["x"] and r["e"] == want["e"]
    assert costs[12] == costs[0]
