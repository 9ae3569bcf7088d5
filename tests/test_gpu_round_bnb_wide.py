"""The branch and bound over a round's problems of up to 1024 columns on the GPU (fclu_round_bnb_wide) against the Python mirror
(cluster_solve.exact_bnb_wide), exactly: status, cost2, every mask word, node count and capped tasks of every problem, n_taken and
nodes_total.  The single-word sizes on the grid (where the mirror is also the 64-column definition); families of 63 .. 129 columns and the
two-optima tie in one call; a conflict pair, a gap row and a gap group beyond column 63; segment counts at the word and lane boundaries
of the segment side; random problems of more than 64 columns, proven and capped; 1024 columns; node caps, one task a launch, the node
budget, tables that do not fit, two rounds, a resident round, what stays valid behind the call, a call's times, the refusals, the loop with device_rounds
on a partition of more than 64 reps and the loop on files.

A tint's first and last segment are always informative, so a staged problem has at least one informative segment: the count 0 is run by
tools/bnb_wide_host_check.py on a model of its own (the same header code), and the counts here are 1, 2, 63, 64, 65 and 130."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

import cluster_util as cu
import round_util as ru
from freddie_amd import cluster, cluster_prep, cluster_solve
from test_gpu_incumbents import flips_tint, grid_tints
from test_gpu_round_bnb import BIG, SETTINGS, STATUS, family, garbage_of, models_of
from test_gpu_round_models import all_problems, stage

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

from bnb_host_check import family_tint  # noqa: E402
from bnb_wide_host_check import tie_tint  # noqa: E402

pytestmark = pytest.mark.gpu

WORDS = cluster_prep.BNB_WIDE_WORDS


@pytest.fixture(scope="module")
def ctx():
    c = cluster_prep.Context(0)
    yield c
    c.close()


def mirror(models, settings, ub2, min_cols, max_cols, depth, node_cap, max_nodes, narrow=False):
    """(per problem None (refused or not taken) or (status, cost2, mask, nodes, capped); problems taken), by the rule of
    include/freddie_cluster.h: a model, the sizes, tables that fit, then ascending (columns, problem) inside the budget.  narrow: a problem
    of at most 64 columns is also held against exact_bnb(), the 64-column definition."""
    want, n_taken, total = [None] * len(models), 0, 0
    fits = lambda m: cluster_prep.bnb_wide_lds_bytes(m["n_cols"], len(m["inf_seg"])) <= cluster_prep.BNB_WIDE_LDS_BYTES
    for R, p in sorted((m["n_cols"], p) for p, m in enumerate(models) if m["refused"] is None and min_cols <= m["n_cols"] <= max_cols and fits(m)):
        if total + (node_cap << min(R, depth)) > max_nodes:
            break
        n_taken, total = n_taken + 1, total + (node_cap << min(R, depth))
        bound = None if ub2[p] < 0 else int(ub2[p])
        got = cluster_solve.exact_bnb_wide(models[p], settings, bound, depth, node_cap)
        if narrow and R <= 64:
            assert got == cluster_solve.exact_bnb(models[p], settings, bound, depth, node_cap)
        want[p] = (STATUS[got["status"]], -1 if got["mask"] is None else got["cost2"], got["mask"] or 0, got["nodes"], got["capped"])
    return want, n_taken


def check(got, want, n_taken, problems):
    assert got["n_prob"] == len(want) == len(problems)
    assert got["n_taken"] == n_taken
    assert got["mask"].shape == (len(want), WORDS) and got["mask"].dtype == np.uint64
    for p, w in enumerate(want):
        words = [int(v) for v in got["mask"][p]]
        mine = (int(got["status"][p]), int(got["cost2"][p]), words, int(got["nodes"][p]), int(got["capped"][p]))
        solution = cluster_prep.round_bnb_wide_solution(got, p)
        if w is None:
            assert mine == (-2, -1, [0] * WORDS, 0, 0) and solution is None, (p, mine)
            continue
        assert mine == (w[0], w[1], [w[2] >> (64 * i) & (2 ** 64 - 1) for i in range(WORDS)], w[3], w[4]), (p, mine, w)
        x = [w[2] >> c & 1 for c in range(len(problems[p][2]))]
        if w[0] == 0:
            assert solution == (w[1] / 2.0, x)
        elif w[0] == 1:
            assert solution == "infeasible"
        else:
            assert solution == (("unproven", w[1] / 2.0, x) if w[1] >= 0 else ("unproven", None, None))
    assert got["nodes_total"] == sum(w[3] for w in want if w is not None)


def compare(ctx, tints, part0, problems, settings=SETTINGS, bound=True, min_cols=1, max_cols=1024, depth=6, node_cap=4096, max_nodes=BIG, narrow=False,
            resident=False):
    """One round on the device and through the mirror; bound: the device's greedy incumbents' cost2 bounds both."""
    models = models_of(tints, problems, settings)
    ctx.round_models([part0[t] + q for t, q, _ in problems], [rem for _, _, rem in problems], fetch=not resident)
    garbage = garbage_of(tints, problems, settings)
    ub2 = ctx.round_incumbents(garbage, settings["epsilon"], settings["offset"])["cost2"] if bound else np.full(len(problems), -1, np.int64)
    got = ctx.round_bnb_wide(garbage, ub2, settings["epsilon"], settings["offset"], min_cols, max_cols, max_nodes, depth, node_cap)
    want, n_taken = mirror(models, settings, ub2, min_cols, max_cols, depth, node_cap, max_nodes, narrow)
    check(got, want, n_taken, problems)
    return got, want


def whole(tints):
    return all_problems(tints, lambda t, q, rids: rids)


@pytest.mark.parametrize("max_ilp", [1000, 3])
def test_single_word_sizes_on_the_grid(ctx, max_ilp):
    """Every partition of the 80 grid tints in one call at min_cols = 1 and depth 3: R below, at and above the prefix depth, dead
    prefixes (max_ilp 3 brings pairs), refused problems left in.  One word a set: the mirror equals exact_bnb() on every one of them."""
    tints = grid_tints()
    part0 = stage(ctx, tints, maximum_ilp_size=max_ilp)
    problems = all_problems(tints, lambda t, q, rids: rids[::-1] if t % 3 == 0 else rids)
    for bound in (True, False):
        got, want = compare(ctx, tints, part0, problems, cluster.ilp_settings("exons" if max_ilp == 3 else "constant"), bound, depth=3, narrow=True)
        taken = [w for w in want if w is not None]
        assert all(w[4] == 0 for w in taken) and sum(w[0] == 0 for w in taken) > len(want) // 2 and any(w[2] for w in taken)
        sizes = set(len(rem) for _, _, rem in problems)
        assert min(sizes) < 3 and 3 in sizes and 4 in sizes
        if max_ilp == 1000:
            assert any(w is None for w in want)
    assert got["n_launches"] >= 1 and all(v >= 0 for v in ctx.round_bnb_wide_timing().values())


BOUNDARY_SHAPES = [(63, 31), (64, 32), (65, 64), (65, 32), (127, 64), (128, 64), (129, 128)]


@pytest.fixture(scope="module")
def boundary():
    return [family(t, R, n_low) for t, (R, n_low) in enumerate(BOUNDARY_SHAPES)] + [tie_tint(len(BOUNDARY_SHAPES))]


def boundary_problems():
    return [(t, 0, list(range(R))) for t, (R, _) in enumerate(BOUNDARY_SHAPES)] + [(len(BOUNDARY_SHAPES), 0, list(range(128)))]


def test_word_boundaries_and_the_tie(ctx, boundary):
    """Families of 63, 64, 65, 127, 128 and 129 columns and the 128-column tie in one call, so problems of one, two and three words share a
    launch: the optimum is exactly the upper family, and of the tie's two optimal sets -- columns 0 .. 63 and columns 64 .. 127, equal by
    the yardstick's cost -- the lower one wins."""
    tints = boundary
    part0 = stage(ctx, tints)
    assert [len(t["partitions"]) for t in tints] == [1] * len(tints)
    problems = boundary_problems()
    got, want = compare(ctx, tints, part0, problems)
    for (R, n_low), w in zip(BOUNDARY_SHAPES, want):
        assert w[0] == 0 and w[2] == ((1 << R) - 1) ^ ((1 << n_low) - 1) and w[4] == 0
    tie = tints[-1]
    incomp = tie["partitions"][0][1]
    low = ru.subset_cost(tie, incomp, list(range(128)), set(range(64)), SETTINGS)
    high = ru.subset_cost(tie, incomp, list(range(128)), set(range(64, 128)), SETTINGS)
    assert low is not None and low == high and want[-1][:3] == (0, int(2 * low), (1 << 64) - 1)
    assert got["n_launches"] == 1
    assert [int(v) for v in got["mask"][2][:2]] == [0, 1] and [int(v) for v in got["mask"][6][:3]] == [0, 0, 1]
    compare(ctx, tints, part0, [(t, q, rem[::-1]) for t, q, rem in problems], node_cap=512)               # (the families at the other end)
    compare(ctx, tints, part0, problems, bound=False, depth=2, node_cap=300)


def test_pairs_rows_and_groups_beyond_column_63(ctx):
    """A family of 6 reps with ones at the segments 1 .. 3 and one of 64 with zeros there, the columns in reverse, so that the 6 are the
    columns 64 .. 69: every conflict pair crosses the word, the gap group (0, 4) holds segments only columns from 64 on support, a
    member's row that its own support violates from below sits at column 67 and one that nothing violates at column 0; then the same
    in plain order."""
    tints = [family_tint(0, 70, 6, gaps={69: {(0, 4): 30}, 2: {(0, 4): 5}})[0], family_tint(1, 70, 6, gaps={69: {(0, 4): 2000}})[0]]
    part0 = stage(ctx, tints)
    assert [len(t["partitions"]) for t in tints] == [1, 1]
    for pick in (lambda rem: rem[::-1], lambda rem: rem):
        problems = [(t, 0, pick(list(range(70)))) for t in range(2)]
        models = models_of(tints, problems, SETTINGS)
        assert all(m["refused"] is None and len(m["pairs"]) == 6 * 64 and m["gap_rows"] for m in models)
        if pick([0, 1])[0]:
            assert sorted(c for c, _, _ in models[0]["gap_rows"]) == [0, 67] and all(a >= 64 > b or b >= 64 > a for a, b in models[0]["pairs"])
            k = models[0]["inf_seg"].index(2)
            assert min(models[0]["support"][k]) == 64
        for bound in (True, False):
            got, want = compare(ctx, tints, part0, problems, bound=bound, node_cap=600)
            assert all(w is not None for w in want) and want[0][1] >= 0
            assert want[1][1] == -1 and want[1][0] == (2 if want[1][4] else 1)     # (a gap of 2000 breaks its row inside and outside the set: no leaf)


SEGMENT_COUNTS = {1: (1, []), 2: (2, []), 63: (110, [3 + 5 * k for k in range(19)] + [100, 101]), 64: (115, [1] + [5 + 5 * k for k in range(20)]),
                  65: (110, [3 + 5 * k for k in range(21)]), 130: (220, [1] + [5 + 5 * k for k in range(42)])}


def counted_tint(tid, n, M, places):
    """n reps of all ones over M segments, rep i > 0 with a 0 at one of ``places`` in turn (one partition, as flips_tint()): the informative
    segments are the ends, the places and their neighbours.  Rep 1 has a gap around its place."""
    rows = []
    for i in range(n):
        row = [1] * M
        if i and places:
            row[places[(i - 1) % len(places)]] = 0
        rows.append(row)
    return ru.make_tint(tid, rows, {1: {(places[0] - 1, places[0] + 1): 3}} if places else None)


@pytest.mark.parametrize("E", sorted(SEGMENT_COUNTS))
def test_segment_counts(ctx, E):
    """70 columns over exactly 1, 2, 63, 64, 65 and 130 informative segments: the word and lane boundaries of the segment side."""
    M, places = SEGMENT_COUNTS[E]
    tints = [counted_tint(0, 70, M, places)]
    part0 = stage(ctx, tints)
    problems = whole(tints)
    models = models_of(tints, problems, SETTINGS)
    assert [(m["n_cols"], len(m["inf_seg"]), m["refused"]) for m in models] == [(70, E, None)]
    got, want = compare(ctx, tints, part0, problems, node_cap=256)
    assert want[0] is not None
    compare(ctx, tints, part0, [(0, 0, problems[0][2][::-1])], cluster.ilp_settings("introns"), bound=False, depth=3, node_cap=128)


def random_tints(seeds, n, M, with_gaps):
    tints = []
    for seed in seeds:
        rng = random.Random(seed)
        rows = ru.random_rows(rng, n, M, const_runs=seed % 2 == 0, flip=0.1)
        gaps, polys = ru.random_gaps(rng, rows, p=0.7) if with_gaps else ({}, {})
        tints.append(ru.make_tint(seed, rows, gaps, polys, members={i: rng.randrange(1, 4) for i in range(n)}))
    return tints


def test_random_problems_proven(ctx):
    """70 reps over 12 segments, seeds 1, 2 and 4, without gaps: whole partitions at depth 6 and node_cap 2^14.  The device's partitions
    are what is searched -- 69, 68 and 69 of the 70 reps with the pairs the pruning leaves, not the 70 columns without pairs of the
    host's figures: seed 1 is proven in 5 248 nodes, seeds 2 and 4 end with 64 and 15 capped tasks after 1 048 576 and 493 380 nodes, all
    of them the mirror's counts (which is what takes this test its fourteen seconds)."""
    tints = random_tints((1, 2, 4), 70, 12, False)
    part0 = stage(ctx, tints)
    problems = whole(tints)
    got, want = compare(ctx, tints, part0, problems, node_cap=1 << 14)
    assert any(w is not None and w[0] == 0 and w[3] > 1000 for w in want)


def test_random_problems_capped(ctx):
    """The same rows with gaps, staged with max_ilp 40 too (which brings pairs), at node_cap 4096 and 256: capped tasks, unproven
    problems, and proven ones beside them."""
    tints = random_tints((1, 2, 4), 70, 12, True) + random_tints((5,), 130, 12, True)
    ends = set()
    for max_ilp, node_cap in ((1000, 4096), (40, 256)):
        part0 = stage(ctx, tints, maximum_ilp_size=max_ilp)
        problems = whole(tints)
        got, want = compare(ctx, tints, part0, problems, node_cap=node_cap)
        ends |= set((w[0], w[4] > 0) for w in want if w is not None)
    assert (2, True) in ends and (0, False) in ends


def test_1024_columns(ctx):
    """1024 reps of one row, one partition, no gaps and no pairs, depth 0, node_cap 4096: sixteen words a set, one task, every column in
    after 1024 include children, a leaf and 1024 exclude children the bound drops."""
    tints = [ru.make_tint(0, [[1] * 8] * 1024)]
    part0 = stage(ctx, tints, maximum_ilp_size=1024)
    assert [len(rids) for rids, _ in tints[0]["partitions"]] == [1024]
    got, want = compare(ctx, tints, part0, whole(tints), depth=0)
    assert want[0][0] == 0 and want[0][2] == (1 << 1024) - 1 and want[0][3] == 2049
    assert [int(v) for v in got["mask"][0]] == [2 ** 64 - 1] * 16


@pytest.mark.parametrize("node_cap", [1, 7])
def test_node_caps(ctx, boundary, node_cap):
    """Every task stops at 1 resp. 7 nodes: capped tasks, unproven problems, every count the mirror's."""
    tints = boundary
    part0 = stage(ctx, tints)
    for bound in (True, False):
        got, want = compare(ctx, tints, part0, boundary_problems(), bound=bound, depth=2, node_cap=node_cap)
        assert all(w[0] == 2 and w[4] > 0 and w[3] <= 4 * node_cap for w in want)


def test_one_task_a_launch(ctx, boundary, monkeypatch):
    """FCLU_BNB_WIDE_SLICE=1: every task is a launch of its own, and a problem crosses launches; the results are the same."""
    tints = boundary
    part0 = stage(ctx, tints)
    problems = boundary_problems()[2:5]
    plain, want = compare(ctx, tints, part0, problems, depth=4)
    assert plain["n_launches"] == 1
    monkeypatch.setenv("FCLU_BNB_WIDE_SLICE", "1")
    sliced, _ = compare(ctx, tints, part0, problems, depth=4)
    assert sliced["n_launches"] == 3 * 16
    monkeypatch.setenv("FCLU_BNB_WIDE_SLICE", "11")
    some, _ = compare(ctx, tints, part0, problems, depth=4)
    assert 1 < some["n_launches"] < 16
    for k in ("status", "cost2", "mask", "nodes", "capped"):
        assert sliced[k].tolist() == plain[k].tolist() == some[k].tolist()


def test_the_budget_and_tables_that_do_not_fit(ctx):
    """Problems of 70, 66 and 68 columns at depth 4 and node_cap 10: 160 nodes of budget each, taken in ascending (columns, problem).  500
    reps with a flip of their own each leave about 1500 informative segments, 16 x 500 x 24 bytes of tables: not taken, whatever the
    budget."""
    tints = [flips_tint(0, 70, 44), flips_tint(1, 66, 44), flips_tint(2, 68, 44)]
    part0 = stage(ctx, tints)
    problems = whole(tints)
    for budget, taken in ((320, 2), (479, 2), (480, 3), (319, 1), (160, 1), (159, 0), (1, 0)):
        got, want = compare(ctx, tints, part0, problems, depth=4, node_cap=10, max_nodes=budget)
        assert got["n_taken"] == taken
        assert [w is not None for w in want] == [taken >= 3, taken >= 1, taken >= 2]
    got, want = compare(ctx, tints, part0, problems, min_cols=67, max_cols=69)
    assert [w is not None for w in want] == [False, False, True]
    got, want = compare(ctx, tints, part0, problems, min_cols=0, max_cols=0)
    assert want == [None] * 3 and (got["n_taken"], got["n_launches"], got["nodes_total"]) == (0, 0, 0)
    big = [flips_tint(0, 500, 2600), flips_tint(1, 66, 44)]
    part0 = stage(ctx, big)
    problems = whole(big)
    models = models_of(big, problems, SETTINGS)
    wide = [p for p, m in enumerate(models) if cluster_prep.bnb_wide_lds_bytes(m["n_cols"], len(m["inf_seg"])) > cluster_prep.BNB_WIDE_LDS_BYTES]
    assert wide and cluster_prep.bnb_wide_lds_bytes(1024, 576) <= cluster_prep.BNB_WIDE_LDS_BYTES < cluster_prep.bnb_wide_lds_bytes(1024, 577)
    got, want = compare(ctx, big, part0, problems, min_cols=0, node_cap=64)
    assert all(want[p] is None for p in wide) and want[-1] is not None


def test_two_rounds_a_resident_round_and_what_stays_valid(ctx, boundary):
    """Two rounds on one context, each followed by one behind a resident round; behind the call the round's own results, the incumbents',
    the exact call's and the 64-column search's are where they were."""
    tints = grid_tints()[::8] + boundary[1:4]
    part0 = stage(ctx, tints)
    for pick in (lambda t, q, rids: rids, lambda t, q, rids: rids[1::2][::-1]):
        problems = all_problems(tints, pick)
        models = models_of(tints, problems, SETTINGS)
        arr = ctx.round_models([part0[t] + q for t, q, _ in problems], [rem for _, _, rem in problems])
        garbage = garbage_of(tints, problems, SETTINGS)
        inc = ctx.round_incumbents(garbage, SETTINGS["epsilon"], SETTINGS["offset"])
        exact = ctx.round_exact(garbage, SETTINGS["epsilon"], SETTINGS["offset"], 12, 1 << 40)
        bnb = ctx.round_bnb(garbage, inc["cost2"], SETTINGS["epsilon"], SETTINGS["offset"], 13, 64, BIG, 3, 4096)
        got = ctx.round_bnb_wide(garbage, inc["cost2"], SETTINGS["epsilon"], SETTINGS["offset"], 1, 1024, BIG, 3, 4096)
        check(got, *mirror(models, SETTINGS, inc["cost2"], 1, 1024, 3, 4096, BIG), problems)
        r = cluster_prep._Rounds()
        assert ctx._L.fclu_round_results(ctx._h, ctypes.byref(r)) == 0 and r.n_prob == len(problems)
        assert cluster_prep._copy_out(r.inf_seg, int(r.n_inf), np.int32).tolist() == arr["inf_seg"].tolist()
        assert cluster_prep._copy_out(r.rows, 3 * int(r.n_gap_rows), np.int32).tolist() == arr["rows"].reshape(-1).tolist()
        i = cluster_prep._Incumbents()
        assert ctx._L.fclu_round_incumbent_results(ctx._h, ctypes.byref(i)) == 0 and i.n_prob == len(problems)
        assert cluster_prep._copy_out(i.cost2, i.n_prob, np.int64).tolist() == inc["cost2"].tolist()
        assert cluster_prep._copy_out(i.mem, int(i.n_mem), np.int32).tolist() == inc["mem"].tolist()
        x = cluster_prep._Exact()
        assert ctx._L.fclu_round_exact_results(ctx._h, ctypes.byref(x)) == 0 and x.n_prob == len(problems)
        assert cluster_prep._copy_out(x.cost2, x.n_prob, np.int64).tolist() == exact["cost2"].tolist()
        assert cluster_prep._copy_out(x.mask, x.n_prob, np.uint32).tolist() == exact["mask"].tolist()
        b = cluster_prep._Bnb()
        assert ctx._L.fclu_round_bnb_results(ctx._h, ctypes.byref(b)) == 0 and b.n_prob == len(problems)
        for key, dtype in (("status", np.int32), ("cost2", np.int64), ("mask", np.uint64), ("nodes", np.int64)):
            assert cluster_prep._copy_out(getattr(b, key), b.n_prob, dtype).tolist() == bnb[key].tolist()
        for p in range(len(problems)):                       # the searches and the enumeration agree problem for problem
            if got["status"][p] == 0 and exact["cost2"][p] >= 0:
                assert (int(got["cost2"][p]), int(got["mask"][p][0])) == (int(exact["cost2"][p]), int(exact["mask"][p]))
            if bnb["status"][p] >= 0:
                assert (int(got["status"][p]), int(got["cost2"][p]), int(got["mask"][p][0]), int(got["nodes"][p])) == (
                    int(bnb["status"][p]), int(bnb["cost2"][p]), int(bnb["mask"][p]), int(bnb["nodes"][p]))
        compare(ctx, tints, part0, problems, resident=True, depth=3)


def test_a_calls_times_are_its_own(ctx, boundary, monkeypatch):
    """The three searches one after another on one context, calls of many launches between calls of one: every call's times are finite
    and not negative, stay what they were behind the later calls, and where a call had one launch its longest launch is its whole search
    -- the elapsed time between the same two events, so equal to the bit."""
    tints = [flips_tint(0, 12, 44)] + boundary[1:4]
    part0 = stage(ctx, tints)
    problems = whole(tints)
    ctx.round_models([part0[t] + q for t, q, _ in problems], [rem for _, _, rem in problems])
    garbage = garbage_of(tints, problems, SETTINGS)
    ub2 = ctx.round_incumbents(garbage, SETTINGS["epsilon"], SETTINGS["offset"])["cost2"]
    args = (SETTINGS["epsilon"], SETTINGS["offset"])

    def sound(got, times):
        assert all(np.isfinite(v) and v >= 0 for v in times.values()), times
        if got["n_launches"] == 1:
            assert times["longest_launch_ms"] == times["search_ms"], times
        return times

    monkeypatch.setenv("FCLU_EXACT_SLICE", "64")
    exact = ctx.round_exact(garbage, *args, 12, 1 << 40)
    t_exact = sound(exact, ctx.round_exact_timing())
    assert exact["n_launches"] > 1
    bnb = ctx.round_bnb(garbage, ub2, *args, 1, 64, BIG, 3, 4096)
    t_bnb = sound(bnb, ctx.round_bnb_timing())
    assert bnb["n_launches"] == 1 and bnb["n_taken"] >= 1
    monkeypatch.setenv("FCLU_BNB_WIDE_SLICE", "1")
    wide = ctx.round_bnb_wide(garbage, ub2, *args, 1, 1024, BIG, 3, 4096)
    t_wide = sound(wide, ctx.round_bnb_wide_timing())
    assert wide["n_launches"] > exact["n_launches"]
    assert ctx.round_exact_timing() == t_exact and ctx.round_bnb_timing() == t_bnb
    again = ctx.round_bnb(garbage, ub2, *args, 1, 64, BIG, 3, 4096)
    t_again = sound(again, ctx.round_bnb_timing())
    assert again["n_launches"] == 1
    assert ctx.round_exact_timing() == t_exact and ctx.round_bnb_wide_timing() == t_wide and ctx.round_bnb_timing() == t_again


def test_refusals(ctx):
    fresh = cluster_prep.Context(0)
    try:
        with pytest.raises(cluster_prep.ClusterError) as e:
            fresh.round_bnb_wide([], [], 0.2, 20, 1, 1024, BIG)
        assert e.value.code == 1
        assert fresh._L.fclu_round_bnb_wide(fresh._h, None, None, 0.8, 1.2, 20, 1, 1024, 6, 4096, 1000) == 1           # FCLU_ERR_ARG
        assert b"fclu_round_models" in fresh._L.fclu_last_error(fresh._h)
        b = cluster_prep._Bnb()
        assert fresh._L.fclu_round_bnb_wide_results(fresh._h, ctypes.byref(b)) == 1
    finally:
        fresh.close()
    tints = [flips_tint(0, 66, 44), flips_tint(1, 5, 12)]
    part0 = stage(ctx, tints)
    problems = whole(tints)
    compare(ctx, tints, part0, problems, node_cap=64)
    none = [-1, -1]
    for garbage, word in (([3.0] * 70 + [3.25], "multiple of 0.5"), ([3.0] * 70, "70 garbage costs"), ([3.0] * 70 + [-1.0], "multiple of 0.5")):
        with pytest.raises(cluster_prep.ClusterError, match=word):
            ctx.round_bnb_wide(garbage, none, 0.2, 20, 1, 1024, BIG)
    with pytest.raises(cluster_prep.ClusterError, match="3 bounds"):
        ctx.round_bnb_wide([3.0] * 71, [-1] * 3, 0.2, 20, 1, 1024, BIG)
    for min_cols, max_cols, depth, node_cap, max_nodes, word in ((1, 1025, 6, 4096, BIG, "max_cols"), (-1, 1024, 6, 4096, BIG, "min_cols"), (9, 8, 6, 4096, BIG, "min_cols"),
                                                                 (1, 1024, 21, 4096, BIG, "depth"), (1, 1024, -1, 4096, BIG, "depth"), (1, 1024, 6, 0, BIG, "node_cap"),
                                                                 (1, 1024, 6, 4096, 0, "max_nodes"), (1, 1024, 6, 4096, -5, "max_nodes")):
        with pytest.raises(cluster_prep.ClusterError, match=word) as e:
            ctx.round_bnb_wide([3.0] * 71, none, 0.2, 20, min_cols, max_cols, max_nodes, depth, node_cap)
        assert e.value.code == 1
    g2, ub2 = np.full(71, 6, np.int32), np.full(2, -1, np.int64)
    call = lambda g, u, offset=20, node_cap=64, max_nodes=BIG: ctx._L.fclu_round_bnb_wide(ctx._h, g, u, 0.8, 1.2, offset, 1, 1024, 6, node_cap, max_nodes)
    assert call(g2.ctypes.data, ub2.ctypes.data, offset=-1) == 1
    assert call(None, ub2.ctypes.data) == 1 and b"g2 is null" in ctx._L.fclu_last_error(ctx._h)
    assert call(g2.ctypes.data, None) == 1 and b"ub2 is null" in ctx._L.fclu_last_error(ctx._h)
    g2[4] = -1
    assert call(g2.ctypes.data, ub2.ctypes.data) == 1 and b"g2[4]" in ctx._L.fclu_last_error(ctx._h)
    g2[4] = 6
    assert call(g2.ctypes.data, ub2.ctypes.data) == 0
    assert ctx._L.fclu_round_bnb_wide(ctx._h, g2.ctypes.data, ub2.ctypes.data, float("nan"), 1.2, 20, 1, 1024, 6, 64, BIG) == 1
    compare(ctx, tints, part0, problems, node_cap=64)                                       # the context stays usable
    many = [flips_tint(t, 13, 12) for t in range(3)]
    part0 = stage(ctx, many)
    probs = whole(many)
    ctx.round_models([part0[t] + q for t, q, _ in probs], [rem for _, _, rem in probs])
    with pytest.raises(cluster_prep.ClusterError, match="launches") as e:                     # 3 x 2^13 tasks, one a launch
        ctx.round_bnb_wide([3.0] * 39, [-1] * 3, 0.2, 20, 1, 1024, 1 << 62, 13, 1 << 30)
    assert e.value.code == cluster_prep.ERR_UNSUPPORTED
    part0 = stage(ctx, tints)
    compare(ctx, tints, part0, problems, node_cap=64)
    host = cu.random_tint(3, 30, 20)
    cluster_prep.partition_reads_batch([host], 1000, ctx, verbose=False)                    # fclu_partition ends the rounds' source
    assert call(g2.ctypes.data, ub2.ctypes.data) == 1
    with pytest.raises(cluster_prep.ClusterError):
        ctx.round_bnb_wide([3.0] * 71, none, 0.2, 20, 1, 1024, BIG)
    part0 = stage(ctx, tints)
    compare(ctx, tints, part0, problems, node_cap=64)


def test_the_loop_with_device_rounds_on_a_partition_of_70_reps(ctx):
    """cluster_tints() under wide_cols = 128 on a staged tint whose one partition holds 70 reps (72 with the two that tie the families):
    the first round's set is proven by the wide search, and with device_rounds on it goes through round_readout -- the records, the logs
    and the isoforms are those of the run with device_rounds off, and no solve job is made for a proven problem."""
    got = {}
    for flag in (False, True):
        tints = [family_tint(0, 70, 6)[0]]
        part0 = stage(ctx, tints)
        assert len(tints[0]["partitions"]) == 1 and len(tints[0]["partitions"][0][0]) == 72
        record, jobs = [], []
        settings = cluster.ilp_settings(min_isoform_size=2, wide_cols=128, device_rounds=flag)
        logs = cluster.cluster_tints(tints, part0, ctx, settings, solve=lambda m, s: jobs.append(m["n_cols"]) or cluster_solve.solve_round(m, s),
                                     on_round=lambda r: record.append((r["partition"], r["round"], r["remaining"], r["status"], r["x"], r["e"], r["cost"])))
        got[flag] = (logs, record, [(t["isoforms"], t["garbage_rids"]) for t in tints])
        assert record[0][3] == "OPTIMAL" and len(record[0][4]) == 72 and any(record[0][4][64:]) and all(n <= 64 for n in jobs)
        assert sorted(tints[0]["isoforms"][0]["rid_to_corrections"]) == sorted(record[0][2][c] for c, v in enumerate(record[0][4]) if v)
    assert got[True] == got[False]


def test_the_loop_on_files(ctx, tmp_path):
    """cluster_files() under exact_cols = 12, bnb_cols = 14, wide_cols = 32 on fixture files staged with max_ilp = 20: problems of 15 ..
    20 columns go to the wide search.  Where every taken problem of the first round is proven its costs are those of the run with
    wide_cols = 0 (the tie rule may pick another optimal set than HiGHS, so later rounds can differ); a proven problem never reaches the
    solver."""
    paths = []
    for name in ("e_plateau_touch", "g1_dense", "g1_retention"):
        paths.append(cu.segment_tsv_file(name, tmp_path))
    costs, solved = {}, {}
    for wide_cols in (32, 0):
        record, calls = [], []

        def solve(model, settings):
            calls.append((model["key"], model["n_cols"], model.get("incumbent")))
            return cluster_solve.solve_round(model, settings)

        settings = cluster.ilp_settings(max_ilp=20, exact_cols=12, bnb_cols=14, wide_cols=wide_cols, max_rounds=30 if wide_cols else 1)
        out = list(cluster.cluster_files(paths, settings, ctx=ctx, solve=solve, on_round=record.append))
        assert len(out) == len(paths) and len(record) > 5
        costs[wide_cols] = sorted((r["tint"]["id"], r["partition"], r["status"], r["cost"]) for r in record if r["round"] == 0)
        solved[wide_cols] = calls
        if wide_cols:
            big = [r for r in record if 14 < len(r["remaining"]) <= 32]
            assert big, "no problem of 15 .. 32 columns: the search had nothing to take"
            asked = set(key for key, _, _ in calls)
            proven = 0
            for r in big:
                model = ru.restate(r["tint"], r["incomp"], r["remaining"])
                model["garbage"] = ru.garbage_costs(r["tint"], r["remaining"], "constant")
                model["max_lg"] = sum(s[2] for s in r["tint"]["segs"])
                greedy = cluster_solve.greedy_incumbent(model, settings)
                want = cluster_solve.exact_bnb_wide(model, settings, None if greedy is None else greedy["cost2"],
                                                    node_cap=cluster_solve.bnb_wide_node_cap(32))
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
