"""The greedy round incumbents on the GPU (fclu_round_incumbents) against the Python mirror (cluster_solve.greedy_incumbent), exactly:
cost2, chosen start, members and both step counts of every problem, on a grid of small problems in one batch (refused problems left
in) and on hand-built ones where the kernels can go wrong -- one column, columns and segments around word boundaries, a set every pair
of which is in conflict, ties between columns and between starts, repair by one member and down to the empty set, a problem without a
feasible start, few and many seeds, both row paths in one batch, two rounds on one context -- then the refusals and the command line."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import cluster_util as cu
import round_util as ru
from freddie_amd import cluster, cluster_prep, cluster_solve
from test_gpu_round_models import all_problems, big_tint, stage

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = cluster.ilp_settings()


@pytest.fixture(scope="module")
def ctx():
    c = cluster_prep.Context(0)
    yield c
    c.close()


def mirror(tints, problems, settings, max_seeds):
    """Per problem None (refused), or (the mirror's result or None when no start is feasible,)."""
    out = []
    for t, q, rem in problems:
        model = ru.restate(tints[t], tints[t]["partitions"][q][1], rem)
        if model["refused"] is not None:
            out.append(None)
            continue
        model["garbage"] = ru.garbage_costs(tints[t], rem, settings["recycle_model"])
        model["max_lg"] = sum(s[2] for s in tints[t]["segs"])
        out.append((cluster_solve.greedy_incumbent(model, settings, max_seeds),))
    return out


def device(ctx, tints, part0, problems, settings, max_seeds):
    arr = ctx.round_models([part0[t] + q for t, q, _ in problems], [rem for _, _, rem in problems])
    garbage = [g for t, _, rem in problems for g in ru.garbage_costs(tints[t], rem, settings["recycle_model"])]
    return arr, ctx.round_incumbents(garbage, settings["epsilon"], settings["offset"], max_seeds)


def check(inc, want, problems):
    assert inc["n_prob"] == len(want) == len(problems)
    for p, w in enumerate(want):
        got = (int(inc["cost2"][p]), int(inc["start"][p]), inc["mem"][int(inc["mem_off"][p]):int(inc["mem_off"][p + 1])].tolist(),
               int(inc["grow_steps"][p]), int(inc["repair_steps"][p]))
        if w is None or w[0] is None:
            assert got == (-1, -1, [], 0, 0), (p, got)
            assert cluster_prep.round_incumbent(inc, p) is None
            continue
        m = w[0]
        assert got == (m["cost2"], m["start"], m["members"], m["grow_steps"], m["repair_steps"]), (p, got, m)
        assert cluster_prep.round_incumbent(inc, p) == (m["cost"], m["x"])


def compare(ctx, tints, part0, problems, settings=SETTINGS, max_seeds=64):
    want = mirror(tints, problems, settings, max_seeds)
    arr, inc = device(ctx, tints, part0, problems, settings, max_seeds)
    assert [int(r) >= 0 for r in arr["refused"]] == [w is None for w in want]
    check(inc, want, problems)
    return inc, want


def grid_tints():
    """The tints of the host test's grid (seeds 1 .. 40, with and without gaps), as read_segment() leaves them."""
    tints = []
    for seed in range(1, 41):
        n, M = 6 + seed % 7, 5 + seed % 9
        for with_gaps in (False, True):
            rng = random.Random(seed)
            rows = ru.random_rows(rng, n, M, const_runs=seed % 2 == 0, flip=0.1)
            gaps, polys = ru.random_gaps(rng, rows, p=0.7) if with_gaps else ({}, {})
            tints.append(ru.make_tint(len(tints), rows, gaps, polys, members={i: rng.randrange(1, 4) for i in range(n)}))
    return tints


@pytest.mark.parametrize("recycle_model,max_ilp,max_seeds", [("constant", 1000, 64), ("constant", 3, 64), ("exons", 1000, 1), ("introns", 3, 3),
                                                             ("introns", 1000, 1000)])
def test_grid_in_one_batch(ctx, recycle_model, max_ilp, max_seeds):
    """Every partition of the 80 grid tints in ONE call, the refused problems among them: they come back as -1 and the rest are the
    mirror's.  max_ilp 3 splits the components, which is where incompatible pairs come from; half costs under exons / introns."""
    tints = grid_tints()
    part0 = stage(ctx, tints, maximum_ilp_size=max_ilp)
    problems = all_problems(tints, lambda t, q, rids: rids[::-1] if t % 3 == 0 else rids)
    inc, want = compare(ctx, tints, part0, problems, cluster.ilp_settings(recycle_model), max_seeds)
    assert any(w is None for w in want) and sum(1 for w in want if w and w[0] and w[0]["members"]) > len(want) // 2
    assert any(w and w[0] and w[0]["repair_steps"] for w in want)
    if max_ilp == 3:
        assert sum(len(inc) for tint in tints for _, inc in tint["partitions"]) > 0


def flips_tint(tid, n, M, gaps=None, seg_lens=None):
    """n reps, one partition whatever max_ilp >= n is: all ones, rep i > 0 with a 0 at one of the places 3, 8, 13, ... < M - 3 in turn
    (two flips apart at the most: a complete graph).  Only the ends, the flips and their neighbours are informative."""
    places = list(range(3, M - 3, 5))
    rows = []
    for i in range(n):
        row = [1] * M
        if i:
            row[places[(i - 1) % len(places)]] = 0
        rows.append(row)
    return ru.make_tint(tid, rows, gaps, seg_lens=seg_lens)


def star_tint(tid, leaves, M=40):
    """Leaves two flips from the centre (the last rep) at places of their own: four flips from each other, so no two leaves are
    compatible, and the pruning keeps a leaf's one edge.  One partition; every pair of leaves is in its pair list."""
    rows = []
    for i in range(leaves):
        row = [1] * M
        row[2 + 4 * i] = row[3 + 4 * i] = 0
        rows.append(row)
    rows.append([1] * M)
    assert 3 + 4 * (leaves - 1) < M - 1
    return ru.make_tint(tid, rows)


def test_columns_around_word_boundaries(ctx):
    """R = 1, 63, 64, 65 columns (the member, blocked and conflict rows are one or two words, or three), whole and out of order."""
    rng = random.Random(1)
    tints = [big_tint(t, R, 40, 20 + t) for t, R in enumerate([1, 63, 64, 65])] + [flips_tint(4, 65, 44)]
    part0 = stage(ctx, tints)
    assert [len(t["partitions"]) for t in tints] == [1] * 5
    compare(ctx, tints, part0, all_problems(tints, lambda t, q, rids: rids))
    inc, want = compare(ctx, tints, part0, all_problems(tints, lambda t, q, rids: rng.sample(rids, len(rids))), max_seeds=1000)
    assert want[0][0]["members"] == [] and want[0][0]["repair_steps"] == 1        # (big_tint's rep 0 has a gap of length 0: it joins and leaves)
    assert all(len(w[0]["members"]) >= 60 for w in want[1:])


def test_257_columns(ctx):
    """Nine words a column set, more columns than a workgroup has threads; four seeds keep the mirror quick."""
    tints = [big_tint(0, 257, 40, 3)]
    part0 = stage(ctx, tints)
    inc, want = compare(ctx, tints, part0, all_problems(tints, lambda t, q, rids: rids), max_seeds=4)
    assert len(want) == 1 and len(want[0][0]["members"]) > 200


@pytest.mark.parametrize("M", [31, 32, 33, 64, 65])
def test_segments_around_word_boundaries(ctx, M):
    rng = random.Random(M)
    rows = ru.random_rows(rng, 40, M)
    tints = [ru.make_tint(7, rows, *ru.random_gaps(rng, rows)), big_tint(1, 30, M, M)]
    part0 = stage(ctx, tints)
    inc, want = compare(ctx, tints, part0, all_problems(tints, lambda t, q, rids: rids))
    assert any(w and w[0] and len(w[0]["members"]) > 1 for w in want)


def test_every_pair_in_conflict_and_both_ties(ctx):
    """The leaves of a star without its centre: every pair is in conflict, so a set is one member.  Every leaf has the same delta2 from
    the empty set (the smallest column wins) and every start ends at the same cost2 (the earliest start wins): column 0 from start 0,
    whatever order the columns come in.  With the centre: it and one leaf."""
    tints = [star_tint(0, 9), star_tint(1, 9)]
    part0 = stage(ctx, tints)
    assert [len(t["partitions"]) for t in tints] == [1, 1] and len(tints[0]["partitions"][0][1]) == 36
    problems = [(0, 0, [5, 3, 8, 0, 1, 2, 4, 7, 6]), (1, 0, list(range(10))[::-1])]
    for max_seeds in (1, 3, 64):
        inc, want = compare(ctx, tints, part0, problems, max_seeds=max_seeds)
        assert want[0][0]["members"] == [0] and want[0][0]["start"] == 0 and want[0][0]["cost2"] == 2 * 3 * 8
        assert len(want[1][0]["members"]) == 2 and 0 in want[1][0]["members"]          # (the centre is column 0 there)
    solo = [(0, 0, [4]), (1, 0, [9])]                                                   # R = 1, with and without a pair list behind it
    inc, want = compare(ctx, tints, part0, solo)
    assert [w[0]["members"] for w in want] == [[0], [0]]


def test_no_pairs_no_gaps_and_repairs(ctx):
    """Complete graphs of 8 reps over 12 segments (lengths 10, 13, ..., 213 in all; G of the gap (2, 9) is 64 once all are in):
    0: no pair, no gap: everything joins;  1: one rep's gap of 5 is violated (0.8 x 64 - 20 > 5): repair takes that rep out, once;
    2: every rep's gap of 150 is violated whatever E is (1.2 x 64 + 20 < 150) but holds for a rep outside (150 <= 20 + 213): repair
    strips the set to empty;  3: a gap of 500 > 20 + 213 breaks a rep outside too unless E is large, which its own row forbids: no
    start is feasible and the problem has no incumbent;  4: no column at all: the empty start, cost 0."""
    gap = (2, 9)
    tints = [flips_tint(0, 8, 12), flips_tint(1, 8, 12, {3: {gap: 5}}), flips_tint(2, 8, 12, {i: {gap: 150} for i in range(8)}),
             flips_tint(3, 8, 12, {3: {gap: 500}}), flips_tint(4, 3, 12)]
    part0 = stage(ctx, tints)
    assert [len(t["partitions"]) for t in tints] == [1] * 5 and not any(t["partitions"][0][1] for t in tints)
    problems = all_problems(tints, lambda t, q, rids: rids if t < 4 else [])
    inc, want = compare(ctx, tints, part0, problems)
    assert want[0][0]["members"] == list(range(8)) and want[0][0]["repair_steps"] == 0
    assert sorted(problems[1][2][c] for c in want[1][0]["members"]) == [0, 1, 2, 4, 5, 6, 7] and want[1][0]["repair_steps"] == 1
    assert want[2][0]["members"] == [] and want[2][0]["cost2"] == 2 * 3 * 8 and want[2][0]["repair_steps"] == 8
    assert want[3][0] is None and inc["cost2"][3] == -1
    assert (want[4][0]["cost2"], want[4][0]["start"], want[4][0]["members"]) == (0, 0, [])


def test_300_by_150(ctx):
    tints = [big_tint(0, 300, 150, 4)]
    part0 = stage(ctx, tints)
    inc, want = compare(ctx, tints, part0, all_problems(tints, lambda t, q, rids: rids), max_seeds=6)
    assert len(want) == 1 and len(want[0][0]["members"]) > 100
    assert all(v >= 0 for v in ctx.round_incumbent_timing().values())


def test_both_row_paths_and_two_rounds(ctx, monkeypatch):
    """Small problems and one of 400 reps in one call, with the rows in LDS, with the LDS path off and with a low LDS limit (some
    problems on either side of it); then the next round on the same context with fewer remaining reps.  The round's own results stay
    readable behind the incumbents."""
    tints = grid_tints()[::4] + [big_tint(99, 400, 70, 9)]
    part0 = stage(ctx, tints)
    first = all_problems(tints, lambda t, q, rids: rids)
    second = all_problems(tints, lambda t, q, rids: rids[1::2][::-1])
    want = {"first": mirror(tints, first, SETTINGS, 3), "second": mirror(tints, second, SETTINGS, 3)}
    for env in ({}, {"FCLU_ROUND_LDS": "0"}, {"FCLU_ROUND_LDS_BYTES": "600"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for name, problems in (("first", first), ("second", second)):
            arr, inc = device(ctx, tints, part0, problems, SETTINGS, 3)
            check(inc, want[name], problems)
            r = cluster_prep._Rounds()
            assert ctx._L.fclu_round_results(ctx._h, ctypes.byref(r)) == 0 and r.n_prob == len(problems)
            assert cluster_prep._copy_out(r.inf_seg, int(r.n_inf), np.int32).tolist() == arr["inf_seg"].tolist()
            assert cluster_prep._copy_out(r.rows, 3 * int(r.n_gap_rows), np.int32).tolist() == arr["rows"].reshape(-1).tolist()
        for k in env:
            monkeypatch.delenv(k)


def test_refusals(ctx):
    fresh = cluster_prep.Context(0)
    try:
        with pytest.raises(cluster_prep.ClusterError) as e:
            fresh.round_incumbents([], 0.2, 20)
        assert e.value.code == 1
        assert fresh._L.fclu_round_incumbents(fresh._h, None, 0.8, 1.2, 20, 64) == 1          # FCLU_ERR_ARG
        assert b"fclu_round_models" in fresh._L.fclu_last_error(fresh._h)
    finally:
        fresh.close()
    tints = [flips_tint(0, 8, 12), flips_tint(1, 5, 12)]
    part0 = stage(ctx, tints)
    problems = all_problems(tints, lambda t, q, rids: rids)
    compare(ctx, tints, part0, problems)
    for garbage, word in (([3.0] * 12 + [3.25], "multiple of 0.5"), ([3.0] * 12, "12 garbage costs"), ([3.0] * 12 + [-1.0], "multiple of 0.5")):
        with pytest.raises(cluster_prep.ClusterError, match=word):
            ctx.round_incumbents(garbage, 0.2, 20)
    with pytest.raises(cluster_prep.ClusterError, match="max_seeds"):
        ctx.round_incumbents([3.0] * 13, 0.2, 20, max_seeds=0)
    g2 = np.full(13, 6, np.int32)
    assert ctx._L.fclu_round_incumbents(ctx._h, g2.ctypes.data, 0.8, 1.2, -1, 64) == 1
    compare(ctx, tints, part0, problems)                                                    # the context stays usable
    host = cu.random_tint(3, 30, 20)
    cluster_prep.partition_reads_batch([host], 1000, ctx, verbose=False)                    # fclu_partition ends the rounds' source
    assert ctx._L.fclu_round_incumbents(ctx._h, g2.ctypes.data, 0.8, 1.2, 20, 64) == 1
    with pytest.raises(cluster_prep.ClusterError):
        ctx.round_incumbents([3.0] * 13, 0.2, 20)
    part0 = stage(ctx, tints)
    compare(ctx, tints, part0, problems)


def test_end_to_end_cli_with_the_cutoff(ctx, tmp_path):
    """py/freddie_cluster.py --incumbent cutoff on the fixture files of test_end_to_end_cli: it runs, every solve is OPTIMAL, and every
    round's cost equals the plain run's."""
    seg = tmp_path / "segment" / "chr1"
    seg.mkdir(parents=True)
    names = [n for n in cu.cluster_names() if cu.load_cluster(n)["read_reps"]][:4]
    ids = []
    for name in names:
        src = cu.segment_tsv_file(name, tmp_path)
        tint = list(cluster_prep.read_segment(src).values())[0]
        ids.append(tint["id"])
        os.replace(src, str(seg / ("segment_chr1_%d.tsv" % tint["id"])))
    res = subprocess.run([sys.executable, os.path.join(ROOT, "py", "freddie_cluster.py"), "-s", str(tmp_path / "segment"), "-o", str(tmp_path / "out"),
                          "-l", str(tmp_path / "logs"), "--incumbent", "cutoff"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    for tid in ids:
        assert os.path.exists(tmp_path / "out" / "chr1" / ("cluster_chr1_%d.tsv" % tid))
        log = (tmp_path / "logs" / "chr1" / str(tid) / "timeout.log").read_text().splitlines()
        assert log and all(l.split("\t")[0] == "OPTIMAL" for l in log)
    paths = [str(seg / ("segment_chr1_%d.tsv" % tid)) for tid in ids]
    costs = {}
    for mode in ("off", "cutoff"):
        record = []
        assert len(list(cluster.cluster_files(paths, cluster.ilp_settings(incumbent=mode), ctx=ctx, on_round=record.append))) == len(paths)
        costs[mode] = sorted((r["tint"]["id"], r["partition"], r["round"], r["status"], r["cost"]) for r in record)
    assert costs["off"] and costs["off"] == costs["cutoff"]
