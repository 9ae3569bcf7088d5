"""The round models on the GPU (fclu_round_models): every array of every problem against the plain restatement of tests/round_util.py,
exactly (integer work), on crafted problems where the kernels can go wrong: word boundaries, uninformative runs across them, constant
columns of both values side by side, empty and one-rep remaining sets, subsets out of order, filtered pair lists, gap groups with
shared keys and both tails' pseudo-gaps, the refusal, both paths (LDS and device memory) in one batch, and two rounds on one context.
The last test runs py/freddie_cluster.py from segment_*.tsv fixtures."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import cluster_util as cu
import round_util as ru
from freddie_amd import cluster_prep

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONSTANT = dict(recycle_model="constant")
SEGMENTS = [1, 2, 3, 31, 32, 33, 64, 65, 600]


@pytest.fixture(scope="module")
def ctx():
    c = cluster_prep.Context(0)
    yield c
    c.close()


def stage(ctx, tints, maximum_ilp_size=1000):
    """Partition the tints on the device (which leaves rows and pair lists there), leave them as preprocess_ilp() + partition_reads()
    do, and hand the gaps and segment lengths to the context.  Returns the partitions' first id per tint."""
    packed, prep, arr = cluster_prep.cluster_arrays_batch(tints, maximum_ilp_size, ctx)
    cluster_prep._ilp_data_from_prep(tints, packed, prep, CONSTANT)
    for t, tint in enumerate(tints):
        tint["partitions"] = cluster_prep._partitions_from_arrays(arr, t, False)
    ctx.round_setup(*cluster_prep.round_gaps(tints))
    return arr["tint_part_off"].tolist()


def run(ctx, tints, part0, problems):
    """problems: [(tint index, partition index in the tint, remaining rep ids)].  Returns (arrays, [restatement per problem])."""
    arr = ctx.round_models([part0[t] + q for t, q, _ in problems], [rem for _, _, rem in problems])
    want = [ru.restate(tints[t], tints[t]["partitions"][q][1], rem) for t, q, rem in problems]
    return arr, want


def check(arr, want):
    assert arr["n_prob"] == len(want)
    for p, w in enumerate(want):
        w = dict(w)
        refused = w.pop("refused")
        if refused is not None:
            assert arr["refused"][p] == refused, (p, int(arr["refused"][p]), refused)
            assert cluster_prep.round_model(arr, p) is None
            continue
        assert arr["refused"][p] == -1, (p, int(arr["refused"][p]))
        got = cluster_prep.round_model(arr, p)
        for key in w:
            assert got[key] == w[key], (p, key, got[key], w[key])


def all_problems(tints, pick):
    return [(t, q, pick(t, q, list(rids))) for t, tint in enumerate(tints) for q, (rids, _) in enumerate(tint["partitions"])]


@pytest.mark.parametrize("M", SEGMENTS)
def test_segment_counts(ctx, M):
    """Rows of 1, 2, 3 segments, around one and two words, and wider than 512: whole partitions, then halves out of order."""
    rng = random.Random(M)
    rows = ru.random_rows(rng, 40, M)
    gaps, polys = ru.random_gaps(rng, rows)
    tints = [ru.make_tint(7, rows, gaps, polys)]
    part0 = stage(ctx, tints)
    arr, want = run(ctx, tints, part0, all_problems(tints, lambda t, q, rids: rids))
    check(arr, want)
    arr, want = run(ctx, tints, part0, all_problems(tints, lambda t, q, rids: rng.sample(rids, (len(rids) + 1) // 2)))
    check(arr, want)


def test_one_rep_and_empty(ctx):
    rng = random.Random(5)
    tints = [ru.make_tint(t, ru.random_rows(rng, 12, M)) for t, M in enumerate([1, 2, 3, 33, 70])]
    part0 = stage(ctx, tints)
    check(*run(ctx, tints, part0, all_problems(tints, lambda t, q, rids: rids[-1:])))
    check(*run(ctx, tints, part0, all_problems(tints, lambda t, q, rids: [])))


def runs_tint(tid, M, a, b, value, n=6):
    """Reps that agree (value) on the segments a .. b and differ everywhere else: a .. b is a constant stretch, a + 1 .. b - 1 uninformative."""
    rows = []
    for i in range(n):
        rows.append([value if a <= j <= b else (1 if (i + j) % 2 == 0 else 0) for j in range(M)])
    return ru.make_tint(tid, rows)


def test_uninformative_runs_at_word_boundaries(ctx):
    """Uninformative runs that end at bit 30, at bit 31 exactly, cross bits 31 / 32 and 63 / 64, of zeros and of ones; and all-0 columns
    next to all-1 columns, each constant but informative.  The reps agree on a .. b in every subset, so whatever partitions the tints
    fall into, none of a + 1 .. b - 1 is informative in any of them."""
    shapes = [(70, 20, 31, 1), (70, 20, 31, 0), (70, 20, 32, 1), (70, 20, 32, 0), (70, 28, 36, 1), (70, 30, 33, 0), (70, 31, 32, 1),
              (130, 60, 68, 0), (64, 50, 63, 1), (65, 0, 64, 1)]
    tints = [runs_tint(t, M, a, b, v) for t, (M, a, b, v) in enumerate(shapes)]
    mixed = [[(0 if 10 <= j < 20 else 1 if 20 <= j < 40 else (i + j) % 2) for j in range(48)] for i in range(5)]
    tints.append(ru.make_tint(len(shapes), mixed))
    part0 = stage(ctx, tints)
    problems = all_problems(tints, lambda t, q, rids: rids)
    arr, want = run(ctx, tints, part0, problems)
    check(arr, want)
    for (t, _, rem), w in zip(problems, want):
        assert rem
        if t < len(shapes):
            _, a, b, _ = shapes[t]
            assert not set(range(a + 1, b)) & set(w["inf_seg"]), (t, w["inf_seg"])
        else:                                             # columns 10 .. 19 hold 0, 20 .. 39 hold 1: the seam stays informative
            assert 19 in w["inf_seg"] and 20 in w["inf_seg"] and not set(range(11, 19)) & set(w["inf_seg"])
    whole = [w for (t, _, rem), w in zip(problems, want) if t == 2 and len(rem) > 1 and len(set(map(tuple, (tints[2]["ilp_data"]["I"][i] for i in rem)))) > 1]
    for w in whole:                                       # both row patterns present: the run 21 .. 31 is all that is dropped
        assert [j for j in range(70) if j not in w["inf_seg"]] == list(range(21, 32))


def pairs_tint(tid, seed, n=60, M=24):
    rng = random.Random(seed)
    return ru.make_tint(tid, ru.random_rows(rng, n, M, n_patterns=5, const_runs=False, flip=0.08))


def test_pairs_filtered(ctx):
    """Partitions with incompatible pairs (components split into chunks of 7 nodes): all remaining keeps every pair in order, one
    remaining rep or none filters every pair, a shuffled half keeps some."""
    rng = random.Random(11)
    tints = [pairs_tint(t, 40 + t) for t in range(4)]
    part0 = stage(ctx, tints, maximum_ilp_size=7)
    assert sum(len(inc) for tint in tints for _, inc in tint["partitions"]) > 0
    arr, want = run(ctx, tints, part0, all_problems(tints, lambda t, q, rids: rids))
    check(arr, want)
    assert arr["n_pairs"] == sum(len(inc) for tint in tints for _, inc in tint["partitions"])
    arr, want = run(ctx, tints, part0, all_problems(tints, lambda t, q, rids: rids[:1]))
    check(arr, want)
    assert arr["n_pairs"] == 0
    check(*run(ctx, tints, part0, all_problems(tints, lambda t, q, rids: rng.sample(rids, (len(rids) + 1) // 2))))


def test_gap_groups(ctx):
    """Reps with no gap, one and several; two reps sharing a key; the pseudo-gaps of both tails; a gap next to its neighbour (nothing
    strictly between)."""
    M = 40
    rows = [[(1 if (i * 7 + j * 3) % 5 < 3 else 0) for j in range(M)] for i in range(10)]
    for r in rows:
        r[0] = r[M - 1] = 1
    gaps = {1: {(3, 9): 50}, 2: {(3, 9): 70, (12, 13): 5, (20, 38): 100}, 4: {(0, 39): 400, (3, 9): 1}, 7: {(20, 38): 30}}
    polys = {3: {"SA": (20, 44)}, 5: {"ET": (15, 9)}, 6: {"ST": (30, 2)}, 7: {"EA": (12, 77)}, 8: {"SA": (5, 1)}}
    tints = [ru.make_tint(3, rows, gaps, polys)]
    part0 = stage(ctx, tints)
    arr, want = run(ctx, tints, part0, all_problems(tints, lambda t, q, rids: rids))
    check(arr, want)
    assert arr["n_gap_rows"] == 11                        # seven internal gaps and four pseudo-gaps (rep 8's tail is too short)
    assert any(j1 == -1 for w in want for j1, _ in w["groups"]) and any(j2 == M for w in want for _, j2 in w["groups"])
    check(*run(ctx, tints, part0, all_problems(tints, lambda t, q, rids: rids[::-1])))


def test_refusal_names_problem_and_column(ctx):
    """A gap whose endpoint lies inside a constant stretch: the reference asserts (:467-468).  The problem is refused with its smallest
    offending column; the other problems of the batch come out right, and so does the next call."""
    bad = runs_tint(0, 40, 10, 20, 1)
    for i in (2, 4):
        bad["reads"][bad["read_reps"][i][0]]["gaps"][(12, 30)] = 33
    good = runs_tint(1, 40, 10, 20, 1)
    good["reads"][3]["gaps"][(5, 30)] = 12
    tints = [good, bad, runs_tint(2, 33, 3, 9, 0)]
    part0 = stage(ctx, tints)
    problems = all_problems(tints, lambda t, q, rids: rids[::-1])
    arr, want = run(ctx, tints, part0, problems)
    refused = [(p, w["refused"]) for p, w in enumerate(want) if w["refused"] is not None]
    assert refused, "the crafted problem must be one the reference raises on"
    check(arr, want)
    assert [(p, int(c)) for p, c in enumerate(arr["refused"]) if c >= 0] == refused
    check(*run(ctx, tints, part0, all_problems(tints, lambda t, q, rids: rids)))


def test_argument_refusals(ctx):
    tints = [pairs_tint(0, 3, n=20)]
    part0 = stage(ctx, tints, maximum_ilp_size=7)
    rids = tints[0]["partitions"][0][0]
    other = [i for i in range(20) if i not in rids]
    for parts, rem, word in (([part0[0], part0[0]], [rids, rids], "twice"), ([part0[0]], [[rids[0], rids[0]]], "problem 0 column 1"),
                             ([part0[0]], [[99]], "problem 0 column 0"), ([part0[0] + 1000], [[]], "partition")):
        with pytest.raises(cluster_prep.ClusterError, match=word):
            ctx.round_models(parts, rem)
    if other:
        with pytest.raises(cluster_prep.ClusterError, match="not in partition"):
            ctx.round_models([part0[0]], [[other[0]]])
    check(*run(ctx, tints, part0, all_problems(tints, lambda t, q, r: r)))          # the context stays usable


def big_tint(tid, n, M, seed):
    """n reps in one partition: a handful of patterns one flip apart (a complete graph), with 0 -> 2 swaps so that C varies."""
    rng = random.Random(seed)
    base = [1 if rng.random() < 0.7 else 0 for _ in range(M)]
    base[M // 3:M // 3 + 6] = [1] * 6
    pats = [list(base)]
    for k in range(4):
        p = list(base); p[2 + 5 * k] ^= 1; pats.append(p)
    rows = [[2 if v == 0 and rng.random() < 0.4 else v for v in pats[rng.randrange(5)]] for _ in range(n)]
    gaps = {i: {(0, M - 1): i} for i in range(0, n, 97)}
    return ru.make_tint(tid, rows, gaps)


def small_tints(rng, n):
    """n tints of three to eight reps with gaps and tails, their segment counts around the word boundaries."""
    tints = []
    for t in range(n):
        M = rng.choice([5, 31, 32, 33, 64, 65, 90])
        rows = ru.random_rows(rng, rng.randrange(3, 9), M)
        tints.append(ru.make_tint(t, rows, *ru.random_gaps(rng, rows)))
    return tints


def test_batch_of_both_paths_and_two_rounds(ctx, monkeypatch):
    """300 small problems and one of 1 500 reps in one call (rows in LDS, rows in device memory); then round r + 1 on the same context
    with other remaining sets; then everything again with the LDS path off and with a low LDS limit."""
    tints = small_tints(random.Random(2), 300)
    tints.append(big_tint(300, 1500, 70, 9))
    part0 = stage(ctx, tints)
    assert max(len(rids) for rids, _ in tints[300]["partitions"]) == 1500
    first = all_problems(tints, lambda t, q, rids: rids)
    assert len(first) >= 301
    second = all_problems(tints, lambda t, q, rids: rids[1::2][::-1])
    want = {}
    for env in ({}, {"FCLU_ROUND_LDS": "0"}, {"FCLU_ROUND_LDS_BYTES": "600"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for name, problems in (("first", first), ("second", second)):
            arr = ctx.round_models([part0[t] + q for t, q, _ in problems], [rem for _, _, rem in problems])
            if name not in want:
                want[name] = [ru.restate(tints[t], tints[t]["partitions"][q][1], rem) for t, q, rem in problems]
            check(arr, want[name])
        for k in env:
            monkeypatch.delenv(k)
    assert all(v >= 0 for v in ctx.round_timing().values())


def test_setup_needs_a_partition_call(ctx):
    tint = cu.random_tint(3, 30, 20)
    cluster_prep.partition_reads_batch([tint], 1000, ctx, verbose=False)      # (host rows: nothing of preprocess on the device)
    with pytest.raises(cluster_prep.ClusterError, match="fclu_round_setup"):
        ctx.round_setup(np.zeros(31, np.int64), np.zeros((0, 3), np.int32), np.array([0, 20]), np.full(20, 10, np.int32))


GRAMMAR_HEAD = re.compile(r"#[^\t]+\t[0-9]+\t[0-9]+(,[0-9]+)*\n$")
GRAMMAR_ISO = re.compile(r"isoform_[0-9]+\t[0-9]+\t[01]+\n$")
GRAMMAR_READ = re.compile(r"[0-9]+\t[^\t]+\t[^\t]+\t[+-]\t[0-9]+\t[0-9]+\t[NSE]\t([0-9]+|\*)\t[012X-]+(\t[012X-](\([0-9]+\))?)+(\t[SE][AT]:\([0-9]+, [0-9]+\))*\n$")


def test_end_to_end_cli(ctx, tmp_path):
    """segment_*.tsv fixtures through py/freddie_cluster.py: the output follows the reference's grammar line by line, freddie_amd.isoforms
    reads it, and every round's cost on problems small enough equals the brute force's."""
    from freddie_amd import cluster, isoforms
    seg = tmp_path / "segment" / "chr1"
    seg.mkdir(parents=True)
    names = [n for n in cu.cluster_names() if cu.load_cluster(n)["read_reps"]][:4]
    ids = []
    for name in names:
        src = cu.segment_tsv_file(name, tmp_path)
        tint = list(cluster_prep.read_segment(src).values())[0]
        ids.append(tint["id"])
        os.replace(src, str(seg / ("segment_chr1_%d.tsv" % tint["id"])))
    assert len(set(ids)) == len(ids)
    out = tmp_path / "out"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "py", "freddie_cluster.py"), "-s", str(tmp_path / "segment"), "-o", str(out),
                          "-l", str(tmp_path / "logs")], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    for tid in ids:
        path = out / "chr1" / ("cluster_chr1_%d.tsv" % tid)
        lines = open(path).readlines()
        assert GRAMMAR_HEAD.match(lines[0])
        for line in lines[1:]:
            assert GRAMMAR_ISO.match(line) or GRAMMAR_READ.match(line), line
        segments, _, _ = isoforms.read_cluster(str(path))
        assert [key[1] for key in segments] == [tid]
        assert os.path.exists(tmp_path / "logs" / "chr1" / str(tid) / "timeout.log")
    # the rounds' costs against the brute force, in process, on the same files
    record = []
    paths = [str(seg / ("segment_chr1_%d.tsv" % tid)) for tid in ids]
    settings = cluster.ilp_settings()
    assert len(list(cluster.cluster_files(paths, settings, ctx=ctx, on_round=record.append))) == len(paths)
    small = [r for r in record if len(r["remaining"]) <= 12]
    assert small
    for r in small:
        best = ru.brute_force(r["tint"], r["incomp"], r["remaining"], settings)
        assert best is not None and r["status"] == "OPTIMAL" and abs(r["cost"] - best[0]) < 0.25, (r["cost"], best)
