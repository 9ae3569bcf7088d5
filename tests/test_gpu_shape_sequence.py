"""One context, a fixed sequence of small batches, each of which changes one of the facts that shape what a run launches (small
batch, k_tiny's share, solved whole or through the arenas, huge / giant problems, 32-bit DP counts, the label arena's form): a
captured graph is valid only for the shape it was captured under, and the library keeps that by comparing shapes, not by remembering
to drop the graph wherever a fact changes.  Every batch is run three times and compared with the oracle each time: the sized first
run, the run that captures (the capture count, the last word of the `sync` tap, rises by exactly one), and the replay of that
capture (the count does not move).  Under FSEG_NO_FORK=1 every replay is a graph; with the default a run that forks replays as
plain launches, so only the small batches capture.  Each step asserts from the launch census that its fact did flip.

What the batches hold was checked with the oracle (problems of >= 3 candidates, the widest problem's reads, the largest problem):
A 24 / 85 / 28, B 152 / 15 / 28, C 287 / 15 / 28, D 290 / 599 / 28, H 22 / 300 / 71, G 7 / 119 / 141, W 2 / 90 000 / 17 --
against FSEG_TINY_FROM=100 (B, C, D have k_tiny's list), the 256 problems of a small batch (C, D are not small) and
FSEG_FUSE_LANES=200 (D, H, W go through the arenas)."""
import functools

import pytest

import util
from freddie_amd import _lib

pytestmark = pytest.mark.gpu

ENV = {"FSEG_TINY_FROM": "100", "FSEG_FUSE_LANES": "200"}
HUGE, GIANT = dict(max_problem_size=100), dict(max_problem_size=150, variance_factor=9.99)
DECISIONS = ("small_batch", "tiny_on", "fuse_on", "label_packed", "score", "arena_dp")


@functools.lru_cache(maxsize=None)
def partitions():
    mp = util.make_partition
    many = [mp(s, n_reads=300, n_exons=960, rp=0.15) for s in (21, 22)]                      # ~150 problems each, most of them tiny
    return dict(A=[mp(1, n_reads=300, n_exons=120, rp=0.05)], B=many[:1], C=many,
                D=many + [mp(4242, n_reads=600, n_exons=14, rp=0.02, max_span=0)],             # ... and a problem that sees 599 reads
                H=[mp(3, n_reads=300, n_exons=150, rp=0.3, max_span=0)],                       # a problem of 71 candidates under max_problem_size 100
                G=[mp(77, n_reads=120, n_exons=400, rp=0.3, max_span=0)],                      # ... of 141 under 150
                W=[util.weighted_partition(77, 300, 14, 300, rp=0.5, jp=0.8, jsd=6.0)])        # 300 reps that stand for 90 000 reads


@functools.lru_cache(maxsize=None)
def oracles(batch, params):
    return [util.run_oracle(p, dict(params)) for p in partitions()[batch]]


def huge(paths):
    return bool(paths["score"] & 16)


def giant(paths):
    return bool(paths["score"] & 32)


def wide_counts(paths):
    return paths["arena_dp"] == 4


def word(name):
    return lambda paths: paths[name]


# (batch, parameters, the fact the step is there for, its value now -- the step before had the other --, what the run must have seen)
STEPS = [
    ("A", {}, None, None, lambda sz: sz["n_problems"] <= 100 and sz["max_problem_reads"] <= 200),
    ("B", {}, word("tiny_on"), 1, lambda sz: 100 < sz["n_problems"] <= 256),
    ("C", {}, word("small_batch"), 0, lambda sz: sz["n_problems"] > 256),
    ("D", {}, word("fuse_on"), 0, lambda sz: sz["max_problem_reads"] > 200 and sz["n_problems"] > 256),
    ("C", {}, word("fuse_on"), 1, lambda sz: sz["max_problem_reads"] <= 200),
    ("B", {}, word("small_batch"), 1, lambda sz: 100 < sz["n_problems"] <= 256),
    ("A", {}, word("tiny_on"), 0, lambda sz: sz["n_problems"] <= 100),
    ("A", dict(threshold_rate=1.0), word("label_packed"), 0, None),
    ("A", dict(threshold_rate=0.9), word("label_packed"), 1, None),
    ("H", HUGE, huge, True, lambda sz: 60 < sz["max_problem_size"] <= 128),
    ("A", HUGE, huge, False, lambda sz: sz["max_problem_size"] <= 60),
    ("G", GIANT, giant, True, lambda sz: 128 < sz["max_problem_size"] <= 150),
    ("W", {}, wide_counts, True, lambda sz: sz["max_problem_reads"] >= 65536 and sz["max_problem_size"] <= 60),
    ("A", {}, wide_counts, False, None),
]


@pytest.mark.parametrize("env", [{"FSEG_NO_FORK": "1"}, {}], ids=["graphs", "default"])
def test_one_context_through_every_shape(env, monkeypatch):
    for k, v in {**ENV, **env}.items():
        monkeypatch.setenv(k, v)
    graphs_always = "FSEG_NO_FORK" in env
    ctx = _lib.Context(0)
    try:
        first = before = None
        for step, (name, params, fact, want, seen) in enumerate(STEPS):
            parts, want_res, where = partitions()[name], oracles(name, tuple(sorted(params.items()))), "step %d (%s)" % (step, name)
            util.run_gpu(ctx, parts, params)                            # the sized first run
            util.compare_partitions(ctx, parts, want_res)
            paths, captures = ctx.paths(), int(ctx.tap("sync")[9])
            assert seen is None or seen(ctx.sizes()), (where, ctx.sizes())
            if fact is not None:                                        # the step's fact is what it is for, and was not before
                assert fact(paths) == want and fact(before) != want, (where, paths, before)
            for run in (1, 2):
                ctx.run(); ctx.sync()
                util.compare_partitions(ctx, parts, want_res)
                now = int(ctx.tap("sync")[9])
                if run == 1:                                            # a new batch: nothing captured before fits it
                    assert now - captures == 1 if graphs_always else now - captures in (0, 1), (where, now, captures)
                else:                                                   # ... and what was captured then fits now
                    assert now == captures, (where, now, captures)
                captures = now
                assert [ctx.paths()[k] for k in DECISIONS] == [paths[k] for k in DECISIONS], (where, run)
            first, before = first or paths, paths
        same = DECISIONS + ("wave_on", "key32", "known", "n_solve0", "n_solve1", "n_solve2", "n_tiny", "tiny_kernel", "solve8")
        assert [paths[k] for k in same] == [first[k] for k in same]     # the first batch again: the same launches
        assert not graphs_always or captures == len(STEPS)
    finally:
        ctx.close()
