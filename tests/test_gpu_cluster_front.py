"""The front of the clustering pre-ILP work on the GPU (fclu_preprocess, fclu_partition_reads): per rep I / C / FL and the
dedupe against the fixtures of the reference's own preprocess_ilp() / partition_reads() and against the plain restatement of
tests/front_util.py on crafted label rows; forced hash collisions; the one-call path against the present one (host front +
Context.partition); the refusals.  Integer work: everything is compared exactly."""
import copy

import numpy as np
import pytest

import cluster_util as cu
import front_util as fu
from freddie_amd import cluster_prep
from oracle import cluster_oracle

pytestmark = pytest.mark.gpu

CONSTANT = dict(recycle_model="constant")
FUZZ_M = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 301]
FUZZ_REPS = [1, 2, 63, 64, 65, 257, 1000]


@pytest.fixture(scope="module")
def ctx():
    c = cluster_prep.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fixtures(tmp_path_factory):
    """name -> (tint as read_segment() leaves it, the same after host preprocess_ilp(), the fixture)."""
    d = tmp_path_factory.mktemp("front")
    out = {}
    for name in cu.cluster_names():
        tint = list(cluster_prep.read_segment(cu.segment_tsv_file(name, d)).values())[0]
        host = copy.deepcopy(tint)
        cluster_prep.preprocess_ilp(host, CONSTANT)
        out[name] = (tint, host, cu.load_cluster(name))
    return out


def fixture_outputs(host, golden):
    """What the device must give for a fixture tint: I, C, FL and categories of the reference's own run; nodes of unique_data_of."""
    I = [[int(ch) for ch in row] for row in golden["I"]]
    tail = [fu.TAILS.index(golden["reads"][m[0]]["poly_tail_category"]) for m in golden["read_reps"]]
    uniq = cluster_oracle.unique_data_of(host)
    rep_node = [None] * len(I)
    for q, (_, members) in enumerate(uniq):
        for i in members:
            rep_node[i] = q
    return dict(I=I, C=[[int(ch) for ch in row] for row in golden["C"]], FL=[tuple(x) for x in golden["FL"]],
                raw=[cluster_prep.find_segment_read(I, i) for i in range(len(I))], tail=tail,
                nodes=[(u[1][0], u[1]) for u in uniq], rep_node=rep_node)


def partitions_of(arr, t):
    return [[rids, [list(p) for p in pairs]] for rids, pairs in cluster_prep._partitions_from_arrays(arr, t, False)]


def assert_same_arrays(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def check_fixture_batch(ctx, fixtures, names):
    tints = [fixtures[n][0] for n in names]
    packed = cluster_prep.pack_labels(tints)
    prep = ctx.preprocess(packed)
    for t, n in enumerate(names):
        want = fixture_outputs(fixtures[n][1], fixtures[n][2])
        assert packed["tail"][int(packed["rep_off"][t]):int(packed["rep_off"][t + 1])].tolist() == want["tail"]
        fu.check_prep_against(prep, packed, t, want)
    for size in (7, 1000):
        prep2, parts = ctx.partition_labels(packed, size)
        assert_same_arrays(prep, prep2)
        for t, n in enumerate(names):
            assert partitions_of(parts, t) == fixtures[n][2]["partitions"][str(size)], (n, size)
    return prep


def test_reference_fixtures_as_one_batch(ctx, fixtures):
    names = cu.cluster_names()
    assert len(names) == 12
    prep = check_fixture_batch(ctx, fixtures, names)
    rows = {n: int(prep["row_off"][t + 1] - prep["row_off"][t]) for t, n in enumerate(names)}
    reps = {n: len(fixtures[n][0]["read_reps"]) for n in names}
    assert (reps["g3_ont"], rows["g3_ont"]) == (989, 978) and (reps["e_plateau_touch"], rows["e_plateau_touch"]) == (4, 3)
    assert (reps["g_tiny"], rows["g_tiny"]) == (6, 5)


@pytest.mark.parametrize("name", cu.cluster_names())
def test_reference_fixture_singly(ctx, fixtures, name):
    check_fixture_batch(ctx, fixtures, [name])


def test_preprocess_ilp_batch_leaves_tints_as_the_host_does(ctx, fixtures):
    names = cu.cluster_names()
    tints = [copy.deepcopy(fixtures[n][0]) for n in names]
    cluster_prep.preprocess_ilp_batch(tints, CONSTANT, ctx)
    n_pseudo = 0
    for tint, n in zip(tints, names):
        host = fixtures[n][1]
        assert tint == host, n                                           # ilp_data, categories, gaps with their pseudo-gap keys
        M = len(tint["segs"])
        for members in tint["read_reps"]:
            rep = tint["reads"][members[0]]
            assert all(tint["reads"][r]["gaps"] is rep["gaps"] for r in members)      # one dict object a rep (:311-313)
            n_pseudo += sum(1 for a, b in rep["gaps"] if a == -1 or b == M)
    assert n_pseudo > 0
    with pytest.raises(AttributeError):                                  # the reference's exons model calls .values() on a list
        cluster_prep.preprocess_ilp_batch([copy.deepcopy(fixtures["g_tiny"][0])], dict(recycle_model="exons"), ctx)
    with pytest.raises(AttributeError):
        cluster_prep.preprocess_ilp_batch([copy.deepcopy(fixtures["g_tiny"][0])], dict(recycle_model="introns"), ctx)
    # partition_reads_batch on tints without ilp_data: the one-call path, tints left as preprocess_ilp + partition_reads leave them
    fresh = [copy.deepcopy(fixtures[n][0]) for n in names[:4]]
    done = copy.deepcopy(fixtures[names[4]][1])
    cluster_prep.partition_reads_batch(fresh + [done], 7, ctx, verbose=False)
    for tint, n in zip(fresh + [done], names[:5]):
        assert cu.canon_partitions(tint) == fixtures[n][2]["partitions"]["7"]
        assert tint["ilp_data"] == fixtures[n][1]["ilp_data"]


# ---- crafted fuzz against the restatement --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fuzz():
    """(tints, pack_labels, restatement per tint): every M of FUZZ_M with every rep count of FUZZ_REPS, a zero-rep tint in the middle."""
    tints = []
    for a, M in enumerate(FUZZ_M):
        for b, n in enumerate(FUZZ_REPS):
            tints.append(fu.crafted_tint(1000 * a + b, n, M, pool=3 + (a + b) % 5))
    empty = fu.label_tint(7, [], [], None); empty["segs"] = [(0, 1, 1)] * 40
    tints.insert(len(tints) // 2, empty)
    want = [fu.tint_outputs(t) for t in tints]
    # the generator does what the issue asks of it
    assert any(len(w["nodes"]) < len(w["I"]) / 4 for w in want)                                  # large groups
    assert any(any(nd[1] != list(range(nd[1][0], nd[1][0] + len(nd[1]))) for nd in w["nodes"]) for w in want)   # interleaved
    both = set()
    for w in want:
        by_I = {}
        for i, row in enumerate(w["I"]):
            by_I.setdefault(tuple(row), set()).add((w["FL"][i], w["tail"][i]))
        for s in by_I.values():
            both.update("tail" for x in s for y in s if x[0] == y[0] and x[1] != y[1])
            both.update("FL" for x in s for y in s if x[0] != y[0])
    assert both == {"tail", "FL"}                                        # equal I, distinct nodes: by tail only and by FL through it
    return tints, cluster_prep.pack_labels(tints), want


@pytest.fixture(scope="module")
def fuzz_default(ctx, fuzz):
    return ctx.preprocess(fuzz[1]), ctx.partition_labels(fuzz[1], 50)


def test_crafted_fuzz_against_the_restatement(fuzz, fuzz_default):
    tints, packed, want = fuzz
    prep = fuzz_default[0]
    assert prep["n_tint"] == len(tints) and prep["n_reps"] == sum(len(t["read_reps"]) for t in tints)
    for t in range(len(tints)):
        fu.check_prep_against(prep, packed, t, want[t])
    assert_same_arrays(prep, fuzz_default[1][0])


@pytest.mark.parametrize("bits", ["0", "3"])
def test_forced_hash_collisions_change_nothing(ctx, fuzz, fuzz_default, bits, monkeypatch):
    monkeypatch.setenv("FCLU_HASH_BITS", bits)
    assert_same_arrays(ctx.preprocess(fuzz[1]), fuzz_default[0])
    prep, parts = ctx.partition_labels(fuzz[1], 50)
    assert_same_arrays(prep, fuzz_default[1][0])
    assert_same_arrays(parts, fuzz_default[1][1])


# ---- the one-call path against host front + Context.partition ---------------------------------------------------------
@pytest.fixture(scope="module")
def random_label_tints():
    shapes = [(1, 5), (2, 1), (63, 31), (64, 32), (65, 33), (130, 64), (200, 65), (257, 100), (40, 300), (1400, 60)]
    tints = [fu.labels_from_preprocessed(cu.random_tint(100 + k, n, m), seed=k, twos=0.2, dup=0.2) for k, (n, m) in enumerate(shapes)]
    host = copy.deepcopy(tints)
    for t in host:
        cluster_prep.preprocess_ilp(t, CONSTANT)
    uniq = [cluster_prep.unique_structures(t) for t in host]
    assert len(host[-1]["read_reps"]) >= 1100 and len(uniq[-1]) * ((len(uniq[-1]) + 63) // 64) > 7808     # beyond one workgroup's LDS
    assert any(len(u) < 0.9 * len(t["read_reps"]) for u, t in zip(uniq, host))                          # and the dedupe has work
    return tints, uniq


@pytest.mark.parametrize("part_lds", [None, "0"], ids=["components-in-lds", "components-per-pass"])
def test_one_call_equals_host_front_and_partition(ctx, random_label_tints, part_lds, monkeypatch):
    if part_lds is None:
        monkeypatch.delenv("FCLU_PART_LDS", raising=False)
    else:
        monkeypatch.setenv("FCLU_PART_LDS", part_lds)
    tints, uniq = random_label_tints
    structures, members = cluster_prep.pack_structures(uniq), cluster_prep.pack_members(uniq)
    packed = cluster_prep.pack_labels(tints)
    for size in (50, 1000):
        want = ctx.partition(structures, members, size)
        prep, got = ctx.partition_labels(packed, size)
        assert_same_arrays(got, want)
        ps = cluster_prep.prep_structures(prep, packed["n_seg"])
        assert ps["n_tint"] == structures["n_tint"]
        for k in structures:
            if k != "n_tint":
                assert np.array_equal(ps[k], structures[k]), k
        assert_same_arrays(cluster_prep.prep_members(prep), members)
    tm = ctx.preprocess_timing()
    assert tm["rows_ms"] > 0 and tm["dedupe_ms"] > 0


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(ctx):
    tints = [fu.crafted_tint(1, 5, 20), fu.crafted_tint(2, 9, 33), fu.crafted_tint(3, 4, 16)]
    good = cluster_prep.pack_labels(tints)
    want = ctx.preprocess(good)
    LW = 3                                                                # words a row of tint 1 (33 labels)
    lab1 = int(good["lab_off"][1])

    def refused(change, code, match):
        bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        change(bad)
        for call in (lambda: ctx.preprocess(bad), lambda: ctx.partition_labels(bad, 10)):
            with pytest.raises(cluster_prep.ClusterError, match=match) as e:
                call()
            assert e.value.code == code
        assert_same_arrays(ctx.preprocess(good), want)                    # the context goes on working

    def code3(b):
        b["labels"][lab1 + 6 * LW + 1] |= np.uint32(3 << 4)               # tint 1, rep 6, label 18
    refused(code3, 1, r"tint 1 rep 6.*code 3")

    def beyond(b):
        b["labels"][lab1 + 4 * LW + 2] |= np.uint32(1 << 2)               # label 33 of a row of 33 labels (0 .. 32)
    refused(beyond, 1, r"tint 1 rep 4.*beyond")

    def tail3(b):
        b["tail"][int(good["rep_off"][2]) + 3] = 3
    refused(tail3, 1, r"tint 2 rep 3.*tail")

    def lab_off(b):
        b["lab_off"][2:] += 1
        b["labels"] = np.concatenate([b["labels"], np.zeros(1, np.uint32)])
    refused(lab_off, 1, r"tint 1.*lab_off")

    def negative(b):
        b["rep_off"][2] = 3                                               # tint 1 would own -2 reps
    refused(negative, 1, r"tint 1.*negative")

    def negative_segments(b):
        b["n_seg"][0] = -1
    refused(negative_segments, 1, r"tint 0.*negative")

    def empty(b):
        b["n_tint"] = 0
    refused(empty, 1, "empty batch")

    def too_long(b):
        b["n_seg"][2] = 9601
    refused(too_long, cluster_prep.ERR_UNSUPPORTED, r"tint 2 has 9601 segments")

    with pytest.raises(cluster_prep.ClusterError, match="maximum_ilp_size"):
        ctx.partition_labels(good, 0)
    # 9600 segments are taken
    long_tint = fu.crafted_tint(9, 3, 9600)
    packed = cluster_prep.pack_labels([long_tint])
    fu.check_prep_against(ctx.preprocess(packed), packed, 0, fu.tint_outputs(long_tint))
    prep, parts = ctx.partition_labels(good, 10)
    assert_same_arrays(prep, want)
    assert int(parts["tint_part_off"][-1]) >= 3


# ---- buffer lifetime: one context through growing, refused, smaller and empty calls ------------------------------------
def lifetime_batch(shapes, seed):
    """(label tints packed, the same tints after host preprocess_ilp(), their unique rows packed, the rows' members)."""
    tints = [fu.labels_from_preprocessed(cu.random_tint(seed + k, n, m), seed=k) if n else dict(fu.label_tint(seed + k, [], [], None), segs=[(0, 1, 1)] * m)
             for k, (n, m) in enumerate(shapes)]
    host = copy.deepcopy(tints)
    for t in host:
        cluster_prep.preprocess_ilp(t, CONSTANT)
    uniq = [cluster_prep.unique_structures(t) for t in host]
    return cluster_prep.pack_labels(tints), host, cluster_prep.pack_structures(uniq), cluster_prep.pack_members(uniq)


def lifetime_calls(c, batch, size=50):
    """Every array a batch gives: the one-call path, then the graph and the partition behind the host's front."""
    packed, host, structures, _ = batch
    prep, parts = c.partition_labels(packed, size)
    adj, rounds = c.compat_graph(structures)
    return dict(prep=prep, parts=parts, graph=dict(adj=adj, rounds=rounds), batch=cluster_prep.partition_arrays_batch(host, size, c))


@pytest.mark.parametrize("per_pass", [False, True], ids=["in-lds", "per-pass"])
def test_one_context_through_many_calls_equals_fresh_contexts(per_pass, monkeypatch):
    """Buffers that grew for one call serve the next: three tints across the 64-row tile edge, a refused call, a smaller batch, a batch
    without a rep and the first batch again on ONE context give, call by call, what a fresh context gives.  per-pass: a lower LDS limit
    sends the 130-rep tint through the per-pass pruning kernels (and all components through theirs), so the burst loop runs too."""
    for name, value in (("FCLU_PRUNE_LDS_WORDS", "300"), ("FCLU_PART_LDS", "0")):
        if per_pass:
            monkeypatch.setenv(name, value)
        else:
            monkeypatch.delenv(name, raising=False)
    first = lifetime_batch([(130, 64), (65, 33), (1, 5)], 300)
    small = lifetime_batch([(63, 31)], 310)
    no_reps = lifetime_batch([(0, 40), (0, 7)], 320)
    assert first[2]["row_off"][1] > 64 and int(no_reps[0]["rep_off"][-1]) == 0

    def fresh(batch):
        c = cluster_prep.Context(0)
        try:
            return lifetime_calls(c, batch)
        finally:
            c.close()

    def same(got, want):
        assert sorted(got) == sorted(want)
        for k in got:
            assert_same_arrays({n: np.asarray(v) for n, v in got[k].items()}, {n: np.asarray(v) for n, v in want[k].items()})

    want = {id(b): fresh(b) for b in (first, small, no_reps)}
    c = cluster_prep.Context(0)
    try:
        same(lifetime_calls(c, first), want[id(first)])
        bad = dict(first[2]); bad["last"] = first[2]["last"].copy(); bad["last"][0] = 64        # beyond the last segment (0 .. 63)
        with pytest.raises(cluster_prep.ClusterError, match="out of range"):
            c.compat_graph(bad)
        with pytest.raises(cluster_prep.ClusterError, match="out of range"):
            c.partition(bad, first[3], 50)
        with pytest.raises(cluster_prep.ClusterError, match="fclu_partition_results: no result"):
            c._partition_arrays("fclu_partition_results", 0)
        for b in (small, no_reps, first):
            same(lifetime_calls(c, b), want[id(b)])
    finally:
        c.close()
    for _ in range(20):
        cluster_prep.Context(0).close()
