"""partition_reads() behind the dedupe as one device computation (Context.partition / partition_adj: connected components,
the even split, members and incompatible pairs, py/freddie_cluster.py:256-274) against tint['partitions'] as the
reference's own function wrote it (fixtures), against the CPU oracle's components plus a literal restatement of :258-274
on crafted graphs, and against the host tail it replaces.  Integer work: everything is compared exactly."""
import copy
import functools

import numpy as np
import pytest

import cluster_util as cu
import partition_util as pu
from freddie_amd import cluster_prep

pytestmark = pytest.mark.gpu

PATHS = pytest.mark.parametrize("part_lds", [None, "0"], ids=["lds", "per-pass"])


@pytest.fixture(scope="module")
def ctx():
    c = cluster_prep.Context(0)
    yield c
    c.close()


def set_path(monkeypatch, part_lds):
    if part_lds is None:
        monkeypatch.delenv("FCLU_PART_LDS", raising=False)
    else:
        monkeypatch.setenv("FCLU_PART_LDS", part_lds)


# ---- 1: the reference's own outputs --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference_cases():
    """{maximum_ilp_size: [(tint, partitions in JSON shape)]} from every fixture that stores that size."""
    by_size = {}
    for case in cu.random_partition_cases():
        tint = cu.random_tint(case["seed"], case["n_reps"], case["n_segs"], **case["kw"])
        for size, parts in case["partitions"].items():
            by_size.setdefault(int(size), []).append((tint, parts))
    return by_size


@PATHS
def test_reference_outputs_random_tints(ctx, part_lds, monkeypatch):
    set_path(monkeypatch, part_lds)
    by_size = reference_cases()
    assert len(cu.random_partition_cases()) >= 10 and sum(len(v) for v in by_size.values()) >= len(cu.random_partition_cases())
    for size, cases in sorted(by_size.items()):
        arr = cluster_prep.partition_arrays_batch([t for t, _ in cases], size, ctx)            # all tints of a size in one batch
        for k, (tint, parts) in enumerate(cases):
            assert pu.arrays_to_json(arr, k) == parts, "batched, seed %d, maximum_ilp_size %d" % (tint["id"], size)
            single = cluster_prep.partition_arrays_batch([tint], size, ctx)
            assert pu.arrays_to_json(single, 0) == parts, "single, seed %d, maximum_ilp_size %d" % (tint["id"], size)


@PATHS
def test_reference_outputs_segment_goldens(ctx, part_lds, monkeypatch, tmp_path):
    set_path(monkeypatch, part_lds)
    tints, refs = [], []
    for name in cu.cluster_names():
        tint = list(cluster_prep.read_segment(cu.segment_tsv_file(name, tmp_path)).values())[0]
        cluster_prep.preprocess_ilp(tint, dict(recycle_model="constant"))
        tints.append(tint)
        refs.append(cu.load_cluster(name)["partitions"])
    for size in (7, 1000):
        arr = cluster_prep.partition_arrays_batch(tints, size, ctx)
        for k, tint in enumerate(tints):
            assert pu.arrays_to_json(arr, k) == refs[k][str(size)], "batched, tint %d, maximum_ilp_size %d" % (k, size)
            single = cluster_prep.partition_arrays_batch([tint], size, ctx)
            assert pu.arrays_to_json(single, 0) == refs[k][str(size)], "single, tint %d, maximum_ilp_size %d" % (k, size)


# ---- 2: crafted graphs through partition_adj ---------------------------------------------------------------------------
SIZES = (1, 2, 63, 64, 65, 129, 200)


@functools.lru_cache(maxsize=None)
def crafted_batch():
    """Every graph kind at every node count, with an empty tint in the middle of the batch."""
    mats = [fn(n) for fn in pu.GRAPHS.values() for n in SIZES]
    mats.insert(len(mats) // 2, np.zeros((0, 0), bool))
    per_tint, members = pu.members_for([A.shape[0] for A in mats])
    return mats, per_tint, members, pu.pack_adj(mats)


@functools.lru_cache(maxsize=None)
def crafted_expected(size):
    mats, per_tint, _, _ = crafted_batch()
    return [pu.expected_partitions(A, per_tint[t], size) for t, A in enumerate(mats)]


def check_arrays(arr, t, row0, A, mult, labels, parts, what):
    """Tint t of a result against (labels, [(nodes, rids, pairs)]) and the numpy pair counts."""
    n = A.shape[0]
    q0, q1 = int(arr["tint_part_off"][t]), int(arr["tint_part_off"][t + 1])
    assert np.array_equal(arr["label"][row0:row0 + n], labels), what + ": labels"
    assert q1 - q0 == len(parts), what + ": number of partitions"
    for q, (nodes, rids, pairs) in zip(range(q0, q1), parts):
        assert arr["part_nodes"][arr["part_node_off"][q]:arr["part_node_off"][q + 1]].tolist() == nodes, what + ": nodes"
        assert arr["part_rids"][arr["part_rid_off"][q]:arr["part_rid_off"][q + 1]].tolist() == rids, what + ": rep ids"
        n_pairs = int(arr["part_pair_off"][q + 1] - arr["part_pair_off"][q])
        assert n_pairs == pu.pair_count(A, nodes, mult), what + ": pair count"
        assert np.array_equal(arr["pairs"][arr["part_pair_off"][q]:arr["part_pair_off"][q + 1]], np.asarray(pairs, np.int32).reshape(-1, 2)), what + ": pairs"


def check_crafted(ctx, size):
    """crafted_batch() through partition_adj under maximum_ilp_size = size, against crafted_expected(size)."""
    mats, per_tint, members, (row_off, adj_off, adj) = crafted_batch()
    arr = ctx.partition_adj(row_off, adj_off, adj, members, size)
    assert arr["tint_part_off"][0] == 0 and arr["tint_part_off"][-1] == len(arr["part_node_off"]) - 1
    assert arr["part_node_off"][-1] == row_off[-1] and arr["part_rid_off"][-1] == members["mem_off"][-1]
    assert arr["part_pair_off"][-1] == len(arr["pairs"])
    kinds = [(k, n) for k in pu.GRAPHS for n in SIZES]
    kinds.insert(len(kinds) // 2, ("empty", 0))
    mult = np.diff(members["mem_off"])
    for t, A in enumerate(mats):
        labels, parts = crafted_expected(size)[t]
        r0 = int(row_off[t])
        check_arrays(arr, t, r0, A, mult[r0:r0 + A.shape[0]], labels, parts, "%s of %d nodes, maximum_ilp_size %d" % (kinds[t] + (size,)))
    e = len(mats) // 2
    assert mats[e].shape[0] == 0 and arr["tint_part_off"][e] == arr["tint_part_off"][e + 1]     # the empty tint: no partition


@PATHS
@pytest.mark.parametrize("size", [1, 2, 7, 64, 65, 1000])
def test_crafted_graphs(ctx, size, part_lds, monkeypatch):
    set_path(monkeypatch, part_lds)
    check_crafted(ctx, size)


# ---- 3: a tint beyond one workgroup's LDS ---------------------------------------------------------------------------------
def test_per_pass_path_at_its_own_size(ctx, monkeypatch):
    """1 100 nodes are 18 words a row, 19 800 words: beyond kPruneLdsWords, so the per-pass kernels take this tint whatever the
    switch says, next to a small tint that one workgroup takes whole and a path of 1 000 nodes, which neighbour-minimum
    propagation alone would need 1 000 passes for."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    monkeypatch.delenv("FCLU_PART_LDS", raising=False)
    rng = np.random.default_rng(11)
    n = 1100
    A = np.zeros((n, n), bool)
    e = rng.integers(0, n, (900, 2))
    e = e[e[:, 0] != e[:, 1]]
    A[e[:, 0], e[:, 1]] = True
    A |= A.T
    mats = [A, pu.two_cliques(65), pu.path(1000)]
    per_tint, members = pu.members_for([m.shape[0] for m in mats], max_mult=3)
    row_off, adj_off, adj = pu.pack_adj(mats)
    size = 400
    arr = ctx.partition_adj(row_off, adj_off, adj, members, size)
    mult = np.diff(members["mem_off"])
    for t, M in enumerate(mats):
        r0, r1 = int(row_off[t]), int(row_off[t + 1])
        _, lab = connected_components(csr_matrix(M), directed=False)
        first = np.full(lab.max() + 1, M.shape[0])
        np.minimum.at(first, lab, np.arange(M.shape[0]))
        labels = first[lab].astype(np.int32)                                          # scipy's component -> its smallest node
        if t == 2:
            assert not labels.any()                                                   # the path is one component
        mem_off = members["mem_off"][r0:r1 + 1] - members["mem_off"][r0]
        mem = members["mem"][members["mem_off"][r0]:members["mem_off"][r1]]
        parts = pu.expected_partitions_numpy(M, labels, mem_off, mem, size)
        check_arrays(arr, t, r0, M, mult[r0:r1], labels, parts, "tint %d" % t)
    assert (np.diff(arr["part_node_off"]) <= size).all()
    tm = ctx.partition_timing()
    assert tm["components_ms"] > 0 and tm["pairs_ms"] > 0


# ---- 4: the whole function against the host tail it replaces --------------------------------------------------------------
def test_device_path_equals_host_tail(ctx, monkeypatch, capsys):
    shapes = [(1, 5), (2, 1), (63, 31), (64, 32), (65, 33), (130, 64), (200, 65), (257, 100), (40, 300)]
    tints = [cu.random_tint(100 + k, n, m) for k, (n, m) in enumerate(shapes)]
    tints.append(cu.random_tint(200, 150, 20, n_isoforms=2, noise=0.0, tail_p=0.0))      # many reps with the same structure
    tints.append(cu.random_tint(201, 120, 24, n_isoforms=12, noise=0.1, tail_p=0.6))
    host = copy.deepcopy(tints)
    monkeypatch.setenv("FCLU_HOST_PARTITIONS", "1")
    cluster_prep.partition_reads_batch(host, 50, ctx, verbose=True)
    host_lines = capsys.readouterr().out
    monkeypatch.delenv("FCLU_HOST_PARTITIONS")
    cluster_prep.partition_reads_batch(tints, 50, ctx, verbose=True)
    assert capsys.readouterr().out == host_lines                                      # the reference's progress line (:262)
    for a, b in zip(tints, host):
        assert a["partitions"] == b["partitions"]
        assert all(type(p) is tuple for _, incomp in a["partitions"] for p in incomp[:3])
    one = copy.deepcopy(tints[9]); del one["partitions"]
    cluster_prep.partition_reads(one, 50, ctx=ctx, verbose=False)
    assert one["partitions"] == host[9]["partitions"]


# ---- 5: refusals ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(ctx):
    mats = [pu.ring(70), pu.path(5)]
    _, members = pu.members_for([70, 5])
    row_off, adj_off, adj = pu.pack_adj(mats)
    good = ctx.partition_adj(row_off, adj_off, adj, members, 7)

    bad = adj.copy(); bad[3 * 2] ^= np.uint64(1 << 20)                   # tint 0, row 3: bit (3, 20) without (20, 3)
    with pytest.raises(cluster_prep.ClusterError, match="not symmetric"):
        ctx.partition_adj(row_off, adj_off, bad, members, 7)
    bad = adj.copy(); bad[4 * 2] |= np.uint64(1 << 4)                    # (4, 4)
    with pytest.raises(cluster_prep.ClusterError, match="diagonal"):
        ctx.partition_adj(row_off, adj_off, bad, members, 7)
    bad = adj.copy(); bad[int(adj_off[1]) + 2] |= np.uint64(1 << 5)      # tint 1 has 5 nodes: column 5 does not exist
    with pytest.raises(cluster_prep.ClusterError, match="beyond N"):
        ctx.partition_adj(row_off, adj_off, bad, members, 7)
    with pytest.raises(cluster_prep.ClusterError, match="maximum_ilp_size"):
        ctx.partition_adj(row_off, adj_off, adj, members, 0)
    off = members["mem_off"].copy(); off[10] = off[9] - 1
    with pytest.raises(cluster_prep.ClusterError, match="not monotone"):
        ctx.partition_adj(row_off, adj_off, adj, dict(mem_off=off, mem=members["mem"]), 7)
    tint = cu.random_tint(5, 30, 12)
    uniq = [cluster_prep.unique_structures(tint)]
    with pytest.raises(cluster_prep.ClusterError, match="maximum_ilp_size"):
        ctx.partition(cluster_prep.pack_structures(uniq), cluster_prep.pack_members(uniq), 0)

    again = ctx.partition_adj(row_off, adj_off, adj, members, 7)
    assert sorted(good) == sorted(again) and all(np.array_equal(good[k], again[k]) for k in good)
