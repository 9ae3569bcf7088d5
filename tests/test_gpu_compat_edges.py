"""The built cases of tests/compat_cases.py on the device: k_compat<RANK> and the three prunings (k_prune_lds; k_prune_edges;
k_deg1 + k_prune) through Context.compat_graph, raw and pruned, the whole matrix word for word against the model, `rounds` against
the model's passes, and the launch census (Context.last_paths) of every run against what that run must have launched -- asserted,
not assumed.  Every batch runs twice on one context and the second answer is the first: a stale second copy of the matrix, stale
flags or a buffer a larger batch left behind would show.  Group C takes crafted graphs of more than 64 adjacency words through the
components; the largest gadget tint goes through Context.partition.  tests/test_compat_cases_host.py shows on the CPU that the model
is the oracle and that every case reaches its edge."""
import numpy as np
import pytest

import compat_cases as cc
import partition_util as pu
from freddie_amd import cluster_prep

pytestmark = pytest.mark.gpu

KNOBS = ("FCLU_RANK", "FCLU_PRUNE_LDS", "FCLU_PRUNE_EDGES", "FCLU_PRUNE_LDS_WORDS", "FCLU_PART_LDS")
SWITCHES = {"default": {}, "masked": {"FCLU_RANK": "0"}, "per-pass": {"FCLU_PRUNE_LDS": "0"},
            "or-of-rows": {"FCLU_PRUNE_LDS": "0", "FCLU_PRUNE_EDGES": "0"}, "lds-300": {"FCLU_PRUNE_LDS_WORDS": "300"}}
BATCHES = cc.batches()
R_W = [b for b in BATCHES if b[0] in "RW"]
P = [b for b in BATCHES if b[0] == "P"]


@pytest.fixture(scope="module")
def ctx():
    c = cluster_prep.Context(0)
    yield c
    c.close()


def set_switches(monkeypatch, switch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in SWITCHES[switch].items():
        monkeypatch.setenv(k, v)


def expected_paths(tints, passes, switch, prune):
    """The census a run must leave, from the shapes and the switches: compat_run's own decisions restated, so on its own it would follow a
    wrong host rule -- the literal assertions in the tests below (rank up to 207 words, edge_chunks 1 / 2, OR of rows, the LDS count from
    the sizes, passes 4 / 1 / 2) are the independent half of the check."""
    env = SWITCHES[switch]
    aw = [(x.n + 63) // 64 for x in tints]
    want = dict(compat_form="rank" if max(x.words for x in tints) <= cc.RANK_WORDS and env.get("FCLU_RANK") != "0" else "masked",
                tiles=sum(a * (a + 1) // 2 for a in aw), lds_tints=0, pass_kernel=None, edge_chunks=0, passes_enqueued=0, passes_ran=0)
    if not prune:
        return want
    limit = int(env.get("FCLU_PRUNE_LDS_WORDS", cc.PRUNE_LDS_WORDS)) if env.get("FCLU_PRUNE_LDS") != "0" else -1
    in_lds = [x.n * a <= limit for x, a in zip(tints, aw)]
    want["lds_tints"] = sum(in_lds)
    large = [k for k in range(len(tints)) if not in_lds[k]]
    if large:
        edge_walk = env.get("FCLU_PRUNE_EDGES") != "0"
        want.update(pass_kernel="edge_walk" if edge_walk else "or_of_rows",
                    edge_chunks=(max(aw[k] for k in large) + 63) // 64 if edge_walk else 0,
                    passes_enqueued=4, passes_ran=2 if any(passes[k] for k in large) else 1)
    return want


def model_words(tints, which):
    """The model's matrices in the layout compat_graph returns."""
    return pu.pack_adj([cc.model_of(x.name)[which] for x in tints])[2]


def run_batch(ctx, name, switch):
    tints = [cc.tint(n) for n in BATCHES[name]]
    packed = cc.pack(tints)
    passes = [cc.model_of(x.name)[2] for x in tints]
    want_raw, want_pruned = model_words(tints, 0), model_words(tints, 1)
    assert set(passes) <= {0, 1}
    census = None
    for again in range(2):
        raw, _ = ctx.compat_graph(packed, prune=False)
        paths_raw = ctx.last_paths()
        pruned, rounds = ctx.compat_graph(packed, prune=True)
        paths = ctx.last_paths()
        for t, x in enumerate(tints):
            a0, a1 = int(packed["adj_off"][t]), int(packed["adj_off"][t + 1])
            assert np.array_equal(raw[a0:a1], want_raw[a0:a1]), "%s, run %d: compatibility graph of %s differs" % (name, again, x.name)
            assert np.array_equal(pruned[a0:a1], want_pruned[a0:a1]), "%s, run %d: pruned graph of %s differs" % (name, again, x.name)
        assert rounds.tolist() == passes, (name, again)
        assert paths_raw == expected_paths(tints, passes, switch, False), (name, again, paths_raw)
        assert paths == expected_paths(tints, passes, switch, True), (name, again, paths)
        census = paths
    return census


# ---- Groups R and W: the rule and the row widths, both forms of k_compat --------------------------------------------------------------
@pytest.mark.parametrize("switch", ["default", "masked"])
@pytest.mark.parametrize("batch", R_W)
def test_rule_and_widths(ctx, batch, switch, monkeypatch):
    set_switches(monkeypatch, switch)
    census = run_batch(ctx, batch, switch)
    widest = max(cc.tint(n).words for n in BATCHES[batch])
    # rows of at most 207 words take the rank form under the default switches; 208 words and more, and a batch that holds such a tint,
    # take the masked form whole
    assert census["compat_form"] == ("rank" if switch == "default" and widest <= 207 else "masked")
    if batch == "W-6624+6625":
        assert widest == 208 and census["compat_form"] == "masked" and census["tiles"] == 6
    if batch == "R":
        assert census["lds_tints"] == 9 and census["pass_kernel"] is None


# ---- Group P: the prunings ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", ["default", "per-pass", "or-of-rows", "lds-300"])
@pytest.mark.parametrize("batch", P)
def test_pruning_gadgets(ctx, batch, switch, monkeypatch):
    set_switches(monkeypatch, switch)
    census = run_batch(ctx, batch, switch)
    sizes = [cc.tint(n).n for n in BATCHES[batch]]
    assert census["compat_form"] == "rank"
    large = [n for n in sizes if switch in ("per-pass", "or-of-rows") or n * ((n + 63) // 64) > (300 if switch == "lds-300" else 7808)]
    assert census["lds_tints"] == len(sizes) - len(large)
    if switch == "or-of-rows":
        assert census["pass_kernel"] == "or_of_rows" and census["edge_chunks"] == 0
    elif large:
        assert census["pass_kernel"] == "edge_walk" and census["edge_chunks"] == (2 if max(large) >= 4097 else 1)
    else:
        assert census["pass_kernel"] is None and census["passes_enqueued"] == 0
    if large:                                            # a burst of four: the removing pass and the one that finds nothing, or the latter alone
        still = batch == "P-still" or (batch == "P-still+small" and len(large) == 1)      # (the small tint removes; is it an LDS tint here?)
        assert (census["passes_enqueued"], census["passes_ran"]) == (4, 1 if still else 2)


def test_large_batch_behind_and_in_front_of_small_ones(monkeypatch):
    """A context of its own: buffers grow with the large batch and stay; the batches behind it find them larger than they need."""
    set_switches(monkeypatch, "default")
    c = cluster_prep.Context(0)
    try:
        for name in ("P-small", "P-4161", "P-small", "W-9600", "R", "P-mixed", "W-33", "P-4096"):
            run_batch(c, name, "default")
    finally:
        c.close()


# ---- Group C: components of graphs beyond 64 adjacency words -----------------------------------------------------------------------------
def scipy_labels(A):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    _, lab = connected_components(csr_matrix(A), directed=False)
    first = np.full(lab.max() + 1, A.shape[0])
    np.minimum.at(first, lab, np.arange(A.shape[0]))
    return first[lab].astype(np.int32)                                                # a component -> its smallest node


def check_parts(arr, t, r0, A, labels, mem_off, mem, size, what):
    n = A.shape[0]
    parts = pu.expected_partitions_numpy(A, labels, mem_off, mem, size)
    q0, q1 = int(arr["tint_part_off"][t]), int(arr["tint_part_off"][t + 1])
    assert np.array_equal(arr["label"][r0:r0 + n], labels), what + ": labels"
    assert q1 - q0 == len(parts), what + ": number of partitions"
    for q, (nodes, rids, pairs) in zip(range(q0, q1), parts):
        assert arr["part_nodes"][arr["part_node_off"][q]:arr["part_node_off"][q + 1]].tolist() == nodes, what + ": nodes"
        assert arr["part_rids"][arr["part_rid_off"][q]:arr["part_rid_off"][q + 1]].tolist() == rids, what + ": rep ids"
        assert np.array_equal(arr["pairs"][arr["part_pair_off"][q]:arr["part_pair_off"][q + 1]], pairs), what + ": pairs"


@pytest.mark.parametrize("part_lds", [None, "0"], ids=["lds", "per-pass"])
@pytest.mark.parametrize("n", [4097, 4161])
def test_components_beyond_64_words(ctx, n, part_lds, monkeypatch):
    """65 and 66 words a row: k_cc_hook's second trip over a row.  A path, a star whose hub is the last node, a shuffled path and the
    component that straddles every word edge, beside a small tint that one workgroup takes unless the switch says otherwise."""
    set_switches(monkeypatch, "default")
    if part_lds is not None:
        monkeypatch.setenv("FCLU_PART_LDS", part_lds)
    mats = [pu.path(n), pu.star(n), pu.two_cliques(65), pu.shuffled_path(n), pu.straddle(n)]
    _, members = pu.members_for([m.shape[0] for m in mats], max_mult=2)
    row_off, adj_off, adj = pu.pack_adj(mats)
    arr = ctx.partition_adj(row_off, adj_off, adj, members, 400)
    for t, A in enumerate(mats):
        r0, r1 = int(row_off[t]), int(row_off[t + 1])
        labels = scipy_labels(A)
        if t in (0, 1, 3):
            assert not labels.any()                                                   # one component
        mem_off = members["mem_off"][r0:r1 + 1] - members["mem_off"][r0]
        mem = members["mem"][members["mem_off"][r0]:members["mem_off"][r1]]
        check_parts(arr, t, r0, A, labels, mem_off, mem, 400, "tint %d of %d nodes" % (t, A.shape[0]))
    assert (np.diff(arr["part_node_off"]) <= 400).all()
    # no graph was built (it is the caller's): the whole census is zero
    assert ctx.last_paths() == dict(compat_form=None, tiles=0, lds_tints=0, pass_kernel=None, edge_chunks=0, passes_enqueued=0, passes_ran=0)


@pytest.mark.parametrize("part_lds", [None, "0"], ids=["lds", "per-pass"])
def test_partition_of_the_largest_gadget_tint(ctx, part_lds, monkeypatch):
    """Context.partition on the tint of 4 161 rows: the graph, its pruning and the components without leaving the device, against the
    model's pruned graph."""
    set_switches(monkeypatch, "default")
    if part_lds is not None:
        monkeypatch.setenv("FCLU_PART_LDS", part_lds)
    xs = [cc.tint("P-4161"), cc.tint("P-130")]
    packed = cc.pack(xs)
    R = int(packed["row_off"][-1])
    members = dict(mem_off=np.arange(R + 1, dtype=np.int64), mem=(np.arange(R, dtype=np.int32) * 3 + 1))
    arr = ctx.partition(packed, members, 400)
    paths = ctx.last_paths()
    assert (paths["compat_form"], paths["pass_kernel"], paths["edge_chunks"], paths["lds_tints"]) == ("rank", "edge_walk", 2, 1)
    for t, x in enumerate(xs):
        r0 = int(packed["row_off"][t])
        A = cc.model_of(x.name)[1]
        check_parts(arr, t, r0, A, scipy_labels(A), np.arange(x.n + 1, dtype=np.int64), members["mem"][r0:r0 + x.n], 400, x.name)
