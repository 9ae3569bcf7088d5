"""The cluster library's capped grids (freddie_amd/csrc/freddie_cluster.hip, capped_grid()): every launch whose grid a constant caps
walks what lies beyond it in a grid-stride loop, and the batches of the other cluster tests are far too small to run such a loop twice.

  under FCLU_GRID_CAP = 1 and 3   the batches the other tests craft (their helpers, imported), through every stage, against the same
                                  plain references: one workgroup does everything; three divide nothing and leave some idle at the end
  at the production caps          two batches tiled in numpy (grid_util.tile_packed) from two dozen distinct tints of 40 to 130 rows, the
                                  order of the copies another in every block: 1.2 M rows in 14 400 tints under FCLU_PRUNE_LDS=0 and
                                  FCLU_PART_LDS=0 for the graph and the partition, 1.15 M reps for the rows and the dedupe.  The reference is
                                  computed once per distinct tint and every copy's slice compared with it.

Every case asserts, by host arithmetic on the batch's sizes and the caps read from the source (grid_util.trips), that the loops it
names run at least twice; test_batches_run_their_loops_twice does the same for all of them without a device.  Left to the knob alone,
because a batch beyond them does not fit a test of a few seconds: the 16.7 M lane slots of k_rows / k_gkeys / k_readout_corr, the 2 M
label words of k_ggather and the 1 M columns, gap rows and groups of the k_gap_* kernels.  Integer work: everything is compared exactly."""
import copy
import functools
import random

import numpy as np
import pytest

import cluster_util as cu
import front_util as fu
import grid_util as gu
import partition_util as pu
import round_util as ru
import test_gpu_cluster as t_graph
import test_gpu_cluster_front as t_front
import test_gpu_partition as t_part
import test_gpu_round_models as t_round
import test_gpu_round_readout as t_readout
import test_gpu_segment_groups as t_groups
from freddie_amd import cluster_prep
from oracle import cluster_oracle
from test_gpu_incumbents import grid_tints

gpu = pytest.mark.gpu
fuzz = t_front.fuzz                  # the other modules' fixtures, by their names
batches = t_groups.batches

CONSTANT = dict(recycle_model="constant")
KNOB = pytest.mark.parametrize("cap", [1, 3], ids=["one-workgroup", "three-workgroups"])
FRONT_SIZE = 50
PART_SIZES = (1, 7, 64, 1000)
GROUP_LOOPS = dict(shapes=("k_gkeys", "k_heads", "k_gleader", "k_greps", "k_mem_off", "k_ggather"),
                   many=("k_gkeys", "k_heads", "k_gleader", "k_greps", "k_mem_off"), big=("k_gkeys", "k_heads", "k_gleader", "k_greps", "k_mem_off"))


@pytest.fixture(scope="module")
def ctx():
    c = cluster_prep.Context(0)
    yield c
    c.close()


def set_env(monkeypatch, **env):
    """FCLU_<name> = value for every name given; None: unset."""
    for name, value in env.items():
        if value is None:
            monkeypatch.delenv("FCLU_" + name, raising=False)
        else:
            monkeypatch.setenv("FCLU_" + name, str(value))


def assert_twice(loops, names=None):
    for name in names or loops:
        assert loops[name] >= 2, "%s runs its loop %d time(s): %r" % (name, loops[name], loops)


# ---- what each case's loops run, from the batch's sizes ---------------------------------------------------------------------------
def front_loops(fuzz, cap):
    """The rows and the dedupe of the fuzz batch, and behind them the graph's tiles and the partition of its unique rows (pruning and
    components run in LDS there: one workgroup a tint, no stride)."""
    _, packed, want = fuzz
    rows = [len(w["nodes"]) for w in want]
    loops = gu.front_trips(np.diff(packed["rep_off"]), packed["n_seg"], cap)
    loops["k_compat"] = gu.graph_trips(rows, cap)["k_compat"]
    part = gu.partition_trips(sum(rows), len(rows), cap)
    loops.update({k: part[k] for k in ("k_cc_init", "k_bounds", "k_chunk", "k_offsets", "k_pairs", "k_members")})
    return loops


def group_loops(b, cap):
    lw = [max((int(m) + 15) // 16, 1) for m in b.arrays.a["n_seg"]]
    return gu.group_trips(b.arrays.a, sum(len(tint["read_reps"]) * w for (tint, _), w in zip(b.want, lw)), cap)


def graph_loops(rows, cap, edge_walk):
    loops = gu.graph_trips(rows, cap)
    return {k: loops[k] for k in (("k_compat", "k_degree", "k_prune_edges") if edge_walk else ("k_compat", "k_degree", "k_deg1", "k_prune"))}


def crafted_loops(cap, per_pass):
    row_off = t_part.crafted_batch()[3][0]
    loops = gu.partition_trips(int(row_off[-1]), len(row_off) - 1, cap)
    return loops if per_pass else {k: v for k, v in loops.items() if k not in ("k_cc_hook", "k_cc_jump")}


def round_loops(problems, want, cap):
    return gu.round_trips(len(problems), sum(len(rem) for _, _, rem in problems), sum(len(w["gap_rows"]) for w in want),
                          sum(len(w["groups"]) for w in want), cap)


def readout_loops(tints, problems, sets, cap):
    with_set = [(len(s), max((len(tints[t]["segs"]) + 31) // 32, 1)) for (t, _, _), s in zip(problems, sets) if s]
    return dict(k_readout_corr=gu.trips("k_readout_corr", gu.slots([n for n, _ in with_set], [w for _, w in with_set]), cap))


def round_batch():
    return t_round.small_tints(random.Random(2), 300)


def whole(tints):
    return t_round.all_problems(tints, lambda t, q, rids: rids)


# ---- the small batches under the knob -----------------------------------------------------------------------------------------------
def oracle_partitions(tints, size):
    """The tints' partitions by the host's preprocess_ilp() and the oracle's partition_reads(), in the fixtures' JSON shape."""
    out = []
    for tint in copy.deepcopy(tints):
        cluster_prep.preprocess_ilp(tint, CONSTANT)
        cluster_oracle.partition_reads(tint, size)
        out.append(cu.canon_partitions(tint))
    return out


@pytest.fixture(scope="module")
def fuzz_parts(fuzz):
    return oracle_partitions(fuzz[0], FRONT_SIZE)


@pytest.fixture(scope="module")
def fuzz_plain(ctx, fuzz):
    """The fuzz batch with the knob unset: (preprocess(), partition_labels())."""
    return ctx.preprocess(fuzz[1]), ctx.partition_labels(fuzz[1], FRONT_SIZE)


@gpu
@KNOB
@pytest.mark.parametrize("hash_bits", [None, "0"], ids=["default-hash", "one-bucket"])
def test_front_and_dedupe(ctx, fuzz, fuzz_parts, fuzz_plain, cap, hash_bits, monkeypatch):
    """k_rows, k_heads, k_leader (with FCLU_HASH_BITS=0 its walk through a bucket of a whole tint), k_nodes, k_mem_off; k_compat's tiles
    and the partition's kernels behind them.  Checked against the restatement and the oracle, and equal to the run with the knob unset."""
    tints, packed, want = fuzz
    plain = fuzz_plain
    assert_twice(front_loops(fuzz, cap))
    set_env(monkeypatch, PRUNE_LDS=None, PART_LDS=None, GRID_CAP=cap, HASH_BITS=hash_bits)
    prep = ctx.preprocess(packed)
    for t in range(len(tints)):
        fu.check_prep_against(prep, packed, t, want[t])
    prep2, parts = ctx.partition_labels(packed, FRONT_SIZE)
    for t in range(len(tints)):
        fu.check_prep_against(prep2, packed, t, want[t])
        assert t_front.partitions_of(parts, t) == fuzz_parts[t], t
    t_front.assert_same_arrays(prep, plain[0])
    t_front.assert_same_arrays(prep2, plain[1][0])
    t_front.assert_same_arrays(parts, plain[1][1])


@gpu
@KNOB
@pytest.mark.parametrize("name", sorted(GROUP_LOOPS))
def test_read_grouping(ctx, batches, name, cap, monkeypatch):
    """k_gkeys, k_heads, k_gleader, k_greps, k_mem_off, and k_ggather where the reps' rows are long enough (shapes)."""
    b = batches[name]
    assert_twice(group_loops(b, cap), GROUP_LOOPS[name])
    set_env(monkeypatch, HASH_BITS=None, PRUNE_LDS=None, PART_LDS=None, GRID_CAP=cap)
    t_groups.check_groups(ctx.group_reads(b.arrays), b)
    t_groups.check_partitioned(ctx.partition_segment(b.arrays, t_groups.SIZE), b)


@gpu
@KNOB
@pytest.mark.parametrize("rank", ["1", "0"], ids=["rank-tables", "masked-sums"])
@pytest.mark.parametrize("edges", [None, "0"], ids=["edge-walk", "or-of-rows"])
def test_graph_per_pass(ctx, cap, rank, edges, monkeypatch):
    """k_compat's tile loop in both forms, k_degree, and the pass in both forms: k_prune_edges, or k_deg1 and k_prune."""
    set_env(monkeypatch, PRUNE_LDS="0", PRUNE_LDS_WORDS=None, PRUNE_EDGES=edges, RANK=rank, GRID_CAP=cap)
    uniq = t_graph.check_graphs(ctx, t_graph.batched_tints())
    paths = ctx.last_paths()
    assert paths["pass_kernel"] == ("edge_walk" if edges is None else "or_of_rows") and paths["compat_form"] == ("rank" if rank == "1" else "masked")
    assert paths["lds_tints"] == 0 and paths["passes_ran"] >= 2
    loops = graph_loops([len(u) for u in uniq], cap, edges is None)
    assert loops["k_compat"] == gu.trips("k_compat", paths["tiles"], cap)              # the census' own count of tiles
    assert_twice(loops)


@gpu
@KNOB
@pytest.mark.parametrize("part_lds", [None, "0"], ids=["lds", "per-pass"])
@pytest.mark.parametrize("size", PART_SIZES)
def test_partition_of_crafted_graphs(ctx, size, part_lds, cap, monkeypatch):
    """k_cc_init, k_bounds, k_chunk, k_pairs in both forms, k_members, k_offsets; with FCLU_PART_LDS=0 k_cc_hook and k_cc_jump."""
    assert_twice(crafted_loops(cap, part_lds == "0"))
    set_env(monkeypatch, PART_LDS=part_lds, GRID_CAP=cap)
    t_part.check_crafted(ctx, size)


@gpu
@KNOB
def test_round_models_with_gap_groups(ctx, cap, monkeypatch):
    """k_gap_keys, k_gap_heads, k_gap_groups and k_gap_fill on 300 tints' problems (k_round takes a workgroup a problem: no stride)."""
    set_env(monkeypatch, HASH_BITS=None, PRUNE_LDS=None, PART_LDS=None, ROUND_LDS=None, ROUND_LDS_BYTES=None, GRID_CAP=cap)
    tints = round_batch()
    part0 = t_round.stage(ctx, tints)
    problems = whole(tints)
    arr, want = t_round.run(ctx, tints, part0, problems)
    t_round.check(arr, want)
    assert arr["n_gap_rows"] == sum(len(w["gap_rows"]) for w in want) and arr["n_grp"] == sum(len(w["groups"]) for w in want)
    assert any(w["refused"] is None and len(w["groups"]) > 1 for w in want)
    assert_twice(round_loops(problems, want, cap))


@gpu
@KNOB
def test_readout_of_the_grid_batch(ctx, cap, monkeypatch):
    """k_readout_corr on every problem of the grid batch with all its columns accepted, against the host's read-out."""
    set_env(monkeypatch, HASH_BITS=None, PRUNE_LDS=None, PART_LDS=None, ROUND_LDS=None, ROUND_LDS_BYTES=None, GRID_CAP=cap)
    tints = grid_tints()
    part0 = t_round.stage(ctx, tints)
    problems = whole(tints)
    _, out, sets = t_readout.readout(ctx, tints, part0, problems, [list(range(len(rem))) for _, _, rem in problems])
    assert out["n_sets"] > len(problems) // 2
    assert_twice(readout_loops(tints, problems, sets, cap))


# ---- the production caps, knob unset ---------------------------------------------------------------------------------------------
BLOCKS_GRAPH = 600                   # 24 distinct tints a block
BLOCKS_FRONT = 560
PROD_SIZE = 7                        # maximum_ilp_size: chunks of seven nodes keep the pair list at a few million
GRAPH_KINDS = (dict(), dict(n_isoforms=12, noise=0.1, tail_p=0.6), dict(n_isoforms=3, noise=0.01, tail_p=0.1))
FRONT_M = (1, 2, 3, 7, 15, 16, 17, 24, 31, 32, 32, 32)


def pack_rows(rows, M):
    """0 / 1 lists of M entries as uint32 words, 32 a word, the first in the low bit."""
    W = max((M + 31) // 32, 1)
    bits = np.zeros((len(rows), W * 32), np.uint8)
    if rows and M:
        bits[:, :M] = np.asarray(rows, np.uint8).reshape(len(rows), M)
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint32).reshape(len(rows), W)


@functools.lru_cache(maxsize=None)
def graph_distinct():
    """24 distinct tints: (their unique rows, pack_structures(), pack_members())."""
    tints = [cu.random_tint(500 + k, 46 + (k * 37) % 89, 20 + 3 * k, **GRAPH_KINDS[k % 3]) for k in range(24)]
    uniq = [cluster_prep.unique_structures(t) for t in tints]
    return uniq, cluster_prep.pack_structures(uniq), cluster_prep.pack_members(uniq)


@functools.lru_cache(maxsize=None)
def graph_reference():
    """Per distinct tint, by the oracle: (raw adjacency words, pruned adjacency words, passes, labels, partitions of PROD_SIZE)."""
    out = []
    for u in graph_distinct()[0]:
        n = len(u)
        edges = cluster_oracle.compat_edges(u)
        nb, passes = cluster_oracle.prune(n, edges)
        A = t_graph.oracle_matrix(n, nb)
        labels, parts = pu.expected_partitions(A, [members for _, members in u], PROD_SIZE)
        out.append((pu.pack_adj([t_graph.oracle_matrix(n, edges)])[2], pu.pack_adj([A])[2], passes, labels, parts))
    return out


@functools.lru_cache(maxsize=None)
def graph_tiled():
    _, packed, members = graph_distinct()
    return gu.tile_packed(packed, BLOCKS_GRAPH, members)


@functools.lru_cache(maxsize=None)
def front_distinct():
    tints = [fu.crafted_tint(700 + k, 46 + (k * 37) % 85, FRONT_M[k % 12], pool=3 + k % 5) for k in range(24)]
    return tints, cluster_prep.pack_labels(tints), [fu.tint_outputs(t) for t in tints]


@functools.lru_cache(maxsize=None)
def front_tiled():
    return gu.tile_packed(front_distinct()[1], BLOCKS_FRONT)


def graph_production_loops():
    big, src, _ = graph_tiled()
    rows = np.diff(big["row_off"]).tolist()
    loops = gu.graph_trips(rows)
    loops.update(gu.partition_trips(sum(rows), len(rows)))
    return loops


def front_production_loops():
    big, _ = front_tiled()
    loops = gu.front_trips(np.diff(big["rep_off"]), big["n_seg"])
    del loops["k_rows"]              # (a lane a rep at rows of one word: 1.15 M of its 16.7 M slots)
    return loops


def every_row_is(got, want, what):
    assert np.array_equal(got, np.broadcast_to(np.asarray(want, got.dtype), got.shape)), what


def same_in_every_copy(arr, idx, want, what):
    every_row_is(arr[idx], want, what)


@gpu
@pytest.mark.parametrize("edges", [None, "0"], ids=["edge-walk", "or-of-rows"])
def test_graph_and_partition_beyond_the_caps(ctx, edges, monkeypatch):
    """1.2 M rows, 14 400 tints: k_compat's 8192 tiles; k_degree's 16 384 rows; the 262 144 (row, chunk) items of k_prune_edges, or the
    16 384 word columns of k_deg1 and the 65 536 rows of k_prune; the 262 144 rows of wave_grid (k_cc_hook, k_pairs, k_members) and the
    1 048 576 of row_grid (k_cc_init, k_cc_jump, k_bounds, k_chunk, k_offsets)."""
    set_env(monkeypatch, PRUNE_LDS="0", PRUNE_LDS_WORDS=None, PART_LDS="0", PRUNE_EDGES=edges, RANK=None, GRID_CAP=None)
    loops = graph_production_loops()
    assert_twice(loops, [k for k in loops if k not in (("k_deg1", "k_prune") if edges is None else ("k_prune_edges",))])
    uniq = graph_distinct()[0]
    ref = graph_reference()
    big, src, members = graph_tiled()
    assert min(len(u) for u in uniq) >= 40 and max(len(u) for u in uniq) <= 130 and len({r[2] for r in ref}) > 1
    raw, _ = ctx.compat_graph(big, prune=False)
    assert ctx.last_paths()["tiles"] > gu.CAPS["kCapCompat"]
    pruned, rounds = ctx.compat_graph(big, prune=True)
    paths = ctx.last_paths()
    assert paths["pass_kernel"] == ("edge_walk" if edges is None else "or_of_rows") and paths["lds_tints"] == 0
    check_graph_copies(raw, pruned, rounds, ctx.partition(big, members, PROD_SIZE))


def check_graph_copies(raw, pruned, rounds, arr):
    """The tiled batch's graphs, pass counts and partition arrays: every copy's slice against its distinct tint's reference."""
    ref = graph_reference()
    big, src, members = graph_tiled()
    n_parts = np.array([len(r[4]) for r in ref])
    n_pairs = np.array([sum(len(p[2]) for p in r[4]) for r in ref])
    assert arr["tint_part_off"][-1] == n_parts[src].sum() == len(arr["part_node_off"]) - 1
    assert arr["part_node_off"][-1] == big["row_off"][-1] and arr["part_rid_off"][-1] == members["mem_off"][-1] == len(arr["part_rids"])
    assert arr["part_pair_off"][-1] == n_pairs[src].sum() == len(arr["pairs"])
    for d, (raw_words, words, passes, labels, parts) in enumerate(ref):
        what = "copies of tint %d" % d
        at, idx = gu.copies(big["adj_off"], src, d)
        same_in_every_copy(raw, idx, raw_words, what + ": compatibility graph")
        same_in_every_copy(pruned, idx, words, what + ": pruned graph")
        assert (rounds[at] == passes).all(), what + ": passes"
        _, rows = gu.copies(big["row_off"], src, d)
        row0 = big["row_off"][at][:, None]
        same_in_every_copy(arr["label"], rows, labels, what + ": labels")
        q0 = arr["tint_part_off"][at]
        assert (arr["tint_part_off"][at + 1] - q0 == len(parts)).all(), what + ": number of partitions"
        q = q0[:, None] + np.arange(len(parts) + 1)[None, :]
        every_row_is(arr["part_node_off"][q] - row0, np.cumsum([0] + [len(p[0]) for p in parts]), what + ": node offsets")
        same_in_every_copy(arr["part_nodes"], rows, [v for p in parts for v in p[0]], what + ": nodes")
        rid0 = members["mem_off"][big["row_off"][at]][:, None]
        every_row_is(arr["part_rid_off"][q] - rid0, np.cumsum([0] + [len(p[1]) for p in parts]), what + ": rep id offsets")
        rids = [r for p in parts for r in p[1]]
        same_in_every_copy(arr["part_rids"], rid0 + np.arange(len(rids))[None, :], rids, what + ": rep ids")
        pair0 = arr["part_pair_off"][q0][:, None]
        every_row_is(arr["part_pair_off"][q] - pair0, np.cumsum([0] + [len(p[2]) for p in parts]), what + ": pair offsets")
        pairs = np.asarray([pr for p in parts for pr in p[2]], np.int32).reshape(-1, 2)
        same_in_every_copy(arr["pairs"], pair0 + np.arange(len(pairs))[None, :], pairs, what + ": pairs")


@gpu
def test_front_beyond_the_caps(ctx, monkeypatch):
    """1.15 M reps of at most 32 segments in 13 440 tints: the 1 048 576 items of item_grid (k_heads, k_leader, k_nodes, k_mem_off)."""
    set_env(monkeypatch, HASH_BITS=None, PRUNE_LDS=None, PART_LDS=None, GRID_CAP=None)
    assert_twice(front_production_loops())
    tints, packed, want = front_distinct()
    big, src = front_tiled()
    assert big["rep_off"][-1] > 1048576 and max(big["n_seg"]) <= 32 and big["labels"].nbytes < 9e6
    check_front_copies(ctx.preprocess(big))


def check_front_copies(prep):
    """The tiled batch's preprocess() arrays: every copy's slice against the restatement of its distinct tint."""
    tints, packed, want = front_distinct()
    big, src = front_tiled()
    n_nodes = np.array([len(w["nodes"]) for w in want])
    assert prep["n_reps"] == big["rep_off"][-1] and prep["n_rows"] == n_nodes[src].sum()
    assert np.array_equal(np.diff(prep["rep_bits_off"]), np.diff(big["rep_off"])) and np.array_equal(np.diff(prep["row_off"]), n_nodes[src])
    assert np.array_equal(prep["bits_off"], prep["row_off"]) and np.array_equal(np.diff(prep["adj_off"]), (n_nodes * ((n_nodes + 63) // 64))[src])
    for d, w in enumerate(want):
        what = "copies of tint %d" % d
        M = int(packed["n_seg"][d])
        at, reps = gu.copies(big["rep_off"], src, d)
        for name, key in (("i_bits", "I"), ("c_bits", "C")):
            same_in_every_copy(prep[name], reps, pack_rows(w[key], M).reshape(-1), what + ": " + key)
        for name, values in (("raw_first", [x[0] for x in w["raw"]]), ("raw_last", [x[1] for x in w["raw"]]), ("first", [x[0] for x in w["FL"]]),
                             ("last", [x[1] for x in w["FL"]]), ("rep_node", w["rep_node"]), ("mem", [i for nd in w["nodes"] for i in nd[1]])):
            same_in_every_copy(prep[name], reps, values, what + ": " + name)
        lead = [nd[0] for nd in w["nodes"]]
        _, rows = gu.copies(prep["row_off"], src, d)
        for name, values in (("node_rep", lead), ("bits", pack_rows([w["I"][i] for i in lead], M).reshape(-1)), ("node_first", [w["FL"][i][0] for i in lead]),
                             ("node_last", [w["FL"][i][1] for i in lead]), ("node_tail", [w["tail"][i] for i in lead])):
            same_in_every_copy(prep[name], rows, values, what + ": " + name)
        mo = prep["mem_off"][prep["row_off"][at][:, None] + np.arange(len(lead) + 1)[None, :]] - big["rep_off"][at][:, None]
        every_row_is(mo, np.cumsum([0] + [len(nd[1]) for nd in w["nodes"]]), what + ": member offsets")


# ---- the same arithmetic without a device -----------------------------------------------------------------------------------------
def host_staged(tints):
    """The tints as the host's preprocess_ilp() and the oracle's partition_reads() leave them (what stage() does on the device)."""
    for tint in tints:
        cluster_prep.preprocess_ilp(tint, CONSTANT)
        cluster_oracle.partition_reads(tint, 1000)
    return tints


def test_batches_run_their_loops_twice(fuzz, batches):
    assert sorted(gu.CAPS) == sorted({cap for cap, _ in gu.LAUNCHES.values()}) and len(gu.CAPS) == 10
    assert gu.striding_kernels() == sorted(gu.LAUNCHES)                                   # every kernel that reads gridDim is in the table
    assert gu.trips("k_degree", 16384) == 1 and gu.trips("k_degree", 16385) == 2 and gu.trips("k_degree", 13, 3) == 2 and gu.trips("k_chunk", 257, 1) == 2
    graph_rows = [len(cluster_prep.unique_structures(t)) for t in t_graph.batched_tints()]
    rounds = host_staged(round_batch())
    round_want = [ru.restate(rounds[t], rounds[t]["partitions"][q][1], rem) for t, q, rem in whole(rounds)]
    grid = host_staged(grid_tints())
    grid_sets = [list(range(len(rem))) if ru.restate(grid[t], grid[t]["partitions"][q][1], rem)["refused"] is None else [] for t, q, rem in whole(grid)]
    for cap in (1, 3):
        assert_twice(front_loops(fuzz, cap))
        for name, names in GROUP_LOOPS.items():
            assert_twice(group_loops(batches[name], cap), names)
        for edge_walk in (True, False):
            assert_twice(graph_loops(graph_rows, cap, edge_walk))
        for per_pass in (True, False):
            assert_twice(crafted_loops(cap, per_pass))
        assert_twice(round_loops(whole(rounds), round_want, cap))
        assert_twice(readout_loops(grid, whole(grid), grid_sets, cap))
    # the production batches: every loop they name, with the knob unset
    loops = graph_production_loops()
    assert sorted(loops) == sorted(["k_compat", "k_degree", "k_deg1", "k_prune", "k_prune_edges", "k_cc_init", "k_cc_jump", "k_bounds", "k_chunk",
                                    "k_offsets", "k_cc_hook", "k_pairs", "k_members"])
    assert_twice(loops)
    big, src, members = graph_tiled()
    rows = np.diff(big["row_off"])
    assert rows.min() >= 40 and rows.max() <= 130 and rows.sum() > 4 * gu.CAPS["kCapWaveGrid"] and len(set(rows.tolist())) >= 12
    assert sum(a * (a + 1) // 2 for a in ((rows + 63) // 64).tolist()) > gu.CAPS["kCapCompat"]
    assert_twice(front_production_loops())
    front, fsrc = front_tiled()
    assert front["rep_off"][-1] > 256 * gu.CAPS["kCapItemGrid"] and front["n_seg"].max() <= 32 and front["labels"].nbytes < 9e6
    # the copies' order differs from block to block, and the tiled arrays are their sources' slices
    for s, T in ((src, 24), (fsrc, 24)):
        blocks = s.reshape(-1, T)
        assert (np.sort(blocks, axis=1) == np.arange(T)).all() and len({tuple(b) for b in blocks.tolist()}) == len(blocks)
    _, packed, small_members = graph_distinct()
    for t in (0, 1, len(src) // 2, len(src) - 1):
        d = int(src[t])
        for off, names in (("row_off", ("first", "last", "tail")), ("bits_off", ("bits",))):
            for name in names:
                assert np.array_equal(big[name][big[off][t]:big[off][t + 1]], packed[name][packed[off][d]:packed[off][d + 1]]), (t, name)
        assert big["adj_off"][t + 1] - big["adj_off"][t] == packed["adj_off"][d + 1] - packed["adj_off"][d] and big["n_seg"][t] == packed["n_seg"][d]
        r0, r1, s0, s1 = int(big["row_off"][t]), int(big["row_off"][t + 1]), int(packed["row_off"][d]), int(packed["row_off"][d + 1])
        assert np.array_equal(np.diff(members["mem_off"][r0:r1 + 1]), np.diff(small_members["mem_off"][s0:s1 + 1]))
        assert np.array_equal(members["mem"][members["mem_off"][r0]:members["mem_off"][r1]],
                              small_members["mem"][small_members["mem_off"][s0]:small_members["mem_off"][s1]])
