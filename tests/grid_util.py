"""Shared helpers of the cluster library's grid tests (tests/test_gpu_cluster_grid.py): the caps of the capped launches as
freddie_amd/csrc/freddie_cluster.hip names them, how often a launch's grid-stride loop runs for a given amount of work, and
batches large enough for the production caps, tiled in numpy from a couple of dozen distinct tints."""
import os
import re

import numpy as np

_SRC = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "freddie_amd", "csrc", "freddie_cluster.hip")).read()
CAPS = {name: int(value) for name, value in re.findall(r"^constexpr int (kCap\w+) = (\d+);", _SRC, re.M)}

# kernel -> (its cap, the work units a workgroup takes in one iteration of its loop): a workgroup is 256 threads, four waves
LAUNCHES = dict(
    k_compat=("kCapCompat", 1), k_degree=("kCapDegree", 4), k_deg1=("kCapDegree", 4), k_prune=("kCapPrune", 4), k_prune_edges=("kCapPruneEdges", 4),
    k_cc_init=("kCapRowGrid", 256), k_cc_jump=("kCapRowGrid", 256), k_bounds=("kCapRowGrid", 256), k_chunk=("kCapRowGrid", 256),
    k_offsets=("kCapRowGrid", 256), k_cc_hook=("kCapWaveGrid", 4), k_pairs=("kCapWaveGrid", 4), k_members=("kCapWaveGrid", 4),
    k_heads=("kCapItemGrid", 256), k_leader=("kCapItemGrid", 256), k_nodes=("kCapItemGrid", 256), k_mem_off=("kCapItemGrid", 256),
    k_gleader=("kCapItemGrid", 256), k_greps=("kCapItemGrid", 256), k_rows=("kCapSlots", 256), k_gkeys=("kCapSlots", 256),
    k_readout_corr=("kCapSlots", 256), k_ggather=("kCapGather", 256), k_gap_keys=("kCapGaps", 256), k_gap_heads=("kCapGaps", 256),
    k_gap_groups=("kCapGaps", 256), k_gap_fill=("kCapGaps", 256))


def striding_kernels():
    """The __global__ kernels of the source whose body reads gridDim: those that walk beyond their grid."""
    bodies = re.split(r"__global__ void (?:__launch_bounds__\(\w+\) )?(\w+)\(", _SRC)[1:]
    return sorted({name for name, body in zip(bodies[0::2], bodies[1::2]) if "gridDim" in body})


def ceil_div(a, b):
    return -(-int(a) // int(b))


def trips(kernel, items, knob=None, grid_work=None):
    """How often the busiest workgroup of `kernel` runs its grid-stride loop over `items` work units, under FCLU_GRID_CAP=knob (None:
    unset).  grid_work: what the host sizes the grid by, where that is not the loop's own count (k_chunk's one entry more)."""
    cap, share = LAUNCHES[kernel]
    grid = min(ceil_div(items if grid_work is None else grid_work, share), CAPS[cap])
    if knob is not None:
        grid = min(grid, int(knob))
    return ceil_div(items, grid * share) if grid > 0 else 0


def slots(counts, units):
    """The lane slots of k_rows / k_gkeys / k_readout_corr: an item gets the smallest power of two of lanes that holds its units (64 at
    the most), and a tint's (problem's) slots start at a multiple of 64."""
    total = 0
    for n, u in zip(counts, units):
        g = 1
        while g < 64 and g < u:
            g *= 2
        total += ceil_div(int(n) * g, 64) * 64
    return total


def graph_trips(row_counts, knob=None, edge_chunks=1):
    """{kernel: trips} of the graph's per-pass kernels (FCLU_PRUNE_LDS=0) for tints of the given unique-row counts."""
    R = int(sum(row_counts))
    aw = [ceil_div(n, 64) for n in row_counts]
    tiles, words = sum(a * (a + 1) // 2 for a in aw), sum(aw)
    return dict(k_compat=trips("k_compat", tiles, knob), k_degree=trips("k_degree", R, knob), k_deg1=trips("k_deg1", words, knob),
                k_prune=trips("k_prune", R, knob), k_prune_edges=trips("k_prune_edges", R * edge_chunks, knob))


def partition_trips(R, T, knob=None):
    """{kernel: trips} of the partition's kernels for R rows in T tints."""
    out = {k: trips(k, R, knob, R + 1) for k in ("k_cc_init", "k_cc_jump", "k_bounds")}
    out["k_chunk"] = trips("k_chunk", R + 1, knob)
    out["k_offsets"] = trips("k_offsets", max(R, T) + 1, knob)
    out.update({k: trips(k, R, knob) for k in ("k_cc_hook", "k_pairs", "k_members")})
    return out


def front_trips(rep_counts, n_seg, knob=None):
    """{kernel: trips} of the rows and the dedupe for tints of the given rep and segment counts."""
    N = int(sum(rep_counts))
    n_slots = slots(rep_counts, [max(ceil_div(m, 32), 1) for m in n_seg])
    return dict(k_rows=trips("k_rows", n_slots, knob), k_heads=trips("k_heads", N, knob), k_leader=trips("k_leader", N, knob),
                k_nodes=trips("k_nodes", N, knob, N + 1), k_mem_off=trips("k_mem_off", N + 1, knob))


def group_trips(a, n_rep_words, knob=None):
    """{kernel: trips} of the read grouping for the fclu_segment arrays a, whose reps' rows have n_rep_words label words in all."""
    counts = np.diff(a["read_off"]).tolist()
    N = int(a["read_off"][-1])
    lw = [max(ceil_div(m, 16), 1) for m in a["n_seg"]]
    units = [w // 4 if w % 4 == 0 and int(o) % 4 == 0 else w for w, o in zip(lw, a["lab_off"])]
    return dict(k_gkeys=trips("k_gkeys", slots(counts, units), knob), k_heads=trips("k_heads", N, knob), k_gleader=trips("k_gleader", N, knob),
                k_greps=trips("k_greps", N, knob), k_mem_off=trips("k_mem_off", N + 1, knob), k_ggather=trips("k_ggather", n_rep_words, knob))


def round_trips(P, C, G, n_grp, knob=None):
    """{kernel: trips} of the gap kernels of a round: P problems, C columns, G gap rows, n_grp groups."""
    return dict(k_gap_keys=trips("k_gap_keys", C, knob), k_gap_heads=trips("k_gap_heads", G, knob, max(G, P) + 1),
                k_gap_groups=trips("k_gap_groups", max(G, P) + 1, knob), k_gap_fill=trips("k_gap_fill", n_grp, knob))


# ---- tiled batches --------------------------------------------------------------------------------------------------------
def gather_csr(off, src):
    """The segments src of a CSR offset array laid end to end: (their offsets, the index of every element in the old array)."""
    off = np.asarray(off, np.int64)
    src = np.asarray(src, np.int64)
    n = off[src + 1] - off[src]
    new_off = np.zeros(len(src) + 1, np.int64)
    np.cumsum(n, out=new_off[1:])
    idx = np.repeat(off[src] - new_off[:-1], n) + np.arange(int(new_off[-1]), dtype=np.int64)
    return new_off, idx


def block_orders(T, k, seed=1):
    """The source tint of every tint of k blocks of T: each block another permutation, so that a tint's neighbours -- and whatever
    stands a grid stride further on -- differ from block to block."""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.permutation(T) for _ in range(k)])


# offset array -> the arrays it indexes, for pack_structures() and pack_labels() dicts; adj_off indexes the result alone
_LAYOUT = dict(row_off=("first", "last", "tail"), bits_off=("bits",), adj_off=(), rep_off=("tail",), lab_off=("labels",))


def tile_packed(packed, k, members=None, seed=1):
    """k permuted copies of every tint of a pack_structures() or pack_labels() batch as one batch, in numpy: (the batch, src = the tint
    each of its tints is a copy of[, the tiled pack_members() dict])."""
    src = block_orders(packed["n_tint"], k, seed)
    out = dict(n_tint=len(src), n_seg=np.asarray(packed["n_seg"])[src])
    for off_name, names in _LAYOUT.items():
        if off_name in packed:
            out[off_name], idx = gather_csr(packed[off_name], src)
            for name in names:
                out[name] = np.ascontiguousarray(np.asarray(packed[name])[idx])
    if members is None:
        return out, src
    _, rows = gather_csr(packed["row_off"], src)
    mem_off, idx = gather_csr(members["mem_off"], rows)
    return out, src, dict(mem_off=mem_off, mem=np.ascontiguousarray(np.asarray(members["mem"])[idx]))


def copies(off, src, d, width=None):
    """Index array [copies of tint d, its elements]: where every copy of source tint d keeps its elements of an array indexed by off."""
    at = np.flatnonzero(src == d)
    n = int(off[at[0] + 1] - off[at[0]]) if width is None else width
    return at, off[at][:, None] + np.arange(n, dtype=np.int64)[None, :]
