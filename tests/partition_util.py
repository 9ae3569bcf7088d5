"""Shared helpers of the partition tests (Context.partition / partition_adj): packed graphs, member lists with
multiplicities, the expected arrays from the CPU oracle's components plus a literal restatement of
py/freddie_cluster.py:258-274, and a vectorised numpy form of the same for graphs too large for Python loops."""
from math import ceil

import numpy as np

from oracle import cluster_oracle


def arrays_to_json(arr, t):
    """tint t of a batch result in the fixtures' JSON shape: [[rids, [[rid_1, rid_2], ...]], ...]."""
    out = []
    for q in range(int(arr["tint_part_off"][t]), int(arr["tint_part_off"][t + 1])):
        rids = arr["part_rids"][arr["part_rid_off"][q]:arr["part_rid_off"][q + 1]].tolist()
        out.append([rids, arr["pairs"][arr["part_pair_off"][q]:arr["part_pair_off"][q + 1]].tolist()])
    return out


def pack_adj(mats):
    """(row_off, adj_off, adj) in the layout of fclu_compat_graph for a list of boolean N x N matrices."""
    row_off, adj_off, words = [0], [0], []
    for A in mats:
        n = A.shape[0]
        aw = (n + 63) // 64
        row_off.append(row_off[-1] + n)
        adj_off.append(adj_off[-1] + n * aw)
        if n:
            bits = np.zeros((n, aw * 64), np.uint8)
            bits[:, :n] = A
            words.append(np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(-1))
    adj = np.concatenate(words) if words else np.zeros(0, np.uint64)
    return np.array(row_off, np.int64), np.array(adj_off, np.int64), adj


def members_for(sizes, max_mult=5):
    """Member lists for tints of the given node counts: multiplicities 1 .. max_mult, rep ids neither contiguous nor sorted.
    Returns (per tint [[rid, ...] per node], dict(mem_off, mem))."""
    per_tint, flat, counter = [], [], 0
    for t, n in enumerate(sizes):
        lists = []
        for i in range(n):
            mult = 1 + (i * 7 + t) % max_mult
            lists.append([(c * 7919 + 13) % 1000003 for c in range(counter, counter + mult)])
            counter += mult
        per_tint.append(lists)
        flat.extend(lists)
    mem_off = np.zeros(len(flat) + 1, np.int64)
    np.cumsum([len(x) for x in flat], out=mem_off[1:])
    mem = np.array([r for x in flat for r in x], np.int32)
    return per_tint, dict(mem_off=mem_off, mem=mem)


def oracle_components(A):
    n = A.shape[0]
    return cluster_oracle.connected_components(n, [set(np.flatnonzero(A[i]).tolist()) for i in range(n)])


def expected_partitions(A, members, maximum_ilp_size):
    """(labels, [(nodes, rids, pairs)]) of one graph: the oracle's components, then :258-274 word for word."""
    n = A.shape[0]
    labels = np.zeros(n, np.int32)
    parts = []
    for comp in oracle_components(A):
        labels[comp] = comp[0]
        for c in cluster_oracle.split_list_evenly(comp, maximum_ilp_size):
            rids, incomp = [], []
            for idx, i in enumerate(c):
                rids.extend(members[i])
                for j in c[idx + 1:]:
                    if A[i, j]:
                        continue
                    for rid_1 in members[i]:
                        for rid_2 in members[j]:
                            incomp.append([rid_1, rid_2])
            parts.append((list(c), rids, incomp))
    return labels, parts


def pair_count(A, nodes, mult):
    """sum of mult_i * mult_j over the non-adjacent i < j of a chunk, in numpy."""
    nodes = np.asarray(nodes)
    non = np.triu(~A[np.ix_(nodes, nodes)], 1)
    m = mult[nodes].astype(np.int64)
    return int((non * np.outer(m, m)).sum())


def expected_partitions_numpy(A, labels, mem_off, mem, maximum_ilp_size):
    """The same rule vectorised, from component labels (smallest node of each component): [(nodes, rids, pairs int32 [n, 2])]."""
    parts = []
    order = np.argsort(labels, kind="stable")
    groups = np.split(order, np.flatnonzero(np.diff(labels[order])) + 1) if len(order) else []
    mult = np.diff(mem_off)
    for comp in groups:
        n = len(comp)
        p = ceil(n / maximum_ilp_size)
        s = ceil(n / p)
        for idx in range(0, p * s, s):
            c = comp[idx:idx + s]
            rids = np.concatenate([mem[mem_off[i]:mem_off[i + 1]] for i in c])
            ii, jj = np.nonzero(np.triu(~A[np.ix_(c, c)], 1))             # row-major: i ascending, then j ascending
            I, J = c[ii], c[jj]
            mi, mj = mult[I], mult[J]
            tot = mi * mj
            start = np.cumsum(tot) - tot
            which = np.repeat(np.arange(len(I)), tot)
            local = np.arange(int(tot.sum())) - start[which]
            a, b = local // mj[which], local % mj[which]
            pairs = np.stack([mem[mem_off[I][which] + a], mem[mem_off[J][which] + b]], axis=1).astype(np.int32).reshape(-1, 2)
            parts.append((c.tolist(), rids.tolist(), pairs))
    return parts


# ---- crafted graphs ---------------------------------------------------------------------------------------------
def _from_edges(n, edges):
    A = np.zeros((n, n), bool)
    for i, j in edges:
        if i != j:
            A[i, j] = A[j, i] = True
    return A


def path(n):
    return _from_edges(n, [(i, i + 1) for i in range(n - 1)])


def shuffled_path(n, seed=5):
    order = np.random.default_rng(seed).permutation(n).tolist()
    return _from_edges(n, list(zip(order[:-1], order[1:])))


def ring(n):
    return _from_edges(n, [(i, (i + 1) % n) for i in range(n)])


def star(n):
    """The hub is the LAST node: every label has to travel down to node 0 through it."""
    return _from_edges(n, [(n - 1, i) for i in range(n - 1)])


def two_cliques(n):
    h = n // 2
    e = [(i, j) for i in range(h) for j in range(i + 1, h)] + [(i, j) for i in range(h, n) for j in range(i + 1, n)]
    return _from_edges(n, e + ([(h - 1, h)] if 0 < h < n else []))


def isolated(n):
    return np.zeros((n, n), bool)


def complete(n):
    return ~np.eye(n, dtype=bool)


def straddle(n):
    """One component made of every third node around each 64-column word boundary (the whole range when n is small), the rest
    isolated: its nodes' bits lie in two words of a row and its chunks interleave with other components' nodes."""
    nodes = [v for b in range(64, n, 64) for v in range(max(b - 9, 0), min(b + 9, n), 3)] or list(range(0, n, 3))
    return _from_edges(n, list(zip(nodes[:-1], nodes[1:])))


GRAPHS = dict(path=path, shuffled_path=shuffled_path, ring=ring, star=star, two_cliques=two_cliques, isolated=isolated,
              complete=complete, straddle=straddle)
