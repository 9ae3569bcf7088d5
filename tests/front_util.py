"""The front of the clustering stage's pre-ILP work restated in plain numpy / Python -- the yardstick of the GPU tests of
fclu_preprocess / fclu_partition_reads -- and generators of crafted label-row tints.

  rep_outputs()   per rep what preprocess_ilp() (py/freddie_cluster.py:285-310) and find_segment_read() (:175-183) give
  first_occurrence_dedupe()   the dedupe of :203-215: nodes in order of their smallest rep, members ascending
tests/test_cluster_front_host.py pins both against the fixtures the reference's own source wrote.
"""
import random

import numpy as np

TAILS = "NSE"


def rep_outputs(data, tail, M):
    """data: M label codes (0, 1, 2); tail: 0 'N', 1 'S', 2 'E'.  -> dict(I, C, raw, FL)."""
    I = [v & 1 for v in data[:M]]
    ones = [j for j, v in enumerate(I) if v == 1]
    raw = (ones[0], ones[-1]) if ones else (-1, M - 1)
    lo, hi = raw
    if tail == 1:
        lo = 0
    elif tail == 2:
        hi = M - 1
    C = [1 if (lo <= j <= hi and data[j] == 0) else 0 for j in range(M)]
    return dict(I=I, C=C, raw=raw, FL=(lo, hi))


def first_occurrence_dedupe(I_rows, FL, tail):
    """-> (nodes [(rep of first occurrence, [member reps ascending])] in first-occurrence order, rep_node [node per rep])."""
    seen, nodes, rep_node = dict(), [], []
    for i, row in enumerate(I_rows):
        key = (tuple(row), FL[i][0], FL[i][1], tail[i])
        if key not in seen:
            seen[key] = len(nodes)
            nodes.append((i, []))
        nodes[seen[key]][1].append(i)
        rep_node.append(seen[key])
    return nodes, rep_node


def tint_outputs(tint):
    """The restatement on a label tint (reads with 'data' and 'poly_tail'): dict(I, C, raw, FL, tail, nodes, rep_node)."""
    from freddie_amd import cluster_prep
    M = len(tint["segs"])
    tail = cluster_prep.tail_categories(tint).tolist()
    outs = [rep_outputs(tint["reads"][m[0]]["data"], tail[i], M) for i, m in enumerate(tint["read_reps"])]
    nodes, rep_node = first_occurrence_dedupe([o["I"] for o in outs], [o["FL"] for o in outs], tail)
    return dict(I=[o["I"] for o in outs], C=[o["C"] for o in outs], raw=[o["raw"] for o in outs], FL=[o["FL"] for o in outs],
                tail=tail, nodes=nodes, rep_node=rep_node)


_POLY = {0: [dict(), dict(SA=(5, 2)), dict(SA=(20, 1), ET=(30, 2)), dict(EA=(10, 4))],        # 'N': none, short, two entries, exactly 10
         1: [dict(SA=(11, 3)), dict(ST=(40, 0))], 2: [dict(EA=(25, 3)), dict(ET=(12, 7))]}


def label_tint(tid, rows, tails, rng):
    """A tint as read_segment() leaves it (one read a rep) from label rows and tail categories."""
    M = len(rows[0]) if rows else 0
    reads = [dict(id=i, name="r%d" % i, chr="c", strand="+", tint=tid, data=list(row), gaps=dict(), softclip=dict(),
                  poly_tail=dict(rng.choice(_POLY[tails[i]]))) for i, row in enumerate(rows)]
    return dict(id=tid, chr="c", segs=[(10 * j, 10 * j + 10, 10) for j in range(M)], reads=reads, read_reps=[[i] for i in range(len(rows))])


def crafted_tint(seed, n_reps, M, pool=6):
    """Rows drawn from a small pool (large, interleaved groups): label 2 at the ends and inside a span, all-zero and all-2 rows
    with every tail, rows equal in I that differ in the tail only, or in FL only through the tail's override."""
    rng = random.Random(seed)
    base = []
    for _ in range(pool):
        a = rng.randrange(M); b = rng.randrange(a, M)
        row = [0] * M
        for j in range(a, b + 1):
            row[j] = 1 if rng.random() < 0.7 else (2 if rng.random() < 0.4 else 0)
        if a > 0 and rng.random() < 0.5:
            row[rng.randrange(a)] = 2                                         # a 2 in front of the span
        if b + 1 < M and rng.random() < 0.5:
            row[rng.randrange(b + 1, M)] = 2                                  # and behind it
        base.append(row)
    base.append([0] * M)
    base.append([2] * M)
    twos = list(base[0]); twos[:] = [2 if v == 0 and rng.random() < 0.5 else v for v in twos]
    base.append(twos)                                                         # the same I as base[0], another C
    choices = [(row, t) for row in base for t in (0, 1, 2)]                   # the same row under every tail
    picks = [choices[rng.randrange(len(choices))] for _ in range(n_reps)]
    return label_tint(seed, [p[0] for p in picks], [p[1] for p in picks], rng)


def labels_from_preprocessed(tint, seed=0, twos=0.0, dup=0.0):
    """A label tint whose preprocess_ilp() gives the I / FL / categories of a cluster_util.random_tint(): label = I, a share
    `twos` of the zeros written as 2, and a share `dup` of the reps replaced by copies of earlier reps (so the dedupe collapses
    them)."""
    rng = random.Random(seed)
    n = len(tint["read_reps"])
    I = tint["ilp_data"]["I"]
    rows, tails = [], []
    for i in range(n):
        if i and rng.random() < dup:
            k = rng.randrange(i)
            rows.append(rows[k]); tails.append(tails[k])
            continue
        row = [2 if (v == 0 and twos and rng.random() < twos) else v for v in I[i]]
        rows.append(row)
        tails.append(TAILS.index(tint["reads"][tint["read_reps"][i][0]]["poly_tail_category"]))
    return label_tint(tint["id"], rows, tails, rng)


def check_prep_against(prep, packed, t, want):
    """Context.preprocess() arrays of tint t of a batch against tint_outputs() of that tint; exact."""
    r0, r1 = int(packed["rep_off"][t]), int(packed["rep_off"][t + 1])
    n, M = r1 - r0, int(packed["n_seg"][t])
    W = max((M + 31) // 32, 1)
    b0 = int(prep["rep_bits_off"][t])
    assert int(prep["rep_bits_off"][t + 1]) - b0 == n * W
    for name, key in (("i_bits", "I"), ("c_bits", "C")):
        words = prep[name][b0:b0 + n * W].reshape(n, W)
        got = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")
        assert not got[:, M:].any(), "%s: bits beyond M" % name
        assert got[:, :M].tolist() == want[key], "tint %d: %s differs" % (t, key)
    assert list(zip(prep["raw_first"][r0:r1].tolist(), prep["raw_last"][r0:r1].tolist())) == [tuple(x) for x in want["raw"]]
    assert list(zip(prep["first"][r0:r1].tolist(), prep["last"][r0:r1].tolist())) == [tuple(x) for x in want["FL"]]
    # nodes and members
    n0, n1 = int(prep["row_off"][t]), int(prep["row_off"][t + 1])
    nodes = want["nodes"]
    assert n1 - n0 == len(nodes), "tint %d: %d nodes, expected %d" % (t, n1 - n0, len(nodes))
    assert prep["rep_node"][r0:r1].tolist() == want["rep_node"]
    assert prep["node_rep"][n0:n1].tolist() == [nd[0] for nd in nodes]
    mo = prep["mem_off"]
    assert [prep["mem"][int(mo[q]):int(mo[q + 1])].tolist() for q in range(n0, n1)] == [nd[1] for nd in nodes]
    assert int(prep["bits_off"][t + 1] - prep["bits_off"][t]) == len(nodes) * W
    assert int(prep["adj_off"][t + 1] - prep["adj_off"][t]) == len(nodes) * ((len(nodes) + 63) // 64)
    nb = prep["bits"][int(prep["bits_off"][t]):int(prep["bits_off"][t + 1])].reshape(len(nodes), W)
    got = np.unpackbits(nb.view(np.uint8), axis=1, bitorder="little")[:, :M].tolist() if nodes else []
    assert got == [want["I"][nd[0]] for nd in nodes]
    assert list(zip(prep["node_first"][n0:n1].tolist(), prep["node_last"][n0:n1].tolist())) == [tuple(want["FL"][nd[0]]) for nd in nodes]
    assert prep["node_tail"][n0:n1].tolist() == [want["tail"][nd[0]] for nd in nodes]
