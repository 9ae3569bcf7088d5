"""The compatibility and pruning cases (tests/compat_cases.py) on the CPU: the model equals the oracle (oracle/cluster_oracle.py:
compat_edges, prune) wherever the oracle's pair loop is affordable; every case reaches the edge it was built for, checked from its
inputs; each mutation a case names changes that case's matrix, and every mutation is named somewhere; and the pruning reaches its
fixed point after at most one removing pass on every case (DESIGN.md has the argument)."""
import numpy as np
import pytest

import cluster_util as cu
import compat_cases as cc
from freddie_amd import cluster_prep
from oracle import cluster_oracle

NAMES = [x.name for x in cc.all_tints()]


def oracle_matrices(structures):
    n = len(structures)
    edges = cluster_oracle.compat_edges(structures)
    raw = np.zeros((n, n), bool)
    for i, j in edges:
        raw[i, j] = raw[j, i] = True
    nb, passes = cluster_oracle.prune(n, edges)
    pruned = np.zeros((n, n), bool)
    for i, s in enumerate(nb):
        pruned[i, list(s)] = True
    return raw, pruned, passes


# ---- the model is the oracle ---------------------------------------------------------------------------------------------------
SMALL = [x.name for x in cc.all_tints() if x.n <= 130]     # Groups R and W up to 130 rows -- 207, 208 and 300 words a row among them -- and
                                                            # the small Group P copy


@pytest.mark.parametrize("name", SMALL)
def test_model_equals_oracle_on_the_small_cases(name):
    """Whole matrices: compat_edges, prune and its passes."""
    raw, pruned, passes = cc.model_of(name)
    o_raw, o_pruned, o_passes = oracle_matrices(cc.structures(cc.tint(name)))
    assert np.array_equal(raw, o_raw) and np.array_equal(pruned, o_pruned) and passes == o_passes


def test_the_small_cases_are_the_ones_asked_for():
    assert set(SMALL) == {"R-special", "P-130"} | {"W-%d" % M for M in cc.W_SEGS}


@pytest.mark.parametrize("seed", range(36))
def test_model_equals_oracle_on_random_structure_sets(seed):
    rng = np.random.default_rng(seed)
    n, m = int(rng.integers(2, 70)), int(rng.integers(1, 90))
    t = cu.random_tint(4000 + seed, n, m, n_isoforms=int(rng.integers(1, 8)), noise=float(rng.choice([0.0, 0.03, 0.1])),
                       tail_p=float(rng.choice([0.0, 0.3, 0.6])))
    uniq = cluster_prep.unique_structures(t)
    rows = np.array([u[0][0] for u in uniq], bool).reshape(len(uniq), m)
    first, last = [u[0][1][0] for u in uniq], [u[0][1][1] for u in uniq]
    tail = ["NSE".index(u[0][1][2]) for u in uniq]
    raw = cc.compat_model(rows, first, last, tail)
    pruned, passes = cc.prune_model(raw)
    o_raw, o_pruned, o_passes = oracle_matrices(uniq)
    assert np.array_equal(raw, o_raw) and np.array_equal(pruned, o_pruned) and passes == o_passes


def test_pack_is_pack_structures():
    """pack() lays a tint out as cluster_prep.pack_structures() does."""
    xs = [cc.tint("R-special"), cc.tint("W-33"), cc.tint("P-130")]
    a = cc.pack(xs)
    b = cluster_prep.pack_structures([cc.structures(x) for x in xs])
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---- the library would take them -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_rows_are_what_the_library_takes(name):
    """check_rows: first >= -1, last < n_seg, tail <= 2, every covered segment inside [first, last]; at most kMaxWords words a row."""
    x = cc.tint(name)
    assert (x.first >= -1).all() and (x.last < x.n_seg).all() and (x.tail <= 2).all() and x.n_seg <= cc.MAX_WORDS * 32
    seg = np.arange(x.n_seg)
    assert not (x.rows & ((seg[None, :] < x.first[:, None]) | (seg[None, :] > x.last[:, None]))).any()


# ---- mutations ---------------------------------------------------------------------------------------------------------------------
MUTATED = [(x.name, m) for x in cc.all_tints() for m in x.mutations]


@pytest.mark.parametrize("name,mutation", MUTATED)
def test_named_mutation_changes_the_case(name, mutation):
    x = cc.tint(name)
    raw, pruned, _ = cc.model_of(name)
    if mutation in cc.COMPAT_MUTATIONS:
        assert not np.array_equal(cc.compat_model(x.rows, x.first, x.last, x.tail, mutation), raw), (name, mutation)
    else:
        assert not np.array_equal(cc.prune_model(raw, mutation)[0], pruned), (name, mutation)


def test_every_mutation_is_named_and_every_case_names_one():
    named = {m for x in cc.all_tints() for m in x.mutations}
    assert named == set(cc.COMPAT_MUTATIONS) | set(cc.PRUNE_MUTATIONS)
    structural = {"W-1", "P-still-4161"}                    # one segment a row: nothing to differ in; a tint no pass touches
    assert {x.name for x in cc.all_tints() if not x.mutations} == structural


def test_passes_at_most_one_everywhere():
    assert {cc.model_of(n)[2] for n in NAMES} == {0, 1}
    assert cc.model_of("P-still-4161")[2] == 0 and all(cc.model_of("P-%d" % n)[2] == 1 for n in cc.P_SIZES)


# ---- every case reaches its edge ------------------------------------------------------------------------------------------------------
def test_rule_grid_reaches_its_edges():
    grid = cc.rule_grid()
    assert 1500 <= len(grid) <= 2000 and sum(x.n for x in cc.group_r()) <= 4200 and max(x.n for x in cc.group_r()) <= 500
    seen = {g[:4] for g in grid}
    assert {g[0] for g in seen} == set(cc.R_STARTS) and {g[1] for g in seen} == set(cc.R_LENGTHS)
    assert {g[2] for g in seen} == set(cc.R_DIFFS) and {g[3] for g in seen} == set(cc.R_SAME)
    for f, o, diff, same, a, b in grid:
        l = f + o - 1
        A, B = np.zeros(cc.R_SEG, bool), np.zeros(cc.R_SEG, bool)
        A[a[3]] = True; B[b[3]] = True
        assert (max(a[0], b[0]), min(a[1], b[1])) == (f, l)                              # the overlap is the one asked for
        assert int((A[f:l + 1] ^ B[f:l + 1]).sum()) == diff
        n_same = int((A[f:l + 1] & B[f:l + 1]).sum())
        assert n_same == {"none": 0, "one": 1, "many": o - diff}[same] or (same == "many" and o == diff)
        assert B[l + 1] and (f == 0 or A[f - 1])                                        # covered bits just outside the overlap
    # the overlap's ends at a word's first and last bit, overlaps of one, two and three-plus words, differing bits on both sides of a word edge
    assert {f & 31 for f, o, *_ in grid} >= {0, 1, 30, 31} and {(f + o - 1) & 31 for f, o, *_ in grid} >= {0, 1, 30, 31}
    assert {min((f + o - 1) // 32 - f // 32, 2) for f, o, *_ in grid} == {0, 1, 2}
    sides = set()
    for f, o, diff, same, a, b in grid:
        A, B = np.zeros(cc.R_SEG, bool), np.zeros(cc.R_SEG, bool)
        A[a[3]] = True; B[b[3]] = True
        d = np.flatnonzero(A[f:f + o] ^ B[f:f + o]) + f
        sides |= {int(p) & 31 for p in d if f < p < f + o - 1}
    assert {0, 31} <= sides


def test_special_tint_reaches_its_edges():
    x = cc.tint("R-special")
    raw = cc.model_of("R-special")[0]
    a, b = x.what["adjacent"]
    assert x.first[b] - x.last[a] == 1 and not raw[a, b]                                 # o = 0
    a, b = x.what["apart"]
    assert x.first[b] - x.last[a] == 2 and not raw[a, b]                                 # o = -1
    assert len(x.what["tails"]) == 18 and {(ta, tb, acc) for _, _, ta, tb, acc in x.what["tails"]} == {
        (ta, tb, acc) for ta in range(3) for tb in range(3) for acc in (True, False)}
    for a, b, ta, tb, accept in x.what["tails"]:
        assert (x.tail[a], x.tail[b]) == (ta, tb)
        assert raw[a, b] == (accept and not (ta and tb and ta != tb)), (ta, tb, accept)
    e1, e2, full = x.what["empty"]
    assert (x.first[e1], x.last[e1]) == (-1, x.n_seg - 1) == (x.first[e2], x.last[e2]) and not x.rows[[e1, e2]].any() and x.rows[full].all()
    assert not raw[e1].any() and not raw[e2].any()


@pytest.mark.parametrize("M", cc.W_SEGS)
def test_width_tints_reach_their_edges(M):
    x = cc.tint("W-%d" % M)
    raw = cc.model_of(x.name)[0]
    W = max((M + 31) // 32, 1)
    assert x.n == 65 and (x.n + 63) // 64 == 2 and x.words == W
    assert {6623: 207, 6624: 207, 6625: 208, 9599: 300, 9600: 300, 1: 1, 31: 1, 32: 1, 33: 2, 64: 2, 65: 3}[M] == W
    assert (W <= cc.RANK_WORDS) == (M <= 6624)
    assert x.rows[0].all() and (x.first[0], x.last[0]) == (0, M - 1)                      # the fully covered row: rank 32 (W - 1) at its last word
    assert int(x.rows[0, :32 * (W - 1)].sum()) == 32 * (W - 1)
    assert x.first[1] == 32 * (W - 1) and x.last[2] == min(31, M - 1)                     # overlap with row 0: the last / the first word only
    if M > 3:
        assert x.rows[64].sum() == M - 1 and not x.rows[64, M - 2] and raw[0, 64] and raw[64, 0]
    want_words = sorted({0, W // 2, W - 1})
    if M >= 5:
        assert sorted({w for w, _ in x.holes}) == want_words and {len(h) for _, h in x.holes} == {1, 2, 3}
        for k, (w, hole) in enumerate(x.holes):
            assert all(p // 32 == w for p in hole)
            row = 3 + k
            assert int((~x.rows[row]).sum()) == len(hole) and raw[0, row] == (len(hole) < 3)   # diff 1, 2: compatible; diff 3: not


GADGET_TINTS = ["P-%d" % n for n in cc.P_SIZES]


@pytest.mark.parametrize("name", GADGET_TINTS + ["P-still-4161"])
def test_gadgets_reach_their_edges(name):
    x = cc.tint(name)
    raw, pruned, passes = cc.model_of(name)
    deg = raw.sum(1)
    aw = (x.n + 63) // 64
    assert x.n_seg <= cc.RANK_WORDS * 32                                              # the default form is the rank form
    assert (x.n * aw <= cc.PRUNE_LDS_WORDS) == (x.n == 130)
    kinds = {}
    for g in x.gadgets:
        kinds.setdefault(g["kind"], []).append(g)
        rows = g["rows"]
        sub_raw, sub = raw[np.ix_(rows, rows)], pruned[np.ix_(rows, rows)]
        assert raw[rows].sum() == sub_raw.sum()                                       # a gadget's nodes touch nothing outside it
        if g["expect"] == "kept":
            assert np.array_equal(sub, sub_raw) and sub_raw.any()
        elif g["expect"] == "none":
            assert not sub.any() and (sub_raw.sum(1) >= 2).all() and not ((sub_raw.astype(int) @ sub_raw.astype(int)) * sub_raw).any()
        elif g["expect"] == "interior":                                               # a path in node order: the end edges stay
            k = len(rows)
            want = np.zeros((k, k), bool)
            for i in (0, k - 2):
                want[i, i + 1] = want[i + 1, i] = True
            assert np.array_equal(sub, want) and int(sub_raw.sum()) == 2 * (k - 1)
        elif g["expect"] == "x":                                                      # hub rows[0] loses exactly x = rows[1]
            hub, xx = rows[0], rows[1]
            assert deg[hub] == g["degree"] and raw[hub, xx] and not pruned[hub, xx] and not pruned[xx, hub]
            assert pruned[hub].sum() == g["degree"] - 1
            nb = np.flatnonzero(raw[hub])
            assert xx == (nb[0] if g["x"] == "first" else nb[-1])
            if g["placement"] == "word":
                assert len(set(nb // 64)) == 1
            elif x.n >= 1000 and g["degree"] >= 3:
                assert len(set(nb // 64)) >= 3
            if g.get("paired"):
                assert ((raw[hub].astype(int) @ raw.astype(int)) * raw[hub])[[v for v in nb if v != xx]].sum() >= g["degree"] - 2
    if name == "P-still-4161":
        assert passes == 0 and set(kinds) == {"star", "clique"} and max(r for g in x.gadgets for r in g["rows"]) >= cc.CHUNK
        return
    assert passes == 1
    hubs = [g for g in kinds["hub"] if g["degree"] > 1]
    assert {g["degree"] for g in kinds["hub"]} >= set(cc.HUB_DEGREES) and {g["x"] for g in hubs} == {"first", "last"}
    # x in the remainder batch of a row walked four neighbours at a time: the last of 5 and of 9, and every one of 2 and 3
    assert {g["degree"] for g in hubs if g["x"] == "last"} >= ({5, 9} if x.n >= 1000 else {9}) and {2, 3} <= {g["degree"] for g in hubs}
    if x.n >= 1000:
        assert {g["placement"] for g in hubs} >= {"word", "spread"} and any(g["paired"] for g in hubs)
        assert {(g["degree"], g["x"], g["placement"]) for g in kinds["hub"]} >= {(d, w, p) for d in cc.HUB_DEGREES for w in ("first", "last")
                                                                                  for p in ("word", "spread")}
    assert sorted(len(g["rows"]) for g in kinds["path"]) == [2, 3, 4, 5, 6]
    if x.n >= cc.CHUNK + 8:                                                           # the cases on both sides of column 4 096
        C = cc.CHUNK
        r, c, k = kinds["q2_triangle"][0]["rows"]
        assert r < C and c < C <= k and not (raw[r, :C] & raw[c, :C]).any() and (raw[r, C:] & raw[c, C:]).any() and pruned[r, c]
        r, k, c = kinds["high_c_low_common"][0]["rows"]
        assert r < C <= c and k < C and (raw[r, :C] & raw[c, :C]).any() and not (raw[r, C:] & raw[c, C:]).any() and pruned[r, c]
        r, c, k = kinds["high_c_high_common"][0]["rows"]
        assert r < C <= min(c, k) and not (raw[r, :C] & raw[c, :C]).any() and pruned[r, c] and not raw[r, :C].any()   # r: neighbours in chunk 1 only
        r, _, c = kinds["high_c_leaf"][0]["rows"]
        assert r < C <= c and deg[c] == 1 and deg[r] == 2 and not (raw[r] & raw[c]).any() and pruned[r, c]
        _, r, c, _ = kinds["high_c_removed"][0]["rows"]
        assert r < C <= c and raw[r, c] and not pruned[r, c] and not pruned[c, r] and not raw[c, C:].any()           # c: neighbours in chunk 0 only
        hub = kinds["star_high_leaves"][0]["rows"][0]
        assert hub < C and not raw[hub, :C].any() and raw[hub, C:].sum() == 3
        across = [g for g in hubs if g["placement"] == "across"][0]
        nb = np.flatnonzero(raw[across["rows"][0]])
        assert (nb >= C).sum() == 2 and across["rows"][1] >= C
    elif x.n == cc.CHUNK + 1:
        r, c, k = kinds["q2_triangle"][0]["rows"]
        assert k == cc.CHUNK and not (raw[r, :k] & raw[c, :k]).any() and pruned[r, c]


def test_batches_are_what_the_device_tests_assume():
    b = cc.batches()
    assert all(n in NAMES for names in b.values() for n in names)
    sizes = lambda key: [cc.tint(n).n for n in b[key]]
    assert sizes("P-mixed") == [130, 4161, 1100] and sizes("P-still+removing") == [4161, 1100]
    assert [cc.model_of(n)[2] for n in b["P-still+removing"]] == [0, 1]
    assert [cc.model_of(n)[2] for n in b["P-still+small"]] == [0, 1] and sizes("P-still+small") == [4161, 130]
    assert [cc.tint(n).words for n in b["W-6624+6625"]] == [207, 208]
    big = cc.tint("P-4161")
    assert big.n * ((big.n_seg + 31) // 32) <= 4161 * 131                               # the largest device input
