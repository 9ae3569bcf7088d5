"""segment_*.tsv files to read_reps, ilp_data's rows and tint['partitions'] on the GPU (fclu_group_reads, fclu_partition_segment
behind cluster_prep.read_segment_arrays): against the pinned Python side -- cluster_prep.read_segment() for the grouping, host
preprocess_ilp() and the partition oracle behind it.  Integer work: everything is compared exactly."""
import copy
import os
import random

import numpy as np
import pytest

import cluster_util as cu
import front_util as fu
from freddie_amd import cluster_prep
from oracle import cluster_oracle

pytestmark = pytest.mark.gpu

CONSTANT = dict(recycle_model="constant")
SIZE = 7
MS = [1, 16, 17, 32, 33, 64, 128, 1025, 2049]   # label-word and bit-word boundaries, rows of whole 16-byte quads, more words than lanes
READS = [1, 63, 64, 65]


# ---- files ---------------------------------------------------------------------------------------------------------
def gap_field(rng, M, n_internal):
    """A gaps field: n_internal internal gaps with distinct keys, sometimes soft clips and poly tails."""
    out = []
    for j in sorted(rng.sample(range(M - 1), n_internal)) if n_internal else []:
        out.append("%d-%d:%d," % (j, j + 1, rng.choice([3, 10, 11, 25])))
    if rng.random() < 0.3:
        out.insert(rng.randrange(len(out) + 1), "%sSC:%d," % (rng.choice("SE"), rng.randrange(50)))
    for key in rng.sample(["SA", "ST", "EA", "ET"], rng.choice([0, 0, 1, 1, 2])):
        out.append("%s_%d:%d," % (key, rng.choice([5, 10, 11, 30]), rng.choice([0, 10, 11, 40])))
    return out


def same_rep_variant(rng, row, gaps):
    """Another read of the same rep: 0 <-> 2, small gaps resized, soft clips changed, the poly tail's base swapped."""
    row = [rng.choice("02") if c in "02" and rng.random() < 0.3 else c for c in row]
    out = []
    for g in gaps:
        if g[0].isdigit() and int(g[:-1].split(":")[1]) <= 10 and rng.random() < 0.5:
            g = g.split(":")[0] + ":%d," % rng.randrange(11)
        elif g[1:3] == "SC":
            g = g[:4] + "%d," % rng.randrange(50)
        out.append(g)
    return row, out


def tint_lines(rng, tid, M, n, pool, rid0=0, distinct=False):
    variants = []
    for _ in range(pool):
        a = rng.randrange(M); b = rng.randrange(a, M)
        row = ["0"] * M
        for j in range(a, b + 1):
            row[j] = "1" if rng.random() < 0.7 else rng.choice("02")
        for j in rng.sample(range(M), min(M, 3)):
            if row[j] == "0":
                row[j] = "2"
        variants.append((row, gap_field(rng, M, rng.randrange(min(M, 4)))))
    lines = ["#ctg\t%d\t%s\n" % (tid, ",".join(str(100 + 10 * j) for j in range(M + 1)))]
    for i in range(n):
        row, gaps = same_rep_variant(rng, *variants[i % pool if distinct else rng.randrange(pool)])
        if distinct:
            gaps = ["0-1:%d," % (11 + i)] + [g for g in gaps if not g.startswith("0-1:")]
        lines.append("%d\tr%d\tctg\t%s\t%d\t%s\t%s\n" % (rid0 + i, i, rng.choice("+-"), tid, "".join(row), "".join(gaps)))
    return lines


PAIRS_M = 80
ROW = "0011101110" + "10" * 35


def pair_lines(tid):
    """Reads that differ in ONE thing from the one in front of them (see test_pairs for what each pair must do)."""
    many = "".join("%d-%d:%d," % (j, j + 1, 11 + j) for j in range(70))
    cases = [(ROW, ""), (ROW.replace("0", "2", 3), ""),                                        # 0 vs 2: one rep, C from the first read
             (ROW, "3-4:10,"), (ROW, "3-4:5,"), (ROW, "3-4:11,"),                              # 10 vs 5: one rep; 10 vs 11: two
             (ROW, "3-4:11,5-6:12,"), (ROW, "3-4:12,5-6:11,"),                                 # gap order
             (ROW, "SA_5:12,"), (ROW, "EA_5:12,"), (ROW, "3-4:12,"),                           # S vs E; gap token vs poly token, same number
             (ROW, many), (ROW, many[:-3] + "99,"),                                            # 70 tokens, the last differs
             (ROW, many[:many.index("64-65")]), (ROW, "7-8:13,"),                              # 64 tokens; one token
             (ROW[:-1] + "1", ""), (ROW[:-1] + "2", ""),                                       # the last label of the row (2 counts as 0)
             (ROW, "ST_20:12,"), (ROW, "SA_5:12,ESC:3,")]                                      # same token, another tail category: one rep
    lines = ["#ctg\t%d\t%s\n" % (tid, ",".join(str(10 * j) for j in range(PAIRS_M + 1)))]
    for i, (row, gaps) in enumerate(cases):
        lines.append("%d\tp%d\tctg\t+\t%d\t%s\t%s\n" % (i, i, tid, row, gaps))
    return lines


def expectation(paths):
    """Per tint of the batch, in batch order: (the mirror's tint, the same after host preprocess_ilp() + the oracle's partition_reads())."""
    out = []
    for p in paths:
        for tint in cluster_prep.read_segment(p).values():
            done = copy.deepcopy(tint)
            cluster_prep.preprocess_ilp(done, CONSTANT)
            cluster_oracle.partition_reads(done, SIZE)
            out.append((tint, done))
    return out


class Batch:
    def __init__(self, d, name, files):
        self.paths = []
        for i, lines in enumerate(files):
            p = os.path.join(str(d), "segment_%s_%d.tsv" % (name, i))
            open(p, "w").write("".join(lines))
            self.paths.append(p)
        self.want = expectation(self.paths)
        self.arrays = cluster_prep.read_segment_arrays(self.paths, 4)
        assert not self.arrays.declined


@pytest.fixture(scope="module")
def ctx():
    c = cluster_prep.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batches(tmp_path_factory):
    d = tmp_path_factory.mktemp("groups")
    rng = random.Random(11)
    shapes = [tint_lines(rng, 100 * a + b, M, n, pool=1 + (a + b) % 5) for a, M in enumerate(MS) for b, n in enumerate(READS)]
    many = [sum((tint_lines(rng, 1000 + t, rng.choice([1, 5, 16, 17, 40]), rng.randrange(3, 41), pool=rng.randrange(1, 6)) for t in range(65)), [])]
    big = [tint_lines(rng, 1, 40, 5000, pool=9), tint_lines(rng, 2, 33, 500, pool=7) + tint_lines(rng, 3, 40, 200, pool=40, distinct=True)]
    small = [pair_lines(4), tint_lines(rng, 5, 17, 30, pool=3) + ["#ctg\t6\t1,2,3\n"]]
    # rows of whole quads (LW % 4 == 0): the first three tints start at a multiple of four words (16-byte loads), a three-word tint then
    # shifts the two behind it off it (the word-by-word loop at LW % 4 == 0); 4 160 segments: 65 quads, more than a read has lanes
    quads = [tint_lines(rng, 10, 64, 65, pool=6), tint_lines(rng, 11, 128, 64, pool=5), tint_lines(rng, 12, 4160, 8, pool=4),
             tint_lines(rng, 13, 1, 3, pool=2), tint_lines(rng, 14, 64, 40, pool=6), tint_lines(rng, 15, 49, 33, pool=3)]
    return dict(shapes=Batch(d, "shapes", shapes), many=Batch(d, "many", many), big=Batch(d, "big", big), small=Batch(d, "small", small),
                quads=Batch(d, "quads", quads))


# ---- comparisons -----------------------------------------------------------------------------------------------------
def check_groups(groups, b):
    a = b.arrays.a
    assert groups["n_tint"] == len(b.want) and groups["n_reads"] == int(a["read_off"][-1])
    mo = groups["rep_mem_off"]
    for t, (tint, _) in enumerate(b.want):
        reps = tint["read_reps"]
        q0, q1 = int(groups["rep_off"][t]), int(groups["rep_off"][t + 1])
        r0, r1 = int(a["read_off"][t]), int(a["read_off"][t + 1])
        assert q1 - q0 == len(reps), "tint %d: %d reps, expected %d" % (t, q1 - q0, len(reps))
        assert [groups["rep_mem"][int(mo[q]):int(mo[q + 1])].tolist() for q in range(q0, q1)] == reps
        assert groups["rep_first"][q0:q1].tolist() == [m[0] for m in reps]
        rep_of = [None] * (r1 - r0)
        for i, m in enumerate(reps):
            for r in m:
                rep_of[r] = i
        assert groups["read_rep"][r0:r1].tolist() == rep_of
    assert groups["n_reps"] == int(groups["rep_off"][-1]) == len(mo) - 1


def check_partitioned(result, b):
    groups, prep, arr = result
    check_groups(groups, b)
    packed = dict(rep_off=groups["rep_off"], n_seg=b.arrays.a["n_seg"])
    for t, (tint, done) in enumerate(b.want):
        fu.check_prep_against(prep, packed, t, fu.tint_outputs(tint))
    got = cluster_prep.tints_from_arrays(b.arrays, groups, prep, arr, CONSTANT)
    for t, (tint, done) in enumerate(b.want):
        assert cu.canon_partitions(got[t]) == cu.canon_partitions(done), "tint %d" % t
        assert got[t] == done, "tint %d" % t                     # ilp_data (C from the first read), pseudo-gaps, categories on every member
        for members in got[t]["read_reps"]:
            assert all(got[t]["reads"][r]["gaps"] is got[t]["reads"][members[0]]["gaps"] for r in members)
    assert cluster_prep.tints_from_arrays(b.arrays, groups) == [w[0] for w in b.want]


def assert_same(x, y):
    for u, v in zip(x, y):
        assert sorted(u) == sorted(v)
        for k in u:
            assert np.array_equal(u[k], v[k]), k


# ---- tests -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["shapes", "many", "big", "small", "quads"])
def test_groups_and_partitions_match_the_python_side(ctx, batches, name):
    b = batches[name]
    check_groups(ctx.group_reads(b.arrays), b)
    check_partitioned(ctx.partition_segment(b.arrays, SIZE), b)
    t = ctx.group_timing()
    assert t["keys_ms"] > 0 and t["dedupe_ms"] > 0


def test_shapes_cover_what_they_should(batches):
    assert sorted({(len(t["segs"]), len(t["reads"])) for t, _ in batches["shapes"].want}) == sorted((M, n) for M in MS for n in READS)
    assert len(batches["many"].want) == 65 and all(3 <= len(t["reads"]) <= 40 for t, _ in batches["many"].want)
    big = [t for t, _ in batches["big"].want]
    assert [len(t["reads"]) for t in big] == [5000, 500, 200]
    assert len(big[1]["read_reps"]) == 7 and len(big[2]["read_reps"]) == 200 and len(big[0]["read_reps"]) == 9
    q = batches["quads"].arrays.a
    lw = [max((int(M) + 15) // 16, 1) for M in q["n_seg"]]
    assert lw == [4, 8, 260, 1, 4, 4] and [int(o) % 4 for o in q["lab_off"][:6]] == [0, 0, 0, 0, 3, 3]
    n_tok = np.diff(batches["small"].arrays.a["tok_off"])[:18].tolist()
    assert {0, 1, 64, 70} <= set(n_tok)


def test_pairs(ctx, batches):
    """The pairs of pair_lines(): what each single difference must do, by the mirror and by the device."""
    b = batches["small"]
    groups = ctx.group_reads(b.arrays)
    for rep in (b.want[0][0]["read_reps"], None):
        if rep is None:
            q0, q1, mo = int(groups["rep_off"][0]), int(groups["rep_off"][1]), groups["rep_mem_off"]
            rep = [groups["rep_mem"][int(mo[q]):int(mo[q + 1])].tolist() for q in range(q0, q1)]
        of = {r: i for i, m in enumerate(rep) for r in m}
        assert of[0] == of[1] and of[2] == of[3] != of[0] and of[4] != of[2]
        assert of[5] != of[6] and of[7] != of[8] and of[7] != of[9] and of[8] != of[9]
        assert of[10] != of[11] and of[12] not in (of[10], of[11]) and of[13] != of[9]
        assert of[14] != of[0] and of[15] == of[0] and of[16] == of[7] == of[17]
    _, prep, _ = ctx.partition_segment(b.arrays, SIZE)
    M = PAIRS_M
    W = (M + 31) // 32
    c0 = np.unpackbits(prep["c_bits"][:W].view(np.uint8), bitorder="little")[:M].tolist()
    first, last = ROW.index("1"), ROW.rindex("1")
    assert c0 == [1 if (first <= j <= last and ROW[j] == "0") else 0 for j in range(M)]      # the first read's zeros, not the second's 2s


def test_hash_bits_never_decide(ctx, batches, monkeypatch):
    b = batches["big"]
    results = []
    for bits in ("0", "4", None, "0"):
        if bits is None:
            monkeypatch.delenv("FCLU_HASH_BITS", raising=False)
        else:
            monkeypatch.setenv("FCLU_HASH_BITS", bits)
        results.append(ctx.partition_segment(b.arrays, SIZE))
    monkeypatch.delenv("FCLU_HASH_BITS", raising=False)
    check_partitioned(results[0], b)
    for r in results[1:]:
        assert_same(r, results[0])
    monkeypatch.setenv("FCLU_HASH_BITS", "4")
    check_partitioned(ctx.partition_segment(batches["shapes"].arrays, SIZE), batches["shapes"])


def test_replay_on_one_context(batches):
    c = cluster_prep.Context(0)
    try:
        check_partitioned(c.partition_segment(batches["small"].arrays, SIZE), batches["small"])
        check_partitioned(c.partition_segment(batches["big"].arrays, SIZE), batches["big"])        # the buffers grow
        check_groups(c.group_reads(batches["many"].arrays), batches["many"])
        check_partitioned(c.partition_segment(batches["small"].arrays, SIZE), batches["small"])
    finally:
        c.close()


def label_batch(shapes, seed):
    """pack_labels() of random tints of (reps, segments): the tints of test_gpu_cluster_front.lifetime_batch()."""
    return cluster_prep.pack_labels([fu.labels_from_preprocessed(cu.random_tint(seed + k, n, m), seed=k) for k, (n, m) in enumerate(shapes)])


def round_zero(c, b, result):
    """round_setup() + round_models() of every partition's first round, behind partition_segment(b) = result on c.  The inputs are made
    once, from the first result: the caller asserts that every later one equals it."""
    if not hasattr(b, "round_inputs"):
        tints = cluster_prep.tints_from_arrays(b.arrays, *result, CONSTANT)
        b.round_inputs = (cluster_prep.round_gaps(tints), [list(p[0]) for t in tints for p in t["partitions"]])
    gaps, rem = b.round_inputs
    c.round_setup(*gaps)
    return c.round_models(list(range(len(rem))), rem)


@pytest.mark.parametrize("hash_bits", [None, "0"], ids=["default-hash", "one-bucket"])
def test_one_scratch_under_both_dedupes_equals_fresh_contexts(batches, monkeypatch, hash_bits):
    """The grouping and the reps' dedupe share one scratch set, re-grown between them: ONE context through label batches with more reps
    than the segment batch before them had reads, 5 000 reads that grow the scratch under the grouping with 216 reps that reuse it under
    the dedupe, the round models behind that, a refusal in the last read of the last tint and the first batch again gives, call by
    call, every array (and the refusal's text) a fresh context gives for that call alone."""
    if hash_bits is None:
        monkeypatch.delenv("FCLU_HASH_BITS", raising=False)
    else:
        monkeypatch.setenv("FCLU_HASH_BITS", hash_bits)
    small, many, big = batches["small"].arrays, batches["many"].arrays, batches["big"].arrays
    L = label_batch([(130, 64), (65, 33), (1, 5)], 300)
    assert int(L["rep_off"][-1]) > int(small.a["read_off"][-1]) and int(big.a["read_off"][-1]) == 5700
    bad = dict(many.a)
    assert int(bad["read_off"][-1]) > int(bad["read_off"][-2])
    bad["labels"] = np.array(bad["labels"], np.uint32)
    bad["labels"][int(bad["lab_off"][-1]) - max((int(bad["n_seg"][-1]) + 15) // 16, 1)] |= 3       # the last read's first label

    def big_and_round_zero(c):
        result = c.partition_segment(big, SIZE)
        return result + (round_zero(c, batches["big"], result),)

    def refused(c):
        with pytest.raises(cluster_prep.ClusterError) as e:
            c.group_reads(bad)
        return (dict(code=e.value.code, message=str(e.value)),)

    calls = [lambda c: c.partition_segment(small, SIZE), lambda c: c.partition_labels(L, SIZE), lambda c: (c.group_reads(many),),
             lambda c: (c.preprocess(L),), big_and_round_zero, refused, lambda c: c.partition_segment(small, SIZE)]

    def fresh(call):
        c = cluster_prep.Context(0)
        try:
            return call(c)
        finally:
            c.close()

    want = [fresh(call) for call in calls]
    assert "tint 64 read %d: a label with code 3" % (int(np.diff(bad["read_off"])[-1]) - 1) in want[5][0]["message"]
    assert int(want[4][1]["n_reps"]) == 216 and want[4][3]["n_prob"] > 0
    c = cluster_prep.Context(0)
    try:
        for call, w in zip(calls, want):
            got = call(c)
            assert len(got) == len(w)
            assert_same(got, w)
    finally:
        c.close()


def test_files_batch_entry(ctx, batches):
    b = batches["many"]
    arrays, groups, prep, arr = cluster_prep.cluster_files_batch(b.paths, SIZE, ctx, CONSTANT, threads=2)
    check_partitioned((groups, prep, arr), b)
    assert groups["garbage_cost"].tolist() == [3 * len(m) for t, _ in b.want for m in t["read_reps"]]


def segment_dict(rows, M, tok=None, tail=None):
    """fclu_segment arrays of one tint from label rows (lists of 0 / 1 / 2 / 3)."""
    LW = max((M + 15) // 16, 1)
    n = len(rows)
    codes = np.zeros((n, LW * 16), np.uint64)
    for i, r in enumerate(rows):
        codes[i, :len(r)] = r
    labels = (codes << (2 * (np.arange(LW * 16, dtype=np.uint64) % 16))).reshape(n, LW, 16).sum(axis=2).astype(np.uint32).reshape(-1)
    tok = tok or [[] for _ in rows]
    return dict(n_tint=1, read_off=np.array([0, n], np.int64), n_seg=np.array([M], np.int32), lab_off=np.array([0, n * LW], np.int64),
                labels=labels, tok_off=np.cumsum([0] + [len(x) for x in tok]).astype(np.int64),
                tok=np.array([v for x in tok for v in x], np.uint32), tail=np.array(tail or [0] * n, np.uint8))


def test_refusals_leave_the_context_usable(batches):
    c = cluster_prep.Context(0)
    good = [[1, 0, 1, 2, 1] * 4, [1, 2, 1, 0, 1] * 4, [0, 0, 1, 1, 0] * 4]

    def refused(a, code, *words):
        for call in (c.group_reads, lambda x: c.partition_segment(x, SIZE)):
            with pytest.raises(cluster_prep.ClusterError) as e:
                call(a)
            assert e.value.code == code, str(e.value)
            for w in words:
                assert w in str(e.value), str(e.value)
            check_partitioned(c.partition_segment(batches["small"].arrays, SIZE), batches["small"])

    try:
        g = c.group_reads(segment_dict(good, 20, tok=[[5], [5], [5]]))
        assert g["read_rep"].tolist() == [0, 0, 1] and g["rep_first"].tolist() == [0, 2]
        bad = copy.deepcopy(good); bad[2][7] = 3
        refused(segment_dict(bad, 20), 1, "tint 0 read 2", "code 3")
        refused(segment_dict(good, 19), 1, "tint 0 read 0", "beyond")
        refused(segment_dict(good, 20, tail=[0, 3, 0]), 1, "tint 0 read 1", "tail category 3")
        a = segment_dict(good, 20); a["lab_off"] = np.array([0, 7], np.int64); a["labels"] = np.zeros(7, np.uint32)
        refused(a, 1, "tint 0", "lab_off")
        a = segment_dict(good, 20, tok=[[1, 2], [3], []]); a["tok_off"] = np.array([0, 2, 1, 3], np.int64)
        refused(a, 1, "tint 0 read 1", "tok_off")
        a = segment_dict(good, 20); a["read_off"] = np.array([0, -1], np.int64)
        refused(a, 1, "tint 0")
        a = segment_dict(good, 20); a["n_tint"] = 0
        a["read_off"] = a["read_off"][:1]; a["lab_off"] = a["lab_off"][:1]; a["n_seg"] = a["n_seg"][:0]
        refused(a, 1, "empty batch")
        refused(segment_dict([[1] * 9601], 9601), 3, "9601 segments")
        quad = [[1, 0, 2, 1] * 16, [0, 1, 1, 2] * 16, [1, 0, 0, 1] * 16]           # LW = 4, rows at 16-byte offsets: the uint4 loads
        g = c.group_reads(segment_dict(quad, 64))
        assert g["read_rep"].tolist() == [0, 1, 0]
        bad = copy.deepcopy(quad); bad[1][63] = 3
        refused(segment_dict(bad, 64), 1, "tint 0 read 1", "code 3")
        bad = copy.deepcopy(quad); bad[2][17] = 3
        refused(segment_dict(bad, 64), 1, "tint 0 read 2", "code 3")
        refused(segment_dict(quad, 63), 1, "tint 0 read 0", "beyond")
        refused(segment_dict(quad, 49), 1, "tint 0 read 0", "beyond")
    finally:
        c.close()
