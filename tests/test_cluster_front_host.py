"""The front of the clustering pre-ILP work, CPU side: the plain restatement the GPU tests measure against (tests/front_util.py)
pinned to the fixtures the reference's own source wrote (I, C, FL of preprocess_ilp(), the unique structures of partition_reads()),
and the packers of the device call's input.  No GPU."""
import numpy as np
import pytest

import cluster_util as cu
import front_util as fu
from freddie_amd import cluster_prep
from oracle import cluster_oracle


@pytest.mark.parametrize("name", cu.cluster_names())
def test_restatement_matches_reference_fixtures(name, tmp_path):
    want = cu.load_cluster(name)
    tint = list(cluster_prep.read_segment(cu.segment_tsv_file(name, tmp_path)).values())[0]
    got = fu.tint_outputs(tint)
    assert ["".join(map(str, r)) for r in got["I"]] == want["I"]
    assert ["".join(map(str, r)) for r in got["C"]] == want["C"]
    assert [list(x) for x in got["FL"]] == want["FL"]
    cats = [fu.TAILS[c] for c in got["tail"]]
    assert cats == [want["reads"][m[0]]["poly_tail_category"] for m in want["read_reps"]]
    # node order and members: the reference's unique_data (:203-215) on the host mirror's preprocess_ilp()
    cluster_prep.preprocess_ilp(tint, dict(recycle_model="constant"))
    uniq = cluster_oracle.unique_data_of(tint)
    assert [nd[1] for nd in got["nodes"]] == [u[1] for u in uniq]
    assert [nd[0] for nd in got["nodes"]] == [u[1][0] for u in uniq]
    assert [(tuple(got["I"][nd[0]]), (got["FL"][nd[0]][0], got["FL"][nd[0]][1], cats[nd[0]])) for nd in got["nodes"]] == [u[0] for u in uniq]
    # find_segment_read(): the raw values are the mirror's
    assert got["raw"] == [cluster_prep.find_segment_read(tint["ilp_data"]["I"], i) for i in range(len(tint["read_reps"]))]


def _unpack(words, M):
    return [(int(words[s >> 4]) >> (2 * (s & 15))) & 3 for s in range(M)]


@pytest.mark.parametrize("M", [1, 16, 17, 33])
def test_pack_labels_layout(M):
    import random
    rng = random.Random(M)
    rows = [[rng.randrange(3) for _ in range(M)] for _ in range(5)]
    a = fu.label_tint(1, rows, [0, 1, 2, 0, 1], rng)
    empty = fu.label_tint(2, [], [], rng); empty["segs"] = [(0, 1, 1)] * 7            # a zero-rep tint in the middle
    b = fu.label_tint(3, rows[:2], [2, 0], rng)
    pk = cluster_prep.pack_labels([a, empty, b])
    LW = max((M + 15) // 16, 1)
    assert pk["n_tint"] == 3 and pk["rep_off"].tolist() == [0, 5, 5, 7] and pk["n_seg"].tolist() == [M, 7, M]
    assert pk["lab_off"].tolist() == [0, 5 * LW, 5 * LW, 7 * LW]
    assert pk["labels"].dtype == np.uint32 and pk["labels"].size == 7 * LW
    assert pk["tail"].tolist() == [0, 1, 2, 0, 1, 2, 0]
    for k, row in enumerate(rows + rows[:2]):
        words = pk["labels"][k * LW:(k + 1) * LW]
        assert _unpack(words, M) == row
        assert all(((int(words[s >> 4]) >> (2 * (s & 15))) & 3) == 0 for s in range(M, LW * 16))     # nothing beyond M
    # the little-endian word view of bytes that hold four labels each, first label in the low bits (fseg_results_packed)
    by = pk["labels"][:LW].view(np.uint8)
    assert [(int(by[s >> 2]) >> (2 * (s & 3))) & 3 for s in range(M)] == rows[0]


def test_tail_categories_on_the_five_read_file(tmp_path):
    p = tmp_path / "segment_c_2.tsv"
    p.write_text("#c\t2\t0,10,20,30,40\n"
                 "0\ta\tc\t+\t2\t1201\t0-3:5,SSC:4,\n"
                 "1\tb\tc\t+\t2\t1001\t0-3:9,ESC:7,\n"
                 "2\tc\tc\t+\t2\t1001\t0-3:11,\n"
                 "3\td\tc\t-\t2\t1001\tEA_25:3,ESC:2,\n"
                 "4\te\tc\t-\t2\t1001\tET_30:0,\n")
    tint = cluster_prep.read_segment(str(p))[2]
    assert cluster_prep.tail_categories(tint).tolist() == [0, 0, 2]
    assert cluster_prep.tail_categories(tint).dtype == np.uint8
    got = fu.tint_outputs(tint)
    assert got["FL"] == [(0, 3), (0, 3), (0, 3)] and got["I"][0] == [1, 0, 0, 1]
    assert got["C"] == [[0, 0, 1, 0], [0, 1, 1, 0], [0, 1, 1, 0]]
    # short tails, tails at both ends and a start tail
    for poly, want in ((dict(SA=(10, 1)), 0), (dict(SA=(11, 1)), 1), (dict(ST=(99, 1)), 1), (dict(EA=(11, 0)), 2),
                       (dict(SA=(20, 1), EA=(20, 1)), 0), (dict(), 0)):
        tint["reads"][0]["poly_tail"] = poly
        assert cluster_prep.tail_categories(tint)[0] == want


def test_restatement_on_crafted_rows():
    out = fu.rep_outputs([2, 0, 1, 2, 0, 1, 0, 2], 0, 8)
    assert out["I"] == [0, 0, 1, 0, 0, 1, 0, 0] and out["raw"] == (2, 5) and out["FL"] == (2, 5)
    assert out["C"] == [0, 0, 0, 0, 1, 0, 0, 0]                                  # a 2 inside the span is not a 0
    assert fu.rep_outputs([2, 0, 1, 2, 0, 1, 0, 2], 1, 8)["C"] == [0, 1, 0, 0, 1, 0, 0, 0]
    assert fu.rep_outputs([2, 0, 1, 2, 0, 1, 0, 2], 2, 8)["FL"] == (2, 7)
    z = fu.rep_outputs([0, 0, 2], 0, 3)
    assert z["raw"] == (-1, 2) and z["FL"] == (-1, 2) and z["C"] == [1, 1, 0]     # no 1: every 0 counts (:308-310 with first = -1)
    assert fu.rep_outputs([2, 2], 2, 2) == dict(I=[0, 0], C=[0, 0], raw=(-1, 1), FL=(-1, 1))
    nodes, rep_node = fu.first_occurrence_dedupe([[1, 0], [0, 1], [1, 0], [1, 0], [0, 1]], [(0, 0), (1, 1), (0, 0), (0, 1), (1, 1)], [0, 0, 0, 2, 1])
    assert nodes == [(0, [0, 2]), (1, [1]), (3, [3]), (4, [4])] and rep_node == [0, 1, 0, 2, 3]
