"""Clustering pre-ILP, CPU side of the partition arrays: the member layout Context.partition() takes.  No GPU."""
import numpy as np

import cluster_util as cu
from freddie_amd import cluster_prep


def test_pack_members_layout():
    a = [((1, 0), (0, 0, "N")), ((0, 1), (1, 1, "N"))]
    uniq = [[(a[0], [4, 9, 2]), (a[1], [7])], [], [(a[0], [0]), (a[1], [3, 1])]]
    pm = cluster_prep.pack_members(uniq)
    assert pm["mem_off"].dtype == np.int64 and pm["mem"].dtype == np.int32
    assert pm["mem_off"].tolist() == [0, 3, 4, 5, 7]
    assert pm["mem"].tolist() == [4, 9, 2, 7, 0, 3, 1]               # rows in pack_structures() order, members as given
    assert cluster_prep.pack_structures(uniq)["row_off"].tolist() == [0, 2, 2, 4]
    empty = cluster_prep.pack_members([[], []])
    assert empty["mem_off"].tolist() == [0] and empty["mem"].size == 0


def test_pack_members_of_a_tint_with_duplicate_structures():
    tint = cu.random_tint(200, 150, 20, n_isoforms=2, noise=0.0, tail_p=0.0)
    uniq = cluster_prep.unique_structures(tint)
    assert len(uniq) < 150                                             # reps do share structures here
    pm = cluster_prep.pack_members([uniq])
    assert pm["mem_off"][-1] == 150 and sorted(pm["mem"].tolist()) == list(range(150))
    for r, (_, members) in enumerate(uniq):
        assert pm["mem"][pm["mem_off"][r]:pm["mem_off"][r + 1]].tolist() == members


def test_exports_name_the_partition_calls():
    for name in ("fclu_partition", "fclu_partition_adj", "fclu_partition_results", "fclu_partition_timing"):
        assert name in cluster_prep.EXPORTS
