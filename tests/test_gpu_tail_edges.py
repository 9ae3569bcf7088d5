"""S6-S7 at their edges, on the device: k_segments' inner-sum test with the deciding counts on and beside the first and last inner
position, at block and tile edges and over more than 64 tiles; k_refine in LDS and in global memory (ties, plateaus, peaks 19 / 20 /
21 apart, radius 50 and 0); k_label_cols / k_label_reads with the column table in LDS and in global memory, every rep-block size,
reads on the columns' edges and across the sentinel, packed and as bytes.  Cases: tests/edge_cases.py; every tap against the CPU
oracle on the first run and on the replay."""
import numpy as np
import pytest

import edge_cases as ec
import util

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("length", ec.INNER_LENS)
def test_inner_sum_on_the_boundary(length):
    ec.run_on_gpu("inner", length, iv_threads=256 if length > 30000 else 64)


@pytest.mark.parametrize("sigma", list(ec.REFINE_SIGMAS))
def test_refinement_in_lds_and_in_global_memory(sigma):
    ec.run_on_gpu("refine", sigma, smooth_r=20 if sigma == "sigma5" else 0, iv_threads=64)


@pytest.mark.parametrize("mode", ["packed", "rate1", "bytes"])
@pytest.mark.parametrize("S", ec.LABEL_COLS)
def test_labels_at_column_table_and_rep_block_edges(S, mode, monkeypatch):
    if mode == "bytes":
        monkeypatch.setenv("FSEG_LABEL_BYTES", "1")
    else:
        monkeypatch.delenv("FSEG_LABEL_BYTES", raising=False)
    rate = 1.0 if mode == "rate1" else 0.9
    labels, packed = ec.run_on_gpu("label", S, rate, label_packed=int(mode == "packed"))
    want = np.concatenate([o["labels"].ravel() for o in ec.oracles("label", S, rate)]) + ord("0")
    assert np.array_equal(labels, want)
    assert np.array_equal(packed, util.pack_labels(want))
