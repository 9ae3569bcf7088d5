"""bench.py --dump-outputs without a GPU: the files written from a job's results do not depend on how the job is cut into batches,
and the label sample decodes the two-bit labels of Context.results(packed=True).  The oracle stands in for the library."""
import os
import sys

import numpy as np

import util
from freddie_amd import pack, synth

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def oracle_results(n_part=5):
    w = dict(synth.WORKLOADS["config3"], n_reads=200)
    w.pop("n_partitions")
    outs = []
    for i in range(n_part):
        g = synth.generate(i, with_seq=False, **w)
        part = pack.pack_partition(g.iv_start, g.iv_end, g.read_exon_off, g.ex_ts, g.ex_te, dedupe=True)
        o = util.run_oracle(part, dict(bench.PARAMS["default"]))
        assert o["error"] == 0, o["errmsg"]
        outs.append((o["final_pos"], np.asarray(o["labels"], np.uint8).ravel()))
    return outs


def batch_results(outs, ids):
    """A batch of partitions ``ids`` as Context.results(packed=True) returns it."""
    fps, labs = [outs[i][0] for i in ids], [outs[i][1] for i in ids]
    pfo = np.concatenate([[0], np.cumsum([len(f) for f in fps])]).astype(np.int64)
    lo = np.concatenate([[0], np.cumsum([len(x) for x in labs])]).astype(np.int64)
    packed = util.pack_labels(np.concatenate(labs) + ord("0"))
    return pfo, np.concatenate(fps).astype(np.int32), lo, packed


def test_dump_does_not_depend_on_the_batches(tmp_path):
    outs = oracle_results()
    got = {}
    for name, groups in (("one", [[0, 1, 2, 3, 4]]), ("three", [[0, 1], [2], [3, 4]])):
        d = str(tmp_path / name)
        bench.write_outputs(d, "", [bench.dump_batch(g, batch_results(outs, g), 300) for g in groups])
        got[name] = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert sorted(got["one"]) == ["final_pos", "final_pos_offsets", "label_offsets", "label_sample", "label_sample_index"]
    for k, a in got["one"].items():
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, got["three"][k]), k
    a = got["one"]
    assert np.array_equal(a["final_pos"], np.concatenate([fp for fp, _ in outs]))
    assert np.array_equal(a["final_pos_offsets"], np.concatenate([[0], np.cumsum([len(fp) for fp, _ in outs])]))
    labels = np.concatenate([lab for _, lab in outs])
    assert a["label_offsets"][-1] == len(labels) and len(a["label_sample"]) == 5 * 300
    assert np.array_equal(a["label_sample"], labels[a["label_sample_index"].astype(np.int64)])
