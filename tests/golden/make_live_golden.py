#!/usr/bin/env python3
"""Mint the fixtures of tests/test_live_reference.py by running the REFERENCE (imported unmodified by tests/golden/refrun.py) on the
inputs those tests generate.  Only where the reference is installed (the build container); what this writes is data:

  tests/golden/live/<case>.npz   the case's generator and run arguments (JSON), the sha256 of its input TSVs, the reference's
                                 smoothed signal Y, final positions,
                                 the labels of every read rep (first read of the rep) and, for the poly-clip cases, the bytes of its
                                 segment_*.tsv

Usage: python tests/golden/make_live_golden.py
"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "live")
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from freddie_amd import synth  # noqa: E402

CONTIG = "chrS"


def seeded_case(seed):
    """Generator and run arguments drawn from ``seed`` (test_oracle_vs_live_reference)."""
    rng = np.random.default_rng(seed)
    gen = dict(n_reads=int(rng.integers(50, 400)), n_exons=int(rng.integers(5, 120)), rp=float(rng.choice([0, .05, .3])),
               jp=float(rng.choice([0, .3, .8])), jsd=float(rng.choice([2, 6])), max_span=int(rng.choice([0, 6, 14])))
    run = dict(sigma=float(rng.choice([3.0, 5.0, 8.0])), threshold_rate=float(rng.choice([.8, .9, .95])),
               min_read_support_outside=int(rng.choice([0, 3, 10])), max_problem_size=int(rng.choice([20, 50])))
    return gen, run


# name: (tint id = generator index, generator arguments, run arguments, soft clips rewritten with poly-A / poly-T runs)
CASES = {"seed%d" % s: (s,) + seeded_case(s) + (False,) for s in (101, 102, 103)}
CASES["threshold_rate_one"] = (7, dict(n_reads=300, n_exons=60, rp=0.1),
                               dict(sigma=5.0, threshold_rate=1.0, min_read_support_outside=3, max_problem_size=50), False)
CASES["large_problems"] = (5, dict(n_reads=300, n_exons=150, rp=0.3, max_span=0),
                           dict(sigma=5.0, threshold_rate=0.9, min_read_support_outside=3, max_problem_size=100, variance_factor=9.0), False)
for _s in (31, 33):
    CASES["poly_clips%d" % _s] = (_s, dict(n_reads=240, n_exons=30, rp=0.1), {}, True)


def write_inputs(name, d):
    """The case's split / reads TSVs under ``d``/chrS (what the reference reads and the native parser parses)."""
    tid, gen, _, poly = CASES[name]
    synth.generate(tid, write_dir=d, **gen)
    if poly:
        from test_host_native import craft_poly_clips
        craft_poly_clips(d, CONTIG, tid, tid)


def inputs_digest(d):
    """sha256 over the names and bytes of the input TSVs under ``d`` (the fixture records the inputs it was minted from)."""
    h = hashlib.sha256()
    for dp, _, fs in sorted(os.walk(d)):
        for f in sorted(fs):
            with open(os.path.join(dp, f), "rb") as fh:
                h.update(f.encode() + b"\0" + fh.read())
    return h.hexdigest()


def load(name):
    """(generator arguments, run arguments, recorded arrays) of a case; the arguments must be the ones the fixture was minted with."""
    with np.load(os.path.join(OUT, name + ".npz")) as z:
        rec = dict(z)
    tid, gen, run, _ = CASES[name]
    if json.loads(str(rec.pop("args"))) != dict(tid=tid, gen=gen, run=run):
        raise ValueError("tests/golden/live/%s.npz was minted from other arguments: rerun tests/golden/make_live_golden.py" % name)
    return gen, run, rec


def mint(name):
    import refrun
    tid, gen, run, poly = CASES[name]
    with tempfile.TemporaryDirectory() as tmp:
        d, out = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        write_inputs(name, d)
        tint, rec = refrun.run_recorded(d, out, CONTIG, tid, **run)
        arrays = dict(args=np.array(json.dumps(dict(tid=tid, gen=gen, run=run))), inputs_sha256=np.array(inputs_digest(d)),
                      Y=np.concatenate(rec["Y"]).astype(np.float64),
                      final_positions=np.array(tint["final_positions"], np.int32),
                      labels=np.array([tint["reads"][ridxs[0]]["data"] for _, ridxs in tint["read_reps"]], np.uint8))
        if poly:
            with open(os.path.join(out, CONTIG, "segment_%s_%d.tsv" % (CONTIG, tid)), "rb") as f:
                arrays["segment_tsv"] = np.frombuffer(f.read(), np.uint8)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **arrays)
    print("%-20s reps=%d final=%d Y=%d" % (name, len(arrays["labels"]), len(arrays["final_positions"]), len(arrays["Y"])))


if __name__ == "__main__":
    import refrun
    if not refrun.available():
        raise SystemExit("the reference is not installed (%s)" % refrun.REF_PATH)
    os.makedirs(OUT, exist_ok=True)
    for n in CASES:
        mint(n)
