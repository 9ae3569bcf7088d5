#!/usr/bin/env python3
"""Mint the fixtures of the segmentation-visualisation script by running the REFERENCE's py/freddie_segment_vis.py, unmodified,
as a child process (it needs only numpy).

Inputs:
  s_<golden>  the segment TSV stored in tests/golden/<golden>.npz, the split TSV the golden was minted from (regenerated
              from its seed, or the committed edge case: test_host_mirror.input_dir()) and a GTF crafted around its
              boundaries (vis_util.gtf_around());
  c_* / x_*   the crafted cases of vis_util.cases() (small coordinates: the reference walks range(0, first boundary) for
              every object it flags on the first segment).
Stored per case in tests/golden/vis/<case>.json.gz: the inputs (texts; for s_* the golden's name and the split's sha256
instead of the split and segment texts), the reference's stdout, exit status and exception class, its pickle as
type-tagged JSON (vis_util.typed()), the pickle's sha256 and pickle.DEFAULT_PROTOCOL of the interpreter that ran it.
Build container only.   Usage: python tests/golden/make_vis_golden.py
"""
import gzip
import hashlib
import json
import os
import pickle
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import vis_util  # noqa: E402

REFERENCE = "/root/reference/py/freddie_segment_vis.py"


def run_reference(case, work):
    paths = vis_util.write_inputs(case, work)
    out = os.path.join(work, "out.pickle")
    if os.path.exists(out):
        os.remove(out)
    r = subprocess.run([sys.executable, REFERENCE, "-s", paths["split"], "-g", paths["segment"], "-a", paths["gtf"], "-o", out],
                       capture_output=True, text=True, cwd=work, timeout=600)
    doc = dict(stdout=r.stdout, returncode=r.returncode, protocol=pickle.DEFAULT_PROTOCOL,
               exception=r.stderr.strip().splitlines()[-1].split(":")[0] if r.returncode else None)
    if os.path.exists(out):
        blob = open(out, "rb").read()
        doc["pickle_sha256"] = hashlib.sha256(blob).hexdigest()
        doc["pickle"] = vis_util.typed(pickle.loads(blob))
    else:
        doc["pickle_sha256"] = doc["pickle"] = None
    return doc


def main():
    out_dir = vis_util.VIS_DIR
    os.makedirs(out_dir, exist_ok=True)
    index = {}
    with tempfile.TemporaryDirectory() as work:
        jobs = []
        for name in vis_util.GOLDEN_SOURCES:
            case = vis_util.golden_case(name, os.path.join(work, "in"))
            stored = dict(source=name, gtf=case["gtf"], split_sha256=hashlib.sha256(case["split"].encode()).hexdigest())
            jobs.append(("s_" + name, case, stored))
        for name, case in sorted(vis_util.cases().items()):
            jobs.append((name, case, dict(case)))
        for name, case, stored in jobs:
            doc = dict(stored, **run_reference(case, work))
            with gzip.GzipFile(os.path.join(out_dir, name + ".json.gz"), "wb", mtime=0) as fz:
                fz.write(json.dumps(doc, sort_keys=True).encode())
            index[name] = dict(returncode=doc["returncode"], exception=doc["exception"], stdout_lines=doc["stdout"].count("\n"),
                               pickle_sha256=doc["pickle_sha256"])
            print(name, index[name])
    json.dump(dict(reference="vpc-ccg/freddie py/freddie_segment_vis.py, run unmodified as a child process",
                   protocol=pickle.DEFAULT_PROTOCOL, cases=index),
              open(os.path.join(out_dir, "INDEX.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
