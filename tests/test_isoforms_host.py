"""Isoform-consensus stage (row N4), CPU side: the host mirror's readers and GTF writer plus the oracle's loops must
reproduce the GTF the reference itself wrote for the fixture inputs (tests/golden/make_isoforms_golden.py); the C-ABI
library's symbols; loud failure without a GPU."""
import copy
import os
import re

import numpy as np
import pytest

import isoforms_util as iu
from freddie_amd import build, isoforms
from oracle import isoforms_oracle
from test_host_mirror import input_dir


def oracle_gtf(ctsv, split_tsv, m, w):
    segments, reads, isos = isoforms.read_cluster(ctsv)
    isoforms_oracle.isoforms_cons(isos, segments, reads)
    isoforms.read_split(split_tsv, reads)
    isoforms_oracle.correct_boundaries("starts", isos, reads, m, w)
    isoforms_oracle.correct_boundaries("ends", isos, reads, m, w)
    recs = isoforms.get_gtf_records(isos)
    recs.sort()
    return "".join(r + "\n" for _, r in recs)


@pytest.mark.parametrize("name", iu.names())
def test_oracle_and_host_mirror_reproduce_the_reference_gtf(name, tmp_path):
    doc, ctsv, split_tsv, _, _ = iu.write_case(name, tmp_path, input_dir)
    for m, w in iu.settings():
        assert oracle_gtf(ctsv, split_tsv, m, w) == doc["gtf"]["%g,%d" % (m, w)], (name, m, w)


def test_fixtures_exercise_the_boundary_correction():
    changed = 0
    for name in iu.names():
        g = iu.load(name)["gtf"]
        changed += g["0.5,8"] != g["0.5,0"]
    assert changed >= 3


def test_read_cluster_skips_garbage_and_isoform_lines(tmp_path):
    p = tmp_path / "cluster_c_1.tsv"
    p.write_text("#c\t1\t10,20,30\nisoform_0\t1\t11\n5\tr5\tc\t+\t1\t0\tN\t0\t11\t1\t1\n6\tr6\tc\t+\t1\t0\tS\t*\t10\t1\t0\n")
    segments, reads, isos = isoforms.read_cluster(str(p))
    assert segments == {("c", 1): [(10, 20), (20, 30)]} and list(reads) == [5]
    assert isos == {("c", 1, 0, 0): dict(rids={5})}
    p.write_text("#c\t1\t10,20,30\n5\tr5\tc\t+\t1\t0\tN\t0\t1\t1\n")
    with pytest.raises(AssertionError):                    # label string shorter than the segment list (:192-193)
        isoforms.read_cluster(str(p))


def test_isoforms_library_exports_every_declared_symbol():
    text = open(os.path.join(build.INCLUDE, "freddie_isoforms.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(fiso_[a-z_]+)\s*\(", text)))
    assert declared == sorted(isoforms.EXPORTS)
    L = isoforms.load()
    for name in declared:
        assert hasattr(L, name)
    assert L.fiso_abi_version() == 1


def test_isoforms_fails_loudly_without_a_gpu():
    import torch
    if torch.cuda.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(isoforms.IsoformsError, match="no CPU fallback"):
        isoforms.Context(0)


# ---- the plain numpy references of the GPU tests (isoforms_util.plain_counts / plain_votes) against the oracle's loops ----------
_JOBS = [(1, 12, 30, 40), (2, 3, 200, 70), (3, 40, 4, 9), (4, 2, 3, 1), (5, 6, 25, 17)]


def _job_arrays(isos, segments, reads):
    """A job as isoforms_cons_batch() lays it out: rows one after another, in the order of the isoforms and their sorted reads."""
    iro, n_seg, off, lab, tail = [0], [], [], [], []
    for key, isoform in isos.items():
        M = len(segments[(key[0], key[1])])
        for rid in sorted(isoform["rids"]):
            off.append(sum(len(x) for x in lab)); lab.append(reads[rid]["data"]); tail.append("NSE".index(reads[rid]["tail"]))
        iro.append(len(lab)); n_seg.append(M)
    return (np.asarray(iro), np.asarray(n_seg), np.asarray(off), np.frombuffer("".join(lab).encode(), np.uint8),
            np.asarray(tail, np.uint8))


@pytest.mark.parametrize("job", _JOBS)
def test_plain_counts_are_the_oracles_counts(job):
    isos, segments, reads = iu.random_job(*job)
    iro, n_seg, off, lab, tail = _job_arrays(isos, segments, reads)
    cons, cov, tails = iu.plain_counts(iro, n_seg, off, lab, tail)
    seg_off = np.concatenate([[0], np.cumsum(n_seg)])
    want = copy.deepcopy(isos)
    isoforms_oracle.isoforms_cons(want, segments, reads)
    assert any("starts" in v for v in want.values())
    for i, (key, isoform) in enumerate(isos.items()):
        M = int(n_seg[i])
        x, c, t = [0] * M, [0] * M, {"N": 0, "S": 0, "E": 0}       # accumulated as isoforms_oracle.isoforms_cons does
        for rid in isoform["rids"]:
            read = reads[rid]
            if "1" not in read["data"]:
                continue
            first, last = (0, M - 1) if read["tail"] == "S" else (read["data"].index("1"), M - 1 - read["data"][::-1].index("1"))
            for j in range(first, last + 1):
                x[j] += read["data"][j] == "1"
                c[j] += 1
            t[read["tail"]] += 1
        assert cons[seg_off[i]:seg_off[i + 1]].tolist() == x, key
        assert cov[seg_off[i]:seg_off[i + 1]].tolist() == c, key
        assert tails[i].tolist() == [t["N"], t["S"], t["E"]], key
        # and the oracle's own decisions follow from these counts
        flags = [a / b > 0.5 if a >= 3 else False for a, b in zip(x, c)]
        assert (True in flags) == ("starts" in want[key])
        if True in flags:
            assert want[key]["strand"] == ("-" if tails[i][1] > tails[i][2] else "+")
            segs = segments[(key[0], key[1])]
            assert want[key]["starts"] == [segs[j][0] for j in range(M) if flags[j] and (j == 0 or not flags[j - 1])]
            assert want[key]["ends"] == [segs[j][1] for j in range(M) if flags[j] and (j == M - 1 or not flags[j + 1])]


@pytest.mark.parametrize("job", _JOBS)
@pytest.mark.parametrize("w", [1, 8, 20])
def test_plain_votes_are_the_oracles_cur_dicts(job, w):
    isos, segments, reads = iu.random_job(*job)
    isoforms_oracle.isoforms_cons(isos, segments, reads)
    total = 0
    for side in ("starts", "ends"):
        with_side = [v for v in isos.values() if side in v]
        iro, ibo, ib, rbo, rb = [0], [0], [], [0], []
        for isoform in with_side:
            for rid in sorted(isoform["rids"]):
                rb.extend(reads[rid][side]); rbo.append(len(rb))
            ib.extend(isoform[side]); iro.append(len(rbo) - 1); ibo.append(len(ib))
        votes = iu.plain_votes(iro, ibo, ib, rbo, rb, w)
        assert votes.shape == (len(ib), 2 * w + 1) and votes.dtype == np.int32
        for i, isoform in enumerate(with_side):
            for idx, iso_s in enumerate(isoform[side]):
                cur = {x: 0 for x in range(-w, w + 1)}               # as isoforms_oracle.correct_boundaries builds it
                for rid in isoform["rids"]:
                    for read_s in reads[rid][side]:
                        x = read_s - iso_s
                        if x in cur:
                            cur[x] += 1
                assert votes[ibo[i] + idx].tolist() == [cur[x] for x in range(-w, w + 1)]
        total += int(votes.sum())
        # the oracle's corrected boundaries follow from these votes (the largest offset with a majority wins)
        for m in (0.5, 0.8):
            want = copy.deepcopy(isos)
            isoforms_oracle.correct_boundaries(side, want, reads, m, w)
            for i, (key, isoform) in enumerate((k, v) for k, v in isos.items() if side in v):
                moved = list(isoform[side])
                for idx in range(len(moved)):
                    for k, v in enumerate(votes[ibo[i] + idx].tolist()):
                        if v / len(isoform["rids"]) >= m:
                            moved[idx] = isoform[side][idx] + k - w
                assert want[key][side] == moved
    assert total > 0
