"""tests/label_cases.py on the CPU: every batch reaches the edge it is named after, shown with the oracle alone -- the reps of every
partition against the unit and the block, the exons of a unit against kLabelExons, the column tables against kLabelStage, which of
k_label_reads' four label_rep instances a batch's units take, where a unit's first exon sits in the exon arrays, and the geometry of exons
against columns that the merge has to get right."""
import numpy as np
import pytest

import label_cases as lc
from freddie_amd import tables


def unique_parts(name):
    names, parts, _ = lc.batch(name)
    seen, out = set(), []
    for n, p, o in zip(names, parts, lc.oracles(name)):
        if id(p) not in seen:
            seen.add(id(p)); out.append((n, p, o))
    return out


def columns(o):
    """(fp, sentinel mask) of a partition: column c is [fp[c], fp[c+1]); the last final position of an interval starts a sentinel."""
    fp = np.asarray(o["final_pos"], np.int64)
    sent = np.zeros(len(fp) - 1, bool)
    sent[np.asarray(o["final_off"][1:-1], np.int64) - 1] = True
    return fp, sent


def reps(p):
    off = np.asarray(p.rep_exon_off, np.int64)
    return [(p.ex_ts[a:b].astype(np.int64), p.ex_te[a:b].astype(np.int64)) for a, b in zip(off[:-1], off[1:])]


@pytest.mark.parametrize("name", list(lc.BATCHES))
def test_the_oracle_accepts_every_partition(name):
    for n, p, o in unique_parts(name):
        assert o["error"] == 0, (n, o["errmsg"])
        assert o["labels"].shape == (p.n_reps, len(o["final_pos"]) - 1)
        assert (o["labels"] != 0).any(), n                           # some label is written, not only the arena's fill


def test_rep_counts_sit_on_the_unit_and_block_edges():
    names, parts, _ = lc.batch("main")
    got = {n: p.n_reps for n, p in zip(names, parts) if n.startswith("reps-")}
    assert got == {"reps-%d" % n: n for n in lc.REP_COUNTS}
    assert {lc.UNIT - 1, lc.UNIT, lc.UNIT + 1, lc.BLOCK - 1, lc.BLOCK, lc.BLOCK + 1, 1} == set(lc.REP_COUNTS)
    rows = lc.units("main")
    # a partial last unit of 1 and of 63 reps, whole units, a second block of one rep
    assert {1, lc.UNIT - 1, lc.UNIT} <= {r[1] for r in rows}
    assert sum(r[0] == names.index("reps-257") for r in rows) == 5


@pytest.mark.parametrize("name", ["main", "bytes", "flat"])
def test_units_sit_on_the_exon_stage(name):
    rows = lc.units(name)
    n_ex = [r[3] for r in rows]
    assert {lc.LABEL_EXONS - 1, lc.LABEL_EXONS, lc.LABEL_EXONS + 1} <= set(n_ex)          # ... in one launch
    for r in rows:
        assert r[6] == (r[3] <= lc.LABEL_EXONS)
    # staged and unstaged units follow each other inside one partition, and a short last unit follows an unstaged one
    seq = [(r[0], r[6]) for r in rows]
    assert any(a[0] == b[0] and a[1] and not b[1] for a, b in zip(seq, seq[1:]))
    assert any(a[0] == b[0] and not a[1] and b[1] for a, b in zip(seq, seq[1:]))


def test_all_four_instances_run():
    for name in ("main", "bytes"):
        assert {(r[5], r[6]) for r in lc.units(name)} == {(True, True), (True, False), (False, True), (False, False)}, name
    by_S = {}
    for name in lc.BATCHES:
        for r in lc.units(name):
            by_S.setdefault(r[4], set()).add(r[6])
    # S = 1, kLabelStage and kLabelStage + 1, each with staged and with unstaged exons
    for S in (1, lc.LABEL_STAGE, lc.LABEL_STAGE + 1):
        assert by_S[S] == {True, False}, S
    assert all(r[5] == (r[4] <= lc.LABEL_STAGE) for name in lc.BATCHES for r in lc.units(name))


def test_first_exons_at_every_residue():
    rows = lc.units("main")
    for n_ex in (lc.LABEL_EXONS - 1, lc.LABEL_EXONS, lc.LABEL_EXONS + 1):
        assert {r[2] % 4 for r in rows if r[3] == n_ex} == {0, 1, 2, 3}, n_ex
    names, parts, _ = lc.batch("main")
    assert all(int(p.rep_exon_off[-1]) == 1 for n, p in zip(names, parts) if n.startswith("pad-"))


def test_geometry_of_exons_against_columns():
    seen = set()
    for n, p, o in unique_parts("main"):
        fp, sent = columns(o)
        S = len(fp) - 1
        cols = np.flatnonzero(~sent)
        starts, ends = set(fp[cols].tolist()), set(fp[cols + 1].tolist())
        n_iv = len(o["final_off"]) - 1
        for ts, te in reps(p):
            k = len(ts)
            seen.add("exons-%d" % k)
            if set((te + 1).tolist()) & starts: seen.add("ends on fp[c] - 1")
            if set(te.tolist()) & starts: seen.add("ends on fp[c]")
            if set((ts + 1).tolist()) & ends: seen.add("starts on fp[c+1] - 1")
            if set(ts.tolist()) & ends: seen.add("starts on fp[c+1]")
            if int(ts[0]) in starts: seen.add("read starts on a column's edge")
            if n_iv == 2 and ts[0] < fp[o["final_off"][1] - 1] and te[-1] >= fp[o["final_off"][1]]: seen.add("across the sentinel")
            # exons that overlap each column
            c0 = np.searchsorted(fp, ts, "right") - 1
            c1 = np.searchsorted(fp, te, "right") - 1
            hit = np.zeros(S + 1, np.int64)
            for a, b in zip(c0, c1):
                hit[max(a, 0):min(b, S - 1) + 1] += 1
            if (hit[:S][~sent] >= 3).any(): seen.add("three exons in one column")
            if (hit[:S][~sent] >= 2).any(): seen.add("two exons in one column")
    want = {"exons-1", "exons-14", "ends on fp[c] - 1", "ends on fp[c]", "starts on fp[c+1] - 1", "starts on fp[c+1]",
            "read starts on a column's edge", "across the sentinel", "two exons in one column"}
    assert want <= seen, want - seen
    # the one-column partitions: every exon of a rep lies in the same column
    for n, p, o in unique_parts("flat"):
        if n.startswith("S1"):
            assert len(o["final_pos"]) == 2 and max(len(ts) for ts, _ in reps(p)) >= (15 if n == "S1-exons" else 1)


def test_byte_label_batch_mixes_default_2_and_default_0():
    names, parts, params = lc.batch("bytes")
    assert np.asarray(tables.smooth_threshold(params["threshold_rate"]))[-1] == 1.0 and params["threshold_rate"] < 1.0
    assert np.asarray(tables.smooth_threshold(lc.batch("main")[2]["threshold_rate"])).max() < 1.0
    for n, p, o in zip(names, parts, lc.oracles("bytes")):
        fp, sent = columns(o)
        wide = np.flatnonzero((np.diff(fp) == 106) & ~sent)          # a segment of exactly 107 positions
        assert (len(wide) > 0) == n.startswith("has2"), n
        if len(wide):
            c = int(wide[0])
            away = [i for i, (ts, te) in enumerate(reps(p)) if te[-1] < fp[c] or ts[0] >= fp[c + 1]]
            assert away and (o["labels"][away, c] == 2).all()       # a read without coverage there is '2'
    assert [n.startswith("has2") for n in names] == [True, False, True, False, True, True, False]
