"""The batches of tests/threshold_chain_cases.py under the CPU oracle alone: every named partition holds the count it is named after,
the counts have the chunk, leaf, sweep and flag-group structure they are there for, every count stands before and behind another one
on a workgroup, and state carried over from the partition before -- its leaf table, its values in LDS, or a last LDS value that never
arrived -- would change the threshold's bits.  What tests/test_gpu_threshold_chain.py compares the device with."""
import numpy as np
import pytest

import threshold_cases as tc
import threshold_chain_cases as cc

CHUNK, GRID = cc.CHUNK, cc.GRID


def count_of(name):
    return int(name[2:]) if name.startswith("m-") else None


@pytest.mark.parametrize("kind", cc.KINDS)
def test_counts_are_the_ones_named_and_paired(kind):
    names, parts, params = cc.case(kind)
    assert len(parts) == GRID + 32 and params["ignore_ends"] == (kind == "nan")
    for name, part, o in zip(names, parts, cc.oracles(kind)):
        assert o["error"] == 0, (name, o["errmsg"])
        v, m = tc.values(o), count_of(name)
        if m is None:
            assert 8 <= len(v) <= 128, name                    # filler: one leaf
        else:
            assert len(v) == m and len(part.iv_start) == 1 and (m == 0 or m == int(o["pos_off"][-1])), (name, len(v))
            assert np.isnan(o["threshold"]) == (m == 0), name
        if m is not None and 0 < m <= 2 * CHUNK + 1:           # the plain-Python model the stale variants are built on is the oracle
            assert tc.model_threshold(v, params["variance_factor"]) == o["threshold"], name
    pr = cc.pairs(kind)
    for k, (a, b) in enumerate(pr):                            # the same workgroup: k, then k + GRID
        assert names[k] == "m-%d" % a and names[k + GRID] == "m-%d" % b
    assert [count_of(n) for n in names].count(None) == GRID + 32 - 2 * len(pr)
    counts = set(cc.COUNTS[kind])
    assert {a for a, _ in pr} == {b for _, b in pr} == counts  # every count is walked first and second
    if kind == "ends":
        assert all((a, b) in pr and (b, a) in pr for a, b in zip(cc.COUNTS[kind], cc.COUNTS[kind][1:]))
    else:
        assert all((0, m) in pr and (m, 0) in pr for m in cc.COUNTS[kind][1:])


def test_counts_reach_the_edges_of_the_chain():
    s = {m: cc.structure(m) for m in cc.COUNTS["ends"] + [0]}
    assert s[0]["nch"] == 0 and s[0]["leaves"] == []
    assert [s[m]["leaves"] for m in (2, 7, 8, 9, 128)] == [[2], [7], [8], [9], [128]]          # one leaf: below 8, with and without a tail
    assert s[129]["leaves"] == [64, 65]
    assert len(s[CHUNK - 1]["leaves"]) == 65 and s[CHUNK - 1]["nfull"] == 0                    # the general tree: a second round of 64 leaf slots
    # V ends on a chunk end (and on the last LDS value): no partial chunk, no table; one value more: a chunk of one value, in v
    assert (s[CHUNK]["nfull"], s[CHUNK]["m_last"], s[CHUNK]["in_lds"]) == (1, 0, cc.LDS_VALS)
    assert (s[CHUNK + 1]["nfull"], s[CHUNK + 1]["m_last"], s[CHUNK + 1]["in_lds"]) == (1, 1, cc.LDS_VALS)
    assert s[CHUNK - 1]["in_lds"] == cc.LDS_VALS - 1 == CHUNK - 1
    assert (s[2 * CHUNK]["nfull"], s[2 * CHUNK]["m_last"]) == (2, 0) and (s[2 * CHUNK + 1]["nch"], s[2 * CHUNK + 1]["m_last"]) == (3, 1)
    over = cc.SWEEP_CHUNKS * CHUNK + 1                                                       # one chunk more than a sweep holds: the partial one
    assert (s[over]["nch"], s[over]["sweeps"], s[over]["nfull"]) == (cc.SWEEP_CHUNKS + 1, 2, cc.SWEEP_CHUNKS)
    assert (s[cc.BIG]["nch"], s[cc.BIG]["sweeps"]) == (18, 5) and s[cc.BIG]["nch"] % cc.SWEEP_CHUNKS == 2 and len(s[cc.BIG]["leaves"]) == 8
    assert all(s[m]["sweeps"] == 1 for m in cc.COUNTS["ends"] if 0 < m <= cc.SWEEP_CHUNKS * CHUNK)
    # more flag groups a wave than it keeps words of, wherever the partition starts in the batch; every other partition: kept ones only
    for kind in cc.KINDS:
        names, parts, _ = cc.case(kind)
        start = 0
        for name, o in zip(names, cc.oracles(kind)):
            L = int(o["pos_off"][-1])
            gpw = cc.groups_per_wave(L, start)
            if name == "m-%d" % cc.BIG:
                assert gpw == cc.KEEP_GROUPS + 1 and 7 * gpw < (L + 2047) // 2048, (name, gpw)  # the eighth wave has groups too
            else:
                assert gpw <= cc.KEEP_GROUPS, (name, gpw)
            start += L
    assert cc.case("nan")[0].count("m-%d" % cc.BIG) == 0 and cc.case("ends")[0].count("m-%d" % cc.BIG) == 4


@pytest.mark.parametrize("kind", cc.KINDS)
def test_stale_state_changes_the_threshold(kind):
    names, parts, params = cc.case(kind)
    orc, vf = cc.oracles(kind), params["variance_factor"]
    table = values = last = 0
    for k, (a, b) in enumerate(cc.pairs(kind)):
        va, vb, want = tc.values(orc[k]), tc.values(orc[k + GRID]), orc[k + GRID]["threshold"]
        if b == 0:
            continue
        sa, sb = cc.structure(a), cc.structure(b)
        if sb["m_last"]:
            # with its own table the model is the oracle; with the table of the partition before, where that is another one, it is not
            assert cc.stale_table_threshold(vb, sb["m_last"], vf) == want, (a, b)
            # (a longer table over a chunk that lies in v, not in LDS, adds the zeros of the model: a chunk of one value keeps its bits)
            if sa["m_last"] and sa["m_last"] != sb["m_last"] and (b < cc.LDS_VALS or sa["m_last"] < sb["m_last"]):
                assert cc.stale_table_threshold(vb, sa["m_last"], vf, va) != want, (a, b)
                table += 1
        if a:
            assert cc.stale_values_threshold(vb, va, vf) != want, (a, b)
            assert cc.stale_values_threshold(vb, va, vf, only_last=True) != want, (a, b)
            values += 1
        else:                                                  # behind the empty partition: the values before it are some filler's or none
            assert cc.stale_values_threshold(vb, va, vf, only_last=True) != want, (a, b)
            last += 1
    assert (values, last) == ((26, 0) if kind == "ends" else (0, 11)) and (table >= 10 if kind == "ends" else table == 0)
