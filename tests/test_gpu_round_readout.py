"""The round read-out on the GPU (fclu_round_readout) against the numpy mirror (cluster_prep.readout_mirror) and the definition
(cluster.read_out), byte for byte: segment counts at the ends of a label word and of a bit word and the widest row, tints of different M
in one batch (rows that start at multiples of 16 and elsewhere; both store paths in the census), single members, all columns, column 0 a
member and not, sets beyond column 63, an empty set between two, every set empty, the hand-built rows, a second round on one context;
the refusals, each followed by a good call; the resident models against the fetched ones through incumbents, exact and branch and bound;
and the loop on files with device_rounds on and off."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest

import cluster_util as cu
import round_util as ru
from freddie_amd import cluster, cluster_prep, cluster_solve
from test_gpu_incumbents import grid_tints
from test_gpu_round_models import all_problems, stage

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import readout_host_check as rc  # noqa: E402

pytestmark = pytest.mark.gpu

SETTINGS = cluster.ilp_settings()
KEYS = ("exon_off", "exons", "mem_off", "corr_off", "corr", "e_off", "e")


@pytest.fixture(scope="module")
def ctx():
    c = cluster_prep.Context(0)
    yield c
    c.close()


@pytest.fixture
def shapes(ctx):
    """The shapes, staged on the context: (tints, part0)."""
    tints = rc.shape_tints()
    return tints, stage(ctx, tints)


def unpack(arr, p, M):
    words = arr["inf_bits"][int(arr["inf_bits_off"][p]):int(arr["inf_bits_off"][p + 1])]
    return [(int(words[j >> 5]) >> (j & 31)) & 1 for j in range(M)]


def readout(ctx, tints, part0, problems, sets, fetch=True, definition=True):
    """One round and its read-out on the device, compared with the mirror on the device's own informative rows (which are
    informative_segs()') and, problem by problem, with cluster.read_out().  A refused problem gets no set.  Returns (arr, out, sets)."""
    arr = ctx.round_models([part0[t] + q for t, q, _ in problems], [rem for _, _, rem in problems], fetch=fetch)
    sets = [[] if arr["refused"][p] >= 0 else list(s) for p, s in enumerate(sets)]
    out = ctx.round_readout(sets)
    informative = [unpack(arr, p, len(tints[t]["segs"])) for p, (t, _, _) in enumerate(problems)]
    want = cluster_prep.readout_mirror(tints, [(t, rem) for t, _, rem in problems], sets, informative)
    for key in KEYS:
        assert np.array_equal(out[key], want[key]), key
    assert (out["n_sets"], out["n_mem"]) == (want["n_sets"], want["n_mem"]) == (sum(1 for s in sets if s), sum(len(s) for s in sets))
    for p, (t, _, rem) in enumerate(problems):
        got = cluster_prep.readout_isoform(out, p, rem)
        assert (got is None) == (not sets[p])
        if got is None or not definition:
            continue
        assert informative[p] == [int(v) for v in ru.informative_segs(tints[t], rem)]
        inf_seg = [j for j, v in enumerate(informative[p]) if v]
        I = tints[t]["ilp_data"]["I"]
        e = [int(any(I[rem[c]][j] for c in sets[p])) for j in inf_seg]
        x = [int(c in set(sets[p])) for c in range(len(rem))]
        assert got == (cluster.read_out(tints[t], rem, dict(inf_seg=inf_seg), x, e), e), p
    paths = ctx.readout_paths()
    assert (paths["sets"], paths["members"]) == (out["n_sets"], out["n_mem"])
    return arr, out, sets


def variant_problems(tints, name):
    problems, sets = [], []
    for t, tint in enumerate(tints):
        for q, (rids, _) in enumerate(tint["partitions"]):
            rem, members = rc.set_variant(name, rids)
            problems.append((t, q, rem))
            sets.append(members)
    return problems, sets


@pytest.mark.parametrize("fetch", [True, False], ids=["fetched", "resident"])
@pytest.mark.parametrize("name", rc.VARIANTS)
def test_shapes_in_one_batch(ctx, shapes, name, fetch):
    """Every partition of every shape in ONE call under one set variant: M = 1 .. 130 and 9 600, 300 columns, the hand-built rows."""
    tints, part0 = shapes
    problems, sets = variant_problems(tints, name)
    arr, out, sets = readout(ctx, tints, part0, problems, sets, fetch)
    assert set(len(t["segs"]) for t in tints) >= set(rc.SEGMENTS) | {rc.WIDEST}
    sizes = [len(rem) for _, _, rem in problems]
    assert max(sizes) == 300 and any(len(tints[t]["segs"]) == rc.WIDEST and len(rem) == 3 for t, _, rem in problems)
    paths = ctx.readout_paths()
    timing = ctx.round_readout_timing()
    if name == "empty":
        assert out["n_sets"] == 0 and all(out[k].size == 0 for k in ("exons", "corr", "e")) and not paths["wide_stores"] and not paths["byte_stores"]
        assert not out["exon_off"].any() and not out["corr_off"].any() and not out["e_off"].any()
        return
    assert paths["byte_stores"]
    assert 0 < timing["exons_ms"] < 50 and 0 < timing["corr_ms"] < 50      # (a launch stays far under what one may take)
    big = sizes.index(300)
    if name == "from_64":
        assert sets[big] == list(range(63, 300))
    if name == "without_0":
        assert sets[big] and 0 not in sets[big] and sum(1 for s, n in zip(sets, sizes) if n >= 2 and s and 0 not in s) > 3
    if name == "all":
        assert sets[big] == list(range(300))
    if name == "odd_reversed":
        assert any(not s for s in sets) and any(s for s in sets)


def same_rows(tid, M, n):
    """n reps of one I row (one node, so one partition), told apart by 0 -> 2 swaps."""
    row = [0 if j % 3 == 1 else 1 for j in range(M)]
    return ru.make_tint(tid, [[2 if v == 0 and (i + j) % 2 else v for j, v in enumerate(row)] for i in range(n)])


def test_rows_at_and_off_multiples_of_16(ctx):
    """Members' rows of 16, 32, 17 and 64 bytes behind one another: the rows of the first two start at multiples of 16 and are stored 16
    bytes at a time; the second 17-byte row and the 64-byte rows start elsewhere and go byte by byte, as does the 17th byte.  Then a batch
    that takes the wide path alone, and one that takes the byte path alone."""
    for shape, wide, single in (([(16, 4), (32, 3), (17, 2), (64, 2)], True, True), ([(16, 3), (32, 2), (64, 1)], True, False), ([(15, 5), (1, 2)], False, True)):
        tints = [same_rows(t, M, n) for t, (M, n) in enumerate(shape)]
        part0 = stage(ctx, tints)
        assert [len(t["partitions"]) for t in tints] == [1] * len(shape)
        problems = all_problems(tints, lambda t, q, rids: rids)
        for fetch in (True, False):
            arr, out, sets = readout(ctx, tints, part0, problems, [list(range(n)) for _, n in shape], fetch)
            paths = ctx.readout_paths()
            assert (paths["wide_stores"], paths["byte_stores"]) == (wide, single)
            assert out["corr_off"].tolist() == np.cumsum([0] + [M * n for M, n in shape]).tolist()


def test_the_hand_built_rows_hold_what_they_name(ctx, shapes):
    """In the batch above: a label 2 on an informative and on an uninformative segment, a C bit under an exon bit 0 and under 1, C cut by
    FL behind both tails, a problem whose segments are all informative and one where no interior segment is."""
    tints, part0 = shapes
    problems, sets = variant_problems(tints, "all")
    arr, out, sets = readout(ctx, tints, part0, problems, sets)
    seen = set()
    for p, (t, _, rem) in enumerate(problems):
        iso = cluster_prep.readout_isoform(out, p, rem)
        if iso is None:
            continue
        inf = unpack(arr, p, len(tints[t]["segs"]))
        M = len(inf)
        if all(inf):
            seen.add("all informative")
        if M > 2 and not any(inf[1:-1]) and inf[0] and inf[-1]:
            seen.add("no interior segment informative")
        C = tints[t]["ilp_data"]["C"]
        for rid, corr in iso[0]["rid_to_corrections"].items():
            data = tints[t]["reads"][tints[t]["read_reps"][rid][0]]["data"]
            for j in range(M):
                if data[j] == 2:
                    seen.add("2 informative" if inf[j] else "2 uninformative")
                    assert corr[j] == ("2" if inf[j] else "-")
                if C[rid][j] and inf[j]:
                    seen.add("C with exon %d" % iso[0]["exons"][j])
                    assert corr[j] == ("X" if iso[0]["exons"][j] else "0")
            first = tints[t]["ilp_data"]["FL"][rid]
            if first[0] == 0 and data[0] != 1:
                seen.add("start tail")
            if first[1] == M - 1 and data[M - 1] != 1 and any(v == 1 for v in data):
                seen.add("end tail")
    assert seen >= {"all informative", "no interior segment informative", "2 informative", "2 uninformative", "C with exon 0", "C with exon 1",
                    "start tail", "end tail"}, seen


def test_column_0_not_a_member_gives_the_uninformative_values(ctx, shapes):
    """Column 0 alone outside the set: off the informative segments the exon row is column 0's I row, a non-member's."""
    tints, part0 = shapes
    problems, sets = variant_problems(tints, "without_0")
    arr, out, sets = readout(ctx, tints, part0, problems, sets)
    checked = 0
    for p, (t, _, rem) in enumerate(problems):
        iso = cluster_prep.readout_isoform(out, p, rem)
        if iso is None:
            continue
        inf = unpack(arr, p, len(tints[t]["segs"]))
        row = tints[t]["ilp_data"]["I"][rem[0]]
        assert rem[0] not in iso[0]["rid_to_corrections"]
        assert [v for v, on in zip(iso[0]["exons"], inf) if not on] == [v for v, on in zip(row, inf) if not on]
        checked += sum(1 for on in inf if not on)
    assert checked > 100


def test_an_empty_set_between_two_and_a_second_round(ctx, shapes):
    tints, part0 = shapes
    problems = all_problems(tints, lambda t, q, rids: rids)
    sets = [[] if p % 3 == 1 else list(range(len(rem))) for p, (_, _, rem) in enumerate(problems)]
    arr, out, sets = readout(ctx, tints, part0, problems, sets, fetch=False)
    lens = [int(out["exon_off"][p + 1] - out["exon_off"][p]) for p in range(len(problems))]
    assert any(lens[p - 1] and not lens[p] and lens[p + 1] for p in range(1, len(problems) - 1))
    fewer = all_problems(tints, lambda t, q, rids: rids[1::2][::-1])        # the next round: fewer reps, another order
    fewer = [(t, q, rem) for t, q, rem in fewer if rem]
    sets = [list(range(0, len(rem), 2)) for _, _, rem in fewer]
    readout(ctx, tints, part0, fewer, sets, fetch=False)
    readout(ctx, tints, part0, fewer, [[len(rem) - 1] for _, _, rem in fewer], fetch=True)


def test_sets_beyond_column_63(ctx, shapes):
    """The 300-column problem: column 63 a member, column 299 a member, a set of the columns 64 and above alone."""
    tints, part0 = shapes
    t = max(range(len(tints)), key=lambda k: len(tints[k]["read_reps"]))
    assert len(tints[t]["partitions"]) == 1 and len(tints[t]["partitions"][0][0]) == 300
    rem = list(tints[t]["partitions"][0][0])
    for members in ([63], [299], list(range(64, 300)), [0, 63, 64, 299], list(range(0, 300, 7))):
        arr, out, _ = readout(ctx, tints, part0, [(t, 0, rem)], [members])
        assert out["n_mem"] == len(members)


def test_resident_models_serve_the_later_calls(ctx):
    """The grid batch: behind round_models(fetch=False) the incumbents, the exact call and the branch and bound give what they give
    behind fetch=True; fclu_round_results names the small arrays alone and round_model() refuses."""
    tints = grid_tints()
    part0 = stage(ctx, tints, maximum_ilp_size=3)
    problems = all_problems(tints, lambda t, q, rids: rids[::-1] if t % 3 == 0 else rids)
    garbage = [g for t, _, rem in problems for g in ru.garbage_costs(tints[t], rem, "constant")]
    got = {}
    for fetch in (True, False):
        arr = ctx.round_models([part0[t] + q for t, q, _ in problems], [rem for _, _, rem in problems], fetch=fetch)
        inc = ctx.round_incumbents(garbage, SETTINGS["epsilon"], SETTINGS["offset"])
        exact = ctx.round_exact(garbage, SETTINGS["epsilon"], SETTINGS["offset"], 12, 1 << 40)
        bnb = ctx.round_bnb(garbage, inc["cost2"], SETTINGS["epsilon"], SETTINGS["offset"], 1, 64, 1 << 34, 3, 4096)
        got[fetch] = (arr, inc, exact, bnb)
        r = cluster_prep._Rounds()
        assert ctx._L.fclu_round_results(ctx._h, ctypes.byref(r)) == 0 and r.n_prob == len(problems)
        big = ("inf_off", "inf_seg", "sup_off", "sup_cols", "corr_off", "corr_seg", "pair_off", "pairs", "grp_off", "grp", "grp_seg_off", "grp_seg", "grp_len",
               "row_off", "rows")
        assert all(getattr(r, n) for n in ("refused", "inf_bits_off", "inf_bits", "col_off"))
        assert all(bool(getattr(r, n)) == fetch for n in big)
    full, res = got[True][0], got[False][0]
    assert res["resident"] and sorted(res) == sorted(["resident", "n_prob", "refused", "col_off", "inf_bits_off", "inf_bits"] + list(cluster_prep._ROUND_COUNTS))
    for key in ("refused", "col_off", "inf_bits_off", "inf_bits"):
        assert np.array_equal(full[key], res[key]), key
    assert all(full[n] == res[n] for n in cluster_prep._ROUND_COUNTS) and (full["refused"] >= 0).any()
    with pytest.raises(cluster_prep.ClusterError, match="stayed on the device"):
        cluster_prep.round_model(res, 0)
    for a, b in zip(got[True][1:], got[False][1:]):
        for key in a:
            assert np.array_equal(a[key], b[key]), key
    assert (got[False][2]["cost2"] >= 0).sum() > len(problems) // 2 and (got[False][3]["status"] == 0).any()


def test_refusals_each_followed_by_a_good_call(ctx):
    fresh = cluster_prep.Context(0)
    try:
        with pytest.raises(cluster_prep.ClusterError) as e:                  # no round behind the call
            fresh.round_readout([])
        assert e.value.code == 1
        off = np.zeros(1, np.int64)
        assert fresh._L.fclu_round_readout(fresh._h, off.ctypes.data, None) == 1 and b"fclu_round_models" in fresh._L.fclu_last_error(fresh._h)
        o = cluster_prep._Readout()
        assert fresh._L.fclu_round_readout_results(fresh._h, ctypes.byref(o)) == 1
    finally:
        fresh.close()
    tints = grid_tints()
    part0 = stage(ctx, tints)
    with pytest.raises(cluster_prep.ClusterError):                           # staged, and still no round
        ctx.round_readout([])
    problems = all_problems(tints, lambda t, q, rids: rids)
    good = lambda: readout(ctx, tints, part0, problems, [list(range(len(rem))) for _, _, rem in problems], fetch=False)
    arr, out, sets = good()
    refused = [p for p in range(len(problems)) if arr["refused"][p] >= 0]
    wide = [p for p in range(len(problems)) if arr["refused"][p] < 0 and len(problems[p][2]) >= 3]
    assert refused and wide
    p, R = wide[0], len(problems[wide[0]][2])
    bad = {"outside": ([R], "problem %d: column %d is outside" % (p, R)), "negative": ([-1], "problem %d: column -1 is outside" % p),
           "twice": ([1, 1], "problem %d: column 1 follows column 1" % p), "descending": ([2, 0], "problem %d: column 0 follows column 2" % p)}
    for name, (members, word) in bad.items():
        with pytest.raises(cluster_prep.ClusterError, match=word) as e:
            ctx.round_readout([members if k == p else [] for k in range(len(problems))])
        assert e.value.code == 1, name
        assert ctx.readout_paths() == dict(sets=0, members=0, wide_stores=False, byte_stores=False)
        o = cluster_prep._Readout()
        assert ctx._L.fclu_round_readout_results(ctx._h, ctypes.byref(o)) == 1
        good()
    with pytest.raises(cluster_prep.ClusterError, match="problem %d: a set for a refused problem" % refused[0]) as e:
        ctx.round_readout([[0] if k == refused[0] else [] for k in range(len(problems))])
    assert e.value.code == 1
    good()
    with pytest.raises(cluster_prep.ClusterError, match="sets for the"):
        ctx.round_readout([[0]])
    sel_off = np.zeros(len(problems) + 1, np.int64)
    sel_off[1] = -1
    assert ctx._L.fclu_round_readout(ctx._h, sel_off.ctypes.data, np.zeros(1, np.int32).ctypes.data) == 1 and b"sel_off falls" in ctx._L.fclu_last_error(ctx._h)
    sel_off[:] = 1
    assert ctx._L.fclu_round_readout(ctx._h, sel_off.ctypes.data, np.zeros(1, np.int32).ctypes.data) == 1 and b"starts at 0" in ctx._L.fclu_last_error(ctx._h)
    good()


class Solver:
    """A deterministic solve: the enumeration's mirror up to 12 columns, the branch and bound's behind the greedy's bound above; the rule
    of both is the smallest cost, then the smallest mask, so no tie is left to a solver's mood.  Answers are kept by the model's content."""

    def __init__(self):
        self.calls, self.known = [], {}

    def __call__(self, model, settings):
        self.calls.append(model["key"])
        key = repr([model[k] for k in ("n_cols", "inf_seg", "support", "corrections", "pairs", "groups", "group_segs", "gap_rows", "garbage", "max_lg")])
        if key not in self.known:
            if model["n_cols"] <= 12:
                got = cluster_solve.exact_small(model, settings)
            else:
                greedy = cluster_solve.greedy_incumbent(model, settings)
                got = cluster_solve.exact_bnb(model, settings, None if greedy is None else greedy["cost2"])
                if got["x"] is None:
                    got = greedy
            self.known[key] = (cluster_solve.NO_SOLUTION, None, None) if got is None else (cluster_solve.OPTIMAL, got["x"], got["e"])
        return self.known[key]


LOOPS = {"gpu_proves": dict(max_ilp=40, exact_cols=24, bnb_cols=64), "some_to_the_solver": dict(max_ilp=40, exact_cols=12, bnb_cols=0),
         "all_to_the_solver": dict(max_ilp=20, exact_cols=12, exact_masks=1)}


@pytest.fixture(scope="module")
def solver():
    return Solver()


@pytest.mark.parametrize("name", sorted(LOOPS))
def test_the_loop_on_files(ctx, solver, tmp_path, name):
    """cluster_files() on fixture files with device_rounds on and off: the tints, the logs, the on_round sequence and the cluster_*.tsv
    bytes are the same, and with the flag on a model is built exactly for the problems that reach the solver."""
    paths = [cu.segment_tsv_file(n, tmp_path) for n in ("e_plateau_touch", "g1_dense", "g1_retention")]
    runs = {}
    for flag in (False, True):
        record, built = [], []
        solver.calls = []

        def counting(arr, p):
            built.append(p)
            return cluster_prep.round_model(arr, p)

        settings = cluster.ilp_settings(device_rounds=flag, **LOOPS[name])
        out = list(cluster.cluster_files(paths, settings, ctx=ctx, solve=solver, on_round=record.append, round_model=counting))
        assert len(out) == len(paths) and len(record) > 5
        tsv = []
        for tints, _ in out:
            for tint in tints:
                f = io.StringIO()
                cluster.output_isoforms(tint, f)
                tsv.append(f.getvalue())
        runs[flag] = dict(
            tints=[(t["id"], t["isoforms"], t["garbage_rids"], [(r.get("corrections"), r.get("isoform"), r.get("partition")) for r in t["reads"]])
                   for tints, _ in out for t in tints],
            logs=[logs for _, logs in out], tsv=tsv, built=len(built), solved=list(solver.calls),
            rounds=[(r["tint"]["id"], r["partition"], r["round"], r["remaining"], r["status"], r["x"], r["e"], r["cost"]) for r in record])
    off, on = runs[False], runs[True]
    for key in ("tints", "logs", "rounds", "tsv", "solved"):
        assert on[key] == off[key], key
    assert any(iso for _, iso, _, _ in on["tints"]) and all(text.startswith("#") for text in on["tsv"])
    assert off["built"] == len(off["rounds"])
    assert on["built"] == len(on["solved"])                  # no model for a problem the GPU proved
    if name == "gpu_proves":
        assert on["built"] < len(on["rounds"]) // 2
    elif name == "some_to_the_solver":
        assert 0 < on["built"] < len(on["rounds"])
    else:
        assert on["built"] == len(on["rounds"])
