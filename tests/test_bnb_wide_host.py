"""The branch and bound over problems of up to 1024 columns without a GPU: the mirror cluster_solve.exact_bnb_wide() -- the definition of
fclu_round_bnb_wide -- against exact_bnb() where both apply, on built problems of 65 .. 200 columns whose optimum lies at the upper
columns, on the two-optima tie across the word boundary, the cap, the arguments; the settings and command-line flags; the loop
cluster_tints() through a stand-in context whose round_bnb_wide() is the mirror, with device_rounds on a partition of 70 reps too; and the kernels' per-lane code on the host."""
import os
import subprocess
import sys

import numpy as np
import pytest

import round_util as ru
from freddie_amd import cluster, cluster_prep, cluster_solve
from test_bnb_host import BnbContext, run_bnb_loop, summary
from test_device_rounds_host import DeviceContext, outcome
from test_incumbent_host import loop_tints
from test_round_host import model_of, small_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bnb_host_check import family_model, family_tint, greedy2  # noqa: E402
from bnb_wide_host_check import bare_model, tie_model  # noqa: E402


def test_equals_the_64_column_mirror_on_the_grid():
    """The 40-seed grid with and without gaps and pairs, with the greedy's bound and without one, at depths 0 .. 12 and three caps: whole
    dicts, node counts included."""
    n = capped = 0
    for seed in range(1, 41):
        for with_gaps, with_pairs in ((False, False), (True, False), (False, True), (True, True)):
            tint, incomp = small_case(seed, 6 + seed % 7, 5 + seed % 9, with_gaps, with_pairs)
            settings = cluster.ilp_settings(cluster_solve.RECYCLE_MODELS[seed % 3])
            model = model_of(tint, incomp, list(range(6 + seed % 7)), settings)
            if model["refused"] is not None:
                continue
            depth, node_cap = (0, 1, 2, 3, 12)[seed % 5], (1, 7, 4096)[seed // 5 % 3]
            for ub2 in (None, greedy2(model, settings)):
                want = cluster_solve.exact_bnb(model, settings, ub2, depth, node_cap)
                assert cluster_solve.exact_bnb_wide(model, settings, ub2, depth, node_cap) == want
                n += 1
                capped += want["capped"] > 0
    assert n > 200 and capped
    assert cluster_solve.exact_bnb_wide(model, settings) == cluster_solve.exact_bnb(model, settings)      # (the defaults agree at this size)


@pytest.mark.parametrize("R,n_low", [(33, 32), (64, 32)])
def test_equals_the_64_column_mirror_on_the_families(R, n_low):
    settings = cluster.ilp_settings()
    model = family_model(R, n_low)[0]
    for ub2, depth, node_cap in ((greedy2(model, settings), 6, 4096), (None, 3, 64)):
        assert cluster_solve.exact_bnb_wide(model, settings, ub2, depth, node_cap) == cluster_solve.exact_bnb(model, settings, ub2, depth, node_cap)


@pytest.mark.parametrize("R,n_low", [(65, 64), (65, 32), (128, 64), (129, 128), (200, 70)])
def test_the_optimum_beyond_column_63(R, n_low):
    """Two families, every cross pair incompatible, the cheaper one at the columns n_low .. R - 1: bounded by the greedy at depth 6 the
    search ends optimal with exactly those columns and no task capped."""
    settings = cluster.ilp_settings()
    model = family_model(R, n_low)[0]
    got = cluster_solve.exact_bnb_wide(model, settings, greedy2(model, settings), 6)
    assert got["status"] == "optimal" and got["capped"] == 0
    assert got["mask"] == ((1 << R) - 1) ^ ((1 << n_low) - 1) and got["members"] == list(range(n_low, R))
    assert got["cost2"] == 2 * ((R - n_low - 1) + 3 * n_low) and got["x"] == [0] * n_low + [1] * (R - n_low)


def test_the_smaller_mask_wins_across_the_word_boundary():
    """128 columns, two optimal sets and no third: the columns 0 .. 63 and the columns 64 .. 127, equal by the yardstick's cost.  The
    smaller integer is the lower set, whose most significant word is empty."""
    settings = cluster.ilp_settings()
    model, tint, incomp = tie_model()
    remaining = list(range(128))
    low, high = ru.subset_cost(tint, incomp, remaining, set(range(64)), settings), ru.subset_cost(tint, incomp, remaining, set(range(64, 128)), settings)
    assert low is not None and low == high
    for ub2 in (None, int(2 * low)):
        got = cluster_solve.exact_bnb_wide(model, settings, ub2, 6)
        assert (got["status"], got["cost"], got["mask"], got["capped"]) == ("optimal", low, (1 << 64) - 1, 0)
    assert cluster_solve.exact_bnb_wide(model, settings, int(2 * low) - 1, 6)["status"] == "unproven"       # nothing is cheaper
    for drop in (0, 5, 63, 64, 100, 127):                    # no third optimum next to either
        for base in (set(range(64)), set(range(64, 128))):
            other = ru.subset_cost(tint, incomp, remaining, base ^ {drop} if drop in base else base, settings)
            assert drop not in base or other > low


def test_the_cap():
    """65 columns at depth 2: with 40 nodes a task the four tasks stop capped and the search is unproven with the best set so far; the
    counts are node_cap a capped task."""
    settings = cluster.ilp_settings()
    model = family_model(65, 32)[0]
    got = cluster_solve.exact_bnb_wide(model, settings, None, 2, 40)
    assert got["status"] == "unproven" and got["capped"] > 0 and got["nodes"] <= 4 * 40
    tb = cluster_solve.bnb_tables(model, settings, cluster_solve.BNB_WIDE_MAX_COLS)
    tasks = [cluster_solve.bnb_task(tb, t, 2, None, 40) for t in range(4)]
    assert all(n == 40 for _, _, n, cap in tasks if cap) and got["nodes"] == sum(t[2] for t in tasks)
    one = cluster_solve.exact_bnb_wide(model, settings, None, 2, 1)
    assert one["status"] == "unproven" and one["nodes"] == 4 and one["mask"] is None
    assert cluster_solve.bnb_wide_node_cap(64) == cluster_solve.BNB_NODE_CAP and all(cluster_solve.bnb_wide_node_cap(R) >= 4 * R for R in (65, 128, 256, 1024))


def test_arguments():
    settings = cluster.ilp_settings()
    with pytest.raises(ValueError, match="1024 at the most"):
        cluster_solve.exact_bnb_wide(bare_model(1025), settings)
    got = cluster_solve.exact_bnb_wide(bare_model(1024), settings, None, 0, 4096)
    assert (got["status"], got["cost2"], got["mask"], got["nodes"]) == ("optimal", 0, (1 << 1024) - 1, 2049)
    with pytest.raises(ValueError, match="at least 0 and 1"):
        cluster_solve.exact_bnb_wide(bare_model(70), settings, None, -1)
    with pytest.raises(ValueError, match="at least 0 and 1"):
        cluster_solve.exact_bnb_wide(bare_model(70), settings, None, 6, 0)
    with pytest.raises(ValueError, match="64 at the most"):  # (the 64-column mirror refuses what it refused)
        cluster_solve.exact_bnb(bare_model(65), settings)


def test_the_lds_rule_and_the_solution():
    """bnb_wide_lds_bytes() is the header's bw_lds_bytes(): 16 R ceil(E / 64) + 4 R + 64 (9 W + 2 ceil(E / 64)), rounded up to 16."""
    assert cluster_prep.bnb_wide_lds_bytes(70, 0) == (4 * 70 + 64 * 18 + 15) // 16 * 16
    assert cluster_prep.bnb_wide_lds_bytes(1024, 576) == 16 * 1024 * 9 + 4096 + 64 * (144 + 18) <= cluster_prep.BNB_WIDE_LDS_BYTES
    assert cluster_prep.bnb_wide_lds_bytes(1024, 577) > cluster_prep.BNB_WIDE_LDS_BYTES
    header = open(os.path.join(ROOT, "freddie_amd", "csrc", "clu_bnb_wide.h")).read()
    assert "constexpr int kBwWaves = %d;" % cluster_prep.BNB_WIDE_WAVES in header and "constexpr int kBwLdsBytes = 160 * 1024;" in header
    mask = np.zeros((5, 16), np.uint64)
    mask[0, 0], mask[3, 0], mask[3, 1] = 5, 1, 2
    arr = dict(col_off=np.array([0, 3, 5, 6, 72, 74]), status=np.array([0, 1, -2, 2, 2], np.int32), cost2=np.array([7, -1, -1, 9, -1]), mask=mask)
    assert cluster_prep.round_bnb_wide_solution(arr, 0) == (3.5, [1, 0, 1])
    assert cluster_prep.round_bnb_wide_solution(arr, 1) == "infeasible"
    assert cluster_prep.round_bnb_wide_solution(arr, 2) is None
    assert cluster_prep.round_bnb_wide_solution(arr, 3) == ("unproven", 4.5, [1] + [0] * 64 + [1])
    assert cluster_prep.round_bnb_wide_solution(arr, 4) == ("unproven", None, None)


def test_settings_and_cli_flags(tmp_path):
    settings = cluster.ilp_settings()
    assert settings["wide_cols"] == 0 and settings["wide_nodes"] == cluster.WIDE_NODES
    cluster.check_wide(settings)
    cluster.check_wide(cluster.ilp_settings(wide_cols=1024, wide_nodes=1))
    cluster.check_wide({})                                   # (settings from before the feature)
    with pytest.raises(ValueError, match="wide_cols"):
        cluster.check_wide(cluster.ilp_settings(wide_cols=1025))
    with pytest.raises(ValueError, match="wide_cols"):
        cluster.check_wide(cluster.ilp_settings(wide_cols=-1))
    with pytest.raises(ValueError, match="wide_nodes"):
        cluster.check_wide(cluster.ilp_settings(wide_cols=300, wide_nodes=0))
    assert cluster.ilp_settings(wide_cols=200, device_rounds=True)["device_rounds"] is True
    cluster.check_device_rounds(dict(device_rounds=True, wide_cols=200))
    with pytest.raises(ValueError, match="bnb_cols"):        # (the 64-column search keeps its limit)
        cluster.check_bnb(cluster.ilp_settings(bnb_cols=65))
    base = ["-s", str(tmp_path)]
    args = cluster.parse_args(base)
    assert args.exact_wide == 0 and args.wide_nodes == cluster.WIDE_NODES
    for n in (0, 1, 65, 1024):
        assert cluster.parse_args(base + ["--exact-wide", str(n)]).exact_wide == n
    assert cluster.parse_args(base + ["--exact-wide", "400", "--wide-nodes", "1000"]).wide_nodes == 1000
    assert cluster.parse_args(base + ["--exact-wide", "400", "--device-rounds"]).device_rounds is True
    for bad in (["--exact-wide", "1025"], ["--exact-wide", "-1"], ["--exact-wide", "x"], ["--wide-nodes", "0"], ["--exact-bnb", "65"]):
        with pytest.raises(SystemExit):
            cluster.parse_args(base + bad)


class WideContext(BnbContext):
    """BnbContext with a round_bnb_wide() that is the mirror behind the library's rule of which problems are taken."""

    def __init__(self, tints, part0, depth, node_cap):
        BnbContext.__init__(self, tints, part0, depth, node_cap)
        self.wide_calls, self.wide_args = 0, []

    def round_bnb_wide(self, garbage, ub2, epsilon, offset, min_cols, max_cols, max_nodes, depth=None, node_cap=None):
        self.wide_calls += 1
        self.wide_args.append((min_cols, max_cols, max_nodes))
        col_off = np.cumsum([0] + [len(rem) for _, rem in self.problems])
        assert len(garbage) == col_off[-1] and len(ub2) == len(self.problems)
        P = len(self.problems)
        status, cost2, mask, total = [-2] * P, [-1] * P, np.zeros((P, 16), np.uint64), 0
        for R, p in sorted((len(rem), p) for p, (_, rem) in enumerate(self.problems) if min_cols <= len(rem) <= max_cols):
            if total + (self.node_cap << min(R, self.depth)) > max_nodes:
                break
            total += self.node_cap << min(R, self.depth)
            q = self.problems[p][0]
            tint = self.tints[max(k for k in range(len(self.part0)) if self.part0[k] <= q)]
            model = dict(self.model(p), garbage=list(garbage[col_off[p]:col_off[p + 1]]), max_lg=sum(s[2] for s in tint["segs"]))
            got = cluster_solve.exact_bnb_wide(model, dict(epsilon=epsilon, offset=offset), None if ub2[p] < 0 else int(ub2[p]), self.depth, self.node_cap)
            status[p] = ("optimal", "infeasible", "unproven").index(got["status"])
            if got["mask"] is not None:
                cost2[p] = got["cost2"]
                for w in range(16):
                    mask[p, w] = got["mask"] >> (64 * w) & (2 ** 64 - 1)
            self.results.append((q, tuple(self.problems[p][1]), got))
        return dict(n_prob=P, col_off=col_off, status=np.array(status, np.int32), cost2=np.array(cost2, np.int64), mask=mask)


def run_wide_loop(monkeypatch, depth, node_cap, settings):
    tints, part0 = loop_tints()
    ctx = WideContext(tints, part0, depth, node_cap)
    monkeypatch.setattr(cluster_prep, "round_model", lambda arr, p: arr.model(p))
    record, jobs = [], []

    def solve(model, s):
        jobs.append((model["key"], model["n_cols"], model.get("incumbent")))
        return cluster_solve.solve_round(model, s)

    logs = cluster.cluster_tints(tints, part0, ctx, settings, solve=solve, on_round=record.append)
    return ctx, logs, record, jobs


def test_loop_a_proven_problem_gets_no_solve_job(monkeypatch):
    """Partitions of 4 .. 6 reps under wide_cols = 12.  With room to finish every problem is proven and the solver is never called, one
    round_bnb_wide and one round_incumbents call a round, and the records are those of the 64-column search; with 4 nodes a task some
    searches stop early and each of those makes one job."""
    base = dict(min_isoform_size=2)
    ctx, logs, record, jobs = run_wide_loop(monkeypatch, 12, 4096, cluster.ilp_settings(wide_cols=12, **base))
    rounds = len(set(r["round"] for r in record))
    assert record and not jobs and ctx.wide_calls == ctx.incumbent_calls == rounds and ctx.bnb_calls == 0
    assert all(got["status"] == "optimal" for _, _, got in ctx.results) and len(ctx.results) == len(record)
    assert set(ctx.wide_args) == {(1, 12, cluster.WIDE_NODES)}
    for r in record:
        assert r["status"] == "OPTIMAL" and r["cost"] == ru.brute_force(r["tint"], r["incomp"], r["remaining"], cluster.ilp_settings())[0]
    narrow = run_bnb_loop(monkeypatch, 12, 4096, cluster.ilp_settings(bnb_cols=12, **base))
    assert summary(record) == summary(narrow[2]) and logs == narrow[1]

    ctx, logs, record, jobs = run_wide_loop(monkeypatch, 2, 4, cluster.ilp_settings(wide_cols=12, **base))
    unproven = [got for _, _, got in ctx.results if got["status"] == "unproven"]
    assert unproven and len(jobs) == len(unproven) and any(inc is not None for _, _, inc in jobs)
    assert all(r["status"] == "OPTIMAL" for r in record)


def test_loop_without_the_feature_makes_no_call_and_respects_the_sizes(monkeypatch):
    """wide_cols = 0, settings that do not know the feature, and a wide_cols at or under bnb_cols: no round_bnb_wide call, the same
    records.  Beside the 64-column search the wide one starts behind it and shares the incumbents call."""
    base = dict(min_isoform_size=2)
    ctx0, logs0, record0, jobs0 = run_wide_loop(monkeypatch, 12, 4096, cluster.ilp_settings(wide_cols=0, **base))
    assert ctx0.wide_calls == 0 and ctx0.incumbent_calls == 0 and len(jobs0) == len(record0) > 0
    old = {k: v for k, v in cluster.ilp_settings(**base).items() if not k.startswith("wide_")}
    ctx1, logs1, record1, jobs1 = run_wide_loop(monkeypatch, 12, 4096, old)
    assert ctx1.wide_calls == 0 and logs0 == logs1 and jobs0 == jobs1
    ctx2, _, _, _ = run_wide_loop(monkeypatch, 12, 4096, cluster.ilp_settings(bnb_cols=12, wide_cols=12, **base))
    assert ctx2.wide_calls == 0 and ctx2.bnb_calls > 0
    ctx3, _, record3, jobs3 = run_wide_loop(monkeypatch, 12, 4096, cluster.ilp_settings(bnb_cols=4, wide_cols=12, max_rounds=1, **base))
    assert ctx3.wide_args == [(5, 12, cluster.WIDE_NODES)] and ctx3.bnb_calls == 1 and ctx3.incumbent_calls == 1 and not jobs3
    assert sorted(len(r["remaining"]) for r in record3)[-1] > 4 and all(r["status"] == "OPTIMAL" for r in record3)


class WideDeviceContext(DeviceContext):
    """DeviceContext (resident round_models(), a round_readout() that is the mirror) with WideContext's round_bnb_wide()."""
    round_bnb_wide = WideContext.round_bnb_wide

    def __init__(self, tints, part0, depth, node_cap):
        DeviceContext.__init__(self, tints, part0)
        self.depth, self.node_cap, self.results, self.wide_calls, self.wide_args = depth, node_cap, [], 0, []


def wide_loop_tints():
    """One tint, one partition of 70 reps: a family of 6 and one of 64, every cross pair incompatible (family_tint())."""
    tint, incomp = family_tint(0, 70, 6)
    cluster_prep.preprocess_ilp(tint, dict(recycle_model="constant"))
    tint["partitions"] = [(list(range(70)), incomp)]
    return [tint], [0]


def test_loop_with_device_rounds_reads_out_a_set_of_two_words():
    """wide_cols = 128 alone enables device_rounds.  A partition of 70 reps: the first round's proven set is the columns 6 .. 69, its x
    reaches the read-out as a list of 70 and crosses the word; the tints, the logs and the on_round sequence are those of the run with
    device_rounds off, no model is built on the host and no solve job made."""
    got = {}
    for flag in (False, True):
        tints, part0 = wide_loop_tints()
        ctx = WideDeviceContext(tints, part0, 6, 4096)
        record, jobs = [], []
        settings = cluster.ilp_settings(min_isoform_size=2, wide_cols=128, device_rounds=flag)
        logs = cluster.cluster_tints(tints, part0, ctx, settings, solve=lambda m, s: jobs.append(m["key"]) or cluster_solve.solve_round(m, s),
                                     on_round=lambda r: record.append((r["partition"], r["round"], r["remaining"], r["status"], r["x"], r["e"], r["cost"])),
                                     round_model=ctx.build)
        got[flag] = (logs, record, outcome(tints))
        assert not jobs and ctx.wide_calls == len(record) >= 2 and set(ctx.wide_args) == {(1, 128, cluster.WIDE_NODES)}
        assert record[0][3] == "OPTIMAL" and record[0][4] == [0] * 6 + [1] * 64 and record[0][6] == (70 - 6 - 1) + 3 * 6
        if flag:
            assert ctx.built == 0 and all(not fetch for _, fetch in ctx.model_calls) and ctx.readouts[0] == 1
            members = tints[0]["isoforms"][0]["rid_to_corrections"]
            assert sorted(members) == list(range(6, 70))
    assert got[True] == got[False]


def test_kernel_bodies_on_the_host():
    """What the lanes of k_bw_prep / k_bw_search compute and the task walk (freddie_amd/csrc/clu_bnb_wide.h), compiled for the host with
    the address and undefined-behaviour sanitizers and run over every task of a third of the grid's problems and of built ones of 65 ..
    300 columns, the lanes of a wave one after another, against the mirror."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bnb_wide_host_check.py")], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and " 0 differ" in res.stdout, res.stdout + res.stderr
