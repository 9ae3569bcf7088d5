"""The greedy round incumbents without a GPU: the Python mirror (cluster_solve.greedy_incumbent, the definition the device reproduces)
against the brute force and the model's own rows on a grid of small problems, the cutoff and the fallback of solve_round(), the loop
(cluster_tints) through a stand-in context whose round_incumbents() is the mirror, and the command line's flag."""
import functools
import io
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import round_util as ru
from freddie_amd import cluster, cluster_prep, cluster_solve, isoforms
from test_round_host import model_of, small_case

FLAVOURS = [(False, False), (True, False), (False, True), (True, True)]


@functools.lru_cache(maxsize=None)
def grid():
    """The grid's cases that are neither refused nor infeasible, each with every feasible subset's correction count, computed once
    (round_util.subset_cost under the constant model, whose garbage share is subtracted: feasibility and corrections do not depend on the
    recycle model).  [(tint, incomp, remaining, {subset as a bit mask: corrections})]"""
    settings = cluster.ilp_settings()
    out = []
    for seed in range(1, 41):
        n, M = 6 + seed % 7, 5 + seed % 9
        for with_gaps, with_pairs in FLAVOURS:
            tint, incomp = small_case(seed, n, M, with_gaps, with_pairs)
            remaining = list(range(n))
            if ru.restate(tint, incomp, remaining)["refused"] is not None:
                continue
            garbage = ru.garbage_costs(tint, remaining, "constant")
            feasible = {}
            for mask in range(1 << n):
                chosen = set(c for c in range(n) if mask >> c & 1)
                cost = ru.subset_cost(tint, incomp, remaining, chosen, settings)
                if cost is not None:
                    feasible[mask] = cost - sum(g for c, g in enumerate(garbage) if c not in chosen)
            if feasible:
                out.append((tint, incomp, remaining, feasible))
    return out


def row_violation(model, settings, x, e):
    """The largest violation of build_rows()' rows by (x, e, o = x and e and C)."""
    cost, (data, rows, cols), lo, hi, ub, _ = cluster_solve.build_rows(model, settings)
    on = {j for j, v in zip(model["inf_seg"], e) if v}
    o = [int(x[c] and j in on) for c, segs in enumerate(model["corrections"]) for j in segs]
    v = np.array(list(x) + list(e) + o, float)
    assert (v <= ub + 1e-9).all()
    if not len(lo):
        return 0.0
    from scipy.sparse import csr_matrix
    a = csr_matrix((data, (rows, cols)), shape=(lo.size, v.size)) @ v
    return max(float((lo - a).max()), float((a - hi).max()), 0.0)


@pytest.mark.parametrize("recycle_model", cluster_solve.RECYCLE_MODELS)
def test_mirror_on_the_grid(recycle_model):
    """132 cases of the 160 are neither refused nor infeasible.  Optimum reached: constant 127 of 132 (worst ratio 1.200), exons 130 of
    132 (1.113), introns 129 of 132 (1.188); the floor of 90 % only catches a broken greedy."""
    settings = cluster.ilp_settings(recycle_model)
    cases = grid()
    assert len(cases) == 132
    optimal, worst = 0, 1.0
    for tint, incomp, remaining, feasible in cases:
        model = model_of(tint, incomp, remaining, settings)
        garbage = model["garbage"]
        n = len(remaining)
        best = min(corr + sum(g for c, g in enumerate(garbage) if not mask >> c & 1) for mask, corr in feasible.items())
        inc = cluster_solve.greedy_incumbent(model, settings)
        chosen = set(inc["members"])
        assert inc["x"] == [int(c in chosen) for c in range(n)] and inc["cost"] == inc["cost2"] / 2.0
        mine = ru.subset_cost(tint, incomp, remaining, chosen, settings)
        assert mine is not None, "the incumbent is infeasible under the definitions"
        assert mine == inc["cost"] == cluster_solve.round_cost(model, inc["x"], inc["e"])
        assert inc["cost"] >= best - 1e-9
        assert inc["e"] == [int(any(inc["x"][c] for c in support)) for support in model["support"]]
        assert row_violation(model, settings, inc["x"], inc["e"]) <= 1e-6
        optimal += inc["cost"] == best
        worst = max(worst, inc["cost"] / best if best else 1.0)
    print("%s: optimum reached in %d of %d, worst ratio %.3f" % (recycle_model, optimal, len(cases), worst))
    assert optimal >= 0.9 * len(cases)


def test_mirror_arguments():
    tint, incomp = small_case(3, 8, 9, True, True)
    settings = cluster.ilp_settings()
    model = model_of(tint, incomp, list(range(8)), settings)
    with pytest.raises(ValueError, match="max_seeds"):
        cluster_solve.greedy_incumbent(model, settings, 0)
    with pytest.raises(ValueError, match="multiple of 0.5"):
        cluster_solve.greedy_incumbent(dict(model, garbage=[3.25] * 8), settings)
    with pytest.raises(ValueError, match="8 columns"):
        cluster_solve.greedy_incumbent(dict(model, garbage=[3.0] * 7), settings)
    one = cluster_solve.greedy_incumbent(model, settings, 1)
    many = cluster_solve.greedy_incumbent(model, settings, 1000)
    assert one["start"] in (0, 1) and many["start"] <= 8 and many["cost2"] <= one["cost2"]
    empty = cluster_solve.greedy_incumbent(dict(model_of(tint, incomp, [], settings)), settings)
    assert empty["cost2"] == 0 and empty["members"] == [] and empty["start"] == 0


@pytest.mark.parametrize("recycle_model", cluster_solve.RECYCLE_MODELS)
@pytest.mark.parametrize("with_gaps,with_pairs", FLAVOURS)
def test_solve_with_an_incumbent_reaches_the_brute_force_cost(recycle_model, with_gaps, with_pairs):
    """The cases of test_solve_reaches_the_brute_force_cost with the cutoff row: the optimum stays feasible (costs are multiples of 0.5)."""
    settings = cluster.ilp_settings(recycle_model, incumbent="cutoff")
    solved = 0
    for seed, n, M in ((1, 4, 5), (2, 7, 12), (3, 10, 9), (4, 12, 12), (5, 12, 3), (6, 9, 12)):
        tint, incomp = small_case(seed, n, M, with_gaps, with_pairs)
        remaining = list(range(n))
        random.Random(seed).shuffle(remaining)
        model = model_of(tint, incomp, remaining, settings)
        if model["refused"] is not None:
            continue
        best = ru.brute_force(tint, incomp, remaining, settings)
        inc = cluster_solve.greedy_incumbent(model, settings)
        if best is None:                                     # no feasible subset: no start of the greedy ends feasible either
            assert inc is None
            continue
        assert inc is not None and inc["cost"] >= best[0]
        model["incumbent"] = (inc["cost"], inc["x"])
        status, x, e = cluster_solve.solve_round(model, settings)
        solved += 1
        assert status == cluster_solve.OPTIMAL
        mine = ru.subset_cost(tint, incomp, remaining, set(c for c, v in enumerate(x) if v), settings)
        assert mine is not None and abs(mine - best[0]) < 0.25, (seed, mine, best[0])
        assert abs(cluster_solve.round_cost(model, x, e) - best[0]) < 0.25
    assert solved >= 3


class TimedOut:
    status, x = 1, None


def patch_timeout(monkeypatch):
    import scipy.optimize
    monkeypatch.setattr(scipy.optimize, "milp", lambda *a, **k: TimedOut())


def test_timeout_returns_the_incumbent_only_under_fallback(monkeypatch):
    patch_timeout(monkeypatch)
    tint, incomp = small_case(4, 12, 12, True, True)
    remaining = list(range(12))
    for mode in cluster_solve.INCUMBENT_MODES:
        settings = cluster.ilp_settings(incumbent=mode)
        model = model_of(tint, incomp, remaining, settings)
        inc = cluster_solve.greedy_incumbent(model, settings)
        assert inc["members"]
        if mode != "off":
            model["incumbent"] = (inc["cost"], inc["x"])
        status, x, e = cluster_solve.solve_round(model, settings)
        if mode == "fallback":
            assert (status, x, e) == (cluster_solve.INCUMBENT, inc["x"], inc["e"])
        else:
            assert (status, x, e) == (cluster_solve.NO_SOLUTION, None, None)
    with pytest.raises(ValueError, match="incumbent mode"):
        cluster_solve.check_settings(cluster.ilp_settings(incumbent="warm"))


class MirrorContext:
    """Context.round_models() / round_incumbents() from the restatement and the mirror: the loop without a GPU."""

    def __init__(self, tints, part0):
        self.tints, self.part0, self.incumbent_calls = tints, part0, 0

    def model(self, p):
        q, remaining = self.problems[p]
        t = max(k for k in range(len(self.part0)) if self.part0[k] <= q)
        m = ru.restate(self.tints[t], self.tints[t]["partitions"][q - self.part0[t]][1], remaining)
        assert m.pop("refused") is None
        return m

    def round_models(self, parts, remaining):
        self.problems = [(p, list(r)) for p, r in zip(parts, remaining)]
        return self

    def round_incumbents(self, garbage, epsilon, offset, max_seeds=64):
        self.incumbent_calls += 1
        col_off, cost2, mem_off, mem = [0], [], [0], []
        for p, (_, remaining) in enumerate(self.problems):
            col_off.append(col_off[-1] + len(remaining))
            q = self.problems[p][0]
            tint = self.tints[max(k for k in range(len(self.part0)) if self.part0[k] <= q)]
            inc = cluster_solve.greedy_incumbent(dict(self.model(p), garbage=list(garbage[col_off[p]:col_off[p + 1]]), max_lg=sum(s[2] for s in tint["segs"])),
                                                 dict(epsilon=epsilon, offset=offset), max_seeds)
            cost2.append(-1 if inc is None else inc["cost2"]); mem.extend(inc["members"] if inc else []); mem_off.append(len(mem))
        assert len(garbage) == col_off[-1]
        return dict(n_prob=len(cost2), col_off=np.array(col_off), cost2=np.array(cost2), mem_off=np.array(mem_off), mem=np.array(mem, np.int32))


def loop_tints():
    tints = []
    for seed, n, M in ((2, 9, 12), (4, 12, 12), (6, 9, 12), (8, 11, 10)):
        tint, incomp = small_case(seed, n, M, False, True)   # (no gaps: no later round's subset is one the reference refuses)
        half = n // 2
        tint["partitions"] = [(list(range(half)), [p for p in incomp if p[0] < half and p[1] < half]),
                              (list(range(half, n)), [p for p in incomp if p[0] >= half and p[1] >= half])]
        tints.append(tint)
    return tints, [0, 2, 4, 6]


def run_loop(monkeypatch, mode):
    tints, part0 = loop_tints()
    ctx = MirrorContext(tints, part0)
    monkeypatch.setattr(cluster_prep, "round_model", lambda arr, p: arr.model(p))
    record = []
    logs = cluster.cluster_tints(tints, part0, ctx, cluster.ilp_settings(min_isoform_size=2, incumbent=mode), on_round=record.append)
    return tints, ctx, logs, record


def test_loop_off_makes_no_call_and_cutoff_reaches_the_same_costs(monkeypatch):
    _, ctx_off, logs_off, rec_off = run_loop(monkeypatch, "off")
    assert ctx_off.incumbent_calls == 0 and rec_off
    _, ctx_cut, logs_cut, rec_cut = run_loop(monkeypatch, "cutoff")
    assert ctx_cut.incumbent_calls == len(set(r["round"] for r in rec_cut)) > 0
    key = lambda r: (r["tint"]["id"], r["partition"], r["round"])
    assert sorted((key(r), r["status"], r["cost"]) for r in rec_off) == sorted((key(r), r["status"], r["cost"]) for r in rec_cut)
    assert all(l[0] == "OPTIMAL" for lines in logs_cut for l in lines)


def test_loop_fallback_goes_on_behind_a_timeout(monkeypatch, tmp_path):
    patch_timeout(monkeypatch)
    _, _, logs_cut, rec_cut = run_loop(monkeypatch, "cutoff")
    assert rec_cut and all(r["status"] == "NO_SOLUTION" and r["round"] == 0 for r in rec_cut)      # every partition abandoned at once
    tints, ctx, logs, record = run_loop(monkeypatch, "fallback")
    assert all(r["status"] == "INCUMBENT" and r["cost"] is not None for r in record)
    assert max(r["round"] for r in record) >= 1, "no partition went past its first round"
    assert all(l[0] == "INCUMBENT" for lines in logs for l in lines) and any(logs)
    assert any(t["isoforms"] for t in tints)
    for tint in tints:
        out = io.StringIO()
        cluster.output_isoforms(tint, out)
        path = tmp_path / ("cluster_chr1_%d.tsv" % tint["id"])
        path.write_text(out.getvalue())
        segments, reads, _ = isoforms.read_cluster(str(path))
        assert [k[1] for k in segments] == [tint["id"]]
        assert bool(reads) == bool(tint["isoforms"])


def test_cli_flag(tmp_path):
    base = ["-s", str(tmp_path)]
    assert cluster.parse_args(base).incumbent == "off"
    for mode in ("off", "cutoff", "fallback"):
        assert cluster.parse_args(base + ["--incumbent", mode]).incumbent == mode
    for bad in ("on", "warm", ""):
        with pytest.raises(SystemExit):
            cluster.parse_args(base + ["--incumbent", bad])
    assert cluster.ilp_settings()["incumbent"] == "off" and cluster.ilp_settings(incumbent="fallback")["incumbent"] == "fallback"


def test_kernel_bodies_on_the_host():
    """What one thread of k_inc_start / k_inc_pick computes (freddie_amd/csrc/clu_incumbent.h), compiled for the host with the address and
    undefined-behaviour sanitizers and run over a workgroup's threads in the kernels' order of steps, against the mirror: both row paths."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, os.path.join(root, "tools", "incumbent_host_check.py"), "--cases", "24"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "both paths: 0 differ" in res.stdout, res.stdout + res.stderr
