"""Host side of the clustering rounds, without a GPU: the restatement's informative rows against the reference's own, the loop, read-out
and writer against the reference's cluster_*.tsv bytes (recorded solutions replayed through the solver interface), the HiGHS solve against
the brute force of tests/round_util.py, the command line's refusals and a command-line run through a stand-in context."""
import gzip
import io
import json
import os
import random

import pytest

import cluster_util as cu
import goldens
import round_util as ru
from freddie_amd import cluster, cluster_prep, cluster_solve

CONSTANT = dict(recycle_model="constant")


def small_case(seed, n, M, with_gaps, with_pairs):
    rng = random.Random(seed)
    rows = ru.random_rows(rng, n, M, const_runs=seed % 2 == 0, flip=0.1)
    gaps, polys = ru.random_gaps(rng, rows, p=0.7) if with_gaps else ({}, {})
    tint = ru.make_tint(seed, rows, gaps, polys, members={i: rng.randrange(1, 4) for i in range(n)})
    cluster_prep.preprocess_ilp(tint, CONSTANT)
    incomp = [(a, b) for a in range(n) for b in range(a + 1, n) if rng.random() < 0.25] if with_pairs else []
    return tint, incomp


def model_of(tint, incomp, remaining, settings):
    model = ru.restate(tint, incomp, remaining)
    model["garbage"] = ru.garbage_costs(tint, remaining, settings["recycle_model"])
    model["max_lg"] = sum(s[2] for s in tint["segs"])
    return model


def round_cases():
    """The reference's own results (tests/golden/make_round_golden.py): per case the rounds cluster_tint() ran -- remaining set,
    informative_segs() row, the recorded solution -- and the cluster_*.tsv it wrote."""
    path = os.path.join(goldens.GOLDEN_DIR, "rounds", "rounds.json.gz")
    return json.loads(gzip.open(path).read().decode())


CASES = round_cases()
CASE_IDS = ["%s-%d-%d-%d" % (c["name"], c["max_ilp"], c["min_isoform_size"], c["max_rounds"]) for c in CASES]


def fixture_tint(case, tmp_path):
    """The case's tint as the host mirror's read_segment() + preprocess_ilp() leave it, with the reference's own partitions."""
    tint = list(cluster_prep.read_segment(cu.segment_tsv_file(case["name"], tmp_path)).values())[0]
    cluster_prep.preprocess_ilp(tint, CONSTANT)
    tint["partitions"] = [(list(rids), [tuple(p) for p in inc]) for rids, inc in cu.load_cluster(case["name"])["partitions"][str(case["max_ilp"])]]
    return tint


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_restatement_informative_rows_equal_the_reference(case, tmp_path):
    tint = fixture_tint(case, tmp_path)
    assert case["rounds"]
    for r in case["rounds"]:
        got = "".join("1" if v else "0" for v in ru.informative_segs(tint, r["remaining"]))
        assert got == r["informative"], (r["partition"], r["round"])


@pytest.mark.parametrize("recycle_model", cluster_solve.RECYCLE_MODELS)
@pytest.mark.parametrize("with_gaps,with_pairs", [(False, False), (True, False), (False, True), (True, True)])
def test_solve_reaches_the_brute_force_cost(recycle_model, with_gaps, with_pairs):
    """Costs are multiples of 0.5: equality is abs(diff) < 0.25.  The solver's x must be feasible under the brute force's own check."""
    settings = cluster.ilp_settings(recycle_model)
    solved = 0
    for seed, n, M in ((1, 4, 5), (2, 7, 12), (3, 10, 9), (4, 12, 12), (5, 12, 3), (6, 9, 12)):
        tint, incomp = small_case(seed, n, M, with_gaps, with_pairs)
        remaining = list(range(n))
        random.Random(seed).shuffle(remaining)
        model = model_of(tint, incomp, remaining, settings)
        if model["refused"] is not None:
            continue
        best = ru.brute_force(tint, incomp, remaining, settings)
        status, x, e = cluster_solve.solve_round(model, settings)
        if best is None:                                     # the reference's model has no solution either
            assert status == cluster_solve.NO_SOLUTION
            continue
        best_cost = best[0]
        solved += 1
        assert status == cluster_solve.OPTIMAL
        chosen = set(c for c, v in enumerate(x) if v)
        mine = ru.subset_cost(tint, incomp, remaining, chosen, settings)
        assert mine is not None, "the solver's x is infeasible under the definitions"
        assert abs(mine - best_cost) < 0.25, (seed, mine, best_cost)
        assert abs(cluster_solve.round_cost(model, x, e) - best_cost) < 0.25
    assert solved >= 3


def test_relative_model_is_refused():
    with pytest.raises(ValueError, match="relative"):
        cluster_solve.solve_round(dict(n_cols=0, inf_seg=[]), cluster.ilp_settings("relative"))


class StandInContext:
    """Context.round_models() from the restatement: the loop and the writer without a GPU."""

    def __init__(self, tints, part0):
        self.tints, self.part0 = tints, part0

    def round_models(self, parts, remaining):
        self.problems = [(p, list(r)) for p, r in zip(parts, remaining)]
        return self


    def round_setup(self, *arrays):
        pass

    def close(self):
        pass


def restated_models(monkeypatch, tints):
    """cluster_prep.round_model() of a StandInContext's result: the restatement of the problem."""
    def model(arr, p):
        q, remaining = arr.problems[p]
        t = max(k for k in range(len(arr.part0)) if arr.part0[k] <= q)
        m = ru.restate(tints[t], tints[t]["partitions"][q - arr.part0[t]][1], remaining)
        m.pop("refused")
        return m
    monkeypatch.setattr(cluster_prep, "round_model", model)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_loop_and_writer_give_the_reference_tsv_bytes(case, tmp_path, monkeypatch):
    """The round-batched loop, the read-out and the writer, fed the recorded solutions through the solver interface: byte for byte the
    file the reference's cluster_tint() + output_isoforms() wrote with the same solutions, and the same remaining set in every round."""
    tint = fixture_tint(case, tmp_path)
    recorded = {(r["partition"], r["round"]): r for r in case["rounds"]}
    used = set()

    def replay(model, settings):
        _, q, round_num = model["key"]
        r = recorded[(q, round_num)]
        used.add((q, round_num))
        assert model["n_cols"] == len(r["remaining"]) and model["words"] == ru.restate(tint, [], r["remaining"])["words"]
        return r["status"], r["x"], r["e"]

    ctx = StandInContext([tint], [0])
    restated_models(monkeypatch, [tint])
    settings = cluster.ilp_settings(min_isoform_size=case["min_isoform_size"], max_rounds=case["max_rounds"], max_ilp=case["max_ilp"])
    logs = cluster.cluster_tints([tint], [0], ctx, settings, solve=replay)
    assert used == set(recorded)
    assert [(l[2], l[3], l[4]) for l in logs[0]] == sorted((r["partition"], r["round"], len(r["remaining"])) for r in case["rounds"])
    out = io.StringIO()
    cluster.output_isoforms(tint, out)
    assert out.getvalue().encode() == case["tsv"].encode()


def test_cli_run_through_a_stand_in_context(tmp_path, monkeypatch):
    """The command line end to end without a GPU: directory walk, output and log layout, files the isoforms stage reads.  The stand-in
    context takes the place of the device calls; staging goes through the host mirror and the reference's stored partitions."""
    from freddie_amd import isoforms
    cases = [c for c in CASES if c["name"] in ("e_plateau_touch", "g_tiny") and c["max_ilp"] == 1000][:2]
    seg = tmp_path / "segment" / "ctg"
    seg.mkdir(parents=True)
    tints = {}
    for case in cases:
        tint = fixture_tint(case, tmp_path)
        tints[str(seg / ("segment_ctg_%d.tsv" % tint["id"]))] = tint
        os.replace(cu.segment_tsv_file(case["name"], tmp_path), str(seg / ("segment_ctg_%d.tsv" % tint["id"])))
    (tmp_path / "segment" / "not_a_contig.txt").write_text("x")

    def stage_files(paths, settings, ctx, threads=8):
        batch = [tints[p] for p in paths]
        ctx.part0 = [sum(len(t["partitions"]) for t in batch[:k]) for k in range(len(batch))]
        restated_models(monkeypatch, batch)
        return batch, ctx.part0, list(range(len(batch) + 1))

    monkeypatch.setattr(cluster, "stage_files", stage_files)
    out, logs = tmp_path / "out", tmp_path / "logs"
    argv = ["-s", str(tmp_path / "segment") + "/", "-o", str(out), "-l", str(logs), "-is", "2"]
    assert cluster.main(argv, make_context=lambda device: StandInContext([], [])) == 0
    for tint in tints.values():
        segments, reads, _ = isoforms.read_cluster(str(out / "ctg" / ("cluster_ctg_%d.tsv" % tint["id"])))
        assert [k[1] for k in segments] == [tint["id"]]
        log = (logs / "ctg" / str(tint["id"]) / "timeout.log").read_text().splitlines()
        assert log and all(l.split("\t")[0] in ("OPTIMAL", "NO_SOLUTION") for l in log)
    with pytest.raises(FileExistsError):                     # exist_ok=False, as the reference
        cluster.main(argv, make_context=lambda device: StandInContext([], []))


def test_cli_refusals(tmp_path, capsys):
    for bad in (["-go", "-1"], ["-e", "-0.1"], ["-to", "0"], ["-t", "0"], ["-is", "-1"], ["-mr", "-1"], ["-rm", "nothing"]):
        with pytest.raises(AssertionError):
            cluster.parse_args(["-s", str(tmp_path)] + bad)
    with pytest.raises(SystemExit):
        cluster.parse_args([])
    seg = tmp_path / "seg"
    (seg / "chr1").mkdir(parents=True)
    with pytest.raises(ValueError, match="relative"):
        cluster.main(["-s", str(seg), "-o", str(tmp_path / "out"), "-rm", "relative"])
    with pytest.raises(SystemExit):
        cluster.parse_args(["--help"])
    text = capsys.readouterr().out
    assert "HiGHS" in text and "ties" in text and ".lp" in text
