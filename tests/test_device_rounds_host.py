"""The loop under device_rounds without a GPU: the flag's validation on the command line and in ilp_settings(), and cluster_tints() on a
stand-in context whose round_readout() is the numpy mirror -- the tints, the logs and the on_round sequence are those of the run with the
flag off, no model is built for a problem the exact call answered, and the other problems are modelled by a second call on them alone."""
import copy

import numpy as np
import pytest

import round_util as ru
from freddie_amd import cluster, cluster_prep
from test_exact_host import ExactContext
from test_incumbent_host import loop_tints


class DeviceContext(ExactContext):
    """ExactContext with round_models(fetch=False) -- the small arrays alone -- and a round_readout() that is the mirror."""

    def __init__(self, tints, part0):
        ExactContext.__init__(self, tints, part0)
        self.model_calls, self.readouts, self.built = [], [], 0

    def tint_of(self, q):
        return max(k for k in range(len(self.part0)) if self.part0[k] <= q)

    def round_models(self, parts, remaining, fetch=True):
        ExactContext.round_models(self, parts, remaining)
        self.model_calls.append((len(parts), fetch))
        if fetch:
            return self
        self.informative = [[int(v) for v in ru.informative_segs(self.tints[self.tint_of(q)], rem)] for q, rem in self.problems]
        words = [cluster_prep._pack_bits([inf], len(inf))[0] for inf in self.informative]
        return dict(resident=True, n_prob=len(parts), refused=np.full(len(parts), -1, np.int32), inf_bits=np.concatenate(words),
                    inf_bits_off=np.cumsum([0] + [len(w) for w in words]))

    def round_readout(self, sets):
        assert len(sets) == len(self.problems) and self.model_calls[-1][1] is False, "the read-out stands behind the resident call"
        self.readouts.append(sum(1 for x in sets if x))
        return cluster_prep.readout_mirror(self.tints, [(self.tint_of(q), rem) for q, rem in self.problems], sets, self.informative)

    def build(self, arr, p):
        self.built += 1
        return arr.model(p)


def run(device_rounds, min_isoform_size=2, **settings):
    tints, part0 = loop_tints()
    ctx = DeviceContext(tints, part0)
    record = []
    logs = cluster.cluster_tints(tints, part0, ctx, cluster.ilp_settings(min_isoform_size=min_isoform_size, device_rounds=device_rounds, **settings),
                                 on_round=lambda r: record.append((r["tint"]["id"], r["partition"], r["round"], r["remaining"], r["status"], r["x"], r["e"], r["cost"])),
                                 round_model=ctx.build)
    return tints, ctx, logs, record


def outcome(tints):
    return [(t["isoforms"], t["garbage_rids"], [(r.get("corrections"), r.get("isoform"), r.get("partition")) for r in t["reads"]]) for t in tints]


@pytest.mark.parametrize("settings", [dict(exact_cols=12), dict(exact_cols=4), dict(exact_cols=12, exact_masks=32), dict(exact_cols=5, incumbent="cutoff"),
                                      dict(exact_cols=12, min_isoform_size=4)], ids=["all", "some", "budget", "cutoff", "min4"])
def test_the_flag_changes_nothing_but_the_work(settings):
    t_off, c_off, logs_off, rec_off = run(False, **settings)
    t_on, c_on, logs_on, rec_on = run(True, **settings)
    assert rec_off and any(t["isoforms"] for t in t_off)
    assert logs_on == logs_off and rec_on == rec_off and outcome(t_on) == outcome(t_off)
    assert all(fetch for _, fetch in c_off.model_calls) and c_off.built == len(rec_off) and not c_off.readouts
    rounds = len(set(r[2] for r in rec_on))
    assert [fetch for _, fetch in c_on.model_calls].count(False) == rounds and c_on.model_calls[0][1] is False
    assert c_on.built == len(rec_on) - c_on.taken                     # a model only where the exact call took nothing
    assert sum(n for n, fetch in c_on.model_calls if fetch) == c_on.built          # ... from calls on those problems alone
    if settings == dict(exact_cols=12):
        assert c_on.built == 0 and all(not fetch for _, fetch in c_on.model_calls) and sum(c_on.readouts) > 0
    else:
        assert 0 < c_on.taken


def test_without_on_round_the_results_are_the_same():
    tints, part0 = loop_tints()
    want = copy.deepcopy(run(False, exact_cols=12)[0])
    ctx = DeviceContext(tints, part0)
    cluster.cluster_tints(tints, part0, ctx, cluster.ilp_settings(min_isoform_size=2, exact_cols=12, device_rounds=True), round_model=ctx.build)
    assert outcome(tints) == outcome(want)


def test_a_refused_problem_raises_as_today():
    tints, part0 = loop_tints()

    class Refusing(DeviceContext):
        def round_models(self, parts, remaining, fetch=True):
            arr = DeviceContext.round_models(self, parts, remaining, fetch)
            arr["refused"][1] = 2
            return arr

    with pytest.raises(cluster_prep.ClusterError, match=r"partition 1 round 0: a gap of column 2 \(rep %d\)" % tints[0]["partitions"][1][0][2]):
        cluster.cluster_tints(tints, part0, Refusing(tints, part0), cluster.ilp_settings(min_isoform_size=2, exact_cols=12, device_rounds=True))


def test_settings_and_flags(tmp_path):
    assert cluster.ilp_settings()["device_rounds"] is False
    assert cluster.ilp_settings(exact_cols=3, device_rounds=True)["device_rounds"] is True
    assert cluster.ilp_settings(bnb_cols=40, device_rounds=True)["device_rounds"] is True
    with pytest.raises(ValueError, match="device_rounds"):
        cluster.ilp_settings(device_rounds=True)
    with pytest.raises(ValueError, match="device_rounds"):
        cluster.check_device_rounds(dict(device_rounds=True, exact_cols=0, bnb_cols=0))
    cluster.check_device_rounds(dict())                      # (settings from before the flag)
    base = ["-s", str(tmp_path)]
    assert cluster.parse_args(base).device_rounds is False
    assert cluster.parse_args(base + ["--exact-small", "12", "--device-rounds"]).device_rounds is True
    assert cluster.parse_args(base + ["--exact-bnb", "64", "--device-rounds"]).device_rounds is True
    with pytest.raises(SystemExit):
        cluster.parse_args(base + ["--device-rounds"])
    with pytest.raises(SystemExit):
        cluster.parse_args(base + ["--device-rounds", "--exact-small", "0"])
    tints, part0 = loop_tints()
    with pytest.raises(ValueError, match="device_rounds"):
        cluster.cluster_tints(tints, part0, None, dict(cluster.ilp_settings(), device_rounds=True))
