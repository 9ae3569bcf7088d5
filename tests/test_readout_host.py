"""The round read-out without a GPU: the numpy mirror of the kernels' word arithmetic (cluster_prep.readout_words / readout_mirror) against
the definition, cluster.read_out(), on every feasible set of the grid's problems and on the shapes of the GPU test; named one-rule
mutations of the mirror, each of which a named case catches; and the kernels' own per-thread code (freddie_amd/csrc/clu_readout.h)
compiled for the host with sanitizers and compared with the mirror word by word."""
import os
import subprocess
import sys

import numpy as np
import pytest

import round_util as ru
from freddie_amd import cluster, cluster_prep
from test_incumbent_host import grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import readout_host_check as rc  # noqa: E402


def definition(tint, remaining, members, inf=None):
    """cluster.read_out() of the set, with e as the model defines it: the OR of the members' I bits on the informative segments.  inf: an
    informative row of the caller's in place of informative_segs()'s."""
    inf = ru.informative_segs(tint, remaining) if inf is None else inf
    inf_seg = [j for j, v in enumerate(inf) if v]
    I = tint["ilp_data"]["I"]
    e = [int(any(I[remaining[c]][j] for c in members)) for j in inf_seg]
    x = [int(c in set(members)) for c in range(len(remaining))]
    return cluster.read_out(tint, remaining, dict(inf_seg=inf_seg), x, e), e, inf


def mirrored(tint, remaining, members, inf, rule=None):
    out = cluster_prep.readout_mirror([tint], [(0, remaining)], [members], [[int(v) for v in inf]], rule)
    return cluster_prep.readout_isoform(out, 0, remaining)


def test_mirror_is_read_out_on_every_feasible_set_of_the_grid():
    checked = 0
    for tint, incomp, remaining, feasible in grid():
        M = len(tint["segs"])
        inf = ru.informative_segs(tint, remaining)
        I, C, labels = cluster_prep.readout_rows(tint, remaining)
        inf_w = cluster_prep._pack_bits([[int(v) for v in inf]], M)[0]
        for mask in feasible:
            members = [c for c in range(len(remaining)) if mask >> c & 1]
            if not members:
                continue
            want, e, _ = definition(tint, remaining, members)
            ex, corr = cluster_prep.readout_words(I, C, labels, inf_w, members, M)
            exons = [(int(ex[j >> 5]) >> (j & 31)) & 1 for j in range(M)]
            assert exons == want["exons"], (tint["id"], mask)
            assert [exons[j] for j in range(M) if inf[j]] == e
            for k, c in enumerate(members):
                assert list(bytes(corr[k].tolist()).decode("ascii")) == want["rid_to_corrections"][remaining[c]], (tint["id"], mask, c)
            checked += 1
    assert checked == 51649


def test_mirror_is_read_out_on_the_shapes():
    """Every tint of the GPU test's shapes as one problem, under every set variant; the flat arrays and what readout_isoform() cuts out."""
    seen = set()
    for tint, remaining, members, inf in rc.host_problems():
        got = mirrored(tint, remaining, members, inf)
        if not members:
            assert got is None
            continue
        want, e, _ = definition(tint, remaining, members)
        assert got[0]["exons"] == want["exons"] and got[1] == e, tint["id"]
        assert got[0]["rid_to_corrections"] == want["rid_to_corrections"], tint["id"]
        assert list(got[0]["rid_to_corrections"]) == [remaining[c] for c in members]
        seen.add(len(tint["segs"]))
    assert seen >= set(rc.SEGMENTS) | {rc.WIDEST}


def crafted():
    rows, polys = rc.crafted_rows()
    tint = ru.make_tint(0, rows, {}, polys)
    cluster_prep.preprocess_ilp(tint, dict(recycle_model="constant"))
    return tint


# a named case = (remaining reps of the hand-built tint, accepted columns); each mutation names the case that must catch it
CASES = {
    "column_0_not_a_member": ([5, 0, 2], [1, 2]),            # rep 5 (zeros at 0 .. 2) is column 0 only; with informative_segs()' own row an
                                                             # uninformative segment is constant over the columns, so the case hands in a row
                                                             # of its own in which 0 .. 2 are not informative: read_out() takes inf_seg as given
    "c_bit_without_exon_bit": ([0, 2, 5], [1]),              # rep 2 alone: its 0 at 20 is a C bit and the exon bit there is 0
    "label_2_and_dashes": ([0, 1, 2], [0, 1]),               # rep 1: a 2 on the informative 10 and on the uninformative 11
    "thirty_three_segments": None,                           # (built below: the last word holds one segment)
}
MUTATIONS = {"first_member": "column_0_not_a_member", "x_without_exon": "c_bit_without_exon_bit", "no_dash": "label_2_and_dashes",
             "label2_as_0": "label_2_and_dashes", "no_tail_mask": "thirty_three_segments"}


def named_case(name):
    """(tint, remaining, members, informative row or None for informative_segs()')"""
    if name == "thirty_three_segments":
        tint = ru.make_tint(1, [[1] * 33, [1] * 32 + [0], [0] + [1] * 32])
        cluster_prep.preprocess_ilp(tint, dict(recycle_model="constant"))
        return tint, [0, 1, 2], [0, 1], None
    inf = [j > 2 for j in range(40)] if name == "column_0_not_a_member" else None
    return (crafted(),) + CASES[name] + (inf,)


def test_the_named_cases_hold_what_they_name():
    tint, remaining, members, inf = named_case("column_0_not_a_member")
    want, _, inf = definition(tint, remaining, members, inf)
    I = tint["ilp_data"]["I"]
    assert I[5][0:3] == [0, 0, 0] and I[0][0:3] == [1, 1, 1] and want["exons"][0:3] == [0, 0, 0] and want["exons"][3] == 1
    tint, remaining, members, _ = named_case("c_bit_without_exon_bit")
    want, _, inf = definition(tint, remaining, members)
    assert tint["ilp_data"]["C"][2][20] == 1 and inf[20] and want["exons"][20] == 0 and want["rid_to_corrections"][2][20] == "0"
    both, _, _ = definition(tint, remaining, [0, 1])
    assert both["exons"][20] == 1 and both["rid_to_corrections"][2][20] == "X"           # ... and beside rep 0 the exon bit is 1
    tint, remaining, members, _ = named_case("label_2_and_dashes")
    want, _, inf = definition(tint, remaining, members)
    assert inf[10] and not inf[11] and want["rid_to_corrections"][1][10] == "2" and want["rid_to_corrections"][1][11] == "-"
    C = tint["ilp_data"]["C"]                                                           # FL: the tails widen C, the same zeros without one stay 0
    assert C[3][0:3] == [1, 1, 1] and C[4][36:40] == [1, 1, 1, 1] and C[5][0:3] == [0, 0, 0]


@pytest.mark.parametrize("rule", sorted(MUTATIONS))
def test_a_mutation_changes_its_named_case(rule):
    tint, remaining, members, inf = named_case(MUTATIONS[rule])
    want, e, inf = definition(tint, remaining, members, inf)
    assert mirrored(tint, remaining, members, inf) == (want, e)
    if rule == "no_tail_mask":           # the bits behind M: an informative word that holds some must not reach the exon word, nor e
        M = len(tint["segs"])
        I, C, labels = cluster_prep.readout_rows(tint, remaining)
        dirty = cluster_prep._pack_bits([[int(v) for v in inf]], M)[0] | np.array([0, 0xfffffffe], np.uint32)
        I[:, 1] |= np.uint32(0xfffffff0)
        clean = cluster_prep.readout_words(I, C, labels, dirty, members, M)
        broken = cluster_prep.readout_words(I, C, labels, dirty, members, M, rule)
        assert int(clean[0][1]) >> 1 == 0 and int(broken[0][1]) >> 1 != 0
        return
    assert mirrored(tint, remaining, members, inf, rule) != (want, e)


def test_round_model_refuses_a_resident_result():
    arr = dict(resident=True, refused=np.array([-1], np.int32))
    with pytest.raises(cluster_prep.ClusterError, match="stayed on the device"):
        cluster_prep.round_model(arr, 0)


def test_exports_name_the_new_entry_points():
    for name in ("fclu_round_models_resident", "fclu_round_readout", "fclu_round_readout_results", "fclu_round_readout_timing"):
        assert name in cluster_prep.EXPORTS


def test_kernel_bodies_on_the_host():
    """What one lane of k_readout_exons / k_readout_corr computes (freddie_amd/csrc/clu_readout.h), compiled for the host with the address
    and undefined-behaviour sanitizers, against the mirror word by word: random rows, every row offset 0 .. 17, and the shapes."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "readout_host_check.py"), "--cases", "150"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and " 0 differ" in res.stdout, res.stdout + res.stderr
