"""The scoring stage's launch list (freddie_amd/csrc/seg_score_plan.h) without a GPU: tools/score_plan_host_check.cpp, built with the
address and undefined-behaviour sanitizers and run as a child process, prints the list for a table of facts and plans; every list is
compared, in order and field by field, with the list written out here.  The expected lists were read out of the launch macros and the
three-pass plan interpreter that enqueue_run had before the header existed (the rules are restated beside each case)."""
import functools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = -1

# every class non-empty, a few wide problems per class, the hand-over arena laid out for all three lists and both counter widths
BASE = dict(known=1, fuse=1, tiny_on=1, wave=1, forking=1, wide_solve=1, key32=1, n_solve=(400, 120, 30), n_wide=(3, 2, 1), n_tiny=500,
            prob_cap=2000, split_dp=7, dpx_n=(400, 120, 30), dpx_cnt=(2, 2, 2), dpx_nm_fits=1, dpx_arena=1, split_grid_cap=1 << 20,
            wide_one_max=256)
DEFAULT = "gM|W|hB|gST"
OFF = (0, 1, (1, 0, 0, 0), (-1, -1, -1, -1), 0, 0)       # no plan: ScorePlan as constructed


def op(kind, cls, cnt=0, dpw=0, n=0, lane=MAIN):
    return (kind, cls, cnt, dpw, n, lane)


# the default plan's list: W opens its stream (pass 0), h and B theirs (pass 1), then the rest
DEFAULT_OPS = [op("wide_all", -1, 2, 0, 6, 0), op("gate_h", 2, n=6, lane=1), op("split", 2, 1, 512, 30, 1), op("gate_g", 2, n=36),
               op("split", 1, 1, 64, 120), op("gate_g", 2, n=36, lane=2), op("split", 0, 1, 64, 400, 2), op("wave", 3, n=500, lane=2)]
DEFAULT_PLAN = (1, 4, (1, 1, 1, 1), (-1, 0, 1, 2), 6, 1)


def swap(ops, at, new):
    return ops[:at] + [new] + ops[at + 1:]


# both instances of a class back to back (a plan without W, the chains without a plan): 8-bit over the list, 16-bit over its wide problems
def pair(cls, lane, kind="split"):
    dpw = 0 if kind == "fused" else (512 if cls == 2 else 64)
    return [op(kind, cls, 1, dpw, BASE["n_solve"][cls], lane), op(kind, cls, 2, dpw, BASE["n_wide"][cls], lane)]


NO_WIDE_OPS = [op("split", 2, 1, 512, 30, 0), op("gate_g", 2, n=30), op("split", 1, 1, 64, 120), op("gate_g", 2, n=30, lane=1),
               op("split", 0, 1, 64, 400, 1), op("wave", 3, n=500, lane=1)]
CHAINS_MAIN = pair(2, MAIN) + pair(1, MAIN) + pair(0, MAIN) + [op("wave", 3, n=500)]

CASES = {
    # 1. the default plan
    "default": (dict(BASE, plan=DEFAULT), DEFAULT_PLAN, DEFAULT_OPS),
    # 10. the DP keys' width picks the instance where an op is launched, not the op
    "default_key64": (dict(BASE, plan=DEFAULT, key32=0), DEFAULT_PLAN, DEFAULT_OPS),
    # 2. nothing for W: its segment is unused, hB takes side 0 and gST side 1, h has no workgroups to wait for
    "no_wide_problems": (dict(BASE, plan=DEFAULT, n_wide=(0, 0, 0)), (1, 4, (1, 0, 1, 1), (-1, -1, 0, 1), 0, 1), NO_WIDE_OPS),
    "wide_solve_off": (dict(BASE, plan=DEFAULT, wide_solve=0), (1, 4, (1, 0, 1, 1), (-1, -1, 0, 1), 6, 1), NO_WIDE_OPS),
    # 3. more wide problems than one launch takes: the classes' 16-bit instances, large then mid then small, on W's stream; h waits
    # for n_wide[2] workgroups, g for n_solve[2] + n_wide[2]
    "wide_per_class": (dict(BASE, plan=DEFAULT, n_wide=(200, 50, 7)), (1, 4, (1, 1, 1, 1), (-1, 0, 1, 2), 257, 0),
                       [op("split", 2, 2, 512, 7, 0), op("split", 1, 2, 64, 50, 0), op("split", 0, 2, 64, 200, 0), op("gate_h", 2, n=7, lane=1),
                        op("split", 2, 1, 512, 30, 1), op("gate_g", 2, n=37), op("split", 1, 1, 64, 120), op("gate_g", 2, n=37, lane=2),
                        op("split", 0, 1, 64, 400, 2), op("wave", 3, n=500, lane=2)]),
    # 4. plans without W: both instances of a class back to back; the gates wait for 30 + n_wide[2] workgroups
    "BM|gTS": (dict(BASE, plan="BM|gTS"), (1, 2, (1, 1, 0, 0), (-1, 0, -1, -1), 6, 0),
               pair(2, MAIN) + pair(1, MAIN) + [op("gate_g", 2, n=31, lane=0), op("wave", 3, n=500, lane=0)] + pair(0, 0)),
    "gM|B|gTS": (dict(BASE, plan="gM|B|gTS"), (1, 3, (1, 1, 1, 0), (-1, 0, 1, -1), 6, 0),
                 pair(2, 0) + [op("gate_g", 2, n=31)] + pair(1, MAIN) + [op("gate_g", 2, n=31, lane=1), op("wave", 3, n=500, lane=1)] + pair(0, 1)),
    "B|gM|gS|gT": (dict(BASE, plan="B|gM|gS|gT"), (1, 4, (1, 1, 1, 1), (-1, 0, 1, 2), 6, 0),
                   pair(2, MAIN) + [op("gate_g", 2, n=31, lane=0)] + pair(1, 0) + [op("gate_g", 2, n=31, lane=1)] + pair(0, 1) +
                   [op("gate_g", 2, n=31, lane=2), op("wave", 3, n=500, lane=2)]),
    # (a B behind a gate does not open its stream: everything in plan order, on main)
    "gBMTS": (dict(BASE, plan="gBMTS"), (1, 1, (1, 0, 0, 0), (-1, -1, -1, -1), 6, 0),
              [op("gate_g", 2, n=31)] + pair(2, MAIN) + pair(1, MAIN) + [op("wave", 3, n=500)] + pair(0, MAIN)),
    # 5. not a plan: the three chains (on the main stream: no arena-path kernels to run beside), the tiny kernel last
    "plan_0": (dict(BASE, plan="0"), OFF, CHAINS_MAIN),
    "plan_empty": (dict(BASE, plan=""), OFF, CHAINS_MAIN),
    "plan_four_bars": (dict(BASE, plan="B|M|S|g|T"), OFF, CHAINS_MAIN),
    "plan_class_twice": (dict(BASE, plan="gM|W|hB|gSTB"), OFF, CHAINS_MAIN),
    "plan_too_long": (dict(BASE, plan=DEFAULT + "g" * 21), OFF, CHAINS_MAIN),
    "not_forking": (dict(BASE, plan=DEFAULT, forking=0), OFF, CHAINS_MAIN),
    "no_large_class": (dict(BASE, plan=DEFAULT, n_solve=(400, 120, 0), n_wide=(3, 2, 0)), OFF,
                       pair(1, MAIN) + pair(0, MAIN) + [op("wave", 3, n=500)]),
    # ... beside arena-path work in a forking run: large on main, mid on side 0, small on side 1, k_score before k_solve, tiny on side 2
    "chains_forked": (dict(BASE, plan=DEFAULT, any_arena=1, n_cls_work=(50, 20, 5, 0)), OFF,
                      [op("score", 2)] + pair(2, MAIN) + [op("score", 1, lane=0)] + pair(1, 0) + [op("score", 0, lane=1)] + pair(0, 1) +
                      [op("wave", 3, n=500, lane=2)]),
    # (a class without arena work items has no k_score)
    "chains_forked_no_mid_work": (dict(BASE, plan=DEFAULT, any_arena=1, n_cls_work=(50, 0, 5, 0)), OFF,
                                  [op("score", 2)] + pair(2, MAIN) + pair(1, 0) + [op("score", 0, lane=1)] + pair(0, 1) +
                                  [op("wave", 3, n=500, lane=2)]),
    # 6. an empty mid class: its gate still launches, M emits nothing
    "empty_mid": (dict(BASE, plan=DEFAULT, n_solve=(400, 0, 30), n_wide=(3, 0, 1), dpx_n=(400, 0, 30)), (1, 4, (1, 1, 1, 1), (-1, 0, 1, 2), 4, 1),
                  [op("wide_all", -1, 2, 0, 4, 0), op("gate_h", 2, n=4, lane=1), op("split", 2, 1, 512, 30, 1), op("gate_g", 2, n=34),
                   op("gate_g", 2, n=34, lane=2), op("split", 0, 1, 64, 400, 2), op("wave", 3, n=500, lane=2)]),
    # 7. the split path refused: the class's bit off, a list beyond the grid cap, beyond what was laid out, counters wider than laid
    # out (asked with two bytes because the class has wide problems, though this launch starts the 8-bit instance only), no arena
    "split_bit_off": (dict(BASE, plan=DEFAULT, split_dp=5), DEFAULT_PLAN, swap(DEFAULT_OPS, 4, op("fused", 1, 1, 0, 120))),
    "split_bit_off_key64": (dict(BASE, plan=DEFAULT, split_dp=5, key32=0), DEFAULT_PLAN, swap(DEFAULT_OPS, 4, op("fused", 1, 1, 0, 120))),
    "split_grid_cap": (dict(BASE, plan=DEFAULT, split_grid_cap=399), DEFAULT_PLAN, swap(DEFAULT_OPS, 6, op("fused", 0, 1, 0, 400, 2))),
    "split_dpx_n": (dict(BASE, plan=DEFAULT, dpx_n=(399, 120, 30)), DEFAULT_PLAN, swap(DEFAULT_OPS, 6, op("fused", 0, 1, 0, 400, 2))),
    "split_dpx_cnt_wide_class": (dict(BASE, plan=DEFAULT, dpx_cnt=(2, 1, 2)), DEFAULT_PLAN, swap(DEFAULT_OPS, 4, op("fused", 1, 1, 0, 120))),
    "split_dpx_cnt_narrow_class": (dict(BASE, plan=DEFAULT, dpx_cnt=(2, 1, 2), n_wide=(3, 0, 3)), DEFAULT_PLAN, DEFAULT_OPS),
    "split_no_arena": (dict(BASE, plan=DEFAULT, dpx_arena=0), DEFAULT_PLAN,
                       swap(swap(swap(DEFAULT_OPS, 2, op("fused", 2, 1, 0, 30, 1)), 4, op("fused", 1, 1, 0, 120)), 6, op("fused", 0, 1, 0, 400, 2))),
    "split_other_nm": (dict(BASE, plan=DEFAULT, dpx_nm_fits=0), DEFAULT_PLAN,
                       swap(swap(swap(DEFAULT_OPS, 2, op("fused", 2, 1, 0, 30, 1)), 4, op("fused", 1, 1, 0, 120)), 6, op("fused", 0, 1, 0, 400, 2))),
    # ... and FSEG_SPLIT_DP bit 3: the large class's k_dpw by one wave a problem
    "split_dpw_64": (dict(BASE, plan=DEFAULT, split_dp=15), DEFAULT_PLAN, swap(DEFAULT_OPS, 2, op("split", 2, 1, 64, 30, 1))),
    # 8. list sizes unknown (then the arena path may have work): both instances of every class over prob_cap, whatever wide_solve says
    "unknown_small_batch": (dict(BASE, plan=DEFAULT, known=0, any_arena=1, small_batch=1, forking=0, wide_solve=0), OFF,
                            [op("score", -1), op("fused", -1, 1, 0, 2000), op("fused", -1, 2, 0, 2000), op("wave", 3, n=2000)]),
    "unknown_chains": (dict(BASE, plan=DEFAULT, known=0, any_arena=1, wide_solve=0), OFF,
                       [op("score", 2), op("fused", 2, 1, 0, 2000), op("fused", 2, 2, 0, 2000),
                        op("score", 1, lane=0), op("fused", 1, 1, 0, 2000, 0), op("fused", 1, 2, 0, 2000, 0),
                        op("score", 0, lane=1), op("fused", 0, 1, 0, 2000, 1), op("fused", 0, 2, 0, 2000, 1), op("wave", 3, n=2000, lane=2)]),
    # 9. a small batch, sized: one k_score for every class (with arena work) and the solve pair over the three lists together
    "small_batch_arena": (dict(BASE, plan=DEFAULT, small_batch=1, forking=0, any_arena=1, n_cls_work=(5, 2, 1, 0)), OFF,
                          [op("score", -1), op("fused", -1, 1, 0, 550), op("fused", -1, 2, 0, 550), op("wave", 3, n=500)]),
    "small_batch_solve_only": (dict(BASE, plan=DEFAULT, small_batch=1, forking=0, wide_solve=0), OFF,
                               [op("fused", -1, 1, 0, 550), op("wave", 3, n=500)]),
    # 11. the tiny problems' kernel
    "tiny_without_wave": (dict(BASE, plan=DEFAULT, wave=0), OFF, CHAINS_MAIN[:-1] + [op("tiny", 3, n=500)]),
    "tiny_off": (dict(BASE, plan=DEFAULT, forking=0, tiny_on=0), OFF, CHAINS_MAIN[:-1]),
    # (nothing goes to k_solve, nothing to the arena path of this sized batch: only the tiny problems' kernel is left)
    "fuse_off": (dict(BASE, plan=DEFAULT, fuse=0), OFF, [op("wave", 3, n=500)]),
    "no_problems": (dict(BASE, plan=DEFAULT, prob_cap=0), OFF, []),
}


def case_line(facts):
    return " ".join("%s=%s" % (k, ",".join(map(str, v)) if isinstance(v, tuple) else v) for k, v in facts.items())


def run_tool(lines, tmp):
    exe = os.path.join(str(tmp), "score_plan_host_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "freddie_amd", "csrc"), os.path.join(ROOT, "tools", "score_plan_host_check.cpp"), "-o", exe])
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    out, plan, ops = [], None, []
    for line in res.stdout.splitlines():
        w = line.split()
        if w[0] == "plan":
            v = [int(x) for x in w[1:]]
            plan = (v[0], v[1], tuple(v[2:6]), tuple(v[6:10]), v[10], v[11])
        elif w[0] == "op":
            ops.append((w[1],) + tuple(int(x) for x in w[2:]))
        else:
            out.append((plan, ops))
            plan, ops = None, []
    return out


@functools.lru_cache(maxsize=None)
def results(tmp):
    names = list(CASES)
    got = run_tool([case_line(CASES[n][0]) for n in names] + [case_line(dict(BASE, plan="BMST" + "W" * 27, n_wide=(200, 50, 7)))], tmp)
    assert len(got) == len(names) + 1
    return dict(zip(names + ["longest"], got))


@pytest.fixture(scope="module")
def tool_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("score_plan")


@pytest.mark.parametrize("name", list(CASES))
def test_launch_list(name, tool_dir):
    _, want_plan, want_ops = CASES[name]
    got_plan, got_ops = results(tool_dir)[name]
    assert got_plan == want_plan
    assert got_ops == want_ops


def test_default_plan_census(tool_dir):
    """What the census words (include/freddie_seg.h: a bit per class, 8 for a launch over every class; FSEG_TAP_PATHS' dpw: 8 for the
    512-thread k_dpw) come to for the default plan's list: solve8 = 7, wide16 = 8, dpw = 15."""
    _, ops = results(tool_dir)["default"]
    solve8 = wide16 = dpw = 0
    for kind, cls, cnt, threads, _, _ in ops:
        if kind in ("fused", "split", "wide_all"):
            bit = 8 if cls < 0 else 1 << cls
            solve8, wide16 = (solve8 | bit, wide16) if cnt == 1 else (solve8, wide16 | bit)
        if kind == "split":
            dpw |= (1 << cls) | (8 if threads == 512 else 0)
    assert (solve8, wide16, dpw) == (7, 8, 15)


def test_longest_plan_fits_the_list(tool_dir):
    """31 characters, 27 of them a W that launches three instances each: 4 + 81 launches, below the list's capacity of 3 * 31."""
    plan, ops = results(tool_dir)["longest"]
    assert plan[0] == 1 and len(ops) == 85
    assert ops[:4] == [("split", 2, 1, 512, 30, MAIN), ("split", 1, 1, 64, 120, MAIN), ("split", 0, 1, 64, 400, MAIN), ("wave", 3, 0, 0, 500, MAIN)]
    assert ops[4:] == 27 * [("split", 2, 2, 512, 7, MAIN), ("split", 1, 2, 64, 50, MAIN), ("split", 0, 2, 64, 200, MAIN)]
