"""The upload's host plan (freddie_amd/csrc/seg_upload_plan.h) and the reaction to a run's status record (seg_run_react.h) without
a GPU: tools/upload_plan_host_check.cpp, built with the address and undefined-behaviour sanitizers and run as a child process.

Plan and tables: the program allocates every table at exactly the plan's count (a write past it ends the program), and what it prints
is compared with a restatement per POSITION: one loop over the batch's positions says which tile, histogram chunk and compaction
block each lies in -- no ceil-divisions, no cursors, nothing of the header's arithmetic.  The batches are the smallest that reach
each edge (tile, chunk, rep block, compaction block, the 16-bit counters' limit).

Reaction: what every status bit gives under each kind of run, written out here as read off finish_run_impl and run_sized before
the two shared one function."""
import functools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE, POS_BLOCK, REP_BLOCK, COUNT_MAX16 = 512, 32768, 256, 65535
ARG, INPUT, UNSUPPORTED = 1, 3, 4


def batch(parts, hist16=1, yraw16=1):
    """parts: [(intervals [(start, end)], reps [(weight, exons [(ts, te)])])] -> the flat arrays of fseg_batch"""
    b = dict(part_iv_off=[0], iv_start=[], iv_end=[], part_rep_off=[0], rep_weight=[], rep_exon_off=[0], ex_ts=[], ex_te=[], hist16=hist16, yraw16=yraw16)
    for ivs, reps in parts:
        b["iv_start"] += [s for s, _ in ivs]
        b["iv_end"] += [e for _, e in ivs]
        b["part_iv_off"].append(len(b["iv_start"]))
        for w, exons in reps:
            b["rep_weight"].append(w)
            b["ex_ts"] += [s for s, _ in exons]
            b["ex_te"] += [e for _, e in exons]
            b["rep_exon_off"].append(len(b["ex_ts"]))
        b["part_rep_off"].append(len(b["rep_weight"]))
    return b


def iv_of(n, start=100):
    return (start, start + n - 1)         # an interval owns start .. end inclusive


def reps(n, weight=1, exon=(100, 101)):
    return [(weight, [exon])] * n


ONE = ([iv_of(2)], reps(1))
BATCHES = {
    # start < end: two positions are the least an interval can own (the one-position interval is among the refusals)
    "smallest": batch([ONE]),
    "tile_minus_equal_plus": batch([([iv_of(TILE - 1, 0), iv_of(TILE, 1000), iv_of(TILE + 1, 2000)], reps(2))]),
    # few positions: the chunks are halved down to 1024 positions
    "chunk_minus_equal_plus": batch([([iv_of(1023)], reps(1)), ([iv_of(1024)], reps(1)), ([iv_of(1025)], reps(3, 2))]),
    "chunk_spans_three_intervals": batch([([iv_of(500, 0), iv_of(100, 1000), iv_of(500, 2000), iv_of(30, 3000)], reps(1))]),
    "chunk_ends_with_interval": batch([([iv_of(1024, 0), iv_of(10, 5000)], reps(1)), ([iv_of(2048, 0), iv_of(2, 5000)], reps(1))]),
    "rep_blocks": batch([([iv_of(5)], reps(255)), ([iv_of(5)], reps(256)), ([iv_of(5)], reps(257)), ([iv_of(5)], [])]),
    "pos_block_equal": batch([([iv_of(POS_BLOCK - 10, 0), iv_of(10, 40000)], reps(1))]),
    "pos_block_plus": batch([([iv_of(POS_BLOCK - 10, 0), iv_of(11, 40000)], reps(1))]),
    "pos_block_starts_interval": batch([([iv_of(POS_BLOCK, 0), iv_of(2, 40000)], reps(1)), ONE]),
    # 2 * 32 767 hits cannot overflow a 16-bit counter: not counted; 32 768 lanes are, and their ends do not coincide
    "lanes_32767": batch([([iv_of(100)], [(32767, [(100, 150), (150, 199)])])]),
    "lanes_32768": batch([([iv_of(100)], [(32768, [(100, 150), (160, 199)])])]),
    # ... the most exon ends on one coordinate: 40 000 + 25 535 = 65 535 at 150 keeps the packed counters, one more read does not
    "ends_65535": batch([ONE, ([iv_of(100)], [(40000, [(100, 150)]), (25535, [(150, 199)]), (7, [(120, 130)])])]),
    "ends_65536": batch([ONE, ([iv_of(100)], [(40000, [(100, 150)]), (25536, [(150, 199)]), (7, [(120, 130)])])]),
    "ends_65536_twice_by_one_rep": batch([([iv_of(100)], [(32768, [(100, 150), (150, 199)])])]),
    "hist16_off": batch([ONE, ([iv_of(3000)], reps(3))], hist16=0),
    "yraw16_off": batch([ONE, ([iv_of(3000)], reps(3))], yraw16=0),
}

REFUSALS = {
    "iv_off_from_1": (dict(batch([ONE]), part_iv_off=[1, 1]), ARG, "fseg_upload: offsets must start at 0"),
    "rep_off_from_1": (dict(batch([ONE]), part_rep_off=[1, 1]), ARG, "fseg_upload: offsets must start at 0"),
    "exon_off_from_1": (dict(batch([ONE]), rep_exon_off=[1, 1]), ARG, "fseg_upload: offsets must start at 0"),
    "no_intervals_at_all": (dict(batch([ONE]), part_iv_off=[0, 0]), ARG, "fseg_upload: bad offsets"),
    "negative_reps": (dict(batch([ONE]), part_rep_off=[0, -1]), ARG, "fseg_upload: bad offsets"),
    "negative_exons": (dict(batch([ONE]), rep_exon_off=[0, -1]), ARG, "rep_exon_off not monotone"),
    "too_many_exons": (dict(batch([ONE]), rep_exon_off=[0, 2**31 - 1]), UNSUPPORTED, "batch has 2147483647 exons; split it (limit 2^31-1 per upload)"),
    "empty_partition": (dict(batch([ONE, ONE]), part_iv_off=[0, 0, 2]), INPUT, "partition 0 has no intervals"),
    "rep_off_descends": (dict(batch([([iv_of(2)], reps(2)), ONE, ONE]), part_rep_off=[0, 3, 2, 4]), ARG, "part_rep_off not monotone"),
    "one_position_interval": (batch([ONE, ([(7, 7)], reps(1))]), INPUT, "partition 1: interval with start >= end (py/freddie_segment.py:140)"),
    "intervals_touch": (batch([([(0, 9), (9, 20)], reps(1))]), INPUT, "partition 0: intervals overlap or are unordered (py/freddie_segment.py:138)"),
    "intervals_unordered": (batch([ONE, ONE, ([(50, 60), (10, 20)], reps(1))]), INPUT, "partition 2: intervals overlap or are unordered (py/freddie_segment.py:138)"),
    "too_many_positions": (batch([([(-2**30, 2**30 - 2)], reps(1))]), UNSUPPORTED, "batch has 2147483647 positions; split it (limit 2^31-1 per upload)"),
    "weight_0": (batch([([iv_of(2)], [(1, [(100, 101)]), (0, [(100, 101)])])]), INPUT, "rep 1 has weight 0 (< 1)"),
    "exon_off_descends": (dict(batch([([iv_of(2)], reps(3))]), rep_exon_off=[0, 2, 1, 3]), ARG, "rep_exon_off not monotone"),
    "too_many_reads": (batch([([iv_of(2)], reps(1, 2**30) + reps(1, 2**30 - 1))]), UNSUPPORTED, "batch has 2147483647 reads; split it (limit 2^31-1 per upload)"),
    # ("batch too large", the refusal of 2^31 - 1 tiles or chunks, cannot be reached: every tile and chunk holds a position, and that
    # many positions are refused before)
}


def restate(b):
    """What the plan and the tables must be, position by position."""
    K, n_part = len(b["iv_start"]), len(b["part_iv_off"]) - 1
    part_of_iv = [p for p in range(n_part) for _ in range(b["part_iv_off"][p], b["part_iv_off"][p + 1])]
    NPOS = sum(e - s + 1 for s, e in zip(b["iv_start"], b["iv_end"]))
    weights = np.array(b["rep_weight"], dtype=np.int64)
    lanes = [int(weights[b["part_rep_off"][p]:b["part_rep_off"][p + 1]].sum()) for p in range(n_part)]
    most_ends = 0
    for p in range(n_part):
        hits = {}
        for r in range(b["part_rep_off"][p], b["part_rep_off"][p + 1]):
            for e in range(b["rep_exon_off"][r], b["rep_exon_off"][r + 1]):
                for x in (b["ex_ts"][e], b["ex_te"][e]):
                    hits[x] = hits.get(x, 0) + b["rep_weight"][r]
        most_ends = max([most_ends] + list(hits.values()))
    packed = bool(b["hist16"]) and most_ends <= COUNT_MAX16
    chunk = 16384 if packed else 8192
    while chunk > 1024 and NPOS // chunk < 512:
        chunk //= 2
    pos_off, iv_tile0, tiles, blk_iv0, chunks, part_pos = [], [], [], [], [], [0] * n_part
    q = 0
    for k in range(K):
        p, length = part_of_iv[k], b["iv_end"][k] - b["iv_start"][k] + 1
        pos_off.append(q)
        for y in range(length):
            if y == 0:
                iv_tile0.append(len(tiles))
            if y % TILE == 0:
                tiles.append((pos_off[k], y, length))
            if q % POS_BLOCK == 0:
                blk_iv0.append(k)
            if part_pos[p] % chunk == 0:
                chunks.append([p, q, 0, b["iv_start"][k] + y, None])
            chunks[-1][2] += 1
            chunks[-1][4] = b["iv_start"][k] + y
            part_pos[p] += 1
            q += 1
    assert q == NPOS
    rb = [(p, r) for p in range(n_part) for r in range(b["part_rep_off"][p], b["part_rep_off"][p + 1]) if (r - b["part_rep_off"][p]) % REP_BLOCK == 0]
    n_exons = np.diff(np.array(b["rep_exon_off"], dtype=np.int64))
    n_reps = np.diff(np.array(b["part_rep_off"], dtype=np.int64))
    facts = [n_part, K, len(weights), len(b["ex_ts"]), NPOS, sum(lanes), max(part_pos), max(lanes), len(tiles), len(chunks), len(rb),
             int(n_exons.max()) if len(n_exons) else 0, int((weights != 1).any()), int(packed), int(packed and bool(b["yraw16"]))]
    nbp = len(blk_iv0)
    return {
        "facts": facts, "more": [int(n_reps.max()), chunk, -(-NPOS // 8192), nbp],
        "counts": [n_part + 1, K, K + 1, len(tiles), nbp + 1, len(rb), len(chunks)],
        "part_pos": part_pos, "part_lanes": lanes,
        "pos_off": pos_off + [NPOS], "part_lane_off": [0] + list(np.cumsum(lanes)), "iv_part": part_of_iv, "iv_tile0": iv_tile0,
        "tile_desc": tiles, "blk_iv0": blk_iv0 + [K - 1], "rb_part": [p for p, _ in rb], "rb_r0": [r for _, r in rb],
        "hc_part": [c[0] for c in chunks], "hc_p0": [c[1] for c in chunks], "hc_n": [c[2] for c in chunks],
        "hc_glo": [c[3] for c in chunks], "hc_ghi": [c[4] for c in chunks],
    }


# ---- the reaction to a status record
BITS = dict(exon_interval=1, break_assert=2, problem_too_large=4, overflow_pairs=8, overflow_tri=16, overflow_work=32, overflow_labels=64,
            overflow_problems=128, overflow_chunks=256, overflow_cov=512, overflow_nm=1024, need_wide_dp=2048, scan_stall=4096, wave_stage=8192,
            wide_missed=16384, sync_timeout=32768)
CAPS = (1000,) * 7          # problems, work items, pairs, triples, label bytes, chunks, coverage
QUIET = dict(err=0, n_prob=10, n_work=10, pair_used=10, tri_used=10, label_bytes=10, n_vchunks=10, cov_used=10, max_n=20, max_ln=100, dp_huge=0,
             have_huge=0, dp_wide_counts=0, run_events_only=0, nm_giant=0, cap=CAPS)
NOTHING = dict(outcome="done", fail="none", attempt=1, scan_fallback=0, wave_off=0, sync_timeout=0, nm_big_max=0, have_huge=0, dp_wide_counts=0, giant=0,
               adopt_counts=0, cap=CAPS)
# a record that asks for nothing: piece A takes the sizes over (and always sizes the giant kernels' scratch: prepare_giant also
# turns it off), piece B goes on to the labels, a whole run is complete
CLEAN = {"A": dict(NOTHING, giant=1, adopt_counts=1), "B": NOTHING, "R": dict(NOTHING, adopt_counts=1)}
INPUT_FAIL = {"A": dict(NOTHING, outcome="fail", fail="input"), "B": dict(NOTHING, outcome="fail", fail="input"),
              "R": dict(NOTHING, outcome="fail", fail="input", adopt_counts=1)}     # (a whole run that ends with an input error has run: its sizes are taken)
SIZED_OVERFLOW = dict(NOTHING, outcome="fail", fail="sized_overflow")
REDO = dict(NOTHING, outcome="redo")
# an overflow bit: piece A writes into no arena (the bit cannot be its own), piece B's capacities were exact, a whole run goes again
# (the counts stay below the capacities here: nothing grows)
OVERFLOW = {"A": CLEAN["A"], "B": SIZED_OVERFLOW, "R": REDO}
STALL = {k: dict(REDO, scan_fallback=1) for k in "ABR"}


def grown(i, v=2000):
    return CAPS[:i] + (v,) + CAPS[i + 1:]


REACTIONS = {("quiet", k): (QUIET, CLEAN[k]) for k in "ABR"}
for name in ("exon_interval", "break_assert", "problem_too_large"):
    REACTIONS.update({(name, k): (dict(QUIET, err=BITS[name]), INPUT_FAIL[k]) for k in "ABR"})
for name in ("overflow_pairs", "overflow_tri", "overflow_work", "overflow_problems", "overflow_chunks", "overflow_cov"):
    REACTIONS.update({(name, k): (dict(QUIET, err=BITS[name]), OVERFLOW[k]) for k in "ABR"})
REACTIONS.update({
    # the label arena is sized after piece B: its bit is no overflow there
    ("overflow_labels", "A"): (dict(QUIET, err=64), CLEAN["A"]), ("overflow_labels", "B"): (dict(QUIET, err=64), CLEAN["B"]),
    ("overflow_labels", "R"): (dict(QUIET, err=64), REDO),
    ("overflow_nm", "A"): (dict(QUIET, err=1024), CLEAN["A"]), ("overflow_nm", "B"): (dict(QUIET, err=1024), SIZED_OVERFLOW),
    ("overflow_nm", "R"): (dict(QUIET, err=1024), dict(REDO, nm_big_max=1)),
    # a whole run goes by the record's widest problem, not by the bit
    ("need_wide_dp", "A"): (dict(QUIET, err=2048), CLEAN["A"]), ("need_wide_dp", "B"): (dict(QUIET, err=2048), SIZED_OVERFLOW),
    ("need_wide_dp", "R"): (dict(QUIET, err=2048), CLEAN["R"]),
    ("wave_stage", "A"): (dict(QUIET, err=8192), CLEAN["A"]), ("wave_stage", "B"): (dict(QUIET, err=8192), dict(REDO, wave_off=1)),
    ("wave_stage", "R"): (dict(QUIET, err=8192), dict(REDO, wave_off=1)),
    # piece A has not looked at what the problems keep
    ("wide_missed", "A"): (dict(QUIET, err=16384), CLEAN["A"]), ("wide_missed", "B"): (dict(QUIET, err=16384), INPUT_FAIL["B"]),
    ("wide_missed", "R"): (dict(QUIET, err=16384), INPUT_FAIL["R"]),
    # a time-out: once more with events -- not one of the sized run's attempts, one of the whole run's
    ("sync_timeout", "A"): (dict(QUIET, err=32768), CLEAN["A"]), ("sync_timeout", "B"): (dict(QUIET, err=32768), dict(REDO, sync_timeout=1, attempt=0)),
    ("sync_timeout", "R"): (dict(QUIET, err=32768), dict(REDO, sync_timeout=1)),
    ("sync_timeout_without_waiters", "B"): (dict(QUIET, err=32768, run_events_only=1), dict(NOTHING, outcome="fail", fail="timeout_no_waiters")),
    ("sync_timeout_without_waiters", "R"): (dict(QUIET, err=32768, run_events_only=1), dict(NOTHING, outcome="fail", fail="timeout_no_waiters")),
    # what is no bit: a huge problem, a giant one, a problem that sees 65 536 reads, a count above its capacity
    ("huge", "A"): (dict(QUIET, dp_huge=3), dict(CLEAN["A"], have_huge=1)), ("huge", "B"): (dict(QUIET, dp_huge=3), CLEAN["B"]),
    ("huge", "R"): (dict(QUIET, dp_huge=3), dict(REDO, have_huge=1)),
    ("huge_already", "R"): (dict(QUIET, dp_huge=3, have_huge=1), dict(CLEAN["R"], have_huge=1)),
    ("huge_gone", "A"): (dict(QUIET, have_huge=1), CLEAN["A"]), ("huge_gone", "R"): (dict(QUIET, have_huge=1), dict(CLEAN["R"], have_huge=1)),
    ("giant", "A"): (dict(QUIET, max_n=200), CLEAN["A"]), ("giant", "B"): (dict(QUIET, max_n=200), CLEAN["B"]),
    ("giant", "R"): (dict(QUIET, max_n=200), dict(REDO, giant=1)),
    ("giant_sized_for", "R"): (dict(QUIET, max_n=200, nm_giant=200), CLEAN["R"]),
    ("giant_128", "R"): (dict(QUIET, max_n=128), CLEAN["R"]), ("giant_1024", "R"): (dict(QUIET, max_n=1024), dict(REDO, giant=1)),
    ("giant_1025", "R"): (dict(QUIET, max_n=1025), CLEAN["R"]),
    ("wide_counts", "A"): (dict(QUIET, max_ln=65536), dict(CLEAN["A"], dp_wide_counts=1)), ("wide_counts", "B"): (dict(QUIET, max_ln=65536), CLEAN["B"]),
    ("wide_counts", "R"): (dict(QUIET, max_ln=65536), dict(REDO, dp_wide_counts=1)),
    ("wide_counts_65535", "R"): (dict(QUIET, max_ln=65535), CLEAN["R"]),
    ("wide_counts_already", "R"): (dict(QUIET, max_ln=65536, dp_wide_counts=1), dict(CLEAN["R"], dp_wide_counts=1)),
    ("wide_counts_gone", "A"): (dict(QUIET, dp_wide_counts=1), CLEAN["A"]),
    # capacities: piece A makes them at least the counts, a whole run adds an eighth and 64
    ("more_problems", "A"): (dict(QUIET, n_prob=2000), dict(CLEAN["A"], cap=grown(0))), ("more_problems", "B"): (dict(QUIET, n_prob=2000), CLEAN["B"]),
    ("more_problems", "R"): (dict(QUIET, n_prob=2000), dict(REDO, cap=grown(0, 2314))),
    ("more_of_all", "A"): (dict(QUIET, n_prob=2000, n_work=2001, pair_used=2002, tri_used=2003, label_bytes=2004, n_vchunks=2005, cov_used=2006),
                           dict(CLEAN["A"], cap=(2000, 2001, 2002, 2003, 1000, 1000, 2006))),
    ("more_of_all", "R"): (dict(QUIET, n_prob=2000, n_work=2001, pair_used=2002, tri_used=2003, label_bytes=2004, n_vchunks=2005, cov_used=2006),
                           dict(REDO, cap=(2314, 2315, 2316, 2317, 2318, 1000, 2320))),
    ("as_many_as_fit", "R"): (dict(QUIET, n_prob=1000, label_bytes=1000), CLEAN["R"]),
    ("more_chunks", "R"): (dict(QUIET, n_vchunks=2000), REDO),
    # what occurs together: a sized piece reacts to the first, a whole run to all
    ("stall_with_overflow", "A"): (dict(QUIET, err=4096 | 8), STALL["A"]), ("stall_with_overflow", "B"): (dict(QUIET, err=4096 | 8), STALL["B"]),
    ("stall_with_overflow", "R"): (dict(QUIET, err=4096 | 8, pair_used=2000), dict(STALL["R"], cap=grown(2, 2314))),
    ("timeout_with_wave_stage", "A"): (dict(QUIET, err=32768 | 8192), CLEAN["A"]),
    ("timeout_with_wave_stage", "B"): (dict(QUIET, err=32768 | 8192), dict(REDO, sync_timeout=1, attempt=0)),
    ("timeout_with_wave_stage", "R"): (dict(QUIET, err=32768 | 8192), dict(REDO, sync_timeout=1, wave_off=1)),
    ("huge_with_giant", "A"): (dict(QUIET, dp_huge=1, max_n=200), dict(CLEAN["A"], have_huge=1)),
    ("huge_with_giant", "B"): (dict(QUIET, dp_huge=1, max_n=200), CLEAN["B"]),
    ("huge_with_giant", "R"): (dict(QUIET, dp_huge=1, max_n=200), dict(REDO, have_huge=1, giant=1)),
    ("input_error_with_overflow", "R"): (dict(QUIET, err=1 | 16), REDO),          # (grown and run again first: the error is reported by the run that fits)
})
REACTIONS.update({("scan_stall", k): (dict(QUIET, err=4096), STALL[k]) for k in "ABR"})


def test_every_bit_under_every_kind():
    for name in BITS:
        for kind in "ABR":
            assert (name, kind) in REACTIONS


# ---- the tool
def batch_lines(b):
    lines = ["batch hist16=%d yraw16=%d" % (b["hist16"], b["yraw16"])]
    for name in ("part_iv_off", "iv_start", "iv_end", "part_rep_off", "rep_weight", "rep_exon_off", "ex_ts", "ex_te"):
        lines.append("%s %s" % (name, ",".join(str(v) for v in b[name])))
    return lines + ["end"]


def react_line(kind, given):
    return "react kind=%s " % kind + " ".join("%s=%s" % (k, ",".join(map(str, v)) if isinstance(v, tuple) else v) for k, v in given.items())


@functools.lru_cache(maxsize=None)
def results(tmp):
    exe = os.path.join(str(tmp), "upload_plan_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "freddie_amd", "csrc"), os.path.join(ROOT, "tools", "upload_plan_host_check.cpp"), "-o", exe], check=True)
    batches = {**BATCHES, **{n: r[0] for n, r in REFUSALS.items()}}
    lines = [l for b in batches.values() for l in batch_lines(b)] + [react_line(k[1], v[0]) for k, v in REACTIONS.items()]
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "", p.stderr[-3000:]          # the sanitizers write to stderr
    out, plans, reactions = p.stdout.splitlines(), [], []
    cur = None
    for line in out:
        w = line.split(" ")
        if w[0] == "plan":
            cur = {"rc": int(w[1]), "msg": line.split(" ", 2)[2]}
        elif w[0] == "end":
            plans.append(cur)
        elif w[0] == "reaction":
            r = dict(outcome=w[1], fail=w[2])
            for kv in w[3:]:
                k, v = kv.split("=")
                r[k] = tuple(int(x) for x in v.split(",")) if k == "cap" else int(v)
            reactions.append(r)
        elif w[0] == "tile_desc":
            cur[w[0]] = [tuple(int(x) for x in t.split(":")) for t in w[1:]]
        else:
            cur[w[0]] = [int(x) for x in w[1:]]
    assert len(plans) == len(batches) and len(reactions) == len(REACTIONS)
    return dict(zip(batches, plans)), dict(zip(REACTIONS, reactions))


@pytest.fixture(scope="module")
def tool_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("upload_plan")


@pytest.mark.parametrize("name", list(BATCHES))
def test_plan_and_tables(name, tool_dir):
    got = dict(results(tool_dir)[0][name])
    assert (got.pop("rc"), got.pop("msg")) == (0, "")
    want = restate(BATCHES[name])
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == [int(v) if not isinstance(v, tuple) else v for v in want[key]], key


def test_the_batches_reach_their_edges(tool_dir):
    """The cases are what their names say (from the tool's own output: a case that missed its edge would check nothing)."""
    got = results(tool_dir)[0]
    facts = lambda n: dict(zip(("n_part K R I NPOS LANES max_part_pos max_part_lanes n_tiles n_hist_chunks n_rep_blocks max_rep_exons expanded hist_packed "
                                "yraw_narrow").split(), got[n]["facts"]))
    assert [t[2] for t in got["tile_minus_equal_plus"]["tile_desc"]] == [511, 512, 513, 513]
    assert got["chunk_minus_equal_plus"]["more"][1] == 1024 and got["chunk_minus_equal_plus"]["hc_n"] == [1023, 1024, 1024, 1]
    assert got["chunk_spans_three_intervals"]["hc_n"] == [1024, 106] and got["chunk_spans_three_intervals"]["hc_ghi"][0] == 2000 + 423
    assert got["chunk_ends_with_interval"]["hc_n"] == [1024, 10, 1024, 1024, 2] and got["chunk_ends_with_interval"]["hc_glo"] == [0, 5000, 0, 1024, 5000]
    assert got["rep_blocks"]["rb_r0"] == [0, 255, 511, 767] and got["rep_blocks"]["rb_part"] == [0, 1, 2, 2]
    assert (facts("pos_block_equal")["NPOS"], got["pos_block_equal"]["blk_iv0"]) == (POS_BLOCK, [0, 1])
    assert (facts("pos_block_plus")["NPOS"], got["pos_block_plus"]["blk_iv0"]) == (POS_BLOCK + 1, [0, 1, 1])
    assert got["pos_block_starts_interval"]["blk_iv0"] == [0, 1, 2]
    assert [facts(n)["max_part_lanes"] for n in ("lanes_32767", "lanes_32768")] == [32767, 32768]
    assert [facts(n)["hist_packed"] for n in ("lanes_32767", "lanes_32768", "ends_65535", "ends_65536", "ends_65536_twice_by_one_rep")] == [1, 1, 1, 0, 0]
    assert [(facts(n)["hist_packed"], facts(n)["yraw_narrow"]) for n in ("hist16_off", "yraw16_off", "smallest")] == [(0, 0), (1, 0), (1, 1)]


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusal(name, tool_dir):
    _, code, message = REFUSALS[name]
    assert results(tool_dir)[0][name] == {"rc": code, "msg": message}


@pytest.mark.parametrize("name,kind", list(REACTIONS))
def test_reaction(name, kind, tool_dir):
    assert results(tool_dir)[1][(name, kind)] == REACTIONS[(name, kind)][1]
