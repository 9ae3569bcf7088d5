#!/usr/bin/env python3
"""The kernels' per-thread code of the round read-out (freddie_amd/csrc/clu_readout.h) against the numpy mirror
(cluster_prep.readout_words) without a GPU: builds tools/readout_host_check.cpp with the address and undefined-behaviour sanitizers,
feeds it problems as the device sees them (packed I, C and label rows, the informative words, the accepted columns and the byte offset
the members' rows start at) and compares the exon words, the exon bytes, e and every member's characters.  The problems: random rows of
1 .. 200 segments with random informative words (bits behind M set too: the code must cut them), every offset 0 .. 17 of the rows'
start, and the shapes of the GPU test (shape_tints(): segment counts at the ends of a label word and of a bit word, 9 600 segments, 300
columns, the hand-built rows) under every set of set_variants().

    python tools/readout_host_check.py [--cases N]
"""
import argparse
import os
import random
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import round_util as ru  # noqa: E402
from freddie_amd import cluster_prep  # noqa: E402

SEGMENTS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130]
WIDEST = 9600


def flip_rows(rng, n, M, two=0.3):
    """n rows one flip from a base pattern at the most (compatible with each other: they tend to share a partition), with a constant
    stretch (uninformative segments) where M has room for one, and 0 -> 2 swaps."""
    base = [1 if rng.random() < 0.7 else 0 for _ in range(M)]
    if M >= 8:
        a = rng.randrange(M - 5)
        base[a:a + 5] = [rng.randrange(2)] * 5
    rows = []
    for i in range(n):
        row = list(base)
        if i and M > 1:
            row[rng.randrange(M)] ^= 1
        rows.append([2 if v == 0 and rng.random() < two else v for v in row])
    return rows


def pattern_rows(rng, n, M, two=0.4):
    """n rows drawn from five patterns one flip apart at interior places (a complete compatibility graph: one partition), with 0 -> 2
    swaps so that C varies where I does not."""
    base = [1 if rng.random() < 0.7 else 0 for _ in range(M)]
    base[0] = base[M - 1] = 1
    base[M // 3:M // 3 + 6] = [1] * 6
    pats = [list(base)]
    for k in range(4):
        p = list(base)
        p[2 + 5 * k] ^= 1
        pats.append(p)
    return [[2 if v == 0 and rng.random() < two else v for v in pats[rng.randrange(5)]] for _ in range(n)]


def crafted_rows():
    """40 segments.  Segments 1 .. 8 (ones) and 11 (zeros) are uninformative in every subset; rep 1 has a label 2 on the informative
    segment 10 and on the uninformative 11; rep 2 has a 0 at 20 (a C bit whose exon bit is 1 beside rep 0 and 0 alone); rep 3 starts at
    segment 3 behind a start tail and rep 4 ends at 35 before an end tail, so FL widens C over the zeros outside; rep 5 has the same
    zeros without a tail, where C stays 0."""
    base = [1] * 40
    base[10:13] = [0, 0, 0]
    rows = [list(base) for _ in range(6)]
    rows[1][10] = rows[1][11] = 2
    rows[2][20] = 0
    rows[3][0:3] = [0, 0, 0]
    rows[4][36:40] = [0, 0, 0, 0]
    rows[5][0:3] = [0, 0, 0]
    polys = {3: {"SA": (25, 7)}, 4: {"ET": (30, 9)}}
    return rows, polys


def shape_tints():
    """The tints of the GPU test, as read_segment() leaves them: one per segment count, the hand-built rows, every segment informative,
    no interior segment informative, 300 reps of 70 segments, and one tint of 9 600 segments."""
    tints = []
    for M in SEGMENTS:
        rng = random.Random(1000 + M)
        rows = flip_rows(rng, 9, M)
        polys = ru.random_gaps(rng, rows, p=0.0)[1] if M >= 16 else {}
        tints.append(ru.make_tint(len(tints), rows, {}, polys, members={i: rng.randrange(1, 4) for i in range(len(rows))}))
    rows, polys = crafted_rows()
    tints.append(ru.make_tint(len(tints), rows, {}, polys))
    tints.append(ru.make_tint(len(tints), [[(j + 1) % 2 for j in range(21)] for _ in range(4)]))      # every segment informative
    tints.append(ru.make_tint(len(tints), [[1] * 37 for _ in range(5)]))                               # only the two ends are
    tints.append(ru.make_tint(len(tints), pattern_rows(random.Random(7), 300, 70)))
    tints.append(ru.make_tint(len(tints), pattern_rows(random.Random(8), 3, WIDEST, two=0.1)))
    return tints


VARIANTS = ("first", "all", "without_0", "last", "odd_reversed", "from_64", "empty")


def set_variant(name, rids):
    """(remaining, accepted columns) of a partition's reps under one of VARIANTS: a single member; all R columns; column 0 not a member
    (the uninformative values come from a non-member); column R - 1 alone; the remaining reps reversed and every other column; the columns
    63 and above (a set beyond a 64-bit mask, where the problem is that large); no set."""
    rids, R = list(rids), len(rids)
    if name == "first":
        return rids, [0]
    if name == "all":
        return rids, list(range(R))
    if name == "without_0":
        return rids, list(range(1, R))
    if name == "last":
        return rids, [R - 1]
    if name == "odd_reversed":
        return rids[::-1], list(range(1, R, 2))
    if name == "from_64":
        return rids, list(range(63, R)) if R > 63 else sorted({0, R - 1})
    return rids, []


def host_problems():
    """[(tint, remaining, set, informative)] of the shapes for a host without partitions: every tint's reps as one problem."""
    out = []
    for tint in shape_tints():
        cluster_prep.preprocess_ilp(tint, dict(recycle_model="constant"))
        for name in VARIANTS:
            remaining, members = set_variant(name, range(len(tint["read_reps"])))
            out.append((tint, remaining, members, [int(v) for v in ru.informative_segs(tint, remaining)]))
    return out


def problem_text(M, I, C, labels, inf, members, row_offset):
    out = [M, I.shape[0], len(members), row_offset] + list(members)
    for a in (I, C, labels, inf):
        out.extend(np.asarray(a, np.uint32).reshape(-1).tolist())
    return " ".join(map(str, out))


def expected(M, I, C, labels, inf, members):
    ex, corr = cluster_prep.readout_words(I, C, labels, inf, members, M)
    j = np.arange(M)
    row = (ex[j >> 5] >> (j & 31).astype(np.uint32)) & 1
    valid_inf = [(int(inf[k >> 5]) >> (k & 31)) & 1 for k in range(M)]
    lines = [" ".join("%08x" % int(w) for w in ex), "".join(map(str, row.tolist())), "".join(str(int(row[k])) for k in range(M) if valid_inf[k])]
    lines.extend(bytes(r.tolist()).decode("ascii") for r in corr)
    return lines


def cases(n_random):
    rng = random.Random(31)
    for k in range(n_random):
        M = rng.choice([1, 2, 3, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 100, 130, 200])
        R = rng.choice([1, 2, 3, 9, 70])
        W, LW = max((M + 31) // 32, 1), max((M + 15) // 16, 1)
        data = np.array([[rng.choice([0, 1, 1, 2]) if j < M else 0 for j in range(LW * 16)] for _ in range(R)], np.uint32)
        labels = np.zeros((R, LW), np.uint32)
        for j in range(LW * 16):
            labels[:, j >> 4] |= data[:, j] << np.uint32(2 * (j & 15))
        I = cluster_prep._pack_bits((data[:, :M] == 1).astype(np.uint8), M)
        C = cluster_prep._pack_bits(((data[:, :M] == 0) & (np.random.RandomState(k).rand(R, M) < 0.8)).astype(np.uint8), M)
        inf = np.array([rng.getrandbits(32) | (rng.getrandbits(32) if k % 2 else 0) for _ in range(W)], np.uint32)      # (bits behind M too)
        members = sorted(rng.sample(range(R), rng.randrange(1, R + 1)))
        yield M, I, C, labels, inf, members, k % 18
    for tint, remaining, members, inf in host_problems():
        if not members:
            continue
        M = len(tint["segs"])
        I, C, labels = cluster_prep.readout_rows(tint, remaining)
        for row_offset in ((0, 5) if M < 1000 else (0,)):
            yield M, I, C, labels, cluster_prep._pack_bits([inf], M)[0], members, row_offset


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=300, help="random problems beside the shapes")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "readout_host_check")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I", os.path.join(ROOT, "freddie_amd", "csrc"), os.path.join(ROOT, "tools", "readout_host_check.cpp"), "-o", exe])
        texts, want = [], []
        for M, I, C, labels, inf, members, row_offset in cases(args.cases):
            texts.append(problem_text(M, I, C, labels, inf, members, row_offset))
            want.append(expected(M, I, C, labels, inf, members))
        res = subprocess.run([exe], input="\n".join(texts) + "\n", capture_output=True, text=True)
        if res.returncode != 0:
            sys.exit("the harness failed:\n" + res.stderr[-4000:])
        lines = res.stdout.split("\n")
        bad, wide, single, at = 0, 0, 0, 0
        for k, w in enumerate(want):
            got = lines[at:at + len(w)]
            counts = lines[at + len(w)].split()
            at += len(w) + 1
            wide, single = wide + int(counts[0]), single + int(counts[1])
            if got != w:
                bad += 1
                if bad <= 3:
                    print("case %d differs:" % k)
                    for a, b in zip(got, w):
                        if a != b:
                            print("  got    %s\n  mirror %s" % (a[:160], b[:160]))
        print("%d problems: %d differ (%d 16-byte stores, %d single bytes)" % (len(want), bad, wide, single))
        return 1 if bad or not wide or not single else 0


if __name__ == "__main__":
    sys.exit(main())
