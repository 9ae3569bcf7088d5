"""Hand-built batches for k_label_reads (csrc/seg_tail.hip) at the edges of what it stages: reps per partition on the unit
(64 reps) and block (256 reps) edges, the exons of a unit one below, on and one above kLabelExons, column tables of 1, kLabelStage
and kLabelStage + 1 columns crossed with those, a unit's first exon at every residue mod 4 of the exon arrays, and the geometry the
merge has to get right.  tests/test_label_cases_host.py shows on the CPU that every batch reaches its edge;
tests/test_gpu_label_lds.py runs the batches on the device.

A partition's columns are made the way tests/edge_cases.py makes them: one heavy rep (weight 60) whose exons' ends become the final
positions; every other rep has weight 1 and inner exon ends that lie on those positions (or has one exon: under ignore_ends its
ends count nothing), so the column table is the skeleton's whatever reps are added."""
import functools

import numpy as np

import util

LABEL_STAGE = 1024     # kLabelStage (csrc/seg_common.h)
LABEL_EXONS = 960      # kLabelExons
UNIT = 64              # reps of a unit (a workgroup's share of a 256-rep block)
BLOCK = 256
S0 = 1000

PARAMS = dict(sigma=3.0, variance_factor=0.01, min_read_support_outside=1000)
PARAMS_FLAT = dict(sigma=3.0, variance_factor=9.99, min_read_support_outside=1000)      # no candidate but the intervals' ends
RATE_HAS2 = 0.9999     # smooth_threshold()'s last entry rounds to 1.0: a segment of exactly 107 positions has lo < 0
REP_COUNTS = [1, 63, 64, 65, 255, 256, 257]


class Skeleton:
    """Two intervals and the heavy rep's exons (30 positions an exon: positions 10 .. 24 of every 30), as tests/edge_cases.label_part
    lays them out: S columns, the sentinel between the intervals among them.  head: the first exon's last position relative to the
    interval's start (106: the first column has exactly 107 positions)."""

    def __init__(self, S, head=24, at=S0):
        E = (S - 1) // 2 if S % 2 else S // 2
        E1 = E // 2
        d = head - 24
        a0, a1 = at, at + d + 30 * E1 + (20 if S % 2 else -6)
        b0 = a1 + 500
        ex = [(a0 + 10, a0 + head)] + [(a0 + d + 10 + 30 * i, a0 + d + 24 + 30 * i) for i in range(1, E1)]
        ex += [(b0 + 10 + 30 * i, b0 + 24 + 30 * i) for i in range(E - E1)]
        b1 = ex[-1][1] + 40
        self.S, self.E, self.E1, self.ex, self.ivs = S, E, E1, ex, [(a0, a1), (b0, b1)]
        self.bounds = sorted({a0, a1, b0, b1} | {x for e in ex for x in e} - {ex[0][0], ex[-1][1]})
        assert len(self.bounds) - 1 == S, (len(self.bounds) - 1, S)
        self.sent = sum(g <= a1 for g in self.bounds) - 1        # the sentinel column
        self.end = b1 + 100

    def chain(self, j, k, d0=-3, d1=3):
        """A rep of k exons: the heavy rep's exons j .. j + k - 1 (inner ends on final positions), its first start and last end moved."""
        e = self.ex[j:j + k]
        assert len(e) == k
        if k == 1:
            return [(e[0][0] + d0, e[0][1] + d1)]
        return [(e[0][0] + d0, e[0][1])] + e[1:-1] + [(e[-1][0], e[-1][1] + d1)]

    def geometry(self):
        """Single exons against the columns' edges (as edge_cases.label_part places them), exons across the sentinel, a read that
        starts exactly on a column's edge, and reps with several short exons inside one column (weight 1 each: no final position)."""
        b, S, (iv_a, iv_b) = self.bounds, self.S, self.ivs
        reads = []

        def add(x, y):
            if iv_a[0] <= x < y <= iv_a[1] or iv_b[0] <= x < y <= iv_b[1]:
                reads.append([(x, y)])
        for i in (1, 2):                                            # across the sentinel, inner ends on final positions
            reads.append([(b[self.sent - 2 * i] - 3, self.ex[self.E1 - 1][1]), (self.ex[self.E1][0], self.ex[self.E1 + i][1] + 3)])
        for c in [3, self.sent - 2, self.sent + 2, S - 4]:
            g0, g1 = b[c], b[c + 1]
            add(g0 + 2, g0 + 6)
            for end in (g0 - 1, g0, g1 - 1, g1):
                add(b[c - 2] + 1, end)                              # ends on fp[c] - 1, fp[c], fp[c+1] - 1, fp[c+1]
                add(end, b[c + 3] - 1)                              # starts there
            add(g0, b[c + 2] + 1)                                   # starts exactly on the column's edge
        g0 = b[5]
        reads.append([(g0 + 1, g0 + 3), (g0 + 5, g0 + 7), (g0 + 9, g0 + 11)])      # three short exons inside one column
        reads.append([(b[4] - 5, g0 + 4), (g0 + 6, b[7] + 2)])                        # two exons that meet inside a column
        return reads

    def part(self, reads):
        reads = [self.ex] + reads
        return util.hand(self.ivs, reads, [60] + [1] * (len(reads) - 1))


def mixed_reps(sk, n, seed):
    """n reps of 1 .. 14 exons over the skeleton, the geometry reads first."""
    rng = np.random.default_rng(seed)
    reads = sk.geometry()[:n]
    while len(reads) < n:
        k = int(rng.integers(1, min(14, sk.E) + 1))
        j = int(rng.integers(0, sk.E - k + 1))
        reads.append(sk.chain(j, k, -int(rng.integers(0, 8)), int(rng.integers(0, 5))))
    return reads


def count_part(n_reps, seed, S=41, head=24):
    """A partition of n_reps reps in all (the heavy rep among them)."""
    sk = Skeleton(S, head)
    reads = mixed_reps(sk, n_reps - 1, seed)
    if n_reps > 30:
        reads[-1] = sk.chain(1, 14)                                 # a 14-exon rep as the partition's last
        reads[-2] = sk.chain(2, 1)
    return sk.part(reads)


def exon_part(S, head=24):
    """Three units whose exons number kLabelExons, kLabelExons - 1 and kLabelExons + 1 (in that order: a staged unit on either side of
    ... and then one that is not), and a last unit of three reps.  Unit 0 holds the heavy rep; 64 reps of 15 exons are 960."""
    sk = Skeleton(S, head)
    n0 = len(sk.ex)
    rest = LABEL_EXONS - n0                                         # unit 0: the heavy rep and 63 more
    reads = []
    per = [rest // 63 + (i < rest % 63) for i in range(63)]
    assert sum(per) == rest and min(per) >= 1 and max(per) <= sk.E
    for i, k in enumerate(per):
        reads.append(sk.chain(i % (sk.E - k + 1), k, -(i % 7), i % 4))
    for total in (LABEL_EXONS - 1, LABEL_EXONS + 1):
        per = [total // 64 + (i < total % 64) for i in range(64)]
        assert max(per) <= sk.E
        for i, k in enumerate(per):
            reads.append(sk.chain((3 * i) % (sk.E - k + 1), k, -(i % 5), i % 3))
    reads += [sk.chain(0, 2), sk.chain(1, 1), sk.chain(2, 3)]
    return sk.part(reads)


FLAT_LEN = 41          # positions of the one-column interval: no refinement (its ends are not more than 40 apart), under 50 candidates


def flat_part(n_units_exons):
    """S = 1: one interval of 41 positions and nothing chosen inside it (PARAMS_FLAT: no candidate is fixed and none has the support;
    the interval is too short for refinement and for an anchor of max_problem_size).  Units of the given exon totals: a rep of k
    exons is k exons of two positions, one after the other, from an offset that moves with the rep; every third rep's first exon
    starts with the interval and every fourth's last exon ends with it -- the coverage of the one column runs from 2 to 39 positions."""
    reads = []
    for total in n_units_exons:
        per = [total // 64 + (i < total % 64) for i in range(64)]
        assert max(per) <= 16
        for k in per:
            i = len(reads)
            a = S0 + 2 + i % (FLAT_LEN - 2 * k - 4)
            r = [(a + 2 * j, a + 2 * j + 1) for j in range(k)]
            if i % 3 == 0: r[0] = (S0, r[0][1])
            if i % 4 == 0: r[-1] = (r[-1][0], S0 + FLAT_LEN - 1)
            reads.append(r)
    return util.hand([(S0, S0 + FLAT_LEN - 1)], reads)


def pad_part(n_exons, at):
    """One rep of n_exons (1 .. 3) short exons in an interval of its own: it moves the next partition's first exon by n_exons."""
    r = [(at + 10 + 20 * i, at + 20 + 20 * i) for i in range(n_exons)]
    return util.hand([(at, at + 100)], [r])


def main_batch():
    """Packed labels (rate 0.9): every rep count; the exon cases under column tables of kLabelStage (LDS) and kLabelStage + 1 (global
    memory) columns; the exon case over a small column table four times, each behind a one-exon partition, so that its units' first exons sit at every
    residue mod 4."""
    names, parts = [], []
    for n in REP_COUNTS:
        names.append("reps-%d" % n); parts.append(count_part(n, n))
    for S in (LABEL_STAGE, LABEL_STAGE + 1):
        names.append("exons-S%d" % S); parts.append(exon_part(S))
    small = exon_part(41)
    for i in range(4):
        names += ["pad-%d" % i, "exons-small-%d" % i]; parts += [pad_part(1, 500), small]
    return names, parts, dict(PARAMS, threshold_rate=0.9)


def bytes_batch():
    """Label bytes (rate 0.9999: the table's last entry is 1.0): partitions with a 107-position column (part_has2: every row is first
    rewritten with the columns' defaults) and without, rep counts around the unit, all four instances."""
    names = ["has2-reps-65", "plain-reps-63", "has2-exons-small", "plain-exons-small", "has2-exons-S1025", "has2-reps-257", "plain-reps-1"]
    parts = [count_part(65, 1, head=106), count_part(63, 2), exon_part(41, head=106), exon_part(41), exon_part(LABEL_STAGE + 1, head=106),
             count_part(257, 3, head=106), count_part(1, 4)]
    return names, parts, dict(PARAMS, threshold_rate=RATE_HAS2)


def flat_batch():
    """S = 1 crossed with the exon cases, between two-interval partitions (under these parameters they have three columns, the
    sentinel in the middle): one workgroup then walks units of different shapes in turn."""
    names = ["S1-exons", "two-intervals-65", "S1-small", "two-intervals-exons"]
    parts = [flat_part([LABEL_EXONS, LABEL_EXONS + 1, LABEL_EXONS - 1, 70]), count_part(65, 7), flat_part([64]), exon_part(41)]
    return names, parts, dict(PARAMS_FLAT, threshold_rate=0.9)


BATCHES = dict(main=main_batch, bytes=bytes_batch, flat=flat_batch)


@functools.lru_cache(maxsize=None)
def batch(name):
    return BATCHES[name]()


@functools.lru_cache(maxsize=None)
def oracles(name):
    _, parts, params = batch(name)
    done = {}
    out = []
    for p in parts:                                                 # (a partition that a batch holds several times is computed once)
        if id(p) not in done:
            done[id(p)] = util.run_oracle(p, params)
        out.append(done[id(p)])
    return out


def units(name):
    """The units of a batch as the kernel forms them, a row each: (partition, reps, first exon in the batch's arrays, exons, S, column
    table staged, exons staged)."""
    _, parts, _ = batch(name)
    rows, e0 = [], 0
    for p, (part, o) in enumerate(zip(parts, oracles(name))):
        S = len(o["final_pos"]) - 1
        off = np.asarray(part.rep_exon_off, np.int64)
        for b0 in range(0, part.n_reps, BLOCK):
            for r0 in range(b0, min(b0 + BLOCK, part.n_reps), UNIT):
                r1 = min(r0 + UNIT, part.n_reps)
                n_ex = int(off[r1] - off[r0])
                rows.append((p, r1 - r0, e0 + int(off[r0]), n_ex, S, S <= LABEL_STAGE, n_ex <= LABEL_EXONS))
        e0 += int(off[-1])
    return rows
