"""Isoform-consensus kernels (k_consensus, k_consensus_rows, k_votes) at the places the larger tests never reach: hand-written
small cases, byte counters that fill up to the flush exactly, a workgroup's second and third isoform, rows stored anywhere in
the label buffer, every row of the vote matrix (coordinates at both ends of the int32 range included), and inputs the library
refuses.  Every comparison is integer-exact; the references are isoforms_util.plain_counts / plain_votes, which
tests/test_isoforms_host.py ties to the oracle without a GPU."""
import numpy as np
import pytest

import isoforms_util as iu
from freddie_amd import isoforms

pytestmark = pytest.mark.gpu
GRID = 8192                      # workgroups of a launch: min(n_iso, 8192) in freddie_isoforms.hip
N, S, E = 0, 1, 2                # tail codes
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


@pytest.fixture(scope="module")
def ctx():
    c = isoforms.Context(0)
    yield c
    c.close()


def _u8(s):
    return np.frombuffer(s.encode("ascii"), np.uint8)


def _batch(isos):
    """[(M, rows (n, M) uint8, tails (n,))] -> iso_read_off, n_seg, read_lab_off, labels, tail: rows one after another."""
    n_seg = np.asarray([m for m, _, _ in isos], np.int64)
    per = np.asarray([len(t) for _, _, t in isos], np.int64)
    iro = np.concatenate([[0], np.cumsum(per)])
    off = np.concatenate([[0], np.cumsum(np.repeat(n_seg, per))])[:-1]
    lab = np.concatenate([np.asarray(r, np.uint8).reshape(-1) for _, r, _ in isos] + [np.zeros(0, np.uint8)])
    tail = np.concatenate([np.asarray(t, np.uint8) for _, _, t in isos] + [np.zeros(0, np.uint8)])
    return iro, n_seg, off, lab, tail


def _check_counts(ctx, arrays, want, packed_labels=None, what=None):
    """Raw and two-bit labels through ctx.consensus, all three results against ``want``."""
    iro, n_seg, off, lab, tail = arrays
    for packed in (False, True):
        labels = (isoforms.pack_labels(lab) if packed_labels is None else packed_labels) if packed else lab
        _, cons, cov, tails = ctx.consensus(iro, n_seg, off, labels, tail, packed=packed)
        assert np.array_equal(cons, want[0]), (what, packed)
        assert np.array_equal(cov, want[1]), (what, packed)
        assert np.array_equal(tails, want[2]), (what, packed)


# ---- a. literal cases: expectations written out by hand ------------------------------------------------------------------
_LITERAL = [
    # M = 5, seven reads
    (5, [("01210", N),          # span 1..3: cov 0 1 1 1 0, cons 0 1 0 1 0
         ("00100", S),          # 'S' with a single '1': the whole row is covered, cons only where the '1' is
         ("00220", S),          # 'S' without a '1': counted nowhere, not in tails either
         ("21012", E),          # '2' at both ends: span 1..3 again
         ("20002", N),          # no '1': not counted
         ("10000", N),          # a '1' only in column 0
         ("00001", E)],         # a '1' only in column M - 1
     [1, 2, 1, 2, 1], [2, 3, 3, 3, 2], [2, 1, 2]),
    # one read: fewer than three reads in an isoform
    (5, [("01210", N)], [0, 1, 0, 1, 0], [0, 1, 1, 1, 0], [1, 0, 0]),
    # M = 17: the second lane of a read's group holds one label
    (17, [("00000000000000011", N),     # first '1' at 15, last at 16: the span crosses the 16-label lane boundary
          ("21000000000000012", N),     # '2' at both ends, span 1..15
          ("00000000000000001", E),     # column M - 1 alone
          ("10000000000000000", S)],    # column 0 alone, 'S': covers the row
     [1, 1] + [0] * 13 + [2, 2], [1] + [2] * 14 + [3, 3], [2, 1, 1]),
]


def _literal():
    arrays = _batch([(m, np.stack([_u8(s) for s, _ in reads]), [t for _, t in reads]) for m, reads, _, _, _ in _LITERAL])
    want = (np.concatenate([x for _, _, x, _, _ in _LITERAL]).astype(np.int32),
            np.concatenate([c for _, _, _, c, _ in _LITERAL]).astype(np.int32),
            np.asarray([t for _, _, _, _, t in _LITERAL], np.int32))
    return arrays, want


@pytest.mark.parametrize("rows_switch", ["1", "0"])
def test_literal_cases(ctx, rows_switch, monkeypatch):
    monkeypatch.setenv("FISO_ROWS", rows_switch)
    arrays, want = _literal()
    plain = iu.plain_counts(*arrays)
    assert all(np.array_equal(a, b) for a, b in zip(plain, want))      # the helper, tied to hand-checked numbers
    _check_counts(ctx, arrays, want)


# ---- b. byte counters that reach the flush exactly ------------------------------------------------------------------------
@pytest.mark.parametrize("rows_switch", ["1", "0"])
@pytest.mark.parametrize("M", [16, 150, 1024])
def test_byte_counters_fill_up_to_the_flush(ctx, M, rows_switch, monkeypatch):
    """Every label is '1' and an isoform's reads share one tail value, so in k_consensus_rows every counter byte of a busy lane
    and the tail byte gain 1 per row load.  A wave takes L (+1 for the odd read) row loads when the isoform has 4 * rpw * L
    reads; the L bracket 254 = the loads between flushes (255 rounded down to the 2 loads in flight) and twice that.
    Expected without a reference: every count is the number of reads.  Second round: column M // 2 holds '0' in every read."""
    monkeypatch.setenv("FISO_ROWS", rows_switch)
    rpw = 64 // -(-M // 16)
    counts = [4 * rpw * L + r for L in (253, 254, 255, 256, 508, 509) for r in (0, 1)]
    full = np.full((3 * max(counts), M), ord("1"), np.uint8)
    holed = full.copy()
    holed[:, M // 2] = ord("0")
    for hole, rows in ((False, full), (True, holed)):
        lab = rows.reshape(-1)
        lab2 = isoforms.pack_labels(lab)
        for n in counts:
            arrays = (np.arange(4) * n, [M] * 3, np.arange(3 * n) * M, lab[:3 * n * M], np.repeat(np.arange(3, dtype=np.uint8), n))
            cov = np.full(3 * M, n, np.int32)
            cons = cov.copy()
            if hole:
                cons[M // 2::M] = 0
            _check_counts(ctx, arrays, (cons, cov, n * np.eye(3, dtype=np.int32)), lab2[:(3 * n * M + 3) // 4], (n, hole))


# ---- c. a workgroup's second and third isoform ----------------------------------------------------------------------------
# (row length, reads where the block index is below 100, reads above, kind); consecutive visits of a workgroup take consecutive
# entries, so every entry is somebody's first, second and third isoform and each is followed by a very different one
_VISITS = [(1024, 40, 8, "any"), (1, 70, 70, "any"), (513, 10, 10, "any"), (161, 300, 40, "any"), (48, 0, 0, "any"), (33, 5, 5, "any"),
           (0, 4, 4, "any"), (17, 6, 6, "any"), (100, 20, 20, "no 1"), (100, 20, 20, "all S")]


@pytest.fixture(scope="module")
def grid_reuse():
    rng = np.random.default_rng(31)
    pool = rng.choice(_u8("0012"), size=6 << 20, p=[0.45, 0.25, 0.25, 0.05])
    used = [0]

    def take(n, m):
        used[0] += n * m
        return pool[used[0] - n * m:used[0]].reshape(n, m)

    isos = []
    for i in range(2 * GRID + 300):
        b, visit = i % GRID, i // GRID
        if b < 300:
            m, n_low, n_high, kind = _VISITS[(b + visit) % len(_VISITS)]
            n = n_low if b < 100 else n_high
        else:
            m, n, kind = int(rng.integers(1, 41)), int(rng.integers(1, 4)), "any"
        rows = take(n, m)
        if kind == "no 1":
            rows = np.where(rows == ord("1"), ord("0"), rows).astype(np.uint8)
        isos.append((m, rows, np.ones(n, np.uint8) if kind == "all S" else rng.integers(0, 3, n).astype(np.uint8)))
    longer = [(1025, take(7, 1025), rng.integers(0, 3, 7)), (3000, take(12, 3000), rng.integers(0, 3, 12))]
    assert used[0] <= len(pool)
    one = _batch(isos)
    want = iu.plain_counts(*one)
    extra = iu.plain_counts(*_batch(longer))
    two = _batch(isos + longer)
    return (one, want, isoforms.pack_labels(one[3])), (two, tuple(np.concatenate([a, b]) for a, b in zip(want, extra)), isoforms.pack_labels(two[3]))


@pytest.mark.parametrize("rows_switch", ["1", "0"])
def test_a_workgroup_serves_three_isoforms(ctx, grid_reuse, rows_switch, monkeypatch):
    """2 * 8192 + 300 isoforms on 8192 workgroups: workgroup b serves b, b + 8192 and b + 16384, for b < 300 three isoforms
    that differ sharply (1 024 labels, then 1, then 513; reads, then none; M = 0; no '1' anywhere; all 'S').  The second
    call appends rows longer than 1 024 labels, which sends the whole call to the two-pass kernel."""
    monkeypatch.setenv("FISO_ROWS", rows_switch)
    for k, (arrays, want, packed) in enumerate(grid_reuse):
        assert len(arrays[1]) >= 2 * GRID + 300 and want[0].sum() > 0
        _check_counts(ctx, arrays, want, packed, "call %d" % k)


# ---- d. rows anywhere in the label buffer ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scattered():
    rng = np.random.default_rng(41)
    n_seg = np.asarray([1, 15, 16, 17, 31, 32, 33, 150, 160, 161, 255, 256, 511, 513, 1000, 1024, 20, 48, 100, 0] * 2)
    per = rng.integers(5, 41, len(n_seg))
    desc = 7                                                    # this isoform's rows lie in descending order (M = 150)
    slot_iso, read_slot, shared = [], [], 0                     # a slot = one stored row
    for i in range(len(n_seg)):
        own = []
        for _ in range(per[i]):
            if own and i != desc and rng.random() < 0.1:
                read_slot.append(int(rng.choice(own))); shared += 1      # this read points at another read's row
            else:
                own.append(len(slot_iso)); read_slot.append(len(slot_iso)); slot_iso.append(i)
    order = rng.permutation(len(slot_iso))
    if n_seg[slot_iso[order[-1]]] == 0:                          # the last row of the buffer has labels
        k = next(k for k in range(len(order)) if n_seg[slot_iso[order[k]]] > 0)
        order[[k, -1]] = order[[-1, k]]
    start = np.zeros(len(slot_iso), np.int64)
    pos = 0
    for s in order:
        pos += int(rng.integers(0, 38))                         # a gap of 0..37 labels in front of every row
        start[s] = pos
        pos += int(n_seg[slot_iso[s]])
    lab = rng.choice(_u8("0012"), size=pos, p=[0.45, 0.25, 0.25, 0.05])       # the gaps hold labels too: reading them would show
    mine = [s for s in range(len(slot_iso)) if slot_iso[s] == desc]
    start[mine] = np.sort(start[mine])[::-1]
    for s in range(0, len(slot_iso), 9):                        # some rows without a '1'
        lab[start[s]:start[s] + n_seg[slot_iso[s]]] = ord("0")
    off = start[read_slot]
    iro = np.concatenate([[0], np.cumsum(per)])
    tail = rng.integers(0, 3, len(off)).astype(np.uint8)
    return (iro, n_seg, off, lab, tail), desc, shared


@pytest.mark.parametrize("rows_switch", ["1", "0"])
def test_rows_anywhere_in_the_buffer(ctx, scattered, rows_switch, monkeypatch):
    """read_lab_off is arbitrary: a random permutation of the rows with gaps, shared rows, one isoform in descending order,
    every start residue mod 16 (raw) and mod 4 (packed), and the last row ending with the buffer, which is passed at exactly
    that length (the kernels' vector loads past it land in the library's padding)."""
    monkeypatch.setenv("FISO_ROWS", rows_switch)
    (iro, n_seg, off, lab, tail), desc, shared = scattered
    m_of = np.repeat(n_seg, np.diff(iro))
    assert shared >= len(off) // 20
    assert len(np.unique(off[m_of > 0])) < (m_of > 0).sum()           # rows that two reads share
    assert (np.diff(off) < 0).sum() > len(off) // 4                    # out of order
    by_off = np.argsort(off[m_of > 0])
    assert (np.diff(off[m_of > 0][by_off]) > m_of[m_of > 0][by_off][:-1]).any()      # with gaps between rows
    assert (np.diff(off[iro[desc]:iro[desc + 1]]) < 0).all()
    assert set((off[m_of > 0] % 16).tolist()) == set(range(16))
    assert set((off[m_of > 0] % 4).tolist()) == set(range(4))
    top = np.flatnonzero(m_of > 0)[np.argmax(off[m_of > 0])]
    assert off[top] + m_of[top] == len(lab) == (off + m_of).max()
    packed = isoforms.pack_labels(lab)
    assert len(packed) == (len(lab) + 3) // 4
    want = iu.plain_counts(iro, n_seg, off, lab, tail)
    assert want[0].sum() > 0
    _check_counts(ctx, (iro, n_seg, off, lab, tail), want, packed)


# ---- e. every vote row ----------------------------------------------------------------------------------------------------
def _vote_arrays(isos):
    """[(isoform boundaries, [a read's boundaries, ...])] -> iso_read_off, iso_b_off, iso_bound, read_b_off, read_bound"""
    iro, ibo, ib, rbo, rb = [0], [0], [], [0], []
    for bounds, reads in isos:
        for r in reads:
            rb.extend(r); rbo.append(len(rb))
        ib.extend(bounds); iro.append(len(rbo) - 1); ibo.append(len(ib))
    return (np.asarray(iro, np.int64), np.asarray(ibo, np.int64), np.asarray(ib, np.int64).astype(np.int32), np.asarray(rbo, np.int64),
            np.asarray(rb, np.int64).astype(np.int32))


def _around(b, w):
    return [b - w, b + w, b - (w + 1), b + (w + 1), b]


def _vote_batch(w):
    rng = np.random.default_rng(50 + w)
    fill = []
    for _ in range(50):                                         # ordinary isoforms: close boundaries, reads of 0..4 boundaries
        base = int(rng.integers(-300, 300))
        bounds = sorted((base + rng.integers(0, 4 * w + 4, int(rng.integers(0, 7)))).tolist())
        fill.append((bounds, [(base + rng.integers(-w - 2, 5 * w + 6, int(rng.integers(0, 5)))).tolist() for _ in range(int(rng.integers(0, 9)))]))
    steps = np.cumsum([1000, 1, 2, w, w + 1, 2 * w, 2 * w + 1]).tolist()      # boundaries 1, 2, w, w + 1, 2w, 2w + 1 apart
    spaced = (steps, [[], _around(steps[0], w), [], _around(steps[3], w), _around(steps[-1], w), [steps[1], steps[2] + w], []])
    equal = ([500, 500, 510, 510, 510, 530], [_around(500, w), [], _around(510, w) + [505], [530, 530 - w]])     # runs of 2 and 3 equal ones
    no_reads = ([100, 200, 300], [])
    no_bounds = ([], [[100, 200], [], [300]])
    nothing = ([], [])
    crowd = ([7777], [[7777 + w]] * 5000)                       # one counter reads 5 000
    thirty = [10000 + 100 * k for k in range(30)]
    many = (thirty, [r.tolist() for r in rng.permutation(np.arange(9950, 12950)).reshape(300, 10)])      # 3 000 distinct read boundaries
    negative = ([-5000, -5000 + w, -3], [_around(-5000, w), [-3 - w, -3 + w, -3], [-5000 + 2 * w]])
    top = ([I32_MAX - 3, I32_MAX], [[I32_MAX], [I32_MAX - w]])
    bottom = ([I32_MIN, I32_MIN + 3], [[I32_MIN], [I32_MIN + w]])
    return fill[:10] + [spaced, no_bounds, equal, nothing, no_reads] + fill[10:20] + [crowd, many] + fill[20:35] + [negative, top, bottom] + fill[35:]


@pytest.mark.parametrize("w", [1, 8, 20])
def test_every_vote_row(ctx, w):
    """k_votes against plain_votes on a crafted batch: isoform boundaries closer than the window and equal ones, read boundaries at
    +-w and +-(w + 1), reads and isoforms without boundaries, isoforms without reads, 5 000 votes on one counter, 3 000 read
    boundaries of one isoform, negative coordinates and both ends of the int32 range (where v + w and v - w leave int32)."""
    isos = _vote_batch(w)
    arrays = _vote_arrays(isos)
    want = iu.plain_votes(*arrays, w)
    assert want.sum() > 0 and ((want > 0).sum(1) >= 2).any() and want.max() == 5000
    top, bottom = int(arrays[1][len(isos) - 17]), int(arrays[1][len(isos) - 16])      # the first vote rows of the two isoforms at the ends
    assert isos[-17][0][1] == I32_MAX and isos[-16][0][0] == I32_MIN
    hand = np.zeros(2 * w + 1, np.int32)
    hand[w] = 1; hand[0] = 1                                    # boundary 2^31 - 1: reads at it and w below it
    assert np.array_equal(want[top + 1], hand)
    assert np.array_equal(want[bottom], hand[::-1])             # boundary -2^31: reads at it and w above it
    assert want[top].sum() == (2 if w >= 3 else 0) == want[bottom + 1].sum()      # boundaries 3 inside the range: distances 3 and 3 - w
    got = ctx.boundary_votes(*arrays, w)
    assert np.array_equal(got[[top, top + 1, bottom, bottom + 1]], want[[top, top + 1, bottom, bottom + 1]])
    assert np.array_equal(got, want)
    # a workgroup's second isoform, some of them without boundaries (the kernel's early `continue`)
    pattern = [([10, 12, 12 + w], [[10], [11, 12 + w]]), ([], [[5]]), ([0], []), ([-3, 40], [[], [-3 + w, 40 - w - 1]]), ([], [])]
    isos = (pattern * ((GRID + 200) // len(pattern) + 1))[:GRID + 200]
    arrays = _vote_arrays(isos)
    assert (np.diff(arrays[1])[GRID:] == 0).any() and (np.diff(arrays[1])[GRID:] > 0).any()
    want = iu.plain_votes(*arrays, w)
    assert want[int(arrays[1][GRID]):].sum() > 0
    assert np.array_equal(ctx.boundary_votes(*arrays, w), want)


# ---- f. refusals ----------------------------------------------------------------------------------------------------------
def _literal_still_holds(ctx):
    arrays, want = _literal()
    _check_counts(ctx, arrays, want)


def test_refusals_leave_the_context_usable(ctx):
    """Every input here is turned away by the host checks of consensus_impl / fiso_boundary_votes before anything is launched."""
    _literal_still_holds(ctx)
    iro, ibo, ib, rbo, rb = [0, 2, 3], [0, 2, 4], [10, 20, 5, 5], [0, 1, 2, 3], [10, 20, 5]       # (equal boundaries are fine)
    assert ctx.boundary_votes(iro, ibo, ib, rbo, rb, 2).tolist() == [[0, 0, 1, 0, 0], [0, 0, 1, 0, 0], [0, 0, 1, 0, 0], [0, 0, 1, 0, 0]]
    for w in (0, 21):
        with pytest.raises(isoforms.IsoformsError, match=r"window must be in \[1, 20\]"):
            ctx.boundary_votes(iro, ibo, ib, rbo, rb, w)
    with pytest.raises(isoforms.IsoformsError, match="isoform 1: boundaries are not ascending"):
        ctx.boundary_votes(iro, ibo, [10, 20, 5, 4], rbo, rb, 2)
    for name, k in (("iso_read_off", 0), ("iso_b_off", 1), ("read_b_off", 3)):
        good = [iro, ibo, ib, rbo, rb]
        for bad, msg in (([1] + good[k][1:], name + " does not start at 0"), (good[k][:1] + [good[k][2], good[k][1]] + good[k][3:], name + " is not monotone at 1")):
            args = list(good)
            args[k] = bad
            with pytest.raises(isoforms.IsoformsError, match=msg):
                ctx.boundary_votes(*args, 2)
    with pytest.raises(isoforms.IsoformsError):
        ctx.boundary_votes([0], [0], [], [0], [], 2)             # n_iso == 0
    _literal_still_holds(ctx)

    (iro, n_seg, off, lab, tail), _ = _literal()
    for bad_iro, msg in ((np.concatenate([[1], iro[1:]]), "iso_read_off does not start at 0"), (iro[[0, 2, 1, 3]], "iso_read_off is not monotone at 1")):
        with pytest.raises(isoforms.IsoformsError, match=msg):
            ctx.consensus(bad_iro, n_seg, off, lab, tail)
    bad_tail = tail.copy()
    bad_tail[9] = 3
    with pytest.raises(isoforms.IsoformsError, match="read 9: bad label offset or tail"):
        ctx.consensus(iro, n_seg, off, lab, bad_tail)
    bad_off = off.copy()
    bad_off[4] = -1
    for packed in (False, True):
        with pytest.raises(isoforms.IsoformsError, match="read 4: bad label offset or tail"):
            ctx.consensus(iro, n_seg, bad_off, isoforms.pack_labels(lab) if packed else lab, tail, packed=packed)
    with pytest.raises(isoforms.IsoformsError):
        ctx.consensus([0], [], [], [], [])                       # n_iso == 0
    _literal_still_holds(ctx)

    # iso_seg_off is the wrapper's own cumsum, so the disagreement with n_seg goes through the C interface
    a = [np.ascontiguousarray(iro, np.int64), np.ascontiguousarray(n_seg, np.int32), np.asarray([0, 5, 9, 26], np.int64),
         np.ascontiguousarray(off, np.int64), lab, tail]
    out = [np.zeros(27, np.int32), np.zeros(27, np.int32), np.zeros(9, np.int32)]
    rc = ctx._L.fiso_consensus(ctx._h, 3, *[x.ctypes.data for x in a + out])
    assert rc != 0 and ctx._L.fiso_last_error(ctx._h).decode() == "isoform 1: iso_seg_off does not match n_seg"
    a[2] = np.asarray([0, 5, 10, 27], np.int64)
    assert ctx._L.fiso_consensus(ctx._h, 3, *[x.ctypes.data for x in a + out]) == 0       # the same arrays with the right offsets
    assert np.array_equal(out[0], _literal()[1][0])
    _literal_still_holds(ctx)
