"""Built cases for the upload's device-side preparation (csrc/seg_upload.hip, lex_copy_tile in seg_common.h, the radix wrapper in
freddie_seg_sort.hip): the model of the lane list, the exon stream and the histogram chunks' lane ranges in numpy, its named one-rule
mutations, a literal restatement of the reference's per-read asserts, and the batches, each named after the edge it was built for.

The model is the one tests/test_gpu_paths.py::test_lane_preparation_on_the_device and util.lanes_range state:
order = lexsort((arange, first)), lanes = repeat(order, weight), start = first[lanes], pmax = maximum.accumulate(last[lanes]), a
lane's exon range, the lane-ordered stream of (ts, te) pairs and every lane's range in it; per histogram chunk
llo = searchsorted(pmax, glo, 'left') and lhi = llo + searchsorted(start[llo:], ghi, 'right') over the partition's lanes, with the
chunking (p0, n, glo, ghi) derived here from the constants of seg_common.h and the intervals alone.

Groups: N rep counts around the in-LDS sort's sizes, T order and ties, M where the running maximum is carried, W weights, X the
exon stream's 4 096-exon chunks, B counts of partitions and rep blocks, H lanes exactly on a chunk's bounds, V validation.  Small
partitions are written with util.hand; the large ones (up to 16 640 reps, 65 837 partitions) are the same PackedPartition built from
arrays (build()).  tests/test_lane_cases_host.py shows on the CPU that every case reaches its edge and that every mutation is seen;
tests/test_gpu_lane_edges.py runs the batches.

Group V's refused batches are documented status returns (FSEG_ERR_INPUT), not faults.  Read before the first run: during the upload no
kernel indexes memory by an exon's value -- k_prep_reps reads ex_ts / ex_te at indices from rep_exon_off (monotone and bounded: checked
on the host) and the interval arrays at kk in [k0, k1); k_lanes / k_lane_* and lex_copy_tile address by rep, by scanned counts and by
rep_exon_off; k_hist_ranges compares values.  The first run's front is enqueued before the upload's verdict is read, and k_hist there
does index its counters by position -- after its own test that ts lies in an interval that also holds te's upper end.  A reversed exon
(ts > te) is therefore built with BOTH ends inside one interval, never with te in front of the interval's start."""
import functools

import numpy as np

import util
from freddie_amd import pack

# csrc/seg_common.h
SORT_MAX = 2048          # kLaneSortMax: the largest partition k_lanes sorts in LDS
TILE = 256               # reps per tile of k_lanes / per block of the block kernels
SCAN = 64                # blocks per trip of k_lane_block_scan's loop
LEX = 4096               # kLexChunk
GRID = 65536             # grid_for(.., 65536): the grid-stride loops' largest grid
CHUNK32, CHUNK16 = 8192, 16384      # kHistChunk, kHistChunk16
CHUNK_MIN, CHUNK_WGS = 1024, 512    # fseg_upload: halve the chunk while the batch has fewer than 512 of them
COUNT16 = 65535          # kHistCountMax16
INT_MIN = -2 ** 31

ENDS = dict(ignore_ends=False)     # single-exon reps count on the histogram only when their ends do


def build(ivs, counts, ts, te, weights=None):
    """util.hand from arrays: intervals [(start, end)], exons per rep, every exon's (ts, te); a rep per read."""
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    part = pack.pack_partition([s for s, _ in ivs], [e for _, e in ivs], off, np.asarray(ts, np.int32), np.asarray(te, np.int32), dedupe=False)
    assert len(part.ex_ts) == off[-1]
    if weights is not None:
        part.rep_weight = np.asarray(weights, np.int32)
    return part


def single(first, last, weights=None, ivs=None):
    """Single-exon reps (first, last) on one interval that holds them all."""
    first, last = np.asarray(first, np.int64), np.asarray(last, np.int64)
    assert (first < last).all()
    ivs = ivs or [(int(first.min()) - 10, int(last.max()) + 10)]
    return build(ivs, np.ones(len(first), np.int64), first, last, weights)


def firsts(p):
    return p.ex_ts[p.rep_exon_off[:-1]]


def lasts(p):
    return p.ex_te[p.rep_exon_off[1:] - 1]


def sorted_order(p):
    return np.lexsort((np.arange(p.n_reps), firsts(p)))


# ---- the model -------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("tie_reverse", "tie_by_last", "pmax_reset_64", "pmax_reset_256", "pmax_reset_16384", "pmax_exclusive", "lane_carry_dropped",
             "stream_reset_4096", "llo_right", "lhi_left", "glo_plus", "glo_minus", "ghi_plus", "ghi_minus", "key_unsigned")


def model_partition(p, mut=None):
    """The partition's lanes and exon stream, offsets relative to the partition.  `mut`: one rule changed (MUTATIONS)."""
    R = p.n_reps
    first, last, idx = firsts(p), lasts(p), np.arange(R)
    if mut == "tie_reverse":
        order = np.lexsort((-idx, first))
    elif mut == "tie_by_last":
        order = np.lexsort((idx, last, first))
    elif mut == "key_unsigned":                                      # the position as an unsigned word, no bias: negative positions sort last
        order = np.lexsort((idx, first.astype(np.uint32)))
    else:
        order = np.lexsort((idx, first))
    w = p.rep_weight[order].astype(np.int64)
    sl = last[order]
    reset = dict(pmax_reset_64=64, pmax_reset_256=TILE, pmax_reset_16384=TILE * SCAN).get(mut)
    if reset:                                                        # a carry lost: from wave to wave, tile to tile, trip to trip
        m = np.concatenate([np.maximum.accumulate(sl[i:i + reset]) for i in range(0, R, reset)])
    else:
        m = np.maximum.accumulate(sl)
    if mut == "pmax_exclusive":
        m = np.concatenate([[INT_MIN], m[:-1]]).astype(sl.dtype)
    excl = np.cumsum(w) - w
    base = excl - excl[idx // TILE * TILE] if mut == "lane_carry_dropped" else excl       # every tile starts at the partition's lane 0
    nl = int(w.sum())
    src = np.repeat(idx, w)                                          # the sorted rep of every emitted lane
    dest = np.repeat(base, w) + (np.arange(nl) - np.repeat(excl, w))
    ne = np.diff(p.rep_exon_off)[order]
    eoff = np.cumsum(ne) - ne
    I = int(ne.sum())

    def put(values, shape=()):
        out = np.zeros((nl,) + shape, values.dtype)
        out[dest] = values[src]
        return out
    start, pmax = put(first[order]), put(m)
    exons = put(np.stack([p.rep_exon_off[order], p.rep_exon_off[order + 1]], axis=1), (2,))
    stream = put(np.stack([eoff, eoff + ne], axis=1), (2,))
    src_ex = np.repeat(p.rep_exon_off[order], ne) + (np.arange(I) - np.repeat(eoff, ne))
    dest_ex = np.arange(I)
    if mut == "stream_reset_4096":                                   # a tile's piece written chunk over chunk
        tile_e0 = np.repeat(eoff[idx // TILE * TILE], ne)
        dest_ex = tile_e0 + (dest_ex - tile_e0) % LEX
    estream = np.zeros((I, 2), np.int32)
    estream[dest_ex] = np.stack([p.ex_ts[src_ex], p.ex_te[src_ex]], axis=1)
    return dict(order=order, start=start.astype(np.int32), pmax=pmax.astype(np.int32), exons=exons, stream=stream, estream=estream)


def hist_packed(parts):
    """fseg_upload's choice of S1's counter width: packed unless a position of a partition of more than 32 767 lanes can count past 65 535."""
    for p in parts:
        if 2 * int(p.rep_weight.sum()) <= COUNT16:
            continue
        w = np.repeat(p.rep_weight.astype(np.int64), np.diff(p.rep_exon_off))
        _, inv = np.unique(np.concatenate([p.ex_ts, p.ex_te]), return_inverse=True)
        if np.bincount(inv, np.concatenate([w, w])).max() > COUNT16:
            return False
    return True


def chunk_size(parts):
    npos = sum(int((p.iv_end.astype(np.int64) - p.iv_start + 1).sum()) for p in parts)
    chunk = CHUNK16 if hist_packed(parts) else CHUNK32
    while chunk > CHUNK_MIN and npos // chunk < CHUNK_WGS:
        chunk >>= 1
    return chunk


def chunks(p, chunk):
    """The partition's histogram chunks: (first position, positions, genomic coordinate of the first / the last position)."""
    pos_off = np.concatenate([[0], np.cumsum(p.iv_end.astype(np.int64) - p.iv_start + 1)])
    q0 = np.arange(0, pos_off[-1], chunk)
    q1 = np.minimum(q0 + chunk, pos_off[-1]) - 1

    def coord(q):
        k = np.searchsorted(pos_off, q, "right") - 1
        return p.iv_start[k] + q - pos_off[k]
    return q0, q1 - q0 + 1, coord(q0), coord(q1)


def model_ranges(p, m, chunk, mut=None):
    """int64[chunks][4]: (p0, n, llo, lhi), relative to the partition's first position and first lane."""
    q0, n, glo, ghi = chunks(p, chunk)
    glo = glo + dict(glo_plus=1, glo_minus=-1).get(mut, 0)
    ghi = ghi + dict(ghi_plus=1, ghi_minus=-1).get(mut, 0)
    rows = np.zeros((len(q0), 4), np.int64)
    rows[:, 0], rows[:, 1] = q0, n
    for c in range(len(q0)):
        llo = int(np.searchsorted(m["pmax"], glo[c], "right" if mut == "llo_right" else "left"))
        rows[c, 2] = llo
        rows[c, 3] = llo + int(np.searchsorted(m["start"][llo:], ghi[c], "left" if mut == "lhi_left" else "right"))
    return rows


def model_batch(parts, mut=None):
    """What the taps of a batch must hold: lane_start, lane_pmax, lane_exons, lane_stream, exon_stream, hist_ranges, and the census
    words the batch decides (hist16; lane_sort without the switch)."""
    chunk = chunk_size(parts)
    seen = {}                                                        # a batch may repeat a partition many times over
    out = dict(lane_start=[], lane_pmax=[], lane_exons=[], lane_stream=[], exon_stream=[], hist_ranges=[])
    l0 = e0 = p0 = 0
    lane_off = [0]
    for p in parts:
        if id(p) not in seen:
            m = model_partition(p, mut)
            seen[id(p)] = (m, model_ranges(p, m, chunk, mut))
        m, rows = seen[id(p)]
        out["lane_start"].append(m["start"]); out["lane_pmax"].append(m["pmax"])
        out["lane_exons"].append(m["exons"] + e0); out["lane_stream"].append(m["stream"] + e0); out["exon_stream"].append(m["estream"])
        out["hist_ranges"].append(rows + np.array([p0, 0, l0, l0]))
        l0 += len(m["start"]); e0 += len(p.ex_ts); p0 += int((p.iv_end.astype(np.int64) - p.iv_start + 1).sum())
        lane_off.append(l0)
    out = {k: np.concatenate(v) for k, v in out.items()}
    out["lane_stream"] = out["lane_stream"].astype(np.int32)
    out["part_lane_off"] = np.array(lane_off)
    out["chunk"] = chunk
    out["hist16"] = int(hist_packed(parts))
    out["lane_sort"] = int(max(p.n_reps for p in parts) > SORT_MAX)
    return out


TAPS = ("lane_start", "lane_pmax", "lane_exons", "lane_stream", "exon_stream", "hist_ranges")


def differs(a, b):
    return [k for k in TAPS if not np.array_equal(a[k], b[k])]


# ---- validation: the reference's asserts, read by read ----------------------------------------------------------------------------------
RULES = ("ends", "order", "interval", "no_exons")          # in the order check_prep settles a tie (the error word's bits)
MESSAGES = dict(ends="rep %d: exon with start >= end (py/freddie_segment.py:160)",
                order="rep %d: exons out of order (py/freddie_segment.py:158)",
                interval="rep %d: an exon does not lie inside one tint interval (py/freddie_segment.py:668)",
                no_exons="rep %d has no exons")


def offenders(parts):
    """py/freddie_segment.py:158-161 and :666-668 restated as a loop over the batch's reps (a rep without exons is this library's own
    rule: the reference cannot write one).  Returns {rule: smallest offending rep of the batch}."""
    bad = {}
    r = 0
    for p in parts:
        ivs = list(zip(p.iv_start.tolist(), p.iv_end.tolist()))

        def pos_to_Y_idx(q):                                         # :652-657: the interval whose positions s..e hold q (KeyError: None)
            for k, (s, e) in enumerate(ivs):
                if s <= q <= e:
                    return k
            return None
        for i in range(p.n_reps):
            ex = list(zip(p.ex_ts[p.rep_exon_off[i]:p.rep_exon_off[i + 1]].tolist(), p.ex_te[p.rep_exon_off[i]:p.rep_exon_off[i + 1]].tolist()))
            broke = []
            if not ex:
                broke.append("no_exons")
            if not all(aet <= bst for (_, aet), (bst, _) in zip(ex[:-1], ex[1:])):          # :158
                broke.append("order")
            if not all(st < et for st, et in ex):                                              # :160
                broke.append("ends")
            for ts, te in ex:                                                                  # :666-668
                ks, ke = pos_to_Y_idx(ts), pos_to_Y_idx(te)
                if ks is None or ke is None or ks != ke:
                    broke.append("interval")
            for rule in broke:
                bad.setdefault(rule, r)
            r += 1
    return bad


def verdict(parts):
    """None, or (rule, rep) as check_prep names it: the rule whose smallest offending rep is smallest."""
    bad = offenders(parts)
    if not bad:
        return None
    rule = min(bad, key=lambda k: (bad[k], RULES.index(k)))
    return rule, bad[rule]


# ---- builders ----------------------------------------------------------------------------------------------------------------------------
def scattered(n, seed, base=1000, spread=None):
    """n single-exon reps of a few positions, first positions drawn from `spread` values (ties wherever n > spread)."""
    rng = np.random.default_rng(seed)
    first = base + rng.integers(0, spread or max(4, n // 2), n)
    last = first + rng.integers(1, 30, n)
    return single(first, last)


N_SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1025, 2047, 2048)
N_ORDER = (1, 2048, 2, 1025, 3, 513, 63, 257, 64, 2047, 65, 1023, 255, 512, 256, 511)      # neighbours differ in tile count


@functools.lru_cache(maxsize=None)
def n_part(n):
    return scattered(n, 100 + n, base=1000 + 37 * n)


def ties_partition(n, runs, how, seed=7):
    """n reps whose sorted first positions rise by 3 except inside `runs` = [(a, b)]: sorted indices a..b share one first position.
    Last positions do not follow the first ones, so an order by last position is another order.  how: the input's order."""
    step = np.full(n, 3)
    for a, b in runs:
        step[a + 1:b + 1] = 0
    first = 5000 + np.cumsum(step)
    rng = np.random.default_rng(seed)
    last = first + rng.integers(1, 40, n)
    perm = dict(sorted=np.arange(n), reverse=np.arange(n)[::-1], shuffled=rng.permutation(n))[how]
    return single(first[perm], last[perm])


def order_partitions():
    runs = [(250, 260), (505, 520)]                       # across the edge of tile 0, and across index 512 of the 1 024-key network
    parts = {"T-sorted": ties_partition(700, runs, "sorted"), "T-reverse": ties_partition(700, runs, "reverse"),
             "T-shuffled": ties_partition(700, runs, "shuffled")}
    rng = np.random.default_rng(11)
    one = np.full(700, 9000)
    parts["T-one-first"] = single(one, one + rng.permutation(700) + 1)
    hi = ties_partition(300, [(120, 135)], "shuffled", seed=3)
    for name, shift in (("T-2^30", 2 ** 30 + 12345), ("T-2e9", 2_000_000_000)):
        parts[name] = single(firsts(hi).astype(np.int64) + shift, lasts(hi).astype(np.int64) + shift)
    return parts


def max_partition(n, where, seed=5):
    """n single-exon reps with strictly rising first positions, given to the library shuffled.  where: the sorted index of the one rep
    whose last position lies beyond every other's, or 'rising' / 'falling' (last positions strictly so, in sorted order)."""
    i = np.arange(n)
    if where == "falling":
        first, last = 1000 + i, 1000 + 2 * n + 10 - i
    else:
        first, last = 1000 + 2 * i, 1000 + 2 * i + 3
        if where != "rising":
            last = last.copy(); last[where] = 1000 + 2 * n + 50
    perm = np.random.default_rng(seed).permutation(n)
    return single(first[perm], last[perm], ivs=[(990, 1000 + 2 * n + 100)])


M_WHERE = (0, 63, 64, 255, 256, "last", "rising", "falling")
M_SIZES = (300, 2049, 16385, 16640)


def max_batch(n):
    parts = [max_partition(n, n - 1 if w == "last" else w) for w in M_WHERE]
    if n == 16640:
        parts.insert(1, max_partition(16384, 0))          # exactly 64 blocks beside the 65-block ones
    return parts


W_HEAVY = 70005


def weight_batch():
    n = 600

    def part(weights, seed):
        p = scattered(n, seed, spread=10 * n)
        p.rep_weight = np.asarray(weights, np.int32)
        return p

    def heavy_at(j, seed):                                 # the heavy rep at sorted index j
        p = part(np.ones(n), seed)
        p.rep_weight[sorted_order(p)[j]] = W_HEAVY
        return p
    rng = np.random.default_rng(21)
    return [part(np.ones(n), 30), heavy_at(0, 31), heavy_at(n - 1, 32), heavy_at(255, 33), heavy_at(256, 34), part(rng.integers(2, 6, n), 35)]


def exon_partition(counts, weights=None, seed=0):
    """Reps of counts[i] exons, given in sorted order of their first positions: exon j of rep i is (s_i + 10 j, s_i + 10 j + 5), the
    first positions s_i = 1000 + 3 i.  One long interval holds them all.  The reps are handed over shuffled."""
    counts = np.asarray(counts, np.int64)
    n = len(counts)
    s = 1000 + 3 * np.arange(n)
    j = np.arange(counts.sum()) - np.repeat(np.cumsum(counts) - counts, counts)
    ts = np.repeat(s, counts) + 10 * j
    perm = np.random.default_rng(seed).permutation(n)
    off = np.cumsum(counts) - counts
    idx = np.concatenate([np.arange(off[r], off[r] + counts[r]) for r in perm])
    w = None if weights is None else np.asarray(weights)[perm]
    return build([(900, int(ts.max()) + 100)], counts[perm], ts[idx], ts[idx] + 5, w)


def tile_counts(total, n=TILE):
    c = np.full(n, total // n)
    c[:total % n] += 1
    return c


X_TOTALS = (4095, 4096, 4097, 8192, 8193)


def exon_batch():
    parts = [exon_partition(tile_counts(t), seed=t) for t in X_TOTALS]
    straddle = np.concatenate([tile_counts(4080, 255), [40], tile_counts(300, 44)])      # sorted rep 255 owns exons 4 080..4 119 of tile 0
    parts.append(exon_partition(straddle, seed=1))
    long_ = np.concatenate([np.full(10, 3), [4097], np.full(20, 2), [9000], np.full(5, 1)])
    parts.append(exon_partition(long_, seed=2))
    parts.append(exon_partition(np.ones(300, np.int64), seed=3))                           # one exon a rep
    rng = np.random.default_rng(4)
    parts.append(exon_partition(tile_counts(5000, 300), weights=rng.integers(1, 5, 300), seed=4))   # copies share one stream range
    return parts


TINY = [single([100, 120], [130, 125]), single([5000], [5040]), single([70, 60, 65], [90, 95, 66]), single([300, 300], [310, 305]),
        single([2 ** 20], [2 ** 20 + 9]), single([44, 40, 42], [50, 49, 48]), single([900], [901])]
B_COUNTS = (1, 2, 3, 4, 5, 8, 9, 256, 257)
B_LARGE = GRID + 1 + 300


def tiny_batch(n):
    return [TINY[i % 7] for i in range(n)]


H_BOUND_CHUNKS, H_EMPTY_CHUNK = (0, 1, 3, 4, 8), 6


def hist_partition(chunk):
    """Three intervals A, B, C of 3, about 1.5 and about 4 chunks: chunk 1 lies in the middle of A, chunk 3 starts on B's first
    position, chunk 4 spans the gap between B and C, chunk 6 is reached by no read, chunk 8 is the (short) last one.  For each of
    chunks 0, 1, 3, 4 and 8: reads whose last position is glo - 1 and glo, whose first is ghi and ghi + 1 -- or, where that
    coordinate is no position of the partition or no exon can have it, the nearest one that can."""
    c = chunk
    lens = [3 * c, c + c // 2 - 24, 4 * c - c // 4 - 11]
    ivs, s = [], 10000
    for n in lens:
        ivs.append((s, s + n - 1)); s += n + 500
    p = build(ivs, [1], [ivs[0][0]], [ivs[0][0] + 1])
    q0, n, glo, ghi = chunks(p, c)
    assert len(q0) == 9 and glo[3] == ivs[1][0] and ghi[4] > ivs[2][0] and glo[4] < ivs[1][1] and n[8] < c

    def inside(a, b):
        return any(s <= a and b <= e for s, e in ivs)
    reads = set()
    for ch in H_BOUND_CHUNKS:
        for a, b in ((glo[ch] - 6, glo[ch] - 1), (glo[ch] - 5, glo[ch]), (ghi[ch], ghi[ch] + 5), (ghi[ch] + 1, ghi[ch] + 6)):
            if inside(a, b):
                reads.add((int(a), int(b)))
    reads.add((ivs[0][1] - 4, ivs[0][1]))                                # the last position in front of chunk 3 that a read can end on
    reads.add((ivs[1][0], ivs[1][0] + 3))                                # ... and the read that starts on glo of chunk 3
    reads.add((ivs[2][1] - 7, ivs[2][1]))                                # the partition's last position
    reads = sorted(reads)
    return util.hand(ivs, [[r] for r in reads[::-1]])                    # given in falling order


def filler():
    """What tests/test_gpu_hist_packed.chunk_edges uses: enough positions for chunks of full size."""
    n_fill = CHUNK_WGS * CHUNK16 // 4
    f_iv = [(100 + i * (n_fill + 10), 100 + i * (n_fill + 10) + n_fill - 1) for i in range(4)]
    reads = [[(a + 5, a + 90), (a + 100, a + 400), (a + 1000, b - 7)] for a, b in f_iv] + [[(f_iv[0][0] + 7, f_iv[0][0] + 300)]]
    return util.hand(f_iv, reads)


V_IVS = [(1000, 3000), (3100, 5000), (5100, 7000)]


def v_reps(n, seed, k=0):
    """n two-exon reps (a, a + 20), (a + 30, a + 50) inside interval k of V_IVS."""
    a = V_IVS[k][0] + 5 + np.random.default_rng(seed).integers(0, 1800, n)
    return [[(int(x), int(x) + 20), (int(x) + 30, int(x) + 50)] for x in a]


def accepted_batch():
    s0, e0 = V_IVS[0]
    s2, e2 = V_IVS[2]
    return [util.hand(V_IVS, [[(s0, s0 + 9), (e0 - 9, e0)], [(s0, e0)]] + v_reps(5, 1)),                   # ts == iv_start, te == iv_end
            util.hand(V_IVS, [[(1100, 1200), (1200, 1300), (1300, 1400)], [(3100, 3200), (3200, 5000)]]),     # prev_te == ts
            util.hand(V_IVS, v_reps(6, 2, 0)),                                                              # wholly in the first interval
            util.hand(V_IVS, v_reps(6, 3, 2) + [[(s2, e2)]]),                                               # wholly in the last interval
            util.hand(V_IVS, [[(s2 + 7, s2 + 90)], [(s2, s2 + 1), (e2 - 1, e2)]] + v_reps(3, 4, 1))]        # the first exon in the last interval


def v_base(big):
    """The good batch the refusals are cut from: 300 + 40 reps, or 300 + 2 049 (the block path by itself)."""
    return [util.hand(V_IVS, v_reps(300, 10)), util.hand(V_IVS, v_reps(2049 if big else 40, 11, 1))]


def _set(ex):
    def f(exons):
        for i, x in ex.items():
            exons[i] = x
        return exons
    return f


# rule, what becomes of the rep's exons [(a, a + 20), (a + 30, a + 50)]: every bad exon stays clear of k_hist's counters (module docstring)
REFUSALS = {
    "ts==te": ("ends", lambda ex: [(ex[0][0], ex[0][0]), ex[1]]),
    "ts>te": ("ends", lambda ex: [(ex[0][1], ex[0][0]), ex[1]]),                     # both ends inside the rep's interval
    "prev_te==ts+1": ("order", lambda ex: [ex[0], (ex[0][1] - 1, ex[1][1])]),
    "in-the-gap": ("interval", lambda ex: [ex[0], (3040, 3060)] if ex[0][0] < 3000 else [ex[0], (5020, 5060)]),
    "spans-two": ("interval", lambda ex: [ex[0], (2990, 3110)] if ex[0][0] < 2900 else [ex[0], (4990, 5110)]),
    "te==iv_end+1": ("interval", lambda ex: [ex[0], (2980, 3001)] if ex[0][0] < 2900 else [ex[0], (4980, 5001)]),
    "before-the-first": ("interval", lambda ex: [(900, 950), ex[1]]),
    "after-the-last": ("interval", lambda ex: [ex[0], (7010, 7050)]),
    "no-exons": ("no_exons", lambda ex: []),
}
PLACES = ("rep-0", "rep-255", "rep-256", "last-rep", "in-2049")


def place(where):
    """(big, the batch's rep)"""
    return dict([("rep-0", (False, 0)), ("rep-255", (False, 255)), ("rep-256", (False, 256)), ("last-rep", (False, 339)), ("in-2049", (True, 300 + 1000))])[where]


def spoiled(parts, edits):
    """`parts` with the exons of some of the batch's reps rewritten: edits = {rep: function of the rep's exon list}."""
    out, r0 = [], 0
    for p in parts:
        reads = [list(zip(p.ex_ts[a:b].tolist(), p.ex_te[a:b].tolist())) for a, b in zip(p.rep_exon_off[:-1], p.rep_exon_off[1:])]
        for r, f in edits.items():
            if r0 <= r < r0 + p.n_reps:
                reads[r - r0] = f(reads[r - r0])
        ivs = list(zip(p.iv_start.tolist(), p.iv_end.tolist()))
        ex = np.array([x for rd in reads for x in rd], np.int64).reshape(-1, 2)
        out.append(build(ivs, [len(rd) for rd in reads], ex[:, 0], ex[:, 1]))
        r0 += p.n_reps
    return out


def refused(name, where):
    big, r = place(where)
    return spoiled(v_base(big), {r: REFUSALS[name][1]})


# two bad reps: different rules in different blocks and partitions (the smaller rep is named), and one rule twice
PAIRS = {"interval@20+ends@310": {20: REFUSALS["after-the-last"][1], 310: REFUSALS["ts==te"][1]},
         "ends@320+interval@5": {320: REFUSALS["ts>te"][1], 5: REFUSALS["spans-two"][1]},
         "order@257+order@300": {257: REFUSALS["prev_te==ts+1"][1], 300: REFUSALS["prev_te==ts+1"][1]}}


# ---- the batches ---------------------------------------------------------------------------------------------------------------------------
# name -> (partitions, parameters of the whole run)
@functools.lru_cache(maxsize=None)
def batch(name):
    g = name.split("-")[0]
    if g == "N":
        what = name[2:]
        if what == "all":
            return [n_part(n) for n in N_ORDER], ENDS
        if what == "all+2049":
            return [n_part(n) for n in N_ORDER[:8]] + [scattered(2049, 77, base=400000)] + [n_part(n) for n in N_ORDER[8:]], ENDS
        return [n_part(int(what))], ENDS
    if g == "T":
        parts = order_partitions()
        if name == "T-order":
            return [parts[k] for k in ("T-sorted", "T-reverse", "T-shuffled", "T-one-first", "T-2^30")], ENDS
        if name == "T-2e9":
            return [parts["T-2e9"]], ENDS
        if name == "T-partition-word":                    # a later partition's coordinates lie below an earlier one's
            return [parts["T-2^30"], parts["T-shuffled"], n_part(65), parts["T-one-first"], n_part(3)], ENDS
    if g == "M":
        return max_batch(int(name[2:])), ENDS
    if name == "W":
        return weight_batch(), ENDS
    if name == "X":
        return exon_batch(), ENDS
    if g == "B":
        n = int(name[2:])
        return tiny_batch(n), ENDS
    if name == "H-1024":
        return [n_part(3), hist_partition(CHUNK_MIN)], ENDS
    if name == "H-full":
        return [n_part(3), hist_partition(CHUNK16), filler()], ENDS
    if name == "V-accepted":
        return accepted_batch(), ENDS
    if name == "V-base":
        return v_base(False), ENDS
    raise KeyError(name)


BATCHES = (["N-%d" % n for n in N_SIZES] + ["N-all", "N-all+2049", "T-order", "T-2e9", "T-partition-word"] + ["M-%d" % n for n in M_SIZES]
           + ["W", "X"] + ["B-%d" % n for n in B_COUNTS + (B_LARGE,)] + ["H-1024", "H-full", "V-accepted", "V-base"])

# the mutations each batch was built to see (tests/test_lane_cases_host.py asserts every one, and that every mutation has a batch).
# key_unsigned has none: it reorders only negative positions, which are not built -- the host test shows it
# changes nothing at 2^30 and 2 000 000 000 and what it would change below zero.
SEES = {
    "T-order": ("tie_reverse", "tie_by_last"),
    "N-all": ("tie_reverse", "pmax_reset_64", "pmax_reset_256", "pmax_exclusive", "lane_carry_dropped"),
    "M-300": ("pmax_reset_64", "pmax_reset_256", "pmax_exclusive"),
    "M-2049": ("pmax_reset_64", "pmax_reset_256", "pmax_exclusive"),
    "M-16385": ("pmax_reset_64", "pmax_reset_256", "pmax_reset_16384", "pmax_exclusive"),
    "M-16640": ("pmax_reset_64", "pmax_reset_256", "pmax_reset_16384", "pmax_exclusive"),
    "W": ("lane_carry_dropped",),
    "X": ("stream_reset_4096", "lane_carry_dropped"),
    "H-1024": ("llo_right", "lhi_left", "glo_plus", "glo_minus", "ghi_plus", "ghi_minus"),
    "H-full": ("llo_right", "lhi_left", "glo_plus", "glo_minus", "ghi_plus", "ghi_minus"),
}


@functools.lru_cache(maxsize=None)
def oracles(name):
    parts, params = batch(name)
    seen = {}
    for p in parts:
        if id(p) not in seen:
            seen[id(p)] = util.run_oracle(p, params)
    return [seen[id(p)] for p in parts]
