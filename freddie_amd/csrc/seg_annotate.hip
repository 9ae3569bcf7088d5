// seg_annotate.hip -- per-READ annotation of a segmented batch: the unaligned gaps between a read's runs of label 1, its soft
// clips and its poly-A / poly-T tails (get_unaligned_gaps_and_polyA and helpers, py/freddie_segment.py:289-472), as flat arrays in
// the layout of fhost_segments (include/freddie_host.h).  The reads of a rep share the (ts, te) exons and the label row; query
// coordinates, CIGARs, strand and sequence are the read's own (AnnotIn, uploaded by fseg_annotate).
//
// Decomposition (a lane per read, a lane per window for the poly pass; the poly recurrence is sequential per window):
//   k_an_count   runs of label 1 of the read's row -> gap / clip counts, q_ssc and q_esc (:375-390)
//   k_an_poly    the two soft-clip windows of a read: best poly run (:352-367 with the caller's choice :397-408, :427-439)
//   k_an_scan1/2/3   exclusive scan of the three per-read counts (gaps, clips, polys) into the CSR offsets
//   k_an_emit    internal gaps (j1, j2, len) with the CIGAR threading (:289-349, :455-471), clips, polys, tail category, key tokens
// Every reference assert is a per-read status code (kAn* below), never a fault: a CIGAR that runs out stops the walk, a window
// index outside the sequence is a code; the smallest failing read of the batch is kept in AnnotOut::first_bad.
// Label rows and sequences are read as whole 32-bit words (16 two-bit codes); all-zero label words are skipped.
#include "seg_kernels.h"

namespace fseg {

namespace {

// 16 labels [16 w, 16 w + 16) of the arena as two-bit codes, from either form of the arena
__device__ inline unsigned an_lab_word(const AnnotIn &a, i64 w) {
    if (a.lab2) return a.lab2[w];
    const uint4 v = reinterpret_cast<const uint4 *>(a.lab1)[w];        // ASCII '0' / '1' / '2': the low two bits are the code
    auto pk = [](unsigned x) { x &= 0x03030303u; return (x | (x >> 6) | (x >> 12) | (x >> 18)) & 0xffu; };
    return pk(v.x) | (pk(v.y) << 8) | (pk(v.z) << 16) | (pk(v.w) << 24);
}

// f(i, j) for every maximal run [i, j] of label 1 in the row of S labels that starts at label g0 of the arena, ascending
template <typename F>
__device__ inline void an_for_runs(const AnnotIn &a, i64 g0, i64 S, F f) {
    if (S <= 0) return;
    const i64 g1 = g0 + S;
    i64 rs = -1;
    for (i64 w = g0 >> 4; w <= (g1 - 1) >> 4; ++w) {
        const i64 base = w << 4;
        unsigned x = an_lab_word(a, w);
        unsigned ones = x & ~(x >> 1) & 0x55555555u;
        if (base < g0) ones &= ~0u << (2 * (int)(g0 - base));
        if (base + 16 > g1) ones &= (1u << (2 * (int)(g1 - base))) - 1u;
        if (ones == 0u) {                                   // (rows are mostly '0')
            if (rs >= 0) { f(rs, base - 1 - g0); rs = -1; }
            continue;
        }
        if (ones == 0x55555555u) { if (rs < 0) rs = base - g0; continue; }
        for (int k = 0; k < 16; ++k) {
            const i64 g = base + k;
            if ((ones >> (2 * k)) & 1u) { if (rs < 0) rs = g - g0; }
            else if (rs >= 0) { f(rs, g - 1 - g0); rs = -1; }
        }
    }
    if (rs >= 0) f(rs, S - 1);
}

struct AnRead {       // where a read's exons live: (ts, te) with its rep, (qs, qe, CIGAR) with the read
    i64 e0, q0;
    int m;
    i64 g0, S;        // its rep's label row
    const int *fp;    // its partition's final positions (S + 1 of them)
};

__device__ inline AnRead an_read(const AnnotIn &a, i64 r) {
    AnRead R;
    const int p = a.read_part[r];
    const i64 rep = a.part_rep_off[p] + a.read_rep[r];
    R.e0 = a.rep_exon_off[rep];
    R.m = (int)(a.rep_exon_off[rep + 1] - R.e0);
    R.q0 = a.read_q_off[r];
    const i64 f0 = a.pfo[p], F = a.pfo[p + 1] - f0;
    R.S = F - 1;
    R.fp = a.final_pos + f0;
    R.g0 = a.label_off[p] + (i64)a.read_rep[r] * R.S;
    return R;
}

// forward_thread_cigar (:289-304): every op is clipped to the goal, insertions too
__device__ inline int an_thread(const AnnotIn &a, i64 qx, i64 t_goal, i64 t_pos, i64 q_pos, i64 &out) {
    if (t_pos > t_goal) return kAnThreadOrder;
    i64 idx = a.cig_off[qx];
    const i64 end = a.cig_off[qx + 1];
    while (t_pos < t_goal) {
        if (idx >= end) return kAnCigarShort;
        i64 step = a.cig_len[idx];
        if (step > t_goal - t_pos) step = t_goal - t_pos;
        const unsigned char op = a.cig_op[idx];
        if (op == 'M' || op == 'X' || op == '=') { t_pos += step; q_pos += step; }
        else if (op == 'D') t_pos += step;
        else if (op == 'I') q_pos += step;
        ++idx;
    }
    out = q_pos;
    return 0;
}

// get_interval_start (:307-326); `from`: the exon the scan starts at (the queries of a read come with ascending positions)
__device__ inline int an_after(const AnnotIn &a, const AnRead &R, i64 start, i64 &q, i64 &slack, int &from) {
    for (int x = from; x < R.m; ++x) {
        const i64 ts = a.ex_ts[R.e0 + x], te = a.ex_te[R.e0 + x];
        if (te < start) continue;
        from = x;
        const i64 qs = a.qs[R.q0 + x], qe = a.qe[R.q0 + x];
        if (start < ts) { q = qs; slack = start - ts; }
        else {
            const int rc = an_thread(a, R.q0 + x, start, ts, qs, q);
            if (rc) return rc;
            slack = 0;
        }
        if (!(slack <= 0 && qs <= q && q <= qe)) return kAnStartRange;
        return 0;
    }
    return kAnStartNone;
}

// get_interval_end (:329-349): the LAST exon with ts <= end, found forwards from `from` (an exon known to start at or before an
// earlier, smaller position; 0 finds the same exon as the reference's backward scan)
__device__ inline int an_before(const AnnotIn &a, const AnRead &R, i64 end, i64 &q, i64 &slack, int &from) {
    if (R.m <= 0) return kAnEndNone;
    int x = from;
    while (x + 1 < R.m && a.ex_ts[R.e0 + x + 1] <= end) ++x;
    if (a.ex_ts[R.e0 + x] > end) return kAnEndNone;
    from = x;
    const i64 ts = a.ex_ts[R.e0 + x], te = a.ex_te[R.e0 + x];
    const i64 qs = a.qs[R.q0 + x], qe = a.qe[R.q0 + x];
    if (te < end) { q = qe; slack = te - end; }
    else {
        const int rc = an_thread(a, R.q0 + x, end, ts, qs, q);
        if (rc) return rc;
        slack = 0;
    }
    if (!(slack <= 0 && 0 <= q && q <= qe)) return kAnEndRange;
    return 0;
}

}  // namespace

// ---- runs, counts and the read's ends ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_an_count(AnnotIn a, AnnotOut o) {
    for (i64 r = (i64)blockIdx.x * 256 + threadIdx.x; r < a.n_read; r += (i64)gridDim.x * 256) {
        const AnRead R = an_read(a, r);
        i64 n_runs = 0, first = 0, last = 0;
        an_for_runs(a, R.g0, R.S, [&](i64 i, i64 j) { if (n_runs == 0) first = i; last = j; ++n_runs; });
        int st = 0;
        i64 q_ssc = 0, q_esc = 0;
        if (n_runs > 0) {                                       // a read with no label 1 has nothing at all (:372-373)
            i64 slack;
            int from = 0;
            st = an_after(a, R, R.fp[first], q_ssc, slack, from);
            from = 0;
            if (!st) st = an_before(a, R, R.fp[last + 1], q_esc, slack, from);
            if (!st && !(0 <= q_ssc && q_ssc <= q_esc && q_esc <= (i64)a.seq_len[r])) st = kAnClipOrder;
        }
        o.cnt[r] = n_runs > 0 ? (int)(n_runs - 1) : 0;
        o.cnt[a.n_read + r] = n_runs > 0 ? 2 : 0;
        o.ends[r] = make_int4(n_runs > 0 ? 1 : 0, st, (int)q_ssc, (int)q_esc);
    }
}

// ---- poly tails: a lane per window ---------------------------------------------------------------------------------
// best_poly of the host library, letter for letter: scores +1 / -2 floored at 0, each positive run cut at its LAST maximum, a run
// needs length >= 20 and purity >= 0.85 (an IEEE double division), the purest wins, the first on ties, an A run beats a T run
// unless the T run is strictly purer.  A '-' read is scanned from the end of the stored sequence backwards for the complement.
__global__ void __launch_bounds__(256) k_an_poly(AnnotIn a, AnnotOut o) {
    for (i64 w = (i64)blockIdx.x * 256 + threadIdx.x; w < 2 * a.n_read; w += (i64)gridDim.x * 256) {
        const i64 r = w >> 1;
        const int side = (int)(w & 1);
        const int4 e = o.ends[r];
        int4 res = make_int4(0, 0, 0, 0);                       // (0 none / 1 A / 2 T, first, len, status)
        if (e.x && !e.y) {
            const i64 n = a.seq_len[r];
            const bool minus = a.strand[r] == '-';
            const i64 s0 = side ? e.w : 0, e0 = side ? n : e.z;
            i64 count = e0 - s0;
            if (count != 0) {
                if (count < 0) count = 0;
                const i64 idx0 = minus ? n - 1 - s0 : s0;       // the first element of the window must exist (:355)
                if (idx0 < 0 || idx0 >= n) res.w = kAnPolyIndex;
                else {
                    if (!minus && s0 + count > n) count = n - s0;
                    if (minus && n - 1 - s0 - (count - 1) < 0) count = n - s0;
                    if (count >= 20) {
                        struct Scan { int prev, best_s, in_run, have; i64 run_i, best_i, hits_run, hits_best, first, len; double purity; };
                        Scan sc[2];
                        for (int z = 0; z < 2; ++z) sc[z] = Scan{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0};
                        const unsigned tgt0 = minus ? 1u : 0u, tgt1 = minus ? 0u : 1u;      // class codes: 0 'A', 1 'T', 2 anything else
                        auto emit = [](Scan &z) {
                            const i64 len = z.best_i + 1 - z.run_i;
                            if (len < 20) return;
                            const double purity = __ddiv_rn((double)z.hits_best, (double)len);
                            if (purity < 0.85) return;
                            if (!z.have || purity > z.purity) { z.first = z.run_i; z.len = len; z.purity = purity; z.have = 1; }
                        };
                        auto step = [&](Scan &z, int m, i64 t) {
                            int s = z.prev + (m ? 1 : -2);
                            if (s < 0) s = 0;
                            if (s > 0) {
                                if (!z.in_run) { z.in_run = 1; z.run_i = t; z.best_s = 0; z.hits_run = 0; }
                                z.hits_run += m;
                                if (s >= z.best_s) { z.best_s = s; z.best_i = t; z.hits_best = z.hits_run; }
                            } else if (z.in_run) { emit(z); z.in_run = 0; }
                            z.prev = s;
                        };
                        const i64 lo = minus ? n - s0 - count : s0;            // the window in stored coordinates: [lo, lo + count)
                        const i64 gbase = a.seq_off[r];
                        i64 wi = -1;
                        unsigned wv = 0;
                        for (i64 t = 0; t < count; ++t) {
                            const i64 g = gbase + (minus ? lo + count - 1 - t : lo + t);
                            if ((g >> 4) != wi) { wi = g >> 4; wv = a.seq_cls[wi]; }
                            const unsigned c = (wv >> (2 * (int)(g & 15))) & 3u;
                            step(sc[0], c == tgt0, t);
                            step(sc[1], c == tgt1, t);
                        }
                        if (sc[0].in_run) emit(sc[0]);
                        if (sc[1].in_run) emit(sc[1]);
                        int pick = -1;
                        if (sc[0].have && (!sc[1].have || !(sc[1].purity > sc[0].purity))) pick = 0;
                        else if (sc[1].have) pick = 1;
                        if (pick >= 0) {
                            const i64 first = sc[pick].first, len = sc[pick].len;
                            res.x = pick + 1; res.y = (int)first; res.z = (int)len;
                            if (!side) {
                                const i64 q_ssc = e.z, gap = q_ssc - first - len;
                                if (!(0 <= first && first < q_ssc && 0 <= gap && gap < q_ssc)) res.w = kAnStartPoly;
                            } else {
                                const i64 room = n - e.w;
                                if (!(0 <= first && first < room && room - first > 0)) res.w = kAnEndPoly;
                            }
                        }
                    }
                }
            }
        }
        o.poly[w] = res;
    }
}

// ---- exclusive scan of the three count arrays (gaps, clips, polys -> off: [3][n + 1]) --------------------------------------
constexpr int kAnScanItems = kAnScanItemsPerBlock;      // counts per workgroup: 256 threads x 4

// count i of array arr: 0 gaps, 1 clips (both written by k_an_count), 2 polys (what the read's two windows found)
__device__ inline int an_cnt(const int *cnt, const int4 *poly, int arr, i64 n, i64 i) {
    if (arr < 2) return cnt[(i64)arr * n + i];
    return (poly[2 * i].x ? 1 : 0) + (poly[2 * i + 1].x ? 1 : 0);
}

__global__ void __launch_bounds__(256) k_an_scan1(const int *cnt, const int4 *poly, i64 n, i64 nb, i64 *bsum) {
    __shared__ i64 sh[256];
    const int arr = blockIdx.y;
    const i64 i0 = (i64)blockIdx.x * kAnScanItems + threadIdx.x * 4;
    i64 s = 0;
    for (int k = 0; k < 4; ++k) if (i0 + k < n) s += an_cnt(cnt, poly, arr, n, i0 + k);
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum[(i64)arr * nb + blockIdx.x] = sh[0];
}

// one workgroup per array: the block sums become exclusive prefixes, a contiguous piece per thread
__global__ void __launch_bounds__(256) k_an_scan2(i64 nb, i64 *bsum) {
    __shared__ i64 sh[256];
    i64 *b = bsum + (i64)blockIdx.x * nb;
    const i64 per = (nb + 255) / 256, i0 = (i64)threadIdx.x * per, i1 = i0 + per < nb ? i0 + per : nb;
    i64 s = 0;
    for (i64 i = i0; i < i1; ++i) s += b[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) { i64 run = 0; for (int t = 0; t < 256; ++t) { const i64 v = sh[t]; sh[t] = run; run += v; } }
    __syncthreads();
    i64 run = sh[threadIdx.x];
    for (i64 i = i0; i < i1; ++i) { const i64 v = b[i]; b[i] = run; run += v; }
}

__global__ void __launch_bounds__(256) k_an_scan3(const int *cnt, const int4 *poly, i64 n, i64 nb, const i64 *bsum, i64 *off) {
    __shared__ i64 sh[256];
    const int arr = blockIdx.y;
    const i64 i0 = (i64)blockIdx.x * kAnScanItems + threadIdx.x * 4;
    int v[4];
    i64 s = 0;
    for (int k = 0; k < 4; ++k) { v[k] = i0 + k < n ? an_cnt(cnt, poly, arr, n, i0 + k) : 0; s += v[k]; }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {                       // inclusive scan of the threads' sums
        const i64 add = (int)threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
        __syncthreads();
        sh[threadIdx.x] += add;
        __syncthreads();
    }
    i64 run = bsum[(i64)arr * nb + blockIdx.x] + sh[threadIdx.x] - s;
    i64 *out = off + (i64)arr * (n + 1);
    for (int k = 0; k < 4; ++k) {
        if (i0 + k < n) out[i0 + k] = run;
        run += v[k];
        if (i0 + k == n - 1) out[n] = run;
    }
}

// ---- internal gaps and the derived per-read outputs --------------------------------------------------------------------
// Emission order: a read's gaps ascend by j1 and its key tokens follow them; then the poly entries, the E keys before the S keys,
// and the clips ESC before SSC -- the order the tokens have in a line of the segment TSV ('E' sorts before 'S').  The TSV puts the
// gap tokens in STRING order ("10-..." before "2-..."), which is the writer's business; nothing downstream depends on the order
// of a read's gaps (the rep grouping compares reads with equal label rows, whose j1 lists are equal).
__global__ void __launch_bounds__(256) k_an_emit(AnnotIn a, AnnotOut o) {
    const i64 n = a.n_read;
    const i64 *gap_off = o.off, *clip_off = o.off + (n + 1), *poly_off = o.off + 2 * (n + 1);
    for (i64 r = (i64)blockIdx.x * 256 + threadIdx.x; r < n; r += (i64)gridDim.x * 256) {
        const int4 e = o.ends[r];
        const i64 tok0 = gap_off[r] + poly_off[r];
        o.tok_off[r] = tok0;
        if (r == n - 1) o.tok_off[n] = gap_off[n] + poly_off[n];
        int st = e.y;
        unsigned char tail = 0;
        if (e.x) {
            const int4 ps = o.poly[2 * r], pe = o.poly[2 * r + 1];
            if (!st) st = ps.w;
            if (!st) st = pe.w;
            const i64 length = a.seq_len[r];
            const AnRead R = an_read(a, r);
            // internal gaps (:455-471)
            int *gaps = o.gaps + gap_off[r] * 3;
            unsigned *tok = o.tok + tok0;
            i64 k = 0, prev_last = -1;
            int xa = 0, xb = 0, gst = 0;
            an_for_runs(a, R.g0, R.S, [&](i64 i, i64 j) {
                if (prev_last >= 0) {
                    const i64 last1 = prev_last, first2 = i;
                    i64 q_a = 0, q_b = 0, slack_a = 0, slack_b = 0, size = 0;
                    if (!gst) gst = an_before(a, R, R.fp[last1 + 1], q_a, slack_a, xb);
                    if (!gst) gst = an_after(a, R, R.fp[first2], q_b, slack_b, xa);
                    if (!gst && !(0 < q_a && q_a <= q_b && q_b < length)) gst = kAnGapOrder;
                    if (!gst) {
                        size = q_b - q_a + slack_a + slack_b;
                        if (size < 0) size = 0;
                        if (!(size < length && last1 < first2)) gst = kAnGapSize;
                    }
                    if (gst) size = 0;
                    gaps[3 * k] = (int)last1; gaps[3 * k + 1] = (int)first2; gaps[3 * k + 2] = (int)size;
                    tok[k] = size > 10 ? (unsigned)size : 0u;
                    ++k;
                }
                prev_last = j;
            });
            if (!st) st = gst;
            // clips, polys, tail, the poly key tokens: the end of the read first
            int *clips = o.clips + clip_off[r] * 2, *polys = o.polys + poly_off[r] * 3;
            const i64 esc = pe.x ? length - e.w - pe.y : length - e.w, ssc = ps.x ? (i64)ps.y : (i64)e.z;
            clips[0] = 1; clips[1] = (int)esc; clips[2] = 0; clips[3] = (int)ssc;
            int np = 0;
            if (pe.x) {
                polys[0] = 2 + (pe.x - 1); polys[1] = pe.z; polys[2] = pe.y;
                tok[k++] = 0x80000000u | 0x40000000u | (pe.y > 10 ? (unsigned)pe.y : 0u);
                tail = pe.z > 10 ? 2 : 0;
                ++np;
            }
            if (ps.x) {
                const int gap = e.z - ps.y - ps.z;
                polys[3 * np] = ps.x - 1; polys[3 * np + 1] = ps.z; polys[3 * np + 2] = gap;
                tok[k++] = 0x80000000u | (gap > 10 ? (unsigned)gap : 0u);
                tail = ps.z > 10 ? 1 : 0;
                ++np;
            }
            if (np != 1) tail = 0;
        }
        o.tail[r] = tail;
        o.status[r] = st;
        if (st) atomicMin(o.first_bad, (unsigned long long)r);
    }
}

// part_final_off of the resident run: the per-interval offsets at the partitions' first intervals
__global__ void __launch_bounds__(256) k_an_pfo(int n_part, const i64 *part_iv_off, const i64 *final_off, i64 *pfo) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p <= n_part) pfo[p] = final_off[part_iv_off[p]];
}

}  // namespace fseg
