// clu_exact.h -- what one thread of the exact small-problem solve (fclu_round_exact; k_exact_prep / k_exact_search in freddie_cluster.hip)
// computes for one column set S of a problem of at most 24 columns: the conflict test, the gap rows, the cost and the packed key.  Host and
// device: tools/exact_host_check.cpp runs the same functions over every mask of a problem and is compared with the Python mirror
// (cluster_solve.exact_small) where there is no GPU.  The definition is the mirror's docstring.
//
// The transposed table: S is a 32-bit mask, bit c = column c.  Informative segment k of the problem owns two words, tab[2 k] = the columns
// with I = 1 there (its support) and tab[2 k + 1] = the columns with C = 1 there; e_k = (support & S) != 0 and the members' corrections at
// k are popcount(corr & S).  conf[c] = the columns in conflict with c.  A gap group's segments carry their support word (gsup) beside
// their length, so G_g = the lengths whose support meets S.  Nothing here indexes with a value it has read without clamping it first.
#ifndef CLU_EXACT_H
#define CLU_EXACT_H

#include <stdint.h>

#if defined(__HIPCC__)
#define EX_HD __host__ __device__ __forceinline__
#else
#define EX_HD inline
#endif

typedef long long ex_i64;
typedef unsigned long long ex_u64;

constexpr int kExactMaxCols = 24;              // a mask fits the key's low 24 bits
constexpr ex_u64 kExactKeyNone = ~0ull;        // no feasible set (cost2 < 2^36: no key of a set reaches it)

EX_HD int ex_popc(unsigned x) { return __builtin_popcount(x); }
EX_HD int ex_ctz(unsigned x) { return __builtin_ctz(x); }
EX_HD ex_i64 ex_clamp(ex_i64 v, ex_i64 lo, ex_i64 hi) { return v < lo ? lo : v > hi ? hi : v; }

// the smallest key wins: the smaller cost2, then the smaller mask
EX_HD ex_u64 ex_key(ex_i64 cost2, unsigned S) { return ((ex_u64)cost2 << kExactMaxCols) | (ex_u64)(S & 0xffffffu); }
EX_HD ex_i64 ex_key_cost2(ex_u64 key) { return (ex_i64)(key >> kExactMaxCols); }
EX_HD unsigned ex_key_mask(ex_u64 key) { return (unsigned)(key & 0xffffffull); }

// an incompatible pair lies inside S
EX_HD bool ex_conflict(unsigned S, const unsigned *conf, int R) {
    for (unsigned m = S; m; m &= m - 1) {
        const int c = (int)ex_clamp(ex_ctz(m), 0, R - 1);
        if (conf[c] & S) return true;
    }
    return false;
}

// (lo_f G - offset - slack > l + 1e-9) or (hi_f G + offset + slack < l - 1e-9) in doubles, every operation rounded on its own and in this
// order, never fused: the yardstick's test (tests/round_util.py, subset_cost), tolerance included.  slack: 0 for a member's row,
// MAX_ISOFORM_LG for the row of a column outside the set.
EX_HD bool ex_row_violated(ex_i64 G, int l, double lo_f, double hi_f, int offset, ex_i64 slack) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double g = (double)G, o = (double)offset, s = (double)slack, len = (double)l;
    const double lo = lo_f * g;
    const double hi = hi_f * g;
    const double a = lo - o, b = hi + o;
    const double a2 = a - s, b2 = b + s;
    const double up = len + 1e-9, down = len - 1e-9;
    return a2 > up || b2 < down;
}

// every gap row [r0, r1) of the problem holds under S.  rows = (column, group local to the problem, l) triples; group g owns the segments
// [grp_seg_off[grp0 + g], grp_seg_off[grp0 + g + 1]) of gsup / grp_len.  Every index read from memory is clamped: n_grp groups and
// n_grp_seg group segments in the batch (both >= 1 when there is a row), R columns in the problem.
EX_HD bool ex_rows_hold(unsigned S, ex_i64 r0, ex_i64 r1, const int *rows, int R, ex_i64 grp0, ex_i64 n_grp, const ex_i64 *grp_seg_off, ex_i64 n_grp_seg,
                        const unsigned *gsup, const int *grp_len, double lo_f, double hi_f, int offset, ex_i64 max_lg) {
    for (ex_i64 r = r0; r < r1; ++r) {
        const int c = (int)ex_clamp(rows[3 * r], 0, R - 1);
        const ex_i64 g = ex_clamp(grp0 + rows[3 * r + 1], 0, n_grp - 1);
        const ex_i64 s0 = ex_clamp(grp_seg_off[g], 0, n_grp_seg), s1 = ex_clamp(grp_seg_off[g + 1], s0, n_grp_seg);
        ex_i64 G = 0;
        for (ex_i64 s = s0; s < s1; ++s) G += (gsup[s] & S) ? grp_len[s] : 0;
        if (ex_row_violated(G, rows[3 * r + 2], lo_f, hi_f, offset, (S >> c) & 1u ? 0 : max_lg)) return false;
    }
    return true;
}

// cost2 of S: the g2 of the columns outside, twice the members' corrections on the segments in e
EX_HD ex_i64 ex_cost2(unsigned S, const unsigned *tab, int E, const int *g2, int R) {
    ex_i64 out = 0;
    for (int c = 0; c < R; ++c) out += (S >> c) & 1u ? 0 : g2[c];
    int corr = 0;
    for (int k = 0; k < E; ++k) corr += (tab[2 * k] & S) ? ex_popc(tab[2 * k + 1] & S) : 0;
    return out + 2ll * corr;
}

// one mask, whole: the conflict test first, then the rows, then the cost
EX_HD ex_u64 ex_mask_key(unsigned S, const unsigned *tab, int E, const unsigned *conf, const int *g2, int R, ex_i64 r0, ex_i64 r1, const int *rows,
                         ex_i64 grp0, ex_i64 n_grp, const ex_i64 *grp_seg_off, ex_i64 n_grp_seg, const unsigned *gsup, const int *grp_len, double lo_f,
                         double hi_f, int offset, ex_i64 max_lg) {
    if (ex_conflict(S, conf, R)) return kExactKeyNone;
    if (!ex_rows_hold(S, r0, r1, rows, R, grp0, n_grp, grp_seg_off, n_grp_seg, gsup, grp_len, lo_f, hi_f, offset, max_lg)) return kExactKeyNone;
    return ex_key(ex_cost2(S, tab, E, g2, R), S);
}

// the place of segment j among the ascending inf[0 .. n), or -1
EX_HD int ex_find_seg(const int *inf, int n, int j) {
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (inf[mid] < j) lo = mid + 1; else hi = mid; }
    return lo < n && inf[lo] == j ? lo : -1;
}

#endif
