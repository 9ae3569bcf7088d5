// clu_incumbent.h -- what one thread of the greedy round incumbents (fclu_round_incumbents; k_inc_conflict / k_inc_start / k_inc_pick in
// freddie_cluster.hip) computes: a candidate's delta2, a member's violated gap rows, a column's share of the score, the packed keys and
// the starts.  Host and device: tools/incumbent_host_check.cpp runs the same functions over a workgroup's threads one after the other and
// is compared with the Python mirror (cluster_solve.greedy_incumbent) where there is no GPU.  The definition is the mirror's docstring.
//
// Rows: a column's I and C rows (W uint32 words, ANDed with the problem's informative row by whoever stages or reads them), E the OR of the
// members' I rows, cnt[j] the members with C = 1 at segment j.  Nothing here indexes with a value it has read without clamping it first.
#ifndef CLU_INCUMBENT_H
#define CLU_INCUMBENT_H

#include <stdint.h>

#if defined(__HIPCC__)
#define INC_HD __host__ __device__ __forceinline__
#else
#define INC_HD inline
#endif

typedef long long inc_i64;
typedef unsigned long long inc_u64;

INC_HD int inc_popc(unsigned x) { return __builtin_popcount(x); }
INC_HD int inc_ctz(unsigned x) { return __builtin_ctz(x); }
INC_HD int inc_clamp(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
INC_HD bool inc_bit(const unsigned *row, int c) { return (row[c >> 5] >> (c & 31)) & 1u; }

// start k of n seeded starts over R columns: column floor(k R / n); k == n (and every start of a problem without columns) is the empty set
INC_HD int inc_start_col(int k, int n, int R) { return k < n ? (int)((inc_i64)k * R / n) : -1; }

// the smallest key wins: the smaller delta2, then the smaller column
constexpr inc_u64 kIncKeyNone = ~0ull;
INC_HD inc_u64 inc_grow_key(int delta2, int c) { return ((inc_u64)((unsigned)delta2 ^ 0x80000000u) << 32) | (unsigned)c; }
INC_HD int inc_key_delta2(inc_u64 key) { return (int)((unsigned)(key >> 32) ^ 0x80000000u); }
INC_HD int inc_key_col(inc_u64 key) { return (int)(unsigned)(key & 0xffffffffull); }
// the smallest key wins: the larger count of violated rows, then the smaller column
INC_HD inc_u64 inc_repair_key(int violated, int c) { return ((inc_u64)(0xffffffffu - (unsigned)violated) << 32) | (unsigned)c; }

// delta2 of adding a column with the rows ri / rc (stride-1 words, W of them; `inf` ANDed on when the rows are the raw ones, else null)
INC_HD int inc_delta2(const unsigned *ri, const unsigned *rc, const unsigned *inf, int W, const unsigned *E, const int *cnt, int g2) {
    int corr = 0;
    for (int w = 0; w < W; ++w) {
        const unsigned m = inf ? inf[w] : 0xffffffffu, e = E[w];
        unsigned nw = ri[w] & m & ~e;
        corr += inc_popc(rc[w] & m & (e | nw));
        while (nw) { corr += cnt[w * 32 + inc_ctz(nw)]; nw &= nw - 1; }
    }
    return 2 * corr - g2;
}

// word w of a new member's rows: E takes its I bits, cnt its C bits (one thread a word: no two touch one counter)
INC_HD void inc_add_word(unsigned iw, unsigned cw, int w, unsigned *E, int *cnt) {
    E[w] |= iw;
    while (cw) { cnt[w * 32 + inc_ctz(cw)] += 1; cw &= cw - 1; }
}

// lo_f G - offset > l  or  hi_f G + offset < l, in doubles: one rounded multiply, one rounded add or subtract, never fused.  offset: the
// gap offset for a member's row; the gap offset + MAX_ISOFORM_LG (one exact integer) for the row of a column outside the set
INC_HD bool inc_row_violated(inc_i64 G, int l, double lo_f, double hi_f, inc_i64 offset) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double g = (double)G, o = (double)offset, len = (double)l;
    const double lo = lo_f * g;
    const double hi = hi_f * g;
    const double a = lo - o, b = hi + o;
    return a > len || b < len;
}

// the violated ones among the gap rows [r0, r1) of one column (offset as inc_row_violated's): rows = (column, group local to the problem, l) triples, group g owns the
// segments grp_seg / grp_len [grp_seg_off[grp0 + g], grp_seg_off[grp0 + g + 1]).  Every index read from memory is clamped: n_grp groups
// and n_grp_seg group segments in the batch (both >= 1 when there is a row), M segments in the problem.
INC_HD int inc_violations(inc_i64 r0, inc_i64 r1, const int *rows, inc_i64 grp0, inc_i64 n_grp, const inc_i64 *grp_seg_off, inc_i64 n_grp_seg,
                          const int *grp_seg, const int *grp_len, int M, const unsigned *E, double lo_f, double hi_f, inc_i64 offset) {
    int bad = 0;
    for (inc_i64 r = r0; r < r1; ++r) {
        inc_i64 g = grp0 + rows[3 * r + 1];
        g = g < 0 ? 0 : g > n_grp - 1 ? n_grp - 1 : g;
        inc_i64 s0 = grp_seg_off[g], s1 = grp_seg_off[g + 1];
        s0 = s0 < 0 ? 0 : s0 > n_grp_seg ? n_grp_seg : s0;
        s1 = s1 < s0 ? s0 : s1 > n_grp_seg ? n_grp_seg : s1;
        inc_i64 G = 0;
        for (inc_i64 s = s0; s < s1; ++s) {
            const int j = inc_clamp(grp_seg[s], 0, M - 1);
            if (inc_bit(E, j)) G += grp_len[s];
        }
        bad += inc_row_violated(G, rows[3 * r + 2], lo_f, hi_f, offset) ? 1 : 0;
    }
    return bad;
}

// a column's share of cost2: twice its corrections under E when it is a member, its g2 otherwise
INC_HD inc_i64 inc_score_col(bool member, const unsigned *rc, const unsigned *inf, int W, const unsigned *E, int g2) {
    if (!member) return g2;
    int corr = 0;
    for (int w = 0; w < W; ++w) corr += inc_popc(rc[w] & (inf ? inf[w] : 0xffffffffu) & E[w]);
    return 2ll * corr;
}

#endif
