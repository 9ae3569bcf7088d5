// clu_bnb.h -- what one lane of the branch and bound over a round's problems of up to 64 columns (fclu_round_bnb; k_bnb_prep / k_bnb_search
// in freddie_cluster.hip) computes: the bound of a node, the lower-side row test, the leaf test and one whole task.  Host and device:
// tools/bnb_host_check.cpp runs the same functions over every task of a problem and is compared with the Python mirror
// (cluster_solve.exact_bnb), whose docstring is the definition -- node counts included.
//
// The tables are clu_exact.h's with 64-bit words: S is a 64-bit mask, bit c = column c; informative segment k owns tab[2 k] = its support
// and tab[2 k + 1] = the columns with C = 1 there; conf[c] = the columns in conflict with c; a gap group's segments carry their support word
// (gsup) beside their length.  Nothing here indexes with a value it has read without clamping it first.
#ifndef CLU_BNB_H
#define CLU_BNB_H

#include "clu_exact.h"

constexpr int kBnbMaxCols = 64;
constexpr ex_i64 kBnbNone = 1ll << 62;         // "no bound": no cost2 reaches it (cost2 < 2^38 at 64 columns)

EX_HD int bnb_popc(ex_u64 x) { return __builtin_popcountll(x); }
EX_HD int bnb_ctz(ex_u64 x) { return __builtin_ctzll(x); }
EX_HD ex_u64 bnb_low(int d) { return d >= 64 ? ~0ull : (1ull << d) - 1ull; }      // columns 0 .. d - 1

// One problem as a lane sees it: tab, conf and g2 are its own (in LDS on the device), the rows and groups the batch's.
struct BnbView {
    const ex_u64 *tab, *conf; const int *g2;
    int E, R;
    ex_i64 r0, r1; const int *rows;                          // its gap rows [r0, r1): (column, group local to the problem, l)
    ex_i64 grp0, n_grp; const ex_i64 *grp_seg_off; ex_i64 n_grp_seg; const ex_u64 *gsup; const int *grp_len;
    double lo_f, hi_f; int offset; ex_i64 max_lg;
};

// an incompatible pair lies inside S
EX_HD bool bnb_conflict(const BnbView &v, ex_u64 S) {
    for (ex_u64 m = S; m; m &= m - 1) {
        const int c = (int)ex_clamp(bnb_ctz(m), 0, v.R - 1);
        if (v.conf[c] & S) return true;
    }
    return false;
}

// G of row r under S: the lengths of its group's segments whose support meets S
EX_HD ex_i64 bnb_row_G(const BnbView &v, ex_u64 S, ex_i64 r) {
    const ex_i64 g = ex_clamp(v.grp0 + v.rows[3 * r + 1], 0, v.n_grp - 1);
    const ex_i64 s0 = ex_clamp(v.grp_seg_off[g], 0, v.n_grp_seg), s1 = ex_clamp(v.grp_seg_off[g + 1], s0, v.n_grp_seg);
    ex_i64 G = 0;
    for (ex_i64 s = s0; s < s1; ++s) G += (v.gsup[s] & S) ? v.grp_len[s] : 0;
    return G;
}

// lo_f G - offset > l + 1e-9: the lower side of ex_row_violated for a member (slack 0), the same operations in the same order, none fused
EX_HD bool bnb_row_low(ex_i64 G, int l, double lo_f, int offset) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double g = (double)G, o = (double)offset, len = (double)l;
    const double lo = lo_f * g;
    const double a = lo - o;
    const double up = len + 1e-9;
    return a > up;
}

constexpr int kBnbPlanes = 14;                // a column's corrections on e_in are counted in 14 bits: below 2^14 = 16 384 informative segments

// LB2 of the node (columns 0 .. d - 1 fixed, S of them in; S has no bit at or above d).  One pass over the segments: a segment of e_in adds
// its members' corrections to the sum and its correction word, cut to the free columns (at or above d, in conflict with no member), to 64
// counters held as bit planes -- plane b is bit b of every column's count, and adding a word is a ripple of and / xor that ends where the
// carry is empty.  The planes live in registers (the loops over them unroll), so a node costs E steps, not E steps a column; four segments
// are read before the first is used, so that a lane waits for the table once in four steps.
EX_HD ex_i64 bnb_lb2(const BnbView &v, ex_u64 S, int d) {
    ex_i64 lb = 0;
    ex_u64 blocked = 0;
    for (ex_u64 m = bnb_low(d) & ~S; m; m &= m - 1) lb += v.g2[(int)ex_clamp(bnb_ctz(m), 0, v.R - 1)];
    for (ex_u64 m = S; m; m &= m - 1) blocked |= v.conf[(int)ex_clamp(bnb_ctz(m), 0, v.R - 1)];
    const ex_u64 rest = bnb_low(v.R) & ~bnb_low(d), free_cols = rest & ~blocked;
    ex_u64 plane[kBnbPlanes];
    for (int b = 0; b < kBnbPlanes; ++b) plane[b] = 0ull;
    int corr = 0;
    for (int k0 = 0; k0 < v.E; k0 += 4) {
        ex_u64 sw[4], cw[4];
        for (int i = 0; i < 4; ++i) {                        // (behind the last segment: the last one again, with an empty support)
            const int k = k0 + i < v.E ? k0 + i : v.E - 1;
            sw[i] = k0 + i < v.E ? v.tab[2 * k] : 0ull;
            cw[i] = v.tab[2 * k + 1];
        }
        for (int i = 0; i < 4; ++i) {
            const ex_u64 w = (sw[i] & S) ? cw[i] : 0ull;
            corr += bnb_popc(w & S);
            ex_u64 carry = w & free_cols;
            for (int b = 0; b < kBnbPlanes; ++b) {
                if (!carry) break;
                const ex_u64 both = plane[b] & carry;
                plane[b] ^= carry;
                carry = both;
            }
        }
    }
    lb += 2ll * corr;
    int used = 0;                                            // planes with a bit: the counts are below 2^used
    for (int b = 0; b < kBnbPlanes; ++b) used = plane[b] ? b + 1 : used;
    for (ex_u64 m = rest & blocked; m; m &= m - 1) lb += v.g2[(int)ex_clamp(bnb_ctz(m), 0, v.R - 1)];
    for (ex_u64 m = free_cols; m; m &= m - 1) {              // min(g2_c, 2 |C_c & e_in|)
        const int c = (int)ex_clamp(bnb_ctz(m), 0, v.R - 1);
        int cnt = 0;
        for (int b = 0; b < kBnbPlanes; ++b) {
            if (b >= used) break;
            cnt |= (int)(plane[b] >> c & 1ull) << b;
        }
        const int g = v.g2[c], in2 = 2 * cnt;
        lb += in2 < g ? in2 : g;
    }
    return lb;
}

// the node is dropped: its bound exceeds best2, or a member's row is violated from below already.  rows: false for an exclude child, whose
// S is its parent's, which passed the rows' test
EX_HD bool bnb_pruned(const BnbView &v, ex_u64 S, int d, ex_i64 best2, bool rows) {
    if (bnb_lb2(v, S, d) > best2) return true;
    for (ex_i64 r = v.r0; rows && r < v.r1; ++r) {
        const int c = (int)ex_clamp(v.rows[3 * r], 0, v.R - 1);
        if ((S >> c & 1ull) && bnb_row_low(bnb_row_G(v, S, r), v.rows[3 * r + 2], v.lo_f, v.offset)) return true;
    }
    return false;
}

// a leaf: S over all R columns is feasible (the 64-bit ex_conflict and ex_rows_hold) and *cost2 is its cost (the 64-bit ex_cost2)
EX_HD bool bnb_leaf(const BnbView &v, ex_u64 S, ex_i64 *cost2) {
    if (bnb_conflict(v, S)) return false;
    for (ex_i64 r = v.r0; r < v.r1; ++r) {
        const int c = (int)ex_clamp(v.rows[3 * r], 0, v.R - 1);
        if (ex_row_violated(bnb_row_G(v, S, r), v.rows[3 * r + 2], v.lo_f, v.hi_f, v.offset, (S >> c & 1ull) ? 0 : v.max_lg)) return false;
    }
    ex_i64 out = 0;
    for (ex_u64 m = bnb_low(v.R) & ~S; m; m &= m - 1) out += v.g2[(int)ex_clamp(bnb_ctz(m), 0, v.R - 1)];
    int corr = 0;
    for (int k = 0; k < v.E; ++k) corr += (v.tab[2 * k] & S) ? bnb_popc(v.tab[2 * k + 1] & S) : 0;
    *cost2 = out + 2ll * corr;
    return true;
}

struct BnbResult { ex_i64 cost2; ex_u64 mask; int nodes, capped; };      // cost2 -1 and mask 0: the task found no leaf

// Task t of the problem's 2^D (D = min(R, depth), 0 <= t < 2^D), ub2 < 0 = no bound, node_cap >= 1.  The stack: frame d is S's low d bits
// and bit d of tried_in / tried_out, so its at most 64 frames are three words; the loop runs at most 3 * node_cap + 64 times.
EX_HD BnbResult bnb_task(const BnbView &v, ex_u64 t, int D, ex_i64 ub2, int node_cap) {
    const int R = v.R;
    BnbResult res = {-1, 0ull, 1, 0};
    ex_i64 best2 = ub2 < 0 ? kBnbNone : ub2;
    bool have = false;
    ex_u64 S = t & bnb_low(D);
    if (bnb_conflict(v, S)) return res;
    if (D >= R) {
        ex_i64 cost2;
        if (bnb_leaf(v, S, &cost2) && cost2 <= best2) { res.cost2 = cost2; res.mask = S; }
        return res;
    }
    if (bnb_pruned(v, S, D, best2, true)) return res;
    int d = D;
    ex_u64 tried_in = 0, tried_out = 0;
    for (;;) {
        const ex_u64 bit = 1ull << d, Sd = S & (bit - 1ull);
        if (tried_out & bit) {                               // both children done: pop
            if (d == D) break;
            --d;
            continue;
        }
        ex_u64 child;
        if (!(tried_in & bit)) {
            tried_in |= bit;
            if (v.conf[d] & Sd) continue;
            child = Sd | bit;
        } else {
            tried_out |= bit;
            child = Sd;
        }
        if (res.nodes >= node_cap) { res.capped = 1; break; }
        ++res.nodes;
        if (d + 1 == R) {
            ex_i64 cost2;
            if (bnb_leaf(v, child, &cost2) && (cost2 < best2 || (cost2 == best2 && (!have || child < res.mask)))) {
                best2 = cost2; res.mask = child; have = true;
            }
        } else if (!bnb_pruned(v, child, d + 1, best2, child != Sd)) {
            S = child; ++d;
            tried_in &= ~(1ull << d); tried_out &= ~(1ull << d);
        }
    }
    if (have) res.cost2 = best2;
    return res;
}

// the smaller (cost2, mask) of two task results, -1 = none
EX_HD bool bnb_better(ex_i64 cost2, ex_u64 mask, ex_i64 than2, ex_u64 than_mask) {
    return cost2 >= 0 && (than2 < 0 || cost2 < than2 || (cost2 == than2 && mask < than_mask));
}

#endif
