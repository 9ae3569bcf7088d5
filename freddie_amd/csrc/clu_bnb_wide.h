// clu_bnb_wide.h -- the branch and bound over a round's problems of up to 1024 columns (fclu_round_bnb_wide; k_bw_prep / k_bw_search /
// k_bw_reduce in freddie_cluster.hip): what a lane computes on column sets of W = ceil(R / 64) words, and the walk of one task, which a
// whole wave runs together.  Host and device: tools/bnb_wide_host_check.cpp runs the same functions, the lanes of a wave one after
// another, and is compared with the Python mirror (cluster_solve.exact_bnb_wide), whose docstring -- exact_bnb()'s -- is the definition,
// node counts included.
//
// The tables are by column: icol[c * EW + w] = word w of the informative segments column c supports (bit k = segment k, EW =
// ceil(E / 64) words; a lane per word reads neighbouring words), ccol[w * R + c] = word w of the segments with C = 1 at column c (a lane
// per column reads neighbouring words), conf[c * W + w] = word w of the columns in conflict with c.  A gap group's segments carry their
// place among the informative segments (gk, -1 = none) beside their length.  e_in and the blocked columns are functions of the set S
// alone: they are kept for the last set evaluated and for the one before (the parent an exclude child comes back to), and grow by one
// column's rows for an include child.  Nothing in this header indexes with a value it has read from the round's arrays (rows, groups, places)
// without clamping it first; the view's own pointers and sizes are the caller's.
#ifndef CLU_BNB_WIDE_H
#define CLU_BNB_WIDE_H

#include "clu_bnb.h"

constexpr int kBwMaxCols = 1024;
constexpr int kBwMaxWords = kBwMaxCols / 64;   // a result's set: 16 words, low word first
constexpr int kBwLanes = 64;                   // a wave: one task
constexpr int kBwWaves = 8;                    // waves, and so tasks, of a workgroup
constexpr int kBwLdsBytes = 160 * 1024;        // a workgroup's LDS on this part

EX_HD int bw_words(int n) { return n <= 64 ? 1 : (n + 63) >> 6; }                      // (at least one, so that word 0 exists)
EX_HD int bw_ewords(int E) { return (E + 63) >> 6; }
EX_HD int bw_bit(const ex_u64 *a, int c) { return (int)(a[c >> 6] >> (c & 63) & 1ull); }

// words of a wave's own state: S, child, tried_in, tried_out, best | kept set, set before, blocked, blocked before | e_in, e_in before
EX_HD int bw_state_words(int W, int EW) { return 9 * W + 2 * EW; }
// words of a problem's tables in LDS: icol and ccol
EX_HD ex_i64 bw_table_words(int R, int E) { return 2ll * R * bw_ewords(E); }
// The LDS a problem of R columns and E informative segments needs: its two tables, g2 and every wave's state.  A problem is taken when this
// is at most kBwLdsBytes (the Python mirror of the rule: cluster_prep.bnb_wide_lds_bytes).
EX_HD ex_i64 bw_lds_bytes(int R, int E) {
    const ex_i64 b = 8 * bw_table_words(R, E) + 4ll * R + 8ll * kBwWaves * bw_state_words(bw_words(R), bw_ewords(E));
    return (b + 15) & ~15ll;
}

struct BwView {
    const ex_u64 *icol, *ccol, *conf; const int *g2;
    int E, R, W, EW;
    ex_i64 r0, r1; const int *rows;                          // its gap rows [r0, r1): (column, group local to the problem, l)
    ex_i64 grp0, n_grp; const ex_i64 *grp_seg_off; ex_i64 n_grp_seg; const int *gk; const int *grp_len;
    double lo_f, hi_f; int offset; ex_i64 max_lg;
    ex_u64 *st;                                              // the wave's state, bw_state_words(W, EW) words
};

// word w of the conflict test: a blocked column lies inside S
EX_HD bool bw_conflict_word(const ex_u64 *blk, const ex_u64 *S, int w) { return (blk[w] & S[w]) != 0ull; }

// G of row r under e_in: the lengths of its group's segments that are informative and in e_in (their support meets S)
EX_HD ex_i64 bw_row_G(const BwView &v, const ex_u64 *e, ex_i64 r) {
    const ex_i64 g = ex_clamp(v.grp0 + v.rows[3 * r + 1], 0, v.n_grp - 1);
    const ex_i64 s0 = ex_clamp(v.grp_seg_off[g], 0, v.n_grp_seg), s1 = ex_clamp(v.grp_seg_off[g + 1], s0, v.n_grp_seg);
    ex_i64 G = 0;
    for (ex_i64 s = s0; s < s1; ++s) {
        const int k = v.gk[s];
        if (k >= 0 && k < v.E && bw_bit(e, k)) G += v.grp_len[s];
    }
    return G;
}

// a member's row r is violated from below (bnb_row_low), false for the row of a column outside S
EX_HD bool bw_row_low(const BwView &v, const ex_u64 *S, const ex_u64 *e, ex_i64 r) {
    const int c = (int)ex_clamp(v.rows[3 * r], 0, v.R - 1);
    return bw_bit(S, c) && bnb_row_low(bw_row_G(v, e, r), v.rows[3 * r + 2], v.lo_f, v.offset);
}

// the leaf's test of row r (ex_row_violated): slack 0 for a member, max_lg for a column outside
EX_HD bool bw_row_leaf(const BwView &v, const ex_u64 *S, const ex_u64 *e, ex_i64 r) {
    const int c = (int)ex_clamp(v.rows[3 * r], 0, v.R - 1);
    return ex_row_violated(bw_row_G(v, e, r), v.rows[3 * r + 2], v.lo_f, v.hi_f, v.offset, bw_bit(S, c) ? 0 : v.max_lg);
}

// column c's piece of LB2 at a node of depth d (S has no bit at or above d): fixed out g2_c, fixed in 2 |C_c & e_in|; free: g2_c when
// blocked, else min(g2_c, 2 |C_c & e_in|).  At d = R the pieces sum to the leaf's cost2.
EX_HD ex_i64 bw_col_term(const BwView &v, const ex_u64 *S, const ex_u64 *blk, const ex_u64 *e, int c, int d) {
    const ex_i64 g = v.g2[c];
    if (c < d ? !bw_bit(S, c) : bw_bit(blk, c)) return g;
    int cnt = 0;
    for (int w = 0; w < v.EW; ++w) cnt += bnb_popc(v.ccol[(ex_i64)w * v.R + c] & e[w]);
    const ex_i64 in2 = 2ll * cnt;
    return c < d ? in2 : in2 < g ? in2 : g;
}

// mask a is the smaller integer: most significant word first
EX_HD bool bw_less(const ex_u64 *a, const ex_u64 *b, int W) {
    for (int w = W - 1; w >= 0; --w)
        if (a[w] != b[w]) return a[w] < b[w];
    return false;
}

// the smaller (cost2, mask) of two results, -1 = none
EX_HD bool bw_better(ex_i64 cost2, const ex_u64 *mask, ex_i64 than2, const ex_u64 *than_mask, int W) {
    return cost2 >= 0 && (than2 < 0 || cost2 < than2 || (cost2 == than2 && bw_less(mask, than_mask, W)));
}

// The lanes of a wave on the host, one after another (the device's wave is BwDevWave in freddie_cluster.hip): f(lane) is a lane's share.
struct BwHostWave {
    template <class F> ex_i64 sum(F f) { ex_i64 s = 0; for (int l = 0; l < kBwLanes; ++l) s += f(l); return s; }
    template <class F> bool any(F f) { bool a = false; for (int l = 0; l < kBwLanes; ++l) a = f(l) || a; return a; }
    template <class F> void each(F f) { for (int l = 0; l < kBwLanes; ++l) f(l); }
    void sync() {}
};

// e_in and blocked of the set S, in the wave's state: kept when S is the kept set, taken back when it is the set before, grown by the
// new columns' rows when the kept set lies inside S (the kept set becomes the set before), else built from nothing.  The set words are
// the same in every lane, which reads what it wrote itself; e_in and blocked are written a word a lane, so a sync stands on either side.
template <class Wave>
EX_HD void bw_cache(const BwView &v, Wave &wv, const ex_u64 *S) {
    const int W = v.W, EW = v.EW;
    ex_u64 *Sc = v.st + 5 * W, *Sb = Sc + W, *blk = Sb + W, *blkb = blk + W, *e = blkb + W, *eb = e + EW;
    bool same = true, back = true, sub = true;
    for (int w = 0; w < W; ++w) { same = same && Sc[w] == S[w]; back = back && Sb[w] == S[w]; sub = sub && !(Sc[w] & ~S[w]); }
    if (same) return;
    wv.sync();
    if (back) {
        wv.each([&](int lane) {
            for (int x = lane; x < EW; x += kBwLanes) e[x] = eb[x];
            for (int x = lane; x < W; x += kBwLanes) blk[x] = blkb[x];
        });
        for (int w = 0; w < W; ++w) Sc[w] = S[w];
        wv.sync();
        return;
    }
    wv.each([&](int lane) {
        for (int x = lane; x < EW; x += kBwLanes) { if (sub) eb[x] = e[x]; else e[x] = 0ull; }
        for (int x = lane; x < W; x += kBwLanes) { if (sub) blkb[x] = blk[x]; else blk[x] = 0ull; }
    });
    for (int w = 0; w < W; ++w) { if (sub) Sb[w] = Sc[w]; else Sc[w] = 0ull; }
    wv.sync();
    for (int w = 0; w < W; ++w)
        for (ex_u64 m = S[w] & ~Sc[w]; m; m &= m - 1) {
            const ex_i64 c = ex_clamp(64 * w + bnb_ctz(m), 0, v.R - 1);
            wv.each([&](int lane) {
                for (int x = lane; x < EW; x += kBwLanes) e[x] |= v.icol[c * EW + x];
                for (int x = lane; x < W; x += kBwLanes) blk[x] |= v.conf[c * W + x];
            });
        }
    for (int w = 0; w < W; ++w) Sc[w] = S[w];
    wv.sync();
}

// the node is dropped: its bound exceeds best2, or a member's row is violated from below already.  rows: false for an exclude child
template <class Wave>
EX_HD bool bw_pruned(const BwView &v, Wave &wv, const ex_u64 *S, int d, ex_i64 best2, bool rows) {
    bw_cache(v, wv, S);
    const ex_u64 *blk = v.st + 7 * v.W, *e = v.st + 9 * v.W;
    const ex_i64 lb = wv.sum([&](int lane) {
        ex_i64 part = 0;
        for (int c = lane; c < v.R; c += kBwLanes) part += bw_col_term(v, S, blk, e, c, d);
        return part;
    });
    if (lb > best2) return true;
    if (!rows) return false;
    return wv.any([&](int lane) {
        for (ex_i64 r = v.r0 + lane; r < v.r1; r += kBwLanes)
            if (bw_row_low(v, S, e, r)) return true;
        return false;
    });
}

// a leaf: S over all R columns is feasible and *cost2 is its cost
template <class Wave>
EX_HD bool bw_leaf(const BwView &v, Wave &wv, const ex_u64 *S, ex_i64 *cost2) {
    bw_cache(v, wv, S);
    const ex_u64 *blk = v.st + 7 * v.W, *e = v.st + 9 * v.W;
    const bool bad = wv.any([&](int lane) {
        for (int w = lane; w < v.W; w += kBwLanes)
            if (bw_conflict_word(blk, S, w)) return true;
        for (ex_i64 r = v.r0 + lane; r < v.r1; r += kBwLanes)
            if (bw_row_leaf(v, S, e, r)) return true;
        return false;
    });
    if (bad) return false;
    *cost2 = wv.sum([&](int lane) {
        ex_i64 part = 0;
        for (int c = lane; c < v.R; c += kBwLanes) part += bw_col_term(v, S, blk, e, c, v.R);
        return part;
    });
    return true;
}

struct BwResult { ex_i64 cost2; int nodes, capped, d; };     // cost2 -1: the task found no leaf; its set is the state's fifth array (zero without one); d: the level a capped task stopped at

// The task on the prefix (prefix, L) -- the columns 0 .. L - 1 are fixed, the prefix's low L bits say which are in; n_prefix of its W
// words are given, the others are empty; L is clamped to [0, R] -- ub2 < 0 = no bound, node_cap >= 1: bnb_prefix_task()'s walk, step for
// step, on sets of W words.  The stack: frame d is S's low d bits and bit d of tried_in / tried_out.  A capped task takes the progress
// bit of the child it did not evaluate back and leaves its frame in the state: S, tried_in and tried_out (the first, third and fourth
// array) and res.d.
template <class Wave>
EX_HD BwResult bw_task_from(const BwView &v, Wave &wv, const ex_u64 *prefix, int n_prefix, int L, ex_i64 ub2, int node_cap) {
    const int R = v.R, W = v.W, n_st = bw_state_words(W, v.EW);
    ex_u64 *S = v.st, *child = S + W, *tin = child + W, *tout = tin + W, *best = tout + W;
    wv.sync();
    wv.each([&](int lane) { for (int x = lane; x < n_st; x += kBwLanes) v.st[x] = 0ull; });
    wv.sync();
    L = (int)ex_clamp(L, 0, R);
    BwResult res = {-1, 1, 0, L};
    ex_i64 best2 = ub2 < 0 ? kBnbNone : ub2, cost2 = 0;
    bool have = false;
    for (int w = 0; w < W && w < n_prefix; ++w) S[w] = 64 * w + 64 <= L ? prefix[w] : 64 * w < L ? prefix[w] & bnb_low(L - 64 * w) : 0ull;
    bw_cache(v, wv, S);
    const ex_u64 *blk = v.st + 7 * W;
    if (wv.any([&](int lane) {
            for (int w = lane; w < W; w += kBwLanes)
                if (bw_conflict_word(blk, S, w)) return true;
            return false;
        }))
        return res;
    if (L >= R) {
        if (bw_leaf(v, wv, S, &cost2) && cost2 <= best2) {
            res.cost2 = cost2;
            for (int w = 0; w < W; ++w) best[w] = S[w];
        }
        return res;
    }
    if (bw_pruned(v, wv, S, L, best2, true)) return res;
    int d = L;
    for (;;) {
        const int wd = d >> 6;
        const ex_u64 bit = 1ull << (d & 63);
        if (tout[wd] & bit) {                                // both children done: pop
            if (d == L) break;
            --d;
            continue;
        }
        for (int w = 0; w < W; ++w) child[w] = w < wd ? S[w] : w == wd ? S[w] & (bit - 1ull) : 0ull;
        bool in;
        if (!(tin[wd] & bit)) {
            tin[wd] |= bit;
            const ex_u64 *row = v.conf + ex_clamp(d, 0, R - 1) * W;
            if (wv.any([&](int lane) {
                    for (int w = lane; w < W; w += kBwLanes)
                        if (row[w] & child[w]) return true;
                    return false;
                }))
                continue;
            child[wd] |= bit;
            in = true;
        } else {
            tout[wd] |= bit;
            in = false;
        }
        if (res.nodes >= node_cap) {                         // the child is not evaluated: its progress bit is taken back
            if (in) tin[wd] &= ~bit; else tout[wd] &= ~bit;
            res.capped = 1; res.d = d;
            break;
        }
        ++res.nodes;
        if (d + 1 == R) {
            if (bw_leaf(v, wv, child, &cost2) && (cost2 < best2 || (cost2 == best2 && (!have || bw_less(child, best, W))))) {
                best2 = cost2; have = true;
                for (int w = 0; w < W; ++w) best[w] = child[w];
            }
        } else if (!bw_pruned(v, wv, child, d + 1, best2, in)) {
            for (int w = 0; w < W; ++w) S[w] = child[w];
            ++d;
            tin[d >> 6] &= ~(1ull << (d & 63)); tout[d >> 6] &= ~(1ull << (d & 63));
        }
    }
    if (have) res.cost2 = best2;
    return res;
}

// Task t of the problem's 2^D (D = min(R, depth) <= 20, 0 <= t < 2^D): the task on the prefix (t, D).
template <class Wave>
EX_HD BwResult bw_task(const BwView &v, Wave &wv, ex_u64 t, int D, ex_i64 ub2, int node_cap) {
    const ex_u64 prefix = t & bnb_low(D);
    return bw_task_from(v, wv, &prefix, 1, D, ub2, node_cap);
}

// ---- the open children of a capped task (cluster_solve.bnb_open_children) ---------------------------------------------------------
// A capped task's frame: S, tried_in and tried_out of W words each (after the roll-back), the prefix length L and the level d it stopped
// at, 0 <= L <= d < R.  A record is a prefix of the next pass: its length, then its W words.
EX_HD int bw_record_words(int W) { return 1 + W; }
EX_HD int bw_frame_words(int W) { return 3 * W + 1; }        // S, tried_in, tried_out, then L | d << 32

// bits lo .. hi - 1 of word w
EX_HD ex_u64 bw_range_word(int w, int lo, int hi) {
    const int a = lo - 64 * w, b = hi - 64 * w;
    if (b <= 0 || a >= 64) return 0ull;
    return (b >= 64 ? ~0ull : bnb_low(b)) & ~(a <= 0 ? 0ull : bnb_low(a));
}

// the include child at level d is open: tried_in bit d is clear and no column of S's low d bits conflicts with column d
template <class Wave>
EX_HD bool bw_open_include(Wave &wv, const ex_u64 *conf_row, const ex_u64 *S, const ex_u64 *tin, int d, int W) {
    if (bw_bit(tin, d)) return false;
    return !wv.any([&](int lane) {
        for (int w = lane; w < W; w += kBwLanes)
            if (conf_row[w] & S[w] & bw_range_word(w, 0, d)) return true;
        return false;
    });
}

// The number of open children: the levels L .. d - 1 whose tried_out bit is clear, the exclude child at d (its tried_out bit is clear in
// every capped frame) and the include child at d when it is open.
EX_HD int bw_open_count(const ex_u64 *tout, int L, int d, int W, bool include_open) {
    int n = include_open && !bw_bit(tout, d) ? 1 : 0;
    for (int w = 0; w < W; ++w) n += bnb_popc(~tout[w] & bw_range_word(w, L, d + 1));
    return n;
}

// Writes the open children as records of 1 + W words at rec, by ascending level, at level d the include child first; max_records bounds
// what is written.  A lane writes every 64th word of a record.  Returns the records written.
template <class Wave>
EX_HD int bw_open_emit(Wave &wv, const ex_u64 *S, const ex_u64 *tout, int L, int d, int W, bool include_open, ex_u64 *rec, ex_i64 max_records) {
    const int rw = bw_record_words(W);
    int n = 0;
    for (int w = 0; w < W; ++w)
        for (ex_u64 m = ~tout[w] & bw_range_word(w, L, d + 1); m; m &= m - 1) {
            const int j = 64 * w + bnb_ctz(m);
            for (int inc = (j == d && include_open) ? 1 : 0; inc >= 0; --inc) {
                if (n >= max_records) return n;
                ex_u64 *out = rec + (ex_i64)n * rw;
                wv.each([&](int lane) {
                    if (lane == 0) out[0] = (ex_u64)(j + 1);
                    for (int x = lane; x < W; x += kBwLanes)
                        out[1 + x] = (S[x] & bw_range_word(x, 0, j)) | (inc && x == (j >> 6) ? 1ull << (j & 63) : 0ull);
                });
                ++n;
            }
        }
    return n;
}

#endif
