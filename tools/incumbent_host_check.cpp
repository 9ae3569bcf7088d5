// incumbent_host_check.cpp -- the per-thread functions of the greedy round incumbents (freddie_amd/csrc/clu_incumbent.h, what
// k_inc_start / k_inc_pick of freddie_cluster.hip call) run on the host: a workgroup's 256 threads one after the other, in the kernels'
// order of steps, over problems read from standard input.  tools/incumbent_host_check.py feeds it problems and compares what it prints
// with the Python mirror (cluster_solve.greedy_incumbent).  Build:  g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined
// -I freddie_amd/csrc tools/incumbent_host_check.cpp -o incumbent_host_check     (every array is a std::vector: an index outside one stops it)
//
// Input, whitespace separated, one problem after the other until the end of the input:
//   R M max_seeds offset max_lg lo_f hi_f (the doubles as C99 hex floats) | I rows (R x W words, W = max(ceil(M / 32), 1)) | C rows | informative
//   row (W) | g2 (R) | n_pairs, pairs (2 each) | n_grp, grp_seg_off (n_grp + 1), grp_seg, grp_len | col_row_off (R + 1), rows (3 each)
// Output per problem and path (rows ANDed beforehand as the LDS path stages them; raw rows with the informative row beside them):
//   cost2 start grow_steps repair_steps n_members members...      (-1 -1 0 0 0 when no start is feasible)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "clu_incumbent.h"

namespace {

constexpr int kThreads = 256;

struct Problem {
    int R = 0, M = 0, W = 1, CW = 1, max_seeds = 1, offset = 0;
    inc_i64 max_lg = 0;
    double lo_f = 1.0, hi_f = 1.0;
    std::vector<unsigned> ibits, cbits, inf, conf;
    std::vector<int> g2, grp_seg, grp_len, rows;
    std::vector<inc_i64> grp_seg_off, col_row_off;
    inc_i64 n_grp = 0, n_grp_seg = 0, n_rows = 0;
};

bool read_int(long long &v) { return scanf("%lld", &v) == 1; }

long long need_int() {
    long long v;
    if (!read_int(v)) { fprintf(stderr, "input ends inside a problem\n"); exit(2); }
    return v;
}

double need_double() {
    char buf[64];
    if (scanf("%63s", buf) != 1) { fprintf(stderr, "input ends inside a problem\n"); exit(2); }
    return strtod(buf, nullptr);
}

bool read_problem(Problem &p) {
    long long v;
    if (!read_int(v)) return false;
    p = Problem();
    p.R = (int)v; p.M = (int)need_int(); p.max_seeds = (int)need_int(); p.offset = (int)need_int(); p.max_lg = need_int();
    p.lo_f = need_double(); p.hi_f = need_double();
    p.W = (p.M + 31) / 32 > 1 ? (p.M + 31) / 32 : 1;
    p.CW = (p.R + 31) / 32 > 1 ? (p.R + 31) / 32 : 1;
    const size_t RW = (size_t)p.R * p.W;
    p.ibits.resize(RW); p.cbits.resize(RW); p.inf.resize((size_t)p.W); p.g2.resize((size_t)p.R);
    for (auto &x : p.ibits) x = (unsigned)need_int();
    for (auto &x : p.cbits) x = (unsigned)need_int();
    for (auto &x : p.inf) x = (unsigned)need_int();
    for (auto &x : p.g2) x = (int)need_int();
    p.conf.assign((size_t)p.R * p.CW, 0u);
    const long long n_pairs = need_int();
    for (long long i = 0; i < n_pairs; ++i) {               // k_inc_conflict
        const int a = (int)need_int(), b = (int)need_int();
        if ((unsigned)a < (unsigned)p.R && (unsigned)b < (unsigned)p.R) {
            p.conf[(size_t)a * p.CW + (b >> 5)] |= 1u << (b & 31);
            p.conf[(size_t)b * p.CW + (a >> 5)] |= 1u << (a & 31);
        }
    }
    p.n_grp = need_int();
    p.grp_seg_off.resize((size_t)p.n_grp + 1);
    for (auto &x : p.grp_seg_off) x = need_int();
    p.n_grp_seg = p.grp_seg_off.back();
    p.grp_seg.resize((size_t)p.n_grp_seg); p.grp_len.resize((size_t)p.n_grp_seg);
    for (auto &x : p.grp_seg) x = (int)need_int();
    for (auto &x : p.grp_len) x = (int)need_int();
    p.col_row_off.resize((size_t)p.R + 1);
    for (auto &x : p.col_row_off) x = need_int();
    p.n_rows = p.col_row_off.back();
    p.rows.resize(3 * (size_t)p.n_rows);
    for (auto &x : p.rows) x = (int)need_int();
    return true;
}

struct StartResult { inc_i64 cost2; int grow, repair; std::vector<unsigned> members; };
constexpr inc_i64 kNoCost = 0x7fffffffffffffffll;

// k_inc_start for one (problem, start); staged: the LDS path's rows (ANDed with the informative row, no row beside them)
StartResult run_start(const Problem &p, int k, int n_seeds, bool staged) {
    const int R = p.R, W = p.W, CW = p.CW;
    std::vector<unsigned> ri(p.ibits), rc(p.cbits);
    if (staged)
        for (int c = 0; c < R; ++c)
            for (int w = 0; w < W; ++w) { ri[(size_t)c * W + w] &= p.inf[(size_t)w]; rc[(size_t)c * W + w] &= p.inf[(size_t)w]; }
    const unsigned *inf = staged ? nullptr : p.inf.data();
    std::vector<unsigned> E((size_t)W, 0u), mem((size_t)CW, 0u), blk((size_t)CW, 0u);
    std::vector<int> cnt((size_t)W * 32, 0);
    const auto row_i = [&](int c) { return ri.data() + (size_t)c * W; };
    const auto row_c = [&](int c) { return rc.data() + (size_t)c * W; };
    const auto add = [&](int c) {
        for (int tid = 0; tid < kThreads; ++tid) {
            for (int w = tid; w < W; w += kThreads) inc_add_word(row_i(c)[w] & p.inf[(size_t)w], row_c(c)[w] & p.inf[(size_t)w], w, E.data(), cnt.data());
            for (int w = tid; w < CW; w += kThreads) blk[(size_t)w] |= p.conf[(size_t)c * CW + w];
            if (tid == 0) mem[(size_t)(c >> 5)] |= 1u << (c & 31);
        }
    };
    const int seed = inc_start_col(k, n_seeds, R);
    if (seed >= 0 && seed < R) add(seed);
    StartResult out = {0, 0, 0, {}};
    for (int step = 0; step < R; ++step) {
        inc_u64 best = kIncKeyNone;
        for (int tid = 0; tid < kThreads; ++tid)
            for (int c = tid; c < R; c += kThreads) {
                if (inc_bit(mem.data(), c) || inc_bit(blk.data(), c)) continue;
                const inc_u64 kk = inc_grow_key(inc_delta2(row_i(c), row_c(c), inf, W, E.data(), cnt.data(), p.g2[(size_t)c]), c);
                best = kk < best ? kk : best;
            }
        if (best == kIncKeyNone || inc_key_delta2(best) >= 0) break;
        add(inc_clamp(inc_key_col(best), 0, R - 1));
        ++out.grow;
    }
    for (int step = 0; step < R; ++step) {
        inc_u64 best = kIncKeyNone;
        for (int tid = 0; tid < kThreads; ++tid)
            for (int c = tid; c < R; c += kThreads) {
                if (!inc_bit(mem.data(), c)) continue;
                inc_i64 r0 = p.col_row_off[(size_t)c], r1 = p.col_row_off[(size_t)c + 1];
                r0 = r0 < 0 ? 0 : r0 > p.n_rows ? p.n_rows : r0;
                r1 = r1 < r0 ? r0 : r1 > p.n_rows ? p.n_rows : r1;
                const int bad = inc_violations(r0, r1, p.rows.data(), 0, p.n_grp, p.grp_seg_off.data(), p.n_grp_seg, p.grp_seg.data(), p.grp_len.data(),
                                               p.M, E.data(), p.lo_f, p.hi_f, (inc_i64)p.offset);
                if (bad) { const inc_u64 kk = inc_repair_key(bad, c); best = kk < best ? kk : best; }
            }
        if (best == kIncKeyNone) break;
        const int gone = inc_clamp(inc_key_col(best), 0, R - 1);
        mem[(size_t)(gone >> 5)] &= ~(1u << (gone & 31));
        for (int w = 0; w < W; ++w) E[(size_t)w] = 0u;
        const int stripes = W >= kThreads ? 1 : kThreads / W;
        for (int tid = 0; tid < kThreads; ++tid)
            for (int x = tid; x < stripes * W; x += kThreads) {
                const int st = x / W, w = x - st * W;
                unsigned o = 0u;
                for (int c = st; c < R; c += stripes) if (inc_bit(mem.data(), c)) o |= row_i(c)[w] & p.inf[(size_t)w];
                E[(size_t)w] |= o;
            }
        ++out.repair;
    }
    int bad_out = 0;
    for (int c = 0; c < R; ++c) {
        const bool in = inc_bit(mem.data(), c);
        out.cost2 += inc_score_col(in, row_c(c), inf, W, E.data(), p.g2[(size_t)c]);
        if (!in) {
            inc_i64 r0 = p.col_row_off[(size_t)c], r1 = p.col_row_off[(size_t)c + 1];
            r0 = r0 < 0 ? 0 : r0 > p.n_rows ? p.n_rows : r0;
            r1 = r1 < r0 ? r0 : r1 > p.n_rows ? p.n_rows : r1;
            bad_out += inc_violations(r0, r1, p.rows.data(), 0, p.n_grp, p.grp_seg_off.data(), p.n_grp_seg, p.grp_seg.data(), p.grp_len.data(), p.M,
                                      E.data(), p.lo_f, p.hi_f, (inc_i64)p.offset + p.max_lg);
        }
    }
    if (bad_out) out.cost2 = kNoCost;
    out.members = mem;
    return out;
}

void run_problem(const Problem &p, bool staged) {
    const int n_seeds = p.R < p.max_seeds ? p.R : p.max_seeds;
    StartResult best = {0, 0, 0, {}};
    int at = -1;
    for (int k = 0; k <= n_seeds; ++k) {                     // k_inc_pick: the smallest cost2, then the earliest start
        StartResult r = run_start(p, k, n_seeds, staged);
        if (r.cost2 != kNoCost && (at < 0 || r.cost2 < best.cost2)) { best = r; at = k; }
    }
    if (at < 0) { printf("-1 -1 0 0 0\n"); return; }
    std::vector<int> members;
    for (int c = 0; c < p.R; ++c) if (inc_bit(best.members.data(), c)) members.push_back(c);
    printf("%lld %d %d %d %zu", best.cost2, at, best.grow, best.repair, members.size());
    for (int c : members) printf(" %d", c);
    printf("\n");
}

}  // namespace

int main() {
    Problem p;
    while (read_problem(p)) {
        run_problem(p, true);
        run_problem(p, false);
    }
    return 0;
}
