// bnb_wide_host_check.cpp -- the per-lane functions and the task walk of the branch and bound over a round's problems of up to 1024
// columns (freddie_amd/csrc/clu_bnb_wide.h, what k_bw_prep / k_bw_search of freddie_cluster.hip call) run on the host: the by-column
// tables built as the prep kernel builds them, then every task of the problem, the lanes of a wave one after another (BwHostWave).
// tools/bnb_wide_host_check.py feeds it problems and compares what it prints, task by task, with the Python mirror (cluster_solve.bnb_task
// on exact_bnb_wide's tables).
// Build:  g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I freddie_amd/csrc tools/bnb_wide_host_check.cpp -o bnb_wide_host_check
// (every array is a std::vector of its exact size; the sanitizers stop a read outside one)
//
// Input: that of tools/bnb_host_check.cpp, R up to 1024.
// Output per task:  cost2 nodes capped mask     (the mask as one hexadecimal number; -1 and 0 when the task found no leaf)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "clu_bnb_wide.h"

namespace {

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

template <typename T>
void need_ints(std::vector<T> &v, size_t n) {
    v.resize(n);
    for (auto &x : v) x = (T)need_int();
}

struct Problem {
    int R = 0, depth = 0, node_cap = 1, offset = 0;
    ex_i64 ub2 = -1, max_lg = 0, n_inf = 0, n_grp = 0, n_grp_seg = 0, n_rows = 0;
    double lo_f = 1.0, hi_f = 1.0;
    std::vector<int> inf_seg, sup_cols, corr_seg, g2, pairs, grp_seg, grp_len, rows;
    std::vector<ex_i64> sup_off, corr_off, grp_seg_off;
};

bool read_problem(Problem &p) {
    long long v;
    if (!read_int(v)) return false;
    p = Problem();
    p.R = (int)v; p.depth = (int)need_int(); p.node_cap = (int)need_int(); p.ub2 = need_int(); p.offset = (int)need_int(); p.max_lg = need_int();
    p.lo_f = need_double(); p.hi_f = need_double();
    if (p.R < 0 || p.R > kBwMaxCols || p.depth < 0 || p.depth > 20 || p.node_cap < 1) { fprintf(stderr, "bad problem header\n"); exit(2); }
    p.n_inf = need_int();
    need_ints(p.inf_seg, (size_t)p.n_inf);
    need_ints(p.sup_off, (size_t)p.n_inf + 1);
    need_ints(p.sup_cols, (size_t)p.sup_off.back());
    need_ints(p.corr_off, (size_t)p.R + 1);
    need_ints(p.corr_seg, (size_t)p.corr_off.back());
    need_ints(p.g2, (size_t)p.R);
    need_ints(p.pairs, 2 * (size_t)need_int());
    p.n_grp = need_int();
    need_ints(p.grp_seg_off, (size_t)p.n_grp + 1);
    p.n_grp_seg = p.grp_seg_off.back();
    need_ints(p.grp_seg, (size_t)p.n_grp_seg);
    need_ints(p.grp_len, (size_t)p.n_grp_seg);
    p.n_rows = need_int();
    need_ints(p.rows, 3 * (size_t)p.n_rows);
    return true;
}

void run_problem(const Problem &p) {
    const int R = p.R, E = (int)p.n_inf, W = bw_words(R), EW = bw_ewords(E);
    if (bw_lds_bytes(R, E) > kBwLdsBytes) { fprintf(stderr, "the tables of %d columns and %d segments do not fit\n", R, E); exit(2); }
    // ---- k_bw_prep
    std::vector<ex_u64> icol((size_t)R * EW, 0ull), ccol((size_t)R * EW, 0ull), conf((size_t)R * W, 0ull);
    std::vector<int> gk((size_t)p.n_grp_seg, -1);
    const ex_i64 n_sup = (ex_i64)p.sup_cols.size();
    for (int k = 0; k < E; ++k) {
        const ex_i64 a = ex_clamp(p.sup_off.at((size_t)k), 0, n_sup), b = ex_clamp(p.sup_off.at((size_t)k + 1), a, n_sup);
        for (ex_i64 s = a; s < b; ++s) {
            const int c = p.sup_cols.at((size_t)s);
            if ((unsigned)c < (unsigned)R) icol.at((size_t)c * EW + (k >> 6)) |= 1ull << (k & 63);
        }
    }
    for (int c = 0; c < R; ++c)
        for (ex_i64 x = p.corr_off.at((size_t)c); x < p.corr_off.at((size_t)c + 1); ++x) {
            const int k = ex_find_seg(p.inf_seg.data(), E, p.corr_seg.at((size_t)x));
            if (k >= 0) ccol.at((size_t)(k >> 6) * R + c) |= 1ull << (k & 63);
        }
    for (size_t i = 0; i + 1 < p.pairs.size(); i += 2) {
        const int a = p.pairs[i], b = p.pairs[i + 1];
        if ((unsigned)a < (unsigned)R && (unsigned)b < (unsigned)R) {
            conf.at((size_t)a * W + (b >> 6)) |= 1ull << (b & 63);
            conf.at((size_t)b * W + (a >> 6)) |= 1ull << (a & 63);
        }
    }
    for (ex_i64 s = 0; s < p.n_grp_seg; ++s) gk.at((size_t)s) = ex_find_seg(p.inf_seg.data(), E, p.grp_seg.at((size_t)s));
    // ---- k_bw_search, task by task
    std::vector<ex_u64> st((size_t)bw_state_words(W, EW), ~0ull);
    BwView v;
    v.icol = icol.data(); v.ccol = ccol.data(); v.conf = conf.data(); v.g2 = p.g2.data(); v.E = E; v.R = R; v.W = W; v.EW = EW;
    v.r0 = 0; v.r1 = p.n_grp > 0 ? p.n_rows : 0; v.rows = p.rows.data();
    v.grp0 = 0; v.n_grp = p.n_grp; v.grp_seg_off = p.grp_seg_off.data(); v.n_grp_seg = p.n_grp_seg; v.gk = gk.data(); v.grp_len = p.grp_len.data();
    v.lo_f = p.lo_f; v.hi_f = p.hi_f; v.offset = p.offset; v.max_lg = p.max_lg;
    v.st = st.data();
    BwHostWave wv;
    const int D = R < p.depth ? R : p.depth;
    for (ex_u64 t = 0; t < (1ull << D); ++t) {
        const BwResult r = bw_task(v, wv, t, D, p.ub2, p.node_cap);
        printf("%lld %d %d ", r.cost2, r.nodes, r.capped);
        for (int w = W - 1; w >= 0; --w) printf("%016llx", st[4 * (size_t)W + w]);
        printf("\n");
    }
}

}  // namespace

int main() {
    Problem p;
    while (read_problem(p)) run_problem(p);
    return 0;
}
