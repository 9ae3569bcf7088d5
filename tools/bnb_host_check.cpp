// bnb_host_check.cpp -- the per-lane functions of the branch and bound over a round's larger problems (freddie_amd/csrc/clu_bnb.h, what
// k_bnb_prep / k_bnb_search of freddie_cluster.hip call) run on the host: the 64-bit transposed table built as the prep kernel builds it,
// then every task of the problem, one after the other.  tools/bnb_host_check.py feeds it problems and compares what it prints, task by
// task, with the Python mirror (cluster_solve.bnb_task).
// Build:  g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I freddie_amd/csrc tools/bnb_host_check.cpp -o bnb_host_check
// (every array is a std::vector with a spare element behind it; the sanitizers stop a read outside one)
//
// Input, whitespace separated, one problem after the other until the end of the input:
//   R depth node_cap ub2 offset max_lg lo_f hi_f (the doubles as C99 hex floats; ub2 < 0: none) | n_inf, inf_seg | sup_off (n_inf + 1), sup_cols |
//   corr_off (R + 1), corr_seg | g2 (R) | n_pairs, pairs (2 each) | n_grp, grp_seg_off (n_grp + 1), grp_seg, grp_len | n_rows, rows (3 each)
// Output per task:  cost2 mask nodes capped     (-1 0 when the task found no leaf)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "clu_bnb.h"

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
    if (p.R < 0 || p.R > kBnbMaxCols || p.depth < 0 || p.depth > 20 || p.node_cap < 1) { fprintf(stderr, "bad problem header\n"); exit(2); }
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

// bnb_sup_word of freddie_cluster.hip
ex_u64 sup_word(const Problem &p, ex_i64 k) {
    const ex_i64 n_sup = (ex_i64)p.sup_cols.size();
    const ex_i64 a = ex_clamp(p.sup_off.at((size_t)k), 0, n_sup), b = ex_clamp(p.sup_off.at((size_t)k + 1), a, n_sup);
    ex_u64 m = 0ull;
    for (ex_i64 s = a; s < b; ++s) { const int c = p.sup_cols.at((size_t)s); if ((unsigned)c < (unsigned)p.R) m |= 1ull << c; }
    return m;
}

void run_problem(const Problem &p) {
    const int R = p.R, E = (int)p.n_inf;
    // ---- k_bnb_prep
    std::vector<ex_u64> tab(2 * (size_t)E + 2, 0ull), conf((size_t)R + 1, 0ull), gsup((size_t)p.n_grp_seg + 1, 0ull);
    for (int k = 0; k < E; ++k) tab.at(2 * (size_t)k) = sup_word(p, k);
    for (int c = 0; c < R; ++c)
        for (ex_i64 x = p.corr_off.at((size_t)c); x < p.corr_off.at((size_t)c + 1); ++x) {
            const int k = ex_find_seg(p.inf_seg.data(), E, p.corr_seg.at((size_t)x));
            if (k >= 0) tab.at(2 * (size_t)k + 1) |= 1ull << c;
        }
    for (size_t i = 0; i + 1 < p.pairs.size(); i += 2) {
        const int a = p.pairs[i], b = p.pairs[i + 1];
        if ((unsigned)a < (unsigned)R && (unsigned)b < (unsigned)R) { conf.at((size_t)a) |= 1ull << b; conf.at((size_t)b) |= 1ull << a; }
    }
    for (ex_i64 s = 0; s < p.n_grp_seg; ++s) {
        const int k = ex_find_seg(p.inf_seg.data(), E, p.grp_seg.at((size_t)s));
        gsup.at((size_t)s) = k >= 0 ? sup_word(p, k) : 0ull;
    }
    // ---- k_bnb_search, task by task
    std::vector<int> g2 = p.g2, rows = p.rows, grp_len = p.grp_len;
    g2.push_back(0); rows.push_back(0); grp_len.push_back(0);
    BnbView v;
    v.tab = tab.data(); v.conf = conf.data(); v.g2 = g2.data(); v.E = E; v.R = R;
    v.r0 = 0; v.r1 = p.n_grp > 0 ? p.n_rows : 0; v.rows = rows.data();
    v.grp0 = 0; v.n_grp = p.n_grp; v.grp_seg_off = p.grp_seg_off.data(); v.n_grp_seg = p.n_grp_seg; v.gsup = gsup.data(); v.grp_len = grp_len.data();
    v.lo_f = p.lo_f; v.hi_f = p.hi_f; v.offset = p.offset; v.max_lg = p.max_lg;
    const int D = R < p.depth ? R : p.depth;
    for (ex_u64 t = 0; t < (1ull << D); ++t) {
        const BnbResult r = bnb_task(v, t, D, p.ub2, p.node_cap);
        printf("%lld %llu %d %d\n", r.cost2, r.mask, r.nodes, r.capped);
    }
}

}  // namespace

int main() {
    Problem p;
    while (read_problem(p)) run_problem(p);
    return 0;
}
