// exact_host_check.cpp -- the per-thread functions of the exact small-problem solve (freddie_amd/csrc/clu_exact.h, what k_exact_prep /
// k_exact_search of freddie_cluster.hip call) run on the host: the transposed table built as the prep kernel builds it, then every mask
// of the problem in slices of `slice` masks, a slice's 256 threads one after the other, the smallest key kept as the atomic minimum keeps
// it.  tools/exact_host_check.py feeds it problems and compares what it prints with the Python mirror (cluster_solve.exact_small).
// Build:  g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -I freddie_amd/csrc tools/exact_host_check.cpp -o exact_host_check
// (every array is a std::vector read through at(): an index outside one stops the run)
//
// Input, whitespace separated, one problem after the other until the end of the input:
//   R slice offset max_lg lo_f hi_f (the doubles as C99 hex floats) | n_inf, inf_seg | sup_off (n_inf + 1), sup_cols | corr_off (R + 1), corr_seg |
//   g2 (R) | n_pairs, pairs (2 each) | n_grp, grp_seg_off (n_grp + 1), grp_seg, grp_len | n_rows, rows (3 each: column, group, l)
// Output per problem:  cost2 mask     (-1 0 when no column set is feasible)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "clu_exact.h"

namespace {

constexpr int kThreads = 256;

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
    int R = 0, slice = 1, offset = 0;
    ex_i64 max_lg = 0, n_inf = 0, n_grp = 0, n_grp_seg = 0, n_rows = 0;
    double lo_f = 1.0, hi_f = 1.0;
    std::vector<int> inf_seg, sup_cols, corr_seg, g2, pairs, grp_seg, grp_len, rows;
    std::vector<ex_i64> sup_off, corr_off, grp_seg_off;
};

bool read_problem(Problem &p) {
    long long v;
    if (!read_int(v)) return false;
    p = Problem();
    p.R = (int)v; p.slice = (int)need_int(); p.offset = (int)need_int(); p.max_lg = need_int();
    p.lo_f = need_double(); p.hi_f = need_double();
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

// exact_sup_word of freddie_cluster.hip
unsigned sup_word(const Problem &p, ex_i64 k) {
    const ex_i64 n_sup = (ex_i64)p.sup_cols.size();
    const ex_i64 a = ex_clamp(p.sup_off.at((size_t)k), 0, n_sup), b = ex_clamp(p.sup_off.at((size_t)k + 1), a, n_sup);
    unsigned m = 0u;
    for (ex_i64 s = a; s < b; ++s) { const int c = p.sup_cols.at((size_t)s); if ((unsigned)c < (unsigned)p.R) m |= 1u << c; }
    return m;
}

void run_problem(const Problem &p) {
    const int R = p.R, E = (int)p.n_inf;
    // ---- k_exact_prep
    std::vector<unsigned> tab(2 * (size_t)E + 2, 0u), conf((size_t)R + 1, 0u), gsup((size_t)p.n_grp_seg + 1, 0u);
    for (int k = 0; k < E; ++k) tab.at(2 * (size_t)k) = sup_word(p, k);
    for (int c = 0; c < R; ++c)
        for (ex_i64 x = p.corr_off.at((size_t)c); x < p.corr_off.at((size_t)c + 1); ++x) {
            const int k = ex_find_seg(p.inf_seg.data(), E, p.corr_seg.at((size_t)x));
            if (k >= 0) tab.at(2 * (size_t)k + 1) |= 1u << c;
        }
    for (size_t i = 0; i + 1 < p.pairs.size(); i += 2) {
        const int a = p.pairs[i], b = p.pairs[i + 1];
        if ((unsigned)a < (unsigned)R && (unsigned)b < (unsigned)R) { conf.at((size_t)a) |= 1u << b; conf.at((size_t)b) |= 1u << a; }
    }
    for (ex_i64 s = 0; s < p.n_grp_seg; ++s) {
        const int k = ex_find_seg(p.inf_seg.data(), E, p.grp_seg.at((size_t)s));
        gsup.at((size_t)s) = k >= 0 ? sup_word(p, k) : 0u;
    }
    // ---- k_exact_search, slice by slice
    const ex_i64 r1 = p.n_grp > 0 ? p.n_rows : 0;
    ex_u64 best = kExactKeyNone;
    const ex_i64 total = 1ll << R;
    for (ex_i64 lo = 0; lo < total; lo += p.slice) {
        const unsigned n = (unsigned)(total - lo < p.slice ? total - lo : p.slice);
        ex_u64 slice_best = kExactKeyNone;
        for (int tid = 0; tid < kThreads; ++tid)
            for (unsigned i = (unsigned)tid; i < n; i += kThreads) {
                const ex_u64 kk = ex_mask_key((unsigned)lo + i, tab.data(), E, conf.data(), p.g2.data(), R, 0, r1, p.rows.data(), 0, p.n_grp, p.grp_seg_off.data(),
                                              p.n_grp_seg, gsup.data(), p.grp_len.data(), p.lo_f, p.hi_f, p.offset, p.max_lg);
                slice_best = kk < slice_best ? kk : slice_best;
            }
        best = slice_best < best ? slice_best : best;
    }
    if (best == kExactKeyNone) printf("-1 0\n");
    else printf("%lld %u\n", ex_key_cost2(best), ex_key_mask(best));
}

}  // namespace

int main() {
    Problem p;
    while (read_problem(p)) run_problem(p);
    return 0;
}
