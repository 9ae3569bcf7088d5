// bnb_passes_host_check.cpp -- the passes of the branch and bound over a round's problems of up to 1024 columns run on the host: the
// walk on a prefix, the roll-back of a capped task and its open children (bw_task_from, bw_open_include, bw_open_count, bw_open_emit of
// freddie_amd/csrc/clu_bnb_wide.h, what k_bw_search / k_bw_search_from / k_bw_emit of freddie_cluster.hip call), the lanes of a wave one
// after another (BwHostWave).  A pass's tasks are the records the pass before wrote, in the order it wrote them, each bounded by the
// smaller of ub2 and the best cost2 of the passes before.  tools/bnb_passes_host_check.py feeds it problems and compares what it prints,
// task by task, with the Python mirror (cluster_solve.bnb_prefix_task on exact_bnb_wide's tables).
// Build:  g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I freddie_amd/csrc tools/bnb_passes_host_check.cpp -o bnb_passes_host_check
// (every array is a std::vector of its exact size; the sanitizers stop a read outside one)
//
// Input: "passes max_tasks" and then a problem of tools/bnb_host_check.cpp, R up to 1024.
// Output per task:  pass L cost2 nodes capped open mask     (the mask as one hexadecimal number; -1 and 0 when the task found no leaf)
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
    int R = 0, depth = 0, node_cap = 1, offset = 0, passes = 1;
    ex_i64 ub2 = -1, max_lg = 0, n_inf = 0, n_grp = 0, n_grp_seg = 0, n_rows = 0, max_tasks = 0;
    double lo_f = 1.0, hi_f = 1.0;
    std::vector<int> inf_seg, sup_cols, corr_seg, g2, pairs, grp_seg, grp_len, rows;
    std::vector<ex_i64> sup_off, corr_off, grp_seg_off;
};

bool read_problem(Problem &p) {
    long long v;
    if (!read_int(v)) return false;
    p = Problem();
    p.passes = (int)v; p.max_tasks = need_int();
    p.R = (int)need_int(); p.depth = (int)need_int(); p.node_cap = (int)need_int(); p.ub2 = need_int(); p.offset = (int)need_int(); p.max_lg = need_int();
    p.lo_f = need_double(); p.hi_f = need_double();
    if (p.R < 0 || p.R > kBwMaxCols || p.depth < 0 || p.depth > 20 || p.node_cap < 1 || p.passes < 1 || p.max_tasks < 1) { fprintf(stderr, "bad problem header\n"); exit(2); }
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
    const int R = p.R, E = (int)p.n_inf, W = bw_words(R), EW = bw_ewords(E), rw = bw_record_words(W);
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
    // ---- the passes
    std::vector<ex_u64> st((size_t)bw_state_words(W, EW), ~0ull);
    BwView v;
    v.icol = icol.data(); v.ccol = ccol.data(); v.conf = conf.data(); v.g2 = p.g2.data(); v.E = E; v.R = R; v.W = W; v.EW = EW;
    v.r0 = 0; v.r1 = p.n_grp > 0 ? p.n_rows : 0; v.rows = p.rows.data();
    v.grp0 = 0; v.n_grp = p.n_grp; v.grp_seg_off = p.grp_seg_off.data(); v.n_grp_seg = p.n_grp_seg; v.gk = gk.data(); v.grp_len = p.grp_len.data();
    v.lo_f = p.lo_f; v.hi_f = p.hi_f; v.offset = p.offset; v.max_lg = p.max_lg;
    v.st = st.data();
    BwHostWave wv;
    const int D = R < p.depth ? R : p.depth;
    std::vector<ex_u64> recs((size_t)rw << D, 0ull), next;   // pass 1: the prefixes (t, D)
    for (ex_u64 t = 0; t < (1ull << D); ++t) { recs[(size_t)t * rw] = (ex_u64)D; recs[(size_t)t * rw + 1] = t; }
    ex_i64 found2 = -1;
    for (int pass = 1; pass <= p.passes && !recs.empty(); ++pass) {
        const ex_i64 bound = found2 < 0 ? p.ub2 : p.ub2 < 0 ? found2 : found2 < p.ub2 ? found2 : p.ub2;
        const size_t n_tasks = recs.size() / (size_t)rw;
        next.clear();
        ex_i64 pass2 = -1;
        for (size_t i = 0; i < n_tasks; ++i) {
            const ex_u64 *rec = recs.data() + i * (size_t)rw;
            const int L = (int)rec[0];
            // (the first pass through bw_task, as k_bw_search runs it)
            const BwResult r = pass == 1 ? bw_task(v, wv, rec[1], D, bound, p.node_cap) : bw_task_from(v, wv, rec + 1, W, L, bound, p.node_cap);
            int n_open = 0;
            if (r.capped) {
                const ex_u64 *S = st.data(), *tin = S + 2 * W, *tout = S + 3 * W;
                const bool inc = bw_open_include(wv, conf.data() + (size_t)r.d * W, S, tin, r.d, W);
                n_open = bw_open_count(tout, L, r.d, W, inc);
                const size_t at = next.size();
                next.resize(at + (size_t)n_open * rw, ~0ull);  // exactly the counted records: the sanitizer stops a write beyond them
                const int wrote = bw_open_emit(wv, S, tout, L, r.d, W, inc, next.data() + at, n_open);
                if (wrote != n_open) { fprintf(stderr, "%d records counted, %d written\n", n_open, wrote); exit(3); }
            }
            if (r.cost2 >= 0 && (pass2 < 0 || r.cost2 < pass2)) pass2 = r.cost2;
            printf("%d %d %lld %d %d %d ", pass, L, r.cost2, r.nodes, r.capped, n_open);
            for (int w = W - 1; w >= 0; --w) printf("%016llx", st[4 * (size_t)W + w]);
            printf("\n");
        }
        if (pass2 >= 0 && (found2 < 0 || pass2 < found2)) found2 = pass2;
        if ((ex_i64)(next.size() / (size_t)rw) > p.max_tasks) break;
        recs.swap(next);
    }
}

}  // namespace

int main() {
    Problem p;
    while (read_problem(p)) run_problem(p);
    return 0;
}
