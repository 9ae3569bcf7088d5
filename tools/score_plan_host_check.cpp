// score_plan_host_check.cpp -- the scoring stage's launch list (freddie_amd/csrc/seg_score_plan.h) without a GPU.
// Reads one case per line from stdin, "key=value" fields separated by blanks (flags 0 / 1, arrays comma-separated, plan= the
// FSEG_SCORE_PLAN string, possibly empty; what a line leaves out keeps ScoreFacts' default), and prints per case
//     plan <on> <n_seg> <used x4> <side_of x4> <n_wide_all> <wide_one>
//     op <kind> <cls> <cnt_bytes> <dpw_threads> <n> <lane>        (one line per launch, in host order)
//     end
// tests/test_score_plan_host.py builds it with the address and undefined-behaviour sanitizers and holds the expected lists.
//     g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I freddie_amd/csrc tools/score_plan_host_check.cpp
#include "seg_score_plan.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

using namespace fseg;

static const char *kind_name(ScoreKind k) {
    switch (k) {
    case ScoreKind::Score: return "score";
    case ScoreKind::SolveFused: return "fused";
    case ScoreKind::SolveSplit: return "split";
    case ScoreKind::WideAll: return "wide_all";
    case ScoreKind::Wave: return "wave";
    case ScoreKind::Tiny: return "tiny";
    case ScoreKind::GateG: return "gate_g";
    case ScoreKind::GateH: return "gate_h";
    }
    return "?";
}

template <typename T, int N>
static bool read_list(const std::string &v, T (&out)[N]) {
    std::istringstream in(v);
    std::string piece;
    int n = 0;
    while (std::getline(in, piece, ',')) { if (n == N) return false; out[n++] = (T)atoll(piece.c_str()); }
    return n == N;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        ScoreFacts f;
        std::string plan;
        bool do_score = true;
        std::istringstream fields(line);
        std::string field;
        while (fields >> field) {
            const size_t eq = field.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "no '=' in \"%s\"\n", field.c_str()); return 2; }
            const std::string key = field.substr(0, eq), v = field.substr(eq + 1);
            const long long num = atoll(v.c_str());
            bool ok = true;
            if (key == "plan") plan = v;
            else if (key == "do_score") do_score = num != 0;
            else if (key == "known") f.known = num != 0;
            else if (key == "small_batch") f.small_batch = num != 0;
            else if (key == "any_arena") f.any_arena = num != 0;
            else if (key == "fuse") f.fuse = num != 0;
            else if (key == "tiny_on") f.tiny_on = num != 0;
            else if (key == "wave") f.wave = num != 0;
            else if (key == "forking") f.forking = num != 0;
            else if (key == "wide_solve") f.wide_solve = num != 0;
            else if (key == "key32") f.key32 = num != 0;
            else if (key == "n_solve") ok = read_list(v, f.n_solve);
            else if (key == "n_wide") ok = read_list(v, f.n_wide);
            else if (key == "n_tiny") f.n_tiny = num;
            else if (key == "n_cls_work") ok = read_list(v, f.n_cls_work);
            else if (key == "prob_cap") f.prob_cap = num;
            else if (key == "split_dp") f.split_dp = (int)num;
            else if (key == "dpx_n") ok = read_list(v, f.dpx_n);
            else if (key == "dpx_cnt") ok = read_list(v, f.dpx_cnt);
            else if (key == "dpx_nm_fits") f.dpx_nm_fits = num != 0;
            else if (key == "dpx_arena") f.dpx_arena = num != 0;
            else if (key == "split_grid_cap") f.split_grid_cap = num;
            else if (key == "wide_one_max") f.wide_one_max = num;
            else ok = false;
            if (!ok) { fprintf(stderr, "bad field \"%s\"\n", field.c_str()); return 2; }
        }
        const ScorePlan p = parse_score_plan(f, plan.c_str(), do_score);
        ScoreOps ops;
        plan_score_ops(f, p, ops);
        printf("plan %d %d %d %d %d %d %d %d %d %d %lld %d\n", (int)p.on, p.n_seg, (int)p.used[0], (int)p.used[1], (int)p.used[2], (int)p.used[3],
               p.side_of[0], p.side_of[1], p.side_of[2], p.side_of[3], p.n_wide_all, (int)p.wide_one);
        for (int i = 0; i < ops.n; ++i) {
            const ScoreOp &o = ops.op[i];
            printf("op %s %d %d %d %lld %d\n", kind_name(o.kind), o.cls, o.cnt_bytes, o.dpw_threads, o.n, o.lane);
        }
        printf("end\n");
    }
    return 0;
}
