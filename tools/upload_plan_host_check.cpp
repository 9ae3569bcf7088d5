// upload_plan_host_check.cpp -- the upload's host plan (freddie_amd/csrc/seg_upload_plan.h) and the reaction to a run's status
// record (freddie_amd/csrc/seg_run_react.h) without a GPU.  Reads cases from stdin:
//     batch hist16=<0|1> yraw16=<0|1>             then one line per array of fseg_batch, "<name> v,v,v" (an array a refusal
//     part_iv_off 0,2                             never reaches may be left out), then
//     end
// prints "plan <rc> <message>" and, for an accepted batch, the plan's members and every table of fill_upload_tables(), a line
// each.  Every table is allocated at exactly the plan's count, so the address sanitizer sees any write past it.
//     react kind=<A|B|R> err=<n> <Status member>=<n> ... have_huge=.. dp_wide_counts=.. run_events_only=.. nm_giant=.. cap=<7 values>
// prints the Reaction of decide_reaction(), a line.  tests/test_upload_plan_host.py builds this with the address and
// undefined-behaviour sanitizers and holds what both must give.
//     g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include -I freddie_amd/csrc tools/upload_plan_host_check.cpp
#include "seg_run_react.h"

#include <cstdlib>
#include <iostream>
#include <map>
#include <memory>
#include <sstream>
#include <string>

using namespace fseg;

template <typename T>
static std::vector<T> read_list(const std::string &v) {
    std::vector<T> out;
    std::istringstream in(v);
    std::string piece;
    while (std::getline(in, piece, ',')) out.push_back((T)atoll(piece.c_str()));
    return out;
}
static std::map<std::string, std::string> read_fields(std::istringstream &fields) {
    std::map<std::string, std::string> kv;
    std::string field;
    while (fields >> field) {
        const size_t eq = field.find('=');
        if (eq == std::string::npos) { fprintf(stderr, "no '=' in \"%s\"\n", field.c_str()); exit(2); }
        kv[field.substr(0, eq)] = field.substr(eq + 1);
    }
    return kv;
}
template <typename T>
static void print_row(const char *name, const T *v, size_t n) {
    printf("%s", name);
    for (size_t i = 0; i < n; ++i) printf(" %lld", (long long)v[i]);
    printf("\n");
}
template <typename T> static std::unique_ptr<T[]> exactly(size_t n) { return std::unique_ptr<T[]>(new T[n]); }

static int do_batch(std::istringstream &head) {
    const auto opt = read_fields(head);
    std::map<std::string, std::string> rows;
    std::string line;
    while (std::getline(std::cin, line) && line != "end") {
        const size_t sp = line.find(' ');
        rows[line.substr(0, sp)] = sp == std::string::npos ? "" : line.substr(sp + 1);
    }
    const auto part_iv_off = read_list<int64_t>(rows["part_iv_off"]), part_rep_off = read_list<int64_t>(rows["part_rep_off"]),
               rep_exon_off = read_list<int64_t>(rows["rep_exon_off"]);
    const auto iv_start = read_list<int32_t>(rows["iv_start"]), iv_end = read_list<int32_t>(rows["iv_end"]), rep_weight = read_list<int32_t>(rows["rep_weight"]),
               ex_ts = read_list<int32_t>(rows["ex_ts"]), ex_te = read_list<int32_t>(rows["ex_te"]);
    fseg_batch b{};
    b.n_part = (int)part_iv_off.size() - 1;
    b.part_iv_off = part_iv_off.data(); b.iv_start = iv_start.data(); b.iv_end = iv_end.data();
    b.part_rep_off = part_rep_off.data(); b.rep_weight = rep_weight.data(); b.rep_exon_off = rep_exon_off.data();
    b.ex_ts = ex_ts.data(); b.ex_te = ex_te.data();
    const UploadPlan pl = plan_upload(b, atoi(opt.at("hist16").c_str()), atoi(opt.at("yraw16").c_str()));
    printf("plan %d %s\n", pl.rc, pl.msg);
    if (pl.rc != FSEG_OK) { printf("end\n"); return 0; }
    const BatchFacts &f = pl.batch;
    printf("facts %d %lld %lld %lld %lld %lld %lld %lld %d %d %d %lld %d %d %d\n", f.n_part, f.K, f.R, f.I, f.NPOS, f.LANES, f.max_part_pos, f.max_part_lanes,
           f.n_tiles, f.n_hist_chunks, f.n_rep_blocks, f.max_rep_exons, (int)f.expanded, (int)f.hist_packed, (int)f.yraw_narrow);
    printf("more %lld %d %lld %lld\n", pl.max_part_reps, pl.hist_chunk, pl.nb, pl.nbp);
    printf("counts %zu %zu %zu %zu %zu %zu %zu\n", pl.n.part_off, pl.n.iv, pl.n.pos_off, pl.n.tiles, pl.n.blk_iv0, pl.n.rep_blocks, pl.n.chunks);
    print_row("part_pos", pl.part_pos.data(), pl.part_pos.size());
    print_row("part_lanes", pl.part_lanes.data(), pl.part_lanes.size());
    auto pos_off = exactly<i64>(pl.n.pos_off), part_lane_off = exactly<i64>(pl.n.part_off), hc_p0 = exactly<i64>(pl.n.chunks);
    auto iv_part = exactly<int>(pl.n.iv), iv_tile0 = exactly<int>(pl.n.iv), blk_iv0 = exactly<int>(pl.n.blk_iv0);
    auto rb_part = exactly<int>(pl.n.rep_blocks), rb_r0 = exactly<int>(pl.n.rep_blocks);
    auto hc_part = exactly<int>(pl.n.chunks), hc_n = exactly<int>(pl.n.chunks), hc_glo = exactly<int>(pl.n.chunks), hc_ghi = exactly<int>(pl.n.chunks);
    auto tile_desc = exactly<TileDesc>(pl.n.tiles);
    fill_upload_tables(b, pl, UploadTables{pos_off.get(), part_lane_off.get(), iv_part.get(), iv_tile0.get(), tile_desc.get(), blk_iv0.get(),
                                           rb_part.get(), rb_r0.get(), hc_part.get(), hc_p0.get(), hc_n.get(), hc_glo.get(), hc_ghi.get()});
    print_row("pos_off", pos_off.get(), pl.n.pos_off);
    print_row("part_lane_off", part_lane_off.get(), pl.n.part_off);
    print_row("iv_part", iv_part.get(), pl.n.iv);
    print_row("iv_tile0", iv_tile0.get(), pl.n.iv);
    printf("tile_desc");
    for (size_t i = 0; i < pl.n.tiles; ++i) printf(" %lld:%d:%d", tile_desc[i].base, tile_desc[i].y0, tile_desc[i].len);
    printf("\n");
    print_row("blk_iv0", blk_iv0.get(), pl.n.blk_iv0);
    print_row("rb_part", rb_part.get(), pl.n.rep_blocks);
    print_row("rb_r0", rb_r0.get(), pl.n.rep_blocks);
    print_row("hc_part", hc_part.get(), pl.n.chunks);
    print_row("hc_p0", hc_p0.get(), pl.n.chunks);
    print_row("hc_n", hc_n.get(), pl.n.chunks);
    print_row("hc_glo", hc_glo.get(), pl.n.chunks);
    print_row("hc_ghi", hc_ghi.get(), pl.n.chunks);
    printf("end\n");
    return 0;
}

static int do_react(std::istringstream &fields) {
    Status s{};
    ReactFacts f;
    RunKind kind = RunKind::Replay;
    for (const auto &[key, v] : read_fields(fields)) {
        const unsigned long long num = strtoull(v.c_str(), nullptr, 0);
        if (key == "kind") kind = v == "A" ? RunKind::SizedA : (v == "B" ? RunKind::SizedB : RunKind::Replay);
        else if (key == "err") s.err = (unsigned)num;
        else if (key == "n_prob") s.n_prob = num;
        else if (key == "n_work") s.n_work = num;
        else if (key == "pair_used") s.pair_used = num;
        else if (key == "tri_used") s.tri_used = num;
        else if (key == "label_bytes") s.label_bytes = num;
        else if (key == "n_vchunks") s.n_vchunks = num;
        else if (key == "cov_used") s.cov_used = num;
        else if (key == "max_n") s.max_n = (unsigned)num;
        else if (key == "max_ln") s.max_ln = (unsigned)num;
        else if (key == "dp_huge") s.dp_cls[2] = num;
        else if (key == "have_huge") f.have_huge = num != 0;
        else if (key == "dp_wide_counts") f.dp_wide_counts = num != 0;
        else if (key == "run_events_only") f.run_events_only = num != 0;
        else if (key == "nm_giant") f.nm_giant = (int)num;
        else if (key == "cap") { const auto c = read_list<i64>(v); if (c.size() != CAP_COUNT) return 2; for (int k = 0; k < CAP_COUNT; ++k) f.cap[k] = c[(size_t)k]; }
        else { fprintf(stderr, "bad field \"%s\"\n", key.c_str()); return 2; }
    }
    const Reaction r = decide_reaction(s, f, kind);
    static const char *const outcomes[] = {"done", "redo", "fail"}, *const fails[] = {"none", "input", "sized_overflow", "timeout_no_waiters"};
    printf("reaction %s %s attempt=%d scan_fallback=%d wave_off=%d sync_timeout=%d nm_big_max=%d have_huge=%d dp_wide_counts=%d giant=%d adopt_counts=%d cap=",
           outcomes[(int)r.outcome], fails[(int)r.fail], (int)r.uses_attempt, (int)r.scan_fallback, (int)r.wave_off, (int)r.sync_timeout, (int)r.nm_big_max,
           (int)r.have_huge, (int)r.dp_wide_counts, (int)r.giant, (int)r.adopt_counts);
    for (int k = 0; k < CAP_COUNT; ++k) printf("%s%lld", k ? "," : "", r.cap[k]);
    printf("\n");
    return 0;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream fields(line);
        std::string what;
        fields >> what;
        int rc = 2;
        if (what == "batch") rc = do_batch(fields);
        else if (what == "react") rc = do_react(fields);
        else fprintf(stderr, "unknown case \"%s\"\n", what.c_str());
        if (rc) return rc;
    }
    return 0;
}
