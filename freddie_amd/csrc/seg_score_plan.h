// seg_score_plan.h -- what the interval-scoring stage launches: which kernel instance over which list, on which stream, in which
// host order.  One decision, as plain C++ (no HIP, nothing of seg_common.h): enqueue_run fills in ScoreFacts, parses the plan and
// walks the list plan_score_ops() returns; tools/score_plan_host_check.cpp prints that list without a GPU
// (tests/test_score_plan_host.py holds the lists the rules must give).
//
// Two ways a problem is scored (prob_kind): the arena path's work items (k_score per size class) and the problems that see few
// reads, whole, one workgroup each (k_solve per size class: 8-bit counters up to 255 reads, 16-bit counters for the class's "wide"
// problems); the problems with a handful of candidates take a wave each (k_wave, or k_tiny).  A batch usually holds only one kind.
#pragma once
#include <cstring>

namespace fseg {

// FSEG_SCORE_PLAN (default "gM|W|hB|gST"): how the k_solve / k_wave launches of a batch share the chip.  Streams separated by
// '|' (the first is the main stream; the segments that have something to launch take the side streams in order); B M S T = the
// large / mid / small / tiny class -- a class on the split path is k_solve (rounds) followed by k_dpw (its DPs) --, W = the
// 16-bit-counter instances over the wide problems, g = k_gate (wait until the large class's workgroups, both instances', are
// placed), h = wait until the 16-bit instance's are.  Any other character launches nothing.
// Measured on config4 (250 k-read batch, stage alone, tools/r4_plans.sh):
//   * everything on the main stream 0.19-0.21 ms; a stream each without a gate 0.21 (the dispatcher runs them in the reverse of
//     their launch order: a large-class workgroup needs eight wave slots and half a CU's LDS at once);
//   * round 3's "BM|gTS" 0.161-0.165: the tiny class in the large class's shadow, then small beside mid;
//   * a cross-stream dependency costs ~9 us (fork or join), so the chain that ends LAST belongs on the main stream, where the
//     stage's end needs no join: the mid class (gate, rounds, DPs) on main, the large class on a side stream of its own, tiny +
//     small on a third: 0.144-0.149 with the split path ("B|gM|gTS"; the same chains with the large class on main: 0.154-0.167;
//     per-problem clocks, tools/r4_ticks.sh: 133 us from first start to last end either way);
//   * the 16-bit instances first (batches of 1 000-read partitions): see the passes in parse_score_plan().
// A plan is used by a sized batch of k_solve / k_wave problems only whose run forks (ScorePlan::on); anything that does not name
// each class once, batches with arena-path problems and small batches keep the chains of plan_score_ops().
constexpr int kScorePlanChars = 31;     // what fseg_ctx::score_plan holds
constexpr int kScoreSide = 3;           // side streams of a context (fseg_ctx::kSide)

// each of B M S T exactly once, at most a side stream per '|' (read_switches: a plan that fails is dropped, the batch runs unplanned)
inline bool score_plan_valid(const char *s) {
    int seen[4] = {0, 0, 0, 0}, bars = 0;
    size_t len = 0;
    static const char kinds[] = "BMST";
    for (; s[len]; ++len) {
        if (const char *at = static_cast<const char *>(memchr(kinds, s[len], 4))) ++seen[at - kinds];
        bars += s[len] == '|';
    }
    return seen[0] == 1 && seen[1] == 1 && seen[2] == 1 && seen[3] == 1 && bars <= kScoreSide && len <= (size_t)kScorePlanChars;
}

// what the stage's decisions read, filled in once per enqueue
struct ScoreFacts {
    bool known = false;         // list sizes known (the batch has been sized or has run): launches over an empty list are left out
    bool small_batch = false, any_arena = false;
    bool fuse = false;          // the batch's problems go to k_solve (use_fuse && fuse_on)
    bool tiny_on = false, wave = false;
    bool forking = false;       // the run may use the side streams
    bool wide_solve = false;    // some problem of the batch sees more than kFuseLanes reads
    bool key32 = false;         // 32-bit DP keys (no sum of a chain can reach 2^24)
    long long n_solve[3] = {0, 0, 0}, n_wide[3] = {0, 0, 0}, n_tiny = 0, n_cls_work[4] = {0, 0, 0, 0}, prob_cap = 0;
    // the hand-over arena between k_solve<.., SPLIT> and k_dpw as alloc_arenas() laid it out
    int split_dp = 0;           // FSEG_SPLIT_DP: bit 0 / 1 / 2 = the small / mid / large class hands its DPs to k_dpw, bit 3 = the large class's k_dpw by one wave
    long long dpx_n[3] = {0, 0, 0};
    int dpx_cnt[3] = {1, 1, 1};
    bool dpx_nm_fits = false;   // laid out for this batch's largest problem (dpx_nm == nm_big)
    bool dpx_arena = false;     // ... and allocated
    long long split_grid_cap = 0, wide_one_max = 0;     // kSplitGridCap, fseg_ctx::kWideOneMax
};

// one character of a plan: what it is, the segment it is in, the pass that launches it
struct PlanItem { char what; signed char seg, pass; };
struct ScorePlan {
    bool on = false;            // this enqueue launches by the plan
    int n_seg = 1;
    bool used[4] = {true, false, false, false};     // a stream whose kernels have nothing to do is left alone
    int side_of[4] = {-1, -1, -1, -1};
    long long n_wide_all = 0;
    bool wide_one = false, has_w = false;
    int n_item = 0;
    PlanItem item[kScorePlanChars];
};

// The plan string, parsed once.  `do_score`: this enqueue holds the scoring stage.
// W: the problems of every class that see more than kFuseLanes reads -- a handful per batch, most of which keep fewer and are
// only looked at -- in ONE launch of the large class's 16-bit instance, a workgroup each (as a launch per class on the tiny
// class's stream they held it back 46-60 us on config3 / config5: tools/run_gaps.py); batches with more than wide_one_max such problems keep the
// per-class instances (in a row on W's stream).
// Three passes order the host's launches: the large class's launches that OPEN their stream go out first -- the 16-bit instance
// (W, pass 0), then the 8-bit one (B, behind `h` = a gate on W's workgroups having started: pass 1; an `h` leaves its segment
// still opening) --, everything else follows in plan order (pass 2; a stream's own order is kept).  Why: a workgroup of the
// 16-bit instance holds up to 120 KB of LDS (n <= 60: planes 28 + coverage 16 + 16-bit counters 68 KB) and fits no CU that has
// one of the 8-bit instance's (81 KB); enqueued behind it, config3's one real wide problem was placed 135-150 us into the stage,
// when the 8-bit instance and the classes behind the gate had drained, and the stage took 0.29 ms (tools/stage_timeline.py).  A class has a handful of
// wide problems: placed first they take a few CUs and the 8-bit instance the rest.
inline ScorePlan parse_score_plan(const ScoreFacts &f, const char *plan, bool do_score) {
    ScorePlan p;
    p.on = do_score && f.prob_cap > 0 && f.known && !f.any_arena && !f.small_batch && f.forking && f.n_solve[2] > 0 && f.fuse && f.wave && score_plan_valid(plan);
    if (!p.on) return p;
    p.n_wide_all = f.n_wide[0] + f.n_wide[1] + f.n_wide[2];
    p.has_w = strchr(plan, 'W') != nullptr;
    p.wide_one = p.n_wide_all <= f.wide_one_max && p.has_w;
    bool opens = true;
    for (const char *q = plan; *q; ++q) {
        if (*q == '|') { ++p.n_seg; opens = true; continue; }
        const int seg = p.n_seg - 1;
        if (*q != 'W' || (f.wide_solve && p.n_wide_all > 0)) p.used[seg] = true;
        const int pass = !opens ? 2 : (*q == 'W' ? 0 : ((*q == 'B' || *q == 'h') ? 1 : 2));
        if (*q != 'h') opens = false;
        p.item[p.n_item++] = PlanItem{*q, (signed char)seg, (signed char)pass};
    }
    // (the segments that have something to launch take the side streams in order: the first ones start first)
    for (int k = 1, nx = 0; k < p.n_seg; ++k) if (p.used[k]) p.side_of[k] = nx++;
    return p;
}

// One launch of the stage: one kernel instance over one list on one stream.
enum class ScoreKind {
    Score,          // k_score of a class (the arena path's work items; the grid follows the arena's capacity: n is 0)
    SolveFused,     // k_solve, the DP as its workgroups' tail
    SolveSplit,     // k_solve<.., SPLIT>, followed by its k_dpw on the same stream
    WideAll,        // k_solve<kNMax, 16-bit> over every class's wide problems (wide_all), a workgroup each
    Wave, Tiny,     // k_wave / k_tiny over the tiny problems' list
    GateG, GateH,   // k_gate on the large class's workgroups (n of them) / on its 16-bit instance's
};
struct ScoreOp {
    ScoreKind kind;
    int cls;            // 0 / 1 / 2 the small / mid / large class, 3 the tiny problems' list, -1 every class in one launch
    int cnt_bytes;      // k_solve: counter width (1 or 2); 0 elsewhere
    int dpw_threads;    // SolveSplit: k_dpw's workgroup (512 or 64); 0 elsewhere
    long long n;        // the items the grid is computed from (a gate: the workgroups it waits for)
    int lane;           // -1 the main stream, 0..2 that side stream
};
// The longest list is a plan's: a plan has at most kScorePlanChars characters, a character launches at most three kernels (a W
// of a batch with more than wide_one_max wide problems: a 16-bit instance per class; B M S: two instances; T g h: one) -- 93.
// Without a plan: three chains of a k_score and two k_solve instances, and the tiny kernel -- 10.
constexpr int kScoreOpsMax = 3 * kScorePlanChars;
struct ScoreOps {
    int n = 0;
    ScoreOp op[kScoreOpsMax];
    void push(const ScoreOp &o) { if (n < kScoreOpsMax) op[n++] = o; }
};

// the bounds of solve list `l` (0..2 the classes, 3 the tiny problems, < 0 the three classes together) when the host knows them
inline long long list_lb(const ScoreFacts &f, int l) {
    return !f.known ? -1 : (l <= 0 ? 0 : (l == 1 ? f.n_solve[0] : (l == 2 ? f.n_solve[0] + f.n_solve[1] : f.n_solve[0] + f.n_solve[1] + f.n_solve[2])));
}
inline long long list_ln(const ScoreFacts &f, int l) {
    return !f.known ? -1 : (l < 0 ? f.n_solve[0] + f.n_solve[1] + f.n_solve[2] : (l == 3 ? f.n_tiny : f.n_solve[l]));
}
// (a 16-bit-counter instance of a sized batch goes over its class's WIDE problems only: wide_n of them, through wide_items)
inline long long wide_n(const ScoreFacts &f, int cls, int cnt_bytes) { return (f.known && cls >= 0 && cls < 3 && cnt_bytes == 2) ? f.n_wide[cls] : -1; }
// the class's 16-bit instance has something to do
inline bool wide_needed(const ScoreFacts &f, int cls) { return !f.known || (f.wide_solve && (cls < 0 || f.n_wide[cls] > 0)); }
// the split path (k_solve<.., SPLIT> then k_dpw on the same stream) for a list that fits the hand-over arena as laid out.
// (Until round 5 only where the context has the device to itself: host memory -> host memory, eight contexts, the two were
// within the noise -- 383 against 388 M reads/s; over resident batches the split is 1.8 % faster; FSEG_SPLIT_ALWAYS=0.)
// (k_dpw takes the problem its workgroup index names -- no grid stride --, so a list longer than the grid cap of the two launches
// keeps the DP as k_solve's tail)
inline bool split_ok(const ScoreFacts &f, int cls, int cnt_bytes) {
    return f.known && cls >= 0 && cls < 3 && ((f.split_dp >> cls) & 1) && f.dpx_n[cls] > 0 && f.n_solve[cls] <= f.dpx_n[cls] && f.dpx_nm_fits &&
           f.n_solve[cls] <= f.split_grid_cap && cnt_bytes <= f.dpx_cnt[cls] && f.dpx_arena;
}

// the k_solve launches of one class over n_items problems on `lane`; which: 1 = the instance with 8-bit counters, 2 = the one
// with 16-bit counters if the class has problems for it, 3 = both, back to back
inline void push_solve(const ScoreFacts &f, ScoreOps &out, int lane, int cls, long long n_items, int which) {
    const bool wide = wide_needed(f, cls);
    // (a class that needs the wide instance asks for a hand-over arena of two counter bytes, also where only the 8-bit instance
    // is being launched: both instances of a class take the same path)
    const bool split = split_ok(f, cls, wide ? 2 : 1);
    // the large class's DPs by workgroups of eight waves (k_dpw<.., 512>: 27 us alone instead of 38; FSEG_SPLIT_DP bit 3: by one)
    const int dpw = !split ? 0 : ((cls == 2 && !(f.split_dp & 8)) ? 512 : 64);
    for (int cnt = 1; cnt <= 2; ++cnt) {
        if (!(which & cnt) || (cnt == 2 && !wide)) continue;
        const long long wn = wide_n(f, cls, cnt);
        out.push(ScoreOp{split ? ScoreKind::SolveSplit : ScoreKind::SolveFused, cls, cnt, dpw, wn >= 0 ? wn : n_items, lane});
    }
}

inline void plan_score_ops(const ScoreFacts &f, const ScorePlan &p, ScoreOps &out) {
    out.n = 0;
    if (f.prob_cap <= 0) return;
    const bool any_solve = f.fuse && (!f.known || f.n_solve[0] + f.n_solve[1] + f.n_solve[2] > 0);
    const long long cap = f.prob_cap;
    if (p.on) {
        // (a plan with W: B M S launch their 8-bit instances only; without: both instances, one after the other)
        const int wb = p.has_w ? 1 : 3;
        // the large class's workgroups a start gate waits for: the 8-bit instance's and the 16-bit instance's (one per wide
        // problem) -- the latter need 90 KB of LDS each and find no room once the other classes are in
        const long long wide_wgs = p.wide_one ? (f.wide_solve ? p.n_wide_all : 0) : (wide_needed(f, 2) ? f.n_wide[2] : 0);
        const long long big_wgs = f.n_solve[2] + wide_wgs;
        for (int pass = 0; pass < 3; ++pass)
            for (int i = 0; i < p.n_item; ++i) {
                const PlanItem &it = p.item[i];
                if (!p.used[it.seg] || it.pass != pass) continue;
                const int lane = it.seg == 0 ? -1 : p.side_of[it.seg];
                switch (it.what) {      // (an empty class launches nothing; its gate still does)
                case 'B': push_solve(f, out, lane, 2, f.n_solve[2], wb); break;
                case 'M': if (f.n_solve[1] > 0) push_solve(f, out, lane, 1, f.n_solve[1], wb); break;
                case 'S': if (f.n_solve[0] > 0) push_solve(f, out, lane, 0, f.n_solve[0], wb); break;
                case 'W':
                    if (!f.wide_solve || p.n_wide_all == 0) break;
                    if (p.wide_one) {   // (the DP stays the workgroup's tail: nothing to hand over, no second placement)
                        out.push(ScoreOp{ScoreKind::WideAll, -1, 2, 0, p.n_wide_all, lane});
                    } else {
                        for (int cls = 2; cls >= 0; --cls) if (cls == 2 || f.n_solve[cls] > 0) push_solve(f, out, lane, cls, f.n_solve[cls], 2);
                    }
                    break;
                case 'T': if (f.n_tiny > 0) out.push(ScoreOp{ScoreKind::Wave, 3, 0, 0, f.n_tiny, lane}); break;
                case 'g': out.push(ScoreOp{ScoreKind::GateG, 2, 0, 0, big_wgs < 512 ? big_wgs : 512, lane}); break;
                case 'h':               // the 16-bit instance's workgroups (up to 120 KB of LDS each) take their CUs first
                    if (wide_wgs > 0) out.push(ScoreOp{ScoreKind::GateH, 2, 0, 0, wide_wgs < 256 ? wide_wgs : 256, lane});
                    break;
                default: break;
                }
            }
        return;
    }
    // Without a plan the classes' chains take side streams only beside the arena path's work-item kernels (and only in a run
    // that forks): batches of k_solve problems alone that cannot use a plan keep to the main stream.
    const bool side = f.any_arena && f.forking;
    if (f.small_batch) {        // few work items, few problems: one launch for every size class
        if (f.any_arena) out.push(ScoreOp{ScoreKind::Score, -1, 0, 0, 0, -1});
        if (any_solve) push_solve(f, out, -1, -1, f.known ? f.n_solve[0] + f.n_solve[1] + f.n_solve[2] : cap, 3);
    } else {                    // the size classes own disjoint problems: three chains, large (the long pole) on main, mid, small
        for (int cls = 2; cls >= 0; --cls) {
            const int lane = (cls == 2 || !side) ? -1 : 1 - cls;
            if (f.any_arena && (!f.known || f.n_cls_work[cls] > 0)) out.push(ScoreOp{ScoreKind::Score, cls, 0, 0, 0, lane});
            if (any_solve && (!f.known || f.n_solve[cls] > 0)) push_solve(f, out, lane, cls, f.known ? f.n_solve[cls] : cap, 3);
        }
    }
    // the problems with a handful of candidates, whole (coverage, labels, counts, DP), beside the others (launched after the
    // classes whose workgroups need half a CU's LDS each)
    if (f.tiny_on) out.push(ScoreOp{f.wave ? ScoreKind::Wave : ScoreKind::Tiny, 3, 0, 0, f.known ? f.n_tiny : cap, side ? 2 : -1});
}

}  // namespace fseg
