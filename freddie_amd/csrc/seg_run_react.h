// seg_run_react.h -- the status record of a run and what the host does about it, as plain C++ (no HIP): decide_reaction() maps
// a Status, the context's present facts and the kind of run that wrote it to the adaptations to apply and an outcome.
// react_to_status() (freddie_seg.hip) applies them; tools/upload_plan_host_check.cpp prints them without a GPU
// (tests/test_upload_plan_host.py holds what every status bit must give under every kind of run).
#pragma once
#include "seg_upload_plan.h"

namespace fseg {

constexpr int kNMax = 60;              // largest DP problem handled by the LDS-resident scoring kernel
constexpr int kNHuge = 128;            // 60 < n <= 128 (max_problem_size up to ~115): the global-count-table kernels k_score_huge / k_dp_huge
                                       // (pair planes and the DP's tables in LDS)
constexpr int kNGiant = 1024;          // 128 < n <= 1024 (max_problem_size up to 1 000: what the CLI accepts): k_score_giant / k_dp_giant,
                                       // every per-pair table in global scratch -- slow, complete (the reference's own optimize() is
                                       // O(n^3 R) Python there: nobody runs it for long)

// error bits of Status::err
enum : unsigned {
    kErrExonInterval = 1u,     // an exon is not inside one tint interval (py/freddie_segment.py:668)
    kErrBreakAssert = 2u,      // break_large_problems: assert max_c_idx_y_v > 0 / index out of range (:640-643)
    kErrProblemTooLarge = 4u,  // a DP problem has more than kNGiant candidates
    kErrOverflowPairs = 8u,
    kErrOverflowTri = 16u,
    kErrOverflowWork = 32u,
    kErrOverflowLabels = 64u,
    kErrOverflowProblems = 128u,
    kErrOverflowChunks = 256u,
    kErrOverflowCov = 512u,
    kErrOverflowNm = 1024u,
    kErrWideMissed = 16384u,   // internal: a problem keeps more reads than k_prob_range counted for it (the 8-bit instance met it)
    kErrWaveStage = 8192u,     // a wave kernel (k_wave) met a read with more exons than its LDS stage holds: rerun without them
    kErrScanStall = 4096u,     // the look-back scan gave up waiting for a predecessor block: rerun with the three-pass scan
    kErrSyncTimeout = 32768u,  // a device-side waiter of the scoring stage (k_wait_word) gave up: the stage was skipped, rerun with events
    kErrNeedWideDp = 2048u,    // a problem sees >= 65536 reads: its DP needs the 32-bit count table    // a problem is larger than the LDS carve-up this launch was sized for
};

struct Status {
    unsigned err;
    unsigned pad;
    u64 n_vals;        // number of Y > 0 values (all partitions)
    u64 n_vchunks;     // 8192-element chunks of the threshold reduction
    u64 n_cand;
    u64 n_prob;
    u64 n_work;
    u64 pair_used;
    u64 tri_used;
    u64 n_rseg;
    u64 n_final;
    u64 label_bytes;
    u64 cov_used;      // elements of the coverage arena
    unsigned max_n;    // largest DP problem of this run
    unsigned max_ln;   // most reads any DP problem of this run examines (>= 65536: the DP needs 32-bit counts)
    u64 cls_work[4];   // work items per problem-size class (n <= 16, <= 32, <= kNMax, <= kNHuge)
    u64 cls_queue[3];  // dynamic work counters of the scoring kernels
    u64 dp_cls[3];     // DP problems with n <= kDpSmall / <= kNMax / larger
    u64 cov_queue;
    u64 solve_cls[3];  // problems solved whole by k_solve (n <= 16 / <= 32 / <= kNMax)
    u64 n_tiny;        // problems solved whole by k_tiny (their list follows the three solve lists)
    unsigned list_cur[8];   // k_prob_emit's cursors into the four solve lists: [2 * list] from the front (expensive problems), [2 * list + 1] from the back
    unsigned wide_cls[4];   // solve-list problems per size class that see more than kFuseLanes reads (16-bit counters); [3] unused
    unsigned wide_cur[4];   // k_prob_emit's cursors into the per-class lists of those problems (wide_items); [3]: into the list of all of them (wide_all)
    unsigned gate_wide;     // workgroups of the large class's 16-bit instance that have started ('h' in a plan: the 8-bit instance waits for them)
    unsigned gate;          // large-class workgroups that have started (k_gate holds the small classes back until they are placed)
                            // (a counter of the mid class's 2 000 workgroups, bumped by each as it started, cost that kernel 10 of
                            // its 62 us: these two count a few hundred)
    unsigned sync_abort;    // a device-side waiter timed out: the scoring kernels behind it end at once (their input may not exist yet)
    unsigned pad2;
    // (Round 6 tried a start counter for the mid class here -- a gate 'i' that holds the small class back until the mid class's first
    // workgroups are placed.  Beside sync_abort, which every workgroup of the stage reads, eight counters took the stage from 0.125 to
    // 0.151 ms; on 128-byte lines of their own they cost nothing, and the gate gained nothing: 0.120-0.127 ms.  Removed.)
};

// Which run wrote the record: the sized first run of a batch after its piece A (histogram .. problem scan) or B (problem list ..
// label plan), or a whole run (a replay, or the first run under FSEG_NO_SIZED).
enum class RunKind { SizedA, SizedB, Replay };
enum class Outcome { Done, Redo, Fail };
enum class FailKind { None, Input, SizedOverflow, TimeoutNoWaiters, };
enum { CAP_PROB, CAP_WORK, CAP_PAIR, CAP_TRI, CAP_LABEL, CAP_CHUNK, CAP_COV, CAP_COUNT };

// what the decision reads of the context
struct ReactFacts {
    bool have_huge = false, dp_wide_counts = false;
    bool run_events_only = false;       // the run had no device-side waiters (it is the rerun after a time-out)
    int nm_giant = 0;
    i64 cap[CAP_COUNT] = {};            // the arenas' capacities
};

struct Reaction {
    Outcome outcome = Outcome::Done;
    FailKind fail = FailKind::None;
    bool uses_attempt = true;           // a Redo counts against the caller's attempts
    // adaptations: what the context takes over before the outcome is acted on
    bool scan_fallback = false;         // the three-pass scan from now on (scan_single_max = 0, the forced stall off)
    bool wave_off = false;              // no wave kernels for this context; the list sizes no longer hold
    bool sync_timeout = false;          // note_sync_timeout(): the rerun forks and joins with events
    bool nm_big_max = false;            // the big-problem kernels' LDS carve-up at its largest
    bool have_huge = false, dp_wide_counts = false;     // the values from now on
    bool giant = false;                 // prepare_giant(max_n)
    bool adopt_counts = false;          // note_counts() and adapt_to(): the record's sizes are the batch's
    i64 cap[CAP_COUNT] = {};            // the capacities from now on (alloc_arenas is the caller's, where it goes on)
};

constexpr unsigned kErrInputSized = kErrExonInterval | kErrBreakAssert | kErrProblemTooLarge;     // the reference would have aborted
constexpr unsigned kErrInputAny = kErrInputSized | kErrWideMissed;                                 // what run_input_errors() reports
constexpr unsigned kErrOverflowGrown = kErrOverflowPairs | kErrOverflowTri | kErrOverflowWork | kErrOverflowLabels |
                                       kErrOverflowProblems | kErrOverflowChunks | kErrOverflowCov;
// (the label arena is sized after piece B: its bit is not an overflow there)
constexpr unsigned kErrOverflowSized = (kErrOverflowGrown & ~kErrOverflowLabels) | kErrOverflowNm | kErrNeedWideDp;

// What each kind of run does about what the record says.  Where the kinds differ, the difference is meant:
//
//                        SizedA                 SizedB                          Replay
//   scan stall           scan fallback, Redo    scan fallback, Redo             scan fallback, Redo (with everything else the record asks for)
//   arena overflow       (cannot: nothing       Fail: the capacities were       grow the arena, Redo
//    / Nm / wide DP       is written yet)       exact, an internal error
//   capacities           at least the counts    --                              a count above its capacity: grown by an eighth, Redo
//   time-out             --                     Redo with events, NOT an        Redo with events (one of the four attempts)
//                                               attempt; in a run without
//                                               waiters Fail (internal)         the same Fail
//   wave stage           --                     wave kernels off, Redo          wave kernels off, Redo
//   huge / giant / wide  taken from the record  --                              turned on where the record asks, Redo; never off
//    counts               (on AND off), Done                                     (the batch is the same)
//   input errors         Fail, no results       Fail, no results                reported when the run is otherwise Done: the sizes are
//                        (wide-missed: B only)                                  adopted and the run counts as completed
//   attempts             three, "the compaction scans stalled repeatedly"       four, "arena sizing did not converge"
//
// A sized piece reacts to ONE thing per record, in the order of the rows (a stall hides an overflow, a time-out a wave stage: the
// redone piece raises the other again); a replay applies everything the record asks for and goes again once.
inline Reaction decide_reaction(const Status &s, const ReactFacts &f, RunKind kind) {
    Reaction r;
    r.have_huge = f.have_huge; r.dp_wide_counts = f.dp_wide_counts;
    for (int k = 0; k < CAP_COUNT; ++k) r.cap[k] = f.cap[k];
    const i64 used[CAP_COUNT] = {(i64)s.n_prob, (i64)s.n_work, (i64)s.pair_used, (i64)s.tri_used, (i64)s.label_bytes, (i64)s.n_vchunks, (i64)s.cov_used};
    auto end = [&r](Outcome o, FailKind fk = FailKind::None) { r.outcome = o; r.fail = fk; return r; };
    if (kind != RunKind::Replay) {
        if (s.err & kErrScanStall) { r.scan_fallback = true; return end(Outcome::Redo); }
        if (kind == RunKind::SizedA) {
            if (s.err & kErrInputSized) return end(Outcome::Fail, FailKind::Input);
            for (int k : {CAP_PROB, CAP_WORK, CAP_PAIR, CAP_TRI, CAP_COV}) r.cap[k] = std::max(r.cap[k], used[k]);
            r.have_huge = s.dp_cls[2] > 0;
            r.giant = true;
            r.dp_wide_counts = (i64)s.max_ln >= 65536;
            r.adopt_counts = true;
            return end(Outcome::Done);
        }
        if (s.err & kErrOverflowSized) return end(Outcome::Fail, FailKind::SizedOverflow);
        // (what B's scoring kernels can raise besides: a result that is garbage fails HERE, not after the label stage; a wave kernel
        // that met a read it cannot stage turns the wave kernels off and the sized attempt starts over)
        if (s.err & kErrSyncTimeout) {                       // a device-side waiter gave up (the stage was skipped): once more, with events
            if (f.run_events_only) return end(Outcome::Fail, FailKind::TimeoutNoWaiters);
            r.sync_timeout = true; r.uses_attempt = false;
            return end(Outcome::Redo);
        }
        if (s.err & kErrWideMissed) return end(Outcome::Fail, FailKind::Input);
        if (s.err & kErrWaveStage) { r.wave_off = true; return end(Outcome::Redo); }
        if (s.err & kErrInputSized) return end(Outcome::Fail, FailKind::Input);
        return end(Outcome::Done);
    }
    if ((s.err & kErrSyncTimeout) && f.run_events_only) return end(Outcome::Fail, FailKind::TimeoutNoWaiters);
    bool redo = (s.err & kErrOverflowGrown) != 0;
    if (s.err & kErrOverflowNm) { redo = true; r.nm_big_max = true; }
    if (s.err & kErrWaveStage) { redo = true; r.wave_off = true; }              // k_tiny / k_solve fetch exons read by read
    if (s.err & kErrSyncTimeout) { redo = true; r.sync_timeout = true; }        // the stage was skipped: this run again, with events
    if ((i64)s.max_ln >= 65536 && !f.dp_wide_counts) { redo = true; r.dp_wide_counts = true; }
    if (s.err & kErrScanStall) { redo = true; r.scan_fallback = true; }
    if (s.dp_cls[2] > 0 && !f.have_huge) { redo = true; r.have_huge = true; }   // rerun with the huge-problem kernels
    if ((int)s.max_n > kNHuge && (int)s.max_n <= kNGiant && (int)s.max_n > f.nm_giant) { redo = true; r.giant = true; }   // ... and the giant ones, sized for this run's largest problem
    for (int k = 0; k < CAP_COUNT; ++k) if (used[k] > f.cap[k]) redo = true;
    if (!redo) {
        r.adopt_counts = true;
        return (s.err & kErrInputAny) ? end(Outcome::Fail, FailKind::Input) : end(Outcome::Done);
    }
    for (int k : {CAP_PROB, CAP_WORK, CAP_PAIR, CAP_TRI, CAP_LABEL, CAP_COV})   // (the chunk arena's capacity is an upper bound from the upload: never grown)
        if (used[k] > r.cap[k]) r.cap[k] = used[k] + used[k] / 8 + 64;
    return end(Outcome::Redo);
}

}  // namespace fseg
