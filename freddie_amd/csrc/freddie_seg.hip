// freddie_seg.hip -- the HOST side of libfreddie_seg.so, the gfx950 (MI355X) library of the canonical-segmentation path: contexts,
// slabs and arenas, the launch sequence of a run, the sized first run, uploads, results, and the C-ABI of include/freddie_seg.h.
// The launch sequence is enqueue_run: it builds a Run (what the call computes once: streams, geometry, the scoring stage's launch
// list, the fork / join state) and calls a function per segment of the pipeline -- seg_pre1, seg_pre2, seg_score, seg_post1,
// seg_post2 --, each a list of launches; a kernel family with several instances or callers has its argument list once, in a
// launch_* function.  This unit defines no kernel: they live in the stage families' translation units (seg_front / seg_problems /
// seg_score_arena / seg_score_fused + seg_solve16|32|60 / seg_tail / seg_upload .hip; shared definitions seg_common.h,
// declarations seg_kernels.h); freddie_amd/build.py compiles the units side by side.
//
// What each kernel computes is defined by the reference's py/freddie_segment.py (cited per
// kernel as file:line); how it computes it is specific to this implementation:
//   * a batch of independent partitions lives in HBM as flat CSR arrays (include/freddie_seg.h);
//   * every data-dependent size (candidates, DP problems, final positions, label bytes) is
//     produced and consumed on the device; the host only reads one small status record at the
//     end of a run and grows an arena + re-runs when a capacity was exceeded, so the steady
//     state has no host synchronisation inside the pipeline;
//   * the interval-scoring stage never materialises the reference's (N+1)xR uint32 coverage
//     matrix: per DP problem it derives, for 64 reads at a time, the window-local coverage
//     prefix of each read from its exon list, turns the n*(n-1)/2 pair tests into 1-bit planes
//     in LDS, and counts out(i,j,k) with AND + popcount into an LDS-resident table.
//
// No CPU fallback exists in this library: without a GPU fseg_create() fails.
#include "seg_kernels.h"
#include "seg_score_plan.h"

using namespace fseg;

namespace {

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// A DevBuf<T> is a VIEW of device memory that holds T: into one of the context's slabs (the buffers of a batch are carved out
// of three device allocations -- inputs (one host-to-device copy fills it), position-sized work arrays, data-dependent arenas --
// so a new batch costs no allocator call unless it is larger than every batch before it), or, as the base of an OwnDev<T>, of an
// allocation with a life of its own.  T is what the kernels take: the carve-up, the launches and every copy get their sizes from it
// (bytes(n)).  DevBuf<void> holds different types per batch or region: its sizes are bytes, its readers name the type (as<T>()).
template <typename T> struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;      // bytes
    static size_t bytes(size_t n) { return n * sizeof(T); }
};
template <> struct DevBuf<void> {
    void *p = nullptr;
    size_t cap = 0;
    static size_t bytes(size_t n) { return n; }
    template <typename U> U *as() const { return static_cast<U *>(p); }
};
template <typename T> size_t bytes_of(const DevBuf<T> &, size_t n) { return DevBuf<T>::bytes(n); }   // n elements of this buffer
// The owners: each frees what it holds when it goes, none can be copied.
struct NoCopy { NoCopy() = default; NoCopy(const NoCopy &) = delete; NoCopy &operator=(const NoCopy &) = delete; };
template <typename T> struct OwnDev : DevBuf<T>, NoCopy {   // a device allocation of its own (ensure() grows it)
    ~OwnDev() { if (this->p) (void)hipFree(this->p); }
    hipError_t alloc(size_t bytes) { this->cap = bytes; return hipMalloc(&this->p, bytes); }   // exactly these bytes
};
struct Slab : OwnDev<void> {};                        // ... that buffers are carved out of (reserve() grows it)
template <typename T> struct Pinned : NoCopy {        // pinned host memory (reserve_host() grows it; alloc(): exactly one T)
    T *p = nullptr;
    size_t cap = 0;
    ~Pinned() { if (p) (void)hipHostFree(p); }
    hipError_t alloc() { cap = sizeof(T); return hipHostMalloc(&p, sizeof(T), hipHostMallocDefault); }
    T *operator->() const { return p; }
    T &operator*() const { return *p; }
};
// offsets of consecutive 256-byte-aligned buffers inside a slab: add() them all (n elements each, plus padding bytes where a
// kernel reads past the end), reserve the slab, then bind()
struct Carve {
    struct Item { void *buf; void (*set)(void *buf, char *p, size_t cap); size_t off, bytes; };
    std::vector<Item> items;
    size_t total = 0;
    template <typename T> void add(DevBuf<T> &b, size_t n, size_t pad_bytes = 0) {
        const size_t off = total, bytes = DevBuf<T>::bytes(n) + pad_bytes;
        items.push_back(Item{&b, [](void *buf, char *p, size_t cap) { auto *d = static_cast<DevBuf<T> *>(buf); d->p = static_cast<T *>(static_cast<void *>(p)); d->cap = cap; }, off, bytes});
        total = (off + bytes + 255) & ~(size_t)255;
    }
    void bind(void *base) const { for (const Item &it : items) it.set(it.buf, static_cast<char *>(base) + it.off, it.bytes); }
};
// where a buffer carved out of the allocation at dev_base lies in the host image of that allocation
template <typename T> T *mirror_of(char *host_base, const void *dev_base, const DevBuf<T> &d) {
    return static_cast<T *>(static_cast<void *>(host_base + (reinterpret_cast<const char *>(d.p) - static_cast<const char *>(dev_base))));
}

enum Stage { ST_HIST, ST_SMOOTH, ST_THRESHOLD, ST_CANDIDATES, ST_FIX, ST_SCORE_PREP, ST_SCORE, ST_DP, ST_REFINE, ST_FINAL, ST_LABEL, ST_COUNT,
             ST_GRAPH_PRE = ST_COUNT, ST_GRAPH_POST, ST_REPORTED };
// Plain launches (the first run of a batch, or FSEG_NO_GRAPH=1): every stage is bracketed by its own pair of events.
// Graph replay with profiling: graph(before scoring) | events around plain launches of the scoring kernel |
// graph(after); the two graphs are reported as graph_pre / graph_post.
const char *kStageNames[ST_REPORTED] = {"histogram", "smooth", "threshold", "candidates", "fix_split", "scoring_prep",
                                        "interval_scoring", "dp", "refine", "final_positions", "labels", "graph_pre",
                                        "graph_post"};

// segments of one run (bit mask of enqueue_run)
enum : unsigned {
    SEG_PRE1 = 1u,     // status reset, histogram .. problem ranges and the problem scan: every arena size is known after it
    SEG_PRE2 = 2u,     // problem list, pair thresholds, window coverage
    SEG_SCORE = 4u,    // the interval-scoring kernels
    SEG_POST1 = 8u,    // DP, refinement, final positions, label columns: the label arena's size is known after it
    SEG_POST2 = 16u,   // label arena fill + per-read labels
    SEG_STATUS = 32u,  // status record to the host
    SEG_ALL = 63u,
};

}  // namespace

hipError_t fseg_sort_pairs(void *tmp, size_t *tmp_bytes, const unsigned long long *keys_in, unsigned long long *keys_out,
                           const int *vals_in, int *vals_out, size_t n, unsigned end_bit, hipStream_t stream);   // freddie_seg_sort.hip

// The host values that shape what enqueue_run launches and that the context changes between two runs of one batch: a captured
// graph has them baked in, so it is valid for exactly the shape it was captured under (run_impl compares `shape` with the copy
// kept beside the graph and recaptures when they differ; nobody drops a graph because one of these changed).  What else a
// capture bakes in -- slab and arena pointers, capacities, parameters -- changes only where a resource's life ends, and those
// places drop the graph themselves (alloc_arenas, fseg_upload, fseg_set_params).  Each member names its reader in Run / seg_*.
// Compared as bytes: no padding (the static_assert), so the members are ordered by size and the tail is filled by hand.
struct LaunchShape {
    // what the lists of the resident batch hold (read from the status record; exact once the batch has run or been sized):
    // launches over an empty list are skipped (score_facts)
    i64 n_solve[3] = {0, 0, 0}, n_cls_work[4] = {0, 0, 0, 0}, n_arena_prob = 0, n_tiny = 0;
    i64 n_wide[3] = {0, 0, 0};  // of n_solve: problems that need the 16-bit-counter instances
    i64 scan_single_max = 512;  // scan blocks up to which the compactions use the single-pass look-back scan (FSEG_SCAN_SINGLE_MAX; Run::scan_single)
    const void *d_labels = nullptr, *d_packed = nullptr;    // the label arenas' allocations as of this run (launch_dp, seg_post2)
    int nm_big = kNMax;         // LDS carve-up of the big-problem kernels: largest problem of the batch, rounded up (nm_of)
    int nm_giant = 0;           // a problem with more than kNHuge candidates: its size (rounded up: the LDS carve-up and scratch piece of the giant kernels); 0: none
    bool counts_known = false;  // the list sizes above are this batch's (score_facts)
    bool small_batch = false;   // one stream, one launch per stage over all classes (would_fork, score_facts)
    bool tiny_on = false;       // many problems (> tiny_from): problems with <= kTiny candidates go to k_tiny (Run::split)
    bool fuse_on = true;        // this batch's problems go to k_solve: decided per batch -- when its widest problem sees at most
                                // kFuseLanes reads, i.e. all of them qualify (measured: a batch of 500-read partitions gains 8 %, while
                                // batches whose problems straddle the limit run both paths side by side and lose up to 8 %)
    bool wide_solve = true;     // some problem of the batch sees more than kFuseLanes reads: the 16-bit-counter instances of k_solve run too (score_facts)
    bool prob_self_scan = false; // k_prob_emit adds up the candidate blocks itself (few candidates; Run::prob_bs)
    bool have_huge = false;     // the batch has a problem with more than kNMax candidates: launch the huge kernels (seg_score, seg_post1)
    bool dp_wide_counts = false; // some problem sees >= 65536 reads: DP stages 32-bit counts (seg_post1)
    bool use_wave = true;       // FSEG_NO_WAVE=1, or a wave kernel met a read it cannot stage: k_tiny / k_solve<16> instead of the wave kernels (wave_on)
    bool force_scan_stall = false;   // FSEG_FORCE_SCAN_STALL=1 (tests): the first look-back run reports a stall (seg_pre1)
    bool profiling = false;     // fseg_set_profiling: the replay is two graphs around a bracketed scoring stage (run_impl), ...
    bool profile_all = true;    // ... false (mode 2): only the interval-scoring stage is bracketed by events (Run::begin), ...
    bool profile_plain = false; // ... mode 3: every stage bracketed on replays too, plain launches instead of the graph (run_impl)
    char fill[3] = {0, 0, 0};
    bool operator==(const LaunchShape &o) const { return memcmp(this, &o, sizeof o) == 0; }
};
static_assert(std::has_unique_object_representations_v<LaunchShape>, "LaunchShape is compared as bytes: no padding");

struct fseg_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    bool have_params = false, have_batch = false, ran = false, pending = false;
    bool fetched = false;        // the results of the last run are in the pinned result buffers
    fseg_params P{};
    std::vector<double> w_main, w_refine, h_table;
    BatchFacts batch;          // the resident batch's facts, assigned whole from the upload's plan (seg_upload_plan.h)
    int thr_part = -1;         // FSEG_THR_PART=0 / 1: the threshold per partition by one workgroup (k_thr_part) never / whenever possible; -1: batches of many partitions
    int hist16 = -1;           // FSEG_HIST16=0 / 1: S1 with 32-bit LDS counters always / with packed 16-bit ones wherever no count can overflow; -1: the same as 1
    i64 label_grid = 0;        // FSEG_LABEL_GRID=<n> (tests): the label launch takes at most n workgroups, so that one walks several units; 0: 65 536
    int yraw16 = -1;           // FSEG_YRAW16=0 / 1: the histogram in device memory int32 always / uint16 wherever S1 runs packed; -1: the same as 1
    int iv_cand = -1;          // FSEG_IV_CAND=0 / 1: S4 and S6 by intervals (k_fix, k_segments) always / by candidates (k_fix_cand, k_segments_cand) wherever iv_threads is 64; -1: from kIvCandFrom intervals on
    std::vector<i64> part_iv_off, part_rep_off;
    // The three slabs and the buffers that live outside them.  Every DevBuf<T> below is a view into a slab, every OwnDev<T> /
    // Slab / Pinned<T> an owner that frees itself when the context goes (~fseg_ctx has the order).  Untyped (DevBuf<void> /
    // OwnDev<void>, read through as<T>()) are the buffers whose element is not one type: d_y_raw (int32 or uint16 per batch),
    // d_labels (bytes, cleared and packed as uint4), d_sort_tmp and d_giant (scratch that a sort / a kernel carves up itself),
    // and the annotate arenas d_an_in / d_an_work / d_an_out (carved into typed local views per call).
    Slab slab_in, slab_pos, slab_arena;
    Pinned<char> h_stage;        // pinned image of the input slab's uploaded part
    Pinned<char> h_res;          // pinned results: final offsets | final positions | label offsets | labels
    size_t res_off[4] = {0, 0, 0, 0};
    std::vector<i64> res_pfo;    // part_final_off gathered from the per-interval offsets
    OwnDev<void> d_labels;       // label arena (sized after the final positions are known)
    OwnDev<unsigned> d_packed;   // the same at two bits per label, for the trip to the host
    int fetched_packed = -1;     // what the pinned result buffer holds: -1 nothing, 0 label bytes, 1 packed labels
    // Round 5: the labels are WRITTEN at two bits each (k_label_reads ORs the codes of a rep's non-'0' labels into d_packed, a word
    // at a time) whenever no column's default can be '2' (threshold_rate < 1: a read without coverage is never ambiguous) -- the
    // 75 MB byte arena of a 250 k-read batch is then neither filled (15 us) nor packed (25 us); fseg_results / fseg_download unpack
    // it on demand.  FSEG_LABEL_BYTES=1 keeps the byte arena as the primary form (and threshold_rate = 1 always does).
    // "No column's default can be '2'" is a property of the TABLE, not of the rate: smooth_threshold() rounds to two decimals, so a rate
    // in about (0.99972, 1) has a last entry of 1.0 (0.9999: segments of exactly 107 positions have h = 1, l = 0, lo = -1 and every
    // read is '2' there -- golden e_tau9999_len107).  label_has2 is computed from the table by fseg_set_params.
    bool label_packed_ok = true;
    bool label_has2 = false;         // some segment length has h >= 1 (lo < 0): a read without coverage is '2' there -> byte arena
    bool run_label_packed = false;   // the resident run's labels live in d_packed
    bool labels_unpacked = false;    // ... and d_labels holds their byte form (made on demand)
    OwnDev<void> d_sort_tmp;
    // device buffers: inputs (slab_in, uploaded)
    DevBuf<i64> d_part_iv_off, d_part_rep_off, d_part_lane_off, d_pos_off, d_rep_exon_off, d_hc_p0, d_rb_sum, d_rb_base;
    DevBuf<int> d_iv_start, d_iv_end, d_iv_part, d_rep_weight, d_ex_ts, d_ex_te, d_iv_tile0, d_blk_iv0, d_rb_part, d_rb_r0, d_rb_max, d_rb_cmax,
        d_hc_part, d_hc_n, d_hc_glo, d_hc_ghi;
    DevBuf<TileDesc> d_tile_desc;
    // slab_in, derived on the device by the upload
    DevBuf<longlong2> d_lane_ex;
    DevBuf<int> d_lane_start, d_lane_pmax, d_val_a, d_val_b, d_rep_last;
    DevBuf<i64> d_hc_llo, d_hc_lhi, d_rb_esum, d_rb_ebase;
    DevBuf<u64> d_key_a, d_key_b;
    DevBuf<int2> d_lane_lx, d_lex;      // the exons again as one (ts, te) stream in lane order, and every lane's range in it
    OwnDev<double> d_w_main, d_w_refine, d_h_table;        // parameter tables (own allocations)
    OwnDev<int2> d_thr_tab;
    // device buffers: position-sized (slab_pos)
    DevBuf<unsigned> d_bits;     // the three flag masks (Y > 0, candidate, final position), a bit per position each, cleared per run
    DevBuf<void> d_y_raw;        // S1's histogram: int32, or uint16 where the batch's counters are (yraw_narrow)
    DevBuf<double> d_y, d_v, d_g, d_csum, d_mean, d_thr;
    DevBuf<u64> d_scan_state;
    DevBuf<int> d_bsum, d_gsum, d_bsum_side, d_pk, d_part_has2;
    DevBuf<unsigned char> d_pf, d_kp;
    DevBuf<i64> d_voff, d_chunk_off, d_label_off;
    // candidate-sized (slab_pos)
    DevBuf<i64> d_cand_off, d_final_off, d_prob_bs;
    DevBuf<int> d_cand_y, d_final_y, d_final_pos, d_final_iv, d_blk_pre, d_tile_tot, d_seg_iv, d_seg_prev, d_rseg_c, d_cand_pn, d_cand_ll, d_cand_ln;
    DevBuf<int> d_tile_defer;   // per smoothing tile: start of the plateau that reaches the tile's end (-1: none)
    DevBuf<unsigned char> d_fixed0, d_added, d_fixed, d_chosen, d_col_zero, d_cand_wide;
    DevBuf<int2> d_col_thr;
    // problems / arenas (slab_arena)
    DevBuf<int> d_prob_iv, d_prob_start, d_prob_n, d_prob_flags, d_prob_chain, d_prob_lane_lo, d_prob_lane_n, d_dp_items, d_solve_items;
    DevBuf<i64> d_prob_pair_off, d_prob_tri_off, d_prob_cov_off;
    DevBuf<ProbDesc> d_solve_desc, d_prob_desc;
    DevBuf<int2> d_work_pc, d_pair_thr;
    DevBuf<int4> d_cls_items;
    DevBuf<unsigned char> d_work_active;
    DevBuf<unsigned> d_amb, d_out, d_cov;
    // hand-over arena between k_solve<.., SPLIT> and k_dpw (dpx_slot_bytes per problem of the three solve lists), laid out by
    // alloc_arenas() for the counts it knew: a launch takes the split path only for a list that fits what was laid out
    DevBuf<int> d_wide_items;    // per solve list: the list positions of the problems that see more than kFuseLanes reads (k_prob_emit)
    DevBuf<int> d_wide_all;      // ... of the three lists together (positions from the first list's start)
    DevBuf<unsigned char> d_dpx;
    i64 dpx_base[3] = {0, 0, 0}, dpx_stride[3] = {0, 0, 0}, dpx_n[3] = {0, 0, 0};
    int dpx_nm = 0, dpx_cnt[3] = {1, 1, 1};
    static constexpr i64 kWideOneMax = 256;   // plan 'W' takes a batch's wide problems in one launch when there are at most this many
    int split_dp = 7;           // FSEG_SPLIT_DP: bit 0 / 1 / 2 = the small / mid / large class hands its DPs to k_dpw (0: the DP stays the tail of k_solve's workgroups);
                                // bit 3 = the large class's k_dpw by one wave a problem (as the other classes') instead of eight
    i64 prob_cap = 0, work_cap = 0, pair_cap = 0, tri_cap = 0, label_cap = 0, chunk_cap = 0, cov_cap = 0;
    OwnDev<Status> d_status; OwnDev<PrepStatus> d_prep; OwnDev<unsigned long long> d_tacc;
    OwnDev<SyncWords> d_sync;    // the scoring stage's device-side fork / join (k_wait_word)
    unsigned sync_gen = 0;       // generation of the last stage enqueued with device-side waiters
    // What a waiter waits at most, in ticks of the 100 MHz clock, per 2^18 reads of the batch: 10 ms, at most 20 (FSEG_SYNC_TICKS; tests
    // force a time-out with 1).  Round 5's 20 ms DID run out, four times in one 8-context trace -- for two reasons, both removed in
    // round 6: a later context's side stream could share its own main stream's hardware queue (probe_side_queues), and two contexts that
    // started together could both fork (claim_device).  What is left is honest waiting: the fork waiters sleep through k_fix ..
    // k_prob_emit (median 49-68 us), the join waiter through what the side chains need beyond the main stream's -- plus whatever is in
    // front of the owner's kernels in its hardware queue: other contexts' kernels (168 and 235 us in two traced 8-context runs) or a
    // large copy to pageable memory (40 MB of a test's taps hold a queue for milliseconds: one time-out at 2 ms in 1 600 forked runs of
    // tests/test_gpu_contexts_stress.py; 200 us, the figure first tried, lost four to six waits per bench run).  A time-out costs the
    // limit AND a rerun of the batch, and with the two causes above gone a waiter only ever waits for work that completes: the limit
    // is the exit every launch must have, not a schedule.
    unsigned sync_ticks = 1000000u;
    unsigned sync_timeouts = 0;  // runs of this context that a waiter gave up on (each was redone with events); FSEG_TAP_SYNC[6]
    unsigned forked_runs = 0;    // runs of this context that owned the device (side streams in use); FSEG_TAP_SYNC[7]
    bool run_events_only = false;   // this run: no device-side waiters (it is the rerun after a timeout)
    bool dev_sync = true;        // FSEG_DEV_SYNC=0: the stage's side streams are forked and joined with events only (also after a waiter timed out)
    Pinned<Status> h_status; Pinned<PrepStatus> h_prep;
    bool prep_checked = false;   // the upload's device-side validation has been read back
    bool counted_in_flight = false, counted_live = false;
    // Which side streams may carry a device-side waiter: those whose hardware queue is NOT the main stream's (probe_side_queues).
    // The runtime multiplexes a process's streams onto four hardware queues as they are created: the first context of a device makes
    // its four streams back to back (queues 1 2 3 4: the third side stream shares the main stream's), a later context makes its side
    // streams when it first forks and they land wherever the count of streams then points -- round 5's 8-context trace had four
    // k_wait_word of 20 ms during which NOTHING else ran on the GPU: a waiter in front of its own main stream.
    bool side_probed = false;
    bool side_ok[3] = {false, false, false};
    unsigned probe_gen = 0;
    bool owns_device = false;    // this context holds the device's owner word: the only one that may fork over side streams (claim_device)
    int hsa_agent = -1;         // index into the HSA agent table (-1: not looked up yet, -2: unavailable)
    hsa_signal_t hsa_sig = {0};
    int hsa_cpu = 0;            // index of the CPU agent that owns the pinned result buffer ...
    const void *hsa_dst_base = nullptr;   // ... as asked for this allocation of it
    LaunchShape shape;           // what a captured graph was launched under (above)
    OwnDev<void> d_giant;        // the giant kernels' scratch: kGiantWgs pieces of giant_scratch_bytes(shape.nm_giant) (own allocation)
    bool use_graph = true;      // replay the launch sequence as hipGraphs from the second run of a batch on (FSEG_NO_GRAPH=1 disables)
    // ... when the run keeps to ONE stream (other contexts' batches in flight, small batches, FSEG_NO_FORK=1).  A run that
    // forks is replayed as plain launches: launching a graph with cross-stream edges costs the host 0.5-0.6 ms (ROCm 7.2,
    // the 250 k-read batch: 0.51 ms against 0.17 ms for the ~60 plain launches and 0.03 ms for the one-stream graph), more than
    // the GPU needs for the stages before the scoring stage -- the side streams' packets arrive late and the replay takes
    // 1.13 ms instead of 0.71 (profiles/r04_replay_modes.txt; the forked graph was a switch, FSEG_GRAPH_FORK, until round 6).
    bool run_plain = false;     // this run: plain launches (set by fseg_run)
    bool run_linear = false;    // this run: one stream whatever else holds (a graph is being captured)
    bool use_sized = true;      // the first run of a batch stops twice to size its arenas exactly (FSEG_NO_SIZED=1: guess, and re-run on overflow)
    static constexpr i64 kProbSelfMax = 4 * kProbBlock;   // candidates up to which it does
    hipGraph_t graph[2] = {nullptr, nullptr};            // [0] whole pipeline, or before / after scoring when profiling
    hipGraphExec_t graph_exec[2] = {nullptr, nullptr};
    int n_graphs = 0;
    LaunchShape graph_shape;     // the shape the graphs were captured under: run_impl replays them only while `shape` equals it
    unsigned graph_captures = 0; // captures this context has made (one per shape a replay met); FSEG_TAP_SYNC[9]
    bool last_sized = false;     // the pending run was launched stage by stage (per-stage events valid)
    hipEvent_t ev_b[ST_COUNT] = {}, ev_e[ST_COUNT] = {};
    hipEvent_t ev_g[4] = {};
    float stage_ms[ST_REPORTED] = {};
    // Independent kernels of one run (threshold | candidates, the scoring size classes, the DP classes) go to side
    // streams (pair thresholds | coverage was tried too: the branch cost more than the overlap gave) between a fork and a join, so a captured run becomes a graph with parallel
    // branches (FSEG_NO_FORK=1 keeps everything on the one stream).
    // (four streams in all: the runtime multiplexes a process's streams onto four hardware queues, and two streams that
    // share one run one after the other -- with seven streams the threshold and candidate chains stopped overlapping)
    static constexpr int kSide = 3, kForkEvents = 32;
    hipStream_t side[kSide] = {};
    hipEvent_t fj[kForkEvents] = {};
    bool use_fork = true;
    bool force_key64 = false;
    bool wide_by_seen = false;  // FSEG_WIDE_BY_SEEN=1 (tests)
    char score_plan[kScorePlanChars + 1] = "gM|W|hB|gST";   // FSEG_SCORE_PLAN (see seg_score_plan.h; anything that does not name each class once = one stream)
    bool use_fuse = true;       // FSEG_NO_FUSE=1: no problem goes to k_solve (everything that is not tiny takes the arena path)
    // Reads the widest problem of a batch may see for the batch's problems to be solved whole (k_solve / k_wave) instead of going
    // through the arena path; FSEG_FUSE_LANES=1023 admits batches of 1 000-read partitions (their widest problems see ~300 reads:
    // the 16-bit-counter instances of k_solve take those).  Measured on 250 x 1 000-read batches (config3 / config5): one batch
    // alone on the GPU is quicker solved whole (0.82 / 0.76 against 0.85 / 0.82 ms per replayed batch), eight contexts taking
    // turns are not (config3: 249 against 301 M reads/s; config5: equal) -- the few wide problems are long, thin launches -- so
    // the default keeps such batches on the arena path.
    int fuse_lanes = kFuseLanesDefault;
    i64 tiny_from = 256;        // problems above which k_tiny is used (FSEG_TINY_FROM; tests force 0)
    bool trace = false;         // FSEG_TRACE=1: phase timers of upload / run on stderr
    bool force_global_sort = false;   // FSEG_GLOBAL_SORT=1 (tests): the batch-wide radix sort whatever the partition sizes
    // FSEG_TAP_PATHS (include/freddie_seg.h has the words): what the last enqueue of each stage launched.  A stage's words are reset
    // where the stage's segment of enqueue_run begins (the scoring stage's: kScoreCensus); the masks and counts are written in the branches that launch, so they say what ran, not
    // what the switches asked for (the six decisions of the batch -- small_batch, tiny_on, wave_on, fuse_on, known, plan -- are the
    // values those branches test, copied where the stage begins); a replayed graph keeps the words of its capture.
    enum { PATH_SMALL_BATCH, PATH_TINY_ON, PATH_WAVE_ON, PATH_FUSE_ON, PATH_KEY32, PATH_THR_PART, PATH_LABEL_PACKED, PATH_N_SOLVE,
           PATH_N_WIDE = PATH_N_SOLVE + 3, PATH_N_TINY = PATH_N_WIDE + 3, PATH_N_WORK, PATH_DPW, PATH_WIDE16, PATH_KNOWN, PATH_SOLVE8,
           PATH_TINY_KERNEL, PATH_SCORE, PATH_ARENA_DP, PATH_PLAN, PATH_N_ARENA_PROB, PATH_N_SCORE, PATH_HIST16 = PATH_N_SCORE + 3, PATH_IV_THREADS,
           PATH_SMOOTH_R, PATH_YRAW16, PATH_LANE_SORT, PATH_IV_CAND, PATH_WORDS };
    int paths[PATH_WORDS] = {};
    // fseg_annotate: the uploaded reads (one allocation, mirrored by a pinned image), per-read work arrays, the emitted lists, and
    // the pinned buffers fseg_annotation() points into (own allocations: nothing of a run or of fseg_results* touches them)
    OwnDev<void> d_an_in, d_an_work, d_an_out;
    Pinned<char> h_an_in, h_an;
    bool have_annot = false;
    fseg_annot annot{};
    ~fseg_ctx();                // streams drained, graphs, HSA signal, events, streams -- then the owners above free themselves, as members
};

namespace {

int fail(fseg_ctx *c, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    // A failed HIP call leaves its code as the calling thread's "last error": consumed here, or the next -- successful --
    // upload or run on this host thread would trip over it at its hipGetLastError() check.
    if (code == FSEG_ERR_HIP) (void)hipGetLastError();
    return code;
}
thread_local std::string g_create_error;      // fseg_create has no context to put its message in: the calling thread's own

#define HIP_TRY(c, expr)                                                                         \
    do {                                                                                         \
        hipError_t e__ = (expr);                                                                 \
        if (e__ != hipSuccess) return fail((c), FSEG_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e__)); \
    } while (0)
#define TRY(expr) do { int rc__ = (expr); if (rc__) return rc__; } while (0)

// Contexts of one device that have a batch in flight (uploaded or running, results not yet complete).  A context forks its
// run over side streams only when it is alone on the device: with several contexts taking turns (the CLI, the benchmark's
// timed steps) the other contexts' kernels already fill what one stream leaves idle, and the extra streams only crowd the
// hardware queues (three contexts: 1.44 -> 1.28 ms per 250 k-read batch without them).
// Forking (and with it the device-side waiters of the scoring stage) needs more than that count: two contexts that start together
// could both read "alone", and then each parks one-wave spinners on side streams that share hardware queues with the other's
// main stream -- a cycle that only the waiters' time limit broke (round 5's 8-context trace: four 20 ms k_wait_word).  So a run
// forks only after it has CLAIMED the device: one compare-and-swap on the device's owner word, taken by fseg_run when nobody
// else is in flight, given back when the run has completed (finish_run).  Losers, and whoever arrives while the word is held,
// keep to one stream.  With one forking context per device a waiter can only sit in front of kernels that do not feed it.
static std::atomic<int> g_in_flight[64];
static std::atomic<int> g_live[64];
static std::atomic<const fseg_ctx *> g_owner[64];
static void set_in_flight(fseg_ctx *c, bool on);
static bool others_in_flight(const fseg_ctx *c);
static bool would_fork(const fseg_ctx *c);
static void claim_device(fseg_ctx *c);
static void release_device(fseg_ctx *c);

struct Tick {
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    double ms() { auto n = std::chrono::steady_clock::now(); double d = std::chrono::duration<double, std::milli>(n - t).count(); t = n; return d; }
};

// own allocation (parameter tables, label arena, sort scratch): grows, never shrinks
template <typename T>
int ensure(fseg_ctx *c, OwnDev<T> &b, size_t bytes) {
    if (bytes <= b.cap && b.p) return FSEG_OK;
    if (b.p) HIP_TRY(c, hipFree(b.p));
    b.p = nullptr; b.cap = 0;
    size_t want = bytes < 256 ? 256 : bytes + bytes / 4;          // headroom: batches of a run are of similar, not equal, size
    HIP_TRY(c, hipMalloc(&b.p, want));
    b.cap = want;
    return FSEG_OK;
}
// keep: the slab's contents must survive growing it (device-to-device copy of the old allocation)
int reserve(fseg_ctx *c, Slab &s, size_t bytes, bool keep = false) {
    if (bytes <= s.cap && s.p) return FSEG_OK;
    const size_t want = bytes + bytes / 4 + 4096;
    void *np = nullptr;
    HIP_TRY(c, hipMalloc(&np, want));
    if (s.p) {
        if (keep) HIP_TRY(c, hipMemcpyAsync(np, s.p, s.cap, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipFree(s.p));
    }
    s.p = np; s.cap = want;
    return FSEG_OK;
}
int reserve_host(fseg_ctx *c, Pinned<char> &h, size_t bytes) {
    if (bytes <= h.cap && h.p) return FSEG_OK;
    if (h.p) HIP_TRY(c, hipHostFree(h.p));
    h.p = nullptr; h.cap = 0;
    const size_t want = bytes + bytes / 4 + 4096;
    HIP_TRY(c, hipHostMalloc(&h.p, want, hipHostMallocDefault));
    h.cap = want;
    return FSEG_OK;
}
template <typename T>
int upload_vec(fseg_ctx *c, OwnDev<T> &b, const T *src, size_t n) {
    int rc = ensure(c, b, bytes_of(b, n));
    if (rc) return rc;
    if (n) HIP_TRY(c, hipMemcpyAsync(b.p, src, bytes_of(b, n), hipMemcpyHostToDevice, c->stream));
    return FSEG_OK;
}
// where a buffer of the input slab lies in the slab's pinned staging image (its uploaded part only)
template <typename T> T *host_of(const fseg_ctx *c, const DevBuf<T> &d) { return mirror_of(c->h_stage.p, c->slab_in.p, d); }

// A blocking copy on the context's OWN stream.  (Never hipMemcpy: it runs on the legacy stream, which must not be touched while another
// thread of the process -- another context -- is capturing a graph: "operation would make the legacy stream depend on a capturing blocking
// stream".  Found by tests/test_gpu_contexts_stress.py in round 6: taps, and the side-stream probe of a context that forks for the first
// time while another replays on one stream.)
hipError_t copy_sync(fseg_ctx *c, void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t q = nullptr) {
    if (!q) q = c->stream;
    hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, q);
    if (e == hipSuccess) e = hipStreamSynchronize(q);
    return e;
}

int grid_for(i64 items, int per_block, int max_blocks) {
    i64 g = (items + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > max_blocks) g = max_blocks;
    return (int)g;
}


inline size_t dp_lds_for(int nm, int count_bytes) {
    return (size_t)(nm * (nm - 1) / 2) * (8 + 4 + 1) + (size_t)(nm * (nm - 1) * (nm - 2) / 6 + 4) * count_bytes + 16;
}
constexpr size_t kLdsPerWg = 160 * 1024;

void drop_graph(fseg_ctx *c) {
    for (int g = 0; g < 2; ++g) {
        if (c->graph_exec[g]) { (void)hipGraphExecDestroy(c->graph_exec[g]); c->graph_exec[g] = nullptr; }
        if (c->graph[g]) { (void)hipGraphDestroy(c->graph[g]); c->graph[g] = nullptr; }
    }
    c->n_graphs = 0;
}

// (re)bind the data-dependent arenas for the current capacities; the label arena is its own allocation because it is
// sized after everything else of a run has been written
// the label arena for label_cap labels: two bits each (d_packed) when this context's parameters allow it, else bytes (d_labels)
bool labels_packed(const fseg_ctx *c) { return c->label_packed_ok && c->have_params && !c->label_has2; }
int ensure_label_arena(fseg_ctx *c) {
    if (labels_packed(c)) return ensure(c, c->d_packed, bytes_of(c->d_packed, (size_t)((c->label_cap + 15) / 16)) + 16);
    return ensure(c, c->d_labels, (size_t)c->label_cap + 16);
}
int alloc_arenas(fseg_ctx *c) {
    drop_graph(c);
    Carve cv;
    const size_t n_prob = (size_t)c->prob_cap, nw = (size_t)c->work_cap;
    cv.add(c->d_prob_iv, n_prob); cv.add(c->d_prob_start, n_prob); cv.add(c->d_prob_n, n_prob); cv.add(c->d_prob_pair_off, n_prob); cv.add(c->d_prob_tri_off, n_prob);
    cv.add(c->d_prob_flags, n_prob); cv.add(c->d_prob_chain, n_prob); cv.add(c->d_dp_items, n_prob); cv.add(c->d_solve_items, n_prob);
    cv.add(c->d_wide_items, n_prob); cv.add(c->d_wide_all, n_prob); cv.add(c->d_solve_desc, n_prob);
    cv.add(c->d_prob_cov_off, n_prob); cv.add(c->d_prob_lane_lo, n_prob); cv.add(c->d_prob_lane_n, n_prob); cv.add(c->d_prob_desc, n_prob);
    cv.add(c->d_work_pc, nw); cv.add(c->d_cls_items, nw); cv.add(c->d_work_active, nw);
    cv.add(c->d_cov, (size_t)c->cov_cap);
    cv.add(c->d_pair_thr, (size_t)c->pair_cap); cv.add(c->d_amb, (size_t)c->pair_cap);
    cv.add(c->d_out, (size_t)c->tri_cap);
    {
        size_t bytes = 0;
        const int nms[3] = {kClsSmall, kClsMid, c->shape.nm_big};
        for (int q = 0; q < 3; ++q) {
            const bool on = ((c->split_dp >> q) & 1) && c->shape.counts_known && c->use_fuse && c->shape.fuse_on && c->shape.n_solve[q] > 0;
            c->dpx_cnt[q] = (c->shape.wide_solve && c->shape.n_wide[q] > 0) ? 2 : 1;
            c->dpx_stride[q] = (i64)dpx_slot_bytes(nms[q], c->dpx_cnt[q]);
            c->dpx_n[q] = on ? c->shape.n_solve[q] : 0;
            c->dpx_base[q] = (i64)bytes;
            bytes += (size_t)c->dpx_n[q] * (size_t)c->dpx_stride[q];
        }
        c->dpx_nm = c->shape.nm_big;
        cv.add(c->d_dpx, bytes);
    }
    TRY(reserve(c, c->slab_arena, cv.total));
    cv.bind(c->slab_arena.p);
    TRY(ensure_label_arena(c));
    return FSEG_OK;
}

// the wave kernels need the exon stream's pieces to fit their LDS stage (k_wave): a batch with a rep of more exons keeps
// k_tiny / k_solve for its small problems
bool wave_on(const fseg_ctx *c) { return c->shape.use_wave && c->batch.max_rep_exons <= kWaveRepExons; }
ProbSplit split_of(const fseg_ctx *c, bool tiny, bool fuse) {
    return ProbSplit{tiny ? kTiny : 0, (c->use_fuse && fuse) ? c->fuse_lanes : -1};
}

// The scoring stage's launches (seg_score walks the list of seg_score_plan.h): a function per kernel family, the family's
// argument list written once, and the dispatchers that map an op to the instance -- only instances the kernels' units instantiate
// (kInstances in seg_solve16 / 32 / 60 .hip, seg_score_fused.hip, seg_score_arena.hip).
static_assert(kScoreSide == fseg_ctx::kSide, "a plan's segments beyond the first take a side stream each");
#ifdef FSEG_SCORE_TIMING
#define FSEG_TARG , c->d_tacc.p
#else
#define FSEG_TARG
#endif
#ifndef FSEG_WG_SMALL
#define FSEG_WG_SMALL 4096
#endif
#ifndef FSEG_WG_MID
#define FSEG_WG_MID 2048
#endif
#ifndef FSEG_WG_TINY
#define FSEG_WG_TINY 4096
#endif
// the candidates a kernel of size class NM lays its LDS out for: the large class's follow the batch's largest problem
template <int NM> int nm_of(const fseg_ctx *c) { return NM == kNMax ? c->shape.nm_big : NM; }
// a 16-bit instance over one class of a sized batch walks the class's wide problems through wide_items, the one launch over
// every class's through wide_all
const int *wide_list(const fseg_ctx *c, const ScoreFacts &f, const ScoreOp &op) {
    return op.kind == ScoreKind::WideAll ? c->d_wide_all.p : (wide_n(f, op.cls, op.cnt_bytes) >= 0 ? c->d_wide_items.p : nullptr);
}
template <int NM>
void launch_score(fseg_ctx *c, hipStream_t q, const ScoreOp &op, const ProblemArrays &pr) {
    constexpr int max_wg = NM == kNMax ? 512 : (NM == kClsMid ? 1280 : 2048);
    const int work_grid = grid_for(c->work_cap, 1, 4096);
    hipLaunchKernelGGL(k_score<NM>, dim3(work_grid < max_wg ? work_grid : max_wg), dim3(ScoreCfg<NM>::kThreads),
                       score_lds_for(nm_of<NM>(c), NM + 1), q, c->d_status.p, op.cls, nm_of<NM>(c), pr, c->prob_cap, c->d_cls_items.p,
                       c->d_prob_desc.p, c->work_cap, c->d_cand_off.p, c->d_cand_y.p, c->d_work_active.p, c->d_cov.p,
                       c->cov_cap, c->d_pair_thr.p, c->pair_cap, c->d_out.p, c->tri_cap, c->d_amb.p FSEG_TARG);
}
// (an unsized batch: grid-stride workgroups up to the class's cap over prob_cap; sized: a workgroup per problem of the list)
template <int NM, typename CntT, typename V, bool SPLIT>
void launch_solve(fseg_ctx *c, hipStream_t q, const ScoreOp &op, const ScoreFacts &f, const ProblemArrays &pr) {
    constexpr int max_wg = NM == kNMax ? 512 : (NM == kClsMid ? FSEG_WG_MID : FSEG_WG_SMALL);
    hipLaunchKernelGGL((k_solve<NM, CntT, V, SPLIT>), dim3(grid_for(op.n, 1, f.known ? (1 << 20) : max_wg)), dim3(SolveCfg<NM>::kThreads),
                       solve_lds_for(nm_of<NM>(c), NM + 1, (int)sizeof(CntT)), q, c->d_status.p, op.cls, nm_of<NM>(c), list_lb(f, op.cls),
                       f.known ? op.n : (i64)-1, pr, c->d_solve_desc.p, c->prob_cap, c->d_cand_y.p, c->d_lane_lx.p, c->d_lex.p,
                       c->d_h_table.p, c->P.h_len, c->P.threshold_rate, c->d_thr_tab.p, c->P.min_read_support_outside, c->d_chosen.p,
                       SPLIT ? c->d_dpx.p + c->dpx_base[op.cls] : (unsigned char *)nullptr, SPLIT ? c->dpx_stride[op.cls] : (i64)0,
                       wide_list(c, f, op) FSEG_TARG);
}
template <int NM, typename CntT, typename V, int T>
void launch_dpw(fseg_ctx *c, hipStream_t q, const ScoreOp &op, const ScoreFacts &f, const ProblemArrays &pr) {
    c->paths[fseg_ctx::PATH_DPW] |= (1 << op.cls) | (T == 512 ? 8 : 0);
    hipLaunchKernelGGL((k_dpw<NM, CntT, V, T>), dim3(grid_for(op.n, 1, (int)kSplitGridCap)), dim3(T),
                       dpw_lds_for(nm_of<NM>(c), (int)sizeof(V), (int)sizeof(CntT)), q, c->d_status.p, nm_of<NM>(c), list_lb(f, op.cls), op.n, pr,
                       c->d_solve_desc.p, c->d_dpx.p + c->dpx_base[op.cls], c->dpx_stride[op.cls],
                       c->P.min_read_support_outside, c->d_chosen.p, wide_list(c, f, op) FSEG_TARG);
}
// one wave per problem on the exon stream: the list op.cls names (3: the tiny problems')
template <int NM, typename V>
void launch_wave(fseg_ctx *c, hipStream_t q, const ScoreOp &op, const ScoreFacts &f, const ProblemArrays &pr) {
    hipLaunchKernelGGL((k_wave<NM, V>), dim3(grid_for(op.n, 4, FSEG_WG_TINY)), dim3(256), 0, q, c->d_status.p,
                       c->d_solve_desc.p, c->prob_cap, op.cls, pr, c->d_cand_y.p, c->d_lane_lx.p,
                       c->d_lex.p, c->d_h_table.p, c->P.h_len, c->P.threshold_rate,
                       c->d_thr_tab.p, c->P.min_read_support_outside, c->d_chosen.p,
                       list_lb(f, op.cls), list_ln(f, op.cls) FSEG_TARG);
}
// A k_solve op's instance: the size class (one launch over every class is the large class's), the counter width, 32-bit DP keys
// when the batch allows them.  The split path is k_solve<.., int, SPLIT> (its rounds need no keys) then k_dpw (the DPs, keyed as
// the fused instance would be; `with_dpw` false: a diagnostic build leaves them out); eight waves a workgroup exist for the
// large class only.
template <int NM, typename CntT>
void launch_solve_as(fseg_ctx *c, hipStream_t q, const ScoreOp &op, const ScoreFacts &f, const ProblemArrays &pr, bool with_dpw) {
    if (op.kind != ScoreKind::SolveSplit) {
        if (f.key32) launch_solve<NM, CntT, int, false>(c, q, op, f, pr); else launch_solve<NM, CntT, i64, false>(c, q, op, f, pr);
        return;
    }
    launch_solve<NM, CntT, int, true>(c, q, op, f, pr);
    if (!with_dpw) return;
    if constexpr (NM == kNMax) if (op.dpw_threads == 512) {
        if (f.key32) launch_dpw<NM, CntT, int, 512>(c, q, op, f, pr); else launch_dpw<NM, CntT, i64, 512>(c, q, op, f, pr);
        return;
    }
    if (f.key32) launch_dpw<NM, CntT, int, 64>(c, q, op, f, pr); else launch_dpw<NM, CntT, i64, 64>(c, q, op, f, pr);
}
template <int NM>
void launch_class(fseg_ctx *c, hipStream_t q, const ScoreOp &op, const ScoreFacts &f, const ProblemArrays &pr, bool with_dpw) {
    if (op.kind == ScoreKind::Score) launch_score<NM>(c, q, op, pr);
    else if (op.cnt_bytes == 2) launch_solve_as<NM, unsigned short>(c, q, op, f, pr, with_dpw);
    else launch_solve_as<NM, unsigned char>(c, q, op, f, pr, with_dpw);
}
// k_score / k_solve ops
void launch_class_op(fseg_ctx *c, hipStream_t q, const ScoreOp &op, const ScoreFacts &f, const ProblemArrays &pr, bool with_dpw) {
    if (op.cls == 0) launch_class<kClsSmall>(c, q, op, f, pr, with_dpw);
    else if (op.cls == 1) launch_class<kClsMid>(c, q, op, f, pr, with_dpw);
    else launch_class<kNMax>(c, q, op, f, pr, with_dpw);
}

// the problem kernels' grid (k_prob_range, k_prob_scan1, k_prob_emit)
int prob_grid(const fseg_ctx *c) { return grid_for(c->batch.NPOS / 8 / kProbBlock + 1, 1, 1024); }
// what the scoring stage's decisions read (seg_score_plan.h), from the context
ScoreFacts score_facts(const fseg_ctx *c, bool forking) {
    ScoreFacts f;
    // list sizes known (the batch has been sized or has run): launches over an empty list are left out
    f.known = c->shape.counts_known; f.small_batch = c->shape.small_batch; f.any_arena = !f.known || c->shape.n_arena_prob > 0; f.fuse = c->use_fuse && c->shape.fuse_on;
    f.tiny_on = c->shape.tiny_on; f.wave = wave_on(c); f.forking = forking; f.wide_solve = c->shape.wide_solve;
    // 32-bit DP keys (dp_solve_push) when no sum of a chain can reach 2^24: at most 32 links times the reads of the largest partition
    f.key32 = c->batch.max_part_lanes < kKey32Reads && !c->force_key64;     // (FSEG_FORCE_KEY64=1: the 64-bit instances whatever the batch)
    for (int q = 0; q < 3; ++q) { f.n_solve[q] = c->shape.n_solve[q]; f.n_wide[q] = c->shape.n_wide[q]; f.dpx_n[q] = c->dpx_n[q]; f.dpx_cnt[q] = c->dpx_cnt[q]; }
    for (int q = 0; q < 4; ++q) f.n_cls_work[q] = c->shape.n_cls_work[q];
    f.n_tiny = c->shape.n_tiny; f.prob_cap = c->prob_cap; f.split_dp = c->split_dp;
    f.dpx_nm_fits = c->dpx_nm == c->shape.nm_big; f.dpx_arena = c->d_dpx.p != nullptr;
    f.split_grid_cap = kSplitGridCap; f.wide_one_max = fseg_ctx::kWideOneMax;
    return f;
}

// What one call of enqueue_run computes once and every segment of the call reads (the members' initialisers, in this order), the
// call's fork / join state, and what a segment leaves for a later one of the same call.  Built on the stack per call; the
// segments' functions (seg_pre1 .. seg_post2) take it.
struct Run {
    fseg_ctx *c;
    unsigned segs;              // the segments this call enqueues
    bool sized;                 // the first run of a batch, launched piecewise (see enqueue_run)
    hipStream_t s = c->stream;
    Status *st = c->d_status.p;
    // the flag masks: Y > 0 | candidate | final position, flag_words(NPOS) words each
    unsigned *flag_pos_bits = c->d_bits.p, *flag_cand_bits = flag_pos_bits + flag_words(c->batch.NPOS), *flag_final_bits = flag_cand_bits + flag_words(c->batch.NPOS);
    bool stage_events = c->shape.profiling && (sized || c->run_plain);   // the stages are bracketed by events (begin / end)
    // Small batches (one partition, few problems) are chains of launch-latency-sized kernels: branches only add
    // cross-stream dependencies there (measured: config2 +4 %), so they stay on the one stream.
    bool forking = would_fork(c) && !c->run_linear;
    // look-back state of the three compactions (values, candidates, final positions): scan_nb words each of d_scan_state
    i64 scan_nb = scan_blocks(c->batch.NPOS);
    int scan_grid = scan_nb > 0 ? (int)scan_nb : 1;       // exactly one workgroup per scan block (look-back)
    // single-pass look-back scan while the chain of blocks is short; block sums + one scanning workgroup beyond that
    bool scan_single = scan_nb <= c->shape.scan_single_max;
    int *bsum_side = scan_single ? nullptr : c->d_bsum_side.p;     // block sums of the scan that runs on a side stream (values)
    // the two position compactions: blocks of kPosBlock positions (a quarter of the words of look-back state, same layout).  The
    // look-back chain keeps its limit in POSITIONS (FSEG_SCAN_SINGLE_MAX blocks of kScanBlock, as it was measured): beyond it
    // block sums + group sums that the emitting workgroups add up themselves (k_pos_count), no scanning workgroup between
    int pos_grid = (int)std::max<i64>(pos_blocks(c->batch.NPOS), 1);     // exactly one workgroup per block
    int *bsum = scan_single ? nullptr : c->d_bsum.p;
    int *gsum = scan_single ? nullptr : c->d_gsum.p;
    i64 avg_len = c->batch.NPOS / (c->batch.K > 0 ? c->batch.K : 1);        // positions per interval
    int iv_threads = avg_len > 65536 ? 1024 : (avg_len > 16384 ? 256 : 64);    // the block of k_fix and k_segments
    // ... or both by candidates (k_fix_cand, k_segments_cand): batches of many short intervals, where a wave per interval walks many
    // of them with a few lanes at work (seg_common.h: kIvCandFrom; profiles/iv_cand.txt).  One decision for S4 and S6.
    bool iv_cand = iv_threads == 64 && (c->iv_cand == 1 || (c->iv_cand < 0 && c->batch.K >= kIvCandFrom));
    int iv_cand_grid = grid_for(c->batch.NPOS / 64 / kIvCandOwn + 1, 1, 4096);       // (the kernels stride over the runs st->n_cand makes)
    int pg = prob_grid(c);
    // few candidates: the emit kernel scans by itself, one launch instead of three (never in a sized run: there the
    // host reads the scan's totals before the emit kernel is launched)
    i64 *prob_bs = (c->shape.prob_self_scan && !sized) ? nullptr : c->d_prob_bs.p;
    ProblemArrays pr{c->d_prob_iv.p, c->d_prob_start.p, c->d_prob_n.p,
                     c->d_prob_pair_off.p, c->d_prob_tri_off.p, c->d_prob_flags.p,
                     c->d_prob_chain.p, c->d_prob_cov_off.p, c->d_prob_lane_lo.p,
                     c->d_prob_lane_n.p};
    ProbSplit split = split_of(c, c->shape.tiny_on, c->shape.fuse_on);
    // What the scoring stage of this enqueue launches -- which instance over which list on which stream, in which host order:
    // seg_score_plan.h has the rules and what was measured for them -- is decided HERE, the plan (FSEG_SCORE_PLAN) with it: with the
    // device-side fork (k_wait_word) a plan's side streams are forked in front of the stage's predecessors, so that the events'
    // latency (10-15 us each) is over when k_prob_emit ends.
    ScoreFacts facts = score_facts(c, forking);
    ScorePlan ps = parse_score_plan(facts, c->score_plan, segs & SEG_SCORE);
    ScoreOps ops;               // (filled in by the constructor when the call holds the scoring stage)
    // device-side fork / join (k_wait_word): plain launches only (never inside a capture), and only when this enqueue holds
    // k_prob_emit, whose last workgroup is what the side streams wait for; only on side streams whose hardware queue is not the
    // main stream's (side_ok, probed once: a waiter there would sit in front of the kernel it waits for)
    bool dev_sync = ps.on && c->dev_sync && !c->run_events_only && (segs & SEG_PRE2) && (sized || c->run_plain) && c->d_sync.p != nullptr;
    SyncWords *sw = c->d_sync.p;
    unsigned sync_gen = dev_sync ? ++c->sync_gen : 0;
    // (a context's first stages with waiters also load the stage's code objects and make the runtime allocate scratch for the side
    // streams' queues -- hundreds of microseconds, once: tools/waiter_probe.py)
    unsigned sync_ticks = (unsigned)std::min<i64>((i64)c->sync_ticks * std::max<i64>(1, c->batch.LANES >> 18), 2000000);
    i64 labels_n16 = (c->label_cap + 15) / 16;            // the arena is allocated in multiples of 16 bytes
    bool lab_packed = labels_packed(c);                   // (two-bit labels: the arena is cleared by a memset, nothing rides)
    // the label arena's '0' fill rides the big-problem DP launch as extra workgroups -- unless the run is being sized
    // (the arena's size is not known yet) or there is no DP launch
    // (not where the stages are bracketed by events: the fill is the labels stage's work, and a DP bracket that holds it says nothing about the DP)
    bool ride_fill = !sized && c->prob_cap > 0 && c->label_cap > 0 && facts.any_arena && !stage_events && !lab_packed;
    // What a segment leaves for a later one of the same call: SEG_PRE2 opens the scoring stage's bracket in front of the arena
    // path's coverage launches (they are interval scoring), so SEG_SCORE must not open it again.
    bool score_begun = false;
    int fj_next = 0;
    hipError_t fj_err = hipSuccess;

    Run(fseg_ctx *ctx, unsigned segs_, bool sized_) : c(ctx), segs(segs_), sized(sized_) { if (segs & SEG_SCORE) plan_score_ops(facts, ps, ops); }
    void begin(int i) const { if (stage_events && (c->shape.profile_all || i == ST_SCORE)) (void)hipEventRecord(c->ev_b[i], s); }
    void end(int i) const { if (stage_events && (c->shape.profile_all || i == ST_SCORE)) (void)hipEventRecord(c->ev_e[i], s); }
    // fork(k): side stream k continues from here; join(k): the main stream waits for it.  Every fork is joined before
    // enqueue_run returns, so a capture of the main stream ends with all branches merged.
    hipEvent_t fj_event() { hipEvent_t e = c->fj[fj_next % fseg_ctx::kForkEvents]; ++fj_next; return e; }
    hipStream_t fork(int k) {
        if (!forking) return s;
        hipEvent_t e = fj_event();
        hipError_t r = hipEventRecord(e, s);
        if (r == hipSuccess) r = hipStreamWaitEvent(c->side[k], e, 0);
        if (r != hipSuccess) fj_err = r;
        return c->side[k];
    }
    void join(int k) {
        if (!forking) return;
        hipEvent_t e = fj_event();
        hipError_t r = hipEventRecord(e, c->side[k]);
        if (r == hipSuccess) r = hipStreamWaitEvent(s, e, 0);
        if (r != hipSuccess) fj_err = r;
    }
    // segment k of the plan runs on a side stream behind a device-side waiter
    bool dev_side(int k) const { return dev_sync && k >= 1 && k < ps.n_seg && ps.used[k] && ps.side_of[k] >= 0 && ps.side_of[k] < fseg_ctx::kSide && c->side_ok[ps.side_of[k]]; }
    // The fork is EARLY (the event in front of k_fix: its latency hides behind the stage's predecessors), the waiters' launches come
    // LATE on the host -- behind k_prob_emit's --: a waiter then never spins on the device while the host has not yet enqueued the
    // kernel it waits for (a host thread that is descheduled, or held up in the runtime beside another context's large pageable copy,
    // between the two was one way to a time-out: tests/test_gpu_contexts_stress.py); on the device nothing moves -- the host is four
    // launches (~20 us) ahead of the event either way.
    void early_fork() {
        if (!dev_sync) return;
        for (int k = 1; k < ps.n_seg; ++k) if (dev_side(k)) (void)fork(ps.side_of[k]);
    }
    void launch_fork_waiters() const {
        if (!dev_sync) return;
        for (int k = 1; k < ps.n_seg; ++k) if (dev_side(k))
            hipLaunchKernelGGL(k_wait_word, dim3(1), dim3(64), 0, c->side[ps.side_of[k]], st, &sw->emit_gen, 1u, sync_gen, sync_ticks);
    }
};

// The launches of the other stages whose argument list is needed more than once (an instance per counter type, a second caller):
// the list written once, as the scoring stage's above.  A kernel with one launch site is launched where its stage's function has it.
// S1 (the chunks were laid out on upload for one counter width: one instance per launch)
template <int BITS, typename OUT>
void launch_hist(const Run &r) {
    fseg_ctx *c = r.c;
    hipLaunchKernelGGL((k_hist<BITS, OUT>), dim3(grid_for(c->batch.n_hist_chunks, 1, 16384)), dim3(512), 0, r.s, c->batch.n_hist_chunks,
                       c->d_hc_part.p, c->d_hc_p0.p, c->d_hc_n.p, c->d_hc_glo.p,
                       c->d_hc_ghi.p, c->d_hc_llo.p, c->d_hc_lhi.p, c->d_part_iv_off.p, c->d_iv_start.p, c->d_iv_end.p,
                       c->d_pos_off.p, c->d_part_lane_off.p, c->d_lane_lx.p,
                       c->d_lane_start.p, c->d_lane_pmax.p,
                       c->d_lex.p, c->P.ignore_ends, c->d_y_raw.as<OUT>(), r.st,
                       c->d_scan_state.p, r.scan_single ? r.scan_nb * 3 : 0);
}
// S2, radius RV (0: the loop) over the histogram as S1 left it
template <int RV, typename COUNT>
void launch_smooth(const Run &r) {
    fseg_ctx *c = r.c;
    hipLaunchKernelGGL((k_smooth<RV, COUNT>), dim3(grid_for(c->batch.n_tiles, 1, 16384)), dim3(kSmoothThreads), 0, r.s, c->batch.n_tiles, c->d_tile_desc.p,
                       c->d_y_raw.as<COUNT>(), c->d_w_main.p,
                       c->P.radius_main, c->d_y.p, r.flag_pos_bits,
                       r.flag_cand_bits, c->d_blk_pre.p, c->d_tile_tot.p, c->d_tile_defer.p);
}
template <int RV>
void launch_smooth_as(const Run &r) {
    if (r.c->batch.yraw_narrow) launch_smooth<RV, uint16_t>(r); else launch_smooth<RV, int>(r);
}
// A position compaction (`plane` 1: the candidates, 2: the final positions) on the main stream: the flagged positions' values,
// positions and intervals into the lists, every interval's offset into off[0 .. K]
void launch_positions(const Run &r, const unsigned *flags, int plane, u64 *total, i64 *off, int *out_y, int *out_pos, int *out_iv) {
    fseg_ctx *c = r.c;
    if (!r.scan_single)
        hipLaunchKernelGGL(k_pos_count, dim3(grid_for(pos_groups(c->batch.NPOS), 1, 4096)), dim3(kPosCountThreads), 0, r.s, flags, c->batch.NPOS, r.bsum, r.gsum);
    hipLaunchKernelGGL(k_scan_emit<kEmitPositions>, dim3(r.pos_grid), dim3(256), 0, r.s, flags, c->batch.NPOS,
                       r.bsum, r.gsum, c->d_scan_state.p + plane * r.scan_nb, total, off + c->batch.K, &r.st->err, (const double *)nullptr, (double *)nullptr, c->batch.K, c->d_pos_off.p,
                       c->d_iv_start.p, c->d_blk_iv0.p, out_y, out_pos,
                       off, 0, out_iv);
}
// The problem ranges under `split`, with the block sums of the problem scan (bs) or without (null), and the scan as launches of
// its own (blocks: k_prob_scan1 makes the block sums): S4, and the sized first run's rescan under another split
void launch_prob_range(fseg_ctx *c, ProbSplit split, i64 *bs) {
    hipLaunchKernelGGL(k_prob_range, dim3(prob_grid(c)), dim3(kRangeThreads), 0, c->stream, c->d_status.p, c->d_cand_pn.p,
                       c->d_seg_iv.p, c->d_cand_y.p, c->d_iv_part.p, c->d_iv_start.p,
                       c->d_part_lane_off.p, c->d_lane_start.p, c->d_lane_pmax.p,
                       c->d_cand_ll.p, c->d_cand_ln.p, c->d_cand_wide.p, c->d_lane_lx.p,
                       c->d_lex.p, c->wide_by_seen ? 1 : 0, split.fuse_lanes, bs, split);
}
void launch_prob_scan(fseg_ctx *c, ProbSplit split, i64 *bs, bool blocks) {
    if (blocks)
        hipLaunchKernelGGL(k_prob_scan1, dim3(prob_grid(c)), dim3(256), 0, c->stream, c->d_status.p, c->d_cand_pn.p, c->d_cand_ln.p, c->d_cand_wide.p, bs, split);
    hipLaunchKernelGGL(k_prob_scan2, dim3(1), dim3(256), 0, c->stream, c->d_status.p, bs);
}
// The arena path's DP: the list of `dp_class` (-1: every class in one launch) by dp_blocks workgroups, the problems of more than
// n_lo candidates.  The large class's launch carries the label arena, and fill_blocks more workgroups that fill it (Run::ride_fill).
template <int NM, int T, typename OUTT>
void launch_dp(const Run &r, hipStream_t q, int dp_class, int n_lo, int dp_blocks, int fill_blocks) {
    fseg_ctx *c = r.c;
    hipLaunchKernelGGL((k_dp<NM, T, OUTT>), dim3(dp_blocks + fill_blocks), dim3(T),
                       dp_lds_for(nm_of<NM>(c), (int)sizeof(OUTT)), q, r.st, dp_class, nm_of<NM>(c), c->d_dp_items.p, r.pr,
                       c->d_prob_desc.p, c->prob_cap, c->d_cand_off.p, c->d_cand_y.p, c->d_iv_part.p,
                       c->d_part_lane_off.p, c->d_out.p, c->tri_cap, c->d_amb.p,
                       c->d_pair_thr.p, c->pair_cap, c->P.min_read_support_outside,
                       c->d_chosen.p, n_lo, dp_blocks,
                       NM == kNMax ? c->d_labels.as<uint4>() : (uint4 *)nullptr, NM == kNMax ? r.labels_n16 : (i64)0 FSEG_TARG);
}
// the small DP class's list: a wave per problem of up to kDpWave candidates (q_small), and beside them (q_mid) ...
template <typename OUTT>
void launch_dp_waves(const Run &r, hipStream_t q_small, hipStream_t q_mid) {
    fseg_ctx *c = r.c;
    hipLaunchKernelGGL((k_dp_waves<OUTT>), dim3(grid_for(c->prob_cap, 4, 2048)), dim3(256),
                       dp_lds_for(kDpSmall, (int)sizeof(OUTT)) > 4 * dp_wave_bytes<OUTT>() ? dp_lds_for(kDpSmall, (int)sizeof(OUTT)) : 4 * dp_wave_bytes<OUTT>(),
                       q_small, r.st, c->d_dp_items.p, r.pr, c->d_prob_desc.p, c->prob_cap,
                       c->d_cand_y.p, c->d_out.p, c->tri_cap, c->d_amb.p,
                       c->d_pair_thr.p, c->pair_cap, c->P.min_read_support_outside, c->d_chosen.p, 0);
    // ... the problems of the list with 17 .. 32 candidates: one workgroup each, so that none waits behind another
    launch_dp<kDpSmall, 256, OUTT>(r, q_mid, 0, kDpWave, grid_for(c->prob_cap, 1, 8192), 0);
}
// S6 (the histogram as S1 left it: uint16 where it ran packed)
template <typename COUNT>
void launch_refine(const Run &r) {
    fseg_ctx *c = r.c;
    if (r.iv_cand)
        hipLaunchKernelGGL(k_segments_cand<COUNT>, dim3(r.iv_cand_grid), dim3(kIvCandThreads), 0, r.s, c->d_pos_off.p,
                           c->d_cand_off.p, c->d_cand_y.p, c->d_seg_iv.p, c->d_y_raw.as<COUNT>(), c->d_blk_pre.p, c->d_tile_tot.p,
                           c->d_iv_tile0.p, c->d_chosen.p, r.flag_final_bits, c->d_rseg_c.p, c->d_seg_prev.p, r.st);
    else
        hipLaunchKernelGGL(k_segments<COUNT>, dim3(grid_for(c->batch.K, 1, 8192)), dim3(r.iv_threads), 0, r.s, c->batch.K, c->d_pos_off.p,
                           c->d_cand_off.p, c->d_cand_y.p, c->d_y_raw.as<COUNT>(), c->d_blk_pre.p, c->d_tile_tot.p, c->d_iv_tile0.p,
                           c->d_chosen.p, r.flag_final_bits, c->d_rseg_c.p,
                           c->d_seg_prev.p, r.st);
    hipLaunchKernelGGL(k_refine<COUNT>, dim3(2048), dim3(64), 0, r.s, r.st, c->d_seg_iv.p, c->d_rseg_c.p,
                       c->d_seg_prev.p, c->d_cand_y.p, c->d_pos_off.p, c->d_y_raw.as<COUNT>(),
                       c->d_w_refine.p, c->P.radius_refine, c->P.sigma, c->d_g.p, c->d_pk.p,
                       c->d_pf.p, c->d_kp.p, r.flag_final_bits);
}

// SEG_PRE1: status reset, histogram .. problem ranges and the problem scan
void seg_pre1(Run &r) {
    fseg_ctx *c = r.c;
    hipStream_t s = r.s;
    Status *st = r.st;
    const int n_part = c->batch.n_part;
    const i64 K = c->batch.K, NPOS = c->batch.NPOS;
    {   // Status and the flag planes (OR-ed into: k_smooth, k_peaks_edges, k_segments, k_refine) by one launch (two memsets were three fill kernels)
        const i64 nw = 3 * (i64)flag_words(NPOS);
        hipLaunchKernelGGL(k_clear, dim3(grid_for(nw / 4 + 1, 256, 2048)), dim3(256), 0, s, st, c->d_bits.p, nw);
    }
    r.begin(ST_HIST);
    // S1
    c->paths[fseg_ctx::PATH_HIST16] = c->batch.hist_packed;
    c->paths[fseg_ctx::PATH_YRAW16] = c->batch.yraw_narrow;
    if (c->batch.yraw_narrow) launch_hist<16, uint16_t>(r);
    else if (c->batch.hist_packed) launch_hist<16, int>(r);
    else launch_hist<32, int>(r);
    r.end(ST_HIST); r.begin(ST_SMOOTH);
    // S2
    // sigma = 5 (default) and sigma = 3 (config 5) have their own unrolled instances; any other radius runs the loop
    if (c->P.radius_main == 20) { c->paths[fseg_ctx::PATH_SMOOTH_R] = 20; launch_smooth_as<20>(r); }
    else if (c->P.radius_main == 12) { c->paths[fseg_ctx::PATH_SMOOTH_R] = 12; launch_smooth_as<12>(r); }
    else { c->paths[fseg_ctx::PATH_SMOOTH_R] = 0; launch_smooth_as<0>(r); }
    r.end(ST_SMOOTH);
    // S3a threshold: needs only the smoothed signal, like the candidates (S3b) -- the two chains run side by side
    hipStream_t q = r.fork(0);
    if (r.stage_events && c->shape.profile_all) (void)hipEventRecord(c->ev_b[ST_THRESHOLD], q);
    // batches of many partitions of moderate size: a workgroup per partition does the whole threshold (k_thr_part); a batch of a
    // few large partitions (config 2: one) keeps the batch-wide compaction and a workgroup per 8192-value chunk
    // (Until the end of round 5 a context that shares the device kept the chunk kernels: host memory -> host memory, eight contexts, the job
    // ran at 368 M reads/s with k_thr_part against 381 M without -- a difference inside that figure's box noise, as it turned out.
    // Over resident batches, three pairs of runs in one call: 527.6 / 530.8 / 531.5 with it, 524.1 / 524.4 / 503.7 without: one launch
    // of 47 us instead of seven that hold a hardware queue for 84.)
    const bool thr_part_fits = c->batch.max_part_pos <= (i64)kThrPartMaxChunks * 8192;
    const bool thr_part = thr_part_fits && (c->thr_part == 1 || (c->thr_part < 0 && n_part >= 64));
    if (thr_part) {
        c->paths[fseg_ctx::PATH_THR_PART] = 1;
        hipLaunchKernelGGL(k_thr_part, dim3(grid_for(n_part, 1, 4096)), dim3(512), 0, q, n_part, c->d_part_iv_off.p, c->d_pos_off.p, NPOS,
                           r.flag_pos_bits, c->d_y.p, c->d_v.p, c->P.variance_factor, c->d_mean.p, c->d_thr.p);
    } else {
        c->paths[fseg_ctx::PATH_THR_PART] = 0;
        u64 *scan_state = c->d_scan_state.p;
        if (!r.scan_single) {
            hipLaunchKernelGGL(k_scan1, dim3(grid_for(r.scan_nb, 1, 4096)), dim3(256), 0, q, r.flag_pos_bits, NPOS, r.bsum_side);
            hipLaunchKernelGGL(k_scan2, dim3(1), dim3(kScan2Threads), 0, q, r.bsum_side, r.scan_nb, &st->n_vals, (i64 *)nullptr);
        }
        hipLaunchKernelGGL(k_scan_emit<kEmitValues>, dim3(r.scan_grid), dim3(256), 0, q, r.flag_pos_bits, NPOS,
                           r.bsum_side, (const int *)nullptr, scan_state, &st->n_vals, (i64 *)nullptr, &st->err, c->d_y.p, c->d_v.p, K, c->d_pos_off.p,
                           c->d_iv_start.p, c->d_blk_iv0.p, (int *)nullptr, (int *)nullptr, (i64 *)nullptr,
                           c->shape.force_scan_stall ? 1 : 0, (int *)nullptr);
        hipLaunchKernelGGL(k_voff, dim3(grid_for(n_part + 1, 1, 2048)), dim3(64), 0, q, n_part, c->d_part_iv_off.p,
                           c->d_pos_off.p, NPOS, r.flag_pos_bits, r.bsum_side, scan_state, &st->n_vals,
                           c->d_voff.p);
        hipLaunchKernelGGL(k_vplan, dim3(1), dim3(256), 0, q, n_part, c->d_part_iv_off.p, c->d_pos_off.p, NPOS,
                           c->d_voff.p, c->d_chunk_off.p, st, c->chunk_cap);
        int chunk_grid = grid_for(c->chunk_cap, 1, 4096);
        double *csum0 = c->d_csum.p, *csum1 = csum0 + c->chunk_cap;
        for (int pass = 0; pass < 2; ++pass)
            hipLaunchKernelGGL(k_vsum_chunks, dim3(chunk_grid), dim3(512), 0, q, n_part, c->d_voff.p,
                               c->d_chunk_off.p, c->d_v.p, csum0, pass, pass ? csum1 : csum0, c->chunk_cap);
        hipLaunchKernelGGL(k_vsum_part, dim3(grid_for(n_part, 64, 1024)), dim3(64), 0, q, n_part, c->d_voff.p,
                           c->d_chunk_off.p, csum0, csum1, c->P.variance_factor, c->d_mean.p,
                           c->d_thr.p, c->chunk_cap);
    }
    if (r.stage_events && c->shape.profile_all) (void)hipEventRecord(c->ev_e[ST_THRESHOLD], q);
    r.begin(ST_CANDIDATES);
    // S3b candidates
    hipLaunchKernelGGL(k_peaks_edges, dim3(grid_for(c->batch.n_tiles, 256, 4096)), dim3(256), 0, s, c->batch.n_tiles, c->d_tile_desc.p,
                       c->d_tile_defer.p, c->d_y.p, r.flag_cand_bits, c->d_part_has2.p, n_part);
    // (every candidate's interval with it: what k_fix_cand, k_prob_range, k_prob_emit, k_segments_cand and k_refine index by)
    launch_positions(r, r.flag_cand_bits, 1, &st->n_cand, c->d_cand_off.p, c->d_cand_y.p, nullptr, c->d_seg_iv.p);
    r.end(ST_CANDIDATES);
    r.join(0);
    r.early_fork();
    r.begin(ST_FIX);
    // S4
    c->paths[fseg_ctx::PATH_IV_THREADS] = r.iv_threads;              // (k_segments, S6, is launched with the same block)
    c->paths[fseg_ctx::PATH_IV_CAND] = r.iv_cand;
    if (r.iv_cand)
        hipLaunchKernelGGL(k_fix_cand, dim3(r.iv_cand_grid), dim3(kIvCandThreads), 0, s, c->d_pos_off.p,
                           c->d_iv_part.p, c->d_cand_off.p, c->d_cand_y.p, c->d_y.p,
                           c->d_thr.p, c->P.max_problem_size, c->d_fixed0.p,
                           c->d_added.p, c->d_fixed.p, c->d_chosen.p,
                           c->d_cand_pn.p, c->d_seg_iv.p, st);
    else
        hipLaunchKernelGGL(k_fix, dim3(grid_for(K, 1, 8192)), dim3(r.iv_threads), 0, s, K, c->d_pos_off.p,
                           c->d_iv_part.p, c->d_cand_off.p, c->d_cand_y.p, c->d_y.p,
                           c->d_thr.p, c->P.max_problem_size, c->d_fixed0.p,
                           c->d_added.p, c->d_fixed.p, c->d_chosen.p,
                           c->d_cand_pn.p, c->d_seg_iv.p, st);
    // (with the block sums of the problem scan when the scan is a launch of its own: k_prob_scan1 is the rescan's only)
    launch_prob_range(c, r.split, r.prob_bs);
    if (r.prob_bs) launch_prob_scan(c, r.split, r.prob_bs, false);
    r.end(ST_FIX);
}

// SEG_PRE2: problem list, pair thresholds, window coverage
void seg_pre2(Run &r) {
    fseg_ctx *c = r.c;
    hipStream_t s = r.s;
    Status *st = r.st;
    const ProblemArrays &pr = r.pr;
    if (!(r.segs & SEG_PRE1)) r.early_fork();
    r.begin(ST_SCORE_PREP);
    hipLaunchKernelGGL(k_prob_emit, dim3(r.pg), dim3(256), 0, s, st, c->d_cand_pn.p, c->d_cand_ll.p,
                       c->d_cand_ln.p, c->d_seg_iv.p, c->d_cand_off.p, r.prob_bs,
                       pr, c->prob_cap, c->d_work_pc.p, c->d_cls_items.p,
                       c->work_cap, c->d_dp_items.p, c->d_prob_desc.p, c->d_iv_start.p,
                       c->d_iv_part.p, c->d_part_lane_off.p, r.split, c->d_solve_items.p, c->d_solve_desc.p,
                       c->d_wide_items.p, c->d_wide_all.p, c->d_cand_wide.p,
                       r.dev_sync ? r.sw : (SyncWords *)nullptr, r.sync_gen);
    r.launch_fork_waiters();
    // S5.  The arena path's window coverage (and pair thresholds) are launches of their own in front of k_score: they are
    // interval scoring (get_cumulative_coverage :188-246 -- the solve-list kernels do the same inside their workgroups), so
    // where the stages are bracketed by events the scoring stage's bracket opens here
    if (c->prob_cap > 0 && r.facts.any_arena) {
        if (r.stage_events && (r.segs & SEG_SCORE)) { r.end(ST_SCORE_PREP); r.begin(ST_SCORE); r.score_begun = true; }
        const int work_grid = grid_for(c->work_cap, 1, 4096);
        const int cov_blocks = work_grid < 2048 ? work_grid : 2048;
        const int pt_blocks = c->shape.small_batch ? grid_for(c->prob_cap, 1, 512) : 0;       // fused only for small batches
        if (!pt_blocks)
            hipLaunchKernelGGL(k_pair_thresholds, dim3(grid_for(c->prob_cap, 1, 2048)), dim3(256), 0, s, st, pr,
                               c->d_prob_desc.p, c->prob_cap, c->d_cand_off.p, c->d_cand_y.p,
                               c->d_h_table.p, c->P.h_len,
                               c->P.threshold_rate, c->d_pair_thr.p, c->pair_cap, c->d_amb.p,
                               c->d_out.p, c->tri_cap);
        hipLaunchKernelGGL(k_cov, dim3(cov_blocks + pt_blocks), dim3(kLaneChunk), 0, s, st,
                           c->d_prob_desc.p, c->prob_cap, c->d_work_pc.p, c->work_cap, c->d_cand_off.p,
                           c->d_cand_y.p, c->d_iv_start.p, c->d_lane_lx.p,
                           c->d_lex.p,
                           c->d_cov.p, c->cov_cap, c->d_work_active.p,
                           cov_blocks, pr, c->d_h_table.p, c->P.h_len, c->P.threshold_rate, c->d_pair_thr.p,
                           c->pair_cap, c->d_amb.p, c->d_out.p, c->tri_cap);
    }
    if (!r.score_begun) r.end(ST_SCORE_PREP);
}

// The census words (fseg_ctx::paths) by who writes them: the scoring stage resets ITS words where it begins, the others are
// written by their own stages (PATH_LANE_SORT by the upload).  A new word joins one of the two lists, or this does not compile.
constexpr int kScoreCensus[] = {
    fseg_ctx::PATH_SMALL_BATCH, fseg_ctx::PATH_TINY_ON, fseg_ctx::PATH_WAVE_ON, fseg_ctx::PATH_FUSE_ON, fseg_ctx::PATH_KEY32,
    fseg_ctx::PATH_N_SOLVE, fseg_ctx::PATH_N_SOLVE + 1, fseg_ctx::PATH_N_SOLVE + 2, fseg_ctx::PATH_N_WIDE, fseg_ctx::PATH_N_WIDE + 1,
    fseg_ctx::PATH_N_WIDE + 2, fseg_ctx::PATH_N_TINY, fseg_ctx::PATH_N_WORK, fseg_ctx::PATH_DPW, fseg_ctx::PATH_WIDE16, fseg_ctx::PATH_KNOWN,
    fseg_ctx::PATH_SOLVE8, fseg_ctx::PATH_TINY_KERNEL, fseg_ctx::PATH_SCORE, fseg_ctx::PATH_PLAN, fseg_ctx::PATH_N_ARENA_PROB,
    fseg_ctx::PATH_N_SCORE, fseg_ctx::PATH_N_SCORE + 1, fseg_ctx::PATH_N_SCORE + 2};
constexpr int kOtherCensus[] = {fseg_ctx::PATH_THR_PART, fseg_ctx::PATH_LABEL_PACKED, fseg_ctx::PATH_ARENA_DP, fseg_ctx::PATH_HIST16,
                                fseg_ctx::PATH_IV_THREADS, fseg_ctx::PATH_SMOOTH_R, fseg_ctx::PATH_YRAW16, fseg_ctx::PATH_LANE_SORT, fseg_ctx::PATH_IV_CAND};
constexpr bool census_covered() {
    int seen[fseg_ctx::PATH_WORDS] = {};
    for (int w : kScoreCensus) ++seen[w];
    for (int w : kOtherCensus) ++seen[w];
    for (int n : seen) if (n != 1) return false;
    return true;
}
static_assert(census_covered(), "every census word is the scoring stage's or another stage's, none both");

// SEG_SCORE: the interval-scoring kernels
void seg_score(Run &r) {
    fseg_ctx *c = r.c;
    hipStream_t s = r.s;
    Status *st = r.st;
    const ProblemArrays &pr = r.pr;
    const ScoreFacts &facts = r.facts;
    const ScorePlan &ps = r.ps;
    const bool known = facts.known, any_arena = facts.any_arena;
    const int tiny_max = c->shape.tiny_on ? kTiny : 0;
    if (!r.score_begun) r.begin(ST_SCORE);
    int *const census = c->paths;
    for (int w : kScoreCensus) census[w] = 0;
    census[fseg_ctx::PATH_SMALL_BATCH] = c->shape.small_batch; census[fseg_ctx::PATH_TINY_ON] = c->shape.tiny_on; census[fseg_ctx::PATH_WAVE_ON] = facts.wave;
    census[fseg_ctx::PATH_FUSE_ON] = c->use_fuse && c->shape.fuse_on; census[fseg_ctx::PATH_KNOWN] = known; census[fseg_ctx::PATH_PLAN] = ps.on;
    if (c->prob_cap > 0) {
        // What the stage launches is the list r.ops (seg_score_plan.h: which instance over which list on which stream, and why),
        // made where the Run is built.  Here the side streams are forked, the list is walked -- its order is the host's
        // launch order -- and the streams are joined.
        const bool sfork = any_arena;                               // (the arena path's work-item kernels keep their streams)
        // (forked here: a side stream continues from where it was forked)
        if (tiny_max > 0 && sfork) (void)r.fork(2);
        if (!c->shape.small_batch && sfork) { (void)r.fork(0); (void)r.fork(1); }
        if (ps.on) {
            // every side stream continues from HERE (the stage's begin event, when it is being recorded, is the first side
            // stream's fork: one marker packet less in front of everything -- each is ~5 us on its queue)
            // (every side stream on that one event: 0.135 -> 0.137-0.149 ms -- the records stagger the streams' starts)
            bool shared = !(r.stage_events && r.forking);
            for (int k = 1; k < ps.n_seg; ++k) if (ps.used[k]) {
                if (r.dev_side(k)) continue;         // forked early; its waiter (k_wait_word) is what the stream runs first
                if (!shared) {
                    shared = true;
                    if (hipError_t e = hipStreamWaitEvent(c->side[ps.side_of[k]], c->ev_b[ST_SCORE], 0); e != hipSuccess) r.fj_err = e;
                } else (void)r.fork(ps.side_of[k]);
            }
        }
        census[fseg_ctx::PATH_KEY32] = facts.key32;
        // the census of this stage's launches (cls < 0: one launch over every class)
        auto note_solve = [&](int cls, int cnt_bytes) {
            census[cnt_bytes == 2 ? fseg_ctx::PATH_WIDE16 : fseg_ctx::PATH_SOLVE8] |= cls < 0 ? 8 : 1 << cls;
            for (int q = 0; q < 3; ++q) if (cls < 0 || q == cls) {
                census[fseg_ctx::PATH_N_SOLVE + q] = known ? (int)c->shape.n_solve[q] : -1;
                if (cnt_bytes == 2) census[fseg_ctx::PATH_N_WIDE + q] = known ? (int)c->shape.n_wide[q] : -1;
            }
        };
        auto note_score = [&](int cls) {
            census[fseg_ctx::PATH_SCORE] |= cls < 0 ? 8 : 1 << cls;
            census[fseg_ctx::PATH_N_WORK] = known ? (int)(c->shape.n_cls_work[0] + c->shape.n_cls_work[1] + c->shape.n_cls_work[2] + c->shape.n_cls_work[3]) : -1;
            census[fseg_ctx::PATH_N_ARENA_PROB] = known ? (int)c->shape.n_arena_prob : -1;
            for (int q = 0; q < 3; ++q) if (cls < 0 || q == cls) census[fseg_ctx::PATH_N_SCORE + q] = known ? (int)c->shape.n_cls_work[q] : -1;
        };
        auto note_tiny = [&](int kernel) { census[fseg_ctx::PATH_TINY_KERNEL] = kernel; census[fseg_ctx::PATH_N_TINY] = known ? (int)c->shape.n_tiny : -1; };
        bool with_dpw = true;
#ifdef FSEG_ABLATE_STAGE
        // diagnostic build (wrong results, honest timing): FSEG_ABLATE = bit mask of what a planned stage leaves out --
        // 1 the DP launches (k_dpw), 2 the large class (B and what W launches), 4 the gates, 8 the mid class, 16 the small class, 32 the tiny class
        static const int abl = getenv("FSEG_ABLATE") ? atoi(getenv("FSEG_ABLATE")) : 0;
        with_dpw = !(ps.on && (abl & 1));
        auto ablated = [&](const ScoreOp &op) {
            const bool gate = op.kind == ScoreKind::GateG || op.kind == ScoreKind::GateH;
            const bool of_w = op.kind == ScoreKind::WideAll || (ps.has_w && op.cnt_bytes == 2);
            const int cls = (gate || op.kind == ScoreKind::Wave) ? -1 : (of_w ? 2 : op.cls);
            return ps.on && (((abl & 2) && cls == 2) || ((abl & 4) && gate) || ((abl & 8) && cls == 1) || ((abl & 16) && cls == 0) ||
                             ((abl & 32) && op.kind == ScoreKind::Wave));
        };
#endif
        for (int i = 0; i < r.ops.n; ++i) {
            const ScoreOp &op = r.ops.op[i];
            hipStream_t q = op.lane < 0 ? s : c->side[op.lane];
            // (a plan's side streams' waiters are released by k_prob_emit's last workgroup: emit_done)
#ifdef FSEG_ABLATE_STAGE
            if (ablated(op)) continue;
#endif
            switch (op.kind) {
            case ScoreKind::Score: note_score(op.cls); launch_class_op(c, q, op, facts, pr, with_dpw); break;
            case ScoreKind::SolveFused: case ScoreKind::SolveSplit: case ScoreKind::WideAll:
                note_solve(op.cls, op.cnt_bytes); launch_class_op(c, q, op, facts, pr, with_dpw); break;
            case ScoreKind::Wave:
                note_tiny(1);
                if (facts.key32) launch_wave<kTiny, int>(c, q, op, facts, pr); else launch_wave<kTiny, i64>(c, q, op, facts, pr);
                break;
            case ScoreKind::Tiny:
                note_tiny(2);
                hipLaunchKernelGGL(k_tiny, dim3(grid_for(op.n, 4, FSEG_WG_TINY)), dim3(256), 0, q, st, c->d_solve_desc.p,
                                   c->prob_cap, tiny_max, pr, c->d_cand_y.p, c->d_lane_ex.p,
                                   c->d_ex_ts.p, c->d_ex_te.p, c->d_h_table.p, c->P.h_len, c->P.threshold_rate,
                                   c->d_thr_tab.p, c->P.min_read_support_outside, c->d_chosen.p, list_lb(facts, 3), list_ln(facts, 3) FSEG_TARG);
                break;
            case ScoreKind::GateG: hipLaunchKernelGGL(k_gate, dim3(1), dim3(64), 0, q, st, 0, (unsigned)op.n, 3000u); break;
            case ScoreKind::GateH: hipLaunchKernelGGL(k_gate, dim3(1), dim3(64), 0, q, st, 2, (unsigned)op.n, 1500u); break;
            }
        }
        if (ps.on) {
            // join: a side chain with a device-side fork ends with k_signal and the main stream waits for the words (one wave in
            // front of k_segments) instead of two marker + barrier packets per side stream
            unsigned dev_mask = 0;
            for (int k = 1; k < ps.n_seg; ++k) if (ps.used[k]) {
                if (r.dev_side(k)) { hipLaunchKernelGGL(k_signal, dim3(1), dim3(64), 0, c->side[ps.side_of[k]], &r.sw->side_gen[ps.side_of[k]], r.sync_gen); dev_mask |= 1u << ps.side_of[k]; }
                else r.join(ps.side_of[k]);
            }
            if (dev_mask) hipLaunchKernelGGL(k_wait_word, dim3(1), dim3(64), 0, s, st, r.sw->side_gen, dev_mask, r.sync_gen, r.sync_ticks);
        }
        // (the tiny problems' kernel is joined at the end of this stage, so the stage's time bracket covers all scoring work)
        if (!c->shape.small_batch && sfork) { r.join(0); r.join(1); }
        if (c->shape.have_huge && any_arena) {
            census[fseg_ctx::PATH_SCORE] |= 16;
            hipLaunchKernelGGL(k_score_huge, dim3(256), dim3(512), kHugeScoreLds, s, st, c->d_dp_items.p, pr,
                               c->d_prob_desc.p, c->prob_cap, c->work_cap, c->d_cand_y.p,
                               c->d_cov.p, c->cov_cap, c->d_pair_thr.p, c->pair_cap,
                               c->d_out.p, c->tri_cap, c->d_amb.p);
        }
        if (c->shape.have_huge && c->shape.nm_giant > 0 && any_arena && c->d_giant.p) {
            census[fseg_ctx::PATH_SCORE] |= 32;
            hipLaunchKernelGGL(k_score_giant, dim3(kGiantWgs), dim3(512), giant_score_lds(c->shape.nm_giant), s, st, c->d_dp_items.p, pr,
                               c->d_prob_desc.p, c->prob_cap, c->work_cap, c->d_cand_y.p,
                               c->d_cov.p, c->cov_cap, c->d_pair_thr.p, c->pair_cap,
                               c->d_out.p, c->tri_cap, c->d_amb.p, c->shape.nm_giant,
                               c->d_giant.as<unsigned char>(), (i64)giant_scratch_bytes(c->shape.nm_giant));
        }
        if (tiny_max > 0 && sfork) r.join(2);    // k_tiny is interval scoring too: inside the stage's time bracket
    }
    r.end(ST_SCORE);
}

// SEG_POST1: DP, refinement, final positions, label columns
void seg_post1(Run &r) {
    fseg_ctx *c = r.c;
    hipStream_t s = r.s;
    Status *st = r.st;
    const ProblemArrays &pr = r.pr;
    const int tiny_max = c->shape.tiny_on ? kTiny : 0;
    r.begin(ST_DP);
    c->paths[fseg_ctx::PATH_ARENA_DP] = 0;
    if (c->prob_cap > 0 && r.facts.any_arena) {
        c->paths[fseg_ctx::PATH_ARENA_DP] = c->shape.dp_wide_counts ? 4 : 2;
        int dp_grid = grid_for(c->prob_cap, 1, 1024);
        const int fill_blocks = r.ride_fill ? grid_for(r.labels_n16 / 8 + 1, 512, 512) : 0;
        // 16-bit count tables unless some problem sees >= 65536 reads;
        // 512 threads (8 waves share the c2 loop) when the tables of the largest problem leave room for their scratch.
        // small_batch: one launch over every problem; otherwise one launch per DP class list.
        hipStream_t q_small = c->shape.small_batch ? s : r.fork(0);    // the DP classes own disjoint problems
        hipStream_t q_mid = c->shape.small_batch ? s : r.fork(1);
        const int big_class = c->shape.small_batch ? -1 : 1;
        if (c->shape.dp_wide_counts) {
            const bool wide_wg = dp_lds_for(c->shape.nm_big, 4) + 8 * 1024 <= kLdsPerWg;
            const int dp_blocks = dp_grid < 256 ? dp_grid : 256;
            if (!c->shape.small_batch) launch_dp_waves<unsigned>(r, q_small, q_mid);
            if (wide_wg) launch_dp<kNMax, 512, unsigned>(r, s, big_class, tiny_max, dp_blocks, fill_blocks);
            else launch_dp<kNMax, 256, unsigned>(r, s, big_class, tiny_max, dp_blocks, fill_blocks);
        } else {
            if (!c->shape.small_batch) launch_dp_waves<unsigned short>(r, q_small, q_mid);
            launch_dp<kNMax, 512, unsigned short>(r, s, big_class, tiny_max, dp_grid < 512 ? dp_grid : 512, fill_blocks);
        }
        if (!c->shape.small_batch) { r.join(0); r.join(1); }
        if (c->shape.have_huge)
            hipLaunchKernelGGL(k_dp_huge, dim3(dp_grid < 256 ? dp_grid : 256), dim3(512), kHugeDpLds, s, st, c->d_dp_items.p,
                               pr, c->d_prob_desc.p, c->prob_cap, c->d_cand_y.p, c->d_out.p,
                               c->tri_cap, c->d_amb.p, c->d_pair_thr.p, c->pair_cap,
                               c->P.min_read_support_outside, c->d_chosen.p);
        if (c->shape.have_huge && c->shape.nm_giant > 0 && c->d_giant.p)
            hipLaunchKernelGGL(k_dp_giant, dim3(kGiantWgs), dim3(512), giant_dp_lds(c->shape.nm_giant), s, st, c->d_dp_items.p,
                               pr, c->d_prob_desc.p, c->prob_cap, c->d_cand_y.p, c->d_out.p,
                               c->tri_cap, c->d_amb.p, c->d_pair_thr.p, c->pair_cap,
                               c->P.min_read_support_outside, c->d_chosen.p, c->shape.nm_giant,
                               c->d_giant.as<unsigned char>(), (i64)giant_scratch_bytes(c->shape.nm_giant));
    }
    r.end(ST_DP); r.begin(ST_REFINE);
    // S6
    if (c->batch.yraw_narrow) launch_refine<uint16_t>(r);
    else launch_refine<int>(r);
    r.end(ST_REFINE); r.begin(ST_FINAL);
    launch_positions(r, r.flag_final_bits, 2, &st->n_final, c->d_final_off.p, c->d_final_y.p, c->d_final_pos.p, c->d_final_iv.p);
    // S7, first half: per-column thresholds and the label arena's plan
    hipLaunchKernelGGL(k_label_cols, dim3(grid_for(c->batch.NPOS / 8 + 1, 256, 2048)), dim3(256), 0, s, c->batch.K, c->d_final_off.p,
                       c->d_final_y.p, c->d_final_iv.p, c->d_iv_part.p, c->d_h_table.p, c->P.h_len,
                       c->P.threshold_rate, c->d_thr_tab.p, c->d_col_thr.p, c->d_col_zero.p,
                       c->d_part_has2.p, c->batch.n_part, c->d_part_iv_off.p, c->d_part_rep_off.p,
                       c->d_label_off.p, st, c->label_cap);
    r.end(ST_FINAL);
}

// SEG_POST2: label arena fill + per-read labels; a sized run fills exactly label_fill_bytes with a kernel of its own
void seg_post2(Run &r, i64 label_fill_bytes) {
    fseg_ctx *c = r.c;
    hipStream_t s = r.s;
    const bool lab_packed = r.lab_packed;
    r.begin(ST_LABEL);
    if (c->label_cap > 0) {
        c->run_label_packed = lab_packed; c->labels_unpacked = false;
        c->paths[fseg_ctx::PATH_LABEL_PACKED] = lab_packed;
        const i64 n16 = r.sized ? (label_fill_bytes + 15) / 16 : r.labels_n16;
        if (lab_packed) {
            if (n16 > 0)                                            // (one launch: a hipMemsetAsync of 19 MB is two fill kernels here)
                hipLaunchKernelGGL(k_clear, dim3(grid_for(n16 / 4 + 1, 256, 4096)), dim3(256), 0, s, (Status *)nullptr, c->d_packed.p, n16);
        } else if (!r.ride_fill) {                                  // no DP launch carried the fill
            if (n16 > 0)
                hipLaunchKernelGGL(k_label_zero, dim3(grid_for(n16 / 8 + 1, 256, 4096)), dim3(256), 0, s, c->d_labels.as<uint4>(), n16);
        }
        const int lab_grid = grid_for((i64)c->batch.n_rep_blocks * kLabelSplit, 1, c->label_grid > 0 && c->label_grid < 65536 ? c->label_grid : 65536);
        hipLaunchKernelGGL(k_label_reads, dim3(lab_grid), dim3(256), 0, s, c->batch.n_rep_blocks,
                           c->d_rb_part.p, c->d_rb_r0.p, c->d_label_off.p, c->label_cap, c->batch.n_part,
                           c->d_part_iv_off.p, c->d_part_rep_off.p, c->d_final_off.p,
                           c->d_final_pos.p, c->d_col_thr.p, c->d_rep_exon_off.p,
                           c->d_ex_ts.p, c->d_ex_te.p, c->d_col_zero.p,
                           c->d_part_has2.p, c->d_labels.as<unsigned char>(), lab_packed ? c->d_packed.p : (unsigned *)nullptr);
    }
    r.end(ST_LABEL);
}

// Enqueue the segments `segs` of one run on the context's stream: the launch sequence of the pipeline, a function per segment.
// A call holds any subset: everything (a replay as plain launches, a capture), the sized first run's three pieces, the halves
// of a profiled replay's two graphs and the scoring stage between them.
//   sized: the run is being launched piecewise with the host reading the sizes in between (first run of a batch):
//          the problem scan always runs as its own kernels (their totals are what the host waits for) and the label
//          arena is filled by its own kernel over exactly label_fill_bytes.
int enqueue_run(fseg_ctx *c, unsigned segs, bool sized = false, i64 label_fill_bytes = 0) {
    Run r(c, segs, sized);
    if (segs & SEG_PRE1) seg_pre1(r);
    if (segs & SEG_PRE2) seg_pre2(r);
    if (segs & SEG_SCORE) seg_score(r);
    if (segs & SEG_POST1) seg_post1(r);
    if (segs & SEG_POST2) seg_post2(r, label_fill_bytes);
    if (segs & SEG_STATUS) HIP_TRY(c, hipMemcpyAsync(c->h_status.p, r.st, sizeof(Status), hipMemcpyDeviceToHost, r.s));
    HIP_TRY(c, r.fj_err);
    HIP_TRY(c, hipGetLastError());
    return FSEG_OK;
}

// wait for the stream: poll for a while (a run is well under a millisecond on a resident batch and the blocking
// wait's wake-up costs tens of microseconds), then block
hipError_t wait_stream(fseg_ctx *c) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        hipError_t e = hipStreamQuery(c->stream);
        if (e != hipErrorNotReady) { (void)hipGetLastError(); return e; }     // NotReady must not linger as the thread's last error
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
    (void)hipGetLastError();
    return hipStreamSynchronize(c->stream);
}

// the device-side validation of the last upload (read once, with the first status record of the batch)
int check_prep(fseg_ctx *c) {
    if (c->prep_checked) return FSEG_OK;
    c->prep_checked = true;
    const PrepStatus &ps = *c->h_prep;
    if (!ps.err) return FSEG_OK;
    int q = 0;
    for (int i = 1; i < 4; ++i) if (((ps.err >> i) & 1u) && (!((ps.err >> q) & 1u) || ps.bad_rep[i] < ps.bad_rep[q])) q = i;
    if (!((ps.err >> q) & 1u)) for (q = 0; q < 4 && !((ps.err >> q) & 1u); ++q) {}
    const long long r = (long long)ps.bad_rep[q];
    c->have_batch = false;
    switch (1u << q) {
        case kPrepExonEnds: return fail(c, FSEG_ERR_INPUT, "rep %lld: exon with start >= end (py/freddie_segment.py:160)", r);
        case kPrepExonOrder: return fail(c, FSEG_ERR_INPUT, "rep %lld: exons out of order (py/freddie_segment.py:158)", r);
        case kPrepExonInterval: return fail(c, FSEG_ERR_INPUT, "rep %lld: an exon does not lie inside one tint interval (py/freddie_segment.py:668)", r);
        default: return fail(c, FSEG_ERR_INPUT, "rep %lld has no exons", r);
    }
}

// what the status record of a finished run says about the run's input (the reference's assertions)
int run_input_errors(fseg_ctx *c, const Status &s) {
    if (s.err & kErrExonInterval) return fail(c, FSEG_ERR_INPUT, "an exon does not lie inside one tint interval (py/freddie_segment.py:668)");
    if (s.err & kErrBreakAssert) return fail(c, FSEG_ERR_INPUT, "break_large_problems: candidate window out of range or no positive signal (py/freddie_segment.py:640-643)");
    if (s.err & kErrWideMissed) return fail(c, FSEG_ERR_HIP, "internal: a problem keeps more reads than were counted for it (kErrWideMissed)");
    if (s.err & kErrProblemTooLarge) return fail(c, FSEG_ERR_UNSUPPORTED, "a DP problem has more than %d candidates (max_problem_size beyond 1000 is not supported)", kNGiant);
    return FSEG_OK;
}

// the giant-problem kernels' LDS carve-up and scratch for a run whose largest problem has max_n candidates
int prepare_giant(fseg_ctx *c, int max_n) {
    if (max_n <= kNHuge || max_n > kNGiant) { if (max_n <= kNHuge) c->shape.nm_giant = 0; return FSEG_OK; }
    int want = (max_n + 7) & ~7;
    if (want > kNGiant) want = kNGiant;
    if (want > c->shape.nm_giant || c->shape.nm_giant == 0) c->shape.nm_giant = want;
    TRY(ensure(c, c->d_giant, (size_t)kGiantWgs * giant_scratch_bytes(c->shape.nm_giant)));
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_score_giant), hipFuncAttributeMaxDynamicSharedMemorySize, (int)giant_score_lds(kNGiant));
    if (e != hipSuccess) return fail(c, FSEG_ERR_HIP, "hipFuncSetAttribute(k_score_giant): %s", hipGetErrorString(e));
    return FSEG_OK;
}

// what the lists of the batch hold, from the status record of a run (or of the sizing pass)
void note_counts(fseg_ctx *c, const Status &s) {
    for (int q = 0; q < 3; ++q) c->shape.n_solve[q] = (i64)s.solve_cls[q];
    c->shape.n_tiny = (i64)s.n_tiny;
    for (int q = 0; q < 3; ++q) c->shape.n_wide[q] = (i64)s.wide_cls[q];
    for (int q = 0; q < 4; ++q) c->shape.n_cls_work[q] = (i64)s.cls_work[q];
    c->shape.n_arena_prob = (i64)s.dp_cls[0] + (i64)s.dp_cls[1] + (i64)s.dp_cls[2];
    c->shape.counts_known = true;
}

// launch parameters that follow from the sizes of a run (exact in a sized run, last run's otherwise)
void adapt_to(fseg_ctx *c, const Status &s) {
    const bool old_tiny = c->shape.tiny_on, old_fuse = c->shape.fuse_on;
    c->shape.small_batch = (i64)s.n_prob <= 256 && (i64)s.n_work <= 1024;
    c->shape.tiny_on = (i64)s.n_prob > c->tiny_from;                  // depends on the problem count only, which k_tiny does not change
    c->shape.fuse_on = (i64)s.max_ln <= c->fuse_lanes;                 // (the widest problem does not depend on the split either)
    c->shape.wide_solve = (i64)s.max_ln > kFuseLanes;                  // some problem needs the 16-bit counters
    // (the lists' sizes were counted under the old division of the problems: a run under the new one must not take them from the host --
    // an unsized first run of a batch with more than tiny_from problems turns k_tiny's share on for the replay, whose list bounds then
    // came from the run without it: kErrOverflowNm on every attempt, "arena sizing did not converge"; found in round 5)
    if (old_fuse != c->shape.fuse_on || old_tiny != c->shape.tiny_on) c->shape.counts_known = false;
    c->shape.prob_self_scan = (i64)s.n_cand <= fseg_ctx::kProbSelfMax;
    {   // the big-problem LDS carve-up: the largest problem (+ headroom, multiple of 4)
        int want = (int)s.max_n + 3;
        want = (want + 3) & ~3;
        if (want < kClsMid + 4) want = kClsMid + 4;
        if (want > kNMax) want = kNMax;
        c->shape.nm_big = want;
    }
}

void collect_stage_times(fseg_ctx *c, int timed_graphs) {
    if (!c->shape.profiling) return;
    for (int i = 0; i < ST_REPORTED; ++i) c->stage_ms[i] = 0.f;
    if (timed_graphs == 2) {
        (void)hipEventElapsedTime(&c->stage_ms[ST_GRAPH_PRE], c->ev_g[0], c->ev_g[1]);
        (void)hipEventElapsedTime(&c->stage_ms[ST_SCORE], c->ev_g[1], c->ev_g[2]);
        (void)hipEventElapsedTime(&c->stage_ms[ST_GRAPH_POST], c->ev_g[2], c->ev_g[3]);
    } else if (c->last_sized || c->run_plain) {
        for (int i = 0; i < ST_COUNT; ++i) {
            if (!c->shape.profile_all && i != ST_SCORE) continue;
            if (hipEventElapsedTime(&c->stage_ms[i], c->ev_b[i], c->ev_e[i]) != hipSuccess) { c->stage_ms[i] = 0.f; (void)hipGetLastError(); }
        }
    }
}

// A device-side waiter gave up: the run is redone with events (run_events_only), the context keeps its waiters for later runs
// unless it keeps happening (three times: events for good).  Counted and exposed (FSEG_TAP_SYNC): a time-out is a stall of the
// waiter's limit plus a rerun, and nothing else would show it.
static void note_sync_timeout(fseg_ctx *c) {
    c->run_events_only = true;
    if (++c->sync_timeouts >= 3 && c->dev_sync) {
        c->dev_sync = false;
        if (c->trace) fprintf(stderr, "[fseg] %u runs lost a device-side waiter to its time limit: this context forks and joins with events from now on\n", c->sync_timeouts);
    } else if (c->trace) fprintf(stderr, "[fseg] a device-side waiter reached its time limit: the run is redone with events\n");
}

static void set_in_flight(fseg_ctx *c, bool on) {
    if (!on) release_device(c);
    if (c->counted_in_flight == on || c->device < 0 || c->device >= 64) return;
    c->counted_in_flight = on;
    g_in_flight[c->device].fetch_add(on ? 1 : -1, std::memory_order_acq_rel);
}
static void claim_device(fseg_ctx *c) {
    if (c->owns_device || c->device < 0 || c->device >= 64 || !c->use_fork || others_in_flight(c)) return;
    const fseg_ctx *nobody = nullptr;
    if (g_owner[c->device].compare_exchange_strong(nobody, c, std::memory_order_acq_rel)) c->owns_device = true;
}
static void release_device(fseg_ctx *c) {
    if (!c->owns_device) return;
    c->owns_device = false;
    g_owner[c->device].store(nullptr, std::memory_order_release);
}
static bool others_in_flight(const fseg_ctx *c) {
    if (c->device < 0 || c->device >= 64) return false;
    return g_in_flight[c->device].load(std::memory_order_acquire) - (c->counted_in_flight ? 1 : 0) > 0;
}
// the run owns the device and is worth branching (see Run::forking)
static bool would_fork(const fseg_ctx *c) { return c->use_fork && !c->shape.small_batch && c->owns_device && c->side[0] != nullptr; }
static int finish_run_impl(fseg_ctx *c);
int finish_run(fseg_ctx *c) {
    const int rc = finish_run_impl(c);
    if (!c->pending) set_in_flight(c, false);
    return rc;
}
// What the host does about the status record of a run of `kind`: seg_run_react.h decides (the table there has what each kind
// does and where the kinds differ on purpose), this applies the adaptations to the context and says how the caller goes on --
// Done: with the next piece, or the run is complete; Redo: enqueue the same again (after alloc_arenas where capacities may have
// grown); Fail: return rc.  Both run paths end here: finish_run_impl (Replay) and run_sized (SizedA, SizedB).
struct Verdict { Outcome outcome; int rc; bool uses_attempt; };
Verdict react_to_status(fseg_ctx *c, const Status &s, RunKind kind) {
    i64 *const caps[CAP_COUNT] = {&c->prob_cap, &c->work_cap, &c->pair_cap, &c->tri_cap, &c->label_cap, &c->chunk_cap, &c->cov_cap};
    ReactFacts f;
    f.have_huge = c->shape.have_huge; f.dp_wide_counts = c->shape.dp_wide_counts; f.run_events_only = c->run_events_only; f.nm_giant = c->shape.nm_giant;
    for (int k = 0; k < CAP_COUNT; ++k) f.cap[k] = *caps[k];
    const Reaction r = decide_reaction(s, f, kind);
    if (r.scan_fallback) { c->shape.scan_single_max = 0; c->shape.force_scan_stall = false; }      // redo with the three-pass scan
    if (r.wave_off) { c->shape.use_wave = false; c->shape.counts_known = false; }
    if (r.sync_timeout) note_sync_timeout(c);
    if (r.nm_big_max) c->shape.nm_big = kNMax;
    c->shape.have_huge = r.have_huge; c->shape.dp_wide_counts = r.dp_wide_counts;
    for (int k = 0; k < CAP_COUNT; ++k) *caps[k] = r.cap[k];
    if (r.giant) { const int rc = prepare_giant(c, (int)s.max_n); if (rc) return {Outcome::Fail, rc, true}; }
    if (r.adopt_counts) {
        if (kind == RunKind::Replay) {                   // the run is complete
            c->pending = false;
            c->ran = true;
            collect_stage_times(c, c->run_plain ? 0 : c->n_graphs);
        }
        note_counts(c, s);
        adapt_to(c, s);
    }
    switch (r.fail) {
        case FailKind::None: break;
        case FailKind::Input:
            if (kind != RunKind::Replay) { c->pending = false; c->ran = false; }
            return {Outcome::Fail, run_input_errors(c, s), true};
        case FailKind::SizedOverflow: return {Outcome::Fail, fail(c, FSEG_ERR_HIP, "internal: a sized run overflowed an arena (status %#x)", s.err), true};
        case FailKind::TimeoutNoWaiters: return {Outcome::Fail, fail(c, FSEG_ERR_HIP, "internal: a waiter timed out in a run without waiters (status %#x)", s.err), true};
    }
    return {r.outcome, FSEG_OK, r.uses_attempt};
}

// wait for the run; grow arenas and re-run if a capacity was exceeded (never after a sized run: its capacities are exact)
static int finish_run_impl(fseg_ctx *c) {
    for (int attempt = 0; attempt < 4; ++attempt) {
        HIP_TRY(c, wait_stream(c));
        TRY(check_prep(c));
        const Verdict v = react_to_status(c, *c->h_status, RunKind::Replay);
        if (v.outcome != Outcome::Redo) return v.rc;
        TRY(alloc_arenas(c));
        c->last_sized = false;
        TRY(enqueue_run(c, SEG_ALL));
    }
    {
        const Status &s = *c->h_status;
        return fail(c, FSEG_ERR_HIP, "arena sizing did not converge (status %#x; %llu problems / cap %lld, %llu work items / %lld, pairs %llu / %lld, triples %llu / %lld, "
                    "coverage %llu / %lld, label bytes %llu / %lld, chunks %llu / %lld, widest problem sees %u reads)", s.err,
                    (unsigned long long)s.n_prob, (long long)c->prob_cap, (unsigned long long)s.n_work, (long long)c->work_cap, (unsigned long long)s.pair_used, (long long)c->pair_cap,
                    (unsigned long long)s.tri_used, (long long)c->tri_cap, (unsigned long long)s.cov_used, (long long)c->cov_cap, (unsigned long long)s.label_bytes, (long long)c->label_cap,
                    (unsigned long long)s.n_vchunks, (long long)c->chunk_cap, s.max_ln);
    }
}

// Which of the context's side streams run BESIDE its main stream (see side_ok).  Once per context, by the first run that owns the
// device: per side stream a k_probe_wait on it, then a k_signal on the (drained) main stream.  The limit is generous (2 ms: kernels of
// other contexts may be ahead of the signal in the main stream's hardware queue); a probe that runs out only costs that stream its
// waiters (events instead), never correctness.
int probe_side_queues(fseg_ctx *c) {
    if (c->side_probed || !c->side[0] || !c->d_sync.p) return FSEG_OK;
    c->side_probed = true;
    SyncWords *sw = c->d_sync.p;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < fseg_ctx::kSide; ++k) {
        const unsigned gen = ++c->probe_gen;
        unsigned res = 0;
        HIP_TRY(c, hipMemsetAsync(&sw->probe_result, 0, sizeof(unsigned), c->side[k]));
        hipLaunchKernelGGL(k_probe_wait, dim3(1), dim3(64), 0, c->side[k], &sw->probe_word, gen, &sw->probe_result, 200000u);
        hipLaunchKernelGGL(k_signal, dim3(1), dim3(64), 0, c->stream, &sw->probe_word, gen);
        HIP_TRY(c, hipStreamSynchronize(c->side[k]));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, copy_sync(c, &res, &sw->probe_result, sizeof res, hipMemcpyDeviceToHost, c->side[k]));
        c->side_ok[k] = res == 1u;
    }
    if (c->trace) fprintf(stderr, "[fseg] side streams beside the main stream (device-side waiters allowed): %d %d %d\n", (int)c->side_ok[0], (int)c->side_ok[1], (int)c->side_ok[2]);
    return FSEG_OK;
}

// First run of a batch: launched in three pieces with the host reading the status record in between, so every arena is
// sized exactly before anything is written into it -- no guessed capacities, no overflow re-run.
//   A  histogram .. problem scan   -> problems, work items, pairs, triples, coverage elements, largest / widest problem
//   B  problem list .. label plan  -> final positions, label bytes
//   C  labels
// The two waits cost a few tens of microseconds each; with two contexts per GPU (the CLI) another batch's kernels fill them.
int run_sized(fseg_ctx *c) {
    Tick tk;
    double t_a = 0, t_b = 0;
    for (int attempt = 0; attempt < 3; ++attempt) {          // (attempts = redone scans; a waiter's time-out has a retry of its own, once per run)
        // A
        TRY(enqueue_run(c, SEG_PRE1 | SEG_STATUS, true));
        HIP_TRY(c, wait_stream(c));
        TRY(check_prep(c));
        Status s = *c->h_status;
        if (!(s.err & kErrScanStall)) {   // (a stalled scan has no totals: the reaction below redoes the piece)
            // k_tiny's share of the problems was decided from the previous batch: if this batch decides otherwise, the
            // arena sizes change with it -- redo the (cheap) problem scan under the right setting
            const bool tiny = (i64)s.n_prob > c->tiny_from;
            const bool fuse = (i64)s.max_ln <= c->fuse_lanes;
            if (tiny != c->shape.tiny_on || fuse != c->shape.fuse_on) {
                if (c->trace) fprintf(stderr, "[fseg] problem split changed (tiny %d -> %d, fused %d -> %d; %llu problems, widest sees %u reads): rescan\n",
                                      (int)c->shape.tiny_on, (int)tiny, (int)c->shape.fuse_on, (int)fuse, (unsigned long long)s.n_prob, s.max_ln);
                const bool fuse_turned_on = fuse && !c->shape.fuse_on;
                c->shape.tiny_on = tiny; c->shape.fuse_on = fuse;
                const ProbSplit split = split_of(c, tiny, fuse);
                Status *st = c->d_status.p;
                if (fuse_turned_on) launch_prob_range(c, split, nullptr);   // the first pass did not count the reads the wide problems keep: nobody was going to ask
                // (the scan ADDS to the per-class counts of wide problems: the first scan's must not stay in them)
                HIP_TRY(c, hipMemsetAsync(reinterpret_cast<char *>(st) + offsetof(Status, wide_cls), 0, sizeof(st->wide_cls), c->stream));
                launch_prob_scan(c, split, c->d_prob_bs.p, true);
                HIP_TRY(c, hipMemcpyAsync(c->h_status.p, st, sizeof(Status), hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(c, wait_stream(c));
                s = *c->h_status;
            }
        }
        t_a = tk.ms();
        const Verdict va = react_to_status(c, s, RunKind::SizedA);      // the capacities, the huge / giant / wide-count kernels, the list sizes
        if (va.outcome == Outcome::Fail) return va.rc;
        if (va.outcome == Outcome::Redo) continue;
        TRY(alloc_arenas(c));
        // B
        TRY(enqueue_run(c, SEG_PRE2 | SEG_SCORE | SEG_POST1 | SEG_STATUS, true));
        HIP_TRY(c, wait_stream(c));
        s = *c->h_status;
        t_b = tk.ms();
        const Verdict vb = react_to_status(c, s, RunKind::SizedB);
        if (vb.outcome == Outcome::Fail) return vb.rc;
        if (vb.outcome == Outcome::Redo) { if (!vb.uses_attempt) --attempt; continue; }
        // C
        if ((i64)s.label_bytes > c->label_cap) {
            c->label_cap = (i64)s.label_bytes;
            TRY(ensure_label_arena(c));
            if (!labels_packed(c)) c->label_cap = (i64)c->d_labels.cap - 16;
        }
        TRY(enqueue_run(c, SEG_POST2, true, (i64)s.label_bytes));
        c->h_status->err &= ~kErrOverflowLabels;       // the plan was made against the old capacity; the arena has been grown since
        c->pending = true;
        c->last_sized = true;
        if (c->trace) fprintf(stderr, "[fseg] run (sized): A %.3f ms, B %.3f ms, C enqueued %.3f ms; %llu problems (fused %llu / %llu / %llu, widest sees %u reads), %llu work items, %llu label bytes\n",
                              t_a, t_b, tk.ms(), (unsigned long long)s.n_prob, (unsigned long long)s.solve_cls[0], (unsigned long long)s.solve_cls[1],
                              (unsigned long long)s.solve_cls[2], s.max_ln, (unsigned long long)s.n_work, (unsigned long long)s.label_bytes);
        return FSEG_OK;
    }
    return fail(c, FSEG_ERR_HIP, "the compaction scans stalled repeatedly");
}

// fseg_create, first half: what a context allocates and creates up front (on failure the caller deletes the context: that releases it)
struct LdsAttr { const void *fn; size_t bytes; template <typename F> LdsAttr(F *f, size_t b) : fn(reinterpret_cast<const void *>(f)), bytes(b) {} };
hipError_t init_resources(fseg_ctx *c, bool first_on_device) {
#define CREATE_TRY(expr) do { const hipError_t e__ = (expr); if (e__ != hipSuccess) return e__; } while (0)
    CREATE_TRY(hipSetDevice(c->device));
    CREATE_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    CREATE_TRY(c->h_status.alloc()); CREATE_TRY(c->h_prep.alloc());
    CREATE_TRY(c->d_status.alloc(sizeof(Status))); CREATE_TRY(c->d_prep.alloc(sizeof(PrepStatus)));
    CREATE_TRY(c->d_tacc.alloc(kTaccBytes));
    CREATE_TRY(hipMemsetAsync(c->d_tacc.p, 0, kTaccBytes, c->stream));
    CREATE_TRY(c->d_sync.alloc(sizeof(SyncWords)));
    CREATE_TRY(hipMemsetAsync(c->d_sync.p, 0, sizeof(SyncWords), c->stream));
    for (int i = 0; i < ST_COUNT; ++i) { CREATE_TRY(hipEventCreate(&c->ev_b[i])); CREATE_TRY(hipEventCreate(&c->ev_e[i])); }
    for (int i = 0; i < 4; ++i) CREATE_TRY(hipEventCreate(&c->ev_g[i]));
    // The side streams: at once for the first context of a device (the usual single-context user gets its four streams on
    // four hardware queues), otherwise by the first run that forks: the runtime spreads a process's streams over its few
    // hardware queues in creation order, and contexts that take turns on a device use their main streams only -- created
    // back to back, those land on different queues.
    if (first_on_device)
        for (int i = 0; i < fseg_ctx::kSide; ++i) CREATE_TRY(hipStreamCreateWithFlags(&c->side[i], hipStreamNonBlocking));
    for (int i = 0; i < fseg_ctx::kForkEvents; ++i) CREATE_TRY(hipEventCreateWithFlags(&c->fj[i], hipEventDisableTiming));
    // the kernels that are launched with more dynamic LDS than the default limit, and the most each may ask for
    const LdsAttr lds_attrs[] = {
        {k_score<kNMax>, ScoreCfg<kNMax>::kLds},
        {k_dp<kNMax, 256, unsigned>, dp_lds_for(kNMax, 4)},
        {k_dp<kNMax, 512, unsigned>, kLdsPerWg - 8 * 1024},
        {k_dp<kNMax, 512, unsigned short>, dp_lds_for(kNMax, 2)},
        {k_score_huge, kHugeScoreLds},
        {k_solve<kNMax, unsigned char, int, false>, solve_lds_for(kNMax, kNMax + 1, 1)},
        {k_solve<kNMax, unsigned char, i64, false>, solve_lds_for(kNMax, kNMax + 1, 1)},
        {k_solve<kNMax, unsigned short, int, false>, solve_lds_for(kNMax, kNMax + 1, 2)},
        {k_solve<kNMax, unsigned short, i64, false>, solve_lds_for(kNMax, kNMax + 1, 2)},
        {k_solve<kNMax, unsigned char, int, true>, solve_lds_for(kNMax, kNMax + 1, 1)},
        {k_solve<kNMax, unsigned short, int, true>, solve_lds_for(kNMax, kNMax + 1, 2)},
        {k_dpw<kNMax, unsigned char, int, 64>, dpw_lds_for(kNMax, 4, 1)},
        {k_dpw<kNMax, unsigned short, int, 64>, dpw_lds_for(kNMax, 4, 2)},
        {k_dpw<kNMax, unsigned char, i64, 64>, dpw_lds_for(kNMax, 8, 1)},
        {k_dpw<kNMax, unsigned short, i64, 64>, dpw_lds_for(kNMax, 8, 2)},
        {k_dpw<kNMax, unsigned char, int, 512>, dpw_lds_for(kNMax, 4, 1)},
        {k_dpw<kNMax, unsigned short, int, 512>, dpw_lds_for(kNMax, 4, 2)},
        {k_dpw<kNMax, unsigned char, i64, 512>, dpw_lds_for(kNMax, 8, 1)},
        {k_dpw<kNMax, unsigned short, i64, 512>, dpw_lds_for(kNMax, 8, 2)},
        {k_dp_huge, kHugeDpLds},
    };
    for (const auto &a : lds_attrs) CREATE_TRY(hipFuncSetAttribute(a.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.bytes));
#undef CREATE_TRY
    return hipSuccess;
}

// The FSEG_* switches, read once per context: a flag is on where the value begins with '1'; an off-flag turns its default off where it
// begins with '0'; a tri-state takes '0' or '1', else "decide per batch" stays; an integer is taken where the value is not empty.
bool env_flag(const char *name) { const char *v = getenv(name); return v && v[0] == '1'; }
bool env_off(const char *name) { const char *v = getenv(name); return v && v[0] == '0'; }
void env_tri(const char *name, int &out) { const char *v = getenv(name); if (v && (v[0] == '0' || v[0] == '1')) out = v[0] - '0'; }
bool env_int(const char *name, i64 &out) { const char *v = getenv(name); if (!v || !v[0]) return false; out = atoll(v); return true; }
const char *env_str(const char *name) { return getenv(name); }

void read_switches(fseg_ctx *c) {
    i64 v = 0;
    if (env_off("FSEG_DEV_SYNC")) c->dev_sync = false;
    if (env_flag("FSEG_LABEL_BYTES")) c->label_packed_ok = false;
    env_tri("FSEG_THR_PART", c->thr_part);
    env_tri("FSEG_HIST16", c->hist16);
    env_tri("FSEG_YRAW16", c->yraw16);
    env_tri("FSEG_IV_CAND", c->iv_cand);
    if (env_int("FSEG_LABEL_GRID", v) && v > 0) c->label_grid = v;
    if (env_int("FSEG_SYNC_TICKS", v) && v > 0) c->sync_ticks = (unsigned)v;
    if (env_flag("FSEG_NO_GRAPH")) c->use_graph = false;
    if (env_flag("FSEG_NO_FORK")) c->use_fork = false;
    if (env_flag("FSEG_NO_FUSE")) c->use_fuse = false;
    if (env_flag("FSEG_NO_WAVE")) c->shape.use_wave = false;
    if (env_flag("FSEG_FORCE_KEY64")) c->force_key64 = true;
    if (env_flag("FSEG_WIDE_BY_SEEN")) c->wide_by_seen = true;
    if (const char *s = env_str("FSEG_SPLIT_DP")) c->split_dp = atoi(s) & 15;       // (set but empty counts: 0, no class hands its DPs over)
    if (const char *s = env_str("FSEG_SCORE_PLAN")) snprintf(c->score_plan, sizeof c->score_plan, "%s", s);
    if (!score_plan_valid(c->score_plan)) c->score_plan[0] = 0;
    if (env_int("FSEG_FUSE_LANES", v) && v > 0 && v <= kFuseLanesWide) c->fuse_lanes = (int)v;
    if (env_flag("FSEG_NO_SIZED")) c->use_sized = false;
    if (env_flag("FSEG_TRACE")) c->trace = true;
    if (env_flag("FSEG_GLOBAL_SORT")) c->force_global_sort = true;
    if (env_flag("FSEG_FORCE_SCAN_STALL")) c->shape.force_scan_stall = true;
    if (env_int("FSEG_TINY_FROM", v)) c->tiny_from = v;
    if (env_int("FSEG_SCAN_SINGLE_MAX", v)) c->shape.scan_single_max = v;
}

}  // namespace

fseg_ctx::~fseg_ctx() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    for (hipStream_t q : side) if (q) (void)hipStreamSynchronize(q);
    drop_graph(this);
    if (hsa_agent >= 0) (void)hsa_signal_destroy(hsa_sig);
    for (hipEvent_t e : ev_b) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev_e) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev_g) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : fj) if (e) (void)hipEventDestroy(e);
    for (hipStream_t q : side) if (q) (void)hipStreamDestroy(q);
    if (stream) (void)hipStreamDestroy(stream);
}

// ---------------------------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

int fseg_abi_version(void) { return FSEG_ABI_VERSION; }

#ifndef FREDDIE_SOURCE_HASH
#define FREDDIE_SOURCE_HASH ""
#endif
static const char freddie_source_stamp[] __attribute__((used)) = "FREDDIE_SRC_HASH=" FREDDIE_SOURCE_HASH;
const char *fseg_source_hash(void) { return freddie_source_stamp + 17; }

const char *fseg_last_error(const fseg_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int fseg_create(int device, fseg_ctx **out) {
    if (!out) return FSEG_ERR_ARG;
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        g_create_error = std::string("no HIP device available: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0") +
                         " (this library has no CPU fallback)";
        return FSEG_ERR_HIP;
    }
    if (device < 0 || device >= n) { g_create_error = "device ordinal out of range"; return FSEG_ERR_ARG; }
    fseg_ctx *c = new fseg_ctx();
    c->device = device;
    c->counted_live = device >= 0 && device < 64;
    const bool first_on_device = c->counted_live && g_live[device].fetch_add(1) == 0;
    e = init_resources(c, first_on_device);
    if (e != hipSuccess) {           // (whatever had been made by then goes with the context)
        g_create_error = std::string("context creation failed: ") + hipGetErrorString(e);
        if (c->counted_live) g_live[device].fetch_sub(1);
        delete c;
        return FSEG_ERR_HIP;
    }
    read_switches(c);
    *out = c;
    return FSEG_OK;
}

void fseg_destroy(fseg_ctx *c) {
    if (!c) return;
    set_in_flight(c, false);
    release_device(c);
    if (c->counted_live) { g_live[c->device].fetch_sub(1); c->counted_live = false; }
    delete c;
}

int fseg_set_params(fseg_ctx *c, const fseg_params *p) {
    if (!c || !p) return FSEG_ERR_ARG;
    // the ranges parse_args() asserts (py/freddie_segment.py:104-109)
    if (!(p->threshold_rate >= 0.5 && p->threshold_rate <= 1.0)) return fail(c, FSEG_ERR_ARG, "threshold_rate must be in [0.5, 1]");
    if (!(p->variance_factor > 0 && p->variance_factor < 10)) return fail(c, FSEG_ERR_ARG, "variance_factor must be in (0, 10)");
    if (!(p->sigma > 0 && p->sigma <= 50)) return fail(c, FSEG_ERR_ARG, "sigma must be in (0, 50]");
    if (!(p->max_problem_size > 3)) return fail(c, FSEG_ERR_ARG, "max_problem_size must be > 3");
    if (p->min_read_support_outside < 0) return fail(c, FSEG_ERR_ARG, "min_read_support_outside must be >= 0");
    if (p->radius_main < 0 || p->radius_main > kMaxRadius || p->radius_refine < 0 || p->radius_refine > kMaxRadius)
        return fail(c, FSEG_ERR_ARG, "Gaussian radius out of range");
    if (!p->w_main || !p->w_refine || !p->h_table || p->h_len <= 0) return fail(c, FSEG_ERR_ARG, "missing weight / threshold tables");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    drop_graph(c);
    c->P = *p;
    c->w_main.assign(p->w_main, p->w_main + p->radius_main + 1);
    c->w_refine.assign(p->w_refine, p->w_refine + p->radius_refine + 1);
    c->h_table.assign(p->h_table, p->h_table + p->h_len);
    c->P.w_main = c->w_main.data(); c->P.w_refine = c->w_refine.data(); c->P.h_table = c->h_table.data();
    TRY(upload_vec(c, c->d_w_main, c->w_main.data(), c->w_main.size()));
    TRY(upload_vec(c, c->d_w_refine, c->w_refine.data(), c->w_refine.size()));
    TRY(upload_vec(c, c->d_h_table, c->h_table.data(), c->h_table.size()));
    TRY(ensure(c, c->d_thr_tab, (size_t)kThrTab * sizeof(int2)));
    hipLaunchKernelGGL(k_thr_table, dim3(kThrTab / 256), dim3(256), 0, c->stream, c->d_h_table.p, c->P.h_len,
                       c->P.threshold_rate, c->d_thr_tab.p);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // lo < 0 (label_thresholds: no v >= 0 with v / L < 1 - h) exactly where h >= 1: the rate itself, or an entry of the table that
    // round(y, 2) took to 1.0 (segment lengths start at 1)
    c->label_has2 = !(p->threshold_rate < 1.0);
    for (int L = 1; L < p->h_len; ++L) if (!(c->h_table[(size_t)L] < 1.0)) c->label_has2 = true;
    c->have_params = true;
    c->ran = false;          // results of an earlier run belong to other parameters
    c->shape.counts_known = false; // ... and so do the sizes of its lists
    return FSEG_OK;
}

// One pinned staging image, one host-to-device copy, then the device derives what used to be host work (validation
// of every exon, the per-partition sort of the reps, the lane list, the histogram chunks' lane ranges).  Returns
// without waiting for the device: what the device-side validation finds is reported by the first call that waits
// (fseg_run / fseg_sync / fseg_download ...).
static int upload_impl(fseg_ctx *c, const fseg_batch *b);
int fseg_upload(fseg_ctx *c, const fseg_batch *b) {
    const int rc = upload_impl(c, b);
    if (rc != FSEG_OK && c) set_in_flight(c, false);     // nothing of this batch will run: the device's other contexts may fork again
    return rc;
}
static int launch_prep(fseg_ctx *c, const UploadPlan &pl);
static int carve_work(fseg_ctx *c, const UploadPlan &pl);
// plan (seg_upload_plan.h) | carve the input slab by the plan's counts | fill the derived tables | stage the caller's arrays |
// one copy, the device-side preparation | the work slabs and arenas
static int upload_impl(fseg_ctx *c, const fseg_batch *b) {
    if (!c || !b) return FSEG_ERR_ARG;
    if (b->n_part <= 0 || !b->part_iv_off || !b->iv_start || !b->iv_end || !b->part_rep_off || !b->rep_weight ||
        !b->rep_exon_off || !b->ex_ts || !b->ex_te)
        return fail(c, FSEG_ERR_ARG, "fseg_upload: null array or empty batch");
    HIP_TRY(c, hipSetDevice(c->device));
    Tick tk;
    // the previous batch's work (and its copy out of the staging image) must be over before its buffers are reused
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->pending = false; c->have_batch = false; c->ran = false; c->fetched = false; c->shape.counts_known = false;
    set_in_flight(c, true);                              // until the run that follows has completed (finish_run)
    const UploadPlan pl = plan_upload(*b, c->hist16, c->yraw16);
    if (pl.rc != FSEG_OK) return fail(c, pl.rc, "%s", pl.msg);
    const BatchFacts &f = pl.batch;
    // ---- the input slab: [uploaded part, mirrored by the pinned staging image][device-derived part]
    Carve in;
    in.add(c->d_part_iv_off, pl.n.part_off); in.add(c->d_part_rep_off, pl.n.part_off); in.add(c->d_part_lane_off, pl.n.part_off);
    in.add(c->d_iv_start, pl.n.iv); in.add(c->d_iv_end, pl.n.iv); in.add(c->d_pos_off, pl.n.pos_off); in.add(c->d_iv_part, pl.n.iv); in.add(c->d_iv_tile0, pl.n.iv);
    in.add(c->d_tile_desc, pl.n.tiles);
    in.add(c->d_blk_iv0, pl.n.blk_iv0);
    in.add(c->d_rb_part, pl.n.rep_blocks); in.add(c->d_rb_r0, pl.n.rep_blocks);
    in.add(c->d_hc_part, pl.n.chunks); in.add(c->d_hc_p0, pl.n.chunks); in.add(c->d_hc_n, pl.n.chunks); in.add(c->d_hc_glo, pl.n.chunks); in.add(c->d_hc_ghi, pl.n.chunks);
    in.add(c->d_rep_exon_off, f.R + 1); in.add(c->d_rep_weight, f.R);
    in.add(c->d_ex_ts, f.I, kExonPad); in.add(c->d_ex_te, f.I, kExonPad);
    const size_t up_bytes = in.total;
    in.add(c->d_lane_ex, f.LANES); in.add(c->d_lane_start, f.LANES); in.add(c->d_lane_pmax, f.LANES);
    in.add(c->d_hc_llo, pl.n.chunks); in.add(c->d_hc_lhi, pl.n.chunks);
    in.add(c->d_key_a, f.R); in.add(c->d_key_b, f.R); in.add(c->d_val_a, f.R); in.add(c->d_val_b, f.R); in.add(c->d_rep_last, f.R);
    in.add(c->d_rb_sum, pl.n.rep_blocks); in.add(c->d_rb_base, pl.n.rep_blocks); in.add(c->d_rb_max, pl.n.rep_blocks); in.add(c->d_rb_cmax, pl.n.rep_blocks);
    in.add(c->d_rb_esum, pl.n.rep_blocks); in.add(c->d_rb_ebase, pl.n.rep_blocks);
    in.add(c->d_lane_lx, f.LANES, 64); in.add(c->d_lex, f.I, kLexPad);
    TRY(reserve(c, c->slab_in, in.total));
    in.bind(c->slab_in.p);
    TRY(reserve_host(c, c->h_stage, up_bytes));
    const double t_plan = tk.ms();
    // ---- the small derived tables, written straight into the staging image
    fill_upload_tables(*b, pl, UploadTables{host_of(c, c->d_pos_off), host_of(c, c->d_part_lane_off), host_of(c, c->d_iv_part), host_of(c, c->d_iv_tile0),
                                            host_of(c, c->d_tile_desc), host_of(c, c->d_blk_iv0), host_of(c, c->d_rb_part), host_of(c, c->d_rb_r0),
                                            host_of(c, c->d_hc_part), host_of(c, c->d_hc_p0), host_of(c, c->d_hc_n), host_of(c, c->d_hc_glo), host_of(c, c->d_hc_ghi)});
    const double t_tables = tk.ms();
    // ---- the caller's arrays
    auto stage_in = [&](const auto &d, const auto *src, size_t n) {
        static_assert(sizeof(*src) == sizeof(*d.p), "the caller's array and the buffer hold the same element");
        memcpy(host_of(c, d), src, d.bytes(n));
    };
    stage_in(c->d_part_iv_off, b->part_iv_off, pl.n.part_off); stage_in(c->d_part_rep_off, b->part_rep_off, pl.n.part_off);
    stage_in(c->d_iv_start, b->iv_start, pl.n.iv); stage_in(c->d_iv_end, b->iv_end, pl.n.iv);
    stage_in(c->d_rep_exon_off, b->rep_exon_off, (size_t)f.R + 1); stage_in(c->d_rep_weight, b->rep_weight, (size_t)f.R);
    stage_in(c->d_ex_ts, b->ex_ts, (size_t)f.I); stage_in(c->d_ex_te, b->ex_te, (size_t)f.I);
    const double t_copy = tk.ms();
    c->batch = f;
    c->part_iv_off.assign(b->part_iv_off, b->part_iv_off + f.n_part + 1);
    c->part_rep_off.assign(b->part_rep_off, b->part_rep_off + f.n_part + 1);
    HIP_TRY(c, hipMemcpyAsync(c->slab_in.p, c->h_stage.p, up_bytes, hipMemcpyHostToDevice, c->stream));
    TRY(launch_prep(c, pl));
    TRY(carve_work(c, pl));
    drop_graph(c);
    c->have_batch = true;
    if (c->trace)
        fprintf(stderr, "[fseg] upload: plan %.3f ms, tables %.3f ms, copy-in %.3f ms (%.1f MB), enqueue %.3f ms; %lld positions, %lld reps, %lld exons\n",
                t_plan, t_tables, t_copy, up_bytes / 1e6, tk.ms(), (long long)f.NPOS, (long long)f.R, (long long)f.I);
    return FSEG_OK;
}

// The device-side preparation of an uploaded batch: validation of every exon, the per-partition sort of the reps, the lane list,
// the histogram chunks' lane ranges
static int launch_prep(fseg_ctx *c, const UploadPlan &pl) {
    const int np = pl.batch.n_part;
    const i64 R = pl.batch.R, n_rep_blocks = pl.batch.n_rep_blocks, n_chunks = pl.batch.n_hist_chunks, max_part_reps = pl.max_part_reps;
    hipStream_t s = c->stream;
    // ---- device-side preparation
    {
        PrepStatus init;
        init.err = 0; init.pad = 0;
        for (int q = 0; q < 4; ++q) init.bad_rep[q] = 0x7fffffffffffffffLL;
        *c->h_prep = init;
        HIP_TRY(c, hipMemcpyAsync(c->d_prep.p, c->h_prep.p, sizeof(PrepStatus), hipMemcpyHostToDevice, s));
        c->prep_checked = false;
    }
    if (R > 0) {
        hipLaunchKernelGGL(k_prep_reps, dim3(grid_for(n_rep_blocks, 1, 65536)), dim3(256), 0, s, (int)n_rep_blocks, c->d_rb_part.p,
                           c->d_rb_r0.p, c->d_part_rep_off.p, c->d_part_iv_off.p, c->d_iv_start.p,
                           c->d_iv_end.p, c->d_rep_exon_off.p, c->d_ex_ts.p, c->d_ex_te.p,
                           c->d_key_a.p, c->d_val_a.p, c->d_rep_last.p, c->d_prep.p);
        // small partitions (the usual case) sort themselves inside k_lanes; a batch with a large one goes through the
        // batch-wide radix sort (FSEG_GLOBAL_SORT=1 forces it: tests)
        const bool sort_here = max_part_reps <= kLaneSortMax && !c->force_global_sort;
        if (!sort_here) {
            unsigned end_bit = 33;
            while (end_bit < 64 && ((u64)np >> (end_bit - 32)) != 0) ++end_bit;
            size_t tmp_bytes = 0;
            HIP_TRY(c, fseg_sort_pairs(nullptr, &tmp_bytes, c->d_key_a.p, c->d_key_b.p, c->d_val_a.p, c->d_val_b.p,
                                       (size_t)R, end_bit, s));
            TRY(ensure(c, c->d_sort_tmp, tmp_bytes));
            HIP_TRY(c, fseg_sort_pairs(c->d_sort_tmp.p, &tmp_bytes, c->d_key_a.p, c->d_key_b.p, c->d_val_a.p,
                                       c->d_val_b.p, (size_t)R, end_bit, s));
        }
        if (sort_here) {
            c->paths[fseg_ctx::PATH_LANE_SORT] = 0;
            hipLaunchKernelGGL(k_lanes, dim3(grid_for(np, 1, 65536)), dim3(256), 0, s, np, c->d_part_rep_off.p, c->d_part_lane_off.p,
                               c->d_key_b.p, c->d_val_b.p, c->d_rep_weight.p, c->d_rep_last.p,
                               c->d_rep_exon_off.p, c->d_lane_ex.p, c->d_lane_start.p, c->d_lane_pmax.p,
                               1, c->d_key_a.p, c->d_ex_ts.p, c->d_ex_te.p, c->d_lane_lx.p, c->d_lex.p);
        } else {
            const int rbg = grid_for(n_rep_blocks, 1, 65536);
            c->paths[fseg_ctx::PATH_LANE_SORT] = 1;
            hipLaunchKernelGGL(k_lane_blocks, dim3(rbg), dim3(256), 0, s, (int)n_rep_blocks, c->d_rb_part.p, c->d_rb_r0.p,
                               c->d_part_rep_off.p, c->d_val_b.p, c->d_rep_weight.p, c->d_rep_last.p,
                               c->d_rb_sum.p, c->d_rb_max.p, c->d_rep_exon_off.p, c->d_rb_esum.p);
            hipLaunchKernelGGL(k_lane_block_scan, dim3(grid_for(np, 4, 4096)), dim3(256), 0, s, np, (int)n_rep_blocks, c->d_rb_part.p,
                               c->d_part_lane_off.p, c->d_rb_sum.p, c->d_rb_max.p, c->d_rb_base.p,
                               c->d_rb_cmax.p, c->d_part_rep_off.p, c->d_rep_exon_off.p, c->d_rb_esum.p,
                               c->d_rb_ebase.p);
            hipLaunchKernelGGL(k_lane_emit, dim3(rbg), dim3(256), 0, s, (int)n_rep_blocks, c->d_rb_part.p, c->d_rb_r0.p,
                               c->d_part_rep_off.p, c->d_key_b.p, c->d_val_b.p, c->d_rep_weight.p,
                               c->d_rep_last.p, c->d_rep_exon_off.p, c->d_rb_base.p, c->d_rb_cmax.p,
                               c->d_lane_ex.p, c->d_lane_start.p, c->d_lane_pmax.p, c->d_rb_ebase.p,
                               c->d_ex_ts.p, c->d_ex_te.p, c->d_lane_lx.p, c->d_lex.p);
        }
    }
    hipLaunchKernelGGL(k_hist_ranges, dim3(grid_for(n_chunks, 256, 4096)), dim3(256), 0, s, (int)n_chunks, c->d_hc_part.p,
                       c->d_hc_glo.p, c->d_hc_ghi.p, c->d_part_lane_off.p, c->d_lane_start.p,
                       c->d_lane_pmax.p, c->d_hc_llo.p, c->d_hc_lhi.p);
    HIP_TRY(c, hipMemcpyAsync(c->h_prep.p, c->d_prep.p, sizeof(PrepStatus), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipGetLastError());
    return FSEG_OK;
}

// The position- and candidate-sized work buffers (candidates and finals are distinct positions, so NPOS bounds them) and the arenas
static int carve_work(fseg_ctx *c, const UploadPlan &pl) {
    const int np = pl.batch.n_part;
    const i64 NPOS = pl.batch.NPOS, K = pl.batch.K, n_tiles = pl.batch.n_tiles, nb = pl.nb, nbp = pl.nbp;
    const bool yraw_narrow = pl.batch.yraw_narrow;
    const size_t np8 = (size_t)NPOS + 64;
    auto atleast = [](i64 &cap, i64 v) { if (cap < v) cap = v; };
    atleast(c->chunk_cap, NPOS / 8192 + np + 8);              // an upper bound, not a guess
    Carve cv;
    cv.add(c->d_y_raw, np8 * (yraw_narrow ? sizeof(uint16_t) : sizeof(int))); cv.add(c->d_y, np8);      // (an array starts on a multiple of 256 bytes whatever the one before it holds)
    cv.add(c->d_bits, 3 * flag_words(np8));
    cv.add(c->d_v, np8);
    cv.add(c->d_scan_state, ((size_t)nb * 3 + 1));
    cv.add(c->d_bsum, ((size_t)nbp + 2));
    cv.add(c->d_gsum, ((size_t)pos_groups(NPOS) + 2));
    cv.add(c->d_bsum_side, ((size_t)nb + 2));
    cv.add(c->d_g, np8); cv.add(c->d_pk, np8); cv.add(c->d_pf, np8); cv.add(c->d_kp, np8);
    cv.add(c->d_part_has2, ((size_t)np + 1));
    cv.add(c->d_tile_tot, ((size_t)n_tiles + 1));
    cv.add(c->d_blk_pre, ((size_t)n_tiles + 1) * (kSmoothTile / kSumBlock));
    cv.add(c->d_tile_defer, ((size_t)n_tiles + 1));
    cv.add(c->d_voff, ((size_t)np + 2)); cv.add(c->d_chunk_off, ((size_t)np + 2));
    cv.add(c->d_mean, ((size_t)np + 1)); cv.add(c->d_thr, ((size_t)np + 1));
    cv.add(c->d_label_off, ((size_t)np + 2));
    cv.add(c->d_csum, (size_t)c->chunk_cap * 2);     // chunk sums of both passes
    cv.add(c->d_cand_off, ((size_t)K + 2)); cv.add(c->d_final_off, ((size_t)K + 2));
    cv.add(c->d_cand_y, np8); cv.add(c->d_fixed0, np8); cv.add(c->d_added, np8);
    cv.add(c->d_fixed, np8); cv.add(c->d_chosen, np8);
    cv.add(c->d_final_y, np8); cv.add(c->d_final_pos, np8); cv.add(c->d_final_iv, np8); cv.add(c->d_col_thr, np8); cv.add(c->d_col_zero, np8);
    cv.add(c->d_seg_iv, np8); cv.add(c->d_seg_prev, np8); cv.add(c->d_rseg_c, np8);
    cv.add(c->d_cand_pn, np8); cv.add(c->d_cand_ll, np8); cv.add(c->d_cand_ln, np8); cv.add(c->d_cand_wide, np8);
    cv.add(c->d_prob_bs, ((size_t)NPOS / kProbBlock + 2) * kProbCols);
    TRY(reserve(c, c->slab_pos, cv.total));
    cv.bind(c->slab_pos.p);
    // arena capacities: a sized first run makes them exact; without it (FSEG_NO_SIZED) these are first guesses that
    // finish_run() grows
    atleast(c->prob_cap, 1024); atleast(c->work_cap, 1024); atleast(c->pair_cap, 1 << 16); atleast(c->tri_cap, 1 << 18);
    atleast(c->label_cap, 1 << 16); atleast(c->cov_cap, 1 << 18);
    TRY(alloc_arenas(c));
    return FSEG_OK;
}

static int run_impl(fseg_ctx *c);
int fseg_run(fseg_ctx *c) {
    const int rc = run_impl(c);
    if (rc != FSEG_OK && c && !c->pending) set_in_flight(c, false);
    return rc;
}
static int run_impl(fseg_ctx *c) {
    if (!c) return FSEG_ERR_ARG;
    if (!c->have_params || !c->have_batch) return fail(c, FSEG_ERR_ARG, "fseg_run: set parameters and upload a batch first");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->pending) TRY(finish_run(c));
    c->fetched = false;
    c->run_events_only = false;
    set_in_flight(c, true);
    claim_device(c);
    if (c->owns_device) ++c->forked_runs;
    if (c->use_fork && !c->side[0] && c->owns_device) {
        hipStream_t made[fseg_ctx::kSide] = {};
        hipError_t e = hipSuccess;
        for (int i = 0; e == hipSuccess && i < fseg_ctx::kSide; ++i) e = hipStreamCreateWithFlags(&made[i], hipStreamNonBlocking);
        if (e != hipSuccess) {
            for (hipStream_t m : made) if (m) (void)hipStreamDestroy(m);
            return fail(c, FSEG_ERR_HIP, "hipStreamCreateWithFlags: %s", hipGetErrorString(e));
        }
        for (int i = 0; i < fseg_ctx::kSide; ++i) c->side[i] = made[i];
    }
    if (c->owns_device && c->dev_sync && !c->side_probed) TRY(probe_side_queues(c));
    // first run of a batch: piecewise with exact arena sizes; afterwards the sizes are known and the same launch
    // sequence is replayed (as a hipGraph unless disabled)
    if (!c->ran && c->use_sized) return run_sized(c);
    if (c->label_cap > 0) {
        // (the label arena of THIS run's form: a context whose parameters moved between threshold_rate < 1 -- two bits per label --
        // and threshold_rate = 1 -- bytes -- has so far only the other one; nothing to do otherwise)
        TRY(ensure_label_arena(c));
    }
    c->shape.d_labels = c->d_labels.p; c->shape.d_packed = c->d_packed.p;
    c->last_sized = false;
    c->run_plain = !c->use_graph || c->shape.profile_plain || would_fork(c);
    if (!c->run_plain) {
        c->run_linear = true;
        struct Unset { fseg_ctx *c; ~Unset() { c->run_linear = false; } } unset{c};
        if (c->n_graphs > 0 && !(c->shape == c->graph_shape)) drop_graph(c);     // captured under another shape: not this run's launches
        if (c->n_graphs == 0) {
            const int want = c->shape.profiling ? 2 : 1;
            bool ok = true;
            for (int g = 0; g < want && ok; ++g) {
                HIP_TRY(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
                int rc = enqueue_run(c, want == 1 ? SEG_ALL : (g == 0 ? (SEG_PRE1 | SEG_PRE2) : (SEG_POST1 | SEG_POST2 | SEG_STATUS)));
                hipError_t e = hipStreamEndCapture(c->stream, &c->graph[g]);
                if (rc == FSEG_OK && e == hipSuccess) e = hipGraphInstantiate(&c->graph_exec[g], c->graph[g], nullptr, nullptr, 0);
                ok = rc == FSEG_OK && e == hipSuccess;
            }
            if (ok) { c->n_graphs = want; c->graph_shape = c->shape; ++c->graph_captures; }
            else {                                         // capture not possible: fall back to plain launches
                (void)hipGetLastError();
                drop_graph(c);
                c->use_graph = false;
                c->run_plain = true;
            }
        }
        if (c->n_graphs == 1) {
            HIP_TRY(c, hipGraphLaunch(c->graph_exec[0], c->stream));
            c->pending = true;
            return FSEG_OK;
        }
        if (c->n_graphs == 2) {
            HIP_TRY(c, hipEventRecord(c->ev_g[0], c->stream));
            HIP_TRY(c, hipGraphLaunch(c->graph_exec[0], c->stream));
            HIP_TRY(c, hipEventRecord(c->ev_g[1], c->stream));
            TRY(enqueue_run(c, SEG_SCORE));
            HIP_TRY(c, hipEventRecord(c->ev_g[2], c->stream));
            HIP_TRY(c, hipGraphLaunch(c->graph_exec[1], c->stream));
            HIP_TRY(c, hipEventRecord(c->ev_g[3], c->stream));
            c->pending = true;
            return FSEG_OK;
        }
    }
    TRY(enqueue_run(c, SEG_ALL));
    c->pending = true;
    return FSEG_OK;
}

int fseg_sync(fseg_ctx *c) {
    if (!c) return FSEG_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->pending) return finish_run(c);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->have_batch) TRY(check_prep(c));
    return FSEG_OK;
}

int fseg_get_sizes(fseg_ctx *c, fseg_sizes *out) {
    if (!c || !out) return FSEG_ERR_ARG;
    TRY(fseg_sync(c));
    if (!c->ran) return fail(c, FSEG_ERR_ARG, "no completed run");
    out->n_final = (int64_t)c->h_status->n_final;
    out->label_bytes = (int64_t)c->h_status->label_bytes;
    out->n_cand = (int64_t)c->h_status->n_cand;
    out->n_problems = (int64_t)c->h_status->n_prob;
    out->n_positions = c->batch.NPOS;
    out->max_problem_size = (int64_t)c->h_status->max_n;
    out->max_problem_reads = (int64_t)c->h_status->max_ln;
    return FSEG_OK;
}

// Results of the last run in the context's pinned host buffers (one device-to-host copy each, no pageable staging):
// valid until the next fseg_results / fseg_results_packed on this context (nothing else writes them: see include/freddie_seg.h).
// Large device-to-host copies go to an SDMA engine through the HSA runtime.  hipMemcpyAsync performs a large copy to pinned
// host memory with a copy KERNEL (256 workgroups that wait on PCIe): it holds its hardware queue for the 340 us the copy
// takes, and the kernels of the contexts that share the queue behind it (six contexts taking turns: 253 -> 280 M reads/s
// with the copy on SDMA).  The HSA agent of a HIP device is found by its PCI address; if anything of this fails the copy
// falls back to hipMemcpyAsync (FSEG_NO_SDMA_D2H=1 forces that).
struct HsaAgents { hsa_agent_t gpu[64]; unsigned bdf[64]; unsigned dom[64]; int n_gpu = 0; hsa_agent_t cpu[16]; int n_cpu = 0; bool ok = false; };
static hsa_status_t hsa_agent_cb(hsa_agent_t a, void *data) {
    HsaAgents *h = static_cast<HsaAgents *>(data);
    hsa_device_type_t t;
    if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
    if (t == HSA_DEVICE_TYPE_GPU) {
        if (h->n_gpu < 64) {
            unsigned bdf = 0, dom = 0;
            (void)hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_BDFID, &bdf);
            (void)hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_DOMAIN, &dom);
            h->gpu[h->n_gpu] = a; h->bdf[h->n_gpu] = bdf & 0xffffu; h->dom[h->n_gpu] = dom; ++h->n_gpu;
        }
    } else if (t == HSA_DEVICE_TYPE_CPU) { if (h->n_cpu < 16) h->cpu[h->n_cpu++] = a; }
    return HSA_STATUS_SUCCESS;
}
static HsaAgents &hsa_agents() {
    static HsaAgents h;
    static std::once_flag once;
    std::call_once(once, [] {
        const char *v = getenv("FSEG_NO_SDMA_D2H");
        if (v && v[0] == '1') return;
        if (hsa_init() == HSA_STATUS_SUCCESS && hsa_iterate_agents(hsa_agent_cb, &h) == HSA_STATUS_SUCCESS) h.ok = h.n_gpu > 0 && h.n_cpu > 0;
    });
    return h;
}
// the copy is issued when the stream's work is over (the caller has waited for it) and waited for here
static bool sdma_d2h(fseg_ctx *c, void *dst_pinned, const void *src_dev, size_t bytes) {
    HsaAgents &h = hsa_agents();
    if (!h.ok) return false;
    if (c->hsa_agent < 0) {                              // once per context: the agent with the device's PCI address
        c->hsa_agent = -2;
        hipDeviceProp_t pr;
        if (hipGetDeviceProperties(&pr, c->device) == hipSuccess) {
            const unsigned bdf = ((unsigned)pr.pciBusID << 8) | ((unsigned)pr.pciDeviceID << 3);
            for (int i = 0; i < h.n_gpu; ++i)
                if ((h.bdf[i] & 0xfff8u) == bdf && h.dom[i] == (unsigned)pr.pciDomainID) c->hsa_agent = i;
        }
        if (c->hsa_agent >= 0 && hsa_signal_create(1, 0, nullptr, &c->hsa_sig) != HSA_STATUS_SUCCESS) c->hsa_agent = -2;
    }
    if (c->hsa_agent < 0) return false;
    // the destination's agent: the CPU (NUMA node) that owns the pinned buffer, asked of the runtime whenever the buffer has
    // been reallocated; the first CPU agent if it will not say
    if (c->hsa_dst_base != c->h_res.p) {
        c->hsa_dst_base = c->h_res.p;
        c->hsa_cpu = 0;
        hsa_amd_pointer_info_t info;
        memset(&info, 0, sizeof info);
        info.size = sizeof info;
        if (hsa_amd_pointer_info(dst_pinned, &info, nullptr, nullptr, nullptr) == HSA_STATUS_SUCCESS)
            for (int i = 0; i < h.n_cpu; ++i) if (h.cpu[i].handle == info.agentOwner.handle) c->hsa_cpu = i;
    }
    hsa_signal_store_relaxed(c->hsa_sig, 1);
    if (hsa_amd_memory_async_copy(dst_pinned, h.cpu[c->hsa_cpu], src_dev, h.gpu[c->hsa_agent], bytes, 0, nullptr, c->hsa_sig) != HSA_STATUS_SUCCESS) return false;
    // a copy that completes takes the signal from 1 to 0; one that FAILS drives it negative, which also ends the wait:
    // then nothing can be said about the destination -- this context stays off the engine and the caller copies again
    const hsa_signal_value_t v = hsa_signal_wait_scacquire(c->hsa_sig, HSA_SIGNAL_CONDITION_LT, 1, UINT64_MAX, HSA_WAIT_STATE_BLOCKED);
    if (v != 0) {
        c->hsa_agent = -2;
        if (c->trace) fprintf(stderr, "[fseg] SDMA result copy failed (signal %lld): falling back to the runtime's copy\n", (long long)v);
        return false;
    }
    return true;
}

// the byte form of labels that the run wrote at two bits each (fseg_results / fseg_download; once per run)
static int unpack_labels(fseg_ctx *c, size_t lb) {
    if (!c->run_label_packed || c->labels_unpacked || lb == 0) return FSEG_OK;
    TRY(ensure(c, c->d_labels, lb + 32));
    const i64 n16 = (i64)((lb + 15) / 16);
    hipLaunchKernelGGL(k_unpack_labels, dim3(grid_for(n16, 256 * 4, 2048)), dim3(256), 0, c->stream, c->d_packed.p, c->d_labels.as<uint4>(), n16);
    c->labels_unpacked = true;
    return FSEG_OK;
}

static int results_impl(fseg_ctx *c, const int64_t **part_final_off, const int32_t **final_pos, const int64_t **label_off,
                        const uint8_t **labels, bool packed) {
    if (!c) return FSEG_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->pending && !c->ran) return fail(c, FSEG_ERR_ARG, "no completed run");
    hipStream_t s = c->stream;
    if (!c->fetched || c->fetched_packed != (packed ? 1 : 0)) {
        // a sized run knows its result sizes before its last kernels have finished: the copies queue up right behind them
        if (!(c->pending && c->last_sized)) TRY(fseg_sync(c));
        if (!c->pending && !c->ran) return fail(c, FSEG_ERR_ARG, "no completed run");
        const size_t nf = (size_t)c->h_status->n_final, lb = (size_t)c->h_status->label_bytes;
        size_t off = 0;
        auto take = [&](int i, size_t bytes) { c->res_off[i] = off; off = (off + bytes + 255) & ~(size_t)255; };
        take(0, bytes_of(c->d_final_off, (size_t)c->batch.K + 1)); take(1, bytes_of(c->d_final_pos, nf)); take(2, bytes_of(c->d_label_off, (size_t)c->batch.n_part + 1));
        take(3, packed ? bytes_of(c->d_packed, (lb + 15) / 16) : lb);
        TRY(reserve_host(c, c->h_res, off));
        char *h = c->h_res.p;
        HIP_TRY(c, hipMemcpyAsync(h + c->res_off[0], c->d_final_off.p, bytes_of(c->d_final_off, (size_t)c->batch.K + 1), hipMemcpyDeviceToHost, s));
        if (nf) HIP_TRY(c, hipMemcpyAsync(h + c->res_off[1], c->d_final_pos.p, bytes_of(c->d_final_pos, nf), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h + c->res_off[2], c->d_label_off.p, bytes_of(c->d_label_off, (size_t)c->batch.n_part + 1), hipMemcpyDeviceToHost, s));
        const void *big_src = nullptr;                       // the label matrix: on SDMA when it is large (see sdma_d2h)
        size_t big_bytes = 0;
        if (lb && !packed) { TRY(unpack_labels(c, lb)); big_src = c->d_labels.p; big_bytes = lb; }
        if (lb && packed) {
            // (the label arena is allocated with 16 spare bytes: the last, partial group of 16 labels is read whole)
            const i64 n16 = (i64)((lb + 15) / 16);
            if (!c->run_label_packed) {                      // the run wrote bytes (threshold_rate = 1, FSEG_LABEL_BYTES=1): pack them
                TRY(ensure(c, c->d_packed, bytes_of(c->d_packed, (size_t)n16)));
                hipLaunchKernelGGL(k_pack_labels, dim3(grid_for(n16, 256 * 4, 2048)), dim3(256), 0, s, c->d_labels.as<uint4>(),
                                   c->d_packed.p, n16);
            }
            big_src = c->d_packed.p; big_bytes = bytes_of(c->d_packed, (size_t)n16);
        }
        if (big_bytes >= (1u << 20) && hsa_agents().ok && c->hsa_agent != -2) {
            if (c->pending) TRY(finish_run(c));
            else HIP_TRY(c, hipStreamSynchronize(s));
            if (!c->ran) return fail(c, FSEG_ERR_ARG, "no completed run");
            if (sdma_d2h(c, h + c->res_off[3], big_src, big_bytes)) big_bytes = 0;
        }
        if (big_bytes) HIP_TRY(c, hipMemcpyAsync(h + c->res_off[3], big_src, big_bytes, hipMemcpyDeviceToHost, s));
        if (c->pending) TRY(finish_run(c));
        else HIP_TRY(c, hipStreamSynchronize(s));
        if (!c->ran) return fail(c, FSEG_ERR_ARG, "no completed run");
        const i64 *fo = reinterpret_cast<const i64 *>(h + c->res_off[0]);
        c->res_pfo.resize((size_t)c->batch.n_part + 1);
        for (int p = 0; p <= c->batch.n_part; ++p) c->res_pfo[(size_t)p] = fo[(size_t)c->part_iv_off[(size_t)p]];
        c->fetched = true;
        c->fetched_packed = packed ? 1 : 0;
    }
    const char *h = c->h_res.p;
    if (part_final_off) *part_final_off = reinterpret_cast<const int64_t *>(c->res_pfo.data());
    if (final_pos) *final_pos = reinterpret_cast<const int32_t *>(h + c->res_off[1]);
    if (label_off) *label_off = reinterpret_cast<const int64_t *>(h + c->res_off[2]);
    if (labels) *labels = reinterpret_cast<const uint8_t *>(h + c->res_off[3]);
    return FSEG_OK;
}

int fseg_results(fseg_ctx *c, const int64_t **part_final_off, const int32_t **final_pos, const int64_t **label_off,
                 const uint8_t **labels) {
    return results_impl(c, part_final_off, final_pos, label_off, labels, false);
}
int fseg_results_packed(fseg_ctx *c, const int64_t **part_final_off, const int32_t **final_pos, const int64_t **label_off,
                        const uint8_t **labels2) {
    return results_impl(c, part_final_off, final_pos, label_off, labels2, true);
}

int fseg_download(fseg_ctx *c, int64_t *part_final_off, int32_t *final_pos, int64_t *label_off, uint8_t *labels) {
    if (!c) return FSEG_ERR_ARG;
    TRY(fseg_sync(c));
    if (!c->ran) return fail(c, FSEG_ERR_ARG, "no completed run");
    hipStream_t s = c->stream;
    if (part_final_off) {
        std::vector<i64> fo((size_t)c->batch.K + 1);
        HIP_TRY(c, hipMemcpyAsync(fo.data(), c->d_final_off.p, bytes_of(c->d_final_off, fo.size()), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        for (int p = 0; p <= c->batch.n_part; ++p) part_final_off[p] = fo[(size_t)c->part_iv_off[p]];
    }
    if (final_pos) HIP_TRY(c, hipMemcpyAsync(final_pos, c->d_final_pos.p, bytes_of(c->d_final_pos, (size_t)c->h_status->n_final), hipMemcpyDeviceToHost, s));
    if (label_off) HIP_TRY(c, hipMemcpyAsync(label_off, c->d_label_off.p, bytes_of(c->d_label_off, (size_t)c->batch.n_part + 1), hipMemcpyDeviceToHost, s));
    if (labels && c->h_status->label_bytes) {
        TRY(unpack_labels(c, (size_t)c->h_status->label_bytes));
        HIP_TRY(c, hipMemcpyAsync(labels, c->d_labels.p, (size_t)c->h_status->label_bytes, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    return FSEG_OK;
}

// ---- per-read annotation (seg_annotate.hip) --------------------------------------------------------------------------------
// the reference asserts a read can fire, in the order of the kAn* codes (seg_kernels.h); the texts are the host writer's
static const char *const kAnMessages[kAnCodes] = {
    "", "forward_thread_cigar: t_pos > t_goal (:290)", "forward_thread_cigar: CIGAR exhausted before the goal (:293)",
    "get_interval_start: slack / query position out of range (:323-324)", "get_interval_start: no exon at or after the position (:326)",
    "get_interval_end: slack / query position out of range (:346-347)", "get_interval_end: no exon at or before the position (:349)",
    "find_longest_poly: sequence index out of range (:355)", "soft-clip positions out of order (:389)",
    "start poly tail out of range (:405,:410)", "end poly tail out of range (:435,:441,:450)",
    "unaligned gap positions out of order (:462)", "unaligned gap size out of range (:466-468)"};

static int annotate_impl(fseg_ctx *c, const fseg_reads *rd, const int64_t *label_off, const uint8_t *labels2,
                         const int64_t *part_final_off, const int32_t *final_pos) {
    if (!c || !rd) return FSEG_ERR_ARG;
    c->have_annot = false;
    const bool given = label_off || labels2 || part_final_off || final_pos;
    if (given && !(label_off && part_final_off && final_pos))
        return fail(c, FSEG_ERR_ARG, "fseg_annotate: give label_off, part_final_off and final_pos together (labels2 may be null only when there are no labels)");
    if (!c->have_batch) return fail(c, FSEG_ERR_ARG, "fseg_annotate: upload a batch first");
    HIP_TRY(c, hipSetDevice(c->device));
    TRY(fseg_sync(c));
    if (!given && !c->ran) return fail(c, FSEG_ERR_ARG, "fseg_annotate: no completed run");
    const i64 n = rd->n_read;
    if (n < 0 || n >= 0x7fffffffLL) return fail(c, FSEG_ERR_ARG, "fseg_annotate: bad n_read");
    if (n > 0 && (!rd->read_part || !rd->read_rep || !rd->strand || !rd->seq_len || !rd->seq_off || !rd->read_q_off || !rd->qs || !rd->qe ||
                  !rd->cig_off || !rd->cig_op || !rd->cig_len))
        return fail(c, FSEG_ERR_ARG, "fseg_annotate: null array");
    const int np = c->batch.n_part;
    // ---- argument checks: everything a kernel indexes with is bounded here
    const i64 *h_rep_exon_off = host_of(c, c->d_rep_exon_off);
    if (n > 0 && (rd->seq_off[0] != 0 || rd->read_q_off[0] != 0)) return fail(c, FSEG_ERR_ARG, "fseg_annotate: read 0: offsets must start at 0");
    for (i64 r = 0; r < n; ++r) {
        const int p = rd->read_part[r], rep = rd->read_rep[r];
        if (p < 0 || p >= np) return fail(c, FSEG_ERR_ARG, "fseg_annotate: read %lld: partition %d is outside the batch (%d partitions)", (long long)r, p, np);
        const i64 n_rep = c->part_rep_off[(size_t)p + 1] - c->part_rep_off[(size_t)p];
        if (rep < 0 || rep >= n_rep) return fail(c, FSEG_ERR_ARG, "fseg_annotate: read %lld: rep %d is beyond the %lld reps of partition %d", (long long)r, rep, (long long)n_rep, p);
        if (rd->seq_off[r + 1] < rd->seq_off[r]) return fail(c, FSEG_ERR_ARG, "fseg_annotate: read %lld: seq_off does not ascend", (long long)r);
        if (rd->seq_len[r] < 0 || rd->seq_len[r] > rd->seq_off[r + 1] - rd->seq_off[r])
            return fail(c, FSEG_ERR_ARG, "fseg_annotate: read %lld: seq_len is not inside its seq_off span", (long long)r);
        if (rd->read_q_off[r + 1] < rd->read_q_off[r]) return fail(c, FSEG_ERR_ARG, "fseg_annotate: read %lld: read_q_off does not ascend", (long long)r);
        const i64 g = c->part_rep_off[(size_t)p] + rep, m = h_rep_exon_off[g + 1] - h_rep_exon_off[g];
        if (rd->read_q_off[r + 1] - rd->read_q_off[r] != m)
            return fail(c, FSEG_ERR_ARG, "fseg_annotate: read %lld: read_q_off spans %lld exons, its rep has %lld", (long long)r,
                        (long long)(rd->read_q_off[r + 1] - rd->read_q_off[r]), (long long)m);
        if (rd->strand[r] != '+' && rd->strand[r] != '-') return fail(c, FSEG_ERR_ARG, "fseg_annotate: read %lld: strand is neither '+' nor '-'", (long long)r);
        for (i64 x = rd->read_q_off[r]; x < rd->read_q_off[r + 1]; ++x)
            if (rd->cig_off[x + 1] < rd->cig_off[x] || rd->cig_off[x] < 0) return fail(c, FSEG_ERR_ARG, "fseg_annotate: read %lld: cig_off does not ascend", (long long)r);
    }
    const i64 NQ = n ? rd->read_q_off[n] : 0, NC = NQ ? rd->cig_off[NQ] : 0, NL = n ? rd->seq_off[n] : 0;
    if (NL > 0 && !rd->seq_classes) return fail(c, FSEG_ERR_ARG, "fseg_annotate: null array");
    i64 n_final = 0, n_label = 0;
    if (given) {
        if (part_final_off[0] != 0 || label_off[0] != 0) return fail(c, FSEG_ERR_ARG, "fseg_annotate: partition 0: offsets must start at 0");
        for (int p = 0; p < np; ++p) {
            const i64 F = part_final_off[p + 1] - part_final_off[p], n_rep = c->part_rep_off[(size_t)p + 1] - c->part_rep_off[(size_t)p];
            if (F < 0) return fail(c, FSEG_ERR_ARG, "fseg_annotate: partition %d: part_final_off does not ascend", p);
            if (label_off[p + 1] - label_off[p] != n_rep * (F > 0 ? F - 1 : 0))
                return fail(c, FSEG_ERR_ARG, "fseg_annotate: partition %d: label_off does not span reps x (final positions - 1) labels", p);
        }
        n_final = part_final_off[np]; n_label = label_off[np];
        if (n_label > 0 && !labels2) return fail(c, FSEG_ERR_ARG, "fseg_annotate: labels2 is null");
    }
    hipStream_t s = c->stream;
    // ---- the inputs: one pinned image, one copy
    DevBuf<int> i_part, i_rep, i_slen, i_qs, i_qe, i_clen, i_fp;
    DevBuf<unsigned char> i_strand, i_cop;
    DevBuf<i64> i_soff, i_qoff, i_coff, i_pfo, i_loff;
    DevBuf<unsigned> i_cls, i_lab;           // 16 sequence classes / 16 labels a word
    Carve in;
    const size_t cls_words = (size_t)((NL + 15) / 16), lab_bytes = (size_t)((n_label + 3) / 4), lab_words = (size_t)((n_label + 15) / 16);
    in.add(i_part, (size_t)n); in.add(i_rep, (size_t)n); in.add(i_strand, (size_t)n); in.add(i_slen, (size_t)n);
    in.add(i_soff, (size_t)n + 1); in.add(i_qoff, (size_t)n + 1); in.add(i_qs, (size_t)NQ); in.add(i_qe, (size_t)NQ);
    in.add(i_coff, (size_t)NQ + 1); in.add(i_cop, (size_t)NC); in.add(i_clen, (size_t)NC); in.add(i_cls, cls_words);
    in.add(i_pfo, (size_t)np + 1);
    if (given) { in.add(i_fp, (size_t)n_final); in.add(i_loff, (size_t)np + 1); in.add(i_lab, lab_words); }
    TRY(ensure(c, c->d_an_in, in.total + 256));
    TRY(reserve_host(c, c->h_an_in, in.total + 256));
    in.bind(c->d_an_in.p);
    char *hin = c->h_an_in.p;
    auto put = [&](const auto &d, const void *src, size_t n_el) {
        if (n_el) memcpy(mirror_of(hin, c->d_an_in.p, d), src, d.bytes(n_el));
    };
    put(i_part, rd->read_part, (size_t)n); put(i_rep, rd->read_rep, (size_t)n); put(i_strand, rd->strand, (size_t)n);
    put(i_slen, rd->seq_len, (size_t)n);
    const i64 zero = 0;
    put(i_soff, n ? (const void *)rd->seq_off : &zero, (size_t)n + 1); put(i_qoff, n ? (const void *)rd->read_q_off : &zero, (size_t)n + 1);
    put(i_qs, rd->qs, (size_t)NQ); put(i_qe, rd->qe, (size_t)NQ);
    put(i_coff, NQ ? (const void *)rd->cig_off : &zero, (size_t)NQ + 1); put(i_cop, rd->cig_op, (size_t)NC); put(i_clen, rd->cig_len, (size_t)NC);
    put(i_cls, rd->seq_classes, cls_words);
    if (given) {
        put(i_pfo, part_final_off, (size_t)np + 1); put(i_fp, final_pos, (size_t)n_final); put(i_loff, label_off, (size_t)np + 1);
        if (lab_words) {                     // the caller's array ends with its last byte, the image with a whole word
            unsigned *h_lab = mirror_of(hin, c->d_an_in.p, i_lab);
            memset(h_lab, 0, i_lab.bytes(lab_words));
            memcpy(h_lab, labels2, lab_bytes);
        }
    }
    HIP_TRY(c, hipMemcpyAsync(c->d_an_in.p, hin, in.total, hipMemcpyHostToDevice, s));
    // ---- work arrays
    const i64 nb = (n + kAnScanItemsPerBlock - 1) / kAnScanItemsPerBlock;
    DevBuf<int> w_cnt, w_status;
    DevBuf<int4> w_ends, w_poly;
    DevBuf<i64> w_off, w_tok_off, w_bsum;
    DevBuf<unsigned char> w_tail;
    DevBuf<unsigned long long> w_bad;
    Carve wk;
    wk.add(w_cnt, (size_t)n * 2); wk.add(w_ends, (size_t)n); wk.add(w_poly, (size_t)n * 2); wk.add(w_off, ((size_t)n + 1) * 3);
    wk.add(w_tok_off, (size_t)n + 1); wk.add(w_tail, (size_t)n); wk.add(w_status, (size_t)n); wk.add(w_bad, 1); wk.add(w_bsum, (size_t)nb * 3 + 1);
    TRY(ensure(c, c->d_an_work, wk.total + 256));
    wk.bind(c->d_an_work.p);
    AnnotIn a{};
    a.n_read = n;
    a.read_part = i_part.p; a.read_rep = i_rep.p; a.strand = i_strand.p; a.seq_len = i_slen.p;
    a.seq_off = i_soff.p; a.read_q_off = i_qoff.p; a.qs = i_qs.p; a.qe = i_qe.p; a.cig_off = i_coff.p;
    a.cig_op = i_cop.p; a.cig_len = i_clen.p; a.seq_cls = i_cls.p;
    a.part_rep_off = c->d_part_rep_off.p; a.rep_exon_off = c->d_rep_exon_off.p; a.ex_ts = c->d_ex_ts.p; a.ex_te = c->d_ex_te.p;
    a.pfo = i_pfo.p;
    if (given) { a.final_pos = i_fp.p; a.label_off = i_loff.p; a.lab2 = i_lab.p; a.lab1 = nullptr; }
    else {
        hipLaunchKernelGGL(k_an_pfo, dim3(grid_for(np + 1, 256, 65536)), dim3(256), 0, s, np, c->d_part_iv_off.p, c->d_final_off.p, i_pfo.p);
        a.final_pos = c->d_final_pos.p; a.label_off = c->d_label_off.p;
        a.lab2 = c->run_label_packed ? c->d_packed.p : nullptr;
        a.lab1 = c->run_label_packed ? nullptr : c->d_labels.as<unsigned char>();
    }
    AnnotOut o{};
    o.cnt = w_cnt.p; o.ends = w_ends.p; o.poly = w_poly.p; o.off = w_off.p; o.tok_off = w_tok_off.p;
    o.tail = w_tail.p; o.status = w_status.p; o.first_bad = w_bad.p;
    // pinned results: offsets and the per-read bytes first (their sizes are known), the lists behind them
    size_t hoff[9], htotal = 0;
    auto take = [&](int i, size_t bytes) { hoff[i] = htotal; htotal = (htotal + bytes + 255) & ~(size_t)255; };
    const size_t off_bytes = bytes_of(w_tok_off, (size_t)n + 1);     // one list of offsets: those of w_off and w_tok_off
    take(0, off_bytes); take(1, off_bytes); take(2, off_bytes); take(3, off_bytes); take(4, (size_t)n + 8);
    const size_t head = htotal;
    TRY(reserve_host(c, c->h_an, head + 4096));
    i64 *totals = reinterpret_cast<i64 *>(c->h_an.p);       // (scratch until the results land)
    totals[0] = totals[1] = totals[2] = 0;
    unsigned long long *h_bad = reinterpret_cast<unsigned long long *>(c->h_an.p + 64);
    *h_bad = ~0ull;
    if (n > 0) {
        HIP_TRY(c, hipMemsetAsync(w_bad.p, 0xff, 8, s));
        const int g = grid_for(n, 256, 65536);
        hipLaunchKernelGGL(k_an_count, dim3(g), dim3(256), 0, s, a, o);
        hipLaunchKernelGGL(k_an_poly, dim3(grid_for(2 * n, 256, 65536)), dim3(256), 0, s, a, o);
        hipLaunchKernelGGL(k_an_scan1, dim3((unsigned)nb, 3), dim3(256), 0, s, o.cnt, o.poly, n, nb, w_bsum.p);
        hipLaunchKernelGGL(k_an_scan2, dim3(3), dim3(256), 0, s, nb, w_bsum.p);
        hipLaunchKernelGGL(k_an_scan3, dim3((unsigned)nb, 3), dim3(256), 0, s, o.cnt, o.poly, n, nb, w_bsum.p, o.off);
        for (int k = 0; k < 3; ++k) HIP_TRY(c, hipMemcpyAsync(&totals[k], o.off + (size_t)k * ((size_t)n + 1) + (size_t)n, sizeof(i64), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(s));
    }
    const i64 G = totals[0], C = totals[1], Pn = totals[2];
    DevBuf<int> o_gaps, o_clips, o_polys;
    DevBuf<unsigned> o_tok;
    Carve ov;
    ov.add(o_gaps, (size_t)G * 3); ov.add(o_clips, (size_t)C * 2); ov.add(o_polys, (size_t)Pn * 3); ov.add(o_tok, (size_t)(G + Pn));
    TRY(ensure(c, c->d_an_out, ov.total + 256));
    ov.bind(c->d_an_out.p);
    o.gaps = o_gaps.p; o.clips = o_clips.p; o.polys = o_polys.p; o.tok = o_tok.p;
    take(5, o_gaps.cap); take(6, o_clips.cap); take(7, o_polys.cap); take(8, o_tok.cap);
    TRY(reserve_host(c, c->h_an, htotal + 4096));
    char *h = c->h_an.p;
    if (n > 0) {
        hipLaunchKernelGGL(k_an_emit, dim3(grid_for(n, 256, 65536)), dim3(256), 0, s, a, o);
        HIP_TRY(c, hipGetLastError());
        unsigned long long *bad = reinterpret_cast<unsigned long long *>(h + htotal);
        HIP_TRY(c, hipMemcpyAsync(bad, w_bad.p, 8, hipMemcpyDeviceToHost, s));
        for (int k = 0; k < 3; ++k) HIP_TRY(c, hipMemcpyAsync(h + hoff[k], o.off + (size_t)k * ((size_t)n + 1), off_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h + hoff[3], o.tok_off, off_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h + hoff[4], o.tail, (size_t)n, hipMemcpyDeviceToHost, s));
        if (G) HIP_TRY(c, hipMemcpyAsync(h + hoff[5], o.gaps, o_gaps.cap, hipMemcpyDeviceToHost, s));
        if (C) HIP_TRY(c, hipMemcpyAsync(h + hoff[6], o.clips, o_clips.cap, hipMemcpyDeviceToHost, s));
        if (Pn) HIP_TRY(c, hipMemcpyAsync(h + hoff[7], o.polys, o_polys.cap, hipMemcpyDeviceToHost, s));
        if (G + Pn) HIP_TRY(c, hipMemcpyAsync(h + hoff[8], o.tok, o_tok.cap, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        if (*bad != ~0ull) {
            const i64 r = (i64)*bad;
            int code = 0;
            HIP_TRY(c, copy_sync(c, &code, o.status + r, 4, hipMemcpyDeviceToHost));
            return fail(c, FSEG_ERR_INPUT, "fseg_annotate: partition %d, read %lld: %s (reference: py/freddie_segment.py)", rd->read_part[r], (long long)r,
                        code > 0 && code < kAnCodes ? kAnMessages[code] : "unknown status");
        }
    } else {
        for (int k = 0; k < 4; ++k) *reinterpret_cast<i64 *>(h + hoff[k]) = 0;
    }
    fseg_annot &A = c->annot;
    A.n_read = n;
    A.gap_off = reinterpret_cast<const int64_t *>(h + hoff[0]); A.clip_off = reinterpret_cast<const int64_t *>(h + hoff[1]);
    A.poly_off = reinterpret_cast<const int64_t *>(h + hoff[2]); A.tok_off = reinterpret_cast<const int64_t *>(h + hoff[3]);
    A.tail = reinterpret_cast<const uint8_t *>(h + hoff[4]);
    A.gaps = reinterpret_cast<const int32_t *>(h + hoff[5]); A.clips = reinterpret_cast<const int32_t *>(h + hoff[6]);
    A.polys = reinterpret_cast<const int32_t *>(h + hoff[7]); A.tok = reinterpret_cast<const uint32_t *>(h + hoff[8]);
    c->have_annot = true;
    return FSEG_OK;
}

int32_t fseg_annotate(fseg_ctx *c, const fseg_reads *reads, const int64_t *label_off, const uint8_t *labels2,
                      const int64_t *part_final_off, const int32_t *final_pos) {
    return annotate_impl(c, reads, label_off, labels2, part_final_off, final_pos);
}

int32_t fseg_annotation(fseg_ctx *c, fseg_annot *out) {
    if (!c || !out) return FSEG_ERR_ARG;
    if (!c->have_annot) return fail(c, FSEG_ERR_ARG, "fseg_annotation: no completed fseg_annotate");
    *out = c->annot;
    return FSEG_OK;
}

int fseg_tap(fseg_ctx *c, int what, void *dst, int64_t cap_bytes, int64_t *n_bytes) {
    if (!c || !n_bytes) return FSEG_ERR_ARG;
    TRY(fseg_sync(c));
    if (!c->ran) return fail(c, FSEG_ERR_ARG, "no completed run");
    const Status &st = *c->h_status;
    auto from_dev = [&](const auto &buf, i64 n) -> int {     // n elements of a device buffer
        const i64 bytes = (i64)buf.bytes((size_t)n);
        *n_bytes = bytes;
        if (dst && cap_bytes > 0 && bytes > 0) HIP_TRY(c, copy_sync(c, dst, buf.p, (size_t)(bytes < cap_bytes ? bytes : cap_bytes), hipMemcpyDeviceToHost));
        return FSEG_OK;
    };
    auto from_host = [&](const void *words, size_t bytes) {  // a tap that the host puts together
        *n_bytes = (i64)bytes;
        if (dst && cap_bytes > 0) memcpy(dst, words, bytes < (size_t)cap_bytes ? bytes : (size_t)cap_bytes);
        return FSEG_OK;
    };
    switch (what) {
        case FSEG_TAP_POS_OFF: return from_dev(c->d_pos_off, c->batch.K + 1);
        case FSEG_TAP_Y_RAW: {                                             // int32 whatever the device holds: uint16 is widened here
            if (!c->batch.yraw_narrow) return from_dev(DevBuf<int32_t>{c->d_y_raw.as<int32_t>()}, c->batch.NPOS);
            const i64 bytes = (i64)DevBuf<int32_t>::bytes((size_t)c->batch.NPOS);
            *n_bytes = bytes;
            if (dst && cap_bytes > 0 && bytes > 0) {
                std::vector<uint16_t> narrow((size_t)c->batch.NPOS);
                HIP_TRY(c, copy_sync(c, narrow.data(), c->d_y_raw.p, narrow.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
                const i64 n = (bytes < cap_bytes ? bytes : cap_bytes) / (i64)sizeof(int32_t);
                for (i64 i = 0; i < n; ++i) static_cast<int32_t *>(dst)[i] = (int32_t)narrow[(size_t)i];
            }
            return FSEG_OK;
        }
        case FSEG_TAP_Y: return from_dev(c->d_y, c->batch.NPOS);
        case FSEG_TAP_THRESHOLD: return from_dev(c->d_thr, c->batch.n_part);
        case FSEG_TAP_CAND_OFF: return from_dev(c->d_cand_off, c->batch.K + 1);
        case FSEG_TAP_CAND_Y: return from_dev(c->d_cand_y, (i64)st.n_cand);
        case FSEG_TAP_FIXED: return from_dev(c->d_fixed, (i64)st.n_cand);
        case FSEG_TAP_CHOSEN: return from_dev(c->d_chosen, (i64)st.n_cand);
        case FSEG_TAP_FINAL_OFF: return from_dev(c->d_final_off, c->batch.K + 1);
        case FSEG_TAP_FINAL_Y: return from_dev(c->d_final_y, (i64)st.n_final);
        case FSEG_TAP_PROBLEMS: {                                          // a row per problem: interval, first candidate, candidates, chain
            const size_t n = (size_t)st.n_prob;
            const DevBuf<int> *cols[4] = {&c->d_prob_iv, &c->d_prob_start, &c->d_prob_n, &c->d_prob_chain};
            std::vector<int> col(n), rows(n * 4);
            for (int k = 0; k < 4 && n; ++k) {
                HIP_TRY(c, copy_sync(c, col.data(), cols[k]->p, bytes_of(*cols[k], n), hipMemcpyDeviceToHost));
                for (size_t i = 0; i < n; ++i) rows[4 * i + k] = col[i];
            }
            return from_host(rows.data(), rows.size() * sizeof(int));
        }
        case FSEG_TAP_LANE_START: return from_dev(c->d_lane_start, c->batch.LANES);
        case FSEG_TAP_LANE_PMAX: return from_dev(c->d_lane_pmax, c->batch.LANES);
        case FSEG_TAP_LANE_EXONS: return from_dev(c->d_lane_ex, c->batch.LANES);
        case FSEG_TAP_LANE_STREAM: return from_dev(c->d_lane_lx, c->batch.LANES);
        case FSEG_TAP_EXON_STREAM: return from_dev(c->d_lex, c->batch.I);
        case FSEG_TAP_SYNC: {
            SyncWords w{};
            HIP_TRY(c, copy_sync(c, &w, c->d_sync.p, sizeof w, hipMemcpyDeviceToHost));
            const int words[] = {(int)c->sync_gen, c->dev_sync ? 1 : 0, (int)w.emit_gen, (int)w.side_gen[0], (int)w.side_gen[1], (int)w.emit_ctr,
                                 (int)c->sync_timeouts, (int)c->forked_runs, (c->side_probed ? 8 : 0) | (c->side_ok[0] ? 1 : 0) | (c->side_ok[1] ? 2 : 0) | (c->side_ok[2] ? 4 : 0),
                                 (int)c->graph_captures};
            return from_host(words, sizeof words);
        }
        case FSEG_TAP_PATHS: return from_host(c->paths, sizeof c->paths);
        case FSEG_TAP_HIST_RANGES: {                                       // a row per histogram chunk: first position, positions, lane range
            const size_t n = (size_t)c->batch.n_hist_chunks;
            std::vector<i64> col(n), rows(n * 4);
            std::vector<int> cnt(n);
            const DevBuf<i64> *cols[3] = {&c->d_hc_p0, &c->d_hc_llo, &c->d_hc_lhi};
            for (int k = 0; k < 3 && n; ++k) {
                HIP_TRY(c, copy_sync(c, col.data(), cols[k]->p, bytes_of(*cols[k], n), hipMemcpyDeviceToHost));
                for (size_t i = 0; i < n; ++i) rows[4 * i + (k ? k + 1 : 0)] = col[i];
            }
            if (n) HIP_TRY(c, copy_sync(c, cnt.data(), c->d_hc_n.p, bytes_of(c->d_hc_n, n), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < n; ++i) rows[4 * i + 1] = cnt[i];
            return from_host(rows.data(), rows.size() * sizeof(i64));
        }
        default: return fail(c, FSEG_ERR_ARG, "unknown tap %d", what);
    }
}

int fseg_set_profiling(fseg_ctx *c, int on) {
    if (!c) return FSEG_ERR_ARG;
    c->shape.profiling = on != 0;
    c->shape.profile_all = on != 2;
    c->shape.profile_plain = on == 3;         // every stage bracketed on replays too: plain launches instead of the graph
    return FSEG_OK;
}
int fseg_n_stages(void) { return ST_REPORTED; }
const char *fseg_stage_name(int i) { return (i >= 0 && i < ST_REPORTED) ? kStageNames[i] : ""; }
int fseg_stage_ms(fseg_ctx *c, float *ms) {
    if (!c || !ms) return FSEG_ERR_ARG;
    TRY(fseg_sync(c));
    for (int i = 0; i < ST_REPORTED; ++i) ms[i] = c->stage_ms[i];
    return FSEG_OK;
}

#ifdef FSEG_SCORE_TIMING
int fseg_debug_score_timing(fseg_ctx *c, unsigned long long *out8) {
    if (!c || !out8 || !c->d_tacc.p) return FSEG_ERR_ARG;
    if (copy_sync(c, out8, c->d_tacc.p, 128, hipMemcpyDeviceToHost) != hipSuccess) return FSEG_ERR_HIP;   /* 16 slots */
    (void)hipMemsetAsync(c->d_tacc.p, 0, 120, c->stream); (void)hipStreamSynchronize(c->stream);   /* slot 15 = the k_solve class being timed: kept */
    return FSEG_OK;
}
int fseg_debug_prob_ticks(fseg_ctx *c, unsigned long long *out4, long long n_prob) {     /* 4 values per problem */
    if (!c || !out4 || n_prob < 0 || (size_t)n_prob > kTaccProbs) return FSEG_ERR_ARG;
    if (copy_sync(c, out4, reinterpret_cast<char *>(c->d_tacc.p) + 128, (size_t)n_prob * 32, hipMemcpyDeviceToHost) != hipSuccess) return FSEG_ERR_HIP;
    return FSEG_OK;
}
int fseg_debug_dp_ticks(fseg_ctx *c, unsigned long long *out4, long long n_prob) {       /* k_dpw's records: (ticks, -, -, start tick) */
    if (!c || !out4 || n_prob < 0 || (size_t)n_prob > kTaccProbs) return FSEG_ERR_ARG;
    if (copy_sync(c, out4, reinterpret_cast<char *>(c->d_tacc.p) + 128 + kTaccProbs * 32, (size_t)n_prob * 32, hipMemcpyDeviceToHost) != hipSuccess) return FSEG_ERR_HIP;
    return FSEG_OK;
}
int fseg_debug_timed_class(fseg_ctx *c, int cls) {
    unsigned long long v = (unsigned long long)(long long)cls;
    if (!c || copy_sync(c, reinterpret_cast<char *>(c->d_tacc.p) + 120, &v, 8, hipMemcpyHostToDevice) != hipSuccess) return FSEG_ERR_HIP;
    return FSEG_OK;
}
#endif

int64_t fseg_scoring_algorithmic_bytes(fseg_ctx *c) {
    if (!c || !c->ran) return -1;
    // per partition 4*(N_p + K_p)*R_p + 4*R_p, R_p = read reps
    std::vector<i64> co((size_t)c->batch.K + 1);
    if (copy_sync(c, co.data(), c->d_cand_off.p, bytes_of(c->d_cand_off, co.size()), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    i64 total = 0;
    for (int p = 0; p < c->batch.n_part; ++p) {
        i64 Np = co[(size_t)c->part_iv_off[p + 1]] - co[(size_t)c->part_iv_off[p]];
        i64 Kp = c->part_iv_off[p + 1] - c->part_iv_off[p];
        i64 Rp = c->part_rep_off[p + 1] - c->part_rep_off[p];
        total += 4 * (Np + Kp) * Rp + 4 * Rp;
    }
    return total;
}

}  // extern "C"

