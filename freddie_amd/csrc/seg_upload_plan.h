// seg_upload_plan.h -- what fseg_upload decides and derives on the host, as plain C++ (no HIP): plan_upload() validates a batch
// as read_split() asserts it and counts everything the input slab is carved from; fill_upload_tables() writes the small derived
// tables (position offsets, smoothing tiles, compaction blocks, rep blocks, histogram chunks).  Every table's element count is a
// member of the plan (UploadPlan::n): upload_impl carves the slab from those members and fill_upload_tables() writes exactly that
// many elements, so size and fill are stated once.  tools/upload_plan_host_check.cpp runs both without a GPU, every table
// allocated at exactly its count under the address sanitizer (tests/test_upload_plan_host.py restates the tables per position).
// The constants and TileDesc here are the ones the kernels read (seg_common.h includes this header).
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <utility>
#include <vector>

#include "freddie_seg.h"

namespace fseg {

typedef long long i64;
typedef unsigned long long u64;

constexpr int kSmoothShift = 9;
constexpr int kSmoothTile = 1 << kSmoothShift;   // positions per smoothing tile: intervals average ~1.5 K positions in many-partition
                                                 // batches, and a tile never spans two intervals -- 512 keeps the tiles ~95 % full
constexpr int kScanBlock = 8192;       // elements per scan workgroup (256 threads x one 32-bit word of flags): the Y > 0 values (k_scan_emit<kEmitValues>, k_voff)
// look-back state of the three compactions (values, candidates, final positions): scan_blocks(NPOS) words each, zeroed per run
inline i64 scan_blocks(i64 n) { return (n + kScanBlock - 1) / kScanBlock; }
constexpr int kPosBlock = 32768;       // positions per workgroup of a position compaction (256 threads x four words)
inline i64 pos_blocks(i64 n) { return (n + kPosBlock - 1) / kPosBlock; }
constexpr int kRepBlock = 256;         // reps per rep block (k_prep_reps, k_lane_blocks, k_label_reads: a thread per rep)

// S1's chunks: kHistChunk consecutive positions of one partition with 32-bit LDS counters ...
constexpr int kHistChunk = 8192;
// The same 32 KB of LDS as two 16-bit counters per word (k_hist<16>: position i of the chunk is half i & 1 of word i >> 1) hold twice
// the positions: half the chunks, so half the visits of a read that spans its partition, half the table stagings and barriers.
// A low half never carries into its neighbour because the host takes this instance only for batches in which no position's
// count can exceed 65 535 (plan_upload: hist_packed).
// Such a batch's histogram is uint16 in device memory as well (FSEG_YRAW16, default on): the write-out is then a copy of the LDS
// words.  For that the chunk's counters start at half-word p0 & 7 of the LDS array (p0: the chunk's first position in the batch), so
// 16-byte group j of the array is 16-byte group (p0 >> 3) + j of the histogram -- aligned on both sides -- and the array is one group
// longer.  Only a chunk's first and last group can hold a neighbouring chunk's positions: those leave as 2-byte stores.
#ifndef FSEG_HIST_CHUNK16
#define FSEG_HIST_CHUNK16 16384
#endif
constexpr int kHistChunk16 = FSEG_HIST_CHUNK16;
static_assert(kHistChunk16 % 8 == 0, "the packed counters are zeroed sixteen bytes at a time");
constexpr int kHistCountMax16 = 65535;
constexpr int kHistChunkMin = 1024, kHistWgsWanted = 512;   // chunks are halved down to the one while a batch gives fewer than the other

constexpr i64 kUploadLimit = 0x7fffffffLL;       // exons, positions, reads, tiles, chunks of one upload: below 2^31 - 1 (the kernels index them with int)

struct alignas(16) TileDesc {
    i64 base;       // position of the interval's first element (pos_off[interval])
    int y0;         // first position of the tile inside the interval
    int len;        // interval length
};

// the facts of the resident batch that the context keeps (fseg_ctx::batch)
struct BatchFacts {
    int n_part = 0;
    i64 K = 0, R = 0, I = 0, NPOS = 0, LANES = 0;     // intervals, reps, exons, positions, reads
    i64 max_part_pos = 0;      // positions of the batch's largest partition (k_thr_part takes partitions of up to kThrPartMaxChunks * 8192)
    i64 max_part_lanes = 0;    // reads of the batch's largest partition (what bounds a DP sum: 32-bit keys below 2^18)
    int n_tiles = 0, n_hist_chunks = 0, n_rep_blocks = 0;
    i64 max_rep_exons = 0;     // most exons of one rep
    bool expanded = false;     // some rep stands for more than one read
    bool hist_packed = false;  // the chunks were planned for k_hist<16> (kHistChunk16 positions, every count <= 65 535)
    bool yraw_narrow = false;  // d_y_raw holds uint16 (hist_packed and the switch): S1's output, S2's and S6's input
};

struct UploadPlan {
    int rc = FSEG_OK;          // a refusal: the code and the message of fseg_upload
    char msg[192] = "";
    BatchFacts batch;
    i64 max_part_reps = 0;     // reps of the largest partition (k_lanes sorts up to kLaneSortMax itself)
    int hist_chunk = 0;        // positions per histogram chunk
    i64 nb = 0, nbp = 0;       // scan_blocks(NPOS), pos_blocks(NPOS)
    std::vector<i64> part_pos, part_lanes;      // per partition: positions, reads
    // element counts of the uploaded tables: what the input slab is carved with and what fill_upload_tables() writes
    struct Counts {
        size_t part_off = 0;   // part_iv_off, part_rep_off, part_lane_off: n_part + 1
        size_t iv = 0;         // iv_start, iv_end, iv_part, iv_tile0: K
        size_t pos_off = 0;    // K + 1
        size_t tiles = 0;      // tile_desc
        size_t blk_iv0 = 0;    // nbp + 1
        size_t rep_blocks = 0; // rb_part, rb_r0 (and the device-derived rb_* arrays)
        size_t chunks = 0;     // hc_part, hc_p0, hc_n, hc_glo, hc_ghi (and hc_llo, hc_lhi)
    } n;
};

// host images of the thirteen derived tables, each of the plan's count
struct UploadTables {
    i64 *pos_off, *part_lane_off;      // n.pos_off, n.part_off
    int *iv_part, *iv_tile0;           // n.iv
    TileDesc *tile_desc;               // n.tiles
    int *blk_iv0;                      // n.blk_iv0
    int *rb_part, *rb_r0;              // n.rep_blocks
    int *hc_part; i64 *hc_p0; int *hc_n, *hc_glo, *hc_ghi;   // n.chunks
};

inline UploadPlan &refuse(UploadPlan &pl, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(pl.msg, sizeof pl.msg, fmt, ap);
    va_end(ap);
    pl.rc = code;
    return pl;
}

// The batch's validation at the partition / interval / rep level (as read_split() asserts it, :138-140) and every count of the
// upload, in one walk over the partitions' intervals and one over the reps.  hist16 / yraw16: the switches (0: never).
inline UploadPlan plan_upload(const fseg_batch &b, int hist16, int yraw16) {
    UploadPlan pl;
    BatchFacts &f = pl.batch;
    const int np = b.n_part;
    const i64 K = b.part_iv_off[np], R = b.part_rep_off[np];
    if (b.part_iv_off[0] != 0 || b.part_rep_off[0] != 0 || b.rep_exon_off[0] != 0)
        return refuse(pl, FSEG_ERR_ARG, "fseg_upload: offsets must start at 0");
    if (K <= 0 || R < 0) return refuse(pl, FSEG_ERR_ARG, "fseg_upload: bad offsets");
    const i64 I = b.rep_exon_off[R];
    if (I < 0) return refuse(pl, FSEG_ERR_ARG, "rep_exon_off not monotone");
    if (I >= kUploadLimit) return refuse(pl, FSEG_ERR_UNSUPPORTED, "batch has %lld exons; split it (limit 2^31-1 per upload)", (long long)I);
    i64 NPOS = 0, n_tiles = 0, lanes = 0, n_rep_blocks = 0;
    pl.part_pos.assign((size_t)np, 0); pl.part_lanes.assign((size_t)np, 0);
    for (int p = 0; p < np; ++p) {
        const i64 k0 = b.part_iv_off[p], k1 = b.part_iv_off[p + 1];
        if (k1 <= k0) return refuse(pl, FSEG_ERR_INPUT, "partition %d has no intervals", p);
        if (b.part_rep_off[p + 1] < b.part_rep_off[p]) return refuse(pl, FSEG_ERR_ARG, "part_rep_off not monotone");
        i64 pos = 0;
        for (i64 k = k0; k < k1; ++k) {
            if (!(b.iv_start[k] < b.iv_end[k])) return refuse(pl, FSEG_ERR_INPUT, "partition %d: interval with start >= end (py/freddie_segment.py:140)", p);
            if (k > k0 && !(b.iv_end[k - 1] < b.iv_start[k])) return refuse(pl, FSEG_ERR_INPUT, "partition %d: intervals overlap or are unordered (py/freddie_segment.py:138)", p);
            const i64 len = (i64)b.iv_end[k] - b.iv_start[k] + 1;       // an interval owns positions s..e inclusive (:652-659)
            pos += len;
            n_tiles += (len + kSmoothTile - 1) / kSmoothTile;
        }
        pl.part_pos[(size_t)p] = pos;
        NPOS += pos;
        f.max_part_pos = std::max(f.max_part_pos, pos);
        const i64 reps = b.part_rep_off[p + 1] - b.part_rep_off[p];
        n_rep_blocks += (reps + kRepBlock - 1) / kRepBlock;
        pl.max_part_reps = std::max(pl.max_part_reps, reps);
    }
    if (NPOS >= kUploadLimit) return refuse(pl, FSEG_ERR_UNSUPPORTED, "batch has %lld positions; split it (limit 2^31-1 per upload)", (long long)NPOS);
    for (i64 r = 0, p = 0; r < R; ++r) {
        const int w = b.rep_weight[r];
        if (w < 1) return refuse(pl, FSEG_ERR_INPUT, "rep %lld has weight %d (< 1)", (long long)r, w);
        if (w != 1) f.expanded = true;
        lanes += w;
        while (r >= b.part_rep_off[p + 1]) ++p;         // (part_rep_off ascends from 0 to R: checked above)
        pl.part_lanes[(size_t)p] += w;
        if (b.rep_exon_off[r + 1] < b.rep_exon_off[r]) return refuse(pl, FSEG_ERR_ARG, "rep_exon_off not monotone");
        f.max_rep_exons = std::max<i64>(f.max_rep_exons, b.rep_exon_off[r + 1] - b.rep_exon_off[r]);
    }
    if (lanes >= kUploadLimit) return refuse(pl, FSEG_ERR_UNSUPPORTED, "batch has %lld reads; split it (limit 2^31-1 per upload)", (long long)lanes);
    // S1's counter width.  The packed instance (two 16-bit counters per LDS word, chunks of twice the positions) is taken where no
    // position's count can exceed 65 535.  A read hits a position at most twice (an exon may end where the next begins), so a
    // partition of up to 32 767 lanes cannot get there -- every partition of an ordinary batch.  A larger one is counted here:
    // its reps' exon ends, sorted, each with its weight (ignore_ends only takes hits away).  One width per batch.
    f.hist_packed = hist16 != 0;
    for (int p = 0; p < np; ++p) {
        f.max_part_lanes = std::max(f.max_part_lanes, pl.part_lanes[(size_t)p]);
        if (!f.hist_packed || 2 * pl.part_lanes[(size_t)p] <= kHistCountMax16) continue;
        const i64 r0 = b.part_rep_off[p], r1 = b.part_rep_off[p + 1];
        std::vector<std::pair<int, int>> ends;
        ends.reserve((size_t)(2 * (b.rep_exon_off[r1] - b.rep_exon_off[r0])));
        for (i64 r = r0; r < r1; ++r)
            for (i64 e = b.rep_exon_off[r]; e < b.rep_exon_off[r + 1]; ++e) {
                ends.emplace_back(b.ex_ts[e], b.rep_weight[r]);
                ends.emplace_back(b.ex_te[e], b.rep_weight[r]);
            }
        std::sort(ends.begin(), ends.end());
        i64 count = 0;
        for (size_t i = 0; i < ends.size() && f.hist_packed; ++i) {
            count = (i > 0 && ends[i].first == ends[i - 1].first ? count : 0) + ends[i].second;
            if (count > kHistCountMax16) f.hist_packed = false;
        }
    }
    // The histogram's element in device memory follows: uint16 where the counters are (one width per batch, decided before the
    // position slab is carved), unless FSEG_YRAW16=0 keeps it int32.
    f.yraw_narrow = f.hist_packed && yraw16 != 0;
    // histogram chunks: consecutive positions of one partition; as large as possible (fewer reads are visited twice)
    // while still giving >= 512 workgroups
    pl.hist_chunk = f.hist_packed ? kHistChunk16 : kHistChunk;
    while (pl.hist_chunk > kHistChunkMin && NPOS / pl.hist_chunk < kHistWgsWanted) pl.hist_chunk >>= 1;
    i64 n_chunks = 0;
    for (int p = 0; p < np; ++p) n_chunks += (pl.part_pos[(size_t)p] + pl.hist_chunk - 1) / pl.hist_chunk;
    pl.nb = scan_blocks(NPOS); pl.nbp = pos_blocks(NPOS);
    if (n_tiles >= kUploadLimit || n_chunks >= kUploadLimit) return refuse(pl, FSEG_ERR_UNSUPPORTED, "batch too large");
    f.n_part = np; f.K = K; f.R = R; f.I = I; f.NPOS = NPOS; f.LANES = lanes;
    f.n_tiles = (int)n_tiles; f.n_hist_chunks = (int)n_chunks; f.n_rep_blocks = (int)n_rep_blocks;
    pl.n.part_off = (size_t)np + 1; pl.n.iv = (size_t)K; pl.n.pos_off = (size_t)K + 1; pl.n.tiles = (size_t)n_tiles;
    pl.n.blk_iv0 = (size_t)pl.nbp + 1; pl.n.rep_blocks = (size_t)n_rep_blocks; pl.n.chunks = (size_t)n_chunks;
    return pl;
}

// The derived tables of an accepted plan.  The cursors t / rb / ch / bq end at the plan's counts (the walk above counted with the
// same strides); what is written is t.tile_desc[0 .. n.tiles), t.blk_iv0[0 .. n.blk_iv0) and so on, nothing beyond.
inline void fill_upload_tables(const fseg_batch &b, const UploadPlan &pl, const UploadTables &t) {
    const int np = pl.batch.n_part;
    const i64 nbp = pl.nbp;
    t.pos_off[0] = 0; t.part_lane_off[0] = 0;
    i64 tile = 0, rb = 0, ch = 0, bq = 0;
    for (int p = 0; p < np; ++p) {
        const i64 k0 = b.part_iv_off[p], k1 = b.part_iv_off[p + 1];
        for (i64 k = k0; k < k1; ++k) {
            const i64 len = (i64)b.iv_end[k] - b.iv_start[k] + 1;
            t.iv_part[k] = p;
            t.pos_off[k + 1] = t.pos_off[k] + len;
            t.iv_tile0[k] = (int)tile;
            for (i64 y = 0; y < len; y += kSmoothTile) t.tile_desc[tile++] = TileDesc{t.pos_off[k], (int)y, (int)len};
            // interval of the first position of every block of the position compactions
            for (; bq < nbp && bq * kPosBlock < t.pos_off[k + 1]; ++bq) t.blk_iv0[bq] = (int)k;
        }
        for (i64 r = b.part_rep_off[p]; r < b.part_rep_off[p + 1]; r += kRepBlock) { t.rb_part[rb] = p; t.rb_r0[rb] = (int)r; ++rb; }
        t.part_lane_off[p + 1] = t.part_lane_off[p] + pl.part_lanes[(size_t)p];
        // histogram chunks of the partition, with the genomic position of the chunk's first and last position (a
        // chunk may span several intervals of its partition)
        const i64 P0 = t.pos_off[k0], P1 = P0 + pl.part_pos[(size_t)p];
        i64 k = k0;
        for (i64 q0 = P0; q0 < P1; q0 += pl.hist_chunk) {
            const i64 q1 = std::min<i64>(q0 + pl.hist_chunk, P1) - 1;
            while (t.pos_off[k + 1] <= q0) ++k;
            i64 kk = k;
            while (t.pos_off[kk + 1] <= q1) ++kk;
            t.hc_part[ch] = p; t.hc_p0[ch] = q0; t.hc_n[ch] = (int)(q1 - q0 + 1);
            t.hc_glo[ch] = b.iv_start[k] + (int)(q0 - t.pos_off[k]);
            t.hc_ghi[ch] = b.iv_start[kk] + (int)(q1 - t.pos_off[kk]);
            ++ch;
        }
    }
    t.blk_iv0[nbp] = (int)(pl.batch.K - 1);
}

}  // namespace fseg
