// freddie_cluster.hip -- gfx950 kernels + C-ABI (include/freddie_cluster.h) for the pre-ILP work of the clustering
// stage: the pairwise read-compatibility graph of partition_reads() (py/freddie_cluster.py:217-234) and its iterated
// edge pruning (:240-255), for a batch of tints per call; and, behind the pruned graph on the device, the rest of the function
// (fclu_partition): connected components (:256-257), the even split (:258-260) and the incompatible rep pairs (:261-273).
// In front of the graph (fclu_preprocess, fclu_partition_reads): preprocess_ilp()'s per-rep I / C / FL (:285-310) from label rows at two
// bits a label, and the dedupe of reps with the same structure (:203-215); the unique rows go to the graph without leaving the device.
//
// Reads are bit rows (bit s = the read covers segment s), so the reference's two list comprehensions over the
// overlap [f, l] (:229, :232) become popcounts of (a & b & mask) and ((a ^ b) & mask).  The graph is a symmetric
// bit matrix; a 64 x 64 tile of it is one workgroup's unit of work, lane = column, so a row's 64 edge bits are one
// wave ballot and one 8-byte store.  Pruning keeps an edge when either end has no other neighbour or the two ends
// share a neighbour (:247-251): the columns that share a neighbour with row r are the OR of the rows of r's
// neighbours, one wave per row; every pass reads the previous pass' matrix only (the reference removes the edges
// of a pass together, :252) and passes repeat until one removes nothing (:254).
// The file, in order:  1. the kernels, stage by stage
//   2. Buf<T> (typed, owning, growing memory) and fclu_ctx, whose buffers free themselves
//   3. helpers: fail / HIP_TRY, the test knobs (read_knobs, once a call), run_burst, fetch
//   4. the stages: stage_tints, compat_run; part_* behind partition_device; the dedupe, once (describe_rows, dedupe_classes,
//      dedupe_members, report_row_errors) for prep_* behind preprocess_device and for group_device; round_* behind round_device
//   5. the C ABI, one extern "C" block
#include "freddie_cluster.h"

#include <hip/hip_runtime.h>

#include "clu_incumbent.h"   // (behind the runtime: its functions are __host__ __device__)
#include "clu_exact.h"
#include "clu_bnb.h"
#include "clu_bnb_wide.h"
#include "clu_readout.h"
#include "clu_plan.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

typedef long long i64;
typedef unsigned long long u64;

constexpr int kTile = 64;           // rows and columns per tile
constexpr int kMaxWords = 300;      // uint32 words per read row the LDS staging of k_compat can hold (9600 segments)

struct TintDesc {
    i64 row0, bits_off, adj_off;
    int n, n_seg, w, aw;            // rows, segments, uint32 words per read row, uint64 words per adjacency row
    int in_lds;                     // the tint's pruning runs whole in one workgroup's LDS (k_prune_lds): the per-pass kernels skip its rows
    int cc_lds;                     // the same for its connected components (k_cc_lds)
};

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// bits [f, l] of the 32-bit word number w (f <= l, both inside the row)
__device__ __forceinline__ unsigned range_mask(int f, int l, int w) {
    const int lo = f - w * 32, hi = l - w * 32;
    unsigned m = 0xffffffffu;
    if (lo > 0) m &= 0xffffffffu << lo;
    if (hi < 31) m &= 0xffffffffu >> (31 - hi);
    return m;
}

// ---- pairwise compatibility (py/freddie_cluster.py:217-234) ------------------------------------------------------
// The relation is symmetric, so only the tiles on and above the diagonal are computed: a workgroup writes its tile's rows (a
// row's 64 edge bits are one ballot) AND the transposed tile (lane = column keeps its own bit of every row; the waves' sixteen
// rows each meet in LDS).
// RANK (rows of at most kRankWords words): besides the bit rows, the number of a row's bits in front of each of its words is
// staged (16 bits each; as 8-byte entries {word, rank} the big tint ran at two workgroups per CU instead of three and
// took 3.0 instead of 2.0 ms).  A read's bits lie inside [first, last] (checked on the host), so over the pair's overlap [f, l]
//   same = popcount(a & b) over the overlap's words, no mask (a & b has no bit outside [f, l]);
//   diff = bits of a in [f, l] + bits of b in [f, l] - 2 same, and "bits of a in [f, l]" is the ranks of the overlap's first and
//          last word and two masked popcounts of those words -- which the sum over the overlap reads anyway.
// Most overlaps lie in one or two words: the first and the last word are taken outside the loop (four LDS reads a pair), the
// loop runs over what lies between (its trip count is the longest overlap of the wave's 64 pairs).
// !RANK: longer rows (up to kMaxWords): both sums with a range mask per word.
constexpr int kRankWords = 207;     // (64 + 64) rows x (4 + 2) bytes x 207 words + the static arrays <= 160 KB of LDS

template <bool RANK>
__global__ void __launch_bounds__(256) k_compat(int n_tiles, const int4 *tiles, const TintDesc *tints, const unsigned *bits,
                                                const int *first, const int *last, const unsigned char *tail, u64 *adj) {
    extern __shared__ unsigned lds[];
    __shared__ int row_f[kTile], row_l[kTile], row_t[kTile];
    __shared__ unsigned col_part[4][kTile];
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int ti = blockIdx.x; ti < n_tiles; ti += gridDim.x) {
        const int4 tile = tiles[ti];
        const TintDesc d = tints[tile.x];
        const int W = d.w, Wp = W | 1;                  // odd row stride: lanes reading the same word of 64 rows spread over the banks
        unsigned *rows = lds, *cols = lds + kTile * Wp;
        unsigned short *rrank = reinterpret_cast<unsigned short *>(cols + kTile * Wp), *crank = rrank + kTile * Wp;
        const unsigned *B = bits + d.bits_off;
        const int r0 = tile.y * kTile, c0 = tile.z * kTile;
        __syncthreads();
        {
            const float inv_w = 1.0f / (float)W;        // x / W for x < 64 * kMaxWords: a float quotient and one correction
            for (int x = threadIdx.x; x < kTile * W; x += blockDim.x) {
                int q = (int)((float)x * inv_w), w = x - q * W;
                if (w >= W) { ++q; w -= W; } else if (w < 0) { --q; w += W; }
                rows[q * Wp + w] = r0 + q < d.n ? B[(i64)(r0 + q) * W + w] : 0u;
                cols[q * Wp + w] = c0 + q < d.n ? B[(i64)(c0 + q) * W + w] : 0u;
            }
        }
        // the tile's rows' first / last covered segment and tail, staged with the bit rows (round 5): the row loop below read them
        // from global memory, three wave-uniform loads in front of every row's 64 pairs -- a microsecond of latency per row
        if (threadIdx.x < kTile) {
            const int row = r0 + threadIdx.x;
            const bool ok = row < d.n;
            row_f[threadIdx.x] = ok ? first[d.row0 + row] : 0;
            row_l[threadIdx.x] = ok ? last[d.row0 + row] : -1;
            row_t[threadIdx.x] = ok ? tail[d.row0 + row] : 0;
        }
        __syncthreads();
        if (RANK) {
            if (threadIdx.x < 2 * kTile) {              // a thread per staged row: the bits in front of each of its words
                const unsigned *src = (threadIdx.x < kTile ? rows : cols) + (threadIdx.x & (kTile - 1)) * Wp;
                unsigned short *dst = (threadIdx.x < kTile ? rrank : crank) + (threadIdx.x & (kTile - 1)) * Wp;
                unsigned run = 0;
                for (int w = 0; w < W; ++w) { dst[w] = (unsigned short)run; run += __popc(src[w]); }
            }
            __syncthreads();
        }
        const int col = c0 + lane;
        const bool col_ok = col < d.n;
        int f2 = 0, l2 = -1, t2 = 0;
        if (col_ok) { f2 = first[d.row0 + col]; l2 = last[d.row0 + col]; t2 = tail[d.row0 + col]; }
        const unsigned *b = cols + lane * Wp;
        const unsigned short *rb = crank + lane * Wp;
        unsigned mine = 0;                               // this column's edge bits of the wave's sixteen rows
        for (int k = 0; k < kTile / 4; ++k) {
            const int rr = wave * (kTile / 4) + k, row = r0 + rr;
            if (row >= d.n) break;
            const int f1 = row_f[rr], l1 = row_l[rr], t1 = row_t[rr];
            const int f = f1 > f2 ? f1 : f2, l = l1 < l2 ? l1 : l2;         // overlap of the two reads (:224-226)
            const int o = l - f + 1;
            bool edge = false;
            // poly-A tails on different ends: incompatible (:222-223); f < 0 only when neither read covers any segment: then no
            // common segment either (:228-230).  (Straight-line code that computes every pair and drops the untested ones at the
            // end was slower: whole waves skip here -- 0.168 against 0.151 ms on 400 tints of 500 reads.)
            if (col_ok && col != row && !(t1 != 0 && t2 != 0 && t1 != t2) && o >= 1 && f >= 0) {
                const unsigned *a = rows + rr * Wp;
                int same = 0, diff = 0;
                if (RANK) {
                    const unsigned short *ra = rrank + rr * Wp;
                    const int wf = f >> 5, wl = l >> 5;
                    const unsigned a0 = a[wf], a1 = a[wl], b0 = b[wf], b1 = b[wl];
                    same = __popc(a0 & b0);                                             // segments both reads cover (:229)
                    if (wl > wf) {
                        same += __popc(a1 & b1);
                        for (int w = wf + 1; w < wl; ++w) same += __popc(a[w] & b[w]);
                    }
                    const unsigned below_f = (1u << (f & 31)) - 1u, upto_l = 0xffffffffu >> (31 - (l & 31));
                    const int in_a = (int)ra[wl] + __popc(a1 & upto_l) - (int)ra[wf] - __popc(a0 & below_f);
                    const int in_b = (int)rb[wl] + __popc(b1 & upto_l) - (int)rb[wf] - __popc(b0 & below_f);
                    diff = in_a + in_b - 2 * same;                                      // segments where they differ (:232)
                } else {
                    for (int w = f >> 5; w <= (l >> 5); ++w) {
                        const unsigned m = range_mask(f, l, w), x = a[w], y = b[w];
                        same += __popc(x & y & m);           // segments both reads cover (:229)
                        diff += __popc((x ^ y) & m);         // segments where they differ (:232)
                    }
                }
                edge = same >= 1 && ((o > 3 && diff < 3) || (o <= 3 && diff == 0));   // :230, :234
            }
            const u64 word = __ballot(edge);
            if (lane == 0) adj[d.adj_off + (i64)row * d.aw + tile.z] = word;
            mine |= (unsigned)edge << k;
        }
        if (tile.y != tile.z) {                          // (workgroup-uniform) the tile below the diagonal: this one transposed
            col_part[wave][lane] = mine;
            __syncthreads();
            if (threadIdx.x < kTile && col_ok)
                adj[d.adj_off + (i64)col * d.aw + tile.y] = (u64)col_part[0][lane] | ((u64)col_part[1][lane] << 16) |
                                                            ((u64)col_part[2][lane] << 32) | ((u64)col_part[3][lane] << 48);
        }
    }
}

// ---- degrees ---------------------------------------------------------------------------------------------------
// `gate` (all three kernels of a pass): the "some edge was removed" word of the PREVIOUS pass, or null for the first pass of
// a burst.  The host enqueues several passes back to back and reads the flags once per burst; the passes after the one that
// removed nothing find their gate at zero and return at once (py/freddie_cluster.py:240-255 loops until nothing changes).
__global__ void __launch_bounds__(256) k_degree(i64 n_rows_total, const int *row_tint, const TintDesc *tints, const u64 *adj, int *deg,
                                                const int *gate) {
    if (gate && *gate == 0) return;
    const int lane = lane_id();
    const i64 wave_g = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((i64)gridDim.x * blockDim.x) >> 6;
    for (i64 r = wave_g; r < n_rows_total; r += n_waves) {
        const TintDesc d = tints[row_tint[r]];
        if (d.in_lds) continue;
        const u64 *a = adj + d.adj_off + (r - d.row0) * d.aw;
        int c = 0;
        for (int w = lane; w < d.aw; w += 64) c += __popcll(a[w]);
        for (int s = 32; s >= 1; s >>= 1) c += __shfl_xor(c, s);
        if (lane == 0) deg[r] = c;
    }
}

// ---- one pruning pass (py/freddie_cluster.py:243-252) ------------------------------------------------------------
// new(r, c) = old(r, c) and (deg r == 1 or deg c == 1 or r and c share a neighbour).
// "r and c share a neighbour" for all c at once: H(r) = OR of the rows of r's neighbours (the matrix is symmetric, so
// bit c of neighbour k's row says k ~ c).  One wave per row, lanes = 64 consecutive words of the row, the loop runs over
// the set bits of row r (wave-uniform) and ORs the neighbour's words (a coalesced read of the neighbour's row): the
// work is sum(deg) * words instead of one LDS-staged 64 x 64 block pair per tile of the matrix.
__global__ void __launch_bounds__(256) k_deg1(int n_words_total, const int2 *word_tint, const TintDesc *tints, const int *deg, u64 *deg1,
                                              const int *gate) {
    if (gate && *gate == 0) return;
    // deg1[tint word z] bit c = column 64 z + c has exactly one neighbour
    const int lane = lane_id();
    const i64 wave_g = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((i64)gridDim.x * blockDim.x) >> 6;
    for (i64 x = wave_g; x < n_words_total; x += n_waves) {
        const int2 wt = word_tint[x];                    // (tint, word index inside the tint)
        const TintDesc d = tints[wt.x];
        if (d.in_lds) continue;
        const int col = wt.y * 64 + lane;
        const u64 m = __ballot(col < d.n && deg[d.row0 + col] == 1);
        if (lane == 0) deg1[x] = m;
    }
}
// The same pass, edge by edge (round 6; rows of at most kEdgeChunks x 64 words = 32 768 reads): only the columns c that ARE neighbours
// of r need an answer, and "r and c share a neighbour" is "row r AND row c is not empty" (the matrix is symmetric).  A wave takes a row,
// keeps it in registers (lane = word, kEdgeChunks words a lane), walks its set bits in order and for each neighbour c reads row c 64 words
// at a time until a word of the AND is not zero -- in these graphs (reads of one gene: triangles everywhere) the first 512 bytes nearly
// always answer, where the OR of all of N(r)'s rows (k_prune below) reads every row whole, once per 64-word chunk of the output:
// 19 539 reads, mean degree 239: 8.7 -> ~2 ms a pass.  Removed bits are cleared in the lane that holds their word.
constexpr int kEdgeChunks = 8;

__global__ void __launch_bounds__(256) k_prune_edges(i64 n_rows_total, int max_chunks, const int *row_tint, const TintDesc *tints, const u64 *old_adj, const int *deg,
                                                     u64 *new_adj, int *changed /* per tint */, int *pass_any, const int *gate) {
    if (gate && *gate == 0) return;
    const int lane = lane_id();
    const i64 wave_g = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((i64)gridDim.x * blockDim.x) >> 6;
    // a work item = (row r, 64-word chunk qc of it): the wave tests the neighbours whose bits lie in that chunk and writes that chunk of
    // the new row.  (A wave per ROW ended with its longest rows: degrees reach 7 000 where the mean is 239.)
    for (i64 item = wave_g; item < n_rows_total * max_chunks; item += n_waves) {
        const i64 r = item / max_chunks;
        const int qc = (int)(item - r * max_chunks);
        const int t = row_tint[r];
        const TintDesc d = tints[t];
        if (d.in_lds) continue;
        const u64 *A = old_adj + d.adj_off;
        const i64 rl = r - d.row0;
        const int aw = d.aw, n_chunks = (aw + 63) >> 6;
        if (qc >= n_chunks) continue;
        u64 mine[kEdgeChunks];
#pragma unroll
        for (int q = 0; q < kEdgeChunks; ++q) { const int z = q * 64 + lane; mine[q] = (q < n_chunks && z < aw) ? A[rl * aw + z] : 0ull; }
        u64 own = 0;                                          // this item's chunk of the row
#pragma unroll
        for (int q = 0; q < kEdgeChunks; ++q) if (q == qc) own = mine[q];
        u64 keep = own;
        const int deg_r = deg[r];
        bool any_change = false;
        if (deg_r > 1) {                                       // (deg 1: the edge stays; deg 0: nothing to do)
            // Neighbours are taken FOUR at a time: their degrees and the first 64 words of their rows are asked for together and
            // looked at afterwards -- one neighbour at a time the walk was a chain of two dependent loads (~1 us) per neighbour.
            i64 bc[4] = {0, 0, 0, 0}; int bl[4] = {0, 0, 0, 0}, bb[4] = {0, 0, 0, 0};
            int cnt = 0;
            auto flush = [&]() {
                int dg[4]; u64 cw[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) dg[u] = deg[d.row0 + bc[u < cnt ? u : 0]];
#pragma unroll
                for (int u = 0; u < 4; ++u) cw[u] = lane < aw ? A[bc[u < cnt ? u : 0] * aw + lane] : 0ull;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (u >= cnt) break;
                    bool stays = dg[u] == 1;
                    if (!stays) stays = __ballot((cw[u] & mine[0]) != 0ull) != 0ull;
                    if (!stays) {
                        const u64 *C = A + bc[u] * aw;
#pragma unroll
                        for (int q2 = 1; q2 < kEdgeChunks; ++q2) {
                            if (q2 >= n_chunks) break;
                            const int z = q2 * 64 + lane;
                            const u64 w2 = z < aw ? C[z] : 0ull;
                            if (__ballot((w2 & mine[q2]) != 0ull)) { stays = true; break; }
                        }
                    }
                    if (!stays) { if (lane == bl[u]) keep &= ~(1ull << bb[u]); any_change = true; }
                }
                cnt = 0;
            };
            u64 have = __ballot(own != 0ull);                  // the lanes whose word of this chunk holds a neighbour
            while (have) {
                const int L = __builtin_amdgcn_readfirstlane(__ffsll((long long)have) - 1);     // (wave-uniform: a scalar for readlane)
                have &= have - 1;
                u64 word = ((u64)(unsigned)__builtin_amdgcn_readlane((int)(own >> 32), L) << 32) | (u64)(unsigned)__builtin_amdgcn_readlane((int)own, L);
                while (word) {
                    const int b = __builtin_amdgcn_readfirstlane(__ffsll((long long)word) - 1);
                    word &= word - 1;
                    // (the newest neighbour enters at slot 0 and the others move up: static register indices, no scratch; the order
                    // inside a batch does not matter)
#pragma unroll
                    for (int u = 3; u > 0; --u) { bc[u] = bc[u - 1]; bl[u] = bl[u - 1]; bb[u] = bb[u - 1]; }
                    bc[0] = ((i64)qc * 64 + L) * 64 + b; bl[0] = L; bb[0] = b;                 // the neighbour (wave-uniform)
                    if (++cnt == 4) flush();
                }
            }
            if (cnt) flush();
        }
        { const int z = qc * 64 + lane; if (z < aw) new_adj[d.adj_off + rl * aw + z] = keep; }
        if (any_change && lane == 0) { changed[t] = 1; *pass_any = 1; }
    }
}

__global__ void __launch_bounds__(256) k_prune(i64 n_rows_total, const int *row_tint, const TintDesc *tints, const i64 *tint_word0,
                                               const u64 *old_adj, const int *deg, const u64 *deg1, u64 *new_adj,
                                               int *changed /* per tint */, int *pass_any, const int *gate) {
    if (gate && *gate == 0) return;
    const int lane = lane_id();
    const i64 wave_g = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((i64)gridDim.x * blockDim.x) >> 6;
    for (i64 r = wave_g; r < n_rows_total; r += n_waves) {
        const int t = row_tint[r];
        const TintDesc d = tints[t];
        if (d.in_lds) continue;
        const u64 *A = old_adj + d.adj_off;
        const i64 rl = r - d.row0;
        const int deg_r = deg[r];
        const u64 *d1 = deg1 + tint_word0[t];
        bool any_change = false;
        for (int z0 = 0; z0 < d.aw; z0 += 64) {
            const int z = z0 + lane;
            const bool zin = z < d.aw;
            const u64 oldw = zin ? A[rl * d.aw + z] : 0ull;
            u64 keep = ~0ull;
            if (deg_r != 1) {                            // wave-uniform
                u64 acc = 0;
                for (int wi = 0; wi < d.aw; ++wi) {
                    u64 word = A[rl * d.aw + wi];        // the same address in every lane
                    while (word) {
                        const int k = wi * 64 + __ffsll((long long)word) - 1;
                        word &= word - 1;
                        acc |= A[(i64)k * d.aw + (zin ? z : 0)];
                    }
                }
                keep = acc | (zin ? d1[z] : 0ull);
            }
            const u64 neww = oldw & keep;
            if (zin) new_adj[d.adj_off + rl * d.aw + z] = neww;
            any_change |= neww != oldw;
        }
        if (__ballot(any_change) && lane == 0) { changed[t] = 1; *pass_any = 1; }
    }
}

// ---- the whole pruning of a small tint by ONE workgroup, in LDS (round 6) ------------------------------------------
// A tint whose bit matrix fits LDS twice (rows x words <= kPruneLdsWords: 500 reads are 32 KB a copy) is pruned to its fixed point
// without leaving the workgroup: degrees, the "exactly one neighbour" column mask, one pass into the other copy, again until a pass
// removes nothing (:240-255) -- no launch per pass, no flags to the host, no pass over tints that are already done.  The per-pass
// kernels above are what tints too large for this use (and they skip the rows of the tints that are not theirs).
// A thread owns (row r, word z) pairs: new = old & (deg r == 1 ? all : H(r)[z] | deg1[z]) with H(r) = OR of the rows of r's
// neighbours; only the bits of old[r][z] that are not excused by deg1 need a common neighbour, and the walk over r's neighbours
// ends as soon as they all have one (in these graphs -- reads of one gene -- after a handful of neighbours).
constexpr int kPruneLdsWords = 7808;       // u64 words of one copy: 2 x 61 KB, two such workgroups share a CU's LDS with room for the rest

__global__ void __launch_bounds__(256) k_prune_lds(const int *small_tints, const TintDesc *tints, u64 *adj0, u64 *adj1, int *rounds) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    __shared__ int s_changed;
    const int t = small_tints[blockIdx.x];
    const TintDesc d = tints[t];
    const int n = d.n, aw = d.aw, nw = n * aw;
    u64 *buf[2] = {reinterpret_cast<u64 *>(lds_raw), reinterpret_cast<u64 *>(lds_raw) + nw};
    u64 *d1 = buf[1] + nw;
    unsigned short *deg = reinterpret_cast<unsigned short *>(d1 + aw);
    for (int x = threadIdx.x; x < nw; x += blockDim.x) buf[0][x] = adj0[d.adj_off + x];
    __syncthreads();
    int cur = 0, n_rounds = 0;
    for (;;) {
        const u64 *old = buf[cur];
        u64 *nxt = buf[cur ^ 1];
        for (int r = threadIdx.x; r < n; r += blockDim.x) {
            int c = 0;
            for (int z = 0; z < aw; ++z) c += __popcll(old[r * aw + z]);
            deg[r] = (unsigned short)c;
        }
        if (threadIdx.x == 0) s_changed = 0;
        __syncthreads();
        for (int z = threadIdx.x; z < aw; z += blockDim.x) {
            u64 m = 0;
            for (int b = 0; b < 64; ++b) { const int col = z * 64 + b; if (col < n && deg[col] == 1) m |= 1ull << b; }
            d1[z] = m;
        }
        __syncthreads();
        bool ch = false;
        for (int x = threadIdx.x; x < nw; x += blockDim.x) {
            const int r = x / aw, z = x - r * aw;
            const u64 oldw = old[x];
            u64 neww = oldw;
            if (oldw && deg[r] != 1) {
                const u64 need = oldw & ~d1[z];                 // these bits stay only with a common neighbour
                u64 acc = 0;
                for (int wi = 0; wi < aw && (need & ~acc); ++wi) {
                    u64 word = old[r * aw + wi];
                    while (word && (need & ~acc)) {
                        const int k = wi * 64 + __ffsll((long long)word) - 1;
                        word &= word - 1;
                        acc |= old[k * aw + z];
                    }
                }
                neww = oldw & (acc | d1[z]);
            }
            nxt[x] = neww;
            ch |= neww != oldw;
        }
        if (ch) s_changed = 1;
        __syncthreads();
        const int any = s_changed;
        __syncthreads();                                        // (everybody has read the flag before the next pass clears it)
        cur ^= 1;
        if (!any) break;
        ++n_rounds;
    }
    for (int x = threadIdx.x; x < nw; x += blockDim.x) { const u64 v = buf[cur][x]; adj0[d.adj_off + x] = v; adj1[d.adj_off + x] = v; }
    if (threadIdx.x == 0) rounds[t] = n_rounds;
}

// ================================================================================================================
// The rest of partition_reads() (py/freddie_cluster.py:256-274) on the pruned matrix, where the pruning left it.
// ================================================================================================================
// ---- connected components (:256-257) -------------------------------------------------------------------------
// parent[] over the rows of the whole batch (global row indices; a row starts as its own parent).  A pass is
//   hook:  m = the smallest parent among v's neighbours; when m < parent[v], both parent[v] and parent[parent[v]] take m (atomic min)
//   jump:  parent[v] = the root of v's chain (follow parent until it stops moving)
// and passes repeat until one changes nothing (hooking plus pointer jumping in the style of Shiloach-Vishkin / FastSV: a path of
// 1 000 nodes takes about ten passes, where neighbour-minimum propagation alone takes 1 000).  Every value a parent ever holds is a
// node of v's own component that is no larger than v, and values only fall; so a read that races with a write sees an older, larger,
// still valid value, and the one state in which a pass changes nothing is parent[v] = the smallest node of v's component: its
// label, which orders the components as networkx yields them (by first node).
__global__ void __launch_bounds__(256) k_cc_init(i64 n_rows_total, int *parent) {
    for (i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows_total; r += (i64)gridDim.x * blockDim.x) parent[r] = (int)r;
}

// `gate`: as in the pruning passes, the "something changed" word of the previous pass of the burst.
__global__ void __launch_bounds__(256) k_cc_hook(i64 n_rows_total, const int *row_tint, const TintDesc *tints, const u64 *adj, int *parent,
                                                 int *pass_any, const int *gate) {
    if (gate && *gate == 0) return;
    const int lane = lane_id();
    const i64 wave_g = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((i64)gridDim.x * blockDim.x) >> 6;
    for (i64 r = wave_g; r < n_rows_total; r += n_waves) {
        const TintDesc d = tints[row_tint[r]];
        if (d.cc_lds) continue;
        const u64 *a = adj + d.adj_off + (r - d.row0) * d.aw;
        const int pv = parent[r];
        int m = pv;
        for (int z = lane; z < d.aw; z += 64) {
            u64 word = a[z];
            while (word) {
                const int u = z * 64 + __ffsll((long long)word) - 1;
                word &= word - 1;
                const int pu = parent[d.row0 + u];
                m = pu < m ? pu : m;
            }
        }
        for (int s = 32; s >= 1; s >>= 1) { const int o = __shfl_xor(m, s); m = o < m ? o : m; }
        if (lane == 0 && m < pv) { atomicMin(&parent[pv], m); atomicMin(&parent[r], m); *pass_any = 1; }
    }
}

__global__ void __launch_bounds__(256) k_cc_jump(i64 n_rows_total, const int *row_tint, const TintDesc *tints, int *parent, int *pass_any,
                                                 const int *gate) {
    if (gate && *gate == 0) return;
    for (i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows_total; r += (i64)gridDim.x * blockDim.x) {
        if (tints[row_tint[r]].cc_lds) continue;
        const int p0 = parent[r];
        int p = p0, q = parent[p];
        while (q != p) { p = q; q = parent[p]; }          // (strictly falling: it ends at a root)
        if (p != p0) { parent[r] = p; *pass_any = 1; }
    }
}

// A tint whose matrix fits one workgroup's LDS (the pruning's own criterion, kPruneLdsWords): the same passes by one workgroup, to the
// end, with no flag to the host.
__global__ void __launch_bounds__(256) k_cc_lds(const int *small_tints, const TintDesc *tints, const u64 *adj, int *parent) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    __shared__ int s_changed;
    const TintDesc d = tints[small_tints[blockIdx.x]];
    const int n = d.n, aw = d.aw, nw = n * aw;
    u64 *A = reinterpret_cast<u64 *>(lds_raw);
    int *par = reinterpret_cast<int *>(A + nw);
    for (int x = threadIdx.x; x < nw; x += blockDim.x) A[x] = adj[d.adj_off + x];
    for (int v = threadIdx.x; v < n; v += blockDim.x) par[v] = v;
    for (;;) {
        if (threadIdx.x == 0) s_changed = 0;
        __syncthreads();
        for (int v = threadIdx.x; v < n; v += blockDim.x) {
            const int pv = par[v];
            int m = pv;
            for (int z = 0; z < aw; ++z) {
                u64 word = A[v * aw + z];
                while (word) {
                    const int u = z * 64 + __ffsll((long long)word) - 1;
                    word &= word - 1;
                    const int pu = par[u];
                    m = pu < m ? pu : m;
                }
            }
            if (m < pv) { atomicMin(&par[pv], m); atomicMin(&par[v], m); s_changed = 1; }
        }
        __syncthreads();
        for (int v = threadIdx.x; v < n; v += blockDim.x) {
            const int p0 = par[v];
            int p = p0, q = par[p];
            while (q != p) { p = q; q = par[p]; }
            if (p != p0) { par[v] = p; s_changed = 1; }
        }
        __syncthreads();
        const int any = s_changed;
        __syncthreads();                                        // (everybody has read the flag before the next pass clears it)
        if (!any) break;
    }
    for (int v = threadIdx.x; v < n; v += blockDim.x) parent[d.row0 + v] = (int)d.row0 + par[v];
}

// ---- even split of the components (:258-260, split_list_evenly :112-116) -----------------------------------------
// The rows of the batch, sorted (stable) by their label, are the partitions' node lists laid end to end: tints in order, in a tint
// the components by their smallest node, in a component the nodes ascending, and a chunk is a run of s of them.  skey / sval = label
// and row at sorted position k.  A label is its component's smallest row, so it is also the row at the component's first position.
__global__ void __launch_bounds__(256) k_bounds(i64 n_rows_total, const unsigned *skey, int *comp_start, int *comp_end) {
    for (i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x; k < n_rows_total; k += (i64)gridDim.x * blockDim.x) {
        const unsigned key = skey[k];
        if (k == 0 || skey[k - 1] != key) comp_start[key] = (int)k;
        if (k == n_rows_total - 1 || skey[k + 1] != key) comp_end[key] = (int)(k + 1);
    }
}

// Per sorted position (and one entry behind the last, all zero, for the scans): does a chunk start here, where does this one end,
// how many rep ids does the node stand for; and the two per-row outputs, label and node, local to the tint.
__global__ void __launch_bounds__(256) k_chunk(i64 n_rows_total, i64 max_size, const unsigned *skey, const int *sval, const int *comp_start,
                                               const int *comp_end, const i64 *mem_off, const int *row_tint, const TintDesc *tints,
                                               const int *parent, i64 *head, int *chunk_end, i64 *smult, int *label_out, int *node_out) {
    for (i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x; k <= n_rows_total; k += (i64)gridDim.x * blockDim.x) {
        if (k == n_rows_total) { head[k] = 0; smult[k] = 0; continue; }
        const unsigned key = skey[k];
        const i64 st = comp_start[key], n = comp_end[key] - st;
        const i64 p = (n + max_size - 1) / max_size, s = (n + p - 1) / p;      // :113-114 in integers
        const i64 pos = k - st, ch = pos / s;
        head[k] = pos == ch * s ? 1 : 0;
        const i64 ce = st + (ch + 1) * s;
        chunk_end[k] = (int)(ce < st + n ? ce : st + n);
        const int v = sval[k];
        smult[k] = mem_off[v + 1] - mem_off[v];
        node_out[k] = v - (int)tints[row_tint[v]].row0;
        label_out[k] = parent[k] - (int)tints[row_tint[k]].row0;
    }
}

// ---- incompatible pairs (:261-273) ------------------------------------------------------------------------------
// A wave per sorted position k = (partition, node i): the nodes j behind it in its chunk, 64 at a time (lane = j); a lane whose j
// has no edge to i stands for mult(i) * mult(j) pairs.  EMIT = false: the wave's total, cnt[k].  EMIT = true: the pairs themselves,
// behind pair_base[k] (the exclusive scan of cnt) in the reference's loop order -- j ascending (a prefix sum over the lanes), then
// rid_1 of i, then rid_2 of j.  A lane writes its own block when it is small (multiplicity 1: the lanes' pairs are neighbours in
// memory); a block of more than kLanePairs pairs is written by the whole wave.
constexpr int kLanePairs = 16;

template <bool EMIT>
__global__ void __launch_bounds__(256) k_pairs(i64 n_rows_total, const int *sval, const int *chunk_end, const i64 *smult, const int *row_tint,
                                               const TintDesc *tints, const u64 *adj, i64 *cnt, const i64 *pair_base, const i64 *mem_off,
                                               const int *mem, int2 *pairs) {
    const int lane = lane_id();
    const i64 wave_g = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((i64)gridDim.x * blockDim.x) >> 6;
    for (i64 k = wave_g; k < n_rows_total; k += n_waves) {
        const int i = sval[k];
        const TintDesc d = tints[row_tint[i]];
        const u64 *row = adj + d.adj_off + (i64)(i - d.row0) * d.aw;
        const i64 mi = smult[k], ce = chunk_end[k];
        const int *mem_i = mem + mem_off[i];
        const i64 base_k = EMIT ? pair_base[k] : 0;
        i64 run = 0;                                           // sum of mult(j) over the non-neighbours j taken so far
        for (i64 k0 = k + 1; k0 < ce; k0 += 64) {
            const i64 k2 = k0 + lane;
            i64 w = 0;
            int jrow = 0;
            if (k2 < ce) {
                jrow = sval[k2];
                const int j = jrow - (int)d.row0;
                if (!((row[j >> 6] >> (j & 63)) & 1ull)) w = smult[k2];
            }
            i64 inc = w;
            for (int s = 1; s < 64; s <<= 1) { const i64 o = __shfl_up(inc, s); if (lane >= s) inc += o; }
            if (EMIT) {
                const i64 base = base_k + mi * (run + inc - w), block = mi * w;
                if (block > 0 && block <= kLanePairs) {
                    const int *mem_j = mem + mem_off[jrow];
                    i64 x = base;
                    for (i64 a = 0; a < mi; ++a) for (i64 b = 0; b < w; ++b) pairs[x++] = make_int2(mem_i[a], mem_j[b]);
                }
                u64 big = __ballot(block > kLanePairs);
                while (big) {
                    const int L = __ffsll((long long)big) - 1;
                    big &= big - 1;
                    const i64 bL = __shfl(base, L), wL = __shfl(w, L);
                    const int *mem_j = mem + mem_off[__shfl(jrow, L)];
                    for (i64 x = lane; x < mi * wL; x += 64) { const i64 a = x / wL; pairs[bL + x] = make_int2(mem_i[a], mem_j[x - a * wL]); }
                }
            }
            run += __shfl(inc, 63);
        }
        if (!EMIT && lane == 0) cnt[k] = mi * run;
    }
}

// ---- partition members: the rep ids of a partition's nodes, end to end ---------------------------------------------
__global__ void __launch_bounds__(256) k_members(i64 n_rows_total, const int *sval, const i64 *smult, const i64 *rid_pos, const i64 *mem_off,
                                                 const int *mem, int *part_rids) {
    const int lane = lane_id();
    const i64 wave_g = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((i64)gridDim.x * blockDim.x) >> 6;
    for (i64 k = wave_g; k < n_rows_total; k += n_waves) {
        const int *src = mem + mem_off[sval[k]];
        int *dst = part_rids + rid_pos[k];
        for (i64 x = lane; x < smult[k]; x += 64) dst[x] = src[x];
    }
}

// ---- the offset arrays: partition q starts where the q-th chunk head stands (part_id = exclusive scan of head) -----------
__global__ void __launch_bounds__(256) k_offsets(i64 n_rows_total, int n_tint, const TintDesc *tints, const i64 *head, const i64 *part_id,
                                                 const i64 *rid_pos, const i64 *pair_base, i64 *tint_part_off, i64 *part_node_off,
                                                 i64 *part_rid_off, i64 *part_pair_off) {
    const i64 last = n_rows_total > n_tint ? n_rows_total : n_tint;
    for (i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x; k <= last; k += (i64)gridDim.x * blockDim.x) {
        if (k == n_rows_total || (k < n_rows_total && head[k])) {
            const i64 q = part_id[k];
            part_node_off[q] = k; part_rid_off[q] = rid_pos[k]; part_pair_off[q] = pair_base[k];
        }
        if (k <= n_tint) tint_part_off[k] = part_id[k < n_tint ? tints[k].row0 : n_rows_total];
    }
}

// ================================================================================================================
// The front of partition_reads(): preprocess_ilp() per rep (py/freddie_cluster.py:285-310, :175-183) and the dedupe of reps
// with the same structure (:203-215), from label rows at two bits a label (fclu_reads).
// ================================================================================================================
struct PrepTint {
    i64 item0, lab_off, rbits_off, slot0;  // first rep; first label word; first word of the reps' I / C rows; first lane slot of k_rows
    int n, n_seg, lw, w, g_log2;            // reps, segments, label words and bit words per row, log2 of the lanes a rep gets
};

// the 32 even bits of x, packed
__device__ __forceinline__ unsigned even_bits(u64 x) {
    x &= 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x >> 4)) & 0x00ff00ff00ff00ffull;
    x = (x | (x >> 8)) & 0x0000ffff0000ffffull;
    return (unsigned)(x | (x >> 16));
}

__device__ __forceinline__ unsigned mix32(unsigned h) {
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

// bits [f, l] of word w of a row, for any f, l (none when the word lies outside, or l < f)
__device__ __forceinline__ unsigned span_mask(int f, int l, int w) {
    if (l < f || w * 32 + 31 < f || w * 32 > l) return 0u;
    return range_mask(f, l, w);
}

// ---- per rep: I, C, raw first / last, FL, and the dedupe's sort key ------------------------------------------------
// A rep gets g = 2^g_log2 lanes (the smallest power of two that holds its W words, 64 at the most), so a wave takes 64 / g reps: rows
// of one or two words do not cost a wave each.  A tint's slots start at a multiple of 64: a wave works on one tint, and a rep's lanes
// are g consecutive lanes, so the min / max / sum over its words are xor shuffles below g.  A lane's bit word w comes from the label
// words 2w and 2w + 1: I = the low bit of each label (2 counts as 0, :287-288), "label is 0" = neither bit; C is that, cut to
// [first, last] in a second pass over the lane's own words (:308-310).  err[0..2]: the smallest rep with a label 3, with a bit behind
// its M labels, with a tail category above 2.
__global__ void __launch_bounds__(256) k_rows(int n_tint, i64 n_slots, const PrepTint *pt, const unsigned *labels, const unsigned char *tail,
                                              unsigned hash_mask, unsigned *ibits, unsigned *cbits, int *raw_first, int *raw_last, int *first,
                                              int *last, int *rep_tint, u64 *key, int *val, int *err) {
    const int lane = lane_id();
    const i64 wave_g = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((i64)gridDim.x * blockDim.x) >> 6;
    for (i64 s0 = wave_g * 64; s0 < n_slots; s0 += n_waves * 64) {
        int lo = 0, hi = n_tint - 1;                          // the last tint whose slots start at or before s0 (wave-uniform)
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (pt[mid].slot0 <= s0) lo = mid; else hi = mid - 1; }
        const int t = __builtin_amdgcn_readfirstlane(lo);
        const PrepTint d = pt[t];
        const int g = 1 << d.g_log2, sub = lane & (g - 1);
        const i64 r = (s0 - d.slot0 + lane) >> d.g_log2;
        const bool ok = r < d.n;
        const i64 rep = d.item0 + (ok ? r : 0);
        const unsigned *lab = labels + d.lab_off + (ok ? r : 0) * d.lw;
        unsigned *ib = ibits + d.rbits_off + (ok ? r : 0) * d.w, *cb = cbits + d.rbits_off + (ok ? r : 0) * d.w;
        int fmin = 0x7fffffff, lmax = -1, bad = 0;
        unsigned h = 0;
        if (ok)
            for (int w = sub; w < d.w; w += g) {
                const u64 x = (u64)lab[2 * w] | (2 * w + 1 < d.lw ? (u64)lab[2 * w + 1] << 32 : 0ull);
                int nv = d.n_seg - 32 * w; nv = nv > 32 ? 32 : (nv < 0 ? 0 : nv);
                const u64 vm = nv >= 32 ? ~0ull : ((1ull << (2 * nv)) - 1ull);
                const u64 b0 = x & 0x5555555555555555ull, b1 = (x >> 1) & 0x5555555555555555ull;
                if (b0 & b1 & vm) bad |= 1;
                if (x & ~vm) bad |= 2;
                const unsigned iw = even_bits(b0 & ~b1 & vm), zw = even_bits(~(b0 | b1) & vm);
                ib[w] = iw; cb[w] = zw;
                if (iw) {
                    const int a = w * 32 + __ffs((int)iw) - 1, z = w * 32 + 31 - __clz((int)iw);
                    fmin = a < fmin ? a : fmin; lmax = z > lmax ? z : lmax;
                }
                h += mix32(iw ^ ((unsigned)w * 0x9e3779b9u + 0x7f4a7c15u));
            }
        for (int s = g >> 1; s >= 1; s >>= 1) {
            const int of = __shfl_xor(fmin, s), ol = __shfl_xor(lmax, s);
            fmin = of < fmin ? of : fmin; lmax = ol > lmax ? ol : lmax;
            h += (unsigned)__shfl_xor((int)h, s);
        }
        const int tl = ok ? tail[rep] : 0;
        if (tl > 2) bad |= 4;
        const int rf = fmin == 0x7fffffff ? -1 : fmin, rl = fmin == 0x7fffffff ? d.n_seg - 1 : lmax;     // find_segment_read (:175-183)
        const int f = tl == 1 ? 0 : rf, l = tl == 2 ? d.n_seg - 1 : rl;                                  // the tail's override (:297, :300)
        if (ok) {
            for (int w = sub; w < d.w; w += g) cb[w] &= span_mask(f < 0 ? 0 : f, l, w);
            if (bad & 1) atomicMin(&err[0], (int)rep);
            if (bad & 2) atomicMin(&err[1], (int)rep);
            if (bad & 4) atomicMin(&err[2], (int)rep);
            if (sub == 0) {
                raw_first[rep] = rf; raw_last[rep] = rl; first[rep] = f; last[rep] = l; rep_tint[rep] = t;
                const unsigned hh = mix32(h ^ mix32((unsigned)f * 0x9e3779b9u + (unsigned)l) ^ ((unsigned)tl * 0x27d4eb2fu));
                key[rep] = ((u64)(unsigned)t << 32) | (u64)(hh & hash_mask);
                val[rep] = (int)rep;
            }
        }
    }
}

// ---- the dedupe (:203-215) --------------------------------------------------------------------------------------
// The reps, sorted (stable) by (tint, hash): a bucket = the run of one key, its reps ascending.  The hash only makes the buckets; a
// rep's class is decided on the whole row: its leader is the FIRST rep of its bucket with the same I row, first, last and tail --
// the smallest rep of its class, whatever else shares the bucket and however the classes interleave in it.  Without collisions the
// bucket's first rep answers at once.
__global__ void __launch_bounds__(256) k_heads(i64 n, const u64 *skey, int *head) {
    for (i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (i64)gridDim.x * blockDim.x)
        head[k] = (k > 0 && skey[k - 1] == skey[k]) ? 0 : (int)k;
}

__global__ void __launch_bounds__(256) k_leader(i64 n, const u64 *skey, const int *sval, const int *bstart, const PrepTint *pt, const unsigned *ibits,
                                                const int *first, const int *last, const unsigned char *tail, int *leader, int *flag) {
    for (i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (i64)gridDim.x * blockDim.x) {
        const PrepTint d = pt[(int)(skey[k] >> 32)];
        const int rep = sval[k];
        const unsigned *a = ibits + d.rbits_off + (i64)(rep - d.item0) * d.w;
        const int fa = first[rep], la = last[rep], ta = tail[rep];
        int lead = rep;
        for (i64 j = bstart[k]; j < k; ++j) {
            const int other = sval[j];
            if (first[other] != fa || last[other] != la || tail[other] != ta) continue;
            const unsigned *b = ibits + d.rbits_off + (i64)(other - d.item0) * d.w;
            bool same = true;
            for (int w = 0; w < d.w; ++w) if (a[w] != b[w]) { same = false; break; }
            if (same) { lead = other; break; }
        }
        leader[rep] = lead;
        flag[rep] = lead == rep ? 1 : 0;
    }
}

// off[t] = the number of leaders in front of tint t's first item (id: the exclusive scan of flag, n_items + 1 entries): the tints' row_off
// behind the reps' dedupe (D = PrepTint), their rep_off behind the reads' grouping (D = GroupTint)
template <typename D>
__global__ void __launch_bounds__(256) k_class_off(int n_tint, i64 n_items, const D *tints, const int *id, i64 *off) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t <= n_tint) off[t] = id[t < n_tint ? tints[t].item0 : n_items];
}

// Nodes are numbered by their smallest rep (the leader): the leaders' scan IS the numbering.  A rep learns its node; a leader hands
// its row, first, last and tail to the node's place in the arrays k_compat reads (the batch's layout, fclu_batch).
__global__ void __launch_bounds__(256) k_nodes(i64 n_reps, const int *rep_tint, const PrepTint *pt, const TintDesc *tints, const int *leader,
                                               const int *node_id, const unsigned *ibits, const int *first, const int *last,
                                               const unsigned char *tail, int *rep_node, unsigned *nkey, int *nval, int *node_rep,
                                               unsigned *bits, int *nfirst, int *nlast, unsigned char *ntail) {
    for (i64 rep = (i64)blockIdx.x * blockDim.x + threadIdx.x; rep < n_reps; rep += (i64)gridDim.x * blockDim.x) {
        const int t = rep_tint[rep];
        const PrepTint p = pt[t];
        const TintDesc d = tints[t];
        const int lead = leader[rep], node = node_id[lead];
        rep_node[rep] = node - (int)d.row0;
        nkey[rep] = (unsigned)node;
        nval[rep] = (int)(rep - p.item0);
        if (lead == rep) {
            node_rep[node] = (int)(rep - p.item0);
            nfirst[node] = first[rep]; nlast[node] = last[rep]; ntail[node] = tail[rep];
            const unsigned *src = ibits + p.rbits_off + (rep - p.item0) * p.w;
            unsigned *dst = bits + d.bits_off + (i64)(node - d.row0) * d.w;
            for (int w = 0; w < p.w; ++w) dst[w] = src[w];
        }
    }
}

// the reps sorted (stable) by node are the nodes' member lists end to end, each ascending: node q's starts where its key first stands
__global__ void __launch_bounds__(256) k_mem_off(i64 n_reps, i64 n_rows, const unsigned *skey, i64 *mem_off) {
    for (i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x; k <= n_reps; k += (i64)gridDim.x * blockDim.x) {
        if (k == n_reps) mem_off[n_rows] = n_reps;
        else if (k == 0 || skey[k - 1] != skey[k]) mem_off[skey[k]] = k;
    }
}

// ================================================================================================================
// In front of preprocess_ilp(): read_segment()'s grouping of a tint's reads into reps (py/freddie_cluster.py:154-164), from ALL
// reads' label rows and key token streams (fclu_segment).  Two reads share a rep exactly when their I rows (2 counts as 0) and
// their token streams are equal; the dedupe's shape: hash, stable sort by (tint, hash), leaders on whole rows, scan, members.
// ================================================================================================================
struct GroupTint {
    i64 item0, lab_off, slot0;              // first read; first label word; first lane slot of k_gkeys
    int n, n_seg, lw, g_log2, vec;          // reads, segments, label words a row, log2 of the lanes a read gets, rows are whole 16-byte quads
};

// the I row of a label word, left where it stands: the low bit of every label that is not 3 (labels are 0, 1, 2 here)
__device__ __forceinline__ unsigned i_spread(unsigned x) { return x & 0x55555555u & ~(x >> 1); }

// one label word of a read's row for the key: its share of the hash, and the two refusals (a label 3, a bit behind the M labels)
__device__ __forceinline__ unsigned key_word(unsigned x, int w, int n_seg, int &bad) {
    int nv = n_seg - 16 * w; nv = nv > 16 ? 16 : (nv < 0 ? 0 : nv);
    const unsigned vm = nv >= 16 ? 0xffffffffu : ((1u << (2 * nv)) - 1u);
    if (x & (x >> 1) & 0x55555555u & vm) bad |= 1;
    if (x & ~vm) bad |= 2;
    return mix32((i_spread(x) & vm) ^ ((unsigned)w * 0x9e3779b9u + 0x7f4a7c15u));
}

// ---- per read: the sort key (tint, hash of I row + token stream) ------------------------------------------------------
// k_rows' lane grouping: a read gets g = 2^g_log2 consecutive lanes (the smallest power of two that holds its label words -- its
// 16-byte quads where every row of the tint is whole quads, which a lane then loads at once -- 64 at the most, looping beyond), a
// tint's slots start at a multiple of 64, so a wave works on one tint and the sum below g is xor shuffles.  err[0..2]: the smallest
// read with a label 3, with a bit behind its M labels, with a tail category above 2.
__global__ void __launch_bounds__(256) k_gkeys(int n_tint, i64 n_slots, const GroupTint *gt, const unsigned *labels, const i64 *tok_off,
                                               const unsigned *tok, const unsigned char *tail, unsigned hash_mask, int *read_tint, u64 *key,
                                               int *val, int *err) {
    const int lane = lane_id();
    const i64 wave_g = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((i64)gridDim.x * blockDim.x) >> 6;
    for (i64 s0 = wave_g * 64; s0 < n_slots; s0 += n_waves * 64) {
        int lo = 0, hi = n_tint - 1;                          // the last tint whose slots start at or before s0 (wave-uniform)
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (gt[mid].slot0 <= s0) lo = mid; else hi = mid - 1; }
        const int t = __builtin_amdgcn_readfirstlane(lo);
        const GroupTint d = gt[t];
        const int g = 1 << d.g_log2, sub = lane & (g - 1);
        const i64 r = (s0 - d.slot0 + lane) >> d.g_log2;
        const bool ok = r < d.n;
        const i64 read = d.item0 + (ok ? r : 0);
        const unsigned *lab = labels + d.lab_off + (ok ? r : 0) * d.lw;
        int bad = 0;
        unsigned h = 0;
        if (ok) {
            if (d.vec) {
                const uint4 *lab4 = reinterpret_cast<const uint4 *>(lab);
                for (int q = sub; q < (d.lw >> 2); q += g) {
                    const uint4 v = lab4[q];
                    h += key_word(v.x, 4 * q, d.n_seg, bad); h += key_word(v.y, 4 * q + 1, d.n_seg, bad);
                    h += key_word(v.z, 4 * q + 2, d.n_seg, bad); h += key_word(v.w, 4 * q + 3, d.n_seg, bad);
                }
            } else
                for (int w = sub; w < d.lw; w += g) h += key_word(lab[w], w, d.n_seg, bad);
            const i64 t0 = tok_off[read], nt = tok_off[read + 1] - t0;
            for (i64 k = sub; k < nt; k += g) h += mix32(tok[t0 + k] ^ ((unsigned)k * 0x85ebca6bu + 0x165667b1u));
            if (sub == 0) h += mix32((unsigned)nt * 0x27d4eb2fu + 1u);
        }
        for (int s = g >> 1; s >= 1; s >>= 1) h += (unsigned)__shfl_xor((int)h, s);
        if (ok) {
            if (bad & 1) atomicMin(&err[0], (int)read);
            if (bad & 2) atomicMin(&err[1], (int)read);
            if (sub == 0) {
                if (tail[read] > 2) atomicMin(&err[2], (int)read);
                read_tint[read] = t;
                key[read] = ((u64)(unsigned)t << 32) | (u64)(mix32(h) & hash_mask);
                val[read] = (int)read;
            }
        }
    }
}

// A read's leader: the FIRST read of its bucket whose WHOLE I row and WHOLE token stream are equal (k_leader's rule; the hash never
// decides).  The other read's tokens are read through addresses clamped to its own stream (to the array, when it has none), and what
// they say counts only when the two streams are equally long.
__global__ void __launch_bounds__(256) k_gleader(i64 n, const u64 *skey, const int *sval, const int *bstart, const GroupTint *gt, const unsigned *labels,
                                                 const i64 *tok_off, const unsigned *tok, i64 n_tok, int *leader, int *flag) {
    for (i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (i64)gridDim.x * blockDim.x) {
        const GroupTint d = gt[(int)(skey[k] >> 32)];
        const int read = sval[k];
        const unsigned *a = labels + d.lab_off + (i64)(read - d.item0) * d.lw;
        const i64 ta = tok_off[read], na = tok_off[read + 1] - ta;
        int lead = read;
        for (i64 j = bstart[k]; j < k; ++j) {
            const int other = sval[j];
            const unsigned *b = labels + d.lab_off + (i64)(other - d.item0) * d.lw;
            const i64 tb = tok_off[other], nb = tok_off[other + 1] - tb;
            bool same = true;
            for (int w = 0; w < d.lw; ++w) if (i_spread(a[w]) != i_spread(b[w])) { same = false; break; }
            if (!same) continue;
            for (i64 x = 0; x < na; ++x) {
                i64 at = tb + (x < nb ? x : 0);
                at = at < n_tok ? at : n_tok - 1;
                if (tok[ta + x] != tok[at]) { same = false; break; }
            }
            if (same && na == nb) { lead = other; break; }
        }
        leader[read] = lead;
        flag[read] = lead == read ? 1 : 0;
    }
}

// Reps are numbered by their first read (the leader): the leaders' scan IS the numbering (Python's dict insertion order, :162-164).
// A read learns its rep; a leader is its rep's first read.  nkey / nval: the second sort's input (rep of the batch, read of the tint).
__global__ void __launch_bounds__(256) k_greps(i64 n_reads, const int *read_tint, const GroupTint *gt, const int *leader, const int *rep_id,
                                               int *read_rep, unsigned *nkey, int *nval, int *rep_first) {
    for (i64 read = (i64)blockIdx.x * blockDim.x + threadIdx.x; read < n_reads; read += (i64)gridDim.x * blockDim.x) {
        const GroupTint d = gt[read_tint[read]];
        const int lead = leader[read], rep = rep_id[lead];
        read_rep[read] = rep - rep_id[d.item0];
        nkey[read] = (unsigned)rep;
        nval[read] = (int)(read - d.item0);
        if (lead == read) rep_first[rep] = (int)(read - d.item0);
    }
}

// The reps' rows and tails, where k_rows reads them (fclu_reads' layout): a rep's row is its FIRST read's, with its 2s (:286-289), and
// so is its tail.  A thread a label word: rep_lab_off[t] = the first word of tint t's reps.
__global__ void __launch_bounds__(256) k_ggather(int n_tint, i64 n_words, const GroupTint *gt, const i64 *rep_off, const i64 *rep_lab_off,
                                                 const int *rep_first, const unsigned *labels, const unsigned char *tail, unsigned *rep_labels,
                                                 unsigned char *rep_tail) {
    for (i64 x = (i64)blockIdx.x * blockDim.x + threadIdx.x; x < n_words; x += (i64)gridDim.x * blockDim.x) {
        int lo = 0, hi = n_tint - 1;                          // the last tint whose words start at or before x
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (rep_lab_off[mid] <= x) lo = mid; else hi = mid - 1; }
        const GroupTint d = gt[lo];
        const i64 y = x - rep_lab_off[lo], r = y / d.lw;
        const int w = (int)(y - r * d.lw);
        const i64 rep = rep_off[lo] + r, first = rep_first[rep];
        rep_labels[x] = labels[d.lab_off + first * d.lw + w];
        if (w == 0) rep_tail[rep] = tail[d.item0 + first];
    }
}

// ================================================================================================================
// A round's ILP models as arrays (fclu_round_models): what run_ilp() builds its model from (py/freddie_cluster.py:359, :397-535), for
// round r of many partitions at once.  A problem = a partition and its remaining reps ("columns", in the caller's order).
// ================================================================================================================
struct RoundProb {
    i64 col0, rbits_off, rep0, pair0, pair1, inf_off, seg0;   // first column (in rids); the tint's first I / C word, first rep and first
                                                              // segment length; the partition's pairs; the informative row's first word
    int n, n_seg, w, tint;                                    // columns, segments, words per row; the tint (the host's own note)
};

constexpr int kRoundCounts = 4;                  // per problem: informative segments, support entries, correction terms, pairs
constexpr int kRoundLdsBytes = 96 * 1024;        // I and C rows of a problem staged in LDS up to this (beside about 5 KB of static arrays: one such
                                                 // workgroup a CU; two from about 75 KB down)
constexpr int kRoundTinyBytes = 16 * 1024;       // problems up to this are launched apart, with their own LDS size: a batch's one large problem
                                                 // does not cost hundreds of small ones their occupancy

// exclusive prefix sum of v over the workgroup's 256 threads (total: the sum); s_wave: 4 words of LDS; synchronises before it returns
__device__ __forceinline__ i64 block_scan(i64 v, i64 &total, i64 *s_wave) {
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    i64 inc = v;
    for (int s = 1; s < 64; s <<= 1) { const i64 o = __shfl_up(inc, s); if (lane >= s) inc += o; }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    i64 before = 0;
    total = 0;
    for (int x = 0; x < 4; ++x) { const i64 t = s_wave[x]; if (x < wave) before += t; total += t; }
    __syncthreads();
    return before + inc - v;
}

// a[0 .. n) (counts, written by this workgroup) -> base + their exclusive prefix sums, in place
__device__ __forceinline__ void block_scan_inplace(i64 *a, int n, i64 base, i64 *s_wave) {
    __syncthreads();
    i64 carry = base;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + (int)threadIdx.x;
        const i64 v = i < n ? a[i] : 0;
        i64 total;
        const i64 ex = block_scan(v, total, s_wave);
        if (i < n) a[i] = carry + ex;
        carry += total;
    }
    __syncthreads();
}

// A workgroup per problem.  LDS: the I and C rows of the remaining reps are staged (row stride W | 1 words, so that a lane per column
// does not hit one bank); !LDS: they are read where preprocess left them.
// EMIT = false, the counts: the AND and the OR of the columns' I words (a stripe of columns per lane, met in LDS atomics -- AND and OR do
// not depend on the order), the informative row (informative_segs(), :331-344: segment j is dropped when the columns j - 1, j, j + 1 hold
// one value each and the same one; "column holds only 0" = ~OR, "only 1" = AND, the neighbours by shifts with the carries of the words
// next door; bits behind M count as "holds both", which keeps segment M - 1, and bit 0 has no left neighbour, which keeps segment 0),
// col_of (the membership mask of :500-502) and the problem's four totals.
// EMIT = true, behind the scan of the totals: the informative segments; support (per informative j its columns, a wave per segment, a
// ballot per 64 columns); the correction terms (per column its informative j with C = 1); the pairs with both ends remaining, in the
// partition's order (a prefix sum over the workgroup per 256 pairs).  Nothing depends on the order atomics arrive in.
template <bool LDS, bool EMIT>
__global__ void __launch_bounds__(256) k_round(const int *list, int P, const RoundProb *probs, const unsigned *ibits, const unsigned *cbits,
                                               const int *rids, int *col_of, const int2 *part_pairs, unsigned *inf_bits, i64 *cnt,
                                               const i64 *scan, int *inf_seg, i64 *sup_off, int *sup_cols, i64 *corr_off, int *corr_seg,
                                               int2 *out_pairs) {
    extern __shared__ unsigned s_rows[];
    __shared__ unsigned s_and[kMaxWords], s_or[kMaxWords], s_inf[kMaxWords];
    __shared__ int s_rank[kMaxWords];
    __shared__ i64 s_wave[4];
    __shared__ int s_tot[kRoundCounts];
    const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    const int p = list[blockIdx.x];
    const RoundProb d = probs[p];
    const int R = d.n, W = d.w, M = d.n_seg, S = W | 1;
    const int *prids = rids + d.col0;
    if (LDS) {
        for (int x = tid; x < R * W; x += 256) {
            const int c = x / W, w = x - c * W;
            const i64 src = d.rbits_off + (i64)prids[c] * W + w;
            s_rows[c * S + w] = ibits[src];
            s_rows[(R + c) * S + w] = cbits[src];
        }
    }
    const auto row_i = [&](int c, int w) { return LDS ? s_rows[c * S + w] : ibits[d.rbits_off + (i64)prids[c] * W + w]; };
    const auto row_c = [&](int c, int w) { return LDS ? s_rows[(R + c) * S + w] : cbits[d.rbits_off + (i64)prids[c] * W + w]; };
    if (!EMIT) {
        for (int c = tid; c < R; c += 256) col_of[d.rep0 + prids[c]] = c;
        for (int w = tid; w < W; w += 256) { s_and[w] = 0xffffffffu; s_or[w] = 0u; }
        if (tid < kRoundCounts) s_tot[tid] = 0;
        __syncthreads();
        const int stripes = W >= 256 ? 1 : 256 / W;
        for (int x = tid; x < stripes * W; x += 256) {
            const int st = x / W, w = x - st * W;
            unsigned a = 0xffffffffu, o = 0u;
            for (int c = st; c < R; c += stripes) { const unsigned v = row_i(c, w); a &= v; o |= v; }
            atomicAnd(&s_and[w], a); atomicOr(&s_or[w], o);
        }
        __syncthreads();
        int n_inf = 0;
        for (int w = tid; w < W; w += 256) {
            const int rest = M - w * 32;                       // the row's bits in this word: all of them valid, or the low `rest`
            const unsigned valid = rest >= 32 ? 0xffffffffu : rest <= 0 ? 0u : (1u << rest) - 1u;
            unsigned inf = valid;
            if (R > 0) {
                const int wl = max(w - 1, 0), wr = min(w + 1, W - 1);                 // (clamped; the carry is dropped where there is no word)
                const int rest_r = M - wr * 32;
                const unsigned valid_r = rest_r >= 32 ? 0xffffffffu : rest_r <= 0 ? 0u : (1u << rest_r) - 1u;
                const unsigned z = ~s_or[w] & valid, zl = w > 0 ? ~s_or[wl] : 0u, zr = w + 1 < W ? ~s_or[wr] & valid_r : 0u;
                const unsigned a = s_and[w] & valid, al = w > 0 ? s_and[wl] : 0u, ar = w + 1 < W ? s_and[wr] & valid_r : 0u;
                const unsigned u0 = z & ((z << 1) | (zl >> 31)) & ((z >> 1) | (zr << 31));
                const unsigned u1 = a & ((a << 1) | (al >> 31)) & ((a >> 1) | (ar << 31));
                inf = valid & ~(u0 | u1);
            }
            s_inf[w] = inf;
            inf_bits[d.inf_off + w] = inf;
            n_inf += __popc(inf);
        }
        __syncthreads();
        int n_sup = 0, n_corr = 0, n_pair = 0;
        for (int x = tid; x < R * W; x += 256) {
            const int c = x / W, w = x - c * W;
            n_sup += __popc(row_i(c, w) & s_inf[w]);
            n_corr += __popc(row_c(c, w) & s_inf[w]);
        }
        for (i64 i = d.pair0 + tid; i < d.pair1; i += 256) {
            const int2 pr = part_pairs[i];
            n_pair += (col_of[d.rep0 + pr.x] >= 0 && col_of[d.rep0 + pr.y] >= 0) ? 1 : 0;
        }
        int v[kRoundCounts] = {n_inf, n_sup, n_corr, n_pair};
        for (int k = 0; k < kRoundCounts; ++k) {
            for (int s = 32; s > 0; s >>= 1) v[k] += __shfl_xor(v[k], s);
            if (lane == 0) atomicAdd(&s_tot[k], v[k]);
        }
        __syncthreads();
        if (tid < kRoundCounts) cnt[(i64)tid * (P + 1) + p] = s_tot[tid];
        return;
    }
    // ---- EMIT
    const i64 inf_base = scan[p], sup_base = scan[(i64)(P + 1) + p] - scan[(i64)(P + 1)];
    const i64 corr_base = scan[2ll * (P + 1) + p] - scan[2ll * (P + 1)], pair_base = scan[3ll * (P + 1) + p] - scan[3ll * (P + 1)];
    for (int w = tid; w < W; w += 256) s_inf[w] = inf_bits[d.inf_off + w];
    __syncthreads();
    i64 carry = 0;
    for (int w0 = 0; w0 < W; w0 += 256) {                        // the informative segments in front of every word, and the segments themselves
        const int w = w0 + tid;
        unsigned m = w < W ? s_inf[w] : 0u;
        i64 total;
        const i64 ex = block_scan(__popc(m), total, s_wave);
        if (w < W) s_rank[w] = (int)(carry + ex);
        i64 x = inf_base + carry + ex;
        while (m) { inf_seg[x++] = w * 32 + __ffs((int)m) - 1; m &= m - 1; }
        carry += total;
    }
    __syncthreads();
    const int n_inf = (int)carry;
    i64 *my_sup = sup_off + inf_base;
    for (int pass = 0; pass < 2; ++pass) {                        // support: the counts, their prefix sums in place, the columns
        for (int j = wave; j < M; j += 4) {
            const unsigned m = s_inf[j >> 5];
            if (!((m >> (j & 31)) & 1u)) continue;
            const int k = s_rank[j >> 5] + __popc(m & ((1u << (j & 31)) - 1u));
            const i64 base = pass ? my_sup[k] : 0;
            int run = 0;
            for (int c0 = 0; c0 < R; c0 += 64) {
                const int c = min(c0 + lane, R - 1);
                const bool on = c0 + lane < R && ((row_i(c, j >> 5) >> (j & 31)) & 1u);
                const u64 b = __ballot(on);
                if (pass && on) sup_cols[base + run + __popcll(b & ((1ull << lane) - 1ull))] = c;
                run += __popcll(b);
            }
            if (!pass && lane == 0) my_sup[k] = run;
        }
        if (!pass) block_scan_inplace(my_sup, n_inf, sup_base, s_wave);
    }
    i64 *my_corr = corr_off + d.col0;                            // the correction terms: the same three steps, a lane per column
    for (int c = tid; c < R; c += 256) {
        int n = 0;
        for (int w = 0; w < W; ++w) n += __popc(row_c(c, w) & s_inf[w]);
        my_corr[c] = n;
    }
    block_scan_inplace(my_corr, R, corr_base, s_wave);
    for (int c = tid; c < R; c += 256) {
        i64 x = my_corr[c];
        for (int w = 0; w < W; ++w) {
            unsigned m = row_c(c, w) & s_inf[w];
            while (m) { corr_seg[x++] = w * 32 + __ffs((int)m) - 1; m &= m - 1; }
        }
    }
    i64 run = pair_base;                                         // the pairs
    for (i64 i0 = d.pair0; i0 < d.pair1; i0 += 256) {
        const i64 i = i0 + tid;
        const int2 pr = part_pairs[min(i, d.pair1 - 1)];
        const int a = col_of[d.rep0 + pr.x], b = col_of[d.rep0 + pr.y];
        const bool keep = i < d.pair1 && a >= 0 && b >= 0;
        i64 total;
        const i64 ex = block_scan(keep ? 1 : 0, total, s_wave);
        if (keep) out_pairs[run + ex] = make_int2(a, b);
        run += total;
    }
}

// ---- gap groups (:462-497) -------------------------------------------------------------------------------------------
// A row = (column, gap of its rep), in column order then the rep's own order: row_off per column comes from the host, which holds the
// reps' gap counts.  A row's key = (problem, (j1 + 1) * (M + 2) + j2 + 1) (a rep without a 1 and an 'S' tail has the pseudo-gap (-1, -1)): sorted, the runs of one key are the problems' distinct (j1, j2),
// ascending -- the groups, numbered through the batch.
__global__ void __launch_bounds__(256) k_gap_keys(i64 n_cols, const int *col_prob, const RoundProb *probs, const int *rids, const i64 *gap_off,
                                                  const int *gaps, const i64 *row_off, u64 *key, int *val, int *rows) {
    for (i64 cg = (i64)blockIdx.x * blockDim.x + threadIdx.x; cg < n_cols; cg += (i64)gridDim.x * blockDim.x) {
        const int p = col_prob[cg];
        const RoundProb d = probs[p];
        const i64 g0 = gap_off[d.rep0 + rids[cg]], n = gap_off[d.rep0 + rids[cg] + 1] - g0, r0 = row_off[cg];
        for (i64 g = 0; g < n; ++g) {
            const int j1 = gaps[3 * (g0 + g)], j2 = gaps[3 * (g0 + g) + 1];
            key[r0 + g] = ((u64)(unsigned)p << 32) | (u64)((i64)(j1 + 1) * (d.n_seg + 2) + (j2 + 1));
            val[r0 + g] = (int)(r0 + g);
            rows[3 * (r0 + g)] = (int)(cg - d.col0);
            rows[3 * (r0 + g) + 2] = gaps[3 * (g0 + g) + 2];
        }
    }
}

__global__ void __launch_bounds__(256) k_gap_heads(i64 n, const u64 *skey, i64 *head) {
    for (i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (i64)gridDim.x * blockDim.x)
        head[k] = (k > 0 && skey[k - 1] == skey[k]) ? 0 : 1;
}

__device__ __forceinline__ int inf_bit(const unsigned *row, int j) { return (row[j >> 5] >> (j & 31)) & 1u; }

// gid = the inclusive scan of head: sorted row k belongs to group gid[k] - 1.  Per sorted row: its group, local to the problem, and the
// refusal of :467-468 (the smallest column of a problem whose gap has an uninformative endpoint; Python's j % M: -1 is M - 1, M is 0; a rep without a 1 has first = -1, so j2 = -1 occurs).
// Per head: the group's (j1, j2), its problem and its count of informative segments strictly between.  Per problem: grp_off.
__global__ void __launch_bounds__(256) k_gap_groups(i64 n, int P, const u64 *skey, const int *sval, const i64 *gid, const i64 *prob_row_off,
                                                    const RoundProb *probs, const unsigned *inf_bits, int *rows, int *grp, int *grp_prob,
                                                    i64 *grp_cnt, i64 *grp_off, int *refused) {
    const i64 last = n > P ? n : P;
    for (i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x; k <= last; k += (i64)gridDim.x * blockDim.x) {
        if (k <= P) { const i64 r = prob_row_off[k]; grp_off[k] = r < n ? gid[r] - 1 : gid[n - 1]; }
        if (k >= n) continue;
        const int p = (int)(skey[k] >> 32);
        const RoundProb d = probs[p];
        const i64 kk = (i64)(skey[k] & 0xffffffffull), g = gid[k] - 1;
        const int j1 = (int)(kk / (d.n_seg + 2)) - 1, j2 = (int)(kk % (d.n_seg + 2)) - 1;
        const unsigned *inf = inf_bits + d.inf_off;
        const int r = sval[k];
        rows[3 * (i64)r + 1] = (int)(g - (gid[prob_row_off[p]] - 1));
        if (!inf_bit(inf, j1 < 0 ? d.n_seg - 1 : j1) || !inf_bit(inf, j2 < 0 ? d.n_seg - 1 : j2 >= d.n_seg ? 0 : j2)) atomicMin(&refused[p], rows[3 * (i64)r]);
        if (k == 0 || skey[k - 1] != skey[k]) {
            grp[2 * g] = j1; grp[2 * g + 1] = j2; grp_prob[g] = p;
            int n_between = 0;
            for (int w = (j1 + 1) >> 5; w <= (j2 - 1) >> 5 && j1 + 1 <= j2 - 1; ++w) n_between += __popc(inf[w] & span_mask(j1 + 1, j2 - 1, w));
            grp_cnt[g] = n_between;
        }
    }
}

// a group's informative segments strictly between j1 and j2, with their lengths (GAPI_C1, :474-481), behind the scan of the counts
__global__ void __launch_bounds__(256) k_gap_fill(const i64 *gid, i64 n_rows, const int *grp, const int *grp_prob, const i64 *grp_seg_off,
                                                  const RoundProb *probs, const unsigned *inf_bits, const int *seg_len, int *grp_seg, int *grp_len) {
    const i64 n_grp = gid[n_rows - 1];
    for (i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x; g < n_grp; g += (i64)gridDim.x * blockDim.x) {
        const RoundProb d = probs[grp_prob[g]];
        const unsigned *inf = inf_bits + d.inf_off;
        const int j1 = grp[2 * g], j2 = grp[2 * g + 1];
        i64 x = grp_seg_off[g];
        for (int w = (j1 + 1) >> 5; w <= (j2 - 1) >> 5 && j1 + 1 <= j2 - 1; ++w) {
            unsigned m = inf[w] & span_mask(j1 + 1, j2 - 1, w);
            while (m) { const int j = w * 32 + __ffs((int)m) - 1; grp_seg[x] = j; grp_len[x] = seg_len[d.seg0 + j]; ++x; m &= m - 1; }
        }
    }
}

// ================================================================================================================
// Greedy round incumbents (fclu_round_incumbents): with K = 2 a round's model is a function of the chosen column set S alone (e = the OR
// of the members' I rows on the informative segments, cost = the members' popcount(C & e) + the others' garbage costs, no incompatible
// pair in S, every gap row of a member holding), so a feasible S of low cost is bit-row arithmetic on what fclu_round_models has just
// left on the device.  The definition is cluster_solve.greedy_incumbent()'s docstring; what one thread computes is clu_incumbent.h.
// ================================================================================================================
struct IncProb {
    i64 col0, rbits_off, inf_off;     // RoundProb's: first column; the tint's first I / C word; the informative row
    i64 conf_off, pair0, pair1;       // the problem's R x cw conflict matrix (uint32 words); its pairs, as columns, in the round's pair list
    i64 grp0;                         // its first gap group, numbered through the batch
    i64 slot0, mrow_off;              // its starts' first result slot; their member rows' first word (cw words a start)
    i64 max_lg;                       // MAX_ISOFORM_LG: the tint's summed segment lengths, the slack of the gap rows of a column outside the set
    int n, n_seg, w, cw, n_starts, n_seeds;   // columns, segments, words per row, words per column set; starts = n_seeds + 1 (the last is empty)
};

constexpr i64 kIncNoCost = 0x7fffffffffffffffll;   // cost2 of a start that is not feasible
constexpr int kIncMaxCols = 32768;    // columns of one problem: delta2 stays inside 32 bits (2 x 9600 x 32769 < 2^31) and a start is blockIdx.y

// the smallest of the workgroup's 256 keys, in every thread; s_key: 4 words of LDS; synchronises before it returns
__device__ __forceinline__ u64 block_min_key(u64 v, u64 *s_key) {
    for (int s = 32; s > 0; s >>= 1) { const u64 o = __shfl_xor(v, s); v = o < v ? o : v; }
    if (lane_id() == 0) s_key[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 r = s_key[0];
    for (int x = 1; x < 4; ++x) r = s_key[x] < r ? s_key[x] : r;
    __syncthreads();
    return r;
}

// Each problem's remaining pairs as a symmetric R x R bit matrix (zeroed before the launch).  A workgroup per problem; OR does not depend
// on the order the atomics arrive in.  A pair with an end outside the problem's columns cannot come from k_round, and sets nothing.
__global__ void __launch_bounds__(256) k_inc_conflict(const int *list, const IncProb *probs, const int2 *pairs, unsigned *conf) {
    const IncProb d = probs[list[blockIdx.x]];
    for (i64 i = d.pair0 + threadIdx.x; i < d.pair1; i += 256) {
        const int2 pr = pairs[i];
        const bool ok = (unsigned)pr.x < (unsigned)d.n && (unsigned)pr.y < (unsigned)d.n;
        const int a = inc_clamp(pr.x, 0, d.n - 1), b = inc_clamp(pr.y, 0, d.n - 1);
        if (ok) {
            atomicOr(&conf[d.conf_off + (i64)a * d.cw + (b >> 5)], 1u << (b & 31));
            atomicOr(&conf[d.conf_off + (i64)b * d.cw + (a >> 5)], 1u << (a & 31));
        }
    }
}

// dynamic LDS of k_inc_start for one problem: cnt (a counter per bit of a row), the member and the blocked bit rows, and (LDS) the I and
// C rows at k_round's stride
inline size_t inc_lds_bytes(int R, int W, int CW, bool rows) { return 4 * ((size_t)W * 32 + 2 * (size_t)CW + (rows ? 2 * (size_t)R * (size_t)(W | 1) : 0)); }

// A workgroup per (problem, start): blockIdx.x = the problem (through list), blockIdx.y = the start.  Grow, repair and score of that one
// start, whole, with every loop bounded by R; the candidates (grow) and the members (repair) are spread over the threads and a step's
// choice is ONE packed key reduced over the workgroup (smaller delta2, then smaller column; more violated rows, then smaller column).
// LDS: the rows (ANDed with the informative row) are staged as in k_round; !LDS: read where preprocess left them and ANDed on the way.
// Results per start: cost2, the two step counts and the member bit row; k_inc_pick chooses.  No workgroup reads another's.
template <bool LDS>
__global__ void __launch_bounds__(256) k_inc_start(const int *list, const IncProb *probs, const unsigned *ibits, const unsigned *cbits, const int *rids,
                                                   const unsigned *inf_bits, const unsigned *conf, const int *g2, const i64 *col_row_off, i64 n_rows,
                                                   const int *rows, const i64 *grp_seg_off, const int *grp_seg, const int *grp_len, i64 n_grp,
                                                   i64 n_grp_seg, double lo_f, double hi_f, int offset, i64 *cost2, int *steps, unsigned *mrows) {
    extern __shared__ unsigned s_dyn[];
    __shared__ unsigned s_E[kMaxWords], s_inf[kMaxWords];
    __shared__ u64 s_key[4];
    __shared__ i64 s_sum[4];
    __shared__ int s_bad[4];
    const IncProb d = probs[list[blockIdx.x]];
    const int k = blockIdx.y;
    if (k >= d.n_starts) return;                              // (the grid's height is the batch's largest count of starts)
    const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    const int R = d.n, W = d.w, M = d.n_seg, CW = d.cw, S = W | 1;
    int *s_cnt = reinterpret_cast<int *>(s_dyn);
    unsigned *s_mem = s_dyn + W * 32, *s_blk = s_mem + CW, *s_rows = s_blk + CW;
    const int *prids = rids + d.col0;
    const int *pg2 = g2 + d.col0;
    for (int x = tid; x < W * 32; x += 256) s_cnt[x] = 0;
    for (int x = tid; x < 2 * CW; x += 256) s_mem[x] = 0u;   // (member and blocked rows lie side by side)
    for (int w = tid; w < W; w += 256) { s_E[w] = 0u; s_inf[w] = inf_bits[d.inf_off + w]; }
    __syncthreads();
    if (LDS) {
        for (int x = tid; x < R * W; x += 256) {
            const int c = x / W, w = x - c * W;
            const i64 src = d.rbits_off + (i64)prids[c] * W + w;
            s_rows[c * S + w] = ibits[src] & s_inf[w];
            s_rows[(R + c) * S + w] = cbits[src] & s_inf[w];
        }
        __syncthreads();
    }
    const unsigned *inf = LDS ? nullptr : s_inf;             // (the staged rows carry the informative row already)
    const auto row_i = [&](int c) { return LDS ? s_rows + c * S : ibits + d.rbits_off + (i64)prids[c] * W; };
    const auto row_c = [&](int c) { return LDS ? s_rows + (R + c) * S : cbits + d.rbits_off + (i64)prids[c] * W; };
    const auto add = [&](int c) {                             // c is the workgroup's: E, cnt, blocked and the member row take column c
        const unsigned *ri = row_i(c), *rc = row_c(c);
        for (int w = tid; w < W; w += 256) inc_add_word(ri[w] & s_inf[w], rc[w] & s_inf[w], w, s_E, s_cnt);
        for (int w = tid; w < CW; w += 256) s_blk[w] |= conf[d.conf_off + (i64)c * CW + w];
        if (tid == 0) s_mem[c >> 5] |= 1u << (c & 31);
        __syncthreads();
    };
    const int seed = inc_start_col(k, d.n_seeds, R);
    if (seed >= 0 && seed < R) add(seed);
    int grow = 0, repair = 0;
    for (int step = 0; step < R; ++step) {                    // ---- grow
        u64 key = kIncKeyNone;
        for (int c = tid; c < R; c += 256) {
            if (inc_bit(s_mem, c) || inc_bit(s_blk, c)) continue;
            const u64 kk = inc_grow_key(inc_delta2(row_i(c), row_c(c), inf, W, s_E, s_cnt, pg2[c]), c);
            key = kk < key ? kk : key;
        }
        key = block_min_key(key, s_key);
        if (key == kIncKeyNone || inc_key_delta2(key) >= 0) break;
        add(inc_clamp(inc_key_col(key), 0, R - 1));
        ++grow;
    }
    for (int step = 0; step < R; ++step) {                    // ---- repair: at most one member leaves a step
        u64 key = kIncKeyNone;
        for (int c = tid; c < R; c += 256) {
            if (!inc_bit(s_mem, c)) continue;
            i64 r0 = col_row_off[d.col0 + c], r1 = col_row_off[d.col0 + c + 1];
            r0 = r0 < 0 ? 0 : r0 > n_rows ? n_rows : r0;
            r1 = r1 < r0 ? r0 : r1 > n_rows ? n_rows : r1;
            const int bad = inc_violations(r0, r1, rows, d.grp0, n_grp, grp_seg_off, n_grp_seg, grp_seg, grp_len, M, s_E, lo_f, hi_f, (i64)offset);
            if (bad) { const u64 kk = inc_repair_key(bad, c); key = kk < key ? kk : key; }
        }
        key = block_min_key(key, s_key);
        if (key == kIncKeyNone) break;
        const int out = inc_clamp(inc_key_col(key), 0, R - 1);
        if (tid == 0) s_mem[out >> 5] &= ~(1u << (out & 31));
        for (int w = tid; w < W; w += 256) s_E[w] = 0u;
        __syncthreads();
        const int stripes = W >= 256 ? 1 : 256 / W;           // E again from the members that are left (OR: any order)
        for (int x = tid; x < stripes * W; x += 256) {
            const int st = x / W, w = x - st * W;
            unsigned o = 0u;
            for (int c = st; c < R; c += stripes) if (inc_bit(s_mem, c)) o |= row_i(c)[w] & s_inf[w];
            if (o) atomicOr(&s_E[w], o);
        }
        __syncthreads();
        ++repair;
    }
    i64 sum = 0;                                              // ---- score, from scratch; a violated row of a column outside the set (its
    int bad_out = 0;                                          //      slack is MAX_ISOFORM_LG, no more) leaves the start without a cost
    for (int c = tid; c < R; c += 256) {
        const bool in = inc_bit(s_mem, c);
        sum += inc_score_col(in, row_c(c), inf, W, s_E, pg2[c]);
        if (!in) {
            i64 r0 = col_row_off[d.col0 + c], r1 = col_row_off[d.col0 + c + 1];
            r0 = r0 < 0 ? 0 : r0 > n_rows ? n_rows : r0;
            r1 = r1 < r0 ? r0 : r1 > n_rows ? n_rows : r1;
            bad_out += inc_violations(r0, r1, rows, d.grp0, n_grp, grp_seg_off, n_grp_seg, grp_seg, grp_len, M, s_E, lo_f, hi_f, (i64)offset + d.max_lg);
        }
    }
    for (int s = 32; s > 0; s >>= 1) { sum += __shfl_xor(sum, s); bad_out += __shfl_xor(bad_out, s); }
    if (lane == 0) { s_sum[wave] = sum; s_bad[wave] = bad_out; }
    __syncthreads();
    if (tid == 0) {
        cost2[d.slot0 + k] = s_bad[0] + s_bad[1] + s_bad[2] + s_bad[3] ? kIncNoCost : s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        steps[2 * (d.slot0 + k)] = grow; steps[2 * (d.slot0 + k) + 1] = repair;
    }
    for (int w = tid; w < CW; w += 256) mrows[d.mrow_off + (i64)k * CW + w] = s_mem[w];
}

// A workgroup per problem: the feasible start with the smallest cost2, at equal cost2 the earliest; its cost2, number and step counts, and its
// members, ascending, at the front of the problem's own columns of mem_cols (mem_cnt of them; the host lays them end to end).
__global__ void __launch_bounds__(256) k_inc_pick(const int *list, const IncProb *probs, const i64 *cost2, const int *steps, const unsigned *mrows,
                                                  i64 *out_cost2, int *out_start, int *out_grow, int *out_repair, int *mem_cols, int *mem_cnt) {
    __shared__ i64 s_cost[256];
    __shared__ int s_start[256];
    __shared__ i64 s_wave[4];
    const int p = list[blockIdx.x], tid = threadIdx.x;
    const IncProb d = probs[p];
    i64 best = kIncNoCost;
    int at = 0x7fffffff;
    for (int k = tid; k < d.n_starts; k += 256) {            // (k ascends: a thread keeps its earliest)
        const i64 v = cost2[d.slot0 + k];
        if (v < best) { best = v; at = k; }
    }
    s_cost[tid] = best; s_start[tid] = at;
    __syncthreads();
    for (int x = 0; x < 256; ++x)
        if (s_cost[x] < best || (s_cost[x] == best && s_start[x] < at)) { best = s_cost[x]; at = s_start[x]; }
    if (best == kIncNoCost) return;                           // no feasible start: the problem keeps cost2 = -1, start = -1 and no member
    at = inc_clamp(at, 0, d.n_starts - 1);
    if (tid == 0) { out_cost2[p] = best; out_start[p] = at; out_grow[p] = steps[2 * (d.slot0 + at)]; out_repair[p] = steps[2 * (d.slot0 + at) + 1]; }
    i64 carry = 0;
    for (int w0 = 0; w0 < d.cw; w0 += 256) {
        const int w = w0 + tid;
        unsigned m = w < d.cw ? mrows[d.mrow_off + (i64)at * d.cw + w] : 0u;
        i64 total;
        i64 x = carry + block_scan(__popc(m), total, s_wave);
        while (m) { if (x < d.n) mem_cols[d.col0 + x] = w * 32 + __ffs((int)m) - 1; ++x; m &= m - 1; }
        carry += total;
    }
    if (tid == 0) mem_cnt[p] = (int)(carry < d.n ? carry : d.n);
}

// ================================================================================================================
// The exact solve of a round's small problems (fclu_round_exact): a problem of R <= 24 columns has 2^R column sets, each a few bit
// operations on the transposed model (per informative segment the mask of its support and of the columns with C = 1; per column the mask
// of its conflicts; per gap-group segment its support mask beside its length).  Every set is evaluated and the smallest
// (cost2, mask) is the proven optimum.  The definition is cluster_solve.exact_small()'s docstring; what one thread computes is clu_exact.h.
// ================================================================================================================
struct ExactProb {
    i64 col0, inf0;                   // first column (its conflict word and g2); first informative segment, numbered through the batch (table: 2 words each)
    i64 pair0, pair1;                 // its pairs, as columns, in the round's pair list
    i64 grp0, grp1, row0, row1;       // its gap groups and gap rows, numbered through the batch
    i64 max_lg;                       // MAX_ISOFORM_LG: the slack of the gap rows of a column outside the set
    int n, n_inf;                     // columns (<= 24), informative segments (<= 32 kMaxWords)
};

constexpr int kExactWgMasks = 4096;           // masks one workgroup evaluates (16 a thread): staging the table is a small share of it
constexpr i64 kExactLaunchMasks = 1ll << 24;  // masks one launch evaluates (profiles/cluster_exact.txt: the longest launch stays far under 50 ms)
constexpr int kExactMaxLaunches = 4096;       // launches of one call (an event each)
constexpr int kExactLdsBytes = 80 * 1024;     // the reduction's 4 keys, 2 x 9600 table words, 2 x 24 words of conflicts and g2

// the support word (W: 32 bits for the exact solve, 64 for the branch and bound) of informative segment k (numbered through the batch);
// sup_off closes with n_sup, which the device array does not hold
template <typename W>
__device__ __forceinline__ W sup_word(i64 k, const i64 *sup_off, i64 n_inf, const int *sup_cols, i64 n_sup, int R) {
    const i64 a = ex_clamp(sup_off[k], 0, n_sup), b = ex_clamp(k + 1 < n_inf ? sup_off[k + 1] : n_sup, a, n_sup);
    W m = 0;
    for (i64 s = a; s < b; ++s) { const int c = sup_cols[s]; if ((unsigned)c < (unsigned)R) m |= W(1) << c; }
    return m;
}

// A workgroup per taken problem of at most 8 sizeof(W) columns: its transposed table (zeroed before the launch: the support words are stored,
// the correction words and the conflict words are ORed in, which does not depend on the order the atomics arrive in) and its groups' support
// words.  fclu_round_exact runs it with 32-bit words, fclu_round_bnb with 64-bit ones.
template <typename W>
__global__ void __launch_bounds__(256) k_narrow_prep(const int *list, const ExactProb *probs, const int *inf_seg, const i64 *sup_off, i64 n_inf, const int *sup_cols,
                                                     i64 n_sup, const i64 *corr_off, i64 n_cols, const int *corr_seg, i64 n_corr, const int2 *pairs,
                                                     const i64 *grp_seg_off, const int *grp_seg, i64 n_grp_seg, W *tab, W *conf, W *gsup) {
    const ExactProb d = probs[list[blockIdx.x]];
    const int R = d.n, E = d.n_inf, tid = threadIdx.x;
    const int *inf = inf_seg + d.inf0;
    for (int k = tid; k < E; k += 256) tab[2 * (d.inf0 + k)] = sup_word<W>(d.inf0 + k, sup_off, n_inf, sup_cols, n_sup, R);
    for (int c = 0; c < R; ++c) {
        const i64 a = ex_clamp(corr_off[d.col0 + c], 0, n_corr), b = ex_clamp(d.col0 + c + 1 < n_cols ? corr_off[d.col0 + c + 1] : n_corr, a, n_corr);
        for (i64 x = a + tid; x < b; x += 256) {
            const int k = ex_find_seg(inf, E, corr_seg[x]);
            if (k >= 0) atomicOr(&tab[2 * (d.inf0 + k) + 1], W(1) << c);
        }
    }
    for (i64 i = d.pair0 + tid; i < d.pair1; i += 256) {
        const int2 pr = pairs[i];
        if ((unsigned)pr.x < (unsigned)R && (unsigned)pr.y < (unsigned)R) {
            atomicOr(&conf[d.col0 + pr.x], W(1) << pr.y);
            atomicOr(&conf[d.col0 + pr.y], W(1) << pr.x);
        }
    }
    if (d.grp1 > d.grp0) {
        const i64 s0 = ex_clamp(grp_seg_off[d.grp0], 0, n_grp_seg), s1 = ex_clamp(grp_seg_off[d.grp1], s0, n_grp_seg);
        for (i64 s = s0 + tid; s < s1; s += 256) {
            const int k = ex_find_seg(inf, E, grp_seg[s]);
            gsup[s] = k >= 0 ? sup_word<W>(d.inf0 + k, sup_off, n_inf, sup_cols, n_sup, R) : W(0);
        }
    }
}

// A workgroup per item = (problem, first mask, masks): the problem's table, conflict words and g2 are staged in LDS (every lane reads the
// same word: a broadcast), a lane takes every 256th mask of the slice, and the slice's smallest key reaches the problem's word by one
// atomic minimum, whose result does not depend on the order the slices arrive in.  No workgroup waits for another; every loop is bounded
// by the slice and the table sizes.
__global__ void __launch_bounds__(256) k_exact_search(const int4 *items, const ExactProb *probs, const unsigned *tab, const unsigned *conf, const int *g2,
                                                      const int *rows, i64 n_rows, const i64 *grp_seg_off, i64 n_grp, i64 n_grp_seg, const unsigned *gsup,
                                                      const int *grp_len, double lo_f, double hi_f, int offset, u64 *best) {
    extern __shared__ __attribute__((aligned(16))) unsigned s_exact[];
    const int4 it = items[blockIdx.x];
    const ExactProb d = probs[it.x];
    const int R = d.n, E = d.n_inf, tid = threadIdx.x;
    u64 *s_key = reinterpret_cast<u64 *>(s_exact);
    unsigned *s_tab = s_exact + 8, *s_conf = s_tab + 2 * E;
    int *s_g2 = reinterpret_cast<int *>(s_conf + R);
    for (int x = tid; x < 2 * E; x += 256) s_tab[x] = tab[2 * d.inf0 + x];
    if (tid < R) { s_conf[tid] = conf[d.col0 + tid]; s_g2[tid] = g2[d.col0 + tid]; }
    __syncthreads();
    const i64 r0 = ex_clamp(d.row0, 0, n_rows), r1 = ex_clamp(d.row1, r0, n_rows);
    const unsigned lo = (unsigned)it.y, n = (unsigned)it.z;
    u64 key = kExactKeyNone;
    for (unsigned i = tid; i < n; i += 256) {
        const u64 kk = ex_mask_key(lo + i, s_tab, E, s_conf, s_g2, R, r0, r1, rows, d.grp0, n_grp, grp_seg_off, n_grp_seg, gsup, grp_len, lo_f, hi_f, offset,
                                   d.max_lg);
        key = kk < key ? kk : key;
    }
    key = block_min_key(key, s_key);
    if (tid == 0 && key != kExactKeyNone) atomicMin(&best[it.x], key);
}

// ================================================================================================================
// The branch and bound over a round's problems of up to 64 columns (fclu_round_bnb): a problem's first D = min(R, depth) columns are
// fixed by a task number, a lane runs one task depth first with the bound, the row test and the leaf test of clu_bnb.h, and the
// smallest (cost2, mask) over a problem's tasks is its proven optimum when no task ran into node_cap.  The definition is
// cluster_solve.exact_bnb()'s docstring.  The tables are k_narrow_prep's with 64-bit words; the problems' descriptor is ExactProb.
// ================================================================================================================
constexpr int kBnbWgTasks = 256;               // tasks one workgroup runs: one a lane
constexpr i64 kBnbLaunchNodes = 1ll << 24;     // task-nodes of budget (tasks x node_cap) one launch holds (profiles/cluster_bnb.txt)
constexpr int kBnbMaxLaunches = 4096;          // launches of one call (an event each)
constexpr int kBnbMaxDepth = 20;               // 2^20 tasks a problem at the most
constexpr int kBnbLdsBytes = 160 * 1024;       // a workgroup's LDS on this part: 16 bytes an informative segment, 12 a column
constexpr int kBnbMaxInf = (kBnbLdsBytes - 12 * kBnbMaxCols) / 16;      // 10 192 informative segments (a row holds 32 kMaxWords = 9 600: every model fits)
static_assert(kBnbMaxInf < (1 << kBnbPlanes), "bnb_lb2 counts a column's corrections in kBnbPlanes bits");

struct BnbTask { i64 cost2; u64 mask; int nodes, capped; };      // a task's result (BnbResult of clu_bnb.h)

// A workgroup per item = (problem, first task, tasks <= 256, -): the problem's table, conflict words and g2 are staged in LDS, lane i runs
// task first + i and writes its result to the problem's place task_off[problem] + task of the per-task array.  Tasks share nothing and no
// workgroup waits for another; every loop is bounded by R, the table sizes or node_cap.
__global__ void __launch_bounds__(256) k_bnb_search(const int4 *items, const ExactProb *probs, const u64 *tab, const u64 *conf, const int *g2, const i64 *ub2,
                                                    const int *rows, i64 n_rows, const i64 *grp_seg_off, i64 n_grp, i64 n_grp_seg, const u64 *gsup,
                                                    const int *grp_len, double lo_f, double hi_f, int offset, int depth, int node_cap, const i64 *task_off,
                                                    BnbTask *tasks) {
    extern __shared__ __attribute__((aligned(16))) u64 s_bnb[];
    const int4 it = items[blockIdx.x];
    const ExactProb d = probs[it.x];
    const int R = d.n, E = d.n_inf, tid = threadIdx.x;
    u64 *s_tab = s_bnb, *s_conf = s_tab + 2 * E;
    int *s_g2 = reinterpret_cast<int *>(s_conf + R);
    for (int x = tid; x < 2 * E; x += 256) s_tab[x] = tab[2 * d.inf0 + x];
    if (tid < R) { s_conf[tid] = conf[d.col0 + tid]; s_g2[tid] = g2[d.col0 + tid]; }
    __syncthreads();
    if (tid >= it.z) return;
    BnbView v;
    v.tab = s_tab; v.conf = s_conf; v.g2 = s_g2; v.E = E; v.R = R;
    v.r0 = ex_clamp(d.row0, 0, n_rows); v.r1 = ex_clamp(d.row1, v.r0, n_rows); v.rows = rows;
    v.grp0 = d.grp0; v.n_grp = n_grp; v.grp_seg_off = grp_seg_off; v.n_grp_seg = n_grp_seg; v.gsup = gsup; v.grp_len = grp_len;
    v.lo_f = lo_f; v.hi_f = hi_f; v.offset = offset; v.max_lg = d.max_lg;
    const int D = R < depth ? R : depth;
    const u64 t = (u64)(unsigned)it.y + (u64)tid;
    if (t >> D) return;                                      // (no such task: the host cuts the items inside 2^D)
    const BnbResult r = bnb_task(v, t, D, ub2[it.x], node_cap);
    BnbTask out;
    out.cost2 = r.cost2; out.mask = r.mask; out.nodes = r.nodes; out.capped = r.capped;
    tasks[task_off[it.x] + (i64)t] = out;
}

struct BnbOut { i64 cost2; u64 mask; i64 nodes; i64 capped; };   // a problem's result: cost2 -1 and mask 0 when no task found a leaf

// A workgroup per taken problem: the smallest (cost2, mask) of its n_tasks tasks, their nodes summed, the capped ones counted.  A lane
// folds every 256th task and a tree in LDS folds the 256 partial results; a minimum and two sums, so nothing depends on an order.
__global__ void __launch_bounds__(256) k_bnb_reduce(const int *list, const i64 *task_off, const i64 *n_tasks, const BnbTask *tasks, BnbOut *out) {
    __shared__ BnbOut s_part[256];
    const int p = list[blockIdx.x], tid = threadIdx.x;
    const i64 t0 = task_off[p], n = n_tasks[p];
    BnbOut acc = {-1, 0ull, 0, 0};
    for (i64 t = tid; t < n; t += 256) {
        const BnbTask r = tasks[t0 + t];
        if (bnb_better(r.cost2, r.mask, acc.cost2, acc.mask)) { acc.cost2 = r.cost2; acc.mask = r.mask; }
        acc.nodes += r.nodes; acc.capped += r.capped ? 1 : 0;
    }
    s_part[tid] = acc;
    __syncthreads();
    for (int step = 128; step > 0; step >>= 1) {
        if (tid < step) {
            BnbOut a = s_part[tid];
            const BnbOut b = s_part[tid + step];
            if (bnb_better(b.cost2, b.mask, a.cost2, a.mask)) { a.cost2 = b.cost2; a.mask = b.mask; }
            a.nodes += b.nodes; a.capped += b.capped;
            s_part[tid] = a;
        }
        __syncthreads();
    }
    if (tid == 0) out[p] = s_part[0];
}

// ================================================================================================================
// The same search for problems of up to 1024 columns (fclu_round_bnb_wide): a column set is W = ceil(R / 64) words, a wave runs one
// task -- the walk of clu_bnb_wide.h, bw_task, whose control flow is the same in all its lanes -- and the lanes share a node's work:
// e_in and the blocked columns a word a lane, the columns' pieces of LB2 and the gap rows one a lane, a wave reduction for the sum and
// the verdict.  The definition is cluster_solve.exact_bnb_wide()'s docstring.
// ================================================================================================================
constexpr i64 kBwLaunchNodes = 1ll << 26;      // task-nodes of budget (tasks x node_cap) one launch holds (profiles/cluster_bnb_wide.txt)
constexpr int kBwMaxLaunches = 4096;           // launches of one call (an event each)
constexpr int kBwThreads = kBwWaves * kBwLanes;
constexpr int kBwMaxPasses = 16;               // passes of one fclu_round_bnb_wide_passes call
constexpr i64 kBwMaxPassTasks = 1ll << 16;     // a problem whose next pass would hold more tasks is not continued
constexpr int kBwFromItem = 8;                 // records a workgroup of a later pass walks, eight at a time.  Measured (profiles/cluster_bnb_wide_passes.txt): the
                                               // open subtrees of this workload are long walks, so a wave's second turn doubles the launch -- 8 / 64 / 512 records
                                               // an item give a longest launch of 29.7 / 88.2 / 88.5 ms at 490 columns and 4 096 nodes, and 18 ms each at 245

struct BwProb {
    ExactProb b;
    i64 tab0, conf0;                  // its first table word (icol, R x EW words, then ccol, EW x R words) and first conflict word (R x W words)
    int W, EW;
};

// A workgroup per taken problem: its tables by column, its conflict rows (all zeroed before the launch and ORed into, which does not depend
// on the order the atomics arrive in) and its groups' segments' places among the informative segments.
__global__ void __launch_bounds__(256) k_bw_prep(const int *list, const BwProb *probs, const int *inf_seg, const i64 *sup_off, i64 n_inf, const int *sup_cols, i64 n_sup,
                                                 const i64 *corr_off, i64 n_cols, const int *corr_seg, i64 n_corr, const int2 *pairs, const i64 *grp_seg_off,
                                                 const int *grp_seg, i64 n_grp_seg, u64 *tab, u64 *conf, int *gk) {
    const BwProb q = probs[list[blockIdx.x]];
    const ExactProb d = q.b;
    const int R = d.n, E = d.n_inf, W = q.W, EW = q.EW, tid = threadIdx.x;
    const int *inf = inf_seg + d.inf0;
    u64 *icol = tab + q.tab0, *ccol = icol + (i64)R * EW, *cf = conf + q.conf0;
    for (int k = tid; k < E; k += 256) {
        const i64 a = ex_clamp(sup_off[d.inf0 + k], 0, n_sup), b = ex_clamp(d.inf0 + k + 1 < n_inf ? sup_off[d.inf0 + k + 1] : n_sup, a, n_sup);
        for (i64 s = a; s < b; ++s) {
            const int c = sup_cols[s];
            if ((unsigned)c < (unsigned)R) atomicOr(&icol[(i64)c * EW + (k >> 6)], 1ull << (k & 63));
        }
    }
    for (int c = 0; c < R; ++c) {
        const i64 a = ex_clamp(corr_off[d.col0 + c], 0, n_corr), b = ex_clamp(d.col0 + c + 1 < n_cols ? corr_off[d.col0 + c + 1] : n_corr, a, n_corr);
        for (i64 x = a + tid; x < b; x += 256) {
            const int k = ex_find_seg(inf, E, corr_seg[x]);
            if (k >= 0) atomicOr(&ccol[(i64)(k >> 6) * R + c], 1ull << (k & 63));
        }
    }
    for (i64 i = d.pair0 + tid; i < d.pair1; i += 256) {
        const int2 pr = pairs[i];
        if ((unsigned)pr.x < (unsigned)R && (unsigned)pr.y < (unsigned)R) {
            atomicOr(&cf[(i64)pr.x * W + (pr.y >> 6)], 1ull << (pr.y & 63));
            atomicOr(&cf[(i64)pr.y * W + (pr.x >> 6)], 1ull << (pr.x & 63));
        }
    }
    if (d.grp1 > d.grp0) {
        const i64 s0 = ex_clamp(grp_seg_off[d.grp0], 0, n_grp_seg), s1 = ex_clamp(grp_seg_off[d.grp1], s0, n_grp_seg);
        for (i64 s = s0 + tid; s < s1; s += 256) gk[s] = ex_find_seg(inf, E, grp_seg[s]);
    }
}

// The lanes of a wave on the device (BwHostWave of clu_bnb_wide.h on the host).  sync: what a lane wrote to the wave's LDS state is
// there for the other lanes of the wave (they run in step; the fence keeps the compiler and the LDS counter in line).
struct BwDevWave {
    int lane;
    template <class F> __device__ __forceinline__ i64 sum(F f) {
        i64 x = f(lane);
        for (int s = 32; s > 0; s >>= 1) x += __shfl_xor(x, s);
        return x;
    }
    template <class F> __device__ __forceinline__ bool any(F f) { return __any(f(lane) ? 1 : 0) != 0; }
    template <class F> __device__ __forceinline__ void each(F f) { f(lane); }
    __device__ __forceinline__ void sync() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
};

struct BwTask { i64 cost2; int nodes, capped; u64 mask[kBwMaxWords]; };  // a task's result: cost2 -1 and an empty mask when it found no leaf

// What a pass leaves for the next one (fclu_round_bnb_wide_passes; all null for a single pass): per capped task its frame -- S, tried_in,
// tried_out of W words each and L | d << 32, at frame_off[problem] + task * (3 W + 1) words -- and per task the number of its open
// children (0 where it is not capped).
struct BwSplitOut { u64 *frames; const i64 *frame_off; int *open_cnt; };

// The body of k_bw_search and k_bw_search_from.  A workgroup per item = (problem, first task, tasks, -): the problem's tables by column and
// g2 are staged in LDS once, wave i runs the tasks first + i, first + i + 8, ... (k_bw_search's items hold at most 8) on its own state
// words behind them and writes the result to the problem's place task_off[problem] + task of the per-task array.  kFrom: a task's prefix
// and its length are a record of 1 + W words at rec_off[problem] + task * (1 + W); else task t is the prefix (t, D).  Tasks share nothing
// and no workgroup waits for another; every loop is bounded by R, the table sizes, the item's tasks or node_cap.  The items, the
// descriptors and their offsets (it.x, tab0, conf0, task_off, rec_off, frame_off) are the host's own, built and checked in
// bnb_wide_device before the launch, and are used as they are, as in k_bnb_search; what comes from the round's arrays and from the
// records is clamped.
template <bool kFrom>
__device__ __forceinline__ void bw_search_body(const int4 *items, const BwProb *probs, const u64 *tab, const u64 *conf, const int *g2, const i64 *bound,
                                               const int *rows, i64 n_rows, const i64 *grp_seg_off, i64 n_grp, i64 n_grp_seg, const int *gk, const int *grp_len,
                                               double lo_f, double hi_f, int offset, int depth, int node_cap, const i64 *task_off, BwTask *tasks, const u64 *rec,
                                               const i64 *rec_off, BwSplitOut so) {
    extern __shared__ __attribute__((aligned(16))) u64 s_bw[];
    const int4 it = items[blockIdx.x];
    const BwProb q = probs[it.x];
    const ExactProb d = q.b;
    const int R = d.n, E = d.n_inf, W = q.W, EW = q.EW, tid = threadIdx.x, wave = tid / kBwLanes;
    const i64 n_tab = 2ll * R * EW;
    const int n_st = bw_state_words(W, EW);
    u64 *s_state = s_bw + n_tab;
    int *s_g2 = reinterpret_cast<int *>(s_state + (i64)kBwWaves * n_st);
    for (i64 x = tid; x < n_tab; x += kBwThreads) s_bw[x] = tab[q.tab0 + x];
    for (int c = tid; c < R; c += kBwThreads) s_g2[c] = g2[d.col0 + c];
    __syncthreads();
    const int D = R < depth ? R : depth;
    BwView v;
    v.icol = s_bw; v.ccol = s_bw + (i64)R * EW; v.conf = conf + q.conf0; v.g2 = s_g2; v.E = E; v.R = R; v.W = W; v.EW = EW;
    v.r0 = ex_clamp(d.row0, 0, n_rows); v.r1 = ex_clamp(d.row1, v.r0, n_rows); v.rows = rows;
    v.grp0 = d.grp0; v.n_grp = n_grp; v.grp_seg_off = grp_seg_off; v.n_grp_seg = n_grp_seg; v.gk = gk; v.grp_len = grp_len;
    v.lo_f = lo_f; v.hi_f = hi_f; v.offset = offset; v.max_lg = d.max_lg;
    v.st = s_state + (i64)wave * n_st;
    BwDevWave wv = {tid % kBwLanes};
    const i64 b2 = bound[it.x];
    // (the first pass's items hold at most eight tasks: one turn, as before the passes)
    for (int i = wave; i < it.z; i = kFrom ? i + kBwWaves : it.z) {
        const u64 t = (u64)(unsigned)it.y + (u64)i;
        int L = D;
        BwResult r;
        if (kFrom) {
            const u64 *rc = rec + rec_off[it.x] + (i64)t * bw_record_words(W);
            L = (int)ex_clamp((i64)rc[0], 0, R);
            r = bw_task_from(v, wv, rc + 1, W, L, b2, node_cap);
        } else {
            if (t >> D) return;                              // (no such task: the host cuts the items inside 2^D)
            r = bw_task(v, wv, t, D, b2, node_cap);
        }
        wv.sync();
        BwTask *out = tasks + task_off[it.x] + (i64)t;
        if (wv.lane == 0) { out->cost2 = r.cost2; out->nodes = r.nodes; out->capped = r.capped; }
        if (wv.lane < kBwMaxWords) out->mask[wv.lane] = r.cost2 >= 0 && wv.lane < W ? v.st[4 * W + wv.lane] : 0ull;
        if (so.open_cnt) {
            int n_open = 0;
            if (r.capped && R > 0) {
                const u64 *S = v.st, *tin = S + 2 * W, *tout = S + 3 * W;
                const int dl = (int)ex_clamp(r.d, L, R - 1);
                n_open = bw_open_count(tout, L, dl, W, bw_open_include(wv, v.conf + (i64)dl * W, S, tin, dl, W));
                u64 *fr = so.frames + so.frame_off[it.x] + (i64)t * bw_frame_words(W);
                for (int x = wv.lane; x < W; x += kBwLanes) { fr[x] = S[x]; fr[W + x] = tin[x]; fr[2 * W + x] = tout[x]; }
                if (wv.lane == 0) fr[3 * W] = (u64)(unsigned)L | (u64)(unsigned)dl << 32;
            }
            if (wv.lane == 0) so.open_cnt[task_off[it.x] + (i64)t] = n_open;
        }
    }
}

// The first pass: task t of a problem's 2^D is the prefix (t, D), bounded by ub2.
__global__ void __launch_bounds__(kBwThreads) k_bw_search(const int4 *items, const BwProb *probs, const u64 *tab, const u64 *conf, const int *g2, const i64 *ub2,
                                                          const int *rows, i64 n_rows, const i64 *grp_seg_off, i64 n_grp, i64 n_grp_seg, const int *gk,
                                                          const int *grp_len, double lo_f, double hi_f, int offset, int depth, int node_cap, const i64 *task_off,
                                                          BwTask *tasks, BwSplitOut so) {
    bw_search_body<false>(items, probs, tab, conf, g2, ub2, rows, n_rows, grp_seg_off, n_grp, n_grp_seg, gk, grp_len, lo_f, hi_f, offset, depth, node_cap, task_off,
                          tasks, nullptr, nullptr, so);
}

// A later pass: the tasks are the records k_bw_emit wrote, bounded per problem by the smaller of ub2 and the best cost2 found so far.
__global__ void __launch_bounds__(kBwThreads) k_bw_search_from(const int4 *items, const BwProb *probs, const u64 *tab, const u64 *conf, const int *g2,
                                                               const i64 *bound, const int *rows, i64 n_rows, const i64 *grp_seg_off, i64 n_grp, i64 n_grp_seg,
                                                               const int *gk, const int *grp_len, double lo_f, double hi_f, int offset, int depth, int node_cap,
                                                               const i64 *task_off, BwTask *tasks, const u64 *rec, const i64 *rec_off, BwSplitOut so) {
    bw_search_body<true>(items, probs, tab, conf, g2, bound, rows, n_rows, grp_seg_off, n_grp, n_grp_seg, gk, grp_len, lo_f, hi_f, offset, depth, node_cap, task_off,
                         tasks, rec, rec_off, so);
}

// Behind a pass's search, a workgroup per problem of the pass: the exclusive scan of its tasks' open counts (a task's first record among
// the problem's) and their sum for the host, 256 tasks a step.
__global__ void __launch_bounds__(256) k_bw_split(const int *list, const i64 *task_off, const i64 *n_tasks, const int *open_cnt, i64 *open_off, i64 *n_open) {
    __shared__ i64 s_scan[256];
    const int p = list[blockIdx.x], tid = threadIdx.x;
    const i64 n = n_tasks[p], base = task_off[p];
    i64 running = 0;
    for (i64 lo = 0; lo < n; lo += 256) {
        const i64 t = lo + tid;
        const i64 mine = t < n ? ex_clamp(open_cnt[base + t], 0, kBwMaxCols + 1) : 0;
        s_scan[tid] = mine;
        __syncthreads();
        for (int step = 1; step < 256; step <<= 1) {
            const i64 add = tid >= step ? s_scan[tid - step] : 0;
            __syncthreads();
            s_scan[tid] += add;
            __syncthreads();
        }
        if (t < n) open_off[base + t] = running + s_scan[tid] - mine;
        running += s_scan[255];
        __syncthreads();
    }
    if (tid == 0) n_open[p] = running;
}

// In front of a pass's search, a workgroup per item of the pass before: wave i writes the open children of the item's capped tasks
// first + i, first + i + 8, ... as the records open_off[task] .. of the problem's range, which starts at rec_off[problem] (-1: the problem
// is not continued) and holds n_open[problem] records.  What the frames hold is clamped, and no record is written outside the range.
__global__ void __launch_bounds__(kBwThreads) k_bw_emit(const int4 *items, const BwProb *probs, const u64 *conf, const i64 *task_off, const u64 *frames,
                                                        const i64 *frame_off, const int *open_cnt, const i64 *open_off, const i64 *n_open, u64 *rec,
                                                        const i64 *rec_off) {
    const int4 it = items[blockIdx.x];
    const i64 r0 = rec_off[it.x], total = n_open[it.x];
    if (r0 < 0) return;
    const BwProb q = probs[it.x];
    const int R = q.b.n, W = q.W, wave = threadIdx.x / kBwLanes;
    if (R <= 0) return;
    BwDevWave wv = {(int)threadIdx.x % kBwLanes};
    for (int i = wave; i < it.z; i += kBwWaves) {
        const i64 t = (i64)it.y + i, at = task_off[it.x] + t;
        const i64 cnt = open_cnt[at], first = open_off[at];
        if (cnt <= 0 || first < 0 || first >= total) continue;
        const u64 *fr = frames + frame_off[it.x] + t * bw_frame_words(W);
        const int L = (int)ex_clamp((i64)(fr[3 * W] & 0xffffffffull), 0, R - 1), d = (int)ex_clamp((i64)(fr[3 * W] >> 32), L, R - 1);
        const bool inc = bw_open_include(wv, conf + q.conf0 + (i64)d * W, fr, fr + W, d, W);
        bw_open_emit(wv, fr, fr + 2 * W, L, d, W, inc, rec + r0 + first * bw_record_words(W), cnt < total - first ? cnt : total - first);
    }
}

struct BwOut { i64 cost2, task, nodes, capped; };             // a problem's result: cost2 -1 when no task found a leaf; task: the one whose set it is

// A workgroup per taken problem: the smallest (cost2, mask) of its n_tasks tasks as that task's number, their nodes summed, the capped
// ones counted; then the set's 16 words.  A lane folds every 256th task and a tree in LDS folds the 256 partial results; a minimum and
// two sums, so nothing depends on an order (two tasks never hold the same set).
__global__ void __launch_bounds__(256) k_bw_reduce(const int *list, const BwProb *probs, const i64 *task_off, const i64 *n_tasks, const BwTask *tasks, BwOut *out,
                                                   u64 *out_mask) {
    __shared__ BwOut s_part[256];
    const int p = list[blockIdx.x], tid = threadIdx.x, W = probs[p].W;
    const i64 n = n_tasks[p];
    const BwTask *mine = tasks + task_off[p];
    BwOut acc = {-1, 0, 0, 0};
    for (i64 t = tid; t < n; t += 256) {
        const BwTask &r = mine[t];
        if (bw_better(r.cost2, r.mask, acc.cost2, mine[acc.task].mask, W)) { acc.cost2 = r.cost2; acc.task = t; }
        acc.nodes += r.nodes; acc.capped += r.capped ? 1 : 0;
    }
    s_part[tid] = acc;
    __syncthreads();
    for (int step = 128; step > 0; step >>= 1) {
        if (tid < step) {
            BwOut a = s_part[tid];
            const BwOut b = s_part[tid + step];
            if (bw_better(b.cost2, mine[b.task].mask, a.cost2, mine[a.task].mask, W)) { a.cost2 = b.cost2; a.task = b.task; }
            a.nodes += b.nodes; a.capped += b.capped;
            s_part[tid] = a;
        }
        __syncthreads();
    }
    const BwOut r = s_part[0];
    if (tid == 0) out[p] = r;
    if (tid < kBwMaxWords) out_mask[(i64)p * kBwMaxWords + tid] = r.cost2 >= 0 ? mine[r.task].mask[tid] : 0ull;
}

// the bound a problem's next pass starts at: the smaller of ub2 (< 0: none) and the best cost2 found so far (< 0: none); -1: none
__device__ __forceinline__ i64 bw_next_bound(i64 ub2, i64 cost2) { return cost2 < 0 ? ub2 : ub2 < 0 || cost2 < ub2 ? cost2 : ub2; }

// Behind k_bw_reduce, a lane per problem of the first pass.
__global__ void __launch_bounds__(256) k_bw_bound(const int *list, int n_list, const i64 *ub2, const BwOut *out, i64 *bound) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= n_list) return;
    const int p = list[x];
    bound[p] = bw_next_bound(ub2[p], out[p].cost2);
}

// k_bw_reduce for a later pass: a workgroup per problem of the pass folds its tasks as k_bw_reduce does and then folds that into the
// problem's running result -- the smaller (cost2, mask), the nodes summed, the open tasks those of this pass -- and sets the next bound.
__global__ void __launch_bounds__(256) k_bw_fold(const int *list, const BwProb *probs, const i64 *task_off, const i64 *n_tasks, const BwTask *tasks, const i64 *ub2,
                                                 BwOut *out, u64 *out_mask, i64 *bound) {
    __shared__ BwOut s_part[256];
    __shared__ u64 s_prev[kBwMaxWords];
    const int p = list[blockIdx.x], tid = threadIdx.x, W = probs[p].W;
    const i64 n = n_tasks[p];
    const BwTask *mine = tasks + task_off[p];
    if (tid < kBwMaxWords) s_prev[tid] = out_mask[(i64)p * kBwMaxWords + tid];
    BwOut acc = {-1, 0, 0, 0};
    for (i64 t = tid; t < n; t += 256) {
        const BwTask &r = mine[t];
        if (bw_better(r.cost2, r.mask, acc.cost2, mine[acc.task].mask, W)) { acc.cost2 = r.cost2; acc.task = t; }
        acc.nodes += r.nodes; acc.capped += r.capped ? 1 : 0;
    }
    s_part[tid] = acc;
    __syncthreads();
    for (int step = 128; step > 0; step >>= 1) {
        if (tid < step) {
            BwOut a = s_part[tid];
            const BwOut b = s_part[tid + step];
            if (bw_better(b.cost2, mine[b.task].mask, a.cost2, mine[a.task].mask, W)) { a.cost2 = b.cost2; a.task = b.task; }
            a.nodes += b.nodes; a.capped += b.capped;
            s_part[tid] = a;
        }
        __syncthreads();
    }
    const BwOut r = s_part[0], before = out[p];
    const bool better = n > 0 && bw_better(r.cost2, mine[r.task].mask, before.cost2, s_prev, W);
    __syncthreads();                                         // (every lane has read out[p] and s_prev)
    const i64 cost2 = better ? r.cost2 : before.cost2;
    if (tid == 0) {
        out[p] = BwOut{cost2, r.task, before.nodes + r.nodes, r.capped};
        bound[p] = bw_next_bound(ub2[p], cost2);
    }
    if (better && tid < kBwMaxWords) out_mask[(i64)p * kBwMaxWords + tid] = mine[r.task].mask[tid];
}

// ================================================================================================================
// The read-out of a round (fclu_round_readout): run_ilp()'s isoform (py/freddie_cluster.py:601-635; cluster.read_out) of every problem
// with an accepted column set, from the rows the context holds -- the reps' I, C and label rows, the round's informative rows and rids.
// What a lane computes per word is clu_readout.h.
// ================================================================================================================
struct ReadoutProb {
    i64 col0, rbits_off, lab_off, inf_off, sel0, exon0, corr0, e0, slot0;   // first column (in rids); the tint's first I / C word and first label word; the
                                                                             // informative (and exon) row's first word; the set's first member (in sel); the
                                                                             // first byte of the exon row, of the members' rows and of e; first lane slot
    int n, n_sel, n_seg, w, lw, n_reps, n_e, g_log2;                         // columns, members, segments, bit and label words per row, the tint's reps, the
                                                                             // informative segments, log2 of the lanes a member gets
};

// the rep (local to the tint) of column c, column and rep clamped
__device__ __forceinline__ i64 readout_rep(const ReadoutProb &d, const int *rids, int c) {
    return ro_clamp(rids[d.col0 + ro_clamp(c, 0, d.n - 1)], 0, d.n_reps - 1);
}

// A workgroup per problem with a set: lanes across the words, a loop over the members for the OR of their I words; with the informative
// word and column 0's the exon word (kept in ex_bits, laid out as inf_bits, for k_readout_corr), then the row as bytes 0 / 1 and e, the exon
// bits at the informative segments in ascending order (a prefix sum of the words' counts).
__global__ void __launch_bounds__(256) k_readout_exons(const ReadoutProb *probs, const int *rids, const int *sel, const unsigned *ibits, const unsigned *inf_bits,
                                                       unsigned *ex_bits, unsigned char *exons, unsigned char *e) {
    __shared__ unsigned s_ex[kMaxWords], s_inf[kMaxWords];
    __shared__ i64 s_wave[4];
    const int tid = threadIdx.x;
    const ReadoutProb d = probs[blockIdx.x];
    if (d.n <= 0 || d.n_reps <= 0) return;                       // (the host gives no such problem a set)
    const int W = min(max(d.w, 1), kMaxWords), M = min(max(d.n_seg, 0), 32 * W);
    const i64 row0 = d.rbits_off + readout_rep(d, rids, 0) * d.w;
    for (int w = tid; w < W; w += 256) {
        unsigned acc = 0u;
        for (int m = 0; m < d.n_sel; ++m) acc |= ibits[d.rbits_off + readout_rep(d, rids, sel[d.sel0 + m]) * d.w + w];
        const unsigned valid = ro_valid(M, w), inf = inf_bits[d.inf_off + w] & valid;
        const unsigned ex = ro_exon_word(acc, ibits[row0 + w], inf, valid);
        s_ex[w] = ex; s_inf[w] = inf;
        ex_bits[d.inf_off + w] = ex;
    }
    __syncthreads();
    for (int k = tid; 4 * k < M; k += 256) {                     // four segments a lane: one store where the row starts at a multiple of 4
        const unsigned v = ro_exon_bytes4(s_ex[k >> 3], k & 7);
        unsigned char *out = exons + d.exon0 + 4 * k;
        if (!(d.exon0 & 3) && 4 * k + 3 < M) *reinterpret_cast<unsigned *>(out) = v;
        else for (int b = 0; b < 4 && 4 * k + b < M; ++b) out[b] = (unsigned char)(v >> (8 * b));
    }
    i64 carry = 0;
    for (int w0 = 0; w0 < W; w0 += 256) {
        const int w = w0 + tid;
        unsigned m = w < W ? s_inf[w] : 0u;
        const unsigned ex = w < W ? s_ex[w] : 0u;
        i64 total;
        i64 x = carry + block_scan(__popc(m), total, s_wave);
        for (; m; m &= m - 1, ++x)
            if (x < d.n_e) e[d.e0 + x] = (unsigned char)((ex >> (__ffs((int)m) - 1)) & 1u);
        carry += total;
    }
}

// A lane per (member, bit word), k_rows' grouping: a member gets g = 2^g_log2 lanes (the smallest power of two that holds its W words, 64
// at the most) and a problem's slots start at a multiple of 64, so a wave works on one problem and one-word rows do not cost a wave each.
// A lane reads its two label words, its C word, the informative and the exon word and writes its up to 32 characters: 16 at a time where
// the address is a multiple of 16, alone at the ragged ends and in rows that start elsewhere (ro_store_halves).  No lane writes a byte of
// another's.
__global__ void __launch_bounds__(256) k_readout_corr(int n_set, i64 n_slots, const ReadoutProb *probs, const int *rids, const int *sel, const unsigned *labels,
                                                      const unsigned *cbits, const unsigned *inf_bits, const unsigned *ex_bits, unsigned char *corr) {
    const int lane = lane_id();
    const i64 wave_g = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((i64)gridDim.x * blockDim.x) >> 6;
    for (i64 s0 = wave_g * 64; s0 < n_slots; s0 += n_waves * 64) {
        int lo = 0, hi = n_set - 1;                               // the last problem whose slots start at or before s0 (wave-uniform)
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (probs[mid].slot0 <= s0) lo = mid; else hi = mid - 1; }
        const ReadoutProb d = probs[__builtin_amdgcn_readfirstlane(lo)];
        const int g_log2 = min(max(d.g_log2, 0), 6), g = 1 << g_log2, sub = lane & (g - 1);
        const i64 m = (s0 - d.slot0 + lane) >> g_log2;
        if (m < 0 || m >= d.n_sel || d.n <= 0 || d.n_reps <= 0) continue;
        const int W = min(max(d.w, 1), kMaxWords), M = min(max(d.n_seg, 0), 32 * W), LW = max(d.lw, 1);
        const i64 rep = readout_rep(d, rids, sel[d.sel0 + m]);
        const unsigned *lab = labels + d.lab_off + rep * LW, *cb = cbits + d.rbits_off + rep * d.w;
        const i64 row = d.corr0 + m * (i64)M;
        for (int w = sub; w < W; w += g) {
            const int nv = ro_word_segs(M, w);
            const u64 x = (u64)lab[min(2 * w, LW - 1)] | (2 * w + 1 < LW ? (u64)lab[2 * w + 1] << 32 : 0ull);
            const unsigned cw = cb[w], inf = inf_bits[d.inf_off + w] & ro_valid(M, w), ex = ex_bits[d.inf_off + w];
            unsigned char *out = corr + row + 32 * w;
            const int halves = ro_store_halves((u64)(row + 32 * w), nv);
            if (halves & 1)
                *reinterpret_cast<uint4 *>(out) = make_uint4(ro_corr_bytes4(x, cw, inf, ex, 0), ro_corr_bytes4(x, cw, inf, ex, 1), ro_corr_bytes4(x, cw, inf, ex, 2),
                                                             ro_corr_bytes4(x, cw, inf, ex, 3));
            if (halves & 2)
                *reinterpret_cast<uint4 *>(out + 16) = make_uint4(ro_corr_bytes4(x, cw, inf, ex, 4), ro_corr_bytes4(x, cw, inf, ex, 5), ro_corr_bytes4(x, cw, inf, ex, 6),
                                                                  ro_corr_bytes4(x, cw, inf, ex, 7));
            for (int b = (halves & 2) ? 32 : (halves & 1) ? 16 : 0; b < nv; ++b) out[b] = (unsigned char)ro_corr_byte(x, cw, inf, ex, b);
        }
    }
}

}  // namespace

// ---- buffers and the context -------------------------------------------------------------------------------------------
// Memory that lives with the context and only ever grows: T *p is used as it is, bytes(n) serves the copies, the destructor frees.
// kPinned: pinned host memory (HostBuf<T>) instead of device memory.
template <typename T, bool kPinned = false>
struct Buf {
    T *p = nullptr;
    size_t cap = 0;                                          // bytes
    Buf() = default;
    Buf(const Buf &) = delete;
    ~Buf() { (void)release(); }
    static size_t bytes(size_t n) { return n * sizeof(T); }
    hipError_t release() {
        const hipError_t e = !p ? hipSuccess : kPinned ? hipHostFree(p) : hipFree(p);
        p = nullptr; cap = 0;
        return e;
    }
    hipError_t alloc(size_t n_bytes) {                       // exactly n_bytes; p is null before it
        void *q = nullptr;
        const hipError_t e = kPinned ? hipHostMalloc(&q, n_bytes, hipHostMallocDefault) : hipMalloc(&q, n_bytes);
        if (e == hipSuccess) { p = static_cast<T *>(q); cap = n_bytes; }
        return e;
    }
    hipError_t grow(size_t n) {                              // never shrinks; room for n elements and a quarter of slack, at least 16 bytes
        if (p && bytes(n) <= cap) return hipSuccess;
        const hipError_t e = release();
        return e != hipSuccess ? e : alloc((n ? bytes(n) : 16) + bytes(n) / 4);
    }
};
template <typename T> using HostBuf = Buf<T, true>;

constexpr int kBurst = 4;     // gated passes (pruning, components) enqueued per host round trip

struct fclu_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // every event, one list to create and destroy; by stage: the graph (ev), fclu_partition (pev), _preprocess (qev), _group_reads (gev), _round_models (rev),
    // _round_incumbents (iev), _round_exact's prep (xev), _round_bnb's prep and reduction (bev), _round_readout (oev), _round_bnb_wide's prep and reduction (wev).
    // launch_ev: an event in front of and behind every search launch of the round call that is running, created as a call needs them (the
    // calls follow one another on the stream and each reads its times before it returns)
    hipEvent_t events[3 + 6 + 6 + 5 + 5 + 4 + 2 + 3 + 3 + 3] = {};
    hipEvent_t *const ev = events, *const pev = ev + 3, *const qev = pev + 6, *const gev = qev + 6, *const rev = gev + 5, *const iev = rev + 5, *const xev = iev + 4, *const bev = xev + 2, *const oev = bev + 3, *const wev = oev + 3;
    std::vector<hipEvent_t> launch_ev;
    std::string err;
    float compat_ms = 0.f, prune_ms = 0.f;
    int32_t paths[FCLU_N_PATHS] = {};     // the last graph call's launch census and the last read-out's (fclu_last_paths)
    Buf<TintDesc> tints; Buf<int4> tiles; Buf<int2> word_tint; Buf<i64> tint_word0;
    Buf<unsigned> bits; Buf<unsigned char> tail; Buf<u64> adj[2], deg1;
    Buf<int> row_tint, first, last, deg, small_tints, small_rounds;
    Buf<int> pass_any;        // a burst's flags: kBurst "this pass changed something" words, then (pruning) kBurst x n_tint per-tint words
    HostBuf<int> h_flags;     // their pinned copy
    // fclu_partition(): the batch the last graph call left on the device, work arrays, results (pinned, context-owned)
    std::vector<TintDesc> h_tints;
    int adj_cur = 0;
    float components_ms = 0.f, pairs_ms = 0.f;
    Buf<int> parent, rows, sval, comp_start, comp_end, chunk_end, d_label, d_nodes, mem, d_part_rids;
    Buf<i64> head, part_id, smult, rid_pos, cnt, pair_base, d_tint_part_off, d_part_node_off, d_part_rid_off, d_part_pair_off, mem_off;
    Buf<unsigned> skey; Buf<int2> d_pairs; Buf<char> tmp;
    HostBuf<i64> h_tot;       // {partitions, pairs}
    HostBuf<int64_t> h_tint_part_off, h_part_node_off, h_part_rid_off, h_part_pair_off;
    HostBuf<int32_t> h_part_nodes, h_part_rids, h_label; HostBuf<int2> h_pairs;
    fclu_parts parts = {};
    bool have_parts = false;
    // The dedupe's scratch, one set for both of its users (the reps' dedupe of fclu_preprocess, the reads' grouping of fclu_group_reads):
    // the keys and their sort, the buckets' heads and starts, the leaders, their scan (id: the class numbering, n + 1 entries), the second
    // sort's input, rocPRIM's temporary storage, and the three refusal words with their pinned copy.  What makes the sharing sound: a
    // stage's use of it ends before that stage returns (dedupe_classes .. dedupe_members, on the one stream), and nothing in it is a result
    // or a round's source -- those are the stages' own (pd / gd, c->mem / c->mem_off; pd.ibits, pd.cbits and d_pairs feed the rounds).
    struct Dedupe {
        Buf<u64> key, skey; Buf<unsigned> nkey, snkey; Buf<char> tmp;
        Buf<int> val, sval, head, bstart, leader, flag, id, nval, err;
        HostBuf<int> h_err;
    } dd;
    // fclu_preprocess() / fclu_partition_reads(): device arrays (pd) and the pinned copies fclu_preprocess_results() hands out (ph)
    struct {
        Buf<PrepTint> tints; Buf<unsigned char> tail; Buf<i64> row_off;
        Buf<unsigned> labels, ibits, cbits;
        Buf<int> rfirst, rlast, first, last, rep_tint, rep_node, node_rep;
    } pd;
    struct {
        HostBuf<int64_t> row_off, bits_off, adj_off, rbits_off, mem_off;
        HostBuf<uint32_t> ibits, cbits, bits; HostBuf<uint8_t> ntail;
        HostBuf<int32_t> first, last, rfirst, rlast, rep_node, node_rep, mem, nfirst, nlast;
    } ph;
    float rows_ms = 0.f, dedupe_ms = 0.f;
    fclu_prep prep = {};
    bool have_prep = false;
    // fclu_group_reads() / fclu_partition_segment(): device arrays (gd) and the pinned copies fclu_group_results() hands out (gh)
    struct {
        Buf<GroupTint> tints; Buf<unsigned char> tail; Buf<i64> tok_off, rep_off, rep_lab_off, mem_off;
        Buf<unsigned> labels, tok;
        Buf<int> read_tint, read_rep, mem, rep_first;
    } gd;
    struct {
        HostBuf<int64_t> rep_off, rep_lab_off, mem_off; HostBuf<int32_t> read_rep, mem, rep_first;
    } gh;
    float gkeys_ms = 0.f, gdedupe_ms = 0.f;
    fclu_groups groups = {};
    bool have_groups = false;
    // fclu_round_setup() / fclu_round_models(): what the last fclu_partition_reads() / fclu_partition_segment() left on the device is the
    // source (pd.ibits / pd.cbits, d_pairs); device arrays (rd), the pinned copies fclu_round_results() hands out (rh), and what the host
    // keeps of the batch to check and lay out a round's problems
    struct {
        Buf<RoundProb> probs; Buf<u64> key, skey; Buf<unsigned> inf_bits; Buf<int2> pairs; Buf<char> tmp;
        Buf<i64> gap_off, col_row_off, prob_row_off, cnt, scan, head, gid, grp_cnt, grp_seg_off, grp_off, sup_off, corr_off;
        Buf<int> gaps, seg_len, col_of, rids, col_prob, list, val, sval, rows, grp, grp_prob, refused, inf_seg, sup_cols, corr_seg, grp_seg, grp_len;
    } rd;
    struct {
        HostBuf<int64_t> scan, inf_bits_off, inf_off, sup_off, col_off, corr_off, pair_off, grp_off, grp_seg_off, row_off;
        HostBuf<uint32_t> inf_bits; HostBuf<int2> pairs;
        HostBuf<int32_t> refused, inf_seg, sup_cols, corr_seg, grp, grp_seg, grp_len, rows;
    } rh;
    std::vector<int64_t> r_rep_off, r_gap_off, r_seg_off, r_rep_part, r_max_lg;
    std::vector<int64_t> r_lab_off;           // per tint the first label word of its reps' rows in pd.labels (the read-out's)
    std::vector<int32_t> r_n_seg, r_part_tint, r_rep_stamp, r_part_stamp;
    int r_epoch = 0;
    bool round_src_ok = false, round_ready = false;
    bool rounds_resident = false;             // the last fclu_round_models call was fclu_round_models_resident: c->rounds names the small arrays only
    float rcount_ms = 0.f, rgaps_ms = 0.f, rfill_ms = 0.f;
    fclu_rounds rounds = {};
    bool have_rounds = false;
    // fclu_round_incumbents(): the last fclu_round_models() call's device arrays (rd) are the input and r_probs is what the host kept of its
    // problems; device arrays (id: the conflict matrices, per start cost2 / step counts / member rows, per problem the choice) and the pinned
    // copies fclu_round_incumbent_results() hands out (ih; mem_cols / mem_cnt are the members as the device leaves them, a problem's at its
    // own columns, which the host lays end to end into mem)
    std::vector<RoundProb> r_probs;
    struct {
        Buf<IncProb> probs; Buf<unsigned> conf, mrows; Buf<i64> start_cost2, cost2;
        Buf<int> list, g2, steps, start, grow, repair, mem_cols, mem_cnt;
    } id;
    struct {
        HostBuf<int64_t> cost2, mem_off; HostBuf<int32_t> start, grow, repair, mem, mem_cols, mem_cnt;
    } ih;
    float iconf_ms = 0.f, istart_ms = 0.f, ipick_ms = 0.f;
    fclu_incumbents incs = {};
    bool have_incs = false;
    // fclu_round_exact(), fclu_round_bnb(), fclu_round_bnb_wide(): the same input.  One driver serves the three (run_round_call and the
    // helpers in front of it); a call owns its device arrays and the pinned copies its _results() hands out.  RoundCallBufs is what every call
    // uploads (the work items, the taken problems' list, g2), SearchBufs what the two searches add (the bounds, per problem its first task and
    // task count); SearchHost is the searches' pinned side (a result per problem as the device leaves it, and the arrays of fclu_bnb).
    struct RoundCallBufs { Buf<int4> items; Buf<int> list, g2; };
    struct SearchBufs : RoundCallBufs { Buf<i64> ub2, task_off, n_tasks; };
    template <typename Out> struct SearchHost { HostBuf<Out> out; HostBuf<int64_t> cost2, nodes; HostBuf<uint64_t> mask; HostBuf<int32_t> status, capped; };
    // fclu_round_exact(): xd adds the problems, the transposed tables, the conflict words, the groups' support words and a key per problem
    struct : RoundCallBufs {
        Buf<ExactProb> probs; Buf<unsigned> tab, conf, gsup; Buf<u64> best;
    } xd;
    struct {
        HostBuf<u64> best; HostBuf<int64_t> cost2; HostBuf<uint32_t> mask;
    } xh;
    float xprep_ms = 0.f, xsearch_ms = 0.f, xlongest_ms = 0.f;
    fclu_exact exact = {};
    bool have_exact = false;
    // fclu_round_bnb(): bd adds the problems, the 64-bit tables, conflict words and groups' support words, a result per task and per problem
    struct : SearchBufs {
        Buf<ExactProb> probs; Buf<u64> tab, conf, gsup; Buf<BnbTask> tasks; Buf<BnbOut> out;
    } bd;
    SearchHost<BnbOut> bh;
    float bprep_ms = 0.f, bsearch_ms = 0.f, blongest_ms = 0.f;
    fclu_bnb bnb = {};
    bool have_bnb = false;
    // fclu_round_bnb_wide(): wd adds the problems, the tables by column, the conflict rows, the group segments' places, a result per task
    // and per problem with its 16 mask words
    // fclu_round_bnb_wide_passes(): what a pass leaves for the next (ps, by the pass's parity: the emit in front of pass k + 1 reads pass k's
    // while pass k + 1's are sized), the records, and per problem their first word, the open children, the bound and the pass's task count
    struct BwPassBufs { Buf<int4> items; Buf<i64> task_off, frame_off, open_off; Buf<u64> frames; Buf<int> open_cnt; };
    struct : SearchBufs {
        Buf<BwProb> probs; Buf<u64> tab, conf, out_mask; Buf<BwTask> tasks; Buf<BwOut> out; Buf<int> gk;
        BwPassBufs ps[2]; Buf<u64> rec; Buf<i64> rec_off, n_open, bound;
    } wd;
    SearchHost<BwOut> wh;
    HostBuf<int64_t> w_n_open;
    std::vector<int64_t> w_pass_stats;                       // five numbers a pass that ran
    float wprep_ms = 0.f, wsearch_ms = 0.f, wlongest_ms = 0.f;
    fclu_bnb_wide wide = {};
    bool have_wide = false;
    // fclu_round_readout(): the same input and the reps' rows (pd.ibits / cbits / labels); device arrays (od: the problems with a set, the
    // sets, the exon words, the three outputs) and the pinned copies fclu_round_readout_results() hands out (oh)
    struct {
        Buf<ReadoutProb> probs; Buf<int> sel; Buf<unsigned> ex_bits; Buf<unsigned char> exons, corr, e;
    } od;
    struct {
        HostBuf<int64_t> exon_off, mem_off, corr_off, e_off; HostBuf<uint8_t> exons, corr, e;
    } oh;
    float oexon_ms = 0.f, ocorr_ms = 0.f;
    fclu_readout readout = {};
    bool have_readout = false;
    // (the buffers free themselves behind it, on this device)
    ~fclu_ctx() {
        (void)hipSetDevice(device);
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
        for (hipEvent_t e : events) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : launch_ev) if (e) (void)hipEventDestroy(e);
    }
};

namespace {

// ---- helpers: errors, test knobs, the burst loop -------------------------------------------------------------------------
std::string g_create_error;

int fail(fclu_ctx *c, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_error = buf;
    return code;
}

#define HIP_TRY(c, expr) \
    do { hipError_t e__ = (expr); if (e__ != hipSuccess) return fail((c), FCLU_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e__)); } while (0)
#define RC_TRY(expr) \
    do { const int rc__ = (expr); if (rc__ != FCLU_OK) return rc__; } while (0)

// Test knobs: environment variables read at the start of every entry point that runs kernels (the tests flip them between calls on
// one context) and handed down to the stages.
//   FCLU_PART_LDS=0         part_lds         no tint's components in one workgroup's LDS (k_cc_lds): all take the per-pass kernels
//   FCLU_PRUNE_LDS=0        prune_lds        the same for the pruning (k_prune_lds)
//   FCLU_PRUNE_LDS_WORDS=n  prune_lds_words  0 < n < kPruneLdsWords: a lower limit of k_prune_lds, so that small tints take both ways in one batch
//   FCLU_RANK=0             rank             k_compat keeps the masked sums whatever the rows' length
//   FCLU_PRUNE_EDGES=0      prune_edges      the pass as OR of rows (k_deg1, k_prune) whatever the shapes
//   FCLU_HASH_BITS=n        hash_mask        n < 32: the dedupe's hash cut to n bits forces collisions; 0: one bucket a tint
//   FCLU_ROUND_LDS=0        round_lds        no problem's rows in LDS (k_round<true, .>): all read them from device memory
//   FCLU_ROUND_LDS_BYTES=n  round_lds_bytes  0 < n < kRoundLdsBytes: a lower limit of the LDS path, so that small problems take both ways in one batch
//   FCLU_EXACT_SLICE=n      exact_slice      0 < n < kExactWgMasks: fclu_round_exact gives a workgroup n masks and a launch 16 n, so that a small problem crosses
//                                            many slices and several launches
//   FCLU_BNB_SLICE=n        bnb_slice        n > 0: fclu_round_bnb gives a launch n tasks (and a workgroup min(n, 256)), so that a problem crosses several launches
//   FCLU_BNB_WIDE_SLICE=n   bnb_wide_slice   n > 0: fclu_round_bnb_wide gives a launch n tasks (and a workgroup min(n, 8)), so that a problem crosses several launches
//                                            (every pass of fclu_round_bnb_wide_passes)
//   FCLU_BNB_WIDE_ITEM=n    bnb_wide_item    0 < n <= 4096: the records a workgroup of a later pass of fclu_round_bnb_wide_passes walks (kBwFromItem; profiles)
//   FCLU_GRID_CAP=n         grid_cap         n >= 1: every launch of capped_grid() takes min(its own grid, n) workgroups, so that a small batch runs the
//                                            kernels' grid-stride loops more than once (1: one workgroup does everything)
struct Knobs {
    bool part_lds, prune_lds, rank, prune_edges, round_lds;
    i64 prune_lds_words, round_lds_bytes, exact_slice, bnb_slice, bnb_wide_slice, bnb_wide_item, grid_cap;
    unsigned hash_mask;
};

Knobs read_knobs() {
    const auto off = [](const char *name) { const char *e = getenv(name); return e && e[0] == '0'; };
    Knobs k;
    k.part_lds = !off("FCLU_PART_LDS"); k.prune_lds = !off("FCLU_PRUNE_LDS"); k.rank = !off("FCLU_RANK"); k.prune_edges = !off("FCLU_PRUNE_EDGES");
    const char *w = getenv("FCLU_PRUNE_LDS_WORDS");
    k.prune_lds_words = (w && atoll(w) > 0 && atoll(w) < kPruneLdsWords) ? atoll(w) : kPruneLdsWords;
    k.round_lds = !off("FCLU_ROUND_LDS");
    const char *rb = getenv("FCLU_ROUND_LDS_BYTES");
    k.round_lds_bytes = (rb && atoll(rb) > 0 && atoll(rb) < kRoundLdsBytes) ? atoll(rb) : kRoundLdsBytes;
    const char *xs = getenv("FCLU_EXACT_SLICE");
    k.exact_slice = (xs && atoll(xs) > 0 && atoll(xs) < kExactWgMasks) ? atoll(xs) : 0;
    const char *bs = getenv("FCLU_BNB_SLICE");
    k.bnb_slice = (bs && atoll(bs) > 0 && atoll(bs) < (1ll << 30)) ? atoll(bs) : 0;
    const char *ws = getenv("FCLU_BNB_WIDE_SLICE");
    k.bnb_wide_slice = (ws && atoll(ws) > 0 && atoll(ws) < (1ll << 30)) ? atoll(ws) : 0;
    const char *wi = getenv("FCLU_BNB_WIDE_ITEM");
    k.bnb_wide_item = (wi && atoll(wi) > 0 && atoll(wi) <= 4096) ? atoll(wi) : kBwFromItem;
    const char *hb = getenv("FCLU_HASH_BITS");
    k.hash_mask = (hb && hb[0] >= '0' && hb[0] <= '9' && atoi(hb) < 32) ? (1u << atoi(hb)) - 1u : 0xffffffffu;
    const char *gc = getenv("FCLU_GRID_CAP");
    k.grid_cap = (gc && atoll(gc) >= 1 && atoll(gc) < (1ll << 30)) ? atoll(gc) : 0;
    return k;
}

// The grids that a constant caps: the kernel walks what lies beyond its grid in a grid-stride loop (no cluster kernel waits for another
// workgroup, so any grid from one workgroup up computes the same).  The tests read these names.
constexpr int kCapCompat = 8192;        // k_compat: a workgroup a tile
constexpr int kCapDegree = 4096;        // k_degree, k_deg1: a wave a row / an adjacency word column
constexpr int kCapPrune = 16384;        // k_prune: a wave a row
constexpr int kCapPruneEdges = 65536;   // k_prune_edges: a wave a (row, chunk)
constexpr int kCapRowGrid = 4096;       // a thread a row: k_cc_init, k_cc_jump, k_bounds, k_chunk, k_offsets
constexpr int kCapWaveGrid = 65536;     // a wave a row: k_cc_hook, k_pairs, k_members
constexpr int kCapItemGrid = 4096;      // a thread an item of the dedupe: k_heads, k_leader, k_nodes, k_mem_off, k_gleader, k_greps
constexpr int kCapSlots = 65536;        // a lane a slot: k_rows, k_gkeys, k_readout_corr
constexpr int kCapGather = 8192;        // k_ggather: a thread a label word
constexpr int kCapGaps = 4096;          // a thread a column, gap row or group: k_gap_keys, k_gap_heads, k_gap_groups, k_gap_fill

// the workgroups of such a launch: work units at share a workgroup, at most cap, and at most FCLU_GRID_CAP where that is set
unsigned capped_grid(i64 work, i64 share, int cap, const Knobs &k) {
    i64 grid = std::min<i64>((work + share - 1) / share, cap);
    if (k.grid_cap > 0) grid = std::min(grid, k.grid_cap);
    return (unsigned)grid;
}

// One burst: kBurst passes enqueued per host round trip, pass q gated on pass q - 1's "changed something" word, so the host reads the
// flags once per burst and not once per pass.  enqueue(q, any, gate) launches pass q, which sets *any.  The first n_flags words of d_flags
// (the kBurst pass words in front) are cleared before the passes and copied to h_flags behind them.  ran: the passes that ran, 0 .. the
// first that changed nothing (inclusive); done: one of them changed nothing.
template <typename F>
int run_burst(fclu_ctx *c, Buf<int> &d_flags, HostBuf<int> &h_flags, size_t n_flags, F &&enqueue, int &ran, bool &done) {
    hipStream_t s = c->stream;
    HIP_TRY(c, hipMemsetAsync(d_flags.p, 0, d_flags.bytes(n_flags), s));
    for (int q = 0; q < kBurst; ++q) enqueue(q, d_flags.p + q, q ? d_flags.p + (q - 1) : nullptr);
    HIP_TRY(c, hipMemcpyAsync(h_flags.p, d_flags.p, d_flags.bytes(n_flags), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    for (ran = 0, done = false; ran < kBurst && !done; ++ran) done = !h_flags.p[ran];
    return FCLU_OK;
}

// A result array: its pinned buffer grown to n elements, filled from the device (copy; the caller synchronises) and handed out as field.
template <typename H, typename D>
int fetch(fclu_ctx *c, HostBuf<H> &h, const D *src, size_t n, bool copy, const H *&field) {
    static_assert(sizeof(H) == sizeof(D), "one element size on the device and in pinned memory");
    HIP_TRY(c, h.grow(n));
    if (copy && n) HIP_TRY(c, hipMemcpyAsync(h.p, src, h.bytes(n), hipMemcpyDeviceToHost, c->stream));
    field = h.p;
    return FCLU_OK;
}

int bits_for(i64 n) { int b = 1; while (b < 32 && (1ll << b) < n) ++b; return b; }

// the *_timing entry points: two times of the last call, each wanted or not
int two_times(float *a, float va, float *b, float vb) { if (a) *a = va; if (b) *b = vb; return FCLU_OK; }

int three_times(float *a, float va, float *b, float vb, float *d, float vd) { if (d) *d = vd; return two_times(a, va, b, vb); }

// A round call's result struct, when the call stands (fclu_round_*_results; call: the entry point that makes it).
template <typename Result>
int round_call_results(fclu_ctx *c, bool have, const Result &r, Result *out, const char *call) {
    if (!have || !c->have_rounds) return fail(c, FCLU_ERR_ARG, "%s_results: no result (the last %s call failed, none was made, or a later call ended it)", call, call);
    *out = r;
    return FCLU_OK;
}

// ---- staging of a batch ------------------------------------------------------------------------------------------------------
// What the host derives from a batch's shape (stage_tints) and the graph kernels are launched with (compat_run).
struct Staged {
    int T = 0, n_tiles = 0, max_w = 1, max_aw_large = 0;
    i64 R = 0, n_bits = 0, n_adj = 0;
    bool any_large = false, empty = false;
    std::vector<int> small_tints;                        // pruned whole in LDS (k_prune_lds)
    size_t small_lds = 0;
    // what the uploads read: alive until the call that staged them has synchronised
    std::vector<TintDesc> tints;
    std::vector<int4> tiles;
    std::vector<int> row_tint;
    std::vector<int2> word_tint;                         // every adjacency word column of every tint: (tint, word)
    std::vector<i64> tint_word0;
};

// Tint t's descriptor from the batch's offsets, with the shape refusals: the kernels index with these and nothing else.  n_seg and
// bits_off null (fclu_partition_adj: a graph without rows): no segments, one word a row at offset 0.
int describe_tint(fclu_ctx *c, int t, const Knobs &k, int32_t prune, const int64_t *row_off, const int32_t *n_seg, const int64_t *bits_off,
                  const int64_t *adj_off, TintDesc &d) {
    d = TintDesc();
    d.row0 = row_off[t];
    const i64 n = row_off[t + 1] - d.row0;
    if (!n_seg && (n < 0 || n > (1 << 30))) return fail(c, FCLU_ERR_ARG, "tint %d: bad row count", t);
    if (n_seg && (n < 0 || n > (1 << 30) || n_seg[t] < 0)) return fail(c, FCLU_ERR_ARG, "tint %d: bad row count or segment count", t);
    d.n = (int)n; d.n_seg = n_seg ? n_seg[t] : 0;
    d.w = std::max((d.n_seg + 31) / 32, 1);
    d.aw = (d.n + 63) / 64;
    d.adj_off = adj_off[t];
    d.in_lds = (prune && k.prune_lds && d.n > 0 && d.n <= 65535 && (i64)d.n * d.aw <= k.prune_lds_words) ? 1 : 0;
    d.cc_lds = (k.part_lds && d.n > 0 && (i64)d.n * d.aw <= kPruneLdsWords) ? 1 : 0;      // (the pruning's criterion)
    if (bits_off) {
        d.bits_off = bits_off[t];
        if (bits_off[t + 1] - d.bits_off != (i64)d.n * d.w) return fail(c, FCLU_ERR_ARG, "tint %d: bits_off does not match rows x words", t);
    }
    if (adj_off[t + 1] - d.adj_off != (i64)d.n * d.aw) return fail(c, FCLU_ERR_ARG, "tint %d: adj_off does not match rows x words", t);
    if (d.w > kMaxWords) return fail(c, FCLU_ERR_UNSUPPORTED, "tint %d has %d segments; this build stages at most %d", t, d.n_seg, kMaxWords * 32);
    return FCLU_OK;
}

// The caller's rows of tint t: first / last / tail in range and the bits inside [first, last] (first / last ARE a read's first and last
// covered segment, :175-183): k_compat counts on it.
int check_rows(fclu_ctx *c, int t, const TintDesc &d, const fclu_batch *b) {
    for (i64 r = 0; r < d.n; ++r) {
        const int f = b->first[d.row0 + r], l = b->last[d.row0 + r];
        if (f < -1 || l >= (d.n_seg > 0 ? d.n_seg : 1) || b->tail[d.row0 + r] > 2) return fail(c, FCLU_ERR_ARG, "tint %d read %lld: first/last/tail out of range", t, r);
        const uint32_t *rw = b->bits + d.bits_off + r * d.w;
        for (int w = 0; w < d.w; ++w) {
            uint32_t allowed = 0;
            if (f >= 0 && l >= f && w >= (f >> 5) && w <= (l >> 5)) {
                allowed = 0xffffffffu;
                if (w == (f >> 5)) allowed &= 0xffffffffu << (f & 31);
                if (w == (l >> 5)) allowed &= 0xffffffffu >> (31 - (l & 31));
            }
            if (rw[w] & ~allowed) return fail(c, FCLU_ERR_ARG, "tint %d read %lld: a covered segment outside [first, last]", t, r);
        }
    }
    return FCLU_OK;
}

// The caller's matrix of tint t (fclu_partition_adj): symmetric, an empty diagonal, no bit at a column >= N (the kernels index nodes with its bits).
int check_adj(fclu_ctx *c, int t, const TintDesc &d, const uint64_t *adj) {
    const uint64_t *A = adj + d.adj_off;
    for (i64 r = 0; r < d.n; ++r)
        for (int z = 0; z < d.aw; ++z) {
            uint64_t word = A[r * d.aw + z];
            if (z == d.aw - 1 && (d.n & 63) && (word >> (d.n & 63)))
                return fail(c, FCLU_ERR_ARG, "tint %d row %lld: adjacency bit at a column beyond N = %d", t, r, d.n);
            while (word) {
                const i64 col = (i64)z * 64 + __builtin_ctzll(word);
                word &= word - 1;
                if (col == r) return fail(c, FCLU_ERR_ARG, "tint %d row %lld: adjacency bit on the diagonal", t, r);
                if (!((A[col * d.aw + (r >> 6)] >> (r & 63)) & 1ull))
                    return fail(c, FCLU_ERR_ARG, "tint %d: adjacency not symmetric: (%lld, %lld) set, (%lld, %lld) not", t, r, col, col, r);
            }
        }
    return FCLU_OK;
}

// the device buffers of a staged batch and of its graph
int grow_staged(fclu_ctx *c, const Staged &st) {
    const size_t R = (size_t)st.R, T = (size_t)st.T, n_words = st.word_tint.size();
    HIP_TRY(c, c->tints.grow(T)); HIP_TRY(c, c->tiles.grow(st.tiles.size())); HIP_TRY(c, c->bits.grow((size_t)st.n_bits)); HIP_TRY(c, c->tail.grow(R));
    for (Buf<int> *b : {&c->row_tint, &c->first, &c->last, &c->deg}) HIP_TRY(c, b->grow(R));
    HIP_TRY(c, c->adj[0].grow((size_t)st.n_adj)); HIP_TRY(c, c->adj[1].grow((size_t)st.n_adj));
    HIP_TRY(c, c->word_tint.grow(n_words)); HIP_TRY(c, c->tint_word0.grow(T + 1)); HIP_TRY(c, c->deg1.grow(n_words));
    HIP_TRY(c, c->pass_any.grow(kBurst * (T + 1))); HIP_TRY(c, c->h_flags.grow(kBurst * (T + 1)));
    HIP_TRY(c, c->small_tints.grow(st.small_tints.size() + 1)); HIP_TRY(c, c->small_rounds.grow(T));
    return FCLU_OK;
}

// the descriptors, tiles and maps of a staged batch to the device (st outlives the copies)
int upload_staged(fclu_ctx *c, const Staged &st) {
    hipStream_t s = c->stream;
    HIP_TRY(c, hipMemcpyAsync(c->tints.p, st.tints.data(), c->tints.bytes(st.tints.size()), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->tiles.p, st.tiles.data(), c->tiles.bytes(st.tiles.size()), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->row_tint.p, st.row_tint.data(), c->row_tint.bytes(st.row_tint.size()), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->word_tint.p, st.word_tint.data(), c->word_tint.bytes(st.word_tint.size()), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->tint_word0.p, st.tint_word0.data(), c->tint_word0.bytes(st.tint_word0.size()), hipMemcpyHostToDevice, s));
    return FCLU_OK;
}

// Host staging of a batch: the tints' descriptors, tiles and row / word maps, the device buffers grown and the maps uploaded.  b: the
// caller's rows, checked against their tint (fclu_compat_graph, fclu_partition), or null when the rows were made on the device
// (fclu_partition_reads: first / last / tail in range and bits inside [first, last] by construction).
int stage_tints(fclu_ctx *c, const Knobs &k, int T, const int64_t *row_off, const int32_t *n_seg, const int64_t *bits_off, const int64_t *adj_off,
                int32_t prune, const fclu_batch *b, Staged &st) {
    HIP_TRY(c, hipSetDevice(c->device));
    st.T = T; st.R = row_off[T]; st.n_bits = bits_off[T]; st.n_adj = adj_off[T];
    st.tints.assign((size_t)T, TintDesc()); st.row_tint.assign((size_t)st.R, 0); st.tint_word0.assign((size_t)T + 1, 0);
    for (int t = 0; t < T; ++t) {
        TintDesc &d = st.tints[(size_t)t];
        RC_TRY(describe_tint(c, t, k, prune, row_off, n_seg, bits_off, adj_off, d));
        if (d.in_lds) { st.small_tints.push_back(t); st.small_lds = std::max(st.small_lds, ((size_t)2 * d.n * d.aw + d.aw) * 8 + (size_t)d.n * 2 + 16); }
        else if (d.n > 0) { st.any_large = true; st.max_aw_large = std::max(st.max_aw_large, d.aw); }
        st.max_w = std::max(st.max_w, d.w);
        if (b) RC_TRY(check_rows(c, t, d, b));
        std::fill_n(st.row_tint.begin() + d.row0, d.n, t);
        for (int ti = 0; ti < d.aw; ++ti) for (int tj = ti; tj < d.aw; ++tj) st.tiles.push_back(make_int4(t, ti, tj, 0));   // (on and above the diagonal)
        for (int z = 0; z < d.aw; ++z) st.word_tint.push_back(make_int2(t, z));
        st.tint_word0[(size_t)t + 1] = (i64)st.word_tint.size();
    }
    st.n_tiles = (int)st.tiles.size();
    c->compat_ms = c->prune_ms = 0.f;
    std::fill_n(c->paths, FCLU_N_PATHS, 0);
    c->h_tints = st.tints;
    c->adj_cur = 0;
    st.empty = st.n_tiles == 0 || st.R == 0;
    if (st.empty) return FCLU_OK;
    RC_TRY(grow_staged(c, st));
    return upload_staged(c, st);
}

// ---- the graph: compatibility and pruning ----------------------------------------------------------------------------------
// The graph of a staged batch whose rows (c->bits / first / last / tail) are on the device: compatibility, then pruning.  The pruned
// matrix stays on the device in c->adj[c->adj_cur] (with the tints' descriptors in c->tints / c->h_tints and c->row_tint) for
// partition_device(); adj_out may be null.
int compat_run(fclu_ctx *c, const Staged &st, const Knobs &k, int32_t prune, uint64_t *adj_out, int32_t *rounds_out) {
    hipStream_t s = c->stream;
    const unsigned grid = capped_grid(st.n_tiles, 1, kCapCompat, k);
    // rows of at most kRankWords words: the rank tables ride along
    const bool rank = st.max_w <= kRankWords && k.rank;
    const size_t lds = (size_t)2 * kTile * (st.max_w | 1) * (rank ? 6 : 4);
    HIP_TRY(c, hipEventRecord(c->ev[0], s));
    hipLaunchKernelGGL(!rank ? k_compat<false> : k_compat<true>, dim3(grid), dim3(256), lds, s, st.n_tiles, c->tiles.p, c->tints.p, c->bits.p, c->first.p,
                       c->last.p, c->tail.p, c->adj[0].p);
    c->paths[FCLU_PATH_COMPAT_FORM] = rank ? FCLU_FORM_RANK : FCLU_FORM_MASKED;
    c->paths[FCLU_PATH_TILES] = st.n_tiles;
    HIP_TRY(c, hipEventRecord(c->ev[1], s));
    int cur = 0;
    if (prune && !st.small_tints.empty()) {
        // (the final matrix of such a tint goes into BOTH copies: whichever the per-pass kernels of the large tints end on holds it)
        HIP_TRY(c, hipMemcpyAsync(c->small_tints.p, st.small_tints.data(), c->small_tints.bytes(st.small_tints.size()), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_prune_lds, dim3((unsigned)st.small_tints.size()), dim3(256), st.small_lds, s, c->small_tints.p, c->tints.p, c->adj[0].p,
                           c->adj[1].p, c->small_rounds.p);
        c->paths[FCLU_PATH_LDS_TINTS] = (int32_t)st.small_tints.size();
    }
    if (prune && st.any_large) {
        // the loop of :240-255 usually ends after two or three passes
        const i64 R = st.R;
        const int T = st.T, n_words = (int)st.word_tint.size();
        const unsigned deg_grid = capped_grid(R, 4, kCapDegree, k);
        // the pass edge by edge (k_prune_edges) when every tint of the per-pass kernels has rows of at most kEdgeChunks x 64 words
        const bool edge_walk = st.max_aw_large <= kEdgeChunks * 64 && k.prune_edges;
        const int edge_chunks = (st.max_aw_large + 63) / 64 > 0 ? (st.max_aw_large + 63) / 64 : 1;
        c->paths[FCLU_PATH_PASS_KERNEL] = edge_walk ? FCLU_PASS_EDGE_WALK : FCLU_PASS_OR_OF_ROWS;
        c->paths[FCLU_PATH_EDGE_CHUNKS] = edge_walk ? edge_chunks : 0;
        int *d_changed = c->pass_any.p + kBurst;             // per pass and tint
        const int *h_changed = c->h_flags.p + kBurst;
        const auto pass = [&](int q, int *any, const int *gate) {
            const int from = cur ^ (q & 1), to = from ^ 1;
            hipLaunchKernelGGL(k_degree, dim3(deg_grid), dim3(256), 0, s, R, c->row_tint.p, c->tints.p, c->adj[from].p, c->deg.p, gate);
            if (edge_walk)
                hipLaunchKernelGGL(k_prune_edges, dim3(capped_grid(R * edge_chunks, 4, kCapPruneEdges, k)), dim3(256), 0, s, R, edge_chunks,
                                   c->row_tint.p, c->tints.p, c->adj[from].p, c->deg.p, c->adj[to].p, d_changed + (size_t)q * T, any, gate);
            else {
                hipLaunchKernelGGL(k_deg1, dim3(capped_grid(n_words, 4, kCapDegree, k)), dim3(256), 0, s, n_words, c->word_tint.p, c->tints.p,
                                   c->deg.p, c->deg1.p, gate);
                hipLaunchKernelGGL(k_prune, dim3(capped_grid(R, 4, kCapPrune, k)), dim3(256), 0, s, R, c->row_tint.p, c->tints.p, c->tint_word0.p,
                                   c->adj[from].p, c->deg.p, c->deg1.p, c->adj[to].p, d_changed + (size_t)q * T, any, gate);
            }
        };
        bool done = false;
        for (int burst = 0; burst < (1 << 18) && !done; ++burst) {
            int ran = 0;
            RC_TRY(run_burst(c, c->pass_any, c->h_flags, (size_t)kBurst * (T + 1), pass, ran, done));
            for (int q = 0; q < ran; ++q)
                if (rounds_out) for (int t = 0; t < T; ++t) if (h_changed[(size_t)q * T + t]) rounds_out[t] += 1;
            cur ^= ran & 1;                                  // (each pass that ran wrote the other buffer)
            c->paths[FCLU_PATH_PASSES_ENQUEUED] += kBurst;
            c->paths[FCLU_PATH_PASSES_RAN] += ran;
        }
    }
    HIP_TRY(c, hipEventRecord(c->ev[2], s));
    c->adj_cur = cur;
    if (adj_out) HIP_TRY(c, hipMemcpyAsync(adj_out, c->adj[cur].p, c->adj[cur].bytes((size_t)st.n_adj), hipMemcpyDeviceToHost, s));
    std::vector<int> small_rounds;
    if (prune && rounds_out && !st.small_tints.empty()) {
        small_rounds.resize((size_t)st.T);
        HIP_TRY(c, hipMemcpyAsync(small_rounds.data(), c->small_rounds.p, c->small_rounds.bytes((size_t)st.T), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    if (!small_rounds.empty()) for (int t : st.small_tints) rounds_out[t] = small_rounds[(size_t)t];
    HIP_TRY(c, hipGetLastError());
    (void)hipEventElapsedTime(&c->compat_ms, c->ev[0], c->ev[1]);
    (void)hipEventElapsedTime(&c->prune_ms, c->ev[1], c->ev[2]);
    return FCLU_OK;
}

// The graph of a batch of the caller's rows: staging with every check, the rows' upload, the kernels.
int compat_device(fclu_ctx *c, const Knobs &k, const fclu_batch *b, int32_t prune, uint64_t *adj_out, int32_t *rounds_out) {
    if (b->n_tint <= 0) return fail(c, FCLU_ERR_ARG, "fclu_compat_graph: empty batch");
    Staged st;
    RC_TRY(stage_tints(c, k, b->n_tint, b->row_off, b->n_seg, b->bits_off, b->adj_off, prune, b, st));
    if (rounds_out) for (int t = 0; t < st.T; ++t) rounds_out[t] = 0;
    if (st.empty) return FCLU_OK;
    hipStream_t s = c->stream;
    HIP_TRY(c, hipMemcpyAsync(c->bits.p, b->bits, c->bits.bytes((size_t)st.n_bits), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->first.p, b->first, c->first.bytes((size_t)st.R), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->last.p, b->last, c->last.bytes((size_t)st.R), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->tail.p, b->tail, c->tail.bytes((size_t)st.R), hipMemcpyHostToDevice, s));
    return compat_run(c, st, k, prune, adj_out, rounds_out);
}

// ---- partition_reads() behind the graph (:256-274) ---------------------------------------------------------------
int check_members(fclu_ctx *c, i64 R, const int64_t *mem_off, const int32_t *mem, int32_t maximum_ilp_size) {
    if (maximum_ilp_size < 1) return fail(c, FCLU_ERR_ARG, "maximum_ilp_size is %d: it must be at least 1", (int)maximum_ilp_size);
    if (R < 0 || R >= (1ll << 31)) return fail(c, FCLU_ERR_ARG, "bad row count %lld", R);
    if (!mem_off) return fail(c, FCLU_ERR_ARG, "mem_off is null");
    if (mem_off[0] != 0) return fail(c, FCLU_ERR_ARG, "mem_off[0] is %lld, not 0", (i64)mem_off[0]);
    for (i64 r = 0; r < R; ++r)
        if (mem_off[r + 1] < mem_off[r]) return fail(c, FCLU_ERR_ARG, "mem_off is not monotone at row %lld (%lld after %lld)", r, (i64)mem_off[r + 1], (i64)mem_off[r]);
    if (mem_off[R] > 0 && !mem) return fail(c, FCLU_ERR_ARG, "mem is null");
    return FCLU_OK;
}

// what the stages of one partition call share
struct PartRun {
    int T = 0, max_size = 1, end_bit = 1, row_grid = 1, wave_grid = 1;
    i64 R = 0, n_mem = 0, P = 0, n_pairs = 0;
    size_t sort_bytes = 0, scan_bytes = 0;
};

// The pair list, device and pinned: as large as the graphs make it, so exactly that, and a batch's that does not fit is refused.
int grow_pairs(fclu_ctx *c, i64 n_pairs) {
    const size_t need = c->d_pairs.bytes((size_t)n_pairs);
    if (n_pairs > 2147483647ll)
        return fail(c, FCLU_ERR_UNSUPPORTED, "%lld incompatible pairs in this batch: more than the 2147483647 a call returns", n_pairs);
    if (need > c->d_pairs.cap) {
        HIP_TRY(c, c->d_pairs.release());
        size_t free_b = 0, total_b = 0;
        HIP_TRY(c, hipMemGetInfo(&free_b, &total_b));
        if (need + (64u << 20) > free_b)
            return fail(c, FCLU_ERR_UNSUPPORTED, "%lld incompatible pairs in this batch (%lld bytes) do not fit the device's free memory (%lld bytes)",
                        n_pairs, n_pairs * 8, (i64)free_b);
        if (c->d_pairs.alloc(need) != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, FCLU_ERR_UNSUPPORTED, "%lld incompatible pairs in this batch: no device memory for %lld bytes", n_pairs, n_pairs * 8);
        }
    }
    if (need > c->h_pairs.cap || !c->h_pairs.p) {
        HIP_TRY(c, c->h_pairs.release());
        if (c->h_pairs.alloc(std::max<size_t>(need, 16)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, FCLU_ERR_UNSUPPORTED, "%lld incompatible pairs in this batch: no pinned host memory for %lld bytes", n_pairs, n_pairs * 8);
        }
    }
    return FCLU_OK;
}

// fclu_parts of the call: the pinned buffers grown, filled from the device (copy; the caller synchronises) and handed out
int part_results(fclu_ctx *c, const PartRun &p, bool copy) {
    fclu_parts &o = c->parts;
    const size_t T1 = (size_t)p.T + 1, P1 = (size_t)p.P + 1, R = (size_t)p.R;
    RC_TRY(fetch(c, c->h_tint_part_off, c->d_tint_part_off.p, T1, copy, o.tint_part_off));
    RC_TRY(fetch(c, c->h_part_node_off, c->d_part_node_off.p, P1, copy, o.part_node_off));
    RC_TRY(fetch(c, c->h_part_rid_off, c->d_part_rid_off.p, P1, copy, o.part_rid_off));
    RC_TRY(fetch(c, c->h_part_pair_off, c->d_part_pair_off.p, P1, copy, o.part_pair_off));
    RC_TRY(fetch(c, c->h_part_nodes, c->d_nodes.p, R, copy, o.part_nodes));
    RC_TRY(fetch(c, c->h_label, c->d_label.p, R, copy, o.label));
    RC_TRY(fetch(c, c->h_part_rids, c->d_part_rids.p, (size_t)p.n_mem, copy, o.part_rids));
    if (copy && p.n_pairs) HIP_TRY(c, hipMemcpyAsync(c->h_pairs.p, c->d_pairs.p, c->d_pairs.bytes((size_t)p.n_pairs), hipMemcpyDeviceToHost, c->stream));
    o.pairs = &c->h_pairs.p->x;                              // (grow_pairs: never null)
    o.n_tint = p.T; o.n_rows = p.R; o.n_part = p.P; o.n_rids = p.n_mem; o.n_pairs = p.n_pairs;
    return FCLU_OK;
}

// nothing but empty tints
int part_empty(fclu_ctx *c, int T) {
    PartRun p;
    p.T = T;
    RC_TRY(grow_pairs(c, 0));
    RC_TRY(part_results(c, p, false));
    memset(c->h_tint_part_off.p, 0, c->h_tint_part_off.bytes((size_t)T + 1));
    *c->h_part_node_off.p = *c->h_part_rid_off.p = *c->h_part_pair_off.p = 0;
    return FCLU_OK;
}

// The work arrays, the members' upload (mem_off null: on the device already) and the connected components: c->parent behind it.
int part_components(fclu_ctx *c, const Knobs &k, PartRun &p, const int64_t *mem_off, const int32_t *mem) {
    hipStream_t s = c->stream;
    const i64 R = p.R;
    std::vector<int> small;
    size_t small_lds = 0;
    bool any_large = false;
    for (int t = 0; t < p.T; ++t) {
        const TintDesc &d = c->h_tints[(size_t)t];
        if (d.cc_lds) { small.push_back(t); small_lds = std::max(small_lds, (size_t)d.n * d.aw * 8 + (size_t)d.n * 4); }
        else if (d.n > 0) any_large = true;
    }
    const size_t R1 = (size_t)R + 1;
    for (Buf<int> *b : {&c->parent, &c->rows, &c->sval, &c->comp_start, &c->comp_end, &c->chunk_end, &c->d_label, &c->d_nodes}) HIP_TRY(c, b->grow((size_t)R));
    for (Buf<i64> *b : {&c->head, &c->part_id, &c->smult, &c->rid_pos, &c->cnt, &c->pair_base, &c->d_part_node_off, &c->d_part_rid_off, &c->d_part_pair_off, &c->mem_off})
        HIP_TRY(c, b->grow(R1));
    HIP_TRY(c, c->skey.grow((size_t)R));
    HIP_TRY(c, c->d_tint_part_off.grow((size_t)p.T + 1));
    HIP_TRY(c, c->mem.grow((size_t)p.n_mem)); HIP_TRY(c, c->d_part_rids.grow((size_t)p.n_mem));
    HIP_TRY(c, c->small_tints.grow(small.size() + 1));
    HIP_TRY(c, c->pass_any.grow(kBurst)); HIP_TRY(c, c->h_flags.grow(kBurst)); HIP_TRY(c, c->h_tot.grow(2));
    p.end_bit = bits_for(R);
    unsigned *parent_key = reinterpret_cast<unsigned *>(c->parent.p);            // (the sort's keys: the roots, unsigned)
    HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, p.sort_bytes, parent_key, c->skey.p, c->rows.p, c->sval.p, (size_t)R, 0u, (unsigned)p.end_bit, s));
    HIP_TRY(c, rocprim::exclusive_scan(nullptr, p.scan_bytes, c->head.p, c->part_id.p, (i64)0, R1, rocprim::plus<i64>(), s));
    HIP_TRY(c, c->tmp.grow(std::max(p.sort_bytes, p.scan_bytes)));
    if (mem_off) {
        HIP_TRY(c, hipMemcpyAsync(c->mem_off.p, mem_off, c->mem_off.bytes(R1), hipMemcpyHostToDevice, s));
        if (p.n_mem) HIP_TRY(c, hipMemcpyAsync(c->mem.p, mem, c->mem.bytes((size_t)p.n_mem), hipMemcpyHostToDevice, s));
    }
    if (!small.empty()) HIP_TRY(c, hipMemcpyAsync(c->small_tints.p, small.data(), c->small_tints.bytes(small.size()), hipMemcpyHostToDevice, s));

    p.row_grid = (int)capped_grid(R + 1, 256, kCapRowGrid, k); p.wave_grid = (int)capped_grid(R, 4, kCapWaveGrid, k);    // (k_chunk: R + 1 entries)
    const u64 *d_adj = c->adj[c->adj_cur].p;
    HIP_TRY(c, hipEventRecord(c->pev[0], s));
    hipLaunchKernelGGL(k_cc_init, dim3(p.row_grid), dim3(256), 0, s, R, c->parent.p);
    hipLaunchKernelGGL(k_cc_init, dim3(p.row_grid), dim3(256), 0, s, R, c->rows.p);     // (the sort's values: the rows themselves)
    if (!small.empty())
        hipLaunchKernelGGL(k_cc_lds, dim3((unsigned)small.size()), dim3(256), small_lds, s, c->small_tints.p, c->tints.p, d_adj, c->parent.p);
    if (any_large) {
        const auto pass = [&](int, int *any, const int *gate) {
            hipLaunchKernelGGL(k_cc_hook, dim3(p.wave_grid), dim3(256), 0, s, R, c->row_tint.p, c->tints.p, d_adj, c->parent.p, any, gate);
            hipLaunchKernelGGL(k_cc_jump, dim3(p.row_grid), dim3(256), 0, s, R, c->row_tint.p, c->tints.p, c->parent.p, any, gate);
        };
        bool done = false;
        for (int burst = 0, ran = 0; !done; ++burst) {
            if (burst >= (1 << 16)) return fail(c, FCLU_ERR_HIP, "connected components did not converge");
            RC_TRY(run_burst(c, c->pass_any, c->h_flags, kBurst, pass, ran, done));
        }
    }
    HIP_TRY(c, hipEventRecord(c->pev[1], s));
    return FCLU_OK;
}

// The even split, the members' positions and the pair counts: behind it p.P and p.n_pairs, the call's totals.
int part_split(fclu_ctx *c, const Knobs &k, PartRun &p) {
    hipStream_t s = c->stream;
    const i64 R = p.R;
    const size_t R1 = (size_t)R + 1;
    const u64 *d_adj = c->adj[c->adj_cur].p;
    HIP_TRY(c, rocprim::radix_sort_pairs(c->tmp.p, p.sort_bytes, reinterpret_cast<unsigned *>(c->parent.p), c->skey.p, c->rows.p, c->sval.p, (size_t)R, 0u,
                                         (unsigned)p.end_bit, s));
    hipLaunchKernelGGL(k_bounds, dim3(p.row_grid), dim3(256), 0, s, R, c->skey.p, c->comp_start.p, c->comp_end.p);
    hipLaunchKernelGGL(k_chunk, dim3(p.row_grid), dim3(256), 0, s, R, (i64)p.max_size, c->skey.p, c->sval.p, c->comp_start.p, c->comp_end.p, c->mem_off.p,
                       c->row_tint.p, c->tints.p, c->parent.p, c->head.p, c->chunk_end.p, c->smult.p, c->d_label.p, c->d_nodes.p);
    size_t sb = p.scan_bytes;
    HIP_TRY(c, rocprim::exclusive_scan(c->tmp.p, sb, c->head.p, c->part_id.p, (i64)0, R1, rocprim::plus<i64>(), s));
    sb = p.scan_bytes;
    HIP_TRY(c, rocprim::exclusive_scan(c->tmp.p, sb, c->smult.p, c->rid_pos.p, (i64)0, R1, rocprim::plus<i64>(), s));
    HIP_TRY(c, hipMemsetAsync(c->cnt.p + R, 0, c->cnt.bytes(1), s));
    HIP_TRY(c, hipEventRecord(c->pev[2], s));
    hipLaunchKernelGGL(k_pairs<false>, dim3(p.wave_grid), dim3(256), 0, s, R, c->sval.p, c->chunk_end.p, c->smult.p, c->row_tint.p, c->tints.p, d_adj,
                       c->cnt.p, (const i64 *)nullptr, c->mem_off.p, c->mem.p, (int2 *)nullptr);
    HIP_TRY(c, hipEventRecord(c->pev[3], s));
    sb = p.scan_bytes;
    HIP_TRY(c, rocprim::exclusive_scan(c->tmp.p, sb, c->cnt.p, c->pair_base.p, (i64)0, R1, rocprim::plus<i64>(), s));
    const i64 RT = std::max<i64>(R, p.T);
    hipLaunchKernelGGL(k_offsets, dim3(capped_grid(RT + 1, 256, kCapRowGrid, k)), dim3(256), 0, s, R, p.T, c->tints.p, c->head.p, c->part_id.p, c->rid_pos.p,
                       c->pair_base.p, c->d_tint_part_off.p, c->d_part_node_off.p, c->d_part_rid_off.p, c->d_part_pair_off.p);
    HIP_TRY(c, hipMemcpyAsync(c->h_tot.p, c->part_id.p + R, c->h_tot.bytes(1), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(c->h_tot.p + 1, c->pair_base.p + R, c->h_tot.bytes(1), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    p.P = c->h_tot.p[0]; p.n_pairs = c->h_tot.p[1];
    if (p.P < 0 || p.P > R || p.n_pairs < 0) return fail(c, FCLU_ERR_HIP, "partition totals out of range (%lld partitions, %lld pairs)", p.P, p.n_pairs);
    return FCLU_OK;
}

// The pairs and the partitions' members, and everything to the host.
int part_emit(fclu_ctx *c, const PartRun &p) {
    hipStream_t s = c->stream;
    RC_TRY(grow_pairs(c, p.n_pairs));
    HIP_TRY(c, hipEventRecord(c->pev[4], s));
    if (p.n_pairs)
        hipLaunchKernelGGL(k_pairs<true>, dim3(p.wave_grid), dim3(256), 0, s, p.R, c->sval.p, c->chunk_end.p, c->smult.p, c->row_tint.p, c->tints.p,
                           c->adj[c->adj_cur].p, (i64 *)nullptr, c->pair_base.p, c->mem_off.p, c->mem.p, c->d_pairs.p);
    if (p.n_mem)
        hipLaunchKernelGGL(k_members, dim3(p.wave_grid), dim3(256), 0, s, p.R, c->sval.p, c->smult.p, c->rid_pos.p, c->mem_off.p, c->mem.p, c->d_part_rids.p);
    HIP_TRY(c, hipEventRecord(c->pev[5], s));
    RC_TRY(part_results(c, p, true));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    float a = 0.f, b = 0.f;
    (void)hipEventElapsedTime(&c->components_ms, c->pev[0], c->pev[1]);
    (void)hipEventElapsedTime(&a, c->pev[2], c->pev[3]);
    (void)hipEventElapsedTime(&b, c->pev[4], c->pev[5]);
    c->pairs_ms = a + b;
    return FCLU_OK;
}

// c->tints / c->h_tints / c->row_tint describe the batch and c->adj[c->adj_cur] holds its pruned matrices.  mem_off null: the members
// are on the device already (c->mem_off, c->mem: n_mem_device rep ids), where the dedupe left them.
int partition_device(fclu_ctx *c, const Knobs &k, int T, i64 R, const int64_t *mem_off, const int32_t *mem, i64 n_mem_device, int32_t maximum_ilp_size) {
    HIP_TRY(c, hipSetDevice(c->device));
    c->components_ms = c->pairs_ms = 0.f;
    if (R == 0) RC_TRY(part_empty(c, T));
    else {
        PartRun p;
        p.T = T; p.R = R; p.max_size = maximum_ilp_size; p.n_mem = mem_off ? mem_off[R] : n_mem_device;
        RC_TRY(part_components(c, k, p, mem_off, mem));
        RC_TRY(part_split(c, k, p));
        RC_TRY(part_emit(c, p));
    }
    c->have_parts = true;
    return FCLU_OK;
}

// ---- the dedupe, once for its two users: reps -> nodes (prep_rows, prep_nodes) and reads -> reps (group_device) ----------------
// An item is a rep there and a read here, a class a node and a rep.  The scratch is c->dd (see fclu_ctx).
unsigned item_grid(i64 n, const Knobs &k) { return capped_grid(n, 256, kCapItemGrid, k); }

// rocPRIM's stable sort of (key, value) pairs by the keys' low bits, tmp its temporary storage; need: no sort, only what it takes of tmp
template <typename K>
int sort_pairs(fclu_ctx *c, Buf<char> &tmp, size_t *need, K *key, K *skey, int *val, int *sval, size_t n, unsigned bits) {
    size_t tb = tmp.cap;
    HIP_TRY(c, rocprim::radix_sort_pairs(need ? nullptr : (void *)tmp.p, need ? *need : tb, key, skey, val, sval, n, 0u, bits, c->stream));
    return FCLU_OK;
}

// the two times of a stage from its five events: the key kernel; the dedupe in front of and behind the stage's synchronisation
void stage_times(hipEvent_t *e, float &keys_ms, float &dedupe_ms) {
    float a = 0.f, b = 0.f;
    (void)hipEventElapsedTime(&keys_ms, e[0], e[1]);
    (void)hipEventElapsedTime(&a, e[1], e[2]);
    (void)hipEventElapsedTime(&b, e[3], e[4]);
    dedupe_ms = a + b;
}

// The tints' descriptors from the batch's offsets, with the offsets' and the shapes' refusals: what PrepTint and GroupTint share.  lane_units(d): the caller's
// own fields of d, and the number of units a row's lanes share out (g_log2: the smallest power of two that holds them, 64 at the most).
// n_slots: the lane slots of the key kernel, every tint's starting at a multiple of 64.
template <typename D, typename U>
int describe_rows(fclu_ctx *c, const char *entry, const char *noun, int T, const int64_t *item_off, const int32_t *n_seg, const int64_t *lab_off,
                  U &&lane_units, std::vector<D> &tints, i64 &n_slots) {
    if (!item_off || !n_seg || !lab_off) return fail(c, FCLU_ERR_ARG, "%s: %s_off, n_seg or lab_off is null", entry, noun);
    if (item_off[0] != 0 || lab_off[0] != 0) return fail(c, FCLU_ERR_ARG, "%s: %s_off and lab_off start at 0", entry, noun);
    tints.assign((size_t)T, D());
    n_slots = 0;
    for (int t = 0; t < T; ++t) {
        D &d = tints[(size_t)t];
        const i64 n = item_off[t + 1] - item_off[t];
        if (n < 0 || n > (1 << 30) || n_seg[t] < 0)
            return fail(c, FCLU_ERR_ARG, "tint %d: negative or too large %s count (%lld) or segment count (%d)", t, noun, n, (int)n_seg[t]);
        if (n_seg[t] > kMaxWords * 32)
            return fail(c, FCLU_ERR_UNSUPPORTED, "tint %d has %d segments; this build stages at most %d", t, (int)n_seg[t], kMaxWords * 32);
        d.item0 = item_off[t]; d.lab_off = lab_off[t]; d.slot0 = n_slots;
        d.n = (int)n; d.n_seg = n_seg[t]; d.lw = std::max((d.n_seg + 15) / 16, 1);
        const int units = lane_units(d);
        d.g_log2 = 0; while (d.g_log2 < 6 && (1 << d.g_log2) < units) ++d.g_log2;
        if (lab_off[t + 1] - d.lab_off != n * d.lw)
            return fail(c, FCLU_ERR_ARG, "tint %d: lab_off does not match %ss x words (%lld words for %lld %ss of %d)", t, noun,
                        (i64)(lab_off[t + 1] - d.lab_off), n, noun, d.lw);
        n_slots += ((n << d.g_log2) + 63) / 64 * 64;
    }
    if (item_off[T] >= 0x7f7f7f7fll) return fail(c, FCLU_ERR_ARG, "%s: %lld %ss in one batch", entry, (i64)item_off[T], noun);
    return FCLU_OK;
}

// From the key kernel to the tints' class counts, with the stage's one synchronisation at its end.  The callables launch the caller's
// kernels (as run_burst's does): launch_keys fills dd.key (tint, hash), dd.val (the item) and dd.err[0..2] (the smallest refused item);
// launch_leader dd.leader and dd.flag; launch_offsets runs k_class_off into d_off (T + 1 entries, h_off on the host) and whatever else of
// the caller's needs no count from the host.  ev[0], ev[1]: around the key kernel; ev[2]: behind launch_offsets.  dd.id = the exclusive
// scan of flag is the classes' numbering (N + 1 entries); behind the call, report_row_errors() says what dd.h_err holds.
template <typename K, typename L, typename O>
int dedupe_classes(fclu_ctx *c, const Knobs &k, int T, i64 N, hipEvent_t *ev, K &&launch_keys, L &&launch_leader, O &&launch_offsets, const i64 *d_off,
                   int64_t *h_off) {
    hipStream_t s = c->stream;
    auto &D = c->dd;
    const size_t n = (size_t)N, N1 = n + 1;
    for (Buf<int> *b : {&D.val, &D.sval, &D.head, &D.bstart, &D.leader, &D.nval}) HIP_TRY(c, b->grow(n));
    HIP_TRY(c, D.key.grow(n)); HIP_TRY(c, D.skey.grow(n)); HIP_TRY(c, D.nkey.grow(n)); HIP_TRY(c, D.snkey.grow(n));
    HIP_TRY(c, D.flag.grow(N1)); HIP_TRY(c, D.id.grow(N1)); HIP_TRY(c, D.err.grow(4)); HIP_TRY(c, D.h_err.grow(4));
    const unsigned key_bits = 32u + (unsigned)bits_for(T);
    size_t sort_a = 0, sort_b = 0, scan_a = 0, scan_b = 0;                 // (sort_b: dedupe_members' sort, whose values go to the caller's array)
    RC_TRY(sort_pairs(c, D.tmp, &sort_a, D.key.p, D.skey.p, D.val.p, D.sval.p, n, key_bits));
    RC_TRY(sort_pairs(c, D.tmp, &sort_b, D.nkey.p, D.snkey.p, D.nval.p, D.sval.p, n, (unsigned)bits_for(N)));
    HIP_TRY(c, rocprim::inclusive_scan(nullptr, scan_a, D.head.p, D.bstart.p, n, rocprim::maximum<int>(), s));
    HIP_TRY(c, rocprim::exclusive_scan(nullptr, scan_b, D.flag.p, D.id.p, 0, N1, rocprim::plus<int>(), s));
    HIP_TRY(c, D.tmp.grow(std::max(std::max(sort_a, sort_b), std::max(scan_a, scan_b))));
    HIP_TRY(c, hipMemsetAsync(D.err.p, 0x7f, D.err.bytes(4), s));
    HIP_TRY(c, hipMemsetAsync(D.flag.p + N, 0, D.flag.bytes(1), s));
    HIP_TRY(c, hipEventRecord(ev[0], s));
    launch_keys();
    HIP_TRY(c, hipEventRecord(ev[1], s));
    // refusals first: a tail above 2 or a label 3 has no meaning, and the sort's keys of such a batch are not needed
    HIP_TRY(c, hipMemcpyAsync(D.h_err.p, D.err.p, D.err.bytes(4), hipMemcpyDeviceToHost, s));
    RC_TRY(sort_pairs(c, D.tmp, nullptr, D.key.p, D.skey.p, D.val.p, D.sval.p, n, key_bits));
    hipLaunchKernelGGL(k_heads, dim3(item_grid(N, k)), dim3(256), 0, s, N, D.skey.p, D.head.p);
    size_t tb = D.tmp.cap;
    HIP_TRY(c, rocprim::inclusive_scan(D.tmp.p, tb, D.head.p, D.bstart.p, n, rocprim::maximum<int>(), s));
    launch_leader();
    tb = D.tmp.cap;
    HIP_TRY(c, rocprim::exclusive_scan(D.tmp.p, tb, D.flag.p, D.id.p, 0, N1, rocprim::plus<int>(), s));
    launch_offsets();
    HIP_TRY(c, hipEventRecord(ev[2], s));
    HIP_TRY(c, hipMemcpyAsync(h_off, d_off, sizeof(i64) * ((size_t)T + 1), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    return FCLU_OK;
}

// The classes' member lists, behind the caller's numbering kernel (dd.nkey: an item's class, dd.nval: the item within its tint): the items
// sorted (stable) by class are the lists end to end, each ascending (mem); class q's starts where its key first stands (mem_off).
int dedupe_members(fclu_ctx *c, const Knobs &k, i64 N, i64 n_classes, int *mem, i64 *mem_off) {
    auto &D = c->dd;
    RC_TRY(sort_pairs(c, D.tmp, nullptr, D.nkey.p, D.snkey.p, D.nval.p, mem, (size_t)N, (unsigned)bits_for(N)));
    hipLaunchKernelGGL(k_mem_off, dim3(item_grid(N + 1, k)), dim3(256), 0, c->stream, N, n_classes, D.snkey.p, mem_off);   // (N + 1 entries)
    return FCLU_OK;
}

// What the key kernel refused (dd.h_err, behind dedupe_classes): the smallest item with a tail category above 2, with a label 3, with a
// bit behind its tint's labels.  tail: the caller's bytes, or null when they are not on the host (the grouping has refused such a tail
// already; no number to print).
int report_row_errors(fclu_ctx *c, const char *noun, int T, const int64_t *item_off, const int32_t *n_seg, const uint8_t *tail) {
    const int kinds[3] = {2, 0, 1};                          // the tail first: it is the caller's own byte, the labels come from a file
    for (int kind : kinds) {
        const i64 item = c->dd.h_err.p[kind];
        if (item == 0x7f7f7f7f) continue;
        int t = 0;
        while (t + 1 < T && item_off[t + 1] <= item) ++t;
        const i64 r = item - item_off[t];
        if (kind == 2 && !tail) return fail(c, FCLU_ERR_ARG, "tint %d %s %lld: tail category above 2 (0 'N', 1 'S', 2 'E')", t, noun, r);
        if (kind == 2) return fail(c, FCLU_ERR_ARG, "tint %d %s %lld: tail category %d (0 'N', 1 'S', 2 'E')", t, noun, r, (int)tail[item]);
        if (kind == 0) return fail(c, FCLU_ERR_ARG, "tint %d %s %lld: a label with code 3 (labels are 0, 1, 2)", t, noun, r);
        return fail(c, FCLU_ERR_ARG, "tint %d %s %lld: a nonzero bit beyond the tint's %d labels", t, noun, r, (int)n_seg[t]);
    }
    return FCLU_OK;
}

// ---- preprocess_ilp() + the dedupe of a batch of label rows ----------------------------------------------------------
// what the two halves share
struct PrepRun {
    int T = 0;
    i64 N = 0, n_rbits = 0, R = 0, n_bits = 0;           // reps, words of their I / C rows; unique rows, words of theirs
    std::vector<PrepTint> pt;
};

// Rows and dedupe up to the tints' counts of unique rows: only row_off (n_tint + 1 counts) and the three error words come back to the
// host here, for the refusals and for the unique rows' layout as a batch (c->ph.row_off / bits_off / adj_off).
// on_device: the rows and tails are in c->pd.labels / c->pd.tail already, where the grouping gathered them (group_device), checked there.
int prep_rows(fclu_ctx *c, const Knobs &k, const fclu_reads *rd, bool on_device, PrepRun &p) {
    if (!rd || rd->n_tint <= 0) return fail(c, FCLU_ERR_ARG, "fclu_preprocess: empty batch");
    HIP_TRY(c, hipSetDevice(c->device));
    const int T = p.T = rd->n_tint;
    auto &D = c->pd;
    auto &H = c->ph;
    for (HostBuf<int64_t> *h : {&H.row_off, &H.bits_off, &H.adj_off, &H.rbits_off}) HIP_TRY(c, h->grow((size_t)T + 1));
    i64 n_slots = 0;
    const auto words = [](PrepTint &d) { return d.w = std::max((d.n_seg + 31) / 32, 1); };                // a lane a bit word
    RC_TRY(describe_rows(c, "fclu_preprocess", "rep", T, rd->rep_off, rd->n_seg, rd->lab_off, words, p.pt, n_slots));
    H.rbits_off.p[0] = 0;                                    // the reps' I / C rows end to end
    for (int t = 0; t < T; ++t) { PrepTint &d = p.pt[(size_t)t]; d.rbits_off = H.rbits_off.p[t]; H.rbits_off.p[t + 1] = d.rbits_off + (i64)d.n * d.w; }
    const i64 N = p.N = rd->rep_off[T], n_lab = rd->lab_off[T];
    p.n_rbits = H.rbits_off.p[T];
    if (N > 0 && !on_device && (!rd->labels || !rd->tail)) return fail(c, FCLU_ERR_ARG, "fclu_preprocess: labels or tail is null");
    int64_t *h_row_off = H.row_off.p;
    if (N > 0) {
        hipStream_t s = c->stream;
        auto &S = c->dd;
        HIP_TRY(c, D.tints.grow((size_t)T)); HIP_TRY(c, D.row_off.grow((size_t)T + 1));
        HIP_TRY(c, D.labels.grow((size_t)n_lab)); HIP_TRY(c, D.tail.grow((size_t)N));
        HIP_TRY(c, D.ibits.grow((size_t)p.n_rbits)); HIP_TRY(c, D.cbits.grow((size_t)p.n_rbits));
        for (Buf<int> *b : {&D.rfirst, &D.rlast, &D.first, &D.last, &D.rep_tint, &D.rep_node, &D.node_rep, &c->mem}) HIP_TRY(c, b->grow((size_t)N));
        HIP_TRY(c, hipMemcpyAsync(D.tints.p, p.pt.data(), D.tints.bytes((size_t)T), hipMemcpyHostToDevice, s));
        if (!on_device) {
            HIP_TRY(c, hipMemcpyAsync(D.labels.p, rd->labels, D.labels.bytes((size_t)n_lab), hipMemcpyHostToDevice, s));
            HIP_TRY(c, hipMemcpyAsync(D.tail.p, rd->tail, D.tail.bytes((size_t)N), hipMemcpyHostToDevice, s));
        }
        const auto keys = [&]() {
            hipLaunchKernelGGL(k_rows, dim3(capped_grid(n_slots, 256, kCapSlots, k)), dim3(256), 0, s, T, n_slots, D.tints.p, D.labels.p, D.tail.p,
                               k.hash_mask, D.ibits.p, D.cbits.p, D.rfirst.p, D.rlast.p, D.first.p, D.last.p, D.rep_tint.p, S.key.p, S.val.p, S.err.p);
        };
        const auto leader = [&]() {
            hipLaunchKernelGGL(k_leader, dim3(item_grid(N, k)), dim3(256), 0, s, N, S.skey.p, S.sval.p, S.bstart.p, D.tints.p, D.ibits.p, D.first.p, D.last.p,
                               D.tail.p, S.leader.p, S.flag.p);
        };
        const auto offsets = [&]() {
            hipLaunchKernelGGL(k_class_off<PrepTint>, dim3((unsigned)(T + 256) / 256), dim3(256), 0, s, T, N, D.tints.p, S.id.p, D.row_off.p);
        };
        RC_TRY(dedupe_classes(c, k, T, N, c->qev, keys, leader, offsets, D.row_off.p, h_row_off));
        RC_TRY(report_row_errors(c, "rep", T, rd->rep_off, rd->n_seg, on_device ? nullptr : rd->tail));
    } else {
        memset(h_row_off, 0, H.row_off.bytes((size_t)T + 1));
    }
    // ---- the unique rows as a batch
    H.bits_off.p[0] = H.adj_off.p[0] = 0;
    for (int t = 0; t < T; ++t) {
        const i64 n = h_row_off[t + 1] - h_row_off[t];
        if (n < 0 || n > rd->rep_off[t + 1] - rd->rep_off[t]) return fail(c, FCLU_ERR_HIP, "tint %d: %lld unique rows of %lld reps", t, n, (i64)(rd->rep_off[t + 1] - rd->rep_off[t]));
        H.bits_off.p[t + 1] = H.bits_off.p[t] + n * p.pt[(size_t)t].w;
        H.adj_off.p[t + 1] = H.adj_off.p[t] + n * ((n + 63) / 64);
    }
    p.R = h_row_off[T]; p.n_bits = H.bits_off.p[T];
    return FCLU_OK;
}

// The nodes behind stage_tints(): c->bits / first / last / tail hold them in fclu_batch's layout, c->mem_off / c->mem their members, and
// the pinned copies of everything fclu_prep names are on their way (the caller synchronises).
int prep_nodes(fclu_ctx *c, const Knobs &k, const PrepRun &p) {
    hipStream_t s = c->stream;
    auto &D = c->pd;
    auto &H = c->ph;
    const i64 N = p.N, R = p.R;
    const bool copy = N > 0;
    if (copy) {
        auto &S = c->dd;
        HIP_TRY(c, c->mem_off.grow((size_t)R + 1));
        HIP_TRY(c, hipEventRecord(c->qev[3], s));
        hipLaunchKernelGGL(k_nodes, dim3(item_grid(N + 1, k)), dim3(256), 0, s, N, D.rep_tint.p, D.tints.p, c->tints.p, S.leader.p, S.id.p, D.ibits.p, D.first.p,
                           D.last.p, D.tail.p, D.rep_node.p, S.nkey.p, S.nval.p, D.node_rep.p, c->bits.p, c->first.p, c->last.p, c->tail.p);
        RC_TRY(dedupe_members(c, k, N, R, c->mem.p, c->mem_off.p));
        HIP_TRY(c, hipEventRecord(c->qev[4], s));
    }
    // the result set: {pinned buffer, device source, element count, fclu_prep's field}
    fclu_prep &o = c->prep;
    const size_t nN = (size_t)N, nR = (size_t)R, nW = (size_t)p.n_rbits;
    RC_TRY(fetch(c, H.ibits, D.ibits.p, nW, copy, o.i_bits));
    RC_TRY(fetch(c, H.cbits, D.cbits.p, nW, copy, o.c_bits));
    RC_TRY(fetch(c, H.first, D.first.p, nN, copy, o.first));
    RC_TRY(fetch(c, H.last, D.last.p, nN, copy, o.last));
    RC_TRY(fetch(c, H.rfirst, D.rfirst.p, nN, copy, o.raw_first));
    RC_TRY(fetch(c, H.rlast, D.rlast.p, nN, copy, o.raw_last));
    RC_TRY(fetch(c, H.rep_node, D.rep_node.p, nN, copy, o.rep_node));
    RC_TRY(fetch(c, H.node_rep, D.node_rep.p, nR, copy, o.node_rep));
    RC_TRY(fetch(c, H.mem_off, c->mem_off.p, nR + 1, copy, o.mem_off));
    RC_TRY(fetch(c, H.mem, c->mem.p, nN, copy, o.mem));
    RC_TRY(fetch(c, H.bits, c->bits.p, (size_t)p.n_bits, copy, o.bits));
    RC_TRY(fetch(c, H.nfirst, c->first.p, nR, copy, o.node_first));
    RC_TRY(fetch(c, H.nlast, c->last.p, nR, copy, o.node_last));
    RC_TRY(fetch(c, H.ntail, c->tail.p, nR, copy, o.node_tail));
    if (!copy) *H.mem_off.p = 0;
    o.n_tint = p.T; o.n_reps = N; o.n_rows = R;
    o.row_off = H.row_off.p; o.bits_off = H.bits_off.p; o.adj_off = H.adj_off.p; o.rep_bits_off = H.rbits_off.p;
    return FCLU_OK;
}

// Rows, dedupe and the staging of the unique rows as a batch: st is what compat_run() needs.
int preprocess_device(fclu_ctx *c, const Knobs &k, const fclu_reads *rd, int32_t prune, Staged &st, i64 &n_reps_out, bool on_device = false) {
    c->have_prep = false;
    c->round_src_ok = c->round_ready = c->have_rounds = false;
    c->rows_ms = c->dedupe_ms = 0.f;
    PrepRun p;
    RC_TRY(prep_rows(c, k, rd, on_device, p));
    n_reps_out = p.N;
    RC_TRY(stage_tints(c, k, p.T, c->ph.row_off.p, rd->n_seg, c->ph.bits_off.p, c->ph.adj_off.p, prune, nullptr, st));
    return prep_nodes(c, k, p);
}

// the kernels' times of the call that has just synchronised
void preprocess_times(fclu_ctx *c, i64 n_reps) { if (n_reps > 0) stage_times(c->qev, c->rows_ms, c->dedupe_ms); }

// ---- read_segment()'s rep grouping of a batch of tints (:154-164) ---------------------------------------------------------
// Keys, the dedupe, the reps' numbering and members.  gather (fclu_partition_segment): the reps' rows and tails go into c->pd.labels /
// c->pd.tail (fclu_reads' layout, at c->gh.rep_off / c->gh.rep_lab_off), where prep_rows() takes them without another upload; the grouping
// alone leaves the preprocess stage's device arrays as they are.  One synchronisation in the middle (dedupe_classes): the tints' rep
// counts size the members' offsets and decide the layout of the gathered rows.  It synchronises at its end: the scratch is free again.
int group_device(fclu_ctx *c, const Knobs &k, const fclu_segment *in, bool gather, i64 &n_reps_out) {
    c->have_groups = false;
    c->round_src_ok = c->round_ready = c->have_rounds = false;
    c->gkeys_ms = c->gdedupe_ms = 0.f;
    if (!in || in->n_tint <= 0) return fail(c, FCLU_ERR_ARG, "fclu_group_reads: empty batch");
    HIP_TRY(c, hipSetDevice(c->device));
    const int T = in->n_tint;
    auto &D = c->gd;
    auto &H = c->gh;
    HIP_TRY(c, H.rep_off.grow((size_t)T + 1)); HIP_TRY(c, H.rep_lab_off.grow((size_t)T + 1));
    std::vector<GroupTint> gt;
    i64 n_slots = 0;
    // a lane a 16-byte quad where every row of the tint is whole quads, else a label word
    const auto quads = [](GroupTint &d) { d.vec = (d.lw % 4 == 0 && d.lab_off % 4 == 0) ? 1 : 0; return d.vec ? d.lw / 4 : d.lw; };
    RC_TRY(describe_rows(c, "fclu_group_reads", "read", T, in->read_off, in->n_seg, in->lab_off, quads, gt, n_slots));
    const i64 N = in->read_off[T], n_lab = in->lab_off[T];
    if (N > 0 && (!in->labels || !in->tail || !in->tok_off)) return fail(c, FCLU_ERR_ARG, "fclu_group_reads: labels, tail or tok_off is null");
    i64 n_tok = 0;
    if (N > 0) {
        if (in->tok_off[0] != 0) return fail(c, FCLU_ERR_ARG, "fclu_group_reads: tok_off[0] is %lld, not 0", (i64)in->tok_off[0]);
        int t = 0;
        for (i64 r = 0; r < N; ++r)
            if (in->tok_off[r + 1] < in->tok_off[r]) {
                while (t + 1 < T && in->read_off[t + 1] <= r) ++t;
                return fail(c, FCLU_ERR_ARG, "tint %d read %lld: tok_off falls (%lld after %lld)", t, r - in->read_off[t], (i64)in->tok_off[r + 1], (i64)in->tok_off[r]);
            }
        n_tok = in->tok_off[N];
        if (n_tok > 0 && !in->tok) return fail(c, FCLU_ERR_ARG, "fclu_group_reads: tok is null");
    }
    int64_t *h_rep_off = H.rep_off.p, *h_rep_lab_off = H.rep_lab_off.p;
    i64 n_reps = 0, n_rep_lab = 0;
    fclu_groups &o = c->groups;
    if (N > 0) {
        hipStream_t s = c->stream;
        auto &S = c->dd;
        const size_t N1 = (size_t)N + 1;
        HIP_TRY(c, D.tints.grow((size_t)T)); HIP_TRY(c, D.labels.grow((size_t)n_lab)); HIP_TRY(c, D.tail.grow((size_t)N));
        HIP_TRY(c, D.tok_off.grow(N1)); HIP_TRY(c, D.tok.grow((size_t)std::max<i64>(n_tok, 1)));
        for (Buf<int> *b : {&D.read_tint, &D.read_rep, &D.mem, &D.rep_first}) HIP_TRY(c, b->grow((size_t)N));
        HIP_TRY(c, D.mem_off.grow(N1)); HIP_TRY(c, D.rep_off.grow((size_t)T + 1)); HIP_TRY(c, D.rep_lab_off.grow((size_t)T + 1));
        HIP_TRY(c, hipMemcpyAsync(D.tints.p, gt.data(), D.tints.bytes((size_t)T), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(D.labels.p, in->labels, D.labels.bytes((size_t)n_lab), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(D.tail.p, in->tail, D.tail.bytes((size_t)N), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(D.tok_off.p, in->tok_off, D.tok_off.bytes(N1), hipMemcpyHostToDevice, s));
        if (n_tok) HIP_TRY(c, hipMemcpyAsync(D.tok.p, in->tok, D.tok.bytes((size_t)n_tok), hipMemcpyHostToDevice, s));
        else HIP_TRY(c, hipMemsetAsync(D.tok.p, 0, D.tok.bytes(1), s));
        const auto keys = [&]() {
            hipLaunchKernelGGL(k_gkeys, dim3(capped_grid(n_slots, 256, kCapSlots, k)), dim3(256), 0, s, T, n_slots, D.tints.p, D.labels.p, D.tok_off.p,
                               D.tok.p, D.tail.p, k.hash_mask, D.read_tint.p, S.key.p, S.val.p, S.err.p);
        };
        const auto leader = [&]() {
            hipLaunchKernelGGL(k_gleader, dim3(item_grid(N, k)), dim3(256), 0, s, N, S.skey.p, S.sval.p, S.bstart.p, D.tints.p, D.labels.p, D.tok_off.p, D.tok.p,
                               std::max<i64>(n_tok, 1), S.leader.p, S.flag.p);
        };
        const auto offsets = [&]() {                         // (the numbering needs no count from the host: in front of the synchronisation)
            hipLaunchKernelGGL(k_class_off<GroupTint>, dim3((unsigned)(T + 256) / 256), dim3(256), 0, s, T, N, D.tints.p, S.id.p, D.rep_off.p);
            hipLaunchKernelGGL(k_greps, dim3(item_grid(N, k)), dim3(256), 0, s, N, D.read_tint.p, D.tints.p, S.leader.p, S.id.p, D.read_rep.p, S.nkey.p, S.nval.p,
                               D.rep_first.p);
        };
        RC_TRY(dedupe_classes(c, k, T, N, c->gev, keys, leader, offsets, D.rep_off.p, h_rep_off));
        RC_TRY(report_row_errors(c, "read", T, in->read_off, in->n_seg, in->tail));
        // ---- the reps' rows as fclu_reads: their layout from the tints' rep counts
        h_rep_lab_off[0] = 0;
        for (int t = 0; t < T; ++t) {
            const i64 n = h_rep_off[t + 1] - h_rep_off[t];
            if (n < 0 || n > gt[(size_t)t].n || (n == 0) != (gt[(size_t)t].n == 0))
                return fail(c, FCLU_ERR_HIP, "tint %d: %lld reps of %d reads", t, n, gt[(size_t)t].n);
            h_rep_lab_off[t + 1] = h_rep_lab_off[t] + n * gt[(size_t)t].lw;
        }
        n_reps = h_rep_off[T]; n_rep_lab = h_rep_lab_off[T];
        if (gather) {
            HIP_TRY(c, c->pd.labels.grow((size_t)n_rep_lab)); HIP_TRY(c, c->pd.tail.grow((size_t)n_reps));
            HIP_TRY(c, hipMemcpyAsync(D.rep_lab_off.p, h_rep_lab_off, D.rep_lab_off.bytes((size_t)T + 1), hipMemcpyHostToDevice, s));
        }
        HIP_TRY(c, hipEventRecord(c->gev[3], s));
        RC_TRY(dedupe_members(c, k, N, n_reps, D.mem.p, D.mem_off.p));
        if (gather)
            hipLaunchKernelGGL(k_ggather, dim3(capped_grid(n_rep_lab, 256, kCapGather, k)), dim3(256), 0, s, T, n_rep_lab, D.tints.p, D.rep_off.p,
                               D.rep_lab_off.p, D.rep_first.p, D.labels.p, D.tail.p, c->pd.labels.p, c->pd.tail.p);
        HIP_TRY(c, hipEventRecord(c->gev[4], s));
    } else {
        memset(h_rep_off, 0, H.rep_off.bytes((size_t)T + 1));
        memset(h_rep_lab_off, 0, H.rep_lab_off.bytes((size_t)T + 1));
    }
    const bool copy = N > 0;
    RC_TRY(fetch(c, H.read_rep, D.read_rep.p, (size_t)N, copy, o.read_rep));
    RC_TRY(fetch(c, H.mem_off, D.mem_off.p, (size_t)n_reps + 1, copy, o.rep_mem_off));
    RC_TRY(fetch(c, H.mem, D.mem.p, (size_t)N, copy, o.rep_mem));
    RC_TRY(fetch(c, H.rep_first, D.rep_first.p, (size_t)n_reps, copy, o.rep_first));
    if (!copy) *H.mem_off.p = 0;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if (copy) stage_times(c->gev, c->gkeys_ms, c->gdedupe_ms);
    o.n_tint = T; o.n_reads = N; o.n_reps = n_reps; o.rep_off = h_rep_off;
    n_reps_out = n_reps;
    c->have_groups = true;
    return FCLU_OK;
}

// ---- a round's models (fclu_round_setup, fclu_round_models) ----------------------------------------------------------------
// The I / C rows (c->pd.ibits / cbits), the pair lists (c->d_pairs) and the partitions (c->parts, pinned) of the call that has just
// succeeded are the rounds' source: the host keeps the batch's shape.
void round_source(fclu_ctx *c, const fclu_reads *rd) {
    c->r_rep_off.assign(rd->rep_off, rd->rep_off + rd->n_tint + 1);
    c->r_n_seg.assign(rd->n_seg, rd->n_seg + rd->n_tint);
    c->r_lab_off.assign(rd->lab_off, rd->lab_off + rd->n_tint + 1);
    c->round_src_ok = true;
}

int round_setup(fclu_ctx *c, const int64_t *gap_off, const int32_t *gaps, const int64_t *seg_off, const int32_t *seg_len) {
    c->round_ready = c->have_rounds = false;
    if (!c->round_src_ok || !c->have_parts)
        return fail(c, FCLU_ERR_ARG, "fclu_round_setup: the context holds no fclu_partition_reads() / fclu_partition_segment() result");
    if (!gap_off || !seg_off) return fail(c, FCLU_ERR_ARG, "fclu_round_setup: gap_off or seg_off is null");
    HIP_TRY(c, hipSetDevice(c->device));
    const int T = (int)c->r_n_seg.size();
    const i64 N = c->r_rep_off[(size_t)T];
    if (gap_off[0] != 0 || seg_off[0] != 0) return fail(c, FCLU_ERR_ARG, "fclu_round_setup: gap_off and seg_off start at 0");
    for (int t = 0; t < T; ++t) {
        const int M = c->r_n_seg[(size_t)t];
        if (seg_off[t + 1] - seg_off[t] != M)
            return fail(c, FCLU_ERR_ARG, "tint %d: %lld segment lengths for %d segments", t, (i64)(seg_off[t + 1] - seg_off[t]), M);
        for (i64 r = c->r_rep_off[(size_t)t]; r < c->r_rep_off[(size_t)t + 1]; ++r) {
            if (gap_off[r + 1] < gap_off[r] || gap_off[r + 1] > 2147483647ll) return fail(c, FCLU_ERR_ARG, "fclu_round_setup: gap_off falls or is too large at rep %lld", r);
            for (i64 g = gap_off[r]; g < gap_off[r + 1]; ++g) {
                if (!gaps) return fail(c, FCLU_ERR_ARG, "fclu_round_setup: gaps is null");
                const int j1 = gaps[3 * g], j2 = gaps[3 * g + 1];
                if (M < 1 || j1 < -1 || j1 > j2 || j2 > M || j1 > M - 1)
                    return fail(c, FCLU_ERR_ARG, "tint %d rep %lld: gap (%d, %d) outside -1 <= j1 <= j2 <= %d", t, r - c->r_rep_off[(size_t)t], j1, j2, M);
            }
        }
    }
    const i64 n_gaps = gap_off[N], n_seg_total = seg_off[T];
    if (n_seg_total > 0 && !seg_len) return fail(c, FCLU_ERR_ARG, "fclu_round_setup: seg_len is null");
    // rep -> partition, partition -> tint, from the partition call's pinned results
    const fclu_parts &pp = c->parts;
    c->r_rep_part.assign((size_t)N, -1);
    c->r_part_tint.assign((size_t)pp.n_part, 0);
    for (int t = 0; t < T; ++t)
        for (i64 q = pp.tint_part_off[t]; q < pp.tint_part_off[t + 1]; ++q) {
            c->r_part_tint[(size_t)q] = t;
            for (i64 x = pp.part_rid_off[q]; x < pp.part_rid_off[q + 1]; ++x) c->r_rep_part[(size_t)(c->r_rep_off[(size_t)t] + pp.part_rids[x])] = q;
        }
    c->r_rep_stamp.assign((size_t)N, 0); c->r_part_stamp.assign((size_t)pp.n_part, 0);
    c->r_epoch = 0;
    c->r_gap_off.assign(gap_off, gap_off + N + 1);
    c->r_seg_off.assign(seg_off, seg_off + T + 1);
    c->r_max_lg.assign((size_t)T, 0);
    for (int t = 0; t < T; ++t) for (i64 j = seg_off[t]; j < seg_off[t + 1]; ++j) c->r_max_lg[(size_t)t] += seg_len[j];
    auto &D = c->rd;
    hipStream_t s = c->stream;
    HIP_TRY(c, D.gap_off.grow((size_t)N + 1)); HIP_TRY(c, D.gaps.grow((size_t)n_gaps * 3)); HIP_TRY(c, D.seg_len.grow((size_t)n_seg_total));
    HIP_TRY(c, D.col_of.grow((size_t)N));
    HIP_TRY(c, hipMemcpyAsync(D.gap_off.p, gap_off, D.gap_off.bytes((size_t)N + 1), hipMemcpyHostToDevice, s));
    if (n_gaps) HIP_TRY(c, hipMemcpyAsync(D.gaps.p, gaps, D.gaps.bytes((size_t)n_gaps * 3), hipMemcpyHostToDevice, s));
    if (n_seg_total) HIP_TRY(c, hipMemcpyAsync(D.seg_len.p, seg_len, D.seg_len.bytes((size_t)n_seg_total), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    c->round_ready = true;
    return FCLU_OK;
}

// what the host derives from a round's problems
struct RoundRun {
    int P = 0;
    i64 C = 0, G = 0, n_inf_bits = 0;                      // columns, gap rows, words of the informative rows
    std::vector<RoundProb> probs;
    std::vector<int> col_prob, tiny, small, large;          // problems by path: LDS up to kRoundTinyBytes, LDS, device memory
    std::vector<i64> col_row_off, prob_row_off, inf_bits_off;
    size_t tiny_lds = 0, small_lds = 0;
};

// The problems checked (every refusal names problem and column) and laid out.
int round_stage(fclu_ctx *c, const Knobs &k, const fclu_round_batch *b, RoundRun &r) {
    const int P = r.P = b->n_prob;
    const fclu_parts &pp = c->parts;
    if (b->rid_off[0] != 0) return fail(c, FCLU_ERR_ARG, "fclu_round_models: rid_off starts at 0");
    const i64 C = r.C = b->rid_off[P];
    if (C < 0 || C > 2147483647ll) return fail(c, FCLU_ERR_ARG, "fclu_round_models: %lld columns in one batch", C);
    if (C > 0 && !b->rids) return fail(c, FCLU_ERR_ARG, "fclu_round_models: rids is null");
    r.probs.assign((size_t)P, RoundProb());
    r.col_prob.resize((size_t)C); r.col_row_off.resize((size_t)C + 1); r.prob_row_off.resize((size_t)P + 1); r.inf_bits_off.resize((size_t)P + 1);
    const int epoch = ++c->r_epoch;
    i64 G = 0, n_inf_bits = 0;
    for (int p = 0; p < P; ++p) {
        const i64 q = b->part[p], c0 = b->rid_off[p], n = b->rid_off[p + 1] - c0;
        if (q < 0 || q >= pp.n_part) return fail(c, FCLU_ERR_ARG, "problem %d: partition %lld of %lld", p, q, (i64)pp.n_part);
        if (n < 0 || b->rid_off[p + 1] > C) return fail(c, FCLU_ERR_ARG, "problem %d: rid_off falls", p);
        if (c->r_part_stamp[(size_t)q] == epoch) return fail(c, FCLU_ERR_ARG, "problem %d: partition %lld is in this batch twice", p, q);
        c->r_part_stamp[(size_t)q] = epoch;
        const int t = c->r_part_tint[(size_t)q];
        RoundProb &d = r.probs[(size_t)p];
        d.col0 = c0; d.rbits_off = c->ph.rbits_off.p[t]; d.rep0 = c->r_rep_off[(size_t)t]; d.pair0 = pp.part_pair_off[q]; d.pair1 = pp.part_pair_off[q + 1];
        d.inf_off = n_inf_bits; d.seg0 = c->r_seg_off[(size_t)t];
        d.n = (int)n; d.n_seg = c->r_n_seg[(size_t)t]; d.w = std::max((d.n_seg + 31) / 32, 1); d.tint = t;
        const i64 n_t = c->r_rep_off[(size_t)t + 1] - d.rep0;
        r.inf_bits_off[(size_t)p] = n_inf_bits; r.prob_row_off[(size_t)p] = G;
        n_inf_bits += d.w;
        for (i64 x = 0; x < n; ++x) {
            const i64 rid = b->rids[c0 + x];
            if (rid < 0 || rid >= n_t) return fail(c, FCLU_ERR_ARG, "problem %d column %lld: rep %lld of %lld", p, x, rid, n_t);
            const size_t rep = (size_t)(d.rep0 + rid);
            if (c->r_rep_part[rep] != q) return fail(c, FCLU_ERR_ARG, "problem %d column %lld: rep %lld is not in partition %lld", p, x, rid, q);
            if (c->r_rep_stamp[rep] == epoch) return fail(c, FCLU_ERR_ARG, "problem %d column %lld: rep %lld is in the problem twice", p, x, rid);
            c->r_rep_stamp[rep] = epoch;
            r.col_prob[(size_t)(c0 + x)] = p; r.col_row_off[(size_t)(c0 + x)] = G;
            G += c->r_gap_off[rep + 1] - c->r_gap_off[rep];
        }
        const size_t lds = 2 * (size_t)n * (size_t)(d.w | 1) * 4;
        if ((i64)n * d.w > 2147483647ll) return fail(c, FCLU_ERR_UNSUPPORTED, "problem %d: %lld columns of %d words are more than one workgroup indexes", p, n, d.w);
        if (k.round_lds && lds <= (size_t)std::min<i64>(k.round_lds_bytes, kRoundTinyBytes)) { r.tiny.push_back(p); r.tiny_lds = std::max(r.tiny_lds, lds); }
        else if (k.round_lds && lds <= (size_t)k.round_lds_bytes) { r.small.push_back(p); r.small_lds = std::max(r.small_lds, lds); }
        else r.large.push_back(p);
    }
    r.col_row_off[(size_t)C] = r.prob_row_off[(size_t)P] = G; r.inf_bits_off[(size_t)P] = n_inf_bits;
    if (G > 2147483647ll) return fail(c, FCLU_ERR_UNSUPPORTED, "fclu_round_models: %lld gap rows in one batch", G);
    r.G = G; r.n_inf_bits = n_inf_bits;
    return FCLU_OK;
}

template <bool EMIT>
void round_launch(fclu_ctx *c, const RoundRun &r) {
    auto &D = c->rd;
    const int nT = (int)r.tiny.size(), nS = (int)r.small.size(), nL = (int)r.large.size();
    const auto lds_launch = [&](int n, int first, size_t lds) {
        if (n)
            hipLaunchKernelGGL((k_round<true, EMIT>), dim3((unsigned)n), dim3(256), lds, c->stream, D.list.p + first, r.P, D.probs.p, c->pd.ibits.p, c->pd.cbits.p,
                               D.rids.p, D.col_of.p, c->d_pairs.p, D.inf_bits.p, D.cnt.p, D.scan.p, D.inf_seg.p, D.sup_off.p, D.sup_cols.p, D.corr_off.p, D.corr_seg.p, D.pairs.p);
    };
    lds_launch(nT, 0, r.tiny_lds);
    lds_launch(nS, nT, r.small_lds);
    if (nL)
        hipLaunchKernelGGL((k_round<false, EMIT>), dim3((unsigned)nL), dim3(256), 0, c->stream, D.list.p + nT + nS, r.P, D.probs.p, c->pd.ibits.p, c->pd.cbits.p,
                           D.rids.p, D.col_of.p, c->d_pairs.p, D.inf_bits.p, D.cnt.p, D.scan.p, D.inf_seg.p, D.sup_off.p, D.sup_cols.p, D.corr_off.p, D.corr_seg.p, D.pairs.p);
}

// resident (fclu_round_models_resident): the same kernels and device arrays; of the results only the small per-problem arrays come to the
// host -- what the later round calls and the read-out need of them -- and the model's own arrays stay where they are.
int round_device(fclu_ctx *c, const Knobs &k, const fclu_round_batch *b, bool resident) {
    c->have_rounds = c->have_incs = c->have_exact = c->have_bnb = c->have_wide = c->have_readout = false;
    c->rcount_ms = c->rgaps_ms = c->rfill_ms = 0.f;
    if (!c->round_ready || !c->round_src_ok || !c->have_parts)
        return fail(c, FCLU_ERR_ARG, "fclu_round_models: no fclu_round_setup() behind the context's last partition call");
    if (!b || b->n_prob <= 0 || !b->part || !b->rid_off) return fail(c, FCLU_ERR_ARG, "fclu_round_models: empty batch or null arrays");
    HIP_TRY(c, hipSetDevice(c->device));
    RoundRun r;
    RC_TRY(round_stage(c, k, b, r));
    auto &D = c->rd;
    auto &H = c->rh;
    hipStream_t s = c->stream;
    const int P = r.P;
    const i64 C = r.C, G = r.G;
    const size_t P1 = (size_t)P + 1, nCnt = (size_t)kRoundCounts * P1, nC = (size_t)C, nG = (size_t)G;
    const i64 N = c->r_rep_off.back();
    HIP_TRY(c, D.probs.grow((size_t)P)); HIP_TRY(c, D.list.grow((size_t)P)); HIP_TRY(c, D.rids.grow(nC)); HIP_TRY(c, D.col_prob.grow(nC));
    HIP_TRY(c, D.col_row_off.grow(nC + 1)); HIP_TRY(c, D.prob_row_off.grow(P1)); HIP_TRY(c, D.cnt.grow(nCnt)); HIP_TRY(c, D.scan.grow(nCnt));
    HIP_TRY(c, D.inf_bits.grow((size_t)r.n_inf_bits)); HIP_TRY(c, D.refused.grow((size_t)P)); HIP_TRY(c, D.corr_off.grow(nC + 1)); HIP_TRY(c, D.grp_off.grow(P1));
    HIP_TRY(c, D.key.grow(nG)); HIP_TRY(c, D.skey.grow(nG)); HIP_TRY(c, D.val.grow(nG)); HIP_TRY(c, D.sval.grow(nG)); HIP_TRY(c, D.rows.grow(3 * nG));
    HIP_TRY(c, D.head.grow(nG)); HIP_TRY(c, D.gid.grow(nG)); HIP_TRY(c, D.grp.grow(2 * nG)); HIP_TRY(c, D.grp_prob.grow(nG));
    HIP_TRY(c, D.grp_cnt.grow(nG + 1)); HIP_TRY(c, D.grp_seg_off.grow(nG + 1));
    HIP_TRY(c, H.scan.grow(nCnt)); HIP_TRY(c, c->h_tot.grow(2));
    const unsigned key_bits = 32u + (unsigned)bits_for(P);
    size_t tmp_a = 0, tmp_b = 0, tmp_c = 0, tmp_d = 0;
    HIP_TRY(c, rocprim::exclusive_scan(nullptr, tmp_a, D.cnt.p, D.scan.p, (i64)0, nCnt, rocprim::plus<i64>(), s));
    if (G) {
        RC_TRY(sort_pairs(c, D.tmp, &tmp_b, D.key.p, D.skey.p, D.val.p, D.sval.p, nG, key_bits));
        HIP_TRY(c, rocprim::inclusive_scan(nullptr, tmp_c, D.head.p, D.gid.p, nG, rocprim::plus<i64>(), s));
        HIP_TRY(c, rocprim::exclusive_scan(nullptr, tmp_d, D.grp_cnt.p, D.grp_seg_off.p, (i64)0, nG + 1, rocprim::plus<i64>(), s));
    }
    const size_t tmp_bytes = std::max(std::max(tmp_a, tmp_b), std::max(tmp_c, tmp_d));
    HIP_TRY(c, D.tmp.grow(tmp_bytes));
    std::vector<int> list(r.tiny);
    list.insert(list.end(), r.small.begin(), r.small.end());
    list.insert(list.end(), r.large.begin(), r.large.end());
    HIP_TRY(c, hipMemcpyAsync(D.probs.p, r.probs.data(), D.probs.bytes((size_t)P), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(D.list.p, list.data(), D.list.bytes((size_t)P), hipMemcpyHostToDevice, s));
    if (C) {
        HIP_TRY(c, hipMemcpyAsync(D.rids.p, b->rids, D.rids.bytes(nC), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(D.col_prob.p, r.col_prob.data(), D.col_prob.bytes(nC), hipMemcpyHostToDevice, s));
    }
    HIP_TRY(c, hipMemcpyAsync(D.col_row_off.p, r.col_row_off.data(), D.col_row_off.bytes(nC + 1), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(D.prob_row_off.p, r.prob_row_off.data(), D.prob_row_off.bytes(P1), hipMemcpyHostToDevice, s));
    if (N) HIP_TRY(c, hipMemsetAsync(D.col_of.p, 0xff, D.col_of.bytes((size_t)N), s));
    HIP_TRY(c, hipMemsetAsync(D.cnt.p, 0, D.cnt.bytes(nCnt), s));
    HIP_TRY(c, hipMemsetAsync(D.refused.p, 0x7f, D.refused.bytes((size_t)P), s));
    HIP_TRY(c, hipMemsetAsync(D.grp_off.p, 0, D.grp_off.bytes(P1), s));
    // ---- the counts: column reduction, informative rows, totals
    HIP_TRY(c, hipEventRecord(c->rev[0], s));
    round_launch<false>(c, r);
    size_t tb = tmp_bytes;
    HIP_TRY(c, rocprim::exclusive_scan(D.tmp.p, tb, D.cnt.p, D.scan.p, (i64)0, nCnt, rocprim::plus<i64>(), s));
    HIP_TRY(c, hipEventRecord(c->rev[1], s));
    // ---- the gap groups
    const unsigned row_grid = capped_grid(std::max<i64>(G, P) + 1, 256, kCapGaps, k);       // (k_gap_groups: P + 1 offsets)
    if (G) {
        hipLaunchKernelGGL(k_gap_keys, dim3(capped_grid(C, 256, kCapGaps, k)), dim3(256), 0, s, C, D.col_prob.p, D.probs.p, D.rids.p, D.gap_off.p,
                           D.gaps.p, D.col_row_off.p, D.key.p, D.val.p, D.rows.p);
        RC_TRY(sort_pairs(c, D.tmp, nullptr, D.key.p, D.skey.p, D.val.p, D.sval.p, nG, key_bits));
        hipLaunchKernelGGL(k_gap_heads, dim3(row_grid), dim3(256), 0, s, G, D.skey.p, D.head.p);
        tb = tmp_bytes;
        HIP_TRY(c, rocprim::inclusive_scan(D.tmp.p, tb, D.head.p, D.gid.p, nG, rocprim::plus<i64>(), s));
        HIP_TRY(c, hipMemsetAsync(D.grp_cnt.p, 0, D.grp_cnt.bytes(nG + 1), s));
        hipLaunchKernelGGL(k_gap_groups, dim3(row_grid), dim3(256), 0, s, G, P, D.skey.p, D.sval.p, D.gid.p, D.prob_row_off.p, D.probs.p, D.inf_bits.p, D.rows.p,
                           D.grp.p, D.grp_prob.p, D.grp_cnt.p, D.grp_off.p, D.refused.p);
        tb = tmp_bytes;
        HIP_TRY(c, rocprim::exclusive_scan(D.tmp.p, tb, D.grp_cnt.p, D.grp_seg_off.p, (i64)0, nG + 1, rocprim::plus<i64>(), s));
        HIP_TRY(c, hipMemcpyAsync(c->h_tot.p, D.gid.p + (G - 1), c->h_tot.bytes(1), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(c->h_tot.p + 1, D.grp_seg_off.p + G, c->h_tot.bytes(1), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(c, hipEventRecord(c->rev[2], s));
    HIP_TRY(c, hipMemcpyAsync(H.scan.p, D.scan.p, D.scan.bytes(nCnt), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    i64 tot[kRoundCounts];
    for (int x = 0; x < kRoundCounts; ++x) tot[x] = H.scan.p[(size_t)x * P1 + P] - H.scan.p[(size_t)x * P1];
    const i64 n_inf = tot[0], n_sup = tot[1], n_corr = tot[2], n_pairs = tot[3], n_grp = G ? c->h_tot.p[0] : 0, n_grp_seg = G ? c->h_tot.p[1] : 0;
    if (n_inf < 0 || n_inf > r.n_inf_bits * 32 || n_sup < 0 || n_corr < 0 || n_pairs < 0 || n_pairs > c->parts.n_pairs || n_grp < 0 || n_grp > G || n_grp_seg < 0)
        return fail(c, FCLU_ERR_HIP, "round totals out of range (%lld informative, %lld support, %lld corrections, %lld pairs, %lld groups)", n_inf, n_sup, n_corr, n_pairs, n_grp);
    // ---- the fills
    HIP_TRY(c, D.inf_seg.grow((size_t)n_inf)); HIP_TRY(c, D.sup_off.grow((size_t)n_inf + 1)); HIP_TRY(c, D.sup_cols.grow((size_t)n_sup));
    HIP_TRY(c, D.corr_seg.grow((size_t)n_corr)); HIP_TRY(c, D.pairs.grow((size_t)n_pairs));
    HIP_TRY(c, D.grp_seg.grow((size_t)n_grp_seg)); HIP_TRY(c, D.grp_len.grow((size_t)n_grp_seg));
    HIP_TRY(c, hipEventRecord(c->rev[3], s));
    round_launch<true>(c, r);
    if (n_grp)
        hipLaunchKernelGGL(k_gap_fill, dim3(capped_grid(n_grp, 256, kCapGaps, k)), dim3(256), 0, s, D.gid.p, G, D.grp.p, D.grp_prob.p, D.grp_seg_off.p,
                           D.probs.p, D.inf_bits.p, D.seg_len.p, D.grp_seg.p, D.grp_len.p);
    HIP_TRY(c, hipEventRecord(c->rev[4], s));
    fclu_rounds &o = c->rounds;
    // (the three CSR offset arrays close with their total, which the host writes: room for it before the copies are enqueued)
    if (!resident) { HIP_TRY(c, H.sup_off.grow((size_t)n_inf + 1)); HIP_TRY(c, H.corr_off.grow(nC + 1)); HIP_TRY(c, H.grp_seg_off.grow((size_t)n_grp + 1)); }
    o = fclu_rounds();
    RC_TRY(fetch(c, H.refused, D.refused.p, (size_t)P, true, o.refused));
    RC_TRY(fetch(c, H.inf_bits, D.inf_bits.p, (size_t)r.n_inf_bits, true, o.inf_bits));
    RC_TRY(fetch(c, H.grp_off, D.grp_off.p, P1, true, o.grp_off));
    if (!resident) {
        const int2 *h_pairs = nullptr;
        RC_TRY(fetch(c, H.inf_seg, D.inf_seg.p, (size_t)n_inf, true, o.inf_seg));
        RC_TRY(fetch(c, H.sup_off, D.sup_off.p, (size_t)n_inf, true, o.sup_off));
        RC_TRY(fetch(c, H.sup_cols, D.sup_cols.p, (size_t)n_sup, true, o.sup_cols));
        RC_TRY(fetch(c, H.corr_off, D.corr_off.p, nC, true, o.corr_off));
        RC_TRY(fetch(c, H.corr_seg, D.corr_seg.p, (size_t)n_corr, true, o.corr_seg));
        RC_TRY(fetch(c, H.pairs, D.pairs.p, (size_t)n_pairs, true, h_pairs));
        o.pairs = &h_pairs->x;
        RC_TRY(fetch(c, H.grp, D.grp.p, 2 * (size_t)n_grp, true, o.grp));
        RC_TRY(fetch(c, H.grp_seg_off, D.grp_seg_off.p, (size_t)n_grp, true, o.grp_seg_off));
        RC_TRY(fetch(c, H.grp_seg, D.grp_seg.p, (size_t)n_grp_seg, true, o.grp_seg));
        RC_TRY(fetch(c, H.grp_len, D.grp_len.p, (size_t)n_grp_seg, true, o.grp_len));
        RC_TRY(fetch(c, H.rows, D.rows.p, 3 * nG, true, o.rows));
    }
    for (HostBuf<int64_t> *h : {&H.inf_bits_off, &H.inf_off, &H.col_off, &H.pair_off, &H.row_off}) HIP_TRY(c, h->grow(P1));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    if (!resident) { H.sup_off.p[n_inf] = n_sup; H.corr_off.p[C] = n_corr; H.grp_seg_off.p[n_grp] = n_grp_seg; }
    for (int p = 0; p <= P; ++p) {
        H.inf_bits_off.p[p] = r.inf_bits_off[(size_t)p];
        H.inf_off.p[p] = H.scan.p[p] - H.scan.p[0];
        H.pair_off.p[p] = H.scan.p[3 * P1 + p] - H.scan.p[3 * P1];
        H.col_off.p[p] = b->rid_off[p];
        H.row_off.p[p] = r.prob_row_off[(size_t)p];
    }
    for (int p = 0; p < P; ++p) if (H.refused.p[p] == 0x7f7f7f7f) H.refused.p[p] = -1;
    o.inf_bits_off = H.inf_bits_off.p; o.inf_off = H.inf_off.p; o.col_off = H.col_off.p; o.pair_off = H.pair_off.p; o.row_off = H.row_off.p;
    o.n_prob = P; o.n_cols = C; o.n_inf = n_inf; o.n_sup = n_sup; o.n_corr = n_corr; o.n_pairs = n_pairs; o.n_grp = n_grp; o.n_grp_seg = n_grp_seg;
    o.n_gap_rows = G;
    (void)hipEventElapsedTime(&c->rcount_ms, c->rev[0], c->rev[1]);
    (void)hipEventElapsedTime(&c->rgaps_ms, c->rev[1], c->rev[2]);
    (void)hipEventElapsedTime(&c->rfill_ms, c->rev[3], c->rev[4]);
    c->r_probs = r.probs;
    c->rounds_resident = resident;
    c->have_rounds = true;
    return FCLU_OK;
}

// ---- greedy incumbents of the last round's problems (fclu_round_incumbents) ---------------------------------------------------
int incumbents_device(fclu_ctx *c, const Knobs &k, const int32_t *g2, double lo_f, double hi_f, int32_t offset, int32_t max_seeds) {
    c->have_incs = false;
    c->iconf_ms = c->istart_ms = c->ipick_ms = 0.f;
    if (!c->have_rounds || !c->round_ready || !c->round_src_ok || !c->have_parts)
        return fail(c, FCLU_ERR_ARG, "fclu_round_incumbents: no successful fclu_round_models() stands behind the call (none was made, it failed, or a later "
                                     "call ended the rounds' source)");
    const fclu_rounds &o = c->rounds;
    const int P = o.n_prob;
    const i64 C = o.n_cols, G = o.n_gap_rows;
    if (max_seeds < 1) return fail(c, FCLU_ERR_ARG, "fclu_round_incumbents: max_seeds is %d, it must be at least 1", (int)max_seeds);
    if (offset < 0 || !(lo_f == lo_f) || !(hi_f == hi_f) || lo_f - lo_f != 0.0 || hi_f - hi_f != 0.0)
        return fail(c, FCLU_ERR_ARG, "fclu_round_incumbents: offset is negative or a factor is not finite");
    if (C > 0 && !g2) return fail(c, FCLU_ERR_ARG, "fclu_round_incumbents: g2 is null");
    for (i64 x = 0; x < C; ++x) if (g2[x] < 0) return fail(c, FCLU_ERR_ARG, "fclu_round_incumbents: g2[%lld] is negative", x);
    if ((int)c->r_probs.size() != P) return fail(c, FCLU_ERR_ARG, "fclu_round_incumbents: the round's problems are gone");
    HIP_TRY(c, hipSetDevice(c->device));
    auto &D = c->id;
    auto &H = c->ih;
    auto &RD = c->rd;
    hipStream_t s = c->stream;
    std::vector<IncProb> probs((size_t)P);
    std::vector<int> groups[3];                              // by path, as the models': rows in LDS (tiny, small), rows in device memory
    size_t lds[3] = {0, 0, 0};
    int height[3] = {0, 0, 0};
    i64 n_conf = 0, n_slots = 0, n_mrow = 0;
    for (int p = 0; p < P; ++p) {
        const RoundProb &rp = c->r_probs[(size_t)p];
        IncProb &d = probs[(size_t)p];
        d.col0 = rp.col0; d.rbits_off = rp.rbits_off; d.inf_off = rp.inf_off;
        d.n = rp.n; d.n_seg = rp.n_seg; d.w = rp.w; d.cw = std::max((rp.n + 31) / 32, 1);
        d.n_seeds = std::min(rp.n, (int)max_seeds); d.n_starts = d.n_seeds + 1;
        d.conf_off = n_conf; d.pair0 = o.pair_off[p]; d.pair1 = o.pair_off[p + 1]; d.grp0 = o.grp_off[p];
        d.slot0 = n_slots; d.mrow_off = n_mrow; d.max_lg = c->r_max_lg[(size_t)rp.tint];
        if (o.refused[p] >= 0) continue;                     // no model: cost2 -1, skipped
        if (d.n > kIncMaxCols) return fail(c, FCLU_ERR_UNSUPPORTED, "problem %d: %d columns, fclu_round_incumbents takes %d at the most", p, d.n, kIncMaxCols);
        if (d.pair0 < 0 || d.pair1 < d.pair0 || d.pair1 > o.n_pairs || d.grp0 < 0 || d.grp0 > o.n_grp)
            return fail(c, FCLU_ERR_HIP, "problem %d: the round's offsets are out of range", p);
        n_conf += (i64)d.n * d.cw; n_slots += d.n_starts; n_mrow += (i64)d.n_starts * d.cw;
        const size_t row_bytes = 2 * (size_t)d.n * (size_t)(d.w | 1) * 4;
        const int path = !k.round_lds || row_bytes > (size_t)k.round_lds_bytes ? 2 : row_bytes <= (size_t)std::min<i64>(k.round_lds_bytes, kRoundTinyBytes) ? 0 : 1;
        groups[path].push_back(p);
        lds[path] = std::max(lds[path], inc_lds_bytes(d.n, d.w, d.cw, path < 2));
        height[path] = std::max(height[path], d.n_starts);
    }
    const size_t need = D.conf.bytes((size_t)n_conf);
    if (need > D.conf.cap) {                                 // sized from the sum of R^2: a batch's that does not fit is refused
        HIP_TRY(c, D.conf.release());
        size_t free_b = 0, total_b = 0;
        HIP_TRY(c, hipMemGetInfo(&free_b, &total_b));
        if (need + need / 4 + (64u << 20) > free_b)
            return fail(c, FCLU_ERR_UNSUPPORTED, "the conflict matrices of this round (%lld bytes) do not fit the device's free memory (%lld bytes)", (i64)need, (i64)free_b);
    }
    std::vector<int> list;
    for (const auto &g : groups) list.insert(list.end(), g.begin(), g.end());
    const size_t nL = list.size(), nP = (size_t)P, nC = (size_t)C;
    HIP_TRY(c, D.conf.grow((size_t)n_conf)); HIP_TRY(c, D.probs.grow(nP)); HIP_TRY(c, D.list.grow(nL)); HIP_TRY(c, D.g2.grow(nC));
    HIP_TRY(c, D.start_cost2.grow((size_t)n_slots)); HIP_TRY(c, D.steps.grow(2 * (size_t)n_slots)); HIP_TRY(c, D.mrows.grow((size_t)n_mrow));
    HIP_TRY(c, D.cost2.grow(nP)); HIP_TRY(c, D.start.grow(nP)); HIP_TRY(c, D.grow.grow(nP)); HIP_TRY(c, D.repair.grow(nP));
    HIP_TRY(c, D.mem_cols.grow(nC)); HIP_TRY(c, D.mem_cnt.grow(nP));
    HIP_TRY(c, H.cost2.grow(nP)); HIP_TRY(c, H.start.grow(nP)); HIP_TRY(c, H.grow.grow(nP)); HIP_TRY(c, H.repair.grow(nP));
    HIP_TRY(c, H.mem_cols.grow(nC)); HIP_TRY(c, H.mem_cnt.grow(nP)); HIP_TRY(c, H.mem.grow(nC)); HIP_TRY(c, H.mem_off.grow(nP + 1));
    HIP_TRY(c, hipMemcpyAsync(D.probs.p, probs.data(), D.probs.bytes(nP), hipMemcpyHostToDevice, s));
    if (nL) HIP_TRY(c, hipMemcpyAsync(D.list.p, list.data(), D.list.bytes(nL), hipMemcpyHostToDevice, s));
    if (C) HIP_TRY(c, hipMemcpyAsync(D.g2.p, g2, D.g2.bytes(nC), hipMemcpyHostToDevice, s));
    if (n_conf) HIP_TRY(c, hipMemsetAsync(D.conf.p, 0, D.conf.bytes((size_t)n_conf), s));
    HIP_TRY(c, hipMemsetAsync(D.cost2.p, 0xff, D.cost2.bytes(nP), s));          // -1: what a refused problem keeps
    HIP_TRY(c, hipMemsetAsync(D.start.p, 0xff, D.start.bytes(nP), s));
    HIP_TRY(c, hipMemsetAsync(D.grow.p, 0, D.grow.bytes(nP), s));
    HIP_TRY(c, hipMemsetAsync(D.repair.p, 0, D.repair.bytes(nP), s));
    HIP_TRY(c, hipMemsetAsync(D.mem_cnt.p, 0, D.mem_cnt.bytes(nP), s));
    HIP_TRY(c, hipEventRecord(c->iev[0], s));
    if (nL) hipLaunchKernelGGL(k_inc_conflict, dim3((unsigned)nL), dim3(256), 0, s, D.list.p, D.probs.p, RD.pairs.p, D.conf.p);
    HIP_TRY(c, hipEventRecord(c->iev[1], s));
    size_t first = 0;
    for (int path = 0; path < 3; ++path) {
        const size_t n = groups[path].size();
        if (n) {
            const auto kernel = path < 2 ? k_inc_start<true> : k_inc_start<false>;
            hipLaunchKernelGGL(kernel, dim3((unsigned)n, (unsigned)height[path]), dim3(256), lds[path], s, D.list.p + first, D.probs.p, c->pd.ibits.p, c->pd.cbits.p,
                               RD.rids.p, RD.inf_bits.p, D.conf.p, D.g2.p, RD.col_row_off.p, G, RD.rows.p, RD.grp_seg_off.p, RD.grp_seg.p, RD.grp_len.p, (i64)o.n_grp,
                               (i64)o.n_grp_seg, lo_f, hi_f, (int)offset, D.start_cost2.p, D.steps.p, D.mrows.p);
        }
        first += n;
    }
    HIP_TRY(c, hipEventRecord(c->iev[2], s));
    if (nL)
        hipLaunchKernelGGL(k_inc_pick, dim3((unsigned)nL), dim3(256), 0, s, D.list.p, D.probs.p, D.start_cost2.p, D.steps.p, D.mrows.p, D.cost2.p, D.start.p, D.grow.p,
                           D.repair.p, D.mem_cols.p, D.mem_cnt.p);
    HIP_TRY(c, hipEventRecord(c->iev[3], s));
    HIP_TRY(c, hipMemcpyAsync(H.cost2.p, D.cost2.p, D.cost2.bytes(nP), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(H.start.p, D.start.p, D.start.bytes(nP), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(H.grow.p, D.grow.p, D.grow.bytes(nP), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(H.repair.p, D.repair.p, D.repair.bytes(nP), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(H.mem_cnt.p, D.mem_cnt.p, D.mem_cnt.bytes(nP), hipMemcpyDeviceToHost, s));
    if (C) HIP_TRY(c, hipMemcpyAsync(H.mem_cols.p, D.mem_cols.p, D.mem_cols.bytes(nC), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    i64 n_mem = 0;
    for (int p = 0; p < P; ++p) {                            // the members end to end
        const IncProb &d = probs[(size_t)p];
        const int cnt = H.mem_cnt.p[p];
        if (cnt < 0 || cnt > d.n) return fail(c, FCLU_ERR_HIP, "problem %d: %d members for %d columns", p, cnt, d.n);
        H.mem_off.p[p] = n_mem;
        for (int x = 0; x < cnt; ++x) H.mem.p[n_mem + x] = H.mem_cols.p[d.col0 + x];
        n_mem += cnt;
    }
    H.mem_off.p[P] = n_mem;
    fclu_incumbents &r = c->incs;
    r.n_prob = P; r.n_mem = n_mem; r.cost2 = H.cost2.p; r.start = H.start.p; r.grow_steps = H.grow.p; r.repair_steps = H.repair.p;
    r.mem_off = H.mem_off.p; r.mem = H.mem.p;
    (void)hipEventElapsedTime(&c->iconf_ms, c->iev[0], c->iev[1]);
    (void)hipEventElapsedTime(&c->istart_ms, c->iev[1], c->iev[2]);
    (void)hipEventElapsedTime(&c->ipick_ms, c->iev[2], c->iev[3]);
    c->have_incs = true;
    return FCLU_OK;
}

// ---- the searches over the last round's problems (fclu_round_exact, fclu_round_bnb, fclu_round_bnb_wide): the shared driver -------
// Problem p of the last round as the round calls describe it to their kernels, and whether its offsets lie inside the round's arrays
// (asked only of a problem that is taken).
void fill_exact_prob(const fclu_ctx *c, int p, ExactProb &d) {
    const fclu_rounds &o = c->rounds;
    const RoundProb &rp = c->r_probs[(size_t)p];
    d.col0 = rp.col0; d.inf0 = o.inf_off[p]; d.pair0 = o.pair_off[p]; d.pair1 = o.pair_off[p + 1];
    d.grp0 = o.grp_off[p]; d.grp1 = o.grp_off[p + 1]; d.row0 = o.row_off[p]; d.row1 = o.row_off[p + 1];
    d.max_lg = c->r_max_lg[(size_t)rp.tint];
    d.n = rp.n; d.n_inf = (int)(o.inf_off[p + 1] - o.inf_off[p]);
}

bool exact_prob_in_range(const fclu_ctx *c, int p, const ExactProb &d) {
    const fclu_rounds &o = c->rounds;
    return !(d.inf0 < 0 || o.inf_off[p + 1] < d.inf0 || o.inf_off[p + 1] > o.n_inf || d.n_inf > kMaxWords * 32 || d.pair0 < 0 || d.pair1 < d.pair0 ||
             d.pair1 > o.n_pairs || d.grp0 < 0 || d.grp1 < d.grp0 || d.grp1 > o.n_grp || d.row0 < 0 || d.row1 < d.row0 || d.row1 > o.n_gap_rows || d.col0 < 0 ||
             d.col0 + d.n > o.n_cols);
}

// What every round call checks before it touches the device, in the order the refusals fire: a round stands behind the call, the call's own
// numbers (own_args), offset and the factors, g2 is there, the call's other arrays are (own_arrays), g2 is not negative, the host still
// has the round's problems.  name: the entry point, for the message.
template <typename OwnArgs, typename OwnArrays>
int round_preconditions(fclu_ctx *c, const char *name, const int32_t *g2, double lo_f, double hi_f, int32_t offset, OwnArgs own_args, OwnArrays own_arrays) {
    if (!c->have_rounds || !c->round_ready || !c->round_src_ok || !c->have_parts)
        return fail(c, FCLU_ERR_ARG, "%s: no successful fclu_round_models() stands behind the call (none was made, it failed, or a later "
                                     "call ended the rounds' source)", name);
    const i64 C = c->rounds.n_cols;
    RC_TRY(own_args());
    if (offset < 0 || !(lo_f == lo_f) || !(hi_f == hi_f) || lo_f - lo_f != 0.0 || hi_f - hi_f != 0.0)
        return fail(c, FCLU_ERR_ARG, "%s: offset is negative or a factor is not finite", name);
    if (C > 0 && !g2) return fail(c, FCLU_ERR_ARG, "%s: g2 is null", name);
    RC_TRY(own_arrays());
    for (i64 x = 0; x < C; ++x) if (g2[x] < 0) return fail(c, FCLU_ERR_ARG, "%s: g2[%lld] is negative", name, x);
    if ((int)c->r_probs.size() != c->rounds.n_prob) return fail(c, FCLU_ERR_ARG, "%s: the round's problems are gone", name);
    return FCLU_OK;
}

// round_preconditions with what the two branch-and-bound calls add: the sizes (cols_limit: the most columns the call's kernels take), depth,
// node_cap, max_nodes, and the bounds.
int bnb_preconditions(fclu_ctx *c, const char *name, int cols_limit, const int32_t *g2, const int64_t *ub2, double lo_f, double hi_f, int32_t offset, int32_t min_cols,
                      int32_t max_cols, int32_t depth, int32_t node_cap, int64_t max_nodes) {
    return round_preconditions(c, name, g2, lo_f, hi_f, offset, [&]() -> int {
        if (min_cols < 0 || max_cols < min_cols || max_cols > cols_limit)
            return fail(c, FCLU_ERR_ARG, "%s: min_cols is %d and max_cols %d, they must be 0 <= min_cols <= max_cols <= %d", name, (int)min_cols, (int)max_cols, cols_limit);
        if (depth < 0 || depth > kBnbMaxDepth) return fail(c, FCLU_ERR_ARG, "%s: depth is %d, it must lie in [0, %d]", name, (int)depth, kBnbMaxDepth);
        if (node_cap < 1) return fail(c, FCLU_ERR_ARG, "%s: node_cap is %d, it must be at least 1", name, (int)node_cap);
        if (max_nodes < 1) return fail(c, FCLU_ERR_ARG, "%s: max_nodes is %lld, it must be at least 1", name, (i64)max_nodes);
        return FCLU_OK;
    }, [&]() -> int { return c->rounds.n_prob > 0 && !ub2 ? fail(c, FCLU_ERR_ARG, "%s: ub2 is null", name) : (int)FCLU_OK; });
}

// Every problem's descriptor (at(p): where the caller keeps it) and the call's candidates: the problems that have a model and are not
// outside the call's sizes (the caller's predicate), their offsets checked, in ascending (columns, problem).
template <typename At, typename Outside>
int select_probs(fclu_ctx *c, At at, Outside outside, std::vector<std::pair<int, int>> &order) {
    const fclu_rounds &o = c->rounds;
    for (int p = 0; p < o.n_prob; ++p) {
        ExactProb &d = at(p);
        fill_exact_prob(c, p, d);
        if (o.refused[p] >= 0 || outside(d)) continue;       // no model, or not this call's: its result stays the default
        if (!exact_prob_in_range(c, p, d)) return fail(c, FCLU_ERR_HIP, "problem %d: the round's offsets are out of range", p);
        if (o.n_grp == 0) d.row0 = d.row1 = 0;               // (a row has a group: nothing to index without one)
        order.emplace_back(d.n, p);
    }
    std::sort(order.begin(), order.end());
    return FCLU_OK;
}

// A call issues max_launches launches at the most (units, budget: the refusal's words for what a launch holds and what to lower), with an
// event in front of the first and behind each.
int launches_ready(fclu_ctx *c, const char *name, const char *units, const char *budget, const LaunchPlan &plan, int max_launches) {
    if (plan.n_launch() > (size_t)max_launches)
        return fail(c, FCLU_ERR_UNSUPPORTED, "%s: %lld %s need %lld launches, a call issues %d at the most: lower %s", name, plan.total_units, units,
                    (i64)plan.n_launch(), max_launches, budget);
    while (c->launch_ev.size() < plan.n_launch() + 1) {
        hipEvent_t e = nullptr;
        HIP_TRY(c, hipEventCreate(&e));
        c->launch_ev.push_back(e);
    }
    return FCLU_OK;
}

static_assert(sizeof(PlanItem) == sizeof(int4), "the kernels read a plan's items as int4");

// What every call uploads: the problems, the taken ones' list, the work items, g2.
template <typename Prob>
int upload_plan(fclu_ctx *c, fclu_ctx::RoundCallBufs &D, Buf<Prob> &d_probs, const std::vector<Prob> &probs, const LaunchPlan &plan, const int32_t *g2) {
    const size_t nP = probs.size(), nL = plan.list.size(), nI = plan.items.size(), nC = (size_t)c->rounds.n_cols;
    hipStream_t s = c->stream;
    HIP_TRY(c, d_probs.grow(nP)); HIP_TRY(c, D.list.grow(nL)); HIP_TRY(c, D.items.grow(nI)); HIP_TRY(c, D.g2.grow(nC));
    if (nP) HIP_TRY(c, hipMemcpyAsync(d_probs.p, probs.data(), d_probs.bytes(nP), hipMemcpyHostToDevice, s));
    if (nL) HIP_TRY(c, hipMemcpyAsync(D.list.p, plan.list.data(), D.list.bytes(nL), hipMemcpyHostToDevice, s));
    if (nI) HIP_TRY(c, hipMemcpyAsync(D.items.p, plan.items.data(), D.items.bytes(nI), hipMemcpyHostToDevice, s));
    if (nC) HIP_TRY(c, hipMemcpyAsync(D.g2.p, g2, D.g2.bytes(nC), hipMemcpyHostToDevice, s));
    return FCLU_OK;
}

// What the two searches add: the bounds, per problem its first task and task count, the zeroed per-problem results; and room for the
// results' pinned side (the mask words are the caller's).
template <typename Out>
int upload_search(fclu_ctx *c, fclu_ctx::SearchBufs &D, Buf<Out> &d_out, fclu_ctx::SearchHost<Out> &H, const int64_t *ub2, const LaunchPlan &plan) {
    const size_t nP = plan.n_units.size();
    hipStream_t s = c->stream;
    HIP_TRY(c, D.ub2.grow(nP)); HIP_TRY(c, D.task_off.grow(nP)); HIP_TRY(c, D.n_tasks.grow(nP)); HIP_TRY(c, d_out.grow(nP));
    HIP_TRY(c, H.out.grow(nP)); HIP_TRY(c, H.cost2.grow(nP)); HIP_TRY(c, H.nodes.grow(nP)); HIP_TRY(c, H.status.grow(nP)); HIP_TRY(c, H.capped.grow(nP));
    if (nP) {
        HIP_TRY(c, hipMemcpyAsync(D.ub2.p, ub2, D.ub2.bytes(nP), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(D.task_off.p, plan.unit_off.data(), D.task_off.bytes(nP), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(D.n_tasks.p, plan.n_units.data(), D.n_tasks.bytes(nP), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemsetAsync(d_out.p, 0, d_out.bytes(nP), s));
    }
    return FCLU_OK;
}

// A call's kernels on the stream and its times: prep() between ev[0] and ev[1], launch(l) for each of the plan's launches with an event
// behind it, behind() for what follows the last launch (a reduction and its event, the downloads); then the one wait of the call.
template <typename Prep, typename Launch, typename Behind>
int run_round_call(fclu_ctx *c, hipEvent_t *ev, size_t n_launch, float &prep_ms, float &search_ms, float &longest_ms, Prep prep, Launch launch, Behind behind) {
    hipStream_t s = c->stream;
    HIP_TRY(c, hipEventRecord(ev[0], s));
    prep();
    HIP_TRY(c, hipEventRecord(ev[1], s));
    HIP_TRY(c, hipEventRecord(c->launch_ev[0], s));
    for (size_t l = 0; l < n_launch; ++l) {
        launch(l);
        HIP_TRY(c, hipEventRecord(c->launch_ev[l + 1], s));
    }
    RC_TRY(behind());
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    (void)hipEventElapsedTime(&prep_ms, ev[0], ev[1]);
    if (n_launch) (void)hipEventElapsedTime(&search_ms, c->launch_ev[0], c->launch_ev[n_launch]);
    for (size_t l = 0; l < n_launch; ++l) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, c->launch_ev[l], c->launch_ev[l + 1]);
        longest_ms = std::max(longest_ms, ms);
    }
    return FCLU_OK;
}

// The two searches' results (fclu_bnb and fclu_bnb_wide have one layout): every problem's default, the taken ones' from what the device
// left in H.out, and the call's totals.  The mask words are the caller's.
template <typename Out, typename Result>
void fold_search(int P, const LaunchPlan &plan, fclu_ctx::SearchHost<Out> &H, const int64_t *ub2, Result &r) {
    for (int p = 0; p < P; ++p) { H.status.p[p] = FCLU_BNB_NOT_TAKEN; H.cost2.p[p] = -1; H.nodes.p[p] = 0; H.capped.p[p] = 0; }
    i64 nodes_total = 0;
    for (const int p : plan.list) {
        const Out &t = H.out.p[p];
        const bool found = t.cost2 >= 0;
        H.cost2.p[p] = found ? t.cost2 : -1; H.nodes.p[p] = t.nodes; H.capped.p[p] = (int32_t)t.capped;
        H.status.p[p] = t.capped > 0 ? FCLU_BNB_UNPROVEN : found ? FCLU_BNB_OPTIMAL : ub2[p] < 0 ? FCLU_BNB_INFEASIBLE : FCLU_BNB_UNPROVEN;
        nodes_total += t.nodes;
    }
    r.n_prob = P; r.status = H.status.p; r.cost2 = H.cost2.p; r.mask = H.mask.p; r.nodes = H.nodes.p; r.capped = H.capped.p;
    r.n_taken = (int64_t)plan.list.size(); r.n_launches = (int64_t)plan.n_launch(); r.nodes_total = nodes_total;
}

// ---- the exact solve of the last round's small problems (fclu_round_exact) ------------------------------------------------------
int exact_device(fclu_ctx *c, const Knobs &k, const int32_t *g2, double lo_f, double hi_f, int32_t offset, int32_t max_cols, int64_t max_masks) {
    c->have_exact = false;
    c->xprep_ms = c->xsearch_ms = c->xlongest_ms = 0.f;
    RC_TRY(round_preconditions(c, "fclu_round_exact", g2, lo_f, hi_f, offset, [&]() -> int {
        if (max_cols < 0 || max_cols > kExactMaxCols) return fail(c, FCLU_ERR_ARG, "fclu_round_exact: max_cols is %d, it must lie in [0, %d]", (int)max_cols, kExactMaxCols);
        if (max_masks < 1) return fail(c, FCLU_ERR_ARG, "fclu_round_exact: max_masks is %lld, it must be at least 1", (i64)max_masks);
        return FCLU_OK;
    }, []() -> int { return FCLU_OK; }));
    const fclu_rounds &o = c->rounds;
    const int P = o.n_prob;
    const i64 C = o.n_cols, G = o.n_gap_rows;
    HIP_TRY(c, hipSetDevice(c->device));
    auto &D = c->xd;
    auto &H = c->xh;
    auto &RD = c->rd;
    hipStream_t s = c->stream;
    // ---- which problems are taken: ascending (R, problem) while the running total of 2^R stays inside the budget
    std::vector<ExactProb> probs((size_t)P);
    std::vector<std::pair<int, int>> order;
    RC_TRY(select_probs(c, [&](int p) -> ExactProb & { return probs[(size_t)p]; }, [&](const ExactProb &d) { return d.n > max_cols; }, order));
    const int wg_masks = k.exact_slice ? (int)k.exact_slice : kExactWgMasks;
    const i64 launch_masks = k.exact_slice ? 16 * k.exact_slice : kExactLaunchMasks;
    const LaunchPlan plan = plan_launches(order, (size_t)P, [&](int p) { return 1ll << probs[(size_t)p].n; }, 1, max_masks, wg_masks, launch_masks, [&](int p) {
        const ExactProb &d = probs[(size_t)p];
        return (size_t)(32 + 4 * (2 * d.n_inf + 2 * d.n) + 15) & ~(size_t)15;
    });
    RC_TRY(launches_ready(c, "fclu_round_exact", "masks", "max_masks", plan, kExactMaxLaunches));
    const size_t nL = plan.list.size(), nP = (size_t)P, nC = (size_t)C;
    RC_TRY(upload_plan(c, D, D.probs, probs, plan, g2));
    HIP_TRY(c, D.tab.grow(2 * (size_t)o.n_inf)); HIP_TRY(c, D.conf.grow(nC)); HIP_TRY(c, D.gsup.grow((size_t)o.n_grp_seg)); HIP_TRY(c, D.best.grow(nP));
    HIP_TRY(c, H.best.grow(nP)); HIP_TRY(c, H.cost2.grow(nP)); HIP_TRY(c, H.mask.grow(nP));
    if (o.n_inf) HIP_TRY(c, hipMemsetAsync(D.tab.p, 0, D.tab.bytes(2 * (size_t)o.n_inf), s));
    if (C) HIP_TRY(c, hipMemsetAsync(D.conf.p, 0, D.conf.bytes(nC), s));
    HIP_TRY(c, hipMemsetAsync(D.best.p, 0xff, D.best.bytes(nP), s));            // kExactKeyNone
    RC_TRY(run_round_call(c, c->xev, plan.n_launch(), c->xprep_ms, c->xsearch_ms, c->xlongest_ms, [&] {
        if (nL)
            hipLaunchKernelGGL(k_narrow_prep<unsigned>, dim3((unsigned)nL), dim3(256), 0, s, D.list.p, D.probs.p, RD.inf_seg.p, RD.sup_off.p, (i64)o.n_inf, RD.sup_cols.p,
                               (i64)o.n_sup, RD.corr_off.p, C, RD.corr_seg.p, (i64)o.n_corr, RD.pairs.p, RD.grp_seg_off.p, RD.grp_seg.p, (i64)o.n_grp_seg, D.tab.p, D.conf.p,
                               D.gsup.p);
    }, [&](size_t l) {
        hipLaunchKernelGGL(k_exact_search, dim3((unsigned)(plan.launch_first[l + 1] - plan.launch_first[l])), dim3(256), plan.launch_lds[l], s,
                           D.items.p + plan.launch_first[l], D.probs.p, D.tab.p, D.conf.p, D.g2.p, RD.rows.p, G, RD.grp_seg_off.p, (i64)o.n_grp, (i64)o.n_grp_seg, D.gsup.p,
                           RD.grp_len.p, lo_f, hi_f, (int)offset, D.best.p);
    }, [&]() -> int {
        HIP_TRY(c, hipMemcpyAsync(H.best.p, D.best.p, D.best.bytes(nP), hipMemcpyDeviceToHost, s));
        return FCLU_OK;
    }));
    for (int p = 0; p < P; ++p) { H.cost2.p[p] = -2; H.mask.p[p] = 0u; }
    for (const int p : plan.list) {
        const u64 key = H.best.p[p];
        H.cost2.p[p] = key == kExactKeyNone ? -1 : ex_key_cost2(key);
        H.mask.p[p] = key == kExactKeyNone ? 0u : ex_key_mask(key);
    }
    fclu_exact &r = c->exact;
    r.n_prob = P; r.cost2 = H.cost2.p; r.mask = H.mask.p; r.n_taken = (int64_t)nL; r.n_masks = plan.total_units; r.n_launches = (int64_t)plan.n_launch();
    c->have_exact = true;
    return FCLU_OK;
}

// ---- the branch and bound over the last round's larger problems (fclu_round_bnb) ------------------------------------------------
int bnb_device(fclu_ctx *c, const Knobs &k, const int32_t *g2, const int64_t *ub2, double lo_f, double hi_f, int32_t offset, int32_t min_cols, int32_t max_cols,
               int32_t depth, int32_t node_cap, int64_t max_nodes) {
    c->have_bnb = false;
    c->bprep_ms = c->bsearch_ms = c->blongest_ms = 0.f;
    RC_TRY(bnb_preconditions(c, "fclu_round_bnb", kBnbMaxCols, g2, ub2, lo_f, hi_f, offset, min_cols, max_cols, depth, node_cap, max_nodes));
    const fclu_rounds &o = c->rounds;
    const int P = o.n_prob;
    const i64 C = o.n_cols, G = o.n_gap_rows;
    HIP_TRY(c, hipSetDevice(c->device));
    auto &D = c->bd;
    auto &H = c->bh;
    auto &RD = c->rd;
    hipStream_t s = c->stream;
    // ---- which problems are taken: ascending (R, problem) while the running total of 2^D x node_cap stays inside the budget
    std::vector<ExactProb> probs((size_t)P);
    std::vector<std::pair<int, int>> order;
    RC_TRY(select_probs(c, [&](int p) -> ExactProb & { return probs[(size_t)p]; },
                        [&](const ExactProb &d) { return d.n < min_cols || d.n > max_cols || d.n_inf > kBnbMaxInf; }, order));     // outside the sizes, or tables beyond LDS
    const i64 launch_tasks = k.bnb_slice ? k.bnb_slice : std::max<i64>(kBnbLaunchNodes / node_cap, 1);
    const i64 wg_tasks = std::min<i64>(kBnbWgTasks, launch_tasks);
    const LaunchPlan plan = plan_launches(order, (size_t)P, [&](int p) { return 1ll << std::min<int>(probs[(size_t)p].n, depth); }, node_cap, max_nodes, wg_tasks,
                                          launch_tasks, [&](int p) {
        const ExactProb &d = probs[(size_t)p];
        return (size_t)(16 * d.n_inf + 12 * d.n + 15) & ~(size_t)15;
    });
    RC_TRY(launches_ready(c, "fclu_round_bnb", "tasks", "max_nodes", plan, kBnbMaxLaunches));
    const size_t nL = plan.list.size(), nP = (size_t)P, nC = (size_t)C;
    RC_TRY(upload_plan(c, D, D.probs, probs, plan, g2));
    RC_TRY(upload_search(c, D, D.out, H, ub2, plan));
    HIP_TRY(c, D.tab.grow(2 * (size_t)o.n_inf)); HIP_TRY(c, D.conf.grow(nC)); HIP_TRY(c, D.gsup.grow((size_t)o.n_grp_seg));
    HIP_TRY(c, D.tasks.grow((size_t)plan.total_units)); HIP_TRY(c, H.mask.grow(nP));
    if (o.n_inf) HIP_TRY(c, hipMemsetAsync(D.tab.p, 0, D.tab.bytes(2 * (size_t)o.n_inf), s));
    if (C) HIP_TRY(c, hipMemsetAsync(D.conf.p, 0, D.conf.bytes(nC), s));
    RC_TRY(run_round_call(c, c->bev, plan.n_launch(), c->bprep_ms, c->bsearch_ms, c->blongest_ms, [&] {
        if (nL)
            hipLaunchKernelGGL(k_narrow_prep<u64>, dim3((unsigned)nL), dim3(256), 0, s, D.list.p, D.probs.p, RD.inf_seg.p, RD.sup_off.p, (i64)o.n_inf, RD.sup_cols.p,
                               (i64)o.n_sup, RD.corr_off.p, C, RD.corr_seg.p, (i64)o.n_corr, RD.pairs.p, RD.grp_seg_off.p, RD.grp_seg.p, (i64)o.n_grp_seg, D.tab.p, D.conf.p,
                               D.gsup.p);
    }, [&](size_t l) {
        hipLaunchKernelGGL(k_bnb_search, dim3((unsigned)(plan.launch_first[l + 1] - plan.launch_first[l])), dim3(256), plan.launch_lds[l], s,
                           D.items.p + plan.launch_first[l], D.probs.p, D.tab.p, D.conf.p, D.g2.p, D.ub2.p, RD.rows.p, G, RD.grp_seg_off.p, (i64)o.n_grp, (i64)o.n_grp_seg,
                           D.gsup.p, RD.grp_len.p, lo_f, hi_f, (int)offset, (int)depth, (int)node_cap, D.task_off.p, D.tasks.p);
    }, [&]() -> int {
        if (nL) hipLaunchKernelGGL(k_bnb_reduce, dim3((unsigned)nL), dim3(256), 0, s, D.list.p, D.task_off.p, D.n_tasks.p, D.tasks.p, D.out.p);
        HIP_TRY(c, hipEventRecord(c->bev[2], s));
        if (nP) HIP_TRY(c, hipMemcpyAsync(H.out.p, D.out.p, D.out.bytes(nP), hipMemcpyDeviceToHost, s));
        return FCLU_OK;
    }));
    fold_search(P, plan, H, ub2, c->bnb);
    for (int p = 0; p < P; ++p) H.mask.p[p] = 0ull;
    for (const int p : plan.list) if (H.out.p[p].cost2 >= 0) H.mask.p[p] = H.out.p[p].mask;
    c->have_bnb = true;
    return FCLU_OK;
}

// ---- the same search over the last round's problems of up to 1024 columns (fclu_round_bnb_wide, fclu_round_bnb_wide_passes) -----
// One pass is fclu_round_bnb_wide.  With more, a pass's search leaves the capped tasks' frames and open counts, k_bw_split scans them and
// the host reads the per-problem counts back -- the one read-back of a pass -- plans the next pass from them (the problems of this pass
// in their order, a task an open child) and k_bw_emit writes the records in front of its search.
int bnb_wide_device(fclu_ctx *c, const Knobs &k, const int32_t *g2, const int64_t *ub2, double lo_f, double hi_f, int32_t offset, int32_t min_cols,
                    int32_t max_cols, int32_t depth, int32_t node_cap, int64_t max_nodes, int32_t passes) {
    c->have_wide = false;
    c->wprep_ms = c->wsearch_ms = c->wlongest_ms = 0.f;
    c->w_pass_stats.clear();
    const char *name = passes < 0 ? "fclu_round_bnb_wide" : "fclu_round_bnb_wide_passes";
    if (passes < 0) passes = 1;
    else if (passes < 1 || passes > kBwMaxPasses) return fail(c, FCLU_ERR_ARG, "%s: passes is %d, it must lie in [1, %d]", name, (int)passes, kBwMaxPasses);
    RC_TRY(bnb_preconditions(c, name, kBwMaxCols, g2, ub2, lo_f, hi_f, offset, min_cols, max_cols, depth, node_cap, max_nodes));
    const fclu_rounds &o = c->rounds;
    const int P = o.n_prob;
    const i64 C = o.n_cols, G = o.n_gap_rows;
    HIP_TRY(c, hipSetDevice(c->device));
    auto &D = c->wd;
    auto &H = c->wh;
    auto &RD = c->rd;
    hipStream_t s = c->stream;
    const bool more = passes > 1;
    // ---- which problems are taken: ascending (R, problem) while the running total of 2^D x node_cap stays inside the budget
    std::vector<BwProb> probs((size_t)P);                    // (tab0 = conf0 = 0 until a problem is taken)
    std::vector<std::pair<int, int>> order;
    RC_TRY(select_probs(c, [&](int p) -> ExactProb & { return probs[(size_t)p].b; }, [&](const ExactProb &d) {
        return d.n < min_cols || d.n > max_cols || d.n_inf < 0 || bw_lds_bytes(d.n, d.n_inf) > kBwLdsBytes;                         // outside the sizes, or tables beyond LDS
    }, order));
    for (BwProb &q : probs) { q.W = bw_words(q.b.n); q.EW = bw_ewords(q.b.n_inf); }
    const i64 launch_tasks = k.bnb_wide_slice ? k.bnb_wide_slice : std::max<i64>(kBwLaunchNodes / node_cap, 1);
    const i64 wg_tasks = std::min<i64>(kBwWaves, launch_tasks);
    const auto lds_of = [&](int p) { return (size_t)bw_lds_bytes(probs[(size_t)p].b.n, probs[(size_t)p].b.n_inf); };
    LaunchPlan plan = plan_launches(order, (size_t)P, [&](int p) { return 1ll << std::min<int>(probs[(size_t)p].b.n, depth); }, node_cap, max_nodes, wg_tasks,
                                    launch_tasks, lds_of);
    i64 n_tab = 0, n_conf = 0;
    for (const int p : plan.list) {                          // the taken problems' tables and conflict rows, end to end
        BwProb &q = probs[(size_t)p];
        q.tab0 = n_tab; q.conf0 = n_conf;
        n_tab += bw_table_words(q.b.n, q.b.n_inf); n_conf += (i64)q.b.n * q.W;
    }
    RC_TRY(launches_ready(c, name, "tasks", "max_nodes", plan, kBwMaxLaunches));
    const size_t nL = plan.list.size(), nP = (size_t)P;
    RC_TRY(upload_plan(c, D, D.probs, probs, plan, g2));
    RC_TRY(upload_search(c, D, D.out, H, ub2, plan));
    HIP_TRY(c, D.tab.grow((size_t)n_tab)); HIP_TRY(c, D.conf.grow((size_t)n_conf)); HIP_TRY(c, D.gk.grow((size_t)o.n_grp_seg));
    HIP_TRY(c, D.tasks.grow((size_t)plan.total_units)); HIP_TRY(c, D.out_mask.grow(nP * kBwMaxWords)); HIP_TRY(c, H.mask.grow(nP * kBwMaxWords));
    if (nP) HIP_TRY(c, hipMemsetAsync(D.out_mask.p, 0, D.out_mask.bytes(nP * kBwMaxWords), s));
    if (n_tab) HIP_TRY(c, hipMemsetAsync(D.tab.p, 0, D.tab.bytes((size_t)n_tab), s));
    if (n_conf) HIP_TRY(c, hipMemsetAsync(D.conf.p, 0, D.conf.bytes((size_t)n_conf), s));
    // what a pass leaves for the next: the frames' places (a problem's tasks end to end, 3 W + 1 words each) and the per-task counts
    std::vector<i64> frame_off((size_t)P, 0), rec_off((size_t)P, -1);
    const auto size_pass = [&](const LaunchPlan &pl, fclu_ctx::BwPassBufs &B) -> int {
        i64 n_frame = 0;
        for (const int p : pl.list) { frame_off[(size_t)p] = n_frame; n_frame += pl.n_units[(size_t)p] * bw_frame_words(probs[(size_t)p].W); }
        const size_t nT = (size_t)pl.total_units;
        HIP_TRY(c, B.frames.grow((size_t)n_frame)); HIP_TRY(c, B.frame_off.grow(nP)); HIP_TRY(c, B.open_cnt.grow(nT)); HIP_TRY(c, B.open_off.grow(nT));
        HIP_TRY(c, D.n_open.grow(nP)); HIP_TRY(c, D.bound.grow(nP)); HIP_TRY(c, c->w_n_open.grow(nP));
        if (nP) HIP_TRY(c, hipMemcpyAsync(B.frame_off.p, frame_off.data(), B.frame_off.bytes(nP), hipMemcpyHostToDevice, s));
        return FCLU_OK;
    };
    // behind a pass's reduction: the scan of the open counts and the per-problem counts' way to the host
    const auto split_pass = [&](const LaunchPlan &pl, fclu_ctx::BwPassBufs &B, const i64 *task_off) -> int {
        if (nP) HIP_TRY(c, hipMemsetAsync(D.n_open.p, 0, D.n_open.bytes(nP), s));       // (a problem outside this pass has no open child)
        if (!pl.list.empty())
            hipLaunchKernelGGL(k_bw_split, dim3((unsigned)pl.list.size()), dim3(256), 0, s, D.list.p, task_off, D.n_tasks.p, B.open_cnt.p, B.open_off.p, D.n_open.p);
        if (nP) HIP_TRY(c, hipMemcpyAsync(c->w_n_open.p, D.n_open.p, D.n_open.bytes(nP), hipMemcpyDeviceToHost, s));
        return FCLU_OK;
    };
    const auto download = [&]() -> int {
        HIP_TRY(c, hipEventRecord(c->wev[2], s));
        if (nP) {
            HIP_TRY(c, hipMemcpyAsync(H.out.p, D.out.p, D.out.bytes(nP), hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipMemcpyAsync(H.mask.p, D.out_mask.p, D.out_mask.bytes(nP * kBwMaxWords), hipMemcpyDeviceToHost, s));
        }
        return FCLU_OK;
    };
    // a pass's row of fclu_round_bnb_wide_pass_stats, from the running results before and behind it
    std::vector<i64> nodes_before((size_t)P, 0);
    const auto pass_row = [&](const LaunchPlan &pl) {
        i64 nodes = 0, capped = 0;
        for (const int p : pl.list) { nodes += H.out.p[p].nodes - nodes_before[(size_t)p]; capped += H.out.p[p].capped; nodes_before[(size_t)p] = H.out.p[p].nodes; }
        for (const i64 x : {pl.total_units, nodes, capped, (i64)pl.n_launch(), (i64)pl.list.size()}) c->w_pass_stats.push_back(x);
    };
    if (more) RC_TRY(size_pass(plan, D.ps[1]));
    const BwSplitOut none = {nullptr, nullptr, nullptr};
    RC_TRY(run_round_call(c, c->wev, plan.n_launch(), c->wprep_ms, c->wsearch_ms, c->wlongest_ms, [&] {
        if (nL)
            hipLaunchKernelGGL(k_bw_prep, dim3((unsigned)nL), dim3(256), 0, s, D.list.p, D.probs.p, RD.inf_seg.p, RD.sup_off.p, (i64)o.n_inf, RD.sup_cols.p, (i64)o.n_sup,
                               RD.corr_off.p, C, RD.corr_seg.p, (i64)o.n_corr, RD.pairs.p, RD.grp_seg_off.p, RD.grp_seg.p, (i64)o.n_grp_seg, D.tab.p, D.conf.p, D.gk.p);
    }, [&](size_t l) {
        hipLaunchKernelGGL(k_bw_search, dim3((unsigned)(plan.launch_first[l + 1] - plan.launch_first[l])), dim3(kBwThreads), plan.launch_lds[l], s,
                           D.items.p + plan.launch_first[l], D.probs.p, D.tab.p, D.conf.p, D.g2.p, D.ub2.p, RD.rows.p, G, RD.grp_seg_off.p, (i64)o.n_grp, (i64)o.n_grp_seg,
                           D.gk.p, RD.grp_len.p, lo_f, hi_f, (int)offset, (int)depth, (int)node_cap, D.task_off.p, D.tasks.p,
                           more ? BwSplitOut{D.ps[1].frames.p, D.ps[1].frame_off.p, D.ps[1].open_cnt.p} : none);
    }, [&]() -> int {
        if (nL) hipLaunchKernelGGL(k_bw_reduce, dim3((unsigned)nL), dim3(256), 0, s, D.list.p, D.probs.p, D.task_off.p, D.n_tasks.p, D.tasks.p, D.out.p, D.out_mask.p);
        if (more && nL) hipLaunchKernelGGL(k_bw_bound, dim3((unsigned)((nL + 255) / 256)), dim3(256), 0, s, D.list.p, (int)nL, D.ub2.p, D.out.p, D.bound.p);
        if (more) RC_TRY(split_pass(plan, D.ps[1], D.task_off.p));
        return download();
    }));
    pass_row(plan);
    LaunchPlan first;                                        // (the results cover the first pass's problems: fold_search's list)
    first.list = plan.list;
    i64 n_launches = (i64)plan.n_launch();
    // ---- the later passes
    const int4 *prev_items = D.items.p;
    const i64 *prev_task_off = D.task_off.p;
    for (int pass = 2; pass <= passes; ++pass) {
        // the problems of the pass before, in their order, that have open children and not more than a pass may hold
        std::vector<std::pair<int, int>> next;
        for (const int p : plan.list) {
            const i64 n = c->w_n_open.p[p];
            if (n < 0 || n > plan.n_units[(size_t)p] * (i64)(kBwMaxCols + 1)) return fail(c, FCLU_ERR_HIP, "%s: problem %d: %lld open children of %lld tasks", name, p, n, plan.n_units[(size_t)p]);
            if (n > 0 && n <= kBwMaxPassTasks) next.emplace_back(probs[(size_t)p].b.n, p);
        }
        const i64 wg_recs = std::min<i64>(k.bnb_wide_item, launch_tasks);
        LaunchPlan pl = plan_launches(next, (size_t)P, [&](int p) { return (long long)c->w_n_open.p[p]; }, node_cap, max_nodes, wg_recs, launch_tasks, lds_of);
        if (pl.list.empty()) break;                          // nothing is open, or the first open problem is beyond the budget: no launch
        RC_TRY(launches_ready(c, name, "tasks", "max_nodes", pl, kBwMaxLaunches));
        fclu_ctx::BwPassBufs &B = D.ps[pass & 1], &Bp = D.ps[(pass - 1) & 1];
        const size_t nLk = pl.list.size(), nI = pl.items.size();
        i64 n_rec = 0;
        std::fill(rec_off.begin(), rec_off.end(), -1);
        for (const int p : pl.list) { rec_off[(size_t)p] = n_rec; n_rec += pl.n_units[(size_t)p] * bw_record_words(probs[(size_t)p].W); }
        const size_t prev_n_items = plan.items.size();
        HIP_TRY(c, B.items.grow(nI)); HIP_TRY(c, B.task_off.grow(nP)); HIP_TRY(c, D.rec.grow((size_t)n_rec)); HIP_TRY(c, D.rec_off.grow(nP));
        HIP_TRY(c, D.tasks.grow((size_t)pl.total_units));
        HIP_TRY(c, hipMemcpyAsync(D.list.p, pl.list.data(), D.list.bytes(nLk), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(B.items.p, pl.items.data(), B.items.bytes(nI), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(B.task_off.p, pl.unit_off.data(), B.task_off.bytes(nP), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(D.n_tasks.p, pl.n_units.data(), D.n_tasks.bytes(nP), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(D.rec_off.p, rec_off.data(), D.rec_off.bytes(nP), hipMemcpyHostToDevice, s));
        RC_TRY(size_pass(pl, B));
        float prep_ms = 0.f, search_ms = 0.f;
        RC_TRY(run_round_call(c, c->wev, pl.n_launch(), prep_ms, search_ms, c->wlongest_ms, [&] {
            hipLaunchKernelGGL(k_bw_emit, dim3((unsigned)prev_n_items), dim3(kBwThreads), 0, s, prev_items, D.probs.p, D.conf.p, prev_task_off, Bp.frames.p, Bp.frame_off.p,
                               Bp.open_cnt.p, Bp.open_off.p, D.n_open.p, D.rec.p, D.rec_off.p);
        }, [&](size_t l) {
            hipLaunchKernelGGL(k_bw_search_from, dim3((unsigned)(pl.launch_first[l + 1] - pl.launch_first[l])), dim3(kBwThreads), pl.launch_lds[l], s,
                               B.items.p + pl.launch_first[l], D.probs.p, D.tab.p, D.conf.p, D.g2.p, D.bound.p, RD.rows.p, G, RD.grp_seg_off.p, (i64)o.n_grp,
                               (i64)o.n_grp_seg, D.gk.p, RD.grp_len.p, lo_f, hi_f, (int)offset, (int)depth, (int)node_cap, B.task_off.p, D.tasks.p, D.rec.p, D.rec_off.p,
                               BwSplitOut{B.frames.p, B.frame_off.p, B.open_cnt.p});
        }, [&]() -> int {
            hipLaunchKernelGGL(k_bw_fold, dim3((unsigned)nLk), dim3(256), 0, s, D.list.p, D.probs.p, B.task_off.p, D.n_tasks.p, D.tasks.p, D.ub2.p, D.out.p, D.out_mask.p,
                               D.bound.p);
            RC_TRY(split_pass(pl, B, B.task_off.p));
            return download();
        }));
        c->wprep_ms += prep_ms; c->wsearch_ms += search_ms;
        pass_row(pl);
        n_launches += (i64)pl.n_launch();
        prev_items = B.items.p; prev_task_off = B.task_off.p;
        plan = std::move(pl);
    }
    fold_search(P, first, H, ub2, c->wide);
    c->wide.n_launches = n_launches;
    c->have_wide = true;
    return FCLU_OK;
}

// ---- the read-out of the last round's accepted sets (fclu_round_readout) --------------------------------------------------------
// Every refusal is the host's, before any launch: the kernels get sets that are inside their problems, and clamp what they read all the same.
int readout_device(fclu_ctx *c, const Knobs &k, const int64_t *sel_off, const int32_t *sel) {
    c->have_readout = false;
    c->oexon_ms = c->ocorr_ms = 0.f;
    c->paths[FCLU_PATH_READOUT_SETS] = c->paths[FCLU_PATH_READOUT_MEMBERS] = c->paths[FCLU_PATH_READOUT_STORES] = 0;
    if (!c->have_rounds || !c->round_ready || !c->round_src_ok || !c->have_parts)
        return fail(c, FCLU_ERR_ARG, "fclu_round_readout: no successful fclu_round_models() stands behind the call (none was made, it failed, or a later "
                                     "call ended the rounds' source)");
    const fclu_rounds &o = c->rounds;
    const int P = o.n_prob;
    if ((int)c->r_probs.size() != P || c->r_lab_off.size() != c->r_n_seg.size() + 1) return fail(c, FCLU_ERR_ARG, "fclu_round_readout: the round's problems are gone");
    if (!sel_off) return fail(c, FCLU_ERR_ARG, "fclu_round_readout: sel_off is null");
    if (sel_off[0] != 0) return fail(c, FCLU_ERR_ARG, "fclu_round_readout: sel_off starts at 0");
    auto &D = c->od;
    auto &H = c->oh;
    const size_t P1 = (size_t)P + 1;
    for (HostBuf<int64_t> *h : {&H.exon_off, &H.mem_off, &H.corr_off, &H.e_off}) HIP_TRY(c, h->grow(P1));
    std::vector<ReadoutProb> probs;
    i64 n_exon = 0, n_corr = 0, n_e = 0, n_slots = 0;
    bool wide = false, narrow = false;
    for (int p = 0; p < P; ++p) {
        const i64 m0 = sel_off[p], n = sel_off[p + 1] - m0;
        H.exon_off.p[p] = n_exon; H.mem_off.p[p] = m0; H.corr_off.p[p] = n_corr; H.e_off.p[p] = n_e;
        if (n < 0 || sel_off[p + 1] > 2147483647ll) return fail(c, FCLU_ERR_ARG, "problem %d: sel_off falls or is too large", p);
        if (n == 0) continue;
        if (!sel) return fail(c, FCLU_ERR_ARG, "fclu_round_readout: sel is null");
        const RoundProb &rp = c->r_probs[(size_t)p];
        if (o.refused[p] >= 0)
            return fail(c, FCLU_ERR_ARG, "problem %d: a set for a refused problem (column %d has a gap that ends on an uninformative segment: no model)", p, (int)o.refused[p]);
        int prev = -1;
        for (i64 x = 0; x < n; ++x) {
            const int col = sel[m0 + x];
            if (col < 0 || col >= rp.n) return fail(c, FCLU_ERR_ARG, "problem %d: column %d is outside the problem's %d columns", p, col, rp.n);
            if (col <= prev) return fail(c, FCLU_ERR_ARG, "problem %d: column %d follows column %d; a set is strictly ascending", p, col, prev);
            prev = col;
        }
        const i64 n_inf = o.inf_off[p + 1] - o.inf_off[p];
        if (n_inf < 0 || n_inf > rp.n_seg || rp.w > kMaxWords) return fail(c, FCLU_ERR_HIP, "problem %d: the round's offsets are out of range", p);
        ReadoutProb d;
        d.col0 = rp.col0; d.rbits_off = rp.rbits_off; d.lab_off = c->r_lab_off[(size_t)rp.tint]; d.inf_off = rp.inf_off; d.sel0 = m0;
        d.exon0 = n_exon; d.corr0 = n_corr; d.e0 = n_e; d.slot0 = n_slots;
        d.n = rp.n; d.n_sel = (int)n; d.n_seg = rp.n_seg; d.w = rp.w; d.lw = std::max((rp.n_seg + 15) / 16, 1);
        d.n_reps = (int)(c->r_rep_off[(size_t)rp.tint + 1] - c->r_rep_off[(size_t)rp.tint]); d.n_e = (int)n_inf;
        d.g_log2 = 0; while (d.g_log2 < 6 && (1 << d.g_log2) < d.w) ++d.g_log2;
        probs.push_back(d);
        // The census' store word is the host's prediction from the rows' addresses, not a report of the kernel's: ro_store_halves' rule
        // restated (a word's address is its row's plus a multiple of 32, so a row is aligned or not as a whole).
        for (i64 x = 0; x < n; ++x) {
            const bool aligned = ((n_corr + x * rp.n_seg) & 15) == 0;
            wide = wide || (aligned && rp.n_seg >= 16);
            narrow = narrow || (rp.n_seg > 0 && (!aligned || (rp.n_seg & 15)));
        }
        n_exon += rp.n_seg; n_corr += n * (i64)rp.n_seg; n_e += n_inf;
        n_slots += ((n << d.g_log2) + 63) / 64 * 64;
    }
    const i64 n_mem = sel_off[P];
    H.exon_off.p[P] = n_exon; H.mem_off.p[P] = n_mem; H.corr_off.p[P] = n_corr; H.e_off.p[P] = n_e;
    const size_t nS = probs.size();
    HIP_TRY(c, H.exons.grow((size_t)n_exon)); HIP_TRY(c, H.corr.grow((size_t)n_corr)); HIP_TRY(c, H.e.grow((size_t)n_e));
    if (nS) {
        HIP_TRY(c, hipSetDevice(c->device));
        hipStream_t s = c->stream;
        const i64 n_words = o.inf_bits_off[P];
        HIP_TRY(c, D.probs.grow(nS)); HIP_TRY(c, D.sel.grow((size_t)n_mem)); HIP_TRY(c, D.ex_bits.grow((size_t)n_words));
        HIP_TRY(c, D.exons.grow((size_t)n_exon)); HIP_TRY(c, D.corr.grow((size_t)n_corr)); HIP_TRY(c, D.e.grow((size_t)n_e));
        HIP_TRY(c, hipMemcpyAsync(D.probs.p, probs.data(), D.probs.bytes(nS), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(D.sel.p, sel, D.sel.bytes((size_t)n_mem), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipEventRecord(c->oev[0], s));
        hipLaunchKernelGGL(k_readout_exons, dim3((unsigned)nS), dim3(256), 0, s, D.probs.p, c->rd.rids.p, D.sel.p, c->pd.ibits.p, c->rd.inf_bits.p, D.ex_bits.p, D.exons.p,
                           D.e.p);
        HIP_TRY(c, hipEventRecord(c->oev[1], s));
        hipLaunchKernelGGL(k_readout_corr, dim3(capped_grid(n_slots, 256, kCapSlots, k)), dim3(256), 0, s, (int)nS, n_slots, D.probs.p, c->rd.rids.p, D.sel.p,
                           c->pd.labels.p, c->pd.cbits.p, c->rd.inf_bits.p, D.ex_bits.p, D.corr.p);
        HIP_TRY(c, hipEventRecord(c->oev[2], s));
        if (n_exon) HIP_TRY(c, hipMemcpyAsync(H.exons.p, D.exons.p, (size_t)n_exon, hipMemcpyDeviceToHost, s));
        if (n_corr) HIP_TRY(c, hipMemcpyAsync(H.corr.p, D.corr.p, (size_t)n_corr, hipMemcpyDeviceToHost, s));
        if (n_e) HIP_TRY(c, hipMemcpyAsync(H.e.p, D.e.p, (size_t)n_e, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        HIP_TRY(c, hipGetLastError());
        (void)hipEventElapsedTime(&c->oexon_ms, c->oev[0], c->oev[1]);
        (void)hipEventElapsedTime(&c->ocorr_ms, c->oev[1], c->oev[2]);
    }
    fclu_readout &r = c->readout;
    r.n_prob = P; r.n_sets = (int64_t)nS; r.n_mem = n_mem; r.n_exon_bytes = n_exon; r.n_corr_bytes = n_corr; r.n_e = n_e;
    r.exon_off = H.exon_off.p; r.mem_off = H.mem_off.p; r.corr_off = H.corr_off.p; r.e_off = H.e_off.p;
    r.exons = H.exons.p; r.corr = H.corr.p; r.e = H.e.p;
    c->paths[FCLU_PATH_READOUT_SETS] = (int32_t)nS; c->paths[FCLU_PATH_READOUT_MEMBERS] = (int32_t)n_mem;
    c->paths[FCLU_PATH_READOUT_STORES] = (wide ? FCLU_STORE_WIDE : 0) | (narrow ? FCLU_STORE_BYTES : 0);
    c->have_readout = true;
    return FCLU_OK;
}

}  // namespace

// ---- the C ABI ------------------------------------------------------------------------------------------------------------
extern "C" {

int fclu_abi_version(void) { return 1; }

int fclu_create(int device, fclu_ctx **out) {
    if (!out) return FCLU_ERR_ARG;
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, FCLU_ERR_HIP, "no HIP device available: %s (this library has no CPU fallback)",
                    e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    if (device < 0 || device >= n) return fail(nullptr, FCLU_ERR_ARG, "device ordinal out of range");
    fclu_ctx *c = new fclu_ctx();
    c->device = device;
    e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    for (hipEvent_t &ev : c->events) if (e == hipSuccess) e = hipEventCreate(&ev);
    const struct { const void *kernel; int lds; } dyn[] = {                // the most dynamic LDS a launch asks for
        {reinterpret_cast<const void *>(k_cc_lds), 80 * 1024},
        {reinterpret_cast<const void *>(k_compat<false>), 2 * kTile * (kMaxWords | 1) * 4},
        {reinterpret_cast<const void *>(k_compat<true>), 2 * kTile * (kRankWords | 1) * 6},
        {reinterpret_cast<const void *>(k_prune_lds), 150 * 1024},
        {reinterpret_cast<const void *>(k_round<true, false>), kRoundLdsBytes},
        {reinterpret_cast<const void *>(k_round<true, true>), kRoundLdsBytes},
        {reinterpret_cast<const void *>(k_inc_start<true>), (int)inc_lds_bytes(0, kMaxWords, (kIncMaxCols + 31) / 32, false) + kRoundLdsBytes},
        {reinterpret_cast<const void *>(k_inc_start<false>), (int)inc_lds_bytes(0, kMaxWords, (kIncMaxCols + 31) / 32, false)},
        {reinterpret_cast<const void *>(k_exact_search), kExactLdsBytes},
        {reinterpret_cast<const void *>(k_bnb_search), kBnbLdsBytes},
        {reinterpret_cast<const void *>(k_bw_search), kBwLdsBytes},
        {reinterpret_cast<const void *>(k_bw_search_from), kBwLdsBytes}};
    for (const auto &d : dyn) if (e == hipSuccess) e = hipFuncSetAttribute(d.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, d.lds);
    if (e != hipSuccess) {
        fail(nullptr, FCLU_ERR_HIP, "context creation failed: %s", hipGetErrorString(e));
        delete c;
        return FCLU_ERR_HIP;
    }
    *out = c;
    return FCLU_OK;
}

void fclu_destroy(fclu_ctx *c) { delete c; }

const char *fclu_last_error(const fclu_ctx *c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int fclu_compat_graph(fclu_ctx *c, const fclu_batch *b, int32_t prune, uint64_t *adj_out, int32_t *rounds_out) {
    if (!c || !b || !adj_out) return FCLU_ERR_ARG;
    return compat_device(c, read_knobs(), b, prune, adj_out, rounds_out);
}

int fclu_last_timing(fclu_ctx *c, float *compat_ms, float *prune_ms) { return c ? two_times(compat_ms, c->compat_ms, prune_ms, c->prune_ms) : FCLU_ERR_ARG; }

int fclu_last_paths(fclu_ctx *c, int32_t *out, int32_t n) {
    if (!c || !out || n < 0) return FCLU_ERR_ARG;
    std::copy_n(c->paths, std::min<int32_t>(n, FCLU_N_PATHS), out);
    return FCLU_OK;
}

int fclu_partition(fclu_ctx *c, const fclu_batch *b, const int64_t *mem_off, const int32_t *mem, int32_t maximum_ilp_size) {
    if (!c || !b) return FCLU_ERR_ARG;
    c->have_parts = false;
    c->round_src_ok = c->round_ready = c->have_rounds = false;
    if (b->n_tint <= 0) return fail(c, FCLU_ERR_ARG, "fclu_partition: empty batch");
    RC_TRY(check_members(c, b->row_off[b->n_tint], mem_off, mem, maximum_ilp_size));
    const Knobs k = read_knobs();
    RC_TRY(compat_device(c, k, b, 1, nullptr, nullptr));
    return partition_device(c, k, b->n_tint, b->row_off[b->n_tint], mem_off, mem, 0, maximum_ilp_size);
}

int fclu_partition_adj(fclu_ctx *c, int32_t n_tint, const int64_t *row_off, const int64_t *adj_off, const uint64_t *adj,
                       const int64_t *mem_off, const int32_t *mem, int32_t maximum_ilp_size) {
    if (!c || !row_off || !adj_off) return FCLU_ERR_ARG;
    c->have_parts = false;
    c->round_src_ok = c->round_ready = c->have_rounds = false;
    if (n_tint <= 0) return fail(c, FCLU_ERR_ARG, "fclu_partition_adj: empty batch");
    HIP_TRY(c, hipSetDevice(c->device));
    const Knobs k = read_knobs();
    const int T = n_tint;
    const i64 R = row_off[T], n_adj = adj_off[T];
    if (row_off[0] != 0 || adj_off[0] != 0 || R < 0 || R >= (1ll << 31)) return fail(c, FCLU_ERR_ARG, "fclu_partition_adj: bad row_off / adj_off");
    if (n_adj > 0 && !adj) return FCLU_ERR_ARG;
    std::vector<TintDesc> tints((size_t)T);
    std::vector<int> row_tint((size_t)R);
    for (int t = 0; t < T; ++t) {
        TintDesc &d = tints[(size_t)t];
        RC_TRY(describe_tint(c, t, k, 0, row_off, nullptr, nullptr, adj_off, d));
        RC_TRY(check_adj(c, t, d, adj));
        std::fill_n(row_tint.begin() + d.row0, d.n, t);
    }
    RC_TRY(check_members(c, R, mem_off, mem, maximum_ilp_size));
    c->h_tints = tints;
    c->adj_cur = 0;
    c->compat_ms = c->prune_ms = 0.f;
    std::fill_n(c->paths, FCLU_N_PATHS, 0);
    if (R > 0) {
        hipStream_t s = c->stream;
        HIP_TRY(c, c->tints.grow((size_t)T));
        HIP_TRY(c, c->row_tint.grow((size_t)R));
        HIP_TRY(c, c->adj[0].grow((size_t)n_adj));
        HIP_TRY(c, hipMemcpyAsync(c->tints.p, tints.data(), c->tints.bytes((size_t)T), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(c->row_tint.p, row_tint.data(), c->row_tint.bytes((size_t)R), hipMemcpyHostToDevice, s));
        if (n_adj) HIP_TRY(c, hipMemcpyAsync(c->adj[0].p, adj, c->adj[0].bytes((size_t)n_adj), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipStreamSynchronize(s));              // (the host vectors go out of scope)
    }
    return partition_device(c, k, T, R, mem_off, mem, 0, maximum_ilp_size);
}

int fclu_partition_results(fclu_ctx *c, fclu_parts *out) {
    if (!c || !out) return FCLU_ERR_ARG;
    if (!c->have_parts) return fail(c, FCLU_ERR_ARG, "fclu_partition_results: no result (the last fclu_partition call failed or none was made)");
    *out = c->parts;
    return FCLU_OK;
}

int fclu_partition_timing(fclu_ctx *c, float *components_ms, float *pairs_ms) {
    return c ? two_times(components_ms, c->components_ms, pairs_ms, c->pairs_ms) : FCLU_ERR_ARG;
}

int fclu_preprocess(fclu_ctx *c, const fclu_reads *reads) {
    if (!c) return FCLU_ERR_ARG;
    Staged st;
    i64 n_reps = 0;
    RC_TRY(preprocess_device(c, read_knobs(), reads, 1, st, n_reps));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    preprocess_times(c, n_reps);
    c->have_prep = true;
    return FCLU_OK;
}

int fclu_partition_reads(fclu_ctx *c, const fclu_reads *reads, int32_t maximum_ilp_size) {
    if (!c) return FCLU_ERR_ARG;
    c->have_parts = false;
    c->have_prep = false;
    if (maximum_ilp_size < 1) return fail(c, FCLU_ERR_ARG, "maximum_ilp_size is %d: it must be at least 1", (int)maximum_ilp_size);
    const Knobs k = read_knobs();
    Staged st;
    i64 n_reps = 0;
    RC_TRY(preprocess_device(c, k, reads, 1, st, n_reps));
    if (!st.empty) RC_TRY(compat_run(c, st, k, 1, nullptr, nullptr));          // (it synchronises: the pinned copies have landed)
    else HIP_TRY(c, hipStreamSynchronize(c->stream));
    preprocess_times(c, n_reps);
    c->have_prep = true;
    RC_TRY(partition_device(c, k, reads->n_tint, st.R, nullptr, nullptr, n_reps, maximum_ilp_size));
    round_source(c, reads);
    return FCLU_OK;
}

int fclu_preprocess_results(fclu_ctx *c, fclu_prep *out) {
    if (!c || !out) return FCLU_ERR_ARG;
    if (!c->have_prep) return fail(c, FCLU_ERR_ARG, "fclu_preprocess_results: no result (the last fclu_preprocess / fclu_partition_reads call failed or none was made)");
    *out = c->prep;
    return FCLU_OK;
}

int fclu_preprocess_timing(fclu_ctx *c, float *rows_ms, float *dedupe_ms) { return c ? two_times(rows_ms, c->rows_ms, dedupe_ms, c->dedupe_ms) : FCLU_ERR_ARG; }

int fclu_group_reads(fclu_ctx *c, const fclu_segment *in) {
    if (!c) return FCLU_ERR_ARG;
    i64 n_reps = 0;
    return group_device(c, read_knobs(), in, false, n_reps);
}

int fclu_partition_segment(fclu_ctx *c, const fclu_segment *in, int32_t maximum_ilp_size) {
    if (!c) return FCLU_ERR_ARG;
    c->have_parts = false;
    c->have_prep = false;
    c->have_groups = false;
    if (maximum_ilp_size < 1) return fail(c, FCLU_ERR_ARG, "maximum_ilp_size is %d: it must be at least 1", (int)maximum_ilp_size);
    const Knobs k = read_knobs();
    i64 n_reps = 0;
    RC_TRY(group_device(c, k, in, true, n_reps));
    // the reps as fclu_reads: offsets from the grouping's pinned results, rows and tails on the device already
    fclu_reads rd = {};
    rd.n_tint = in->n_tint; rd.rep_off = c->gh.rep_off.p; rd.n_seg = in->n_seg; rd.lab_off = c->gh.rep_lab_off.p;
    Staged st;
    const int rc = [&]() {
        RC_TRY(preprocess_device(c, k, &rd, 1, st, n_reps, true));
        if (!st.empty) RC_TRY(compat_run(c, st, k, 1, nullptr, nullptr));
        else HIP_TRY(c, hipStreamSynchronize(c->stream));
        preprocess_times(c, n_reps);
        c->have_prep = true;
        return partition_device(c, k, in->n_tint, st.R, nullptr, nullptr, n_reps, maximum_ilp_size);
    }();
    if (rc != FCLU_OK) c->have_groups = c->have_prep = false;
    else round_source(c, &rd);
    return rc;
}

int fclu_group_results(fclu_ctx *c, fclu_groups *out) {
    if (!c || !out) return FCLU_ERR_ARG;
    if (!c->have_groups) return fail(c, FCLU_ERR_ARG, "fclu_group_results: no result (the last fclu_group_reads / fclu_partition_segment call failed or none was made)");
    *out = c->groups;
    return FCLU_OK;
}

int fclu_group_timing(fclu_ctx *c, float *keys_ms, float *dedupe_ms) { return c ? two_times(keys_ms, c->gkeys_ms, dedupe_ms, c->gdedupe_ms) : FCLU_ERR_ARG; }

int fclu_round_setup(fclu_ctx *c, const int64_t *gap_off, const int32_t *gaps, const int64_t *seg_off, const int32_t *seg_len) {
    return c ? round_setup(c, gap_off, gaps, seg_off, seg_len) : FCLU_ERR_ARG;
}

int fclu_round_models(fclu_ctx *c, const fclu_round_batch *b) { return c ? round_device(c, read_knobs(), b, false) : FCLU_ERR_ARG; }

int fclu_round_models_resident(fclu_ctx *c, const fclu_round_batch *b) { return c ? round_device(c, read_knobs(), b, true) : FCLU_ERR_ARG; }

int fclu_round_results(fclu_ctx *c, fclu_rounds *out) {
    if (!c || !out) return FCLU_ERR_ARG;
    if (!c->have_rounds) return fail(c, FCLU_ERR_ARG, "fclu_round_results: no result (the last fclu_round_models call failed or none was made)");
    *out = c->rounds;
    if (c->rounds_resident)                                  // (the library keeps these four for its own later calls; the model they index is not here)
        out->inf_off = out->pair_off = out->grp_off = out->row_off = nullptr;
    return FCLU_OK;
}

int fclu_round_timing(fclu_ctx *c, float *count_ms, float *gaps_ms, float *fill_ms) {
    return c ? three_times(count_ms, c->rcount_ms, gaps_ms, c->rgaps_ms, fill_ms, c->rfill_ms) : FCLU_ERR_ARG;
}

int fclu_round_incumbents(fclu_ctx *c, const int32_t *g2, double lo_f, double hi_f, int32_t offset, int32_t max_seeds) {
    return c ? incumbents_device(c, read_knobs(), g2, lo_f, hi_f, offset, max_seeds) : FCLU_ERR_ARG;
}

int fclu_round_incumbent_results(fclu_ctx *c, fclu_incumbents *out) {
    if (!c || !out) return FCLU_ERR_ARG;
    if (!c->have_incs || !c->have_rounds)
        return fail(c, FCLU_ERR_ARG, "fclu_round_incumbent_results: no result (the last fclu_round_incumbents call failed, none was made, or a later call ended it)");
    *out = c->incs;
    return FCLU_OK;
}

int fclu_round_incumbent_timing(fclu_ctx *c, float *conflict_ms, float *starts_ms, float *pick_ms) {
    return c ? three_times(conflict_ms, c->iconf_ms, starts_ms, c->istart_ms, pick_ms, c->ipick_ms) : FCLU_ERR_ARG;
}

int fclu_round_exact(fclu_ctx *c, const int32_t *g2, double lo_f, double hi_f, int32_t offset, int32_t max_cols, int64_t max_masks) {
    return c ? exact_device(c, read_knobs(), g2, lo_f, hi_f, offset, max_cols, max_masks) : FCLU_ERR_ARG;
}

int fclu_round_exact_results(fclu_ctx *c, fclu_exact *out) { return c && out ? round_call_results(c, c->have_exact, c->exact, out, "fclu_round_exact") : FCLU_ERR_ARG; }

int fclu_round_exact_timing(fclu_ctx *c, float *prep_ms, float *search_ms, float *longest_launch_ms) {
    return c ? three_times(prep_ms, c->xprep_ms, search_ms, c->xsearch_ms, longest_launch_ms, c->xlongest_ms) : FCLU_ERR_ARG;
}

int fclu_round_bnb(fclu_ctx *c, const int32_t *g2, const int64_t *ub2, double lo_f, double hi_f, int32_t offset, int32_t min_cols, int32_t max_cols,
                   int32_t depth, int32_t node_cap, int64_t max_nodes) {
    return c ? bnb_device(c, read_knobs(), g2, ub2, lo_f, hi_f, offset, min_cols, max_cols, depth, node_cap, max_nodes) : FCLU_ERR_ARG;
}

int fclu_round_bnb_results(fclu_ctx *c, fclu_bnb *out) { return c && out ? round_call_results(c, c->have_bnb, c->bnb, out, "fclu_round_bnb") : FCLU_ERR_ARG; }

int fclu_round_bnb_timing(fclu_ctx *c, float *prep_ms, float *search_ms, float *longest_launch_ms) {
    return c ? three_times(prep_ms, c->bprep_ms, search_ms, c->bsearch_ms, longest_launch_ms, c->blongest_ms) : FCLU_ERR_ARG;
}

int fclu_round_bnb_wide(fclu_ctx *c, const int32_t *g2, const int64_t *ub2, double lo_f, double hi_f, int32_t offset, int32_t min_cols, int32_t max_cols,
                        int32_t depth, int32_t node_cap, int64_t max_nodes) {
    return c ? bnb_wide_device(c, read_knobs(), g2, ub2, lo_f, hi_f, offset, min_cols, max_cols, depth, node_cap, max_nodes, -1) : FCLU_ERR_ARG;
}

int fclu_round_bnb_wide_passes(fclu_ctx *c, const int32_t *g2, const int64_t *ub2, double lo_f, double hi_f, int32_t offset, int32_t min_cols, int32_t max_cols,
                               int32_t depth, int32_t node_cap, int64_t max_nodes, int32_t passes) {
    return c ? bnb_wide_device(c, read_knobs(), g2, ub2, lo_f, hi_f, offset, min_cols, max_cols, depth, node_cap, max_nodes, passes < 0 ? 0 : passes) : FCLU_ERR_ARG;
}

int fclu_round_bnb_wide_pass_stats(fclu_ctx *c, int64_t *out, int32_t n) {
    if (!c || n < 0 || (n > 0 && !out)) return FCLU_ERR_ARG;
    if (!c->have_wide || !c->have_rounds)
        return fail(c, FCLU_ERR_ARG, "fclu_round_bnb_wide_pass_stats: no result (the last fclu_round_bnb_wide call failed, none was made, or a later call ended it)");
    for (size_t x = 0; x < 5 * (size_t)n; ++x) out[x] = x < c->w_pass_stats.size() ? c->w_pass_stats[x] : 0;
    return FCLU_OK;
}

int fclu_round_bnb_wide_results(fclu_ctx *c, fclu_bnb_wide *out) { return c && out ? round_call_results(c, c->have_wide, c->wide, out, "fclu_round_bnb_wide") : FCLU_ERR_ARG; }

int fclu_round_bnb_wide_timing(fclu_ctx *c, float *prep_ms, float *search_ms, float *longest_launch_ms) {
    return c ? three_times(prep_ms, c->wprep_ms, search_ms, c->wsearch_ms, longest_launch_ms, c->wlongest_ms) : FCLU_ERR_ARG;
}

int fclu_round_readout(fclu_ctx *c, const int64_t *sel_off, const int32_t *sel) { return c ? readout_device(c, read_knobs(), sel_off, sel) : FCLU_ERR_ARG; }

int fclu_round_readout_results(fclu_ctx *c, fclu_readout *out) {
    if (!c || !out) return FCLU_ERR_ARG;
    if (!c->have_readout || !c->have_rounds)
        return fail(c, FCLU_ERR_ARG, "fclu_round_readout_results: no result (the last fclu_round_readout call failed, none was made, or a later call ended it)");
    *out = c->readout;
    return FCLU_OK;
}

int fclu_round_readout_timing(fclu_ctx *c, float *exons_ms, float *corr_ms) { return c ? two_times(exons_ms, c->oexon_ms, corr_ms, c->ocorr_ms) : FCLU_ERR_ARG; }

}  // extern "C"

#ifdef FREDDIE_SOURCE_HASH
/* what this binary was built from (freddie_amd/build.py looks for the marker in the file) */
static const char freddie_source_stamp[] __attribute__((used)) = "FREDDIE_SRC_HASH=" FREDDIE_SOURCE_HASH;
#endif
