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
#include "freddie_cluster.h"

#include <hip/hip_runtime.h>
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
    i64 rep0, lab_off, rbits_off, slot0;   // first rep; first label word; first word of the reps' I / C rows; first lane slot of k_rows
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
        const i64 rep = d.rep0 + (ok ? r : 0);
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
        const unsigned *a = ibits + d.rbits_off + (i64)(rep - d.rep0) * d.w;
        const int fa = first[rep], la = last[rep], ta = tail[rep];
        int lead = rep;
        for (i64 j = bstart[k]; j < k; ++j) {
            const int other = sval[j];
            if (first[other] != fa || last[other] != la || tail[other] != ta) continue;
            const unsigned *b = ibits + d.rbits_off + (i64)(other - d.rep0) * d.w;
            bool same = true;
            for (int w = 0; w < d.w; ++w) if (a[w] != b[w]) { same = false; break; }
            if (same) { lead = other; break; }
        }
        leader[rep] = lead;
        flag[rep] = lead == rep ? 1 : 0;
    }
}

// row_off[t] = the number of leaders in front of tint t's first rep (node_id: the exclusive scan of flag, n_reps + 1 entries)
__global__ void __launch_bounds__(256) k_row_off(int n_tint, i64 n_reps, const PrepTint *pt, const int *node_id, i64 *row_off) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t <= n_tint) row_off[t] = node_id[t < n_tint ? pt[t].rep0 : n_reps];
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
        nval[rep] = (int)(rep - p.rep0);
        if (lead == rep) {
            node_rep[node] = (int)(rep - p.rep0);
            nfirst[node] = first[rep]; nlast[node] = last[rep]; ntail[node] = tail[rep];
            const unsigned *src = ibits + p.rbits_off + (rep - p.rep0) * p.w;
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

}  // namespace

struct GrowBuf {              // device buffer that lives with the context and only ever grows
    void *p = nullptr;
    size_t cap = 0;
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};
struct HostBuf {              // the same in pinned host memory
    void *p = nullptr;
    size_t cap = 0;
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};
struct fclu_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[3] = {};
    std::string err;
    float compat_ms = 0.f, prune_ms = 0.f;
    GrowBuf tints, tiles, row_tint, bits, first, last, tail, adj[2], deg, changed, word_tint, tint_word0, deg1, pass_any, small_tints, small_rounds;
    int *h_flags = nullptr;   // pinned: per-pass flags of a burst + per-tint flags
    size_t h_flags_cap = 0;
    // fclu_partition(): the batch the last graph call left on the device, work arrays, results (pinned, context-owned)
    std::vector<TintDesc> h_tints;
    int adj_cur = 0;
    hipEvent_t pev[6] = {};
    float components_ms = 0.f, pairs_ms = 0.f;
    GrowBuf parent, skey, rows, sval, comp_start, comp_end, chunk_end, head, part_id, smult, rid_pos, cnt, pair_base, d_label, d_nodes,
            d_tint_part_off, d_part_node_off, d_part_rid_off, d_part_pair_off, mem_off, mem, d_part_rids, d_pairs, tmp;
    HostBuf h_cc_flags, h_tint_part_off, h_part_node_off, h_part_nodes, h_part_rid_off, h_part_rids, h_part_pair_off, h_pairs, h_label;
    fclu_parts parts = {};
    bool have_parts = false;
    // fclu_preprocess() / fclu_partition_reads(): device arrays (P_*) and the pinned copies fclu_preprocess_results() hands out (Q_*)
    GrowBuf pd[32];
    HostBuf ph[24];
    hipEvent_t qev[6] = {};
    float rows_ms = 0.f, dedupe_ms = 0.f;
    fclu_prep prep = {};
    bool have_prep = false;
};

namespace {

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

hipError_t grow(GrowBuf &b, size_t bytes) {
    if (b.p && bytes <= b.cap) return hipSuccess;
    if (b.p) { hipError_t e = hipFree(b.p); b.p = nullptr; b.cap = 0; if (e != hipSuccess) return e; }
    const size_t want = (bytes ? bytes : 16) + bytes / 4;
    hipError_t e = hipMalloc(&b.p, want);
    if (e == hipSuccess) b.cap = want;
    return e;
}
constexpr int kBurst = 4;     // pruning passes enqueued per host round trip

// connected components of a tint in one workgroup's LDS: the pruning's criterion; FCLU_PART_LDS=0: never (tests)
int cc_in_lds(int n, int aw) {
    const char *e = getenv("FCLU_PART_LDS");
    return (!(e && e[0] == '0') && n > 0 && (i64)n * aw <= kPruneLdsWords) ? 1 : 0;
}

#define HIP_TRY(c, expr)                                                                                     \
    do {                                                                                                     \
        hipError_t e__ = (expr);                                                                             \
        if (e__ != hipSuccess) return fail((c), FCLU_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e__));      \
    } while (0)

int compat_device(fclu_ctx *c, const fclu_batch *b, int32_t prune, uint64_t *adj_out, int32_t *rounds_out);
int check_members(fclu_ctx *c, i64 R, const int64_t *mem_off, const int32_t *mem, int32_t maximum_ilp_size);
int partition_device(fclu_ctx *c, int T, i64 R, const int64_t *mem_off, const int32_t *mem, i64 n_mem_device, int32_t maximum_ilp_size);

}  // namespace

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
    for (int i = 0; e == hipSuccess && i < 3; ++i) e = hipEventCreate(&c->ev[i]);
    for (int i = 0; e == hipSuccess && i < 6; ++i) e = hipEventCreate(&c->pev[i]);
    for (int i = 0; e == hipSuccess && i < 6; ++i) e = hipEventCreate(&c->qev[i]);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_cc_lds), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_compat<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                2 * kTile * (kMaxWords | 1) * 4);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_compat<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                2 * kTile * (kRankWords | 1) * 6);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_prune_lds), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    if (e != hipSuccess) {
        fail(nullptr, FCLU_ERR_HIP, "context creation failed: %s", hipGetErrorString(e));
        delete c;
        return FCLU_ERR_HIP;
    }
    *out = c;
    return FCLU_OK;
}

void fclu_destroy(fclu_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    for (int i = 0; i < 3; ++i) if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
    for (int i = 0; i < 6; ++i) if (c->pev[i]) (void)hipEventDestroy(c->pev[i]);
    for (int i = 0; i < 6; ++i) if (c->qev[i]) (void)hipEventDestroy(c->qev[i]);
    for (GrowBuf &b : c->pd) if (b.p) (void)hipFree(b.p);
    for (HostBuf &b : c->ph) if (b.p) (void)hipHostFree(b.p);
    GrowBuf *bufs[] = {&c->tints, &c->tiles, &c->row_tint, &c->bits, &c->first, &c->last, &c->tail, &c->adj[0], &c->adj[1], &c->deg,
                       &c->changed, &c->word_tint, &c->tint_word0, &c->deg1, &c->pass_any, &c->small_tints, &c->small_rounds,
                       &c->parent, &c->skey, &c->rows, &c->sval, &c->comp_start, &c->comp_end, &c->chunk_end, &c->head, &c->part_id, &c->smult,
                       &c->rid_pos, &c->cnt, &c->pair_base, &c->d_label, &c->d_nodes, &c->d_tint_part_off, &c->d_part_node_off,
                       &c->d_part_rid_off, &c->d_part_pair_off, &c->mem_off, &c->mem, &c->d_part_rids, &c->d_pairs, &c->tmp};
    for (GrowBuf *b : bufs) if (b->p) (void)hipFree(b->p);
    HostBuf *hbufs[] = {&c->h_cc_flags, &c->h_tint_part_off, &c->h_part_node_off, &c->h_part_nodes, &c->h_part_rid_off, &c->h_part_rids,
                        &c->h_part_pair_off, &c->h_pairs, &c->h_label};
    for (HostBuf *b : hbufs) if (b->p) (void)hipHostFree(b->p);
    if (c->h_flags) (void)hipHostFree(c->h_flags);
    delete c;
}

const char *fclu_last_error(const fclu_ctx *c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int fclu_compat_graph(fclu_ctx *c, const fclu_batch *b, int32_t prune, uint64_t *adj_out, int32_t *rounds_out) {
    if (!c || !b || !adj_out) return FCLU_ERR_ARG;
    return compat_device(c, b, prune, adj_out, rounds_out);
}

}  // extern "C"

namespace {

// What the host derives from a batch's shape (stage_tints) and the graph kernels are launched with (compat_run).
struct Staged {
    int T = 0, n_tiles = 0, max_w = 1, max_aw_large = 0, n_words = 0;
    i64 R = 0, n_bits = 0, n_adj = 0;
    bool any_large = false, empty = false;
    std::vector<int> small_tints;                        // pruned whole in LDS (k_prune_lds); FCLU_PRUNE_LDS=0: none (tests)
    size_t small_lds = 0;
    // what the uploads read: alive until the call that staged them has synchronised
    std::vector<TintDesc> tints;
    std::vector<int4> tiles;
    std::vector<int> row_tint;
    std::vector<int2> word_tint;                         // every adjacency word column of every tint: (tint, word)
    std::vector<i64> tint_word0;
};

// Host staging of a batch: the shape checks, the tints' descriptors, tiles and row / word maps, device buffers grown and the maps
// uploaded.  b: the caller's rows, checked against their tint (fclu_compat_graph, fclu_partition), or null when the rows were made on
// the device (fclu_partition_reads: first / last / tail in range and bits inside [first, last] by construction).
int stage_tints(fclu_ctx *c, int T, const int64_t *row_off, const int32_t *n_seg, const int64_t *bits_off, const int64_t *adj_off,
                int32_t prune, const fclu_batch *b, Staged &st) {
    HIP_TRY(c, hipSetDevice(c->device));
    const i64 R = row_off[T];
    // host-side shape checks: the kernels index with these and nothing else
    std::vector<TintDesc> &tints = st.tints;
    std::vector<int4> &tiles = st.tiles;
    std::vector<int> &row_tint = st.row_tint;
    std::vector<int2> &word_tint = st.word_tint;
    std::vector<i64> &tint_word0 = st.tint_word0;
    std::vector<int> &small_tints = st.small_tints;
    tints.assign((size_t)T, TintDesc()); row_tint.assign((size_t)R, 0); tint_word0.assign((size_t)T + 1, 0);
    const char *lds_env = getenv("FCLU_PRUNE_LDS");
    const bool lds_ok = !(lds_env && lds_env[0] == '0');
    const char *ldsw_env = getenv("FCLU_PRUNE_LDS_WORDS");                // (tests: a lower limit, so that small tints take both ways in one batch)
    const i64 lds_words = (ldsw_env && atoll(ldsw_env) > 0 && atoll(ldsw_env) < kPruneLdsWords) ? atoll(ldsw_env) : kPruneLdsWords;
    size_t small_lds = 0;
    bool any_large = false;
    int max_w = 1, max_aw_large = 0;
    for (int t = 0; t < T; ++t) {
        TintDesc &d = tints[(size_t)t];
        d.row0 = row_off[t];
        const i64 n = row_off[t + 1] - d.row0;
        if (n < 0 || n > (1 << 30) || n_seg[t] < 0) return fail(c, FCLU_ERR_ARG, "tint %d: bad row count or segment count", t);
        d.n = (int)n; d.n_seg = n_seg[t];
        d.w = (d.n_seg + 31) / 32; if (d.w < 1) d.w = 1;
        d.aw = (d.n + 63) / 64;
        d.bits_off = bits_off[t]; d.adj_off = adj_off[t];
        d.in_lds = (prune && lds_ok && d.n > 0 && d.n <= 65535 && (i64)d.n * d.aw <= lds_words) ? 1 : 0;
        d.cc_lds = cc_in_lds(d.n, d.aw);
        if (d.in_lds) { small_tints.push_back(t); small_lds = std::max(small_lds, ((size_t)2 * d.n * d.aw + d.aw) * 8 + (size_t)d.n * 2 + 16); }
        else if (d.n > 0) { any_large = true; max_aw_large = std::max(max_aw_large, d.aw); }
        if (bits_off[t + 1] - d.bits_off != (i64)d.n * d.w) return fail(c, FCLU_ERR_ARG, "tint %d: bits_off does not match rows x words", t);
        if (adj_off[t + 1] - d.adj_off != (i64)d.n * d.aw) return fail(c, FCLU_ERR_ARG, "tint %d: adj_off does not match rows x words", t);
        if (d.w > kMaxWords) return fail(c, FCLU_ERR_UNSUPPORTED, "tint %d has %d segments; this build stages at most %d", t, d.n_seg, kMaxWords * 32);
        if (d.w > max_w) max_w = d.w;
        for (i64 r = 0; r < n; ++r) {
            row_tint[(size_t)(d.row0 + r)] = t;
            if (!b) continue;
            const int f = b->first[d.row0 + r], l = b->last[d.row0 + r];
            if (f < -1 || l >= (d.n_seg > 0 ? d.n_seg : 1) || b->tail[d.row0 + r] > 2) return fail(c, FCLU_ERR_ARG, "tint %d read %lld: first/last/tail out of range", t, r);
            // a read's bits lie inside [first, last] (first / last ARE its first and last covered segment, :175-183): k_compat counts on it
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
        for (int ti = 0; ti < d.aw; ++ti) for (int tj = ti; tj < d.aw; ++tj) tiles.push_back(make_int4(t, ti, tj, 0));   // (on and above the diagonal)
        for (int z = 0; z < d.aw; ++z) word_tint.push_back(make_int2(t, z));
        tint_word0[(size_t)t + 1] = (i64)word_tint.size();
    }
    const i64 n_bits = bits_off[T], n_adj = adj_off[T];
    const int n_tiles = (int)tiles.size();
    st.T = T; st.R = R; st.n_bits = n_bits; st.n_adj = n_adj; st.n_tiles = n_tiles; st.max_w = max_w; st.max_aw_large = max_aw_large;
    st.any_large = any_large; st.small_lds = small_lds; st.n_words = (int)word_tint.size();
    c->compat_ms = c->prune_ms = 0.f;
    c->h_tints = tints;
    c->adj_cur = 0;
    st.empty = n_tiles == 0 || R == 0;
    if (st.empty) return FCLU_OK;

    GrowBuf &d_tints = c->tints, &d_tiles = c->tiles, &d_row_tint = c->row_tint, &d_bits = c->bits, &d_first = c->first, &d_last = c->last,
            &d_tail = c->tail, &d_deg = c->deg, &d_changed = c->changed, &d_word_tint = c->word_tint, &d_tint_word0 = c->tint_word0,
            &d_deg1 = c->deg1, &d_pass_any = c->pass_any;
    GrowBuf *d_adj = c->adj;
    HIP_TRY(c, grow(d_tints, tints.size() * sizeof(TintDesc)));
    HIP_TRY(c, grow(d_tiles, tiles.size() * sizeof(int4)));
    HIP_TRY(c, grow(d_row_tint, (size_t)R * 4));
    HIP_TRY(c, grow(d_bits, (size_t)n_bits * 4));
    HIP_TRY(c, grow(d_first, (size_t)R * 4));
    HIP_TRY(c, grow(d_last, (size_t)R * 4));
    HIP_TRY(c, grow(d_tail, (size_t)R));
    HIP_TRY(c, grow(d_adj[0], (size_t)n_adj * 8));
    HIP_TRY(c, grow(d_adj[1], (size_t)n_adj * 8));
    HIP_TRY(c, grow(d_deg, (size_t)R * 4));
    HIP_TRY(c, grow(d_changed, (size_t)kBurst * T * 4));
    HIP_TRY(c, grow(d_word_tint, word_tint.size() * sizeof(int2)));
    HIP_TRY(c, grow(d_tint_word0, tint_word0.size() * 8));
    HIP_TRY(c, grow(d_deg1, word_tint.size() * 8));
    HIP_TRY(c, grow(d_pass_any, (size_t)kBurst * 4));
    HIP_TRY(c, grow(c->small_tints, small_tints.size() * 4 + 4));
    HIP_TRY(c, grow(c->small_rounds, (size_t)T * 4));
    {
        const size_t need = ((size_t)kBurst * T + kBurst) * 4;
        if (need > c->h_flags_cap) {
            if (c->h_flags) HIP_TRY(c, hipHostFree(c->h_flags));
            c->h_flags = nullptr; c->h_flags_cap = 0;
            HIP_TRY(c, hipHostMalloc((void **)&c->h_flags, need + need / 4, hipHostMallocDefault));
            c->h_flags_cap = need + need / 4;
        }
    }
    hipStream_t s = c->stream;
    HIP_TRY(c, hipMemcpyAsync(d_tints.p, tints.data(), tints.size() * sizeof(TintDesc), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_tiles.p, tiles.data(), tiles.size() * sizeof(int4), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_row_tint.p, row_tint.data(), (size_t)R * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_word_tint.p, word_tint.data(), word_tint.size() * sizeof(int2), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_tint_word0.p, tint_word0.data(), tint_word0.size() * 8, hipMemcpyHostToDevice, s));
    return FCLU_OK;
}

// The graph of a staged batch whose rows (c->bits / first / last / tail) are on the device: compatibility, then pruning.  The pruned
// matrix stays on the device in c->adj[c->adj_cur] (with the tints' descriptors in c->tints / c->h_tints and c->row_tint) for
// partition_device(); adj_out may be null.
int compat_run(fclu_ctx *c, const Staged &st, int32_t prune, uint64_t *adj_out, int32_t *rounds_out) {
    const int T = st.T, n_tiles = st.n_tiles, max_w = st.max_w, max_aw_large = st.max_aw_large;
    const i64 R = st.R, n_adj = st.n_adj;
    const bool any_large = st.any_large;
    const std::vector<int> &small_tints = st.small_tints;
    const size_t small_lds = st.small_lds;
    GrowBuf &d_tints = c->tints, &d_tiles = c->tiles, &d_row_tint = c->row_tint, &d_bits = c->bits, &d_first = c->first, &d_last = c->last,
            &d_tail = c->tail, &d_deg = c->deg, &d_changed = c->changed, &d_word_tint = c->word_tint, &d_tint_word0 = c->tint_word0,
            &d_deg1 = c->deg1, &d_pass_any = c->pass_any;
    GrowBuf *d_adj = c->adj;
    hipStream_t s = c->stream;

    const int grid = n_tiles < 8192 ? n_tiles : 8192;
    // rows of at most kRankWords words: the rank tables ride along (FCLU_RANK=0 keeps the masked sums: tests)
    const char *rank_env = getenv("FCLU_RANK");
    const bool rank = max_w <= kRankWords && !(rank_env && rank_env[0] == '0');
    const size_t lds = (size_t)2 * kTile * (max_w | 1) * (rank ? 6 : 4);
    HIP_TRY(c, hipEventRecord(c->ev[0], s));
    if (rank)
        hipLaunchKernelGGL(k_compat<true>, dim3(grid), dim3(256), lds, s, n_tiles, d_tiles.as<int4>(), d_tints.as<TintDesc>(),
                           d_bits.as<unsigned>(), d_first.as<int>(), d_last.as<int>(), d_tail.as<unsigned char>(), d_adj[0].as<u64>());
    else
        hipLaunchKernelGGL(k_compat<false>, dim3(grid), dim3(256), lds, s, n_tiles, d_tiles.as<int4>(), d_tints.as<TintDesc>(),
                           d_bits.as<unsigned>(), d_first.as<int>(), d_last.as<int>(), d_tail.as<unsigned char>(), d_adj[0].as<u64>());
    HIP_TRY(c, hipEventRecord(c->ev[1], s));
    int cur = 0;
    if (prune && !small_tints.empty()) {
        // (the final matrix of such a tint goes into BOTH copies: whichever the per-pass kernels of the large tints end on holds it)
        HIP_TRY(c, hipMemcpyAsync(c->small_tints.p, small_tints.data(), small_tints.size() * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_prune_lds, dim3((unsigned)small_tints.size()), dim3(256), small_lds, s, c->small_tints.as<int>(), d_tints.as<TintDesc>(),
                           d_adj[0].as<u64>(), d_adj[1].as<u64>(), c->small_rounds.as<int>());
    }
    if (prune && any_large) {
        // Passes are enqueued kBurst at a time; pass q of a burst is gated on pass q-1's "removed something" word, so the host
        // reads the flags once per burst instead of once per pass (the loop of :240-255 usually ends after two or three).
        const int deg_grid = (int)((R + 3) / 4 < 4096 ? (R + 3) / 4 : 4096);
        // the pass edge by edge (k_prune_edges) when every tint of the per-pass kernels has rows of at most kEdgeChunks x 64 words;
        // FCLU_PRUNE_EDGES=0: the OR-of-rows form whatever the shapes (tests)
        const char *edge_env = getenv("FCLU_PRUNE_EDGES");
        const bool edge_walk = max_aw_large <= kEdgeChunks * 64 && !(edge_env && edge_env[0] == '0');
        const int edge_chunks = (max_aw_large + 63) / 64 > 0 ? (max_aw_large + 63) / 64 : 1;
        const int n_words = st.n_words;
        int *h_any = c->h_flags, *h_changed = c->h_flags + kBurst;
        bool done = false;
        for (int burst = 0; burst < (1 << 18) && !done; ++burst) {
            HIP_TRY(c, hipMemsetAsync(d_changed.p, 0, (size_t)kBurst * T * 4, s));
            HIP_TRY(c, hipMemsetAsync(d_pass_any.p, 0, (size_t)kBurst * 4, s));
            for (int q = 0; q < kBurst; ++q) {
                const int *gate = q ? d_pass_any.as<int>() + (q - 1) : nullptr;
                const int from = cur ^ (q & 1), to = from ^ 1;
                hipLaunchKernelGGL(k_degree, dim3(deg_grid), dim3(256), 0, s, R, d_row_tint.as<int>(), d_tints.as<TintDesc>(),
                                   d_adj[from].as<u64>(), d_deg.as<int>(), gate);
                if (edge_walk)
                    hipLaunchKernelGGL(k_prune_edges, dim3((int)((R * edge_chunks + 3) / 4 < 65536 ? (R * edge_chunks + 3) / 4 : 65536)), dim3(256), 0, s, R, edge_chunks,
                                       d_row_tint.as<int>(), d_tints.as<TintDesc>(), d_adj[from].as<u64>(), d_deg.as<int>(), d_adj[to].as<u64>(),
                                       d_changed.as<int>() + (size_t)q * T, d_pass_any.as<int>() + q, gate);
                else {
                hipLaunchKernelGGL(k_deg1, dim3((n_words + 3) / 4 < 4096 ? (n_words + 3) / 4 : 4096), dim3(256), 0, s, n_words,
                                   d_word_tint.as<int2>(), d_tints.as<TintDesc>(), d_deg.as<int>(), d_deg1.as<u64>(), gate);
                hipLaunchKernelGGL(k_prune, dim3((int)((R + 3) / 4 < 16384 ? (R + 3) / 4 : 16384)), dim3(256), 0, s, R, d_row_tint.as<int>(),
                                   d_tints.as<TintDesc>(), d_tint_word0.as<i64>(), d_adj[from].as<u64>(), d_deg.as<int>(),
                                   d_deg1.as<u64>(), d_adj[to].as<u64>(), d_changed.as<int>() + (size_t)q * T, d_pass_any.as<int>() + q, gate);
                }
            }
            HIP_TRY(c, hipMemcpyAsync(h_any, d_pass_any.p, (size_t)kBurst * 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipMemcpyAsync(h_changed, d_changed.p, (size_t)kBurst * T * 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipStreamSynchronize(s));
            // the passes that ran: 0 .. first pass that removed nothing (inclusive); each of them wrote the other buffer
            int ran = 0;
            for (int q = 0; q < kBurst; ++q) { ++ran; if (!h_any[q]) { done = true; break; } }
            for (int q = 0; q < ran; ++q)
                if (rounds_out) for (int t = 0; t < T; ++t) if (h_changed[(size_t)q * T + t]) rounds_out[t] += 1;
            cur ^= ran & 1;
        }
    }
    HIP_TRY(c, hipEventRecord(c->ev[2], s));
    c->adj_cur = cur;
    if (adj_out) HIP_TRY(c, hipMemcpyAsync(adj_out, d_adj[cur].p, (size_t)n_adj * 8, hipMemcpyDeviceToHost, s));
    std::vector<int> small_rounds;
    if (prune && rounds_out && !small_tints.empty()) {
        small_rounds.resize((size_t)T);
        HIP_TRY(c, hipMemcpyAsync(small_rounds.data(), c->small_rounds.p, (size_t)T * 4, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    if (!small_rounds.empty()) for (int t : small_tints) rounds_out[t] = small_rounds[(size_t)t];
    HIP_TRY(c, hipGetLastError());
    (void)hipEventElapsedTime(&c->compat_ms, c->ev[0], c->ev[1]);
    (void)hipEventElapsedTime(&c->prune_ms, c->ev[1], c->ev[2]);
    return FCLU_OK;
}

// The graph of a batch of the caller's rows: staging with every check, the rows' upload, the kernels.
int compat_device(fclu_ctx *c, const fclu_batch *b, int32_t prune, uint64_t *adj_out, int32_t *rounds_out) {
    if (b->n_tint <= 0) return fail(c, FCLU_ERR_ARG, "fclu_compat_graph: empty batch");
    Staged st;
    const int rc = stage_tints(c, b->n_tint, b->row_off, b->n_seg, b->bits_off, b->adj_off, prune, b, st);
    if (rc != FCLU_OK) return rc;
    if (rounds_out) for (int t = 0; t < st.T; ++t) rounds_out[t] = 0;
    if (st.empty) return FCLU_OK;
    hipStream_t s = c->stream;
    HIP_TRY(c, hipMemcpyAsync(c->bits.p, b->bits, (size_t)st.n_bits * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->first.p, b->first, (size_t)st.R * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->last.p, b->last, (size_t)st.R * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->tail.p, b->tail, (size_t)st.R, hipMemcpyHostToDevice, s));
    return compat_run(c, st, prune, adj_out, rounds_out);
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

hipError_t grow_host(HostBuf &b, size_t bytes) {
    if (b.p && bytes <= b.cap) return hipSuccess;
    if (b.p) { hipError_t e = hipHostFree(b.p); b.p = nullptr; b.cap = 0; if (e != hipSuccess) return e; }
    const size_t want = (bytes ? bytes : 16) + bytes / 4;
    hipError_t e = hipHostMalloc(&b.p, want, hipHostMallocDefault);
    if (e == hipSuccess) b.cap = want;
    return e;
}

int bits_for(i64 n) { int b = 1; while (b < 32 && (1ll << b) < n) ++b; return b; }

// c->tints / c->h_tints / c->row_tint describe the batch and c->adj[c->adj_cur] holds its pruned matrices.  mem_off null: the members
// are on the device already (c->mem_off, c->mem: n_mem_device rep ids), where the dedupe left them.
int partition_device(fclu_ctx *c, int T, i64 R, const int64_t *mem_off, const int32_t *mem, i64 n_mem_device, int32_t maximum_ilp_size) {
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    c->components_ms = c->pairs_ms = 0.f;
    fclu_parts &out = c->parts;
    HIP_TRY(c, grow_host(c->h_tint_part_off, (size_t)(T + 1) * 8));
    if (R == 0) {                                            // nothing but empty tints
        HIP_TRY(c, grow_host(c->h_part_node_off, 8)); HIP_TRY(c, grow_host(c->h_part_rid_off, 8)); HIP_TRY(c, grow_host(c->h_part_pair_off, 8));
        HIP_TRY(c, grow_host(c->h_part_nodes, 0)); HIP_TRY(c, grow_host(c->h_part_rids, 0)); HIP_TRY(c, grow_host(c->h_pairs, 0)); HIP_TRY(c, grow_host(c->h_label, 0));
        memset(c->h_tint_part_off.p, 0, (size_t)(T + 1) * 8);
        *c->h_part_node_off.as<i64>() = *c->h_part_rid_off.as<i64>() = *c->h_part_pair_off.as<i64>() = 0;
        out.n_tint = T; out.n_rows = out.n_part = out.n_rids = out.n_pairs = 0;
    } else {
        const u64 *d_adj = c->adj[c->adj_cur].as<u64>();
        const TintDesc *d_tints = c->tints.as<TintDesc>();
        const int *d_row_tint = c->row_tint.as<int>();
        const i64 n_mem = mem_off ? mem_off[R] : n_mem_device;
        std::vector<int> small;
        size_t small_lds = 0;
        bool any_large = false;
        for (int t = 0; t < T; ++t) {
            const TintDesc &d = c->h_tints[(size_t)t];
            if (d.cc_lds) { small.push_back(t); small_lds = std::max(small_lds, (size_t)d.n * d.aw * 8 + (size_t)d.n * 4); }
            else if (d.n > 0) any_large = true;
        }
        const size_t R1 = (size_t)R + 1;
        HIP_TRY(c, grow(c->parent, (size_t)R * 4)); HIP_TRY(c, grow(c->skey, (size_t)R * 4));
        HIP_TRY(c, grow(c->rows, (size_t)R * 4)); HIP_TRY(c, grow(c->sval, (size_t)R * 4));
        HIP_TRY(c, grow(c->comp_start, (size_t)R * 4)); HIP_TRY(c, grow(c->comp_end, (size_t)R * 4)); HIP_TRY(c, grow(c->chunk_end, (size_t)R * 4));
        HIP_TRY(c, grow(c->head, R1 * 8)); HIP_TRY(c, grow(c->part_id, R1 * 8)); HIP_TRY(c, grow(c->smult, R1 * 8)); HIP_TRY(c, grow(c->rid_pos, R1 * 8));
        HIP_TRY(c, grow(c->cnt, R1 * 8)); HIP_TRY(c, grow(c->pair_base, R1 * 8));
        HIP_TRY(c, grow(c->d_label, (size_t)R * 4)); HIP_TRY(c, grow(c->d_nodes, (size_t)R * 4));
        HIP_TRY(c, grow(c->d_tint_part_off, (size_t)(T + 1) * 8)); HIP_TRY(c, grow(c->d_part_node_off, R1 * 8));
        HIP_TRY(c, grow(c->d_part_rid_off, R1 * 8)); HIP_TRY(c, grow(c->d_part_pair_off, R1 * 8));
        HIP_TRY(c, grow(c->mem_off, R1 * 8)); HIP_TRY(c, grow(c->mem, (size_t)n_mem * 4)); HIP_TRY(c, grow(c->d_part_rids, (size_t)n_mem * 4));
        HIP_TRY(c, grow(c->small_tints, small.size() * 4 + 4));
        HIP_TRY(c, grow(c->pass_any, (size_t)kBurst * 4));
        HIP_TRY(c, grow_host(c->h_cc_flags, (size_t)kBurst * 4 + 16));
        const int end_bit = bits_for(R);
        size_t sort_bytes = 0, scan_bytes = 0;
        HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, sort_bytes, c->parent.as<unsigned>(), c->skey.as<unsigned>(), c->rows.as<int>(), c->sval.as<int>(),
                                             (size_t)R, 0u, (unsigned)end_bit, s));
        HIP_TRY(c, rocprim::exclusive_scan(nullptr, scan_bytes, c->head.as<i64>(), c->part_id.as<i64>(), (i64)0, R1, rocprim::plus<i64>(), s));
        const size_t tmp_bytes = std::max(sort_bytes, scan_bytes);
        HIP_TRY(c, grow(c->tmp, tmp_bytes));
        if (mem_off) {
            HIP_TRY(c, hipMemcpyAsync(c->mem_off.p, mem_off, R1 * 8, hipMemcpyHostToDevice, s));
            if (n_mem) HIP_TRY(c, hipMemcpyAsync(c->mem.p, mem, (size_t)n_mem * 4, hipMemcpyHostToDevice, s));
        }
        if (!small.empty()) HIP_TRY(c, hipMemcpyAsync(c->small_tints.p, small.data(), small.size() * 4, hipMemcpyHostToDevice, s));

        const int row_grid = (int)std::min<i64>((R + 256) / 256, 4096), wave_grid = (int)std::min<i64>((R + 3) / 4, 65536);
        int *d_parent = c->parent.as<int>();
        // ---- components
        HIP_TRY(c, hipEventRecord(c->pev[0], s));
        hipLaunchKernelGGL(k_cc_init, dim3(row_grid), dim3(256), 0, s, R, d_parent);
        hipLaunchKernelGGL(k_cc_init, dim3(row_grid), dim3(256), 0, s, R, c->rows.as<int>());     // (the sort's values: the rows themselves)
        if (!small.empty())
            hipLaunchKernelGGL(k_cc_lds, dim3((unsigned)small.size()), dim3(256), small_lds, s, c->small_tints.as<int>(), d_tints, d_adj, d_parent);
        if (any_large) {
            // as in the pruning: kBurst passes per host round trip, pass q gated on pass q - 1's "something changed" word
            int *h_any = c->h_cc_flags.as<int>(), *d_any = c->pass_any.as<int>();
            bool done = false;
            for (int burst = 0; !done; ++burst) {
                if (burst >= (1 << 16)) return fail(c, FCLU_ERR_HIP, "connected components did not converge");
                HIP_TRY(c, hipMemsetAsync(d_any, 0, (size_t)kBurst * 4, s));
                for (int q = 0; q < kBurst; ++q) {
                    const int *gate = q ? d_any + (q - 1) : nullptr;
                    hipLaunchKernelGGL(k_cc_hook, dim3(wave_grid), dim3(256), 0, s, R, d_row_tint, d_tints, d_adj, d_parent, d_any + q, gate);
                    hipLaunchKernelGGL(k_cc_jump, dim3(row_grid), dim3(256), 0, s, R, d_row_tint, d_tints, d_parent, d_any + q, gate);
                }
                HIP_TRY(c, hipMemcpyAsync(h_any, d_any, (size_t)kBurst * 4, hipMemcpyDeviceToHost, s));
                HIP_TRY(c, hipStreamSynchronize(s));
                for (int q = 0; q < kBurst; ++q) if (!h_any[q]) { done = true; break; }
            }
        }
        HIP_TRY(c, hipEventRecord(c->pev[1], s));
        // ---- even split, members' positions, pair counts
        HIP_TRY(c, rocprim::radix_sort_pairs(c->tmp.p, sort_bytes, c->parent.as<unsigned>(), c->skey.as<unsigned>(), c->rows.as<int>(), c->sval.as<int>(),
                                             (size_t)R, 0u, (unsigned)end_bit, s));
        hipLaunchKernelGGL(k_bounds, dim3(row_grid), dim3(256), 0, s, R, c->skey.as<unsigned>(), c->comp_start.as<int>(), c->comp_end.as<int>());
        hipLaunchKernelGGL(k_chunk, dim3(row_grid), dim3(256), 0, s, R, (i64)maximum_ilp_size, c->skey.as<unsigned>(), c->sval.as<int>(), c->comp_start.as<int>(),
                           c->comp_end.as<int>(), c->mem_off.as<i64>(), d_row_tint, d_tints, d_parent, c->head.as<i64>(), c->chunk_end.as<int>(),
                           c->smult.as<i64>(), c->d_label.as<int>(), c->d_nodes.as<int>());
        size_t sb = scan_bytes;
        HIP_TRY(c, rocprim::exclusive_scan(c->tmp.p, sb, c->head.as<i64>(), c->part_id.as<i64>(), (i64)0, R1, rocprim::plus<i64>(), s));
        sb = scan_bytes;
        HIP_TRY(c, rocprim::exclusive_scan(c->tmp.p, sb, c->smult.as<i64>(), c->rid_pos.as<i64>(), (i64)0, R1, rocprim::plus<i64>(), s));
        HIP_TRY(c, hipMemsetAsync(c->cnt.as<i64>() + R, 0, 8, s));
        HIP_TRY(c, hipEventRecord(c->pev[2], s));
        hipLaunchKernelGGL(k_pairs<false>, dim3(wave_grid), dim3(256), 0, s, R, c->sval.as<int>(), c->chunk_end.as<int>(), c->smult.as<i64>(), d_row_tint, d_tints,
                           d_adj, c->cnt.as<i64>(), (const i64 *)nullptr, c->mem_off.as<i64>(), c->mem.as<int>(), (int2 *)nullptr);
        HIP_TRY(c, hipEventRecord(c->pev[3], s));
        sb = scan_bytes;
        HIP_TRY(c, rocprim::exclusive_scan(c->tmp.p, sb, c->cnt.as<i64>(), c->pair_base.as<i64>(), (i64)0, R1, rocprim::plus<i64>(), s));
        const i64 RT = std::max<i64>(R, T);
        hipLaunchKernelGGL(k_offsets, dim3((int)std::min<i64>((RT + 256) / 256, 4096)), dim3(256), 0, s, R, T, d_tints, c->head.as<i64>(), c->part_id.as<i64>(),
                           c->rid_pos.as<i64>(), c->pair_base.as<i64>(), c->d_tint_part_off.as<i64>(), c->d_part_node_off.as<i64>(),
                           c->d_part_rid_off.as<i64>(), c->d_part_pair_off.as<i64>());
        i64 *h_tot = reinterpret_cast<i64 *>(c->h_cc_flags.as<int>() + kBurst);            // {partitions, pairs}
        HIP_TRY(c, hipMemcpyAsync(h_tot, c->part_id.as<i64>() + R, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h_tot + 1, c->pair_base.as<i64>() + R, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        HIP_TRY(c, hipGetLastError());
        const i64 P = h_tot[0], n_pairs = h_tot[1];
        if (P < 0 || P > R || n_pairs < 0) return fail(c, FCLU_ERR_HIP, "partition totals out of range (%lld partitions, %lld pairs)", P, n_pairs);
        // ---- the pair list: as large as the graphs make it
        if (n_pairs > 2147483647ll)
            return fail(c, FCLU_ERR_UNSUPPORTED, "%lld incompatible pairs in this batch: more than the 2147483647 a call returns", n_pairs);
        if ((size_t)n_pairs * 8 > c->d_pairs.cap) {
            if (c->d_pairs.p) { HIP_TRY(c, hipFree(c->d_pairs.p)); c->d_pairs.p = nullptr; c->d_pairs.cap = 0; }
            size_t free_b = 0, total_b = 0;
            HIP_TRY(c, hipMemGetInfo(&free_b, &total_b));
            if ((size_t)n_pairs * 8 + (64u << 20) > free_b)
                return fail(c, FCLU_ERR_UNSUPPORTED, "%lld incompatible pairs in this batch (%lld bytes) do not fit the device's free memory (%lld bytes)",
                            n_pairs, n_pairs * 8, (i64)free_b);
            if (hipMalloc(&c->d_pairs.p, (size_t)n_pairs * 8) != hipSuccess) {
                (void)hipGetLastError(); c->d_pairs.p = nullptr;
                return fail(c, FCLU_ERR_UNSUPPORTED, "%lld incompatible pairs in this batch: no device memory for %lld bytes", n_pairs, n_pairs * 8);
            }
            c->d_pairs.cap = (size_t)n_pairs * 8;
        }
        if ((size_t)n_pairs * 8 > c->h_pairs.cap || !c->h_pairs.p) {
            if (c->h_pairs.p) { HIP_TRY(c, hipHostFree(c->h_pairs.p)); c->h_pairs.p = nullptr; c->h_pairs.cap = 0; }
            const size_t want = std::max<size_t>((size_t)n_pairs * 8, 16);
            if (hipHostMalloc(&c->h_pairs.p, want, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError(); c->h_pairs.p = nullptr;
                return fail(c, FCLU_ERR_UNSUPPORTED, "%lld incompatible pairs in this batch: no pinned host memory for %lld bytes", n_pairs, n_pairs * 8);
            }
            c->h_pairs.cap = want;
        }
        HIP_TRY(c, grow_host(c->h_part_node_off, (size_t)(P + 1) * 8)); HIP_TRY(c, grow_host(c->h_part_rid_off, (size_t)(P + 1) * 8));
        HIP_TRY(c, grow_host(c->h_part_pair_off, (size_t)(P + 1) * 8));
        HIP_TRY(c, grow_host(c->h_part_nodes, (size_t)R * 4)); HIP_TRY(c, grow_host(c->h_label, (size_t)R * 4)); HIP_TRY(c, grow_host(c->h_part_rids, (size_t)n_mem * 4));
        HIP_TRY(c, hipEventRecord(c->pev[4], s));
        if (n_pairs)
            hipLaunchKernelGGL(k_pairs<true>, dim3(wave_grid), dim3(256), 0, s, R, c->sval.as<int>(), c->chunk_end.as<int>(), c->smult.as<i64>(), d_row_tint, d_tints,
                               d_adj, (i64 *)nullptr, c->pair_base.as<i64>(), c->mem_off.as<i64>(), c->mem.as<int>(), c->d_pairs.as<int2>());
        if (n_mem)
            hipLaunchKernelGGL(k_members, dim3(wave_grid), dim3(256), 0, s, R, c->sval.as<int>(), c->smult.as<i64>(), c->rid_pos.as<i64>(), c->mem_off.as<i64>(),
                               c->mem.as<int>(), c->d_part_rids.as<int>());
        HIP_TRY(c, hipEventRecord(c->pev[5], s));
        HIP_TRY(c, hipMemcpyAsync(c->h_tint_part_off.p, c->d_tint_part_off.p, (size_t)(T + 1) * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(c->h_part_node_off.p, c->d_part_node_off.p, (size_t)(P + 1) * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(c->h_part_rid_off.p, c->d_part_rid_off.p, (size_t)(P + 1) * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(c->h_part_pair_off.p, c->d_part_pair_off.p, (size_t)(P + 1) * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(c->h_part_nodes.p, c->d_nodes.p, (size_t)R * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(c->h_label.p, c->d_label.p, (size_t)R * 4, hipMemcpyDeviceToHost, s));
        if (n_mem) HIP_TRY(c, hipMemcpyAsync(c->h_part_rids.p, c->d_part_rids.p, (size_t)n_mem * 4, hipMemcpyDeviceToHost, s));
        if (n_pairs) HIP_TRY(c, hipMemcpyAsync(c->h_pairs.p, c->d_pairs.p, (size_t)n_pairs * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        HIP_TRY(c, hipGetLastError());
        float a = 0.f, b = 0.f;
        (void)hipEventElapsedTime(&c->components_ms, c->pev[0], c->pev[1]);
        (void)hipEventElapsedTime(&a, c->pev[2], c->pev[3]);
        (void)hipEventElapsedTime(&b, c->pev[4], c->pev[5]);
        c->pairs_ms = a + b;
        out.n_tint = T; out.n_rows = R; out.n_part = P; out.n_rids = n_mem; out.n_pairs = n_pairs;
    }
    out.tint_part_off = c->h_tint_part_off.as<int64_t>();
    out.part_node_off = c->h_part_node_off.as<int64_t>(); out.part_nodes = c->h_part_nodes.as<int32_t>();
    out.part_rid_off = c->h_part_rid_off.as<int64_t>(); out.part_rids = c->h_part_rids.as<int32_t>();
    out.part_pair_off = c->h_part_pair_off.as<int64_t>(); out.pairs = c->h_pairs.as<int32_t>();
    out.label = c->h_label.as<int32_t>();
    c->have_parts = true;
    return FCLU_OK;
}


// ---- preprocess_ilp() + the dedupe of a batch of label rows ----------------------------------------------------------
enum { P_TINTS, P_LABELS, P_TAIL, P_IBITS, P_CBITS, P_RFIRST, P_RLAST, P_FIRST, P_LAST, P_REP_TINT, P_KEY, P_SKEY, P_VAL, P_SVAL, P_HEAD,
       P_BSTART, P_LEADER, P_FLAG, P_NODE_ID, P_ROW_OFF, P_REP_NODE, P_NODE_REP, P_NKEY, P_SNKEY, P_NVAL, P_ERR, P_TMP };
enum { Q_ROW_OFF, Q_BITS_OFF, Q_ADJ_OFF, Q_RBITS_OFF, Q_IBITS, Q_CBITS, Q_FIRST, Q_LAST, Q_RFIRST, Q_RLAST, Q_REP_NODE, Q_NODE_REP, Q_MEM_OFF,
       Q_MEM, Q_BITS, Q_NFIRST, Q_NLAST, Q_NTAIL, Q_ERR };

// Rows, dedupe and the staging of the unique rows as a batch: behind it c->bits / first / last / tail hold the nodes in fclu_batch's
// layout, c->mem_off / c->mem their members, st what compat_run() needs, and the pinned copies of everything are on their way (the
// caller synchronises).  Between the two halves only row_off (n_tint + 1 counts) and the three error words come back to the host.
int preprocess_device(fclu_ctx *c, const fclu_reads *rd, int32_t prune, Staged &st, i64 &n_reps_out) {
    c->have_prep = false;
    c->rows_ms = c->dedupe_ms = 0.f;
    if (!rd || rd->n_tint <= 0) return fail(c, FCLU_ERR_ARG, "fclu_preprocess: empty batch");
    if (!rd->rep_off || !rd->n_seg || !rd->lab_off) return fail(c, FCLU_ERR_ARG, "fclu_preprocess: rep_off, n_seg or lab_off is null");
    HIP_TRY(c, hipSetDevice(c->device));
    const int T = rd->n_tint;
    if (rd->rep_off[0] != 0 || rd->lab_off[0] != 0) return fail(c, FCLU_ERR_ARG, "fclu_preprocess: rep_off and lab_off start at 0");
    std::vector<PrepTint> pt((size_t)T);
    std::vector<int64_t> rbits_off((size_t)T + 1, 0);
    i64 n_slots = 0;
    for (int t = 0; t < T; ++t) {
        PrepTint &d = pt[(size_t)t];
        const i64 n = rd->rep_off[t + 1] - rd->rep_off[t];
        if (n < 0 || n > (1 << 30) || rd->n_seg[t] < 0)
            return fail(c, FCLU_ERR_ARG, "tint %d: negative or too large rep count (%lld) or segment count (%d)", t, n, (int)rd->n_seg[t]);
        if (rd->n_seg[t] > kMaxWords * 32)
            return fail(c, FCLU_ERR_UNSUPPORTED, "tint %d has %d segments; this build stages at most %d", t, (int)rd->n_seg[t], kMaxWords * 32);
        d.rep0 = rd->rep_off[t]; d.lab_off = rd->lab_off[t]; d.rbits_off = rbits_off[(size_t)t]; d.slot0 = n_slots;
        d.n = (int)n; d.n_seg = rd->n_seg[t];
        d.lw = std::max((d.n_seg + 15) / 16, 1); d.w = std::max((d.n_seg + 31) / 32, 1);
        d.g_log2 = 0; while (d.g_log2 < 6 && (1 << d.g_log2) < d.w) ++d.g_log2;
        if (rd->lab_off[t + 1] - d.lab_off != n * d.lw)
            return fail(c, FCLU_ERR_ARG, "tint %d: lab_off does not match reps x words (%lld words for %lld reps of %d)", t,
                        (i64)(rd->lab_off[t + 1] - d.lab_off), n, d.lw);
        rbits_off[(size_t)t + 1] = d.rbits_off + n * d.w;
        n_slots += ((n << d.g_log2) + 63) / 64 * 64;
    }
    const i64 N = rd->rep_off[T], n_lab = rd->lab_off[T], n_rbits = rbits_off[(size_t)T];
    if (N >= 0x7f7f7f7fll) return fail(c, FCLU_ERR_ARG, "fclu_preprocess: %lld reps in one batch", N);
    if (N > 0 && (!rd->labels || !rd->tail)) return fail(c, FCLU_ERR_ARG, "fclu_preprocess: labels or tail is null");
    n_reps_out = N;
    const char *hb_env = getenv("FCLU_HASH_BITS");           // (tests: a hash cut to n bits forces collisions; 0: one bucket a tint)
    unsigned hash_mask = 0xffffffffu;
    if (hb_env && hb_env[0] >= '0' && hb_env[0] <= '9' && atoi(hb_env) < 32) hash_mask = (1u << atoi(hb_env)) - 1u;

    GrowBuf *D = c->pd;
    HostBuf *H = c->ph;
    hipStream_t s = c->stream;
    const size_t N1 = (size_t)N + 1;
    HIP_TRY(c, grow_host(H[Q_ROW_OFF], (size_t)(T + 1) * 8)); HIP_TRY(c, grow_host(H[Q_BITS_OFF], (size_t)(T + 1) * 8));
    HIP_TRY(c, grow_host(H[Q_ADJ_OFF], (size_t)(T + 1) * 8)); HIP_TRY(c, grow_host(H[Q_RBITS_OFF], (size_t)(T + 1) * 8));
    HIP_TRY(c, grow_host(H[Q_ERR], 16));
    HIP_TRY(c, grow_host(H[Q_IBITS], (size_t)n_rbits * 4)); HIP_TRY(c, grow_host(H[Q_CBITS], (size_t)n_rbits * 4));
    for (int q : {Q_FIRST, Q_LAST, Q_RFIRST, Q_RLAST, Q_REP_NODE, Q_MEM}) HIP_TRY(c, grow_host(H[q], (size_t)N * 4));
    memcpy(H[Q_RBITS_OFF].p, rbits_off.data(), (size_t)(T + 1) * 8);
    i64 *h_row_off = H[Q_ROW_OFF].as<i64>(), *h_bits_off = H[Q_BITS_OFF].as<i64>(), *h_adj_off = H[Q_ADJ_OFF].as<i64>();
    int *h_err = H[Q_ERR].as<int>();
    if (N > 0) {
        HIP_TRY(c, grow(D[P_TINTS], pt.size() * sizeof(PrepTint)));
        HIP_TRY(c, grow(D[P_LABELS], (size_t)n_lab * 4)); HIP_TRY(c, grow(D[P_TAIL], (size_t)N));
        HIP_TRY(c, grow(D[P_IBITS], (size_t)n_rbits * 4)); HIP_TRY(c, grow(D[P_CBITS], (size_t)n_rbits * 4));
        for (int q : {P_RFIRST, P_RLAST, P_FIRST, P_LAST, P_REP_TINT, P_VAL, P_SVAL, P_HEAD, P_BSTART, P_LEADER, P_REP_NODE, P_NODE_REP, P_NKEY, P_SNKEY, P_NVAL})
            HIP_TRY(c, grow(D[q], (size_t)N * 4));
        HIP_TRY(c, grow(D[P_FLAG], N1 * 4)); HIP_TRY(c, grow(D[P_NODE_ID], N1 * 4));
        HIP_TRY(c, grow(D[P_KEY], (size_t)N * 8)); HIP_TRY(c, grow(D[P_SKEY], (size_t)N * 8));
        HIP_TRY(c, grow(D[P_ROW_OFF], (size_t)(T + 1) * 8)); HIP_TRY(c, grow(D[P_ERR], 16));
        HIP_TRY(c, grow(c->mem, (size_t)N * 4));
        const unsigned key_bits = 32u + (unsigned)bits_for(T), node_bits = (unsigned)bits_for(N);
        size_t sort_a = 0, sort_b = 0, scan_a = 0, scan_b = 0;
        HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, sort_a, D[P_KEY].as<u64>(), D[P_SKEY].as<u64>(), D[P_VAL].as<int>(), D[P_SVAL].as<int>(), (size_t)N, 0u, key_bits, s));
        HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, sort_b, D[P_NKEY].as<unsigned>(), D[P_SNKEY].as<unsigned>(), D[P_NVAL].as<int>(), c->mem.as<int>(), (size_t)N, 0u, node_bits, s));
        HIP_TRY(c, rocprim::inclusive_scan(nullptr, scan_a, D[P_HEAD].as<int>(), D[P_BSTART].as<int>(), (size_t)N, rocprim::maximum<int>(), s));
        HIP_TRY(c, rocprim::exclusive_scan(nullptr, scan_b, D[P_FLAG].as<int>(), D[P_NODE_ID].as<int>(), 0, N1, rocprim::plus<int>(), s));
        const size_t tmp_bytes = std::max(std::max(sort_a, sort_b), std::max(scan_a, scan_b));
        HIP_TRY(c, grow(D[P_TMP], tmp_bytes));
        HIP_TRY(c, hipMemcpyAsync(D[P_TINTS].p, pt.data(), pt.size() * sizeof(PrepTint), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(D[P_LABELS].p, rd->labels, (size_t)n_lab * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(D[P_TAIL].p, rd->tail, (size_t)N, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemsetAsync(D[P_ERR].p, 0x7f, 16, s));
        HIP_TRY(c, hipMemsetAsync(D[P_FLAG].as<int>() + N, 0, 4, s));
        const int rep_grid = (int)std::min<i64>((N + 255) / 256, 4096);
        const PrepTint *d_pt = D[P_TINTS].as<PrepTint>();
        HIP_TRY(c, hipEventRecord(c->qev[0], s));
        hipLaunchKernelGGL(k_rows, dim3((unsigned)std::min<i64>((n_slots + 255) / 256, 65536)), dim3(256), 0, s, T, n_slots, d_pt, D[P_LABELS].as<unsigned>(),
                           D[P_TAIL].as<unsigned char>(), hash_mask, D[P_IBITS].as<unsigned>(), D[P_CBITS].as<unsigned>(), D[P_RFIRST].as<int>(),
                           D[P_RLAST].as<int>(), D[P_FIRST].as<int>(), D[P_LAST].as<int>(), D[P_REP_TINT].as<int>(), D[P_KEY].as<u64>(), D[P_VAL].as<int>(),
                           D[P_ERR].as<int>());
        HIP_TRY(c, hipEventRecord(c->qev[1], s));
        // refusals first: a tail above 2 or a label 3 has no meaning, and the sort's keys of such a batch are not needed
        HIP_TRY(c, hipMemcpyAsync(h_err, D[P_ERR].p, 16, hipMemcpyDeviceToHost, s));
        size_t tb = tmp_bytes;
        HIP_TRY(c, rocprim::radix_sort_pairs(D[P_TMP].p, tb, D[P_KEY].as<u64>(), D[P_SKEY].as<u64>(), D[P_VAL].as<int>(), D[P_SVAL].as<int>(), (size_t)N, 0u, key_bits, s));
        hipLaunchKernelGGL(k_heads, dim3(rep_grid), dim3(256), 0, s, N, D[P_SKEY].as<u64>(), D[P_HEAD].as<int>());
        tb = tmp_bytes;
        HIP_TRY(c, rocprim::inclusive_scan(D[P_TMP].p, tb, D[P_HEAD].as<int>(), D[P_BSTART].as<int>(), (size_t)N, rocprim::maximum<int>(), s));
        hipLaunchKernelGGL(k_leader, dim3(rep_grid), dim3(256), 0, s, N, D[P_SKEY].as<u64>(), D[P_SVAL].as<int>(), D[P_BSTART].as<int>(), d_pt,
                           D[P_IBITS].as<unsigned>(), D[P_FIRST].as<int>(), D[P_LAST].as<int>(), D[P_TAIL].as<unsigned char>(), D[P_LEADER].as<int>(),
                           D[P_FLAG].as<int>());
        tb = tmp_bytes;
        HIP_TRY(c, rocprim::exclusive_scan(D[P_TMP].p, tb, D[P_FLAG].as<int>(), D[P_NODE_ID].as<int>(), 0, N1, rocprim::plus<int>(), s));
        hipLaunchKernelGGL(k_row_off, dim3((unsigned)(T + 256) / 256), dim3(256), 0, s, T, N, d_pt, D[P_NODE_ID].as<int>(), D[P_ROW_OFF].as<i64>());
        HIP_TRY(c, hipEventRecord(c->qev[2], s));
        HIP_TRY(c, hipMemcpyAsync(h_row_off, D[P_ROW_OFF].p, (size_t)(T + 1) * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        HIP_TRY(c, hipGetLastError());
        const int kinds[3] = {2, 0, 1};                      // the tail first: it is the caller's own byte, the labels come from a file
        for (int k : kinds) {
            if (h_err[k] == 0x7f7f7f7f) continue;
            const i64 rep = h_err[k];
            int t = 0;
            while (t + 1 < T && rd->rep_off[t + 1] <= rep) ++t;
            const i64 r = rep - rd->rep_off[t];
            if (k == 2) return fail(c, FCLU_ERR_ARG, "tint %d rep %lld: tail category %d (0 'N', 1 'S', 2 'E')", t, r, (int)rd->tail[rep]);
            if (k == 0) return fail(c, FCLU_ERR_ARG, "tint %d rep %lld: a label with code 3 (labels are 0, 1, 2)", t, r);
            return fail(c, FCLU_ERR_ARG, "tint %d rep %lld: a nonzero bit beyond the tint's %d labels", t, r, (int)rd->n_seg[t]);
        }
    } else {
        memset(h_row_off, 0, (size_t)(T + 1) * 8);
    }
    // ---- the unique rows as a batch
    h_bits_off[0] = h_adj_off[0] = 0;
    for (int t = 0; t < T; ++t) {
        const i64 n = h_row_off[t + 1] - h_row_off[t];
        if (n < 0 || n > rd->rep_off[t + 1] - rd->rep_off[t]) return fail(c, FCLU_ERR_HIP, "tint %d: %lld unique rows of %lld reps", t, n, (i64)(rd->rep_off[t + 1] - rd->rep_off[t]));
        h_bits_off[t + 1] = h_bits_off[t] + n * pt[(size_t)t].w;
        h_adj_off[t + 1] = h_adj_off[t] + n * ((n + 63) / 64);
    }
    const i64 R = h_row_off[T], n_bits = h_bits_off[T];
    int rc = stage_tints(c, T, H[Q_ROW_OFF].as<int64_t>(), rd->n_seg, H[Q_BITS_OFF].as<int64_t>(), H[Q_ADJ_OFF].as<int64_t>(), prune, nullptr, st);
    if (rc != FCLU_OK) return rc;
    HIP_TRY(c, grow_host(H[Q_NODE_REP], (size_t)R * 4)); HIP_TRY(c, grow_host(H[Q_MEM_OFF], (size_t)(R + 1) * 8));
    HIP_TRY(c, grow_host(H[Q_BITS], (size_t)n_bits * 4)); HIP_TRY(c, grow_host(H[Q_NFIRST], (size_t)R * 4));
    HIP_TRY(c, grow_host(H[Q_NLAST], (size_t)R * 4)); HIP_TRY(c, grow_host(H[Q_NTAIL], (size_t)R));
    *H[Q_MEM_OFF].as<i64>() = 0;
    if (N > 0) {
        HIP_TRY(c, grow(c->mem_off, (size_t)(R + 1) * 8));
        const int rep_grid = (int)std::min<i64>((N + 256) / 256, 4096);
        HIP_TRY(c, hipEventRecord(c->qev[3], s));
        hipLaunchKernelGGL(k_nodes, dim3(rep_grid), dim3(256), 0, s, N, D[P_REP_TINT].as<int>(), D[P_TINTS].as<PrepTint>(), c->tints.as<TintDesc>(),
                           D[P_LEADER].as<int>(), D[P_NODE_ID].as<int>(), D[P_IBITS].as<unsigned>(), D[P_FIRST].as<int>(), D[P_LAST].as<int>(),
                           D[P_TAIL].as<unsigned char>(), D[P_REP_NODE].as<int>(), D[P_NKEY].as<unsigned>(), D[P_NVAL].as<int>(), D[P_NODE_REP].as<int>(),
                           c->bits.as<unsigned>(), c->first.as<int>(), c->last.as<int>(), c->tail.as<unsigned char>());
        size_t tb = D[P_TMP].cap;
        HIP_TRY(c, rocprim::radix_sort_pairs(D[P_TMP].p, tb, D[P_NKEY].as<unsigned>(), D[P_SNKEY].as<unsigned>(), D[P_NVAL].as<int>(), c->mem.as<int>(), (size_t)N, 0u,
                                             (unsigned)bits_for(N), s));
        hipLaunchKernelGGL(k_mem_off, dim3(rep_grid), dim3(256), 0, s, N, R, D[P_SNKEY].as<unsigned>(), c->mem_off.as<i64>());
        HIP_TRY(c, hipEventRecord(c->qev[4], s));
        HIP_TRY(c, hipMemcpyAsync(H[Q_IBITS].p, D[P_IBITS].p, (size_t)n_rbits * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(H[Q_CBITS].p, D[P_CBITS].p, (size_t)n_rbits * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(H[Q_FIRST].p, D[P_FIRST].p, (size_t)N * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(H[Q_LAST].p, D[P_LAST].p, (size_t)N * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(H[Q_RFIRST].p, D[P_RFIRST].p, (size_t)N * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(H[Q_RLAST].p, D[P_RLAST].p, (size_t)N * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(H[Q_REP_NODE].p, D[P_REP_NODE].p, (size_t)N * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(H[Q_NODE_REP].p, D[P_NODE_REP].p, (size_t)R * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(H[Q_MEM_OFF].p, c->mem_off.p, (size_t)(R + 1) * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(H[Q_MEM].p, c->mem.p, (size_t)N * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(H[Q_BITS].p, c->bits.p, (size_t)n_bits * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(H[Q_NFIRST].p, c->first.p, (size_t)R * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(H[Q_NLAST].p, c->last.p, (size_t)R * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(H[Q_NTAIL].p, c->tail.p, (size_t)R, hipMemcpyDeviceToHost, s));
    }
    fclu_prep &o = c->prep;
    o.n_tint = T; o.n_reps = N; o.n_rows = R;
    o.row_off = H[Q_ROW_OFF].as<int64_t>(); o.bits_off = H[Q_BITS_OFF].as<int64_t>(); o.adj_off = H[Q_ADJ_OFF].as<int64_t>();
    o.rep_bits_off = H[Q_RBITS_OFF].as<int64_t>();
    o.i_bits = H[Q_IBITS].as<uint32_t>(); o.c_bits = H[Q_CBITS].as<uint32_t>();
    o.first = H[Q_FIRST].as<int32_t>(); o.last = H[Q_LAST].as<int32_t>(); o.raw_first = H[Q_RFIRST].as<int32_t>(); o.raw_last = H[Q_RLAST].as<int32_t>();
    o.rep_node = H[Q_REP_NODE].as<int32_t>(); o.node_rep = H[Q_NODE_REP].as<int32_t>();
    o.mem_off = H[Q_MEM_OFF].as<int64_t>(); o.mem = H[Q_MEM].as<int32_t>();
    o.bits = H[Q_BITS].as<uint32_t>(); o.node_first = H[Q_NFIRST].as<int32_t>(); o.node_last = H[Q_NLAST].as<int32_t>(); o.node_tail = H[Q_NTAIL].as<uint8_t>();
    return FCLU_OK;
}

// the kernels' times of the call that has just synchronised
void preprocess_times(fclu_ctx *c, i64 n_reps) {
    if (n_reps <= 0) return;
    float a = 0.f, b = 0.f;
    (void)hipEventElapsedTime(&c->rows_ms, c->qev[0], c->qev[1]);
    (void)hipEventElapsedTime(&a, c->qev[1], c->qev[2]);
    (void)hipEventElapsedTime(&b, c->qev[3], c->qev[4]);
    c->dedupe_ms = a + b;
}

}  // namespace

extern "C" {

int fclu_preprocess(fclu_ctx *c, const fclu_reads *reads) {
    if (!c) return FCLU_ERR_ARG;
    Staged st;
    i64 n_reps = 0;
    const int rc = preprocess_device(c, reads, 1, st, n_reps);
    if (rc != FCLU_OK) return rc;
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
    Staged st;
    i64 n_reps = 0;
    int rc = preprocess_device(c, reads, 1, st, n_reps);
    if (rc != FCLU_OK) return rc;
    if (!st.empty) rc = compat_run(c, st, 1, nullptr, nullptr);          // (it synchronises: the pinned copies have landed)
    else HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (rc != FCLU_OK) return rc;
    preprocess_times(c, n_reps);
    c->have_prep = true;
    return partition_device(c, reads->n_tint, st.R, nullptr, nullptr, n_reps, maximum_ilp_size);
}

int fclu_preprocess_results(fclu_ctx *c, fclu_prep *out) {
    if (!c || !out) return FCLU_ERR_ARG;
    if (!c->have_prep) return fail(c, FCLU_ERR_ARG, "fclu_preprocess_results: no result (the last fclu_preprocess / fclu_partition_reads call failed or none was made)");
    *out = c->prep;
    return FCLU_OK;
}

int fclu_preprocess_timing(fclu_ctx *c, float *rows_ms, float *dedupe_ms) {
    if (!c) return FCLU_ERR_ARG;
    if (rows_ms) *rows_ms = c->rows_ms;
    if (dedupe_ms) *dedupe_ms = c->dedupe_ms;
    return FCLU_OK;
}

int fclu_partition(fclu_ctx *c, const fclu_batch *b, const int64_t *mem_off, const int32_t *mem, int32_t maximum_ilp_size) {
    if (!c || !b) return FCLU_ERR_ARG;
    c->have_parts = false;
    if (b->n_tint <= 0) return fail(c, FCLU_ERR_ARG, "fclu_partition: empty batch");
    int rc = check_members(c, b->row_off[b->n_tint], mem_off, mem, maximum_ilp_size);
    if (rc == FCLU_OK) rc = compat_device(c, b, 1, nullptr, nullptr);
    if (rc == FCLU_OK) rc = partition_device(c, b->n_tint, b->row_off[b->n_tint], mem_off, mem, 0, maximum_ilp_size);
    return rc;
}

int fclu_partition_adj(fclu_ctx *c, int32_t n_tint, const int64_t *row_off, const int64_t *adj_off, const uint64_t *adj,
                       const int64_t *mem_off, const int32_t *mem, int32_t maximum_ilp_size) {
    if (!c || !row_off || !adj_off) return FCLU_ERR_ARG;
    c->have_parts = false;
    if (n_tint <= 0) return fail(c, FCLU_ERR_ARG, "fclu_partition_adj: empty batch");
    HIP_TRY(c, hipSetDevice(c->device));
    const int T = n_tint;
    const i64 R = row_off[T], n_adj = adj_off[T];
    if (row_off[0] != 0 || adj_off[0] != 0 || R < 0 || R >= (1ll << 31)) return fail(c, FCLU_ERR_ARG, "fclu_partition_adj: bad row_off / adj_off");
    if (n_adj > 0 && !adj) return FCLU_ERR_ARG;
    std::vector<TintDesc> tints((size_t)T);
    std::vector<int> row_tint((size_t)R);
    for (int t = 0; t < T; ++t) {
        TintDesc &d = tints[(size_t)t];
        d = TintDesc();
        d.row0 = row_off[t];
        const i64 n = row_off[t + 1] - d.row0;
        if (n < 0 || n > (1 << 30)) return fail(c, FCLU_ERR_ARG, "tint %d: bad row count", t);
        d.n = (int)n; d.aw = (d.n + 63) / 64; d.adj_off = adj_off[t]; d.w = 1;
        d.cc_lds = cc_in_lds(d.n, d.aw);
        if (adj_off[t + 1] - d.adj_off != (i64)d.n * d.aw) return fail(c, FCLU_ERR_ARG, "tint %d: adj_off does not match rows x words", t);
        // the matrix is the caller's: symmetric, an empty diagonal, no bit at a column >= N (the kernels index nodes with its bits)
        const uint64_t *A = adj + d.adj_off;
        for (i64 r = 0; r < n; ++r) {
            row_tint[(size_t)(d.row0 + r)] = t;
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
        }
    }
    int rc = check_members(c, R, mem_off, mem, maximum_ilp_size);
    if (rc != FCLU_OK) return rc;
    c->h_tints = tints;
    c->adj_cur = 0;
    c->compat_ms = c->prune_ms = 0.f;
    if (R > 0) {
        hipStream_t s = c->stream;
        HIP_TRY(c, grow(c->tints, tints.size() * sizeof(TintDesc)));
        HIP_TRY(c, grow(c->row_tint, (size_t)R * 4));
        HIP_TRY(c, grow(c->adj[0], (size_t)n_adj * 8));
        HIP_TRY(c, hipMemcpyAsync(c->tints.p, tints.data(), tints.size() * sizeof(TintDesc), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(c->row_tint.p, row_tint.data(), (size_t)R * 4, hipMemcpyHostToDevice, s));
        if (n_adj) HIP_TRY(c, hipMemcpyAsync(c->adj[0].p, adj, (size_t)n_adj * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipStreamSynchronize(s));              // (the host vectors go out of scope)
    }
    return partition_device(c, T, R, mem_off, mem, 0, maximum_ilp_size);
}

int fclu_partition_results(fclu_ctx *c, fclu_parts *out) {
    if (!c || !out) return FCLU_ERR_ARG;
    if (!c->have_parts) return fail(c, FCLU_ERR_ARG, "fclu_partition_results: no result (the last fclu_partition call failed or none was made)");
    *out = c->parts;
    return FCLU_OK;
}

int fclu_partition_timing(fclu_ctx *c, float *components_ms, float *pairs_ms) {
    if (!c) return FCLU_ERR_ARG;
    if (components_ms) *components_ms = c->components_ms;
    if (pairs_ms) *pairs_ms = c->pairs_ms;
    return FCLU_OK;
}

int fclu_last_timing(fclu_ctx *c, float *compat_ms, float *prune_ms) {
    if (!c) return FCLU_ERR_ARG;
    if (compat_ms) *compat_ms = c->compat_ms;
    if (prune_ms) *prune_ms = c->prune_ms;
    return FCLU_OK;
}

}  // extern "C"

#ifdef FREDDIE_SOURCE_HASH
/* what this binary was built from (freddie_amd/build.py looks for the marker in the file) */
static const char freddie_source_stamp[] __attribute__((used)) = "FREDDIE_SRC_HASH=" FREDDIE_SOURCE_HASH;
#endif
