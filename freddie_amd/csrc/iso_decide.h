// iso_decide.h -- the kernels of fiso_isoforms() (include/freddie_isoforms.h): isoforms_cons() (py/freddie_isoforms.py
// :203-250) and correct_boundaries() (:122-140) with their decisions, from one bit per label.  Included by
// freddie_isoforms.hip inside its anonymous namespace, after its typedefs.  Neither the counts nor the votes reach device
// memory: k_iso_exons keeps cons / cov in registers and LDS and writes exons, k_iso_correct keeps the vote table in LDS and
// writes boundaries.
#ifndef FREDDIE_ISO_DECIDE_H
#define FREDDIE_ISO_DECIDE_H

constexpr int kIsoRowMax = 1024;                 // segments of an isoform: 16 words of bits, 4 segments per thread
constexpr int kIsoWords = kIsoRowMax / 64;
// Tile sizes (fiso_isoforms_limits reports them).  LDS is 160 KiB per CU and these kernels have little else to hide latency
// with than other workgroups, so a workgroup stays near 40 KiB (three to a CU).  A read's row in LDS is W | 1 words long:
// with an odd stride in 8-byte words the 32 lanes of a ds_read_b64 group (bank = (address / 4) mod 64), each on its own
// read's row, fall on 32 different bank pairs.  A vote row is 2w + 1 ints, odd as it is.
constexpr int kIsoReadTile = 256;                // reads: 256 x 17 x 8 = 34 816 bytes
constexpr int kIsoBoundTile = 256;               // isoform boundaries: 256 x 41 x 4 = 41 984 bytes at window 20
constexpr int kIsoWindowMax = 20;                // (:45)

// One workgroup of 256 threads per isoform.  A tile of reads' bit rows goes to LDS in one coalesced pass (an isoform's rows are
// contiguous in `bits`).  Thread q takes read q of the tile: first / last set bit over its W words, +1 / -1 into the coverage
// difference array, its tail counted.  Thread t owns segments t, t + 256, ..: cons[j] = the tile's reads whose bit j is set
// (a '1' always lies inside its read's span); the 64 lanes of a wave test 64 consecutive bits of ONE word per read, so the LDS
// read is a broadcast.  After the last tile: cov = running sum of the differences, flags, exon index = running sum of the
// run starts, and the exons go to the isoform's capacity slots.
__global__ void __launch_bounds__(256) k_iso_exons(int n_iso, const int *__restrict__ iso_tint, const i64 *__restrict__ tint_pos_off,
                                                   const int *__restrict__ pos, const i64 *__restrict__ iso_read_off,
                                                   const i64 *__restrict__ iso_bits_off, const u64 *__restrict__ bits,
                                                   const unsigned char *__restrict__ tail, const i64 *__restrict__ exon_off,
                                                   int *n_exon, int *start, int *end, int *seg_first, int *seg_last,
                                                   unsigned char *strand, int *tails) {
    __shared__ u64 tile_s[kIsoReadTile * (kIsoWords + 1)];
    __shared__ int diff_s[kIsoRowMax + 1], cons_s[kIsoRowMax];
    __shared__ unsigned char flag_s[kIsoRowMax + 2];                      // flag of segment j at j + 1, a zero on either side
    __shared__ int t_s[3], wtot_s[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = blockIdx.x; i < n_iso; i += gridDim.x) {
        const int t = iso_tint[i];
        const i64 p0 = tint_pos_off[t];
        const int M = (int)(tint_pos_off[t + 1] - p0) - 1;                // 0 <= M <= kIsoRowMax: the host refuses anything else
        const int W = (M + 63) >> 6, Ws = W | 1;
        const i64 r0 = iso_read_off[i], r1 = iso_read_off[i + 1];
        const u64 *rows = bits + iso_bits_off[i];
        __syncthreads();                                                  // (the previous isoform is done with LDS)
        for (int j = tid; j <= M; j += 256) diff_s[j] = 0;
        if (tid < 3) t_s[tid] = 0;
        int x[4] = {0, 0, 0, 0};
        for (i64 rb = r0; rb < r1; rb += kIsoReadTile) {
            const int n = (int)(r1 - rb < kIsoReadTile ? r1 - rb : kIsoReadTile);
            __syncthreads();                                              // (the previous tile has been read; the zeroes are in)
            const u64 *src = rows + (rb - r0) * W;
            for (int idx = tid; idx < n * W; idx += 256) { const int q = idx / W; tile_s[q * Ws + (idx - q * W)] = src[idx]; }
            __syncthreads();
            if (tid < n) {
                int first = -1, last = -1;
                for (int k = 0; k < W; ++k) {
                    const u64 w = tile_s[tid * Ws + k];
                    if (w) { if (first < 0) first = 64 * k + __builtin_ctzll(w); last = 64 * k + 63 - __builtin_clzll(w); }
                }
                if (first >= 0) {                                         // a read without a '1' is skipped (:215-216)
                    const int tl = tail[rb + tid];
                    if (tl == 1) { first = 0; last = M - 1; }             // 'S': the whole tint (:217-224)
                    atomicAdd(&diff_s[first], 1); atomicAdd(&diff_s[last + 1], -1);
                    atomicAdd(&t_s[tl], 1);
                }
            }
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int j = tid + 256 * kk;
                if (j < M) {
                    const u64 *col = tile_s + (j >> 6);
                    const int sh = j & 63;
                    int s = 0;
                    for (int q = 0; q < n; ++q) s += (int)((col[q * Ws] >> sh) & 1ULL);
                    x[kk] += s;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) if (tid + 256 * kk < M) cons_s[tid + 256 * kk] = x[kk];
        if (tid == 0) { flag_s[0] = 0; flag_s[M + 1] = 0; }
        __syncthreads();
        const int j4 = 4 * tid;                                           // from here a thread has four consecutive segments
        {   // coverage = the running sum of diff_s; the flag of :233
            int v[4], run = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) { run += j4 + k < M ? diff_s[j4 + k] : 0; v[k] = run; }
            int inc = run;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(inc, d); if (lane >= d) inc += y; }
            if (lane == 63) wtot_s[0][wave] = inc;
            __syncthreads();
            int before = inc - run;
            for (int w = 0; w < wave; ++w) before += wtot_s[0][w];
            // x / c > 0.5 in doubles (:233) is 2x > c in integers: for counts below 2^31 both are exact in a double, and where
            // 2x > c the quotient is above 0.5 by x / c - 0.5 = (2x - c) / (2c) >= 1 / (2c), far more than an ulp of 0.5, so the
            // rounded quotient compares as the exact one does; where 2x <= c the exact quotient is at most 0.5 and rounding is
            // monotone.  (x >= 3 implies c >= 3: no division by zero is skipped.)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j4 + k < M) { const int c = cons_s[j4 + k]; flag_s[j4 + k + 1] = c >= 3 && 2 * (i64)c > (i64)(before + v[k]); }
        }
        __syncthreads();
        {   // exons = maximal runs of flags (:242-248): the exon's index is the number of run starts up to the segment, less one
            int v[4], run = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) { run += j4 + k < M ? (flag_s[j4 + k + 1] && !flag_s[j4 + k]) : 0; v[k] = run; }
            int inc = run;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(inc, d); if (lane >= d) inc += y; }
            if (lane == 63) wtot_s[1][wave] = inc;
            __syncthreads();
            int before = inc - run;
            for (int w = 0; w < wave; ++w) before += wtot_s[1][w];
            const i64 eo = exon_off[i];                                   // (M + 1) / 2 slots: runs have a gap between them
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = j4 + k;
                if (j < M && flag_s[j + 1]) {
                    const i64 e = eo + before + v[k] - 1;
                    if (!flag_s[j]) { seg_first[e] = j; start[e] = pos[p0 + j]; }
                    if (!flag_s[j + 2]) { seg_last[e] = j; end[e] = pos[p0 + j + 1]; }
                }
            }
            if (tid == 0) {
                const int total = wtot_s[1][0] + wtot_s[1][1] + wtot_s[1][2] + wtot_s[1][3];
                n_exon[i] = total;
                strand[i] = total == 0 ? 0 : (t_s[1] > t_s[2] ? '-' : '+');   // (:236-239)
            }
            if (tid < 3) tails[3 * (i64)i + tid] = t_s[tid];
        }
    }
}

// One workgroup per isoform that has exons; starts first, then ends, each against its own uncorrected boundaries (a tile of
// them in LDS, ascending: positions are).  Every thread takes member-read boundaries of that side: lower bound of
// boundary - window among the tile's, then a walk while the isoform boundary is <= boundary + window, one LDS atomic per vote
// (differences in 64 bits: boundary +- window leaves int32 at the ends of the range).  Then thread k decides boundary k of the
// tile: the LARGEST x whose v / N reaches the threshold wins, as the reference's ascending loop leaves it (:138-140); the
// division is the reference's, an IEEE double division of two integers that a double holds exactly.
__global__ void __launch_bounds__(256) k_iso_correct(int n_iso, const i64 *__restrict__ iso_read_off, const i64 *__restrict__ iso_q_off,
                                                     const int *__restrict__ read_start, const int *__restrict__ read_end,
                                                     const i64 *__restrict__ exon_off, const int *__restrict__ n_exon,
                                                     int *start, int *end, int window, double threshold) {
    __shared__ int b_s[kIsoBoundTile];
    __shared__ int vote_s[kIsoBoundTile * (2 * kIsoWindowMax + 1)];
    const int tid = threadIdx.x, nx = 2 * window + 1;
    for (int i = blockIdx.x; i < n_iso; i += gridDim.x) {
        const int ne = n_exon[i];
        if (ne == 0) continue;                                            // (the whole workgroup)
        const double N = (double)(iso_read_off[i + 1] - iso_read_off[i]); // skipped reads included: len(isoform['rids']) (:138)
        const i64 q0 = iso_q_off[i], q1 = iso_q_off[i + 1];               // the member reads' boundaries are contiguous
        const i64 eo = exon_off[i];
        for (int side = 0; side < 2; ++side) {
            int *bnd = (side ? end : start) + eo;
            const int *rbnd = side ? read_end : read_start;
            for (int k0 = 0; k0 < ne; k0 += kIsoBoundTile) {
                const int nt = ne - k0 < kIsoBoundTile ? ne - k0 : kIsoBoundTile;
                __syncthreads();                                          // (the previous tile's decisions are out)
                if (tid < nt) b_s[tid] = bnd[k0 + tid];
                for (int idx = tid; idx < nt * nx; idx += 256) vote_s[idx] = 0;
                __syncthreads();
                for (i64 q = q0 + tid; q < q1; q += 256) {
                    const i64 v = rbnd[q];
                    int lo = 0, hi = nt;
                    while (lo < hi) { const int mid = (lo + hi) >> 1; if ((i64)b_s[mid] < v - window) lo = mid + 1; else hi = mid; }
                    for (int k = lo; k < nt && (i64)b_s[k] <= v + window; ++k) atomicAdd(&vote_s[k * nx + (int)(v - b_s[k]) + window], 1);
                }
                __syncthreads();
                if (tid < nt) {
                    const i64 b = b_s[tid];
                    i64 out = b;
                    for (int xo = window; xo >= -window; --xo)
                        if ((double)vote_s[tid * nx + xo + window] / N >= threshold) { out = b + xo; break; }   // (a read boundary lies at b + xo: int32)
                    bnd[k0 + tid] = (int)out;
                }
            }
        }
    }
}

#endif
