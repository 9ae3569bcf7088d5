// freddie_vis.hip -- gfx950 kernels + C-ABI (include/freddie_vis.h) of get_data() (py/freddie_segment_vis.py:199-222): for
// every object (read or annotated transcript) the segments it flags and their coverage class.
//
// The reference builds the set of an object's positions and, per flagged segment, tests every position of the segment
// against it.  Here, per object, its intervals are sorted by start (one batch-wide radix sort on (object, start)); then
//   - the flag conditions B[j] <= s <= B[j+1] or s <= B[j] <= e give one contiguous index range per interval,
//     [lower_bound(B[1..S], s), upper_bound(B[0..S-1], max(s, e)) - 1], and the ranges' lower ends grow with s, so a
//     running maximum of the upper ends leaves each interval the part of its range no earlier interval flagged: disjoint,
//     ascending, and its length is the interval's share of the output;
//   - the union of the intervals' [s, e) is the pieces [max(s, running max of the earlier e), e), ascending and disjoint,
//     with their prefix lengths: F(x) = |locs & (-inf, x)| is one binary search over the object's pieces.
// k_count does both scans (a wave per object), an exclusive scan over the intervals gives every output slot, and k_emit
// (a thread per flagged segment) writes (j, class of F(B[j+1]) - F(B[j]) over B[j+1] - B[j]).
#include "freddie_vis.h"

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <climits>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

namespace {

typedef long long i64;
typedef unsigned long long u64;

// first index k of a[0..n) with a[k] >= v (lower) / a[k] > v (upper)
__device__ __forceinline__ i64 lower_bound(const int *a, i64 n, i64 v) {
    i64 lo = 0, hi = n;
    while (lo < hi) { const i64 m = (lo + hi) >> 1; if ((i64)a[m] < v) lo = m + 1; else hi = m; }
    return lo;
}
__device__ __forceinline__ i64 upper_bound(const int *a, i64 n, i64 v) {
    i64 lo = 0, hi = n;
    while (lo < hi) { const i64 m = (lo + hi) >> 1; if ((i64)a[m] <= v) lo = m + 1; else hi = m; }
    return lo;
}
__device__ __forceinline__ i64 upper_bound64(const i64 *a, i64 n, i64 v) {
    i64 lo = 0, hi = n;
    while (lo < hi) { const i64 m = (lo + hi) >> 1; if (a[m] <= v) lo = m + 1; else hi = m; }
    return lo;
}

// sort keys: object in the high word, start + 2^31 in the low word (the order of int32 starts)
__global__ void k_keys(i64 n_obj, i64 n_iv, const i64 *iv_off, const int2 *iv, u64 *key, int *end) {
    for (i64 q = blockIdx.x * (i64)blockDim.x + threadIdx.x; q < n_iv; q += (i64)gridDim.x * blockDim.x) {
        const i64 o = upper_bound64(iv_off, n_obj + 1, q) - 1;          // iv_off[o] <= q < iv_off[o + 1]
        const int2 v = iv[q];
        key[q] = ((u64)o << 32) | (u64)((unsigned)v.x ^ 0x80000000u);
        end[q] = v.y;
    }
}

__device__ __forceinline__ i64 wave_incl_max(i64 v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const i64 t = __shfl_up(v, d, 64); if (lane >= d) v = v > t ? v : t; }
    return v;
}
__device__ __forceinline__ i64 wave_incl_sum(i64 v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const i64 t = __shfl_up(v, d, 64); if (lane >= d) v += t; }
    return v;
}

// One wave per object, its sorted intervals 64 at a time, the running maxima / sums carried across chunks.
// Per sorted interval q: ps (piece start), cum (length of the earlier pieces), first (first newly flagged segment) and
// cnt[q] (how many); an object whose pieces have no length is reported through *bad (lowest index).
__global__ void __launch_bounds__(256) k_count(i64 n_obj, const i64 *iv_off, const int *obj_chrom, const i64 *bound_off,
                                               const int *bounds, const u64 *key, const int *end, int *ps_out, i64 *cum_out,
                                               int *first_out, i64 *cnt_out, u64 *bad) {
    const int lane = threadIdx.x & 63;
    const i64 waves = (i64)gridDim.x * (blockDim.x >> 6);
    for (i64 o = blockIdx.x * (i64)(blockDim.x >> 6) + (threadIdx.x >> 6); o < n_obj; o += waves) {
        const i64 q0 = iv_off[o], q1 = iv_off[o + 1];
        const int c = obj_chrom[o];
        const int *B = bounds + bound_off[c];
        const i64 nb = bound_off[c + 1] - bound_off[c];
        const i64 S = nb > 1 ? nb - 1 : 0;                                 // segments
        i64 hi_carry = -1, e_carry = LLONG_MIN, cum_carry = 0;
        for (i64 base = q0; base < q1; base += 64) {
            const i64 q = base + lane;
            const bool on = q < q1;
            const i64 s = on ? (i64)(int)((unsigned)key[q] ^ 0x80000000u) : 0;
            const i64 e = on ? (i64)end[q] : LLONG_MIN;
            i64 lo = 0, hi = -1;
            if (on && S > 0) {
                lo = lower_bound(B + 1, S, s);                              // first j with B[j+1] >= s
                hi = upper_bound(B, S, s > e ? s : e) - 1;                  // last j with B[j] <= max(s, e)
            }
            const i64 hi_incl = wave_incl_max(hi, lane);
            i64 hi_prev = __shfl_up(hi_incl, 1, 64);
            hi_prev = lane == 0 ? hi_carry : (hi_prev > hi_carry ? hi_prev : hi_carry);
            const i64 first = lo > hi_prev + 1 ? lo : hi_prev + 1;
            const i64 cnt = on && hi >= first ? hi - first + 1 : 0;

            const i64 e_incl = wave_incl_max(e, lane);
            i64 e_prev = __shfl_up(e_incl, 1, 64);
            e_prev = lane == 0 ? e_carry : (e_prev > e_carry ? e_prev : e_carry);
            const i64 ps = s > e_prev ? s : e_prev;
            const i64 len = on && e > ps ? e - ps : 0;
            const i64 len_incl = wave_incl_sum(len, lane);
            if (on) {
                ps_out[q] = (int)ps;                                        // (max of int32 values: non-decreasing along q)
                cum_out[q] = cum_carry + len_incl - len;
                first_out[q] = (int)(cnt ? first : 0);
                cnt_out[q] = cnt;
            }
            const i64 hi_all = __shfl(hi_incl, 63, 64), e_all = __shfl(e_incl, 63, 64), len_all = __shfl(len_incl, 63, 64);
            hi_carry = hi_all > hi_carry ? hi_all : hi_carry;
            e_carry = e_all > e_carry ? e_all : e_carry;
            cum_carry += len_all;
        }
        if (lane == 0 && cum_carry == 0) atomicMin(bad, (u64)o);
    }
}

// |locs & (-inf, x)| of the object whose sorted intervals are [qa, qb)
__device__ __forceinline__ i64 covered_below(i64 x, i64 qa, i64 qb, const int *ps, const i64 *cum, const int *end) {
    const i64 k = qa + upper_bound(ps + qa, qb - qa, x) - 1;                // last piece starting at or before x
    if (k < qa) return 0;
    const i64 p = ps[k], e = end[k];
    const i64 len = e > p ? e - p : 0;
    const i64 in = x - p < len ? x - p : len;
    return cum[k] + in;
}

// One thread per flagged segment: off[q] <= t < off[q + 1] names its interval.
__global__ void k_emit(i64 total, i64 n_iv, const i64 *off, const u64 *key, const i64 *iv_off, const int *obj_chrom,
                       const i64 *bound_off, const int *bounds, const int *ps, const i64 *cum, const int *end, const int *first,
                       int *seg_out, signed char *cls_out) {
    for (i64 t = blockIdx.x * (i64)blockDim.x + threadIdx.x; t < total; t += (i64)gridDim.x * blockDim.x) {
        const i64 q = upper_bound64(off, n_iv + 1, t) - 1;
        const i64 o = (i64)(key[q] >> 32);
        const i64 qa = iv_off[o], qb = iv_off[o + 1];
        const int *B = bounds + bound_off[obj_chrom[o]];
        const i64 j = first[q] + (t - off[q]);
        const i64 b0 = B[j], b1 = B[j + 1];
        const i64 k = covered_below(b1, qa, qb, ps, cum, end) - covered_below(b0, qa, qb, ps, cum, end);
        const i64 n = b1 - b0;
        // c = k / n in fp64 against 0.9 / 0.1 (:215-220).  10k > 9n decides c > 0.9 exactly: where k/n != 9/10 the two differ
        // by at least 1/(10n) > 2^-36 (n < 2^32), far above fp64's rounding near 0.9 (2^-53), and where k/n == 9/10 the quotient
        // rounds to the same double as the literal 0.9, which is not greater; likewise 10k < n for c < 0.1.
        seg_out[t] = (int)j;
        cls_out[t] = (signed char)(10 * k > 9 * n ? 1 : (10 * k < n ? 0 : 2));
    }
}

__global__ void k_flag_off(i64 n_obj, const i64 *iv_off, const i64 *off, i64 *flag_off) {
    for (i64 o = blockIdx.x * (i64)blockDim.x + threadIdx.x; o <= n_obj; o += (i64)gridDim.x * blockDim.x) flag_off[o] = off[iv_off[o]];
}

}  // namespace

struct fvis_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {};
    std::string err;
    float kernel_ms = 0.f;
    std::vector<int64_t> flag_off;
    std::vector<int32_t> seg;
    std::vector<int8_t> cls;
};

namespace {

std::string g_create_error;

int fail(fvis_ctx *c, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_error = buf;
    return code;
}

struct Dev {
    void *p = nullptr;
    ~Dev() { if (p) (void)hipFree(p); }
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

#define HIP_TRY(c, expr)                                                                                     \
    do {                                                                                                     \
        hipError_t e__ = (expr);                                                                             \
        if (e__ != hipSuccess) return fail((c), FVIS_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e__));      \
    } while (0)
#define TRY(expr) do { int rc__ = (expr); if (rc__) return rc__; } while (0)

int alloc(fvis_ctx *c, Dev &d, size_t bytes) {
    HIP_TRY(c, hipMalloc(&d.p, bytes + 16));
    return FVIS_OK;
}
template <typename T>
int to_device(fvis_ctx *c, Dev &d, const T *src, size_t n) {
    TRY(alloc(c, d, n * sizeof(T)));
    if (n) HIP_TRY(c, hipMemcpyAsync(d.p, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return FVIS_OK;
}

int check_offsets(fvis_ctx *c, const char *what, const int64_t *off, i64 n) {
    if (off[0] != 0) return fail(c, FVIS_ERR_ARG, "%s does not start at 0", what);
    for (i64 i = 0; i < n; ++i) if (off[i + 1] < off[i]) return fail(c, FVIS_ERR_ARG, "%s is not monotone at %lld", what, i);
    return FVIS_OK;
}

unsigned bit_width(u64 v) { unsigned b = 0; while (v) { ++b; v >>= 1; } return b; }

}  // namespace

extern "C" {

int fvis_abi_version(void) { return 1; }

#ifndef FREDDIE_SOURCE_HASH
#define FREDDIE_SOURCE_HASH ""
#endif
/* what this binary was built from (freddie_amd/build.py looks for the marker in the file) */
static const char freddie_source_stamp[] __attribute__((used)) = "FREDDIE_SRC_HASH=" FREDDIE_SOURCE_HASH;
const char *fvis_source_hash(void) { return freddie_source_stamp + 17; }

int fvis_create(int device, fvis_ctx **out) {
    if (!out) return FVIS_ERR_ARG;
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, FVIS_ERR_HIP, "no HIP device available: %s (this library has no CPU fallback)",
                    e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    if (device < 0 || device >= n) return fail(nullptr, FVIS_ERR_ARG, "device ordinal out of range");
    fvis_ctx *c = new fvis_ctx();
    c->device = device;
    e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    for (int i = 0; e == hipSuccess && i < 4; ++i) e = hipEventCreate(&c->ev[i]);
    if (e != hipSuccess) {
        fail(nullptr, FVIS_ERR_HIP, "context creation failed: %s", hipGetErrorString(e));
        fvis_destroy(c);
        return FVIS_ERR_HIP;
    }
    *out = c;
    return FVIS_OK;
}

void fvis_destroy(fvis_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    for (int i = 0; i < 4; ++i) if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
    delete c;
}

const char *fvis_last_error(const fvis_ctx *c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int fvis_classify(fvis_ctx *c, int32_t n_chrom, const int64_t *bound_off, const int32_t *bounds, int64_t n_obj,
                  const int32_t *obj_chrom, const int64_t *iv_off, const int32_t *iv, int64_t *bad) {
    if (!c) return FVIS_ERR_ARG;
    if (bad) *bad = -1;
    c->flag_off.clear(); c->seg.clear(); c->cls.clear();
    c->kernel_ms = 0.f;
    if (n_chrom < 0 || n_obj < 0 || !bound_off || !iv_off || (n_obj > 0 && !obj_chrom) || !bad)
        return fail(c, FVIS_ERR_ARG, "null pointer or negative count");
    if (n_obj >= ((i64)1 << 31)) return fail(c, FVIS_ERR_ARG, "more than 2^31 - 1 objects in one call");
    HIP_TRY(c, hipSetDevice(c->device));
    TRY(check_offsets(c, "bound_off", bound_off, n_chrom));
    TRY(check_offsets(c, "iv_off", iv_off, n_obj));
    const i64 NB = bound_off[n_chrom], NQ = iv_off[n_obj];
    if ((NB > 0 && !bounds) || (NQ > 0 && !iv)) return fail(c, FVIS_ERR_ARG, "null pointer");
    for (int ch = 0; ch < n_chrom; ++ch)
        for (i64 k = bound_off[ch] + 1; k < bound_off[ch + 1]; ++k)
            if (bounds[k] <= bounds[k - 1]) {
                *bad = ch;
                return fail(c, FVIS_ERR_BOUNDS, "chromosome %d: boundaries are not strictly ascending at %lld", ch, k - bound_off[ch]);
            }
    for (i64 o = 0; o < n_obj; ++o)
        if (obj_chrom[o] < 0 || obj_chrom[o] >= n_chrom) return fail(c, FVIS_ERR_ARG, "object %lld: chromosome index out of range", o);
    c->flag_off.assign((size_t)n_obj + 1, 0);
    if (n_obj == 0) return FVIS_OK;

    hipStream_t s = c->stream;
    Dev d_bo, d_b, d_oc, d_io, d_iv, d_key[2], d_end[2], d_ps, d_cum, d_first, d_cnt, d_off, d_bad, d_fo, d_tmp, d_seg, d_cls;
    TRY(to_device(c, d_bo, bound_off, (size_t)n_chrom + 1));
    TRY(to_device(c, d_b, bounds, (size_t)NB));
    TRY(to_device(c, d_oc, obj_chrom, (size_t)n_obj));
    TRY(to_device(c, d_io, iv_off, (size_t)n_obj + 1));
    TRY(to_device(c, d_iv, iv, (size_t)NQ * 2));
    for (int b = 0; b < 2; ++b) { TRY(alloc(c, d_key[b], (size_t)NQ * 8)); TRY(alloc(c, d_end[b], (size_t)NQ * 4)); }
    TRY(alloc(c, d_ps, (size_t)NQ * 4));
    TRY(alloc(c, d_cum, (size_t)NQ * 8));
    TRY(alloc(c, d_first, (size_t)NQ * 4));
    TRY(alloc(c, d_cnt, (size_t)(NQ + 1) * 8));
    TRY(alloc(c, d_off, (size_t)(NQ + 1) * 8));
    TRY(alloc(c, d_bad, 8));
    TRY(alloc(c, d_fo, (size_t)(n_obj + 1) * 8));
    // temporary storage of the sort and the scan: the larger of the two
    const unsigned end_bit = 32 + bit_width((u64)n_obj - 1);
    size_t sort_bytes = 0, scan_bytes = 0;
    HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, sort_bytes, d_key[0].as<u64>(), d_key[1].as<u64>(), d_end[0].as<int>(),
                                         d_end[1].as<int>(), (size_t)NQ, 0u, end_bit, s));
    HIP_TRY(c, rocprim::exclusive_scan(nullptr, scan_bytes, d_cnt.as<i64>(), d_off.as<i64>(), (i64)0, (size_t)NQ + 1,
                                       rocprim::plus<i64>(), s));
    TRY(alloc(c, d_tmp, sort_bytes > scan_bytes ? sort_bytes : scan_bytes));

    HIP_TRY(c, hipEventRecord(c->ev[0], s));
    HIP_TRY(c, hipMemsetAsync(d_bad.p, 0xff, 8, s));
    HIP_TRY(c, hipMemsetAsync(d_cnt.as<i64>() + NQ, 0, 8, s));
    const int blocks_q = (int)(NQ / 256 + 1 < 8192 ? NQ / 256 + 1 : 8192);
    if (NQ) {
        hipLaunchKernelGGL(k_keys, dim3(blocks_q), dim3(256), 0, s, (i64)n_obj, NQ, d_io.as<i64>(), d_iv.as<int2>(), d_key[0].as<u64>(),
                           d_end[0].as<int>());
        HIP_TRY(c, rocprim::radix_sort_pairs(d_tmp.p, sort_bytes, d_key[0].as<u64>(), d_key[1].as<u64>(), d_end[0].as<int>(),
                                             d_end[1].as<int>(), (size_t)NQ, 0u, end_bit, s));
    }
    const i64 blocks_o = n_obj / 4 + 1;
    hipLaunchKernelGGL(k_count, dim3((unsigned)(blocks_o < 16384 ? blocks_o : 16384)), dim3(256), 0, s, (i64)n_obj, d_io.as<i64>(),
                       d_oc.as<int>(), d_bo.as<i64>(), d_b.as<int>(), d_key[1].as<u64>(), d_end[1].as<int>(), d_ps.as<int>(),
                       d_cum.as<i64>(), d_first.as<int>(), d_cnt.as<i64>(), d_bad.as<u64>());
    HIP_TRY(c, rocprim::exclusive_scan(d_tmp.p, scan_bytes, d_cnt.as<i64>(), d_off.as<i64>(), (i64)0, (size_t)NQ + 1,
                                       rocprim::plus<i64>(), s));
    const i64 blocks_f = n_obj / 256 + 1;
    hipLaunchKernelGGL(k_flag_off, dim3((unsigned)(blocks_f < 8192 ? blocks_f : 8192)), dim3(256), 0, s, (i64)n_obj, d_io.as<i64>(),
                       d_off.as<i64>(), d_fo.as<i64>());
    HIP_TRY(c, hipEventRecord(c->ev[1], s));
    u64 bad_obj = 0;
    HIP_TRY(c, hipMemcpyAsync(&bad_obj, d_bad.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(c->flag_off.data(), d_fo.p, (size_t)(n_obj + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    float ms0 = 0.f;
    (void)hipEventElapsedTime(&ms0, c->ev[0], c->ev[1]);
    if (bad_obj != ~0ull) {
        *bad = (int64_t)bad_obj;
        c->flag_off.clear();
        return fail(c, FVIS_ERR_EMPTY, "object %lld covers no position (every interval has s >= e)", (i64)bad_obj);
    }
    const i64 T = c->flag_off[(size_t)n_obj];
    c->seg.resize((size_t)T);
    c->cls.resize((size_t)T);
    c->kernel_ms = ms0;
    if (T == 0) return FVIS_OK;
    TRY(alloc(c, d_seg, (size_t)T * 4));
    TRY(alloc(c, d_cls, (size_t)T));
    HIP_TRY(c, hipEventRecord(c->ev[2], s));
    const i64 blocks_t = T / 256 + 1;
    hipLaunchKernelGGL(k_emit, dim3((unsigned)(blocks_t < 16384 ? blocks_t : 16384)), dim3(256), 0, s, T, NQ, d_off.as<i64>(),
                       d_key[1].as<u64>(), d_io.as<i64>(), d_oc.as<int>(), d_bo.as<i64>(), d_b.as<int>(), d_ps.as<int>(),
                       d_cum.as<i64>(), d_end[1].as<int>(), d_first.as<int>(), d_seg.as<int>(), d_cls.as<signed char>());
    HIP_TRY(c, hipEventRecord(c->ev[3], s));
    HIP_TRY(c, hipMemcpyAsync(c->seg.data(), d_seg.p, (size_t)T * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(c->cls.data(), d_cls.p, (size_t)T, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    float ms1 = 0.f;
    (void)hipEventElapsedTime(&ms1, c->ev[2], c->ev[3]);
    c->kernel_ms = ms0 + ms1;
    return FVIS_OK;
}

int fvis_results(fvis_ctx *c, const int64_t **flag_off, const int32_t **seg, const int8_t **cls) {
    if (!c || !flag_off || !seg || !cls) return FVIS_ERR_ARG;
    *flag_off = c->flag_off.data();
    *seg = c->seg.data();
    *cls = c->cls.data();
    return FVIS_OK;
}

int fvis_last_kernel_ms(fvis_ctx *c, float *ms) {
    if (!c || !ms) return FVIS_ERR_ARG;
    *ms = c->kernel_ms;
    return FVIS_OK;
}

}  // extern "C"
