/*
 * freddie_vis.h -- C-ABI of the GPU part of the segmentation-visualisation script (py/freddie_segment_vis.py).
 *
 * It replaces get_data() (py/freddie_segment_vis.py:199-222), run by the reference once per read and per annotated
 * transcript: for every object (a list of (s, e) intervals) and every canonical segment [B[j], B[j+1]) of its chromosome,
 *   - segment j is flagged iff some interval has B[j] <= s <= B[j+1] or s <= B[j] <= e (closed comparisons);
 *   - a flagged segment's class is 1, 0 or 2 as the covered fraction c = |locs & [B[j], B[j+1])| / (B[j+1] - B[j]) is
 *     > 0.9, < 0.1 or neither, where locs is the union of range(s, e) over the object's intervals.
 * The readers, the segment track and the pickle stay on the host (freddie_amd/segment_vis.py).
 *
 * Layout (caller-owned host arrays): chromosome c's boundaries are bounds[bound_off[c] .. bound_off[c+1]), strictly
 * ascending; a list of fewer than two boundaries has no segment.  Object o belongs to chromosome obj_chrom[o] and owns the
 * intervals iv[2 q], iv[2 q + 1] (s, e) for q in iv_off[o] .. iv_off[o+1], in any order; empty and reversed (s >= e)
 * intervals are allowed, as in the reference.
 */
#ifndef FREDDIE_VIS_H
#define FREDDIE_VIS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fvis_ctx fvis_ctx;

enum {
    FVIS_OK = 0,
    FVIS_ERR_ARG = 1,       /* null pointer, offsets not starting at 0 or not monotone, chromosome index out of range */
    FVIS_ERR_HIP = 2,
    FVIS_ERR_BOUNDS = 3,    /* a boundary list that is not strictly ascending */
    FVIS_ERR_EMPTY = 4      /* an object whose intervals cover no position (min() of an empty set in the reference, :201-203) */
};

int fvis_abi_version(void);
int fvis_create(int device, fvis_ctx **out);      /* fails when no HIP device is usable: there is no CPU fallback */
void fvis_destroy(fvis_ctx *c);
const char *fvis_last_error(const fvis_ctx *c);   /* c may be NULL: error of the last failed fvis_create() */
const char *fvis_source_hash(void);               /* the hash of the sources this binary was built from (freddie_amd/build.py) */

/* One batch of objects of any chromosomes.  On FVIS_ERR_BOUNDS *bad receives the chromosome, on FVIS_ERR_EMPTY the lowest
 * index of an object that covers no position; otherwise -1.  Coordinates are int32: a caller holding wider values reports
 * them itself. */
int fvis_classify(fvis_ctx *c, int32_t n_chrom, const int64_t *bound_off, const int32_t *bounds, int64_t n_obj,
                  const int32_t *obj_chrom, const int64_t *iv_off, const int32_t *iv, int64_t *bad);

/* Results of the last successful fvis_classify(), owned by the context and valid until its next fvis_classify() or
 * fvis_destroy(): object o's flagged segments are seg[flag_off[o] .. flag_off[o+1]), ascending, with their classes
 * (0, 1, 2) at the same places of cls; flag_off has n_obj + 1 entries. */
int fvis_results(fvis_ctx *c, const int64_t **flag_off, const int32_t **seg, const int8_t **cls);

/* Kernel time of the last call (HIP events on the library's stream), ms. */
int fvis_last_kernel_ms(fvis_ctx *c, float *ms);

#ifdef __cplusplus
}
#endif
#endif
