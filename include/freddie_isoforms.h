/*
 * freddie_isoforms.h -- C-ABI of the GPU part of the isoform-consensus stage.
 *
 * It replaces the two per-read loops of the reference's py/freddie_isoforms.py:
 *   - isoforms_cons()       :203-250   per isoform and segment: how many member reads span the segment (cov) and how
 *                                      many of those cover it (cons); per isoform the poly-tail categories of its reads
 *   - correct_boundaries()  :122-140   per isoform boundary: votes of the member reads' alignment boundaries that lie
 *                                      within +-correction_window of it, by offset
 * The decisions taken from these integers (x/c > 0.5 with x >= 3, v/N >= majority_threshold, strand, exon runs) can be
 * taken in either place.  fiso_consensus* / fiso_boundary_votes return the integers and leave the decisions to the host
 * (freddie_amd/isoforms.py, --decide host, the default).  fiso_isoforms (below) takes them on the device as well: one
 * call, one bit per label in, every isoform's strand and corrected exons out, and neither counts nor votes leave the
 * chip (--decide gpu).  The cluster / split TSV readers (:143-201) and the GTF writer (:72-119) are host Python either way.
 *
 * Layout (caller-owned host arrays): reads are grouped by isoform, isoform i owns reads iso_read_off[i] ..
 * iso_read_off[i+1]; read r's corrected labels are the n_seg[i] ASCII bytes at labels[read_lab_off[r]] and its
 * poly-tail category 'N','S','E' is tail[r] = 0,1,2.  Results for isoform i start at iso_seg_off[i] (one int32 per
 * segment) and at 3 * i (tails).
 */
#ifndef FREDDIE_ISOFORMS_H
#define FREDDIE_ISOFORMS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fiso_ctx fiso_ctx;

enum { FISO_OK = 0, FISO_ERR_ARG = 1, FISO_ERR_HIP = 2 };

int fiso_abi_version(void);
int fiso_create(int device, fiso_ctx **out);      /* fails when no HIP device is usable: there is no CPU fallback */
void fiso_destroy(fiso_ctx *c);
const char *fiso_last_error(const fiso_ctx *c);   /* c may be NULL: error of the last failed fiso_create() */

/* isoforms_cons() counts (py/freddie_isoforms.py:203-232).  A read without any '1' is skipped altogether (:215-216);
 * a read with tail 'S' spans every segment (:217-224, as written in the reference: both tests are on 'S'). */
int fiso_consensus(fiso_ctx *c, int32_t n_iso, const int64_t *iso_read_off, const int32_t *n_seg, const int64_t *iso_seg_off,
                   const int64_t *read_lab_off, const uint8_t *labels, const uint8_t *tail,
                   int32_t *cons_out, int32_t *cov_out, int32_t *tails_out);

/* The same with the labels at two bits each, in the layout fseg_results_packed() (include/freddie_seg.h) delivers: label g of
 * the arena = bits 2(g & 3).. of labels2[g >> 2], code = ASCII & 3; read_lab_off still counts labels.  A quarter of the bytes
 * across PCIe and out of HBM; for a producer that holds the packed form (the text TSVs the stages exchange hold bytes). */
int fiso_consensus_packed(fiso_ctx *c, int32_t n_iso, const int64_t *iso_read_off, const int32_t *n_seg, const int64_t *iso_seg_off,
                          const int64_t *read_lab_off, const uint8_t *labels2, const uint8_t *tail,
                          int32_t *cons_out, int32_t *cov_out, int32_t *tails_out);

/* correct_boundaries() votes for one side (py/freddie_isoforms.py:129-137).  Isoform i owns the (ascending) boundaries
 * iso_bound[iso_b_off[i] .. iso_b_off[i+1]); read r owns read_bound[read_b_off[r] .. read_b_off[r+1]).
 * votes_out[(iso_b_off[i] + idx) * (2 * window + 1) + (x + window)] = number of (read, boundary) of isoform i with
 * boundary - iso_bound == x.  window in [1, 20] (:45). */
int fiso_boundary_votes(fiso_ctx *c, int32_t n_iso, const int64_t *iso_read_off, const int64_t *iso_b_off, const int32_t *iso_bound,
                        const int64_t *read_b_off, const int32_t *read_bound, int32_t window, int32_t *votes_out);

/* Kernel time of the last call (HIP events on the library's stream), ms. */
int fiso_last_kernel_ms(fiso_ctx *c, float *ms);

/* ---- isoforms_cons() + correct_boundaries() of both sides, decisions included, in one call ----------------------------
 * Input: tint t owns the M_t + 1 strictly ascending segment positions pos[tint_pos_off[t] .. tint_pos_off[t+1]); isoform i
 * belongs to tint iso_tint[i] (M = M_t segments) and owns reads iso_read_off[i] .. iso_read_off[i+1]; read r owns the
 * W = ceil(M / 64) words bits[read_bits_off[r] .. read_bits_off[r+1]) (rows are contiguous: read_bits_off has one entry
 * per read and one more, and advances by W), bit j & 63 of word j >> 6 set when label j is '1' -- 'X', '-', '0' and '2'
 * all count as not '1', which is all isoforms_cons() asks (:213-231); its alignment intervals are read_start / read_end
 * [read_b_off[r] .. read_b_off[r+1]).
 *
 * What is decided (the reference's semantics, oracle/isoforms_oracle.py):
 *   counts     a read without a set bit is skipped; an 'S' read with a set bit spans segments 0 .. M - 1, any other read
 *              its first .. last set bit; tails counts the reads that are not skipped
 *   exon flag  cons >= 3 && 2 * cons > cov; exons are the maximal runs of flags, from pos[first] to pos[last + 1]
 *   strand     '-' exactly when tails[S] > tails[E]
 *   correction window == 0: none.  Otherwise per side and boundary b (uncorrected): v[x] = the (member read, boundary of
 *              that side) pairs with boundary - b == x (64-bit differences), |x| <= window; N = the isoform's reads, skipped
 *              ones included; the boundary becomes b + x for the largest x with (double)v / (double)N >= majority_threshold.
 *
 * Refusals are made on the host before any launch, name the refused item in fiso_last_error() and leave the context
 * usable: FISO_ERR_ARG for malformed input (offsets, a bit set beyond M, a tail above 2, an iso_tint out of range,
 * positions that are not strictly ascending, window outside [0, 20], threshold outside [0.5, 1]); FISO_ERR_UNSUPPORTED
 * for an isoform of more than fiso_isoforms_limits()[0] segments. */
enum { FISO_ERR_UNSUPPORTED = 3 };

typedef struct {
    int32_t n_tint;  const int64_t *tint_pos_off;  const int32_t *pos;   /* tint t: M_t + 1 segment positions */
    int32_t n_iso;   const int32_t *iso_tint;      const int64_t *iso_read_off;
    const int64_t *read_bits_off;  const uint64_t *bits;  /* read r of isoform i: W = ceil(M / 64) words, bit j = label j is '1' */
    const uint8_t *tail;                                   /* 0 N, 1 S, 2 E */
    const int64_t *read_b_off;  const int32_t *read_start;  const int32_t *read_end;   /* the read's alignment intervals */
} fiso_input;

int fiso_isoforms(fiso_ctx *c, const fiso_input *in, double majority_threshold, int32_t window);

typedef struct {
    int32_t n_iso;
    const int64_t *exon_off;   /* capacity layout: isoform i owns (M + 1) / 2 slots from exon_off[i] */
    const int32_t *n_exon;     /* slots in use; 0 = no exon, the reference's `continue` at :232-233 */
    const int32_t *start, *end;           /* corrected */
    const int32_t *seg_first, *seg_last;  /* the run of segments behind each exon */
    const uint8_t *strand;     /* '+' / '-', 0 without an exon */
    const int32_t *tails;      /* 3 an isoform, as fiso_consensus gives them */
} fiso_isoforms_out;

/* The last successful fiso_isoforms() call's results: pinned host memory, owned by the context until its next call
 * (slots an isoform does not use hold 0).  FISO_ERR_ARG without a successful call behind it. */
int fiso_isoforms_results(fiso_ctx *c, fiso_isoforms_out *out);
/* out = {longest supported row (1024 segments), reads per LDS tile of k_iso_exons, boundaries per LDS tile of k_iso_correct, 0} */
int fiso_isoforms_limits(int32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif
