/*
 * freddie_host.h -- C-ABI of the native host side of the segmentation stage:
 * multi-threaded parsing of split_*.tsv / reads_*.tsv into the flat arrays fseg_upload() takes, and
 * multi-threaded gaps / poly-A annotation + segment_*.tsv writing from the device results.
 *
 * It replaces, for the batched CLI path, the reference's Python
 *   read_split()      py/freddie_segment.py:121-171  (incl. the read_reps grouping :165-170)
 *   read_sequence()   py/freddie_segment.py:174-185
 *   get_unaligned_gaps_and_polyA() and helpers   py/freddie_segment.py:289-472
 *   the writer part of run_segment()             py/freddie_segment.py:703-732
 * and (row N2) a binary side-car of a partition's two TSVs that the loader takes instead of parsing them again.
 * It does no segmentation arithmetic (that is libfreddie_seg.so's job, on the GPU).
 */
#ifndef FREDDIE_HOST_H
#define FREDDIE_HOST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fhost_batch fhost_batch;

/* Parse n partitions (split_paths[i], reads_paths[i]) with n_threads worker threads.
 * Returns NULL on allocation failure; otherwise a batch whose fhost_error() is "" on success. */
fhost_batch *fhost_load(const char *const *split_paths, const char *const *reads_paths, int32_t n, int32_t n_threads);
void fhost_free(fhost_batch *b);
const char *fhost_error(const fhost_batch *b);   /* "" when the batch is usable */

/* Sizes and flat arrays in exactly the layout of fseg_batch (include/freddie_seg.h).  Pointers stay valid
 * until fhost_free(). */
int32_t fhost_n_part(const fhost_batch *b);
int64_t fhost_n_reads(const fhost_batch *b);
const int64_t *fhost_part_iv_off(const fhost_batch *b);
const int32_t *fhost_iv_start(const fhost_batch *b);
const int32_t *fhost_iv_end(const fhost_batch *b);
const int64_t *fhost_part_rep_off(const fhost_batch *b);
const int32_t *fhost_rep_weight(const fhost_batch *b);
const int64_t *fhost_rep_exon_off(const fhost_batch *b);
const int32_t *fhost_ex_ts(const fhost_batch *b);
const int32_t *fhost_ex_te(const fhost_batch *b);

/* Annotate and write: for partition p the device results are final positions
 * final_pos[part_final_off[p] .. part_final_off[p+1]) and the label rows of its read reps at
 * labels[label_off[p] + rep * (F_p - 1)] (ASCII '0','1','2'; what fseg_download() returns).
 * out_paths[p] receives segment_<contig>_<tint>.tsv.  Returns 0 on success; on failure fhost_error() says
 * which reference assertion would have fired. */
int32_t fhost_write(fhost_batch *b, const int64_t *part_final_off, const int32_t *final_pos, const int64_t *label_off,
                    const uint8_t *labels, const char *const *out_paths, int32_t n_threads);

/* The same with the labels at two bits each, as fseg_results_packed() hands them over (label byte g of the arena =
 * bits 2(g & 3).. of labels2[g >> 2]; label_off still counts labels): the rows are unpacked straight into the TSV. */
int32_t fhost_write_packed(fhost_batch *b, const int64_t *part_final_off, const int32_t *final_pos, const int64_t *label_off,
                           const uint8_t *labels2, const char *const *out_paths, int32_t n_threads);

/* ---- the annotation computed elsewhere (include/freddie_seg.h, fseg_annotate) ------------------------------------------------
 * fhost_reads begins with the fields of fseg_reads, in its order and with its meaning, so that a pointer to it is a pointer to an
 * fseg_reads: the per-read arrays of a loaded batch, partitions in batch order and a partition's reads in file order; every read's
 * letters start on a word of seq_classes.  The class codes (0 'A', 1 'T', 2 any other byte) are built from the TSV letters or from
 * the side-car's packed letters and exception list, on n_threads.  Pointers stay valid until fhost_free(). */
typedef struct {
    int64_t n_read;
    const int32_t *read_part;
    const int32_t *read_rep;
    const uint8_t *strand;
    const int32_t *seq_len;
    const int64_t *seq_off;
    const int64_t *read_q_off;
    const int32_t *qs;
    const int32_t *qe;
    const int64_t *cig_off;
    const uint8_t *cig_op;
    const int32_t *cig_len;
    const uint32_t *seq_classes;
    const int64_t *read_id;        /* (beyond fseg_reads: the read ids of the split TSVs) */
} fhost_reads;
int32_t fhost_read_arrays(fhost_batch *b, int32_t n_threads, fhost_reads *out);   /* 0 on success */

/* The tint ids and contigs of the batch's partitions and the names and contigs of its reads (fhost_reads' order): views, not
 * NUL-terminated, into the split TSVs or side-cars the batch keeps mapped until fhost_free(). */
typedef struct {
    int32_t n_part;
    int64_t n_read;
    const int64_t *part_id;
    const char *const *part_chr;
    const int32_t *part_chr_len;
    const char *const *name;
    const int32_t *name_len;
    const char *const *chr;
    const int32_t *chr_len;
} fhost_names;
int32_t fhost_read_names(fhost_batch *b, fhost_names *out);   /* 0 on success */

/* fseg_annot, field for field (and so the gap / clip / poly lists and tail of fhost_segments below), for the batch's reads in
 * fhost_reads' order. */
typedef struct {
    int64_t n_read;
    const int64_t *gap_off;
    const int32_t *gaps;
    const int64_t *clip_off;
    const int32_t *clips;
    const int64_t *poly_off;
    const int32_t *polys;
    const uint8_t *tail;
    const int64_t *tok_off;
    const uint32_t *tok;
} fhost_annot;

/* fhost_write_packed with the annotation GIVEN instead of computed: formats its tokens and puts them in the line order of
 * sorted(set(...)) (py/freddie_segment.py:472); the order of a read's gaps in `annotation` does not matter.  tail, tok_off and tok
 * are not read.  The bytes equal fhost_write_packed's when the annotation equals what it computes. */
int32_t fhost_write_annotated(fhost_batch *b, const int64_t *part_final_off, const int32_t *final_pos, const int64_t *label_off,
                              const uint8_t *labels2, const fhost_annot *annotation, const char *const *out_paths, int32_t n_threads);

/* ---- binary side-car ------------------------------------------------------------
 * split_<contig>_<tint>.fsc, written next to the TSVs that py/freddie_split.py:445-481 produces, holds the parsed
 * form of both files (flat exon / CIGAR arrays, the read_reps grouping of py/freddie_segment.py:165-170, sequences
 * at two bits per base with an exception list for bytes other than ACGT).  A side-car is used only when the sizes
 * and mtimes recorded in it equal those of its two TSVs (and, with verify_checksum, its payload checksum holds);
 * otherwise the TSVs are parsed, so results never depend on whether side-cars exist. */

/* Like fhost_load(); sidecar_paths may be NULL, and any entry may be NULL. */
fhost_batch *fhost_load_sidecar(const char *const *split_paths, const char *const *reads_paths,
                                const char *const *sidecar_paths, int32_t n, int32_t n_threads, int32_t verify_checksum);
int32_t fhost_n_from_sidecar(const fhost_batch *b);   /* partitions of the batch that came from a side-car */

/* Write the side-car of every partition of a loaded batch (atomically: temp file + rename).  Returns 0 on success. */
int32_t fhost_sidecar_write(fhost_batch *b, const char *const *split_paths, const char *const *reads_paths,
                            const char *const *sidecar_paths, int32_t n_threads);

/* ---- the split directory's listing and the empty .log files (round 6) ---------------------------------------------------
 * What main() does before and around the batches as loops of system calls (py/freddie_segment.py:852-857: one directory per
 * contig, one split_<contig>_<tint>.tsv per partition; :695: an empty segment_*.log per partition), natively and on n_threads:
 * fhost_discover lists every split_*.tsv of every contig directory with its size (what the scatter and the batching weigh a
 * partition by); fhost_touch creates (or truncates) the given files. */
typedef struct fhost_listing fhost_listing;
fhost_listing *fhost_discover(const char *split_dir, int32_t n_threads);   /* NULL: out of memory; else check fhost_listing_error() */
void fhost_listing_free(fhost_listing *l);
const char *fhost_listing_error(const fhost_listing *l);                   /* "" when the listing is usable */
int64_t fhost_listing_n(const fhost_listing *l);                           /* partitions found */
int32_t fhost_listing_n_contigs(const fhost_listing *l);
const char *fhost_listing_contig(const fhost_listing *l, int32_t k);       /* name of contig directory k */
const int32_t *fhost_listing_contig_of(const fhost_listing *l);            /* per partition: index of its contig directory */
const int64_t *fhost_listing_tint(const fhost_listing *l);                 /* per partition: the tint id from the file name */
const int64_t *fhost_listing_size(const fhost_listing *l);                 /* per partition: bytes of its split TSV */
int32_t fhost_touch(const char *const *paths, int32_t n, int32_t n_threads);   /* 0 on success */

/* ---- segment_<contig>_<tint>.tsv of the clustering stage -----------------------------------
 * The native form of the reference's read_segment() (py/freddie_cluster.py:119-172, grammar :15-34) up to the rep grouping, which
 * the GPU does (include/freddie_cluster.h, fclu_group_reads): n files are mapped and parsed on at most n_threads threads into flat
 * arrays, the tints in file order, then header order inside a file; a tint's reads in file order.
 * The reader never guesses.  It DECLINES a file (file_declined, with file_line and file_reason) whose lines the grammar does not
 * match, on which an assert of :131-136 or :165-169 would fire, or that holds a read whose tint has no header yet, a number with
 * a leading zero, a number that does not fit (18 digits; 2^30 in the gaps field), a gap key (j1, j2) or a poly-tail key twice
 * in one line, or a line without a newline.  A declined file has no tints in the arrays: the caller runs the Python mirror on it.
 * Names and contigs are views: offset and length into the file's mapping file_map[tint_file[t]], alive until the free call.
 * The key token stream of a read (what besides the I row decides its rep, :155-158): its internal gaps' len > 10 ? len : 0 in
 * line order, then per poly entry 0x80000000 | (key E.: 0x40000000) | (gap > 10 ? gap : 0) in line order. */
typedef struct fhost_segments {
    void *owner;
    int32_t n_file, n_tint;
    int64_t n_read;
    /* per file */
    const int32_t *file_declined;       /* 1: declined */
    const int64_t *file_line;           /* the line (from 1) that declined it, else 0 */
    const char *const *file_reason;     /* "" or why */
    const char *const *file_map;        /* the mapping (NULL: empty or declined) */
    const int64_t *file_tint_off;       /* n_file + 1 */
    /* per tint */
    const int64_t *tint_id;
    const int32_t *tint_file;
    const int64_t *tint_chr_off;
    const int32_t *tint_chr_len;
    const int32_t *n_seg;               /* M_t = positions - 1 */
    const int64_t *pos_off;             /* n_tint + 1 */
    const int64_t *pos;                 /* the segment positions */
    const int64_t *read_off;            /* n_tint + 1 */
    const int64_t *lab_off;             /* n_tint + 1, uint32 words: read r of tint t has its row at lab_off[t] + r * LW_t */
    /* per read */
    const int64_t *rid;
    const uint8_t *strand;              /* '+' or '-' */
    const int64_t *name_off;
    const int32_t *name_len;
    const int64_t *chr_off;
    const int32_t *chr_len;
    const uint32_t *labels;             /* fclu_reads' layout: two bits a label (ASCII & 3), LW_t = max(ceil(M_t / 16), 1) words a row */
    const uint8_t *tail;                /* 0 'N', 1 'S', 2 'E' (:293-304): exactly one poly entry, SA/ST resp. EA/ET, length > 10 */
    const int64_t *gap_off;             /* n_read + 1 */
    const int32_t *gaps;                /* (j1, j2, len) */
    const int64_t *clip_off;            /* n_read + 1 */
    const int32_t *clips;               /* (0 SSC / 1 ESC, len) */
    const int64_t *poly_off;            /* n_read + 1 */
    const int32_t *polys;               /* (0 SA / 1 ST / 2 EA / 3 ET, len, gap) */
    const int64_t *tok_off;             /* n_read + 1 */
    const uint32_t *tok;
} fhost_segments;

/* 0 on success (declined files included); out is zeroed otherwise. */
int32_t fhost_read_segment(const char *const *paths, int32_t n, int32_t n_threads, fhost_segments *out);
void fhost_segments_free(fhost_segments *s);

#ifdef __cplusplus
}
#endif
#endif
