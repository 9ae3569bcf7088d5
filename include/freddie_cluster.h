/*
 * freddie_cluster.h -- C-ABI of the GPU part of the clustering stage's pre-ILP work.
 *
 * It replaces the reference's preprocess_ilp() and partition_reads() (py/freddie_cluster.py:277-328, :196-274):
 *   - per rep, I / C / FL and find_segment_read()      py/freddie_cluster.py:285-310, :175-183   (fclu_preprocess)
 *   - the dedupe of reps with the same structure       py/freddie_cluster.py:203-215             (fclu_preprocess)
 *   - the pairwise read compatibility test            py/freddie_cluster.py:217-234
 *   - the iterated edge pruning of the compatibility graph   py/freddie_cluster.py:240-255
 *   - connected components, the even split of large components and the incompatible rep pairs of every partition
 *                                                      py/freddie_cluster.py:256-274   (fclu_partition)
 * for a batch of transcriptional intervals ("tints") at once.  fclu_partition_reads() runs all of it in one call, from label
 * rows at two bits a label to tint['partitions'] as flat arrays: the unique rows and their members go from the dedupe to
 * the graph on the device.  The entry points behind the dedupe (fclu_compat_graph, fclu_partition) still take unique rows
 * a caller made on the host (freddie_amd/cluster_prep.py: unique_structures(), pack_structures()).  In front of all of it,
 * fclu_group_reads() / fclu_partition_segment() take ALL reads of the tints as the native segment_*.tsv reader leaves them
 * (include/freddie_host.h, fhost_read_segment: label rows, key token streams, tail categories) and group them into reps
 * (read_segment()'s read_reps, :154-164) on the device.  garbage_cost (from the members' counts) and the gaps dicts are host code.
 * The ILP's solve is not here; what run_ilp() builds its model from is: fclu_round_models() (at the end of this header) gives round r of
 * many partitions as flat arrays, from the rows and pair lists the calls above left on the device.  Problems of at most 24 columns need no
 * ILP: fclu_round_exact() enumerates their column sets and returns the proven optimum, and fclu_round_bnb() searches problems of up to 64
 * columns by branch and bound (fclu_round_bnb_wide(): up to 1024, a wave a task).  A round whose problems are answered there needs no model on the host: fclu_round_models_resident() leaves
 * the models on the device, and fclu_round_readout() (the last section) turns the accepted column sets into the round's isoforms -- exon
 * rows and the members' correction strings -- from the rows the context holds.
 *
 * Data layout (caller-owned host arrays, copied by the call):
 *   tint t owns the unique reads row_off[t] .. row_off[t+1]  (N_t of them; "unique" = py/freddie_cluster.py:207-215)
 *   every unique read of tint t is a row of W_t = ceil(M_t / 32) uint32 words at bits[bits_off[t] + r * W_t]:
 *     bit s of the row = I[read][s] (1 = the read covers segment s; label 2 counts as 0, :287-288)
 *   first[r], last[r] = FL[read] (:301), tail[r] = poly_tail_category 'N','S','E' as 0,1,2 (:291-300)
 * Result: for tint t a symmetric N_t x N_t bit matrix, row r at adj[adj_off[t] + r * AW_t], AW_t = ceil(N_t / 64)
 * uint64 words, bit c of the row = the graph has the edge (r, c) after pruning (prune != 0) or before it (prune == 0).
 *
 * fclu_partition() goes on from the pruned matrix without taking it off the device and returns tint['partitions'] of the
 * whole batch as flat arrays (fclu_parts).  The partitions of the batch are numbered through: tint t owns the partitions
 * tint_part_off[t] .. tint_part_off[t+1], in the reference's order (components by their smallest node, a component's
 * chunks in order).  Partition q has
 *   the nodes  part_nodes[part_node_off[q] .. part_node_off[q+1]]     unique-read indices local to the tint, ascending
 *   the rep ids part_rids[part_rid_off[q] .. part_rid_off[q+1]]        tint['partitions'][.][0]: its nodes' members, in order
 *   the pairs  pairs[2 * part_pair_off[q] .. 2 * part_pair_off[q+1]]  tint['partitions'][.][1]: (rid_1, rid_2) two int32 a
 *                                                                     pair, in the reference's loop order (:263-273)
 * and label[r] is the smallest node of the component of unique read r (local to its tint).
 */
#ifndef FREDDIE_CLUSTER_H
#define FREDDIE_CLUSTER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fclu_ctx fclu_ctx;

enum { FCLU_OK = 0, FCLU_ERR_ARG = 1, FCLU_ERR_HIP = 2, FCLU_ERR_UNSUPPORTED = 3 };

int fclu_abi_version(void);
/* One context per device and host thread.  Fails (no CPU fallback) when no HIP device is usable. */
int fclu_create(int device, fclu_ctx **out);
void fclu_destroy(fclu_ctx *c);
const char *fclu_last_error(const fclu_ctx *c);   /* c may be NULL: error of the last failed fclu_create() */

typedef struct fclu_batch {
    int32_t n_tint;
    const int64_t *row_off;    /* n_tint + 1 */
    const int32_t *n_seg;      /* n_tint: M_t */
    const int64_t *bits_off;   /* n_tint + 1, in uint32 words */
    const uint32_t *bits;
    const int32_t *first;      /* row_off[n_tint] */
    const int32_t *last;
    const uint8_t *tail;
    const int64_t *adj_off;    /* n_tint + 1, in uint64 words */
} fclu_batch;

/* Compatibility graph of every tint of the batch.  adj_out: adj_off[n_tint] uint64 words (caller-owned).
 * rounds_out (may be NULL): per tint, the number of pruning passes that removed at least one edge.
 * FCLU_GRID_CAP=<n> (read at every call that launches kernels; tests): the launches whose grid a constant caps take at most n
 * workgroups, so that a small batch runs their grid-stride loops more than once; the results do not depend on it. */
int fclu_compat_graph(fclu_ctx *c, const fclu_batch *b, int32_t prune, uint64_t *adj_out, int32_t *rounds_out);

/* Duration of the kernels of the last fclu_compat_graph() call, from HIP events on the library's stream (ms). */
int fclu_last_timing(fclu_ctx *c, float *compat_ms, float *prune_ms);

/* Launch census of the graph stage: which kernels the last call that built a graph (fclu_compat_graph, fclu_partition,
 * fclu_partition_reads, fclu_partition_segment) launched, as the host decided it.  All zero behind a call that built none
 * (an empty batch, fclu_partition_adj).  The first min(n, FCLU_N_PATHS) values go to out. */
enum {
    FCLU_PATH_COMPAT_FORM = 0,      /* k_compat: FCLU_FORM_RANK (rank tables) or FCLU_FORM_MASKED (a range mask per word) */
    FCLU_PATH_TILES = 1,            /* 64 x 64 tiles on and above the diagonals, all tints */
    FCLU_PATH_LDS_TINTS = 2,        /* tints pruned whole by one workgroup (k_prune_lds); 0 without pruning */
    FCLU_PATH_PASS_KERNEL = 3,      /* the per-pass kernels: 0 not launched, FCLU_PASS_EDGE_WALK (k_prune_edges) or
                                       FCLU_PASS_OR_OF_ROWS (k_deg1 + k_prune) */
    FCLU_PATH_EDGE_CHUNKS = 4,      /* k_prune_edges: 64-word chunks of the longest adjacency row it takes; 0 otherwise */
    FCLU_PATH_PASSES_ENQUEUED = 5,  /* per-pass launches enqueued (whole bursts) */
    FCLU_PATH_PASSES_RAN = 6,       /* of those, the passes that ran: up to and with the first that removed nothing */
    /* the read-out's words: those of the last fclu_round_readout() call (zero behind a refused one, and behind a later graph call) */
    FCLU_PATH_READOUT_SETS = 7,     /* problems with a set: the workgroups of k_readout_exons */
    FCLU_PATH_READOUT_MEMBERS = 8,  /* members over all sets: the rows k_readout_corr wrote */
    FCLU_PATH_READOUT_STORES = 9,   /* FCLU_STORE_WIDE: some lane stores 16 bytes at once; FCLU_STORE_BYTES: some byte is stored alone -- as the host
                                       predicts it from the rows' addresses by the kernel's rule (clu_readout.h, ro_store_halves); the kernel reports
                                       nothing, so the word says which paths the batch calls for, not that they ran */
    FCLU_N_PATHS = 10
};
enum { FCLU_FORM_RANK = 1, FCLU_FORM_MASKED = 2 };
enum { FCLU_PASS_EDGE_WALK = 1, FCLU_PASS_OR_OF_ROWS = 2 };
enum { FCLU_STORE_WIDE = 1, FCLU_STORE_BYTES = 2 };
int fclu_last_paths(fclu_ctx *c, int32_t *out, int32_t n);

/* ---- the rest of partition_reads(): components, even split, members and incompatible pairs (:256-274) ----
 * mem_off: int64[row_off[n_tint] + 1], starts at 0 and never falls; mem[mem_off[r] .. mem_off[r+1]] = the rep ids of
 * unique read r (unique_data[r][1]).  maximum_ilp_size >= 1.
 * FCLU_ERR_UNSUPPORTED: the batch's pair list has more than 2^31 - 1 pairs or does not fit the device's free memory
 * (fclu_last_error names the total); a caller splits the batch. */
int fclu_partition(fclu_ctx *c, const fclu_batch *b, const int64_t *mem_off, const int32_t *mem, int32_t maximum_ilp_size);

/* The same behind a graph of the caller's, in the layout fclu_compat_graph() writes (row_off, adj_off: n_tint + 1).  The
 * matrix must be symmetric with an empty diagonal and no bit at a column >= N_t: FCLU_ERR_ARG otherwise. */
int fclu_partition_adj(fclu_ctx *c, int32_t n_tint, const int64_t *row_off, const int64_t *adj_off, const uint64_t *adj,
                       const int64_t *mem_off, const int32_t *mem, int32_t maximum_ilp_size);

typedef struct fclu_parts {
    int32_t n_tint;
    int64_t n_rows, n_part, n_rids, n_pairs;   /* lengths: label / part_nodes, partitions, part_rids, pairs (in pairs) */
    const int64_t *tint_part_off;              /* n_tint + 1 */
    const int64_t *part_node_off;              /* n_part + 1 */
    const int32_t *part_nodes;                 /* n_rows */
    const int64_t *part_rid_off;               /* n_part + 1 */
    const int32_t *part_rids;                  /* n_rids */
    const int64_t *part_pair_off;              /* n_part + 1, counted in pairs */
    const int32_t *pairs;                      /* 2 * n_pairs */
    const int32_t *label;                      /* n_rows */
} fclu_parts;

/* Result of the last successful fclu_partition() / fclu_partition_adj(): pointers into pinned host buffers the context
 * owns, valid until the context's next call. */
int fclu_partition_results(fclu_ctx *c, fclu_parts *out);

/* Kernel time of the last partition call behind the graph, from HIP events (ms): the components; the pair count + emit
 * (with the members' copy).  The graph's own time is fclu_last_timing()'s. */
int fclu_partition_timing(fclu_ctx *c, float *components_ms, float *pairs_ms);

/* ---- the front: preprocess_ilp() per rep and the dedupe, from label rows (:277-328, :203-215) ----
 * Caller-owned host arrays, copied by the call. */
typedef struct fclu_reads {
    int32_t n_tint;
    const int64_t *rep_off;    /* n_tint + 1: tint t owns the reps rep_off[t] .. rep_off[t+1], in read_reps order */
    const int32_t *n_seg;      /* n_tint: M_t */
    const int64_t *lab_off;    /* n_tint + 1, in uint32 words; a rep's row is LW_t = max(ceil(M_t / 16), 1) words */
    const uint32_t *labels;    /* label s of a row at bits 2 * (s & 15) of word s >> 4; code = ASCII & 3 (0, 1, 2); the bits
                                  beyond M_t are zero */
    const uint8_t *tail;       /* per rep: 0 'N', 1 'S', 2 'E' -- the category of :293-304, decided by the host from the
                                  parsed poly_tail dict (exactly one entry, key SA/ST resp. EA/ET, length > 10) */
} fclu_reads;

/* Per rep: I (label & 1; 2 counts as 0) and C (label 0 inside [max(first, 0), last]) as bit rows of W_t = max(ceil(M_t / 32), 1)
 * uint32 words, raw_first / raw_last (find_segment_read: (-1, M_t - 1) for a row without a 1), first / last (FL: the raw values,
 * first = 0 for tail 'S', last = M_t - 1 for tail 'E').  Reps of a tint with equal (I row, first, last, tail) are one unique row
 * ("node"); nodes are numbered by their smallest rep, a node's members are its reps, ascending.  The hash that buckets the rows
 * never decides: equality is tested on the whole row.
 * FCLU_ERR_ARG (fclu_last_error names tint and rep): a label 3, a nonzero bit beyond M_t, a tail above 2, lab_off that is not
 * reps x LW_t, negative counts, an empty batch.  FCLU_ERR_UNSUPPORTED: more than 9600 segments.  The context stays usable.
 * FCLU_HASH_BITS=<n> (read at the call; tests): the hash cut to n bits, 0 = one bucket a tint. */
int fclu_preprocess(fclu_ctx *c, const fclu_reads *reads);

typedef struct fclu_prep {
    int32_t n_tint;
    int64_t n_reps, n_rows;                    /* reps and unique rows of the batch */
    const int64_t *row_off, *bits_off, *adj_off;   /* n_tint + 1 each: the unique rows as a fclu_batch */
    const int64_t *rep_bits_off;               /* n_tint + 1, uint32 words: rep i of tint t has its I / C row at rep_bits_off[t] + i * W_t */
    const uint32_t *i_bits, *c_bits;           /* rep_bits_off[n_tint] */
    const int32_t *first, *last;               /* n_reps: FL */
    const int32_t *raw_first, *raw_last;       /* n_reps: find_segment_read() */
    const int32_t *rep_node;                   /* n_reps: the rep's node, local to the tint */
    const int32_t *node_rep;                   /* n_rows: the node's smallest rep, local to the tint */
    const int64_t *mem_off;                    /* n_rows + 1 */
    const int32_t *mem;                        /* n_reps: the nodes' members (rep ids local to the tint), fclu_partition's mem */
    const uint32_t *bits;                      /* bits_off[n_tint]: the nodes' rows, fclu_batch's bits */
    const int32_t *node_first, *node_last;     /* n_rows: fclu_batch's first / last */
    const uint8_t *node_tail;                  /* n_rows: fclu_batch's tail */
} fclu_prep;

/* Result of the last successful fclu_preprocess() / fclu_partition_reads(): pointers into pinned host buffers the context
 * owns, valid until the context's next call. */
int fclu_preprocess_results(fclu_ctx *c, fclu_prep *out);

/* preprocess, dedupe, compatibility graph, pruning and partition in one call; fclu_partition_results() and
 * fclu_preprocess_results() hold the results.  Refusals: fclu_preprocess()'s and fclu_partition()'s. */
int fclu_partition_reads(fclu_ctx *c, const fclu_reads *reads, int32_t maximum_ilp_size);

/* Kernel time of the last fclu_preprocess() / fclu_partition_reads() from HIP events (ms): the per-rep rows; the dedupe
 * (sorts, scans, leaders, nodes and members). */
int fclu_preprocess_timing(fclu_ctx *c, float *rows_ms, float *dedupe_ms);

/* ---- in front of the front: read_segment()'s grouping of reads into reps (:154-164) ----
 * ALL reads of every tint, as the native reader leaves them (include/freddie_host.h, fhost_read_segment).  Caller-owned host
 * arrays, copied by the call. */
typedef struct fclu_segment {
    int32_t n_tint;
    const int64_t *read_off;   /* n_tint + 1: tint t owns the reads read_off[t] .. read_off[t+1], in file order */
    const int32_t *n_seg;      /* n_tint: M_t */
    const int64_t *lab_off;    /* n_tint + 1, uint32 words; a read's row is LW_t words, in fclu_reads' layout */
    const uint32_t *labels;
    const int64_t *tok_off;    /* reads + 1: a read's key token stream, tok[tok_off[r] .. tok_off[r+1]] */
    const uint32_t *tok;
    const uint8_t *tail;       /* per read: 0 'N', 1 'S', 2 'E' */
} fclu_segment;

/* Two reads of a tint share a rep exactly when their I rows (label & 1; 2 counts as 0) and their token streams are equal.  Reps are
 * numbered by their first read (Python's dict insertion order), a rep's members are its reads, ascending.  The hash that buckets
 * the reads never decides (FCLU_HASH_BITS cuts it too).  Refusals as fclu_preprocess's, naming tint and read, and tok_off that
 * does not start at 0 or falls.  The context stays usable. */
int fclu_group_reads(fclu_ctx *c, const fclu_segment *in);

/* grouping, preprocess (a rep's row and tail are its FIRST read's), dedupe, graph, pruning and partition in one call: after the
 * upload everything stays on the device.  fclu_group_results(), fclu_preprocess_results() and fclu_partition_results() hold the
 * results, the latter two as after fclu_partition_reads() on the reps.  Refusals: fclu_group_reads()'s and fclu_partition()'s. */
int fclu_partition_segment(fclu_ctx *c, const fclu_segment *in, int32_t maximum_ilp_size);

typedef struct fclu_groups {
    int32_t n_tint;
    int64_t n_reads, n_reps;
    const int64_t *rep_off;        /* n_tint + 1: tint t owns the reps rep_off[t] .. rep_off[t+1] */
    const int32_t *read_rep;       /* n_reads: the read's rep, local to the tint */
    const int64_t *rep_mem_off;    /* n_reps + 1 */
    const int32_t *rep_mem;        /* n_reads: read_reps[i], read indices local to the tint, ascending; len(read_reps[i]) is
                                      rep_mem_off's difference (garbage_cost) */
    const int32_t *rep_first;      /* n_reps: read_reps[i][0] */
} fclu_groups;

/* Result of the last successful fclu_group_reads() / fclu_partition_segment(): pointers into pinned host buffers the context
 * owns, valid until the context's next call. */
int fclu_group_results(fclu_ctx *c, fclu_groups *out);

/* Kernel time of the grouping of the last such call from HIP events (ms): the keys; sorts, scans, leaders and members, and in
 * fclu_partition_segment() the gather of the reps' rows and tails into the preprocess stage's device arrays (fclu_group_reads()
 * does not gather, and leaves those arrays alone). */
int fclu_group_timing(fclu_ctx *c, float *keys_ms, float *dedupe_ms);

/* ---- a round's ILP models as arrays: informative_segs() (:331-344) and what run_ilp() builds from (:397-535), K = 2 ----
 * The source is what the context's last fclu_partition_reads() / fclu_partition_segment() left on the device (the reps' I and C rows,
 * the partitions' pair lists); a call that overwrites them in between (fclu_preprocess, fclu_partition, fclu_partition_adj,
 * fclu_group_reads) ends that, and fclu_round_setup() then refuses; fclu_compat_graph() leaves them alone.
 * fclu_round_setup(), once per batch of tints: rep r of the batch (rep_off[t] + i) has the gaps gaps[3 * gap_off[r] .. 3 * gap_off[r + 1]),
 * triples (j1, j2, l) in the order of the rep's first read's gaps dict as preprocess_ilp() leaves it, the pseudo-gaps (-1, first) /
 * (last, M) of :299 / :303 included (-1 <= j1 <= j2 <= M_t, j1 < M_t, M_t >= 1: FCLU_ERR_ARG otherwise; a rep without a 1 has first = -1); segment j of tint t is seg_len[seg_off[t] + j]
 * long.  Caller-owned host arrays, copied by the call. */
int fclu_round_setup(fclu_ctx *c, const int64_t *gap_off, const int32_t *gaps, const int64_t *seg_off, const int32_t *seg_len);

/* A batch of problems: problem p is partition part[p] (numbered through the batch, as in fclu_parts) with the remaining reps
 * rids[rid_off[p] .. rid_off[p + 1]) (local to the tint) in the caller's order; "column" = a rep's position in that list.
 * FCLU_ERR_ARG, naming problem and column: a partition twice in the batch, a rep outside its tint, outside the partition or twice in
 * the problem.  The context stays usable. */
typedef struct fclu_round_batch {
    int32_t n_prob;
    const int64_t *part;       /* n_prob */
    const int64_t *rid_off;    /* n_prob + 1 */
    const int32_t *rids;
} fclu_round_batch;

int fclu_round_models(fclu_ctx *c, const fclu_round_batch *b);

/* Every order is fixed.  Integers only: (1 +- epsilon), the offset and MAX_ISOFORM_LG are the host's. */
typedef struct fclu_rounds {
    int32_t n_prob;
    int64_t n_cols, n_inf, n_sup, n_corr, n_pairs, n_grp, n_grp_seg, n_gap_rows;
    const int32_t *refused;        /* n_prob: -1, or the smallest column with a gap (j1, j2) whose informative[j1 % M] or informative[j2 % M]
                                      is false -- the reference's asserts :467-468; the arrays of such a problem are not a model */
    const int64_t *inf_bits_off;   /* n_prob + 1, uint32 words: problem p's informative row, W_t words, bit j = informative[j] */
    const uint32_t *inf_bits;
    const int64_t *inf_off;        /* n_prob + 1: problem p's informative segments inf_seg[inf_off[p] .. inf_off[p + 1]), ascending */
    const int32_t *inf_seg;        /* n_inf */
    const int64_t *sup_off;        /* n_inf + 1: beside inf_seg; the columns with I = 1 at that segment, ascending */
    const int32_t *sup_cols;       /* n_sup */
    const int64_t *col_off;        /* n_prob + 1: = rid_off */
    const int64_t *corr_off;       /* n_cols + 1: per column the informative j with C = 1, ascending (OBJ[i][j][1], :522-535) */
    const int32_t *corr_seg;       /* n_corr */
    const int64_t *pair_off;       /* n_prob + 1, in pairs */
    const int32_t *pairs;          /* 2 * n_pairs: the partition's pairs with both ends remaining, as columns, in the partition's order */
    const int64_t *grp_off;        /* n_prob + 1: the problem's gap groups, the distinct (j1, j2) of its columns' gaps, ascending */
    const int32_t *grp;            /* 2 * n_grp: j1, j2 */
    const int64_t *grp_seg_off;    /* n_grp + 1: the group's informative segments strictly between j1 and j2, ascending (GAPI_C1) */
    const int32_t *grp_seg, *grp_len;   /* n_grp_seg: segment, its length */
    const int64_t *row_off;        /* n_prob + 1: the problem's (column, gap) rows, in column order then the rep's own gap order */
    const int32_t *rows;           /* 3 * n_gap_rows: column, group (local to the problem), l (GAPR_C1 / GAPR_C2) */
} fclu_rounds;

/* Result of the last successful fclu_round_models(): pointers into pinned host buffers the context owns, valid until the context's
 * next call.  The partition and preprocess results stay valid behind a round call. */
int fclu_round_results(fclu_ctx *c, fclu_rounds *out);

/* The same call with the models left on the device: the same kernels and the same device arrays, so that fclu_round_incumbents(),
 * fclu_round_exact(), fclu_round_bnb() and fclu_round_readout() run behind it unchanged, and only the small per-problem arrays come to the
 * host.  fclu_round_results() behind it fills n_prob, the counts, refused, col_off, inf_bits_off and inf_bits and leaves every other pointer
 * null.  Refusals as fclu_round_models'. */
int fclu_round_models_resident(fclu_ctx *c, const fclu_round_batch *b);

/* Kernel time of the last fclu_round_models() from HIP events (ms): column reduction, informative rows and counts with their scan; the
 * gap groups (keys, sort, groups); the fills. */
int fclu_round_timing(fclu_ctx *c, float *count_ms, float *gaps_ms, float *fill_ms);

/* ---- greedy incumbents of a round's problems: a feasible column set per problem, as cutoff and fallback of the solve ----
 * With K = 2 a round's model is a function of the chosen column set S alone: e = the OR of the members' I rows on the informative
 * segments, cost = sum over S of popcount(C_c & e) + the others' garbage costs, no incompatible pair inside S, every gap row of a member
 * holding.  Per problem, min(R, max_seeds) seeded starts (start k = {floor(k R / n)}) and the empty start are grown greedily (the column
 * with the smallest delta2, then the smallest column, while delta2 < 0), repaired (while a member has a violated gap row, the member with
 * the most, then the smallest column, leaves) and scored; the smallest cost2, then the earliest start, is the incumbent.  A start that
 * leaves a gap row of a column OUTSIDE the set violated (the model gives such a row MAX_ISOFORM_LG -- the tint's summed segment lengths,
 * from fclu_round_setup's seg_len -- of slack and no more: the same test with offset + MAX_ISOFORM_LG for offset) is not feasible and is
 * left out; a problem without a feasible start has no incumbent.  The definition, every tie included, is freddie_amd/cluster_solve.py
 * greedy_incumbent(), which the device reproduces exactly.
 * The batch is that of the context's last successful fclu_round_models(), whose device arrays are the input; g2[n_cols] = twice each
 * column's garbage cost (>= 0); a member's row (g, l) is violated when lo_f * G_g - offset > l or hi_f * G_g + offset < l in doubles (one
 * rounded multiply, one rounded add, no fused multiply-add), lo_f = 1 - epsilon and hi_f = 1 + epsilon being the host's; max_seeds >= 1.
 * FCLU_ERR_ARG: no such fclu_round_models() behind the call, the rounds' source ended by a later call (see above), a bad argument.
 * FCLU_ERR_UNSUPPORTED: a problem of more than 32768 columns; conflict matrices (the sum of R^2 bits) beyond the device's free memory
 * (fclu_last_error names the total).  The context stays usable.  FCLU_ROUND_LDS / FCLU_ROUND_LDS_BYTES split the problems as they do
 * for fclu_round_models(). */
int fclu_round_incumbents(fclu_ctx *c, const int32_t *g2, double lo_f, double hi_f, int32_t offset, int32_t max_seeds);

typedef struct fclu_incumbents {
    int32_t n_prob;
    int64_t n_mem;
    const int64_t *cost2;          /* n_prob: twice the incumbent's cost; -1 for a refused problem (no model: skipped) and for one without a feasible start */
    const int32_t *start;          /* n_prob: the chosen start (min(R, max_seeds) = the empty one); -1 where cost2 is */
    const int32_t *grow_steps, *repair_steps;   /* n_prob: columns the chosen start added / members it lost */
    const int64_t *mem_off;        /* n_prob + 1 */
    const int32_t *mem;            /* n_mem: the members (columns), ascending */
} fclu_incumbents;

/* Result of the last successful fclu_round_incumbents(): pointers into pinned host buffers the context owns, valid until the context's
 * next call.  The round results stay valid behind it. */
int fclu_round_incumbent_results(fclu_ctx *c, fclu_incumbents *out);

/* Kernel time of the last fclu_round_incumbents() from HIP events (ms): the conflict matrices; the starts (grow, repair, score); the choice. */
int fclu_round_incumbent_timing(fclu_ctx *c, float *conflict_ms, float *starts_ms, float *pick_ms);

/* ---- the exact solve of a round's small problems: a proven optimum per problem by enumeration, with no matrix and no solver ----
 * The model is the one above (a function of the chosen column set S alone); a problem of R columns has 2^R sets, masks 0 .. 2^R - 1 with
 * bit c = column c.  S is feasible when no incompatible pair lies inside it and every gap row (c, g, l) of the problem holds: with G_g = the
 * summed lengths of group g's segments whose support meets S and slack = 0 when c is in S, else MAX_ISOFORM_LG, the row is violated when
 *   lo_f * G_g - offset - slack > l + 1e-9   or   hi_f * G_g + offset + slack < l - 1e-9
 * in doubles, every operation rounded on its own, in this order, none fused.  The tolerance is the model's (a proven optimum must not
 * exclude what the rows admit: with epsilon 0.15, offset 20, G = 200 the row l = 250 holds with equality, and 1.15 * 200 + 20 < 250 in
 * doubles); the incumbents above have none, because an incumbent must be feasible for everybody.  cost2 = the g2 of the columns outside S +
 * twice the members' corrections on the segments some member covers; the smallest cost2 wins, then the smallest mask.  The definition is
 * freddie_amd/cluster_solve.py exact_small(), which the device reproduces exactly.
 * Input as fclu_round_incumbents': the device arrays of the context's last successful fclu_round_models(), g2[n_cols] >= 0 (below 2^31; a
 * problem's cost2 stays below 2^36), lo_f, hi_f, offset.  A problem is taken when it has a model (is not refused), has at most max_cols
 * columns and fits the budget: the problems are taken in ascending (columns, problem index) while the running total of 2^R stays
 * <= max_masks, a choice the host makes.  The call is cut into launches of a bounded number of masks, so that no single launch runs long.
 * FCLU_ERR_ARG: fclu_round_incumbents' cases; max_cols outside [0, 24]; max_masks < 1.  FCLU_ERR_UNSUPPORTED: a budget that needs more
 * than 4096 launches.  The context stays usable.  FCLU_EXACT_SLICE=<masks> (read at the call; tests): fewer masks a workgroup and a
 * launch, so that a 12-column problem crosses many slices and several launches. */
int fclu_round_exact(fclu_ctx *c, const int32_t *g2, double lo_f, double hi_f, int32_t offset, int32_t max_cols, int64_t max_masks);

typedef struct fclu_exact {
    int32_t n_prob;
    const int64_t *cost2;          /* n_prob: twice the optimum's cost; -1 when no column set is feasible; -2 when the problem was not taken or is refused */
    const uint32_t *mask;          /* n_prob: the optimal column set, bit c = column c; 0 where cost2 < 0 */
    int64_t n_taken;               /* problems taken */
    int64_t n_masks;               /* masks evaluated: the sum of 2^R over the taken problems */
    int64_t n_launches;            /* search launches issued (the one launch that transposes the models is not counted) */
} fclu_exact;

/* Result of the last successful fclu_round_exact(): pointers into pinned host buffers the context owns, valid until the context's next
 * call.  The round results and the incumbents' results stay valid behind it. */
int fclu_round_exact_results(fclu_ctx *c, fclu_exact *out);

/* Kernel time of the last fclu_round_exact() from HIP events (ms): the transposed tables; all search launches; the longest of them. */
int fclu_round_exact_timing(fclu_ctx *c, float *prep_ms, float *search_ms, float *longest_launch_ms);

/* ---- branch and bound over a round's larger problems: a proven optimum of a problem of up to 64 columns where the search finishes ----
 * The model and the rule of the result are fclu_round_exact's: S feasible by the same test, the smallest cost2, then the smallest mask
 * (64 bits, bit c = column c).  D = min(R, depth); task t of a problem's 2^D fixes columns 0 .. D - 1 (bit c of t = column c is in) and is
 * searched depth first over the columns D .. R - 1, the include child first where the column conflicts with no member, then the exclude
 * child.  A node (columns 0 .. d - 1 fixed, S of them in) is dropped when its lower bound exceeds the task's best cost2 so far --
 *   LB2 = the g2 of the columns fixed out + 2 * the members' corrections on the segments some member covers (e_in)
 *         + over the columns c >= d: g2_c when c conflicts with a member, else min(g2_c, 2 * c's corrections on e_in),
 * strictly, so that every set of optimal cost is reached -- or when a member's row is violated from below already
 * (lo_f * G - offset > l + 1e-9, the doubles of the row test above; G only grows).  A leaf (d = R) is tested by the whole test above.  A
 * task's best starts at ub2[p] (>= 0: a bound, e.g. the incumbent's cost2, which a leaf may equal; < 0: none).  Every child evaluated
 * counts one node, the prefix one; a task whose count has reached node_cap when it wants another child stops and is capped, and its best
 * leaf still counts.  Tasks share nothing, so the result, node counts included, is a function of the arguments.  The definition is
 * freddie_amd/cluster_solve.py exact_bnb(), which the device reproduces exactly; what a lane computes is freddie_amd/csrc/clu_bnb.h.
 * Input as fclu_round_exact's, and ub2[n_prob].  A problem is taken when it has a model, min_cols <= R <= max_cols <= 64, its tables fit
 * one workgroup's LDS (160 KiB: 16 bytes an informative segment and 12 a column, 10 192 informative segments; a row holds 9 600 at the
 * most, so every model fits) and it fits the budget: ascending (columns, problem index) while the running total of 2^D * node_cap stays
 * <= max_nodes, a choice the host makes.  A launch holds at most 2^24 task-nodes of budget (tasks * node_cap; at least one task).
 * FCLU_ERR_ARG: fclu_round_exact's cases; ub2 null with problems; min_cols < 0, max_cols < min_cols or > 64; depth outside [0, 20];
 * node_cap < 1; max_nodes < 1.  FCLU_ERR_UNSUPPORTED: a budget that needs more than 4096 launches.  The context stays usable.
 * FCLU_BNB_SLICE=<tasks> (read at the call; tests): a launch holds that many tasks. */
int fclu_round_bnb(fclu_ctx *c, const int32_t *g2, const int64_t *ub2, double lo_f, double hi_f, int32_t offset, int32_t min_cols, int32_t max_cols,
                   int32_t depth, int32_t node_cap, int64_t max_nodes);

#define FCLU_BNB_OPTIMAL 0
#define FCLU_BNB_INFEASIBLE 1
#define FCLU_BNB_UNPROVEN 2
#define FCLU_BNB_NOT_TAKEN (-2)

typedef struct fclu_bnb {
    int32_t n_prob;
    const int32_t *status;         /* n_prob: 0 optimal (no task capped, a leaf at or under the bound); 1 infeasible (no task capped, no leaf, no bound);
                                      2 unproven (a task capped, or a bound and no leaf under it); -2 not taken or refused */
    const int64_t *cost2;          /* n_prob: twice the cost of the best set found; -1 where there is none */
    const uint64_t *mask;          /* n_prob: that set, bit c = column c; 0 where cost2 < 0 */
    const int64_t *nodes;          /* n_prob: nodes counted over the problem's tasks; 0 where it was not taken */
    const int32_t *capped;         /* n_prob: tasks that stopped at node_cap */
    int64_t n_taken;               /* problems taken */
    int64_t n_launches;            /* search launches issued */
    int64_t nodes_total;           /* the taken problems' nodes summed */
} fclu_bnb;

/* Result of the last successful fclu_round_bnb(): pointers into pinned host buffers the context owns, valid until the context's next
 * call.  The round's, the incumbents' and the exact call's results stay valid behind it. */
int fclu_round_bnb_results(fclu_ctx *c, fclu_bnb *out);

/* Kernel time of the last fclu_round_bnb() from HIP events (ms): the tables; all search launches; the longest of them. */
int fclu_round_bnb_timing(fclu_ctx *c, float *prep_ms, float *search_ms, float *longest_launch_ms);

/* ---- the same search for problems of up to 1024 columns ----
 * fclu_round_bnb()'s search, word for word (the definition is freddie_amd/cluster_solve.py exact_bnb_wide(), which the device reproduces
 * exactly, node counts included), on column sets of W = ceil(R / 64) words: a wave runs one task and its 64 lanes share the work inside
 * a node (freddie_amd/csrc/clu_bnb_wide.h).  Input as fclu_round_bnb's.  A problem is taken when it has a model, min_cols <= R <=
 * max_cols <= 1024, its tables fit one workgroup's LDS -- bw_lds_bytes(R, E) of clu_bnb_wide.h, 16 R ceil(E / 64) + 4 R + 64 (9 W + 2
 * ceil(E / 64)) bytes rounded up to 16, at most 160 KiB -- and it fits the budget: ascending (columns, problem index) while the running
 * total of 2^D * node_cap stays <= max_nodes.  A launch holds at most 2^26 task-nodes of budget (tasks * node_cap; at least one task).
 * FCLU_ERR_ARG: fclu_round_bnb's cases with 1024 for 64, all refused on the host before any launch.  FCLU_ERR_UNSUPPORTED: a budget that
 * needs more than 4096 launches.  The context stays usable.  FCLU_BNB_WIDE_SLICE=<tasks> (read at the call; tests): a launch holds that
 * many tasks. */
int fclu_round_bnb_wide(fclu_ctx *c, const int32_t *g2, const int64_t *ub2, double lo_f, double hi_f, int32_t offset, int32_t min_cols, int32_t max_cols,
                        int32_t depth, int32_t node_cap, int64_t max_nodes);

#define FCLU_BNB_WIDE_WORDS 16

typedef struct fclu_bnb_wide {
    int32_t n_prob;
    const int32_t *status;         /* n_prob: as fclu_bnb's */
    const int64_t *cost2;          /* n_prob: twice the cost of the best set found; -1 where there is none */
    const uint64_t *mask;          /* 16 n_prob: that set, 16 words a problem, low word first, bit c & 63 of word c >> 6 = column c; 0 where cost2 < 0 */
    const int64_t *nodes;          /* n_prob: nodes counted over the problem's tasks; 0 where it was not taken */
    const int32_t *capped;         /* n_prob: tasks that stopped at node_cap */
    int64_t n_taken;               /* problems taken */
    int64_t n_launches;            /* search launches issued */
    int64_t nodes_total;           /* the taken problems' nodes summed */
} fclu_bnb_wide;

/* Result of the last successful fclu_round_bnb_wide(): pointers into pinned host buffers the context owns, valid until the context's
 * next call.  The round's, the incumbents', the exact call's and fclu_round_bnb's results stay valid behind it. */
int fclu_round_bnb_wide_results(fclu_ctx *c, fclu_bnb_wide *out);

/* Kernel time of the last fclu_round_bnb_wide() or fclu_round_bnb_wide_passes() from HIP events (ms): the tables and the later passes'
 * records; all search launches of all passes; the longest of them. */
int fclu_round_bnb_wide_timing(fclu_ctx *c, float *prep_ms, float *search_ms, float *longest_launch_ms);

/* ---- the same search continued: a capped task's open subtrees become the tasks of a further pass ----
 * fclu_round_bnb_wide() with up to `passes` passes (the definition is freddie_amd/cluster_solve.py exact_bnb_wide(passes=...), which the
 * device reproduces exactly, node counts included).  Pass 1 is fclu_round_bnb_wide's search.  A task that stops at node_cap leaves its
 * stack; every level of it whose exclude child was not tried, and the child it stopped in front of, is an open subtree.  Pass k + 1 runs
 * the open subtrees of pass k's capped tasks as tasks of their own, node_cap nodes each at the most, every one bounded by the smaller of
 * ub2 and the best cost2 any task of the problem found in the passes before.  Before a pass the host reads the per-problem numbers of
 * open subtrees back (the one read-back of a pass) and takes the problems of the pass before in their order -- ascending (columns, problem
 * index) -- while the running total of tasks * node_cap stays <= max_nodes; the first problem that does not fit ends the taking: it and
 * every problem behind it are not continued in this or a later pass.  A problem whose next pass would hold more than 2^16 tasks is not
 * continued either.  The call ends when no problem is continued or after `passes` passes.  A problem's result is the smallest (cost2,
 * set) over all its tasks of all passes, its nodes are summed over the passes and `capped` counts the tasks still open, that is the capped
 * tasks of the last pass it took part in; the status follows fclu_bnb's rule with those.  Results: fclu_round_bnb_wide_results(), whose
 * layout is unchanged; n_launches counts the search launches of all passes.  passes == 1 equals fclu_round_bnb_wide() in every result
 * word.  FCLU_ERR_ARG: fclu_round_bnb_wide's cases, and passes outside [1, 16].  FCLU_BNB_WIDE_SLICE applies to every pass. */
int fclu_round_bnb_wide_passes(fclu_ctx *c, const int32_t *g2, const int64_t *ub2, double lo_f, double hi_f, int32_t offset, int32_t min_cols, int32_t max_cols,
                               int32_t depth, int32_t node_cap, int64_t max_nodes, int32_t passes);

#define FCLU_BNB_WIDE_PASS_STATS 5

/* The passes of the last successful fclu_round_bnb_wide() / fclu_round_bnb_wide_passes(): out has room for n rows of
 * FCLU_BNB_WIDE_PASS_STATS int64 -- a pass's tasks, their nodes, the capped ones, the search launches, the problems that took part --
 * row k for pass k + 1; the rows of passes that did not run are zero (a pass that ran has at least one task). */
int fclu_round_bnb_wide_pass_stats(fclu_ctx *c, int64_t *out, int32_t n);

/* ---- the read-out of a round: run_ilp()'s isoform (:601-635) of every problem with an accepted column set, on the device ----
 * The batch is that of the context's last successful fclu_round_models() / fclu_round_models_resident().  Problem p's accepted columns are
 * sel[sel_off[p] .. sel_off[p + 1]), ascending; an empty range means "no isoform this round" and gives empty outputs.  Any number of
 * columns: the sets are lists, so a solver's answer goes through the same call as a mask of fclu_round_exact / fclu_round_bnb.
 * Per problem with a set, M_t = the tint's segments:
 *   exons  M_t bytes 0 / 1: on an informative segment the OR of the members' I bits, elsewhere the I bit of column 0 of the problem (the
 *          first remaining rep, member or not)
 *   corr   M_t ASCII bytes per member, in set order: '-' on an uninformative segment, 'X' where the member's C bit and the exon bit are 1,
 *          otherwise the label '0', '1' or '2' of the rep's row (its first read's)
 *   e      the exon values at the problem's informative segments, ascending (what a solver returns beside x)
 * The definition is freddie_amd/cluster.py read_out(); what a lane computes is freddie_amd/csrc/clu_readout.h.
 * FCLU_ERR_ARG, naming problem and column: a column outside the problem, a set that is not strictly ascending, a set for a refused problem,
 * sel_off that does not start at 0 or falls, no such round behind the call.  Every refusal is made before a kernel is launched; the context
 * stays usable, and the round's results stay valid behind the call. */
int fclu_round_readout(fclu_ctx *c, const int64_t *sel_off, const int32_t *sel);

typedef struct fclu_readout {
    int32_t n_prob;
    int64_t n_sets, n_mem, n_exon_bytes, n_corr_bytes, n_e;   /* problems with a set, members, lengths of exons, corr and e */
    const int64_t *exon_off;       /* n_prob + 1, bytes: problem p's exon row (M_t bytes, or none) */
    const uint8_t *exons;
    const int64_t *mem_off;        /* n_prob + 1: = sel_off */
    const int64_t *corr_off;       /* n_prob + 1, bytes: member k of problem p has its row at corr_off[p] + k * M_t */
    const uint8_t *corr;
    const int64_t *e_off;          /* n_prob + 1 */
    const uint8_t *e;
} fclu_readout;

/* Result of the last successful fclu_round_readout(): pointers into pinned host buffers the context owns, valid until the context's next
 * call. */
int fclu_round_readout_results(fclu_ctx *c, fclu_readout *out);

/* Kernel time of the last fclu_round_readout() from HIP events (ms): the exon rows with e; the corrections. */
int fclu_round_readout_timing(fclu_ctx *c, float *exons_ms, float *corr_ms);

#ifdef __cplusplus
}
#endif
#endif
