/* merge_gpu.h -- interface between merge.c (host: layouts, label universe, pass plan, label numbering, file assembly) and
 * merge_kernels.hip (device: decode, stable sort, replay, compaction, packing).  Private. */
#ifndef UTREE_MERGE_GPU_H
#define UTREE_MERGE_GPU_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* what h_u_of_ix holds for a label line the edit drops (utree_merge_files_edit); universe ids stay below it (n_u < 2^24) */
#define UTK_MERGE_DROP 0xFFFFFFu

typedef struct {
    const char *h_ublob; uint64_t ublob_bytes;              /* universe: every input label and every ';'-prefix of one, NUL-terminated */
    const uint64_t *h_uoff; uint32_t n_u;
    const uint32_t *h_trunc_off;                            /* [n_u + 1]                                                    */
    const uint32_t *h_trunc_ids; uint32_t n_trunc;          /* trunc_ids[trunc_off[u] + m - 1] = u cut before its m-th ';'  */
    uint32_t n_in;
    const uint32_t *const *h_u_of_ix;                       /* [n_in][n_lines[i]]: universe id of input i's label index     */
    const uint32_t *n_lines;
    uint32_t W, I_out;
    int gg, device, any_ctr;
    int has_minus;                                          /* some slice is a MINUS input's: which records are fed is known only after the sort, so
                                                               the fold dates the labels of the records it feeds, not the decode */
    uint64_t cap_nodes;                                     /* nodes of the largest pass                                    */
    uint64_t cap_raw;                                       /* bytes of the largest pass's records as utk_merge_slice lays them out */
    int compare;                                            /* the handle is utree_compare_files': two inputs, utk_compare_pass instead of
                                                               utk_merge_pass, nothing is dated, numbered or emitted; or
                                                               utree_inspect_file's: one input, utk_inspect_pass */
} utk_merge_cfg;

/* one contiguous stretch of one input's nodes, all of one pass's word range */
typedef struct {
    uint32_t input, is_ctr, I;
    uint32_t minus;                  /* a MINUS input's slice: words only.  MINUS slices come before the regular ones in a pass */
    uint64_t n;                      /* records: rec bytes each at file_off of fd; they go to raw_off (a multiple of 256) of the pass's device buffer */
    int fd; uint64_t file_off;
    uint64_t raw_off;
    uint64_t g0;                     /* event clock of its first node: nodes of the earlier inputs + index in its input     */
    int has_prev; uint64_t prev_hi, prev_lo;   /* the word of the node in front of the slice                               */
    const uint64_t *h_bins;          /* .ctr: n_bins + 1 bin starts, the first one that of prefix p_lo                      */
    uint32_t p_lo, n_bins;
    uint64_t first;                  /* .ctr: index of the first record in its input (what the bin starts count)           */
} utk_merge_slice;

typedef struct {
    uint64_t n_nodes, n_shared, n_relabelled, n_dropped;
    uint64_t n_label_dropped;        /* regular records whose label line maps to UTK_MERGE_DROP                             */
    uint64_t n_subtracted;           /* regular records with a label, not fed because a MINUS slice holds their word        */
    uint32_t err;                    /* bit 0: a `.ubt` slice not strictly ascending; 1: a node index without a label line; 2: `.ctr` words not ascending */
} utk_merge_pass_out;

typedef struct utk_merge_dev utk_merge_dev;
int utk_merge_limit(int device, uint32_t W, uint32_t rec_max, uint64_t *nodes);       /* nodes a pass may hold, from the free HBM */
int utk_merge_open(const utk_merge_cfg *cfg, utk_merge_dev **out);
/* read the slices through two pinned staging buffers (the read of one chunk overlaps the upload of the one before), decode them in
 * input order, sort, replay, compact: the pass's nodes stay on the device until the next pass.  UTREE_E_IO: slice *io_slice could not be read */
int utk_merge_pass(utk_merge_dev *D, const utk_merge_slice *sl, uint32_t n_sl, int count_stats, utk_merge_pass_out *out, uint32_t *io_slice);
int utk_merge_events(utk_merge_dev *D, uint64_t *h_first_time);                        /* [n_u]: 2g a node g carried the label, 2g+1 a cut at node g made it, ~0 never */
int utk_merge_set_ix(utk_merge_dev *D, const uint32_t *h_ix_of_u, uint32_t n_labels);
int utk_merge_emit(utk_merge_dev *D, int fd);                                          /* the last pass's records to fd: packing and download of a chunk overlap the write of the one before */
int utk_merge_counts(utk_merge_dev *D, uint64_t *h_per_label);
void utk_merge_close(utk_merge_dev *D);

/* ---- utree_compare_files (compare.c): the same handle, slices, staging, decode and sort; input 0 is A, input 1 is B ---- */
#define UTK_COMPARE_FIGURES 5        /* per universe label: same, only_a, only_b, left, arrived */
typedef struct {
    uint64_t n_changed;              /* words of the pass in both inputs under different labels                             */
    uint64_t n_moves;                /* distinct (label in A, label in B) pairs among them, for utk_compare_moves            */
    uint32_t err;                    /* as utk_merge_pass_out's                                                             */
} utk_compare_pass_out;
int utk_compare_limit(int device, uint32_t W, uint32_t rec_max, uint32_t n_u, uint64_t *nodes);   /* utk_merge_limit less the counters */
/* b_g0: the event clock of B's first node (= A's nodes): what tells a lone record's input.  The counters add up over the passes. */
int utk_compare_pass(utk_merge_dev *D, const utk_merge_slice *sl, uint32_t n_sl, uint64_t b_g0, utk_compare_pass_out *out, uint32_t *io_slice);
int utk_compare_moves(utk_merge_dev *D, uint64_t *h_keys, uint32_t *h_counts);          /* the last pass's n_moves pairs, key = label in A << 24 | label in B, ascending */
int utk_compare_figures(utk_merge_dev *D, uint64_t *h_fig);                            /* [UTK_COMPARE_FIGURES][n_u] */

/* ---- utree_inspect_file (inspect.c, inspect_kernels.hip): the same handle (opened with `compare` set and one input), slices, staging,
 * decode and sort.  The pass's nodes, ascending, are appended at index `at` of the caller's device arrays, which hold `cap` nodes: the
 * words' low halves, their high halves (W = 16, else NULL) and the universe label ids.  The passes ascend, so the arrays end up sorted.
 * *n: the pass's nodes; *err as utk_merge_pass_out's (then nothing was appended). ---- */
int utk_inspect_pass(utk_merge_dev *D, const utk_merge_slice *sl, uint32_t n_sl, uint64_t at, uint64_t cap, uint64_t *d_lo, uint64_t *d_hi,
                     uint32_t *d_lab, uint64_t *n, uint32_t *err, uint32_t *io_slice);

#ifdef __cplusplus
}
#endif
#endif
