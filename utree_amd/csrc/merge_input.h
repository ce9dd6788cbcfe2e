/* merge_input.h -- what merge.c and compare.c share on the host (the functions are in merge.c): one input database as it reads (`.ubt` or
 * `.ctr`, told apart by structure; include/utree_amd.h states the refusals), the plan of passes over contiguous ranges of the words' top 24
 * bits, and a pass's slices.  Private. */
#ifndef UTREE_MERGE_INPUT_H
#define UTREE_MERGE_INPUT_H
#include <stdint.h>
#include <stdio.h>
#include "utree_internal.h"
#include "merge_gpu.h"
#include "label_edit.h"
#include "strtab.h"

typedef struct {
    const char *path;
    int fd;
    const uint8_t *map; uint64_t size;
    int is_ctr;
    uint32_t W, I, rec, binw;
    uint64_t n, rec_off, tail_off;
    uint64_t *bins;                  /* .ctr: NPREFIX + 1 bin starts */
    uint32_t *u_of_ix; uint32_t n_lines;       /* distinct label texts in order of first appearance (the loader's numbering) -> universe id */
    uint64_t g0;                     /* nodes of the inputs in front */
} merge_in;

/* sets utree_last_hip_error to fmt (two %s: path, more) and returns rc */
int utree_merge_fail_text(int rc, const char *fmt, const char *path, const char *more);

/* header, layout, bin table, label lines -> universe.  `in` is zeroed with fd = -1 by the caller and closed by it whatever comes back.
 * R (or NULL): each distinct label text goes through the label edit; its edited text enters the universe in its place, a dropped one maps to
 * UTK_MERGE_DROP; es (or NULL) counts what the edit did, tsv (or NULL) gets the preview's line per text.  minus: a MINUS input gives words
 * only, its label lines are not read. */
int utree_merge_input_open(merge_in *in, const char *path, label_universe *L, le_rules *R, utree_merge_edit_stats *es, int minus, FILE *tsv);
void utree_merge_input_close(merge_in *in);

/* The passes over ins[0 .. n_in), n_read nodes in all: pass p takes the words whose top 24 bits lie in [bounds[p], bounds[p + 1]), so a run
 * of equal words is never split and a `.ctr`'s slice is a range of bins.  A pass holds at most `limit` nodes (UTREE_TEST_MERGE_PASS_NODES
 * lowers what a pass aims at, never below one prefix); *cap_nodes / *cap_raw: the largest pass's nodes and record bytes as the slices lay
 * them out.  `name` is the path a failure names.  *bounds is the caller's to free. */
int utree_merge_plan(const merge_in *ins, int n_in, uint64_t n_read, uint64_t limit, const char *name, uint32_t **bounds, uint32_t *n_pass,
                     uint64_t *cap_nodes, uint64_t *cap_raw);

/* sl[0 .. n_in): every input's slice of pass p; the first n_minus inputs are MINUS inputs */
void utree_merge_slices(const merge_in *ins, int n_in, int n_minus, const uint32_t *bounds, uint32_t p, utk_merge_slice *sl);

#endif
