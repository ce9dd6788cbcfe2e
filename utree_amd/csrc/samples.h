/* samples.h -- launcher of samples_kernels.hip (per-sample taxon table of multiplexed reads, samples.c), private. */
#ifndef UTREE_SAMPLES_H
#define UTREE_SAMPLES_H
#include <stdint.h>
#include "utree_internal.h"
#ifdef __cplusplus
extern "C" {
#endif

#define UTK_SAMPLES_F_TABLE 1ull              /* error word: more distinct ids than sample_capacity, or no free slot within the probe limit */
#define UTK_SAMPLES_F_ARENA 2ull              /* ... the arena of id bytes is used up */
#define UTK_SAMPLES_F_CELLS 4ull              /* ... a (sample, taxon) cell found no free slot in the cell table */
#define UTK_SAMPLES_F_LABEL 8ull              /* ... a classified record names a label the database does not have */
#define UTK_SAMPLES_F_NAME  16ull             /* ... a name lies outside the text it is said to be in */
#define UTK_SAMPLES_F_CUT   32ull             /* ... a taxon of more than UTK_SAMPLES_CUT_MAX bytes: the packed cell key cannot hold its length */
#define UTK_SAMPLES_MISC_WORDS 4u             /* d_misc: {records added, error word, arena cursor, distinct ids} */
#define UTK_SAMPLES_ARENA_PER_SAMPLE 256u     /* arena bytes per sample of the capacity (ids are tens of bytes; a lane that loses a claim leaves its copy unused) */

/* A cell key packs (sample slot, label, cut) into 64 bits: 20 | 28 | 16.  cut: the bytes of the label the line prints, UTK_SAMPLES_CUT_WHOLE for
 * the whole label, UTK_SAMPLES_CUT_EMPTY for the empty taxon (label 0).  All ones is the free slot: no database has label 2^28 - 1. */
#define UTK_SAMPLES_SLOT_BITS 20u
#define UTK_SAMPLES_LABEL_BITS 28u
#define UTK_SAMPLES_CUT_MAX 0xFFFCu
#define UTK_SAMPLES_CUT_UNCL 0xFFFDu          /* in the workgroup's LDS table only: the sample's reads without a line */
#define UTK_SAMPLES_CUT_WHOLE 0xFFFEu
#define UTK_SAMPLES_CUT_EMPTY 0xFFFFu

/* The device side of a handle.  A sample is the slot its id claimed: ids[s] = arena offset << 32 | id length + 1 (0 while free), the id's bytes
 * at arena[offset ..], complete before the key is published; index[s] = the dense index the claim took from misc[3]; reads[s] / uncl[s] = the
 * sample's reads and its reads without a line.  cells: {key, reads} pairs, key as above. */
typedef struct {
    unsigned long long *ids;        /* [id_mask + 1]           */
    uint32_t *index;                /* [id_mask + 1]           */
    unsigned long long *reads;      /* [id_mask + 1]           */
    unsigned long long *uncl;       /* [id_mask + 1]           */
    unsigned long long *cells;      /* [2 * (cell_mask + 1)]   */
    unsigned long long *misc;       /* [UTK_SAMPLES_MISC_WORDS] */
    uint8_t *arena;
    uint64_t arena_cap;
    uint32_t id_mask, cell_mask, sample_cap, n_labels;
    uint32_t delim, pad;
} utk_samples_tab;

/* n records and their names -- name r is d_text[d_name_off[r] .. + d_name_len[r]), d_text holds text_bytes bytes -- into the table; misc[0] += n;
 * asynchronous on `stream` */
int utk_samples_add(const utk_samples_tab *t, const uint8_t *d_text, uint64_t text_bytes, const uint32_t *d_name_off, const uint32_t *d_name_len,
                    const utree_result *d_res, uint32_t n, int n_cu, void *stream);

#ifdef __cplusplus
}
#endif
#endif
