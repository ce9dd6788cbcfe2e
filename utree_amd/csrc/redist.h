/* redist.h -- launchers of redist_kernels.hip (candidate sets of ambiguous reads and their redistribution, redist.c), private. */
#ifndef UTREE_REDIST_H
#define UTREE_REDIST_H
#include <stdint.h>
#include "utree_internal.h"
#ifdef __cplusplus
extern "C" {
#endif

#define UTK_REDIST_ARENA_PER_SLOT 8u          /* arena labels per table slot */
#define UTK_REDIST_F_TABLE 1ull               /* error word: no free slot within the probe limit */
#define UTK_REDIST_F_ARENA 2ull               /* ... the arena is used up */
#define UTK_REDIST_F_LABEL 4ull               /* ... a record named a label the database does not have */
#define UTK_REDIST_MISC_WORDS 8u              /* d_misc: {reads, error word, arena cursor, changes, ambiguous reads, -, -, -} */
/* the error word in words (redist.c): `lead` in front of every phrase, `sep` behind every one but the last of the three */
void utree_redist_flags_text(unsigned long long f, const char *lead, const char *sep, char *msg, size_t cap);

/* The device side of a handle.  A slot is {key, reads}: key = arena offset << 32 | labels of the set (>= 2), 0 while free; the set's labels are
 * file-order indices at arena[offset ..], complete before the key is published.  single[l] = reads whose only candidate is l. */
typedef struct {
    unsigned long long *slots;      /* [2 * (mask + 1)] */
    uint32_t *arena;
    unsigned long long *single;     /* [n_labels] */
    unsigned long long *misc;       /* [UTK_REDIST_MISC_WORDS] */
    uint64_t arena_cap;
    uint32_t mask, n_labels;
} utk_redist_tab;

/* the candidate sets of a batch whose records still wait for utk_vote (RANK_PENDING / CUT_PENDING, or finished) into the table; misc[0] +=
 * n_reads; d_key: NULL, or where every read's key goes (include/utree_amd.h: UTREE_REDIST_KEY_NONE; another instantiation of the kernel);
 * asynchronous on `stream` */
int utk_redist_add(const utk_redist_tab *t, const utk_image *im, const utree_result *d_res, const utk_workspace *ws, uint32_t n_reads, int n_cu,
                   uint32_t *d_key, void *stream);
/* n_sets sets given flat -- set i is d_labels[d_first[i] .. + d_n[i]) with d_reads[i] reads -- re-inserted (utree_redist_merge) */
int utk_redist_insert(const utk_redist_tab *t, const unsigned long long *d_reads, const unsigned long long *d_first, const uint32_t *d_n,
                      const uint32_t *d_labels, uint64_t n_sets, void *stream);
/* dst[i] += src[i] over n 64-bit counters */
int utk_redist_sum(unsigned long long *dst, const unsigned long long *src, uint64_t n, void *stream);
/* T0: tally[l] = single[l] + reads of every set that contains l; misc[4] = reads of all sets */
int utk_redist_tally0(const utk_redist_tab *t, unsigned long long *tally, void *stream);
/* one pass: next[l] = single[l] + reads of the sets whose richest candidate under `prev` is l; misc[3] = sum over l of |next[l] - prev[l]| */
int utk_redist_pass(const utk_redist_tab *t, const unsigned long long *prev, unsigned long long *next, void *stream);

/* every slot's winner under `tally` and its number of candidates: d_win[s] = win(set s, tally), d_ncand[s] = |set s| (free: ~0 and 0); no atomics */
int utk_redist_winner(const utk_redist_tab *t, const unsigned long long *tally, uint32_t *d_win, uint32_t *d_ncand, void *stream);
/* n keys of the table -> label and candidates of each read, from d_win / d_ncand: a pure gather (d_ncand_out may be NULL) */
int utk_redist_assign(const utk_redist_tab *t, const uint32_t *d_win, const uint32_t *d_ncand, const uint32_t *d_key, uint64_t n, uint32_t *d_label,
                      uint32_t *d_ncand_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
