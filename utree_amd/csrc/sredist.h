/* sredist.h -- launchers of sredist_kernels.hip (candidate sets per sample and their redistribution within each sample, sredist.c), private. */
#ifndef UTREE_SREDIST_H
#define UTREE_SREDIST_H
#include <stdint.h>
#include "utree_internal.h"
#include "redist.h"
#include "samples.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The device side of a handle: the id table of a sample table (samples.h; its reads / uncl count per sample, its cell table holds the cells of
 * this report) and the table of multi-label sets of a redistribution (redist.h; `single` is NULL and the slots' read counts stay 0: the reads
 * are counted per cell).  A cell key is sample slot << 32 | set handle; the handle is UTK_SREDIST_ONE | label for one candidate, else the set's
 * slot.  All ones is the free cell slot: a sample slot has 20 bits.  Each of the two tables has its error word (misc[1]). */
#define UTK_SREDIST_ONE 0x80000000u
typedef struct { utk_samples_tab s; utk_redist_tab r; } utk_sredist_tab;

/* one cell as the host gives it (utree_sredist_insert): `reads` reads of sample `sample` (an index into the ids given with it) whose candidates
 * are labels[first .. first + n) */
typedef utree_sredist_cell utk_sredist_cell;

/* the batch's reads into the tables, records as utk_redist_add takes them, names as utk_samples_add does; s.misc[0] += n; asynchronous */
int utk_sredist_add(const utk_sredist_tab *t, const utk_image *im, const utree_result *d_res, const utk_workspace *ws, const uint8_t *d_text,
                    uint64_t text_bytes, const uint32_t *d_name_off, const uint32_t *d_name_len, uint32_t n, int n_cu, void *stream);
/* n_samples ids (bytes d_ids[d_id_off[i] .. d_id_off[i + 1])) interned, their slots to d_slot_of, their reads and unclassified reads added;
 * then n_cells cells of those samples; s.misc[0] += n_reads */
int utk_sredist_insert(const utk_sredist_tab *t, const uint8_t *d_ids, const uint64_t *d_id_off, const unsigned long long *d_reads,
                       const unsigned long long *d_uncl, uint32_t n_samples, uint32_t *d_slot_of, const utk_sredist_cell *d_cells,
                       const uint32_t *d_labels, uint64_t n_cells, unsigned long long n_reads, void *stream);

/* The solver's problem, flat: cell c has `reads` reads of sample `sample` whose candidates are the tally indices member[first .. first + n);
 * a sample's tally indices are consecutive and ascend with the file-order label index (the tie-break compares them); seg[i] = the sample of
 * tally index i; act[s] = the sample's position among the samples still active, 0xFFFFFFFF once it has stopped. */
typedef struct {
    const utk_sredist_cell *cells; const uint32_t *member; const uint32_t *seg; const uint32_t *act;
    uint64_t n_cells, n_tally;
} utk_sredist_problem;
/* T0: tally[i] = reads of the cells that contain i */
int utk_sredist_tally0(const utk_sredist_problem *p, unsigned long long *tally, void *stream);
/* one pass over the active samples: next[i] = reads of the cells whose richest member under prev is i, changes[act[s]] = sum |next - prev| over
 * sample s's indices (n_active words); a stopped sample keeps its tally: next[i] = prev[i].  all != 0: every sample is evaluated, no changes */
int utk_sredist_pass(const utk_sredist_problem *p, const unsigned long long *prev, unsigned long long *next, unsigned long long *changes,
                     uint32_t n_active, int all, void *stream);

#ifdef __cplusplus
}
#endif
#endif
