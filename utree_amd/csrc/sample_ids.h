/* sample_ids.h -- the id-table half of a per-sample handle (sample_ids.c), private: what samples.c and sredist.c both do with a utk_samples_tab. */
#ifndef UTREE_SAMPLE_IDS_H
#define UTREE_SAMPLE_IDS_H
#include <stddef.h>
#include <stdint.h>
#include "samples.h"

/* A report's name in front of every text, and the phrases in which the two reports really differ. */
typedef struct {
    const char *report;             /* "sample table"                                               */
    const char *counters;           /* whose counters the first check names: "id table" or "tables" */
    const char *cells_full;         /* UTK_SAMPLES_F_CELLS                                          */
    const char *bad_name;           /* UTK_SAMPLES_F_NAME                                           */
} utree_sample_ids_text;

/* One block ids | reads | uncl | cells | misc | index | arena on `device` (made the current one) and `t` set up over it; not yet reset.  UTREE_E_ARG for a
 * capacity or delimiter out of range, UTREE_E_UNSUPPORTED for more labels than a cell key holds, UTREE_E_NOMEM, UTREE_E_HIP; `t` is all zero then. */
int utree_sample_ids_create(utk_samples_tab *t, int device, uint32_t sample_capacity, uint32_t cell_capacity, int delim, uint64_t n_labels);
/* every counter zero, every cell free (the arena is written before it is read); no wait before or after */
int utree_sample_ids_reset(const utk_samples_tab *t);
void utree_sample_ids_free(utk_samples_tab *t);

/* UTREE_OK when the error word fs is 0 and `more` -- the texts of the caller's own flags, " phrase; phrase" -- is empty; else the text, UTREE_E_DEVICE */
int utree_sample_ids_check_flags(const utree_sample_ids_text *x, unsigned long long fs, const char *more);

/* A read-back: the samples dense (index i is the one its id took when it was claimed) and the cell table as the device left it, for the caller
 * to decode its own keys. */
typedef struct {
    size_t S, id_bytes;
    uint64_t n_reads;                               /* misc[0]: set whenever the counters could be copied, whatever they then said */
    uint8_t *ids; uint64_t *id_off, *reads, *uncl;  /* id_off [S + 1]; malloc'ed, the caller may take them (and set them NULL)     */
    uint64_t *sum;                                  /* [S]: the reads of each sample's cells, as utree_sample_ids_count adds them  */
    const unsigned long long *cells;                /* {key, reads} x cell_slots: key all ones = free                              */
    uint32_t cell_slots, id_slots;
    unsigned long long *slot_key;                   /* [id_slots]: 0 = no sample (the copied block begins here)                    */
    const uint32_t *index;                          /* [id_slots]: slot -> dense index                                             */
} utree_sample_ids_view;

/* waits for the current device, copies counters and arena and validates them; UTREE_E_DEVICE with a text when a batch set a flag (`more` as above) or
 * the id table is inconsistent.  utree_sample_ids_view_free in every case. */
int utree_sample_ids_read(const utk_samples_tab *t, const utree_sample_ids_text *x, const char *more, utree_sample_ids_view *v);
void utree_sample_ids_view_free(utree_sample_ids_view *v);
/* a cell of `reads` reads whose key names the sample in `slot`: its dense index; UTREE_E_DEVICE with a text when the slot holds none */
int utree_sample_ids_count(const utree_sample_ids_text *x, utree_sample_ids_view *v, uint32_t slot, uint64_t reads, uint32_t *sample);
/* once every cell is counted: every sample's reads = its unclassified + its cells, and all reads = n_reads, or UTREE_E_DEVICE with a text */
int utree_sample_ids_check_sums(const utree_sample_ids_text *x, const utree_sample_ids_view *v);

#endif
