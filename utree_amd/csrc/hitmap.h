/* hitmap.h -- between hitmap.c and hitmap_kernels.hip (not part of the public ABI). */
#ifndef UTREE_HITMAP_H
#define UTREE_HITMAP_H
#include "utree_internal.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UTK_HM_SEG 32u        /* window starts per item of the code pass                     */
#define UTK_HM_GROUP 64u      /* windows per group of the run passes: one wavefront's ballot */

/* the workspace of one call, carved by hitmap.c; every array is 256-byte aligned */
typedef struct {
    uint64_t *wcnt, *woff;        /* [n_reads + 1] windows of each query, and their exclusive scan (woff[n_reads] = the batch's windows) */
    uint64_t *icnt, *ioff;        /* [n_reads + 1] items of each query, scanned                                                            */
    uint32_t *codes;              /* [wcap] one code per window of every query, queries in order                                           */
    uint32_t *starts;             /* [(wcap >> 5) + 2] bit g: window g is its query's first                                                */
    uint64_t *gcnt, *gbase;       /* [n_groups + 1] run heads of each group of UTK_HM_GROUP windows, scanned                              */
    uint64_t *gfirst, *gnext;     /* [n_groups + 1] REVERSED (entry n_groups - g): the group's first head, and the first head at or behind it */
    unsigned int *flag;           /* 0, or why the batch has no map: 2 = more windows than wcap, 3 = a query of 2^32 windows or more       */
    void *scan_tmp; size_t scan_tmp_bytes;
    uint64_t wcap, n_groups;
} utk_hitmap_ws;

/* bounds the host derives from (n_reads, total_bases, do_rc): windows, groups, items */
static inline uint64_t utk_hitmap_wcap(uint32_t n_reads, uint64_t total_bases, int do_rc) {
    return do_rc ? 2 * total_bases + (uint64_t)n_reads : total_bases;          /* a query has at most len(q) windows */
}
static inline uint64_t utk_hitmap_groups(uint64_t wcap) { return wcap / UTK_HM_GROUP + 1; }

size_t utk_hitmap_scan_temp_bytes(uint32_t n_reads, uint64_t n_groups);
int utk_hitmap_run(const utk_image *im, const uint8_t *d_bases, const uint64_t *d_off, const uint32_t *d_len, uint32_t n_reads, uint64_t total_bases,
                   int do_rc, uint64_t *d_run_off, utree_hit_run *d_runs, uint64_t run_capacity, utree_hitmap_meta *d_meta, const utk_hitmap_ws *ws,
                   int n_cu, void *stream);

#ifdef __cplusplus
}
#endif
#endif
