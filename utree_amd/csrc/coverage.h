/* coverage.h -- launchers of coverage_kernels.hip (distinct database k-mers covered per taxon, coverage.c), private. */
#ifndef UTREE_COVERAGE_H
#define UTREE_COVERAGE_H
#include <stdint.h>
#include "utree_internal.h"
#ifdef __cplusplus
extern "C" {
#endif

/* What the coverage kernels probe: the .ctr's own bin table and node dump, in file order, as the file holds them (records of
 * SZ = W + I - 3 packed bytes).  `recs` is 8-byte aligned and followed by at least UTK_COV_PAD readable bytes: a record is read as
 * aligned 8-byte words. */
#define UTK_COV_PAD 16u
typedef struct {
    const uint64_t *recs;
    const void *binix;              /* 2^24 + 1 entries, 4 bytes each, or 8 with off64 */
    uint64_t n_nodes;
    uint32_t W, I, n_labels, off64;
} utk_cov_db;

/* windows of the reads -> the node each hit ends on -> its bit in `bitmap` (n_nodes bits), d_hits[label] += 1 per hit, *d_reads += n_reads;
 * asynchronous on `stream` */
int utk_coverage_add(const utk_cov_db *db, const uint8_t *d_bases, const uint64_t *d_off, const uint32_t *d_len, uint32_t n_reads, int do_rc,
                     uint32_t *bitmap, unsigned long long *d_hits, unsigned long long *d_reads, void *stream);
/* one pass over dump and bitmap: d_db[l] += records whose stored index is l, d_cov[l] += those whose bit is set (l < n_labels) */
int utk_coverage_count(const utk_cov_db *db, const uint32_t *bitmap, unsigned long long *d_db, unsigned long long *d_cov, int n_cu, void *stream);
/* dst |= src over n 32-bit words; dst += src over n 64-bit counters */
int utk_coverage_or(uint32_t *dst, const uint32_t *src, uint64_t n, void *stream);
int utk_coverage_sum(unsigned long long *dst, const unsigned long long *src, uint64_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif
