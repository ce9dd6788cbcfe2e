/* tiles.h -- between tiles.c and tiles_kernels.hip (not part of the public ABI). */
#ifndef UTREE_TILES_H
#define UTREE_TILES_H
#include "utree_internal.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the workspace of one utree_tiles_plan, carved by tiles.c; both arrays are 256-byte aligned */
typedef struct {
    uint64_t *tcnt;               /* [n_reads + 1] tiles of each query (the last entry 0) */
    void *scan_tmp; size_t scan_tmp_bytes;
} utk_tiles_ws;

/* tiles of a query of L bases: the contract's closed form, on the host and on the device */
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint64_t utk_tiles_of(uint64_t L, uint64_t W, uint64_t S) { return L <= W ? 1 : 1 + (L - W + S - 1) / S; }

size_t utk_tiles_scan_temp_bytes(uint32_t n_reads);
int utk_tiles_plan(const uint32_t *d_len, uint32_t n_reads, uint32_t W, uint32_t S, uint64_t *d_tile_first, utree_tiles_meta *d_meta,
                   const utk_tiles_ws *ws, void *stream);
int utk_tiles_views(const uint64_t *d_off, const uint32_t *d_len, uint32_t n_reads, uint32_t W, uint32_t S, const uint64_t *d_tile_first,
                    uint64_t first_tile, uint32_t n_tiles, uint64_t *d_toff, uint32_t *d_tlen, uint32_t *d_tquery, uint32_t *d_tindex,
                    utree_tiles_meta *d_meta, void *stream);

#ifdef __cplusplus
}
#endif
#endif
