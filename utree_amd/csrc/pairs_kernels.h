/* pairs_kernels.h -- launcher of pairs_kernels.hip (the device join of paired-end mates), private. */
#ifndef UTREE_PAIRS_KERNELS_H
#define UTREE_PAIRS_KERNELS_H
#include <stddef.h>
#include <stdint.h>
#include "utree_internal.h"
#ifdef __cplusplus
extern "C" {
#endif

/* utree_pairs_meta.error */
#define UTK_PAIRS_E_CAPACITY 1u    /* the joined bytes exceed joined_capacity: nothing was written                  */
#define UTK_PAIRS_E_LENGTH   2u    /* a pair's joined length does not fit 32 bits: nothing was written               */

/* all of utree_pairs_join on `stream`; n_pairs > 0.  Returns a hipError_t as int. */
int utk_pairs_join(const uint8_t *d_bases1, const uint64_t *d_off1, const uint32_t *d_len1, const uint8_t *d_bases2, const uint64_t *d_off2,
                   const uint32_t *d_len2, uint32_t n_pairs, uint8_t *d_joined, uint64_t joined_capacity, uint64_t *d_joff, uint32_t *d_jlen,
                   utree_pairs_meta *d_meta, void *stream);

#ifdef __cplusplus
}
#endif
#endif
