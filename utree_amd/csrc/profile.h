/* profile.h -- launcher of profile_kernels.hip (per-taxon read counts, profile.c), private. */
#ifndef UTREE_PROFILE_H
#define UTREE_PROFILE_H
#include <stdint.h>
#include "utree_internal.h"
#ifdef __cplusplus
extern "C" {
#endif

#define PROF_F_FULL  1u     /* a truncated taxon found no free slot in the device table: the counts are incomplete */
#define PROF_F_LABEL 2u     /* a classified record names a label the database does not have                      */

/* adds n records into the counters (profile_kernels.hip: layout of d_whole / d_table / d_misc); asynchronous on `stream` */
int utk_profile_add(const utree_result *d_res, uint32_t n, uint32_t n_labels, unsigned long long *d_whole, unsigned long long *d_table,
                    uint32_t mask, unsigned long long *d_misc, int n_cu, void *stream);

#ifdef __cplusplus
}
#endif
#endif
