/* inspect_gpu.h -- interface between inspect.c (host: input, universe, passes, roll-up, writers) and inspect_kernels.hip (device: the
 * resident sorted database, its directory, the neighbour pass and the table of label pairs).  Private. */
#ifndef UTREE_INSPECT_GPU_H
#define UTREE_INSPECT_GPU_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define UTK_INSPECT_FIGURES 4        /* per universe label: isolated, same, lineage, conflict */
#define UTK_INSPECT_KEY_SET (1ull << 24)   /* distinct pairs the key set holds when no pairs file is asked for */

typedef struct {
    uint32_t W;
    int device;
    uint64_t n;                      /* nodes of the database: what the resident arrays hold                                  */
    uint32_t n_u;                    /* the universe, as utk_merge_cfg has it                                                 */
    const uint32_t *h_depth;         /* [n_u]: ';' in the label's text = how many cuts it has                                 */
    const uint32_t *h_trunc_off; const uint32_t *h_trunc_ids; uint32_t n_trunc;
    uint64_t pair_cap;               /* distinct (label, label) pairs the table holds                                         */
    int with_counts;                 /* the pairs are wanted with their counts (a pairs file), not only counted                */
} utk_inspect_cfg;

typedef struct {
    uint64_t pair_events, distinct_pairs;
    uint32_t overflow;               /* more distinct pairs than pair_cap: nothing else of the result is to be used           */
    double seconds;                  /* directory and neighbour pass                                                          */
} utk_inspect_out;

typedef struct utk_inspect_dev utk_inspect_dev;
uint64_t utk_inspect_resident_bytes(uint32_t W, uint64_t n);                   /* 12 bytes per node, 20 for W = 16 */
/* the resident arrays, the directory, the counters and the pair table.  UTREE_E_NOMEM: the device has no room for them */
int utk_inspect_open(const utk_inspect_cfg *cfg, utk_inspect_dev **out);
void utk_inspect_arrays(utk_inspect_dev *D, uint64_t **d_lo, uint64_t **d_hi, uint32_t **d_lab);   /* for utk_inspect_pass; d_hi NULL unless W = 16 */
/* n: the nodes the passes appended, strictly ascending.  Directory over the words' top 24 bits, then the neighbour pass */
int utk_inspect_neighbours(utk_inspect_dev *D, uint64_t n, utk_inspect_out *out);
int utk_inspect_figures(utk_inspect_dev *D, uint64_t *h_fig);                  /* [UTK_INSPECT_FIGURES][n_u] */
int utk_inspect_pairs(utk_inspect_dev *D, uint64_t *h_keys, uint64_t *h_counts);   /* distinct_pairs entries in no order, key = label of the node << 24 | label of its neighbour */
void utk_inspect_close(utk_inspect_dev *D);

#ifdef __cplusplus
}
#endif
#endif
