/* main_merge.c -- the `utree-mergeGG` (-DUTREE_MERGE_GG) and `utree-merge` command lines:
 *
 *     utree-merge[GG] output.ubt input1 [input2 ...]
 *
 * The inputs are `.ubt` or `.ctr` databases of one PACKSIZE; the output is the `.ubt` of include/utree_amd.h's merge (GG: colliding labels
 * are cut to their common prefix as BUILD_GG does; plain: a collision is BAD as in BUILD).  UTREE_IXTYPE=16|32 sets the output's index
 * width (default: the widest input's), UTREE_DEVICE picks the GPU.  Exit codes: 0 done, 1 a file cannot be opened or written, 2 malformed
 * or unsupported input, 3 memory or device.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/utree_amd.h"

#define VER "[v2.0RF SigNature Edition]"          /* itree.c:1350 */
#ifdef UTREE_MERGE_GG
#define DO_GG 1
#else
#define DO_GG 0
#endif

static int exit_of(int rc) { return rc == UTREE_E_IO ? 1 : (rc == UTREE_E_FORMAT || rc == UTREE_E_UNSUPPORTED || rc == UTREE_E_ARG) ? 2 : 3; }

int main(int argc, char *argv[]) {
    if (argc < 3) {
        printf(VER " usage: utree-merge%s output.ubt input1 [input2 ...]\n", DO_GG ? "GG" : "");
        exit(1);
    }
    printf("This is UTree " VER "\n");
    uint32_t I = 0;
    if (getenv("UTREE_IXTYPE")) I = atoi(getenv("UTREE_IXTYPE")) == 32 ? 4 : atoi(getenv("UTREE_IXTYPE")) == 16 ? 2 : 0;
    const int device = getenv("UTREE_DEVICE") ? atoi(getenv("UTREE_DEVICE")) : 0;
    for (int i = 2; i < argc; ++i) {
        utree_merge_input in;
        const int rc = utree_merge_probe(argv[i], &in);
        if (rc) { fprintf(stderr, "ERROR: %s [%s]\n", utree_strerror(rc), utree_last_hip_error()); exit(exit_of(rc)); }
        printf("%s: %s, %llu nodes [%llu labels]\n", argv[i], in.is_ctr ? ".ctr" : ".ubt", (unsigned long long)in.n_nodes, (unsigned long long)in.n_labels);
    }
    utree_merge_stats st;
    const int rc = utree_merge_files((const char *const *)(argv + 2), argc - 2, argv[1], I, DO_GG, device, &st);
    if (rc) { fprintf(stderr, "ERROR: %s [%s]\n", utree_strerror(rc), utree_last_hip_error()); exit(exit_of(rc)); }
    printf("Total nodes in tree: %llu [%llu labels]\n", (unsigned long long)st.n_nodes, (unsigned long long)st.n_labels);   /* itree.c:1337 */
    puts("Tree written.");
    fprintf(stderr, "[utree_amd] merge %.3f s: %u inputs, %llu nodes in, %llu shared, %llu relabelled, %llu dropped, %u passes\n", st.seconds,
            st.n_inputs, (unsigned long long)st.n_in_nodes, (unsigned long long)st.n_shared, (unsigned long long)st.n_relabelled,
            (unsigned long long)st.n_dropped, st.n_passes);
    exit(0);
}
