/* main_compare.c -- the `utree-compare` command line:
 *
 *     utree-compare old.{ubt,ctr} new.{ubt,ctr} report.tsv [moves.tsv]
 *
 * The inputs are `.ubt` or `.ctr` databases of one PACKSIZE, in any mix; report.tsv gets the per-taxon k-mer figures of include/utree_amd.h's
 * compare, moves.tsv (optional) one line per distinct (label in old, label in new) pair among the k-mers whose label changed.  Neither input
 * is changed.  UTREE_DEVICE picks the GPU.  Exit codes, the merge's: 0 done (identical or not -- the last line of stdout says which), 1 a file
 * cannot be opened or written, 2 malformed or unsupported input, 3 memory or device.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/utree_amd.h"

#define VER "[v2.0RF SigNature Edition]"          /* itree.c:1350 */

static int exit_of(int rc) { return rc == UTREE_E_IO ? 1 : (rc == UTREE_E_FORMAT || rc == UTREE_E_UNSUPPORTED || rc == UTREE_E_ARG) ? 2 : 3; }

int main(int argc, char *argv[]) {
    if (argc < 4 || argc > 5) {
        printf(VER " usage: utree-compare old.{ubt,ctr} new.{ubt,ctr} report.tsv [moves.tsv]\n");
        exit(1);
    }
    printf("This is UTree " VER "\n");
    const int device = getenv("UTREE_DEVICE") ? atoi(getenv("UTREE_DEVICE")) : 0;
    for (int i = 1; i <= 2; ++i) {
        utree_merge_input in;
        const int rc = utree_merge_probe(argv[i], &in);
        if (rc) { fprintf(stderr, "ERROR: %s [%s]\n", utree_strerror(rc), utree_last_hip_error()); exit(exit_of(rc)); }
        printf("%s: %s, %llu nodes [%llu labels]\n", argv[i], in.is_ctr ? ".ctr" : ".ubt", (unsigned long long)in.n_nodes, (unsigned long long)in.n_labels);
    }
    utree_compare_stats st;
    const int rc = utree_compare_files(argv[1], argv[2], argv[3], argc == 5 ? argv[4] : NULL, device, &st);
    if (rc) { fprintf(stderr, "ERROR: %s [%s]\n", utree_strerror(rc), utree_last_hip_error()); exit(exit_of(rc)); }
    printf("Words: %llu, both %llu, same %llu, changed %llu, only in old %llu, only in new %llu\n", (unsigned long long)st.words,
           (unsigned long long)st.both, (unsigned long long)st.same, (unsigned long long)st.left, (unsigned long long)st.only_a,
           (unsigned long long)st.only_b);
    puts(st.identical ? "identical" : "different");
    fprintf(stderr, "[utree_amd] compare %.3f s: %llu + %llu nodes, %llu + %llu labels, %llu distinct moves, %u passes\n", st.seconds,
            (unsigned long long)st.a, (unsigned long long)st.b, (unsigned long long)st.a_labels, (unsigned long long)st.b_labels,
            (unsigned long long)st.n_moves, st.n_passes);
    exit(0);
}
