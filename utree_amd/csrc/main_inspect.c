/* main_inspect.c -- the `utree-inspect` command line:
 *
 *     utree-inspect db.{ubt,ctr} report.tsv [pairs.tsv]
 *
 * The input is a `.ubt` or `.ctr` database; report.tsv gets the per-taxon figures of include/utree_amd.h's inspection -- how many of each
 * taxon's k-mers have no neighbour one substitution away, only neighbours of their own label, neighbours on their lineage, or neighbours
 * under another taxon -- and pairs.tsv (optional) one line per distinct ordered pair of label texts that are one substitution apart.  The
 * input is not changed.  UTREE_DEVICE picks the GPU, UTREE_INSPECT_PAIRS the distinct pairs pairs.tsv may hold (default 2^22).  Exit codes,
 * the merge's: 0 done (clean or not -- the last line of stdout says which), 1 a file cannot be opened or written, 2 malformed or
 * unsupported input, 3 memory or device.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/utree_amd.h"

#define VER "[v2.0RF SigNature Edition]"          /* itree.c:1350 */

static int exit_of(int rc) { return rc == UTREE_E_IO ? 1 : (rc == UTREE_E_FORMAT || rc == UTREE_E_UNSUPPORTED || rc == UTREE_E_ARG) ? 2 : 3; }

int main(int argc, char *argv[]) {
    if (argc < 3 || argc > 4) {
        printf(VER " usage: utree-inspect db.{ubt,ctr} report.tsv [pairs.tsv]\n");
        exit(1);
    }
    printf("This is UTree " VER "\n");
    const int device = getenv("UTREE_DEVICE") ? atoi(getenv("UTREE_DEVICE")) : 0;
    utree_merge_input in;
    int rc = utree_merge_probe(argv[1], &in);
    if (rc) { fprintf(stderr, "ERROR: %s [%s]\n", utree_strerror(rc), utree_last_hip_error()); exit(exit_of(rc)); }
    printf("%s: %s, %llu nodes [%llu labels]\n", argv[1], in.is_ctr ? ".ctr" : ".ubt", (unsigned long long)in.n_nodes, (unsigned long long)in.n_labels);
    utree_inspect_stats st;
    rc = utree_inspect_file(argv[1], argv[2], argc == 4 ? argv[3] : NULL, device, &st);
    if (rc) { fprintf(stderr, "ERROR: %s [%s]\n", utree_strerror(rc), utree_last_hip_error()); exit(exit_of(rc)); }
    printf("K-mers: %llu, isolated %llu, same %llu, lineage %llu, conflict %llu\n", (unsigned long long)st.kmers, (unsigned long long)st.isolated,
           (unsigned long long)st.same, (unsigned long long)st.lineage, (unsigned long long)st.conflict);
    puts(st.clean ? "clean" : "conflicts");
    fprintf(stderr, "[utree_amd] inspect %.3f s (neighbour pass %.3f s): %llu nodes, %llu labels, %llu pair events, %llu distinct pairs, %u passes\n",
            st.seconds, st.seconds_neighbours, (unsigned long long)st.kmers, (unsigned long long)st.labels, (unsigned long long)st.pair_events,
            (unsigned long long)st.distinct_pairs, st.n_passes);
    exit(0);
}
