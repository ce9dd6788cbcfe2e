/* main_merge.c -- the `utree-mergeGG` (-DUTREE_MERGE_GG) and `utree-merge` command lines:
 *
 *     utree-merge[GG] output.ubt input1 [input2 ...]
 *
 * The inputs are `.ubt` or `.ctr` databases of one PACKSIZE; the output is the `.ubt` of include/utree_amd.h's merge (GG: colliding labels
 * are cut to their common prefix as BUILD_GG does; plain: a collision is BAD as in BUILD).  UTREE_IXTYPE=16|32 sets the output's index
 * width (default: the widest input's), UTREE_DEVICE picks the GPU.  Exit codes: 0 done, 1 a file cannot be opened or written, 2 malformed
 * or unsupported input, 3 memory or device.
 *
 * Editing while merging (utree_merge_files_edit), opted into by the environment: UTREE_MERGE_RANKS=n cuts every label to its first n
 * ranks, UTREE_MERGE_DROP / UTREE_MERGE_KEEP name a file of clades to drop / to keep, UTREE_MERGE_RENAME a file of `old TAB new` lines,
 * UTREE_MERGE_MINUS a ':'-separated list of databases whose k-mers are subtracted.  UTREE_MERGE_PREVIEW=file.tsv writes what the label
 * edit would do to every label (utree_merge_edit_preview) and stops: no device is opened, output.ubt is not created, exit code 0.
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
    /* ---- the edit, if any ---- */
    utree_merge_edit ed;
    memset(&ed, 0, sizeof ed);
    ed.size = (uint32_t)sizeof ed;
    const char *minus[256];
    const char *e = getenv("UTREE_MERGE_RANKS");
    int editing = 0;
    if (e && *e) {
        char *end;
        const unsigned long v = strtoul(e, &end, 10);
        if (*e < '0' || *e > '9' || *end || v > 255) { fprintf(stderr, "ERROR: UTREE_MERGE_RANKS is a number from 0 to 255\n"); exit(2); }
        ed.ranks = (uint32_t)v;
        editing = 1;
    }
    if ((e = getenv("UTREE_MERGE_DROP")) && *e) { ed.drop_path = e; editing = 1; }
    if ((e = getenv("UTREE_MERGE_KEEP")) && *e) { ed.keep_path = e; editing = 1; }
    if ((e = getenv("UTREE_MERGE_RENAME")) && *e) { ed.rename_path = e; editing = 1; }
    if ((e = getenv("UTREE_MERGE_MINUS")) && *e) {
        char *list = strdup(e);
        if (!list) exit(3);
        for (char *tok = strtok(list, ":"); tok; tok = strtok(NULL, ":")) {
            if (ed.n_minus == 256) { fprintf(stderr, "ERROR: UTREE_MERGE_MINUS names more than 256 databases\n"); exit(2); }
            minus[ed.n_minus++] = tok;
        }
        ed.minus_paths = minus;
        editing = 1;
    }
    const char *preview = getenv("UTREE_MERGE_PREVIEW");
    if (preview && !*preview) preview = NULL;
    for (int i = 2; i < argc + (preview ? 0 : ed.n_minus); ++i) {
        const char *path = i < argc ? argv[i] : minus[i - argc];
        utree_merge_input in;
        const int rc = utree_merge_probe(path, &in);
        if (rc) { fprintf(stderr, "ERROR: %s [%s]\n", utree_strerror(rc), utree_last_hip_error()); exit(exit_of(rc)); }
        printf("%s: %s, %llu nodes [%llu labels]\n", path, in.is_ctr ? ".ctr" : ".ubt", (unsigned long long)in.n_nodes, (unsigned long long)in.n_labels);
    }
    utree_merge_edit_stats es;
    if (preview) {
        const int rc = utree_merge_edit_preview((const char *const *)(argv + 2), argc - 2, &ed, preview, &es);
        if (rc) { fprintf(stderr, "ERROR: %s [%s]\n", utree_strerror(rc), utree_last_hip_error()); exit(exit_of(rc)); }
        fprintf(stderr, "[utree_amd] edit preview: %llu label lines, %llu dropped, %llu renamed, %llu cut, %llu rules unmatched, %llu nodes dropped\n",
                (unsigned long long)es.n_label_lines, (unsigned long long)es.n_labels_dropped, (unsigned long long)es.n_labels_renamed,
                (unsigned long long)es.n_labels_cut, (unsigned long long)es.n_rules_unmatched, (unsigned long long)es.n_nodes_dropped);
        exit(0);
    }
    utree_merge_stats st;
    const int rc = editing ? utree_merge_files_edit((const char *const *)(argv + 2), argc - 2, argv[1], I, DO_GG, device, &ed, &st, &es)
                           : utree_merge_files((const char *const *)(argv + 2), argc - 2, argv[1], I, DO_GG, device, &st);
    if (rc) { fprintf(stderr, "ERROR: %s [%s]\n", utree_strerror(rc), utree_last_hip_error()); exit(exit_of(rc)); }
    printf("Total nodes in tree: %llu [%llu labels]\n", (unsigned long long)st.n_nodes, (unsigned long long)st.n_labels);   /* itree.c:1337 */
    puts("Tree written.");
    fprintf(stderr, "[utree_amd] merge %.3f s: %u inputs, %llu nodes in, %llu shared, %llu relabelled, %llu dropped, %u passes\n", st.seconds,
            st.n_inputs, (unsigned long long)st.n_in_nodes, (unsigned long long)st.n_shared, (unsigned long long)st.n_relabelled,
            (unsigned long long)st.n_dropped, st.n_passes);
    if (editing)
        fprintf(stderr, "[utree_amd] edit: %llu label lines, %llu dropped, %llu renamed, %llu cut, %llu rules unmatched, %llu nodes dropped, %llu minus nodes, %llu nodes subtracted\n",
                (unsigned long long)es.n_label_lines, (unsigned long long)es.n_labels_dropped, (unsigned long long)es.n_labels_renamed,
                (unsigned long long)es.n_labels_cut, (unsigned long long)es.n_rules_unmatched, (unsigned long long)es.n_nodes_dropped,
                (unsigned long long)es.n_minus_nodes, (unsigned long long)es.n_nodes_subtracted);
    exit(0);
}
