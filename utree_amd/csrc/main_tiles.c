/* main_tiles.c -- the `utree-tiles` command line:
 *
 *     utree-tiles db.ctr contigs.fa tiles.tsv [segments.tsv] [RC]
 *
 * Long queries -- contigs, genomes, nanopore reads -- classified tile by tile (include/utree_amd.h: utree_tiles_file).  tiles.tsv gets, for
 * every tile with a hit, the line `xtree-searchGG` prints for that stretch as a read of its own, under the name <name>:<start>-<end>;
 * segments.tsv (optional) the maximal runs of consecutive tiles of one taxon.  The queries are uploaded once: a tile is a view into them.
 *     UTREE_TILE_BP=<W>     tile length in bases (default 1000; 1 .. 16777214)
 *     UTREE_TILE_STEP=<S>   step from one tile to the next (default W/2, at least 1; 1 .. W)
 *     UTREE_INPUT=auto|fastq|fasta   as for xtree-searchGG: FASTQ / multi-line FASTA, plain or gzip (default: two lines per record)
 *     UTREE_TILES_BATCH=<n> tiles per classify batch (default and most 2097152)
 *     UTREE_DEVICE=<d>      the GPU
 * A malformed value is refused with a line that names the variable, exit 2.  Exit codes, the merge's: 0 done, 1 a file cannot be opened or
 * written, 2 malformed or unsupported input -- a malformed record as in xtree-searchGG: the reference's message, and the tiles of the
 * queries in front of it are written --, 3 memory or device.  A run that fails otherwise leaves neither file.
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/utree_amd.h"

#define VER "[v2.0RF SigNature Edition]"          /* itree.c:1350 */

static int exit_of(int rc) { return rc == UTREE_E_IO ? 1 : (rc == UTREE_E_FORMAT || rc == UTREE_E_UNSUPPORTED || rc == UTREE_E_ARG || rc == UTREE_E_NOLABELS) ? 2 : 3; }

/* the whole of `s` as a decimal number in [lo, hi]; else the line that names the variable, and exit 2 */
static unsigned long env_number(const char *name, const char *s, unsigned long lo, unsigned long hi) {
    char *end = NULL;
    errno = 0;
    const unsigned long long v = strtoull(s, &end, 10);
    if (!*s || *s == '-' || *s == '+' || *s == ' ' || !end || *end || errno || v < lo || v > hi) {
        fprintf(stderr, "ERROR: %s must be a number from %lu to %lu, not \"%s\"\n", name, lo, hi, s);
        exit(2);
    }
    return (unsigned long)v;
}

int main(int argc, char *argv[]) {
    const int do_rc = argc >= 2 && !strcmp(argv[argc - 1], "RC");
    argc -= do_rc;
    if (argc < 4 || argc > 5) {
        printf(VER " usage: utree-tiles db.ctr contigs.fa tiles.tsv [segments.tsv] [RC]\n");
        exit(1);
    }
    printf("This is UTree " VER "\n");
    utree_tiles_params prm = {.size = sizeof prm, .tile_bp = 1000, .do_rc = do_rc, .input_format = UTREE_INPUT_REFERENCE, .host_threads = 0};
    const char *e;
    if ((e = getenv("UTREE_TILE_BP"))) prm.tile_bp = (uint32_t)env_number("UTREE_TILE_BP", e, 1, UTREE_TILE_MAX_BP);
    prm.step_bp = prm.tile_bp / 2 ? prm.tile_bp / 2 : 1;
    if ((e = getenv("UTREE_TILE_STEP"))) prm.step_bp = (uint32_t)env_number("UTREE_TILE_STEP", e, 1, prm.tile_bp);
    if ((e = getenv("UTREE_TILES_BATCH"))) (void)env_number("UTREE_TILES_BATCH", e, 1, UTREE_TILES_MAX_BATCH);   /* (the library reads it) */
    if ((e = getenv("UTREE_INPUT"))) {
        if (!strcmp(e, "auto")) prm.input_format = UTREE_INPUT_AUTO;
        else if (!strcmp(e, "fastq")) prm.input_format = UTREE_INPUT_FASTQ;
        else if (!strcmp(e, "fasta")) prm.input_format = UTREE_INPUT_FASTA_MULTILINE;
        else { fprintf(stderr, "ERROR: UTREE_INPUT must be auto, fastq or fasta, not \"%s\"\n", e); exit(2); }
    }
    int device = 0;
    if ((e = getenv("UTREE_DEVICE"))) device = (int)env_number("UTREE_DEVICE", e, 0, 1023);
    printf("Reverse complement consideration is %sabled.\n", do_rc ? "en" : "dis");
    printf("Tiles of %u bases every %u.\n", prm.tile_bp, prm.step_bp);

    utree_ctr *ctr = NULL;
    int rc = utree_ctr_open(argv[1], &ctr);
    if (rc) { fprintf(stderr, "ERROR: %s: %s\n", argv[1], utree_strerror(rc)); exit(exit_of(rc)); }
    utree_ctr_info ci;
    utree_ctr_get_info(ctr, &ci);
    printf("Nodes in input tree: %llu (PACKSIZE=%u) [%u labels]\n", (unsigned long long)ci.n_nodes, ci.W << 2, ci.n_labels);
    utree_dev *dev = NULL;
    rc = utree_dev_upload(ctr, device, UTREE_FINE_AUTO, &dev);
    if (rc) { fprintf(stderr, "ERROR: device image: %s [%s]\n", utree_strerror(rc), utree_last_hip_error()); utree_ctr_close(ctr); exit(rc == UTREE_E_FORMAT ? 2 : 3); }
    puts("Tree read.");
    fflush(stdout);

    utree_tiles_stats st = {.size = sizeof st};
    rc = utree_tiles_file(ctr, dev, argv[2], argv[3], argc == 5 ? argv[4] : NULL, &prm, &st);
    utree_dev_free(dev);                                                                  /* (every way out from here on has given both back) */
    utree_ctr_close(ctr);
    if (rc == UTREE_E_IO) { puts("Invalid input files"); exit(1); }                      /* itree.c:835 */
    if (rc && rc != UTREE_E_FASTA) { fprintf(stderr, "ERROR: %s [%s]\n", utree_strerror(rc), utree_last_hip_error()); exit(exit_of(rc)); }
    printf("Queries: %llu, tiles %llu, classified %llu, segments %llu\n", (unsigned long long)st.n_queries, (unsigned long long)st.n_tiles,
           (unsigned long long)st.classified, (unsigned long long)st.segments);
    fflush(stdout);
    if (rc == UTREE_E_FASTA) {
        switch (st.fasta_error.code) {                                                    /* itree.c:872, 880, 886, 888 */
            case 1: fprintf(stderr, "ERROR: can't read sequence L %llu\n", (unsigned long long)st.fasta_error.read_index); break;
            case 2: fprintf(stderr, "ERROR: no header '>' [L %llu]\n", (unsigned long long)st.fasta_error.read_index); break;
            case 3: fprintf(stderr, "ERROR: sequence begins '>' [L %llu]\n", (unsigned long long)st.fasta_error.read_index); break;
            case 4: fprintf(stderr, "ERROR: empty query line %llu\n", (unsigned long long)st.fasta_error.read_index); break;
            default: fprintf(stderr, "ERROR: query line too long\n");
        }
        exit(2);
    }
    fprintf(stderr, "[utree_amd] tiles %.3f s (%.0f tiles/s), device %.3f s, %llu batches\n", st.seconds_total,
            st.seconds_total > 0 ? (double)st.n_tiles / st.seconds_total : 0.0, st.seconds_device, (unsigned long long)st.n_batches);
    exit(0);
}
