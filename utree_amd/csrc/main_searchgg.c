/* main_searchgg.c -- the `xtree-searchGG` command line, unchanged (itree.c:1357-1377, README.md:5-7):
 *
 *     xtree-searchGG compTree.ctr fastaToSearch.fa output.txt [threads] [SPEED <X>] [RC]
 *
 * and, compiled with -DUTREE_RANK_SPECIFIC, the rank-specific `xtree-search` (itree.c -D SEARCH; README.md:71-76),
 * whose compile-time knobs SLACK / SPARSITY / TOLERANCE_THRESHOLD (itree.c:952-960) are read from the
 * environment here: UTREE_SLACK, UTREE_SPARSITY, UTREE_TOLERANCE (defaults 2, 4, 2).  It uses one GPU.
 *
 * Same positional arguments, same stdout banners, same exit codes (0 bad/malformed DB, 1 usage or input
 * file, 2 malformed read, 3 out of memory / short tree).  New behaviour is reachable only through
 * environment variables so the command line stays bit-compatible:
 *     UTREE_GPUS=<n>        number of GPUs to use (default: all visible)
 *     UTREE_FINE_BITS=<F>   extra prefix bits of the device index (default: auto)
 *     UTREE_INPUT=auto|fastq|fasta   opt-in: FASTQ / multi-line FASTA records, plain or gzip (default: the reference's
 *                           two-lines-per-read framing, bit-compatible)
 *     UTREE_OUTPUT_PARTS=<P> opt-in: the output as P files output.txt.part000 ... (their concatenation is output.txt as the reference writes
 *                           it with one thread); ONE new file fills at ~6 GB/s on a Linux host whatever writes it, P files P times that
 *     UTREE_PROFILE=<path>  opt-in: also write the sample's per-taxon read counts to <path> (include/utree_amd.h: utree_profile_write;
 *                           the taxon of a read is the second column of its output line), counted on the GPU while it searches; stdout
 *                           and the output are those of a run without it.  A path that cannot be opened: a message on stderr, exit 1,
 *                           before the search (nothing is created there).  A profile that cannot be written after the search (the file,
 *                           a table too small: UTREE_PROFILE_CAPACITY): the usual stdout, a message on stderr, exit 1.  A search that fails
 *                           leaves the path as it was.  Unset: no profile, no extra work
 *     UTREE_COVERAGE=<path> opt-in, xtree-searchGG only (xtree-search ignores it): also write, per taxon, the k-mers the database holds, the
 *                           DISTINCT ones the sample hit and the hits (include/utree_amd.h: utree_coverage_write), collected on the GPU
 *                           while it searches; needs the node dump a second time in HBM (utree_coverage_bytes).  Path checks, failures and
 *                           exit codes as for UTREE_PROFILE, with which it may be combined.  Unset: nothing of it runs
 *     UTREE_REDISTRIBUTE=<path> opt-in, xtree-searchGG only (xtree-search ignores it): also write the sample's reads redistributed among the labels
 *                           each read hit most often (include/utree_amd.h: utree_redist_write) -- the candidate sets are collected on the GPU
 *                           while it searches, one more pass per batch, and iterated there after the search.  Path checks, failures and exit
 *                           codes as for UTREE_PROFILE, with which and with UTREE_COVERAGE / UTREE_MATES it may be combined.
 *                           UTREE_REDIST_PASSES=<1..1000> caps the passes (default 100; 1: one pass, xtree's fast mode),
 *                           UTREE_REDIST_CAPACITY=<slots> sizes the table of distinct sets (default 2^22).  Unset: nothing of it runs
 *     UTREE_REDISTRIBUTE_READS=<path> opt-in, xtree-searchGG only (xtree-search ignores it, as it ignores UTREE_REDISTRIBUTE): also write, for every
 *                           query that has a line in the output and in that order, "name \t label text \t n_candidates": the label the
 *                           redistribution assigns the read to (include/utree_amd.h: utree_redist_assign), the text whole; n_candidates 1: the
 *                           read never had another candidate.  No header; pairs print under mate 1's name.  With or without
 *                           UTREE_REDISTRIBUTE (one solve serves both files; UTREE_REDIST_PASSES and UTREE_REDIST_CAPACITY apply), and
 *                           with everything that combines with it.  The search takes the host framing pipeline and spools the reads' keys to
 *                           <path>.spool, which is removed on every way out.  Path checks, failures and exit codes as for UTREE_REDISTRIBUTE
 *     UTREE_HITMAP=<path>   opt-in, xtree-searchGG only (xtree-search says so in one line on stderr and ignores it): also write, for EVERY query, which
 *                           label each of its k-mer windows hit, in window order, as runs "code:count" (include/utree_amd.h: utree_hitmap_format),
 *                           and the label texts to <path>.labels (line i = label index i).  The map is written in step with the output, so
 *                           after a malformed record both files hold the same queries; stdout, the output and the other reports are those of a
 *                           run without it.  May be combined with UTREE_PROFILE, UTREE_COVERAGE, UTREE_REDISTRIBUTE, UTREE_MATES /
 *                           UTREE_INTERLEAVED and UTREE_INPUT.  A path that cannot be opened: a message on stderr, exit 1, before the search.
 *                           A map that cannot be written while searching: the usual stdout, a message on stderr, exit 1
 *     UTREE_SAMPLE_TABLE=<path> opt-in, both binaries: the reads file is a combined one whose records are named <sample>_<n>; also write the taxon x
 *                           sample matrix of read counts to <path> (include/utree_amd.h: utree_samples_write), the ids interned and the cells
 *                           counted on the GPU while it searches; stdout, the output, the pipeline and the other reports are those of a run
 *                           without it.  UTREE_SAMPLE_DELIM=<one byte> is the delimiter in front of <n> (default '_'; not TAB, space, CR or LF:
 *                           anything else is a message and exit 1), UTREE_SAMPLE_CAPACITY=<ids> (default 2^16) and UTREE_SAMPLE_CELLS=<slots>
 *                           (default 2^22) size the tables.  May be combined with every other variable.  Path checks as for UTREE_PROFILE.  A
 *                           file named without the convention (every read its own sample) ends after a complete search: the usual stdout, one
 *                           line on stderr that names UTREE_SAMPLE_CAPACITY, exit 1.  Unset: nothing is allocated, uploaded or launched
 *     UTREE_SAMPLE_REDISTRIBUTE=<path> opt-in, xtree-searchGG only (xtree-search ignores it, as it ignores UTREE_REDISTRIBUTE): also write the taxon x
 *                           sample matrix with every sample's ambiguous reads redistributed WITHIN that sample (include/utree_amd.h:
 *                           utree_sredist_write) -- the cells (sample, candidate set) are counted on the GPU while it searches, one more pass
 *                           per batch, and every sample iterated there after the search.  Sample ids, UTREE_SAMPLE_DELIM, UTREE_SAMPLE_CAPACITY
 *                           and UTREE_SAMPLE_CELLS as for UTREE_SAMPLE_TABLE, UTREE_REDIST_PASSES and UTREE_REDIST_CAPACITY as for
 *                           UTREE_REDISTRIBUTE; may be combined with every other variable; path checks and the ending of a file named without
 *                           the convention as for UTREE_SAMPLE_TABLE.  Unset: nothing is allocated, uploaded or launched
 *     UTREE_MATES=<path>    opt-in, xtree-searchGG only: paired-end reads.  fastaToSearch.fa holds the first mates, <path> the second; pair i is
 *                           record i of both.  A pair is searched as ONE query, mate 1 + "N" + mate 2, and prints one line under mate 1's name
 *                           (include/utree_amd.h: utree_search_request; mate names are not compared); "Searched N queries" and the profile
 *                           count pairs.  Works with UTREE_INPUT, UTREE_PROFILE and UTREE_COVERAGE.  A mates file that cannot be opened:
 *                           "Invalid input files", exit 1, before the tree is loaded.  Files of unequal record counts: the complete pairs are
 *                           written, a message on stderr, exit 2
 *     UTREE_INTERLEAVED=1   opt-in, xtree-searchGG only: fastaToSearch.fa holds both mates, records 2i and 2i+1 are pair i.  Setting both
 *                           variables is an error (exit 1); xtree-search reads no pairs and exits with 1 when either is set
 * `threads` sizes the host formatting team (the GPU does the search).  `SPEED` is parsed and ignored, as
 * in the reference (itree.c:858, 907-918).
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#ifdef _OPENMP
#include <omp.h>
#endif
#include "../../include/utree_amd.h"

#define VER "[v2.0RF SigNature Edition]"          /* itree.c:1350 */
#ifdef UTREE_RANK_SPECIFIC
#define DO_GG 0
#else
#define DO_GG 1
#endif
static const char *TYPEARR[17] = {"NA", "uint8_t", "uint16_t", "NA", "uint32_t", "NA", "NA", "NA", "uint64_t", "NA", "NA",
                                  "NA", "NA", "NA", "NA", "NA", "__uint128_t"};

/* can the report file `path` be opened for writing?  Else a message and exit 1.  Nothing is created or changed here: a search that fails leaves
 * the path as it was (the file is written after a successful search) */
static void check_report_path(const char *path, const char *what) {
    int f = open(path, O_WRONLY | O_CREAT | O_EXCL, 0644);
    const int created = f >= 0;
    if (f < 0 && errno == EEXIST) f = open(path, O_WRONLY);
    if (f < 0) { fprintf(stderr, "ERROR: cannot open the %s file %s: %s\n", what, path, strerror(errno)); exit(1); }
    close(f);
    if (created) unlink(path);
}

int main(int argc, char *argv[]) {
    if (argc < 4) {                                                                       /* itree.c:1358-1360 */
        printf(VER " usage: xtree-search%s compTree.ctr fastaToSearch.fa output.txt [threads] [SPEED <X>] [RC]\n", DO_GG ? "GG" : "");
        exit(1);
    }
    printf("This is UTree " VER "\n");
    int doRC = !strcmp(argv[argc - 1], "RC"), threads = 1;                                /* itree.c:1362-1364 */
    argc -= doRC;
    int speed = 0;
    if (!strcmp(argv[argc - 2], "SPEED")) speed = atoi(argv[argc - 1]), argc -= 2;
    printf("Reverse complement consideration is %sabled.\n", doRC ? "en" : "dis");
    printf("Searching at speed %d.\n", speed);
#ifdef _OPENMP
    threads = argc >= 5 ? atoi(argv[4]) : omp_get_max_threads();                          /* itree.c:1368-1370 */
#else
    threads = argc >= 5 ? atoi(argv[4]) : 1;
#endif
    printf("Using up to %d threads.\n", threads);

    /* everything the environment asks for goes into ONE request; what the rank-specific search has no use for is not read (or, where a user
     * would wonder, refused or reported) */
    utree_search_request req = {.size = sizeof req, .do_rc = doRC, .host_threads = threads, .input_format = UTREE_INPUT_REFERENCE,
                                .reads_path = argv[2], .out_path = argv[3], .sample_delim = '_'};
    const char *mates = getenv("UTREE_MATES");
    const char *ei_pairs = getenv("UTREE_INTERLEAVED");
    const int interleaved = ei_pairs && *ei_pairs && strcmp(ei_pairs, "0");
    if (mates && !*mates) mates = NULL;
    if (!DO_GG && (mates || interleaved)) { fputs("ERROR: the rank-specific search reads no pairs (UTREE_MATES / UTREE_INTERLEAVED are for xtree-searchGG)\n", stderr); exit(1); }
    if (mates && interleaved) { fputs("ERROR: UTREE_MATES and UTREE_INTERLEAVED are both set: the mates are in a file of their own or in the reads file, not both\n", stderr); exit(1); }
    if (mates) {                                                                          /* before the tree is loaded: it may take minutes */
        int f = open(mates, O_RDONLY);
        if (f < 0) { puts("Invalid input files"); exit(1); }                             /* itree.c:835 */
        close(f);
    }
    req.mates_path = mates; req.interleaved = interleaved;
    /* the reports: a path that is unset or empty is no report; the others must be writable now */
    const char *p;
    if ((p = getenv("UTREE_PROFILE")) && *p) { check_report_path(p, "profile"); req.profile_path = p; }
    if (DO_GG && (p = getenv("UTREE_COVERAGE")) && *p) { check_report_path(p, "coverage"); req.coverage_path = p; }
    if (DO_GG && (p = getenv("UTREE_REDISTRIBUTE")) && *p) { check_report_path(p, "redistribution"); req.redistribute_path = p; }
    if (DO_GG && (p = getenv("UTREE_SAMPLE_REDISTRIBUTE")) && *p) { check_report_path(p, "sample redistribution"); req.sample_redistribute_path = p; }
    if (DO_GG && (p = getenv("UTREE_REDISTRIBUTE_READS")) && *p) { check_report_path(p, "redistributed reads"); req.redistribute_reads_path = p; }
    if ((req.redistribute_path || req.sample_redistribute_path || req.redistribute_reads_path) && getenv("UTREE_REDIST_PASSES")) {   /* (else 0: the default) */
        const long v = atol(getenv("UTREE_REDIST_PASSES"));
        if (v < 1 || v > 1000) { fputs("ERROR: UTREE_REDIST_PASSES must be 1 .. 1000\n", stderr); exit(1); }
        req.max_passes = (uint32_t)v;
    }
    if ((p = getenv("UTREE_HITMAP")) && *p) {
        if (DO_GG) { check_report_path(p, "hit map"); req.hitmap_path = p; }
        else fputs("[utree_amd] UTREE_HITMAP is ignored: the rank-specific search looks at a hit-dependent subset of windows and has no hit map\n", stderr);
    }
    if ((p = getenv("UTREE_SAMPLE_TABLE")) && *p) { check_report_path(p, "sample table"); req.samples_path = p; }
    const char *sd = getenv("UTREE_SAMPLE_DELIM");
    if (sd) {
        if (strlen(sd) != 1 || sd[0] == '\t' || sd[0] == ' ' || sd[0] == '\r' || sd[0] == '\n') {
            fputs("ERROR: UTREE_SAMPLE_DELIM must be one byte, and not TAB, space, CR or LF\n", stderr); exit(1);
        }
        req.sample_delim = (unsigned char)sd[0];
    }

    utree_ctr *ctr = NULL;
    int rc = utree_ctr_open(argv[1], &ctr);
    if (rc == UTREE_E_IO) { puts("Invalid DB file"); exit(0); }                          /* itree.c:735 */
    if (rc == UTREE_E_FORMAT) { puts("Tree malformatted."); exit(0); }                   /* itree.c:738 */
    if (rc == UTREE_E_UNSUPPORTED) {
        /* the reference's own words for a tree its build does not read (itree.c:746-751): what the header asks for */
        uint64_t md[4] = {0, 0, 0, 0};
        FILE *dp = fopen(argv[1], "rb");
        if (dp) { if (fread(md, sizeof *md, 4, dp) != 4) md[0] = 0; fclose(dp); }
        printf("ERROR. Input tree requires PACKSIZE=%u, CNTTYPE=%s, IXTYPE=%s\n", (unsigned)(md[0] << 2), md[1] <= 16 ? TYPEARR[md[1]] : "NA", md[2] <= 16 ? TYPEARR[md[2]] : "NA");
        exit(0);
    }
    if (rc == UTREE_E_NOLABELS) { puts("No annotation found in tree file."); exit(0); }   /* itree.c:776 */
    if (rc) { fprintf(stderr, "%s\n", utree_strerror(rc)); exit(3); }
    utree_ctr_info ci;
    utree_ctr_get_info(ctr, &ci);
    if (ci.binix_width == 4) puts("Using 32-bit counters");                              /* itree.c:754-755 */
    else puts("Holey smokes, a tree of over 4 billion k-mers. Here goes...");
    printf("%llu elements read.\n", (unsigned long long)((1u << 24) + 1));                /* itree.c:761 */
    printf("Nodes in input tree: %llu (PACKSIZE=%u, CNTTYPE=%s, IXTYPE=%s, SZ=%d)\n", (unsigned long long)ci.n_nodes,
           ci.W << 2, TYPEARR[0], TYPEARR[ci.I], (int)ci.SZ);                             /* itree.c:764-765 */

    int n_vis = 0;
    if (hipGetDeviceCount(&n_vis) != hipSuccess || n_vis < 1) { fputs("ERROR: no gfx950 device visible\n", stderr); exit(3); }
    int n_dev = n_vis;
    const char *eg = getenv("UTREE_GPUS");
    if (eg && atoi(eg) > 0 && atoi(eg) < n_dev) n_dev = atoi(eg);
    if (!DO_GG) n_dev = 1;                                                                /* reads depend on their predecessors */
    utree_dev **devs = (utree_dev **)calloc((size_t)n_dev, sizeof(utree_dev *));
    int *ids = (int *)calloc((size_t)n_dev, sizeof(int));
    for (int i = 0; i < n_dev; ++i) ids[i] = i;
    rc = utree_dev_upload(ctr, 0, UTREE_FINE_AUTO, &devs[0]);
    if (rc == UTREE_E_FORMAT) { puts("Error in reading tree."); exit(3); }                /* itree.c:768 */
    if (rc) { fprintf(stderr, "ERROR: device image: %s\n", utree_strerror(rc)); exit(3); }
    printf("Read %llu nodes.\n", (unsigned long long)ci.n_nodes);                         /* itree.c:769 */
    if (ci.bin_total != ci.n_nodes)                                                       /* itree.c:792-793 */
        printf("Warning: detected nodes %u != %u\n", (unsigned)ci.bin_total, (unsigned)ci.n_nodes);
    utree_dev *built = devs[0];
    int how = UTREE_FANOUT_NONE;
    rc = utree_dev_fanout(ctr, built, ids, n_dev, UTREE_FINE_AUTO, devs, &how);           /* RCCL broadcast; on failure every GPU loads over PCIe */
    if (rc) { fprintf(stderr, "ERROR: tree on %d GPUs: %s\n", n_dev, utree_strerror(rc)); exit(3); }
    if (how == UTREE_FANOUT_BROADCAST)
        fprintf(stderr, "[utree_amd] tree replicated to %d GPU(s) by RCCL broadcast in %.3f s\n", n_dev, utree_dev_replicate_seconds());
#ifndef UTREE_RANK_SPECIFIC
    { int prc = utree_search_prepare(ctr, devs, n_dev, doRC);
      if (prc) fprintf(stderr, "[utree_amd] warning: the search buffers could not be allocated ahead (%s); the search allocates them itself\n", utree_strerror(prc)); }                                   /* the search's pinned / device buffers: part of "database resident" */
#endif
    puts("Tree read.");                                                                   /* itree.c:826 */
    utree_dev_info di;
    utree_dev_get_info(devs[0], &di);
    fprintf(stderr, "[utree_amd] %d GPU(s), image %.2f GiB, fine_bits=%u, irregular bins=%llu%s\n", n_dev,
            (double)di.image_bytes / 1073741824.0, di.fine_bits, (unsigned long long)di.irregular_bins,
            di.generic_mode ? " (generic mode)" : "");
    fflush(stdout);

    utree_search_stats st;
    const char *ei = getenv("UTREE_INPUT");
    if (ei && !strcmp(ei, "auto")) req.input_format = UTREE_INPUT_AUTO;
    else if (ei && !strcmp(ei, "fastq")) req.input_format = UTREE_INPUT_FASTQ;
    else if (ei && !strcmp(ei, "fasta")) req.input_format = UTREE_INPUT_FASTA_MULTILINE;
#ifdef UTREE_RANK_SPECIFIC
    utree_rank_params prm;
    utree_rank_params_default(&prm);
    if (getenv("UTREE_SLACK")) prm.slack = (uint32_t)atoi(getenv("UTREE_SLACK"));
    if (getenv("UTREE_SPARSITY")) prm.sparsity = (uint32_t)atoi(getenv("UTREE_SPARSITY"));
    if (getenv("UTREE_TOLERANCE")) prm.tolerance = (uint32_t)atoi(getenv("UTREE_TOLERANCE"));
    req.rank = &prm;
#endif
    rc = utree_search_run(ctr, devs, n_dev, &req, &st);
    if (rc == UTREE_E_IO) { puts("Invalid input files"); exit(1); }                      /* itree.c:835 */
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
    if (rc == UTREE_E_PAIRS) { fprintf(stderr, "ERROR: %s\n", utree_last_hip_error()); exit(2); }   /* the complete pairs are written */
    if (rc && rc != UTREE_E_PROFILE && rc != UTREE_E_COVERAGE && rc != UTREE_E_HITMAP) { fprintf(stderr, "ERROR: %s\n", utree_strerror(rc)); exit(3); }
    printf("Good finds: %llu\n", (unsigned long long)st.good_finds);                      /* itree.c:1106 */
    printf("Searched %llu queries\n", (unsigned long long)st.n_reads);                    /* itree.c:1375 */
    fprintf(stderr, "[utree_amd] search %.3f s (%.0f reads/s), GPU batches %.3f s%s\n", st.seconds_total,
            st.seconds_total > 0 ? (double)st.n_reads / st.seconds_total : 0.0, st.seconds_kernels,
            st.pipeline ? " (lane-seconds; framing and formatting on the GPU)" : "");
    if (rc == UTREE_E_PROFILE || rc == UTREE_E_COVERAGE || rc == UTREE_E_HITMAP) fprintf(stderr, "ERROR: %s\n", utree_last_hip_error());    /* the search and its output are complete; the profile / redistribution / coverage file is not */
    for (int i = n_dev - 1; i >= 0; --i) utree_dev_free(devs[i]);
    if (devs[0] != built) utree_dev_free(built);                                          /* UTREE_RCCL_FORCE: devs[0] was a replica */
    utree_ctr_close(ctr);
    exit(rc == UTREE_E_PROFILE || rc == UTREE_E_COVERAGE || rc == UTREE_E_HITMAP ? 1 : 0);
}
