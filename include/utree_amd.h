/* utree_amd.h -- C-ABI of the MI355X-native SEARCH_GG path (libutree_amd.so).
 *
 * Drop-in boundary for ONE path of knights-lab/UTree: `xtree-searchGG` (itree.c compiled -D SEARCH_GG).
 * The reference has no FFI; its path sits behind two internal C seams and one operator:
 *
 *     UTree *XT_read32(char *db, char delim)                                   itree.c:733
 *     size_t XT_doSearch32(UTree*, char *in, char *out, int doCollapse(=8),
 *                          int lv(ignored), int doRC)                          itree.c:833
 *     IXTYPE XT_getIX32(UTree*, WTYPE word)                                    itree.c:720
 *
 * Every entry point below names the seam / lines it replaces.  Conventions:
 *   - plain pointers and sizes only; `d_` = device (HBM) pointer, `h_` = host pointer;
 *   - nothing calls exit(): functions return UTREE_OK or an error code; the CLI (xtree-searchGG) maps the
 *     codes to the reference's exit codes and messages;
 *   - `.ctr` files are consumed unchanged (layout: itree.c:1301-1313 writer, 736-775 reader);
 *   - PACKSIZE / IXTYPE are compile-time in the reference (itree.c:35-70) and run-time here: W in {4,8,16}
 *     (k = 16, 32, 64: every PACKSIZE the reference compiles with, README.md:87-88) and I in {2,4} are dispatched from the file
 *     header; PACKSIZE=16 trees are built (utree_build_file with W = 4), compressed and searched both ways (GG and rank-specific);
 *   - there is no CPU fallback: every compute entry point needs a gfx950 device and fails with
 *     UTREE_E_HIP otherwise.
 */
#ifndef UTREE_AMD_H
#define UTREE_AMD_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define UTREE_ABI_VERSION 4

enum {
    UTREE_OK = 0,
    UTREE_E_IO = 1,          /* cannot open / read ("Invalid DB file", itree.c:735; "Invalid input files", 835) */
    UTREE_E_FORMAT = 2,      /* "Tree malformatted." (738), short bin table / node dump (768)                   */
    UTREE_E_UNSUPPORTED = 3, /* header names a W / count / I this build has no kernel for (746-751)             */
    UTREE_E_NOMEM = 4,       /* host or device allocation failed (862, 1018)                                    */
    UTREE_E_HIP = 5,         /* HIP runtime error, or no gfx950 device                                          */
    UTREE_E_ARG = 6,         /* bad argument                                                                    */
    UTREE_E_NOLABELS = 7,    /* no label text after the node dump ("No annotation found in tree file.", 776)    */
    UTREE_E_FASTA = 8,       /* malformed read: details in utree_fasta_error (872, 880, 886, 888 -> exit 2)     */
    UTREE_E_RCCL = 9,
    UTREE_E_BUILD = 10,      /* BUILD input rejected: details in utree_build_stats.error_kind                   */
    UTREE_E_DEVICE = 11,     /* a batch's kernels found the workspace too small for it (utree_classify_poll)    */
    UTREE_E_PROFILE = 12,    /* the search itself succeeded, its profile was not written: utree_last_hip_error
                                says why (utree_search_file_profile)                                            */
    UTREE_E_COVERAGE = 13,   /* ... its coverage file was not written (utree_search_file_coverage)              */
    UTREE_E_PAIRS = 14,      /* paired input: one file holds fewer records than the other, or an interleaved file an
                                odd number; the complete pairs in front were classified and written, and
                                utree_last_hip_error names the shorter file (utree_search_pairs_file)            */
    UTREE_E_HITMAP = 15      /* ... its hit map was not written (utree_search_file_hitmap): utree_last_hip_error says why.
                                utree_strerror keeps its catch-all text for this code; the cause is in that message */
};

const char *utree_strerror(int code);
/* what the calling thread's last UTREE_E_HIP / UTREE_E_DEVICE was: the failing HIP call and the runtime's message for it (no
 * counterpart in the reference, which has no device; "" when there was none); after UTREE_E_PROFILE / UTREE_E_COVERAGE, why the
 * file (profile, redistribution, coverage) was not written; after UTREE_E_PAIRS, which file ended first */
const char *utree_last_hip_error(void);
int utree_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * Host side of the database: header, bin table, labels.   Replaces XT_read32 (itree.c:733-828) and
 * readSamplesFPdelim (itree.c:1154-1223).  The node dump is NOT copied to host memory: it is streamed
 * from the file to HBM by utree_dev_upload.
 * ---------------------------------------------------------------------------------------------- */
typedef struct utree_ctr utree_ctr;

typedef struct {
    uint32_t W;            /* bytes per packed k-mer word: header[0] (4 => k=16, 8 => k=32, 16 => k=64)  */
    uint32_t I;            /* bytes per label index:       header[2]                                     */
    uint32_t k;            /* 4*W                                                                        */
    uint32_t SZ;           /* bytes per stored record = W + I - 3 (itree.c:691)                           */
    uint64_t n_nodes;      /* header[3]                                                                  */
    uint32_t n_labels;     /* distinct labels, = maxIX (itree.c:855)                                      */
    uint32_t binix_width;  /* 4 iff n_nodes < UINT32_MAX else 8 (itree.c:757)                             */
    uint64_t bin_total;    /* last bin-table entry; the reference only warns if != n_nodes (792-793)      */
    uint64_t file_bytes;
} utree_ctr_info;

int utree_ctr_open(const char *path, utree_ctr **out);
/* Same object from pieces already in memory (synthetic DBs, tests). `binix` has 2^24+1 entries of
 * `binix_width` bytes; `h_records` (n_nodes*SZ bytes) may be NULL when the records are handed over on the
 * device (utree_dev_build).  `label_text` is the file tail verbatim.  Everything given is copied. */
int utree_ctr_from_memory(uint32_t W, uint32_t I, uint64_t n_nodes, const void *binix, uint32_t binix_width,
                          const void *h_records, const char *label_text, size_t label_len, utree_ctr **out);
void utree_ctr_close(utree_ctr *ctr);
int utree_ctr_get_info(const utree_ctr *ctr, utree_ctr_info *info);
/* Label text by file-order index (UTree.SampStrings[ix], itree.c:134,856). NULL when ix >= n_labels. */
const char *utree_ctr_label(const utree_ctr *ctr, uint32_t ix, uint32_t *len);

/* ------------------------------------------------------------------------------------------------
 * Device image: one flat HBM allocation holding the table of 64-byte buckets addressed by (canonical) minimizer hash and orientation, the
 * 8-byte-aligned records, the labels in strcmp order and the rank tables (layout: DESIGN.md §3).  It replaces UTree.Dump / UTree.BinIx
 * (itree.c:140-141) as seen by XT_getIX32.  Because it is flat and position independent, ONE RCCL
 * broadcast replicates a database to the other GPUs of a node.
 * ---------------------------------------------------------------------------------------------- */
typedef struct utree_dev utree_dev;

#define UTREE_FINE_AUTO (-1)

/* Bytes of HBM the image needs for `ctr`.  `fine_bits` (0..8) bounds the width of a bucket from below, 2^(8-fine_bits)
 * hash values: UTREE_FINE_AUTO = 8 unless the table would exceed UTREE_TABLE_MAX_GB (default 96; then the largest value that
 * fits).  k = 64 at fine_bits 8: where one hash value still holds more nodes than a bucket its slot is several pairs of buckets
 *  as long as the table stays within the same cap -- 47 GiB for 568 M 64-mers (8.5 GB on disk). */
size_t utree_dev_image_bytes(const utree_ctr *ctr, int fine_bits);
/* Stream the node dump (from the .ctr file or the host copy given to utree_ctr_from_memory) to `device`
 * and build the image there. */
int utree_dev_upload(const utree_ctr *ctr, int device, int fine_bits, utree_dev **out);
/* seconds of the calling process's last utree_dev_upload: {device + image allocation and labels, node dump file -> pinned memory -> HBM
 * (repacked as it arrives), bin-table check + minimizer sort + buckets, all of it} -- XT_read32's time (itree.c:733-828) has no such split */
int utree_dev_upload_seconds(double *h_out4);
/* Build from raw on-disk pieces that already sit in HBM on `device`: `d_binix` = (2^24+1) entries of
 * ctr's binix_width, `d_records` = n_nodes*SZ packed bytes.  If `d_image` is non-NULL it must have
 * utree_dev_image_bytes() bytes and the image is built in place (caller-owned, e.g. a torch tensor). */
int utree_dev_build(const utree_ctr *ctr, int device, int fine_bits, const void *d_binix, const void *d_records,
                    void *d_image, size_t image_bytes, void *stream, utree_dev **out);
/* The flat image (for ncclBroadcast / torch.distributed.broadcast) ... */
int utree_dev_image(const utree_dev *dev, void **d_image, size_t *bytes);
/* ... and adopting a received copy on another device (not owned by the handle). */
int utree_dev_attach(const utree_ctr *ctr, int device, void *d_image, size_t bytes, utree_dev **out);
void utree_dev_free(utree_dev *dev);

typedef struct {
    uint32_t fine_bits;
    uint32_t record_bytes;      /* bytes per in-HBM record (8, 16 or 24)                                 */
    uint64_t image_bytes;
    uint64_t irregular_bins;    /* bins not strictly ascending (e.g. COMPRESS' first-bin quirk): searched
                                   with the reference's exact probe sequence                             */
    uint32_t generic_mode;      /* 1: bin table not monotone -> every lookup uses the exact probe path   */
    int32_t  device;
    uint32_t vote_table;        /* 1: the image carries the label table the vote decides from (every label
                                   has at most 8 ';'-separated tokens and 255 bytes, 16-bit label indices)   */
    uint32_t lane_pass;         /* 1: the lane-per-read classify kernels take this image (else the
                                   wave-per-read kernels: k = 64 with 32-bit labels, many irregular bins)   */
    uint32_t bucket_bytes;      /* 64 (default) or 128 (UTREE_BUCKET_BYTES=128 when the image is built: a third
                                   less HBM, classify kernels 5-10 % slower); 0: a PACKSIZE=16 tree, whose image is a
                                   direct-address table of all 2^32 words' answers                         */
    uint32_t strand_views;      /* 1: the image stores every k-mer under its mirrored minimizer view too (where that differs), so a
                                   search with RC finds a window and its reverse complement in ONE pass over the read: both are
                                   in the two buckets of one pair                     */
    uint32_t overflow_chains;   /* 1: heavy overflow runs (one minimizer's k-mers in many related genomes) are stored as chains of
                                   consecutive k-mers (k = 32); 0 with UTREE_OVF_CHAINS=0 at build time  (ABI 4) */
    uint32_t pad0;
    uint64_t overflow_bytes;    /* bytes of the image's overflow area                                         (ABI 4) */
} utree_dev_info;
int utree_dev_get_info(const utree_dev *dev, utree_dev_info *info);

/* Replicate dev0's image to the other devices by ncclBroadcast (RCCL over xGMI; pieces of at most 1 GiB) and attach it
 * there: what the reference's worker team gets by sharing one UTree in host memory (itree.c:1009-1018).  devices[0] must be
 * dev0's device, no device twice.  out[0] = dev0; out[1..] own their replicas; on failure nothing is handed back.
 * Rehearsal on one GPU: with UTREE_RCCL_FORCE=1 in the environment n_devices == 1 still builds the communicator and sends the
 * image through ncclBroadcast into a second allocation on the same card, and out[0] is a NEW handle owning that replica
 * (the caller still owns dev0). */
int utree_dev_replicate(const utree_ctr *ctr, utree_dev *dev0, const int *devices, int n_devices, utree_dev **out);
/* seconds the calling process's last utree_dev_replicate / utree_dev_replicate_rank spent between the first ncclBroadcast of
 * the image and the drained streams (0 when it had nothing to send) */
double utree_dev_replicate_seconds(void);
/* What the command line does with n_devices > 1: utree_dev_replicate; if that fails, a warning on stderr and
 * utree_dev_upload(ctr, devices[i], fine_bits) for every other device -- each GPU then reads the database from the host over
 * PCIe.  *how (may be NULL) says which it was. */
enum { UTREE_FANOUT_NONE = 0, UTREE_FANOUT_BROADCAST = 1, UTREE_FANOUT_UPLOAD = 2 };
int utree_dev_fanout(const utree_ctr *ctr, utree_dev *dev0, const int *devices, int n_devices, int fine_bits, utree_dev **out, int *how);
/* the same with the two steps passed in (utree_dev_fanout passes utree_dev_replicate and utree_dev_upload): the seam the
 * fallback branch is tested through on a machine without a GPU */
typedef int (*utree_replicate_fn)(const utree_ctr *, utree_dev *, const int *, int, utree_dev **);
typedef int (*utree_upload_fn)(const utree_ctr *, int, int, utree_dev **);
int utree_dev_fanout_with(const utree_ctr *ctr, utree_dev *dev0, const int *devices, int n_devices, int fine_bits, utree_dev **out, int *how,
                          utree_replicate_fn replicate, utree_upload_fn upload);
/* The same broadcast with one PROCESS per GPU: the root makes an id (utree_rccl_unique_id, UTREE_RCCL_ID_BYTES bytes) and hands
 * it to the other ranks over the launcher's control channel; every rank then calls utree_dev_replicate_rank with its own
 * device.  Root: dev0 = its image, *out = dev0.  Others: dev0 = NULL, `ctr` may describe the database (checked against the
 * image header) or be NULL; *out = a handle that owns the received copy.  UTREE_RCCL_FORCE=1: world == 1 runs the whole
 * sequence on a communicator of one rank and *out owns a replica on the same card, as for utree_dev_replicate. */
#define UTREE_RCCL_ID_BYTES 128
int utree_rccl_unique_id(void *id_out, size_t cap);
int utree_dev_replicate_rank(const utree_ctr *ctr, utree_dev *dev0, int device, int rank, int world, int root, const void *id_bytes,
                             size_t id_len, utree_dev **out);

/* ------------------------------------------------------------------------------------------------
 * The hot path.  Replaces, for a batch of reads, the body of XT_doSearch32's GG branch:
 *   reverse-complement append (itree.c:891-898), k-mer roller XT_WORD_SEARCH (903-933), node lookup
 *   XT_getIX32 (720-730, 699-707), hit filter (929-931), tally (1031-1040), sort (1041), vote (1044-1088).
 * One utree_result per read, in input order.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    uint32_t label;   /* file-order label index whose text is printed (Tax_Cnt[ed-1] / first hit)          */
    int32_t  cut;     /* -2: whole label; -1: empty taxon; >=0: first `cut` bytes of the label (1087-1088)  */
    uint32_t found;   /* foundUniq; 0 => the reference prints no line for this read (1028)                  */
    uint32_t uix;     /* distinct labels among the hits; 1 => "*" instead of "sl;ol" (1032, 1040)           */
    uint32_t sl, ol;  /* support pair of the last level examined (1071)                                     */
} utree_result;

/* Device workspace a batch needs (tally lists, vote worklist). */
size_t utree_classify_workspace_bytes(const utree_dev *dev, uint32_t n_reads, uint64_t total_bases, uint32_t max_len,
                                      int do_rc);
/* d_bases: raw sequence bytes as they stand in the FASTA (any case, any byte); read r is
 * d_bases[d_off[r] .. d_off[r]+d_len[r]).  total_bases = sum of d_len, max_len = max of d_len (both are
 * by-products of framing; they size the workspace and select the long-read kernel).  Asynchronous on
 * `stream` (a hipStream_t, NULL = default stream); d_out is valid once the stream has drained. */
int utree_classify_batch(utree_dev *dev, const uint8_t *d_bases, const uint64_t *d_off, const uint32_t *d_len,
                         uint32_t n_reads, uint64_t total_bases, uint32_t max_len, int do_rc, utree_result *d_out,
                         void *d_workspace, size_t workspace_bytes, void *stream);
/* A batch's kernels check what the workspace's sizing rules out -- (rank, count) lists past their capacity, more long reads or
 * pieces of long reads than the tables hold: total_bases / max_len did not describe the batch -- and report it in an error word
 * that comes back with the batch (no kernel writes past a buffer, none drops a read silently).  Once `stream` has drained,
 * utree_classify_poll returns UTREE_E_DEVICE if a batch finished since the last call reported something (its results are not to
 * be used; utree_last_hip_error says what), else UTREE_OK.  utree_classify_batch also returns UTREE_E_DEVICE when an EARLIER
 * batch's report has arrived by the time it is called (the new batch has been launched all the same; the condition stays until
 * utree_classify_poll has returned it once).  utree_search_file polls after every chunk. */
int utree_classify_poll(utree_dev *dev);
/* The innermost operator alone (XT_getIX32, itree.c:720): words (hi:lo, hi = 0 for k = 32) -> stored label
 * index, 0xFFFFFFFF when absent or when the stored index is >= n_labels.  For tests and micro-benchmarks. */
int utree_lookup_words(utree_dev *dev, const uint64_t *d_hi, const uint64_t *d_lo, uint64_t n, uint32_t *d_ix,
                       void *stream);
/* Name of the dominant kernel as rocprofv3 reports it and the wall time (ms) HIP events measured around
 * its launches since the last call with reset != 0 (bench.py's roofline leg). */
const char *utree_classify_kernel_name(const utree_dev *dev);
/* Measurement aid for the byte model of the bucketed image (bench.py, DESIGN.md sections 4 and 6): over the reads of up to 640 staged
 * bases, h_counts5 = { reads, valid k-mer windows, distinct 64-byte buckets per read (summed), distinct 128-byte HBM lines per
 * read (summed), distinct buckets that carry an overflow descriptor }.  Synchronous.  Evaluated window by window with the
 * load-time minimizer code, independently of the search kernels' sliding minimum. */
int utree_model_counts(utree_dev *dev, const uint8_t *d_bases, const uint64_t *d_off, const uint32_t *d_len, uint32_t n_reads,
                       int do_rc, uint64_t *h_counts5, void *stream);
int utree_classify_kernel_time(utree_dev *dev, int reset, double *ms_total, uint64_t *launches);

/* ------------------------------------------------------------------------------------------------
 * Host framing and formatting.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int      code;        /* 0, or the reference's condition: 1 can't read sequence (872), 2 no header '>'
                             (880), 3 sequence begins '>' (886), 4 empty query line (888)                 */
    uint64_t read_index;  /* 1-based read number as the reference prints it                               */
} utree_fasta_error;

/* Frame reads in h_buf[0..n) exactly as XT_INITIATE_WS does with two fgets per read (itree.c:866-890):
 * name = bytes after '>' up to the first space / newline / NUL; sequence = next line minus one '\n' then
 * one '\r'.  When `final` is 0 an incomplete trailing read is left for the next call (*consumed < n).
 * Arrays must hold max_reads entries.  Returns UTREE_OK or UTREE_E_FASTA (reads framed before the bad one
 * are still returned, as the reference classifies them before it exits). */
int utree_fasta_frame(const uint8_t *h_buf, size_t n, int final, size_t max_reads, uint64_t *seq_off,
                      uint32_t *seq_len, uint64_t *name_off, uint32_t *name_len, size_t *n_reads,
                      size_t *consumed, utree_fasta_error *err);
/* Output lines (itree.c:1032, 1040, 1096) for n reads into h_out; reads with found == 0 emit nothing.
 * Returns bytes written, or (size_t)-1 if cap is too small.  *good_finds += lines written (1029). */
size_t utree_format_records(const utree_ctr *ctr, const uint8_t *h_buf, const uint64_t *name_off,
                            const uint32_t *name_len, const utree_result *h_res, size_t n, char *h_out, size_t cap,
                            uint64_t *good_finds);

/* Opt-in input formats the reference does not read.  UTREE_INPUT_REFERENCE is the reference's
 * framing (utree_fasta_frame); the others frame complete records serially and, for multi-line FASTA, compact the sequence
 * lines in place.  Error codes: 1 truncated record, 2 record does not start with '@' / '>', 3 FASTQ separator line is not
 * '+', 5 sequence too long.  With a non-reference format the *_opts file functions also read gzip-compressed input.
 * These formats are not read with fgets(…, LINELEN), so no line of theirs is split: a FASTQ record whose sequence and quality
 * lines have LINELEN - 2 = 16 777 214 bytes each, plain or gzip, and a FASTA record of that many bases wrapped over lines are
 * framed whole and give the output line of the same bases as one two-line FASTA record. */
enum { UTREE_INPUT_REFERENCE = 0, UTREE_INPUT_FASTQ = 1, UTREE_INPUT_FASTA_MULTILINE = 2, UTREE_INPUT_AUTO = 3 };
int utree_reads_frame(uint8_t *h_buf, size_t n, int final, int format, size_t max_reads, uint64_t *seq_off,
                      uint32_t *seq_len, uint64_t *name_off, uint32_t *name_len, size_t *n_reads, size_t *consumed,
                      utree_fasta_error *err);

/* ------------------------------------------------------------------------------------------------
 * Whole search = XT_doSearch32(utree, in, out, 8, speed, doRC) (itree.c:833-1108, GG branch), reads
 * sharded over `n_dev` device images, output lines in input order (= the reference with 1 thread).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    uint64_t n_reads;       /* return value of XT_doSearch32: sequences parsed (itree.c:1107)             */
    uint64_t good_finds;    /* "Good finds: %llu" (1106)                                                  */
    double   seconds_total, seconds_kernels;
    utree_fasta_error fasta_error;
    /* Where the time went.  pipeline 1 = device text pipeline (framing and formatting on the GPU; the host only moves
     * bytes): the figures are LANE-seconds, summed over the n_lanes host threads that each carry one chunk at a time
     * through all stages.  pipeline 0 = host framing / formatting (rank-specific search, opt-in input formats, malformed
     * input): seconds of the four overlapped stage threads; seconds_frame = host framing, seconds_classify_format =
     * H2D + kernels + D2H, seconds_d2h = host formatting. */
    int      pipeline, n_lanes;
    double   seconds_read;              /* file -> pinned memory                                                      */
    double   seconds_frame;             /* H2D of the chunk + newline scan + framing kernels (until the host knows the read count) */
    double   seconds_classify_format;   /* classify + vote + line lengths (until the host knows the text length)      */
    double   seconds_order_wait;        /* waiting for the earlier chunks' text lengths (output offsets are in input order) and for the file (one writer at a time) */
    double   seconds_d2h;               /* format kernel + D2H of the text                                            */
    double   seconds_write;             /* pwrite                                                                     */
    uint64_t bytes_in, bytes_out;
} utree_search_stats;

/* utree_search_run (below) with reads_path = fasta_path, out_path, do_rc, host_threads set. */
int utree_search_file(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *fasta_path,
                      const char *out_path, int do_rc, int host_threads, utree_search_stats *stats);
/* Optional: allocate the search's pinned and device buffers now (they are kept in the device handles and reused by later
 * searches), so that the first search does not pay for them -- "database resident" then includes them. */
int utree_search_prepare(const utree_ctr *ctr, utree_dev **devs, int n_dev, int do_rc);
/* ... and input_format. */
int utree_search_file_opts(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path,
                           const char *out_path, int do_rc, int host_threads, int input_format, utree_search_stats *stats);

/* ------------------------------------------------------------------------------------------------
 * Rank-specific search = the `xtree-search` binary (itree.c -D SEARCH: XT_doSearch32 with doCollapse = 0,
 * itree.c:969-1007, 1376).  SURVEY.md §8(f) rank 1.  Same `.ctr`, framing, windows and node lookups as the GG
 * path; different hit selection and vote, with the reference's compile-time knobs as run-time parameters.
 *
 * Reads are NOT independent here: the reference's vote also counts one entry an earlier read left in its hit
 * array (itree.c:982), so batches must be submitted in file order, on one device image per input file; the image
 * carries that array from batch to batch.  utree_rank_reset() starts a new file.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    uint32_t slack;       /* SLACK (itree.c:955, default 2): most >= slack * secondMost, or no line               */
    uint32_t sparsity;    /* SPARSITY (itree.c:958, default 4): a hit skips PACKSIZE/sparsity - 1 windows (950)   */
    uint32_t tolerance;   /* TOLERANCE_THRESHOLD (itree.c:952, default 2): most >= tolerance, or no line          */
} utree_rank_params;
void utree_rank_params_default(utree_rank_params *p);

size_t utree_rank_workspace_bytes(const utree_dev *dev, uint32_t n_reads, uint64_t total_bases, uint32_t max_len,
                                  int do_rc, const utree_rank_params *params);
/* Arguments as utree_classify_batch.  d_out[r]: found = hits kept (foundUniq, itree.c:930), label = mostIX,
 * sl = most, ol = secondMost (itree.c:986-997), cut = -2 if the reference prints the read (1000-1002) else -4;
 * uix is 0. */
int utree_rank_batch(utree_dev *dev, const uint8_t *d_bases, const uint64_t *d_off, const uint32_t *d_len,
                     uint32_t n_reads, uint64_t total_bases, uint32_t max_len, int do_rc,
                     const utree_rank_params *params, utree_result *d_out, void *d_workspace, size_t workspace_bytes,
                     void *stream);
/* Forget the carried array (a fresh process of the reference). */
int utree_rank_reset(utree_dev *dev);
/* "name \t label \t %f \t %d \n" (itree.c:1002); same conventions as utree_format_records. */
size_t utree_format_rank_records(const utree_ctr *ctr, const uint8_t *h_buf, const uint64_t *name_off,
                                 const uint32_t *name_len, const utree_result *h_res, size_t n, char *h_out, size_t cap,
                                 uint64_t *good_finds);
/* utree_search_run with rank = params on the one handle `dev`, and reads_path, out_path, do_rc, host_threads set; _opts: and input_format. */
int utree_rank_search_file(const utree_ctr *ctr, utree_dev *dev, const char *fasta_path, const char *out_path,
                           int do_rc, const utree_rank_params *params, int host_threads, utree_search_stats *stats);
int utree_rank_search_file_opts(const utree_ctr *ctr, utree_dev *dev, const char *reads_path, const char *out_path,
                                int do_rc, const utree_rank_params *params, int host_threads, int input_format,
                                utree_search_stats *stats);

/* ------------------------------------------------------------------------------------------------
 * Per-taxon read-count profiles (no counterpart in the reference, which writes only the per-read lines).  A read's taxon is the
 * second column of its output line -- the interpolated taxonomy of the GG search (itree.c:1032, 1040, 1087-1096; it may be empty),
 * the printed label of the rank-specific one (982, 1002) -- and a read without a line is unclassified.  The counters live on ONE
 * device; a batch's utree_result records are added by one kernel pass that counts in LDS first.  Entries are
 * keyed as the records are, (label, cut): cut -2 whole label, -1 empty taxon, >= 0 the label's first `cut` bytes; different keys
 * that print the same text are merged by utree_profile_write, which also takes entries of several devices.  File layout:
 *     # reads\t<N>\tclassified\t<G>\tunclassified\t<N-G>\n
 *     # taxon\tassigned\tclade\n
 *     <s>\t<assigned>\t<clade>\n   for every assigned taxon and every ';'-prefix of one, in unsigned bytewise order (shorter first)
 * where `assigned` counts the lines that print exactly s and `clade` the lines whose taxon is s or begins with s + ";".
 * ---------------------------------------------------------------------------------------------- */
typedef struct utree_profile utree_profile;
/* Counters on dev's device for dev's labels.  `truncated_capacity`: slots of the table of truncated taxa (rounded up to a power of
 * two; 16 B of HBM each) -- keep it at twice the distinct (label, cut >= 0) keys a search can produce.  Whole labels, the empty
 * taxon and unclassified reads need no slot. */
int utree_profile_create(utree_dev *dev, uint32_t truncated_capacity, utree_profile **out);
/* Adds n_reads records (GG or rank-specific) on `stream` (a hipStream_t, NULL = default stream), asynchronously; any number of
 * streams may add to one profile at the same time. */
int utree_profile_add(utree_profile *p, const utree_result *d_res, uint32_t n_reads, void *stream);
/* Zeroes the counters (synchronous: waits for the device first). */
int utree_profile_reset(utree_profile *p);
typedef struct { uint32_t label; int32_t cut; uint64_t reads; } utree_profile_entry;
/* the most entries utree_profile_read can return for p: n_labels + table slots + 1 */
size_t utree_profile_max_entries(const utree_profile *p);
/* Synchronous (waits for the device).  Writes up to `cap` entries with reads > 0 into h and their number into *n (UTREE_E_ARG if
 * that exceeds cap); *n_reads = records added, *n_classified = records that print a line (either may be NULL).  UTREE_E_DEVICE
 * when the table of truncated taxa was too small for a batch, or a record named a label the database does not have: the counts
 * are then incomplete. */
int utree_profile_read(utree_profile *p, utree_profile_entry *h, size_t cap, size_t *n, uint64_t *n_reads, uint64_t *n_classified);
void utree_profile_free(utree_profile *p);
/* Host: entries from any number of devices (label indices of ctr) -> merged by text, rolled up, written to `path` in the layout
 * above; classified = the sum of the entries' reads. */
int utree_profile_write(const utree_ctr *ctr, const utree_profile_entry *e, size_t n, uint64_t n_reads, const char *path);
/* utree_search_file_opts / utree_rank_search_file_opts with profile_path set as well. */
int utree_search_file_profile(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path, const char *out_path,
                              int do_rc, int host_threads, int input_format, const char *profile_path, utree_search_stats *stats);
int utree_rank_search_file_profile(const utree_ctr *ctr, utree_dev *dev, const char *reads_path, const char *out_path, int do_rc,
                                   const utree_rank_params *params, int host_threads, int input_format, const char *profile_path,
                                   utree_search_stats *stats);

/* ------------------------------------------------------------------------------------------------
 * Distinct database k-mers covered per taxon (no counterpart in itree.c; the idea of KrakenUniq's and xtree's coverage reports).  A read
 * count alone does not say whether ten thousand reads pile up on forty k-mers or spread over forty thousand.  For the GG search's windows
 * (itree.c:903-927; with RC the read's and its reverse complement's), a window is a HIT when XT_getIX32 (720-730, 699-707) ends on a record
 * whose stored label index is < n_labels (929); the hit's NODE is that record's position in the dump.  Per label l:
 *     db_kmers[l]  records of the dump whose stored index is l (reachable or not)
 *     hits[l]      hit windows with label l, every occurrence
 *     covered[l]   distinct nodes among them            (covered <= db_kmers and covered <= hits, always)
 * The image cannot name a node (a k-mer may be stored there twice, in an overflow run or in a chain), so a coverage handle keeps the .ctr's
 * bin table and node dump in file order in HBM itself, plus one bit per node and one counter per label: utree_coverage_bytes -- for 1.2 G
 * 32-mers 8.5 GB of records, 64 MB of bin table and a 152 MB bitmap per device, next to the image.  File layout:
 *     # reads\t<N>\thits\t<H>\tcovered\t<D>\tdb_kmers\t<T>\n
 *     # taxon\tdb_kmers\tcovered\thits\tclade_db_kmers\tclade_covered\tclade_hits\n
 *     <s>\t...\n    for every label text with hits > 0 and every ';'-prefix of one, in unsigned bytewise order (shorter first)
 * The first three figures are those of the label(s) whose text is exactly s, the clade_ figures sum over ALL labels of the database, hit or
 * not, whose text is s or begins with s + ";".  The rank-specific search examines a hit-dependent subset of windows and has no coverage.
 * ---------------------------------------------------------------------------------------------- */
typedef struct utree_coverage utree_coverage;
/* bytes of HBM a coverage handle for ctr takes */
size_t utree_coverage_bytes(const utree_ctr *ctr);
/* A handle on dev's device.  d_binix / d_records: the raw on-disk pieces in HBM as for utree_dev_build (they are copied; the caller keeps
 * its own), or both NULL to stream the dump from the .ctr file / the host copy as utree_dev_upload does. */
int utree_coverage_create(const utree_ctr *ctr, utree_dev *dev, const void *d_binix, const void *d_records, utree_coverage **out);
/* Adds the reads of a batch, given as utree_classify_batch takes them, on `stream` (a hipStream_t, NULL = default stream), asynchronously;
 * any number of streams may add to one handle at the same time.  Reads of any length; shorter than k or empty ones count as reads. */
int utree_coverage_add(utree_coverage *c, const uint8_t *d_bases, const uint64_t *d_off, const uint32_t *d_len, uint32_t n_reads, int do_rc,
                       void *stream);
/* Clears bitmap and counters (synchronous: waits for the device first). */
int utree_coverage_reset(utree_coverage *c);
/* dst += src: bitmaps OR-ed, hit counters and reads added (synchronous; the handles may be on different devices, same database) */
int utree_coverage_merge(utree_coverage *dst, utree_coverage *src);
typedef struct { uint32_t label, pad; uint64_t db_kmers, covered, hits; } utree_coverage_entry;
/* Synchronous: one streaming pass over dump and bitmap, then ONE entry per label (index order; cap >= n_labels, else UTREE_E_ARG with
 * *n = n_labels); *n_reads = reads added, *n_hits = the sum of the entries' hits (either may be NULL). */
int utree_coverage_read(utree_coverage *c, utree_coverage_entry *h, size_t cap, size_t *n, uint64_t *n_reads, uint64_t *n_hits);
void utree_coverage_free(utree_coverage *c);
/* Host only: entries (label indices of ctr; several with one label are added up) -> merged by text, rolled up, written to `path`. */
int utree_coverage_write(const utree_ctr *ctr, const utree_coverage_entry *e, size_t n, uint64_t n_reads, const char *path);
/* utree_search_file_profile with coverage_path set as well. */
int utree_search_file_coverage(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path, const char *out_path, int do_rc,
                               int host_threads, int input_format, const char *profile_path, const char *coverage_path,
                               utree_search_stats *stats);

/* ------------------------------------------------------------------------------------------------
 * Paired-end reads: both mates of a pair cast ONE vote.  Neither the reference nor its input format knows pairs, but the reference fixes
 * what a pair's answer must be: with RC it searches read + 'N' + revcomp(read) as one query (itree.c:891-898) -- a byte that is no base
 * breaks the k-mer windows and the hits of both sides go into one list for one vote.  A pair is the same thing with the second mate in
 * the reverse complement's place:
 *   - pair i is record i of the reads file with record i of the mates file, or records 2i and 2i+1 of one interleaved file; each file is
 *     framed by the chosen UTREE_INPUT_* format's framing and its framing errors keep their codes (read_index counts that file's records);
 *   - its result, and its output line if it has one, are those of the single query named by mate 1's name whose sequence is
 *     seq1 + "N" + seq2, bytes as framed: always len1 + 1 + len2 bytes, also when a mate is empty.  With RC the existing path appends the
 *     joined query's reverse complement, so all four strands are covered;
 *   - one line per pair with found > 0, in input order, columns unchanged;
 *   - mate NAMES ARE NOT COMPARED (the /1 and /2, " 1:N:0" and " 2:N:0" conventions differ): mate 2's name is ignored;
 *   - n_reads, "Searched N queries" and the profile's "# reads" count pairs;
 *   - unequal record counts: UTREE_E_PAIRS, after the complete pairs in front were classified and written (as the reads before a
 *     malformed one are); utree_last_hip_error names the shorter file;
 *   - a pair whose joined length exceeds 16 MiB (LINELEN, itree.c:836) is the framing error "sequence too long", code 5, read_index =
 *     the pair's number;
 *   - GG search only: the rank-specific search carries state from read to read and reads no pairs.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    uint64_t total_bases;   /* joined bytes of the batch: the sum of len1 + 1 + len2                                   */
    uint32_t max_len;       /* the longest joined query                                                                */
    uint32_t error;         /* 0; 1: the joined bytes exceed joined_capacity; 2: a pair's length does not fit 32 bits --
                               then no joined byte was written and d_joff / d_jlen are not to be used                  */
} utree_pairs_meta;
/* The device join in front of utree_classify_batch: for pair i, d_joined[d_joff[i] .. d_joff[i] + d_jlen[i]) = mate 1's bytes, 'N', mate
 * 2's bytes, with d_jlen[i] = d_len1[i] + 1 + d_len2[i] and tight offsets (d_joff[0] = 0).  Mates are given as utree_classify_batch takes
 * reads, at any alignment and in any order; both mate buffers may be the same buffer.  The caller sizes d_joined as total1 + total2 +
 * n_pairs bytes (= joined_capacity) and d_joff / d_jlen for n_pairs entries; *d_meta (device memory) is filled on the way.  No byte at or
 * beyond the joined total is written; a capacity that is too small sets meta.error and writes nothing.  Asynchronous on `stream` (a
 * hipStream_t, NULL = default stream). */
int utree_pairs_join(utree_dev *dev, const uint8_t *d_bases1, const uint64_t *d_off1, const uint32_t *d_len1, const uint8_t *d_bases2,
                     const uint64_t *d_off2, const uint32_t *d_len2, uint32_t n_pairs, uint8_t *d_joined, uint64_t joined_capacity,
                     uint64_t *d_joff, uint32_t *d_jlen, utree_pairs_meta *d_meta, void *stream);
/* utree_search_file_coverage with mates_path set as well, or -- mates_path NULL -- interleaved = 1. */
int utree_search_pairs_file(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path, const char *mates_path,
                            const char *out_path, int do_rc, int host_threads, int input_format, const char *profile_path,
                            const char *coverage_path, utree_search_stats *stats);

/* ------------------------------------------------------------------------------------------------
 * Redistribution of ambiguous reads among tied labels (no counterpart in itree.c; the "capitalist redistribution" of the same author's
 * xtree, xtree.c:1190-1234 and 1321-1403, which the reference's README names as the condition of its recall claim: "after Bracken-like
 * redistribution of lower-rank hits").  The vote interpolates a read that hits two sibling species three times each to their genus; this
 * step instead keeps the labels a read hit most often and lets the sample decide among them.  GG search only.
 *   Hits.  For a read (or a joined pair; with RC the read + 'N' + its reverse complement) a window is a HIT when XT_getIX32 ends on a record
 *     whose stored label index is < n_labels, as for the coverage above; c[l] = hit windows with file-order label index l.
 *   Candidates.  A read's candidate SET is { l : c[l] == max c }: none without a hit (the read stays unclassified), exactly the label of a
 *     read with one distinct label, no cap on the size.  Labels are label INDICES: two indices with one text are two labels until the file
 *     is written.
 *   Passes.  N = reads searched (a pair counts once), T0[l] = reads whose set contains l.  win(S, T) = the l in S with the largest T[l], the
 *     SMALLEST file-order index among equal tallies.  Pass p = 1, 2, ... computes T_p[l] = reads with win(S, T_{p-1}) == l and
 *     changes_p = sum over l of |T_p[l] - T_{p-1}[l]|; passes run while p <= max_passes and, after the first, while the previous
 *     changes > N / 100000 (integer division, xtree.c:1360-1362).  At least one pass runs; max_passes = 1 is xtree's fast mode.  With P
 *     passes run, assigned[l] = reads with win(S, T_P) == l (the final assignment of xtree.c:1389-1398: one more evaluation, not T_P itself),
 *     unique[l] = reads whose set is exactly {l}, ambiguous = reads with more than one candidate.
 *   xtree's special case for an empty taxonomy string (firstIx) is NOT taken over: a label is a label.
 * File layout (labels of equal text merged at write time, as the profile does; keyed on `assigned`):
 *     # reads\t<N>\tclassified\t<G>\tunclassified\t<N-G>\tambiguous\t<A>\tpasses\t<P>\n
 *     # taxon\tassigned\tunique\tclade_assigned\tclade_unique\n
 *     <s>\t...\n    for every label text with assigned > 0 and every ';'-prefix of one, in unsigned bytewise order (shorter first)
 * G is the profile's `classified` (every read with found > 0 has a candidate): the `assigned` column sums to it.
 * What this is not: a read whose best label is itself an interior taxon stays there (BUILD_GG relabels colliding k-mers to shorter labels,
 * itree.c:268-307); there is no genome-length or k-mer-distribution normalisation.  The per-read reassignment is a report of its own:
 * utree_redist_classify_batch_keys / utree_redist_assign / utree_redist_reads_format below (UTREE_REDISTRIBUTE_READS).
 *
 * A handle lives on ONE device for one database: a 64-bit counter per label for the single-candidate reads, an open-addressed table of the
 * multi-label sets with their read counts (16 B a slot) and an arena of eight labels per slot for the sets' members.
 * ---------------------------------------------------------------------------------------------- */
typedef struct utree_redist utree_redist;
#define UTREE_REDIST_DEFAULT_CAPACITY (1u << 22)
#define UTREE_REDIST_DEFAULT_PASSES 100
/* set_capacity: slots of the table of multi-label sets (rounded up to a power of two, at most 2^28) -- keep it at twice the distinct sets a
 * search can produce. */
int utree_redist_create(utree_dev *dev, uint32_t set_capacity, utree_redist **out);
/* Forgets every set (synchronous: waits for the device first). */
int utree_redist_reset(utree_redist *rd);
void utree_redist_free(utree_redist *rd);
/* utree_classify_batch (same arguments, `dev` = the image rd was created for; d_out bit for bit the same) that also adds the candidate sets
 * of the batch's reads to rd: ONE more kernel between the classify kernels and the vote, which reads the per-read label lists the vote
 * consumes.  Any number of streams may add to one handle at the same time. */
int utree_redist_classify_batch(utree_redist *rd, utree_dev *dev, const uint8_t *d_bases, const uint64_t *d_off, const uint32_t *d_len,
                                uint32_t n_reads, uint64_t total_bases, uint32_t max_len, int do_rc, utree_result *d_out, void *d_workspace,
                                size_t workspace_bytes, void *stream);
typedef struct { uint64_t reads, first; uint32_t n, pad; } utree_redist_set;
/* The read-back (synchronous): every distinct candidate set with its read count -- set i is the file-order label indices
 * h_labels[h_sets[i].first .. + h_sets[i].n), in no particular order, single-label sets included.  *n_sets / *n_labels = what there is;
 * UTREE_E_ARG when set_cap / label_cap are smaller (nothing is written then: call with 0, 0 to size the arrays).  *n_reads = reads added,
 * *n_classified = the sum of the sets' reads (either may be NULL).  UTREE_E_DEVICE when the table or the arena was too small for a batch:
 * the sets are then incomplete. */
int utree_redist_read(utree_redist *rd, utree_redist_set *h_sets, size_t set_cap, uint32_t *h_labels, size_t label_cap, size_t *n_sets,
                      size_t *n_labels, uint64_t *n_reads, uint64_t *n_classified);
/* dst += src: src's sets re-inserted into dst, its counters and reads added (synchronous; the handles may be on different devices, same
 * database). */
int utree_redist_merge(utree_redist *dst, utree_redist *src);
typedef struct { uint32_t label, pad; uint64_t assigned, unique; } utree_redist_entry;
/* The passes, on the device (synchronous; max_passes 1 .. 1000).  One entry per label with a non-zero figure, index order; *n = their number
 * (UTREE_E_ARG if that exceeds cap; cap = the database's labels always suffices); *passes = P, *ambiguous = A (either may be NULL).  The
 * handle keeps its sets: more batches may be added and solved again.  UTREE_E_DEVICE as for utree_redist_read. */
int utree_redist_solve(utree_redist *rd, uint32_t max_passes, utree_redist_entry *h, size_t cap, size_t *n, uint32_t *passes, uint64_t *ambiguous);
/* Host only: entries (label indices of ctr; several with one label are added up) -> merged by text, rolled up, written to `path`. */
int utree_redist_write(const utree_ctr *ctr, const utree_redist_entry *e, size_t n, uint64_t n_reads, uint64_t ambiguous, uint32_t passes,
                       const char *path);
/* ---- each read's redistributed label (xtree's --perq-out) ----
 * A KEY per read says where its candidates are: UTREE_REDIST_KEY_NONE -- no hit (found == 0), or the pass refused the read (it has then set
 * the handle's error word, as without keys); l < 0x80000000 -- the read's only candidate is the file-order label index l;
 * 0x80000000 | slot -- its candidates are the set in `slot` of the handle's table (at most 2^28 slots).  Every read of a batch gets exactly
 * one key.  Keys of a handle stay valid until utree_redist_reset: utree_redist_merge INTO a handle only adds slots and never moves one, so the
 * keys a handle gave before a merge are still right after it.  Nothing is normalised, and a read whose best label is an interior taxon stays
 * there, as above. */
#define UTREE_REDIST_KEY_NONE 0xFFFFFFFFu
/* utree_redist_classify_batch (same arguments, d_out bit for bit the same, the same sets added) that also writes d_key[0 .. n_reads).
 * UTREE_E_UNSUPPORTED for a database of 2^31 labels or more, UTREE_E_ARG for d_key == NULL with n_reads > 0. */
int utree_redist_classify_batch_keys(utree_redist *rd, utree_dev *dev, const uint8_t *d_bases, const uint64_t *d_off, const uint32_t *d_len,
                                     uint32_t n_reads, uint64_t total_bases, uint32_t max_len, int do_rc, utree_result *d_out, void *d_workspace,
                                     size_t workspace_bytes, uint32_t *d_key, void *stream);
/* The assignment of n keys.  d_key: keys of `keys`' table, on its device, as are d_label and d_ncand (may be NULL).  `solved`: `keys` itself, or
 * the handle `keys` was merged into, after utree_redist_solve -- a later add, insert, merge into or reset of `solved` ends that state.
 * d_label[r] = win(S_r, T_P), the label utree_redist_solve's `assigned` counts read r under, d_ncand[r] = |S_r| (1: the read never had another
 * candidate); KEY_NONE gives 0xFFFFFFFF and 0; a key that names no label of the database and no occupied slot of the table gives 0xFFFFFFFF and
 * 0xFFFFFFFF, and nothing is read for it.  UTREE_E_ARG when `solved` is not in the solved state, the handles are of different databases, or
 * d_key or d_label is NULL with n > 0.  With solved != keys the call first brings T_P over to `keys`' device; the winners of `keys`' slots are
 * computed once per solve, not per call.  Synchronous up to that point, asynchronous on `stream` afterwards. */
int utree_redist_assign(utree_redist *keys, utree_redist *solved, const uint32_t *d_key, uint64_t n, uint32_t *d_label, uint32_t *d_ncand,
                        void *stream);
/* Host only: one line "name\tlabel text\tncand\n" for every read with label != 0xFFFFFFFF, in order; name = names[name_off[i] .. + name_len[i]),
 * the label text whole (never a ';'-prefix; it may be empty).  Returns bytes written, or (size_t)-1 when cap is too small or a label is none of
 * ctr's -- as utree_hitmap_format. */
size_t utree_redist_reads_format(const utree_ctr *ctr, const uint8_t *names, const uint64_t *name_off, const uint32_t *name_len,
                                 const uint32_t *label, const uint32_t *ncand, size_t n, char *out, size_t cap);
/* utree_search_file_coverage with mates_path, interleaved, redistribute_path and max_passes set as well. */
int utree_search_file_redistribute(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path, const char *mates_path,
                                   int interleaved, const char *out_path, int do_rc, int host_threads, int input_format,
                                   const char *profile_path, const char *coverage_path, const char *redistribute_path, uint32_t max_passes,
                                   utree_search_stats *stats);

/* ------------------------------------------------------------------------------------------------
 * Per-query k-mer hit map: which label each window of a query hit, in window order (no counterpart in the reference's output: it builds
 * exactly this list per read -- AllTheKingsHorses[foundUniq-1] = ix, itree.c:935 -- and drops it after the vote).  GG search only: the
 * rank-specific search examines a hit-dependent subset of windows and has no map.
 *   Query.  q is the byte string the reference searches: the read as framed; with RC read + 'N' + revcomp(read) (itree.c:891-898); a pair is
 *     mate1 + 'N' + mate2 (utree_pairs_join) and with RC that joined string + 'N' + its reverse complement.  Positions are positions in q:
 *     with L the read's (joined pair's) length, window p = 2L+1-k-s of q is the reverse complement of the read's window s.
 *   Windows.  len(q) >= k: n_windows = len(q) - k + 1, else 0.  Window p has one code: UTREE_HIT_INVALID when some byte of q[p .. p+k) is not
 *     one of ACGTacgt (the k windows around a joining 'N' are of this kind); the file-order label index ix when XT_getIX32(word) returns
 *     ix < n_labels (a HIT, itree.c:929); UTREE_HIT_MISS otherwise.  A database of more than 0xFFFFFFFE labels: UTREE_E_UNSUPPORTED.
 *   Runs.  A query's map is the list of maximal stretches of equal code in window order, (code, count); the counts sum to n_windows, those of
 *     the hit runs to the read's `found` (column 3 of its output line), and the distinct hit codes number its `uix` (column 4).
 * ---------------------------------------------------------------------------------------------- */
#define UTREE_HIT_MISS    0xFFFFFFFFu
#define UTREE_HIT_INVALID 0xFFFFFFFEu
typedef struct { uint32_t code, count; } utree_hit_run;
/* error 0; 1: run_capacity too small (size d_runs for total_runs and call again); 2: total_bases is smaller than the reads' lengths add up to;
 * 3: a query of 2^32 windows or more (a run's count is 32 bits).  With 2 or 3 there is no map: total_runs = 0 and every offset is 0. */
typedef struct { uint64_t total_runs, total_windows; uint32_t error, pad; } utree_hitmap_meta;
/* bytes of d_workspace for a batch: 4 per window of q for the codes, 1/8 for the queries' starts, 32 per 64 windows and per read for the scans */
size_t utree_hitmap_workspace_bytes(const utree_dev *dev, uint32_t n_reads, uint64_t total_bases, int do_rc);
/* The maps of a batch, reads given as utree_classify_batch takes them (any lengths, empty reads and reads shorter than k included; pairs:
 * utree_pairs_join first).  Asynchronous on `stream`.  Read r's runs are d_runs[d_run_off[r] .. d_run_off[r + 1]); d_run_off (n_reads + 1
 * entries) and *d_meta are always complete; when total_runs > run_capacity, error is 1 and NO element of d_runs at or beyond run_capacity is
 * written (those below are the map's).  run_capacity = total_windows always suffices.  Every window is looked up once, in the device image;
 * the call keeps no state outside d_workspace, so any number of streams may run it on one handle at the same time. */
int utree_hitmap_batch(utree_dev *dev, const uint8_t *d_bases, const uint64_t *d_off, const uint32_t *d_len, uint32_t n_reads,
                       uint64_t total_bases, int do_rc, uint64_t *d_run_off /* n_reads + 1 */, utree_hit_run *d_runs,
                       uint64_t run_capacity, utree_hitmap_meta *d_meta, void *d_workspace, size_t workspace_bytes, void *stream);
/* Host only: one line for EVERY query, in input order (a query without an output line still has a map):
 *     name \t n_windows \t found \t tokens \n
 * tokens = the runs as code:count separated by one space (empty when n_windows == 0); a code prints as the decimal label index for a hit,
 * '-' for a miss, 'N' for an invalid window.  name = h_buf[name_off[i] .. + name_len[i]), what the output file prints for the query.
 * h_run_off: n + 1 entries into h_runs.  Returns bytes written, or (size_t)-1 if cap is too small. */
size_t utree_hitmap_format(const uint8_t *h_buf, const uint64_t *name_off, const uint32_t *name_len, const uint64_t *h_run_off,
                           const utree_hit_run *h_runs, size_t n, char *h_out, size_t cap);
/* utree_search_file_redistribute with hitmap_path set as well. */
int utree_search_file_hitmap(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path, const char *mates_path,
                             int interleaved, const char *out_path, int do_rc, int host_threads, int input_format,
                             const char *profile_path, const char *coverage_path, const char *redistribute_path, uint32_t max_passes,
                             const char *hitmap_path, utree_search_stats *stats);

/* ------------------------------------------------------------------------------------------------
 * Per-sample taxon table of multiplexed reads (no counterpart in itree.c, whose users parse the per-read lines in a script).  Pipelines hand
 * the search ONE combined reads file whose records are named <sample>_<n> (PlateA.well7_1532); what they take away is a taxon x sample matrix.
 *   Sample id.  Taken from the name the output line prints (a pair: mate 1's name; with an opt-in input format the name that format's framing
 *     yields): the bytes before the LAST occurrence of the delimiter byte (default '_').  A name without the delimiter is its own id; an id may
 *     be empty (the name "_7", an empty name).  Ids are compared as byte strings, never by hash alone.
 *   Figures.  For every (sample, taxon) the number of the sample's reads whose output line prints exactly that taxon -- the profile's `assigned`,
 *     keyed (label, cut) as the profile's entries and merged by printed text exactly as utree_profile_write merges; per sample all its reads and
 *     its reads without a line.
 *   File.  Every line ends in '\n', fields are separated by one TAB:
 *     # reads\t<N>\tclassified\t<G>\tunclassified\t<N-G>\tsamples\t<S>
 *     # taxon\t<id_1>\t...\t<id_S>
 *     # reads\t<n_1>\t...\t<n_S>
 *     # unclassified\t<u_1>\t...\t<u_S>
 *     <taxon>\t<c_1>\t...\t<c_S>          one line per taxon some sample assigned a read to
 *     Samples are in unsigned bytewise order of their raw ids, shorter first, and so are the taxa; the empty taxon is a line that begins with
 *     the TAB, as in the profile.  There are NO ';'-prefix rows: the matrix holds `assigned`, and a matrix of `assigned` sums to any rank by
 *     adding the rows below a prefix (the profile's `clade` column is that sum over all samples).  In a printed id a TAB, a CR and a backslash
 *     appear as \t, \r, \\; nothing else is escaped.  With S = 0 the three '#' lines after the first end right after their first field.
 *   A reader can check: column j sums to n_j - u_j; a row sums to that taxon's `assigned` in the profile of the same run; the n_j sum to N.
 * The ids are interned and the cells counted on ONE device while a chunk's text and records are there.
 * ---------------------------------------------------------------------------------------------- */
#define UTREE_SAMPLES_DEFAULT_CAPACITY (1u << 16)   /* distinct sample ids of a search's handles; UTREE_SAMPLE_CAPACITY overrides */
#define UTREE_SAMPLES_DEFAULT_CELLS    (1u << 22)   /* slots of their (sample, taxon) cell tables; UTREE_SAMPLE_CELLS overrides   */
typedef struct utree_samples utree_samples;
/* A table on dev's device for dev's labels.  sample_capacity: the most distinct ids (1 .. 2^19; the id table has twice the slots, 28 B of HBM
 * each, and the ids' bytes an arena of 256 B per sample, 1 MiB at least); cell_capacity: slots of the (sample, label, cut) cell table (rounded
 * up to a power of two, 16 B each) -- keep it at twice the distinct cells.  delim: the delimiter byte, not TAB, space, CR or LF (else
 * UTREE_E_ARG).  UTREE_E_UNSUPPORTED for a database of 2^28 labels or more. */
int utree_samples_create(utree_dev *dev, uint32_t sample_capacity, uint32_t cell_capacity, int delim, utree_samples **out);
/* Adds n_reads records and their names on `stream`, asynchronously: record r's name is d_text[d_name_off[r] .. + d_name_len[r]), offsets
 * relative to d_text, which holds text_bytes bytes (a name that leaves them is refused, not read).  Any number of streams may add to one handle
 * at the same time. */
int utree_samples_add(utree_samples *s, const uint8_t *d_text, uint64_t text_bytes, const uint32_t *d_name_off, const uint32_t *d_name_len,
                      const utree_result *d_res, uint32_t n_reads, void *stream);
/* Empties the table (synchronous: waits for the device first). */
int utree_samples_reset(utree_samples *s);
void utree_samples_free(utree_samples *s);
typedef struct { uint32_t sample, label; int32_t cut; uint32_t pad; uint64_t reads; } utree_samples_cell;   /* (label, cut) as utree_profile_entry */
/* Synchronous (waits for the device).  Sample i (numbered in the order the device first claimed the ids: another device numbers them otherwise)
 * has the id h_ids[h_id_off[i] .. h_id_off[i + 1]), h_reads[i] reads of which h_unclassified[i] print no line; the cells with reads > 0 go to
 * h_cells.  h_id_off has sample_cap + 1 entries, h_reads and h_unclassified sample_cap.  *n_samples, *n_id_bytes, *n_cells are always set when
 * the device's state is sound: UTREE_E_ARG when one exceeds its capacity (nothing else is written then: size the arrays and call again).
 * *n_reads (may be NULL) = records added.  UTREE_E_DEVICE when a batch found the id table, the arena or the cell table full, a record named a
 * label the database lacks, a name lay outside its text, a taxon was longer than 65532 bytes, or the counters do not add up: there is no table
 * then, and utree_last_hip_error names the cause and the knob. */
int utree_samples_read(utree_samples *s, uint8_t *h_ids, size_t id_cap, uint64_t *h_id_off, uint64_t *h_reads, uint64_t *h_unclassified,
                       size_t sample_cap, utree_samples_cell *h_cells, size_t cell_cap, size_t *n_samples, size_t *n_id_bytes, size_t *n_cells,
                       uint64_t *n_reads);
/* one handle's read-back, as utree_samples_read fills it */
typedef struct {
    const uint8_t *ids; const uint64_t *id_off; const uint64_t *reads, *unclassified; size_t n_samples;
    const utree_samples_cell *cells; size_t n_cells; uint64_t n_reads;
} utree_samples_table;
/* Host only: the read-backs of any number of handles (label indices of ctr) -> one file in the layout above.  Samples are merged by id text and
 * taxa by printed text, so several devices may number their samples independently.  UTREE_E_ARG when the figures contradict each other (a
 * sample's reads are not its unclassified reads plus its cells, the samples' reads not n_reads, a cell names no sample or label). */
int utree_samples_write(const utree_ctr *ctr, const utree_samples_table *tabs, size_t n_tabs, const char *path);
/* utree_search_file_hitmap with samples_path and sample_delim = delim set as well. */
int utree_search_file_samples(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path, const char *mates_path,
                              int interleaved, const char *out_path, int do_rc, int host_threads, int input_format,
                              const char *profile_path, const char *coverage_path, const char *redistribute_path, uint32_t max_passes,
                              const char *hitmap_path, const char *samples_path, int delim, utree_search_stats *stats);
/* utree_rank_search_file_profile with samples_path and sample_delim = delim set as well. */
int utree_rank_search_file_samples(const utree_ctr *ctr, utree_dev *dev, const char *reads_path, const char *out_path, int do_rc,
                                   const utree_rank_params *params, int host_threads, int input_format, const char *profile_path,
                                   const char *samples_path, int delim, utree_search_stats *stats);

/* ------------------------------------------------------------------------------------------------
 * Ambiguous reads redistributed PER SAMPLE of a multiplexed file (UTREE_SAMPLE_REDISTRIBUTE; GG search only).  The two reports above do
 * not compose: the sample table's cells are the vote's `assigned`, and the redistribution takes the whole file for one community, so a taxon
 * that is rich in sample A pulls sample B's ambiguous reads towards it.  This report is the taxon x sample matrix with every sample's
 * ambiguous reads redistributed within that sample.
 *   Sample id.  As the sample table defines it: the printed name before its LAST delimiter byte (default '_'); a name without the delimiter
 *     is its own id, an id may be empty, a pair takes mate 1's name.  Ids are compared as bytes, never by hash alone.
 *   Candidate sets.  As utree_redist_* defines them: { l : c[l] == max c } over file-order label indices, none for a read without a hit, no cap.
 *   Per sample s.  R_s = the sample's reads (a pair counts once), N_s = |R_s|.  The redistribution's definition applies with R_s in the place
 *     of "the reads searched": T0_s[l] = reads of R_s whose set contains l; win takes the largest T_s, on equal tallies the smallest
 *     file-order index; pass p runs while p <= max_passes and, after the first, while the previous changes_s > N_s / 100000 (integer
 *     division).  At least one pass runs; a sample that has stopped stays stopped while the others go on, P_s is its own pass count.
 *     assigned_s[l] is one more evaluation under T_{P_s}; unique_s[l] = reads whose set is exactly {l}; ambiguous_s = reads with more than one
 *     candidate.  max_passes (1 .. 1000, default UTREE_REDIST_DEFAULT_PASSES) is the same for every sample.
 *   File.  Fields are separated by one TAB, every line ends in '\n', samples and taxa in unsigned bytewise order (shorter first), ids escaped
 *     as the sample table escapes them:
 *     # reads\t<N>\tclassified\t<G>\tunclassified\t<N-G>\tambiguous\t<A>\tsamples\t<S>
 *     # taxon\t<id_1>\t...\t<id_S>
 *     # reads\t<n_1>...
 *     # unclassified\t<u_1>...
 *     # ambiguous\t<a_1>...
 *     # passes\t<P_1>...
 *     <taxon>\t<assigned_1>\t...\t<assigned_S>     one line per label text with assigned > 0 in some sample
 *     Labels of equal text are merged at write time; there are no ';'-prefix rows; with S = 0 the '#' lines after the first end after their
 *     first field.
 *   A reader can check: column j sums to n_j - u_j; the `# reads` and `# unclassified` rows are the sample table's rows for the same run; for
 *     a file that holds one sample the column is the `assigned` column (rows with assigned > 0) of the redistribution's file for the same run
 *     and `# passes` that file's `passes`.
 * What this is not: no per-read reassignment, no normalisation, no rank-specific search.
 *
 * A handle lives on ONE device for one database: an id table and arena as the sample table has them, a table of multi-label sets with its
 * arena as the redistribution has it, and an open-addressed table of {key, reads} cells, 16 B a slot; a cell is (sample, candidate set)
 * (DESIGN.md section 7).
 * ---------------------------------------------------------------------------------------------- */
typedef struct utree_sredist utree_sredist;
/* sample_capacity: the most distinct ids (1 .. 2^19); set_capacity: slots for distinct multi-label sets (rounded up to a power of two, at most
 * 2^28); cell_capacity: slots of the cell table (rounded up to a power of two, at most 2^30) -- keep both at twice what a search can produce.
 * delim as for utree_samples_create.  UTREE_E_ARG beyond those bounds, UTREE_E_UNSUPPORTED for a database of 2^28 labels or more. */
int utree_sredist_create(utree_dev *dev, uint32_t sample_capacity, uint32_t set_capacity, uint32_t cell_capacity, int delim, utree_sredist **out);
/* Forgets everything (synchronous: waits for the device first). */
int utree_sredist_reset(utree_sredist *h);
void utree_sredist_free(utree_sredist *h);
/* utree_classify_batch (same arguments, `dev` = the image h was created for; d_out bit for bit the same) that also counts the batch's reads
 * per (sample, candidate set): one more kernel between the classify kernels and the vote.  Read r's name is d_text[d_name_off[r] .. +
 * d_name_len[r]) of d_text's text_bytes bytes, as utree_samples_add takes it.  Any number of streams may add to one handle at the same time. */
int utree_sredist_classify_batch(utree_sredist *h, utree_dev *dev, const uint8_t *d_bases, const uint64_t *d_off, const uint32_t *d_len,
                                 uint32_t n_reads, uint64_t total_bases, uint32_t max_len, int do_rc, const uint8_t *d_text, uint64_t text_bytes,
                                 const uint32_t *d_name_off, const uint32_t *d_name_len, utree_result *d_out, void *d_workspace,
                                 size_t workspace_bytes, void *stream);
/* `reads` reads of sample `sample` whose candidate set is the file-order label indices labels[first .. first + n), n >= 1 */
typedef struct { uint32_t sample, n; uint64_t first, reads; } utree_sredist_cell;
/* The read-back (synchronous).  Samples as utree_samples_read returns them (ids, h_id_off with sample_cap + 1 entries, reads, unclassified; numbered
 * in the order the device first claimed the ids); the cells with reads > 0 into h_cells, their labels into h_labels, single-label sets included.
 * *n_samples, *n_id_bytes, *n_cells, *n_labels are always set when the device's state is sound: UTREE_E_ARG when one exceeds its capacity
 * (nothing else is written then: call with zero capacities to size the arrays).  *n_reads (may be NULL) = records added.  UTREE_E_DEVICE when
 * a batch found the id table or its arena, the set table or its arena or the cell table full, a record named a label the database lacks, a name
 * lay outside its text, or the counters do not add up: utree_last_hip_error names the cause and the knob. */
int utree_sredist_read(utree_sredist *h, uint8_t *h_ids, size_t id_cap, uint64_t *h_id_off, uint64_t *h_reads, uint64_t *h_unclassified,
                       size_t sample_cap, utree_sredist_cell *h_cells, size_t cell_cap, uint32_t *h_labels, size_t label_cap, size_t *n_samples,
                       size_t *n_id_bytes, size_t *n_cells, size_t *n_labels, uint64_t *n_reads);
/* The same flat form given on the host and inserted (synchronous): n_samples ids with their reads and unclassified reads, n_cells cells of
 * those samples, n_reads records.  A sample's reads must be its unclassified reads plus its cells' for the handle to read back. */
int utree_sredist_insert(utree_sredist *h, const uint8_t *ids, const uint64_t *id_off, const uint64_t *reads, const uint64_t *unclassified,
                         size_t n_samples, const utree_sredist_cell *cells, size_t n_cells, const uint32_t *labels, size_t n_labels,
                         uint64_t n_reads);
/* dst += src: a read of src followed by an insert into dst (the handles may be on different devices, same database). */
int utree_sredist_merge(utree_sredist *dst, utree_sredist *src);
typedef struct { uint32_t sample, label; uint64_t assigned, unique; } utree_sredist_entry;
/* The passes of every sample, on the device (synchronous; max_passes 1 .. 1000): tallies only for the (sample, label) pairs that occur, the
 * host reads one word per still-active sample per pass.  One entry per (sample, label) with a non-zero figure, by sample (utree_sredist_read's
 * numbering), then label; *n = their number (UTREE_E_ARG if that exceeds cap; the read-back's *n_labels always suffices).  h_passes[s] = P_s and
 * h_ambiguous[s] for the *n_samples samples (UTREE_E_ARG if sample_cap is smaller; either array may be NULL).  The handle keeps its state. */
int utree_sredist_solve(utree_sredist *h, uint32_t max_passes, utree_sredist_entry *e, size_t cap, size_t *n, uint32_t *h_passes,
                        uint64_t *h_ambiguous, size_t sample_cap, size_t *n_samples);
/* Host only (runs without a GPU): the samples of a read-back, the figures of a solve (label indices of ctr) -> the file above.  UTREE_E_ARG when
 * the figures contradict each other (a sample's assigned reads are not its reads minus its unclassified reads, the samples' reads not n_reads,
 * more ambiguous than classified reads, an entry names no sample or label, two samples with one id, passes outside 1 .. 1000). */
int utree_sredist_write(const utree_ctr *ctr, const uint8_t *ids, const uint64_t *id_off, const uint64_t *reads, const uint64_t *unclassified,
                        const uint32_t *passes, const uint64_t *ambiguous, size_t n_samples, const utree_sredist_entry *e, size_t n_entries,
                        uint64_t n_reads, const char *path);
/* utree_search_file_samples with sample_redistribute_path set as well: every field of the GG search's request. */
int utree_search_file_sample_redistribute(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path, const char *mates_path,
                                          int interleaved, const char *out_path, int do_rc, int host_threads, int input_format,
                                          const char *profile_path, const char *coverage_path, const char *redistribute_path, uint32_t max_passes,
                                          const char *hitmap_path, const char *samples_path, int delim, const char *sample_redistribute_path,
                                          utree_search_stats *stats);

/* ------------------------------------------------------------------------------------------------
 * One whole-file search, described by one request.  Every utree_search_file* / utree_search_pairs_file / utree_rank_search_file* entry point
 * above is a fixed-argument form of this call: it fills the fields its comment names, leaves the rest 0 / NULL and calls utree_search_run.
 * A report's path that is NULL means: no such report -- nothing of it is allocated, uploaded or launched, and the per-read output, stdout, the
 * stats and the other reports are those of a search without it.  A search that fails returns its own code and leaves every report path as it
 * was; the reports are written when the search has succeeded, in the order coverage, redistribution, redistributed reads, sample table, per-sample
 * redistribution, profile, and only when the devices counted every read exactly once.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    uint32_t size;                    /* = sizeof(utree_search_request), or the size of the layout without redistribute_reads_path (a caller built
                                         before that field: a request without that report); anything else is UTREE_E_ARG                      */
    int do_rc, host_threads;          /* RC; the host formatting team (<= 0: as many as OpenMP gives, at most 16)                              */
    int input_format;                 /* UTREE_INPUT_*; AUTO looks at the first byte; a non-reference format also reads gzip through zlib       */
    const char *reads_path;           /* the reads; with mates_path the first mates; with interleaved records 2i and 2i+1 are pair i           */
    const char *mates_path;           /* NULL, or the file of second mates (not with interleaved).  Pairs take the host framing pipeline
                                         (stats.pipeline == 0) and every report sees the joined queries (no window crosses the 'N')           */
    int interleaved;
    const char *out_path;
    const utree_rank_params *rank;    /* non-NULL: the rank-specific search on ONE device handle (n_dev must be 1), whose carried array is reset
                                         first (utree_rank_reset).  It reads no pairs and writes a profile and a sample table only: any of
                                         coverage_path, redistribute_path, hitmap_path, sample_redistribute_path, redistribute_reads_path is
                                         UTREE_E_ARG                                                                                          */
    const char *profile_path;         /* per-taxon read counts, each device handle counting its own reads (UTREE_PROFILE_CAPACITY truncated-taxon
                                         slots, default 2^20).  Not written: UTREE_E_PROFILE, utree_last_hip_error says why                   */
    const char *coverage_path;        /* distinct database k-mers covered per taxon; one handle per device handle, merged before the file is
                                         written.  Not written: UTREE_E_COVERAGE (a profile that failed too keeps UTREE_E_PROFILE)            */
    const char *redistribute_path;    /* ambiguous reads redistributed among tied labels; one handle per device handle (UTREE_REDIST_CAPACITY
                                         slots, default 2^22), merged into the first and solved.  Not written -- the file, a table too small,
                                         reads not added once --: UTREE_E_PROFILE (no code of its own), utree_last_hip_error names the file and
                                         the cause.  (A search into a pipe that the host pipeline has to take over half-way cannot take back the
                                         sets of the chunks it drops: it ends with this error rather than a wrong table.)                      */
    uint32_t max_passes;              /* of the redistributions (0: the default; more than 1000 with any of their paths: UTREE_E_ARG)         */
    const char *hitmap_path;          /* every query's hit map, and the label texts to <hitmap_path>.labels, line i (0-based) = label index i.
                                         Written in step with the output: the writer stage commits a chunk's output lines and its map lines
                                         together, so after a framing error or UTREE_E_PAIRS both files hold the same queries.  Always the host
                                         framing pipeline.  Not written: UTREE_E_HITMAP (a report that failed too keeps its own code)         */
    const char *samples_path;         /* taxon x sample table, ids cut at sample_delim.  The pipeline stays what it would be (a search the device
                                         text pipeline takes stays there).  Not written -- the file, a capacity (UTREE_SAMPLE_CAPACITY, default
                                         2^16 ids; UTREE_SAMPLE_CELLS, default 2^22 cells) --: UTREE_E_PROFILE, as for redistribute_path      */
    const char *sample_redistribute_path;  /* that table with every sample's ambiguous reads redistributed within the sample; one handle per
                                         device handle (UTREE_SAMPLE_CAPACITY ids, UTREE_REDIST_CAPACITY sets, UTREE_SAMPLE_CELLS cells).  Not
                                         written: UTREE_E_PROFILE (the profile's failure wins, then the redistribution's, the sample table's,
                                         this report's)                                                                                       */
    int sample_delim;                 /* one byte, 0: '_'; with either sample report not TAB, space, CR or LF (UTREE_E_ARG)                    */
    const char *redistribute_reads_path;   /* each classified query's redistributed label: one line "name \t label text \t n_candidates" per line
                                         of the output, in its order (pairs: under mate 1's name), no header.  With or without
                                         redistribute_path (ONE solve serves both files; max_passes, UTREE_REDIST_CAPACITY apply).  Always the
                                         host framing pipeline; the keys are spooled to <path>.spool while searching (removed on every way out)
                                         and assigned after the solve.  Not written: UTREE_E_PROFILE, ranking with redistribute_path           */
} utree_search_request;
/* The one call that checks a request and runs it: GG search over devs[0 .. n_dev), or the rank-specific one.  Every argument is checked before
 * `ctr` or a device handle is looked at: UTREE_E_ARG for a wrong size, a NULL ctr, devs, reads_path or out_path, n_dev < 1, an input_format
 * that is none, mates_path together with interleaved, and what the fields above say. */
int utree_search_run(const utree_ctr *ctr, utree_dev **devs, int n_dev, const utree_search_request *req, utree_search_stats *stats);

/* ------------------------------------------------------------------------------------------------
 * `.ubt` -> `.ctr` = XT_cmp32(filename, outfile) (itree.c:1234-1315; `xtree-compress`), SURVEY.md §8(f) rank 2.
 * Node dump streamed through `device`; output byte-identical to the reference's, first-bin quirk included.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    uint64_t n_nodes, n_labels;
    uint64_t label_count_total;   /* "Total nodes in tree: %llu" (itree.c:1314): sum of the label counts */
    uint32_t W, I;
    double   seconds;
} utree_compress_stats;

int utree_compress_file(const char *ubt_path, const char *ctr_path, int device, utree_compress_stats *stats);

/* ------------------------------------------------------------------------------------------------
 * Database BUILD = the `utree-build` / `utree-buildGG` binaries (itree.c -D BUILD / BUILD_GG, main 1379-1407:
 * UT_parseSampFastaExternOSFA + UT_writeTreeBinary + UT_writeSamples).  SURVEY.md §8(f) rank 3.
 * FASTA (one header line + one sequence line per reference) + `name \t label` map -> `<ubt_path>` and
 * `<ubt_path>.gg.log` (gg) / `<ubt_path>.log`, byte-identical to the reference's.  PACKSIZE (4*W), IXTYPE (I bytes) and
 * the compression level (itree.c:595-606) are run-time arguments; `gg` selects BUILD_GG's relabelling of colliding
 * k-mers (itree.c:268-307) instead of BUILD's "collision = BAD" (242-266).  k-mers are extracted, sorted and folded
 * on `device`; everything has to fit its HBM at once (about 36 B per k-mer occurrence plus the FASTA itself).
 * ---------------------------------------------------------------------------------------------- */
enum {
    UTREE_BUILD_E_MAP_EMPTY = 1,  /* "Input map empty." (itree.c:512)                         -> reference exit 1 */
    UTREE_BUILD_E_MAP = 2,        /* malformed map line `error_line` (533-553)                -> exit 2           */
    UTREE_BUILD_E_FASTA = 3,      /* header without sequence, reference `error_line` (585)    -> exit 2           */
    UTREE_BUILD_E_NO_KMERS = 4,   /* "Error: no k-mers. Bad input/params!" (631)              -> exit 2           */
    UTREE_BUILD_E_NAME = 5        /* "Error: taxon map incomplete (line %u)" (582)            -> exit 4           */
};
/* which check of the map parser failed (utree_build_stats.map_error when error_kind == UTREE_BUILD_E_MAP); the command
 * line prints the reference's text for each */
enum {
    UTREE_MAP_E_BLANK_NAME = 1,   /* "ERROR: map line %llu\nBlank indices are NOT ALLOWED." (itree.c:530-533)               */
    UTREE_MAP_E_EXTRA_TAB = 2,    /* "map: extra tab, line %llu" (537)                                                      */
    UTREE_MAP_E_NO_TAB = 3,       /* "Err tab1: %llu" (538)                                                                 */
    UTREE_MAP_E_BLANK_LABEL = 4,  /* "\nERROR: map line %llu\nBlank labels are NOT ALLOWED." (541-544)                      */
    UTREE_MAP_E_NO_NEWLINE = 5    /* "Err line counter: %llu" (548): the text ends inside a label                           */
};
typedef struct {
    uint64_t n_seqs;        /* references parsed (return value of UT_parseSampFastaExternOSFA)                    */
    uint64_t n_kmers;       /* k-mers added, repeats included                                                     */
    uint64_t n_nodes;       /* "Total nodes in tree: %llu" (itree.c:1337)                                         */
    uint64_t n_labels;      /* "[%llu labels]"                                                                    */
    uint64_t error_line;
    int      error_kind;    /* UTREE_BUILD_E_* when the call returns UTREE_E_BUILD (or UTREE_E_IO for MAP_EMPTY)  */
    uint32_t W, I;
    double   seconds;
    uint64_t n_distinct;    /* distinct k-mers, BAD ones included: "Done with sequence parse: %llu k-mers made" (626-630) */
    uint64_t map_bytes, map_lines;   /* "Parsed map. %llu bytes, %llu lines." (510, 515)                                  */
    int      map_error;     /* UTREE_MAP_E_* when error_kind == UTREE_BUILD_E_MAP                                         */
} utree_build_stats;

int utree_build_file(const char *fasta_path, const char *map_path, const char *ubt_path, uint32_t W, uint32_t I,
                     int complevel, int gg, int device, utree_build_stats *stats);

/* ------------------------------------------------------------------------------------------------
 * Database MERGE (`utree-merge` / `utree-mergeGG`; the reference has no such tool, but it defines what one must be).
 *
 * A database is what the builder's insert loop (xeTreeU / xeTreeU_RF, itree.c:242-307) holds after being fed (k-mer, label)
 * pairs in some order.  utree_merge_files(in_paths[0 .. n_in), ...) writes the `.ubt` that UT_writeTreeBinary
 * (itree.c:1317-1343) would write for the tree of an IMAGINED BUILD (BUILD_GG for gg = 1, BUILD for gg = 0) that is fed, at
 * compression level 0, one FASTA record of exactly k bases per input node (with lv = 0 a k-base line makes one iteration of
 * the position loop and yields one word, itree.c:584-624): input by input in argument order, within an input in file order,
 * each record mapped to the text of the label its node carries.  So:
 *   - Nodes.  The output holds the distinct words of all inputs, ascending.  A word that occurs in several inputs gets the
 *     fold of its labels in input order; an equal label text changes nothing.  gg: the folded label is the earlier label cut
 *     before the last ';' the two texts share in their common byte prefix, or BAD when they share fewer than two
 *     (critical_cutoff, itree.c:74, 285-304); !gg: any difference is BAD (260-264).  BAD is absorbing within one call and is
 *     not written.  The reference's rule has consequences that are part of the contract: "k;p;c" against "k;p;c;o" gives
 *     "k;p"; a third sibling species of one genus lifts the k-mer from genus to family; the result depends on the input order.
 *   - Labels.  A label gets its index when the first node carrying it is inserted, a prefix label when the collision that
 *     creates it happens; a text already present keeps its index (addSampleU, itree.c:593 and 299).  A label line of an input
 *     that none of its nodes carries is not carried over.  The label tail is `text \t nodes carrying it \n` in index order,
 *     header word 3 the sum of those counts.  No `.log` / `.gg.log` is written.
 *   - What it is NOT.  (1) A k-mer that an input's own build dropped as BAD has left no trace in that input and can come back
 *     under another input's label: only a rebuild from FASTA is BAD-exact.  (2) Nothing is known about the compression level:
 *     inputs built at different levels merge, and the result's sensitivity is that of the sparser one.
 *
 * Inputs are `.ubt` or `.ctr` files, told apart by structure: exactly one layout must have a tail that starts inside the file,
 * consists of complete `text \t decimal \n` lines and counts N nodes (else UTREE_E_FORMAT).  Label lines that repeat a text are
 * read as the loader reads them (the first line's index).  A `.ctr`'s words are rebuilt from bin membership + suffix; a bin
 * table that is not non-decreasing, or rebuilt words that are not strictly ascending (xtree-compress's first-bin quirk when the
 * first prefix holds a single node), are UTREE_E_UNSUPPORTED.  A `.ubt` whose words are not strictly ascending, or a node whose
 * index names no label line, is UTREE_E_FORMAT.  Inputs of different I merge; inputs of different W, W outside {4, 8, 16}, more
 * than 65534 labels with a 2-byte index, and 2^24 labels-and-prefixes are UTREE_E_UNSUPPORTED.  I = 0: the widest index among
 * the inputs; else 2 or 4.  UTREE_E_ARG (NULL path, n_in < 1, another I) is returned before a file is opened or the device is
 * touched.  utree_last_hip_error has the detail of every failure; a failed call leaves no output file behind.
 * The nodes go through `device` in passes over contiguous word ranges sized from its free memory (n_passes).
 * utree_merge_probe (host only) reports how one input reads.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    uint64_t n_in_nodes;     /* nodes read, all inputs                                   */
    uint64_t n_nodes;        /* nodes written                                            */
    uint64_t n_shared;       /* distinct words that occur in more than one input         */
    uint64_t n_relabelled;   /* ... written under a label none of their inputs gave them */
    uint64_t n_dropped;      /* ... BAD, not written                                     */
    uint64_t n_labels;       /* label lines written                                      */
    uint32_t W, I, n_inputs, n_passes;
    double   seconds;
} utree_merge_stats;

int utree_merge_files(const char *const *in_paths, int n_in, const char *ubt_path, uint32_t I, int gg, int device,
                      utree_merge_stats *stats);

typedef struct {
    uint32_t W, I;
    uint32_t is_ctr;         /* 0: `.ubt` layout, 1: `.ctr` layout                       */
    uint32_t pad;
    uint64_t n_nodes;
    uint64_t n_labels;       /* distinct label texts                                     */
} utree_merge_input;

int utree_merge_probe(const char *path, utree_merge_input *info);

/* ------------------------------------------------------------------------------------------------
 * EDITING while merging: cut labels to a rank, drop clades, keep only some clades, rename clades, subtract another database's
 * k-mers.  utree_merge_files_edit(in_paths, n_in, ubt_path, I, gg, device, edit, stats, edit_stats) writes the `.ubt` of the
 * merge's imagined build above, fed the nodes of the regular inputs in argument order and file order, EXCEPT
 *   (a) nodes whose label the edit drops,
 *   (b) nodes whose word occurs in any MINUS input (edit->minus_paths) -- for every input, regardless of argument order; a MINUS
 *       input contributes no record and no label, and the label edit does not apply to it,
 * and (c) with every remaining record mapped to the EDITED text of its label.  Everything else is utree_merge_files unchanged:
 * the fold (itree.c:242-307), the creation-order numbering (itree.c:593, 299), "a label line no node carries is not carried
 * over", the 2-byte limit of 65534 labels (applied to the labels AFTER the edit), the refusals of inputs (they hold for MINUS
 * inputs too: same W, `.ubt` or `.ctr`, words strictly ascending; a MINUS input's label indices are not looked at), and "a
 * failed call leaves no output file".  utree_merge_files(...) is utree_merge_files_edit(..., NULL, stats, NULL).
 *
 * The label edit of one label text t, in this order:
 *   1. clade match: a rule taxon p matches t iff t == p or t begins with p followed by ';' ("k__A;p__B" does not match
 *      "k__A;p__Bx");
 *   2. selection, on the original text: t is dropped when a keep file is given and no keep line matches it, or when some drop
 *      line matches it (drop beats keep);
 *   3. rename: among the rename lines `old \t new` whose old matches t, the one with the longest old is applied, once, with no
 *      chaining: t' = new + t[len(old):];
 *   4. ranks: with ranks = n, a t' that holds at least n ';' is cut before its n-th ';' (its first n tokens stay), else it is
 *      unchanged;
 *   5. empty result: an edited text that is empty is UTREE_E_FORMAT (the builder refuses blank labels); utree_last_hip_error
 *      names the label.
 * Rule files: lines end at '\n' (the last may lack it), one trailing '\r' is removed, empty lines are ignored, there is no
 * comment syntax, spaces and bytes above 0x7F are ordinary.  Drop and keep files: the whole line is the taxon, a TAB in it is
 * UTREE_E_FORMAT.  Rename file: exactly one TAB with both sides non-empty, else UTREE_E_FORMAT; two lines with the same old are
 * UTREE_E_FORMAT.  The error text names the file and the 1-based line.  A file that cannot be opened is UTREE_E_IO.  A rule
 * that matches no label line of any regular input is no error: it is counted (n_rules_unmatched), and the preview lists it.
 * UTREE_E_ARG (edit->size, ranks > 255, n_minus < 0, n_minus > 0 with a NULL array or entry, and utree_merge_files' own) comes
 * before any file is touched.
 *
 * With an edit utree_merge_stats reads: n_in_nodes the nodes read from the regular inputs; n_shared (two or more records fed),
 * n_relabelled, n_dropped (BAD) and n_nodes those of the records actually fed.  n_in_nodes == records fed + n_nodes_dropped +
 * n_nodes_subtracted; a node that is both label-dropped and in a MINUS input counts as dropped.
 *
 * LIMITS.  (1) Dropping a clade removes the k-mers still labelled inside it: k-mers that an earlier fold lifted to an ancestor
 * and k-mers an earlier build dropped as BAD do not change back -- only a rebuild is exact.  (2) A rename does not re-fold
 * earlier folds: texts that become equal merge into one label line, nothing else moves.  (3) MINUS is by identical word, as
 * stored: the database holds k-mers in the references' orientation and the search covers the other strand by appending the
 * reverse complement, so a contaminant on the opposite strand is removed only if the MINUS database was built from both
 * strands.  (4) A MINUS database built above compression level 0 holds only a sample of its k-mers (itree.c:603-616: the
 * sampling looks at the bases in front of the k-mer).  Build a MINUS database at level 0 from the host FASTA plus its reverse
 * complement.
 *
 * utree_merge_edit_preview (host only, never touches a device; minus_paths is ignored) writes to tsv_path, per regular input,
 * `# input \t path \t .ubt|.ctr \t nodes \t labels` followed, per distinct label text of that input in line order, by
 * `text \t nodes its first line states \t keep|rename|cut|rename+cut|drop \t edited text (empty for drop)`, and at the end one
 * `# unmatched \t rule file \t line \t rule taxon` per unmatched rule (drop file, keep file, rename file; line order).  Its
 * n_nodes_dropped is the sum of the stated counts of the dropped texts; n_minus_nodes and n_nodes_subtracted are 0.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    uint32_t size;                 /* sizeof(utree_merge_edit), else UTREE_E_ARG */
    uint32_t ranks;                /* 0: none; 1..255: cut each label before its ranks-th ';'; > 255: UTREE_E_ARG */
    const char *drop_path, *keep_path, *rename_path;      /* NULL: none */
    const char *const *minus_paths; int n_minus;          /* n_minus < 0, or > 0 with a NULL array or a NULL entry: UTREE_E_ARG */
} utree_merge_edit;

typedef struct {
    uint64_t n_label_lines;      /* distinct label texts looked at, summed over the regular inputs */
    uint64_t n_labels_dropped, n_labels_renamed, n_labels_cut;   /* of those; a text both renamed and cut counts in both */
    uint64_t n_rules_unmatched;
    uint64_t n_nodes_dropped;    /* regular-input nodes not fed because their label was dropped */
    uint64_t n_minus_nodes;      /* nodes read from the MINUS inputs */
    uint64_t n_nodes_subtracted; /* regular-input nodes the label edit kept, not fed because their word is in a MINUS input */
} utree_merge_edit_stats;

int utree_merge_files_edit(const char *const *in_paths, int n_in, const char *ubt_path, uint32_t I, int gg, int device,
                           const utree_merge_edit *edit, utree_merge_stats *stats, utree_merge_edit_stats *edit_stats);
int utree_merge_edit_preview(const char *const *in_paths, int n_in, const utree_merge_edit *edit, const char *tsv_path,
                             utree_merge_edit_stats *st);

/* ------------------------------------------------------------------------------------------------
 * Database COMPARE (`utree-compare`): what a merge, an edit, a compression or a rebuild did to the k-mers, taxon by taxon.
 *
 * utree_compare_files(a_path, b_path, report_path, moves_path, device, stats) compares database A ("old") with database B
 * ("new") and changes neither.  The inputs are `.ubt` or `.ctr` files in any mix, read exactly as utree_merge_files reads its
 * inputs -- the same layouts told apart by structure, label lines that repeat a text read as the loader reads them, and the
 * same refusals with the same codes (different W or W outside {4, 8, 16}: UTREE_E_UNSUPPORTED; words not strictly ascending or an
 * index without a label line: UTREE_E_FORMAT; a bin table that is not non-decreasing or the first-bin quirk:
 * UTREE_E_UNSUPPORTED).  I may differ between A and B.
 *
 * A word's LABEL is the TEXT of the label its node carries.  Index numbering, index width, file layout, the counts stated in
 * the tail and label lines no node carries are not compared.  Every word of A or B falls into exactly one class:
 *     same      in both, equal label text            only_a    in A only
 *     changed   in both, different label text        only_b    in B only
 * Per label text t there are seven figures: a (words of A labelled t), b (words of B labelled t), same, only_a, only_b, left
 * (labelled t in A and something else in B) and arrived (labelled t in B and something else in A).  For every t
 *     a = same + only_a + left,     b = same + only_b + arrived,     and over all t     sum(left) = sum(arrived) = changed.
 * A MOVE is a pair (label in A, label in B) of a changed word, with the number of words that made it; per `from` text the moves
 * sum to its left, per `to` text to its arrived, and all of them to changed.  Its kind is `lifted` when from begins with to
 * followed by ';' (a fold moved the k-mer to an ancestor), `lowered` for the reverse, `moved` otherwise.
 * IDENTICAL means changed == only_a == only_b == 0.
 *
 * report_path (all fields TAB-separated, lines end in '\n'):
 *     # a <path> .ubt|.ctr <W> <I> <nodes> <labels>                  labels: distinct label texts its nodes carry
 *     # b <path> .ubt|.ctr <W> <I> <nodes> <labels>
 *     # words <union> both <n> same <n> changed <n> only_a <n> only_b <n>
 *     # taxon a b same only_a only_b left arrived clade_a clade_b
 *     <taxon> <a> <b> <same> <only_a> <only_b> <left> <arrived> <clade_a> <clade_b>
 * with one row per label text with a + b > 0 and one per ';'-prefix of such a text, in unsigned bytewise order (the shorter
 * first on a tie).  A row for a pure prefix has zero own figures; clade_a / clade_b sum a / b over every text that equals the
 * row's taxon or begins with it followed by ';' (the profile's clade rule, the merge edit's clade match).
 * moves_path (NULL: not written): the line `# from \t to \t kmers \t kind`, then one line per distinct move, ordered bytewise
 * by from, then by to.
 *
 * What it is NOT.  (1) Words are compared as stored: a database built from the other strand shares nothing with this one.
 * (2) Two databases built at different compression levels hold different samples of their k-mers and differ in most words.
 * (3) A k-mer that B's build dropped as BAD has left no trace in B: it shows as only_a, indistinguishable from one that was
 * subtracted.
 *
 * UTREE_E_ARG (a NULL a_path, b_path, report_path or stats) is returned before a file is opened or the device is touched.  A
 * failed call leaves neither output file behind; utree_last_hip_error has the detail.  The nodes go through `device` in the
 * merge's passes (n_passes): contiguous ranges of the words' top 24 bits, sized from its free memory.
 *
 * utree_compare_write (host only) is the writer of both files.  It takes the inputs' descriptions, n label texts with their five
 * counted figures (a and b follow from the invariants; entries of equal text are added up; an entry without a word makes no
 * row) and n_moves moves between entries (moves of equal text pairs are added up).  UTREE_E_ARG, and no file: a NULL
 * argument other than moves_path and stats, a move that names no entry or whose texts are equal, or moves that do not sum to
 * their entries' left and arrived.  stats (or NULL) gets everything but n_passes and seconds.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    uint64_t a, b;               /* nodes of A, nodes of B                                                   */
    uint64_t same, only_a, only_b, left, arrived;   /* summed over all label texts; left == arrived == changed */
    uint64_t words, both;        /* distinct words of A and B together; words in both = same + changed       */
    uint64_t a_labels, b_labels; /* distinct label texts that nodes of A / of B carry                         */
    uint64_t n_moves;            /* distinct (label in A, label in B) pairs among the changed words           */
    uint32_t W, n_passes;
    uint32_t identical;          /* 1: changed == only_a == only_b == 0                                       */
    uint32_t pad;
    double   seconds;
} utree_compare_stats;           /* 120 bytes */

int utree_compare_files(const char *a_path, const char *b_path, const char *report_path, const char *moves_path, int device,
                        utree_compare_stats *stats);

typedef struct {
    const char *path;            /* as the report's `# a` / `# b` line names it */
    uint32_t is_ctr, W, I, pad;
} utree_compare_input;

typedef struct {
    const char *text; uint32_t len, pad;
    uint64_t same, only_a, only_b, left, arrived;
} utree_compare_entry;

typedef struct {
    uint32_t from, to;           /* indices into the entries */
    uint64_t kmers;
} utree_compare_move;

int utree_compare_write(const utree_compare_input *a, const utree_compare_input *b, const utree_compare_entry *e, size_t n,
                        const utree_compare_move *m, size_t n_moves, const char *report_path, const char *moves_path,
                        utree_compare_stats *stats);

/* ------------------------------------------------------------------------------------------------
 * Database INSPECTION (`utree-inspect`): how safe the k-mers of ONE database are against a single substitution.
 *
 * The search matches k-mers exactly.  A sequencing error or a SNP turns a read's k-mer w into a word one substitution away; if the
 * database holds that word under a label on the same lineage the vote loses nothing, if it holds it under another taxon the read
 * casts a wrong vote.  utree_inspect_file(db_path, report_path, pairs_path, device, stats) counts, from the file alone, which
 * nodes have such neighbours and between which label texts, and changes nothing.
 *
 * INPUT.  The database is the set of its nodes (word, label TEXT), read exactly as utree_merge_files and utree_compare_files
 * read an input: `.ubt` or `.ctr` told apart by structure, W in {4, 8, 16} (k = 16, 32, 64), 2- or 4-byte indices, label lines
 * that repeat a text read as the loader reads them, and the same refusals with the same codes.  Index numbering, index width and
 * label lines no node carries do not matter.
 *
 * NEIGHBOURS.  A neighbour of word w is w ^ (d << 2p) for d in {1, 2, 3} and base position p in [0, k): 3k words (W = 4: only
 * the low 32 bits carry the 16-mer, so 48, not 96).  A neighbour is HELD when some node of the database has that word.
 * ANCESTORS.  Text x is an ancestor of y when y begins with x followed by ';' (the merge edit's clade match; taken literally for
 * the empty text too).  Two texts are ON ONE LINEAGE when they are equal or one is an ancestor of the other.
 * CLASSES.  Every node falls in exactly one class, the worst any held neighbour puts it in:
 *     conflict   some held neighbour's text is off the node's lineage
 *     lineage    otherwise, some held neighbour's text differs from the node's
 *     same       otherwise, at least one neighbour is held
 *     isolated   no neighbour is held
 * (xtree's build log calls isolated + same the adamantine k-mers and conflict the weak ones.)
 * A PAIR EVENT is an ordered (node, held neighbour node) of different label texts; each is found from both ends, so
 * pairs(t, t') = pairs(t', t).  Its kind, seen from the node's text `from` towards the neighbour's text `to`: `ancestor` when to
 * is an ancestor of from, `descendant` for the reverse, `conflict` otherwise.
 *
 * report_path (all fields TAB-separated, lines end in '\n'):
 *     # db <path> .ubt|.ctr <W> <I> <nodes> <labels>                 labels: distinct label texts its nodes carry
 *     # kmers <N> isolated <n> same <n> lineage <n> conflict <n> pair_events <n> distinct_pairs <n>
 *     # taxon kmers isolated same lineage conflict clade_kmers clade_conflict
 *     <taxon> <kmers> <isolated> <same> <lineage> <conflict> <clade_kmers> <clade_conflict>
 * with one row per label text a node carries and one per ';'-prefix of such a text, in unsigned bytewise order (the shorter
 * first on a tie); the clade columns sum kmers / conflict over every text that equals the row's taxon or begins with it followed
 * by ';' (the profile's clade rule).  For every row kmers = isolated + same + lineage + conflict; each of the four class columns
 * sums over all rows to its total on the `# kmers` line, and the kmers column sums to N.
 * pairs_path (NULL: not written): the line `# from \t to \t pairs \t kind`, then one line per distinct ordered pair of different
 * texts with at least one pair event, ordered bytewise by from, then by to.  The pairs column sums to pair_events and the file is
 * symmetric: (a, b, n) stands with (b, a, n), and `ancestor` is mirrored by `descendant`.
 *
 * LIMITS.  (1) Only substitutions are considered, no insertions or deletions.  (2) A database built above compression level 0
 * holds a sample of its k-mers: the figures describe exactly what the search of that file can hit, not the genomes.  (3) Words
 * are compared as stored: a neighbour on the other strand counts only if the database holds it.
 *
 * UTREE_E_ARG (a NULL db_path, report_path or stats) is returned before a file is opened, and the file is read before a device
 * is touched.  A failed call leaves neither output file behind; utree_last_hip_error has the detail.  The whole database is
 * resident on `device` as sorted (word, label) arrays, 12 bytes per node (20 for W = 16), filled in the merge's passes
 * (n_passes); fewer than 2^32 - 1 nodes (UTREE_E_UNSUPPORTED), and UTREE_E_NOMEM names the size when they do not fit.  With a
 * pairs_path the distinct pairs are kept with their counts in a table of UTREE_INSPECT_PAIRS entries (default 2^22, at most
 * 2^28); without one only their keys are kept, to count distinct_pairs, in a set of 2^24.  More distinct pairs than that:
 * UTREE_E_NOMEM, and the text names the knob.
 *
 * utree_inspect_write (host only) is the writer of both files.  It takes the input's description, n label texts with their four
 * class counts (kmers follows; entries of equal text are added up; an entry without a node makes no row) and, when pairs_path is
 * given, n_pairs pairs between entries (pairs of equal text pairs are added up), from which pair_events and distinct_pairs are
 * taken; without a pairs_path `p` is not looked at and the two totals are the arguments'.  UTREE_E_ARG, and no file: a NULL
 * argument other than p, pairs_path and stats, a pair that names no entry or whose texts are equal, or pairs that are not
 * symmetric.  stats (or NULL) gets everything but n_passes and the seconds.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    uint64_t kmers;              /* nodes of the database                                                     */
    uint64_t isolated, same, lineage, conflict;     /* summed over all label texts: they add up to kmers      */
    uint64_t pair_events;        /* ordered (node, held neighbour) pairs of different label texts             */
    uint64_t distinct_pairs;     /* distinct ordered (text, text) pairs among them                            */
    uint64_t labels;             /* distinct label texts that nodes carry                                     */
    uint32_t W, I, is_ctr, n_passes;
    uint32_t clean;              /* 1: conflict == 0                                                          */
    uint32_t pad;
    double   seconds;
    double   seconds_neighbours; /* of those, the directory and the neighbour pass on the device              */
} utree_inspect_stats;           /* 104 bytes */

int utree_inspect_file(const char *db_path, const char *report_path, const char *pairs_path, int device,
                       utree_inspect_stats *stats);

typedef struct {
    const char *text; uint32_t len, pad;
    uint64_t isolated, same, lineage, conflict;
} utree_inspect_entry;

typedef struct {
    uint32_t from, to;           /* indices into the entries: the node's text, its neighbour's text */
    uint64_t pairs;
} utree_inspect_pair;

int utree_inspect_write(const utree_compare_input *db, const utree_inspect_entry *e, size_t n, const utree_inspect_pair *p,
                        size_t n_pairs, uint64_t pair_events, uint64_t distinct_pairs, const char *report_path,
                        const char *pairs_path, utree_inspect_stats *stats);

/* ------------------------------------------------------------------------------------------------
 * Long queries tile by tile (`utree-tiles`; no counterpart in the reference, which gives a query ONE vote over all of its k-mers,
 * itree.c:1044-1088: a 2-Mb contig that is 85 % one taxon and 15 % another reads like one that is uniformly the first).  A tile is a
 * stretch of a query classified as a read of its own; a tile is a VIEW into the bytes of the query that are already in HBM, never a copy.
 *   Parameters.  W = tile_bp, S = step_bp, in bases, 1 <= S <= W <= UTREE_TILE_MAX_BP (16 777 214: the longest line the framing takes);
 *     anything else is UTREE_E_ARG.
 *   Tiles.  A query is framed exactly as the search frames it; its length is L.  n = 1 if L <= W, else 1 + ceil((L - W) / S) tiles;
 *     tile t is q[t*S .. min(t*S + W, L)).  Only the last tile can be shorter than W, and when there is more than one it is longer than
 *     W - S.  (An input format that frames an empty sequence gives it one empty tile.)  L < 2^32 and S >= 1: fewer than 2^32 tiles a query.
 *   Result.  A tile's utree_result is what utree_classify_batch gives for that byte range as a read of its own; with RC that is
 *     tile + 'N' + revcomp(tile), what the reference does with a record holding those bases (itree.c:891-898).
 *   tiles.tsv.  A tile with found > 0 has one line: the reference's output line (itree.c:1032, 1040, 1096) under the name
 *     <name>:<start>-<end>, 1-based and inclusive (the region syntax of `samtools faidx`); query order, then tile order; found == 0 prints
 *     nothing.  The file is byte for byte what `xtree-searchGG db split.fa out.txt 1 [RC]` of the reference writes for the FASTA that holds
 *     one two-line record ><name>:<start>-<end> per tile.
 *   segments.tsv (optional).  Within a query, maximal runs of consecutive tiles of equal class: both unclassified (found == 0), or both
 *     classified with the same taxon TEXT (two labels may print one text; the empty taxon is a classified class of its own).  One line a run,
 *         name \t start \t end \t n_tiles \t C|U \t taxon \t found
 *     start = the first tile's, end = the last tile's, taxon empty for U, found = the sum of the tiles'.  Every query has at least one
 *     line, and the n_tiles column sums to the tiles.
 *   Not supported: pairs (a tile across the joining 'N' means nothing), the rank-specific search, more than one device.
 *
 * Device side, two calls, both asynchronous on `stream` and without state outside what the caller passes.  utree_classify_batch then takes
 * (d_bases, d_toff, d_tlen) unchanged.  What makes that right: no kernel of the classify path writes d_bases or looks at a read's
 * neighbour (there is no d_off[r + 1] anywhere), so overlapping views are reads like any other; its workspace is sized from the total_bases
 * it is GIVEN (dev_image.c: carve), not from the buffer, so a sum of tile lengths above the buffer's size is an ordinary figure.  Pass the
 * meta record's exact total_bases and max_len.  A larger total_bases only sizes more workspace; a larger max_len is also answered
 * correctly but may pick the kernels of longer reads, so it costs time.
 * ---------------------------------------------------------------------------------------------- */
#define UTREE_TILE_MAX_BP 16777214u
#define UTREE_TILES_MAX_BATCH (1u << 21)      /* tiles a call of utree_tiles_views takes: the search's reads per batch */
/* total_tiles: of the batch (both calls write it).  total_bases / max_len: of the range's tiles (utree_tiles_views; 0 from utree_tiles_plan).
 * error: 0; 1 (utree_tiles_views): the range ends behind total_tiles -- nothing was written.  utree_tiles_plan has nothing to report and
 * writes 0: the word is there so that a caller checks one field after either call. */
typedef struct { uint64_t total_tiles, total_bases; uint32_t max_len, error; } utree_tiles_meta;
size_t utree_tiles_workspace_bytes(const utree_dev *dev, uint32_t n_reads);
/* d_tile_first[r] = tiles of the queries in front of r (n_reads + 1 entries; the last is the batch's total): one count kernel and the scan
 * the hit map uses. */
int utree_tiles_plan(utree_dev *dev, const uint32_t *d_len, uint32_t n_reads, uint32_t tile_bp, uint32_t step_bp, uint64_t *d_tile_first,
                     utree_tiles_meta *d_meta, void *d_workspace, size_t workspace_bytes, void *stream);
/* Tiles [first_tile, first_tile + n_tiles) of the batch's numbering, n_tiles <= UTREE_TILES_MAX_BATCH; for the j-th of them d_toff[j] =
 * d_off[q] + t*S (absolute, as utree_classify_batch takes it), d_tlen[j], d_tquery[j] = q, d_tindex[j] = t.  One thread a tile, its query
 * found by binary search in d_tile_first: a query of one tile and one of 30 000 load the lanes alike.  A range may begin and end inside a
 * query.  *d_meta is complete once the stream has drained. */
int utree_tiles_views(utree_dev *dev, const uint64_t *d_off, const uint32_t *d_len, uint32_t n_reads, uint32_t tile_bp, uint32_t step_bp,
                      const uint64_t *d_tile_first, uint64_t first_tile, uint32_t n_tiles, uint64_t *d_toff, uint32_t *d_tlen,
                      uint32_t *d_tquery, uint32_t *d_tindex, utree_tiles_meta *d_meta, void *stream);

/* Host only, thread-safe: the two files' lines for n tiles in order.  Tile j belongs to query q = tquery[j], whose name is
 * h_buf[name_off[q] .. + name_len[q]) and whose length is seq_len[q]; tindex[j] is its number within q.  Both return the bytes written, or
 * (size_t)-1 when cap is too small or a result names a label that is none of ctr's -- as utree_hitmap_format.
 * utree_tiles_format: one line per tile with found > 0; everything behind the name is written by the code utree_format_records uses.
 * *classified (may be NULL) += lines written. */
size_t utree_tiles_format(const utree_ctr *ctr, const uint8_t *h_buf, const uint64_t *name_off, const uint32_t *name_len,
                          const uint32_t *seq_len, uint32_t tile_bp, uint32_t step_bp, const uint32_t *tquery, const uint32_t *tindex,
                          const utree_result *h_res, size_t n, char *h_out, size_t cap, uint64_t *classified);
/* The run that is open behind the tiles seen so far.  Zero it in front of a query's first tile; a caller that formats a query's tiles in
 * several calls (its tiles may straddle sub-batches) passes the same state to each, and flush != 0 with the last, which closes the open run.
 * A call that returns (size_t)-1 leaves the state as it was. */
typedef struct {
    uint32_t open, query;        /* a run is open, of this query                           */
    uint64_t start, end;         /* 1-based, inclusive                                      */
    uint64_t n_tiles, found;
    uint32_t classified, label;  /* C or U; the label whose first taxon_len bytes it prints */
    uint64_t taxon_len;
} utree_tiles_run;               /* 56 bytes */
/* *segments (may be NULL) += lines written. */
size_t utree_tiles_segments_format(const utree_ctr *ctr, const uint8_t *h_buf, const uint64_t *name_off, const uint32_t *name_len,
                                   const uint32_t *seq_len, uint32_t tile_bp, uint32_t step_bp, const uint32_t *tquery,
                                   const uint32_t *tindex, const utree_result *h_res, size_t n, int flush, utree_tiles_run *state,
                                   char *h_out, size_t cap, uint64_t *segments);

/* The whole run: reads_path framed as the search frames it (input_format: UTREE_INPUT_*; gzip with the opt-in formats), every query cut
 * into tiles on the device, the tiles classified in sub-batches of at most UTREE_TILES_BATCH (environment; default and most
 * UTREE_TILES_MAX_BATCH), tiles_path and -- when not NULL -- segments_path written.  `size` of both structs is sizeof the struct.
 * Every argument check comes before ctr or dev is looked at: UTREE_E_ARG for a NULL ctr, dev, reads_path, tiles_path, params or stats, a
 * wrong size, W or S out of range, do_rc other than 0 / 1, an input_format that is none.  A framing error ends the run as it ends the
 * search: the tiles of the queries framed in front of it are written, stats->fasta_error says what, UTREE_E_FASTA.  A run that fails for
 * another reason leaves neither file (UTREE_E_DEVICE also when a tile's result names a label ctr does not have: ctr and dev are of
 * different databases). */
typedef struct {
    uint32_t size;
    uint32_t tile_bp, step_bp;
    int32_t  do_rc, input_format, host_threads;
} utree_tiles_params;            /* 24 bytes */
typedef struct {
    uint32_t size, pad;
    uint64_t n_queries, n_tiles, classified, segments;   /* segments 0 without a segments_path */
    uint64_t bytes_in, n_batches;
    utree_fasta_error fasta_error;
    double   seconds_total, seconds_device;              /* of those, upload to results on the host */
} utree_tiles_stats;             /* 88 bytes */
int utree_tiles_file(const utree_ctr *ctr, utree_dev *dev, const char *reads_path, const char *tiles_path, const char *segments_path,
                     const utree_tiles_params *params, utree_tiles_stats *stats);

#ifdef __cplusplus
}
#endif
#endif
