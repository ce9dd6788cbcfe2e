/* search_dev.h -- the device text pipeline of the whole-file search (search_dev.c), private. */
#ifndef UTREE_SEARCH_DEV_H
#define UTREE_SEARCH_DEV_H
#include "utree_internal.h"
#include "reports.h"

#define LINELEN_MAX 16777216u                  /* itree.c:836 */
/* bytes per chunk (search_dev.c) or per slot and input (search.c): `dflt`; UTREE_CHUNK_BYTES lowers it (tests: many chunk boundaries, and a
 * carry in each file, of a small input) */
static inline size_t utree_chunk_bytes(size_t dflt) {
    const char *e = getenv("UTREE_CHUNK_BYTES");
    return e && atoll(e) >= 64 && (size_t)atoll(e) < dflt ? (size_t)atoll(e) : dflt;
}

/* not an error of the ABI: the input needs the host framing (search.c runs it next) */
#define UTREE_RETRY_HOST 1000

/* When the output cannot seek (a pipe, a FIFO, a tty) the chunks in front of the one that needs the host framing are already out: the
 * host pipeline then CONTINUES -- same descriptor, the input from `in_off` on, the counts so far -- instead of starting over (O_TRUNC does
 * nothing to a pipe: its reader would get the first chunks twice, and closing a FIFO can end its reader).  fo < 0: nothing to continue from,
 * the host pipeline opens the output itself. */
typedef struct { int fo; long long in_off; uint64_t n_reads, good_finds, bytes_in, bytes_out; int parts; } utree_search_resume;
/* parts > 1 (UTREE_OUTPUT_PARTS): the output goes to <out>.part000 ... in input order; a search the host pipeline takes over writes all of it
 * into part 000 and leaves the others empty (the parts' concatenation is the output either way) */
#define UTREE_MAX_OUT_PARTS 64
int utree_output_parts(void);

int utree_search_file_device(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *fasta_path, const char *out_path,
                             int do_rc, int host_threads, utree_reports *rep, utree_search_stats *stats, uint64_t *progress_printed,
                             utree_search_resume *resume);
/* rep: NULL, or the search's reports: a chunk's reads are added to its device's once its output is committed (a chunk that a hand-over to
 * the host pipeline drops is not counted).
 * *progress_printed: "Searched N queries..." lines already on stdout when the call gives up with UTREE_RETRY_HOST: the host
 * pipeline that runs the file again does not print those a second time (the reference prints each once, itree.c:878) */
void utree_search_ctx_free(void *ctx);

/* one request that utree_search_run (search_entry.c) has checked: the search and its reports (search.c) */
int utree_search_checked(const utree_ctr *ctr, utree_dev **devs, int n_dev, const utree_search_request *req, utree_search_stats *stats);

#endif
