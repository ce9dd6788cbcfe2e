/* search.c -- whole-file search: XT_doSearch32's GG branch (itree.c:833-1108) over one or more device
 * images.  Host orchestration in C, four overlapped stages connected by a ring of chunk slots:
 *
 *   reader   : parallel pread of the next ~96 MiB of FASTA into pinned memory, frame the reads (fasta.c;
 *              the reference does this under `omp critical`, itree.c:867-874 -- its scaling limit)
 *   gpu      : shard the framed reads contiguously over the GPUs; per GPU copy the shard's byte span to HBM
 *              as it stands, run the batch kernels, copy the 24-byte results back
 *   formatter: format the lines with a thread team
 *   writer   : write them in input order (= what the reference writes with one thread; with more threads it
 *              writes a permutation)
 *
 * Paired-end input (a request's mates_path / interleaved) takes the same four stages with a second input: the reader frames both files and commits the
 * pairs both buffers hold, the gpu stage uploads both mates' bytes and joins them on the device (pairs_kernels.hip) in front of the batch
 * kernels; formatter and writer see one query per pair, named by mate 1.
 *
 * A hit map (a request's hitmap_path) rides the same slots: the gpu stage launches utree_hitmap_batch behind a shard's classify call on the
 * same device buffers and brings the runs back, the formatter makes the map's lines next to the output's, and the writer commits both.
 *
 * Each read's redistributed label (a request's redistribute_reads_path) is known only after the last read: the gpu stage classifies through the
 * keys entry point and brings a shard's keys back next to its results, the formatter makes one spool record per query that prints a line --
 * key, device handle, name --, the writer appends them to <path>.spool together with the chunk's output lines, and reports.c assigns the spooled
 * keys after the solve.  Host memory does not grow with the number of reads.
 */
#define _FILE_OFFSET_BITS 64
#define _GNU_SOURCE
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <errno.h>
#include <fcntl.h>
#include <pthread.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>
#ifdef _OPENMP
#include <omp.h>
#endif
#include "ctr_host.h"
#include "dev_image.h"
#include "search_dev.h"
#include "reports.h"
#include "pairs_kernels.h"
#include "hitmap.h"

#define CHUNK_BYTES ((size_t)96 << 20)        /* must hold two maximal (16 MiB) lines                    */
#define MAX_READS_PER_BATCH ((size_t)2 << 20)  /* more reads in a chunk (tiny reads) simply take another batch */
#define NSLOTS 4
#define READ_THREADS 4

enum { S_EMPTY = 0, S_FRAMED, S_DONE, S_FORMATTED };
enum { PAIRS_NONE = 0, PAIRS_TWO_FILES, PAIRS_INTERLEAVED };
#define FMT_MAX_THREADS 16

/* paired input: the second mates of a slot's pairs -- a buffer of their own (two files) or spans of the slot's buffer (interleaved) */
typedef struct {
    uint8_t *h_buf;                            /* pinned; two files only                                    */
    uint64_t *seq_off, *name_off, *rel_off;
    uint32_t *seq_len, *name_len;
} mate_t;

typedef struct {
    uint8_t *h_buf;                            /* pinned: the chunk as read from the file                   */
    size_t have;                               /* valid bytes                                               */
    size_t nr, used;                           /* framed reads, bytes they cover                            */
    uint64_t *seq_off, *name_off, *rel_off;
    uint32_t *seq_len, *name_len;
    utree_result *h_res;                       /* pinned                                                    */
    int frame_rc, last;
    utree_fasta_error ferr;
    int state;
    char *fmt_buf[FMT_MAX_THREADS];            /* formatted lines, one piece per formatting thread, in input order */
    size_t fmt_cap[FMT_MAX_THREADS], fmt_len[FMT_MAX_THREADS];
    int fmt_T;
    uint64_t good;
    mate_t m2;                                 /* paired input only                                         */
    utree_pairs_meta *h_meta;                  /* pinned, one per device: what the join reported            */
    /* hit map only: per device its shard [hm_first, + hm_count) of the slot, the shard's run offsets (hm_count + 1 of them at h_run_off +
     * hm_first + g, relative to the shard's first run) and its runs at h_runs + hm_base */
    utree_hitmap_meta *h_hm_meta;              /* pinned, one per device                                    */
    uint64_t *h_run_off;                       /* pinned, MAX_READS_PER_BATCH + n_dev                       */
    utree_hit_run *h_runs; size_t runs_cap;    /* pinned, grows geometrically                               */
    size_t *hm_first, *hm_count; uint64_t *hm_base;
    char *hm_buf[FMT_MAX_THREADS];             /* the map's lines, pieces as fmt_buf's                      */
    size_t hm_cap[FMT_MAX_THREADS], hm_len[FMT_MAX_THREADS];
    /* a report that reads the names only: the names' offsets relative to their shard's uploaded span, and their lengths behind them */
    uint32_t *h_names;                         /* pinned, 2 * MAX_READS_PER_BATCH                           */
    /* redistributed reads only: every read's key (of the table of the device handle that classified it: read r went to handle r / per), and
     * the spool records of the queries that print a line, pieces as fmt_buf's */
    uint32_t *h_key;                           /* pinned, MAX_READS_PER_BATCH                               */
    size_t per;
    char *sp_buf[FMT_MAX_THREADS];
    size_t sp_cap[FMT_MAX_THREADS], sp_len[FMT_MAX_THREADS];
} slot_t;

static int slot_alloc(slot_t *s, size_t chunk, int paired, int n_dev, int hitmap, int names, int keys) {
    if (s->h_buf) return UTREE_OK;
    if (keys && hipHostMalloc((void **)&s->h_key, MAX_READS_PER_BATCH * 4, hipHostMallocDefault) != hipSuccess) return UTREE_E_NOMEM;
    if (names && hipHostMalloc((void **)&s->h_names, 2 * MAX_READS_PER_BATCH * 4, hipHostMallocDefault) != hipSuccess) return UTREE_E_NOMEM;
    if (hitmap) {
        if (hipHostMalloc((void **)&s->h_hm_meta, (size_t)n_dev * sizeof(utree_hitmap_meta), hipHostMallocDefault) != hipSuccess) return UTREE_E_NOMEM;
        if (hipHostMalloc((void **)&s->h_run_off, (MAX_READS_PER_BATCH + (size_t)n_dev) * 8, hipHostMallocDefault) != hipSuccess) return UTREE_E_NOMEM;
        s->hm_first = (size_t *)calloc((size_t)n_dev, sizeof(size_t)); s->hm_count = (size_t *)calloc((size_t)n_dev, sizeof(size_t));
        s->hm_base = (uint64_t *)calloc((size_t)n_dev, 8);
        if (!s->hm_first || !s->hm_count || !s->hm_base) return UTREE_E_NOMEM;
    }
    if (paired) {
        mate_t *m = &s->m2;
        if (paired == PAIRS_TWO_FILES && hipHostMalloc((void **)&m->h_buf, chunk + 64, hipHostMallocDefault) != hipSuccess) return UTREE_E_NOMEM;
        if (hipHostMalloc((void **)&m->rel_off, MAX_READS_PER_BATCH * 8, hipHostMallocDefault) != hipSuccess) return UTREE_E_NOMEM;
        if (hipHostMalloc((void **)&m->seq_len, MAX_READS_PER_BATCH * 4, hipHostMallocDefault) != hipSuccess) return UTREE_E_NOMEM;
        if (hipHostMalloc((void **)&s->h_meta, (size_t)n_dev * sizeof(utree_pairs_meta), hipHostMallocDefault) != hipSuccess) return UTREE_E_NOMEM;
        m->seq_off = (uint64_t *)malloc(MAX_READS_PER_BATCH * 8); m->name_off = (uint64_t *)malloc(MAX_READS_PER_BATCH * 8);
        m->name_len = (uint32_t *)malloc(MAX_READS_PER_BATCH * 4);
        if (!m->seq_off || !m->name_off || !m->name_len) return UTREE_E_NOMEM;
    }
    if (hipHostMalloc((void **)&s->h_buf, chunk + 64, hipHostMallocDefault) != hipSuccess) return UTREE_E_NOMEM;
    if (hipHostMalloc((void **)&s->h_res, MAX_READS_PER_BATCH * sizeof(utree_result), hipHostMallocDefault) != hipSuccess) return UTREE_E_NOMEM;
    if (hipHostMalloc((void **)&s->rel_off, MAX_READS_PER_BATCH * 8, hipHostMallocDefault) != hipSuccess) return UTREE_E_NOMEM;
    if (hipHostMalloc((void **)&s->seq_len, MAX_READS_PER_BATCH * 4, hipHostMallocDefault) != hipSuccess) return UTREE_E_NOMEM;
    s->seq_off = (uint64_t *)malloc(MAX_READS_PER_BATCH * 8); s->name_off = (uint64_t *)malloc(MAX_READS_PER_BATCH * 8);
    s->name_len = (uint32_t *)malloc(MAX_READS_PER_BATCH * 4);
    return (s->seq_off && s->name_off && s->name_len) ? UTREE_OK : UTREE_E_NOMEM;
}

static void slot_free(slot_t *s) {
    void *pinned[] = {s->h_buf, s->h_res, s->rel_off, s->seq_len, s->m2.h_buf, s->m2.rel_off, s->m2.seq_len, s->h_meta, s->h_hm_meta, s->h_run_off,
                      s->h_runs, s->h_names, s->h_key};
    for (size_t i = 0; i < sizeof pinned / sizeof pinned[0]; ++i) if (pinned[i]) hipHostFree(pinned[i]);
    free(s->seq_off); free(s->name_off); free(s->name_len);
    free(s->m2.seq_off); free(s->m2.name_off); free(s->m2.name_len);
    free(s->hm_first); free(s->hm_count); free(s->hm_base);
    for (int t = 0; t < FMT_MAX_THREADS; ++t) { free(s->hm_buf[t]); free(s->fmt_buf[t]); free(s->sp_buf[t]); }
}

typedef struct {
    utree_dev *dev;
    hipStream_t stream;
    uint8_t *d_buf; uint64_t *d_off; uint32_t *d_len; utree_result *d_out; void *d_ws; size_t ws_bytes;
    /* paired input: the second mates as uploaded, and the joined batch the kernels see */
    uint8_t *d_buf2, *d_joined; uint64_t *d_off2, *d_joff; uint32_t *d_len2, *d_jlen; utree_pairs_meta *d_meta; size_t joined_cap;
    uint64_t want_total;                        /* joined bytes of the shard in flight, as the host counted them */
    /* hit map: the shard's run offsets, runs (the worst case: one per window) and meta, and the call's workspace */
    uint64_t *d_run_off; utree_hit_run *d_runs; uint64_t runs_cap; utree_hitmap_meta *d_hm_meta; void *d_hm_ws; size_t hm_ws_bytes;
    uint32_t *d_name_off, *d_name_len;          /* a report that reads the names only: relative to d_buf      */
    uint32_t *d_key;                            /* redistributed reads only: the shard's keys                 */
} gpu_ctx;

/* one input file: plain (a team of pread) or, with an opt-in format, through zlib (plain and gzip alike) */
typedef struct { int fd; gzFile gz; off_t pos; int eof; } input_t;

typedef struct {
    const utree_ctr *ctr;
    const utree_search_request *req;            /* what is searched: the paths, do_rc, rank (non-NULL: the rank-specific `xtree-search`, rank.c, one device) */
    utree_reports *rep;                         /* non-NULL: the search feeds reports (reports.h)            */
    gpu_ctx *G; int n_dev;
    input_t in[2];                              /* input; [1]: the mates file of a paired search             */
    int fo;                                     /* output                                                   */
    int names;                                  /* a report reads the names (utree_reports_wants_names): they go up with the shard */
    int hm, fh;                                 /* a hit map is made; its file (-1 once writing it has failed: the search goes on) */
    char *hm_msg;                               /* why the map could not be written ("" = it could): the writer's to set            */
    int keys, fs;                               /* every read's key is brought back and spooled; the spool (-1 once writing it has failed: the search goes on) */
    char *sp_msg;                               /* why the spool could not be written ("" = it could): the writer's to set          */
    off_t out_pos;
    int paired;                                 /* PAIRS_*, from the request's mates_path / interleaved     */
    size_t chunk;                               /* bytes per slot and input: CHUNK_BYTES; a paired search honours UTREE_CHUNK_BYTES */
    /* what utree_last_hip_error is to say: each text has ONE writer -- the reader stage (UTREE_E_PAIRS) and the gpu stage (a join the
     * device refused) --, and the caller's thread reads the one that belongs to the search's code once the stages have ended */
    char msg_pairs[512], msg_join[256];
    int host_threads;                           /* the request's, resolved                                   */
    int input_format;                           /* the request's UTREE_INPUT_*, AUTO resolved by the reader  */
    slot_t slot[NSLOTS];
    pthread_mutex_t mu; pthread_cond_t cv;
    int rc;                                     /* first error of any stage                                  */
    int stop;
    utree_search_stats st;
    double t_read, t_frame, t_gpu, t_format, t_write;
    uint32_t max_label;
    uint64_t progress_printed;                  /* progress lines the device pipeline printed before it handed the file back */
} pipe_t;

static void set_error(pipe_t *P, int rc) {
    pthread_mutex_lock(&P->mu);
    if (!P->rc) P->rc = rc;
    P->stop = 1;
    pthread_cond_broadcast(&P->cv);
    pthread_mutex_unlock(&P->mu);
}
/* wait until slot reaches `state` (or the pipeline stops); returns 0 if stopped */
static int wait_state(pipe_t *P, slot_t *s, int state) {
    pthread_mutex_lock(&P->mu);
    while (s->state != state && !P->stop) pthread_cond_wait(&P->cv, &P->mu);
    int ok = s->state == state;
    pthread_mutex_unlock(&P->mu);
    return ok;
}
static void set_state(pipe_t *P, slot_t *s, int state) {
    pthread_mutex_lock(&P->mu);
    s->state = state;
    pthread_cond_broadcast(&P->cv);
    pthread_mutex_unlock(&P->mu);
}

/* ---- stage 1: read + frame ------------------------------------------------------------------- */
/* more of `in` behind buf[0 .. *have), up to `cap` bytes in all; in->eof is set where the file ends */
static int fill_chunk(input_t *in, uint8_t *buf, size_t *have_io, size_t cap) {
    size_t have = *have_io;
    if (in->eof || have >= cap) return UTREE_OK;
    if (in->gz) {                                 /* opt-in formats: zlib reads plain and gzip input alike */
        size_t want = cap - have, done = 0;
        while (done < want) {
            int r = gzread(in->gz, buf + have + done, (unsigned)(want - done > (1u << 30) ? (1u << 30) : want - done));
            if (r < 0) return UTREE_E_IO;
            if (r == 0) { in->eof = 1; break; }
            done += (size_t)r;
        }
        have += done;
    } else {
        /* parallel pread: the page-cache copy is the cost; several threads stream it */
        size_t want = cap - have;
        ssize_t got[READ_THREADS];
        int T = READ_THREADS;
        const off_t file_pos = in->pos;
        const int fd = in->fd;
#pragma omp parallel for num_threads(T) schedule(static, 1)
        for (int t = 0; t < T; ++t) {
            size_t a = want * (size_t)t / (size_t)T, b = want * (size_t)(t + 1) / (size_t)T, done = 0;
            got[t] = 0;
            while (done < b - a) {
                ssize_t r = pread(fd, buf + have + a + done, b - a - done, file_pos + (off_t)(a + done));
                if (r < 0) { got[t] = -1; break; }
                if (r == 0) break;
                done += (size_t)r; got[t] = (ssize_t)done;
            }
        }
        size_t total = 0;
        for (int t = 0; t < T; ++t) {
            if (got[t] < 0) return UTREE_E_IO;
            size_t seg = want * (size_t)(t + 1) / (size_t)T - want * (size_t)t / (size_t)T;
            total += (size_t)got[t];
            if ((size_t)got[t] < seg) { in->eof = 1; break; }       /* short segment: end of file inside it */
        }
        have += total; in->pos += (off_t)total;
    }
    *have_io = have;
    return UTREE_OK;
}

static int frame_chunk(int format, uint8_t *buf, size_t have, int final, size_t max_reads, uint64_t *seq_off, uint32_t *seq_len,
                       uint64_t *name_off, uint32_t *name_len, size_t *nr, size_t *used, utree_fasta_error *ferr) {
    return format != UTREE_INPUT_REFERENCE
        ? utree_reads_frame(buf, have, final, format, max_reads, seq_off, seq_len, name_off, name_len, nr, used, ferr)
        : utree_fasta_frame(buf, have, final, max_reads, seq_off, seq_len, name_off, name_len, nr, used, ferr);
}

static void *reader_main(void *arg) {
    pipe_t *P = (pipe_t *)arg;
    input_t *in = &P->in[0];
    size_t carry = 0;                           /* bytes of an incomplete read carried into the next chunk */
    const uint8_t *carry_src = NULL;
    for (int i = 0; !in->eof || carry; ++i) {
        slot_t *s = &P->slot[i % NSLOTS];
        if (!wait_state(P, s, S_EMPTY)) return NULL;
        if (i < NSLOTS) {                       /* pinned memory is slow to allocate: do it while earlier chunks are in flight */
            int arc = slot_alloc(s, P->chunk, PAIRS_NONE, P->n_dev, P->hm, P->names, P->keys);
            if (arc) { set_error(P, arc); return NULL; }
        }
        if (carry) memmove(s->h_buf, carry_src, carry);
        size_t have = carry;
        double t0 = now_s();
        if (fill_chunk(in, s->h_buf, &have, P->chunk)) { set_error(P, UTREE_E_IO); return NULL; }
        double t1 = now_s();
        const int eof = in->eof;
        s->have = have;
        s->nr = 0; s->used = 0; s->frame_rc = UTREE_OK; s->last = 0;
        if (have && P->input_format == UTREE_INPUT_AUTO)
            P->input_format = s->h_buf[0] == '@' ? UTREE_INPUT_FASTQ : UTREE_INPUT_FASTA_MULTILINE;
        if (have) {
            s->frame_rc = frame_chunk(P->input_format, s->h_buf, have, eof, MAX_READS_PER_BATCH, s->seq_off, s->seq_len, s->name_off,
                                      s->name_len, &s->nr, &s->used, &s->ferr);
            if (s->frame_rc != UTREE_OK && s->frame_rc != UTREE_E_FASTA) { set_error(P, s->frame_rc); return NULL; }
            if (s->frame_rc == UTREE_OK && !s->nr && !s->used && !eof) {
                s->frame_rc = UTREE_E_FASTA; s->ferr.code = 5; s->ferr.read_index = 0;   /* a line pair larger than a chunk */
            }
        }
        P->t_read += t1 - t0; P->t_frame += now_s() - t1;
        carry = have - s->used; carry_src = s->h_buf + s->used;
        if (s->frame_rc == UTREE_E_FASTA) { carry = 0; in->eof = 1; }
        if (in->eof && !carry) s->last = 1;
        if (in->eof && carry && s->frame_rc == UTREE_OK && s->used == 0 && s->nr == 0) { s->last = 1; carry = 0; }
        set_state(P, s, S_FRAMED);
        if (s->last) break;
    }
    return NULL;
}

/* ---- stage 1, paired input ---------------------------------------------------------------------
 * Both inputs are framed by the chosen format's framing; a slot commits the pairs BOTH of its buffers hold and the rest of each file goes to
 * the next slot, so the two buffers of a slot always begin at the same pair whatever the lengths of the files' headers.  Interleaved input
 * is one file whose records 2i and 2i+1 are pair i; an odd record at the end of a slot is carried. */
typedef struct {                                /* what a slot did not commit: framed records [from, nr) and the bytes behind them */
    const uint8_t *buf; const uint64_t *name_off, *seq_off; const uint32_t *seq_len;
    size_t from, nr, used, have;
} carry_t;

/* Multi-line FASTA was compacted in place when it was framed, so a framed record is written out again as header line + sequence + '\n'
 * (at most one byte more than it took: the file's last line may lack its newline; the buffers have 64 bytes to spare); the other formats'
 * bytes stand as they were read and are framed again. */
static size_t carry_over(uint8_t *dst, const carry_t *c, int format) {
    size_t w = 0;
    if (!c->buf) return 0;
    if (format == UTREE_INPUT_FASTA_MULTILINE) {
        for (size_t r = c->from; r < c->nr; ++r) {
            const size_t a = (size_t)c->name_off[r] - 1, b = (size_t)c->seq_off[r] + c->seq_len[r];
            memmove(dst + w, c->buf + a, b - a); w += b - a;
            dst[w++] = '\n';
        }
        memmove(dst + w, c->buf + c->used, c->have - c->used); w += c->have - c->used;
    } else {
        const size_t a = c->from < c->nr ? (size_t)c->name_off[c->from] - 1 : c->used;
        memmove(dst, c->buf + a, c->have - a); w = c->have - a;
    }
    return w;
}

/* How a slot of a paired search ends, once its np pairs are known.  Per input k: the slot commits done[k] of the nr[k] records framed in its
 * buffer of have[k] bytes, of which framing took used[k]; frc[k] / fe[k]: a malformed record stopped the framing (it is record nr[k] of the
 * buffer); recs[k]: records the slots before committed.  In this order:
 *   1. a malformed record that is the NEXT record of its file (interleaved: or the mate of the next) ends the search with its own code; its
 *      number counts that file's records.  One further on is carried and met again;
 *   2. one file is used up -- end of file, nothing left in the buffer -- and the other's buffer holds more: UTREE_E_PAIRS (interleaved: the
 *      file is used up with an odd record left); the slot's complete pairs go through the stages first;
 *   3. every file is used up: the last slot;
 *   4. no pair, and a FULL buffer that holds no complete record (interleaved: no two): "sequence too long", as for single reads;
 *   else the next slot goes on behind done[k] (a file that ended exactly at a buffer's end is seen to be used up there). */
static void pairs_verdict(pipe_t *P, slot_t *s, size_t np, const size_t *done, const size_t *nr, const size_t *used, const size_t *have,
                          const int *frc, const utree_fasta_error *fe, const uint64_t *recs, uint64_t pairs) {
    const int two = P->paired == PAIRS_TWO_FILES, nin = two ? 2 : 1;
    int rest[2] = {0, 0}, over[2] = {0, 0};                                               /* the buffer holds more of the file; the file is used up */
    for (int k = 0; k < nin; ++k) {
        rest[k] = done[k] < nr[k] || used[k] < have[k];
        over[k] = !rest[k] && P->in[k].eof;
    }
    for (int k = 0; k < nin; ++k)                                                         /* 1 */
        if (frc[k] == UTREE_E_FASTA && nr[k] - done[k] <= (two ? 0u : 1u)) {
            s->frame_rc = UTREE_E_FASTA; s->ferr = fe[k]; s->ferr.read_index += recs[k];   /* (the framing counts from the buffer's first record) */
            return;
        }
    if (two && over[0] != over[1] && rest[over[0] ? 1 : 0]) {                             /* 2 */
        const int k = over[0] ? 0 : 1;                                                    /* the shorter file */
        s->frame_rc = UTREE_E_PAIRS;
        snprintf(P->msg_pairs, sizeof P->msg_pairs, "paired input: %s file %s ends after %llu records, %s goes on", k ? "the mates" : "the reads",
                 k ? P->req->mates_path : P->req->reads_path, (unsigned long long)(recs[k] + done[k]), k ? P->req->reads_path : P->req->mates_path);
    } else if (!two && P->in[0].eof && used[0] >= have[0] && (nr[0] & 1)) {
        s->frame_rc = UTREE_E_PAIRS;
        snprintf(P->msg_pairs, sizeof P->msg_pairs, "paired input: the interleaved file %s holds an odd number of records (%llu): its last read has no mate",
                 P->req->reads_path, (unsigned long long)(recs[0] + nr[0]));
    } else if (over[0] && (!two || over[1])) s->last = 1;                                 /* 3 */
    else if (!np) {                                                                       /* 4 */
        int full = 0;
        for (int k = 0; k < nin; ++k) full |= have[k] >= P->chunk && nr[k] < (two ? 1u : 2u) && (k == 0 || nr[0] > 0);   /* (the mates are framed only up to the reads' count) */
        if (full) { s->frame_rc = UTREE_E_FASTA; s->ferr.code = 5; s->ferr.read_index = pairs + 1; }
    }
}

static void *reader_pairs_main(void *arg) {
    pipe_t *P = (pipe_t *)arg;
    const int two = P->paired == PAIRS_TWO_FILES, nin = two ? 2 : 1;
    carry_t cy[2];
    uint64_t recs[2] = {0, 0}, pairs = 0;       /* records of each file, pairs, committed by the slots before */
    memset(cy, 0, sizeof cy);
    for (int i = 0;; ++i) {
        slot_t *s = &P->slot[i % NSLOTS];
        mate_t *m = &s->m2;
        if (!wait_state(P, s, S_EMPTY)) return NULL;
        if (i < NSLOTS) {
            int arc = slot_alloc(s, P->chunk, P->paired, P->n_dev, P->hm, P->names, P->keys);
            if (arc) { set_error(P, arc); return NULL; }
        }
        uint8_t *buf[2] = {s->h_buf, m->h_buf};
        uint64_t *seq_off[2] = {s->seq_off, m->seq_off}, *name_off[2] = {s->name_off, m->name_off};
        uint32_t *seq_len[2] = {s->seq_len, m->seq_len}, *name_len[2] = {s->name_len, m->name_len};
        size_t have[2] = {0, 0}, nr[2] = {0, 0}, used[2] = {0, 0};
        int frc[2] = {UTREE_OK, UTREE_OK};
        utree_fasta_error fe[2];
        double t0 = now_s();
        for (int k = 0; k < nin; ++k) {
            have[k] = carry_over(buf[k], &cy[k], P->input_format);
            if (fill_chunk(&P->in[k], buf[k], &have[k], P->chunk)) { set_error(P, UTREE_E_IO); return NULL; }
        }
        double t1 = now_s();
        if (have[0] && P->input_format == UTREE_INPUT_AUTO)
            P->input_format = buf[0][0] == '@' ? UTREE_INPUT_FASTQ : UTREE_INPUT_FASTA_MULTILINE;
        for (int k = 0; k < nin; ++k) {
            memset(&fe[k], 0, sizeof fe[k]);
            const size_t max_reads = k ? nr[0] : MAX_READS_PER_BATCH;                     /* no more mates than reads */
            if (!have[k] || !max_reads) continue;
            frc[k] = frame_chunk(P->input_format, buf[k], have[k], P->in[k].eof, max_reads, seq_off[k], seq_len[k], name_off[k], name_len[k],
                                 &nr[k], &used[k], &fe[k]);
            if (frc[k] != UTREE_OK && frc[k] != UTREE_E_FASTA) { set_error(P, frc[k]); return NULL; }
        }
        size_t np = two ? (nr[0] < nr[1] ? nr[0] : nr[1]) : nr[0] / 2;
        if (!two)                                                                         /* records 2i, 2i+1 -> pair i (an odd last record stays where it is) */
            for (size_t r = 0; r < np; ++r) {
                m->seq_off[r] = s->seq_off[2 * r + 1]; m->seq_len[r] = s->seq_len[2 * r + 1];
                s->seq_off[r] = s->seq_off[2 * r]; s->seq_len[r] = s->seq_len[2 * r];
                s->name_off[r] = s->name_off[2 * r]; s->name_len[r] = s->name_len[2 * r];
            }
        s->have = have[0]; s->used = used[0]; s->frame_rc = UTREE_OK; s->last = 0;
        memset(&s->ferr, 0, sizeof s->ferr);
        for (size_t r = 0; r < np; ++r)
            if ((uint64_t)s->seq_len[r] + 1 + m->seq_len[r] > LINELEN_MAX) {               /* "sequence too long": the pairs before it are written */
                np = r; s->frame_rc = UTREE_E_FASTA; s->ferr.code = 5; s->ferr.read_index = pairs + r + 1;
                break;
            }
        const size_t done[2] = {two ? np : 2 * np, np};                                   /* records of each file this slot commits */
        if (s->frame_rc == UTREE_OK) pairs_verdict(P, s, np, done, nr, used, have, frc, fe, recs, pairs);
        if (s->frame_rc != UTREE_OK) s->last = 1;
        s->nr = np;
        for (int k = 0; k < nin; ++k) {
            cy[k].buf = buf[k]; cy[k].name_off = name_off[k]; cy[k].seq_off = seq_off[k]; cy[k].seq_len = seq_len[k];
            cy[k].from = done[k]; cy[k].nr = nr[k]; cy[k].used = used[k]; cy[k].have = have[k];
            recs[k] += done[k];
        }
        pairs += np;
        P->t_read += t1 - t0; P->t_frame += now_s() - t1;
        const int last = s->last;
        set_state(P, s, S_FRAMED);
        if (last) break;
    }
    return NULL;
}

/* ---- stage 2: GPU ---------------------------------------------------------------------------- */
#define HIPOK(x) do { if ((x) != hipSuccess) { set_error(P, UTREE_E_HIP); return NULL; } } while (0)
#define HIPE(x) do { if ((x) != hipSuccess) return UTREE_E_HIP; } while (0)      /* ... in what gpu_main and search_file call */

/* the hit map of device g's shard, behind its classify call on the same device buffers; meta and offsets come back with the results */
static int hitmap_launch(pipe_t *P, slot_t *s, size_t g, const utree_batch_view *v, size_t first) {
    gpu_ctx *c = &P->G[g];
    const size_t count = v->n_reads;
    s->hm_first[g] = first; s->hm_count[g] = count;
    int e = utree_hitmap_batch(c->dev, v->d_bases, v->d_off, v->d_len, v->n_reads, v->total_bases, v->do_rc, c->d_run_off, c->d_runs, c->runs_cap, c->d_hm_meta,
                               c->d_hm_ws, c->hm_ws_bytes, c->stream);
    if (e) return e;
    if (hipMemcpyAsync(&s->h_hm_meta[g], c->d_hm_meta, sizeof(utree_hitmap_meta), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return UTREE_E_HIP;
    if (hipMemcpyAsync(s->h_run_off + first + g, c->d_run_off, (count + 1) * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return UTREE_E_HIP;
    return UTREE_OK;
}

/* once the streams have drained: exactly the runs there are, the shards' one after the other, into the slot's pinned buffer */
static int hitmap_fetch(pipe_t *P, slot_t *s) {
    uint64_t runs = 0;
    for (int g = 0; g < P->n_dev; ++g) {
        if (!s->hm_count[g]) continue;
        if (s->h_hm_meta[g].error) {
            snprintf(P->msg_join, sizeof P->msg_join, "the hit map of a batch reported error %u (%llu runs, %llu windows)", s->h_hm_meta[g].error,
                     (unsigned long long)s->h_hm_meta[g].total_runs, (unsigned long long)s->h_hm_meta[g].total_windows);
            return UTREE_E_DEVICE;
        }
        s->hm_base[g] = runs; runs += s->h_hm_meta[g].total_runs;
    }
    if (runs > s->runs_cap) {
        size_t cap = s->runs_cap ? s->runs_cap : (size_t)1 << 20;
        while (cap < runs) cap *= 2;
        if (s->h_runs) hipHostFree(s->h_runs);
        s->h_runs = NULL; s->runs_cap = 0;
        if (hipHostMalloc((void **)&s->h_runs, cap * sizeof(utree_hit_run), hipHostMallocDefault) != hipSuccess) return UTREE_E_NOMEM;
        s->runs_cap = cap;
    }
    for (int g = 0; g < P->n_dev; ++g) {
        if (!s->hm_count[g] || !s->h_hm_meta[g].total_runs) continue;
        if (hipSetDevice(P->G[g].dev->device) != hipSuccess ||
            hipMemcpyAsync(s->h_runs + s->hm_base[g], P->G[g].d_runs, s->h_hm_meta[g].total_runs * sizeof(utree_hit_run), hipMemcpyDeviceToHost,
                           P->G[g].stream) != hipSuccess) return UTREE_E_HIP;
    }
    for (int g = 0; g < P->n_dev; ++g)
        if (s->hm_count[g] && (hipSetDevice(P->G[g].dev->device) != hipSuccess || hipStreamSynchronize(P->G[g].stream) != hipSuccess)) return UTREE_E_HIP;
    return UTREE_OK;
}

/* the names of device g's shard [first, first + count) for the reports that read them: offsets relative to the uploaded span, which begins
 * at h_buf + lo and holds `span` bytes, on the shard's stream */
static int names_upload(pipe_t *P, slot_t *s, size_t g, size_t first, size_t count, size_t lo, size_t span) {
    gpu_ctx *c = &P->G[g];
    if (span >= ((uint64_t)1 << 32)) return UTREE_E_ARG;
    uint32_t *rel = s->h_names + first, *len = s->h_names + MAX_READS_PER_BATCH + first;
    for (size_t r = 0; r < count; ++r) {
        if (s->name_off[first + r] < lo || s->name_off[first + r] - lo + s->name_len[first + r] > span) return UTREE_E_ARG;   /* (cannot happen: a name precedes its read) */
        rel[r] = (uint32_t)(s->name_off[first + r] - lo); len[r] = s->name_len[first + r];
    }
    if (hipMemcpyAsync(c->d_name_off, rel, count * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess) return UTREE_E_HIP;
    if (hipMemcpyAsync(c->d_name_len, len, count * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess) return UTREE_E_HIP;
    return UTREE_OK;
}

/* Stage device g's shard [first, first + count) of slot `s`: the byte span and the framed arrays go up as they stand, on the shard's stream, and
 * *v is the batch the kernels see.  *lo: where in h_buf the uploaded span -- the view's text, with names -- begins. */
static int stage_reads(pipe_t *P, slot_t *s, size_t g, size_t first, size_t count, utree_batch_view *v, size_t *lo_out) {
    gpu_ctx *c = &P->G[g];
    const size_t last = first + count - 1;
    size_t lo = (size_t)s->seq_off[first], hi = (size_t)s->seq_off[last] + s->seq_len[last];
    if (P->names && (size_t)s->name_off[first] < lo) lo = (size_t)s->name_off[first];      /* the span from the first name on: the names are read there */
    uint64_t total = 0; uint32_t mx = 0;
    for (size_t r = first; r <= last; ++r) {
        s->rel_off[r] = s->seq_off[r] - lo; total += s->seq_len[r];
        if (s->seq_len[r] > mx) mx = s->seq_len[r];
    }
    HIPE(hipSetDevice(c->dev->device));
    HIPE(hipMemcpyAsync(c->d_buf, s->h_buf + lo, hi - lo, hipMemcpyHostToDevice, c->stream));
    HIPE(hipMemcpyAsync(c->d_off, s->rel_off + first, count * 8, hipMemcpyHostToDevice, c->stream));
    HIPE(hipMemcpyAsync(c->d_len, s->seq_len + first, count * 4, hipMemcpyHostToDevice, c->stream));
    *v = (utree_batch_view){c->d_buf, c->d_off, c->d_len, (uint32_t)count, total, mx, P->req->do_rc, c->d_buf, hi - lo, c->d_name_off, c->d_name_len, c->stream};
    *lo_out = lo;
    return UTREE_OK;
}

/* ... of a paired search: both mates' byte spans and framed arrays go up as they stand; the device joins them and the batch kernels, the reports
 * included, see one query per pair.  The view's text is mate 1's span. */
static int stage_pairs(pipe_t *P, slot_t *s, size_t g, size_t first, size_t count, utree_batch_view *v, size_t *lo_out) {
    gpu_ctx *c = &P->G[g];
    const int two = P->paired == PAIRS_TWO_FILES;
    mate_t *m = &s->m2;
    const size_t last = first + count - 1;
    size_t lo1 = (size_t)s->seq_off[first], hi1 = (size_t)s->seq_off[last] + s->seq_len[last];
    size_t lo2 = (size_t)m->seq_off[first], hi2 = (size_t)m->seq_off[last] + m->seq_len[last];
    if (P->names && (size_t)s->name_off[first] < lo1) lo1 = (size_t)s->name_off[first];   /* the span from mate 1's first name on: the names are read there */
    if (!two) { hi1 = hi2; lo2 = lo1; }                                        /* interleaved: one span holds both */
    uint64_t total = 0; uint32_t mx = 0;
    for (size_t r = first; r <= last; ++r) {
        s->rel_off[r] = s->seq_off[r] - lo1; m->rel_off[r] = m->seq_off[r] - lo2;
        const uint32_t jl = s->seq_len[r] + 1u + m->seq_len[r];                /* <= LINELEN_MAX: the reader saw to it */
        total += jl;
        if (jl > mx) mx = jl;
    }
    if (total > c->joined_cap) return UTREE_E_ARG;                             /* (cannot happen: the buffers' bytes + one per pair) */
    HIPE(hipSetDevice(c->dev->device));
    HIPE(hipMemcpyAsync(c->d_buf, s->h_buf + lo1, hi1 - lo1, hipMemcpyHostToDevice, c->stream));
    if (two) HIPE(hipMemcpyAsync(c->d_buf2, m->h_buf + lo2, hi2 - lo2, hipMemcpyHostToDevice, c->stream));
    HIPE(hipMemcpyAsync(c->d_off, s->rel_off + first, count * 8, hipMemcpyHostToDevice, c->stream));
    HIPE(hipMemcpyAsync(c->d_len, s->seq_len + first, count * 4, hipMemcpyHostToDevice, c->stream));
    HIPE(hipMemcpyAsync(c->d_off2, m->rel_off + first, count * 8, hipMemcpyHostToDevice, c->stream));
    HIPE(hipMemcpyAsync(c->d_len2, m->seq_len + first, count * 4, hipMemcpyHostToDevice, c->stream));
    /* the host has the lengths: total and max_len are its own, the join's meta comes back with the results and is checked then */
    const int e = utree_pairs_join(c->dev, c->d_buf, c->d_off, c->d_len, two ? c->d_buf2 : c->d_buf, c->d_off2, c->d_len2, (uint32_t)count,
                                   c->d_joined, total, c->d_joff, c->d_jlen, c->d_meta, c->stream);
    if (e) return e;
    c->want_total = total;
    HIPE(hipMemcpyAsync(&s->h_meta[g], c->d_meta, sizeof(utree_pairs_meta), hipMemcpyDeviceToHost, c->stream));
    *v = (utree_batch_view){c->d_joined, c->d_joff, c->d_jlen, (uint32_t)count, total, mx, P->req->do_rc, c->d_buf, hi1 - lo1, c->d_name_off, c->d_name_len, c->stream};
    *lo_out = lo1;
    return UTREE_OK;
}

static void *gpu_main(void *arg) {
    pipe_t *P = (pipe_t *)arg;
    const utree_rank_params *rank = P->req->rank;
    for (int i = 0;; ++i) {
        slot_t *s = &P->slot[i % NSLOTS];
        if (!wait_state(P, s, S_FRAMED)) return NULL;
        double t0 = now_s();
        size_t nr = s->nr, n_dev = (size_t)P->n_dev;
        size_t per = (nr + n_dev - 1) / n_dev;
        s->per = per ? per : 1;
        for (size_t g = 0; g < n_dev && nr && P->paired; ++g) { memset(&s->h_meta[g], 0, sizeof s->h_meta[g]); P->G[g].want_total = 0; }
        for (size_t g = 0; g < n_dev && P->hm; ++g) { s->hm_first[g] = 0; s->hm_count[g] = 0; s->hm_base[g] = 0; }
        for (size_t g = 0; g < n_dev && nr; ++g) {
            gpu_ctx *c = &P->G[g];
            size_t first = g * per; if (first > nr) first = nr;
            size_t count = first + per <= nr ? per : nr - first;
            if (!count) continue;
            utree_batch_view v;
            size_t lo = 0;
            int e = P->paired ? stage_pairs(P, s, g, first, count, &v, &lo) : stage_reads(P, s, g, first, count, &v, &lo);
            if (!e && P->names) e = names_upload(P, s, g, first, count, lo, (size_t)v.text_bytes);   /* (in front of the classify call: a report may read them there) */
            if (!e) e = rank ? utree_rank_batch(c->dev, v.d_bases, v.d_off, v.d_len, v.n_reads, v.total_bases, v.max_len, v.do_rc, rank, c->d_out, c->d_ws,
                                                c->ws_bytes, c->stream)
                             : utree_reports_classify(P->rep, (int)g, c->dev, &v, c->d_out, c->d_ws, c->ws_bytes, P->keys ? c->d_key : NULL);
            if (!e && P->keys && hipMemcpyAsync(s->h_key + first, c->d_key, count * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess) e = UTREE_E_HIP;
            if (!e) e = utree_reports_add(P->rep, (int)g, &v, c->d_out, rank != NULL);
            if (!e && P->hm) e = hitmap_launch(P, s, g, &v, first);
            if (!e && hipMemcpyAsync(s->h_res + first, c->d_out, count * sizeof(utree_result), hipMemcpyDeviceToHost, c->stream) != hipSuccess) e = UTREE_E_HIP;
            if (e) { set_error(P, e); return NULL; }
        }
        for (size_t g = 0; g < n_dev && nr; ++g) {
            HIPOK(hipSetDevice(P->G[g].dev->device));
            HIPOK(hipStreamSynchronize(P->G[g].stream));
            if (!rank) { int pe = utree_classify_poll(P->G[g].dev); if (pe) { set_error(P, pe); return NULL; } }   /* the batches' error words */
            if (P->paired && (s->h_meta[g].error || s->h_meta[g].total_bases != P->G[g].want_total)) {               /* ... and the join's */
                snprintf(P->msg_join, sizeof P->msg_join, "the device join of a batch of pairs reported error %u, %llu joined bytes where the host counted %llu",
                         s->h_meta[g].error, (unsigned long long)s->h_meta[g].total_bases, (unsigned long long)P->G[g].want_total);
                set_error(P, UTREE_E_DEVICE); return NULL;
            }
        }
        if (P->hm && nr) { int he = hitmap_fetch(P, s); if (he) { set_error(P, he); return NULL; } }
        P->t_gpu += now_s() - t0;
        int last = s->last;
        set_state(P, s, S_DONE);
        if (last) return NULL;
    }
}

/* ---- stage 3: format ------------------------------------------------------------------------ */
static void *format_main(void *arg) {
    pipe_t *P = (pipe_t *)arg;
    int T0 = P->host_threads;
    for (int i = 0;; ++i) {
        slot_t *s = &P->slot[i % NSLOTS];
        if (!wait_state(P, s, S_DONE)) break;
        double t0 = now_s();
        size_t nr = s->nr;
        int T = T0;
        if ((size_t)T > nr / 4096 + 1) T = (int)(nr / 4096 + 1);
        int fail = 0;
        uint64_t good_total = 0;
#pragma omp parallel for num_threads(T) schedule(static, 1) reduction(+ : good_total) reduction(| : fail)
        for (int t = 0; t < T; ++t) {
            size_t a = nr * (size_t)t / (size_t)T, b = nr * (size_t)(t + 1) / (size_t)T, need = 64;
            for (size_t r = a; r < b; ++r) {
                const utree_result *q = &s->h_res[r];
                if (!q->found) continue;
                uint32_t ll = q->label < P->ctr->info.n_labels ? P->ctr->label_len[q->label] : 0;
                need += (size_t)s->name_len[r] + ll + 64;
            }
            if (need > s->fmt_cap[t]) { free(s->fmt_buf[t]); s->fmt_buf[t] = (char *)malloc(need + need / 4); s->fmt_cap[t] = s->fmt_buf[t] ? need + need / 4 : 0; }
            uint64_t good = 0;
            size_t L = !s->fmt_buf[t] ? (size_t)-1
                       : P->req->rank ? utree_format_rank_records(P->ctr, s->h_buf, s->name_off + a, s->name_len + a, s->h_res + a, b - a,
                                                             s->fmt_buf[t], s->fmt_cap[t], &good)
                                 : utree_format_records(P->ctr, s->h_buf, s->name_off + a, s->name_len + a, s->h_res + a, b - a,
                                                        s->fmt_buf[t], s->fmt_cap[t], &good);
            if (L == (size_t)-1) { fail |= 1; s->fmt_len[t] = 0; } else { s->fmt_len[t] = L; good_total += good; }
            if (P->keys) {
                /* the spool records of [a, b): one per query that prints a line, in the lines' order */
                size_t sneed = 0, sl = 0;
                for (size_t r = a; r < b; ++r) if (s->h_res[r].found) sneed += sizeof(utree_spool_rec) + s->name_len[r];
                if (sneed > s->sp_cap[t]) { free(s->sp_buf[t]); s->sp_buf[t] = (char *)malloc(sneed + sneed / 4); s->sp_cap[t] = s->sp_buf[t] ? sneed + sneed / 4 : 0; }
                if (sneed && !s->sp_buf[t]) fail |= 1;
                else for (size_t r = a; r < b; ++r) {
                    if (!s->h_res[r].found) continue;
                    const utree_spool_rec rec = {s->h_key[r], (uint32_t)(r / s->per), s->name_len[r]};
                    memcpy(s->sp_buf[t] + sl, &rec, sizeof rec); sl += sizeof rec;
                    memcpy(s->sp_buf[t] + sl, s->h_buf + s->name_off[r], s->name_len[r]); sl += s->name_len[r];
                }
                s->sp_len[t] = sl;
            }
            if (!P->hm) continue;
            /* the map's lines of [a, b): a line per query; the slice is cut where one device's shard ends and the next one's begins */
            size_t hneed = 64, hl = 0;
            for (size_t r = a; r < b; ++r) hneed += (size_t)s->name_len[r] + 48;
            for (int g = 0; g < P->n_dev; ++g) {
                const size_t f = s->hm_first[g], e = f + s->hm_count[g], x = a > f ? a : f, y = b < e ? b : e;
                if (x < y) hneed += 22 * (size_t)(s->h_run_off[y + (size_t)g] - s->h_run_off[x + (size_t)g]);        /* "4294967295:4294967295 " */
            }
            if (hneed > s->hm_cap[t]) { free(s->hm_buf[t]); s->hm_buf[t] = (char *)malloc(hneed + hneed / 4); s->hm_cap[t] = s->hm_buf[t] ? hneed + hneed / 4 : 0; }
            for (int g = 0; g < P->n_dev && s->hm_buf[t] && hl != (size_t)-1; ++g) {
                const size_t f = s->hm_first[g], e = f + s->hm_count[g], x = a > f ? a : f, y = b < e ? b : e;
                if (x >= y) continue;
                const size_t w = utree_hitmap_format(s->h_buf, s->name_off + x, s->name_len + x, s->h_run_off + x + (size_t)g, s->h_runs + s->hm_base[g], y - x,
                                                     s->hm_buf[t] + hl, s->hm_cap[t] - hl);
                hl = w == (size_t)-1 ? w : hl + w;
            }
            if (!s->hm_buf[t] || hl == (size_t)-1) { fail |= 1; s->hm_len[t] = 0; } else s->hm_len[t] = hl;
        }
        P->t_format += now_s() - t0;
        if (fail) { set_error(P, UTREE_E_NOMEM); break; }
        s->fmt_T = T; s->good = good_total;
        int last = s->last;
        set_state(P, s, S_FORMATTED);
        if (last || s->frame_rc == UTREE_E_FASTA) break;
    }
    return NULL;
}

/* ---- stage 4: write -------------------------------------------------------------------------- */
static void *writer_main(void *arg) {
    pipe_t *P = (pipe_t *)arg;
    uint64_t next_progress = 1048576 * (P->progress_printed + 1);
    for (int i = 0;; ++i) {
        slot_t *s = &P->slot[i % NSLOTS];
        if (!wait_state(P, s, S_FORMATTED)) break;
        double t1 = now_s();
        size_t nr = s->nr;
        /* pieces in input order; writes to one file serialise in the kernel anyway, so one thread issues them */
        for (int t = 0; t < s->fmt_T; ++t) {
            size_t done = 0;
            while (done < s->fmt_len[t]) {
                ssize_t w = write(P->fo, s->fmt_buf[t] + done, s->fmt_len[t] - done);
                if (w <= 0) { set_error(P, UTREE_E_IO); return NULL; }
                done += (size_t)w;
            }
            P->out_pos += (off_t)s->fmt_len[t];
        }
        for (int t = 0; t < s->fmt_T && P->hm && P->fh >= 0; ++t) {                /* the same chunk's map lines: both files hold the same queries */
            size_t done = 0;
            while (done < s->hm_len[t]) {
                ssize_t w = write(P->fh, s->hm_buf[t] + done, s->hm_len[t] - done);
                if (w <= 0) {                                                     /* the search goes on without its map */
                    snprintf(P->hm_msg, 512, "hit map %s: cannot write the file (%s)", P->req->hitmap_path, strerror(errno));
                    close(P->fh); P->fh = -1;
                    break;
                }
                done += (size_t)w;
            }
        }
        for (int t = 0; t < s->fmt_T && P->keys && P->fs >= 0; ++t) {              /* ... and its spool records */
            size_t done = 0;
            while (done < s->sp_len[t]) {
                ssize_t w = write(P->fs, s->sp_buf[t] + done, s->sp_len[t] - done);
                if (w <= 0) {                                                     /* the search goes on without that report */
                    snprintf(P->sp_msg, 512, "cannot write the spool %.300s.spool (%s)", P->req->redistribute_reads_path, strerror(errno));
                    close(P->fs); P->fs = -1;
                    break;
                }
                done += (size_t)w;
            }
        }
        P->t_write += now_s() - t1;
        P->st.good_finds += s->good;
        P->st.n_reads += nr;
        while (P->st.n_reads >= next_progress) {                                  /* itree.c:878 */
            printf("Searched %llu queries...\n", (unsigned long long)next_progress);
            next_progress += 1048576;
        }
        int last = s->last;
        if (s->frame_rc == UTREE_E_FASTA) {                                       /* reads before the bad one are written */
            P->st.fasta_error = s->ferr;
            if (!P->paired) P->st.fasta_error.read_index += P->st.n_reads - nr;   /* (a paired reader counts each file's records itself) */
            set_error(P, UTREE_E_FASTA);
            break;
        }
        if (s->frame_rc == UTREE_E_PAIRS) { set_error(P, UTREE_E_PAIRS); break; } /* ... and the complete pairs before a file ran out */
        set_state(P, s, S_EMPTY);
        if (last) break;
    }
    return NULL;
}

static void free_ctx(gpu_ctx *g) {
    if (!g->dev) return;
    hipSetDevice(g->dev->device);
    if (g->d_buf) hipFree(g->d_buf);
    if (g->d_off) hipFree(g->d_off);
    if (g->d_len) hipFree(g->d_len);
    if (g->d_out) hipFree(g->d_out);
    if (g->d_ws) hipFree(g->d_ws);
    if (g->d_buf2) hipFree(g->d_buf2);
    if (g->d_joined) hipFree(g->d_joined);
    if (g->d_off2) hipFree(g->d_off2);
    if (g->d_len2) hipFree(g->d_len2);
    if (g->d_joff) hipFree(g->d_joff);
    if (g->d_jlen) hipFree(g->d_jlen);
    if (g->d_meta) hipFree(g->d_meta);
    if (g->d_run_off) hipFree(g->d_run_off);
    if (g->d_runs) hipFree(g->d_runs);
    if (g->d_hm_meta) hipFree(g->d_hm_meta);
    if (g->d_hm_ws) hipFree(g->d_hm_ws);
    if (g->d_name_off) hipFree(g->d_name_off);
    if (g->d_name_len) hipFree(g->d_name_len);
    if (g->d_key) hipFree(g->d_key);
    if (g->stream) hipStreamDestroy(g->stream);
}

/* device g's buffers for the slots' shards: the worst case of a shard is the slot's reads and bytes */
static int ctx_alloc(pipe_t *P, gpu_ctx *c, utree_dev *dev) {
    const utree_search_request *req = P->req;
    const int paired = P->paired;
    c->dev = dev;
    HIPE(hipSetDevice(dev->device));
    HIPE(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIPE(hipMalloc((void **)&c->d_buf, P->chunk + 64));
    HIPE(hipMalloc((void **)&c->d_off, MAX_READS_PER_BATCH * 8));
    HIPE(hipMalloc((void **)&c->d_len, MAX_READS_PER_BATCH * 4));
    HIPE(hipMalloc((void **)&c->d_out, MAX_READS_PER_BATCH * sizeof(utree_result)));
    if (paired) {                                                             /* the second mates, and the joined batch: both buffers' bytes + an 'N' per pair */
        c->joined_cap = (paired == PAIRS_TWO_FILES ? 2 : 1) * P->chunk + MAX_READS_PER_BATCH;
        if (paired == PAIRS_TWO_FILES) HIPE(hipMalloc((void **)&c->d_buf2, P->chunk + 64));
        HIPE(hipMalloc((void **)&c->d_joined, c->joined_cap + 64));
        HIPE(hipMalloc((void **)&c->d_off2, MAX_READS_PER_BATCH * 8));
        HIPE(hipMalloc((void **)&c->d_len2, MAX_READS_PER_BATCH * 4));
        HIPE(hipMalloc((void **)&c->d_joff, MAX_READS_PER_BATCH * 8));
        HIPE(hipMalloc((void **)&c->d_jlen, MAX_READS_PER_BATCH * 4));
        HIPE(hipMalloc((void **)&c->d_meta, sizeof(utree_pairs_meta)));
    }
    if (P->hm) {                                                              /* a run per window */
        const uint64_t tb = paired ? c->joined_cap : P->chunk;
        c->runs_cap = utk_hitmap_wcap((uint32_t)MAX_READS_PER_BATCH, tb, req->do_rc);
        c->hm_ws_bytes = utree_hitmap_workspace_bytes(dev, (uint32_t)MAX_READS_PER_BATCH, tb, req->do_rc);
        if (!c->hm_ws_bytes) return UTREE_E_ARG;
        HIPE(hipMalloc((void **)&c->d_run_off, (MAX_READS_PER_BATCH + 1) * 8));
        HIPE(hipMalloc((void **)&c->d_runs, (size_t)(c->runs_cap + 1) * sizeof(utree_hit_run)));
        HIPE(hipMalloc((void **)&c->d_hm_meta, sizeof(utree_hitmap_meta)));
        HIPE(hipMalloc(&c->d_hm_ws, c->hm_ws_bytes));
    }
    if (P->names) {
        HIPE(hipMalloc((void **)&c->d_name_off, MAX_READS_PER_BATCH * 4));
        HIPE(hipMalloc((void **)&c->d_name_len, MAX_READS_PER_BATCH * 4));
    }
    if (P->keys) HIPE(hipMalloc((void **)&c->d_key, MAX_READS_PER_BATCH * 4));
    c->ws_bytes = req->rank ? utree_rank_workspace_bytes(dev, (uint32_t)MAX_READS_PER_BATCH, CHUNK_BYTES, LINELEN_MAX, req->do_rc, req->rank)
                            : utree_classify_workspace_bytes(dev, (uint32_t)MAX_READS_PER_BATCH, paired ? c->joined_cap : CHUNK_BYTES, LINELEN_MAX, req->do_rc);
    if (!c->ws_bytes) return UTREE_E_ARG;
    HIPE(hipMalloc(&c->d_ws, c->ws_bytes));
    return UTREE_OK;
}

/* <hitmap_path>.labels: line i (0-based) is the text of label index i, what a hit's code in the map names */
static int write_labels(const utree_ctr *ctr, const char *hitmap_path, char *msg) {
    char name[4096];
    if (snprintf(name, sizeof name, "%s.labels", hitmap_path) >= (int)sizeof name) { snprintf(msg, 512, "hit map %s: the path is too long", hitmap_path); return 1; }
    FILE *f = fopen(name, "wb");
    int bad = !f;
    for (uint32_t i = 0; f && !bad && i < ctr->info.n_labels; ++i)
        bad = fwrite(ctr->labels[i], 1, ctr->label_len[i], f) != ctr->label_len[i] || fputc('\n', f) == EOF;
    if (f && fclose(f)) bad = 1;
    if (bad) snprintf(msg, 512, "hit map %.400s.labels: cannot write the file (%s)", hitmap_path, strerror(errno));
    return bad;
}

/* the spool of a search that writes each read's redistributed label: <redistribute_reads_path>.spool, created when the search starts and removed
 * on every way out (search_request); fd -1 and msg: it could not be created, or written */
typedef struct { int fd; char path[4096], msg[512]; } spool_t;

/* One search that utree_search_run has checked; rep: the reports it feeds (NULL: none); hm_msg: why the hit map was not written, when it was not;
 * sp: NULL, or the spool the queries' keys go to (closed here) */
static int search_file(const utree_ctr *ctr, utree_dev **devs, int n_dev, const utree_search_request *req, utree_reports *rep, char *hm_msg,
                       spool_t *sp, utree_search_stats *stats) {
    const int paired = req->mates_path ? PAIRS_TWO_FILES : req->interleaved ? PAIRS_INTERLEAVED : PAIRS_NONE;   /* (GG search only) */
    const char *hitmap_path = req->hitmap_path, *out_path = req->out_path;
    int rc = UTREE_OK;
    uint64_t dev_printed = 0;
    utree_search_resume resume;
    memset(&resume, 0, sizeof resume); resume.fo = -1;
    /* The GG search on the reference's input format takes the device text pipeline (search_dev.c); it hands back input it
     * does not take -- malformed records, NUL bytes, lines fgets would split -- and the host framing below then reproduces
     * the reference on it case by case.  UTREE_HOST_TEXT=1 forces the host pipeline (tests, A/B). */
    if (!req->rank && !paired && !hitmap_path && !req->redistribute_reads_path && req->input_format == UTREE_INPUT_REFERENCE && !getenv("UTREE_HOST_TEXT")) {
        rc = utree_search_file_device(ctr, devs, n_dev, req->reads_path, out_path, req->do_rc, req->host_threads, rep, stats, &dev_printed, &resume);
        if (rc != UTREE_RETRY_HOST) return rc;
        rc = UTREE_OK;
        /* the reports carry the chunks the device pipeline has written when this pipeline continues behind them (resume.fo >= 0), as the
         * counts do; when it starts the file over, so do the reports */
        if (resume.fo < 0 && (rc = utree_reports_reset(rep))) return rc;
    }
    double t_start = now_s();
    pipe_t *P = (pipe_t *)calloc(1, sizeof *P);
    if (!P) { if (resume.fo >= 0) close(resume.fo); if (sp && sp->fd >= 0) { close(sp->fd); sp->fd = -1; } return UTREE_E_NOMEM; }
    P->ctr = ctr; P->req = req; P->rep = rep; P->n_dev = n_dev; P->input_format = req->input_format;
    P->progress_printed = dev_printed;
    P->paired = paired; P->chunk = paired || hitmap_path || req->redistribute_reads_path ? utree_chunk_bytes(CHUNK_BYTES) : CHUNK_BYTES;
    P->fs = sp ? sp->fd : -1; P->keys = P->fs >= 0 && utree_reports_wants_keys(rep); P->sp_msg = sp ? sp->msg : NULL;
    if (sp) sp->fd = -1;                                                          /* (this search's to close from here on) */
    P->names = utree_reports_wants_names(rep);
    P->hm = hitmap_path != NULL; P->fh = -1; P->hm_msg = hm_msg;
    P->in[1].fd = -1;
    P->in[0].fd = open(req->reads_path, O_RDONLY);
    if (paired == PAIRS_TWO_FILES && P->in[0].fd >= 0 && (P->in[1].fd = open(req->mates_path, O_RDONLY)) < 0) { close(P->in[0].fd); P->in[0].fd = -1; }
    if (resume.fo >= 0) {
        /* the output is a pipe and the device pipeline has written the chunks in front of `in_off`: go on from there, on the same descriptor */
        P->fo = resume.fo; P->in[0].pos = (off_t)resume.in_off;
        P->st.n_reads = resume.n_reads; P->st.good_finds = resume.good_finds; P->st.bytes_in = resume.bytes_in; P->st.bytes_out = resume.bytes_out;
    } else if (utree_output_parts() > 1) {
        /* UTREE_OUTPUT_PARTS: this pipeline writes in input order with one writer, so all of the output is part 000 and the other parts are
         * empty files -- the parts' concatenation is the output, as with the device pipeline's side-by-side parts */
        char name[4096];
        for (int p = utree_output_parts() - 1; p >= 0; --p) {
            snprintf(name, sizeof name, "%s.part%03d", out_path, p);
            const int f = open(name, O_WRONLY | O_CREAT | O_TRUNC, 0644);
            if (p == 0) P->fo = f; else if (f >= 0) close(f); else { P->fo = -1; break; }
        }
    } else
    P->fo = open(out_path, O_WRONLY | O_CREAT | O_TRUNC, 0644);                   /* fopen(outfile, "wb"), itree.c:834 */
    if (P->in[0].fd < 0 || P->fo < 0) {                                           /* itree.c:835 */
        if (P->in[0].fd >= 0) close(P->in[0].fd);
        if (P->in[1].fd >= 0) close(P->in[1].fd);
        if (P->fo >= 0) close(P->fo);
        if (P->fs >= 0) close(P->fs);
        free(P);
        return UTREE_E_IO;
    }
    if (P->hm) {
        /* a map that cannot be opened, or whose labels cannot be written, does not stop the search: it runs without one and says so at its end */
        P->fh = open(hitmap_path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (P->fh < 0) snprintf(hm_msg, 512, "hit map %s: cannot open the file (%s)", hitmap_path, strerror(errno));
        else if (write_labels(ctr, hitmap_path, hm_msg)) { close(P->fh); P->fh = -1; }
        if (P->fh < 0) P->hm = 0;
    }
    for (int k = 0; k < 2 && req->input_format != UTREE_INPUT_REFERENCE; ++k) {
        if (P->in[k].fd < 0) continue;
        P->in[k].gz = gzdopen(dup(P->in[k].fd), "rb");
        if (!P->in[k].gz) {
            if (P->in[0].gz) gzclose(P->in[0].gz);
            close(P->in[0].fd); if (P->in[1].fd >= 0) close(P->in[1].fd);
            if (P->fh >= 0) close(P->fh);
            if (P->fs >= 0) close(P->fs);
            close(P->fo); free(P);
            return UTREE_E_IO;
        }
        gzbuffer(P->in[k].gz, 1u << 20);
    }
    int host_threads = req->host_threads;
#ifdef _OPENMP
    if (host_threads <= 0) host_threads = omp_get_max_threads();
#else
    host_threads = 1;
#endif
    if (host_threads > 16) host_threads = 16;                                     /* formatting saturates well before that */
    P->host_threads = host_threads;
    pthread_mutex_init(&P->mu, NULL);
    pthread_cond_init(&P->cv, NULL);
    for (uint32_t i = 0; i < ctr->info.n_labels; ++i) if (ctr->label_len[i] > P->max_label) P->max_label = ctr->label_len[i];
    P->G = (gpu_ctx *)calloc((size_t)n_dev, sizeof(gpu_ctx));
    if (!P->G) { rc = UTREE_E_NOMEM; goto done; }
    for (int g = 0; g < n_dev; ++g) if ((rc = ctx_alloc(P, &P->G[g], devs[g]))) goto done;
    {
        pthread_t tr, tg, tf, tw;
        pthread_create(&tr, NULL, paired ? reader_pairs_main : reader_main, P);
        pthread_create(&tg, NULL, gpu_main, P);
        pthread_create(&tf, NULL, format_main, P);
        pthread_create(&tw, NULL, writer_main, P);
        pthread_join(tw, NULL);
        /* the writer ends last on success; on error make sure the others leave their waits */
        pthread_mutex_lock(&P->mu); P->stop = 1; pthread_cond_broadcast(&P->cv); pthread_mutex_unlock(&P->mu);
        pthread_join(tr, NULL);
        pthread_join(tg, NULL);
        pthread_join(tf, NULL);
        rc = P->rc;
        if (rc == UTREE_E_PAIRS) utree_set_error_text(P->msg_pairs);               /* (the text is per thread, and this is the caller's) */
        else if (rc == UTREE_E_DEVICE && P->msg_join[0]) utree_set_error_text(P->msg_join);
    }
done:
    for (int k = 0; k < 2; ++k) {
        if (P->in[k].gz) gzclose(P->in[k].gz);
        if (P->in[k].fd >= 0) close(P->in[k].fd);
    }
    if (P->fo >= 0) close(P->fo);
    if (P->fh >= 0 && close(P->fh) && !hm_msg[0]) snprintf(hm_msg, 512, "hit map %s: cannot write the file (%s)", hitmap_path, strerror(errno));
    if (P->fs >= 0 && close(P->fs) && !sp->msg[0]) snprintf(sp->msg, sizeof sp->msg, "cannot write the spool %.300s (%s)", sp->path, strerror(errno));
    if (P->G) { for (int g = 0; g < n_dev; ++g) free_ctx(&P->G[g]); free(P->G); }
    for (int i = 0; i < NSLOTS; ++i) slot_free(&P->slot[i]);
    P->st.seconds_total = now_s() - t_start;
    P->st.seconds_kernels = P->t_gpu;
    P->st.pipeline = 0; P->st.n_lanes = 1;
    P->st.seconds_read = P->t_read; P->st.seconds_frame = P->t_frame; P->st.seconds_classify_format = P->t_gpu;
    P->st.seconds_d2h = P->t_format; P->st.seconds_write = P->t_write;
    if (timing_on())
        fprintf(stderr, "[utree_amd] stages: read %.3f s, frame %.3f s | gpu %.3f s | format %.3f s, write %.3f s (overlapped)\n",
                P->t_read, P->t_frame, P->t_gpu, P->t_format, P->t_write);
    if (stats) *stats = P->st;
    pthread_mutex_destroy(&P->mu);
    pthread_cond_destroy(&P->cv);
    free(P);
    return rc;
}

int utree_pairs_join(utree_dev *dev, const uint8_t *d_bases1, const uint64_t *d_off1, const uint32_t *d_len1, const uint8_t *d_bases2,
                     const uint64_t *d_off2, const uint32_t *d_len2, uint32_t n_pairs, uint8_t *d_joined, uint64_t joined_capacity,
                     uint64_t *d_joff, uint32_t *d_jlen, utree_pairs_meta *d_meta, void *stream) {
    if (!dev || !d_meta) return UTREE_E_ARG;
    if (n_pairs && (!d_bases1 || !d_off1 || !d_len1 || !d_bases2 || !d_off2 || !d_len2 || !d_joff || !d_jlen || (!d_joined && joined_capacity)))
        return UTREE_E_ARG;
    hipError_t e = hipMemsetAsync(d_meta, 0, sizeof *d_meta, (hipStream_t)stream);
    if (e == hipSuccess && n_pairs)
        e = (hipError_t)utk_pairs_join(d_bases1, d_off1, d_len1, d_bases2, d_off2, d_len2, n_pairs, d_joined, joined_capacity, d_joff, d_jlen,
                                       d_meta, stream);
    if (e != hipSuccess) { utree_dev_set_hip_error((int)e, "utree_pairs_join"); return UTREE_E_HIP; }
    return UTREE_OK;
}

/* One checked request: its reports are fed while searching and written when the search has succeeded (the search's own codes stay its own) */
static int search_request(const utree_ctr *ctr, utree_dev **devs, int n_dev, const utree_search_request *req, utree_search_stats *stats) {
    utree_reports *rep = NULL;
    utree_search_stats st;
    char hm_msg[512] = "";                                         /* why the hit map was not written, when it was not */
    spool_t *sp = NULL;
    memset(&st, 0, sizeof st);
    int rc = utree_reports_create(ctr, devs, n_dev, req, &rep);
    if (!rc && !rep && !req->hitmap_path) return search_file(ctr, devs, n_dev, req, NULL, hm_msg, NULL, stats);   /* no report asked for */
    if (!rc && utree_reports_wants_keys(rep)) {
        /* a spool that cannot be created does not stop the search: it runs without the report and says so at its end */
        if (!(sp = (spool_t *)calloc(1, sizeof *sp))) rc = UTREE_E_NOMEM;
        else if (snprintf(sp->path, sizeof sp->path, "%s.spool", req->redistribute_reads_path) >= (int)sizeof sp->path) {
            sp->fd = -1; sp->path[0] = 0; snprintf(sp->msg, sizeof sp->msg, "the path is too long for its spool");
        } else if ((sp->fd = open(sp->path, O_WRONLY | O_CREAT | O_TRUNC, 0644)) < 0)
            snprintf(sp->msg, sizeof sp->msg, "cannot create the spool %.300s (%s)", sp->path, strerror(errno));
    }
    if (!rc) rc = search_file(ctr, devs, n_dev, req, rep, hm_msg, sp, &st);
    if (sp && sp->fd >= 0) { close(sp->fd); sp->fd = -1; }         /* (a search that ended before it took the spool over) */
    if (!rc && rep) rc = utree_reports_write(rep, ctr, st.n_reads, sp && !sp->msg[0] ? sp->path : NULL, sp ? sp->msg : NULL);
    if (!rc && hm_msg[0]) { utree_set_error_text(hm_msg); rc = UTREE_E_HITMAP; }
    if (sp && sp->path[0]) unlink(sp->path);                       /* on every way out */
    free(sp);
    utree_reports_free(rep);
    if (stats) *stats = st;
    return rc;
}

/* The one place that checks a request, every check in front of the first look at `ctr` or a device handle.  rank: XT_doSearch32(utree, in, out, 0,
 * speed, doRC) (itree.c:1376 without DO_GG): the same pipeline, the batches to ONE device in file order because each read's vote depends on the
 * reads before it (rank.c) -- another vote: no candidate sets; a hit-dependent subset of windows: no map, and no coverage of the GG search's */
int utree_search_run(const utree_ctr *ctr, utree_dev **devs, int n_dev, const utree_search_request *req, utree_search_stats *stats) {
    /* a caller built before redistribute_reads_path gives the size of the layout without it: a request without that report */
    const size_t al = _Alignof(utree_search_request), old_size = (offsetof(utree_search_request, redistribute_reads_path) + al - 1) / al * al;
    utree_search_request grown;
    if (req && req->size == old_size && old_size < sizeof grown) {
        memset(&grown, 0, sizeof grown);
        memcpy(&grown, req, old_size);
        grown.size = sizeof grown;
        req = &grown;
    }
    if (!req || req->size != sizeof *req) return UTREE_E_ARG;
    if (!ctr || !devs || n_dev < 1 || !req->reads_path || !req->out_path) return UTREE_E_ARG;
    if (req->input_format < 0 || req->input_format > UTREE_INPUT_AUTO || (req->mates_path && req->interleaved)) return UTREE_E_ARG;
    const int d = req->sample_delim;
    if ((req->samples_path || req->sample_redistribute_path) && (d < 0 || d > 255 || d == '\t' || d == ' ' || d == '\r' || d == '\n')) return UTREE_E_ARG;
    if ((req->redistribute_path || req->sample_redistribute_path || req->redistribute_reads_path) && req->max_passes > 1000) return UTREE_E_ARG;
    if (req->rank) {
        if (n_dev != 1 || req->mates_path || req->interleaved || req->coverage_path || req->redistribute_path || req->hitmap_path ||
            req->sample_redistribute_path || req->redistribute_reads_path) return UTREE_E_ARG;
        const int rc = utree_rank_reset(devs[0]);
        if (rc) return rc;
    }
    return search_request(ctr, devs, n_dev, req, stats);
}

/* ---- the fixed-argument forms of utree_search_run (include/utree_amd.h) ------------------------------------------------------------------ */
#define REQ(...) const utree_search_request r = {.size = sizeof r, .reads_path = reads_path, .out_path = out_path, .do_rc = do_rc, .host_threads = host_threads, __VA_ARGS__}
#define REPORTS4 .input_format = input_format, .mates_path = mates_path, .interleaved = interleaved, .profile_path = profile_path, \
                 .coverage_path = coverage_path, .redistribute_path = redistribute_path, .max_passes = max_passes

int utree_search_file(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path, const char *out_path,
                      int do_rc, int host_threads, utree_search_stats *stats) {
    REQ(.input_format = UTREE_INPUT_REFERENCE);
    return utree_search_run(ctr, devs, n_dev, &r, stats);
}
int utree_search_file_opts(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path, const char *out_path,
                           int do_rc, int host_threads, int input_format, utree_search_stats *stats) {
    REQ(.input_format = input_format);
    return utree_search_run(ctr, devs, n_dev, &r, stats);
}
int utree_search_file_profile(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path, const char *out_path, int do_rc,
                              int host_threads, int input_format, const char *profile_path, utree_search_stats *stats) {
    REQ(.input_format = input_format, .profile_path = profile_path);
    return utree_search_run(ctr, devs, n_dev, &r, stats);
}
int utree_search_file_coverage(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path, const char *out_path, int do_rc,
                               int host_threads, int input_format, const char *profile_path, const char *coverage_path,
                               utree_search_stats *stats) {
    REQ(.input_format = input_format, .profile_path = profile_path, .coverage_path = coverage_path);
    return utree_search_run(ctr, devs, n_dev, &r, stats);
}
int utree_search_pairs_file(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path, const char *mates_path, const char *out_path,
                            int do_rc, int host_threads, int input_format, const char *profile_path, const char *coverage_path,
                            utree_search_stats *stats) {
    REQ(.input_format = input_format, .mates_path = mates_path, .interleaved = !mates_path, .profile_path = profile_path, .coverage_path = coverage_path);
    return utree_search_run(ctr, devs, n_dev, &r, stats);
}
int utree_search_file_redistribute(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path, const char *mates_path,
                                   int interleaved, const char *out_path, int do_rc, int host_threads, int input_format,
                                   const char *profile_path, const char *coverage_path, const char *redistribute_path, uint32_t max_passes,
                                   utree_search_stats *stats) {
    REQ(REPORTS4);
    return utree_search_run(ctr, devs, n_dev, &r, stats);
}
int utree_search_file_hitmap(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path, const char *mates_path, int interleaved,
                             const char *out_path, int do_rc, int host_threads, int input_format, const char *profile_path,
                             const char *coverage_path, const char *redistribute_path, uint32_t max_passes, const char *hitmap_path,
                             utree_search_stats *stats) {
    REQ(REPORTS4, .hitmap_path = hitmap_path);
    return utree_search_run(ctr, devs, n_dev, &r, stats);
}
int utree_search_file_samples(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path, const char *mates_path, int interleaved,
                              const char *out_path, int do_rc, int host_threads, int input_format, const char *profile_path,
                              const char *coverage_path, const char *redistribute_path, uint32_t max_passes, const char *hitmap_path,
                              const char *samples_path, int delim, utree_search_stats *stats) {
    REQ(REPORTS4, .hitmap_path = hitmap_path, .samples_path = samples_path, .sample_delim = delim);
    return utree_search_run(ctr, devs, n_dev, &r, stats);
}
int utree_search_file_sample_redistribute(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path, const char *mates_path,
                                          int interleaved, const char *out_path, int do_rc, int host_threads, int input_format,
                                          const char *profile_path, const char *coverage_path, const char *redistribute_path, uint32_t max_passes,
                                          const char *hitmap_path, const char *samples_path, int delim, const char *sample_redistribute_path,
                                          utree_search_stats *stats) {
    REQ(REPORTS4, .hitmap_path = hitmap_path, .samples_path = samples_path, .sample_delim = delim, .sample_redistribute_path = sample_redistribute_path);
    return utree_search_run(ctr, devs, n_dev, &r, stats);
}

/* the rank-specific search: one handle; without params there is nothing to run */
int utree_rank_search_file_samples(const utree_ctr *ctr, utree_dev *dev, const char *reads_path, const char *out_path, int do_rc,
                                   const utree_rank_params *params, int host_threads, int input_format, const char *profile_path,
                                   const char *samples_path, int delim, utree_search_stats *stats) {
    if (!dev || !params) return UTREE_E_ARG;
    REQ(.input_format = input_format, .rank = params, .profile_path = profile_path, .samples_path = samples_path, .sample_delim = delim);
    return utree_search_run(ctr, &dev, 1, &r, stats);
}
int utree_rank_search_file_profile(const utree_ctr *ctr, utree_dev *dev, const char *reads_path, const char *out_path, int do_rc,
                                   const utree_rank_params *params, int host_threads, int input_format, const char *profile_path,
                                   utree_search_stats *stats) {
    return utree_rank_search_file_samples(ctr, dev, reads_path, out_path, do_rc, params, host_threads, input_format, profile_path, NULL, 0, stats);
}
int utree_rank_search_file_opts(const utree_ctr *ctr, utree_dev *dev, const char *reads_path, const char *out_path, int do_rc,
                                const utree_rank_params *params, int host_threads, int input_format, utree_search_stats *stats) {
    return utree_rank_search_file_samples(ctr, dev, reads_path, out_path, do_rc, params, host_threads, input_format, NULL, NULL, 0, stats);
}
int utree_rank_search_file(const utree_ctr *ctr, utree_dev *dev, const char *reads_path, const char *out_path, int do_rc,
                           const utree_rank_params *params, int host_threads, utree_search_stats *stats) {
    return utree_rank_search_file_samples(ctr, dev, reads_path, out_path, do_rc, params, host_threads, UTREE_INPUT_REFERENCE, NULL, NULL, 0, stats);
}
