/* search.c -- whole-file search: XT_doSearch32's GG branch (itree.c:833-1108) over one or more device
 * images.  Host orchestration in C, four overlapped stages connected by a ring of chunk slots:
 *
 *   reader   : the next ~96 MiB of FASTA into the slot's pinned memory, framed (search_reader.c: one step per slot; here only its thread)
 *   gpu      : shard the framed reads contiguously over the GPUs; per GPU copy the shard's byte span to HBM
 *              as it stands, run the batch kernels, copy the 24-byte results back
 *   formatter: format the lines with a thread team
 *   writer   : write them in input order (= what the reference writes with one thread; with more threads it
 *              writes a permutation)
 *
 * This file holds the ring, the slots' and devices' buffers -- the optional ones grouped by the feature that asks for them --, stages 2 to 4,
 * and the search of one checked request (utree_search_checked; the request check and the ABI forms are search_entry.c's).
 *
 * Paired-end input (a request's mates_path / interleaved): the reader commits the pairs both of a slot's buffers hold, the gpu stage uploads both
 * mates' bytes and joins them on the device (pairs_kernels.hip) in front of the batch kernels; formatter and writer see one query per pair,
 * named by mate 1.
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
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#ifdef _OPENMP
#include <omp.h>
#endif
#include "ctr_host.h"
#include "dev_image.h"
#include "search_dev.h"
#include "search_reader.h"
#include "reports.h"
#include "hitmap.h"

#define CHUNK_BYTES ((size_t)96 << 20)        /* must hold two maximal (16 MiB) lines                    */
#define MAX_READS_PER_BATCH ((size_t)2 << 20)  /* more reads in a chunk (tiny reads) simply take another batch */
#define NSLOTS 4

enum { S_EMPTY = 0, S_FRAMED, S_DONE, S_FORMATTED };
#define FMT_MAX_THREADS 16

/* what a slot's formatting makes for one file: one growable piece per formatting thread, in input order */
typedef struct { char *buf[FMT_MAX_THREADS]; size_t cap[FMT_MAX_THREADS], len[FMT_MAX_THREADS]; } pieces_t;

/* piece t with room for `need` bytes (its contents are not kept); NULL: no memory */
static char *piece_reserve(pieces_t *p, int t, size_t need) {
    if (need > p->cap[t]) { free(p->buf[t]); p->buf[t] = (char *)malloc(need + need / 4); p->cap[t] = p->buf[t] ? need + need / 4 : 0; }
    return p->buf[t];
}
/* the first T pieces to fd, in order; the bytes written, or -1 (errno: write's) */
static ssize_t pieces_write(int fd, const pieces_t *p, int T) {
    size_t total = 0;
    for (int t = 0; t < T; ++t) {
        size_t done = 0;
        while (done < p->len[t]) {
            ssize_t w = write(fd, p->buf[t] + done, p->len[t] - done);
            if (w <= 0) return -1;
            done += (size_t)w;
        }
        total += done;
    }
    return (ssize_t)total;
}
static void pieces_free(pieces_t *p) { for (int t = 0; t < FMT_MAX_THREADS; ++t) free(p->buf[t]); }

typedef struct {
    frames_t rd;                               /* the reads; rd.buf (pinned): the chunk as read from the file */
    size_t nr;                                 /* framed reads (pairs)                                      */
    utree_result *h_res;                       /* pinned                                                    */
    int frame_rc, last;
    utree_fasta_error ferr;
    int state;
    pieces_t out;                              /* formatted lines                                           */
    int fmt_T;
    uint64_t good;
    struct {                                   /* paired input only                                         */
        frames_t m2;                           /* the second mates of the slot's pairs -- a buffer of their own (two files) or spans of rd.buf (interleaved) */
        utree_pairs_meta *h_meta;              /* pinned, one per device: what the join reported            */
    } pr;
    /* hit map only: per device its shard [first, + count) of the slot, the shard's run offsets (count + 1 of them at h_run_off +
     * first + g, relative to the shard's first run) and its runs at h_runs + base */
    struct {
        utree_hitmap_meta *h_meta;             /* pinned, one per device                                    */
        uint64_t *h_run_off;                   /* pinned, MAX_READS_PER_BATCH + n_dev                       */
        utree_hit_run *h_runs; size_t runs_cap; /* pinned, grows geometrically                              */
        size_t *first, *count; uint64_t *base;
        pieces_t lines;                        /* the map's lines                                           */
    } hm;
    /* a report that reads the names only: the names' offsets relative to their shard's uploaded span, and their lengths behind them */
    struct { uint32_t *h_rel; } nm;            /* pinned, 2 * MAX_READS_PER_BATCH                           */
    /* redistributed reads only: every read's key (of the table of the device handle that classified it: read r went to handle r / per), and
     * the spool records of the queries that print a line */
    struct { uint32_t *h_key; size_t per; pieces_t recs; } ky;   /* h_key: pinned, MAX_READS_PER_BATCH       */
} slot_t;

typedef struct {
    utree_dev *dev;
    hipStream_t stream;
    uint8_t *d_buf; uint64_t *d_off; uint32_t *d_len; utree_result *d_out; void *d_ws; size_t ws_bytes;
    struct {                                    /* paired input: the second mates as uploaded, and the joined batch the kernels see */
        uint8_t *d_buf2, *d_joined; uint64_t *d_off2, *d_joff; uint32_t *d_len2, *d_jlen; utree_pairs_meta *d_meta; size_t joined_cap;
        uint64_t want_total;                    /* joined bytes of the shard in flight, as the host counted them */
    } pr;
    /* hit map: the shard's run offsets, runs (the worst case: one per window) and meta, and the call's workspace */
    struct { uint64_t *d_run_off; utree_hit_run *d_runs; uint64_t runs_cap; utree_hitmap_meta *d_meta; void *d_ws; size_t ws_bytes; } hm;
    struct { uint32_t *d_off, *d_len; } nm;     /* a report that reads the names only: relative to d_buf      */
    struct { uint32_t *d_key; } ky;             /* redistributed reads only: the shard's keys                 */
} gpu_ctx;

typedef struct {
    const utree_ctr *ctr;
    const utree_search_request *req;            /* what is searched: the paths, do_rc, rank (non-NULL: the rank-specific `xtree-search`, rank.c, one device) */
    utree_reports *rep;                         /* non-NULL: the search feeds reports (reports.h)            */
    gpu_ctx *G; int n_dev;
    reader_t rd;                                /* stage 1's state: the input(s), the format, the carries    */
    int fo;                                     /* output                                                   */
    int names;                                  /* a report reads the names (utree_reports_wants_names): they go up with the shard */
    int hm, fh;                                 /* a hit map is made; its file (-1 once writing it has failed: the search goes on) */
    char *hm_msg;                               /* why the map could not be written ("" = it could): the writer's to set            */
    int keys, fs;                               /* every read's key is brought back and spooled; the spool (-1 once writing it has failed: the search goes on) */
    char *sp_msg;                               /* why the spool could not be written ("" = it could): the writer's to set          */
    int paired;                                 /* PAIRS_*, from the request's mates_path / interleaved     */
    size_t chunk;                               /* bytes per slot and input: CHUNK_BYTES; a paired search honours UTREE_CHUNK_BYTES */
    /* what utree_last_hip_error is to say: each text has ONE writer -- the reader stage (UTREE_E_PAIRS) and the gpu stage (a join the
     * device refused) --, and the caller's thread reads the one that belongs to the search's code once the stages have ended */
    char msg_pairs[512], msg_join[256];
    int host_threads;                           /* the request's, resolved                                   */
    slot_t slot[NSLOTS];
    pthread_mutex_t mu; pthread_cond_t cv;
    int rc;                                     /* first error of any stage                                  */
    int stop;
    utree_search_stats st;
    double t_read, t_frame, t_gpu, t_format, t_write;
    uint64_t progress_printed;                  /* progress lines the device pipeline printed before it handed the file back */
} pipe_t;

/* ---- the slots' buffers: the reads' and the results', and per feature what it adds ---------------------------------------------- */
static int pin(void *pp, size_t bytes) { return hipHostMalloc((void **)pp, bytes, hipHostMallocDefault) == hipSuccess ? UTREE_OK : UTREE_E_NOMEM; }
static void unpin(void *p) { if (p) hipHostFree(p); }

/* what goes up to the device as it stands is pinned; buf_bytes 0: no buffer of its own */
static int frames_alloc(frames_t *f, size_t buf_bytes) {
    if ((buf_bytes && pin(&f->buf, buf_bytes)) || pin(&f->rel_off, MAX_READS_PER_BATCH * 8) || pin(&f->seq_len, MAX_READS_PER_BATCH * 4)) return UTREE_E_NOMEM;
    f->seq_off = (uint64_t *)malloc(MAX_READS_PER_BATCH * 8); f->name_off = (uint64_t *)malloc(MAX_READS_PER_BATCH * 8);
    f->name_len = (uint32_t *)malloc(MAX_READS_PER_BATCH * 4);
    return (f->seq_off && f->name_off && f->name_len) ? UTREE_OK : UTREE_E_NOMEM;
}
static void frames_free(frames_t *f) { unpin(f->buf); unpin(f->rel_off); unpin(f->seq_len); free(f->seq_off); free(f->name_off); free(f->name_len); }

static int slot_pairs_alloc(slot_t *s, const pipe_t *P) {
    if (pin(&s->pr.h_meta, (size_t)P->n_dev * sizeof(utree_pairs_meta))) return UTREE_E_NOMEM;
    return frames_alloc(&s->pr.m2, P->paired == PAIRS_TWO_FILES ? P->chunk + 64 : 0);
}
static void slot_pairs_free(slot_t *s) { unpin(s->pr.h_meta); frames_free(&s->pr.m2); }

static int slot_hm_alloc(slot_t *s, const pipe_t *P) {
    const size_t n = (size_t)P->n_dev;
    if (pin(&s->hm.h_meta, n * sizeof(utree_hitmap_meta)) || pin(&s->hm.h_run_off, (MAX_READS_PER_BATCH + n) * 8)) return UTREE_E_NOMEM;
    s->hm.first = (size_t *)calloc(n, sizeof(size_t)); s->hm.count = (size_t *)calloc(n, sizeof(size_t)); s->hm.base = (uint64_t *)calloc(n, 8);
    return (s->hm.first && s->hm.count && s->hm.base) ? UTREE_OK : UTREE_E_NOMEM;
}
static void slot_hm_free(slot_t *s) {
    unpin(s->hm.h_meta); unpin(s->hm.h_run_off); unpin(s->hm.h_runs);
    free(s->hm.first); free(s->hm.count); free(s->hm.base);
    pieces_free(&s->hm.lines);
}

static int slot_names_alloc(slot_t *s) { return pin(&s->nm.h_rel, 2 * MAX_READS_PER_BATCH * 4); }
static void slot_names_free(slot_t *s) { unpin(s->nm.h_rel); }

static int slot_keys_alloc(slot_t *s) { return pin(&s->ky.h_key, MAX_READS_PER_BATCH * 4); }
static void slot_keys_free(slot_t *s) { unpin(s->ky.h_key); pieces_free(&s->ky.recs); }

static int slot_alloc(slot_t *s, const pipe_t *P) {
    if (s->rd.buf) return UTREE_OK;
    int rc = UTREE_OK;
    if (!rc && P->keys) rc = slot_keys_alloc(s);
    if (!rc && P->names) rc = slot_names_alloc(s);
    if (!rc && P->hm) rc = slot_hm_alloc(s, P);
    if (!rc && P->paired) rc = slot_pairs_alloc(s, P);
    if (!rc) rc = pin(&s->h_res, MAX_READS_PER_BATCH * sizeof(utree_result));
    if (!rc) rc = frames_alloc(&s->rd, P->chunk + 64);
    return rc;
}

static void slot_free(slot_t *s) {
    slot_keys_free(s); slot_names_free(s); slot_hm_free(s); slot_pairs_free(s);
    unpin(s->h_res); frames_free(&s->rd); pieces_free(&s->out);
}

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

/* ---- stage 1: read + frame (search_reader.c), a slot per step -------------------------------- */
static void *reader_main(void *arg) {
    pipe_t *P = (pipe_t *)arg;
    for (int i = 0;; ++i) {
        slot_t *s = &P->slot[i % NSLOTS];
        reader_outcome o;
        if (!wait_state(P, s, S_EMPTY)) return NULL;
        if (i < NSLOTS) {                       /* pinned memory is slow to allocate: do it while earlier chunks are in flight */
            int arc = slot_alloc(s, P);
            if (arc) { set_error(P, arc); return NULL; }
        }
        const int rc = P->paired ? reader_pairs_step(&P->rd, &s->rd, &s->pr.m2, &o) : reader_step(&P->rd, &s->rd, &o);
        if (rc) { set_error(P, rc); return NULL; }
        s->nr = o.nr; s->frame_rc = o.frame_rc; s->last = o.last; s->ferr = o.ferr;
        P->t_read += o.t_read; P->t_frame += o.t_frame;
        set_state(P, s, S_FRAMED);
        if (o.last) return NULL;
    }
}

/* ---- stage 2: GPU ---------------------------------------------------------------------------- */
#define HIPOK(x) do { if ((x) != hipSuccess) { set_error(P, UTREE_E_HIP); return NULL; } } while (0)
#define HIPE(x) do { if ((x) != hipSuccess) return UTREE_E_HIP; } while (0)      /* ... in what gpu_main and search_file call */

/* the hit map of device g's shard, behind its classify call on the same device buffers; meta and offsets come back with the results */
static int hitmap_launch(pipe_t *P, slot_t *s, size_t g, const utree_batch_view *v, size_t first) {
    gpu_ctx *c = &P->G[g];
    const size_t count = v->n_reads;
    s->hm.first[g] = first; s->hm.count[g] = count;
    int e = utree_hitmap_batch(c->dev, v->d_bases, v->d_off, v->d_len, v->n_reads, v->total_bases, v->do_rc, c->hm.d_run_off, c->hm.d_runs, c->hm.runs_cap, c->hm.d_meta,
                               c->hm.d_ws, c->hm.ws_bytes, c->stream);
    if (e) return e;
    if (hipMemcpyAsync(&s->hm.h_meta[g], c->hm.d_meta, sizeof(utree_hitmap_meta), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return UTREE_E_HIP;
    if (hipMemcpyAsync(s->hm.h_run_off + first + g, c->hm.d_run_off, (count + 1) * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return UTREE_E_HIP;
    return UTREE_OK;
}

/* once the streams have drained: exactly the runs there are, the shards' one after the other, into the slot's pinned buffer */
static int hitmap_fetch(pipe_t *P, slot_t *s) {
    uint64_t runs = 0;
    for (int g = 0; g < P->n_dev; ++g) {
        if (!s->hm.count[g]) continue;
        if (s->hm.h_meta[g].error) {
            snprintf(P->msg_join, sizeof P->msg_join, "the hit map of a batch reported error %u (%llu runs, %llu windows)", s->hm.h_meta[g].error,
                     (unsigned long long)s->hm.h_meta[g].total_runs, (unsigned long long)s->hm.h_meta[g].total_windows);
            return UTREE_E_DEVICE;
        }
        s->hm.base[g] = runs; runs += s->hm.h_meta[g].total_runs;
    }
    if (runs > s->hm.runs_cap) {
        size_t cap = s->hm.runs_cap ? s->hm.runs_cap : (size_t)1 << 20;
        while (cap < runs) cap *= 2;
        unpin(s->hm.h_runs);
        s->hm.h_runs = NULL; s->hm.runs_cap = 0;
        if (pin(&s->hm.h_runs, cap * sizeof(utree_hit_run))) return UTREE_E_NOMEM;
        s->hm.runs_cap = cap;
    }
    for (int g = 0; g < P->n_dev; ++g) {
        if (!s->hm.count[g] || !s->hm.h_meta[g].total_runs) continue;
        if (hipSetDevice(P->G[g].dev->device) != hipSuccess ||
            hipMemcpyAsync(s->hm.h_runs + s->hm.base[g], P->G[g].hm.d_runs, s->hm.h_meta[g].total_runs * sizeof(utree_hit_run), hipMemcpyDeviceToHost,
                           P->G[g].stream) != hipSuccess) return UTREE_E_HIP;
    }
    for (int g = 0; g < P->n_dev; ++g)
        if (s->hm.count[g] && (hipSetDevice(P->G[g].dev->device) != hipSuccess || hipStreamSynchronize(P->G[g].stream) != hipSuccess)) return UTREE_E_HIP;
    return UTREE_OK;
}

/* the names of device g's shard [first, first + count) for the reports that read them: offsets relative to the uploaded span, which begins
 * at rd.buf + lo and holds `span` bytes, on the shard's stream */
static int names_upload(pipe_t *P, slot_t *s, size_t g, size_t first, size_t count, size_t lo, size_t span) {
    gpu_ctx *c = &P->G[g];
    if (span >= ((uint64_t)1 << 32)) return UTREE_E_ARG;
    uint32_t *rel = s->nm.h_rel + first, *len = s->nm.h_rel + MAX_READS_PER_BATCH + first;
    for (size_t r = 0; r < count; ++r) {
        if (s->rd.name_off[first + r] < lo || s->rd.name_off[first + r] - lo + s->rd.name_len[first + r] > span) return UTREE_E_ARG;   /* (cannot happen: a name precedes its read) */
        rel[r] = (uint32_t)(s->rd.name_off[first + r] - lo); len[r] = s->rd.name_len[first + r];
    }
    if (hipMemcpyAsync(c->nm.d_off, rel, count * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess) return UTREE_E_HIP;
    if (hipMemcpyAsync(c->nm.d_len, len, count * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess) return UTREE_E_HIP;
    return UTREE_OK;
}

/* Stage device g's shard [first, first + count) of slot `s`: the byte span and the framed arrays go up as they stand, on the shard's stream, and
 * *v is the batch the kernels see.  *lo: where in rd.buf the uploaded span -- the view's text, with names -- begins. */
static int stage_reads(pipe_t *P, slot_t *s, size_t g, size_t first, size_t count, utree_batch_view *v, size_t *lo_out) {
    gpu_ctx *c = &P->G[g];
    const size_t last = first + count - 1;
    size_t lo = (size_t)s->rd.seq_off[first], hi = (size_t)s->rd.seq_off[last] + s->rd.seq_len[last];
    if (P->names && (size_t)s->rd.name_off[first] < lo) lo = (size_t)s->rd.name_off[first];      /* the span from the first name on: the names are read there */
    uint64_t total = 0; uint32_t mx = 0;
    for (size_t r = first; r <= last; ++r) {
        s->rd.rel_off[r] = s->rd.seq_off[r] - lo; total += s->rd.seq_len[r];
        if (s->rd.seq_len[r] > mx) mx = s->rd.seq_len[r];
    }
    HIPE(hipSetDevice(c->dev->device));
    HIPE(hipMemcpyAsync(c->d_buf, s->rd.buf + lo, hi - lo, hipMemcpyHostToDevice, c->stream));
    HIPE(hipMemcpyAsync(c->d_off, s->rd.rel_off + first, count * 8, hipMemcpyHostToDevice, c->stream));
    HIPE(hipMemcpyAsync(c->d_len, s->rd.seq_len + first, count * 4, hipMemcpyHostToDevice, c->stream));
    *v = (utree_batch_view){c->d_buf, c->d_off, c->d_len, (uint32_t)count, total, mx, P->req->do_rc, c->d_buf, hi - lo, c->nm.d_off, c->nm.d_len, c->stream};
    *lo_out = lo;
    return UTREE_OK;
}

/* ... of a paired search: both mates' byte spans and framed arrays go up as they stand; the device joins them and the batch kernels, the reports
 * included, see one query per pair.  The view's text is mate 1's span. */
static int stage_pairs(pipe_t *P, slot_t *s, size_t g, size_t first, size_t count, utree_batch_view *v, size_t *lo_out) {
    gpu_ctx *c = &P->G[g];
    const int two = P->paired == PAIRS_TWO_FILES;
    const frames_t *m = &s->pr.m2;
    const size_t last = first + count - 1;
    size_t lo1 = (size_t)s->rd.seq_off[first], hi1 = (size_t)s->rd.seq_off[last] + s->rd.seq_len[last];
    size_t lo2 = (size_t)m->seq_off[first], hi2 = (size_t)m->seq_off[last] + m->seq_len[last];
    if (P->names && (size_t)s->rd.name_off[first] < lo1) lo1 = (size_t)s->rd.name_off[first];   /* the span from mate 1's first name on: the names are read there */
    if (!two) { hi1 = hi2; lo2 = lo1; }                                        /* interleaved: one span holds both */
    uint64_t total = 0; uint32_t mx = 0;
    for (size_t r = first; r <= last; ++r) {
        s->rd.rel_off[r] = s->rd.seq_off[r] - lo1; m->rel_off[r] = m->seq_off[r] - lo2;
        const uint32_t jl = s->rd.seq_len[r] + 1u + m->seq_len[r];                /* <= LINELEN_MAX: the reader saw to it */
        total += jl;
        if (jl > mx) mx = jl;
    }
    if (total > c->pr.joined_cap) return UTREE_E_ARG;                             /* (cannot happen: the buffers' bytes + one per pair) */
    HIPE(hipSetDevice(c->dev->device));
    HIPE(hipMemcpyAsync(c->d_buf, s->rd.buf + lo1, hi1 - lo1, hipMemcpyHostToDevice, c->stream));
    if (two) HIPE(hipMemcpyAsync(c->pr.d_buf2, m->buf + lo2, hi2 - lo2, hipMemcpyHostToDevice, c->stream));
    HIPE(hipMemcpyAsync(c->d_off, s->rd.rel_off + first, count * 8, hipMemcpyHostToDevice, c->stream));
    HIPE(hipMemcpyAsync(c->d_len, s->rd.seq_len + first, count * 4, hipMemcpyHostToDevice, c->stream));
    HIPE(hipMemcpyAsync(c->pr.d_off2, m->rel_off + first, count * 8, hipMemcpyHostToDevice, c->stream));
    HIPE(hipMemcpyAsync(c->pr.d_len2, m->seq_len + first, count * 4, hipMemcpyHostToDevice, c->stream));
    /* the host has the lengths: total and max_len are its own, the join's meta comes back with the results and is checked then */
    const int e = utree_pairs_join(c->dev, c->d_buf, c->d_off, c->d_len, two ? c->pr.d_buf2 : c->d_buf, c->pr.d_off2, c->pr.d_len2, (uint32_t)count,
                                   c->pr.d_joined, total, c->pr.d_joff, c->pr.d_jlen, c->pr.d_meta, c->stream);
    if (e) return e;
    c->pr.want_total = total;
    HIPE(hipMemcpyAsync(&s->pr.h_meta[g], c->pr.d_meta, sizeof(utree_pairs_meta), hipMemcpyDeviceToHost, c->stream));
    *v = (utree_batch_view){c->pr.d_joined, c->pr.d_joff, c->pr.d_jlen, (uint32_t)count, total, mx, P->req->do_rc, c->d_buf, hi1 - lo1, c->nm.d_off, c->nm.d_len, c->stream};
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
        s->ky.per = per ? per : 1;
        for (size_t g = 0; g < n_dev && nr && P->paired; ++g) { memset(&s->pr.h_meta[g], 0, sizeof s->pr.h_meta[g]); P->G[g].pr.want_total = 0; }
        for (size_t g = 0; g < n_dev && P->hm; ++g) { s->hm.first[g] = 0; s->hm.count[g] = 0; s->hm.base[g] = 0; }
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
                             : utree_reports_classify(P->rep, (int)g, c->dev, &v, c->d_out, c->d_ws, c->ws_bytes, P->keys ? c->ky.d_key : NULL);
            if (!e && P->keys && hipMemcpyAsync(s->ky.h_key + first, c->ky.d_key, count * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess) e = UTREE_E_HIP;
            if (!e) e = utree_reports_add(P->rep, (int)g, &v, c->d_out, rank != NULL);
            if (!e && P->hm) e = hitmap_launch(P, s, g, &v, first);
            if (!e && hipMemcpyAsync(s->h_res + first, c->d_out, count * sizeof(utree_result), hipMemcpyDeviceToHost, c->stream) != hipSuccess) e = UTREE_E_HIP;
            if (e) { set_error(P, e); return NULL; }
        }
        for (size_t g = 0; g < n_dev && nr; ++g) {
            HIPOK(hipSetDevice(P->G[g].dev->device));
            HIPOK(hipStreamSynchronize(P->G[g].stream));
            if (!rank) { int pe = utree_classify_poll(P->G[g].dev); if (pe) { set_error(P, pe); return NULL; } }   /* the batches' error words */
            if (P->paired && (s->pr.h_meta[g].error || s->pr.h_meta[g].total_bases != P->G[g].pr.want_total)) {               /* ... and the join's */
                snprintf(P->msg_join, sizeof P->msg_join, "the device join of a batch of pairs reported error %u, %llu joined bytes where the host counted %llu",
                         s->pr.h_meta[g].error, (unsigned long long)s->pr.h_meta[g].total_bases, (unsigned long long)P->G[g].pr.want_total);
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
/* the spool records of [a, b), piece t: one per query that prints a line, in the lines' order.  Nonzero: no memory */
static int format_spool(pipe_t *P, slot_t *s, int t, size_t a, size_t b) {
    size_t need = 0, sl = 0;
    for (size_t r = a; r < b; ++r) if (s->h_res[r].found) need += sizeof(utree_spool_rec) + s->rd.name_len[r];
    char *o = piece_reserve(&s->ky.recs, t, need);
    s->ky.recs.len[t] = 0;
    if (need && !o) return 1;
    for (size_t r = a; r < b; ++r) {
        if (!s->h_res[r].found) continue;
        const utree_spool_rec rec = {s->ky.h_key[r], (uint32_t)(r / s->ky.per), s->rd.name_len[r]};
        memcpy(o + sl, &rec, sizeof rec); sl += sizeof rec;
        memcpy(o + sl, s->rd.buf + s->rd.name_off[r], s->rd.name_len[r]); sl += s->rd.name_len[r];
    }
    s->ky.recs.len[t] = sl;
    return 0;
}

/* the map's lines of [a, b), piece t: a line per query; the slice is cut where one device's shard ends and the next one's begins.  Nonzero: no memory */
static int format_map(pipe_t *P, slot_t *s, int t, size_t a, size_t b) {
    size_t need = 64, hl = 0;
    for (size_t r = a; r < b; ++r) need += (size_t)s->rd.name_len[r] + 48;
    for (int g = 0; g < P->n_dev; ++g) {
        const size_t f = s->hm.first[g], e = f + s->hm.count[g], x = a > f ? a : f, y = b < e ? b : e;
        if (x < y) need += 22 * (size_t)(s->hm.h_run_off[y + (size_t)g] - s->hm.h_run_off[x + (size_t)g]);        /* "4294967295:4294967295 " */
    }
    char *o = piece_reserve(&s->hm.lines, t, need);
    for (int g = 0; g < P->n_dev && o && hl != (size_t)-1; ++g) {
        const size_t f = s->hm.first[g], e = f + s->hm.count[g], x = a > f ? a : f, y = b < e ? b : e;
        if (x >= y) continue;
        const size_t w = utree_hitmap_format(s->rd.buf, s->rd.name_off + x, s->rd.name_len + x, s->hm.h_run_off + x + (size_t)g, s->hm.h_runs + s->hm.base[g], y - x,
                                             o + hl, s->hm.lines.cap[t] - hl);
        hl = w == (size_t)-1 ? w : hl + w;
    }
    s->hm.lines.len[t] = !o || hl == (size_t)-1 ? 0 : hl;
    return !o || hl == (size_t)-1;
}

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
                need += (size_t)s->rd.name_len[r] + ll + 64;
            }
            char *o = piece_reserve(&s->out, t, need);
            uint64_t good = 0;
            size_t L = !o ? (size_t)-1
                       : P->req->rank ? utree_format_rank_records(P->ctr, s->rd.buf, s->rd.name_off + a, s->rd.name_len + a, s->h_res + a, b - a, o, s->out.cap[t], &good)
                                      : utree_format_records(P->ctr, s->rd.buf, s->rd.name_off + a, s->rd.name_len + a, s->h_res + a, b - a, o, s->out.cap[t], &good);
            if (L == (size_t)-1) { fail |= 1; s->out.len[t] = 0; } else { s->out.len[t] = L; good_total += good; }
            if (P->keys) fail |= format_spool(P, s, t, a, b);
            if (P->hm) fail |= format_map(P, s, t, a, b);
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
        if (pieces_write(P->fo, &s->out, s->fmt_T) < 0) { set_error(P, UTREE_E_IO); return NULL; }
        if (P->hm && P->fh >= 0 && pieces_write(P->fh, &s->hm.lines, s->fmt_T) < 0) {   /* the same chunk's map lines: both files hold the same queries */
            snprintf(P->hm_msg, 512, "hit map %s: cannot write the file (%s)", P->req->hitmap_path, strerror(errno));
            close(P->fh); P->fh = -1;                                               /* the search goes on without its map */
        }
        if (P->keys && P->fs >= 0 && pieces_write(P->fs, &s->ky.recs, s->fmt_T) < 0) {   /* ... and its spool records */
            snprintf(P->sp_msg, 512, "cannot write the spool %.300s.spool (%s)", P->req->redistribute_reads_path, strerror(errno));
            close(P->fs); P->fs = -1;                                               /* the search goes on without that report */
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

/* ---- device g's buffers for the slots' shards: the worst case of a shard is the slot's reads and bytes; per feature what it adds ---- */
static int ctx_pairs_alloc(gpu_ctx *c, const pipe_t *P) {                         /* the second mates, and the joined batch: both buffers' bytes + an 'N' per pair */
    c->pr.joined_cap = (P->paired == PAIRS_TWO_FILES ? 2 : 1) * P->chunk + MAX_READS_PER_BATCH;
    if (P->paired == PAIRS_TWO_FILES) HIPE(hipMalloc((void **)&c->pr.d_buf2, P->chunk + 64));
    HIPE(hipMalloc((void **)&c->pr.d_joined, c->pr.joined_cap + 64));
    HIPE(hipMalloc((void **)&c->pr.d_off2, MAX_READS_PER_BATCH * 8));
    HIPE(hipMalloc((void **)&c->pr.d_len2, MAX_READS_PER_BATCH * 4));
    HIPE(hipMalloc((void **)&c->pr.d_joff, MAX_READS_PER_BATCH * 8));
    HIPE(hipMalloc((void **)&c->pr.d_jlen, MAX_READS_PER_BATCH * 4));
    HIPE(hipMalloc((void **)&c->pr.d_meta, sizeof(utree_pairs_meta)));
    return UTREE_OK;
}
static int ctx_hm_alloc(gpu_ctx *c, const pipe_t *P) {                            /* a run per window */
    const uint64_t tb = P->paired ? c->pr.joined_cap : P->chunk;
    c->hm.runs_cap = utk_hitmap_wcap((uint32_t)MAX_READS_PER_BATCH, tb, P->req->do_rc);
    c->hm.ws_bytes = utree_hitmap_workspace_bytes(c->dev, (uint32_t)MAX_READS_PER_BATCH, tb, P->req->do_rc);
    if (!c->hm.ws_bytes) return UTREE_E_ARG;
    HIPE(hipMalloc((void **)&c->hm.d_run_off, (MAX_READS_PER_BATCH + 1) * 8));
    HIPE(hipMalloc((void **)&c->hm.d_runs, (size_t)(c->hm.runs_cap + 1) * sizeof(utree_hit_run)));
    HIPE(hipMalloc((void **)&c->hm.d_meta, sizeof(utree_hitmap_meta)));
    HIPE(hipMalloc(&c->hm.d_ws, c->hm.ws_bytes));
    return UTREE_OK;
}
static int ctx_names_alloc(gpu_ctx *c) { HIPE(hipMalloc((void **)&c->nm.d_off, MAX_READS_PER_BATCH * 4)); HIPE(hipMalloc((void **)&c->nm.d_len, MAX_READS_PER_BATCH * 4)); return UTREE_OK; }
static int ctx_keys_alloc(gpu_ctx *c) { HIPE(hipMalloc((void **)&c->ky.d_key, MAX_READS_PER_BATCH * 4)); return UTREE_OK; }

static int ctx_alloc(pipe_t *P, gpu_ctx *c, utree_dev *dev) {
    const utree_search_request *req = P->req;
    int rc = UTREE_OK;
    c->dev = dev;
    HIPE(hipSetDevice(dev->device));
    HIPE(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIPE(hipMalloc((void **)&c->d_buf, P->chunk + 64));
    HIPE(hipMalloc((void **)&c->d_off, MAX_READS_PER_BATCH * 8));
    HIPE(hipMalloc((void **)&c->d_len, MAX_READS_PER_BATCH * 4));
    HIPE(hipMalloc((void **)&c->d_out, MAX_READS_PER_BATCH * sizeof(utree_result)));
    if (!rc && P->paired) rc = ctx_pairs_alloc(c, P);
    if (!rc && P->hm) rc = ctx_hm_alloc(c, P);
    if (!rc && P->names) rc = ctx_names_alloc(c);
    if (!rc && P->keys) rc = ctx_keys_alloc(c);
    if (rc) return rc;
    c->ws_bytes = req->rank ? utree_rank_workspace_bytes(dev, (uint32_t)MAX_READS_PER_BATCH, CHUNK_BYTES, LINELEN_MAX, req->do_rc, req->rank)
                            : utree_classify_workspace_bytes(dev, (uint32_t)MAX_READS_PER_BATCH, P->paired ? c->pr.joined_cap : CHUNK_BYTES, LINELEN_MAX, req->do_rc);
    if (!c->ws_bytes) return UTREE_E_ARG;
    HIPE(hipMalloc(&c->d_ws, c->ws_bytes));
    return UTREE_OK;
}

static void free_ctx(gpu_ctx *c) {
    void *dev_mem[] = {c->d_buf, c->d_off, c->d_len, c->d_out, c->d_ws, c->pr.d_buf2, c->pr.d_joined, c->pr.d_off2, c->pr.d_len2, c->pr.d_joff, c->pr.d_jlen,
                       c->pr.d_meta, c->hm.d_run_off, c->hm.d_runs, c->hm.d_meta, c->hm.d_ws, c->nm.d_off, c->nm.d_len, c->ky.d_key};
    if (!c->dev) return;
    hipSetDevice(c->dev->device);
    for (size_t i = 0; i < sizeof dev_mem / sizeof dev_mem[0]; ++i) if (dev_mem[i]) hipFree(dev_mem[i]);
    if (c->stream) hipStreamDestroy(c->stream);
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
 * on every way out (utree_search_checked); fd -1 and msg: it could not be created, or written */
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
    pipe_t pipe, *P = &pipe;                                                      /* (the stages end before this call does) */
    int set_up = 0;                                                               /* the files are open: from here on the search gives its stats and its timing line */
    memset(P, 0, sizeof *P);
    pthread_mutex_init(&P->mu, NULL);
    pthread_cond_init(&P->cv, NULL);
    P->ctr = ctr; P->req = req; P->rep = rep; P->n_dev = n_dev;
    P->progress_printed = dev_printed;
    P->paired = paired; P->chunk = paired || hitmap_path || req->redistribute_reads_path ? utree_chunk_bytes(CHUNK_BYTES) : CHUNK_BYTES;
    P->fs = sp ? sp->fd : -1; P->keys = P->fs >= 0 && utree_reports_wants_keys(rep); P->sp_msg = sp ? sp->msg : NULL;
    if (sp) sp->fd = -1;                                                          /* (this search's to close from here on) */
    P->names = utree_reports_wants_names(rep);
    P->hm = hitmap_path != NULL; P->fh = -1; P->hm_msg = hm_msg;
    reader_t *R = &P->rd;
    R->input_format = req->input_format; R->paired = paired; R->chunk = P->chunk; R->max_reads = MAX_READS_PER_BATCH;
    R->reads_path = req->reads_path; R->mates_path = req->mates_path; R->msg_pairs = P->msg_pairs; R->msg_cap = sizeof P->msg_pairs;
    R->in[1].fd = -1;
    R->in[0].fd = open(req->reads_path, O_RDONLY);
    if (paired == PAIRS_TWO_FILES && R->in[0].fd >= 0 && (R->in[1].fd = open(req->mates_path, O_RDONLY)) < 0) { close(R->in[0].fd); R->in[0].fd = -1; }
    if (resume.fo >= 0) {
        /* the output is a pipe and the device pipeline has written the chunks in front of `in_off`: go on from there, on the same descriptor */
        P->fo = resume.fo; R->in[0].pos = (off_t)resume.in_off;
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
    if (R->in[0].fd < 0 || P->fo < 0) { rc = UTREE_E_IO; goto done; }             /* itree.c:835 */
    if (P->hm) {
        /* a map that cannot be opened, or whose labels cannot be written, does not stop the search: it runs without one and says so at its end */
        P->fh = open(hitmap_path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (P->fh < 0) snprintf(hm_msg, 512, "hit map %s: cannot open the file (%s)", hitmap_path, strerror(errno));
        else if (write_labels(ctr, hitmap_path, hm_msg)) { close(P->fh); P->fh = -1; }
        if (P->fh < 0) P->hm = 0;
    }
    for (int k = 0; k < 2 && req->input_format != UTREE_INPUT_REFERENCE; ++k) {
        if (R->in[k].fd < 0) continue;
        R->in[k].gz = gzdopen(dup(R->in[k].fd), "rb");
        if (!R->in[k].gz) { rc = UTREE_E_IO; goto done; }
        gzbuffer(R->in[k].gz, 1u << 20);
    }
    set_up = 1;
    int host_threads = req->host_threads;
#ifdef _OPENMP
    if (host_threads <= 0) host_threads = omp_get_max_threads();
#else
    host_threads = 1;
#endif
    if (host_threads > 16) host_threads = 16;                                     /* formatting saturates well before that */
    P->host_threads = host_threads;
    P->G = (gpu_ctx *)calloc((size_t)n_dev, sizeof(gpu_ctx));
    if (!P->G) { rc = UTREE_E_NOMEM; goto done; }
    for (int g = 0; g < n_dev; ++g) if ((rc = ctx_alloc(P, &P->G[g], devs[g]))) goto done;
    {
        pthread_t tr, tg, tf, tw;
        pthread_create(&tr, NULL, reader_main, P);
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
done:                                                                             /* every way out behind the device pipeline's */
    for (int k = 0; k < 2; ++k) {
        if (R->in[k].gz) gzclose(R->in[k].gz);
        if (R->in[k].fd >= 0) close(R->in[k].fd);
    }
    if (P->fo >= 0) close(P->fo);
    if (P->fh >= 0 && close(P->fh) && !hm_msg[0]) snprintf(hm_msg, 512, "hit map %s: cannot write the file (%s)", hitmap_path, strerror(errno));
    if (P->fs >= 0 && close(P->fs) && !sp->msg[0]) snprintf(sp->msg, sizeof sp->msg, "cannot write the spool %.300s (%s)", sp->path, strerror(errno));
    if (P->G) { for (int g = 0; g < n_dev; ++g) free_ctx(&P->G[g]); free(P->G); }
    for (int i = 0; i < NSLOTS; ++i) slot_free(&P->slot[i]);
    pthread_mutex_destroy(&P->mu);
    pthread_cond_destroy(&P->cv);
    if (!set_up) return rc;                                                       /* an input or the output could not be opened: no stats, no timing line */
    P->st.seconds_total = now_s() - t_start;
    P->st.seconds_kernels = P->t_gpu;
    P->st.pipeline = 0; P->st.n_lanes = 1;
    P->st.seconds_read = P->t_read; P->st.seconds_frame = P->t_frame; P->st.seconds_classify_format = P->t_gpu;
    P->st.seconds_d2h = P->t_format; P->st.seconds_write = P->t_write;
    if (timing_on())
        fprintf(stderr, "[utree_amd] stages: read %.3f s, frame %.3f s | gpu %.3f s | format %.3f s, write %.3f s (overlapped)\n",
                P->t_read, P->t_frame, P->t_gpu, P->t_format, P->t_write);
    if (stats) *stats = P->st;
    return rc;
}

/* One checked request (search_entry.c): its reports are fed while searching and written when the search has succeeded (the search's own codes stay its own) */
int utree_search_checked(const utree_ctr *ctr, utree_dev **devs, int n_dev, const utree_search_request *req, utree_search_stats *stats) {
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
