/* tiles_file.c -- utree_tiles_file (include/utree_amd.h): a reads file in, tiles.tsv and segments.tsv out.
 *
 * Host: reading and framing (search_reader.c: the search's own reader, so the reference's framing, UTREE_INPUT and gzip come with it), the
 * text of both files, the segment merge.  Device: everything per tile -- the plan, the views, the classification.  A chunk's bytes are
 * uploaded once; its tiles are views into them (tiles_kernels.hip) and go through utree_classify_batch in sub-batches of at most
 * UTREE_TILES_BATCH tiles, because a chunk of W/S-fold overlapping tiles holds more of them than a batch takes.  A query never straddles
 * chunks, its tiles may straddle sub-batches: the open run of the segment merge is carried from one sub-batch to the next and closed at the
 * chunk's end.
 *
 * Two slots: a reader thread fills one while this thread carries the other through the device and writes its lines.  Nothing of search.c's
 * ring is used. */
#define _FILE_OFFSET_BITS 64
#define _GNU_SOURCE
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <errno.h>
#include <fcntl.h>
#include <pthread.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>
#ifdef _OPENMP
#include <omp.h>
#endif
#include "ctr_host.h"
#include "dev_image.h"
#include "search_dev.h"
#include "search_reader.h"
#include "tiles.h"

#define TL_CHUNK_BYTES ((size_t)96 << 20)       /* must hold two maximal (16 MiB) lines, as the search's */
#define TL_MAX_READS ((size_t)UTREE_TILES_MAX_BATCH)
#define TL_NSLOTS 2
#define TL_MAX_TEAM 16

typedef struct {
    frames_t f;
    reader_outcome o;
    int rc;                                      /* reader_step's own                                  */
    int full;                                    /* filled and not yet given back                      */
} tslot;

typedef struct {
    reader_t R;
    tslot slot[TL_NSLOTS];
    pthread_mutex_t mu; pthread_cond_t cv;
    int stop;
} treader;

static void *reader_main(void *arg) {
    treader *T = (treader *)arg;
    for (unsigned i = 0;; ++i) {
        tslot *s = &T->slot[i % TL_NSLOTS];
        pthread_mutex_lock(&T->mu);
        while (s->full && !T->stop) pthread_cond_wait(&T->cv, &T->mu);
        const int stop = T->stop;
        pthread_mutex_unlock(&T->mu);
        if (stop) break;
        s->rc = reader_step(&T->R, &s->f, &s->o);
        const int end = s->rc || s->o.last || s->o.frame_rc != UTREE_OK;
        pthread_mutex_lock(&T->mu); s->full = 1; pthread_cond_broadcast(&T->cv); pthread_mutex_unlock(&T->mu);
        if (end) break;
    }
    return NULL;
}

/* everything one run holds, so that one place gives it back */
typedef struct {
    hipStream_t st;
    uint8_t *d_bases; uint64_t *d_off, *d_tile_first, *d_toff; uint32_t *d_len, *d_tlen, *d_tquery, *d_tindex;
    utree_result *d_res; utree_tiles_meta *d_meta; void *d_plan_ws, *d_ws; size_t plan_ws_bytes, ws_bytes;
    utree_result *h_res; uint32_t *h_tquery, *h_tindex; utree_tiles_meta *h_meta;
    char *text[TL_MAX_TEAM + 1]; size_t text_cap[TL_MAX_TEAM + 1];   /* the last: the segments' */
    int ft, fs;
} trun;

#define HIPQ(call, what) do { if ((call) != hipSuccess) { utree_dev_set_hip_error((int)hipGetLastError(), what); rc = UTREE_E_HIP; goto done; } } while (0)

static int write_all(int fd, const char *p, size_t n) {
    while (n) {
        const ssize_t w = write(fd, p, n);
        if (w < 0) { if (errno == EINTR) continue; return -1; }
        p += w; n -= (size_t)w;
    }
    return 0;
}

/* the tile lines of tiles [a, b) of a sub-batch into the run's buffer `k`, grown until they fit */
static size_t format_slice(trun *X, int k, const utree_ctr *ctr, const tslot *s, const utree_tiles_params *p, size_t a, size_t b, uint64_t *lines) {
    for (;;) {
        uint64_t got = 0;
        const size_t w = X->text[k] ? utree_tiles_format(ctr, s->f.buf, s->f.name_off, s->f.name_len, s->f.seq_len, p->tile_bp, p->step_bp,
                                                         X->h_tquery + a, X->h_tindex + a, X->h_res + a, b - a, X->text[k], X->text_cap[k], &got)
                                    : (size_t)-1;
        if (w != (size_t)-1) { *lines = got; return w; }
        if (X->text_cap[k] > ((size_t)1 << 36)) return (size_t)-1;             /* (the labels were checked: only the size is left) */
        const size_t cap = X->text_cap[k] ? X->text_cap[k] * 2 : (size_t)1 << 20;
        char *t = (char *)realloc(X->text[k], cap);
        if (!t) return (size_t)-1;
        X->text[k] = t; X->text_cap[k] = cap;
    }
}

int utree_tiles_file(const utree_ctr *ctr, utree_dev *dev, const char *reads_path, const char *tiles_path, const char *segments_path,
                     const utree_tiles_params *params, utree_tiles_stats *stats) {
    /* every check of the arguments, before a handle is looked at */
    if (!params || !stats || params->size != sizeof *params || stats->size != sizeof *stats) return UTREE_E_ARG;
    if (!reads_path || !tiles_path) return UTREE_E_ARG;
    if (params->step_bp < 1 || params->step_bp > params->tile_bp || params->tile_bp > UTREE_TILE_MAX_BP) return UTREE_E_ARG;
    if ((params->do_rc != 0 && params->do_rc != 1) || params->input_format < UTREE_INPUT_REFERENCE || params->input_format > UTREE_INPUT_AUTO) return UTREE_E_ARG;
    if (!ctr || !dev) return UTREE_E_ARG;
    memset(stats, 0, sizeof *stats); stats->size = sizeof *stats;

    int rc = UTREE_OK, framing = UTREE_OK, started = 0;
    const double t_start = now_s();
    double t_setup = 0, t_wait = 0, t_text = 0, t_end = 0;                     /* buffers and files; waiting for the reader; formatting and writing; giving back */
    const utree_tiles_params *p = params;
    size_t batch = UTREE_TILES_MAX_BATCH;
    { const char *e = getenv("UTREE_TILES_BATCH"); if (e && atoll(e) >= 1 && (size_t)atoll(e) < batch) batch = (size_t)atoll(e); }
    int team = p->host_threads;
#ifdef _OPENMP
    if (team <= 0) team = omp_get_max_threads();
#else
    team = 1;
#endif
    if (team > TL_MAX_TEAM) team = TL_MAX_TEAM;
    if (team < 1) team = 1;

    treader reader, *T = &reader;
    trun run, *X = &run;
    pthread_t tr;
    memset(T, 0, sizeof *T);
    memset(X, 0, sizeof *X);
    X->ft = X->fs = -1;
    pthread_mutex_init(&T->mu, NULL);
    pthread_cond_init(&T->cv, NULL);
    reader_t *R = &T->R;
    const size_t chunk = utree_chunk_bytes(TL_CHUNK_BYTES);
    R->input_format = p->input_format; R->paired = PAIRS_NONE; R->chunk = chunk; R->max_reads = TL_MAX_READS;
    R->reads_path = reads_path; R->in[1].fd = -1;
    R->in[0].fd = open(reads_path, O_RDONLY);
    if (R->in[0].fd < 0) { rc = UTREE_E_IO; goto done; }
    if ((X->ft = open(tiles_path, O_WRONLY | O_CREAT | O_TRUNC, 0644)) < 0) { rc = UTREE_E_IO; goto done; }
    if (segments_path && (X->fs = open(segments_path, O_WRONLY | O_CREAT | O_TRUNC, 0644)) < 0) { rc = UTREE_E_IO; goto done; }
    if (p->input_format != UTREE_INPUT_REFERENCE) {
        if (!(R->in[0].gz = gzdopen(dup(R->in[0].fd), "rb"))) { rc = UTREE_E_IO; goto done; }
        gzbuffer(R->in[0].gz, 1u << 20);
    }

    HIPQ(hipSetDevice(dev->device), "utree_tiles_file: hipSetDevice");
    HIPQ(hipStreamCreate(&X->st), "utree_tiles_file: hipStreamCreate");
    for (int i = 0; i < TL_NSLOTS; ++i) {
        frames_t *f = &T->slot[i].f;
        HIPQ(hipHostMalloc((void **)&f->buf, chunk + 64, 0), "utree_tiles_file: pinned chunk");
        HIPQ(hipHostMalloc((void **)&f->seq_off, TL_MAX_READS * 8, 0), "utree_tiles_file: pinned offsets");
        HIPQ(hipHostMalloc((void **)&f->seq_len, TL_MAX_READS * 4, 0), "utree_tiles_file: pinned lengths");
        f->name_off = (uint64_t *)malloc(TL_MAX_READS * 8); f->name_len = (uint32_t *)malloc(TL_MAX_READS * 4);
        if (!f->name_off || !f->name_len) { rc = UTREE_E_NOMEM; goto done; }
    }
    X->plan_ws_bytes = utree_tiles_workspace_bytes(dev, (uint32_t)TL_MAX_READS);
    if (!X->plan_ws_bytes) { rc = UTREE_E_HIP; goto done; }
    HIPQ(hipMalloc((void **)&X->d_bases, chunk + 256), "utree_tiles_file: chunk");
    HIPQ(hipMalloc((void **)&X->d_off, TL_MAX_READS * 8), "utree_tiles_file: offsets");
    HIPQ(hipMalloc((void **)&X->d_len, TL_MAX_READS * 4), "utree_tiles_file: lengths");
    HIPQ(hipMalloc((void **)&X->d_tile_first, (TL_MAX_READS + 1) * 8), "utree_tiles_file: tile_first");
    HIPQ(hipMalloc(&X->d_plan_ws, X->plan_ws_bytes), "utree_tiles_file: plan workspace");
    HIPQ(hipMalloc((void **)&X->d_toff, batch * 8), "utree_tiles_file: views");
    HIPQ(hipMalloc((void **)&X->d_tlen, batch * 4), "utree_tiles_file: views");
    HIPQ(hipMalloc((void **)&X->d_tquery, batch * 4), "utree_tiles_file: views");
    HIPQ(hipMalloc((void **)&X->d_tindex, batch * 4), "utree_tiles_file: views");
    HIPQ(hipMalloc((void **)&X->d_res, batch * sizeof(utree_result)), "utree_tiles_file: results");
    HIPQ(hipMalloc((void **)&X->d_meta, sizeof(utree_tiles_meta)), "utree_tiles_file: meta");
    HIPQ(hipHostMalloc((void **)&X->h_res, batch * sizeof(utree_result), 0), "utree_tiles_file: pinned results");
    HIPQ(hipHostMalloc((void **)&X->h_tquery, batch * 4, 0), "utree_tiles_file: pinned results");
    HIPQ(hipHostMalloc((void **)&X->h_tindex, batch * 4, 0), "utree_tiles_file: pinned results");
    HIPQ(hipHostMalloc((void **)&X->h_meta, sizeof(utree_tiles_meta), 0), "utree_tiles_file: pinned meta");

    if (pthread_create(&tr, NULL, reader_main, T)) { rc = UTREE_E_NOMEM; goto done; }
    started = 1;
    t_setup = now_s() - t_start;
    for (unsigned i = 0;; ++i) {
        tslot *s = &T->slot[i % TL_NSLOTS];
        const double t_w = now_s();
        pthread_mutex_lock(&T->mu);
        while (!s->full) pthread_cond_wait(&T->cv, &T->mu);
        pthread_mutex_unlock(&T->mu);
        t_wait += now_s() - t_w;
        if (s->rc) { rc = s->rc; goto done; }
        const size_t nr = s->o.nr;
        stats->bytes_in += s->o.used;
        if (nr) {
            const double t_dev = now_s(), t_text0 = t_text;
            utree_tiles_run open_run;
            memset(&open_run, 0, sizeof open_run);
            HIPQ(hipMemcpyAsync(X->d_bases, s->f.buf, s->o.used, hipMemcpyHostToDevice, X->st), "utree_tiles_file: upload");
            HIPQ(hipMemcpyAsync(X->d_off, s->f.seq_off, nr * 8, hipMemcpyHostToDevice, X->st), "utree_tiles_file: upload");
            HIPQ(hipMemcpyAsync(X->d_len, s->f.seq_len, nr * 4, hipMemcpyHostToDevice, X->st), "utree_tiles_file: upload");
            if ((rc = utree_tiles_plan(dev, X->d_len, (uint32_t)nr, p->tile_bp, p->step_bp, X->d_tile_first, X->d_meta, X->d_plan_ws, X->plan_ws_bytes, X->st))) goto done;
            HIPQ(hipMemcpyAsync(X->h_meta, X->d_meta, sizeof *X->h_meta, hipMemcpyDeviceToHost, X->st), "utree_tiles_file: plan meta");
            HIPQ(hipStreamSynchronize(X->st), "utree_tiles_file: plan");
            const uint64_t total = X->h_meta->total_tiles;
            for (uint64_t first = 0; first < total; first += batch) {
                const size_t n = total - first < batch ? (size_t)(total - first) : batch;
                if ((rc = utree_tiles_views(dev, X->d_off, X->d_len, (uint32_t)nr, p->tile_bp, p->step_bp, X->d_tile_first, first, (uint32_t)n, X->d_toff,
                                            X->d_tlen, X->d_tquery, X->d_tindex, X->d_meta, X->st))) goto done;
                HIPQ(hipMemcpyAsync(X->h_meta, X->d_meta, sizeof *X->h_meta, hipMemcpyDeviceToHost, X->st), "utree_tiles_file: views meta");
                HIPQ(hipMemcpyAsync(X->h_tquery, X->d_tquery, n * 4, hipMemcpyDeviceToHost, X->st), "utree_tiles_file: views");
                HIPQ(hipMemcpyAsync(X->h_tindex, X->d_tindex, n * 4, hipMemcpyDeviceToHost, X->st), "utree_tiles_file: views");
                HIPQ(hipStreamSynchronize(X->st), "utree_tiles_file: views");
                if (X->h_meta->error) { utree_set_error_text("utree_tiles_file: a range of tiles behind the plan's total"); rc = UTREE_E_DEVICE; goto done; }
                /* the exact figures of this sub-batch: the classify path sizes its workspace from them and picks its kernels by max_len */
                const uint64_t tb = X->h_meta->total_bases; const uint32_t ml = X->h_meta->max_len;
                const size_t need = utree_classify_workspace_bytes(dev, (uint32_t)n, tb, ml, p->do_rc);
                if (need > X->ws_bytes) {
                    if (X->d_ws) { HIPQ(hipFree(X->d_ws), "utree_tiles_file: workspace"); X->d_ws = NULL; X->ws_bytes = 0; }
                    if (hipMalloc(&X->d_ws, need + need / 4) != hipSuccess) { utree_dev_set_hip_error((int)hipGetLastError(), "utree_tiles_file: classify workspace"); rc = UTREE_E_NOMEM; goto done; }
                    X->ws_bytes = need + need / 4;
                }
                if ((rc = utree_classify_batch(dev, X->d_bases, X->d_toff, X->d_tlen, (uint32_t)n, tb, ml, p->do_rc, X->d_res, X->d_ws, X->ws_bytes, X->st))) goto done;
                HIPQ(hipMemcpyAsync(X->h_res, X->d_res, n * sizeof(utree_result), hipMemcpyDeviceToHost, X->st), "utree_tiles_file: results");
                HIPQ(hipStreamSynchronize(X->st), "utree_tiles_file: classify");
                if ((rc = utree_classify_poll(dev))) goto done;
                ++stats->n_batches;
                /* a result that names no label of ctr can never be printed: it fails here, at once and under its own code, not as a buffer that never fits */
                for (size_t j = 0; j < n; ++j)
                    if (X->h_res[j].found && X->h_res[j].label >= ctr->info.n_labels) {
                        utree_set_error_text("utree_tiles_file: a tile's result names a label the database does not have");
                        rc = UTREE_E_DEVICE; goto done;
                    }

                /* the text: the tile lines by a team, a slice each, written in order; the runs by one thread, their state carried on */
                const double t_tx = now_s();
                size_t len[TL_MAX_TEAM]; uint64_t lines[TL_MAX_TEAM];
                const int tm = n < 4096 ? 1 : team;
#pragma omp parallel for num_threads(tm) schedule(static, 1)
                for (int k = 0; k < tm; ++k) len[k] = format_slice(X, k, ctr, s, p, n * (size_t)k / (size_t)tm, n * (size_t)(k + 1) / (size_t)tm, &lines[k]);
                for (int k = 0; k < tm; ++k) {
                    if (len[k] == (size_t)-1) { rc = UTREE_E_NOMEM; goto done; }
                    if (write_all(X->ft, X->text[k], len[k])) { rc = UTREE_E_IO; goto done; }
                    stats->classified += lines[k];
                }
                if (X->fs >= 0) {
                    const int last = first + n >= total, k = TL_MAX_TEAM;
                    size_t w;
                    for (;;) {
                        uint64_t got = 0;
                        w = X->text[k] ? utree_tiles_segments_format(ctr, s->f.buf, s->f.name_off, s->f.name_len, s->f.seq_len, p->tile_bp, p->step_bp, X->h_tquery,
                                                                     X->h_tindex, X->h_res, n, last, &open_run, X->text[k], X->text_cap[k], &got)
                                       : (size_t)-1;
                        if (w != (size_t)-1) { stats->segments += got; break; }
                        const size_t cap = X->text_cap[k] ? X->text_cap[k] * 2 : (size_t)1 << 20;
                        char *t = cap > ((size_t)1 << 36) ? NULL : (char *)realloc(X->text[k], cap);
                        if (!t) { rc = UTREE_E_NOMEM; goto done; }
                        X->text[k] = t; X->text_cap[k] = cap;
                    }
                    if (write_all(X->fs, X->text[k], w)) { rc = UTREE_E_IO; goto done; }
                }
                stats->n_tiles += n;
                t_text += now_s() - t_tx;
            }
            stats->n_queries += nr;
            stats->seconds_device += now_s() - t_dev - (t_text - t_text0);
        }
        if (s->o.frame_rc == UTREE_E_FASTA) {                                   /* the tiles of the queries in front of it are written */
            framing = UTREE_E_FASTA;
            stats->fasta_error = s->o.ferr;
            stats->fasta_error.read_index += stats->n_queries - nr;               /* (the framing counts from the chunk's first record) */
        } else if (s->o.frame_rc != UTREE_OK) { rc = s->o.frame_rc; goto done; }
        const int end = s->o.last || framing != UTREE_OK;
        pthread_mutex_lock(&T->mu); s->full = 0; pthread_cond_broadcast(&T->cv); pthread_mutex_unlock(&T->mu);
        if (end) break;
    }
done:
    t_end = now_s();
    if (started) {
        pthread_mutex_lock(&T->mu); T->stop = 1; pthread_cond_broadcast(&T->cv); pthread_mutex_unlock(&T->mu);
        pthread_join(tr, NULL);
    }
    if (X->ft >= 0 && close(X->ft) && !rc) rc = UTREE_E_IO;
    if (X->fs >= 0 && close(X->fs) && !rc) rc = UTREE_E_IO;
    if (rc) {                                                                   /* neither file is left behind */
        if (X->ft >= 0) unlink(tiles_path);
        if (X->fs >= 0) unlink(segments_path);
    }
    if (R->in[0].gz) gzclose(R->in[0].gz);
    if (R->in[0].fd >= 0) close(R->in[0].fd);
    if (X->st) (void)hipStreamSynchronize(X->st);
    for (int i = 0; i < TL_NSLOTS; ++i) {
        frames_t *f = &T->slot[i].f;
        if (f->buf) (void)hipHostFree(f->buf);
        if (f->seq_off) (void)hipHostFree(f->seq_off);
        if (f->seq_len) (void)hipHostFree(f->seq_len);
        free(f->name_off); free(f->name_len);
    }
    void *dv[] = {X->d_bases, X->d_off, X->d_len, X->d_tile_first, X->d_plan_ws, X->d_toff, X->d_tlen, X->d_tquery, X->d_tindex, X->d_res, X->d_meta, X->d_ws};
    for (size_t i = 0; i < sizeof dv / sizeof dv[0]; ++i) if (dv[i]) (void)hipFree(dv[i]);
    void *hv[] = {X->h_res, X->h_tquery, X->h_tindex, X->h_meta};
    for (size_t i = 0; i < sizeof hv / sizeof hv[0]; ++i) if (hv[i]) (void)hipHostFree(hv[i]);
    for (int k = 0; k <= TL_MAX_TEAM; ++k) free(X->text[k]);
    if (X->st) (void)hipStreamDestroy(X->st);
    pthread_mutex_destroy(&T->mu);
    pthread_cond_destroy(&T->cv);
    stats->seconds_total = now_s() - t_start;
    if (timing_on())
        fprintf(stderr, "[utree_amd] tiles: %.3f s = buffers and files %.3f + waiting for the reader %.3f + device %.3f + text %.3f + giving back %.3f (%llu batches)\n",
                stats->seconds_total, t_setup, t_wait, stats->seconds_device, t_text, now_s() - t_end, (unsigned long long)stats->n_batches);
    return rc ? rc : framing;
}
