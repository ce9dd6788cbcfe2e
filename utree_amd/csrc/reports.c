/* reports.c -- the opt-in reports of one whole-file search (reports.h): a profile (profile.c), a coverage handle (coverage.c), a redistribution
 * handle (redist.c: the table and / or each read's redistributed label, whose keys the search spools), a sample table (samples.c) and / or a per-sample redistribution handle (sredist.c) per device handle, fed chunk by chunk, merged and written when the search has succeeded. */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif
#include "ctr_host.h"
#include "dev_image.h"
#include "reports.h"

struct utree_reports {
    int n_dev;
    const char *profile_path, *coverage_path, *redist_path, *reads_path, *samples_path, *sredist_path;    /* reads_path: the redistributed reads */
    utree_dev **devs;
    uint32_t redist_passes;
    struct { utree_profile *prof; utree_coverage *cov; utree_redist *rd; utree_samples *smp; utree_sredist *srd; } dev[];      /* NULL: the search writes no such report */
};

int utree_reports_create(const utree_ctr *ctr, utree_dev **devs, int n_dev, const utree_search_request *req, utree_reports **out) {
    *out = NULL;
    if (!req->profile_path && !req->coverage_path && !req->redistribute_path && !req->samples_path && !req->sample_redistribute_path &&
        !req->redistribute_reads_path) return UTREE_OK;
    utree_reports *rep = (utree_reports *)calloc(1, sizeof *rep + (size_t)n_dev * sizeof rep->dev[0]);
    if (!rep) return UTREE_E_NOMEM;
    rep->n_dev = n_dev; rep->profile_path = req->profile_path; rep->coverage_path = req->coverage_path; rep->redist_path = req->redistribute_path;
    rep->samples_path = req->samples_path; rep->sredist_path = req->sample_redistribute_path; rep->reads_path = req->redistribute_reads_path;
    rep->devs = devs;
    rep->redist_passes = req->max_passes ? req->max_passes : UTREE_REDIST_DEFAULT_PASSES;
    const int delim = req->sample_delim ? req->sample_delim : '_';
    const char *e = getenv("UTREE_PROFILE_CAPACITY");
    const uint32_t cap = e && atoll(e) >= 1 && atoll(e) <= (1ll << 30) ? (uint32_t)atoll(e) : UTREE_PROFILE_DEFAULT_CAPACITY;
    int rc = UTREE_OK;
    for (int g = 0; rep->profile_path && g < n_dev && !rc; ++g) rc = utree_profile_create(devs[g], cap, &rep->dev[g].prof);
    for (int g = 0; rep->coverage_path && g < n_dev && !rc; ++g) rc = utree_coverage_create(ctr, devs[g], NULL, NULL, &rep->dev[g].cov);
    const char *er = getenv("UTREE_REDIST_CAPACITY");
    const uint32_t rcap = er && atoll(er) >= 1 && atoll(er) <= (1ll << 28) ? (uint32_t)atoll(er) : UTREE_REDIST_DEFAULT_CAPACITY;
    for (int g = 0; (rep->redist_path || rep->reads_path) && g < n_dev && !rc; ++g) rc = utree_redist_create(devs[g], rcap, &rep->dev[g].rd);
    const char *es = getenv("UTREE_SAMPLE_CAPACITY"), *ec = getenv("UTREE_SAMPLE_CELLS");
    const uint32_t scap = es && atoll(es) >= 1 && atoll(es) <= (1ll << 19) ? (uint32_t)atoll(es) : UTREE_SAMPLES_DEFAULT_CAPACITY;
    const uint32_t ccap = ec && atoll(ec) >= 1 && atoll(ec) <= (1ll << 30) ? (uint32_t)atoll(ec) : UTREE_SAMPLES_DEFAULT_CELLS;
    for (int g = 0; rep->samples_path && g < n_dev && !rc; ++g) rc = utree_samples_create(devs[g], scap, ccap, delim, &rep->dev[g].smp);
    for (int g = 0; rep->sredist_path && g < n_dev && !rc; ++g) rc = utree_sredist_create(devs[g], scap, rcap, ccap, delim, &rep->dev[g].srd);
    if (rc) { utree_reports_free(rep); return rc; }
    *out = rep;
    return UTREE_OK;
}

void utree_reports_free(utree_reports *rep) {
    if (!rep) return;
    for (int g = 0; g < rep->n_dev; ++g) utree_profile_free(rep->dev[g].prof);
    for (int g = 0; g < rep->n_dev; ++g) utree_coverage_free(rep->dev[g].cov);
    for (int g = 0; g < rep->n_dev; ++g) utree_redist_free(rep->dev[g].rd);
    for (int g = 0; g < rep->n_dev; ++g) utree_samples_free(rep->dev[g].smp);
    for (int g = 0; g < rep->n_dev; ++g) utree_sredist_free(rep->dev[g].srd);
    free(rep);
}

int utree_reports_reset(utree_reports *rep) {
    int rc = UTREE_OK;
    for (int g = 0; rep && g < rep->n_dev && !rc; ++g) if (rep->dev[g].prof) rc = utree_profile_reset(rep->dev[g].prof);
    for (int g = 0; rep && g < rep->n_dev && !rc; ++g) if (rep->dev[g].cov) rc = utree_coverage_reset(rep->dev[g].cov);
    for (int g = 0; rep && g < rep->n_dev && !rc; ++g) if (rep->dev[g].rd) rc = utree_redist_reset(rep->dev[g].rd);
    for (int g = 0; rep && g < rep->n_dev && !rc; ++g) if (rep->dev[g].smp) rc = utree_samples_reset(rep->dev[g].smp);
    for (int g = 0; rep && g < rep->n_dev && !rc; ++g) if (rep->dev[g].srd) rc = utree_sredist_reset(rep->dev[g].srd);
    return rc;
}

int utree_reports_classify(utree_reports *rep, int g, utree_dev *dev, const utree_batch_view *v, utree_result *d_out, void *d_workspace,
                           size_t workspace_bytes, uint32_t *d_key) {
    return utree_classify_view(dev, v, d_out, d_workspace, workspace_bytes, rep ? rep->dev[g].rd : NULL, rep ? rep->dev[g].srd : NULL,   /* (each batch feeds both when both are written) */
                               rep && rep->dev[g].rd ? d_key : NULL);
}

int utree_reports_wants_keys(const utree_reports *rep) { return rep && rep->reads_path; }

int utree_reports_wants_names(const utree_reports *rep) { return rep && (rep->samples_path || rep->sredist_path); }

int utree_reports_add(utree_reports *rep, int g, const utree_batch_view *v, const utree_result *d_res, int rank) {
    if (!rep) return UTREE_OK;
    int rc = rep->dev[g].prof ? utree_profile_add(rep->dev[g].prof, d_res, v->n_reads, v->stream) : UTREE_OK;
    if (!rc && rep->dev[g].smp) rc = utree_samples_add(rep->dev[g].smp, v->d_text, v->text_bytes, v->d_name_off, v->d_name_len, d_res, v->n_reads, v->stream);
    if (!rc && rep->dev[g].cov && !rank) rc = utree_coverage_add(rep->dev[g].cov, v->d_bases, v->d_off, v->d_len, v->n_reads, v->do_rc, v->stream);
    return rc;
}

/* reads every device's entries, checks that they counted n_reads_expected reads (else UTREE_E_DEVICE) and writes the file */
static int write_profile(const utree_reports *rep, const utree_ctr *ctr, uint64_t n_reads_expected) {
    const char *path = rep->profile_path;
    size_t total = 0;
    for (int g = 0; g < rep->n_dev; ++g) total += utree_profile_max_entries(rep->dev[g].prof);
    utree_profile_entry *e = (utree_profile_entry *)malloc((total ? total : 1) * sizeof *e);
    if (!e) return UTREE_E_NOMEM;
    size_t at = 0;
    uint64_t reads = 0;
    int rc = UTREE_OK;
    for (int g = 0; g < rep->n_dev && !rc; ++g) {
        size_t k = 0;
        uint64_t nr = 0;
        rc = utree_profile_read(rep->dev[g].prof, e + at, total - at, &k, &nr, NULL);
        at += k; reads += nr;
    }
    char msg[256];
    if (rc == UTREE_E_DEVICE)
        snprintf(msg, sizeof msg, "profile %s: the table of truncated taxa was too small (raise UTREE_PROFILE_CAPACITY), or a read named no label", path);
    else if (rc)
        snprintf(msg, sizeof msg, "profile %s: the counters could not be read back (%s)", path, utree_strerror(rc));
    else if (reads != n_reads_expected) {                          /* every read counted exactly once, or no file */
        snprintf(msg, sizeof msg, "profile %s: %llu reads counted, the search read %llu", path, (unsigned long long)reads,
                 (unsigned long long)n_reads_expected);
        rc = UTREE_E_DEVICE;
    } else if ((rc = utree_profile_write(ctr, e, at, reads, path)))
        snprintf(msg, sizeof msg, "profile %s: cannot write the file (%s)", path, utree_strerror(rc));
    if (rc) utree_set_error_text(msg);
    free(e);
    return rc;
}

/* merges the devices' handles into the first, checks that n_reads_expected reads were added (else UTREE_E_DEVICE) and writes the file */
static int write_coverage(const utree_reports *rep, const utree_ctr *ctr, uint64_t n_reads_expected) {
    const char *path = rep->coverage_path;
    int rc = UTREE_OK;
    size_t k = 0;
    uint64_t reads = 0;
    utree_coverage_entry *e = (utree_coverage_entry *)malloc(((size_t)ctr->info.n_labels + 1) * sizeof *e);
    if (!e) return UTREE_E_NOMEM;
    for (int g = 1; g < rep->n_dev && !rc; ++g) rc = utree_coverage_merge(rep->dev[0].cov, rep->dev[g].cov);
    if (!rc) rc = utree_coverage_read(rep->dev[0].cov, e, ctr->info.n_labels, &k, &reads, NULL);
    char msg[256];
    if (rc) snprintf(msg, sizeof msg, "coverage %s: the counters could not be merged and read back (%s)", path, utree_strerror(rc));
    else if (reads != n_reads_expected) {                          /* every read added exactly once, or no file */
        snprintf(msg, sizeof msg, "coverage %s: %llu reads added, the search read %llu", path, (unsigned long long)reads,
                 (unsigned long long)n_reads_expected);
        rc = UTREE_E_DEVICE;
    } else if ((rc = utree_coverage_write(ctr, e, k, reads, path)))
        snprintf(msg, sizeof msg, "coverage %s: cannot write the file (%s)", path, utree_strerror(rc));
    if (rc) utree_set_error_text(msg);
    free(e);
    return rc;
}

/* ---- each read's redistributed label: the spool's keys assigned block by block ------------------------------------------------------------ */
#define SPOOL_BLOCK ((size_t)1 << 20)          /* records of a block (the search's batches hold at most twice as many) */
#define SPOOL_RAW_BYTES ((size_t)64 << 20)     /* bytes of the spool read at a time (more only for one record that is longer) */
#define SPOOL_FMT_THREADS 16

typedef struct {                               /* one block: the records in file order, and their keys grouped by device handle */
    uint32_t *dev, *name_len, *label, *ncand, *pos;
    uint64_t *name_off;                        /* into `names`, the spool's bytes as they were read: the block's records are names[0 .. used) */
    uint8_t *names; size_t names_cap, have, used; int eof;
    uint32_t *h_key, *h_label, *h_ncand;       /* pinned, grouped: handle g's records are [first[g], first[g + 1]) */
    size_t *first, *at;                        /* [n_dev + 1], [n_dev] */
    char *out; size_t out_cap;
} spool_block;

static void block_free(spool_block *b) {
    free(b->dev); free(b->name_len); free(b->label); free(b->ncand); free(b->pos); free(b->name_off); free(b->names); free(b->first); free(b->at); free(b->out);
    if (b->h_key) hipHostFree(b->h_key);
    if (b->h_label) hipHostFree(b->h_label);
    if (b->h_ncand) hipHostFree(b->h_ncand);
}

static int block_alloc(spool_block *b, int n_dev) {
    memset(b, 0, sizeof *b);
    b->dev = (uint32_t *)malloc(SPOOL_BLOCK * 4); b->name_len = (uint32_t *)malloc(SPOOL_BLOCK * 4); b->label = (uint32_t *)malloc(SPOOL_BLOCK * 4);
    b->ncand = (uint32_t *)malloc(SPOOL_BLOCK * 4); b->pos = (uint32_t *)malloc(SPOOL_BLOCK * 4); b->name_off = (uint64_t *)malloc(SPOOL_BLOCK * 8);
    b->first = (size_t *)malloc(((size_t)n_dev + 1) * sizeof(size_t)); b->at = (size_t *)malloc((size_t)n_dev * sizeof(size_t));
    b->names = (uint8_t *)malloc(SPOOL_RAW_BYTES); b->names_cap = b->names ? SPOOL_RAW_BYTES : 0;
    if (!b->dev || !b->name_len || !b->label || !b->ncand || !b->pos || !b->name_off || !b->first || !b->at || !b->names) return UTREE_E_NOMEM;
    if (hipHostMalloc((void **)&b->h_key, SPOOL_BLOCK * 4, hipHostMallocDefault) != hipSuccess || hipHostMalloc((void **)&b->h_label, SPOOL_BLOCK * 4, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void **)&b->h_ncand, SPOOL_BLOCK * 4, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return UTREE_E_NOMEM; }
    return UTREE_OK;
}

/* the next block of the spool: the next whole records in the buffer, at most SPOOL_BLOCK, parsed where they were read (when none is left, the
 * rest is carried to the buffer's front and up to SPOOL_RAW_BYTES more are read behind it); 0 records at the spool's end.  The keys wait in label[] (assign_block groups them) */
static int block_read(FILE *f, spool_block *b, int n_dev, size_t *n_out) {
    *n_out = 0;
    for (;;) {
        size_t n = 0, at = b->used;
        while (n < SPOOL_BLOCK && b->have - at >= sizeof(utree_spool_rec)) {
            utree_spool_rec r;
            memcpy(&r, b->names + at, sizeof r);
            if (r.dev >= (uint32_t)n_dev) return UTREE_E_FORMAT;
            if (b->have - at - sizeof r < r.name_len) break;
            b->label[n] = r.key; b->dev[n] = r.dev; b->name_len[n] = r.name_len; b->name_off[n] = at + sizeof r;
            at += sizeof r + r.name_len; ++n;
        }
        b->used = at;
        if (n) { *n_out = n; return UTREE_OK; }
        /* no whole record is left in the buffer: the rest goes to its front and more is read behind it */
        if (b->eof) return b->have > b->used ? UTREE_E_FORMAT : UTREE_OK;     /* (bytes that are no whole record: the spool was cut short) */
        memmove(b->names, b->names + b->used, b->have - b->used); b->have -= b->used; b->used = 0;
        if (b->have == b->names_cap) {                                        /* one record longer than the buffer */
            uint8_t *p = (uint8_t *)realloc(b->names, 2 * b->names_cap);
            if (!p) return UTREE_E_NOMEM;
            b->names = p; b->names_cap *= 2;
        }
        const size_t got = fread(b->names + b->have, 1, b->names_cap - b->have, f);
        b->have += got;
        if (!got) { if (ferror(f)) return UTREE_E_IO; b->eof = 1; }
    }
}

/* n records: their keys grouped by device handle so that each meets its own table, up, utree_redist_assign against the solved first handle, down;
 * every step asynchronous on the handle's stream, one wait per stream at the end; then label / ncand in file order */
static int assign_block(const utree_reports *rep, spool_block *b, size_t n, hipStream_t *streams, uint32_t **d_buf) {
    const int G = rep->n_dev;
    for (int g = 0; g <= G; ++g) b->first[g] = 0;
    for (size_t i = 0; i < n; ++i) ++b->first[b->dev[i] + 1];
    for (int g = 0; g < G; ++g) b->first[g + 1] += b->first[g];
    for (int g = 0; g < G; ++g) b->at[g] = b->first[g];
    for (size_t i = 0; i < n; ++i) { b->pos[i] = (uint32_t)b->at[b->dev[i]]++; b->h_key[b->pos[i]] = b->label[i]; }     /* (label[] held the keys) */
    int rc = UTREE_OK;
    for (int g = 0; g < G && !rc; ++g) {
        const size_t a = b->first[g], c = b->first[g + 1] - a;
        if (!c) continue;
        if (hipSetDevice(rep->devs[g]->device) != hipSuccess) return UTREE_E_HIP;
        if (!streams[g] && hipStreamCreateWithFlags(&streams[g], hipStreamNonBlocking) != hipSuccess) return UTREE_E_HIP;
        if (!d_buf[g] && hipMalloc((void **)&d_buf[g], 3 * SPOOL_BLOCK * 4) != hipSuccess) { (void)hipGetLastError(); return UTREE_E_NOMEM; }
        uint32_t *d_key = d_buf[g], *d_label = d_key + SPOOL_BLOCK, *d_ncand = d_label + SPOOL_BLOCK;
        if (hipMemcpyAsync(d_key, b->h_key + a, c * 4, hipMemcpyHostToDevice, streams[g]) != hipSuccess) return UTREE_E_HIP;
        rc = utree_redist_assign(rep->dev[g].rd, rep->dev[0].rd, d_key, c, d_label, d_ncand, streams[g]);
        if (!rc && (hipMemcpyAsync(b->h_label + a, d_label, c * 4, hipMemcpyDeviceToHost, streams[g]) != hipSuccess ||
                    hipMemcpyAsync(b->h_ncand + a, d_ncand, c * 4, hipMemcpyDeviceToHost, streams[g]) != hipSuccess)) rc = UTREE_E_HIP;
    }
    for (int g = 0; g < G; ++g)
        if (b->first[g + 1] > b->first[g] && streams[g] &&
            (hipSetDevice(rep->devs[g]->device) != hipSuccess || hipStreamSynchronize(streams[g]) != hipSuccess) && !rc) rc = UTREE_E_HIP;
    if (rc) return rc;
    for (size_t i = 0; i < n; ++i) {
        b->label[i] = b->h_label[b->pos[i]]; b->ncand[i] = b->h_ncand[b->pos[i]];
        if (b->label[i] == 0xFFFFFFFFu) return UTREE_E_DEVICE;                  /* a query that printed a line has a candidate */
    }
    return UTREE_OK;
}

/* after the solve of the first handle: the spool's records, block by block, to lines of `path` */
static int write_redist_reads(const utree_reports *rep, const utree_ctr *ctr, const char *spool_path, const char *spool_err) {
    const char *path = rep->reads_path;
    char msg[700];
    if (!spool_path) {
        snprintf(msg, sizeof msg, "redistributed reads %s: %s", path, spool_err && spool_err[0] ? spool_err : "the search kept no spool");
        utree_set_error_text(msg);
        return UTREE_E_IO;
    }
    const int G = rep->n_dev;
    int rc = UTREE_OK;
    spool_block b;
    memset(&b, 0, sizeof b);
    hipStream_t *streams = (hipStream_t *)calloc((size_t)G, sizeof *streams);
    uint32_t **d_buf = (uint32_t **)calloc((size_t)G, sizeof *d_buf);
    FILE *in = NULL, *out = NULL;
    const char *why = "out of memory";
    if (!streams || !d_buf || (rc = block_alloc(&b, G))) { rc = UTREE_E_NOMEM; goto done; }
    if (!(in = fopen(spool_path, "rb"))) { rc = UTREE_E_IO; why = "cannot read the spool back"; goto done; }
    if (!(out = fopen(path, "wb"))) { rc = UTREE_E_IO; why = "cannot write the file"; goto done; }
    for (;;) {
        size_t n = 0;
        if ((rc = block_read(in, &b, G, &n))) { why = "the spool is damaged"; break; }
        if (!n) break;
        if ((rc = assign_block(rep, &b, n, streams, d_buf))) { why = rc == UTREE_E_DEVICE ? "a spooled key names no candidate set" : "the keys could not be assigned"; break; }
        /* the lines, made by a team: piece t is records [n t / T, n (t + 1) / T), into its own stretch of the buffer */
        int T = SPOOL_FMT_THREADS;
#ifdef _OPENMP
        if (omp_get_max_threads() < T) T = omp_get_max_threads();
#else
        T = 1;
#endif
        if ((size_t)T > n / 4096 + 1) T = (int)(n / 4096 + 1);
        size_t off[SPOOL_FMT_THREADS + 1], len[SPOOL_FMT_THREADS];
        off[0] = 0;
        for (int t = 0; t < T; ++t) {
            size_t need = 0;
            for (size_t i = n * (size_t)t / (size_t)T; i < n * (size_t)(t + 1) / (size_t)T; ++i)
                need += (size_t)b.name_len[i] + (b.label[i] < ctr->info.n_labels ? ctr->label_len[b.label[i]] : 0) + 16;
            off[t + 1] = off[t] + need;
        }
        if (off[T] > b.out_cap) { free(b.out); b.out = (char *)malloc(off[T] + off[T] / 4); b.out_cap = b.out ? off[T] + off[T] / 4 : 0; }
        if (!b.out) { rc = UTREE_E_NOMEM; why = "out of memory"; break; }
#pragma omp parallel for num_threads(T) schedule(static, 1)
        for (int t = 0; t < T; ++t) {
            const size_t lo = n * (size_t)t / (size_t)T, hi = n * (size_t)(t + 1) / (size_t)T;
            len[t] = utree_redist_reads_format(ctr, b.names, b.name_off + lo, b.name_len + lo, b.label + lo, b.ncand + lo, hi - lo, b.out + off[t], off[t + 1] - off[t]);
        }
        for (int t = 0; t < T && !rc; ++t) {
            if (len[t] == (size_t)-1) { rc = UTREE_E_DEVICE; why = "an assigned label is none of the database's"; }
            else if (fwrite(b.out + off[t], 1, len[t], out) != len[t]) { rc = UTREE_E_IO; why = "cannot write the file"; }
        }
        if (rc) break;
    }
done:
    if (in) fclose(in);
    if (out && fclose(out) && !rc) { rc = UTREE_E_IO; why = "cannot write the file"; }
    for (int g = 0; g < G && streams && d_buf; ++g) {
        if (!streams[g] && !d_buf[g]) continue;
        hipSetDevice(rep->devs[g]->device);
        if (d_buf[g]) hipFree(d_buf[g]);
        if (streams[g]) hipStreamDestroy(streams[g]);
    }
    free(streams); free(d_buf);
    block_free(&b);
    if (rc) {
        snprintf(msg, sizeof msg, "redistributed reads %s: %s (%s)", path, why, rc == UTREE_E_IO && errno ? strerror(errno) : utree_strerror(rc));
        utree_set_error_text(msg);
    }
    return rc;
}

/* merges the devices' handles into the first, checks that n_reads_expected reads were added (else UTREE_E_DEVICE), solves ONCE and writes the
 * redistribution's table and / or each read's redistributed label; the first failure's text stands */
static int write_redist(const utree_reports *rep, const utree_ctr *ctr, uint64_t n_reads_expected, const char *spool_path, const char *spool_err) {
    const char *path = rep->redist_path ? rep->redist_path : rep->reads_path, *what = rep->redist_path ? "redistribution" : "redistributed reads";
    int rc = UTREE_OK;
    size_t k = 0;
    uint64_t reads = 0, ambiguous = 0;
    uint32_t passes = 0;
    utree_redist_entry *e = (utree_redist_entry *)malloc(((size_t)ctr->info.n_labels + 1) * sizeof *e);
    if (!e) return UTREE_E_NOMEM;
    for (int g = 1; g < rep->n_dev && !rc; ++g) rc = utree_redist_merge(rep->dev[0].rd, rep->dev[g].rd);
    if (!rc) rc = utree_redist_reads(rep->dev[0].rd, &reads);
    char msg[400];
    if (rc == UTREE_E_DEVICE) snprintf(msg, sizeof msg, "%s %s: %s", what, path, utree_last_hip_error());
    else if (rc) snprintf(msg, sizeof msg, "%s %s: the sets could not be merged and read back (%s)", what, path, utree_strerror(rc));
    else if (reads != n_reads_expected) {                          /* every read added exactly once, or no file */
        snprintf(msg, sizeof msg, "%s %s: %llu reads added, the search read %llu", what, path, (unsigned long long)reads,
                 (unsigned long long)n_reads_expected);
        rc = UTREE_E_DEVICE;
    } else if ((rc = utree_redist_solve(rep->dev[0].rd, rep->redist_passes, e, ctr->info.n_labels, &k, &passes, &ambiguous)))
        snprintf(msg, sizeof msg, "%s %s: the passes failed (%s)", what, path, utree_strerror(rc));
    if (rc) { utree_set_error_text(msg); free(e); return rc; }
    if (rep->redist_path && (rc = utree_redist_write(ctr, e, k, reads, ambiguous, passes, path))) {
        snprintf(msg, sizeof msg, "redistribution %s: cannot write the file (%s)", path, utree_strerror(rc));
        utree_set_error_text(msg);
    }
    free(e);
    if (rep->reads_path) {
        char keep[400];
        if (rc) snprintf(keep, sizeof keep, "%s", msg);
        const int rr = write_redist_reads(rep, ctr, spool_path, spool_err);
        if (rc) utree_set_error_text(keep); else rc = rr;
    }
    return rc;
}

/* reads every device's table back, checks that n_reads_expected reads were added (else UTREE_E_DEVICE) and writes the merged file */
static int write_samples(const utree_reports *rep, const utree_ctr *ctr, uint64_t n_reads_expected) {
    const char *path = rep->samples_path;
    utree_samples_table *tabs = (utree_samples_table *)calloc((size_t)rep->n_dev, sizeof *tabs);
    if (!tabs) return UTREE_E_NOMEM;
    int rc = UTREE_OK;
    uint64_t reads = 0;
    for (int g = 0; g < rep->n_dev && !rc; ++g) {
        size_t ns = 0, nb = 0, nc = 0;
        rc = utree_samples_read(rep->dev[g].smp, NULL, 0, NULL, NULL, NULL, 0, NULL, 0, &ns, &nb, &nc, NULL);     /* the sizes */
        if (rc == UTREE_E_ARG) rc = UTREE_OK;
        if (rc) break;
        uint8_t *ids = (uint8_t *)malloc(nb ? nb : 1);
        uint64_t *w = (uint64_t *)malloc((3 * ns + 1) * 8);
        utree_samples_cell *cells = (utree_samples_cell *)malloc((nc ? nc : 1) * sizeof *cells);
        tabs[g].ids = ids; tabs[g].id_off = w; tabs[g].reads = w ? w + ns + 1 : NULL; tabs[g].unclassified = w ? w + 2 * ns + 1 : NULL; tabs[g].cells = cells;
        if (!ids || !w || !cells) { rc = UTREE_E_NOMEM; break; }
        rc = utree_samples_read(rep->dev[g].smp, ids, nb, w, w + ns + 1, w + 2 * ns + 1, ns, cells, nc, &tabs[g].n_samples, &nb, &tabs[g].n_cells,
                                &tabs[g].n_reads);
        reads += tabs[g].n_reads;
    }
    char msg[700];
    if (rc == UTREE_E_DEVICE) {                                    /* (the read-back's text begins "sample table: ") */
        const char *why = utree_last_hip_error();
        snprintf(msg, sizeof msg, "sample table %s: %s", path, strncmp(why, "sample table: ", 14) ? why : why + 14);
    }
    else if (rc) snprintf(msg, sizeof msg, "sample table %s: the tables could not be read back (%s)", path, utree_strerror(rc));
    else if (reads != n_reads_expected) {                          /* every read added exactly once, or no file */
        snprintf(msg, sizeof msg, "sample table %s: %llu reads added, the search read %llu", path, (unsigned long long)reads,
                 (unsigned long long)n_reads_expected);
        rc = UTREE_E_DEVICE;
    } else if ((rc = utree_samples_write(ctr, tabs, (size_t)rep->n_dev, path)))
        snprintf(msg, sizeof msg, "sample table %s: cannot write the file (%s)", path, utree_strerror(rc));
    if (rc) utree_set_error_text(msg);
    for (int g = 0; g < rep->n_dev; ++g) { free((void *)tabs[g].ids); free((void *)tabs[g].id_off); free((void *)tabs[g].cells); }
    free(tabs);
    return rc;
}

/* merges the devices' handles into the first, checks that n_reads_expected reads were added (else UTREE_E_DEVICE), solves every sample and writes
 * the file */
static int write_sredist(const utree_reports *rep, const utree_ctr *ctr, uint64_t n_reads_expected) {
    const char *path = rep->sredist_path;
    utree_sredist *h = rep->dev[0].srd;
    int rc = UTREE_OK;
    uint64_t reads = 0;
    size_t ns = 0, nb = 0, nc = 0, nl = 0, k = 0;
    uint8_t *ids = NULL;
    uint64_t *w = NULL;
    uint32_t *passes = NULL;
    utree_sredist_entry *e = NULL;
    for (int g = 1; g < rep->n_dev && !rc; ++g) rc = utree_sredist_merge(h, rep->dev[g].srd);
    if (!rc) rc = utree_sredist_reads(h, &reads);
    char msg[1100];
    if (!rc && reads != n_reads_expected) {                        /* every read added exactly once, or no file */
        snprintf(msg, sizeof msg, "sample redistribution %s: %llu reads added, the search read %llu", path, (unsigned long long)reads,
                 (unsigned long long)n_reads_expected);
        utree_set_error_text(msg);
        return UTREE_E_DEVICE;
    }
    if (!rc) {
        rc = utree_sredist_read(h, NULL, 0, NULL, NULL, NULL, 0, NULL, 0, NULL, 0, &ns, &nb, &nc, &nl, NULL);      /* the sizes */
        if (rc == UTREE_E_ARG) rc = UTREE_OK;
    }
    if (!rc) {
        ids = (uint8_t *)malloc(nb ? nb : 1);
        w = (uint64_t *)malloc((4 * ns + 1) * 8);                  /* id_off [ns + 1] | reads | unclassified | ambiguous */
        passes = (uint32_t *)malloc((ns ? ns : 1) * 4);
        e = (utree_sredist_entry *)malloc((nl ? nl : 1) * sizeof *e);
        utree_sredist_cell *cells = (utree_sredist_cell *)malloc((nc ? nc : 1) * sizeof *cells);
        uint32_t *labels = (uint32_t *)malloc((nl ? nl : 1) * 4);
        if (!ids || !w || !passes || !e || !cells || !labels) rc = UTREE_E_NOMEM;
        else rc = utree_sredist_read(h, ids, nb, w, w + ns + 1, w + 2 * ns + 1, ns, cells, nc, labels, nl, &ns, &nb, &nc, &nl, NULL);
        free(cells); free(labels);
    }
    if (rc == UTREE_E_DEVICE) {                                    /* (the read-back's text begins "sample redistribution:") */
        const char *why = utree_last_hip_error();
        snprintf(msg, sizeof msg, "sample redistribution %s:%s", path, strncmp(why, "sample redistribution:", 22) ? why : why + 22);
    }
    else if (rc) snprintf(msg, sizeof msg, "sample redistribution %s: the tables could not be merged and read back (%s)", path, utree_strerror(rc));
    else if ((rc = utree_sredist_solve(h, rep->redist_passes, e, nl, &k, passes, w + 3 * ns + 1, ns, NULL)))
        snprintf(msg, sizeof msg, "sample redistribution %s: the passes failed (%s)", path, utree_strerror(rc));
    else if ((rc = utree_sredist_write(ctr, ids, w, w + ns + 1, w + 2 * ns + 1, passes, w + 3 * ns + 1, ns, e, k, reads, path)))
        snprintf(msg, sizeof msg, "sample redistribution %s: cannot write the file (%s)", path, utree_strerror(rc));
    if (rc) utree_set_error_text(msg);
    free(ids); free(w); free(passes); free(e);
    return rc;
}

int utree_reports_write(utree_reports *rep, const utree_ctr *ctr, uint64_t n_reads, const char *spool_path, const char *spool_err) {
    if (!rep) return UTREE_OK;
    const int ce = rep->coverage_path ? write_coverage(rep, ctr, n_reads) : UTREE_OK;
    char keep[1200];
    const int re = rep->redist_path || rep->reads_path ? write_redist(rep, ctr, n_reads, spool_path, spool_err) : UTREE_OK;
    if (re) snprintf(keep, sizeof keep, "%s", utree_last_hip_error());
    const int se = rep->samples_path ? write_samples(rep, ctr, n_reads) : UTREE_OK;
    if (se && !re) snprintf(keep, sizeof keep, "%s", utree_last_hip_error());          /* (the redistribution's failure wins) */
    const int sre = rep->sredist_path ? write_sredist(rep, ctr, n_reads) : UTREE_OK;
    if (sre && !re && !se) snprintf(keep, sizeof keep, "%s", utree_last_hip_error());  /* (... then the sample table's) */
    if (rep->profile_path && write_profile(rep, ctr, n_reads)) return UTREE_E_PROFILE;
    if (re || se || sre) { utree_set_error_text(keep); return UTREE_E_PROFILE; }      /* (no code of their own; a profile that was written sets no text) */
    return ce ? UTREE_E_COVERAGE : UTREE_OK;      /* (a profile that was written sets no text: the coverage's stands) */
}
