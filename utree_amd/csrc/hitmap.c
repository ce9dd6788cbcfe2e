/* hitmap.c -- the per-query k-mer hit map (include/utree_amd.h: utree_hitmap_*): argument checks, the workspace and the launches of
 * hitmap_kernels.hip on the caller's stream, and the host formatter of the map's lines. */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <string.h>
#include "dev_image.h"
#include "hitmap.h"

static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

/* the arrays of utk_hitmap_ws behind `base` (NULL: only their size); returns the bytes they take */
static size_t carve(utk_hitmap_ws *w, char *base, uint32_t n_reads, uint64_t total_bases, int do_rc) {
    size_t at = 0;
    const size_t nr1 = (size_t)n_reads + 1;
    memset(w, 0, sizeof *w);
    w->wcap = utk_hitmap_wcap(n_reads, total_bases, do_rc);
    w->n_groups = utk_hitmap_groups(w->wcap);
    const size_t ng1 = (size_t)w->n_groups + 1;
#define TAKE(field, type, count) do { w->field = (type *)(base ? base + at : NULL); at += up256((size_t)(count) * sizeof(type)); } while (0)
    TAKE(flag, unsigned int, 1);
    TAKE(wcnt, uint64_t, nr1); TAKE(woff, uint64_t, nr1); TAKE(icnt, uint64_t, nr1); TAKE(ioff, uint64_t, nr1);
    TAKE(gcnt, uint64_t, ng1); TAKE(gbase, uint64_t, ng1); TAKE(gfirst, uint64_t, ng1); TAKE(gnext, uint64_t, ng1);
    TAKE(starts, uint32_t, (w->wcap >> 5) + 2);
    TAKE(codes, uint32_t, w->wcap + 1);
#undef TAKE
    w->scan_tmp_bytes = utk_hitmap_scan_temp_bytes(n_reads, w->n_groups);
    w->scan_tmp = base ? base + at : NULL;
    if (!w->scan_tmp_bytes) return 0;
    return at + up256(w->scan_tmp_bytes);
}

size_t utree_hitmap_workspace_bytes(const utree_dev *dev, uint32_t n_reads, uint64_t total_bases, int do_rc) {
    utk_hitmap_ws w;
    if (!dev) return 0;
    return carve(&w, NULL, n_reads, total_bases, do_rc) + 256;                  /* (+ the alignment of the caller's pointer) */
}

int utree_hitmap_batch(utree_dev *dev, const uint8_t *d_bases, const uint64_t *d_off, const uint32_t *d_len, uint32_t n_reads, uint64_t total_bases,
                       int do_rc, uint64_t *d_run_off, utree_hit_run *d_runs, uint64_t run_capacity, utree_hitmap_meta *d_meta, void *d_workspace,
                       size_t workspace_bytes, void *stream) {
    if (!dev || !d_run_off || !d_meta || !d_workspace || (run_capacity && !d_runs)) return UTREE_E_ARG;
    if (n_reads && (!d_off || !d_len || (total_bases && !d_bases))) return UTREE_E_ARG;
    if (dev->hdr.n_labels > UTREE_HIT_INVALID) return UTREE_E_UNSUPPORTED;       /* (a label index would read as a code) */
    utk_hitmap_ws w;
    char *base = (char *)(((uintptr_t)d_workspace + 255) & ~(uintptr_t)255);
    const size_t need = carve(&w, base, n_reads, total_bases, do_rc);
    if (!need || (size_t)(base - (char *)d_workspace) + need > workspace_bytes) return UTREE_E_ARG;
    if (hipSetDevice(dev->device) != hipSuccess) { utree_dev_set_hip_error((int)hipGetLastError(), "utree_hitmap_batch: hipSetDevice"); return UTREE_E_HIP; }
    const int e = utk_hitmap_run(&dev->kimg, d_bases, d_off, d_len, n_reads, total_bases, do_rc, d_run_off, d_runs, run_capacity, d_meta, &w, dev->n_cu,
                                 stream);
    if (e) { utree_dev_set_hip_error(e, "utree_hitmap_batch"); return UTREE_E_HIP; }
    return UTREE_OK;
}

/* ---- host: the map's lines ---------------------------------------------------------------------------------------------------------- */
static size_t put_u64(char *dst, uint64_t v) {
    char t[24];
    size_t n = 0;
    do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    for (size_t i = 0; i < n; ++i) dst[i] = t[n - 1 - i];
    return n;
}

size_t utree_hitmap_format(const uint8_t *h_buf, const uint64_t *name_off, const uint32_t *name_len, const uint64_t *h_run_off,
                           const utree_hit_run *h_runs, size_t n, char *h_out, size_t cap) {
    size_t at = 0;
    char tok[48];
    for (size_t i = 0; i < n; ++i) {
        const uint64_t a = h_run_off[i], b = h_run_off[i + 1];
        uint64_t windows = 0, found = 0;
        for (uint64_t j = a; j < b; ++j) {
            windows += h_runs[j].count;
            if (h_runs[j].code < UTREE_HIT_INVALID) found += h_runs[j].count;
        }
        if (at + name_len[i] > cap) return (size_t)-1;
        memcpy(h_out + at, h_buf + name_off[i], name_len[i]); at += name_len[i];
        size_t t = 0;
        tok[t++] = '\t'; t += put_u64(tok + t, windows);
        tok[t++] = '\t'; t += put_u64(tok + t, found);
        tok[t++] = '\t';
        if (at + t > cap) return (size_t)-1;
        memcpy(h_out + at, tok, t); at += t;
        for (uint64_t j = a; j < b; ++j) {
            t = 0;
            if (j > a) tok[t++] = ' ';
            if (h_runs[j].code == UTREE_HIT_MISS) tok[t++] = '-';
            else if (h_runs[j].code == UTREE_HIT_INVALID) tok[t++] = 'N';
            else t += put_u64(tok + t, h_runs[j].code);
            tok[t++] = ':'; t += put_u64(tok + t, h_runs[j].count);
            if (at + t > cap) return (size_t)-1;
            memcpy(h_out + at, tok, t); at += t;
        }
        if (at + 1 > cap) return (size_t)-1;
        h_out[at++] = '\n';
    }
    return at;
}
