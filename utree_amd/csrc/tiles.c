/* tiles.c -- long queries tile by tile (include/utree_amd.h: utree_tiles_*): argument checks, the workspace and the launches of
 * tiles_kernels.hip on the caller's stream, and the host formatters of the two files' lines.  The whole run is tiles_file.c. */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ctr_host.h"
#include "dev_image.h"
#include "tiles.h"

static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
static int params_ok(uint32_t W, uint32_t S) { return S >= 1 && S <= W && W <= UTREE_TILE_MAX_BP; }

/* the arrays of utk_tiles_ws behind `base` (NULL: only their size); returns the bytes they take */
static size_t carve(utk_tiles_ws *w, char *base, uint32_t n_reads) {
    memset(w, 0, sizeof *w);
    w->tcnt = (uint64_t *)base;
    const size_t at = up256(((size_t)n_reads + 1) * sizeof(uint64_t));
    w->scan_tmp_bytes = utk_tiles_scan_temp_bytes(n_reads);
    w->scan_tmp = base ? base + at : NULL;
    if (!w->scan_tmp_bytes) return 0;
    return at + up256(w->scan_tmp_bytes);
}

size_t utree_tiles_workspace_bytes(const utree_dev *dev, uint32_t n_reads) {
    utk_tiles_ws w;
    if (!dev) return 0;
    return carve(&w, NULL, n_reads) + 256;                                      /* (+ the alignment of the caller's pointer) */
}

int utree_tiles_plan(utree_dev *dev, const uint32_t *d_len, uint32_t n_reads, uint32_t tile_bp, uint32_t step_bp, uint64_t *d_tile_first,
                     utree_tiles_meta *d_meta, void *d_workspace, size_t workspace_bytes, void *stream) {
    if (!dev || !d_tile_first || !d_meta || !d_workspace || (n_reads && !d_len) || !params_ok(tile_bp, step_bp)) return UTREE_E_ARG;
    utk_tiles_ws w;
    char *base = (char *)(((uintptr_t)d_workspace + 255) & ~(uintptr_t)255);
    const size_t need = carve(&w, base, n_reads);
    /* what utree_tiles_workspace_bytes said, wherever the pointer lies: a caller one byte short is told so on every run, not only on those
     * whose allocation happens to need the whole alignment slack */
    if (!need || workspace_bytes < need + 256) return UTREE_E_ARG;
    if (hipSetDevice(dev->device) != hipSuccess) { utree_dev_set_hip_error((int)hipGetLastError(), "utree_tiles_plan: hipSetDevice"); return UTREE_E_HIP; }
    const int e = utk_tiles_plan(d_len, n_reads, tile_bp, step_bp, d_tile_first, d_meta, &w, stream);
    if (e) { utree_dev_set_hip_error(e, "utree_tiles_plan"); return UTREE_E_HIP; }
    return UTREE_OK;
}

int utree_tiles_views(utree_dev *dev, const uint64_t *d_off, const uint32_t *d_len, uint32_t n_reads, uint32_t tile_bp, uint32_t step_bp,
                      const uint64_t *d_tile_first, uint64_t first_tile, uint32_t n_tiles, uint64_t *d_toff, uint32_t *d_tlen,
                      uint32_t *d_tquery, uint32_t *d_tindex, utree_tiles_meta *d_meta, void *stream) {
    if (!dev || !d_tile_first || !d_meta || !params_ok(tile_bp, step_bp) || n_tiles > UTREE_TILES_MAX_BATCH) return UTREE_E_ARG;
    if (n_reads && (!d_off || !d_len)) return UTREE_E_ARG;
    if (n_tiles && (!d_toff || !d_tlen || !d_tquery || !d_tindex)) return UTREE_E_ARG;
    if (hipSetDevice(dev->device) != hipSuccess) { utree_dev_set_hip_error((int)hipGetLastError(), "utree_tiles_views: hipSetDevice"); return UTREE_E_HIP; }
    const int e = utk_tiles_views(d_off, d_len, n_reads, tile_bp, step_bp, d_tile_first, first_tile, n_tiles, d_toff, d_tlen, d_tquery, d_tindex, d_meta,
                                  stream);
    if (e) { utree_dev_set_hip_error(e, "utree_tiles_views"); return UTREE_E_HIP; }
    return UTREE_OK;
}

/* ---- host: the two files' lines ------------------------------------------------------------------------------------------------------ */
static size_t put_u64(char *dst, uint64_t v) {
    char t[24];
    size_t n = 0;
    do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    for (size_t i = 0; i < n; ++i) dst[i] = t[n - 1 - i];
    return n;
}

/* tile t of a query of L bases: its first and last base, 1-based (an empty query's one tile: 1 and 0) */
static void tile_span(uint64_t L, uint32_t W, uint32_t S, uint32_t t, uint64_t *start, uint64_t *end) {
    const uint64_t a = (uint64_t)t * S;
    *start = a + 1;
    *end = a + W < L ? a + W : L;
}

/* Where a line of at most `room` bytes is put together: in place when that much is left behind h_out[at], else in a block of its own, from
 * which line_done copies what the line really took -- so a cap is too small exactly when the text does not fit, never because of the slack. */
static char *line_begin(char *h_out, size_t at, size_t cap, size_t room, char **tmp) {
    *tmp = NULL;
    if (at <= cap && room <= cap - at) return h_out + at;
    return *tmp = (char *)malloc(room);
}
static size_t line_done(char *h_out, size_t at, size_t cap, char *tmp, size_t len) {
    if (!tmp) return len;
    const int fits = at <= cap && len <= cap - at;
    if (fits) memcpy(h_out + at, tmp, len);
    free(tmp);
    return fits ? len : (size_t)-1;
}

size_t utree_tiles_format(const utree_ctr *ctr, const uint8_t *h_buf, const uint64_t *name_off, const uint32_t *name_len,
                          const uint32_t *seq_len, uint32_t tile_bp, uint32_t step_bp, const uint32_t *tquery, const uint32_t *tindex,
                          const utree_result *h_res, size_t n, char *h_out, size_t cap, uint64_t *classified) {
    size_t at = 0;
    uint64_t lines = 0;
    for (size_t j = 0; j < n; ++j) {
        const utree_result *r = &h_res[j];
        if (!r->found) continue;                                                /* itree.c:1028: no hit, no line */
        const uint32_t q = tquery[j];
        const char *lab;
        const size_t ll = utk_record_taxon(ctr, r, &lab);
        if (ll == (size_t)-1) return (size_t)-1;
        char *tmp, *o = line_begin(h_out, at, cap, (size_t)name_len[q] + 44 + ll + UTK_RECORD_TAIL_MAX, &tmp);   /* (":", "-" and two numbers of at most 20 digits) */
        if (!o) return (size_t)-1;
        const char *o0 = o;
        uint64_t start, end;
        tile_span(seq_len[q], tile_bp, step_bp, tindex[j], &start, &end);
        memcpy(o, h_buf + name_off[q], name_len[q]); o += name_len[q];
        *o++ = ':'; o += put_u64(o, start);
        *o++ = '-'; o += put_u64(o, end);
        o = utk_record_tail(lab, ll, r, o);
        const size_t w = line_done(h_out, at, cap, tmp, (size_t)(o - o0));
        if (w == (size_t)-1) return (size_t)-1;
        at += w;
        ++lines;
    }
    if (classified) *classified += lines;
    return at;
}

/* the line of a closed run behind h_out[at]; bytes written, or (size_t)-1 */
static size_t put_run(const utree_ctr *ctr, const uint8_t *h_buf, const uint64_t *name_off, const uint32_t *name_len, const utree_tiles_run *s,
                      char *h_out, size_t at, size_t cap) {
    const size_t tl = s->classified ? (size_t)s->taxon_len : 0;
    char *tmp, *out = line_begin(h_out, at, cap, (size_t)name_len[s->query] + tl + 4 * 21 + 8, &tmp);
    if (!out) return (size_t)-1;
    size_t w = 0;
    memcpy(out, h_buf + name_off[s->query], name_len[s->query]); w += name_len[s->query];
    out[w++] = '\t'; w += put_u64(out + w, s->start);
    out[w++] = '\t'; w += put_u64(out + w, s->end);
    out[w++] = '\t'; w += put_u64(out + w, s->n_tiles);
    out[w++] = '\t'; out[w++] = s->classified ? 'C' : 'U';
    out[w++] = '\t';
    if (tl) { memcpy(out + w, ctr->labels[s->label], tl); w += tl; }
    out[w++] = '\t'; w += put_u64(out + w, s->found);
    out[w++] = '\n';
    return line_done(h_out, at, cap, tmp, w);
}

size_t utree_tiles_segments_format(const utree_ctr *ctr, const uint8_t *h_buf, const uint64_t *name_off, const uint32_t *name_len,
                                   const uint32_t *seq_len, uint32_t tile_bp, uint32_t step_bp, const uint32_t *tquery,
                                   const uint32_t *tindex, const utree_result *h_res, size_t n, int flush, utree_tiles_run *state,
                                   char *h_out, size_t cap, uint64_t *segments) {
    utree_tiles_run s = *state;                                                 /* committed at the end: a call that fails changes nothing */
    size_t at = 0;
    uint64_t lines = 0;
    for (size_t j = 0; j < n; ++j) {
        const utree_result *r = &h_res[j];
        const uint32_t q = tquery[j], cls = r->found != 0;
        const char *lab = NULL;
        size_t ll = 0;
        if (cls && (ll = utk_record_taxon(ctr, r, &lab)) == (size_t)-1) return (size_t)-1;
        uint64_t start, end;
        tile_span(seq_len[q], tile_bp, step_bp, tindex[j], &start, &end);
        /* equal class: both unclassified, or the same taxon TEXT (two labels may print one text; the empty taxon is a class of its own) */
        const int same = s.open && s.query == q && s.classified == cls &&
                         (!cls || (s.taxon_len == ll && !memcmp(ctr->labels[s.label], lab, ll)));
        if (same) { s.end = end; ++s.n_tiles; s.found += r->found; continue; }
        if (s.open) {
            const size_t w = put_run(ctr, h_buf, name_off, name_len, &s, h_out, at, cap);
            if (w == (size_t)-1) return (size_t)-1;
            at += w; ++lines;
        }
        s.open = 1; s.query = q; s.start = start; s.end = end; s.n_tiles = 1; s.found = r->found;
        s.classified = cls; s.label = cls ? r->label : 0; s.taxon_len = ll;
    }
    if (flush && s.open) {
        const size_t w = put_run(ctr, h_buf, name_off, name_len, &s, h_out, at, cap);
        if (w == (size_t)-1) return (size_t)-1;
        at += w; ++lines;
        memset(&s, 0, sizeof s);
    }
    *state = s;
    if (segments) *segments += lines;
    return at;
}
