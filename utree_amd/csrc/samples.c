/* samples.c -- per-sample taxon tables of multiplexed reads (include/utree_amd.h: utree_samples_*).
 *
 * A combined reads file names its records <sample>_<n>; a read's sample id is its name up to the last delimiter byte, its taxon the second
 * column of its output line.  The ids are interned and the (sample, taxon) cells counted on the device while the chunk is there
 * (samples_kernels.hip); here the handle, the read-back -- sample ids, per-sample reads / unclassified, cells keyed (sample, label, cut) -- and the
 * host-only writer, which merges any number of read-backs: samples by id text, taxa by printed text, exactly as utree_profile_write merges.
 */
#define _GNU_SOURCE
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ctr_host.h"
#include "dev_image.h"
#include "samples.h"

struct utree_samples {
    int device, n_cu;
    uint32_t id_slots, cell_slots;      /* powers of two */
    uint8_t *d_mem;                     /* ids | reads | uncl | cells | misc | index | arena */
    size_t bytes, counters_bytes;       /* counters_bytes: everything in front of the arena  */
    utk_samples_tab tab;
};

static void flags_text(unsigned long long f, char *msg, size_t cap) {
    snprintf(msg, cap, "sample table:%s%s%s%s%s%s",
             f & UTK_SAMPLES_F_TABLE ? " more distinct sample ids than the table holds (raise UTREE_SAMPLE_CAPACITY; is the delimiter right?);" : "",
             f & UTK_SAMPLES_F_ARENA ? " the arena of id bytes is used up (raise UTREE_SAMPLE_CAPACITY; is the delimiter right?);" : "",
             f & UTK_SAMPLES_F_CELLS ? " the table of (sample, taxon) cells is full (raise UTREE_SAMPLE_CELLS);" : "",
             f & UTK_SAMPLES_F_LABEL ? " a record names a label the database does not have;" : "",
             f & UTK_SAMPLES_F_NAME ? " a name lies outside its chunk;" : "",
             f & UTK_SAMPLES_F_CUT ? " a taxon of more than 65532 bytes;" : "");
    const size_t l = strlen(msg);
    if (l && msg[l - 1] == ';') msg[l - 1] = 0;
}

int utree_samples_create(utree_dev *dev, uint32_t sample_capacity, uint32_t cell_capacity, int delim, utree_samples **out) {
    if (!dev || !out) return UTREE_E_ARG;
    *out = NULL;
    if (!sample_capacity || sample_capacity > (1u << (UTK_SAMPLES_SLOT_BITS - 1)) || !cell_capacity || cell_capacity > (1u << 30)) return UTREE_E_ARG;
    if (delim < 0 || delim > 255 || delim == '\t' || delim == ' ' || delim == '\r' || delim == '\n') return UTREE_E_ARG;
    if (dev->hdr.n_labels >= (1ull << UTK_SAMPLES_LABEL_BITS)) return UTREE_E_UNSUPPORTED;       /* the packed cell key has 28 bits for the label */
    utree_samples *s = (utree_samples *)calloc(1, sizeof *s);
    if (!s) return UTREE_E_NOMEM;
    s->device = dev->device; s->n_cu = dev->n_cu;
    s->id_slots = 16; s->cell_slots = 16;
    while (s->id_slots < 2 * sample_capacity) s->id_slots <<= 1;          /* at most half full: short probe chains */
    while (s->cell_slots < cell_capacity) s->cell_slots <<= 1;
    uint64_t arena = (uint64_t)sample_capacity * UTK_SAMPLES_ARENA_PER_SAMPLE;
    if (arena < (1u << 20)) arena = 1u << 20;
    if (arena > 0xFFFFFF00ull) arena = 0xFFFFFF00ull;                     /* a key holds the offset in 32 bits */
    const size_t ids = (size_t)s->id_slots * 8, cells = 2 * (size_t)s->cell_slots * 8, misc = UTK_SAMPLES_MISC_WORDS * 8, index = (size_t)s->id_slots * 4;
    s->counters_bytes = 3 * ids + cells + misc + index;
    s->bytes = s->counters_bytes + (size_t)arena;
    if (hipSetDevice(s->device) != hipSuccess) { free(s); return UTREE_E_HIP; }
    if (hipMalloc((void **)&s->d_mem, s->bytes) != hipSuccess) { (void)hipGetLastError(); free(s); return UTREE_E_NOMEM; }
    utk_samples_tab *t = &s->tab;
    t->ids = (unsigned long long *)s->d_mem; t->reads = t->ids + s->id_slots; t->uncl = t->reads + s->id_slots;
    t->cells = t->uncl + s->id_slots; t->misc = t->cells + 2 * (size_t)s->cell_slots;
    t->index = (uint32_t *)(t->misc + UTK_SAMPLES_MISC_WORDS); t->arena = (uint8_t *)(t->index + s->id_slots);
    t->arena_cap = arena; t->id_mask = s->id_slots - 1; t->cell_mask = s->cell_slots - 1; t->sample_cap = sample_capacity;
    t->n_labels = (uint32_t)dev->hdr.n_labels; t->delim = (uint32_t)delim;
    int rc = utree_samples_reset(s);
    if (rc) { utree_samples_free(s); return rc; }
    *out = s;
    return UTREE_OK;
}

int utree_samples_reset(utree_samples *s) {
    if (!s) return UTREE_E_ARG;
    if (hipSetDevice(s->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return UTREE_E_HIP;   /* adds in flight on any stream */
    if (hipMemset(s->d_mem, 0, s->counters_bytes) != hipSuccess) return UTREE_E_HIP;                          /* (the arena is written before it is read) */
    if (hipMemset(s->tab.cells, 0xFF, 2 * (size_t)s->cell_slots * 8) != hipSuccess) return UTREE_E_HIP;       /* every cell key free (all ones) ... */
    if (hipMemset2D(s->tab.cells + 1, 16, 0, 8, s->cell_slots) != hipSuccess) return UTREE_E_HIP;             /* ... and every count zero           */
    return hipDeviceSynchronize() == hipSuccess ? UTREE_OK : UTREE_E_HIP;
}

int utree_samples_add(utree_samples *s, const uint8_t *d_text, uint64_t text_bytes, const uint32_t *d_name_off, const uint32_t *d_name_len,
                      const utree_result *d_res, uint32_t n_reads, void *stream) {
    if (!s || (n_reads && (!d_name_off || !d_name_len || !d_res || (!d_text && text_bytes)))) return UTREE_E_ARG;
    if (!n_reads) return UTREE_OK;
    if (hipSetDevice(s->device) != hipSuccess) return UTREE_E_HIP;
    return utk_samples_add(&s->tab, d_text, text_bytes, d_name_off, d_name_len, d_res, n_reads, s->n_cu, stream) ? UTREE_E_HIP : UTREE_OK;
}

void utree_samples_free(utree_samples *s) {
    if (!s) return;
    if (s->d_mem) { hipSetDevice(s->device); hipDeviceSynchronize(); hipFree(s->d_mem); }
    free(s);
}

int utree_samples_read(utree_samples *s, uint8_t *h_ids, size_t id_cap, uint64_t *h_id_off, uint64_t *h_reads, uint64_t *h_unclassified,
                       size_t sample_cap, utree_samples_cell *h_cells, size_t cell_cap, size_t *n_samples, size_t *n_id_bytes, size_t *n_cells,
                       uint64_t *n_reads) {
    if (!s || !n_samples || !n_id_bytes || !n_cells || (id_cap && !h_ids) || (sample_cap && (!h_id_off || !h_reads || !h_unclassified)) ||
        (cell_cap && !h_cells)) return UTREE_E_ARG;
    *n_samples = 0; *n_id_bytes = 0; *n_cells = 0;
    if (n_reads) *n_reads = 0;
    uint8_t *m = (uint8_t *)malloc(s->counters_bytes), *arena = NULL;
    uint32_t *slot_of = NULL;                                       /* dense index -> slot */
    if (!m) return UTREE_E_NOMEM;
    int rc = UTREE_OK;
    char msg[512];
    if (hipSetDevice(s->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(m, s->d_mem, s->counters_bytes, hipMemcpyDeviceToHost) != hipSuccess) { free(m); return UTREE_E_HIP; }
    const unsigned long long *ids = (const unsigned long long *)m, *reads = ids + s->id_slots, *uncl = reads + s->id_slots,
                             *cells = uncl + s->id_slots, *misc = cells + 2 * (size_t)s->cell_slots;
    const uint32_t *index = (const uint32_t *)(misc + UTK_SAMPLES_MISC_WORDS);
    if (n_reads) *n_reads = misc[0];
    if (misc[1]) { flags_text(misc[1], msg, sizeof msg); utree_set_error_text(msg); rc = UTREE_E_DEVICE; goto done; }
    const uint64_t S = misc[3], used = misc[2];
    if (S > s->tab.sample_cap || used > s->tab.arena_cap) { utree_set_error_text("sample table: the counters of the id table are inconsistent"); rc = UTREE_E_DEVICE; goto done; }
    slot_of = (uint32_t *)malloc((S ? S : 1) * sizeof *slot_of);
    arena = (uint8_t *)malloc(used ? used : 1);
    if (!slot_of || !arena) { rc = UTREE_E_NOMEM; goto done; }
    if (used && hipMemcpy(arena, s->tab.arena, used, hipMemcpyDeviceToHost) != hipSuccess) { rc = UTREE_E_HIP; goto done; }
    for (uint64_t i = 0; i < S; ++i) slot_of[i] = 0xFFFFFFFFu;
    uint64_t claimed = 0, id_bytes = 0;
    for (uint32_t k = 0; k < s->id_slots; ++k) {
        if (!ids[k]) continue;
        const uint64_t at = ids[k] >> 32, len = (uint32_t)ids[k] - 1u;
        if (index[k] >= S || slot_of[index[k]] != 0xFFFFFFFFu || at + len > used) {
            utree_set_error_text("sample table: a slot of the id table is inconsistent"); rc = UTREE_E_DEVICE; goto done;
        }
        slot_of[index[k]] = k; ++claimed; id_bytes += len;
    }
    if (claimed != S) { utree_set_error_text("sample table: the id table holds another number of ids than were claimed"); rc = UTREE_E_DEVICE; goto done; }
    size_t nc = 0;
    for (uint32_t c = 0; c < s->cell_slots; ++c) nc += cells[2 * (size_t)c] != ~0ull && cells[2 * (size_t)c + 1];
    *n_samples = (size_t)S; *n_id_bytes = (size_t)id_bytes; *n_cells = nc;
    if (S > sample_cap || id_bytes > id_cap || nc > cell_cap) { rc = UTREE_E_ARG; goto done; }       /* the sizes are set: call again with room */
    uint64_t w = 0;
    for (uint64_t i = 0; i < S; ++i) {
        const uint32_t k = slot_of[i];
        const uint64_t at = ids[k] >> 32, len = (uint32_t)ids[k] - 1u;
        h_id_off[i] = w;
        if (len) memcpy(h_ids + w, arena + at, len);
        w += len;
        h_reads[i] = reads[k]; h_unclassified[i] = uncl[k];
    }
    if (h_id_off) h_id_off[S] = w;                                  /* (sample_cap + 1 entries) */
    uint64_t *sum = (uint64_t *)calloc(S ? S : 1, 8);               /* per sample: reads = unclassified + its cells, or the table is not written */
    if (!sum) { rc = UTREE_E_NOMEM; goto done; }
    size_t q = 0;
    for (uint32_t c = 0; c < s->cell_slots; ++c) {
        const unsigned long long key = cells[2 * (size_t)c], cnt = cells[2 * (size_t)c + 1];
        if (key == ~0ull || !cnt) continue;
        const uint32_t slot = (uint32_t)(key >> (UTK_SAMPLES_LABEL_BITS + 16u)), cut = (uint32_t)(key & 0xFFFFu);
        if (slot >= s->id_slots || !ids[slot]) { free(sum); utree_set_error_text("sample table: a cell names no sample"); rc = UTREE_E_DEVICE; goto done; }
        h_cells[q].sample = index[slot];
        h_cells[q].label = (uint32_t)(key >> 16) & ((1u << UTK_SAMPLES_LABEL_BITS) - 1u);
        h_cells[q].cut = cut == UTK_SAMPLES_CUT_WHOLE ? -2 : cut == UTK_SAMPLES_CUT_EMPTY ? -1 : (int32_t)cut;
        h_cells[q].pad = 0; h_cells[q].reads = cnt;
        sum[index[slot]] += cnt;
        ++q;
    }
    uint64_t total = 0;
    for (uint64_t i = 0; i < S && !rc; ++i) {
        total += h_reads[i];
        if (h_reads[i] != h_unclassified[i] + sum[i]) rc = UTREE_E_DEVICE;
    }
    if (!rc && total != misc[0]) rc = UTREE_E_DEVICE;
    if (rc) utree_set_error_text("sample table: the samples' reads do not add up to the records added");
    free(sum);
done:
    free(m); free(arena); free(slot_of);
    return rc;
}

/* ---- host: any number of read-backs -> one table ----------------------------------------------------------------------------- */
typedef struct { const uint8_t *s; uint64_t len; uint64_t reads, uncl; size_t tab; uint32_t sample; uint32_t col; } smp_t;
typedef struct { const char *s; uint32_t len; uint32_t col; uint64_t reads; } cell_t;

static int text_cmp(const void *a, uint64_t la, const void *b, uint64_t lb) {
    const uint64_t m = la < lb ? la : lb;
    const int c = m ? memcmp(a, b, m) : 0;
    if (c) return c;
    return la < lb ? -1 : la > lb;
}
static int smp_cmp(const void *a, const void *b) {
    const smp_t *x = (const smp_t *)a, *y = (const smp_t *)b;
    return text_cmp(x->s, x->len, y->s, y->len);
}
static int smp_back_cmp(const void *a, const void *b) {                /* back into (read-back, sample) order */
    const smp_t *x = (const smp_t *)a, *y = (const smp_t *)b;
    if (x->tab != y->tab) return x->tab < y->tab ? -1 : 1;
    return x->sample < y->sample ? -1 : x->sample > y->sample;
}
static int cell_cmp(const void *a, const void *b) {
    const cell_t *x = (const cell_t *)a, *y = (const cell_t *)b;
    const int c = text_cmp(x->s, x->len, y->s, y->len);
    if (c) return c;
    return x->col < y->col ? -1 : x->col > y->col;
}
static int put_id(FILE *f, const uint8_t *s, uint64_t len) {           /* TAB, CR and backslash escaped, nothing else */
    for (uint64_t i = 0; i < len; ++i) {
        const int c = s[i];
        const int r = c == '\t' ? fputs("\\t", f) : c == '\r' ? fputs("\\r", f) : c == '\\' ? fputs("\\\\", f) : fputc(c, f);
        if (r == EOF) return 1;
    }
    return 0;
}

int utree_samples_write(const utree_ctr *ctr, const utree_samples_table *tabs, size_t n_tabs, const char *path) {
    if (!ctr || (n_tabs && !tabs) || !path) return UTREE_E_ARG;
    size_t ns = 0, nc = 0;
    uint64_t N = 0;
    for (size_t t = 0; t < n_tabs; ++t) {
        if ((tabs[t].n_samples && (!tabs[t].id_off || !tabs[t].reads || !tabs[t].unclassified)) || (tabs[t].n_cells && !tabs[t].cells)) return UTREE_E_ARG;
        ns += tabs[t].n_samples; nc += tabs[t].n_cells; N += tabs[t].n_reads;
    }
    smp_t *sm = (smp_t *)calloc(ns ? ns : 1, sizeof *sm);
    cell_t *ce = (cell_t *)calloc(nc ? nc : 1, sizeof *ce);
    size_t *first = (size_t *)calloc(n_tabs + 1, sizeof *first);        /* read-back t's samples are sm[first[t] ..] once sorted back */
    uint64_t *col_reads = NULL, *col_uncl = NULL, *col_sum = NULL;
    const uint8_t **col_s = NULL; uint64_t *col_len = NULL;
    int rc = UTREE_OK;
    FILE *f = NULL;
    if (!sm || !ce || !first) { rc = UTREE_E_NOMEM; goto done; }
    size_t k = 0;
    for (size_t t = 0; t < n_tabs; ++t) {
        first[t] = k;
        for (size_t i = 0; i < tabs[t].n_samples; ++i, ++k) {
            if (tabs[t].id_off[i + 1] < tabs[t].id_off[i]) { rc = UTREE_E_ARG; goto done; }
            sm[k].len = tabs[t].id_off[i + 1] - tabs[t].id_off[i];
            sm[k].s = sm[k].len ? tabs[t].ids + tabs[t].id_off[i] : (const uint8_t *)"";
            sm[k].reads = tabs[t].reads[i]; sm[k].uncl = tabs[t].unclassified[i]; sm[k].tab = t; sm[k].sample = (uint32_t)i;
        }
    }
    /* the columns: one per distinct id text, in unsigned bytewise order (shorter first) */
    qsort(sm, ns, sizeof *sm, smp_cmp);
    size_t S = 0;
    for (size_t i = 0; i < ns; ++i) {
        if (i && smp_cmp(&sm[i - 1], &sm[i])) ++S;
        sm[i].col = (uint32_t)S;
    }
    if (ns) ++S;
    col_reads = (uint64_t *)calloc(S ? S : 1, 8); col_uncl = (uint64_t *)calloc(S ? S : 1, 8); col_sum = (uint64_t *)calloc(S ? S : 1, 8);
    col_s = (const uint8_t **)calloc(S ? S : 1, sizeof *col_s); col_len = (uint64_t *)calloc(S ? S : 1, 8);
    if (!col_reads || !col_uncl || !col_sum || !col_s || !col_len) { rc = UTREE_E_NOMEM; goto done; }
    uint64_t total = 0;
    for (size_t i = 0; i < ns; ++i) {
        col_reads[sm[i].col] += sm[i].reads; col_uncl[sm[i].col] += sm[i].uncl; col_s[sm[i].col] = sm[i].s; col_len[sm[i].col] = sm[i].len;
        total += sm[i].reads;
    }
    if (total != N) { rc = UTREE_E_ARG; goto done; }                     /* the samples' reads are the reads */
    qsort(sm, ns, sizeof *sm, smp_back_cmp);
    /* the cells: the text each prints (utree_profile_write's rule), its column; merged by both */
    size_t q = 0;
    uint64_t G = 0;
    for (size_t t = 0; t < n_tabs; ++t)
        for (size_t i = 0; i < tabs[t].n_cells; ++i) {
            const utree_samples_cell *c = &tabs[t].cells[i];
            if (!c->reads) continue;
            if (c->sample >= tabs[t].n_samples) { rc = UTREE_E_ARG; goto done; }
            uint32_t len = 0;
            const char *s = "";
            if (c->cut != -1) {
                if (c->label >= ctr->info.n_labels) { rc = UTREE_E_ARG; goto done; }
                s = ctr->labels[c->label];
                len = ctr->label_len[c->label];
                if (c->cut >= 0 && (uint32_t)c->cut < len) len = (uint32_t)c->cut;
            }
            ce[q].s = s; ce[q].len = len; ce[q].col = sm[first[t] + c->sample].col; ce[q].reads = c->reads;
            G += c->reads;
            ++q;
        }
    qsort(ce, q, sizeof *ce, cell_cmp);
    size_t w = 0;
    for (size_t i = 0; i < q; ++i) {
        if (w && !cell_cmp(&ce[w - 1], &ce[i])) ce[w - 1].reads += ce[i].reads;
        else ce[w++] = ce[i];
    }
    for (size_t i = 0; i < w; ++i) col_sum[ce[i].col] += ce[i].reads;
    for (size_t j = 0; j < S; ++j)
        if (col_uncl[j] > col_reads[j] || col_sum[j] != col_reads[j] - col_uncl[j]) { rc = UTREE_E_ARG; goto done; }   /* column j sums to n_j - u_j */
    f = fopen(path, "wb");
    if (!f) { rc = UTREE_E_IO; goto done; }
    int bad = fprintf(f, "# reads\t%llu\tclassified\t%llu\tunclassified\t%llu\tsamples\t%llu\n", (unsigned long long)N, (unsigned long long)G,
                      (unsigned long long)(N - G), (unsigned long long)S) < 0;
    bad |= fputs("# taxon", f) < 0;
    for (size_t j = 0; j < S && !bad; ++j) bad = fputc('\t', f) == EOF || put_id(f, col_s[j], col_len[j]);
    bad |= fputs("\n# reads", f) < 0;
    for (size_t j = 0; j < S && !bad; ++j) bad = fprintf(f, "\t%llu", (unsigned long long)col_reads[j]) < 0;
    bad |= fputs("\n# unclassified", f) < 0;
    for (size_t j = 0; j < S && !bad; ++j) bad = fprintf(f, "\t%llu", (unsigned long long)col_uncl[j]) < 0;
    bad |= fputc('\n', f) == EOF;
    for (size_t i = 0; i < w && !bad;) {                                 /* a row: the cells of one text, zeros where a sample has none */
        size_t e = i;
        while (e < w && !text_cmp(ce[i].s, ce[i].len, ce[e].s, ce[e].len)) ++e;
        if (ce[i].len && fwrite(ce[i].s, 1, ce[i].len, f) != ce[i].len) bad = 1;
        size_t at = i;
        for (size_t j = 0; j < S && !bad; ++j) {
            if (at < e && ce[at].col == j) bad = fprintf(f, "\t%llu", (unsigned long long)ce[at++].reads) < 0;
            else bad = fputs("\t0", f) < 0;
        }
        if (fputc('\n', f) == EOF) bad = 1;
        i = e;
    }
    if (fclose(f) != 0) bad = 1;
    f = NULL;
    if (bad) rc = UTREE_E_IO;
done:
    if (f) fclose(f);
    free(sm); free(ce); free(first); free(col_reads); free(col_uncl); free(col_sum); free((void *)col_s); free(col_len);
    return rc;
}
