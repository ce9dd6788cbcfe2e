/* sredist.c -- ambiguous reads redistributed per sample of a multiplexed file (include/utree_amd.h: utree_sredist_*).
 *
 * The handle keeps, on the device and for a whole search, the id table of a sample table (sample_ids.c), the table of multi-label candidate sets
 * of a redistribution (redist.c) and a cell table keyed (sample, candidate set), fed by one pass per batch between the classify kernels and
 * the vote (sredist_kernels.hip).  Here: the handle, the read-back into a flat form, its insert (and so the merge of two handles), the solver's
 * host side -- every sample's labels renumbered in ascending file-order index into one flat tally, so that 65 536 samples x 1 M labels cost
 * what occurs and the tie-break survives; the passes run on the device, a stopped sample's tally frozen -- and the host-only writer's checks
 * (the matrix itself: taxon_table.c).
 */
#define _GNU_SOURCE
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ctr_host.h"
#include "dev_image.h"
#include "sample_ids.h"
#include "sredist.h"
#include "taxon_table.h"

struct utree_sredist {
    int device, n_cu;
    uint32_t n_labels;
    utk_sredist_tab tab;                /* s: one device block (sample_ids.c); r.slots, r.arena, r.misc: allocations of their own */
};

#define CHK(x) do { if ((x) != hipSuccess) { utree_dev_set_hip_error((int)hipGetLastError(), #x); rc = UTREE_E_HIP; goto fail; } } while (0)

static const utree_sample_ids_text TEXT = {"sample redistribution", "tables", "the table of (sample, candidate set) cells is full (raise UTREE_SAMPLE_CELLS)",
                                           "a name lies outside its chunk, or a cell names no sample"};

int utree_sredist_create(utree_dev *dev, uint32_t sample_capacity, uint32_t set_capacity, uint32_t cell_capacity, int delim, utree_sredist **out) {
    if (!dev || !out) return UTREE_E_ARG;
    *out = NULL;
    if (!set_capacity || set_capacity > (1u << 28)) return UTREE_E_ARG;
    utree_sredist *h = (utree_sredist *)calloc(1, sizeof *h);
    if (!h) return UTREE_E_NOMEM;
    h->device = dev->device; h->n_cu = dev->n_cu; h->n_labels = (uint32_t)dev->hdr.n_labels;
    int rc = utree_sample_ids_create(&h->tab.s, h->device, sample_capacity, cell_capacity, delim, dev->hdr.n_labels);
    if (rc) { free(h); return rc; }
    uint32_t set_slots = 1;
    while (set_slots < set_capacity) set_slots <<= 1;
    utk_redist_tab *r = &h->tab.r;
    r->mask = set_slots - 1; r->n_labels = h->n_labels; r->arena_cap = (uint64_t)set_slots * UTK_REDIST_ARENA_PER_SLOT;
    if (hipMalloc((void **)&r->slots, (size_t)set_slots * 16) != hipSuccess || hipMalloc((void **)&r->arena, r->arena_cap * 4) != hipSuccess ||
        hipMalloc((void **)&r->misc, UTK_REDIST_MISC_WORDS * 8) != hipSuccess) {
        (void)hipGetLastError();
        rc = UTREE_E_NOMEM;
    }
    if (!rc) rc = utree_sredist_reset(h);
    if (rc) { utree_sredist_free(h); return rc; }
    *out = h;
    return UTREE_OK;
}

int utree_sredist_reset(utree_sredist *h) {
    if (!h) return UTREE_E_ARG;
    if (hipSetDevice(h->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return UTREE_E_HIP;   /* adds in flight on any stream */
    const int rc = utree_sample_ids_reset(&h->tab.s);                                                         /* (the arenas are written before they are read) */
    if (rc) return rc;
    if (hipMemset(h->tab.r.slots, 0, ((size_t)h->tab.r.mask + 1) * 16) != hipSuccess) return UTREE_E_HIP;     /* set key 0 = free */
    if (hipMemset(h->tab.r.misc, 0, UTK_REDIST_MISC_WORDS * 8) != hipSuccess) return UTREE_E_HIP;
    return hipDeviceSynchronize() == hipSuccess ? UTREE_OK : UTREE_E_HIP;
}

void utree_sredist_free(utree_sredist *h) {
    if (!h) return;
    hipSetDevice(h->device);
    hipDeviceSynchronize();
    utree_sample_ids_free(&h->tab.s);
    if (h->tab.r.slots) hipFree(h->tab.r.slots);
    if (h->tab.r.arena) hipFree(h->tab.r.arena);
    if (h->tab.r.misc) hipFree(h->tab.r.misc);
    free(h);
}

int utree_sredist_add_pending(utree_sredist *h, const utk_image *im, const utree_result *d_res, const utk_workspace *ws, const uint8_t *d_text,
                              uint64_t text_bytes, const uint32_t *d_name_off, const uint32_t *d_name_len, uint32_t n_reads, int n_cu, void *stream) {
    const int e = utk_sredist_add(&h->tab, im, d_res, ws, d_text, text_bytes, d_name_off, d_name_len, n_reads, n_cu, stream);
    if (e) { utree_dev_set_hip_error(e, "utk_sredist_add"); return UTREE_E_HIP; }
    return UTREE_OK;
}

int utree_sredist_classify_batch(utree_sredist *h, utree_dev *dev, const uint8_t *d_bases, const uint64_t *d_off, const uint32_t *d_len,
                                 uint32_t n_reads, uint64_t total_bases, uint32_t max_len, int do_rc, const uint8_t *d_text, uint64_t text_bytes,
                                 const uint32_t *d_name_off, const uint32_t *d_name_len, utree_result *d_out, void *d_workspace,
                                 size_t workspace_bytes, void *stream) {
    if (!h || !dev || h->device != dev->device || h->n_labels != dev->hdr.n_labels) return UTREE_E_ARG;
    if (n_reads && (!d_name_off || !d_name_len || (!d_text && text_bytes))) return UTREE_E_ARG;
    const utree_batch_view v = {d_bases, d_off, d_len, n_reads, total_bases, max_len, do_rc, d_text, text_bytes, d_name_off, d_name_len, stream};
    return utree_classify_view(dev, &v, d_out, d_workspace, workspace_bytes, NULL, h, NULL);
}

/* ---- the device's state as one flat table on the host ------------------------------------------------------------------------------------- */
typedef struct {
    size_t S, id_bytes, n_cells, n_labels;
    uint64_t n_reads;
    uint8_t *ids; uint64_t *id_off, *reads, *uncl;     /* id_off [S + 1] */
    utree_sredist_cell *cells; uint32_t *labels;
} flat_t;

static void flat_free(flat_t *f) {
    free(f->ids); free(f->id_off); free(f->reads); free(f->uncl); free(f->cells); free(f->labels);
    memset(f, 0, sizeof *f);
}

/* everything the device holds (synchronous); UTREE_E_DEVICE with a text when a batch set a flag or the counters do not add up */
static int collect(utree_sredist *h, flat_t *f) {
    memset(f, 0, sizeof *f);
    int rc = UTREE_OK;
    const size_t set_slots = (size_t)h->tab.r.mask + 1;
    unsigned long long *slots = NULL, rmisc[UTK_REDIST_MISC_WORDS];
    uint32_t *sarena = NULL;
    char more[320];
    utree_sample_ids_view v = {0};
    CHK(hipSetDevice(h->device));
    CHK(hipDeviceSynchronize());
    CHK(hipMemcpy(rmisc, h->tab.r.misc, sizeof rmisc, hipMemcpyDeviceToHost));
    utree_redist_flags_text(rmisc[1], " ", ";", more, sizeof more);
    rc = utree_sample_ids_read(&h->tab.s, &TEXT, more, &v);
    f->n_reads = v.n_reads;
    if (rc) goto fail;
    const size_t S = v.S;
    const uint64_t sused = rmisc[2];
    if (sused > h->tab.r.arena_cap) { utree_set_error_text("sample redistribution: the counters of the tables are inconsistent"); rc = UTREE_E_DEVICE; goto fail; }
    slots = (unsigned long long *)malloc(set_slots * 16);
    sarena = (uint32_t *)malloc((sused ? sused : 1) * 4);
    if (!slots || !sarena) { rc = UTREE_E_NOMEM; goto fail; }
    CHK(hipMemcpy(slots, h->tab.r.slots, set_slots * 16, hipMemcpyDeviceToHost));
    if (sused) CHK(hipMemcpy(sarena, h->tab.r.arena, sused * 4, hipMemcpyDeviceToHost));
    size_t nc = 0, nl = 0;
    for (uint32_t c = 0; c < v.cell_slots; ++c) {
        const unsigned long long key = v.cells[2 * (size_t)c], cnt = v.cells[2 * (size_t)c + 1];
        if (key == ~0ull || !cnt) continue;
        const uint32_t hd = (uint32_t)key;
        uint32_t sample;
        uint64_t n = 1;
        if ((rc = utree_sample_ids_count(&TEXT, &v, (uint32_t)(key >> 32), cnt, &sample))) goto fail;
        if (hd & UTK_SREDIST_ONE) { if ((hd & ~UTK_SREDIST_ONE) >= h->n_labels) n = 0; }
        else if (hd >= set_slots || !slots[2 * (size_t)hd] || (slots[2 * (size_t)hd] >> 32) + (uint32_t)slots[2 * (size_t)hd] > sused) n = 0;
        else n = (uint32_t)slots[2 * (size_t)hd];
        if (!n) { utree_set_error_text("sample redistribution: a cell names no candidate set"); rc = UTREE_E_DEVICE; goto fail; }
        ++nc; nl += n;
    }
    f->S = S; f->id_bytes = v.id_bytes; f->n_cells = nc; f->n_labels = nl;
    f->cells = (utree_sredist_cell *)malloc((nc ? nc : 1) * sizeof *f->cells);
    f->labels = (uint32_t *)malloc((nl ? nl : 1) * 4);
    if (!f->cells || !f->labels) { rc = UTREE_E_NOMEM; goto fail; }
    size_t q = 0, li = 0;
    for (uint32_t c = 0; c < v.cell_slots; ++c) {
        const unsigned long long key = v.cells[2 * (size_t)c], cnt = v.cells[2 * (size_t)c + 1];
        if (key == ~0ull || !cnt) continue;
        const uint32_t slot = (uint32_t)(key >> 32), hd = (uint32_t)key;
        utree_sredist_cell *e = &f->cells[q++];
        e->sample = v.index[slot]; e->first = li; e->reads = cnt;
        if (hd & UTK_SREDIST_ONE) { e->n = 1; f->labels[li++] = hd & ~UTK_SREDIST_ONE; }
        else {
            e->n = (uint32_t)slots[2 * (size_t)hd];
            memcpy(f->labels + li, sarena + (slots[2 * (size_t)hd] >> 32), (size_t)e->n * 4);
            li += e->n;
        }
    }
    if ((rc = utree_sample_ids_check_sums(&TEXT, &v))) goto fail;
    f->ids = v.ids; f->id_off = v.id_off; f->reads = v.reads; f->uncl = v.uncl;      /* the samples, dense: the flat table's from here on */
    v.ids = NULL; v.id_off = NULL; v.reads = NULL; v.uncl = NULL;
fail:
    free(slots); free(sarena);
    utree_sample_ids_view_free(&v);
    if (rc) { const uint64_t nr = f->n_reads; flat_free(f); f->n_reads = nr; }
    return rc;
}

/* reads added so far, after a wait for the device; UTREE_E_DEVICE when a batch set a flag (reports.c) */
int utree_sredist_reads(utree_sredist *h, uint64_t *n_reads) {
    if (!h || !n_reads) return UTREE_E_ARG;
    int rc = UTREE_OK;
    unsigned long long misc[UTK_SAMPLES_MISC_WORDS], rmisc[UTK_REDIST_MISC_WORDS];
    CHK(hipSetDevice(h->device));
    CHK(hipDeviceSynchronize());
    CHK(hipMemcpy(misc, h->tab.s.misc, sizeof misc, hipMemcpyDeviceToHost));
    CHK(hipMemcpy(rmisc, h->tab.r.misc, sizeof rmisc, hipMemcpyDeviceToHost));
    *n_reads = misc[0];
    char more[320];
    utree_redist_flags_text(rmisc[1], " ", ";", more, sizeof more);
    rc = utree_sample_ids_check_flags(&TEXT, misc[1], more);
fail:
    return rc;
}

int utree_sredist_read(utree_sredist *h, uint8_t *h_ids, size_t id_cap, uint64_t *h_id_off, uint64_t *h_reads, uint64_t *h_unclassified,
                       size_t sample_cap, utree_sredist_cell *h_cells, size_t cell_cap, uint32_t *h_labels, size_t label_cap, size_t *n_samples,
                       size_t *n_id_bytes, size_t *n_cells, size_t *n_labels, uint64_t *n_reads) {
    if (!h || !n_samples || !n_id_bytes || !n_cells || !n_labels || (id_cap && !h_ids) || (sample_cap && (!h_id_off || !h_reads || !h_unclassified)) ||
        (cell_cap && !h_cells) || (label_cap && !h_labels)) return UTREE_E_ARG;
    *n_samples = 0; *n_id_bytes = 0; *n_cells = 0; *n_labels = 0;
    flat_t f;
    const int rc = collect(h, &f);
    if (n_reads) *n_reads = f.n_reads;
    if (rc) return rc;
    *n_samples = f.S; *n_id_bytes = f.id_bytes; *n_cells = f.n_cells; *n_labels = f.n_labels;
    if (f.S > sample_cap || f.id_bytes > id_cap || f.n_cells > cell_cap || f.n_labels > label_cap) { flat_free(&f); return UTREE_E_ARG; }
    if (f.id_bytes) memcpy(h_ids, f.ids, f.id_bytes);
    if (h_id_off) memcpy(h_id_off, f.id_off, (f.S + 1) * 8);
    if (f.S) { memcpy(h_reads, f.reads, f.S * 8); memcpy(h_unclassified, f.uncl, f.S * 8); }
    if (f.n_cells) memcpy(h_cells, f.cells, f.n_cells * sizeof *h_cells);
    if (f.n_labels) memcpy(h_labels, f.labels, f.n_labels * 4);
    flat_free(&f);
    return UTREE_OK;
}

int utree_sredist_insert(utree_sredist *h, const uint8_t *ids, const uint64_t *id_off, const uint64_t *reads, const uint64_t *unclassified,
                         size_t n_samples, const utree_sredist_cell *cells, size_t n_cells, const uint32_t *labels, size_t n_labels,
                         uint64_t n_reads) {
    if (!h || (n_samples && (!id_off || !reads || !unclassified)) || (n_cells && (!cells || !labels)) || n_samples > h->tab.s.sample_cap) return UTREE_E_ARG;
    const uint64_t zero_off[1] = {0};
    if (!n_samples) id_off = zero_off;
    for (size_t i = 0; i < n_samples; ++i) if (id_off[i + 1] < id_off[i] || id_off[i + 1] - id_off[i] > 0xFFFFFFFEull) return UTREE_E_ARG;
    const uint64_t id_bytes = id_off[n_samples];
    if (id_bytes && !ids) return UTREE_E_ARG;
    for (size_t i = 0; i < n_cells; ++i)
        if (cells[i].sample >= n_samples || cells[i].first > n_labels || cells[i].n > n_labels - cells[i].first) return UTREE_E_ARG;
    /* one device block: id_off [S + 1] | reads [S] | uncl [S] | cells | labels | slot_of [S] | id bytes */
    const size_t o_reads = (n_samples + 1) * 8, o_uncl = o_reads + n_samples * 8, o_cells = o_uncl + n_samples * 8,
                 o_labels = o_cells + n_cells * sizeof *cells, o_slot = o_labels + n_labels * 4, o_ids = o_slot + n_samples * 4,
                 bytes = o_ids + (size_t)id_bytes;
    int rc = UTREE_OK;
    uint8_t *d = NULL;
    CHK(hipSetDevice(h->device));
    CHK(hipDeviceSynchronize());
    if (hipMalloc((void **)&d, bytes) != hipSuccess) { (void)hipGetLastError(); return UTREE_E_NOMEM; }
    CHK(hipMemcpy(d, id_off, (n_samples + 1) * 8, hipMemcpyHostToDevice));
    if (n_samples) { CHK(hipMemcpy(d + o_reads, reads, n_samples * 8, hipMemcpyHostToDevice)); CHK(hipMemcpy(d + o_uncl, unclassified, n_samples * 8, hipMemcpyHostToDevice)); }
    if (n_cells) CHK(hipMemcpy(d + o_cells, cells, n_cells * sizeof *cells, hipMemcpyHostToDevice));
    if (n_labels) CHK(hipMemcpy(d + o_labels, labels, n_labels * 4, hipMemcpyHostToDevice));
    if (id_bytes) CHK(hipMemcpy(d + o_ids, ids, (size_t)id_bytes, hipMemcpyHostToDevice));
    if (utk_sredist_insert(&h->tab, d + o_ids, (const uint64_t *)d, (const unsigned long long *)(d + o_reads), (const unsigned long long *)(d + o_uncl),
                           (uint32_t)n_samples, (uint32_t *)(d + o_slot), (const utk_sredist_cell *)(d + o_cells), (const uint32_t *)(d + o_labels),
                           n_cells, n_reads, NULL)) { rc = UTREE_E_HIP; goto fail; }
    CHK(hipDeviceSynchronize());
fail:
    (void)hipDeviceSynchronize();
    if (d) hipFree(d);
    return rc;
}

int utree_sredist_merge(utree_sredist *dst, utree_sredist *src) {
    if (!dst || !src || dst == src || dst->n_labels != src->n_labels) return UTREE_E_ARG;
    flat_t f;
    int rc = collect(src, &f);
    if (rc) return rc;
    rc = utree_sredist_insert(dst, f.ids, f.id_off, f.reads, f.uncl, f.S, f.cells, f.n_cells, f.labels, f.n_labels, f.n_reads);
    flat_free(&f);
    return rc;
}

/* ---- the solver's host side --------------------------------------------------------------------------------------------------------------- */
static int u64_cmp(const void *a, const void *b) {
    const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;
    return x < y ? -1 : x > y;
}

int utree_sredist_solve(utree_sredist *h, uint32_t max_passes, utree_sredist_entry *e, size_t cap, size_t *n, uint32_t *h_passes,
                        uint64_t *h_ambiguous, size_t sample_cap, size_t *n_samples) {
    if (!h || !n || (cap && !e) || max_passes < 1 || max_passes > 1000) return UTREE_E_ARG;
    *n = 0;
    if (n_samples) *n_samples = 0;
    flat_t f;
    int rc = collect(h, &f);
    if (rc) return rc;
    const size_t S = f.S, nc = f.n_cells, nl = f.n_labels;
    if (n_samples) *n_samples = S;
    /* the (sample, label) pairs that occur, ascending: a pair's position is its tally index */
    uint64_t *pair = (uint64_t *)malloc((nl ? nl : 1) * 8), *uniq = (uint64_t *)calloc(nl ? nl : 1, 8), *amb = (uint64_t *)calloc(S ? S : 1, 8);
    uint64_t *assigned = NULL, *changes = (uint64_t *)malloc((S ? S : 1) * 8);
    uint32_t *member = (uint32_t *)malloc((nl ? nl : 1) * 4), *seg = NULL, *act = (uint32_t *)malloc((S ? S : 1) * 4);
    uint32_t *passes = (uint32_t *)calloc(S ? S : 1, 4), *order = (uint32_t *)malloc((S ? S : 1) * 4);
    uint8_t *d = NULL;
    size_t nt = 0;
    if (!pair || !uniq || !amb || !changes || !member || !act || !passes || !order) { rc = UTREE_E_NOMEM; goto fail; }
    for (size_t c = 0; c < nc; ++c)
        for (uint32_t i = 0; i < f.cells[c].n; ++i) pair[f.cells[c].first + i] = (uint64_t)f.cells[c].sample << 32 | f.labels[f.cells[c].first + i];
    qsort(pair, nl, 8, u64_cmp);
    for (size_t i = 0; i < nl; ++i) if (!i || pair[i] != pair[i - 1]) pair[nt++] = pair[i];
    seg = (uint32_t *)malloc((nt ? nt : 1) * 4);
    assigned = (uint64_t *)calloc(nt ? nt : 1, 8);
    if (!seg || !assigned) { rc = UTREE_E_NOMEM; goto fail; }
    for (size_t i = 0; i < nt; ++i) seg[i] = (uint32_t)(pair[i] >> 32);
    for (size_t c = 0; c < nc; ++c) {
        const utree_sredist_cell *ce = &f.cells[c];
        for (uint32_t i = 0; i < ce->n; ++i) {
            const uint64_t key = (uint64_t)ce->sample << 32 | f.labels[ce->first + i];
            const uint64_t *at = (const uint64_t *)bsearch(&key, pair, nt, 8, u64_cmp);
            member[ce->first + i] = (uint32_t)(at - pair);
        }
        if (ce->n == 1) uniq[member[ce->first]] += ce->reads; else amb[ce->sample] += ce->reads;
    }
    if (nt > 0xFFFFFFFEull) { rc = UTREE_E_UNSUPPORTED; goto fail; }
    if (nt && nc) {
        /* one device block: tally [2][nt] | changes [S] | cells | member | seg | act [S] */
        const size_t o_ch = 2 * nt * 8, o_cells = o_ch + S * 8, o_mem = o_cells + nc * sizeof *f.cells, o_seg = o_mem + nl * 4, o_act = o_seg + nt * 4,
                     bytes = o_act + S * 4;
        CHK(hipSetDevice(h->device));
        if (hipMalloc((void **)&d, bytes) != hipSuccess) { (void)hipGetLastError(); rc = UTREE_E_NOMEM; goto fail; }
        CHK(hipMemcpy(d + o_cells, f.cells, nc * sizeof *f.cells, hipMemcpyHostToDevice));
        CHK(hipMemcpy(d + o_mem, member, nl * 4, hipMemcpyHostToDevice));
        CHK(hipMemcpy(d + o_seg, seg, nt * 4, hipMemcpyHostToDevice));
        const utk_sredist_problem p = {(const utk_sredist_cell *)(d + o_cells), (const uint32_t *)(d + o_mem), (const uint32_t *)(d + o_seg),
                                       (const uint32_t *)(d + o_act), nc, nt};
        unsigned long long *prev = (unsigned long long *)d, *next = prev + nt, *d_ch = (unsigned long long *)(d + o_ch);
        if (utk_sredist_tally0(&p, prev, NULL)) { rc = UTREE_E_HIP; goto fail; }
        size_t n_act = S;
        for (size_t s = 0; s < S; ++s) { act[s] = (uint32_t)s; order[s] = (uint32_t)s; }
        while (n_act) {
            CHK(hipMemcpy(d + o_act, act, S * 4, hipMemcpyHostToDevice));
            if (utk_sredist_pass(&p, prev, next, d_ch, (uint32_t)n_act, 0, NULL)) { rc = UTREE_E_HIP; goto fail; }
            CHK(hipMemcpy(changes, d_ch, n_act * 8, hipMemcpyDeviceToHost));       /* one word per still-active sample */
            { unsigned long long *t = prev; prev = next; next = t; }
            size_t keep = 0;
            for (size_t k = 0; k < n_act; ++k) {
                const uint32_t s = order[k];
                ++passes[s];
                if (passes[s] >= max_passes || changes[k] <= f.reads[s] / 100000) act[s] = 0xFFFFFFFFu;     /* stopped: its tally is frozen from here on */
                else { act[s] = (uint32_t)keep; order[keep++] = s; }
            }
            n_act = keep;
        }
        /* the final assignment: one more evaluation of every sample under its own T_P (not T_P itself) */
        if (utk_sredist_pass(&p, prev, next, d_ch, 0, 1, NULL)) { rc = UTREE_E_HIP; goto fail; }
        CHK(hipMemcpy(assigned, next, nt * 8, hipMemcpyDeviceToHost));
    } else for (size_t s = 0; s < S; ++s) passes[s] = 1;                            /* nothing to move: the one pass every sample runs */
    size_t k = 0;
    for (size_t i = 0; i < nt; ++i) if (assigned[i] || uniq[i]) {
        if (k < cap) { e[k].sample = seg[i]; e[k].label = (uint32_t)pair[i]; e[k].assigned = assigned[i]; e[k].unique = uniq[i]; }
        ++k;
    }
    *n = k;
    if (k > cap || ((h_passes || h_ambiguous) && S > sample_cap)) rc = UTREE_E_ARG;
    else {
        if (h_passes && S) memcpy(h_passes, passes, S * 4);
        if (h_ambiguous && S) memcpy(h_ambiguous, amb, S * 8);
    }
fail:
    (void)hipDeviceSynchronize();
    if (d) hipFree(d);
    free(pair); free(uniq); free(amb); free(assigned); free(changes); free(member); free(seg); free(act); free(passes); free(order);
    flat_free(&f);
    return rc;
}

/* ---- host: the samples of a read-back and the figures of a solve -> the file ---------------------------------------------------------------- */
int utree_sredist_write(const utree_ctr *ctr, const uint8_t *ids, const uint64_t *id_off, const uint64_t *reads, const uint64_t *unclassified,
                        const uint32_t *passes, const uint64_t *ambiguous, size_t n_samples, const utree_sredist_entry *e, size_t n_entries,
                        uint64_t n_reads, const char *path) {
    if (!ctr || !path || (n_samples && (!id_off || !reads || !unclassified || !passes || !ambiguous)) || (n_entries && !e)) return UTREE_E_ARG;
    const size_t S = n_samples;
    utree_matrix_col *col = (utree_matrix_col *)calloc(S ? S : 1, sizeof *col);         /* column i is sample i; two samples with one id are refused by the writer */
    utree_matrix_cell *row = (utree_matrix_cell *)calloc(n_entries ? n_entries : 1, sizeof *row);
    uint64_t *passes64 = (uint64_t *)calloc(S ? S : 1, 8);
    int rc = UTREE_OK;
    if (!col || !row || !passes64) { rc = UTREE_E_NOMEM; goto done; }
    uint64_t total = 0, A = 0, G = 0;
    for (size_t i = 0; i < S; ++i) {
        if (id_off[i + 1] < id_off[i] || (id_off[i + 1] > id_off[i] && !ids)) { rc = UTREE_E_ARG; goto done; }
        col[i].len = id_off[i + 1] - id_off[i];
        col[i].s = col[i].len ? ids + id_off[i] : (const uint8_t *)"";
        col[i].reads = reads[i]; col[i].uncl = unclassified[i]; passes64[i] = passes[i];
        if (unclassified[i] > reads[i] || ambiguous[i] > reads[i] - unclassified[i] || passes[i] < 1 || passes[i] > 1000) { rc = UTREE_E_ARG; goto done; }
        total += reads[i]; A += ambiguous[i];
    }
    if (total != n_reads) { rc = UTREE_E_ARG; goto done; }                /* the samples' reads are the reads */
    size_t q = 0;
    for (size_t i = 0; i < n_entries; ++i) {
        if (e[i].sample >= S || e[i].label >= ctr->info.n_labels) { rc = UTREE_E_ARG; goto done; }
        if (!e[i].assigned) continue;
        row[q].s = ctr->labels[e[i].label]; row[q].len = ctr->label_len[e[i].label]; row[q].col = e[i].sample; row[q].reads = e[i].assigned;
        G += e[i].assigned;
        ++q;
    }
    char header[200];
    snprintf(header, sizeof header, "# reads\t%llu\tclassified\t%llu\tunclassified\t%llu\tambiguous\t%llu", (unsigned long long)n_reads,
             (unsigned long long)G, (unsigned long long)(n_reads - G), (unsigned long long)A);
    const utree_matrix_extra extra[2] = {{"ambiguous", ambiguous}, {"passes", passes64}};
    rc = utree_sample_matrix_write(header, col, S, 0, extra, 2, row, q, path);          /* labels of equal text are one row */
done:
    free(col); free(row); free(passes64);
    return rc;
}
