/* sredist.c -- ambiguous reads redistributed per sample of a multiplexed file (include/utree_amd.h: utree_sredist_*).
 *
 * The handle keeps, on the device and for a whole search, the id table of a sample table (samples.c), the table of multi-label candidate sets
 * of a redistribution (redist.c) and a cell table keyed (sample, candidate set), fed by one pass per batch between the classify kernels and
 * the vote (sredist_kernels.hip).  Here: the handle, the read-back into a flat form, its insert (and so the merge of two handles), the solver's
 * host side -- every sample's labels renumbered in ascending file-order index into one flat tally, so that 65 536 samples x 1 M labels cost
 * what occurs and the tie-break survives; the passes run on the device, a stopped sample's tally frozen -- and the host-only writer.
 */
#define _GNU_SOURCE
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ctr_host.h"
#include "dev_image.h"
#include "sredist.h"

struct utree_sredist {
    int device, n_cu;
    uint32_t id_slots, cell_slots, n_labels;
    uint8_t *d_mem;                     /* ids | reads | uncl | cells | misc | index | arena, as samples.c lays them out */
    size_t bytes, counters_bytes;       /* counters_bytes: everything in front of the arena */
    utk_sredist_tab tab;                /* r.slots, r.arena, r.misc: allocations of their own */
};

#define CHK(x) do { if ((x) != hipSuccess) { utree_dev_set_hip_error((int)hipGetLastError(), #x); rc = UTREE_E_HIP; goto fail; } } while (0)

static int check_flags(unsigned long long fs, unsigned long long fr) {
    if (!fs && !fr) return UTREE_OK;
    char msg[900];
    snprintf(msg, sizeof msg, "sample redistribution:%s%s%s%s%s%s%s",
             fs & UTK_SAMPLES_F_TABLE ? " more distinct sample ids than the table holds (raise UTREE_SAMPLE_CAPACITY; is the delimiter right?);" : "",
             fs & UTK_SAMPLES_F_ARENA ? " the arena of id bytes is used up (raise UTREE_SAMPLE_CAPACITY; is the delimiter right?);" : "",
             fs & UTK_SAMPLES_F_CELLS ? " the table of (sample, candidate set) cells is full (raise UTREE_SAMPLE_CELLS);" : "",
             fs & UTK_SAMPLES_F_NAME ? " a name lies outside its chunk, or a cell names no sample;" : "",
             fr & UTK_REDIST_F_TABLE ? " the table of candidate sets was too small (raise UTREE_REDIST_CAPACITY);" : "",
             fr & UTK_REDIST_F_ARENA ? " the arena of the sets' labels was too small (raise UTREE_REDIST_CAPACITY);" : "",
             fr & UTK_REDIST_F_LABEL ? " a record named a label the database does not have;" : "");
    const size_t l = strlen(msg);
    if (l && msg[l - 1] == ';') msg[l - 1] = 0;
    utree_set_error_text(msg);
    return UTREE_E_DEVICE;
}

int utree_sredist_create(utree_dev *dev, uint32_t sample_capacity, uint32_t set_capacity, uint32_t cell_capacity, int delim, utree_sredist **out) {
    if (!dev || !out) return UTREE_E_ARG;
    *out = NULL;
    if (!sample_capacity || sample_capacity > (1u << (UTK_SAMPLES_SLOT_BITS - 1)) || !set_capacity || set_capacity > (1u << 28) || !cell_capacity ||
        cell_capacity > (1u << 30)) return UTREE_E_ARG;
    if (delim < 0 || delim > 255 || delim == '\t' || delim == ' ' || delim == '\r' || delim == '\n') return UTREE_E_ARG;
    if (dev->hdr.n_labels >= (1ull << 28)) return UTREE_E_UNSUPPORTED;            /* a set handle has 28 bits for the label */
    utree_sredist *h = (utree_sredist *)calloc(1, sizeof *h);
    if (!h) return UTREE_E_NOMEM;
    h->device = dev->device; h->n_cu = dev->n_cu; h->n_labels = (uint32_t)dev->hdr.n_labels;
    h->id_slots = 16; h->cell_slots = 16;
    uint32_t set_slots = 1;
    while (h->id_slots < 2 * sample_capacity) h->id_slots <<= 1;                  /* at most half full: short probe chains */
    while (h->cell_slots < cell_capacity) h->cell_slots <<= 1;
    while (set_slots < set_capacity) set_slots <<= 1;
    uint64_t arena = (uint64_t)sample_capacity * UTK_SAMPLES_ARENA_PER_SAMPLE;
    if (arena < (1u << 20)) arena = 1u << 20;
    if (arena > 0xFFFFFF00ull) arena = 0xFFFFFF00ull;                             /* a key holds the offset in 32 bits */
    const size_t ids = (size_t)h->id_slots * 8, cells = 2 * (size_t)h->cell_slots * 8, misc = UTK_SAMPLES_MISC_WORDS * 8, index = (size_t)h->id_slots * 4;
    h->counters_bytes = 3 * ids + cells + misc + index;
    h->bytes = h->counters_bytes + (size_t)arena;
    utk_samples_tab *t = &h->tab.s;
    utk_redist_tab *r = &h->tab.r;
    r->mask = set_slots - 1; r->n_labels = h->n_labels; r->arena_cap = (uint64_t)set_slots * UTK_REDIST_ARENA_PER_SLOT;
    if (hipSetDevice(h->device) != hipSuccess) { free(h); return UTREE_E_HIP; }
    if (hipMalloc((void **)&h->d_mem, h->bytes) != hipSuccess || hipMalloc((void **)&r->slots, (size_t)set_slots * 16) != hipSuccess ||
        hipMalloc((void **)&r->arena, r->arena_cap * 4) != hipSuccess || hipMalloc((void **)&r->misc, UTK_REDIST_MISC_WORDS * 8) != hipSuccess) {
        (void)hipGetLastError();
        utree_sredist_free(h);
        return UTREE_E_NOMEM;
    }
    t->ids = (unsigned long long *)h->d_mem; t->reads = t->ids + h->id_slots; t->uncl = t->reads + h->id_slots;
    t->cells = t->uncl + h->id_slots; t->misc = t->cells + 2 * (size_t)h->cell_slots;
    t->index = (uint32_t *)(t->misc + UTK_SAMPLES_MISC_WORDS); t->arena = (uint8_t *)(t->index + h->id_slots);
    t->arena_cap = arena; t->id_mask = h->id_slots - 1; t->cell_mask = h->cell_slots - 1; t->sample_cap = sample_capacity;
    t->n_labels = h->n_labels; t->delim = (uint32_t)delim;
    const int rc = utree_sredist_reset(h);
    if (rc) { utree_sredist_free(h); return rc; }
    *out = h;
    return UTREE_OK;
}

int utree_sredist_reset(utree_sredist *h) {
    if (!h) return UTREE_E_ARG;
    if (hipSetDevice(h->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return UTREE_E_HIP;   /* adds in flight on any stream */
    if (hipMemset(h->d_mem, 0, h->counters_bytes) != hipSuccess) return UTREE_E_HIP;                          /* (the arenas are written before they are read) */
    if (hipMemset(h->tab.s.cells, 0xFF, 2 * (size_t)h->cell_slots * 8) != hipSuccess) return UTREE_E_HIP;     /* every cell key free (all ones) ... */
    if (hipMemset2D(h->tab.s.cells + 1, 16, 0, 8, h->cell_slots) != hipSuccess) return UTREE_E_HIP;           /* ... and every count zero           */
    if (hipMemset(h->tab.r.slots, 0, ((size_t)h->tab.r.mask + 1) * 16) != hipSuccess) return UTREE_E_HIP;     /* set key 0 = free */
    if (hipMemset(h->tab.r.misc, 0, UTK_REDIST_MISC_WORDS * 8) != hipSuccess) return UTREE_E_HIP;
    return hipDeviceSynchronize() == hipSuccess ? UTREE_OK : UTREE_E_HIP;
}

void utree_sredist_free(utree_sredist *h) {
    if (!h) return;
    hipSetDevice(h->device);
    hipDeviceSynchronize();
    if (h->d_mem) hipFree(h->d_mem);
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
    return utree_classify_batch_reports(dev, d_bases, d_off, d_len, n_reads, total_bases, max_len, do_rc, d_out, d_workspace, workspace_bytes, stream,
                                        NULL, h, d_text, text_bytes, d_name_off, d_name_len);
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
    uint8_t *m = (uint8_t *)malloc(h->counters_bytes), *arena = NULL;
    unsigned long long *slots = NULL, rmisc[UTK_REDIST_MISC_WORDS];
    uint32_t *sarena = NULL, *slot_of = NULL;
    uint64_t *sum = NULL;
    if (!m) return UTREE_E_NOMEM;
    CHK(hipSetDevice(h->device));
    CHK(hipDeviceSynchronize());
    CHK(hipMemcpy(m, h->d_mem, h->counters_bytes, hipMemcpyDeviceToHost));
    CHK(hipMemcpy(rmisc, h->tab.r.misc, sizeof rmisc, hipMemcpyDeviceToHost));
    const unsigned long long *ids = (const unsigned long long *)m, *reads = ids + h->id_slots, *uncl = reads + h->id_slots,
                             *cells = uncl + h->id_slots, *misc = cells + 2 * (size_t)h->cell_slots;
    const uint32_t *index = (const uint32_t *)(misc + UTK_SAMPLES_MISC_WORDS);
    f->n_reads = misc[0];
    if ((rc = check_flags(misc[1], rmisc[1]))) goto fail;
    const uint64_t S = misc[3], used = misc[2], sused = rmisc[2];
    if (S > h->tab.s.sample_cap || used > h->tab.s.arena_cap || sused > h->tab.r.arena_cap) {
        utree_set_error_text("sample redistribution: the counters of the tables are inconsistent"); rc = UTREE_E_DEVICE; goto fail;
    }
    slot_of = (uint32_t *)malloc((S ? S : 1) * sizeof *slot_of);
    arena = (uint8_t *)malloc(used ? used : 1);
    slots = (unsigned long long *)malloc(set_slots * 16);
    sarena = (uint32_t *)malloc((sused ? sused : 1) * 4);
    if (!slot_of || !arena || !slots || !sarena) { rc = UTREE_E_NOMEM; goto fail; }
    if (used) CHK(hipMemcpy(arena, h->tab.s.arena, used, hipMemcpyDeviceToHost));
    CHK(hipMemcpy(slots, h->tab.r.slots, set_slots * 16, hipMemcpyDeviceToHost));
    if (sused) CHK(hipMemcpy(sarena, h->tab.r.arena, sused * 4, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < S; ++i) slot_of[i] = 0xFFFFFFFFu;
    uint64_t claimed = 0, id_bytes = 0;
    for (uint32_t k = 0; k < h->id_slots; ++k) {
        if (!ids[k]) continue;
        const uint64_t at = ids[k] >> 32, len = (uint32_t)ids[k] - 1u;
        if (index[k] >= S || slot_of[index[k]] != 0xFFFFFFFFu || at + len > used) {
            utree_set_error_text("sample redistribution: a slot of the id table is inconsistent"); rc = UTREE_E_DEVICE; goto fail;
        }
        slot_of[index[k]] = k; ++claimed; id_bytes += len;
    }
    if (claimed != S) { utree_set_error_text("sample redistribution: the id table holds another number of ids than were claimed"); rc = UTREE_E_DEVICE; goto fail; }
    size_t nc = 0, nl = 0;
    for (uint32_t c = 0; c < h->cell_slots; ++c) {
        const unsigned long long key = cells[2 * (size_t)c], cnt = cells[2 * (size_t)c + 1];
        if (key == ~0ull || !cnt) continue;
        const uint32_t slot = (uint32_t)(key >> 32), hd = (uint32_t)key;
        uint64_t n = 1;
        if (slot >= h->id_slots || !ids[slot]) { utree_set_error_text("sample redistribution: a cell names no sample"); rc = UTREE_E_DEVICE; goto fail; }
        if (hd & UTK_SREDIST_ONE) { if ((hd & ~UTK_SREDIST_ONE) >= h->n_labels) n = 0; }
        else if (hd >= set_slots || !slots[2 * (size_t)hd] || (slots[2 * (size_t)hd] >> 32) + (uint32_t)slots[2 * (size_t)hd] > sused) n = 0;
        else n = (uint32_t)slots[2 * (size_t)hd];
        if (!n) { utree_set_error_text("sample redistribution: a cell names no candidate set"); rc = UTREE_E_DEVICE; goto fail; }
        ++nc; nl += n;
    }
    f->S = (size_t)S; f->id_bytes = (size_t)id_bytes; f->n_cells = nc; f->n_labels = nl;
    f->ids = (uint8_t *)malloc(id_bytes ? id_bytes : 1);
    f->id_off = (uint64_t *)malloc((S + 1) * 8); f->reads = (uint64_t *)malloc((S ? S : 1) * 8); f->uncl = (uint64_t *)malloc((S ? S : 1) * 8);
    f->cells = (utree_sredist_cell *)malloc((nc ? nc : 1) * sizeof *f->cells);
    f->labels = (uint32_t *)malloc((nl ? nl : 1) * 4);
    sum = (uint64_t *)calloc(S ? S : 1, 8);
    if (!f->ids || !f->id_off || !f->reads || !f->uncl || !f->cells || !f->labels || !sum) { rc = UTREE_E_NOMEM; goto fail; }
    uint64_t w = 0, total = 0;
    for (uint64_t i = 0; i < S; ++i) {
        const uint32_t k = slot_of[i];
        const uint64_t at = ids[k] >> 32, len = (uint32_t)ids[k] - 1u;
        f->id_off[i] = w;
        if (len) memcpy(f->ids + w, arena + at, len);
        w += len;
        f->reads[i] = reads[k]; f->uncl[i] = uncl[k];
        total += reads[k];
    }
    f->id_off[S] = w;
    size_t q = 0, li = 0;
    for (uint32_t c = 0; c < h->cell_slots; ++c) {
        const unsigned long long key = cells[2 * (size_t)c], cnt = cells[2 * (size_t)c + 1];
        if (key == ~0ull || !cnt) continue;
        const uint32_t slot = (uint32_t)(key >> 32), hd = (uint32_t)key;
        utree_sredist_cell *e = &f->cells[q++];
        e->sample = index[slot]; e->first = li; e->reads = cnt;
        if (hd & UTK_SREDIST_ONE) { e->n = 1; f->labels[li++] = hd & ~UTK_SREDIST_ONE; }
        else {
            e->n = (uint32_t)slots[2 * (size_t)hd];
            memcpy(f->labels + li, sarena + (slots[2 * (size_t)hd] >> 32), (size_t)e->n * 4);
            li += e->n;
        }
        sum[e->sample] += cnt;
    }
    for (uint64_t i = 0; i < S && !rc; ++i) if (f->reads[i] != f->uncl[i] + sum[i]) rc = UTREE_E_DEVICE;     /* per sample: reads = unclassified + its cells */
    if (!rc && total != misc[0]) rc = UTREE_E_DEVICE;
    if (rc) utree_set_error_text("sample redistribution: the samples' reads do not add up to the records added");
fail:
    free(m); free(arena); free(slots); free(sarena); free(slot_of); free(sum);
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
    rc = check_flags(misc[1], rmisc[1]);
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
typedef struct { const uint8_t *s; uint64_t len; uint32_t sample; } col_t;
typedef struct { const char *s; uint32_t len; uint32_t col; uint64_t reads; } row_t;

static int text_cmp(const void *a, uint64_t la, const void *b, uint64_t lb) {
    const uint64_t m = la < lb ? la : lb;
    const int c = m ? memcmp(a, b, m) : 0;
    if (c) return c;
    return la < lb ? -1 : la > lb;
}
static int col_cmp(const void *a, const void *b) {
    const col_t *x = (const col_t *)a, *y = (const col_t *)b;
    return text_cmp(x->s, x->len, y->s, y->len);
}
static int row_cmp(const void *a, const void *b) {
    const row_t *x = (const row_t *)a, *y = (const row_t *)b;
    const int c = text_cmp(x->s, x->len, y->s, y->len);
    if (c) return c;
    return x->col < y->col ? -1 : x->col > y->col;
}
static int put_id(FILE *f, const uint8_t *s, uint64_t len) {           /* TAB, CR and backslash escaped, nothing else (the sample table's escapes) */
    for (uint64_t i = 0; i < len; ++i) {
        const int c = s[i];
        const int r = c == '\t' ? fputs("\\t", f) : c == '\r' ? fputs("\\r", f) : c == '\\' ? fputs("\\\\", f) : fputc(c, f);
        if (r == EOF) return 1;
    }
    return 0;
}

int utree_sredist_write(const utree_ctr *ctr, const uint8_t *ids, const uint64_t *id_off, const uint64_t *reads, const uint64_t *unclassified,
                        const uint32_t *passes, const uint64_t *ambiguous, size_t n_samples, const utree_sredist_entry *e, size_t n_entries,
                        uint64_t n_reads, const char *path) {
    if (!ctr || !path || (n_samples && (!id_off || !reads || !unclassified || !passes || !ambiguous)) || (n_entries && !e)) return UTREE_E_ARG;
    const size_t S = n_samples;
    col_t *col = (col_t *)calloc(S ? S : 1, sizeof *col);
    row_t *row = (row_t *)calloc(n_entries ? n_entries : 1, sizeof *row);
    uint32_t *col_of = (uint32_t *)calloc(S ? S : 1, 4);
    uint64_t *col_sum = (uint64_t *)calloc(S ? S : 1, 8);
    int rc = UTREE_OK;
    FILE *f = NULL;
    if (!col || !row || !col_of || !col_sum) { rc = UTREE_E_NOMEM; goto done; }
    uint64_t total = 0, A = 0, G = 0;
    for (size_t i = 0; i < S; ++i) {
        if (id_off[i + 1] < id_off[i] || (id_off[i + 1] > id_off[i] && !ids)) { rc = UTREE_E_ARG; goto done; }
        col[i].len = id_off[i + 1] - id_off[i];
        col[i].s = col[i].len ? ids + id_off[i] : (const uint8_t *)"";
        col[i].sample = (uint32_t)i;
        if (unclassified[i] > reads[i] || ambiguous[i] > reads[i] - unclassified[i] || passes[i] < 1 || passes[i] > 1000) { rc = UTREE_E_ARG; goto done; }
        total += reads[i]; A += ambiguous[i];
    }
    if (total != n_reads) { rc = UTREE_E_ARG; goto done; }                /* the samples' reads are the reads */
    qsort(col, S, sizeof *col, col_cmp);                                 /* the columns: unsigned bytewise order, shorter first */
    for (size_t j = 0; j < S; ++j) {
        if (j && !col_cmp(&col[j - 1], &col[j])) { rc = UTREE_E_ARG; goto done; }      /* two samples with one id */
        col_of[col[j].sample] = (uint32_t)j;
    }
    size_t q = 0;
    for (size_t i = 0; i < n_entries; ++i) {
        if (e[i].sample >= S || e[i].label >= ctr->info.n_labels) { rc = UTREE_E_ARG; goto done; }
        if (!e[i].assigned) continue;
        row[q].s = ctr->labels[e[i].label]; row[q].len = ctr->label_len[e[i].label]; row[q].col = col_of[e[i].sample]; row[q].reads = e[i].assigned;
        col_sum[row[q].col] += e[i].assigned; G += e[i].assigned;
        ++q;
    }
    for (size_t i = 0; i < S; ++i)
        if (col_sum[col_of[i]] != reads[i] - unclassified[i]) { rc = UTREE_E_ARG; goto done; }       /* column j sums to n_j - u_j */
    qsort(row, q, sizeof *row, row_cmp);
    size_t w = 0;
    for (size_t i = 0; i < q; ++i) {                                     /* labels of equal text are one row */
        if (w && !row_cmp(&row[w - 1], &row[i])) row[w - 1].reads += row[i].reads;
        else row[w++] = row[i];
    }
    f = fopen(path, "wb");
    if (!f) { rc = UTREE_E_IO; goto done; }
    int bad = fprintf(f, "# reads\t%llu\tclassified\t%llu\tunclassified\t%llu\tambiguous\t%llu\tsamples\t%llu\n", (unsigned long long)n_reads,
                      (unsigned long long)G, (unsigned long long)(n_reads - G), (unsigned long long)A, (unsigned long long)S) < 0;
    bad |= fputs("# taxon", f) < 0;
    for (size_t j = 0; j < S && !bad; ++j) bad = fputc('\t', f) == EOF || put_id(f, col[j].s, col[j].len);
    bad |= fputs("\n# reads", f) < 0;
    for (size_t j = 0; j < S && !bad; ++j) bad = fprintf(f, "\t%llu", (unsigned long long)reads[col[j].sample]) < 0;
    bad |= fputs("\n# unclassified", f) < 0;
    for (size_t j = 0; j < S && !bad; ++j) bad = fprintf(f, "\t%llu", (unsigned long long)unclassified[col[j].sample]) < 0;
    bad |= fputs("\n# ambiguous", f) < 0;
    for (size_t j = 0; j < S && !bad; ++j) bad = fprintf(f, "\t%llu", (unsigned long long)ambiguous[col[j].sample]) < 0;
    bad |= fputs("\n# passes", f) < 0;
    for (size_t j = 0; j < S && !bad; ++j) bad = fprintf(f, "\t%u", passes[col[j].sample]) < 0;
    bad |= fputc('\n', f) == EOF;
    for (size_t i = 0; i < w && !bad;) {                                 /* a row: the cells of one text, zeros where a sample has none */
        size_t end = i;
        while (end < w && !text_cmp(row[i].s, row[i].len, row[end].s, row[end].len)) ++end;
        if (row[i].len && fwrite(row[i].s, 1, row[i].len, f) != row[i].len) bad = 1;
        size_t at = i;
        for (size_t j = 0; j < S && !bad; ++j) {
            if (at < end && row[at].col == j) bad = fprintf(f, "\t%llu", (unsigned long long)row[at++].reads) < 0;
            else bad = fputs("\t0", f) < 0;
        }
        if (fputc('\n', f) == EOF) bad = 1;
        i = end;
    }
    if (fclose(f) != 0) bad = 1;
    f = NULL;
    if (bad) rc = UTREE_E_IO;
done:
    if (f) fclose(f);
    free(col); free(row); free(col_of); free(col_sum);
    return rc;
}
