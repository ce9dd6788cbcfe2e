/* sample_ids.c -- the id-table half of a per-sample handle: the one device block a utk_samples_tab points into, its reset, and the read-back of
 * the samples -- ids, reads, unclassified, dense in the order the ids were claimed -- with every check of the id table.  The sample table
 * (samples.c) and the per-sample redistribution (sredist.c) differ in what a cell key holds; each decodes its own from the view given here.
 */
#define _GNU_SOURCE
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "dev_image.h"
#include "sample_ids.h"

#define CHK(x) do { if ((x) != hipSuccess) { utree_dev_set_hip_error((int)hipGetLastError(), #x); rc = UTREE_E_HIP; goto fail; } } while (0)

static int fail_text(const utree_sample_ids_text *x, const char *what, const char *whose) {
    char msg[160];
    snprintf(msg, sizeof msg, what, x->report, whose);
    utree_set_error_text(msg);
    return UTREE_E_DEVICE;
}

/* everything in front of the arena */
static size_t counters_bytes(const utk_samples_tab *t) { return (size_t)(t->arena - (const uint8_t *)t->ids); }

int utree_sample_ids_create(utk_samples_tab *t, int device, uint32_t sample_capacity, uint32_t cell_capacity, int delim, uint64_t n_labels) {
    memset(t, 0, sizeof *t);
    if (!sample_capacity || sample_capacity > (1u << (UTK_SAMPLES_SLOT_BITS - 1)) || !cell_capacity || cell_capacity > (1u << 30)) return UTREE_E_ARG;
    if (delim < 0 || delim > 255 || delim == '\t' || delim == ' ' || delim == '\r' || delim == '\n') return UTREE_E_ARG;
    if (n_labels >= (1ull << UTK_SAMPLES_LABEL_BITS)) return UTREE_E_UNSUPPORTED;         /* a packed cell key and a set handle have 28 bits for the label */
    uint32_t id_slots = 16, cell_slots = 16;
    while (id_slots < 2 * sample_capacity) id_slots <<= 1;                  /* at most half full: short probe chains */
    while (cell_slots < cell_capacity) cell_slots <<= 1;
    uint64_t arena = (uint64_t)sample_capacity * UTK_SAMPLES_ARENA_PER_SAMPLE;
    if (arena < (1u << 20)) arena = 1u << 20;
    if (arena > 0xFFFFFF00ull) arena = 0xFFFFFF00ull;                       /* a key holds the offset in 32 bits */
    const size_t counters = 3 * (size_t)id_slots * 8 + 2 * (size_t)cell_slots * 8 + UTK_SAMPLES_MISC_WORDS * 8 + (size_t)id_slots * 4;
    if (hipSetDevice(device) != hipSuccess) return UTREE_E_HIP;
    if (hipMalloc((void **)&t->ids, counters + (size_t)arena) != hipSuccess) { (void)hipGetLastError(); t->ids = NULL; return UTREE_E_NOMEM; }
    t->reads = t->ids + id_slots; t->uncl = t->reads + id_slots;
    t->cells = t->uncl + id_slots; t->misc = t->cells + 2 * (size_t)cell_slots;
    t->index = (uint32_t *)(t->misc + UTK_SAMPLES_MISC_WORDS); t->arena = (uint8_t *)(t->index + id_slots);
    t->arena_cap = arena; t->id_mask = id_slots - 1; t->cell_mask = cell_slots - 1; t->sample_cap = sample_capacity;
    t->n_labels = (uint32_t)n_labels; t->delim = (uint32_t)delim;
    return UTREE_OK;
}

int utree_sample_ids_reset(const utk_samples_tab *t) {
    const size_t cell_slots = (size_t)t->cell_mask + 1;
    if (hipMemset(t->ids, 0, counters_bytes(t)) != hipSuccess) return UTREE_E_HIP;             /* (the arena is written before it is read) */
    if (hipMemset(t->cells, 0xFF, 2 * cell_slots * 8) != hipSuccess) return UTREE_E_HIP;       /* every cell key free (all ones) ... */
    if (hipMemset2D(t->cells + 1, 16, 0, 8, cell_slots) != hipSuccess) return UTREE_E_HIP;     /* ... and every count zero           */
    return UTREE_OK;
}

void utree_sample_ids_free(utk_samples_tab *t) {
    if (t->ids) hipFree(t->ids);
    memset(t, 0, sizeof *t);
}

int utree_sample_ids_check_flags(const utree_sample_ids_text *x, unsigned long long f, const char *more) {
    if (!f && !*more) return UTREE_OK;
    char msg[900];
    snprintf(msg, sizeof msg, "%s:%s%s%s%s%s%s%s%s%s%s%s", x->report,
             f & UTK_SAMPLES_F_TABLE ? " more distinct sample ids than the table holds (raise UTREE_SAMPLE_CAPACITY; is the delimiter right?);" : "",
             f & UTK_SAMPLES_F_ARENA ? " the arena of id bytes is used up (raise UTREE_SAMPLE_CAPACITY; is the delimiter right?);" : "",
             f & UTK_SAMPLES_F_CELLS ? " " : "", f & UTK_SAMPLES_F_CELLS ? x->cells_full : "", f & UTK_SAMPLES_F_CELLS ? ";" : "",
             f & UTK_SAMPLES_F_LABEL ? " a record names a label the database does not have;" : "",
             f & UTK_SAMPLES_F_NAME ? " " : "", f & UTK_SAMPLES_F_NAME ? x->bad_name : "", f & UTK_SAMPLES_F_NAME ? ";" : "",
             f & UTK_SAMPLES_F_CUT ? " a taxon of more than 65532 bytes;" : "", more);
    const size_t l = strlen(msg);
    if (l && msg[l - 1] == ';') msg[l - 1] = 0;
    utree_set_error_text(msg);
    return UTREE_E_DEVICE;
}

void utree_sample_ids_view_free(utree_sample_ids_view *v) {
    const uint64_t n_reads = v->n_reads;
    free(v->slot_key); free(v->ids); free(v->id_off); free(v->reads); free(v->uncl); free(v->sum);
    memset(v, 0, sizeof *v);
    v->n_reads = n_reads;
}

int utree_sample_ids_read(const utk_samples_tab *t, const utree_sample_ids_text *x, const char *more, utree_sample_ids_view *v) {
    memset(v, 0, sizeof *v);
    int rc = UTREE_OK;
    const uint32_t id_slots = t->id_mask + 1, cell_slots = t->cell_mask + 1;
    uint8_t *arena = NULL;
    uint32_t *slot_of = NULL;                                       /* dense index -> slot */
    if (!(v->slot_key = (unsigned long long *)malloc(counters_bytes(t)))) return UTREE_E_NOMEM;
    CHK(hipDeviceSynchronize());
    CHK(hipMemcpy(v->slot_key, t->ids, counters_bytes(t), hipMemcpyDeviceToHost));
    const unsigned long long *ids = v->slot_key, *reads = ids + id_slots, *uncl = reads + id_slots,
                             *cells = uncl + id_slots, *misc = cells + 2 * (size_t)cell_slots;
    const uint32_t *index = (const uint32_t *)(misc + UTK_SAMPLES_MISC_WORDS);
    v->n_reads = misc[0];
    v->cells = cells; v->cell_slots = cell_slots; v->id_slots = id_slots; v->index = index;
    if ((rc = utree_sample_ids_check_flags(x, misc[1], more))) goto fail;
    const uint64_t S = misc[3], used = misc[2];
    if (S > t->sample_cap || used > t->arena_cap) { rc = fail_text(x, "%s: the counters of the %s are inconsistent", x->counters); goto fail; }
    slot_of = (uint32_t *)malloc((S ? S : 1) * sizeof *slot_of);
    arena = (uint8_t *)malloc(used ? used : 1);
    if (!slot_of || !arena) { rc = UTREE_E_NOMEM; goto fail; }
    if (used) CHK(hipMemcpy(arena, t->arena, used, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < S; ++i) slot_of[i] = 0xFFFFFFFFu;
    uint64_t claimed = 0, id_bytes = 0;
    for (uint32_t k = 0; k < id_slots; ++k) {
        if (!ids[k]) continue;
        const uint64_t at = ids[k] >> 32, len = (uint32_t)ids[k] - 1u;
        if (index[k] >= S || slot_of[index[k]] != 0xFFFFFFFFu || at + len > used) { rc = fail_text(x, "%s: a slot of the id table is inconsistent", ""); goto fail; }
        slot_of[index[k]] = k; ++claimed; id_bytes += len;
    }
    if (claimed != S) { rc = fail_text(x, "%s: the id table holds another number of ids than were claimed", ""); goto fail; }
    v->S = (size_t)S; v->id_bytes = (size_t)id_bytes;
    v->ids = (uint8_t *)malloc(id_bytes ? id_bytes : 1);
    v->id_off = (uint64_t *)malloc((S + 1) * 8); v->reads = (uint64_t *)malloc((S ? S : 1) * 8); v->uncl = (uint64_t *)malloc((S ? S : 1) * 8);
    v->sum = (uint64_t *)calloc(S ? S : 1, 8);
    if (!v->ids || !v->id_off || !v->reads || !v->uncl || !v->sum) { rc = UTREE_E_NOMEM; goto fail; }
    uint64_t w = 0;
    for (uint64_t i = 0; i < S; ++i) {
        const uint32_t k = slot_of[i];
        const uint64_t at = ids[k] >> 32, len = (uint32_t)ids[k] - 1u;
        v->id_off[i] = w;
        if (len) memcpy(v->ids + w, arena + at, len);
        w += len;
        v->reads[i] = reads[k]; v->uncl[i] = uncl[k];
    }
    v->id_off[S] = w;
fail:
    free(arena); free(slot_of);
    if (rc) utree_sample_ids_view_free(v);
    return rc;
}

int utree_sample_ids_count(const utree_sample_ids_text *x, utree_sample_ids_view *v, uint32_t slot, uint64_t reads, uint32_t *sample) {
    if (slot >= v->id_slots || !v->slot_key[slot]) return fail_text(x, "%s: a cell names no sample", "");
    *sample = v->index[slot];
    v->sum[*sample] += reads;
    return UTREE_OK;
}

int utree_sample_ids_check_sums(const utree_sample_ids_text *x, const utree_sample_ids_view *v) {
    uint64_t total = 0;
    int bad = 0;
    for (size_t i = 0; i < v->S; ++i) {
        total += v->reads[i];
        bad |= v->reads[i] != v->uncl[i] + v->sum[i];
    }
    return !bad && total == v->n_reads ? UTREE_OK : fail_text(x, "%s: the samples' reads do not add up to the records added", "");
}
