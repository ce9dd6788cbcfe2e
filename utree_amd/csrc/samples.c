/* samples.c -- per-sample taxon tables of multiplexed reads (include/utree_amd.h: utree_samples_*).
 *
 * A combined reads file names its records <sample>_<n>; a read's sample id is its name up to the last delimiter byte, its taxon the second
 * column of its output line.  The ids are interned and the (sample, taxon) cells counted on the device while the chunk is there
 * (samples_kernels.hip); here the handle over the id table (sample_ids.c), the read-back -- sample ids, per-sample reads / unclassified, cells
 * keyed (sample, label, cut) -- and the host-only writer, which lays any number of read-backs side by side for the matrix writer (taxon_table.c):
 * that merges samples by id text and taxa by printed text, exactly as utree_profile_write merges.
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
#include "samples.h"
#include "taxon_table.h"

struct utree_samples {
    int device, n_cu;
    utk_samples_tab tab;                /* one device block (sample_ids.c) */
};

static const utree_sample_ids_text TEXT = {"sample table", "id table", "the table of (sample, taxon) cells is full (raise UTREE_SAMPLE_CELLS)",
                                           "a name lies outside its chunk"};

int utree_samples_create(utree_dev *dev, uint32_t sample_capacity, uint32_t cell_capacity, int delim, utree_samples **out) {
    if (!dev || !out) return UTREE_E_ARG;
    *out = NULL;
    utree_samples *s = (utree_samples *)calloc(1, sizeof *s);
    if (!s) return UTREE_E_NOMEM;
    s->device = dev->device; s->n_cu = dev->n_cu;
    int rc = utree_sample_ids_create(&s->tab, s->device, sample_capacity, cell_capacity, delim, dev->hdr.n_labels);
    if (!rc) rc = utree_samples_reset(s);
    if (rc) { utree_samples_free(s); return rc; }
    *out = s;
    return UTREE_OK;
}

int utree_samples_reset(utree_samples *s) {
    if (!s) return UTREE_E_ARG;
    if (hipSetDevice(s->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return UTREE_E_HIP;   /* adds in flight on any stream */
    const int rc = utree_sample_ids_reset(&s->tab);
    if (rc) return rc;
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
    if (s->tab.ids) { hipSetDevice(s->device); hipDeviceSynchronize(); utree_sample_ids_free(&s->tab); }
    free(s);
}

int utree_samples_read(utree_samples *s, uint8_t *h_ids, size_t id_cap, uint64_t *h_id_off, uint64_t *h_reads, uint64_t *h_unclassified,
                       size_t sample_cap, utree_samples_cell *h_cells, size_t cell_cap, size_t *n_samples, size_t *n_id_bytes, size_t *n_cells,
                       uint64_t *n_reads) {
    if (!s || !n_samples || !n_id_bytes || !n_cells || (id_cap && !h_ids) || (sample_cap && (!h_id_off || !h_reads || !h_unclassified)) ||
        (cell_cap && !h_cells)) return UTREE_E_ARG;
    *n_samples = 0; *n_id_bytes = 0; *n_cells = 0;
    if (n_reads) *n_reads = 0;
    if (hipSetDevice(s->device) != hipSuccess) return UTREE_E_HIP;
    utree_sample_ids_view v;
    int rc = utree_sample_ids_read(&s->tab, &TEXT, "", &v);
    if (n_reads) *n_reads = v.n_reads;
    if (rc) return rc;
    const size_t S = v.S;
    size_t nc = 0;
    for (uint32_t c = 0; c < v.cell_slots; ++c) nc += v.cells[2 * (size_t)c] != ~0ull && v.cells[2 * (size_t)c + 1];
    *n_samples = S; *n_id_bytes = v.id_bytes; *n_cells = nc;
    if (S > sample_cap || v.id_bytes > id_cap || nc > cell_cap) { rc = UTREE_E_ARG; goto done; }     /* the sizes are set: call again with room */
    if (v.id_bytes) memcpy(h_ids, v.ids, v.id_bytes);
    if (h_id_off) memcpy(h_id_off, v.id_off, (S + 1) * 8);          /* (sample_cap + 1 entries) */
    if (S) { memcpy(h_reads, v.reads, S * 8); memcpy(h_unclassified, v.uncl, S * 8); }
    size_t q = 0;
    for (uint32_t c = 0; c < v.cell_slots; ++c) {
        const unsigned long long key = v.cells[2 * (size_t)c], cnt = v.cells[2 * (size_t)c + 1];
        if (key == ~0ull || !cnt) continue;
        const uint32_t cut = (uint32_t)(key & 0xFFFFu);
        if ((rc = utree_sample_ids_count(&TEXT, &v, (uint32_t)(key >> (UTK_SAMPLES_LABEL_BITS + 16u)), cnt, &h_cells[q].sample))) goto done;
        h_cells[q].label = (uint32_t)(key >> 16) & ((1u << UTK_SAMPLES_LABEL_BITS) - 1u);
        h_cells[q].cut = cut == UTK_SAMPLES_CUT_WHOLE ? -2 : cut == UTK_SAMPLES_CUT_EMPTY ? -1 : (int32_t)cut;
        h_cells[q].pad = 0; h_cells[q].reads = cnt;
        ++q;
    }
    rc = utree_sample_ids_check_sums(&TEXT, &v);                   /* or the table is not written */
done:
    utree_sample_ids_view_free(&v);
    return rc;
}

/* ---- host: any number of read-backs -> one table ----------------------------------------------------------------------------- */
int utree_samples_write(const utree_ctr *ctr, const utree_samples_table *tabs, size_t n_tabs, const char *path) {
    if (!ctr || (n_tabs && !tabs) || !path) return UTREE_E_ARG;
    size_t ns = 0, nc = 0;
    uint64_t N = 0;
    for (size_t t = 0; t < n_tabs; ++t) {
        if ((tabs[t].n_samples && (!tabs[t].id_off || !tabs[t].reads || !tabs[t].unclassified)) || (tabs[t].n_cells && !tabs[t].cells)) return UTREE_E_ARG;
        ns += tabs[t].n_samples; nc += tabs[t].n_cells; N += tabs[t].n_reads;
    }
    utree_matrix_col *col = (utree_matrix_col *)calloc(ns ? ns : 1, sizeof *col);       /* one per (read-back, sample); the writer merges those of one id */
    utree_matrix_cell *ce = (utree_matrix_cell *)calloc(nc ? nc : 1, sizeof *ce);
    int rc = UTREE_OK;
    if (!col || !ce) { rc = UTREE_E_NOMEM; goto done; }
    size_t k = 0, q = 0;
    uint64_t total = 0, G = 0;
    for (size_t t = 0; t < n_tabs; ++t) {
        const size_t first = k;
        for (size_t i = 0; i < tabs[t].n_samples; ++i, ++k) {
            if (tabs[t].id_off[i + 1] < tabs[t].id_off[i]) { rc = UTREE_E_ARG; goto done; }
            col[k].len = tabs[t].id_off[i + 1] - tabs[t].id_off[i];
            col[k].s = col[k].len ? tabs[t].ids + tabs[t].id_off[i] : (const uint8_t *)"";
            col[k].reads = tabs[t].reads[i]; col[k].uncl = tabs[t].unclassified[i];
            total += tabs[t].reads[i];
        }
        /* the cells: the text each prints (utree_profile_write's rule), its column */
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
            ce[q].s = s; ce[q].len = len; ce[q].col = (uint32_t)(first + c->sample); ce[q].reads = c->reads;
            G += c->reads;
            ++q;
        }
    }
    if (total != N) { rc = UTREE_E_ARG; goto done; }                     /* the samples' reads are the reads */
    char header[128];
    snprintf(header, sizeof header, "# reads\t%llu\tclassified\t%llu\tunclassified\t%llu", (unsigned long long)N, (unsigned long long)G, (unsigned long long)(N - G));
    rc = utree_sample_matrix_write(header, col, ns, 1, NULL, 0, ce, q, path);
done:
    free(col); free(ce);
    return rc;
}
