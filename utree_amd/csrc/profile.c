/* profile.c -- per-taxon read-count profiles (include/utree_amd.h: utree_profile_*).
 *
 * A read's taxon is the second column of its output line (itree.c:982, 1002 rank-specific; 1032, 1040, 1087-1096 GG); a read without a
 * line is unclassified.  The counters sit on the device (profile_kernels.hip) and are read back as (label, cut, reads) entries; the text
 * of an entry is what the line prints, so entries of any number of devices are merged by that text here, rolled up over the ';'-prefixes
 * of every taxon and written as
 *
 *     # reads\t<N>\tclassified\t<G>\tunclassified\t<N-G>\n
 *     # taxon\tassigned\tclade\n
 *     <taxon>\t<assigned>\t<clade>\n      one row per taxon and ';'-prefix, in unsigned bytewise order (shorter first on a tie)
 */
#define _GNU_SOURCE
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ctr_host.h"
#include "dev_image.h"
#include "profile.h"
#include "taxon_table.h"

struct utree_profile {
    int device, n_cu;
    uint32_t n_labels, cap;             /* cap: slots of the truncated-taxon table, a power of two */
    unsigned long long *d_mem;          /* d_whole[n_labels] | d_table[2 * cap] | d_misc[4]       */
    unsigned long long *d_whole, *d_table, *d_misc;
    size_t bytes;
};

int utree_profile_create(utree_dev *dev, uint32_t truncated_capacity, utree_profile **out) {
    if (!dev || !out || !truncated_capacity || truncated_capacity > (1u << 30)) return UTREE_E_ARG;
    *out = NULL;
    uint32_t cap = 16;
    while (cap < truncated_capacity) cap <<= 1;
    utree_profile *p = (utree_profile *)calloc(1, sizeof *p);
    if (!p) return UTREE_E_NOMEM;
    p->device = dev->device; p->n_cu = dev->n_cu; p->n_labels = dev->hdr.n_labels; p->cap = cap;
    p->bytes = ((size_t)p->n_labels + 2 * (size_t)cap + 4) * 8;
    if (hipSetDevice(p->device) != hipSuccess) { free(p); return UTREE_E_HIP; }
    if (hipMalloc((void **)&p->d_mem, p->bytes) != hipSuccess) { (void)hipGetLastError(); free(p); return UTREE_E_NOMEM; }
    p->d_whole = p->d_mem; p->d_table = p->d_whole + p->n_labels; p->d_misc = p->d_table + 2 * (size_t)cap;
    int rc = utree_profile_reset(p);
    if (rc) { utree_profile_free(p); return rc; }
    *out = p;
    return UTREE_OK;
}

int utree_profile_reset(utree_profile *p) {
    if (!p) return UTREE_E_ARG;
    if (hipSetDevice(p->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return UTREE_E_HIP;   /* adds in flight on any stream */
    if (hipMemset(p->d_whole, 0, (size_t)p->n_labels * 8) != hipSuccess) return UTREE_E_HIP;
    if (hipMemset(p->d_table, 0xFF, 2 * (size_t)p->cap * 8) != hipSuccess) return UTREE_E_HIP;    /* every key free (all ones) ...   */
    if (hipMemset2D(p->d_table + 1, 16, 0, 8, p->cap) != hipSuccess) return UTREE_E_HIP;         /* ... and every count zero        */
    if (hipMemset(p->d_misc, 0, 4 * 8) != hipSuccess) return UTREE_E_HIP;
    return hipDeviceSynchronize() == hipSuccess ? UTREE_OK : UTREE_E_HIP;
}

int utree_profile_add(utree_profile *p, const utree_result *d_res, uint32_t n_reads, void *stream) {
    if (!p || (!d_res && n_reads)) return UTREE_E_ARG;
    if (!n_reads) return UTREE_OK;
    if (hipSetDevice(p->device) != hipSuccess) return UTREE_E_HIP;
    return utk_profile_add(d_res, n_reads, p->n_labels, p->d_whole, p->d_table, p->cap - 1, p->d_misc, p->n_cu, stream) ? UTREE_E_HIP
                                                                                                                          : UTREE_OK;
}

size_t utree_profile_max_entries(const utree_profile *p) { return p ? (size_t)p->n_labels + p->cap + 1 : 0; }

int utree_profile_read(utree_profile *p, utree_profile_entry *h, size_t cap, size_t *n, uint64_t *n_reads, uint64_t *n_classified) {
    if (!p || !n || (cap && !h)) return UTREE_E_ARG;
    *n = 0;
    unsigned long long *m = (unsigned long long *)malloc(p->bytes);
    if (!m) return UTREE_E_NOMEM;
    if (hipSetDevice(p->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(m, p->d_mem, p->bytes, hipMemcpyDeviceToHost) != hipSuccess) { free(m); return UTREE_E_HIP; }
    const unsigned long long *whole = m, *table = m + p->n_labels, *misc = table + 2 * (size_t)p->cap;
    size_t k = 0;
    int rc = UTREE_OK;
#define PUT(l_, c_, r_) do { if (k < cap) { h[k].label = (l_); h[k].cut = (c_); h[k].reads = (r_); } ++k; } while (0)
    if (misc[2]) PUT(0, -1, misc[2]);
    for (uint32_t i = 0; i < p->n_labels; ++i) if (whole[i]) PUT(i, -2, whole[i]);
    for (uint32_t i = 0; i < p->cap; ++i)
        if (table[2 * i] != ~0ull && table[2 * i + 1]) PUT((uint32_t)(table[2 * i] >> 32), (int32_t)(uint32_t)table[2 * i], table[2 * i + 1]);
#undef PUT
    *n = k;
    if (n_reads) *n_reads = misc[0];
    if (n_classified) *n_classified = misc[0] - misc[1];
    if (k > cap) rc = UTREE_E_ARG;
    if (misc[3]) rc = UTREE_E_DEVICE;               /* PROF_F_FULL: the table was too small; PROF_F_LABEL: a record names no label */
    free(m);
    return rc;
}

void utree_profile_free(utree_profile *p) {
    if (!p) return;
    if (p->d_mem) { hipSetDevice(p->device); hipDeviceSynchronize(); hipFree(p->d_mem); }
    free(p);
}

/* ---- host: the entries' texts and counts as rows of the taxon table (taxon_table.c) ------------------------------------- */
int utree_profile_write(const utree_ctr *ctr, const utree_profile_entry *e, size_t n, uint64_t n_reads, const char *path) {
    if (!ctr || (n && !e) || !path) return UTREE_E_ARG;
    uint64_t classified = 0;
    utree_taxon_row *t = (utree_taxon_row *)calloc(n ? n : 1, sizeof *t);
    if (!t) return UTREE_E_NOMEM;
    size_t nt = 0;
    for (size_t i = 0; i < n; ++i) {                       /* the text each entry's lines print (utree_format_records, rank: the label) */
        if (!e[i].reads) continue;
        uint32_t len = 0;
        const char *s = "";
        if (e[i].cut != -1) {
            if (e[i].label >= ctr->info.n_labels) { free(t); return UTREE_E_ARG; }
            s = ctr->labels[e[i].label];
            len = ctr->label_len[e[i].label];
            if (e[i].cut >= 0 && (uint32_t)e[i].cut < len) len = (uint32_t)e[i].cut;
        }
        t[nt].s = s; t[nt].len = len; t[nt].own[0] = e[i].reads;
        classified += e[i].reads;
        ++nt;
    }
    char header[256];
    snprintf(header, sizeof header, "# reads\t%llu\tclassified\t%llu\tunclassified\t%llu\n# taxon\tassigned\tclade\n", (unsigned long long)n_reads,
             (unsigned long long)classified, (unsigned long long)(n_reads - classified));
    const int rc = utree_taxon_table_write(t, nt, 1, 0, header, path);     /* one figure, the reads: every row is an assigned taxon or a prefix of one */
    free(t);
    return rc;
}
