/* coverage.c -- distinct database k-mers covered per taxon (include/utree_amd.h: utree_coverage_*).
 *
 * A window of a read is a hit when XT_getIX32 (itree.c:720-730, 699-707) ends on a record whose stored label index is < n_labels (929); the
 * hit's node is that record's position in the dump.  Per label: db_kmers = records of the dump that store it, hits = hit windows, covered =
 * distinct nodes among them.  The handle keeps the .ctr's bin table and node dump as the file holds them in HBM, plus a bitmap of n_nodes bits
 * and one hit counter per label (coverage_kernels.hip); entries of all labels are read back, merged by label text, rolled up over the
 * ';'-prefixes of every hit taxon and written as
 *
 *     # reads\t<N>\thits\t<H>\tcovered\t<D>\tdb_kmers\t<T>\n
 *     # taxon\tdb_kmers\tcovered\thits\tclade_db_kmers\tclade_covered\tclade_hits\n
 *     <taxon>\t...\n      one row per hit taxon and ';'-prefix of one, in unsigned bytewise order (shorter first on a tie)
 */
#define _GNU_SOURCE
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "ctr_host.h"
#include "dev_image.h"
#include "coverage.h"
#include "taxon_table.h"

struct utree_coverage {
    int device, n_cu;
    utk_cov_db db;                      /* recs / binix point into d_recs / d_binix                     */
    void *d_recs, *d_binix;
    size_t recs_bytes, binix_bytes, bitmap_words;
    uint32_t *d_bitmap;
    unsigned long long *d_counts;       /* d_hits[n_labels] | d_db[n_labels] | d_cov[n_labels] | reads */
    uint32_t n_labels;
};

static size_t recs_alloc_bytes(const utree_ctr_info *in) { return (((size_t)in->n_nodes * in->SZ + 7) & ~(size_t)7) + UTK_COV_PAD; }
static size_t bitmap_words(const utree_ctr_info *in) { return (size_t)((in->n_nodes + 31) / 32) + 1; }

size_t utree_coverage_bytes(const utree_ctr *ctr) {
    if (!ctr) return 0;
    const utree_ctr_info *in = &ctr->info;
    return recs_alloc_bytes(in) + (size_t)UTREE_NUMBINS * in->binix_width + bitmap_words(in) * 4 + (3 * (size_t)in->n_labels + 1) * 8;
}

#define CHK(x) do { if ((x) != hipSuccess) { utree_dev_set_hip_error((int)hipGetLastError(), #x); rc = UTREE_E_HIP; goto fail; } } while (0)

/* the node dump from the .ctr file (or the host copy) into c->d_recs, through two pinned buffers */
static int stream_dump(const utree_ctr *ctr, utree_coverage *c) {
    int rc = UTREE_OK, fd = -1;
    const size_t total = (size_t)ctr->info.n_nodes * ctr->info.SZ, piece = (size_t)64 << 20;
    void *h_pin[2] = {NULL, NULL};
    hipEvent_t ev[2] = {NULL, NULL};
    if (!total) return UTREE_OK;
    if (ctr->h_records) {
        CHK(hipMemcpy(c->d_recs, ctr->h_records, total, hipMemcpyHostToDevice));
        return UTREE_OK;
    }
    for (int i = 0; i < 2; ++i) {
        CHK(hipHostMalloc(&h_pin[i], total < piece ? total : piece, hipHostMallocDefault));
        CHK(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
    }
    fd = open(ctr->path, O_RDONLY);
    if (fd < 0) { rc = UTREE_E_IO; goto fail; }
    size_t done = 0;
    for (int slot = 0; done < total; slot ^= 1) {
        const size_t bytes = total - done < piece ? total - done : piece;
        CHK(hipEventSynchronize(ev[slot]));
        if (utree_pread_team(fd, h_pin[slot], bytes, ctr->records_file_off + done, 8)) { rc = UTREE_E_FORMAT; goto fail; }
        CHK(hipMemcpyAsync((char *)c->d_recs + done, h_pin[slot], bytes, hipMemcpyHostToDevice, NULL));
        CHK(hipEventRecord(ev[slot], NULL));
        done += bytes;
    }
    CHK(hipDeviceSynchronize());
fail:
    if (fd >= 0) close(fd);
    (void)hipDeviceSynchronize();
    for (int i = 0; i < 2; ++i) {
        if (h_pin[i]) hipHostFree(h_pin[i]);
        if (ev[i]) hipEventDestroy(ev[i]);
    }
    return rc;
}

int utree_coverage_create(const utree_ctr *ctr, utree_dev *dev, const void *d_binix, const void *d_records, utree_coverage **out) {
    if (!ctr || !dev || !out || (!d_binix) != (!d_records)) return UTREE_E_ARG;
    *out = NULL;
    const utree_ctr_info *in = &ctr->info;
    if (!(in->W == 4 || in->W == 8 || in->W == 16) || !(in->I == 2 || in->I == 4)) return UTREE_E_UNSUPPORTED;
    if (!d_records && !ctr->path && !ctr->h_records && in->n_nodes) return UTREE_E_ARG;
    int rc = UTREE_OK;
    utree_coverage *c = (utree_coverage *)calloc(1, sizeof *c);
    if (!c) return UTREE_E_NOMEM;
    c->device = dev->device; c->n_cu = dev->n_cu; c->n_labels = in->n_labels;
    c->recs_bytes = recs_alloc_bytes(in);
    c->binix_bytes = (size_t)UTREE_NUMBINS * in->binix_width;
    c->bitmap_words = bitmap_words(in);
    if (hipSetDevice(c->device) != hipSuccess) { free(c); return UTREE_E_HIP; }
    if (hipMalloc(&c->d_recs, c->recs_bytes) != hipSuccess || hipMalloc(&c->d_binix, c->binix_bytes) != hipSuccess ||
        hipMalloc((void **)&c->d_bitmap, c->bitmap_words * 4) != hipSuccess ||
        hipMalloc((void **)&c->d_counts, (3 * (size_t)c->n_labels + 1) * 8) != hipSuccess) {
        (void)hipGetLastError();
        utree_coverage_free(c);
        return UTREE_E_NOMEM;
    }
    const size_t total = (size_t)in->n_nodes * in->SZ;
    CHK(hipMemset((char *)c->d_recs + (total & ~(size_t)7), 0, c->recs_bytes - (total & ~(size_t)7)));     /* the padding reads as zeros */
    if (d_records) {
        CHK(hipMemcpy(c->d_recs, d_records, total, hipMemcpyDeviceToDevice));
        CHK(hipMemcpy(c->d_binix, d_binix, c->binix_bytes, hipMemcpyDeviceToDevice));
    } else {
        if ((rc = stream_dump(ctr, c))) goto fail;
        CHK(hipMemcpy(c->d_binix, ctr->binix_raw, c->binix_bytes, hipMemcpyHostToDevice));
    }
    c->db.recs = (const uint64_t *)c->d_recs; c->db.binix = c->d_binix; c->db.n_nodes = in->n_nodes;
    c->db.W = in->W; c->db.I = in->I; c->db.n_labels = in->n_labels; c->db.off64 = in->binix_width == 8;
    if ((rc = utree_coverage_reset(c))) goto fail;
    *out = c;
    return UTREE_OK;
fail:
    utree_coverage_free(c);
    return rc;
}

int utree_coverage_reset(utree_coverage *c) {
    if (!c) return UTREE_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return UTREE_E_HIP;    /* adds in flight on any stream */
    if (hipMemset(c->d_bitmap, 0, c->bitmap_words * 4) != hipSuccess) return UTREE_E_HIP;
    if (hipMemset(c->d_counts, 0, (3 * (size_t)c->n_labels + 1) * 8) != hipSuccess) return UTREE_E_HIP;
    return hipDeviceSynchronize() == hipSuccess ? UTREE_OK : UTREE_E_HIP;
}

int utree_coverage_add(utree_coverage *c, const uint8_t *d_bases, const uint64_t *d_off, const uint32_t *d_len, uint32_t n_reads, int do_rc,
                       void *stream) {
    if (!c || (n_reads && (!d_bases || !d_off || !d_len))) return UTREE_E_ARG;
    if (!n_reads) return UTREE_OK;
    if (hipSetDevice(c->device) != hipSuccess) return UTREE_E_HIP;
    return utk_coverage_add(&c->db, d_bases, d_off, d_len, n_reads, do_rc, c->d_bitmap, c->d_counts, c->d_counts + 3 * (size_t)c->n_labels, stream)
               ? UTREE_E_HIP : UTREE_OK;
}

int utree_coverage_merge(utree_coverage *dst, utree_coverage *src) {
    if (!dst || !src || dst == src) return UTREE_E_ARG;
    if (dst->n_labels != src->n_labels || dst->db.n_nodes != src->db.n_nodes || dst->db.W != src->db.W || dst->db.I != src->db.I) return UTREE_E_ARG;
    int rc = UTREE_OK;
    void *tmp = NULL;
    const size_t bm = dst->bitmap_words * 4, cn = (size_t)dst->n_labels * 8;
    if (hipSetDevice(src->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return UTREE_E_HIP;
    if (hipSetDevice(dst->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return UTREE_E_HIP;
    if (hipMalloc(&tmp, bm + cn + 8) != hipSuccess) { (void)hipGetLastError(); return UTREE_E_NOMEM; }
    /* the source's bitmap, hit counters and read count come over in one piece each; the other counters are made by utree_coverage_read */
    CHK(hipMemcpyPeer(tmp, dst->device, src->d_bitmap, src->device, bm));
    CHK(hipMemcpyPeer((char *)tmp + bm, dst->device, src->d_counts, src->device, cn));
    CHK(hipMemcpyPeer((char *)tmp + bm + cn, dst->device, src->d_counts + 3 * (size_t)src->n_labels, src->device, 8));
    if (utk_coverage_or(dst->d_bitmap, (const uint32_t *)tmp, dst->bitmap_words, NULL) ||
        utk_coverage_sum(dst->d_counts, (const unsigned long long *)((char *)tmp + bm), dst->n_labels, NULL) ||
        utk_coverage_sum(dst->d_counts + 3 * (size_t)dst->n_labels, (const unsigned long long *)((char *)tmp + bm + cn), 1, NULL)) {
        rc = UTREE_E_HIP;
        goto fail;
    }
    CHK(hipDeviceSynchronize());
fail:
    (void)hipDeviceSynchronize();
    hipFree(tmp);
    return rc;
}

int utree_coverage_read(utree_coverage *c, utree_coverage_entry *h, size_t cap, size_t *n, uint64_t *n_reads, uint64_t *n_hits) {
    if (!c || !n || (cap && !h)) return UTREE_E_ARG;
    *n = c->n_labels;
    if (cap < c->n_labels) return UTREE_E_ARG;
    const size_t nl = c->n_labels, words = 3 * nl + 1;
    unsigned long long *m = (unsigned long long *)malloc(words * 8);
    if (!m) return UTREE_E_NOMEM;
    int rc = UTREE_OK;
    CHK(hipSetDevice(c->device));
    CHK(hipDeviceSynchronize());
    CHK(hipMemset(c->d_counts + nl, 0, 2 * nl * 8));
    if (utk_coverage_count(&c->db, c->d_bitmap, c->d_counts + nl, c->d_counts + 2 * nl, c->n_cu, NULL)) { rc = UTREE_E_HIP; goto fail; }
    CHK(hipMemcpy(m, c->d_counts, words * 8, hipMemcpyDeviceToHost));
    uint64_t hits = 0;
    for (size_t i = 0; i < nl; ++i) {
        h[i].label = (uint32_t)i; h[i].pad = 0;
        h[i].hits = m[i]; h[i].db_kmers = m[nl + i]; h[i].covered = m[2 * nl + i];
        hits += m[i];
    }
    if (n_reads) *n_reads = m[3 * nl];
    if (n_hits) *n_hits = hits;
fail:
    free(m);
    return rc;
}

void utree_coverage_free(utree_coverage *c) {
    if (!c) return;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    if (c->d_recs) hipFree(c->d_recs);
    if (c->d_binix) hipFree(c->d_binix);
    if (c->d_bitmap) hipFree(c->d_bitmap);
    if (c->d_counts) hipFree(c->d_counts);
    free(c);
}

/* ---- host: every label's figures as rows of the taxon table (taxon_table.c) ----------------------------------------------- */
int utree_coverage_write(const utree_ctr *ctr, const utree_coverage_entry *e, size_t n, uint64_t n_reads, const char *path) {
    if (!ctr || (n && !e) || !path) return UTREE_E_ARG;
    uint64_t tot[3] = {0, 0, 0};
    utree_taxon_row *t = (utree_taxon_row *)calloc(n ? n : 1, sizeof *t);      /* own: {db_kmers, covered, hits} */
    if (!t) return UTREE_E_NOMEM;
    for (size_t i = 0; i < n; ++i) {                        /* every label of the database, hit or not */
        if (e[i].label >= ctr->info.n_labels) { free(t); return UTREE_E_ARG; }
        t[i].s = ctr->labels[e[i].label]; t[i].len = ctr->label_len[e[i].label];
        t[i].own[0] = e[i].db_kmers; t[i].own[1] = e[i].covered; t[i].own[2] = e[i].hits;
        for (int q = 0; q < 3; ++q) tot[q] += t[i].own[q];
    }
    char header[320];
    snprintf(header, sizeof header, "# reads\t%llu\thits\t%llu\tcovered\t%llu\tdb_kmers\t%llu\n"
                                    "# taxon\tdb_kmers\tcovered\thits\tclade_db_kmers\tclade_covered\tclade_hits\n",
             (unsigned long long)n_reads, (unsigned long long)tot[2], (unsigned long long)tot[1], (unsigned long long)tot[0]);
    const int rc = utree_taxon_table_write(t, n, 3, 2, header, path);       /* the rows are the HIT taxa and their prefixes; the clades sum over all labels */
    free(t);
    return rc;
}
