/* reports.c -- the opt-in reports of one whole-file search (reports.h): a profile (profile.c), a coverage handle (coverage.c), a redistribution
 * handle (redist.c), a sample table (samples.c) and / or a per-sample redistribution handle (sredist.c) per device handle, fed chunk by chunk, merged and written when the search has succeeded. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ctr_host.h"
#include "dev_image.h"
#include "reports.h"

struct utree_reports {
    int n_dev;
    const char *profile_path, *coverage_path, *redist_path, *samples_path, *sredist_path;
    uint32_t redist_passes;
    struct { utree_profile *prof; utree_coverage *cov; utree_redist *rd; utree_samples *smp; utree_sredist *srd; } dev[];      /* NULL: the search writes no such report */
};

int utree_reports_create(const utree_ctr *ctr, utree_dev **devs, int n_dev, const utree_search_request *req, utree_reports **out) {
    *out = NULL;
    if (!req->profile_path && !req->coverage_path && !req->redistribute_path && !req->samples_path && !req->sample_redistribute_path) return UTREE_OK;
    utree_reports *rep = (utree_reports *)calloc(1, sizeof *rep + (size_t)n_dev * sizeof rep->dev[0]);
    if (!rep) return UTREE_E_NOMEM;
    rep->n_dev = n_dev; rep->profile_path = req->profile_path; rep->coverage_path = req->coverage_path; rep->redist_path = req->redistribute_path;
    rep->samples_path = req->samples_path; rep->sredist_path = req->sample_redistribute_path;
    rep->redist_passes = req->max_passes ? req->max_passes : UTREE_REDIST_DEFAULT_PASSES;
    const int delim = req->sample_delim ? req->sample_delim : '_';
    const char *e = getenv("UTREE_PROFILE_CAPACITY");
    const uint32_t cap = e && atoll(e) >= 1 && atoll(e) <= (1ll << 30) ? (uint32_t)atoll(e) : UTREE_PROFILE_DEFAULT_CAPACITY;
    int rc = UTREE_OK;
    for (int g = 0; rep->profile_path && g < n_dev && !rc; ++g) rc = utree_profile_create(devs[g], cap, &rep->dev[g].prof);
    for (int g = 0; rep->coverage_path && g < n_dev && !rc; ++g) rc = utree_coverage_create(ctr, devs[g], NULL, NULL, &rep->dev[g].cov);
    const char *er = getenv("UTREE_REDIST_CAPACITY");
    const uint32_t rcap = er && atoll(er) >= 1 && atoll(er) <= (1ll << 28) ? (uint32_t)atoll(er) : UTREE_REDIST_DEFAULT_CAPACITY;
    for (int g = 0; rep->redist_path && g < n_dev && !rc; ++g) rc = utree_redist_create(devs[g], rcap, &rep->dev[g].rd);
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
                           size_t workspace_bytes) {
    return utree_classify_view(dev, v, d_out, d_workspace, workspace_bytes, rep ? rep->dev[g].rd : NULL, rep ? rep->dev[g].srd : NULL);   /* (each batch feeds both when both are written) */
}

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

/* merges the devices' handles into the first, checks that n_reads_expected reads were added (else UTREE_E_DEVICE), solves and writes the file */
static int write_redist(const utree_reports *rep, const utree_ctr *ctr, uint64_t n_reads_expected) {
    const char *path = rep->redist_path;
    int rc = UTREE_OK;
    size_t k = 0;
    uint64_t reads = 0, ambiguous = 0;
    uint32_t passes = 0;
    utree_redist_entry *e = (utree_redist_entry *)malloc(((size_t)ctr->info.n_labels + 1) * sizeof *e);
    if (!e) return UTREE_E_NOMEM;
    for (int g = 1; g < rep->n_dev && !rc; ++g) rc = utree_redist_merge(rep->dev[0].rd, rep->dev[g].rd);
    if (!rc) rc = utree_redist_reads(rep->dev[0].rd, &reads);
    char msg[400];
    if (rc == UTREE_E_DEVICE) snprintf(msg, sizeof msg, "redistribution %s: %s", path, utree_last_hip_error());
    else if (rc) snprintf(msg, sizeof msg, "redistribution %s: the sets could not be merged and read back (%s)", path, utree_strerror(rc));
    else if (reads != n_reads_expected) {                          /* every read added exactly once, or no file */
        snprintf(msg, sizeof msg, "redistribution %s: %llu reads added, the search read %llu", path, (unsigned long long)reads,
                 (unsigned long long)n_reads_expected);
        rc = UTREE_E_DEVICE;
    } else if ((rc = utree_redist_solve(rep->dev[0].rd, rep->redist_passes, e, ctr->info.n_labels, &k, &passes, &ambiguous)))
        snprintf(msg, sizeof msg, "redistribution %s: the passes failed (%s)", path, utree_strerror(rc));
    else if ((rc = utree_redist_write(ctr, e, k, reads, ambiguous, passes, path)))
        snprintf(msg, sizeof msg, "redistribution %s: cannot write the file (%s)", path, utree_strerror(rc));
    if (rc) utree_set_error_text(msg);
    free(e);
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

int utree_reports_write(utree_reports *rep, const utree_ctr *ctr, uint64_t n_reads) {
    if (!rep) return UTREE_OK;
    const int ce = rep->coverage_path ? write_coverage(rep, ctr, n_reads) : UTREE_OK;
    char keep[1200];
    const int re = rep->redist_path ? write_redist(rep, ctr, n_reads) : UTREE_OK;
    if (re) snprintf(keep, sizeof keep, "%s", utree_last_hip_error());
    const int se = rep->samples_path ? write_samples(rep, ctr, n_reads) : UTREE_OK;
    if (se && !re) snprintf(keep, sizeof keep, "%s", utree_last_hip_error());          /* (the redistribution's failure wins) */
    const int sre = rep->sredist_path ? write_sredist(rep, ctr, n_reads) : UTREE_OK;
    if (sre && !re && !se) snprintf(keep, sizeof keep, "%s", utree_last_hip_error());  /* (... then the sample table's) */
    if (rep->profile_path && write_profile(rep, ctr, n_reads)) return UTREE_E_PROFILE;
    if (re || se || sre) { utree_set_error_text(keep); return UTREE_E_PROFILE; }      /* (no code of their own; a profile that was written sets no text) */
    return ce ? UTREE_E_COVERAGE : UTREE_OK;      /* (a profile that was written sets no text: the coverage's stands) */
}
