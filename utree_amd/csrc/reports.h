/* reports.h -- the opt-in reports a whole-file search feeds while it runs (reports.c), private.
 *
 * One object per search: for every device handle the profile (UTREE_PROFILE), the coverage handle (UTREE_COVERAGE), the redistribution handle
 * (UTREE_REDISTRIBUTE, UTREE_REDISTRIBUTE_READS), the sample table (UTREE_SAMPLE_TABLE) and / or the per-sample redistribution handle (UTREE_SAMPLE_REDISTRIBUTE) its
 * reads go into.  The pipelines (search.c, search_dev.c) only pass it on, make their classify call through
 * utree_reports_classify and call utree_reports_add; which reports there are, when they are reset, merged and written is decided in reports.c
 * and by search.c's one caller of create / write / free. */
#ifndef UTREE_REPORTS_H
#define UTREE_REPORTS_H
#include "utree_internal.h"

#define UTREE_PROFILE_DEFAULT_CAPACITY (1u << 20)   /* truncated-taxon slots of a search's profiles; UTREE_PROFILE_CAPACITY overrides */
/* (set slots of a search's redistribution handles: UTREE_REDIST_DEFAULT_CAPACITY, include/utree_amd.h; UTREE_REDIST_CAPACITY overrides) */
/* (ids and cells of a search's sample tables: UTREE_SAMPLES_DEFAULT_CAPACITY / _CELLS; UTREE_SAMPLE_CAPACITY / UTREE_SAMPLE_CELLS override) */

typedef struct utree_reports utree_reports;

/* The reports `req` names: *out = NULL when all its report paths are NULL: nothing is allocated and nothing launched.  The request is borrowed
 * until utree_reports_free.  req->max_passes: of the redistribution and of the per-sample redistribution (0: UTREE_REDIST_DEFAULT_PASSES);
 * req->sample_delim: the delimiter byte of the sample table and of the per-sample redistribution (0: '_'); the latter's capacities are the other
 * two reports'.  (utree_search_run has checked the request.) */
int utree_reports_create(const utree_ctr *ctr, utree_dev **devs, int n_dev, const utree_search_request *req, utree_reports **out);
/* do utree_reports_classify or utree_reports_add read the names?  Else a pipeline that frames on the host need not upload them (rep == NULL: no) */
int utree_reports_wants_names(const utree_reports *rep);
/* The GG search's classify call of device handle `g` (= devs[g]) on the batch `v`: utree_classify_batch, or -- when the search writes a
 * redistribution, per sample or not -- that call with the batch's candidate sets added to g's handles.  The view's names are those of the
 * utree_reports_add that follows (read only when utree_reports_wants_names, and then already on the device on the view's stream).  The sets go
 * in at classify time, unlike utree_reports_add's records: a batch that is classified but not committed afterwards is found by
 * utree_reports_write's count of the reads. */
int utree_reports_classify(utree_reports *rep, int g, utree_dev *dev, const utree_batch_view *v, utree_result *d_out, void *d_workspace,
                           size_t workspace_bytes, uint32_t *d_key);
/* does the search write each read's redistributed label (a request's redistribute_reads_path)?  Then the host pipeline gives every classify call
 * a d_key (n_reads keys of device handle g's table come back in it; NULL otherwise) and spools, for every query that prints a line and in the
 * output's order, one record {key, g, name length} followed by the name's bytes (rep == NULL: no) */
int utree_reports_wants_keys(const utree_reports *rep);
typedef struct { uint32_t key, dev, name_len; } utree_spool_rec;
/* the reads of `v`, of device handle `g`, whose output is committed: their records d_res into its profile, records and names into its sample
 * table and -- unless `rank`: the coverage counts the GG search's windows -- the reads into its coverage handle; asynchronous on the view's
 * stream.  The names are read only when utree_reports_wants_names.  rep == NULL: nothing. */
int utree_reports_add(utree_reports *rep, int g, const utree_batch_view *v, const utree_result *d_res, int rank);
/* the search starts the file over: so do the reports */
int utree_reports_reset(utree_reports *rep);
/* after a search that succeeded and read n_reads reads: merges the devices' figures, checks that every read was counted exactly once and writes
 * the files: the coverage, the redistribution, the redistributed reads (one solve serves both), the sample table, the per-sample redistribution,
 * the profile.  0, UTREE_E_PROFILE (the profile, the redistribution or the redistributed reads, the sample table or the per-sample
 * redistribution: those have no code of their own) or UTREE_E_COVERAGE (the profile's failure wins, then the redistribution's, the sample
 * table's, the per-sample redistribution's); utree_last_hip_error says why.  spool_path: the complete spool of a search whose
 * utree_reports_wants_keys (NULL with spool_err = why there is none: that report then fails with those words) */
int utree_reports_write(utree_reports *rep, const utree_ctr *ctr, uint64_t n_reads, const char *spool_path, const char *spool_err);
void utree_reports_free(utree_reports *rep);

#endif
