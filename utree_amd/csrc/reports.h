/* reports.h -- the opt-in reports a whole-file search feeds while it runs (reports.c), private.
 *
 * One object per search: for every device handle the profile (UTREE_PROFILE), the coverage handle (UTREE_COVERAGE), the redistribution handle
 * (UTREE_REDISTRIBUTE), the sample table (UTREE_SAMPLE_TABLE) and / or the per-sample redistribution handle (UTREE_SAMPLE_REDISTRIBUTE) its
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

/* *out = NULL when all paths are NULL: nothing is allocated and nothing launched.  The paths are borrowed until utree_reports_free.
 * redist_passes: max_passes of the redistribution and of the per-sample redistribution (0: UTREE_REDIST_DEFAULT_PASSES); samples_delim: the
 * delimiter byte of the sample table and of the per-sample redistribution (0: '_'); the latter's capacities are the other two reports'. */
int utree_reports_create(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *profile_path, const char *coverage_path,
                         const char *redist_path, uint32_t redist_passes, const char *samples_path, int samples_delim, const char *sredist_path,
                         utree_reports **out);
/* do utree_reports_classify or utree_reports_add read the names?  Else a pipeline that frames on the host need not upload them (rep == NULL: no) */
int utree_reports_wants_names(const utree_reports *rep);
/* The GG search's classify call of device handle `g` (= devs[g]): utree_classify_batch, or -- when the search writes a redistribution, per
 * sample or not -- that call with the batch's candidate sets added to g's handles.  The names are those of the utree_reports_add that follows
 * (read only when utree_reports_wants_names, and then already on the device on `stream`).  The sets go in at classify time, unlike
 * utree_reports_add's records: a batch that is classified but not committed afterwards is found by utree_reports_write's count of the reads. */
int utree_reports_classify(utree_reports *rep, int g, utree_dev *dev, const uint8_t *d_bases, const uint64_t *d_off, const uint32_t *d_len,
                           uint32_t n_reads, uint64_t total_bases, uint32_t max_len, int do_rc, utree_result *d_out, void *d_workspace,
                           size_t workspace_bytes, const uint8_t *d_text, uint64_t text_bytes, const uint32_t *d_name_off,
                           const uint32_t *d_name_len, void *stream);
/* n reads of device handle `g` whose output is committed: their records into its profile, records and names into its sample table and --
 * unless `rank`: the coverage counts the GG search's windows -- the reads into its coverage handle; asynchronous on `stream`.  Name r is
 * d_text[d_name_off[r] .. + d_name_len[r]) of d_text's text_bytes bytes; read only when utree_reports_wants_names.  rep == NULL: nothing. */
int utree_reports_add(utree_reports *rep, int g, const uint8_t *d_bases, const uint64_t *d_off, const uint32_t *d_len,
                      const utree_result *d_res, uint32_t n, int do_rc, int rank, const uint8_t *d_text, uint64_t text_bytes,
                      const uint32_t *d_name_off, const uint32_t *d_name_len, void *stream);
/* the search starts the file over: so do the reports */
int utree_reports_reset(utree_reports *rep);
/* after a search that succeeded and read n_reads reads: merges the devices' figures, checks that every read was counted exactly once and writes
 * the files: the coverage, the redistribution, the sample table, the per-sample redistribution, the profile.  0, UTREE_E_PROFILE (the profile,
 * the redistribution, the sample table or the per-sample redistribution: those have no code of their own) or UTREE_E_COVERAGE (the profile's
 * failure wins, then the redistribution's, the sample table's, the per-sample redistribution's);
 * utree_last_hip_error says why */
int utree_reports_write(utree_reports *rep, const utree_ctr *ctr, uint64_t n_reads);
void utree_reports_free(utree_reports *rep);

#endif
