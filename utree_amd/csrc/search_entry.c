/* search_entry.c -- the front door of the whole-file search: utree_search_run checks a request and hands it to utree_search_checked (search.c);
 * the fixed-argument forms of include/utree_amd.h fill a request in; and utree_pairs_join, the C-ABI form of the pairs kernels' launcher. */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <string.h>
#include "dev_image.h"
#include "search_dev.h"
#include "pairs_kernels.h"

/* The one place that checks a request, every check in front of the first look at `ctr` or a device handle.  rank: XT_doSearch32(utree, in, out, 0,
 * speed, doRC) (itree.c:1376 without DO_GG): the same pipeline, the batches to ONE device in file order because each read's vote depends on the
 * reads before it (rank.c) -- another vote: no candidate sets; a hit-dependent subset of windows: no map, and no coverage of the GG search's */
int utree_search_run(const utree_ctr *ctr, utree_dev **devs, int n_dev, const utree_search_request *req, utree_search_stats *stats) {
    /* a caller built before redistribute_reads_path gives the size of the layout without it: a request without that report */
    const size_t al = _Alignof(utree_search_request), old_size = (offsetof(utree_search_request, redistribute_reads_path) + al - 1) / al * al;
    utree_search_request grown;
    if (req && req->size == old_size && old_size < sizeof grown) {
        memset(&grown, 0, sizeof grown);
        memcpy(&grown, req, old_size);
        grown.size = sizeof grown;
        req = &grown;
    }
    if (!req || req->size != sizeof *req) return UTREE_E_ARG;
    if (!ctr || !devs || n_dev < 1 || !req->reads_path || !req->out_path) return UTREE_E_ARG;
    if (req->input_format < 0 || req->input_format > UTREE_INPUT_AUTO || (req->mates_path && req->interleaved)) return UTREE_E_ARG;
    const int d = req->sample_delim;
    if ((req->samples_path || req->sample_redistribute_path) && (d < 0 || d > 255 || d == '\t' || d == ' ' || d == '\r' || d == '\n')) return UTREE_E_ARG;
    if ((req->redistribute_path || req->sample_redistribute_path || req->redistribute_reads_path) && req->max_passes > 1000) return UTREE_E_ARG;
    if (req->rank) {
        if (n_dev != 1 || req->mates_path || req->interleaved || req->coverage_path || req->redistribute_path || req->hitmap_path ||
            req->sample_redistribute_path || req->redistribute_reads_path) return UTREE_E_ARG;
        const int rc = utree_rank_reset(devs[0]);
        if (rc) return rc;
    }
    return utree_search_checked(ctr, devs, n_dev, req, stats);
}

/* ---- the fixed-argument forms of utree_search_run (include/utree_amd.h) ------------------------------------------------------------------ */
#define REQ(...) const utree_search_request r = {.size = sizeof r, .reads_path = reads_path, .out_path = out_path, .do_rc = do_rc, .host_threads = host_threads, __VA_ARGS__}
#define REPORTS4 .input_format = input_format, .mates_path = mates_path, .interleaved = interleaved, .profile_path = profile_path, \
                 .coverage_path = coverage_path, .redistribute_path = redistribute_path, .max_passes = max_passes

int utree_search_file(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path, const char *out_path,
                      int do_rc, int host_threads, utree_search_stats *stats) {
    REQ(.input_format = UTREE_INPUT_REFERENCE);
    return utree_search_run(ctr, devs, n_dev, &r, stats);
}
int utree_search_file_opts(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path, const char *out_path,
                           int do_rc, int host_threads, int input_format, utree_search_stats *stats) {
    REQ(.input_format = input_format);
    return utree_search_run(ctr, devs, n_dev, &r, stats);
}
int utree_search_file_profile(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path, const char *out_path, int do_rc,
                              int host_threads, int input_format, const char *profile_path, utree_search_stats *stats) {
    REQ(.input_format = input_format, .profile_path = profile_path);
    return utree_search_run(ctr, devs, n_dev, &r, stats);
}
int utree_search_file_coverage(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path, const char *out_path, int do_rc,
                               int host_threads, int input_format, const char *profile_path, const char *coverage_path,
                               utree_search_stats *stats) {
    REQ(.input_format = input_format, .profile_path = profile_path, .coverage_path = coverage_path);
    return utree_search_run(ctr, devs, n_dev, &r, stats);
}
int utree_search_pairs_file(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path, const char *mates_path, const char *out_path,
                            int do_rc, int host_threads, int input_format, const char *profile_path, const char *coverage_path,
                            utree_search_stats *stats) {
    REQ(.input_format = input_format, .mates_path = mates_path, .interleaved = !mates_path, .profile_path = profile_path, .coverage_path = coverage_path);
    return utree_search_run(ctr, devs, n_dev, &r, stats);
}
int utree_search_file_redistribute(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path, const char *mates_path,
                                   int interleaved, const char *out_path, int do_rc, int host_threads, int input_format,
                                   const char *profile_path, const char *coverage_path, const char *redistribute_path, uint32_t max_passes,
                                   utree_search_stats *stats) {
    REQ(REPORTS4);
    return utree_search_run(ctr, devs, n_dev, &r, stats);
}
int utree_search_file_hitmap(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path, const char *mates_path, int interleaved,
                             const char *out_path, int do_rc, int host_threads, int input_format, const char *profile_path,
                             const char *coverage_path, const char *redistribute_path, uint32_t max_passes, const char *hitmap_path,
                             utree_search_stats *stats) {
    REQ(REPORTS4, .hitmap_path = hitmap_path);
    return utree_search_run(ctr, devs, n_dev, &r, stats);
}
int utree_search_file_samples(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path, const char *mates_path, int interleaved,
                              const char *out_path, int do_rc, int host_threads, int input_format, const char *profile_path,
                              const char *coverage_path, const char *redistribute_path, uint32_t max_passes, const char *hitmap_path,
                              const char *samples_path, int delim, utree_search_stats *stats) {
    REQ(REPORTS4, .hitmap_path = hitmap_path, .samples_path = samples_path, .sample_delim = delim);
    return utree_search_run(ctr, devs, n_dev, &r, stats);
}
int utree_search_file_sample_redistribute(const utree_ctr *ctr, utree_dev **devs, int n_dev, const char *reads_path, const char *mates_path,
                                          int interleaved, const char *out_path, int do_rc, int host_threads, int input_format,
                                          const char *profile_path, const char *coverage_path, const char *redistribute_path, uint32_t max_passes,
                                          const char *hitmap_path, const char *samples_path, int delim, const char *sample_redistribute_path,
                                          utree_search_stats *stats) {
    REQ(REPORTS4, .hitmap_path = hitmap_path, .samples_path = samples_path, .sample_delim = delim, .sample_redistribute_path = sample_redistribute_path);
    return utree_search_run(ctr, devs, n_dev, &r, stats);
}

/* the rank-specific search: one handle; without params there is nothing to run */
int utree_rank_search_file_samples(const utree_ctr *ctr, utree_dev *dev, const char *reads_path, const char *out_path, int do_rc,
                                   const utree_rank_params *params, int host_threads, int input_format, const char *profile_path,
                                   const char *samples_path, int delim, utree_search_stats *stats) {
    if (!dev || !params) return UTREE_E_ARG;
    REQ(.input_format = input_format, .rank = params, .profile_path = profile_path, .samples_path = samples_path, .sample_delim = delim);
    return utree_search_run(ctr, &dev, 1, &r, stats);
}
int utree_rank_search_file_profile(const utree_ctr *ctr, utree_dev *dev, const char *reads_path, const char *out_path, int do_rc,
                                   const utree_rank_params *params, int host_threads, int input_format, const char *profile_path,
                                   utree_search_stats *stats) {
    return utree_rank_search_file_samples(ctr, dev, reads_path, out_path, do_rc, params, host_threads, input_format, profile_path, NULL, 0, stats);
}
int utree_rank_search_file_opts(const utree_ctr *ctr, utree_dev *dev, const char *reads_path, const char *out_path, int do_rc,
                                const utree_rank_params *params, int host_threads, int input_format, utree_search_stats *stats) {
    return utree_rank_search_file_samples(ctr, dev, reads_path, out_path, do_rc, params, host_threads, input_format, NULL, NULL, 0, stats);
}
int utree_rank_search_file(const utree_ctr *ctr, utree_dev *dev, const char *reads_path, const char *out_path, int do_rc,
                           const utree_rank_params *params, int host_threads, utree_search_stats *stats) {
    return utree_rank_search_file_samples(ctr, dev, reads_path, out_path, do_rc, params, host_threads, UTREE_INPUT_REFERENCE, NULL, NULL, 0, stats);
}

int utree_pairs_join(utree_dev *dev, const uint8_t *d_bases1, const uint64_t *d_off1, const uint32_t *d_len1, const uint8_t *d_bases2,
                     const uint64_t *d_off2, const uint32_t *d_len2, uint32_t n_pairs, uint8_t *d_joined, uint64_t joined_capacity,
                     uint64_t *d_joff, uint32_t *d_jlen, utree_pairs_meta *d_meta, void *stream) {
    if (!dev || !d_meta) return UTREE_E_ARG;
    if (n_pairs && (!d_bases1 || !d_off1 || !d_len1 || !d_bases2 || !d_off2 || !d_len2 || !d_joff || !d_jlen || (!d_joined && joined_capacity)))
        return UTREE_E_ARG;
    hipError_t e = hipMemsetAsync(d_meta, 0, sizeof *d_meta, (hipStream_t)stream);
    if (e == hipSuccess && n_pairs)
        e = (hipError_t)utk_pairs_join(d_bases1, d_off1, d_len1, d_bases2, d_off2, d_len2, n_pairs, d_joined, joined_capacity, d_joff, d_jlen,
                                       d_meta, stream);
    if (e != hipSuccess) { utree_dev_set_hip_error((int)e, "utree_pairs_join"); return UTREE_E_HIP; }
    return UTREE_OK;
}
