/* redist.c -- redistribution of ambiguous reads among tied labels (include/utree_amd.h: utree_redist_*).
 *
 * A read's candidate set is the labels tied for its highest hit count; the handle keeps every distinct set with its read count on the device
 * for a whole search (redist_kernels.hip: a counter per label for the single-candidate reads, a table of the multi-label sets, their members
 * in an arena), fed by one pass per batch between the classify kernels and the vote (utree_classify_view, dev_image.c).  The passes
 * iterate there: each set goes to its richest member under the previous tally until the tallies stop moving; the host reads one word per
 * pass.  Entries of all labels are merged by label text, rolled up over the ';'-prefixes and written as
 *
 *     # reads\t<N>\tclassified\t<G>\tunclassified\t<N-G>\tambiguous\t<A>\tpasses\t<P>\n
 *     # taxon\tassigned\tunique\tclade_assigned\tclade_unique\n
 *     <taxon>\t...\n      one row per taxon with assigned > 0 and ';'-prefix of one, in unsigned bytewise order (shorter first on a tie)
 *
 * What it is not: a read whose best label is an interior taxon stays there (BUILD_GG relabels colliding k-mers to shorter labels); nothing is
 * normalised by genome length or k-mer distribution.
 *
 * Each read's redistributed label (utree_redist_classify_batch_keys, utree_redist_assign, utree_redist_reads_format): the per-batch pass can also
 * write a key per read -- nothing, a label, or the slot its set is in --, a solve keeps its final tally T_P in the handle, and the assignment
 * of any number of keys is then win(set, T_P) per slot, computed once per solve, and a gather.  The same limits hold: an interior best label
 * stays, nothing is normalised.
 */
#define _GNU_SOURCE
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ctr_host.h"
#include "dev_image.h"
#include "redist.h"
#include "taxon_table.h"

struct utree_redist {
    int device, n_cu;
    utk_redist_tab tab;                 /* device pointers */
    unsigned long long *d_tally;        /* [2][n_labels]: the passes' previous and next tally */
    uint32_t n_labels;
    /* the last solve, kept for utree_redist_assign: T_P is tp (one half of d_tally).  `solved` is cleared, and `changed` counted up, by every
     * later add, insert, merge into and reset (adds come from several threads: atomics) */
    int solved;
    unsigned changed;
    unsigned long long *tp, solve_id;   /* solve_id: unique per solve of any handle */
    uint32_t passes;
    /* the assignment's side, for the keys of THIS handle's table: win(slot, T_P) and the slot's candidates, (mask + 1) * 4 bytes each, allocated
     * on first use; valid for the solve win_of of a handle whose tally was here (d_tp when it was another's) while `changed` is win_changed */
    uint32_t *d_win, *d_ncand;
    unsigned long long *d_tp, win_of;
    unsigned win_changed;
};
static unsigned long long g_solve_id;
static void touched(utree_redist *rd) {
    __atomic_store_n(&rd->solved, 0, __ATOMIC_RELEASE);
    __atomic_fetch_add(&rd->changed, 1u, __ATOMIC_RELAXED);
}

#define CHK(x) do { if ((x) != hipSuccess) { utree_dev_set_hip_error((int)hipGetLastError(), #x); rc = UTREE_E_HIP; goto fail; } } while (0)

int utree_redist_create(utree_dev *dev, uint32_t set_capacity, utree_redist **out) {
    if (!dev || !out || !set_capacity) return UTREE_E_ARG;
    *out = NULL;
    uint32_t cap = 1;
    while (cap < set_capacity && cap < (1u << 28)) cap <<= 1;
    utree_redist *rd = (utree_redist *)calloc(1, sizeof *rd);
    if (!rd) return UTREE_E_NOMEM;
    rd->device = dev->device; rd->n_cu = dev->n_cu; rd->n_labels = dev->hdr.n_labels;
    rd->tab.mask = cap - 1; rd->tab.n_labels = rd->n_labels; rd->tab.arena_cap = (uint64_t)cap * UTK_REDIST_ARENA_PER_SLOT;
    const size_t nl = rd->n_labels ? rd->n_labels : 1;
    if (hipSetDevice(rd->device) != hipSuccess) { free(rd); return UTREE_E_HIP; }
    if (hipMalloc((void **)&rd->tab.slots, (size_t)cap * 16) != hipSuccess || hipMalloc((void **)&rd->tab.arena, rd->tab.arena_cap * 4) != hipSuccess ||
        hipMalloc((void **)&rd->tab.single, nl * 8) != hipSuccess || hipMalloc((void **)&rd->tab.misc, UTK_REDIST_MISC_WORDS * 8) != hipSuccess ||
        hipMalloc((void **)&rd->d_tally, 2 * nl * 8) != hipSuccess) {
        (void)hipGetLastError();
        utree_redist_free(rd);
        return UTREE_E_NOMEM;
    }
    const int rc = utree_redist_reset(rd);
    if (rc) { utree_redist_free(rd); return rc; }
    *out = rd;
    return UTREE_OK;
}

int utree_redist_reset(utree_redist *rd) {
    if (!rd) return UTREE_E_ARG;
    touched(rd);
    if (hipSetDevice(rd->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return UTREE_E_HIP;    /* adds in flight on any stream */
    if (hipMemset(rd->tab.slots, 0, ((size_t)rd->tab.mask + 1) * 16) != hipSuccess) return UTREE_E_HIP;        /* key 0 = free */
    if (hipMemset(rd->tab.single, 0, (size_t)(rd->n_labels ? rd->n_labels : 1) * 8) != hipSuccess) return UTREE_E_HIP;
    if (hipMemset(rd->tab.misc, 0, UTK_REDIST_MISC_WORDS * 8) != hipSuccess) return UTREE_E_HIP;
    return hipDeviceSynchronize() == hipSuccess ? UTREE_OK : UTREE_E_HIP;
}

void utree_redist_free(utree_redist *rd) {
    if (!rd) return;
    hipSetDevice(rd->device);
    hipDeviceSynchronize();
    if (rd->tab.slots) hipFree(rd->tab.slots);
    if (rd->tab.arena) hipFree(rd->tab.arena);
    if (rd->tab.single) hipFree(rd->tab.single);
    if (rd->tab.misc) hipFree(rd->tab.misc);
    if (rd->d_tally) hipFree(rd->d_tally);
    if (rd->d_win) hipFree(rd->d_win);
    if (rd->d_ncand) hipFree(rd->d_ncand);
    if (rd->d_tp) hipFree(rd->d_tp);
    free(rd);
}

int utree_redist_add_pending(utree_redist *rd, const utk_image *im, const utree_result *d_res, const utk_workspace *ws, uint32_t n_reads, int n_cu,
                             uint32_t *d_key, void *stream) {
    touched(rd);
    const int e = utk_redist_add(&rd->tab, im, d_res, ws, n_reads, n_cu, d_key, stream);
    if (e) { utree_dev_set_hip_error(e, "utk_redist_add"); return UTREE_E_HIP; }
    return UTREE_OK;
}

int utree_redist_classify_batch(utree_redist *rd, utree_dev *dev, const uint8_t *d_bases, const uint64_t *d_off, const uint32_t *d_len,
                                uint32_t n_reads, uint64_t total_bases, uint32_t max_len, int do_rc, utree_result *d_out, void *d_workspace,
                                size_t workspace_bytes, void *stream) {
    if (!rd || !dev || rd->device != dev->device || rd->n_labels != dev->hdr.n_labels) return UTREE_E_ARG;
    const utree_batch_view v = {d_bases, d_off, d_len, n_reads, total_bases, max_len, do_rc, NULL, 0, NULL, NULL, stream};
    return utree_classify_view(dev, &v, d_out, d_workspace, workspace_bytes, rd, NULL, NULL);
}

int utree_redist_classify_batch_keys(utree_redist *rd, utree_dev *dev, const uint8_t *d_bases, const uint64_t *d_off, const uint32_t *d_len,
                                     uint32_t n_reads, uint64_t total_bases, uint32_t max_len, int do_rc, utree_result *d_out, void *d_workspace,
                                     size_t workspace_bytes, uint32_t *d_key, void *stream) {
    if (!rd || !dev || rd->device != dev->device || rd->n_labels != dev->hdr.n_labels || (n_reads && !d_key)) return UTREE_E_ARG;
    if (rd->n_labels >= 0x80000000u) return UTREE_E_UNSUPPORTED;               /* a label key is below 2^31 */
    const utree_batch_view v = {d_bases, d_off, d_len, n_reads, total_bases, max_len, do_rc, NULL, 0, NULL, NULL, stream};
    return utree_classify_view(dev, &v, d_out, d_workspace, workspace_bytes, rd, NULL, d_key);
}

/* the handle's error word as a code and a text */
void utree_redist_flags_text(unsigned long long f, const char *lead, const char *sep, char *msg, size_t cap) {
    snprintf(msg, cap, "%s%s%s%s%s%s%s%s", f & UTK_REDIST_F_TABLE ? lead : "",
             f & UTK_REDIST_F_TABLE ? "the table of candidate sets was too small (raise UTREE_REDIST_CAPACITY)" : "", f & UTK_REDIST_F_TABLE ? sep : "",
             f & UTK_REDIST_F_ARENA ? lead : "",
             f & UTK_REDIST_F_ARENA ? "the arena of the sets' labels was too small (raise UTREE_REDIST_CAPACITY)" : "", f & UTK_REDIST_F_ARENA ? sep : "",
             f & UTK_REDIST_F_LABEL ? lead : "", f & UTK_REDIST_F_LABEL ? "a record named a label the database does not have" : "");
}

static int check_flags(unsigned long long f) {
    if (!f) return UTREE_OK;
    char msg[320];
    const int at = snprintf(msg, sizeof msg, "redistribution: ");
    utree_redist_flags_text(f, "", " ", msg + at, sizeof msg - at);
    utree_set_error_text(msg);
    return UTREE_E_DEVICE;
}

/* reads added so far, after a wait for the device; UTREE_E_DEVICE when a batch found the table or the arena too small (reports.c) */
int utree_redist_reads(utree_redist *rd, uint64_t *n_reads) {
    if (!rd || !n_reads) return UTREE_E_ARG;
    int rc = UTREE_OK;
    unsigned long long misc[UTK_REDIST_MISC_WORDS];
    CHK(hipSetDevice(rd->device));
    CHK(hipDeviceSynchronize());
    CHK(hipMemcpy(misc, rd->tab.misc, sizeof misc, hipMemcpyDeviceToHost));
    *n_reads = misc[0];
    rc = check_flags(misc[1]);
fail:
    return rc;
}

/* everything the device holds, on the host (malloc'ed; the caller frees): slots [2 * (mask + 1)], arena [*arena_n], single [n_labels], misc */
static int fetch(utree_redist *rd, unsigned long long **slots, uint32_t **arena, uint64_t *arena_n, unsigned long long **single,
                 unsigned long long *misc) {
    int rc = UTREE_OK;
    *slots = NULL; *arena = NULL; *single = NULL;
    CHK(hipSetDevice(rd->device));
    CHK(hipDeviceSynchronize());
    CHK(hipMemcpy(misc, rd->tab.misc, UTK_REDIST_MISC_WORDS * 8, hipMemcpyDeviceToHost));
    if ((rc = check_flags(misc[1]))) return rc;
    const size_t ns = (size_t)rd->tab.mask + 1;
    *arena_n = misc[2] < rd->tab.arena_cap ? misc[2] : rd->tab.arena_cap;
    *slots = (unsigned long long *)malloc(ns * 16);
    *arena = (uint32_t *)malloc((*arena_n ? *arena_n : 1) * 4);
    *single = (unsigned long long *)malloc((size_t)(rd->n_labels ? rd->n_labels : 1) * 8);
    if (!*slots || !*arena || !*single) { rc = UTREE_E_NOMEM; goto fail; }
    CHK(hipMemcpy(*slots, rd->tab.slots, ns * 16, hipMemcpyDeviceToHost));
    if (*arena_n) CHK(hipMemcpy(*arena, rd->tab.arena, *arena_n * 4, hipMemcpyDeviceToHost));
    if (rd->n_labels) CHK(hipMemcpy(*single, rd->tab.single, (size_t)rd->n_labels * 8, hipMemcpyDeviceToHost));
    return UTREE_OK;
fail:
    free(*slots); free(*arena); free(*single);
    *slots = NULL; *arena = NULL; *single = NULL;
    return rc;
}

int utree_redist_read(utree_redist *rd, utree_redist_set *h_sets, size_t set_cap, uint32_t *h_labels, size_t label_cap, size_t *n_sets,
                      size_t *n_labels, uint64_t *n_reads, uint64_t *n_classified) {
    if (!rd || !n_sets || !n_labels || (set_cap && !h_sets) || (label_cap && !h_labels)) return UTREE_E_ARG;
    unsigned long long *slots, *single, misc[UTK_REDIST_MISC_WORDS];
    uint32_t *arena;
    uint64_t arena_n;
    int rc = fetch(rd, &slots, &arena, &arena_n, &single, misc);
    if (rc) return rc;
    const size_t ns = (size_t)rd->tab.mask + 1;
    size_t sets = 0, labels = 0;
    uint64_t classified = 0;
    for (uint32_t l = 0; l < rd->n_labels; ++l) if (single[l]) { ++sets; ++labels; classified += single[l]; }
    for (size_t s = 0; s < ns; ++s) if (slots[2 * s]) {
        const uint64_t at = slots[2 * s] >> 32, n = (uint32_t)slots[2 * s];
        if (at + n > arena_n) { rc = UTREE_E_DEVICE; utree_set_error_text("redistribution: a slot points outside the arena"); goto done; }
        ++sets; labels += n; classified += slots[2 * s + 1];
    }
    *n_sets = sets; *n_labels = labels;
    if (n_reads) *n_reads = misc[0];
    if (n_classified) *n_classified = classified;
    if (sets > set_cap || labels > label_cap) { rc = UTREE_E_ARG; goto done; }
    size_t si = 0, li = 0;
    for (uint32_t l = 0; l < rd->n_labels; ++l) if (single[l]) {
        h_sets[si].reads = single[l]; h_sets[si].first = li; h_sets[si].n = 1; h_sets[si].pad = 0;
        h_labels[li++] = l; ++si;
    }
    for (size_t s = 0; s < ns; ++s) if (slots[2 * s]) {
        const uint64_t at = slots[2 * s] >> 32;
        const uint32_t n = (uint32_t)slots[2 * s];
        h_sets[si].reads = slots[2 * s + 1]; h_sets[si].first = li; h_sets[si].n = n; h_sets[si].pad = 0;
        memcpy(h_labels + li, arena + at, (size_t)n * 4);
        li += n; ++si;
    }
done:
    free(slots); free(arena); free(single);
    return rc;
}

int utree_redist_merge(utree_redist *dst, utree_redist *src) {
    if (!dst || !src || dst == src || dst->n_labels != src->n_labels) return UTREE_E_ARG;
    touched(dst);                                                       /* (slots are only added: dst's keys stay valid) */
    size_t ns = 0, nl = 0;
    uint64_t reads = 0;
    int rc = utree_redist_read(src, NULL, 0, NULL, 0, &ns, &nl, &reads, NULL);
    if (rc && rc != UTREE_E_ARG) return rc;
    /* one host block, one device block: reads [ns + 1] (the last: src's reads added) | first [ns] | labels [nl] | n [ns] */
    const size_t bytes = (ns + 1) * 8 + ns * 8 + nl * 4 + ns * 4;
    utree_redist_set *sets = (utree_redist_set *)malloc((ns ? ns : 1) * sizeof *sets);
    char *h = (char *)malloc(bytes);
    void *d = NULL;
    if (!sets || !h) { free(sets); free(h); return UTREE_E_NOMEM; }
    unsigned long long *h_reads = (unsigned long long *)h, *h_first = h_reads + ns + 1;
    uint32_t *h_labels = (uint32_t *)(h_first + ns), *h_n = h_labels + nl;
    rc = utree_redist_read(src, sets, ns, h_labels, nl, &ns, &nl, &reads, NULL);
    if (rc) goto fail;
    for (size_t i = 0; i < ns; ++i) { h_reads[i] = sets[i].reads; h_first[i] = sets[i].first; h_n[i] = sets[i].n; }
    h_reads[ns] = reads;
    CHK(hipSetDevice(dst->device));
    CHK(hipDeviceSynchronize());
    if (hipMalloc(&d, bytes) != hipSuccess) { (void)hipGetLastError(); rc = UTREE_E_NOMEM; goto fail; }
    CHK(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));
    {
        const unsigned long long *d_reads = (const unsigned long long *)d, *d_first = d_reads + ns + 1;
        const uint32_t *d_labels = (const uint32_t *)(d_first + ns), *d_n = d_labels + nl;
        if (utk_redist_insert(&dst->tab, d_reads, d_first, d_n, d_labels, ns, NULL) || utk_redist_sum(dst->tab.misc, d_reads + ns, 1, NULL)) {
            rc = UTREE_E_HIP;
            goto fail;
        }
    }
    CHK(hipDeviceSynchronize());
fail:
    (void)hipDeviceSynchronize();
    if (d) hipFree(d);
    free(sets); free(h);
    return rc;
}

int utree_redist_solve(utree_redist *rd, uint32_t max_passes, utree_redist_entry *h, size_t cap, size_t *n, uint32_t *passes, uint64_t *ambiguous) {
    if (!rd || !n || (cap && !h) || max_passes < 1 || max_passes > 1000) return UTREE_E_ARG;
    int rc = UTREE_OK;
    const size_t nl = rd->n_labels;
    unsigned long long misc[UTK_REDIST_MISC_WORDS], *m = NULL;
    unsigned long long *prev = rd->d_tally, *next = rd->d_tally + (nl ? nl : 1);
    uint32_t p = 0;
    *n = 0;
    const unsigned changed = __atomic_load_n(&rd->changed, __ATOMIC_RELAXED);
    __atomic_store_n(&rd->solved, 0, __ATOMIC_RELEASE);
    CHK(hipSetDevice(rd->device));
    CHK(hipDeviceSynchronize());
    CHK(hipMemcpy(misc, rd->tab.misc, sizeof misc, hipMemcpyDeviceToHost));
    if ((rc = check_flags(misc[1]))) return rc;
    const unsigned long long reads = misc[0];
    if (utk_redist_tally0(&rd->tab, prev, NULL)) { rc = UTREE_E_HIP; goto fail; }
    for (;;) {
        unsigned long long changes = 0;
        if (utk_redist_pass(&rd->tab, prev, next, NULL)) { rc = UTREE_E_HIP; goto fail; }
        CHK(hipMemcpy(&changes, rd->tab.misc + 3, 8, hipMemcpyDeviceToHost));       /* the one word the host reads per pass */
        { unsigned long long *t = prev; prev = next; next = t; }
        ++p;
        if (p >= max_passes || changes <= reads / 100000) break;
    }
    /* the final assignment: one more evaluation under T_P (not T_P itself) */
    if (utk_redist_pass(&rd->tab, prev, next, NULL)) { rc = UTREE_E_HIP; goto fail; }
    m = (unsigned long long *)malloc((nl ? nl : 1) * 16);
    if (!m) { rc = UTREE_E_NOMEM; goto fail; }
    if (nl) {
        CHK(hipMemcpy(m, next, nl * 8, hipMemcpyDeviceToHost));
        CHK(hipMemcpy(m + nl, rd->tab.single, nl * 8, hipMemcpyDeviceToHost));
    }
    CHK(hipMemcpy(misc, rd->tab.misc, sizeof misc, hipMemcpyDeviceToHost));
    size_t k = 0;
    for (size_t l = 0; l < nl; ++l) if (m[l] || m[nl + l]) {
        if (k < cap) { h[k].label = (uint32_t)l; h[k].pad = 0; h[k].assigned = m[l]; h[k].unique = m[nl + l]; }
        ++k;
    }
    *n = k;
    if (k > cap) rc = UTREE_E_ARG;
    if (passes) *passes = p;
    if (ambiguous) *ambiguous = misc[4];
    CHK(hipDeviceSynchronize());
    /* T_P stays where the loop left it, for utree_redist_assign (nothing was added meanwhile: else the tally is not that of the table) */
    if (__atomic_load_n(&rd->changed, __ATOMIC_RELAXED) == changed) {
        rd->tp = prev; rd->passes = p; rd->solve_id = __atomic_add_fetch(&g_solve_id, 1ull, __ATOMIC_RELAXED);
        __atomic_store_n(&rd->solved, 1, __ATOMIC_RELEASE);
    }
fail:
    (void)hipDeviceSynchronize();
    free(m);
    return rc;
}

int utree_redist_assign(utree_redist *keys, utree_redist *solved, const uint32_t *d_key, uint64_t n, uint32_t *d_label, uint32_t *d_ncand,
                        void *stream) {
    if (!keys || !solved || keys->n_labels != solved->n_labels || !__atomic_load_n(&solved->solved, __ATOMIC_ACQUIRE)) return UTREE_E_ARG;
    if (n && (!d_key || !d_label)) return UTREE_E_ARG;
    int rc = UTREE_OK;
    void *h = NULL;
    const size_t nl = keys->n_labels ? keys->n_labels : 1, ns = (size_t)keys->tab.mask + 1;
    const unsigned changed = __atomic_load_n(&keys->changed, __ATOMIC_RELAXED);
    CHK(hipSetDevice(keys->device));
    if (!keys->d_win || keys->win_of != solved->solve_id || keys->win_changed != changed) {
        /* once per solve: T_P to this device, every slot's winner under it.  Synchronous: the tally's owner may go on to solve again */
        if (!keys->d_win && (hipMalloc((void **)&keys->d_win, ns * 4) != hipSuccess || hipMalloc((void **)&keys->d_ncand, ns * 4) != hipSuccess)) {
            (void)hipGetLastError();
            if (keys->d_win) hipFree(keys->d_win);
            keys->d_win = NULL; keys->d_ncand = NULL;
            return UTREE_E_NOMEM;
        }
        keys->win_of = 0;
        const unsigned long long *tp = solved->tp;
        if (solved != keys) {
            if (!keys->d_tp && hipMalloc((void **)&keys->d_tp, nl * 8) != hipSuccess) { (void)hipGetLastError(); keys->d_tp = NULL; return UTREE_E_NOMEM; }
            if (solved->device == keys->device) CHK(hipMemcpy(keys->d_tp, solved->tp, nl * 8, hipMemcpyDeviceToDevice));
            else {                                                      /* through the host: any two devices */
                if (!(h = malloc(nl * 8))) return UTREE_E_NOMEM;
                CHK(hipSetDevice(solved->device));
                CHK(hipMemcpy(h, solved->tp, nl * 8, hipMemcpyDeviceToHost));
                CHK(hipSetDevice(keys->device));
                CHK(hipMemcpy(keys->d_tp, h, nl * 8, hipMemcpyHostToDevice));
            }
            tp = keys->d_tp;
        }
        CHK(hipDeviceSynchronize());                                    /* adds to this table in flight on any stream */
        if (utk_redist_winner(&keys->tab, tp, keys->d_win, keys->d_ncand, NULL)) { rc = UTREE_E_HIP; goto fail; }
        CHK(hipStreamSynchronize(NULL));
        keys->win_of = solved->solve_id; keys->win_changed = changed;
    }
    if (utk_redist_assign(&keys->tab, keys->d_win, keys->d_ncand, d_key, n, d_label, d_ncand, stream)) {
        utree_dev_set_hip_error((int)hipGetLastError(), "utk_redist_assign");
        rc = UTREE_E_HIP;
    }
fail:
    free(h);
    return rc;
}

/* ---- host: one line per read that has a label ------------------------------------------------------------------------------- */
size_t utree_redist_reads_format(const utree_ctr *ctr, const uint8_t *names, const uint64_t *name_off, const uint32_t *name_len,
                                 const uint32_t *label, const uint32_t *ncand, size_t n, char *out, size_t cap) {
    size_t at = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t l = label[i];
        if (l == 0xFFFFFFFFu) continue;
        if (l >= ctr->info.n_labels) return (size_t)-1;
        char tok[16];
        size_t t = 0;
        uint32_t v = ncand[i];
        do { tok[t++] = (char)('0' + v % 10); v /= 10; } while (v);
        const size_t ll = ctr->label_len[l], need = (size_t)name_len[i] + 1 + ll + 1 + t + 1;
        if (need > cap - at) return (size_t)-1;
        memcpy(out + at, names + name_off[i], name_len[i]); at += name_len[i];
        out[at++] = '\t';
        memcpy(out + at, ctr->labels[l], ll); at += ll;
        out[at++] = '\t';
        while (t) out[at++] = tok[--t];
        out[at++] = '\n';
    }
    return at;
}

/* ---- host: every label's figures as rows of the taxon table (taxon_table.c) ----------------------------------------------- */
int utree_redist_write(const utree_ctr *ctr, const utree_redist_entry *e, size_t n, uint64_t n_reads, uint64_t ambiguous, uint32_t passes,
                       const char *path) {
    if (!ctr || (n && !e) || !path) return UTREE_E_ARG;
    uint64_t classified = 0;
    utree_taxon_row *t = (utree_taxon_row *)calloc(n ? n : 1, sizeof *t);      /* own: {assigned, unique} */
    if (!t) return UTREE_E_NOMEM;
    for (size_t i = 0; i < n; ++i) {
        if (e[i].label >= ctr->info.n_labels) { free(t); return UTREE_E_ARG; }
        t[i].s = ctr->labels[e[i].label]; t[i].len = ctr->label_len[e[i].label];
        t[i].own[0] = e[i].assigned; t[i].own[1] = e[i].unique;
        classified += e[i].assigned;
    }
    char header[320];
    snprintf(header, sizeof header, "# reads\t%llu\tclassified\t%llu\tunclassified\t%llu\tambiguous\t%llu\tpasses\t%u\n"
                                    "# taxon\tassigned\tunique\tclade_assigned\tclade_unique\n",
             (unsigned long long)n_reads, (unsigned long long)classified, (unsigned long long)(n_reads - classified), (unsigned long long)ambiguous,
             passes);
    const int rc = utree_taxon_table_write(t, n, 2, 0, header, path);
    free(t);
    return rc;
}
