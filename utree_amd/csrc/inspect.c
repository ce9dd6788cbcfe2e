/* inspect.c -- host side of utree_inspect_file (`utree-inspect`) and the writer of its two files, utree_inspect_write.  include/utree_amd.h
 * states what an inspection is.  The input is opened, cut into passes and laid out in slices by the merge's own functions (merge_input.h),
 * as the only input over its label universe; the merge's device handle decodes and sorts each pass (merge_kernels.hip: utk_inspect_pass)
 * into the resident arrays of inspect_kernels.hip, which then classifies every node by its 3k neighbours and counts the label pairs.  Here:
 * the plan, the depth of every universe label for the device's lineage test, the roll-up by text and both writers.
 */
#define _FILE_OFFSET_BITS 64
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "utree_internal.h"
#include "merge_input.h"
#include "inspect_gpu.h"
#include "taxon_table.h"

enum { F_KMERS, F_ISOLATED, F_SAME, F_LINEAGE, F_CONFLICT, N_FIG };            /* a row's own figures, in the order the report prints them */

/* ---- the writer ------------------------------------------------------------------------------------------------------------------ */
static int by_entry_text(const void *x, const void *y, void *entries) {
    const utree_inspect_entry *e = (const utree_inspect_entry *)entries, *a = &e[*(const uint32_t *)x], *b = &e[*(const uint32_t *)y];
    return utree_text_cmp(a->text, a->len, b->text, b->len);
}
typedef struct { uint32_t from, to; uint64_t pairs; } group_pair;              /* between rows, which stand in text order */
static int by_from_to(const void *x, const void *y) {
    const group_pair *a = (const group_pair *)x, *b = (const group_pair *)y;
    if (a->from != b->from) return a->from < b->from ? -1 : 1;
    return a->to < b->to ? -1 : a->to > b->to;
}
static const char *kind_of(const utree_taxon_row *from, const utree_taxon_row *to) {
    if (from->len > to->len && from->s[to->len] == ';' && !memcmp(from->s, to->s, to->len)) return "ancestor";
    if (to->len > from->len && to->s[from->len] == ';' && !memcmp(from->s, to->s, from->len)) return "descendant";
    return "conflict";
}

int utree_inspect_write(const utree_compare_input *db, const utree_inspect_entry *e, size_t n, const utree_inspect_pair *p, size_t n_pairs,
                        uint64_t pair_events, uint64_t distinct_pairs, const char *report_path, const char *pairs_path, utree_inspect_stats *stats) {
    if (!db || !db->path || !report_path || (n && !e) || n >= 0xFFFFFFFFu) return UTREE_E_ARG;
    if (!pairs_path) { p = NULL; n_pairs = 0; }
    if (n_pairs && !p) return UTREE_E_ARG;
    for (size_t i = 0; i < n; ++i) if (e[i].len && !e[i].text) return UTREE_E_ARG;
    for (size_t i = 0; i < n_pairs; ++i) if (p[i].from >= n || p[i].to >= n) return UTREE_E_ARG;
    utree_inspect_stats st; memset(&st, 0, sizeof st);
    int rc = UTREE_OK;
    static const int clade_of[2] = {F_KMERS, F_CONFLICT};
    uint32_t *order = (uint32_t *)malloc(4 * (n ? n : 1)), *row_of = (uint32_t *)malloc(4 * (n ? n : 1));
    utree_taxon_row *t = (utree_taxon_row *)calloc(n ? n : 1, sizeof *t);
    group_pair *gp = (group_pair *)malloc(sizeof *gp * (n_pairs ? n_pairs : 1));
    char *header = (char *)malloc(strlen(db->path) + 1024);
    size_t nt = 0, ngp = 0;
    if (!order || !row_of || !t || !gp || !header) { rc = UTREE_E_NOMEM; goto done; }
    /* ---- one row per distinct text, in text order; entries of equal text are added up ---- */
    for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
    qsort_r(order, n, 4, by_entry_text, (void *)e);
    for (size_t i = 0; i < n; ++i) {
        const utree_inspect_entry *x = &e[order[i]];
        if (!nt || utree_text_cmp(t[nt - 1].s, t[nt - 1].len, x->text, x->len)) { t[nt].s = x->text; t[nt].len = x->len; ++nt; }
        uint64_t *own = t[nt - 1].own;
        own[F_ISOLATED] += x->isolated; own[F_SAME] += x->same; own[F_LINEAGE] += x->lineage; own[F_CONFLICT] += x->conflict;
        row_of[order[i]] = (uint32_t)(nt - 1);
    }
    for (size_t r = 0; r < nt; ++r) {
        uint64_t *own = t[r].own;
        own[F_KMERS] = own[F_ISOLATED] + own[F_SAME] + own[F_LINEAGE] + own[F_CONFLICT];
        st.kmers += own[F_KMERS]; st.isolated += own[F_ISOLATED]; st.same += own[F_SAME]; st.lineage += own[F_LINEAGE]; st.conflict += own[F_CONFLICT];
        st.labels += own[F_KMERS] != 0;
    }
    /* ---- the pairs between rows, equal pairs added up; every pair must stand with its mirror image ---- */
    for (size_t i = 0; i < n_pairs; ++i) {
        gp[i].from = row_of[p[i].from]; gp[i].to = row_of[p[i].to]; gp[i].pairs = p[i].pairs;
        if (gp[i].from == gp[i].to) { rc = UTREE_E_ARG; goto done; }
    }
    qsort(gp, n_pairs, sizeof *gp, by_from_to);
    for (size_t i = 0; i < n_pairs; ++i) {
        if (!gp[i].pairs) continue;                                            /* no event: not a pair */
        if (ngp && !by_from_to(&gp[ngp - 1], &gp[i])) gp[ngp - 1].pairs += gp[i].pairs;
        else gp[ngp++] = gp[i];
    }
    for (size_t i = 0; i < ngp; ++i) {
        const group_pair mirror = {gp[i].to, gp[i].from, 0}, *m = (const group_pair *)bsearch(&mirror, gp, ngp, sizeof *gp, by_from_to);
        if (!m || m->pairs != gp[i].pairs || !t[gp[i].from].own[F_KMERS] || !t[gp[i].to].own[F_KMERS]) { rc = UTREE_E_ARG; goto done; }
    }
    if (pairs_path) {
        for (size_t i = 0; i < ngp; ++i) st.pair_events += gp[i].pairs;
        st.distinct_pairs = ngp;
    } else { st.pair_events = pair_events; st.distinct_pairs = distinct_pairs; }
    st.W = db->W; st.I = db->I; st.is_ctr = db->is_ctr;
    st.clean = !st.conflict;
    /* ---- the report: rows without a node leave (the table merges and sorts in place: compact first) ---- */
    {
        size_t w = 0;
        for (size_t r = 0; r < nt; ++r) if (t[r].own[F_KMERS]) { row_of[r] = (uint32_t)w; t[w++] = t[r]; }    /* row_of: old row -> kept row; a row a pair names has nodes */
        for (size_t i = 0; i < ngp; ++i) { gp[i].from = row_of[gp[i].from]; gp[i].to = row_of[gp[i].to]; }
        nt = w;
    }
    sprintf(header, "# db\t%s\t%s\t%u\t%u\t%llu\t%llu\n"
                    "# kmers\t%llu\tisolated\t%llu\tsame\t%llu\tlineage\t%llu\tconflict\t%llu\tpair_events\t%llu\tdistinct_pairs\t%llu\n"
                    "# taxon\tkmers\tisolated\tsame\tlineage\tconflict\tclade_kmers\tclade_conflict\n",
            db->path, db->is_ctr ? ".ctr" : ".ubt", db->W, db->I, (unsigned long long)st.kmers, (unsigned long long)st.labels,
            (unsigned long long)st.kmers, (unsigned long long)st.isolated, (unsigned long long)st.same, (unsigned long long)st.lineage,
            (unsigned long long)st.conflict, (unsigned long long)st.pair_events, (unsigned long long)st.distinct_pairs);
    if (pairs_path) {                                                          /* before the table, which sorts and merges t in place */
        FILE *f = fopen(pairs_path, "wb");
        if (!f) { rc = utree_merge_fail_text(UTREE_E_IO, "%s: cannot create%s", pairs_path, ""); goto done; }
        int bad = fputs("# from\tto\tpairs\tkind\n", f) < 0;
        for (size_t i = 0; i < ngp && !bad; ++i) {
            const utree_taxon_row *x = &t[gp[i].from], *y = &t[gp[i].to];
            if (x->len && fwrite(x->s, 1, x->len, f) != x->len) bad = 1;
            if (fputc('\t', f) == EOF) bad = 1;
            if (y->len && fwrite(y->s, 1, y->len, f) != y->len) bad = 1;
            if (fprintf(f, "\t%llu\t%s\n", (unsigned long long)gp[i].pairs, kind_of(x, y)) < 0) bad = 1;
        }
        if (fclose(f) != 0) bad = 1;
        if (bad) { rc = utree_merge_fail_text(UTREE_E_IO, "%s: cannot write%s", pairs_path, ""); goto done; }
    }
    rc = utree_taxon_table_write_pick(t, nt, N_FIG, clade_of, 2, -1, header, report_path);
    if (rc == UTREE_E_IO) utree_merge_fail_text(rc, "%s: cannot write%s", report_path, "");
done:
    if (rc == UTREE_E_IO || rc == UTREE_E_NOMEM) {                             /* a failed call leaves neither file behind (UTREE_E_ARG came before either was created) */
        unlink(report_path);
        if (pairs_path) unlink(pairs_path);
    }
    free(order); free(row_of); free(t); free(gp); free(header);
    if (stats && !rc) *stats = st;
    return rc;
}

/* ---- the inspection -------------------------------------------------------------------------------------------------------------- */
static int fail_num(int rc, const char *fmt, const char *path, uint64_t v) {
    char num[32];
    snprintf(num, sizeof num, "%llu", (unsigned long long)v);
    return utree_merge_fail_text(rc, fmt, path, num);
}

int utree_inspect_file(const char *db_path, const char *report_path, const char *pairs_path, int device, utree_inspect_stats *stats) {
    if (!db_path || !report_path || !stats) return UTREE_E_ARG;
    const double t0 = now_s();
    utree_inspect_stats st; memset(&st, 0, sizeof st);
    int rc = UTREE_OK;
    merge_in in; memset(&in, 0, sizeof in);
    in.fd = -1;
    label_universe L; memset(&L, 0, sizeof L);
    uint32_t *bounds = NULL, n_pass = 0, *depth = NULL, *entry_of_u = NULL;
    utk_merge_dev *D = NULL;
    utk_inspect_dev *X = NULL;
    uint64_t *fig = NULL, *h_keys = NULL, *h_counts = NULL;
    utree_inspect_entry *e = NULL;
    utree_inspect_pair *pr = NULL;
    size_t n_e = 0, n_pr = 0;
    utk_inspect_out no; memset(&no, 0, sizeof no);
    /* ---- the input, as the merge reads one ---- */
    rc = utree_merge_input_open(&in, db_path, &L, NULL, NULL, 0, NULL);
    if (rc) goto done;
    const uint32_t W = in.W;
    st.W = W; st.I = in.I; st.is_ctr = (uint32_t)in.is_ctr;
    if (in.n >= 0xFFFFFFFFull) { rc = utree_merge_fail_text(UTREE_E_UNSUPPORTED, "%s: 2^32 - 1 nodes or more%s", db_path, ""); goto done; }
    if (universe_close(&L)) { rc = UTREE_E_NOMEM; goto done; }
    const uint32_t n_u = L.U.n;
    uint64_t pair_cap = pairs_path ? 1ull << 22 : UTK_INSPECT_KEY_SET;
    {
        const char *k = getenv("UTREE_INSPECT_PAIRS");
        if (pairs_path && k && *k) {
            char *end = NULL;
            const unsigned long long v = strtoull(k, &end, 10);
            if (*end || !v || v > (1ull << 28)) { rc = utree_merge_fail_text(UTREE_E_ARG, "UTREE_INSPECT_PAIRS=%s: not a number of pairs from 1 to 2^28%s", k, ""); goto done; }
            pair_cap = v;
        }
    }
    if (in.n) {
        /* ---- the device: the resident database first, the merge's passes in what memory is left ---- */
        depth = (uint32_t *)calloc(n_u ? n_u : 1, 4);
        if (!depth) { rc = UTREE_E_NOMEM; goto done; }
        for (uint32_t u = 0; u < n_u; ++u) {
            const char *s = L.U.blob + L.U.off[u];
            for (uint32_t q = 0; q < L.U.len[u]; ++q) depth[u] += s[q] == ';';
        }
        const utk_inspect_cfg xc = {W, device, in.n, n_u, depth, L.trunc_off, L.trunc_ids, L.n_trunc, pair_cap, pairs_path != NULL};
        rc = utk_inspect_open(&xc, &X);
        if (rc == UTREE_E_NOMEM) { rc = fail_num(rc, "%s: its nodes need %s bytes resident on the device, which does not have them free", db_path, utk_inspect_resident_bytes(W, in.n)); goto done; }
        if (rc) goto done;
        uint64_t limit = 0, cap_nodes = 0, cap_raw = 0, at = 0, *d_lo = NULL, *d_hi = NULL;
        uint32_t *d_lab = NULL;
        utk_inspect_arrays(X, &d_lo, &d_hi, &d_lab);
        rc = utk_compare_limit(device, W, in.rec, n_u, &limit);
        if (rc) goto done;
        rc = utree_merge_plan(&in, 1, in.n, limit, report_path, &bounds, &n_pass, &cap_nodes, &cap_raw);
        if (rc) goto done;
        st.n_passes = n_pass;
        const uint32_t *maps[1] = {in.u_of_ix};
        const uint32_t n_lines[1] = {in.n_lines};
        utk_merge_cfg cfg = {L.U.blob, L.U.blob_n, L.U.off, n_u, L.trunc_off, L.trunc_ids, L.n_trunc, 1, maps, n_lines, W, 4, 0, device,
                             in.is_ctr, 0, cap_nodes, cap_raw, 1};
        rc = utk_merge_open(&cfg, &D);                                         /* (it copies what it needs of cfg's arrays to the device) */
        if (rc) goto done;
        for (uint32_t p = 0; p < n_pass; ++p) {
            utk_merge_slice sl[1];
            utree_merge_slices(&in, 1, 0, bounds, p, sl);
            uint64_t got = 0;
            uint32_t err = 0, io_slice = 0;
            rc = utk_inspect_pass(D, sl, 1, at, in.n, d_lo, d_hi, d_lab, &got, &err, &io_slice);
            if (rc == UTREE_E_IO) utree_merge_fail_text(rc, "%s: cannot read its nodes%s", in.path, "");
            if (rc) goto done;
            if (err & 2u) { rc = utree_merge_fail_text(UTREE_E_FORMAT, "%s: a node's label index names no label line of its input%s", report_path, ""); goto done; }
            if (err & 1u) { rc = utree_merge_fail_text(UTREE_E_FORMAT, "%s: the words of a .ubt input are not strictly ascending%s", report_path, ""); goto done; }
            if (err & 4u) { rc = utree_merge_fail_text(UTREE_E_UNSUPPORTED, "%s: a .ctr input whose words, rebuilt from its bins, are not strictly ascending (xtree-compress's first-bin quirk does that when the first prefix holds one node): its words cannot be reconstructed%s", report_path, ""); goto done; }
            at += got;
        }
        utk_merge_close(D); D = NULL;                                          /* the passes' buffers go before the neighbour pass */
        if (at != in.n) { rc = utree_merge_fail_text(UTREE_E_HIP, "%s: the passes do not cover the input's nodes%s", report_path, ""); goto done; }
        /* ---- the neighbour pass ---- */
        rc = utk_inspect_neighbours(X, at, &no);
        if (rc) goto done;
        if (timing_on()) fprintf(stderr, "[utree_amd] inspect: neighbour pass %.6f s, %llu nodes, %llu lookups\n", no.seconds, (unsigned long long)at,
                                 (unsigned long long)at * 3ull * (W == 4 ? 16u : 4u * W));
        if (no.overflow) {
            rc = pairs_path ? fail_num(UTREE_E_NOMEM, "%s: more than UTREE_INSPECT_PAIRS=%s distinct label pairs one substitution apart; raise it", db_path, pair_cap)
                            : fail_num(UTREE_E_NOMEM, "%s: more than %s distinct label pairs one substitution apart: too many to count", db_path, pair_cap);
            goto done;
        }
        st.seconds_neighbours = no.seconds;
    }
    /* ---- figures per label text, the pairs ---- */
    fig = (uint64_t *)calloc((size_t)UTK_INSPECT_FIGURES * (n_u ? n_u : 1), 8);
    entry_of_u = (uint32_t *)malloc(4 * (size_t)(n_u ? n_u : 1));
    e = (utree_inspect_entry *)calloc(n_u ? n_u : 1, sizeof *e);
    const size_t n_dev_pairs = pairs_path ? (size_t)no.distinct_pairs : 0;
    pr = (utree_inspect_pair *)calloc(n_dev_pairs ? n_dev_pairs : 1, sizeof *pr);
    h_keys = (uint64_t *)malloc(8 * (n_dev_pairs ? n_dev_pairs : 1)); h_counts = (uint64_t *)malloc(8 * (n_dev_pairs ? n_dev_pairs : 1));
    if (!fig || !entry_of_u || !e || !pr || !h_keys || !h_counts) { rc = UTREE_E_NOMEM; goto done; }
    if (X) { rc = utk_inspect_figures(X, fig); if (rc) goto done; }
    for (uint32_t u = 0; u < n_u; ++u) {
        const uint64_t iso = fig[u], same = fig[(size_t)n_u + u], lin = fig[2 * (size_t)n_u + u], con = fig[3 * (size_t)n_u + u];
        entry_of_u[u] = 0xFFFFFFFFu;
        if (!(iso | same | lin | con)) continue;                               /* a ';'-prefix or a label line that no node carries */
        entry_of_u[u] = (uint32_t)n_e;
        e[n_e].text = L.U.blob + L.U.off[u]; e[n_e].len = L.U.len[u];
        e[n_e].isolated = iso; e[n_e].same = same; e[n_e].lineage = lin; e[n_e].conflict = con;
        ++n_e;
    }
    if (n_dev_pairs) {
        rc = utk_inspect_pairs(X, h_keys, h_counts);
        if (rc) goto done;
        for (size_t i = 0; i < n_dev_pairs; ++i) {
            const uint32_t from = (uint32_t)(h_keys[i] >> 24), to = (uint32_t)(h_keys[i] & 0xFFFFFFu);
            if (from >= n_u || to >= n_u || entry_of_u[from] == 0xFFFFFFFFu || entry_of_u[to] == 0xFFFFFFFFu) { rc = utree_merge_fail_text(UTREE_E_HIP, "%s: the device reported a pair between labels without nodes%s", report_path, ""); goto done; }
            pr[n_pr].from = entry_of_u[from]; pr[n_pr].to = entry_of_u[to]; pr[n_pr].pairs = h_counts[i];
            ++n_pr;
        }
    }
    {
        const utree_compare_input id = {db_path, (uint32_t)in.is_ctr, W, in.I, 0};
        const uint32_t passes = st.n_passes;
        const double nb = st.seconds_neighbours;
        rc = utree_inspect_write(&id, e, n_e, pr, n_pr, no.pair_events, no.distinct_pairs, report_path, pairs_path, &st);
        if (rc == UTREE_E_ARG) rc = utree_merge_fail_text(UTREE_E_HIP, "%s: the device's pairs are not symmetric%s", report_path, "");
        st.n_passes = passes; st.seconds_neighbours = nb; st.W = W; st.I = in.I; st.is_ctr = (uint32_t)in.is_ctr;
        if (!rc && (st.kmers != in.n || st.pair_events != no.pair_events || st.distinct_pairs != no.distinct_pairs)) {
            rc = utree_merge_fail_text(UTREE_E_HIP, "%s: the device's counters do not cover the input's nodes and pairs%s", report_path, "");
            unlink(report_path);
            if (pairs_path) unlink(pairs_path);
        }
    }
done:
    if (D) utk_merge_close(D);
    if (X) utk_inspect_close(X);
    utree_merge_input_close(&in);
    universe_free(&L);
    free(bounds); free(depth); free(entry_of_u); free(fig); free(h_keys); free(h_counts); free(e); free(pr);
    st.seconds = now_s() - t0;
    *stats = st;
    return rc;
}
