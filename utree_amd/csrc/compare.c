/* compare.c -- host side of utree_compare_files (`utree-compare`) and the writer of its two files, utree_compare_write.  include/utree_amd.h
 * states what a compare is.  The inputs are opened, cut into passes and laid out in slices by the merge's own functions (merge_input.h), with A
 * as input 0 and B as input 1 over one label universe, so equal text is an equal id; the device (merge_kernels.hip: utk_compare_pass) decodes
 * and sorts as for a merge, classifies every run of equal words into per-label counters and hands back each pass's distinct (label in A, label
 * in B) pairs, which are added up here across the passes.
 */
#define _FILE_OFFSET_BITS 64
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "utree_internal.h"
#include "merge_input.h"
#include "taxon_table.h"

enum { F_A, F_B, F_SAME, F_ONLY_A, F_ONLY_B, F_LEFT, F_ARRIVED, N_FIG };       /* a row's own figures, in the order the report prints them */

/* ---- the writer ------------------------------------------------------------------------------------------------------------------ */
static int by_entry_text(const void *x, const void *y, void *entries) {
    const utree_compare_entry *e = (const utree_compare_entry *)entries, *a = &e[*(const uint32_t *)x], *b = &e[*(const uint32_t *)y];
    return utree_text_cmp(a->text, a->len, b->text, b->len);
}
typedef struct { uint32_t from, to; uint64_t kmers; } group_move;              /* between rows, which stand in text order */
static int by_from_to(const void *x, const void *y) {
    const group_move *a = (const group_move *)x, *b = (const group_move *)y;
    if (a->from != b->from) return a->from < b->from ? -1 : 1;
    return a->to < b->to ? -1 : a->to > b->to;
}
static const char *kind_of(const utree_taxon_row *from, const utree_taxon_row *to) {
    if (from->len > to->len && from->s[to->len] == ';' && !memcmp(from->s, to->s, to->len)) return "lifted";
    if (to->len > from->len && to->s[from->len] == ';' && !memcmp(from->s, to->s, from->len)) return "lowered";
    return "moved";
}

int utree_compare_write(const utree_compare_input *a, const utree_compare_input *b, const utree_compare_entry *e, size_t n,
                        const utree_compare_move *m, size_t n_moves, const char *report_path, const char *moves_path, utree_compare_stats *stats) {
    if (!a || !b || !a->path || !b->path || !report_path || (n && !e) || (n_moves && !m) || n >= 0xFFFFFFFFu) return UTREE_E_ARG;
    for (size_t i = 0; i < n; ++i) if (e[i].len && !e[i].text) return UTREE_E_ARG;
    for (size_t i = 0; i < n_moves; ++i) if (m[i].from >= n || m[i].to >= n) return UTREE_E_ARG;
    utree_compare_stats st; memset(&st, 0, sizeof st);
    int rc = UTREE_OK;
    uint32_t *order = (uint32_t *)malloc(4 * (n ? n : 1)), *row_of = (uint32_t *)malloc(4 * (n ? n : 1));
    utree_taxon_row *t = (utree_taxon_row *)calloc(n ? n : 1, sizeof *t);
    group_move *gm = (group_move *)malloc(sizeof *gm * (n_moves ? n_moves : 1));
    uint64_t *out_sum = (uint64_t *)calloc(2 * (n ? n : 1), 8), *in_sum = out_sum ? out_sum + (n ? n : 1) : NULL;
    char *header = (char *)malloc(strlen(a->path) + strlen(b->path) + 1024);
    size_t nt = 0, ngm = 0;
    if (!order || !row_of || !t || !gm || !out_sum || !header) { rc = UTREE_E_NOMEM; goto done; }
    /* ---- one row per distinct text, in text order; entries of equal text are added up ---- */
    for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
    qsort_r(order, n, 4, by_entry_text, (void *)e);
    for (size_t i = 0; i < n; ++i) {
        const utree_compare_entry *x = &e[order[i]];
        if (!nt || utree_text_cmp(t[nt - 1].s, t[nt - 1].len, x->text, x->len)) { t[nt].s = x->text; t[nt].len = x->len; ++nt; }
        uint64_t *own = t[nt - 1].own;
        own[F_SAME] += x->same; own[F_ONLY_A] += x->only_a; own[F_ONLY_B] += x->only_b; own[F_LEFT] += x->left; own[F_ARRIVED] += x->arrived;
        row_of[order[i]] = (uint32_t)(nt - 1);
    }
    for (size_t r = 0; r < nt; ++r) {
        uint64_t *own = t[r].own;
        own[F_A] = own[F_SAME] + own[F_ONLY_A] + own[F_LEFT];
        own[F_B] = own[F_SAME] + own[F_ONLY_B] + own[F_ARRIVED];
        st.a += own[F_A]; st.b += own[F_B]; st.same += own[F_SAME]; st.only_a += own[F_ONLY_A]; st.only_b += own[F_ONLY_B];
        st.left += own[F_LEFT]; st.arrived += own[F_ARRIVED];
        st.a_labels += own[F_A] != 0; st.b_labels += own[F_B] != 0;
    }
    /* ---- the moves between rows, equal pairs added up; they must account for every row's left and arrived ---- */
    for (size_t i = 0; i < n_moves; ++i) {
        gm[i].from = row_of[m[i].from]; gm[i].to = row_of[m[i].to]; gm[i].kmers = m[i].kmers;
        if (gm[i].from == gm[i].to) { rc = UTREE_E_ARG; goto done; }
    }
    qsort(gm, n_moves, sizeof *gm, by_from_to);
    for (size_t i = 0; i < n_moves; ++i) {
        if (!gm[i].kmers) continue;                                            /* no word made it: not a move */
        if (ngm && !by_from_to(&gm[ngm - 1], &gm[i])) gm[ngm - 1].kmers += gm[i].kmers;
        else gm[ngm++] = gm[i];
        out_sum[gm[i].from] += gm[i].kmers; in_sum[gm[i].to] += gm[i].kmers;
    }
    for (size_t r = 0; r < nt; ++r) if (out_sum[r] != t[r].own[F_LEFT] || in_sum[r] != t[r].own[F_ARRIVED]) { rc = UTREE_E_ARG; goto done; }
    if (st.left != st.arrived) { rc = UTREE_E_ARG; goto done; }
    st.n_moves = ngm;
    st.both = st.same + st.left;
    st.words = st.both + st.only_a + st.only_b;
    st.W = a->W;
    st.identical = !st.left && !st.only_a && !st.only_b;
    /* ---- the report: rows without a word leave (the table merges and sorts in place: compact first) ---- */
    {
        size_t w = 0;
        for (size_t r = 0; r < nt; ++r) if (t[r].own[F_A] + t[r].own[F_B]) { row_of[r] = (uint32_t)w; t[w++] = t[r]; }   /* row_of: old row -> kept row; a row a move names has words */
        for (size_t i = 0; i < ngm; ++i) { gm[i].from = row_of[gm[i].from]; gm[i].to = row_of[gm[i].to]; }
        nt = w;
    }
    sprintf(header, "# a\t%s\t%s\t%u\t%u\t%llu\t%llu\n# b\t%s\t%s\t%u\t%u\t%llu\t%llu\n"
                    "# words\t%llu\tboth\t%llu\tsame\t%llu\tchanged\t%llu\tonly_a\t%llu\tonly_b\t%llu\n"
                    "# taxon\ta\tb\tsame\tonly_a\tonly_b\tleft\tarrived\tclade_a\tclade_b\n",
            a->path, a->is_ctr ? ".ctr" : ".ubt", a->W, a->I, (unsigned long long)st.a, (unsigned long long)st.a_labels,
            b->path, b->is_ctr ? ".ctr" : ".ubt", b->W, b->I, (unsigned long long)st.b, (unsigned long long)st.b_labels,
            (unsigned long long)st.words, (unsigned long long)st.both, (unsigned long long)st.same, (unsigned long long)st.left,
            (unsigned long long)st.only_a, (unsigned long long)st.only_b);
    if (moves_path) {                                                          /* before the table, which sorts and merges t in place */
        FILE *f = fopen(moves_path, "wb");
        if (!f) { rc = utree_merge_fail_text(UTREE_E_IO, "%s: cannot create%s", moves_path, ""); goto done; }
        int bad = fputs("# from\tto\tkmers\tkind\n", f) < 0;
        for (size_t i = 0; i < ngm && !bad; ++i) {
            const utree_taxon_row *x = &t[gm[i].from], *y = &t[gm[i].to];
            if (x->len && fwrite(x->s, 1, x->len, f) != x->len) bad = 1;
            if (fputc('\t', f) == EOF) bad = 1;
            if (y->len && fwrite(y->s, 1, y->len, f) != y->len) bad = 1;
            if (fprintf(f, "\t%llu\t%s\n", (unsigned long long)gm[i].kmers, kind_of(x, y)) < 0) bad = 1;
        }
        if (fclose(f) != 0) bad = 1;
        if (bad) { rc = utree_merge_fail_text(UTREE_E_IO, "%s: cannot write%s", moves_path, ""); goto done; }
    }
    rc = utree_taxon_table_write_wide(t, nt, N_FIG, 2, -1, header, report_path);
    if (rc == UTREE_E_IO) utree_merge_fail_text(rc, "%s: cannot write%s", report_path, "");
done:
    if (rc == UTREE_E_IO || rc == UTREE_E_NOMEM) {                             /* a failed call leaves neither file behind (UTREE_E_ARG came before either was created) */
        unlink(report_path);
        if (moves_path) unlink(moves_path);
    }
    free(order); free(row_of); free(t); free(gm); free(out_sum); free(header);
    if (stats && !rc) *stats = st;
    return rc;
}

/* ---- the compare ----------------------------------------------------------------------------------------------------------------- */
typedef struct { uint64_t key, kmers; } pair_count;                            /* key: universe id in A << 24 | universe id in B */
static int by_key(const void *x, const void *y) {
    const pair_count *a = (const pair_count *)x, *b = (const pair_count *)y;
    return a->key < b->key ? -1 : a->key > b->key;
}

int utree_compare_files(const char *a_path, const char *b_path, const char *report_path, const char *moves_path, int device, utree_compare_stats *stats) {
    if (!a_path || !b_path || !report_path || !stats) return UTREE_E_ARG;
    const double t0 = now_s();
    const char *paths[2] = {a_path, b_path};
    utree_compare_stats st; memset(&st, 0, sizeof st);
    int rc = UTREE_OK;
    merge_in ins[2];
    memset(ins, 0, sizeof ins);
    ins[0].fd = ins[1].fd = -1;
    label_universe L; memset(&L, 0, sizeof L);
    uint32_t *bounds = NULL, n_pass = 0, *entry_of_u = NULL, *h_counts = NULL;
    utk_merge_dev *D = NULL;
    uint64_t *fig = NULL, *h_keys = NULL, h_cap = 0;
    pair_count *pairs = NULL;
    size_t n_pairs = 0, pairs_cap = 0, n_e = 0;
    utree_compare_entry *e = NULL;
    utree_compare_move *mv = NULL;
    /* ---- the inputs, as the merge reads them ---- */
    uint64_t n_read = 0;
    uint32_t rec_max = 0;
    for (int i = 0; i < 2; ++i) {
        rc = utree_merge_input_open(&ins[i], paths[i], &L, NULL, NULL, 0, NULL);
        if (rc) goto done;
        if (i && ins[i].W != ins[0].W) { rc = utree_merge_fail_text(UTREE_E_UNSUPPORTED, "%s: its word size differs from the first input's%s", paths[i], ""); goto done; }
        if (ins[i].rec > rec_max) rec_max = ins[i].rec;
        ins[i].g0 = n_read;
        n_read += ins[i].n;
    }
    const uint32_t W = ins[0].W;
    st.W = W;
    if (n_read >= (1ull << 40)) { rc = utree_merge_fail_text(UTREE_E_UNSUPPORTED, "%s: 2^40 nodes or more in all%s", report_path, ""); goto done; }
    if (universe_close(&L)) { rc = UTREE_E_NOMEM; goto done; }
    const uint32_t n_u = L.U.n;
    /* ---- passes and device ---- */
    uint64_t limit = 0, cap_nodes = 0, cap_raw = 0;
    rc = utk_compare_limit(device, W, rec_max, n_u, &limit);
    if (rc) goto done;
    rc = utree_merge_plan(ins, 2, n_read, limit, report_path, &bounds, &n_pass, &cap_nodes, &cap_raw);
    if (rc) goto done;
    st.n_passes = n_pass;
    {
        const uint32_t *maps[2] = {ins[0].u_of_ix, ins[1].u_of_ix};
        const uint32_t n_lines[2] = {ins[0].n_lines, ins[1].n_lines};
        utk_merge_cfg cfg = {L.U.blob, L.U.blob_n, L.U.off, n_u, L.trunc_off, L.trunc_ids, L.n_trunc, 2, maps, n_lines, W, 4, 0, device,
                             ins[0].is_ctr | ins[1].is_ctr, 0, cap_nodes, cap_raw, 1};
        rc = utk_merge_open(&cfg, &D);                                         /* (it copies what it needs of cfg's arrays to the device) */
        if (rc) goto done;
        for (uint32_t p = 0; p < n_pass; ++p) {
            utk_merge_slice sl[2];
            utree_merge_slices(ins, 2, 0, bounds, p, sl);
            utk_compare_pass_out po;
            uint32_t io_slice = 0;
            rc = utk_compare_pass(D, sl, 2, ins[1].g0, &po, &io_slice);
            if (rc == UTREE_E_IO) utree_merge_fail_text(rc, "%s: cannot read its nodes%s", ins[io_slice].path, "");
            if (rc) goto done;
            if (po.err & 2u) { rc = utree_merge_fail_text(UTREE_E_FORMAT, "%s: a node's label index names no label line of its input%s", report_path, ""); goto done; }
            if (po.err & 1u) { rc = utree_merge_fail_text(UTREE_E_FORMAT, "%s: the words of a .ubt input are not strictly ascending%s", report_path, ""); goto done; }
            if (po.err & 4u) { rc = utree_merge_fail_text(UTREE_E_UNSUPPORTED, "%s: a .ctr input whose words, rebuilt from its bins, are not strictly ascending (xtree-compress's first-bin quirk does that when the first prefix holds one node): its words cannot be reconstructed%s", report_path, ""); goto done; }
            if (!po.n_moves) continue;
            if (n_pairs + po.n_moves > pairs_cap) {
                pairs_cap = (n_pairs + po.n_moves) * 2;
                pair_count *np = (pair_count *)realloc(pairs, sizeof *np * pairs_cap);
                if (!np) { rc = UTREE_E_NOMEM; goto done; }
                pairs = np;
            }
            if (po.n_moves > h_cap) {                                              /* a pass's pairs come down into buffers that grow to the largest pass's */
                free(h_keys); free(h_counts);
                h_cap = po.n_moves;
                h_keys = (uint64_t *)malloc(8 * (size_t)h_cap); h_counts = (uint32_t *)malloc(4 * (size_t)h_cap);
                if (!h_keys || !h_counts) { rc = UTREE_E_NOMEM; goto done; }
            }
            rc = utk_compare_moves(D, h_keys, h_counts);
            if (rc) goto done;
            for (uint64_t i = 0; i < po.n_moves; ++i) { pairs[n_pairs].key = h_keys[i]; pairs[n_pairs].kmers = h_counts[i]; ++n_pairs; }
        }
    }
    /* ---- figures per label text, moves across the passes ---- */
    fig = (uint64_t *)calloc((size_t)UTK_COMPARE_FIGURES * (n_u ? n_u : 1), 8);
    entry_of_u = (uint32_t *)malloc(4 * (size_t)(n_u ? n_u : 1));
    e = (utree_compare_entry *)calloc(n_u ? n_u : 1, sizeof *e);
    mv = (utree_compare_move *)calloc(n_pairs ? n_pairs : 1, sizeof *mv);
    if (!fig || !entry_of_u || !e || !mv) { rc = UTREE_E_NOMEM; goto done; }
    if (n_read) { rc = utk_compare_figures(D, fig); if (rc) goto done; }
    for (uint32_t u = 0; u < n_u; ++u) {
        const uint64_t same = fig[u], only_a = fig[(size_t)n_u + u], only_b = fig[2 * (size_t)n_u + u], left = fig[3 * (size_t)n_u + u], arrived = fig[4 * (size_t)n_u + u];
        entry_of_u[u] = 0xFFFFFFFFu;
        if (!(same | only_a | only_b | left | arrived)) continue;             /* a ';'-prefix or a label line that no node carries */
        entry_of_u[u] = (uint32_t)n_e;
        e[n_e].text = L.U.blob + L.U.off[u]; e[n_e].len = L.U.len[u];
        e[n_e].same = same; e[n_e].only_a = only_a; e[n_e].only_b = only_b; e[n_e].left = left; e[n_e].arrived = arrived;
        ++n_e;
    }
    qsort(pairs, n_pairs, sizeof *pairs, by_key);
    size_t n_mv = 0;
    for (size_t i = 0; i < n_pairs; ++i) {
        const uint32_t from = (uint32_t)(pairs[i].key >> 24), to = (uint32_t)(pairs[i].key & 0xFFFFFFu);
        if (i && pairs[i].key == pairs[i - 1].key) { mv[n_mv - 1].kmers += pairs[i].kmers; continue; }
        if (from >= n_u || to >= n_u || entry_of_u[from] == 0xFFFFFFFFu || entry_of_u[to] == 0xFFFFFFFFu) { rc = utree_merge_fail_text(UTREE_E_HIP, "%s: the device reported a move between labels without words%s", report_path, ""); goto done; }
        mv[n_mv].from = entry_of_u[from]; mv[n_mv].to = entry_of_u[to]; mv[n_mv].kmers = pairs[i].kmers;
        ++n_mv;
    }
    {
        const utree_compare_input ia = {a_path, (uint32_t)ins[0].is_ctr, W, ins[0].I, 0}, ib = {b_path, (uint32_t)ins[1].is_ctr, W, ins[1].I, 0};
        const uint32_t passes = st.n_passes;
        rc = utree_compare_write(&ia, &ib, e, n_e, mv, n_mv, report_path, moves_path, &st);
        if (rc == UTREE_E_ARG) rc = utree_merge_fail_text(UTREE_E_HIP, "%s: the device's counters and moves do not add up%s", report_path, "");
        st.n_passes = passes; st.W = W;
        if (!rc && (st.a != ins[0].n || st.b != ins[1].n)) {
            rc = utree_merge_fail_text(UTREE_E_HIP, "%s: the device's counters do not cover the inputs' nodes%s", report_path, "");
            unlink(report_path);
            if (moves_path) unlink(moves_path);
        }
    }
done:
    if (D) utk_merge_close(D);
    utree_merge_input_close(&ins[0]); utree_merge_input_close(&ins[1]);
    universe_free(&L);
    free(bounds); free(entry_of_u); free(h_counts); free(fig); free(h_keys); free(pairs); free(e); free(mv);
    st.seconds = now_s() - t0;
    *stats = st;
    return rc;
}
