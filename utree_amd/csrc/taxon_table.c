/* taxon_table.c -- host: merge taxa by text, roll up over their ';'-prefixes, write (the profile's and the coverage file's rows; the layouts are
 * in include/utree_amd.h: utree_profile_write, utree_coverage_write); and the matrix of taxa by samples that the sample table and the per-sample
 * redistribution are (utree_samples_write, utree_sredist_write). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "utree_internal.h"
#include "taxon_table.h"

int utree_text_cmp(const void *a, uint64_t la, const void *b, uint64_t lb) {
    const uint64_t m = la < lb ? la : lb;
    const int c = m ? memcmp(a, b, m) : 0;
    if (c) return c;
    return la < lb ? -1 : la > lb;
}
static int row_cmp(const void *a, const void *b) {
    const utree_taxon_row *x = (const utree_taxon_row *)a, *y = (const utree_taxon_row *)b;
    return utree_text_cmp(x->s, x->len, y->s, y->len);
}
/* sort rows by text and add up the own figures of rows of equal text; returns the count left */
static size_t merge_rows(utree_taxon_row *r, size_t n) {
    if (!n) return 0;
    qsort(r, n, sizeof *r, row_cmp);
    size_t w = 0;
    for (size_t i = 1; i < n; ++i) {
        if (!row_cmp(&r[w], &r[i])) for (int q = 0; q < UTREE_TAXON_FIGURES; ++q) r[w].own[q] += r[i].own[q];
        else r[++w] = r[i];
    }
    return w + 1;
}
static utree_taxon_row *find_row(utree_taxon_row *r, size_t n, const char *s, uint32_t len) {
    size_t lo = 0, hi = n;
    while (lo < hi) {
        const size_t mid = (lo + hi) / 2;
        const int c = utree_text_cmp(r[mid].s, r[mid].len, s, len);
        if (!c) return &r[mid];
        if (c < 0) lo = mid + 1; else hi = mid;
    }
    return NULL;
}

int utree_taxon_table_write(utree_taxon_row *t, size_t n, int n_fig, int key, const char *header, const char *path) {
    return utree_taxon_table_write_wide(t, n, n_fig, n_fig, key, header, path);
}

int utree_taxon_table_write_wide(utree_taxon_row *t, size_t n, int n_own, int n_clade, int key, const char *header, const char *path) {
    static const int first[UTREE_TAXON_FIGURES] = {0, 1, 2, 3, 4, 5, 6};
    return utree_taxon_table_write_pick(t, n, n_own, first, n_clade, key, header, path);
}

int utree_taxon_table_write_pick(utree_taxon_row *t, size_t n, int n_own, const int *clade_of, int n_clade, int key, const char *header, const char *path) {
    const size_t nt = merge_rows(t, n);                      /* one row per distinct text */
    size_t nr = 0;
    for (size_t i = 0; i < nt; ++i) {
        if (key >= 0 && !t[i].own[key]) continue;
        ++nr;
        for (uint32_t j = 0; j < t[i].len; ++j) nr += t[i].s[j] == ';';
    }
    utree_taxon_row *r = (utree_taxon_row *)calloc(nr ? nr : 1, sizeof *r);
    if (!r) return UTREE_E_NOMEM;
    size_t k = 0;
    for (size_t i = 0; i < nt; ++i) {                        /* the rows: every text with the key figure and every ';'-prefix of one */
        if (key >= 0 && !t[i].own[key]) continue;
        r[k++] = t[i];
        for (uint32_t j = 0; j < t[i].len; ++j)
            if (t[i].s[j] == ';') { r[k].s = t[i].s; r[k].len = j; ++k; }
    }
    nr = merge_rows(r, k);
    for (size_t i = 0; i < nr; ++i) {                        /* a prefix row that is also some input's whole text (key figure or not) shows that input's figures */
        const utree_taxon_row *o = find_row(t, nt, r[i].s, r[i].len);
        for (int q = 0; q < UTREE_TAXON_FIGURES; ++q) { r[i].own[q] = o ? o->own[q] : 0; r[i].clade[q] = 0; }
    }
    for (size_t i = 0; i < nt; ++i) {                        /* clade figures: over ALL inputs whose text is the row's or begins with it + ';' */
        utree_taxon_row *o = find_row(r, nr, t[i].s, t[i].len);
        if (o) for (int q = 0; q < n_clade; ++q) o->clade[q] += t[i].own[clade_of[q]];
        for (uint32_t j = 0; j < t[i].len; ++j)
            if (t[i].s[j] == ';' && (o = find_row(r, nr, t[i].s, j))) for (int q = 0; q < n_clade; ++q) o->clade[q] += t[i].own[clade_of[q]];
    }
    FILE *f = fopen(path, "wb");
    if (!f) { free(r); return UTREE_E_IO; }
    int bad = fputs(header, f) < 0;
    for (size_t i = 0; i < nr && !bad; ++i) {
        if (r[i].len && fwrite(r[i].s, 1, r[i].len, f) != r[i].len) bad = 1;
        for (int q = 0; q < n_own + n_clade; ++q)
            if (fprintf(f, "\t%llu", (unsigned long long)(q < n_own ? r[i].own[q] : r[i].clade[q - n_own])) < 0) bad = 1;
        if (fputc('\n', f) == EOF) bad = 1;
    }
    free(r);
    if (fclose(f) != 0) bad = 1;
    return bad ? UTREE_E_IO : UTREE_OK;
}

/* ---- taxa by samples --------------------------------------------------------------------------------------------------------- */
static int col_cmp(const void *a, const void *b) {
    const utree_matrix_col *x = *(const utree_matrix_col *const *)a, *y = *(const utree_matrix_col *const *)b;
    return utree_text_cmp(x->s, x->len, y->s, y->len);
}
static int cell_cmp(const void *a, const void *b) {
    const utree_matrix_cell *x = (const utree_matrix_cell *)a, *y = (const utree_matrix_cell *)b;
    const int c = utree_text_cmp(x->s, x->len, y->s, y->len);
    if (c) return c;
    return x->col < y->col ? -1 : x->col > y->col;
}
static int put_id(FILE *f, const uint8_t *s, uint64_t len) {           /* TAB, CR and backslash escaped, nothing else */
    for (uint64_t i = 0; i < len; ++i) {
        const int c = s[i];
        const int r = c == '\t' ? fputs("\\t", f) : c == '\r' ? fputs("\\r", f) : c == '\\' ? fputs("\\\\", f) : fputc(c, f);
        if (r == EOF) return 1;
    }
    return 0;
}

int utree_sample_matrix_write(const char *header, const utree_matrix_col *col, size_t S, int merge, const utree_matrix_extra *extra, size_t n_extra,
                              utree_matrix_cell *e, size_t q, const char *path) {
    const size_t R = 3 + n_extra;                                        /* figures of a column: reads, unclassified, the extra rows, the sum of its cells */
    const utree_matrix_col **by = (const utree_matrix_col **)calloc(S ? S : 1, sizeof *by);     /* written position -> (first) column */
    uint32_t *pos = (uint32_t *)calloc(S ? S : 1, 4);                    /* the caller's column -> written position */
    uint64_t *fig = (uint64_t *)calloc((S ? S : 1) * R, 8), *sum = fig + (R - 1) * S;           /* fig[r * S + j]: figure r of written column j */
    size_t C = 0;
    int rc = UTREE_OK;
    FILE *f = NULL;
    if (!by || !pos || !fig) { rc = UTREE_E_NOMEM; goto done; }
    for (size_t j = 0; j < S; ++j) by[j] = &col[j];
    qsort(by, S, sizeof *by, col_cmp);                                   /* the columns: unsigned bytewise order, shorter first */
    for (size_t j = 0; j < S; ++j) {
        const size_t i = (size_t)(by[j] - col);
        if (!j || col_cmp(&by[j - 1], &by[j])) by[C++] = by[j];
        else if (!merge) { rc = UTREE_E_ARG; goto done; }                /* two samples with one id */
        pos[i] = (uint32_t)(C - 1);
        fig[C - 1] += col[i].reads; fig[S + C - 1] += col[i].uncl;
        for (size_t x = 0; x < n_extra; ++x) fig[(2 + x) * S + C - 1] += extra[x].v[i];
    }
    for (size_t i = 0; i < q; ++i) {
        if (e[i].col >= S) { rc = UTREE_E_ARG; goto done; }
        e[i].col = pos[e[i].col];
    }
    qsort(e, q, sizeof *e, cell_cmp);
    size_t w = 0;
    for (size_t i = 0; i < q; ++i) {                                     /* entries of equal text in one column are one cell */
        if (w && !cell_cmp(&e[w - 1], &e[i])) e[w - 1].reads += e[i].reads;
        else e[w++] = e[i];
    }
    for (size_t i = 0; i < w; ++i) sum[e[i].col] += e[i].reads;
    for (size_t j = 0; j < C; ++j)
        if (fig[S + j] > fig[j] || sum[j] != fig[j] - fig[S + j]) { rc = UTREE_E_ARG; goto done; }      /* column j sums to n_j - u_j */
    f = fopen(path, "wb");
    if (!f) { rc = UTREE_E_IO; goto done; }
    int bad = fprintf(f, "%s\tsamples\t%llu\n# taxon", header, (unsigned long long)C) < 0;
    for (size_t j = 0; j < C && !bad; ++j) bad = fputc('\t', f) == EOF || put_id(f, by[j]->s, by[j]->len);
    for (size_t r = 0; r + 1 < R; ++r) {
        bad |= fprintf(f, "\n# %s", r == 0 ? "reads" : r == 1 ? "unclassified" : extra[r - 2].name) < 0;
        for (size_t j = 0; j < C && !bad; ++j) bad = fprintf(f, "\t%llu", (unsigned long long)fig[r * S + j]) < 0;
    }
    bad |= fputc('\n', f) == EOF;
    for (size_t i = 0; i < w && !bad;) {                                 /* a row: the cells of one text, zeros where a sample has none */
        size_t end = i;
        while (end < w && !utree_text_cmp(e[i].s, e[i].len, e[end].s, e[end].len)) ++end;
        if (e[i].len && fwrite(e[i].s, 1, e[i].len, f) != e[i].len) bad = 1;
        size_t at = i;
        for (size_t j = 0; j < C && !bad; ++j) {
            if (at < end && e[at].col == j) bad = fprintf(f, "\t%llu", (unsigned long long)e[at++].reads) < 0;
            else bad = fputs("\t0", f) < 0;
        }
        if (fputc('\n', f) == EOF) bad = 1;
        i = end;
    }
    if (fclose(f) != 0) bad = 1;
    f = NULL;
    if (bad) rc = UTREE_E_IO;
done:
    if (f) fclose(f);
    free((void *)by); free(pos); free(fig);
    return rc;
}
