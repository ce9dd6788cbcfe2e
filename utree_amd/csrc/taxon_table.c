/* taxon_table.c -- host: merge taxa by text, roll up over their ';'-prefixes, write (the profile's and the coverage file's rows; the layouts are
 * in include/utree_amd.h: utree_profile_write, utree_coverage_write). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "utree_internal.h"
#include "taxon_table.h"

static int text_cmp(const char *a, uint32_t la, const char *b, uint32_t lb) {
    const uint32_t m = la < lb ? la : lb;
    const int c = m ? memcmp(a, b, m) : 0;
    if (c) return c;
    return la < lb ? -1 : la > lb;
}
static int row_cmp(const void *a, const void *b) {
    const utree_taxon_row *x = (const utree_taxon_row *)a, *y = (const utree_taxon_row *)b;
    return text_cmp(x->s, x->len, y->s, y->len);
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
        const int c = text_cmp(r[mid].s, r[mid].len, s, len);
        if (!c) return &r[mid];
        if (c < 0) lo = mid + 1; else hi = mid;
    }
    return NULL;
}

int utree_taxon_table_write(utree_taxon_row *t, size_t n, int n_fig, int key, const char *header, const char *path) {
    const size_t nt = merge_rows(t, n);                      /* one row per distinct text */
    size_t nr = 0;
    for (size_t i = 0; i < nt; ++i) {
        if (!t[i].own[key]) continue;
        ++nr;
        for (uint32_t j = 0; j < t[i].len; ++j) nr += t[i].s[j] == ';';
    }
    utree_taxon_row *r = (utree_taxon_row *)calloc(nr ? nr : 1, sizeof *r);
    if (!r) return UTREE_E_NOMEM;
    size_t k = 0;
    for (size_t i = 0; i < nt; ++i) {                        /* the rows: every text with the key figure and every ';'-prefix of one */
        if (!t[i].own[key]) continue;
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
        if (o) for (int q = 0; q < n_fig; ++q) o->clade[q] += t[i].own[q];
        for (uint32_t j = 0; j < t[i].len; ++j)
            if (t[i].s[j] == ';' && (o = find_row(r, nr, t[i].s, j))) for (int q = 0; q < n_fig; ++q) o->clade[q] += t[i].own[q];
    }
    FILE *f = fopen(path, "wb");
    if (!f) { free(r); return UTREE_E_IO; }
    int bad = fputs(header, f) < 0;
    for (size_t i = 0; i < nr && !bad; ++i) {
        if (r[i].len && fwrite(r[i].s, 1, r[i].len, f) != r[i].len) bad = 1;
        for (int q = 0; q < 2 * n_fig; ++q)
            if (fprintf(f, "\t%llu", (unsigned long long)(q < n_fig ? r[i].own[q] : r[i].clade[q - n_fig])) < 0) bad = 1;
        if (fputc('\n', f) == EOF) bad = 1;
    }
    free(r);
    if (fclose(f) != 0) bad = 1;
    return bad ? UTREE_E_IO : UTREE_OK;
}
