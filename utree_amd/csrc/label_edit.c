/* label_edit.c -- rule files and the per-label edit of utree_merge_files_edit; include/utree_amd.h states the contract, label_edit.h the
 * interface.  No device, no HIP: only libc and strtab.h. */
#define _FILE_OFFSET_BITS 64
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/utree_amd.h"
#include "label_edit.h"
#include "strtab.h"

enum { T_DROP = 0, T_KEEP = 1, T_OLD = 2, T_NEW = 3 };
#define NONE 0xFFFFFFFFu

typedef struct { uint32_t tab, id; uint64_t line; } rule_line;

struct le_rules {
    uint32_t ranks;
    char *path[3];                   /* NULL: no such file */
    strtab tab[4];                   /* the taxa of the drop lines, of the keep lines, the `old` and the `new` sides of the rename lines */
    uint32_t *new_of, new_cap;       /* id in tab[T_OLD] -> id in tab[T_NEW] */
    uint8_t *hit[3];                 /* per id: some label matched it */
    rule_line *lines; uint64_t n_lines, lines_cap;
    char *buf; size_t buf_cap;       /* le_apply's renamed text */
};

static int fail(int rc, char *err, size_t errn, const char *path, uint64_t line, const char *what) {
    if (err && errn) {
        if (line) snprintf(err, errn, "%s: line %llu: %s", path, (unsigned long long)line, what);
        else snprintf(err, errn, "%s: %s", path, what);
    }
    return rc;
}

static int push_line(le_rules *R, uint32_t tab, uint32_t id, uint64_t line) {
    if (R->n_lines == R->lines_cap) {
        const uint64_t nc = R->lines_cap ? R->lines_cap * 2 : 256;
        rule_line *a = (rule_line *)realloc(R->lines, sizeof(rule_line) * nc);
        if (!a) return -1;
        R->lines = a; R->lines_cap = nc;
    }
    R->lines[R->n_lines].tab = tab; R->lines[R->n_lines].id = id; R->lines[R->n_lines].line = line;
    ++R->n_lines;
    return 0;
}

/* one rule file: lines end at '\n' (the last one may lack it), one trailing '\r' goes, empty lines are skipped */
static int load_file(le_rules *R, uint32_t tab, const char *path, char *err, size_t errn) {
    FILE *f = fopen(path, "rb");
    if (!f) return fail(UTREE_E_IO, err, errn, path, 0, "cannot open the rule file");
    char *data = NULL;
    size_t n = 0, cap = 0;
    for (;;) {
        if (n + 65536 > cap) {
            cap = cap ? cap * 2 : (1u << 17);
            char *d = (char *)realloc(data, cap);
            if (!d) { free(data); fclose(f); return UTREE_E_NOMEM; }
            data = d;
        }
        const size_t got = fread(data + n, 1, cap - n, f);
        n += got;
        if (!got) break;
    }
    const int bad = ferror(f);
    fclose(f);
    if (bad) { free(data); return fail(UTREE_E_IO, err, errn, path, 0, "cannot read the rule file"); }
    int rc = UTREE_OK;
    uint64_t line = 0;
    for (size_t p = 0; p < n && !rc;) {
        const char *nl = (const char *)memchr(data + p, '\n', n - p);
        const char *s = data + p;
        size_t ll = nl ? (size_t)(nl - s) : n - p;
        p += ll + 1;
        ++line;
        if (ll && s[ll - 1] == '\r') --ll;
        if (!ll) continue;
        const char *tabc = (const char *)memchr(s, '\t', ll);
        int fresh;
        if (tab != T_OLD) {
            if (tabc) { rc = fail(UTREE_E_FORMAT, err, errn, path, line, "a TAB in a taxon line"); break; }
            const uint32_t id = st_intern(&R->tab[tab], s, ll, &fresh);
            if (id == NONE || push_line(R, tab, id, line)) rc = UTREE_E_NOMEM;
            continue;
        }
        const size_t lo = tabc ? (size_t)(tabc - s) : 0, ln = tabc ? ll - lo - 1 : 0;
        if (!tabc || !lo || !ln || memchr(tabc + 1, '\t', ln)) { rc = fail(UTREE_E_FORMAT, err, errn, path, line, "a rename line is `old TAB new`, one TAB, neither side empty"); break; }
        const uint32_t id = st_intern(&R->tab[T_OLD], s, lo, &fresh);
        if (id == NONE) { rc = UTREE_E_NOMEM; break; }
        if (!fresh) { rc = fail(UTREE_E_FORMAT, err, errn, path, line, "a second rename line with the same `old`"); break; }
        if (id >= R->new_cap) {
            const uint32_t nc = R->new_cap ? R->new_cap * 2 : 256;
            uint32_t *a = (uint32_t *)realloc(R->new_of, 4ull * nc);
            if (!a) { rc = UTREE_E_NOMEM; break; }
            R->new_of = a; R->new_cap = nc;
        }
        R->new_of[id] = st_intern(&R->tab[T_NEW], tabc + 1, ln, &fresh);
        if (R->new_of[id] == NONE || push_line(R, T_OLD, id, line)) rc = UTREE_E_NOMEM;
    }
    free(data);
    return rc;
}

void le_free(le_rules *R) {
    if (!R) return;
    for (int k = 0; k < 4; ++k) st_free(&R->tab[k]);
    for (int k = 0; k < 3; ++k) { free(R->path[k]); free(R->hit[k]); }
    free(R->new_of); free(R->lines); free(R->buf);
    free(R);
}

int le_load(le_rules **out, uint32_t ranks, const char *drop_path, const char *keep_path, const char *rename_path, char *err, size_t errn) {
    le_rules *R = (le_rules *)calloc(1, sizeof *R);
    if (!R) return UTREE_E_NOMEM;
    R->ranks = ranks;
    const char *paths[3] = {drop_path, keep_path, rename_path};
    int rc = UTREE_OK;
    for (uint32_t k = 0; k < 3 && !rc; ++k) {
        if (!paths[k]) continue;
        R->path[k] = strdup(paths[k]);
        if (!R->path[k]) { rc = UTREE_E_NOMEM; break; }
        rc = load_file(R, k, paths[k], err, errn);
        if (!rc && !(R->hit[k] = (uint8_t *)calloc((size_t)R->tab[k].n + 1, 1))) rc = UTREE_E_NOMEM;
    }
    if (rc) { le_free(R); return rc; }
    *out = R;
    return UTREE_OK;
}

/* the id of s[0 .. n) whose hash (strtab.h's hbytes) is h, or NONE */
static uint32_t find(const strtab *t, uint64_t h, const char *s, size_t n) {
    if (!t->nslot) return NONE;
    for (uint64_t q = h & (t->nslot - 1); t->slot[q] != NONE; q = (q + 1) & (t->nslot - 1)) {
        const uint32_t i = t->slot[q];
        if (t->len[i] == n && !memcmp(t->blob + t->off[i], s, n)) return i;
    }
    return NONE;
}

int le_apply(le_rules *R, const char *t, size_t n, const char **text, size_t *text_n) {
    /* a rule taxon matches t when it is t or t up to one of its ';': hbytes is a running hash, so every such prefix is looked up on one walk */
    int dropped = 0, kept = 0;
    uint32_t ren = NONE;
    size_t ren_len = 0;
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i <= n; ++i) {
        if (i == n || t[i] == ';') {
            uint32_t id;
            if (R->path[T_DROP] && (id = find(&R->tab[T_DROP], h, t, i)) != NONE) { dropped = 1; R->hit[T_DROP][id] = 1; }
            if (R->path[T_KEEP] && (id = find(&R->tab[T_KEEP], h, t, i)) != NONE) { kept = 1; R->hit[T_KEEP][id] = 1; }
            if (R->path[T_OLD] && (id = find(&R->tab[T_OLD], h, t, i)) != NONE) { ren = id; ren_len = i; R->hit[T_OLD][id] = 1; }   /* the longest comes last */
        }
        if (i < n) { h ^= (uint8_t)t[i]; h *= 1099511628211ull; }
    }
    *text = t; *text_n = n;
    if (dropped || (R->path[T_KEEP] && !kept)) return LE_DROP;                 /* selection sees the original text; drop beats keep */
    int act = LE_KEEP;
    if (ren != NONE) {                                                         /* once, no chaining: new + what followed old */
        const strtab *N = &R->tab[T_NEW];
        const uint32_t ni = R->new_of[ren];
        const size_t need = (size_t)N->len[ni] + (n - ren_len);
        if (need + 1 > R->buf_cap) {
            char *b = (char *)realloc(R->buf, need * 2 + 64);
            if (!b) return -1;
            R->buf = b; R->buf_cap = need * 2 + 64;
        }
        memcpy(R->buf, N->blob + N->off[ni], N->len[ni]);
        memcpy(R->buf + N->len[ni], t + ren_len, n - ren_len);
        *text = R->buf; *text_n = need;
        act |= LE_RENAME;
    }
    if (R->ranks) {                                                            /* cut before the ranks-th ';', if there is one */
        uint32_t semis = 0;
        for (size_t i = 0; i < *text_n; ++i)
            if ((*text)[i] == ';' && ++semis == R->ranks) { *text_n = i; act |= LE_CUT; break; }
    }
    return act;
}

uint64_t le_unmatched(const le_rules *R) {
    uint64_t c = 0;
    for (uint64_t i = 0; i < R->n_lines; ++i) c += !R->hit[R->lines[i].tab][R->lines[i].id];
    return c;
}

void le_each_unmatched(const le_rules *R, le_unmatched_fn fn, void *ctx) {
    for (uint64_t i = 0; i < R->n_lines; ++i) {
        const rule_line *l = &R->lines[i];
        if (R->hit[l->tab][l->id]) continue;
        const strtab *t = &R->tab[l->tab];
        fn(ctx, R->path[l->tab], l->line, t->blob + t->off[l->id], t->len[l->id]);
    }
}
