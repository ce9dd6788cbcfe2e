/* strtab.h -- interning of byte strings (ptr, len) -> dense ids, strings kept NUL-terminated in one blob; and the label "universe" the
 * device folds over (build_fold.hpp): every label text and every cut of it before a ';' (what xeTreeU_RF can turn it into,
 * itree.c:286-301).  Shared by build.c and merge.c.  Private. */
#ifndef UTREE_STRTAB_H
#define UTREE_STRTAB_H
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { char *blob; uint64_t blob_n, blob_cap; uint64_t *off; uint32_t *len; uint32_t n, cap; uint32_t *slot; uint32_t nslot; } strtab;
static inline uint64_t hbytes(const char *s, size_t n) { uint64_t h = 1469598103934665603ull; for (size_t i = 0; i < n; ++i) { h ^= (uint8_t)s[i]; h *= 1099511628211ull; } return h; }
static inline int st_rehash(strtab *t) {
    uint32_t ns = t->nslot ? t->nslot * 2 : 4096;
    uint32_t *sl = (uint32_t *)malloc(sizeof(uint32_t) * ns);
    if (!sl) return -1;
    memset(sl, 0xFF, sizeof(uint32_t) * ns);
    for (uint32_t i = 0; i < t->n; ++i) {
        uint64_t h = hbytes(t->blob + t->off[i], t->len[i]) & (ns - 1);
        while (sl[h] != 0xFFFFFFFFu) h = (h + 1) & (ns - 1);
        sl[h] = i;
    }
    free(t->slot); t->slot = sl; t->nslot = ns;
    return 0;
}
/* id of s[0..n); *fresh = 1 when it was added now.  0xFFFFFFFF on allocation failure. */
static inline uint32_t st_intern(strtab *t, const char *s, size_t n, int *fresh) {
    if ((uint64_t)t->n * 2 >= t->nslot && st_rehash(t)) return 0xFFFFFFFFu;
    uint64_t h = hbytes(s, n) & (t->nslot - 1);
    while (t->slot[h] != 0xFFFFFFFFu) {
        uint32_t i = t->slot[h];
        if (t->len[i] == n && !memcmp(t->blob + t->off[i], s, n)) { *fresh = 0; return i; }
        h = (h + 1) & (t->nslot - 1);
    }
    if (t->n == t->cap) {
        uint32_t nc = t->cap ? t->cap * 2 : 1024;
        uint64_t *o = (uint64_t *)realloc(t->off, sizeof(uint64_t) * nc);
        uint32_t *l = (uint32_t *)realloc(t->len, sizeof(uint32_t) * nc);
        if (o) t->off = o;
        if (l) t->len = l;
        if (!o || !l) return 0xFFFFFFFFu;
        t->cap = nc;
    }
    if (t->blob_n + n + 1 > t->blob_cap) {
        uint64_t nc = t->blob_cap ? t->blob_cap * 2 : (1u << 16);
        while (nc < t->blob_n + n + 1) nc *= 2;
        char *b = (char *)realloc(t->blob, nc);
        if (!b) return 0xFFFFFFFFu;
        t->blob = b; t->blob_cap = nc;
    }
    memcpy(t->blob + t->blob_n, s, n); t->blob[t->blob_n + n] = 0;
    t->off[t->n] = t->blob_n; t->len[t->n] = (uint32_t)n;
    t->blob_n += n + 1;
    t->slot[h] = t->n;
    *fresh = 1;
    return t->n++;
}
static inline void st_free(strtab *t) { free(t->blob); free(t->off); free(t->len); free(t->slot); }

/* the universe: a strtab plus, per id u, the ids of its cuts -- trunc_ids[trunc_off[u] + m - 1] = u cut before its m-th ';' */
typedef struct { strtab U; uint32_t *trunc_off, *trunc_ids; uint32_t n_trunc, trunc_cap; } label_universe;

/* id of lab[0..ll) with all its cuts present; 0xFFFFFFFF on allocation failure */
static inline uint32_t universe_add(label_universe *L, const char *lab, size_t ll) {
    int fresh;
    uint32_t u = st_intern(&L->U, lab, ll, &fresh);
    if (u == 0xFFFFFFFFu || !fresh) return u;
    uint32_t semis = 0;
    for (size_t q = 0; q < ll; ++q) semis += lab[q] == ';';
    if (L->U.n + semis + 8 > L->trunc_cap || L->n_trunc + semis + 8 > L->trunc_cap) {
        uint32_t nc = L->trunc_cap ? L->trunc_cap * 2 : 4096;
        while (nc < L->U.n + semis + 8 || nc < L->n_trunc + semis + 8) nc *= 2;
        uint32_t *a = (uint32_t *)realloc(L->trunc_off, sizeof(uint32_t) * nc), *b = (uint32_t *)realloc(L->trunc_ids, sizeof(uint32_t) * nc);
        if (a) L->trunc_off = a;
        if (b) L->trunc_ids = b;
        if (!a || !b) return 0xFFFFFFFFu;
        L->trunc_cap = nc;
    }
    const uint32_t list = L->n_trunc;
    L->trunc_off[u] = list;
    for (size_t q = 0; q < ll; ++q) if (lab[q] == ';') {
        int f2;
        uint32_t c = st_intern(&L->U, lab, q, &f2);
        if (c == 0xFFFFFFFFu) return 0xFFFFFFFFu;
        if (f2) L->trunc_off[c] = list;                                     /* its own cuts are the first m entries of this list */
        L->trunc_ids[L->n_trunc++] = c;
    }
    return u;
}
/* after the last universe_add: trunc_off[n] closes the table; nonzero on allocation failure */
static inline int universe_close(label_universe *L) {
    if (L->U.n + 1 > L->trunc_cap) {
        uint32_t *a = (uint32_t *)realloc(L->trunc_off, sizeof(uint32_t) * (L->U.n + 8));
        if (!a) return -1;
        L->trunc_off = a;
    }
    L->trunc_off[L->U.n] = L->n_trunc;
    return 0;
}
static inline void universe_free(label_universe *L) { st_free(&L->U); free(L->trunc_off); free(L->trunc_ids); }

#endif
