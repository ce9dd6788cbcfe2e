/* merge.c -- host side of utree_merge_files (`utree-merge`, `utree-mergeGG`): the inputs' layouts (`.ubt` or `.ctr`, told apart by
 * structure), their label lines, the label universe the device folds over, the plan of passes over contiguous ranges of words, the
 * numbering of labels in the order the imagined build creates them, and the `.ubt` written (UT_writeTreeBinary, itree.c:1317-1343).
 * The node work is in merge_kernels.hip; include/utree_amd.h states what a merge is.  utree_merge_files_edit is the same call with an edit:
 * each label line goes through label_edit.c on its way into the universe, MINUS inputs are further slices of every pass, and
 * utree_merge_edit_preview shows what the label edit would do without a device.  The input reader, the pass plan and the slice layout are
 * shared with compare.c (merge_input.h).
 */
#define _FILE_OFFSET_BITS 64
#define _GNU_SOURCE
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include "utree_internal.h"
#include "dev_image.h"
#include "merge_input.h"

#define NPREFIX (1u << 24)
#define fail_text utree_merge_fail_text          /* shared with compare.c (merge_input.h) */

int utree_merge_fail_text(int rc, const char *fmt, const char *path, const char *more) {
    char msg[512];
    snprintf(msg, sizeof msg, fmt, path, more);
    utree_set_error_text(msg);
    return rc;
}

/* the tail at `off`: complete `text \t decimal \n` lines whose counts sum to n */
static int tail_ok(const uint8_t *m, uint64_t size, uint64_t off, uint64_t n) {
    if (off > size) return 0;
    uint64_t sum = 0, p = off;
    while (p < size) {
        const uint8_t *nl = (const uint8_t *)memchr(m + p, '\n', size - p);
        if (!nl) return 0;
        const uint8_t *tab = (const uint8_t *)memchr(m + p, '\t', (size_t)(nl - (m + p)));
        if (!tab || tab == m + p || tab + 1 == nl) return 0;
        uint64_t v = 0;
        for (const uint8_t *d = tab + 1; d < nl; ++d) {
            if (*d < '0' || *d > '9' || v > (1ull << 60)) return 0;
            v = v * 10 + (uint64_t)(*d - '0');
        }
        sum += v;
        if (sum > n) return 0;
        p = (uint64_t)(nl - m) + 1;
    }
    return sum == n;
}

void utree_merge_input_close(merge_in *in) {
    if (in->map && in->map != MAP_FAILED) munmap((void *)in->map, in->size ? in->size : 1);
    if (in->fd >= 0) close(in->fd);
    free(in->bins); free(in->u_of_ix);
}

int utree_merge_input_open(merge_in *in, const char *path, label_universe *L, le_rules *R, utree_merge_edit_stats *es, int minus, FILE *tsv) {
    in->path = path;
    in->fd = open(path, O_RDONLY);
    if (in->fd < 0) return fail_text(UTREE_E_IO, "%s: cannot open%s", path, "");
    struct stat sb;
    if (fstat(in->fd, &sb) || !S_ISREG(sb.st_mode)) return fail_text(UTREE_E_IO, "%s: not a readable file%s", path, "");
    in->size = (uint64_t)sb.st_size;
    if (in->size < 32) return fail_text(UTREE_E_FORMAT, "%s: shorter than a header%s", path, "");
    in->map = (const uint8_t *)mmap(NULL, in->size, PROT_READ, MAP_PRIVATE, in->fd, 0);
    if (in->map == MAP_FAILED) { in->map = NULL; return fail_text(UTREE_E_IO, "%s: cannot map%s", path, ""); }
    uint64_t md[4];
    memcpy(md, in->map, 32);
    if (md[1] != 0 || (md[2] != 2 && md[2] != 4) || md[0] > 64) return fail_text(UTREE_E_FORMAT, "%s: not a .ubt / .ctr header%s", path, "");
    if (md[0] != 4 && md[0] != 8 && md[0] != 16) return fail_text(UTREE_E_UNSUPPORTED, "%s: word size is not 4, 8 or 16 bytes%s", path, "");
    in->W = (uint32_t)md[0]; in->I = (uint32_t)md[2]; in->n = md[3];
    if (in->n > in->size) return fail_text(UTREE_E_FORMAT, "%s: more nodes than bytes%s", path, "");
    /* exactly one layout must have a tail that starts inside the file, is made of complete lines, and counts n nodes */
    const uint64_t ubt_tail = 32 + in->n * (in->W + in->I);
    in->binw = in->n < 0xFFFFFFFFull ? 4 : 8;                                          /* itree.c:1301-1306 */
    const uint64_t ctr_rec = 32 + (uint64_t)UTREE_NUMBINS * in->binw, ctr_tail = ctr_rec + in->n * (in->W + in->I - 3);
    const int as_ubt = tail_ok(in->map, in->size, ubt_tail, in->n), as_ctr = tail_ok(in->map, in->size, ctr_tail, in->n);
    if (as_ubt == as_ctr) return fail_text(UTREE_E_FORMAT, "%s: %s", path, as_ubt ? "reads as a .ubt and as a .ctr" : "neither a .ubt nor a .ctr: no layout ends in label lines that count its nodes");
    in->is_ctr = as_ctr;
    in->rec = in->is_ctr ? in->W + in->I - 3 : in->W + in->I;
    in->rec_off = in->is_ctr ? ctr_rec : 32;
    in->tail_off = in->is_ctr ? ctr_tail : ubt_tail;
    if (in->is_ctr) {
        in->bins = (uint64_t *)malloc(8ull * UTREE_NUMBINS);
        if (!in->bins) return UTREE_E_NOMEM;
        const uint8_t *b = in->map + 32;
        int mono = 1;
        for (uint32_t p = 0; p < UTREE_NUMBINS; ++p) {
            uint64_t v;
            if (in->binw == 4) { uint32_t t; memcpy(&t, b + 4ull * p, 4); v = t; } else memcpy(&v, b + 8ull * p, 8);
            in->bins[p] = v;
            if (p && v < in->bins[p - 1]) mono = 0;
        }
        if (!mono || in->bins[0] != 0 || in->bins[NPREFIX] != in->n)
            return fail_text(UTREE_E_UNSUPPORTED, "%s: a .ctr whose bin table is not non-decreasing from 0 to its node count: its words cannot be reconstructed%s", path, "");
    }
    /* label lines as the loader reads them (itree.c:191-220): a text's index is that of its first line */
    if (!minus) {
        strtab own; memset(&own, 0, sizeof own);
        uint32_t cap = 0;
        uint64_t p = in->tail_off;
        int rc = UTREE_OK;
        while (p < in->size && !rc) {
            const uint8_t *nl = (const uint8_t *)memchr(in->map + p, '\n', in->size - p);
            const uint8_t *tab = (const uint8_t *)memchr(in->map + p, '\t', (size_t)(nl - (in->map + p)));
            int fresh;
            const size_t ll = (size_t)(tab - (in->map + p));
            uint32_t d = st_intern(&own, (const char *)in->map + p, ll, &fresh);
            if (d == 0xFFFFFFFFu) { rc = UTREE_E_NOMEM; break; }
            if (fresh) {
                if (d >= cap) {
                    cap = cap ? cap * 2 : 1024;
                    uint32_t *a = (uint32_t *)realloc(in->u_of_ix, 4ull * cap);
                    if (!a) { rc = UTREE_E_NOMEM; break; }
                    in->u_of_ix = a;
                }
                const char *text = (const char *)in->map + p;
                size_t tn = ll;
                const int act = R ? le_apply(R, text, ll, &text, &tn) : LE_KEEP;
                if (act < 0) { rc = UTREE_E_NOMEM; break; }
                if (es) { ++es->n_label_lines; es->n_labels_dropped += act == LE_DROP; es->n_labels_renamed += act != LE_DROP && (act & LE_RENAME); es->n_labels_cut += act != LE_DROP && (act & LE_CUT); }
                uint32_t u = UTK_MERGE_DROP;
                if (act != LE_DROP) {
                    if (!tn) {                                                 /* the builder refuses blank labels */
                        char name[300];
                        snprintf(name, sizeof name, "%.*s", (int)(ll < 280 ? ll : 280), (const char *)in->map + p);
                        rc = fail_text(UTREE_E_FORMAT, "%s: the edit leaves label `%s` empty", path, name);
                        break;
                    }
                    u = universe_add(L, text, tn);
                    if (u == 0xFFFFFFFFu) { rc = UTREE_E_NOMEM; break; }
                    if (L->U.n >= (1u << 24)) rc = fail_text(UTREE_E_UNSUPPORTED, "%s: labels and their ';'-prefixes reach 2^24%s", path, "");
                }
                if (tsv) {
                    static const char *const names[4] = {"keep", "rename", "cut", "rename+cut"};
                    fwrite(in->map + p, 1, ll, tsv); fputc('\t', tsv);
                    fwrite(tab + 1, 1, (size_t)(nl - tab - 1), tsv);
                    fprintf(tsv, "\t%s\t", act == LE_DROP ? "drop" : names[act & 3]);
                    if (act != LE_DROP) fwrite(text, 1, tn, tsv);
                    fputc('\n', tsv);
                    if (act == LE_DROP && es) es->n_nodes_dropped += strtoull((const char *)tab + 1, NULL, 10);
                }
                in->u_of_ix[d] = u;
                in->n_lines = d + 1;
            }
            p = (uint64_t)(nl - in->map) + 1;
        }
        st_free(&own);
        if (rc) return rc;
    }
    return UTREE_OK;
}

int utree_merge_probe(const char *path, utree_merge_input *info) {
    if (!path || !info) return UTREE_E_ARG;
    merge_in in; memset(&in, 0, sizeof in);
    in.fd = -1;
    label_universe L; memset(&L, 0, sizeof L);
    const int rc = utree_merge_input_open(&in, path, &L, NULL, NULL, 0, NULL);
    memset(info, 0, sizeof *info);
    if (!rc) { info->W = in.W; info->I = in.I; info->is_ctr = (uint32_t)in.is_ctr; info->n_nodes = in.n; info->n_labels = in.n_lines; }
    utree_merge_input_close(&in);
    universe_free(&L);
    return rc;
}

static void rec_word(const merge_in *in, uint64_t node, uint64_t *hi, uint64_t *lo) {      /* .ubt only */
    const uint8_t *r = in->map + in->rec_off + node * in->rec;
    *hi = 0; *lo = 0;
    memcpy(lo, r, in->W == 4 ? 4 : 8);
    if (in->W == 16) memcpy(hi, r + 8, 8);
}

/* nodes of the input whose word's top 24 bits are below P (P <= 2^24) */
static uint64_t count_below(const merge_in *in, uint32_t P) {
    if (P >= NPREFIX) return in->n;
    if (in->is_ctr) return in->bins[P];
    const uint64_t bound = (uint64_t)P << (in->W == 4 ? 8 : 40);                          /* of lo (W = 4, 8) or hi (W = 16) */
    uint64_t a = 0, b = in->n;
    while (a < b) {
        const uint64_t m = a + ((b - a) >> 1);
        uint64_t hi, lo;
        rec_word(in, m, &hi, &lo);
        if ((in->W == 16 ? hi : lo) < bound) a = m + 1; else b = m;
    }
    return a;
}

static uint64_t total_below(const merge_in *ins, int n_in, uint32_t P) {
    uint64_t t = 0;
    for (int i = 0; i < n_in; ++i) t += count_below(&ins[i], P);
    return t;
}

int utree_merge_plan(const merge_in *ins, int n_all, uint64_t n_read, uint64_t limit, const char *name, uint32_t **bounds_out, uint32_t *n_pass_out,
                     uint64_t *cap_nodes_out, uint64_t *cap_raw_out) {
    uint32_t *bounds = NULL, n_pass = 0, bounds_cap = 0;
    uint64_t cap_nodes = 0, cap_raw = 0, want = limit;
    const char *e = getenv("UTREE_TEST_MERGE_PASS_NODES");                                /* test hook: small inputs in many passes */
    if (e && atoll(e) > 0 && (uint64_t)atoll(e) < want) want = (uint64_t)atoll(e);
    uint32_t P0 = 0;
    uint64_t below0 = 0;
    while (below0 < n_read) {
        uint32_t a = P0 + 1, b = NPREFIX;                                                 /* the largest P1 in [a, b] with at most `want` nodes in [P0, P1); a itself if none */
        if (total_below(ins, n_all, b) - below0 <= want) a = b;
        else while (a < b) {
            const uint32_t m = a + ((b - a + 1) >> 1);
            if (total_below(ins, n_all, m) - below0 <= want) a = m; else b = m - 1;
        }
        if (total_below(ins, n_all, a) == below0) ++a;                                     /* nothing below the prefix that alone exceeds `want`: no empty pass, take that prefix */
        const uint64_t below1 = total_below(ins, n_all, a);
        if (below1 - below0 > limit) { free(bounds); return fail_text(UTREE_E_NOMEM, "%s: the nodes that share one 24-bit prefix do not fit the device's free memory%s", name, ""); }
        if (n_pass + 2 > bounds_cap) {
            bounds_cap = bounds_cap ? bounds_cap * 2 : 64;
            uint32_t *nb = (uint32_t *)realloc(bounds, 4ull * bounds_cap);
            if (!nb) { free(bounds); return UTREE_E_NOMEM; }
            bounds = nb;
        }
        if (!n_pass) bounds[0] = 0;
        bounds[++n_pass] = a;
        if (below1 - below0 > cap_nodes) cap_nodes = below1 - below0;
        uint64_t raw = 0;
        for (int i = 0; i < n_all; ++i) raw += ((count_below(&ins[i], a) - count_below(&ins[i], P0)) * ins[i].rec + 255) & ~255ull;
        if (raw > cap_raw) cap_raw = raw;
        P0 = a; below0 = below1;
    }
    *bounds_out = bounds; *n_pass_out = n_pass; *cap_nodes_out = cap_nodes; *cap_raw_out = cap_raw;
    return UTREE_OK;
}

void utree_merge_slices(const merge_in *ins, int n_all, int n_minus, const uint32_t *bounds, uint32_t p, utk_merge_slice *sl) {
    uint64_t raw_off = 0;
    for (int i = 0; i < n_all; ++i) {
        const merge_in *in = &ins[i];
        utk_merge_slice *s = &sl[i];
        memset(s, 0, sizeof *s);
        const uint64_t first = count_below(in, bounds[p]), end = count_below(in, bounds[p + 1]);
        s->input = (uint32_t)i; s->is_ctr = (uint32_t)in->is_ctr; s->I = in->I; s->minus = i < n_minus;
        s->n = end - first; s->raw_off = raw_off; s->g0 = in->g0 + first; s->first = first;
        s->fd = in->fd; s->file_off = in->rec_off + first * in->rec;
        if (!s->n) continue;
        raw_off += (s->n * in->rec + 255) & ~255ull;
        if (in->is_ctr) {
            s->p_lo = bounds[p]; s->n_bins = bounds[p + 1] - bounds[p]; s->h_bins = in->bins + bounds[p];
            if (first) {                                                                   /* the node in front lies in the last non-empty bin below */
                uint32_t q = bounds[p];
                while (q && in->bins[q] >= first) --q;                                     /* bins[q] < first <= bins[q + 1] */
                const uint8_t *r = in->map + in->rec_off + (first - 1) * in->rec;
                uint64_t suf_lo = 0, suf_hi = 0;
                memcpy(&suf_lo, r, in->W == 16 ? 8 : in->W - 3);
                if (in->W == 16) memcpy(&suf_hi, r + 8, 5);
                s->has_prev = 1;
                if (in->W == 4) s->prev_lo = ((uint64_t)q << 8) | suf_lo;
                else if (in->W == 8) s->prev_lo = ((uint64_t)q << 40) | suf_lo;
                else { s->prev_lo = suf_lo; s->prev_hi = ((uint64_t)q << 40) | suf_hi; }
            }
        } else if (first) { s->has_prev = 1; rec_word(in, first - 1, &s->prev_hi, &s->prev_lo); }
    }
}

typedef struct { uint64_t time; uint32_t u; } event;
static int by_time(const void *a, const void *b) {
    const event *x = (const event *)a, *y = (const event *)b;
    return x->time < y->time ? -1 : x->time > y->time;
}

static int write_all(int fd, const void *p, size_t n) {
    const char *c = (const char *)p;
    while (n) { ssize_t w = write(fd, c, n); if (w <= 0) return -1; c += w; n -= (size_t)w; }
    return 0;
}

static int edit_args_bad(const utree_merge_edit *e) {
    if (e->size != sizeof(utree_merge_edit) || e->ranks > 255 || e->n_minus < 0 || (e->n_minus > 0 && !e->minus_paths)) return 1;
    for (int i = 0; i < e->n_minus; ++i) if (!e->minus_paths[i]) return 1;
    return 0;
}

static int load_rules(const utree_merge_edit *e, le_rules **R) {
    char msg[512];
    msg[0] = 0;
    const int rc = le_load(R, e->ranks, e->drop_path, e->keep_path, e->rename_path, msg, sizeof msg);
    if (rc && msg[0]) utree_set_error_text(msg);
    return rc;
}

static void preview_unmatched(void *ctx, const char *file, uint64_t line, const char *text, size_t text_n) {
    FILE *out = (FILE *)ctx;
    fprintf(out, "# unmatched\t%s\t%llu\t", file, (unsigned long long)line);
    fwrite(text, 1, text_n, out);
    fputc('\n', out);
}

int utree_merge_edit_preview(const char *const *in_paths, int n_in, const utree_merge_edit *edit, const char *tsv_path, utree_merge_edit_stats *stats) {
    if (!in_paths || n_in < 1 || !edit || !tsv_path || edit_args_bad(edit)) return UTREE_E_ARG;
    for (int i = 0; i < n_in; ++i) if (!in_paths[i]) return UTREE_E_ARG;
    utree_merge_edit_stats es; memset(&es, 0, sizeof es);
    le_rules *R = NULL;
    label_universe L; memset(&L, 0, sizeof L);
    FILE *out = NULL;
    int rc = load_rules(edit, &R);
    if (!rc && !(out = fopen(tsv_path, "wb"))) rc = fail_text(UTREE_E_IO, "%s: cannot create%s", tsv_path, "");
    for (int i = 0; i < n_in && !rc; ++i) {
        merge_in in; memset(&in, 0, sizeof in);
        in.fd = -1;
        char *lines = NULL; size_t lines_n = 0;
        FILE *mem = open_memstream(&lines, &lines_n);                                      /* the input's line comes first and states how many follow */
        if (!mem) rc = UTREE_E_NOMEM;
        else {
            rc = utree_merge_input_open(&in, in_paths[i], &L, R, &es, 0, mem);
            if (fclose(mem) && !rc) rc = UTREE_E_NOMEM;
        }
        if (!rc) {
            fprintf(out, "# input\t%s\t%s\t%llu\t%u\n", in_paths[i], in.is_ctr ? ".ctr" : ".ubt", (unsigned long long)in.n, in.n_lines);
            fwrite(lines, 1, lines_n, out);
        }
        free(lines);
        utree_merge_input_close(&in);
    }
    if (!rc) {
        es.n_rules_unmatched = le_unmatched(R);
        le_each_unmatched(R, preview_unmatched, out);
    }
    if (out) {
        const int bad = ferror(out);
        if ((fclose(out) || bad) && !rc) rc = fail_text(UTREE_E_IO, "%s: cannot write%s", tsv_path, "");
        if (rc) unlink(tsv_path);                                                          /* a failed call leaves no file behind */
    }
    le_free(R);
    universe_free(&L);
    if (stats) *stats = es;
    return rc;
}

int utree_merge_files(const char *const *in_paths, int n_in, const char *ubt_path, uint32_t I, int gg, int device, utree_merge_stats *stats) {
    return utree_merge_files_edit(in_paths, n_in, ubt_path, I, gg, device, NULL, stats, NULL);
}

int utree_merge_files_edit(const char *const *in_paths, int n_in, const char *ubt_path, uint32_t I, int gg, int device,
                           const utree_merge_edit *edit, utree_merge_stats *stats, utree_merge_edit_stats *edit_stats) {
    if (!in_paths || n_in < 1 || !ubt_path || (I != 0 && I != 2 && I != 4)) return UTREE_E_ARG;
    for (int i = 0; i < n_in; ++i) if (!in_paths[i]) return UTREE_E_ARG;
    if (edit && edit_args_bad(edit)) return UTREE_E_ARG;
    const int n_minus = edit ? edit->n_minus : 0, n_all = n_in + n_minus;                   /* ins[]: the MINUS inputs, then the regular ones */
    utree_merge_stats st; memset(&st, 0, sizeof st);
    utree_merge_edit_stats es; memset(&es, 0, sizeof es);
    st.n_inputs = (uint32_t)n_in;
    const double t0 = now_s();
    int rc = UTREE_OK, fd = -1, created = 0;
    merge_in *ins = (merge_in *)calloc((size_t)n_all, sizeof(merge_in));
    le_rules *R = NULL;
    label_universe L; memset(&L, 0, sizeof L);
    uint32_t *bounds = NULL, n_pass = 0, *ix_of_u = NULL, *u_of_ix = NULL, n_labels = 0;
    uint32_t **maps = NULL, *n_lines = NULL;
    uint64_t *first_time = NULL, *per_label = NULL;
    utk_merge_slice *sl = NULL;
    event *ev = NULL;
    utk_merge_dev *D = NULL;
    char *txt = NULL;
    if (!ins) return UTREE_E_NOMEM;
    for (int i = 0; i < n_all; ++i) ins[i].fd = -1;
    if (edit) { rc = load_rules(edit, &R); if (rc) goto done; }
    /* ---- the inputs: the regular ones first, so that a MINUS input of another word size is the one refused ---- */
    uint32_t W = 0, I_out = I, rec_max = 0;
    int any_ctr = 0;
    for (int o = 0; o < n_all; ++o) {
        const int minus = o >= n_in, i = minus ? o - n_in : n_minus + o;
        const char *path = minus ? edit->minus_paths[o - n_in] : in_paths[o];
        rc = utree_merge_input_open(&ins[i], path, &L, R, edit ? &es : NULL, minus, NULL);
        if (rc) goto done;
        if (o && ins[i].W != W) { rc = fail_text(UTREE_E_UNSUPPORTED, "%s: its word size differs from the first input's%s", path, ""); goto done; }
        W = ins[i].W;
        if (ins[i].rec > rec_max) rec_max = ins[i].rec;
        any_ctr |= ins[i].is_ctr;
        if (minus) { es.n_minus_nodes += ins[i].n; continue; }
        if (!I && ins[i].I > I_out) I_out = ins[i].I;
        ins[i].g0 = st.n_in_nodes;
        st.n_in_nodes += ins[i].n;
    }
    st.W = W; st.I = I_out;
    const uint64_t n_read = st.n_in_nodes + es.n_minus_nodes;
    if (n_read >= (1ull << 40)) { rc = fail_text(UTREE_E_UNSUPPORTED, "%s: 2^40 nodes or more in all%s", ubt_path, ""); goto done; }
    if (universe_close(&L)) { rc = UTREE_E_NOMEM; goto done; }
    /* ---- passes: contiguous ranges of the words' top 24 bits, so a run of equal words is never split and a `.ctr`'s slice is a range of bins ---- */
    uint64_t limit = 0, cap_nodes = 0, cap_raw = 0;
    rc = utk_merge_limit(device, W, rec_max, &limit);
    if (rc) goto done;
    rc = utree_merge_plan(ins, n_all, n_read, limit, ubt_path, &bounds, &n_pass, &cap_nodes, &cap_raw);
    if (rc) goto done;
    st.n_passes = n_pass;
    /* ---- device ---- */
    maps = (uint32_t **)calloc((size_t)n_all, sizeof *maps); n_lines = (uint32_t *)calloc((size_t)n_all, 4);
    sl = (utk_merge_slice *)calloc((size_t)n_all, sizeof *sl);
    first_time = (uint64_t *)malloc(8ull * (L.U.n + 1)); ix_of_u = (uint32_t *)malloc(4ull * (L.U.n + 1));
    ev = (event *)malloc(sizeof(event) * (L.U.n + 1ull));
    if (!maps || !n_lines || !sl || !first_time || !ix_of_u || !ev) { rc = UTREE_E_NOMEM; goto done; }
    for (int i = 0; i < n_all; ++i) { maps[i] = ins[i].u_of_ix; n_lines[i] = ins[i].n_lines; }
    {
        utk_merge_cfg cfg = {L.U.blob, L.U.blob_n, L.U.off, L.U.n, L.trunc_off, L.trunc_ids, L.n_trunc, (uint32_t)n_all,
                             (const uint32_t *const *)maps, n_lines, W, I_out, gg, device, any_ctr, n_minus > 0, cap_nodes, cap_raw, 0};
        rc = utk_merge_open(&cfg, &D);
        if (rc) goto done;
    }
    /* One pass: its nodes stay on the device while the labels are numbered.  Several: the label numbers depend on every pass's events, so a
     * first sweep replays all passes for the events alone and a second one replays them again and writes. */
    for (int sweep = 0; sweep < (n_pass > 1 ? 2 : 1); ++sweep) {
        for (uint32_t p = 0; p < n_pass; ++p) {
            utree_merge_slices(ins, n_all, n_minus, bounds, p, sl);        /* MINUS slices in front: the stable sort keeps a MINUS record at the head of its run */
            utk_merge_pass_out po;
            uint32_t io_slice = 0;
            rc = utk_merge_pass(D, sl, (uint32_t)n_all, sweep == 0, &po, &io_slice);
            if (rc == UTREE_E_IO) fail_text(rc, "%s: cannot read its nodes%s", ins[io_slice].path, "");
            if (rc) goto done;
            if (po.err & 2u) { rc = fail_text(UTREE_E_FORMAT, "%s: a node's label index names no label line of its input%s", ubt_path, ""); goto done; }
            if (po.err & 1u) { rc = fail_text(UTREE_E_FORMAT, "%s: the words of a .ubt input are not strictly ascending%s", ubt_path, ""); goto done; }
            if (po.err & 4u) { rc = fail_text(UTREE_E_UNSUPPORTED, "%s: a .ctr input whose words, rebuilt from its bins, are not strictly ascending (xtree-compress's first-bin quirk does that when the first prefix holds one node): its words cannot be reconstructed%s", ubt_path, ""); goto done; }
            if (sweep == 0) { st.n_nodes += po.n_nodes; st.n_shared += po.n_shared; st.n_relabelled += po.n_relabelled; st.n_dropped += po.n_dropped; es.n_nodes_dropped += po.n_label_dropped; es.n_nodes_subtracted += po.n_subtracted; }
            if (n_pass > 1 && sweep == 0) continue;
            if (fd < 0) {
                /* ---- label indices in the imagined build's order of creation (addSampleU, itree.c:593; addSampleUd, 299) ---- */
                uint64_t nev = 0;
                rc = utk_merge_events(D, first_time);
                if (rc) goto done;
                for (uint32_t u = 0; u < L.U.n; ++u) if (first_time[u] != ~0ull) { ev[nev].time = first_time[u]; ev[nev].u = u; ++nev; }
                qsort(ev, nev, sizeof(event), by_time);
                memset(ix_of_u, 0xFF, 4ull * (L.U.n + 1));
                for (uint64_t i = 0; i < nev; ++i) ix_of_u[ev[i].u] = n_labels++;
                st.n_labels = n_labels;
                if (I_out == 2 && n_labels > 65534) {
                    rc = fail_text(UTREE_E_UNSUPPORTED, "%s: more than 65534 labels do not fit a 2-byte index (65534 and 65535 are EMPTY_IX and BAD_IX): ask for the 4-byte index (I = 4, UTREE_IXTYPE=32)%s", ubt_path, "");
                    goto done;
                }
                rc = utk_merge_set_ix(D, ix_of_u, n_labels);
                if (rc) goto done;
                fd = open(ubt_path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
                if (fd < 0) { rc = fail_text(UTREE_E_IO, "%s: cannot create%s", ubt_path, ""); goto done; }
                created = 1;
                uint64_t md[4] = {W, 0, I_out, st.n_nodes};
                if (write_all(fd, md, 32)) { rc = fail_text(UTREE_E_IO, "%s: cannot write%s", ubt_path, ""); goto done; }
            }
            rc = utk_merge_emit(D, fd);
            if (rc) { if (rc == UTREE_E_IO) fail_text(rc, "%s: cannot write%s", ubt_path, ""); goto done; }
        }
    }
    if (fd < 0) {                                                                          /* inputs without a node: the header alone */
        fd = open(ubt_path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (fd < 0) { rc = fail_text(UTREE_E_IO, "%s: cannot create%s", ubt_path, ""); goto done; }
        created = 1;
        uint64_t md[4] = {W, 0, I_out, 0};
        if (write_all(fd, md, 32)) { rc = fail_text(UTREE_E_IO, "%s: cannot write%s", ubt_path, ""); goto done; }
    }
    /* ---- label lines in index order: text \t nodes carrying it ---- */
    {
        per_label = (uint64_t *)calloc(n_labels ? n_labels : 1, 8);
        u_of_ix = (uint32_t *)malloc(4ull * (n_labels ? n_labels : 1));
        txt = (char *)malloc((size_t)L.U.blob_n + 32ull * n_labels + 64);
        if (!per_label || !u_of_ix || !txt) { rc = UTREE_E_NOMEM; goto done; }
        if (n_labels) { rc = utk_merge_counts(D, per_label); if (rc) goto done; }
        for (uint32_t u = 0; u < L.U.n; ++u) if (ix_of_u[u] != 0xFFFFFFFFu) u_of_ix[ix_of_u[u]] = u;
        size_t o = 0;
        for (uint32_t i = 0; i < n_labels; ++i) {
            const uint32_t u = u_of_ix[i];
            memcpy(txt + o, L.U.blob + L.U.off[u], L.U.len[u]); o += L.U.len[u];
            o += (size_t)sprintf(txt + o, "\t%llu\n", (unsigned long long)per_label[i]);
        }
        if (write_all(fd, txt, o)) { rc = fail_text(UTREE_E_IO, "%s: cannot write%s", ubt_path, ""); goto done; }
    }
    if (close(fd)) { fd = -1; rc = fail_text(UTREE_E_IO, "%s: cannot write%s", ubt_path, ""); goto done; }
    fd = -1;
done:
    if (fd >= 0) close(fd);
    if (rc && created) unlink(ubt_path);                                                   /* a failed call leaves no output file behind */
    if (D) utk_merge_close(D);
    if (ins) { for (int i = 0; i < n_all; ++i) utree_merge_input_close(&ins[i]); free(ins); }
    if (R) es.n_rules_unmatched = le_unmatched(R);
    le_free(R);
    universe_free(&L);
    free(bounds); free(ix_of_u); free(u_of_ix); free(maps); free(n_lines); free(first_time); free(per_label); free(sl); free(ev); free(txt);
    st.seconds = now_s() - t0;
    if (stats) *stats = st;
    if (edit_stats) *edit_stats = es;
    return rc;
}
