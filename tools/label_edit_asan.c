/* label_edit_asan.c -- the rule-file parser and the label edit of utree_merge_files_edit (utree_amd/csrc/label_edit.c) as a stand-alone
 * host program for AddressSanitizer + UndefinedBehaviorSanitizer: `make -C utree_amd/csrc label-edit-asan`.  It writes hostile rule files
 * into a temporary directory, loads them, edits a list of labels and checks what comes back.  No GPU, no Python.  Exit code 0: all as
 * expected and no sanitizer report. */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "../include/utree_amd.h"
#include "../utree_amd/csrc/label_edit.h"

static int failures;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static char dir[64];
static const char *put(const char *name, const char *data, size_t n) {
    static char paths[8][128];
    static int turn;
    char *p = paths[turn++ & 7];
    snprintf(p, 128, "%s/%s", dir, name);
    FILE *f = fopen(p, "wb");
    if (!f || fwrite(data, 1, n, f) != n || fclose(f)) { perror(p); exit(1); }
    return p;
}
#define PUT(name, lit) put(name, lit, sizeof(lit) - 1)

static int load_code(const char *drop, const char *keep, const char *ren, char *msg) {
    le_rules *R = NULL;
    msg[0] = 0;
    const int rc = le_load(&R, 0, drop, keep, ren, msg, 256);
    if (!rc) le_free(R);
    return rc;
}

/* the edit of `t` under R: "<action>:<text>" into out */
static void edit(le_rules *R, const char *t, size_t n, char *out) {
    const char *text; size_t tn;
    const int act = le_apply(R, t, n, &text, &tn);
    if (act == LE_DROP) { strcpy(out, "drop:"); return; }
    const int at = sprintf(out, "%d:", act);
    memcpy(out + at, text, tn);                                                                /* a text may hold a NUL */
    out[at + tn] = 0;
}

static void count_unmatched(void *ctx, const char *file, uint64_t line, const char *text, size_t n) {
    (void)file; (void)text; (void)n;
    *(uint64_t *)ctx += line;
}

int main(void) {
    char msg[256], out[4096];
    strcpy(dir, "/tmp/label_edit_asan.XXXXXX");
    if (!mkdtemp(dir)) { perror("mkdtemp"); return 1; }

    /* malformed files: the code, and the line the text names */
    CHECK(load_code(PUT("d1", "k__A\n\nk__B\tx\n"), NULL, NULL, msg) == UTREE_E_FORMAT && strstr(msg, "line 3") && strstr(msg, "/d1"));
    CHECK(load_code(NULL, PUT("k1", "\tk__A"), NULL, msg) == UTREE_E_FORMAT && strstr(msg, "line 1"));
    CHECK(load_code(NULL, NULL, PUT("r1", "a\tb\r\nno tab\r\n"), msg) == UTREE_E_FORMAT && strstr(msg, "line 2"));
    CHECK(load_code(NULL, NULL, PUT("r2", "a\tb\tc\n"), msg) == UTREE_E_FORMAT && strstr(msg, "line 1"));
    CHECK(load_code(NULL, NULL, PUT("r3", "a\tb\n\tc\n"), msg) == UTREE_E_FORMAT && strstr(msg, "line 2"));
    CHECK(load_code(NULL, NULL, PUT("r4", "a\tb\nc\t\n"), msg) == UTREE_E_FORMAT && strstr(msg, "line 2"));
    CHECK(load_code(NULL, NULL, PUT("r5", "a\tb\n\n\na\tc"), msg) == UTREE_E_FORMAT && strstr(msg, "line 4"));
    CHECK(load_code(NULL, NULL, PUT("r6", "a\t\r\n"), msg) == UTREE_E_FORMAT && strstr(msg, "line 1"));
    CHECK(load_code("/nonexistent/rules", NULL, NULL, msg) == UTREE_E_IO && strstr(msg, "/nonexistent/rules"));
    CHECK(load_code(PUT("e1", ""), PUT("e2", "\n\r\n\n"), PUT("e3", "\r\n"), msg) == UTREE_OK);

    /* CRLF, a last line without '\n', spaces, bytes 0x80-0xFF and a NUL inside a taxon */
    le_rules *R = NULL;
    CHECK(le_load(&R, 3, PUT("drop", "k__A;p__Gone\r\nk__Never\r\nk__\xFF\x80 x"), PUT("keep", "k__A\nk__\xFF\x80 x\nk__Z\0z\n"),
                  PUT("ren", "k__A;p__B\tk__A;p__Q\nk__A\tk__N\r\nk__A;p__Q\tk__A;p__R\nk__A;p__E\t;"), msg, sizeof msg) == UTREE_OK);
    if (R) {
        edit(R, "k__A;p__B;c__C;o__D", 19, out); CHECK(!strcmp(out, "3:k__A;p__Q;c__C"));      /* the longest old, once, then the cut */
        edit(R, "k__A;p__Bx;c__C", 15, out); CHECK(!strcmp(out, "1:k__N;p__Bx;c__C"));          /* a plain prefix is no clade match */
        edit(R, "k__A;p__Q", 9, out); CHECK(!strcmp(out, "1:k__A;p__R"));
        edit(R, "k__A;p__Gone;c__C", 17, out); CHECK(!strcmp(out, "drop:"));                    /* drop beats keep */
        edit(R, "k__A;p__Gonex", 13, out); CHECK(!strcmp(out, "1:k__N;p__Gonex"));
        edit(R, "k__\xFF\x80 x;p", 10, out); CHECK(!strcmp(out, "drop:"));
        edit(R, "k__B;p__B", 9, out); CHECK(!strcmp(out, "drop:"));                             /* no keep line matches */
        edit(R, "k__Z\0z;a;b;c;d", 14, out); CHECK(!memcmp(out, "2:k__Z\0z;a;b", 12));
        edit(R, "k__A", 4, out); CHECK(!strcmp(out, "1:k__N"));
        edit(R, "k__A;p__E;x;y;z", 15, out); CHECK(!strcmp(out, "3:;;x"));
        edit(R, "", 0, out); CHECK(!strcmp(out, "drop:"));
        edit(R, ";", 1, out); CHECK(!strcmp(out, "drop:"));
        char *big = (char *)malloc(1 << 16);                                                    /* a long label: the rename buffer grows */
        if (big) {
            memcpy(big, "k__A;p__B", 9);
            memset(big + 9, 'x', (1 << 16) - 9);
            const char *text; size_t tn;
            CHECK(le_apply(R, big, 1 << 16, &text, &tn) == LE_RENAME && tn == (1 << 16) && !memcmp(text, "k__N;p__Bxx", 11));
            free(big);
        }
        CHECK(le_unmatched(R) == 1);                                                            /* k__Never */
        uint64_t lines = 0;
        le_each_unmatched(R, count_unmatched, &lines);
        CHECK(lines == 2);
        le_free(R);
    }
    /* no files: the identity, and a rank cut alone */
    R = NULL;
    CHECK(le_load(&R, 0, NULL, NULL, NULL, msg, sizeof msg) == UTREE_OK);
    if (R) { edit(R, "a;b;c", 5, out); CHECK(!strcmp(out, "0:a;b;c")); CHECK(le_unmatched(R) == 0); le_free(R); }
    R = NULL;
    CHECK(le_load(&R, 1, NULL, NULL, NULL, msg, sizeof msg) == UTREE_OK);
    if (R) {
        edit(R, ";x", 2, out); CHECK(!strcmp(out, "2:"));                                       /* empty: the caller refuses it */
        edit(R, "a", 1, out); CHECK(!strcmp(out, "0:a"));
        edit(R, "a;", 2, out); CHECK(!strcmp(out, "2:a"));
        le_free(R);
    }
    char cmd[160];
    snprintf(cmd, sizeof cmd, "rm -rf %s", dir);
    if (system(cmd)) ++failures;
    if (failures) { fprintf(stderr, "label_edit_asan: %d checks failed\n", failures); return 1; }
    puts("label_edit_asan: ok");
    return 0;
}
