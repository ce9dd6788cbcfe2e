/* tiles_format_asan.c -- utree_tiles_format and utree_tiles_segments_format (utree_amd/csrc/tiles.c) under AddressSanitizer +
 * UndefinedBehaviorSanitizer, as a stand-alone host program: no GPU, no Python; the device side of tiles.c is stubbed out.  The hand-made
 * results sit on the formatters' edges -- no hit at a query's first and last tile, two (label, cut) of one text side by side, the empty
 * taxon, uix == 1, the largest numbers the fields hold, a cut beyond the label -- and every cap from 0 to the exact size gets a heap block of
 * exactly that size, so a byte written behind cap is a report; the segments are also formatted tile by tile with the run carried in the
 * state.  `make -C utree_amd/csrc tiles-format-asan`, or from the repository root:
 *
 *     gcc -std=gnu11 -g -O1 -fopenmp -fsanitize=address,undefined -fno-omit-frame-pointer -I/opt/rocm/include tools/tiles_format_asan.c \
 *         utree_amd/csrc/tiles.c utree_amd/csrc/fasta.c utree_amd/csrc/ctr_host.c -lz -o /tmp/tiles_format_asan && /tmp/tiles_format_asan
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../utree_amd/csrc/tiles.h"
/* stubs for what tiles.c links against */
size_t utk_tiles_scan_temp_bytes(uint32_t n) { return 1024; }
int utk_tiles_plan(const uint32_t *l, uint32_t n, uint32_t W, uint32_t S, uint64_t *tf, utree_tiles_meta *m, const utk_tiles_ws *ws, void *st) { return 0; }
int utk_tiles_views(const uint64_t *o, const uint32_t *l, uint32_t n, uint32_t W, uint32_t S, const uint64_t *tf, uint64_t first, uint32_t nt, uint64_t *toff,
                    uint32_t *tlen, uint32_t *tq, uint32_t *ti, utree_tiles_meta *m, void *st) { return 0; }
void utree_dev_set_hip_error(int e, const char *w) {}
hipError_t hipSetDevice(int d) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }

#define NT 11
static const char *names = "firstsecond_queryq3";
static const uint64_t noff[3] = {0, 5, 17};
static const uint32_t nlen[3] = {5, 12, 2}, slen[3] = {95, 10, 61};          /* W = 20, S = 15: 6, 1 and 4 tiles */
static const uint32_t tq[NT] = {0, 0, 0, 0, 0, 0, 1, 2, 2, 2, 2}, ti[NT] = {0, 1, 2, 3, 4, 5, 0, 0, 1, 2, 3};
static const utree_result res[NT] = {
    {0, -2, 0, 0, 0, 0}, {0, -2, 5, 2, 3, 2}, {1, 9, 4294967295u, 3, 4294967295u, 7}, {1, -2, 1, 1, 0, 0}, {0, -1, 2, 2, 1, 1}, {0, -2, 0, 0, 0, 0},
    {2, 100000, 9, 4, 5, 4}, {1, -2, 0, 5, 9, 9}, {2, -1, 0, 0, 0, 0}, {0, -1, 3, 1, 0, 0}, {0, -1, 3, 1, 0, 0}};
static const char *want_tiles =
    "first:16-35\tk__A;p__B\t5\t2\t3;2\n" "first:31-50\tk__A;p__B\t4294967295\t3\t4294967295;7\n" "first:46-65\tk__A;p__B;c__C\t1\t1\t*\n"
    "first:61-80\t\t2\t2\t1;1\n" "second_query:1-10\tk__Z\t9\t4\t5;4\n" "q3:31-50\t\t3\t1\t*\n" "q3:46-61\t\t3\t1\t*\n";
static const char *want_segs =
    "first\t1\t20\t1\tU\t\t0\n" "first\t16\t50\t2\tC\tk__A;p__B\t4294967300\n" "first\t46\t65\t1\tC\tk__A;p__B;c__C\t1\n" "first\t61\t80\t1\tC\t\t2\n"
    "first\t76\t95\t1\tU\t\t0\n" "second_query\t1\t10\t1\tC\tk__Z\t9\n" "q3\t1\t35\t2\tU\t\t0\n" "q3\t31\t61\t2\tC\t\t6\n";

int main(void) {
    static const char labels[] = "k__A;p__B\t1\nk__A;p__B;c__C\t1\nk__Z\t1\n";
    uint32_t *binix = (uint32_t *)calloc(UTREE_NUMBINS, 4);
    utree_ctr *ctr = NULL;
    if (!binix || utree_ctr_from_memory(8, 2, 1, binix, 4, NULL, labels, sizeof labels - 1, &ctr)) { puts("no database"); return 1; }
    free(binix);
    const uint8_t *nm = (const uint8_t *)names;
    char *big = malloc(4096);
    uint64_t lines = 0, segs = 0;
    utree_tiles_run st;
    memset(&st, 0, sizeof st);
    const size_t full = utree_tiles_format(ctr, nm, noff, nlen, slen, 20, 15, tq, ti, res, NT, big, 4096, &lines);
    if (full != strlen(want_tiles) || memcmp(big, want_tiles, full) || lines != 7) { printf("tiles differ:\n%.*s", (int)full, big); return 1; }
    const size_t sfull = utree_tiles_segments_format(ctr, nm, noff, nlen, slen, 20, 15, tq, ti, res, NT, 1, &st, big, 4096, &segs);
    if (sfull != strlen(want_segs) || memcmp(big, want_segs, sfull) || segs != 8 || st.open) { printf("segments differ:\n%.*s", (int)sfull, big); return 1; }
    for (size_t cap = 0; cap <= full || cap <= sfull; ++cap) {          /* an exactly sized heap block: any byte past cap is an ASan report */
        char *out = malloc(cap ? cap : 1);
        size_t r = utree_tiles_format(ctr, nm, noff, nlen, slen, 20, 15, tq, ti, res, NT, out, cap, NULL);
        if ((cap < full) != (r == (size_t)-1) || (cap >= full && (r != full || memcmp(out, want_tiles, full)))) { printf("tiles: wrong at cap %zu\n", cap); return 1; }
        utree_tiles_run s2, s0;
        memset(&s2, 0, sizeof s2); s2.open = 1; s2.query = 1; s2.start = 1; s2.end = 5; s2.n_tiles = 3;      /* (a run left open by an earlier call: one more line) */
        s0 = s2;
        memset(&st, 0, sizeof st);
        r = utree_tiles_segments_format(ctr, nm, noff, nlen, slen, 20, 15, tq, ti, res, NT, 1, cap < sfull ? &s2 : &st, out, cap, NULL);
        if ((cap < sfull) != (r == (size_t)-1) || (cap >= sfull && (r != sfull || memcmp(out, want_segs, sfull)))) { printf("segments: wrong at cap %zu\n", cap); return 1; }
        if (memcmp(&s2, &s0, sizeof s0)) { printf("segments: a failed call changed the state at cap %zu\n", cap); return 1; }
        free(out);
    }
    /* tile by tile, the run carried in the state: the same text */
    size_t at = 0;
    memset(&st, 0, sizeof st); segs = 0;
    for (size_t j = 0; j < NT; ++j) {
        char *out = malloc(256);
        size_t r = utree_tiles_segments_format(ctr, nm, noff, nlen, slen, 20, 15, tq + j, ti + j, res + j, 1, j + 1 == NT, &st, out, 256, &segs);
        if (r == (size_t)-1 || at + r > 4096) { puts("segments: a tile at a time failed"); return 1; }
        memcpy(big + at, out, r); at += r;
        free(out);
    }
    if (at != sfull || memcmp(big, want_segs, sfull) || segs != 8) { puts("segments: a tile at a time differs"); return 1; }
    /* a label that is none of the database's */
    utree_result bad = {3, -2, 1, 1, 0, 0};
    if (utree_tiles_format(ctr, nm, noff, nlen, slen, 20, 15, tq, ti, &bad, 1, big, 4096, NULL) != (size_t)-1) { puts("a foreign label went through"); return 1; }
    memset(&st, 0, sizeof st);
    if (utree_tiles_segments_format(ctr, nm, noff, nlen, slen, 20, 15, tq, ti, &bad, 1, 1, &st, big, 4096, NULL) != (size_t)-1) { puts("a foreign label went through"); return 1; }
    free(big);
    utree_ctr_close(ctr);
    puts("tiles_format_asan: ok");
    return 0;
}
