/* redist_reads_format_asan.c -- utree_redist_reads_format (csrc/redist.c) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone
 * host program: no GPU, no Python; the device side of redist.c and the taxon table are stubbed out.  Every cap from 0 to the exact size gets a heap
 * block of exactly that size, so a byte written behind cap is a report; names and label texts are heap blocks of exactly their size too.
 * `make -C utree_amd/csrc redist-reads-format-asan` builds and runs it; by hand, from the repository root:
 *
 *     gcc -std=gnu11 -g -O1 -fsanitize=address,undefined -fno-omit-frame-pointer -I/opt/rocm/include tools/redist_reads_format_asan.c \
 *         utree_amd/csrc/redist.c -o /tmp/redist_reads_format_asan && /tmp/redist_reads_format_asan
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../utree_amd/csrc/ctr_host.h"
#include "../utree_amd/csrc/dev_image.h"
#include "../utree_amd/csrc/redist.h"
#include "../utree_amd/csrc/taxon_table.h"
/* stubs for what redist.c links against */
int utk_redist_add(const utk_redist_tab *t, const utk_image *im, const utree_result *r, const utk_workspace *ws, uint32_t n, int n_cu, uint32_t *k, void *st) { return 0; }
int utk_redist_insert(const utk_redist_tab *t, const unsigned long long *r, const unsigned long long *f, const uint32_t *n, const uint32_t *l, uint64_t ns, void *st) { return 0; }
int utk_redist_sum(unsigned long long *d, const unsigned long long *s, uint64_t n, void *st) { return 0; }
int utk_redist_tally0(const utk_redist_tab *t, unsigned long long *ta, void *st) { return 0; }
int utk_redist_pass(const utk_redist_tab *t, const unsigned long long *p, unsigned long long *n, void *st) { return 0; }
int utk_redist_winner(const utk_redist_tab *t, const unsigned long long *ta, uint32_t *w, uint32_t *n, void *st) { return 0; }
int utk_redist_assign(const utk_redist_tab *t, const uint32_t *w, const uint32_t *nc, const uint32_t *k, uint64_t n, uint32_t *l, uint32_t *o, void *st) { return 0; }
int utree_classify_view(utree_dev *d, const utree_batch_view *v, utree_result *o, void *w, size_t wb, struct utree_redist *rd, struct utree_sredist *srd, uint32_t *k) { return 0; }
int utree_taxon_table_write(utree_taxon_row *rows, size_t n, int n_fig, int keyed, const char *header, const char *path) { return 0; }
void utree_dev_set_hip_error(int e, const char *w) {}
void utree_set_error_text(const char *m) {}
hipError_t hipSetDevice(int d) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t s) { return hipSuccess; }
hipError_t hipMalloc(void **p, size_t n) { *p = NULL; return hipErrorOutOfMemory; }
hipError_t hipFree(void *p) { return hipSuccess; }
hipError_t hipMemset(void *p, int v, size_t n) { return hipSuccess; }
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind k) { return hipSuccess; }

static void *exact(const char *s, size_t n) { void *p = malloc(n ? n : 1); memcpy(p, s, n); return p; }

int main(void) {
    /* labels: a usual one, an empty one, one with a space; names: a usual one, one with a space, a skipped read's, an empty one */
    const char *texts[3] = {"k__A;p__B;c__C", "", "k__Q x"};
    utree_ctr ctr;
    memset(&ctr, 0, sizeof ctr);
    ctr.info.n_labels = 3;
    char *labels[3]; uint32_t label_len[3];
    for (int i = 0; i < 3; ++i) { label_len[i] = (uint32_t)strlen(texts[i]); labels[i] = exact(texts[i], label_len[i]); }
    ctr.labels = (void *)labels; ctr.label_len = label_len;
    const char *all = "read/1two wordsskippedlast";
    uint8_t *names = exact(all, strlen(all));
    uint64_t noff[5] = {0, 6, 15, 22, 22}; uint32_t nlen[5] = {6, 9, 7, 0, 4};
    uint32_t label[5] = {0, 2, 0xFFFFFFFFu, 1, 0}, ncand[5] = {1, 15, 0, 4294967295u, 3};
    char *big = malloc(4096);
    const size_t full = utree_redist_reads_format(&ctr, names, noff, nlen, label, ncand, 5, big, 4096);
    const char *want = "read/1\tk__A;p__B;c__C\t1\ntwo words\tk__Q x\t15\n\t\t4294967295\nlast\tk__A;p__B;c__C\t3\n";
    if (full != strlen(want) || memcmp(big, want, full)) { printf("wrong bytes\n%.*s", (int)full, big); return 1; }
    printf("full %zu\n%.*s", full, (int)full, big);
    for (size_t cap = 0; cap <= full; ++cap) {               /* an exactly sized heap block: any byte past cap is an ASan report */
        char *out = malloc(cap ? cap : 1);
        const size_t r = utree_redist_reads_format(&ctr, names, noff, nlen, label, ncand, 5, out, cap);
        if ((cap < full) != (r == (size_t)-1)) { printf("wrong at cap %zu\n", cap); return 1; }
        if (cap == full && memcmp(out, want, full)) { puts("wrong bytes at the exact cap"); return 1; }
        free(out);
    }
    label[4] = 3;                                            /* a label the database does not have: refused, not read */
    if (utree_redist_reads_format(&ctr, names, noff, nlen, label, ncand, 5, big, 4096) != (size_t)-1) { puts("a bad label was taken"); return 1; }
    if (utree_redist_reads_format(&ctr, names, noff, nlen, label, ncand, 0, big, 0) != 0) { puts("no reads: not 0"); return 1; }
    for (int i = 0; i < 3; ++i) free(labels[i]);
    free(names); free(big);
    puts("ok");
    return 0;
}
