/* hitmap_format_asan.c -- utree_hitmap_format (csrc/hitmap.c) under AddressSanitizer + UndefinedBehaviorSanitizer, as a
 * stand-alone host program: no GPU, no Python; the device side of hitmap.c is stubbed out.  Every cap from 0 to the exact size gets a heap block of exactly
 * that size, so a byte written behind cap is a report.  From the repository root:
 *
 *     gcc -std=gnu11 -g -O1 -fsanitize=address,undefined -fno-omit-frame-pointer -I/opt/rocm/include tools/hitmap_format_asan.c utree_amd/csrc/hitmap.c \
 *         -o /tmp/hitmap_format_asan && /tmp/hitmap_format_asan
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../utree_amd/csrc/hitmap.h"
/* stubs for what hitmap.c links against */
size_t utk_hitmap_scan_temp_bytes(uint32_t n, uint64_t g) { return 1024; }
int utk_hitmap_run(const utk_image *im, const uint8_t *b, const uint64_t *o, const uint32_t *l, uint32_t n, uint64_t tb, int rc, uint64_t *ro, utree_hit_run *r, uint64_t cap, utree_hitmap_meta *m, const utk_hitmap_ws *ws, int n_cu, void *st) { return 0; }
void utree_dev_set_hip_error(int e, const char *w) {}
hipError_t hipSetDevice(int d) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
int main(void) {
    const char *names = "read/1emptyr3bigx";
    uint64_t noff[5] = {0, 6, 11, 13, 16}; uint32_t nlen[5] = {6, 5, 2, 3, 1};
    utree_hit_run runs[9] = {{7,3},{0xFFFFFFFFu,2},{0xFFFFFFFEu,32},{0,1},{4294967293u,5},{0xFFFFFFFFu,119},{12,4294967295u},{0xFFFFFFFEu,1234567890u},{0xFFFFFFFEu,1}};
    uint64_t roff[6] = {0, 5, 5, 6, 8, 9};
    char *big = malloc(4096);
    size_t full = utree_hitmap_format((const uint8_t *)names, noff, nlen, roff, runs, 5, big, 4096);
    printf("full %zu\n%.*s", full, (int)full, big);
    for (size_t cap = 0; cap <= full; ++cap) {               /* an exactly sized heap block: any byte past cap is an ASan report */
        char *out = malloc(cap ? cap : 1);
        size_t r = utree_hitmap_format((const uint8_t *)names, noff, nlen, roff, runs, 5, out, cap);
        if ((cap < full) != (r == (size_t)-1)) { printf("wrong at cap %zu\n", cap); return 1; }
        free(out);
    }
    free(big);
    puts("ok");
    return 0;
}
