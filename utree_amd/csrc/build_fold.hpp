// build_fold.hpp -- the step of the reference's insert loop (xeTreeU / xeTreeU_RF, itree.c:242-307) that build_gpu.hip (the occurrences of a
// k-mer in a FASTA) and merge_kernels.hip (the nodes that carry a word in several databases) both replay: what a node's label becomes when
// the same word arrives under another label.  Labels are ids into the host-built "universe" of all label texts and their ';'-prefixes.
#ifndef UTREE_BUILD_FOLD_HPP
#define UTREE_BUILD_FOLD_HPP
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace utk_fold {

constexpr uint32_t ST_BAD = 0xFFFFFFFFu, ST_SKIP = 0xFFFFFFFEu;

struct universe {
    const char *blob; const uint64_t *off;         // NUL-terminated strings
    const uint32_t *trunc_off, *trunc_ids;         // trunc_ids[trunc_off[u] + m - 1] = u cut before its m-th ';'
};

// itree.c:286-295: ';' the two labels have in common before their first difference
__device__ __forceinline__ uint32_t shared_semicolons(const universe &U, uint32_t a, uint32_t b) {
    const char *x = U.blob + U.off[a], *y = U.blob + U.off[b];
    uint32_t n = 0;
    for (;; ++x, ++y) {
        const char c = *x;
        if (c != *y || !c) return n;
        n += c == ';';
    }
}

// the node holds `st` (never ST_BAD: BAD is absorbing, the caller stops there) and the word arrives under `nu`.
// Returns true when a cut produced the new st (the reference creates or finds that label then, itree.c:297-299).
template <bool GG>
__device__ __forceinline__ bool fold_next(const universe &U, uint32_t &st, uint32_t nu) {
    if (nu == st) return false;                                             // same label: nothing happens (262, 280)
    if (!GG) { st = ST_BAD; return false; }                                 // 264
    const uint32_t m = shared_semicolons(U, st, nu);
    if (m < 2) { st = ST_BAD; return false; }                               // critical_cutoff (74, 295)
    st = U.trunc_ids[U.trunc_off[st] + m - 1];                              // 296-301
    return true;
}

}  // namespace utk_fold
#endif
