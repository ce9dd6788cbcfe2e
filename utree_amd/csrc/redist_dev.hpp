// redist_dev.hpp -- the device side of the table of candidate sets (redist.h: utk_redist_tab), shared by redist_kernels.hip and
// sredist_kernels.hip: the tied maximum of a read's (rank, count) list as a sequence of labels, and the insert of such a sequence.
//
// Insert: probe read-only and compare WHOLE sets (a hash alone would merge two sets silently); only on a miss write the labels to freshly
// reserved arena space and claim the free slot with one compare-and-swap of the key (release: the labels are visible before the key).  Whoever
// loses that race compares against the winner's labels -- complete, they were written before the claim --, takes the slot when they are
// equal (its own arena space stays unused) and probes on otherwise, keeping its space for the next free slot.  No lane ever waits for another
// lane to publish: the lanes of a wavefront make no independent progress.  A table or arena that is used up sets a flag in the error word.
#ifndef UTREE_REDIST_DEV_HPP
#define UTREE_REDIST_DEV_HPP
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "redist.h"

#define RD_PROBES 4096u
#define RD_FREE 0ull                       // a key holds at least two labels in its low word: never 0
#define RD_NO_SLOT 0xFFFFFFFFu             // rd_insert: the set found no slot (the error word says why)
#define RD_CUT_PENDING (-3)                // as in kernels.hip (vote_k finishes those records)
#define RD_RANK_PENDING (-4)

__device__ __forceinline__ void rd_add(unsigned long long *p, unsigned long long v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void rd_flag(const utk_redist_tab &t, unsigned long long f) {
    (void)__hip_atomic_fetch_or(t.misc + 1, f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t rd_mix(uint32_t h, uint32_t v) {
    h ^= v; h *= 0x9E3779B1u; h ^= h >> 15; h *= 0x85EBCA77u;
    return h ^ (h >> 13);
}

// the tied entries of a (rank, count) list as file-order indices, in list order: the first four in registers (most sets are that small: the
// hash and every compare then read no memory), the rest by walking the list on from `pos4`
struct TiedSeq {
    const uint64_t *T; const uint32_t *r2i; uint32_t mx, uix, n_labels, c0, c1, c2, c3, pos4, idx, pos;
    __device__ void reset() { idx = 0; pos = pos4; }
    __device__ uint32_t next() {                           // ~0: beyond the list, or a rank the database does not have (rd_insert refuses it)
        const uint32_t i = idx++;
        if (i < 4u) return i == 0u ? c0 : i == 1u ? c1 : i == 2u ? c2 : c3;
        while (pos < uix) { const uint64_t e = T[pos++]; if ((uint32_t)(e >> 32) == mx) return (uint32_t)e < n_labels ? r2i[(uint32_t)e] : 0xFFFFFFFFu; }
        return 0xFFFFFFFFu;
    }
};
struct FlatSeq {
    const uint32_t *p; uint32_t pos;
    __device__ void reset() { pos = 0; }
    __device__ uint32_t next() { return p[pos++]; }
};

// `reads` reads whose candidate set is the n (>= 2) labels of `seq`; returns the set's slot, RD_NO_SLOT when it has none
template <class SEQ>
__device__ uint32_t rd_insert(const utk_redist_tab &t, SEQ &seq, uint32_t n, unsigned long long reads) {
    uint32_t h = 0x811C9DC5u;
    seq.reset();
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t l = seq.next();
        if (l >= t.n_labels) { rd_flag(t, UTK_REDIST_F_LABEL); return RD_NO_SLOT; }      // every label in the arena indexes a tally
        h = rd_mix(h, l);
    }
    unsigned long long mine = RD_FREE;                     // the key of this lane's own arena copy, once written
    const uint32_t probes = t.mask + 1 < RD_PROBES ? t.mask + 1 : RD_PROBES;
    for (uint32_t p = 0; p < probes; ++p) {
        const uint32_t at_slot = (h + p) & t.mask;
        unsigned long long *slot = t.slots + 2 * (size_t)at_slot;
        unsigned long long k = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == RD_FREE) {
            if (mine == RD_FREE) {
                const unsigned long long at = __hip_atomic_fetch_add(t.misc + 2, (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (at + n > t.arena_cap) { rd_flag(t, UTK_REDIST_F_ARENA); return RD_NO_SLOT; }
                seq.reset();
                for (uint32_t i = 0; i < n; ++i) t.arena[at + i] = seq.next();
                mine = at << 32 | n;
            }
            unsigned long long expect = RD_FREE;
            if (__hip_atomic_compare_exchange_strong(slot, &expect, mine, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)) {
                if (reads) rd_add(slot + 1, reads);
                return at_slot;
            }
            k = expect;                                    // somebody else's set, complete: compare like any occupied slot
        }
        if ((uint32_t)k != n) continue;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");           // the labels behind a key that has been seen
        const uint32_t *a = t.arena + (k >> 32);
        bool same = true;
        seq.reset();
        for (uint32_t i = 0; i < n && same; ++i) same = __hip_atomic_load(a + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == seq.next();
        if (same) { if (reads) rd_add(slot + 1, reads); return at_slot; }
    }
    rd_flag(t, UTK_REDIST_F_TABLE);
    return RD_NO_SLOT;
}

#endif
