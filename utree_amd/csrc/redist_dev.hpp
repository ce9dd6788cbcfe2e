// redist_dev.hpp -- the device side of the table of candidate sets (redist.h: utk_redist_tab), shared by redist_kernels.hip and
// sredist_kernels.hip: the scans of a read's (rank, count) list for its tied maximum (rd_scan_listed, rd_scan_tied), that maximum as a sequence
// of labels, and the insert of such a sequence.
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
#include <type_traits>
#include "redist.h"

#define RD_PROBES 4096u
#define RD_FREE 0ull                       // a key holds at least two labels in its low word: never 0
#define RD_NO_SLOT 0xFFFFFFFFu             // rd_insert: the set found no slot (the error word says why)
#define RD_CUT_PENDING (-3)                // as in kernels.hip (vote_k finishes those records)
#define RD_RANK_PENDING (-4)
#define RD_UNROLL 4                        // queued reads a thread scans side by side (rd_scan_listed)

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

// RD_UNROLL queued reads per thread -- queue entries first, first + BLOCK, ... below qn --, each with a (rank, count) list whose tied maximum is
// its candidate set.  The four reads' records, list entries and index look-ups are requested side by side: every step of one read's chain is a
// dependent load, and most listed reads end as a single candidate (one label has the most hits), so the loads are the cost.
//   decode(i, r, tag)   queue entry i -> the read's record index and whatever else the sinks want of it
//   one(tag, c)         the read's only candidate is the file-order index c (~0: a rank the database does not have)
//   many(r, tag)        it has several: onto the second queue
//   none(tag)           it has none (an empty list: refused, the error word is set); may be left out
struct RdNoSink {};
template <uint32_t BLOCK, class DECODE, class ONE, class MANY, class NONE = RdNoSink>
__device__ __forceinline__ void rd_scan_listed(const utk_redist_tab &t, const uint32_t *__restrict__ rank2ix, const utree_result *__restrict__ res,
                                               const uint64_t *__restrict__ tally, uint32_t first, uint32_t qn, DECODE decode, ONE one, MANY many,
                                               NONE none = NONE()) {
    const uint32_t nl = t.n_labels;
    uint32_t uix[RD_UNROLL], mx[RD_UNROLL], ties[RD_UNROLL], k0[RD_UNROLL], rr[RD_UNROLL], tag[RD_UNROLL], umax = 0;
    const uint64_t *T[RD_UNROLL];
#pragma unroll
    for (int u = 0; u < RD_UNROLL; ++u) {
        const uint32_t i = first + (uint32_t)u * BLOCK;
        uix[u] = 0; T[u] = tally; mx[u] = 0; ties[u] = 0; k0[u] = 0; rr[u] = 0; tag[u] = 0;
        if (i < qn) {
            decode(i, rr[u], tag[u]);
            const uint32_t *rec = (const uint32_t *)&res[rr[u]];
            uix[u] = rec[3];
            T[u] = tally + ((uint64_t)rec[4] | ((uint64_t)rec[5] << 32));
        }
    }
#pragma unroll
    for (int u = 0; u < RD_UNROLL; ++u) umax = uix[u] > umax ? uix[u] : umax;
    for (uint32_t i = 0; i < umax; ++i) {
        uint64_t e[RD_UNROLL];
#pragma unroll
        for (int u = 0; u < RD_UNROLL; ++u) e[u] = i < uix[u] ? T[u][i] : 0ull;
#pragma unroll
        for (int u = 0; u < RD_UNROLL; ++u) {
            if (i >= uix[u]) continue;
            const uint32_t c = (uint32_t)(e[u] >> 32), rk = (uint32_t)e[u];
            if (c > mx[u]) { mx[u] = c; ties[u] = 1; k0[u] = rk; }
            else if (c == mx[u]) ++ties[u];
        }
    }
    uint32_t c0[RD_UNROLL];
#pragma unroll
    for (int u = 0; u < RD_UNROLL; ++u) c0[u] = ties[u] == 1 && k0[u] < nl ? rank2ix[k0[u]] : 0xFFFFFFFFu;
#pragma unroll
    for (int u = 0; u < RD_UNROLL; ++u) {
        if (first + (uint32_t)u * BLOCK >= qn) continue;
        if (!ties[u] || !mx[u]) {                                                   // (an empty list: the classify kernels write none; never dropped silently)
            rd_flag(t, UTK_REDIST_F_LABEL);
            if constexpr (!std::is_same<NONE, RdNoSink>::value) none(tag[u]);
            continue;
        }
        if (ties[u] == 1) one(tag[u], c0[u]);
        else many(rr[u], tag[u]);                                                   // several candidates: the table, with full wavefronts
    }
}

// the list of record r scanned once more, its tied maximum into `seq`; returns how many are tied (below 2: `seq` is not set)
__device__ __forceinline__ uint32_t rd_scan_tied(const utk_redist_tab &t, const uint32_t *__restrict__ rank2ix, const utree_result *__restrict__ res,
                                                 const uint64_t *__restrict__ tally, uint32_t r, TiedSeq &seq) {
    const uint32_t *rec = (const uint32_t *)&res[r];
    const uint32_t uix = rec[3], nl = t.n_labels;
    const uint64_t *T = tally + ((uint64_t)rec[4] | ((uint64_t)rec[5] << 32));
    uint32_t mx = 0, ties = 0, k0 = 0, k1 = 0, k2 = 0, k3 = 0, pos4 = 0;
    for (uint32_t i = 0; i < uix; ++i) {
        const uint64_t e = T[i];
        const uint32_t c = (uint32_t)(e >> 32), rk = (uint32_t)e;
        if (c > mx) { mx = c; ties = 1; k0 = rk; }
        else if (c == mx) {
            if (ties == 1) k1 = rk; else if (ties == 2) k2 = rk; else if (ties == 3) { k3 = rk; pos4 = i + 1; }
            ++ties;
        }
    }
    if (ties < 2) return ties;
    seq = {T, rank2ix, mx, uix, nl, k0 < nl ? rank2ix[k0] : 0xFFFFFFFFu, k1 < nl ? rank2ix[k1] : 0xFFFFFFFFu,
           ties > 2 && k2 < nl ? rank2ix[k2] : 0xFFFFFFFFu, ties > 3 && k3 < nl ? rank2ix[k3] : 0xFFFFFFFFu, pos4, 0, 0};
    return ties;
}

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
