// samples_dev.hpp -- the device side of the table of sample ids and of the {key, reads} cell table (samples.h: utk_samples_tab), shared by
// samples_kernels.hip and sredist_kernels.hip: the intern of an id, a batch's names resolved to sample slots a wavefront at a time (sm_resolve),
// a workgroup's hash table of cells in LDS (SmCells) and the add to the cell table behind it.
//
// Interning takes over redist_dev.hpp's insert, which has no lane waiting for another: probe read-only and compare WHOLE ids; on a miss
// write the bytes to arena space reserved with one atomic and claim the free slot with one compare-and-swap (release); whoever loses that race
// compares against the winner's bytes -- complete, they were written before the claim -- and probes on, keeping its copy for the next free
// slot.
#ifndef UTREE_SAMPLES_DEV_HPP
#define UTREE_SAMPLES_DEV_HPP
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "samples.h"

#define SM_DEV_PROBES 4096u
#define SM_KEY_FREE (~0ull)                // an unused cell slot (and "no run yet")
#define SM_ID_FREE 0ull                    // an unused id slot: a key's low word is the id's length + 1
#define SM_NONE 0xFFFFFFFFu                // no sample: the error word says why
#define SM_LDS_PROBES 32u

__device__ __forceinline__ uint64_t sm_mix(uint64_t k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    return k ^ (k >> 33);
}
__device__ __forceinline__ void sm_add(unsigned long long *p, unsigned long long v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void sm_flag(const utk_samples_tab &t, unsigned long long f) {
    (void)__hip_atomic_fetch_or(t.misc + 1, f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// bytes of the name in front of its last delimiter; the whole name when it has none
__device__ __forceinline__ uint32_t sm_id_len(const uint8_t *__restrict__ name, uint32_t len, uint32_t delim) {
    for (uint32_t i = len; i > 0; --i) if (name[i - 1] == delim) return i - 1;
    return len;
}
__device__ __forceinline__ bool sm_same(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) if (a[i] != b[i]) return false;
    return true;
}

// the slot of the id's n bytes, claimed when no slot holds them yet; SM_NONE (and a flag) when the table or the arena has no room
__device__ uint32_t sm_intern(const utk_samples_tab &t, const uint8_t *__restrict__ id, uint32_t n) {
    uint32_t h = 0x811C9DC5u;
    for (uint32_t i = 0; i < n; ++i) h = (h ^ id[i]) * 0x01000193u;
    h ^= h >> 15; h *= 0x85EBCA77u; h ^= h >> 13;
    unsigned long long mine = SM_ID_FREE;                  // the key of this lane's own arena copy, once written
    const uint32_t probes = t.id_mask + 1 < SM_DEV_PROBES ? t.id_mask + 1 : SM_DEV_PROBES;
    for (uint32_t p = 0; p < probes; ++p) {
        const uint32_t s = (h + p) & t.id_mask;
        unsigned long long *slot = t.ids + s;
        unsigned long long k = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == SM_ID_FREE) {
            if (mine == SM_ID_FREE) {
                const unsigned long long at = __hip_atomic_fetch_add(t.misc + 2, (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (at + n > t.arena_cap) { sm_flag(t, UTK_SAMPLES_F_ARENA); return SM_NONE; }
                for (uint32_t i = 0; i < n; ++i) t.arena[at + i] = id[i];
                mine = at << 32 | (n + 1u);
            }
            unsigned long long expect = SM_ID_FREE;
            if (__hip_atomic_compare_exchange_strong(slot, &expect, mine, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)) {
                const unsigned long long c = __hip_atomic_fetch_add(t.misc + 3, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (c >= t.sample_cap) { sm_flag(t, UTK_SAMPLES_F_TABLE); return SM_NONE; }
                t.index[s] = (uint32_t)c;
                return s;
            }
            k = expect;                                    // somebody else's id, complete: compare like any occupied slot
        }
        if ((uint32_t)k != n + 1u) continue;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");           // the bytes behind a key that has been seen
        const uint8_t *a = t.arena + (k >> 32);
        bool same = true;
        for (uint32_t i = 0; i < n && same; ++i) same = __hip_atomic_load(a + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == id[i];
        if (same) return s;
    }
    sm_flag(t, UTK_SAMPLES_F_TABLE);
    return SM_NONE;
}

// The id a thread resolved one round before, and its slot: a combined file is a concatenation of samples, so it is most often this round's too.
struct SmPrev { uint32_t off = 0, idl = 0, slot = SM_NONE; bool ok = false; };

// The sample slot of one record per lane: the name is text[off .. off + nlen) (`ok`: the lane has a record), its id the bytes in front of the
// last delimiter.  A lane compares its id with its predecessor lane's (length, then bytes) and then with `pv`'s; only a lane that begins a run in
// both senses goes to the table, and the lanes behind it take its slot from a wavefront shuffle.  False: no record, or a name outside the text
// (UTK_SAMPLES_F_NAME into `flags`); `slot` may still be SM_NONE for a record (the table flagged why).
// EVERY lane of the workgroup calls this the same number of times, records or not: the shuffles and the ballot need whole wavefronts.
__device__ __forceinline__ bool sm_resolve(const utk_samples_tab &t, const uint8_t *__restrict__ text, uint64_t text_bytes, uint32_t off, uint32_t nlen,
                                           bool ok, uint32_t lane, SmPrev &pv, uint32_t &flags, uint32_t &slot) {
    bool valid = ok;
    if (valid && ((uint64_t)off > text_bytes || (uint64_t)nlen > text_bytes - off)) { flags |= (uint32_t)UTK_SAMPLES_F_NAME; valid = false; }
    const uint8_t *id = text + (valid ? off : 0u);
    const uint32_t idl = valid ? sm_id_len(id, nlen, t.delim) : 0u;
    // the predecessor in record order is the lane below
    const uint32_t p_off = (uint32_t)__shfl_up((int)off, 1), p_idl = (uint32_t)__shfl_up((int)idl, 1);
    const int p_valid = __shfl_up((int)valid, 1);
    bool head = valid;
    if (valid && lane > 0 && p_valid && p_idl == idl && sm_same(id, text + p_off, idl)) head = false;
    slot = SM_NONE;
    if (head) {
        if (pv.ok && pv.idl == idl && sm_same(id, text + pv.off, idl)) slot = pv.slot;
        else slot = sm_intern(t, id, idl);
    }
    // every lane takes the slot of the nearest head at or below it (a valid lane 0 is one; lanes beyond the batch's end follow no valid lane)
    const uint64_t heads = __ballot(head);
    const uint64_t below = heads & ((2ull << lane) - 1ull);
    const int src = below ? 63 - __clzll((long long)below) : (int)lane;
    slot = (uint32_t)__shfl((int)slot, src);
    if (valid) { pv.off = off; pv.idl = idl; pv.slot = slot; pv.ok = true; }
    return valid;
}

// cnt reads into the slot of the cell table that holds `key` (never all ones), claimed when no slot holds it yet; the full flag when there is none
__device__ void sm_cell_add(const utk_samples_tab &t, uint64_t key, unsigned long long cnt) {
    const uint32_t h = (uint32_t)sm_mix(key);
    const uint32_t probes = t.cell_mask + 1 < SM_DEV_PROBES ? t.cell_mask + 1 : SM_DEV_PROBES;
    for (uint32_t p = 0; p < probes; ++p) {
        unsigned long long *c = t.cells + 2 * (size_t)((h + p) & t.cell_mask);
        unsigned long long k = __hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == SM_KEY_FREE) {
            k = SM_KEY_FREE;
            __hip_atomic_compare_exchange_strong(c, &k, (unsigned long long)key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (k == SM_KEY_FREE) k = key;     // we claimed it
        }
        if (k == key) { sm_add(c + 1, cnt); return; }
    }
    sm_flag(t, UTK_SAMPLES_F_CELLS);
}

// A workgroup's hash table of cells in LDS: counts gather here and leave for the device tables once, at the end.  SINK (key, cnt) is what takes a
// count to the device tables -- one that found no room within the probe limit, and every non-zero slot in flush.
template <uint32_t SLOTS>
struct SmCells {
    unsigned long long key[SLOTS];
    uint32_t cnt[SLOTS];
    __device__ __forceinline__ void init(uint32_t tid, uint32_t block) {              // (a barrier before the first add)
        for (uint32_t i = tid; i < SLOTS; i += block) { key[i] = SM_KEY_FREE; cnt[i] = 0; }
    }
    template <class SINK>
    __device__ __forceinline__ void add(uint64_t k0, uint32_t n, SINK sink) {
        if (!n) return;
        const uint32_t h = (uint32_t)sm_mix(k0);
        for (uint32_t p = 0; p < SM_LDS_PROBES; ++p) {
            const uint32_t i = (h + p) & (SLOTS - 1);
            unsigned long long k = key[i];
            if (k == SM_KEY_FREE) {
                k = atomicCAS(&key[i], SM_KEY_FREE, (unsigned long long)k0);
                if (k == SM_KEY_FREE) k = k0;
            }
            if (k == k0) { atomicAdd(&cnt[i], n); return; }
        }
        sink(k0, n);
    }
    template <class SINK>
    __device__ __forceinline__ void flush(uint32_t tid, uint32_t block, SINK sink) {  // (a barrier after the last add)
        for (uint32_t i = tid; i < SLOTS; i += block)
            if (key[i] != SM_KEY_FREE && cnt[i]) sink(key[i], cnt[i]);
    }
};

#endif
