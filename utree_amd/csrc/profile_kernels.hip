// profile_kernels.hip -- per-taxon read counts of a batch's utree_result records (utree_profile_add, profile.c).
//
// One pass over the records.  A read's taxon is the key (label, cut) of its record (include/utree_amd.h: utree_result); the counters
// live on the device for the whole search:
//   d_whole[label]   reads whose line prints the whole label (cut = -2, or any cut below -1 other than -4)
//   d_table          open-addressed {key, count} slots for truncated taxa, key = label << 32 | cut (cut >= 0), linear probing
//   d_misc           {total reads, unclassified (found == 0 or cut == -4), empty taxon (cut == -1), error flags}
//
// Real samples are dominated by a few taxa, so one atomic per read on one word would serialise (MI355X_MICROARCH.md: ~88 returning
// device-scope atomics per us on one word).  Each workgroup first counts in LDS -- a dense counter per label for the first PROF_DENSE
// labels and a small hash table for everything else -- and each thread keeps a run of equal keys in registers, so a batch of one hot taxon
// costs one LDS add per thread.  At the end the workgroup adds its non-zero slots to the device counters, one no-return atomic each; the
// dense counters go out in label order, so a wave's adds land on consecutive words.  A key the LDS table has no room for goes to the
// device counters directly.  A truncated key the device table has no room for sets PROF_F_FULL: the read-back returns UTREE_E_DEVICE.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "profile.h"

#define PROF_BLOCK 1024
#define PROF_DENSE 28672u                  // labels counted by index in LDS: 112 KiB
#define PROF_HSLOTS 2048u                  // LDS hash slots: 16 KiB of keys + 8 KiB of counts
#define PROF_LDS_PROBES 32u
#define PROF_DEV_PROBES 1024u
#define KEY_FREE (~0ull)                   // an unused slot (and "no run yet")
#define KEY_UNCL (~0ull - 1)               // no line
#define KEY_EMPTY (~0ull - 2)              // the empty taxon
// real keys have label < n_labels <= 0xFFFFFFFF, so their high word is at most 0xFFFFFFFE: they never meet the three above

__device__ __forceinline__ uint64_t prof_mix(uint64_t k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    return k ^ (k >> 33);
}

__device__ __forceinline__ void dev_add(unsigned long long *p, unsigned long long v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// whole label -> d_whole; truncated -> the device table (or the full flag)
__device__ void prof_global_add(uint64_t key, uint32_t cnt, unsigned long long *d_whole, unsigned long long *d_table, uint32_t mask,
                                unsigned long long *d_misc) {
    const uint32_t cut = (uint32_t)key;
    if (cut == 0xFFFFFFFEu) { dev_add(d_whole + (key >> 32), cnt); return; }
    const uint32_t h = (uint32_t)prof_mix(key);
    const uint32_t probes = mask + 1 < PROF_DEV_PROBES ? mask + 1 : PROF_DEV_PROBES;
    for (uint32_t p = 0; p < probes; ++p) {
        unsigned long long *slot = d_table + 2 * (size_t)((h + p) & mask);
        unsigned long long k = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == KEY_FREE) {
            k = KEY_FREE;
            __hip_atomic_compare_exchange_strong(slot, &k, (unsigned long long)key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
            if (k == KEY_FREE) k = key;     // we claimed it
        }
        if (k == key) { dev_add(slot + 1, cnt); return; }
    }
    (void)__hip_atomic_fetch_or(d_misc + 3, (unsigned long long)PROF_F_FULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct ProfLds {
    uint32_t dense[PROF_DENSE];
    unsigned long long key[PROF_HSLOTS];
    uint32_t cnt[PROF_HSLOTS];
    uint32_t uncl, empty, flags;
};

__device__ void prof_lds_add(ProfLds &s, uint64_t key, uint32_t cnt, uint32_t n_dense, unsigned long long *d_whole,
                             unsigned long long *d_table, uint32_t mask, unsigned long long *d_misc) {
    if (!cnt) return;
    if (key == KEY_UNCL) { atomicAdd(&s.uncl, cnt); return; }
    if (key == KEY_EMPTY) { atomicAdd(&s.empty, cnt); return; }
    if ((uint32_t)key == 0xFFFFFFFEu && (key >> 32) < n_dense) { atomicAdd(&s.dense[key >> 32], cnt); return; }
    const uint32_t h = (uint32_t)prof_mix(key);
    for (uint32_t p = 0; p < PROF_LDS_PROBES; ++p) {
        const uint32_t i = (h + p) & (PROF_HSLOTS - 1);
        unsigned long long k = s.key[i];
        if (k == KEY_FREE) {
            k = atomicCAS(&s.key[i], KEY_FREE, (unsigned long long)key);
            if (k == KEY_FREE) k = key;
        }
        if (k == key) { atomicAdd(&s.cnt[i], cnt); return; }
    }
    prof_global_add(key, cnt, d_whole, d_table, mask, d_misc);
}

__device__ __forceinline__ uint64_t prof_key(uint32_t label, int32_t cut, uint32_t found, uint32_t n_labels, uint32_t &bad) {
    if (!found || cut == -4) return KEY_UNCL;
    if (cut == -1) return KEY_EMPTY;
    if (label >= n_labels) { bad = 1; return KEY_FREE; }           // no line can name it (utree_format_records fails on it too)
    return (uint64_t)label << 32 | (cut >= 0 ? (uint32_t)cut : 0xFFFFFFFEu);
}

#define PROF_UNROLL 4

__global__ void __launch_bounds__(PROF_BLOCK) profile_add_k(const utree_result *__restrict__ res, uint32_t n, uint32_t per_block,
                                                            uint32_t n_labels, unsigned long long *d_whole, unsigned long long *d_table,
                                                            uint32_t mask, unsigned long long *d_misc) {
    __shared__ ProfLds s;
    const uint32_t n_dense = n_labels < PROF_DENSE ? n_labels : PROF_DENSE;
    for (uint32_t i = threadIdx.x; i < n_dense; i += PROF_BLOCK) s.dense[i] = 0;
    for (uint32_t i = threadIdx.x; i < PROF_HSLOTS; i += PROF_BLOCK) { s.key[i] = KEY_FREE; s.cnt[i] = 0; }
    if (threadIdx.x == 0) { s.uncl = 0; s.empty = 0; s.flags = 0; }
    __syncthreads();

    const uint64_t begin = (uint64_t)blockIdx.x * per_block;
    const uint64_t end = begin + per_block < n ? begin + per_block : n;
    uint64_t run = KEY_FREE;
    uint32_t run_n = 0, bad = 0;
    for (uint64_t r0 = begin + threadIdx.x; r0 < end; r0 += PROF_UNROLL * PROF_BLOCK) {
        uint32_t lab[PROF_UNROLL], fnd[PROF_UNROLL];
        int32_t cut[PROF_UNROLL];
#pragma unroll
        for (int u = 0; u < PROF_UNROLL; ++u) {                      // all loads first: four records in flight per thread
            const uint64_t r = r0 + (uint64_t)u * PROF_BLOCK;
            lab[u] = 0; cut[u] = -4; fnd[u] = 0;
            if (r < end) { lab[u] = res[r].label; cut[u] = res[r].cut; fnd[u] = res[r].found; }
        }
#pragma unroll
        for (int u = 0; u < PROF_UNROLL; ++u) {
            if (r0 + (uint64_t)u * PROF_BLOCK >= end) break;
            const uint64_t key = prof_key(lab[u], cut[u], fnd[u], n_labels, bad);
            if (key == KEY_FREE) continue;
            if (key == run) { ++run_n; continue; }
            prof_lds_add(s, run, run_n, n_dense, d_whole, d_table, mask, d_misc);
            run = key; run_n = 1;
        }
    }
    prof_lds_add(s, run, run_n, n_dense, d_whole, d_table, mask, d_misc);
    if (bad) atomicOr(&s.flags, (uint32_t)PROF_F_LABEL);
    __syncthreads();

    for (uint32_t i = threadIdx.x; i < n_dense; i += PROF_BLOCK)
        if (s.dense[i]) dev_add(d_whole + i, s.dense[i]);
    for (uint32_t i = threadIdx.x; i < PROF_HSLOTS; i += PROF_BLOCK)
        if (s.key[i] != KEY_FREE && s.cnt[i]) prof_global_add(s.key[i], s.cnt[i], d_whole, d_table, mask, d_misc);
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0) dev_add(d_misc + 0, n);
        if (s.uncl) dev_add(d_misc + 1, s.uncl);
        if (s.empty) dev_add(d_misc + 2, s.empty);
        if (s.flags) (void)__hip_atomic_fetch_or(d_misc + 3, (unsigned long long)s.flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

extern "C" int utk_profile_add(const utree_result *d_res, uint32_t n, uint32_t n_labels, unsigned long long *d_whole,
                               unsigned long long *d_table, uint32_t mask, unsigned long long *d_misc, int n_cu, void *stream) {
    if (!n) return 0;
    // one workgroup per CU (the LDS counters take 136 KiB of its 160), each over a contiguous run of records; small batches take fewer
    uint32_t blocks = (uint32_t)(n_cu > 0 ? n_cu : 256);
    const uint32_t min_per = 4u * PROF_UNROLL * PROF_BLOCK;
    if ((n + min_per - 1) / min_per < blocks) blocks = (n + min_per - 1) / min_per;
    const uint32_t per = (uint32_t)(((uint64_t)n + blocks - 1) / blocks);
    hipLaunchKernelGGL(profile_add_k, dim3(blocks), dim3(PROF_BLOCK), 0, (hipStream_t)stream, d_res, n, per, n_labels, d_whole, d_table,
                       mask, d_misc);
    return (int)hipGetLastError();
}
