// samples_kernels.hip -- per-sample taxon counts of a batch of multiplexed reads (utree_samples_add, samples.c).
//
// One pass over a batch's records and names.  A read's sample id is its name up to the LAST delimiter byte (the whole name without one); its
// taxon is the key (label, cut) of its record, as in profile_kernels.hip.  The state lives on the device for the whole search (samples.h):
//   ids / arena      open-addressed table of the distinct ids; a slot's key points at the id's bytes in the arena.  A sample IS its slot here:
//                    every counter is indexed by the slot, so no lane ever needs a number another lane has yet to publish
//   index            the dense index a claim took from the counter of distinct ids (the read-back's numbering; the counter is the capacity check)
//   reads / uncl     per sample: all its reads, its reads without a line
//   cells            open-addressed {key, reads} slots, key = sample slot | label | cut packed into 64 bits
//
// Interning takes over redist_kernels.hip's insert, which has no lane waiting for another: probe read-only and compare WHOLE ids; on a miss
// write the bytes to arena space reserved with one atomic and claim the free slot with one compare-and-swap (release); whoever loses that race
// compares against the winner's bytes -- complete, they were written before the claim -- and probes on, keeping its copy for the next free
// slot.  A combined file is a concatenation of samples, so ids arrive in long runs: only a lane whose id differs from its predecessor lane's and
// from the one it had 1024 records before goes to the table (samples_dev.hpp: sm_resolve).
//
// Counting is profile_add_k's: one workgroup per CU, a hash table of cells in LDS, runs of equal keys carried in registers, and at the end one
// no-return atomic per non-zero LDS slot into the device tables.  Unclassified reads are a cell of their own in LDS only (cut =
// UTK_SAMPLES_CUT_UNCL) and leave it for uncl[]; every flushed count also goes to reads[], so the read-back can check reads = uncl + cells per
// sample.  Nothing is dropped silently: a full id table or arena, a full cell table, a label the database lacks, a name outside the text and a
// taxon too long for the packed key each set a bit of the error word, and the read-back then fails.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "samples.h"
#include "samples_dev.hpp"

#define SM_BLOCK 1024
#define SM_HSLOTS 8192u                    // LDS hash slots: 64 KiB of keys + 32 KiB of counts
#define SM_UNROLL 4

__device__ __forceinline__ uint64_t sm_key(uint32_t slot, uint32_t label, uint32_t cut16) {
    return (uint64_t)slot << (UTK_SAMPLES_LABEL_BITS + 16u) | (uint64_t)label << 16 | cut16;
}

// cnt reads of a cell into the device tables: the sample's reads, then its unclassified reads or the cell's slot (or the full flag)
__device__ void sm_global_add(const utk_samples_tab &t, uint64_t key, uint32_t cnt) {
    const uint32_t slot = (uint32_t)(key >> (UTK_SAMPLES_LABEL_BITS + 16u));
    sm_add(t.reads + slot, cnt);
    if ((uint32_t)(key & 0xFFFFu) == UTK_SAMPLES_CUT_UNCL) { sm_add(t.uncl + slot, cnt); return; }
    sm_cell_add(t, key, cnt);
}

struct SmLds {
    SmCells<SM_HSLOTS> cells;
    uint32_t flags;
};

__device__ void sm_lds_add(SmLds &s, const utk_samples_tab &t, uint64_t key, uint32_t cnt) {
    s.cells.add(key, cnt, [&](uint64_t k, uint32_t c) { sm_global_add(t, k, c); });
}

__global__ void __launch_bounds__(SM_BLOCK) samples_add_k(utk_samples_tab t, const uint8_t *__restrict__ text, uint64_t text_bytes,
                                                          const uint32_t *__restrict__ name_off, const uint32_t *__restrict__ name_len,
                                                          const utree_result *__restrict__ res, uint32_t n, uint32_t per_block) {
    __shared__ SmLds s;
    s.cells.init(threadIdx.x, SM_BLOCK);
    if (threadIdx.x == 0) s.flags = 0;
    __syncthreads();

    const uint64_t begin = (uint64_t)blockIdx.x * per_block;
    const uint64_t end = begin + per_block < n ? begin + per_block : n;
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t run = SM_KEY_FREE;
    uint32_t run_n = 0, flags = 0;
    SmPrev pv;
    for (uint64_t b0 = begin; b0 < end; b0 += (uint64_t)SM_UNROLL * SM_BLOCK) {       // (the same trips in every lane: sm_resolve needs them all)
        uint32_t off[SM_UNROLL], nlen[SM_UNROLL], lab[SM_UNROLL], fnd[SM_UNROLL];
        int32_t cut[SM_UNROLL];
        bool ok[SM_UNROLL];
#pragma unroll
        for (int u = 0; u < SM_UNROLL; ++u) {                        // all loads first: four records in flight per thread
            const uint64_t r = b0 + (uint64_t)u * SM_BLOCK + threadIdx.x;
            ok[u] = r < end; off[u] = 0; nlen[u] = 0; lab[u] = 0; cut[u] = -4; fnd[u] = 0;
            if (ok[u]) { off[u] = name_off[r]; nlen[u] = name_len[r]; lab[u] = res[r].label; cut[u] = res[r].cut; fnd[u] = res[r].found; }
        }
#pragma unroll
        for (int u = 0; u < SM_UNROLL; ++u) {
            uint32_t slot;
            const bool valid = sm_resolve(t, text, text_bytes, off[u], nlen[u], ok[u], lane, pv, flags, slot);
            if (valid && slot != SM_NONE) {
                uint64_t key = SM_KEY_FREE;
                if (!fnd[u] || cut[u] == -4) key = sm_key(slot, 0, UTK_SAMPLES_CUT_UNCL);
                else if (cut[u] == -1) key = sm_key(slot, 0, UTK_SAMPLES_CUT_EMPTY);
                else if (lab[u] >= t.n_labels) flags |= (uint32_t)UTK_SAMPLES_F_LABEL;      // no line can name it (utree_format_records fails on it too)
                else if (cut[u] > (int32_t)UTK_SAMPLES_CUT_MAX) flags |= (uint32_t)UTK_SAMPLES_F_CUT;
                else key = sm_key(slot, lab[u], cut[u] >= 0 ? (uint32_t)cut[u] : UTK_SAMPLES_CUT_WHOLE);
                if (key != SM_KEY_FREE) {
                    if (key == run) ++run_n;
                    else { sm_lds_add(s, t, run, run_n); run = key; run_n = 1; }
                }
            }
        }
    }
    sm_lds_add(s, t, run, run_n);
    if (flags) atomicOr(&s.flags, flags);
    __syncthreads();

    s.cells.flush(threadIdx.x, SM_BLOCK, [&](uint64_t k, uint32_t c) { sm_global_add(t, k, c); });
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0) sm_add(t.misc + 0, n);
        if (s.flags) sm_flag(t, s.flags);
    }
}

extern "C" int utk_samples_add(const utk_samples_tab *t, const uint8_t *d_text, uint64_t text_bytes, const uint32_t *d_name_off,
                               const uint32_t *d_name_len, const utree_result *d_res, uint32_t n, int n_cu, void *stream) {
    if (!n) return 0;
    // one workgroup per CU (the LDS table takes 96 KiB of its 160), each over a contiguous run of records; small batches take fewer
    uint32_t blocks = (uint32_t)(n_cu > 0 ? n_cu : 256);
    const uint32_t min_per = 4u * SM_UNROLL * SM_BLOCK;
    if ((n + min_per - 1) / min_per < blocks) blocks = (n + min_per - 1) / min_per;
    const uint32_t per = (uint32_t)(((uint64_t)n + blocks - 1) / blocks);
    hipLaunchKernelGGL(samples_add_k, dim3(blocks), dim3(SM_BLOCK), 0, (hipStream_t)stream, *t, d_text, text_bytes, d_name_off, d_name_len, d_res, n,
                       per);
    return (int)hipGetLastError();
}
