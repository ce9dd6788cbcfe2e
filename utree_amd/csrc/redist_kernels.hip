// redist_kernels.hip -- the candidate sets of ambiguous reads, kept on the device for a whole search, and their redistribution (redist.c,
// include/utree_amd.h: utree_redist_*).
//
// redist_add_k runs between a batch's classify kernels and vote_k, one lane per read, as vote_k walks the same records: a read's distinct
// labels and their hit counts still stand as a (rank, count) list in the workspace (ascending rank), the record points at it.  The labels tied
// for the highest count are the read's candidate set.  One candidate: a counter per label (d_single), counted in LDS first for the reason
// profile_kernels.hip gives -- a sample is dominated by a few taxa and one atomic per read on one word would serialise.  More: the set goes
// into an open-addressed table of {key, reads} slots, key = arena offset << 32 | labels (0: free), the labels (file-order indices, in the list's order:
// equal sets arrive as equal sequences) in an arena.
//
// Insert (redist_dev.hpp): whole sets are compared, a key is published only after its labels, no lane waits for another; a table or arena
// that is used up sets a flag in the error word; the read-back then fails (UTREE_E_DEVICE), no read is dropped silently.
//
// Keys (redist_add_k<true>, include/utree_amd.h: utree_redist_classify_batch_keys): the same pass also writes, per read, where its candidates
// are -- nothing, a label, or the slot rd_insert found or claimed for its set -- one 4-byte store at each place a read's fate is known.  After a
// solve redist_winner_k evaluates win(set, T_P) once per slot, and redist_assign_k gathers each read's label and number of candidates by key.
//
// redist_tally0_k / redist_pass_k: one thread per slot; the set's reads go to every member (T0) or to the richest member under the previous
// tally, the smallest file-order index on a tie (a pass), one no-return atomic each; the singleton counters enter every tally as a constant;
// redist_changes_k reduces sum |next - prev| to one word, the only thing the host reads per pass.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "redist.h"
#include "redist_dev.hpp"

#define RD_BLOCK 1024
#define RD_DENSE 27648u                    // labels counted by index in LDS: 108 KiB

#define RD_TILE 4096u                      // reads a workgroup takes per round = the capacity of its queue of listed reads
#define RD_Q2 8192u                        // capacity of its queue of reads with several candidates, emptied when a further round might not fit
struct RdLds { uint32_t dense[RD_DENSE]; uint32_t q[RD_TILE]; uint32_t q2[RD_Q2]; uint32_t qn, q2n; };

__device__ __forceinline__ void rd_single(const utk_redist_tab &t, RdLds &s, uint32_t n_dense, uint32_t one) {
    if (one >= t.n_labels) { rd_flag(t, UTK_REDIST_F_LABEL); return; }
    if (one < n_dense) atomicAdd(&s.dense[one], 1u);
    else rd_add(t.single + one, 1ull);
}
// the key of a read whose only candidate is `one` (a label rd_single refuses: none)
__device__ __forceinline__ uint32_t rd_key_single(const utk_redist_tab &t, uint32_t one) { return one < t.n_labels ? one : UTREE_REDIST_KEY_NONE; }

// RD_UNROLL queued reads per thread (redist_dev.hpp: rd_scan_listed): one candidate is counted, several go on the second queue; KEYS: the
// read's index is the tag, and a read that ends here gets its key
template <bool KEYS>
__device__ void rd_listed(const utk_redist_tab &t, RdLds &s, uint32_t n_dense, const uint32_t *__restrict__ rank2ix, const utree_result *__restrict__ res,
                          const uint64_t *__restrict__ tally, uint32_t first, uint32_t qn, uint32_t *__restrict__ key) {
    rd_scan_listed<RD_BLOCK>(t, rank2ix, res, tally, first, qn,
                             [&](uint32_t i, uint32_t &r, uint32_t &tag) { r = s.q[i]; if (KEYS) tag = r; },
                             [&](uint32_t tag, uint32_t one) { rd_single(t, s, n_dense, one); if (KEYS) key[tag] = rd_key_single(t, one); },
                             [&](uint32_t r, uint32_t) { s.q2[atomicAdd(&s.q2n, 1u)] = r; },
                             [&](uint32_t tag) { if (KEYS) key[tag] = UTREE_REDIST_KEY_NONE; });
}

// a queued read with several candidates: its set into the table; KEYS: the slot it is in is the read's key
template <bool KEYS>
__device__ void rd_multi(const utk_redist_tab &t, const uint32_t *__restrict__ rank2ix, const utree_result *__restrict__ res,
                         const uint64_t *__restrict__ tally, uint32_t r, uint32_t *__restrict__ key) {
    TiedSeq seq;
    const uint32_t ties = rd_scan_tied(t, rank2ix, res, tally, r, seq);
    if (ties < 2) {                                               // (rd_listed queued it for having more: never dropped silently)
        rd_flag(t, UTK_REDIST_F_LABEL);
        if (KEYS) key[r] = UTREE_REDIST_KEY_NONE;
        return;
    }
    const uint32_t slot = rd_insert(t, seq, ties, 1ull);
    if (KEYS) key[r] = slot == RD_NO_SLOT ? UTREE_REDIST_KEY_NONE : 0x80000000u | slot;
}

// Rounds of RD_TILE reads per workgroup.  First every thread takes its records, four loads in flight: no hit -- nothing; one distinct label --
// counted in LDS; a list -- the read's index goes on the workgroup's queue.  Then that queue is dealt out over all lanes, which find each
// list's tied maximum: one candidate is counted, several put the read on a second queue, and that one is dealt out in turn when it may not
// hold another round's reads.  A wavefront executes the union of its lanes' paths, and a probe of the table is a chain of device-scope
// round trips: with one read in twelve ambiguous nearly every wavefront ran that chain for a few of its lanes in every step when the reads were
// taken as they came (measured: 2.6 ms per 16 M reads that way, 1.9 ms with the first queue alone, of which 1.7 ms were the probes).
// KEYS: key[r] is written for every read r of the batch, once, where the read leaves the pass (false: `key` is not looked at).
template <bool KEYS>
__global__ void __launch_bounds__(RD_BLOCK) redist_add_k(utk_redist_tab t, const uint32_t *__restrict__ rank2ix, const utree_result *__restrict__ res,
                                                         const uint64_t *__restrict__ tally, uint32_t n, uint32_t per_block, uint32_t *__restrict__ key) {
    __shared__ RdLds s;
    const uint32_t n_dense = t.n_labels < RD_DENSE ? t.n_labels : RD_DENSE;
    for (uint32_t i = threadIdx.x; i < n_dense; i += RD_BLOCK) s.dense[i] = 0;
    const uint64_t begin = (uint64_t)blockIdx.x * per_block;
    const uint64_t end = begin + per_block < n ? begin + per_block : n;
    for (uint64_t tile = begin; tile < end; tile += RD_TILE) {
        const uint64_t tend = tile + RD_TILE < end ? tile + RD_TILE : end;
        if (threadIdx.x == 0) { s.qn = 0; if (tile == begin) s.q2n = 0; }
        __syncthreads();
        for (uint64_t r0 = tile + threadIdx.x; r0 < tend; r0 += RD_UNROLL * RD_BLOCK) {
            uint32_t lab[RD_UNROLL], fnd[RD_UNROLL];
            int32_t cut[RD_UNROLL];
#pragma unroll
            for (int u = 0; u < RD_UNROLL; ++u) {
                const uint64_t r = r0 + (uint64_t)u * RD_BLOCK;
                lab[u] = 0; cut[u] = -2; fnd[u] = 0;
                if (r < tend) { lab[u] = res[r].label; cut[u] = res[r].cut; fnd[u] = res[r].found; }
            }
#pragma unroll
            for (int u = 0; u < RD_UNROLL; ++u) {
                const uint64_t r = r0 + (uint64_t)u * RD_BLOCK;
                if (!fnd[u]) { if (KEYS && r < tend) key[r] = UTREE_REDIST_KEY_NONE; continue; }
                if (cut[u] == RD_CUT_PENDING) s.q[atomicAdd(&s.qn, 1u)] = (uint32_t)r;     // (at most RD_TILE per round)
                else if (cut[u] == RD_RANK_PENDING) {
                    const uint32_t one = lab[u] < t.n_labels ? rank2ix[lab[u]] : 0xFFFFFFFFu;
                    rd_single(t, s, n_dense, one);
                    if (KEYS) key[r] = rd_key_single(t, one);
                } else {
                    rd_single(t, s, n_dense, lab[u]);     // finished by classify_long_k: one label, already a file-order index
                    if (KEYS) key[r] = rd_key_single(t, lab[u]);
                }
            }
        }
        __syncthreads();
        const uint32_t qn = s.qn;
        for (uint32_t i = threadIdx.x; i < qn; i += RD_UNROLL * RD_BLOCK) rd_listed<KEYS>(t, s, n_dense, rank2ix, res, tally, i, qn, key);
        __syncthreads();
        const uint32_t q2n = s.q2n;
        if (q2n + RD_TILE > RD_Q2 || tend == end) {                 // (the same decision in every thread)
            for (uint32_t i = threadIdx.x; i < q2n; i += RD_BLOCK) rd_multi<KEYS>(t, rank2ix, res, tally, s.q2[i], key);
            __syncthreads();
            if (threadIdx.x == 0) s.q2n = 0;
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_dense; i += RD_BLOCK)
        if (s.dense[i]) rd_add(t.single + i, s.dense[i]);
    if (blockIdx.x == 0 && threadIdx.x == 0) rd_add(t.misc + 0, n);
}

__global__ void __launch_bounds__(256) redist_insert_k(utk_redist_tab t, const unsigned long long *__restrict__ reads,
                                                       const unsigned long long *__restrict__ first, const uint32_t *__restrict__ cnt,
                                                       const uint32_t *__restrict__ labels, uint64_t n_sets) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_sets || !reads[i]) return;
    const uint32_t *p = labels + first[i];
    for (uint32_t j = 0; j < cnt[i]; ++j) if (p[j] >= t.n_labels) { rd_flag(t, UTK_REDIST_F_LABEL); return; }
    if (cnt[i] == 1) { rd_add(t.single + p[0], reads[i]); return; }
    if (!cnt[i]) return;
    FlatSeq seq = {p, 0};
    rd_insert(t, seq, cnt[i], reads[i]);
}

__global__ void __launch_bounds__(256) redist_sum_k(unsigned long long *dst, const unsigned long long *__restrict__ src, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) if (src[i]) dst[i] += src[i];
}

// PASS false: every member gets the set's reads (T0), the sets' reads summed into misc[4]; true: the richest member under `prev`
template <bool PASS>
__global__ void __launch_bounds__(256) redist_pass_k(utk_redist_tab t, const unsigned long long *__restrict__ prev, unsigned long long *next) {
    unsigned long long amb = 0;
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s <= t.mask; s += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long k = t.slots[2 * s];
        if (k == RD_FREE) continue;
        const unsigned long long reads = t.slots[2 * s + 1];
        const uint32_t *a = t.arena + (k >> 32);
        const uint32_t n = (uint32_t)k;
        if (!PASS) {
            for (uint32_t i = 0; i < n; ++i) rd_add(next + a[i], reads);
            amb += reads;
        } else {
            uint32_t best = a[0];
            unsigned long long tb = prev[best];
            for (uint32_t i = 1; i < n; ++i) {
                const uint32_t l = a[i];
                const unsigned long long tl = prev[l];
                if (tl > tb || (tl == tb && l < best)) { best = l; tb = tl; }
            }
            rd_add(next + best, reads);
        }
    }
    if (!PASS) {
        for (int d = 32; d; d >>= 1) amb += __shfl_down(amb, d);
        if ((threadIdx.x & 63u) == 0 && amb) rd_add(t.misc + 4, amb);
    }
}

// win(set, tally) and the set's size, per slot: what redist_pass_k<true> evaluates, kept instead of counted (free slots: ~0 and 0)
__global__ void __launch_bounds__(256) redist_winner_k(utk_redist_tab t, const unsigned long long *__restrict__ tally, uint32_t *__restrict__ win,
                                                       uint32_t *__restrict__ ncand) {
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s <= t.mask; s += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long k = t.slots[2 * s];
        if (k == RD_FREE) { win[s] = 0xFFFFFFFFu; ncand[s] = 0; continue; }
        const uint32_t *a = t.arena + (k >> 32);
        const uint32_t n = (uint32_t)k;
        uint32_t best = a[0];
        unsigned long long tb = tally[best];
        for (uint32_t i = 1; i < n; ++i) {
            const uint32_t l = a[i];
            const unsigned long long tl = tally[l];
            if (tl > tb || (tl == tb && l < best)) { best = l; tb = tl; }
        }
        win[s] = best; ncand[s] = n;
    }
}

// one thread per read, a gather by key: every comparison stands in front of the load it guards, a bad key reads nothing
__global__ void __launch_bounds__(256) redist_assign_k(utk_redist_tab t, const uint32_t *__restrict__ win, const uint32_t *__restrict__ ncand,
                                                       const uint32_t *__restrict__ key, uint64_t n, uint32_t *__restrict__ label,
                                                       uint32_t *__restrict__ ncand_out) {
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t k = key[r];
        uint32_t l = 0xFFFFFFFFu, c = 0xFFFFFFFFu;
        if (k == UTREE_REDIST_KEY_NONE) c = 0;
        else if (k < 0x80000000u) { if (k < t.n_labels) { l = k; c = 1; } }
        else {
            const uint32_t s = k & 0x7FFFFFFFu;
            if (s <= t.mask && t.slots[2 * (size_t)s] != RD_FREE) { l = win[s]; c = ncand[s]; }
        }
        label[r] = l;
        if (ncand_out) ncand_out[r] = c;
    }
}

__global__ void __launch_bounds__(256) redist_changes_k(const unsigned long long *__restrict__ prev, const unsigned long long *__restrict__ next, uint32_t n,
                                                        unsigned long long *out) {
    unsigned long long c = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        c += next[i] > prev[i] ? next[i] - prev[i] : prev[i] - next[i];
    for (int d = 32; d; d >>= 1) c += __shfl_down(c, d);
    if ((threadIdx.x & 63u) == 0 && c) rd_add(out, c);
}

static inline uint32_t grid_for(uint64_t n, uint32_t block, uint32_t most) {
    uint64_t g = (n + block - 1) / block;
    return (uint32_t)(g < 1 ? 1 : g > most ? most : g);
}

extern "C" int utk_redist_add(const utk_redist_tab *t, const utk_image *im, const utree_result *d_res, const utk_workspace *ws, uint32_t n_reads,
                              int n_cu, uint32_t *d_key, void *stream) {
    if (!n_reads) return 0;
    // one workgroup per CU at most (the LDS counters take 112 KiB of its 160), each over a contiguous run of records
    uint32_t blocks = (uint32_t)(n_cu > 0 ? n_cu : 256);
    const uint32_t min_per = 4u * RD_BLOCK;
    if ((n_reads + min_per - 1) / min_per < blocks) blocks = (n_reads + min_per - 1) / min_per;
    const uint32_t per = (uint32_t)(((uint64_t)n_reads + blocks - 1) / blocks);
    if (d_key)
        hipLaunchKernelGGL(redist_add_k<true>, dim3(blocks), dim3(RD_BLOCK), 0, (hipStream_t)stream, *t, im->rank2ix, d_res, ws->tally, n_reads, per, d_key);
    else
        hipLaunchKernelGGL(redist_add_k<false>, dim3(blocks), dim3(RD_BLOCK), 0, (hipStream_t)stream, *t, im->rank2ix, d_res, ws->tally, n_reads, per,
                           (uint32_t *)NULL);
    return (int)hipGetLastError();
}

extern "C" int utk_redist_insert(const utk_redist_tab *t, const unsigned long long *d_reads, const unsigned long long *d_first, const uint32_t *d_n,
                                 const uint32_t *d_labels, uint64_t n_sets, void *stream) {
    if (!n_sets) return 0;
    hipLaunchKernelGGL(redist_insert_k, dim3((uint32_t)((n_sets + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *t, d_reads, d_first, d_n, d_labels,
                       n_sets);
    return (int)hipGetLastError();
}

extern "C" int utk_redist_sum(unsigned long long *dst, const unsigned long long *src, uint64_t n, void *stream) {
    if (!n) return 0;
    hipLaunchKernelGGL(redist_sum_k, dim3(grid_for(n, 256, 4096)), dim3(256), 0, (hipStream_t)stream, dst, src, n);
    return (int)hipGetLastError();
}

extern "C" int utk_redist_tally0(const utk_redist_tab *t, unsigned long long *tally, void *stream) {
    hipError_t e = hipMemcpyAsync(tally, t->single, (size_t)t->n_labels * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemsetAsync(t->misc + 4, 0, 8, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(redist_pass_k<false>, dim3(grid_for((uint64_t)t->mask + 1, 256, 4096)), dim3(256), 0, (hipStream_t)stream, *t,
                       (const unsigned long long *)NULL, tally);
    return (int)hipGetLastError();
}

extern "C" int utk_redist_pass(const utk_redist_tab *t, const unsigned long long *prev, unsigned long long *next, void *stream) {
    hipError_t e = hipMemcpyAsync(next, t->single, (size_t)t->n_labels * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemsetAsync(t->misc + 3, 0, 8, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(redist_pass_k<true>, dim3(grid_for((uint64_t)t->mask + 1, 256, 4096)), dim3(256), 0, (hipStream_t)stream, *t, prev, next);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(redist_changes_k, dim3(grid_for(t->n_labels, 256, 1024)), dim3(256), 0, (hipStream_t)stream, prev, next, t->n_labels, t->misc + 3);
    return (int)hipGetLastError();
}

extern "C" int utk_redist_winner(const utk_redist_tab *t, const unsigned long long *tally, uint32_t *d_win, uint32_t *d_ncand, void *stream) {
    hipLaunchKernelGGL(redist_winner_k, dim3(grid_for((uint64_t)t->mask + 1, 256, 4096)), dim3(256), 0, (hipStream_t)stream, *t, tally, d_win, d_ncand);
    return (int)hipGetLastError();
}

extern "C" int utk_redist_assign(const utk_redist_tab *t, const uint32_t *d_win, const uint32_t *d_ncand, const uint32_t *d_key, uint64_t n,
                                 uint32_t *d_label, uint32_t *d_ncand_out, void *stream) {
    if (!n) return 0;
    hipLaunchKernelGGL(redist_assign_k, dim3(grid_for(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, *t, d_win, d_ncand, d_key, n, d_label, d_ncand_out);
    return (int)hipGetLastError();
}
