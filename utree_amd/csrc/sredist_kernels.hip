// sredist_kernels.hip -- the candidate sets of a batch of multiplexed reads counted per sample, and the redistribution of every sample's
// ambiguous reads within that sample (utree_sredist_*, sredist.c).
//
// sredist_add_k runs where redist_add_k runs -- between a batch's classify kernels and vote_k, while a read's (rank, count) list still stands
// in the workspace -- and reads the names samples_add_k reads.  For a read it interns the sample id (samples_dev.hpp), finds the labels tied for
// the highest count, and counts the cell (sample slot, set handle): the handle of a single candidate is the label itself, several candidates
// are a set of the table redist_kernels.hip keeps (redist_dev.hpp) and the handle its slot.  What the two kernels learned is kept:
//   ids      only a lane whose id is neither its predecessor lane's nor the one it had 1024 records before goes to the id table (sm_resolve)
//   counts   a hash table of cells in the workgroup's LDS (SmCells), runs of equal keys carried in registers; a read without a hit is a cell of its
//            own there and leaves it for uncl[]
//   queues   a read with a list goes on the workgroup's queue with its sample slot; that queue is dealt out over all lanes, which find each
//            list's tied maximum; several candidates put the read on a second queue, dealt out when it may not hold another round's reads: no
//            wavefront runs the set table's probe chain for a few of its lanes
// Nothing is dropped silently: every condition the two tables flag is flagged in their error words here too.
//
// The solver (sredist_tally0_k / sredist_init_k / sredist_pass_k / sredist_changes_k) runs over the cells the host laid out flat (sredist.h:
// utk_sredist_problem): tallies only for the (sample, label) pairs that occur, one thread per cell, one no-return atomic each; the changes are
// reduced per sample -- a wavefront whose indices lie in one sample adds one word -- into one word per active sample.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sredist.h"
#include "redist_dev.hpp"
#include "samples_dev.hpp"

#define SR_BLOCK 1024
#define SR_UNROLL 4
static_assert(SR_UNROLL == RD_UNROLL, "sredist_add_k deals its queue out in rd_scan_listed's steps");
#define SR_TILE 4096u                      // reads a workgroup takes per round = the capacity of its queue of listed reads (a 12-bit position)
#define SR_Q2 8192u                        // capacity of its queue of reads with several candidates
#define SR_HSLOTS 4096u                    // LDS hash slots: 32 KiB of keys + 16 KiB of counts
#define SR_UNCL 0xFFFFFFFFu                // the handle of a sample's reads without a hit, in LDS only

struct SrLds {
    SmCells<SR_HSLOTS> cells;
    uint32_t q[SR_TILE];                   // position in the round | sample slot << 12
    uint2 q2[SR_Q2];                       // {record, sample slot}
    uint32_t qn, q2n, flags;
};

__device__ __forceinline__ uint64_t sr_key(uint32_t slot, uint32_t handle) { return (uint64_t)slot << 32 | handle; }

// cnt reads of a cell into the device tables: the sample's reads, then its unclassified reads or the cell's slot
__device__ void sr_global_add(const utk_sredist_tab &t, uint64_t key, uint32_t cnt) {
    const uint32_t slot = (uint32_t)(key >> 32);
    sm_add(t.s.reads + slot, cnt);
    if ((uint32_t)key == SR_UNCL) { sm_add(t.s.uncl + slot, cnt); return; }
    sm_cell_add(t.s, key, cnt);
}

__device__ void sr_lds_add(SrLds &s, const utk_sredist_tab &t, uint64_t key, uint32_t cnt) {
    s.cells.add(key, cnt, [&](uint64_t k, uint32_t c) { sr_global_add(t, k, c); });
}

// one read of sample `slot` whose only candidate is the file-order index `one`
__device__ __forceinline__ void sr_single(SrLds &s, const utk_sredist_tab &t, uint32_t slot, uint32_t one) {
    if (one >= t.r.n_labels) { rd_flag(t.r, UTK_REDIST_F_LABEL); return; }
    sr_lds_add(s, t, sr_key(slot, UTK_SREDIST_ONE | one), 1u);
}

// RD_UNROLL queued reads per thread (redist_dev.hpp: rd_scan_listed), each with the sample slot its queue entry carries
__device__ void sr_listed(const utk_sredist_tab &t, SrLds &s, const uint32_t *__restrict__ rank2ix, const utree_result *__restrict__ res,
                          const uint64_t *__restrict__ tally, uint64_t tile, uint32_t first, uint32_t qn) {
    rd_scan_listed<SR_BLOCK>(t.r, rank2ix, res, tally, first, qn,
                             [&](uint32_t i, uint32_t &r, uint32_t &slot) { const uint32_t e = s.q[i]; r = (uint32_t)(tile + (e & (SR_TILE - 1u))); slot = e >> 12; },
                             [&](uint32_t slot, uint32_t one) { sr_single(s, t, slot, one); },
                             [&](uint32_t r, uint32_t slot) { s.q2[atomicAdd(&s.q2n, 1u)] = make_uint2(r, slot); });
}

// a queued read with several candidates: its set into the table, its cell counted
__device__ void sr_multi(const utk_sredist_tab &t, SrLds &s, const uint32_t *__restrict__ rank2ix, const utree_result *__restrict__ res,
                         const uint64_t *__restrict__ tally, uint2 q) {
    TiedSeq seq;
    const uint32_t ties = rd_scan_tied(t.r, rank2ix, res, tally, q.x, seq);
    if (ties < 2) { rd_flag(t.r, UTK_REDIST_F_LABEL); return; }       // (sr_listed queued it for having more: never dropped silently)
    const uint32_t set = rd_insert(t.r, seq, ties, 0ull);
    if (set != RD_NO_SLOT) sr_lds_add(s, t, sr_key(q.y, set), 1u);
}

__global__ void __launch_bounds__(SR_BLOCK) sredist_add_k(utk_sredist_tab t, const uint32_t *__restrict__ rank2ix, const utree_result *__restrict__ res,
                                                          const uint64_t *__restrict__ tally, const uint8_t *__restrict__ text, uint64_t text_bytes,
                                                          const uint32_t *__restrict__ name_off, const uint32_t *__restrict__ name_len, uint32_t n,
                                                          uint32_t per_block) {
    __shared__ SrLds s;
    s.cells.init(threadIdx.x, SR_BLOCK);
    if (threadIdx.x == 0) { s.flags = 0; s.q2n = 0; }

    const uint64_t begin = (uint64_t)blockIdx.x * per_block;
    const uint64_t end = begin + per_block < n ? begin + per_block : n;
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t run = SM_KEY_FREE;
    uint32_t run_n = 0, flags = 0;
    SmPrev pv;
    for (uint64_t tile = begin; tile < end; tile += SR_TILE) {                     // (the same trips in every lane: sm_resolve needs them all)
        const uint64_t tend = tile + SR_TILE < end ? tile + SR_TILE : end;
        if (threadIdx.x == 0) s.qn = 0;
        __syncthreads();
        uint32_t off[SR_UNROLL], nlen[SR_UNROLL], lab[SR_UNROLL], fnd[SR_UNROLL];
        int32_t cut[SR_UNROLL];
        bool ok[SR_UNROLL];
#pragma unroll
        for (int u = 0; u < SR_UNROLL; ++u) {                                      // all loads first: four records in flight per thread
            const uint64_t r = tile + (uint64_t)u * SR_BLOCK + threadIdx.x;
            ok[u] = r < tend; off[u] = 0; nlen[u] = 0; lab[u] = 0; cut[u] = -2; fnd[u] = 0;
            if (ok[u]) { off[u] = name_off[r]; nlen[u] = name_len[r]; lab[u] = res[r].label; cut[u] = res[r].cut; fnd[u] = res[r].found; }
        }
#pragma unroll
        for (int u = 0; u < SR_UNROLL; ++u) {
            uint32_t slot;
            const bool valid = sm_resolve(t.s, text, text_bytes, off[u], nlen[u], ok[u], lane, pv, flags, slot);
            uint64_t key = SM_KEY_FREE;
            if (!valid || slot == SM_NONE) {}
            else if (!fnd[u]) key = sr_key(slot, SR_UNCL);
            else if (cut[u] == RD_CUT_PENDING) s.q[atomicAdd(&s.qn, 1u)] = ((uint32_t)u * SR_BLOCK + threadIdx.x) | (slot << 12);   // (at most SR_TILE per round)
            else {
                // one distinct label: a rank the vote has yet to turn into an index, or -- finished by classify_long_k -- a file-order index
                const uint32_t one = cut[u] == RD_RANK_PENDING ? (lab[u] < t.r.n_labels ? rank2ix[lab[u]] : 0xFFFFFFFFu) : lab[u];
                if (one >= t.r.n_labels) flags |= 0x80000000u;
                else key = sr_key(slot, UTK_SREDIST_ONE | one);
            }
            if (key != SM_KEY_FREE) {
                if (key == run) ++run_n;
                else { sr_lds_add(s, t, run, run_n); run = key; run_n = 1; }
            }
        }
        __syncthreads();
        const uint32_t qn = s.qn;
        for (uint32_t i = threadIdx.x; i < qn; i += SR_UNROLL * SR_BLOCK) sr_listed(t, s, rank2ix, res, tally, tile, i, qn);
        __syncthreads();
        const uint32_t q2n = s.q2n;
        if (q2n + SR_TILE > SR_Q2 || tend == end) {                               // (the same decision in every thread)
            for (uint32_t i = threadIdx.x; i < q2n; i += SR_BLOCK) sr_multi(t, s, rank2ix, res, tally, s.q2[i]);
            __syncthreads();
            if (threadIdx.x == 0) s.q2n = 0;
        }
    }
    if (run != SM_KEY_FREE) sr_lds_add(s, t, run, run_n);
    if (flags) atomicOr(&s.flags, flags);
    __syncthreads();

    s.cells.flush(threadIdx.x, SR_BLOCK, [&](uint64_t k, uint32_t c) { sr_global_add(t, k, c); });
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0) sm_add(t.s.misc + 0, n);
        if (s.flags & 0x7FFFFFFFu) sm_flag(t.s, s.flags & 0x7FFFFFFFu);
        if (s.flags & 0x80000000u) rd_flag(t.r, UTK_REDIST_F_LABEL);
    }
}

// ---- sets, ids and counts given on the host (utree_sredist_insert, utree_sredist_merge) ----------------------------------------------------
__global__ void __launch_bounds__(256) sredist_insert_ids_k(utk_sredist_tab t, const uint8_t *__restrict__ ids, const uint64_t *__restrict__ id_off,
                                                            const unsigned long long *__restrict__ reads, const unsigned long long *__restrict__ uncl,
                                                            uint32_t n_samples, uint32_t *slot_of, unsigned long long n_reads) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) sm_add(t.s.misc + 0, n_reads);
    if (i >= n_samples) return;
    const uint32_t slot = sm_intern(t.s, ids + id_off[i], (uint32_t)(id_off[i + 1] - id_off[i]));
    slot_of[i] = slot;
    if (slot == SM_NONE) return;
    if (reads[i]) sm_add(t.s.reads + slot, reads[i]);
    if (uncl[i]) sm_add(t.s.uncl + slot, uncl[i]);
}

__global__ void __launch_bounds__(256) sredist_insert_cells_k(utk_sredist_tab t, const uint32_t *__restrict__ slot_of, uint32_t n_samples,
                                                              const utk_sredist_cell *__restrict__ cells, const uint32_t *__restrict__ labels,
                                                              uint64_t n_cells) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_cells) return;
    const utk_sredist_cell c = cells[i];
    if (!c.reads || !c.n) return;
    if (c.sample >= n_samples) { sm_flag(t.s, UTK_SAMPLES_F_NAME); return; }
    const uint32_t slot = slot_of[c.sample];
    if (slot == SM_NONE) return;                           // (the id found no room: flagged)
    const uint32_t *p = labels + c.first;
    uint32_t handle;
    if (c.n == 1) {
        if (p[0] >= t.r.n_labels) { rd_flag(t.r, UTK_REDIST_F_LABEL); return; }
        handle = UTK_SREDIST_ONE | p[0];
    } else {
        FlatSeq seq = {p, 0};
        handle = rd_insert(t.r, seq, c.n, 0ull);
        if (handle == RD_NO_SLOT) return;
    }
    sm_cell_add(t.s, sr_key(slot, handle), c.reads);
}

// ---- the solver ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) sredist_tally0_k(utk_sredist_problem p, unsigned long long *tally) {
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < p.n_cells; c += (uint64_t)gridDim.x * blockDim.x) {
        const utk_sredist_cell e = p.cells[c];
        const uint32_t *m = p.member + e.first;
        for (uint32_t i = 0; i < e.n; ++i) rd_add(tally + m[i], e.reads);
    }
}

// next = 0 where the sample is evaluated in the pass that follows, its frozen tally where it has stopped
__global__ void __launch_bounds__(256) sredist_init_k(utk_sredist_problem p, const unsigned long long *__restrict__ prev, unsigned long long *next, int all) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.n_tally; i += (uint64_t)gridDim.x * blockDim.x)
        next[i] = all || p.act[p.seg[i]] != 0xFFFFFFFFu ? 0ull : prev[i];
}

__global__ void __launch_bounds__(256) sredist_pass_k(utk_sredist_problem p, const unsigned long long *__restrict__ prev, unsigned long long *next, int all) {
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < p.n_cells; c += (uint64_t)gridDim.x * blockDim.x) {
        const utk_sredist_cell e = p.cells[c];
        if (!all && p.act[e.sample] == 0xFFFFFFFFu) continue;
        const uint32_t *m = p.member + e.first;
        uint32_t best = m[0];
        unsigned long long tb = prev[best];
        for (uint32_t i = 1; i < e.n; ++i) {
            const uint32_t l = m[i];
            const unsigned long long tl = prev[l];
            if (tl > tb || (tl == tb && l < best)) { best = l; tb = tl; }
        }
        rd_add(next + best, e.reads);
    }
}

// changes[act[s]] += sum over s's tally indices of |next - prev|: a wavefront whose 64 indices lie in one sample adds one word
__global__ void __launch_bounds__(256) sredist_changes_k(utk_sredist_problem p, const unsigned long long *__restrict__ prev,
                                                         const unsigned long long *__restrict__ next, unsigned long long *changes) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < p.n_tally; i0 += stride) {       // (i0: the wavefront's first index)
        const uint64_t i = i0 + (threadIdx.x & 63u);
        uint32_t a = 0xFFFFFFFFu;
        unsigned long long d = 0;
        if (i < p.n_tally) {
            a = p.act[p.seg[i]];
            if (a != 0xFFFFFFFFu) d = next[i] > prev[i] ? next[i] - prev[i] : prev[i] - next[i];
        }
        const uint64_t moved = __ballot(d != 0);
        if (!moved) continue;                                              // (the same in every lane)
        const uint32_t af = (uint32_t)__shfl((int)a, __ffsll((long long)moved) - 1);
        if (__all(!d || a == af)) {
            unsigned long long sum = d;
            for (int k = 32; k; k >>= 1) sum += __shfl_down(sum, k);
            if ((threadIdx.x & 63u) == 0) rd_add(changes + af, sum);
        } else if (d) rd_add(changes + a, d);
    }
}

static inline uint32_t grid_for(uint64_t n, uint32_t block, uint32_t most) {
    uint64_t g = (n + block - 1) / block;
    return (uint32_t)(g < 1 ? 1 : g > most ? most : g);
}

extern "C" int utk_sredist_add(const utk_sredist_tab *t, const utk_image *im, const utree_result *d_res, const utk_workspace *ws, const uint8_t *d_text,
                               uint64_t text_bytes, const uint32_t *d_name_off, const uint32_t *d_name_len, uint32_t n, int n_cu, void *stream) {
    if (!n) return 0;
    // one workgroup per CU (its LDS tables and queues take 128 KiB of the CU's 160), each over a contiguous run of records; small batches take fewer
    uint32_t blocks = (uint32_t)(n_cu > 0 ? n_cu : 256);
    const uint32_t min_per = 4u * SR_TILE;
    if ((n + min_per - 1) / min_per < blocks) blocks = (n + min_per - 1) / min_per;
    const uint32_t per = (uint32_t)(((uint64_t)n + blocks - 1) / blocks);
    hipLaunchKernelGGL(sredist_add_k, dim3(blocks), dim3(SR_BLOCK), 0, (hipStream_t)stream, *t, im->rank2ix, d_res, ws->tally, d_text, text_bytes,
                       d_name_off, d_name_len, n, per);
    return (int)hipGetLastError();
}

extern "C" int utk_sredist_insert(const utk_sredist_tab *t, const uint8_t *d_ids, const uint64_t *d_id_off, const unsigned long long *d_reads,
                                  const unsigned long long *d_uncl, uint32_t n_samples, uint32_t *d_slot_of, const utk_sredist_cell *d_cells,
                                  const uint32_t *d_labels, uint64_t n_cells, unsigned long long n_reads, void *stream) {
    hipLaunchKernelGGL(sredist_insert_ids_k, dim3((n_samples + 255) / 256 ? (n_samples + 255) / 256 : 1), dim3(256), 0, (hipStream_t)stream, *t, d_ids,
                       d_id_off, d_reads, d_uncl, n_samples, d_slot_of, n_reads);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !n_cells) return (int)e;
    hipLaunchKernelGGL(sredist_insert_cells_k, dim3((uint32_t)((n_cells + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *t, d_slot_of, n_samples,
                       d_cells, d_labels, n_cells);
    return (int)hipGetLastError();
}

extern "C" int utk_sredist_tally0(const utk_sredist_problem *p, unsigned long long *tally, void *stream) {
    if (!p->n_tally) return 0;
    const hipError_t e = hipMemsetAsync(tally, 0, p->n_tally * 8, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    if (!p->n_cells) return 0;
    hipLaunchKernelGGL(sredist_tally0_k, dim3(grid_for(p->n_cells, 256, 4096)), dim3(256), 0, (hipStream_t)stream, *p, tally);
    return (int)hipGetLastError();
}

extern "C" int utk_sredist_pass(const utk_sredist_problem *p, const unsigned long long *prev, unsigned long long *next, unsigned long long *changes,
                                uint32_t n_active, int all, void *stream) {
    if (!p->n_tally || !p->n_cells) return 0;
    hipError_t e = hipSuccess;
    if (!all && n_active) e = hipMemsetAsync(changes, 0, (size_t)n_active * 8, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(sredist_init_k, dim3(grid_for(p->n_tally, 256, 4096)), dim3(256), 0, (hipStream_t)stream, *p, prev, next, all);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(sredist_pass_k, dim3(grid_for(p->n_cells, 256, 4096)), dim3(256), 0, (hipStream_t)stream, *p, prev, next, all);
    if ((e = hipGetLastError()) != hipSuccess || all) return (int)e;
    hipLaunchKernelGGL(sredist_changes_k, dim3(grid_for(p->n_tally, 256, 1024)), dim3(256), 0, (hipStream_t)stream, *p, prev, next, changes);
    return (int)hipGetLastError();
}
