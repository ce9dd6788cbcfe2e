// inspect_kernels.hip -- the device side of utree_inspect_file (`utree-inspect`).  gfx950 only.
//
// The whole database is resident as three sorted arrays -- the words' low halves, their high halves (W = 16) and the universe label ids --
// which the merge's passes (merge_kernels.hip: utk_inspect_pass) fill in ascending order.  Then:
//
//   directory_k<W>     one thread per value c of the words' top 24 bits: dir[c] = the first node whose top bits are >= c (a binary search),
//                      dir[2^24] = n.  Cell c is [dir[c], dir[c + 1]).
//   neighbours_k<W>    ONE LANE PER NODE.  A lane walks the k base positions of its word and looks up the three substitutions of each, the
//                      three searches of a position in lock-step (three loads in flight per lane):
//                        - a position below the directory's bits leaves the word in its own cell: the lane searches the part of that cell on
//                          the neighbour's side of the node, between bounds it loaded once.  Consecutive lanes hold consecutive nodes, so
//                          these probes of a wavefront fall into the few lines the wavefront's own loads have just brought in;
//                        - a position inside the top 24 bits (12 of the 32 at k = 32) lands in another cell: two directory entries, then
//                          the search of that cell.  The nodes of a wavefront mostly share a cell, so at one position they all probe one
//                          other cell: measured, the pass fetches about 140-280 bytes per node from HBM.
//                      Each held neighbour under another label is a pair event: it decides the node's class through the universe's
//                      truncation tables (x is an ancestor of y when x is y cut before its (depth(x) + 1)-th ';') and adds to the pair
//                      table.  A lane adds up a run of equal pairs before it touches the table.  The class bumps fig[class][label], a
//                      wavefront of one slot adding once.
//   pair table         open addressing over keys label << 24 | neighbour's label (48 bits), 2 slots per distinct pair of capacity; a
//                      slot is claimed with one compare-and-swap, counted with one add.  More distinct pairs than the capacity set the
//                      overflow word and every later add returns at once: probing is bounded by the slots, nothing is written beyond them.
//   pairs_collect_k    the filled slots, compacted for the host (in no order: the host sorts them by text).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include "utree_internal.h"
#include "inspect_gpu.h"

extern "C" void utree_dev_set_hip_error(int err, const char *what);

namespace {

constexpr int BLOCK = 256;
constexpr uint32_t CELLS = 1u << 24;
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint64_t EMPTY = ~0ull;                           // no key: keys have 48 bits
constexpr uint32_t CL_ISOLATED = 0, CL_SAME = 1, CL_LINEAGE = 2, CL_CONFLICT = 3;
static_assert(UTK_INSPECT_FIGURES == 4, "fig[] holds one row of n_u counters per class");

// bases of a word (W = 4: only the low 32 bits carry the 16-mer) and the bit at which its top 24 bits start
template <int W> struct geom {
    static constexpr int K = W == 4 ? 16 : 4 * W;
    static constexpr int CELL_SHIFT = W == 4 ? 8 : W == 8 ? 40 : 104;
};

template <int W> __device__ __forceinline__ uint32_t cell_of(uint64_t hi, uint64_t lo) {
    return W == 4 ? (uint32_t)(lo >> 8) & 0xFFFFFFu : W == 8 ? (uint32_t)(lo >> 40) : (uint32_t)(hi >> 40);
}

template <int W>
__global__ __launch_bounds__(BLOCK) void directory_k(const uint64_t *__restrict__ lo, const uint64_t *__restrict__ hi, uint32_t n,
                                                     uint32_t *__restrict__ dir) {
    const uint64_t c = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (c > CELLS) return;
    uint32_t a = 0, b = n;                                  // the first node whose cell is >= c
    while (a < b) {
        const uint32_t m = a + ((b - a) >> 1);
        if (cell_of<W>(W == 16 ? hi[m] : 0, W == 16 ? 0 : lo[m]) < c) a = m + 1; else b = m;
    }
    dir[c] = a;
}

struct lineage_tabs { const uint32_t *depth, *toff, *tids; };
// x's text is y's cut before a ';': trunc_ids[trunc_off[y] + m - 1] is y cut before its m-th ';', and such a cut holds m - 1 of them
__device__ __forceinline__ bool ancestor(const lineage_tabs &T, uint32_t x, uint32_t y) {
    const uint32_t dx = T.depth[x];
    return dx < T.depth[y] && T.tids[T.toff[y] + dx] == x;
}

struct pair_table {
    unsigned long long *keys, *counts;                      // counts: NULL when the pairs are only counted
    uint64_t mask, cap;
    unsigned long long *n_distinct;
    uint32_t *overflow;
};

__device__ __forceinline__ void pair_add(const pair_table &P, uint64_t key, uint32_t n) {
    if (__atomic_load_n(P.overflow, __ATOMIC_RELAXED)) return;
    uint64_t h = ((key * 0x9E3779B97F4A7C15ull) >> 32) & P.mask;
    for (uint64_t step = 0; step <= P.mask; ++step, h = (h + 1) & P.mask) {
        unsigned long long k = __atomic_load_n(&P.keys[h], __ATOMIC_RELAXED);
        if (k == EMPTY) {
            k = atomicCAS(&P.keys[h], (unsigned long long)EMPTY, (unsigned long long)key);
            if (k == EMPTY) {
                if (atomicAdd(P.n_distinct, 1ull) + 1 > P.cap) { atomicOr(P.overflow, 1u); return; }
                k = key;
            }
        }
        if (k == key) { if (P.counts) atomicAdd(&P.counts[h], (unsigned long long)n); return; }
    }
    atomicOr(P.overflow, 1u);                               // every slot holds another key
}

// ++fig[slot] for every lane that is `on`: neighbours in word order mostly share a label and a class, so a wavefront of one slot adds once
__device__ __forceinline__ void wave_add(bool on, uint32_t slot, unsigned long long *__restrict__ fig) {
    const uint64_t m = __ballot(on);
    if (!m) return;
    const uint32_t lead = (uint32_t)__builtin_ctzll(m);
    const uint32_t slot0 = (uint32_t)__shfl((int)slot, (int)lead);
    const uint64_t same = __ballot(on && slot == slot0);
    if (same == m) { if ((threadIdx.x & 63u) == lead) atomicAdd(&fig[slot0], (unsigned long long)__popcll(m)); }
    else if (on) atomicAdd(&fig[slot], 1ull);
}

// three lower-bound searches in lock-step: j[q] = the index in [a[q], b[q]) of word (thi[q], tlo[q]), or NONE
template <int W>
__device__ __forceinline__ void find3(const uint64_t *__restrict__ lo, const uint64_t *__restrict__ hi, uint32_t (&a)[3], uint32_t (&b)[3],
                                      const uint64_t (&thi)[3], const uint64_t (&tlo)[3], uint32_t (&j)[3]) {
    const uint32_t end[3] = {b[0], b[1], b[2]};
    while ((a[0] < b[0]) | (a[1] < b[1]) | (a[2] < b[2])) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (a[q] < b[q]) {
                const uint32_t m = a[q] + ((b[q] - a[q]) >> 1);
                const uint64_t l = lo[m];
                bool less = l < tlo[q];
                if (W == 16) { const uint64_t h = hi[m]; less = h < thi[q] || (h == thi[q] && less); }
                if (less) a[q] = m + 1; else b[q] = m;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q)
        j[q] = (a[q] < end[q] && lo[a[q]] == tlo[q] && (W != 16 || hi[a[q]] == thi[q])) ? a[q] : NONE;
}

template <int W>
__global__ __launch_bounds__(BLOCK) void neighbours_k(const uint64_t *__restrict__ lo, const uint64_t *__restrict__ hi,
                                                      const uint32_t *__restrict__ lab, uint32_t n, const uint32_t *__restrict__ dir,
                                                      lineage_tabs T, uint32_t n_u, unsigned long long *__restrict__ fig, pair_table P,
                                                      unsigned long long *__restrict__ events) {
    __shared__ unsigned long long s_events;
    if (!threadIdx.x) s_events = 0;
    __syncthreads();
    const uint64_t i64 = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = i64 < n;
    const uint32_t i = (uint32_t)i64;
    uint32_t cls = CL_ISOLATED, u = 0, my_events = 0;
    if (live) {
        const uint64_t wlo = lo[i], whi = W == 16 ? hi[i] : 0;
        u = lab[i];
        const uint32_t c = cell_of<W>(whi, wlo), own_a = dir[c], own_b = dir[c + 1];
        bool held = false, diff = false, conflict = false;
        uint64_t run_key = EMPTY;
        uint32_t run_n = 0;
        for (int p = 0; p < geom<W>::K; ++p) {
            const int bit = 2 * p;
            uint64_t thi[3], tlo[3];
            uint32_t a[3], b[3], j[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                thi[q] = whi; tlo[q] = wlo;
                if (W == 16 && bit >= 64) thi[q] ^= (uint64_t)(q + 1) << (bit - 64); else tlo[q] ^= (uint64_t)(q + 1) << bit;
                if (bit >= geom<W>::CELL_SHIFT) {           // another cell: through the directory
                    const uint32_t c2 = cell_of<W>(thi[q], tlo[q]);
                    a[q] = dir[c2]; b[q] = dir[c2 + 1];
                } else {                                    // its own cell, on the neighbour's side of the node
                    const bool up = (W == 16 && bit >= 64) ? thi[q] > whi : tlo[q] > wlo;
                    a[q] = up ? i + 1 : own_a; b[q] = up ? own_b : i;
                }
            }
            find3<W>(lo, hi, a, b, thi, tlo, j);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                if (j[q] == NONE) continue;
                held = true;
                const uint32_t v = lab[j[q]];
                if (v == u) continue;
                diff = true;
                ++my_events;
                if (!ancestor(T, u, v) && !ancestor(T, v, u)) conflict = true;
                const uint64_t key = ((uint64_t)u << 24) | v;
                if (key == run_key) ++run_n;
                else { if (run_n) pair_add(P, run_key, run_n); run_key = key; run_n = 1; }
            }
        }
        if (run_n) pair_add(P, run_key, run_n);
        cls = conflict ? CL_CONFLICT : diff ? CL_LINEAGE : held ? CL_SAME : CL_ISOLATED;
    }
    wave_add(live, cls * n_u + u, fig);
    if (my_events) atomicAdd(&s_events, (unsigned long long)my_events);
    __syncthreads();
    if (!threadIdx.x && s_events) atomicAdd(events, s_events);
}

__global__ __launch_bounds__(BLOCK) void pairs_collect_k(pair_table P, uint64_t slots, unsigned long long *__restrict__ out_keys,
                                                         unsigned long long *__restrict__ out_counts, unsigned long long *__restrict__ n_out,
                                                         uint64_t out_cap) {
    const uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= slots) return;
    const unsigned long long k = P.keys[s];
    if (k == EMPTY) return;
    const unsigned long long at = atomicAdd(n_out, 1ull);
    if (at < out_cap) { out_keys[at] = k; out_counts[at] = P.counts[s]; }
}

template <typename Fn> bool dispatch_w(int W, Fn &&fn) {
    if (W == 4) fn(std::integral_constant<int, 4>{});
    else if (W == 8) fn(std::integral_constant<int, 8>{});
    else if (W == 16) fn(std::integral_constant<int, 16>{});
    else return false;
    return true;
}

#define HK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { utree_dev_set_hip_error((int)e_, "inspect: " #x); rc = e_ == hipErrorOutOfMemory ? UTREE_E_NOMEM : UTREE_E_HIP; goto fail; } } while (0)

template <typename T> hipError_t dmalloc(T **p, uint64_t n) { return hipMalloc((void **)p, (n ? n : 1) * sizeof(T)); }

enum { SC_EVENTS, SC_DISTINCT, SC_OVERFLOW, SC_COLLECTED, N_SC };

}  // namespace

struct utk_inspect_dev {
    utk_inspect_cfg cfg;
    uint64_t *lo, *hi;
    uint32_t *lab, *dir, *depth, *toff, *tids;
    unsigned long long *fig, *keys, *counts, *scal;
    uint64_t slots, distinct;
};

extern "C" {

uint64_t utk_inspect_resident_bytes(uint32_t W, uint64_t n) { return n * (W == 16 ? 20ull : 12ull); }

void utk_inspect_close(utk_inspect_dev *D) {
    if (!D) return;
    (void)hipSetDevice(D->cfg.device);
    (void)hipDeviceSynchronize();
    void *dev[] = {D->lo, D->hi, D->lab, D->dir, D->depth, D->toff, D->tids, D->fig, D->keys, D->counts, D->scal};
    for (void *p : dev) if (p) (void)hipFree(p);
    free(D);
}

int utk_inspect_open(const utk_inspect_cfg *cfg, utk_inspect_dev **out) {
    int rc = UTREE_OK;
    if (!dispatch_w((int)cfg->W, [](auto) {}) || cfg->n >= 0xFFFFFFFFull || !cfg->pair_cap || cfg->pair_cap > (1ull << 28) || cfg->n_u >= (1u << 24)) return UTREE_E_ARG;
    utk_inspect_dev *D = (utk_inspect_dev *)calloc(1, sizeof *D);
    if (!D) return UTREE_E_NOMEM;
    D->cfg = *cfg;
    D->slots = 64;
    while (D->slots < 2 * cfg->pair_cap) D->slots <<= 1;
    HK(hipSetDevice(cfg->device));
    HK(dmalloc(&D->lo, cfg->n));
    if (cfg->W == 16) HK(dmalloc(&D->hi, cfg->n));
    HK(dmalloc(&D->lab, cfg->n));
    HK(dmalloc(&D->dir, (uint64_t)CELLS + 1));
    HK(dmalloc(&D->depth, cfg->n_u)); HK(dmalloc(&D->toff, (uint64_t)cfg->n_u + 1)); HK(dmalloc(&D->tids, cfg->n_trunc));
    HK(dmalloc(&D->fig, (uint64_t)UTK_INSPECT_FIGURES * cfg->n_u));
    HK(dmalloc(&D->keys, D->slots));
    if (cfg->with_counts) HK(dmalloc(&D->counts, D->slots));
    HK(dmalloc(&D->scal, (uint64_t)N_SC));
    if (cfg->n_u) HK(hipMemcpy(D->depth, cfg->h_depth, 4ull * cfg->n_u, hipMemcpyHostToDevice));
    HK(hipMemcpy(D->toff, cfg->h_trunc_off, 4ull * (cfg->n_u + 1ull), hipMemcpyHostToDevice));
    if (cfg->n_trunc) HK(hipMemcpy(D->tids, cfg->h_trunc_ids, 4ull * cfg->n_trunc, hipMemcpyHostToDevice));
    HK(hipMemset(D->fig, 0, 8ull * UTK_INSPECT_FIGURES * (cfg->n_u ? cfg->n_u : 1)));
    HK(hipMemset(D->keys, 0xFF, 8ull * D->slots));
    if (D->counts) HK(hipMemset(D->counts, 0, 8ull * D->slots));
    HK(hipMemset(D->scal, 0, 8ull * N_SC));
    HK(hipDeviceSynchronize());
    *out = D;
    return UTREE_OK;
fail:
    utk_inspect_close(D);
    return rc;
}

void utk_inspect_arrays(utk_inspect_dev *D, uint64_t **d_lo, uint64_t **d_hi, uint32_t **d_lab) { *d_lo = D->lo; *d_hi = D->hi; *d_lab = D->lab; }

int utk_inspect_neighbours(utk_inspect_dev *D, uint64_t n, utk_inspect_out *out) {
    int rc = UTREE_OK;
    unsigned long long h_sc[N_SC] = {0};
    memset(out, 0, sizeof *out);
    if (n > D->cfg.n) return UTREE_E_ARG;
    if (!n) return UTREE_OK;
    HK(hipSetDevice(D->cfg.device));
    {
        const double t0 = now_s();
        const lineage_tabs T = {D->depth, D->toff, D->tids};
        const pair_table P = {D->keys, D->counts, D->slots - 1, D->cfg.pair_cap, D->scal + SC_DISTINCT, (uint32_t *)(D->scal + SC_OVERFLOW)};
        const unsigned gd = (unsigned)(((uint64_t)CELLS + 1 + BLOCK - 1) / BLOCK), gn = (unsigned)((n + BLOCK - 1) / BLOCK);
        dispatch_w((int)D->cfg.W, [&](auto w) {
            constexpr int WV = decltype(w)::value;
            directory_k<WV><<<dim3(gd), dim3(BLOCK)>>>(D->lo, D->hi, (uint32_t)n, D->dir);
            neighbours_k<WV><<<dim3(gn), dim3(BLOCK)>>>(D->lo, D->hi, D->lab, (uint32_t)n, D->dir, T, D->cfg.n_u, D->fig, P, D->scal + SC_EVENTS);
        });
        HK(hipGetLastError());
        HK(hipMemcpy(h_sc, D->scal, 8ull * N_SC, hipMemcpyDeviceToHost));
        HK(hipDeviceSynchronize());
        out->seconds = now_s() - t0;
    }
    out->pair_events = h_sc[SC_EVENTS];
    out->distinct_pairs = h_sc[SC_DISTINCT];
    out->overflow = h_sc[SC_OVERFLOW] != 0;
    D->distinct = out->overflow ? 0 : out->distinct_pairs;
fail:
    if (rc) (void)hipDeviceSynchronize();
    return rc;
}

int utk_inspect_figures(utk_inspect_dev *D, uint64_t *h_fig) {
    int rc = UTREE_OK;
    HK(hipSetDevice(D->cfg.device));
    if (D->cfg.n_u) HK(hipMemcpy(h_fig, D->fig, 8ull * UTK_INSPECT_FIGURES * D->cfg.n_u, hipMemcpyDeviceToHost));
fail:
    return rc;
}

int utk_inspect_pairs(utk_inspect_dev *D, uint64_t *h_keys, uint64_t *h_counts) {
    int rc = UTREE_OK;
    unsigned long long *d_keys = nullptr, *d_counts = nullptr, got = 0;
    if (!D->counts) return UTREE_E_ARG;
    if (!D->distinct) return UTREE_OK;
    HK(hipSetDevice(D->cfg.device));
    HK(dmalloc(&d_keys, D->distinct)); HK(dmalloc(&d_counts, D->distinct));
    {
        const pair_table P = {D->keys, D->counts, D->slots - 1, D->cfg.pair_cap, D->scal + SC_DISTINCT, (uint32_t *)(D->scal + SC_OVERFLOW)};
        HK(hipMemset(D->scal + SC_COLLECTED, 0, 8));
        pairs_collect_k<<<dim3((unsigned)((D->slots + BLOCK - 1) / BLOCK)), dim3(BLOCK)>>>(P, D->slots, d_keys, d_counts, D->scal + SC_COLLECTED, D->distinct);
        HK(hipGetLastError());
        HK(hipMemcpy(&got, D->scal + SC_COLLECTED, 8, hipMemcpyDeviceToHost));
        if (got != D->distinct) { rc = UTREE_E_HIP; utree_dev_set_hip_error(0, "inspect: the pair table holds another number of pairs than it counted"); goto fail; }
        HK(hipMemcpy(h_keys, d_keys, 8ull * D->distinct, hipMemcpyDeviceToHost));
        HK(hipMemcpy(h_counts, d_counts, 8ull * D->distinct, hipMemcpyDeviceToHost));
    }
fail:
    if (rc) (void)hipDeviceSynchronize();
    if (d_keys) (void)hipFree(d_keys);
    if (d_counts) (void)hipFree(d_counts);
    return rc;
}

}  // extern "C"
