// merge_kernels.hip -- the device side of utree_merge_files (`utree-merge` / `utree-mergeGG`).  gfx950 only.
//
// A merge is the builder's insert loop (itree.c:242-307) fed the nodes of the inputs, input by input, each in file order.  One pass
// handles one contiguous range of words, of which every input holds one contiguous slice:
//
//   (host)                        each slice: file -> one of two pinned staging buffers -> device, the read of a chunk overlapping the
//                                 upload of the one before; the output goes back the same way (utk_merge_emit)
//   decode_k<W, CTR>              a block stages 256 records (7-20 bytes at odd strides) as coalesced dwords in LDS; a thread takes its
//                                 record from there -> (word hi/lo, event clock (input, node) | universe label); checks the order of the
//                                 words and the label index on the way; the first node that carries a label dates the label
//   rocprim                       stable radix sort by word: slices are laid out in input order, so equal words stay in input order
//   merge_fold_k                  one thread per distinct word replays its run (at most one node per input) with build_fold.hpp's step
//   rocprim::select               words that are not BAD, ascending
//   merge_pack_k                  W+I-byte records as the file holds them + nodes per label
//
// utree_merge_files_edit rides in the value word of that one sort.  A record whose label line the edit drops carries DROP in place of a
// universe id; a MINUS input's record (words only: its slice's label indices are never looked at) is VAL_MINUS.  MINUS slices are laid
// out in front of the regular ones, so the stable sort leaves a MINUS record at the head of its run: such a run feeds nothing, any other
// run folds the records that are not DROP.  With a MINUS input the records fed are known only after the sort, so merge_fold_k dates the
// labels then (has_minus); without one decode_k dates them as before.
//
// utree_compare_files (`utree-compare`) shares the front half -- staging, decode_k, the sort: decode_sort -- with A and B as the two inputs:
//   compare_runs_k                a run is one record or two, A's first: its head adds to the per-label counters same / only_a / only_b /
//                                 left / arrived (a wavefront of one counter adds once) and a changed word appends label A << 24 | label B
//   rocprim                       radix sort of those keys, run-length encoding -> the pass's distinct moves and their counts
//
// utree_inspect_file (`utree-inspect`) shares the same front half with its database as the only input:
//   inspect_append_k              the sorted pass, as (word, universe label), to the end of the resident arrays of inspect_kernels.hip
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <type_traits>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include "utree_internal.h"
#include "merge_gpu.h"
#include "build_fold.hpp"

extern "C" void utree_dev_set_hip_error(int err, const char *what);

namespace {

using utk_fold::ST_BAD;
using utk_fold::ST_SKIP;
using utk_fold::universe;
constexpr int BLOCK = 256;
constexpr int REC_MAX = 20;                                // W = 16, I = 4
constexpr uint32_t ERR_UBT_ORDER = 1u, ERR_IX = 2u, ERR_CTR_ORDER = 4u;
constexpr uint32_t DROP = UTK_MERGE_DROP;                  // in the label field of a value: the record is not fed
constexpr uint64_t VAL_MINUS = ~0ull;                      // no regular record has it: event clocks stay below 2^40 - 1
constexpr uint32_t ROLE_DATES = 0, ROLE_REGULAR = 1, ROLE_MINUS = 2;   // a regular slice whose records date their labels here / in the fold; a MINUS slice
constexpr int STAT_SHARED = 0, STAT_RELABELLED = 1, STAT_BAD = 2, STAT_LABEL_DROPPED = 3, STAT_SUBTRACTED = 4, N_STATS = 8;

struct slice_dev {
    const uint32_t *raw;             // the slice's records, dword aligned, readable up to the dword that holds the last byte
    uint64_t n;
    uint64_t g0;
    const uint32_t *u_of_ix; uint32_t n_lines;
    uint32_t I;
    int has_prev; uint64_t prev_hi, prev_lo;
    const uint64_t *bins; uint32_t p_lo, n_bins; uint64_t first;       // .ctr
    uint32_t role;
};

__device__ __forceinline__ void wave_count(bool pred, unsigned long long *ctr) {
    const uint64_t m = __ballot(pred);
    if (m && (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(m)) atomicAdd(ctr, (unsigned long long)__popcll(m));
}

// the 256 records of this block as dwords into LDS: consecutive lanes load consecutive dwords
__device__ __forceinline__ void stage_records(const uint32_t *__restrict__ raw, uint64_t n, uint32_t rec, uint32_t *s) {
    const uint64_t total_dw = (n * rec + 3) / 4;
    const uint64_t base = (uint64_t)blockIdx.x * (BLOCK / 4) * rec;         // 256 * rec bytes = 64 * rec dwords per block
    for (uint32_t d = threadIdx.x; d < (BLOCK / 4) * rec; d += BLOCK) {
        const uint64_t g = base + d;
        s[d] = g < total_dw ? raw[g] : 0u;
    }
    __syncthreads();
}

__device__ __forceinline__ uint64_t le_bytes(const uint8_t *p, int n) {
    uint64_t v = 0;
    for (int b = 0; b < n; ++b) v |= (uint64_t)p[b] << (8 * b);
    return v;
}

// `.ubt` record: the W-byte little-endian word, then the I-byte index (itree.c:1317-1343)
template <int W> __device__ __forceinline__ void ubt_word(const uint8_t *p, uint64_t &hi, uint64_t &lo) {
    lo = le_bytes(p, W == 4 ? 4 : 8);
    hi = W == 16 ? le_bytes(p + 8, 8) : 0;
}

// `.ctr` record: the low W-3 bytes of the word, then the index; the top 24 bits are the bin the record lies in (itree.c:1301-1313)
template <int W> __device__ __forceinline__ void ctr_word(const uint8_t *p, uint32_t prefix, uint64_t &hi, uint64_t &lo) {
    if (W == 4) { hi = 0; lo = ((uint64_t)prefix << 8) | p[0]; }
    else if (W == 8) { hi = 0; lo = ((uint64_t)prefix << 40) | le_bytes(p, 5); }
    else { lo = le_bytes(p, 8); hi = ((uint64_t)prefix << 40) | le_bytes(p + 8, 5); }
}

// bins[0 .. n_bins] non-decreasing, bins[0] <= node < bins[n_bins]: the q with bins[q] <= node < bins[q + 1]
__device__ __forceinline__ uint32_t bin_of(const uint64_t *__restrict__ bins, uint32_t n_bins, uint64_t node) {
    uint32_t a = 0, b = n_bins;                                             // invariant: bins[a] <= node < bins[b]
    while (b - a > 1) { const uint32_t m = a + ((b - a) >> 1); if (bins[m] <= node) a = m; else b = m; }
    return a;
}

template <int W, bool CTR>
__global__ __launch_bounds__(BLOCK) void decode_k(slice_dev S, uint64_t at, uint64_t *__restrict__ key_lo, uint64_t *__restrict__ key_hi,
                                                  uint64_t *__restrict__ val, unsigned long long *__restrict__ first_time,
                                                  uint32_t *__restrict__ err, unsigned long long *__restrict__ stats) {
    __shared__ uint32_t s_raw[(BLOCK / 4) * REC_MAX];
    __shared__ uint64_t s_lo[BLOCK], s_hi[W == 16 ? BLOCK : 1];
    const uint32_t rec = (CTR ? W - 3 : W) + S.I;
    stage_records(S.raw, S.n, rec, s_raw);
    const uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = j < S.n;
    const uint8_t *p = (const uint8_t *)s_raw + threadIdx.x * rec;
    uint64_t hi = 0, lo = 0;
    if (live) {
        if (CTR) ctr_word<W>(p, S.p_lo + bin_of(S.bins, S.n_bins, S.first + j), hi, lo);
        else ubt_word<W>(p, hi, lo);
    }
    s_lo[threadIdx.x] = lo;
    if (W == 16) s_hi[threadIdx.x] = hi;
    __syncthreads();
    if (!live) return;
    // strictly ascending against the node in front (the reference dumps its trees in order, 399-417; a merge relies on it)
    bool have = true;
    uint64_t phi = 0, plo = 0;
    if (threadIdx.x) { plo = s_lo[threadIdx.x - 1]; if (W == 16) phi = s_hi[threadIdx.x - 1]; }
    else if (j) {
        const uint8_t *q = (const uint8_t *)S.raw + (j - 1) * rec;          // the last record of the block in front
        uint8_t tmp[REC_MAX];
        for (uint32_t b = 0; b < rec; ++b) tmp[b] = q[b];
        if (CTR) ctr_word<W>(tmp, S.p_lo + bin_of(S.bins, S.n_bins, S.first + j - 1), phi, plo);
        else ubt_word<W>(tmp, phi, plo);
    } else { have = S.has_prev != 0; phi = S.prev_hi; plo = S.prev_lo; }
    if (have && !(phi < hi || (phi == hi && plo < lo))) atomicOr(err, CTR ? ERR_CTR_ORDER : ERR_UBT_ORDER);
    key_lo[at + j] = lo;
    if (W == 16) key_hi[at + j] = hi;
    if (S.role == ROLE_MINUS) { val[at + j] = VAL_MINUS; return; }          // uniform over the launch: words only
    const uint32_t ix = (uint32_t)le_bytes(p + (CTR ? W - 3 : W), (int)S.I);
    uint32_t u = 0;
    if (ix < S.n_lines) u = S.u_of_ix[ix]; else atomicOr(err, ERR_IX);
    const uint64_t g = S.g0 + j;
    val[at + j] = (g << 24) | u;
    const bool dropped = ix < S.n_lines && u == DROP;                       // the edit dropped its label line: not fed, dates nothing
    wave_count(dropped, stats + STAT_LABEL_DROPPED);
    // addSampleU (itree.c:593): the label is created when the first record that carries it is parsed.  Clocks ascend with the
    // thread index, so all but the first few carriers of a label see a smaller time already there and skip the atomic.
    if (S.role == ROLE_DATES && ix < S.n_lines && !dropped && first_time[u] > 2 * g) atomicMin(&first_time[u], (unsigned long long)(2 * g));
}

__global__ void iota_k(uint64_t *idx, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) idx[i] = i;
}
__global__ void gather64_k(const uint64_t *__restrict__ src, const uint64_t *__restrict__ idx, uint64_t *__restrict__ dst, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}

// stats[STAT_SHARED] words that two or more records fed carry, [STAT_RELABELLED] of them relabelled, [STAT_BAD] of them BAD,
// [STAT_SUBTRACTED] records with a label that a MINUS record's run keeps from being fed
template <int W, bool GG>
__global__ __launch_bounds__(BLOCK) void merge_fold_k(const uint64_t *__restrict__ key_lo, const uint64_t *__restrict__ key_hi,
                                                      const uint64_t *__restrict__ val, uint64_t n, universe U,
                                                      unsigned long long *__restrict__ first_time, uint32_t *__restrict__ state_out,
                                                      unsigned long long *__restrict__ stats, int date) {
    const uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint64_t lo = j < n ? key_lo[j] : 0, hi = (W == 16 && j < n) ? key_hi[j] : 0;
    const bool head = j < n && !(j && key_lo[j - 1] == lo && (W != 16 || key_hi[j - 1] == hi));
    uint32_t st = ST_SKIP;                                                  // a run that feeds no record writes nothing
    bool shared = false, relabelled = false;
    if (head && val[j] == VAL_MINUS) {
        // a MINUS input holds the word (its records lead the run): nothing is fed; the records that would have been are counted
        uint32_t sub = 0;
        for (uint64_t t = j + 1; t < n && key_lo[t] == lo && (W != 16 || key_hi[t] == hi); ++t) {
            const uint64_t v = val[t];
            sub += v != VAL_MINUS && (uint32_t)(v & 0xFFFFFFu) != DROP;
        }
        if (sub) atomicAdd(&stats[STAT_SUBTRACTED], (unsigned long long)sub);
    } else if (head) {
        uint32_t fed = 0;
        uint64_t t = j;
        for (; t < n && (t == j || (key_lo[t] == lo && (W != 16 || key_hi[t] == hi))); ++t) {
            const uint64_t v = val[t];
            const uint32_t u = (uint32_t)(v & 0xFFFFFFu);
            if (u == DROP) continue;                                        // its label line was dropped: as if the input lacked the word
            if (date && first_time[u] > (v >> 24) << 1) atomicMin(&first_time[u], (unsigned long long)((v >> 24) << 1));   // addSampleU (593), see decode_k
            if (++fed == 1) { st = u; continue; }
            if (st == ST_BAD) continue;                                     // BAD is absorbing (263, 281); the run is walked to its end for `shared`
            const bool cut = utk_fold::fold_next<GG>(U, st, u);
            if (cut && st != ST_BAD) atomicMin(&first_time[st], (unsigned long long)(((v >> 24) << 1) | 1ull));   // event clock: 2 * node + 1
        }
        shared = fed > 1;
        if (shared && st != ST_BAD) {
            relabelled = true;
            for (uint64_t q = j; q < t; ++q) if ((uint32_t)(val[q] & 0xFFFFFFu) == st) relabelled = false;
        }
    }
    if (j < n) state_out[j] = st;
    wave_count(shared, stats + STAT_SHARED);
    wave_count(relabelled, stats + STAT_RELABELLED);
    wave_count(shared && st == ST_BAD, stats + STAT_BAD);
}

struct is_node { __device__ bool operator()(uint32_t s) const { return s < ST_SKIP; } };

template <int W, int I>
__global__ __launch_bounds__(BLOCK) void merge_pack_k(const uint64_t *__restrict__ lo, const uint64_t *__restrict__ hi,
                                                      const uint32_t *__restrict__ st, const uint32_t *__restrict__ ix_of_u, uint64_t first,
                                                      uint64_t count, uint8_t *__restrict__ out, unsigned long long *__restrict__ per_label) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = i < count;
    uint32_t ix = 0;
    if (live) {
        ix = ix_of_u[st[first + i]];
        uint8_t *o = out + i * (uint64_t)(W + I);
        const uint64_t l = lo[first + i];
#pragma unroll
        for (int b = 0; b < (W == 4 ? 4 : 8); ++b) o[b] = (uint8_t)(l >> (8 * b));   // fwrite(&word) of a little-endian WTYPE (402-404)
        if (W == 16) {
            const uint64_t h = hi[first + i];
#pragma unroll
            for (int b = 0; b < 8; ++b) o[8 + b] = (uint8_t)(h >> (8 * b));
        }
#pragma unroll
        for (int b = 0; b < I; ++b) o[W + b] = (uint8_t)(ix >> (8 * b));
    }
    // ++cnts[tree->ix] (412): neighbours in word order mostly share a label, so a wavefront of one label adds once
    const uint64_t m = __ballot(live);
    if (!m) return;
    const uint32_t lead = (uint32_t)__builtin_ctzll(m);
    const uint32_t ix0 = (uint32_t)__shfl((int)ix, (int)lead);
    const uint64_t same = __ballot(live && ix == ix0);
    if (same == m) { if ((threadIdx.x & 63u) == lead) atomicAdd(&per_label[ix0], (unsigned long long)__popcll(m)); }
    else if (live) atomicAdd(&per_label[ix], 1ull);
}

// ---- utree_compare_files: A's slice lies in front of B's, so after the stable sort a run is one record (a word only A or only B holds) or
// two, A's first.  fig[c * n_u + u]: words of class c under universe label u.
constexpr uint32_t CMP_SAME = 0, CMP_ONLY_A = 1, CMP_ONLY_B = 2, CMP_LEFT = 3, CMP_ARRIVED = 4;
constexpr int STAT_MOVES = 5;                              // changed words of the pass = move keys appended
static_assert(UTK_COMPARE_FIGURES == 5, "fig[] holds one row of n_u counters per class");

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

// The head of each run classifies it.  A record is B's when its event clock has reached b_g0, the clock of B's first node.  A changed word
// also appends its move key (label in A << 24 | label in B) to move_keys[0 .. stats[STAT_MOVES]), a wavefront reserving its places with one
// atomic; the order of the keys does not matter, they are sorted next.  At most n / 2 words are changed, so move_keys[n] cannot overflow.
template <int W>
__global__ __launch_bounds__(BLOCK) void compare_runs_k(const uint64_t *__restrict__ key_lo, const uint64_t *__restrict__ key_hi,
                                                        const uint64_t *__restrict__ val, uint64_t n, uint64_t b_g0, uint32_t n_u,
                                                        unsigned long long *__restrict__ fig, uint64_t *__restrict__ move_keys,
                                                        unsigned long long *__restrict__ stats) {
    const uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint64_t lo = j < n ? key_lo[j] : 0, hi = (W == 16 && j < n) ? key_hi[j] : 0;
    const bool head = j < n && !(j && key_lo[j - 1] == lo && (W != 16 || key_hi[j - 1] == hi));
    bool changed = false;
    uint32_t slot = 0, slot2 = 0;
    uint64_t key = 0;
    if (head) {
        const uint64_t v = val[j];
        const uint32_t u = (uint32_t)(v & 0xFFFFFFu);
        if (j + 1 < n && key_lo[j + 1] == lo && (W != 16 || key_hi[j + 1] == hi)) {
            const uint32_t ub = (uint32_t)(val[j + 1] & 0xFFFFFFu);
            changed = ub != u;
            slot = (changed ? CMP_LEFT : CMP_SAME) * n_u + u;
            slot2 = CMP_ARRIVED * n_u + ub;
            key = ((uint64_t)u << 24) | ub;
        } else slot = ((v >> 24) >= b_g0 ? CMP_ONLY_B : CMP_ONLY_A) * n_u + u;
    }
    wave_add(head, slot, fig);
    wave_add(changed, slot2, fig);
    const uint64_t m = __ballot(changed);
    if (!m) return;
    const uint32_t lane = threadIdx.x & 63u, lead = (uint32_t)__builtin_ctzll(m);
    unsigned long long base = 0;
    if (lane == lead) base = atomicAdd(&stats[STAT_MOVES], (unsigned long long)__popcll(m));
    const uint32_t b_lo = (uint32_t)__shfl((int)(uint32_t)base, (int)lead), b_hi = (uint32_t)__shfl((int)(uint32_t)(base >> 32), (int)lead);
    if (changed) move_keys[(((uint64_t)b_hi << 32) | b_lo) + (uint64_t)__popcll(m & ((1ull << lane) - 1ull))] = key;
}

// ---- utree_inspect_file: one input, so every run is one record; the sorted pass goes to the resident arrays as (word, universe label)
__global__ __launch_bounds__(BLOCK) void inspect_append_k(const uint64_t *__restrict__ key_lo, const uint64_t *__restrict__ key_hi,
                                                          const uint64_t *__restrict__ val, uint64_t n, uint64_t *__restrict__ out_lo,
                                                          uint64_t *__restrict__ out_hi, uint32_t *__restrict__ out_lab) {
    const uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    out_lo[j] = key_lo[j];
    if (out_hi) out_hi[j] = key_hi[j];
    out_lab[j] = (uint32_t)(val[j] & 0xFFFFFFu);
}

template <typename Fn> bool dispatch_w(int W, Fn &&fn) {
    if (W == 4) fn(std::integral_constant<int, 4>{});
    else if (W == 8) fn(std::integral_constant<int, 8>{});
    else if (W == 16) fn(std::integral_constant<int, 16>{});
    else return false;
    return true;
}

#define HK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { utree_dev_set_hip_error((int)e_, "merge: " #x); rc = e_ == hipErrorOutOfMemory ? UTREE_E_NOMEM : UTREE_E_HIP; goto fail; } } while (0)

template <typename T> hipError_t dmalloc(T **p, uint64_t n) { return hipMalloc((void **)p, (n ? n : 1) * sizeof(T)); }

/* the u64 buffers, two states, the raw records, rocprim's scratch for a sort of (u64, u64) pairs (it may hold a second copy of both) and for select */
uint64_t bytes_per_node(uint32_t W, uint32_t rec_max) { return (W == 16 ? 7ull : 4ull) * 8 + 8 + rec_max + 16 + 4; }

}  // namespace

struct utk_merge_dev {
    utk_merge_cfg cfg;
    uint64_t cap;
    uint8_t *h_stage[2], *d_raw; hipEvent_t ev[2]; uint64_t stage_bytes;
    uint64_t *b[7];                                 // node-sized buffers: W != 16 uses four of them
    uint32_t *st, *st2;
    uint64_t *d_bins;
    uint32_t **d_u_of_ix;                           // host array of device pointers
    char *d_ublob; uint64_t *d_uoff; uint32_t *d_toff, *d_tids;
    unsigned long long *d_first, *d_stats, *d_nsel, *d_cnt;
    uint32_t *d_err, *d_ix;
    uint8_t *d_out[2], *h_out[2]; uint64_t out_chunk;
    uint32_t n_labels;
    uint64_t seg_n; const uint64_t *seg_lo, *seg_hi; const uint32_t *seg_st;
    unsigned long long *d_fig;                      // compare: [N_CMP][n_u] words per class and label, summed over the passes
    uint64_t moves_n;                               // compare: (key, count) pairs of the last pass, keys in b[0], counts in st
};

// The front half of a pass, shared by the merge and the compare: every slice from its file through the two pinned staging buffers onto the
// device, decoded in slice order, then the stable sort by word.  *n: the pass's records; *err: what decode_k found (then nothing is sorted);
// *s_lo, *s_hi (W = 16), *s_val: the sorted words and values.  Afterwards b[0] and b[1] hold nothing that is still needed.
static int decode_sort(utk_merge_dev *D, const utk_merge_slice *sl, uint32_t n_sl, uint64_t *n_out, uint32_t *err, uint64_t **s_lo_out,
                       uint64_t **s_hi_out, uint64_t **s_val_out, uint32_t *io_slice) {
    int rc = UTREE_OK;
    const int W = (int)D->cfg.W;
    void *tmp = nullptr;
    size_t tb = 0;
    uint64_t n = 0;
    int turn = 0, used[2] = {0, 0};
    uint32_t h_err = 0;
    uint64_t *k_lo = D->b[0], *k_val = D->b[1], *s_lo, *s_hi = nullptr, *s_val;
    *n_out = 0; *err = 0;
    HK(hipSetDevice(D->cfg.device));
    for (uint32_t s = 0; s < n_sl; ++s) {
        const uint64_t rec = (sl[s].is_ctr ? D->cfg.W - 3 : D->cfg.W) + sl[s].I;
        if ((sl[s].raw_off & 255u) || sl[s].raw_off + sl[s].n * rec > D->cfg.cap_raw || sl[s].input >= D->cfg.n_in) return UTREE_E_ARG;
        if (sl[s].is_ctr && (!D->d_bins || sl[s].n_bins > UTREE_NUMBINS - 1)) return UTREE_E_ARG;
        n += sl[s].n;
    }
    if (n > D->cap) return UTREE_E_ARG;
    HK(hipMemset(D->d_err, 0, 4));
    HK(hipMemset(D->d_stats, 0, 8 * N_STATS));
    if (!n) return UTREE_OK;
    {
        uint64_t at = 0;
        for (uint32_t s = 0; s < n_sl; ++s) {
            if (!sl[s].n) continue;
            // the slice's records: file -> staging buffer (a team of host threads) -> device; the upload of one chunk runs while the next is read
            const uint64_t bytes = sl[s].n * ((sl[s].is_ctr ? D->cfg.W - 3 : D->cfg.W) + sl[s].I);
            for (uint64_t done = 0; done < bytes; done += D->stage_bytes, turn ^= 1) {
                const uint64_t part = bytes - done < D->stage_bytes ? bytes - done : D->stage_bytes;
                if (used[turn]) HK(hipEventSynchronize(D->ev[turn]));
                if (utree_pread_team(sl[s].fd, D->h_stage[turn], part, sl[s].file_off + done, 8)) { *io_slice = s; rc = UTREE_E_IO; goto fail; }
                HK(hipMemcpyAsync(D->d_raw + sl[s].raw_off + done, D->h_stage[turn], part, hipMemcpyHostToDevice, 0));
                HK(hipEventRecord(D->ev[turn], 0));
                used[turn] = 1;
            }
            if (sl[s].is_ctr) HK(hipMemcpy(D->d_bins, sl[s].h_bins, 8ull * (sl[s].n_bins + 1ull), hipMemcpyHostToDevice));
            const slice_dev S = {(const uint32_t *)(D->d_raw + sl[s].raw_off), sl[s].n, sl[s].g0, D->d_u_of_ix[sl[s].input], D->cfg.n_lines[sl[s].input],
                                 sl[s].I, sl[s].has_prev, sl[s].prev_hi, sl[s].prev_lo, D->d_bins, sl[s].p_lo, sl[s].n_bins, sl[s].first,
                                 sl[s].minus ? ROLE_MINUS : (D->cfg.has_minus || D->cfg.compare) ? ROLE_REGULAR : ROLE_DATES};
            const unsigned gb = (unsigned)((sl[s].n + BLOCK - 1) / BLOCK);
            const bool ctr = sl[s].is_ctr != 0;
            dispatch_w(W, [&](auto w) {
                constexpr int WV = decltype(w)::value;
                if (ctr) decode_k<WV, true><<<dim3(gb), dim3(BLOCK)>>>(S, at, k_lo, D->b[4], k_val, D->d_first, D->d_err, D->d_stats);
                else decode_k<WV, false><<<dim3(gb), dim3(BLOCK)>>>(S, at, k_lo, D->b[4], k_val, D->d_first, D->d_err, D->d_stats);
            });
            HK(hipGetLastError());
            if (ctr) HK(hipDeviceSynchronize());                            /* the bin scratch is reused by the next `.ctr` slice */
            at += sl[s].n;
        }
    }
    HK(hipMemcpy(&h_err, D->d_err, 4, hipMemcpyDeviceToHost));
    *err = h_err;
    *n_out = n;
    if (h_err) return UTREE_OK;
    {
        const unsigned gb = (unsigned)((n + BLOCK - 1) / BLOCK);
        // ---- stable sort by word (W = 4: only the low 32 bits carry the 16-mer) ----
        if (W != 16) {
            const unsigned end_bit = W == 4 ? 32u : 64u;
            s_lo = D->b[2]; s_val = D->b[3];
            HK(rocprim::radix_sort_pairs(nullptr, tb, k_lo, s_lo, k_val, s_val, n, 0, end_bit));
            HK(hipMalloc(&tmp, tb ? tb : 8));
            HK(rocprim::radix_sort_pairs(tmp, tb, k_lo, s_lo, k_val, s_val, n, 0, end_bit));
        } else {
            // least significant half first, then the most significant half (both stable); permutations carried as indices
            uint64_t *k_hi = D->b[4], *idx = D->b[2], *idx2 = D->b[3], *a_lo = D->b[5], *g_hi = D->b[6];
            iota_k<<<dim3(gb), dim3(BLOCK)>>>(idx, n);
            HK(rocprim::radix_sort_pairs(nullptr, tb, k_lo, a_lo, idx, idx2, n, 0, 64));
            HK(hipMalloc(&tmp, tb ? tb : 8));
            HK(rocprim::radix_sort_pairs(tmp, tb, k_lo, a_lo, idx, idx2, n, 0, 64));      /* idx2 = order by lo */
            gather64_k<<<dim3(gb), dim3(BLOCK)>>>(k_hi, idx2, g_hi, n);
            HK(rocprim::radix_sort_pairs(tmp, tb, g_hi, k_hi, idx2, idx, n, 0, 64));      /* k_hi sorted, idx = final order */
            gather64_k<<<dim3(gb), dim3(BLOCK)>>>(k_lo, idx, a_lo, n);
            gather64_k<<<dim3(gb), dim3(BLOCK)>>>(k_val, idx, g_hi, n);
            s_lo = a_lo; s_hi = k_hi; s_val = g_hi;
        }
        HK(hipGetLastError());
        HK(hipDeviceSynchronize());
        HK(hipFree(tmp)); tmp = nullptr;
        *s_lo_out = s_lo; *s_hi_out = s_hi; *s_val_out = s_val;
    }
fail:
    if (rc) (void)hipDeviceSynchronize();
    if (tmp) (void)hipFree(tmp);
    return rc;
}

extern "C" {

int utk_merge_limit(int device, uint32_t W, uint32_t rec_max, uint64_t *nodes) {
    int rc = UTREE_OK;
    size_t free_b = 0, total_b = 0;
    HK(hipSetDevice(device));
    HK(hipMemGetInfo(&free_b, &total_b));
    {
        const uint64_t reserve = (uint64_t)2 << 30;                         /* universe, bin table, output chunk, rocprim's scratch */
        uint64_t lim = (free_b > reserve ? free_b - reserve : 0) / bytes_per_node(W, rec_max);
        if (lim > (1ull << 31) - 1) lim = (1ull << 31) - 1;                 /* rocprim sorts fewer than 2^31 items */
        *nodes = lim;
    }
fail:
    return rc;
}

/* The compare's pass holds what the merge's holds, less the second state array and the output chunks.  After the sort by word its move keys
 * (at most half the pass's nodes, 8 bytes each) are sorted and run-length-encoded in place of the two buffers the unsorted records came in,
 * and rocprim's scratch for that (a second copy of the keys) takes the room the first sort's scratch has given back: bytes_per_node covers
 * it.  What comes on top is the five counters per universe label. */
int utk_compare_limit(int device, uint32_t W, uint32_t rec_max, uint32_t n_u, uint64_t *nodes) {
    int rc = UTREE_OK;
    size_t free_b = 0, total_b = 0;
    HK(hipSetDevice(device));
    HK(hipMemGetInfo(&free_b, &total_b));
    {
        const uint64_t reserve = ((uint64_t)2 << 30) + 8ull * UTK_COMPARE_FIGURES * n_u;
        uint64_t lim = (free_b > reserve ? free_b - reserve : 0) / bytes_per_node(W, rec_max);
        if (lim > (1ull << 31) - 1) lim = (1ull << 31) - 1;                 /* rocprim sorts fewer than 2^31 items */
        *nodes = lim;
    }
fail:
    return rc;
}

void utk_merge_close(utk_merge_dev *D) {
    if (!D) return;
    (void)hipSetDevice(D->cfg.device);
    (void)hipDeviceSynchronize();
    for (int q = 0; q < 2; ++q) {
        if (D->h_stage[q]) (void)hipHostFree(D->h_stage[q]);
        if (D->h_out[q]) (void)hipHostFree(D->h_out[q]);
        if (D->d_out[q]) (void)hipFree(D->d_out[q]);
        if (D->ev[q]) (void)hipEventDestroy(D->ev[q]);
    }
    void *dev[] = {D->d_raw, D->b[0], D->b[1], D->b[2], D->b[3], D->b[4], D->b[5], D->b[6], D->st, D->st2, D->d_bins, D->d_ublob, D->d_uoff,
                   D->d_toff, D->d_tids, D->d_first, D->d_stats, D->d_nsel, D->d_cnt, D->d_err, D->d_ix, D->d_fig};
    for (void *p : dev) if (p) (void)hipFree(p);
    if (D->d_u_of_ix) { for (uint32_t i = 0; i < D->cfg.n_in; ++i) if (D->d_u_of_ix[i]) (void)hipFree(D->d_u_of_ix[i]); free(D->d_u_of_ix); }
    free(D);
}

int utk_merge_open(const utk_merge_cfg *cfg, utk_merge_dev **out) {
    int rc = UTREE_OK;
    if (!dispatch_w((int)cfg->W, [](auto) {}) || (cfg->I_out != 2 && cfg->I_out != 4)) return UTREE_E_ARG;
    utk_merge_dev *D = (utk_merge_dev *)calloc(1, sizeof *D);
    if (!D) return UTREE_E_NOMEM;
    D->cfg = *cfg;
    D->cap = cfg->cap_nodes ? cfg->cap_nodes : 1;
    D->out_chunk = D->cap < (16ull << 20) ? D->cap : (16ull << 20);
    D->stage_bytes = cfg->cap_raw + 512 < (256ull << 20) ? cfg->cap_raw + 512 : (256ull << 20);
    {   /* test hooks: small inputs in many staging chunks and many output chunks; they only lower a size, to 1 at the least */
        const char *e = getenv("UTREE_TEST_MERGE_STAGE_BYTES");
        if (e && atoll(e) > 0 && (uint64_t)atoll(e) < D->stage_bytes) D->stage_bytes = (uint64_t)atoll(e);
        e = getenv("UTREE_TEST_MERGE_OUT_NODES");
        if (e && atoll(e) > 0 && (uint64_t)atoll(e) < D->out_chunk) D->out_chunk = (uint64_t)atoll(e);
    }
    D->d_u_of_ix = (uint32_t **)calloc(cfg->n_in, sizeof(uint32_t *));
    if (!D->d_u_of_ix) { rc = UTREE_E_NOMEM; goto fail; }
    HK(hipSetDevice(cfg->device));
    for (int q = 0; q < 2; ++q) {
        HK(hipHostMalloc((void **)&D->h_stage[q], D->stage_bytes, hipHostMallocDefault));
        HK(hipEventCreateWithFlags(&D->ev[q], hipEventDisableTiming));
    }
    HK(dmalloc(&D->d_raw, cfg->cap_raw + 512));
    for (int q = 0; q < (cfg->W == 16 ? 7 : 4); ++q) HK(dmalloc(&D->b[q], D->cap));
    HK(dmalloc(&D->st, D->cap));
    if (!cfg->compare) HK(dmalloc(&D->st2, D->cap));
    if (cfg->any_ctr) HK(dmalloc(&D->d_bins, (uint64_t)UTREE_NUMBINS + 1));
    HK(dmalloc(&D->d_ublob, cfg->ublob_bytes + 8)); HK(dmalloc(&D->d_uoff, cfg->n_u)); HK(dmalloc(&D->d_toff, (uint64_t)cfg->n_u + 1));
    HK(dmalloc(&D->d_tids, cfg->n_trunc)); HK(dmalloc(&D->d_first, cfg->n_u)); HK(dmalloc(&D->d_stats, N_STATS)); HK(dmalloc(&D->d_nsel, 1));
    HK(dmalloc(&D->d_err, 1)); HK(dmalloc(&D->d_ix, cfg->n_u));
    if (cfg->compare) {
        HK(dmalloc(&D->d_fig, (uint64_t)UTK_COMPARE_FIGURES * cfg->n_u));
        HK(hipMemset(D->d_fig, 0, 8ull * UTK_COMPARE_FIGURES * (cfg->n_u ? cfg->n_u : 1)));
    }
    for (int q = 0; q < (cfg->compare ? 0 : 2); ++q) {                      /* a compare writes no nodes */
        HK(dmalloc(&D->d_out[q], D->out_chunk * (cfg->W + cfg->I_out)));
        HK(hipHostMalloc((void **)&D->h_out[q], D->out_chunk * (cfg->W + cfg->I_out) + 8, hipHostMallocDefault));
    }
    if (cfg->ublob_bytes) HK(hipMemcpy(D->d_ublob, cfg->h_ublob, cfg->ublob_bytes, hipMemcpyHostToDevice));
    if (cfg->n_u) {
        HK(hipMemcpy(D->d_uoff, cfg->h_uoff, 8ull * cfg->n_u, hipMemcpyHostToDevice));
        HK(hipMemset(D->d_first, 0xFF, 8ull * cfg->n_u));
    }
    HK(hipMemcpy(D->d_toff, cfg->h_trunc_off, 4ull * (cfg->n_u + 1ull), hipMemcpyHostToDevice));
    if (cfg->n_trunc) HK(hipMemcpy(D->d_tids, cfg->h_trunc_ids, 4ull * cfg->n_trunc, hipMemcpyHostToDevice));
    for (uint32_t i = 0; i < cfg->n_in; ++i) {
        HK(dmalloc(&D->d_u_of_ix[i], cfg->n_lines[i]));
        if (cfg->n_lines[i]) HK(hipMemcpy(D->d_u_of_ix[i], cfg->h_u_of_ix[i], 4ull * cfg->n_lines[i], hipMemcpyHostToDevice));
    }
    *out = D;
    return UTREE_OK;
fail:
    utk_merge_close(D);
    return rc;
}

int utk_merge_pass(utk_merge_dev *D, const utk_merge_slice *sl, uint32_t n_sl, int count_stats, utk_merge_pass_out *out, uint32_t *io_slice) {
    int rc = UTREE_OK;
    const int W = (int)D->cfg.W;
    const universe U = {D->d_ublob, D->d_uoff, D->d_toff, D->d_tids};
    void *tmp = nullptr;
    size_t tb = 0, tb2 = 0;
    uint64_t n = 0;
    unsigned long long h_stats[N_STATS] = {0}, nn = 0;
    uint64_t *s_lo = nullptr, *s_hi = nullptr, *s_val = nullptr;
    memset(out, 0, sizeof *out);
    D->seg_n = 0;
    rc = decode_sort(D, sl, n_sl, &n, &out->err, &s_lo, &s_hi, &s_val, io_slice);
    if (rc || !n || out->err) return rc;                                    /* the caller names the error; indices were not looked up */
    {
        const unsigned gb = (unsigned)((n + BLOCK - 1) / BLOCK);
        // ---- replay each run of equal words ----
        dispatch_w(W, [&](auto w) {
            constexpr int WV = decltype(w)::value;
            if (D->cfg.gg) merge_fold_k<WV, true><<<dim3(gb), dim3(BLOCK)>>>(s_lo, s_hi, s_val, n, U, D->d_first, D->st, D->d_stats, D->cfg.has_minus);
            else merge_fold_k<WV, false><<<dim3(gb), dim3(BLOCK)>>>(s_lo, s_hi, s_val, n, U, D->d_first, D->st, D->d_stats, D->cfg.has_minus);
        });
        HK(hipGetLastError());
        // ---- keep what is not BAD, ascending: the sorted buffers are compacted into the ones the unsorted words came in ----
        {
            auto flags = rocprim::make_transform_iterator(D->st, is_node());
            HK(rocprim::select(nullptr, tb, D->st, flags, D->st2, D->d_nsel, n));
            HK(rocprim::select(nullptr, tb2, s_lo, flags, D->b[0], D->d_nsel, n));
            if (tb2 > tb) tb = tb2;
            HK(hipMalloc(&tmp, tb ? tb : 8));
            HK(rocprim::select(tmp, tb, s_lo, flags, D->b[0], D->d_nsel, n));
            if (W == 16) HK(rocprim::select(tmp, tb, s_hi, flags, D->b[1], D->d_nsel, n));
            HK(rocprim::select(tmp, tb, D->st, flags, D->st2, D->d_nsel, n));
            HK(hipMemcpy(&nn, D->d_nsel, 8, hipMemcpyDeviceToHost));
            HK(hipMemcpy(h_stats, D->d_stats, 8 * N_STATS, hipMemcpyDeviceToHost));
            HK(hipDeviceSynchronize());
            HK(hipFree(tmp)); tmp = nullptr;
        }
        D->seg_n = nn; D->seg_lo = D->b[0]; D->seg_hi = W == 16 ? D->b[1] : nullptr; D->seg_st = D->st2;
        out->n_nodes = nn;
        if (count_stats) {
            out->n_shared = h_stats[STAT_SHARED]; out->n_relabelled = h_stats[STAT_RELABELLED]; out->n_dropped = h_stats[STAT_BAD];
            out->n_label_dropped = h_stats[STAT_LABEL_DROPPED]; out->n_subtracted = h_stats[STAT_SUBTRACTED];
        }
    }
fail:
    if (rc) (void)hipDeviceSynchronize();
    if (tmp) (void)hipFree(tmp);
    return rc;
}

int utk_compare_pass(utk_merge_dev *D, const utk_merge_slice *sl, uint32_t n_sl, uint64_t b_g0, utk_compare_pass_out *out, uint32_t *io_slice) {
    int rc = UTREE_OK;
    const int W = (int)D->cfg.W;
    void *tmp = nullptr;
    size_t tb = 0, tb2 = 0;
    uint64_t n = 0;
    unsigned long long h_stats[N_STATS] = {0}, runs = 0;
    uint64_t *s_lo = nullptr, *s_hi = nullptr, *s_val = nullptr;
    memset(out, 0, sizeof *out);
    D->moves_n = 0;
    if (!D->cfg.compare) return UTREE_E_ARG;
    rc = decode_sort(D, sl, n_sl, &n, &out->err, &s_lo, &s_hi, &s_val, io_slice);
    if (rc || !n || out->err) return rc;
    {
        const unsigned gb = (unsigned)((n + BLOCK - 1) / BLOCK);
        uint64_t *keys = D->b[0], *sorted = D->b[1];                        /* the unsorted words and values: free since the sort */
        dispatch_w(W, [&](auto w) {
            constexpr int WV = decltype(w)::value;
            compare_runs_k<WV><<<dim3(gb), dim3(BLOCK)>>>(s_lo, s_hi, s_val, n, b_g0, D->cfg.n_u, D->d_fig, keys, D->d_stats);
        });
        HK(hipGetLastError());
        HK(hipMemcpy(h_stats, D->d_stats, 8 * N_STATS, hipMemcpyDeviceToHost));
        const uint64_t m = h_stats[STAT_MOVES];
        if (m > n / 2) { rc = UTREE_E_HIP; utree_dev_set_hip_error(0, "compare: more changed words than runs of two"); goto fail; }
        if (m) {
            // ---- the distinct (label in A, label in B) pairs of the pass and how many words made each move ----
            HK(rocprim::radix_sort_keys(nullptr, tb, keys, sorted, m, 0, 48));
            HK(rocprim::run_length_encode(nullptr, tb2, sorted, (unsigned int)m, keys, D->st, D->d_nsel));
            if (tb2 > tb) tb = tb2;
            HK(hipMalloc(&tmp, tb ? tb : 8));
            HK(rocprim::radix_sort_keys(tmp, tb, keys, sorted, m, 0, 48));
            HK(rocprim::run_length_encode(tmp, tb, sorted, (unsigned int)m, keys, D->st, D->d_nsel));
            HK(hipMemcpy(&runs, D->d_nsel, 8, hipMemcpyDeviceToHost));
            HK(hipDeviceSynchronize());
            HK(hipFree(tmp)); tmp = nullptr;
        }
        D->moves_n = runs;
        out->n_changed = m;
        out->n_moves = runs;
    }
fail:
    if (rc) (void)hipDeviceSynchronize();
    if (tmp) (void)hipFree(tmp);
    return rc;
}

int utk_inspect_pass(utk_merge_dev *D, const utk_merge_slice *sl, uint32_t n_sl, uint64_t at, uint64_t cap, uint64_t *d_lo, uint64_t *d_hi,
                     uint32_t *d_lab, uint64_t *n_out, uint32_t *err, uint32_t *io_slice) {
    int rc = UTREE_OK;
    uint64_t n = 0;
    uint64_t *s_lo = nullptr, *s_hi = nullptr, *s_val = nullptr;
    *n_out = 0; *err = 0;
    if (!D->cfg.compare || D->cfg.n_in != 1 || !d_lo || !d_lab || (D->cfg.W == 16) != (d_hi != nullptr)) return UTREE_E_ARG;
    rc = decode_sort(D, sl, n_sl, &n, err, &s_lo, &s_hi, &s_val, io_slice);
    if (rc || !n || *err) return rc;
    if (at > cap || n > cap - at) return UTREE_E_ARG;                       /* never beyond the resident arrays */
    inspect_append_k<<<dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK)>>>(s_lo, s_hi, s_val, n, d_lo + at, d_hi ? d_hi + at : nullptr, d_lab + at);
    HK(hipGetLastError());
    HK(hipDeviceSynchronize());
    *n_out = n;
fail:
    if (rc) (void)hipDeviceSynchronize();
    return rc;
}

int utk_compare_moves(utk_merge_dev *D, uint64_t *h_keys, uint32_t *h_counts) {
    int rc = UTREE_OK;
    HK(hipSetDevice(D->cfg.device));
    if (D->moves_n) {
        HK(hipMemcpy(h_keys, D->b[0], 8ull * D->moves_n, hipMemcpyDeviceToHost));
        HK(hipMemcpy(h_counts, D->st, 4ull * D->moves_n, hipMemcpyDeviceToHost));
    }
fail:
    return rc;
}

int utk_compare_figures(utk_merge_dev *D, uint64_t *h_fig) {
    int rc = UTREE_OK;
    HK(hipSetDevice(D->cfg.device));
    if (D->cfg.n_u) HK(hipMemcpy(h_fig, D->d_fig, 8ull * UTK_COMPARE_FIGURES * D->cfg.n_u, hipMemcpyDeviceToHost));
fail:
    return rc;
}

int utk_merge_events(utk_merge_dev *D, uint64_t *h_first_time) {
    int rc = UTREE_OK;
    HK(hipSetDevice(D->cfg.device));
    if (D->cfg.n_u) HK(hipMemcpy(h_first_time, D->d_first, 8ull * D->cfg.n_u, hipMemcpyDeviceToHost));
fail:
    return rc;
}

int utk_merge_set_ix(utk_merge_dev *D, const uint32_t *h_ix_of_u, uint32_t n_labels) {
    int rc = UTREE_OK;
    HK(hipSetDevice(D->cfg.device));
    if (D->d_cnt) { HK(hipFree(D->d_cnt)); D->d_cnt = nullptr; }
    HK(dmalloc(&D->d_cnt, n_labels));
    HK(hipMemset(D->d_cnt, 0, 8ull * (n_labels ? n_labels : 1)));
    if (D->cfg.n_u) HK(hipMemcpy(D->d_ix, h_ix_of_u, 4ull * D->cfg.n_u, hipMemcpyHostToDevice));
    D->n_labels = n_labels;
fail:
    return rc;
}

int utk_merge_emit(utk_merge_dev *D, int fd) {
    int rc = UTREE_OK;
    const uint64_t rec = (uint64_t)D->cfg.W + D->cfg.I_out;
    HK(hipSetDevice(D->cfg.device));
    {
        // chunk c is packed and downloaded (asynchronously) into buffer c & 1 while chunk c - 1 is written from the other one
        uint64_t pend_bytes = 0; int pend = -1, c = 0;
        for (uint64_t first = 0; first < D->seg_n || pend >= 0; first += D->out_chunk, ++c) {
            uint64_t cnt = 0;
            if (first < D->seg_n) {
                cnt = D->seg_n - first < D->out_chunk ? D->seg_n - first : D->out_chunk;
                const unsigned gb = (unsigned)((cnt + BLOCK - 1) / BLOCK);
                uint8_t *d_out = D->d_out[c & 1];
                dispatch_w((int)D->cfg.W, [&](auto w) {
                    constexpr int WV = decltype(w)::value;
                    if (D->cfg.I_out == 2) merge_pack_k<WV, 2><<<dim3(gb), dim3(BLOCK)>>>(D->seg_lo, D->seg_hi, D->seg_st, D->d_ix, first, cnt, d_out, D->d_cnt);
                    else merge_pack_k<WV, 4><<<dim3(gb), dim3(BLOCK)>>>(D->seg_lo, D->seg_hi, D->seg_st, D->d_ix, first, cnt, d_out, D->d_cnt);
                });
                HK(hipGetLastError());
                HK(hipMemcpyAsync(D->h_out[c & 1], d_out, cnt * rec, hipMemcpyDeviceToHost, 0));
                HK(hipEventRecord(D->ev[c & 1], 0));
            }
            if (pend >= 0) {
                uint64_t done = 0;
                while (done < pend_bytes) {
                    ssize_t w = write(fd, D->h_out[pend] + done, pend_bytes - done);
                    if (w <= 0) { rc = UTREE_E_IO; goto fail; }
                    done += (uint64_t)w;
                }
                pend = -1;
            }
            if (cnt) { HK(hipEventSynchronize(D->ev[c & 1])); pend = c & 1; pend_bytes = cnt * rec; }
        }
    }
fail:
    if (rc) (void)hipDeviceSynchronize();
    return rc;
}

int utk_merge_counts(utk_merge_dev *D, uint64_t *h_per_label) {
    int rc = UTREE_OK;
    HK(hipSetDevice(D->cfg.device));
    if (D->n_labels) HK(hipMemcpy(h_per_label, D->d_cnt, 8ull * D->n_labels, hipMemcpyDeviceToHost));
fail:
    return rc;
}

}  // extern "C"
