// pairs_kernels.hip -- paired-end reads: the two mates of a pair joined into ONE query, mate 1 + 'N' + mate 2, in front of the classify
// kernels (include/utree_amd.h: utree_pairs_join).  gfx950 / wave64 only.
//
// The reference reads no pairs, but it fixes what a pair's answer must be: with RC it searches read + 'N' + revcomp(read) as one query
// (itree.c:891-898) -- a byte that is no base breaks the k-mer windows (903-927) and the hits of both sides go into one list for one vote.
// A pair joined the same way needs no classify, vote or report code of its own: those take any (d_bases, d_off, d_len).
//
//   pairs_count_k / pairs_scan_k / pairs_emit_k   len1 + 1 + len2 -> tight joined offsets (u64) and lengths (u32), total, longest: the
//                     three passes of text_kernels.hip's newline scan; the per-block sums live in the offset array itself (entry
//                     1024 b holds block b's sum, then its prefix, then -- the same number -- pair 1024 b's offset): no workspace
//   pairs_gather_k    partitioned by OUTPUT: a run is 16 consecutive joined bytes, a thread owns four of them, a workgroup a tile of
//                     16 KiB.  The tile's first pair comes from a 64-ary search over the offsets (one probe per lane and step: four
//                     steps for 16 M pairs); the offsets, source offsets and mate-1 lengths of the tile's pairs go to LDS in ONE round
//                     of loads, and a thread finds its runs' pairs there.  A run is put together piece by piece, a piece being an 'N'
//                     or the part of one mate the run holds -- the whole run 17 times of 19 with 150 bp mates, three pieces where it
//                     crosses a pair's middle: one 16-byte load per piece at whatever alignment the source has, placed inside the
//                     mate, shifted and masked (mates under 16 bytes: byte loads); then one 16-byte store.  Work is
//                     proportional to bytes: a 16 Mb mate is 1024 tiles, a tile of one-byte pairs 5461 pairs (more than the LDS arrays
//                     hold: its threads look their pairs up in HBM instead, fourteen search steps at most).
//
// Nothing is written outside [0, total): a joined buffer that is too small, or a pair longer than 32 bits hold, sets meta.error and the
// gather pass returns at once.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "utree_internal.h"
#include "pairs_kernels.h"

namespace {

constexpr uint32_t TB = 256;                       // threads per block
constexpr uint32_t SCAN_ITEMS = 4 * TB;            // pairs per block of the count and emit passes
constexpr uint32_t RUN = 16;                       // joined bytes of one run of the gather pass: one 16-byte store
constexpr uint32_t RUNS = 4;                       // runs per thread
constexpr uint32_t TILE = TB * RUN * RUNS;         // joined bytes per workgroup: 16 KiB
constexpr uint32_t TILE_OFFS = 128;                // pairs of a tile kept in LDS: pairs of 128 bytes and more on average (150 bp mates: 55)

__device__ __forceinline__ uint64_t joined_len(const uint32_t *__restrict__ len1, const uint32_t *__restrict__ len2, uint64_t i) {
    return (uint64_t)len1[i] + 1u + (uint64_t)len2[i];
}

__global__ __launch_bounds__(TB) void pairs_count_k(const uint32_t *__restrict__ len1, const uint32_t *__restrict__ len2, uint32_t n,
                                                    uint64_t *__restrict__ joff, utree_pairs_meta *__restrict__ meta) {
    __shared__ uint64_t s_part[TB / 64];
    const uint64_t first = (uint64_t)blockIdx.x * SCAN_ITEMS;
    uint64_t sum = 0, mx = 0;
#pragma unroll
    for (uint32_t k = 0; k < SCAN_ITEMS / TB; ++k) {
        const uint64_t i = first + k * TB + threadIdx.x;
        if (i < n) { const uint64_t l = joined_len(len1, len2, i); sum += l; mx = l > mx ? l : mx; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o);
        const uint64_t m2 = __shfl_xor(mx, o); mx = m2 > mx ? m2 : mx;
    }
    if ((threadIdx.x & 63u) == 0) {
        s_part[threadIdx.x >> 6] = sum;
        atomicMax(&meta->max_len, mx > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)mx);
        if (mx > 0xFFFFFFFFull) atomicOr(&meta->error, UTK_PAIRS_E_LENGTH);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t t = 0;
        for (uint32_t i = 0; i < TB / 64; ++i) t += s_part[i];
        joff[first] = t;
    }
}

// exclusive prefix of the per-block sums (entries 0, 1024, 2048, ... of joff), one workgroup: 16 M pairs are 16 K blocks
__global__ __launch_bounds__(1024) void pairs_scan_k(uint64_t *__restrict__ joff, uint32_t nb, uint64_t capacity, utree_pairs_meta *__restrict__ meta) {
    __shared__ uint64_t s_tot[1024];
    const uint32_t per = (nb + 1023) / 1024, lo = threadIdx.x * per < nb ? threadIdx.x * per : nb, hi = lo + per < nb ? lo + per : nb;
    uint64_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += joff[(uint64_t)i * SCAN_ITEMS];
    s_tot[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {                                             // Hillis-Steele, inclusive
        const uint64_t v = threadIdx.x >= d ? s_tot[threadIdx.x - d] : 0;
        __syncthreads();
        s_tot[threadIdx.x] += v;
        __syncthreads();
    }
    uint64_t run = s_tot[threadIdx.x] - sum;
    for (uint32_t i = lo; i < hi; ++i) { const uint64_t c = joff[(uint64_t)i * SCAN_ITEMS]; joff[(uint64_t)i * SCAN_ITEMS] = run; run += c; }
    if (threadIdx.x == 1023) {
        meta->total_bases = s_tot[1023];
        if (s_tot[1023] > capacity) atomicOr(&meta->error, UTK_PAIRS_E_CAPACITY);
    }
}

__global__ __launch_bounds__(TB) void pairs_emit_k(const uint32_t *__restrict__ len1, const uint32_t *__restrict__ len2, uint32_t n,
                                                   uint64_t *__restrict__ joff, uint32_t *__restrict__ jlen) {
    __shared__ uint64_t s_part[TB / 64];
    const uint64_t first = (uint64_t)blockIdx.x * SCAN_ITEMS;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint64_t base = joff[first];                                                          // the block's prefix (= its first pair's offset)
#pragma unroll
    for (uint32_t k = 0; k < SCAN_ITEMS / TB; ++k) {
        const uint64_t i = first + k * TB + threadIdx.x;
        const uint64_t l = i < n ? joined_len(len1, len2, i) : 0;
        uint64_t inc = l;                                                                 // inclusive scan over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint64_t v = __shfl_up(inc, d); if (lane >= (uint32_t)d) inc += v; }
        if (lane == 63) s_part[w] = inc;
        __syncthreads();                                                                  // (every thread has read joff[first] by now)
        uint64_t at = base + inc - l, all = 0;
        for (uint32_t i2 = 0; i2 < TB / 64; ++i2) { if (i2 < w) at += s_part[i2]; all += s_part[i2]; }
        if (i < n) { joff[i] = at; jlen[i] = l > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)l; }
        base += all;
        __syncthreads();
    }
}

struct __attribute__((packed)) bytes16 { uint64_t a, b; };                                 // sixteen bytes at any alignment
typedef unsigned __int128 u128;

// what a tile's threads look up per pair, for the first TILE_OFFS pairs that begin at or behind the tile's first byte
struct tile_lds {
    uint64_t joff[TILE_OFFS + 1];
    uint64_t off1[TILE_OFFS], off2[TILE_OFFS];
    uint32_t len1[TILE_OFFS];
};
struct gather_args {
    const uint8_t *b1; const uint64_t *off1; const uint32_t *len1;
    const uint8_t *b2; const uint64_t *off2;
    const uint64_t *joff;
    uint32_t n, p0;                                  // pairs; the pair the tile's first byte lies in
    uint64_t total;
};

// pair p0 + j as the tile sees it: from LDS, or -- a tile of tiny pairs, more of them than the LDS arrays hold -- from HBM
template <bool LDS> __device__ __forceinline__ uint64_t pair_start(const gather_args &g, const tile_lds &t, uint32_t j) {
    if (LDS) return t.joff[j];
    const uint64_t idx = (uint64_t)g.p0 + j;
    return idx < g.n ? g.joff[idx] : g.total;
}
template <bool LDS> __device__ __forceinline__ void pair_mates(const gather_args &g, const tile_lds &t, uint32_t j, uint32_t &l1, uint64_t &o1, uint64_t &o2) {
    if (LDS) { l1 = t.len1[j]; o1 = t.off1[j]; o2 = t.off2[j]; }
    else { const uint64_t idx = (uint64_t)g.p0 + j; l1 = g.len1[idx]; o1 = g.off1[idx]; o2 = g.off2[idx]; }
}

// joined bytes [o, o + nvalid), nvalid <= RUN, o - t0 < TILE.  jl: a pair known to begin at or before o (the thread's previous run's).
template <bool LDS>
__device__ __forceinline__ void gather_run(const gather_args &g, const tile_lds &t, uint64_t t0, uint64_t o, uint32_t nvalid, uint32_t &jl,
                                           uint8_t *__restrict__ dst) {
    // my pair: the last j with start(j) <= o.  start(j) >= t0 + j for j >= 1, so start(o - t0 + 1) > o
    uint32_t jh = (uint32_t)(o - t0) + 1;
    if (LDS && jh > TILE_OFFS) jh = TILE_OFFS;                                            // (start(TILE_OFFS) is at or past the tile's end)
    while (jh - jl > 1) {
        const uint32_t mid = (jl + jh) >> 1;
        if (pair_start<LDS>(g, t, mid) <= o) jl = mid; else jh = mid;
    }
    uint32_t j = jl, l1;
    uint64_t start = pair_start<LDS>(g, t, j), next = pair_start<LDS>(g, t, j + 1), o1, o2;
    pair_mates<LDS>(g, t, j, l1, o1, o2);
    // The run piece by piece: a piece is an 'N' or the part of ONE mate the run holds (the whole run, 17 times of 19 with 150 bp mates; three
    // pieces where it crosses a pair's middle).  A piece of a mate of sixteen bytes or more is one 16-byte load placed INSIDE the mate -- at
    // the piece where that fits, else pulled back from the mate's end or up to its start --, shifted to where the piece belongs and masked;
    // shorter mates are read byte by byte.  No load reaches outside a mate.
    u128 acc = 0;
    uint32_t d = 0;                                                                       // bytes of the run that are in place
    while (d < nvalid) {
        const uint64_t pos = o + d;
        if (pos >= next) {                                                                // (pos < total: there is a next pair)
            ++j; start = next; next = pair_start<LDS>(g, t, j + 1);
            pair_mates<LDS>(g, t, j, l1, o1, o2);
        }
        const uint64_t x = pos - start;
        if (x == l1) { acc |= (u128)'N' << (8 * d); ++d; continue; }
        const bool first = x < l1;
        const uint8_t *mate = first ? g.b1 + o1 : g.b2 + o2;
        const uint64_t mlen = first ? l1 : next - start - l1 - 1, mx = first ? x : x - l1 - 1;   // the mate's length, my place in it
        const uint32_t cnt = mlen - mx < nvalid - d ? (uint32_t)(mlen - mx) : nvalid - d;
        if (mlen >= RUN) {
            int64_t at = (int64_t)mx - (int64_t)d;                                        // where the load would put the piece in place by itself
            at = at < 0 ? 0 : at > (int64_t)(mlen - RUN) ? (int64_t)(mlen - RUN) : at;
            const bytes16 v = *(const bytes16 *)(mate + at);
            u128 w = ((u128)v.b << 64) | v.a;
            const int sh = (int)((int64_t)mx - at) - (int)d;                              // the piece's place in the load minus its place in the run
            w = sh >= 0 ? w >> (8 * sh) : w << (8 * -sh);
            const u128 mask = cnt == RUN ? ~(u128)0 : (((u128)1 << (8 * cnt)) - 1) << (8 * d);
            acc |= w & mask;
        } else
            for (uint32_t k = 0; k < cnt; ++k) acc |= (u128)mate[mx + k] << (8 * (d + k));
        d += cnt;
    }
    const uint64_t a = (uint64_t)acc, b = (uint64_t)(acc >> 64);
    if (nvalid == RUN && ((uintptr_t)dst & 15u) == 0) *(ulonglong2 *)dst = make_ulonglong2(a, b);
    else for (uint32_t i = 0; i < nvalid; ++i) dst[i] = (uint8_t)((i < 8 ? a >> (8 * i) : b >> (8 * (i - 8))) & 0xFFu);
}

__global__ __launch_bounds__(TB) void pairs_gather_k(const uint8_t *__restrict__ b1, const uint64_t *__restrict__ off1, const uint32_t *__restrict__ len1,
                                                     const uint8_t *__restrict__ b2, const uint64_t *__restrict__ off2, const uint32_t *__restrict__ len2,
                                                     uint32_t n, uint8_t *__restrict__ joined, const uint64_t *__restrict__ joff,
                                                     const utree_pairs_meta *__restrict__ meta) {
    __shared__ tile_lds t;
    if (meta->error) return;
    const uint64_t total = meta->total_bases;
    const uint64_t t0 = (uint64_t)blockIdx.x * TILE;
    if (t0 >= total) return;                                                              // (the grid covers the buffer's capacity)
    const uint64_t tend = t0 + TILE < total ? t0 + TILE : total;
    // p0 = the pair byte t0 lies in: the last one whose offset is <= t0 (offsets ascend strictly: a pair has at least its 'N')
    uint32_t lo = 0, hi = n;
    const uint32_t lane = threadIdx.x & 63u;
    while (hi - lo > 1) {
        const uint32_t step = (hi - lo + 63) / 64;
        const uint64_t idx = (uint64_t)lo + (uint64_t)(lane + 1) * step;
        const bool le = idx < hi && joff[idx] <= t0;
        const uint32_t c = (uint32_t)__popcll(__ballot(le));                              // <= 63: the last lane's probe is at or past hi
        lo += c * step;
        hi = hi - lo > step ? lo + step : hi;
    }
    gather_args g = {b1, off1, len1, b2, off2, joff, n, (uint32_t)__builtin_amdgcn_readfirstlane((int)lo), total};
    for (uint32_t j = threadIdx.x; j <= TILE_OFFS; j += TB) {
        const uint64_t idx = (uint64_t)g.p0 + j;
        const bool in = idx < n;
        t.joff[j] = in ? joff[idx] : total;
        if (j < TILE_OFFS) { t.off1[j] = in ? off1[idx] : 0; t.off2[j] = in ? off2[idx] : 0; t.len1[j] = in ? len1[idx] : 0; }
    }
    __syncthreads();
    const bool in_lds = t.joff[TILE_OFFS] >= tend;                                        // every pair of the tile is among those in LDS
    uint32_t jl = 0;
#pragma unroll 1
    for (uint32_t r = 0; r < RUNS; ++r) {                                                 // the thread's runs lie TB * RUN bytes apart: a wave's stores are contiguous
        const uint64_t o = t0 + ((uint64_t)r * TB + threadIdx.x) * RUN;
        if (o >= tend) break;
        const uint32_t nvalid = tend - o < RUN ? (uint32_t)(tend - o) : RUN;
        if (in_lds) gather_run<true>(g, t, t0, o, nvalid, jl, joined + o);
        else gather_run<false>(g, t, t0, o, nvalid, jl, joined + o);
    }
}

}  // namespace

extern "C" int utk_pairs_join(const uint8_t *d_bases1, const uint64_t *d_off1, const uint32_t *d_len1, const uint8_t *d_bases2,
                              const uint64_t *d_off2, const uint32_t *d_len2, uint32_t n_pairs, uint8_t *d_joined, uint64_t joined_capacity,
                              uint64_t *d_joff, uint32_t *d_jlen, utree_pairs_meta *d_meta, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    const uint32_t nb = (uint32_t)(((uint64_t)n_pairs + SCAN_ITEMS - 1) / SCAN_ITEMS);
    const uint64_t tiles = (joined_capacity + TILE - 1) / TILE;
    if (tiles > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    pairs_count_k<<<dim3(nb), dim3(TB), 0, st>>>(d_len1, d_len2, n_pairs, d_joff, d_meta);
    pairs_scan_k<<<dim3(1), dim3(1024), 0, st>>>(d_joff, nb, joined_capacity, d_meta);
    pairs_emit_k<<<dim3(nb), dim3(TB), 0, st>>>(d_len1, d_len2, n_pairs, d_joff, d_jlen);
    if (tiles)
        pairs_gather_k<<<dim3((uint32_t)tiles), dim3(TB), 0, st>>>(d_bases1, d_off1, d_len1, d_bases2, d_off2, d_len2, n_pairs, d_joined, d_joff, d_meta);
    return (int)hipGetLastError();
}
