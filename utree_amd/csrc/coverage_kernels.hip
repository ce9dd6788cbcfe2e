// coverage_kernels.hip -- which database k-mers a sample touched (utree_coverage_*, coverage.c).
//
// coverage_add_k    reads -> windows (itree.c:903-927: every k-base window of ACGTacgt bytes; with RC also its reverse complement) -> XT_getIX32
//                   over the node dump in file order (itree.c:720-730 with the probe of 699-707) -> for a hit (stored index < n_labels, 929) the
//                   bit of the record's position in a bitmap of n_nodes bits, and one count for the record's label.
// coverage_count_k  one streaming pass over dump and bitmap -> per label the records the dump holds and those whose bit is set.
//
// The node POSITION is what the report needs, and the bucketed image cannot give it (a k-mer may sit there under two views, in an overflow
// run or as part of a chain), so these kernels probe the .ctr's own bin table and packed records, kept in HBM by the coverage handle.  They are
// independent of the search kernels: a window is rolled base by base and looked up the reference's way.
//
// Work: an ITEM is COV_SEG consecutive window starts of one read, one thread per item.  A workgroup takes a tile of reads, scans their item
// counts in LDS and deals the items out to its threads, so a tile of 150-bp reads (four items each) and a tile that holds one 100-kb read keep
// all lanes busy alike.  Reads of more than COV_PIECE_SEGS items are left to a second launch whose grid has COV_LONG_Y workgroups per tile, each
// taking an equal stretch of every such read: a 16-Mb read goes over COV_LONG_Y x 4 waves.
//
// A real sample hits the same nodes and the same labels over and over (MI355X_MICROARCH.md: ~88 returning atomics per us on ONE word):
//  * the bit is tested with a plain load first and set with an atomic OR that returns nothing only when it is not there yet (a stale zero from the
//    vector cache costs one redundant OR, never a wrong bit);
//  * a thread keeps a run of equal labels in registers, a workgroup counts in LDS (dense counters for the first COV_DENSE labels, a small hash
//    table for the rest) and adds its non-zero slots to the device counters at its end, one no-return atomic each, as profile_add_k does.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "coverage.h"

namespace {

constexpr uint32_t COV_BLOCK = 256;
constexpr uint32_t COV_SEG = 32;            // window starts per item
constexpr uint32_t COV_PIECE_SEGS = 128;    // reads of up to this many items (4096 windows) go through the short launch
constexpr uint32_t COV_TILE = 256;          // reads per workgroup, short launch
constexpr uint32_t COV_LONG_TILE = 4096;    // ... long launch (it only looks for the long ones)
constexpr uint32_t COV_LONG_Y = 32;         // workgroups that share a long read
constexpr uint32_t COV_DENSE = 2048;        // labels counted by index in LDS
constexpr uint32_t COV_HSLOTS = 1024;       // LDS hash slots for the other labels
constexpr uint32_t COV_LDS_PROBES = 16;
constexpr uint32_t KEY_FREE = 0xFFFFFFFFu;  // (labels are < n_labels <= 0xFFFFFFFF)
constexpr uint64_t M40 = (1ull << 40) - 1;

__device__ __forceinline__ void dev_add(unsigned long long *p, unsigned long long v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- per-workgroup label counters ----------------------------------------------------------------------------------------------
struct CovLds {
    uint32_t dense[COV_DENSE];
    uint32_t key[COV_HSLOTS];
    uint32_t cnt[COV_HSLOTS];
};

__device__ void lds_init(CovLds &s, uint32_t n_dense) {
    for (uint32_t i = threadIdx.x; i < n_dense; i += COV_BLOCK) s.dense[i] = 0;
    for (uint32_t i = threadIdx.x; i < COV_HSLOTS; i += COV_BLOCK) { s.key[i] = KEY_FREE; s.cnt[i] = 0; }
}

__device__ void lds_add(CovLds &s, uint32_t label, uint32_t cnt, uint32_t n_dense, unsigned long long *d_counts) {
    if (!cnt) return;
    if (label < n_dense) { atomicAdd(&s.dense[label], cnt); return; }
    const uint32_t h = label * 0x9E3779B1u >> 22;
    for (uint32_t p = 0; p < COV_LDS_PROBES; ++p) {
        const uint32_t i = (h + p) & (COV_HSLOTS - 1);
        uint32_t k = s.key[i];
        if (k == KEY_FREE) {
            k = atomicCAS(&s.key[i], KEY_FREE, label);
            if (k == KEY_FREE) k = label;
        }
        if (k == label) { atomicAdd(&s.cnt[i], cnt); return; }
    }
    dev_add(d_counts + label, cnt);          // no room in the workgroup's table
}

// (after a __syncthreads) the dense counters go out in label order: a wave's adds land on consecutive words
__device__ void lds_flush(const CovLds &s, uint32_t n_dense, unsigned long long *d_counts) {
    for (uint32_t i = threadIdx.x; i < n_dense; i += COV_BLOCK)
        if (s.dense[i]) dev_add(d_counts + i, s.dense[i]);
    for (uint32_t i = threadIdx.x; i < COV_HSLOTS; i += COV_BLOCK)
        if (s.key[i] != KEY_FREE && s.cnt[i]) dev_add(d_counts + s.key[i], s.cnt[i]);
}

// ---- the packed node dump ---------------------------------------------------------------------------------------------------------
// eight bytes at byte address a of the dump (little endian), from the two aligned words that hold them (UTK_COV_PAD: the second one exists)
__device__ __forceinline__ uint64_t load8(const uint64_t *__restrict__ recs, uint64_t a) {
    const uint64_t q = a >> 3;
    const uint32_t sh = (uint32_t)(a & 7u) * 8u;
    const uint64_t x = recs[q], y = recs[q + 1];
    return sh ? (x >> sh) | (y << (64u - sh)) : x;
}

template <int W, int I> __device__ __forceinline__ uint32_t rec_ix(const uint64_t *__restrict__ recs, uint64_t p) {
    constexpr uint64_t SZ = W + I - 3;
    const uint64_t v = load8(recs, p * SZ + (W - 3));
    return I == 2 ? (uint32_t)v & 0xFFFFu : (uint32_t)v;
}

// stored suffix of record p <= the query's?  (eq: are they equal)
template <int W, int I> __device__ __forceinline__ bool rec_le(const uint64_t *__restrict__ recs, uint64_t p, uint64_t qhi, uint64_t qlo, bool &eq) {
    constexpr uint64_t SZ = W + I - 3;
    if constexpr (W == 16) {
        const uint64_t lo = load8(recs, p * SZ), hi = load8(recs, p * SZ + 8) & M40;
        eq = hi == qhi && lo == qlo;
        return hi < qhi || (hi == qhi && lo <= qlo);
    } else {
        const uint64_t lo = load8(recs, p * SZ) & (W == 8 ? M40 : 0xFFull);
        eq = lo == qlo;
        return lo <= qlo;
    }
}

// XT_getIX32 over the dump: the position of the record the lookup ends on when that record is a hit, else ~0
template <int W, int I, typename OT>
__device__ __forceinline__ uint64_t probe(const utk_cov_db &db, uint64_t khi, uint64_t klo, uint32_t &label) {
    uint32_t pre;
    uint64_t qhi = 0, qlo;
    if constexpr (W == 16) { pre = (uint32_t)(khi >> 40); qhi = khi & M40; qlo = klo; }
    else if constexpr (W == 8) { pre = (uint32_t)(klo >> 40); qlo = klo & M40; }
    else { pre = (uint32_t)(klo >> 8) & 0xFFFFFFu; qlo = klo & 0xFFull; }
    const OT *bx = (const OT *)db.binix;
    uint64_t s = bx[pre], e = bx[pre + 1];
    if (e > db.n_nodes) e = db.n_nodes;              // (a bin table that points past the dump: never read there)
    if (s >= e) return ~0ull;
    uint64_t pos = s, size = e - s - 1;
    bool eq;
    while (size) {
        const uint64_t w = size >> 1;
        if (rec_le<W, I>(db.recs, pos + w + 1, qhi, qlo, eq)) { pos += w + 1; size -= w + 1; }
        else size = w;
    }
    (void)rec_le<W, I>(db.recs, pos, qhi, qlo, eq);
    if (!eq) return ~0ull;
    label = rec_ix<W, I>(db.recs, pos);
    return label < db.n_labels ? pos : ~0ull;
}

__device__ __forceinline__ void mark(uint32_t *__restrict__ bitmap, uint64_t p) {
    uint32_t *w = bitmap + (p >> 5);
    const uint32_t m = 1u << (p & 31u);
    if (!(*w & m)) (void)__hip_atomic_fetch_or(w, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- reads -> hits ------------------------------------------------------------------------------------------------------------------
// items of read r for workgroup row y: {first item, count}
template <int W, bool LONG> __device__ __forceinline__ void read_items(uint32_t len, uint32_t y, uint64_t &first, uint64_t &count) {
    constexpr uint32_t K = 4 * W;
    const uint64_t nwin = len >= K ? (uint64_t)len - K + 1 : 0;
    const uint64_t nseg = (nwin + COV_SEG - 1) / COV_SEG;
    if constexpr (!LONG) { first = 0; count = nseg <= COV_PIECE_SEGS ? nseg : 0; }
    else if (nseg <= COV_PIECE_SEGS) { first = 0; count = 0; }
    else { first = nseg * y / COV_LONG_Y; count = nseg * (y + 1) / COV_LONG_Y - first; }
}

template <int W, int I, typename OT, bool LONG>
__global__ void __launch_bounds__(COV_BLOCK) coverage_add_k(utk_cov_db db, const uint8_t *__restrict__ bases, const uint64_t *__restrict__ off,
                                                            const uint32_t *__restrict__ len, uint32_t n_reads, int do_rc,
                                                            uint32_t *__restrict__ bitmap, unsigned long long *__restrict__ d_hits,
                                                            unsigned long long *__restrict__ d_reads) {
    constexpr uint32_t K = 4 * W;
    constexpr uint32_t TILE = LONG ? COV_LONG_TILE : COV_TILE, RPT = TILE / COV_BLOCK;
    __shared__ CovLds s;
    __shared__ uint64_t s_start[TILE + 1];
    __shared__ uint64_t s_wave[COV_BLOCK / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6, y = blockIdx.y;
    const uint64_t r0 = (uint64_t)blockIdx.x * TILE;
    if (!LONG && blockIdx.x == 0 && tid == 0) dev_add(d_reads, n_reads);

    // the tile's item counts, scanned: thread t has reads r0 + t * RPT ...
    uint64_t cnt[RPT], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < RPT; ++j) {
        const uint64_t r = r0 + (uint64_t)tid * RPT + j;
        uint64_t first;
        cnt[j] = 0;
        if (r < n_reads) read_items<W, LONG>(len[r], y, first, cnt[j]);
        sum += cnt[j];
    }
    uint64_t x = sum;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) { const uint64_t v = __shfl_up(x, d); if (lane >= d) x += v; }
    if (lane == 63) s_wave[wv] = x;
    __syncthreads();
    uint64_t before = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < COV_BLOCK / 64; ++w) { if (w < wv) before += s_wave[w]; total += s_wave[w]; }
    if (!total) return;                                       // (uniform) nothing here for this workgroup: the long launch on short reads
    uint64_t at = before + x - sum;
#pragma unroll
    for (uint32_t j = 0; j < RPT; ++j) { s_start[tid * RPT + j] = at; at += cnt[j]; }
    if (tid == COV_BLOCK - 1) s_start[TILE] = total;
    const uint32_t n_dense = db.n_labels < COV_DENSE ? db.n_labels : COV_DENSE;
    lds_init(s, n_dense);
    __syncthreads();

    uint32_t run_lab = KEY_FREE, run_n = 0;
    for (uint64_t it = tid; it < total; it += COV_BLOCK) {
        uint32_t lo = 0, hi = TILE;                           // the last read whose start is <= it (reads without items share a start with the next)
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (s_start[mid] <= it) lo = mid; else hi = mid; }
        const uint64_t r = r0 + lo;
        const uint32_t L = len[r];
        const uint64_t o = off[r];
        uint64_t first, n_it;
        read_items<W, LONG>(L, y, first, n_it);
        const uint64_t w0 = (first + (it - s_start[lo])) * COV_SEG;       // first window start of the item
        const uint64_t nwin = (uint64_t)L - K + 1;
        const uint64_t w1 = w0 + COV_SEG < nwin ? w0 + COV_SEG : nwin;    // one past its last
        uint64_t fhi = 0, flo = 0, rhi = 0, rlo = 0;
        uint32_t ok = 0;                                                  // ACGT bytes in a row up to here
        for (uint64_t j = w0; j < w1 + K - 1; ++j) {
            const uint32_t b = bases[o + j], u = b & 0xDFu;
            if (!(u == 'A' || u == 'C' || u == 'G' || u == 'T')) { ok = 0; continue; }
            const uint32_t g = (b >> 1) & 3u;
            const uint64_t code = g ^ (g >> 1), comp = code ^ 3u;         // A 0, C 1, G 2, T 3 (itree.c:110-121)
            if constexpr (W == 16) {
                fhi = (fhi << 2) | (flo >> 62); flo = (flo << 2) | code;
                rlo = (rlo >> 2) | (rhi << 62); rhi = (rhi >> 2) | (comp << 62);
            } else if constexpr (W == 8) {
                flo = (flo << 2) | code;
                rlo = (rlo >> 2) | (comp << 62);
            } else {
                flo = ((flo << 2) | code) & 0xFFFFFFFFull;
                rlo = (rlo >> 2) | (comp << 30);
            }
            if (++ok < K) continue;
            for (int strand = 0; strand < (do_rc ? 2 : 1); ++strand) {
                uint32_t label = 0;
                const uint64_t p = strand ? probe<W, I, OT>(db, rhi, rlo, label) : probe<W, I, OT>(db, fhi, flo, label);
                if (p == ~0ull) continue;
                mark(bitmap, p);
                if (label == run_lab) ++run_n;
                else { lds_add(s, run_lab, run_n, n_dense, d_hits); run_lab = label; run_n = 1; }
            }
        }
    }
    lds_add(s, run_lab, run_n, n_dense, d_hits);
    __syncthreads();
    lds_flush(s, n_dense, d_hits);
}

// ---- dump + bitmap -> per-label figures -------------------------------------------------------------------------------------------------
template <int W, int I>
__global__ void __launch_bounds__(COV_BLOCK) coverage_count_k(utk_cov_db db, const uint32_t *__restrict__ bitmap, uint64_t per_block,
                                                              unsigned long long *__restrict__ d_db, unsigned long long *__restrict__ d_cov) {
    __shared__ CovLds s_db, s_cov;
    const uint32_t n_dense = db.n_labels < COV_DENSE ? db.n_labels : COV_DENSE;
    lds_init(s_db, n_dense);
    lds_init(s_cov, n_dense);
    __syncthreads();
    const uint64_t begin = (uint64_t)blockIdx.x * per_block;
    const uint64_t end = begin + per_block < db.n_nodes ? begin + per_block : db.n_nodes;
    for (uint64_t p = begin + threadIdx.x; p < end; p += COV_BLOCK) {
        const uint32_t ix = rec_ix<W, I>(db.recs, p);
        if (ix >= db.n_labels) continue;
        lds_add(s_db, ix, 1, n_dense, d_db);
        if (bitmap[p >> 5] >> (p & 31u) & 1u) lds_add(s_cov, ix, 1, n_dense, d_cov);
    }
    __syncthreads();
    lds_flush(s_db, n_dense, d_db);
    lds_flush(s_cov, n_dense, d_cov);
}

__global__ void __launch_bounds__(COV_BLOCK) coverage_or_k(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * COV_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * COV_BLOCK) dst[i] |= src[i];
}
__global__ void __launch_bounds__(COV_BLOCK) coverage_sum_k(unsigned long long *__restrict__ dst, const unsigned long long *__restrict__ src, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * COV_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * COV_BLOCK) dst[i] += src[i];
}

template <int V> using IC = std::integral_constant<int, V>;
template <typename Fn> int dispatch_wi(uint32_t W, uint32_t I, Fn &&fn) {
    if (W == 4 && I == 2) fn(IC<4>{}, IC<2>{});
    else if (W == 4 && I == 4) fn(IC<4>{}, IC<4>{});
    else if (W == 8 && I == 2) fn(IC<8>{}, IC<2>{});
    else if (W == 8 && I == 4) fn(IC<8>{}, IC<4>{});
    else if (W == 16 && I == 2) fn(IC<16>{}, IC<2>{});
    else if (W == 16 && I == 4) fn(IC<16>{}, IC<4>{});
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

template <int W, int I, typename OT>
void launch_add(const utk_cov_db &db, const uint8_t *d_bases, const uint64_t *d_off, const uint32_t *d_len, uint32_t n_reads, int do_rc,
                uint32_t *bitmap, unsigned long long *d_hits, unsigned long long *d_reads, hipStream_t st) {
    const uint32_t tiles = (n_reads + COV_TILE - 1) / COV_TILE, long_tiles = (n_reads + COV_LONG_TILE - 1) / COV_LONG_TILE;
    hipLaunchKernelGGL((coverage_add_k<W, I, OT, false>), dim3(tiles), dim3(COV_BLOCK), 0, st, db, d_bases, d_off, d_len, n_reads, do_rc,
                       bitmap, d_hits, d_reads);
    hipLaunchKernelGGL((coverage_add_k<W, I, OT, true>), dim3(long_tiles, COV_LONG_Y), dim3(COV_BLOCK), 0, st, db, d_bases, d_off, d_len,
                       n_reads, do_rc, bitmap, d_hits, d_reads);
}

}  // namespace

extern "C" int utk_coverage_add(const utk_cov_db *db, const uint8_t *d_bases, const uint64_t *d_off, const uint32_t *d_len, uint32_t n_reads,
                                int do_rc, uint32_t *bitmap, unsigned long long *d_hits, unsigned long long *d_reads, void *stream) {
    if (!n_reads) return 0;
    return dispatch_wi(db->W, db->I, [&](auto w, auto i) {
        if (db->off64) launch_add<decltype(w)::value, decltype(i)::value, uint64_t>(*db, d_bases, d_off, d_len, n_reads, do_rc, bitmap, d_hits, d_reads, (hipStream_t)stream);
        else launch_add<decltype(w)::value, decltype(i)::value, uint32_t>(*db, d_bases, d_off, d_len, n_reads, do_rc, bitmap, d_hits, d_reads, (hipStream_t)stream);
    });
}

extern "C" int utk_coverage_count(const utk_cov_db *db, const uint32_t *bitmap, unsigned long long *d_db, unsigned long long *d_cov, int n_cu,
                                  void *stream) {
    if (!db->n_nodes) return 0;
    // a workgroup's LDS counters are 32-bit: at most 2^31 records each; otherwise four workgroups per CU over contiguous stretches
    uint64_t blocks = (uint64_t)(n_cu > 0 ? n_cu : 256) * 4;
    const uint64_t min_per = 16u * COV_BLOCK;
    if ((db->n_nodes + min_per - 1) / min_per < blocks) blocks = (db->n_nodes + min_per - 1) / min_per;
    if ((db->n_nodes + blocks - 1) / blocks > (1ull << 31)) blocks = (db->n_nodes + (1ull << 31) - 1) >> 31;
    const uint64_t per = (db->n_nodes + blocks - 1) / blocks;
    return dispatch_wi(db->W, db->I, [&](auto w, auto i) {
        hipLaunchKernelGGL((coverage_count_k<decltype(w)::value, decltype(i)::value>), dim3((uint32_t)blocks), dim3(COV_BLOCK), 0,
                           (hipStream_t)stream, *db, bitmap, per, d_db, d_cov);
    });
}

extern "C" int utk_coverage_or(uint32_t *dst, const uint32_t *src, uint64_t n, void *stream) {
    if (!n) return 0;
    const uint64_t want = (n + COV_BLOCK - 1) / COV_BLOCK;
    hipLaunchKernelGGL(coverage_or_k, dim3((uint32_t)(want < 4096 ? want : 4096)), dim3(COV_BLOCK), 0, (hipStream_t)stream, dst, src, n);
    return (int)hipGetLastError();
}

extern "C" int utk_coverage_sum(unsigned long long *dst, const unsigned long long *src, uint64_t n, void *stream) {
    if (!n) return 0;
    const uint64_t want = (n + COV_BLOCK - 1) / COV_BLOCK;
    hipLaunchKernelGGL(coverage_sum_k, dim3((uint32_t)(want < 4096 ? want : 4096)), dim3(COV_BLOCK), 0, (hipStream_t)stream, dst, src, n);
    return (int)hipGetLastError();
}
