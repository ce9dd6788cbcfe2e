// tiles_kernels.hip -- the tiles of long queries as VIEWS into the batch's bases (utree_tiles_plan / utree_tiles_views, tiles.c).
//
// A query of L bases has n = 1 (L <= W) or 1 + ceil((L - W) / S) tiles, tile t = q[t*S .. min(t*S + W, L)).  A tile is classified as a
// read of its own by the classify kernels unchanged: they take any (d_bases, d_off, d_len), never write d_bases and never look at a
// read's neighbour, so all that is made here is offsets and lengths -- not a base is copied.
//
//   tl_count_k   per query its tiles; rocprim scans them: tile_first[] (the scan the hit map uses)
//   tl_total_k   the plan's meta record
//   tl_views_k   one thread per tile of the range [first_tile, first_tile + n): its query by binary search in tile_first[] -- queries of one
//                tile and a query of 30 000 sit in one batch, so no thread loops over a query -- then four coalesced stores; the range's
//                bases and its longest tile are reduced per wave, per block, and added to the meta record with one atomic each per block
// Neither kernel needs LDS beyond the four partial sums of a block.  Nothing is kept between calls.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <rocprim/device/device_scan.hpp>
#include "tiles.h"

namespace {

constexpr uint32_t TL_BLOCK = 256;

__global__ void __launch_bounds__(TL_BLOCK) tl_count_k(const uint32_t *__restrict__ len, uint32_t n_reads, uint32_t W, uint32_t S,
                                                       uint64_t *__restrict__ tcnt) {
    const uint64_t i = (uint64_t)blockIdx.x * TL_BLOCK + threadIdx.x;
    if (i > n_reads) return;
    tcnt[i] = i < n_reads ? utk_tiles_of(len[i], W, S) : 0;
}

__global__ void tl_total_k(const uint64_t *__restrict__ tile_first, uint32_t n_reads, utree_tiles_meta *__restrict__ meta) {
    meta->total_tiles = tile_first[n_reads];
    meta->total_bases = 0; meta->max_len = 0; meta->error = 0;
}

// *meta is all zero when the kernel starts
__global__ void __launch_bounds__(TL_BLOCK) tl_views_k(const uint64_t *__restrict__ off, const uint32_t *__restrict__ len, uint32_t n_reads, uint32_t W,
                                                       uint32_t S, const uint64_t *__restrict__ tile_first, uint64_t first_tile, uint32_t n,
                                                       uint64_t *__restrict__ toff, uint32_t *__restrict__ tlen, uint32_t *__restrict__ tquery,
                                                       uint32_t *__restrict__ tindex, utree_tiles_meta *__restrict__ meta) {
    __shared__ uint64_t s_sum[TL_BLOCK / 64];
    __shared__ uint32_t s_max[TL_BLOCK / 64];
    const uint64_t total = tile_first[n_reads];
    const uint32_t j = blockIdx.x * TL_BLOCK + threadIdx.x;                              // n <= 2^21
    if (j == 0) meta->total_tiles = total;
    if (first_tile > total || n > total - first_tile) {                                  // the range ends behind the batch's tiles: nothing is written
        if (j == 0) meta->error = 1;
        return;
    }
    uint64_t sum = 0;
    uint32_t mx = 0;
    if (j < n) {
        const uint64_t g = first_tile + j;                                               // g < total, so n_reads >= 1
        uint32_t lo = 0, hi = n_reads;                                                   // the last query whose first tile is <= g (every query has a tile)
        while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (tile_first[mid] <= g) lo = mid; else hi = mid; }
        const uint64_t t = g - tile_first[lo], start = t * S, L = len[lo];               // t < tiles of lo: start < L, or L == 0 == start
        const uint64_t l = L - start < W ? L - start : W;
        toff[j] = off[lo] + start; tlen[j] = (uint32_t)l; tquery[j] = lo; tindex[j] = (uint32_t)t;
        sum = l; mx = (uint32_t)l;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o);
        const uint32_t m2 = __shfl_xor(mx, o); mx = m2 > mx ? m2 : mx;
    }
    if ((threadIdx.x & 63u) == 0) { s_sum[threadIdx.x >> 6] = sum; s_max[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < TL_BLOCK / 64; ++w) { sum += s_sum[w]; mx = s_max[w] > mx ? s_max[w] : mx; }
        if (sum) atomicAdd((unsigned long long *)&meta->total_bases, (unsigned long long)sum);
        if (mx) atomicMax(&meta->max_len, mx);
    }
}

}  // namespace

extern "C" size_t utk_tiles_scan_temp_bytes(uint32_t n_reads) {
    size_t a = 0;
    if (rocprim::exclusive_scan(nullptr, a, (const uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0, (size_t)n_reads + 1, rocprim::plus<uint64_t>()) != hipSuccess) return 0;
    return a + 256;
}

extern "C" int utk_tiles_plan(const uint32_t *d_len, uint32_t n_reads, uint32_t W, uint32_t S, uint64_t *d_tile_first, utree_tiles_meta *d_meta,
                              const utk_tiles_ws *ws, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    const uint32_t blocks = (uint32_t)(((uint64_t)n_reads + 1 + TL_BLOCK - 1) / TL_BLOCK);
    hipLaunchKernelGGL(tl_count_k, dim3(blocks), dim3(TL_BLOCK), 0, st, d_len, n_reads, W, S, ws->tcnt);
    size_t tb = ws->scan_tmp_bytes;
    if ((e = rocprim::exclusive_scan(ws->scan_tmp, tb, (const uint64_t *)ws->tcnt, d_tile_first, (uint64_t)0, (size_t)n_reads + 1, rocprim::plus<uint64_t>(), st)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(tl_total_k, dim3(1), dim3(1), 0, st, (const uint64_t *)d_tile_first, n_reads, d_meta);
    return (int)hipGetLastError();
}

extern "C" int utk_tiles_views(const uint64_t *d_off, const uint32_t *d_len, uint32_t n_reads, uint32_t W, uint32_t S, const uint64_t *d_tile_first,
                               uint64_t first_tile, uint32_t n_tiles, uint64_t *d_toff, uint32_t *d_tlen, uint32_t *d_tquery, uint32_t *d_tindex,
                               utree_tiles_meta *d_meta, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if ((e = hipMemsetAsync(d_meta, 0, sizeof *d_meta, st)) != hipSuccess) return (int)e;
    const uint32_t blocks = n_tiles ? (n_tiles + TL_BLOCK - 1) / TL_BLOCK : 1;            // (an empty range still writes its meta)
    hipLaunchKernelGGL(tl_views_k, dim3(blocks), dim3(TL_BLOCK), 0, st, d_off, d_len, n_reads, W, S, d_tile_first, first_tile, n_tiles, d_toff, d_tlen,
                       d_tquery, d_tindex, d_meta);
    return (int)hipGetLastError();
}
