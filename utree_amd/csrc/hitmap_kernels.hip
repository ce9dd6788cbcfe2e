// hitmap_kernels.hip -- which label each k-mer window of a query hit, in window order, as runs (utree_hitmap_batch, hitmap.c).
//
// A query q is what the search looks at: the read, or with RC read + 'N' + its reverse complement (itree.c:891-898).  Window p of q has ONE code:
// UTREE_HIT_INVALID when a byte of q[p .. p+k) is no base, else the file-order label index XT_getIX32 gives for its word when that is a label
// (itree.c:929), else UTREE_HIT_MISS.  The map of a query is the list of maximal stretches of equal code, (code, count).
//
//   hm_count_k    per query: its windows, and its ITEMS -- stretches of UTK_HM_SEG window starts of the forward strand (with RC also the windows
//                 that hold the 'N', which are invalid by construction).  rocprim scans both: woff[], ioff[]
//   hm_codes_k    one thread per item, found by binary search in ioff[]: a 150-bp read and a 16-Mb contig load the lanes alike.  The thread
//                 rolls the forward and the reverse-complement word base by base, looks each up ONCE in the image (lookup_word: buckets of
//                 either size, overflow runs and chains, the exact-probe path, the PACKSIZE=16 table) and stores the forward code at
//                 woff[r] + s and the reverse one at woff[r] + 2L+1-k-s: 4 bytes per window.  The item of window 0 marks the query's start
//   hm_heads_k    head(g) = g starts a query || code[g] != code[g-1]; a wavefront per group of 64 windows counts its heads by ballot and notes
//                 its first.  rocprim: heads before each group (the run index of its first head), and -- over the reversed array -- the first
//                 head at or behind each group
//   hm_scatter_k  a head writes (code, next head - itself) at its run index when that is < run_capacity: the next head from the ballot, else
//                 from the scanned array -- no walk however long the run
//   hm_offsets_k  per query the run index of its first window (the heads of at most 63 windows in front of it are counted again); the last
//                 thread writes the meta
// Nothing is kept between calls: every array lies in the caller's workspace, so calls on different streams do not meet.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <rocprim/device/device_scan.hpp>
#include "wave_common.hpp"
#include "hitmap.h"

using namespace utk;

namespace {

constexpr uint32_t HM_BLOCK = 256;

__global__ void __launch_bounds__(HM_BLOCK) hm_count_k(const uint32_t *__restrict__ len, uint32_t n_reads, int do_rc, uint32_t K, utk_hitmap_ws ws) {
    const uint64_t i = (uint64_t)blockIdx.x * HM_BLOCK + threadIdx.x;
    if (i > n_reads) return;
    uint64_t nw = 0, ext = 0;
    if (i < n_reads) {
        const uint64_t L = len[i], qlen = do_rc ? 2 * L + 1 : L;
        nw = qlen >= K ? qlen - K + 1 : 0;
        if (nw > 0xFFFFFFFFull) { atomicMax(ws.flag, 3u); nw = 0; }              // a run's count is 32 bits
        ext = do_rc ? (L + 1 < nw ? L + 1 : nw) : nw;                            // forward windows, then those with the 'N'
    }
    ws.wcnt[i] = nw;
    ws.icnt[i] = (ext + UTK_HM_SEG - 1) / UTK_HM_SEG;
}

__global__ void hm_check_k(uint32_t n_reads, utk_hitmap_ws ws) {
    if (ws.woff[n_reads] > ws.wcap) atomicMax(ws.flag, 2u);                      // the caller's total_bases was too small: nothing is written
}

template <int W, int I, bool EXC, typename OFF> __device__ __forceinline__ uint32_t hit_code(const utk_image &im, uint64_t khi, uint64_t klo) {
    const uint32_t rank = lookup_word<W, I, EXC, OFF>(im, W == 16 ? khi : 0ull, klo);
    if (rank >= im.n_labels) return UTREE_HIT_MISS;
    const uint32_t ix = im.rank2ix[rank];
    return ix < im.n_labels ? ix : UTREE_HIT_MISS;
}

template <int W, int I, bool EXC, typename OFF>
__global__ void __launch_bounds__(HM_BLOCK) hm_codes_k(utk_image im, const uint8_t *__restrict__ bases, const uint64_t *__restrict__ off,
                                                       const uint32_t *__restrict__ len, uint32_t n_reads, int do_rc, utk_hitmap_ws ws) {
    constexpr uint32_t K = 4 * W;
    if (*ws.flag) return;
    const uint64_t n_items = ws.ioff[n_reads];
    for (uint64_t it = (uint64_t)blockIdx.x * HM_BLOCK + threadIdx.x; it < n_items; it += (uint64_t)gridDim.x * HM_BLOCK) {
        uint32_t lo = 0, hi = n_reads;                            // the last query whose first item is <= it (queries without items share theirs with the next)
        while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (ws.ioff[mid] <= it) lo = mid; else hi = mid; }
        const uint32_t r = lo;
        const uint64_t L = len[r], o = off[r], wbase = ws.woff[r], nw = ws.wcnt[r];
        const uint64_t fw = L >= K ? L - K + 1 : 0;               // windows of the forward strand
        const uint64_t ext = do_rc ? (L + 1 < nw ? L + 1 : nw) : nw;
        const uint64_t w0 = (it - ws.ioff[r]) * UTK_HM_SEG;
        const uint64_t w1 = w0 + UTK_HM_SEG < ext ? w0 + UTK_HM_SEG : ext;
        if (w0 == 0) atomicOr(&ws.starts[wbase >> 5], 1u << (wbase & 31u));
        uint64_t fhi = 0, flo = 0, rhi = 0, rlo = 0;
        uint32_t ok = 0;                                          // bases in a row up to here
        for (uint64_t j = w0; j < w1 + K - 1; ++j) {
            bool bad = true;
            uint32_t b = 0;
            if (j < L) { b = bases[o + j]; const uint32_t u = b & 0xDFu; bad = !(u == 'A' || u == 'C' || u == 'G' || u == 'T'); }   // (behind the read: the 'N')
            if (bad) ok = 0;
            else {
                const uint32_t g = (b >> 1) & 3u;
                const uint64_t code = g ^ (g >> 1), comp = code ^ 3u;            // A 0, C 1, G 2, T 3 (itree.c:110-121)
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
                ++ok;
            }
            if (j + 1 < w0 + K) continue;
            const uint64_t s = j + 1 - K;                                        // the window that ends at j: w0 <= s < w1 <= nw
            uint32_t fc = UTREE_HIT_INVALID, rc = UTREE_HIT_INVALID;
            if (ok >= K) {
                fc = hit_code<W, I, EXC, OFF>(im, fhi, flo);
                if (do_rc) rc = hit_code<W, I, EXC, OFF>(im, rhi, rlo);
            }
            ws.codes[wbase + s] = fc;
            if (do_rc && s < fw) ws.codes[wbase + (2 * L + 1 - K - s)] = rc;     // L + 1 <= 2L+1-k-s <= 2L+1-k < nw
        }
    }
}

__device__ __forceinline__ bool is_head(const utk_hitmap_ws &ws, uint64_t g, uint64_t total) {
    if (g >= total) return false;
    if (g == 0 || ((ws.starts[g >> 5] >> (g & 31u)) & 1u)) return true;
    return ws.codes[g] != ws.codes[g - 1];
}

__global__ void __launch_bounds__(HM_BLOCK) hm_heads_k(uint32_t n_reads, utk_hitmap_ws ws) {
    const uint64_t total = *ws.flag ? 0 : ws.woff[n_reads];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_waves = (uint64_t)gridDim.x * (HM_BLOCK / 64);
    for (uint64_t grp = (uint64_t)blockIdx.x * (HM_BLOCK / 64) + (threadIdx.x >> 6); grp <= ws.n_groups; grp += n_waves) {
        const uint64_t m = __ballot(is_head(ws, grp * UTK_HM_GROUP + lane, total));
        if (lane == 0) {
            ws.gcnt[grp] = (uint64_t)__popcll(m);
            ws.gfirst[ws.n_groups - grp] = m ? grp * UTK_HM_GROUP + (uint64_t)(__ffsll((unsigned long long)m) - 1) : ~0ull;
        }
    }
}

__global__ void __launch_bounds__(HM_BLOCK) hm_scatter_k(uint32_t n_reads, utk_hitmap_ws ws, utree_hit_run *__restrict__ runs, uint64_t cap) {
    if (*ws.flag) return;
    const uint64_t total = ws.woff[n_reads];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_waves = (uint64_t)gridDim.x * (HM_BLOCK / 64);
    for (uint64_t grp = (uint64_t)blockIdx.x * (HM_BLOCK / 64) + (threadIdx.x >> 6); grp * UTK_HM_GROUP < total; grp += n_waves) {
        const uint64_t g = grp * UTK_HM_GROUP + lane;
        const bool h = is_head(ws, g, total);
        const uint64_t m = __ballot(h);
        if (!h) continue;
        const uint64_t idx = ws.gbase[grp] + lanes_below(m);
        if (idx >= cap) continue;                                                // never written: the caller sizes the array from the meta
        const uint64_t above = lane == 63u ? 0ull : m >> (lane + 1u);
        uint64_t next;
        if (above) next = g + (uint64_t)__ffsll((unsigned long long)above);
        else { next = ws.gnext[ws.n_groups - (grp + 1)]; if (next > total) next = total; }   // (no head behind: the batch's end)
        utree_hit_run run;
        run.code = ws.codes[g]; run.count = (uint32_t)(next - g);
        runs[idx] = run;
    }
}

__global__ void __launch_bounds__(HM_BLOCK) hm_offsets_k(uint32_t n_reads, utk_hitmap_ws ws, uint64_t *__restrict__ run_off, uint64_t cap,
                                                         utree_hitmap_meta *__restrict__ meta) {
    const uint64_t r = (uint64_t)blockIdx.x * HM_BLOCK + threadIdx.x;
    if (r > n_reads) return;
    const uint32_t flag = *ws.flag;
    const uint64_t total = flag ? 0 : ws.woff[n_reads];
    uint64_t idx = 0;
    if (!flag) {
        const uint64_t g = ws.woff[r], g0 = g & ~(uint64_t)(UTK_HM_GROUP - 1);    // g <= total <= wcap: a group the scan covers
        idx = ws.gbase[g >> 6];
        for (uint64_t x = g0; x < g; ++x) idx += is_head(ws, x, total);
    }
    run_off[r] = idx;
    if (r == n_reads) {
        meta->total_runs = flag ? 0 : ws.gbase[ws.n_groups];
        meta->total_windows = total;
        meta->error = flag ? flag : (meta->total_runs > cap ? 1u : 0u);
        meta->pad = 0;
    }
}

uint32_t grid_for(uint64_t threads, int n_cu, uint32_t per_cu) {
    const uint64_t want = (threads + HM_BLOCK - 1) / HM_BLOCK, cap = (uint64_t)(n_cu > 0 ? n_cu : 256) * per_cu;
    return (uint32_t)(want < 1 ? 1 : want < cap ? want : cap);
}

}  // namespace

extern "C" size_t utk_hitmap_scan_temp_bytes(uint32_t n_reads, uint64_t n_groups) {
    size_t a = 0, b = 0, c = 0;
    if (rocprim::exclusive_scan(nullptr, a, (const uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0, (size_t)n_reads + 1, rocprim::plus<uint64_t>()) != hipSuccess) return 0;
    if (rocprim::exclusive_scan(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0, (size_t)n_groups + 1, rocprim::plus<uint64_t>()) != hipSuccess) return 0;
    if (rocprim::inclusive_scan(nullptr, c, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)n_groups + 1, rocprim::minimum<uint64_t>()) != hipSuccess) return 0;
    if (b > a) a = b;
    if (c > a) a = c;
    return a + 256;
}

extern "C" int utk_hitmap_run(const utk_image *im, const uint8_t *d_bases, const uint64_t *d_off, const uint32_t *d_len, uint32_t n_reads,
                              uint64_t total_bases, int do_rc, uint64_t *d_run_off, utree_hit_run *d_runs, uint64_t run_capacity,
                              utree_hitmap_meta *d_meta, const utk_hitmap_ws *ws, int n_cu, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    size_t tb;
    const uint32_t read_blocks = (uint32_t)(((uint64_t)n_reads + 1 + HM_BLOCK - 1) / HM_BLOCK);
    if ((e = hipMemsetAsync(ws->flag, 0, sizeof *ws->flag, st)) != hipSuccess) return (int)e;
    if ((e = hipMemsetAsync(ws->starts, 0, ((size_t)(ws->wcap >> 5) + 2) * 4, st)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(hm_count_k, dim3(read_blocks), dim3(HM_BLOCK), 0, st, d_len, n_reads, do_rc, 4u * im->W, *ws);
    tb = ws->scan_tmp_bytes;
    if ((e = rocprim::exclusive_scan(ws->scan_tmp, tb, (const uint64_t *)ws->wcnt, ws->woff, (uint64_t)0, (size_t)n_reads + 1, rocprim::plus<uint64_t>(), st)) != hipSuccess) return (int)e;
    tb = ws->scan_tmp_bytes;
    if ((e = rocprim::exclusive_scan(ws->scan_tmp, tb, (const uint64_t *)ws->icnt, ws->ioff, (uint64_t)0, (size_t)n_reads + 1, rocprim::plus<uint64_t>(), st)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(hm_check_k, dim3(1), dim3(1), 0, st, n_reads, *ws);
    if (n_reads) {
        const uint64_t items = total_bases / UTK_HM_SEG + 2ull * n_reads;        // (an upper bound: the kernel strides over what there is)
        const int drc = dispatch_img_all(im, [&](auto w, auto i, auto exc, auto offt) {
            hipLaunchKernelGGL((hm_codes_k<decltype(w)::value, decltype(i)::value, decltype(exc)::value, decltype(offt)>), dim3(grid_for(items, n_cu, 32)),
                               dim3(HM_BLOCK), 0, st, *im, d_bases, d_off, d_len, n_reads, do_rc, *ws);
        });
        if (drc) return drc;
    }
    hipLaunchKernelGGL(hm_heads_k, dim3(grid_for((ws->n_groups + 1) * 64, n_cu, 32)), dim3(HM_BLOCK), 0, st, n_reads, *ws);
    tb = ws->scan_tmp_bytes;
    if ((e = rocprim::exclusive_scan(ws->scan_tmp, tb, (const uint64_t *)ws->gcnt, ws->gbase, (uint64_t)0, (size_t)ws->n_groups + 1, rocprim::plus<uint64_t>(), st)) != hipSuccess) return (int)e;
    tb = ws->scan_tmp_bytes;
    if ((e = rocprim::inclusive_scan(ws->scan_tmp, tb, (const uint64_t *)ws->gfirst, ws->gnext, (size_t)ws->n_groups + 1, rocprim::minimum<uint64_t>(), st)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(hm_scatter_k, dim3(grid_for((ws->n_groups + 1) * 64, n_cu, 32)), dim3(HM_BLOCK), 0, st, n_reads, *ws, d_runs, run_capacity);
    hipLaunchKernelGGL(hm_offsets_k, dim3(read_blocks), dim3(HM_BLOCK), 0, st, n_reads, *ws, d_run_off, run_capacity, d_meta);
    return (int)hipGetLastError();
}
