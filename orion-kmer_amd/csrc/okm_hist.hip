// okm_hist.hip — the count histogram (abundance spectrum) of a counted table,
// read where the table lies (okm_count_histogram): hist[min(count, n_bins - 1)]
// += 1 per distinct key, plus the table's entries, the sum of its counts and
// its largest count.  Only counts are read, never keys.
//
// Binning.  A spectrum can be concentrated (all of a wave's counts in a few
// low bins), and 64 lanes of LDS atomics then queue on a few addresses.  Each
// lane therefore keeps the counts 1..kHistRegs in registers of its own (one
// compare + add per bin and entry, no memory access, the same cost for every
// spectrum); only the rest goes to the workgroup's LDS histogram (bins below
// kHistLds) or, above that, straight to the global histogram.  The count is
// clamped to the last bin BEFORE the path is chosen.  At the end the registers
// are summed per wave and added to the LDS bins, and the workgroup flushes its
// non-zero LDS bins with one global atomic each.  OKM_HIST_NAIVE (a build
// flag, for the A/B in profiles/AB_LOG.md) drops the registers: every entry
// below kHistLds is a per-lane LDS atomic.
//
// Grid.  Every workgroup ends on the same few words (the summary, the hot low
// bins), and atomics on one line queue at the memory side: with 4096
// workgroups of 256 threads and one summary update per wave, that queue was
// the whole kernel (0.63 ms at C2 whatever the walk and the binning did,
// profiles/AB_LOG.md).  Hence few, large workgroups -- at most one of 1024
// threads per CU -- and one set of global atomics per workgroup.
#include <hip/hip_runtime.h>

#include "okm_dev_common.h"
#include "okm_internal.h"

namespace okm {

constexpr uint32_t kHistLds = 4096;  // low bins a workgroup keeps in LDS (u32 each: 16 KB)
constexpr int kHistRegs = 8;         // counts 1..kHistRegs: per-lane registers
constexpr int kHistFly = 8;          // pending walk: loads in flight per lane
constexpr int kHistBlock = 1024;     // 16 waves: few, large workgroups keep the end-of-kernel atomics few
constexpr uint32_t kHistGrid = 256;  // workgroups at most, one per CU (a lane or an LDS bin sees < 2^32 entries up to 2^50)

struct HistAcc {
    uint32_t r[kHistRegs];
    ull n, sum, mx;
};

__device__ __forceinline__ void hist_init(HistAcc &a, uint32_t *lds, uint32_t nlds) {
#pragma unroll
    for (int q = 0; q < kHistRegs; ++q) a.r[q] = 0;
    a.n = a.sum = a.mx = 0;
    for (uint32_t b = threadIdx.x; b < nlds; b += blockDim.x) lds[b] = 0;
    __syncthreads();
}

// One entry.  last = n_bins - 1 (the bin of every count >= last); nlds =
// min(n_bins, kHistLds).
__device__ __forceinline__ void hist_add(HistAcc &a, uint64_t c, uint64_t last, uint32_t nlds, uint32_t *lds,
                                         ull *__restrict__ hist) {
    a.n += 1;
    a.sum += c;
    a.mx = c > a.mx ? c : a.mx;
    const uint64_t b = c < last ? c : last;  // clamp first: 5e9 lands in the last bin whatever its path
#ifndef OKM_HIST_NAIVE
    const uint32_t lo = b <= (uint64_t)kHistRegs ? (uint32_t)b : 0u;
#pragma unroll
    for (int q = 0; q < kHistRegs; ++q) a.r[q] += lo == (uint32_t)(q + 1) ? 1u : 0u;
    if (lo) return;
#endif
    if (b < nlds)
        atomicAdd(&lds[(uint32_t)b], 1u);
    else
        atomicAdd(&hist[b], 1ull);
}

__device__ __forceinline__ ull wave_sum(ull v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ ull wave_max(ull v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const ull o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// Every wave of the workgroup calls this once (no early return before it).
// summary: [0] += entries, [1] += sum of counts (mod 2^64), [2] = max count.
__device__ __forceinline__ void hist_flush(HistAcc &a, uint32_t nlds, uint32_t *lds, ull *__restrict__ hist,
                                           ull *__restrict__ summary) {
    const bool lead = (threadIdx.x & 63u) == 0;
#ifndef OKM_HIST_NAIVE
#pragma unroll
    for (int q = 0; q < kHistRegs; ++q) {
        const ull t = wave_sum(a.r[q]);
        // t > 0 implies q + 1 <= last < n_bins (a clamped count): the bin exists
        if (lead && t) {
            if ((uint32_t)(q + 1) < nlds)
                atomicAdd(&lds[q + 1], (uint32_t)t);
            else
                atomicAdd(&hist[q + 1], t);
        }
    }
#endif
    // one summary update per workgroup (see "Grid" above)
    __shared__ ull wred[3][kHistBlock / 64];
    const ull n = wave_sum(a.n), s = wave_sum(a.sum), m = wave_max(a.mx);
    if (lead) {
        wred[0][threadIdx.x >> 6] = n;
        wred[1][threadIdx.x >> 6] = s;
        wred[2][threadIdx.x >> 6] = m;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ull bn = 0, bs = 0, bm = 0;
        for (uint32_t w = 0; w < blockDim.x / 64u; ++w) {
            bn += wred[0][w];
            bs += wred[1][w];
            bm = wred[2][w] > bm ? wred[2][w] : bm;
        }
        if (bn) {
            atomicAdd(&summary[0], bn);
            atomicAdd(&summary[1], bs);
            atomicMax(&summary[2], bm);
        }
    }
    for (uint32_t b = threadIdx.x; b < nlds; b += blockDim.x) {
        const uint32_t v = lds[b];
        if (v) atomicAdd(&hist[b], (ull)v);
    }
}

// The pending segmented table (okm_ctx::Pending): item i's counts are the
// n_out[i] words at sc + items[i].out_off (u32 when NARROW).  With few waves,
// an item-by-item walk (k_compact_items' walk without its keys) would leave
// each wave a dependent round of at most 1 KB per 256 entries and item.  So a
// wave takes a contiguous range of items, 64 at a time: one descriptor per
// lane, a wave scan of their sizes, and then the group's entries as ONE flat
// range with kHistFly loads in flight per lane whatever the item boundaries;
// each lane finds the item of its position with a cursor that only moves
// forward (the descriptors stay in their lanes' registers, read by shuffle).
template <bool NARROW>
__global__ __launch_bounds__(kHistBlock) void k_hist_items(const DevItem *__restrict__ items, uint32_t nitems,
                                                    const ull *__restrict__ n_out, const uint64_t *__restrict__ sc,
                                                    uint64_t last, uint32_t nlds, ull *__restrict__ hist,
                                                    ull *__restrict__ summary) {
    __shared__ uint32_t lds[kHistLds];
    HistAcc a;
    hist_init(a, lds, nlds);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nwaves = gridDim.x * (kHistBlock / 64u);
    const uint32_t per = (nitems + nwaves - 1u) / nwaves;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(blockIdx.x * (kHistBlock / 64u) + (threadIdx.x >> 6));
    const uint32_t i0 = (uint32_t)min((uint64_t)wv * per, (uint64_t)nitems);
    const uint32_t i1 = (uint32_t)min((uint64_t)i0 + per, (uint64_t)nitems);
    const uint32_t *sc32 = reinterpret_cast<const uint32_t *>(sc);
    for (uint32_t base = i0; base < i1; base += 64u) {  // wave-uniform: every lane stays in (the shuffles need them)
        const uint32_t cnt = i1 - base < 64u ? i1 - base : 64u;
        ull my_n = 0, my_off = 0;
        if (lane < cnt) {
            my_n = n_out[base + lane];
            my_off = items[base + lane].out_off;
        }
        const ull incl = wave_incl_scan(my_n);     // entries of the group's items up to and including this lane's
        const ull dlt = my_off - (incl - my_n);    // flat position -> index into sc (wrapping arithmetic is exact)
        const ull total = __shfl(incl, 63, 64);
        uint32_t t = 0;                            // this lane's cursor: the item its position lies in
        ull end = __shfl(incl, 0, 64), delta = __shfl(dlt, 0, 64);
        for (ull eb = 0; eb < total; eb += 64u * kHistFly) {
            ull at[kHistFly], c[kHistFly];
            bool ok[kHistFly];
#pragma unroll
            for (int q = 0; q < kHistFly; ++q) {
                const ull e = eb + 64u * q + lane;
                ok[q] = e < total;
                // positions rise, so the cursor only moves forward; e < total = incl[63] keeps it below 64
                while (__any(ok[q] && e >= end)) {
                    if (ok[q] && e >= end) ++t;
                    end = __shfl(incl, (int)t, 64);
                    delta = __shfl(dlt, (int)t, 64);
                }
                at[q] = e + delta;
            }
#pragma unroll
            for (int q = 0; q < kHistFly; ++q) c[q] = !ok[q] ? 0 : NARROW ? (ull)sc32[at[q]] : (ull)sc[at[q]];
#pragma unroll
            for (int q = 0; q < kHistFly; ++q)
                if (ok[q]) hist_add(a, c[q], last, nlds, lds, hist);
        }
    }
    hist_flush(a, nlds, lds, hist, summary);
}

// A dense table's counts[n] (a gathered, directly counted or folded table, or
// one uploaded slice of a host-resident one): grid-stride tiles of 4 x kHistBlock.
__global__ __launch_bounds__(kHistBlock) void k_hist_dense(const uint64_t *__restrict__ counts, uint64_t n, uint64_t last,
                                                    uint32_t nlds, ull *__restrict__ hist,
                                                    ull *__restrict__ summary) {
    __shared__ uint32_t lds[kHistLds];
    HistAcc a;
    hist_init(a, lds, nlds);
    constexpr uint64_t tile = 4 * kHistBlock;
    const uint64_t stride = (uint64_t)gridDim.x * tile;
    for (uint64_t base = (uint64_t)blockIdx.x * tile; base < n; base += stride) {
        const uint64_t j = base + threadIdx.x;
        if (base + tile <= n) {
            uint64_t c[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) c[q] = counts[j + kHistBlock * q];
#pragma unroll
            for (int q = 0; q < 4; ++q) hist_add(a, c[q], last, nlds, lds, hist);
        } else {
            for (uint64_t i = j; i < n; i += kHistBlock) hist_add(a, counts[i], last, nlds, lds, hist);
        }
    }
    hist_flush(a, nlds, lds, hist, summary);
}

void launch_hist_items(void *stream, const DevItem *items, uint32_t nitems, const unsigned long long *n_out,
                       const uint64_t *counts, bool narrow, uint64_t n_bins, unsigned long long *hist,
                       unsigned long long *summary) {
    if (!nitems) return;
    const uint32_t nlds = (uint32_t)(n_bins < kHistLds ? n_bins : kHistLds);
    // eight items per wave or more
    const uint32_t want = nitems / (8u * kHistBlock / 64u) + 1u;
    const dim3 g(want < kHistGrid ? want : kHistGrid), b(kHistBlock);
    hipStream_t s = (hipStream_t)stream;
    if (narrow)
        hipLaunchKernelGGL(k_hist_items<true>, g, b, 0, s, items, nitems, n_out, counts, n_bins - 1, nlds, hist,
                           summary);
    else
        hipLaunchKernelGGL(k_hist_items<false>, g, b, 0, s, items, nitems, n_out, counts, n_bins - 1, nlds, hist,
                           summary);
}

void launch_hist_dense(void *stream, const uint64_t *counts, uint64_t n, uint64_t n_bins, unsigned long long *hist,
                       unsigned long long *summary) {
    if (!n) return;
    const uint32_t nlds = (uint32_t)(n_bins < kHistLds ? n_bins : kHistLds);
    const uint64_t want = (n + 4 * kHistBlock - 1) / (4 * kHistBlock);
    const dim3 g((uint32_t)(want < kHistGrid ? want : kHistGrid)), b(kHistBlock);
    hipLaunchKernelGGL(k_hist_dense, g, b, 0, (hipStream_t)stream, counts, n, n_bins - 1, nlds, hist, summary);
}

}  // namespace okm
