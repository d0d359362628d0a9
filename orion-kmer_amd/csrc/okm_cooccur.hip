// okm_cooccur.hip — the co-occurrence (Gram) matrix of a membership table
// (okm_count_mask_matrix).  Every entry's count is read as a mask of up to 64
// bits (sample i added its keys with weight 1 << i), and
//   matrix[i][j] = entries whose mask has bits i and j,   i, j < n_bits
//   occupancy[p] = entries whose mask has exactly p of its low n_bits bits
// That is B^T B of the (entries x n_bits) bit matrix B.  Only counts are read,
// never keys, where the table lies: the walks are okm_hist.hip's (a pending
// table as one flat range per 64 item descriptors, u32 or u64 counts, several
// loads in flight per lane; a dense table or an uploaded slice in grid-stride
// tiles), in few large workgroups, at most one per CU.
//
// One wave step takes 64 entries, one mask per lane.
//   Transpose.  The 64 x 64 bit block is turned so that lane i holds column
//   word col_i (bit l: lane l's mask has bit i).  Two ways, chosen per walk and
//   width by the measurement in profiles/AB_LOG.md (OKM_MM_TRANSPOSE forces one):
//   NB ballots with lane j keeping the j-th, or a 6-step butterfly on lane
//   pairs (swap the off-diagonal blocks of 32, 16, .. 1 bits with lane ^ s).
//   Gram.  Lane i owns row i in NB u32 registers: for every j (unrolled, wave
//   uniform) col_j is broadcast with two readlanes into scalars and acc[j] +=
//   popcount(col_i & col_j), two 32-bit bit counts whose add operand carries
//   the accumulator: 64 one-bit multiply-accumulates per VALU instruction.
// Matrix instructions do not fit: the narrowest MFMA operand is 8 bits (4 on
// some forms), so an MFMA spends 8 operand bits where the popcount spends one,
// and the masks would first have to be expanded to bytes.
//
// No overflow by the grid arithmetic: a lane adds at most 64 per step and an
// LDS cell takes a whole workgroup's sums, so both hold while a workgroup sees
// fewer than 2^32 entries -- with kMmGrid workgroups, a table (or slice) below
// 2^40 entries, more than device memory holds.  A smaller grid is only taken
// for a smaller table.  Nothing is flushed in between.
//
// Occupancy: each lane's popcount of its own masked entry into an LDS
// histogram of n_bits + 1 bins (all-core tables queue on one address: a few
// percent of the Gram loop).
//
// Flush.  The workgroup's waves add their rows into one LDS matrix, stored
// [j][i] so that the 64 lanes of one add hit 64 banks.  Beyond 16 columns the
// workgroup then stores the matrix and the occupancy plainly as its partial,
// and a small kernel sums the partials into the u64 result; up to 16 columns
// it adds its non-zero cells with one global u64 atomic each (OKM_MM_FLUSH
// forces one way; both measured in profiles/AB_LOG.md).
#include <hip/hip_runtime.h>

#include "okm_dev_common.h"
#include "okm_internal.h"

namespace okm {

constexpr int kMmBlock = 1024;     // 16 waves
constexpr uint32_t kMmGrid = 256;  // workgroups at most, one per CU
constexpr int kMmFly = 4;          // loads in flight per lane (acc[] leaves the registers for no more)
constexpr uint32_t kMmPart = 64 * 64 + 128;  // u32 words of a workgroup's partial: the [j][i] matrix, then the occupancy

#ifndef OKM_MM_TRANSPOSE
#define OKM_MM_TRANSPOSE 2  // 0: ballots, 1: butterfly, 2: by width (profiles/AB_LOG.md)
#endif
// Measured at 8 and 64 columns: the ballots win at 8 in both walks (0.65 vs 1.47 ms pending) and at 64 in the
// pending walk (2.68 vs 2.99 ms); the butterfly wins at 64 in the dense walk (2.27 vs 2.64 ms).
template <int NB, bool DENSE>
constexpr bool mm_butterfly() {
    return OKM_MM_TRANSPOSE == 2 ? DENSE && NB > 16 : OKM_MM_TRANSPOSE == 1;
}
#ifndef OKM_MM_FLUSH
#define OKM_MM_FLUSH 2  // 0: partials + reduce, 1: global atomics, 2: by width (profiles/AB_LOG.md)
#endif
// Up to 16 columns a workgroup has at most 273 words to add, and the atomics measured 10 % of the kernel
// faster than the reduce pass behind the partials; beyond that the two are within 2 %, and the partials cost
// the same whatever the masks hold.
template <int NB>
constexpr bool mm_atomic_flush() {
    return OKM_MM_FLUSH == 2 ? NB <= 16 : OKM_MM_FLUSH == 1;
}

// col of this lane for the wave's 64 masks (every lane of the wave calls it).
template <int NB, bool DENSE>
__device__ __forceinline__ ull mm_transpose(ull m, uint32_t lane) {
    if (mm_butterfly<NB, DENSE>()) {
        ull x = m;
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            // bits whose index has bit s clear: the left half of every 2s-wide block
            const ull left = s == 32 ? 0x00000000FFFFFFFFull : s == 16 ? 0x0000FFFF0000FFFFull
                             : s == 8 ? 0x00FF00FF00FF00FFull : s == 4 ? 0x0F0F0F0F0F0F0F0Full
                             : s == 2 ? 0x3333333333333333ull : 0x5555555555555555ull;
            const ull y = __shfl_xor(x, s, 64);
            // [[A B] [C D]] -> [[A C] [B D]]: the upper lane keeps A and takes C, the lower takes B and keeps D
            x = (lane & (uint32_t)s) ? ((x & ~left) | ((y & ~left) >> s)) : ((x & left) | ((y & left) << s));
        }
        return x;
    }
    ull col = 0;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const ull b = __ballot((int)((m >> j) & 1ull));
        col = lane == (uint32_t)j ? b : col;
    }
    return col;
}

// One wave step: the masks of 64 entries (0 for a lane beyond the range), already cut to the low n_bits.
template <int NB, bool DENSE>
__device__ __forceinline__ void mm_step(ull m, uint32_t lane, uint32_t (&acc)[NB]) {
    const ull col = mm_transpose<NB, DENSE>(m, lane);
    const uint32_t clo = (uint32_t)col, chi = (uint32_t)(col >> 32);
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)clo, j);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)chi, j);
        acc[j] += __popc(clo & lo) + __popc(chi & hi);
    }
}

struct MmLds {
    uint32_t mat[64 * 64];  // [j][i]
    uint32_t occ[128];
};

template <int NB>
__device__ __forceinline__ void mm_init(uint32_t (&acc)[NB], MmLds &l) {
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[j] = 0;
    for (uint32_t c = threadIdx.x; c < kMmPart; c += blockDim.x) (c < 4096 ? l.mat[c] : l.occ[c - 4096]) = 0;
    __syncthreads();
}

// Every wave of the workgroup calls this once (no early return before it).
// out: n_bits * n_bits matrix words, then n_bits + 1 occupancy words.
template <int NB>
__device__ __forceinline__ void mm_flush(uint32_t (&acc)[NB], MmLds &l, uint32_t n_bits, uint32_t *__restrict__ part,
                                         ull *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int j = 0; j < NB; ++j)
        if (acc[j]) atomicAdd(&l.mat[j * 64 + lane], acc[j]);
    __syncthreads();
    if (mm_atomic_flush<NB>()) {
        for (uint32_t c = threadIdx.x; c < kMmPart; c += blockDim.x) {
            const uint32_t j = c >> 6, i = c & 63u;
            if (c < 4096) {
                if (i < n_bits && j < n_bits && l.mat[c]) atomicAdd(&out[i * n_bits + j], (ull)l.mat[c]);
            } else if (c - 4096 <= n_bits && l.occ[c - 4096]) {
                atomicAdd(&out[n_bits * n_bits + (c - 4096)], (ull)l.occ[c - 4096]);
            }
        }
        return;
    }
    uint32_t *mine = part + (size_t)blockIdx.x * kMmPart;
    for (uint32_t c = threadIdx.x; c < kMmPart; c += blockDim.x) mine[c] = c < 4096 ? l.mat[c] : l.occ[c - 4096];
}

// out += the sum of nparts partials, cell by cell (one thread each; launches of one stream follow each other).
__global__ void k_mm_reduce(const uint32_t *__restrict__ part, uint32_t nparts, uint32_t n_bits, ull *__restrict__ out) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= kMmPart) return;
    const uint32_t j = c >> 6, i = c & 63u;
    const bool cell = c < 4096 && i < n_bits && j < n_bits, bin = c >= 4096 && c - 4096 <= n_bits;
    if (!cell && !bin) return;
    ull sum = 0;
    for (uint32_t g = 0; g < nparts; ++g) sum += part[(size_t)g * kMmPart + c];
    out[cell ? i * n_bits + j : n_bits * n_bits + (c - 4096)] += sum;
}

// The pending segmented table, walked as k_hist_items walks it: a wave takes a
// contiguous range of items, 64 descriptors at a time, and reads the group's
// entries as one flat range; each lane finds the item of its position with a
// cursor that only moves forward.  Every 64 consecutive positions are one step.
template <int NB, bool NARROW>
__global__ __launch_bounds__(kMmBlock) void k_mm_items(const DevItem *__restrict__ items, uint32_t nitems,
                                                const ull *__restrict__ n_out, const uint64_t *__restrict__ sc,
                                                uint32_t n_bits, uint32_t *__restrict__ part, ull *__restrict__ out) {
    __shared__ MmLds l;
    uint32_t acc[NB];
    mm_init<NB>(acc, l);
    const ull keep = n_bits >= 64 ? ~0ull : (1ull << n_bits) - 1ull;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nwaves = gridDim.x * (kMmBlock / 64u);
    const uint32_t per = (nitems + nwaves - 1u) / nwaves;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(blockIdx.x * (kMmBlock / 64u) + (threadIdx.x >> 6));
    const uint32_t i0 = (uint32_t)min((uint64_t)wv * per, (uint64_t)nitems);
    const uint32_t i1 = (uint32_t)min((uint64_t)i0 + per, (uint64_t)nitems);
    const uint32_t *sc32 = reinterpret_cast<const uint32_t *>(sc);
    for (uint32_t base = i0; base < i1; base += 64u) {  // wave-uniform: every lane stays in
        const uint32_t cnt = i1 - base < 64u ? i1 - base : 64u;
        ull my_n = 0, my_off = 0;
        if (lane < cnt) {
            my_n = n_out[base + lane];
            my_off = items[base + lane].out_off;
        }
        const ull incl = wave_incl_scan(my_n);
        const ull dlt = my_off - (incl - my_n);  // flat position -> index into sc (wrapping arithmetic is exact)
        const ull total = __shfl(incl, 63, 64);
        uint32_t t = 0;
        ull end = __shfl(incl, 0, 64), delta = __shfl(dlt, 0, 64);
        for (ull eb = 0; eb < total; eb += 64u * kMmFly) {
            ull at[kMmFly], m[kMmFly];
            bool ok[kMmFly];
#pragma unroll
            for (int q = 0; q < kMmFly; ++q) {
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
            for (int q = 0; q < kMmFly; ++q) m[q] = !ok[q] ? 0 : (NARROW ? (ull)sc32[at[q]] : (ull)sc[at[q]]) & keep;
#pragma unroll
            for (int q = 0; q < kMmFly; ++q) {
                if (eb + 64u * q < total) {  // wave-uniform: else the step is empty
                    if (ok[q]) atomicAdd(&l.occ[__popcll(m[q])], 1u);
                    mm_step<NB, false>(m[q], lane, acc);
                }
            }
        }
    }
    mm_flush<NB>(acc, l, n_bits, part, out);
}

// A dense table's counts[n] (or one uploaded slice of a host-resident one):
// grid-stride tiles of kMmFly x kMmBlock; a wave's 64 consecutive entries are one step.
template <int NB>
__global__ __launch_bounds__(kMmBlock) void k_mm_dense(const uint64_t *__restrict__ counts, uint64_t n, uint32_t n_bits,
                                                uint32_t *__restrict__ part, ull *__restrict__ out) {
    __shared__ MmLds l;
    uint32_t acc[NB];
    mm_init<NB>(acc, l);
    const ull keep = n_bits >= 64 ? ~0ull : (1ull << n_bits) - 1ull;
    const uint32_t lane = threadIdx.x & 63u;
    constexpr uint64_t tile = (uint64_t)kMmFly * kMmBlock;
    const uint64_t stride = (uint64_t)gridDim.x * tile;
    for (uint64_t base = (uint64_t)blockIdx.x * tile; base < n; base += stride) {
        ull m[kMmFly];
        bool ok[kMmFly];
#pragma unroll
        for (int q = 0; q < kMmFly; ++q) {
            const uint64_t j = base + threadIdx.x + (uint64_t)kMmBlock * q;
            ok[q] = j < n;
            m[q] = ok[q] ? counts[j] & keep : 0;
        }
#pragma unroll
        for (int q = 0; q < kMmFly; ++q) {
            if (base + (threadIdx.x & ~63u) + (uint64_t)kMmBlock * q < n) {  // wave-uniform: else the step is empty
                if (ok[q]) atomicAdd(&l.occ[__popcll(m[q])], 1u);
                mm_step<NB, true>(m[q], lane, acc);
            }
        }
    }
    mm_flush<NB>(acc, l, n_bits, part, out);
}

size_t mask_matrix_part_words() { return (size_t)kMmGrid * kMmPart; }

// (nothing behind the widths whose workgroups flushed with atomics)
static void mm_reduce(hipStream_t s, const uint32_t *part, uint32_t nparts, uint32_t n_bits, unsigned long long *out) {
    if (n_bits <= 16 ? mm_atomic_flush<16>() : mm_atomic_flush<64>()) return;
    hipLaunchKernelGGL(k_mm_reduce, dim3((kMmPart + 255u) / 256u), dim3(256), 0, s, part, nparts, n_bits, out);
}

// The kernels are built for 8, 16, 32 and 64 columns: the narrowest that holds n_bits runs.
#define OKM_MM_BY_WIDTH(LAUNCH) \
    do {                        \
        if (n_bits <= 8) {      \
            LAUNCH(8);          \
        } else if (n_bits <= 16) { \
            LAUNCH(16);         \
        } else if (n_bits <= 32) { \
            LAUNCH(32);         \
        } else {                \
            LAUNCH(64);         \
        }                       \
    } while (0)

void launch_mask_matrix_items(void *stream, const DevItem *items, uint32_t nitems, const unsigned long long *n_out,
                              const uint64_t *counts, bool narrow, uint32_t n_bits, uint32_t *part,
                              unsigned long long *out) {
    if (!nitems) return;
    // eight items per wave or more
    const uint32_t want = nitems / (8u * kMmBlock / 64u) + 1u;
    const dim3 g(want < kMmGrid ? want : kMmGrid), b(kMmBlock);
    hipStream_t s = (hipStream_t)stream;
#define OKM_MM_ITEMS(NB)                                                                                              \
    if (narrow)                                                                                                       \
        hipLaunchKernelGGL((k_mm_items<NB, true>), g, b, 0, s, items, nitems, n_out, counts, n_bits, part, out);     \
    else                                                                                                              \
        hipLaunchKernelGGL((k_mm_items<NB, false>), g, b, 0, s, items, nitems, n_out, counts, n_bits, part, out)
    OKM_MM_BY_WIDTH(OKM_MM_ITEMS);
#undef OKM_MM_ITEMS
    mm_reduce(s, part, g.x, n_bits, out);
}

void launch_mask_matrix_dense(void *stream, const uint64_t *counts, uint64_t n, uint32_t n_bits, uint32_t *part,
                              unsigned long long *out) {
    if (!n) return;
    const uint64_t tile = (uint64_t)kMmFly * kMmBlock, want = (n + tile - 1) / tile;
    const dim3 g((uint32_t)(want < kMmGrid ? want : kMmGrid)), b(kMmBlock);
    hipStream_t s = (hipStream_t)stream;
#define OKM_MM_DENSE(NB) hipLaunchKernelGGL((k_mm_dense<NB>), g, b, 0, s, counts, n, n_bits, part, out)
    OKM_MM_BY_WIDTH(OKM_MM_DENSE);
#undef OKM_MM_DENSE
    mm_reduce(s, part, g.x, n_bits, out);
}

// w[i] = weight for i < n: sample i's membership bit, one per kept key (okm_pairwise_shared).
__global__ void k_fill_weight(uint64_t *__restrict__ w, uint64_t n, uint64_t weight) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        w[i] = weight;
}

void launch_fill_weight(void *stream, uint64_t *w, uint64_t n, uint64_t weight) {
    if (!n) return;
    const uint64_t want = (n + 255) / 256;
    hipLaunchKernelGGL(k_fill_weight, dim3((uint32_t)(want < 4096 ? want : 4096)), dim3(256), 0, (hipStream_t)stream, w,
                       n, weight);
}

}  // namespace okm
