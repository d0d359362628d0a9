// okm_cmp_stage.h — how the two merges of counted tables (okm_compare.hip,
// okm_combine.hip) bring a piece of a run into LDS.
#pragma once

#include "okm_dev_common.h"

namespace okm {

constexpr int kCmpBlock = 256;

// A count as LDS holds it: u32, saturated.  kCmpSat from a u64 table means "fetch it" (the user then reads
// the count itself from memory), so every form stages 4 bytes per count and has the same LDS footprint.
constexpr uint32_t kCmpSat = 0xFFFFFFFFu;

// A tile's entries: what one workgroup of a merge stages of the driving table (and of the other one, per chunk).
#ifndef OKM_CMP_TILE  // a build flag, for the A/B in profiles/AB_LOG.md
#define OKM_CMP_TILE 1024
#endif
template <typename KT> struct CmpTileOf { static constexpr uint32_t T = OKM_CMP_TILE / (sizeof(KT) / 8); };

// n entries of a run into LDS, from entry `off` on: keys, and counts at counts[coff + off ...].  (One key
// per lane and load: 16-byte loads of two keys, with the unaligned head and tail apart, measured 12 %
// slower, profiles/AB_LOG.md.)
template <typename KT, bool NARROW>
__device__ __forceinline__ void cmp_stage(const LookItem *__restrict__ d, ull off, uint32_t n,
                                          const uint64_t *__restrict__ counts, KT *lk, uint32_t *lc) {
    const KT *kp = reinterpret_cast<const KT *>(gload(&d->keys)) + off;
    const ull cb = gload(&d->coff) + off;
    const uint32_t *c32 = reinterpret_cast<const uint32_t *>(counts);
    for (uint32_t i = threadIdx.x; i < n; i += kCmpBlock) {
        lk[i] = gload(kp + i);
        if (NARROW) {
            lc[i] = gload(c32 + cb + i);
        } else {
            const ull c = gload(counts + cb + i);
            lc[i] = c < kCmpSat ? (uint32_t)c : kCmpSat;
        }
    }
}

// The same with the side's threshold applied while staging: an entry below min_count is staged as 0 ("not
// kept"; a table holds no count 0), a kept one saturated as above.  A user that only asks "kept?" and
// "which bin of at most 2^16?" (okm_jointhist.hip) then never needs the count itself, whatever the
// threshold: the comparison is made on the full count, before it is narrowed.
template <typename KT, bool NARROW>
__device__ __forceinline__ void cmp_stage_kept(const LookItem *__restrict__ d, ull off, uint32_t n,
                                               const uint64_t *__restrict__ counts, ull min_count, KT *lk,
                                               uint32_t *lc) {
    const KT *kp = reinterpret_cast<const KT *>(gload(&d->keys)) + off;
    const ull cb = gload(&d->coff) + off;
    const uint32_t *c32 = reinterpret_cast<const uint32_t *>(counts);
    for (uint32_t i = threadIdx.x; i < n; i += kCmpBlock) {
        lk[i] = gload(kp + i);
        const ull c = NARROW ? (ull)gload(c32 + cb + i) : (ull)gload(counts + cb + i);
        lc[i] = c < min_count ? 0u : c < kCmpSat ? (uint32_t)c : kCmpSat;
    }
}

}  // namespace okm
