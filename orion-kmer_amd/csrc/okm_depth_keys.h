// okm_depth_keys.h -- a key type's side of the window scan the in-place
// readers of read batches share (okm_depth.hip, okm_solid.hip): a thread owns
// kKeySeg consecutive window starts, loaded and coded by okm_scan.h.
#pragma once

#include "okm_dev_common.h"
#include "okm_scan.h"

namespace okm {

// Window starts per thread: the loads of okm_scan.h come in 16-byte words
// (window starts + a 32 or 64 byte halo), so 16 is the smallest run.
constexpr int kKeySeg = 16;

// A key type's side of the scan: the halo its windows need, the valid windows
// of the thread's run and the canonical key of window j.
template <typename KT> struct DepthKeys;
template <> struct DepthKeys<ull> {
    static constexpr int kHalo = 32;
    static constexpr int kNP = WinWords<kKeySeg, 32>::kLoad / 16;
    __device__ static __forceinline__ uint32_t valid_mask(const Codes<kNP> &c, uint32_t k) {
        return ~invalid_windows<kKeySeg, kNP>(c, k) & ((1u << kKeySeg) - 1u);
    }
    // window_key_nv's value from 64-bit slices: with k known only at run time
    // its 32-bit funnel shifts index the code words by k, which puts them in
    // scratch memory (as k_query_hits<0> has them); here only j, a
    // compile-time constant, picks words, and the kernel waits on its
    // searches, not on these shifts.
    __device__ static __forceinline__ ull key(const Codes<kNP> &c, int j, uint32_t k) {
        const uint64_t f = fwd_top64(c, j) >> (64u - 2u * k);                               // kmer.rs:37-57
        const uint64_t r = rc_low64(c, j) & (k >= 32 ? ~0ull : ((1ull << (2u * k)) - 1ull));  // kmer.rs:79-94
        return f < r ? f : r;                                                                // kmer.rs:99-106
    }
};
template <> struct DepthKeys<K128> {
    static constexpr int kHalo = 64;
    static constexpr int kNP = WinWords<kKeySeg, 64>::kLoad / 16;
    __device__ static __forceinline__ uint32_t valid_mask(const Codes<kNP> &c, uint32_t k) {
        const uint64_t km = k >= 64 ? ~0ull : ((1ull << k) - 1ull);
        uint32_t m = 0;
#pragma unroll
        for (int j = 0; j < kKeySeg; ++j) m |= ((bad_low64(c, j) & km) == 0 ? 1u : 0u) << j;
        return m;
    }
    __device__ static __forceinline__ K128 key(const Codes<kNP> &c, int j, uint32_t k) {
        bool valid;
        return window_key128(c, j, k, &valid);
    }
};

}  // namespace okm
