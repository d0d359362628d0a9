// okm_read_scan.h -- the front of the window scan that the in-place readers of
// read batches share (okm_depth.hip k_read_depths, okm_solid.hip k_solid_mask):
// a workgroup of kScanBlock threads takes kScanTile batch bytes, a thread
// kScanSeg consecutive window starts, and opens with
//     typename SK::Words ww;   load_windows<kScanSeg, SK::kHalo>(seq, n, w0, ww);
//     typename SK::Coded c;    make_codes<SK::kNP, false>(ww.w, c);
//     vmask = SK::valid_mask(c, k);   tab.begin();
// (SK = ScanKeys<KT>; okm_scan.h's loads and codes, count's normalisation),
// then per window j: live = bit j of vmask, the key SK::key(c, j, k) or
// KeyOps<KT>::empty(), and tab.find() of a finder of okm_search.h.  Those
// lines stand in both kernels, not in a function here: the compiler
// simplifies a function on its own before it inlines it, and every wrapper
// tried (a struct of the three values with load / begin / find, free
// functions over the kernels' own locals, the find step alone) changed the
// instructions and the register allocation of kernels that are at the edge
// of an occupancy step (profiles/AB_LOG.md).  What a kernel does with
// (live, hit, count) is its own: rows in one, bits in the other.
#pragma once

#include "okm_dev_common.h"
#include "okm_scan.h"

namespace okm {

constexpr int kScanBlock = 256;
// Window starts per thread: the loads of okm_scan.h come in 16-byte words
// (window starts + a 32 or 64 byte halo), so 16 is the smallest run; a longer
// one only adds loaded words to carry (24 at k > 32 already).
constexpr int kScanSeg = 16;
constexpr int kScanTile = kScanBlock * kScanSeg;  // 4096 bytes per workgroup

// A key type's side of the scan: the halo its windows need, the valid windows
// of the thread's run and the canonical key of window j.
template <typename KT> struct ScanKeys;
template <> struct ScanKeys<ull> {
    static constexpr int kHalo = 32;
    typedef WinWords<kScanSeg, kHalo> Words;
    static constexpr int kNP = Words::kLoad / 16;
    typedef Codes<kNP> Coded;
    __device__ static __forceinline__ uint32_t valid_mask(const Codes<kNP> &c, uint32_t k) {
        return ~invalid_windows<kScanSeg, kNP>(c, k) & ((1u << kScanSeg) - 1u);
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
template <> struct ScanKeys<K128> {
    static constexpr int kHalo = 64;
    typedef WinWords<kScanSeg, kHalo> Words;
    static constexpr int kNP = Words::kLoad / 16;
    typedef Codes<kNP> Coded;
    __device__ static __forceinline__ uint32_t valid_mask(const Codes<kNP> &c, uint32_t k) {
        const uint64_t km = k >= 64 ? ~0ull : ((1ull << k) - 1ull);
        uint32_t m = 0;
#pragma unroll
        for (int j = 0; j < kScanSeg; ++j) m |= ((bad_low64(c, j) & km) == 0 ? 1u : 0u) << j;
        return m;
    }
    __device__ static __forceinline__ K128 key(const Codes<kNP> &c, int j, uint32_t k) {
        bool valid;
        return window_key128(c, j, k, &valid);
    }
};

// Bit j: byte j of the thread's kScanSeg is a separator.  Two forms of the same
// 16 bits: both compare each of the 16 bytes with the separator, a byte a step
// or four bytes a step (as pack4 gathers its bad bits).  Both remain because
// each kernel keeps the one it was measured with: the compiler turns them into
// different instructions, and a kernel whose form changes has to be timed
// again before the other form can go (profiles/AB_LOG.md has the registers
// and instruction counts of the swap; its timing is not taken yet).
__device__ __forceinline__ uint32_t sep_mask_bytes(const uint32_t *w) {  // k_read_depths
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < kScanSeg; ++i)
        m |= (((w[i >> 2] >> ((i & 3) * 8)) & 0xFFu) == OKM_RECORD_SEPARATOR ? 1u : 0u) << i;
    return m;
}
__device__ __forceinline__ uint32_t sep_mask_words(const uint32_t *w) {  // k_solid_mask
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < kScanSeg / 4; ++i) {
        const uint32_t z = zero_bytes(w[i] ^ (0x01010101u * OKM_RECORD_SEPARATOR));
        m |= ((((z >> 7) & 0x01010101u) * 0x00204081u) >> 21 & 0xFu) << (4 * i);
    }
    return m;
}

}  // namespace okm
