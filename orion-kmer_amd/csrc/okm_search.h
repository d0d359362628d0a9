// okm_search.h — the search every in-place reader of a counted table shares
// (okm_lookup.hip, okm_depth.hip).
//
// Every representation of the table is sorted by key, so a lookup is a search,
// and all of them use one routine, search_last_le: the position of the last
// key <= the query in a sorted range read through an accessor.  Its step count
// depends on the range's length only, never on the data, so a lane can keep
// several queries in flight (QF) that issue their loads together, level by
// level.
#pragma once

#include "okm_dev_common.h"

namespace okm {

// A sorted range of keys in device memory.
template <typename KT>
struct FlatKeys {
    const KT *p;
    __device__ __forceinline__ KT operator()(ull i) const { return gload(p + i); }
};

// For each of QF independent searches: pos[f] = the index of the last key of
// a[f](0 .. n[f]) that is <= q[f], and last[f] = that key.  When every key is
// larger, pos[f] = 0 and last[f] = a[f](0); the caller tells the two apart by
// comparing last[f] with q[f].  n[f] == 0: nothing is read, pos[f] = 0.
// The range [pos, pos + len) always holds the answer; a step halves len
// whatever the comparison says, so searches of equal length stay in step.
template <typename KT, int QF, typename ACC>
__device__ __forceinline__ void search_last_le(const ACC (&a)[QF], const ull (&n)[QF], const KT (&q)[QF],
                                               ull (&pos)[QF], KT (&last)[QF]) {
    typedef KeyOps<KT> O;
    ull len[QF];
    bool more = false;
#pragma unroll
    for (int f = 0; f < QF; ++f) {
        pos[f] = 0;
        len[f] = n[f];
        last[f] = O::empty();
        more |= len[f] > 1;
    }
    while (more) {
        KT k[QF];
#pragma unroll
        for (int f = 0; f < QF; ++f) k[f] = len[f] > 1 ? a[f](pos[f] + (len[f] >> 1)) : O::empty();
        more = false;
#pragma unroll
        for (int f = 0; f < QF; ++f)
            if (len[f] > 1) {
                const ull half = len[f] >> 1;
                if (!O::lt(q[f], k[f])) {
                    pos[f] += half;
                    last[f] = k[f];
                }
                len[f] -= half;
                more |= len[f] > 1;
            }
    }
#pragma unroll
    for (int f = 0; f < QF; ++f)
        if (n[f] && pos[f] == 0) last[f] = a[f](0);  // never moved: last is not a[0] yet
}

template <typename KT>
__device__ __forceinline__ KT load_query(const ull *queries, ull i);
template <>
__device__ __forceinline__ ull load_query<ull>(const ull *queries, ull i) {
    return queries[i];
}
// (two word loads: a caller's okm_key128 array need not be 16-byte aligned)
template <>
__device__ __forceinline__ K128 load_query<K128>(const ull *queries, ull i) {
    return K128{queries[2 * i], queries[2 * i + 1]};
}

}  // namespace okm
