// okm_search.h — the search every in-place reader of a counted table shares
// (okm_lookup.hip, okm_depth.hip, okm_compare.hip), and the two finders built
// on it: FindDense and FindItems, one per form of a TableView
// (okm_internal.h), used by the lookup, the depth and the solid kernels;
// with_finder picks the one that reads a view.
//
// Every representation of the table is sorted by key, so a lookup is a search,
// and all of them use one routine, search_last_le: the position of the last
// key <= the query in a sorted range read through an accessor.  Its step count
// depends on the range's length only, never on the data, so a lane can keep
// several queries in flight (QF) that issue their loads together, level by
// level.  (The compare's k_cmp_bounds searches for ranges, not for hits, and
// calls search_last_le itself.)
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

// The table's two forms: find() answers QF queries at once (live[f]: query f
// is one), hit[f] and, where hit, its count (else 0).  begin() runs once per
// thread before the first find().

// keys[n] / counts[n], a dense table or one uploaded slice (n == 0: an empty
// table, nothing is read)
template <typename KT, int QF>
struct FindDense {
    typedef KT Key;
    const KT *keys;
    const uint64_t *counts;
    ull n;
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void find(const KT (&q)[QF], const bool (&live)[QF], ull (&cnt)[QF],
                                         bool (&hit)[QF]) const {
        typedef KeyOps<KT> O;
        FlatKeys<KT> a[QF];
        ull len[QF], pos[QF];
        KT last[QF];
#pragma unroll
        for (int f = 0; f < QF; ++f) {
            a[f].p = keys;
            len[f] = live[f] ? n : 0;
        }
        search_last_le<KT, QF>(a, len, q, pos, last);
#pragma unroll
        for (int f = 0; f < QF; ++f) {
            hit[f] = len[f] && O::eq(last[f], q[f]);
            cnt[f] = hit[f] ? counts[pos[f]] : 0;
        }
    }
};

// The pending per-item runs behind launch_lookup_index's first-key index, two
// levels: the item whose range holds the query, then that item's run, whose
// count lies at the same position; NARROW: the runs' counts are u32.
template <typename KT, bool NARROW, int QF>
struct FindItems {
    typedef KT Key;
    const KT *first;
    const LookItem *desc;
    const ull *n_desc;
    const uint64_t *sc;
    ull m;
    __device__ __forceinline__ void begin() { m = *n_desc; }
    __device__ __forceinline__ void find(const KT (&q)[QF], const bool (&live)[QF], ull (&cnt)[QF],
                                         bool (&hit)[QF]) const {
        typedef KeyOps<KT> O;
        FlatKeys<KT> a[QF];
        ull len[QF], pos[QF], coff[QF];
        KT last[QF];
#pragma unroll
        for (int f = 0; f < QF; ++f) {
            a[f].p = first;
            len[f] = live[f] ? m : 0;
        }
        // the item whose first key is the last one <= the query: no other item's range can hold it
        search_last_le<KT, QF>(a, len, q, pos, last);
#pragma unroll
        for (int f = 0; f < QF; ++f) {
            const bool owned = len[f] && !O::lt(q[f], last[f]);  // else: below the table's first key
            len[f] = 0;
            coff[f] = 0;
            if (owned) {
                const LookItem *d = desc + pos[f];
                a[f].p = reinterpret_cast<const KT *>(gload(&d->keys));
                coff[f] = gload(&d->coff);
                len[f] = gload(&d->n);
            }
        }
        search_last_le<KT, QF>(a, len, q, pos, last);
        const uint32_t *sc32 = reinterpret_cast<const uint32_t *>(sc);
#pragma unroll
        for (int f = 0; f < QF; ++f) {
            hit[f] = len[f] && O::eq(last[f], q[f]);
            cnt[f] = !hit[f] ? 0 : NARROW ? (ull)sc32[coff[f] + pos[f]] : (ull)sc[coff[f] + pos[f]];
        }
    }
};

// f(tab), tab the finder that reads view t: its Key by `wide`, its form by the
// view's, FLY searches in flight.  (Host side: f launches a kernel with it.)
template <typename KT, int FLY, typename F>
inline void with_finder_of(const TableView &t, F f) {
    const KT *first = reinterpret_cast<const KT *>(t.first);
    if (!t.runs)
        f(FindDense<KT, FLY>{reinterpret_cast<const KT *>(t.keys), t.counts, t.n});
    else if (t.narrow)
        f(FindItems<KT, true, FLY>{first, t.desc, t.n_desc, t.counts, 0});
    else
        f(FindItems<KT, false, FLY>{first, t.desc, t.n_desc, t.counts, 0});
}
template <int FLY, typename F>
inline void with_finder(const TableView &t, bool wide, F f) {
    if (wide)
        with_finder_of<K128, FLY>(t, f);
    else
        with_finder_of<ull, FLY>(t, f);
}

}  // namespace okm
