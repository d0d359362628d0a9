// okm_lookup.hip — the counts of given keys in a counted table, searched where
// the table lies (okm_lookup_counts): out[i] = count of query i, 0 when absent.
//
// Every representation of the table is sorted by key, so a lookup is a search,
// and all of them use one routine, search_last_le (okm_search.h).  A lane can
// keep several queries in flight that issue their loads together, level by
// level; the lookup kernels keep kLookFly.
//
// Dense table: one search of keys[0, n).  Pending table (okm_ctx::Pending, the
// per-item runs k_compact_items would gather): two levels.  The first keys of
// the items that own a key are gathered once per call into a small array
// (launch_lookup_index: 8 or 16 bytes per item, L2-resident), the first search
// finds the item whose range holds the query, the second searches that item's
// run and reads its count (u32 when narrow) at the same position.
#include <hip/hip_runtime.h>

#include "okm_dev_common.h"
#include "okm_internal.h"
#include "okm_search.h"

namespace okm {

#ifndef OKM_LOOK_FLY  // a build flag, for the A/B in profiles/AB_LOG.md
#define OKM_LOOK_FLY 1
#endif

constexpr int kLookBlock = 256;
// Queries in flight per lane.  One: the kernels are bound by the memory
// system's rate of random 64-byte reads, not by a lane's latency, and 2 / 4 / 8
// in flight measured 2 / 19 / 24 % slower on the pending C2 table (registers
// for occupancy; profiles/AB_LOG.md).
constexpr int kLookFly = OKM_LOOK_FLY;

// *found += the workgroup's hits: one atomic per workgroup at most.  Every
// wave of the workgroup calls this once.
__device__ __forceinline__ void look_found(uint32_t mine, ull *__restrict__ found) {
    __shared__ uint32_t wred[kLookBlock / 64];
    uint32_t v = mine;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63u) == 0) wred[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < kLookBlock / 64; ++w) t += wred[w];
        if (t) atomicAdd(found, (ull)t);
    }
}

template <typename KT, bool HITS_ONLY>
__global__ __launch_bounds__(kLookBlock) void k_lookup_dense(const KT *__restrict__ keys,
                                                             const uint64_t *__restrict__ counts, ull n,
                                                             const ull *__restrict__ queries, ull nq,
                                                             ull *__restrict__ out, ull *__restrict__ found) {
    typedef KeyOps<KT> O;
    const ull base = (ull)blockIdx.x * (kLookBlock * kLookFly) + threadIdx.x;
    FlatKeys<KT> a[kLookFly];
    ull len[kLookFly], pos[kLookFly];
    KT q[kLookFly], last[kLookFly];
#pragma unroll
    for (int f = 0; f < kLookFly; ++f) {
        const ull i = base + (ull)f * kLookBlock;
        a[f].p = keys;
        len[f] = i < nq ? n : 0;
        q[f] = i < nq ? load_query<KT>(queries, i) : O::empty();
    }
    search_last_le<KT, kLookFly>(a, len, q, pos, last);
    uint32_t hits = 0;
    ull c[kLookFly];
#pragma unroll
    for (int f = 0; f < kLookFly; ++f) {
        const bool hit = len[f] && O::eq(last[f], q[f]);
        c[f] = hit ? counts[pos[f]] : 0;
        hits += hit ? 1u : 0u;
    }
#pragma unroll
    for (int f = 0; f < kLookFly; ++f) {
        const ull i = base + (ull)f * kLookBlock;
        if (i < nq && (!HITS_ONLY || c[f])) out[i] = c[f];  // (a table entry's count is never 0)
    }
    look_found(hits, found);
}

template <typename KT, bool NARROW>
__global__ __launch_bounds__(kLookBlock) void k_lookup_items(const KT *__restrict__ first,
                                                             const LookItem *__restrict__ desc,
                                                             const ull *__restrict__ n_desc,
                                                             const uint64_t *__restrict__ sc,
                                                             const ull *__restrict__ queries, ull nq,
                                                             ull *__restrict__ out, ull *__restrict__ found) {
    typedef KeyOps<KT> O;
    const ull m = *n_desc;
    const ull base = (ull)blockIdx.x * (kLookBlock * kLookFly) + threadIdx.x;
    FlatKeys<KT> a[kLookFly];
    ull len[kLookFly], pos[kLookFly], coff[kLookFly];
    KT q[kLookFly], last[kLookFly];
#pragma unroll
    for (int f = 0; f < kLookFly; ++f) {
        const ull i = base + (ull)f * kLookBlock;
        a[f].p = first;
        len[f] = i < nq ? m : 0;
        q[f] = i < nq ? load_query<KT>(queries, i) : O::empty();
    }
    // the item whose first key is the last one <= the query: no other item's range can hold it
    search_last_le<KT, kLookFly>(a, len, q, pos, last);
#pragma unroll
    for (int f = 0; f < kLookFly; ++f) {
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
    search_last_le<KT, kLookFly>(a, len, q, pos, last);
    const uint32_t *sc32 = reinterpret_cast<const uint32_t *>(sc);
    uint32_t hits = 0;
    ull c[kLookFly];
#pragma unroll
    for (int f = 0; f < kLookFly; ++f) {
        const bool hit = len[f] && O::eq(last[f], q[f]);
        c[f] = !hit ? 0 : NARROW ? (ull)sc32[coff[f] + pos[f]] : (ull)sc[coff[f] + pos[f]];
        hits += hit ? 1u : 0u;
    }
#pragma unroll
    for (int f = 0; f < kLookFly; ++f) {
        const ull i = base + (ull)f * kLookBlock;
        if (i < nq) out[i] = c[f];
    }
    look_found(hits, found);
}

// flags[i] = item i owns a key, i < nitems; flags[nitems] = 0 (the scan's total lands there)
__global__ __launch_bounds__(256) void k_lookup_flags(const DevItem *__restrict__ items, uint32_t nitems,
                                                      const ull *__restrict__ n_out, ull *__restrict__ flags) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i <= nitems) flags[i] = i < nitems && items[i].pad != kItemEmpty && n_out[i] ? 1ull : 0ull;
}

// pos = the exclusive scan of the flags: a kept item has pos[i + 1] > pos[i].
template <typename KT>
__global__ __launch_bounds__(256) void k_lookup_index(const DevItem *__restrict__ items, uint32_t nitems,
                                                      const ull *__restrict__ n_out, const ull *__restrict__ pos,
                                                      const KT *__restrict__ sk, KT *__restrict__ first,
                                                      LookItem *__restrict__ desc) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nitems) return;
    const ull p = pos[i];
    if (pos[i + 1] == p) return;
    // sk == nullptr: the runs were staged in place, over the items' own keys (as k_compact_items reads them)
    const ull off = items[i].out_off;
    const KT *kb = sk ? sk + off : reinterpret_cast<const KT *>(items[i].keys0);
    first[p] = gload(kb);
    LookItem d;
    d.keys = reinterpret_cast<const uint64_t *>(kb);
    d.coff = off;
    d.n = n_out[i];
    desc[p] = d;
}

void launch_lookup_index(void *stream, const DevItem *items, uint32_t nitems, const unsigned long long *n_out,
                         const uint64_t *src_keys, bool wide, unsigned long long *pos, unsigned long long *scan_tmp,
                         uint64_t *first, LookItem *desc) {
    hipStream_t s = (hipStream_t)stream;
    const dim3 g(nitems / 256u + 1u), b(256);
    hipLaunchKernelGGL(k_lookup_flags, g, b, 0, s, items, nitems, n_out, pos);
    launch_exclusive_scan(stream, pos, pos, (uint64_t)nitems + 1, scan_tmp);
    if (wide)
        hipLaunchKernelGGL(k_lookup_index<K128>, g, b, 0, s, items, nitems, n_out, pos,
                           reinterpret_cast<const K128 *>(src_keys), reinterpret_cast<K128 *>(first), desc);
    else
        hipLaunchKernelGGL(k_lookup_index<ull>, g, b, 0, s, items, nitems, n_out, pos,
                           reinterpret_cast<const ull *>(src_keys), reinterpret_cast<ull *>(first), desc);
}

// One workgroup per kLookBlock * kLookFly queries, no cap and no stride: a
// grid of 2^31 - 1 covers 2^41 queries, more than a device can hold.
static dim3 look_grid(uint64_t nq) {
    return dim3((uint32_t)((nq + kLookBlock * kLookFly - 1) / (kLookBlock * kLookFly)));
}

void launch_lookup_items(void *stream, const uint64_t *first, const LookItem *desc, const unsigned long long *n_desc,
                         const uint64_t *src_counts, bool narrow, bool wide, const uint64_t *queries, uint64_t nq,
                         uint64_t *out, unsigned long long *found) {
    if (!nq) return;
    hipStream_t s = (hipStream_t)stream;
    const dim3 g = look_grid(nq), b(kLookBlock);
    const K128 *f2 = reinterpret_cast<const K128 *>(first);
    const ull *f1 = reinterpret_cast<const ull *>(first);
    const ull *q = reinterpret_cast<const ull *>(queries);
    ull *o = reinterpret_cast<ull *>(out);
    if (wide && narrow)
        hipLaunchKernelGGL((k_lookup_items<K128, true>), g, b, 0, s, f2, desc, n_desc, src_counts, q, nq, o, found);
    else if (wide)
        hipLaunchKernelGGL((k_lookup_items<K128, false>), g, b, 0, s, f2, desc, n_desc, src_counts, q, nq, o, found);
    else if (narrow)
        hipLaunchKernelGGL((k_lookup_items<ull, true>), g, b, 0, s, f1, desc, n_desc, src_counts, q, nq, o, found);
    else
        hipLaunchKernelGGL((k_lookup_items<ull, false>), g, b, 0, s, f1, desc, n_desc, src_counts, q, nq, o, found);
}

void launch_lookup_dense(void *stream, const uint64_t *keys, const uint64_t *counts, uint64_t n, bool wide,
                         const uint64_t *queries, uint64_t nq, uint64_t *out, unsigned long long *found,
                         bool hits_only) {
    if (!nq) return;
    hipStream_t s = (hipStream_t)stream;
    const dim3 g = look_grid(nq), b(kLookBlock);
    const K128 *k2 = reinterpret_cast<const K128 *>(keys);
    const ull *k1 = reinterpret_cast<const ull *>(keys);
    const ull *q = reinterpret_cast<const ull *>(queries);
    ull *o = reinterpret_cast<ull *>(out);
    if (wide && hits_only)
        hipLaunchKernelGGL((k_lookup_dense<K128, true>), g, b, 0, s, k2, counts, n, q, nq, o, found);
    else if (wide)
        hipLaunchKernelGGL((k_lookup_dense<K128, false>), g, b, 0, s, k2, counts, n, q, nq, o, found);
    else if (hits_only)
        hipLaunchKernelGGL((k_lookup_dense<ull, true>), g, b, 0, s, k1, counts, n, q, nq, o, found);
    else
        hipLaunchKernelGGL((k_lookup_dense<ull, false>), g, b, 0, s, k1, counts, n, q, nq, o, found);
}

}  // namespace okm
