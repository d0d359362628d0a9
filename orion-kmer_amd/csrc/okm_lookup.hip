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

// The two lookup kernels: load the queries, find them (okm_search.h), store.
// HITS_ONLY is a property of the store: one slice of several writes only what
// it finds.
template <typename KT, typename TAB, bool HITS_ONLY>
__device__ __forceinline__ void look_queries(TAB tab, const ull *__restrict__ queries, ull nq, ull *__restrict__ out,
                                             ull *__restrict__ found) {
    typedef KeyOps<KT> O;
    const ull base = (ull)blockIdx.x * (kLookBlock * kLookFly) + threadIdx.x;
    KT q[kLookFly];
    bool live[kLookFly], hit[kLookFly];
    ull c[kLookFly];
    tab.begin();
#pragma unroll
    for (int f = 0; f < kLookFly; ++f) {
        const ull i = base + (ull)f * kLookBlock;
        live[f] = i < nq;
        q[f] = live[f] ? load_query<KT>(queries, i) : O::empty();
    }
    tab.find(q, live, c, hit);
    uint32_t hits = 0;
#pragma unroll
    for (int f = 0; f < kLookFly; ++f) {
        const ull i = base + (ull)f * kLookBlock;
        hits += hit[f] ? 1u : 0u;
        if (live[f] && (!HITS_ONLY || c[f])) out[i] = c[f];  // (a table entry's count is never 0)
    }
    look_found(hits, found);
}

template <typename KT, bool HITS_ONLY>
__global__ __launch_bounds__(kLookBlock) void k_lookup_dense(const KT *__restrict__ keys,
                                                             const uint64_t *__restrict__ counts, ull n,
                                                             const ull *__restrict__ queries, ull nq,
                                                             ull *__restrict__ out, ull *__restrict__ found) {
    look_queries<KT, FindDense<KT, kLookFly>, HITS_ONLY>({keys, counts, n}, queries, nq, out, found);
}

template <typename KT, bool NARROW>
__global__ __launch_bounds__(kLookBlock) void k_lookup_items(const KT *__restrict__ first,
                                                             const LookItem *__restrict__ desc,
                                                             const ull *__restrict__ n_desc,
                                                             const uint64_t *__restrict__ sc,
                                                             const ull *__restrict__ queries, ull nq,
                                                             ull *__restrict__ out, ull *__restrict__ found) {
    look_queries<KT, FindItems<KT, NARROW, kLookFly>, false>({first, desc, n_desc, sc, 0}, queries, nq, out, found);
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

void launch_lookup(void *stream, const TableView &t, bool wide, const uint64_t *queries, uint64_t nq, uint64_t *out,
                   unsigned long long *found, bool hits_only) {
    if (!nq) return;
    hipStream_t s = (hipStream_t)stream;
    const dim3 g = look_grid(nq), b(kLookBlock);
    const ull *q = reinterpret_cast<const ull *>(queries);
    ull *o = reinterpret_cast<ull *>(out);
    if (t.runs) {
        const K128 *f2 = reinterpret_cast<const K128 *>(t.first);
        const ull *f1 = reinterpret_cast<const ull *>(t.first), *nd = t.n_desc;
        const uint64_t *sc = t.counts;
        if (wide && t.narrow)
            hipLaunchKernelGGL((k_lookup_items<K128, true>), g, b, 0, s, f2, t.desc, nd, sc, q, nq, o, found);
        else if (wide)
            hipLaunchKernelGGL((k_lookup_items<K128, false>), g, b, 0, s, f2, t.desc, nd, sc, q, nq, o, found);
        else if (t.narrow)
            hipLaunchKernelGGL((k_lookup_items<ull, true>), g, b, 0, s, f1, t.desc, nd, sc, q, nq, o, found);
        else
            hipLaunchKernelGGL((k_lookup_items<ull, false>), g, b, 0, s, f1, t.desc, nd, sc, q, nq, o, found);
        return;
    }
    const K128 *k2 = reinterpret_cast<const K128 *>(t.keys);
    const ull *k1 = reinterpret_cast<const ull *>(t.keys);
    if (wide && hits_only)
        hipLaunchKernelGGL((k_lookup_dense<K128, true>), g, b, 0, s, k2, t.counts, t.n, q, nq, o, found);
    else if (wide)
        hipLaunchKernelGGL((k_lookup_dense<K128, false>), g, b, 0, s, k2, t.counts, t.n, q, nq, o, found);
    else if (hits_only)
        hipLaunchKernelGGL((k_lookup_dense<ull, true>), g, b, 0, s, k1, t.counts, t.n, q, nq, o, found);
    else
        hipLaunchKernelGGL((k_lookup_dense<ull, false>), g, b, 0, s, k1, t.counts, t.n, q, nq, o, found);
}

}  // namespace okm
