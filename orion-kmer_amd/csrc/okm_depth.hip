// okm_depth.hip — per-record k-mer depth of a batch of reads against a counted
// table, searched where the table lies (okm_read_depths): for every record the
// number of its valid windows, how many of their canonical k-mers are in the
// table, how many reach min_count, and the sum / smallest / largest of the
// present windows' counts.
//
// One kernel goes from the batch bytes to the rows: no key array is written
// and nothing of the table is gathered.  A thread owns kDepthSeg consecutive
// window starts.  It builds the 2-bit codes and the valid mask once
// (okm_scan.h, count's normalisation), then takes the windows kDepthFly at a
// time (one: see there): their canonical keys from the codes, their searches
// level by level with the loads of all of them in flight together
// (search_last_le, okm_search.h), and their counts added to six register
// accumulators.  Which record a window belongs to comes from the separators
// before it: a prefix per tile (k_depth_sep_count + a scan) plus a block scan,
// as k_query_hits has it.
// The accumulators leave at a record change and at the end of the thread's run
// as 64-bit global atomics on the record's row: add, add, add, max, max.
//
// `min` is accumulated as the LARGEST ~count: its identity is then the 0 the
// rows start from, every slice of a host-resident table adds into the same
// rows, and one small kernel over the rows (k_depth_fix) turns the field
// round at the end of the launch sequence: min = present ? ~field : 0.
#include <hip/hip_runtime.h>

#include "okm_dev_common.h"
#include "okm_internal.h"
#include "okm_scan.h"
#include "okm_search.h"

namespace okm {

#ifndef OKM_DEPTH_FLY  // build flags, for the A/Bs in profiles/AB_LOG.md
#define OKM_DEPTH_FLY 1
#endif
#ifndef OKM_DEPTH_WAVE
#define OKM_DEPTH_WAVE 1
#endif

constexpr int kDepthBlock = 256;
// Window starts per thread: the loads of okm_scan.h come in 16-byte words
// (window starts + a 32 or 64 byte halo), so 16 is the smallest run; a longer
// one only adds loaded words to carry (24 at k > 32 already).
constexpr int kDepthSeg = 16;
constexpr int kDepthTile = kDepthBlock * kDepthSeg;  // 4096 bytes per workgroup
// Searches a lane keeps in flight.  One, as in the lookup (okm_lookup.hip
// kLookFly): the kernel is bound by the memory system's rate of random 64-byte
// reads, which the waves of a CU already fill, and a search in flight holds
// its key, range, position and last key in registers that cost occupancy.  On
// the C2 batch against its own pending / dense table 1 / 2 / 4 / 8 in flight
// measured 77.5 / 79.0 / 81.5 / 96.0 ms and 97.5 / 104.3 / 111.3 / 110.7 ms
// (profiles/AB_LOG.md).
constexpr int kDepthFly = OKM_DEPTH_FLY;
static_assert(kDepthSeg % kDepthFly == 0, "whole groups of searches");
constexpr int kRowWords = 6;  // okm_read_depth: windows, present, solid, sum, min, max
static_assert(sizeof(okm_read_depth) == kRowWords * sizeof(ull), "rows are six u64");

__device__ __forceinline__ uint32_t depth_sep_bytes(uint32_t w) {  // separator bytes in a word
    const uint32_t x = w ^ (0x01010101u * OKM_RECORD_SEPARATOR);
    return __popc(zero_bytes(x));
}

__device__ __forceinline__ uint32_t depth_sep_mask(const uint32_t *w) {  // bit j: byte j is a separator
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < kDepthSeg; ++i)
        m |= (((w[i >> 2] >> ((i & 3) * 8)) & 0xFFu) == OKM_RECORD_SEPARATOR ? 1u : 0u) << i;
    return m;
}

// tile_cnt[t] = separators among the bytes of tile t (bytes at or past n: none)
__global__ __launch_bounds__(kDepthBlock) void k_depth_sep_count(const uint8_t *__restrict__ seq, uint64_t n,
                                                                 ull *__restrict__ tile_cnt) {
    __shared__ ull wsum[kDepthBlock / 64];
    const uint64_t w0 = (uint64_t)blockIdx.x * kDepthTile + (uint64_t)threadIdx.x * kDepthSeg;
    uint32_t c = 0;
    if (w0 + kDepthSeg <= n) {
        const uint4 v = *reinterpret_cast<const uint4 *>(seq + w0);
        c = depth_sep_bytes(v.x) + depth_sep_bytes(v.y) + depth_sep_bytes(v.z) + depth_sep_bytes(v.w);
    } else {
        for (uint64_t i = w0; i < n; ++i) c += seq[i] == OKM_RECORD_SEPARATOR;
    }
    ull tot;
    block_excl_scan<kDepthBlock>((ull)c, wsum, &tot);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = tot;
}

// The table's representations: find() answers kDepthFly windows at once
// (live[f]: window f is valid), hit[f] and, where hit, its count.

// keys[n] / counts[n], dense (n == 0: an empty table, nothing is read)
template <typename KT>
struct DepthDense {
    const KT *keys;
    const uint64_t *counts;
    ull n;
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void find(const KT (&q)[kDepthFly], const bool (&live)[kDepthFly],
                                         ull (&cnt)[kDepthFly], bool (&hit)[kDepthFly]) const {
        typedef KeyOps<KT> O;
        FlatKeys<KT> a[kDepthFly];
        ull len[kDepthFly], pos[kDepthFly];
        KT last[kDepthFly];
#pragma unroll
        for (int f = 0; f < kDepthFly; ++f) {
            a[f].p = keys;
            len[f] = live[f] ? n : 0;
        }
        search_last_le<KT, kDepthFly>(a, len, q, pos, last);
#pragma unroll
        for (int f = 0; f < kDepthFly; ++f) {
            hit[f] = len[f] && O::eq(last[f], q[f]);
            cnt[f] = hit[f] ? counts[pos[f]] : 0;
        }
    }
};

// The pending per-item runs behind launch_lookup_index's first-key index, as
// k_lookup_items searches them; NARROW: the runs' counts are u32.
template <typename KT, bool NARROW>
struct DepthItems {
    const KT *first;
    const LookItem *desc;
    const ull *n_desc;
    const uint64_t *sc;
    ull m;
    __device__ __forceinline__ void begin() { m = *n_desc; }
    __device__ __forceinline__ void find(const KT (&q)[kDepthFly], const bool (&live)[kDepthFly],
                                         ull (&cnt)[kDepthFly], bool (&hit)[kDepthFly]) const {
        typedef KeyOps<KT> O;
        FlatKeys<KT> a[kDepthFly];
        ull len[kDepthFly], pos[kDepthFly], coff[kDepthFly];
        KT last[kDepthFly];
#pragma unroll
        for (int f = 0; f < kDepthFly; ++f) {
            a[f].p = first;
            len[f] = live[f] ? m : 0;
        }
        // the item whose first key is the last one <= the window's key
        search_last_le<KT, kDepthFly>(a, len, q, pos, last);
#pragma unroll
        for (int f = 0; f < kDepthFly; ++f) {
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
        search_last_le<KT, kDepthFly>(a, len, q, pos, last);
        const uint32_t *sc32 = reinterpret_cast<const uint32_t *>(sc);
#pragma unroll
        for (int f = 0; f < kDepthFly; ++f) {
            hit[f] = len[f] && O::eq(last[f], q[f]);
            cnt[f] = !hit[f] ? 0 : NARROW ? (ull)sc32[coff[f] + pos[f]] : (ull)sc[coff[f] + pos[f]];
        }
    }
};

// A key type's side of the scan: the halo its windows need, the valid windows
// of the thread's run and the canonical key of window j.
template <typename KT> struct DepthKeys;
template <> struct DepthKeys<ull> {
    static constexpr int kHalo = 32;
    static constexpr int kNP = WinWords<kDepthSeg, 32>::kLoad / 16;
    __device__ static __forceinline__ uint32_t valid_mask(const Codes<kNP> &c, uint32_t k) {
        return ~invalid_windows<kDepthSeg, kNP>(c, k) & ((1u << kDepthSeg) - 1u);
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
    static constexpr int kNP = WinWords<kDepthSeg, 64>::kLoad / 16;
    __device__ static __forceinline__ uint32_t valid_mask(const Codes<kNP> &c, uint32_t k) {
        const uint64_t km = k >= 64 ? ~0ull : ((1ull << k) - 1ull);
        uint32_t m = 0;
#pragma unroll
        for (int j = 0; j < kDepthSeg; ++j) m |= ((bad_low64(c, j) & km) == 0 ? 1u : 0u) << j;
        return m;
    }
    __device__ static __forceinline__ K128 key(const Codes<kNP> &c, int j, uint32_t k) {
        bool valid;
        return window_key128(c, j, k, &valid);
    }
};

// What a thread has seen of the record it is in.
struct DepthAcc {
    uint32_t windows, present, solid;
    ull sum, nmin, mx;  // nmin: the largest ~count (0: none)
};

// WIN: this launch also counts the windows (the first slice's launch only).
template <bool WIN>
__device__ __forceinline__ void depth_flush(ull *__restrict__ rows, uint64_t nrec, ull rec, const DepthAcc &a) {
    if (rec >= nrec) return;  // more separators than the caller's n_records
    ull *r = rows + rec * kRowWords;
    if (WIN && a.windows) atomicAdd(r + 0, (ull)a.windows);
    if (a.present) {
        atomicAdd(r + 1, (ull)a.present);
        if (a.solid) atomicAdd(r + 2, (ull)a.solid);
        atomicAdd(r + 3, a.sum);
        atomicMax(r + 4, a.nmin);
        atomicMax(r + 5, a.mx);
    }
}

template <typename KT, typename TAB, bool WIN>
__global__ __launch_bounds__(kDepthBlock) void k_read_depths(const uint8_t *__restrict__ seq, uint64_t n,
                                                             const ull *__restrict__ tile_pre, TAB tab, uint32_t k,
                                                             ull min_count, ull *__restrict__ rows, uint64_t nrec) {
    typedef KeyOps<KT> O;
    typedef DepthKeys<KT> DK;
    __shared__ ull wsum[kDepthBlock / 64];
    const uint64_t w0 = (uint64_t)blockIdx.x * kDepthTile + (uint64_t)threadIdx.x * kDepthSeg;
    WinWords<kDepthSeg, DK::kHalo> ww;
    load_windows<kDepthSeg, DK::kHalo>(seq, n, w0, ww);  // bytes at or past n read as 0: no base, no separator
    const uint32_t sepm = depth_sep_mask(ww.w);
    ull tot;
    ull rec = tile_pre[blockIdx.x] + block_excl_scan<kDepthBlock>((ull)__popc(sepm), wsum, &tot);
    // (no thread leaves early: the wave reduction below needs every lane)
    Codes<DK::kNP> c;
    make_codes<DK::kNP, false>(ww.w, c);  // count's validity: either case, U reads as T
    const uint32_t vmask = DK::valid_mask(c, k);
    tab.begin();
    DepthAcc acc = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int g = 0; g < kDepthSeg / kDepthFly; ++g) {
        KT q[kDepthFly];
        bool live[kDepthFly], hit[kDepthFly];
        ull cnt[kDepthFly];
#pragma unroll
        for (int f = 0; f < kDepthFly; ++f) {
            const int j = g * kDepthFly + f;
            live[f] = (vmask >> j) & 1u;
            q[f] = live[f] ? DK::key(c, j, k) : O::empty();
        }
        tab.find(q, live, cnt, hit);
#pragma unroll
        for (int f = 0; f < kDepthFly; ++f) {
            const int j = g * kDepthFly + f;
            if ((sepm >> j) & 1u) {  // byte j ends a record: window j is none, the next belongs to the next record
                depth_flush<WIN>(rows, nrec, rec, acc);
                acc = DepthAcc{0, 0, 0, 0, 0, 0};
                ++rec;
            }
            acc.windows += live[f] ? 1u : 0u;
            if (hit[f]) {
                acc.present += 1u;
                acc.solid += cnt[f] >= min_count ? 1u : 0u;
                acc.sum += cnt[f];
                acc.nmin = max(acc.nmin, ~cnt[f]);
                acc.mx = max(acc.mx, cnt[f]);
            }
        }
    }
#if OKM_DEPTH_WAVE
    // A wave whose 1024 bytes hold no separator lies inside one record (a long
    // read): its 64 partial rows become one before they leave, so the row
    // takes one flush per wave instead of 64 (ONT-like reads against their own
    // pending table: 125.1 ms against 134.8 without; profiles/AB_LOG.md).
    if (__ballot(sepm != 0) == 0) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            acc.windows += __shfl_xor(acc.windows, d, 64);
            acc.present += __shfl_xor(acc.present, d, 64);
            acc.solid += __shfl_xor(acc.solid, d, 64);
            acc.sum += __shfl_xor(acc.sum, d, 64);
            acc.nmin = max(acc.nmin, __shfl_xor(acc.nmin, d, 64));
            acc.mx = max(acc.mx, __shfl_xor(acc.mx, d, 64));
        }
        if ((threadIdx.x & 63u) != 0) return;
    }
#endif
    depth_flush<WIN>(rows, nrec, rec, acc);
}

// The rows' min field holds the largest ~count: turn it round.
__global__ __launch_bounds__(256) void k_depth_fix(ull *__restrict__ rows, uint64_t nrec) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrec) return;
    ull *r = rows + i * kRowWords;
    r[4] = r[1] ? ~r[4] : 0ull;
}

uint64_t depth_tiles(uint64_t n_bytes) { return (n_bytes + kDepthTile - 1) / kDepthTile; }

template <typename KT, typename TAB>
static void launch_depth_tab(hipStream_t s, uint32_t ntiles, const uint8_t *seq, uint64_t n, const ull *pre,
                             const TAB &tab, uint32_t k, uint64_t min_count, bool count_windows, ull *rows,
                             uint64_t nrec) {
    if (count_windows)
        hipLaunchKernelGGL((k_read_depths<KT, TAB, true>), dim3(ntiles), dim3(kDepthBlock), 0, s, seq, n, pre, tab, k,
                           (ull)min_count, rows, nrec);
    else
        hipLaunchKernelGGL((k_read_depths<KT, TAB, false>), dim3(ntiles), dim3(kDepthBlock), 0, s, seq, n, pre, tab, k,
                           (ull)min_count, rows, nrec);
}

template <typename KT>
static void launch_depth_key(hipStream_t s, uint32_t ntiles, const uint8_t *seq, uint64_t n, const ull *pre,
                             const DepthTable &t, uint32_t k, uint64_t min_count, bool count_windows, ull *rows,
                             uint64_t nrec) {
    if (!t.items) {
        const DepthDense<KT> tab{reinterpret_cast<const KT *>(t.keys), t.counts, t.n};
        launch_depth_tab<KT>(s, ntiles, seq, n, pre, tab, k, min_count, count_windows, rows, nrec);
    } else if (t.narrow) {
        const DepthItems<KT, true> tab{reinterpret_cast<const KT *>(t.first), t.desc, t.n_desc, t.sc, 0};
        launch_depth_tab<KT>(s, ntiles, seq, n, pre, tab, k, min_count, count_windows, rows, nrec);
    } else {
        const DepthItems<KT, false> tab{reinterpret_cast<const KT *>(t.first), t.desc, t.n_desc, t.sc, 0};
        launch_depth_tab<KT>(s, ntiles, seq, n, pre, tab, k, min_count, count_windows, rows, nrec);
    }
}

void launch_read_depths(void *stream, const uint8_t *seq, uint64_t n, uint64_t nrec, uint32_t k, bool wide,
                        const DepthTable &t, uint64_t min_count, bool count_windows, unsigned long long *tiles,
                        okm_read_depth *rows) {
    if (!n || !nrec) return;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t nt = depth_tiles(n);  // < 2^31 (the caller's check)
    ull *cnt = tiles, *pre = cnt + nt, *scr = pre + nt;
    hipLaunchKernelGGL(k_depth_sep_count, dim3((uint32_t)nt), dim3(kDepthBlock), 0, s, seq, n, cnt);
    launch_exclusive_scan(stream, cnt, pre, nt, scr);
    ull *r = reinterpret_cast<ull *>(rows);
    if (wide)
        launch_depth_key<K128>(s, (uint32_t)nt, seq, n, pre, t, k, min_count, count_windows, r, nrec);
    else
        launch_depth_key<ull>(s, (uint32_t)nt, seq, n, pre, t, k, min_count, count_windows, r, nrec);
}

void launch_read_depths_fix(void *stream, okm_read_depth *rows, uint64_t nrec) {
    if (!nrec) return;
    hipLaunchKernelGGL(k_depth_fix, dim3((uint32_t)((nrec + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<ull *>(rows), nrec);
}

}  // namespace okm
