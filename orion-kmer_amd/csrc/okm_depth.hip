// okm_depth.hip — per-record k-mer depth of a batch of reads against a counted
// table, searched where the table lies (okm_read_depths): for every record the
// number of its valid windows, how many of their canonical k-mers are in the
// table, how many reach min_count, and the sum / smallest / largest of the
// present windows' counts.
//
// One kernel goes from the batch bytes to the rows: no key array is written
// and nothing of the table is gathered.  A thread owns kScanSeg consecutive
// window starts (the read-batch scan, okm_read_scan.h).  It builds the 2-bit
// codes and the valid mask once, then takes the windows kDepthFly at a
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
#include "okm_read_scan.h"
#include "okm_scan.h"
#include "okm_search.h"

namespace okm {

#ifndef OKM_DEPTH_FLY  // build flags, for the A/Bs in profiles/AB_LOG.md
#define OKM_DEPTH_FLY 1
#endif
#ifndef OKM_DEPTH_WAVE
#define OKM_DEPTH_WAVE 1
#endif

// Searches a lane keeps in flight.  One, as in the lookup (okm_lookup.hip
// kLookFly): the kernel is bound by the memory system's rate of random 64-byte
// reads, which the waves of a CU already fill, and a search in flight holds
// its key, range, position and last key in registers that cost occupancy.  On
// the C2 batch against its own pending / dense table 1 / 2 / 4 / 8 in flight
// measured 77.5 / 79.0 / 81.5 / 96.0 ms and 97.5 / 104.3 / 111.3 / 110.7 ms
// (profiles/AB_LOG.md).
constexpr int kDepthFly = OKM_DEPTH_FLY;
static_assert(kScanSeg % kDepthFly == 0, "whole groups of searches");
constexpr int kRowWords = 6;  // okm_read_depth: windows, present, solid, sum, min, max
static_assert(sizeof(okm_read_depth) == kRowWords * sizeof(ull), "rows are six u64");

__device__ __forceinline__ uint32_t depth_sep_bytes(uint32_t w) {  // separator bytes in a word
    const uint32_t x = w ^ (0x01010101u * OKM_RECORD_SEPARATOR);
    return __popc(zero_bytes(x));
}

// tile_cnt[t] = separators among the bytes of tile t (bytes at or past n: none)
__global__ __launch_bounds__(kScanBlock) void k_depth_sep_count(const uint8_t *__restrict__ seq, uint64_t n,
                                                                ull *__restrict__ tile_cnt) {
    __shared__ ull wsum[kScanBlock / 64];
    const uint64_t w0 = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanSeg;
    uint32_t c = 0;
    if (w0 + kScanSeg <= n) {
        const uint4 v = *reinterpret_cast<const uint4 *>(seq + w0);
        c = depth_sep_bytes(v.x) + depth_sep_bytes(v.y) + depth_sep_bytes(v.z) + depth_sep_bytes(v.w);
    } else {
        for (uint64_t i = w0; i < n; ++i) c += seq[i] == OKM_RECORD_SEPARATOR;
    }
    ull tot;
    block_excl_scan<kScanBlock>((ull)c, wsum, &tot);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = tot;
}

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
__global__ __launch_bounds__(kScanBlock) void k_read_depths(const uint8_t *__restrict__ seq, uint64_t n,
                                                            const ull *__restrict__ tile_pre, TAB tab, uint32_t k,
                                                            ull min_count, ull *__restrict__ rows, uint64_t nrec) {
    typedef KeyOps<KT> O;
    typedef ScanKeys<KT> SK;
    __shared__ ull wsum[kScanBlock / 64];
    const uint64_t w0 = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanSeg;
    typename SK::Words ww;
    load_windows<kScanSeg, SK::kHalo>(seq, n, w0, ww);  // bytes at or past n read as 0: no base, no separator
    const uint32_t sepm = sep_mask_bytes(ww.w);
    ull tot;
    ull rec = tile_pre[blockIdx.x] + block_excl_scan<kScanBlock>((ull)__popc(sepm), wsum, &tot);
    // (no thread leaves early: the wave reduction below needs every lane)
    typename SK::Coded c;
    make_codes<SK::kNP, false>(ww.w, c);  // count's validity: either case, U reads as T
    const uint32_t vmask = SK::valid_mask(c, k);
    tab.begin();
    DepthAcc acc = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int g = 0; g < kScanSeg / kDepthFly; ++g) {
        KT q[kDepthFly];
        bool live[kDepthFly], hit[kDepthFly];
        ull cnt[kDepthFly];
#pragma unroll
        for (int f = 0; f < kDepthFly; ++f) {
            const int j = g * kDepthFly + f;
            live[f] = (vmask >> j) & 1u;
            q[f] = live[f] ? SK::key(c, j, k) : O::empty();
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

uint64_t depth_tiles(uint64_t n_bytes) { return (n_bytes + kScanTile - 1) / kScanTile; }

void launch_depth_sep_count(void *stream, const uint8_t *seq, uint64_t n, unsigned long long *tile_cnt) {
    hipLaunchKernelGGL(k_depth_sep_count, dim3((uint32_t)depth_tiles(n)), dim3(kScanBlock), 0, (hipStream_t)stream, seq,
                       n, tile_cnt);
}

void launch_read_depths(void *stream, const uint8_t *seq, uint64_t n, uint64_t nrec, uint32_t k, bool wide,
                        const TableView &t, uint64_t min_count, bool count_windows, unsigned long long *tiles,
                        okm_read_depth *rows) {
    if (!n || !nrec) return;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t nt = depth_tiles(n);  // < 2^31 (the caller's check)
    ull *cnt = tiles, *pre = cnt + nt, *scr = pre + nt;
    launch_depth_sep_count(stream, seq, n, cnt);
    launch_exclusive_scan(stream, cnt, pre, nt, scr);
    ull *r = reinterpret_cast<ull *>(rows);
    with_finder<kDepthFly>(t, wide, [&](const auto &tab) {
        typedef std::decay_t<decltype(tab)> TAB;
        typedef typename TAB::Key KT;
        if (count_windows)
            hipLaunchKernelGGL((k_read_depths<KT, TAB, true>), dim3((uint32_t)nt), dim3(kScanBlock), 0, s, seq, n, pre,
                               tab, k, (ull)min_count, r, nrec);
        else
            hipLaunchKernelGGL((k_read_depths<KT, TAB, false>), dim3((uint32_t)nt), dim3(kScanBlock), 0, s, seq, n, pre,
                               tab, k, (ull)min_count, r, nrec);
    });
}

void launch_read_depths_fix(void *stream, okm_read_depth *rows, uint64_t nrec) {
    if (!nrec) return;
    hipLaunchKernelGGL(k_depth_fix, dim3((uint32_t)((nrec + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<ull *>(rows), nrec);
}

}  // namespace okm
