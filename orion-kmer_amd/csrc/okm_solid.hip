// okm_solid.hip — per-record solid runs of a batch of reads against a counted
// table (okm_read_solid_runs): for every record how many window positions
// (slots) it has, how many are solid (the window is valid, its canonical k-mer
// is in the table and its count reaches min_count), the longest run of
// consecutive solid slots, and the solid runs at its two ends.
//
// A run cannot cross records: the window that starts on a separator is
// invalid.  So over the whole batch the solid bits form one bit string whose
// maximal runs of ones each belong to one record, and the work splits in two:
//
// Stage 1, k_solid_mask: the search.  The read-batch scan of okm_read_scan.h
// (256 threads, 16 window starts each), one search in flight through
// FindDense / FindItems, but a thread forms 16 solid bits and
// 16 separator bits and stores them, coalesced, into two bit planes of one bit
// per batch byte (bit p & 63 of word p >> 6).  The first launch of a batch
// stores both planes plainly, over whole stage-2 tiles, so nothing is zeroed
// beforehand; every further slice of a host-resident table ORs its hits into
// the solid plane.  A thread owns its 16 bits: no atomics.  No record index,
// no scan.
//
// Stage 2 reads the planes only, n / 4 bytes.  A thread takes one 64-bit word
// of each plane, a wave 4096 positions, a workgroup 16384 (a tile):
//   k_runs_init   rows[r] = {start: past the end (0 for r = 0), end: n, 0 ...}
//   k_runs_tiles  per tile: its separators and the summary (all ones?,
//                 trailing ones) of its solid bits; the separator counts are
//                 then scanned (launch_exclusive_scan)
//   k_runs_carry  one workgroup scans the tile summaries, 256 per round, with
//                 combine(a, b) = b.all ? (a.all, a.suf + b.suf) : b: the run
//                 that enters each tile.  A plain reduce-then-scan: no kernel
//                 waits on another workgroup, no flags, no look-back.
//   k_runs_rows   redoes the scan inside the tile with the carry; every run
//                 END (bit i set, bit i + 1 clear; bit 64 is the next word's
//                 bit 0) knows its length from the ones below it in the word
//                 (+ the run entering the word when they reach bit 0), its
//                 record from the separator rank, and does one atomicMax on
//                 the row's packed best, len << 32 | (2^32 - 1 - start), so
//                 equal lengths resolve to the earliest start.  lead / trail
//                 are plain stores by the one run that starts behind a
//                 separator (or at 0) / ends k positions before one (or before
//                 n).  solid is a popcount per (thread, record piece), reduced
//                 per wave first when the wave holds no separator.
//                 The record starts and ends are scattered HERE (this kernel
//                 has the separator rank; k_runs_tiles does not), into the
//                 rows' own slots / run_start words, so no array of starts
//                 exists; lead and trail do not need them, they look at the
//                 separator plane.
//   k_runs_fix    per row: slots from start and end, the best unpacked,
//                 run_start relative to the record.
// Positions are 32 bits in the packed best: a batch holds < 2^32 bytes.
#include <hip/hip_runtime.h>

#include "okm_dev_common.h"
#include "okm_internal.h"
#include "okm_read_scan.h"
#include "okm_scan.h"
#include "okm_search.h"

namespace okm {

constexpr int kRunsBlock = 256;
constexpr int kRunsTile = kRunsBlock * 64;         // 16384 positions per stage-2 workgroup
static_assert(kRunsTile % kScanTile == 0, "stage 1 fills whole stage-2 tiles");
constexpr int kSolidRowWords = 6;  // okm_solid_run: slots, solid, run_start, run_len, lead, trail
static_assert(sizeof(okm_solid_run) == kSolidRowWords * sizeof(ull), "rows are six u64");
// Until k_runs_fix the row's words hold: 0 the record's first byte, 2 its end
// (its separator, or n), 3 the packed best; 1, 4 and 5 are final.
enum { kRowStart = 0, kRowSolid = 1, kRowEnd = 2, kRowBest = 3, kRowLead = 4, kRowTrail = 5 };

uint64_t solid_tiles(uint64_t n_bytes) { return (n_bytes + kRunsTile - 1) / kRunsTile; }
uint64_t solid_plane_words(uint64_t n_bytes) { return solid_tiles(n_bytes) * kRunsBlock; }

// ---------------------------------------------------------------------------
// Stage 1
// ---------------------------------------------------------------------------

// FIRST: the batch's first launch: stores both planes (zeros where there is
// nothing); otherwise ORs this table's hits into the solid plane.
template <typename KT, typename TAB, bool FIRST>
__global__ __launch_bounds__(kScanBlock) void k_solid_mask(const uint8_t *__restrict__ seq, uint64_t n, TAB tab,
                                                           uint32_t k, ull min_count, uint16_t *__restrict__ solid,
                                                           uint16_t *__restrict__ sep) {
    typedef KeyOps<KT> O;
    typedef ScanKeys<KT> SK;
    const uint64_t t = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;  // the planes' 16-bit word of this thread
    const uint64_t w0 = t * kScanSeg;
    typename SK::Words ww;
    load_windows<kScanSeg, SK::kHalo>(seq, n, w0, ww);  // bytes at or past n read as 0: no base, no separator
    typename SK::Coded c;
    make_codes<SK::kNP, false>(ww.w, c);  // count's validity: either case, U reads as T
    const uint32_t vmask = SK::valid_mask(c, k);
    tab.begin();
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < kScanSeg; ++j) {
        KT q[1];
        bool live[1], hit[1];
        ull cnt[1];
        live[0] = (vmask >> j) & 1u;
        q[0] = live[0] ? SK::key(c, j, k) : O::empty();
        tab.find(q, live, cnt, hit);
        bits |= (hit[0] && cnt[0] >= min_count ? 1u : 0u) << j;
    }
    if (FIRST) {
        solid[t] = (uint16_t)bits;
        sep[t] = (uint16_t)sep_mask_words(ww.w);
    } else if (bits) {
        solid[t] |= (uint16_t)bits;
    }
}

void launch_solid_mask(void *stream, const uint8_t *seq, uint64_t n, uint32_t k, bool wide, const TableView &t,
                       uint64_t min_count, bool first, unsigned long long *planes) {
    if (!n) return;
    const uint64_t words = solid_plane_words(n);
    uint16_t *solid = reinterpret_cast<uint16_t *>(planes), *sep = reinterpret_cast<uint16_t *>(planes + words);
    // the first launch covers the planes' every word; a later one only the batch
    const uint64_t bytes = first ? solid_tiles(n) * kRunsTile : n;
    const uint32_t nblocks = (uint32_t)((bytes + kScanTile - 1) / kScanTile);  // n < 2^32
    with_finder<1>(t, wide, [&](const auto &tab) {
        typedef std::decay_t<decltype(tab)> TAB;
        typedef typename TAB::Key KT;
        if (first)
            hipLaunchKernelGGL((k_solid_mask<KT, TAB, true>), dim3(nblocks), dim3(kScanBlock), 0, (hipStream_t)stream,
                               seq, n, tab, k, (ull)min_count, solid, sep);
        else
            hipLaunchKernelGGL((k_solid_mask<KT, TAB, false>), dim3(nblocks), dim3(kScanBlock), 0, (hipStream_t)stream,
                               seq, n, tab, k, (ull)min_count, solid, sep);
    });
}

// ---------------------------------------------------------------------------
// Stage 2
// ---------------------------------------------------------------------------

// A stretch of solid bits in batch order, summarised: bit 63 = it is all ones,
// the low bits = the ones at its end (its length when all ones).  kRunAll
// alone is the empty stretch, the operator's identity.
constexpr ull kRunAll = 1ull << 63;

__device__ __forceinline__ ull run_comb(ull a, ull b) {  // a, then b
    return (b >> 63) ? a + (b & ~kRunAll) : b;
}

__device__ __forceinline__ ull run_word(ull s) {  // position order is bit order: the end is the top
    return s == ~0ull ? (kRunAll | 64ull) : (ull)__clzll((long long)~s);
}

__device__ __forceinline__ ull below(int i) { return (1ull << i) - 1ull; }  // i < 64

// Exclusive scan of one summary per thread over the workgroup, in thread order;
// *total = all of them.  lds: kRunsBlock / 64 words.  Two barriers.
__device__ __forceinline__ ull block_excl_runs(ull v, ull *lds, ull *total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    ull inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const ull o = __shfl_up(inc, d, 64);
        if (lane >= d) inc = run_comb(o, inc);
    }
    if (lane == 63) lds[wid] = inc;
    lds_sync();
    ull pre = kRunAll, tot = kRunAll;
#pragma unroll
    for (int w = 0; w < kRunsBlock / 64; ++w) {
        const ull s = lds[w];
        if (w < wid) pre = run_comb(pre, s);
        tot = run_comb(tot, s);
    }
    lds_sync();
    ull ex = __shfl_up(inc, 1, 64);
    if (lane == 0) ex = kRunAll;
    *total = tot;
    return run_comb(pre, ex);
}

__global__ __launch_bounds__(256) void k_runs_init(ull *__restrict__ rows, uint64_t nrec, uint64_t n) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= nrec) return;
    ull *row = rows + r * kSolidRowWords;
    row[kRowStart] = r ? n + 1 : 0;  // until a separator says otherwise: no such record
    row[kRowSolid] = 0;
    row[kRowEnd] = n;  // ... and an unterminated one ends with the batch
    row[kRowBest] = row[kRowLead] = row[kRowTrail] = 0;
}

// tile_sep[t] = separators in tile t, tile_sum[t] = the summary of its solid
// bits: a wave reduction by shuffles (lane i comes to hold lanes i .. i + 2d -
// 1, in order), then the four waves through LDS.
__global__ __launch_bounds__(kRunsBlock) void k_runs_tiles(const ull *__restrict__ solid, const ull *__restrict__ sep,
                                                           ull *__restrict__ tile_sep, ull *__restrict__ tile_sum) {
    __shared__ ull lsum[kRunsBlock / 64], lsep[kRunsBlock / 64];
    const uint64_t w = (uint64_t)blockIdx.x * kRunsBlock + threadIdx.x;
    ull sum = run_word(solid[w]), ns = (ull)__popcll(sep[w]);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        sum = run_comb(sum, __shfl_down(sum, d, 64));
        ns += __shfl_down(ns, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        lsum[threadIdx.x >> 6] = sum;
        lsep[threadIdx.x >> 6] = ns;
    }
    lds_sync();
    if (threadIdx.x == 0) {
        sum = kRunAll;
        ns = 0;
#pragma unroll
        for (int i = 0; i < kRunsBlock / 64; ++i) {
            sum = run_comb(sum, lsum[i]);
            ns += lsep[i];
        }
        tile_sum[blockIdx.x] = sum;
        tile_sep[blockIdx.x] = ns;
    }
}

// carry[t] = the summary of everything before tile t.  ONE workgroup.
__global__ __launch_bounds__(kRunsBlock) void k_runs_carry(const ull *__restrict__ tile_sum, uint64_t ntiles,
                                                           ull *__restrict__ carry) {
    __shared__ ull lds[kRunsBlock / 64];
    ull before = kRunAll;  // everything before this round
    for (uint64_t base = 0; base < ntiles; base += kRunsBlock) {
        const uint64_t t = base + threadIdx.x;
        ull tot;
        const ull ex = block_excl_runs(t < ntiles ? tile_sum[t] : kRunAll, lds, &tot);
        if (t < ntiles) carry[t] = run_comb(before, ex);
        before = run_comb(before, tot);
    }
}

__device__ __forceinline__ bool plane_bit(const ull *__restrict__ plane, uint64_t p) {
    return (plane[p >> 6] >> (p & 63)) & 1ull;
}

__global__ __launch_bounds__(kRunsBlock) void k_runs_rows(const ull *__restrict__ solid, const ull *__restrict__ sep,
                                                          uint64_t nwords, uint64_t n, uint32_t k,
                                                          const ull *__restrict__ tile_pre,
                                                          const ull *__restrict__ carry, ull *__restrict__ rows,
                                                          uint64_t nrec) {
    __shared__ ull lds[kRunsBlock / 64], wsum[kRunsBlock / 64];
    const uint64_t w = (uint64_t)blockIdx.x * kRunsBlock + threadIdx.x;  // < nwords: whole tiles
    const uint64_t p0 = w * 64;
    const ull s = solid[w], e = sep[w];
    ull tot;
    // the solid positions right before this word, and the record its first position lies in
    const ull in = run_comb(carry[blockIdx.x], block_excl_runs(run_word(s), lds, &tot)) & ~kRunAll;
    const ull rec = tile_pre[blockIdx.x] + block_excl_scan<kRunsBlock>((ull)__popcll(e), wsum, &tot);
    // (no thread leaves early: the wave reduction below needs every lane)

    // solid per record piece of the word; a separator ends its record and starts the next
    if (__ballot(e != 0) == 0) {  // the wave lies inside one record: one add for its 4096 positions
        ull c = (ull)__popcll(s);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
        if ((threadIdx.x & 63) == 0 && c && rec < nrec) atomicAdd(rows + rec * kSolidRowWords + kRowSolid, c);
    } else {
        ull m = e, r = rec;
        for (int lo = 0; lo < 64;) {
            const int hi = m ? __ffsll((long long)m) - 1 : 64;  // the piece [lo, hi)
            const ull piece = s & ~below(lo) & (hi < 64 ? below(hi) : ~0ull);
            if (piece && r < nrec) atomicAdd(rows + r * kSolidRowWords + kRowSolid, (ull)__popcll(piece));
            if (hi == 64) break;
            if (r < nrec) rows[r * kSolidRowWords + kRowEnd] = p0 + hi;
            if (r + 1 < nrec) rows[(r + 1) * kSolidRowWords + kRowStart] = p0 + hi + 1;
            ++r;
            lo = hi + 1;
            m &= m - 1;
        }
    }

    // every run that ends in this word
    const ull nxt = w + 1 < nwords ? solid[w + 1] & 1ull : 0ull;
    for (ull ends = s & ~((s >> 1) | (nxt << 63)); ends; ends &= ends - 1) {
        const int i = __ffsll((long long)ends) - 1;
        const ull r = rec + (ull)__popcll(e & below(i));  // (a solid position is no separator)
        if (r >= nrec) continue;
        const ull zb = ~s & below(i);  // the zeros below the end: the run starts above the highest
        const ull len = zb ? (ull)(i - (63 - __clzll((long long)zb))) : (ull)(i + 1) + in;
        const uint64_t end = p0 + i;
        if (len > end + 1 || end + k > n) continue;  // cannot be: a run lies inside the batch, its windows too
        const uint64_t start = end + 1 - len;
        ull *row = rows + r * kSolidRowWords;
        atomicMax(row + kRowBest, (len << 32) | (0xFFFFFFFFull - start));
        if (start == 0 || plane_bit(sep, start - 1)) row[kRowLead] = len;
        // the window at `end` is valid: no separator in [end, end + k), and end + k <= n
        const uint64_t q = end + k;
        if (q >= n || plane_bit(sep, q)) row[kRowTrail] = len;
    }
}

__global__ __launch_bounds__(256) void k_runs_fix(ull *__restrict__ rows, uint64_t nrec, uint32_t k) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= nrec) return;
    ull *row = rows + r * kSolidRowWords;
    const ull start = row[kRowStart], end = row[kRowEnd], best = row[kRowBest];
    const ull len = end > start ? end - start : 0;  // (a row past the last record: start = n + 1)
    const ull run_len = best >> 32;
    row[0] = len >= k ? len - k + 1 : 0;
    row[2] = run_len ? (0xFFFFFFFFull - (best & 0xFFFFFFFFull)) - start : 0;
    row[3] = run_len;
}

void launch_solid_runs(void *stream, uint64_t n, uint64_t nrec, uint32_t k, const unsigned long long *planes,
                       unsigned long long *tiles, okm_solid_run *rows) {
    if (!n || !nrec) return;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t nt = solid_tiles(n), words = solid_plane_words(n);  // nt <= 2^18
    const ull *solid = planes, *sep = planes + words;
    ull *cnt = tiles, *pre = cnt + nt, *sum = pre + nt, *carry = sum + nt, *scr = carry + nt;
    ull *r = reinterpret_cast<ull *>(rows);
    const uint32_t rblocks = (uint32_t)((nrec + 255) / 256);
    hipLaunchKernelGGL(k_runs_init, dim3(rblocks), dim3(256), 0, s, r, nrec, n);
    hipLaunchKernelGGL(k_runs_tiles, dim3((uint32_t)nt), dim3(kRunsBlock), 0, s, solid, sep, cnt, sum);
    launch_exclusive_scan(stream, cnt, pre, nt, scr);
    hipLaunchKernelGGL(k_runs_carry, dim3(1), dim3(kRunsBlock), 0, s, sum, nt, carry);
    hipLaunchKernelGGL(k_runs_rows, dim3((uint32_t)nt), dim3(kRunsBlock), 0, s, solid, sep, words, n, k, pre, carry, r,
                       nrec);
    hipLaunchKernelGGL(k_runs_fix, dim3(rblocks), dim3(256), 0, s, r, nrec, k);
}

}  // namespace okm
