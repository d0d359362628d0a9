// okm_compare.hip — two counted tables compared where they lie
// (okm_compare_counts): the keys both hold, with the sums of their counts, and
// each side's own totals.
//
// Both tables are sorted by key, so the comparison is a merge, not a search
// per key: every entry of either table is read from memory once.
//
// One view for every representation: a TableView's run list (the first key of
// every run, a LookItem per run, the number of runs on the device).  For a count's pending
// per-item runs it is what launch_lookup_index builds; a dense table (or one
// uploaded slice of a host-resident one) is cut into pieces of one tile by
// k_cmp_cut.  The kernels below have one form per key type and count width, not
// one per pair of representations.
//
// The driving table D (the caller passes the larger one) is split into tiles
// of at most T consecutive entries of one run (k_cmp_tile_counts + a scan).
// k_cmp_bounds, one thread per tile, finds the tile's run and the range of the
// other table S that its key span [first, last] covers, by the two-level
// search the lookup uses: ~50 dependent loads per tile that would otherwise
// stand in front of every workgroup of the merge, where one thread per tile
// lets occupancy hide them.  k_compare_tiles, one workgroup per tile, loads the
// tile's keys and counts into LDS once, streams its S range through a second
// LDS buffer in chunks of at most T entries (walking from S run to S run by
// the descriptors: the runs are not contiguous), and merges each chunk with
// the tile: every thread takes an equal share of the merged sequence by a
// diagonal (merge-path) search and walks it; equal keys are the shared ones.
//
// LDS per workgroup: the keys of both buffers and a u32 per count, whatever
// the tables' count width (a u64 count is staged saturated; a match that finds
// the saturated value fetches the count itself, and a chunk of S then ends
// where the next run's counts do not follow on in memory):
//   u64 keys,  T = 1024: 2 x 8 KB + 2 x 4 KB = 24 KB: six workgroups per CU
//   K128 keys, T = 512:  2 x 8 KB + 2 x 2 KB = 20 KB: seven
// of gfx950's 160 KB.  The merge waits on the chain of dependent global loads
// in front of every tile (tile, descriptor, keys), not on LDS, so the resident
// workgroups decide: T = 1024 measured 1.58 ms against 2.43 at 2048 and 1.87
// at 512 on two pending C2 tables, and two dense tables with their u64 counts
// staged whole (32 KB, five workgroups) took 1.85 ms against 1.52 staged as
// u32 (profiles/AB_LOG.md).  Counts lie in LDS beside their keys, so a match
// costs two LDS reads whatever S run its key came from.
//
// Known limits.  The work is split by D's tiles, so an S that is dense inside
// one tile's key span is streamed by that tile's workgroup alone; with the
// larger table as D, tables of real k-mers keep that range near one chunk.
// k_cmp_totals takes one workgroup per run, so a table of few, very long runs
// would stream its counts through few workgroups; a count's runs hold at most
// a few thousand entries and a dense table is cut into pieces of T.
#include <hip/hip_runtime.h>

#include "okm_cmp_stage.h"
#include "okm_dev_common.h"
#include "okm_internal.h"
#include "okm_search.h"

namespace okm {

constexpr uint32_t kCmpSlots = 256, kCmpSlotWords = 16;  // the merge's result slots: one 128-B line each

uint32_t compare_tile(bool wide) { return wide ? CmpTileOf<K128>::T : CmpTileOf<ull>::T; }

uint64_t compare_max_tiles(uint64_t n, uint32_t max_runs, uint32_t tile) {
    return n / tile + max_runs + 1;  // sum of ceil(n_r / T) <= n / T + runs
}

// A dense table as a run list: pieces of T entries.
template <typename KT>
__global__ __launch_bounds__(256) void k_cmp_cut(const KT *__restrict__ keys, ull n, uint32_t T,
                                                 KT *__restrict__ first, LookItem *__restrict__ desc,
                                                 ull *__restrict__ n_desc) {
    const ull i = (ull)blockIdx.x * 256 + threadIdx.x, nr = (n + T - 1) / T;
    if (i == 0) *n_desc = nr;
    if (i >= nr) return;
    first[i] = keys[i * T];
    LookItem d;
    d.keys = reinterpret_cast<const uint64_t *>(keys + i * T);
    d.coff = i * T;
    d.n = n - i * T < T ? n - i * T : T;
    desc[i] = d;
}

// cnt[r] = tiles of run r, r < *n_desc; 0 for the slots up to max_runs (the scan's total lands in the last)
__global__ __launch_bounds__(256) void k_cmp_tile_counts(const LookItem *__restrict__ desc,
                                                         const ull *__restrict__ n_desc, uint32_t max_runs,
                                                         uint32_t T, ull *__restrict__ cnt) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i <= max_runs) cnt[i] = i < max_runs && i < *n_desc ? (desc[i].n + T - 1) / T : 0ull;
}

// wave sums of v[0..N), then one LDS word set per wave, then N atomics per
// workgroup at most (none when v[0], the entry count, is 0 over the workgroup).
// Every wave of the workgroup calls this once.
template <int N>
__device__ __forceinline__ void cmp_flush(ull (&v)[N], ull *__restrict__ out) {
    __shared__ ull wred[kCmpBlock / 64][N];
#pragma unroll
    for (int q = 0; q < N; ++q) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v[q] += __shfl_xor(v[q], d, 64);
        if ((threadIdx.x & 63u) == 0) wred[threadIdx.x >> 6][q] = v[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ull t[N];
#pragma unroll
        for (int q = 0; q < N; ++q) {
            t[q] = 0;
#pragma unroll
            for (int w = 0; w < kCmpBlock / 64; ++w) t[q] += wred[w][q];
        }
        if (t[0]) {
#pragma unroll
            for (int q = 0; q < N; ++q) atomicAdd(&out[q], t[q]);
        }
    }
}

// out[0] += entries with count >= min_count, out[1] += the sum of their counts
// (mod 2^64): only the counts are read, run by run, u32 words when NARROW.
template <bool NARROW>
__global__ __launch_bounds__(kCmpBlock) void k_cmp_totals(const LookItem *__restrict__ desc,
                                                          const ull *__restrict__ n_desc,
                                                          const uint64_t *__restrict__ sc, ull min_count,
                                                          ull *__restrict__ out) {
    const ull m = *n_desc;
    const uint32_t *sc32 = reinterpret_cast<const uint32_t *>(sc);
    ull v[2] = {0, 0};
    for (ull r = blockIdx.x; r < m; r += gridDim.x) {
        const ull n = desc[r].n, coff = desc[r].coff;
        for (ull i = threadIdx.x; i < n; i += kCmpBlock) {
            const ull c = NARROW ? (ull)sc32[coff + i] : (ull)sc[coff + i];
            if (c >= min_count) {
                v[0] += 1;
                v[1] += c;
            }
        }
    }
    cmp_flush<2>(v, out);
}

// One thread per tile of D: its run and place in it, and the S range that its
// key span covers, [(s_run0, s_off0), (s_run1, s_off1)): an empty one is
// written as s_run0 = 1 > s_run1 = 0.  toff = the exclusive scan of the runs'
// tile counts (toff[max_runs] = tiles in all).
template <typename KT>
__global__ __launch_bounds__(256) void k_cmp_bounds(const LookItem *__restrict__ ddesc,
                                                    const ull *__restrict__ dn_desc, const ull *__restrict__ toff,
                                                    uint32_t max_runs, const KT *__restrict__ sfirst,
                                                    const LookItem *__restrict__ sdesc,
                                                    const ull *__restrict__ sn_desc, uint32_t T,
                                                    CmpTile *__restrict__ tiles) {
    typedef KeyOps<KT> O;
    const ull t = (ull)blockIdx.x * 256 + threadIdx.x;
    if (t >= toff[max_runs]) return;
    // every run has a tile, so toff rises strictly over the runs and the last toff[r] <= t is t's run: no
    // producer of a run list writes an empty run (launch_lookup_index drops the items that own no key,
    // k_cmp_cut's pieces hold at least one entry); one that did would break this search
    const FlatKeys<ull> ta[1] = {{toff}};
    const ull tn[1] = {*dn_desc}, tq[1] = {t};
    ull tp[1], tl[1];
    search_last_le<ull, 1>(ta, tn, tq, tp, tl);
    const LookItem *d = ddesc + tp[0];
    const KT *kp = reinterpret_cast<const KT *>(gload(&d->keys));
    const ull dn = gload(&d->n), d_off = (t - tl[0]) * T;
    const uint32_t d_len = (uint32_t)(dn - d_off < T ? dn - d_off : T);
    const KT q[2] = {gload(kp + d_off), gload(kp + d_off + d_len - 1)};
    // the S run whose first key is the last one <= q, then the last key <= q in it (as k_lookup_items)
    const ull ms = *sn_desc;
    FlatKeys<KT> a[2] = {{sfirst}, {sfirst}};
    ull len[2] = {ms, ms}, pos[2], run[2];
    KT last[2];
    search_last_le<KT, 2>(a, len, q, pos, last);
    bool owned[2];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        owned[f] = len[f] && !O::lt(q[f], last[f]);  // else: below S's first key
        run[f] = pos[f];
        len[f] = 0;
        if (owned[f]) {
            a[f].p = reinterpret_cast<const KT *>(gload(&sdesc[pos[f]].keys));
            len[f] = gload(&sdesc[pos[f]].n);
        }
    }
    search_last_le<KT, 2>(a, len, q, pos, last);
    // begin: the first S entry >= the tile's first key (past a run's end: the next run's first)
    ull r0 = 0, o0 = 0;
    if (owned[0]) {
        r0 = run[0];
        o0 = pos[0] + (O::eq(last[0], q[0]) ? 0 : 1);
        if (o0 == len[0]) {
            ++r0;
            o0 = 0;
        }
    }
    // end: behind the last S entry <= the tile's last key
    const ull r1 = owned[1] ? run[1] : 0, o1 = owned[1] ? pos[1] + 1 : 0;
    CmpTile w;
    w.d_run = (uint32_t)tp[0];
    w.d_len = d_len;
    w.d_off = d_off;
    const bool empty = r0 > r1 || (r0 == r1 && o0 >= o1);
    w.s_run0 = empty ? 1u : (uint32_t)r0;
    w.s_run1 = empty ? 0u : (uint32_t)r1;
    w.s_off0 = empty ? 0 : o0;
    w.s_off1 = empty ? 0 : o1;
    tiles[t] = w;
}

// out[0] += keys in both tables whose counts pass both thresholds, out[1] +=
// the sum of min(count_d, count_s) over them, out[2] += of count_d, out[3] +=
// of count_s (all mod 2^64).  One workgroup per tile of D; workgroups past the
// last tile (the grid is the host's bound) and tiles with an empty S range
// leave at once.
template <typename KT, bool NARROW_D, bool NARROW_S>
__global__ __launch_bounds__(kCmpBlock) void k_compare_tiles(const CmpTile *__restrict__ tiles,
                                                             const ull *__restrict__ n_tiles,
                                                             const LookItem *__restrict__ ddesc,
                                                             const uint64_t *__restrict__ dcounts,
                                                             const LookItem *__restrict__ sdesc,
                                                             const uint64_t *__restrict__ scounts, ull min_d,
                                                             ull min_s, ull *__restrict__ out) {
    typedef KeyOps<KT> O;
    constexpr uint32_t T = CmpTileOf<KT>::T;
    __shared__ KT dk[T], sk[T];
    __shared__ uint32_t dc[T], sc[T];
    if (blockIdx.x >= *n_tiles) return;
    const CmpTile t = tiles[blockIdx.x];
    if (t.s_run0 > t.s_run1 || (t.s_run0 == t.s_run1 && t.s_off0 >= t.s_off1)) return;
    const uint32_t dl = t.d_len;
    cmp_stage<KT, NARROW_D>(ddesc + t.d_run, t.d_off, dl, dcounts, dk, dc);
    const ull dc0 = gload(&ddesc[t.d_run].coff) + t.d_off;  // where the tile's counts lie
    ull v[4] = {0, 0, 0, 0};
    uint32_t run = t.s_run0;
    ull off = t.s_off0;
    for (;;) {  // one chunk of the S range per round; every value that steers the loops is workgroup-uniform
        uint32_t sl = 0;
        ull sc0 = 0;  // where the chunk's counts lie: one range of the count array (a saturated one is fetched)
        while (sl < T && run <= t.s_run1) {
            const ull rend = run == t.s_run1 ? t.s_off1 : gload(&sdesc[run].n);
            if (off >= rend) {  // this run is done (the last one: the range is)
                if (run == t.s_run1) break;
                ++run;
                off = 0;
                continue;
            }
            const uint32_t take = (uint32_t)(rend - off < T - sl ? rend - off : T - sl);
            if (!NARROW_S) {  // u64 counts: the chunk ends where the next run's counts do not follow on
                const ull at = gload(&sdesc[run].coff) + off;
                if (!sl) sc0 = at;
                if (at != sc0 + sl) break;
            }
            cmp_stage<KT, NARROW_S>(sdesc + run, off, take, scounts, sk + sl, sc + sl);
            sl += take;
            off += take;
        }
        if (!sl) break;
        __syncthreads();
        // this thread's share of the merged sequence (ties: D's entry first): steps [diag, dend)
        const uint32_t total = dl + sl, per = (total + kCmpBlock - 1) / kCmpBlock;
        const uint32_t diag = min(threadIdx.x * per, total), dend = min(diag + per, total);
        uint32_t lo = diag > sl ? diag - sl : 0u, hi = min(diag, dl);
        while (lo < hi) {  // i = D entries among the first diag merged ones
            const uint32_t mid = (lo + hi) >> 1;
            if (!O::lt(sk[diag - 1 - mid], dk[mid]))
                lo = mid + 1;
            else
                hi = mid;
        }
        uint32_t i = lo, j = diag - lo;
        KT kd = i < dl ? dk[i] : O::empty(), ks = j < sl ? sk[j] : O::empty();
        for (uint32_t step = diag; step < dend; ++step) {
            const bool has_d = i < dl, has_s = j < sl;
            if (has_d && (!has_s || !O::lt(ks, kd))) {
                if (has_s && O::eq(kd, ks)) {  // S's equal key is still ahead of j: each pair is seen once
                    ull cd = dc[i], cs = sc[j];
                    if (!NARROW_D && cd == kCmpSat) cd = dcounts[dc0 + i];
                    if (!NARROW_S && cs == kCmpSat) cs = scounts[sc0 + j];
                    if (cd >= min_d && cs >= min_s) {
                        v[0] += 1;
                        v[1] += cd < cs ? cd : cs;
                        v[2] += cd;
                        v[3] += cs;
                    }
                }
                ++i;
                if (i < dl) kd = dk[i];
            } else {
                ++j;
                if (j < sl) ks = sk[j];
            }
        }
        __syncthreads();  // the next chunk overwrites sk / sc
    }
    // every workgroup ends on these four sums, and atomics on one line queue at the memory side (54 K tiles on
    // one line: 3.5 ms where the merge itself takes under 1; profiles/AB_LOG.md): kCmpSlots lines take them in turn
    cmp_flush<4>(v, out + (size_t)(blockIdx.x % kCmpSlots) * kCmpSlotWords);
}

// out[q] += the sum of the slots' word q, q < 4: one workgroup, one slot per thread.
__global__ __launch_bounds__(kCmpBlock) void k_cmp_fold(const ull *__restrict__ slots, ull *__restrict__ out) {
    static_assert(kCmpSlots == kCmpBlock, "one slot per thread");
    ull v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = slots[(size_t)threadIdx.x * kCmpSlotWords + q];
    cmp_flush<4>(v, out);
}

size_t compare_slot_words() { return (size_t)kCmpSlots * kCmpSlotWords; }

void launch_compare_fold(void *stream, const unsigned long long *slots, unsigned long long *out) {
    hipLaunchKernelGGL(k_cmp_fold, dim3(1), dim3(kCmpBlock), 0, (hipStream_t)stream, slots, out);
}

void launch_compare_cut(void *stream, const uint64_t *keys, uint64_t n, bool wide, uint32_t T, uint64_t *first,
                        LookItem *desc, unsigned long long *n_desc) {
    const dim3 g((uint32_t)((n + T - 1) / T / 256 + 1)), b(256);
    hipStream_t s = (hipStream_t)stream;
    if (wide)
        hipLaunchKernelGGL(k_cmp_cut<K128>, g, b, 0, s, reinterpret_cast<const K128 *>(keys), n, T,
                           reinterpret_cast<K128 *>(first), desc, n_desc);
    else
        hipLaunchKernelGGL(k_cmp_cut<ull>, g, b, 0, s, reinterpret_cast<const ull *>(keys), n, T,
                           reinterpret_cast<ull *>(first), desc, n_desc);
}

void launch_compare_totals(void *stream, const TableView &v, uint64_t min_count, unsigned long long *out) {
    if (!v.max_runs) return;
    const dim3 g(v.max_runs < 2048u ? v.max_runs : 2048u), b(kCmpBlock);
    hipStream_t s = (hipStream_t)stream;
    if (v.narrow)
        hipLaunchKernelGGL(k_cmp_totals<true>, g, b, 0, s, v.desc, v.n_desc, v.counts, min_count, out);
    else
        hipLaunchKernelGGL(k_cmp_totals<false>, g, b, 0, s, v.desc, v.n_desc, v.counts, min_count, out);
}

template <typename KT>
static void compare_bounds(hipStream_t s, const TableView &d, const TableView &sv, const unsigned long long *toff,
                           CmpTile *tiles) {
    const uint32_t T = compare_tile(sizeof(KT) == 16);
    const uint64_t max_tiles = compare_max_tiles(d.n, d.max_runs, T);
    hipLaunchKernelGGL(k_cmp_bounds<KT>, dim3((uint32_t)(max_tiles / 256 + 1)), dim3(256), 0, s, d.desc, d.n_desc, toff,
                       d.max_runs, reinterpret_cast<const KT *>(sv.first), sv.desc, sv.n_desc, T, tiles);
}

void launch_compare_bounds(void *stream, const TableView &d, const TableView &sv, bool wide,
                           const unsigned long long *toff, CmpTile *tiles) {
    if (wide)
        compare_bounds<K128>((hipStream_t)stream, d, sv, toff, tiles);
    else
        compare_bounds<ull>((hipStream_t)stream, d, sv, toff, tiles);
}

template <typename KT>
static void compare_tiles(hipStream_t s, const TableView &d, const TableView &sv, uint64_t min_d, uint64_t min_s,
                          const unsigned long long *toff, CmpTile *tiles, unsigned long long *out) {
    const uint64_t max_tiles = compare_max_tiles(d.n, d.max_runs, compare_tile(sizeof(KT) == 16));
    compare_bounds<KT>(s, d, sv, toff, tiles);
    const dim3 g((uint32_t)max_tiles), b(kCmpBlock);
    const unsigned long long *nt = toff + d.max_runs;
#define OKM_CMP_LAUNCH(ND, NS)                                                                                 \
    hipLaunchKernelGGL((k_compare_tiles<KT, ND, NS>), g, b, 0, s, tiles, nt, d.desc, d.counts, sv.desc, sv.counts, \
                       min_d, min_s, out)
    if (d.narrow && sv.narrow)
        OKM_CMP_LAUNCH(true, true);
    else if (d.narrow)
        OKM_CMP_LAUNCH(true, false);
    else if (sv.narrow)
        OKM_CMP_LAUNCH(false, true);
    else
        OKM_CMP_LAUNCH(false, false);
#undef OKM_CMP_LAUNCH
}

void launch_compare_tile_offsets(void *stream, const TableView &d, uint32_t tile, unsigned long long *toff,
                                 unsigned long long *scan_tmp) {
    hipLaunchKernelGGL(k_cmp_tile_counts, dim3(d.max_runs / 256u + 1u), dim3(256), 0, (hipStream_t)stream, d.desc,
                       d.n_desc, d.max_runs, tile, toff);
    launch_exclusive_scan(stream, toff, toff, (uint64_t)d.max_runs + 1, scan_tmp);
}

void launch_compare(void *stream, const TableView &d, const TableView &sv, bool wide, uint64_t min_d, uint64_t min_s,
                    unsigned long long *toff, unsigned long long *scan_tmp, CmpTile *tiles, unsigned long long *out) {
    if (!d.max_runs || !sv.max_runs) return;
    hipStream_t s = (hipStream_t)stream;
    launch_compare_tile_offsets(stream, d, compare_tile(wide), toff, scan_tmp);
    if (wide)
        compare_tiles<K128>(s, d, sv, min_d, min_s, toff, tiles, out);
    else
        compare_tiles<ull>(s, d, sv, min_d, min_s, toff, tiles, out);
}

}  // namespace okm
