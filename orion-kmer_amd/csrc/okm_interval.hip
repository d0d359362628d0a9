// okm_interval.hip — per-record count intervals of a batch of reads against a
// counted table (okm_read_count_intervals): every maximal stretch of a record
// whose windows' counts lie in [lo, hi], an absent k-mer counting 0, as rows
// {record, start, end} in (record, start) order.  The one reader whose output
// has no fixed size.
//
// Stage 1, k_interval_mask: the search, k_solid_mask's (okm_solid.hip) with
// another predicate.  The read-batch scan of okm_read_scan.h (256 threads, 16
// window starts each), one search in flight, 16 selected bits and 16 separator
// bits a thread, stored into the two bit planes of the solid runs (one bit per
// batch byte, bit p & 63 of word p >> 6, whole stage-2 tiles).  The first
// launch of a batch stores both planes plainly, with
//     bit = valid && (hit ? lo <= count <= hi : lo == 0);
// every further slice of a host-resident table OVERRIDES the thread's own bits
// where it hit (set or cleared by the count) and leaves them alone where it
// missed: a key lies in at most one slice, so the lo == 0 default survives for
// exactly the k-mers no slice holds.  Not an OR, no atomics.
//
// Stage 2 reads the planes only.  A thread takes one 64-bit word of each
// plane, a workgroup 16384 positions (a tile), as k_runs_* do.  Its word of
// the plane the runs are taken from is
//     slot units, or k = 1:  sel[w]
//     base units:            the bases a selected window covers: sel dilated
//                            by k - 1, x | x << 1 | ... | x << (k - 1), in
//                            log steps over the 128-bit pair sel[w - 1] : sel[w]
//                            (k - 1 <= 63: one neighbour is enough).  Never
//                            stored.
// with the plane's bit below the word (bit 63 of the word before) and above it
// (bit 0 of the next) from the neighbours' sel words alone.  A run START is a
// set bit over a clear one, a run END a set bit under a clear one.
//   k_interval_tiles   per tile: its run starts and its separators; both are
//                      then scanned (launch_exclusive_scan)
//   k_interval_bounds  first[r] = the batch position of record r's first byte,
//                      from the separator plane and its scan
//   k_interval_emit    redoes both scans inside the tile.  A run's row is the
//                      number of starts before its start; the thread that
//                      holds its end knows the same number as (starts at
//                      positions <= end) - 1.  So start and end are two plain
//                      stores, by possibly different threads of different
//                      tiles: no carry of run lengths, no look-back, no
//                      atomics.  Nothing is stored at or past `cap`.
// Rows of records past nrec lie behind all others (rows ascend by record), so
// they are cut off by the total alone: the thread that holds separator nrec - 1
// stores the starts before it as the total, or the batch's last thread all of
// them when there is no such separator.  One writer either way.
// Positions are 32 bits in first[]: a batch holds < 2^32 bytes.
#include <hip/hip_runtime.h>

#include "okm_dev_common.h"
#include "okm_internal.h"
#include "okm_read_scan.h"
#include "okm_scan.h"
#include "okm_search.h"

namespace okm {

constexpr int kIvalBlock = 256;
constexpr int kIvalTile = kIvalBlock * 64;  // the solid runs' tile: the planes are theirs
static_assert(sizeof(okm_count_interval) == 3 * sizeof(ull), "rows are three u64");
enum { kIvalRecord = 0, kIvalStart = 1, kIvalEnd = 2 };

// first[] holds a record for every separator of the batch at most, and none past nrec
static uint64_t interval_records(uint64_t n_bytes, uint64_t nrec) { return nrec < n_bytes + 1 ? nrec : n_bytes + 1; }

uint64_t interval_tile_words(uint64_t n_bytes, uint64_t nrec) {
    const uint64_t nt = solid_tiles(n_bytes);
    // run starts and separators per tile (+ 1: the totals), their scans, the scans' scratch, the total, first[]
    return 4 * (nt + 1) + scan_tmp_elems(nt + 1) + 1 + (interval_records(n_bytes, nrec) + 1) / 2;
}

// ---------------------------------------------------------------------------
// Stage 1
// ---------------------------------------------------------------------------

// FIRST: the batch's first launch: stores both planes (zeros where there is
// nothing); otherwise this table's hits override the thread's own bits.
template <typename KT, typename TAB, bool FIRST>
__global__ __launch_bounds__(kScanBlock) void k_interval_mask(const uint8_t *__restrict__ seq, uint64_t n, TAB tab,
                                                              uint32_t k, ull lo, ull hi, uint16_t *__restrict__ sel,
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
    uint32_t bits = 0, hits = 0;
#pragma unroll
    for (int j = 0; j < kScanSeg; ++j) {
        KT q[1];
        bool live[1], hit[1];
        ull cnt[1];
        live[0] = (vmask >> j) & 1u;
        q[0] = live[0] ? SK::key(c, j, k) : O::empty();
        tab.find(q, live, cnt, hit);
        const bool found = live[0] && hit[0];
        hits |= (found ? 1u : 0u) << j;
        const bool on = found ? lo <= cnt[0] && cnt[0] <= hi : FIRST && live[0] && lo == 0;
        bits |= (on ? 1u : 0u) << j;
    }
    if (FIRST) {
        sel[t] = (uint16_t)bits;
        sep[t] = (uint16_t)sep_mask_words(ww.w);
    } else if (hits) {
        sel[t] = (uint16_t)((sel[t] & ~hits) | bits);
    }
}

void launch_interval_mask(void *stream, const uint8_t *seq, uint64_t n, uint32_t k, bool wide, const TableView &t,
                          uint64_t lo, uint64_t hi, bool first, unsigned long long *planes) {
    if (!n) return;
    const uint64_t words = solid_plane_words(n);
    uint16_t *sel = reinterpret_cast<uint16_t *>(planes), *sep = reinterpret_cast<uint16_t *>(planes + words);
    // the first launch covers the planes' every word; a later one only the batch
    const uint64_t bytes = first ? solid_tiles(n) * kIvalTile : n;
    const uint32_t nblocks = (uint32_t)((bytes + kScanTile - 1) / kScanTile);  // n < 2^32
    with_finder<1>(t, wide, [&](const auto &tab) {
        typedef std::decay_t<decltype(tab)> TAB;
        typedef typename TAB::Key KT;
        if (first)
            hipLaunchKernelGGL((k_interval_mask<KT, TAB, true>), dim3(nblocks), dim3(kScanBlock), 0,
                               (hipStream_t)stream, seq, n, tab, k, (ull)lo, (ull)hi, sel, sep);
        else
            hipLaunchKernelGGL((k_interval_mask<KT, TAB, false>), dim3(nblocks), dim3(kScanBlock), 0,
                               (hipStream_t)stream, seq, n, tab, k, (ull)lo, (ull)hi, sel, sep);
    });
}

// ---------------------------------------------------------------------------
// Stage 2
// ---------------------------------------------------------------------------

__device__ __forceinline__ ull ival_below(int i) { return (1ull << i) - 1ull; }  // i < 64

// Word w of the plane the runs are taken from, and its run starts and ends.
// d = 0: the selection plane itself; else it dilated by d (= k - 1, 1 .. 63).
struct IvalWord {
    ull starts, ends;
};
__device__ __forceinline__ IvalWord interval_word(const ull *__restrict__ sel, uint64_t w, uint64_t nwords,
                                                  uint32_t d) {
    const ull cur = sel[w], prv = w ? sel[w - 1] : 0ull, nxt = w + 1 < nwords ? sel[w + 1] : 0ull;
    ull b = cur, under = prv >> 63, over = nxt & 1ull;
    if (d) {
        ull hi = cur, lo = prv;  // the pair hi : lo, dilated by d; only hi is wanted
        uint32_t len = 1;        // hi : lo bit j = any selected slot in j - len + 1 .. j
        while (2 * len <= d + 1) {
            hi |= (hi << len) | (lo >> (64 - len));  // len <= 32
            lo |= lo << len;
            len *= 2;
        }
        const uint32_t r = d + 1 - len;  // < len: the two stretches of len overlap
        if (r) hi |= (hi << r) | (lo >> (64 - r));
        b = hi;
        // bit 63 of the word before: a selected slot among its top d + 1; bit 0 of the next: its own
        // slot 0 or one of this word's top d
        under = (prv >> (63 - d)) != 0;
        over |= (cur >> (64 - d)) != 0;
    }
    IvalWord o;
    o.starts = b & ~((b << 1) | under);
    o.ends = b & ~((b >> 1) | (over << 63));
    return o;
}

// tile_run[t] = run starts in tile t, tile_sep[t] = its separators; entry
// gridDim.x of both = 0, so that the scans' entry gridDim.x is the total.
__global__ __launch_bounds__(kIvalBlock) void k_interval_tiles(const ull *__restrict__ sel, const ull *__restrict__ sep,
                                                               uint64_t nwords, uint32_t d, ull *__restrict__ tile_run,
                                                               ull *__restrict__ tile_sep) {
    __shared__ ull lrun[kIvalBlock / 64], lsep[kIvalBlock / 64];
    const uint64_t w = (uint64_t)blockIdx.x * kIvalBlock + threadIdx.x;  // < nwords: whole tiles
    ull nr = (ull)__popcll(interval_word(sel, w, nwords, d).starts), ns = (ull)__popcll(sep[w]);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        nr += __shfl_xor(nr, s, 64);
        ns += __shfl_xor(ns, s, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        lrun[threadIdx.x >> 6] = nr;
        lsep[threadIdx.x >> 6] = ns;
    }
    lds_sync();
    if (threadIdx.x == 0) {
        nr = ns = 0;
#pragma unroll
        for (int i = 0; i < kIvalBlock / 64; ++i) {
            nr += lrun[i];
            ns += lsep[i];
        }
        tile_run[blockIdx.x] = nr;
        tile_sep[blockIdx.x] = ns;
        if (blockIdx.x == 0) tile_run[gridDim.x] = tile_sep[gridDim.x] = 0;
    }
}

// first[r] = the position behind separator r - 1 (0 for r = 0), r < nfirst.
// k_quantile_bounds finds the same from the batch's bytes; here the separator
// plane is at hand, an eighth of them.
__global__ __launch_bounds__(kIvalBlock) void k_interval_bounds(const ull *__restrict__ sep,
                                                                const ull *__restrict__ sep_pre,
                                                                uint32_t *__restrict__ first, uint64_t nfirst) {
    __shared__ ull wsum[kIvalBlock / 64];
    const uint64_t w = (uint64_t)blockIdx.x * kIvalBlock + threadIdx.x;
    ull e = sep[w], tot;
    ull rec = sep_pre[blockIdx.x] + block_excl_scan<kIvalBlock>((ull)__popcll(e), wsum, &tot) + 1;
    if (w == 0) first[0] = 0;  // nfirst >= 1
    for (; e; e &= e - 1, ++rec)
        if (rec < nfirst) first[rec] = (uint32_t)(w * 64 + (uint64_t)__ffsll((long long)e));  // < 2^32: see above
}

__global__ __launch_bounds__(kIvalBlock) void k_interval_emit(const ull *__restrict__ sel, const ull *__restrict__ sep,
                                                              uint64_t nwords, uint32_t d,
                                                              const ull *__restrict__ run_pre,
                                                              const ull *__restrict__ sep_pre,
                                                              const uint32_t *__restrict__ first, uint64_t nrec,
                                                              uint64_t rec0, ull *__restrict__ rows, uint64_t cap,
                                                              ull *__restrict__ total) {
    __shared__ ull wrun[kIvalBlock / 64], wsep[kIvalBlock / 64];
    const uint64_t w = (uint64_t)blockIdx.x * kIvalBlock + threadIdx.x;  // < nwords: whole tiles
    const uint64_t p0 = w * 64;
    const IvalWord b = interval_word(sel, w, nwords, d);
    const ull e = sep[w];
    ull tot;
    // the run starts before this word, and the record its first position lies in
    const ull before = run_pre[blockIdx.x] + block_excl_scan<kIvalBlock>((ull)__popcll(b.starts), wrun, &tot);
    const ull rec = sep_pre[blockIdx.x] + block_excl_scan<kIvalBlock>((ull)__popcll(e), wsep, &tot);

    // the total: the starts before separator nrec - 1, or all of them
    for (ull m = e; m; m &= m - 1) {
        const int i = __ffsll((long long)m) - 1;
        if (rec + (ull)__popcll(e & ival_below(i)) == nrec - 1) *total = before + (ull)__popcll(b.starts & ival_below(i));
    }
    if (w + 1 == nwords && rec + (ull)__popcll(e) < nrec) *total = before + (ull)__popcll(b.starts);

    // a run never holds a separator, so its record is the one of either end
    for (ull m = b.starts; m; m &= m - 1) {
        const int i = __ffsll((long long)m) - 1;
        const ull r = rec + (ull)__popcll(e & ival_below(i)), at = before + (ull)__popcll(b.starts & ival_below(i));
        if (r >= nrec || at >= cap) continue;
        rows[at * 3 + kIvalRecord] = rec0 + r;
        rows[at * 3 + kIvalStart] = p0 + i - first[r];
    }
    for (ull m = b.ends; m; m &= m - 1) {
        const int i = __ffsll((long long)m) - 1;
        const ull r = rec + (ull)__popcll(e & ival_below(i));
        // the starts at positions <= i, less one: a run that ends here started at or before i
        const ull at = before + (ull)__popcll(b.starts & (ival_below(i) | (1ull << i))) - 1;
        if (r >= nrec || at >= cap) continue;
        rows[at * 3 + kIvalEnd] = p0 + i + 1 - first[r];
    }
}

// The planes into the tiles' scans and first[]: everything the rows need but a place to go.
void launch_interval_index(void *stream, uint64_t n, uint64_t nrec, uint32_t k, bool slots,
                           const unsigned long long *planes, unsigned long long *tiles) {
    if (!n || !nrec) return;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t nt = solid_tiles(n), words = solid_plane_words(n);  // nt <= 2^18
    const ull *sel = planes, *sep = planes + words;
    ull *run = tiles, *sepc = run + nt + 1, *run_pre = sepc + nt + 1, *sep_pre = run_pre + nt + 1;
    ull *scr = sep_pre + nt + 1, *total = scr + scan_tmp_elems(nt + 1);
    uint32_t *first = reinterpret_cast<uint32_t *>(total + 1);
    const uint32_t d = slots ? 0u : k - 1;
    hipLaunchKernelGGL(k_interval_tiles, dim3((uint32_t)nt), dim3(kIvalBlock), 0, s, sel, sep, words, d, run, sepc);
    launch_exclusive_scan(stream, run, run_pre, nt + 1, scr);
    launch_exclusive_scan(stream, sepc, sep_pre, nt + 1, scr);
    hipLaunchKernelGGL(k_interval_bounds, dim3((uint32_t)nt), dim3(kIvalBlock), 0, s, sep, sep_pre, first,
                       interval_records(n, nrec));
}

// After launch_interval_index: rows[0 .. min(total, cap)) (device; null when
// cap == 0), records numbered from rec0; returns where the total lies (device).
const unsigned long long *launch_interval_rows(void *stream, uint64_t n, uint64_t nrec, uint32_t k, bool slots,
                                               const unsigned long long *planes, unsigned long long *tiles,
                                               uint64_t rec0, okm_count_interval *rows, uint64_t cap) {
    const uint64_t nt = solid_tiles(n), words = solid_plane_words(n);
    const ull *sel = planes, *sep = planes + words;
    ull *run_pre = tiles + 2 * (nt + 1), *sep_pre = run_pre + nt + 1;
    ull *total = sep_pre + nt + 1 + scan_tmp_elems(nt + 1);
    const uint32_t *first = reinterpret_cast<const uint32_t *>(total + 1);
    hipLaunchKernelGGL(k_interval_emit, dim3((uint32_t)nt), dim3(kIvalBlock), 0, (hipStream_t)stream, sel, sep, words,
                       slots ? 0u : k - 1, run_pre, sep_pre, first, nrec, rec0, reinterpret_cast<ull *>(rows), cap,
                       total);
    return total;
}

}  // namespace okm
