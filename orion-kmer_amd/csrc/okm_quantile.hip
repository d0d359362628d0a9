// okm_quantile.hip — per-record count quantiles of a batch of reads against a
// counted table (okm_read_count_quantiles): for every record the number of its
// valid windows and, for up to OKM_MAX_QUANTILES fractions num / den, the
// element at index min(floor(windows * num / den), windows - 1) of its windows'
// counts sorted ascending (an absent k-mer counts 0), every count clipped to
// OKM_QUANTILE_COUNT_MAX first.  The median of a read is 1 / 2.
//
// Stage 1, k_quantile_counts: the search.  The read-batch scan of
// okm_read_scan.h (256 threads, 16 window starts each), one search in flight
// through FindDense / FindItems, but a thread writes 16 consecutive uint32_t of
// a COUNT PLANE, one word per batch byte: kQuantNone (2^32 - 1) where the slot
// has no valid window, else the window's clipped count, 0 when absent.  The
// first launch of a batch stores its every word (whole tiles, positions at or
// past n included), so nothing is zeroed beforehand; every further slice of a
// host-resident table stores its hits only: the slices' keys are disjoint and
// a thread owns its words, so these are plain stores, no atomics.
//
// kQuantNone sorts above every count, so a record's positions [start, end) are
// ranked as they lie: every window with an N falls off the top while rank <
// windows (and so would the last k - 1 positions, which no window starts at:
// stage 2 leaves them out).  Stage 2 reads the plane only:
//   k_quantile_init    ends[r] = n (an unterminated last record, a missing
//                      one), the long-record counter = 0
//   k_depth_sep_count + scan: the separators before every tile (okm_depth.hip)
//   k_quantile_bounds  ends[r] = the position of separator r; record r is
//                      [ends[r - 1] + 1, ends[r])
//   k_quantile_wave    one wave per record of at most kQuantWave slots, in
//                      registers; a longer record goes onto a list (the wave
//                      that owns a record is the first place that knows its
//                      two ends, which may lie in different tiles)
//   k_quantile_block   a fixed grid of workgroups strides over that list, the
//                      counter read on the device: a record of at most
//                      kQuantLds slots is staged in LDS once, a longer one
//                      streams from the plane on every pass
// Both selections are exact radix selects from the most significant end and
// skip what the OR of the record's counts shows to be zero: typical coverage
// counts take one 8-bit digit pass, or about 8 one-bit steps, not 32 bits.
// Positions are 32 bits: a batch holds < 2^32 bytes.
#include <hip/hip_runtime.h>

#include "okm_dev_common.h"
#include "okm_internal.h"
#include "okm_read_scan.h"
#include "okm_scan.h"
#include "okm_search.h"

namespace okm {

constexpr uint32_t kQuantNone = 0xFFFFFFFFu;  // the plane's word of a slot without a valid window
static_assert(OKM_QUANTILE_COUNT_MAX == kQuantNone - 1, "the largest count sorts right below the sentinel");
constexpr int kQuantWave = 512;                // slots of the longest record one wave selects from
constexpr int kQuantRegs = kQuantWave / 64;    // ... in this many registers a lane
constexpr int kQuantBlock = 256;
constexpr int kQuantLds = 8192;                // slots of the longest record staged in LDS (32 KB)
constexpr int kQuantGrid = 1024;               // workgroups that share the long records
constexpr int kQuantWaves = kQuantBlock / 64;

uint64_t quant_tiles(uint64_t n_bytes) { return (n_bytes + kScanTile - 1) / kScanTile; }
uint64_t quant_plane_words(uint64_t n_bytes) { return quant_tiles(n_bytes) * (kScanTile / 2); }
uint64_t quant_tile_words(uint64_t n_bytes, uint64_t nrec) {
    const uint64_t nt = quant_tiles(n_bytes);
    return 2 * nt + scan_tmp_elems(nt) + 1 + nrec;  // tile counts, their scan, its scratch, the counter, ends + list
}

// ---------------------------------------------------------------------------
// Stage 1
// ---------------------------------------------------------------------------

// FIRST: the batch's first launch: stores the thread's 16 words whatever they
// are; otherwise stores this table's hits.
template <typename KT, typename TAB, bool FIRST>
__global__ __launch_bounds__(kScanBlock) void k_quantile_counts(const uint8_t *__restrict__ seq, uint64_t n, TAB tab,
                                                                uint32_t k, uint32_t *__restrict__ plane) {
    typedef KeyOps<KT> O;
    typedef ScanKeys<KT> SK;
    const uint64_t t = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
    const uint64_t w0 = t * kScanSeg;  // the thread's first window start, and its first word of the plane
    typename SK::Words ww;
    load_windows<kScanSeg, SK::kHalo>(seq, n, w0, ww);  // bytes at or past n read as 0: no base, no separator
    typename SK::Coded c;
    make_codes<SK::kNP, false>(ww.w, c);  // count's validity: either case, U reads as T
    const uint32_t vmask = SK::valid_mask(c, k);
    tab.begin();
#pragma unroll
    for (int g = 0; g < kScanSeg / 4; ++g) {  // four words a 16-byte store
        uint32_t v[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const int j = 4 * g + f;
            KT q[1];
            bool live[1], hit[1];
            ull cnt[1];
            live[0] = (vmask >> j) & 1u;
            q[0] = live[0] ? SK::key(c, j, k) : O::empty();
            tab.find(q, live, cnt, hit);
            const uint32_t clipped = cnt[0] > OKM_QUANTILE_COUNT_MAX ? (uint32_t)OKM_QUANTILE_COUNT_MAX : (uint32_t)cnt[0];
            if (FIRST)
                v[f] = live[0] ? (hit[0] ? clipped : 0u) : kQuantNone;
            else if (hit[0])
                plane[w0 + j] = clipped;
        }
        if (FIRST) *reinterpret_cast<uint4 *>(plane + w0 + 4 * g) = make_uint4(v[0], v[1], v[2], v[3]);
    }
}

void launch_quantile_counts(void *stream, const uint8_t *seq, uint64_t n, uint32_t k, bool wide, const TableView &t,
                            bool first, unsigned long long *plane) {
    if (!n) return;
    // every launch covers whole tiles: the plane has a word for each of their positions
    const uint32_t nblocks = (uint32_t)quant_tiles(n);  // n < 2^32
    uint32_t *p = reinterpret_cast<uint32_t *>(plane);
    with_finder<1>(t, wide, [&](const auto &tab) {
        typedef std::decay_t<decltype(tab)> TAB;
        typedef typename TAB::Key KT;
        if (first)
            hipLaunchKernelGGL((k_quantile_counts<KT, TAB, true>), dim3(nblocks), dim3(kScanBlock), 0,
                               (hipStream_t)stream, seq, n, tab, k, p);
        else
            hipLaunchKernelGGL((k_quantile_counts<KT, TAB, false>), dim3(nblocks), dim3(kScanBlock), 0,
                               (hipStream_t)stream, seq, n, tab, k, p);
    });
}

// ---------------------------------------------------------------------------
// Stage 2
// ---------------------------------------------------------------------------

struct QuantSpec {
    uint32_t nq;
    uint32_t num[OKM_MAX_QUANTILES], den[OKM_MAX_QUANTILES];
};

__device__ __forceinline__ uint32_t quant_rank(ull windows, uint32_t num, uint32_t den) {  // windows > 0
    const ull i = windows * num / den;  // windows < 2^32, num <= den
    return (uint32_t)(i < windows ? i : windows - 1);
}

// Record r's first position and its slots: the positions a window of the
// record can start at, bytes - k + 1 (0: shorter than k, or no such record).
// The k - 1 positions behind them hold kQuantNone and are never read.
__device__ __forceinline__ void quant_record(const uint32_t *__restrict__ ends, ull r, uint32_t k, ull *start,
                                             ull *len) {
    const ull s = r ? (ull)ends[r - 1] + 1 : 0, e = ends[r];
    *start = s;
    *len = e >= s + k ? e - s - k + 1 : 0;
}

__global__ __launch_bounds__(256) void k_quantile_init(uint32_t *__restrict__ ends, uint64_t nrec, uint64_t n,
                                                       ull *__restrict__ n_long) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r == 0) *n_long = 0;
    if (r < nrec) ends[r] = (uint32_t)n;  // until a separator says otherwise
}

// ends[r] = the position of the batch's separator r, from the separators
// before the tile (tile_pre) and a block scan, the way k_read_depths finds rec.
__global__ __launch_bounds__(kScanBlock) void k_quantile_bounds(const uint8_t *__restrict__ seq, uint64_t n,
                                                                const ull *__restrict__ tile_pre,
                                                                uint32_t *__restrict__ ends, uint64_t nrec) {
    __shared__ ull wsum[kScanBlock / 64];
    const uint64_t w0 = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanSeg;
    uint32_t w[kScanSeg / 4] = {0, 0, 0, 0};
    if (w0 + kScanSeg <= n) {
        const uint4 v = *reinterpret_cast<const uint4 *>(seq + w0);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else {
#pragma unroll
        for (int i = 0; i < kScanSeg; ++i)
            if (w0 + i < n) w[i >> 2] |= (uint32_t)seq[w0 + i] << ((i & 3) * 8);
    }
    uint32_t m = sep_mask_words(w);
    ull tot;
    ull rec = tile_pre[blockIdx.x] + block_excl_scan<kScanBlock>((ull)__popc(m), wsum, &tot);
    for (; m; m &= m - 1, ++rec)
        if (rec < nrec) ends[rec] = (uint32_t)(w0 + (uint32_t)(__ffs((int)m) - 1));
}

// One wave per record of at most kQuantWave positions.  Lane l holds positions
// l, l + 64, ... in kQuantRegs registers; `cand` has bit i set while register i
// is still a candidate.  The select walks the bits from the highest one set in
// any valid value down to 0: c0 = candidates with the bit clear (a ballot and a
// popcount per register: the same number in every lane, no shuffle); rank < c0
// keeps them, else rank -= c0 and the ones stay.
__global__ __launch_bounds__(kQuantBlock) void k_quantile_wave(const uint32_t *__restrict__ plane,
                                                               const uint32_t *__restrict__ ends, uint64_t nrec,
                                                               uint32_t k, QuantSpec qs, ull *__restrict__ rows,
                                                               uint32_t *__restrict__ list, ull *__restrict__ n_long) {
    const uint32_t lane = threadIdx.x & 63u;
    const ull r = (ull)blockIdx.x * kQuantWaves + (threadIdx.x >> 6);
    if (r >= nrec) return;  // (the whole wave; this kernel has no barrier)
    ull start, len;
    quant_record(ends, r, k, &start, &len);
    if (len > kQuantWave) {  // k_quantile_block's: r < 2^32, it has a separator or ends the batch
        if (lane == 0) list[atomicAdd(n_long, 1ull)] = (uint32_t)r;
        return;
    }
    uint32_t v[kQuantRegs], valid = 0, orv = 0, windows = 0;
#pragma unroll
    for (int i = 0; i < kQuantRegs; ++i) {
        const uint32_t p = lane + 64u * i;
        v[i] = p < len ? plane[start + p] : kQuantNone;
        const bool ok = v[i] != kQuantNone;
        windows += (uint32_t)__popcll(__ballot(ok));
        if (ok) {
            valid |= 1u << i;
            orv |= v[i];
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) orv |= __shfl_xor(orv, d, 64);
    ull *row = rows + r * (1 + qs.nq);
    if (lane == 0) row[0] = windows;
#pragma unroll
    for (int qi = 0; qi < OKM_MAX_QUANTILES; ++qi) {
        if (qi >= (int)qs.nq) break;
        uint32_t val = 0;
        if (windows && orv) {
            uint32_t rank = quant_rank(windows, qs.num[qi], qs.den[qi]), cand = valid;
            for (int b = 31 - __clz((int)orv); b >= 0; --b) {
                uint32_t c0 = 0;
#pragma unroll
                for (int i = 0; i < kQuantRegs; ++i)
                    c0 += (uint32_t)__popcll(__ballot(((cand >> i) & 1u) && !((v[i] >> b) & 1u)));
                const uint32_t keep = rank < c0 ? 0u : 1u;  // the bit's value among the candidates that stay
                if (keep) {
                    rank -= c0;
                    val |= 1u << b;
                }
#pragma unroll
                for (int i = 0; i < kQuantRegs; ++i)
                    if (((v[i] >> b) & 1u) != keep) cand &= ~(1u << i);
            }
        }
        if (lane == 0) row[1 + qi] = val;
    }
}

// The long records: workgroup g takes list entries g, g + gridDim.x, ...  Per
// record: pass 0 counts the windows and ORs the valid values; then per
// quantile a radix select on 8-bit digits from the top, skipping the bytes
// that are zero in the OR.  A digit pass histograms the candidates (the valid
// values whose higher bytes equal the prefix so far) into wave-private LDS
// histograms -- real counts pile into one or two bins, which four histograms
// spread over four atomic units -- then wave 0 adds the four, scans the 256
// bins four a lane, finds the bin in which the running total first exceeds the
// rank and hands the bin and the rank inside it to everybody through LDS.
__global__ __launch_bounds__(kQuantBlock) void k_quantile_block(const uint32_t *__restrict__ plane,
                                                                const uint32_t *__restrict__ ends, uint32_t k,
                                                                QuantSpec qs,
                                                                ull *__restrict__ rows,
                                                                const uint32_t *__restrict__ list,
                                                                const ull *__restrict__ n_long) {
    __shared__ uint32_t stage[kQuantLds];
    __shared__ uint32_t hist[kQuantWaves][256];
    __shared__ uint32_t red_n[kQuantWaves], red_or[kQuantWaves], pick[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const ull nl = *n_long;
    for (ull li = blockIdx.x; li < nl; li += gridDim.x) {
        const ull r = list[li];
        ull start, len;
        quant_record(ends, r, k, &start, &len);
        const uint32_t *src = plane + start;
        const bool staged = len <= kQuantLds;
        if (staged) {
            for (ull p = tid; p < len; p += kQuantBlock) stage[p] = src[p];
            lds_sync();
        }
        const auto at = [&](ull p) { return staged ? stage[p] : src[p]; };

        uint32_t cnt = 0, orv = 0;
        for (ull p = tid; p < len; p += kQuantBlock) {
            const uint32_t v = at(p);
            if (v != kQuantNone) {
                ++cnt;
                orv |= v;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            cnt += __shfl_xor(cnt, d, 64);
            orv |= __shfl_xor(orv, d, 64);
        }
        if (lane == 0) {
            red_n[wid] = cnt;
            red_or[wid] = orv;
        }
        lds_sync();
        ull windows = 0;
        orv = 0;
#pragma unroll
        for (int w = 0; w < kQuantWaves; ++w) {
            windows += red_n[w];
            orv |= red_or[w];
        }
        ull *row = rows + r * (1 + qs.nq);
        if (tid == 0) row[0] = windows;

        for (uint32_t qi = 0; qi < qs.nq; ++qi) {
            uint32_t prefix = 0, himask = 0;
            uint32_t rank = windows ? quant_rank(windows, qs.num[qi], qs.den[qi]) : 0;
            for (int sh = 24; windows && sh >= 0; sh -= 8) {
                if (((orv >> sh) & 0xFFu) == 0) continue;  // every valid value's byte here is 0, the prefix's too
#pragma unroll
                for (int w = 0; w < kQuantWaves; ++w) hist[w][tid] = 0;
                lds_sync();
                for (ull p = tid; p < len; p += kQuantBlock) {
                    const uint32_t v = at(p);
                    if (v != kQuantNone && (v & himask) == prefix) atomicAdd(&hist[wid][(v >> sh) & 0xFFu], 1u);
                }
                lds_sync();
                if (wid == 0) {
                    uint32_t h[4], s = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        h[j] = 0;
#pragma unroll
                        for (int w = 0; w < kQuantWaves; ++w) h[j] += hist[w][4 * lane + j];
                        s += h[j];
                    }
                    uint32_t below = wave_incl_scan32(s) - s;  // candidates in the bins before this lane's four
                    if (below <= rank && rank - below < s) {  // one lane: rank < the candidates
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            if (rank - below < h[j]) {
                                pick[0] = 4 * lane + j;
                                pick[1] = rank - below;
                                break;
                            }
                            below += h[j];
                        }
                    }
                }
                lds_sync();
                prefix |= pick[0] << sh;
                himask |= 0xFFu << sh;
                rank = pick[1];
            }
            if (tid == 0) row[1 + qi] = prefix;
        }
        lds_sync();  // stage, red_* and pick are the next record's from here
    }
}

void launch_quantile_select(void *stream, const uint8_t *seq, uint64_t n, uint64_t nrec, uint32_t k,
                            const okm_quantile *q, uint32_t nq, const unsigned long long *plane,
                            unsigned long long *tiles, uint64_t *rows) {
    if (!n || !nrec) return;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t nt = quant_tiles(n);  // <= 2^20
    ull *cnt = tiles, *pre = cnt + nt, *scr = pre + nt, *n_long = scr + scan_tmp_elems(nt);
    uint32_t *ends = reinterpret_cast<uint32_t *>(n_long + 1), *list = ends + nrec;
    const uint32_t *p = reinterpret_cast<const uint32_t *>(plane);
    QuantSpec qs = {nq, {0, 0, 0, 0}, {1, 1, 1, 1}};
    for (uint32_t i = 0; i < nq; ++i) qs.num[i] = q[i].num, qs.den[i] = q[i].den;
    hipLaunchKernelGGL(k_quantile_init, dim3((uint32_t)((nrec + 255) / 256)), dim3(256), 0, s, ends, nrec, n, n_long);
    launch_depth_sep_count(stream, seq, n, cnt);
    launch_exclusive_scan(stream, cnt, pre, nt, scr);
    hipLaunchKernelGGL(k_quantile_bounds, dim3((uint32_t)nt), dim3(kScanBlock), 0, s, seq, n, pre, ends, nrec);
    hipLaunchKernelGGL(k_quantile_wave, dim3((uint32_t)((nrec + kQuantWaves - 1) / kQuantWaves)), dim3(kQuantBlock), 0,
                       s, p, ends, nrec, k, qs, reinterpret_cast<ull *>(rows), list, n_long);
    hipLaunchKernelGGL(k_quantile_block, dim3(kQuantGrid), dim3(kQuantBlock), 0, s, p, ends, k, qs,
                       reinterpret_cast<ull *>(rows), list, n_long);
}

}  // namespace okm
