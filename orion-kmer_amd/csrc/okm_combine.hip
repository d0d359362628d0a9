// okm_combine.hip — two counted tables merged into a third (okm_combine_counts):
// union, the two intersections, difference and subtract, each a sorted
// (key, u64 count) table written once.
//
// It is the compare's merge (okm_compare.hip) with an output.  Both tables are
// read where they lie, through a TableView's run list; the larger one drives
// (D), cut into tiles of at most T consecutive entries of one run
// (k_cmp_tile_counts + a scan, as there), and one workgroup merges a tile with
// the part of the other table (S) that belongs to it, chunk by chunk through
// LDS, every thread taking an equal share of the merged sequence by a diagonal
// (merge-path) search.  What differs:
//
// Tile ranges without gaps.  The compare hands a tile the S entries inside its
// key span; an S entry between two tiles, below the first or above the last is
// nobody's.  Here it has to be emitted (a union, and every asymmetric
// operation whose left side is S), so k_comb_bounds gives tile t the S range
// (last key of tile t-1, last key of tile t]: the first tile begins at S's
// first entry and the last one ends behind S's last.  Only the range's end is
// searched; its beginning is the end stored for tile t-1.  Every S entry
// belongs to exactly one tile, and a key both tables hold meets its partner in
// the tile that holds D's copy.
//
// A tile's S range may be many chunks long, and D's entries are emitted too, so
// a chunk takes with it the D entries up to its last key (one binary search in
// LDS, the same in every thread); the last chunk takes the rest.  The output
// of a tile is then sorted chunk by chunk.
//
// Two passes and no workgroup ever waits for another.  Pass 1 (WRITE = false)
// performs the merge and writes one number per tile: the entries it emits.  A
// scan turns them into offsets, the host reads the total and allocates the
// output at its exact size, and pass 2 repeats the merge: in each chunk a
// thread keeps what it emits in registers (at most 2T / 256 entries), a
// workgroup-wide exclusive scan of the threads' numbers (wave shuffles, one LDS
// word per wave) gives it its place, and it stores its entries, a contiguous
// stretch, at tile offset + chunks so far + thread prefix.
//
// The functor CombOp<OP, SWAPPED> maps (has_d, count_d, has_s, count_s), after
// the thresholds, to "emit or not, with which count"; SWAPPED says that the
// left table a is S (the asymmetric operations, when b is the larger table).
//
// LDS per workgroup, as the compare's: the keys of both buffers and a saturated
// u32 per count (a saturated one from a u64 table is fetched from memory when
// used, by every entry, matched or not, and a chunk of S ends where the next
// run's counts do not follow on in memory):
//   u64 keys,  T = 1024: 2 x 8 KB + 2 x 4 KB = 24 KB: six workgroups per CU
//   K128 keys, T = 512:  2 x 8 KB + 2 x 2 KB = 20 KB: seven
// The output leaves the workgroup straight from the registers.  The other
// candidate, OKM_COMB_STAGE_OUT=1, compacts a chunk's entries into an LDS
// buffer (2T keys and u64 counts: 32 KB more, two workgroups per CU) and copies
// it out in full lines; profiles/AB_LOG.md has both times.
#include <hip/hip_runtime.h>

#include "okm_cmp_stage.h"
#include "okm_dev_common.h"
#include "okm_internal.h"
#include "okm_search.h"

namespace okm {

#ifndef OKM_COMB_TILE  // build flags, for the A/B in profiles/AB_LOG.md
#define OKM_COMB_TILE 1024
#endif
#ifndef OKM_COMB_STAGE_OUT
#define OKM_COMB_STAGE_OUT 0
#endif
template <typename KT> struct CombTileOf { static constexpr uint32_t T = OKM_COMB_TILE / (sizeof(KT) / 8); };
constexpr bool kCombStageOut = OKM_COMB_STAGE_OUT != 0;

uint32_t combine_tile(bool wide) { return wide ? CombTileOf<K128>::T : CombTileOf<ull>::T; }

// One thread per tile of D: its run and place in it, and where its S range
// ends: behind the last S entry <= the tile's last key, (0, 0) when there is
// none, behind S's last entry for the last tile.  sn_desc == nullptr: S is
// empty, every range ends at (0, 0) and no descriptor of S is read.
template <typename KT>
__global__ __launch_bounds__(256) void k_comb_bounds(const LookItem *__restrict__ ddesc,
                                                     const ull *__restrict__ dn_desc, const ull *__restrict__ toff,
                                                     uint32_t max_runs, const KT *__restrict__ sfirst,
                                                     const LookItem *__restrict__ sdesc,
                                                     const ull *__restrict__ sn_desc, uint32_t T,
                                                     CombTile *__restrict__ tiles) {
    typedef KeyOps<KT> O;
    const ull t = (ull)blockIdx.x * 256 + threadIdx.x, nt = toff[max_runs];
    if (t >= nt) return;
    // the last toff[r] <= t is t's run (every run has a tile: k_cmp_bounds)
    const FlatKeys<ull> ta[1] = {{toff}};
    const ull tn[1] = {*dn_desc}, tq[1] = {t};
    ull tp[1], tl[1];
    search_last_le<ull, 1>(ta, tn, tq, tp, tl);
    const LookItem *d = ddesc + tp[0];
    const KT *kp = reinterpret_cast<const KT *>(gload(&d->keys));
    const ull dn = gload(&d->n), d_off = (t - tl[0]) * T;
    const uint32_t d_len = (uint32_t)(dn - d_off < T ? dn - d_off : T);
    const ull ms = sn_desc ? *sn_desc : 0;
    ull r1 = 0, o1 = 0;
    if (ms && t + 1 == nt) {
        r1 = ms - 1;
        o1 = gload(&sdesc[r1].n);
    } else if (ms) {
        const KT q[1] = {gload(kp + d_off + d_len - 1)};
        FlatKeys<KT> a[1] = {{sfirst}};
        ull len[1] = {ms}, pos[1];
        KT last[1];
        search_last_le<KT, 1>(a, len, q, pos, last);
        if (!O::lt(q[0], last[0])) {  // else: the whole of S lies above this tile
            r1 = pos[0];
            a[0].p = reinterpret_cast<const KT *>(gload(&sdesc[r1].keys));
            len[0] = gload(&sdesc[r1].n);
            search_last_le<KT, 1>(a, len, q, pos, last);  // (the run's first key is <= q: there is one)
            o1 = pos[0] + 1;
        }
    }
    CombTile w;
    w.d_run = (uint32_t)tp[0];
    w.d_len = d_len;
    w.d_off = d_off;
    w.s_run1 = (uint32_t)r1;
    w.s_off1 = o1;
    tiles[t] = w;
}

// What one key's two sides become.  h*: the side holds the key with a count
// that passes its threshold (else its count is 0).  a is D unless SWAPPED.
template <int OP, bool SWAPPED>
struct CombOp {
    __device__ static __forceinline__ bool apply(bool hd, ull cd, bool hs, ull cs, ull *out) {
        const bool ha = SWAPPED ? hs : hd, hb = SWAPPED ? hd : hs;
        const ull ca = SWAPPED ? cs : cd, cb = SWAPPED ? cd : cs;
        switch (OP) {
        case OKM_COMBINE_UNION: {
            const ull s = (ha ? ca : 0) + (hb ? cb : 0);
            *out = ha && hb && s < ca ? ~0ull : s;
            return ha || hb;
        }
        case OKM_COMBINE_INTERSECT_MIN:
            *out = ca < cb ? ca : cb;
            return ha && hb;
        case OKM_COMBINE_INTERSECT_A:
            *out = ca;
            return ha && hb;
        case OKM_COMBINE_DIFFERENCE:
            *out = ca;
            return ha && !hb;
        default:  // OKM_COMBINE_SUBTRACT
            *out = hb ? ca - cb : ca;
            return ha && (!hb || ca > cb);
        }
    }
};

// One workgroup per tile of D; workgroups past the last tile (the grid is the
// host's bound) leave at once.  WRITE = false: tile_n[tile] = the entries the
// tile emits.  WRITE = true: tile_n[tile] is where its entries go in okeys /
// ocounts.
template <typename KT, bool NARROW_D, bool NARROW_S, int OP, bool SWAPPED, bool WRITE>
__global__ __launch_bounds__(kCmpBlock) void k_combine_tiles(const CombTile *__restrict__ tiles,
                                                             const ull *__restrict__ n_tiles,
                                                             const LookItem *__restrict__ ddesc,
                                                             const uint64_t *__restrict__ dcounts,
                                                             const LookItem *__restrict__ sdesc,
                                                             const uint64_t *__restrict__ scounts, ull min_d,
                                                             ull min_s, ull *__restrict__ tile_n,
                                                             KT *__restrict__ okeys, ull *__restrict__ ocounts) {
    typedef KeyOps<KT> O;
    constexpr uint32_t T = CombTileOf<KT>::T, PER = 2 * T / kCmpBlock;
    constexpr bool STAGE = WRITE && kCombStageOut;
    static_assert(PER >= 1 && PER <= 32, "a thread's share of a chunk is kept in registers, one mask bit each");
    __shared__ KT dk[T], sk[T];
    __shared__ uint32_t dc[T], sc[T];
    __shared__ ull wsum[kCmpBlock / 64];
    __shared__ KT ok[STAGE ? 2 * T : 1];
    __shared__ ull oc[STAGE ? 2 * T : 1];
    if (blockIdx.x >= *n_tiles) return;
    const CombTile t = tiles[blockIdx.x];
    uint32_t run = 0;  // the S range begins where the tile before ends
    ull off = 0;
    if (blockIdx.x) {
        run = tiles[blockIdx.x - 1].s_run1;
        off = tiles[blockIdx.x - 1].s_off1;
    }
    const uint32_t dl = t.d_len;
    cmp_stage<KT, NARROW_D>(ddesc + t.d_run, t.d_off, dl, dcounts, dk, dc);
    const ull dc0 = gload(&ddesc[t.d_run].coff) + t.d_off;  // where the tile's counts lie
    uint32_t d0 = 0;                                        // D entries that earlier chunks took
    ull base = WRITE ? tile_n[blockIdx.x] : 0, mine = 0;
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
        // a range with entries left never ends a round on an empty chunk: !last implies sl > 0
        const bool last = run > t.s_run1 || (run == t.s_run1 && off >= t.s_off1);
        __syncthreads();
        uint32_t d1 = dl;  // this chunk takes D's entries [d0, d1): up to its last key, the last chunk all
        if (!last) {
            const KT e = sk[sl - 1];
            uint32_t lo = d0;
            while (lo < d1) {
                const uint32_t mid = (lo + d1) >> 1;
                if (!O::lt(e, dk[mid]))
                    lo = mid + 1;
                else
                    d1 = mid;
            }
        }
        const KT *dkp = dk + d0;
        const uint32_t *dcp = dc + d0;
        const uint32_t dn = d1 - d0;
        // this thread's share of the merged sequence (ties: D's entry first): steps [diag, dend)
        const uint32_t total = dn + sl, per = (total + kCmpBlock - 1) / kCmpBlock;
        const uint32_t diag = min(threadIdx.x * per, total), dend = min(diag + per, total);
        uint32_t lo = diag > sl ? diag - sl : 0u, hi = min(diag, dn);
        while (lo < hi) {  // i = D entries among the first diag merged ones
            const uint32_t mid = (lo + hi) >> 1;
            if (!O::lt(sk[diag - 1 - mid], dkp[mid]))
                lo = mid + 1;
            else
                hi = mid;
        }
        uint32_t i = lo, j = diag - lo, ne = 0, mask = 0;
        KT kd = i < dn ? dkp[i] : O::empty(), ks = j < sl ? sk[j] : O::empty();
        KT ek[PER];
        ull ec[PER];
#pragma unroll
        for (uint32_t e = 0; e < PER; ++e) {
            if (diag + e >= dend) continue;
            const bool has_d = i < dn, has_s = j < sl;
            KT key;
            ull cd = 0, cs = 0;  // 0: the side does not hold the key (no threshold lets 0 pass)
            if (has_d && (!has_s || !O::lt(ks, kd))) {
                key = kd;
                cd = dcp[i];
                if (!NARROW_D && cd == kCmpSat) cd = dcounts[dc0 + d0 + i];
                if (has_s && O::eq(kd, ks)) {  // S's equal key is still ahead of j: the pair is emitted here
                    cs = sc[j];
                    if (!NARROW_S && cs == kCmpSat) cs = scounts[sc0 + j];
                }
                ++i;
                if (i < dn) kd = dkp[i];
            } else {
                key = ks;
                if (!(i > 0 && O::eq(dkp[i - 1], ks))) {  // else D's copy, just before it, has emitted the pair
                    cs = sc[j];
                    if (!NARROW_S && cs == kCmpSat) cs = scounts[sc0 + j];
                }
                ++j;
                if (j < sl) ks = sk[j];
            }
            ull c;
            if (CombOp<OP, SWAPPED>::apply(cd >= min_d, cd, cs >= min_s, cs, &c)) {
                ++ne;
                if (WRITE) {
                    mask |= 1u << e;
                    ek[e] = key;
                    ec[e] = c;
                }
            }
        }
        if (WRITE) {
            ull tot;  // wsum: the round's closing barrier stands between these reads and the next round's writes
            ull o = block_excl_scan_1b<kCmpBlock>(ne, wsum, &tot);
            if (!STAGE) o += base;
#pragma unroll
            for (uint32_t e = 0; e < PER; ++e)
                if (mask >> e & 1u) {
                    if (STAGE) {
                        ok[o] = ek[e];
                        oc[o] = ec[e];
                    } else {
                        okeys[o] = ek[e];
                        ocounts[o] = ec[e];
                    }
                    ++o;
                }
            if (STAGE) {
                __syncthreads();
                for (uint32_t x = threadIdx.x; x < (uint32_t)tot; x += kCmpBlock) {
                    okeys[base + x] = ok[x];
                    ocounts[base + x] = oc[x];
                }
            }
            base += tot;
        } else {
            mine += ne;
        }
        if (last) break;
        d0 = d1;
        __syncthreads();  // the next chunk overwrites sk / sc (and ok / oc)
    }
    if (!WRITE) {
        ull tot;
        block_excl_scan_1b<kCmpBlock>(mine, wsum, &tot);
        if (threadIdx.x == 0) tile_n[blockIdx.x] = tot;
    }
}

namespace {
struct CombArgs {
    hipStream_t s;
    const TableView *d, *sv;
    uint64_t min_d, min_s, max_tiles;
    const CombTile *tiles;
    const unsigned long long *n_tiles;
    unsigned long long *tile_n;
    uint64_t *okeys, *ocounts;  // null: pass 1
};

template <typename KT, bool ND, bool NS, int OP, bool SW>
void combine_pass(const CombArgs &a) {
    const dim3 g((uint32_t)a.max_tiles), b(kCmpBlock);
    unsigned long long *oc = reinterpret_cast<unsigned long long *>(a.ocounts);
    if (a.okeys)
        hipLaunchKernelGGL((k_combine_tiles<KT, ND, NS, OP, SW, true>), g, b, 0, a.s, a.tiles, a.n_tiles, a.d->desc,
                           a.d->counts, a.sv->desc, a.sv->counts, a.min_d, a.min_s, a.tile_n,
                           reinterpret_cast<KT *>(a.okeys), oc);
    else
        hipLaunchKernelGGL((k_combine_tiles<KT, ND, NS, OP, SW, false>), g, b, 0, a.s, a.tiles, a.n_tiles, a.d->desc,
                           a.d->counts, a.sv->desc, a.sv->counts, a.min_d, a.min_s, a.tile_n,
                           reinterpret_cast<KT *>(a.okeys), oc);
}

template <typename KT, bool ND, bool NS>
void combine_op(const CombArgs &a, int op, bool swapped) {
    switch (op) {  // (the symmetric two have one form)
    case OKM_COMBINE_UNION: return combine_pass<KT, ND, NS, OKM_COMBINE_UNION, false>(a);
    case OKM_COMBINE_INTERSECT_MIN: return combine_pass<KT, ND, NS, OKM_COMBINE_INTERSECT_MIN, false>(a);
#define OKM_COMB_CASE(OP) \
    case OP: return swapped ? combine_pass<KT, ND, NS, OP, true>(a) : combine_pass<KT, ND, NS, OP, false>(a);
        OKM_COMB_CASE(OKM_COMBINE_INTERSECT_A)
        OKM_COMB_CASE(OKM_COMBINE_DIFFERENCE)
        OKM_COMB_CASE(OKM_COMBINE_SUBTRACT)
#undef OKM_COMB_CASE
    }
}

template <typename KT>
void combine_widths(const CombArgs &a, int op, bool swapped) {
    if (a.d->narrow && a.sv->narrow)
        combine_op<KT, true, true>(a, op, swapped);
    else if (a.d->narrow)
        combine_op<KT, true, false>(a, op, swapped);
    else if (a.sv->narrow)
        combine_op<KT, false, true>(a, op, swapped);
    else
        combine_op<KT, false, false>(a, op, swapped);
}
}  // namespace

void launch_combine_count(void *stream, const TableView &d, const TableView &sv, bool wide, int op, bool swapped,
                          uint64_t min_d, uint64_t min_s, unsigned long long *toff, unsigned long long *scan_tmp,
                          CombTile *tiles, unsigned long long *tile_n, unsigned long long *tile_scan_tmp) {
    hipStream_t s = (hipStream_t)stream;
    const uint32_t T = combine_tile(wide);
    const uint64_t max_tiles = compare_max_tiles(d.n, d.max_runs, T);
    launch_compare_tile_offsets(stream, d, T, toff, scan_tmp);
    const dim3 g((uint32_t)(max_tiles / 256 + 1)), b(256);
    if (wide)
        hipLaunchKernelGGL(k_comb_bounds<K128>, g, b, 0, s, d.desc, d.n_desc, toff, d.max_runs,
                           reinterpret_cast<const K128 *>(sv.first), sv.desc, sv.n_desc, T, tiles);
    else
        hipLaunchKernelGGL(k_comb_bounds<ull>, g, b, 0, s, d.desc, d.n_desc, toff, d.max_runs,
                           reinterpret_cast<const ull *>(sv.first), sv.desc, sv.n_desc, T, tiles);
    const CombArgs a{s, &d, &sv, min_d, min_s, max_tiles, tiles, toff + d.max_runs, tile_n, nullptr, nullptr};
    if (wide)
        combine_widths<K128>(a, op, swapped);
    else
        combine_widths<ull>(a, op, swapped);
    launch_exclusive_scan(stream, tile_n, tile_n, max_tiles + 1, tile_scan_tmp);
}

void launch_combine_write(void *stream, const TableView &d, const TableView &sv, bool wide, int op, bool swapped,
                          uint64_t min_d, uint64_t min_s, const unsigned long long *toff, const CombTile *tiles,
                          unsigned long long *tile_off, uint64_t *okeys, uint64_t *ocounts) {
    const uint64_t max_tiles = compare_max_tiles(d.n, d.max_runs, combine_tile(wide));
    const CombArgs a{(hipStream_t)stream, &d, &sv, min_d, min_s, max_tiles, tiles, toff + d.max_runs, tile_off, okeys,
                     ocounts};
    if (wide)
        combine_widths<K128>(a, op, swapped);
    else
        combine_widths<ull>(a, op, swapped);
}

}  // namespace okm
