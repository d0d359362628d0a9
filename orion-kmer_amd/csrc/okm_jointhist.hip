// okm_jointhist.hip — the joint count spectrum of two counted tables, read
// where they lie (okm_compare_histogram): M[ca][cb] = the number of distinct
// keys with count ca in table a and cb in table b (KAT comp, Merqury's
// spectra-cn), both clamped to their side's last bin.
//
// Only the shared part needs the merge: the cells with ca >= 1 and cb >= 1,
// the keys that both tables keep.  Column 0 and row 0 are each side's kept
// count histogram (okm_hist.hip's walks, with the side's threshold) minus the
// shared cells of the row / column; k_joint_finish does the two subtractions.
// So nothing that only one table holds is attributed in the merge, and two
// host-resident tables' slice pairs simply add.
//
// k_joint_tiles is okm_compare.hip's merge (the same tiles and bounds, the
// same staging, the same merge-path split) with a binning epilogue.
//
// Clamped counts.  A bin needs min(count, bins - 1) with bins <= 65536, so the
// saturated u32 that LDS keeps of a u64 count always lands in the last bin:
// the count itself is never fetched again, and a chunk of S is therefore free
// to run over S runs whose counts do not follow on in memory (k_compare_tiles
// needs both).  The thresholds are applied while staging (cmp_stage_kept: on
// the full count; an entry below its side's threshold is staged as 0), so
// every threshold is exact, those past 2^32 - 1 included.
//
// Binning.  The two hazards the histogram and the compare measured:
//   * thousands of workgroups that each end on the same few global lines
//     queue at the memory side.  Hence persistent workgroups: the grid is
//     kJointPerCU workgroups per CU, each walks tiles blockIdx.x, += gridDim.x
//     and keeps ONE LDS matrix over all of them, flushed once at the end, one
//     global atomic per non-zero bin.
//   * a spectrum is concentrated (a == b: the diagonal's first bins; two read
//     sets of one genome: a blob around the two coverages), and the lanes of a
//     wave that hit one LDS address queue.  Measured, that queue does not
//     matter beside the merge's dependent loads: a match is a plain per-lane
//     LDS atomic.  Joining the lanes with equal bins by ballot first, so that
//     one lane adds their number (OKM_JOINT_BALLOT, a build flag kept for the
//     A/B), took 5.92 ms against 2.80 on two pending C2 tables and 3.41
//     against 2.52 on a == b, where every match of a wave hits one bin: the
//     blob spreads a wave's matches over many bins and every distinct bin
//     costs a round of ballots (profiles/AB_LOG.md).
// The LDS matrix is the low corner ca < Ra, cb < Rb in u32 (joint_corner: at
// most kJointCorner bins, 8 KB; a narrow side gives the wide one the rows).
// With the merge's 24 / 20 KB of staging that is 32 / 28 KB per workgroup:
// five per CU of gfx950's 160 KB, one fewer than the compare's six.  Pairs
// outside the corner are the rare high counts and go to the global matrix
// directly.  The counts are clamped BEFORE the path is chosen.
//
// Bounds.  An LDS bin is u32 and holds what one workgroup matched: at most
// the driving table's entries / grid, below 2^32 for any table that fits the
// machine (a host-resident table comes in slices of 2^26).  Matrix indices are
// below bins_a * bins_b because both counts are clamped first; LDS indices are
// below Ra * Rb because the corner test precedes them.
//
// Known limit: a spectrum whose mass lies past the corner (coverage above ~40
// on both sides with two wide matrices) bins through global atomics.
#include <hip/hip_runtime.h>

#include "okm_cmp_stage.h"
#include "okm_dev_common.h"
#include "okm_internal.h"

namespace okm {

constexpr uint32_t kJointCorner = 2048;  // u32 bins a workgroup keeps in LDS
constexpr uint32_t kJointSide = 45;      // the square corner: 45 x 45 <= kJointCorner
constexpr uint32_t kJointPerCU = 5;      // resident workgroups per CU that the LDS footprint leaves

void joint_corner(uint64_t bins_a, uint64_t bins_b, uint32_t *ra, uint32_t *rb) {
    uint64_t a = bins_a < kJointSide ? bins_a : kJointSide, b = bins_b < kJointSide ? bins_b : kJointSide;
    if (b < kJointSide)
        a = bins_a < kJointCorner / b ? bins_a : kJointCorner / b;
    else if (a < kJointSide)
        b = bins_b < kJointCorner / a ? bins_b : kJointCorner / a;
    *ra = (uint32_t)a;
    *rb = (uint32_t)b;
}

struct JointGeom {
    uint32_t last_d, last_s;      // bins - 1 of the driving / the other side
    uint32_t rd, rs;              // the LDS corner, rd * rs <= kJointCorner
    uint32_t stride_d, stride_s;  // cell (cd, cs) lies at matrix[cd * stride_d + cs * stride_s]
};

// One step of every lane of the wave (all 64 call this together): hit = this
// lane matched a pair that both sides keep, with the staged counts cd, cs.
__device__ __forceinline__ void joint_add(bool hit, uint32_t cd, uint32_t cs, const JointGeom &g, uint32_t *corner,
                                          ull *__restrict__ matrix) {
    const uint32_t bd = cd < g.last_d ? cd : g.last_d, bs = cs < g.last_s ? cs : g.last_s;  // clamp first
    const bool in = hit && bd < g.rd && bs < g.rs;
    if (hit && !in) atomicAdd(&matrix[(size_t)bd * g.stride_d + (size_t)bs * g.stride_s], 1ull);
    const uint32_t bin = bd * g.rs + bs;
#ifndef OKM_JOINT_BALLOT
    if (in) atomicAdd(&corner[bin], 1u);
#else
    ull todo = __ballot(in);
    while (todo) {  // wave-uniform: one round per distinct bin among the lanes
        const int lead = __ffsll((long long)todo) - 1;
        const uint32_t b = (uint32_t)__shfl((int)bin, lead, 64);
        const ull same = __ballot(in && bin == b);
        if ((int)(threadIdx.x & 63u) == lead) atomicAdd(&corner[b], (uint32_t)__popcll(same));
        todo &= ~same;
    }
#endif
}

template <typename KT, bool NARROW_D, bool NARROW_S>
__global__ __launch_bounds__(kCmpBlock) void k_joint_tiles(const CmpTile *__restrict__ tiles,
                                                           const ull *__restrict__ n_tiles,
                                                           const LookItem *__restrict__ ddesc,
                                                           const uint64_t *__restrict__ dcounts,
                                                           const LookItem *__restrict__ sdesc,
                                                           const uint64_t *__restrict__ scounts, ull min_d, ull min_s,
                                                           JointGeom g, ull *__restrict__ matrix) {
    typedef KeyOps<KT> O;
    constexpr uint32_t T = CmpTileOf<KT>::T;
    __shared__ KT dk[T], sk[T];
    __shared__ uint32_t dc[T], sc[T];
    __shared__ uint32_t corner[kJointCorner];
    const uint32_t nc = g.rd * g.rs;
    for (uint32_t b = threadIdx.x; b < nc; b += kCmpBlock) corner[b] = 0;
    __syncthreads();
    const ull nt = *n_tiles;
    for (ull ti = blockIdx.x; ti < nt; ti += gridDim.x) {  // every value that steers the loops is workgroup-uniform
        const CmpTile t = tiles[ti];
        if (t.s_run0 > t.s_run1 || (t.s_run0 == t.s_run1 && t.s_off0 >= t.s_off1)) continue;
        const uint32_t dl = t.d_len;
        // (the last walk of the tile before ended on a barrier: dk / dc are free)
        cmp_stage_kept<KT, NARROW_D>(ddesc + t.d_run, t.d_off, dl, dcounts, min_d, dk, dc);
        uint32_t run = t.s_run0;
        ull off = t.s_off0;
        for (;;) {  // one chunk of the S range per round, over as many S runs as it takes
            uint32_t sl = 0;
            while (sl < T && run <= t.s_run1) {
                const ull rend = run == t.s_run1 ? t.s_off1 : gload(&sdesc[run].n);
                if (off >= rend) {  // this run is done (the last one: the range is)
                    if (run == t.s_run1) break;
                    ++run;
                    off = 0;
                    continue;
                }
                const uint32_t take = (uint32_t)(rend - off < T - sl ? rend - off : T - sl);
                cmp_stage_kept<KT, NARROW_S>(sdesc + run, off, take, scounts, min_s, sk + sl, sc + sl);
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
            for (uint32_t q = 0; q < per; ++q) {  // per steps for every lane: joint_add is wave-uniform
                bool hit = false;
                uint32_t cd = 0, cs = 0;
                if (diag + q < dend) {
                    const bool has_d = i < dl, has_s = j < sl;
                    if (has_d && (!has_s || !O::lt(ks, kd))) {
                        if (has_s && O::eq(kd, ks)) {  // S's equal key is still ahead of j: each pair is seen once
                            cd = dc[i];
                            cs = sc[j];
                            hit = cd && cs;  // kept on both sides
                        }
                        ++i;
                        if (i < dl) kd = dk[i];
                    } else {
                        ++j;
                        if (j < sl) ks = sk[j];
                    }
                }
                joint_add(hit, cd, cs, g, corner, matrix);
            }
            __syncthreads();  // the next chunk overwrites sk / sc, the next tile dk / dc
        }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < nc; b += kCmpBlock) {
        const uint32_t v = corner[b];
        if (v) atomicAdd(&matrix[(size_t)(b / g.rs) * g.stride_d + (size_t)(b % g.rs) * g.stride_s], (ull)v);
    }
}

// Workgroup r < bins_a: row r; the others: column r - bins_a.  Reads only
// cells with ca >= 1 and cb >= 1, writes only column 0 / row 0; matrix[0][0]
// stays 0.
__global__ __launch_bounds__(256) void k_joint_finish(ull *__restrict__ matrix, const ull *__restrict__ hist_a,
                                                      const ull *__restrict__ hist_b, uint32_t bins_a,
                                                      uint32_t bins_b) {
    __shared__ ull wred[4];
    const bool row = blockIdx.x < bins_a;
    const uint32_t at = row ? blockIdx.x : blockIdx.x - bins_a;
    if (at == 0) return;
    ull v = 0;
    if (row)
        for (uint32_t cb = 1 + threadIdx.x; cb < bins_b; cb += 256) v += matrix[(size_t)at * bins_b + cb];
    else
        for (uint32_t ca = 1 + threadIdx.x; ca < bins_a; ca += 256) v += matrix[(size_t)ca * bins_b + at];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63u) == 0) wred[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        v = wred[0] + wred[1] + wred[2] + wred[3];
        if (row)
            matrix[(size_t)at * bins_b] = hist_a[at] - v;
        else
            matrix[at] = hist_b[at] - v;
    }
}

template <typename KT>
static void joint_tiles(hipStream_t s, const TableView &d, const TableView &sv, uint64_t min_d, uint64_t min_s,
                        const JointGeom &g, const unsigned long long *toff, const CmpTile *tiles,
                        unsigned long long *matrix) {
    const uint64_t max_tiles = compare_max_tiles(d.n, d.max_runs, CmpTileOf<KT>::T);
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        cus = 256;
    const uint64_t resident = (uint64_t)cus * kJointPerCU;
    const dim3 grid((uint32_t)(max_tiles < resident ? max_tiles : resident)), b(kCmpBlock);
    const unsigned long long *nt = toff + d.max_runs;
#define OKM_JOINT_LAUNCH(ND, NS)                                                                                \
    hipLaunchKernelGGL((k_joint_tiles<KT, ND, NS>), grid, b, 0, s, tiles, nt, d.desc, d.counts, sv.desc, sv.counts, \
                       min_d, min_s, g, matrix)
    if (d.narrow && sv.narrow)
        OKM_JOINT_LAUNCH(true, true);
    else if (d.narrow)
        OKM_JOINT_LAUNCH(true, false);
    else if (sv.narrow)
        OKM_JOINT_LAUNCH(false, true);
    else
        OKM_JOINT_LAUNCH(false, false);
#undef OKM_JOINT_LAUNCH
}

void launch_joint_tiles(void *stream, const TableView &d, const TableView &sv, bool wide, bool a_drives, uint64_t min_d,
                        uint64_t min_s, uint64_t bins_a, uint64_t bins_b, unsigned long long *toff,
                        unsigned long long *scan_tmp, CmpTile *tiles, unsigned long long *matrix) {
    if (!d.max_runs || !sv.max_runs) return;
    uint32_t ra, rb;
    joint_corner(bins_a, bins_b, &ra, &rb);
    JointGeom g;
    g.last_d = (uint32_t)((a_drives ? bins_a : bins_b) - 1);
    g.last_s = (uint32_t)((a_drives ? bins_b : bins_a) - 1);
    g.rd = a_drives ? ra : rb;
    g.rs = a_drives ? rb : ra;
    g.stride_d = a_drives ? (uint32_t)bins_b : 1u;
    g.stride_s = a_drives ? 1u : (uint32_t)bins_b;
    launch_compare_tile_offsets(stream, d, compare_tile(wide), toff, scan_tmp);
    launch_compare_bounds(stream, d, sv, wide, toff, tiles);
    if (wide)
        joint_tiles<K128>((hipStream_t)stream, d, sv, min_d, min_s, g, toff, tiles, matrix);
    else
        joint_tiles<ull>((hipStream_t)stream, d, sv, min_d, min_s, g, toff, tiles, matrix);
}

void launch_joint_finish(void *stream, unsigned long long *matrix, const unsigned long long *hist_a,
                         const unsigned long long *hist_b, uint64_t bins_a, uint64_t bins_b) {
    hipLaunchKernelGGL(k_joint_finish, dim3((uint32_t)(bins_a + bins_b)), dim3(256), 0, (hipStream_t)stream, matrix,
                       hist_a, hist_b, (uint32_t)bins_a, (uint32_t)bins_b);
}

}  // namespace okm
