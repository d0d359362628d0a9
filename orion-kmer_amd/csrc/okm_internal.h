// okm_internal.h — internal declarations shared by the library's translation
// units (not part of the C ABI).
#pragma once

#include <stdint.h>
#include <stddef.h>
#include <string>
#include <vector>

#include "orion_kmer.h"

namespace okm {

// thread-local last error (okm_last_error)
void set_error(const std::string &msg);
okm_status fail(okm_status s, const std::string &msg);

constexpr uint64_t kEmptyKey = ~0ull;

// Page-locked host memory (hipHostMalloc) for the host translation units
// (okm_group.cpp's device-to-file stream); nullptr on failure.
void *host_pinned_alloc(size_t bytes);
void host_pinned_free(void *p);
// Device-to-host copy issued on `device` (this thread's current device is set
// to it first, so the copy does not queue behind device 0's null stream).
okm_status memcpy_d2h_on(int device, void *dst, const void *src, size_t bytes);
// Test hook value (orion_kmer_testing.h okm_test_knob), -1 when unset.
int64_t test_knob(int knob);
// OKM_TEST_FAIL_ALLOC: counts one device arena allocation; true for the one that is to fail.
bool test_fail_alloc();

// Give back the idle device memory every context's pool on `device` caches
// (a hipMalloc outside the pools, e.g. a communicator buffer, retries after it).
void trim_device_pools(int device);
// Device bytes held outside the arenas (communicator buffers) count against
// the per-device budget too: +bytes when allocated, -bytes when freed.
void device_bytes_add(int device, int64_t delta);
// Would `bytes` more device memory pass the per-device budget (OKM_HBM_CAP)?
bool device_over_budget(int device, size_t bytes);

// The counted table where it lies: device memory, or (*on_host) page-locked
// host memory when count_spilled left it there (okm_group_write_counts_tsv
// streams either without moving it).
okm_status result_view(okm_ctx *c, const uint64_t **keys, const uint64_t **counts, uint64_t *n, bool *on_host);
// okm_merge_owned at one rank: the owner takes the local context's table
// without a copy (the two swap device pools); the local is left reset.
okm_status adopt_result(okm_ctx *owner, okm_ctx *local, bool *adopted);
// Whether adopt_result would adopt (counts the local; changes nothing else):
// okm_merge_owned_n adopts every table or none.
okm_status can_adopt_result(okm_ctx *owner, okm_ctx *local, bool *adoptable);

// Context accessors for the other translation units (okm_probe.hip).
int ctx_device(const okm_ctx *c);
bool ctx_is_wide(const okm_ctx *c);  // never a canonical key
uint32_t ctx_k(const okm_ctx *c);
// Key density of the next count's sorted runs (okm_merge_owned's owner): pairs
// per top-`fine_bits` key bin over the whole key space (zero outside the
// owner's range).  count_sorted_plan sizes each L1 part's split from the
// densest of its fine bins, so the first plan fits; okm_reset / the count
// clear it.  fine == nullptr clears.
void set_sorted_hint(okm_ctx *c, const unsigned long long *fine, uint32_t fine_bits);
bool ctx_is_set(const okm_ctx *c);

// ----------------------------------------------------------------------------
// Device-side launchers (okm_device.hip).  All take a hipStream_t as void*.
// ----------------------------------------------------------------------------

// A run of keys in device memory (optionally weighted).
struct DevSeg {
    const uint64_t *keys;
    const uint64_t *counts;  // nullptr => every key weighs 1
    uint64_t len;
    uint64_t key_base;       // (key >> shift) - key_base = local bin in [0, nlocal)
    uint32_t out_base;       // first output bin of this segment (compact numbering)
    uint32_t shift;          // kSingleBin (255) => a single bin
    uint32_t nlocal;         // bins this segment splits into (<= pass maximum)
    uint32_t pad;
};

// One unit of partition-pass work: a slice of a segment.
struct DevChunk {
    uint32_t seg;
    uint32_t pad;
    uint64_t begin;
    uint64_t len;
};

// One partition to count in LDS: segs[seg_begin, seg_begin + seg_count).
constexpr uint32_t kItemEmpty = 1;

struct DevItem {
    uint32_t seg_begin;
    uint32_t seg_count;
    uint64_t out_off;        // where its sorted distinct entries go (scratch)
    uint32_t rem_bits;       // key bits below the item's common prefix
    uint32_t pad;            // kItemEmpty: an empty fan-out slot (no segment read)
    uint64_t total;          // instances over all its segments
    const uint64_t *keys0;   // seg_count == 1: its segment's keys / counts (no
    const uint64_t *counts0; //   dependent segment load in the count kernels)
};

// Sampled L1 placement: bin b's claim cursor lives at cursor[b * kL1CurStride]
// (a stride > 1, every cursor on its own 128-B line, measured no faster).
constexpr uint32_t kL1CurStride = 1;

struct ExtractGeom {
    uint64_t n;        // bytes in the batch
    uint32_t k;
    uint32_t shift;    // bin = key >> shift (64 => single bin)
    uint32_t nbins;    // 1 << l1 bits
    uint32_t nblocks;  // persistent blocks (chunks)
    uint64_t chunk;    // window starts per block (multiple of the tile)
    uint32_t stride;   // block b covers chunk b * stride (> 1: a sample of the batch)
};

// L1: k-mer extraction from a batch, histogram by top key bits.
void launch_extract_hist(void *stream, const uint8_t *seq, const ExtractGeom &g, uint32_t *HC,
                         unsigned long long *Hg);
// L1: k-mer extraction + scatter into key-range partitions.  HC != null:
// exact placement from launch_extract_hist's per-block counts.  HC == null:
// sampled capacities (launch_l1_capacity), one claim per (tile, bin); a run
// crossing cap_end[bin] is dropped and *ovf set (the caller redoes the batch).
void launch_extract_scatter(void *stream, const uint8_t *seq, const ExtractGeom &g,
                            const uint32_t *HC, unsigned long long *cursor, uint64_t *out_keys,
                            const unsigned long long *cap_end, unsigned long long *ovf);
void launch_l1_capacity(void *stream, const unsigned long long *Hs, uint32_t nb, double scale, double mul,
                        uint32_t align, unsigned long long limit, unsigned long long *cursor,
                        unsigned long long *l1cap);

// Generic key-range partition pass over a chunk list.  max_local bounds every
// segment's nlocal; HC is nchunks x max_local (null: only Hg, e.g. a sample).
// wide: keys are K128 (two u64 each; pointers stay uint64_t*, lengths count keys).
void launch_part_hist(void *stream, const DevSeg *segs, const DevChunk *chunks, uint32_t nchunks,
                      uint32_t max_local, uint32_t *HC, unsigned long long *Hg, bool wide);
// HC null (tile mode only): sampled capacities, bin b's slot ends at
// cap_end[b]; one claim per (tile, bin), a crossing run is dropped and *ovf set.
void launch_part_scatter(void *stream, const DevSeg *segs, const DevChunk *chunks,
                         uint32_t nchunks, uint32_t max_local, const uint32_t *HC,
                         unsigned long long *cursor, uint64_t *out_keys, uint64_t *out_counts, bool wide,
                         const unsigned long long *cap_end = nullptr, unsigned long long *ovf = nullptr);
// Sampled partition capacities: H[b] (sampled count of output bin b) becomes
// the bin's capacity (in place); parents sorted by out_base.
struct DevCapParent {
    uint32_t out_base;
    uint32_t pad;
    double scale;            // parent keys / sampled parent keys
};
void launch_part_capacity(void *stream, unsigned long long *H, uint32_t nout, const DevCapParent *parents,
                          uint32_t nparents, double mul);
// Pads [end[b], roundup(end[b], line)) of every bin with the empty key (bins
// start on 128-B lines: 16 u64 / 8 K128 keys; end = the cursor after the scatter).
// cap (optional): skip bins whose end passed cap[b] (an overflowed sampled placement).
void launch_fill_line_tails(void *stream, const unsigned long long *end, uint32_t nbins, uint64_t *keys, bool wide,
                            const unsigned long long *cap = nullptr);
uint32_t extract_tile();
uint32_t extract_max_bins(bool wide);  // L1 bins: k <= 32 kernels vs k in 33..64
// L1 key bits a context extracts with: wide keys, or k <= 32 counting batch by
// batch (9) vs folding many batches into one table (10)
uint32_t extract_l1_bits(bool wide, bool folding);
uint32_t part_max_bins(bool weighted, bool wide);

// Exclusive scan of n u64 values (in -> out, out may equal in); tmp >= scan_tmp_elems(n).
size_t scan_tmp_elems(uint64_t n);
void launch_exclusive_scan(void *stream, const unsigned long long *in, unsigned long long *out,
                           uint64_t n, unsigned long long *tmp);

// LDS counting of partitions (okm_count.hip); writes sorted distinct
// (key,count) at out_off and n_out[item] (counts u32 unless weighted).  ctl[0] = error word, ctl[1] =
// deferred-item count (both zeroed before the launch).  An item holds at most count_item_capacity() instances unless
// its rem_bits <= count_dense_bits() (direct-address counting, any size).
uint32_t count_item_capacity();
uint32_t count_dense_bits();
// ctl[1] counts deferred items (list `defer`, nitems entries) for the second
// kernel of the launch.
void launch_count_items(void *stream, const DevItem *items, uint32_t nitems, const DevSeg *segs,
                        uint64_t *out_keys, uint64_t *out_counts, unsigned long long *n_out,
                        unsigned long long *ctl, uint32_t *defer, bool weighted, bool wide,
                        const unsigned long long *guard = nullptr, const unsigned long long *d_nitems = nullptr,
                        bool nowrite = false,  // nowrite: n_out only (weighted or wide launches)
                        bool narrow = false,
                        // multi_seg: some item may span several segments.  false (unweighted keys of
                        // at most 64 bits): the single-segment tag kernel, which hands any other item
                        // to the slow kernel -- exact either way, slower when such items are common
                        bool multi_seg = false);
// Wide keys straight into a caller's table (okm_count.hip: items by ticket,
// each run at its look-back prefix; no staging, no compaction).  status:
// nitems words and ctl[0..1] zeroed by the caller; fin_keys / fin_counts at
// the table's next entry, or at its start when fin_base (device) holds it.
void launch_count_direct(void *stream, const DevItem *items, uint32_t nitems, const DevSeg *segs,
                         unsigned long long *n_out, unsigned long long *ctl, bool weighted,
                         const unsigned long long *guard, const unsigned long long *d_nitems,
                         unsigned long long *status, uint64_t *fin_keys, uint64_t *fin_counts,
                         const unsigned long long *fin_base);  // weighted: u32 staged counts (ctl[0] |= 8 when one does not fit)

// k-way merge of sorted runs (okm_merge.hip): items as built by
// launch_sorted_items (each segment of an item a sorted unique run of keys),
// at most merge_item_capacity() instances and merge_max_runs() segments per
// item (else ctl[0] = 3).  write=0: n_out[item] = the item's distinct keys;
// write=1: its sorted distinct keys and summed u64 counts at
// out_keys/out_counts + dense_off[item] (the exclusive scan of n_out).
uint32_t merge_item_capacity();
uint32_t merge_max_runs();
void launch_merge_items(void *stream, const DevItem *items, uint32_t nitems, const DevSeg *segs,
                        unsigned long long *n_out, const unsigned long long *dense_off, uint64_t *out_keys,
                        uint64_t *out_counts, unsigned long long *ctl, bool weighted, bool wide, bool write);

// A part that took part in a device-side split round: its children are the
// output bins [out_base, out_base + nlocal) of the round.
struct DevParent {
    uint32_t out_base;
    uint32_t rem;            // key bits below the children's common prefix
};

// Fan-out of a round's children (k_fan_split): a child larger than one item
// (but <= split_max) is split in place by its next 1..bits key bits (the
// fewest that bring it to <= target); every child owns 2^bits item slots in
// key order, slots past its own sub-ranges are empty items.
struct DevFanJob {
    uint64_t off, len;
    uint32_t item0, bits, rem, pad;
    uint64_t doff;  // the child's first staged output slot (dense: the scan of child lengths)
};
struct FanOut {
    uint32_t bits = 0;          // 0: one item per child (no fan-out)
    uint32_t pad = 0;
    uint64_t target = 0;        // sub-range size aimed at
    uint64_t split_max = 0;     // largest child one job takes (fan_split_max())
    DevFanJob *jobs = nullptr;  // [nout]; job count in flags[3]
};
uint64_t fan_split_max();
// Unweighted jobs of at most this many keys are split in place (dk == sk):
// the register variant reads a job's keys before it writes any.
uint64_t fan_split_max_in_place();

// d_nitems (count kernels, compaction): when given, the item count is
// min(nitems, *d_nitems) -- a count known only on the device.

// One item (and one segment) per output bin of a split round, straight from
// the device offsets (nout + 1 entries; bin b ends at ends[b], or at
// offs[b + 1] when ends is null).  flags[0] += children that are still too
// big for one item; flags[1] |= 2 when a child needs 64-bit counting;
// flags[2] = max child length; flags[3] / flags[4] = fan-out jobs of <= / >
// 16 Ki keys (filed from the front / the back of fan.jobs[nout]).  Count and compact
// kernels given `guard` (= flags) return at once when guard[0] or guard[1] is
// set.  With fan.bits, item/segment slot i * 2^bits + j belongs to child i.
// doff (optional): every child's first staged output slot, the exclusive scan
// of the child lengths (launch_child_offsets) -- items then stage their
// (key, count) runs densely (L.total slots) instead of at their level offsets
// (the level's padded size).
void launch_make_items(void *stream, const unsigned long long *offs, const unsigned long long *ends, uint32_t nout,
                       const DevParent *parents, uint32_t nparents, const uint64_t *lk, const uint64_t *lc,
                       DevItem *items, DevSeg *segs, uint64_t item_max, uint32_t capbits,
                       unsigned long long *flags, uint32_t kw, const FanOut &fan,
                       const unsigned long long *doff = nullptr);
// doff[b] = sum of the lengths of children < b (b = 0..nout); tmp >= scan_tmp_elems(nout + 1).
void launch_child_offsets(void *stream, const unsigned long long *offs, const unsigned long long *ends, uint32_t nout,
                          unsigned long long *doff, unsigned long long *tmp);
// The fan-out jobs (flags[3] of them, <= max_jobs): keys of [off, off + len)
// of sk/sc are split into the same range of dk/dc and their sub-items written;
// oflags[0] += sub-ranges still too big, oflags[2] = max sub-range.
void launch_fan_split(void *stream, const DevFanJob *jobs, uint32_t max_jobs, const unsigned long long *flags,
                      const uint64_t *sk, const uint64_t *sc, uint64_t *dk, uint64_t *dc, DevItem *items,
                      DevSeg *segs, uint64_t item_max, uint32_t capbits, unsigned long long *oflags, bool wide);

// Sorted runs (okm_add_sorted_pairs_device).  out[b] = first index whose
// (key >> shift) >= b, b = 0..nbins (out[nbins] = n).
void launch_bin_bounds(void *stream, const uint64_t *keys, uint64_t n, uint32_t shift, uint32_t nbins,
                       unsigned long long *out, bool wide);
struct DevSortedPart {
    uint32_t bin;        // L1 bin of the part
    uint32_t bits;       // split into 2^bits children (0: one item)
    uint32_t item_base;  // first item of its children
    uint32_t slot;       // row of the part in the rbins table
};
// One multi-segment item per child (bounds: nitems * nruns words of scratch):
// segs[i * nruns + r] = the child's key range
// in run r (rbins[slot * nruns + r] = the part's range in run r); itemtot[i]
// = its instances; flags[0] += children still too big, flags[1] = max;
// part_max[slot] = the part's largest child (per-part replanning).
void launch_sorted_items(void *stream, const DevSortedPart *parts, uint32_t nparts, uint32_t nitems,
                         const DevSeg *rbins, uint32_t nruns, uint32_t shift1, DevItem *items, DevSeg *segs,
                         unsigned long long *itemtot, uint64_t item_max, uint32_t capbits, unsigned long long *flags,
                         bool wide, unsigned long long *bounds, unsigned long long *part_max);
void launch_set_out_off(void *stream, DevItem *items, uint32_t nitems, const unsigned long long *off);

// Gather the per-item results into dense arrays given exclusive offsets
// (nothing when a guard word or *err is set).  narrow: the per-item counts
// are u32 (unweighted count launches), widened to u64 here.
void launch_compact_items(void *stream, const DevItem *items, uint32_t nitems,
                          const unsigned long long *n_out, const unsigned long long *dense_off,
                          const uint64_t *src_keys, const uint64_t *src_counts,
                          uint64_t *dst_keys, uint64_t *dst_counts, bool wide, bool narrow,
                          const unsigned long long *guard = nullptr, const unsigned long long *err = nullptr,
                          const unsigned long long *d_nitems = nullptr, const unsigned long long *d_base = nullptr);
// Pipelined key-range groups: bit 63 of the device-side table base marks a
// pass in which a group was abandoned; no later group writes then.
constexpr unsigned long long kBasePoison = 1ull << 63;
// d_base (pipelined key-range groups): the compaction writes at dst + *d_base,
// and launch_advance_base then adds the group's distinct keys (*total) to it
// -- nothing of either when a guard word or *err is set.
void launch_advance_base(void *stream, unsigned long long *d_base, const unsigned long long *total,
                         const unsigned long long *guard, const unsigned long long *err);
// Drop the empty fan-out slots of items[0, nslots) (order kept) into out;
// *d_nitems (= pos[nslots]) receives the number kept.  flags/pos: nslots + 1
// words each, scan_tmp: scan_tmp_elems(nslots + 1).
void launch_item_compact(void *stream, const DevItem *items, uint32_t nslots, DevItem *out,
                         unsigned long long *flags, unsigned long long *pos, unsigned long long *scan_tmp);

// Filter (count >= min) with order preserved; flags/scan in tmp.
void launch_filter_count(void *stream, const uint64_t *counts, uint64_t n, uint64_t min_count,
                         unsigned long long *block_counts, uint32_t nblocks_hint);
void launch_filter_scatter(void *stream, const uint64_t *keys, const uint64_t *counts, uint64_t n,
                           uint64_t min_count, const unsigned long long *block_offsets,
                           uint64_t *dst_keys, uint64_t *dst_counts, bool wide);
uint32_t filter_blocks(uint64_t n);

// Count histogram (okm_hist.hip): hist[min(count, n_bins - 1)] += 1 per entry;
// summary[0] += entries, [1] += sum of counts, [2] = max count.  Both
// accumulate into what hist / summary hold (zeroed by the caller).  The items
// form reads the pending segmented table's counts (u32 when narrow) where the
// count kernels staged them; the dense form a flat u64 array.  Only entries
// with count >= min_count take part (1: every entry; the joint histogram's
// marginals pass their side's threshold).
void launch_hist_items(void *stream, const DevItem *items, uint32_t nitems, const unsigned long long *n_out,
                       const uint64_t *counts, bool narrow, uint64_t min_count, uint64_t n_bins,
                       unsigned long long *hist, unsigned long long *summary);
void launch_hist_dense(void *stream, const uint64_t *counts, uint64_t n, uint64_t min_count, uint64_t n_bins,
                       unsigned long long *hist, unsigned long long *summary);

// Co-occurrence matrix of a membership table (okm_cooccur.hip): every count is
// a mask of n_bits bits (1..64; higher bits ignored), out[i * n_bits + j] +=
// entries whose mask has bits i and j, out[n_bits * n_bits + p] += entries with
// p bits set.  out (zeroed by the caller) takes any number of launches.  The
// two forms read what launch_hist_items / launch_hist_dense read.  part:
// mask_matrix_part_words() u32 words of scratch, the workgroups' partials.
size_t mask_matrix_part_words();
void launch_mask_matrix_items(void *stream, const DevItem *items, uint32_t nitems, const unsigned long long *n_out,
                              const uint64_t *counts, bool narrow, uint32_t n_bits, uint32_t *part,
                              unsigned long long *out);
void launch_mask_matrix_dense(void *stream, const uint64_t *counts, uint64_t n, uint32_t n_bits, uint32_t *part,
                              unsigned long long *out);
// w[0, n) = weight (okm_pairwise_shared: sample i's membership bit beside its keys).
void launch_fill_weight(void *stream, uint64_t *w, uint64_t n, uint64_t weight);

// A counted table as the in-place readers' kernels see it (the lookup, the
// depth, the compare): one of two forms, both sorted by key.  The host's
// TableReader (okm_engine.hip) fills it for the representation the table lies
// in.  wide: keys are K128 (two u64 each; pointers stay uint64_t*, lengths
// count keys).
// The run list is the pending segmented table behind launch_lookup_index's
// index: the first key of every item that owns one (not kItemEmpty, n_out >
// 0), in item order, and a descriptor of its run.  launch_compare_cut writes
// the same arrays for a flat table.
struct LookItem {
    const uint64_t *keys;  // the run's ascending keys
    uint64_t coff;         // its counts start at counts[coff] (u32 or u64 words)
    uint64_t n;            // entries, > 0
};
struct TableView {
    bool runs = false;                            // the run list below is filled: read the table through it
    uint64_t n = 0;                               // entries (0: an empty table, nothing is read)
    const uint64_t *keys = nullptr;               // flat: keys[n], a dense table or one uploaded slice
    const uint64_t *counts = nullptr;             // flat: counts[n]; run r's at counts[desc[r].coff] (u32 when narrow)
    const uint64_t *first = nullptr;              // the first key of every run
    const LookItem *desc = nullptr;
    const unsigned long long *n_desc = nullptr;   // device: runs
    uint32_t max_runs = 0;                        // the host's bound of *n_desc
    bool narrow = false;
};

// Count lookup (okm_lookup.hip): out[i] = the count of query i in the table,
// *found += queries present.
// launch_lookup_index builds a pending table's run list.  Scratch: pos =
// nitems + 1 words (pos[nitems] = items kept, read on the device), scan_tmp =
// scan_tmp_elems(nitems + 1), first = nitems keys, desc = nitems LookItem.
void launch_lookup_index(void *stream, const DevItem *items, uint32_t nitems, const unsigned long long *n_out,
                         const uint64_t *src_keys, bool wide, unsigned long long *pos, unsigned long long *scan_tmp,
                         uint64_t *first, LookItem *desc);
// hits_only (a flat view only): absent queries leave out[i] as it is (one
// slice of a host-resident table; out zeroed by the caller).
void launch_lookup(void *stream, const TableView &t, bool wide, const uint64_t *queries, uint64_t nq, uint64_t *out,
                   unsigned long long *found, bool hits_only);

// Count compare (okm_compare.hip): two counted tables merged where they lie.
// Every representation is read through a TableView's run list;
// launch_compare_cut writes one for a flat table keys[n] (pieces of `tile`
// entries, the call's compare_tile: first and desc hold ceil(n / tile)
// entries, *n_desc receives that number).
// One tile of the driving table and the range of the other table under its key span (k_cmp_bounds).
struct CmpTile {
    uint32_t d_run, d_len;
    uint64_t d_off;
    uint32_t s_run0, s_run1;
    uint64_t s_off0, s_off1;
};
uint32_t compare_tile(bool wide);
uint64_t compare_max_tiles(uint64_t n, uint32_t max_runs, uint32_t tile);
void launch_compare_cut(void *stream, const uint64_t *keys, uint64_t n, bool wide, uint32_t tile, uint64_t *first,
                        LookItem *desc, unsigned long long *n_desc);
// out[0] += entries of v with count >= min_count, out[1] += the sum of their counts (mod 2^64).
void launch_compare_totals(void *stream, const TableView &v, uint64_t min_count, unsigned long long *out);
// Over the keys in both d and s whose counts pass min_d / min_s: their
// number, sum of min(count_d, count_s), sum of count_d, sum of count_s, added
// into words 0..3 of one of the slots of out (compare_slot_words() words,
// zeroed by the caller; any number of launches add into them);
// launch_compare_fold then adds the slots' sums to out4[0..3].  d drives (the larger table).  Scratch:
// toff = d.max_runs + 1 words, scan_tmp = scan_tmp_elems(d.max_runs + 1),
// tiles = compare_max_tiles(d.n, d.max_runs, compare_tile(wide)).
void launch_compare(void *stream, const TableView &d, const TableView &s, bool wide, uint64_t min_d, uint64_t min_s,
                    unsigned long long *toff, unsigned long long *scan_tmp, CmpTile *tiles, unsigned long long *out);
size_t compare_slot_words();
void launch_compare_fold(void *stream, const unsigned long long *slots, unsigned long long *out4);
// toff[r] = tiles of `tile` entries in d's runs before run r (toff[d.max_runs] = tiles in all): toff = d.max_runs + 1
// words, scan_tmp = scan_tmp_elems(d.max_runs + 1).
void launch_compare_tile_offsets(void *stream, const TableView &d, uint32_t tile, unsigned long long *toff,
                                 unsigned long long *scan_tmp);
// tiles[t] = tile t of d (cut at compare_tile(wide), toff as above) and the range of s under its key span.
void launch_compare_bounds(void *stream, const TableView &d, const TableView &s, bool wide,
                           const unsigned long long *toff, CmpTile *tiles);

// Joint count histogram (okm_jointhist.hip): the matrix of okm_compare_histogram.
// joint_corner: the low corner Ra x Rb of a bins_a x bins_b matrix that a
// workgroup of the merge keeps in LDS (Ra * Rb <= 2048; a narrow side leaves
// the wide one its rows).
void joint_corner(uint64_t bins_a, uint64_t bins_b, uint32_t *ra, uint32_t *rb);
// matrix[min(ca, bins_a - 1) * bins_b + min(cb, bins_b - 1)] += 1 per key kept
// on both sides (count >= its side's threshold).  d drives (the larger table);
// a_drives says which of the two is a.  Scratch as launch_compare's; matrix is
// zeroed by the caller and any number of launches add into it.
void launch_joint_tiles(void *stream, const TableView &d, const TableView &s, bool wide, bool a_drives, uint64_t min_d,
                        uint64_t min_s, uint64_t bins_a, uint64_t bins_b, unsigned long long *toff,
                        unsigned long long *scan_tmp, CmpTile *tiles, unsigned long long *matrix);
// Column 0 and row 0 from the two kept marginals: matrix[ca][0] = hist_a[ca] -
// the row's shared cells, matrix[0][cb] = hist_b[cb] - the column's.
void launch_joint_finish(void *stream, unsigned long long *matrix, const unsigned long long *hist_a,
                         const unsigned long long *hist_b, uint64_t bins_a, uint64_t bins_b);

// Table combine (okm_combine.hip): two counted tables merged into a sorted
// (key, u64 count) table; op is an okm_combine_op, d drives (the larger
// table), swapped: the call's left table a is s.  Views are run lists cut at
// combine_tile(wide); an empty s is a view of no runs.
// One tile of the driving table and where its range of the other table ends
// (it begins where the tile before ends; k_comb_bounds).
struct CombTile {
    uint32_t d_run, d_len;
    uint64_t d_off;
    uint32_t s_run1, pad_;
    uint64_t s_off1;
};
uint32_t combine_tile(bool wide);
// Pass 1.  Scratch: toff / scan_tmp as launch_compare_tile_offsets, tiles =
// M = compare_max_tiles(d.n, d.max_runs, combine_tile(wide)), tile_n = M + 1
// words zeroed by the caller, tile_scan_tmp = scan_tmp_elems(M + 1).
// Afterwards tile_n[t] = the output offset of tile t and tile_n[M] = the
// output's entries.
void launch_combine_count(void *stream, const TableView &d, const TableView &s, bool wide, int op, bool swapped,
                          uint64_t min_d, uint64_t min_s, unsigned long long *toff, unsigned long long *scan_tmp,
                          CombTile *tiles, unsigned long long *tile_n, unsigned long long *tile_scan_tmp);
// Pass 2, with pass 1's toff, tiles and tile offsets: okeys / ocounts hold tile_n[M] entries.
void launch_combine_write(void *stream, const TableView &d, const TableView &s, bool wide, int op, bool swapped,
                          uint64_t min_d, uint64_t min_s, const unsigned long long *toff, const CombTile *tiles,
                          unsigned long long *tile_off, uint64_t *okeys, uint64_t *ocounts);

// Per-record k-mer depth (okm_depth.hip): one scan of a device batch (records
// joined by separators, 16-byte aligned, n bytes) against one representation
// of the table; rows[r] accumulates record r's okm_read_depth (r = separators
// before the window, rows past nrec dropped).  The table is searched through
// the view's finder (okm_search.h with_finder).
// Rows start zeroed; any number of launches (slices of a host-resident table)
// add into them, exactly one of them with count_windows; the min field holds
// the largest ~count until launch_read_depths_fix turns it round, once, after
// the last launch.  tiles: 2 * depth_tiles(n) + scan_tmp_elems(depth_tiles(n))
// words of scratch; depth_tiles(n) < 2^31.
uint64_t depth_tiles(uint64_t n_bytes);
// tile_cnt[t] = the separators among the bytes of scan tile t, depth_tiles(n) words (the quantiles' bounds too).
void launch_depth_sep_count(void *stream, const uint8_t *seq, uint64_t n, unsigned long long *tile_cnt);
void launch_read_depths(void *stream, const uint8_t *seq, uint64_t n, uint64_t nrec, uint32_t k, bool wide,
                        const TableView &t, uint64_t min_count, bool count_windows, unsigned long long *tiles,
                        okm_read_depth *rows);
void launch_read_depths_fix(void *stream, okm_read_depth *rows, uint64_t nrec);
// a += b for rows taken over the same reads against tables of disjoint keys
// (the slices of a host-resident table, the owners of a group): the rule
// orion_kmer.h states for okm_read_depth.  windows is left as a's.
inline void depth_combine(okm_read_depth &a, const okm_read_depth &b) {
    if (!b.present) return;
    a.min = a.present && a.min < b.min ? a.min : b.min;
    a.max = a.max > b.max ? a.max : b.max;
    a.present += b.present;
    a.solid += b.solid;
    a.sum += b.sum;
}

// Per-record solid runs (okm_solid.hip), in two stages over a device batch
// (records joined by separators, 16-byte aligned, 0 < n < 2^32 bytes).
// planes: 2 * solid_plane_words(n) words, the solid bit plane and then the
// separator bit plane, one bit per batch byte.  launch_solid_mask is
// launch_read_depths' scan and search into bits: the batch's first
// launch (`first`) writes both planes whole, every later one (a further slice
// of a host-resident table) ORs its hits into the solid plane.
// launch_solid_runs then turns the planes into rows[nrec] (r = separators
// before the slot, rows past nrec dropped, every row written).  tiles:
// 4 * solid_tiles(n) + scan_tmp_elems(solid_tiles(n)) words of scratch.
uint64_t solid_tiles(uint64_t n_bytes);
uint64_t solid_plane_words(uint64_t n_bytes);
void launch_solid_mask(void *stream, const uint8_t *seq, uint64_t n, uint32_t k, bool wide, const TableView &t,
                       uint64_t min_count, bool first, unsigned long long *planes);
void launch_solid_runs(void *stream, uint64_t n, uint64_t nrec, uint32_t k, const unsigned long long *planes,
                       unsigned long long *tiles, okm_solid_run *rows);

// Per-record count quantiles (okm_quantile.hip), in two stages over a device
// batch (records joined by separators, 16-byte aligned, 0 < n < 2^32 bytes).
// plane: quant_plane_words(n) words, one uint32_t per position of the batch's
// whole scan tiles.  launch_quantile_counts is launch_read_depths' scan and
// search into that plane: the batch's first launch (`first`) writes its every
// word (2^32 - 1: no valid window; else the clipped count, 0 when absent),
// every later one (a further slice of a host-resident table) stores its hits.
// launch_quantile_select then ranks every record's words where they lie into
// rows[nrec * (1 + nq)] (windows, then the nq quantiles; r = separators before
// the record, rows past nrec dropped, every row written).  q: host.  tiles:
// quant_tile_words(n, nrec) words of scratch.
uint64_t quant_plane_words(uint64_t n_bytes);
uint64_t quant_tile_words(uint64_t n_bytes, uint64_t nrec);
void launch_quantile_counts(void *stream, const uint8_t *seq, uint64_t n, uint32_t k, bool wide, const TableView &t,
                            bool first, unsigned long long *plane);
void launch_quantile_select(void *stream, const uint8_t *seq, uint64_t n, uint64_t nrec, uint32_t k,
                            const okm_quantile *q, uint32_t nq, const unsigned long long *plane,
                            unsigned long long *tiles, uint64_t *rows);

// Per-record count intervals (okm_interval.hip), over a device batch as the
// solid runs take it and in their planes (2 * solid_plane_words(n) words).
// launch_interval_mask is launch_solid_mask with the predicate lo <= count <=
// hi, an absent k-mer counting 0: the first launch writes both planes whole,
// every later one (a further slice of a host-resident table) overrides the bits
// of the windows it holds.  launch_interval_index then ranks the runs (of
// slots, or of the bases their windows cover) and the records into tiles,
// interval_tile_words(n, nrec) words of scratch, and launch_interval_rows,
// any number of times after it, writes rows[0 .. min(total, cap)) (rows may be
// null when cap == 0; records numbered from rec0; no row of a record past nrec)
// and returns the device word that holds the total.
uint64_t interval_tile_words(uint64_t n_bytes, uint64_t nrec);
void launch_interval_mask(void *stream, const uint8_t *seq, uint64_t n, uint32_t k, bool wide, const TableView &t,
                          uint64_t lo, uint64_t hi, bool first, unsigned long long *planes);
void launch_interval_index(void *stream, uint64_t n, uint64_t nrec, uint32_t k, bool slots,
                           const unsigned long long *planes, unsigned long long *tiles);
const unsigned long long *launch_interval_rows(void *stream, uint64_t n, uint64_t nrec, uint32_t k, bool slots,
                                               const unsigned long long *planes, unsigned long long *tiles,
                                               uint64_t rec0, okm_count_interval *rows, uint64_t cap);

// FASTA/FASTQ text to the batch layout (okm_text.hip), over one chunk of n >= 1
// bytes of 16-B aligned text, n < 2^31.  Tile words: text_tiles(n) each.
//   launch_text_lines       tile_sum[t]: FASTQ the tile's newlines; FASTA bit 0 a
//                           line starts in it, bit 1 the last such line is a header
//                           (at_start: the chunk's first byte starts a line)
//   launch_text_scan        one workgroup: the sum (out[t] = base + in[0, t)) or,
//                           with `state`, the header bit at each tile's first byte;
//                           init (optional): the chunk's status words, see below
//   launch_text_keep_count  tile_keep[t] = kept bytes | FASTA headers << 32; FASTQ
//                           writes every newline's position to nlidx[0, nl_cap)
//   launch_text_compact     the kept bytes to out + (tile_off[t] & 2^32 - 1);
//                           *out_end = the end of the output
//   launch_text_check       FASTQ records over nlidx[0, nnl): words[0] = min of
//                           record * 8 + TextError over the failing records (~0:
//                           none), words[1] = end of the last record looked at,
//                           words[6] = records looked at; `last`: the text ends here
//   launch_text_tail        words[3] = the chunk ends in '\n', bytes of words[8..15]
//                           = the output's last 64 bytes (its end is words[2])
//   launch_text_blank       *flag = 1 when text[0, n) holds a byte other than CR / LF
enum TextError : uint32_t { kTextBlank = 1, kTextNoAt = 2, kTextTruncated = 3, kTextNoPlus = 4, kTextLengths = 5 };
uint64_t text_tiles(uint64_t n_bytes);
void launch_text_lines(void *stream, bool fastq, const uint8_t *text, uint64_t n, uint32_t at_start,
                       unsigned long long *tile_sum);
void launch_text_scan(void *stream, const unsigned long long *in, uint64_t nt, unsigned long long base, bool state,
                      unsigned long long *out, unsigned long long *total, unsigned long long *init);
void launch_text_keep_count(void *stream, bool fastq, const uint8_t *text, uint64_t n, uint32_t at_start,
                            const unsigned long long *tile_state, unsigned long long *tile_keep, uint32_t *nlidx,
                            uint64_t nl_cap);
void launch_text_compact(void *stream, bool fastq, const uint8_t *text, uint64_t n, uint32_t at_start,
                         const unsigned long long *tile_state, const unsigned long long *tile_off, uint8_t *out,
                         unsigned long long *out_end);
void launch_text_check(void *stream, const uint8_t *text, uint64_t n, const uint32_t *nlidx, uint64_t nnl, bool last,
                       unsigned long long *words);
void launch_text_tail(void *stream, const uint8_t *out, const uint8_t *text, uint64_t n, unsigned long long *words);
void launch_text_blank(void *stream, const uint8_t *text, uint64_t n, unsigned long long *flag);

// |A ∩ B| of sorted unique arrays (merge-path style binary search per element).
void launch_intersect_count(void *stream, const uint64_t *a, uint64_t na, const uint64_t *b,
                            uint64_t nb, unsigned long long *out, bool wide);

}  // namespace okm
