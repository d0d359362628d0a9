// okm_text.hip — FASTA/FASTQ text to the batch layout, on the device.
//
// The batch layout the extraction takes (whitespace-free records joined by
// '\n') is a subsequence of the file's own bytes: FASTQ keeps the sequence
// lines (index % 4 == 1) with their '\n'; FASTA keeps the non-header lines
// without their whitespace and every header line's '\n'.  So parsing is a
// classification of bytes by line and a stream compaction:
//
//   k_text_lines  per 16 KiB tile: its newlines (FASTQ), or whether a line
//                 starts in it and whether the last such line is a header
//   k_text_scan   one workgroup over the tile words: a sum, or the "last
//                 writer wins" state; reduce-then-scan, nobody waits
//   k_text_keep   the 64-bit keep mask of each thread's 64 bytes; first pass
//                 counts (and writes the FASTQ newline index), second pass
//                 compacts through an LDS tile and copies out in 16-B stores
//   k_text_check  FASTQ: one thread per record over the newline index, the
//                 host parser's conditions (okm_fastx.cpp next_span)
//
// A thread owns 64 bytes: four 16-B loads, every mask by SWAR compares.  No
// load starts at or past the text's last granule (clamped as
// load_windows_clamped does) and bytes at or past n are in no mask.
#include "okm_dev_common.h"
#include "okm_scan.h"

namespace okm {
namespace {

constexpr int kTextBlock = 256;
constexpr uint32_t kTextRun = 64;                       // bytes per thread
constexpr uint32_t kTextTile = kTextBlock * kTextRun;  // 16 KiB per workgroup

// One bit per byte of x that equals c.
__device__ __forceinline__ uint32_t eq4(uint32_t x, uint32_t c) {
    const uint32_t m = zero_bytes(x ^ (c * 0x01010101u));
    return ((((m >> 7) & 0x01010101u) * 0x00204081u) >> 21) & 0xFu;
}

struct RunMasks {
    uint64_t valid;  // bytes before n
    uint64_t nl;     // '\n'
    uint64_t ws;     // space, tab, CR, '\n'
    uint64_t gt;     // '>'
};

// The 64 bytes at p0 (a multiple of 64) of the 16-B aligned text and their masks.
__device__ __forceinline__ RunMasks load_run(const uint8_t *__restrict__ text, uint64_t n, uint64_t p0, uint32_t *w) {
    const uint64_t lastg = (n - 1) >> 4;  // n >= 1
    const uint4 *p = reinterpret_cast<const uint4 *>(text);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint64_t g = (p0 >> 4) + (uint64_t)q;
        const uint4 v = gload(p + (g < lastg ? g : lastg));
        w[4 * q + 0] = v.x;
        w[4 * q + 1] = v.y;
        w[4 * q + 2] = v.z;
        w[4 * q + 3] = v.w;
    }
    RunMasks m;
    m.valid = p0 >= n ? 0ull : (n - p0 >= 64 ? ~0ull : ((1ull << (n - p0)) - 1ull));
    m.nl = m.ws = m.gt = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint32_t x = w[i];
        const uint32_t a = eq4(x, '\n');
        const uint32_t b = a | eq4(x, ' ') | eq4(x, '\t') | eq4(x, '\r');
        m.nl |= (uint64_t)a << (4 * i);
        m.ws |= (uint64_t)b << (4 * i);
        m.gt |= (uint64_t)eq4(x, '>') << (4 * i);
    }
    m.nl &= m.valid;
    m.ws &= m.valid;
    m.gt &= m.valid;
    return m;
}

// Line starts among the thread's bytes: after each '\n', and at its first
// byte when the byte before it is one (at the text's first byte: `at_start`).
__device__ __forceinline__ uint64_t line_starts(const uint8_t *__restrict__ text, uint64_t n, uint64_t p0,
                                                const RunMasks &m, uint32_t at_start) {
    uint64_t first = 0;
    if (p0 == 0) first = at_start & 1u;
    else if (p0 < n) first = text[p0 - 1] == '\n';
    return ((m.nl << 1) | first) & m.valid;
}

// Block-wide maximum scan: the largest value of the threads before this one
// (0 when none), *total = the largest of all.  wmax: kTextBlock / 64 words.
__device__ __forceinline__ ull block_excl_max(ull v, ull *wmax, ull *total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    ull inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const ull o = __shfl_up(inc, d, 64);
        if (lane >= d && o > inc) inc = o;
    }
    ull ex = __shfl_up(inc, 1, 64);
    if (lane == 0) ex = 0;
    if (lane == 63) wmax[wid] = inc;
    lds_sync();
    ull tot = 0;
#pragma unroll
    for (int i = 0; i < kTextBlock / 64; ++i) {
        const ull s = wmax[i];
        if (i < wid && s > ex) ex = s;
        if (s > tot) tot = s;
    }
    lds_sync();
    *total = tot;
    return ex;
}

// A line-start summary as a word whose maximum is the LAST writer: 0 = no
// line starts here, else (position rank + 1) * 2 + (that line is a header).
__device__ __forceinline__ ull start_word(uint64_t starts, uint64_t gt, uint64_t rank) {
    if (!starts) return 0;
    const int last = 63 - __clzll((long long)starts);
    return ((rank + 1) << 1) | ((gt >> last) & 1ull);
}

template <bool FQ>
__global__ __launch_bounds__(kTextBlock) void k_text_lines(const uint8_t *__restrict__ text, uint64_t n,
                                                           uint32_t at_start, ull *__restrict__ tile_sum) {
    __shared__ ull wred[kTextBlock / 64];
    const uint64_t p0 = (uint64_t)blockIdx.x * kTextTile + (uint64_t)threadIdx.x * kTextRun;
    uint32_t w[16];
    const RunMasks m = load_run(text, n, p0, w);
    ull tot;
    if (FQ) {
        (void)block_excl_scan<kTextBlock>((ull)__popcll(m.nl), wred, &tot);
    } else {
        const uint64_t starts = line_starts(text, n, p0, m, at_start);
        (void)block_excl_max(start_word(starts, m.gt, threadIdx.x), wred, &tot);
        tot = tot ? (1ull | ((tot & 1ull) << 1)) : 0ull;  // bit 0: a line starts here, bit 1: the last is a header
    }
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = tot;
}

// One workgroup over the tile words.  state == 0: out[t] = base + the sum of
// in[0, t), *total = base + the sum of all.  state == 1: out[t] = the header
// bit of the last tile before t in which a line starts (base when none),
// *total = that after the last tile.  init: the status words of a new chunk.
__global__ __launch_bounds__(kTextBlock) void k_text_scan(const ull *__restrict__ in, uint64_t nt, ull base, int state,
                                                          ull *__restrict__ out, ull *__restrict__ total,
                                                          ull *__restrict__ init) {
    __shared__ ull wred[kTextBlock / 64];
    ull carry = base;
    for (uint64_t i0 = 0; i0 < nt; i0 += kTextBlock) {
        const uint64_t i = i0 + threadIdx.x;
        const ull v = i < nt ? in[i] : 0ull;
        ull tot;
        if (!state) {
            const ull ex = block_excl_scan<kTextBlock>(v, wred, &tot);
            if (i < nt) out[i] = carry + ex;
            carry += tot;
        } else {
            const ull ex = block_excl_max((v & 1ull) ? (((ull)threadIdx.x + 1) << 1) | ((v >> 1) & 1ull) : 0ull, wred, &tot);
            if (i < nt) out[i] = ex ? (ex & 1ull) : carry;
            if (tot) carry = tot & 1ull;
        }
    }
    if (threadIdx.x == 0) {
        *total = carry;
        if (init) {
            init[0] = ~0ull;  // the lowest failing record and its kind
            init[1] = 0;      // where the last complete record ends
            init[6] = 0;      // records checked
        }
    }
}

// Bits [lo, hi) of a 64-bit word.
__device__ __forceinline__ uint64_t bit_range(int lo, int hi) {
    const uint64_t a = lo >= 64 ? 0ull : ~0ull << lo;
    const uint64_t b = hi >= 64 ? ~0ull : ((1ull << hi) - 1ull);
    return a & b;
}

// COMPACT == false: tile_keep[t] = kept bytes of tile t, FASTA header lines
// that start in it in the high half; FASTQ also writes the position of every
// '\n' to nlidx (nl_cap entries).  COMPACT == true: the kept bytes go to out
// at the low half of tile_off[t], and the last tile writes the end of the
// output to *out_end.  tile_state[t]: FASTQ the line index at the tile's first
// byte, FASTA whether that byte lies in a header line.
template <bool FQ, bool COMPACT>
__global__ __launch_bounds__(kTextBlock) void k_text_keep(const uint8_t *__restrict__ text, uint64_t n,
                                                          uint32_t at_start, const ull *__restrict__ tile_state,
                                                          const ull *__restrict__ tile_off, ull *__restrict__ tile_keep,
                                                          uint32_t *__restrict__ nlidx, uint64_t nl_cap,
                                                          uint8_t *__restrict__ out, ull *__restrict__ out_end) {
    __shared__ ull wred[kTextBlock / 64];
    __shared__ uint32_t wred32[kTextBlock / 64];
    __shared__ uint32_t buf[COMPACT ? kTextTile / 4 + 4 : 1];
    const uint64_t p0 = (uint64_t)blockIdx.x * kTextTile + (uint64_t)threadIdx.x * kTextRun;
    uint32_t w[16];
    const RunMasks m = load_run(text, n, p0, w);
    const ull state0 = tile_state[blockIdx.x];
    uint64_t keep = 0;
    uint32_t headers = 0;
    if (FQ) {
        ull tot;
        const ull before = state0 + block_excl_scan<kTextBlock>((ull)__popcll(m.nl), wred, &tot);  // newlines before p0
        uint32_t cur = (uint32_t)before & 3u;
        int lo = 0;
        ull ord = before;
        for (uint64_t r = m.nl; r; r &= r - 1) {  // per line, not per byte
            const int j = __ffsll((long long)r) - 1;
            if (cur == 1) keep |= bit_range(lo, j + 1);
            if (!COMPACT && ord < nl_cap) nlidx[ord] = (uint32_t)(p0 + (uint64_t)j);
            ++ord;
            cur = (cur + 1) & 3u;
            lo = j + 1;
        }
        if (cur == 1) keep |= bit_range(lo, 64);
        keep &= ~(m.ws & ~m.nl) & m.valid;
    } else {
        const uint64_t starts = line_starts(text, n, p0, m, at_start);
        ull tot;
        const ull ex = block_excl_max(start_word(starts, m.gt, threadIdx.x), wred, &tot);
        uint64_t cur = ex ? (ex & 1ull) : (state0 & 1ull);  // is the line at p0 a header
        uint64_t hdr = 0;
        int lo = 0;
        for (uint64_t r = starts; r; r &= r - 1) {  // per line
            const int j = __ffsll((long long)r) - 1;
            if (cur) hdr |= bit_range(lo, j);
            cur = (m.gt >> j) & 1ull;
            lo = j;
        }
        if (cur) hdr |= bit_range(lo, 64);
        keep = ((hdr & m.nl) | (~hdr & ~m.ws)) & m.valid;
        headers = (uint32_t)__popcll(starts & m.gt);
    }
    const uint32_t kept = (uint32_t)__popcll(keep);
    if (!COMPACT) {
        ull tot;
        (void)block_excl_scan<kTextBlock>((ull)kept | ((ull)headers << 32), wred, &tot);
        if (threadIdx.x == 0) tile_keep[blockIdx.x] = tot;
        return;
    }
    uint32_t tot;
    uint32_t at = block_excl_scan_u32<kTextBlock>(kept, wred32, &tot);
    uint8_t *bytes = reinterpret_cast<uint8_t *>(buf);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        if (((keep >> (16 * g)) & 0xFFFFull) == 0) continue;
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const int j = 16 * g + b;
            if ((keep >> j) & 1ull) bytes[at++] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
        }
    }
    lds_sync();
    const uint64_t off = tile_off[blockIdx.x] & 0xFFFFFFFFull;
    uint8_t *dst = out + off;
    const uint32_t lead = (uint32_t)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u);
    const uint32_t head = lead < tot ? lead : tot;
    const uint32_t nvec = (tot - head) >> 4;
    for (uint32_t i = threadIdx.x; i < head; i += kTextBlock) dst[i] = bytes[i];
    for (uint32_t v = threadIdx.x; v < nvec; v += kTextBlock) {
        const uint32_t s = head + 16 * v, a = s >> 2, sh = (s & 3u) * 8;
        uint32_t x[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) x[i] = buf[a + i];  // a + 4 <= kTextTile / 4
        uint4 r;
        r.x = funnel32(x[1], x[0], sh);
        r.y = funnel32(x[2], x[1], sh);
        r.z = funnel32(x[3], x[2], sh);
        r.w = funnel32(x[4], x[3], sh);
        *reinterpret_cast<uint4 *>(dst + s) = r;
    }
    for (uint32_t i = head + 16 * nvec + threadIdx.x; i < tot; i += kTextBlock) dst[i] = bytes[i];
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *out_end = off + tot;
}

// FASTQ records over the newline index nl[0, nnl): record r is lines 4r ..
// 4r + 3, line i is [i ? nl[i - 1] + 1 : 0, i < nnl ? nl[i] : n).  last: the
// text ends here, so an unterminated last line is a line and a record short of
// four lines is truncated; otherwise only records whose four lines end in
// '\n' are looked at, the rest is presented again.  words[0] = min over the
// failing records of r * 8 + kind, words[1] = where the last record ends,
// words[6] = records.
__global__ __launch_bounds__(kTextBlock) void k_text_check(const uint8_t *__restrict__ text, uint64_t n,
                                                           const uint32_t *__restrict__ nl, uint64_t nnl, uint32_t last,
                                                           ull *__restrict__ words) {
    const uint64_t tail_begin = nnl ? (uint64_t)nl[nnl - 1] + 1 : 0;
    const uint64_t lines = nnl + ((last && tail_begin < n) ? 1 : 0);
    const uint64_t nrec = last ? (lines + 3) / 4 : nnl / 4;
    const uint64_t r = (uint64_t)blockIdx.x * kTextBlock + threadIdx.x;
    if (r >= nrec) return;
    const auto begin = [&](uint64_t i) { return i ? (uint64_t)nl[i - 1] + 1 : 0ull; };  // i <= nnl
    const auto end = [&](uint64_t i) { return i < nnl ? (uint64_t)nl[i] : n; };
    const auto strip = [&](uint64_t b, uint64_t e) {
        while (e > b && text[e - 1] == '\r') --e;
        return e - b;
    };
    const uint8_t c0 = text[begin(4 * r)];  // the line exists, so it begins before n
    uint32_t kind = 0;
    if (c0 == '\n' || c0 == '\r') kind = kTextBlank;
    else if (c0 != '@') kind = kTextNoAt;
    else if (4 * r + 3 >= lines) kind = kTextTruncated;
    else if (text[begin(4 * r + 2)] != '+') kind = kTextNoPlus;
    else if (strip(begin(4 * r + 1), end(4 * r + 1)) != strip(begin(4 * r + 3), end(4 * r + 3))) kind = kTextLengths;
    if (kind) atomicMin(&words[0], (r << 3) | kind);
    if (r == nrec - 1) {
        const uint64_t e = 4 * r + 3 < lines ? end(4 * r + 3) + 1 : n;
        words[1] = e < n ? e : n;
        words[6] = nrec;
    }
}

// After a FASTA chunk: the last 64 bytes of the output (right-aligned, zeros
// in front of a shorter one) and whether the chunk's last byte is a '\n'.
__global__ __launch_bounds__(64) void k_text_tail(const uint8_t *__restrict__ out, const uint8_t *__restrict__ text,
                                                  uint64_t n, ull *__restrict__ words) {
    const uint64_t total = words[2];
    const uint32_t i = threadIdx.x;
    uint8_t *tail = reinterpret_cast<uint8_t *>(words + 8);
    tail[i] = total + i >= 64 ? out[total + i - 64] : (uint8_t)0;
    if (i == 0) words[3] = text[n - 1] == '\n';
}

// *flag = 1 when a byte of text[0, n) is neither CR nor LF (any alignment).
__global__ __launch_bounds__(kTextBlock) void k_text_blank(const uint8_t *__restrict__ text, uint64_t n,
                                                           ull *__restrict__ flag) {
    bool other = false;
    for (uint64_t i = (uint64_t)blockIdx.x * kTextBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kTextBlock)
        other |= text[i] != '\n' && text[i] != '\r';
    if (other) *flag = 1;
}

}  // namespace

uint64_t text_tiles(uint64_t n_bytes) { return (n_bytes + kTextTile - 1) / kTextTile; }

void launch_text_lines(void *stream, bool fastq, const uint8_t *text, uint64_t n, uint32_t at_start,
                       unsigned long long *tile_sum) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t nt = (uint32_t)text_tiles(n);
    if (fastq) hipLaunchKernelGGL(k_text_lines<true>, dim3(nt), dim3(kTextBlock), 0, s, text, n, at_start, tile_sum);
    else hipLaunchKernelGGL(k_text_lines<false>, dim3(nt), dim3(kTextBlock), 0, s, text, n, at_start, tile_sum);
}

void launch_text_scan(void *stream, const unsigned long long *in, uint64_t nt, unsigned long long base, bool state,
                      unsigned long long *out, unsigned long long *total, unsigned long long *init) {
    hipLaunchKernelGGL(k_text_scan, dim3(1), dim3(kTextBlock), 0, static_cast<hipStream_t>(stream), in, nt, base,
                       state ? 1 : 0, out, total, init);
}

void launch_text_keep_count(void *stream, bool fastq, const uint8_t *text, uint64_t n, uint32_t at_start,
                            const unsigned long long *tile_state, unsigned long long *tile_keep, uint32_t *nlidx,
                            uint64_t nl_cap) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t nt = (uint32_t)text_tiles(n);
    if (fastq)
        hipLaunchKernelGGL((k_text_keep<true, false>), dim3(nt), dim3(kTextBlock), 0, s, text, n, at_start, tile_state,
                           nullptr, tile_keep, nlidx, nl_cap, nullptr, nullptr);
    else
        hipLaunchKernelGGL((k_text_keep<false, false>), dim3(nt), dim3(kTextBlock), 0, s, text, n, at_start, tile_state,
                           nullptr, tile_keep, nullptr, 0, nullptr, nullptr);
}

void launch_text_compact(void *stream, bool fastq, const uint8_t *text, uint64_t n, uint32_t at_start,
                         const unsigned long long *tile_state, const unsigned long long *tile_off, uint8_t *out,
                         unsigned long long *out_end) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t nt = (uint32_t)text_tiles(n);
    if (fastq)
        hipLaunchKernelGGL((k_text_keep<true, true>), dim3(nt), dim3(kTextBlock), 0, s, text, n, at_start, tile_state,
                           tile_off, nullptr, nullptr, 0, out, out_end);
    else
        hipLaunchKernelGGL((k_text_keep<false, true>), dim3(nt), dim3(kTextBlock), 0, s, text, n, at_start, tile_state,
                           tile_off, nullptr, nullptr, 0, out, out_end);
}

void launch_text_check(void *stream, const uint8_t *text, uint64_t n, const uint32_t *nlidx, uint64_t nnl, bool last,
                       unsigned long long *words) {
    const uint64_t nrec = last ? (nnl + 4) / 4 : nnl / 4;  // at least the kernel's own number
    if (!nrec) return;
    hipLaunchKernelGGL(k_text_check, dim3((uint32_t)((nrec + kTextBlock - 1) / kTextBlock)), dim3(kTextBlock), 0,
                       static_cast<hipStream_t>(stream), text, n, nlidx, nnl, last ? 1u : 0u, words);
}

void launch_text_tail(void *stream, const uint8_t *out, const uint8_t *text, uint64_t n, unsigned long long *words) {
    hipLaunchKernelGGL(k_text_tail, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), out, text, n, words);
}

void launch_text_blank(void *stream, const uint8_t *text, uint64_t n, unsigned long long *flag) {
    const uint64_t nb = std::min<uint64_t>((n + kTextBlock - 1) / kTextBlock, 1024);
    hipLaunchKernelGGL(k_text_blank, dim3((uint32_t)nb), dim3(kTextBlock), 0, static_cast<hipStream_t>(stream), text, n,
                       flag);
}

}  // namespace okm
