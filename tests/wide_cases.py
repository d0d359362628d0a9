"""Inputs for the wide (k in 33..64) count-shape tests
(tests/test_gpu_wide_item_shapes.py) and their CPU self-check
(tests/test_wide_cases.py): seeded, numpy and Python integers only.

A wide key is a Python int below 4^k, stored as two u64 words [lo, hi].  The
engine gives a key three fields, each a bit range [low, high) of the 2k-bit
key, and each can lie below bit 64 (in lo), above it (in hi) or across it:

  L1 bin       the top 9 bits,                    [2k - 9, 2k)
  partition    b bits below the L1 bin,           [2k - 9 - b, 2k - 9)
               (a part of more than 4096 instances takes a pass of b bits:
               the smallest b that brings its children to 3072 or fewer)
  home         the 12 bits below an item's prefix, [rem - 12, rem), where rem
               is the item's remaining bits: 2k - 9 with no partition pass,
               2k - 9 - b after one

An L1 bin cannot lie wholly below bit 64 at k >= 33 (its top bit is 2k - 1 >=
65); every other (field, side) pair occurs, and KS -- derived below from the
constants, not typed in -- holds, for each field, the largest k where it lies
below bit 64, the smallest and largest k where it straddles it and the
smallest k where it lies above, plus 33 (hi holds 2 bits, all inside the L1
bin), 63 and 64.  PASS_BITS = 5 is the pass a 70 000-key part takes.

   k   L1 shift   rem (no pass)   home shift   L1    partition   home   home after
                                                     (5 bits)           the pass
  33      57           57             45       str     below     below    below
  36      63           63             51       str     below     below    below
  37      65           65             53       above   str       str      below
  38      67           67             55       above   str       str      below
  39      69           69             57       above   above     str      below
  40      71           71             59       above   above     str      str
  42      75           75             63       above   above     str      str
  43      77           77             65       above   above     above    str
  44      79           79             67       above   above     above    str
  45      81           81             69       above   above     above    above
  63     117          117            105       above   above     above    above
  64     119          119            107       above   above     above    above

"One item" below: keys that share their top 9 bits (PREFIX) and are at most
4096 instances.  Keys need not be canonical (add_pairs takes any key); the
records() flavour turns keys into k-base reads, whose k-mers the engine
canonicalises, and canonical() restates that for the reference.  PREFIX starts
with three A bases, so a key under it is its own canonical form unless it ends
in TTT (and a few ties): records() keeps ~98 % of a shape where it was built,
and all of it where the builder was called with for_records (keys that end in
AAA; the shapes whose instance count is the point).
"""

from collections import Counter

import numpy as np

# The constants the shapes aim at.  Hard-coded: the tests never read kernel
# sources; a changed constant only moves a case off its edge.
L1_BITS = 9          # okm_extract.hip kL1BitsW: L1 bins of a wide key
ITEM_CAP = 4096      # okm_count.hip kCapI: instances per full-mode item
ROW = 512            # okm_count.hip kCB: an item's instances are taken in rows of 512
HOME_BITS = 12       # okm_count.hip kFullHomeBitsW: full-mode homes of a K128 item
DENSE_BITS = 11      # okm_count.hip kDenseBits: direct-address items have <= 11 remaining bits
WINDOW = 64          # okm_count.hip status_window: look-back status words per round trip
SPLIT_TARGET = ITEM_CAP * 3 // 4   # okm_engine.hip count_general: a pass aims below 3/4 of an item

M64 = (1 << 64) - 1
PREFIX = 0b000000101  # the items' L1 bin: not 0, not all-ones, bases A A A + "10 1"

EDGES = (1, 2, ROW - 1, ROW, ROW + 1, ITEM_CAP - 1, ITEM_CAP, ITEM_CAP + 1)
FILL_NS = (ITEM_CAP - 1, ITEM_CAP)
ONE_HOME_NS = (2, ROW + 1, 3000)
SPLIT_NS = (ITEM_CAP + 1, 20_000, 70_000)
M_ITEMS = (1, 2, WINDOW - 1, WINDOW, WINDOW + 1, WINDOW + 2, 2 * WINDOW, 2 * WINDOW + 1, 1 << L1_BITS)
DENSE_LOW_BITS = (8, DENSE_BITS)
# (m, n) of the alternating m_items layouts: 1 key and n instances in turn.
# 3000-instance items inside one look-back window, 1000-instance ones over
# three windows: both stay below the 70 000 keys of the largest input
ALTERNATING = ((40, 3000), (2 * WINDOW + 2, 1000))


def pass_bits(n):
    """Bits of the partition pass a part of n instances takes (count_parts'
    plan: the smallest b >= 1 that brings n >> b to the target or below)."""
    b = 1
    while (n >> b) > SPLIT_TARGET:
        b += 1
    return b


PASS_BITS = pass_bits(max(SPLIT_NS))


def fields(k):
    """name -> (low, high): the bit ranges of the table in the module docstring."""
    top = 2 * k
    rem = top - L1_BITS
    return {
        "l1": (rem, top),
        "partition": (rem - PASS_BITS, rem),
        "home": (rem - HOME_BITS, rem),
        "home_after_pass": (rem - PASS_BITS - HOME_BITS, rem - PASS_BITS),
    }


def side(lo_hi):
    low, high = lo_hi
    return "below" if high <= 64 else "above" if low >= 64 else "straddle"


def _derive_ks():
    ks = {33, 63, 64}
    for name in fields(33):
        by_side = {}
        for k in range(33, 65):
            by_side.setdefault(side(fields(k)[name]), []).append(k)
        if "below" in by_side:
            ks.add(max(by_side["below"]))
        ks.update((min(by_side["straddle"]), max(by_side["straddle"]), min(by_side["above"])))
    return tuple(sorted(ks))


KS = _derive_ks()
# a subset for the shapes that need not run at every k: both ends, one k where
# the home straddles bit 64 with no pass and one where it does after a pass
KS_SOME = (33, 37, 40, 63, 64)
KS_TWINS = tuple(k for k in KS if k >= 37)     # an item has free bits in both words
KS_RUNS = (40, 63)                              # items spanning sorted runs
KS_REPEATED_READ = (33, 42, 64)


# ---------------------------------------------------------------------------
# representation and reference
# ---------------------------------------------------------------------------

def to_pairs(ints):
    """Python ints -> (n, 2) uint64 [lo, hi]."""
    out = np.empty((len(ints), 2), dtype=np.uint64)
    out[:, 0] = np.fromiter((v & M64 for v in ints), dtype=np.uint64, count=len(ints))
    out[:, 1] = np.fromiter((v >> 64 for v in ints), dtype=np.uint64, count=len(ints))
    return out


def from_pairs(pairs):
    pairs = np.asarray(pairs, dtype=np.uint64).reshape(-1, 2)
    return [(int(h) << 64) | int(l) for l, h in pairs]


def reference(ints, weights=None):
    """(sorted distinct keys, their counts) by a Counter over Python ints."""
    c = Counter()
    if weights is None:
        c.update(ints)
    else:
        for v, w in zip(ints, weights):
            c[v] += int(w)
    keys = sorted(c)
    return keys, [c[v] for v in keys]


def _codes(ints, k):
    """(n, k) base codes (A C G T = 0 1 2 3), first base first."""
    p = to_pairs(ints)
    lo, hi = p[:, 0], p[:, 1]
    out = np.empty((len(ints), k), dtype=np.uint8)
    for j in range(k):
        s = 2 * (k - 1 - j)
        w = (hi >> np.uint64(s - 64)) if s >= 64 else (lo >> np.uint64(s))
        out[:, j] = (w & np.uint64(3)).astype(np.uint8)
    return out


def _ints_of_codes(codes):
    n, k = codes.shape
    lo = np.zeros(n, dtype=np.uint64)
    hi = np.zeros(n, dtype=np.uint64)
    for j in range(k):
        s = 2 * (k - 1 - j)
        c = codes[:, j].astype(np.uint64)
        if s >= 64:
            hi |= c << np.uint64(s - 64)
        else:
            lo |= c << np.uint64(s)
    return [(int(h) << 64) | int(l) for l, h in zip(lo, hi)]


def revcomp(ints, k):
    return _ints_of_codes(3 - _codes(ints, k)[:, ::-1])


def canonical(ints, k):
    """min(key, reverse complement) of every key."""
    return [min(v, r) for v, r in zip(ints, revcomp(ints, k))]


def records(ints, k):
    """One k-base read per key: the from-bytes flavour of a shape (the engine
    counts canonical(ints, k))."""
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    return [row.tobytes() for row in acgt[_codes(ints, k)]]


def l1_bin(v, k):
    return v >> (2 * k - L1_BITS)


# ---------------------------------------------------------------------------
# shape builders: (k, seed[, n]) -> ints (and weights where noted)
# ---------------------------------------------------------------------------

def _rng(*seed):
    return np.random.default_rng([int(s) for s in seed])


def _rand_bits(rng, n, bits):
    """n uniform Python ints below 2^bits."""
    out = [0] * n
    for at in range(0, bits, 32):
        w = min(32, bits - at)
        part = rng.integers(0, 1 << w, n, dtype=np.uint64)
        out = [o | (int(p) << at) for o, p in zip(out, part)]
    return out


rand_bits = _rand_bits


def _distinct_bits(rng, n, bits):
    """n distinct uniform ints below 2^bits (needs 2^bits >= 2n)."""
    seen, out = set(), []
    while len(out) < n:
        for v in _rand_bits(rng, 2 * (n - len(out)) + 8, bits):
            if v not in seen and len(out) < n:
                seen.add(v)
                out.append(v)
    return out


def _shuffle(rng, xs):
    return [xs[i] for i in rng.permutation(len(xs))]


def _under(prefix, k):
    return prefix << (2 * k - L1_BITS)


_A3 = 6  # three A bases


def _tail(for_records):
    """for_records: a shape's keys get six zero bits at their low end, and the
    shape's free bits start above them.  A key under PREFIX (AAA...) that ends
    in AAA is below its reverse complement (TTT...), so records() gives the
    engine exactly the keys that were built: the from-bytes flavour then has
    the same instance counts, to the key, as the pairs flavour."""
    return _A3 if for_records else 0


def one_item_repeats(k, seed, n, for_records=False):
    """n instances drawn from max(1, n // 4) keys of one L1 bin."""
    rng = _rng(1, k, seed, n)
    sh = _tail(for_records)
    rem = 2 * k - L1_BITS
    pool = [_under(PREFIX, k) | (v << sh) for v in _distinct_bits(rng, max(1, n // 4), rem - sh)]
    return [pool[i] for i in rng.integers(0, len(pool), n)]


def one_item_distinct(k, seed, n, for_records=False):
    rng = _rng(2, k, seed, n)
    sh = _tail(for_records)
    return [_under(PREFIX, k) | (v << sh) for v in _distinct_bits(rng, n, 2 * k - L1_BITS - sh)]


def one_key_fills_item(k, seed, n, for_records=False):
    """One key n times: one home holds every instance, and the last run-start
    entry (u16) is at its largest value."""
    rng = _rng(3, k, seed, n)
    sh = _tail(for_records)
    return [_under(PREFIX, k) | (_rand_bits(rng, 1, 2 * k - L1_BITS - sh)[0] << sh)] * n


def one_home(k, seed, n, for_records=False, others=300):
    """n distinct keys that agree in everything above their lowest 16 bits (22
    for_records: one full-mode home at every k, as the home field ends at bit
    2k - 21 >= 45, and after a pass still above bit 22), beside `others`
    ordinary keys of the same item."""
    rng = _rng(4, k, seed, n)
    sh = _tail(for_records)
    rem = 2 * k - L1_BITS
    stem = _under(PREFIX, k) | (_rand_bits(rng, 1, rem - 16 - sh)[0] << (16 + sh))
    crowd = [stem | (v << sh) for v in _distinct_bits(rng, n, 16)]
    rest = [_under(PREFIX, k) | (v << sh) for v in _distinct_bits(rng, others, rem - sh)]
    return _shuffle(rng, crowd + rest + rest[:50])


def last_and_first_home(k, seed, for_records=False, homes=(0, 1, (1 << HOME_BITS) - 2, (1 << HOME_BITS) - 1)):
    """Keys in the first two and the last two homes of the item only (odd and
    even homes: the counters are packed u16 pairs; the last home ends at the
    item's instance total)."""
    rng = _rng(5, k, seed)
    sh = _tail(for_records)
    rem = 2 * k - L1_BITS
    out = []
    for h in homes:
        below = _distinct_bits(rng, 40, rem - HOME_BITS - sh)
        keys = [_under(PREFIX, k) | (h << (rem - HOME_BITS)) | (v << sh) for v in below]
        out += keys + keys[:15] + keys[:5]
    return _shuffle(rng, out)


def home_of(v, k, passes=0):
    rem = 2 * k - L1_BITS - passes
    return (v >> (rem - HOME_BITS)) & ((1 << HOME_BITS) - 1)


SPECIAL_LO = (0, M64, 1 << 63, (1 << 63) - 1)


def word_twins(k, seed):
    """One item (k >= 37: free bits in both words).  Pairs of keys equal in lo
    and different in hi, pairs equal in hi and different in lo, each key 1..4
    times, beside keys whose lo is 0, ~0, 1 << 63 and (1 << 63) - 1.  Returns
    (ints, hi_twins, lo_twins): the pairs as (a, b) tuples."""
    rng = _rng(6, k, seed)
    hi_free = 2 * k - L1_BITS - 64
    assert hi_free >= 1
    hi_base = _under(PREFIX, k) >> 64

    def key(hi_low, lo):
        return ((hi_base | hi_low) << 64) | lo

    his = _distinct_bits(rng, 130, hi_free) if hi_free >= 9 else list(range(1 << hi_free))
    los = _distinct_bits(rng, 200, 64)
    hi_twins, lo_twins, ints = [], [], []
    for i in range(60):
        lo = los[i]
        a, b = his[(2 * i) % len(his)], his[(2 * i + 1) % len(his)]
        hi_twins.append((key(a, lo), key(b, lo)))
    for i in range(60):
        h = his[i % len(his)]
        lo_twins.append((key(h, los[60 + 2 * i]), key(h, los[61 + 2 * i])))
    # twins whose differing word differs in one bit only: the lowest, the highest
    lo_twins.append((key(his[0], los[190] & ~1), key(his[0], los[190] | 1)))
    lo_twins.append((key(his[1], los[191] & ~(1 << 63)), key(his[1], los[191] | (1 << 63))))
    hi_twins.append((key(0, los[192]), key(1, los[192])))
    hi_twins.append((key(0, los[193]), key(1 << (hi_free - 1), los[193])))
    for a, b in hi_twins + lo_twins:
        ints += [a] * int(rng.integers(1, 5)) + [b] * int(rng.integers(1, 5))
    for lo in SPECIAL_LO:
        for h in his[:3]:
            ints += [key(h, lo)] * int(rng.integers(1, 4))
    return _shuffle(rng, ints), hi_twins, lo_twins


def dense_item(k, seed, low_bits, n=9000, weighted=False):
    """n instances of keys that share everything above their lowest low_bits
    bits (8, or 11 = the dense limit): the part splits down to a
    direct-address item.  Returns (ints, weights or None)."""
    rng = _rng(7, k, seed, low_bits)
    rem = 2 * k - L1_BITS
    stem = _under(PREFIX, k) | (_rand_bits(rng, 1, rem - low_bits)[0] << low_bits)
    ints = [stem | int(v) for v in rng.integers(0, 1 << low_bits, n)]
    w = [int(x) for x in rng.integers(1, 1001, n)] if weighted else None
    return ints, w


def split_part(k, seed, n, skewed=False, flanks=False, for_records=False):
    """n keys of one L1 bin, uniform below it: one part of more than an item,
    so it takes a partition pass.  skewed: three tight clusters (keys that
    share their top 40 bits below the bin) hold 3/4 of the keys, so the pass's
    bins are very uneven and many are empty.  flanks: 40 keys in each of L1
    bins 0, 1, 510 and 511 too -- parts around the split one, so that key-range
    groups (which are made of whole L1 parts) have something to group
    for_records: see _tail and _bin_keys."""
    rng = _rng(8, k, seed, n, skewed)
    sh = _tail(for_records)
    rem = 2 * k - L1_BITS
    if skewed:
        ints = [_under(PREFIX, k) | (v << sh) for v in _rand_bits(rng, n - 3 * (n // 4), rem - sh)]
        for stem in _distinct_bits(rng, 3, 40):
            ints += [_under(PREFIX, k) | (stem << (rem - 40)) | (v << sh)
                     for v in _rand_bits(rng, n // 4, rem - 40 - sh)]
    else:
        ints = [_under(PREFIX, k) | (v << sh) for v in _rand_bits(rng, n, rem - sh)]
    if flanks:
        for b in (0, 1, (1 << L1_BITS) - 2, (1 << L1_BITS) - 1):
            ints += _bin_keys(k, b, _distinct_bits(rng, 40, rem - 1 - _A_TAIL), for_records)
    return _shuffle(rng, ints)


_A_TAIL = 10  # five A bases


def _bin_keys(k, b, free, for_records):
    """Keys of L1 bin b from values of rem - 11 bits.  for_records: the values
    go above ten zero bits -- a key that ends in AAAAA and does not start with
    TTTTT is its own canonical form, so records() keeps every one of them in
    its bin; else they are the key's low bits.  Either way the bit below the
    bin is 0 (bin 511's keys are not all-ones and start with TTTTG), and key 0
    is not among them."""
    keys = [_under(b, k) | (v << _A_TAIL if for_records else v) for v in free]
    return [v if v else 1 << _A_TAIL for v in keys]


def m_item_bins(m, ends_only=False):
    """The m populated L1 bins: spread over the key space with bin 0 and bin
    511 among them (m >= 2), or -- ends_only -- the lowest m // 2 and the
    highest m - m // 2 bins."""
    nb = 1 << L1_BITS
    if m == 1:
        return [PREFIX]
    if ends_only:
        return list(range(m // 2)) + list(range(nb - (m - m // 2), nb))
    return sorted({(i * (nb - 1)) // (m - 1) for i in range(m)})


def m_items(k, seed, m, alternate=0, ends_only=False, for_records=False):
    """About 50 instances (40 keys, ten of them twice) in each of exactly m L1
    bins.  alternate = n: the items are 1 key and n instances (a tenth of them
    repeats) in turn, so that an item's predecessors finish out of order.
    for_records: keys that records() leaves where they are (_bin_keys)."""
    rng = _rng(9, k, seed, m, alternate)
    rem = 2 * k - L1_BITS
    ints = []
    for i, b in enumerate(m_item_bins(m, ends_only)):
        if alternate:
            n = 1 if i % 2 == 0 else alternate
            keys = _distinct_bits(rng, n - n // 10, rem - 1 - _A_TAIL)
            keys += keys[: n // 10]
        else:
            keys = _distinct_bits(rng, 40, rem - 1 - _A_TAIL)
            keys += keys[:10]
        ints += _bin_keys(k, b, keys, for_records)
    return _shuffle(rng, ints)


def extremes(k, seed):
    """Key 0, the largest key below 4^k that is not all-ones, at k = 64 the
    keys one word away from the empty marker, each a few times, beside 300
    ordinary keys."""
    rng = _rng(10, k, seed)
    top = 1 << (2 * k)
    special = [0, top - 2, top - 1 if k < 64 else top - 3, 1, M64, 1 << 64, (1 << 64) - 2]
    if k == 64:
        special += [(M64 << 64) | 0, (M64 << 64) | (M64 - 1), (0 << 64) | M64, ((M64 >> 1) << 64) | M64,
                    (M64 << 64) | (1 << 63), ((M64 - 1) << 64) | M64]
    ints = []
    for v in special:
        assert v < top
        ints += [v] * int(rng.integers(2, 6))
    ints += _rand_bits(rng, 300, 2 * k - 1)
    return _shuffle(rng, ints), special


BIG_W = 3_000_000_000    # two instances sum past 2^32
LONE_W = 5_000_000_000   # a single weight past 2^32


def weighted(k, seed, n, big=False):
    """one_item_repeats' keys with weights in 1..1000.  big: one key gets two
    instances of weight 3e9 (their sum passes 2^32) and another a lone 5e9.
    Returns (ints, weights)."""
    rng = _rng(11, k, seed, n, big)
    ints = one_item_repeats(k, seed, n)
    w = [int(x) for x in rng.integers(1, 1001, len(ints))]
    if big:
        rem = 2 * k - L1_BITS
        a, b = (_under(PREFIX, k) | v for v in _distinct_bits(rng, 2, rem))
        ints += [a, a, b]
        w += [BIG_W, BIG_W, LONE_W]
    return ints, w


# ---------------------------------------------------------------------------
# from-bytes records
# ---------------------------------------------------------------------------

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def palindrome_records():
    """k = 64: T^32 A^32, the largest canonical key (hi = ~0, lo = 0), its own
    reverse complement; three times, beside a read that holds it mid-way."""
    p = b"T" * 32 + b"A" * 32
    return [p, p, p, b"ACG" + p + b"GTC"]


def poly_a_records(k, instances):
    """Key 0 `instances` times from one record."""
    return [b"A" * (k + instances - 1)]


def repeated_read_records(k, seed, n):
    """One 60-base-longer-than-k read n times beside 20 reads that occur once."""
    rng = _rng(12, k, seed, n)
    read = _ACGT[rng.integers(0, 4, k + 60)].tobytes()
    return [read] * n + [_ACGT[rng.integers(0, 4, k + 80)].tobytes() for _ in range(20)]


def kmers_of_records(recs, k):
    """Every window of every (upper-case ACGT) record as an int, canonical."""
    code = np.full(256, 255, np.uint8)
    for i, ch in enumerate(b"ACGT"):
        code[ch] = i
    ints = []
    for r in recs:
        c = code[np.frombuffer(r, dtype=np.uint8)]
        assert (c < 4).all()
        v = 0
        mask = (1 << (2 * k)) - 1
        for i, x in enumerate(c.tolist()):
            v = ((v << 2) | x) & mask
            if i >= k - 1:
                ints.append(v)
    return canonical(ints, k) if ints else []


def bytes_cases():
    """(name, k, records) of every from-bytes case."""
    yield "palindrome", 64, palindrome_records()
    for k in KS_SOME:
        yield f"polyA-4096[{k}]", k, poly_a_records(k, ITEM_CAP)
        yield f"polyA-4097[{k}]", k, poly_a_records(k, ITEM_CAP + 1)
    for k in KS_REPEATED_READ:
        for n in (ROW, ROW + 1):
            yield f"repeated-read-{n}[{k}]", k, repeated_read_records(k, 0, n)
