"""Inputs and expectations of the multi-GPU exchange edge tests (not a test
file: tests/test_exchange_cases.py checks on the CPU that every case has the
property its name claims; tests/test_gpu_exchange_edges.py runs them through
okm_merge_owned).

Every local table is given as exact (key, count) pairs (KmerCounter.add_pairs),
so a case decides where the slice cuts fall and which counts and key gaps
occur.  The plan of the exchange is a pure function of the tables and is
restated here in numpy:

  hist     the histogram of key >> shift, summed over ranks and tables
  bounds   owner_bounds_np(hist, P): rank r owns bins [bounds[r], bounds[r+1])
  cut      per rank, cut[j] = the number of its keys whose bin is < bounds[j]

From it follow each owner's exact table (expected_tables) and the exact bytes
every rank reports in Comm.last_bytes() (expected_bytes).  Everything is an
exact integer; seeded, numpy and Python integers only.

Cuts only fall on bin boundaries, so the tables are built in "zones": zone z
is the z-th P-th of the bins, and pops[r][z] keys of rank r lie in it.  When
every zone holds the same number of pairs over all ranks, the running total
reaches r/P of the whole exactly in the last populated bin of zone r - 1, the
bound falls between the zones, and rank r's cuts are the running sums of
pops[r].  (Nothing relies on that: every property is asserted from plan().)"""

from collections import namedtuple
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

# The constants the cases aim at.  Hard-coded: the tests never read kernel
# sources; a changed constant makes the self-check fail instead of silently
# moving a case off its edge.
PACK_PER = 4             # okm_dist.hip kPackPer: counts per thread of k_pack_counts / k_widen_counts
PACK_BLOCK = 1024        # okm_dist.hip kPackBlock: counts per workgroup
DELTA_PER = 8            # okm_dist.hip kDeltaPer: keys per thread of k_pack_deltas / k_widen_deltas
DELTA_BLOCK = 2048       # okm_dist.hip kDeltaBlock: keys per workgroup
COUNT_ESCAPE_ABOVE = 255  # okm_dist.hip k_pack_counts: a count > 255 also travels as an escape
DELTA_BITS = 40          # okm_dist.hip k_pack_deltas: a key escape when delta >> 40 is non-zero
FIRST_DELTA_AGAINST = 0  # okm_dist.hip k_pack_deltas: a slice's first key is taken against 0
HIST_BITS = 16           # okm_dist.hip merge_owned_n: bits = min(16, 2k), shift = 2k - bits
PIECE_ALIGN = 8          # okm_dist.hip piece_bytes: the knob rounded down to a multiple of 8, minimum 8

M64 = (1 << 64) - 1
LENGTHS = (0, 1, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025, 2047, 2048, 2049)
COUNT_EDGES = (1, 254, 255, 256, 257, 65535, 65536, 2**32 - 1, 2**32, 2**63)
GAPS = (1, 2**40 - 1, 2**40, 2**40 + 1, 2**41 - 1)
# the gaps of the delta cases in turn: 7 of them, so over 8-key threads the
# three that escape visit every lane
GAP_CYCLE = (1, 2**40 - 1, 2**40, 2**40 + 1, 2**41 - 1, 1, 3)
WIDE_KS = (33, 39, 40, 63)
SMALL_KS = (1, 4, 7, 8, 9)
PIECES = (8, 16, 40, 4104)

Case = namedtuple("Case", "name group k wide mode P owner_mode knobs tables more")
# tables[r] = (keys, counts) of rank r: keys strictly ascending, a uint64 array
# (k <= 32) or a list of Python ints (wide); counts a uint64 array, None in set
# mode.  more: further per-rank table lists merged under the same split
# (okm_merge_owned_n); () for okm_merge_owned.


def geometry(k):
    """(bits, shift) of the owner histogram."""
    bits = min(HIST_BITS, 2 * k)
    return bits, 2 * k - bits


def piece_of(knob):
    """The piece size the library cuts messages at for a piece_bytes knob."""
    return max(knob - knob % PIECE_ALIGN, PIECE_ALIGN)


def to_pairs(ints):
    """Python ints -> (n, 2) uint64 [lo, hi]."""
    out = np.empty((len(ints), 2), dtype=np.uint64)
    out[:, 0] = np.fromiter((v & M64 for v in ints), dtype=np.uint64, count=len(ints))
    out[:, 1] = np.fromiter((v >> 64 for v in ints), dtype=np.uint64, count=len(ints))
    return out


def from_pairs(pairs):
    pairs = np.asarray(pairs, dtype=np.uint64).reshape(-1, 2)
    return [(int(h) << 64) | int(l) for l, h in pairs]


def owner_bounds_np(hist, world):
    """Restatement of okm_dist.hip owner_bounds: cut r just past the bin where
    the running total first reaches r/world of the whole."""
    cum = np.cumsum(np.asarray(hist, dtype=np.float64))
    total = cum[-1] if len(cum) else 0.0
    b = [0]
    for r in range(1, world):
        x = int(np.searchsorted(cum, total * r / world, side="left")) + 1
        b.append(max(b[-1], min(x, len(hist))))
    b.append(len(hist))
    return b


def table_sets(case):
    return (case.tables,) + tuple(case.more)


def bins_of(case, keys):
    _, shift = geometry(case.k)
    if case.wide:
        return np.array([v >> shift for v in keys], dtype=np.int64)
    return (np.asarray(keys, dtype=np.uint64) >> np.uint64(shift)).astype(np.int64)


def _plan(case):
    bits, shift = geometry(case.k)
    nb = 1 << bits
    hist = np.zeros(nb, dtype=np.uint64)
    bins = [[bins_of(case, keys) for keys, _ in ts] for ts in table_sets(case)]
    for per_rank in bins:
        for b in per_rank:
            hist += np.bincount(b, minlength=nb).astype(np.uint64)
    bounds = owner_bounds_np(hist, case.P)
    cuts = [[[int(np.searchsorted(b, x, side="left")) for x in bounds] for b in per_rank] for per_rank in bins]
    return SimpleNamespace(bits=bits, shift=shift, nb=nb, hist=hist, bounds=bounds, cuts=cuts)


_plans = {}


def plan(case):
    """The restated owner split: bits, shift, nb, hist, bounds and
    cuts[table][rank] = cut[0..P]."""
    if case.name not in _plans:
        _plans[case.name] = _plan(case)
    return _plans[case.name]


def slice_of(case, t, r, j):
    """(keys, counts) rank r sends to owner j from table t."""
    c = plan(case).cuts[t][r]
    keys, counts = table_sets(case)[t][r]
    return keys[c[j]:c[j + 1]], None if counts is None else counts[c[j]:c[j + 1]]


def expected_tables(case, t=0):
    """Each owner's table: the union of all ranks' pairs in its bin range,
    counts summed (keys only in set mode: counts None)."""
    out = []
    for j in range(case.P):
        parts = [slice_of(case, t, r, j) for r in range(case.P)]
        if case.wide:
            acc = {}
            for keys, counts in parts:
                for i, v in enumerate(keys):
                    acc[v] = acc.get(v, 0) + (1 if counts is None else int(counts[i]))
            ks = sorted(acc)
            out.append((ks, None if case.mode == "set" else np.array([acc[v] for v in ks], dtype=np.uint64)))
        else:
            allk = np.concatenate([np.asarray(k, dtype=np.uint64) for k, _ in parts])
            ks, inv = np.unique(allk, return_inverse=True)
            if case.mode == "set":
                out.append((ks, None))
            else:
                cs = np.zeros(len(ks), dtype=np.uint64)
                np.add.at(cs, inv, np.concatenate([c for _, c in parts]))
                out.append((ks, cs))
    return out


def deltas_of(keys):
    """The deltas of one slice of one-word keys: the first against 0."""
    keys = np.asarray(keys, dtype=np.uint64)
    return np.diff(np.concatenate([np.array([FIRST_DELTA_AGAINST], np.uint64), keys]))


def count_escapes(counts):
    return 0 if counts is None else int((np.asarray(counts, dtype=np.uint64) > np.uint64(COUNT_ESCAPE_ABOVE)).sum())


def key_escapes(keys):
    return int((deltas_of(keys) >> np.uint64(DELTA_BITS) != 0).sum())


def traffic(case, deltas):
    """bytes[a][b] rank a sends to rank b (a == b included), over all tables:
    pairs * (kb + c) + 16 * count_escapes * c + 16 * key_escapes * d
    (okm_dist.hip move_and_merge)."""
    d = 1 if deltas and not case.wide else 0
    kb = 16 if case.wide else 5 if d else 8
    c = 0 if case.mode == "set" else 1
    out = [[0] * case.P for _ in range(case.P)]
    for t in range(len(table_sets(case))):
        for a in range(case.P):
            for b in range(case.P):
                keys, counts = slice_of(case, t, a, b)
                out[a][b] += len(keys) * (kb + c) + 16 * count_escapes(counts) * c
                if d:
                    out[a][b] += 16 * key_escapes(keys)
    return out


def expected_bytes(case, deltas):
    """[(sent, received)] per rank, as Comm.last_bytes() reports them: the
    traffic to and from the OTHER ranks, in either owner mode."""
    tr = traffic(case, deltas)
    P = case.P
    return [(sum(tr[me][r] for r in range(P) if r != me), sum(tr[r][me] for r in range(P) if r != me))
            for me in range(P)]


def messages(case, deltas):
    """Every point-to-point message of the exchange: (kind, sender, dest,
    element bytes, elements).  The own slice crosses the transport only with
    owner_mode = "local"."""
    d = bool(deltas) and not case.wide
    out = []
    for t in range(len(table_sets(case))):
        for a in range(case.P):
            for b in range(case.P):
                if a == b and case.owner_mode == "separate":
                    continue
                keys, counts = slice_of(case, t, a, b)
                n = len(keys)
                if d:
                    out.append(("keys5", a, b, 1, 5 * n))
                    out.append(("key_escapes", a, b, 8, 2 * key_escapes(keys)))
                else:
                    out.append(("keys", a, b, 8, (2 if case.wide else 1) * n))
                if case.mode != "set":
                    out.append(("count_bytes", a, b, 1, n))
                    out.append(("count_escapes", a, b, 8, 2 * count_escapes(counts)))
    return [m for m in out if m[4]]


# ---------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------

def _rand_bits(rng, bits):
    v = 0
    for at in range(0, bits, 32):
        v |= int(rng.integers(0, 1 << min(32, bits - at))) << at
    return v


def zone_of(k, P, key):
    bits, shift = geometry(k)
    return min((key >> shift) // ((1 << bits) // P), P - 1)


def zone_key(k, P, z, bin_in_zone, low):
    """A key in bin (first bin of zone z) + bin_in_zone with the given low bits."""
    bits, shift = geometry(k)
    return ((z * ((1 << bits) // P) + bin_in_zone) << shift) | low


def zone_tables(k, pops, seed, forced=(), zone_bins=4):
    """Sorted key lists (Python ints), rank r with pops[r][z] keys in zone z.
    The keys of a zone are drawn from one pool over zone_bins of its bins, so
    ranks share some keys and keys share bins; forced = [(rank, key)] are
    part of rank's table (and of its pops), and of no pool."""
    R, P = len(pops), len(pops[0])
    bits, shift = geometry(k)
    W = (1 << bits) // P
    assert W >= zone_bins and shift >= 16
    rng = np.random.default_rng(seed)
    top = (1 << (2 * k)) - 1  # all T: never canonical
    banned = {key for _, key in forced} | {top}
    tables = [set() for _ in range(R)]
    for z in range(P):
        need = max(pops[r][z] for r in range(R))
        bins = sorted(int(b) for b in z * W + rng.choice(W, size=zone_bins, replace=False))
        pool = set()
        while len(pool) < need + need // 2 + 4:
            v = (bins[int(rng.integers(len(bins)))] << shift) | _rand_bits(rng, shift)
            if v not in banned:
                pool.add(v)
        pool = sorted(pool)
        for r in range(R):
            mine = [key for rr, key in forced if rr == r and zone_of(k, P, key) == z]
            m = pops[r][z] - len(mine)
            assert m >= 0, "more forced keys than the zone's population"
            pick = rng.choice(len(pool), size=m, replace=False)
            tables[r] |= {pool[int(i)] for i in pick} | set(mine)
    out = [sorted(t) for t in tables]
    assert [len(t) for t in out] == [sum(p) for p in pops]
    return out


def fill(fixed, P, T=None, pad=6):
    """A P x P population matrix with the given rows, the others sharing what
    is left of every column so that each column sums to T (an int, or one per
    column; default: the largest fixed column sum + pad)."""
    free = [r for r in range(P) if r not in fixed]
    assert free
    col = [sum(row[z] for row in fixed.values()) for z in range(P)]
    if T is None:
        T = max(col) + pad
    Ts = [T] * P if isinstance(T, int) else list(T)
    pops = [[0] * P for _ in range(P)]
    for r, row in fixed.items():
        pops[r] = list(row)
    for z in range(P):
        rem = Ts[z] - col[z]
        assert rem >= 0
        for i, r in enumerate(free):
            pops[r][z] = rem // len(free) + (1 if i < rem % len(free) else 0)
    return pops


def offdiag(P, sizes, pad=2):
    """pops with pops[a][b] = sizes[(a, b)] off the diagonal and the diagonal
    making every column sum equal."""
    pops = [[0] * P for _ in range(P)]
    for (a, b), n in sizes.items():
        pops[a][b] = n
    T = max(sum(pops[a][z] for a in range(P)) for z in range(P)) + pad
    for z in range(P):
        pops[z][z] = T - sum(pops[a][z] for a in range(P))
    return pops


def small_counts(rng, n, escape_every=0):
    """Counts 1 ... 255 (254 and 255 among them), every escape_every-th above."""
    c = rng.choice(np.array([1, 2, 3, 17, 254, 255], dtype=np.uint64), size=n)
    if escape_every and n:
        at = np.arange(int(rng.integers(escape_every)), n, escape_every)
        c[at] = rng.choice(np.array([256, 257, 300, 65536], dtype=np.uint64), size=len(at))
    return c.astype(np.uint64)


def make_case(name, group, k, key_lists, counts, mode="count", owner_mode="separate", knobs=None, more=()):
    wide = k > 32
    P = len(key_lists)

    def table(keys, cnt):
        keys = list(keys) if wide else np.array(keys, dtype=np.uint64)
        return keys, None if mode == "set" or cnt is None else np.asarray(cnt, dtype=np.uint64)

    tables = tuple(table(kl, None if counts is None else counts[r]) for r, kl in enumerate(key_lists))
    more = tuple(tuple(table(kl, cs) for kl, cs in ts) for ts in more)
    return Case(name, group, k, wide, mode, P, owner_mode, dict(knobs or {}), tables, more)


def as_set(case):
    strip = lambda ts: tuple((k, None) for k, _ in ts)
    return case._replace(name=case.name + "_set", group="set", mode="set", tables=strip(case.tables))


def zoned_case(name, group, k, pops, seed, escape_every=5, **kw):
    rng = np.random.default_rng(seed + 1000)
    keys = zone_tables(k, pops, seed, forced=kw.pop("forced", ()))
    counts = [small_counts(rng, len(t), escape_every) for t in keys]
    return make_case(name, group, k, keys, counts, **kw)


# ---------------------------------------------------------------------------
# the groups
# ---------------------------------------------------------------------------

def _lengths():
    """1: rank 0's table has n keys; its tail lies in the slice it sends."""
    out = []
    for n in LENGTHS:
        a = n // 3
        T = n + 6
        out.append(zoned_case(f"len{n}", "lengths", 31, [[a, n - a], [T - a, T - (n - a)]], 100 + n, escape_every=3))
    return out


def _cuts():
    """2: rank 0's cut between its two sent slices at every residue, and on
    the block boundaries of both packers."""
    out = []
    for res in range(1, 8):
        out.append(zoned_case(f"cut{res}", "cuts", 31, fill({0: [3, 37 + res, 13]}, 3), 200 + res))
    out.append(zoned_case("cut1024", "cuts", 31, fill({0: [5, PACK_BLOCK - 5, 9]}, 3), 210))
    out.append(zoned_case("cut2048", "cuts", 31, fill({0: [5, DELTA_BLOCK - 5, 9]}, 3), 211))
    return out


def _empties():
    """3: empty slices, owners of nothing, empty tables."""
    out = [zoned_case("empty_first", "empties", 31, fill({0: [0, 11, 13]}, 3), 300),
           zoned_case("empty_middle", "empties", 31, fill({0: [11, 0, 13]}, 3), 301),
           zoned_case("empty_last", "empties", 31, fill({0: [11, 13, 0]}, 3), 302),
           zoned_case("empty_two_middle_p8", "empties", 31, fill({0: [5, 7, 0, 0, 9, 4, 6, 3]}, 8, T=37), 303)]
    # k = 1: four bins for eight ranks
    rng = np.random.default_rng(304)
    keys = [sorted({r % 4, (r + 1) % 4}) if r != 5 else [] for r in range(8)]
    out.append(make_case("k1_p8", "empties", 1, keys, [small_counts(rng, len(t), 2) for t in keys]))
    out.append(make_case("all_empty", "empties", 31, [[], [], []], [np.zeros(0, np.uint64)] * 3))
    out.append(make_case("one_key", "empties", 31, [[], [zone_key(31, 3, 1, 5, 12345)], []],
                         [np.zeros(0, np.uint64), np.array([300], np.uint64), np.zeros(0, np.uint64)]))
    return out


OWN_ROWS = {"own_empty": [9, 0, 12], "own_whole": [0, 50, 0], "own_blocks": [1021, 3200, 11],
            "own_in_thread": [17, 3, 20]}


def _own():
    """4: rank 1's own (middle) slice, borrowed by a separate owner or sent to
    itself by owner == local."""
    out = []
    for i, (name, row) in enumerate(OWN_ROWS.items()):
        for mode in ("separate", "local"):
            out.append(zoned_case(f"{name}_{mode}", "own", 31, fill({1: row}, 3), 400 + i, owner_mode=mode))
    return out


def _counts():
    """5: count bytes and escapes.  Slices (sender -> owner): 2 -> 0 has no
    escape, 0 -> 2 exactly one (2^63, a key of rank 0 alone), 1 -> 0 three
    hundred, 1 -> 2 one at its first and one at its last position, 2 -> 1
    every edge value; one key of zone 1 is held by every rank."""
    k, P = 31, 3
    pops = fill({0: [20, 30, 25], 1: [320, 15, 40]}, P, T=400)
    lone = zone_key(k, P, 2, 7, 12345)
    everyone = zone_key(k, P, 1, 9, 777)
    forced = [(0, lone)] + [(r, everyone) for r in range(P)]
    out = []
    for name, shares in (("counts_sum_u32max", (2**31, 2**31 - 2, 1)), ("counts_sum_2p32", (2**31, 2**31 - 1, 1))):
        keys = zone_tables(k, pops, 500, forced=forced)
        rng = np.random.default_rng(501)
        counts = [small_counts(rng, len(t)) for t in keys]
        c0 = np.cumsum([0] + pops[0])
        c1 = np.cumsum([0] + pops[1])
        c2 = np.cumsum([0] + pops[2])
        counts[0][keys[0].index(lone)] = 2**63
        counts[1][c1[0]:c1[0] + 300] = rng.choice(np.array(COUNT_EDGES[3:9], dtype=np.uint64), size=300)
        counts[1][c1[2]] = 256
        counts[1][c1[3] - 1] = 2**32
        edges = np.array(COUNT_EDGES[:9], dtype=np.uint64)
        counts[2][c2[1]:c2[2]] = edges[np.arange(pops[2][1]) % len(edges)]
        for r in range(P):
            counts[r][keys[r].index(everyone)] = shares[r]
        assert c0[-1] == len(keys[0])
        out.append(make_case(name, "counts", k, keys, counts))
    return out


def _gap_run(start, n, at=0):
    """n keys from start on with the gaps of GAP_CYCLE in turn (from gap at)."""
    keys = [start]
    for i in range(n - 1):
        keys.append(keys[-1] + GAP_CYCLE[(at + i) % len(GAP_CYCLE)])
    return keys


def _deltas():
    """6: key gaps around 2^40 (P = 2: zone 1 is the upper half of the keys)."""
    out = []
    for k in (31, 32):
        half = 1 << (2 * k - 1)
        r0 = [5, 9, 2**40 + 77, 2**41, 2**42, 2**43, 2**44, 2**45, 2**45 + 1] + _gap_run(half + 2**41, 63)
        r1 = _gap_run(0, 63, at=3) + [half + 100 + 3 * i for i in range(9)]
        rng = np.random.default_rng(600 + k)
        counts = [small_counts(rng, len(r0), 6), small_counts(rng, len(r1), 6)]
        for mode in ("separate", "local"):
            out.append(make_case(f"gaps_k{k}_{mode}", "deltas", k, [r0, r1], counts, owner_mode=mode))
    # k = 32: most pairs lie in the top bin, so owner 0's range is every bin
    # and rank 1 sends small keys and top-bin keys in ONE slice
    top = 0xFFFF << 48
    r0 = [7] + [top + 1000 * i + 1 for i in range(40)]
    r1 = [0, 3, 2**40 + 5] + [top + 1000 * i + 500 for i in range(40)]
    rng = np.random.default_rng(640)
    out.append(make_case("k32_top_after_small", "deltas", 32, [r0, r1],
                         [small_counts(rng, len(r0), 6), small_counts(rng, len(r1), 6)]))
    return out


def _hi_family(k):
    """Keys equal in lo that differ in hi."""
    hmax = (1 << (2 * k - 64)) - 1
    his = sorted(h for h in {0, 1, 2, hmax // 3, hmax // 2 + 1, hmax - 1} if h <= hmax)
    lo = 0x2000_1234_5678_9ABC
    return [(h << 64) | lo for h in his if (h << 64) | lo != (1 << (2 * k)) - 1]


def _wide():
    """8: K128 keys, always two u64 words on the wire.  Counts as in group 5:
    rank 1 holds every edge value, rank 0 sends an escape at the first
    position of its slice for owner 1 and at the last of its slice for owner
    2, 2^63 on a key of its own, and one key of zone 1 is held by every rank
    (sums 2^32 - 1 at k = 33 and 40, 2^32 at k = 39 and 63)."""
    out = []
    edges = np.array(COUNT_EDGES[:9], dtype=np.uint64)
    pops = fill({0: [20, 30, 25]}, 3, T=90)
    for k in WIDE_KS:
        fam = _hi_family(k)
        lone = zone_key(k, 3, 2, 7, 12345)
        everyone = zone_key(k, 3, 1, 9, 777)
        forced = [(0, v) for v in fam] + [(2, v) for v in fam] + [(0, lone)] + [(r, everyone) for r in range(3)]
        shares = (2**31, 2**31 - 2, 1) if k in (33, 40) else (2**31, 2**31 - 1, 1)
        for mode in ("separate", "local") if k == 39 else ("separate",):
            keys = zone_tables(k, pops, 800 + k, forced=forced)
            rng = np.random.default_rng(850 + k)
            counts = [small_counts(rng, len(t)) for t in keys]
            counts[1][:] = rng.choice(edges, size=len(counts[1]))
            c0 = np.cumsum([0] + pops[0])
            counts[0][c0[1]] = 256          # first position of rank 0's slice for owner 1
            counts[0][c0[3] - 1] = 2**32    # last position of its slice for owner 2
            counts[0][keys[0].index(lone)] = 2**63
            for r in range(3):
                counts[r][keys[r].index(everyone)] = shares[r]
            out.append(make_case(f"wide{k}_{mode}", "wide", k, keys, counts, owner_mode=mode))
    return out


def _small_k():
    """9: dense tables: every key below 4^k on every rank."""
    out = []
    for k in SMALL_KS:
        P = 3 if k == 8 else 2
        n = 4**k
        keys = [np.arange(n, dtype=np.uint64) for _ in range(P)]
        counts = [((np.arange(n, dtype=np.uint64) * np.uint64(7 + r)) % np.uint64(300 if r == 0 else 5)) + np.uint64(1)
                  for r in range(P)]
        out.append(make_case(f"dense_k{k}", "small_k", k, keys, counts))
    return out


PIECE_SIZES = {
    # slice sizes (sender, owner): count-byte messages of m * piece, + 1, - 1
    8: {(0, 1): 16, (0, 2): 17, (1, 0): 15, (1, 2): 8, (2, 0): 24, (2, 1): 9},
    16: {(0, 1): 32, (0, 2): 33, (1, 0): 31, (1, 2): 16, (2, 0): 48, (2, 1): 17},
    40: {(0, 1): 80, (0, 2): 81, (1, 0): 79, (1, 2): 40, (2, 0): 8, (2, 1): 120},
    # u64 key messages of 513 words = one piece, + 1, and two pieces - 1; 900 five-byte keys
    # and 310 escape pairs pass the first piece
    4104: {(0, 1): 513, (0, 2): 514, (1, 0): 1025, (1, 2): 900, (2, 0): 30, (2, 1): 320},
}


def _pieces():
    """10: messages cut into pieces (knob piece_bytes)."""
    out = []
    for piece, sizes in PIECE_SIZES.items():
        pops = offdiag(3, sizes)
        for k in (31, 40):
            keys = zone_tables(k, pops, 1000 + piece + k)
            rng = np.random.default_rng(1100 + piece + k)
            counts = [small_counts(rng, len(t), 4) for t in keys]
            if piece == 4104:
                c2 = np.cumsum([0] + pops[2])
                counts[2][c2[1]:c2[1] + 310] = 1000  # (2 -> 1: past the 256 escape pairs of one piece)
            out.append(make_case(f"piece{piece}_k{k}", "pieces", k, keys, counts, knobs={"piece_bytes": piece}))
    return out


def _two_tables():
    """11: okm_merge_owned_n: table B is empty on rank 1 and lies wholly in
    owner 1's range; table A spreads over all owners."""
    k, P = 31, 3
    b_pops = [[0, 12, 0], [0, 0, 0], [0, 18, 0]]
    a_pops = fill({0: [20, 30, 25]}, P, T=[90, 60, 90])
    a = zone_tables(k, a_pops, 1200)
    b = zone_tables(k, b_pops, 1201)
    rng = np.random.default_rng(1202)
    return [make_case("two_tables", "two_tables", k, a, [small_counts(rng, len(t), 4) for t in a],
                      more=(tuple((t, small_counts(rng, len(t), 3)) for t in b),))]


def _single_rank():
    """One rank with owner == local (the general path, a self send/recv):
    groups 1, 5, 6, 10 and a wide table at P = 1, cut = [0, n]."""
    out = []
    for n in LENGTHS:
        out.append(zoned_case(f"one_len{n}", "single", 31, [[n]], 1300 + n, escape_every=3, owner_mode="local"))
    rng = np.random.default_rng(1400)
    keys = zone_tables(31, [[700]], 1401)
    counts = small_counts(rng, 700)
    edges = np.array(COUNT_EDGES, dtype=np.uint64)
    counts[:300] = edges[np.arange(300) % len(edges)]
    counts[-1] = 2**63
    out.append(make_case("one_counts", "single", 31, keys, [counts], owner_mode="local"))
    for k in (31, 32):
        keys = _gap_run(0, 70) + _gap_run((1 << (2 * k - 1)) + 2**41, 70, at=2)
        if k == 32:
            keys += [(0xFFFF << 48) + 9 * i for i in range(20)]
        out.append(make_case(f"one_gaps_k{k}", "single", k, [keys], [small_counts(rng, len(keys), 6)],
                             owner_mode="local"))
    for piece in PIECES:
        n = 900 if piece == 4104 else 33
        keys = zone_tables(31, [[n]], 1500 + piece)
        counts = small_counts(rng, n, 4)
        if piece == 4104:
            counts[100:410] = 1000
        out.append(make_case(f"one_piece{piece}", "single", 31, keys, [counts], owner_mode="local",
                             knobs={"piece_bytes": piece}))
    keys = zone_tables(39, [[100]], 1600, forced=[(0, v) for v in _hi_family(39)])
    out.append(make_case("one_wide39", "single", 39, keys, [small_counts(rng, 100, 4)], owner_mode="local",
                         knobs={"piece_bytes": 40}))
    return out


SET_GROUPS = ("lengths", "cuts", "empties", "own", "deltas")   # 7: groups 1 to 4 and 6 without counts
AUTO_FORMAT = ("len1025", "dense_k7", "empty_two_middle_p8")   # 12: no wire_deltas knob


@lru_cache(maxsize=None)
def all_cases():
    cases = _lengths() + _cuts() + _empties() + _own() + _counts() + _deltas()
    cases += [as_set(c) for c in cases if c.group in SET_GROUPS]
    cases += _wide() + _small_k() + _pieces() + _two_tables() + _single_rank()
    by = {c.name: c for c in cases}
    assert len(by) == len(cases)
    return by


def get(name):
    return all_cases()[name]


def names(*groups, ranks=None):
    """Case names of the groups (all but "single" by default), in order."""
    return [c.name for c in all_cases().values()
            if (c.group in groups if groups else c.group != "single") and (ranks is None or c.P == ranks)]
