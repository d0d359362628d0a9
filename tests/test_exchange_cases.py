"""CPU side of the exchange edge tests: the inputs of tests/exchange_cases.py
really have the properties their names claim, asserted from the restated plan
(plan()), so a changed constant or split rule fails here instead of silently
moving a case off its edge; and the restated owner split equals the library's
host code (okm_owner_bounds) on the cases' own histograms."""

import numpy as np
import pytest

import exchange_cases as ec
import okm

ALL = ec.all_cases()


def group(*names):
    return [c for c in ALL.values() if c.group in names]


def cut(case, r, t=0):
    return ec.plan(case).cuts[t][r]


def sent(case, a, b):
    """Does rank a's slice for owner b pass through the pack kernels' output?"""
    return a != b or case.owner_mode == "local"


def sent_slices(case, t=0):
    for a in range(case.P):
        for b in range(case.P):
            if sent(case, a, b):
                keys, counts = ec.slice_of(case, t, a, b)
                yield a, b, keys, counts


# ---------------------------------------------------------------------------
# the restatement itself
# ---------------------------------------------------------------------------

def test_constants():
    assert ec.PACK_BLOCK == 256 * ec.PACK_PER and ec.DELTA_BLOCK == 256 * ec.DELTA_PER
    assert [ec.geometry(k) for k in (1, 4, 7, 8, 9, 31, 32)] == [(2, 0), (8, 0), (14, 0), (16, 0), (16, 2), (16, 46),
                                                               (16, 48)]
    assert [ec.geometry(k)[1] for k in ec.WIDE_KS] == [50, 62, 64, 110]
    assert [ec.piece_of(v) for v in (8, 15, 16, 40, 4104, 4111)] == [8, 8, 16, 40, 4104, 4104]


@pytest.mark.parametrize("name", list(ALL))
def test_tables_are_valid_and_the_split_is_the_librarys(name):
    case = ALL[name]
    p = ec.plan(case)
    assert case.wide == (case.k > 32) and case.owner_mode in ("separate", "local") and case.mode in ("count", "set")
    for ts in ec.table_sets(case):
        assert len(ts) == case.P
        for keys, counts in ts:
            ints = [int(v) for v in keys]
            assert all(a < b for a, b in zip(ints, ints[1:]))  # strictly ascending
            assert not ints or (0 <= ints[0] and ints[-1] < (1 << (2 * case.k)))
            assert (1 << (2 * case.k)) - 1 not in ints or case.k <= 9  # all T only in the dense tables
            assert (counts is None) == (case.mode == "set")
            if counts is not None:
                assert counts.dtype == np.uint64 and len(counts) == len(ints) and (counts > 0).all()
    assert p.nb == len(p.hist) and int(p.hist.sum()) == sum(len(k) for ts in ec.table_sets(case) for k, _ in ts)
    assert okm.owner_bounds(p.hist, case.P) == p.bounds
    for per_rank, ts in zip(p.cuts, ec.table_sets(case)):
        for c, (keys, _) in zip(per_rank, ts):
            assert c[0] == 0 and c[-1] == len(keys) and all(a <= b for a, b in zip(c, c[1:]))
            b = ec.bins_of(case, keys)
            for j in range(case.P):  # cuts fall on bin boundaries: slice j holds owner j's bins
                assert all(p.bounds[j] <= x < p.bounds[j + 1] for x in b[c[j]:c[j + 1]])


@pytest.mark.parametrize("name", list(ALL))
def test_expectations_are_consistent(name):
    """The owners' ranges are the sorted global table with summed counts (by
    Python integers, so a u64 wrap in the numpy sum would show), and the bytes
    sent equal the bytes received."""
    case = ALL[name]
    for t, ts in enumerate(ec.table_sets(case)):
        want = {}
        for keys, counts in ts:
            for i, v in enumerate(keys):
                want[int(v)] = want.get(int(v), 0) + (1 if counts is None else int(counts[i]))
        assert not want or max(want.values()) < 1 << 64
        got_k, got_c = [], []
        for keys, counts in ec.expected_tables(case, t):
            got_k += [int(v) for v in keys]
            got_c += [1] * len(keys) if counts is None else [int(c) for c in counts]
        assert got_k == sorted(want)
        if case.mode == "count":
            assert got_c == [want[v] for v in got_k]
    for deltas in (0, 1):
        by = ec.expected_bytes(case, deltas)
        assert sum(s for s, _ in by) == sum(r for _, r in by)
    if case.wide:
        assert ec.expected_bytes(case, 1) == ec.expected_bytes(case, 0)
    if case.P == 1:
        assert ec.expected_bytes(case, 1) == [(0, 0)]


def test_expected_bytes_formula():
    case = ALL["counts_sum_2p32"]
    keys, counts = ec.slice_of(case, 0, 1, 0)
    assert len(keys) == 320 and ec.count_escapes(counts) == 300
    assert ec.traffic(case, 0)[1][0] == 320 * 9 + 16 * 300
    assert ec.traffic(case, 1)[1][0] == 320 * 6 + 16 * 300 + 16 * ec.key_escapes(keys)
    s = ec.as_set(case)
    assert ec.traffic(s, 0)[1][0] == 320 * 8 and ec.traffic(s, 1)[1][0] == 320 * 5 + 16 * ec.key_escapes(keys)
    assert ec.deltas_of(np.array([5, 6, 2**40 + 6], np.uint64)).tolist() == [5, 1, 2**40]
    assert ec.key_escapes(np.array([5, 6, 2**40 + 6, 2**41 + 5], np.uint64)) == 1
    assert ec.key_escapes(np.array([2**40], np.uint64)) == 1 and ec.key_escapes(np.array([2**40 - 1], np.uint64)) == 0
    w = ALL["wide40_separate"]
    n = len(ec.slice_of(w, 0, 0, 1)[0])
    assert ec.traffic(w, 1)[0][1] == n * 17 + 16 * ec.count_escapes(ec.slice_of(w, 0, 0, 1)[1])


# ---------------------------------------------------------------------------
# the groups
# ---------------------------------------------------------------------------

def test_1_table_lengths():
    cases = group("lengths")
    assert tuple(len(c.tables[0][0]) for c in cases) == ec.LENGTHS
    assert ec.LENGTHS == (0, 1, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025, 2047, 2048, 2049)
    for c in cases:
        n = len(c.tables[0][0])
        assert c.P == 2 and not c.wide and c.owner_mode == "separate"
        assert n == 0 or cut(c, 0)[1] < n  # the table's tail is in the slice rank 0 sends
        assert len(c.tables[1][0]) > 0 and cut(c, 1)[1] > 0  # rank 1 sends too
    assert any(ec.count_escapes(ec.slice_of(c, 0, 0, 1)[1]) for c in cases)


def test_2_cut_residues():
    cases = group("cuts")
    ends, starts = set(), set()
    for c in cases:
        for r in range(c.P):
            cu = cut(c, r)
            for j in range(c.P):
                if sent(c, r, j) and cu[j + 1] > cu[j]:
                    starts.add(cu[j])
                    ends.add(cu[j + 1])
    both = ends & starts  # a cut that ends one sent slice and starts the next
    for per in (ec.DELTA_PER, ec.PACK_PER):
        assert {x % per for x in both} >= set(range(1, per))
        assert {x % per for x in ends} >= set(range(1, per)) and {x % per for x in starts} >= set(range(1, per))
    assert any(x % ec.DELTA_BLOCK == ec.PACK_BLOCK for x in both)  # on a 1024 boundary that is no 2048 boundary
    assert any(x and x % ec.DELTA_BLOCK == 0 for x in both)


def test_3_empty_slices():
    def widths(name, r=0):
        cu = cut(ALL[name], r)
        return [b - a for a, b in zip(cu, cu[1:])]

    w = widths("empty_first")
    assert w[0] == 0 and w[1] > 0 and w[2] > 0
    w = widths("empty_middle")
    assert w[0] > 0 and w[1] == 0 and w[2] > 0
    w = widths("empty_last")
    assert w[0] > 0 and w[1] > 0 and w[2] == 0
    c = ALL["empty_two_middle_p8"]
    w = widths(c.name)
    assert c.P == 8 and any(w[j] == 0 and w[j + 1] == 0 and min(w[:j]) > 0 and min(w[j + 2:]) > 0 for j in range(1, 6))
    # a thread's 8 keys span the two empty slices
    j = w.index(0)
    assert cut(c, 0)[j] // ec.DELTA_PER == (cut(c, 0)[j + 2]) // ec.DELTA_PER and cut(c, 0)[j] % ec.DELTA_PER
    c = ALL["k1_p8"]
    p = ec.plan(c)
    assert c.k == 1 and c.P == 8 and p.nb == 4 and p.shift == 0
    assert len(set(p.bounds)) < len(p.bounds)  # the bounds repeat
    assert sum(1 for j in range(8) if p.bounds[j] == p.bounds[j + 1]) >= 4  # several owners own nothing
    assert any(len(k) == 0 for k, _ in c.tables)
    c = ALL["all_empty"]
    assert c.P == 3 and all(len(k) == 0 for k, _ in c.tables) and int(ec.plan(c).hist.sum()) == 0
    c = ALL["one_key"]
    assert sorted(len(k) for k, _ in c.tables) == [0, 0, 1]
    owners = [j for j in range(3) if len(ec.expected_tables(c)[j][0])]
    assert len(owners) == 1 and ec.count_escapes(c.tables[1][1]) == 1


def test_4_own_slice():
    for name in ec.OWN_ROWS:
        sep, loc = ALL[name + "_separate"], ALL[name + "_local"]
        assert sep.owner_mode == "separate" and loc.owner_mode == "local" and sep.P == 3
        for (ka, ca), (kb, cb) in zip(sep.tables, loc.tables):  # the same tables
            assert np.array_equal(ka, kb) and np.array_equal(ca, cb)
    c0, c1 = cut(ALL["own_empty_separate"], 1)[1:3]
    assert c0 == c1 and 0 < c0 < len(ALL["own_empty_separate"].tables[1][0])
    c = ALL["own_whole_separate"]
    assert cut(c, 1)[1:3] == [0, len(c.tables[1][0])] and len(c.tables[1][0]) > 0
    assert ec.expected_bytes(c, 0)[1][0] == 0 and ec.expected_bytes(c, 0)[1][1] > 0  # peers still send to it
    s0, s1 = cut(ALL["own_blocks_separate"], 1)[1:3]
    n = len(ALL["own_blocks_separate"].tables[1][0])
    for block, per in ((ec.PACK_BLOCK, ec.PACK_PER), (ec.DELTA_BLOCK, ec.DELTA_PER)):
        assert s0 % per and s1 % per and s0 % block and s1 % block
        first = -(-s0 // block) * block
        assert first + block <= s1  # a whole block inside the own slice
        assert s0 // block < first // block and s1 < n and s1 // block == (n - 1) // block  # sent keys beside it
    s0, s1 = cut(ALL["own_in_thread_separate"], 1)[1:3]
    assert s0 < s1 and s0 // ec.DELTA_PER == (s1 - 1) // ec.DELTA_PER and s0 % ec.DELTA_PER and s1 % ec.DELTA_PER


def test_5_count_bytes():
    cases = group("counts")
    assert ec.COUNT_EDGES == (1, 254, 255, 256, 257, 65535, 65536, 2**32 - 1, 2**32, 2**63)
    sums = set()
    for c in cases:
        seen, n_esc = set(), set()
        first = last = False
        for a, b, keys, counts in sent_slices(c):
            seen |= set(counts.tolist())
            n_esc.add(ec.count_escapes(counts))
            if len(counts):
                first |= int(counts[0]) > 255 and ec.count_escapes(counts) < len(counts)
                last |= int(counts[-1]) > 255 and ec.count_escapes(counts) < len(counts)
        assert seen >= set(ec.COUNT_EDGES)
        assert {0, 1} <= n_esc and any(200 <= x <= 400 for x in n_esc)
        assert first and last
        # one key held by every rank
        common = set(c.tables[0][0].tolist())
        for keys, _ in c.tables[1:]:
            common &= set(keys.tolist())
        tot = {v: sum(int(cs[np.searchsorted(ks, np.uint64(v))]) for ks, cs in c.tables) for v in common}
        sums |= set(tot.values())
    assert 2**32 - 1 in sums and 2**32 in sums  # the owner's u32-staged weighted count and its u64 redo


def test_6_key_deltas():
    cases = group("deltas")
    assert {c.k for c in cases} == {31, 32}
    assert ec.GAPS == (1, 2**40 - 1, 2**40, 2**40 + 1, 2**41 - 1)
    for k in (31, 32):
        gaps, lanes = set(), set()
        first_small = first_big = zero_first = False
        for c in cases:
            if c.k != k:
                continue
            for a, b, keys, _ in sent_slices(c):
                if not len(keys):
                    continue
                d = ec.deltas_of(keys)
                gaps |= set(d[1:].tolist())
                at = cut(c, a)[b] + np.flatnonzero(d >> np.uint64(40))  # table indices of the escaping deltas
                lanes |= set((at % ec.DELTA_PER).tolist())
                first_small |= int(keys[0]) < 2**40
                first_big |= int(keys[0]) >= 2**40
                zero_first |= b == 0 and int(keys[0]) == 0
        assert gaps >= set(ec.GAPS)
        assert lanes == set(range(ec.DELTA_PER))
        assert first_small and first_big and zero_first
    c = ALL["k32_top_after_small"]
    keys = ec.slice_of(c, 0, 1, 0)[0]
    d = ec.deltas_of(keys)
    assert int(keys[0]) == 0 and int((d[1:] >> np.uint64(40)).max()) >= 2**24 - 2**9
    assert int(keys[-1]) >> 48 == 0xFFFF and int(keys[-1]) != 2**64 - 1


def test_7_set_mode():
    sets = group("set")
    assert {c.name for c in sets} == {c.name + "_set" for c in group(*ec.SET_GROUPS)}
    for c in sets:
        o = ALL[c.name[:-4]]
        assert c.mode == "set" and all(cs is None for _, cs in c.tables)
        assert all(np.array_equal(a[0], b[0]) for a, b in zip(c.tables, o.tables))
        assert ec.plan(c).cuts == ec.plan(o).cuts


def test_8_wide_keys():
    cases = group("wide")
    assert tuple(sorted({c.k for c in cases})) == ec.WIDE_KS == (33, 39, 40, 63)
    assert {c.owner_mode for c in cases} == {"separate", "local"}
    sums = set()
    for c in cases:
        p = ec.plan(c)
        straddles = p.shift < 64 < p.shift + p.bits
        assert straddles == (c.k in (33, 39))
        below = only_hi = False
        for a, b, keys, counts in sent_slices(c):
            for x, y in zip(keys, keys[1:]):
                below |= x >> p.shift == y >> p.shift
        for keys, _ in c.tables:
            los = {}
            for v in keys:
                los.setdefault(v & ec.M64, set()).add(v >> 64)
            only_hi |= any(len(h) > 1 for h in los.values())
        assert below and only_hi
        assert all(cut(c, r)[j + 1] > cut(c, r)[j] for r in range(3) for j in range(3))
        seen = set()
        first = last = False
        for a, b, keys, counts in sent_slices(c):
            seen |= set(counts.tolist())
            if len(counts) and ec.count_escapes(counts) < len(counts):
                first |= int(counts[0]) > 255
                last |= int(counts[-1]) > 255
        assert seen >= set(ec.COUNT_EDGES)  # 2^63 among them, in a slice that is sent
        assert first and last  # an escape at the first and at the last position of a sent slice
        common = set(c.tables[0][0])
        for keys, _ in c.tables[1:]:
            common &= set(keys)
        sums |= {sum(int(cs[ks.index(v)]) for ks, cs in c.tables) for v in common}
    assert 2**32 - 1 in sums and 2**32 in sums  # a key held by every rank, as in group 5


def test_9_small_k():
    cases = group("small_k")
    assert tuple(c.k for c in cases) == ec.SMALL_KS == (1, 4, 7, 8, 9)
    assert [ec.plan(c).shift for c in cases] == [0, 0, 0, 0, 2]
    for c in cases:
        for keys, counts in c.tables:
            assert np.array_equal(keys, np.arange(4**c.k, dtype=np.uint64))
        assert ec.count_escapes(c.tables[0][1]) > 0 or c.k == 1
        assert any(s for s, _ in ec.expected_bytes(c, 1))


def test_10_pieces():
    cases = group("pieces")
    assert tuple(sorted({c.knobs["piece_bytes"] for c in cases})) == ec.PIECES == (8, 16, 40, 4104)
    for piece in ec.PIECES:
        assert ec.piece_of(piece) == piece
        exact = more = less = False
        for c in cases:
            if c.knobs["piece_bytes"] != piece:
                continue
            assert sum(len(k) for k, _ in c.tables) < 6000
            for deltas in (0, 1):
                for kind, a, b, esize, n in ec.messages(c, deltas):
                    size = esize * n
                    exact |= size % piece == 0
                    more |= size > piece and size % piece == esize
                    less |= size > piece and esize < piece and size % piece == piece - esize
        assert exact and more and less
    # a 5-byte key, a wide key's two words and an escape pair in different pieces
    key5 = wide = esc = False
    for c in cases:
        piece = c.knobs["piece_bytes"]
        for kind, a, b, esize, n in ec.messages(c, 1):
            size = esize * n
            key5 |= kind == "keys5" and size > piece and piece % 5 != 0
            wide |= kind == "keys" and c.wide and size > piece and piece % 16 != 0
            esc |= kind == "count_escapes" and size > piece and piece % 16 != 0
        if piece == 4104:
            assert any(kind == "count_escapes" and 8 * n > piece for kind, a, b, esize, n in ec.messages(c, 0))
            assert any(kind == "keys5" and n > piece for kind, a, b, esize, n in ec.messages(c, 1)) or c.wide
    assert key5 and wide and esc


def test_11_two_tables():
    (c,) = group("two_tables")
    assert c.mode == "count" and len(c.more) == 1 and c.P == 3
    assert any(len(k) == 0 for k, _ in c.more[0]) and any(len(k) for k, _ in c.more[0])
    owners_b = [j for j in range(3) if len(ec.expected_tables(c, 1)[j][0])]
    assert len(owners_b) == 1
    assert all(len(ec.expected_tables(c, 0)[j][0]) for j in range(3))


def test_12_auto_format_cases():
    cases = [ALL[n] for n in ec.AUTO_FORMAT]
    assert {c.P for c in cases} == {2, 8}
    for c in cases:
        assert not c.wide and "wire_deltas" not in c.knobs
        assert ec.expected_bytes(c, 0) != ec.expected_bytes(c, 1)  # the formats can be told apart


def test_single_rank_subset():
    cases = group("single")
    assert all(c.P == 1 and c.owner_mode == "local" for c in cases)
    assert tuple(len(ALL[f"one_len{n}"].tables[0][0]) for n in ec.LENGTHS) == ec.LENGTHS
    assert set(ALL["one_counts"].tables[0][1].tolist()) >= set(ec.COUNT_EDGES)
    for k in (31, 32):
        keys = ALL[f"one_gaps_k{k}"].tables[0][0]
        d = ec.deltas_of(keys)
        assert set(d[1:].tolist()) >= set(ec.GAPS) and int(keys[0]) == 0
        assert set((np.flatnonzero(d >> np.uint64(40)) % ec.DELTA_PER).tolist()) == set(range(ec.DELTA_PER))
    assert {ALL[f"one_piece{p}"].knobs["piece_bytes"] for p in ec.PIECES} == set(ec.PIECES)
    assert ec.count_escapes(ALL["one_piece4104"].tables[0][1]) >= 300
    assert ALL["one_wide39"].wide
    for c in cases:
        assert ec.plan(c).cuts[0][0] == [0, len(c.tables[0][0])]
