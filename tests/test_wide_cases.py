"""CPU self-check of tests/wide_cases.py: every builder gives the shape it
promises at every k the GPU tests use it with, so that a failure of
tests/test_gpu_wide_item_shapes.py can be trusted (and a builder that silently
stops producing its shape fails here)."""

from collections import Counter

import numpy as np
import pytest

import wide_cases as wc
from oracle import OracleCounterWide

K_IDS = [f"k{k}" for k in wc.KS]


def _valid(ints, k):
    top = 1 << (2 * k)
    assert all(0 <= v < top for v in ints)
    assert all(v != (1 << 128) - 1 for v in ints)


def _one_item(ints, k, cap=wc.ITEM_CAP):
    _valid(ints, k)
    assert {wc.l1_bin(v, k) for v in ints} == {wc.PREFIX}
    assert 0 < wc.PREFIX < (1 << wc.L1_BITS) - 1
    assert len(ints) <= cap


def test_constants_and_ks():
    assert wc.EDGES == (1, 2, 511, 512, 513, 4095, 4096, 4097)
    assert wc.M_ITEMS == (1, 2, 63, 64, 65, 66, 128, 129, 512)
    assert wc.PASS_BITS == 5 and wc.pass_bits(4097) == 1 and wc.pass_bits(20_000) == 3
    assert wc.KS == (33, 36, 37, 38, 39, 40, 42, 43, 44, 45, 63, 64)
    assert {33, 63, 64} <= set(wc.KS) and all(33 <= k <= 64 for k in wc.KS)
    for name in ("l1", "partition", "home", "home_after_pass"):
        sides = {wc.side(wc.fields(k)[name]) for k in wc.KS}
        # (an L1 bin's top bit is 2k - 1 >= 65: never wholly below bit 64)
        assert sides == ({"straddle", "above"} if name == "l1" else {"below", "straddle", "above"}), name
    # the straddling k really put bit 64 inside the field, and 33 keeps hi inside the L1 bin
    assert wc.fields(33)["l1"] == (57, 66)
    for k in wc.KS:
        for name, (low, high) in wc.fields(k).items():
            assert (wc.side((low, high)) == "straddle") == (low < 64 < high)
    for sub in (wc.KS_SOME, wc.KS_TWINS, wc.KS_RUNS, wc.KS_REPEATED_READ):
        assert set(sub) <= set(wc.KS)
    assert len(wc.KS_SOME) >= 4 and {63, 64} <= set(wc.KS_SOME)
    assert any(wc.side(wc.fields(k)["home"]) == "straddle" for k in wc.KS_SOME)
    assert any(wc.side(wc.fields(k)["home"]) == "straddle" for k in wc.KS_RUNS) and 63 in wc.KS_RUNS
    assert min(wc.KS_TWINS) == 37


def test_pairs_round_trip_and_reference():
    ints = [0, 1, wc.M64, 1 << 64, (wc.M64 << 64) | 5, (1 << 128) - 2, 12345 << 70]
    p = wc.to_pairs(ints)
    assert p.dtype == np.uint64 and p.shape == (len(ints), 2)
    assert [int(x) for x in p[:, 0]] == [v & wc.M64 for v in ints]
    assert [int(x) for x in p[:, 1]] == [v >> 64 for v in ints]
    assert wc.from_pairs(p) == ints
    assert wc.from_pairs(p.reshape(-1)) == ints
    keys, counts = wc.reference([5, 3, 5, 1 << 100, 3, 5])
    assert keys == [3, 5, 1 << 100] and counts == [2, 3, 1]
    keys, counts = wc.reference([5, 3, 5], [wc.BIG_W, 7, wc.BIG_W])
    assert keys == [3, 5] and counts == [7, 2 * wc.BIG_W] and counts[1] > 1 << 32


@pytest.mark.parametrize("k", wc.KS, ids=K_IDS)
def test_revcomp_and_records(k):
    import okm
    ints = wc.one_item_distinct(k, 0, 50) + wc.extremes(k, 0)[1]
    ints = [v for v in ints if v != (1 << 128) - 1]
    rc = wc.revcomp(ints, k)
    assert wc.revcomp(rc, k) == ints
    assert rc[:20] == [okm.reverse_complement_u128(v, k) for v in ints[:20]]
    recs = wc.records(ints, k)
    assert all(len(r) == k for r in recs)
    assert [okm.seq_to_u128(r, k) for r in recs[:20]] == ints[:20]
    # PREFIX starts with AAA: nearly every key under it is its own canonical form
    body = wc.one_item_distinct(k, 1, 2000)
    same = sum(a == b for a, b in zip(body, wc.canonical(body, k)))
    assert same >= 0.97 * len(body)


@pytest.mark.parametrize("k", wc.KS, ids=K_IDS)
def test_one_item_builders(k):
    for n in wc.EDGES:
        cap = n  # 4097: one past an item, on purpose
        r = wc.one_item_repeats(k, 0, n)
        _one_item(r, k, cap)
        assert len(r) == n and len(set(r)) <= max(1, n // 4)
        if n >= wc.ROW - 1:
            assert len(set(r)) < n and max(Counter(r).values()) >= 2
        d = wc.one_item_distinct(k, 0, n)
        _one_item(d, k, cap)
        assert len(d) == n == len(set(d))
    for n in wc.FILL_NS:
        f = wc.one_key_fills_item(k, 0, n)
        _one_item(f, k)
        assert len(f) == n and len(set(f)) == 1
    assert wc.one_item_repeats(k, 0, 513) == wc.one_item_repeats(k, 0, 513)  # seeded
    assert wc.one_item_repeats(k, 0, 513) != wc.one_item_repeats(k, 1, 513)


@pytest.mark.parametrize("k", wc.KS, ids=K_IDS)
def test_one_home_and_end_homes(k):
    for n in wc.ONE_HOME_NS:
        ints = wc.one_home(k, 0, n)
        _one_item(ints, k)
        homes = Counter(wc.home_of(v, k) for v in set(ints))
        stem, crowd = Counter(v >> 16 for v in set(ints)).most_common(1)[0]
        assert crowd == n                                   # n keys differ in their lowest 16 bits only
        crowd_keys = [v for v in set(ints) if v >> 16 == stem]
        for passes in (0, 1, wc.PASS_BITS):                 # one home, whatever pass came before
            assert len({wc.home_of(v, k, passes) for v in crowd_keys}) == 1
        assert homes[wc.home_of(crowd_keys[0], k)] >= n
        assert len(homes) >= 200                            # beside ordinary keys
        assert len(ints) == n + 350 and len(set(ints)) == n + 300
    ints = wc.last_and_first_home(k, 0)
    _one_item(ints, k)
    last = (1 << wc.HOME_BITS) - 1
    assert {wc.home_of(v, k) for v in ints} == {0, 1, last - 1, last}
    assert max(Counter(ints).values()) == 3 and len(set(ints)) == 160


@pytest.mark.parametrize("k", wc.KS_TWINS, ids=[f"k{k}" for k in wc.KS_TWINS])
def test_word_twins(k):
    ints, hi_twins, lo_twins = wc.word_twins(k, 0)
    _one_item(ints, k)
    have = Counter(ints)
    assert len(hi_twins) >= 60 and len(lo_twins) >= 60
    for a, b in hi_twins:
        assert a != b and (a & wc.M64) == (b & wc.M64) and (a >> 64) != (b >> 64)
        assert have[a] >= 1 and have[b] >= 1
    for a, b in lo_twins:
        assert a != b and (a >> 64) == (b >> 64) and (a & wc.M64) != (b & wc.M64)
        assert have[a] >= 1 and have[b] >= 1
    assert max(have.values()) >= 3                      # repeats
    los = {v & wc.M64 for v in ints}
    assert set(wc.SPECIAL_LO) <= los
    assert wc.SPECIAL_LO == (0, wc.M64, 1 << 63, (1 << 63) - 1)
    # found without the builder's word: the input itself holds both kinds of pair
    by_lo, by_hi = Counter(v & wc.M64 for v in have), Counter(v >> 64 for v in have)
    assert sum(1 for c in by_lo.values() if c >= 2) >= 50
    assert sum(1 for c in by_hi.values() if c >= 2) >= 2 and len(by_hi) >= 2


@pytest.mark.parametrize("k", wc.KS_SOME, ids=[f"k{k}" for k in wc.KS_SOME])
def test_dense_extremes_weighted(k):
    for low in wc.DENSE_LOW_BITS:
        for w8 in (False, True):
            ints, w = wc.dense_item(k, 0, low, weighted=w8)
            _valid(ints, k)
            assert 5000 <= len(ints) <= 20_000 and len(ints) > wc.ITEM_CAP
            assert len({v >> low for v in ints}) == 1 and {wc.l1_bin(v, k) for v in ints} == {wc.PREFIX}
            assert len(set(ints)) > (1 << low) * 0.95        # nearly every slot, each several times
            assert (w is None) == (not w8)
            if w8:
                assert len(w) == len(ints) and 1 <= min(w) and max(w) <= 1000
    assert wc.DENSE_LOW_BITS == (8, 11)
    ints, special = wc.extremes(k, 0)
    _valid(ints, k)
    have = Counter(ints)
    assert all(have[v] >= 2 for v in special)
    assert 0 in have and max(have) == (1 << (2 * k)) - (2 if k == 64 else 1)
    if k == 64:
        for hi, lo in ((wc.M64, 0), (wc.M64, wc.M64 - 1), (0, wc.M64), (wc.M64 >> 1, wc.M64)):
            assert have[(hi << 64) | lo] >= 2
    assert len(have) >= 300
    for n in wc.EDGES:
        for big in (False, True):
            ints, w = wc.weighted(k, 0, n, big)
            _valid(ints, k)
            assert len(ints) == len(w) == n + (3 if big else 0)
            assert {wc.l1_bin(v, k) for v in ints} == {wc.PREFIX}
            assert ints[:n] == wc.one_item_repeats(k, 0, n)
            assert all(1 <= x <= 1000 for x in w[:n])
            if big:
                _, counts = wc.reference(ints, w)
                assert sorted(c for c in counts if c > 1 << 32) == [wc.LONE_W, 2 * wc.BIG_W]
                assert wc.BIG_W < 1 << 32 < wc.LONE_W


@pytest.mark.parametrize("k", wc.KS, ids=K_IDS)
def test_split_part(k):
    rem = 2 * k - wc.L1_BITS
    for n in wc.SPLIT_NS:
        for skewed in (False, True):
            ints = wc.split_part(k, 0, n, skewed)
            _valid(ints, k)
            assert len(ints) == n > wc.ITEM_CAP                     # more than an item: the part must split
            assert {wc.l1_bin(v, k) for v in ints} == {wc.PREFIX}
            b = wc.pass_bits(n)
            bins = Counter((v >> (rem - b)) & ((1 << b) - 1) for v in ints)
            if skewed:
                stems = Counter(v >> (rem - 40) for v in ints)
                assert sorted(stems.values())[-3:] == [n // 4] * 3
                if n == max(wc.SPLIT_NS):
                    assert max(bins.values()) > 4 * min(bins.values())  # very uneven bins
            else:
                assert len(bins) == 1 << b and max(bins.values()) <= wc.ITEM_CAP
    ints = wc.split_part(k, 0, wc.SPLIT_NS[0], flanks=True)
    _valid(ints, k)
    last = (1 << wc.L1_BITS) - 1
    per_bin = Counter(wc.l1_bin(v, k) for v in ints)
    assert per_bin == {0: 40, 1: 40, wc.PREFIX: wc.SPLIT_NS[0], last - 1: 40, last: 40}


@pytest.mark.parametrize("k", wc.KS_SOME, ids=[f"k{k}" for k in wc.KS_SOME])
def test_m_items(k):
    last = (1 << wc.L1_BITS) - 1
    for m in wc.M_ITEMS:
        for ends_only in (False, True):
            ints = wc.m_items(k, 0, m, ends_only=ends_only)
            _valid(ints, k)
            per_bin = Counter(wc.l1_bin(v, k) for v in ints)
            assert len(per_bin) == m and set(per_bin.values()) == {50}
            assert len(ints) == 50 * m and len(set(ints)) == 40 * m
            if m >= 2:
                assert 0 in per_bin and last in per_bin
            if ends_only and 2 <= m < last:
                gap = [b for b in range(last + 1) if b not in per_bin]
                assert gap == list(range(min(gap), max(gap) + 1))   # one hole in the middle
    # for_records: every key its own canonical form, so the from-bytes flavour
    # populates the same m bins
    for m in (2, wc.WINDOW + 1, 1 << wc.L1_BITS):
        for ends_only in (False, True):
            ints = wc.m_items(k, 0, m, ends_only=ends_only, for_records=True)
            _valid(ints, k)
            assert wc.canonical(ints, k) == ints
            per_bin = Counter(wc.l1_bin(v, k) for v in ints)
            assert len(per_bin) == m and set(per_bin.values()) == {50} and len(set(ints)) == 40 * m
    ints = wc.split_part(k, 0, wc.SPLIT_NS[0], flanks=True, for_records=True)
    flank = [v for v in ints if wc.l1_bin(v, k) != wc.PREFIX]
    assert len(flank) == 160 and wc.canonical(flank, k) == flank
    for m, n in wc.ALTERNATING:
        for_records = m > 2 * wc.WINDOW
        ints = wc.m_items(k, 0, m, alternate=n, for_records=for_records)
        _valid(ints, k)
        if for_records:
            assert wc.canonical(ints, k) == ints
        per_bin = Counter(wc.l1_bin(v, k) for v in ints)
        assert len(per_bin) == m and len(ints) <= 70_000
        sizes = [per_bin[b] for b in sorted(per_bin)]
        assert sizes == [1 if i % 2 == 0 else n for i in range(m)] and n <= wc.ITEM_CAP
        assert len(set(ints)) < len(ints)
    assert wc.ALTERNATING[0][1] == 3000 and wc.ALTERNATING[1][0] > 2 * wc.WINDOW


def _oracle(recs, k):
    oc = OracleCounterWide(k)
    oc.add_records(recs)
    ek, ec = oc.result(1)
    return wc.from_pairs(ek), [int(c) for c in ec]


def test_bytes_cases_against_the_oracle():
    names = []
    for name, k, recs in wc.bytes_cases():
        names.append(name)
        keys, counts = wc.reference(wc.kmers_of_records(recs, k))
        ok, ocnt = _oracle(recs, k)
        assert keys == ok and counts == ocnt, name
        if name.startswith("polyA"):
            assert keys == [0] and counts[0] in (wc.ITEM_CAP, wc.ITEM_CAP + 1)
        if name.startswith("repeated-read"):
            assert max(counts) >= wc.ROW and len(keys) > 1000
    assert len(names) == 1 + 2 * len(wc.KS_SOME) + 2 * len(wc.KS_REPEATED_READ)
    # T^32 A^32: its own reverse complement, hi = ~0 and lo = 0
    keys, counts = wc.reference(wc.kmers_of_records(wc.palindrome_records(), 64))
    assert keys[-1] == wc.M64 << 64 and counts[-1] == 4
    assert wc.canonical([wc.M64 << 64], 64) == [wc.M64 << 64]


@pytest.mark.parametrize("k", wc.KS_SOME, ids=[f"k{k}" for k in wc.KS_SOME])
def test_records_flavour_against_the_oracle(k):
    """records() + canonical(): what the from-bytes flavour of a pairs shape
    counts is what the oracle counts from the same reads."""
    ints = wc.one_item_repeats(k, 0, 513) + wc.extremes(k, 0)[0]
    keys, counts = wc.reference(wc.canonical(ints, k))
    ok, ocnt = _oracle(wc.records(ints, k), k)
    assert keys == ok and counts == ocnt


@pytest.mark.parametrize("k", wc.KS, ids=K_IDS)
def test_for_records_keeps_the_shapes(k):
    """for_records: the same promises, from keys that are their own canonical
    forms -- what the from-bytes flavour counts is what was built."""
    def own(ints):
        _valid(ints, k)
        assert wc.canonical(ints, k) == ints
        assert {wc.l1_bin(v, k) for v in ints} == {wc.PREFIX}
        return ints

    for n in wc.EDGES:
        r = own(wc.one_item_repeats(k, 0, n, for_records=True))
        assert len(r) == n and len(set(r)) <= max(1, n // 4)
        d = own(wc.one_item_distinct(k, 0, n, for_records=True))
        assert len(d) == n == len(set(d))
    for n in wc.FILL_NS:
        f = own(wc.one_key_fills_item(k, 0, n, for_records=True))
        assert len(f) == n and len(set(f)) == 1
    for n in wc.ONE_HOME_NS:
        ints = own(wc.one_home(k, 0, n, for_records=True))
        stem, crowd = Counter(v >> 22 for v in set(ints)).most_common(1)[0]
        assert crowd == n and len(ints) == n + 350 and len(set(ints)) == n + 300
        for passes in (0, 1, wc.PASS_BITS):
            assert len({wc.home_of(v, k, passes) for v in set(ints) if v >> 22 == stem}) == 1
    ints = own(wc.last_and_first_home(k, 0, for_records=True))
    last = (1 << wc.HOME_BITS) - 1
    assert {wc.home_of(v, k) for v in ints} == {0, 1, last - 1, last} and len(set(ints)) == 160
    rem = 2 * k - wc.L1_BITS
    for n in wc.SPLIT_NS[:2]:
        for skewed in (False, True):
            ints = own(wc.split_part(k, 0, n, skewed, for_records=True))
            assert len(ints) == n
            if skewed:
                assert sorted(Counter(v >> (rem - 40) for v in ints).values())[-3:] == [n // 4] * 3
