"""okm_compare_histogram on the device, exact against plain Python dicts, every case both ways."""

import subprocess

import numpy as np
import pytest

import hist_cases as hc
import lookup_cases as lc
import okm
import test_gpu_compare_counts as cc
from okm import _lib, testing
from oracle import OracleCounter, OracleCounterWide

pytestmark = pytest.mark.gpu

K, T, TW, P, BIG = cc.K, cc.T, cc.TW, cc.P, cc.BIG
PAST, BINS = 5_000_000_000, (64, 48)  # PAST: a count that LDS holds saturated
counter, table_of, same_table, two_tables = cc.counter, cc.table_of, cc.same_table, cc.two_tables


def expected(ta, tb, bins, ma=1, mb=1):
    ka = {v: c for v, c in ta.items() if c >= max(ma, 1)}
    kb = {v: c for v, c in tb.items() if c >= max(mb, 1)}
    m = np.zeros(bins, np.uint64)
    for v in ka.keys() | kb.keys():
        m[min(ka.get(v, 0), bins[0] - 1), min(kb.get(v, 0), bins[1] - 1)] += 1
    return m, list(ka.values()), list(kb.values()), len(ka.keys() | kb.keys())


def check(ca, cb, ta, tb, bins=BINS, ma=1, mb=1):
    exp, kept_a, kept_b, union = expected(ta, tb, bins, ma, mb)
    got = ca.compare_histogram(cb, bins, ma, mb)
    assert got.dtype == np.uint64 and np.array_equal(got, exp), np.argwhere(got != exp)[:8]
    # the rows sum to a's kept histogram, the columns to b's (row / column 0: the other side's own), all to the union
    assert np.array_equal(got.sum(1)[1:], hc.expected_hist(kept_a, bins[0])[1:])
    assert np.array_equal(got.sum(0)[1:], hc.expected_hist(kept_b, bins[1])[1:])
    assert int(got.sum()) == union and got[0, 0] == 0
    assert np.array_equal(cb.compare_histogram(ca, bins[::-1], mb, ma), exp.T)
    return exp


@pytest.mark.parametrize("k", [K, 64])
@pytest.mark.parametrize("dense_a,dense_b", [(False, False), (False, True), (True, False), (True, True)])
def test_representation_pairs(dense_a, dense_b, k):
    runs, inp = lc.items()
    ta = table_of(inp)
    tb = {v: 1 + i % 4 for i, v in enumerate(cc.run_edges(runs, ta))}  # B: the edges of A's runs ...
    tb.update({int(v): 2 for v in hc.many_items()[:500]})              # ... and keys all over the key space
    if k > 32:
        ta, tb = ({v << 64 | (v & 0xFF): c for v, c in x.items()} for x in (ta, tb))
    with counter(ta, k, dense=dense_a) as a, counter(tb, k, dense=dense_b) as b:
        before = cc.launches(a), cc.launches(b)
        assert k > 32 or before == (int(dense_a), int(dense_b))  # an unweighted count leaves a pending table (u32 counts)
        assert check(a, b, ta, tb)[1:, 1:].sum() > 0
        assert (cc.launches(a), cc.launches(b)) == before  # nothing was gathered
        same_table(a, ta)


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("k,m", [(K, m) for m in (0, 1, T - 1, T, T + 1, 2 * T + 1)] + [(64, TW + 1), (64, 2 * TW + 1)])
def test_run_and_tile_edges(k, m, dense):
    # A: m keys under one prefix between two populated ranges; B: the edges of A's runs, u64 counts past 2^32
    ta = table_of(hc.one_item(m))
    keys = np.array(sorted(ta), np.uint64)
    runs = [keys[(keys >> np.uint64(hc.LOW_BITS)) == (p >> np.uint64(hc.LOW_BITS))]
            for p in (hc.PREFIX_BELOW, hc.PREFIX, hc.PREFIX_ABOVE)]
    edges = cc.run_edges([r for r in runs if len(r)], ta) + [P + 5, P - 1 + (1 << hc.LOW_BITS)]
    tb = {v: (PAST if v in ta else 1 + i % 7) for i, v in enumerate(sorted(set(edges)))}
    if k > 32:  # the same keys in the high word: neighbours differ in one word only
        ta = {v << 64 | 7: c for v, c in ta.items()}
        tb = {**{v << 64 | 7: c for v, c in tb.items()}, **{v << 64 | 6: 3 for v in list(tb)[::2]}}
    with counter(ta, k, dense=dense) as a, counter(tb, k, weighted=True, dense=dense) as b:
        check(a, b, ta, tb)
        same_table(a, ta)


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("k", [K, 64])
def test_long_s_range_under_one_tile(k, dense):
    t = TW if k > 32 else T
    rng = np.random.default_rng(k)
    low = np.sort(hc._distinct_low(rng, 3 * t + 5))
    lo, hi = P | int(low[0]), P | int(low[-1])
    ts = {**{P | int(v): 1 + i % 5 for i, v in enumerate(low[1:])}, hi: 4}
    td = {lo: 3, hi: 2}
    for p in (hc.PREFIX_BELOW, hc.PREFIX_ABOVE):
        td.update({int(p) | int(v): 1 for v in hc._distinct_low(rng, 2 * t + 9)})
    if k > 32:
        td, ts = ({v << 64 | (v & 0xFFFF): c for v, c in x.items()} for x in (td, ts))
    with counter(td, k, dense=dense) as d, counter(ts, k, dense=dense) as s:
        assert check(d, s, td, ts)[2, 4] == 1


def test_more_tiles_than_workgroups_on_the_diagonal():
    """1.4 M keys once on each side: 1,368 tiles for at most 5 x 256 persistent workgroups, every match on one bin."""
    rng = np.random.default_rng(41)
    keys = np.unique(rng.integers(0, 1 << 62, 1_410_000, dtype=np.uint64))[:1_400_000]
    with okm.KmerCounter(K) as a, okm.KmerCounter(K) as b:
        a.add_pairs(keys)
        b.add_pairs(keys[::3])
        assert a.count() == len(keys) and b.count() == len(keys[::3])
        a.result(1)  # dense: pieces of T
        exp = np.zeros(BINS, np.uint64)
        exp[1, 1], exp[1, 0] = len(keys[::3]), len(keys) - len(keys[::3])
        assert np.array_equal(a.compare_histogram(b, BINS), exp) and np.array_equal(b.compare_histogram(a, BINS[::-1]), exp.T)
        exp[1, 1], exp[1, 0] = len(keys), 0
        assert np.array_equal(a.compare_histogram(a, BINS), exp)  # a against itself


@pytest.mark.parametrize("bins", [BINS, (1001, 6), (2, 2), (65536, 64)])
def test_corner_and_last_bin_edges(bins):
    # every pair of the counts around the LDS corner and around the last bin, past 2^32 and 1
    ra, rb = testing.joint_corner(*bins)
    assert (ra, rb) == {BINS: (45, 45), (1001, 6): (341, 6), (2, 2): (2, 2), (65536, 64): (45, 45)}[bins]
    va, vb = ([1, r - 1, r, n - 2, n - 1, n, PAST] for r, n in ((ra, bins[0]), (rb, bins[1])))
    rng = np.random.default_rng(7)
    keys = [int(v) for v in np.unique(rng.integers(0, 1 << 62, 4000, dtype=np.uint64))[:3 * 49 + 20]]
    pairs = [(x, y) for x in va for y in vb] * 3
    ta = {v: max(x, 1) for v, (x, _) in zip(keys, pairs)}
    tb = {v: max(y, 1) for v, (_, y) in zip(keys, pairs)}
    ta.update({v: PAST for v in keys[len(pairs):len(pairs) + 10]}), tb.update({v: 2 for v in keys[len(pairs) + 10:]})
    with counter(ta, weighted=True) as a, counter(tb, weighted=True, dense=True) as b:
        exp = check(a, b, ta, tb, bins)
        assert exp[bins[0] - 1, bins[1] - 1] >= 3 and exp[bins[0] - 1, 0] >= 10
        check(a, a, ta, ta, bins)  # a is b: the clamped diagonal
        check(a, b, ta, tb, bins, PAST, PAST - 1)  # thresholds past 2^32 - 1 are exact: only PAST is kept
        check(a, b, ta, tb, bins, PAST + 1, 1)


def test_thresholds_and_empty_tables(two_tables):
    ta, tb = two_tables  # counts 1..5 and 1..3
    with counter(ta) as a, counter(tb, dense=True) as b, okm.KmerCounter(K) as never, counter({}) as empty:
        shared = check(a, b, ta, tb)[1:, 1:].sum()
        for ma, mb in [(0, 0), (3, 1), (1, 3), (5, 3), (6, 1), (2, BIG), (6, 4)]:
            exp = check(a, b, ta, tb, BINS, ma, mb)  # to column 0, to row 0, out of the matrix; 6 / 4 / BIG keep nothing
            assert exp[1:, 1:].sum() < shared or (ma, mb) == (0, 0)
        for e in (never, empty):
            assert check(a, e, ta, {}, BINS, 2, 1)[:, 1:].sum() == 0
        assert not check(never, empty, {}, {}).any()


@pytest.mark.parametrize("host_a,host_b", [(True, False), (False, True), (True, True)])
def test_host_resident_tables(two_tables, host_a, host_b):
    ta, tb = two_tables
    with counter(ta) as a, counter(tb) as b:
        want = check(a, b, ta, tb, BINS, 2, 1)
        for c, t, host in ((a, ta, host_a), (b, tb, host_b)):
            if host:
                cc.to_host_table(c, t)
        for sl in (1000, 4096, len(ta)):  # a ragged last slice, several slices, one slice
            testing.set_knob("hist_slice", sl)
            assert np.array_equal(check(a, b, ta, tb, BINS, 2, 1), want)
            assert all(c.engine_info()["host_bytes"] > 0 for c, host in ((a, host_a), (b, host_b)) if host)
        same_table(b, tb)


@pytest.mark.parametrize("sliced", [False, True])
def test_every_allocation_fails_in_turn(two_tables, sliced):
    ta, tb = two_tables
    exp = expected(ta, tb, BINS, 2, 2)[0]

    def attempt(a, b, fail):  # -> the matrix or the error's status, and what the knob still counts
        testing.set_knob("fail_alloc", fail)
        try:
            got = a.compare_histogram(b, BINS, 2, 2)
        except okm.OkmError as e:
            got = e.status
        left = testing.get_knob("fail_alloc")
        testing.set_knob("fail_alloc", -1)
        return got, left

    with counter(ta) as a, counter(tb) as b:
        if sliced:
            cc.to_host_table(a, ta)
            cc.to_host_table(b, tb)
            testing.set_knob("hist_slice", 5000)
        got, left = attempt(a, b, BIG)
        assert np.array_equal(got, exp) and BIG - left > 3
        for n in range(1, BIG - left + 1):
            in_use = testing.device_in_use(a), testing.device_in_use(b)
            got, fired = attempt(a, b, n)
            assert fired == -1, f"allocation {n}: the failure did not fire"
            assert np.array_equal(got, exp) if isinstance(got, np.ndarray) else got == _lib.OKM_E_NOMEM, (n, got)
            assert (testing.device_in_use(a), testing.device_in_use(b)) == in_use, f"allocation {n}: a block was stranded"
            assert np.array_equal(a.compare_histogram(b, BINS, 2, 2), exp)
        same_table(b, tb)


def test_error_codes(two_tables):
    ta, _ = two_tables
    m = np.zeros(1 << 22, np.uint64)
    with counter(ta) as a, okm.KmerCounter(K, "set") as s, okm.KmerCounter(K - 2) as other_k, \
            okm.KmerCounter(40, wide=True) as w:
        s.add_pairs(np.arange(1, 50, dtype=np.uint64))
        ok, bad, state, ptr = _lib.OKM_OK, _lib.OKM_E_ARG, _lib.OKM_E_STATE, m.ctypes.data
        cases = [(x, y, ptr, 8, 8, want) for x, y, want in [(None, a.ctx, bad), (a.ctx, None, bad), (a.ctx, s.ctx, state),
                                                            (s.ctx, a.ctx, state), (a.ctx, other_k.ctx, bad), (w.ctx, a.ctx, bad)]]
        cases += [(a.ctx, a.ctx, None, 8, 8, bad)] + [(a.ctx, a.ctx, ptr, *v) for v in [
            (1, 8, bad), (8, 1, bad), (65537, 2, bad), (2049, 2048, bad), (1 << 63, 1 << 63, bad), (2048, 2048, ok), (65536, 64, ok)]]
        for x, y, r, ba, bb, want in cases:
            assert _lib.load().okm_compare_histogram(x, y, 1, 1, r, ba, bb) == want, (ba, bb)
        check(a, a, ta, ta)  # the table is as it was


@pytest.mark.parametrize("k", [21, 35])
def test_cli_compare_matrix(tmp_path, k):
    rng = np.random.default_rng(k)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 3000)]
    tables, files = [], []
    for i, (lo, hi, n) in enumerate([(0, 2000, 90), (1000, 3000, 60)]):
        reads = [genome[o:o + 100].tobytes() for o in rng.integers(lo, hi - 100, n)]
        fa = tmp_path / f"s{i}.fa"
        fa.write_bytes(b"".join(b">r\n" + r + b"\n" for r in reads))
        oc = (OracleCounterWide if k > 32 else OracleCounter)(k)
        oc.add_records(reads, normalized=True)
        ek, ec = oc.result(1)
        tables.append(dict(zip(lc.from_pairs(ek) if k > 32 else (int(v) for v in ek), (int(c) for c in ec))))
        files.append(str(fa))
    exp = expected(tables[0], tables[1], (5, 4), 2, 1)[0]
    cmp_out, mat = tmp_path / "cmp.tsv", tmp_path / "m.tsv"
    r = subprocess.run([_lib.CLI_PATH, "count", "-k", str(k), "-i", files[0], "-o", str(tmp_path / "out.tsv"), "-m", "2",
                        "--compare", files[1], "--compare-output", str(cmp_out), "--compare-matrix", str(mat),
                        "--compare-matrix-bins", "5,4"] + (["--wide"] if k > 32 else []), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and cmp_out.read_text().startswith("n_a\t"), r.stderr
    assert mat.read_text() == "".join(f"{i}\t{j}\t{int(exp[i, j])}\n" for i in range(5) for j in range(4) if exp[i, j])
