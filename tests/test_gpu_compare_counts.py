"""okm_compare_counts on the device, exact against plain Python dicts, every case both ways."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

import hist_cases as hc
import lookup_cases as lc
import okm
from okm import _lib, testing
from oracle import OracleCounter, OracleCounterWide

pytestmark = pytest.mark.gpu

K = lc.K
M64 = lc.M64
T, TW = 1024, 512  # okm_compare.hip: a tile's entries, u64 / two-word keys
BIG = 10**9
FIELDS = ("n_a", "n_b", "sum_a", "sum_b", "n_shared", "sum_min", "sum_a_shared", "sum_b_shared")
P = int(hc.PREFIX)


def expected(ta, tb, ma=1, mb=1):
    ka = {v: c for v, c in ta.items() if c >= max(ma, 1)}
    kb = {v: c for v, c in tb.items() if c >= max(mb, 1)}
    sh = ka.keys() & kb.keys()
    vals = (len(ka), len(kb), sum(ka.values()), sum(kb.values()), len(sh), sum(min(ka[v], kb[v]) for v in sh),
            sum(ka[v] for v in sh), sum(kb[v] for v in sh))
    return {f: v & M64 for f, v in zip(FIELDS, vals)}


def mirror(d):
    return {f: d[f.replace("_a", "_x").replace("_b", "_a").replace("_x", "_b")] for f in FIELDS}


def check(ca, cb, ta, tb, ma=1, mb=1):
    exp = expected(ta, tb, ma, mb)
    assert ca.compare_counts(cb, ma, mb) == exp
    assert cb.compare_counts(ca, mb, ma) == mirror(exp)
    return exp


def table_of(keys, counts=None):
    ek, ec = hc.table_of(keys, counts)
    return dict(zip((int(v) for v in ek), (int(c) for c in ec)))


def counter(table, k=K, weighted=False, dense=False):
    wide = k > 32
    keys = sorted(table)
    c = okm.KmerCounter(k, wide=wide)
    c.set_timing(True)
    arr = lc.to_pairs(keys) if wide else np.array(keys, np.uint64)
    if weighted:
        c.add_pairs(arr, np.array([table[v] for v in keys], np.uint64))
    else:
        c.add_pairs(np.repeat(arr, [table[v] for v in keys], axis=0))
    assert c.count() == len(table)
    if dense:
        same_table(c, table)
    return c


def same_table(c, table):
    gk, gc = c.result(1)
    keys = lc.from_pairs(gk) if c.wide else [int(v) for v in gk]
    assert dict(zip(keys, (int(x) for x in gc))) == table and keys == sorted(table)


def launches(c, name="compact_items"):
    return c.kernel_stats().get(name, {"launches": 0})["launches"]


def run_edges(runs, present):
    out = set()
    for r in runs:
        for v in (int(r[0]), int(r[-1])):
            out |= {v} | {w for w in (v - 1, v + 1) if w not in present and w >= 0}
    return sorted(out)


@pytest.mark.parametrize("dense_a,dense_b", [(False, False), (False, True), (True, False), (True, True)])
def test_representation_pairs(dense_a, dense_b):
    runs, inp = lc.items()
    ta = table_of(inp)
    tb = {v: 1 + i % 4 for i, v in enumerate(run_edges(runs, ta))}  # B: the edges of A's runs and nothing else
    tb.update({int(v): 2 for v in hc.many_items()[:500]})           # ... but for keys all over the key space
    with counter(ta, dense=dense_a) as a, counter(tb, dense=dense_b) as b:
        before = launches(a), launches(b)
        assert before == (int(dense_a), int(dense_b))  # an unweighted count leaves a pending table
        check(a, b, ta, tb)
        assert (launches(a), launches(b)) == before  # the compare gathered nothing
        same_table(a, ta)
        same_table(b, tb)


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("k,m", [(K, m) for m in (0, 1, T - 1, T, T + 1, 2 * T + 1)] + [(64, TW + 1), (64, 2 * TW + 1)])
def test_run_and_tile_edges(k, m, dense):
    """A: m keys under one prefix between two populated ranges; B: the edges of A's runs, u64 counts past 2^32."""
    ta = table_of(hc.one_item(m))
    keys = np.array(sorted(ta), np.uint64)
    runs = [keys[(keys >> np.uint64(hc.LOW_BITS)) == (p >> np.uint64(hc.LOW_BITS))]
            for p in (hc.PREFIX_BELOW, hc.PREFIX, hc.PREFIX_ABOVE)]
    edges = run_edges([r for r in runs if len(r)], ta) + [P + 5, P - 1 + (1 << hc.LOW_BITS)]
    tb = {v: (5_000_000_000 if v in ta else 1 + i % 7) for i, v in enumerate(sorted(set(edges)))}
    if k > 32:  # the same keys in the high word: neighbours differ in one word only
        ta = {v << 64 | 7: c for v, c in ta.items()}
        tb = {**{v << 64 | 7: c for v, c in tb.items()}, **{v << 64 | 6: 3 for v in list(tb)[::2]}}
    with counter(ta, k, dense=dense) as a, counter(tb, k, weighted=True, dense=dense) as b:
        check(a, b, ta, tb)
        same_table(a, ta)


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("k", [K, 64])
def test_long_s_range_under_one_tile(k, dense):
    """A D run of two keys around 3T + 5 keys of S (several chunks; dense: several S runs), S ending at its run's end."""
    t = TW if k > 32 else T
    rng = np.random.default_rng(k)
    low = np.sort(hc._distinct_low(rng, 3 * t + 5))
    lo, hi = P | int(low[0]), P | int(low[-1])
    ts = {P | int(v): 1 + i % 5 for i, v in enumerate(low[1:])}  # holds D's upper extreme as its run's last key
    ts[hi] = 4
    td = {lo: 3, hi: 2}
    for p in (hc.PREFIX_BELOW, hc.PREFIX_ABOVE):
        td.update({int(p) | int(v): 1 for v in hc._distinct_low(rng, 2 * t + 9)})
    if k > 32:
        td, ts = ({v << 64 | (v & 0xFFFF): c for v, c in x.items()} for x in (td, ts))
    with counter(td, k, dense=dense) as d, counter(ts, k, dense=dense) as s:
        assert check(d, s, td, ts)["sum_min"] == 2


def test_key_extremes():
    keys = lc.k32_table(True)
    ta = table_of(np.concatenate([keys, [np.uint64(M64 - 1)] * 2]))  # key 0, and the largest key a table can hold
    tb = {v: c + 1 for v, c in list(ta.items())[::2]}
    tb.update({0: 1, M64 - 1: 9, M64 - 2: 1})
    below = {v >> 8: c for v, c in ta.items()}            # every key below ...
    above = {(v >> 8) | (0xFE << 56): 2 for v in ta}      # ... every key of this one
    with counter(ta, 32) as a, counter(tb, 32, weighted=True) as b, counter(below, 32) as lo, \
            counter(above, 32, dense=True) as hi, counter(ta, 32, weighted=True) as same:
        exp = check(a, b, ta, tb)
        assert exp["n_shared"] == len(tb) - 1
        assert check(lo, hi, below, above)["n_shared"] == 0  # disjoint
        assert check(a, same, ta, ta)["n_shared"] == len(ta)  # identical
        assert check(a, a, ta, ta)["sum_min"] == exp["sum_a"]  # a is b


@pytest.mark.parametrize("k", [33, 48, 64])
@pytest.mark.parametrize("dense", [False, True])
def test_wide_word_neighbours(k, dense):
    ta, queries = lc.word_neighbours(k)
    top = (1 << (2 * k)) - 1
    tb = {v: 1 + v % 3 for v in queries[::2] if 0 <= v < top}  # keys of A and their one-word neighbours
    with counter(ta, k, dense=dense) as a, counter(tb, k, weighted=True, dense=dense) as b:
        check(a, b, ta, tb)
        same_table(a, ta)
        same_table(b, tb)


def test_counts_and_thresholds():
    rng = np.random.default_rng(3)
    keys = [int(v) for v in np.unique(rng.integers(0, 1 << 62, 6000, dtype=np.uint64))]
    ta = {v: 1 + i % 6 for i, v in enumerate(keys[:5000])}
    tb = {v: 1 + i % 4 for i, v in enumerate(keys[1000:])}
    huge = {v: M64 - 5 for v in keys[:3]}   # sums that wrap 2^64
    huge.update({v: 4 for v in keys[3:40]})
    with counter(ta) as a, counter(tb, dense=True) as b, counter(huge, weighted=True) as h:
        for ma, mb in [(0, 0), (1, 1), (3, 1), (4, 1), (1, 4), (1, 5), (6, 4), (7, 1), (2, BIG)]:
            exp = check(a, b, ta, tb, ma, mb)  # counts == min, min - 1 on each side; 7 / 5 / BIG keep nothing
            assert (exp["n_shared"] == 0) == (ma == 7 or mb >= 5)
        exp = check(h, h, huge, huge)
        assert exp["sum_min"] == exp["sum_a"] == (3 * (M64 - 5) + 4 * 37) & M64 < 1 << 10
        assert check(h, a, huge, ta, 5, 1)["n_shared"] == 3


def to_host_table(c, table):
    testing.set_knob("fail_alloc", 1)  # the dense gather's first allocation fails: the table stays on the host
    same_table(c, table)
    assert c.engine_info()["host_bytes"] > 0


@pytest.fixture(scope="module")
def two_tables():
    rng = np.random.default_rng(9)
    keys = [int(v) for v in np.unique(rng.integers(0, 1 << 62, 14_000, dtype=np.uint64))]
    ta = {v: 1 + i % 5 for i, v in enumerate(keys[:11_003])}
    tb = {v: 1 + i % 3 for i, v in enumerate(keys[4_000:])}
    return ta, tb


@pytest.mark.parametrize("host_a,host_b", [(True, False), (False, True), (True, True)])
def test_host_resident_tables(two_tables, host_a, host_b):
    ta, tb = two_tables
    with counter(ta) as a, counter(tb) as b:
        want = check(a, b, ta, tb, 2, 1)
        for c, t, host in ((a, ta, host_a), (b, tb, host_b)):
            if host:
                to_host_table(c, t)
        for sl in (1000, 4096, len(ta)):  # a ragged last slice, several slices, one slice
            testing.set_knob("hist_slice", sl)
            assert check(a, b, ta, tb, 2, 1) == want
            assert all(c.engine_info()["host_bytes"] > 0 for c, host in ((a, host_a), (b, host_b)) if host)
        same_table(b, tb)


def test_empty_tables(two_tables):
    ta, _ = two_tables
    with counter(ta) as a, okm.KmerCounter(K) as never, counter({}) as empty:
        for e in (never, empty):
            check(a, e, ta, {}, 2, 1)
        assert check(never, empty, {}, {}) == dict.fromkeys(FIELDS, 0)


@pytest.mark.parametrize("sliced", [False, True])
def test_every_allocation_fails_in_turn(two_tables, sliced):
    ta, tb = two_tables
    exp = expected(ta, tb, 2, 2)

    left = [0]

    def attempt(a, b, fail):
        testing.set_knob("fail_alloc", fail)
        try:
            return a.compare_counts(b, 2, 2), None
        except okm.OkmError as e:
            return None, e
        finally:
            left[0] = testing.get_knob("fail_alloc")
            testing.set_knob("fail_alloc", -1)

    with counter(ta) as a, counter(tb) as b:
        if sliced:
            to_host_table(a, ta)
            to_host_table(b, tb)
            testing.set_knob("hist_slice", 5000)
        got, err = attempt(a, b, BIG)
        assert err is None and got == exp
        n_gets = BIG - left[0]
        for n in range(1, n_gets + 1):
            in_use = testing.device_in_use(a), testing.device_in_use(b)
            got, err = attempt(a, b, n)
            assert left[0] == -1, f"allocation {n}: the failure did not fire"
            assert got == exp if err is None else err.status == _lib.OKM_E_NOMEM, (n, err)
            assert (testing.device_in_use(a), testing.device_in_use(b)) == in_use, f"allocation {n}: a block was stranded"
            assert a.compare_counts(b, 2, 2) == exp
        same_table(b, tb)


def test_error_codes(two_tables):
    ta, _ = two_tables
    lib = _lib.load()
    cc = _lib.CountCompare()
    with counter(ta) as a, okm.KmerCounter(K, "set") as s, okm.KmerCounter(K - 2) as other_k, \
            okm.KmerCounter(40, wide=True) as w:
        s.add_pairs(np.arange(1, 50, dtype=np.uint64))
        ref = ctypes.byref(cc)
        for x, y, r, want in [(None, a.ctx, ref, _lib.OKM_E_ARG), (a.ctx, None, ref, _lib.OKM_E_ARG),
                              (a.ctx, a.ctx, None, _lib.OKM_E_ARG), (a.ctx, s.ctx, ref, _lib.OKM_E_STATE),
                              (s.ctx, a.ctx, ref, _lib.OKM_E_STATE), (a.ctx, other_k.ctx, ref, _lib.OKM_E_ARG),
                              (w.ctx, a.ctx, ref, _lib.OKM_E_ARG)]:
            assert lib.okm_compare_counts(x, y, 1, 1, r) == want
        if okm.device_count() > 1:
            with okm.KmerCounter(K, device=1) as far:
                assert lib.okm_compare_counts(a.ctx, far.ctx, 1, 1, ref) == _lib.OKM_E_ARG
        check(a, a, ta, ta)  # the table is as it was


@pytest.mark.parametrize("k", [21, 35])
def test_cli_compare(tmp_path, k):
    rng = np.random.default_rng(k)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = acgt[rng.integers(0, 4, 3000)]
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
    exp = expected(tables[0], tables[1], 2, 1)
    out, cmp_out = tmp_path / "out.tsv", tmp_path / "cmp.tsv"
    r = subprocess.run([_lib.CLI_PATH, "count", "-k", str(k), "-i", files[0], "-o", str(out), "-m", "2", "--compare",
                        files[1], "--compare-output", str(cmp_out)] + (["--wide"] if k > 32 else []),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = cmp_out.read_text().splitlines()
    assert os.path.getsize(out) > 0 and lines[:8] == [f"{f}\t{exp[f]}" for f in FIELDS]
    assert lines[8] == f"jaccard\t{exp['n_shared'] / (exp['n_a'] + exp['n_b'] - exp['n_shared']):.4f}"
    assert [x.split("\t")[0] for x in lines[9:]] == ["weighted_jaccard", "bray_curtis"]
