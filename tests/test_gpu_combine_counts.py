"""okm_combine_counts on the device: the output table exact against plain Python dicts, the inputs left as they were."""

import ctypes
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
T, TW = 1024, 512  # okm_combine.hip: a tile's entries, u64 / two-word keys
BIG = 10**9
OPS = tuple(_lib.COMBINE_OPS)
P = int(hc.PREFIX)


def expected(ta, tb, op, ma=1, mb=1):
    ka = {v: c for v, c in ta.items() if c >= max(ma, 1)}
    kb = {v: c for v, c in tb.items() if c >= max(mb, 1)}
    if op == "union":
        return {v: min(ka.get(v, 0) + kb.get(v, 0), M64) for v in ka.keys() | kb.keys()}
    if op in ("intersect", "intersect_left"):
        return {v: min(ka[v], kb[v]) if op == "intersect" else ka[v] for v in ka.keys() & kb.keys()}
    if op == "difference":
        return {v: c for v, c in ka.items() if v not in kb}
    return {v: c - kb.get(v, 0) for v, c in ka.items() if c > kb.get(v, 0)}


def same_table(c, table):
    gk, gc = c.result(1)
    keys = lc.from_pairs(gk) if c.wide else [int(v) for v in gk]
    assert dict(zip(keys, (int(x) for x in gc))) == table and keys == sorted(table)


def check(a, b, ta, tb, op, ma=1, mb=1):
    exp = expected(ta, tb, op, ma, mb)
    with a.combine(b, op, ma, mb) as out:
        assert out.count() == len(exp)
        cc = out.compare_counts(a)  # a second reader of the table, before the fetch
        same_table(out, exp)
        assert (cc["n_a"], cc["sum_a"], cc["n_shared"]) == (len(exp), sum(exp.values()) & M64, len(exp.keys() & ta.keys()))
    return exp


def check_ops(a, b, ta, tb):
    for op in OPS:
        check(a, b, ta, tb, op)
        check(b, a, tb, ta, op)
    same_table(a, ta)  # the inputs stayed (this reader gathers a pending table: last)
    same_table(b, tb)


def table_of(keys, counts=None):
    ek, ec = hc.table_of(keys, counts)
    return dict(zip((int(v) for v in ek), (int(c) for c in ec)))


def counter(table, k=K, weighted=False, dense=False):
    keys = sorted(table)
    c = okm.KmerCounter(k, wide=k > 32)
    c.set_timing(True)
    arr = lc.to_pairs(keys) if k > 32 else np.array(keys, np.uint64)
    if weighted:
        c.add_pairs(arr, np.array([table[v] for v in keys], np.uint64))
    else:
        c.add_pairs(np.repeat(arr, [table[v] for v in keys], axis=0))
    assert c.count() == len(table)
    if dense:
        same_table(c, table)
    return c


def launches(c, name="compact_items"):
    return c.kernel_stats().get(name, {"launches": 0})["launches"]


def run_edges(runs, present):
    ends = {int(r[i]) for r in runs for i in (0, -1)}
    return sorted(ends | {w for v in ends for w in (v - 1, v + 1) if w not in present and w >= 0})


@pytest.mark.parametrize("dense_a,dense_b", [(False, False), (False, True), (True, False), (True, True)])
def test_representation_pairs(dense_a, dense_b):
    runs, inp = lc.items()
    ta = table_of(inp)
    tb = {v: 1 + i % 4 for i, v in enumerate(run_edges(runs, ta))}  # B: the edges of A's runs, their absent neighbours
    tb.update({int(v): 2 for v in hc.many_items()[:500]})           # ... and keys all over the key space
    with counter(ta, dense=dense_a) as a, counter(tb, dense=dense_b) as b:
        before = launches(a), launches(b)
        assert before == (int(dense_a), int(dense_b))  # an unweighted count leaves a pending table
        for op in OPS:
            check(a, b, ta, tb, op)
            check(b, a, tb, ta, op)
        assert (launches(a), launches(b)) == before  # the combine gathered nothing
        assert launches(a, "combine_counts") == len(OPS)
        same_table(a, ta)
        same_table(b, tb)


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("k,m", [(k, t + d) for k, t in ((K, T), (64, TW)) for d in (-t, 1 - t, -1, 0, 1, t + 1)])
def test_run_and_tile_edges(k, m, dense):
    """A: m keys under one prefix between two populated ranges; B: the edges of A's runs, every other count past 2^32."""
    ta = table_of(hc.one_item(m))
    keys = np.array(sorted(ta), np.uint64)
    runs = [keys[(keys >> np.uint64(hc.LOW_BITS)) == (p >> np.uint64(hc.LOW_BITS))]
            for p in (hc.PREFIX_BELOW, hc.PREFIX, hc.PREFIX_ABOVE)]
    edges = run_edges([r for r in runs if len(r)], ta) + [P + 5, P - 1 + (1 << hc.LOW_BITS)]
    tb = {v: (5_000_000_000 if i % 2 else 1 + i % 7) for i, v in enumerate(sorted(set(edges)))}
    if k > 32:  # the same keys in the high word: neighbours differ in one word only
        ta = {v << 64 | 7: c for v, c in ta.items()}
        tb = {**{v << 64 | 7: c for v, c in tb.items()}, **{v << 64 | 6: 3 for v in list(tb)[::2]}}
    with counter(ta, k, dense=dense) as a, counter(tb, k, weighted=True, dense=dense) as b:
        check_ops(a, b, ta, tb)


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("k", [K, 64])
def test_s_only_entries_everywhere(k, dense):
    """S below D, above it, between two D runs; 3T + 5 (several chunks) in one gap and under one tile's span; both ways."""
    t = TW if k > 32 else T
    rng = np.random.default_rng(k)
    low = np.sort(hc._distinct_low(rng, 3 * t + 5))
    lo, hi = P | int(low[0]), P | int(low[-1])
    ts = {P | int(v): 1 + i % 5 for i, v in enumerate(low[1:])}  # under the span of D's tile (lo, hi); hi is shared
    ts.update({0x2B0 << hc.LOW_BITS | int(v): 1 + i % 3 for i, v in enumerate(low)})  # a gap of D, many chunks
    ts.update({0x001 << hc.LOW_BITS | i: 2 for i in range(5)})
    ts.update({0x3F0 << hc.LOW_BITS | i: 5_000_000_000 for i in range(5)})
    ts.update({0x2A5 << hc.LOW_BITS | int(low[-1]) + 1 + i: 3 for i in range(3)})  # just behind a tile's last key
    td = {lo: 3, hi: 2}
    for p in (int(hc.PREFIX_BELOW), int(hc.PREFIX_ABOVE), 0x300 << hc.LOW_BITS):
        td.update({p | int(v): 1 + i % 2 for i, v in enumerate(hc._distinct_low(rng, 3 * t + 9))})
    assert len(td) > len(ts)
    if k > 32:
        td, ts = ({v << 64 | (v & 0xFFFF): c for v, c in x.items()} for x in (td, ts))
    with counter(td, k, dense=dense) as d, counter(ts, k, weighted=True, dense=dense) as s:
        check_ops(d, s, td, ts)


@pytest.mark.parametrize("case", ["self", "copy", "disjoint", "subtract"])
def test_nothing_emitted(case):
    ta = table_of(hc.one_item(2 * T + 1))
    tb = {"disjoint": {v + 1: c for v, c in ta.items() if v + 1 not in ta},
          "subtract": {v: c + i % 2 for i, (v, c) in enumerate(ta.items())}}.get(case, ta)
    op = {"disjoint": "intersect", "subtract": "subtract"}.get(case, "difference")
    n = ctypes.c_uint64(7)
    with counter(ta) as a, counter(tb) as other, okm.KmerCounter(K) as out:
        b = a if case == "self" else other  # a == b, or an equal copy
        assert _lib.load().okm_combine_counts(a.ctx, b.ctx, _lib.COMBINE_OPS[op], 1, 1, out.ctx, ctypes.byref(n)) == 0
        assert (n.value, out.count()) == (0, 0) and expected(ta, tb, op) == {}
        same_table(out, {})
        assert out.count_histogram(4)[1] == {"n_distinct": 0, "n_instances": 0, "max_count": 0}
        out.add_pairs(np.array([5, 5, 9], np.uint64))
        for c, t in ((out, {5: 2, 9: 1}), (a, ta), (b, tb)):  # the later add works; both inputs stayed
            same_table(c, t)


@pytest.mark.parametrize("k", [33, 48, 64])
@pytest.mark.parametrize("dense", [False, True])
def test_wide_word_neighbours(k, dense):
    ta, queries = lc.word_neighbours(k)
    tb = {v: 1 + v % 3 for v in queries[::2] if 0 <= v < (1 << (2 * k)) - 1}  # keys of A and their one-word neighbours
    with counter(ta, k, dense=dense) as a, counter(tb, k, weighted=True, dense=dense) as b:
        check_ops(a, b, ta, tb)


@pytest.mark.parametrize("op", OPS)
def test_counts_and_thresholds(op):
    rng = np.random.default_rng(3)
    keys = [int(v) for v in np.unique(rng.integers(0, 1 << 62, 6000, dtype=np.uint64))]
    ta = {v: 1 + i % 6 for i, v in enumerate(keys[:5000])}
    tb = {v: 1 + i % 4 for i, v in enumerate(keys[1000:])}
    huge = {keys[0]: M64 - 5, keys[1]: 9, keys[2]: 4, keys[3]: 5, keys[4]: 6}  # union: 2^64 - 1; a - b: -1, 0, 1
    nine = {keys[0]: 9, keys[1]: M64 - 5, keys[2]: 5, keys[3]: 5, keys[4]: 5}
    with counter(ta) as a, counter(tb, dense=True) as b, counter(huge, weighted=True) as h, \
            counter(nine, weighted=True) as g, okm.KmerCounter(K) as never, counter({}) as empty:
        for e in (never, empty):  # a never-fed and a counted-empty context, on either side
            check(a, e, ta, {}, op, 2, 1)
            check(e, a, {}, ta, op, 1, 2)
        check(never, empty, {}, {}, op)
        for ma, mb in [(0, 0), (1, 1), (3, 1), (4, 1), (1, 4), (1, 5), (6, 4), (7, 1), (2, BIG)]:
            check(a, b, ta, tb, op, ma, mb)  # counts == min, min - 1 on each side; 7 / 5 / BIG keep nothing
            check(b, a, tb, ta, op, mb, ma)
        exp = check(h, g, huge, nine, op)
        assert op != "union" or exp[keys[0]] == exp[keys[1]] == M64
        assert op != "subtract" or exp == {keys[0]: M64 - 14, keys[4]: 1}


def test_output_is_a_table():
    ta, tb = table_of(hc.one_item(T + 1)), table_of(hc.many_items()[:4000])
    extra = {**{v: 2 for v in list(ta)[::3]}, 12345: 1}
    with counter(ta) as a, counter(tb) as b, a.combine(b, "union") as out:
        out.add_pairs(np.repeat(np.array(sorted(extra), np.uint64), [extra[v] for v in sorted(extra)]))
        both = expected(expected(ta, tb, "union"), extra, "union")
        assert out.count() == len(both)  # res_is_input: the add went on top of the table
        same_table(out, both)
        check(out, a, both, ta, "difference")  # and it chains


def attempt(a, b, out, fail):
    testing.set_knob("fail_alloc", fail)
    try:
        a.combine(b, "union", 2, 2, out=out)
        err = None
    except okm.OkmError as e:
        err = e
    left = testing.get_knob("fail_alloc")
    testing.set_knob("fail_alloc", -1)
    return err, left


def test_host_resident_input_then_every_allocation_fails_in_turn():
    rng = np.random.default_rng(9)
    keys = [int(v) for v in np.unique(rng.integers(0, 1 << 62, 14_000, dtype=np.uint64))]
    ta = {v: 1 + i % 5 for i, v in enumerate(keys[:11_003])}
    tb = {v: 1 + i % 3 for i, v in enumerate(keys[4_000:])}
    exp = expected(ta, tb, "union", 2, 2)
    with counter(ta) as a, counter(tb) as b, okm.KmerCounter(K) as out:
        testing.set_knob("fail_alloc", 1)  # the dense gather's first allocation fails: b's table stays on the host
        same_table(b, tb)
        assert b.engine_info()["host_bytes"] > 0  # ... and the first combine moves it to the device
        check(a, b, ta, tb, "subtract", 2, 1)
        err, left = attempt(a, b, out, BIG)
        assert err is None
        same_table(out, exp)
        for n in range(1, BIG - left + 1):
            in_use = testing.device_in_use(a), testing.device_in_use(b)
            err, left = attempt(a, b, out, n)
            assert left == -1, f"allocation {n}: the failure did not fire"
            assert err is None or (err.status == _lib.OKM_E_NOMEM and out.count() == 0), (n, err)
            assert (testing.device_in_use(a), testing.device_in_use(b)) == in_use, f"allocation {n}: a block was stranded"
            if err is not None:
                a.combine(b, "union", 2, 2, out=out)  # the next call is exact
            same_table(out, exp)
        same_table(a, ta)
        same_table(b, tb)


def test_error_codes():
    ta, ARG, STATE = table_of(hc.one_item(T + 1)), _lib.OKM_E_ARG, _lib.OKM_E_STATE
    with counter(ta) as a, counter(ta) as b, okm.KmerCounter(K) as out, okm.KmerCounter(K, "set") as s, \
            okm.KmerCounter(K - 2) as other_k, okm.KmerCounter(40, wide=True) as w:
        s.add_pairs(np.arange(1, 50, dtype=np.uint64))
        for x, y, op, o, want in [(None, b, 0, out, ARG), (a, None, 0, out, ARG), (a, b, 0, None, ARG),
                                  (a, b, 0, a, ARG), (a, b, 0, b, ARG), (a, b, 5, out, ARG), (a, b, -1, out, ARG),
                                  (s, b, 0, out, STATE), (a, s, 0, out, STATE), (a, b, 0, s, STATE),
                                  (other_k, b, 0, out, ARG), (a, other_k, 0, out, ARG), (a, b, 0, other_k, ARG),
                                  (a, b, 0, w, ARG), (w, w, 0, out, ARG)]:
            ctx = [c and c.ctx for c in (x, y, o)]
            assert _lib.load().okm_combine_counts(ctx[0], ctx[1], op, 1, 1, ctx[2], None) == want, (op, want)
        check(a, a, ta, ta, "intersect")  # the table is as it was


def cli(*args):
    return subprocess.run([_lib.CLI_PATH, "count", *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("k,op", [(21, "subtract"), (35, "union")])
def test_cli_combine(tmp_path, k, op):
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
    exp, cmb = expected(tables[0], tables[1], op, 2, 3), tmp_path / "cmb.tsv"
    r = cli("-k", str(k), "-i", files[0], "-o", str(tmp_path / "out.tsv"), "-m", "2", "--combine", files[1], "--combine-op", op,
            "--combine-output", str(cmb), "--combine-min-count", "3", *(["--wide"] if k > 32 else []))
    assert r.returncode == 0, r.stderr
    rows = [ln.split("\t") for ln in cmb.read_text().splitlines()]
    got = {sum("ACGT".index(ch) << 2 * (k - 1 - j) for j, ch in enumerate(m)): int(c) for m, c in rows}
    assert got == exp and len(rows) == len(exp) > 0 and [m for m, _ in rows] == sorted(m for m, _ in rows)


FULL = ["--combine", "x.fa", "--combine-op", "union", "--combine-output", "y.tsv"]


@pytest.mark.parametrize("args,said", [
    (FULL[:2], "--combine-op <OP>"), (FULL[:4], "--combine-output <FILE>"), (FULL[4:], "--combine <FASTX>"),
    (["--combine-min-count", "2"], "--combine <FASTX>"),
    (FULL[:3] + ["xor"] + FULL[4:], "invalid value 'xor' for '--combine-op <OP>'"),
    (FULL + ["--combine-min-count", "two"], "invalid value 'two' for '--combine-min-count <N>'"),
    (FULL + ["--gpus", "2"], "'--combine <FASTX>' cannot be used with '--gpus <GPUS>'")])
def test_cli_usage_errors_and_help(args, said):
    r = cli("-k", "21", "-i", "in.fa", "-o", "out.tsv", *args)
    assert r.returncode == 2 and said in r.stderr
    text = cli("--help").stdout
    for flag in ("--combine <FASTX>", "--combine-op <OP>", "--combine-output <FILE>", "--combine-min-count <N>"):
        assert text.count("  " + flag) == 1
