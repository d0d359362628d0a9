"""okm_count_histogram (the abundance spectrum) on the device, exact against
numpy: hist == bincount(minimum(C, n_bins - 1), minlength=n_bins) and summary
== {len(C), sum(C) mod 2^64, max(C)} for the count array C of numpy's (or the
oracle's) table.  The inputs are tests/hist_cases.py's (self-checked on the CPU
by tests/test_hist_cases.py).

The histogram is read from the table where it lies -- a count's pending
per-item runs (u32 or u64 counts), a dense device table, a host-resident table
in slices -- and must leave it there: the run's own kernel statistics show no
gather ("compact_items"), and every later reader gives the exact table."""

import ctypes
import os
import subprocess
import threading
from functools import lru_cache

import numpy as np
import pytest

import hist_cases as hc
import okm
from conftest import GOLDEN
from okm import _lib, testing
from oracle import OracleCounter, OracleCounterWide

pytestmark = pytest.mark.gpu

K = hc.K
BIG = 10**9


def _upload(arr):
    arr = np.ascontiguousarray(arr, dtype=np.uint64)
    buf = okm.DeviceBuffer(max(arr.nbytes, 8))
    if arr.nbytes:
        buf.upload(arr)
    return buf


def _check_hist(got, counts, n_bins):
    hist, sm = got
    assert hist.dtype == np.uint64 and len(hist) == n_bins
    assert np.array_equal(hist, hc.expected_hist(counts, n_bins))
    assert sm == hc.expected_summary(counts)
    assert hist[0] == 0 and int(hist.sum()) == len(counts)


def _same(got, expect):
    return np.array_equal(got[0], expect[0]) and np.array_equal(got[1], expect[1])


# ---------------------------------------------------------------------------
# pending table (the count's own runs), then the dense table
# ---------------------------------------------------------------------------

def _pending_then_dense(keys, n_bins=10001):
    ek, ec = hc.table_of(keys)
    with okm.KmerCounter(K) as c:
        c.set_timing(True)
        c.add_pairs(keys)
        assert c.count() == len(ek)
        first = c.count_histogram(n_bins)
        stats = c.kernel_stats()
        assert stats["count_histogram"]["launches"] == 1, sorted(stats)
        assert "compact_items" not in stats, sorted(stats)  # the pending table was not gathered
        assert stats["count_histogram"]["alg_bytes"] in (4.0 * len(ek), 8.0 * len(ek))  # counts only, no keys
        _check_hist(first, ec, n_bins)
        assert _same(c.result(1), (ek, ec))  # the reader after it: exact, and it gathers
        assert "compact_items" in c.kernel_stats()
        second = c.count_histogram(n_bins)  # now over the dense table
        stats = c.kernel_stats()
        assert stats["count_histogram"]["launches"] == 2 and stats["compact_items"]["launches"] == 1
        assert np.array_equal(second[0], first[0]) and second[1] == first[1]
        assert _same(c.result(1), (ek, ec))


@pytest.mark.parametrize("m", hc.ITEM_SIZES)
def test_pending_item_sizes(m):
    _pending_then_dense(hc.one_item(m))


def test_pending_many_items():
    _pending_then_dense(hc.many_items())
    _pending_then_dense(hc.many_items(), n_bins=151)  # half the counts in the last bin


def test_pending_u32_counts_from_reads():
    """A count from reads stages u32 counts: 4 B per distinct key are read."""
    batch = okm.synth_reads(20_000, 100, genome_len=300_000, genome_seed=5, seed=5)
    oc = OracleCounter(K)
    oc.add_separated(batch)
    ek, ec = oc.result(1)
    buf = okm.DeviceBuffer(len(batch), 0)
    buf.upload(batch)
    try:
        with okm.KmerCounter(K) as c:
            c.set_timing(True)
            c.add_device_batch(buf.address, len(batch))
            got = c.count_histogram(64)  # counts first, as okm_result_size does
            stats = c.kernel_stats()
            assert "compact_items" not in stats and stats["count_histogram"]["alg_bytes"] == 4.0 * len(ek)
            _check_hist(got, ec, 64)
            assert _same(c.result(1), (ek, ec))
    finally:
        buf.free()


@pytest.mark.parametrize("case", ["ones", "threes", "hot"])
def test_concentrated_spectra(case):
    keys = {"ones": lambda: hc.all_one_count(1), "threes": lambda: hc.all_one_count(3),
            "hot": hc.hot_among_singletons}[case]()
    _pending_then_dense(keys)
    if case == "hot":
        _pending_then_dense(keys, n_bins=4097)  # the hot key exactly in the last bin
        _pending_then_dense(keys, n_bins=4098)  # ... and one below it


# ---------------------------------------------------------------------------
# bin edges
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def edge_counter():
    keys, counts = hc.count_equals_index()
    c = okm.KmerCounter(K)
    c.add_pairs(keys, counts)
    assert c.count() == len(keys)
    yield c, hc.table_of(keys, counts)
    c.close()


@pytest.mark.parametrize("n_bins", hc.BIN_EDGE_NBINS)
def test_bin_edges(edge_counter, n_bins):
    c, (ek, ec) = edge_counter
    _check_hist(c.count_histogram(n_bins), ec, n_bins)


@pytest.mark.parametrize("n_bins", [0, 1, (1 << 20) + 2, 1 << 40])
def test_bad_n_bins(edge_counter, n_bins):
    c, (ek, ec) = edge_counter
    buf = np.zeros(4, np.uint64)
    assert _lib.load().okm_count_histogram(c.ctx, buf.ctypes.data, n_bins, None) == _lib.OKM_E_ARG
    assert _lib.load().okm_count_histogram(c.ctx, None, 16, None) == _lib.OKM_E_ARG
    if n_bins in (1, (1 << 20) + 2):
        with pytest.raises(okm.OkmError) as ei:
            c.count_histogram(n_bins)
        assert ei.value.status == _lib.OKM_E_ARG
    assert _same(c.result(1), (ek, ec))


def test_summary_may_be_null(edge_counter):
    c, (ek, ec) = edge_counter
    hist = np.zeros(100, np.uint64)
    _lib.check(_lib.load().okm_count_histogram(c.ctx, hist.ctypes.data, 100, None), "okm_count_histogram")
    assert np.array_equal(hist, hc.expected_hist(ec, 100))


# ---------------------------------------------------------------------------
# counts past 2^32
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("k", [31, 45])
def test_counts_past_u32(k):
    wide = k > 32
    runs, (ek, ec) = hc.past_u32_runs()
    bufs = []
    try:
        with okm.KmerCounter(k, wide=wide) as m:
            m.set_timing(True)
            for keys, counts in runs:
                kk = np.stack([keys, np.zeros_like(keys)], axis=1).reshape(-1) if wide else keys
                bk, bc = _upload(kk), _upload(counts)
                bufs += [bk, bc]
                m.add_sorted_pairs_device(bk.address, bc.address, len(keys))
            for n_bins in (10001, 3000, (1 << 20) + 1):
                hist, sm = m.count_histogram(n_bins)
                _check_hist((hist, sm), ec, n_bins)
                assert hist[n_bins - 1] == 2  # 6e9 and 5e9 both land in the last bin
            assert sm["max_count"] == 6_000_000_000
            assert sm["n_instances"] == sum(int(x) for x in ec)
            gk, gc = m.result(1)
            if wide:
                gk = gk.reshape(-1, 2)[:, 0]
            assert _same((gk, gc), (ek, ec))
    finally:
        for b in bufs:
            b.free()


# ---------------------------------------------------------------------------
# wide keys (k in 33..64): the direct count's dense u64 table, key-range groups
# ---------------------------------------------------------------------------

@lru_cache(maxsize=None)
def _ont(k):
    batch, _lens = okm.synth_long_reads(0.0006, 100_000, genome_seed=6, seed=6, median_len=300.0, min_len=100,
                                        max_len=3000)
    oc = OracleCounterWide(k)
    oc.add_separated(batch)
    return batch, oc.result(1)


WIDE_PATHS = {
    "direct": {},
    "groups_bound_table": {"group_keys": 50_000, "group_exact": 0},
    "groups_exact_tables": {"group_keys": 50_000, "group_exact": 1},
}


@pytest.mark.parametrize("path", list(WIDE_PATHS))
@pytest.mark.parametrize("k", [33, 63])
def test_wide(k, path):
    batch, (ek, ec) = _ont(k)
    assert 1000 < len(ek) and int(ec.max()) >= 3
    for name, v in WIDE_PATHS[path].items():
        testing.set_knob(name, v)
    buf = okm.DeviceBuffer(len(batch), 0)
    buf.upload(batch)
    try:
        with okm.KmerCounter(k, wide=True) as c:
            c.set_timing(True)
            c.add_device_batch(buf.address, len(batch))
            c.count()
            before = c.kernel_stats().get("compact_items", {"launches": 0})["launches"]
            for n_bins in (10001, 3):
                _check_hist(c.count_histogram(n_bins), ec, n_bins)
            # the histogram itself gathered nothing
            assert c.kernel_stats().get("compact_items", {"launches": 0})["launches"] == before
            if path != "direct":
                assert c.engine_info()["groups"] >= 3, c.engine_info()
            assert _same(c.result(1), (ek, ec))
    finally:
        buf.free()


# ---------------------------------------------------------------------------
# host-resident table: only its counts go up, in slices
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_batch():
    batch = okm.synth_reads(8_000, 100, genome_len=150_000, genome_seed=8, seed=8)
    oc = OracleCounter(K)
    oc.add_separated(batch)
    buf = okm.DeviceBuffer(len(batch), 0)
    buf.upload(batch)
    yield batch, buf, oc.result(1)
    buf.free()


def _to_host_table(c, expect):
    """The dense gather's first allocation fails: the table is gathered into
    mapped host memory and stays there."""
    testing.set_knob("fail_alloc", 1)
    assert _same(c.result(1), expect)
    assert testing.get_knob("fail_alloc") == -1, "the failure did not fire"
    assert c.engine_info()["host_bytes"] > 0


def test_host_resident_table_in_slices(small_batch):
    batch, buf, (ek, ec) = small_batch
    assert len(ek) > 3 * 4096 and len(ek) % 1000 and len(ek) % 4096
    with okm.KmerCounter(K) as c:
        c.set_timing(True)
        c.add_device_batch(buf.address, len(batch))
        c.count()
        _to_host_table(c, (ek, ec))
        launches = 0
        for sl in (1000, 4096, len(ek)):  # a ragged last slice, several slices, exactly one
            testing.set_knob("hist_slice", sl)
            _check_hist(c.count_histogram(10001), ec, 10001)
            launches += -(-len(ek) // sl)
            assert c.kernel_stats()["count_histogram"]["launches"] == launches
        testing.set_knob("hist_slice", -1)  # the product's slice: one here
        _check_hist(c.count_histogram(5), ec, 5)
        assert c.engine_info()["host_bytes"] > 0  # still host-resident
        assert _same(c.result(1), (ek, ec))
        assert c.engine_info()["host_bytes"] > 0


# ---------------------------------------------------------------------------
# every allocation of the histogram fails in turn
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("state", ["pending", "dense", "host"])
def test_every_allocation_fails_in_turn(small_batch, state):
    batch, buf, expect = small_batch
    ec = expect[1]
    n_bins = 300

    def prepare(c):
        c.reset()
        c.add_device_batch(buf.address, len(batch))
        c.count()
        if state == "dense":
            assert _same(c.result(1), expect)
        elif state == "host":
            _to_host_table(c, expect)
            testing.set_knob("hist_slice", 5000)

    def attempt(c, fail):
        testing.set_knob("fail_alloc", fail)
        try:
            return c.count_histogram(n_bins), None
        except okm.OkmError as e:
            return None, e
        finally:
            left[0] = testing.get_knob("fail_alloc")
            testing.set_knob("fail_alloc", -1)

    left = [0]
    with okm.KmerCounter(K) as c:
        prepare(c)
        got, err = attempt(c, BIG)
        assert err is None
        _check_hist(got, ec, n_bins)
        n_gets = BIG - left[0]
        print(f"{state}: {n_gets} allocations")
        assert n_gets == (2 if state == "host" else 1)  # the bins + summary words; the upload slice
        for n in range(1, n_gets + 1):
            prepare(c)
            in_use = testing.device_in_use(c)
            got, err = attempt(c, n)
            assert left[0] == -1, f"allocation {n}: the failure did not fire"
            if err is None:
                _check_hist(got, ec, n_bins)
            else:
                assert err.status == _lib.OKM_E_NOMEM, (n, err)
            assert testing.device_in_use(c) == in_use, f"allocation {n}: a block was stranded"
            if state == "host":
                assert c.engine_info()["host_bytes"] > 0
            _check_hist(c.count_histogram(n_bins), ec, n_bins)  # the table is intact: again, cleanly
            assert _same(c.result(1), expect)
            c.reset()
            assert testing.device_in_use(c) == 0 and c.engine_info()["host_bytes"] == 0


# ---------------------------------------------------------------------------
# other states
# ---------------------------------------------------------------------------

def test_before_any_batch_is_all_zeros():
    with okm.KmerCounter(K) as c:
        hist, sm = c.count_histogram(100)
        assert not hist.any() and sm == {"n_distinct": 0, "n_instances": 0, "max_count": 0}
        hist = np.full(7, 99, np.uint64)  # the caller's buffer is zeroed, whatever it held
        _lib.check(_lib.load().okm_count_histogram(c.ctx, hist.ctypes.data, 7, None), "okm_count_histogram")
        assert not hist.any()


def test_set_mode_has_no_counts():
    with okm.KmerCounter(K, "set") as c:
        c.add_pairs(np.arange(1, 100, dtype=np.uint64))
        with pytest.raises(okm.OkmError) as ei:
            c.count_histogram(100)
        assert ei.value.status == _lib.OKM_E_STATE
        keys, _ = c.result(1)
        assert np.array_equal(keys, np.arange(1, 100, dtype=np.uint64))


def test_folded_table():
    """count, then add: the first table becomes a weighted run of the second count."""
    a, b = hc.fold_pairs()
    ek, ec = hc.table_of(np.concatenate([a, b]))
    oc = OracleCounter(K)
    oc.add_pairs(*hc.table_of(a))
    oc.add_pairs(*hc.table_of(b))
    assert _same(oc.result(1), (ek, ec))
    with okm.KmerCounter(K) as c:
        c.add_pairs(a)
        c.count()
        _check_hist(c.count_histogram(50), hc.table_of(a)[1], 50)
        c.add_pairs(b)
        _check_hist(c.count_histogram(50), ec, 50)  # counts the pending batch first
        assert _same(c.result(1), (ek, ec))


def test_count_add_records_count():
    rng = np.random.default_rng(41)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = acgt[rng.integers(0, 4, 5000)]
    reads = [genome[o:o + 90].tobytes() for o in rng.integers(0, 4900, 1500)]
    oc = OracleCounter(K)
    with okm.KmerCounter(K) as c:
        c.add_records(reads[:700])
        oc.add_records(reads[:700])
        c.count()
        _check_hist(c.count_histogram(20), oc.result(1)[1], 20)
        c.add_records(reads[700:])
        oc.add_records(reads[700:])
        c.count()
        ek, ec = oc.result(1)
        _check_hist(c.count_histogram(20), ec, 20)
        _check_hist(c.count_histogram(10001), ec, 10001)
        assert _same(c.result(1), (ek, ec))


# ---------------------------------------------------------------------------
# groups and owners
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def group_reads():
    n, read_len = 12_000, 100
    batch = okm.synth_reads(n, read_len, genome_len=200_000, genome_seed=9, seed=9)
    recs = batch.reshape(n, read_len + 1)
    recs[::50, :read_len] = ord("A")  # a hot key
    batch = np.ascontiguousarray(recs).reshape(-1)
    with okm.KmerCounter(K) as c:  # the one-context histogram of the same reads
        buf = okm.DeviceBuffer(len(batch), 0)
        buf.upload(batch)
        c.add_device_batch(buf.address, len(batch))
        one = c.count_histogram(10001)
        table = c.result(1)
        buf.free()
    oc = OracleCounter(K)
    oc.add_separated(batch)
    assert _same(table, oc.result(1))
    _check_hist(one, table[1], 10001)
    return recs, one


def test_group_of_one_gpu(group_reads):
    """okm_group_count_histogram through a real group (one context per GPU;
    this test has one GPU: more ranks are covered through the loopback owners
    below, since a group of N needs N devices)."""
    recs, (ehist, esm) = group_reads
    lib = _lib.load()
    g = ctypes.c_void_p()
    _lib.check(lib.okm_group_create(ctypes.byref(g), K, 0, 1, None, 0), "okm_group_create")
    try:
        for part in np.array_split(recs, 3):
            seqs = [bytes(r[:-1]) for r in part]
            data, offs = okm.pack_records(seqs)
            _lib.check(lib.okm_group_add_batch(g, data.ctypes.data, offs.ctypes.data, len(offs) - 1, 0),
                       "okm_group_add_batch")
        hist = np.zeros(10001, np.uint64)
        sm = _lib.CountSummary()
        _lib.check(lib.okm_group_count_histogram(g, hist.ctypes.data, 10001, ctypes.byref(sm)),  # counts first
                   "okm_group_count_histogram")
        assert np.array_equal(hist, ehist)
        assert {f: int(getattr(sm, f)) for f, _ in _lib.CountSummary._fields_} == esm
        assert lib.okm_group_count_histogram(g, hist.ctypes.data, 1, None) == _lib.OKM_E_ARG
        assert lib.okm_group_count_histogram(g, None, 100, None) == _lib.OKM_E_ARG
        kp, cp, n = ctypes.POINTER(ctypes.c_uint64)(), ctypes.POINTER(ctypes.c_uint64)(), ctypes.c_uint64()
        _lib.check(lib.okm_group_finish_counts(g, 1, ctypes.byref(kp), ctypes.byref(cp), ctypes.byref(n)),
                   "okm_group_finish_counts")
        counts = np.ctypeslib.as_array(cp, shape=(n.value,)).copy()
        lib.okm_free_result(kp)
        lib.okm_free_result(cp)
        _check_hist((hist, esm), counts, 10001)
    finally:
        lib.okm_group_destroy(g)


def test_set_mode_group_has_no_counts():
    lib = _lib.load()
    g = ctypes.c_void_p()
    _lib.check(lib.okm_group_create(ctypes.byref(g), K, _lib.OKM_MODE_SET, 1, None, 0), "okm_group_create")
    try:
        hist = np.zeros(10, np.uint64)
        assert lib.okm_group_count_histogram(g, hist.ctypes.data, 10, None) == _lib.OKM_E_STATE
    finally:
        lib.okm_group_destroy(g)


@pytest.mark.parametrize("P", [2, 3])
def test_owners_of_a_loopback_merge_sum_to_the_whole(group_reads, P):
    """What okm_group_count_histogram does over N GPUs, on one: the owners of a
    P-rank merge hold disjoint key ranges, so their histograms, entries and
    instances add and the largest count is the largest of theirs."""
    recs, (ehist, esm) = group_reads
    testing.set_knob("loopback_timeout_ms", 60_000)
    shards = [np.ascontiguousarray(p).reshape(-1) for p in np.array_split(recs, P)]
    comms = okm.Comm.init_loopback(P, 0)
    out, err = [None] * P, [None] * P

    def rank(r):
        local, owner = okm.KmerCounter(K), okm.KmerCounter(K)
        buf = okm.DeviceBuffer(len(shards[r]))
        try:
            buf.upload(shards[r])
            local.add_device_batch(buf.address, len(shards[r]))
            comms[r].merge_owned(local, owner)
            out[r] = owner.count_histogram(10001)
        except BaseException as e:  # surfaced below
            err[r] = e
        finally:
            buf.free()
            local.close()
            owner.close()

    th = [threading.Thread(target=rank, args=(r,), daemon=True) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
        assert not t.is_alive(), "a virtual rank hung"
    for c in comms:
        c.close()
    for e in err:
        if e is not None:
            raise e
    assert np.array_equal(sum(h for h, _ in out), ehist)
    assert sum(s["n_distinct"] for _, s in out) == esm["n_distinct"]
    assert sum(s["n_instances"] for _, s in out) == esm["n_instances"]
    assert max(s["max_count"] for _, s in out) == esm["max_count"]
    assert all(s["n_distinct"] > 0 for _, s in out)


# ---------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------

def _cli(*args):
    return subprocess.run([_lib.CLI_PATH, *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("extra", [[], ["--gpus", "1"], ["-m", "2"], ["--histogram-max", "2"]])
def test_cli_histogram(tmp_path, extra):
    fa = os.path.join(GOLDEN, "data", "test_input1.fasta.gz")
    oc = OracleCounter(5)
    oc.add_records(okm.read_fastx_file(fa, True), normalized=True)
    ec = oc.result(1)[1]
    assert int(ec.max()) >= 3  # (a count past --histogram-max 2)
    n_bins = 3 if "--histogram-max" in extra else 10001
    plain, out, h = tmp_path / "plain.tsv", tmp_path / "out.tsv", tmp_path / "h.tsv"
    r = _cli("count", "-k", "5", "-i", fa, "-o", str(plain), *extra)
    assert r.returncode == 0, r.stderr
    r = _cli("count", "-k", "5", "-i", fa, "-o", str(out), "--histogram", str(h), *extra)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == plain.read_bytes() and len(plain.read_bytes()) > 0
    assert h.read_text() == hc.render_tsv(hc.expected_hist(ec, n_bins))  # the whole table, whatever --min-count


@pytest.mark.parametrize("wide", [False, True])
def test_cli_histogram_max_lumps_the_tail(tmp_path, wide):
    k = 35 if wide else 5
    rng = np.random.default_rng(43)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    read = acgt[rng.integers(0, 4, 80)].tobytes().decode()
    fa = tmp_path / "in.fa"
    fa.write_text("".join(f">r{i}\n{read}\n" for i in range(4)) + ">other\n" + "ACGT" * 15 + "\n")
    oc = (OracleCounterWide if wide else OracleCounter)(k)
    oc.add_records(okm.read_fastx_file(str(fa), True), normalized=True)
    ec = oc.result(1)[1]
    assert int(ec.max()) >= 3  # a count past the last bin
    plain, out, h = tmp_path / "plain.tsv", tmp_path / "out.tsv", tmp_path / "h.tsv.gz"
    flags = ["--wide"] if wide else []
    assert _cli("count", "-k", str(k), "-i", str(fa), "-o", str(plain), *flags).returncode == 0
    r = _cli("count", "-k", str(k), "-i", str(fa), "-o", str(out), "--histogram", str(h), "--histogram-max", "2",
             *flags)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == plain.read_bytes()
    import gzip
    exp = hc.expected_hist(ec, 3)
    assert exp[2] == int((ec >= 2).sum()) > 0
    assert gzip.decompress(h.read_bytes()).decode() == hc.render_tsv(exp)
