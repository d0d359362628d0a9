"""okm_read_depths (per-record k-mer depth against the counted table) on the
device, exact against plain Python: per record normalise, enumerate the
windows, canonicalise with the codec functions, look up in a dict, reduce
(tests/depth_cases.py, self-checked on the CPU by tests/test_depth_cases.py).

The table is searched where it lies -- a count's pending per-item runs (u32 or
u64 counts), a dense device table, a host-resident table in slices -- and must
stay there.  Every case runs the host form and the device form; the device
form also without the last separator and with valid bases behind n_bytes."""

import ctypes
import gzip
import subprocess
import threading
from functools import lru_cache

import numpy as np
import pytest

import depth_cases as dc
import okm
from okm import _lib, testing

pytestmark = pytest.mark.gpu

BIG = 10**9
JUNK = 0x77  # what the output buffers hold before a call: every row is written


def _rows(rows):
    return [tuple(int(x) for x in r) for r in rows]


def _host(c, recs, min_count=2, normalized=False, wrapper=True):
    data, offs = okm.pack_records(list(recs))
    out = np.full(len(recs) * 6, JUNK, np.uint64).view(okm.READ_DEPTH_DTYPE)
    _lib.check(_lib.load().okm_read_depths(c.ctx, data.ctypes.data, offs.ctypes.data, len(recs), 1 if normalized else 0,
                                           min_count, out.ctypes.data), "okm_read_depths")
    if wrapper:
        assert np.array_equal(out, c.read_depths(recs, min_count, normalized))
    return out


def _device(c, batch, nrec, min_count=2, behind=b"", shift=0):
    """The device form over `batch` (bytes); `behind`: bytes that lie in the
    buffer after n_bytes; shift: the batch starts this far into the buffer
    (not 16-byte aligned when shift % 16)."""
    raw = np.frombuffer(b"G" * shift + batch + behind, dtype=np.uint8)
    dseq = okm.DeviceBuffer(max(len(raw), 16))
    dout = okm.DeviceBuffer(max(nrec, 1) * 48)
    try:
        if len(raw):
            dseq.upload(raw)
        dout.upload(np.full(max(nrec, 1) * 6, JUNK, np.uint64))
        c.read_depths_device(dseq.address + shift, len(batch), nrec, dout.address, min_count)
        out = np.empty(nrec, okm.READ_DEPTH_DTYPE)
        if nrec:
            dout.download(out)
        return out
    finally:
        dseq.free()
        dout.free()


def _check(c, recs, exp, min_count=2, k=None):
    """Host form (normalized = 0) and device forms of the records against exp."""
    got = _host(c, recs, min_count)
    assert _rows(got) == _rows(exp)
    tail = b"ACGT" * 40  # valid bases behind n_bytes: never looked at
    assert _rows(_device(c, dc.device_batch(recs), len(recs), min_count)) == _rows(exp)
    assert _rows(_device(c, dc.device_batch(recs, terminate_last=False), len(recs), min_count, behind=tail)) == _rows(exp)
    return got


def _launches(c, name):
    return c.kernel_stats().get(name, {"launches": 0})["launches"]


def _table(c):
    return dc.table_of_result(*c.result(1), c.wide)


def _count_reads(c, recs):
    c.add_records(list(recs))
    return c.count()


# ---------------------------------------------------------------------------
# record geometry at every k, against the pending table and then the dense one
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("k", dc.KS)
def test_record_geometry(k):
    recs, names = dc.geometry(k)
    table, exp = dc.geometry_expected(k)
    with okm.KmerCounter(k, wide=k > 32) as c:
        c.set_timing(True)
        assert _count_reads(c, dc.table_reads()) == len(table)  # a count from reads: pending, u32 counts
        before = _launches(c, "compact_items")
        first = _check(c, recs, exp)
        stats = c.kernel_stats()
        assert _launches(c, "compact_items") == before  # the pending table was not gathered
        assert stats["read_depths"]["launches"] == 4  # _host scans twice, _check's device forms once each
        nb = len(dc.device_batch(recs))
        assert stats["read_depths"]["alg_bytes"] == 4 * (nb + 48.0 * len(recs)) - 1  # (one batch without its last separator)
        # shifted by a byte the batch is not 16-byte aligned: it goes through scratch
        assert _rows(_device(c, dc.device_batch(recs), len(recs), shift=1)) == _rows(exp)
        # fewer rows than records: the later records are dropped; more: they stay zero
        assert _rows(_device(c, dc.device_batch(recs), 80)) == _rows(exp[:80])
        more = _device(c, dc.device_batch(recs), len(recs) + 3)
        assert _rows(more[:len(recs)]) == _rows(exp) and _rows(more[len(recs):]) == [(0,) * 6] * 3
        assert _table(c) == table  # the reader after it: exact, and it gathers
        after = _launches(c, "compact_items")
        if k == 31:
            assert (before, after) == (0, 1)  # the table was still pending
        second = _check(c, recs, exp)  # now over the dense table
        assert np.array_equal(first, second)
        assert _launches(c, "compact_items") == after
        # the normalised bytes with normalized = 1 are the same records
        norm = [dc.normalize(r) for r in recs]
        assert _rows(_host(c, norm, normalized=True)) == _rows(exp)


def test_k32_with_key_zero():
    """k = 32 fills the key word: all-A (and all-T) is key 0, and nothing is 2^64 - 1."""
    k = 32
    reads = [b"A" * 40, b"T" * 35, dc.genome()[:100]]
    table = dc.table_of_records(reads, k)
    assert table[0] == 9 + 4 and len(table) == 1 + 69
    recs = [b"A" * 33, b"T" * 32 + b"C", b"a" * 31, dc.genome()[50:130], b"C" * 40, b"AAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAG" * 2]
    exp = dc.expected(recs, k, table)
    assert _rows(exp[:3]) == [(2, 2, 2, 26, 13, 13), (2, 1, 1, 13, 13, 13), (0,) * 6]
    with okm.KmerCounter(k) as c:
        assert _count_reads(c, reads) == len(table)
        _check(c, recs, exp)
        assert _table(c) == table
        _check(c, recs, exp)


# ---------------------------------------------------------------------------
# the table's representations
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("k", [31, 37])
def test_pending_u64_counts_and_a_wrapping_sum(k):
    keys, counts, recs, table = dc.big_count_pairs(k)
    exp = dc.expected(recs, k, table, min_count=(1 << 32) + 8)
    assert 0 < int(exp[0]["solid"]) < int(exp[0]["present"])
    with okm.KmerCounter(k, wide=k > 32) as c:
        c.set_timing(True)
        c.add_pairs(dc.pairs_input(keys, k > 32), np.array(counts, dtype=np.uint64))  # weighted: u64 counts
        assert c.count() == len(table)
        got = _check(c, recs, exp, min_count=(1 << 32) + 8)
        assert int(got[2]["sum"]) == 7 and int(got[2]["max"]) == (1 << 63) + 4  # 2^64 + 7 wrapped
        assert int(got[0]["sum"]) > 1 << 36
        assert "compact_items" not in c.kernel_stats()
        assert _table(c) == table
        _check(c, recs, exp, min_count=(1 << 32) + 8)


@lru_cache(maxsize=None)
def _small():
    """Reads, their table at k = 31 and the rows of a sample of them (and of
    the geometry records) against it."""
    k = 31
    batch = okm.synth_reads(1200, 100, genome_len=40_000, genome_seed=8, seed=8)
    reads = [bytes(r[:-1]) for r in batch.reshape(1200, 101)]
    table = dc.table_of_records(reads, k, normalized=True)
    recs = list(reads[::40]) + [dc.genome()[:200], b"", reads[7][:30], reads[9][:60] + b"N" + reads[11][10:]]
    return k, batch, table, tuple(recs), dc.expected(recs, k, table)


def _to_host_table(c, table):
    """The dense gather's first allocation fails: the table is gathered into
    mapped host memory and stays there."""
    testing.set_knob("fail_alloc", 1)
    assert _table(c) == table
    assert testing.get_knob("fail_alloc") == -1, "the failure did not fire"
    assert c.engine_info()["host_bytes"] > 0


def test_host_resident_table_in_slices():
    k, batch, table, recs, exp = _small()
    n = len(table)
    assert n > 3 * 4096 and n % 1000 and n % 4096 and any(r["present"] for r in exp) and any(r["windows"] > r["present"] for r in exp)
    with okm.KmerCounter(k) as c:
        c.set_timing(True)
        c.add_records([bytes(r[:-1]) for r in batch.reshape(1200, 101)], normalized=True)
        c.count()
        _to_host_table(c, table)
        launches = 0
        try:
            for sl in (1000, 4096, n):  # a ragged last slice, several slices, exactly one
                testing.set_knob("hist_slice", sl)
                assert c.engine_info()["host_bytes"] > 0
                _check(c, recs, exp)
                launches += 4 * -(-n // sl)  # one per slice, for two host calls and two device ones
                assert _launches(c, "read_depths") == launches
                assert c.engine_info()["host_bytes"] > 0  # still host-resident
            # slices and chunks together: every slice scans every chunk
            testing.set_knob("hist_slice", 4096)
            testing.set_knob("depth_chunk", 700)
            assert _rows(_host(c, recs, wrapper=False)) == _rows(exp)
        finally:
            testing.set_knob("hist_slice", -1)
            testing.set_knob("depth_chunk", -1)
        _check(c, recs, exp)  # the product's slice: one here
        assert _launches(c, "compact_items") == 1  # _to_host_table's
        assert _table(c) == table and c.engine_info()["host_bytes"] > 0


def test_folded_table():
    """count, then add: the first table becomes a weighted run of the second count."""
    k = 31
    a, b = dc.table_reads()[:30], dc.table_reads()[20:]
    recs, _ = dc.geometry(k)
    recs = recs[70:]
    ta, tab = dc.table_of_records(a, k), dc.table_of_records(a + b, k)
    with okm.KmerCounter(k) as c:
        _count_reads(c, a)
        first = _check(c, recs, dc.expected(recs, k, ta))
        c.add_records(list(b))
        second = _check(c, recs, dc.expected(recs, k, tab))  # counts the pending batch first
        assert not np.array_equal(first, second)
        assert _table(c) == tab


WIDE_PATHS = {
    "direct": {},
    "groups_bound_table": {"group_keys": 50_000, "group_exact": 0},
    "groups_exact_tables": {"group_keys": 50_000, "group_exact": 1},
}


@lru_cache(maxsize=None)
def _ont(k):
    batch, _lens = okm.synth_long_reads(0.0002, 100_000, genome_seed=6, seed=6, median_len=300.0, min_len=100,
                                        max_len=3000)
    raw = batch.tobytes()
    reads = raw.split(b"\n")
    if reads and reads[-1] == b"":
        reads.pop()
    table = dc.table_of_records(reads, k, normalized=True)
    recs = tuple(reads[::17][:40]) + (dc.genome()[:300], reads[3][:k - 1], reads[5][:k])
    return batch, table, recs, dc.expected(recs, k, table)


@pytest.mark.parametrize("path", list(WIDE_PATHS))
@pytest.mark.parametrize("k", [33, 37, 63, 64])
def test_wide_paths(k, path):
    """The wide count paths tests/test_gpu_lookup_counts.py::test_wide_paths forces."""
    batch, table, recs, exp = _ont(k)
    assert 1000 < len(table) and max(table.values()) >= 2
    buf = okm.DeviceBuffer(len(batch), 0)
    buf.upload(batch)
    try:
        with testing.knobs(**WIDE_PATHS[path]), okm.KmerCounter(k, wide=True) as c:
            c.set_timing(True)
            c.add_device_batch(buf.address, len(batch))
            c.count()
            before = _launches(c, "compact_items")
            got = _check(c, recs, exp)
            assert int(got["max"].max()) >= 2 and int(got[-3]["present"]) == 0 < int(got[-3]["windows"])
            assert _launches(c, "compact_items") == before  # the call itself gathered nothing
            if path != "direct":
                assert c.engine_info()["groups"] >= 3, c.engine_info()
            assert _table(c) == table
    finally:
        buf.free()


# ---------------------------------------------------------------------------
# in place
# ---------------------------------------------------------------------------

def test_later_readers_see_what_they_would_have():
    k, batch, table, recs, exp = _small()
    keys = np.array(sorted(table)[::7], dtype=np.uint64)

    def readers(c, depths):
        c.add_records([bytes(r[:-1]) for r in batch.reshape(1200, 101)], normalized=True)
        c.count()
        if depths:
            _check(c, recs, exp)
            assert "compact_items" not in c.kernel_stats()
        look = c.lookup(keys)
        hist, summary = c.count_histogram(100)
        assert "compact_items" not in c.kernel_stats()  # the table is still pending for all of them
        res = c.result(1)
        assert _launches(c, "compact_items") == 1
        return look, hist, summary, res

    with okm.KmerCounter(k) as c, okm.KmerCounter(k) as d:
        c.set_timing(True)
        d.set_timing(True)
        with_call, without = readers(c, True), readers(d, False)
        assert np.array_equal(with_call[0], without[0]) and np.array_equal(with_call[1], without[1])
        assert with_call[2] == without[2]
        assert np.array_equal(with_call[3][0], without[3][0]) and np.array_equal(with_call[3][1], without[3][1])
        assert dc.table_of_result(*with_call[3], False) == table


# ---------------------------------------------------------------------------
# self-consistency on synthetic reads
# ---------------------------------------------------------------------------

def test_reads_against_their_own_table():
    k, n, ln = 31, 2000, 150
    batch = okm.synth_reads(n, ln, genome_len=60_000, genome_seed=12, seed=12)
    buf = okm.DeviceBuffer(len(batch), 0)
    buf.upload(batch)
    try:
        with okm.KmerCounter(k) as c:
            c.add_device_batch(buf.address, len(batch))
            dev = _device(c, batch.tobytes(), n, min_count=1)
            host = _host(c, [bytes(r[:-1]) for r in batch.reshape(n, ln + 1)], min_count=1, normalized=True)
            assert np.array_equal(dev, host)
            assert np.array_equal(dev["present"], dev["windows"]) and np.array_equal(dev["solid"], dev["windows"])
            assert int(dev["windows"].max()) == ln - k + 1 and int(dev["min"].min()) >= 1
            _hist, summary = c.count_histogram(100)
            assert int(dev["windows"].sum()) == summary["n_instances"]
            keys, counts = c.result(1)
            assert int(dev["sum"].sum()) == int((counts.astype(object) ** 2).sum())  # every key c times, c each time
            assert int(dev["max"].max()) == int(counts.max())
    finally:
        buf.free()


# ---------------------------------------------------------------------------
# min_count
# ---------------------------------------------------------------------------

def test_min_count():
    k = 31
    recs, _ = dc.geometry(k)
    recs = recs[70:]
    table = dc.table_of_records(dc.table_reads(), k)
    top = max(table.values())
    with okm.KmerCounter(k) as c:
        _count_reads(c, dc.table_reads())
        for state in ("pending", "dense"):
            at1 = _check(c, recs, dc.expected(recs, k, table, 1), min_count=1)
            assert np.array_equal(at1["solid"], at1["present"]) and at1["present"].sum() > 0
            attop = _check(c, recs, dc.expected(recs, k, table, top), min_count=top)
            assert 0 < attop["solid"].sum() < at1["solid"].sum()
            above = _check(c, recs, dc.expected(recs, k, table, top + 1), min_count=top + 1)
            assert not above["solid"].any() and np.array_equal(above["present"], at1["present"])
            at0 = _check(c, recs, dc.expected(recs, k, table, 0), min_count=0)  # every present window
            assert np.array_equal(at0["solid"], at0["present"])
            assert _table(c) == table


# ---------------------------------------------------------------------------
# host records go up in chunks of whole records
# ---------------------------------------------------------------------------

def test_host_records_cross_the_chunks():
    k = 31
    recs = dc.chunk_records()
    table = dc.table_of_records(dc.table_reads(), k)
    exp = dc.expected(recs, k, table)
    nchunks = len(dc.chunks_of(recs, dc.CHUNK_BYTES))
    with okm.KmerCounter(k) as c:
        c.set_timing(True)
        _count_reads(c, dc.table_reads())
        for state in ("pending", "dense"):
            whole = _host(c, recs, wrapper=False)
            assert _rows(whole) == _rows(exp)
            n0 = _launches(c, "read_depths")
            with testing.knobs(depth_chunk=dc.CHUNK_BYTES):
                in_use = testing.device_in_use(c)
                assert np.array_equal(_host(c, recs, wrapper=False), whole)
                assert _launches(c, "read_depths") == n0 + nchunks
                assert testing.device_in_use(c) == in_use
            with testing.knobs(depth_chunk=1):  # one record per chunk
                assert np.array_equal(_host(c, recs, wrapper=False), whole)
                assert _launches(c, "read_depths") == n0 + nchunks + len(recs)
            assert _table(c) == table


# ---------------------------------------------------------------------------
# groups and owners
# ---------------------------------------------------------------------------

@lru_cache(maxsize=None)
def _group_reads():
    k, n, ln = 31, 3000, 100
    batch = okm.synth_reads(n, ln, genome_len=50_000, genome_seed=9, seed=9)
    recs = batch.reshape(n, ln + 1)
    reads = [bytes(r[:-1]) for r in recs]
    table = dc.table_of_records(reads, k, normalized=True)
    q = tuple(reads[::60]) + (dc.genome()[:150], b"", reads[1][:50] + dc.genome()[200:260] + reads[2][30:])
    return k, recs, table, q, dc.expected(q, k, table)


def test_group_of_one_gpu():
    """okm_group_read_depths through a real group (one context per GPU; this
    test has one GPU: more ranks are covered through the loopback owners
    below, since a group of N needs N devices)."""
    k, recs, table, q, exp = _group_reads()
    lib = _lib.load()
    g = ctypes.c_void_p()
    _lib.check(lib.okm_group_create(ctypes.byref(g), k, 0, 1, None, 0), "okm_group_create")
    try:
        for part in np.array_split(recs, 3):
            data, offs = okm.pack_records([bytes(r[:-1]) for r in part])
            _lib.check(lib.okm_group_add_batch(g, data.ctypes.data, offs.ctypes.data, len(offs) - 1, 1),
                       "okm_group_add_batch")
        data, offs = okm.pack_records(list(q))
        out = np.full(len(q) * 6, JUNK, np.uint64).view(okm.READ_DEPTH_DTYPE)
        _lib.check(lib.okm_group_read_depths(g, data.ctypes.data, offs.ctypes.data, len(q), 0, 2, out.ctypes.data),  # counts first
                   "okm_group_read_depths")
        assert _rows(out) == _rows(exp)
        assert lib.okm_group_read_depths(g, data.ctypes.data, None, 4, 0, 2, out.ctypes.data) == _lib.OKM_E_ARG
        assert lib.okm_group_read_depths(g, data.ctypes.data, offs.ctypes.data, 4, 0, 2, None) == _lib.OKM_E_ARG
        assert lib.okm_group_read_depths(g, None, None, 0, 0, 2, None) == _lib.OKM_OK
        assert _rows(out) == _rows(exp)
    finally:
        lib.okm_group_destroy(g)
    _lib.check(lib.okm_group_create(ctypes.byref(g), k, _lib.OKM_MODE_SET, 1, None, 0), "okm_group_create")
    try:
        assert lib.okm_group_read_depths(g, data.ctypes.data, offs.ctypes.data, len(q), 0, 2, out.ctypes.data) == _lib.OKM_E_STATE
    finally:
        lib.okm_group_destroy(g)


@pytest.mark.parametrize("P", [2, 3])
def test_owners_of_a_loopback_merge_combine_to_the_whole(P):
    """What okm_group_read_depths does over N GPUs, on one: the owners of a
    P-rank merge hold disjoint key ranges; their rows over the same reads,
    combined by the documented rule, are the rows against the whole table."""
    k, recs, table, q, exp = _group_reads()
    testing.set_knob("loopback_timeout_ms", 60_000)
    shards = [np.ascontiguousarray(p).reshape(-1) for p in np.array_split(recs, P)]
    comms = okm.Comm.init_loopback(P, 0)
    out, err = [None] * P, [None] * P

    def rank(r):
        local, owner = okm.KmerCounter(k), okm.KmerCounter(k)
        buf = okm.DeviceBuffer(len(shards[r]))
        try:
            buf.upload(shards[r])
            local.add_device_batch(buf.address, len(shards[r]))
            comms[r].merge_owned(local, owner)
            out[r] = _host(owner, q, wrapper=False)
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
    assert _rows(dc.combine(out)) == _rows(exp)
    assert all(o["present"].sum() > 0 for o in out)  # every owner holds some of the reads' k-mers
    assert all(np.array_equal(o["windows"], exp["windows"]) for o in out)


# ---------------------------------------------------------------------------
# errors and other states
# ---------------------------------------------------------------------------

def test_before_any_batch_windows_only():
    recs = (dc.genome()[:100], b"", b"ACGTN" * 20, dc.genome()[:30])
    for k in (31, 40):
        with okm.KmerCounter(k, wide=k > 32) as c:
            exp = dc.expected(recs, k, {})
            assert int(exp[0]["windows"]) == 100 - k + 1 and not exp["present"].any()
            _check(c, recs, exp)


def test_null_arguments_and_no_records():
    k = 31
    lib = _lib.load()
    recs = dc.geometry(k)[0][70:80]
    table = dc.table_of_records(dc.table_reads(), k)
    data, offs = okm.pack_records(list(recs))
    out = np.full(len(recs) * 6, JUNK, np.uint64).view(okm.READ_DEPTH_DTYPE)
    with okm.KmerCounter(k) as c:
        _count_reads(c, dc.table_reads())
        n = len(recs)
        assert lib.okm_read_depths(c.ctx, data.ctypes.data, None, n, 0, 2, out.ctypes.data) == _lib.OKM_E_ARG
        assert lib.okm_read_depths(c.ctx, data.ctypes.data, offs.ctypes.data, n, 0, 2, None) == _lib.OKM_E_ARG
        assert lib.okm_read_depths(c.ctx, None, offs.ctypes.data, n, 0, 2, out.ctypes.data) == _lib.OKM_E_ARG
        assert lib.okm_read_depths_device(c.ctx, None, 100, n, 2, 4096) == _lib.OKM_E_ARG
        assert lib.okm_read_depths_device(c.ctx, 4096, 100, n, 2, None) == _lib.OKM_E_ARG
        assert lib.okm_read_depths_device(None, 4096, 100, n, 2, 4096) == _lib.OKM_E_ARG
        # no records: nothing is touched, whatever the pointers
        assert lib.okm_read_depths(c.ctx, None, None, 0, 0, 2, None) == _lib.OKM_OK
        assert lib.okm_read_depths(c.ctx, data.ctypes.data, offs.ctypes.data, 0, 0, 2, out.ctypes.data) == _lib.OKM_OK
        assert lib.okm_read_depths_device(c.ctx, None, 0, 0, 2, None) == _lib.OKM_OK
        assert (out.view(np.uint64) == JUNK).all()
        assert len(c.read_depths([])) == 0
        # records that are all empty need no bytes
        zero = np.zeros(4, np.uint64)
        assert lib.okm_read_depths(c.ctx, None, zero.ctypes.data, 3, 0, 2, out.ctypes.data) == _lib.OKM_OK
        assert _rows(out[:3]) == [(0,) * 6] * 3
        assert _rows(_device(c, b"", 3)) == [(0,) * 6] * 3
        _check(c, recs, dc.expected(recs, k, table))  # the table is as it was


def test_set_mode_has_no_counts():
    with okm.KmerCounter(31, "set") as c:
        c.add_pairs(np.arange(1, 100, dtype=np.uint64))
        with pytest.raises(okm.OkmError) as ei:
            c.read_depths([b"ACGT" * 20])
        assert ei.value.status == _lib.OKM_E_STATE
        with pytest.raises(okm.OkmError) as ei:
            c.read_depths_device(4096, 64, 1, 4096)
        assert ei.value.status == _lib.OKM_E_STATE
        keys, _ = c.result(1)
        assert np.array_equal(keys, np.arange(1, 100, dtype=np.uint64))


@pytest.mark.parametrize("state", ["pending", "dense", "host"])
def test_every_allocation_fails_in_turn(state):
    k, batch, table, recs, exp = _small()
    reads = [bytes(r[:-1]) for r in batch.reshape(1200, 101)]

    def prepare(c):
        c.reset()
        c.add_records(reads, normalized=True)
        c.count()
        if state == "dense":
            assert _table(c) == table
        elif state == "host":
            _to_host_table(c, table)
            testing.set_knob("hist_slice", 5000)

    def attempt(c, fail):
        testing.set_knob("fail_alloc", fail)
        try:
            return _host(c, recs, wrapper=False), None
        except okm.OkmError as e:
            return None, e
        finally:
            left[0] = testing.get_knob("fail_alloc")
            testing.set_knob("fail_alloc", -1)

    left = [0]
    try:
        with okm.KmerCounter(k) as c:
            prepare(c)
            got, err = attempt(c, BIG)
            assert err is None and _rows(got) == _rows(exp)
            n_gets = BIG - left[0]
            print(f"{state}: {n_gets} allocations")
            # the tile words, the chunk's bytes and rows; the pending index's four arrays / the slice's two
            assert n_gets == {"pending": 7, "dense": 3, "host": 5}[state]
            for n in range(1, n_gets + 1):
                prepare(c)
                in_use = testing.device_in_use(c)
                got, err = attempt(c, n)
                assert left[0] == -1, f"allocation {n}: the failure did not fire"
                if err is None:
                    assert _rows(got) == _rows(exp)
                else:
                    assert err.status == _lib.OKM_E_NOMEM, (n, err)
                assert testing.device_in_use(c) == in_use, f"allocation {n}: a block was stranded"
                if state == "host":
                    assert c.engine_info()["host_bytes"] > 0
                assert _rows(_host(c, recs, wrapper=False)) == _rows(exp)  # the table is intact: again, cleanly
                assert _table(c) == table
                c.reset()
                assert testing.device_in_use(c) == 0 and c.engine_info()["host_bytes"] == 0
    finally:
        testing.set_knob("hist_slice", -1)


# ---------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------

def _cli(*args):
    return subprocess.run([_lib.CLI_PATH, *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("k,fmt", [(31, "fastq"), (63, "fasta.gz"), (31, "fasta.gz"), (63, "fastq")])
def test_cli_depth(tmp_path, k, fmt):
    ids, recs, inp = dc.cli_records(k)
    table = dc.table_of_records(inp, k)
    fa = tmp_path / "in.fa"
    fa.write_text(dc.fasta_text([f"t{i}" for i in range(len(inp))], inp))
    if fmt == "fastq":
        reads = tmp_path / "reads.fq"
        reads.write_text(dc.fastq_text(ids, recs))
    else:
        reads = tmp_path / "reads.fa.gz"
        reads.write_bytes(gzip.compress(dc.fasta_text(ids, recs, width=50).encode()))  # multi-line records
    wide = ["--wide"] if k > 32 else []
    plain, out, dep = tmp_path / "plain.tsv", tmp_path / "out.tsv", tmp_path / ("d.tsv.gz" if fmt != "fastq" else "d.tsv")
    assert _cli("count", "-k", str(k), "-i", str(fa), "-o", str(plain), *wide).returncode == 0
    r = _cli("count", "-k", str(k), "-i", str(fa), "-o", str(out), "--depth", str(reads), "--depth-output", str(dep), *wide)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == plain.read_bytes() and len(plain.read_bytes()) > 0
    got = gzip.decompress(dep.read_bytes()).decode() if fmt != "fastq" else dep.read_text()
    exp = dc.expected(recs, k, table, min_count=2, normalized=True)
    assert got == dc.render(ids, exp)
    assert got.splitlines()[3] == ids[3] + "\t0\t0\t0\t0\t0\t0"  # the record shorter than k
    # --depth-min-count
    r = _cli("count", "-k", str(k), "-i", str(fa), "-o", str(out), "--depth", str(reads), "--depth-output", str(dep),
             "--depth-min-count", "3", *wide)
    assert r.returncode == 0, r.stderr
    got3 = gzip.decompress(dep.read_bytes()).decode() if fmt != "fastq" else dep.read_text()
    assert got3 == dc.render(ids, dc.expected(recs, k, table, min_count=3, normalized=True)) != got


def test_cli_depth_with_lookup_and_histogram(tmp_path):
    import hist_cases as hc
    import lookup_cases as lc
    k = 31
    ids, recs, inp = dc.cli_records(k)
    table = dc.table_of_records(inp, k)
    fa, reads, look = tmp_path / "in.fa", tmp_path / "reads.fq", tmp_path / "look.txt"
    fa.write_text(dc.fasta_text([f"t{i}" for i in range(len(inp))], inp))
    reads.write_text(dc.fastq_text(ids, recs))
    kmers = [inp[0][:k].decode(), inp[1][5:5 + k].decode().lower(), "A" * k]
    look.write_text("\n".join(kmers) + "\n")
    out, dep, lo, hi = (tmp_path / n for n in ("out.tsv", "d.tsv", "l.tsv", "h.tsv"))
    r = _cli("count", "-k", str(k), "-i", str(fa), "-o", str(out), "--depth", str(reads), "--depth-output", str(dep),
             "--lookup", str(look), "--lookup-output", str(lo), "--histogram", str(hi), "-v")
    assert r.returncode == 0, r.stderr
    assert dep.read_text() == dc.render(ids, dc.expected(recs, k, table, normalized=True))
    text = {okm.u64_to_seq(v, k).decode(): n for v, n in table.items()}
    assert lo.read_text() == lc.render_lookup(kmers, text)
    assert hi.read_text() == hc.render_tsv(hc.expected_hist(list(table.values()), 10001))
    assert len(out.read_text().splitlines()) == len(table)
