"""okm_read_count_quantiles on the device, exact against plain Python (`expected`), host and device form,
into buffers full of junk."""

import gzip
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import depth_cases as dc
import okm
from okm import _lib, testing

pytestmark = pytest.mark.gpu

JUNK = 0x77
CMAX = (1 << 32) - 2                   # OKM_QUANTILE_COUNT_MAX
Q4 = ((0, 1), (1, 4), (1, 2), (1, 1))  # shallowest, first quartile, khmer's median, deepest
# okm_quantile.hip: a lane's registers hold slots l, l + 64, ...; kQuantWave; kQuantLds (a longer record streams)
LANES, WAVE, LDS = 64, 512, 8192
LONG = 3 * LDS + 901
SLOTS = (1, 2, LANES - 1, LANES, LANES + 1, WAVE - 1, WAVE, WAVE + 1, LDS, LDS + 1, LONG)
GENOME = dc._bases(np.random.default_rng(79), LONG + 100)


def expected(records, k, table, quantiles=Q4):
    out = np.zeros((len(records), 1 + len(quantiles)), np.uint64)
    for r, rec in enumerate(records):
        cs = sorted(min(table.get(v, 0), CMAX) for v in dc.window_keys(dc.normalize(rec), k))
        out[r] = [len(cs)] + [cs[min(len(cs) * a // b, len(cs) - 1)] if cs else 0 for a, b in quantiles]
    return out


def _host(c, recs, quantiles=Q4):
    data, offs = okm.pack_records(list(recs))
    q = np.array(quantiles, np.uint32)
    out = np.full((len(recs), 1 + len(q)), JUNK, np.uint64)
    _lib.check(_lib.load().okm_read_count_quantiles(c.ctx, data.ctypes.data, offs.ctypes.data, len(recs), 0,
                                                    q.ctypes.data, len(q), out.ctypes.data), "okm_read_count_quantiles")
    return out


def _device(c, batch, nrec, quantiles=Q4, behind=b"", shift=0):
    raw = np.frombuffer(b"G" * shift + batch + behind, dtype=np.uint8)
    w = 1 + len(quantiles)
    dseq, dout = okm.DeviceBuffer(max(len(raw), 16)), okm.DeviceBuffer(max(nrec, 1) * w * 8)
    try:
        if len(raw):
            dseq.upload(raw)
        dout.upload(np.full(max(nrec, 1) * w, JUNK, np.uint64))
        c.count_quantiles_device(dseq.address + shift, len(batch), nrec, dout.address, quantiles)
        out = np.empty((nrec, w), np.uint64)
        if nrec:
            dout.download(out)
        return out
    finally:
        dseq.free()
        dout.free()


def _check(c, recs, exp, quantiles=Q4):
    got = _host(c, recs, quantiles)
    assert got.tolist() == exp.tolist()
    assert np.array_equal(got, c.count_quantiles(recs, quantiles))
    assert _device(c, dc.device_batch(recs), len(recs), quantiles).tolist() == exp.tolist()
    cut = dc.device_batch(recs, terminate_last=False)  # ... and unterminated, valid bases behind n_bytes
    assert _device(c, cut, len(recs), quantiles, behind=b"ACGT" * 40).tolist() == exp.tolist()
    return got


def _table(c):
    return dc.table_of_result(*c.result(1), c.wide)


@pytest.mark.parametrize("k", dc.KS)
def test_record_geometry(k):
    recs, table = dc.geometry(k)[0], dc.geometry_expected(k)[0]
    exp = expected(recs, k, table)
    assert (exp[:, 1] < exp[:, 4]).any()  # some record's shallowest and deepest window differ
    with okm.KmerCounter(k, wide=k > 32) as c:
        c.set_timing(True)
        c.add_records(list(dc.table_reads()))
        c.count()
        for state in ("pending", "dense"):
            before = c.kernel_stats().get("compact_items")
            got, depth = _check(c, recs, exp), c.read_depths(recs)
            assert np.array_equal(got[:, 0], depth["windows"])
            assert np.array_equal(got[:, 1], np.where(depth["present"] < depth["windows"], 0, depth["min"]))
            batch = dc.device_batch(recs)
            assert _device(c, batch, len(recs), shift=1).tolist() == exp.tolist()  # not 16-byte aligned: through scratch
            assert _device(c, batch, 80).tolist() == exp[:80].tolist()  # fewer rows than records, and more
            more = _device(c, batch, len(recs) + 3)
            assert more[:len(recs)].tolist() == exp.tolist() and not more[len(recs):].any()
            assert c.kernel_stats().get("compact_items") == before  # the table was read where it lies
            assert _table(c) == table  # ... and this gathers it


@lru_cache(maxsize=None)
def _edge_records(k):
    """One record per slot count, short ones behind each; per selection class an N in the first, a middle, the last
    window."""
    g, recs = GENOME, []
    for s in SLOTS:
        o = 0 if s == LONG else 7 * s % 90
        recs += [g[o:o + s + k - 1], g[100:140], b"", g[7:7 + k], g[300:300 + k - 1]]
    for s in (LANES + 1, WAVE + 1, LDS + 1):
        for at in (0, s // 2, s + k - 2):
            r = bytearray(g[3:3 + s + k - 1])
            r[at] = ord("N")
            recs.append(bytes(r))
    keys = sorted(set(dc.window_keys(g, k)))
    at = {v: j for j, v in enumerate(dc.window_keys(g, k))}  # a key's (last) genome position
    return tuple(recs), keys, [at[v] for v in keys]


DIGITS = (0, 1, 255, 256, 65535, 65536, 1 << 24, CMAX, CMAX + 1, (1 << 32) + 5)  # 0: the key is absent
# the long record is the genome's head: on the ramp the value at rank i is i + 1 (low-byte bin 255, bin 0, bin 1)
RAMP_Q = ((254, LONG), (255, LONG), (256, LONG), (1, 2))
# the digits are drawn evenly, three of the ten clip to CMAX: a long record's 5 %, 15 % ... are the eight values
DIGIT_QS = (((1, 20), (3, 20), (5, 20), (7, 20)), ((9, 20), (11, 20), (13, 20), (19, 20)))


@pytest.mark.parametrize("pattern", ["equal", "digits", "ramp"])
@pytest.mark.parametrize("k", [31, 33])
def test_selection_edges(k, pattern):
    recs, keys, pos = _edge_records(k)
    if pattern == "equal":
        counts = [7] * len(keys)
    elif pattern == "digits":
        counts = [DIGITS[i] for i in np.random.default_rng(k).integers(0, len(DIGITS), len(keys))]
    else:
        counts = [p + 1 for p in pos]
    table = {v: c for v, c in zip(keys, counts) if c}
    calls = {"equal": (Q4,), "digits": DIGIT_QS, "ramp": (RAMP_Q,)}[pattern]
    exps, long_row = [expected(recs, k, table, q) for q in calls], 5 * (len(SLOTS) - 1)
    assert exps[0][:5 * len(SLOTS):5, 0].tolist() == list(SLOTS)
    if pattern == "ramp":
        assert exps[0][long_row].tolist() == [LONG, 255, 256, 257, LONG // 2 + 1]
    if pattern == "digits":
        assert [v for e in exps for v in e[long_row, 1:].tolist()] == sorted(set(min(d, CMAX) for d in DIGITS))
    with okm.KmerCounter(k, wide=k > 32) as c:
        ks = sorted(table)
        c.add_pairs(dc.pairs_input(ks, k > 32), np.array([table[v] for v in ks], dtype=np.uint64))
        for q, exp in zip(calls, exps):
            _check(c, recs, exp, q)


def test_host_resident_table_in_slices_and_chunks():
    k, recs = 31, dc.chunk_records()
    table = dc.table_of_records(recs + dc.table_reads(), k)
    exp, rank, n = expected(recs, k, table), {v: i for i, v in enumerate(sorted(table))}, len(table)
    ws = dc.window_keys(recs[0], k)  # consecutive windows of one record lie in different slices
    assert n > 3000 and len({rank[v] // 1000 for v in ws[:8]}) > 2 and len(set(exp[:, 3].tolist())) > 2
    with okm.KmerCounter(k) as c:
        c.add_records(list(recs + dc.table_reads()))
        c.count()
        testing.set_knob("fail_alloc", 1)  # the dense gather's first allocation fails: the table stays on the host
        assert _table(c) == table and testing.get_knob("fail_alloc") == -1
        for sl in (1000, n):  # several slices with a ragged last one, exactly one
            with testing.knobs(hist_slice=sl):
                assert c.engine_info()["host_bytes"] > 0
                _check(c, recs, exp)
        with testing.knobs(hist_slice=1000, depth_chunk=dc.CHUNK_BYTES):  # slices and chunks cross
            assert len(dc.chunks_of(recs, dc.CHUNK_BYTES)) > 3
            assert _host(c, recs).tolist() == exp.tolist()
        assert c.engine_info()["host_bytes"] > 0 and _table(c) == table


def test_empty_and_wide_folded_table():
    k = 37
    a, b = dc.table_reads()[:30], dc.table_reads()[20:]
    recs = dc.geometry(k)[0][70:]
    with okm.KmerCounter(k, wide=True) as c:
        empty = _check(c, recs, expected(recs, k, {}))  # before any batch: windows only
        assert empty[:, 0].any() and not empty[:, 1:].any()
        c.add_records(list(a))
        first = _check(c, recs, expected(recs, k, dc.table_of_records(a, k)))
        c.add_records(list(b))  # the first table becomes a weighted run of the second count, made by this call
        second = _check(c, recs, expected(recs, k, dc.table_of_records(a + b, k)))
        assert not np.array_equal(first, second)


def test_errors_and_states():
    k, lib = 31, _lib.load()
    recs = dc.geometry(k)[0][70:80]
    data, offs = okm.pack_records(list(recs))
    out = np.full((len(recs), 5), JUNK, np.uint64)
    n, d, o, p = len(recs), data.ctypes.data, offs.ctypes.data, out.ctypes.data
    good, five = np.array(Q4, np.uint32), np.array(Q4 + ((1, 3),), np.uint32)
    den0, above = np.array(((1, 2), (1, 0)), np.uint32), np.array(((3, 2),), np.uint32)
    q = good.ctypes.data
    with okm.KmerCounter(k, "set") as c:
        assert lib.okm_read_count_quantiles(c.ctx, d, o, n, 0, q, 4, p) == _lib.OKM_E_STATE
        assert lib.okm_read_count_quantiles_device(c.ctx, 4096, 64, 1, q, 4, 4096) == _lib.OKM_E_STATE
    with okm.KmerCounter(k) as c:
        c.add_records(list(dc.table_reads()))
        # no quantile, too many, den == 0, num > den, null q
        for qq, nq in ((q, 0), (five.ctypes.data, 5), (den0.ctypes.data, 2), (above.ctypes.data, 1), (None, 1)):
            assert lib.okm_read_count_quantiles(c.ctx, d, o, n, 0, qq, nq, p) == _lib.OKM_E_ARG
            assert lib.okm_read_count_quantiles_device(c.ctx, 4096, 100, n, qq, nq, 4096) == _lib.OKM_E_ARG
        for args in ((c.ctx, d, None, n, 0, q, 4, p), (c.ctx, d, o, n, 0, q, 4, None), (c.ctx, None, o, n, 0, q, 4, p),
                     (None, d, o, n, 0, q, 4, p)):
            assert lib.okm_read_count_quantiles(*args) == _lib.OKM_E_ARG
        for args in ((c.ctx, None, 100, n, q, 4, 4096), (c.ctx, 4096, 100, n, q, 4, None),
                     (c.ctx, 4096, 1 << 32, n, q, 4, 4096)):  # the last: batch too large
            assert lib.okm_read_count_quantiles_device(*args) == _lib.OKM_E_ARG
        assert lib.okm_read_count_quantiles(c.ctx, None, None, 0, 0, q, 4, None) == _lib.OKM_OK  # no records
        assert lib.okm_read_count_quantiles_device(c.ctx, None, 0, 0, q, 4, None) == _lib.OKM_OK
        assert (out == JUNK).all()  # nothing was touched
        assert not _device(c, b"", 3).any()  # records, all of them empty


@pytest.mark.parametrize("state", ["pending", "dense"])
def test_every_allocation_fails_in_turn(state):
    k = 31
    recs, table = dc.geometry(k)[0][60:], dc.geometry_expected(k)[0]
    exp = expected(recs, k, table)
    with okm.KmerCounter(k) as c:
        c.add_records(list(dc.table_reads()))
        c.count()
        assert state == "pending" or _table(c) == table
        for fail in range(1, 20):
            in_use = testing.device_in_use(c)
            testing.set_knob("fail_alloc", fail)
            try:
                got, err = _host(c, recs), None
            except okm.OkmError as e:
                got, err = None, e
            fired, _ = testing.get_knob("fail_alloc") == -1, testing.set_knob("fail_alloc", -1)
            assert testing.device_in_use(c) == in_use, f"allocation {fail}: a block was stranded"
            assert got.tolist() == exp.tolist() if err is None else (err.status == _lib.OKM_E_NOMEM and fired)
            if not fired:
                break  # the call makes fewer allocations than that: it ran untouched
        assert not fired and fail > 4
        assert _table(c) == table
        c.reset()
        assert testing.device_in_use(c) == 0  # an empty arena after okm_reset


@pytest.mark.parametrize("k,fmt", [(31, "fastq"), (63, "fasta.gz")])
def test_cli(tmp_path, k, fmt):
    ids, recs, inp = dc.cli_records(k)
    table = dc.table_of_records(inp, k)
    fa, gz = tmp_path / "in.fa", fmt != "fastq"
    fa.write_text(dc.fasta_text([f"t{i}" for i in range(len(inp))], inp))
    reads, dep = tmp_path / ("reads." + ("fa.gz" if gz else "fq")), tmp_path / ("q.tsv.gz" if gz else "q.tsv")
    text = dc.fasta_text(ids, recs, width=50) if gz else dc.fastq_text(ids, recs)
    reads.write_bytes(gzip.compress(text.encode()) if gz else text.encode())
    args = [_lib.CLI_PATH, "count", "-k", str(k), "-i", str(fa), "-o", str(tmp_path / "out.tsv"), "--quantiles",
            str(reads), "--quantiles-output", str(dep)] + (["--wide"] if k > 32 else [])
    for extra, quantiles in (([], ((1, 2),)), (["--quantiles-at", "0/1,1/4,1/2,1/1"], Q4)):
        r = subprocess.run(args + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        got = gzip.decompress(dep.read_bytes()).decode() if gz else dep.read_text()
        exp = expected(recs, k, table, quantiles)
        assert got == "".join(i + "\t" + "\t".join(map(str, row)) + "\n" for i, row in zip(ids, exp.tolist()))
    r = subprocess.run(args + ["--gpus", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2
    assert "the argument '--quantiles <FASTX>' cannot be used with '--gpus <GPUS>' other than 1" in r.stderr
