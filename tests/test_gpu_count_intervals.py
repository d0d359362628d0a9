"""okm_read_count_intervals on the device, exact against plain Python (per slot: is the window all A/C/G/T and
lo <= dict.get(key, 0) <= hi; then a loop over the bits), host and device form, into buffers full of junk."""

import gzip
import subprocess
from ctypes import byref, c_uint64, c_void_p

import numpy as np
import pytest

import depth_cases as dc
import okm
from okm import _lib, testing
from test_gpu_solid_runs import EDGES, GENOME, LONG, _key, _small, _table

pytestmark = pytest.mark.gpu

JUNK, M64, UNITS = 0x77, dc.M64, ("bases", "slots")


def expected(records, k, table, lo, hi):  # {unit: [(record, start, end)]}
    out = {u: [] for u in UNITS}
    for r, rec in enumerate(records):
        s = dc.normalize(rec).upper().replace(b"U", b"T")
        bits = [all(ch in b"ACGT" for ch in s[j:j + k]) and lo <= table.get(_key(s[j:j + k], k), 0) <= hi
                for j in range(max(len(s) - k + 1, 0))] + [False]
        runs = [j for j in range(len(bits)) if bits[j] != (j > 0 and bits[j - 1])]  # start, end, start, end ...
        out["slots"] += [(r, a, b) for a, b in zip(runs[::2], runs[1::2])]
        bases = []
        for a, b in zip(runs[::2], runs[1::2]):
            if bases and a <= bases[-1][2]:  # overlaps or abuts the stretch before
                bases[-1] = (r, bases[-1][1], b + k - 1)
            else:
                bases.append((r, a, b + k - 1))
        out["bases"] += bases
    return out


def _rows(rows):
    return [tuple(int(x) for x in r) for r in rows]


def _device(c, batch, nrec, lo, hi, unit, behind=b"", shift=0, cap=None):  # (rows written, the total, the status)
    lib, n, u = _lib.load(), c_uint64(JUNK), okm.INTERVAL_UNITS[unit]
    raw = np.frombuffer(b"G" * shift + batch + behind, dtype=np.uint8)
    bufs = [okm.DeviceBuffer(max(len(raw), 16))]
    try:
        if len(raw):
            bufs[0].upload(raw)
        args = (c.ctx, bufs[0].address + shift, len(batch), nrec, lo, hi, u)
        assert lib.okm_read_count_intervals_device(*args, None, 0, byref(n)) == _lib.OKM_OK
        total = n.value
        cap = total if cap is None else cap
        out = np.full((cap + 2, 3), JUNK, np.uint64)
        bufs.append(okm.DeviceBuffer(out.nbytes))
        bufs[1].upload(out)
        status = lib.okm_read_count_intervals_device(*args, bufs[1].address, cap, byref(n))
        bufs[1].download(out)
        assert n.value == total and (out[min(total, cap):] == JUNK).all()  # nothing behind the rows is touched
        return _rows(out[:min(total, cap)]), total, status
    finally:
        for b in bufs:
            b.free()


def _check(c, recs, k, table, lo, hi, units=UNITS):
    exp = expected(recs, k, table, lo, hi)
    for unit in units:
        assert _rows(c.count_intervals(recs, lo, hi, unit)) == exp[unit]
        assert _device(c, dc.device_batch(recs), len(recs), lo, hi, unit) == (exp[unit], len(exp[unit]), _lib.OKM_OK)
        cut = dc.device_batch(recs, terminate_last=False)  # ... and unterminated, valid bases behind n_bytes
        assert _device(c, cut, len(recs), lo, hi, unit, behind=b"ACGT" * 40)[0] == exp[unit]
    return exp


@pytest.mark.parametrize("k", dc.KS)
def test_record_geometry(k):
    recs, table = dc.geometry(k)[0], dc.geometry_expected(k)[0]
    with okm.KmerCounter(k, wide=k > 32) as c:
        c.set_timing(True)
        c.add_records(list(dc.table_reads()))
        c.count()
        for state in ("pending", "dense"):
            before = c.kernel_stats().get("compact_items")
            exp = _check(c, recs, k, table, 2, M64)
            batch = dc.device_batch(recs)
            for unit in UNITS:
                assert _device(c, batch, len(recs), 2, M64, unit, shift=1)[0] == exp[unit]  # not 16-byte aligned
                assert _device(c, batch, 80, 2, M64, unit)[0] == [r for r in exp[unit] if r[0] < 80]  # fewer records
                assert _device(c, batch, len(recs) + 3, 2, M64, unit)[0] == exp[unit]  # ... and more
            assert c.kernel_stats().get("compact_items") == before  # the table was read where it lies
            assert _table(c) == table  # ... and this gathers it


# test_gpu_solid_runs' edges: runs that start and end at bit 63 / 0 / 1 of a word and at the ends of a wave and a tile
@pytest.mark.parametrize("name", [n for n in EDGES if n != "two equal runs"])
@pytest.mark.parametrize("k", [31, 33])
def test_stage2_edges(k, name):
    g, e, first = GENOME, EDGES[name], bytearray(GENOME[:LONG])
    for x in (e if name.startswith("N in") else [p + k for p in e[0]] + [p - 1 for p in e[1]]):
        first[x] = ord("N")
    recs = (bytes(first), g[100:140], b"", g[7:7 + k], g[300:300 + k - 1], g[50_000:50_200], g[51_000:51_100] + b"N")
    with okm.KmerCounter(k, wide=k > 32) as c:
        c.add_records([g, g])  # every window of the genome counts 2
        exp = _check(c, recs, k, {_key(g[j:j + k], k): 2 for j in range(len(g) - k + 1)}, 2, M64)
        assert name != "no N" or exp["bases"][0] == (0, 0, LONG) and exp["slots"][0] == (0, 0, LONG - k + 1)


# The table is the record's windows less the slots of four gaps, k - 1 and k slots wide, astride a word border and a
# tile border: in bases the narrower ones close, in slots all stay.  (At k <= 2 the keys repeat: many more gaps.)
@pytest.mark.parametrize("k", [1, 2, 31, 33, 64])
def test_dilation(k):
    rec = GENOME[:2 * 16384 + 700]
    gaps = [(b - (w + 1) // 2, w) for b, w in ((64 * 9, k - 1), (64 * 20, k), (16384, k - 1), (2 * 16384, k))]
    gone = {_key(rec[j:j + k], k) for a, w in gaps for j in range(a, a + w)}
    keys = sorted({_key(rec[j:j + k], k) for j in range(len(rec) - k + 1)} - gone)
    with okm.KmerCounter(k, wide=k > 32) as c:
        c.add_pairs(dc.pairs_input(keys, k > 32), np.full(len(keys), 2, np.uint64))
        exp = _check(c, (rec, rec[5:400]), k, dict.fromkeys(keys, 2), 2, M64)
        assert k < 31 or [sum(r[0] == 0 for r in exp[u]) for u in UNITS] == [3, 5]  # the first record's rows
        assert k != 1 or exp["slots"] == exp["bases"]


@pytest.mark.parametrize("k", [31, 37])
def test_ranges(k):
    (keys, counts, recs, table), big = dc.big_count_pairs(k), (1 << 32) + 8
    with okm.KmerCounter(k, wide=k > 32) as c:
        every = _check(c, recs, k, {}, 0, M64)  # before any batch: absent selects every valid window
        assert every["bases"] == [(0, 0, 3 * k + 20), (1, 0, 2 * k + 9), (1, 2 * k + 10, 3 * k + 14), (2, 0, k + 1)]
        c.add_pairs(dc.pairs_input(keys, k > 32), np.array(counts, dtype=np.uint64))
        c.count()
        for state in ("pending", "dense"):
            assert _check(c, recs, k, table, 0, M64) == every  # ... and so does any table
            assert _check(c, recs + (dc.genome()[:300] + b"N" * 3,), k, table, 0, 0)["slots"][-1][0] == 3  # absent only
            band = _check(c, recs, k, table, big, big + 60)  # hi below some counts, lo above some
            assert 0 < len(band["slots"]) and band != every
            solid = _check(c, recs, k, table, big, M64, units=("slots",))["slots"]
            runs = c.solid_runs(recs, big)
            for r in range(len(recs)):
                mine = [(e - s, -s) for rr, s, e in solid if rr == r]
                assert sum(ln for ln, _ in mine) == runs[r]["solid"]
                assert max(mine, default=(0, 0)) == (runs[r]["run_len"], -int(runs[r]["run_start"]))
            assert _table(c) == table


def test_host_resident_table_in_slices():
    k, reads, table, recs, _ = _small()
    recs += (reads[3][:50] + dc.genome()[:70] + reads[5][20:],)  # absent windows between present ones
    with okm.KmerCounter(k) as c:
        c.add_records(reads, normalized=True)
        c.count()
        testing.set_knob("fail_alloc", 1)  # the dense gather's first allocation fails: the table stays on the host
        assert _table(c) == table and testing.get_knob("fail_alloc") == -1
        for sl in (1000, 4096, len(table)):  # a ragged last slice, several slices, exactly one
            with testing.knobs(hist_slice=sl):
                assert c.engine_info()["host_bytes"] > 0
                absent = _check(c, recs, k, table, 0, 0)  # the default must survive every slice that misses
                assert len(absent["bases"]) >= 2 and len(_check(c, recs, k, table, 2, M64)["bases"]) > 3
        with testing.knobs(hist_slice=4096, depth_chunk=700):  # slices and chunks cross: `record` stays global
            for lo, hi in ((0, 0), (2, M64)):
                exp = expected(recs, k, table, lo, hi)
                for unit in UNITS:
                    assert _rows(c.count_intervals(recs, lo, hi, unit)) == exp[unit]
        assert c.engine_info()["host_bytes"] > 0 and _table(c) == table


def test_capacity():
    k, reads, table, recs, _ = _small()
    batch, exp = dc.device_batch(recs), expected(recs, k, table, 2, M64)["bases"]
    assert (n := len(exp)) > 4
    with okm.KmerCounter(k) as c:
        c.add_records(reads, normalized=True)
        assert _device(c, batch, len(recs), 2, M64, "bases", cap=n) == (exp, n, _lib.OKM_OK)
        assert _device(c, batch, len(recs), 2, M64, "bases", cap=n - 1) == (exp[:n - 1], n, _lib.OKM_E_OVERFLOW)
        assert _device(c, batch, len(recs), 2, M64, "bases", cap=0) == ([], n, _lib.OKM_E_OVERFLOW)  # a pointer, no room
        assert c.count_intervals_device(0, 0, 5, 0, 0, 2, M64) == 0  # records, all of them empty


def test_errors_and_states():
    k, lib = 31, _lib.load()
    recs = dc.geometry(k)[0][70:80]
    data, offs = okm.pack_records(list(recs))
    out, n = c_void_p(JUNK), c_uint64(JUNK)
    nr, d, o, po, pn = len(recs), data.ctypes.data, offs.ctypes.data, byref(out), byref(n)
    with okm.KmerCounter(k, "set") as c:
        assert lib.okm_read_count_intervals(c.ctx, d, o, nr, 0, 2, 9, 0, po, pn) == _lib.OKM_E_STATE
        assert lib.okm_read_count_intervals_device(c.ctx, 4096, 64, 1, 2, 9, 0, 4096, 1, pn) == _lib.OKM_E_STATE
    with okm.KmerCounter(k) as c:
        host, dev = [c.ctx, d, o, nr, 0, 2, 9, 0, po, pn], [c.ctx, 4096, 100, nr, 2, 9, 0, 4096, 1, pn]
        for i, bad in ((0, None), (1, None), (2, None), (8, None), (9, None), (5, 10), (7, 2)):  # null; lo > hi; unit
            assert lib.okm_read_count_intervals(*host[:i], bad, *host[i + 1:]) == _lib.OKM_E_ARG
        for i, bad in ((1, None), (7, None), (9, None), (4, 10), (6, 7), (2, 1 << 32)):  # the last: batch too large
            assert lib.okm_read_count_intervals_device(*dev[:i], bad, *dev[i + 1:]) == _lib.OKM_E_ARG
        out.value = n.value = JUNK
        assert lib.okm_read_count_intervals(c.ctx, None, None, 0, 0, 2, 9, 0, po, pn) == _lib.OKM_OK  # no records
        assert (out.value, n.value) == (None, 0)
        assert lib.okm_read_count_intervals_device(c.ctx, None, 0, 0, 2, 9, 0, None, 0, pn) == _lib.OKM_OK
        assert len(_check(c, recs, k, {}, 0, 0)["bases"]) >= 7  # before any batch: every valid window is absent
        assert _check(c, recs, k, {}, 1, M64) == {u: [] for u in UNITS}


@pytest.mark.parametrize("state", ["pending", "dense"])
def test_every_allocation_fails_in_turn(state):
    k, reads, table, recs, _ = _small()
    exp = expected(recs, k, table, 2, M64)["bases"]
    with okm.KmerCounter(k) as c:
        c.add_records(reads, normalized=True)
        c.count()
        assert state == "pending" or _table(c) == table
        for fail in range(1, 20):
            in_use = testing.device_in_use(c)
            testing.set_knob("fail_alloc", fail)
            try:
                got, err = _rows(c.count_intervals(recs, 2, M64)), None
            except okm.OkmError as e:
                got, err = None, e
            fired, _ = testing.get_knob("fail_alloc") == -1, testing.set_knob("fail_alloc", -1)
            assert testing.device_in_use(c) == in_use, f"allocation {fail}: a block was stranded"
            assert got == exp if err is None else (err.status == _lib.OKM_E_NOMEM and fired)
            if not fired:
                break  # the call makes fewer allocations than that: it ran untouched
        assert not fired and fail > 4 and _table(c) == table


@pytest.mark.parametrize("k,fmt", [(31, "fastq"), (63, "fasta.gz")])
def test_cli(tmp_path, k, fmt):
    ids, recs, inp = dc.cli_records(k)
    fa, gz, table = tmp_path / "in.fa", fmt != "fastq", dc.table_of_records(inp, k)
    fa.write_text(dc.fasta_text([f"t{i}" for i in range(len(inp))], inp))
    reads, bed = tmp_path / ("reads." + ("fa.gz" if gz else "fq")), tmp_path / ("i.bed.gz" if gz else "i.bed")
    text = dc.fasta_text(ids, recs, width=50) if gz else dc.fastq_text(ids, recs)
    reads.write_bytes(gzip.compress(text.encode()) if gz else text.encode())
    args = [_lib.CLI_PATH, "count", "-k", str(k), "-i", str(fa), "-o", str(tmp_path / "out.tsv"), "--intervals",
            str(reads), "--intervals-output", str(bed)] + (["--wide"] if k > 32 else [])
    for extra, lo, hi, unit in (([], 2, M64, "bases"), (["--intervals-slots", "--intervals-max-count", "3"], 2, 3, "slots"),
                                (["--intervals-min-count", "0", "--intervals-max-count", "0"], 0, 0, "bases")):
        r = subprocess.run(args + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        got = gzip.decompress(bed.read_bytes()).decode() if gz else bed.read_text()
        exp = expected(recs, k, table, lo, hi)[unit]
        assert exp and got == "".join(f"{ids[r]}\t{s}\t{e}\n" for r, s, e in exp)
