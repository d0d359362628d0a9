"""okm_read_solid_runs on the device, exact against plain Python (per slot: is
the window all A/C/G/T and its canonical key in a dict with count >= min_count;
then a loop over the bits), host and device form, into buffers full of junk."""

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


@lru_cache(maxsize=None)
def _key(w, k):
    return okm.canonical_u64(okm.seq_to_u64(w, k), k) if k <= 32 else okm.canonical_u128(okm.seq_to_u128(w, k), k)


def expected(records, k, table, min_count=2):
    out = np.zeros(len(records), dtype=okm.SOLID_RUN_DTYPE)
    for r, rec in enumerate(records):
        s = dc.normalize(rec).upper().replace(b"U", b"T")
        ws = [s[j:j + k] for j in range(max(len(s) - k + 1, 0))]
        bits = [all(ch in b"ACGT" for ch in w) and table.get(_key(w, k), 0) >= max(min_count, 1) for w in ws]
        n, start, best, j = len(bits), 0, 0, 0
        while j < n:
            e = j
            while e < n and bits[e]:
                e += 1
            if e - j > best:
                start, best = j, e - j
            j = e + 1
        lead = next((i for i, b in enumerate(bits) if not b), n)
        trail = next((i for i, b in enumerate(reversed(bits)) if not b), n)
        out[r] = (n, sum(bits), start, best, lead, trail)
    return out


def _rows(rows):
    return [tuple(int(x) for x in r) for r in rows]


def _host(c, recs, min_count=2):
    data, offs = okm.pack_records(list(recs))
    out = np.full(len(recs) * 6, JUNK, np.uint64).view(okm.SOLID_RUN_DTYPE)
    _lib.check(_lib.load().okm_read_solid_runs(c.ctx, data.ctypes.data, offs.ctypes.data, len(recs), 0, min_count,
                                               out.ctypes.data), "okm_read_solid_runs")
    return out


def _device(c, batch, nrec, min_count=2, behind=b"", shift=0):
    raw = np.frombuffer(b"G" * shift + batch + behind, dtype=np.uint8)
    dseq, dout = okm.DeviceBuffer(max(len(raw), 16)), okm.DeviceBuffer(max(nrec, 1) * 48)
    try:
        if len(raw):
            dseq.upload(raw)
        dout.upload(np.full(max(nrec, 1) * 6, JUNK, np.uint64))
        c.solid_runs_device(dseq.address + shift, len(batch), nrec, dout.address, min_count)
        out = np.empty(nrec, okm.SOLID_RUN_DTYPE)
        if nrec:
            dout.download(out)
        return out
    finally:
        dseq.free()
        dout.free()


def _check(c, recs, exp, min_count=2):
    got = _host(c, recs, min_count)
    assert _rows(got) == _rows(exp)
    assert np.array_equal(got, c.solid_runs(recs, min_count))
    assert _rows(_device(c, dc.device_batch(recs), len(recs), min_count)) == _rows(exp)
    cut = dc.device_batch(recs, terminate_last=False)  # ... and unterminated, valid bases behind n_bytes
    assert _rows(_device(c, cut, len(recs), min_count, behind=b"ACGT" * 40)) == _rows(exp)
    return got


def _table(c):
    return dc.table_of_result(*c.result(1), c.wide)


@pytest.mark.parametrize("k", dc.KS)
def test_record_geometry(k):
    recs, table = dc.geometry(k)[0], dc.geometry_expected(k)[0]
    exp = expected(recs, k, table)
    assert exp["run_len"].max() > 1 and (exp["lead"] > 0).any() and (exp["trail"] > 0).any()
    with okm.KmerCounter(k, wide=k > 32) as c:
        c.set_timing(True)
        c.add_records(list(dc.table_reads()))
        c.count()
        for state in ("pending", "dense"):
            before = c.kernel_stats().get("compact_items")
            got = _check(c, recs, exp)
            assert np.array_equal(got["solid"], c.read_depths(recs)["solid"])
            batch = dc.device_batch(recs)
            assert _rows(_device(c, batch, len(recs), shift=1)) == _rows(exp)  # not 16-byte aligned: through scratch
            assert _rows(_device(c, batch, 80)) == _rows(exp[:80])  # fewer rows than records, and more
            more = _device(c, batch, len(recs) + 3)
            assert _rows(more[:len(recs)]) == _rows(exp) and _rows(more[len(recs):]) == [(0,) * 6] * 3
            assert c.kernel_stats().get("compact_items") == before  # the table was read where it lies
            assert _table(c) == table  # ... and this gathers it


# Stage 2's edges: bit 63 / 0 / 1 of a word, the last and first position of a wave (4096) and of a
# workgroup (16384).  A run ends at p with an N at base p + k and starts at p with one at p - 1; record 0
# starts the batch, so its slots are batch positions.  (ends, starts), or the N positions themselves.
LONG = 3 * 16384 + 901
EDGES = {
    "word": ((639, 768, 897), (1279, 1408, 1537)),
    "wave": ((4095, 8192, 12289), (20479, 24576, 28673)),
    "tile ends": ((16383, 32768, 49153), ()),
    "tile starts": ((), (16383, 32768, 49153)),
    "through two whole tiles": ((49152,), (100,)),
    "no N": ((), ()),
    "two equal runs": 40_001,  # an odd length, the only N in its exact middle: the earlier run wins
    "N in the first and last window": (0, LONG - 1),
}
GENOME = dc._bases(np.random.default_rng(77), 60_000)


@pytest.mark.parametrize("name", list(EDGES))
@pytest.mark.parametrize("k", [31, 33])
def test_stage2_edges(k, name):
    g, e = GENOME, EDGES[name]
    if name == "two equal runs":
        first, ns = bytearray(g[:e]), [e // 2]
    else:
        first, ns = bytearray(g[:LONG]), list(e) if name.startswith("N in") else [p + k for p in e[0]] + [p - 1 for p in e[1]]
    for x in ns:
        first[x] = ord("N")
    # the short records behind it begin inside a word
    recs = (bytes(first), g[100:140], b"", g[7:7 + k], g[300:300 + k - 1], g[50_000:50_200], g[51_000:51_100] + b"N")
    exp = expected(recs, k, {_key(g[j:j + k], k): 2 for j in range(len(g) - k + 1)})
    slots, solid, start, run, lead, trail = _rows(exp)[0]
    assert name != "no N" or lead == trail == run == slots == LONG - k + 1
    assert name != "two equal runs" or (start, lead, trail) == (0, run, run)
    with okm.KmerCounter(k, wide=k > 32) as c:
        c.add_records([g, g])  # every window of the genome counts 2
        _check(c, recs, exp)


@lru_cache(maxsize=None)
def _small():
    k = 31
    batch = okm.synth_reads(1200, 100, genome_len=40_000, genome_seed=8, seed=8)
    reads = [bytes(r[:-1]) for r in batch.reshape(1200, 101)]
    table = dc.table_of_records(reads, k, normalized=True)
    recs = tuple(reads[::40]) + (dc.genome()[:200], b"", reads[7][:30], reads[9][:60] + b"N" + reads[11][10:])
    return k, reads, table, recs, expected(recs, k, table)


def test_host_resident_table_in_slices():
    k, reads, table, recs, exp = _small()
    n = len(table)
    assert n > 3 * 4096 and 0 < exp["solid"].sum() < exp["slots"].sum()
    with okm.KmerCounter(k) as c:
        c.add_records(reads, normalized=True)
        c.count()
        testing.set_knob("fail_alloc", 1)  # the dense gather's first allocation fails: the table stays on the host
        assert _table(c) == table and testing.get_knob("fail_alloc") == -1
        for sl in (1000, 4096, n):  # a ragged last slice, several slices, exactly one
            with testing.knobs(hist_slice=sl):
                assert c.engine_info()["host_bytes"] > 0
                _check(c, recs, exp)
        with testing.knobs(hist_slice=4096, depth_chunk=700):  # slices and chunks cross
            assert _rows(_host(c, recs)) == _rows(exp)
        assert c.engine_info()["host_bytes"] > 0 and _table(c) == table


@pytest.mark.parametrize("k", [31, 37])
def test_min_count_and_u64_counts(k):
    keys, counts, recs, table = dc.big_count_pairs(k)
    big = (1 << 32) + 8
    exp = expected(recs, k, table, big)
    assert 0 < int(exp[0]["solid"]) < int(exp[0]["slots"])  # present windows that are not solid
    with okm.KmerCounter(k, wide=k > 32) as c:
        c.add_pairs(dc.pairs_input(keys, k > 32), np.array(counts, dtype=np.uint64))
        c.count()
        for state in ("pending", "dense"):
            _check(c, recs, exp, big)
            at0 = _check(c, recs, expected(recs, k, table, 0), 0)  # 0 behaves as 1: every present window
            assert np.array_equal(at0["solid"], c.read_depths(recs, 1)["present"])
            assert _table(c) == table


def test_errors_and_states():
    k, lib = 31, _lib.load()
    recs = dc.geometry(k)[0][70:80]
    data, offs = okm.pack_records(list(recs))
    out = np.full(len(recs) * 6, JUNK, np.uint64).view(okm.SOLID_RUN_DTYPE)
    n, d, o, p = len(recs), data.ctypes.data, offs.ctypes.data, out.ctypes.data
    with okm.KmerCounter(k, "set") as c:
        assert lib.okm_read_solid_runs(c.ctx, d, o, n, 0, 2, p) == _lib.OKM_E_STATE
        assert lib.okm_read_solid_runs_device(c.ctx, 4096, 64, 1, 2, 4096) == _lib.OKM_E_STATE
    with okm.KmerCounter(k) as c:
        for args in ((c.ctx, d, None, n, 0, 2, p), (c.ctx, d, o, n, 0, 2, None), (c.ctx, None, o, n, 0, 2, p),
                     (None, d, o, n, 0, 2, p)):
            assert lib.okm_read_solid_runs(*args) == _lib.OKM_E_ARG
        for args in ((c.ctx, None, 100, n, 2, 4096), (c.ctx, 4096, 100, n, 2, None),
                     (c.ctx, 4096, 1 << 32, n, 2, 4096)):  # the last: batch too large
            assert lib.okm_read_solid_runs_device(*args) == _lib.OKM_E_ARG
        assert lib.okm_read_solid_runs(c.ctx, None, None, 0, 0, 2, None) == _lib.OKM_OK  # no records: nothing touched
        assert lib.okm_read_solid_runs_device(c.ctx, None, 0, 0, 2, None) == _lib.OKM_OK
        assert (out.view(np.uint64) == JUNK).all()
        _check(c, recs, expected(recs, k, {}))  # before any batch: slots only
        assert _rows(_device(c, b"", 3)) == [(0,) * 6] * 3


@pytest.mark.parametrize("state", ["pending", "dense"])
def test_every_allocation_fails_in_turn(state):
    k, reads, table, recs, exp = _small()
    with okm.KmerCounter(k) as c:
        c.add_records(reads, normalized=True)
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
            assert _rows(got) == _rows(exp) if err is None else (err.status == _lib.OKM_E_NOMEM and fired)
            if not fired:
                break  # the call makes fewer allocations than that: it ran untouched
        assert not fired and fail > 4
        assert _table(c) == table


@pytest.mark.parametrize("k,fmt", [(31, "fastq"), (63, "fasta.gz")])
def test_cli(tmp_path, k, fmt):
    ids, recs, inp = dc.cli_records(k)
    table = dc.table_of_records(inp, k)
    fa, gz = tmp_path / "in.fa", fmt != "fastq"
    fa.write_text(dc.fasta_text([f"t{i}" for i in range(len(inp))], inp))
    reads, dep = tmp_path / ("reads." + ("fa.gz" if gz else "fq")), tmp_path / ("s.tsv.gz" if gz else "s.tsv")
    text = dc.fasta_text(ids, recs, width=50) if gz else dc.fastq_text(ids, recs)
    reads.write_bytes(gzip.compress(text.encode()) if gz else text.encode())
    args = [_lib.CLI_PATH, "count", "-k", str(k), "-i", str(fa), "-o", str(tmp_path / "out.tsv"), "--solid-runs",
            str(reads), "--solid-runs-output", str(dep)] + (["--wide"] if k > 32 else [])
    for extra, mc in (([], 2), (["--solid-runs-min-count", "3"], 3)):
        r = subprocess.run(args + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        got = gzip.decompress(dep.read_bytes()).decode() if gz else dep.read_text()
        exp = expected(recs, k, table, mc)
        assert got == "".join(i + "\t" + "\t".join(str(int(x)) for x in row) + "\n" for i, row in zip(ids, exp))
    r = subprocess.run(args + ["--gpus", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2
    assert "the argument '--solid-runs <FASTX>' cannot be used with '--gpus <GPUS>' other than 1" in r.stderr
