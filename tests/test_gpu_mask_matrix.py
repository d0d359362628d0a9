"""okm_count_mask_matrix on the device, exact against numpy: every count is a
membership mask m, bits = (m >> arange(n_bits)) & 1, M = bits.T @ bits and
occupancy = bincount(bits.sum(1)).  Read from the table where it lies: pending
runs (u32 or u64 counts), dense, host-resident in slices, wide, folded."""

from functools import lru_cache

import numpy as np
import pytest

import hist_cases as hc
import okm
from okm import _lib, testing
from oracle import OracleCounter, OracleCounterWide

pytestmark = pytest.mark.gpu

K = hc.K
N_BITS = [1, 2, 31, 32, 33, 63, 64]


def expected(masks, n_bits):
    masks = np.asarray(masks, dtype=np.uint64)
    bits = ((masks[:, None] >> np.arange(n_bits, dtype=np.uint64)) & np.uint64(1)).astype(np.int64)
    return (bits.T @ bits).astype(np.uint64), np.bincount(bits.sum(1), minlength=n_bits + 1).astype(np.uint64)


def check(got, masks, n_bits):
    m, occ = got
    em, eocc = expected(masks, n_bits)
    assert m.shape == (n_bits, n_bits) and m.dtype == np.uint64 and len(occ) == n_bits + 1
    assert np.array_equal(m, em) and np.array_equal(occ, eocc)
    assert np.array_equal(m, m.T) and int(occ.sum()) == len(masks)
    assert all(int(m[i, i]) == int(((masks >> np.uint64(i)) & np.uint64(1)).sum()) for i in range(n_bits))


def _masks(pattern, n):
    if pattern == "ones":
        return np.full(n, 2 ** 64 - 1, np.uint64)
    if pattern == "round_robin":
        return np.uint64(1) << (np.arange(n, dtype=np.uint64) % np.uint64(64))
    m = np.random.default_rng(n + 7).integers(0, 2 ** 64, n, dtype=np.uint64)
    assert m.all()
    return m


@pytest.mark.parametrize("pattern", ["ones", "round_robin", "random"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 511, 512, 513, 4097, "many_items"])
def test_wave_and_tile_edges(n, pattern):
    if n == "many_items":
        keys = np.unique(hc.many_items())
    else:
        keys = np.unique(np.random.default_rng(n).integers(0, 1 << 62, 2 * n + 8, dtype=np.uint64))[:n]
    masks = _masks(pattern, len(keys))  # keys ascend, so entry e of the table holds masks[e]
    with okm.KmerCounter(K) as c:
        c.set_timing(True)
        if len(keys):
            c.add_pairs(keys, masks)
        assert c.count() == len(keys)
        seen = 0.0
        for state in ("pending", "dense"):
            for n_bits in N_BITS:
                check(c.mask_matrix(n_bits), masks, n_bits)
            if len(keys):
                st = c.kernel_stats()["mask_matrix"]
                assert st["launches"] == len(N_BITS) * (1 + (state == "dense"))
                assert (st["alg_bytes"] - seen) / len(N_BITS) in (4.0 * len(keys), 8.0 * len(keys))  # counts only
                seen = st["alg_bytes"]
            gk, gc = c.result(1)  # the reader after it: exact, and it gathers
            assert np.array_equal(gk, keys) and np.array_equal(gc, masks)


@lru_cache(maxsize=None)
def _reads(k):
    """(device batch bytes, the oracle's counts) of a table counted from reads: u32-staged counts."""
    if k <= 32:
        batch = okm.synth_reads(8_000, 100, genome_len=150_000, genome_seed=8, seed=8)
        oc = OracleCounter(k)
    else:
        batch, _ = okm.synth_long_reads(0.0001, 100_000, genome_seed=6, seed=6, median_len=300.0, min_len=100,
                                        max_len=3000)
        oc = OracleCounterWide(k)
    oc.add_separated(batch)
    return batch, oc.result(1)[1]


@pytest.fixture
def counted(request):
    k = getattr(request, "param", K)
    batch, ec = _reads(k)
    buf = okm.DeviceBuffer(len(batch), 0)
    buf.upload(batch)
    with okm.KmerCounter(k, wide=k > 32) as c:
        c.set_timing(True)
        c.add_device_batch(buf.address, len(batch))
        assert c.count() == len(ec)
        yield c, ec
    buf.free()


def test_narrow_counts(counted):
    c, ec = counted
    check(c.mask_matrix(8), ec, 8)
    assert c.kernel_stats()["mask_matrix"]["alg_bytes"] == 4.0 * len(ec)


@pytest.mark.parametrize("counted", [33, 63], indirect=True)
def test_wide(counted):
    c, ec = counted
    for n_bits in (3, 64):
        check(c.mask_matrix(n_bits), ec, n_bits)


def _to_host_table(c):
    testing.set_knob("fail_alloc", 1)  # the dense gather's first allocation fails: the table stays in host memory
    c.result(1)
    assert testing.get_knob("fail_alloc") == -1 and c.engine_info()["host_bytes"] > 0


def test_host_resident_table_in_slices(counted):
    c, ec = counted
    _to_host_table(c)
    try:
        for sl in (1000, 4096, len(ec)):  # a ragged last slice, several slices, exactly one
            testing.set_knob("hist_slice", sl)
            check(c.mask_matrix(5), ec, 5)
    finally:
        testing.set_knob("hist_slice", -1)
    assert c.engine_info()["host_bytes"] > 0  # still host-resident


def test_folded_table():
    a, b = hc.fold_pairs()
    with okm.KmerCounter(K) as c:
        c.add_pairs(a)
        c.count()
        c.add_pairs(b)
        check(c.mask_matrix(6), hc.table_of(np.concatenate([a, b]))[1], 6)  # counts the pending batch first


def test_errors():
    lib = _lib.load()
    buf = np.full(64 * 64, 9, np.uint64)
    with okm.KmerCounter(K) as c:
        for n_bits in (0, 65):
            assert lib.okm_count_mask_matrix(c.ctx, n_bits, buf.ctypes.data, None) == _lib.OKM_E_ARG
        assert lib.okm_count_mask_matrix(c.ctx, 8, None, None) == _lib.OKM_E_ARG
        m, occ = c.mask_matrix(64)  # an empty context: zeros
        assert not m.any() and not occ.any()
    with okm.KmerCounter(K, "set") as s:
        s.add_pairs(np.arange(1, 100, dtype=np.uint64))
        assert lib.okm_count_mask_matrix(s.ctx, 8, buf.ctypes.data, None) == _lib.OKM_E_STATE


@pytest.mark.parametrize("state", ["pending", "host"])
def test_every_allocation_fails_in_turn(counted, state):
    c, ec = counted
    if state == "host":
        _to_host_table(c)
        testing.set_knob("hist_slice", 5000)
    big = 10 ** 9
    try:
        testing.set_knob("fail_alloc", big)
        check(c.mask_matrix(7), ec, 7)
        n_gets = big - testing.get_knob("fail_alloc")
        assert n_gets == (3 if state == "host" else 2)  # the result, the partials; the upload slice
        for fail in range(1, n_gets + 1):
            in_use = testing.device_in_use(c)
            testing.set_knob("fail_alloc", fail)
            try:
                check(c.mask_matrix(7), ec, 7)
            except okm.OkmError as e:
                assert e.status == _lib.OKM_E_NOMEM, (fail, e)
            assert testing.get_knob("fail_alloc") == -1, f"allocation {fail}: the failure did not fire"
            assert testing.device_in_use(c) == in_use, f"allocation {fail}: a block was stranded"
            check(c.mask_matrix(7), ec, 7)  # the table is intact: again, cleanly
    finally:
        testing.set_knob("fail_alloc", -1)
        testing.set_knob("hist_slice", -1)
