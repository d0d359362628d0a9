"""Extraction at the edges the synth_reads batches of the other GPU tests never
reach (inputs: tests/extract_cases.py, self-checked on the CPU by
tests/test_extract_cases.py):

  1. every k in 1..64 on ragged records (most k take the runtime-k kernels and
     had never run on a GPU);
  2. batches that end WITHOUT a separator at every size around the load
     granule, the thread loads and the tiles, with valid bases lying behind
     them in the device buffer (the scatter kernels' clamped loads re-read the
     last granule there and must mark those bytes invalid, as the histogram
     kernels' byte-exact loads do);
  3. the sampled placement with a 9-byte last sampled tile;
  4. every byte value between valid flanks;
  5. several tiles per workgroup (test knob l1_max_blocks): the scatter
     kernels' tile loop, otherwise entered a second time only past 134 MB.

Every comparison is exact: keys and counts equal to the oracle's table of
exactly the bytes passed, and engine_info()["kmers"] equal to its windows."""

import numpy as np
import pytest

import extract_cases as X
import okm
from okm import testing
from oracle import OracleCounter, OracleCounterWide, count_separated_mt

pytestmark = pytest.mark.gpu

SLACK = 16  # an unaligned batch starts up to 15 bytes into the buffer


@pytest.fixture(scope="module")
def dbuf():
    buf = okm.DeviceBuffer(X.MULTI_BYTES + X.POISON_LEN + SLACK)
    yield buf
    buf.free()


def _oracle(k, data):
    oc = OracleCounterWide(k) if k > 32 else OracleCounter(k)
    oc.add_separated(data)
    return oc.result(1) + (oc.windows,)


def _assert_table(ctr, want, what):
    ek, ec, windows = want
    gk, gc = ctr.result(1)
    info = ctr.engine_info()
    assert info["kmers"] == windows, (what, info["kmers"], windows)
    assert np.array_equal(gk.reshape(ek.shape), ek) and np.array_equal(gc, ec), what
    return info


def _count_device(ctr, dbuf, batch, want, what, offset=0):
    """The batch from the device buffer, POISON right behind it."""
    dbuf.upload(X.with_poison(batch, offset))
    ctr.reset()
    ctr.add_device_batch(dbuf.address + offset, len(batch))
    return _assert_table(ctr, want, what)


def _records(batch):
    """(bytes, offsets) of a terminated device-layout batch for add_batch."""
    assert batch[-1] == X.SEP
    seps = np.flatnonzero(batch == X.SEP)
    offs = np.zeros(len(seps) + 1, np.uint64)
    offs[1:] = seps - np.arange(len(seps))
    return np.ascontiguousarray(batch[batch != X.SEP]), offs


@pytest.mark.parametrize("k", X.EVERY_K)
def test_every_k_ragged(dbuf, k):
    batch = X.every_k_batch(k)
    want = _oracle(k, batch)
    assert want[2] > 0
    with okm.KmerCounter(k, wide=k > 32) as ctr:
        _count_device(ctr, dbuf, batch, want, ("device", k))
        if k not in X.COVERED_KS:
            data, offs = _records(batch)
            ctr.reset()
            ctr.add_batch(data, offs, normalized=False)
            _assert_table(ctr, want, ("host", k))


@pytest.mark.parametrize("k", X.TAIL_KS)
def test_unterminated_tail_before_valid_bytes(dbuf, k):
    with okm.KmerCounter(k, wide=k > 32) as ctr:
        for n in X.TAIL_SIZES(k):
            batch = X.tail_batch(k, n)
            _count_device(ctr, dbuf, batch, _oracle(k, batch), ("tail", k, n))
        if k in X.TAIL_OFFSET_KS:
            # a pointer off 16-byte alignment is copied to the context's staging
            # buffer first: fill that with valid bases (an all-valid batch, counted
            # and reset), so that what lies behind the next, shorter copies is
            # stale valid bases, not the zeros of a fresh allocation
            rng = np.random.default_rng([6000, k])
            full = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 3 * X.T + X.POISON_LEN)]
            _count_device(ctr, dbuf, full, _oracle(k, full), ("staging fill", k), offset=3)
            for n in X.TAIL_OFFSET_SIZES(k):
                batch = X.tail_batch(k, n)
                _count_device(ctr, dbuf, batch, _oracle(k, batch), ("tail+3", k, n), offset=3)


def test_sampled_placement_short_last_sampled_tile():
    k = X.SAMPLED_K
    batch = X.sampled_tail(okm.synth_reads(**X.SAMPLED_READS))
    n = len(batch)
    assert n == 1024 * X.T + 9 and batch[-1] != X.SEP
    ek, ec = count_separated_mt(batch, k, 16)
    buf = okm.DeviceBuffer(n + X.POISON_LEN)
    try:
        buf.upload(X.with_poison(batch))
        with okm.KmerCounter(k) as ctr:
            ctr.set_timing(True)
            ctr.add_device_batch(buf.address, n)
            _assert_table(ctr, (ek, ec, int(ec.sum())), "sampled")
            stats = ctr.kernel_stats()
    finally:
        buf.free()
    assert stats["extract_sample"]["launches"] == 1


@pytest.mark.parametrize("k", [5, 31, 45])
def test_every_byte_value(dbuf, k):
    wide = k > 32
    recs = X.byte_value_records(k, range(256))
    data, offs = okm.pack_records(recs)
    oc = OracleCounterWide(k) if wide else OracleCounter(k)
    oc.add_batch(data, offs, normalized=False)
    with okm.KmerCounter(k, wide=wide) as ctr:
        ctr.add_batch(data, offs, normalized=False)
        _assert_table(ctr, oc.result(1) + (oc.windows,), ("host", k))
        # the device layout is whitespace-free: the four bytes normalize strips stay out
        dev = [r for b, r in enumerate(recs) if b not in b" \t\r\n"]
        assert len(dev) == 252
        batch = np.frombuffer(b"".join(r + b"\n" for r in dev), np.uint8)
        _count_device(ctr, dbuf, batch, _oracle(k, batch), ("device", k))


def _l1_blocks(n, max_blocks):
    """okm_engine.hip l1_batch: workgroups for n bytes, whole tiles each."""
    tiles = -(-n // X.T)
    chunk = -(-tiles // min(tiles, max_blocks)) * X.T
    return -(-n // chunk)


@pytest.mark.parametrize("k", X.MULTI_KS)
def test_several_tiles_per_workgroup(dbuf, k):
    whole, tail = X.multi_batch(k), X.multi_tail_batch(k)
    assert len(whole) == 5 * X.T + 5 and len(tail) == 4 * X.T + k - 1
    wants = [_oracle(k, whole), _oracle(k, tail)]
    with okm.KmerCounter(k, wide=k > 32) as ctr:
        for knob in (1, 2, 3):
            testing.set_knob("l1_max_blocks", knob)
            for batch, want in zip((whole, tail), wants):
                info = _count_device(ctr, dbuf, batch, want, ("blocks", k, knob, len(batch)))
                assert info["l1_blocks"] == _l1_blocks(len(batch), knob), (k, knob, len(batch))
                assert info["l1_blocks"] <= knob
        assert _l1_blocks(len(whole), 1) == 1  # one workgroup walks all six tiles
        testing.set_knob("l1_max_blocks", -1)
        info = _count_device(ctr, dbuf, whole, wants[0], ("blocks", k, "default"))
        assert info["l1_blocks"] == 6  # the product default: one tile per workgroup
