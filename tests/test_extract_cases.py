"""CPU self-check of tests/extract_cases.py against the oracle alone: the
conditions under which the GPU tests of tests/test_gpu_extract_edges.py can
see a failure.  A batch whose tail sits behind a separator, or whose records
miss a special length, would keep those tests green whatever the kernels do."""

import numpy as np
import pytest

import extract_cases as X
from oracle import OracleCounter, OracleCounterWide


def _windows(k, data):
    oc = OracleCounterWide(k) if k > 32 else OracleCounter(k)
    oc.add_separated(data)
    return oc.windows


def _assert_tail_joins_poison(k, b):
    """Reading past the batch makes k-mers its table does not have: beside the
    96 - k + 1 windows inside POISON, at least one spans the batch's end."""
    alone, joined = _windows(k, b), _windows(k, np.concatenate([b, X.POISON]))
    if k == 1:
        assert joined > alone
    else:
        assert joined > alone + (X.POISON_LEN - k + 1), (k, len(b), alone, joined)


def test_poison_is_all_valid_bases():
    assert len(X.POISON) == X.POISON_LEN == 96
    assert set(X.POISON.tobytes()) <= set(b"ACGT")
    for k in (1, 31, 64):
        assert _windows(k, X.POISON) == 96 - k + 1


def test_tail_sizes_cover_the_boundaries():
    for k in X.TAIL_KS:
        s = X.TAIL_SIZES(k)
        assert s == sorted(set(s)) and s[0] == 1 and s[-1] == 3 * X.T + 5
        for n in (max(1, k - 1), k, k + 1, 15, 16, 17, 47, 48, 49, 79, 80, 81, X.W - 1, X.W, X.W + 1, X.W + k - 1,
                  X.T - 1, X.T, X.T + 1, X.T + k - 2, X.T + k - 1, X.T + k, 2 * X.T - 1, 2 * X.T, 2 * X.T + 1):
            assert n in s
        assert set(X.TAIL_OFFSET_SIZES(k)) <= set(s)
    assert set(X.TAIL_OFFSET_KS) <= set(X.TAIL_KS)


@pytest.mark.parametrize("k", X.TAIL_KS)
def test_cut_tail_joins_poison(k):
    for n in X.TAIL_SIZES(k):
        b = X.tail_batch(k, n)
        assert len(b) == n and b[-1] != X.SEP
        assert np.array_equal(b, X.tail_batch(k, n))  # seeded: the GPU test counts these bytes
        _assert_tail_joins_poison(k, b)


@pytest.mark.parametrize("k", X.MULTI_KS)
def test_multi_tile_cut_joins_poison(k):
    b = X.multi_tail_batch(k)
    assert len(b) == 4 * X.T + k - 1
    _assert_tail_joins_poison(k, b)


def test_sampled_cut_joins_poison():
    # the GPU test's own 17 MB batch (synth_reads is host code); windows are
    # local, so its last 4 KiB decide what reading past its end would add
    import okm
    k = X.SAMPLED_K
    reads = okm.synth_reads(**X.SAMPLED_READS)
    b = X.sampled_tail(reads)
    assert len(b) == X.SAMPLED_BYTES == 1024 * X.T + 9 and b[-1] != X.SEP
    assert np.array_equal(b[:-(k - 1)], reads[:X.SAMPLED_BYTES - (k - 1)])
    _assert_tail_joins_poison(k, b[-4096:])


def test_ragged_batches_hold_every_special_length_and_repeats():
    for name, k, b in X.ragged_batches():
        assert b[-1] == X.SEP and len(b) in (X.EVERY_K_BYTES, X.MULTI_BYTES), name
        seps = np.flatnonzero(b == X.SEP)
        lens = set(np.diff(np.concatenate([[-1], seps])) - 1)
        assert set(X.special_lengths(k)) <= lens, (name, sorted(set(X.special_lengths(k)) - lens))
        body = b[b != X.SEP]
        assert {ord("N"), ord("U")} <= set(body) and (body >= ord("a")).any(), name
        oc = OracleCounterWide(k) if k > 32 else OracleCounter(k)
        oc.add_separated(b)
        _, counts = oc.result(1)
        assert oc.windows > 0 and counts.max() > 1, name


def test_ragged_is_seeded():
    assert np.array_equal(X.ragged(5, 31, 1000), X.ragged(5, 31, 1000))
    assert not np.array_equal(X.ragged(5, 31, 1000), X.ragged(6, 31, 1000))


def test_byte_value_records():
    recs = X.byte_value_records(31, range(256))
    assert len(recs) == 256 and all(len(r) == 81 and r[40] == b for b, r in enumerate(recs))
    assert all(set(r[:40] + r[41:]) <= set(b"ACGT") for r in recs)
