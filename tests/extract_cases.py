"""Inputs for the extraction edge tests (tests/test_gpu_extract_edges.py) and
their CPU self-check (tests/test_extract_cases.py): seeded, numpy only.

The GPU suite's usual input is a synth_reads batch: equal-length reads, each
ended by a separator.  Three things it cannot see are built here:

  ragged()  records of every awkward length (0, 1, k-1, k, k+1, 2k, and the
            lengths around the kernels' 16-byte load granule and 48-byte
            thread load) with N, lower case and U, cut from a small genome so
            that counts above 1 occur;
  cut()     a batch that does NOT end with a separator: its last k-1 bytes are
            valid bases, so a kernel that reads past n_bytes joins them to
            whatever follows and makes k-mers the oracle's table lacks;
  POISON    what follows: valid bases, written behind the batch in the device
            buffer (and never passed in n_bytes).

The sizes and ks the GPU tests use are listed here too, so that the CPU test
checks exactly the inputs the GPU tests run.
"""

from functools import lru_cache

import numpy as np

# Tile sizes of the extraction kernels (okm_extract.hip: kTile = 1024 threads
# x 16 windows for k <= 32, kTileW1 = 512 x 16 for k in 33..64).  Hard-coded:
# the tests never read kernel sources; a changed tile only moves the sizes
# below off the boundary they aim at.
T = 16384
W = 8192

SEP = ord("\n")
_BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = np.zeros(256, np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP[_a] = _b

GENOME_LEN = 20_000
POISON_LEN = 96
# 96 upper-case bases, no separator
POISON = _BASES[np.random.default_rng(0xBAD5EED).integers(0, 4, POISON_LEN)].copy()
POISON.setflags(write=False)

EVERY_K = tuple(range(1, 65))                       # k <= 32 narrow, k >= 33 wide
EVERY_K_BYTES = 3 * T + 5                           # three tiles and a 5-byte fourth
# ks that test_gpu_parity.py::test_random_vs_oracle / test_gpu_wide.py count already
COVERED_KS = frozenset({1, 2, 5, 11, 15, 17, 21, 25, 27, 31, 32, 33, 45, 63, 64})
TAIL_KS = (1, 13, 16, 31, 32, 33, 48, 63, 64)
TAIL_OFFSET_KS = (31, 63)                           # also from a pointer 3 bytes off 16-B alignment
MULTI_KS = (13, 31, 63)                             # several tiles per workgroup
MULTI_BYTES = 5 * T + 5
SAMPLED_K = 31
SAMPLED_BYTES = 1024 * T + 9                        # sampled placement, last sampled tile of 9 bytes
# okm.synth_reads arguments of the batch that is cut to SAMPLED_BYTES
SAMPLED_READS = dict(n_reads=112_000, read_len=150, genome_len=5_000_000, genome_seed=5, seed=77,
                     sub_rate=0.01, n_rate=0.001)


def special_lengths(k):
    return sorted({0, 1, k - 1, k, k + 1, 2 * k, 15, 16, 17, 47, 48, 49})


def TAIL_SIZES(k):
    s = {1, max(1, k - 1), k, k + 1,
         15, 16, 17, 47, 48, 49, 79, 80, 81,
         W - 1, W, W + 1, W + k - 1,
         T - 1, T, T + 1, T + k - 2, T + k - 1, T + k,
         2 * T - 1, 2 * T, 2 * T + 1,
         3 * T + 5}
    return sorted(s)


def TAIL_OFFSET_SIZES(k):
    return (17, T + k - 1, 2 * T + 1)


def multi_tail_bytes(k):
    return 4 * T + k - 1


def ragged(seed, k, total_bytes):
    """A device-layout batch of exactly total_bytes bytes: records (either
    strand) of a 20 kb random genome, each ended by a separator; ~30 % of the
    lengths from special_lengths(k), the rest uniform in 1..399; per base ~1 %
    N, ~5 % lower case, ~1 % of the Ts written as U."""
    rng = np.random.default_rng(seed)
    genome = _BASES[rng.integers(0, 4, GENOME_LEN)]
    special = special_lengths(k)
    lens = list(special)
    have = sum(lens) + len(lens)
    while have < total_bytes + 400:
        n = int(rng.choice(special)) if rng.random() < 0.3 else int(rng.integers(1, 400))
        lens.append(n)
        have += n + 1
    lens = [lens[i] for i in rng.permutation(len(lens))]
    parts = []
    for n in lens:
        at = int(rng.integers(0, GENOME_LEN - n + 1))
        rec = genome[at:at + n]
        if rng.random() < 0.5:
            rec = _COMP[rec[::-1]]
        parts.append(rec)
        parts.append(np.array([SEP], np.uint8))
    out = np.concatenate(parts)[:total_bytes].copy()
    body = out != SEP
    r = rng.random(len(out))
    u = body & (out == ord("T")) & (r < 0.01)
    out[u] = ord("U")
    r = rng.random(len(out))
    out[body & (r < 0.01)] = ord("N")
    r = rng.random(len(out))
    low = body & (r < 0.05)
    out[low] |= 0x20
    out[-1] = SEP
    return out


def cut(data, n, k, rng):
    """data[:n] with its last min(n, max(k - 1, 1)) bytes overwritten by random
    upper-case bases: an unterminated batch with a valid tail."""
    out = np.array(data[:n], dtype=np.uint8)
    m = min(n, max(k - 1, 1))
    out[n - m:] = _BASES[rng.integers(0, 4, m)]
    return out


def with_poison(batch, offset=0):
    """What the device buffer holds: `offset` filler bytes, the batch, POISON."""
    return np.concatenate([np.full(offset, ord("A"), np.uint8), batch, POISON])


def _frozen(a):
    a.setflags(write=False)
    return a


@lru_cache(maxsize=None)
def every_k_batch(k):
    return _frozen(ragged(1000 + k, k, EVERY_K_BYTES))


@lru_cache(maxsize=None)
def multi_batch(k):
    return _frozen(ragged(2000 + k, k, MULTI_BYTES))


def tail_batch(k, n):
    """The unterminated batch of n bytes the tail tests count at this k."""
    return cut(every_k_batch(k), n, k, np.random.default_rng([3000, k, n]))


def multi_tail_batch(k):
    return cut(multi_batch(k), multi_tail_bytes(k), k, np.random.default_rng([4000, k]))


def sampled_tail(batch, k=SAMPLED_K):
    """cut() of a terminated batch of at least SAMPLED_BYTES bytes."""
    return cut(batch, SAMPLED_BYTES, k, np.random.default_rng([5000, k]))


def ragged_batches():
    """(name, k, batch) of every ragged batch a GPU test counts."""
    for k in EVERY_K:
        yield f"every_k[{k}]", k, every_k_batch(k)
    for k in MULTI_KS:
        yield f"multi[{k}]", k, multi_batch(k)


def byte_value_records(k, values, seed=7):
    """flank + bytes([b]) + flank for every b in values, 40-base random flanks."""
    rng = np.random.default_rng([seed, k])
    recs = []
    for b in values:
        f = _BASES[rng.integers(0, 4, 80)].tobytes()
        recs.append(f[:40] + bytes([b]) + f[40:])
    return recs
