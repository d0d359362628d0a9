"""Inputs for the probe edge tests (tests/test_gpu_probe_edges.py) and their
CPU self-check (tests/test_probe_cases.py): seeded, numpy only.

The kernels of okm_probe.hip (hash set, hash map, query, classify) are aimed at
where the random MB-scale inputs of tests/test_gpu_query_classify.py do not
reach:

  wrap_keys()      canonical k-mers whose home slot is one of the last two of a
                   1024-slot table: the linear probe of all but two of them
                   crosses the table's end;
  distinct_keys()  distinct keys by construction, for the sizes past the grid
                   caps, where a sort or a Python set costs more than the test;
  LAYOUTS          reference-length layouts for classify: empty references
                   first / last / in runs, several references inside one
                   thread's keys, references that end at thread and block
                   boundaries, keys shared by every reference;
  query_batch()    extract_cases.ragged() records and the set of every second
                   canonical k-mer of their genome; runs of empty records;
                   cut_batch(): an unterminated batch whose tail joins POISON
                   to k-mers that ARE in the set (cut_set), so that a kernel
                   reading past n_bytes counts hits the oracle does not.

The constants the cases aim at are restated here, never read from the kernel
sources: if one changes, a case only loses its aim.
"""

from functools import lru_cache

import numpy as np

import extract_cases as X

# okm_probe.hip, restated ------------------------------------------------------
FMIX_M1 = 0xFF51AFD7ED558CCD        # murmur3 fmix64 multipliers (slot_hash)
FMIX_M2 = 0xC4CEB9FE1A85EC53
MIN_CAP = 1024                      # smallest table (pow2_at_least)
Q_TILE = 4096                       # bytes per query block: 256 threads x
Q_SEG = 16                          #   16 window starts
Q_LOAD = 48                         # bytes a query thread loads (16 + 32 halo)
C_PER = 8                           # classify: reference keys per thread
C_BLOCK = 2048                      #   and per block (256 threads)
GRID_CAP = 1 << 24                  # grid_for: 65536 blocks x 256 threads
ISECT_GRID_CAP = 1 << 21            # k_intersect_count: 8192 blocks x 256 threads

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)   # ~0: the empty slot, kept in a side flag
SEP = X.SEP
POISON = X.POISON                       # 96 valid upper-case bases
_BASES = np.frombuffer(b"ACGT", np.uint8)


def _frozen(a):
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------------------
# hashing
# ---------------------------------------------------------------------------

def slot_hash(keys):
    """murmur3 fmix64 of a uint64 array (numpy's uint64 arithmetic wraps)."""
    x = np.array(keys, dtype=np.uint64, copy=True).reshape(-1)
    x ^= x >> np.uint64(33)
    x *= np.uint64(FMIX_M1)
    x ^= x >> np.uint64(33)
    x *= np.uint64(FMIX_M2)
    x ^= x >> np.uint64(33)
    return x


def home(keys, cap):
    """Home slot in a cap-slot table: the hash's top log2(cap) bits."""
    bits = int(cap).bit_length() - 1
    assert 1 << bits == cap and bits >= 1
    return slot_hash(keys) >> np.uint64(64 - bits)


# ---------------------------------------------------------------------------
# k-mer arithmetic on arrays (builds INPUTS only; expectations come from the
# oracle and from oracle/restate.py)
# ---------------------------------------------------------------------------

def revcomp_values(v, k):
    v = np.asarray(v, dtype=np.uint64)
    rc = np.zeros_like(v)
    for i in range(k):
        b = (v >> np.uint64(2 * i)) & np.uint64(3)
        rc |= (np.uint64(3) - b) << np.uint64(2 * (k - 1 - i))
    return rc


_CODE = np.full(256, 4, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _CODE[_c | 0x20] = _i


def canonical_kmers(seq, k):
    """Canonical k-mer of every valid window of a byte array (A/C/G/T in
    either case valid, as query.rs), in window order."""
    seq = np.asarray(seq, dtype=np.uint8)
    nw = len(seq) - k + 1
    if nw <= 0:
        return np.zeros(0, np.uint64)
    code = _CODE[seq]
    bad = np.concatenate([[0], np.cumsum(code == 4)])
    valid = (bad[k:] - bad[:nw]) == 0
    c = (code & 3).astype(np.uint64)
    fw = np.zeros(nw, np.uint64)
    rc = np.zeros(nw, np.uint64)
    for j in range(k):
        fw |= c[j:j + nw] << np.uint64(2 * (k - 1 - j))
        rc |= (np.uint64(3) - c[j:j + nw]) << np.uint64(2 * j)
    return np.minimum(fw, rc)[valid]


# ---------------------------------------------------------------------------
# hash set / map inputs
# ---------------------------------------------------------------------------

DISTINCT_MULT = 0x9E3779B97F4A7C15      # odd: i -> i * MULT is a bijection mod 2^62


def distinct_keys(n, start=0):
    """n keys below 2^62, distinct from each other and from every
    distinct_keys(m, s) whose index range [s, s + m) is disjoint from
    [start, start + n) (both inside 0..2^62): no sort, no set."""
    i = np.arange(start, start + n, dtype=np.uint64)
    return (i * np.uint64(DISTINCT_MULT)) & np.uint64((1 << 62) - 1)


@lru_cache(maxsize=None)
def _wrap_pool(cap, k, need):
    rng = np.random.default_rng([0x3A9, cap, k])
    got = np.zeros(0, np.uint64)
    hi = 1 << (2 * k)
    for _ in range(64):  # about 1 candidate in 512 * 2 qualifies at cap = 1024
        v = rng.integers(0, hi, size=1 << 20, dtype=np.uint64)
        v = v[home(v, cap) >= np.uint64(cap - 2)]
        v = v[v <= revcomp_values(v, k)]  # canonical_u64(v, k) == v
        got = np.unique(np.concatenate([got, v]))
        if len(got) >= need:
            break
    assert len(got) >= need, (cap, k, len(got), need)
    return _frozen(got[np.random.default_rng([0x3AA, cap, k]).permutation(len(got))][:need].copy())


def wrap_keys(cap, k, n_present, n_absent):
    """(present, absent): disjoint canonical k-mer values whose home is one of
    the last two slots of a cap-slot table.  At most two of `present` fit
    there, so whatever order they are inserted in, the others continue at
    slot 0; an absent key is a miss only after a probe that walks that
    wrapped cluster to its empty slot."""
    pool = _wrap_pool(cap, k, n_present + n_absent)
    return pool[:n_present], pool[n_present:n_present + n_absent]


WRAP_KS = (31, 13)      # a compile-time-k and a runtime-k query kernel
# A set created with capacity_hint <= 256 has MIN_CAP = 1024 slots, and an
# insert of n keys (duplicates count) grows the table when 2 * (size + n) >
# 1024.  The first insert below passes 236 keys and leaves size = 220; giving
# the same 236 again needs 2 * (220 + 236) = 912 slots: the table, and with it
# the wrapped cluster, stays as built until the growth batches.
N_WRAP = 40
N_FILL = 180
N_DUP = 16


def _fresh(rng, n, k, taken):
    """n distinct values below 4^k, none of them in `taken`."""
    out = np.zeros(0, np.uint64)
    while len(out) < n:
        v = np.unique(rng.integers(0, 1 << (2 * k), size=2 * n + 64, dtype=np.uint64))
        v = v[~np.isin(v, taken) & ~np.isin(v, out)]
        out = np.concatenate([out, rng.permutation(v)])
    return out[:n]


@lru_cache(maxsize=None)
def set_case(k):
    """The hash-set case at this k: see the field comments."""
    rng = np.random.default_rng([0x5E7, k])
    present, absent = wrap_keys(MIN_CAP, k, N_WRAP, N_WRAP)
    wrap = np.concatenate([present, absent])
    fill = _fresh(rng, N_FILL, k, wrap)
    members = np.concatenate([present, fill])
    first = rng.permutation(np.concatenate([members, members[rng.integers(0, len(members), N_DUP)]]))
    taken = np.concatenate([wrap, fill])
    grow1_new = _fresh(rng, 400, k, taken)
    taken = np.concatenate([taken, grow1_new])
    grow2_new = _fresh(rng, 1500, k, taken)
    taken = np.concatenate([taken, grow2_new])
    others = _fresh(rng, 500, k, taken)
    case = dict(
        present=present, absent=absent, fill=fill,
        first=first,                            # one insert: 220 distinct keys + 16 duplicates (<= 256)
        n_first=len(members),
        # two growths (1024 -> 2048 -> 8192 slots), each batch with keys that are
        # already there and duplicates of its own
        grow1=rng.permutation(np.concatenate([grow1_new, members[:50], grow1_new[:7]])), n_grow1=400,
        grow2=rng.permutation(np.concatenate([grow2_new, grow1_new[:90], present, grow2_new[:11]])), n_grow2=1500,
        non_members=np.concatenate([absent, others]),
    )
    case["all_members"] = np.concatenate([members, grow1_new, grow2_new])
    assert len(first) <= 256 and 2 * (len(members) + len(first)) <= MIN_CAP
    return {n: (_frozen(v) if isinstance(v, np.ndarray) else v) for n, v in case.items()}


# contains() past the grid cap: GRID_CAP + 300 probes, so that 300 threads take a
# second grid-stride step.  Probe i is member (i mod CONTAINS_SET) of a 1 M-key
# set unless i % 3 == 0, when it is key CONTAINS_SET + i, which no set index is.
CONTAINS_SET = 1 << 20
CONTAINS_PROBES = GRID_CAP + 300


def contains_probes():
    i = np.arange(CONTAINS_PROBES, dtype=np.uint64)
    miss = (i % np.uint64(3)) == 0
    idx = np.where(miss, i + np.uint64(CONTAINS_SET), i % np.uint64(CONTAINS_SET))
    return (idx * np.uint64(DISTINCT_MULT)) & np.uint64((1 << 62) - 1), ~miss


# Rehash past the grid cap: capacity_hint 2^24 gives 2^25 slots; 1 M keys and ~0
# go in; 2^24 more keys need 2 * (2^20 + 1 + 2^24) > 2^25 slots, so the table
# grows once, to 2^26, and k_set_rehash walks old_cap + 1 = 2^25 + 1 words with
# 2^24 threads: every thread loops, and the flag word at index 2^25 belongs to
# thread 0's third step.  Device memory: 256 MB old + 512 MB new table + 151 MB
# of uploaded keys.
REHASH_HINT = 1 << 24
REHASH_FIRST = 1 << 20
REHASH_SECOND = 1 << 24

# Intersection past its grid cap.  The kernel probes the SMALLER array into the
# larger, so b must be the longer one for a's 2^21 + 5 keys to be the probes:
# a = {3 i}; b = {3 i : i even} + {3 i + 1} + {3 i + 2 : i % 4 == 0}.
ISECT_NA = ISECT_GRID_CAP + 5


def intersect_case(na=ISECT_NA):
    """(a, b, |a & b|): sorted distinct keys, the answer known by construction."""
    i = np.arange(na, dtype=np.uint64)
    a = i * np.uint64(3)
    b = np.sort(np.concatenate([a[::2], a + np.uint64(1), a[::4] + np.uint64(2)]))
    return a, b, (na + 1) // 2


# ---------------------------------------------------------------------------
# classify inputs
# ---------------------------------------------------------------------------

CLASSIFY_K = 31
MIN_FREQ = 3                        # counts MIN_FREQ - 1, MIN_FREQ, MIN_FREQ + 1 in turn
BIG = 1 << 40                       # a few counts near 2^40: depth sums pass 2^32
ABOVE_ALL = (1 << 40) + 1000        # a min_freq above every count
N_INPUT = 6000

LONG = [0, 0, 3, 0, 5, 1, 1, 0, 2, 2040, 0, 2048, 1, 4095, 0, 0]
LAYOUTS = {
    # offsets 0 0 3 3 8 9 10 10 12 2052 2052 4100 4101 8196 8196 8196: first and
    # last references empty, a reference that ends at key 8, thread 1 (keys
    # 8..15) in four references, blocks 3 and 4 wholly inside the 4095-key one
    "long": LONG,
    "one_key": [1],
    "one_block": [2048],            # ends exactly with the block
    "block_plus_one": [2049],       # a second block of one key
    "short_run": [int(x) for x in np.random.default_rng(0xC1A).integers(0, 4, 40)],  # 40 references of 0..3 keys
    "all_empty": [0, 0, 0, 0, 0],
    # references that are exactly one block each, an empty one on the block
    # boundary between them, then 8-key references (exactly one thread each)
    "block_aligned": [2048, 0, 2048, 8, 0, 0, 8, 5],
}


@lru_cache(maxsize=None)
def classify_input():
    """(keys, counts) for KmerCounter.add_pairs: distinct keys below 4^31,
    counts cycling through MIN_FREQ - 1, MIN_FREQ, MIN_FREQ + 1, five of them
    raised to about 2^40."""
    rng = np.random.default_rng(0xC1B)
    keys = np.sort(_fresh(rng, N_INPUT, CLASSIFY_K, np.zeros(0, np.uint64)))
    counts = (np.arange(N_INPUT, dtype=np.uint64) % np.uint64(3)) + np.uint64(MIN_FREQ - 1)
    counts[[0, 1, 2, 1000, N_INPUT - 1]] = np.array([BIG, BIG + 1, BIG - 1, BIG + 7, BIG + 999], np.uint64)
    return _frozen(keys), _frozen(counts)


def common_keys():
    """(an input key every non-empty reference holds, a foreign key every
    reference of three keys or more holds).  The input key's count is 2^40."""
    ik, _ = classify_input()
    return ik[0], np.uint64((1 << 61) + 12345)


def _refs(lengths, ik, foreign, common_in, common_foreign, rng):
    refs = []
    biggest = int(np.argmax(lengths)) if max(lengths) >= 2 else -1
    fi = 0
    for r, n in enumerate(lengths):
        if n == 0:
            refs.append(np.zeros(0, np.uint64))
            continue
        fixed = [common_in]
        if n >= 3:
            fixed.append(common_foreign)
        if r == biggest:
            fixed.append(EMPTY)
        fixed = np.array(fixed[:n], np.uint64)
        rest = n - len(fixed)
        n_in = (rest + 1) // 2          # about half of the keys are input keys
        pool = ik[ik != common_in]
        mine = [fixed, rng.choice(pool, n_in, replace=False), foreign[fi:fi + rest - n_in]]
        fi += rest - n_in               # foreign keys other than the common one occur once
        refs.append(rng.permutation(np.concatenate(mine)).astype(np.uint64))
    return refs


@lru_cache(maxsize=None)
def _foreign():
    ik, _ = classify_input()
    rng = np.random.default_rng(0xC1C)
    return _frozen(_fresh(rng, 12000, CLASSIFY_K, np.concatenate([ik, [common_keys()[1]]])))


@lru_cache(maxsize=None)
def layout_refs(name):
    """The references (one key array each, no key twice within one) of a
    layout: about half of each reference's keys are input keys; one input key
    is in every non-empty reference and one foreign key in every reference of
    three keys or more (the union insert's race: one insert wins); the
    longest reference holds ~0."""
    ik, _ = classify_input()
    cin, cfo = common_keys()
    rng = np.random.default_rng([0xC1D, sorted(LAYOUTS).index(name)])
    return tuple(_frozen(r) for r in _refs(LAYOUTS[name], ik, _foreign(), cin, cfo, rng))


@lru_cache(maxsize=None)
def map_wrap_case():
    """(input keys, input counts, references) with <= 512 input keys, so that
    the input map has MIN_CAP slots: 30 wrap keys and 200 others go in, and the
    references hold them, 30 absent wrap keys and foreign keys."""
    rng = np.random.default_rng(0xC1E)
    present, absent = wrap_keys(MIN_CAP, CLASSIFY_K, 30, 30)
    fill = _fresh(rng, 200, CLASSIFY_K, np.concatenate([present, absent]))
    ik = np.concatenate([present, fill])
    order = np.argsort(ik)
    ik = ik[order]
    ic = (np.arange(len(ik), dtype=np.uint64) % np.uint64(5)) + np.uint64(1)
    foreign = _fresh(rng, 100, CLASSIFY_K, np.concatenate([ik, absent]))
    refs = (rng.permutation(np.concatenate([present, absent[:15], fill[:50], foreign[:40]])),
            rng.permutation(np.concatenate([absent, present[:20], foreign[30:]])),
            rng.permutation(np.concatenate([present[10:], fill[40:]])))
    assert len(ik) <= 512
    return _frozen(ik), _frozen(ic), tuple(_frozen(r.astype(np.uint64)) for r in refs)


def classify_expected(refs, ik, ic, min_freq):
    """What classify.rs:195-308 gives for the references `refs` and the input
    table (ik, ic) filtered at min_freq (ic None: every count is 1)."""
    ik = np.asarray(ik, np.uint64)
    ic = np.ones(len(ik), np.uint64) if ic is None else np.asarray(ic, np.uint64)
    keep = ic >= np.uint64(min_freq)
    order = np.argsort(ik[keep])
    fk, fc = ik[keep][order], ic[keep][order]

    def stats(keys):
        if len(fk) == 0 or len(keys) == 0:
            return 0, 0
        pos = np.minimum(np.searchsorted(fk, keys), len(fk) - 1)
        m = fk[pos] == keys
        return int(m.sum()), sum(int(c) for c in fc[pos[m]])

    per = [stats(np.asarray(r, np.uint64)) for r in refs]
    uni = np.unique(np.concatenate([np.asarray(r, np.uint64) for r in refs])) if len(refs) else np.zeros(0, np.uint64)
    um, us = stats(uni)
    return {"n_input": int(keep.sum()),
            "ref_matched": [p[0] for p in per], "ref_sum_depth": [p[1] for p in per],
            "union": int(len(uni)), "matched": um, "sum_depth": us}


# ---------------------------------------------------------------------------
# query inputs
# ---------------------------------------------------------------------------

EVERY_K = tuple(range(1, 33))
CUT_KS = (1, 13, 16, 21, 25, 27, 31, 32)    # the five compile-time kernels, 2k = 32, odd and k = 1 runtime ones
CUT_OFFSET_KS = (31, 25)                    # also from a pointer 3 bytes off 16-B alignment
QUERY_BYTES = 2 * Q_TILE + 5                # two tiles and a 5-byte third


def QUERY_TAIL_SIZES(k):
    s = {1, max(1, k - 1), k, k + 1,
         Q_SEG - 1, Q_SEG, Q_SEG + 1, Q_LOAD - 1, Q_LOAD, Q_LOAD + 1,
         Q_TILE - 1, Q_TILE, Q_TILE + 1, Q_TILE + k - 2, Q_TILE + k - 1, Q_TILE + k,
         2 * Q_TILE + 5}
    return sorted(s)


def _seed(k):
    return 7000 + k


@lru_cache(maxsize=None)
def query_genome(k):
    """The genome extract_cases.ragged(_seed(k), ...) cuts its records from
    (its generator's first draw; tests/test_probe_cases.py checks that the
    batch's windows do hit this genome's k-mers)."""
    return _frozen(_BASES[np.random.default_rng(_seed(k)).integers(0, 4, X.GENOME_LEN)])


@lru_cache(maxsize=None)
def query_batch(k):
    """QUERY_BYTES bytes in the device layout: one record of every special
    length (0, 1, k-1, k, k+1, 2k, 15..17, 47..49), then ragged records, with
    N, lower case and U."""
    g = query_genome(k)
    head = []
    for i, n in enumerate(X.special_lengths(k)):
        head += [g[37 * i:37 * i + n], np.array([SEP], np.uint8)]
    head = np.concatenate(head)
    return _frozen(np.concatenate([head, X.ragged(_seed(k), k, QUERY_BYTES - len(head))]))


@lru_cache(maxsize=None)
def genome_set(k):
    """Every second canonical k-mer (in key order) of the genome: sorted."""
    return _frozen(np.unique(canonical_kmers(query_genome(k), k))[::2].copy())


def records_of(batch):
    """The records of a device-layout batch: a final separator ends the last
    record; without one the last record is what follows the last separator."""
    b = bytes(np.asarray(batch, np.uint8))
    recs = b.split(b"\n")
    return recs[:-1] if b.endswith(b"\n") else recs


def host_records(k):
    """The ragged records for the host entry, which takes raw record bytes:
    two more with bytes the device layout cannot hold or the ragged batch has
    in few places (an inner line break, which kills windows but does not end
    the record; U)."""
    g = query_genome(k).tobytes()
    return records_of(query_batch(k)) + [g[100:160] + b"\n" + g[160:230], g[300:340] + b"U" + g[341:400]]


@lru_cache(maxsize=None)
def empty_run_records(k, run):
    """Records around `run` empty records in a row.  Their separators are bytes
    4088.. of the device layout (behind the separator of the record before
    them at 4087): with run = 40 they cross the tile boundary at
    4096, and threads in it step their record index at every window; with
    run = 4096 + 17 it also covers the whole tile 4096..8191, which is then
    nothing but separators."""
    g = query_genome(k).tobytes()
    recs = [g[500:599], b"N" * 3987]                # 100 + 3988 bytes with their separators
    recs += [b""] * run
    recs += [g[700:700 + n] for n in (k, 2 * k + 3, 90)] + [b"", g[900:1000]]
    return tuple(recs)


EMPTY_RUNS = (40, Q_TILE + 17)


def layout_bytes(recs):
    """The device layout of records: each followed by a separator."""
    return np.frombuffer(b"".join(r + b"\n" for r in recs), np.uint8)


def cut_batch(k, n):
    """query_batch(k) cut to n bytes, its last k - 1 bytes (k = 1: one byte)
    valid bases: an unterminated batch."""
    return X.cut(query_batch(k), n, k, np.random.default_rng([8000, k, n]))


def _join_kmers(k, cut):
    """The canonical k-mers of the windows that start inside the batch and end
    in POISON, were POISON read as its continuation."""
    if k == 1:
        return np.zeros(0, np.uint64)
    return canonical_kmers(np.concatenate([cut[-(k - 1):], POISON[:k - 1]]), k)


@lru_cache(maxsize=None)
def cut_set(k):
    """The set the cut batches are queried against: genome_set(k) and, for
    every size, the k-mers that join the batch's tail to POISON.  A kernel that
    reads past n_bytes finds those and reports hits the oracle, which sees the
    cut records alone, does not.  (k = 1 has no joining window; there POISON's
    own A and T are members.)"""
    parts = [genome_set(k)] + [_join_kmers(k, cut_batch(k, n)) for n in QUERY_TAIL_SIZES(k)]
    return _frozen(np.unique(np.concatenate(parts)))


def with_poison(batch, offset=0):
    """What the device buffer holds: `offset` filler bytes, the batch, POISON."""
    return X.with_poison(batch, offset)


# fewer records than the batch holds: the record after the last one asked for
# has hits (test_probe_cases.py), which must not be written
SHORT_K = 21
SHORT_DROP = 6
