"""CPU self-check of tests/probe_cases.py: every case aims where it says, and
every expectation the GPU tests of tests/test_gpu_probe_edges.py compare
against is computed twice, by implementations that share no code (the C
restatement and oracle/restate.py for query; numpy and a dict-and-loop
restatement for classify; numpy and Python-integer fmix64 for the hash)."""

import numpy as np
import pytest

import okm
import oracle
import probe_cases as P
import restate

M64 = (1 << 64) - 1


def _fmix64(x):
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & M64
    x ^= x >> 33
    return x


# ---------------------------------------------------------------------------
# hash, wrap keys, set inputs
# ---------------------------------------------------------------------------

def test_slot_hash_is_fmix64():
    rng = np.random.default_rng(1)
    v = np.concatenate([rng.integers(0, 1 << 63, 300, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
                        np.array([0, 1, 2, M64, M64 - 1, 1 << 63, (1 << 62) - 1], np.uint64)])
    got = P.slot_hash(v)
    assert [int(x) for x in got] == [_fmix64(int(x)) for x in v]
    assert _fmix64(1) == 0xB456BCFC34C2CB2C  # murmur3's published avalanche of 1
    for cap in (1024, 2048, 1 << 25):
        bits = cap.bit_length() - 1
        assert [int(x) for x in P.home(v, cap)] == [_fmix64(int(x)) >> (64 - bits) for x in v]


def _probe_model(keys, cap):
    """Linear probing, one key at a time: slot of every key."""
    slots = {}
    where = {}
    for key in keys:
        s = int(P.home(np.array([key], np.uint64), cap)[0])
        while s in slots:
            s = (s + 1) & (cap - 1)
        slots[s] = int(key)
        where[int(key)] = s
    return slots, where


@pytest.mark.parametrize("k", sorted(set(P.WRAP_KS + (P.CLASSIFY_K,))))
def test_wrap_keys_wrap(k):
    cap = P.MIN_CAP
    present, absent = P.wrap_keys(cap, k, P.N_WRAP, P.N_WRAP)
    assert len(present) == len(absent) == P.N_WRAP > 2
    both = np.concatenate([present, absent])
    assert len(set(both.tolist())) == 2 * P.N_WRAP  # distinct, present and absent disjoint
    assert (P.home(both, cap) >= cap - 2).all() and (P.home(both, cap) < cap).all()
    for v in both.tolist():
        assert v < 4 ** k and okm.canonical_u64(v, k) == v and restate.canonical_u64(v, k) == v
    # pigeonhole: two slots at the end, so >= n - 2 keys wrap in any order; the
    # model, in two orders, fills slots 0, 1, ... without a gap
    for order in (present, present[::-1]):
        slots, _ = _probe_model(order, cap)
        low = sorted(s for s in slots if s < cap - 2)
        assert low == list(range(len(low))) and len(low) >= P.N_WRAP - 2
    # an absent key's probe walks from its home through the wrap to the first
    # empty slot: at least the wrapped keys
    slots, _ = _probe_model(present, cap)
    for key in absent.tolist():
        s, steps = int(P.home(np.array([key], np.uint64), cap)[0]), 0
        while s in slots:
            s, steps = (s + 1) & (cap - 1), steps + 1
        assert steps >= P.N_WRAP - 1 and s < cap - 2


@pytest.mark.parametrize("k", P.WRAP_KS)
def test_set_case(k):
    c = P.set_case(k)
    first = c["first"]
    # the first insert and its repetition stay within the 1024-slot table
    assert len(first) <= 256 and 2 * (c["n_first"] + len(first)) <= P.MIN_CAP
    assert len(set(first.tolist())) == c["n_first"] == P.N_WRAP + P.N_FILL < len(first)  # duplicates inside
    assert set(c["present"].tolist()) <= set(first.tolist())
    assert not set(c["absent"].tolist()) & set(first.tolist())
    # each growth batch: new keys, keys already present, duplicates; each forces a growth
    seen = set(first.tolist()) | {int(P.EMPTY)}
    cap = P.MIN_CAP
    for name in ("grow1", "grow2"):
        b = c[name]
        assert 2 * (len(seen) + len(b)) > cap
        while cap < 2 * (len(seen) + len(b)):
            cap *= 2
        assert len(set(b.tolist()) - seen) == c["n_" + name]
        assert set(b.tolist()) & seen and len(set(b.tolist())) < len(b)
        seen |= set(b.tolist())
    assert seen - {int(P.EMPTY)} == set(c["all_members"].tolist())
    assert not set(c["non_members"].tolist()) & seen
    assert all(v < 4 ** k for v in seen - {int(P.EMPTY)})
    # the wrap keys still sit in a wrapped cluster with the fillers around them
    slots, where = _probe_model(first, P.MIN_CAP)
    assert sum(1 for key in c["present"].tolist() if where[key] < P.MIN_CAP - 2) >= P.N_WRAP - 2


def test_distinct_keys():
    a = P.distinct_keys(100_000)
    b = P.distinct_keys(50_000, start=100_000)
    assert P.DISTINCT_MULT % 2 == 1  # a bijection mod 2^62: distinct indices, distinct keys
    assert len(np.unique(np.concatenate([a, b]))) == 150_000
    assert int(a.max()) < 1 << 62 and a[1] == P.DISTINCT_MULT & ((1 << 62) - 1)
    assert np.array_equal(P.distinct_keys(7, start=3), P.distinct_keys(10)[3:])


def test_contains_probes_pattern():
    assert P.CONTAINS_PROBES == (1 << 24) + 300 > P.GRID_CAP
    keys, member = P.contains_probes()
    assert len(keys) == P.CONTAINS_PROBES
    # a sample, the start and the part past the grid cap against a Python set
    members = set(P.distinct_keys(P.CONTAINS_SET).tolist())
    idx = np.concatenate([np.arange(2000), np.arange(P.GRID_CAP - 50, P.CONTAINS_PROBES),
                          np.random.default_rng(2).integers(0, P.CONTAINS_PROBES, 20000)])
    assert [int(x) in members for x in keys[idx]] == member[idx].tolist()
    tail = member[P.GRID_CAP:]
    assert tail.any() and not tail.all()


def test_rehash_sizes():
    # okm_kset_create: pow2 >= 2 * hint slots; growth when 2 * (size + n) > slots
    cap = 2 * P.REHASH_HINT
    assert cap == 1 << 25 and cap >= P.GRID_CAP
    assert 2 * (P.REHASH_FIRST + 1) <= cap
    need = 2 * (P.REHASH_FIRST + 1 + P.REHASH_SECOND)
    assert cap < need <= 2 * cap  # one growth, to 2^26
    # peak device memory: old and new table, the uploaded keys (+ 1/8 slack)
    assert 8 * (cap + 1) + 8 * (2 * cap + 1) + 9 * P.REHASH_SECOND * 9 // 8 < 1 << 30


def test_intersect_case():
    a, b, want = P.intersect_case(1001)
    assert want == len(set(a.tolist()) & set(b.tolist())) == 501
    a, b, want = P.intersect_case()
    assert len(a) == (1 << 21) + 5 and len(b) > len(a)  # a is the probing side
    assert (np.diff(a.astype(np.int64)) > 0).all() and (np.diff(b.astype(np.int64)) > 0).all()
    assert want == int(np.isin(a, b).sum())
    assert np.isin(a[P.ISECT_GRID_CAP:], b).tolist() == [True, False, True, False, True]


# ---------------------------------------------------------------------------
# query
# ---------------------------------------------------------------------------

def _both(recs, keys, k):
    """Per-record hits by the C restatement, checked against the pure-Python one."""
    got = oracle.query_hits(list(recs), keys, k)
    kset = set(keys.tolist())
    assert got.tolist() == [restate.query_hits(r, k, kset) for r in recs]
    return got


def _valid_windows(recs, k):
    return sum(sum(restate.seq_to_u64(r[i:i + k], k) is not None for i in range(len(r) - k + 1)) for r in recs)


@pytest.mark.parametrize("k", P.EVERY_K)
def test_query_cases(k):
    batch = P.query_batch(k)
    assert len(batch) == P.QUERY_BYTES == 2 * 4096 + 5 and batch[-1] == P.SEP
    recs = P.records_of(batch)
    assert len(recs) == int((batch == P.SEP).sum())
    assert {len(r) for r in recs} >= {0, 1, k - 1, k, k + 1, 2 * k, 15, 16, 17, 47, 48, 49}
    body = batch[batch != P.SEP]
    assert {ord("N"), ord("U")} <= set(body.tolist()) and (body >= ord("a")).any()
    keys = P.genome_set(k)
    # the set: every second canonical k-mer of the genome, by the C restatement too
    oc = oracle.OracleCounter(k)
    oc.add_records([P.query_genome(k).tobytes()])
    assert np.array_equal(keys, oc.result(1)[0][::2])
    hits = _both(recs, keys, k)
    windows = _valid_windows(recs, k)
    # the records do come from that genome: hits and misses both in bulk
    assert windows > 4000 and windows // 5 < int(hits.sum()) < windows - windows // 5
    host = P.host_records(k)
    assert host[:len(recs)] == recs and b"\n" in host[-2] and b"U" in host[-1]
    h2 = _both(host[-2:], keys, k)
    assert h2.sum() > 0
    for run in P.EMPTY_RUNS:
        er = P.empty_run_records(k, run)
        lay = P.layout_bytes(er)
        seps = lay == P.SEP
        assert seps[4087:4088 + run].all() and not seps[4086] and not seps[4088 + run]
        assert max(len(list(g)) for g in _runs(er)) == run >= 16
        if run > 4096:
            assert seps[4096:8192].all()  # a tile of nothing but separators
        he = _both(er, keys, k)
        assert he[0] > 0 and he[2 + run:].sum() > 0  # hits before and after the run
        assert he[0] < len(er[0]) - k + 1  # and misses


def _runs(recs):
    out, cur = [], []
    for r in recs:
        if r == b"":
            cur.append(r)
        elif cur:
            out.append(cur)
            cur = []
    if cur:
        out.append(cur)
    return out


@pytest.mark.parametrize("k", P.CUT_KS)
def test_cut_cases(k):
    sizes = P.QUERY_TAIL_SIZES(k)
    for n in (1, max(1, k - 1), k, k + 1, 15, 16, 17, 47, 48, 49, 4095, 4096, 4097,
              4096 + k - 2, 4096 + k - 1, 4096 + k, 2 * 4096 + 5):
        assert n in sizes
    assert sizes == sorted(set(sizes)) and sizes[-1] == P.QUERY_BYTES
    keys = P.cut_set(k)
    assert set(P.genome_set(k).tolist()) <= set(keys.tolist())
    changed = 0
    some_hits = some_misses = False
    for n in sizes:
        b = P.cut_batch(k, n)
        assert len(b) == n and np.array_equal(b, P.cut_batch(k, n))
        tail = b[-min(n, max(k - 1, 1)):]
        assert set(tail.tolist()) <= set(b"ACGT")  # ends in k - 1 valid bases, no separator
        recs = P.records_of(b)
        assert len(recs) == int((b == P.SEP).sum()) + 1
        alone = _both(recs, keys, k)
        joined = _both(P.records_of(np.concatenate([b, P.POISON])), keys, k)
        assert len(joined) == len(alone) and np.array_equal(joined[:-1], alone[:-1])
        if k > 1:
            # every window that starts in the tail and ends in POISON is a member
            assert joined[-1] >= alone[-1] + min(n, k - 1), (k, n)
        changed += int(joined[-1] != alone[-1])
        some_hits |= alone.sum() > 0
        some_misses |= alone.sum() < _valid_windows(recs, k)
    assert changed == len(sizes)  # POISON, read as the batch's continuation, changes every size's hits
    assert some_hits and some_misses
    assert set(P.CUT_OFFSET_KS) <= set(P.CUT_KS)


def test_short_records_case():
    k = P.SHORT_K
    recs = P.records_of(P.query_batch(k))
    hits = _both(recs, P.genome_set(k), k)
    n = len(recs) - P.SHORT_DROP
    assert n > 0 and hits[n] > 0 and hits[n:].sum() > hits[n]  # what a missing guard would write


def test_every_k_lists():
    assert P.EVERY_K == tuple(range(1, 33))
    assert P.CUT_KS == (1, 13, 16, 21, 25, 27, 31, 32)
    assert P.CUT_OFFSET_KS == (31, 25)
    assert len(P.POISON) == 96 and set(P.POISON.tolist()) <= set(b"ACGT")
    assert {ord("A"), ord("T")} & set(P.POISON.tolist())


# ---------------------------------------------------------------------------
# classify
# ---------------------------------------------------------------------------

def _classify_loop(refs, ik, ic, min_freq):
    """classify.rs:195-308 with dicts, sets and loops (as oracle/restate.py's
    run_classify_bytes does on files)."""
    filt = {}
    for i, key in enumerate(ik.tolist()):
        c = 1 if ic is None else int(ic[i])
        if c >= min_freq:
            filt[key] = c
    rm, rs, overall, union = [], [], set(), set()
    for r in refs:
        rset = set(r.tolist())
        assert len(rset) == len(r)  # a HashSet: no key twice
        matched = {key for key in rset if key in filt}
        rm.append(len(matched))
        rs.append(sum(filt[key] for key in matched))
        overall |= matched
        union |= rset
    return {"n_input": len(filt), "ref_matched": rm, "ref_sum_depth": rs, "union": len(union),
            "matched": len(overall), "sum_depth": sum(filt[key] for key in overall)}


def test_classify_input():
    ik, ic = P.classify_input()
    assert len(ik) == len(set(ik.tolist())) == P.N_INPUT and int(ik.max()) < 4 ** P.CLASSIFY_K
    vals = set(ic.tolist())
    assert {P.MIN_FREQ - 1, P.MIN_FREQ, P.MIN_FREQ + 1} <= vals
    assert sum(1 for c in vals if abs(c - (1 << 40)) < 1000) >= 4
    assert max(vals) < P.ABOVE_ALL and min(vals) >= 1
    assert 0 < (ic >= P.MIN_FREQ).sum() < len(ic)
    cin, cfo = P.common_keys()
    assert int(ic[ik == cin][0]) >= 1 << 40 and cfo not in ik


@pytest.mark.parametrize("name", sorted(P.LAYOUTS))
@pytest.mark.parametrize("min_freq", [1, P.MIN_FREQ, P.ABOVE_ALL])
def test_classify_expected_two_ways(name, min_freq):
    ik, ic = P.classify_input()
    refs = P.layout_refs(name)
    assert [len(r) for r in refs] == P.LAYOUTS[name]
    want = _classify_loop(refs, ik, ic, min_freq)
    assert P.classify_expected(refs, ik, ic, min_freq) == want
    assert P.classify_expected(refs, ik, None, 1) == _classify_loop(refs, ik, None, 1)
    if min_freq == P.ABOVE_ALL:
        assert want["n_input"] == want["matched"] == 0 and not any(want["ref_matched"])
    elif sum(P.LAYOUTS[name]):
        assert want["matched"] > 0 and want["sum_depth"] >= 1 << 40  # the common input key's count
    if sum(P.LAYOUTS[name]) > 100 and min_freq == P.MIN_FREQ:
        assert want["sum_depth"] > 1 << 32 and want["matched"] < want["union"]


def test_classify_reference_contents():
    ik, _ = P.classify_input()
    cin, cfo = P.common_keys()
    inset = set(ik.tolist())
    for name in P.LAYOUTS:
        refs = P.layout_refs(name)
        with_empty = 0
        for r in refs:
            if len(r) == 0:
                continue
            assert cin in r and (cfo in r) == (len(r) >= 3)
            n_in = sum(1 for key in r.tolist() if key in inset)
            assert abs(n_in - len(r) / 2) <= 2, (name, len(r), n_in)  # about half
            with_empty += int(P.EMPTY in r)
        assert with_empty == (1 if max(P.LAYOUTS[name]) >= 2 else 0), name


def _offsets(name):
    return np.concatenate([[0], np.cumsum(P.LAYOUTS[name])]).astype(np.int64)


def _refs_in(offs, lo, hi):
    """Non-empty references with a key in [lo, hi)."""
    return [r for r in range(len(offs) - 1) if offs[r] < offs[r + 1] and offs[r] < hi and offs[r + 1] > lo]


def test_classify_layout_properties():
    long = P.LAYOUTS["long"]
    assert long == [0, 0, 3, 0, 5, 1, 1, 0, 2, 2040, 0, 2048, 1, 4095, 0, 0]
    assert long[0] == 0 and long[-1] == 0
    assert P.LAYOUTS["one_key"] == [1] and P.LAYOUTS["one_block"] == [2048] and P.LAYOUTS["block_plus_one"] == [2049]
    short = P.LAYOUTS["short_run"]
    assert len(short) == 40 and set(short) == {0, 1, 2, 3}
    assert not any(P.LAYOUTS["all_empty"]) and len(P.LAYOUTS["all_empty"]) > 1

    def threads_spanning(name, n):
        offs = _offsets(name)
        return [t for t in range(-(-int(offs[-1]) // P.C_PER))
                if len(_refs_in(offs, P.C_PER * t, P.C_PER * (t + 1))) >= n]

    def one_ref_blocks(name):
        offs = _offsets(name)
        nk = int(offs[-1])
        return [b for b in range(-(-nk // P.C_BLOCK))
                if len(_refs_in(offs, P.C_BLOCK * b, min(P.C_BLOCK * (b + 1), nk))) == 1]

    assert threads_spanning("long", 4) and threads_spanning("short_run", 3)
    assert one_ref_blocks("long") == [3, 4] and one_ref_blocks("one_block") == [0]
    assert one_ref_blocks("block_plus_one") == [0, 1] and one_ref_blocks("block_aligned") == [0, 1]
    # runs of empty references between keys of one thread
    offs = _offsets("short_run")
    assert any(short[i] == short[i + 1] == 0 for i in range(39))
    # reference ends at multiples of 8 / of 2048, with more keys after them
    ends = {n: set(_offsets(n)[1:].tolist()) for n in P.LAYOUTS}
    assert 8 in ends["long"] and 2048 in ends["one_block"]
    assert {2048, 4096, 4104, 4112} <= ends["block_aligned"] and int(_offsets("block_aligned")[-1]) == 4117
    assert offs[-1] > 8 * 3


def test_map_wrap_case():
    ik, ic, refs = P.map_wrap_case()
    assert len(ik) <= 512 and 2 * len(ik) <= P.MIN_CAP  # the map has 1024 slots
    assert len(set(ik.tolist())) == len(ik) and (ic >= 1).all()
    present, absent = P.wrap_keys(P.MIN_CAP, P.CLASSIFY_K, 30, 30)
    assert set(present.tolist()) <= set(ik.tolist()) and not set(absent.tolist()) & set(ik.tolist())
    allref = set(np.concatenate(refs).tolist())
    assert set(present.tolist()) <= allref and set(absent.tolist()) <= allref
    assert (P.home(np.concatenate([present, absent]), P.MIN_CAP) >= P.MIN_CAP - 2).all()
    want = _classify_loop(refs, ik, ic, 1)
    assert P.classify_expected(refs, ik, ic, 1) == want
    assert 0 < want["matched"] < want["union"] and want["n_input"] == len(ik)
