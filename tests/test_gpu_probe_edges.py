"""The probe kernels of okm_probe.hip (hash set / map, query, classify) and
k_intersect_count at the edges the MB-scale random inputs of
tests/test_gpu_query_classify.py almost never reach (inputs:
tests/probe_cases.py, self-checked on the CPU by tests/test_probe_cases.py):

  1. linear probes that cross the table's last slot, in the set (insert,
     contains, the query kernel's set_probe_rest) and in the classify map
     (the build's CAS loop, map_get), with absent keys that are a miss only
     after the wrapped cluster;
  2. the ~0 side flag through two rehashes, and ~0 in a classify database;
  3. the grid-stride loops past their grid caps: contains with 2^24 + 300
     probes, a rehash of a 2^25-slot table, an intersection of 2^21 + 5 keys;
  4. classify's reference walk: empty references first / last / in runs,
     several references inside one thread's 8 keys, references that end at
     thread and block boundaries, one-reference blocks, ref_offsets[0] != 0,
     keys shared by every reference, the count filter at its threshold,
     depth sums past 2^32, an empty and a set-mode input;
  5. query at every k in 1..32 through both entry points, unterminated batches
     of every size around the 16-byte granule, the 48-byte thread load and the
     4096-byte tile with valid bases behind them, runs of empty records, a
     whole tile of separators, and fewer records asked for than present.

Integer work: every comparison is exact."""

import numpy as np
import pytest

import okm
import oracle
import probe_cases as P

pytestmark = pytest.mark.gpu

SLACK = 16  # an unaligned batch starts up to 15 bytes into the buffer
EMPTY1 = np.array([P.EMPTY], np.uint64)


# ---------------------------------------------------------------------------
# set: wraparound, flag, growth
# ---------------------------------------------------------------------------

def _revcomp(b: bytes) -> bytes:
    return b[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


@pytest.mark.parametrize("k", P.WRAP_KS)
def test_set_wraparound_flag_and_growth(k):
    c = P.set_case(k)
    present, absent, fill = c["present"], c["absent"], c["fill"]
    with okm.KmerSet(k, 0, capacity_hint=200) as s:  # 1024 slots
        assert s.insert(c["first"]) == c["n_first"] == len(s)
        members = np.concatenate([present, fill])
        assert s.contains(members).all()
        assert not s.contains(c["non_members"]).any()
        assert s.insert(c["first"]) == 0 and len(s) == c["n_first"]
        assert s.contains(members).all() and not s.contains(absent).any()

        # k_query_hits' first-slot load and set_probe_rest across the wrap: one
        # read per wrap key, either strand, and all of them joined into one
        seqs = [okm.u64_to_seq(int(v), k) for v in np.concatenate([present, absent])]
        reads = seqs + [_revcomp(q) for q in seqs] + [b"".join(seqs), _revcomp(b"".join(seqs))]
        want = oracle.query_hits(reads, np.sort(members), k)
        assert want[:len(present)].all() and not want[len(present):len(seqs)].any()
        assert np.array_equal(s.query_hits(reads), want)

        # the flag, then two growths: both rehashes carry it
        assert not s.contains(EMPTY1)[0]
        assert s.insert(np.concatenate([EMPTY1, EMPTY1])) == 1 and len(s) == c["n_first"] + 1
        assert s.insert(c["grow1"]) == c["n_grow1"]
        assert s.contains(EMPTY1)[0] and len(s) == c["n_first"] + 1 + c["n_grow1"]
        assert s.insert(c["grow2"]) == c["n_grow2"]
        assert len(s) == len(c["all_members"]) + 1
        assert s.contains(EMPTY1)[0] and s.insert(EMPTY1) == 0
        assert s.contains(c["all_members"]).all()
        assert not s.contains(c["non_members"]).any()
        assert np.array_equal(s.query_hits(reads), oracle.query_hits(reads, np.sort(c["all_members"]), k))


def test_set_flag_absent_survives_growth():
    """A table that never held ~0 does not gain it in a rehash."""
    c = P.set_case(31)
    with okm.KmerSet(31, 0, capacity_hint=10) as s:
        s.insert(c["first"])
        s.insert(c["grow1"])
        s.insert(c["grow2"])
        assert not s.contains(EMPTY1)[0] and len(s) == len(c["all_members"])


# ---------------------------------------------------------------------------
# set: grid-stride paths (the smallest sizes that reach them)
# ---------------------------------------------------------------------------

def test_contains_past_the_grid_cap():
    # grid_for caps the grid at 2^24 threads: 2^24 + 300 probes make 300 threads
    # take a second step (134 MB of probes; nothing smaller gets there)
    keys, member = P.contains_probes()
    assert len(keys) == (1 << 24) + 300
    with okm.KmerSet(31, 0, capacity_hint=P.CONTAINS_SET) as s:
        assert s.insert(P.distinct_keys(P.CONTAINS_SET)) == P.CONTAINS_SET
        got = s.contains(keys)
    assert np.array_equal(got, member)


def test_rehash_past_the_grid_cap():
    # k_set_rehash over a 2^25-slot table with the grid capped at 2^24 threads:
    # every thread loops, the flag word is thread 0's third step.  2^25 slots is
    # the smallest table whose rehash loops in every thread; under 1 GB on the device
    first = P.distinct_keys(P.REHASH_FIRST)
    second = P.distinct_keys(P.REHASH_SECOND, start=P.REHASH_FIRST)
    others = P.distinct_keys(100_000, start=P.REHASH_FIRST + P.REHASH_SECOND)
    with okm.KmerSet(31, 0, capacity_hint=P.REHASH_HINT) as s:
        assert s.insert(np.concatenate([first, EMPTY1])) == P.REHASH_FIRST + 1
        assert s.insert(second) == P.REHASH_SECOND == 1 << 24
        assert len(s) == P.REHASH_FIRST + 1 + P.REHASH_SECOND
        assert s.contains(first).all() and s.contains(EMPTY1)[0]
        sample = second[np.random.default_rng(4).integers(0, len(second), 100_000)]
        assert s.contains(sample).all()
        assert s.contains(second[-300:]).all() and s.contains(second[:300]).all()
        assert not s.contains(others).any()


def _dev(a):
    a = np.ascontiguousarray(a, np.uint64)
    buf = okm.DeviceBuffer(max(8, a.nbytes))
    if a.nbytes:
        buf.upload(a)
    return buf


def test_intersection_past_the_grid_cap_and_edges():
    # k_intersect_count caps its grid at 2^21 threads and probes the smaller
    # array: with 2^21 + 5 keys on that side five threads take a second step
    a, b, want = P.intersect_case()
    assert len(a) == (1 << 21) + 5 < len(b)
    da, db = _dev(a), _dev(b)
    try:
        def isect(oa, na, ob, nb):
            return okm.set_intersection_size_device(da.address + 8 * oa, na, db.address + 8 * ob, nb)

        assert isect(0, len(a), 0, len(b)) == want
        assert okm.set_intersection_size_device(db.address, len(b), da.address, len(a)) == want  # swapped
        assert okm.set_intersection_size_device(da.address, len(a), da.address, len(a)) == len(a)  # identical
        # a = {3 i}, b[0] = 0 = a[0], b[1] = 1, b[2] = 2 (i = 0: all three kinds)
        assert b[:3].tolist() == [0, 1, 2]
        assert isect(0, 1, 0, len(b)) == 1 and isect(1, 1, 0, len(b)) == 0      # na = 1: a hit, a miss
        assert isect(0, len(a), 0, 1) == 1 and isect(0, len(a), 1, 1) == 0      # nb = 1
        assert isect(0, 1, 0, 1) == 1 and isect(1, 1, 1, 1) == 0
        # every a below b[0]: a[:100] < b[1000]; every a above b[-1]: a[-100:] > b[:1000]
        assert a[99] < b[1000] and a[-100] > b[999]
        assert isect(0, 100, 1000, len(b) - 1000) == 0
        assert isect(len(a) - 100, 100, 0, 1000) == 0
        assert isect(0, 1000, 0, 400) == int(np.isin(a[:1000], b[:400]).sum()) > 0
    finally:
        da.free()
        db.free()


# ---------------------------------------------------------------------------
# query: every k, tails, empty records
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def qbuf():
    buf = okm.DeviceBuffer(2 * P.Q_TILE + 5000 + len(P.POISON) + SLACK)
    hits = okm.DeviceBuffer(4 * 8192)
    yield buf, hits
    buf.free()
    hits.free()


GUARD = 0xDEADBEEF


def _query_device(s, qbuf, content, offset, n_bytes, n_records):
    """Per-record hits of the n_bytes at `offset` into the uploaded content;
    the word behind the last record's must stay as it was."""
    buf, hb = qbuf
    buf.upload(content)
    hb.upload(np.full(n_records + 1, GUARD, np.uint32))
    s.query_hits_device(buf.address + offset, n_bytes, n_records, hb.address)
    got = np.zeros(n_records + 1, np.uint32)
    hb.download(got)
    assert got[n_records] == GUARD
    return got[:n_records]


@pytest.mark.parametrize("k", P.EVERY_K)
def test_query_every_k_host_and_device(qbuf, k):
    keys = P.genome_set(k)
    batch = P.query_batch(k)
    recs = P.records_of(batch)
    host = P.host_records(k)
    want = oracle.query_hits(host, keys, k)
    assert 0 < want.sum()
    with okm.KmerSet(k, 0, len(keys)) as s:
        assert s.insert(keys) == len(keys)
        got_host = s.query_hits(host)
        assert np.array_equal(got_host, want), ("host", k)
        got_dev = _query_device(s, qbuf, batch, 0, len(batch), len(recs))
        assert np.array_equal(got_dev, want[:len(recs)]), ("device", k)
        assert np.array_equal(got_dev, got_host[:len(recs)])
        for run in P.EMPTY_RUNS:
            er = list(P.empty_run_records(k, run))
            want_e = oracle.query_hits(er, keys, k)
            assert np.array_equal(s.query_hits(er), want_e), ("host", k, run)
            lay = P.layout_bytes(er)
            assert np.array_equal(_query_device(s, qbuf, lay, 0, len(lay), len(er)), want_e), ("device", k, run)


@pytest.mark.parametrize("k", P.CUT_KS)
def test_query_unterminated_tail_before_valid_bytes(qbuf, k):
    keys = P.cut_set(k)
    with okm.KmerSet(k, 0, len(keys)) as s:
        s.insert(keys)
        for n in P.QUERY_TAIL_SIZES(k):
            b = P.cut_batch(k, n)
            recs = P.records_of(b)
            want = oracle.query_hits(recs, keys, k)
            got = _query_device(s, qbuf, P.with_poison(b), 0, n, len(recs))
            assert np.array_equal(got, want), ("tail", k, n)
            if k in P.CUT_OFFSET_KS:
                # a pointer off 16-byte alignment is copied to the set's staging
                # buffer first.  The batch WITH the poison goes through it once
                # (hits not compared), so that what lies behind the next, shorter
                # copy there is the poison too, not whatever an allocation holds
                both = P.records_of(np.concatenate([b, P.POISON]))
                _query_device(s, qbuf, P.with_poison(b, 3), 3, n + len(P.POISON), len(both))
                got = _query_device(s, qbuf, P.with_poison(b, 3), 3, n, len(recs))
                assert np.array_equal(got, want), ("tail+3", k, n)


def test_query_fewer_records_than_present(qbuf):
    k = P.SHORT_K
    keys = P.genome_set(k)
    batch = P.query_batch(k)
    recs = P.records_of(batch)
    want = oracle.query_hits(recs, keys, k)
    with okm.KmerSet(k, 0, len(keys)) as s:
        s.insert(keys)
        early = int(np.flatnonzero(want)[0])  # the first record with hits: behind the short special lengths
        assert early >= 1
        for n_records in (len(recs) - P.SHORT_DROP, early):
            assert want[n_records] > 0  # the first record left out has hits
            got = _query_device(s, qbuf, batch, 0, len(batch), n_records)  # checks the guard word
            assert np.array_equal(got, want[:n_records]), n_records
        # separators only, and more of them than records asked for
        seps = np.full(P.Q_TILE + 17, P.SEP, np.uint8)
        assert not _query_device(s, qbuf, seps, 0, len(seps), 5).any()


# ---------------------------------------------------------------------------
# classify
# ---------------------------------------------------------------------------

FIELDS = ("ref_matched", "ref_sum_depth", "union", "matched", "sum_depth")


def _plain(res):
    return {f: ([int(x) for x in res[f]] if isinstance(res[f], np.ndarray) else int(res[f])) for f in FIELDS}


def _probe_both(cl, refs, junk_before=0, junk_after=0, junk=None):
    """One database through okm_classifier_probe_db and _probe_db_device;
    with junk keys around it, ref_offsets[0] = junk_before."""
    keys, offs = okm.Classifier.pack_db(list(refs))
    if junk_before or junk_after:
        keys = np.concatenate([junk[:junk_before], keys, junk[len(junk) - junk_after:]])
        offs = offs + np.uint64(junk_before)
    host = _plain(cl.probe_db(packed=(keys, offs)))
    dk = _dev(keys)
    try:
        dev = _plain(cl.probe_db(packed=(None, offs), d_keys=dk.address))
    finally:
        dk.free()
    assert host == dev
    return host


def _want(refs, ik, ic, min_freq):
    w = P.classify_expected(refs, ik, ic, min_freq)
    return w.pop("n_input"), w


@pytest.fixture(scope="module")
def input_counter():
    ik, ic = P.classify_input()
    c = okm.KmerCounter(P.CLASSIFY_K, "count")
    half = len(ik) // 2
    c.add_pairs(ik[:half], ic[:half])
    c.add_pairs(ik[half:], ic[half:])
    gk, gc = c.result(1)
    assert np.array_equal(gk, ik) and np.array_equal(gc, ic)  # the table the classifier reads
    yield c
    c.close()


@pytest.mark.parametrize("min_freq", [1, P.MIN_FREQ, P.ABOVE_ALL])
def test_classify_layouts_and_count_filter(input_counter, min_freq):
    ik, ic = P.classify_input()
    with okm.Classifier(input_counter, min_freq) as cl:
        assert cl.n_input == int((ic >= min_freq).sum())
        for name in sorted(P.LAYOUTS):
            refs = P.layout_refs(name)
            n_in, want = _want(refs, ik, ic, min_freq)
            assert cl.n_input == n_in
            assert _probe_both(cl, refs) == want, (name, min_freq)
            if min_freq == P.ABOVE_ALL:  # an empty map: no match, the union still exact
                assert want["matched"] == 0 and want["union"] == len(np.unique(np.concatenate(refs)))
        # ref_offsets[0] != 0: input keys in front of and behind the database
        junk = ik[ic >= min_freq][:40] if n_in else ik[:40]
        for name in ("long", "short_run", "one_block"):
            refs = P.layout_refs(name)
            want = _want(refs, ik, ic, min_freq)[1]
            assert _probe_both(cl, refs, 5, 3, junk) == want, (name, "offset 5")
            assert _probe_both(cl, refs, 2048, 0, np.resize(junk, 2048)) == want, (name, "offset 2048")
        assert cl.probe_db([])["union"] == 0


def test_classify_depth_sums_past_32_bits(input_counter):
    ik, ic = P.classify_input()
    refs = P.layout_refs("long")
    with okm.Classifier(input_counter, 1) as cl:
        got = _probe_both(cl, refs)
    want = _want(refs, ik, ic, 1)[1]
    assert got == want
    assert want["sum_depth"] > 1 << 40 and max(want["ref_sum_depth"]) > 1 << 40
    # the 2^40 key is in every non-empty reference, once in the union
    assert sum(d >= 1 << 40 for d in want["ref_sum_depth"]) == sum(1 for r in refs if len(r))
    assert want["sum_depth"] < 6 << 40


def test_classify_empty_and_set_mode_input():
    ik, _ = P.classify_input()
    refs = P.layout_refs("long")
    with okm.KmerCounter(P.CLASSIFY_K, "count") as c:  # no batch at all
        with okm.Classifier(c, 1) as cl:
            assert cl.n_input == 0
            assert _probe_both(cl, refs) == _want(refs, ik[:0], None, 1)[1]
    with okm.KmerCounter(P.CLASSIFY_K, "set") as c:  # no counts: every depth is 1
        c.add_pairs(ik)
        with okm.Classifier(c, 1) as cl:
            assert cl.n_input == len(ik)
            for name in ("long", "short_run", "block_aligned"):
                refs = P.layout_refs(name)
                got = _probe_both(cl, refs)
                assert got == _want(refs, ik, None, 1)[1], name
                assert got["ref_sum_depth"] == got["ref_matched"] and got["sum_depth"] == got["matched"] > 0
        with okm.Classifier(c, 2) as cl:  # depth 1 < 2: nothing passes the filter
            assert cl.n_input == 0
            assert _probe_both(cl, refs) == _want(refs, ik, None, 2)[1]


def test_classify_map_wraparound():
    ik, ic, refs = P.map_wrap_case()
    assert len(ik) <= 512  # a 1024-slot map
    with okm.KmerCounter(P.CLASSIFY_K, "count") as c:
        c.add_pairs(ik, ic)
        for min_freq in (1, 3):
            with okm.Classifier(c, min_freq) as cl:
                n_in, want = _want(refs, ik, ic, min_freq)
                assert cl.n_input == n_in
                assert _probe_both(cl, refs) == want, min_freq
