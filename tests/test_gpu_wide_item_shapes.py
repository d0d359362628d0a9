"""Item, partition and look-back shapes of the wide (k in 33..64, two-u64
key) count, exact against Python integers.

Every wide item goes through k_count_slow<K128, ...> (okm_count.hip): full
mode with 4096 homes and a rank-inside-home sort, dense mode on 16-byte slots,
and -- by default -- the direct variant that writes the table itself at a
decoupled look-back prefix.  The inputs (tests/wide_cases.py, self-checked on
the CPU by tests/test_wide_cases.py) put each shape where it can go wrong: row
and capacity edges, one home or one key holding the whole item, the first and
last homes, keys that differ in one word only, dense items, parts that take a
partition pass, item counts around the look-back window, the extreme keys --
at the k where the L1 bin, the partition bin and the home lie below, across
and above the boundary between the key's two words.

Two flavours of every input.  "pairs": the keys as they are through add_pairs,
which always makes a weighted run (a count of 1 per key when none is given),
so it runs the weighted kernels.  "records": one k-base read per key through
add_records, which runs the unweighted kernels -- the ones a count from reads
uses -- on the keys' canonical forms.

Four ways the wide count is launched, each proved by the run's own report:
  direct   one group beside an instance-bound table (the default):
           "compact_items" not in the kernel stats, info["groups"] == 0
  staged   staged runs plus compaction (knobs group_exact = 1, group_keys
           above the total): "compact_items" in the stats
  groups   pipelined key-range groups with the device-side table base (knob
           group_keys small, with and without group_over): info["groups"] >= 3
           and no "compact_items"
  fan      part_max_bits = 2, so a pass leaves oversized children that the
           fan-out splits in place, most slots empty: "fan_split" in the stats
"""

from functools import lru_cache

import numpy as np
import pytest

import okm
import wide_cases as wc
from okm import testing
from oracle import OracleCounterWide

pytestmark = pytest.mark.gpu

_KS = [pytest.param(k, id=f"k{k}") for k in wc.KS]
_KS_SOME = [pytest.param(k, id=f"k{k}") for k in wc.KS_SOME]
_KS_TWINS = [pytest.param(k, id=f"k{k}") for k in wc.KS_TWINS]
FLAVOURS = ("pairs", "records")

_counters = {}


@pytest.fixture(scope="module", autouse=True)
def _close_counters():
    yield
    for c in _counters.values():
        c.close()
    _counters.clear()


def _counter(k):
    """One context per k for the whole module (reset between cases)."""
    if k not in _counters:
        _counters[k] = okm.KmerCounter(k, wide=True)
    c = _counters[k]
    c.reset()
    c.set_timing(True)  # (also clears the kernel stats)
    return c


PATH_KNOBS = {
    "direct": {},
    "staged": {"group_exact": 1, "group_keys": 1 << 40},
    "fan": {"part_max_bits": 2},
    "sorted": {},  # sorted runs (add_sorted_pairs_device): no knob, no launch way to prove
    # "groups" / "groups_over": group_keys comes from the case
}


def _knobs(path, group_keys=None):
    if path in ("groups", "groups_over"):
        kn = {"group_keys": group_keys, "group_exact": 0}
        if path == "groups_over":
            kn["group_over"] = 1
        return kn
    return PATH_KNOBS[path]


def _check_path(path, stats, info, min_groups=3):
    if path == "direct":
        assert "compact_items" not in stats and info["groups"] == 0, (sorted(stats), info)
    elif path == "staged":
        assert "compact_items" in stats, sorted(stats)
    elif path in ("groups", "groups_over"):
        assert info["groups"] >= min_groups and "compact_items" not in stats, (sorted(stats), info)
    elif path == "fan":
        assert "fan_split" in stats and "compact_items" not in stats, sorted(stats)


def _ascending(pairs):
    lo, hi = pairs[:, 0], pairs[:, 1]
    return bool(np.all((hi[1:] > hi[:-1]) | ((hi[1:] == hi[:-1]) & (lo[1:] > lo[:-1]))))


def _count(k, feed, expect, path="direct", group_keys=None, min_groups=3, label=""):
    """Count what feed(counter) adds, under the path's knobs, and compare the
    table -- exactly -- with expect = (pairs of the sorted keys, u64 counts,
    instance or weight total)."""
    ek, ec, total = expect
    with testing.knobs(**_knobs(path, group_keys)):
        c = _counter(k)
        feed(c)
        gk, gc = c.result(1)
        # (a reused context keeps the names of kernels it ran before, at 0 launches)
        stats = {name: st for name, st in c.kernel_stats().items() if st["launches"] > 0}
        info = c.engine_info()
    gk = gk.reshape(-1, 2)
    where = f"{label} k={k} {path}"
    assert gk.shape == ek.shape, (where, gk.shape, ek.shape)
    if not np.array_equal(gk, ek):
        bad = np.flatnonzero((gk != ek).any(axis=1))
        raise AssertionError(f"{where}: {len(bad)} of {len(ek)} keys differ, first at {bad[0]}: "
                             f"got {wc.from_pairs(gk[bad[0]])[0]:#x}, expected {wc.from_pairs(ek[bad[0]])[0]:#x}")
    if not np.array_equal(gc, ec):
        bad = np.flatnonzero(gc != ec)
        raise AssertionError(f"{where}: {len(bad)} of {len(ec)} counts differ, first at {bad[0]}: "
                             f"got {gc[bad[0]]}, expected {ec[bad[0]]}")
    assert gc.dtype == np.uint64
    assert _ascending(gk), where
    assert sum(int(x) for x in gc) == total, where
    assert info["distinct"] == len(ec), (where, info)
    assert "count_items" in stats, (where, sorted(stats))
    _check_path(path, stats, info, min_groups)
    return stats, info


def _expect(ref_ints, weights=None):
    keys, counts = wc.reference(ref_ints, weights)
    total = sum(weights) if weights is not None else len(ref_ints)
    return wc.to_pairs(keys), np.array(counts, dtype=np.uint64), total


# builders that take for_records: the records flavour gets keys that are their
# own canonical forms, so both flavours have the instance counts they aim at
_FOR_RECORDS = {"one_item_repeats", "one_item_distinct", "one_key_fills_item", "one_home", "last_and_first_home",
                "split_part", "m_items"}


@lru_cache(maxsize=40)
def _case(builder, k, flavour, args):
    """(feed, expectation) of builder(k, 0, *args) in one flavour: built once,
    shared by the paths.  A builder may return (ints, extra...)."""
    kw = {"for_records": True} if flavour == "records" and builder in _FOR_RECORDS else {}
    out = getattr(wc, builder)(k, 0, *args, **kw)
    ints = out if isinstance(out, list) else out[0]
    if flavour == "pairs":
        pairs = wc.to_pairs(ints)
        return (lambda c: c.add_pairs(pairs)), _expect(ints)
    recs = wc.records(ints, k)
    canon = wc.canonical(ints, k)
    if kw:
        assert canon == ints
    return (lambda c: c.add_records(recs, normalized=True)), _expect(canon)


def _run_case(builder, k, args, flavour, path, **kw):
    feed, expect = _case(builder, k, flavour, args)
    return _count(k, feed, expect, path, label=f"{builder}{args} {flavour}", **kw)


def _run_weighted(k, ints, weights, path, label):
    pairs, w = wc.to_pairs(ints), np.array(weights, dtype=np.uint64)
    return _count(k, lambda c: c.add_pairs(pairs, w), _expect(ints, weights), path, label=label)


# ---------------------------------------------------------------------------
# shapes 1-6, 9, 10: one item (or a part that splits down to one)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("path", ["direct", "staged"])
@pytest.mark.parametrize("k", _KS)
def test_one_item_rows(k, flavour, path):
    """1, 2, 511 .. 513, 4095 .. 4097 instances of one L1 bin, with repeats
    and all distinct; 4097 is one past an item: the part splits."""
    for n in wc.EDGES:
        _run_case("one_item_repeats", k, (n,), flavour, path)
        _run_case("one_item_distinct", k, (n,), flavour, path)


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("path", ["direct", "staged"])
@pytest.mark.parametrize("k", _KS_SOME)
def test_one_key_fills_the_item(k, flavour, path):
    for n in wc.FILL_NS:
        _, info = _run_case("one_key_fills_item", k, (n,), flavour, path)
        assert info["distinct"] == 1


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("path", ["direct", "staged"])
@pytest.mark.parametrize("k", _KS)
def test_one_home_holds_a_crowd(k, flavour, path):
    """2, 513 and 3000 distinct keys of one full-mode home (the longest rank
    loops) beside ordinary keys."""
    for n in wc.ONE_HOME_NS:
        _run_case("one_home", k, (n,), flavour, path)


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("path", ["direct", "staged"])
@pytest.mark.parametrize("k", _KS_SOME)
def test_first_and_last_homes(k, flavour, path):
    _run_case("last_and_first_home", k, (), flavour, path)


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("path", ["direct", "staged"])
@pytest.mark.parametrize("k", _KS_TWINS)
def test_keys_that_differ_in_one_word(k, flavour, path):
    _run_case("word_twins", k, (), flavour, path)


@pytest.mark.parametrize("path", ["direct", "staged"])
@pytest.mark.parametrize("k", _KS_SOME)
def test_dense_item(k, path):
    """9000 instances over 2^8 and 2^11 keys: the part splits (host rounds)
    down to a direct-address item.  Unweighted from records and from pairs,
    and weighted."""
    for low in wc.DENSE_LOW_BITS:
        for flavour in FLAVOURS:
            _, info = _run_case("dense_item", k, (low,), flavour, path)
            assert info["levels"] >= 1, info
        ints, w = wc.dense_item(k, 0, low, weighted=True)
        _run_weighted(k, ints, w, path, f"dense_item({low}) weighted")


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("path", ["direct", "staged"])
@pytest.mark.parametrize("k", _KS_SOME)
def test_extreme_keys(k, flavour, path):
    """Key 0, the largest key, lo or hi all-ones (one word away from the empty
    marker, which is both)."""
    _run_case("extremes", k, (), flavour, path)


@pytest.mark.parametrize("path", ["direct", "staged"])
@pytest.mark.parametrize("k", _KS_SOME)
def test_weighted_rows(k, path):
    """The row edges with weights in 1..1000; then with one key whose two
    weights sum past 2^32 and one whose lone weight is past it."""
    for n in wc.EDGES:
        for big in (False, True):
            ints, w = wc.weighted(k, 0, n, big)
            _run_weighted(k, ints, w, path, f"weighted({n}, big={big})")


# ---------------------------------------------------------------------------
# shape 7: one L1 part that takes a partition pass
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("path", ["direct", "staged", "fan"])
@pytest.mark.parametrize("k", _KS)
def test_split_part(k, flavour, path):
    """4097, 20 000 and 70 000 keys of one L1 bin, uniform and skewed (three
    tight clusters: uneven and empty partition bins).  Fan-out: a 2-bit pass
    leaves the 20 000- and 70 000-key parts' children oversized (a 4097-key
    part needs one bit and no fan-out)."""
    for n in wc.SPLIT_NS[1:] if path == "fan" else wc.SPLIT_NS:
        for skewed in (False, True):
            _, info = _run_case("split_part", k, (n, skewed), flavour, path)
            assert info["levels"] >= 1, info


@pytest.mark.parametrize("path,flavour", [("groups", "pairs"), ("groups", "records"), ("groups_over", "records")])
@pytest.mark.parametrize("k", _KS)
def test_split_part_between_groups(k, path, flavour):
    """Key-range groups are made of whole L1 parts, so the part that splits
    stands between small parts in L1 bins 0, 1, 510 and 511, every part a
    group of its own: five pipelined groups, the middle one with a pass."""
    for n in wc.SPLIT_NS:
        for skewed in (False, True):
            _, info = _run_case("split_part", k, (n, skewed, True), flavour, path, group_keys=1)
            assert info["groups"] == 5, info


# ---------------------------------------------------------------------------
# shape 8: m items (the look-back window is 64 items)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("path", ["direct", "staged"])
@pytest.mark.parametrize("k", _KS_SOME)
def test_m_items(k, flavour, path):
    """1 .. 512 items of ~50 instances: 63 .. 66 and 128 / 129 items put the
    nearest known prefix one look-back window away and just past it."""
    for m in wc.M_ITEMS:
        _, info = _run_case("m_items", k, (m,), flavour, path)
        assert info["work_items"] == m, info
    for m, n in wc.ALTERNATING:
        _, info = _run_case("m_items", k, (m, n), flavour, path)
        assert info["work_items"] == m, info


@pytest.mark.parametrize("path,flavour", [("groups", "pairs"), ("groups", "records"), ("groups_over", "records")])
@pytest.mark.parametrize("k", _KS_SOME)
def test_m_items_in_groups(k, path, flavour):
    """The items in pipelined groups of about a fifth of them each (m < 3: a
    group per item), spread over the key space and at its two ends only; the
    alternating layouts in groups of about four big items.  (The records
    flavour of m_items is built from keys that are their own canonical forms,
    so it populates the same m bins.)"""
    for m in wc.M_ITEMS[1:]:  # (one item cannot be grouped)
        for ends_only in (False, True):
            _run_case("m_items", k, (m, 0, ends_only), flavour, path,
                      group_keys=50 * max(1, m // 5), min_groups=min(m, 3))
    for m, n in wc.ALTERNATING:
        _run_case("m_items", k, (m, n), flavour, path, group_keys=4 * (n + 1))


@lru_cache(maxsize=8)
def _items_around_a_split_part(k, m):
    ints = wc.m_items(k, 0, m, for_records=True) + wc.split_part(k, 0, 20_000, for_records=True)
    pairs = wc.to_pairs(ints)
    recs = wc.records(ints, k)
    return ({"pairs": lambda c: c.add_pairs(pairs), "records": lambda c: c.add_records(recs, normalized=True)},
            {"pairs": _expect(ints), "records": _expect(wc.canonical(ints, k))})


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("k", _KS_SOME)
def test_m_items_around_a_fan_out(k, flavour):
    """No item of m_items splits, so the fan-out needs a part that does: a
    20 000-key part among the m items.  With 2-bit passes every part gets four
    children of four fan-out slots each: a few full items between many empty
    ones, which the look-back must cross."""
    for m in (wc.WINDOW - 1, wc.WINDOW + 1, 2 * wc.WINDOW + 1):
        feeds, expects = _items_around_a_split_part(k, m)
        _, info = _count(k, feeds[flavour], expects[flavour], "fan", label=f"m_items({m}) + split_part {flavour}")
        assert info["work_items"] > 4 * m, info


# ---------------------------------------------------------------------------
# from bytes, against the oracle too
# ---------------------------------------------------------------------------

def _bytes_cases():
    return [pytest.param(k, recs, id=name) for name, k, recs in wc.bytes_cases()]


@pytest.mark.parametrize("k,recs", _bytes_cases())
@pytest.mark.parametrize("path", ["direct", "staged"])
def test_records_end_to_end(k, recs, path):
    """T^32 A^32 (k = 64: hi = ~0, lo = 0); key 0 with 4096 and 4097 instances
    from one record; one read 512 and 513 times beside reads that occur once."""
    expect = _expect(wc.kmers_of_records(recs, k))
    oc = OracleCounterWide(k)
    oc.add_records(recs)
    ok, ocnt = oc.result(1)
    assert np.array_equal(ok, expect[0]) and np.array_equal(ocnt, expect[1])
    _count(k, lambda c: c.add_records(recs), expect, path, label="records")


# ---------------------------------------------------------------------------
# items that span sorted runs
# ---------------------------------------------------------------------------

def _upload(arr):
    arr = np.ascontiguousarray(arr, dtype=np.uint64)
    buf = okm.DeviceBuffer(max(arr.nbytes, 8))
    buf.upload(arr)
    return buf


@pytest.mark.parametrize("k", [pytest.param(k, id=f"k{k}") for k in wc.KS_RUNS])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nruns", [2, 4, 5, 65])
def test_items_spanning_sorted_runs_wide(nruns, weighted, k):
    """Strictly ascending runs spread over the whole key space: every
    key-range item holds a slice of each run."""
    rng = np.random.default_rng([nruns, k])
    bits = 2 * k - 1
    shared = wc.rand_bits(rng, 1500, bits)  # keys that every run holds
    runs, all_ints, all_w = [], [], []
    for _ in range(nruns):
        keys = sorted(set(wc.rand_bits(rng, 3000, bits) + shared))
        w = [int(x) for x in rng.integers(1, 1000, len(keys))] if weighted else [1] * len(keys)
        runs.append((wc.to_pairs(keys), np.array(w, dtype=np.uint64)))
        all_ints += keys
        all_w += w
    expect = _expect(all_ints, all_w)
    bufs = []

    def feed(c):
        for keys, counts in runs:
            bk = _upload(keys)
            bc = _upload(counts) if weighted else None
            bufs.extend([bk, bc])
            c.add_sorted_pairs_device(bk.address, bc.address if bc else None, len(counts))

    _count(k, feed, expect, "sorted", label=f"{nruns} runs")
    for b in bufs:
        if b:
            b.free()
