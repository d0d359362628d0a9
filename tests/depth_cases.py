"""Inputs and expectations of the read-depth tests (not a test file:
tests/test_depth_cases.py checks on the CPU that every case has the property
its name claims; tests/test_gpu_read_depths.py runs them).

The expectation is always plain Python, per record: normalise, enumerate the
windows, canonicalise each with the codec functions (okm.seq_to_u64 /
canonical_u64, the u128 pair above k = 32), look it up in a dict key -> count,
reduce.  Every number is an exact integer."""

from collections import Counter
from functools import lru_cache

import numpy as np

import okm

FIELDS = ("windows", "present", "solid", "sum", "min", "max")
M64 = (1 << 64) - 1

# the kernel's geometry
SEG = 16              # okm_depth.hip kDepthSeg: window starts per thread
TILE = 4096           # okm_depth.hip kDepthTile = kDepthBlock (256) * kDepthSeg: window starts per workgroup
WAVE = 64 * SEG       # the bytes of one wave: without a separator among them its rows leave as one
CHUNK = 32 << 20      # okm_engine.hip kDepthChunk: packed bytes per uploaded chunk of host records

KS = (1, 15, 31, 32, 33, 37, 63, 64)


# ---------------------------------------------------------------------------
# the expectation
# ---------------------------------------------------------------------------

def normalize(rec: bytes, normalized: bool = False) -> bytes:
    """What reaches the device: okm_add_batch's normalize(false) drops the
    white space; case and U stay for the device to read."""
    if normalized:
        return bytes(rec)
    return bytes(rec).translate(None, b" \t\r\n")


def window_keys(rec: bytes, k: int):
    """The canonical key (a Python int) of every valid window of a normalised
    record, in order: a window holds A/C/G/T only, either case, U as T."""
    s = rec.upper().replace(b"U", b"T")
    out = []
    bad = -1  # the last byte seen that is no base
    for i, ch in enumerate(s):
        if ch not in b"ACGT":
            bad = i
        j = i - k + 1
        if j < 0 or bad >= j:
            continue
        w = s[j:i + 1]
        if k <= 32:
            out.append(okm.canonical_u64(okm.seq_to_u64(w, k), k))
        else:
            out.append(okm.canonical_u128(okm.seq_to_u128(w, k), k))
    return out


def row_of(keys, table, min_count):
    cs = [table[v] for v in keys if v in table]
    return (len(keys), len(cs), sum(1 for c in cs if c >= min_count), sum(cs) & M64,
            min(cs) if cs else 0, max(cs) if cs else 0)


def expected(records, k, table, min_count=2, normalized=False):
    """One row per record against the dict `table` (canonical key -> count)."""
    out = np.zeros(len(records), dtype=okm.READ_DEPTH_DTYPE)
    for i, rec in enumerate(records):
        out[i] = row_of(window_keys(normalize(rec, normalized), k), table, min_count)
    return out


def combine(rows_list):
    """Rows over the same reads against tables of disjoint keys, combined by
    the rule include/orion_kmer.h states: present, solid and sum add, max is
    the larger, min the smaller non-zero one, windows is anybody's."""
    out = rows_list[0].copy()
    for rows in rows_list[1:]:
        assert np.array_equal(rows["windows"], out["windows"])
        for f in ("present", "solid", "sum"):
            out[f] = out[f] + rows[f]  # (uint64: wraps as the engine's sum does)
        out["max"] = np.maximum(out["max"], rows["max"])
        a, b = out["min"], rows["min"]
        out["min"] = np.where(a == 0, b, np.where(b == 0, a, np.minimum(a, b)))
    return out


def table_of_records(records, k, normalized=False):
    """The count table of records as a dict, by the same enumeration."""
    t = Counter()
    for rec in records:
        t.update(window_keys(normalize(rec, normalized), k))
    return dict(t)


def table_of_result(keys, counts, wide):
    """The dict of a KmerCounter.result()."""
    ints = okm.keys128_to_int(keys) if wide else [int(v) for v in keys]
    return dict(zip(ints, (int(c) for c in counts)))


def device_batch(records, terminate_last=True, normalized=False):
    """The device layout of the records: normalised, a separator after each
    (the last one's optional)."""
    b = b"".join(normalize(r, normalized) + b"\n" for r in records)
    return b if terminate_last or not records else b[:-1]


def render(ids, rows):
    """The --depth-output file."""
    return "".join(i + "\t" + "\t".join(str(int(r[f])) for f in FIELDS) + "\n" for i, r in zip(ids, rows))


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _bases(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


@lru_cache(maxsize=None)
def genome():
    return _bases(np.random.default_rng(101), 3000)


@lru_cache(maxsize=None)
def table_reads():
    """The reads the table is counted from: 45 reads of 200 bases of the
    genome (a coverage of 3: counts of 1, 2, 3 ... and stretches nobody read)
    and one stretch 12 more times."""
    rng = np.random.default_rng(103)
    g = genome()
    return tuple(g[o:o + 200] for o in rng.integers(0, len(g) - 200, 45)) + (g[500:700],) * 12


def _mixed(rng, n, k):
    """n bases: stretches of the genome (present in the table) and random
    stretches (absent for all but tiny k) in turn, starting with either."""
    g = genome()
    out, from_genome = b"", bool(rng.integers(0, 2))
    while len(out) < n:
        ln = int(rng.integers(k + 3, 3 * k + 40))
        if from_genome:
            o = int(rng.integers(0, len(g) - ln))
            out += g[o:o + ln]
        else:
            out += _bases(rng, ln)
        from_genome = not from_genome
    return out[:n]


@lru_cache(maxsize=None)
def geometry(k):
    """(records, names): the records of the geometry case at k in batch order.
    names[i] says what record i is there for; `sep_at` of test_depth_cases.py
    checks the positions.  Every record is as the host form takes it with
    normalized = 0 (one holds white space, lower case and U); the last one is
    left without a separator in the device form."""
    rng = np.random.default_rng(1000 + k)
    recs, names = [], []
    pos = [0]  # the batch offset of the next record's first byte

    def add(rec, name):
        recs.append(rec)
        names.append(name)
        pos[0] += len(normalize(rec)) + 1

    def until(sep):
        """A record whose separator lands at batch offset sep."""
        n = sep - pos[0]
        assert n >= 0
        return _mixed(rng, n, k)

    for n, name in ((0, "empty"), (k - 1, "k-1"), (k, "k"), (k + 1, "k+1")):
        add(_mixed(rng, n, k), name)
    for _ in range(70):
        add(b"", "empty run")
    body = max(3 * k + 5, 12)
    for at, name in ((0, "N first"), (body // 2, "N middle"), (body - 1, "N last")):
        r = bytearray(_mixed(rng, body, k))
        r[at] = ord("N")
        add(bytes(r), name)
    r = _mixed(rng, 2 * body, k).lower().replace(b"t", b"u", 3)
    add(r[:body] + b" \r\n\t" + r[body:].upper().replace(b"T", b"U", 2), "lower case, U and white space")
    # ends at a thread's run: the separator is the last byte of a run, the first of the next, the second
    base = (pos[0] // SEG + 8) * SEG
    for d, name in ((-1, "run end - 1"), (0, "run end"), (1, "run end + 1")):
        add(until(base + d), name)
        base += 6 * SEG
    # ... and at a workgroup's tile
    tile = (pos[0] // TILE + 1) * TILE
    for d, name in ((-1, "tile end - 1"), (0, "tile end"), (1, "tile end + 1")):
        add(until(tile + d), name)
        tile += TILE
    add(_mixed(rng, 3 * TILE + 2 * WAVE + 77, k), "long")  # its row is completed by four or five workgroups
    add(_mixed(rng, 2 * body + 3, k), "unterminated")
    return tuple(recs), tuple(names)


def sep_positions(records):
    """Batch offset of every record's separator."""
    out, p = [], 0
    for r in records:
        p += len(normalize(r))
        out.append(p)
        p += 1
    return out


@lru_cache(maxsize=None)
def geometry_expected(k, min_count=2):
    """(table dict, rows) of the geometry case against table_reads()."""
    table = table_of_records(table_reads(), k)
    return table, expected(geometry(k)[0], k, table, min_count)


@lru_cache(maxsize=None)
def big_count_pairs(k):
    """Weighted pairs (ints, counts) over k-mers of the geometry records'
    genome stretches with counts past 2^32, and two records' worth whose sum
    wraps 2^64: (keys, counts, records, table)."""
    recs = [genome()[100:100 + 3 * k + 20], genome()[700:700 + 2 * k + 9] + b"N" + genome()[900:900 + k + 4],
            genome()[1500:1500 + k + 1]]
    keys = sorted(set(v for r in recs[:2] for v in window_keys(r, k)))
    counts = [(1 << 32) + 5 + 3 * i for i in range(len(keys))]
    table = dict(zip(keys, counts))
    # the last record has two windows: their counts sum to 2^64 + 7
    a, b = window_keys(recs[2], k)
    assert a != b
    table[a], table[b] = (1 << 63) + 3, (1 << 63) + 4
    keys = sorted(table)
    return keys, [table[v] for v in keys], tuple(recs), table


def pairs_input(keys, wide):
    """add_pairs' key array of Python ints."""
    if not wide:
        return np.array(keys, dtype=np.uint64)
    out = np.empty((len(keys), 2), dtype=np.uint64)
    out[:, 0] = [v & M64 for v in keys]
    out[:, 1] = [v >> 64 for v in keys]
    return out


@lru_cache(maxsize=None)
def chunk_records():
    """Host records for the chunking case at k = 31 with depth_chunk =
    CHUNK_BYTES: many short records (several chunks), one longer than a chunk,
    one that fills a chunk exactly, empties at the chunk edges."""
    rng = np.random.default_rng(107)
    recs = [_mixed(rng, int(n), 31) for n in rng.integers(20, 300, 40)]
    recs.insert(10, _mixed(rng, 3 * CHUNK_BYTES + 11, 31))
    recs.insert(20, _mixed(rng, CHUNK_BYTES - 1, 31))  # with its separator: exactly a chunk
    recs.insert(21, b"")
    recs.append(b"")
    return tuple(recs)


CHUNK_BYTES = 1500


def chunks_of(records, chunk):
    """The engine's chunking restated: whole records, at least one per chunk,
    as many as fit `chunk` packed bytes."""
    out, i = [], 0
    while i < len(records):
        j, size = i + 1, len(normalize(records[i])) + 1
        while j < len(records) and size + len(normalize(records[j])) + 1 <= chunk:
            size += len(normalize(records[j])) + 1
            j += 1
        out.append((i, j))
        i = j
    return out


def fastq_text(ids, records):
    return "".join(f"@{i}\n{r.decode()}\n+\n{'I' * len(r)}\n" for i, r in zip(ids, records))


def fasta_text(ids, records, width=60):
    out = []
    for i, r in zip(ids, records):
        s = r.decode()
        out.append(f">{i}\n" + "".join(s[o:o + width] + "\n" for o in range(0, len(s), width)))
    return "".join(out)


@lru_cache(maxsize=None)
def cli_records(k):
    """(ids, records, count-input records) of the CLI case: reads with
    present, absent and solid windows, one shorter than k, one with an N."""
    rng = np.random.default_rng(200 + k)
    recs = [_mixed(rng, int(n), k) for n in (3 * k + 11, 5 * k, 2 * k + 1)]
    recs.append(_mixed(rng, k - 1, k))
    r = bytearray(_mixed(rng, 4 * k, k))
    r[2 * k] = ord("N")
    recs.append(bytes(r))
    ids = [f"read{i} some description" for i in range(len(recs))]
    return tuple(ids), tuple(recs), table_reads()[:60]
