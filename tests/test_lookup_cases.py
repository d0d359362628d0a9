"""CPU side of the count lookup: the inputs of tests/lookup_cases.py really have
the properties their names claim, and the CLI's --lookup checks that need no
device (the flags' usage errors and the lookup file's parser, which runs
before the engine starts)."""

import subprocess

import numpy as np
import pytest

import hist_cases as hc
import lookup_cases as lc
from okm import _lib, testing


def run(*args):
    return subprocess.run([_lib.CLI_PATH, *args], capture_output=True, text=True, timeout=60)


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------

def test_expected_is_a_table_lookup():
    keys = np.array([3, 9, 10, 2**63], np.uint64)
    counts = np.array([1, 5_000_000_000, 7, 2], np.uint64)
    q = np.array([10, 0, 3, 3, 11, 2**64 - 1, 2**63, 9], np.uint64)
    got, found = lc.expected(keys, counts, q)
    assert got.tolist() == [7, 0, 1, 1, 0, 0, 2, 5_000_000_000] and found == 5
    assert lc.expected(keys[:0], counts[:0], q)[0].tolist() == [0] * 8
    got, found = lc.expected_wide({5: 2, (1 << 64) | 5: 3}, [5, 6, (1 << 64) | 5, 1 << 64, 5])
    assert got.tolist() == [2, 0, 3, 0, 2] and found == 3


def test_item_runs_lie_under_their_prefixes_in_key_order():
    runs, inp = lc.items()
    assert tuple(len(r) for r in runs) == lc.ITEM_SIZES == (1, 2, 63, 64, 65, 4096)
    assert list(lc.ITEM_PREFIXES) == sorted(lc.ITEM_PREFIXES) and max(lc.ITEM_PREFIXES) < 1 << 10
    for r, p in zip(runs, lc.ITEM_PREFIXES):
        assert np.all(r >> np.uint64(hc.LOW_BITS) == p) and np.all(np.diff(r.astype(object)) > 0)
    ek, ec = hc.table_of(inp)
    assert np.array_equal(ek, np.concatenate(runs))
    assert set(ec[:-4096].tolist()) == {1, 2, 3} and set(ec[-4096:].tolist()) == {1}
    assert int(ek.max()) < 1 << (2 * lc.K)


def test_edge_queries_hit_the_ends_and_miss_beside_them():
    runs, inp = lc.items()
    ek, ec = hc.table_of(inp)
    q = lc.edge_queries(runs)
    got, found = lc.expected(ek, ec, q)
    present = set(ek.tolist())
    n = len(runs)
    assert found >= 2 * n  # (n_found counts queries: the one-key run's first key is also its last)
    for i, r in enumerate(runs):
        first, last, below, above = (int(x) for x in q[4 * i:4 * i + 4])
        assert first == int(r[0]) and last == int(r[-1]) and first in present and last in present
        assert below == first - 1 and above == last + 1
        assert got[4 * i] > 0 and got[4 * i + 1] > 0
    assert int(q[-3]) == 0 < int(q[-2]) < int(ek[0]) < int(ek[-1]) < int(q[-1])
    assert got[-3:].tolist() == [0, 0, 0]


def test_edge_query_neighbours_are_absent():
    runs, inp = lc.items()
    ek, ec = hc.table_of(inp)
    q = lc.edge_queries(runs)
    got, _ = lc.expected(ek, ec, q)
    present = set(ek.tolist())
    for i in range(len(runs)):
        for j in (2, 3):  # one below the first, one above the last
            v = int(q[4 * i + j])
            assert (v in present) == (got[4 * i + j] > 0)
    # at least one of them lands in a gap between two runs, none of these runs is adjacent to the next
    assert all(int(q[4 * i + 3]) < int(runs[i + 1][0]) for i in range(len(runs) - 1))
    # ... and inside the longer runs the neighbour is usually absent, sometimes the next key of the run
    assert sum(1 for i in range(len(runs)) for j in (2, 3) if got[4 * i + j] == 0) >= len(runs)


def test_k32_tables():
    a, b = lc.k32_table(True), lc.k32_table(False)
    assert (a == 0).sum() == 3 and not (b == 0).any()
    for t in (a, b):
        assert not (t == np.uint64(lc.M64)).any() and int(t.max()) > 1 << 63


@pytest.mark.parametrize("k", lc.WIDE_KS)
def test_word_neighbours(k):
    table, queries = lc.word_neighbours(k)
    keys = sorted(table)
    assert (1 << (2 * k)) - 1 not in table and all(0 <= v < 1 << (2 * k) for v in keys)
    his, los = {v >> 64 for v in keys}, {v & lc.M64 for v in keys}
    assert len(his) >= 3 and {0, lc.M64} <= los
    # equal in hi and different in lo; equal in lo and different in hi
    assert any(sum(1 for v in keys if v >> 64 == h) >= 2 for h in his)
    assert any(sum(1 for v in keys if v & lc.M64 == l) >= 2 for l in los)
    got, found = lc.expected_wide(table, queries)
    assert len(queries) == 5 * len(keys) and found >= len(keys)
    assert (got == 0).sum() > len(keys)  # most neighbours are absent
    # a comparison of lo alone, or of hi alone, would find some absent query
    absent = [q for q in queries if q not in table]
    assert any(any(q & lc.M64 == v & lc.M64 for v in keys) for q in absent)
    assert any(any(q >> 64 == v >> 64 for v in keys) for q in absent)
    pairs = lc.table_input(table)
    assert pairs.shape == (sum(table.values()), 2)
    assert sorted(set(lc.from_pairs(pairs))) == keys
    assert lc.from_pairs(lc.to_pairs(queries)) == queries


def test_wide_ks_hold_a_k_whose_item_bits_straddle_the_words():
    import wide_cases as wc
    assert {33, 63, 64} < set(lc.WIDE_KS)
    assert any(wc.side(wc.fields(k)["home"]) == "straddle" for k in lc.WIDE_KS)


def test_lookup_reuses_the_hist_slice_knob():
    assert testing.KNOBS["hist_slice"] == 19 and len(testing.KNOBS) == 20


def test_lookup_file_rendering():
    text, kmers = lc.lookup_file_lines("ACGTTGCAAC", 5, ["AAAAA", "TTTTT", "CCCCC"])
    assert text.startswith(">") and "\n\n" in text and "\r\n" in text
    assert kmers[:3] == ["ACGTT", "cgttg", "GTTGC"] and kmers[-3:] == ["AAAAA", "TTTTT", "CCCCC"]
    assert lc.canonical_text("cgttg") == "CAACG" and lc.canonical_text("AAAAA") == lc.canonical_text("TTTTT")
    assert lc.render_lookup(["cgttg", "AAAAA"], {"CAACG": 4}) == "cgttg\t4\nAAAAA\t0\n"


# ---------------------------------------------------------------------------
# argument checks of the entry points that need no device
# ---------------------------------------------------------------------------

def test_null_arguments_are_refused():
    lib = _lib.load()
    buf = np.zeros(4, np.uint64)
    assert lib.okm_lookup_counts(None, buf.ctypes.data, 4, buf.ctypes.data, 0, None) == _lib.OKM_E_ARG
    assert lib.okm_lookup_counts(None, None, 0, None, 0, None) == _lib.OKM_E_ARG
    assert lib.okm_group_lookup_counts(None, buf.ctypes.data, 4, buf.ctypes.data, None) == _lib.OKM_E_ARG


# ---------------------------------------------------------------------------
# CLI: usage errors (exit 2) and the lookup file's parser, before any device use
# ---------------------------------------------------------------------------

def _count_args(tmp_path, k="5"):
    fa = tmp_path / "a.fa"
    fa.write_text(">a\nACGTACGTTGCA\n")
    return ["count", "-k", k, "-i", str(fa), "-o", str(tmp_path / "o.tsv")]


@pytest.mark.parametrize("given,missing", [("--lookup", "--lookup-output <FILE>"), ("--lookup-output", "--lookup <FILE>")])
def test_cli_lookup_flags_need_each_other(tmp_path, given, missing):
    f = tmp_path / "f.txt"
    f.write_text("ACGTA\n")
    r = run(*_count_args(tmp_path), given, str(f))
    assert r.returncode == 2, r.stderr
    assert "the following required arguments were not provided:\n  " + missing in r.stderr
    assert "For more information, try '--help'." in r.stderr
    assert not (tmp_path / "o.tsv").exists()


def test_cli_lookup_flags_need_values_and_show_in_help():
    assert run("count", "-k", "5", "-i", "a", "-o", "x", "--lookup").returncode == 2
    assert run("count", "-k", "5", "-i", "a", "-o", "x", "--lookup", "f", "--lookup-output").returncode == 2
    h = run("count", "--help")
    assert h.returncode == 0 and "--lookup <FILE>" in h.stdout and "--lookup-output <FILE>" in h.stdout


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("bad,line", [
    ("ACGTA\nACGT\nACGTA\n", 2),                 # a short line
    (">h\n\nACGTA\nACGTAC\n", 4),               # a long line (the skipped lines are numbered too)
    ("ACGTA\r\nacgta\nACGNA\n", 3),             # an N
    ("ACGTA\nACGTA \n", 2),                     # a trailing blank is not a base
    ("ACGTA\nAC>TA\n", 2),                      # '>' is a header only at the start of a line
])
def test_cli_lookup_file_errors_name_the_line(tmp_path, bad, line, wide):
    k = 35 if wide else 5
    if wide:  # the same lines, every k-mer 30 bases longer
        bad = "\n".join(("A" * 30 + l if l and not l.startswith(">") else l) for l in bad.split("\n"))
    f = tmp_path / "look.txt"
    f.write_bytes(bad.encode())
    r = run(*_count_args(tmp_path, str(k)), "--lookup", str(f), "--lookup-output", str(tmp_path / "l.tsv"),
            *(["--wide"] if wide else []))
    assert r.returncode == 1, r.stderr
    assert f"at line {line}:" in r.stderr and "lookup file" in r.stderr and f"expected {k} bases" in r.stderr
    assert not (tmp_path / "o.tsv").exists() and not (tmp_path / "l.tsv").exists()


def test_cli_missing_lookup_file(tmp_path):
    r = run(*_count_args(tmp_path), "--lookup", str(tmp_path / "none.txt"), "--lookup-output", str(tmp_path / "l.tsv"))
    assert r.returncode == 1 and "lookup file" in r.stderr
    assert not (tmp_path / "o.tsv").exists()


@pytest.mark.parametrize("gz", [False, True])
def test_cli_fasta_of_kmers_passes_the_parser(tmp_path, gz):
    """A '>'-headed FASTA of k-mers with blank lines, CRLF and lower case is
    accepted: with -v the parser reports the k-mers it read before the engine
    starts (whatever the engine then does on a machine without a device)."""
    import gzip
    text = ">one\nACGTA\n>two\r\ncgtac\r\n\n>three\nGTACG"  # no newline at the end
    f = tmp_path / ("look.fa.gz" if gz else "look.fa")
    f.write_bytes(gzip.compress(text.encode()) if gz else text.encode())
    r = run(*_count_args(tmp_path), "-v", "--lookup", str(f), "--lookup-output", str(tmp_path / "l.tsv"))
    assert "Read 3 k-mers to look up from" in r.stderr, r.stderr
    assert "Invalid k-mer" not in r.stderr
    if r.returncode == 0:  # a device was there
        from collections import Counter
        table = Counter(lc.canonical_text(m) for m in lc.kmers_of("ACGTACGTTGCA", 5))
        assert (tmp_path / "l.tsv").read_text() == lc.render_lookup(["ACGTA", "cgtac", "GTACG"], table)
