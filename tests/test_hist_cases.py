"""CPU side of the count histogram: the inputs of tests/hist_cases.py really
have the properties their names claim, okm_write_histogram_tsv against a
Python rendering, and the CLI's usage errors for --histogram-max (no device
needed: they are refused before the engine starts)."""

import gzip
import subprocess

import numpy as np
import pytest

import hist_cases as hc
import okm
from okm import _lib, testing


def run(*args):
    return subprocess.run([_lib.CLI_PATH, *args], capture_output=True, text=True, timeout=60)


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------

def test_expected_hist_is_the_clamped_bincount():
    c = np.array([1, 1, 2, 5, 6, 7, 5_000_000_000], np.uint64)
    assert hc.expected_hist(c, 7).tolist() == [0, 2, 1, 0, 0, 1, 3]
    assert hc.expected_hist(c, 2).tolist() == [0, 7]
    assert hc.expected_summary(c) == {"n_distinct": 7, "n_instances": 5_000_000_022, "max_count": 5_000_000_000}
    wrap = np.array([1 << 63, 1 << 63, 5], np.uint64)
    assert hc.expected_summary(wrap)["n_instances"] == 5  # modulo 2^64
    assert hc.expected_summary(np.zeros(0, np.uint64)) == {"n_distinct": 0, "n_instances": 0, "max_count": 0}


@pytest.mark.parametrize("m", hc.ITEM_SIZES)
def test_one_item_case_holds_m_keys_under_the_prefix(m):
    ek, ec = hc.table_of(hc.one_item(m))
    inside = (ek >> np.uint64(hc.LOW_BITS)) == (hc.PREFIX >> np.uint64(hc.LOW_BITS))
    assert int(inside.sum()) == m and (ec[inside] == 1).all()
    assert m <= 4096  # one count item holds them
    # populated ranges on both sides, several count values in them
    assert (ek < hc.PREFIX).sum() == 100 and (ek >= hc.PREFIX_ABOVE).sum() == 100
    assert set(ec[~inside].tolist()) == set(range(1, 8))
    assert int(ek.max()) < 1 << (2 * hc.K)


def test_many_items_case_counts():
    keys = hc.many_items()
    ek, ec = hc.table_of(keys)
    assert len(ek) == 3000 and len(keys) == 451_500
    assert sorted(ec.tolist()) == sorted(((np.arange(3000) % 300) + 1).tolist())
    # spread over far more key ranges than one L1 bin (10 bits at most)
    assert len(np.unique(ek >> np.uint64(52))) > 500


@pytest.mark.parametrize("count", [1, 3])
def test_all_one_count_case_holds_one_count_value(count):
    ek, ec = hc.table_of(hc.all_one_count(count))
    assert len(ek) == 200_000 and set(ec.tolist()) == {count}


def test_hot_among_singletons_case():
    ek, ec = hc.table_of(hc.hot_among_singletons())
    assert len(ek) == 50_001 and int(ec.max()) == 4096
    assert int((ec == 1).sum()) == 50_000


@pytest.mark.parametrize("n_bins", hc.BIN_EDGE_NBINS)
def test_count_at_the_last_bin_edge(n_bins):
    keys, counts = hc.count_equals_index()
    assert len(np.unique(keys)) == len(keys) == hc.BIN_EDGE_TOP
    have = set(counts.tolist())
    assert hc.N_BINS_MIN <= n_bins <= hc.N_BINS_MAX
    if n_bins <= hc.BIN_EDGE_TOP:  # the counts just below, at and just above the last bin
        assert {c for c in (n_bins - 2, n_bins - 1, n_bins) if c >= 1} <= have
        assert hc.expected_hist(counts, n_bins)[n_bins - 1] == hc.BIN_EDGE_TOP - (n_bins - 2)
    else:  # the last bin at or past the largest count: 70,001 -> count 70,000 is the last bin's only key
        assert hc.expected_hist(counts, n_bins)[hc.BIN_EDGE_TOP] == 1
        assert hc.expected_hist(counts, n_bins)[hc.BIN_EDGE_TOP + 1:].sum() == 0
    assert hc.expected_hist(counts, n_bins).sum() == hc.BIN_EDGE_TOP


def test_bin_edge_sweep_brackets_every_power_of_two_lds_size():
    """A private LDS histogram of 2^b u32 bins, b <= 16 (64 KB of the
    workgroup's LDS at most), has its crossover inside the sweep."""
    nb = sorted(hc.BIN_EDGE_NBINS)
    for b in range(1, 17):
        assert nb[0] <= (1 << b) + 1 and any(x > (1 << b) for x in nb)
    assert 4097 in nb and 65536 in nb and 65537 in nb


def test_past_u32_case():
    runs, (ek, ec) = hc.past_u32_runs()
    for keys, counts in runs:
        assert (np.diff(keys.astype(np.int64)) > 0).all() and len(keys) == len(counts)
    big = np.sort(ec)[-2:]
    assert big.tolist() == [5_000_000_000, 6_000_000_000]
    assert int(np.sort(ec)[-3]) < 3000  # everything else far below the last bin used with it
    assert max(int(c.max()) for _, c in runs) < 1 << 33 and int(ec.max()) > 1 << 32


def test_fold_pairs_share_keys():
    a, b = hc.fold_pairs()
    assert len(np.intersect1d(a, b)) > 1000 and len(np.setdiff1d(a, b)) > 1000 and len(np.setdiff1d(b, a)) > 1000


def test_hist_slice_knob_is_number_19():
    assert testing.KNOBS["hist_slice"] == 19 and len(testing.KNOBS) == 20
    testing.set_knob("hist_slice", 1000)
    assert testing.get_knob("hist_slice") == 1000
    testing.set_knob("hist_slice", -1)
    assert testing.get_knob("hist_slice") == -1


# ---------------------------------------------------------------------------
# okm_write_histogram_tsv
# ---------------------------------------------------------------------------

def test_writer_omits_zero_bins_and_labels_the_last_bin(tmp_path):
    hist = np.array([0, 7, 0, 0, 12, 1, 0, 3], np.uint64)  # last bin (label 7) = counts >= 7
    p = tmp_path / "h.tsv"
    okm.write_histogram_tsv(str(p), hist)
    assert p.read_text() == "1\t7\n4\t12\n5\t1\n7\t3\n" == hc.render_tsv(hist)
    # no header line; a last bin holding zero is omitted like any other
    okm.write_histogram_tsv(str(p), np.array([0, 2, 0], np.uint64))
    assert p.read_text() == "1\t2\n"


def test_writer_large_values_and_many_bins(tmp_path):
    rng = np.random.default_rng(3)
    hist = rng.integers(0, 3, hc.N_BINS_MAX).astype(np.uint64)
    hist[1] = np.uint64(18_446_744_073_709_551_615)
    hist[-1] = 9
    p = tmp_path / "big.tsv"
    okm.write_histogram_tsv(str(p), hist)
    txt = p.read_text()
    assert txt == hc.render_tsv(hist)
    assert txt.endswith(f"{hc.N_BINS_MAX - 1}\t9\n")


def test_writer_empty_histogram_gives_empty_file(tmp_path):
    p = tmp_path / "e.tsv"
    p.write_text("stale")
    okm.write_histogram_tsv(str(p), np.zeros(10001, np.uint64))
    assert p.read_bytes() == b""


def test_writer_gz_round_trip(tmp_path):
    hist = hc.expected_hist(np.arange(1, 5000, dtype=np.uint64) % np.uint64(37), 30)
    p = tmp_path / "h.tsv.gz"
    okm.write_histogram_tsv(str(p), hist)
    raw = p.read_bytes()
    assert raw[:2] == b"\x1f\x8b"
    assert gzip.decompress(raw).decode() == hc.render_tsv(hist)


def test_writer_errors(tmp_path):
    with pytest.raises(okm.OkmError) as ei:
        okm.write_histogram_tsv(str(tmp_path / "no" / "such" / "dir" / "h.tsv"), np.ones(3, np.uint64))
    assert ei.value.status == _lib.OKM_E_IO
    assert _lib.load().okm_write_histogram_tsv(None, None, 0) == _lib.OKM_E_ARG


# ---------------------------------------------------------------------------
# argument checks of the entry points that need no device
# ---------------------------------------------------------------------------

def test_null_arguments_are_refused():
    lib = _lib.load()
    buf = np.zeros(4, np.uint64)
    assert lib.okm_count_histogram(None, buf.ctypes.data, 4, None) == _lib.OKM_E_ARG
    assert lib.okm_group_count_histogram(None, buf.ctypes.data, 4, None) == _lib.OKM_E_ARG


# ---------------------------------------------------------------------------
# CLI usage errors (exit 2, worded like --min-count's), before any device use
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["separate", "equals"])
@pytest.mark.parametrize("bad", ["0", "x", "-3", "1.5", "1048577"])
def test_cli_histogram_max_usage_error(tmp_path, bad, form):
    fa = tmp_path / "a.fa"
    fa.write_text(">a\nACGTACGT\n")
    flag = ["--histogram-max", bad] if form == "separate" else [f"--histogram-max={bad}"]
    r = run("count", "-k", "5", "-i", str(fa), "-o", str(tmp_path / "o.tsv"), "--histogram", str(tmp_path / "h.tsv"),
            *flag)
    assert r.returncode == 2, r.stderr
    assert f"invalid value '{bad}' for '--histogram-max <HISTOGRAM_MAX>'" in r.stderr
    assert not (tmp_path / "o.tsv").exists() and not (tmp_path / "h.tsv").exists()


def test_cli_min_count_usage_error_has_the_same_wording(tmp_path):
    r = run("count", "-k", "5", "-i", "a", "-o", str(tmp_path / "o.tsv"), "-m", "x")
    assert r.returncode == 2 and "invalid value 'x' for '--min-count <MIN_COUNT>'" in r.stderr


def test_cli_histogram_flags_need_values_and_show_in_help():
    assert run("count", "-k", "5", "-i", "a", "-o", "x", "--histogram").returncode == 2
    assert run("count", "-k", "5", "-i", "a", "-o", "x", "--histogram-max").returncode == 2
    h = run("count", "--help")
    assert h.returncode == 0 and "--histogram <FILE>" in h.stdout and "--histogram-max <N>" in h.stdout
    # -o stays required
    assert run("count", "-k", "5", "-i", "a", "--histogram", "h.tsv").returncode == 2
