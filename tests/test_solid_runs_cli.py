"""The CLI's --solid-runs flags: the usage errors (exit 2), which return before
any device call; tests/test_gpu_solid_runs.py runs the command itself."""

import subprocess

import pytest

from okm import _lib

NEEDS = "the following required arguments were not provided:\n  "


@pytest.mark.parametrize("given,message", [
    (("--solid-runs", "READS"), NEEDS + "--solid-runs-output <FILE>"),
    (("--solid-runs-output", "OUT"), NEEDS + "--solid-runs <FASTX>"),
    (("--solid-runs-min-count", "3"), NEEDS + "--solid-runs <FASTX>"),
    (("--solid-runs", "READS", "--solid-runs-min-count", "3"), NEEDS + "--solid-runs-output <FILE>"),
] + [(("--solid-runs", "READS", "--solid-runs-output", "OUT", "--solid-runs-min-count", bad),
      f"invalid value '{bad}' for '--solid-runs-min-count <N>'") for bad in ("0", "-1", "two")])
def test_usage_errors(tmp_path, given, message):
    fa, reads = tmp_path / "a.fa", tmp_path / "reads.fa"
    fa.write_text(">a\nACGTACGTTGCA\n")
    reads.write_text(">r\nACGTACGT\n")
    args = [{"READS": str(reads), "OUT": str(tmp_path / "s.tsv")}.get(a, a) for a in given]
    r = subprocess.run([_lib.CLI_PATH, "count", "-k", "5", "-i", str(fa), "-o", str(tmp_path / "o.tsv"), *args],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and message in r.stderr and "For more information, try '--help'." in r.stderr, r.stderr
    assert not (tmp_path / "o.tsv").exists() and not (tmp_path / "s.tsv").exists()
