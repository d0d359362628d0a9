"""The CLI's --intervals flags: the usage errors (exit 2), before any device call."""

import subprocess

import pytest

from okm import _lib

NEEDS = "the following required arguments were not provided:\n  "
BOTH = ("--intervals", "READS", "--intervals-output", "OUT")


@pytest.mark.parametrize("given,message", [
    (("--intervals", "READS"), NEEDS + "--intervals-output <FILE>"),
    (("--intervals-output", "OUT"), NEEDS + "--intervals <FASTX>"),
    (("--intervals-min-count", "0"), NEEDS + "--intervals <FASTX>"),
    (("--intervals-slots",), NEEDS + "--intervals <FASTX>"),
    (BOTH + ("--intervals-min-count", "x"), "invalid value 'x' for '--intervals-min-count <N>'"),
    (BOTH + ("--intervals-max-count", "1"), "invalid value '1' for '--intervals-max-count <N>'"),  # below the default 2
    (BOTH + ("--intervals-min-count", "5", "--intervals-max-count", "4"),
     "invalid value '4' for '--intervals-max-count <N>'"),
    (BOTH + ("--gpus", "2"), "the argument '--intervals <FASTX>' cannot be used with '--gpus <GPUS>' other than 1"),
])
def test_usage_errors(tmp_path, given, message):
    fa, reads = tmp_path / "a.fa", tmp_path / "reads.fa"
    fa.write_text(">a\nACGTACGTTGCA\n")
    reads.write_text(">r\nACGTACGT\n")
    args = [{"READS": str(reads), "OUT": str(tmp_path / "i.bed")}.get(a, a) for a in given]
    r = subprocess.run([_lib.CLI_PATH, "count", "-k", "5", "-i", str(fa), "-o", str(tmp_path / "o.tsv"), *args],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and message in r.stderr and "For more information, try '--help'." in r.stderr, r.stderr
    assert not (tmp_path / "o.tsv").exists() and not (tmp_path / "i.bed").exists()
