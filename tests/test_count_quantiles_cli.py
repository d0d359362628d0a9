"""The CLI's --quantiles flags: the usage errors (exit 2) and the --quantiles-at parser, before any device call."""

import subprocess

import pytest

from okm import _lib

NEEDS = "the following required arguments were not provided:\n  "
BOTH = ("--quantiles", "READS", "--quantiles-output", "OUT")


@pytest.mark.parametrize("given,message", [
    (("--quantiles", "READS"), NEEDS + "--quantiles-output <FILE>"),
    (("--quantiles-output", "OUT"), NEEDS + "--quantiles <FASTX>"),
    (("--quantiles-at", "1/2"), NEEDS + "--quantiles <FASTX>"),
    (("--quantiles", "READS", "--quantiles-at", "1/2"), NEEDS + "--quantiles-output <FILE>"),
] + [(BOTH + ("--quantiles-at", bad), f"invalid value '{bad}' for '--quantiles-at <A/B,...>'")
     for bad in ("1", "1/0", "3/2", "1/2,", ",1/2", "1/2,,1/4", "a/b", "1/2/3", "-1/2", "/2", "1/4294967296",
                 "0/1,1/4,1/2,3/4,1/1")])  # the last: five
def test_usage_errors(tmp_path, given, message):
    fa, reads = tmp_path / "a.fa", tmp_path / "reads.fa"
    fa.write_text(">a\nACGTACGTTGCA\n")
    reads.write_text(">r\nACGTACGT\n")
    args = [{"READS": str(reads), "OUT": str(tmp_path / "q.tsv")}.get(a, a) for a in given]
    r = subprocess.run([_lib.CLI_PATH, "count", "-k", "5", "-i", str(fa), "-o", str(tmp_path / "o.tsv"), *args],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and message in r.stderr and "For more information, try '--help'." in r.stderr, r.stderr
    assert not (tmp_path / "o.tsv").exists() and not (tmp_path / "q.tsv").exists()
