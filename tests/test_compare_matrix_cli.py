"""--compare-matrix / --compare-matrix-bins: usage errors and help lines, before any device call."""

import pytest

from test_compare_cli import BASE, _cli

CMP = ["--compare", "b.fa", "--compare-output", "c.tsv"]
BINS_FLAG = "'--compare-matrix-bins <A>,<B>'"


@pytest.mark.parametrize("extra,needle", [
    (["--compare-matrix", "m.tsv"], "--compare <FASTX>"),
    (["--compare-matrix-bins", "10,10"], "--compare <FASTX>"),
    (CMP + ["--compare-matrix-bins", "10,10"], "--compare-matrix <FILE>"),
    (["--compare", "b.fa", "--compare-matrix", "m.tsv"], "--compare-output <FILE>"),  # an additional output
] + [(CMP + ["--compare-matrix", "m.tsv", "--compare-matrix-bins", v], f"'{v}' for {BINS_FLAG}")
     for v in ("10", "10,", ",10", "10,x", "10,10,10", "1,10", "10,1", "65537,2", "2049,2048", "-5,5")])
def test_usage_errors(extra, needle):
    r = _cli(*BASE, *extra)
    assert r.returncode == 2 and needle in r.stderr and r.stdout == "", r.stderr


def test_help_lists_the_flags():
    r = _cli("count", "--help")
    assert r.returncode == 0
    for flag in ("--compare-matrix <FILE>", "--compare-matrix-bins <A>,<B>"):
        assert sum(line.lstrip().startswith(flag) for line in r.stdout.splitlines()) == 1
