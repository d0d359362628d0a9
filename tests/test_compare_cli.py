import subprocess

import pytest

from okm import _lib

BASE = ["count", "-k", "5", "-i", "in.fa", "-o", "out.tsv"]


def _cli(*args):
    return subprocess.run([_lib.CLI_PATH, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("extra,needle", [
    (["--compare", "b.fa"], "--compare-output <FILE>"),
    (["--compare-output", "c.tsv"], "--compare <FASTX>"),
    (["--compare", "b.fa", "--compare-output", "c.tsv", "--compare-min-count", "2x"], "'2x' for '--compare-min-count <N>'"),
    (["--compare", "b.fa", "--compare-output", "c.tsv", "--gpus", "2"], "'--compare <FASTX>' cannot be used with '--gpus"),
])
def test_usage_errors(extra, needle):
    r = _cli(*BASE, *extra)
    assert r.returncode == 2 and needle in r.stderr and r.stdout == "", r.stderr


def test_help_lists_the_flags():
    r = _cli("count", "--help")
    assert r.returncode == 0
    for flag in ("--compare <FASTX>", "--compare-output <FILE>", "--compare-min-count <N>"):
        assert sum(line.lstrip().startswith(flag) for line in r.stdout.splitlines()) == 1
