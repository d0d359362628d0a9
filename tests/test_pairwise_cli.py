"""`compare --pairwise-output` without a value: the usual usage error, before any GPU work."""

import subprocess

from okm import _lib


def test_pairwise_output_needs_a_value(tmp_path):
    r = subprocess.run([_lib.CLI_PATH, "compare", "--db1", "a.db", "--db2", "b.db", "-o", str(tmp_path / "o.json"),
                        "--pairwise-output"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "a value is required for '--pairwise-output'" in r.stderr and r.stdout == "", r.stderr
    assert not (tmp_path / "o.json").exists()
