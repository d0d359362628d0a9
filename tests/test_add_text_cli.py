"""--device-parse and the text entry points, as far as they go without a device."""

import ctypes
import gzip
import os
import subprocess

from conftest import GOLDEN
from okm import _lib


def test_device_parse_needs_one_gpu(tmp_path):
    fa = tmp_path / "a.fa"
    fa.write_text(">a\nACGTACGTTGCA\n")
    r = subprocess.run([_lib.CLI_PATH, "count", "-k", "5", "-i", str(fa), "-o", str(tmp_path / "o.tsv"),
                        "--device-parse", "--gpus", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, r.stderr
    assert "the argument '--device-parse' cannot be used with '--gpus <GPUS>' other than 1" in r.stderr
    assert "For more information, try '--help'." in r.stderr and not (tmp_path / "o.tsv").exists()


def test_help_line():
    r = subprocess.run([_lib.CLI_PATH, "count", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "      --device-parse  " in r.stdout and "on the GPU" in r.stdout


def test_reader_text_is_the_inflated_file():
    path = os.path.join(GOLDEN, "data", "test_input2.fastq.gz")
    lib, r = _lib.load(), ctypes.c_void_p()
    assert lib.okm_reader_open(ctypes.byref(r), path.encode(), 1) == _lib.OKM_OK
    text, n = ctypes.c_void_p(), ctypes.c_uint64()
    assert lib.okm_reader_text(r, ctypes.byref(text), ctypes.byref(n)) == _lib.OKM_OK
    assert ctypes.string_at(text, n.value) == gzip.decompress(open(path, "rb").read())
    assert lib.okm_reader_text(None, ctypes.byref(text), ctypes.byref(n)) == _lib.OKM_E_ARG
    lib.okm_reader_close(r)


def test_add_text_null_arguments():
    lib, n = _lib.load(), ctypes.c_uint64()
    for fn in (lib.okm_add_text, lib.okm_add_text_device):
        assert fn(None, None, 0, ctypes.byref(n)) in (_lib.OKM_E_ARG, _lib.OKM_E_DEVICE)
