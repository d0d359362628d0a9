"""okm_add_text[_device]: FASTA/FASTQ text parsed on the device, against the
plain-Python restatement (parse_fastx -> normalize -> every window), exactly."""

import contextlib
import functools
import gzip
import os
import subprocess

import numpy as np
import pytest

import okm
import restate
from conftest import GOLDEN
from okm import _lib, testing

pytestmark = pytest.mark.gpu

FORMS = ["host", "device", "device+1"]  # +1: a device pointer that is not 16-B aligned
CODE = {65: 0, 67: 1, 71: 2, 84: 3}


def bases(n, seed):
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, n)])


def build(recs, fastq=False, width=0, eol=b"\n", extra=0, last_eol=True):
    """The one text builder: records (name, sequence) as FASTQ or as FASTA of the given line width."""
    out = b""
    for name, seq in recs:
        if fastq:
            out += b"@" + name + b"h" * extra + eol + seq + eol + b"+" + eol + b"I" * len(seq) + eol
        else:
            lines = [seq[i:i + width] for i in range(0, len(seq), width)] if width else [seq]
            out += b">" + name + eol + b"".join(ln + eol for ln in lines if ln)
    return out if last_eol else out[:len(out) - len(eol)]


@functools.lru_cache(maxsize=None)
def want(text, k):
    table = {}
    for _, raw in restate.parse_fastx(text):
        s = restate.normalize(raw)
        for i in range(len(s) - k + 1):
            if all(c in CODE for c in s[i:i + k]):
                f = r = 0
                for j, c in enumerate(s[i:i + k]):
                    f = f << 2 | CODE[c]
                    r |= (3 - CODE[c]) << (2 * j)
                table[min(f, r)] = table.get(min(f, r), 0) + 1
    return table


def got(ctr):
    keys, counts = ctr.result(1)
    if ctr.wide:
        keys = [int(hi) << 64 | int(lo) for lo, hi in keys]
    return {int(key): int(c) for key, c in zip(keys, counts)}


def add(ctr, text, form):
    if form == "host":
        return ctr.add_text(text)
    import torch
    pad = 1 if form == "device+1" else 0
    t = torch.frombuffer(bytearray(b"\0" * pad + text), dtype=torch.uint8).cuda()[pad:]
    assert t.data_ptr() % 16 == pad
    return ctr.add_text_device(t)


def check(text, k, form, mode="count", chunk=None):
    with okm.KmerCounter(k, mode, 0, wide=k > 32) as ctr:
        with testing.knobs(depth_chunk=chunk) if chunk else contextlib.nullcontext():
            assert add(ctr, text, form) == len(restate.parse_fastx(text))
        if mode == "set":
            assert sorted(got(ctr)) == sorted(want(text, k))
        else:
            assert got(ctr) == want(text, k)


READS = [(b"r%d" % i, bases(n, i)) for i, n in enumerate([70, 150, 33, 1, 64])]


@pytest.mark.parametrize("form", FORMS[:2])
@pytest.mark.parametrize("extra", range(18))
def test_fastq_every_granule_residue(extra, form):
    check(build(READS, fastq=True, extra=extra), 21, form)


def tile_text():
    """> 32 KiB of FASTQ: a sequence line across byte 16384, a '\\n' at byte 32767."""
    text = b""
    for i in range(18):
        seq, hdr = bases(1000, 100 + i), b"r%d" % i
        end = len(text) + 1 + len(hdr) + 1 + len(seq)  # where the sequence line's '\n' falls
        if end <= 32767 < end + 2010:
            hdr += b"x" * (32767 - end)
        text += build([(hdr, seq)], fastq=True)
    assert text[32767:32768] == b"\n" and text[32766] in CODE and text[32768:32769] == b"+"
    assert text[16383] in CODE and text[16384] in CODE
    return text


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k,mode", [(1, "count"), (2, "count"), (31, "count"), (32, "count"), (33, "count"),
                                    (64, "count"), (31, "set")])
def test_tile_borders_every_width(k, mode, form):
    check(tile_text(), k, form, mode)


MIXED = [(b"a x", b"acgtACGTuUNnACGTTGCA AC\tGTACGTAC"), (b"empty", b""), (b"b", b"ACG>TACGTTTGACCA" * 4)]
CONTENT = {
    **{"fasta_w%d%s" % (w, "_crlf" if e == b"\r\n" else ""): build([(b"s", bases(200, 7)), (b"t", bases(61, 8))], width=w, eol=e)
       for w in (1, 60, 61) for e in (b"\n", b"\r\n")},
    "header_only_first": build([(b"e", b"")] + MIXED[::2]),
    "header_only_middle_mixed_bytes": build(MIXED, width=11),
    "header_only_last": build(MIXED[::2] + [(b"e", b"")]),
    "header_only_last_no_eol": build(MIXED[::2] + [(b"e", b"")], last_eol=False),
    "fasta_no_final_eol": build(MIXED, width=7, last_eol=False),
    "fastq_mixed_bytes": build([m for m in MIXED if m[1]], fastq=True),
    "fastq_crlf_no_final_eol": build(READS, fastq=True, eol=b"\r\n", last_eol=False),
    "fastq_quality_at_plus_and_plus_id": b"@q\nACGTACGT\n+q\n@IIIIIII\n@p\nTTGACCAT\n+\n+IIIIIII\n",
    "fastq_trailing_blank": build(READS, fastq=True) + b"\n\r\n",
    "golden_fasta": gzip.decompress(open(os.path.join(GOLDEN, "data", "test_input1.fasta.gz"), "rb").read()),
    "golden_fastq": gzip.decompress(open(os.path.join(GOLDEN, "data", "test_input2.fastq.gz"), "rb").read()),
}


@pytest.mark.parametrize("form", FORMS[:2])
@pytest.mark.parametrize("name", sorted(CONTENT))
def test_content(name, form):
    check(CONTENT[name], 5, form)


def cut_text(c):
    """CRLF FASTA whose cuts at c, 2c and 3c fall between CR and LF, right before a '>' and inside a header."""
    text = b">a\r\n" + bases(c - 5, 1) + b"\r\n" + bases(c - 3, 2) + b"\r\n>" + b"h" * (c + 20) + b"\r\n" + bases(300, 3) + b"\r\n"
    assert text[c - 1:c + 1] == b"\r\n" and text[2 * c:2 * c + 1] == b">" and text.rfind(b"\n", 0, 3 * c) + 1 == 2 * c
    return text


TWICE = bases(2480, 11) + b"GATTACAGATTACAGATTACAG" + bases(2478, 12) + b"GATTACAGATTACAGATTACAG"
CHUNKED = {
    "fastq_150": lambda c: build([(b"r%d" % i, bases(150, 20 + i)) for i in range(6)], fastq=True),
    "fastq_1000": lambda c: build([(b"r%d" % i, bases(1000, 30 + i)) for i in range(3)], fastq=True),
    "fasta_one_line_5000": lambda c: build([(b"s", TWICE)]),
    "fasta_cuts": lambda c: cut_text(max(c, 97)),
}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("c", [1, 97, 700])
@pytest.mark.parametrize("name", sorted(CHUNKED))
def test_chunks(name, c, form):
    text = CHUNKED[name](c)
    assert len(text) > 2 * c
    check(text, 21, form, chunk=c)


def test_add_text_after_add_batch_counts_add():
    text = build(READS, fastq=True)
    with okm.KmerCounter(21, "count", 0) as ctr:
        ctr.add_records([s for _, s in READS])
        ctr.add_text(text)
        assert got(ctr) == {key: 2 * c for key, c in want(text, 21).items()}


GOOD = build([(b"g%d" % i, bases(150, 40 + i)) for i in range(4)], fastq=True)
BAD = {
    "no_at": b"r\nACGT\n+\nIIII\n", "no_plus": b"@r\nACGT\n-\nIIII\n", "lengths": b"@r\nACGT\n+\nIII\n",
    "truncated_1": b"@r\n", "truncated_2": b"@r\nACGT\n", "truncated_3": b"@r\nACGT\n+\n",
    "blank_between": b"\n@r\nACGT\n+\nIIII\n", "empty": None, "first_byte": None,
}


@pytest.mark.parametrize("form", FORMS[:2])
@pytest.mark.parametrize("chunk", [None, 700])
@pytest.mark.parametrize("name", sorted(BAD))
def test_errors_match_the_host_parser(name, chunk, form):
    text = {"empty": b"", "first_byte": b"ACGT\n"}.get(name) if BAD[name] is None else GOOD + BAD[name]
    assert len(GOOD) > 700
    with pytest.raises(_lib.OkmError) as host:
        okm.parse_fastx(text)
    with okm.KmerCounter(21, "count", 0) as ctr:
        with testing.knobs(depth_chunk=chunk) if chunk else contextlib.nullcontext():
            if text or form == "host":  # (no tensor of zero bytes)
                with pytest.raises(_lib.OkmError) as dev:
                    add(ctr, text, form)
                assert dev.value.status == host.value.status
                assert str(dev.value).split(": ", 1)[1] == str(host.value).split(": ", 1)[1]
        ctr.reset()
        assert testing.device_in_use(ctr) == 0
        add(ctr, GOOD, form)
        assert got(ctr) == want(GOOD, 21)


def test_allocation_failures():
    text = build([(b"r%d" % i, bases(150, 50 + i)) for i in range(5)], fastq=True)
    with okm.KmerCounter(21, "count", 0) as ctr, testing.knobs(depth_chunk=700):
        testing.set_knob("fail_alloc", 10 ** 9)
        ctr.add_text(text)
        assert got(ctr) == want(text, 21)
        n = 10 ** 9 - testing.get_knob("fail_alloc")
        assert n >= 8  # two chunks' blocks at least
        for i in range(1, n + 1):
            ctr.reset()
            assert testing.device_in_use(ctr) == 0
            testing.set_knob("fail_alloc", i)
            try:
                ctr.add_text(text)
                table = got(ctr)
            except _lib.OkmError as e:
                assert e.status == _lib.OKM_E_NOMEM, e
            else:
                assert table == want(text, 21), i
            testing.set_knob("fail_alloc", -1)
        ctr.reset()
        assert testing.device_in_use(ctr) == 0


@pytest.mark.parametrize("tail,code", [(b"", 0), (b"@r\nACGT\n+\nIII\n", 1)])
def test_cli_device_parse(tmp_path, tail, code):
    fq = tmp_path / "in.fq"
    fq.write_bytes(build(READS[:3], fastq=True) + tail)
    runs = []
    for flag in ([], ["--device-parse"]):
        out = tmp_path / ("o%d.tsv" % len(flag))
        r = subprocess.run([_lib.CLI_PATH, "count", "-k", "11", "-i", str(fq), "-o", str(out), *flag],
                           capture_output=True, text=True, timeout=120)
        last = [ln.split("] ", 1)[-1] for ln in r.stderr.strip().splitlines()[-1:]]  # without the "[time LEVEL target] "
        assert bool(code) == (last == ["Error: Error reading record from " + str(fq)]), r.stderr
        runs.append((r.returncode, last, out.read_bytes() if out.exists() else None))
    assert runs[0] == runs[1] and (runs[0][0] != 0) == bool(code) and (code or runs[0][2])
