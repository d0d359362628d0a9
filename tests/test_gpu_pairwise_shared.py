"""okm_pairwise_shared on the device, exact against Python sets: M[i][j] =
|kept_i & kept_j| and occupancy[p] = keys kept in exactly p samples, over
samples with planted overlaps; and `compare --pairwise-output`."""

import subprocess
from collections import Counter

import numpy as np
import pytest

import okm
from okm import _lib

pytestmark = pytest.mark.gpu


def _planted(n):
    """Key sets (Python ints) of n samples: a core in all, a block in every
    other sample, private keys; with n >= 3 sample 1 is empty and the last
    sample is sample 0 given again (None)."""
    rng = np.random.default_rng(100 + n)
    pool = [int(x) for x in np.unique(rng.integers(1, 1 << 60, 300 + 40 * n, dtype=np.uint64))]
    core, block, rest = pool[:150], pool[150:250], pool[250:]
    sets = []
    for i in range(n):
        private = rest[37 * i:37 * i + 30 + i]
        sets.append(set(core) | (set(block) if i % 2 == 0 else set()) | set(private))
    if n >= 3:
        sets[1] = set()
        sets[-1] = None
    return sets


@pytest.mark.parametrize("min_count", [1, 2])
@pytest.mark.parametrize("k", [31, 45])
@pytest.mark.parametrize("n", [1, 2, 3, 33, 64])
def test_planted_overlaps(n, k, min_count):
    wide = k > 32
    sets = _planted(n)
    counters, kept = [], []
    try:
        for i, s in enumerate(sets):
            if s is None:  # the same context twice
                counters.append(counters[0])
                kept.append(kept[0])
                continue
            set_mode = i % 3 == 1 or (n < 3 and i == 1)
            lo = np.array(sorted(s), dtype=np.uint64)[::-1]  # (unsorted input)
            keys = np.stack([lo, lo & np.uint64(0xFFFF)], axis=1) if wide else lo  # hi follows from lo: lo names the key
            c = okm.KmerCounter(k, "set" if set_mode else "count", wide=wide)
            counters.append(c)
            if len(lo):
                c.add_pairs(keys, None if set_mode else lo % np.uint64(3) + np.uint64(1))  # counts 1..3
            kept.append(s if set_mode else {x for x in s if x % 3 + 1 >= min_count})
        before = [c.result(1) for c in counters]
        m, occ = okm.pairwise_shared(counters, min_count)
        em = np.array([[len(a & b) for b in kept] for a in kept], dtype=np.uint64).reshape(n, n)
        per_key = Counter(x for s in kept for x in s)
        eocc = np.bincount(list(per_key.values()), minlength=n + 1).astype(np.uint64)
        assert np.array_equal(m, em) and np.array_equal(occ, eocc)
        for c, (bk, bc) in zip(counters, before):  # the samples are as they were
            ak, ac = c.result(1)
            assert np.array_equal(ak, bk) and np.array_equal(ac, bc)
    finally:
        for c in set(counters):
            c.close()


def test_argument_errors():
    lib = _lib.load()
    buf = np.zeros(65 * 65, np.uint64)
    with okm.KmerCounter(31) as a, okm.KmerCounter(21) as b:
        a.add_pairs(np.arange(1, 50, dtype=np.uint64))
        for counters in ([], [a] * 65, [a, b]):
            with pytest.raises(okm.OkmError) as ei:
                okm.pairwise_shared(counters)
            assert ei.value.status == _lib.OKM_E_ARG
        assert lib.okm_pairwise_shared(None, 1, 1, buf.ctypes.data, None) == _lib.OKM_E_ARG
        m, occ = okm.pairwise_shared([a, a])
        assert m.tolist() == [[49, 49], [49, 49]] and occ.tolist() == [0, 0, 49]


def _cli(*args):
    return subprocess.run([_lib.CLI_PATH, "compare", *args], capture_output=True, text=True, timeout=120)


def test_cli_pairwise_output(tmp_path):
    rng = np.random.default_rng(21)
    pool = np.unique(rng.integers(0, 1 << 42, 4000, dtype=np.uint64))
    refs = [(f"ref{i}.fa", np.sort(rng.choice(pool, size, replace=False)))
            for i, size in enumerate([900, 1500, 0, 700, 1200])]
    p1, p2 = str(tmp_path / "a.db"), str(tmp_path / "b.db")
    okm.KmerDb(21, dict(refs[:3])).write(p1)
    okm.KmerDb(21, dict(refs[3:])).write(p2)
    plain, out, pw = tmp_path / "plain.json", tmp_path / "out.json", tmp_path / "pairs.tsv"
    assert _cli("--db1", p1, "--db2", p2, "-o", str(plain)).returncode == 0
    r = _cli("--db1", p1, "--db2", p2, "-o", str(out), "--pairwise-output", str(pw))
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == plain.read_bytes() and plain.stat().st_size > 0
    names = [name for name, _ in refs]
    sets = [set(v.tolist()) for _, v in refs]
    exp = ""
    for i in range(5):
        for j in range(i + 1, 5):
            sh = len(sets[i] & sets[j])
            uni = len(sets[i]) + len(sets[j]) - sh
            exp += f"{names[i]}\t{names[j]}\t{len(sets[i])}\t{len(sets[j])}\t{sh}\t{(sh / uni if uni else 0.0):.6f}\n"
    assert pw.read_text() == exp


def test_cli_more_than_64_references(tmp_path):
    keys = np.arange(1, 20, dtype=np.uint64)
    p1, p2 = str(tmp_path / "a.db"), str(tmp_path / "b.db")
    okm.KmerDb(21, {f"r{i}": keys + np.uint64(i) for i in range(33)}).write(p1)
    okm.KmerDb(21, {f"s{i}": keys + np.uint64(i) for i in range(32)}).write(p2)
    r = _cli("--db1", p1, "--db2", p2, "-o", str(tmp_path / "o.json"), "--pairwise-output", str(tmp_path / "p.tsv"))
    assert r.returncode == 1 and "at most 64 references" in r.stderr and "65" in r.stderr, r.stderr
