"""bench.py's plain run and `--dump-outputs DIR`: the line of a plain run
carries the headline figure and none of the `--full` measurements, and the
dumped float64 arrays are the sorted (key, count) table of the benchmark's own
seeded batch (whole when small, consecutive blocks of it when large), checked
against the table a fresh context counts from the same reads."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import okm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

K, READ_LEN, GENOME_BP, SEED = 31, 150, 100_000_000, 2  # bench.py's configs[1] batch
BLOCK, BLOCKS = 4096, 512                               # bench.py DUMP_BLOCK / DUMP_BLOCKS


def expected_table(reads):
    batch = okm.synth_reads(reads, READ_LEN, genome_len=GENOME_BP, genome_seed=SEED, seed=SEED, first_read=0,
                            sub_rate=0.001, n_rate=0.0001)
    buf = okm.DeviceBuffer(len(batch), 0)
    buf.upload(batch)
    with okm.KmerCounter(K, "count", 0) as c:
        c.add_device_batch(buf.address, len(batch))
        keys, counts = c.result(1)
    buf.free()
    return keys, counts


# 2,000 reads: 240,000 windows, the table is written whole; 60,000 reads: ~7 M
# windows of a 100 Mbp genome, nearly all distinct, above BLOCKS * BLOCK entries
@pytest.mark.parametrize("reads,sampled", [(2_000, False), (60_000, True)])
def test_plain_run_dumps_its_table(tmp_path, reads, sampled):
    d = tmp_path / "dump"
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--reads", str(reads), "--dump-outputs", str(d)],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "bases/s" and line["dtype"] == "u64"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(reads * READ_LEN / (line["ms_per_step"] * 1e-3), rel=1e-2)
    # nothing of --full in a plain run
    for name in ("roofline", "cpu_baseline", "cpu_baseline_mt", "single_job", "with_dense_table"):
        assert line[name] is None, name
    assert line["kernels"] == {} and "c3" not in line

    keys, counts = expected_table(reads)
    n = len(keys)
    assert (n > BLOCKS * BLOCK) == sampled
    files = sorted(os.listdir(d))
    assert files == ["counts.npy", "keys_hi32.npy", "keys_lo32.npy", "summary.npy"]
    assert sum(os.path.getsize(d / f) for f in files) <= 64_000_000
    arr = {f[:-4]: np.load(d / f) for f in files}
    assert all(a.dtype == np.float64 for a in arr.values())
    assert arr["summary"].tolist() == [n, int(counts.sum())]
    got_k = (arr["keys_hi32"].astype(np.uint64) << np.uint64(32)) | arr["keys_lo32"].astype(np.uint64)
    got_c = arr["counts"].astype(np.uint64)
    if not sampled:
        assert np.array_equal(got_k, keys) and np.array_equal(got_c, counts)
        return
    assert got_k.shape == got_c.shape == (BLOCKS * BLOCK,)
    starts = np.searchsorted(keys, got_k[::BLOCK])  # each block: BLOCK consecutive entries of the table
    assert starts[0] == 0 and starts[-1] == n - BLOCK and np.all(np.diff(starts) >= 0)
    idx = (starts[:, None] + np.arange(BLOCK)[None, :]).reshape(-1)
    assert np.array_equal(got_k, keys[idx]) and np.array_equal(got_c, counts[idx])
    assert len(np.unique(starts)) > BLOCKS // 2  # spread over the table, not one block repeated
