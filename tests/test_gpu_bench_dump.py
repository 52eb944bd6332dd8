"""-m gpu: a plain `bench.py` run with `--dump-outputs`.  The result line carries the contract's fields, `--steps` sets the number of
timed steps, the dump is float32 / float64 and under 64 MB, and what it holds is the timed path's output: every sampled chunk's bytes are
the oracle's bytes for the numbers decoded from it (bench.py asserts decode(encode(x)) == x in its warm-up)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import oracle_lib as O  # noqa: E402
import gpu_util as U  # noqa: E402

pytestmark = pytest.mark.gpu


def test_plain_bench_run_dumps_the_last_steps_outputs(tmp_path):
    dump = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--chunks", "64",
                        "--dump-outputs", str(dump)], capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["unit"] == "GB/s" and line["higher_is_better"] is True and line["ms_per_step"] > 0
    assert "cpu_baseline" not in line and "other_workloads" not in line["config"] and line["config"]["oracle_verified_chunks"] == 0
    assert not (tmp_path / "bench_full.json").exists()   # (the full record is written by --full runs only)

    arrays = {f[:-4]: np.load(dump / f) for f in os.listdir(dump)}
    assert set(arrays) == {"compressed_sizes", "sample_chunks", "decoded", "compressed"}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    sizes, pick, dec, comp = arrays["compressed_sizes"], arrays["sample_chunks"], arrays["decoded"], arrays["compressed"]
    assert sizes.shape == (64,) and pick.shape == (8,) and dec.shape == (8, U.N18)
    assert comp.size == int(sizes[pick.astype(np.int64)].sum())
    cfg = O.make_config(mode=1, delta=2, delta_order=1)   # the headline workload, c2
    pos = 0
    for i, row in zip(pick.astype(np.int64), dec):
        got = bytes(comp[pos: pos + int(sizes[i])].astype(np.uint8)); pos += int(sizes[i])
        nums = row.astype(np.uint64)
        assert np.array_equal(nums.astype(np.float64), row)   # (the ramp's numbers are exact in float64)
        assert got == U.chunk_of_file(O.simple_compress(nums, cfg), len(got)), f"chunk {i}: dumped bytes differ from the oracle's"
