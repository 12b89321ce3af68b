"""bench.py as a plain run: --steps timed steps, one JSON line, and --dump-outputs writes the results of the LAST timed step -- the
same files from two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "5", "--warmup", "1", "--docs", "2000000", "--segments", "4", "--batch", "512"]


def _run(dump_dir):
    env = dict(os.environ, FPX_BENCH_SETTLE_S="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *ARGS, "--dump-outputs", str(dump_dir)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    d = _run(tmp_path / "a")
    assert d["steps"] == 5 and d["warmup"] == 1 and d["unit"] == "queries/s" and d["higher_is_better"] is True and d["dtype"] == "u32"
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - 512) < 1e-6 * 512           # value = B x steps / time, ms_per_step = time / steps
    assert d["targets_found"] == d["targets_total"] == 512
    for k in ("by_batch", "end_to_end", "config1", "roofline_block_form", "dist_z", "value_long", "measured_bandwidth"):
        assert k not in d, k                                                       # (--full's)
    assert d["cpu_baseline"] is None
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    fpx = load_package()
    # the last timed step (4) searched resident batch 4 of the eight in rotation: its results rank every query's target first
    _, _, targets = fpx.synth.make_queries(20260928, 4242 + 1000003 * 4, 512, 2000000, 256, query_len=1000)
    ids, sc, n = (np.load(tmp_path / "a" / f"{k}.npy") for k in ("doc_ids", "scores", "counts"))
    assert ids.dtype == np.float64 and ids.shape[0] == 512 and n.shape == (512,)
    assert np.all(n > 0) and np.array_equal(ids[:, 0], targets.astype(np.float64))
    assert np.all(sc[:, 0] > 0)
    _run(tmp_path / "b")
    for f in ("doc_ids", "scores", "counts"):
        assert np.array_equal(np.load(tmp_path / "a" / f"{f}.npy"), np.load(tmp_path / "b" / f"{f}.npy")), f
