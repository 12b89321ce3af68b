"""bench.py --dump-outputs: what the last timed step returned, as .npy files two builds can be compared by (the writer alone here;
tests/test_gpu_bench.py runs the benchmark)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _results(B, cap, seed=5):
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 2**32, size=(B, cap, 2), dtype=np.uint64).astype(np.uint32)     # (slots past a count hold junk)
    out_n = rng.integers(0, cap + 1, size=B).astype(np.uint32)
    return out, out_n


def test_dump_holds_the_results_in_float64_and_zeros_past_the_count(tmp_path):
    out, out_n = _results(300, 40)
    out[0, 0, 0] = 4_000_000_001                       # doc ids beyond float32's exact range survive
    out_n[0] = max(1, out_n[0])
    bench.dump_outputs(str(tmp_path), out, out_n)
    assert sorted(os.listdir(tmp_path)) == ["counts.npy", "doc_ids.npy", "scores.npy"]
    ids, sc, n = (np.load(tmp_path / f"{k}.npy") for k in ("doc_ids", "scores", "counts"))
    assert ids.dtype == sc.dtype == n.dtype == np.float64
    assert ids.shape == sc.shape == (300, 40) and n.shape == (300,)
    assert np.array_equal(n, out_n)
    assert ids[0, 0] == 4_000_000_001
    for q in range(300):
        k = int(out_n[q])
        assert np.array_equal(ids[q, :k], out[q, :k, 0]) and np.array_equal(sc[q, :k], out[q, :k, 1])
        assert not ids[q, k:].any() and not sc[q, k:].any()


def test_a_large_batch_is_sampled_the_same_way_every_time(tmp_path):
    B, cap = 120_000, 40                                # 77 MB of float64 in all: over the 64 MB cap
    out, out_n = _results(B, cap)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), out, out_n)
    bench.dump_outputs(str(b), out.copy(), out_n.copy())
    total = sum(os.path.getsize(a / f) for f in os.listdir(a))
    assert total <= 64 << 20
    qi = np.load(a / "query_index.npy")
    assert 0 < len(qi) < B and np.all(np.diff(qi) > 0)
    for f in os.listdir(a):
        assert np.array_equal(np.load(a / f), np.load(b / f))
    ids, n = np.load(a / "doc_ids.npy"), np.load(a / "counts.npy")
    rows = qi.astype(np.int64)
    assert np.array_equal(n, out_n[rows])
    k = int(out_n[rows[7]])
    assert np.array_equal(ids[7, :k], out[rows[7], :k, 0])
    # ... and a later dump of a batch that fits leaves no stale sample index behind
    small, small_n = _results(100, cap)
    bench.dump_outputs(str(a), small, small_n)
    assert "query_index.npy" not in os.listdir(a)
