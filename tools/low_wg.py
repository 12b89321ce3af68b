#!/usr/bin/env python3
"""tools/low_wg.py -- what option low_wg buys on traffic with score floors of 1 and 2: the 100 M index (bench.py's: 16 synthetic segments,
one packed group), resident batches of 8192 queries of 1000 hashes, one batch in flight.  Four mixes: every query with the legacy
protocol's options (min_score 1, min_score_pct 10, limit 500: src/legacy.zig:192-197); 1 % and 10 % of the queries with them and the rest
HTTP defaults; every query with min_score 1, min_score_pct 0, limit 100 -- nothing raises the floor there, the top-K cut does all the work.
low_wg 0 and 1 ALTERNATE in one process, RUNS (3) runs each per mix, STEPS (40) batches per run after a warm-up; option 0 is the parent's
path (the pipeline) and the baseline of every figure.  One JSON line per run: ms per step, the GPU time of the calls, how many steps ran
k_search_low (path_flags bit 12) and k_search_query's path at all (bit 6), hit records per batch, targets found, and whether the run's
results are byte for byte those of the mix's first low_wg = 0 run.

    DOCS=100000000 python tools/low_wg.py"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch  # noqa: F401  (one HIP runtime in the process: torch's, loaded first)
    import bench
    from __graft_entry__ import load_package
    fpx = load_package()
    synth = fpx.synth
    ctx = fpx.Context(0)
    docs, S, H, B = int(os.environ.get("DOCS", 100_000_000)), 16, 256, int(os.environ.get("BATCH", 8192))
    seed, steps, runs = 20260928, int(os.environ.get("STEPS", 40)), int(os.environ.get("RUNS", 3))
    t0 = time.perf_counter()
    segs, _ = bench.synth_index(fpx, ctx, seed, docs, S, H, set(range(S)))
    docs = (docs // S) * S
    reader = fpx.IndexReader(fpx.Segments(ctx, segs))
    print(json.dumps({"built_s": round(time.perf_counter() - t0, 1), "docs": docs}), flush=True)
    http, legacy = fpx.http_options(), fpx.SearchOptions(max_results=500, min_score=1, min_score_pct=10)
    flat_cut = fpx.SearchOptions(max_results=100, min_score=1, min_score_pct=0)
    rng = np.random.default_rng(15)
    mixes = [("legacy 100 %", legacy, 1.0), ("legacy 1 %", legacy, 0.01), ("legacy 10 %", legacy, 0.1), ("min_score 1, pct 0, limit 100", flat_cut, 1.0)]
    only = os.environ.get("MIXES")
    for m, (label, low_opts, share) in enumerate(mixes):
        if only and str(m) not in only.split(","):
            continue
        qbs, targets = [], []
        for i in range(2):
            f, o, t = synth.make_queries(seed, 4242 + 1000003 * i, B, docs, H, query_len=1000)
            is_low = np.zeros(B, dtype=bool)
            is_low[rng.choice(B, max(1, int(round(share * B))), replace=False)] = True
            qbs.append(fpx.QueryBatch(ctx, options=[low_opts if x else http for x in is_low], flat=(np.ascontiguousarray(f), o)))
            targets.append(t)
        out = out_n = first = None
        for r in range(2 * runs):                                    # low_wg 0, 1, 0, 1, ...
            ctx.set_option("low_wg", r % 2)
            try:
                for i in range(8 if r < 2 else 2):                   # (a path's first batches size its buffers)
                    out, out_n, _ = fpx.search_resident(reader, qbs[i % 2], 0, out, out_n)
                gpu_ms = hits = 0.0
                on_low = on_qs = 0
                t_r = time.perf_counter()
                for i in range(steps):
                    out, out_n, st = fpx.search_resident(reader, qbs[i % 2], 0, out, out_n)
                    gpu_ms += st.total_gpu_ms; hits += st.hits
                    on_low += 1 if st.path_flags & 4096 else 0
                    on_qs += 1 if st.path_flags & 64 else 0
                dt = time.perf_counter() - t_r
            finally:
                ctx.set_option("low_wg", -1)
            t = targets[(steps - 1) % 2]
            used = [out[q, :out_n[q]].tobytes() for q in range(B)]
            if first is None:
                first = used
            print(json.dumps({"mix": label, "low_wg": r % 2, "run": r // 2, "ms_per_step": round(dt / steps * 1e3, 4),
                              "gpu_ms_per_step": round(gpu_ms / steps, 4), "steps": steps, "steps_k_search_low": on_low,
                              "steps_query_per_workgroup": on_qs, "records_per_batch": round(hits / steps),
                              "results_per_query": round(float(out_n[:B].mean()), 2), "same_as_first_low_wg_0_run": used == first,
                              "targets_found": int(sum(1 for q in range(B) if out_n[q] > 0 and out[q, 0, 0] == t[q])), "of": B}), flush=True)
        for q_ in qbs:
            q_.release()


if __name__ == "__main__":
    main()
