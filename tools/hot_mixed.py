#!/usr/bin/env python3
"""tools/hot_mixed.py -- what option hot_wg buys on MIXED traffic: the 100 M index with hot postings (bench.py's dist_z index: 2 % of every
fingerprint's hashes from a pool of 4096 hot values, a hot hash carries the capped 1000 docs in each of the 16 segments), batches of 8192
queries of which 0.1 %, 1 %, 5 % and 25 % keep HOT_PER_QUERY (2) of their target's hot hashes -- 16 000 records per hot hash, more than
k_search_query's LDS array takes -- and the rest none.  hot_wg 0 and 1 ALTERNATE in one process, RUNS (3) runs each per share, STEPS (40)
resident batches per run after a warm-up: under hot_wg = 0 the hand-back and the 32 batches of back-off behind it are inside the run,
as they are in production (what is left of that back-off is drained before the next hot_wg = 1 run starts).  One JSON line per run: ms per step, the GPU time of the calls, how many steps ran k_search_query (path_flags
bit 6) and how many redid queries in doc classes (bit 10), hit records per batch, targets found.

    DOCS=100000000 python tools/hot_mixed.py"""
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
    keep = int(os.environ.get("HOT_PER_QUERY", 2))
    shares = [float(x) for x in os.environ.get("SHARES", "0.001,0.01,0.05,0.25").split(",")]
    t0 = time.perf_counter()
    segs, _ = bench.synth_index(fpx, ctx, seed, docs, S, H, set(range(S)), dist=1)
    docs = (docs // S) * S
    reader = fpx.IndexReader(fpx.Segments(ctx, segs))
    print(json.dumps({"built_s": round(time.perf_counter() - t0, 1), "docs": docs}), flush=True)
    # the pool of hot values (synth_hashes, dist 1)
    k = np.arange(4096, dtype=np.uint64)
    with np.errstate(over="ignore"):
        pool = (synth.mix64(np.uint64(seed) ^ synth._HOT ^ (k << np.uint64(32))) >> np.uint64(32)).astype(np.uint32)
    opts = fpx.http_options()
    rng = np.random.default_rng(11)
    for share in shares:
        qbs, targets, nhot = [], [], 0
        for i in range(2):
            f, o, t = synth.make_queries(seed, 4242 + 1000003 * i, B, docs, H, query_len=1000, dist=1)
            f = f.reshape(B, -1).copy()
            hot = np.isin(f, pool)
            rank = np.cumsum(hot, axis=1)                            # a query's hot hashes, counted from its first
            is_hot_q = np.zeros(B, dtype=bool)
            is_hot_q[rng.choice(B, max(1, int(round(share * B))), replace=False)] = True
            drop = hot & ~(is_hot_q[:, None] & (rank <= keep))       # every hot hash but the first `keep` of a hot query becomes noise
            noise = rng.integers(0, 1 << 32, f.shape, dtype=np.uint64).astype(np.uint32)
            noise[np.isin(noise, pool)] ^= np.uint32(0x55AA55AA)
            f = np.where(drop, noise, f)
            nhot += int((np.isin(f, pool).sum(axis=1) > 0).sum())
            qbs.append(fpx.QueryBatch(ctx, options=opts, flat=(np.ascontiguousarray(f.ravel()), o)))
            targets.append(t)
        out = out_n = None
        for r in range(2 * runs):                                    # hot_wg 0, 1, 0, 1, ...
            ctx.set_option("hot_wg", r % 2)
            try:
                for i in range(8 if r < 2 else 2):                   # (a path's first batches size its buffers)
                    out, out_n, _ = fpx.search_resident(reader, qbs[i % 2], 0, out, out_n)
                # (hot_wg = 1 does not back off, but the hot_wg = 0 run before it has left the snapshot some batches of its back-off: they
                # are taken off here, or they would be timed as this option's)
                for i in range(40 if r % 2 == 1 and share * B <= B // 8 else 0):
                    out, out_n, st = fpx.search_resident(reader, qbs[i % 2], 0, out, out_n)
                    if st.path_flags & 64:
                        break
                gpu_ms = hits = 0.0
                on_qs = redone = 0
                t_r = time.perf_counter()
                for i in range(steps):
                    out, out_n, st = fpx.search_resident(reader, qbs[i % 2], 0, out, out_n)
                    gpu_ms += st.total_gpu_ms; hits += st.hits
                    on_qs += 1 if st.path_flags & 64 else 0
                    redone += 1 if st.path_flags & 1024 else 0
                dt = time.perf_counter() - t_r
            finally:
                ctx.set_option("hot_wg", -1)
            t = targets[(steps - 1) % 2]
            print(json.dumps({"hot_share": share, "hot_queries_per_batch": nhot / 2, "hot_hashes_per_hot_query": keep, "hot_wg": r % 2, "run": r // 2,
                              "ms_per_step": round(dt / steps * 1e3, 4), "gpu_ms_per_step": round(gpu_ms / steps, 4),
                              "steps": steps, "steps_query_per_workgroup": on_qs, "steps_redone_in_classes": redone,
                              "records_per_batch": round(hits / steps), "targets_found": int(sum(1 for q in range(B) if out_n[q] > 0 and out[q, 0, 0] == t[q])), "of": B}), flush=True)
        for q_ in qbs:
            q_.release()


if __name__ == "__main__":
    main()
