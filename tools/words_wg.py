#!/usr/bin/env python3
"""tools/words_wg.py -- what option words_wg buys on an index whose group takes the DIRECTORY + WORDS form by the density rule, nothing
forced: DOCS (10 M) fingerprints x 256 hashes in 16 synthetic segments (2.56 G items, 2.4 positions per 128-byte line), then in 8.  Batches
of 8192 x 1000, resident, eight distinct batches in rotation; words_wg 0 and 1 ALTERNATE in one process, RUNS (3) runs each, STEPS (40)
steps per run after a warm-up, one batch in flight and three.  Three shapes per index: the group alone; + 16 memory segments (the kernel's
MEM instantiation); + a memory segment that re-inserts about a thousand docs of the group with new hashes (the group gets dead sets: the
FILT instantiation, option 2 against 0).  One JSON line per run: ms per step (one and three in flight), probe_kernel_ms, path_flags, and
whether the run's results are byte for byte those of the shape's first words_wg = 0 run.

    python tools/words_wg.py                                        (~15 s per index on an MI355X)
    SEGMENTS=16 python tools/words_wg.py                            one index per process (SEGMENTS=8: group_segments fails on eight members
                                                                    of 320 M items as of round 13 -- profiles/r13_words_wg.txt section 2)
    PLAIN_ONLY=1 FPX_LIB=.../libfpx_prev.so python tools/words_wg.py   the same shapes with no option touched: another build's own path"""
import concurrent.futures as cf
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def same_results(a, b):
    (out_a, n_a), (out_b, n_b) = a, b
    if not np.array_equal(n_a, n_b):
        return False
    valid = np.arange(out_a.shape[1])[None, :] < n_a[:, None].astype(np.int64)
    return bool(np.array_equal(out_a[valid], out_b[valid]))


def main():
    import torch  # noqa: F401  (one HIP runtime in the process: torch's, loaded first)
    import bench
    from __graft_entry__ import load_package
    fpx = load_package()
    ctx = fpx.Context(0)
    docs_all, H, B = int(os.environ.get("DOCS", 10_000_000)), 256, int(os.environ.get("BATCH", 8192))
    steps, runs, nfl = int(os.environ.get("STEPS", 40)), int(os.environ.get("RUNS", 3)), int(os.environ.get("INFLIGHT", 3))
    plain_only = os.environ.get("PLAIN_ONLY") == "1"
    lib = os.path.basename(os.environ.get("FPX_LIB", "libfpx.so"))
    seed = 20260928
    opts = fpx.http_options()
    for S in [int(x) for x in os.environ.get("SEGMENTS", "16,8").split(",")]:
        t0 = time.perf_counter()
        segs, _ = bench.synth_index(fpx, ctx, seed, docs_all, S, H, set(range(S)))
        docs = (docs_all // S) * S
        batches = [fpx.synth.make_queries(seed, 4242 + 1000003 * i, B, docs, H, query_len=1000) for i in range(8)]
        qbs = [fpx.QueryBatch(ctx, options=opts, flat=(f, o)) for f, o, _ in batches]
        next_doc, commit, mems = docs + 1, S + 1, []
        per_mem = 100_000 // H
        for m in range(16):
            ids = np.arange(next_doc, next_doc + per_mem, dtype=np.uint64)
            hh = fpx.synth.synth_hashes(seed + 77, ids, H, 0).astype(np.uint64)
            items = np.sort(((hh << np.uint64(32)) | ids[:, None]).ravel())
            mems.append(fpx.MemorySegment(ctx, items, int(ids[0]), int(ids[-1]), commit, ids.astype(np.uint32)))
            next_doc += per_mem; commit += 1
        again = np.arange(7, docs, docs // 1000, dtype=np.uint64)[:1000]            # docs of the group written again, with other hashes
        hh = fpx.synth.synth_hashes(seed + 78, again, H, 0).astype(np.uint64)
        items = np.sort(((hh << np.uint64(32)) | again[:, None]).ravel())
        rewrite = fpx.MemorySegment(ctx, items, int(again[0]), int(again[-1]), commit, again.astype(np.uint32))
        shapes = [("the group alone", [], 1), ("+ 16 memory segments", mems, 1), ("+ 1000 docs re-inserted", [rewrite], 2)]
        for label, extra, level in shapes:
            snap = fpx.Segments(ctx, list(segs) + extra)
            info = {k: v for k, v in snap.info().items() if k in ("groups", "packed_groups", "group_columns", "direct_solo", "memory")}
            gi = segs[0].group_info()
            if label == shapes[0][0]:
                print(json.dumps({"lib": lib, "segments": S, "docs": docs, "built_s": round(time.perf_counter() - t0, 1), "info": info,
                                  "group": {k: gi[k] for k in ("columns", "line_columns", "packed", "lines", "bytes")}}), flush=True)
            reader = fpx.IndexReader(snap)
            first = None
            for r in range(2 if plain_only else 2 * runs):        # words_wg 0, level, 0, level, ...
                value = None if plain_only else (r % 2) * level
                if value is not None:
                    ctx.set_option("words_wg", value)
                try:
                    dt, agg, out, out_n = bench.timed_resident(fpx, reader, qbs, steps, 8)
                    res = (out.copy(), out_n.copy())
                    bufs = [(np.zeros_like(out), np.zeros_like(out_n)) for _ in range(nfl)]

                    def one(i):
                        o, n_ = bufs[i % nfl]
                        fpx.search_resident(reader, qbs[i % len(qbs)], 0, o, n_)
                    with cf.ThreadPoolExecutor(nfl) as ex:
                        list(ex.map(one, range(4 * nfl)))
                        t_m = time.perf_counter()
                        list(ex.map(one, range(steps * nfl)))
                        dt_m = time.perf_counter() - t_m
                finally:
                    if value is not None:
                        ctx.set_option("words_wg", -1)
                if first is None:
                    first = res
                tg = batches[(8 + steps - 1) % len(batches)][2]
                print(json.dumps({"lib": lib, "segments": S, "snapshot": label, "words_wg": value, "run": r // 2,
                                  "ms_per_step": round(dt / steps * 1e3, 4), "ms_per_step_3_in_flight": round(dt_m / (steps * nfl) * 1e3, 4),
                                  "probe_kernel_ms": round(agg.v["probe_kernel_ms"] / steps, 4), "gpu_ms_per_step": round(agg.v["total_gpu_ms"] / steps, 4),
                                  "path_flags": agg.path_flags, "same_bytes_as_first_run": same_results(first, res),
                                  "targets_found": int(sum(1 for q in range(B) if res[1][q] > 0 and res[0][q, 0, 0] == tg[q])), "of": B}), flush=True)
            snap.release()
            del reader, snap
        for q_ in qbs:
            q_.release()
        for s_ in list(segs) + mems + [rewrite]:
            s_.release()
        del segs, mems, rewrite
        ctx.trim()


if __name__ == "__main__":
    main()
