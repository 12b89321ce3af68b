#!/usr/bin/env python3
"""tools/groups_low_wg.py -- what option groups_wg = 2 buys on traffic with score floors of 1 and 2 over an index of TWO packed groups: the
headline's index (bench.py's: DOCS docs in 16 synthetic segments, one packed group of 16 columns) and, behind it, a second packed group
of 2 and then of 8 more segments of the same size -- DOCS = 100 M where both fit next to each other; the output says which index it was.
Resident batches of 8192 queries of 1000 hashes aimed at docs of BOTH groups, one batch in flight, low_wg = 1 throughout.  tools/low_wg.py's
four mixes: every query with the legacy protocol's options (min_score 1, min_score_pct 10, limit 500: src/legacy.zig:192-197); 1 % and
10 % of the queries with them and the rest HTTP defaults; every query with min_score 1, min_score_pct 0, limit 100.
groups_wg 0, 1 and 2 ALTERNATE in one process, RUNS (3) runs each per mix, STEPS (40) batches per run after a warm-up.  Each level searches
a snapshot made under it.  Levels 0 and 1 are the code as it was and the baseline: under 0 the snapshot is in two parts -- k_search_low on
the large group, the pipeline on the small one, the tables merged --, under 1 a batch with a low floor sends the whole snapshot through
the pipeline; under 2 both groups are walked a query per workgroup, k_search_low and k_search_low_next.  The new level is to be compared
with the better of the two.  One JSON line per run: ms per step, the GPU time of the calls, how many steps set path_flags bit 13 (several
groups a query per workgroup), bit 12 (the sorted tail's kernels), bit 7 (two parts) and bit 6, hit records per batch, targets found, and
whether the run's results are byte for byte those of the mix's first groups_wg = 0 run.

    DOCS=100000000 python tools/groups_low_wg.py"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEVELS = (0, 1, 2)


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
    per = docs // S
    docs = per * S
    first = fpx.IndexReader(fpx.Segments(ctx, segs))               # (the first snapshot: the group of 16)
    info = segs[0].group_info()
    print(json.dumps({"built_s": round(time.perf_counter() - t0, 1), "docs": docs, "first_group": {k: info[k] for k in ("columns", "line_columns", "packed", "bytes")}}), flush=True)
    if not info["packed"]:
        print(json.dumps({"error": "the first group is not packed"}), flush=True)
        return 1
    http, legacy = fpx.http_options(), fpx.SearchOptions(max_results=500, min_score=1, min_score_pct=10)
    flat_cut = fpx.SearchOptions(max_results=100, min_score=1, min_score_pct=0)
    mixes = [("legacy 100 %", legacy, 1.0), ("legacy 1 %", legacy, 0.01), ("legacy 10 %", legacy, 0.1), ("min_score 1, pct 0, limit 100", flat_cut, 1.0)]
    only = os.environ.get("MIXES")
    ctx.set_option("low_wg", 1)
    try:
        for more in [int(x) for x in os.environ.get("SECOND", "2,8").split(",")]:
            t0 = time.perf_counter()
            extra = [fpx.FileSegment.synth(ctx, seed, docs + s * per + 1, per, H, 0, 512, S + 1 + s) for s in range(more)]
            ctx.set_option("group_packed", 1)                      # (a group this sparse would take the directory + words form by itself)
            readers = {}
            try:
                for level in (2, 1, 0):                            # (the second group forms under the first of the three snapshots)
                    ctx.set_option("groups_wg", level)
                    readers[level] = fpx.IndexReader(fpx.Segments(ctx, segs + extra))
            finally:
                ctx.set_option("groups_wg", -1)
                ctx.set_option("group_packed", -2)
            info2 = extra[0].group_info()
            sinfo = readers[2].snapshot.info()
            print(json.dumps({"second_group_segments": more, "second_group_docs": more * per, "built_s": round(time.perf_counter() - t0, 1),
                              "second_group": info2 and {k: info2[k] for k in ("columns", "line_columns", "packed", "bytes")},
                              "snapshot": {k: sinfo[k] for k in ("groups", "packed_groups", "bytes")}}), flush=True)
            if not info2 or not info2["packed"] or sinfo["packed_groups"] != 2:
                print(json.dumps({"error": "the second packed group did not form (no room?)", "reasons": [g.layout_reason for g in extra]}), flush=True)
                return 1
            all_docs = docs + more * per
            rng = np.random.default_rng(20)
            for m, (label, low_opts, share) in enumerate(mixes):
                if only and str(m) not in only.split(","):
                    continue
                qbs, targets = [], []
                for i in range(2):
                    f, o, t = synth.make_queries(seed, 4242 + 1000003 * i, B, all_docs, H, query_len=1000)
                    is_low = np.zeros(B, dtype=bool)
                    is_low[rng.choice(B, max(1, int(round(share * B))), replace=False)] = True
                    qbs.append(fpx.QueryBatch(ctx, options=[low_opts if x else http for x in is_low], flat=(np.ascontiguousarray(f), o)))
                    targets.append(t)
                out = out_n = first_used = None
                for r in range(len(LEVELS) * runs):                  # groups_wg 0, 1, 2, 0, 1, 2, ...
                    level = LEVELS[r % len(LEVELS)]
                    ctx.set_option("groups_wg", level)
                    try:
                        for i in range(8 if r < len(LEVELS) else 2):  # (a path's first batches size its buffers)
                            out, out_n, _ = fpx.search_resident(readers[level], qbs[i % 2], 0, out, out_n)
                        gpu_ms = hits = 0.0
                        on_groups = on_low = on_parts = on_qs = 0
                        t_r = time.perf_counter()
                        for i in range(steps):
                            out, out_n, st = fpx.search_resident(readers[level], qbs[i % 2], 0, out, out_n)
                            gpu_ms += st.total_gpu_ms; hits += st.hits
                            on_groups += 1 if st.path_flags & 8192 else 0
                            on_low += 1 if st.path_flags & 4096 else 0
                            on_parts += 1 if st.path_flags & 128 else 0
                            on_qs += 1 if st.path_flags & 64 else 0
                        dt = time.perf_counter() - t_r
                    finally:
                        ctx.set_option("groups_wg", -1)
                    t = targets[(steps - 1) % 2]
                    used = [out[q, :out_n[q]].tobytes() for q in range(B)]
                    if first_used is None:
                        first_used = used
                    print(json.dumps({"second_group_segments": more, "mix": label, "groups_wg": level, "run": r // len(LEVELS),
                                      "ms_per_step": round(dt / steps * 1e3, 4), "gpu_ms_per_step": round(gpu_ms / steps, 4), "steps": steps,
                                      "steps_several_groups": on_groups, "steps_sorted_tail": on_low, "steps_two_parts": on_parts,
                                      "steps_query_per_workgroup": on_qs, "records_per_batch": round(hits / steps),
                                      "results_per_query": round(float(out_n[:B].mean()), 2), "same_as_first_groups_wg_0_run": used == first_used,
                                      "targets_found": int(sum(1 for q in range(B) if out_n[q] > 0 and out[q, 0, 0] == t[q])),
                                      "targets_in_second_group": int((np.asarray(t) > docs).sum()), "of": B}), flush=True)
                for q_ in qbs:
                    q_.release()
            for rd in readers.values():
                rd.snapshot.release()
            readers.clear()
            for sg in extra:
                sg.release()
            del extra
    finally:
        ctx.set_option("low_wg", -1)
    del first
    return 0


if __name__ == "__main__":
    sys.exit(main())
