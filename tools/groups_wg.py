#!/usr/bin/env python3
"""tools/groups_wg.py -- what option groups_wg buys on an index of TWO packed groups: the headline's index (bench.py's: DOCS docs in 16
synthetic segments, one packed group of 16 columns) and, behind it, a second packed group of 2 and then of 8 more segments of the same
size -- DOCS = 100 M where both fit next to each other (the 100 M index takes 147 GB, a group of 8-column lines 69 GB of lines more);
the output says which index it was.  Resident batches of 8192 queries of 1000 hashes aimed at docs of BOTH groups, one batch in flight.
groups_wg 0 and 1 ALTERNATE in one process, RUNS (3) runs each, STEPS (40) batches per run after a warm-up.  Each option searches a
snapshot made under it: under 0 that is the parent's path -- two parts, the large group by k_search_query, the small one by the pipeline,
the tables merged --, under 1 the two groups are walked one after the other by k_search_query and k_search_next.  One JSON line per run:
ms per step, the GPU time of the calls, how many steps set path_flags bit 13 (several groups a query per workgroup), bit 7 (two parts)
and bit 6, hit records per batch, targets found, and whether the run's results are byte for byte those of the first groups_wg = 0 run.

    DOCS=100000000 python tools/groups_wg.py"""
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
    per = docs // S
    docs = per * S
    first = fpx.IndexReader(fpx.Segments(ctx, segs))               # (the first snapshot: the group of 16)
    info = segs[0].group_info()
    print(json.dumps({"built_s": round(time.perf_counter() - t0, 1), "docs": docs, "first_group": {k: info[k] for k in ("columns", "line_columns", "packed", "bytes")}}), flush=True)
    if not info["packed"]:
        print(json.dumps({"error": "the first group is not packed"}), flush=True)
        return 1
    http = fpx.http_options()
    for more in [int(x) for x in os.environ.get("SECOND", "2,8").split(",")]:
        t0 = time.perf_counter()
        extra = [fpx.FileSegment.synth(ctx, seed, docs + s * per + 1, per, H, 0, 512, S + 1 + s) for s in range(more)]
        ctx.set_option("group_packed", 1)                          # (a group this sparse would take the directory + words form by itself)
        readers = {}
        try:
            for level in (1, 0):                                   # (the second group forms under the first of the two snapshots)
                ctx.set_option("groups_wg", level)
                readers[level] = fpx.IndexReader(fpx.Segments(ctx, segs + extra))
        finally:
            ctx.set_option("groups_wg", -1)
            ctx.set_option("group_packed", -2)
        info2 = extra[0].group_info()
        sinfo = readers[1].snapshot.info()
        print(json.dumps({"second_group_segments": more, "second_group_docs": more * per, "built_s": round(time.perf_counter() - t0, 1),
                          "second_group": info2 and {k: info2[k] for k in ("columns", "line_columns", "packed", "bytes")},
                          "snapshot": {k: sinfo[k] for k in ("groups", "packed_groups", "bytes")}}), flush=True)
        if not info2 or not info2["packed"] or sinfo["packed_groups"] != 2:
            print(json.dumps({"error": "the second packed group did not form (no room?)", "reasons": [g.layout_reason for g in extra]}), flush=True)
            return 1
        all_docs = docs + more * per
        qbs, targets = [], []
        for i in range(2):
            f, o, t = synth.make_queries(seed, 4242 + 1000003 * i, B, all_docs, H, query_len=1000)
            qbs.append(fpx.QueryBatch(ctx, options=http, flat=(np.ascontiguousarray(f), o)))
            targets.append(t)
        out = out_n = first_used = None
        for r in range(2 * runs):                                    # groups_wg 0, 1, 0, 1, ...
            level = r % 2
            ctx.set_option("groups_wg", level)
            try:
                for i in range(8 if r < 2 else 2):                   # (a path's first batches size its buffers)
                    out, out_n, _ = fpx.search_resident(readers[level], qbs[i % 2], 0, out, out_n)
                gpu_ms = hits = 0.0
                on_groups = on_parts = on_qs = 0
                t_r = time.perf_counter()
                for i in range(steps):
                    out, out_n, st = fpx.search_resident(readers[level], qbs[i % 2], 0, out, out_n)
                    gpu_ms += st.total_gpu_ms; hits += st.hits
                    on_groups += 1 if st.path_flags & 8192 else 0
                    on_parts += 1 if st.path_flags & 128 else 0
                    on_qs += 1 if st.path_flags & 64 else 0
                dt = time.perf_counter() - t_r
            finally:
                ctx.set_option("groups_wg", -1)
            t = targets[(steps - 1) % 2]
            used = [out[q, :out_n[q]].tobytes() for q in range(B)]
            if first_used is None:
                first_used = used
            print(json.dumps({"second_group_segments": more, "groups_wg": level, "run": r // 2, "ms_per_step": round(dt / steps * 1e3, 4),
                              "gpu_ms_per_step": round(gpu_ms / steps, 4), "steps": steps, "steps_several_groups": on_groups, "steps_two_parts": on_parts,
                              "steps_query_per_workgroup": on_qs, "records_per_batch": round(hits / steps),
                              "same_as_first_groups_wg_0_run": used == first_used,
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
    del first
    return 0


if __name__ == "__main__":
    sys.exit(main())
