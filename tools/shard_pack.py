#!/usr/bin/env python3
"""tools/shard_pack.py -- what option shard_pack buys a rank of an index sharded by HASH WINDOWS, next to shard_wg alone and to the
pipeline: tools/shard_wg.py's set-up -- on one GPU this process plays rank 0 of WORLDS (2, 4, 8) of the headline's index (bench.py's: DOCS
docs in 16 synthetic segments of 256 hashes per doc), its window slices ONE packed group, the batch resident: BATCH (8192) queries of
1000 hashes, the WHOLE batch as fpx_shard_probe wants it, two batches in rotation.  Timed: fpx_shard_probe alone, THREE levels
ALTERNATING in one process, RUNS (3) runs each, STEPS (40) calls per run after a warm-up:
    shard_wg 0                   the pipeline: the window's keys made, ordered and probed
    shard_wg 1                   k_search_window: a query per workgroup, a lane per query HASH and round
    shard_wg 1 + shard_pack 1    k_search_packed: the window's first occurrences packed before the rounds, a lane per PROBE
One JSON line per run: ms per call (host clock around calls that end in a synchronise), the events around the walk's kernel per call
(fpx_stats.probe_kernel_ms: under shard_wg 0 k_probe_pgroup and k_probe_memtab without the key kernels and k_bin, under 1 the one
kernel), how many calls set path_flags bit 14 (calls_walked) and bit 15 (calls_packed).  After the timed runs ONE comparison per world:
the same batch under all three -- every bin's records, nulls dropped and sorted, the travelling counts and the four statistics must be
equal.

FPX_LIB=path/to/another/libfpx.so loads another build (PLAIN_ONLY=1 times its fpx_shard_probe with no option touched, the same shapes,
for a baseline from a library that knows neither option).

    DOCS=100000000 python tools/shard_pack.py"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bins_sorted(torch, send, counts, cell_cap):
    """every bin's records sorted, nulls (and the places behind the bin's count) as the largest value: [bins, places]; the bins' record counts"""
    c = counts.reshape(-1).to(torch.int64) & 0xFFFFFFFF
    narrow, fill = (c >> 31) != 0, c & 0x7FFFFFFF
    nb = c.numel()
    assert bool(narrow.all()) or not bool(narrow.any())
    rows = send.reshape(nb, cell_cap)
    if bool(narrow.all()):
        rows = rows.view(torch.int32).to(torch.int64) & 0xFFFFFFFF       # two records to a cell
        null = 0xFFFFFFFF
    else:
        null = -1
    places = torch.arange(rows.shape[1], device=rows.device)[None, :]
    rows = torch.where(places < fill[:, None], rows, torch.full_like(rows, null))
    # (an 8-byte record is query << 32 | doc, below 2^63: -1 becomes the largest value as an unsigned one would be)
    key = torch.where(rows == null, torch.full_like(rows, (1 << 62)), rows)
    return torch.sort(key, dim=1).values, (rows != null).sum(dim=1), narrow


def main():
    import torch
    import bench
    from __graft_entry__ import load_package
    fpx = load_package()
    synth = fpx.synth
    ctx = fpx.Context(0)
    docs, S, H, B = int(os.environ.get("DOCS", 100_000_000)), 16, 256, int(os.environ.get("BATCH", 8192))
    seed, steps, runs = 20260928, int(os.environ.get("STEPS", 40)), int(os.environ.get("RUNS", 3))
    plain_only = os.environ.get("PLAIN_ONLY") == "1"
    lib = os.path.basename(os.environ.get("FPX_LIB", "libfpx.so"))
    levels = (None,) if plain_only else ((0, 0), (1, 0), (1, 1))           # (shard_wg, shard_pack)
    per = docs // S
    docs = per * S
    http = fpx.http_options()
    batches = [synth.make_queries(seed, 4242 + 1000003 * i, B, docs, H, query_len=1000) for i in range(2)]
    for world in [int(x) for x in os.environ.get("WORLDS", "2,4,8").split(",")]:
        t0 = time.perf_counter()
        window = (None, (1 << 32) // world - 1)                       # rank 0's
        segs, _ = bench.synth_index(fpx, ctx, seed, docs, S, H, set(range(S)), window=window)
        reader = fpx.IndexReader(fpx.Segments(ctx, segs))
        info, sinfo = segs[0].group_info(), reader.snapshot.info()
        print(json.dumps({"lib": lib, "world": world, "rank": 0, "built_s": round(time.perf_counter() - t0, 1), "docs": docs,
                          "group": info and {k: info[k] for k in ("columns", "line_columns", "packed", "bytes")},
                          "snapshot": {k: sinfo[k] for k in ("groups", "packed_groups", "bytes")}}), flush=True)
        if not info or not info["packed"] or sinfo["groups"] != 1:
            print(json.dumps({"error": "rank 0's slices are not ONE packed group", "reasons": [g.layout_reason for g in segs]}), flush=True)
            return 1
        qbs = [fpx.QueryBatch(ctx, options=http, flat=(np.ascontiguousarray(f), o)) for f, o, _ in batches]
        bpr = fpx.shard_bins_per_rank(B, world)

        def set_level(level):
            if level is not None:
                ctx.set_option("shard_wg", level[0])
                ctx.set_option("shard_pack", level[1])

        # the bins' size: what the larger of the two batches needs, found before anything is timed
        cell_cap, send, counts = 1024, None, None
        for _ in range(6):
            send = torch.zeros((world, bpr, cell_cap), dtype=torch.int64, device="cuda")
            counts = torch.zeros((world, bpr), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            need = max(fpx.shard_probe(reader, qb, world, send.data_ptr(), cell_cap, counts.data_ptr())[1] for qb in qbs)
            if need == 0:
                break
            cell_cap = need
        assert need == 0
        try:
            for r in range(len(levels) * runs):                      # the three levels in turn, RUNS times
                level = levels[r % len(levels)]
                set_level(level)
                for i in range(8 if r < len(levels) else 2):         # (a path's first calls size its buffers)
                    fpx.shard_probe(reader, qbs[i % 2], world, send.data_ptr(), cell_cap, counts.data_ptr())
                probe_ms = hits = 0.0
                walked = packed = 0
                t_r = time.perf_counter()
                for i in range(steps):
                    st, need = fpx.shard_probe(reader, qbs[i % 2], world, send.data_ptr(), cell_cap, counts.data_ptr())
                    probe_ms += st.probe_kernel_ms; hits += st.hits
                    walked += 1 if st.path_flags & 16384 else 0
                    packed += 1 if st.path_flags & 32768 else 0
                dt = time.perf_counter() - t_r
                print(json.dumps({"lib": lib, "world": world, "shard_wg": level and level[0], "shard_pack": level and level[1], "run": r // len(levels), "ms_per_call": round(dt / steps * 1e3, 4),
                                  "probe_kernel_ms_per_call": round(probe_ms / steps, 4), "calls": steps, "calls_walked": walked, "calls_packed": packed,
                                  "records_per_call": round(hits / steps), "cell_cap": cell_cap}), flush=True)
            # ---- the comparison: one batch under every level, the bins record for record
            seen = {}
            for level in levels:
                set_level(level)
                send.fill_(0); counts.fill_(0)
                torch.cuda.synchronize()
                st, need = fpx.shard_probe(reader, qbs[0], world, send.data_ptr(), cell_cap, counts.data_ptr())
                torch.cuda.synchronize()
                rows, nrec, narrow = bins_sorted(torch, send, counts, cell_cap)
                seen[level] = (rows, nrec, narrow, counts.clone(), (st.scanned_blocks, st.scanned_docs, st.probes, st.hits), st.path_flags)
            if not plain_only:
                a, three = seen[levels[0]], [seen[lv] for lv in levels]
                print(json.dumps({"lib": lib, "world": world, "comparison": "shard_wg 0 | shard_wg 1 | shard_wg 1 + shard_pack 1, batch 0", "bins": int(a[1].numel()),
                                  "records": [int(x[1].sum()) for x in three], "narrow_records": [bool(x[2].all()) for x in three],
                                  "bins_equal_record_for_record": all(bool(torch.equal(a[0], x[0])) for x in three),
                                  "counts_equal": all(bool(torch.equal(a[3], x[3])) for x in three),
                                  "statistics": [x[4] for x in three], "statistics_equal": all(a[4] == x[4] for x in three),
                                  "path_flags": [x[5] for x in three]}), flush=True)
        finally:
            if not plain_only:
                ctx.set_option("shard_wg", -1)
                ctx.set_option("shard_pack", -1)
        del send, counts, seen
        for q_ in qbs:
            q_.release()
        reader.snapshot.release()
        for sg in segs:
            sg.release()
        del segs, reader
        ctx.trim()
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
