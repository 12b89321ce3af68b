#!/usr/bin/env python3
"""tools/live_filtered.py -- what k_search_query's FILTERED form (option query_wg 2, csrc/fpx_qsearch.hpp: FILT) buys a live 100 M index
whose packed group has superseded docs or masked columns.  Shapes (tools/live_index.py builds the same additions):

  (a) the group + 16 memory segments that write ~1000 of the group's docs again (half with their own hashes, half with new ones) and
      delete ~100 (tombstones): every column of the group has a dead set
  (b) (a) + the three small file segments (checkpoints) and the merged one of 2.5 M items: two parts, the filtered form on part 0
  (c) the group with two of its columns merged away and not regrouped (outside the snapshot) + the merged segment of 2.5 M items
      next to it (a stand-in: a real merge of two columns would hold their 3.2 G items, searched in part 1 by the pipeline)

Each at query_wg 0, 1 and 2 -- the value in force when the snapshot is made and while it is searched.  One batch of 8192 x 1000 in
flight, resident; every 16th query aims at a doc written in a memory segment.  One JSON line per (shape, option): ms per step, path_flags;
the last batch's results under 1 and 2 are checked byte for byte against 0's ("same_as_0").

    DOCS=100000000 python tools/live_filtered.py"""
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
    ctx = fpx.Context(0)
    docs, S, H, B = int(os.environ.get("DOCS", 100_000_000)), 16, 256, int(os.environ.get("BATCH", 8192))
    seed = 20260928
    steps = int(os.environ.get("STEPS", 40))
    t0 = time.perf_counter()
    segs, _ = bench.synth_index(fpx, ctx, seed, docs, S, H, set(range(S)))
    docs = (docs // S) * S
    opts = fpx.http_options()
    batches = [fpx.synth.make_queries(seed, 4242 + 1000003 * i, B, docs, H, query_len=1000) for i in range(4)]

    next_doc, commit = docs + 1, S + 1
    small = []
    for per in (2000, 2000, 2000):
        small.append(fpx.FileSegment.synth(ctx, seed + 5, next_doc, per, H, 0, 512, commit))
        next_doc += per; commit += 1
    merged = fpx.FileSegment.synth(ctx, seed + 6, next_doc, 10000, H, 0, 512, commit)
    next_doc += 10000; commit += 1
    # 16 memory segments: fresh docs, 62 docs of the group written again (odd ones with their own hashes, even ones with new hashes),
    # 6 of the group's docs deleted
    rng = np.random.default_rng(seed)
    again = np.unique(rng.integers(1, docs + 1, 4 * 16 * 68, dtype=np.uint64))
    rng.shuffle(again)
    again = again[:16 * 68]
    first_mem_doc, per_mem = next_doc, 100_000 // H
    mems, mem_docs = [], []
    for m in range(16):
        ids = np.arange(next_doc, next_doc + per_mem, dtype=np.uint64)
        hh = fpx.synth.synth_hashes(seed + 77, ids, H, 0).astype(np.uint64)
        parts = [((hh << np.uint64(32)) | ids[:, None]).ravel()]
        re_ = np.sort(again[m * 68: m * 68 + 62])
        gone = np.sort(again[m * 68 + 62: (m + 1) * 68])
        for d in re_:
            h = fpx.synth.synth_hashes(seed if d % 2 else seed + 99, [int(d)], H, 0).astype(np.uint64)[0]
            parts.append((h << np.uint64(32)) | d)
        items = np.sort(np.concatenate(parts))
        all_ids = np.concatenate([ids, re_, gone])
        alive = np.concatenate([np.ones(len(ids) + len(re_), np.uint8), np.zeros(len(gone), np.uint8)])
        order = np.argsort(all_ids)
        mems.append(fpx.MemorySegment(ctx, items, int(all_ids.min()), int(all_ids.max()), commit, all_ids[order].astype(np.uint32), alive[order]))
        mem_docs.append(ids[::7])
        mem_docs.append(re_[re_ % 2 == 0])
        next_doc += per_mem; commit += 1
    mem_docs = np.concatenate(mem_docs)
    print(json.dumps({"built_s": round(time.perf_counter() - t0, 1), "docs": docs, "rewritten": 16 * 62, "deleted": 16 * 6}), flush=True)

    def seed_of(d):
        if d >= first_mem_doc:
            return seed + 77
        return seed + 99                                            # (a group doc written again with new hashes)

    def aimed(batch, extra_docs):
        f, o, t = batch[0].copy(), batch[1], batch[2].copy()
        if len(extra_docs):
            for q in range(0, B, 16):
                d = int(extra_docs[(q // 16) % len(extra_docs)])
                f[int(o[q]):int(o[q]) + H] = fpx.synth.synth_hashes(seed_of(d), [d], H, 0)[0]
                t[q] = d
        return f, o, t

    shapes = [("(a) the group + 16 memory segments: ~1000 docs written again, ~100 deleted", list(segs) + mems, mem_docs),
              ("(b) (a) + 3 small file segments + a merged one of 2.5 M items", list(segs) + small + [merged] + mems, mem_docs),
              ("(c) the group, two columns merged away (no regroup) + a merged segment of 2.5 M items", list(segs[2:]) + [merged], np.zeros(0))]
    only = os.environ.get("SHAPES")
    for si, (label, members, extra_docs) in enumerate(shapes):
        if only is not None and str(si) not in only.split(","):
            continue
        qs = [aimed(b, extra_docs) for b in batches]
        qbs = [fpx.QueryBatch(ctx, options=opts, flat=(f, o)) for f, o, _ in qs]
        ref = None
        for qwg in (0, 1, 2):
            ctx.set_option("query_wg", qwg)
            snap = fpx.Segments(ctx, members)
            reader = fpx.IndexReader(snap)
            dt, agg, out, out_n = bench.timed_resident(fpx, reader, qbs, steps, 16)
            last = qs[(16 + steps - 1) % len(qs)]
            found = int(sum(1 for q in range(B) if out_n[q] > 0 and out[q, 0, 0] == last[2][q]))
            res = [out[q, :int(out_n[q])].tobytes() for q in range(B)]
            if qwg == 0:
                ref = res
            print(json.dumps({"shape": label, "query_wg": qwg, "ms_per_step": round(dt / steps * 1e3, 4), "queries_per_s": round(B * steps / dt),
                              "gpu_ms_per_step": round(agg.v["total_gpu_ms"] / steps, 4), "path_flags": agg.path_flags,
                              "same_as_0": res == ref, "targets_found": found, "of": B}), flush=True)
            del reader
            snap.release()
        ctx.set_option("query_wg", -1)
        for q_ in qbs:
            q_.release()


if __name__ == "__main__":
    main()
