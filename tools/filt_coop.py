#!/usr/bin/env python3
"""tools/filt_coop.py -- what option filt_coop (csrc/fpx_qsearch.hpp: k_search_filt, the filtered walk eight lanes to a line behind the
group's union dead-set bitmap) buys a live 100 M index whose packed group has superseded docs or masked columns, next to the filtered
k_search_query (the per-lane walk) that query_wg = 2 runs without it.  The three shapes of tools/live_filtered.py, built the same way:

  (a) the group + 16 memory segments that write ~1000 of the group's docs again and delete ~100: every column has a dead set
  (b) (a) + three small file segments (checkpoints) and a merged one: two parts, the filtered form on part 0
  (c) the group with two of its columns merged away and not regrouped + a merged segment next to it: masked columns, no dead set

Each at query_wg = 2 with filt_coop 0 and 1 ALTERNATING, three runs each in one process -- the value in force when the snapshot is made
and while it is searched.  One batch of 8192 x 1000 in flight, resident; every 16th query aims at a doc written in a memory segment.
One JSON line per run: ms per step, GPU ms per step, path_flags, the bitmap's bytes; the last batch's results under 1 are compared byte
for byte with those under 0 and with query_wg = 0 ("same_as_filt_coop_0", "same_as_query_wg_0").

THE BASELINE THAT COUNTS is the parent commit's library under query_wg = 2, in the same session: run this tool with FPX_LIB naming that
library first -- a library without the option runs query_wg = 2 alone, three times ("filt_coop": null) -- and keep its output; then run
it on this build with AGAINST=<that output>: per shape a verdict by DESIGN 4.0's rule, a gain only when EVERY run of the new form is below
EVERY run of the baseline by more than both spreads together.

    DOCS=100000000 FPX_LIB=.../libfpx_parent.so python tools/filt_coop.py > parent.txt
    DOCS=100000000 AGAINST=parent.txt python tools/filt_coop.py"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RUNS = 3


def verdict(new, base):
    """a gain only when every run of `new` is below every run of `base` by more than both spreads together"""
    spread = (max(new) - min(new)) + (max(base) - min(base))
    if max(new) + spread < min(base):
        return "gain"
    if min(new) - spread > max(base):
        return "loss"
    return "within the spreads"


def main():
    import torch  # noqa: F401  (one HIP runtime in the process: torch's, loaded first)
    import bench
    from __graft_entry__ import load_package
    fpx = load_package()
    ctx = fpx.Context(0)
    try:
        ctx.set_option("filt_coop", -1)
        levels = (0, 1)
    except fpx.FpxError:                                         # (a library from before the option: the baseline)
        levels = (None,)
    lib = os.path.basename(os.environ.get("FPX_LIB", "libfpx.so"))
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
    # 6 of the group's docs deleted (tools/live_filtered.py's)
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
    print(json.dumps({"lib": lib, "built_s": round(time.perf_counter() - t0, 1), "docs": docs, "rewritten": 16 * 62, "deleted": 16 * 6,
                      "filt_coop_levels": list(levels)}), flush=True)

    def seed_of(d):
        return seed + 77 if d >= first_mem_doc else seed + 99      # (else: a group doc written again with new hashes)

    def aimed(batch, extra_docs):
        f, o, t = batch[0].copy(), batch[1], batch[2].copy()
        if len(extra_docs):
            for q in range(0, B, 16):
                d = int(extra_docs[(q // 16) % len(extra_docs)])
                f[int(o[q]):int(o[q]) + H] = fpx.synth.synth_hashes(seed_of(d), [d], H, 0)[0]
                t[q] = d
        return f, o, t

    against = {}
    if os.environ.get("AGAINST"):
        for ln in open(os.environ["AGAINST"]):
            ln = ln.strip()
            if ln.startswith("{") and '"run"' in ln:
                r = json.loads(ln)
                if r.get("query_wg") == 2 and r.get("filt_coop") in (None, 0):
                    against.setdefault(r["shape"][:3], []).append(r)

    shapes = [("(a) the group + 16 memory segments: ~1000 docs written again, ~100 deleted", list(segs) + mems, mem_docs),
              ("(b) (a) + 3 small file segments + a merged one of 2.5 M items", list(segs) + small + [merged] + mems, mem_docs),
              ("(c) the group, two columns merged away (no regroup) + a merged segment of 2.5 M items", list(segs[2:]) + [merged], np.zeros(0))]
    only = os.environ.get("SHAPES")
    for si, (label, members, extra_docs) in enumerate(shapes):
        if only is not None and str(si) not in only.split(","):
            continue
        qs = [aimed(b, extra_docs) for b in batches]
        qbs = [fpx.QueryBatch(ctx, options=opts, flat=(f, o)) for f, o, _ in qs]
        last = qs[(16 + steps - 1) % len(qs)]

        def run(qwg, fc):
            ctx.set_option("query_wg", qwg)
            if fc is not None:
                ctx.set_option("filt_coop", fc)
            snap = fpx.Segments(ctx, members)
            reader = fpx.IndexReader(snap)
            dt, agg, out, out_n = bench.timed_resident(fpx, reader, qbs, steps, 16)
            found = int(sum(1 for q in range(B) if out_n[q] > 0 and out[q, 0, 0] == last[2][q]))
            res = [out[q, :int(out_n[q])].tobytes() for q in range(B)]
            rec = {"lib": lib, "shape": label, "query_wg": qwg, "filt_coop": fc, "ms_per_step": round(dt / steps * 1e3, 4),
                   "gpu_ms_per_step": round(agg.v["total_gpu_ms"] / steps, 4), "path_flags": agg.path_flags,
                   "dead_union_bytes": snap.info().get("dead_union_bytes", 0), "targets_found": found, "of": B}
            del reader
            snap.release()
            return rec, res

        rec0, ref0 = run(0, None if levels == (None,) else 0)
        print(json.dumps(rec0), flush=True)
        by_level, res_of = {fc: [] for fc in levels}, {}
        for r in range(RUNS):
            for fc in levels:
                rec, res = run(2, fc)
                rec["run"] = r
                rec["same_as_query_wg_0"] = res == ref0
                if fc == 1:
                    rec["same_as_filt_coop_0"] = res == res_of.get(0)
                res_of[fc] = res
                by_level[fc].append(rec)
                print(json.dumps(rec), flush=True)
        ctx.set_option("query_wg", -1)
        if levels != (None,):
            ctx.set_option("filt_coop", -1)
            for key in ("ms_per_step", "gpu_ms_per_step"):
                new, own = [r[key] for r in by_level[1]], [r[key] for r in by_level[0]]
                line = {"shape": label[:3], "figure": key, "filt_coop_1": new, "filt_coop_0": own, "against_filt_coop_0": verdict(new, own)}
                if against.get(label[:3]):
                    base = [r[key] for r in against[label[:3]]]
                    line.update({"baseline": base, "baseline_lib": against[label[:3]][0]["lib"], "against_baseline": verdict(new, base),
                                 "filt_coop_0_against_baseline": verdict(own, base)})
                print(json.dumps(line), flush=True)
        for q_ in qbs:
            q_.release()


if __name__ == "__main__":
    main()
