#!/usr/bin/env python3
"""tools/low_wg_coop.py -- what option low_wg = 3 (k_search_low_coop, csrc/fpx_qsearch.hpp: k_search_filt's rounds and tasks -- eight lanes
to a line behind the group's union dead-set bitmap -- with k_search_low's sorted tail) buys on traffic with score floors of 1 and 2 on a
LIVE index, next to low_wg = 2 (k_search_low_filt: the per-lane walk).  Round 16's shape, built as tools/low_wg_filtered.py builds it: the
100 M index (bench.py's: 16 synthetic segments, one packed group) + 16 memory segments that write 992 of its docs again (half with their
own hashes, half with new ones) and delete 96 -- every column of the group has a dead set.  Resident batches of 8192 queries of 1000
hashes, one batch in flight, every 16th query aimed at a doc written in a memory segment.  The four mixes of tools/low_wg.py: every query
with the legacy protocol's options (min_score 1, min_score_pct 10, limit 500); 1 % and 10 % of the queries with them and the rest HTTP
defaults; every query with min_score 1, min_score_pct 0, limit 100.

One process of THIS BUILD: the snapshot is made once under query_wg = 2, filt_coop = 1 (it holds the union bitmap); per mix the batch runs
under query_wg = 0 (the pipeline: the reference results), then under low_wg 2 and 3 ALTERNATING, RUNS (3) runs each of STEPS (40) batches
after a warm-up.  One JSON line per (mix, low_wg, run): ms per step, the GPU time of the calls, how many steps ran which kernel
(path_flags bits 12, 8 and 16), and whether the last batch's results are byte for byte those under query_wg = 0 and under low_wg = 2.
Then ONE process of the PARENT commit's library (PARENT_LIB=path/to/its/libfpx.so, loaded through FPX_LIB) at low_wg = 2, the same runs:
k_search_low_filt before this change, and the baseline that counts.  Every process runs under a time limit; the driver stops at the first
that fails.  At the end a verdict per mix and figure by DESIGN 4.0's rule (round 9's): a gain or a loss only where every run of one side
lies beyond every run of the other by more than both spreads together, else "inside the margin" -- low_wg 3 against the parent's low_wg 2,
low_wg 3 against this build's low_wg 2, and this build's low_wg 2 against the parent's (did k_search_low_filt move?).

    PARENT_LIB=/path/to/parent/libfpx.so DOCS=100000000 python tools/low_wg_coop.py"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KEEP = os.path.join(ROOT, "acoustid-index_amd", "build", "low_wg_coop")
MIXES = ["legacy 100 %", "legacy 1 %", "legacy 10 %", "min_score 1, pct 0, limit 100"]
LOW, FILTERED, COOP, QUERY_WG = 4096, 256, 65536, 64


def child(which):
    import torch  # noqa: F401  (one HIP runtime in the process: torch's, loaded first)
    import bench
    from __graft_entry__ import load_package
    fpx = load_package()
    synth = fpx.synth
    ctx = fpx.Context(0)
    docs, S, H, B = int(os.environ.get("DOCS", 100_000_000)), 16, 256, int(os.environ.get("BATCH", 8192))
    seed, steps, runs = 20260928, int(os.environ.get("STEPS", 40)), int(os.environ.get("RUNS", 3))
    levels = (2,) if which == "parent" else (2, 3)
    t0 = time.perf_counter()
    segs, _ = bench.synth_index(fpx, ctx, seed, docs, S, H, set(range(S)))
    docs = (docs // S) * S
    # tools/live_filtered.py's 16 memory segments: fresh docs, 62 docs of the group written again each (odd ones with their own hashes,
    # even ones with new hashes), 6 of the group's docs deleted each
    next_doc, commit = docs + 1, S + 1
    rng = np.random.default_rng(seed)
    again = np.unique(rng.integers(1, docs + 1, 4 * 16 * 68, dtype=np.uint64))
    rng.shuffle(again)
    again = again[:16 * 68]
    first_mem_doc, per_mem = next_doc, 100_000 // H
    mems, mem_docs = [], []
    for m in range(16):
        ids = np.arange(next_doc, next_doc + per_mem, dtype=np.uint64)
        hh = synth.synth_hashes(seed + 77, ids, H, 0).astype(np.uint64)
        parts = [((hh << np.uint64(32)) | ids[:, None]).ravel()]
        re_ = np.sort(again[m * 68: m * 68 + 62])
        gone = np.sort(again[m * 68 + 62: (m + 1) * 68])
        for d in re_:
            h = synth.synth_hashes(seed if d % 2 else seed + 99, [int(d)], H, 0).astype(np.uint64)[0]
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
    ctx.set_option("query_wg", 2)
    ctx.set_option("filt_coop", 1)                                 # (in force when the snapshot is made: the union bitmap)
    snap = fpx.Segments(ctx, list(segs) + mems)
    reader = fpx.IndexReader(snap)
    print(json.dumps({"library": which, "built_s": round(time.perf_counter() - t0, 1), "docs": docs, "rewritten": 16 * 62, "deleted": 16 * 6,
                      "dead_union_bytes": snap.info().get("dead_union_bytes", 0), "low_wg_levels": list(levels),
                      "lib": os.path.basename(os.environ.get("FPX_LIB", "the tree's"))}), flush=True)
    http, legacy = fpx.http_options(), fpx.SearchOptions(max_results=500, min_score=1, min_score_pct=10)
    flat_cut = fpx.SearchOptions(max_results=100, min_score=1, min_score_pct=0)
    mixes = list(zip(MIXES, [legacy, legacy, legacy, flat_cut], [1.0, 0.01, 0.1, 1.0]))
    only = os.environ.get("MIXES")
    os.makedirs(KEEP, exist_ok=True)
    rng = np.random.default_rng(16)
    for m, (label, low_opts, share) in enumerate(mixes):
        picks = [rng.choice(B, max(1, int(round(share * B))), replace=False) for _ in range(2)]       # (drawn whether the mix runs or not)
        if only and str(m) not in only.split(","):
            continue
        qbs, targets = [], []
        for i in range(2):
            f, o, t = synth.make_queries(seed, 4242 + 1000003 * i, B, docs, H, query_len=1000)
            f, t = np.ascontiguousarray(f).copy(), t.copy()
            for q in range(0, B, 16):                              # every 16th query: a doc written in a memory segment
                d = int(mem_docs[(q // 16) % len(mem_docs)])
                f[int(o[q]):int(o[q]) + H] = synth.synth_hashes(seed + 77 if d >= first_mem_doc else seed + 99, [d], H, 0)[0]
                t[q] = d
            is_low = np.zeros(B, dtype=bool)
            is_low[picks[i]] = True
            qbs.append(fpx.QueryBatch(ctx, options=[low_opts if x else http for x in is_low], flat=(f, o)))
            targets.append(t)

        def run(query_wg, low_wg):
            ctx.set_option("query_wg", query_wg)
            ctx.set_option("low_wg", low_wg)
            out = out_n = None
            for i in range(8):                                     # (a path's first batches size its buffers)
                out, out_n, _ = fpx.search_resident(reader, qbs[i % 2], 0, out, out_n)
            gpu_ms = hits = 0.0
            on = {"k_search_low_coop": 0, "k_search_low_filt": 0, "k_search_filt": 0, "query_per_workgroup": 0}
            t_r = time.perf_counter()
            for i in range(steps):
                out, out_n, st = fpx.search_resident(reader, qbs[i % 2], 0, out, out_n)
                gpu_ms += st.total_gpu_ms; hits += st.hits
                pf = st.path_flags
                on["k_search_low_coop"] += 1 if pf & (LOW | COOP) == (LOW | COOP) else 0
                on["k_search_low_filt"] += 1 if pf & (LOW | FILTERED | COOP) == (LOW | FILTERED) else 0
                on["k_search_filt"] += 1 if pf & (LOW | COOP) == COOP else 0
                on["query_per_workgroup"] += 1 if pf & QUERY_WG else 0
            dt = time.perf_counter() - t_r
            t = targets[(steps - 1) % 2]
            used = b"".join(out[q, :out_n[q]].tobytes() for q in range(B)) + np.asarray(out_n[:B], dtype=np.uint32).tobytes()
            rec = {"library": which, "mix": label, "query_wg": query_wg, "low_wg": low_wg, "ms_per_step": round(dt / steps * 1e3, 4),
                   "gpu_ms_per_step": round(gpu_ms / steps, 4), "steps": steps, "steps_by_kernel": on, "records_per_batch": round(hits / steps),
                   "results_per_query": round(float(out_n[:B].mean()), 2),
                   "targets_found": int(sum(1 for q in range(B) if out_n[q] > 0 and out[q, 0, 0] == t[q])), "of": B}
            return rec, used

        kept = os.path.join(KEEP, f"mix{m}.bin")
        if which == "parent":                                      # (the reference: this build's results under query_wg = 0)
            with open(kept, "rb") as fh:
                ref0 = fh.read()
        else:
            rec0, ref0 = run(0, 0)
            print(json.dumps(rec0), flush=True)
            with open(kept, "wb") as fh:
                fh.write(ref0)
        used_of = {}
        for r in range(runs):
            for lw in levels:                                      # 2, 3, 2, 3, ...
                rec, used = run(2, lw)
                rec["run"] = r
                rec["same_as_query_wg_0"] = used == ref0
                if lw == 3:
                    rec["same_as_low_wg_2"] = used == used_of.get(2)
                used_of[lw] = used
                print(json.dumps(rec), flush=True)
        ctx.set_option("low_wg", -1)
        for q_ in qbs:
            q_.release()


def verdict(new, base):
    """DESIGN 4.0 (round 9's rule) on two lists of a figure: `new` against `base`"""
    both = (max(new) - min(new)) + (max(base) - min(base))
    if max(new) < min(base) - both:
        return "gain"
    if min(new) > max(base) + both:
        return "slower"
    return "inside the margin"


def main():
    parent = os.environ.get("PARENT_LIB")
    if not parent or not os.path.exists(parent):
        sys.exit("PARENT_LIB: the parent commit's libfpx.so (the baseline)")
    limit = int(os.environ.get("RUN_TIMEOUT", 540))
    os.makedirs(KEEP, exist_ok=True)
    for f in os.listdir(KEEP):
        os.remove(os.path.join(KEEP, f))
    rows = {}
    for which in ("this build", "parent"):
        env = dict(os.environ)
        if which == "parent":
            env["FPX_LIB"] = parent
        else:
            env.pop("FPX_LIB", None)
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", which],
                           env=env, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout); sys.stdout.flush()
        if p.returncode != 0:                                      # (nothing more is started on the device after a failure)
            sys.exit(f"low_wg_coop: the process of {which} failed (exit status {p.returncode}), stopping")
        for line in p.stdout.splitlines():
            row = json.loads(line)
            if "run" in row:
                rows.setdefault(row["mix"], {}).setdefault((which, row["low_wg"]), []).append(row)
                if not row["same_as_query_wg_0"] or row.get("same_as_low_wg_2") is False:
                    sys.exit(f"low_wg_coop: {which}, low_wg {row['low_wg']}, run {row['run']}, mix {row['mix']}: results differ")
    for mix, by in rows.items():
        for key in ("ms_per_step", "gpu_ms_per_step"):
            new, own, base = ([r[key] for r in by[k]] for k in (("this build", 3), ("this build", 2), ("parent", 2)))
            print(json.dumps({"mix": mix, "figure": key, "low_wg_3": new, "low_wg_2": own, "parent_low_wg_2": base,
                              "low_wg_3_against_parent_low_wg_2": verdict(new, base), "low_wg_3_against_low_wg_2": verdict(new, own),
                              "low_wg_2_against_parent_low_wg_2": verdict(own, base)}), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
