#!/bin/bash
# tools/pmc_tcp.sh -- the vector-memory front end's ACCESSES of k_search_query and of the calibration kernels (k_bw_pattern<MODE>, k_bw_*):
# one counter pass per library over the headline batch (bench.py --pmc-child), TCP_TOTAL_CACHE_ACCESSES_sum and TCP_TCC_READ_REQ_sum and
# nothing else, with the kernel trace of the same pass for the times.  Per kernel (its last dispatch): accesses per launch, accesses per
# second, read requests to the L2 -- and, for k_search_query, accesses per query hash (HASHES: the batch's hashes, default 8192 x 1000).
# VARIANTS="base <name> ..." as in tools/qs_ab.sh (base = the product, the others acoustid-index_amd/build/exp/libfpx_<name>.so).
# Every GPU step runs under its own time limit and the script stops at the first one that fails.  Output: PMC_TCP_OUT/tcp.txt (default
# acoustid-index_amd/build/pmc_tcp: not tracked).  PMC_TCP_KEEP_HEADS=1 keeps the first lines of the profiler's CSV files next to it.
set -u
cd "$(dirname "$0")/.."
R=$(pwd)
O=${PMC_TCP_OUT:-$R/acoustid-index_amd/build/pmc_tcp}
mkdir -p "$O"
: > "$O/tcp.txt"
lib_of() { if [ "$1" = base ]; then echo "$R/acoustid-index_amd/libfpx.so"; else echo "$R/acoustid-index_amd/build/exp/libfpx_$1.so"; fi; }
step() { "$@"; local rc=$?; if [ $rc -ne 0 ]; then echo "pmc_tcp: step failed (exit status $rc), stopping: $*" | tee -a "$O/tcp.txt"; exit $rc; fi; }
for v in ${VARIANTS:-base}; do
  [ -f "$(lib_of $v)" ] || { echo "pmc_tcp: no library for variant $v"; exit 2; }
  rm -rf "$O/pmc_$v"
  FPX_LIB="$(lib_of $v)" timeout -k 10 400 rocprofv3 --kernel-trace --pmc ${PMC_TCP_COUNTERS:-TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum} --output-format csv -d "$O/pmc_$v" -o pmc -- \
    python "$R/bench.py" --pmc-child --steps 2 --warmup 2 > "$O/pmc_$v.log" 2>&1; rc=$?
  if [ $rc -ne 0 ]; then echo "pmc_tcp: the counter pass of $v failed (exit status $rc), stopping" | tee -a "$O/tcp.txt"; tail -5 "$O/pmc_$v.log"; exit $rc; fi
  step python - "$v" "$O/pmc_$v" "${HASHES:-8192000}" > "$O/part.txt" <<'PY'
import collections, csv, glob, sys
v, d, hashes = sys.argv[1], sys.argv[2], float(sys.argv[3])
want = ("k_search_query", "k_bw_")
ctr = collections.defaultdict(lambda: collections.defaultdict(float))
name, ns = {}, {}
for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if any(w in r["Kernel_Name"] for w in want):
            i = int(r["Dispatch_Id"])
            ctr[i][r["Counter_Name"]] += float(r["Counter_Value"])
            name[i] = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("fpx::", "")
            if r.get("Start_Timestamp") and r.get("End_Timestamp"):
                ns[i] = float(r["End_Timestamp"]) - float(r["Start_Timestamp"])
for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        i = int(r["Dispatch_Id"])
        if i in ctr:
            ns[i] = float(r["End_Timestamp"]) - float(r["Start_Timestamp"])
last = {}
for i in sorted(ctr):
    last[name[i]] = i
print("%s: last dispatch of each kernel; counters %s" % (v, " ".join(sorted({c for i in ctr for c in ctr[i]}))))
for k, i in sorted(last.items()):
    acc = next((x for c, x in ctr[i].items() if "TCC_READ_REQ" not in c), 0.0)
    rd = ctr[i].get("TCP_TCC_READ_REQ_sum", 0.0)
    ms = ns.get(i, 0.0) / 1e6
    line = "%s %-44s %8.4f ms  accesses %9.3f M  %7.2f G/s  read requests to L2 %9.3f M" % (v, k, ms, acc / 1e6, acc / ms / 1e6 if ms else 0.0, rd / 1e6)
    if "k_search_query" in k:
        line += "  per query hash: %.3f accesses, %.3f read requests" % (acc / hashes, rd / hashes)
    print(line)
PY
  tee -a "$O/tcp.txt" < "$O/part.txt"
  [ -n "${PMC_TCP_KEEP_HEADS:-}" ] && for f in $(find "$O/pmc_$v" -name "*.csv"); do echo "== $f"; head -3 "$f"; done > "$O/heads_$v.txt"
  rm -rf "$O/pmc_$v"
done
