#!/bin/bash
# tools/qs_ab.sh -- A/B of k_search_query builds on ONE box, the libraries ALTERNATING: VARIANTS="base <name> ..." (base = the product, the
# others acoustid-index_amd/build/exp/libfpx_<name>.so from tools/build_variant.sh or a copy of another commit's library) x RUNS (3) x two
# settings of the headline batch -- one batch in flight (`--inflight 1`: roofline.avg_launch_ms is the kernel's time) and the plain bench.py
# line (its default batches in flight: value, ms_per_step).  TESTS=1 (default): the kernel's parity tests first.  A variant that has a
# sibling libfpx_<name>_prof.so (built with -DFPX_QS_PROF=1) prints its clocks per query and phase before the runs.  PMC=1: the memory-side
# read requests of the kernel per launch afterwards, counters in a run of their own.
# Every GPU step runs under its own time limit and the script stops at the first one that fails: nothing is started on a device after a
# fault, an abort or a timeout.  Every run is a line of runs.txt in the output directory (QS_AB_OUT, default acoustid-index_amd/build/qs_ab:
# not tracked).
set -u
cd "$(dirname "$0")/.."
R=$(pwd)
O=${QS_AB_OUT:-$R/acoustid-index_amd/build/qs_ab}
mkdir -p $O
: > $O/runs.txt
lib_of() { if [ "$1" = base ]; then echo $R/acoustid-index_amd/libfpx.so; else echo $R/acoustid-index_amd/build/exp/libfpx_$1.so; fi; }
step() { "$@"; local rc=$?; if [ $rc -ne 0 ]; then echo "qs_ab: step failed (exit status $rc), stopping: $*" | tee -a $O/runs.txt; exit $rc; fi; }
if [ "${TESTS:-1}" = 1 ]; then
  timeout -k 10 900 python -m pytest tests/test_gpu_query_wg.py tests/test_gpu_query_wg_words.py -x -q > $O/tests.txt 2>&1; rc=$?
  tail -5 $O/tests.txt
  [ $rc -eq 0 ] || { echo "qs_ab: the parity tests failed (exit status $rc), stopping"; exit $rc; }
fi
for v in ${VARIANTS:-base}; do
  [ -f "$(lib_of $v)" ] || { echo "qs_ab: no library for variant $v"; exit 2; }
  p=$R/acoustid-index_amd/build/exp/libfpx_${v}_prof.so
  if [ -f $p ]; then
    FPX_LIB=$p step timeout -k 10 ${BENCH_TIMEOUT:-200} python bench.py --gpus 1 --steps 20 --warmup 3 --inflight 1 > $O/${v}_prof.json 2> $O/${v}_prof.err
    echo "$v $(grep qs_prof $O/${v}_prof.err | tail -1)" | tee -a $O/runs.txt
  fi
done
for i in $(seq 1 ${RUNS:-3}); do
  for v in ${VARIANTS:-base}; do
    for nfl in 1 0; do
      extra=""; [ $nfl = 1 ] && extra="--inflight 1"
      FPX_LIB=$(lib_of $v) step timeout -k 10 ${BENCH_TIMEOUT:-200} python bench.py --gpus 1 --steps ${STEPS:-20} --warmup 3 $extra > $O/${v}_r${i}_nfl${nfl}.json 2> $O/${v}_r${i}_nfl${nfl}.err
      step python - "$v" "$i" "$O/${v}_r${i}_nfl${nfl}.json" > $O/line.txt <<'PY'
import json, sys
v, i, path = sys.argv[1:4]
r = json.loads(open(path).read().strip().splitlines()[-1])
print(v, "run", i, "inflight", r["inflight"], "value %.0f" % r["value"], "ms_per_step %.4f" % r["ms_per_step"], "kernel_ms %.4f" % r["roofline"]["avg_launch_ms"],
      "found", r["targets_found"], r["roofline"]["kernel"], "hits", r["hits_per_step"])
PY
      tee -a $O/runs.txt < $O/line.txt
    done
  done
done
if [ "${PMC:-0}" = 1 ]; then
  # memory-side requests of k_search_query per launch (the counters and the child of bench.py's own pass), no tracing alongside
  for v in ${VARIANTS:-base}; do
    rm -rf $O/pmc_$v
    FPX_LIB=$(lib_of $v) step timeout -k 10 400 rocprofv3 --pmc TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_128B_sum TCC_EA0_WRREQ_sum TCC_EA0_WRREQ_64B_sum --output-format csv -d $O/pmc_$v -o pmc -- \
      python $R/bench.py --pmc-child --steps 2 --warmup 2 > $O/pmc_$v.log 2>&1
    step python - "$v" "$O/pmc_$v" > $O/line.txt <<'PY'
import collections, csv, glob, sys
v, d = sys.argv[1:3]
agg = collections.defaultdict(lambda: collections.defaultdict(float))
for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if "k_search_query" in r["Kernel_Name"]:
            agg[int(r["Dispatch_Id"])][r["Counter_Name"]] += float(r["Counter_Value"])
c = agg[max(agg)]
print(v, "k_search_query, last launch: read requests %.3f M (128-byte: %.3f M), write requests %.3f M" % (c["TCC_EA0_RDREQ_sum"] / 1e6, c["TCC_EA0_RDREQ_128B_sum"] / 1e6, c["TCC_EA0_WRREQ_sum"] / 1e6))
PY
    tee -a $O/runs.txt < $O/line.txt
    rm -rf $O/pmc_$v
  done
fi
