#!/bin/bash
# usage: tools/pmc.sh <tag> <counters...>   (runs on the GPU box via gpurun)
tag=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
O=${PMC_OUT:-/tmp/pmc}                # the counter CSVs under $O/<tag>/, the run's output in $O/<tag>.log
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --pmc "$@" --output-format csv -d $O/$tag -o $tag -- python $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-latency --docs ${PMC_DOCS:-16000000} > $O/$tag.log 2>&1
