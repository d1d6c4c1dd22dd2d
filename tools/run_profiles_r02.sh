#!/bin/bash
# Round-2 profiles.  Run on the GPU box (via gpurun):  tools/run_profiles_r02.sh [tag]
#   kt        rocprofv3 --kernel-trace --stats of the bench.py --full run (C2 headline + C3 / C5 extras)
#   pmc_*     separate --pmc passes (SQ set, FETCH_SIZE, WRITE_SIZE) over small fixed workloads
# Summarise with tools/summarize_profiles_r02.py <tag> -> profiles/<tag>_*
set -e
tag=${1:-r02}
export TMPDIR=/tmp
R=$PWD/gpurun_out/prof_$tag
rm -rf $R
mkdir -p $R
rocprofv3 --kernel-trace --stats --output-format csv -d $R/kt -- python3 bench.py --full --no-cpu-baseline > $R/kt.log 2>&1
tail -c 400 $R/kt.log | head -c 300; echo
SQ="SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_WAIT_ANY"
for w in workload c3 c5; do
  rocprofv3 --pmc $SQ --output-format csv -d $R/pmc_sq_$w -- python3 tools/profile_$w.py > $R/pmc_sq_$w.log 2>&1
  rocprofv3 --pmc FETCH_SIZE --output-format csv -d $R/pmc_fetch_$w -- python3 tools/profile_$w.py > $R/pmc_fetch_$w.log 2>&1
  rocprofv3 --pmc WRITE_SIZE --output-format csv -d $R/pmc_write_$w -- python3 tools/profile_$w.py > $R/pmc_write_$w.log 2>&1
  echo "pmc $w done"
done
echo profiles done
