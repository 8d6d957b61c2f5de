#!/bin/bash
# round 6, after the row-map change: time line, what the table atomics still cost (ablation)
export DESMAN_HIP_LIB=$PWD/desman_amd/lib/libdesman_hip_ab.so
{
echo "== time line"; python scripts/dbg/r06_s1_clocks.py 2>&1 | grep -E "kernel span|tables staged|load\+Gamma|four items|table atomics|before epilogue|^end"
echo "== no table atomics (dbg 36)"; DESMAN_HIP_STATS_DBG=36 python scripts/dbg/r06_s1_clocks.py 2>&1 | grep -E "kernel span"
echo "== no Esum adds (dbg 20)"; DESMAN_HIP_STATS_DBG=20 python scripts/dbg/r06_s1_clocks.py 2>&1 | grep -E "kernel span"
echo "== no draws (dbg 1)"; DESMAN_HIP_STATS_DBG=1 python scripts/dbg/r06_s1_clocks.py 2>&1 | grep -E "kernel span"
} 2>&1 | tee gpurun_out/r06_after_swz.txt
