# GPU-box check script: [kbench] kernel microbench, parity tests, smoke, bench, [prof] rocprofv3.  Logs under $OUT (default out/).
OUT=${OUT:-out}
mkdir -p $OUT && OUT=$(cd $OUT && pwd)
export PYTHONUNBUFFERED=1
R=${GRAFT_REPO_ROOT:-$PWD}
for a in "$@"; do case $a in
  kbench) timeout 600 python tools/kernel_bench.py > $OUT/kernel_bench.log 2>&1; tail -20 $OUT/kernel_bench.log;;
  tests) timeout 900 python -m pytest tests -m gpu -q -p no:cacheprovider 2>&1 | tail -40 > $OUT/pytest_gpu.log; tail -4 $OUT/pytest_gpu.log;;
  smoke) timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; tail -2 $OUT/smoke.log;;
  bench) timeout 900 python bench.py --steps 10 --warmup 3 --full > $OUT/bench.log 2>&1; tail -2 $OUT/bench.log;;
  benchpab) timeout 900 python bench.py --steps 30 --warmup 30 --pab --full > $OUT/bench_pab.log 2>&1; tail -2 $OUT/bench_pab.log;;
  prof) (cd /tmp && export TMPDIR=/tmp && timeout 900 rocprofv3 --kernel-trace --stats -d $OUT/prof -o bench -- python $R/bench.py --steps 3 --warmup 1 --full --no-cpu-baseline > $OUT/prof.log 2>&1);;
esac; done
# PMC passes (own runs, --kernel-trace only): usage  bash tools/run_gpu_checks.sh pmc
if [ "$1" = "pmc" ]; then
  cd /tmp && export TMPDIR=/tmp
  rocprofv3 -L > $OUT/counters_list.txt 2>&1
  timeout 600 rocprofv3 --kernel-trace --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS -d $OUT/pmc1 -o pmc -- python $R/tools/pmc_probe.py > $OUT/pmc1.log 2>&1
  timeout 600 rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_LDS SQ_INSTS_SALU SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS GRBM_GUI_ACTIVE -d $OUT/pmc2 -o pmc -- python $R/tools/pmc_probe.py > $OUT/pmc2.log 2>&1
  timeout 600 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/pmc3 -o pmc -- python $R/tools/pmc_probe.py > $OUT/pmc3.log 2>&1
  timeout 600 rocprofv3 --kernel-trace --pmc WRITE_SIZE TCC_HIT_sum TCC_MISS_sum -d $OUT/pmc4 -o pmc -- python $R/tools/pmc_probe.py > $OUT/pmc4.log 2>&1
  cd $R; ls $OUT/pmc*/ | head; tail -3 $OUT/pmc1.log
fi
