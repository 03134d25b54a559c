#!/bin/bash
# round 6's record on the final tree, one GPU call: smoke, every GPU test, the bench line, the kernel traces
# (one call, three in flight, exact fp32 one call), the PMC byte passes (greedy; configs[3]'s beam pass on the
# bench workload), the MFMA counter passes.  Each step time-limited; stops at the first failure.
t=${1:-r06g}
R=${GRAFT_REPO_ROOT:-$(pwd)}
cd $R
export PYTHONUNBUFFERED=1
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > gpurun_out/${t}_smoke.log 2>&1 || exit $?
timeout -k 10 900 python -u -m pytest tests -q -m gpu --timeout 240 --timeout-method thread -p no:cacheprovider \
  > gpurun_out/${t}_gpu_tests.log 2>&1 || exit $?
bash tools/gpu.sh bench ${t}_bench || exit $?  # the --full line
bash tools/prof_round.sh $t || exit $?
ND_GEMM_F32=1 bash tools/gpu.sh prof ${t}_exact_one_call --inflight 1 --allow-switches || exit $?
bash tools/pmc_beam.sh $t
