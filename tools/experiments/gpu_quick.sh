# quick check: GPU tests of the touched stage + the headline bench without side legs
set -o pipefail
mkdir -p gpurun_out
timeout -k 10 300 python -u -m pytest tests -x -q --timeout 120 --timeout-method thread -m gpu > gpurun_out/q_t.log 2>&1 &&
O=${FT8_OUT:-out} && mkdir -p $O &&   # the bench log's directory
timeout -k 10 300 python -u bench.py --full --no-cpu --no-h2d --no-subtract --no-drift --no-bp-stress > $O/q_b.log 2> $O/q_b.err
