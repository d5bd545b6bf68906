#!/bin/bash
# conv_h8 vs conv_halo<2,2,4,3,3> on HRNet's 128- and 256-channel 3x3 shapes: timing, then PMC
set -o pipefail
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
out=gpurun_out/${1:-h8pmc}; mkdir -p $out
for h in 1 0 1 0; do  # DVIE_CONV_H8=0: the 4-row halo kernel takes these convs
  DVIE_CONV_H8=$h timeout -k 10 200 python -u tools/conv_tune.py 20 '128->128|256->256' > $out/tune_h8$h.txt 2>&1 || { tail -20 $out/tune_h8$h.txt; exit 1; }
  echo "DVIE_CONV_H8=$h"; cat $out/tune_h8$h.txt
done
for h in 1 0; do
  DVIE_CONV_H8=$h PMC_RX="conv_h8_kernel|conv_halo_kernel" PMC_CMD="python3 tools/conv_tune.py 5 128->128|256->256" bash tools/pmc_kernels.sh ${1:-h8pmc}/pmc_h8$h
done
timeout -k 10 300 python -u -m pytest -x -q --timeout 120 --timeout-method thread tests/test_gpu_parity.py -k warp > $out/pytest_warp.log 2>&1 \
  || { tail -30 $out/pytest_warp.log; exit 1; }
tail -2 $out/pytest_warp.log
