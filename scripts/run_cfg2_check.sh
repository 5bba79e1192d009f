python -m pytest tests/test_gpu_train.py tests/test_gpu_dp.py tests/test_gpu_fpn.py -x -q > gpurun_out/r04l_tests.log 2>&1; echo rc=$?; tail -4 gpurun_out/r04l_tests.log
for i in 1 2; do python bench.py --full --config 2 --steps 20 --warmup 5 2>/dev/null | tail -1 | python -c "
import json, sys
d=json.load(sys.stdin); print(d['value'], d['ms_per_step'], d['roofline']['frac'], d['kernel_ms_per_step'])"; done
bash scripts/prof_stats.sh r04l 2 > /dev/null 2>&1
python scripts/kstats.py gpurun_out/r04l_cfg2_kernel_stats.csv 7 22
