#!/bin/bash
# full GPU test suite + the full bench line (bench.py --full), summarised on stdout
cd /root/repo; mkdir -p gpurun_out
timeout 2400 python -m pytest tests -m gpu -x -q 2>&1 | tail -8 > gpurun_out/pytest_gpu.txt; cat gpurun_out/pytest_gpu.txt
python bench.py --full 2> >(tail -3 >&2) | tail -1 | python -c "
import json, sys
d=json.loads(sys.stdin.read()); print(d['ms_per_step'], d['achieved_tflops_attn_ffn'], d['frac_mfma_peak_attn_ffn'], 'eager', d['eager_ms_per_step']); [print('   ',k['kernel'],k['avg_ms'],k['tflops']) for k in d['kernels']]
for k in ('roofline','vae_decode','b1','train','cpu_baseline','lib'): print(k, json.dumps(d.get(k))[:600])
"
