"""`bench.py --gpus 1 --steps K --warmup W` without `--full`: the lean run.  It prints the contract keys and the figures of the
timed region's own HIP events, and none of the runs and checks `--full` adds after the timed region (stand-alone and
steady-state roofline runs, digests, precision check, f32-encoder run, CPU baseline, secondary rows, bs-1 row).

Like tests/test_00_rccl_gpu.py the benchmark runs as a CHILD process started before anything in the pytest process has
initialised the GPU; if something already has, the test skips and says so."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ONLY = ('bitstream_sha256_first8', 'per_rank', 'precision_check', 'symbol_mismatch_rate', 'delta_bpp', 'bpp_estimated',
             'f32_mode', 'cpu_baseline', 'bitstream_match', 'secondary', 'bs1_eval')


@pytest.mark.gpu
def test_plain_bench_run_times_the_steps_and_nothing_else(tmp_path):
    import torch
    if torch.cuda.device_count() == 0:
        pytest.skip('no HIP device')
    if torch.cuda.is_initialized():
        pytest.skip('this process has already initialised the GPU: the benchmark child process must be started first '
                    '(run the whole suite, or this file alone)')
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    out_dir = str(tmp_path / 'dump')
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--dump-outputs', out_dir]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, 'rc {}\nstdout: {}\nstderr: {}'.format(r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line['metric'] == 'images/s + bpp, Entropic-Student ResNet-50 224^2' and line['unit'] == 'images/s'
    assert line['higher_is_better'] is True and line['dtype'] == 'bf16'
    assert line['steps'] == 3 and line['warmup'] == 1 and line['n_gpus'] == 1
    assert line['value'] > 0 and line['ms_per_step'] > 0
    assert abs(line['value'] - 256 * 1e3 / line['ms_per_step']) <= 1e-6 * line['value']
    assert 1.0 < line['bpp'] < 12.0
    # the timed region's own events: the dominant kernel and the bottleneck's launches, without the runs of their own
    assert line['roofline']['kernel'] in line['kernel_rooflines'] and 0.0 < line['roofline']['frac'] < 1.0
    assert 'steady' not in line['roofline'] and 'frac_steady' not in line['roofline']
    assert 'stand_alone' not in line['bottleneck_forward'] and line['bottleneck_forward']['ms_per_batch_sum_of_its_launches'] > 0
    assert not [k for k in FULL_ONLY if k in line], [k for k in FULL_ONLY if k in line]
    assert sorted(os.listdir(out_dir)) == ['logits.npy', 'nbytes.npy', 'status.npy']
