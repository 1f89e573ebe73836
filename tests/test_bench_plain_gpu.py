"""GPU: a plain bench.py run does only what its headline figure needs - set-up, settle, warm-up, the timed steps, --dump-outputs and the
line - while --full still adds the legs that take runs of their own (host issue burst, GEMM family replay, per-kernel rooflines, the
per-kernel report).  Both at B = 4: what is checked here is which legs run, not their figures."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--settle', '2',
           '--batch', '4', *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{') and '"metric"' in l]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _headline(out):
    assert out['unit'] == 'clips/s' and out['higher_is_better'] is True and out['dtype'] == 'bf16'
    assert out['steps'] == 3 and out['warmup'] == 1 and out['hip_graph'] is True
    assert out['value'] > 0 and abs(out['value'] - 4 * 3 / (out['ms_per_step'] * 3e-3)) < 1e-2 * out['value']


def test_plain_run_runs_no_leg_of_the_full_run(tmp_path):
    out = _bench('--dump-outputs', str(tmp_path))
    _headline(out)
    for k in ('kernels', 'cpu_baseline', 'clocks_under_load', 'host_launch_us_per_step', 'exposed_comm'):
        assert out[k] is None, (k, out[k])
    assert 'other_configs' not in out
    assert out['roofline']['gemm_family'] is None and 'families' not in out['roofline'] and out['roofline']['achieved'] > 0
    arrays = out['dump_outputs']['arrays']
    assert 'params' in arrays and 'grads' in arrays
    assert sorted(f[:-4] for f in os.listdir(tmp_path)) == sorted(arrays)


def test_full_run_still_runs_its_legs():
    out = _bench('--full', '--no-cpu-baseline', '--no-clocks')
    _headline(out)
    assert out['host_launch_us_per_step'] > 0
    gemm = out['roofline']['gemm_family']
    assert gemm and 'error' not in gemm and gemm['launches_per_step'] > 0, gemm
    assert out['roofline'].get('families') and 'error' not in out['roofline'], out['roofline']
    assert out['kernels'] and all('error' not in k for k in out['kernels']), out['kernels']
    assert out['cpu_baseline'] is None and out['clocks_under_load'] is None and 'other_configs' not in out
