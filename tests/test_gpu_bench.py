"""bench.py on the GPU: a plain run prints the headline alone; --full adds what the benchmark measures beyond it."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step')
FULL_ONLY = ('host_enqueue_ms_per_step', 'kernel_time_ms_per_step', 'gpu_idle_frac', 'kernels', 'fp32_products',
             'fwd_ms_per_img', 'configs3')


def run_bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
           '--prewarm-seconds', '0'] + list(extra)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_alone():
    d = run_bench()
    assert all(k in d for k in HEADLINE), d
    assert d['value'] > 100 and d['unit'] == 'images/sec' and d['higher_is_better'] is True and d['steps'] == 3
    assert abs(d['ms_per_step'] - 16 * 1e3 / d['value']) < 1e-2 * d['ms_per_step']
    assert d['roofline'] is None and d['cpu_baseline'] is None
    assert not [k for k in FULL_ONLY if k in d], d


def test_full_run_adds_the_profile():
    """--full with the long legs left out (other arithmetics, eval forward, configs[3], CPU oracle): the per-op profile and
    the roofline of the dominant kernel ride along with the same headline fields."""
    d = run_bench('--full', '--no-fp32-reference', '--no-fwd', '--no-configs3', '--no-cpu-baseline')
    assert all(k in d for k in HEADLINE), d
    assert d['host_enqueue_ms_per_step'] > 0 and d['kernel_time_ms_per_step'] > 0 and d['kernels']
    assert d['roofline']['kernel'] in d['kernels'] and d['roofline']['bound'] in ('hbm', 'mfma')
    assert 'fp32_products' not in d and 'fwd_ms_per_img' not in d and 'configs3' not in d and d['cpu_baseline'] is None
