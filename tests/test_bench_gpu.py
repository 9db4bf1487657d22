"""bench.py on the GPU: a plain run prints the headline line and nothing else; --full adds the legs that take runs of their own."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEG_KEYS = ('initialize_ms_by_objects', 'dataset_sim', 'streaming', 'streaming_fps', 'roofline_cg', 'cpu_baseline', 'leg_errors')


def _line(args, tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '10', '--warmup', '2', '--repeats', '2',
                          '--backbone', 'resnet18', '--size', '240x432', '--report-dir', str(tmp_path)] + args,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith('{"metric"')][-1])


def test_plain_bench_runs_only_the_headline_and_full_adds_the_legs(tmp_path):
    plain = _line([], tmp_path)
    assert plain['valid'] and plain['unit'] == 'frames/s' and plain['higher_is_better'] and plain['dtype'] == 'f32'
    assert plain['value'] > 0 and abs(plain['ms_per_step'] - 1e3 / plain['value']) < 1e-6 * plain['ms_per_step']
    assert plain['repeats']['n'] == 2 and 'roofline' in plain and 'dominant_kernel' not in plain['roofline']
    assert not [k for k in LEG_KEYS if k in plain]
    # the legs are switched on by --full and off one by one by their own options there (CPU baseline and dataset leg skipped: they are long)
    full = _line(['--full', '--no-cpu-baseline', '--no-dataset-sim'], tmp_path)
    assert full['valid'] and 'leg_errors' not in full
    assert set(full['initialize_ms_by_objects']) == {'1', '2', '5'} and full['streaming_fps'] > 0 and full['roofline_cg']['ms_per_run'] > 0
    assert 'cpu_baseline' not in full and 'dataset_sim' not in full
