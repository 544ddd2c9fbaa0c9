"""GPU: a plain bench.py run (no --full) at a small shape: the contract keys of its one line, nothing of the --full
measurements in it, and the outputs of the last timed step (--dump-outputs) -- the same arrays, bit for bit, when the
same command runs again (seeded inputs; at bs >= 2, T >= 512 a train step is bit-reproducible)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', '1',
           '--batch', '2', '--frames', '512', '--dump-outputs', str(out_dir)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def _load(out_dir):
    return {f[:-len('.npy')]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_plain_bench_line_and_outputs(tmp_path):
    line = _bench(tmp_path / 'a', 3)
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in line, k
    assert line['steps'] == 3 and line['warmup'] == 1 and line['n_gpus'] == 1
    assert line['value'] > 0 and line['ms_per_step'] > 0 and line['dtype'] == 'f32' and line['higher_is_better']
    assert abs(line['value'] - 2 * 1e3 / line['ms_per_step']) <= 1e-2 * line['value']
    for k in ('h2d', 'verify', 'split16', 'roofline', 'mfma_kernels', 'kernels', 'cpu_baseline'):
        assert k not in line, k                                  # --full only

    a = _load(tmp_path / 'a')
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    params = [k for k in a if k.startswith('param.')]
    assert len(params) > 100 and all('grad.' + k[len('param.'):] in a for k in params)
    assert any(k.endswith('running_var') for k in a)
    assert round(float(a['loss.total']), 4) == line['config']['loss_total']
    assert all(np.isfinite(v).all() for v in a.values())

    _bench(tmp_path / 'b', 3)
    b = _load(tmp_path / 'b')
    assert sorted(a) == sorted(b)
    differ = [k for k in a if not np.array_equal(a[k], b[k])]
    assert not differ, differ[:10]
