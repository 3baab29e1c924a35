"""bench.py's plain command line (no --full): the headline steps and nothing else -- one JSON line whose headline fields
agree with each other, the last timed step's outputs written by --dump-outputs, and none of the side measurements."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(900)
def test_bench_plain_run_is_headline_only(tmp_path):
    dump = str(tmp_path / 'outputs')
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', '--dump-outputs', dump]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=800)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['metric'] == 'training images/sec at 256x256 (pix2pix GCC)' and d['unit'] == 'images/s'
    assert d['higher_is_better'] is True and d['dtype'] == 'bf16' and d['full'] is False
    assert d['n_gpus'] == 1 and d['steps'] == 2 and d['warmup'] == 1 and d['config']['global_batch'] == 16
    assert d['value'] > 0 and abs(d['value'] - 16 / (d['ms_per_step'] / 1000.0)) < 0.5
    for side in ('roofline', 'loss_check_step1', 'other_configs', 'cpu_baseline', 'allreduce'):
        assert side not in d, side
    names = d['outputs_dumped']['arrays']
    assert 'fake_B' in names and 'student_G_state' in names
    assert sorted(f[:-4] for f in os.listdir(dump)) == sorted(names)
