"""`bench.py --dump-outputs DIR` end to end on the GPU: two runs with the same arguments write the same files byte for byte, and
the files hold what the timed path computed -- the history a direct Context.run over the same days returns and the counters its
last day leaves -- for exactly --steps timed days."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP, SEED = 12, 3, 5
FILES = ('history.npy', 'history_days.npy', 'final_counters.npy')


def _bench_dump(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(STEPS), '--warmup', str(WARMUP),
           '--seed', str(SEED), '--preheat-days', '20', '--no-sizes', '--no-ensemble', '--no-cpu', '--dump-outputs', str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return {f: (out_dir / f).read_bytes() for f in FILES}


def test_bench_dump_is_reproducible_and_is_what_the_timed_run_computed(tmp_path):
    a = _bench_dump(tmp_path / 'a')
    b = _bench_dump(tmp_path / 'b')
    assert a == b
    hist = np.load(tmp_path / 'a' / 'history.npy')
    days = np.load(tmp_path / 'a' / 'history_days.npy')
    final = np.load(tmp_path / 'a' / 'final_counters.npy')
    assert hist.dtype == days.dtype == final.dtype == np.float64
    assert np.array_equal(days, np.arange(WARMUP, WARMUP + STEPS))

    from reina_model_amd import datasets, simulation
    from reina_model_amd.variables import VARIABLE_DEFAULTS
    ctx = simulation.make_context(copy.deepcopy(VARIABLE_DEFAULTS), age_counts=datasets.get_population_for_area(), seed=SEED)
    ctx.run(WARMUP, record_history=False)
    want = ctx.run(STEPS, record_history=True)
    assert want.shape[0] == STEPS and np.array_equal(hist, want)
    assert np.array_equal(final, ctx.engine.read_counters())
