"""bench.py's plain run and ``--dump-outputs`` (driver: ``python bench.py
--gpus 1 --steps K --warmup W [--dump-outputs DIR] [--full]``).

A plain run does the set-up, the warm-up, the K timed steps and the result
line; the legs beside the headline figure run with ``--full`` only.
``--dump-outputs DIR`` writes what the last timed step returned as
``DIR/<name>.npy`` in float32 / float64, at most ``bench.DUMP_BYTES`` in all.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ('parity_check', 'roofline', 'cpu_baseline', 'neighbor_list', 'fine_tune',
             'distributed', 'kernels')


def _args(argv):
    old = sys.argv
    try:
        sys.argv = ['bench.py', *argv]
        return bench.parse()
    finally:
        sys.argv = old


def _out(n=100):
    rng = np.random.default_rng(7)
    return {'energy': torch.tensor(rng.normal(), dtype=torch.float32),
            'atomic_energy': torch.tensor(rng.normal(size=n), dtype=torch.float32),
            'forces': torch.tensor(rng.normal(size=(n, 3)), dtype=torch.float32),
            'virial': torch.tensor(rng.normal(size=6), dtype=torch.float32)}


def test_full_and_dump_outputs_are_off_by_default():
    a = _args(['--gpus', '1', '--steps', '7', '--warmup', '3'])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 3)
    a = _args(['--full', '--dump-outputs', 'somewhere'])
    assert a.full and a.dump_outputs == 'somewhere'


def test_dump_outputs_writes_every_array_as_floats(tmp_path):
    out = _out()
    d = tmp_path / 'a' / 'b'   # created on demand
    bench.dump_outputs(out, str(d))
    assert sorted(os.listdir(d)) == ['atomic_energy.npy', 'energy.npy', 'forces.npy', 'virial.npy']
    for k, v in out.items():
        a = np.load(d / f'{k}.npy')
        assert a.dtype == np.float32 and a.shape == tuple(v.shape)
        assert np.array_equal(a, v.numpy())


def test_dump_outputs_per_rank_names_and_index_arrays(tmp_path):
    out = dict(_out(10), owned=np.arange(10, dtype=np.int64) * 3)
    bench.dump_outputs(out, str(tmp_path), rank=1, world=2)
    assert sorted(os.listdir(tmp_path)) == sorted(f'{k}.rank1.npy' for k in out)
    owned = np.load(tmp_path / 'owned.rank1.npy')
    assert owned.dtype == np.float64 and np.array_equal(owned, out['owned'])


def test_dump_outputs_cap_keeps_a_fixed_sample(tmp_path, monkeypatch):
    """Over the cap every array keeps the same share of its rows, the same
    rows (in order) in every run, and the directory stays under the cap."""
    monkeypatch.setattr(bench, 'DUMP_BYTES', 1000)   # the arrays below: 1,632 bytes
    out = _out(100)
    bench.dump_outputs(out, str(tmp_path / 'x'))
    bench.dump_outputs(out, str(tmp_path / 'y'))
    total = 0
    for k, v in out.items():
        a, b = np.load(tmp_path / 'x' / f'{k}.npy'), np.load(tmp_path / 'y' / f'{k}.npy')
        assert np.array_equal(a, b)
        total += a.nbytes
        if v.ndim == 0:
            assert np.array_equal(a, v.numpy())
            continue
        assert 0 < len(a) < len(v) and a.shape[1:] == tuple(v.shape[1:])
        full = v.numpy()
        rows = [int(np.flatnonzero((full == r).reshape(len(full), -1).all(axis=1))[0]) for r in a]
        assert rows == sorted(set(rows))
    assert total <= 1000
    fa, ea = np.load(tmp_path / 'x' / 'forces.npy'), np.load(tmp_path / 'x' / 'atomic_energy.npy')
    assert len(fa) == len(ea)   # same share of the same-length arrays


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_last_step(tmp_path):
    """One plain run on a 4^3-cell box: --steps sets the timed steps, the line
    carries the headline fields and ms_per_step, the --full legs are null, and
    the dumped arrays are the last step's energy / atomic energies / forces /
    virial (float32, whole: 512 atoms are far under the cap)."""
    env = {k: v for k, v in os.environ.items()
           if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3',
                        '--warmup', '1', '--cells', '4', '--dump-outputs', str(tmp_path)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    n = 8 * 4 ** 3
    assert out['steps'] == 3 and out['warmup'] == 1 and out['n_gpus'] == 1
    assert out['unit'] == 'atoms/s' and out['higher_is_better'] is True and out['dtype'] == bench.DTYPE
    assert out['metric'] == f'atoms/sec energy+force, SevenNet-0 lmax=2, {n}-atom box @1 GPU'
    assert out['ms_per_step'] > 0
    assert abs(out['value'] * out['ms_per_step'] / 1e3 - n) < 1e-2 * n   # both rounded
    assert all(out[k] is None for k in FULL_ONLY), out
    arrays = {k: np.load(tmp_path / f'{k}.npy') for k in ('energy', 'atomic_energy', 'forces', 'virial')}
    assert sorted(os.listdir(tmp_path)) == sorted(f'{k}.npy' for k in arrays)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert arrays['forces'].shape == (n, 3) and arrays['atomic_energy'].shape == (n,)
    assert arrays['virial'].shape == (6,) and arrays['energy'].shape == ()
    assert float(arrays['energy']) == out['energy']
    e = float(arrays['atomic_energy'].astype(np.float64).sum())
    # the library sums the n atomic energies in f32: at worst n half-ulps of the total
    assert abs(e - out['energy']) < n * 2.0 ** -24 * abs(out['energy'])
    assert np.abs(arrays['forces']).max() > 1e-3   # displaced atoms: not an untouched buffer
    # Newton's third law: n forces, each within the suite's 1e-4 eV/A bar, errors independent
    assert np.abs(arrays['forces'].astype(np.float64).sum(axis=0)).max() < n ** 0.5 * 1e-4
