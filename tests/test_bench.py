"""bench.py's own contract: what a plain run prints and does, what --full adds, and the arrays --dump-outputs writes
(window order whatever the number of ranks, a fixed sample of a large step, float64, at most 64 MB)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from util import REPO

import bench  # noqa: E402  (tests/conftest.py puts the repository root on sys.path)
from ballermixplus_amd import _lib  # noqa: E402

HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step')


def test_arguments_plain_by_default():
    a = bench.parse_args(['--gpus', '1', '--steps', '7', '--warmup', '3'])
    assert (a.gpus, a.steps, a.warmup, a.full, a.dump_outputs) == (1, 7, 3, False, None)
    a = bench.parse_args(['--full', '--dump-outputs', 'out'])
    assert a.full and a.dump_outputs == 'out'
    with pytest.raises(SystemExit):
        bench.parse_args(['--steps', '0'])


def test_dump_sample_is_fixed_and_bounded():
    assert np.array_equal(bench.dump_sample(1000), np.arange(1000))
    a = bench.dump_sample(40_000_000)
    b = bench.dump_sample(40_000_000)
    assert len(a) == bench.DUMP_WINDOWS and np.array_equal(a, b)
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < 40_000_000
    # the largest dump: four float64 arrays of DUMP_WINDOWS entries
    assert 4 * 8 * bench.DUMP_WINDOWS <= 64 * 2 ** 20


def _records(n, seed=0):
    rng = np.random.default_rng(seed)
    rec = np.empty(n, dtype=_lib.RECORD_DTYPE)
    rec['clr'] = rng.random(n) * 100
    rec['lin'] = rng.integers(-1, 15810, n)
    rec['nsites'] = rng.integers(0, 5000, n)
    return rec


@pytest.mark.parametrize('world', [2, 3, 8])
def test_ordered_records_undo_the_sharding(world):
    """Per chromosome, rank r holds the test sites distributed.assign gives it, chromosome after chromosome: put back in
    window order they are the one-rank records."""
    from ballermixplus_amd import distributed
    sizes = [10000, 4097, 1, 23456]
    full = _records(sum(sizes))
    offs = np.concatenate(([0], np.cumsum(sizes)))
    per_rank = [[] for _ in range(world)]
    layout = []
    for ci, M in enumerate(sizes):
        parts = distributed.assign(M, world)
        layout.append([len(p) for p in parts])
        for r in range(world):
            per_rank[r].append(full[offs[ci]:offs[ci + 1]][parts[r]])
    last = [np.concatenate(p) for p in per_rank]
    got = bench.ordered_records(last, layout, True, world)
    assert np.array_equal(got, full)
    assert np.array_equal(bench.ordered_records([full], [[len(full)]], True, 1), full)


def test_dump_outputs_writes_float64_arrays(tmp_path):
    rec = _records(5000, seed=3)
    n = bench.dump_outputs(str(tmp_path / 'd'), rec)
    assert n == 5000
    got = {name: np.load(tmp_path / 'd' / (name + '.npy')) for name in ('window', 'clr', 'lin', 'nsites')}
    for a in got.values():
        assert a.dtype == np.float64 and a.shape == (5000,)
    assert np.array_equal(got['window'], np.arange(5000))
    assert np.array_equal(got['clr'], rec['clr'])
    assert np.array_equal(got['lin'], rec['lin'].astype(np.float64))
    assert np.array_equal(got['nsites'], rec['nsites'].astype(np.float64))


@pytest.mark.gpu
def test_plain_run_and_its_outputs(tmp_path):
    """A plain run: exactly the requested steps, the headline fields, none of what --full adds; the dumped arrays are the
    whole last step (400k windows < the sample cap), in window order, and sum to the line's checksum."""
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'BMX_FORCE_DIST', 'BMX_NATIVE_GATHER', 'BMX_DIST_BACKEND', 'BMX_SINGLE_DEVICE'):
        env.pop(k, None)
    out = tmp_path / 'dump'
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
                        '--total-snps', '400000', '--dump-outputs', str(out)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    for k in HEADLINE:
        assert k in d, k
    assert d['unit'] == 'windows/s' and d['higher_is_better'] is True and d['dtype'] == 'f64'
    assert d['steps'] == 3 and d['warmup'] == 1 and d['full'] is False
    W = d['config']['windows_per_step']
    assert abs(d['value'] - W / (d['ms_per_step'] * 1e-3)) < 1e-6 * d['value']
    for k in ('roofline', 'roofline_hbm', 'parity_sample', 'cpu_baseline'):
        assert k not in d, k
    assert 'end_to_end_seconds' not in d['config']
    assert d['dumped_windows'] == W == d['config']['records_per_step']
    got = {name: np.load(out / (name + '.npy')) for name in ('window', 'clr', 'lin', 'nsites')}
    assert sum(os.path.getsize(out / (name + '.npy')) for name in got) <= 64 * 2 ** 20
    for a in got.values():
        assert a.dtype == np.float64 and a.shape == (W,)
    assert np.array_equal(got['window'], np.arange(W))
    assert np.all(np.isfinite(got['clr'])) and np.array_equal(got['lin'], np.round(got['lin']))
    assert float(np.sum(got['clr'])) == pytest.approx(d['config']['checksum_clr'], rel=1e-12)
