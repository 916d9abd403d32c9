"""--profiles without a GPU: flag parsing and refusals (no context is created), the writer, and the host definition of the
profiles on likelihood surfaces the reference made."""
import glob
import os

import numpy as np
import pytest

from util import GOLD, REFT

from ballermixplus_amd import cli, profiles
from ballermixplus_amd import scan as scanmod

EX1 = os.path.join(REFT, 'Example1_fullSweep_200kya_DAF.txt')
SPECT = os.path.join(REFT, 'HC_CEU_Neut_DAF_spect_for_B2.txt')


def test_parse_and_mask():
    assert profiles.parse('abeta,A') == ('A', 'abeta')
    assert profiles.parse('x') == ('x',)
    assert profiles.mask(profiles.parse('A,x,abeta')) == 7
    for bad in ('', 'B', 'A,alpha', 'a'):
        with pytest.raises(ValueError):
            profiles.parse(bad)


@pytest.mark.parametrize('extra,env', [
    (['--profiles', 'A,y', '-o', 'OUT'], {}),
    (['--profiles', 'A'], {}),
    (['--profiles', 'x', '-o', 'OUT', '--getSpect'], {}),
    (['--profiles', 'x', '-o', 'OUT', '--getConfig'], {}),
    (['--profiles', 'abeta', '-o', 'OUT'], {'WORLD_SIZE': '2'}),
])
def test_refusals(extra, env, tmp_path, monkeypatch, capsys):
    from ballermixplus_amd import engine
    made = []
    monkeypatch.setattr(engine, 'Context', lambda *a, **k: made.append(1))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    argv = ['-i', EX1, '--spect', SPECT] + [str(tmp_path / 'o.txt') if a == 'OUT' else a for a in extra]
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 1
    assert '--profiles' in capsys.readouterr().out
    assert not made and not glob.glob(str(tmp_path / '*'))


def test_off_by_default():
    opt = cli.build_parser().parse_args(['-i', EX1, '--spect', SPECT])
    assert opt.profiles is None and cli.profiles_refusal(opt) is None and cli.profile_names(opt) == ()


def _ts_with_na():
    ts = scanmod.TestSites()
    ts.add(100, 1e-4, 1e-4, 0, 5)
    ts.add_na('200\t2e-4\tNA\tNA\tNA\tNA\tNA\n')
    ts.add(300, 3e-4, 3e-4, 0, 5)
    return ts


def test_writer(tmp_path):
    ts = _ts_with_na()
    grid = [0.5, 0.2, 1e3, 1.0]                  # scan order, not ascending
    prof = np.array([[1.5, 0.0, 2.25, 0.125], [0.0, 0.0, 0.0, 0.0]])
    p = str(tmp_path / 'o.profile_abeta.txt')
    profiles.write_profile(p, 'abeta', ts, prof, grid)
    lines = open(p).read().splitlines()
    assert lines[0].split('\t') == ['physPos', 'genPos', 'abeta=0.2', 'abeta=0.5', 'abeta=1.0', 'abeta=1000.0', 'CLR_bal', 'CLR_pos']
    assert lines[1].split('\t') == ['100', '0.0001', '0.0', '1.5', '0.125', '2.25', '2.25', '1.5']
    assert lines[2].split('\t') == ['200', '2e-4'] + ['NA'] * 6
    assert lines[3].split('\t') == ['300', '0.0003'] + ['0.0'] * 6
    x = [0.05, 0.15000000000000002, 0.1]
    p = str(tmp_path / 'o.profile_x.txt')
    profiles.write_profile(p, 'x', ts, np.array([[0.1, 1 / 3, 2.0], [7.0, 8.0, 9.0]]), x)
    lines = open(p).read().splitlines()
    assert lines[0].split('\t') == ['physPos', 'genPos', 'x=0.05', 'x=0.1', 'x=0.15000000000000002']
    assert lines[1].split('\t')[2:] == ['0.1', '2.0', repr(1 / 3)]
    assert lines[2].endswith('NA\tNA\tNA') and len(lines) == 4


def test_writer_empty(tmp_path):
    ts = scanmod.TestSites()
    p = str(tmp_path / 'o.profile_A.txt')
    profiles.write_profile(p, 'A', ts, np.zeros((0, 2)), [100.0, 50.0])
    assert open(p).read() == 'physPos\tgenPos\tA=50.0\tA=100.0\n'


@pytest.mark.parametrize('path', sorted(glob.glob(os.path.join(GOLD, 'surface_ex*.npz'))))
def test_profiles_from_reference_surfaces(path):
    d = np.load(path)
    T = d['T']
    pr = profiles.profiles_from_surface(T)
    assert pr['A'].shape == (T.shape[0],) and pr['x'].shape == (T.shape[1],) and pr['abeta'].shape == (T.shape[2],)
    best = max(float(d['best'][0]), 0.0)
    for k in ('A', 'x', 'abeta'):
        assert np.all(pr[k] >= 0.0)
        assert pr[k].max() == best, (k, pr[k].max(), best)
    iA = int(np.nanargmax(np.where(np.isnan(T), -np.inf, T)) // (T.shape[1] * T.shape[2]))
    assert pr['A'][iA] == best
    assert np.all(pr['A'][np.all(np.isnan(T), axis=(1, 2))] == 0.0)
