"""--support without a GPU: flag parsing and refusals (no context is created), the definition (ballermixplus_amd/support.py) on
a quadratic objective with known profile ends and on the oracle's host objective, and the writer."""
import glob
import math

import numpy as np
import pytest

import cases
from test_refine_cpu import EX1, SPECT, _objective
from util import read_tsv

from ballermixplus_amd import cli, refine, support
from ballermixplus_amd import scan as scanmod


# ---------------------------------------------------------------------------------------------------- flags

def test_flags_off_by_default_and_parsed():
    opt = cli.build_parser().parse_args(['-i', EX1, '--spect', SPECT])
    assert not opt.support and opt.supportDrop is None and opt.supportMin is None and cli.support_refusal(opt) is None
    opt = cli.build_parser().parse_args(['-i', EX1, '--spect', SPECT, '-o', 'o', '--refine', '--support', '--supportDrop', '2.5',
                                         '--supportMin', '7'])
    assert opt.support and opt.supportDrop == 2.5 and opt.supportMin == 7.0
    assert cli.refine_refusal(opt) is None and cli.support_refusal(opt) is None
    assert support.DROP == 3.841458820694124


@pytest.mark.parametrize('extra,env,word', [
    (['--support', '-o', 'OUT'], {}, '--support'),
    (['--refine', '--supportDrop', '2', '-o', 'OUT'], {}, '--supportDrop'),
    (['--refine', '--supportMin', '2', '-o', 'OUT'], {}, '--supportMin'),
    (['--refine', '--support', '--supportDrop', '0', '-o', 'OUT'], {}, '--supportDrop'),
    (['--refine', '--support', '--supportDrop', '-1', '-o', 'OUT'], {}, '--supportDrop'),
    (['--refine', '--support', '--supportDrop', 'inf', '-o', 'OUT'], {}, '--supportDrop'),
    (['--refine', '--support', '--supportDrop', 'nan', '-o', 'OUT'], {}, '--supportDrop'),
    (['--refine', '--support', '--supportMin', 'nan', '-o', 'OUT'], {}, '--supportMin'),
    (['--refine', '--support'], {}, '--refine'),
    (['--refine', '--support', '-o', 'OUT', '--getSpect'], {}, '--refine'),
    (['--refine', '--support', '-o', 'OUT'], {'WORLD_SIZE': '2'}, '--refine'),
])
def test_refusals(extra, env, word, tmp_path, monkeypatch, capsys):
    from ballermixplus_amd import engine
    made = []
    monkeypatch.setattr(engine, 'Context', lambda *a, **k: made.append(1))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    argv = ['-i', EX1, '--spect', SPECT] + [str(tmp_path / 'o.txt') if a == 'OUT' else a for a in extra]
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 1
    assert word in capsys.readouterr().out
    assert not made and not glob.glob(str(tmp_path / '*'))


# ---------------------------------------------------------------------------------------------------- a quadratic objective

C_STAR = (7.0, 0.3, 2.0)
HALF = (0.8, 0.04, 1.0)             # the profile half-widths sqrt(D (Q^-1)_kk) the quadratic is built for
LO, HI = (0.0, 0.01, -10.0), (20.0, 0.99, 10.0)
H0 = (0.05, 0.025, 0.1)


def _quadratic():
    corr = np.array([[1.0, 0.5, -0.3], [0.5, 1.0, 0.2], [-0.3, 0.2, 1.0]])
    sd = np.sqrt(np.array(HALF) ** 2 / support.DROP)
    Sigma = corr * np.outer(sd, sd)
    Q = np.linalg.inv(Sigma)
    T_star = 50.0

    def f(c):
        d = np.array(c) - np.array(C_STAR)
        return T_star - float(d @ Q @ d)
    return f, Q, T_star


def test_quadratic_ends_match_the_analytic_profile():
    f, Q, T_star = _quadratic()
    Ts, Tb, ends = support.support_window(f, C_STAR, (True, True, True), LO, HI, H0)
    assert Ts == T_star and Tb >= Ts and Tb <= Ts + 1e-9
    L = T_star - support.DROP
    Sigma = np.linalg.inv(Q)
    for k in range(3):
        w = math.sqrt(support.DROP * Sigma[k, k])
        for side, s in enumerate((-1, 1)):
            e = ends[k][side]
            assert not e['censored']
            assert abs(e['end'] - (C_STAR[k] + s * w)) <= support.END_TOL[k], (k, s, e['end'], C_STAR[k] + s * w)
            assert e['witness'][k] == e['end'] and e['witness_T'] >= L and e['outside_T'] < L
            assert abs(e['outside'][k] - e['end']) < support.END_TOL[k]
            assert e['evals'] > 0 and e['rounds'] > 0


def test_quadratic_hull_inside_the_interval_is_censored():
    f, Q, T_star = _quadratic()
    hi = (HI[0], C_STAR[1] + 0.02, HI[2])
    Ts, Tb, ends = support.support_window(f, C_STAR, (True, True, True), LO, hi, H0)
    e = ends[1][1]
    assert e['censored'] and e['end'] == hi[1] and e['outside'] is None and e['witness_T'] >= T_star - support.DROP
    assert not ends[1][0]['censored']


def test_quadratic_fixed_coordinate_is_na():
    f, Q, T_star = _quadratic()
    Ts, Tb, ends = support.support_window(f, C_STAR, (True, False, True), LO, HI, H0)
    assert ends[1] == [None, None]
    Sigma2 = np.linalg.inv(Q[np.ix_([0, 2], [0, 2])])     # the profile with x held at its centre value
    for k, kk in ((0, 0), (2, 1)):
        w = math.sqrt(support.DROP * Sigma2[kk, kk])
        for side, s in enumerate((-1, 1)):
            e = ends[k][side]
            assert e['witness'][1] == C_STAR[1]
            assert abs(e['end'] - (C_STAR[k] + s * w)) <= support.END_TOL[k]


# ---------------------------------------------------------------------------------------------------- the oracle's objective

@pytest.mark.parametrize('j', [378, 600])
def test_support_on_oracle(j):
    argv, gold = cases.ALL_CASES['ex1_B2']
    opt, case, ts = cases.host_side(list(argv))
    st = refine.Setup(case.As, case.xs, case.abetas)
    r = read_tsv(gold)[j]
    grid = (float(r[5]), float(r[3]), float(r[4]))
    T = _objective(case, ts, j)
    out = refine.refine_window(T, st, *grid, float(r[2]))
    nat = out[1:4]
    Ts, Tb, ends = support.support_natural(T, st, grid, nat)
    assert Ts == T(*nat) and Tb >= Ts
    L = Ts - support.DROP
    for k in range(3):
        lo, hi = ends[k][0]['end'], ends[k][1]['end']
        assert lo <= nat[k] <= hi
        for e in ends[k]:
            assert e['witness'][k] == e['end'] and e['witness_T'] >= L
            assert T(*e['witness']) == e['witness_T']
            if not e['censored']:
                assert e['outside_T'] < L
                assert abs(refine.to_coord(k, e['outside'][k]) - refine.to_coord(k, e['end'])) < support.END_TOL[k]
            else:
                assert refine.to_coord(k, e['end']) in (st.lo[k], st.hi[k])


# ---------------------------------------------------------------------------------------------------- writer

def _sup(M):
    """fetch_support()'s layout, nothing computed."""
    return {'lo': np.full((M, 3), np.nan), 'hi': np.full((M, 3), np.nan), 'censored': np.zeros((M, 3, 2), dtype=np.int32),
            'rounds': np.full((M, 3, 2), -1, dtype=np.int32), 'T_best': np.full(M, np.nan)}


def _ts_with_na():
    ts = scanmod.TestSites()
    ts.add(100, 1e-4, 1e-4, 0, 5)
    ts.add_na('200\t2e-4\t0\tNA\tNA\tNA\t0\n')
    ts.add(300, 3e-4, 3e-4, 0, 5)
    ts.add(400, 4e-4, 4e-4, 0, 5)
    return ts


def test_writer_na_rows_fixed_columns_and_censored(tmp_path):
    ts = _ts_with_na()
    main = tmp_path / 'o.txt'
    main.write_text(scanmod.HEADER + '100\t0.0001\t12.5\t0.25\t40\t1000\t77\n200\t2e-4\t0\tNA\tNA\tNA\t0\n'
                    '300\t0.0003\t0.0\t0.0\t0.0\t0.0\t0.0\n400\t0.0004\t3.25\t0.5\t1000000000.0\t900\t12\n')
    sup = _sup(3)
    sup['lo'][0] = (800.5, 0.21, 30.25)
    sup['hi'][0] = (1e8, 0.3125, 55.0)
    sup['rounds'][0] = 10
    sup['censored'][0, 0, 1] = 1
    sup['T_best'][0] = 13.5
    sup['lo'][2] = (700.0, np.nan, 1.0)         # x fixed
    sup['hi'][2] = (950.0, np.nan, 2.5)
    sup['rounds'][2] = 4
    sup['rounds'][2, 1] = -1
    sup['censored'][2, 2, 0] = 1
    sup['censored'][2, 1, 1] = 1
    sup['T_best'][2] = 3.25
    out = tmp_path / 'o.txt.support.txt'
    support.write_support(str(out), str(main), ts, np.array([13.0625, 0.0, 3.25]), sup)
    got = out.read_text().splitlines(True)
    assert got == [support.HEADER,
                   '100\t0.0001\t13.0625\t0.21\t0.3125\t30.25\t55.0\t800.5\t100000000.0\t13.5\tA_hi\n',
                   '200\t2e-4\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\n',
                   '300\t0.0003\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\n',
                   '400\t0.0004\t3.25\tNA\tNA\t1.0\t2.5\t700.0\t950.0\t3.25\ts_lo\n']
    assert support.output_name('a/b.txt') == 'a/b.txt.support.txt'


def test_writer_without_na_rows_and_uncensored(tmp_path):
    ts = scanmod.TestSites()
    ts.add_many(np.array([1, 2]), np.array([1e-6, 2e-6]), np.array([1e-6, 2e-6]), np.array([0, 0]), np.array([1, 1]))
    main = tmp_path / 'o.txt'
    main.write_text(scanmod.HEADER + '1\t1e-06\t5.0\t0.3\t5\t900\t3\n2\t2e-06\t6.0\t0.3\t5\t900\t3\n')
    sup = _sup(2)
    sup['lo'][1] = (850.0, 0.25, 4.0)
    sup['hi'][1] = (990.0, 0.35, 6.0)
    sup['rounds'][1] = 3
    sup['T_best'][1] = 6.5
    support.write_support(str(tmp_path / 's.txt'), str(main), ts, np.array([5.0, 6.5]), sup)
    assert (tmp_path / 's.txt').read_text() == support.HEADER + '1\t1e-06\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\n' \
        '2\t2e-06\t6.5\t0.25\t0.35\t4.0\t6.0\t850.0\t990.0\t6.5\t.\n'


def test_writer_without_test_sites(tmp_path):
    ts = scanmod.TestSites()
    ts.add_na('5\t5e-06\t0\tNA\tNA\tNA\t0\n')
    main = tmp_path / 'o.txt'
    main.write_text(scanmod.HEADER + '5\t5e-06\t0\tNA\tNA\tNA\t0\n')
    support.support_and_write(None, str(main), ts, support.DROP, 0.0)
    assert (tmp_path / 'o.txt.support.txt').read_text() == support.HEADER + '5\t5e-06\t' + '\t'.join(['NA'] * 9) + '\n'
