"""--refine without a GPU: flag parsing and refusals (no context is created), bounds and initial steps of the grids, the
compass search on the oracle's objective, the writer, and the host objective against the reference's own T at off-grid
points (tests/golden/refine, made by tests/golden/make_refine_golden.py)."""
import glob
import json
import math
import os

import numpy as np
import pytest

import cases
from util import GOLD, REFT, orc, oracle_R, read_tsv

from ballermixplus_amd import cli, refine
from ballermixplus_amd import scan as scanmod
from ballermixplus_amd.hostmodel import Grids

EX1 = os.path.join(REFT, 'Example1_fullSweep_200kya_DAF.txt')
SPECT = os.path.join(REFT, 'HC_CEU_Neut_DAF_spect_for_B2.txt')
RG = os.path.join(GOLD, 'refine')


# ---------------------------------------------------------------------------------------------------- flags

def test_flags_off_by_default_and_parsed():
    opt = cli.build_parser().parse_args(['-i', EX1, '--spect', SPECT])
    assert not opt.refine and opt.refineMin is None and cli.refine_refusal(opt) is None
    opt = cli.build_parser().parse_args(['-i', EX1, '--spect', SPECT, '-o', 'o', '--refine', '--refineMin', '12.5'])
    assert opt.refine and opt.refineMin == 12.5 and cli.refine_refusal(opt) is None


@pytest.mark.parametrize('extra,env,word', [
    (['--refineMin', '3', '-o', 'OUT'], {}, '--refineMin'),
    (['--refine'], {}, '--refine'),
    (['--refine', '-o', 'OUT', '--getSpect'], {}, '--refine'),
    (['--refine', '-o', 'OUT', '--getConfig'], {}, '--refine'),
    (['--refine', '-o', 'OUT'], {'WORLD_SIZE': '2'}, '--refine'),
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


# ---------------------------------------------------------------------------------------------------- bounds and steps

def _setup(x=None, abeta=None, bal=False, pos=False, listA=None):
    g = Grids(x, abeta, bal, pos, None, listA)
    xs, ab, As = g.scan_order()
    return g, refine.Setup(As, xs, ab)


def test_default_grid_bounds_and_steps():
    g, st = _setup()
    assert st.free == (True, True, True)
    assert st.lo == (math.log(100.0), 0.05, math.log(0.001)) and st.hi == (math.log(1e8), 0.5, math.log(1e9))
    c, nat, h = st.start(5000, 0.25, 40)
    assert nat == (5000.0, 0.25, 40.0) and c == (math.log(5000), 0.25, math.log(40))
    assert h[0] == 0.5 * min(math.log(5000) - math.log(4500), math.log(6000) - math.log(5000))
    xs = sorted(set(g.x))
    i = xs.index(0.25)
    assert h[1] == 0.5 * min(xs[i] - xs[i - 1], xs[i + 1] - xs[i])
    assert h[2] == 0.5 * min(math.log(40) - math.log(35), math.log(45) - math.log(40))
    # hull ends: the one gap
    _, _, h = st.start(1e8, 0.5, 1e9)
    assert h == (0.5 * (math.log(1e8) - math.log(1e6)), 0.5 * (0.5 - xs[-2]), 0.5 * (math.log(1e9) - math.log(1e6)))
    _, _, h = st.start(100, xs[0], 0.001)
    assert h == (0.5 * (math.log(200) - math.log(100)), 0.5 * (xs[1] - xs[0]), 0.5 * (math.log(0.01) - math.log(0.001)))


def test_findbal_findpos_fixx_lista_bounds():
    g, st = _setup(bal=True)
    assert st.lo[2] == math.log(1.0) and st.hi[2] == math.log(1e9)         # alpha_beta >= 1
    g, st = _setup(pos=True)
    assert st.lo[2] == math.log(0.001) and st.hi[2] == math.log(0.8)
    assert st.lo[1] == min(g.x) and st.hi[1] == max(g.x)
    g, st = _setup(x='0.3')
    assert st.free == (True, False, True) and st.lo[1] == st.hi[1] == 0.3
    assert st.start(900, 0.3, 5)[2][1] == 0.0
    g, st = _setup(listA='2500')
    assert st.free == (False, True, True) and st.start(2500, 0.25, 5)[2][0] == 0.0
    g, st = _setup(x='0.3', abeta=7.0, listA='2500')
    assert st.free == (False, False, False)


# ---------------------------------------------------------------------------------------------------- compass on the oracle

def _objective(case, ts, j):
    """T(A, x, abeta) of test site j by the oracle's selection table on a one-value grid."""
    m = case.oracle_model()
    d = case.data
    sizes = sorted(set(int(n) for n in d.sampSizes))
    cache = {}

    def T(A, x, a):
        key = (x, a)
        if key not in cache:
            cache[key] = oracle_R(case.stat, sizes, d.minCount, case.neut.spect, case.neut.sampProps, [x], [a])[0, 0]
        sub, alphas = orc.window_mask(m, A, ts.lo[j], ts.hi[j], ts.test_gen[j])
        if len(sub) == 0:
            return -math.inf
        with np.errstate(divide='ignore', invalid='ignore'):
            return float(2.0 * np.sum(np.log1p(alphas[sub] * cache[key][m.row[sub]])))
    return T


@pytest.mark.parametrize('name,rows', [('ex1_B2', (378, 600)), ('ex2_B2', (592, 900)), ('ex2_B2maf', (700,))])
def test_compass_on_oracle(name, rows):
    argv, gold = cases.ALL_CASES[name]
    opt, case, ts = cases.host_side(list(argv))
    st = refine.Setup(case.As, case.xs, case.abetas)
    ref = read_tsv(gold)
    for j in rows:
        r = ref[j]
        grid_clr = float(r[2])
        A, x, a = float(r[5]), float(r[3]), float(r[4])
        T = _objective(case, ts, j)
        c0, nat0, h0 = st.start(A, x, a)
        f = refine.coord_objective(T, c0, nat0)
        c, Tc, rounds, h = refine.compass(f, c0, st.free, st.lo, st.hi, h0)
        assert Tc >= T(A, x, a) and Tc >= grid_clr * (1 - 1e-9)
        assert rounds < refine.MAX_ROUNDS and all(h[k] < refine.TOL[k] for k in range(3))
        # a compass-local optimum at the last steps that were tried (twice the final ones)
        for d in range(6):
            k = d // 2
            v = min(max(c[k] + 2 * h[k] if d & 1 else c[k] - 2 * h[k], st.lo[k]), st.hi[k])
            if v != c[k]:
                assert f(c[:k] + (v,) + c[k + 1:]) <= Tc
        out = refine.refine_window(T, st, A, x, a, grid_clr)
        assert out[0] >= grid_clr


def test_compass_keeps_fixed_coordinates():
    argv = cases.ALL_CASES['ex2_B2'][0] + ['--fixX', '0.3', '--listA', '900']
    opt, case, ts = cases.host_side(list(argv))
    st = refine.Setup(case.As, case.xs, case.abetas)
    assert st.free == (False, False, True)
    T = _objective(case, ts, 592)
    c0, nat0, h0 = st.start(900.0, 0.3, 1e6)
    seen = []
    f = refine.coord_objective(T, c0, nat0)
    c, Tc, rounds, _ = refine.compass(lambda p: seen.append(p) or f(p), c0, st.free, st.lo, st.hi, h0)
    assert all(p[0] == c0[0] and p[1] == c0[1] for p in seen)
    assert refine.natural_of(c, c0, nat0)[:2] == (900.0, 0.3)


def test_compass_rules_on_a_toy_objective():
    """Ties go to the first candidate in order, non-finite values count as -inf, steps halve only without a move."""
    calls = []

    def f(c):
        calls.append(c)
        return float('nan') if c[1] > 0.6 else -((c[0] - 1.0) ** 2) - (c[1] - 0.4) ** 2 - (c[2] + 0.5) ** 2
    c, T, rounds, h = refine.compass(f, (0.0, 0.5, 0.0), (True, True, True), (-2.0, 0.1, -3.0), (3.0, 0.7, 3.0),
                                     (0.25, 0.05, 0.25))
    assert abs(c[0] - 1.0) < 1e-3 and abs(c[1] - 0.4) < 1e-4 and abs(c[2] + 0.5) < 1e-3
    assert calls[0] == (0.0, 0.5, 0.0)
    c, T, rounds, h = refine.compass(lambda p: 1.0, (0.0, 0.5, 0.0), (True, True, True), (-2.0, 0.1, -3.0), (3.0, 0.7, 3.0),
                                     (0.25, 0.05, 0.25))
    assert c == (0.0, 0.5, 0.0) and all(h[k] < refine.TOL[k] for k in range(3))
    c, T, rounds, h = refine.compass(lambda p: 1.0, (0.0, 0.5, 0.0), (True, True, True), (-2.0, 0.1, -3.0), (3.0, 0.7, 3.0),
                                     (0.25, 0.05, 0.25), max_rounds=3)
    assert rounds == 3 and h == (0.25 / 8, 0.05 / 8, 0.25 / 8)


# ---------------------------------------------------------------------------------------------------- writer

def _ts_with_na():
    ts = scanmod.TestSites()
    ts.add(100, 1e-4, 1e-4, 0, 5)
    ts.add_na('200\t2e-4\tNA\tNA\tNA\tNA\tNA\n')
    ts.add(300, 3e-4, 3e-4, 0, 5)
    ts.add(400, 4e-4, 4e-4, 0, 5)
    return ts


def test_writer_keeps_unimproved_and_na_rows(tmp_path):
    ts = _ts_with_na()
    main = tmp_path / 'o.txt'
    lines = [scanmod.HEADER, '100\t0.0001\t12.5\t0.25\t40\t1000\t77\n', '200\t2e-4\tNA\tNA\tNA\tNA\tNA\n',
             '300\t0.0003\t0.0\t0.0\t0.0\t0.0\t0.0\n', '400\t0.0004\t3.25\t0.5\t1000000000.0\t900\t12\n']
    main.write_text(''.join(lines))
    clr = np.array([12.5, 0.0, 3.25])
    refined = (np.array([13.0625, 0.0, 3.25]), np.array([1100.5, np.nan, 900.0]), np.array([0.2712, np.nan, 0.5]),
               np.array([37.25, np.nan, 1e9]), np.array([80, 0, 12]))
    out = tmp_path / 'o.txt.refined.txt'
    refine.write_refined(str(out), str(main), ts, clr, refined)
    got = out.read_text().splitlines(True)
    assert got[0] == lines[0] and got[2:] == lines[2:]
    assert got[1] == '100\t0.0001\t13.0625\t0.2712\t37.25\t1100.5\t80\n'
    assert refine.improved_rows(clr, refined[0]).tolist() == [0]


def test_writer_without_na_rows(tmp_path):
    ts = scanmod.TestSites()
    ts.add_many(np.array([1, 2]), np.array([1e-6, 2e-6]), np.array([1e-6, 2e-6]), np.array([0, 0]), np.array([1, 1]))
    main = tmp_path / 'o.txt'
    main.write_text(scanmod.HEADER + '1\t1e-06\t5.0\t0.3\t5\t900\t3\n2\t2e-06\t6.0\t0.3\t5\t900\t3\n')
    refine.write_refined(str(tmp_path / 'r.txt'), str(main), ts, np.array([5.0, 6.0]),
                         (np.array([5.0, 6.5]), np.array([900.0, 912.25]), np.array([0.3, 0.31]), np.array([5.0, 5.5]),
                          np.array([3, 4])))
    assert (tmp_path / 'r.txt').read_text() == scanmod.HEADER + '1\t1e-06\t5.0\t0.3\t5\t900\t3\n' \
        '2\t2e-06\t6.5\t0.31\t5.5\t912.25\t4\n'


# ---------------------------------------------------------------------------------------------------- host objective

@pytest.mark.parametrize('name', sorted(f[:-10] for f in os.listdir(RG) if f.endswith('.args.json')))
def test_host_objective_matches_reference_off_grid(name):
    with open(os.path.join(RG, name + '.args.json')) as f:
        args = json.load(f)
    args = [os.path.join(REFT, a) if a.endswith('.txt') else a for a in args]
    x, a, A = (float(args[args.index(k) + 1]) for k in ('--fixX', '--fixAlpha', '--listA'))
    base = [v for i, v in enumerate(args) if v not in ('--fixX', '--fixAlpha', '--listA')
            and (i == 0 or args[i - 1] not in ('--fixX', '--fixAlpha', '--listA'))]
    opt, case, ts = cases.host_side(base)       # the default grid: the objective is evaluated off it
    assert x not in case.xs and a not in case.abetas and A not in case.As
    gold = read_tsv(os.path.join(RG, name + '.tsv'))
    assert len(gold) == len(ts.test_gen)
    m = case.oracle_model()
    hit = 0
    for j, row in enumerate(gold):
        want = float(row[2])
        T = _objective(case, ts, j)(A, x, a)
        if want > 0:
            hit += 1
            assert abs(T - want) <= 1e-9 * want, (j, T, want)
            sub, _ = orc.window_mask(m, A, ts.lo[j], ts.hi[j], ts.test_gen[j])
            assert len(sub) == int(row[6])
        else:
            assert not T > 0
    assert hit >= 5
