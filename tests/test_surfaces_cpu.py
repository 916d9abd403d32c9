"""Likelihood surfaces of selected windows (--surfaces) without a GPU: flags and refusals, the selection rule, the writer, and
the host restatement of the surface against surfaces the reference made."""
import glob
import os

import numpy as np
import pytest

import cases
from util import GOLD, REFT, orc

from ballermixplus_amd import cli, scan as scanmod, surfaces

EX1 = os.path.join(REFT, 'Example1_fullSweep_200kya_DAF.txt')
SPECT = os.path.join(REFT, 'HC_CEU_Neut_DAF_spect_for_B2.txt')


# ------------------------------------------------------------------------------------------------------------ flags

def test_flags_off_by_default_and_parsed():
    opt = cli.build_parser().parse_args(['-i', EX1, '--spect', SPECT])
    assert opt.surfaces is False and opt.surfaceMin is None and opt.surfaceMax is None
    assert cli.surfaces_refusal(opt) is None
    assert (surfaces.MAX_WINDOWS, surfaces.HOST_BYTES) == (1000, 1 << 30)
    opt = cli.build_parser().parse_args(['-i', EX1, '--spect', SPECT, '-o', 'o', '--surfaces', '--surfaceMin', '12.5', '--surfaceMax', '7'])
    assert (opt.surfaces, opt.surfaceMin, opt.surfaceMax) == (True, 12.5, 7)
    assert cli.surfaces_refusal(opt) is None
    opt = cli.build_parser().parse_args(['-i', EX1, '--spect', SPECT, '-o', 'o', '--surfaces', '--peaks', '0.01', '--refine', '--nullPerm', '2'])
    assert cli.surfaces_refusal(opt) is None
    opt = cli.build_parser().parse_args(['-i', EX1, '--spect', SPECT, '-o', 'o', '--surfaces', '--surfaceMin=-inf'])
    assert cli.surfaces_refusal(opt) is None


@pytest.mark.parametrize('extra,env,said', [
    (['--surfaceMin', '3', '-o', 'OUT'], {}, '--surfaceMin needs --surfaces.'),
    (['--surfaceMax', '3', '-o', 'OUT'], {}, '--surfaceMax needs --surfaces.'),
    (['--surfaces', '-o', 'OUT'], {}, '--surfaces needs --peaks G (the surfaces of the apexes) or --surfaceMin C (of the windows with '
                                      'CLR >= C): the surface of every window of a chromosome is never what is meant.'),
    (['--surfaces', '--surfaceMax', '5', '-o', 'OUT'], {}, 'never what is meant'),
    (['--surfaces', '--surfaceMin', 'nan', '-o', 'OUT'], {}, '--surfaceMin takes a number.'),
    (['--surfaces', '--peaks', '0.01', '--surfaceMax', '0', '-o', 'OUT'], {}, '--surfaceMax takes a number of windows >= 1.'),
    (['--surfaces', '--surfaceMin', '1', '--surfaceMax', '-4', '-o', 'OUT'], {}, '--surfaceMax takes a number of windows >= 1.'),
    (['--surfaces', '--surfaceMin', '1', '-o', 'OUT', '--getSpect'], {},
     '--surfaces scans the input; it cannot be combined with --getSpect / --getConfig.'),
    (['--surfaces', '--surfaceMin', '1', '-o', 'OUT', '--getConfig'], {},
     '--surfaces scans the input; it cannot be combined with --getSpect / --getConfig.'),
    (['--surfaces', '--surfaceMin', '1'], {}, '--surfaces needs -o: the surfaces file is written next to the output.'),
    (['--surfaces', '--surfaceMin', '1', '-o', 'OUT'], {'WORLD_SIZE': '2'},
     '--surfaces runs in a single process; multi-rank launches are not supported.'),
    (['--surfaces', '--surfaceMin', '1', '-o', 'OUT'], {'BMX_FORCE_DIST': '1'},
     '--surfaces runs in a single process; multi-rank launches are not supported.'),
])
def test_refusals(extra, env, said, tmp_path, monkeypatch, capsys):
    from ballermixplus_amd import engine
    made = []
    monkeypatch.setattr(engine, 'Context', lambda *a, **k: made.append(1))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    argv = ['-i', EX1, '--spect', SPECT] + [str(tmp_path / 'o.txt') if a == 'OUT' else a for a in extra]
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 1
    assert said in capsys.readouterr().out
    assert not made and not glob.glob(str(tmp_path / '*'))


def test_refused_the_same_with_several_inputs(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(['-i', EX1 + ',' + EX1, '--spect', SPECT, '-o', str(tmp_path / 'd'), '--surfaces'])
    assert e.value.code == 1 and 'never what is meant' in capsys.readouterr().out
    assert not glob.glob(str(tmp_path / '*'))


# -------------------------------------------------------------------------------------------------------- selection

def test_selection_rule():
    clr = np.array([5.0, 9.0, 0.0, 9.0, 2.0, 7.0, 9.0, 3.0])
    lin = np.array([4, 0, -1, 17, 3, 8, 2, -1])
    sel = lambda *a, **k: tuple(v.tolist() if hasattr(v, 'tolist') else v for v in surfaces.select(clr, lin, *a, **k))
    # the threshold is inclusive; rows without a grid result never qualify, whatever their CLR
    assert sel() == ([0, 1, 3, 4, 5, 6], 0)
    assert sel(5.0) == ([0, 1, 3, 5, 6], 0)
    assert sel(5.000001) == ([1, 3, 5, 6], 0)
    assert sel(-np.inf) == ([0, 1, 3, 4, 5, 6], 0)
    assert sel(100.0) == ([], 0)
    # apexes only: the rule above among them (row 7 is an apex without a grid result, row 4 one below the threshold)
    assert sel(0.0, np.array([7, 4, 3], dtype=np.int32)) == ([3, 4], 0)
    assert sel(2.5, np.array([7, 4, 3], dtype=np.int32)) == ([3], 0)
    assert sel(0.0, np.zeros(0, dtype=np.int32)) == ([], 0)
    # the cap keeps the highest CLR, the earlier row among equals, and returns them in row order
    assert sel(0.0, None, 2) == ([1, 3], 4)
    assert sel(0.0, None, 3) == ([1, 3, 6], 3)
    assert sel(0.0, None, 4) == ([1, 3, 5, 6], 2)
    assert sel(0.0, None, 1) == ([1], 5)
    assert sel(0.0, None, 6) == ([0, 1, 3, 4, 5, 6], 0)
    assert sel(0.0, np.array([0, 3, 6]), 2) == ([3, 6], 1)
    rows, dropped = surfaces.select(np.zeros(0), np.zeros(0, dtype=np.int32), 0.0, None, 5)
    assert rows.dtype == np.int64 and len(rows) == 0 and dropped == 0
    rows, dropped = surfaces.select(np.zeros(0), np.zeros(0, dtype=np.int32), 0.0, np.zeros(0, dtype=np.int32), 5)
    assert len(rows) == 0 and dropped == 0


# ----------------------------------------------------------------------------------------------------------- writer

class _Sel:
    grid_A = [2000.0, 100.0, 100000000.0, 500.0]
    grid_x = [0.5, 0.05, 0.25]
    grid_abeta = [10, 0.01, 1000000000.0, 1]


def _fabricated(n):
    nA, nx, nab = len(_Sel.grid_A), len(_Sel.grid_x), len(_Sel.grid_abeta)
    rng = np.random.default_rng(5)
    T = rng.normal(0, 50, (n, nA, nx, nab))
    ns = rng.integers(1, 900, (n, nA)).astype(np.int32)
    T[0, 2] = np.nan
    ns[0, 2] = 0
    T[1, 0, 1, 3] = 0.1 + 0.2              # a value whose shortest repr needs 17 digits
    return T, ns


def test_writer_orders_the_grids_and_prints_the_main_outputs_strings(tmp_path):
    T, ns = _fabricated(3)
    ts = scanmod.TestSites()
    ts.add_many([101, 2050, 99999], [1.5e-05, 0.00205, 0.1], [1.5e-05, 0.00205, 0.1], [0, 0, 0], [9, 9, 9])
    layout = surfaces.Layout(_Sel.grid_A, _Sel.grid_x, _Sel.grid_abeta)
    phys, gen = surfaces.labels(ts, [0, 2])
    path = str(tmp_path / 's.txt')
    surfaces.write_surfaces(path, layout, phys, gen, T[[0, 2]], ns[[0, 2]])
    lines = open(path).read().split('\n')
    assert lines[0] + '\n' == surfaces.HEADER == 'physPos\tgenPos\tA\tx\tabeta\tT\tnSites\n' and lines[-1] == ''
    rows = [l.split('\t') for l in lines[1:-1]]
    assert len(rows) == 2 * 4 * 3 * 4 and all(len(r) == 7 for r in rows)
    # blocks in the order given; the first two columns are the main output's strings of that row
    for b, j in enumerate((0, 2)):
        block = rows[b * 48:(b + 1) * 48]
        main = scanmod.format_row(ts.phys[j], ts.gen_label[j], 1.0, 0, 0, 0, 5, _Sel).split('\t')
        assert all(r[:2] == main[:2] for r in block)
        # A, then x, then abeta ascending, each printed as the main output prints that grid value
        want = [(A, x, a) for A in sorted(_Sel.grid_A) for x in sorted(_Sel.grid_x) for a in sorted(_Sel.grid_abeta)]
        assert [tuple(r[2:5]) for r in block] == [(f'{A}', f'{x}', f'{a}') for A, x, a in want]
        assert block[0][2:5] == ['100.0', '0.05', '0.01'] and block[-1][2:5] == ['100000000.0', '0.5', '1000000000.0']
        for r, (A, x, a) in zip(block, want):
            iA, ix, ia = _Sel.grid_A.index(A), _Sel.grid_x.index(x), _Sel.grid_abeta.index(a)
            v = T[j, iA, ix, ia]
            assert r[5] == ('NA' if np.isnan(v) else repr(float(v))) and r[6] == str(int(ns[j, iA]))
            main = scanmod.format_row(ts.phys[j], ts.gen_label[j], 1.0, ix, ia, iA, 5, _Sel).rstrip('\n').split('\t')
            assert [r[3], r[4], r[2]] == main[3:6]
    assert sum(r[5] == 'NA' for r in rows) == 12 and all(r[6] == '0' for r in rows if r[5] == 'NA')
    # the file read back: the same numbers exactly
    p2, g2, T2, ns2 = surfaces.read_surfaces(path, layout)
    assert (p2, g2) == (phys, gen)
    assert np.array_equal(T2, layout.ascending(T[[0, 2]]), equal_nan=True)
    assert np.array_equal(ns2, ns[[0, 2]][:, layout.oA])
    # 17 significant digits survive
    surfaces.write_surfaces(path, layout, ['1'], ['2.0'], T[1:2], ns[1:2])
    assert '\t0.30000000000000004\t' in open(path).read()


def test_writer_labels_of_float_positions_and_header_only_file(tmp_path):
    ts = scanmod.TestSites()
    ts.add_na('500\t0.0005\t0\tNA\tNA\tNA\t0\n')
    ts.add(1500.0, np.float64(1500.0 * 1e-6), 1500.0 * 1e-6, 3, 9)
    ts.add(np.float64(2500.0), 2500.0 * 1e-6, 2500.0 * 1e-6, 3, 9)
    phys, gen = surfaces.labels(ts, [1, 0])
    for j, (p, g) in zip((1, 0), zip(phys, gen)):
        assert [p, g] == scanmod.format_row(ts.phys[j], ts.gen_label[j], 1.0, 0, 0, 0, 5, _Sel).split('\t')[:2]
    assert phys == ['2500.0', '1500.0']
    layout = surfaces.Layout(_Sel.grid_A, _Sel.grid_x, _Sel.grid_abeta)
    path = str(tmp_path / 'empty.txt')
    surfaces.write_surfaces(path, layout, [], [], np.zeros((0, 4, 3, 4)), np.zeros((0, 4), dtype=np.int32))
    assert open(path).read() == surfaces.HEADER
    assert surfaces.read_surfaces(path, layout)[2].shape == (0, 4, 3, 4)
    assert surfaces.output_name('a/b.txt') == 'a/b.txt.surfaces.txt'


class _FakeCtx:
    """Context stand-in: a scan result and surfaces whose values name their window."""

    def __init__(self, clr, iA):
        self.clr, self.iA, self.calls = np.asarray(clr, dtype=np.float64), np.asarray(iA, dtype=np.int32), []

    def fetch(self):
        z = np.zeros(len(self.clr), dtype=np.int32)
        return self.clr, z, z, self.iA, z

    def surfaces(self, tests):
        self.calls.append(list(tests))
        T = np.empty((len(tests), 4, 3, 4))
        T[:] = np.asarray(tests, dtype=np.float64)[:, None, None, None]
        return T, np.full((len(tests), 4), 7, dtype=np.int32)


def test_surfaces_and_write_batches_and_selects(tmp_path):
    ts = scanmod.TestSites()
    ts.add_many(np.arange(10) * 100, np.arange(10) * 1e-4, np.arange(10) * 1e-4, np.zeros(10, int), np.full(10, 9))
    ctx = _FakeCtx([1, 8, 3, 9, 0, 6, 7, 2, 5, 4], [0, 0, 0, 0, -1, 0, 0, 0, 0, 0])
    out = str(tmp_path / 'o.txt')
    # 48 points = 384 bytes per window: 800 bytes hold two
    got = surfaces.surfaces_and_write(ctx, out, ts, _Sel, 3.0, 5, None, host_bytes=800)
    assert got == (5, 2) and ctx.calls == [[1, 3], [5, 6], [8]]
    layout = surfaces.Layout(_Sel.grid_A, _Sel.grid_x, _Sel.grid_abeta)
    phys, gen, T, ns = surfaces.read_surfaces(surfaces.output_name(out), layout)
    assert phys == ['100', '300', '500', '600', '800'] and gen == [repr(j * 1e-4) for j in (1, 3, 5, 6, 8)]
    assert T[:, 0, 0, 0].tolist() == [1.0, 3.0, 5.0, 6.0, 8.0] and np.all(ns == 7)
    ctx.calls = []
    assert surfaces.surfaces_and_write(ctx, out, ts, _Sel, 0.0, 1000, np.array([3, 4, 9], dtype=np.int32)) == (2, 0)
    assert ctx.calls == [[3, 9]]
    assert surfaces.surfaces_and_write(ctx, out, ts, _Sel, 50.0, 1000, None) == (0, 0)
    assert open(surfaces.output_name(out)).read() == surfaces.HEADER
    assert surfaces.surfaces_and_write(ctx, out, scanmod.TestSites(), _Sel, 0.0, 1000, None) == (0, 0)
    assert open(surfaces.output_name(out)).read() == surfaces.HEADER


# ------------------------------------------------------------------------------------------- the host restatement

SURF = sorted(glob.glob(os.path.join(GOLD, 'surface_*.npz')))


@pytest.mark.parametrize('path', SURF, ids=[os.path.basename(p)[8:-4] for p in SURF])
def test_host_surface_reproduces_reference_likelihood_surface(path):
    """host_surface on the oracle's table (as test_oracle_golden.py builds it) against the reference's calcBaller per grid
    point, with that file's tolerance."""
    z = np.load(path)
    key = 'ex1_B2' if 'ex1_B2' in os.path.basename(path) else 'ex2_B2maf_findBal'
    opt, case, ts = cases.host_side(cases.ALL_CASES[key][0])
    m = case.oracle_model()
    s = int(z['site'])
    Ts, ns = surfaces.host_surface(m.genpos, m.row, m.R, case.As, case.data.genPos[s], 0, m.N - 1, orc.alpha_cut_z())
    ref = z['T']
    assert Ts.shape == ref.shape
    pos = ~np.isnan(ref)            # the reference reports a value only where T > 0
    assert np.all((Ts[~pos] <= 0) | np.isnan(Ts[~pos]))
    assert np.max(np.abs(Ts[pos] - ref[pos]) / np.abs(ref[pos])) < 1e-9
    has = pos.any(axis=(1, 2))
    assert np.array_equal(ns[has], z['nsites'][has])


def test_host_surface_window_bounds_and_empty_windows():
    g = np.array([0.0, 1.0, 2.0, 2.0, 3.0, 10.0])
    rows = np.array([0, 1, 0, 1, 1, 0])
    R = np.array([[[0.5, -0.25]]])
    T, ns = surfaces.host_surface(g, rows, R, [1.0, 100.0, 5.0], 2.0, -3, 99, 10.0)
    # A = 1: sites 0, 1, 4 and 5 (|d| = 2, 1, 1, 8); the two sites at the test position are excluded; A = 100: none; A = 5: 0 (on the cut), 1 and 4
    assert ns.tolist() == [4, 0, 3] and np.isnan(T[1, 0, 0])
    want = 2.0 * (np.log1p(np.exp(-2.0) * 0.5) + np.log1p(np.exp(-1.0) * -0.25) * 2 + np.log1p(np.exp(-8.0) * 0.5))
    assert abs(T[0, 0, 0] - want) < 1e-15
    assert abs(T[2, 0, 0] - 2.0 * (np.log1p(np.exp(-10.0) * 0.5) + 2 * np.log1p(np.exp(-5.0) * -0.25))) < 1e-15
    T, ns = surfaces.host_surface(g, rows, R, [1.0], 2.0, 1, 3, 10.0)
    assert ns.tolist() == [1]
    T, ns = surfaces.host_surface(g, rows, R, [1.0], 2.0, 4, 3, 10.0)
    assert ns.tolist() == [0] and np.isnan(T).all()
    # the cut is inclusive: A |d| == zcut is inside
    assert surfaces.host_surface(g, rows, R, [4.0], 0.0, 0, 5, 8.0)[1].tolist() == [3]
    assert surfaces.host_surface(g, rows, R, [4.0], 0.0, 0, 5, np.nextafter(8.0, 0.0))[1].tolist() == [1]
