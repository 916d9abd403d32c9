"""The goodness-of-fit table of a window (--fit) without a GPU: the host restatement against a literal per-site loop, the
identities of its sums, the class and the bin rule, the summary on hand-written tables, the files, the flags and every refusal,
the prototypes, the conditioning of the cases the GPU tests compare on, and the planted case."""
import math
import os

import numpy as np
import pytest

import fitcases as fc
from util import REFT, REPO, orc

from ballermixplus_amd import _lib, cli, engine, fit, influence, power, surfaces

EX1 = os.path.join(REFT, 'Example1_fullSweep_200kya_DAF.txt')
SPECT = os.path.join(REFT, 'HC_CEU_Neut_DAF_spect_for_B2.txt')
ZCUT = orc.alpha_cut_z()

_cases = {}


def case(name):
    if name not in _cases:
        c = fc.catalogue(engine)[name]()
        _cases[name] = (c, c.R())
    return _cases[name]


def test_the_cut_is_the_librarys():
    assert ZCUT == power.ALPHA_CUT


# ------------------------------------------------------------------------------------------ the restatement, literally

@pytest.mark.parametrize('name', ['ex1_B1', 'ragged', 'lattice', 'excluded'])
def test_host_fit_against_the_literal_loop(name):
    c, R = case(name)
    cat = c.cat
    worst = 0.0
    for q, (w, lin) in enumerate(c.entries):
        if lin < 0:
            continue
        iA, ix, ia = lin // (c.nx * c.nab), (lin // c.nab) % c.nx, lin % c.nab
        O, Es, En, sk = c.host(q, R)
        lO, lEs, lEn, lsk = fc.literal_fit(cat.gen, cat.rows, c.row_off, R, c.gw, c.cls, c.F, c.edges.tolist(), cat.As[iA], ix, ia,
                                           cat.tg[w], cat.lo[w], cat.hi[w], ZCUT)
        assert np.array_equal(O, lO) and sk == lsk, (name, q)
        n_d = O.sum(axis=1)
        # both are float64 sums of the same quotients: only the order of the sites differs
        bound = 1e-13 * np.maximum(1, n_d)[:, None]
        assert np.all(np.abs(Es - lEs) <= bound) and np.all(np.abs(En - lEn) <= bound), (name, q)
        worst = max(worst, float(np.max(np.abs(Es - lEs) / bound)), float(np.max(np.abs(En - lEn) / bound)))
    print('%s: largest |host_fit - literal| / bound = %.3f' % (name, worst))


@pytest.mark.parametrize('name', fc.NAMES)
def test_the_sums_of_the_table(name):
    """sum_c O[d] = n_d, sum_d n_d = the surfaces' nSites at that A, sum_c E[d] = n_d minus the skipped sites."""
    c, R = case(name)
    cat = c.cat
    for q, (w, lin) in enumerate(c.entries):
        O, Es, En, sk = c.host(q, R)
        if lin < 0:
            assert not O.any() and np.isnan(Es).all() and np.isnan(En).all() and sk == 0
            continue
        iA = lin // (c.nx * c.nab)
        idx, z = fit.qualifying(cat.gen, cat.As[iA], cat.tg[w], cat.lo[w], cat.hi[w], ZCUT)
        bins = np.array([sum(1 for e in c.edges.tolist() if v > e) for v in z.tolist()], dtype=np.int64)
        n_d = np.bincount(bins, minlength=c.D)
        assert np.array_equal(O.sum(axis=1), n_d)
        _, ns = surfaces.host_surface(cat.gen, cat.rows, R, [cat.As[iA]], cat.tg[w], cat.lo[w], cat.hi[w], ZCUT)
        assert int(O.sum()) == int(ns[0]) == len(idx)
        # the skipped sites of a bin: those of a size block without an admissible row (the only way to a total of 0 here)
        block = np.searchsorted(c.row_off, cat.rows[idx], side='right') - 1
        dead = np.array([not c.gw[c.row_off[j]:c.row_off[j + 1]].any() for j in range(len(c.sizes))])
        sk_d = np.bincount(bins[dead[block]], minlength=c.D)
        assert sk == int(sk_d.sum())
        tol = fc.TOL * np.maximum(1, n_d)
        assert np.all(np.abs(Es.sum(axis=1) - (n_d - sk_d)) <= tol) and np.all(np.abs(En.sum(axis=1) - (n_d - sk_d)) <= tol)
        assert np.all(Es >= -1e-15) and np.all(En >= 0)


def test_the_cases_hold_what_they_are_for():
    c, R = case('excluded')
    cat = c.cat
    on_zero = c.gw[cat.rows] == 0
    assert on_zero.any() and (cat.rows[on_zero] == c.row_off[1] + 1).any()       # sites on rows with gw = 0: k = 1 < min count among them
    assert np.isnan(R[0, 0][c.gw == 0]).any()                                    # ... and rows with gw = 0 whose R is NaN (g is)
    assert any(c.host(q, R)[3] > 0 for q in range(len(c.entries)))               # ... and skipped sites
    c, _ = case('many_sizes')
    assert len(c.sizes) * c.F * 16 > fc.header_constant('BMX_FIT_LDS_BYTES')
    c, R = case('edges')
    counts = sorted({int(c.host(q, R)[0].sum()) for q in range(len(c.entries))})
    assert set((0, 1, 255, 256, 257, 512, 513)) <= set(counts) and len(c.entries) == 40
    c, _ = case('ragged')
    assert len(c.sizes) == 3 and any(l < 0 for _, l in c.entries)


# ------------------------------------------------------------------------------------------------------ class and bin rule

def test_the_class_rule():
    sizes, off = [4, 10], [0, 5, 16]
    cls = fit.classes('B2', sizes, off, 10)
    assert cls[:5].tolist() == [0, 2, 5, 7, 9]                     # (k * 10) // 4, k = n in the last class
    assert cls[5:].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9]
    assert fit.classes('B2maf', sizes, off, 3)[:5].tolist() == [0, 0, 1, 2, 2]
    assert fit.classes('B2', sizes, off, 1).tolist() == [0] * 16
    b1 = fit.classes('B1', sizes, [0, 2, 4], 6)
    assert b1.tolist() == [0, 1, 0, 1]
    with pytest.raises(ValueError):
        fit.classes('B1', sizes, [0, 2, 4], 1)
    with pytest.raises(ValueError):
        fit.classes('B2', sizes, off, 0)
    c, _ = case('ex1_B1')
    assert c.stat == 'B1' and set(c.cls.tolist()) == {0, 1}
    c, _ = case('ex1_B2maf')
    assert c.stat == 'B2maf' and (c.gw == 0).any()


def test_the_bin_rule_on_the_lattice():
    """z = 16 |g| is exact: the site on an edge and the site one ulp below it fall into the lower bin, the one above into the
    upper."""
    gen, marks = fc.lattice_positions()
    edges = fc.LATTICE_EDGES
    rows = np.zeros(len(gen), dtype=np.int64)
    R = np.zeros((1, 1, 2))
    gw, cls = np.array([0.5, 0.5]), np.array([0, 1])
    for k, e in enumerate(edges):
        below, on, above = marks[e]
        assert 16.0 * below < e and 16.0 * on == e and 16.0 * above > e
        assert np.nextafter(16.0 * below, np.inf) == e and np.nextafter(e, np.inf) == 16.0 * above
        for d, want in ((below, k), (on, k), (above, k + 1)):
            for sign in (-1.0, 1.0):
                i = int(np.nonzero(gen == sign * d)[0][0])
                O, _, _, _ = fit.host_fit(gen, rows, [0, 2], R, gw, cls, 2, edges, 16.0, 0, 0, 0.0, i, i, ZCUT)
                assert O.sum() == 1 and O[want, 0] == 1, (e, d, sign)
    default = fit.default_edges(8, ZCUT)
    assert len(default) == 7 and default[0] == ZCUT / 8 and default[6] == 7 * (ZCUT / 8) and default[6] < ZCUT
    for bad in ([1.0, 1.0], [0.0, 1.0], [2.0, 1.0], [1.0, math.inf], [math.nan]):
        with pytest.raises(ValueError):
            fit.check_edges(bad)


# ------------------------------------------------------------------------------------------------ summary and writers

def test_the_summary_rule_on_a_hand_written_table():
    O = np.array([[10, 2, 1, 0], [6, 7, 0, 0], [1, 0, 0, 0]])
    E = np.array([[8.0, 3.0, 1.5, 0.5], [5.0, 6.0, 1.0, 1.0], [0.5, 0.25, 0.25, 0.0]])
    s = fit.chi_square(O, E, 5.0)
    # bin 0: cell 0 used, rest (O 3, E 5) used; bin 1: cells 0 and 1 used, rest (O 0, E 2) dropped; bin 2: rest (O 1, E 1) dropped
    assert [(d, c) for d, c, _, _ in s['used']] == [(0, 0), (0, 4), (1, 0), (1, 1)]
    assert s['dropped'] == 2 and s['df'] == 4 - 2
    assert abs(s['X2'] - ((10 - 8) ** 2 / 8 + (3 - 5) ** 2 / 5 + 1 / 5 + 1 / 6)) < 1e-15
    En = np.array([[4.0, 4.0, 4.0, 1.0], [6.0, 6.0, 0.5, 0.5], [0.25, 0.25, 0.25, 0.25]])
    w = fit.summarise(O, E, En, 5.0)
    assert w['nSites'] == 27 and w['X2_sel'] == s['X2'] and w['df_sel'] == 2 and w['nPooled'] == 2
    n = fit.chi_square(O, En, 5.0)
    assert w['X2_neu'] == n['X2'] and w['df_neu'] == n['df'] == 3 - 2            # bin 0's rest holds 13 >= 5; no single cell does
    assert (w['worst_bin'], w['worst_class']) == (0, 4) and abs(w['worst_resid'] - (3 - 5) / math.sqrt(5)) < 1e-15
    none = fit.summarise(O, E * 0.01, En, 5.0)
    assert none['X2_sel'] is None and none['X2_neu'] is None and none['nPooled'] is None and none['worst_bin'] is None
    nan = fit.summarise(np.zeros((2, 2), dtype=int), np.full((2, 2), np.nan), np.full((2, 2), np.nan))
    assert nan['nSites'] == 0 and nan['X2_sel'] is None
    only_sel = fit.summarise(O, E, En * 0.01, 5.0)
    assert only_sel['X2_sel'] == s['X2'] and only_sel['X2_neu'] is None and only_sel['df_neu'] is None


class _Sel:
    grid_x, grid_abeta, grid_A = [0.1, 0.5], [1, 20], [100, 2000, 3.5]


def test_both_files_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    D, F, n = 3, 4, 5
    O = rng.integers(0, 30, (n, D, F)).astype(np.int32)
    Es, En = rng.uniform(0, 30, (n, D, F)), rng.uniform(0, 30, (n, D, F))
    O[4] = 0
    Es[4] = En[4] = np.nan
    lin = np.array([0, 5, 11, 7, -1])
    phys, gen, clr = [str(100 * i) for i in range(n)], [repr(0.001 * i) for i in range(n)], [repr(1.5 * i) for i in range(n)]
    skipped = [0, 1, 0, 2, 0]
    edges = [1.0, 4.5]
    out = str(tmp_path / 'o.txt')
    fit.write_fit(out, phys, gen, clr, lin, _Sel, O, Es, En, skipped, edges, ZCUT, 5.0, detail=True)
    names, rows = fit.read_table(fit.output_name(out))
    assert '\t'.join(names) + '\n' == fit.HEADER and len(rows) == n
    for w, r in enumerate(rows):
        s = fit.summarise(O[w], Es[w], En[w], 5.0)
        assert r[:3] == [phys[w], gen[w], clr[w]] and r[3:6] == list(influence.grid_strings(int(lin[w]), _Sel))
        assert int(r[6]) == int(O[w].sum()) and int(r[7]) == skipped[w]
        if s['X2_sel'] is None:
            assert r[8:] == ['NA'] * 8
            continue
        assert float(r[8]) == s['X2_sel'] and int(r[9]) == s['df_sel'] and float(r[10]) == s['X2_neu'] and int(r[11]) == s['df_neu']
        assert int(r[12]) == s['nPooled'] and int(r[13]) == s['worst_bin'] and float(r[15]) == s['worst_resid']
        assert r[14] == ('rest' if s['worst_class'] == F else str(s['worst_class']))
    assert rows[1][3:6] == ['0.1', '20', '2000'] and rows[4][3:6] == ['NA'] * 3 and rows[4][8:] == ['NA'] * 8
    p, g, rO, rEs, rEn = fit.read_cells(fit.cells_name(out), D, F)
    assert p == phys and g == gen and np.array_equal(rO, O)
    assert np.array_equal(rEs, Es, equal_nan=True) and np.array_equal(rEn, En, equal_nan=True)      # repr round-trips
    names, cells = fit.read_table(fit.cells_name(out))
    assert len(cells) == n * D * F and cells[0][2:6] == ['0', '0.0', '1.0', '0'] and cells[F][2:5] == ['1', '1.0', '4.5']
    assert cells[2 * F][3:5] == ['4.5', repr(ZCUT)]
    fit.write_fit(out, [], [], [], [], _Sel, np.zeros((0, D, F)), np.zeros((0, D, F)), np.zeros((0, D, F)), [], edges, ZCUT, detail=True)
    assert open(fit.output_name(out)).read() == fit.HEADER and open(fit.cells_name(out)).read() == fit.CELLS_HEADER


# ------------------------------------------------------------------------------------------------------------ refusals

def test_every_value_refusal():
    v = fit.value_refusal
    assert v(None, None, None, None, None) is None and v(8, 10, 0.0, 1000, 5.0) is None and v(16, 16, -1.0, 1, 0.5) is None
    assert v(0, None, None, None, None) == '--fitBins takes a number of distance bins >= 1.'
    assert v(None, 0, None, None, None) == '--fitClasses takes a number of frequency classes >= 1.'
    assert v(None, 1, None, None, None, True) == ('--fitClasses must be >= 2 with --noFreq: its two rows per sample size are the '
                                                   'classes 0 and 1.')
    assert v(None, 1, None, None, None, False) is None
    assert v(26, 10, None, None, None) == '--fitBins times --fitClasses must be <= 256.'
    assert v(None, 33, None, None, None) == '--fitBins times --fitClasses must be <= 256.'
    assert v(None, None, None, 0, None) == '--fitMax takes a number of windows >= 1.'
    assert v(None, None, math.nan, None, None) == '--fitMin takes a number.'
    for bad in (0.0, -1.0, math.inf, math.nan):
        assert v(None, None, None, None, bad) == '--fitMinExp takes a finite expected count > 0.'


def _refusal(argv, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 1
    return capsys.readouterr().out.strip()


def test_every_cli_refusal(capsys, monkeypatch, tmp_path):
    made = []
    monkeypatch.setattr(engine, 'Context', lambda *a, **k: made.append(1))
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.delenv('BMX_FORCE_DIST', raising=False)
    base = ['-i', EX1, '--spect', SPECT]
    out = ['-o', str(tmp_path / 'o.txt')]
    for flag, val in (('fitBins', '4'), ('fitClasses', '4'), ('fitMin', '3'), ('fitMax', '5'), ('fitMinExp', '2'), ('fitDetail', None)):
        argv = base + out + ['--' + flag] + ([val] if val else [])
        assert _refusal(argv, capsys) == '--%s needs --fit.' % flag
    assert _refusal(base + out + ['--fit', '--fitMin', '1', '--fitBins', '0'], capsys) == '--fitBins takes a number of distance bins >= 1.'
    assert _refusal(base + out + ['--fit', '--fitMin', '1', '--fitBins', '64', '--fitClasses', '5'], capsys) == \
        '--fitBins times --fitClasses must be <= 256.'
    assert _refusal(base + out + ['--fit', '--fitMin', '1', '--noFreq', '--fitClasses', '1'], capsys).startswith('--fitClasses must be >= 2')
    assert _refusal(base + out + ['--fit'], capsys).startswith('--fit needs --peaks G (the fit of the apexes) or --fitMin C')
    assert _refusal(base + out + ['--fit', '--fitMin', '1', '--getSpect'], capsys) == \
        '--fit scans the input; it cannot be combined with --getSpect / --getConfig.'
    assert _refusal(base + ['--fit', '--fitMin', '1'], capsys) == '--fit needs -o: the fit file is written next to the output.'
    monkeypatch.setenv('WORLD_SIZE', '2')
    assert _refusal(base + out + ['--fit', '--fitMin', '1'], capsys) == '--fit runs in a single process; multi-rank launches are not supported.'
    assert not made


def test_the_flags_and_the_prototypes():
    opt = cli.build_parser().parse_args(['-i', 'x', '--spect', 'y', '--fit', '--fitBins', '4', '--fitClasses', '6', '--fitMin', '2.5', '--fitMax', '7',
                                         '--fitMinExp', '3', '--fitDetail'])
    assert (opt.fit, opt.fitBins, opt.fitClasses, opt.fitMin, opt.fitMax, opt.fitMinExp, opt.fitDetail) == (True, 4, 6, 2.5, 7, 3.0, True)
    off = cli.build_parser().parse_args(['-i', 'x', '--spect', 'y'])
    assert off.fit is False and off.fitBins is None and off.fitClasses is None and off.fitMin is None and off.fitMax is None
    assert off.fitMinExp is None and off.fitDetail is False
    assert '--fit [--fitBins D]' in cli.__doc__
    for name in ('bmx_ctx_fit', 'bmx_ctx_fit_ms'):
        assert name in _lib.PROTOTYPES
    with open(os.path.join(REPO, 'include', 'bmxscan.h')) as f:
        h = f.read()
    assert 'int bmx_ctx_fit(bmx_ctx *c, int64_t n, const int32_t *tests, const int32_t *lin' in h and 'int bmx_ctx_fit_ms(' in h
    assert fc.header_constant('BMX_FIT_MAX_CELLS') == fit.MAX_CELLS == 256
    assert len(_lib.PROTOTYPES['bmx_ctx_fit'][1]) == 13


# ----------------------------------------------------------------------------------------------------- decisiveness

@pytest.mark.parametrize('name', fc.NAMES)
def test_the_tolerance_hides_no_conditioning_problem(name):
    """The float64 restatement against the same restatement in long double: within a tenth of the GPU tolerance on every cell."""
    assert np.finfo(np.longdouble).eps < 1e-18
    c, R = case(name)
    worst = 0.0
    for q, (w, lin) in enumerate(c.entries):
        if lin < 0:
            continue
        O, Es, En, sk = c.host(q, R)
        lO, lEs, lEn, lsk = c.host(q, R, dtype=np.longdouble)
        assert np.array_equal(O, lO) and sk == lsk
        bound = fc.TOL * np.maximum(1, O.sum(axis=1))[:, None]
        ratio = max(float(np.max(np.abs(Es - lEs) / bound)), float(np.max(np.abs(En - lEn) / bound)))
        assert ratio <= 0.1, (name, q, ratio)
        worst = max(worst, ratio)
    print('%s: largest |float64 - long double| / tolerance = %.2e' % (name, worst))


# ----------------------------------------------------------------------------------------------------- the planted case

def planted_verdict(O, Es, En):
    """The two inequalities of the planted case on one table; returns the summary."""
    s = fit.summarise(O, Es, En, fit.MIN_EXP)
    used = fit.chi_square(O, Es, fit.MIN_EXP)['used']
    assert len(used) >= 20
    assert s['X2_sel'] <= fc.chi2_quantile(0.999, s['df_sel']), s
    assert s['X2_neu'] > fc.chi2_quantile(0.999, s['df_neu']), s
    return s


def test_the_planted_point_fits_and_neutrality_does_not():
    c, lin = fc.planted(engine)
    assert not np.array_equal(c.cat.rows, fc.example('ex1_B2', engine, [0], 10, 8, 1).cat.rows)
    O, Es, En, sk = c.host(0, c.cat.R())
    assert sk == 0 and O.sum() >= 700
    s = planted_verdict(O, Es, En)
    print('planted: X2_sel %.2f (df %d), X2_neu %.2f (df %d)' % (s['X2_sel'], s['df_sel'], s['X2_neu'], s['df_neu']))


def test_the_quantile():
    assert abs(fc.chi2_quantile(0.999, 10) - 29.588) < 0.05 and abs(fc.chi2_quantile(0.999, 18) - 42.312) < 0.05
