"""The selection-table kernels over statistics, minimum counts and sample sizes (tests/seltable.py): bb_lut_kernel (K1) and its
second copy refine_R against the oracle, with a neutral model that is not flat.  tests/test_seltable_cpu.py proves the cases'
properties with the oracles alone.

Bars (seltable.psel_tolerance).  psel of a pair whose normalising base 1 - sum(excluded) is at least 0.05: relative 1e-12, the bar of
test_device_selection_table_matches_reference; oracle values below 1e-280 absolutely, against 1e-12 of the block's largest value;
B_1's polymorphism row (1 - 2 p) / base absolutely at 1e-12, because its error is that of p (up to 0.5), not relative to the
difference.  1e-6 < base < 0.05: relative 1e-12 / base (an absolute error e of the excluded sum is e / base in psel).
base <= 1e-6 or negative: device and oracle finite, or not, together.  T of refine_R: relative 1e-9, the bar of
tests/test_gpu_refine.py for eval_points.  Scans: CLR rtol 1e-9 / atol 1e-12 as test_multiple_sample_sizes_and_large_tables, the
integer fields exact except on the windows the oracle's own surface lists as near-ties (the rule and thresholds of
tests/gridshape.py), at most a tenth of a run's windows."""
import numpy as np
import pytest

import seltable as st
from test_gpu_refine import Problem
from util import c_oracle, c_scan, oracle_R, orc

pytestmark = pytest.mark.gpu

IDS = [st.case_id(c) for c in st.CASES]
ULP1 = 2.0 ** -52


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _model(case, xs=None, abetas=None):
    from ballermixplus_amd import engine as eng
    spect, props, _ = st.model(case)
    gx, ga = st.grid_of(case)
    return eng.ModelArrays(case[0], case[2], case[1], spect, props, gx if xs is None else xs, ga if abetas is None else abetas)


_LUT = {}


@pytest.fixture
def open_ctx():
    """open_ctx(model, As) -> context; every context a test opened is closed when the test ends, however it ends."""
    from ballermixplus_amd import engine as eng
    made = []

    def make(model, As=(100.0,)):
        ctx = eng.Context(0)
        made.append(ctx)
        ctx.set_model(model, list(As))
        return ctx

    yield make
    for ctx in made:
        ctx.close()


def _lut(case, open_ctx):
    """(psel, R) of the device for a case, fetched once."""
    if case not in _LUT:
        psel, R = open_ctx(_model(case)).fetch_lut()
        psel.setflags(write=False)
        R.setflags(write=False)
        _LUT[case] = (psel, R)
    return _LUT[case]


def _nex_class(case):
    nex = st.nex_of(case[0], case[2])
    return '< 8' if nex < 8 else '8 .. 128' if nex <= 128 else '> 128'


@pytest.mark.parametrize('case', st.CASES, ids=IDS)
def test_psel_matches_the_oracle(case, open_ctx):
    """(a) K1's psel on EVERY row of the table, the rows no site can carry included, against orc.sel_table per size block."""
    psel, _ = _lut(case, open_ctx)
    ref = st.oracle_psel(orc, case)
    assert psel.shape == ref.shape
    base = st.bases(orc, case)
    tol, judged, plain = st.psel_tolerance(case, ref, base)
    err = np.abs(psel - ref)
    big = plain & (np.abs(ref) >= st.SMALL)
    worst, same, n_big = float(np.max(err[big] / np.abs(ref[big]))), int((psel[big] == ref[big]).sum()), int(big.sum())
    ill = judged & ~plain
    print('%s (%s, nex %d: %s): %d entries, %d well-conditioned with worst relative error %.2e (%.1f %% bit-equal), %d ill-conditioned at %.3g of their bar, %d not judged'
          % (st.case_id(case), case[0], st.nex_of(case[0], case[2]), _nex_class(case), ref.size, n_big, worst, 100.0 * same / max(n_big, 1),
             int(ill.sum()), float(np.max(err[ill] / tol[ill])) if ill.any() else 0.0, int((~judged).sum())))
    assert np.isfinite(psel[judged]).all()
    bad = judged & ~(err <= tol)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist(), float(np.max(err[bad] / tol[bad])))
    assert np.array_equal(np.isfinite(psel[~judged]), np.isfinite(ref[~judged]))


@pytest.mark.parametrize('case', st.CASES, ids=IDS)
def test_last_line_of_k1(case, open_ctx):
    """(b) R is bit for bit (psel prop[size]) / g[row] - 1 of the device's own psel (no contraction, IEEE division: the four
    operations have one result), NaN exactly on the rows the spectrum does not list, and agrees with util.oracle_R: an error of
    bar x psel in psel is bar x (1 + R) in R, plus one rounding of the subtraction (an ulp of max(1, |R|))."""
    psel, R = _lut(case, open_ctx)
    g, pr = st.g_and_prop(case)
    with np.errstate(invalid='ignore', over='ignore'):
        want = (psel * pr) / g - 1.0
    gone = np.zeros(len(g), bool)
    gone[st.absent_rows(case)] = True
    assert gone.sum() == len(st.absent_rows(case)) and (case[0] == 'B1' or gone.any())
    assert np.array_equal(np.isnan(R), np.broadcast_to(gone, R.shape))
    diff = _bits(R[:, :, ~gone]) != _bits(want[:, :, ~gone])
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:4].tolist())
    spect, props, _ = st.model(case)
    xs, ab = st.grid_of(case)
    ref = oracle_R(case[0], case[1], case[2], spect, props, xs, ab)
    assert np.array_equal(ref, st.table_R(case, st.oracle_psel(orc, case)), equal_nan=True)
    tol, judged, _ = st.psel_tolerance(case, st.oracle_psel(orc, case), st.bases(orc, case))
    ok = judged & ~gone
    with np.errstate(invalid='ignore', over='ignore'):
        rtol = tol * pr / g + ULP1 * np.maximum(1.0, np.abs(ref))
    err = np.abs(R - ref)
    print('%s: %d entries of R bit-equal to (psel prop) / g - 1, %d NaN rows, worst error of R against the oracle %.3g of its bar'
          % (st.case_id(case), int((~gone).sum()) * R.shape[0] * R.shape[1], int(gone.sum()), float(np.max(err[ok] / rtol[ok]))))
    assert np.all(err[ok] <= rtol[ok])


def test_second_model_on_one_context_is_a_fresh_build(open_ctx):
    """(c) Two set_model calls on one context give the bytes a fresh context gives for the second model (three sample sizes and
    177 rows, then one size and 101 rows under another statistic): the log patch, row_off and both tables are rebuilt."""
    first, second = st.REBUILD_CASES
    assert first[0] != second[0] and len(first[1]) == 3 and len(second[1]) == 1
    ctx = open_ctx(_model(first))
    a0 = ctx.fetch_lut()
    ctx.set_model(_model(second), [100.0])
    a = ctx.fetch_lut()
    b = open_ctx(_model(second)).fetch_lut()
    assert a[0].shape == b[0].shape != a0[0].shape
    for u, v in zip(a, b):
        assert np.array_equal(_bits(u), _bits(v))
    # and back: the larger patch and the three-size row_off again
    ctx.set_model(_model(first), [100.0])
    for u, v in zip(ctx.fetch_lut(), a0):
        assert np.array_equal(_bits(u), _bits(v))


@pytest.mark.parametrize('case', st.REFINE_CASES, ids=[st.case_id(c) for c in st.REFINE_CASES])
def test_refine_R_through_eval_points(case, open_ctx):
    """(d) refine_R: T of 50 test sites (every 8th of 400 sites, whole-chromosome windows) at six off-grid points and two grid
    points against 2 sum log1p(alpha R) with R from the oracle's selection table at that point (Problem.R of
    tests/test_gpu_refine.py).  At the grid points refine_R and K1 differ by the log patch only: T from the device's own table
    is held to the same bar."""
    stat, sizes, m, _ = case
    gen, k, nn = st.chromosome(case, st.N_REFINE)
    model = _model(case)
    rows = model.rows_of(k, nn)
    assert np.array_equal(rows, st.rows_of(case, k, nn))
    As = sorted({p[0] for p in st.OFF_GRID + st.ON_GRID})
    ctx = open_ctx(model, As)
    ctx.set_sites(gen, rows)
    tests = st.refine_tests()
    ctx.set_tests(gen[tests])
    spect, props, _ = st.model(case)
    xs, ab = st.grid_of(case)
    pb = Problem(stat, m, sizes, spect, props, gen, rows, As, xs, ab, gen[tests], np.zeros(len(tests), np.int64), np.full(len(tests), len(gen) - 1, np.int64))
    R_dev = ctx.fetch_lut()[1]
    worst = 0.0
    for A, x, a in st.OFF_GRID + st.ON_GRID:
        assert st.bases(orc, case, [x], [a]).min() >= st.WELL
        T, ns = ctx.eval_points(A, x, a)
        want, wns = st.point_T(gen, rows, pb.R(x, a)[0, 0], tests, A)
        assert np.array_equal(ns, wns)
        assert np.abs(want).min() >= st.T_FLOOR
        rel = np.abs(T - want) / np.abs(want)
        worst = max(worst, float(rel.max()))
        assert np.all(rel <= 1e-9), (A, x, a, float(rel.max()))
        if (A, x, a) in st.ON_GRID:
            own, _ = st.point_T(gen, rows, R_dev[xs.index(x), ab.index(a)], tests, A)
            rel = np.abs(T - own) / np.abs(own)
            worst = max(worst, float(rel.max()))
            assert np.all(rel <= 1e-9), ('grid point', A, x, a, float(rel.max()))
    print('%s: eval_points at %d points x %d test sites, worst relative dT %.3e' % (st.case_id(case), len(st.OFF_GRID + st.ON_GRID), len(tests), worst))


@pytest.mark.parametrize('case', st.E2E_CASES, ids=[st.case_id(c) for c in st.E2E_CASES])
def test_scan_against_a_table_the_device_did_not_make(case, open_ctx):
    """(e) ctx.scan() against c_scan over util.oracle_R: K1 is not in the reference's loop.  3 000 sites, the short grid without the
    ill-conditioned alpha_beta columns, dense test sites 1000 .. 1699 and every 37th site."""
    L = c_oracle()
    xs, ab = st.e2e_grid(orc, case)
    gen, k, nn = st.chromosome(case, st.N_E2E)
    model = _model(case, xs, ab)
    rows = model.rows_of(k, nn)
    assert np.array_equal(rows, st.rows_of(case, k, nn))
    ctx = open_ctx(model, st.A_LIST)
    ctx.set_sites(gen, rows)
    R = st.e2e_table(oracle_R, case, xs, ab)
    for idx in st.e2e_tests():
        lo = np.zeros(len(idx), np.int64)
        hi = np.full(len(idx), st.N_E2E - 1, np.int64)
        ctx.set_tests(gen[idx], lo, hi)
        ctx.scan()
        got = ctx.fetch()
        ref = c_scan(L, R, st.A_LIST, gen, rows, gen[idx], lo, hi)
        tied = st.e2e_ties(L, R, case, idx)[0]
        assert tied.sum() <= st.TIE_LIMIT * len(idx)
        keep = ~tied
        moved = int(np.sum(np.any([got[q][keep] != ref[q][keep] for q in (1, 2, 3, 4)], axis=0)))
        worst = float(np.max(np.abs(got[0] - ref[0]) / np.maximum(np.abs(ref[0]), 1e-300)))
        print('%s, %d windows (%s): %d near-ties listed, %d other windows with another winner, CLR %.4g .. %.4g, worst relative dCLR %.3e'
              % (st.case_id(case), len(idx), ctx.plan()['kernel'], int(tied.sum()), moved, ref[0].min(), ref[0].max(), worst))
        assert np.isfinite(got[0]).all()
        for q, name in ((1, 'x'), (2, 'alpha_beta'), (3, 'A'), (4, 'nSites')):
            assert np.array_equal(got[q][keep], ref[q][keep]), (name, np.where(got[q] != ref[q])[0][:8])
        assert np.allclose(got[0], ref[0], rtol=1e-9, atol=1e-12), worst
