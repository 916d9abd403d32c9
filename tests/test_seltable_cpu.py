"""What tests/seltable.py promises, shown with the oracles alone (no GPU): the number of excluded counts and the conditioning of
every case, the agreement of the two oracles on every entry that tests/test_gpu_seltable.py judges (the floor under the device's
bar), what the union of the cases covers, the rules of the neutral model, the off-grid points of the refine_R test and the near-tie
rule of the end-to-end scans."""
import numpy as np
import pytest

import seltable as st
from util import c_oracle, c_sel_table, oracle_R, orc

from ballermixplus_amd.hostmodel import Grids

IDS = [st.case_id(c) for c in st.CASES]


@pytest.mark.parametrize('case', st.CASES, ids=IDS)
def test_excluded_counts_and_conditioning(case):
    """nex, the smallest base and the number of (size, pair) below 0.05 are those of the table in seltable.FACTS; at least half of
    the pairs, and at least 10, are held to the plain 1e-12 bar."""
    stat, sizes, m, _ = case
    nex = st.nex_of(stat, m)
    for n in sizes:
        assert len(orc.excluded_counts(stat, n, m)) == nex
    b = st.bases(orc, case)
    plain = int((b >= st.WELL).sum())
    print('%s: nex %d, base %.3g .. %.3g, %d of %d (size, pair) below %.2f, %d at or below %.0e' %
          (st.case_id(case), nex, b.min(), b.max(), b.size - plain, b.size, st.WELL, int((b <= st.TINY).sum()), st.TINY))
    if case in st.FACTS:
        want_nex, want_min, want_ill, want_all = st.FACTS[case]
        assert (nex, b.size - plain, b.size) == (want_nex, want_ill, want_all)
        if want_min is None:
            assert abs(b.min()) < st.TINY
        else:
            assert abs(b.min() / want_min - 1.0) < 0.03, b.min()
    else:
        assert case[3] == 'bal' and nex == 9 and plain == b.size == 900
    assert 2 * plain >= b.size
    assert np.all((b >= st.WELL).sum(axis=(1, 2)) >= 10)              # per sample size: of its 20 (450) pairs


@pytest.mark.parametrize('case', st.CASES, ids=IDS)
def test_the_two_oracles_agree_at_the_device_bar(case):
    """oracle/bmx_oracle.py (scipy, as the reference calls it) against oracle/bmx_oracle.c on every judged entry, at the bars the
    device is held to: what separates them (libm against numpy exp / log) is the floor under those bars."""
    L = c_oracle()
    xs, ab = st.grid_of(case)
    ref = st.oracle_psel(orc, case)
    got = np.concatenate([c_sel_table(L, case[0], n, case[2], xs, ab) for n in sorted(case[1])], axis=2)
    tol, judged, plain = st.psel_tolerance(case, ref, st.bases(orc, case))
    assert np.isfinite(ref[judged]).all() and np.isfinite(got[judged]).all()
    err = np.abs(got - ref)
    big = plain & (np.abs(ref) >= st.SMALL)
    worst = float(np.max(err[big] / np.abs(ref[big])))
    print('%s: C oracle against the Python oracle, worst relative difference on well-conditioned entries %.2e, worst share of the bar %.3g'
          % (st.case_id(case), worst, float(np.max(err[judged] / tol[judged]))))
    assert np.all(err[judged] <= tol[judged])
    assert np.array_equal(np.isfinite(got), np.isfinite(ref))


def test_union_of_the_cases():
    stats = {c[0] for c in st.CASES}
    assert stats == set(orc.STATS)
    nex = {st.nex_of(c[0], c[2]) for c in st.CASES}
    assert {0, 1, 8, 9, 24} <= nex and {15, 16, 17} <= nex and any(v > 128 for v in nex)
    for s in ('B2maf', 'B0maf'):
        ns = [n for c in st.CASES if c[0] == s for n in c[1]]
        assert any(n % 2 for n in ns) and any(n % 2 == 0 for n in ns), s
        # the fold-and-halve row k = n / 2 in a block that is not the first
        assert any(n % 2 == 0 for c in st.CASES if c[0] == s for n in sorted(c[1])[1:]), s
    assert any(c[0] == 'B1' and len(c[1]) == 3 for c in st.CASES)
    # Cephes branch points of lgam / lbeta: 33, 143.016, 171.62 -- one case with a size on either side of each
    walk = st.CASES[16][1]
    assert 33 in walk and 34 in walk and 143 in walk and 171 in walk and 172 in walk
    assert any(c[2] == 0 for c in st.CASES) and any(max(c[1]) > 200 for c in st.CASES) and {1, 2, 3} <= {n for c in st.CASES for n in c[1]}
    # sizes of different parity in one model: the row_off walk
    assert any(len({n % 2 for n in c[1]}) == 2 for c in st.CASES)
    assert max(sum(st.rows_per(c[0], n) for n in c[1]) for c in st.CASES if c[3] == 'short') <= 1002
    g = Grids(None, None, True, False, None, None)
    assert list(st.BAL_XS) == g.x and list(st.bal_abetas()) == [float(v) for v in g.abeta]
    for group in (st.REBUILD_CASES, st.REFINE_CASES, st.E2E_CASES):
        assert all(c in st.CASES for c in group)


@pytest.mark.parametrize('case', st.CASES, ids=IDS)
def test_neutral_model_rules(case):
    """g positive and summing to prop(n) over the counts a site of that size can carry, prop distinct and summing to 1, the absent rows as promised, and the table's exponent
    range far below the library's limit of 2^240."""
    spect, props, absent = st.model(case)
    stat, sizes = case[0], sorted(case[1])
    assert abs(sum(props.values()) - 1.0) < 1e-15 and len(set(props.values())) == len(sizes) and min(props.values()) > 0
    for n in sizes:
        nr = st.rows_per(stat, n)
        g = [spect[(k, n)] for k in range(nr) if k not in absent[n]]
        seen = [spect[(k, n)] for k in st.admissible(stat, n, case[2]) if k not in absent[n]]
        assert min(g) > 0 and len(seen) >= 1 and abs(sum(seen) - props[n]) < 1e-12 and len(g) + len(absent[n]) == nr
        assert all((k, n) not in spect for k in absent[n])
        assert len(absent[n]) == (0 if stat == 'B1' else min(3, max(nr - 2, 0)))
    g, pr = st.g_and_prop(case)
    assert np.array_equal(np.nonzero(np.isnan(g))[0], st.absent_rows(case))
    if len(sizes) > 1 and stat != 'B1':
        assert len(st.absent_rows(case)) == sum(min(3, n - 1) for n in sizes)
    R = st.table_R(case, st.oracle_psel(orc, case))
    assert np.array_equal(np.isnan(R), np.broadcast_to(np.isnan(g), R.shape))
    xs, ab = st.grid_of(case)
    assert np.array_equal(R, oracle_R(stat, sizes, case[2], spect, props, xs, ab), equal_nan=True)
    top = float(np.nanmax(R[np.isfinite(R)]))
    print('%s: %d rows, %d absent, log2(1 + max R) = %.1f' % (st.case_id(case), len(g), int(np.isnan(g).sum()), np.log2(1 + top)))
    assert np.log2(1.0 + top) < 60


@pytest.mark.parametrize('case', st.REFINE_CASES, ids=[st.case_id(c) for c in st.REFINE_CASES])
def test_refine_points_are_well_conditioned_and_clear_of_zero(case):
    """Every point of the refine_R test has a base of at least 0.05 at every sample size, the sites carry only admissible, listed
    rows, and every reference T is at least T_FLOOR from 0, so that the relative bar of the GPU test is never a bar on rounding
    noise around 0."""
    stat, sizes, m, _ = case
    gen, k, nn = st.chromosome(case, st.N_REFINE)
    assert np.all(np.diff(gen) > 0) and set(nn.tolist()) == set(sizes)
    spect = st.model(case)[0]
    for a, b in zip(k.tolist(), nn.tolist()):
        assert (a, b) in spect and a in st.admissible(stat, b, m)
    rows = st.rows_of(case, k, nn)
    assert not np.isin(rows, st.absent_rows(case)).any()
    tests = st.refine_tests()
    assert len(tests) == 50
    low = np.inf
    for A, x, a in st.OFF_GRID + st.ON_GRID:
        b = st.bases(orc, case, [x], [a])
        assert b.min() >= st.WELL, (A, x, a, b.min())
        R = st.table_R(case, np.concatenate([orc.sel_table(stat, n, m, [x], [a]) for n in sorted(sizes)], axis=2))[0, 0]
        T, ns = st.point_T(gen, rows, R, tests, A)
        assert np.isfinite(T).all() and ns.min() >= 20
        low = min(low, float(np.abs(T).min()))
        print('%s at A = %g, x = %g, alpha_beta = %g: base %.3g, T %.4g .. %.4g, window %d .. %d sites' % (st.case_id(case), A, x, a, b.min(), T.min(), T.max(), ns.min(), ns.max()))
    assert low >= st.T_FLOOR, low
    for A, x, a in st.ON_GRID:
        assert x in st.XS and a in st.ABETAS
    for A, x, a in st.OFF_GRID:
        assert not (x in st.XS and a in st.ABETAS)


@pytest.mark.parametrize('case', st.E2E_CASES, ids=[st.case_id(c) for c in st.E2E_CASES])
def test_end_to_end_inputs_and_near_ties(case):
    """The end-to-end scans: the ill-conditioned pairs are whole alpha_beta columns and leave a product grid; the near-ties by the rule
    of tests/gridshape.py (runner-up within 1e-7 of T, or within 1e-11, in the oracle's own surface) are at most a tenth of either
    run's windows, and most windows have a winner."""
    stat, sizes, m, _ = case
    xs, ab = st.e2e_grid(orc, case)
    b = st.bases(orc, case)
    assert len(xs) * len(ab) == int((b >= st.WELL).all(axis=0).sum()) and len(ab) >= 3
    gen, k, nn = st.chromosome(case, st.N_E2E)
    spect, props, _ = st.model(case)
    assert np.all(np.diff(gen) > 0) and set(nn.tolist()) == set(sizes)
    for a, c in set(zip(k.tolist(), nn.tolist())):
        assert (a, c) in spect and a in st.admissible(stat, c, m)
    rows = st.rows_of(case, k, nn)
    R = st.e2e_table(oracle_R, case, xs, ab)
    assert np.isfinite(R[:, :, np.unique(rows)]).all()
    for idx in st.e2e_tests():
        tied, best, lin = st.e2e_ties(c_oracle(), R, case, idx)
        print('%s, %d windows: %d near-ties, %d without a winner, CLR up to %.4g' % (st.case_id(case), len(idx), int(tied.sum()), int((lin < 0).sum()), best.max()))
        assert tied.sum() <= st.TIE_LIMIT * len(idx)
        assert (lin >= 0).sum() >= 0.5 * len(idx)
