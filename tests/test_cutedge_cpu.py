"""The inputs of tests/test_gpu_cut_edge.py really put sites on the window cut, and the comparison made there would notice a
membership error: shown here on the CPU, from the definitions and with the table the oracle builds itself.

Every test prints the figures it measured; they are copied into DESIGN.md (section 6)."""
import functools

import numpy as np
import pytest

import cutedge as ce
from util import c_oracle, c_scan, oracle_R, orc

Z = ce.zcut()


@functools.lru_cache(maxsize=None)
def _sel_max(n):
    return float(orc.sel_table('B2', n, 1, ce.XS, ce.ABETAS)[:, :, ce.LOUD_K].max())


@functools.lru_cache(maxsize=None)
def _table(name):
    """R[nx][nab][rows] = P_sel prop / g - 1 as oracle_R builds it, 0 on the rows no site can carry."""
    gen, k, nn, rows, sizes, span = ce.dataset(name)
    spect, props = ce.spectrum(sizes, span, _sel_max(sizes[0]))
    R = oracle_R('B2', sizes, 1, spect, props, ce.XS, ce.ABETAS)
    assert np.isfinite(R[:, :, np.unique(rows)]).all()
    R = np.where(np.isfinite(R), R, 0.0)
    R.setflags(write=False)
    return R


@functools.lru_cache(maxsize=None)
def _single(name):
    """{A: (clr, ix, ia, iA, ns)} of the C oracle's single-A scans of EVERY site as a test site, whole-chromosome windows."""
    gen, k, nn, rows, sizes, span = ce.dataset(name)
    idx = ce.tests_of(1)
    lo, hi = ce.whole(idx)
    return {A: c_scan(c_oracle(), _table(name), [A], gen, rows, gen[idx], lo, hi) for _, A in ce.A_values(ce.SETS[name][0])}


def test_the_recipe_is_what_the_docstring_says():
    assert ce.N == 4096 and len(ce.KS) == 16 and ce.A_NONE * min(ce.H.values()) > 4 * Z
    for layout in ce.LAYOUTS:
        g = ce.positions(layout)
        assert len(g) == ce.N and np.all(np.diff(g) >= 0)
    assert np.array_equal(ce.positions('dyadic'), np.arange(ce.N) * 2.0 ** -17) and np.all(np.diff(ce.positions('decimal')) > 0)
    g = ce.positions('runs')
    u, c = np.unique(g, return_counts=True)
    at = np.round(u / 1e-5).astype(int)
    assert set(c.tolist()) == {1, 3} and np.all((c[:-1] == 3) == (at[:-1] % ce.RUN_EVERY == ce.RUN_AT)) and np.array_equal(u, ce.positions('decimal')[:len(u)])
    figures = {}
    for name, (layout, span, sizes) in ce.SETS.items():
        gen, k, nn, rows, _, _ = ce.dataset(name)
        R = _table(name)
        loud = ce.rows_of(sizes, np.array([ce.LOUD_K]), np.array([sizes[0]]))[0]
        assert np.all(k >= 1) and np.all(k <= nn) and sorted(set(nn.tolist())) == list(sizes)
        assert not span or np.all(rows[::ce.LOUD_EVERY] == loud)
        assert np.array_equal(rows[np.arange(ce.N) % ce.LOUD_EVERY > 0], ce.dataset('decimal0' if sizes == ce.SMALL else name)[3][np.arange(ce.N) % ce.LOUD_EVERY > 0])
        rest = np.unique(rows[rows != loud]) if span else np.unique(rows)
        home = R[ce.HOME[0], ce.HOME[1]]
        assert np.allclose(home[rest], ce.LIFT, rtol=0, atol=1e-9)           # every other row: R = LIFT at the home grid point
        bits = float(np.log2(1.0 + R.max()))
        figures[name] = (round(bits, 6), len(np.unique(rows)), R.shape[2])
        if span:
            assert np.unravel_index(np.argmax(R), R.shape)[2] == loud and abs(bits - (span - ce.MARGIN)) < 1e-6
            assert np.log2(1.0 + np.delete(R, loud, axis=2).max()) < 10
    assert _table('large12').shape[2] == 483 and 483 * 64 * 8 > 160 * 1024      # that R slice does not fit in LDS
    for s in ce.STRIDES:
        assert np.median(np.diff(ce.tests_of(s))) == s
    print('set -> (log2(1 + max R), rows that sites carry, table rows): %r' % (figures,))


@pytest.mark.parametrize('layout', ce.LAYOUTS)
def test_in_out_split(layout):
    """'dyadic': the K-th neighbour on either side of every test site that has one is in at A_in(K) and out at A_out(K), and the
    (K - 1)-th is in at both.  'decimal' and 'runs': per K, some A of the list leaves at least 10 % of the windows with the K-th
    neighbouring position in, and some A at least 10 % with it out."""
    g = ce.positions(layout)
    u = np.unique(g)
    shares = {}
    for K in ce.KS:
        d = u[K:] - u[:-K]
        As = [A for k, A in ce.A_values(layout) if k == K]
        sh = [float(np.mean(A * d <= Z)) for A in As]
        shares[K] = [round(s, 2) for s in sh]
        if layout == 'dyadic':
            assert len(As) == 2 and As[1] == np.nextafter(As[0], np.inf) and sh == [1.0, 0.0]
            assert np.all(d == K * ce.H['dyadic'])
            if K > 1:
                assert np.all(As[1] * (u[K - 1:] - u[:-(K - 1)]) <= Z)
            idx = ce.tests_of(1)
            want = np.minimum(idx, K) + np.minimum(ce.N - 1 - idx, K)
            assert np.array_equal(ce.n_sites(g, idx, As[0], ce.exact(Z)), want)
            assert np.array_equal(ce.n_sites(g, idx, As[1], ce.exact(Z)), np.minimum(idx, K - 1) + np.minimum(ce.N - 1 - idx, K - 1))
        else:
            assert 3 <= len(As) <= 5 and np.all(np.diff(As) > 0)
            assert max(sh) >= 0.1 and min(sh) <= 0.9, (K, sh)
            assert len(np.unique(d)) >= 9
            # the (K - 1)-th position is in and the (K + 1)-th out at every A of the K: only the K-th is in question
            if K > 1:
                assert np.all(As[-1] * (u[K - 1:] - u[:-(K - 1)]) <= Z)
            assert np.all(As[0] * (u[K + 1:] - u[:-(K + 1)]) > Z)
    print('%s: K -> share of the windows whose K-th neighbour is in, per A of the K: %r' % (layout, shares))
    idx = ce.tests_of(1)
    assert not ce.n_sites(g, idx, ce.A_NONE, ce.exact(Z)).any()


@pytest.mark.parametrize('layout', ce.LAYOUTS)
def test_the_product_form_is_the_references_predicate(layout):
    """A d <= zcut and np.exp(-A d) >= 1e-8 agree on every (test site, site, A) used: on every distinct distance between two sites
    of the layout, at every A of the single-A lists and of the multi-A list."""
    g = ce.positions(layout)
    i, j = np.triu_indices(ce.N, 1)
    d = np.unique(g[j] - g[i])
    As = sorted({A for _, A in ce.A_values(layout)} | set(ce.A_list(layout)))
    edge = 0
    for A in As:
        zz = A * d
        a, b = zz <= Z, np.exp(-zz) >= 1e-8
        assert np.array_equal(a, b), (A, d[a != b][:4])
        edge += int(np.sum(np.abs(zz - Z) <= 4 * np.spacing(Z)))
    print('%s: %d distinct distances x %d A values; %d products within 4 ulp of the cut' % (layout, len(d), len(As), edge))
    assert edge >= len(ce.KS)


def _delta(name, A, idx):
    """(|dT| f64[M], T f64[M]): what the winning T of every window of idx moves by when its farthest in-site leaves or its nearest
    out-site enters (the larger of the two), at the oracle's winning grid point; 0 where the window has no winner."""
    gen, k, nn, rows, sizes, span = ce.dataset(name)
    R = _table(name)
    clr, ix, ia, iA, ns = (v[idx] for v in _single(name)[A])
    far, near = ce.boundary_sites(gen, idx, A, ce.exact(Z))
    dT = np.zeros(len(idx))
    for b in (far, near):
        has = (b >= 0) & (iA >= 0)
        bb = np.maximum(b, 0)
        al = np.exp(-(A * np.abs(gen[bb] - gen[idx])))
        with np.errstate(divide='ignore'):
            d = np.abs(2.0 * np.log1p(al * R[np.maximum(ix, 0), np.maximum(ia, 0), rows[bb]]))
        dT = np.maximum(dT, np.where(has, d, 0.0))
    return dT, clr


@pytest.mark.parametrize('name', list(ce.SETS))
def test_positive_and_sensitive(name):
    """Positivity: the C oracle has a winner (iA >= 0, T > 0) on EVERY window that holds a site, at every A, on every set (a window
    without a site -- K = 1 where the neighbour is out, the chromosome's ends, A_NONE -- has none by definition), and its nSites
    is the host restatement's.
    Sensitivity: a window is sensitive when removing its farthest in-site, or adding its nearest out-site, moves the winning T by
    at least SENS_FACTOR = 100 times the GPU module's bar 1e-9 |T| + 1e-12.  Sets with a loud row: at least 16 sensitive windows
    per (K, stride).  Span 0: at least half of the windows per (K, stride) -- at the factor 100 for K <= 8, at QUIET_FACTOR = 10 for
    K = 15, 16, 17; both shares are printed for every K.  (At 100 that half cannot be had from K = 15 on without a loud row.  The
    boundary site moves T by 2e-8 |R_b|; the bar is 1e-9 T with T = 2 sum alpha_i R_i over a window whose alphas are 1e-8^(j / K)
    on either side: sum alpha = 0.02 at K = 4, 0.22 at K = 8, 0.93 at K = 16.  100 times the bar asks for |R_b| >= 10 sum alpha times
    the window's alpha-weighted mean R: a site ten times louder than its window's average, in half of the windows.  Measured at
    100: 0.11, 0.16, 0.17 for K = 15, 16, 17.)"""
    layout, span, sizes = ce.SETS[name]
    gen, k, nn, rows, _, _ = ce.dataset(name)
    idx = ce.tests_of(1)
    empty = 0
    for K, A in ce.A_values(layout):
        clr, ix, ia, iA, ns = _single(name)[A]
        want = ce.n_sites(gen, idx, A, ce.exact(Z))
        assert np.array_equal(iA >= 0, want > 0), (name, K, A, np.nonzero((iA >= 0) != (want > 0))[0][:8])
        assert np.array_equal(ns, want) and np.all(clr[want > 0] > 0)
        empty += int(np.sum(want == 0))
    counts, shares, shares100 = {}, {}, {}
    for K in ce.KS:
        sens = np.zeros(ce.N, bool)
        quiet = np.zeros(ce.N, bool)
        for A in [a for kk, a in ce.A_values(layout) if kk == K]:
            dT, T = _delta(name, A, idx)
            bar = 1e-9 * np.abs(T) + 1e-12
            sens |= dT >= ce.SENS_FACTOR * bar
            quiet |= dT >= ce.QUIET_FACTOR * bar
        for s in ce.STRIDES:
            counts[(K, s)] = int(sens[::s].sum())
            shares[(K, s)] = float(quiet[::s].mean())
            shares100[(K, s)] = float(sens[::s].mean())
    print('%s: %d windows without a site over all A; sensitive windows at stride 1 / 5 / 20 per K: %s'
          % (name, empty, ', '.join('%d: %d / %d / %d' % ((K,) + tuple(counts[(K, s)] for s in ce.STRIDES)) for K in ce.KS)))
    if span:
        assert min(counts.values()) >= 16, (name, {c: v for c, v in counts.items() if v < 16})
    else:
        print('%s: share of sensitive windows (stride 1) at factor 10 / at factor 100 per K: %s'
              % (name, ', '.join('%d: %.2f / %.2f' % (K, shares[(K, 1)], shares100[(K, 1)]) for K in ce.KS)))
        low = {c: round(v, 2) for c, v in shares100.items() if c[0] <= 8 and v < 0.5}
        low.update({c: round(v, 2) for c, v in shares.items() if 8 < c[0] <= 17 and v < 0.5})
        assert not low, (name, low)


def test_wrong_restatements_are_noticed():
    """Two deliberately wrong host restatements -- a precomputed reach d <= zcut / A, and the cut taken from a logarithm
    (-np.log(1e-8) = 18.420680743952367, one ulp above the largest z with exp(-z) >= 1e-8) -- must each miss the oracle's nSites:
    the exact comparison of nSites on these inputs notices an error of one ulp in the predicate."""
    wrong = {'d <= zcut / A': ce.by_division(Z), 'zcut = -log(1e-8)': ce.exact(float(-np.log(1e-8)))}
    assert float(-np.log(1e-8)) == np.nextafter(Z, np.inf)
    idx = ce.tests_of(1)
    for what, pred in wrong.items():
        missed = {}
        for name in ('dyadic12', 'decimal12', 'runs12'):
            layout = ce.SETS[name][0]
            gen = ce.dataset(name)[0]
            n = 0
            for K, A in ce.A_values(layout):
                ns = _single(name)[A][4]
                assert np.array_equal(ce.n_sites(gen, idx, A, ce.exact(Z)), ns)
                n += int(np.sum(ce.n_sites(gen, idx, A, pred) != ns))
            missed[name] = n
        print('%s: windows whose nSites differs from the oracle\'s, over all A: %r' % (what, missed))
        assert max(missed.values()) > 0, what
        assert sum(v > 0 for v in missed.values()) >= 1


def test_the_offgrid_constant_is_the_librarys_cut():
    import offgrid
    import test_influence_cpu
    from ballermixplus_amd import power
    assert offgrid.ZCUT == orc.alpha_cut_z() == 18.420680743952364
    assert test_influence_cpu.ZCUT == power.ALPHA_CUT == offgrid.ZCUT
    assert np.exp(-offgrid.ZCUT) >= 1e-8 > np.exp(-np.nextafter(offgrid.ZCUT, np.inf))


@pytest.mark.parametrize('name', list(ce.SETS))
def test_near_ties_of_the_multi_A_scan(name):
    """The multi-A scan (one A per K, no ulp neighbours): the windows whose runner-up A lies within TIE_BAR = 1e-7 of the winner's
    T are left out of the exact comparison of the indices on the GPU; in the oracle alone they are at most TIE_CAP = 5 % of a set."""
    layout = ce.SETS[name][0]
    As = ce.A_list(layout)
    assert len(As) == len(ce.KS) and np.all(np.diff(As) < 0)
    T = np.stack([_single(name)[A][0] for A in As], axis=1)
    tied = ce.near_ties(T)
    gen, k, nn, rows, _, _ = ce.dataset(name)
    idx = ce.tests_of(1)
    multi = c_scan(c_oracle(), _table(name), As, gen, rows, gen[idx], *ce.whole(idx))
    assert np.array_equal(multi[0], T.max(axis=1)) and np.array_equal(multi[3], np.argmax(T, axis=1))
    margin = np.sort(T, axis=1)
    rel = (margin[:, -1] - margin[:, -2]) / margin[:, -1]
    print('%s: %d of %d windows are near-ties between two A; smallest other margin %.3e; winning A (index: windows) %r'
          % (name, int(tied.sum()), ce.N, float(rel[~tied].min()), dict(zip(*[v.tolist() for v in np.unique(multi[3], return_counts=True)]))))
    assert tied.mean() <= ce.TIE_CAP
    assert np.all(multi[3] >= 0)
