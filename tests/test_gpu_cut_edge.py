"""Every restatement of the window cut in bmxscan.hip with a site within one ulp of it (tests/cutedge.py: lattice positions, an A
per neighbour rank K that puts the K-th neighbour on the cut, a loud row that makes a site at the cut visible at the 1e-9 bar).
tests/test_cutedge_cpu.py proves on the CPU that the neighbours do go in and out, that A d <= zcut is the reference's
exp(-A d) >= 1e-8 on every pair used, that every window with a site has a winner, and that two wrong restatements of the cut are
caught by the comparison of nSites made here.

Expected values: the C oracle, which keeps the reference's exp(-A d) >= 1e-8, fed the device's own table (K2 and finalize are what
is checked).  Bar: (x, alpha_beta, A, nSites) exactly equal; np.allclose(clr, oracle, rtol=1e-9, atol=1e-12).  Every test prints its
worst dCLR (in units of the bar, and relative where CLR >= 1) and its wall time."""
import time

import numpy as np
import pytest

import cutedge as ce
from test_gpu_wide_windows import VARIANTS
from util import c_oracle, c_scan, orc

pytestmark = pytest.mark.gpu

N = ce.N
PREPARED, SOLO = 4, 5
PLANS = {1: ('clr_scan_prepared_kernel<16,%s>', 16, PREPARED), 5: ('clr_scan_prepared_kernel<8,%s>', 8, PREPARED),
         20: ('clr_scan_solo_kernel<%s>', 0, SOLO)}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(autouse=True)
def _wall_time(request):
    t0 = time.perf_counter()
    yield
    print('%s: wall time %.2f s' % (request.node.name, time.perf_counter() - t0))


_MODEL = {}


def _model(name):
    if name not in _MODEL:
        from ballermixplus_amd import engine as eng
        gen, k, nn, rows, sizes, span = ce.dataset(name)
        sel_max = float(orc.sel_table('B2', sizes[0], 1, ce.XS, ce.ABETAS)[:, :, ce.LOUD_K].max())
        spect, props = ce.spectrum(sizes, span, sel_max)
        model = eng.ModelArrays('B2', 1, sizes, spect, props, ce.XS, ce.ABETAS)
        assert np.array_equal(model.rows_of(k, nn), rows)
        _MODEL[name] = model
    return _MODEL[name]


class Scanner:
    """One context on one data set.  A is part of the model, so every A list is a set_model of its own (and the sites after it)."""

    def __init__(self, ctx, name):
        self.ctx, self.name = ctx, name
        self.gen, _, _, self.rows, self.sizes, self.span = ce.dataset(name)
        self.lds = 'true' if self.sizes == ce.SMALL else 'false'

    def model(self, As):
        self.ctx.set_model(_model(self.name), list(As))
        self.ctx.set_sites(self.gen, self.rows)

    def table(self):
        """The device's own table (0 on the rows no site can carry), the oracle's input; once per data set."""
        if self.name not in _TABLE:
            R = self.ctx.fetch_lut()[1]
            assert np.isfinite(R[:, :, np.unique(self.rows)]).all()
            R = np.where(np.isfinite(R), R, 0.0)
            if self.span:
                assert abs(float(np.log2(1.0 + R.max())) - (self.span - ce.MARGIN)) < 1e-6
            R.setflags(write=False)
            _TABLE[self.name] = R
        return _TABLE[self.name]

    def scan(self, idx, lo=None, hi=None, plan=None):
        self.ctx.set_tests(self.gen[idx], lo, hi)
        if plan is not None:
            pl = self.ctx.plan()
            kernel, J, mode = PLANS[plan]
            assert (pl['kernel'], pl['mode']) == (kernel % self.lds, mode) and (not J or pl['J'] == J), (self.name, plan, pl)
            assert pl['use_lds'] == (self.lds == 'true'), pl
        self.ctx.scan()
        return [a.copy() for a in self.ctx.fetch()]


_TABLE = {}
_ORACLE = {}


@pytest.fixture
def scanner():
    from ballermixplus_amd import _lib, engine as eng
    assert float(_lib.lib().bmx_alpha_cut()) == ce.zcut()
    made = []

    def make(name):
        ctx = eng.Context(0)
        made.append(ctx)
        return Scanner(ctx, name)

    yield make
    for ctx in made:
        ctx.close()


def _oracle(name, As, R, window=None):
    """The C oracle's scan of EVERY site as a test site with the A list `As` (a tuple), computed once and shared by the strides,
    plans and variants, which take their test sites' rows of it.  window: None (the whole chromosome) or (K, e) for the index
    windows [t - K - e, t + K + e]."""
    key = (name, As, window)
    if key not in _ORACLE:
        gen, _, _, rows, _, _ = ce.dataset(name)
        idx = ce.tests_of(1)
        lo, hi = ce.whole(idx) if window is None else ce.index_windows(idx, *window)
        out = c_scan(c_oracle(), R, list(As), gen, rows, gen[idx], lo, hi)
        for a in out:
            a.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def _check(got, ref, what, keep=None):
    """Integer fields exactly equal (on `keep`, default everywhere), CLR at the bar everywhere.  Returns (the worst |dCLR| in units
    of the bar 1e-9 |CLR| + 1e-12, the worst relative dCLR of the windows with CLR >= 1)."""
    keep = np.ones(len(ref[0]), bool) if keep is None else keep
    for q, field in ((1, 'x'), (2, 'alpha_beta'), (3, 'A'), (4, 'nSites')):
        bad = np.nonzero((got[q] != ref[q]) & keep)[0]
        assert len(bad) == 0, (what, field, len(bad), bad[:8], got[q][bad[:8]], ref[q][bad[:8]])
    err = np.abs(got[0] - ref[0])
    big = ref[0] >= 1.0
    worst = np.array([float(np.max(err / (1e-9 * np.abs(ref[0]) + 1e-12))), float(np.max(err[big] / ref[0][big])) if big.any() else 0.0])
    assert np.allclose(got[0], ref[0], rtol=1e-9, atol=1e-12), (what, worst)
    return worst


def _no_reach(got, what):
    assert not got[0].any() and not got[4].any() and all(np.all(got[q] == -1) for q in (1, 2, 3)), what


# ----------------------------------------------------------------------------- single-A scans on the default plans
@pytest.mark.parametrize('stride', ce.STRIDES)
@pytest.mark.parametrize('name', list(ce.SETS))
def test_single_A_default_plans(name, stride, scanner):
    """Every A of the set's list -- A_in / A_out per K on 'dyadic', the ulp-stepped values around A0(K) elsewhere, and A_NONE -- as a
    scan of its own at stride 1 (prepared J = 16), 5 (prepared J = 8) and 20 (solo), without index bounds; every test site is
    compared, the first and last ones, whose windows the chromosome clips, included."""
    s = scanner(name)
    idx = ce.tests_of(stride)
    worst, winners, sites = np.zeros(2), 0, 0
    for K, A in ce.A_values(ce.SETS[name][0]):
        s.model([A])
        ref = [v[idx] for v in _oracle(name, (A,), s.table())]
        got = s.scan(idx, plan=stride)
        worst = np.maximum(worst, _check(got, ref, (name, stride, K, A)))
        winners += int(np.sum(ref[3] >= 0))
        sites += int(ref[4].sum())
        if K == 0:
            _no_reach(got, (name, stride))
    scans = len(ce.A_values(ce.SETS[name][0]))
    print('%s stride %d: %d scans of %d windows, %d with a winner, %d window sites in all, worst dCLR %.3f of the bar, %.3e relative where CLR >= 1'
          % (name, stride, scans, len(idx), winners, sites, worst[0], worst[1]))
    assert winners >= 0.9 * scans * len(idx)                     # (K = 1 with the neighbour out, and A_NONE, have no winner)


# ----------------------------------------------------------------------------- the variants
@pytest.mark.parametrize('variant', sorted(VARIANTS))
@pytest.mark.parametrize('name', ('decimal12', 'runs12'))
def test_single_A_variants(name, variant, scanner):
    """The same scans, every site a test site, through prepared J = 16 / 8 / 4 (13, 14, 15), solo on request (16), the round-2
    grouped (12) and per-site (2) kernels and the exact products (10)."""
    s = scanner(name)
    s.ctx.set_variant(variant)
    idx = ce.tests_of(1)
    lo, hi = ce.whole(idx)
    kernel, mode = VARIANTS[variant]
    worst = np.zeros(2)
    for K, A in ce.A_values(ce.SETS[name][0]):
        s.model([A])
        ref = _oracle(name, (A,), s.table())
        s.ctx.set_tests(s.gen[idx], lo, hi)
        pl = s.ctx.plan()
        assert kernel is None or (pl['kernel'], pl['mode']) == (kernel, mode), (variant, pl)
        s.ctx.scan()
        got = s.ctx.fetch()
        worst = np.maximum(worst, _check(got, ref, (name, variant, K, A)))
        if K == 0:
            _no_reach(got, (name, variant))
    print('%s variant %d (%s): worst dCLR %.3f of the bar, %.3e relative where CLR >= 1' % (name, variant, kernel, worst[0], worst[1]))


# ----------------------------------------------------------------------------- index bounds at the cut
@pytest.mark.parametrize('stride', (1, 20))
def test_index_bounds_at_the_cut(stride, scanner):
    """Index windows [t - K, t + K], [t - K + 1, t + K - 1] and [t - K - 1, t + K + 1] at the A values of that K: the window's bound
    coincides with, lies inside, or lies outside the site the cut decides (n_j = min(sites up to the bound, sites the cut lets in))."""
    name = 'decimal12'
    s = scanner(name)
    idx = ce.tests_of(stride)
    worst, cut, bound = np.zeros(2), 0, 0
    for K, A in ce.A_values('decimal'):
        if K == 0:
            continue
        s.model([A])
        free = _oracle(name, (A,), s.table())[4][idx]
        for e in (0, -1, 1):
            lo, hi = ce.index_windows(idx, K, e)
            ref = [v[idx] for v in _oracle(name, (A,), s.table(), (K, e))]
            got = s.scan(idx, lo, hi, plan=stride)
            worst = np.maximum(worst, _check(got, ref, (stride, K, A, e)))
            cut += int(np.sum(ref[4] == free))
            bound += int(np.sum(ref[4] < free))
    print('index bounds, stride %d: nSites decided by the cut in %d windows, by the index bound in %d; worst dCLR %.3f of the bar, %.3e relative where CLR >= 1' % (stride, cut, bound, worst[0], worst[1]))
    assert cut > 1000 and bound > 1000


# ----------------------------------------------------------------------------- the multi-A scan
@pytest.mark.parametrize('stride', ce.STRIDES)
@pytest.mark.parametrize('name', list(ce.SETS))
def test_multi_A_scan_and_profile(name, stride, scanner):
    """One A per K in one scan with the A profile on: every profile column against the oracle's scan with that A alone at the bar;
    max_v profile == CLR bit for bit; the scan's own rows against the oracle's multi-A scan (indices exact except where the
    runner-up A lies within 1e-7 T of the winner -- at most 5 % of the windows --, nSites exact there too); everything bitwise equal
    with the profiles off."""
    s = scanner(name)
    As = tuple(ce.A_list(ce.SETS[name][0]))
    idx = ce.tests_of(stride)
    s.model(As)
    R = s.table()
    off = s.scan(idx, plan=stride)
    s.ctx.set_profiles('A')
    on = s.scan(idx, plan=stride)
    prof = s.ctx.fetch_profile('A')
    for a, b in zip(off, on):
        assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
    assert prof.shape == (len(idx), len(As)) and np.all(prof >= 0.0)
    assert np.array_equal(_bits(prof.max(axis=1)), _bits(on[0]))
    cols = np.stack([_oracle(name, (A,), R)[0][idx] for A in As], axis=1)
    col_worst = float(np.max(np.abs(prof - cols) / (1e-9 * np.abs(cols) + 1e-12)))
    for v, A in enumerate(As):
        assert np.allclose(prof[:, v], cols[:, v], rtol=1e-9, atol=1e-12), (name, stride, ce.KS[v], A)
    tied = ce.near_ties(cols)
    ref = [v[idx] for v in _oracle(name, As, R)]
    assert np.array_equal(ref[0], cols.max(axis=1)) and np.all(ref[3] >= 0)
    worst = _check(on, ref, (name, stride, 'multi-A'), keep=~tied)
    print('%s stride %d, %d A values: %d near-ties left out, winning A (index: windows) %r, worst profile column %.3f of the bar, worst dCLR %.3f of the bar, %.3e relative where CLR >= 1'
          % (name, stride, len(As), int(tied.sum()), dict(zip(*[v.tolist() for v in np.unique(ref[3], return_counts=True)])), col_worst, worst[0], worst[1]))
    assert tied.mean() <= ce.TIE_CAP


# ----------------------------------------------------------------------------- bmx_ctx_eval_points
@pytest.mark.parametrize('name', ('dyadic12', 'decimal12'))
def test_eval_points_at_the_cut(name, scanner):
    """The refine family's range search: every site a test site, and per K every test site takes every ulp-stepped A of that K in
    turn (test site t takes value (t + shift) mod n in call `shift`), at the fixed grid point EVAL_POINT.  nSites exactly the host
    restatement's (A d <= zcut, one multiplication); T within 1e-9 |T| of the host's 2 sum log1p(alpha R) over those sites (the
    bar of test_gpu_refine.check_refined, which test_gpu_offgrid.py applies to this entry point), R being the device's own table."""
    s = scanner(name)
    layout = ce.SETS[name][0]
    s.model(ce.A_list(layout))
    Rp = s.table()[ce.EVAL_POINT[0], ce.EVAL_POINT[1]]
    x, ab = ce.XS[ce.EVAL_POINT[0]], ce.ABETAS[ce.EVAL_POINT[1]]
    idx = ce.tests_of(1)
    s.ctx.set_tests(s.gen[idx])
    inside = ce.exact(ce.zcut())
    worst, calls, edge = 0.0, 0, 0
    for K in ce.KS + (0,):
        vals = np.array([A for k, A in ce.A_values(layout) if k == K])
        for shift in range(len(vals)):
            A = vals[(idx + shift) % len(vals)]
            T, ns = s.ctx.eval_points(A, x, ab)
            want, wn = ce.host_T(s.gen, s.rows, Rp, idx, A, inside)
            bad = np.nonzero(ns != wn)[0]
            assert len(bad) == 0, (name, K, shift, len(bad), bad[:8], ns[bad[:8]], wn[bad[:8]])
            has = wn > 0
            assert np.all(np.isneginf(T[~has])) and np.all(np.isfinite(T[has]))
            err = np.abs(T[has] - want[has]) / np.abs(want[has])
            assert np.all(err <= 1e-9), (name, K, shift, float(err.max()))
            worst = max(worst, float(err.max())) if has.any() else worst
            calls += 1
            if K:
                edge += int(np.sum(wn != np.minimum(idx, K) + np.minimum(N - 1 - idx, K)))
    print('%s: %d eval_points calls of %d points, %d windows without their K-th neighbour on one side or both, worst relative dT %.3e' % (name, calls, N, edge, worst))
    assert edge > 1000


# ----------------------------------------------------------------------------- bmx_ctx_plant_sites
def test_planting_range_at_the_cut(scanner):
    """plant_range_kernel and plant_kernel on 'dyadic': around centres on lattice positions the run of sites in reach is exactly
    2 K + 1 sites at A_in(K) and 2 K - 1 at A_out(K), clipped at the chromosome's ends, and every site whose row changed lies in
    that run and is not the centre's."""
    from ballermixplus_amd import power
    name = 'dyadic12'
    s = scanner(name)
    As = [A for K, A in ce.A_values('dyadic') if K]
    s.model(As)
    model = _model(name)
    R = s.table()
    gw =power.allowed_rows('B2', 1, model.sizes, model.row_off, model.g)
    cidx = np.array([1, 600, 1200, 1800, 2400, 3000, 3600, N - 2])
    changed_all, clipped, undecided, redrawn = 0, 0, 0, 0
    for iA, (K, A) in enumerate([v for v in ce.A_values('dyadic') if v[0]]):
        reachK = K if iA % 2 == 0 else K - 1                      # A_in, A_out
        assert A == As[iA] and np.all(A * np.diff(s.gen[cidx]) > 2.000001 * ce.zcut())
        s.ctx.select_slot(1)
        first, count, changed = s.ctx.plant_sites(0, 1000 + iA, s.gen[cidx], iA, 2, 1, gw)
        g, r = s.ctx.fetch_sites(N)
        s.ctx.select_slot(0)
        lo, hi = np.maximum(cidx - reachK, 0), np.minimum(cidx + reachK, N - 1)
        assert np.array_equal(first, lo) and np.array_equal(count, hi - lo + 1), (K, A, first, count)
        assert np.array_equal(_bits(g), _bits(s.gen))
        moved = np.nonzero(r != s.rows)[0]
        allowed = np.zeros(N, bool)
        for a, b in zip(lo, hi):
            allowed[a:b + 1] = True
        allowed[cidx] = False
        assert np.all(allowed[moved]) and changed == len(moved), (K, A, moved[~allowed[moved]][:8])
        # ... and the rows are the host restatement's (power.planted_rows on the device's table) on every site it decides: a
        # site on the cut is redrawn exactly when A d <= zcut
        want, margin = power.planted_rows(s.gen, s.rows, model.sizes, model.row_off, R[2, 1], gw, A, s.gen[cidx], 1000 + iA, ce.zcut())
        drawn = np.isfinite(margin)
        assert np.array_equal(drawn, allowed) and np.array_equal(r[~drawn], s.rows[~drawn])
        decided = margin > power.MARGIN
        assert np.array_equal(r[decided], want[decided])
        undecided += int(np.sum(~decided))
        redrawn += int(drawn.sum())
        assert drawn.sum() == np.sum(np.maximum(hi - lo, 0))     # (K = 1 at A_out: the centres alone, nothing to redraw)
        changed_all += len(moved)
        clipped += int(np.sum(count < 2 * reachK + 1))
    print('planting: %d calls of %d centres, %d clipped runs, %d sites redrawn (%d not decided by more than power.MARGIN), %d rows changed'
          % (len(As), len(cidx), clipped, redrawn, undecided, changed_all))
    assert changed_all > 1000 and clipped > 20 and undecided <= 0.01 * redrawn
