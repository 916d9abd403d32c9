"""The scan kernels across grid shapes and exact argmax ties (tests/gridshape.py).  Every kernel puts the (x, alpha_beta) pairs on
lanes, 64 per slice; the shapes are chosen around the slice count and the real lanes of the last slice:

    pairs  (nx, nab)           what it hits
       10  (10, 1)             the CLI's --fixAlpha; nab = 1
       51  (1, 51)             the CLI's --fixX; nx = 1
       63  (7, 9)              one slice, one pad lane
       64  (64, 1), (1, 64)    one full slice, no pad lane
       65  (5, 13)             two slices, ONE real lane in the last
      128  (2, 64)             two full slices
      129  (3, 43)             three slices, one real lane in the last, nab does not divide 64
      576  (9, 64)             9 slices: the first count past the 8 XCDs
     1024  (16, 64)            16 full slices
     1037  (17, 61)            17 slices, 13 real lanes in the last, nab does not divide 64, an x value's pairs straddle slices

Test sites: 613 consecutive sites (prepared J = 16: ten workgroup chunks), every 5th site (801: prepared J = 8, nine chunks) and
every 20th (201: solo, thirteen chunks) -- more than eight chunks each and a partial last group, so the XCD decode of the
block index wraps and the padded tail of the launch runs; whole-chromosome and ragged index windows (some empty).  The data hold a
stretch whose windows have NO grid point with T > 0: the windows a pad lane (R = 0, product exactly 1) or a stale lane would steal.
tests/test_gridshape_cpu.py proves all of that with the oracles alone.

Bar, everywhere (that of tests/test_gpu_table_span.py): every result finite; (x, alpha_beta, A, nSites) exactly equal on every
window that is not in gridshape.TIED, with the count of differing windows asserted to be 0; np.allclose(clr, oracle, rtol=1e-9,
atol=1e-12) on EVERY window; windows where the oracle has no winner give exactly clr == 0.0, iA == ix == ia == -1, nSites == 0.
The oracle is fed the device's own table (K2 alone is compared).

On the tie grid (repeated x, alpha_beta and A values: bit-identical table columns) NO window of a duplicate class is excepted: the
first copy in (A, x, alpha_beta) order must win everywhere."""
import numpy as np
import pytest

import gridshape as gs
from util import c_oracle, c_scan

pytestmark = pytest.mark.gpu

N = gs.N
PREPARED, SOLO, PER_SITE = 4, 5, -1


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


_SITES, _MODEL, _TABLE, _ORACLE = {}, {}, {}, {}


def _sites(data):
    if data not in _SITES:
        _SITES[data] = gs.chromosome(data)
    return _SITES[data]


def _model(data, kind):
    if (data, kind) not in _MODEL:
        from ballermixplus_amd import engine as eng
        gen, k, nn = _sites(data)
        spect, props = gs.spectrum(data)
        xs, ab, _ = gs.grids(kind)
        model = eng.ModelArrays('B2', 1, gs.sizes_of(data), spect, props, xs, ab)
        rows = model.rows_of(k, nn)
        assert np.array_equal(rows, gs.rows_of(data))
        _MODEL[(data, kind)] = (model, rows)
    return _MODEL[(data, kind)]


@pytest.fixture
def open_ctx():
    """open_ctx(data set, shape or 'tie') -> (context with that model and the data set's sites, the device's own table with 0 on
    the rows no site can carry); every context a test opened is closed when the test ends, however it ends."""
    from ballermixplus_amd import engine as eng
    made = []

    def make(data, kind):
        model, rows = _model(data, kind)
        ctx = eng.Context(0)
        made.append(ctx)
        ctx.set_model(model, gs.grids(kind)[2])
        ctx.set_sites(_sites(data)[0], rows)
        if (data, kind) not in _TABLE:
            R = ctx.fetch_lut()[1]
            assert np.isfinite(R[:, :, np.unique(rows)]).all()
            R = np.where(np.isfinite(R), R, 0.0)
            R.setflags(write=False)
            _TABLE[(data, kind)] = R
        return ctx, _TABLE[(data, kind)]

    yield make
    for ctx in made:
        ctx.close()


def _windows(data, stride, windows):
    idx = gs.tests_of(stride)
    return (idx,) + gs.windows_of(_sites(data)[0], idx, windows)


def _oracle(data, kind, stride, windows, R):
    """One oracle run per (data set, grid, test sites, windows), shared by plans, variants and tests."""
    key = (data, kind, stride, windows)
    if key not in _ORACLE:
        gen = _sites(data)[0]
        idx, lo, hi = _windows(data, stride, windows)
        out = c_scan(c_oracle(), R, gs.grids(kind)[2], gen, _model(data, kind)[1], gen[idx], lo, hi)
        for a in out:
            a.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def _set_tests(ctx, data, stride, windows):
    idx, lo, hi = _windows(data, stride, windows)
    if windows == 'all':
        ctx.set_tests(_sites(data)[0][idx])                      # no index bounds: the reference's default mode
    else:
        ctx.set_tests(_sites(data)[0][idx], lo, hi)
    return idx, lo, hi


def _scan(ctx, data, stride, windows):
    _set_tests(ctx, data, stride, windows)
    ctx.scan()
    return [a.copy() for a in ctx.fetch()]


def _check(got, ref, what, nslices, tied=()):
    keep = np.ones(len(ref[0]), bool)
    keep[list(tied)] = False
    bad = int(np.sum(~np.isfinite(got[0])))
    worst = float(np.max(np.abs(got[0] - ref[0]) / np.maximum(np.abs(ref[0]), 1e-300)))
    ties = int(np.sum(np.any([got[q][keep] != ref[q][keep] for q in (1, 2, 3, 4)], axis=0)))
    none = ref[3] < 0
    print('%s: %d windows (%d skipped, %d without a winner), %d slices, nSites %d .. %d, CLR %.3g .. %.3g, not finite %d, ties %d, worst relative dCLR %.3e'
          % (what, len(ref[0]), len(tied), int(none.sum()), nslices, ref[4].min(), ref[4].max(), ref[0].min(), ref[0].max(), bad, ties, worst))
    assert bad == 0, (what, bad, got[0][~np.isfinite(got[0])][:4])
    assert len(tied) <= 0.02 * len(keep) and none.sum() >= 5 and (~none).sum() >= 100
    for q, name in ((1, 'x'), (2, 'alpha_beta'), (3, 'A'), (4, 'nSites')):
        assert np.array_equal(got[q][keep], ref[q][keep]), (what, name, np.where(got[q] != ref[q])[0][:8])
    assert ties == 0
    assert np.allclose(got[0], ref[0], rtol=1e-9, atol=1e-12), (what, worst)
    z = none & keep
    assert np.all(got[0][z] == 0.0) and np.all(got[1][z] == -1) and np.all(got[2][z] == -1) and np.all(got[3][z] == -1) and np.all(got[4][z] == 0), what


def _nslices(kind):
    nx, nab = gs.TIE_SHAPE if kind == 'tie' else kind
    return -(-nx * nab // 64)


def _default_plan(stride, lds):
    if stride <= 5:
        return ('clr_scan_prepared_kernel<%d,%s>' % (16 if stride == 1 else 8, lds), PREPARED)
    return ('clr_scan_solo_kernel<%s>' % lds, SOLO)


def _expect_default_plan(ctx, stride, lds, what):
    pl = ctx.plan()
    assert (pl['kernel'], pl['mode']) == _default_plan(stride, lds), (what, pl)
    assert pl['use_lds'] == (lds == 'true')


def _check_records(ctx, got, kind):
    nx, nab = gs.TIE_SHAPE if kind == 'tie' else kind
    rec = ctx.fetch_records()
    want = np.where(got[3] >= 0, (got[3] * nx + got[1]) * nab + got[2], -1)
    assert np.array_equal(rec['lin'], want) and np.array_equal(rec['nsites'], got[4]) and np.array_equal(_bits(rec['clr']), _bits(got[0]))
    assert np.all((got[1] >= -1) & (got[1] < nx) & (got[2] >= -1) & (got[2] < nab))


@pytest.mark.parametrize('windows', ('all', 'ragged'))
@pytest.mark.parametrize('stride', gs.STRIDES)
@pytest.mark.parametrize('shape', gs.SHAPES, ids=lambda s: '%dx%d' % s)
def test_default_plans(shape, stride, windows, open_ctx):
    """Dense -> clr_scan_prepared_kernel<16,true>, stride 5 -> <8,true>, stride 20 -> clr_scan_solo_kernel<true>, on every shape;
    the records' linear index is (iA * nx + ix) * nab + ia of the separate arrays."""
    what = '%dx%d stride %d %s' % (shape + (stride, windows))
    ctx, R = open_ctx('small', shape)
    _set_tests(ctx, 'small', stride, windows)
    _expect_default_plan(ctx, stride, 'true', what)
    ctx.scan()
    got = ctx.fetch()
    _check(got, _oracle('small', shape, stride, windows, R), what, _nslices(shape), gs.TIED.get(('small', shape, stride, windows), ()))
    _check_records(ctx, got, shape)


@pytest.mark.parametrize('stride', (1, 5))
@pytest.mark.parametrize('shape', gs.L2_SHAPES, ids=lambda s: '%dx%d' % s)
def test_table_in_l2(shape, stride, open_ctx):
    """Sample sizes 150, 160, 170: the R slice does not fit in LDS, so the <J, false> prepared forms run."""
    what = 'large %dx%d stride %d' % (shape + (stride,))
    ctx, R = open_ctx('large', shape)
    assert R.shape[2] == 483
    _set_tests(ctx, 'large', stride, 'all')
    _expect_default_plan(ctx, stride, 'false', what)
    ctx.scan()
    _check(ctx.fetch(), _oracle('large', shape, stride, 'all', R), what, _nslices(shape), gs.TIED.get(('large', shape, stride, 'all'), ()))


VARIANTS = {12: ('clr_scan_grouped_kernel<16,true,3>', 3), 2: ('clr_scan_kernel<true>', PER_SITE), 16: ('clr_scan_solo_kernel<true>', SOLO),
            10: ('clr_scan_grouped_kernel<16,true,2>', 2)}


@pytest.mark.parametrize('variant', sorted(VARIANTS))
@pytest.mark.parametrize('shape', gs.VARIANT_SHAPES, ids=lambda s: '%dx%d' % s)
def test_round2_and_diagnostic_variants(shape, variant, open_ctx):
    """The round-2 grouped kernel (12: blockIdx.x % nslices, per-slice rowmax), the per-site kernel (2), solo on request (16) and
    the exact-product form (10) on the dense test sites."""
    ctx, R = open_ctx('small', shape)
    ctx.set_variant(variant)
    _set_tests(ctx, 'small', 1, 'all')
    pl = ctx.plan()
    assert (pl['kernel'], pl['mode']) == VARIANTS[variant], (variant, pl)
    ctx.scan()
    _check(ctx.fetch(), _oracle('small', shape, 1, 'all', R), 'variant %d %dx%d dense' % ((variant,) + shape), _nslices(shape),
           gs.TIED.get(('small', shape, 1, 'all'), ()))


def _surface_atol(R):
    """A sum of W <= N terms 2 log1p(alpha R), each at most 2 max|log1p(R)| in size, summed in another order than the oracle's:
    N eps times the largest term."""
    return N * np.finfo(np.float64).eps * 2.0 * float(np.max(np.abs(np.log1p(R[R > -1.0]))))


def _sample(n_tests, count):
    """`count` test-site indices spread over the whole list, the stretch without winners included."""
    return np.unique(np.linspace(0, n_tests - 1, count).astype(np.int64))


def _profile_reference(T, nA, nx, nab):
    """max(0, the largest T over the other two grids) from a surface T[n][nA][nx][nab] with NaN where the window is empty."""
    t = np.where(np.isnan(T), -np.inf, T)
    return {'A': np.maximum(t.max(axis=(2, 3)), 0.0), 'x': np.maximum(t.max(axis=(1, 3)), 0.0), 'abeta': np.maximum(t.max(axis=(1, 2)), 0.0)}


@pytest.mark.parametrize('stride', gs.STRIDES)
@pytest.mark.parametrize('shape', gs.PROFILE_SHAPES, ids=lambda s: '%dx%d' % s)
def test_profiles(shape, stride, open_ctx):
    """All three profiles: the scan's fields stay bitwise those of the scan without profiles, max_v profile == clr bit for bit on
    every window, and every entry of a sample of windows is the maximum over the other two grids of the device's own surface
    (allclose as above; 0 where no T > 0): the [M][NP] keys and the o + ix * nab strides with nab not dividing 64 and 17 slices."""
    what = 'profiles %dx%d stride %d' % (shape + (stride,))
    ctx, R = open_ctx('small', shape)
    off = _scan(ctx, 'small', stride, 'all')
    ctx.set_profiles(['A', 'x', 'abeta'])
    on = _scan(ctx, 'small', stride, 'all')
    _expect_default_plan(ctx, stride, 'true', what)
    for a, b in zip(off, on):
        assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
    _check(on, _oracle('small', shape, stride, 'all', R), what, _nslices(shape), gs.TIED.get(('small', shape, stride, 'all'), ()))
    prof = {k: ctx.fetch_profile(k) for k in ('A', 'x', 'abeta')}
    nA, (nx, nab) = len(gs.A_LIST), shape
    pick = _sample(len(on[0]), 48)
    assert len(pick) >= 40
    T, ns = ctx.surfaces(pick)
    want = _profile_reference(T, nA, nx, nab)
    for name, n in (('A', nA), ('x', nx), ('abeta', nab)):
        p = prof[name]
        assert p.shape == (len(on[0]), n) and np.isfinite(p).all() and np.all(p >= 0.0), name
        assert np.array_equal(_bits(p.max(axis=1)), _bits(on[0])), name
        worst = float(np.max(np.abs(p[pick] - want[name])))
        print('%s, profile %s: %d windows sampled, %d entries at 0, worst absolute difference to the surface %.3e' % (what, name, len(pick), int((want[name] == 0).sum()), worst))
        assert np.allclose(p[pick], want[name], rtol=1e-9, atol=1e-12), (name, worst)
        assert np.all(p[pick][want[name] == 0.0] <= 1e-12)
        assert (want[name] == 0).any() and (want[name] > 0).any()
    assert np.all(on[0][pick][np.all(want['A'] == 0, axis=1)] == 0.0)


@pytest.mark.parametrize('windows', ('all', 'ragged'))
@pytest.mark.parametrize('shape', gs.SURFACE_SHAPES, ids=lambda s: '%dx%d' % s)
def test_surfaces(shape, windows, open_ctx):
    """bmx_ctx_surface and bmx_ctx_surfaces (slices of 64 and of 256 pairs) against the oracle's 2 sum log1p(alpha R) per grid point
    (orc_surface_sums on the device's table): relative 1e-9 as test_device_likelihood_surface_matches_reference, plus the rounding
    of a sum of N terms where T cancels to near 0; NaN exactly where the oracle's window at that A is empty; the window sizes
    equal; the two entry points bitwise equal."""
    ctx, R = open_ctx('small', shape)
    gen = _sites('small')[0]
    idx, lo, hi = _set_tests(ctx, 'small', 20, windows)
    pick = _sample(len(idx), 24)
    S, ns = gs.surface_sums(c_oracle(), R, gs.A_LIST, gen, _model('small', shape)[1], gen[idx[pick]], lo[pick], hi[pick])
    ref = np.where((ns == 0)[:, :, None], np.nan, 2.0 * S).reshape(len(pick), len(gs.A_LIST), shape[0], shape[1])
    many, ns_many = ctx.surfaces(pick)
    assert np.array_equal(ns_many, ns)
    assert np.array_equal(np.isnan(many), np.isnan(ref))
    if windows == 'ragged':
        assert np.isnan(ref).any() and np.all(np.isnan(ref).all(axis=(2, 3)) | ~np.isnan(ref).any(axis=(2, 3)))
    ok = ~np.isnan(ref)
    atol = _surface_atol(R)
    err = np.abs(many[ok] - ref[ok])
    pos = ref[ok] > 0
    worst_rel = float(np.max(err[pos] / ref[ok][pos]))
    print('surfaces %dx%d %s: %d windows, %d grid points, %d empty (window, A), worst relative difference where T > 0 %.3e, worst absolute %.3e (atol %.1e)'
          % (shape[0], shape[1], windows, len(pick), int(ok.sum()), int((ns == 0).sum()), worst_rel, float(err.max()), atol))
    assert np.all(err <= 1e-9 * np.abs(ref[ok]) + atol)
    for j, t in enumerate(pick):
        one, ns_one = ctx.surface(gen[idx[t]], lo[t], hi[t])
        assert np.array_equal(_bits(one), _bits(many[j])) and np.array_equal(ns_one, ns_many[j]), t


@pytest.mark.parametrize('stride', gs.STRIDES)
@pytest.mark.parametrize('shape', gs.REPEAT_SHAPES, ids=lambda s: '%dx%d' % s)
def test_two_scans_are_bitwise_equal(shape, stride, open_ctx):
    """Two scans of one context, and a context that has never scanned anything else."""
    ctx, _ = open_ctx('small', shape)
    first = _scan(ctx, 'small', stride, 'ragged')
    ctx.scan()
    again = ctx.fetch()
    fresh, _ = open_ctx('small', shape)
    other = _scan(fresh, 'small', stride, 'ragged')
    for b in (again, other):
        assert np.array_equal(_bits(first[0]), _bits(b[0]))
        for q in (1, 2, 3, 4):
            assert np.array_equal(first[q], b[q])
    assert np.isfinite(first[0]).all()


# ----------------------------------------------------------------------------- exact ties
def _check_table_ties(R):
    nx, nab = gs.TIE_SHAPE
    cls = gs.class_of()
    for p in range(nx * nab):
        q = int(cls[p])
        assert np.array_equal(_bits(R[p // nab, p % nab]), _bits(R[q // nab, q % nab])), p       # the device's table columns of repeated values


def _check_first_copy(got, ref, what):
    """The winner is the oracle's on EVERY window outside gridshape.TIED (near-ties between different classes): within a class the
    first copy wins."""
    cls = gs.class_of()
    npairs = gs.TIE_SHAPE[0] * gs.TIE_SHAPE[1]
    w = ref[3] >= 0
    lin = (ref[3] * gs.TIE_SHAPE[0] + ref[1]) * gs.TIE_SHAPE[1] + ref[2]
    assert np.array_equal(cls[lin[w]], lin[w]), what                                            # the oracle's winner is a first copy
    across = int(np.sum([len({(m % npairs) // 64 for m in gs.members_of(c)}) > 1 for c in lin[w]]))
    print('%s: %d winners, %d of a class with copies in both slices, winning A %r' % (what, int(w.sum()), across, np.bincount(ref[3][w], minlength=6).tolist()))
    assert across >= 0.25 * len(lin) and np.all(ref[3][w] < 3)


TIE_CASES = [('small', s, w) for s in gs.STRIDES for w in ('all', 'ragged')] + [('large', 1, 'all'), ('large', 5, 'all')]


@pytest.mark.parametrize('data,stride,windows', TIE_CASES)
def test_exact_ties(data, stride, windows, open_ctx):
    """Repeated x, alpha_beta and A values under the default plans, table in LDS and in L2: (x, alpha_beta, A) equal to the oracle's
    on every window -- the first copy in (A, x, alpha_beta) order wins whether the other copies sit in the same slice, in the
    other slice at a lower lane, or at a later A; no allowance for the duplicate classes (gridshape.TIED lists only near-ties
    between DIFFERENT classes, and has none for these cases)."""
    what = 'ties %s stride %d %s' % (data, stride, windows)
    ctx, R = open_ctx(data, 'tie')
    _check_table_ties(R)
    idx, lo, hi = _set_tests(ctx, data, stride, windows)
    _expect_default_plan(ctx, stride, 'true' if data == 'small' else 'false', what)
    ctx.scan()
    got = ctx.fetch()
    ref = _oracle(data, 'tie', stride, windows, R)
    tied = gs.TIED.get((data, 'tie', stride, windows), ())
    assert len(tied) == 0
    _check(got, ref, what, 2, tied)
    _check_first_copy(got, ref, what)
    _check_records(ctx, got, 'tie')
    # the device's surface shows the copies bit-identical (NaN where the window is empty: the same bits too)
    pick = _sample(len(idx), 24)
    T, ns = ctx.surfaces(pick)
    flat = T.reshape(len(pick), -1)
    assert np.array_equal(_bits(flat), _bits(flat[:, gs.class_of()])), what


@pytest.mark.parametrize('stride', gs.STRIDES)
def test_profiles_on_the_tie_grid(stride, open_ctx):
    """Repeated values of a coordinate have bit-identical profile entries, and the maximum is still the CLR bit for bit."""
    ctx, R = open_ctx('small', 'tie')
    ctx.set_profiles(['A', 'x', 'abeta'])
    on = _scan(ctx, 'small', stride, 'all')
    _check(on, _oracle('small', 'tie', stride, 'all', R), 'profiles on the tie grid, stride %d' % stride, 2)
    for name, index in (('A', gs.TIE_A_IDX), ('x', gs.TIE_X_IDX), ('abeta', gs.TIE_AB_IDX)):
        p = ctx.fetch_profile(name)
        first = [index.index(v) for v in index]
        assert first != list(range(len(index)))
        assert np.array_equal(_bits(p), _bits(p[:, first])), name
        assert np.array_equal(_bits(p.max(axis=1)), _bits(on[0])) and (p > 0).any(), name


@pytest.mark.parametrize('variant', (12, 2))
def test_exact_ties_round2_variants(variant, open_ctx):
    """The round-2 grouped kernel (12) and the per-site kernel (2) classify far sites by a PER-SLICE rowmax, so copies of a grid
    point in different slices may take different arithmetic paths and round differently.  For these two variants the exact
    first-copy rule is required only among the copies within one slice (the winner is the first member of its class in ITS slice,
    the earlier A copy included); across slices the winner must be a member of the oracle's winning class, with nSites equal and
    the CLR within the bar above."""
    ctx, R = open_ctx('small', 'tie')
    ctx.set_variant(variant)
    _set_tests(ctx, 'small', 1, 'all')
    pl = ctx.plan()
    assert (pl['kernel'], pl['mode']) == VARIANTS[variant], pl
    ctx.scan()
    got = ctx.fetch()
    ref = _oracle('small', 'tie', 1, 'all', R)
    cls = gs.class_of()
    nx, nab = gs.TIE_SHAPE
    npairs = nx * nab
    assert np.isfinite(got[0]).all() and np.allclose(got[0], ref[0], rtol=1e-9, atol=1e-12)
    assert np.array_equal(got[3] < 0, ref[3] < 0) and np.array_equal(got[4], ref[4])
    w = ref[3] >= 0
    lin_d = ((got[3] * nx + got[1]) * nab + got[2])[w]
    lin_o = ((ref[3] * nx + ref[1]) * nab + ref[2])[w]
    assert np.array_equal(cls[lin_d], lin_o)                                                     # a member of the oracle's winning class
    moved = 0
    for d in lin_d:
        mates = [m for m in gs.members_of(cls[d]) if (m % npairs) // 64 == (d % npairs) // 64]
        assert d == min(mates), (d, mates)                                                       # first copy within its slice
        moved += d != cls[d]
    z = ~w
    assert z.sum() >= 5 and np.all(got[0][z] == 0.0) and np.all(got[1][z] == -1) and np.all(got[2][z] == -1)
    print('variant %d on the tie grid: %d winners, %d of them a copy in the other slice than the first' % (variant, int(w.sum()), moved))
