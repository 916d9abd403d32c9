"""The scan kernels on wide, uneven windows past their stream caps (tests/widewin.py: a cold-spot chromosome whose A = 100 windows
hold up to 46 000 sites, a run of 500 tied positions, a planted signal that makes the wide A win).  tests/test_widewin_cpu.py
proves on the CPU that these inputs exceed P_FAR_CAP, S_FAR_CAP / FAR_CAP, SER_CAP and MID_CAP and take the exponent-budget
split; here every plan and variant is compared with the C oracle on them.

Bar, unless a test says otherwise: (x, alpha_beta, A, nSites) exactly equal on every window, no tie exemption;
np.allclose(clr, oracle, rtol=1e-9, atol=1e-12) with the oracle fed the device's own table (K2 alone, as the other randomised
tests).  The own-table test feeds the oracle the table the oracle builds and takes test_gpu_round4.py's bound."""
import functools

import numpy as np
import pytest

import widewin as ww
from util import c_oracle, c_scan, oracle_R, orc

pytestmark = pytest.mark.gpu

N = ww.N
PREPARED, SOLO = 4, 5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _sel(n):
    return orc.sel_table('B2', n, 1, [ww.PLANT_X], [ww.PLANT_ABETA])[0, 0]


@functools.lru_cache(maxsize=None)
def _data(kind):
    from ballermixplus_amd import engine as eng
    from ballermixplus_amd.hostmodel import Grids
    gen, k, nn, _ = ww.chromosome(kind, _sel)
    spect, props = ww.spectrum(kind)
    sizes, _ = ww.sizes_and_props(kind)
    xs, ab, _ = Grids(None, None, True, False, None, '100').scan_order()
    model = eng.ModelArrays('B2', 1, sizes, spect, props, xs, ab)
    return dict(gen=gen, k=k, nn=nn, spect=spect, props=props, sizes=sizes, xs=xs, ab=ab, model=model, rows=model.rows_of(k, nn))


def _As(alist):
    from ballermixplus_amd.hostmodel import Grids
    return Grids(None, None, True, False, None, alist).scan_order()[2]


@pytest.fixture
def open_ctx():
    """open_ctx(kind, A list) -> a context with that data set's model and sites; every context a test opened is closed when the
    test ends, however it ends."""
    from ballermixplus_amd import engine as eng
    made = []

    def make(kind, alist):
        d = _data(kind)
        ctx = eng.Context(0)
        made.append(ctx)
        ctx.set_model(d['model'], _As(alist))
        ctx.set_sites(d['gen'], d['rows'])
        return ctx

    yield make
    for ctx in made:
        ctx.close()


_TABLE = {}


def _device_table(kind, ctx):
    """The device's own table, the oracle's input wherever K2 alone is checked (rows no site can carry: 0)."""
    if kind not in _TABLE:
        R = ctx.fetch_lut()[1]
        _TABLE[kind] = np.where(np.isfinite(R), R, 0.0)
        d = _data(kind)
        assert len(d['xs']) * len(d['ab']) == 440 and np.isfinite(R[:, :, np.unique(d['rows'])]).all()
    return _TABLE[kind]


@functools.lru_cache(maxsize=None)
def _own_table():
    d = _data('lds')
    return oracle_R('B2', d['sizes'], 1, d['spect'], d['props'], d['xs'], d['ab'])


_ORACLE = {}


def _oracle(kind, alist, idx, lo, hi, R, table='device'):
    """One oracle run per (data set, A list, test sites and windows, table), shared by plans and variants."""
    key = (kind, alist, table, idx.tobytes(), lo.tobytes(), hi.tobytes())
    if key not in _ORACLE:
        d = _data(kind)
        out = c_scan(c_oracle(), R, _As(alist), d['gen'], d['rows'], d['gen'][idx], lo, hi)
        for a in out:
            a.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def _whole(idx):
    return np.zeros(len(idx), np.int64), np.full(len(idx), N - 1, np.int64)


def _scan(ctx, kind, idx, lo, hi):
    ctx.set_tests(_data(kind)['gen'][idx], lo, hi)
    ctx.scan()
    return [a.copy() for a in ctx.fetch()]


def _check(got, ref, what):
    worst = float(np.max(np.abs(got[0] - ref[0]) / np.maximum(np.abs(ref[0]), 1e-300)))
    print('%s: %d windows, nSites %d .. %d, CLR %.1f .. %.1f, worst relative dCLR %.3e'
          % (what, len(ref[0]), ref[4].min(), ref[4].max(), ref[0].min(), ref[0].max(), worst))
    for q, name in ((1, 'x'), (2, 'alpha_beta'), (3, 'A'), (4, 'nSites')):
        assert np.array_equal(got[q], ref[q]), (what, name, np.where(got[q] != ref[q])[0][:8])
    assert np.allclose(got[0], ref[0], rtol=1e-9, atol=1e-12), (what, worst)
    assert len(ref[0]) <= 96


def _expect_plan(ctx, kind, stride, what):
    pl = ctx.plan()
    lds = 'true' if kind == 'lds' else 'false'
    want = {1: ('clr_scan_prepared_kernel<16,%s>' % lds, 16, PREPARED), 5: ('clr_scan_prepared_kernel<8,%s>' % lds, 8, PREPARED),
            16: ('clr_scan_solo_kernel<%s>' % lds, None, SOLO)}[stride]
    assert pl['kernel'] == want[0] and pl['mode'] == want[2] and (want[1] is None or pl['J'] == want[1]), (what, pl)
    assert pl['use_lds'] == (kind == 'lds') and pl['stream_bytes'] > 0, (what, pl)


# (data set, A list, stride, centre): every stride meets every centre it can -- a strided run inside the tie run would sit on one
# position (widewin.run_around), so 30250 is met at stride 1 only -- and so does every A list
_FIVE = ww.A_LISTS[2]
_PLAN_CASES = [
    ('lds', '100', 1, 6000), ('lds', '100', 5, 30000), ('lds', '100', 16, 6000),
    ('lds', '250', 1, 30000), ('lds', '250', 5, 6000), ('lds', '250', 16, 30000),
    ('lds', _FIVE, 1, 30250), ('lds', _FIVE, 5, 30000), ('lds', _FIVE, 16, 6000),
    ('l2', '100', 1, 30000), ('l2', '100', 5, 6000), ('l2', '100', 16, 30000),
    ('l2', '250', 1, 30250), ('l2', '250', 5, 30000), ('l2', '250', 16, 6000),
    ('l2', _FIVE, 1, 6000), ('l2', _FIVE, 5, 6000), ('l2', _FIVE, 16, 30000),
]


@pytest.mark.parametrize('kind,alist,stride,centre', _PLAN_CASES)
def test_default_plans(kind, alist, stride, centre, open_ctx):
    """83 test sites (five groups of 16 and a partial one) at stride 1 -> clr_scan_prepared_kernel<16,.>, stride 5 -> <8,.>,
    stride 16 -> clr_scan_solo_kernel, on both data sets and all three A lists."""
    what = '%s A=%s stride %d around %d' % (kind, alist, stride, centre)
    ctx = open_ctx(kind, alist)
    R = _device_table(kind, ctx)
    idx = ww.run_around(centre, stride)
    assert len(idx) == 83
    lo, hi = _whole(idx)
    ctx.set_tests(_data(kind)['gen'][idx], lo, hi)
    _expect_plan(ctx, kind, stride, what)
    ctx.scan()
    got = ctx.fetch()
    ref = _oracle(kind, alist, idx, lo, hi, R)
    assert np.all(ref[3] >= 0) and ref[0].min() > 1000          # the wide A wins: nothing here is a comparison of empty results
    _check(got, ref, what)


VARIANTS = {13: ('clr_scan_prepared_kernel<16,true>', PREPARED), 14: ('clr_scan_prepared_kernel<8,true>', PREPARED),
            15: ('clr_scan_prepared_kernel<4,true>', PREPARED), 16: ('clr_scan_solo_kernel<true>', SOLO),
            12: ('clr_scan_grouped_kernel<16,true,3>', 3), 2: ('clr_scan_kernel<true>', -1), 10: (None, None)}


@pytest.mark.parametrize('alist', (ww.A_LISTS[0], ww.A_LISTS[2]))
@pytest.mark.parametrize('variant', sorted(VARIANTS))
def test_variants(variant, alist, open_ctx):
    """Prepared J = 16 / 8 / 4 (13, 14, 15), solo on request (16), the round-2 grouped (12) and per-site (2) kernels and the exact
    products (10) on the uneven windows around 6000 and the two full zones around 30000 (which straddle the tie run's start)."""
    ctx = open_ctx('lds', alist)
    R = _device_table('lds', ctx)
    ctx.set_variant(variant)
    for run in ('c6000', 'c30000'):
        idx = ww.TEST_RUNS[run]
        lo, hi = _whole(idx)
        ctx.set_tests(_data('lds')['gen'][idx], lo, hi)
        name, mode = VARIANTS[variant]
        pl = ctx.plan()
        assert name is None or (pl['kernel'], pl['mode']) == (name, mode), (variant, pl)
        ctx.scan()
        _check(ctx.fetch(), _oracle('lds', alist, idx, lo, hi, R), 'variant %d A=%s %s' % (variant, alist, run))


@pytest.mark.parametrize('alist', (ww.A_LISTS[0], ww.A_LISTS[2]))
def test_far_field_against_exact_products(alist, open_ctx):
    """Variant 0 against variant 10 (every factor 1 + alpha R multiplied): identical integer fields, CLR to 1e-11 relative, the
    bar of test_far_field_moments_against_exact_products, with ~20 000 far sites per zone instead of ~2 000."""
    ctx = open_ctx('lds', alist)
    for run in ('c6000', 'c30000', 'c30250'):
        idx = ww.TEST_RUNS[run]
        lo, hi = _whole(idx)
        out = {}
        for v in (10, 0):
            ctx.set_variant(v)
            out[v] = _scan(ctx, 'lds', idx, lo, hi)
        for q in (1, 2, 3, 4):
            assert np.array_equal(out[0][q], out[10][q]), (run, q)
        worst = float(np.max(np.abs(out[0][0] - out[10][0]) / np.abs(out[10][0])))
        print('far field vs exact products, A=%s %s: worst relative dCLR %.3e' % (alist, run, worst))
        assert np.allclose(out[0][0], out[10][0], rtol=1e-11, atol=1e-13), (run, worst)


@pytest.mark.parametrize('r', (40, 3000, 9000, 15000))
def test_index_windows(r, open_ctx):
    """Index windows lo = i - r, hi = i + r + 1 through the default plan at A = 100: r = 40 ends in the near field, 3000 inside the
    far field below the prepared cap, 9000 and 15000 past it (ragged ends in the overflow region)."""
    ctx = open_ctx('lds', '100')
    R = _device_table('lds', ctx)
    for run in ('c6000', 'c30000'):
        idx = ww.TEST_RUNS[run]
        lo = np.maximum(idx - r, 0).astype(np.int64)
        hi = np.minimum(idx + r + 1, N - 1).astype(np.int64)
        ctx.set_tests(_data('lds')['gen'][idx], lo, hi)
        _expect_plan(ctx, 'lds', 1, (r, run))
        ctx.scan()
        _check(ctx.fetch(), _oracle('lds', '100', idx, lo, hi, R), 'r = %d %s' % (r, run))


@pytest.mark.parametrize('run', ('first', 'last', 'edge', 'straddle', 'c30250'))
def test_chromosome_ends_density_edge_and_tie_run(run, open_ctx):
    """The first and last 64 sites (one zone empty, the other past every cap), a run that starts where the hot spot ends, a group
    across that edge, and groups wholly inside the tie run, through the default plan at A = 100."""
    ctx = open_ctx('lds', '100')
    R = _device_table('lds', ctx)
    idx = ww.TEST_RUNS[run]
    lo, hi = _whole(idx)
    ctx.set_tests(_data('lds')['gen'][idx], lo, hi)
    _expect_plan(ctx, 'lds', 1, run)
    ctx.scan()
    got = ctx.fetch()
    ref = _oracle('lds', '100', idx, lo, hi, R)
    assert np.all(ref[3] == 0) and ref[0].min() > 1000
    _check(got, ref, run)


@pytest.mark.parametrize('run', ('c6000', 'c30000'))
def test_descending_test_sites(run, open_ctx):
    """The same test sites in descending order.  Unsorted test positions go to one test site per wave (clr_scan_solo_kernel), so the
    results must be, bit for bit, the reverse of the ascending results of that kernel (variant 16) -- and meet the oracle like any
    other scan."""
    ctx = open_ctx('lds', '100')
    R = _device_table('lds', ctx)
    idx = ww.TEST_RUNS[run]
    lo, hi = _whole(idx)
    ctx.set_tests(_data('lds')['gen'][idx[::-1]], lo, hi)
    pl = ctx.plan()
    assert (pl['kernel'], pl['mode']) == ('clr_scan_solo_kernel<true>', SOLO), pl
    ctx.scan()
    rev = [a.copy() for a in ctx.fetch()]
    ctx.set_variant(16)
    asc = _scan(ctx, 'lds', idx, lo, hi)
    _check([a[::-1] for a in rev], _oracle('lds', '100', idx, lo, hi, R), 'descending ' + run)
    assert np.array_equal(_bits(rev[0][::-1]), _bits(asc[0]))
    for q in (1, 2, 3, 4):
        assert np.array_equal(rev[q][::-1], asc[q]), q


@pytest.mark.parametrize('stride', (1, 16))
@pytest.mark.parametrize('alist', ww.A_LISTS[:2])
def test_own_table_end_to_end(alist, stride, open_ctx):
    """K1 -> K2 -> finalize against the oracle fed the table the ORACLE builds (oracle_R: scipy's betabinom), never the device's.
    Integer fields exact; CLR to test_gpu_round4.py's own-table bound, max(1e-9, 1e-6 |CLR|)."""
    ctx = open_ctx('lds', alist)
    R = _own_table()
    Rd = ctx.fetch_lut()[1]
    ok = np.isfinite(R)
    assert np.array_equal(ok, np.isfinite(Rd)) and np.max(np.abs(Rd[ok] - R[ok]) / np.maximum(np.abs(R[ok]), 1e-300)) < 1e-9
    for centre in ww.CENTRES[:2]:
        idx = ww.run_around(centre, stride)
        lo, hi = _whole(idx)
        ctx.set_tests(_data('lds')['gen'][idx], lo, hi)
        _expect_plan(ctx, 'lds', stride, (alist, stride, centre))
        ctx.scan()
        got = ctx.fetch()
        ref = _oracle('lds', alist, idx, lo, hi, R, table='own')
        for q in (1, 2, 3, 4):
            assert np.array_equal(got[q], ref[q]), (alist, stride, centre, q)
        err = np.abs(got[0] - ref[0])
        print('own table, A=%s stride %d around %d: worst relative dCLR %.3e' % (alist, stride, centre, float(np.max(err / np.abs(ref[0])))))
        assert np.all(err <= np.maximum(1e-9, 1e-6 * np.abs(ref[0])))


@pytest.mark.parametrize('stride', (1, 16))
def test_profiles_on_wide_windows(stride, open_ctx):
    """README's two promises for --profiles on the <J, LDS, true> instantiations at these sizes: max_v profile_A[t][v] is the CLR
    column bit for bit, and profile_A[t][A = 100] is, bit for bit, the CLR of the same test sites scanned with the list '100'; and
    every column against the C oracle's scan with that A alone."""
    five, one = ww.A_LISTS[2], ww.A_LISTS[0]
    As = _As(five)
    ctx = open_ctx('lds', five)
    R = _device_table('lds', ctx)
    ctx.set_profiles('A')
    ctx1 = open_ctx('lds', one)
    for centre in ww.CENTRES[:2]:
        idx = ww.run_around(centre, stride)
        lo, hi = _whole(idx)
        ctx.set_tests(_data('lds')['gen'][idx], lo, hi)
        _expect_plan(ctx, 'lds', stride, (stride, centre))
        ctx.scan()
        clr, _, _, iA, ns = ctx.fetch()
        prof = ctx.fetch_profile('A')
        assert prof.shape == (len(idx), 5) and np.all(iA >= 0) and ns.max() > 20000
        assert np.array_equal(_bits(prof.max(axis=1)), _bits(clr))
        assert np.all(prof >= 0.0)
        for one_A in five.split(','):                                 # every column against the oracle's scan with that A alone
            o = _oracle('lds', one_A, idx, lo, hi, R)[0]              # (A = 1e6 reaches 1.8e-5: a handful of sites, or the tie run)
            assert np.allclose(prof[:, As.index(float(one_A))], o, rtol=1e-9, atol=1e-12), (stride, centre, one_A)
        alone = _scan(ctx1, 'lds', idx, lo, hi)
        assert np.array_equal(_bits(prof[:, As.index(100.0)]), _bits(alone[0])), (stride, centre)
        wide = iA == As.index(100.0)                                  # where A = 100 wins, the two scans tell the same story
        assert wide.any() and np.array_equal(_bits(clr[wide]), _bits(alone[0][wide])) and np.array_equal(ns[wide], alone[4][wide])


def test_surfaces_on_wide_windows(open_ctx):
    """bmx_ctx_surface and bmx_ctx_surfaces on six of the widest windows against the oracle surface T[A, x, alpha_beta] (device
    table): 1e-9 relative, nSites per A exact, NaN exactly where the oracle's window is empty; the block maximum against the scan's CLR to 1e-12
    relative (test_gpu_surfaces.py's bound)."""
    five = ww.A_LISTS[2]
    As = _As(five)
    d = _data('lds')
    ctx = open_ctx('lds', five)
    R = _device_table('lds', ctx)
    idx = np.array([29980, 29990, 30000, 30250, 30499, 30510])
    lo, hi = _whole(idx)
    got = _scan(ctx, 'lds', idx, lo, hi)
    Ts, nss = ctx.surfaces(np.arange(len(idx)))
    m = orc.Model('B2', d['gen'], d['k'], d['nn'], d['spect'], d['props'], 1, d['xs'], d['ab'], As)
    assert np.array_equal(m.row, d['rows'])
    m.R = R                                               # the device's own table: K2 alone, as everywhere at the 1e-9 bar
    nx, nab = len(d['xs']), len(d['ab'])
    for j, i in enumerate(idx):
        best, ref, ns = orc.clr_lut(m, 0, N - 1, d['gen'][i], surface=True)
        assert ns.max() > 46000 and ns[As.index(1000000.0)] < 1000       # A = 1e6 reaches 1.8e-5: a handful of sites, or the tie run
        T1, ns1 = ctx.surface(d['gen'][i], 0, N - 1)
        for T, n, what in ((Ts[j], nss[j], 'surfaces'), (T1, ns1, 'surface')):
            assert np.array_equal(n, ns), (what, i)
            assert np.array_equal(np.isnan(T), np.isnan(ref)), (what, i)
            has = ~np.isnan(ref)
            err = np.abs(T - ref)
            ok = err <= 1e-9 * np.abs(ref) + 1e-12
            print('%s of site %d: worst excess over 1e-9 |T| + 1e-12: %.3e; smallest |T| %.3e' % (what, i, float(np.nanmax(err - 1e-9 * np.abs(ref) - 1e-12)), float(np.nanmin(np.abs(ref)))))
            assert np.all(ok[has]), (what, i, np.argwhere(has & ~ok)[:4], err[has & ~ok][:4], ref[has & ~ok][:4])
            flat = np.where(np.isnan(T), -np.inf, T).reshape(-1)
            top = int(np.argmax(flat))
            assert flat[top] > 0 and abs(got[0][j] - flat[top]) <= 1e-12 * flat[top], (what, i)
            assert (int(got[3][j]), int(got[1][j]), int(got[2][j])) == (top // (nx * nab), (top // nab) % nx, top % nab), (what, i)
        assert best[1:] == (int(got[1][j]), int(got[2][j]), int(got[3][j]), int(got[4][j]))


@pytest.mark.parametrize('stride', (1, 5, 16))
def test_two_scans_are_bitwise_equal(stride, open_ctx):
    """Two scans of the same wide test sites: the stream is rebuilt per scan, and prep_kernel's moment sums over 20 000 sites per
    zone must not depend on the order anything happens to finish in."""
    ctx = open_ctx('lds', ww.A_LISTS[2])
    for centre in ww.CENTRES[:2]:
        idx = ww.run_around(centre, stride)
        lo, hi = _whole(idx)
        first = _scan(ctx, 'lds', idx, lo, hi)
        ctx.scan()
        again = ctx.fetch()
        assert np.array_equal(_bits(first[0]), _bits(again[0])), (stride, centre, float(np.max(np.abs(first[0] - again[0]))))
        for q in (1, 2, 3, 4):
            assert np.array_equal(first[q], again[q])
        fresh = open_ctx('lds', ww.A_LISTS[2])                 # and a context that has never scanned anything else
        other = _scan(fresh, 'lds', idx, lo, hi)
        fresh.close()
        assert np.array_equal(_bits(first[0]), _bits(other[0])), (stride, centre)
