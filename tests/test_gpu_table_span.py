"""The scan kernels across the selection table's exponent range (tests/tablespan.py: one row's neutral probability sets
span_hi = ceil(log2(1 + max R)) anywhere from 12 to the library's limit of 240; that row rare, common or in a run of 64 sites).
tests/test_tablespan_cpu.py proves on the CPU that the inputs have the span they ask for, that eight factors of the most frequent
row overflow a double from span 129 on, and that no compared window is a near-tie; here every plan and variant is compared with
the C oracle on them.

Bar, everywhere: every result finite; (x, alpha_beta, A, nSites) exactly equal on every window that is not in tablespan.TIED, with the
count of differing windows asserted to be 0 (no "tie within rounding" allowance); np.allclose(clr, oracle, rtol=1e-9, atol=1e-12) on
EVERY window, the listed ones included (their runner-up trails by 8e-4 of a T of 1e4 .. 7e4: far more than rounding, less than the
1e-7 T the exact comparison asks for), with the oracle fed the device's own table (K2 alone, as the other randomised tests)."""
import functools

import numpy as np
import pytest

import tablespan as tb
from util import c_oracle, c_scan, c_sel_table, orc

pytestmark = pytest.mark.gpu

N = tb.N
PREPARED, SOLO, PER_SITE = 4, 5, -1


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _grid(alist=tb.A_LIST):
    from ballermixplus_amd.hostmodel import Grids
    return Grids(None, None, True, False, None, alist).scan_order()


@functools.lru_cache(maxsize=None)
def _sel_max(kind):
    """The largest P_sel of the extreme row over the grid, from the oracle's table (the Python oracle at n = 30, the C oracle at
    n = 150: tests/test_tablespan_cpu.py)."""
    xs, ab, _ = _grid()
    k, n = tb.ext_row(kind)
    if kind == 'large':
        return float(c_sel_table(c_oracle(), 'B2', n, 1, xs, ab)[:, :, k].max())
    return float(orc.sel_table('B2', n, 1, list(xs), list(ab))[:, :, k].max())


@functools.lru_cache(maxsize=None)
def _sites(kind):
    return tb.chromosome(kind)


@functools.lru_cache(maxsize=8)
def _model(kind, span):
    from ballermixplus_amd import engine as eng
    gen, k, nn = _sites(kind)
    spect, props = tb.spectrum(kind, span, _sel_max('large' if kind == 'large' else 'rare'), k, nn)
    xs, ab, _ = _grid()
    model = eng.ModelArrays('B2', 1, tb.sizes_of(kind), spect, props, xs, ab)
    return model, model.rows_of(k, nn)


_TABLE = {}


@pytest.fixture
def open_ctx():
    """open_ctx(data set, span, A list) -> (context with that model and the data set's sites, the device's own table with 0 on the
    rows no site can carry); every context a test opened is closed when the test ends, however it ends."""
    from ballermixplus_amd import engine as eng
    made = []

    def make(kind, span, alist=tb.A_LIST):
        model, rows = _model(kind, span)
        ctx = eng.Context(0)
        made.append(ctx)
        ctx.set_model(model, _grid(alist)[2])
        ctx.set_sites(_sites(kind)[0], rows)
        if (kind, span) not in _TABLE:
            R = ctx.fetch_lut()[1]
            assert np.isfinite(R[:, :, np.unique(rows)]).all()
            R = np.where(np.isfinite(R), R, 0.0)
            bits = float(np.log2(1.0 + R.max()))
            assert int(np.ceil(bits)) == span and abs(bits - (span - tb.MARGIN)) < 1e-6, (kind, span, bits)   # span_hi of set_model
            _TABLE[(kind, span)] = R
        return ctx, _TABLE[(kind, span)]

    yield make
    for ctx in made:
        ctx.close()


_ORACLE = {}


def _oracle(kind, span, alist, idx, R):
    """One oracle run per (data set, span, A list, test sites), shared by plans and variants."""
    key = (kind, span, alist, idx.tobytes())
    if key not in _ORACLE:
        gen = _sites(kind)[0]
        out = c_scan(c_oracle(), R, _grid(alist)[2], gen, _model(kind, span)[1], gen[idx], *tb.windows_of(kind, idx))
        for a in out:
            a.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def _scan(ctx, kind, idx):
    ctx.set_tests(_sites(kind)[0][idx], *tb.windows_of(kind, idx))
    ctx.scan()
    return [a.copy() for a in ctx.fetch()]


def _check(got, ref, what, tied=()):
    keep = np.ones(len(ref[0]), bool)
    keep[list(tied)] = False
    bad = int(np.sum(~np.isfinite(got[0])))
    worst = float(np.max(np.abs(got[0] - ref[0]) / np.maximum(np.abs(ref[0]), 1e-300)))
    ties = int(np.sum(np.any([got[q][keep] != ref[q][keep] for q in (1, 2, 3, 4)], axis=0)))
    print('%s: %d windows (%d skipped), nSites %d .. %d, CLR %.1f .. %.1f, not finite %d, ties %d, worst relative dCLR %.3e'
          % (what, len(ref[0]), len(tied), ref[4].min(), ref[4].max(), ref[0].min(), ref[0].max(), bad, ties, worst))
    assert bad == 0, (what, bad, got[0][~np.isfinite(got[0])][:4])
    assert np.all(ref[3] >= 0) and len(ref[0]) <= 160 and len(tied) <= 0.02 * len(keep)      # no comparison of empty results
    assert ref[0].max() < tb.CLR_LIMIT
    for q, name in ((1, 'x'), (2, 'alpha_beta'), (3, 'A'), (4, 'nSites')):
        assert np.array_equal(got[q][keep], ref[q][keep]), (what, name, np.where(got[q] != ref[q])[0][:8])
    assert ties == 0
    assert np.allclose(got[0], ref[0], rtol=1e-9, atol=1e-12), (what, worst)


def _expect_default_plan(ctx, span, stride, lds, what):
    pl = ctx.plan()
    if span <= tb.GROUP_SPAN_MAX and stride <= 5:
        want = ('clr_scan_prepared_kernel<%d,%s>' % (16 if stride == 1 else 8, lds), PREPARED)
    else:
        want = ('clr_scan_solo_kernel<%s>' % lds, SOLO)
    assert (pl['kernel'], pl['mode']) == want, (what, pl)


_DEFAULT = [(kind, span, stride) for kind in tb.PLACEMENTS for span in tb.SPANS for stride in tb.STRIDES[span <= tb.GROUP_SPAN_MAX]]


@pytest.mark.parametrize('kind,span,stride', _DEFAULT)
def test_default_plans(kind, span, stride, open_ctx):
    """Spans 12, 40, 62 at strides 1 and 5 -> clr_scan_prepared_kernel<16,.> and <8,.> (62: the last grouped span); 63 (the first
    span the planner sends to the solo kernel whatever the stride) to 240 at strides 1 and 20 -> clr_scan_solo_kernel: its limit
    is 8 at span 125, 7 at 126, and from 129 on eight factors of the most frequent row leave the double range."""
    what = '%s span %d stride %d' % (kind, span, stride)
    ctx, R = open_ctx(kind, span)
    idx = tb.tests_of(stride)
    ctx.set_tests(_sites(kind)[0][idx], *tb.windows_of(kind, idx))
    _expect_default_plan(ctx, span, stride, 'true', what)
    ctx.scan()
    _check(ctx.fetch(), _oracle(kind, span, tb.A_LIST, idx, R), what, tb.TIED.get((kind, span, stride), ()))


GROUPED_VARIANTS = {13: ('clr_scan_prepared_kernel<16,true>', PREPARED), 14: ('clr_scan_prepared_kernel<8,true>', PREPARED),
                    15: ('clr_scan_prepared_kernel<4,true>', PREPARED), 12: ('clr_scan_grouped_kernel<16,true,3>', 3),
                    3: ('clr_scan_grouped_kernel<8,true,3>', 3), 4: ('clr_scan_grouped_kernel<4,true,3>', 3),
                    10: ('clr_scan_grouped_kernel<16,true,2>', 2), 8: ('clr_scan_grouped_kernel<16,true,1>', 1),
                    5: ('clr_scan_grouped_kernel<16,true,0>', 0), 16: ('clr_scan_solo_kernel<true>', SOLO)}


@pytest.mark.parametrize('span', (40, 62))
@pytest.mark.parametrize('variant', sorted(GROUPED_VARIANTS))
def test_grouped_variants_on_the_run(variant, span, open_ctx):
    """Prepared J = 16 / 8 / 4 (13, 14, 15), the round-2 forms (12, 3, 4: power sums at J = 16 / 8 / 4; 10: exact products; 8: pairs;
    5: one site per step) and solo on request (16) where a 64-site pass has every factor at 2^39.5 / 2^61.5: one pass of J = 4
    spends 640 / 992 of the 1000-bit budget."""
    ctx, R = open_ctx('run', span)
    ctx.set_variant(variant)
    idx = tb.tests_of(1)
    ctx.set_tests(_sites('run')[0][idx], *tb.windows_of('run', idx))
    pl = ctx.plan()
    assert (pl['kernel'], pl['mode']) == GROUPED_VARIANTS[variant], (variant, pl)
    ctx.scan()
    _check(ctx.fetch(), _oracle('run', span, tb.A_LIST, idx, R), 'variant %d run span %d' % (variant, span), tb.TIED.get(('run', span, 1), ()))


@pytest.mark.parametrize('variant', (0, 13, 12, 16))
def test_single_A(variant, open_ctx):
    """The A list '5000' alone (windows of a few hundred to 1 200 sites) on the run at span 62."""
    ctx, R = open_ctx('run', 62, tb.ONE_A)
    ctx.set_variant(variant)
    idx = tb.tests_of(1)
    got = _scan(ctx, 'run', idx)
    _check(got, _oracle('run', 62, tb.ONE_A, idx, R), 'variant %d run span 62 A=%s' % (variant, tb.ONE_A), tb.TIED.get(('run', 62, 1, tb.ONE_A), ()))


SOLO_RANGE_VARIANTS = {2: ('clr_scan_kernel<true>', PER_SITE), 16: ('clr_scan_solo_kernel<true>', SOLO),
                       0: ('clr_scan_solo_kernel<true>', SOLO), 13: ('clr_scan_kernel<true>', PER_SITE)}


@pytest.mark.parametrize('kind', ('common', 'run'))
@pytest.mark.parametrize('span', (63, 128, 129, 240))
@pytest.mark.parametrize('variant', sorted(SOLO_RANGE_VARIANTS))
def test_variants_past_the_grouped_range(variant, span, kind, open_ctx):
    """The per-site kernel (2: four factors per step), solo on request (16) and by default (0); a request for a grouped form (13)
    outside its domain falls back to the per-site kernel and still gives the oracle's results."""
    ctx, R = open_ctx(kind, span)
    ctx.set_variant(variant)
    idx = tb.tests_of(1)
    ctx.set_tests(_sites(kind)[0][idx], *tb.windows_of(kind, idx))
    pl = ctx.plan()
    assert (pl['kernel'], pl['mode']) == SOLO_RANGE_VARIANTS[variant] and pl['mode'] != PREPARED, (variant, pl)
    ctx.scan()
    _check(ctx.fetch(), _oracle(kind, span, tb.A_LIST, idx, R), 'variant %d %s span %d' % (variant, kind, span), tb.TIED.get((kind, span, 1), ()))


@pytest.mark.parametrize('stride,variant', ((1, 0), (5, 0), (20, 0), (1, 2), (1, 12)))
def test_low_side(stride, variant, open_ctx):
    """A row carried by an eighth of the sites with R down to -1 + 5.9e-7 and site pairs 1e-9 apart next to test sites: factors of
    2^-20 at alpha > 1/2, the span_generic = 54 branch of the grouped kernels' budget."""
    ctx, R = open_ctx('low', tb.LOW_SPAN)
    ctx.set_variant(variant)
    idx = tb.tests_of(stride)
    ctx.set_tests(_sites('low')[0][idx], *tb.windows_of('low', idx))
    if variant == 0:
        _expect_default_plan(ctx, tb.LOW_SPAN, stride, 'true', ('low', stride))
    ctx.scan()
    _check(ctx.fetch(), _oracle('low', tb.LOW_SPAN, tb.A_LIST, idx, R), 'low stride %d variant %d' % (stride, variant),
           tb.TIED.get(('low', tb.LOW_SPAN, stride), ()))


@pytest.mark.parametrize('span,stride', ((50, 1), (50, 5), (200, 1), (200, 20)))
def test_table_in_l2(span, stride, open_ctx):
    """Sample sizes 150, 160, 170: the R slice does not fit in LDS, so the <J, false> prepared forms (span 50) and the solo
    <false> form (span 200) run."""
    ctx, R = open_ctx('large', span)
    assert R.shape[2] == 483
    idx = tb.tests_of(stride)
    ctx.set_tests(_sites('large')[0][idx], *tb.windows_of('large', idx))
    _expect_default_plan(ctx, span, stride, 'false', ('large', span, stride))
    assert not ctx.plan()['use_lds']
    ctx.scan()
    _check(ctx.fetch(), _oracle('large', span, tb.A_LIST, idx, R), 'large span %d stride %d' % (span, stride), tb.TIED.get(('large', span, stride), ()))


@pytest.mark.parametrize('span,stride', ((62, 1), (200, 20)))
def test_profiles(span, stride, open_ctx):
    """All three profiles on the run: the five scan fields stay bitwise equal to the scan without profiles, every profile's
    maximum is the CLR bit for bit, and column v of each profile is the C oracle's scan with that single A, x or alpha_beta."""
    kind = 'run'
    ctx, R = open_ctx(kind, span)
    gen, rows = _sites(kind)[0], _model(kind, span)[1]
    idx = tb.tests_of(stride)
    off = _scan(ctx, kind, idx)
    ctx.set_profiles(['A', 'x', 'abeta'])
    on = _scan(ctx, kind, idx)
    _expect_default_plan(ctx, span, stride, 'true', ('profiles', span, stride))
    for a, b in zip(off, on):
        assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
    _check(on, _oracle(kind, span, tb.A_LIST, idx, R), 'profiles on, run span %d stride %d' % (span, stride), tb.TIED.get((kind, span, stride), ()))
    prof = {k: ctx.fetch_profile(k) for k in ('A', 'x', 'abeta')}
    As = np.asarray(_grid()[2], dtype=np.float64)
    L = c_oracle()
    tg, (lo, hi) = gen[idx], tb.windows_of(kind, idx)
    for name, n in (('A', len(As)), ('x', R.shape[0]), ('abeta', R.shape[1])):
        p = prof[name]
        assert p.shape == (len(idx), n) and np.isfinite(p).all() and np.all(p >= 0.0), name
        assert np.array_equal(_bits(p.max(axis=1)), _bits(on[0])), name
        for v in range(n):
            if name == 'A':
                o = c_scan(L, R, As[v:v + 1], gen, rows, tg, lo, hi)[0]
            elif name == 'x':
                o = c_scan(L, R[v:v + 1], As, gen, rows, tg, lo, hi)[0]
            else:
                o = c_scan(L, R[:, v:v + 1], As, gen, rows, tg, lo, hi)[0]
            assert np.allclose(p[:, v], o, rtol=1e-9, atol=1e-12), (name, v, float(np.max(np.abs(p[:, v] - o))))


@pytest.mark.parametrize('span', (62, 240))
def test_independent_path(span, open_ctx):
    """bmx_ctx_surface (a plain sum of log1p per grid point: no running product, no exponent extraction) on six windows, and
    bmx_ctx_eval_points at the scan's winning grid point: both agree with the scan's winner to 1e-9."""
    kind = 'common'
    ctx, R = open_ctx(kind, span)
    gen = _sites(kind)[0]
    xs, ab, As = _grid()
    idx = np.array([0, 1500, 1530, 1563, 1571, N - 1])
    got = _scan(ctx, kind, idx)
    _check(got, _oracle(kind, span, tb.A_LIST, idx, R), 'six windows, common span %d' % span)
    nx, nab = len(xs), len(ab)
    lo, hi = tb.windows_of(kind, idx)
    for j, i in enumerate(idx):
        T, ns = ctx.surface(gen[i], lo[j], hi[j])
        flat = np.asarray(T).reshape(-1)
        assert np.isfinite(flat).all()
        top = int(np.argmax(flat))
        assert abs(got[0][j] - flat[top]) <= 1e-9 * flat[top], (i, got[0][j], flat[top])
        assert (int(got[3][j]), int(got[1][j]), int(got[2][j])) == (top // (nx * nab), (top // nab) % nx, top % nab), i
        assert ns[got[3][j]] == got[4][j]
    Tp, nsp = ctx.eval_points(np.asarray(As)[got[3]], np.asarray(xs)[got[1]], np.asarray(ab)[got[2]])
    print('eval_points at the winners, span %d: worst relative difference %.3e' % (span, float(np.max(np.abs(Tp - got[0]) / got[0]))))
    assert np.array_equal(nsp, got[4]) and np.allclose(Tp, got[0], rtol=1e-9, atol=0)


def test_limit_and_recovery(open_ctx):
    """A table placed at 2^241.5 is refused by set_model with the limit error, and the context takes a span-240 model next and
    scans it like any other."""
    from ballermixplus_amd import _lib, engine as eng
    held = eng.live_bytes()
    kind = 'rare'
    gen, k, nn = _sites(kind)
    spect, props = tb.spectrum(kind, tb.SPAN_LIMIT + 2, _sel_max(kind), k, nn)         # log2(1 + max R) = 241.5
    xs, ab, As = _grid()
    over = eng.ModelArrays('B2', 1, [tb.NSAMP], spect, props, xs, ab)
    ctx = eng.Context(0)
    try:
        with pytest.raises(_lib.BmxError, match=r'spans more than 2\^240') as e:
            ctx.set_model(over, As)
        assert e.value.code == -4                                                  # BMX_E_LIMIT
        model, rows = _model(kind, tb.SPAN_LIMIT)
        ctx.set_model(model, As)
        ctx.set_sites(gen, rows)
        R = ctx.fetch_lut()[1]
        R = np.where(np.isfinite(R), R, 0.0)
        assert int(np.ceil(np.log2(1.0 + R.max()))) == tb.SPAN_LIMIT
        idx = tb.tests_of(20)
        _check(_scan(ctx, kind, idx), _oracle(kind, tb.SPAN_LIMIT, tb.A_LIST, idx, R), 'span 240 after a refused model')
    finally:
        ctx.close()
    assert eng.live_bytes() == held          # what the refused set_model had allocated went with the context


@pytest.mark.parametrize('stride', (1, 20))
def test_two_scans_are_bitwise_equal(stride, open_ctx):
    """Two scans of the span-240 'common' case, and a context that has never scanned anything else."""
    ctx, _ = open_ctx('common', 240)
    idx = tb.tests_of(stride)
    first = _scan(ctx, 'common', idx)
    ctx.scan()
    again = ctx.fetch()
    fresh, _ = open_ctx('common', 240)
    other = _scan(fresh, 'common', idx)
    for b in (again, other):
        assert np.array_equal(_bits(first[0]), _bits(b[0]))
        for q in (1, 2, 3, 4):
            assert np.array_equal(first[q], b[q])
    assert np.isfinite(first[0]).all()
