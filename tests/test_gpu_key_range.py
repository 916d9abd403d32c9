"""The scan's best key at the ends of its exponent and A-index fields (tests/keyrange.py; tests/test_keyrange_cpu.py proves on the
CPU that the cases reach those ends), on every kernel form the planner can pick, against the C oracle -- and the refusal of a scan
whose winner sits at the exponent clamp.

Bar: (x, alpha_beta, A, nSites) exactly equal on every compared window that is not in keyrange.TIED; np.allclose(clr, oracle,
rtol=1e-9, atol=1e-12) on every compared window, the listed ones included; the oracle is fed the device's own table (K2 alone, as
the other randomised tests).  A window is compared where the oracle's E* <= 131 060 and must be refused (BMX_E_LIMIT) where
E* >= 131 080; every scan of a band holds windows of one side only."""
import ctypes as C
import functools

import numpy as np
import pytest

import keyrange as kr
import tablespan as tb
from util import c_oracle, c_scan, c_sel_table, orc

pytestmark = pytest.mark.gpu

PREPARED, SOLO, PER_SITE = 4, 5, -1
LIMIT = -4                                  # BMX_E_LIMIT
COMPARED = ('rung1', 'rung2', 'rung3', 'inside')
REFUSED = r'CLR past the scan.s range \(\|T\| <= 2 ln 2 x 131070'
WORST = {}                                  # form -> worst relative dCLR seen (printed when the module is done)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _grid(alist=kr.A_HIGH):
    from ballermixplus_amd.hostmodel import Grids
    return Grids(None, None, True, False, None, alist).scan_order()


@functools.lru_cache(maxsize=None)
def _sel_max(k, n):
    """The largest P_sel of row (k, n) over the grid, from the oracle's table."""
    xs, ab, _ = _grid()
    if n > kr.NSAMP:
        return float(c_sel_table(c_oracle(), 'B2', n, 1, xs, ab)[:, :, k].max())
    return float(orc.sel_table('B2', n, 1, list(xs), list(ab))[:, :, k].max())


@functools.lru_cache(maxsize=None)
def _case(name):
    """(model, genPos, counts, rows) of a 'high' set, of 'low' or of 'wide'."""
    from ballermixplus_amd import engine as eng
    xs, ab, _ = _grid()
    if name in ('low', 'lowL'):
        gen, k, nn = kr.low_chromosome(name)
        spect, props = kr.low_spectrum(_sel_max(*kr.low_row(name)), k, nn, name)
        model = eng.ModelArrays('B2', 1, list(kr.low_sizes(name)), spect, props, xs, ab)
    elif name == 'wide':
        gen, k, nn = kr.wide_chromosome()
        cnt = {}
        for a in k.tolist():
            cnt[(a, 50)] = cnt.get((a, 50), 0) + 1
        model = eng.ModelArrays('B2', int(k.min()), [50], {key: v / len(k) for key, v in cnt.items()}, {50: 1.0}, [0.3], [10.0])
    else:
        gen, k, nn = kr.chromosome(name)
        spect, props = kr.spectrum(name, _sel_max(*kr.ext_row(name)), k, nn)
        model = eng.ModelArrays('B2', 1, kr.sizes_of(name), spect, props, xs, ab)
    return model, gen, k, model.rows_of(k, nn)


_TABLE = {}


@pytest.fixture
def open_ctx():
    """open_ctx(case, A values) -> (context with the case's model and sites, the device's own table with 0 on the rows no site
    carries); every context a test opened is closed when the test ends."""
    from ballermixplus_amd import engine as eng
    made = []

    def make(name, As=None):
        model, gen, k, rows = _case(name)
        ctx = eng.Context(0)
        made.append(ctx)
        ctx.set_model(model, _grid()[2] if As is None else As)
        ctx.set_sites(gen, rows)
        if name not in _TABLE:
            R = ctx.fetch_lut()[1]
            assert np.isfinite(R[:, :, np.unique(rows)]).all()
            _TABLE[name] = np.where(np.isfinite(R), R, 0.0)
            if name in kr.SETS:
                assert abs(float(np.log2(1.0 + _TABLE[name].max())) - (kr.SETS[name] - tb.MARGIN)) < 1e-6
        return ctx, _TABLE[name]

    yield make
    for ctx in made:
        ctx.close()


_ORACLE = {}


def _high_tests(name, band, stride):
    gen, k = _case(name)[1:3]
    idx = kr.tests_of(stride)
    return (gen[idx],) + tuple(kr.high_windows(name, band, idx, k))


def _oracle(name, R, As, tg, lo, hi):
    """One oracle run per (case, A list, test sites), shared by plans and variants, read-only."""
    key = (name, np.asarray(As).tobytes(), tg.tobytes(), lo.tobytes(), hi.tobytes())
    if key not in _ORACLE:
        model, gen, k, rows = _case(name)
        out = c_scan(c_oracle(), R, As, gen, rows, tg, lo, hi)
        for a in out:
            a.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def _check(got, ref, what, form, tied=()):
    keep = np.ones(len(ref[0]), bool)
    keep[list(tied)] = False
    win = ref[0] > 0
    worst = float(np.max(np.abs(got[0] - ref[0])[win] / ref[0][win])) if win.any() else 0.0
    WORST[form] = max(WORST.get(form, 0.0), worst)
    print('%s: %d windows (%d skipped), E* %d .. %d, worst relative dCLR %.3e' % (what, len(ref[0]), len(tied), kr.e_star(ref[0]).min(), kr.e_star(ref[0]).max(), worst))
    assert np.isfinite(got[0]).all(), what
    assert kr.e_star(ref[0]).max() <= kr.INSIDE[1]
    for q, nm in ((1, 'x'), (2, 'alpha_beta'), (3, 'A'), (4, 'nSites')):
        assert np.array_equal(got[q][keep], ref[q][keep]), (what, nm, np.where(got[q] != ref[q])[0][:8])
    assert np.allclose(got[0], ref[0], rtol=1e-9, atol=1e-12), (what, worst)
    assert np.array_equal(_bits(got[0][~win]), np.zeros(int((~win).sum()), np.uint64))       # no winner: +0.0, not -0.0


def _in_band(ref, band):
    """The band holds on the oracle fed with the DEVICE's table too (the CPU module proves it on the oracle's own table): every
    inside-band window in [129 000, 131 060], and of a rung's windows as many within +-600 as the CPU module asks for at least."""
    E = kr.e_star(ref[0])
    if band == 'inside':
        assert E.min() >= kr.INSIDE[0] and E.max() <= kr.INSIDE[1], (E.min(), E.max())
    else:
        assert int(np.sum(np.abs(E - kr.RUNGS[band]) <= kr.RUNG_HALF)) >= 12, (band, E.min(), E.max())


def _refused(call):
    from ballermixplus_amd import _lib
    with pytest.raises(_lib.BmxError, match=REFUSED) as e:
        call()
    assert e.value.code == LIMIT


def _want_plan(ctx, kernel, mode, what):
    pl = ctx.plan()
    assert (pl['kernel'], pl['mode']) == (kernel, mode), (what, pl)
    return pl


def _default_kernel(name, stride):
    lds = 'false' if name == 'large' else 'true'
    if name != 's200' and stride <= 5:
        return 'clr_scan_prepared_kernel<%d,%s>' % (16 if stride == 1 else 8, lds), PREPARED
    return 'clr_scan_solo_kernel<%s>' % lds, SOLO


def _bands(ctx, R, name, stride, form, want, profiles=(False,)):
    """Every band of one (set, stride) on the context's current variant: the compared bands against the oracle, then the
    outside band refused (with each profile setting listed)."""
    for band in COMPARED:
        tg, lo, hi = _high_tests(name, band, stride)
        ctx.set_tests(tg, lo, hi)
        _want_plan(ctx, *want, (name, band, stride))
        ctx.scan()
        ref = _oracle(name, R, _grid()[2], tg, lo, hi)
        _in_band(ref, band)
        _check(ctx.fetch(), ref, '%s %s stride %d %s' % (form, name, stride, band), form, kr.TIED.get((name, band, stride), ()))
    tg, lo, hi = _high_tests(name, 'outside', stride)
    ref = _oracle(name, R, _grid()[2], tg, lo, hi)
    assert kr.e_star(ref[0]).min() >= kr.OUTSIDE
    for lo16 in range(0, len(tg), 16):                       # each group of 16 in a scan of its own
        sub = slice(lo16, lo16 + 16)
        ctx.set_tests(tg[sub], lo[sub], hi[sub])
        for on in profiles:
            ctx.set_profiles(7 if on else 0)
            _want_plan(ctx, *want, (name, 'outside', stride))
            ctx.scan()
            _refused(ctx.fetch)
            _refused(ctx.fetch)                              # every time, not only the first
            if on:
                _refused(lambda: ctx.fetch_profile('x'))
        ctx.set_profiles(0)


@pytest.mark.parametrize('name,stride', [(n, s) for n in kr.SETS for s in kr.STRIDES])
def test_default_plans(name, stride, open_ctx):
    """s62: prepared J = 16 / J = 8 / solo at the strides 1 / 5 / 20; s200: solo; large: the <., false> forms."""
    ctx, R = open_ctx(name)
    _bands(ctx, R, name, stride, _default_kernel(name, stride)[0], _default_kernel(name, stride), profiles=(False, True))


VARIANTS = {13: ('clr_scan_prepared_kernel<16,true>', PREPARED), 14: ('clr_scan_prepared_kernel<8,true>', PREPARED),
            15: ('clr_scan_prepared_kernel<4,true>', PREPARED), 16: ('clr_scan_solo_kernel<true>', SOLO),
            12: ('clr_scan_grouped_kernel<16,true,3>', 3), 2: ('clr_scan_kernel<true>', PER_SITE)}


@pytest.mark.parametrize('name,variant', [('s62', v) for v in (13, 14, 15, 16, 12, 2)] + [('s200', 16), ('s200', 2)])
def test_variants(name, variant, open_ctx):
    ctx, R = open_ctx(name)
    ctx.set_variant(variant)
    has_profiles = VARIANTS[variant][1] in (PREPARED, SOLO)
    _bands(ctx, R, name, 1, 'variant %d' % variant, VARIANTS[variant], profiles=(False, True) if has_profiles else (False,))


def _profiles_against_the_oracle(ctx, name, R, As, tg, lo, hi, on, what):
    model, gen, k, rows = _case(name)
    As = np.asarray(As, dtype=np.float64)
    L = c_oracle()
    for nm, n in (('A', len(As)), ('x', R.shape[0]), ('abeta', R.shape[1])):
        p = ctx.fetch_profile(nm)
        assert p.shape == (len(tg), n) and np.isfinite(p).all() and np.all(p >= 0.0), nm
        assert np.array_equal(_bits(p.max(axis=1)), _bits(on[0])), (what, nm)
        for v in range(n):
            if nm == 'A':
                o = c_scan(L, R, As[v:v + 1], gen, rows, tg, lo, hi)[0]
            elif nm == 'x':
                o = c_scan(L, R[v:v + 1], As, gen, rows, tg, lo, hi)[0]
            else:
                o = c_scan(L, R[:, v:v + 1], As, gen, rows, tg, lo, hi)[0]
            assert np.allclose(p[:, v], o, rtol=1e-9, atol=1e-12), (what, nm, v, float(np.max(np.abs(p[:, v] - o))))


@pytest.mark.parametrize('name,stride', [('s62', 1), ('s62', 5), ('s62', 20), ('s200', 1), ('large', 1)])
def test_profiles_inside_the_band(name, stride, open_ctx):
    """All three profiles on the inside-band windows: the scan's fields byte-equal to the scan without profiles, every profile's
    maximum the CLR bit for bit, every column the oracle's scan with that single value; and two scans byte-equal."""
    ctx, R = open_ctx(name)
    tg, lo, hi = _high_tests(name, 'inside', stride)
    ctx.set_tests(tg, lo, hi)
    ctx.scan()
    off = [a.copy() for a in ctx.fetch()]
    ctx.scan()
    for a, b in zip(off, ctx.fetch()):
        assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
    ctx.set_profiles(7)
    ctx.scan()
    on = [a.copy() for a in ctx.fetch()]
    _want_plan(ctx, *_default_kernel(name, stride), ('profiles', name, stride))
    for a, b in zip(off, on):
        assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
    what = 'profiles on, %s stride %d' % (name, stride)
    _in_band(_oracle(name, R, _grid()[2], tg, lo, hi), 'inside')
    _check(on, _oracle(name, R, _grid()[2], tg, lo, hi), what, 'profiles', kr.TIED.get((name, 'inside', stride), ()))
    _profiles_against_the_oracle(ctx, name, R, _grid()[2], tg, lo, hi, on, what)


# ------------------------------------------------------------------------------------------------------------------ low
LOW_FORMS = ([('low', s, 0) for s in kr.STRIDES] + [('low', 1, v) for v in (13, 14, 15, 16, 12, 2)]
             + [('lowL', s, 0) for s in kr.STRIDES])          # 'lowL': the <., false> forms (the 'large' set's default plans)


@pytest.mark.parametrize('name,stride,variant', LOW_FORMS)
def test_low_end(name, stride, variant, open_ctx):
    """Windows whose every grid point is far below neutral, on either side of the -131 071 clamp and far past it, a window with
    an exact zero factor, and one whose first A is deeply negative while the second wins: 'none' is CLR +0.0, lin -1, nSites 0
    and all-zero profiles, without an error.  On every form of the 'high' sets: 'low' for the <., true> ones, 'lowL' (the same
    sites on the sample sizes 150 / 160 / 170) for the <., false> ones."""
    As = _grid(kr.LOW_A)[2]
    ctx, R = open_ctx(name, As)
    ctx.set_variant(variant)
    assert np.all(R[:, :, :8] == -1.0)                       # the device's table too has R = -1 exactly on the rows of share 0.0
    for K in kr.LOW_KS:
        tg, lo, hi, kinds = kr.low_tests(stride, K)
        ref = _oracle(name, R, As, tg, lo, hi)
        assert np.all(ref[3][:-1] == -1) and ref[3][-1] == 1 and 0 < ref[0][-1] < 1e3
        ctx.set_tests(tg, lo, hi)
        pl = ctx.plan()
        if variant == 0:
            assert (pl['kernel'], pl['mode']) == _default_kernel('large' if name == 'lowL' else 's62', stride), pl
        else:
            assert (pl['kernel'], pl['mode']) == VARIANTS[variant], pl
        for which in ((0, 7) if pl['mode'] in (PREPARED, SOLO) else (0,)):
            ctx.set_profiles(which)
            ctx.scan()
            ctx.sync()                                       # no error
            got = ctx.fetch()
            _check(got, ref, '%s stride %d variant %d K %d profiles %d (%s)' % (name, stride, variant, K, which, pl['kernel']), name)
            rec = ctx.fetch_records()
            none = np.arange(len(tg) - 1)
            assert np.array_equal(_bits(got[0][none]), np.zeros(len(none), np.uint64)) and np.array_equal(_bits(rec['clr'][none]), np.zeros(len(none), np.uint64))
            assert np.all(rec['lin'][none] == -1) and np.all(rec['nsites'][none] == 0) and np.all(got[4][none] == 0)
            assert all(np.all(got[q][none] == -1) for q in (1, 2, 3))
            assert got[3][-1] == 1 and got[4][-1] == 64      # 'mixed': nothing stuck from A = 1
            if which:
                for nm in ('A', 'x', 'abeta'):
                    p = ctx.fetch_profile(nm)
                    assert np.array_equal(_bits(p[none]), np.zeros(p[none].shape, np.uint64)), nm
                    assert np.array_equal(_bits(p[-1].max()), _bits(got[0][-1]))
                assert ctx.fetch_profile('A')[-1, 0] == 0.0  # 'mixed' at A = 1: below neutral
        ctx.set_profiles(0)


# ---------------------------------------------------------------------------------------------------------------- wideA
def _wide_tests(stride):
    gen = _case('wide')[1]
    idx = np.arange(0, kr.WIDE_N, stride)
    return gen[idx], np.zeros(len(idx), np.int64), np.full(len(idx), kr.WIDE_N - 1, np.int64)


@pytest.mark.parametrize('grid', list(kr.WIDE_NA) + ['dup'])
def test_wide_A_grids(grid, open_ctx):
    """nA = 8189 and 8190 go through the packed keys (prepared J = 16 / 8, round-2 grouped on request), 8191 and 8192 to the
    one-test-site-per-wave kernels at every stride; winners at the indices 0, 4095, 4096, nA - 2 and nA - 1."""
    nA = 8190 if grid == 'dup' else grid
    As = kr.wide_grid(nA, dup=grid == 'dup')
    ctx, R = open_ctx('wide', As)
    useful = np.nonzero(As < 1e9)[0]
    for stride, variant in ((1, 0), (5, 0), (20, 0), (1, 12)):
        ctx.set_variant(variant)
        tg, lo, hi = _wide_tests(stride)
        ctx.set_tests(tg, lo, hi)
        pl = ctx.plan()
        if nA >= kr.SENTINEL:
            assert pl['mode'] in (SOLO, PER_SITE) and pl['J'] <= 1 and pl['kernel'].startswith(('clr_scan_solo_kernel<', 'clr_scan_kernel<')), (nA, stride, variant, pl)
        elif variant == 12:
            assert (pl['kernel'], pl['mode']) == VARIANTS[12], pl
        elif stride <= 5:
            assert (pl['kernel'], pl['mode']) == ('clr_scan_prepared_kernel<%d,true>' % (16 if stride == 1 else 8), PREPARED), pl
        ref = _oracle('wide', R, As, tg, lo, hi)
        ctx.scan()
        got = ctx.fetch()
        _check(got, ref, 'wideA %s stride %d variant %d (%s)' % (grid, stride, variant, pl['kernel']), 'wideA ' + pl['kernel'])
        if stride == 1:
            wins = [int(np.sum(got[3] == u)) for u in kr.wide_useful(nA)]
            assert (min(wins[:4]) >= 20 and wins[4] == 0 and np.sum(got[3] == 5) >= 20) if grid == 'dup' else min(wins) >= 20, wins
        if pl['mode'] in (PREPARED, SOLO) and stride == 1:
            ctx.set_profiles(1)
            ctx.scan()
            p = ctx.fetch_profile('A')
            dead = np.delete(p, useful, axis=1)
            assert np.array_equal(_bits(dead), np.zeros(dead.shape, np.uint64))            # +0.0 at every index out of reach
            assert np.array_equal(_bits(p.max(axis=1)), _bits(got[0]))
            ctx.set_profiles(0)


@pytest.mark.parametrize('at', (8189, 0))
def test_both_fields(at, open_ctx):
    """The inside-band windows of 's62' with nA = 8190 and A = 20 alone in reach, at index 8189 and at index 0."""
    As = kr.both_grid(at)
    ctx, R = open_ctx('s62', As)
    for stride, variant in ((1, 0), (5, 0), (1, 12), (1, 15)):
        ctx.set_variant(variant)
        tg, lo, hi = _high_tests('s62', 'inside', stride)
        ctx.set_tests(tg, lo, hi)
        pl = ctx.plan()
        assert pl['mode'] in (PREPARED, 3) and pl['J'] >= 4, pl
        ref = _oracle('s62', R, As, tg, lo, hi)
        assert np.all(ref[3] == at)
        _in_band(ref, 'inside')
        ctx.scan()
        _check(ctx.fetch(), ref, 'both at %d stride %d variant %d' % (at, stride, variant), 'both ' + pl['kernel'], kr.TIED.get(('s62', 'inside', stride), ()))


# -------------------------------------------------------------------------------------------------------------- refusal
def _mixed_tests(name, stride, j):
    """The inside-band windows with window j replaced by the same site's outside-band window."""
    tg, lo, hi = _high_tests(name, 'inside', stride)
    _, lo2, hi2 = _high_tests(name, 'outside', stride)
    lo, hi = lo.copy(), hi.copy()
    lo[j], hi[j] = lo2[j], hi2[j]
    return tg, lo, hi


@pytest.mark.parametrize('name,stride', [('s62', 1), ('s62', 20), ('s200', 5)])
def test_refusal_is_kept_per_slot(name, stride, open_ctx):
    """Inside-band windows plus ONE outside window: refused at every fetch until the slot is scanned again; rescanned without
    that window it is byte-equal to a fresh context; another slot, scanned before, stays fetchable and unchanged."""
    from ballermixplus_amd import _lib
    model, gen, k, rows = _case(name)
    ctx, R = open_ctx(name)
    tg, lo, hi = _high_tests(name, 'inside', stride)
    ctx.set_tests(tg, lo, hi)
    ctx.scan()
    first = [a.copy() for a in ctx.fetch()]                  # slot 0
    other, _ = open_ctx(name)                                # a context that never scans anything else
    other.set_tests(tg, lo, hi)
    other.scan()
    fresh = [a.copy() for a in other.fetch()]
    ctx.select_slot(1)
    ctx.set_sites(gen, rows)
    for j in (0, 17, 31):
        ctx.set_tests(*_mixed_tests(name, stride, j))
        ctx.scan()
        for call in (ctx.fetch, ctx.sync, ctx.fetch_records, ctx.fetch, ctx.pack_records):
            _refused(call)
        with pytest.raises(_lib.BmxError, match='slot 1'):
            ctx.fetch()
        ctx.select_slot(0)                                   # the other slot: fetchable, unchanged
        ctx.sync()
        for a, b in zip(first, ctx.fetch()):
            assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
        ctx.select_slot(1)
        _refused(ctx.fetch)                                  # still, after the other slot was read
    ctx.set_tests(tg, lo, hi)
    ctx.scan()
    ctx.sync()
    again = ctx.fetch()
    for a, b in zip(fresh, again):
        assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
    rec = ctx.pack_records()                                 # both slots, in slot order
    assert len(rec) == 2 * len(tg) and np.array_equal(_bits(rec['clr']), np.concatenate([_bits(first[0])] * 2))


def test_refusal_at_every_exit(open_ctx, tmp_path):
    """sync, fetch, fetch_records, fetch_profile, pack_records (host and device), copy_records, scan_write, null_accumulate,
    locate_accumulate, bmx_scan and bmx_scan_multi on an outside-band scan."""
    from ballermixplus_amd import _lib, null
    name, stride = 's62', 1
    model, gen, k, rows = _case(name)
    ctx, R = open_ctx(name)
    tg, lo, hi = _high_tests(name, 'outside', stride)
    M = len(tg)
    ctx.set_profiles(7)
    ctx.set_tests(tg, lo, hi)
    ctx.scan()
    other, _ = open_ctx(name)                                # its records: M x 16 bytes of this GPU's memory to copy into
    other.set_tests(*_high_tests(name, 'rung1', stride))
    other.scan()
    before = other.fetch_records().copy()
    dst = other.records()
    for call in (ctx.sync, ctx.fetch, ctx.fetch_records, lambda: ctx.fetch_profile('A'), lambda: ctx.fetch_profile('abeta'), ctx.pack_records,
                 lambda: ctx.pack_records(device_ptr=dst, cap=M), lambda: ctx.copy_records(dst, M), ctx.fetch):
        _refused(call)
    assert np.array_equal(other.fetch_records().view(np.uint8), before.view(np.uint8))      # nothing was copied out
    ctx.set_profiles(0)
    xs, ab, As = _grid()
    path = str(tmp_path / 'out.txt')
    _refused(lambda: ctx.scan_write(path, np.arange(M), tg, [repr(v) for v in xs], [repr(v) for v in ab], [repr(v) for v in As], chunk=16))
    _refused(ctx.fetch)
    # locate: the state outlives set_tests, so an in-range scan starts it and the replicate's scan is the outside one
    tin = _high_tests(name, 'inside', stride)
    ctx.set_tests(*tin)
    ctx.scan()
    ctx.locate_begin([0], [M - 1], 2)
    ctx.set_tests(tg, lo, hi)
    ctx.scan()
    _refused(lambda: ctx.locate_accumulate(0))
    ctx.set_tests(*tin)
    ctx.scan()
    ctx.locate_accumulate(0)                                 # the next replicate, in range, is taken
    # null: the observed scan in range, a replicate whose permuted rows put windows past it (the key is found with the oracle)
    ctx.null_begin()
    L = c_oracle()
    for key in range(1, 60):
        sigma = null.block_permutation(len(rows), key, 1)
        E = kr.e_star(c_scan(L, R, As, gen, rows[sigma], *tin)[0])
        if E.max() >= kr.OUTSIDE + 100:
            break
    else:
        pytest.fail('no permutation key among 59 puts a window past the range')
    print('null: key %d, E* of the permuted windows %d .. %d' % (key, E.min(), E.max()))
    ctx.permute_rows(key, 1)
    ctx.scan()
    _refused(ctx.null_accumulate)
    ctx.restore_rows()
    # the one-shot calls
    clr = np.zeros(M)
    ix, ia, iA, ns = (np.zeros(M, np.int32) for _ in range(4))
    A = _lib.f64(As)
    g, r, t, l, h = _lib.f64(gen), _lib.i32(rows), _lib.f64(tg), _lib.i64(lo), _lib.i64(hi)
    head = (C.byref(model.c), _lib.as_dp(A), len(A), len(g), _lib.as_dp(g), _lib.as_ip(r), M, _lib.as_dp(t), _lib.as_lp(l), _lib.as_lp(h),
            _lib.as_dp(clr), _lib.as_ip(ix), _lib.as_ip(ia), _lib.as_ip(iA), _lib.as_ip(ns))
    Lb = _lib.lib()
    _refused(lambda: _lib.check(Lb.bmx_scan(*head, 0)))
    dev = _lib.i32([0, 0])
    _refused(lambda: _lib.check(Lb.bmx_scan_multi(*head, 2, _lib.as_ip(dev))))
    assert np.all(clr == 0.0)                                # nothing was handed out


@pytest.mark.parametrize('name', ('s62', 's200'))
def test_off_grid_calls_past_the_range(name, open_ctx):
    """surface, surfaces and eval_points are plain sums: on an outside-band window they still agree with the oracle."""
    ctx, R = open_ctx(name)
    xs, ab, As = _grid()
    tg, lo, hi = _high_tests(name, 'outside', 20)
    ref = _oracle(name, R, As, tg, lo, hi)
    assert kr.e_star(ref[0]).min() >= kr.OUTSIDE
    ctx.set_tests(tg, lo, hi)
    pick = [0, 13, 31]
    Ts, nss = ctx.surfaces(pick)
    for n, j in enumerate(pick):
        T, ns = ctx.surface(tg[j], lo[j], hi[j])
        assert np.array_equal(_bits(T), _bits(Ts[n])) and np.array_equal(ns, nss[n])
        flat = np.asarray(T).reshape(-1)
        top = int(np.argmax(flat))
        assert np.isfinite(flat).all() and abs(flat[top] - ref[0][j]) <= 1e-9 * ref[0][j], (j, flat[top], ref[0][j])
        assert (top // len(ab), top % len(ab)) == (int(ref[1][j]), int(ref[2][j])) and ns[0] == ref[4][j]
    Tp, nsp = ctx.eval_points(As[0], np.asarray(xs)[ref[1]], np.asarray(ab)[ref[2]])
    print('%s: eval_points on outside-band windows, worst relative difference %.3e' % (name, float(np.max(np.abs(Tp - ref[0]) / ref[0]))))
    assert np.array_equal(nsp, ref[4]) and np.allclose(Tp, ref[0], rtol=1e-9, atol=0)


@pytest.fixture(scope='module', autouse=True)
def report_worst_per_form():
    """No test: after the module's last test, prints the worst relative dCLR per kernel form that _check saw in this run (DESIGN.md
    section 6 quotes it).  Every figure was asserted where it was measured."""
    yield
    for form in sorted(WORST):
        print('worst relative dCLR, %s: %.3e' % (form, WORST[form]))
