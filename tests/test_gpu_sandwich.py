"""The sandwich pieces of a window on the GPU (--sandwich): Context.refine_R against the oracle's table, bmx_ctx_sandwich against
the host restatement on the catalogue of sandwichcases.py (fed the device's own five columns, so the comparison is about
summation), J == H bit for bit at B = 1, T against bmx_ctx_eval_points, independence of the list, the chunk seam, the
replicated-sites identity, every error code, and the CLI end to end."""
import functools
import os

import numpy as np
import pytest

import cases
import sandwichcases as sc
from test_gpu_refine import _case_ctx, _cli, _engine, _read
from test_gpu_surfaces import EX1

from ballermixplus_amd import _lib, influence, peaks, refine, sandwich, surfaces
from ballermixplus_amd._lib import BmxError

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(name):
    c = sc.case(name)
    return c, sc.context(c, _engine())


@functools.lru_cache(maxsize=None)
def _device_tabs(name, p, hx=sandwich.HX, hv=sandwich.HV):
    """The device's own five columns of point p of the case."""
    c, ctx = _case(name)
    _, x, ab = c.points[p]
    return np.array([ctx.refine_R(xx, aa) for xx, aa in sandwich.shifted_points(x, ab, hx, hv)])


def _call(c, ctx, block, entries=None, hx=None, hv=None):
    e = c.entries if entries is None else [c.entries[q] for q in entries]
    pts = np.array([c.points[p] for _, p in e], dtype=np.float64).reshape(-1, 3)
    return ctx.sandwich([w for w, _ in e], pts[:, 0], pts[:, 1], pts[:, 2], block, hx, hv)


def _bytes(out, q):
    return b''.join(np.ascontiguousarray(out[k][q]).tobytes() for k in ('T', 'g', 'H', 'J', 'nsites', 'nskipped', 'nblocks'))


# ------------------------------------------------------------------------------------------------- refine_R, the oracle

@pytest.mark.parametrize('name', sc.NAMES)
def test_refine_R_against_the_oracle(name):
    """1 + R relative R_TOL = 1e-9 at the five points of every point of the case (test_sandwich_cpu.py shows every normalising
    base of these points is >= seltable.WELL, so the plain bar holds)."""
    c, ctx = _case(name)
    worst = 0.0
    for p in range(len(c.points)):
        dev, ref = _device_tabs(name, p), sc.oracle_tabs(c, p)
        assert dev.shape == ref.shape and np.array_equal(np.isnan(dev), np.isnan(ref))
        ok = ~np.isnan(ref)
        ratio = np.abs(dev[ok] - ref[ok]) / (sc.R_TOL * np.abs(1.0 + ref[ok]) + 1e-300)
        worst = max(worst, float(ratio.max()))
    print('%s: worst |d(1 + R)| / (1e-9 (1 + R)) = %.3e' % (name, worst))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------- against the host restatement

@pytest.mark.parametrize('block', sc.BLOCKS)
@pytest.mark.parametrize('name', sc.NAMES)
def test_against_host_sandwich(name, block):
    c, ctx = _case(name)
    got = _call(c, ctx, block)
    assert got['T'].shape == (len(c.entries),) and got['g'].shape == (len(c.entries), 3) and got['H'].shape == got['J'].shape == (len(c.entries), 6)
    worst = 0.0
    for q, (w, p) in enumerate(c.entries):
        h = sc.host(c, q, _device_tabs(name, p), block)
        assert (got['nsites'][q], got['nskipped'][q], got['nblocks'][q]) == (h['nsites'], h['nskipped'], h['nblocks']), (name, q)
        if h['nsites'] == h['nskipped']:
            assert got['T'][q] == -np.inf and not got['g'][q].any() and not got['H'][q].any() and not got['J'][q].any()
            continue
        assert np.isfinite(h['T']) and h['T'] != 0.0
        pairs = [(got['T'][q], h['T'], abs(h['T']))] + [(got[k][q], h[k], h['abs' + k]) for k in ('g', 'H', 'J')]       # T: relative
        for dev, ref, scale in pairs:
            ratio = np.max(np.abs(dev - ref) / (sc.TOL * np.asarray(scale) + 1e-300))
            worst = max(worst, float(ratio))
            assert ratio <= 1.0, (name, block, q, ratio)
    print('%s, B = %d: worst ratio to the bound %.3e%s; kernel %.3f ms' % (name, block, worst, ' (ABOVE A TENTH)' if worst > 0.1 else '',
                                                                          ctx.sandwich_ms()))
    if name == 'skip':
        assert got['nskipped'][0] == 1
    else:
        assert not got['nskipped'].any()
    if name == 'one':
        assert set(sc.SIZES) | {sc.N} <= set(got['nsites'].tolist())
    if name == 'slab':
        assert (ctx.model.rows * 45 + 15) // 16 * 16 > 32 * 1024            # the workspace in the slab


@pytest.mark.parametrize('name', sc.NAMES)
def test_block_one_gives_J_equal_to_H_bit_for_bit(name):
    c, ctx = _case(name)
    got = _call(c, ctx, 1)
    assert got['J'].tobytes() == got['H'].tobytes() and np.array_equal(got['nblocks'], got['nsites'] - got['nskipped'])
    assert np.any(got['H'] != 0.0)


@pytest.mark.parametrize('name', sc.NAMES)
def test_T_agrees_with_eval_points(name):
    c, ctx = _case(name)
    got = _call(c, ctx, 7)
    worst = 0.0
    for p, (A, x, ab) in enumerate(c.points):
        T, ns = ctx.eval_points(A, x, ab)
        for q, (w, pp) in enumerate(c.entries):
            if pp != p:
                continue
            assert got['nsites'][q] == ns[w]
            if got['nskipped'][q]:
                continue                    # eval_points has no skipping rule: its T is -inf there
            if not np.isfinite(T[w]):
                assert got['T'][q] == T[w] == -np.inf
            else:
                worst = max(worst, abs(got['T'][q] - T[w]) / abs(T[w]))
    print('%s: worst relative |T - eval_points| %.3e' % (name, worst))
    assert worst <= 1e-12


# --------------------------------------------------------------------------------------------------------- independence

def test_a_window_alone_in_a_list_twice_and_reversed_gives_the_same_bytes():
    c, ctx = _case('three')
    n = len(c.entries)
    for block in (1, 7, 64):
        full = _call(c, ctx, block)
        rev = _call(c, ctx, block, list(range(n))[::-1])
        twice = _call(c, ctx, block, list(range(n)) + list(range(n)))
        for q in range(n):
            assert _bytes(full, q) == _bytes(rev, n - 1 - q) == _bytes(twice, q) == _bytes(twice, n + q), (block, q)
        for q in (0, 3, 10, 19, 27, 28, 38):
            assert _bytes(_call(c, ctx, block, [q]), 0) == _bytes(full, q), (block, q)
    # the steps are part of the window's definition, the list is not
    other = _call(c, ctx, 7, hx=2 * sandwich.HX, hv=2 * sandwich.HV)
    assert other['T'].tobytes() == _call(c, ctx, 7)['T'].tobytes() and other['H'].tobytes() != _call(c, ctx, 7)['H'].tobytes()


def test_the_chunk_seam():
    """A list one chunk and three windows long: the windows either side of the seam are what they are alone."""
    c, ctx = _case('one')
    chunk = sc.header_constant('BMX_SANDWICH_CHUNK_WINDOWS')
    n = chunk + 3
    real = {0: 10, chunk - 1: 19, chunk: 27, chunk + 1: 30, n - 1: 12}
    entries = [0] * n                       # the empty window everywhere else
    for at, q in real.items():
        entries[at] = q
    got = _call(c, ctx, 7, entries)
    for at, q in real.items():
        assert _bytes(got, at) == _bytes(_call(c, ctx, 7, [q]), 0), at
    assert got['T'][5] == -np.inf and got['nsites'][5] == 0
    print('%d windows: kernels %.1f ms' % (n, ctx.sandwich_ms()))


def test_replicated_sites_on_the_device():
    c, ctx = _case('one')
    m = 4
    gen, rows, lo, hi = sc.replicated(c, m)
    ctx.select_slot(1)
    try:
        ctx.set_sites(gen, rows)
        ctx.set_tests(c.tg, lo, hi)
        got = _call(c, ctx, m)
    finally:
        ctx.select_slot(0)
    one = _call(c, ctx, 1)
    st = sc.setup_of(c)
    checked = 0
    for q, (w, p) in enumerate(c.entries):
        assert got['nsites'][q] == m * one['nsites'][q] and got['nblocks'][q] == one['nblocks'][q]
        s = sandwich.summarise(got['T'][q], got['g'][q], got['H'][q], got['J'][q], st, c.points[p])
        if one['nsites'][q] < 8:
            continue
        assert s['status'] == 'ok'
        assert np.all(np.abs(s['eigenvalues'] - 4.0) <= 1e-9), (q, s['eigenvalues'])
        assert all(abs(s['se'][k] - 2.0 * s['se_naive'][k]) <= 1e-9 * s['se'][k] for k in s['kept'])
        checked += 1
    assert checked >= 20


# --------------------------------------------------------------------------------------------------------------- errors

def test_errors():
    L = _lib.lib()
    INVALID, LIMIT, STATE = -1, -4, -5
    c = sc.case('one')
    one = np.zeros(1, dtype=np.int32)
    d1 = np.array([700.0])
    assert L.bmx_ctx_sandwich(None, 1, _lib.as_ip(one), _lib.as_dp(d1), _lib.as_dp(d1), _lib.as_dp(d1), 1, 1e-3, 1e-2,
                              None, None, None, None, None, None, None) == INVALID
    assert L.bmx_ctx_sandwich_ms(None, None) == INVALID and L.bmx_ctx_refine_R(None, 0.3, 10.0, None) == INVALID
    eng = _engine()
    ctx = eng.Context(0)
    ctx.set_model(sc.model_of(c, eng), c.As)
    ctx.set_sites(c.gen, c.rows)
    for call in (lambda: ctx.sandwich([0], 700.0, 0.3, 10.0), ctx.sandwich_ms, lambda: ctx.refine_R(0.3, 10.0)):    # no test sites yet
        with pytest.raises(BmxError) as e:
            call()
        assert e.value.code == STATE
    ctx.set_tests(c.tg, c.lo, c.hi)
    M = len(c.tg)
    T = np.full(2, -7.0)
    g, H, J = np.full((2, 3), -7.0), np.full((2, 6), -7.0), np.full((2, 6), -7.0)
    cnt = [np.full(2, -7, dtype=np.int32) for _ in range(3)]

    def raw(n, tests, A, x, ab, block=1, hx=1e-3, hv=1e-2):
        p = lambda a, f: None if a is None else f(np.ascontiguousarray(a))
        return L.bmx_ctx_sandwich(ctx._h, n, p(tests, _lib.as_ip), p(A, _lib.as_dp), p(x, _lib.as_dp), p(ab, _lib.as_dp), block, hx, hv,
                                  _lib.as_dp(T), _lib.as_dp(g), _lib.as_dp(H), _lib.as_dp(J), *[_lib.as_ip(a) for a in cnt])

    t2 = np.array([3, 4], dtype=np.int32)
    A2, x2, ab2 = np.array([700.0, 50.0]), np.array([0.3, 0.137]), np.array([10.0, 3.3])
    i32 = lambda v: np.array(v, dtype=np.int32)
    assert raw(-1, t2, A2, x2, ab2) == INVALID
    for k in range(4):                                      # every NULL input with n > 0
        args = [t2, A2, x2, ab2]
        args[k] = None
        assert raw(2, *args) == INVALID, k
    for bad in ([-1, 0], [0, M]):
        assert raw(2, i32(bad), A2, x2, ab2) == INVALID and 'index' in L.bmx_last_error().decode()
    for bad in (0.0, -1.0, np.inf, np.nan):
        assert raw(2, t2, np.array([700.0, bad]), x2, ab2) == INVALID, bad
        assert raw(2, t2, A2, x2, np.array([bad, 3.3])) == INVALID, bad
    for bad in (1e-3, 0.0, -0.2, 0.9995, 1.0, np.nan):  # x - hx <= 0 or x + hx >= 1
        assert raw(2, t2, A2, np.array([0.3, bad]), ab2) == INVALID, bad
    assert raw(2, t2, A2, np.array([0.3, 1e-3 + 1e-9]), ab2) == 0
    for bad in (0, -3):
        assert raw(2, t2, A2, x2, ab2, block=bad) == INVALID
    for bad in (0.0, -1e-3, np.inf, np.nan):
        assert raw(2, t2, A2, x2, ab2, hx=bad) == INVALID and raw(2, t2, A2, x2, ab2, hv=bad) == INVALID
    T[:], g[:], H[:], J[:] = -7.0, -7.0, -7.0, -7.0
    for a in cnt:
        a[:] = -7
    assert raw(sc.header_constant('BMX_SANDWICH_MAX_WINDOWS') + 1, t2, A2, x2, ab2) == LIMIT
    assert raw(-1, t2, A2, x2, ab2) == INVALID and raw(2, t2, A2, x2, ab2, block=0) == INVALID
    assert (T == -7.0).all() and (g == -7.0).all() and (H == -7.0).all() and (J == -7.0).all() and all((a == -7).all() for a in cnt)
    fresh = eng.Context(0)                                  # no failed call counts as a call; n == 0 does
    fresh.set_model(sc.model_of(c, eng), c.As)
    fresh.set_sites(c.gen, c.rows)
    fresh.set_tests(c.tg, c.lo, c.hi)
    assert L.bmx_ctx_sandwich(fresh._h, 2, _lib.as_ip(t2), _lib.as_dp(A2), _lib.as_dp(x2), _lib.as_dp(ab2), 0, 1e-3, 1e-2,
                              None, None, None, None, None, None, None) == INVALID
    with pytest.raises(BmxError) as e:
        fresh.sandwich_ms()
    assert e.value.code == STATE
    assert L.bmx_ctx_sandwich(fresh._h, 0, None, None, None, None, 1, 1e-3, 1e-2, None, None, None, None, None, None, None) == 0
    assert fresh.sandwich_ms() == 0.0
    r = fresh.sandwich([], [], [], [])
    assert r['T'].shape == (0,) and r['H'].shape == (0, 6)
    # every output may be NULL
    assert L.bmx_ctx_sandwich(fresh._h, 2, _lib.as_ip(t2), _lib.as_dp(A2), _lib.as_dp(x2), _lib.as_dp(ab2), 1, 1e-3, 1e-2,
                              None, None, None, None, None, None, None) == 0
    assert raw(2, t2, A2, x2, ab2) == 0 and (cnt[0] == [63, 64]).all() and np.isfinite(T).all()
    fresh.close()
    # refine_R: eval_points' argument rules
    R = np.zeros(ctx.model.rows)
    for x, ab in ((0.0, 10.0), (1.0, 10.0), (np.nan, 10.0), (0.3, 0.0), (0.3, -1.0), (0.3, np.inf), (0.3, np.nan)):
        assert L.bmx_ctx_refine_R(ctx._h, x, ab, _lib.as_dp(R)) == INVALID, (x, ab)
    assert L.bmx_ctx_refine_R(ctx._h, 0.3, 10.0, None) == INVALID and L.bmx_ctx_refine_R(ctx._h, 0.3, 10.0, _lib.as_dp(R)) == 0
    ctx.close()


def test_the_call_leaves_the_slot_as_it_was_and_matches_the_grid_table():
    """On a grid point refine_R is the table's column to K1's accuracy, and a call changes nothing of the slot's scan."""
    c, ctx = _case('one')
    ctx.scan()
    before = ctx.fetch()
    _call(c, ctx, 7)
    after = ctx.fetch()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    _, R = ctx.fetch_lut()
    col = ctx.refine_R(c.xs[1], c.abetas[1])
    ok = ~np.isnan(col)
    assert np.array_equal(ok, ~np.isnan(R[1, 1])) and np.all(np.abs(col[ok] - R[1, 1][ok]) <= 1e-9 * np.abs(1.0 + R[1, 1][ok]))


# ------------------------------------------------------------------------------------------------------------------ CLI

def test_cli_end_to_end(tmp_path):
    plain, sw = str(tmp_path / 'plain.txt'), str(tmp_path / 'sw.txt')
    G = '0.0001'
    _cli(EX1 + ['-o', plain, '--peaks', G, '--refine'])
    r = _cli(EX1 + ['-o', sw, '--peaks', G, '--refine', '--sandwich', '--sandwichBlock', '8'])
    assert sorted(os.listdir(tmp_path)) == ['plain.txt', 'plain.txt.peaks.txt', 'plain.txt.refined.txt', 'sw.txt', 'sw.txt.peaks.txt',
                                            'sw.txt.refined.txt', 'sw.txt.sandwich.txt']
    assert _read(plain) == _read(sw) and _read(refine.output_name(plain)) == _read(refine.output_name(sw))
    assert _read(peaks.output_name(plain)) == _read(peaks.output_name(sw))
    assert 'Sandwich: ' in r.stdout and 'blocks of 8 site/s' in r.stdout and '--sandwichMax' not in r.stdout
    # the same windows through the library
    opt, case, ts, sel = _case_ctx(cases.ALL_CASES['ex1_B2'][0])
    ctx = sel.ctx
    ctx.set_tests(ts.test_gen, ts.lo, ts.hi)
    ctx.scan()
    clr, ix, ia, iA, _ = ctx.fetch()
    called = ctx.peaks(float(G), 0.0, peaks.FRAC)
    ctx.refine(0.0)
    ref = ctx.fetch_refined()
    rows, dropped = surfaces.select(clr, iA, 0.0, called['row'], sandwich.MAX_WINDOWS)
    assert len(rows) >= 1 and dropped == 0
    refined = ref['rounds'][rows] >= 0
    assert refined.all()
    A, x, ab = ref['A'][rows], ref['x'][rows], ref['abeta'][rows]
    first = ctx.sandwich(rows, A, x, ab, 8)
    second = ctx.sandwich(rows, A, x, ab, 8, 2 * sandwich.HX, 2 * sandwich.HV)
    phys, gen = surfaces.labels(ts, rows.tolist())
    nx, nab = len(sel.grid_x), len(sel.grid_abeta)
    lin = (iA.astype(np.int64) * nx + ix) * nab + ia
    strings = [(repr(float(ref['x'][t])), repr(float(ref['abeta'][t])), repr(float(ref['A'][t]))) if ref['clr'][t] > clr[t]
               else influence.grid_strings(int(lin[t]), sel) for t in rows.tolist()]
    want = sandwich.rows_of(phys, gen, [repr(float(v)) for v in clr[rows]], strings, ['refined'] * len(rows),
                            list(zip(A.tolist(), x.tolist(), ab.tolist())), refine.Setup(sel.grid_A, sel.grid_x, sel.grid_abeta), first, second)
    got = open(sandwich.output_name(sw)).read()
    assert got == sandwich.HEADER + ''.join(want)
    names, table = sandwich.read_table(sandwich.output_name(sw))
    main = {tuple(l.split('\t')[:2]): l.split('\t') for l in open(sw).readlines()[1:]}
    for row in table:
        assert row[:3] == main[(row[0], row[1])][:3] and row[9] == 'refined' and row[22] in ('ok', 'unstable', 'singular')
    print('\n'.join('\t'.join(r) for r in table[:5]))
    ctx.close()
    # without --refine the point is the grid argmax, and --sandwichMin selects without --peaks
    mn = str(tmp_path / 'mn.txt')
    r2 = _cli(EX1 + ['-o', mn, '--sandwich', '--sandwichMin', '0', '--sandwichMax', '3'])
    names, table = sandwich.read_table(sandwich.output_name(mn))
    main = {tuple(l.rstrip('\n').split('\t')[:2]): l.rstrip('\n').split('\t') for l in open(mn).readlines()[1:]}
    assert _read(mn) == _read(plain) and len(table) == 3 and 'dropped (the 3 with the highest CLR are kept)' in r2.stdout
    for row in table:
        assert row[:6] == main[(row[0], row[1])][:6] and row[9] == 'grid'
