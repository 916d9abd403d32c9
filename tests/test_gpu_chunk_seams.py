"""bmx_ctx_surfaces, _influence, _fit, _cond_surfaces and _base_surfaces across their chunk seams (tests/chunkseams.py holds the cases and the
restated chunk rules; tests/test_chunkseams_cpu.py shows on the host that every case crosses the seam it is named for).

Every call lists tests[q] = q mod 13 over 13 distinct test sites, long enough for a second (or third) chunk.  Two layers:
  * bitwise against a short call: entry q of the long call equals, as bytes (NaNs by bit pattern), entry q mod 13 of ONE call that
    lists the 13 once -- every entry, every output array.  13 divides no chunk length, so a chunk that read or wrote at offset 0
    again would give the numbers of other windows.
  * the 13-entry call against the host restatements (surfaces.host_surface, influence.host_influence, fit.host_fit,
    conditional.host_cond_surface) on the device's own table, at the tolerances those features have: influencecases.REL_TOL of
    max |T|, fitcases.TOL * max(1, n_d), condcases.REL_TOL of the conditional scale; integer fields exact; lin and lin_b exact
    where the host margin exceeds twice the tolerance (at least 99 % of the blocks).  base_surfaces, after ONE baseline_add, against
    cond_surfaces of every window given that locus: the same bytes, which is the contract between the two.
The one-window case lists three windows once: the long one against the vectorised one-point jackknife of chunkseams.py, and the
three against calls that list them apart.

Seconds per test on an MI355X (pytest --durations=0):
    test_block_seam_one_window 3.75 (one thread sums the long window's 4.26 M terms: kernels 1.8 s per call, two calls)
    test_fit_workspace_seam 0.34            test_bytes_seam_surfaces 0.27           test_range_pass_seam 0.25
    test_fit_outputs_seam 0.21              test_threads_seam_cond_surfaces 0.17    test_threads_seam_surfaces 0.14
    test_block_seam_many_windows 0.14       test_bytes_seam_cond_surfaces 0.06      test_bytes_seam_influence 0.05, 0.04
    test_fit_the_two_homes_agree_bit_for_bit 0.02       test_bytes_seam_cond_surfaces_three_chunks_without_T < 0.005
"""
import functools
import time

import numpy as np
import pytest

import chunkseams as cs
import condcases as cc
import fitcases as fc
import influencecases as ic

from ballermixplus_amd import _lib, conditional, fit, influence, surfaces

pytestmark = pytest.mark.gpu

K = cs.K


def _engine():
    from ballermixplus_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def _zcut():
    return float(_lib.lib().bmx_alpha_cut())


@functools.lru_cache(maxsize=None)
def _case(name):
    return cs.CASES[name](_zcut())


_CTX = {}


def _ctx(scene):
    """A scene's context and the device's own table."""
    if scene not in _CTX:
        ctx = cs.scene(scene).context(_engine())
        _CTX[scene] = (ctx, ctx.fetch_lut()[1])
    return _CTX[scene]


@pytest.fixture(scope='module', autouse=True)
def _release():
    """The contexts hold chunk-sized device buffers and four million blocks on the host: closed when the module is done."""
    yield
    for ctx, _ in _CTX.values():
        ctx.close()
    _CTX.clear()
    for f in (_short_surfaces, _short_influence, _short_cond, _short_base, _short_fit):
        f.cache_clear()


def _u(a):
    a = np.ascontiguousarray(a)
    return a.view('u%d' % a.dtype.itemsize)


def _rot_equal(long, short, what):
    """long[q] is short[q mod 13], byte for byte, for every q."""
    L, S = _u(long), _u(short)
    assert len(S) == K and L.shape[1:] == S.shape[1:] and L.dtype == S.dtype, what
    for r in range(K):
        part = L[r::K]
        same = part == S[r]
        if not same.all():
            k = int(np.flatnonzero(~same.reshape(len(part), -1).all(axis=1))[0])
            q = r + K * k
            twin = [j for j in range(K) if np.array_equal(L[q], S[j])]
            raise AssertionError('%s: entry %d of %d is not entry %d of the 13-entry call (it is that of %s); %d entries of this residue differ'
                                 % (what, q, len(L), r, twin or 'none of the 13', int((~same.reshape(len(part), -1).all(axis=1)).sum())))


def _infl_rot_equal(r, short, what):
    """Every per-window and per-block array of a long influence call against the 13-entry call."""
    n = len(r['T_max'])
    assert r['offset'][0] == 0 and len(r['offset']) == n + 1
    for k in ('T_max', 'lin', 'ns_min', 'first_block'):
        _rot_equal(r[k], short[k], '%s %s' % (what, k))
    cnt, cnt13 = np.diff(r['offset']), np.diff(short['offset'])
    _rot_equal(cnt, cnt13, what + ' blocks per window')
    assert all(len(r[k]) == r['offset'][-1] for k in ('m', 'contrib', 'L', 'blin'))
    for j in range(K):
        c, o13 = int(cnt13[j]), int(short['offset'][j])
        if c:
            at = r['offset'][:-1][j::K][:, None] + np.arange(c)
            for k in ('m', 'contrib', 'L', 'blin'):
                got, want = _u(r[k])[at], _u(short[k])[o13:o13 + c]
                same = (got == want).all(axis=1)
                assert same.all(), '%s %s: window %d of %d is not entry %d of the 13-entry call' % (what, k, j + K * int(np.flatnonzero(~same)[0]), n, j)


def _window(r, q):
    a, b = int(r['offset'][q]), int(r['offset'][q + 1])
    return {k: r[k][a:b] for k in ('m', 'contrib', 'L', 'blin')}


# ------------------------------------------------------------------------------------------------ the 13 against the host
def _host_surfaces(sc, R, T, ns):
    worst = 0.0
    for j in range(K):
        Th, nh = surfaces.host_surface(sc.gen, sc.rows, R, sc.As, sc.tg[j], sc.lo[j], sc.hi[j], _zcut())
        assert np.array_equal(ns[j], nh) and np.array_equal(np.isnan(T[j]), np.isnan(Th)), j
        if (nh > 0).any():
            tol = ic.tolerance(Th)
            err = float(np.nanmax(np.abs(T[j] - Th)))
            assert err <= tol, (j, err, tol)
            worst = max(worst, err / tol)
    assert ns[sc.kinds['empty']].max() == 0 and (ns.max(axis=1) > 0).sum() == K - 1
    return worst


def _host_influence(sc, R, r, B, host=None):
    """test_gpu_influence.py's comparison of one call over the scene's windows; returns (worst ratio, lin_b compared, blocks)."""
    worst, compared, blocks = 0.0, 0, 0
    for q in range(len(r['T_max'])):
        if host is not None and host[q] is not None:
            h = host[q]
        else:
            h = influence.host_influence(sc.gen, sc.rows, R, sc.As, sc.tg[q], sc.lo[q], sc.hi[q], _zcut(), min(B, len(sc.gen)))
        d = _window(r, q)
        tol = ic.tolerance(h['T'])
        assert np.array_equal(d['m'], h['m']) and (len(h['m']) == 0 or r['first_block'][q] == h['first_block']), q
        assert r['ns_min'][q] == h['ns_min'] == d['m'].sum()
        assert r['lin'][q] == h['lin'] or abs(r['T_max'][q] - h['T_max']) <= tol
        errs = [abs(r['T_max'][q] - h['T_max'])]
        if len(h['m']):
            errs.append(np.max(np.abs(d['L'] - h['L'])))
            if h['lin'] >= 0 and r['lin'][q] == h['lin']:
                errs.append(np.max(np.abs(d['contrib'] - h['contrib'])))
            else:
                assert h['lin'] >= 0 or np.isnan(d['contrib']).all()
            sure = h['margin'] > 2 * tol
            assert np.array_equal(d['blin'][sure], h['blin'][sure]), (B, q)
            compared += int(sure.sum())
            blocks += len(sure)
        err = float(max(errs))
        worst = max(worst, err / tol if tol else 0.0)
        assert err <= tol, (B, q, err, tol)
    assert blocks > 0 and compared >= 0.99 * blocks, (compared, blocks)
    return worst, compared, blocks


def _margin(T):
    v, l, second = influence.scan_argmax(T)
    return v - second if l >= 0 else float(-np.nanmax(np.where(np.isnan(T), -np.inf, T), initial=-np.inf))


def _host_cond(sc, R, res, ct, cl):
    worst, most = 0.0, 0
    for j in range(K):
        c, l = int(ct[j]), int(cl[j])
        if c < 0 or l < 0:
            Th, nh, sh, S = conditional.host_cond_surface(sc.gen, sc.rows, R, sc.As, sc.tg[j], sc.lo[j], sc.hi[j], None, 0, -1, 0.0, 0, 0, _zcut(),
                                                          scale=True)
        else:
            iA, ix, ia = sc.decode(l)
            Th, nh, sh, S = conditional.host_cond_surface(sc.gen, sc.rows, R, sc.As, sc.tg[j], sc.lo[j], sc.hi[j], sc.tg[c], sc.lo[c], sc.hi[c],
                                                          sc.As[iA], ix, ia, _zcut(), scale=True)
        assert np.array_equal(res['nsites'][j], nh) and np.array_equal(res['nshared'][j], sh), (j, res['nshared'][j], sh)
        assert np.array_equal(np.isnan(res['T'][j]), np.isnan(Th)), j
        most = max(most, int(sh.max()))
        tol = cc.REL_TOL * float(S.max())
        hv, hl, _ = influence.scan_argmax(Th)
        if (nh > 0).any():
            err = float(np.nanmax(np.abs(res['T'][j] - Th)))
            assert err <= tol, (j, err, tol)
            worst = max(worst, err / tol)
        assert abs(res['tmax'][j] - hv) <= tol and (res['lin'][j] == hl or not _margin(Th) > 2 * tol), j
        # tmax and lin are the scan's rule on the device's own T, exactly
        v, l2, _ = influence.scan_argmax(res['T'][j])
        assert np.float64(res['tmax'][j]).tobytes() == np.float64(v).tobytes() and res['lin'][j] == l2, j
    assert most > 0
    return worst


def _host_fit(sc, R, got, lins, gw, cls, F, edges):
    O, Es, En, sk = got
    worst, m = 0.0, sc.model
    for j in range(K):
        if lins[j] < 0:
            assert not O[j].any() and np.isnan(Es[j]).all() and np.isnan(En[j]).all() and sk[j] == 0
            continue
        iA, ix, ia = sc.decode(int(lins[j]))
        hO, hEs, hEn, hsk = fit.host_fit(sc.gen, sc.rows, m.row_off, R, gw, cls, F, edges, sc.As[iA], ix, ia, sc.tg[j], sc.lo[j], sc.hi[j], _zcut())
        assert np.array_equal(O[j], hO) and sk[j] == hsk, j
        bound = fc.TOL * np.maximum(1, hO.sum(axis=1))[:, None]
        es, en = np.abs(Es[j] - hEs) / bound, np.abs(En[j] - hEn) / bound
        assert es.max() <= 1.0 and en.max() <= 1.0, (j, es.max(), en.max())
        worst = max(worst, float(es.max()), float(en.max()))
    assert sum(int(o.sum()) > 0 for o in O) >= K - 3
    return worst


# ------------------------------------------------------------------------------------------------ the 13-entry calls, once each
@functools.lru_cache(maxsize=None)
def _short_surfaces(scene):
    sc, (ctx, R) = cs.scene(scene), _ctx(scene)
    T, ns = ctx.surfaces(cs.rotation(K))
    print('%s: the 13 surfaces against host_surface, worst error %.3g of the tolerance' % (scene, _host_surfaces(sc, R, T, ns)))
    return T, ns


@functools.lru_cache(maxsize=None)
def _short_influence(scene, block):
    sc, (ctx, R) = cs.scene(scene), _ctx(scene)
    r = ctx.influence(cs.rotation(K), block)
    print('%s, block %d: the 13 against host_influence, worst error %.3g of the tolerance, lin_b compared on %d of %d blocks'
          % ((scene, block) + _host_influence(sc, R, r, block)))
    T, ns = _short_surfaces(scene)
    for j in range(K):                                   # the exact relation to the surfaces
        v, l, _ = influence.scan_argmax(T[j])
        assert r['lin'][j] == l and np.float64(r['T_max'][j]).tobytes() == np.float64(v).tobytes() and r['ns_min'][j] == ns[j, int(np.argmin(sc.As))]
    return r


@functools.lru_cache(maxsize=None)
def _short_cond(scene):
    sc, (ctx, R) = cs.scene(scene), _ctx(scene)
    ct, cl = cs.cond_partners(sc.points)
    res = ctx.cond_surfaces(cs.rotation(K), ct, cl, want_T=True)
    print('%s: the 13 pairs against host_cond_surface, worst error %.3g of the tolerance' % (scene, _host_cond(sc, R, res, ct, cl)))
    bare = ctx.cond_surfaces(cs.rotation(K), ct, cl, want_T=False)
    assert bare['T'] is None and all(_u(bare[k]).tobytes() == _u(res[k]).tobytes() for k in ('nsites', 'nshared', 'tmax', 'lin'))
    return res


@functools.lru_cache(maxsize=None)
def _short_base(scene):
    """The 13 windows against a baseline of one locus (chunkseams.base_locus), which stays in the scene's slot for the long calls."""
    sc, (ctx, R) = cs.scene(scene), _ctx(scene)
    t, lin = cs.base_locus(sc)
    ctx.baseline_reset()
    assert ctx.baseline_add(t, lin)[2] > 0
    res = ctx.base_surfaces(cs.rotation(K), want_T=True)
    pair = ctx.cond_surfaces(cs.rotation(K), np.full(K, t, np.int32), np.full(K, lin, np.int32), want_T=True)
    assert all(_u(res[k]).tobytes() == _u(pair[k]).tobytes() for k in ('T', 'nsites', 'nshared', 'tmax', 'lin'))
    assert (res['nshared'].max(axis=1) > 0).sum() >= 2 and not (res['nshared'].max(axis=1) > 0).all()
    bare = ctx.base_surfaces(cs.rotation(K), want_T=False)
    assert bare['T'] is None and all(_u(bare[k]).tobytes() == _u(res[k]).tobytes() for k in ('nsites', 'nshared', 'tmax', 'lin'))
    return res


def _fit_call(scene, call, n=None):
    sc, (ctx, R) = cs.scene(scene), _ctx(scene)
    n = call.n if n is None else n
    F, D = call.kw['F'], call.kw['D']
    gw, cls, edges = cs.fit_arrays(sc, F, D, _zcut())
    lins = cs.fit_lins(sc.points)
    ctx.set_variant(call.kw['variant'])
    try:
        got = ctx.fit(cs.rotation(n), cs.along(lins, n), gw, cls, F, edges)
    finally:
        ctx.set_variant(0)
    return got, (lins, gw, cls, F, edges)


@functools.lru_cache(maxsize=None)
def _short_fit(scene, k):
    sc, (ctx, R) = cs.scene(scene), _ctx(scene)
    call = _case(scene)[1][k]
    got, args = _fit_call(scene, call, K)
    print('%s, F %d, D %d, variant %d: the 13 against host_fit, worst error %.3g of the bound'
          % (scene, call.kw['F'], call.kw['D'], call.kw['variant'], _host_fit(sc, R, got, *args)))
    return got


def _timed(what, t0):
    print('%s: %.2f s' % (what, time.perf_counter() - t0))


# ------------------------------------------------------------------------------------------------ rules 1 and 2
def _surfaces_seam(name, scene):
    sc, calls = _case(name)
    call = [c for c in calls if c.op == 'surfaces'][0]
    assert len(call.cuts['windows']) >= 2
    ctx, R = _ctx(scene)
    T13, ns13 = _short_surfaces(scene)
    t0 = time.perf_counter()
    T, ns = ctx.surfaces(cs.rotation(call.n))
    _timed('%s: surfaces of %d windows in chunks of %s (kernels %.1f ms)' % (name, call.n, call.cuts['windows'], ctx.surfaces_ms()), t0)
    _rot_equal(T, T13, name + ' surfaces T')
    _rot_equal(ns, ns13, name + ' surfaces nsites')


def _cond_seam(name, scene, want_T):
    sc, calls = _case(name)
    call = [c for c in calls if c.op == 'cond' and c.kw['want_T'] == want_T][0]
    assert len(call.cuts['windows']) >= (2 if want_T else 3)
    ctx, R = _ctx(scene)
    short = _short_cond(scene)
    ct, cl = cs.cond_partners(sc.points)
    t0 = time.perf_counter()
    res = ctx.cond_surfaces(cs.rotation(call.n), cs.along(ct, call.n), cs.along(cl, call.n), want_T=want_T)
    _timed('%s: cond_surfaces of %d pairs in chunks of %s, T %s (kernels %.1f ms)'
           % (name, call.n, call.cuts['windows'], 'copied back' if want_T else 'left on the device', ctx.cond_surfaces_ms()), t0)
    for k in ('T', 'nsites', 'nshared', 'tmax', 'lin') if want_T else ('nsites', 'nshared', 'tmax', 'lin'):
        _rot_equal(res[k], short[k], '%s cond_surfaces %s' % (name, k))
    assert want_T or res['T'] is None


def _base_seam(name, scene, want_T):
    sc, calls = _case(name)
    call = [c for c in calls if c.op == 'base' and c.kw['want_T'] == want_T][0]
    assert len(call.cuts['windows']) >= (2 if want_T else 3)
    ctx, R = _ctx(scene)
    short = _short_base(scene)
    t0 = time.perf_counter()
    res = ctx.base_surfaces(cs.rotation(call.n), want_T=want_T)
    _timed('%s: base_surfaces of %d windows in chunks of %s, T %s (kernels %.1f ms)'
           % (name, call.n, call.cuts['windows'], 'copied back' if want_T else 'left on the device', ctx.base_surfaces_ms()), t0)
    for k in ('T', 'nsites', 'nshared', 'tmax', 'lin') if want_T else ('nsites', 'nshared', 'tmax', 'lin'):
        _rot_equal(res[k], short[k], '%s base_surfaces %s' % (name, k))
    assert want_T or res['T'] is None


def _influence_seam(name, scene, block, chunks=2):
    sc, calls = _case(name)
    call = [c for c in calls if c.op == 'influence' and c.kw['block'] == block][0]
    assert len(call.cuts['windows']) >= chunks
    ctx, R = _ctx(scene)
    short = _short_influence(scene, block)
    t0 = time.perf_counter()
    r = ctx.influence(cs.rotation(call.n), block)
    _timed('%s: influence of %d windows, block %d, %d blocks, range pass %s, window chunks %s (kernels %.1f ms)'
           % (name, call.n, block, r['offset'][-1], call.cuts['range'], call.cuts['windows'], ctx.influence_ms()), t0)
    _infl_rot_equal(r, short, '%s influence, block %d' % (name, block))
    return r


def test_bytes_seam_surfaces():
    _surfaces_seam('bytes', 'bytes')


@pytest.mark.parametrize('block', [10 ** 6, 3])
def test_bytes_seam_influence(block):
    _influence_seam('bytes', 'bytes', block)


def test_bytes_seam_cond_surfaces():
    _cond_seam('bytes', 'bytes', True)


def test_bytes_seam_cond_surfaces_three_chunks_without_T():
    _cond_seam('bytes', 'bytes', False)


def test_bytes_seam_base_surfaces():
    _base_seam('bytes', 'bytes', True)


def test_bytes_seam_base_surfaces_three_chunks_without_T():
    _base_seam('bytes', 'bytes', False)


def test_threads_seam_surfaces():
    _surfaces_seam('threads', 'one_pair')


def test_threads_seam_cond_surfaces():
    _cond_seam('threads', 'one_pair', True)


# ------------------------------------------------------------------------------------------------ rules 3 and 4
def test_range_pass_seam():
    """The range pass cuts at 2^20 windows, the window chunks at 1 048 575: one window apart."""
    r = _influence_seam('range', 'one_pair', 10 ** 6)
    assert np.diff(r['offset']).max() == 1


def test_block_seam_many_windows():
    sc, calls = _case('blocks')
    r = _influence_seam('blocks', 'blocks', 1)
    first = calls[0].cuts['windows'][0]
    assert r['offset'][first] <= cs.INFL_CHUNK_BLOCKS < r['offset'][first + 1]          # the device's own counts cut where restated


def test_block_seam_one_window():
    sc, calls = _case('one_window')
    assert calls[0].cuts['windows'] == [1, 1, 1]
    ctx, R = _ctx('one_window')
    t0 = time.perf_counter()
    r = ctx.influence([0, 1, 2], 1)
    _timed('one_window: influence of [short, %d sites, short], block 1 (kernels %.1f ms)' % (len(sc.gen), ctx.influence_ms()), t0)
    assert np.diff(r['offset']).tolist() == [8, len(sc.gen), 8] and len(sc.gen) > cs.INFL_CHUNK_BLOCKS
    long = cs.host_influence_one_point(sc.gen, sc.rows, R[0, 0], sc.As[0], sc.tg[1], sc.lo[1], sc.hi[1], _zcut(), 1)
    assert long['lin'] == 0 and (long['m'] == 0).sum() == 2
    worst, compared, blocks = _host_influence(sc, R, r, 1, host=[None, long, None])
    print('one_window: worst error %.3g of the tolerance %.3g, lin_b compared on %d of %d blocks' % (worst, ic.tolerance(long['T']), compared, blocks))
    # the long window alone, and the two short ones without it: the same bytes
    alone, pair = ctx.influence([1], 1), ctx.influence([0, 2], 1)
    for k in ('T_max', 'lin', 'ns_min', 'first_block'):
        assert _u(r[k]).tobytes() == _u(np.concatenate([pair[k][:1], alone[k], pair[k][1:]])).tobytes(), k
    for k in ('m', 'contrib', 'L', 'blin'):
        assert _u(r[k]).tobytes() == _u(np.concatenate([pair[k][:8], alone[k], pair[k][8:]])).tobytes(), k


# ------------------------------------------------------------------------------------------------ rules 5 and 6
def _fit_seam(name, k=0):
    sc, calls = _case(name)
    call = calls[k]
    assert len(call.cuts['windows']) >= 2
    short = _short_fit(name, k)
    ctx, R = _ctx(name)
    t0 = time.perf_counter()
    got, _ = _fit_call(name, call)
    _timed('%s: fit of %d windows, F %d, D %d, in chunks of %s (kernels %.1f ms)'
           % (name, call.n, call.kw['F'], call.kw['D'], call.cuts['windows'], ctx.fit_ms()), t0)
    for a, b, what in zip(got, short, ('O', 'E_sel', 'E_neu', 'skipped')):
        _rot_equal(a, b, '%s fit %s' % (name, what))


def test_fit_outputs_seam():
    _fit_seam('fit_out')


def test_fit_workspace_seam():
    """The sums of 221 sample sizes x 11 do not fit LDS: the shipped workspace home, cut by the workspace rule."""
    sc, calls = _case('fit_ws')
    assert not cs.fit_step(len(sc.model.sizes), 10, 25)[3]
    _fit_seam('fit_ws')


def test_fit_the_two_homes_agree_bit_for_bit():
    """The same 13 entries with F = 6, where the sums fit LDS: from LDS and, with set_variant(1), from the workspace."""
    sc, calls = _case('fit_ws')
    assert cs.fit_step(len(sc.model.sizes), 6, 25)[3] and not cs.fit_step(len(sc.model.sizes), 6, 25, 1)[3]
    lds, ws = _short_fit('fit_ws', 1), _short_fit('fit_ws', 2)
    for a, b, what in zip(lds, ws, ('O', 'E_sel', 'E_neu', 'skipped')):
        assert _u(a).tobytes() == _u(b).tobytes(), what
