"""Conditional surfaces on the GPU (--conditional): bmx_ctx_cond_surfaces against bmx_ctx_surfaces -- bit for bit where no site is
shared, that is the contract -- and against the host restatement (ballermixplus_amd/conditional.py) with real conditioning loci, on
the example inputs, the ragged chromosome and one built around the tile and reach edges; that a pair's numbers depend on that pair
alone, what the call leaves untouched, its errors, and the CLI end to end."""
import ctypes as C
import os

import numpy as np
import pytest

import cases
import condcases as cc
from test_gpu_refine import _case_ctx, _cli, _engine, _read
from test_gpu_surfaces import EX1, EX2, _same_bits

from ballermixplus_amd import _lib, conditional, influence, peaks, surfaces
from ballermixplus_amd._lib import BmxError

pytestmark = pytest.mark.gpu

MAX_PAIRS = {'ex1_B2': 2, 'ex1_B2_fixX_fixAlpha_listA': 7, 'ex1_B2_w50_s25': 4, 'ragged': 22}     # the host restatement of a pair
#                                                                 of ex1_B2 (31 A x 510 grid pairs x 756 sites) takes two seconds


def _numpy_argmax(T):
    """(tmax f64[n], lin i32[n]) of T[n][...] by the scan's rule in numpy."""
    best = [influence.scan_argmax(t)[:2] for t in T]
    return np.array([b[0] for b in best], dtype=np.float64), np.array([b[1] for b in best], dtype=np.int32)


def _with_empty_window(cat):
    """The case's test sites and one more at the last position whose window is empty: a conditioning locus out of every site's
    reach by its window, whatever the grid.  Returns (tg, lo, hi, its index)."""
    tg, lo, hi = np.append(cat.tg, cat.tg[-1]), np.append(cat.lo, 1), np.append(cat.hi, 0)
    return tg, lo.astype(np.int64), hi.astype(np.int64), len(cat.tg)


def _scan_lin(ctx, name, M):
    """The grid point every test site is held at when it conditions: its scan argmax on the examples; on the synthetic
    chromosomes (windows the scan's own tests do not cover) the scan's rule on its plain-sum surface."""
    if name.startswith('ex'):
        ctx.scan()
        clr, ix, ia, iA, _ = ctx.fetch()
        nx, nab = len(ctx.model.x), len(ctx.model.abeta)
        lin = np.where(iA >= 0, (iA.astype(np.int64) * nx + ix) * nab + ia, -1).astype(np.int32)[:M]
        if (lin < 0).all():                     # the one-pair example: no window has a T > 0, so the scan names no grid point;
            T, _ = ctx.surfaces(np.arange(M, dtype=np.int32))       # the locus is held where its plain-sum surface is highest
            lin = np.argmax(np.where(np.isnan(T), -np.inf, T).reshape(M, -1), axis=1).astype(np.int32)
        return lin
    every = np.arange(M, dtype=np.int32)
    none = np.full(M, -1, dtype=np.int32)
    return ctx.cond_surfaces(every, none, none, want_T=False)['lin']


# ------------------------------------------------------------------------------------------------------ bitwise anchors

@pytest.mark.parametrize('name', cc.NAMES)
def test_without_a_shared_site_it_is_the_surface_bit_for_bit(name):
    eng = _engine()
    cat = cc.catalogue(eng)[name]()
    if name == 'ex1_B2':                        # two slices, the second partial
        assert len(cat.xs) * len(cat.ab) == 510
    if name == 'ex1_B2_fixX_fixAlpha_listA':    # one pair: a slice with 255 idle threads
        assert len(cat.xs) * len(cat.ab) == 1
    ctx = cat.context(eng)
    tg, lo, hi, E = _with_empty_window(cat)
    ctx.set_tests(tg, lo, hi)
    M = len(cat.tg)
    rng = np.random.default_rng(5)
    tests = np.array(cat.windows + rng.integers(0, M, 12).tolist() + [E], dtype=np.int32)
    n = len(tests)
    T0, n0 = ctx.surfaces(tests)
    tm0, l0 = _numpy_argmax(T0)
    assert (n0 > 0).any() and ((l0 >= 0).any() or name == 'ex1_B2_fixX_fixAlpha_listA')      # (that grid's surfaces are all below 0)
    points = len(cat.As) * len(cat.xs) * len(cat.ab)
    some = rng.integers(0, M, n).astype(np.int32)
    anchors = [('cond_test = -1', np.full(n, -1, np.int32), rng.integers(0, points, n).astype(np.int32)),
               ('cond_lin = -1', some, np.full(n, -1, np.int32)),
               ('both', np.full(n, -1, np.int32), np.full(n, -1, np.int32)),
               ('empty conditioning window', np.full(n, E, np.int32), rng.integers(0, points, n).astype(np.int32))]
    far = cc.unreachable(cat)
    if name != 'ex1_B2_fixX_fixAlpha_listA':    # (its largest A, 1000, reaches across the whole example)
        assert far is not None
        anchors.append(('out of reach by distance', np.full(n, far[0], np.int32), np.full(n, far[1], np.int32)))
    for what, ct, cl in anchors:
        r = ctx.cond_surfaces(tests, ct, cl)
        assert _same_bits(r['T'], T0), (name, what)
        assert np.array_equal(r['nsites'], n0) and not r['nshared'].any(), (name, what)
        assert _same_bits(r['tmax'], tm0) and np.array_equal(r['lin'], l0), (name, what)
        assert r['T'].dtype == np.float64 and r['nsites'].dtype == r['nshared'].dtype == r['lin'].dtype == np.int32
    print('%s: %d windows, kernels %.3f ms (surfaces %.3f ms)' % (name, n, ctx.cond_surfaces_ms(), ctx.surfaces_ms()))
    ctx.close()


# ---------------------------------------------------------------------------------------------- against the restatement

def _compare(cat, R, res, pairs, lins, what):
    """Every pair of one call against host_cond_surface on the device's table: NaN pattern, nsites and nshared exact, max |dT| <=
    REL_TOL * max over the grid of 2 sum_i |term_i| (the host's).  Returns (the worst ratio, the largest nshared)."""
    worst, most = 0.0, 0
    for q, ((t, c), l) in enumerate(zip(pairs, lins)):
        Th, nh, sh, S = cc.host_pair(cat, R, t, c, int(l), scale=True, zc=float(_lib.lib().bmx_alpha_cut()))
        assert np.array_equal(res['nsites'][q], nh), (what, q, t, c, res['nsites'][q], nh)
        assert np.array_equal(res['nshared'][q], sh), (what, q, t, c, res['nshared'][q], sh)
        assert np.array_equal(np.isnan(res['T'][q]), np.isnan(Th)), (what, q)
        assert np.array_equal(np.isnan(Th).all(axis=(1, 2)), nh == 0)
        most = max(most, int(sh.max()))
        if (nh > 0).any():
            err, scale = float(np.nanmax(np.abs(res['T'][q] - Th))), float(S.max())
            ratio = err / (cc.REL_TOL * scale)
            print('%s pair %d (%d | %d @ %d): nsites %s, nshared %s, max |dT| %.3g, scale %.3g, ratio %.3g'
                  % (what, q, t, c, l, nh.tolist(), sh.tolist(), err, scale, ratio))
            assert err <= cc.REL_TOL * scale, (what, q, err, scale)
            worst = max(worst, ratio)
    return worst, most


@pytest.mark.parametrize('name', cc.NAMES)
def test_against_the_host_restatement_with_real_conditioning_loci(name):
    eng = _engine()
    cat = cc.catalogue(eng)[name]()
    ctx = cat.context(eng)
    M = len(cat.tg)
    lin = _scan_lin(ctx, name, M)
    assert (lin >= 0).any()
    pairs = cc.neighbours(cat)[:MAX_PAIRS[name]]
    lins = [int(lin[c]) for _, c in pairs]
    res = ctx.cond_surfaces([t for t, _ in pairs], [c for _, c in pairs], lins)
    T0, _ = ctx.surfaces([t for t, _ in pairs])
    _, R = ctx.fetch_lut()
    worst, most = _compare(cat, R, res, pairs, lins, name)
    assert most > 0 and not _same_bits(res['T'], T0)          # the loci are real: sites are shared and the surfaces move
    tm, l = _numpy_argmax(res['T'])
    assert _same_bits(res['tmax'], tm) and np.array_equal(res['lin'], l)
    print('%s: %d pairs, worst |dT| / tolerance %.3g' % (name, len(pairs), worst))
    ctx.close()


# ------------------------------------------------------------------------------------------------- tile and reach edges

def test_tile_and_reach_edges():
    eng = _engine()
    cat = cc.edges(eng)
    ctx = cat.context(eng)
    zcut = float(_lib.lib().bmx_alpha_cut())
    assert zcut == cc.zcut()
    counts = list(cc.COUNTS) + [702]            # the sites of test site 0 (off-site 1.0, the whole chromosome) at every A of the grid
    npairs = len(cat.xs) * len(cat.ab)
    nA = len(cat.As)
    assert nA == 8
    none = ctx.cond_surfaces([0], [-1], [-1])
    assert none['nsites'][0].tolist() == counts
    # 1. the candidate holds 0, 1, 255, 256, 257, 512, 513 sites (one per A); the conditioning locus at the same position holds
    #    exactly counts[k] of them at grid A number k, the boundary one ulp tight: the shared sites are the smaller of the two
    pairs = [(0, 1)] * nA
    lins = [k * npairs + (37 * k + 3) % npairs for k in range(nA)]
    # 2. a conditioning window (test site 2: [300, 420]) that cuts its reach inside a tile
    pairs += [(0, 2)] * 3
    lins += [3 * npairs + 7, 6 * npairs + 100, 7 * npairs + 509]
    # 3. a conditioning position equal to a site's (test site 3): that site is never shared; and the triple's position
    pairs += [(0, 3)] * 3 + [(0, 4), (4, 0), (3, 4)]
    lins += [1 * npairs + 5, 4 * npairs + 250, 7 * npairs + 1, 5 * npairs + 77, 2 * npairs + 300, 6 * npairs + 11]
    # 4. a conditioning locus far out (test site 5): in reach at the smallest A alone; and the far candidate itself
    pairs += [(0, 5), (0, 5), (5, 0), (5, -1)]
    lins += [7 * npairs + 33, 6 * npairs + 33, 7 * npairs + 2, -1]
    res = ctx.cond_surfaces([t for t, _ in pairs], [c for _, c in pairs], lins)
    for k in range(nA):
        assert res['nsites'][k].tolist() == counts
        assert res['nshared'][k].tolist() == [min(a, counts[k]) for a in counts], (k, res['nshared'][k])
    in_window = [int(((cat.As[a] * np.abs(cat.gen[300:421] - 1.0)) <= zcut).sum()) for a in range(nA)]
    assert res['nshared'][nA + 2].tolist() == [min(a, b) for a, b in zip(counts, in_window)] and 0 < in_window[3] < 256 and in_window[7] == 121
    site = int(np.searchsorted(cat.gen, cat.tg[3]))
    assert cat.gen[site] == cat.tg[3]
    q = nA + 5                                   # (0 | 3) at A = 1: every site of the candidate but the one at the conditioning position
    assert res['nshared'][q].tolist() == [a - (1 if cat.As[i] * abs(cat.gen[site] - 1.0) <= zcut else 0) for i, a in enumerate(counts)]
    assert res['nshared'][q][2:].tolist() == [a - 1 for a in counts[2:]]
    assert res['nshared'][nA + 9].tolist() == counts and not res['nshared'][nA + 10].any()       # far out: all at A = 1, none at the next
    _, R = ctx.fetch_lut()
    worst, most = _compare(cat, R, res, pairs, lins, 'edges')
    assert most == 702
    # the far candidate alone has one A with sites and nothing > 0 there: (0, -1), its T finite
    assert np.isfinite(res['T'][-1][7]).all() and (res['T'][-1][7] <= 0).all() and res['tmax'][-1] == 0.0 and res['lin'][-1] == -1
    tm, l = _numpy_argmax(res['T'])
    assert _same_bits(res['tmax'], tm) and np.array_equal(res['lin'], l)
    print('edges: %d pairs, worst |dT| / tolerance %.3g' % (len(pairs), worst))
    ctx.close()


# --------------------------------------------------------------------------------------------------------- independence

def test_a_pair_depends_on_that_pair_alone():
    eng = _engine()
    name = 'ex1_B2'
    cat = cc.catalogue(eng)[name]()
    ctx = cat.context(eng)
    tg, lo, hi, E = _with_empty_window(cat)
    ctx.set_tests(tg, lo, hi)
    M = len(cat.tg)
    lin = _scan_lin(ctx, name, M)
    rng = np.random.default_rng(9)
    t = rng.integers(0, M, 14).astype(np.int32)
    c = np.clip(t + rng.integers(-6, 7, 14), 0, M - 1).astype(np.int32)
    t, c = np.append(t, [E, 5, t[0], t[0]]).astype(np.int32), np.append(c, [3, E, c[0], -1]).astype(np.int32)      # an empty candidate,
    cl = np.where(c >= 0, lin[np.clip(c, 0, M - 1)], -1).astype(np.int32)                    # ... and a repeated pair
    cl[-3] = 17
    full = ctx.cond_surfaces(t, c, cl)
    assert (full['nshared'] > 0).any()
    assert all(_same_bits(full[k][-2], full[k][0]) for k in ('T', 'tmax')) and np.array_equal(full['nshared'][-2], full['nshared'][0])
    for q in (0, 7, len(t) - 4, len(t) - 1):                     # alone
        one = ctx.cond_surfaces(t[q:q + 1], c[q:q + 1], cl[q:q + 1])
        for k in ('T', 'tmax'):
            assert _same_bits(one[k][0], full[k][q]), (k, q)
        for k in ('nsites', 'nshared', 'lin'):
            assert np.array_equal(one[k][0], full[k][q]), (k, q)
    rev = ctx.cond_surfaces(t[::-1], c[::-1], cl[::-1])          # the list reversed
    for k in ('T', 'tmax'):
        assert _same_bits(rev[k][::-1], full[k]), k
    for k in ('nsites', 'nshared', 'lin'):
        assert np.array_equal(rev[k][::-1], full[k]), k
    bare = ctx.cond_surfaces(t, c, cl, want_T=False)             # T_out = NULL
    assert bare['T'] is None and _same_bits(bare['tmax'], full['tmax'])
    for k in ('nsites', 'nshared', 'lin'):
        assert np.array_equal(bare[k], full[k]), k
    tm, l = _numpy_argmax(full['T'])                             # the scan's rule on the returned T, exactly
    assert _same_bits(full['tmax'], tm) and np.array_equal(full['lin'], l)
    q = len(t) - 4                                               # the empty candidate: all NaN, (0, -1)
    assert np.isnan(full['T'][q]).all() and full['tmax'][q] == 0.0 and full['lin'][q] == -1 and not full['nsites'][q].any()
    ctx.close()


def test_all_non_positive_surfaces_have_no_argmax():
    """The one-pair example: every window's plain-sum surface is below 0 at every A of its list (finite, not NaN)."""
    eng = _engine()
    cat = cc.catalogue(eng)['ex1_B2_fixX_fixAlpha_listA']()
    ctx = cat.context(eng)
    M = len(cat.tg)
    every = np.arange(M, dtype=np.int32)
    r = ctx.cond_surfaces(every, np.roll(every, 3), np.full(M, 1, np.int32))
    tm, l = _numpy_argmax(r['T'])
    assert _same_bits(r['tmax'], tm) and np.array_equal(r['lin'], l)
    flat = r['T'].reshape(M, -1)
    dead = np.isfinite(flat).all(axis=1) & (flat <= 0).all(axis=1)
    assert dead.any() and (r['tmax'][dead] == 0.0).all() and (r['lin'][dead] == -1).all()
    ctx.close()


# ----------------------------------------------------------------------------------------------------- state and errors

def _raw(ctx, n, tests, ct, cl, T=None, ns=None, nsh=None, tmax=None, lin=None):
    p = lambda a, f: None if a is None else f(a)
    return ctx._L.bmx_ctx_cond_surfaces(ctx._h, n, p(tests, _lib.as_ip), p(ct, _lib.as_ip), p(cl, _lib.as_ip), p(T, _lib.as_dp),
                                        p(ns, _lib.as_ip), p(nsh, _lib.as_ip), p(tmax, _lib.as_dp), p(lin, _lib.as_ip))


def test_state_and_errors():
    INVALID, STATE = -1, -5
    opt, case, ts, sel = _case_ctx(cases.ALL_CASES['ex1_B2'][0])
    ctx = sel.ctx
    M = len(ts)
    L = ctx._L
    one = np.zeros(1, dtype=np.int32)
    ms = C.c_double()
    assert _raw(ctx, 1, one, one, one) == STATE                  # model and sites, no test sites yet
    assert L.bmx_ctx_cond_surfaces_ms(ctx._h, C.byref(ms)) == STATE
    with pytest.raises(BmxError) as e:
        ctx.cond_surfaces([0], [1], [0])
    assert e.value.code == STATE
    ctx.set_tests(ts.test_gen, ts.lo, ts.hi)
    assert L.bmx_ctx_cond_surfaces_ms(ctx._h, C.byref(ms)) == STATE      # no call yet
    ctx.scan()
    before = ctx.fetch()
    pk = ctx.peaks(0.0002, 5.0)
    T0, n0 = ctx.surfaces([3, M - 1])
    nx, nab = len(sel.model.x), len(sel.model.abeta)
    points = ctx.nA * nx * nab
    lin = np.where(before[3] >= 0, (before[3].astype(np.int64) * nx + before[1]) * nab + before[2], -1).astype(np.int32)
    apex = pk['row']
    assert len(apex) >= 2
    r = ctx.cond_surfaces(apex, np.roll(apex, 1), lin[np.roll(apex, 1)])
    assert r['nshared'].any() and ctx.cond_surfaces_ms() > 0
    after = ctx.fetch()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    pk2 = ctx.fetch_peaks()
    assert all(np.array_equal(pk[f], pk2[f]) for f in peaks.FIELDS)
    T1, n1 = ctx.surfaces([3, M - 1])
    assert _same_bits(T1, T0) and np.array_equal(n1, n0)
    # the errors, each with its code; a refused call writes nothing
    ok = np.array([3, 4], dtype=np.int32)
    T = np.full((2, points), 7.0)
    outs = dict(ns=np.full((2, ctx.nA), 7, np.int32), nsh=np.full((2, ctx.nA), 7, np.int32), tmax=np.full(2, 7.0), lin=np.full(2, 7, np.int32))
    bad = [(None, 2, ok, ok, ok), (ctx, -1, ok, ok, ok), (ctx, 2, None, ok, ok), (ctx, 2, ok, None, ok), (ctx, 2, ok, ok, None),
           (ctx, 2, np.array([3, -1], np.int32), ok, ok), (ctx, 2, np.array([M, 3], np.int32), ok, ok),
           (ctx, 2, ok, np.array([3, -2], np.int32), ok), (ctx, 2, ok, np.array([M, 3], np.int32), ok),
           (ctx, 2, ok, ok, np.array([0, points], np.int32))]
    for who, n, a, b, c in bad:
        if who is None:
            rc = L.bmx_ctx_cond_surfaces(None, n, _lib.as_ip(a), _lib.as_ip(b), _lib.as_ip(c), _lib.as_dp(T), None, None, None, None)
        else:
            rc = _raw(ctx, n, a, b, c, T, **outs)
        assert rc == INVALID, (n, a, b, c, rc)
        assert (T == 7.0).all() and all((v == 7).all() for v in outs.values())
    assert L.bmx_ctx_cond_surfaces_ms(None, C.byref(ms)) == INVALID and L.bmx_ctx_cond_surfaces_ms(ctx._h, None) == INVALID
    with pytest.raises(BmxError) as e:
        ctx.cond_surfaces([0, M], [1, 1], [0, 0])
    assert e.value.code == INVALID and 'index' in str(e.value)
    # the edges of what is allowed: cond_test = -1, cond_lin = the last grid point and any negative value; n == 0; every output NULL
    assert _raw(ctx, 2, ok, np.array([-1, M - 1], np.int32), np.array([points - 1, -9], np.int32), T, **outs) == 0
    assert not (T == 7.0).any() and not (outs['nsh'] == 7).any()
    assert _raw(ctx, 0, None, None, None) == 0 and _raw(ctx, 2, ok, ok, ok) == 0
    e0 = ctx.cond_surfaces([], [], [])
    assert e0['T'].shape == (0, ctx.nA, nx, nab) and e0['nshared'].shape == (0, ctx.nA) and e0['tmax'].shape == (0,)
    assert all(np.array_equal(a, b) for a, b in zip(before, ctx.fetch()))
    # a second slot: the call reads the selected one
    ctx.select_slot(1)
    with pytest.raises(BmxError) as e:
        ctx.cond_surfaces([0], [0], [0])
    assert e.value.code == STATE
    ctx.select_slot(0)
    again = ctx.cond_surfaces(apex, np.roll(apex, 1), lin[np.roll(apex, 1)])
    assert _same_bits(again['T'], r['T']) and np.array_equal(again['nshared'], r['nshared'])
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ CLI

def _rows(path):
    names, rows = conditional.read_table(path)
    assert '\t'.join(names) + '\n' == conditional.HEADER
    return rows


def _recompute(ts, sel, G, peak_min, span=None):
    """The scan, the peak call, the parents and the pairs of one file again, through Context.cond_surfaces."""
    ctx = sel.ctx
    ctx.set_tests(ts.test_gen, ts.lo, ts.hi)
    ctx.scan()
    clr, ix, ia, iA, _ = ctx.fetch()
    nx, nab = len(sel.model.x), len(sel.model.abeta)
    lin = np.where(iA >= 0, (iA.astype(np.int64) * nx + ix) * nab + ia, -1)
    apex = ctx.peaks(G, peak_min)['row'].astype(np.int64)
    zcut = float(_lib.lib().bmx_alpha_cut())
    par = conditional.parents(ts.test_gen, clr, iA, np.array([float(v) for v in sel.grid_A]), apex, zcut, span)
    return clr, lin, iA, apex, par


def _check_rows(rows, apex_rows_of_file, ctx, sel, clr, lin, iA, apex, par, keep):
    nx, nab = len(sel.model.x), len(sel.model.abeta)
    assert [r[:3] for r in rows] == [apex_rows_of_file[k][:3] for k in keep]
    num = lambda v: 'NA' if v is None else (repr(float(v)) if isinstance(v, float) else str(int(v)))
    with_parent = 0
    for r, k in zip(rows, keep):
        j, q = int(apex[k]), int(par[k])
        if q < 0:
            one = ctx.cond_surfaces([j], [-1], [-1])
            assert r[3] == repr(float(one['tmax'][0])) and r[4:] == ['NA'] * 12
            continue
        with_parent += 1
        p = int(apex[q])
        res = ctx.cond_surfaces([j, j, p, p], [-1, p, j, -1], [-1, int(lin[p]), int(lin[j]), -1])
        tm, l = _numpy_argmax(res['T'])
        assert r[3] == repr(float(tm[0])) and r[4:7] == apex_rows_of_file[q][:3]
        assert r[7] == str(int(res['nshared'][1][int(iA[j])]))
        assert r[8] == repr(float(tm[1]))
        assert r[9:12] == list(influence.grid_strings(int(l[1]), sel))
        assert r[12] == (str(int(res['nsites'][1][int(l[1]) // (nx * nab)])) if l[1] >= 0 else 'NA')
        assert r[13] == num(float(tm[1]) / float(tm[0]) if tm[0] > 0 else None)
        assert r[14] == repr(float(tm[2])) and r[15] == num(float(tm[2]) / float(tm[3]) if tm[3] > 0 else None)
    return with_parent


def test_cli_conditional_of_the_apexes(tmp_path):
    plain, cd = str(tmp_path / 'plain.txt'), str(tmp_path / 'cd.txt')
    flags = ['--peaks', '0.00005', '--peakMin', '5']            # (Example 1 spans 0.001 in genPos: five apexes)
    _cli(EX1 + ['-o', plain] + flags)
    r = _cli(EX1 + ['-o', cd] + flags + ['--conditional', '--condSurfaces'])
    assert sorted(os.listdir(tmp_path)) == ['cd.txt', 'cd.txt.conditional.surfaces.txt', 'cd.txt.conditional.txt', 'cd.txt.peaks.txt',
                                            'plain.txt', 'plain.txt.peaks.txt']
    assert _read(plain) == _read(cd) and _read(peaks.output_name(plain)) == _read(peaks.output_name(cd))
    opt, case, ts, sel = _case_ctx(cases.ALL_CASES['ex1_B2'][0])
    ctx = sel.ctx
    clr, lin, iA, apex, par = _recompute(ts, sel, 0.00005, 5.0)
    with open(peaks.output_name(cd)) as f:
        apex_file = [l.rstrip('\n').split('\t') for l in f.readlines()[1:]]
    assert len(apex_file) == len(apex) >= 3
    rows = _rows(conditional.output_name(cd))
    n_par = _check_rows(rows, apex_file, ctx, sel, clr, lin, iA, apex, par, list(range(len(apex))))
    assert n_par == int((par >= 0).sum()) >= 2
    assert 'Conditional: %d apex/es, %d with a parent' % (len(apex), n_par) in r.stdout
    # --condSurfaces: the (j | parent) surfaces, read back, are cond_surfaces' exactly
    layout = surfaces.Layout(sel.grid_A, sel.grid_x, sel.grid_abeta)
    phys, gen, Tf, nf = surfaces.read_surfaces(conditional.surfaces_name(cd), layout)
    kids = [k for k in range(len(apex)) if par[k] >= 0]
    res = ctx.cond_surfaces(apex[kids], apex[par[kids]], lin[apex[par[kids]]])
    assert _same_bits(Tf, layout.ascending(res['T'])) and np.array_equal(nf, res['nsites'][:, layout.oA])
    assert phys == [apex_file[k][0] for k in kids] and gen == [apex_file[k][1] for k in kids]
    ctx.close()


def test_cli_two_files_with_a_floor_and_a_span(tmp_path):
    d1, d2 = tmp_path / 'plain', tmp_path / 'cd'
    ins = EX1[1] + ',' + EX2[1]
    flags = ['-s', '2', '--peaks', '0.00005', '--peakMin', '5']
    _cli(['-i', ins, '--spect', EX1[3], '-o', str(d1)] + flags)
    r = _cli(['-i', ins, '--spect', EX1[3], '-o', str(d2)] + flags + ['--conditional', '--condMin', '35', '--condSpan', '0.0002'])
    outs = sorted(os.listdir(d1))
    assert sorted(f for f in os.listdir(d2) if not f.endswith('.conditional.txt')) == outs
    for f in outs:
        assert _read(d1 / f) == _read(d2 / f), f
    assert r.stdout.count('Conditional: ') == 2
    opt, case, ts, sel = _case_ctx(list(cases.ALL_CASES['ex1_B2'][0]) + ['-s', '2'])
    clr, lin, iA, apex, par = _recompute(ts, sel, 0.00005, 5.0, 0.0002)
    path = str(d2 / (os.path.basename(EX1[1]) + '.out.txt'))
    with open(peaks.output_name(path)) as f:
        apex_file = [l.rstrip('\n').split('\t') for l in f.readlines()[1:]]
    assert len(apex_file) == len(apex)
    keep = [k for k in range(len(apex)) if clr[apex[k]] >= 35.0]
    assert 0 < len(keep) < len(apex)
    assert _check_rows(_rows(conditional.output_name(path)), apex_file, sel.ctx, sel, clr, lin, iA, apex, par, keep) >= 1
    sel.ctx.close()
    # the second file: one row per apex at or above the floor
    path2 = str(d2 / (os.path.basename(EX2[1]) + '.out.txt'))
    with open(peaks.output_name(path2)) as f:
        apex2 = [l.rstrip('\n').split('\t') for l in f.readlines()[1:]]
    assert [r[:3] for r in _rows(conditional.output_name(path2))] == [a[:3] for a in apex2 if float(a[2]) >= 35.0]
