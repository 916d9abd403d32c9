"""Forward stepwise selection on the GPU (--stepwise): bmx_ctx_baseline_reset / _add / _fetch and bmx_ctx_base_surfaces against
bmx_ctx_surfaces (empty baseline) and bmx_ctx_cond_surfaces (one locus) -- bit for bit, that is the contract -- and against the host
restatement (ballermixplus_amd/stepwise.py) after two and three loci; the identity on the fetched baseline; the greedy run against
the host's on the cases whose margins test_stepwise_cpu.py checked; that a window's numbers depend on that window and the baseline
alone, across a chunk seam too; what the calls leave untouched, their refusals, and the CLI end to end.

The tests print the worst |dT| and |dd| they see as shares of their tolerances; the README quotes them."""
import ctypes as C
import os

import numpy as np
import pytest

import cases
import chunkseams as cs
import condcases as cc
import stepcases as sc
from test_gpu_refine import _case_ctx, _cli, _engine, _read
from test_gpu_surfaces import EX1, _same_bits

from ballermixplus_amd import _lib, influence, peaks, stepwise, surfaces
from ballermixplus_amd._lib import BmxError

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -5
FLOATS, INTS = ('T', 'tmax'), ('nsites', 'nshared', 'lin')


def _zc():
    return float(_lib.lib().bmx_alpha_cut())


def _numpy_argmax(T):
    best = [influence.scan_argmax(t)[:2] for t in T]
    return np.array([b[0] for b in best], dtype=np.float64), np.array([b[1] for b in best], dtype=np.int32)


def _same(a, b, what=''):
    for k in FLOATS:
        assert _same_bits(a[k], b[k]), (what, k)
    for k in INTS:
        assert np.array_equal(a[k], b[k]), (what, k)


# ------------------------------------------------------------------------------------------------------ bitwise anchors

@pytest.mark.parametrize('name', cc.NAMES)
def test_against_the_empty_baseline_it_is_the_surface_bit_for_bit(name):
    eng = _engine()
    cat = cc.catalogue(eng)[name]()
    ctx = cat.context(eng)
    tg, lo, hi = np.append(cat.tg, cat.tg[-1]), np.append(cat.lo, 1).astype(np.int64), np.append(cat.hi, 0).astype(np.int64)
    ctx.set_tests(tg, lo, hi)                       # one more test site at the last position whose window is empty
    M = len(cat.tg)
    rng = np.random.default_rng(5)
    tests = np.array(cat.windows + rng.integers(0, M, 12).tolist() + [M], dtype=np.int32)
    T0, n0 = ctx.surfaces(tests)
    tm0, l0 = _numpy_argmax(T0)
    assert (n0 > 0).any()
    ctx.baseline_reset()
    d, cnt = ctx.baseline_fetch()
    assert d.shape == cnt.shape == (len(cat.gen),) and not d.any() and not cnt.any() and cnt.dtype == np.int32
    r = ctx.base_surfaces(tests)
    assert _same_bits(r['T'], T0) and np.array_equal(r['nsites'], n0) and not r['nshared'].any()
    assert _same_bits(r['tmax'], tm0) and np.array_equal(r['lin'], l0)
    assert r['T'].dtype == np.float64 and r['nsites'].dtype == r['nshared'].dtype == r['lin'].dtype == np.int32
    bare = ctx.base_surfaces(tests, want_T=False)
    assert bare['T'] is None and _same_bits(bare['tmax'], tm0) and np.array_equal(bare['lin'], l0) and np.array_equal(bare['nsites'], n0)
    print('%s: %d windows, kernels %.3f ms (surfaces %.3f ms)' % (name, len(tests), ctx.base_surfaces_ms(), ctx.surfaces_ms()))
    ctx.close()


def _one_locus(ctx, cat, c, lin, tests, R):
    """Reset, add the locus (c, lin), and hold base_surfaces of `tests` against cond_surfaces of the pairs (t | c at lin) bit for
    bit, the add's three numbers and the fetched baseline against the host's.  Returns the add's (first, last, n)."""
    ctx.baseline_reset()
    w = ctx.baseline_add(c, lin)
    n = len(tests)
    base = ctx.base_surfaces(tests)
    cond = ctx.cond_surfaces(tests, np.full(n, c, np.int32), np.full(n, lin, np.int32))
    _same(base, cond, (c, lin))
    iA, ix, ia = cc.decode(int(lin), len(cat.xs), len(cat.ab))
    dh, ch = np.zeros(len(cat.gen)), np.zeros(len(cat.gen), dtype=np.int32)
    wh = stepwise.host_baseline_add(dh, ch, cat.gen, cat.rows, R, cat.tg[c], cat.lo[c], cat.hi[c], cat.As[iA], ix, ia, _zc())
    d, cnt = ctx.baseline_fetch()
    assert np.array_equal(cnt, ch) and cnt.max(initial=0) <= 1
    if wh[2]:
        assert w == wh, (c, lin, w, wh)
    else:
        assert w[0] > w[1] and w[2] == 0 and not d.any()
    assert np.all(np.abs(d - dh) <= sc.D_TOL * np.abs(dh))          # (one increment per site: |dh| is the sum of its absolute increments)
    return w


def test_after_one_locus_it_is_the_conditional_surface_bit_for_bit_on_the_edges():
    eng = _engine()
    cat = cc.edges(eng)
    ctx = cat.context(eng)
    _, R = ctx.fetch_lut()
    npairs, nA = len(cat.xs) * len(cat.ab), len(cat.As)
    counts = list(cc.COUNTS) + [702]
    every = np.arange(len(cat.tg), dtype=np.int32)
    # the locus at the candidate's position whose reach at grid A number k holds exactly counts[k] sites, one ulp tight
    for k in range(nA):
        w = _one_locus(ctx, cat, 1, k * npairs + (37 * k + 3) % npairs, every, R)
        assert w[2] == counts[k], (k, w)
        assert ctx.base_surfaces([0])['nshared'][0].tolist() == [min(a, counts[k]) for a in counts]
    # a locus whose window ([300, 420]) cuts its reach inside the first tile; a locus at a site's position (that site is not
    # written); the triple's position; a locus far out: in reach of every site at A = 1, of none at the next A: it writes nothing
    in_window = [int(((cat.As[a] * np.abs(cat.gen[300:421] - 1.0)) <= _zc()).sum()) for a in range(nA)]
    for k, lin in ((3, 3 * npairs + 7), (6, 6 * npairs + 100), (7, 7 * npairs + 509)):
        assert _one_locus(ctx, cat, 2, lin, every, R)[2] == in_window[k]
    assert 0 < in_window[3] < 256 and in_window[7] == 121
    site = int(np.searchsorted(cat.gen, cat.tg[3]))
    assert cat.gen[site] == cat.tg[3]
    w = _one_locus(ctx, cat, 3, 7 * npairs + 1, every, R)
    assert w[2] == 701 and ctx.baseline_fetch()[1][site] == 0
    _one_locus(ctx, cat, 3, 1 * npairs + 5, every, R)
    assert _one_locus(ctx, cat, 4, 5 * npairs + 77, every, R)[2] > 0
    assert _one_locus(ctx, cat, 5, 7 * npairs + 33, every, R)[2] == 702
    before = ctx.surfaces(every)
    w = _one_locus(ctx, cat, 5, 6 * npairs + 33, every, R)
    assert w[0] > w[1] and w[2] == 0
    r = ctx.base_surfaces(every)
    assert _same_bits(r['T'], before[0]) and not r['nshared'].any()
    ctx.close()


@pytest.mark.parametrize('name', cc.NAMES)
def test_after_one_locus_it_is_the_conditional_surface_bit_for_bit(name):
    eng = _engine()
    cat = cc.catalogue(eng)[name]()
    ctx = cat.context(eng)
    _, R = ctx.fetch_lut()
    M = len(cat.tg)
    ctx.baseline_reset()
    lin = ctx.base_surfaces(np.arange(M, dtype=np.int32), want_T=False)['lin']
    pairs = cc.neighbours(cat)[:12]
    shared = 0
    for c in sorted(set(c for _, c in pairs))[:4]:
        tests = np.array(sorted(set([t for t, q in pairs if q == c] + cat.windows)), dtype=np.int32)
        _one_locus(ctx, cat, c, int(lin[c]) if lin[c] >= 0 else 1, tests, R)
        shared += int(ctx.base_surfaces(tests, want_T=False)['nshared'].sum())
    assert shared > 0
    far = cc.unreachable(cat)
    if far is not None:                             # a locus without a site writes nothing
        w = _one_locus(ctx, cat, far[0], far[1], np.array(cat.windows, dtype=np.int32), R)
        assert w[0] > w[1] and w[2] == 0
    ctx.close()


# ---------------------------------------------------------------------------------------------- against the restatement

@pytest.mark.parametrize('name', ('small', 'edges', 'ragged', 'ex1_B2_w50_s25', 'ex1_B2', 'demo2'))
def test_two_and_three_loci_against_the_host_restatement(name):
    eng = _engine()
    c = sc.case(name, eng)
    ctx = c.context(eng)
    _, R = ctx.fetch_lut()
    zc = _zc()
    apex = c.apex.astype(np.int32)
    ctx.baseline_reset()
    first = ctx.base_surfaces(apex, want_T=False)
    top = [k for k in np.argsort(-first['tmax'], kind='stable').tolist() if first['lin'][k] >= 0][:3]
    assert len(top) == 3
    loci = [(int(apex[k]), int(first['lin'][k])) for k in top]
    worst_T, worst_d = 0.0, 0.0
    for m, (t, lin) in enumerate(loci):
        w = ctx.baseline_add(t, lin)
        dh, ch, scale, written = sc.host_baseline(c, loci[:m + 1], R, zc)
        assert w == written[-1]
        if m == 0:
            continue
        d, cnt = ctx.baseline_fetch()
        assert np.array_equal(cnt, ch) and cnt.max() >= 1
        assert not d[ch == 0].any()
        err = np.abs(d - dh)
        assert np.all(err <= sc.D_TOL * scale), float(np.max(err[scale > 0] / scale[scale > 0]))
        worst_d = max(worst_d, float(np.max(err[scale > 0] / (sc.D_TOL * scale[scale > 0]))))
        res = ctx.base_surfaces(apex)
        tm, l = _numpy_argmax(res['T'])
        assert _same_bits(res['tmax'], tm) and np.array_equal(res['lin'], l)
        for q, t2 in enumerate(apex.tolist()):
            Th, nh, sh, S = stepwise.host_base_surface(c.gen, c.rows, R, c.As, c.tg[t2], c.lo[t2], c.hi[t2], dh, ch, zc, scale=True)
            assert np.array_equal(res['nsites'][q], nh) and np.array_equal(res['nshared'][q], sh), (name, m, q)
            assert np.array_equal(np.isnan(res['T'][q]), np.isnan(Th)), (name, m, q)
            if (nh > 0).any():
                e, s = float(np.nanmax(np.abs(res['T'][q] - Th))), float(S.max())
                assert e <= sc.REL_TOL * s, (name, m, q, e, s)
                worst_T = max(worst_T, e / (sc.REL_TOL * s))
    print('%s: loci %s; after two and three: worst |dT| / tolerance %.3g, worst |dd| / tolerance %.3g' % (name, loci, worst_T, worst_d))
    ctx.close()


@pytest.mark.parametrize('name', sc.NAMES)
def test_the_greedy_run_is_the_hosts_and_the_identity_holds(name):
    eng = _engine()
    c = sc.case(name, eng)
    ctx = c.context(eng)
    _, R = ctx.fetch_lut()
    zc = _zc()
    host = c.host_run(R=R, zc=zc)
    dev = stepwise.device_run(ctx, c.apex, c.ranges(), c.C)
    assert dev['order'] == host['order'] and dev['written'] == host['written'], (dev['order'], host['order'])
    for k in ('step', 'lin', 'nsites', 'nshared'):
        assert np.array_equal(dev[k], host[k]), (name, k)
    assert dev['evals'] == host['evals']
    scale = max(float(np.max(host['T_max'])), 1.0)
    for k in ('T_max', 'T'):
        assert np.all(np.abs(dev[k] - host[k]) <= 1e-9 * scale), (name, k)
    d, cnt = ctx.baseline_fetch()
    assert np.array_equal(cnt, host['cnt'])
    # the identity on the fetched baseline; the size of every entry's sum from the host's replay of the same loci
    total = float(dev['T_total'][dev['order'][-1]]) if dev['order'] else 0.0
    whole = 2.0 * float(np.sum(np.log1p(d)))
    size = 2.0 * float(np.sum(np.abs(np.log1p(d))))
    dh, ch = np.zeros(len(c.gen)), np.zeros(len(c.gen), dtype=np.int32)
    for k in dev['order']:
        t, lin = int(c.apex[k]), int(dev['lin'][k])
        S = stepwise.host_base_surface(c.gen, c.rows, R, c.As, c.tg[t], c.lo[t], c.hi[t], dh, ch, zc, scale=True)[3]
        size += float(S.reshape(-1)[lin])
        iA, ix, ia = cc.decode(lin, len(c.xs), len(c.ab))
        stepwise.host_baseline_add(dh, ch, c.gen, c.rows, R, c.tg[t], c.lo[t], c.hi[t], c.As[iA], ix, ia, zc)
    print('%s: accepted %s of %d apexes, %d surfaces; T_total %r, 2 sum log1p(d) %r, |difference| / size %.3g'
          % (name, [int(c.apex[k]) for k in dev['order']], len(c.apex), dev['evals'], total, whole, abs(total - whole) / size if size else 0.0))
    assert abs(total - whole) <= sc.ID_TOL * size
    # the brute form on the device: the skip rule changes no byte
    brute = stepwise.device_run(ctx, c.apex, c.ranges(), c.C, skip=False)
    assert brute['order'] == dev['order'] and brute['written'] == dev['written']
    for k in ('T_max', 'T', 'T_total'):
        assert _same_bits(brute[k], dev[k]), (name, k)
    for k in ('step', 'lin', 'nsites', 'nshared'):
        assert np.array_equal(brute[k], dev[k]), (name, k)
    d2, cnt2 = ctx.baseline_fetch()
    assert _same_bits(d2, d) and np.array_equal(cnt2, cnt)
    ctx.close()


# --------------------------------------------------------------------------------------------------------- independence

def _two_loci(ctx, apex):
    ctx.baseline_reset()
    first = ctx.base_surfaces(apex, want_T=False)
    for k in [k for k in np.argsort(-first['tmax'], kind='stable').tolist() if first['lin'][k] >= 0][:2]:
        assert ctx.baseline_add(int(apex[k]), int(first['lin'][k]))[2] > 0


def test_a_window_depends_on_that_window_and_the_baseline_alone():
    eng = _engine()
    cat = cc.catalogue(eng)['ex1_B2']()
    ctx = cat.context(eng)
    M = len(cat.tg)
    _two_loci(ctx, np.arange(0, M, 40, dtype=np.int32))
    rng = np.random.default_rng(9)
    t = rng.integers(0, M, 14).astype(np.int32)
    t = np.append(t, [t[0], t[0], t[3]]).astype(np.int32)               # repeated
    full = ctx.base_surfaces(t)
    assert (full['nshared'] > 0).any()
    for q in (-1, -2, -3):
        src = 0 if q != -1 else 3
        for k in FLOATS:
            assert _same_bits(full[k][q], full[k][src])
        for k in INTS:
            assert np.array_equal(full[k][q], full[k][src])
    for q in (0, 7, 13):                                                 # alone
        one = ctx.base_surfaces(t[q:q + 1])
        for k in FLOATS:
            assert _same_bits(one[k][0], full[k][q]), (k, q)
        for k in INTS:
            assert np.array_equal(one[k][0], full[k][q]), (k, q)
    rev = ctx.base_surfaces(t[::-1])                                     # the list reversed
    for k in FLOATS:
        assert _same_bits(rev[k][::-1], full[k]), k
    for k in INTS:
        assert np.array_equal(rev[k][::-1], full[k]), k
    bare = ctx.base_surfaces(t, want_T=False)
    assert bare['T'] is None and _same_bits(bare['tmax'], full['tmax']) and np.array_equal(bare['nshared'], full['nshared'])
    ctx.close()


def test_a_list_across_a_chunk_seam_matches_the_windows_asked_singly():
    eng = _engine()
    scene = cs.scene('one_pair')                    # the smallest grid: one pair, 16 A
    step, by_bytes, by_threads = cs.surfaces_step(scene.nA, scene.npairs)
    assert step == by_threads == 1048575
    ctx = scene.context(eng)
    ctx.baseline_reset()
    for t, lin in ((2, 3), (9, 0), (5, 7)):         # three loci among the 13, from every site of a short window to few
        ctx.baseline_add(t, lin)
    assert ctx.baseline_fetch()[1].any()
    singly = [ctx.base_surfaces([q]) for q in range(cs.K)]
    assert any(r['nshared'].any() for r in singly)
    n = step + 5
    full = ctx.base_surfaces(cs.rotation(n))
    at = np.arange(n) % cs.K
    for k in FLOATS:
        assert _same_bits(full[k], np.concatenate([r[k] for r in singly])[at]), k
    for k in INTS:
        assert np.array_equal(full[k], np.concatenate([r[k] for r in singly])[at]), k
    bare = ctx.base_surfaces(cs.rotation(n), want_T=False)
    assert _same_bits(bare['tmax'], full['tmax']) and np.array_equal(bare['lin'], full['lin'])
    ctx.close()


# ----------------------------------------------------------------------------------------------------- state and errors

def _raw_surfaces(ctx, n, tests, T=None, ns=None, nsh=None, tmax=None, lin=None):
    p = lambda a, f: None if a is None else f(a)
    return ctx._L.bmx_ctx_base_surfaces(ctx._h, n, p(tests, _lib.as_ip), p(T, _lib.as_dp), p(ns, _lib.as_ip), p(nsh, _lib.as_ip),
                                        p(tmax, _lib.as_dp), p(lin, _lib.as_ip))


def test_state_and_errors():
    opt, case, ts, sel = _case_ctx(cases.ALL_CASES['ex1_B2'][0])
    ctx = sel.ctx
    M, N = len(ts), len(case.data.genPos)
    L = ctx._L
    one = np.zeros(1, dtype=np.int32)
    ms = C.c_double()
    f, l, nw = C.c_int64(7), C.c_int64(7), C.c_int32(7)
    add = lambda h, t, lin: L.bmx_ctx_baseline_add(h, t, lin, C.byref(f), C.byref(l), C.byref(nw))
    untouched = lambda: (f.value, l.value, nw.value) == (7, 7, 7)
    # a NULL context
    assert L.bmx_ctx_baseline_reset(None) == INVALID and add(None, 0, 0) == INVALID and L.bmx_ctx_baseline_fetch(None, None, None) == INVALID
    assert L.bmx_ctx_base_surfaces(None, 1, _lib.as_ip(one), None, None, None, None, None) == INVALID
    assert L.bmx_ctx_base_surfaces_ms(None, C.byref(ms)) == INVALID and L.bmx_ctx_base_surfaces_ms(ctx._h, None) == INVALID
    # model and sites, no test sites yet: reset works, add and base_surfaces are refused for the state
    assert L.bmx_ctx_baseline_fetch(ctx._h, None, None) == STATE            # no baseline yet
    ctx.baseline_reset()
    assert add(ctx._h, 0, 0) == STATE and _raw_surfaces(ctx, 1, one) == STATE and untouched()
    assert L.bmx_ctx_base_surfaces_ms(ctx._h, C.byref(ms)) == STATE
    ctx.set_tests(ts.test_gen, ts.lo, ts.hi)
    ctx.scan()
    before, rec0 = ctx.fetch(), ctx.fetch_records()
    pk = ctx.peaks(0.00005, 5.0)
    apex = pk['row']
    assert len(apex) >= 3
    nx, nab = len(sel.model.x), len(sel.model.abeta)
    points = ctx.nA * nx * nab
    lin = np.where(before[3] >= 0, (before[3].astype(np.int64) * nx + before[1]) * nab + before[2], -1).astype(np.int32)
    cond0 = ctx.cond_surfaces(apex, np.roll(apex, 1), lin[np.roll(apex, 1)])
    # the refusals of baseline_add, each with its code; nothing is written
    for t, li in ((-1, 0), (M, 0), (0, -1), (0, points)):
        assert add(ctx._h, t, li) == INVALID and untouched(), (t, li)
    d, cnt = ctx.baseline_fetch(N)
    assert not d.any() and not cnt.any()
    with pytest.raises(BmxError) as e:
        ctx.baseline_add(M, 0)
    assert e.value.code == INVALID and 'index' in str(e.value)
    # ... and of base_surfaces
    ok = np.array([3, 4], dtype=np.int32)
    T = np.full((2, points), 7.0)
    outs = dict(ns=np.full((2, ctx.nA), 7, np.int32), nsh=np.full((2, ctx.nA), 7, np.int32), tmax=np.full(2, 7.0), lin=np.full(2, 7, np.int32))
    for n, a in ((-1, ok), (2, None), (2, np.array([3, -1], np.int32)), (2, np.array([M, 3], np.int32))):
        assert _raw_surfaces(ctx, n, a, T, **outs) == INVALID, (n, a)
        assert (T == 7.0).all() and all((v == 7).all() for v in outs.values())
    assert L.bmx_ctx_base_surfaces_ms(ctx._h, C.byref(ms)) == STATE          # no successful call yet
    # a reset, three adds and a base_surfaces call leave everything else as it was
    for k in (0, 1, 2):
        assert ctx.baseline_add(int(apex[k]), int(lin[apex[k]]))[2] > 0
    r = ctx.base_surfaces(apex)
    assert r['nshared'].any() and ctx.base_surfaces_ms() > 0
    assert _raw_surfaces(ctx, 0, None) == 0 and _raw_surfaces(ctx, 2, ok) == 0          # n == 0; every output NULL
    e0 = ctx.base_surfaces([])
    assert e0['T'].shape == (0, ctx.nA, nx, nab) and e0['nshared'].shape == (0, ctx.nA) and e0['tmax'].shape == (0,)
    assert all(np.array_equal(a, b) for a, b in zip(before, ctx.fetch()))
    assert rec0.tobytes() == ctx.fetch_records().tobytes()
    pk2 = ctx.fetch_peaks()
    assert all(np.array_equal(pk[k], pk2[k]) for k in peaks.FIELDS)
    cond1 = ctx.cond_surfaces(apex, np.roll(apex, 1), lin[np.roll(apex, 1)])
    _same(cond1, cond0)
    # fetch with either pointer NULL
    d, cnt = ctx.baseline_fetch(N)
    d2 = np.empty(N)
    assert L.bmx_ctx_baseline_fetch(ctx._h, _lib.as_dp(d2), None) == 0 and _same_bits(d2, d)
    c2 = np.empty(N, dtype=np.int32)
    assert L.bmx_ctx_baseline_fetch(ctx._h, None, _lib.as_ip(c2)) == 0 and np.array_equal(c2, cnt) and cnt.max() >= 2
    # a second slot has no baseline; the first one's is still there
    ctx.select_slot(1)
    assert L.bmx_ctx_baseline_reset(ctx._h) == STATE and L.bmx_ctx_baseline_fetch(ctx._h, None, None) == STATE
    ctx.select_slot(0)
    _same(ctx.base_surfaces(apex), r)
    # set_sites drops the baseline
    g, rows = ctx.fetch_sites(N)
    ctx.set_sites(g, rows)
    ctx.set_tests(ts.test_gen, ts.lo, ts.hi)
    assert add(ctx._h, 0, 0) == STATE and _raw_surfaces(ctx, 1, one) == STATE and L.bmx_ctx_baseline_fetch(ctx._h, None, None) == STATE
    with pytest.raises(BmxError) as e:
        ctx.base_surfaces([0])
    assert e.value.code == STATE
    ctx.baseline_reset()
    assert not ctx.baseline_fetch(N)[1].any()
    assert _same_bits(ctx.base_surfaces(apex)['T'], ctx.surfaces(apex)[0])
    # ... and so do resample_sites and plant_sites on the slot that receives the sites; the source slot keeps its own
    from ballermixplus_amd import power
    m = sel.model
    gw = np.minimum(power.allowed_rows(m.stat, m.min_count, m.sizes, m.row_off, m.g), 1.0)
    ctx.select_slot(1)
    for replace in (lambda: ctx.resample_sites(0, 123, 1), lambda: ctx.plant_sites(0, 77, [float(g[N // 2])], 0, 0, 0, gw)):
        replace()
        assert L.bmx_ctx_baseline_fetch(ctx._h, None, None) == STATE
        ctx.baseline_reset()
        assert L.bmx_ctx_baseline_fetch(ctx._h, None, None) == 0
        replace()
        assert L.bmx_ctx_baseline_fetch(ctx._h, None, None) == STATE and L.bmx_ctx_baseline_reset(ctx._h) == 0
    ctx.select_slot(0)
    assert L.bmx_ctx_baseline_fetch(ctx._h, None, None) == 0
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ CLI

def _host_table(argv, G, peak_min, C, kmax=stepwise.MAX_LOCI):
    """The file the host restatement and the writer produce for one input: the device's scan and peak call, then host_run on the
    device's table.  Returns (rows as lists of strings, the host run, the apex rows, sel)."""
    opt, case, ts, sel = _case_ctx(argv)
    ctx = sel.ctx
    ctx.set_tests(ts.test_gen, ts.lo, ts.hi)
    ctx.scan()
    clr = ctx.fetch()[0]
    apex = ctx.peaks(G, peak_min)['row'].astype(np.int64)
    _, R = ctx.fetch_lut()
    g, rows = ctx.fetch_sites()
    tg, lo, hi = np.asarray(ts.test_gen)[apex], np.asarray(ts.lo)[apex], np.asarray(ts.hi)[apex]
    m = sc.Margins(C)
    out = stepwise.host_run(g, rows, R, [float(v) for v in sel.grid_A], tg, lo, hi, _zc(), C, kmax, watch=m.watch, keep_T=True)
    assert min(m.worst()) > sc.MARGIN, m.worst()
    phys, gen = surfaces.labels(ts, apex.tolist())
    table = [r.rstrip('\n').split('\t') for r in stepwise.table_rows(phys, gen, [repr(float(v)) for v in clr[apex]], out, sel)]
    return table, out, apex, sel, (phys, gen)


FLOAT_COLS = (3, 5, 11, 12)           # T_max, CLR_cond, retained, T_total: sums the host and the device round differently


def _check_file(path, table):
    """The written file against the host's: every column byte for byte but the four sums, which agree to 1e-9 relative."""
    names, rows = stepwise.read_table(path)
    assert '\t'.join(names) + '\n' == stepwise.HEADER and len(rows) == len(table)
    for got, want in zip(rows, table):
        for j, (a, b) in enumerate(zip(got, want)):
            if j in FLOAT_COLS and a != b:
                assert 'NA' not in (a, b) and abs(float(a) - float(b)) <= 1e-9 * max(abs(float(b)), 1.0), (j, got, want)
            else:
                assert a == b, (j, got, want)


def test_cli_on_example_1(tmp_path):
    plain, st = str(tmp_path / 'plain.txt'), str(tmp_path / 'st.txt')
    flags = ['--peaks', '0.00005', '--peakMin', '5']            # (Example 1 spans 0.001 in genPos: five apexes)
    _cli(EX1 + ['-o', plain] + flags)
    r = _cli(EX1 + ['-o', st] + flags + ['--stepwise', '--stepSurfaces'])          # (C: --peakMin's 5)
    assert sorted(os.listdir(tmp_path)) == ['plain.txt', 'plain.txt.peaks.txt', 'st.txt', 'st.txt.peaks.txt', 'st.txt.stepwise.surfaces.txt',
                                            'st.txt.stepwise.txt']
    assert _read(plain) == _read(st) and _read(peaks.output_name(plain)) == _read(peaks.output_name(st))
    table, out, apex, sel, (phys, gen) = _host_table(cases.ALL_CASES['ex1_B2'][0], 0.00005, 5.0, 5.0)
    assert len(apex) >= 3 and 1 <= len(out['order']) < len(apex)
    _check_file(stepwise.output_name(st), table)
    with open(peaks.output_name(st)) as f:
        assert [l.split('\t')[:3] for l in f.readlines()[1:]] == [t[:3] for t in table]
    assert 'Stepwise: %d apex/es, %d accepted (threshold 5.0)' % (len(apex), len(out['order'])) in r.stdout
    # --stepSurfaces: the accepted apexes' surfaces at entry, in order of entry: the device's own, bit for bit
    layout = surfaces.Layout(sel.grid_A, sel.grid_x, sel.grid_abeta)
    fp, fg, Tf, nf = surfaces.read_surfaces(stepwise.surfaces_name(st), layout)
    assert fp == [phys[k] for k in out['order']] and fg == [gen[k] for k in out['order']]
    ctx = sel.ctx
    ctx.baseline_reset()
    for j, k in enumerate(out['order']):
        res = ctx.base_surfaces([int(apex[k])])
        assert _same_bits(Tf[j], layout.ascending(res['T'])[0]) and np.array_equal(nf[j], res['nsites'][0][layout.oA])
        assert np.nanmax(np.abs(Tf[j] - layout.ascending(out['entry_T'][j][None])[0])) <= 1e-9 * float(out['T_max'].max())
        ctx.baseline_add(int(apex[k]), int(out['lin'][k]))
    ctx.close()


def test_cli_on_the_planted_chromosome_and_two_files(tmp_path):
    from ballermixplus_amd import cli
    files = sc.demo_files(tmp_path, 2)
    d1, d2 = tmp_path / 'plain', tmp_path / 'st'
    ins = files[1] + ',' + sc.demo_files(tmp_path, 1, 'one_locus')[1]          # (the second file under the first one's spectrum)
    tail = ['--spect', files[3]] + sc.DEMO_CLI
    cli.main(['-i', ins, '-o', str(d1)] + tail)
    cli.main(['-i', ins, '-o', str(d2)] + tail + ['--stepwise'])
    outs = sorted(os.listdir(d1))
    assert sorted(f for f in os.listdir(d2) if 'stepwise' not in f) == outs
    assert sorted(f for f in os.listdir(d2) if 'stepwise' in f) == ['one_locus.txt.out.txt.stepwise.txt', 'planted.txt.out.txt.stepwise.txt',
                                                                      'stepwise.txt']
    for f in outs:
        assert _read(d1 / f) == _read(d2 / f), f
    # the planted chromosome: C = --peakMin's 5; the host accepts the two planted loci first
    table, out, apex, sel, _ = _host_table(files + sc.DEMO_CLI[:-4], cc.DEMO_SEP, cc.DEMO_MIN, cc.DEMO_MIN)
    sel.ctx.close()
    path = str(d2 / 'planted.txt.out.txt')
    _check_file(stepwise.output_name(path), table)
    sites = apex[out['order'][:2]] * cc.DEMO_STEP
    assert abs(int(sites[0]) - cc.DEMO_CENTRES[1]) <= 4 * cc.DEMO_STEP and abs(int(sites[1]) - cc.DEMO_CENTRES[0]) <= 4 * cc.DEMO_STEP
    assert len(out['order']) > 2 and (out['step'] == 0).any()
    # the genome-wide table: both files' rows in file order with a leading `file` column
    with open(d2 / 'stepwise.txt') as f:
        lines = f.read().split('\n')
    assert lines[0] == 'file\t' + stepwise.HEADER[:-1]
    want = []
    for name in ('planted.txt', 'one_locus.txt'):
        with open(d2 / (name + '.out.txt.stepwise.txt')) as f:
            want += [name + '\t' + l for l in f.read().split('\n')[1:] if l]
    assert [l for l in lines[1:] if l] == want and len(want) > len(table)
