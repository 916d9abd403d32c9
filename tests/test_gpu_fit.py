"""The goodness-of-fit table of a window on the GPU (--fit): bmx_ctx_fit against the host restatement on the catalogue of
fitcases.py, its exact relation to bmx_ctx_surfaces, its independence of the list, the two homes of the prologue sums, what the
call leaves untouched, its errors, the planted case, and the CLI end to end."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import fitcases as fc
from test_fit_cpu import planted_verdict
from test_gpu_refine import _case_ctx, _cli, _engine, _read
from test_gpu_surfaces import EX1, _forty, _same_bits
from util import REPO

from ballermixplus_amd import _lib, fit, peaks, power, surfaces
from ballermixplus_amd._lib import BmxError

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case, its context, the device's own table and cut."""
    c = fc.catalogue(_engine())[name]()
    ctx = c.cat.context(_engine())
    _, R = ctx.fetch_lut()
    return c, ctx, R, float(_lib.lib().bmx_alpha_cut())


def _fit(c, ctx, tests=None, lins=None):
    return ctx.fit(c.tests() if tests is None else tests, c.lins() if lins is None else lins, c.gw, c.cls, c.F, c.edges)


def _compare(c, got, R, zcut, entries=None):
    """O and skipped exactly, E within TOL * max(1, n_d) per cell; returns the worst ratio to the bound."""
    O, Es, En, sk = got
    worst = 0.0
    for q in (range(len(c.entries)) if entries is None else entries):
        hO, hEs, hEn, hsk = c.host(q, R, zcut)
        assert np.array_equal(O[q], hO) and sk[q] == hsk, (c.name, q)
        if c.entries[q][1] < 0:
            assert np.isnan(Es[q]).all() and np.isnan(En[q]).all()
            continue
        bound = fc.TOL * np.maximum(1, hO.sum(axis=1))[:, None]
        es, en = np.abs(Es[q] - hEs) / bound, np.abs(En[q] - hEn) / bound
        print('%s entry %d: n %d, skipped %d, |dE_sel| / bound %.3e, |dE_neu| / bound %.3e' % (c.name, q, hO.sum(), hsk, es.max(), en.max()))
        assert es.max() <= 1.0 and en.max() <= 1.0, (c.name, q, es.max(), en.max())
        worst = max(worst, float(es.max()), float(en.max()))
    return worst


# ------------------------------------------------------------------------------------------- against the host restatement

@pytest.mark.parametrize('name', fc.NAMES)
def test_against_host_fit(name):
    c, ctx, R, zcut = _case(name)
    got = _fit(c, ctx)
    assert got[0].shape == (len(c.entries), c.D, c.F) and got[0].dtype == np.int32 and got[3].shape == (len(c.entries),)
    worst = _compare(c, got, R, zcut)
    print('%s: worst ratio to the bound %.3e%s' % (name, worst, ' (ABOVE A TENTH)' if worst > 0.1 else ''))
    # the sites are the surfaces' sites at that A, exactly
    _, ns = ctx.surfaces(c.tests())
    for q, (w, lin) in enumerate(c.entries):
        if lin >= 0:
            assert int(got[0][q].sum()) == int(ns[q, lin // (c.nx * c.nab)]), (name, q)
    if name == 'many_sizes':
        assert len(c.sizes) * (c.F + 1) * 24 > fc.header_constant('BMX_FIT_LDS_BYTES')         # the workspace in device memory
        for q in (0, 3):           # the conditioning on the device's own table (the CPU test saw a stand-in)
            h, l = c.host(q, R, zcut), c.host(q, R, zcut, dtype=np.longdouble)
            bound = fc.TOL * np.maximum(1, h[0].sum(axis=1))[:, None]
            assert max(np.max(np.abs(h[1] - l[1]) / bound), np.max(np.abs(h[2] - l[2]) / bound)) <= 0.1
    if name == 'excluded':
        assert got[3].max() > 0
    if name == 'edges':
        assert set((0, 1, 255, 256, 257, 512, 513)) <= {int(o.sum()) for o in got[0]}
    print('kernel %.3f ms' % ctx.fit_ms())


def test_the_bin_rule_on_the_device():
    """The lattice case holds, for every edge, a site on it and one an ulp either side, left and right of the test position."""
    c, ctx, R, zcut = _case('lattice')
    gen, marks = fc.lattice_positions()
    q = [k for k, (w, lin) in enumerate(c.entries) if w == 0 and lin // (c.nx * c.nab) == 0][0]      # all sites, A = 16
    O = _fit(c, ctx)[0][q]
    z = fc.LATTICE_A * np.abs(gen)
    z = z[z <= zcut]
    for k, e in enumerate(c.edges.tolist()):
        assert np.count_nonzero(z == e) == 2
        assert O[k].sum() == np.count_nonzero((z > (c.edges[k - 1] if k else 0.0)) & (z <= e))


# --------------------------------------------------------------------------------------------------------- independence

def test_a_window_alone_in_a_list_and_twice_gives_the_same_bits():
    c, ctx, R, zcut = _case('ex1_B2')
    M = len(c.cat.tg)
    tests = np.array(_forty(M, 11), dtype=np.int32)
    points = len(c.cat.As) * c.nx * c.nab
    lins = ((np.arange(len(tests)) * 7919 + 3) % points).astype(np.int32)
    lins[-1], lins[-2] = lins[0], lins[1]            # the repeated indices (M - 1 and pick[0]) with the same grid point
    O, Es, En, sk = ctx.fit(tests, lins, c.gw, c.cls, c.F, c.edges)
    assert len(tests) == 41

    def same(a, qa, b, qb):
        return (np.array_equal(a[0][qa], b[0][qb]) and _same_bits(a[1][qa], b[1][qb]) and _same_bits(a[2][qa], b[2][qb])
                and a[3][qa] == b[3][qb])

    full = (O, Es, En, sk)
    for q in (0, 1, 2, 17, len(tests) - 3, len(tests) - 1):
        one = ctx.fit(tests[q:q + 1], lins[q:q + 1], c.gw, c.cls, c.F, c.edges)
        assert same(full, q, one, 0), q
    assert tests[0] == tests[-1] and tests[1] == tests[-2] and same(full, 0, full, len(tests) - 1) and same(full, 1, full, len(tests) - 2)
    # one window at several grid points in one list: each is its own
    w = int(tests[5])
    three = ctx.fit([w, w, w], [lins[5], -1, lins[6]], c.gw, c.cls, c.F, c.edges)
    assert same(three, 0, full, 5) and not three[0][1].any() and np.isnan(three[1][1]).all() and np.isnan(three[2][1]).all()
    assert three[3][1] == 0 and same(three, 2, ctx.fit([w], [lins[6]], c.gw, c.cls, c.F, c.edges), 0)
    # an unrelated set_tests round trip on another slot changes nothing
    ctx.select_slot(1)
    try:
        ctx.set_sites(c.cat.gen[:300], c.cat.rows[:300])
        ctx.set_tests(c.cat.gen[10:20])
        ctx.fit([0, 3], [5, 9], c.gw, c.cls, c.F, c.edges)
    finally:
        ctx.select_slot(0)
    again = ctx.fit(tests, lins, c.gw, c.cls, c.F, c.edges)
    assert all(same(full, q, again, q) for q in range(len(tests)))


def test_the_two_homes_of_the_prologue_sums_agree():
    """A case that fits LDS, run once from LDS and once from the workspace in device memory (bmx_ctx_set_variant(1)): O and
    skipped equal, E within the tolerance of each other and of the host."""
    c, ctx, R, zcut = _case('ragged')
    assert len(c.sizes) * (c.F + 1) * 24 <= fc.header_constant('BMX_FIT_LDS_BYTES')
    lds = _fit(c, ctx)
    ctx.set_variant(1)
    try:
        glob = _fit(c, ctx)
    finally:
        ctx.set_variant(0)
    assert np.array_equal(lds[0], glob[0]) and np.array_equal(lds[3], glob[3])
    bound = fc.TOL * np.maximum(1, lds[0].sum(axis=2))[:, :, None]
    ok = ~np.isnan(lds[1])
    assert np.array_equal(ok, ~np.isnan(glob[1]))
    assert np.all((np.abs(lds[1] - glob[1]) <= bound)[ok]) and np.all((np.abs(lds[2] - glob[2]) <= bound)[ok])
    _compare(c, glob, R, zcut)


# --------------------------------------------------------------------------------------------------------- call hygiene

def test_the_call_leaves_the_slot_as_it_was():
    c, ctx, R, zcut = _case('ex1_B2')
    ctx.set_profiles('A')
    try:
        ctx.scan()
        pk = ctx.peaks(1e-4, 0.0, peaks.FRAC)
        before, sites, rec, prof = ctx.fetch(), ctx.fetch_sites(len(c.cat.gen)), ctx.fetch_records(), ctx.fetch_profile('A')
        _fit(c, ctx)
        after, sites2, rec2, prof2 = ctx.fetch(), ctx.fetch_sites(len(c.cat.gen)), ctx.fetch_records(), ctx.fetch_profile('A')
        pk2 = ctx.fetch_peaks()
    finally:
        ctx.set_profiles(0)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert all(np.array_equal(a, b) for a, b in zip(sites, sites2)) and rec.tobytes() == rec2.tobytes()
    assert prof.tobytes() == prof2.tobytes() and len(pk['row']) > 0 and all(np.array_equal(pk[k], pk2[k]) for k in pk)


def test_errors():
    L = _lib.lib()
    one = np.zeros(1, dtype=np.int32)
    assert L.bmx_ctx_fit(None, 1, _lib.as_ip(one), _lib.as_ip(one), None, None, 1, None, 1, None, None, None, None) == -1
    assert L.bmx_ctx_fit_ms(None, None) == -1
    opt, case, ts, sel = _case_ctx(cases.ALL_CASES['ex1_B2'][0])
    ctx = sel.ctx
    m = sel.model
    gw = power.allowed_rows(m.stat, m.min_count, m.sizes, m.row_off, m.g)
    F, edges = 4, np.array([1.0, 5.0])
    cls = fit.classes(m.stat, m.sizes, m.row_off, F)
    for call in (lambda: ctx.fit([0], [0], gw, cls, F, edges), ctx.fit_ms):       # model and sites, no test sites yet; no call yet
        with pytest.raises(BmxError) as e:
            call()
        assert e.value.code == -5
    ctx.set_tests(ts.test_gen, ts.lo, ts.hi)
    M, points = len(ts), ctx.nA * len(m.x) * len(m.abeta)
    D = len(edges) + 1
    O = np.full((2, D, F), -7, dtype=np.int32)
    Es, En = np.full((2, D, F), -7.0), np.full((2, D, F), -7.0)
    sk = np.full(2, -7, dtype=np.int32)

    def raw(n, tests, lin, gw_, cls_, F_, edges_, D_, O_=O, Es_=Es, En_=En):
        p = lambda a, f: None if a is None else f(a)
        return L.bmx_ctx_fit(ctx._h, n, p(tests, _lib.as_ip), p(lin, _lib.as_ip), p(gw_, _lib.as_dp), p(cls_, _lib.as_ip), F_,
                             p(edges_, _lib.as_dp), D_, p(O_, _lib.as_ip), p(Es_, _lib.as_dp), p(En_, _lib.as_dp), _lib.as_ip(sk))

    t2, l2 = np.array([0, 1], dtype=np.int32), np.array([0, 1], dtype=np.int32)
    i32 = lambda v: np.array(v, dtype=np.int32)
    assert raw(-1, t2, l2, gw, cls, F, edges, D) == -1
    for k in range(7):                                  # every NULL array with n > 0
        args = [t2, l2, gw, cls, edges, O, Es]
        args[k] = None
        assert raw(2, args[0], args[1], args[2], args[3], F, args[4], D, args[5], args[6]) == -1, k
    assert raw(2, t2, l2, gw, cls, F, edges, D, En_=None) == -1
    for bad in ([-1, 0], [0, M]):
        assert raw(2, i32(bad), l2, gw, cls, F, edges, D) == -1 and 'index' in L.bmx_last_error().decode()
    assert raw(2, t2, i32([0, points]), gw, cls, F, edges, D) == -1 and 'grid point' in L.bmx_last_error().decode()
    for F_, D_ in ((0, 3), (4, 0), (4, 65), (257, 1), (-1, 3)):
        assert raw(2, t2, l2, gw, cls, F_, edges, D_) == -1, (F_, D_)
    for bad in ([1.0, np.inf], [np.nan, 5.0], [0.0, 5.0], [-1.0, 5.0], [5.0, 5.0], [5.0, 1.0]):
        assert raw(2, t2, l2, gw, cls, F, np.array(bad), D) == -1 and 'edges' in L.bmx_last_error().decode(), bad
    for bad in (-1, F):
        c2 = cls.copy()
        c2[len(c2) // 2] = bad
        assert raw(2, t2, l2, gw, c2, F, edges, D) == -1 and 'class' in L.bmx_last_error().decode()
    for bad in (-0.5, 1.5, np.nan, np.inf):
        g2 = gw.copy()
        g2[3] = bad
        assert raw(2, t2, l2, g2, cls, F, edges, D) == -1 and 'gw' in L.bmx_last_error().decode()
    # nothing was written on any of these, and no failed call counts as a call
    assert (O == -7).all() and (Es == -7.0).all() and (En == -7.0).all() and (sk == -7).all()
    with pytest.raises(BmxError) as e:
        ctx.fit_ms()
    assert e.value.code == -5
    assert raw(0, None, None, None, None, F, None, D, None, None, None) == 0 and (O == -7).all()       # n == 0 succeeds
    r = ctx.fit([], [], gw, cls, F, edges)
    assert r[0].shape == (0, D, F) and r[3].shape == (0,) and ctx.fit_ms() == 0.0
    assert raw(2, t2, l2, gw, cls, F, edges, D) == 0 and (O >= 0).all() and (sk >= 0).all()
    assert L.bmx_ctx_fit(ctx._h, 2, _lib.as_ip(t2), _lib.as_ip(l2), _lib.as_dp(gw), _lib.as_ip(cls), F, _lib.as_dp(edges), D,
                         _lib.as_ip(O), _lib.as_dp(Es), _lib.as_dp(En), None) == 0                       # skipped_out may be NULL
    one_bin = ctx.fit([0], [0], gw, cls, F, [])                                                          # D = 1: no edge
    assert one_bin[0].shape == (1, 1, F) and one_bin[0].sum() == O[0].sum()
    ctx.close()


# ------------------------------------------------------------------------------------------------------ the planted case

def test_the_planted_point_fits_on_the_device():
    c, lin = fc.planted(_engine())
    ctx = c.cat.context(_engine())
    O, Es, En, sk = _fit(c, ctx)
    _, R = ctx.fetch_lut()
    _compare(c, (O, Es, En, sk), R, float(_lib.lib().bmx_alpha_cut()))
    s = planted_verdict(O[0], Es[0], En[0])
    print('planted on the device: X2_sel %.2f (df %d), X2_neu %.2f (df %d)' % (s['X2_sel'], s['df_sel'], s['X2_neu'], s['df_neu']))
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ CLI

def _tables_agree(got_out, want_out, D, F):
    """The two files of one run against the files fit.py wrote from the host restatement: strings and counts exactly, expected
    counts within the tolerance, the sums to rounding."""
    gn, g = fit.read_table(fit.output_name(got_out))
    wn, w = fit.read_table(fit.output_name(want_out))
    assert gn == wn and len(g) == len(w) and len(g) > 0
    for a, b in zip(g, w):
        assert a[:8] == b[:8] and a[9] == b[9] and a[11:15] == b[11:15], (a, b)
        for k in (8, 10, 15):
            assert (a[k] == b[k] == 'NA') or abs(float(a[k]) - float(b[k])) <= 1e-9 * max(1.0, abs(float(b[k]))), (k, a, b)
    gp, gg, gO, gEs, gEn = fit.read_cells(fit.cells_name(got_out), D, F)
    wp, wg, wO, wEs, wEn = fit.read_cells(fit.cells_name(want_out), D, F)
    assert gp == wp and gg == wg and np.array_equal(gO, wO) and len(gp) == len(g)
    bound = fc.TOL * np.maximum(1, wO.sum(axis=2))[:, :, None]
    assert np.all(np.abs(gEs - wEs) <= bound) and np.all(np.abs(gEn - wEn) <= bound)


def test_cli_end_to_end(tmp_path):
    plain, pk, mn = str(tmp_path / 'plain.txt'), str(tmp_path / 'pk.txt'), str(tmp_path / 'mn.txt')
    G = '0.0001'
    _cli(EX1 + ['-o', plain, '--peaks', G])
    r = _cli(EX1 + ['-o', pk, '--peaks', G, '--fit', '--fitDetail'])
    r2 = _cli(EX1 + ['-o', mn, '--fit', '--fitMin', '0', '--fitMax', '5', '--fitBins', '4', '--fitClasses', '6', '--fitMinExp', '3',
                     '--fitDetail'])
    assert sorted(os.listdir(tmp_path)) == ['mn.txt', 'mn.txt.fit.cells.txt', 'mn.txt.fit.txt', 'pk.txt', 'pk.txt.fit.cells.txt',
                                            'pk.txt.fit.txt', 'pk.txt.peaks.txt', 'plain.txt', 'plain.txt.peaks.txt']
    assert _read(plain) == _read(pk) == _read(mn) and _read(peaks.output_name(plain)) == _read(peaks.output_name(pk))
    assert 'Fit: ' in r.stdout and '8 distance bin/s x 10 frequency class/es' in r.stdout and '--fitMax' not in r.stdout
    assert 'Fit: 5 window/s, 4 distance bin/s x 6 frequency class/es' in r2.stdout
    # the same windows through the library, the tables by the host restatement on the device's own table
    opt, case, ts, sel = _case_ctx(cases.ALL_CASES['ex1_B2'][0])
    ctx = sel.ctx
    ctx.set_tests(ts.test_gen, ts.lo, ts.hi)
    ctx.scan()
    clr, ix, ia, iA, _ = ctx.fetch()
    called = ctx.peaks(float(G), 0.0, peaks.FRAC)
    _, R = ctx.fetch_lut()
    zcut = float(_lib.lib().bmx_alpha_cut())
    m = sel.model
    nx, nab = len(m.x), len(m.abeta)
    gw = power.allowed_rows(m.stat, m.min_count, m.sizes, m.row_off, m.g)
    gen, rows_of = ctx.fetch_sites(len(case.data.genPos))
    for out, apex, min_clr, max_n, D, F, min_exp in ((pk, called['row'], 0.0, fit.MAX_WINDOWS, 8, 10, 5.0), (mn, None, 0.0, 5, 4, 6, 3.0)):
        sel_rows, dropped = surfaces.select(clr, iA, min_clr, apex, max_n)
        assert len(sel_rows) >= 1
        if out == mn:
            assert len(sel_rows) == 5 and dropped > 0
            assert ('--fitMax: %d more window/s qualified and were dropped (the 5 with the highest CLR are kept).' % dropped) in r2.stdout
        cls, edges = fit.classes(m.stat, m.sizes, m.row_off, F), fit.default_edges(D, zcut)
        lin = ((iA.astype(np.int64) * nx + ix) * nab + ia)[sel_rows]
        tabs = [fit.host_fit(gen, rows_of, m.row_off, R, gw, cls, F, edges, sel.grid_A[iA[t]], ix[t], ia[t], ts.test_gen[t], ts.lo[t],
                             ts.hi[t], zcut) for t in sel_rows.tolist()]
        phys, genl = surfaces.labels(ts, sel_rows.tolist())
        want = str(tmp_path / ('want_' + os.path.basename(out)))
        fit.write_fit(want, phys, genl, [repr(float(v)) for v in clr[sel_rows]], lin, sel, np.array([t[0] for t in tabs]),
                      np.array([t[1] for t in tabs]), np.array([t[2] for t in tabs]), [t[3] for t in tabs], edges, zcut, min_exp, detail=True)
        _tables_agree(out, want, D, F)
        main = {tuple(l.split('\t')[:2]): l.split('\t') for l in open(out).readlines()[1:]}
        for row in fit.read_table(fit.output_name(out))[1]:
            assert row[:6] == main[(row[0], row[1])][:6]                 # the main output's strings, grid point included
    ctx.close()
    bad = subprocess.run([sys.executable, os.path.join(REPO, 'BalLeRMixPlus_amd.py')] + EX1 + ['-o', str(tmp_path / 'x.txt'), '--fitBins', '4'],
                         capture_output=True, text=True, timeout=300, cwd=REPO)
    assert bad.returncode == 1 and bad.stdout.strip() == '--fitBins needs --fit.' and not os.path.exists(str(tmp_path / 'x.txt'))
