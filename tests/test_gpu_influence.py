"""The delete-block jackknife of a window's CLR on the GPU (--influence): bmx_ctx_influence's exact relations to
bmx_ctx_surfaces, its independence of the list, the comparison with the host restatement on the catalogue of influencecases.py
and with real deletion of a block, what the call leaves untouched, its errors, and the CLI end to end."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import cases
import influencecases as ic
from test_gpu_refine import _case_ctx, _cli, _engine, _read
from test_gpu_surfaces import EX2, _forty, _same_bits

from ballermixplus_amd import _lib, influence, peaks, surfaces
from ballermixplus_amd._lib import BmxError

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _cat(name):
    """The case, its context, the device's own table and cut, and one influence() call per block size over its windows."""
    cat = ic.catalogue(_engine())[name]()
    ctx = cat.context(_engine())
    _, R = ctx.fetch_lut()
    zcut = float(_lib.lib().bmx_alpha_cut())
    return cat, ctx, R, zcut


@functools.lru_cache(maxsize=None)
def _host(name, w, B):
    cat, ctx, R, zcut = _cat(name)
    return cat.host(w, B, R, zcut)


def _window(r, q):
    a, b = int(r['offset'][q]), int(r['offset'][q + 1])
    return {k: r[k][a:b] for k in ('m', 'contrib', 'L', 'blin')}


def _scan_rule(T):
    v, l, _ = influence.scan_argmax(T)
    return v, l


# ------------------------------------------------------------------------------------------------------ exact relations

@pytest.mark.parametrize('name', ic.NAMES)
def test_exact_relations_to_the_surfaces(name):
    cat, ctx, R, zcut = _cat(name)
    T, ns = ctx.surfaces(cat.windows)
    iAmin = int(np.argmin(cat.As))
    untouched = 0
    for B in (1, 3, 64, 10 ** 6):
        r = ctx.influence(cat.windows, B)
        assert len(r['offset']) == len(cat.windows) + 1 and r['offset'][0] == 0
        for q, w in enumerate(cat.windows):
            v, l = _scan_rule(T[q])
            assert r['lin'][q] == l and np.float64(r['T_max'][q]).view(np.uint64) == np.float64(v).view(np.uint64), (B, w)
            assert r['ns_min'][q] == ns[q, iAmin]
            h = _host(name, w, B)
            d = _window(r, q)
            # the block range, the offsets and m_b are the host's, exactly
            assert len(d['m']) == len(h['m']) and np.array_equal(d['m'], h['m']), (B, w)
            assert r['first_block'][q] == h['first_block'] or len(h['m']) == 0
            assert r['ns_min'][q] == h['ns_min'] == d['m'].sum()
            if B == 10 ** 6 and len(d['m']):
                # one block holds the window: its contribution is the whole maximum, bit for bit, and nothing is left
                assert len(d['m']) == 1 and d['L'][0] == 0.0 and d['blin'][0] == -1
                if l >= 0:
                    assert _same_bits(d['contrib'], [T[q].reshape(-1)[l]])
                else:
                    assert np.isnan(d['contrib'][0])
            if l < 0:
                assert np.isnan(d['contrib']).all()
            # a block without a site at every A that has a T > 0 cannot change the maximum
            with np.errstate(invalid='ignore'):
                live = (T[q] > 0).any(axis=(1, 2))
            for j in np.nonzero((h['n_b'][live] == 0).all(axis=0))[0].tolist() if l >= 0 else []:
                assert _same_bits(d['L'][j:j + 1], [v]) and d['blin'][j] == l, (B, w, j)
                untouched += 1
    print('%s: %d blocks out of reach of every A with T > 0' % (name, untouched))
    if name in ('ex1_B2', 'ragged'):
        assert untouched > 0


# --------------------------------------------------------------------------------------------------------- independence

def test_a_window_alone_and_in_a_list_gives_the_same_bits():
    cat, ctx, R, zcut = _cat('ex1_B2')
    M = len(cat.tg)
    tests = _forty(M, 11)
    for B in (3, 64):
        r = ctx.influence(tests, B)
        for q in (0, 1, 2, 17, len(tests) - 3, len(tests) - 1):
            one = ctx.influence([tests[q]], B)
            d, e = _window(r, q), _window(one, 0)
            assert r['first_block'][q] == one['first_block'][0] and r['lin'][q] == one['lin'][0] and r['ns_min'][q] == one['ns_min'][0]
            assert _same_bits(r['T_max'][q:q + 1], one['T_max'])
            assert np.array_equal(d['m'], e['m']) and np.array_equal(d['blin'], e['blin'])
            assert _same_bits(d['L'], e['L']) and _same_bits(d['contrib'], e['contrib'])
        # a repeated index gives the same numbers twice
        for a, b in ((1, 2), (0, len(tests) - 1)):
            assert _same_bits(_window(r, a)['L'], _window(r, b)['L']) and _same_bits(_window(r, a)['contrib'], _window(r, b)['contrib'])
    print('kernels %.3f ms' % ctx.influence_ms())


# ------------------------------------------------------------------------------------------- against the host restatement

@pytest.mark.parametrize('name', ic.NAMES)
def test_against_host_influence(name):
    cat, ctx, R, zcut = _cat(name)
    if name == 'ex1_B2':
        assert len(cat.xs) * len(cat.ab) == 510             # two slices of 256 pairs, the second partial
    if name == 'ex1_B2_fixX_fixAlpha_listA':
        assert len(cat.xs) * len(cat.ab) == 1
    if name == 'edges':
        T, ns = ctx.surfaces([0])
        assert sorted(ns[0].tolist()) == sorted(ic.COUNTS + (0,))
    worst, compared, blocks = 0.0, 0, 0
    for B in ic.BLOCKS:
        r = ctx.influence(cat.windows, B)
        for q, w in enumerate(cat.windows):
            h = _host(name, w, B)
            d = _window(r, q)
            tol = ic.tolerance(h['T'])
            assert np.array_equal(d['m'], h['m']) and (len(h['m']) == 0 or r['first_block'][q] == h['first_block'])
            assert r['lin'][q] == h['lin'] or abs(r['T_max'][q] - h['T_max']) <= tol
            errs = [abs(r['T_max'][q] - h['T_max'])]
            if len(h['m']):
                errs.append(np.max(np.abs(d['L'] - h['L'])))
                if h['lin'] >= 0 and r['lin'][q] == h['lin']:
                    errs.append(np.max(np.abs(d['contrib'] - h['contrib'])))
                sure = h['margin'] > 2 * tol
                assert np.array_equal(d['blin'][sure], h['blin'][sure]), (B, w)
                compared += int(sure.sum())
                blocks += len(sure)
            err = float(max(errs))
            worst = max(worst, err / tol if tol else 0.0)
            assert err <= tol, (B, w, err, tol)
    print('%s: largest error %.3e of the tolerance; lin_b compared on %d of %d blocks' % (name, worst, compared, blocks))
    assert blocks > 0 and compared >= 0.99 * blocks


# ------------------------------------------------------------------------------------------------ against real deletion

def test_against_deleting_the_block_from_the_sites():
    cat, ctx, R, zcut = _cat('ex1_B2')
    w, B = cat.windows[1], 8
    r = ctx.influence([w], B)
    d = _window(r, 0)
    own = np.nonzero(d['m'] > 0)[0]
    drop = int(own[np.argmin(d['L'][own])])
    centre = int(np.searchsorted(cat.gen, cat.tg[w])) // B - int(r['first_block'][0])
    pick = sorted({int(own[0]), int(own[-1]), drop, centre, max(centre - 1, 0)})
    assert len(pick) == 5
    tol = ic.tolerance(ctx.surfaces([w])[0])
    N = len(cat.gen)
    ctx.select_slot(1)
    worst = 0.0
    try:
        for j in pick:
            b = int(r['first_block'][0]) + j
            keep = np.ones(N, dtype=bool)
            keep[b * B:(b + 1) * B] = False
            ctx.set_sites(cat.gen[keep], cat.rows[keep])
            ctx.set_tests(cat.tg[w:w + 1], np.zeros(1, np.int64), np.full(1, keep.sum() - 1, np.int64))      # every site, as the case's windows
            v, l = _scan_rule(ctx.surfaces([0])[0])
            ctx.scan()
            clr = ctx.fetch()[0][0]
            print('block %d: L_b %r, surface without it %r, scan without it %r' % (b, d['L'][j], v, clr))
            assert abs(v - d['L'][j]) <= tol and abs(clr - d['L'][j]) <= tol, (b, v, clr, d['L'][j], tol)
            worst = max(worst, abs(v - d['L'][j]), abs(clr - d['L'][j]))
    finally:
        ctx.select_slot(0)
    assert (cat.lo[w], cat.hi[w]) == (0, N - 1)
    print('largest difference %.3e, tolerance %.3e' % (worst, tol))


# --------------------------------------------------------------------------------------------------------- call hygiene

def test_the_call_leaves_the_slot_as_it_was():
    cat, ctx, R, zcut = _cat('ex1_B2')
    ctx.scan()
    before, sites, rec = ctx.fetch(), ctx.fetch_sites(len(cat.gen)), ctx.fetch_records()
    ctx.influence(_forty(len(cat.tg), 5), 2)
    after, sites2, rec2 = ctx.fetch(), ctx.fetch_sites(len(cat.gen)), ctx.fetch_records()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert all(np.array_equal(a, b) for a, b in zip(sites, sites2)) and rec.tobytes() == rec2.tobytes()
    ctx.scan()
    assert all(np.array_equal(a, b) for a, b in zip(before, ctx.fetch())) and rec.tobytes() == ctx.fetch_records().tobytes()


def test_errors():
    L = _lib.lib()
    one = np.zeros(1, dtype=np.int32)
    assert L.bmx_ctx_influence(None, 1, _lib.as_ip(one), 1) == -1
    assert L.bmx_ctx_influence_ms(None, None) == -1 and L.bmx_ctx_influence_count(None, None, None, None) == -1
    assert L.bmx_ctx_fetch_influence(None, None, None, None, None, None, None, None) == -1
    opt, case, ts, sel = _case_ctx(cases.ALL_CASES['ex1_B2'][0])
    ctx = sel.ctx
    for call in (lambda: ctx.influence([0], 1), ctx.influence_ms):          # model and sites, no test sites yet; no call yet
        with pytest.raises(BmxError) as e:
            call()
        assert e.value.code == -5
    assert L.bmx_ctx_influence_count(ctx._h, None, None, None) == -5
    ctx.set_tests(ts.test_gen, ts.lo, ts.hi)
    M = len(ts)
    assert L.bmx_ctx_influence(ctx._h, -1, _lib.as_ip(one), 1) == -1
    assert L.bmx_ctx_influence(ctx._h, 1, None, 1) == -1
    for bad in ([-1], [M], [0, 5, M, 2], [2, -7]):
        with pytest.raises(BmxError) as e:
            ctx.influence(bad, 1)
        assert e.value.code == -1 and 'index' in str(e.value)
    for B in (0, -3):
        with pytest.raises(BmxError) as e:
            ctx.influence([0], B)
        assert e.value.code == -1 and 'block' in str(e.value)
    with pytest.raises(BmxError) as e:              # a failed call leaves no results behind
        ctx.influence_ms()
    assert e.value.code == -5
    r = ctx.influence([], 1)
    assert len(r['T_max']) == 0 and r['offset'].tolist() == [0] and len(r['L']) == 0
    # the cap, by its arithmetic: one window's blocks, listed often enough
    r = ctx.influence([M // 2], 1)
    per = int(r['offset'][1])
    assert per > 500
    n = influence.MAX_RESULTS // per + 1
    with pytest.raises(BmxError) as e:
        ctx.influence(np.full(n, M // 2, dtype=np.int32), 1)
    assert e.value.code == -4 and 'BMX_INFLUENCE_MAX_RESULTS' in str(e.value)
    r2 = ctx.influence(np.full(3, M // 2, dtype=np.int32), 1)           # well below it: the call works as before
    assert r2['offset'].tolist() == [0, per, 2 * per, 3 * per] and _same_bits(r2['L'][:per], r['L'])
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ CLI

def test_cli_end_to_end(tmp_path):
    plain, inf = str(tmp_path / 'plain.txt'), str(tmp_path / 'inf.txt')
    _cli(EX2 + ['-o', plain, '--peaks', '0.01'])
    r = _cli(EX2 + ['-o', inf, '--peaks', '0.01', '--surfaces', '--influence', '--influenceBlock', '8', '--influenceDetail'])
    assert sorted(os.listdir(tmp_path)) == ['inf.txt', 'inf.txt.influence.blocks.txt', 'inf.txt.influence.txt', 'inf.txt.peaks.txt',
                                            'inf.txt.surfaces.txt', 'plain.txt', 'plain.txt.peaks.txt']
    assert _read(plain) == _read(inf) and _read(peaks.output_name(plain)) == _read(peaks.output_name(inf))
    assert 'Influence: ' in r.stdout and 'blocks of 8 site/s' in r.stdout
    # the same windows through the library
    opt, case, ts, sel = _case_ctx(cases.ALL_CASES['ex2_B2'][0])
    ctx = sel.ctx
    ctx.set_tests(ts.test_gen, ts.lo, ts.hi)
    ctx.scan()
    clr, _, _, iA, _ = ctx.fetch()
    pk = ctx.peaks(0.01, 0.0, peaks.FRAC)
    rows, dropped = surfaces.select(clr, iA, 0.0, pk['row'], influence.MAX_WINDOWS)
    assert len(rows) >= 1 and dropped == 0
    res = ctx.influence(rows, 8)
    phys, gen = surfaces.labels(ts, rows.tolist())
    with open(influence.output_name(inf)) as f:
        lines = f.readlines()
    with open(influence.blocks_name(inf)) as f:
        blines = f.readlines()
    assert lines[0] == influence.HEADER and blines[0] == influence.BLOCKS_HEADER and len(lines) == len(rows) + 1
    main = {tuple(l.split('\t')[:2]): l.split('\t') for l in open(inf).readlines()[1:]}
    want_blocks = []
    for q in range(len(rows)):
        d = _window(res, q)
        s = influence.summarise(float(res['T_max'][q]), int(res['lin'][q]), int(res['first_block'][q]), d['m'], d['contrib'], d['L'], d['blin'])
        want = influence.summary_row(phys[q], gen[q], repr(float(clr[rows[q]])), res['T_max'][q], s, case.data.position, 8, sel)
        assert lines[q + 1] == want
        assert lines[q + 1].split('\t')[:3] == main[(phys[q], gen[q])][:3]              # the main output's strings
        want_blocks += influence.block_rows(phys[q], gen[q], res['first_block'][q], d['m'], d['contrib'], d['L'], d['blin'], case.data.position, 8, sel)
    assert blines[1:] == want_blocks and len(want_blocks) == int((res['m'] > 0).sum())
    # T_max is the maximum of the window's block of the surfaces file
    layout = surfaces.Layout(sel.grid_A, sel.grid_x, sel.grid_abeta)
    p2, g2, Tf, nf = surfaces.read_surfaces(surfaces.output_name(inf), layout)
    assert p2 == phys and g2 == gen
    for q in range(len(rows)):
        assert float(lines[q + 1].split('\t')[3]) == np.nanmax(Tf[q]) == res['T_max'][q]
    ctx.close()
