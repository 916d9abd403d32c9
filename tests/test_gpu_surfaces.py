"""Likelihood surfaces of a list of windows on the GPU (--surfaces): bmx_ctx_surfaces against bmx_ctx_surface -- bit for bit, that
is the contract -- on the example inputs and on a chromosome built around the kernel's tile and range edges, against the host
restatement and the reference's own surfaces, what the call leaves untouched, its errors, and the CLI end to end."""
import glob
import os

import numpy as np
import pytest

import cases
from test_gpu_refine import _case_ctx, _cli, _engine, _read
from util import GOLD, REFT

from ballermixplus_amd import peaks, surfaces
from ballermixplus_amd._lib import BmxError

pytestmark = pytest.mark.gpu

EX1 = ['-i', os.path.join(REFT, 'Example1_fullSweep_200kya_DAF.txt'), '--spect', os.path.join(REFT, 'HC_CEU_Neut_DAF_spect_for_B2.txt')]
EX2 = ['-i', os.path.join(REFT, 'Example2_balancing_10MYA_DAF.txt'), '--spect', os.path.join(REFT, 'HC_CEU_Neut_DAF_spect_for_B2.txt')]


def _same_bits(a, b):
    """Equal shapes, NaN at the same places, every other value the same 64 bits."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))


def _check_against_single(ctx, tg, lo, hi, tests, what):
    """One surfaces() call over `tests` against surface() of each: bitwise.  Returns (T, ns)."""
    T, ns = ctx.surfaces(tests)
    assert T.dtype == np.float64 and ns.dtype == np.int32 and T.shape[0] == ns.shape[0] == len(tests)
    for q, t in enumerate(tests):
        T1, n1 = ctx.surface(tg[t], lo[t], hi[t])
        assert np.array_equal(ns[q], n1), (what, q, t, ns[q], n1)
        assert _same_bits(T[q], T1), (what, q, t)
        assert np.array_equal(np.isnan(T[q]).all(axis=(1, 2)), n1 == 0) and not np.isnan(T[q][n1 > 0]).any(), (what, q, t)
    return T, ns


def _forty(M, seed):
    """About 40 test sites of M: the first and the last, unsorted, one index repeated."""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, M, 36).tolist()
    return [M - 1, pick[0]] + pick + [0, pick[0], M - 1]


# ------------------------------------------------------------------------------------------- bitwise, on the examples

@pytest.mark.parametrize('name,pairs', [('ex1_B2', 510), ('ex2_B2maf_findBal', None), ('ex1_B1', None), ('ex1_B2_fixX_fixAlpha_listA', 1),
                                        ('ex1_B2_w50_s25', None), ('ex2_B0_noCenter_2kb', None)])
def test_bitwise_equal_to_single_surfaces_on_the_examples(name, pairs):
    opt, case, ts, sel = _case_ctx(cases.ALL_CASES[name][0])
    ctx = sel.ctx
    if pairs is not None:           # two slices, the second partial / one pair: a slice with 255 idle threads
        assert len(case.xs) * len(case.abetas) == pairs
    ctx.set_tests(ts.test_gen, ts.lo, ts.hi)
    tests = _forty(len(ts), 11)
    T, ns = _check_against_single(ctx, ts.test_gen, ts.lo, ts.hi, tests, name)
    assert T.shape[1:] == (len(case.As), len(case.xs), len(case.abetas))
    assert (ns > 0).any()
    # a repeated index gives the same surface twice
    assert _same_bits(T[1], T[2]) and _same_bits(T[0], T[-1])
    print('%s: %d windows, kernels %.3f ms' % (name, len(tests), ctx.surfaces_ms()))
    ctx.close()


def test_bitwise_equal_with_several_sample_sizes_and_ragged_windows():
    """A model with three sample sizes (the table's rows of three blocks), exact position ties, off-site and duplicated test
    positions, windows that are empty, clipped or do not contain the test position, tiny and huge A."""
    eng = _engine()
    from ballermixplus_amd.hostmodel import Grids
    rng = np.random.default_rng(77)
    N, sizes = 1500, (12, 33, 50)
    scale = 3e-6
    gen = np.sort(np.round(np.cumsum(rng.geometric(0.2, N)).astype(np.float64) / 3) * 3 * scale)
    nn = rng.choice(np.array(sizes), N)
    k = np.array([rng.integers(1, h + 1) for h in nn])
    cnt = {}
    for a, b in zip(k.tolist(), nn.tolist()):
        cnt[(a, b)] = cnt.get((a, b), 0) + 1
    spect = {key: v / N for key, v in cnt.items()}
    props = {int(n): sum(v for (a, b), v in spect.items() if b == n) for n in sizes}
    xs, ab, As = Grids(None, None, False, False, None, '3.5,200.0,1500,40000.0,1e6,1e8,7e8').scan_order()
    model = eng.ModelArrays('B2', 1, sizes, spect, props, xs, ab)
    ctx = eng.Context(0)
    ctx.set_model(model, As)
    ctx.set_sites(gen, model.rows_of(k, nn))
    tg = gen[::7].copy()
    tg[::5] += scale * 0.37
    tg = np.sort(np.concatenate([tg, tg[:5]]))
    M = len(tg)
    c = np.searchsorted(gen, tg)
    lo = np.maximum(c - 150, 0).astype(np.int64)
    hi = np.minimum(c + 151, N - 1).astype(np.int64)
    lo[::4] = np.minimum(lo[::4] + rng.integers(0, 300, len(lo[::4])), N - 1)     # ragged: sometimes empty, sometimes past the test site
    hi[1::4] = np.maximum(hi[1::4] - rng.integers(0, 300, len(hi[1::4])), 0)
    lo[2], hi[2] = -5, 10 * N                                                      # bounds beyond the chromosome are clipped
    ctx.set_tests(tg, lo, hi)
    tests = _forty(M, 3) + [2] + np.nonzero(hi < lo)[0][:3].tolist()
    T, ns = _check_against_single(ctx, tg, lo, hi, tests, 'multi-n')
    assert (ns == 0).any() and (ns > 250).any() and np.isnan(T).any()
    ctx.close()


# ------------------------------------------------------------------------------------------------ tile and range edges

COUNTS = (0, 1, 255, 256, 257, 512, 513)


def _edge_chromosome():
    """700 sites around the off-site position 1.0, alternating sides at distinct distances, and three more sites at one
    position far out.  Returns (gen, tX, tY, the A grid, the distances of the sites from tX, ascending)."""
    h = 5e-5
    j = np.arange(350, dtype=np.float64)
    left, right = 1.0 - (2 * j + 1) * h, 1.0 + (2 * j + 2) * h
    tY = float(right[300])
    gen = np.sort(np.concatenate([left, right, [tY, tY]]))
    tX = 1.0
    assert not (gen == tX).any() and (gen == tY).sum() == 3
    d = np.sort(np.abs(gen - tX))
    assert len(np.unique(d[:520])) == 520
    return gen, tX, tY, d


def _A_for_count(d, K, zcut):
    """An A at which exactly the K nearest sites have A * d <= zcut, the boundary as tight as doubles allow: the largest such A."""
    if K == 0:
        A = zcut / d[0]
        while A * d[0] <= zcut:
            A = np.nextafter(A, np.inf)
        return float(A)
    A = zcut / d[K - 1]
    while A * d[K - 1] > zcut:
        A = np.nextafter(A, 0.0)
    while np.nextafter(A, np.inf) * d[K - 1] <= zcut:
        A = np.nextafter(A, np.inf)
    assert A * d[K - 1] <= zcut < A * d[K]
    return float(A)


def test_tile_and_range_edges():
    eng = _engine()
    from ballermixplus_amd import _lib
    from ballermixplus_amd.hostmodel import Grids
    zcut = float(_lib.lib().bmx_alpha_cut())
    assert 18.4 < zcut < 18.5
    gen, tX, tY, d = _edge_chromosome()
    N = len(gen)
    As = [_A_for_count(d, K, zcut) for K in COUNTS]
    order = [3, 0, 6, 2, 5, 1, 4]                          # a --listA grid in no particular order
    As = [As[i] for i in order] + [1e8]
    rng = np.random.default_rng(4)
    n = 20
    k = rng.integers(1, n + 1, N)
    cnt = {}
    for a in k.tolist():
        cnt[(a, n)] = cnt.get((a, n), 0) + 1
    spect = {key: v / N for key, v in cnt.items()}
    xs, ab, _ = Grids(None, None, False, False, None, None).scan_order()
    model = eng.ModelArrays('B2', 1, [n], spect, {n: 1.0}, xs, ab)
    rows = model.rows_of(k, np.full(N, n))
    ctx = eng.Context(0)
    ctx.set_model(model, As)
    ctx.set_sites(gen, rows)
    iY = int(np.searchsorted(gen, tY))
    # test sites: the off-site position over the whole chromosome; the triple's position; the off-site position in a window that
    # cuts the range on both sides; the triple's position in a window that holds the triple alone; an empty window
    tg = np.array([tX, tX, tY, tY, tY])
    lo = np.array([0, 340, 0, iY, 20], dtype=np.int64)
    hi = np.array([N - 1, 361, N - 1, iY + 2, 19], dtype=np.int64)
    ctx.set_tests(tg, lo, hi)
    T, ns = _check_against_single(ctx, tg, lo, hi, [0, 1, 2, 3, 4], 'edges')
    assert ns[0].tolist() == [COUNTS[i] for i in order] + [0]
    assert ns[1].max() == 22 and ns[3].tolist() == [0] * 8 and ns[4].tolist() == [0] * 8
    _, R = ctx.fetch_lut()
    for q in range(5):
        Th, nh = surfaces.host_surface(gen, rows, R, As, tg[q], lo[q], hi[q], zcut)
        assert np.array_equal(ns[q], nh), (q, ns[q], nh)
        assert np.array_equal(np.isnan(T[q]), np.isnan(Th))
        assert np.array_equal(np.isnan(T[q]).all(axis=(1, 2)), nh == 0)
        if (nh > 0).any():
            err = np.nanmax(np.abs(T[q] - Th)) / np.nanmax(np.abs(Th))
            print('window %d: nsites %s, max |dT| / max |T| = %.2e' % (q, nh.tolist(), err))
            assert err < 1e-9, (q, err)
    # the triple: inside the range at every A (distance 0), never counted
    assert ns[2].tolist() == [int((A * np.abs(gen - tY) <= zcut).sum()) - 3 for A in As]
    ctx.close()


# ------------------------------------------------------------------------------------------------- reference surfaces

SURF = sorted(glob.glob(os.path.join(GOLD, 'surface_*.npz')))


@pytest.mark.parametrize('path', SURF, ids=[os.path.basename(p)[8:-4] for p in SURF])
def test_surfaces_match_reference(path):
    """test_device_likelihood_surface_matches_reference's assertions and tolerances on bmx_ctx_surfaces."""
    z = np.load(path)
    key = 'ex1_B2' if 'ex1_B2' in os.path.basename(path) else 'ex2_B2maf_findBal'
    opt, case, ts, sel = _case_ctx(cases.ALL_CASES[key][0])
    ctx = sel.ctx
    s = int(z['site'])
    assert ts.test_gen[s] == case.data.genPos[s] and (ts.lo[s], ts.hi[s]) == (0, case.data.numSites - 1)
    ctx.set_tests(ts.test_gen, ts.lo, ts.hi)
    ctx.scan()
    clr, ix, ia, iA, n = ctx.fetch()
    Ts, nss = ctx.surfaces([s, 5, s])
    T, ns = Ts[2], nss[2]
    ref = z['T']
    pos = ~np.isnan(ref)                         # the reference reports a value only where T > 0
    assert np.all((T[~pos] <= 0) | np.isnan(T[~pos]))
    assert np.max(np.abs(T[pos] - ref[pos]) / np.abs(ref[pos])) < 1e-9
    has = pos.any(axis=(1, 2))
    assert np.array_equal(ns[has], z['nsites'][has])
    flat = np.where(np.isnan(T), -np.inf, T).reshape(-1)
    best = int(np.argmax(flat))                  # first maximum in (A, x, a) order
    assert flat[best] > 0 and abs(clr[s] - flat[best]) <= 1e-12 * flat[best]
    nx, nab = len(case.xs), len(case.abetas)
    assert (int(iA[s]), int(ix[s]), int(ia[s])) == (best // (nx * nab), (best // nab) % nx, best % nab)
    # the maximum is attained once, so the first maximal row of the file's ascending order names the same grid point
    assert (flat == flat[best]).sum() == 1
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- state

def test_state_slots_and_errors():
    opt, case, ts, sel = _case_ctx(cases.ALL_CASES['ex1_B2'][0])
    ctx = sel.ctx
    M = len(ts)
    with pytest.raises(BmxError) as e:           # model and sites, no test sites yet
        ctx.surfaces([0])
    assert e.value.code == -5
    with pytest.raises(BmxError) as e:
        ctx.surfaces_ms()
    assert e.value.code == -5
    ctx.set_tests(ts.test_gen, ts.lo, ts.hi)
    T0, n0 = ctx.surfaces([3, M - 1])            # needs no scan
    ctx.scan()
    before = ctx.fetch()
    pk = ctx.peaks(0.005, 10.0)
    ctx.refine(0.0)
    refined = ctx.fetch_refined()
    T, ns = ctx.surfaces([3, M - 1] + pk['row'].tolist())
    assert _same_bits(T[:2], T0) and np.array_equal(ns[:2], n0)
    after = ctx.fetch()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    pk2 = ctx.fetch_peaks()
    assert all(np.array_equal(pk[f], pk2[f]) for f in peaks.FIELDS)
    still = ctx.fetch_refined()                  # the refinement made before the call is still there ...
    ctx.refine(0.0)                              # ... and one made after it gives the same
    again = ctx.fetch_refined()
    for f in refined:
        assert np.array_equal(refined[f], still[f], equal_nan=True) and np.array_equal(refined[f], again[f], equal_nan=True), f
    # the errors; a failed call leaves everything as it was
    for bad in ([-1], [M], [0, 5, M, 2], [2, -7]):
        with pytest.raises(BmxError) as e:
            ctx.surfaces(bad)
        assert e.value.code == -1 and 'index' in str(e.value)
    Te, ne = ctx.surfaces([])
    assert Te.shape == (0,) + T.shape[1:] and ne.shape == (0, T.shape[1])
    assert all(np.array_equal(a, b) for a, b in zip(before, ctx.fetch()))
    # a second slot with other sites and test sites: the call reads the selected one
    ctx.select_slot(1)
    half = case.data.numSites // 2
    ctx.set_sites(case.data.genPos[:half], sel.rows[:half])
    tg1 = np.asarray(ts.test_gen[:half:3])
    lo1, hi1 = np.zeros(len(tg1), np.int64), np.full(len(tg1), half - 1, np.int64)
    ctx.set_tests(tg1)
    with pytest.raises(BmxError):
        ctx.surfaces([len(tg1)])
    T1, n1 = _check_against_single(ctx, tg1, lo1, hi1, [len(tg1) - 1, 1], 'slot 1')
    ctx.select_slot(0)
    Tb, nb = ctx.surfaces([3, M - 1])
    assert _same_bits(Tb, T0) and np.array_equal(nb, n0) and not _same_bits(Tb[1], T1[0])
    assert all(np.array_equal(a, b) for a, b in zip(before, ctx.fetch()))
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ CLI

def _blocks(path, layout):
    with open(path) as f:
        lines = f.readlines()
    assert lines[0] == surfaces.HEADER
    rows = [l.rstrip('\n').split('\t') for l in lines[1:]]
    assert len(rows) % layout.points == 0 and all(len(r) == 7 for r in rows)
    return [rows[i:i + layout.points] for i in range(0, len(rows), layout.points)]


def _main_rows(path):
    with open(path) as f:
        return [l.rstrip('\n').split('\t') for l in f.readlines()[1:]]


def _check_blocks_against_main(blocks, main_of, layout):
    """Every block against its row of the main output: the first two columns, nSites per A, and the first maximal T of the
    block -- in the scan's iteration order, the reference's first-maximum rule -- names x_hat, s_hat, A_hat and is the CLR."""
    nA, nx, nab = layout.shape
    # position of every ascending-order row in the scan's iteration order
    it = np.empty(layout.shape, dtype=np.int64)
    for a, iA in enumerate(layout.oA):
        for b, ix in enumerate(layout.ox):
            for c, ia in enumerate(layout.oab):
                it[a, b, c] = (iA * nx + ix) * nab + ia
    it = it.reshape(-1)
    for block, m in zip(blocks, main_of):
        assert all(r[:2] == m[:2] for r in block)
        vals = np.array([-np.inf if r[5] == 'NA' else float(r[5]) for r in block])
        top = vals.max()
        first_asc = int(np.argmax(vals))
        first_it = int(np.argmin(np.where(vals == top, it, it.max() + 1)))
        for first in {first_asc, first_it} if (vals == top).sum() == 1 else {first_it}:
            r = block[first]
            assert [r[3], r[4], r[2], r[6]] == m[3:7], (r, m)
        clr = float(m[2])
        assert top > 0 and abs(clr - top) <= 1e-12 * top, (clr, top)
        assert all(r[5] == repr(float(r[5])) for r in block if r[5] != 'NA')
        assert all((r[5] == 'NA') == (r[6] == '0') for r in block)


def test_cli_surfaces_of_the_apexes(tmp_path):
    plain, sf = str(tmp_path / 'plain.txt'), str(tmp_path / 'sf.txt')
    flags = ['--peaks', '0.0002', '--peakMin', '5']             # (Example 1 spans 0.001 in genPos)
    _cli(EX1 + ['-o', plain] + flags)
    r = _cli(EX1 + ['-o', sf] + flags + ['--surfaces'])
    assert sorted(os.listdir(tmp_path)) == ['plain.txt', 'plain.txt.peaks.txt', 'sf.txt', 'sf.txt.peaks.txt', 'sf.txt.surfaces.txt']
    assert _read(plain) == _read(sf) and _read(peaks.output_name(plain)) == _read(peaks.output_name(sf))
    assert 'Surfaces: ' in r.stdout and 'dropped' not in r.stdout
    opt, case, ts, sel = _case_ctx(cases.ALL_CASES['ex1_B2'][0])
    layout = surfaces.Layout(sel.grid_A, sel.grid_x, sel.grid_abeta)
    blocks = _blocks(surfaces.output_name(sf), layout)
    apex = _main_rows(peaks.output_name(sf))
    assert len(blocks) == len(apex) >= 2
    main = {tuple(m[:2]): m for m in _main_rows(sf)}
    _check_blocks_against_main(blocks, [main[tuple(a[:2])] for a in apex], layout)
    assert [b[0][:2] for b in blocks] == [a[:2] for a in apex]
    # the file read back is ctx.surfaces of the same windows, exactly
    ctx = sel.ctx
    ctx.set_tests(ts.test_gen, ts.lo, ts.hi)
    where = {str(p): j for j, p in enumerate(ts.arrays[0].tolist())}
    rows = [where[a[0]] for a in apex]
    T, ns = ctx.surfaces(rows)
    phys, gen, Tf, nf = surfaces.read_surfaces(surfaces.output_name(sf), layout)
    assert _same_bits(Tf, layout.ascending(T)) and np.array_equal(nf, ns[:, layout.oA])
    assert phys == [a[0] for a in apex] and gen == [a[1] for a in apex]
    ctx.close()


def test_cli_surfaces_by_threshold_and_cap(tmp_path):
    out = str(tmp_path / 'o.txt')
    r = _cli(EX1 + ['-o', out, '-s', '3', '--surfaces', '--surfaceMin', '20', '--surfaceMax', '3'])
    main = _main_rows(out)
    ok = [j for j, m in enumerate(main) if m[5] not in ('NA', '0.0') and float(m[2]) >= 20.0]
    assert len(ok) > 3
    keep = sorted(sorted(ok, key=lambda j: (-float(main[j][2]), j))[:3])
    assert '%d more window/s qualified and were dropped' % (len(ok) - 3) in r.stdout
    opt, case, ts, sel = _case_ctx(cases.ALL_CASES['ex1_B2'][0])
    sel.ctx.close()
    layout = surfaces.Layout(sel.grid_A, sel.grid_x, sel.grid_abeta)
    blocks = _blocks(surfaces.output_name(out), layout)
    assert [b[0][:2] for b in blocks] == [main[j][:2] for j in keep]
    _check_blocks_against_main(blocks, [main[j] for j in keep], layout)
    # a threshold above every CLR: the header only
    _cli(EX1 + ['-o', out, '-s', '3', '--surfaces', '--surfaceMin', '1e9'])
    assert _read(surfaces.output_name(out)) == surfaces.HEADER.encode()


def test_cli_two_files(tmp_path):
    d1, d2 = tmp_path / 'plain', tmp_path / 'sf'
    ins = EX1[1] + ',' + EX2[1]
    flags = ['-s', '2', '--peaks', '0.005', '--peakMin', '10']
    _cli(['-i', ins, '--spect', EX1[3], '-o', str(d1)] + flags)
    _cli(['-i', ins, '--spect', EX1[3], '-o', str(d2)] + flags + ['--surfaces', '--surfaceMin', '15'])
    outs = sorted(os.listdir(d1))
    assert sorted(f for f in os.listdir(d2) if not f.endswith('.surfaces.txt')) == outs
    for f in outs:
        assert _read(d1 / f) == _read(d2 / f), f
    opt, case, ts, sel = _case_ctx(cases.ALL_CASES['ex1_B2'][0])
    sel.ctx.close()
    layout = surfaces.Layout(sel.grid_A, sel.grid_x, sel.grid_abeta)
    for name in (EX1[1], EX2[1]):
        path = str(d2 / (os.path.basename(name) + '.out.txt'))
        apex = [a for a in _main_rows(peaks.output_name(path)) if float(a[2]) >= 15.0]
        blocks = _blocks(surfaces.output_name(path), layout)
        assert len(blocks) == len(apex) >= 1 and [b[0][:2] for b in blocks] == [a[:2] for a in apex]
        main = {tuple(m[:2]): m for m in _main_rows(path)}
        _check_blocks_against_main(blocks, [main[tuple(a[:2])] for a in apex], layout)
