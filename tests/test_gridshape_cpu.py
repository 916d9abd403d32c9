"""The inputs of tests/test_gpu_grid_shapes.py really have the slice counts, pad lanes and chunk counts they are meant to have, are
free of near-ties between distinct grid points, hold windows without a winner, and the tie grids tie exactly -- shown with the
oracles alone (the C oracle's table, scan and per-grid-point sums), so that the GPU tests cannot pass by never meeting these cases.
Every test prints the measured figures."""
import functools
import os
import re

import numpy as np
import pytest

import gridshape as gs
from util import REPO, c_oracle, c_scan, c_sel_table

SMALL_CASES = [('small', shape, stride, w) for shape in gs.SHAPES for stride in gs.STRIDES for w in ('all', 'ragged')]
LARGE_CASES = [('large', shape, stride, 'all') for shape in gs.L2_SHAPES for stride in (1, 5)]
TIE_CASES = [('small', 'tie', stride, w) for stride in gs.STRIDES for w in ('all', 'ragged')] + [('large', 'tie', stride, 'all') for stride in (1, 5)]


@functools.lru_cache(maxsize=4)
def _table(data, kind):
    """The oracle's own table for a shape or the tie grid."""
    xs, ab, _ = gs.grids(kind)
    psel = np.concatenate([c_sel_table(c_oracle(), 'B2', n, 1, xs, ab) for n in gs.sizes_of(data)], axis=2)
    return gs.table_from(psel, data)


@functools.lru_cache(maxsize=None)
def _sites(data):
    gen, k, nn = gs.chromosome(data)
    return gen, k, nn, gs.rows_of(data)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_shapes_are_what_the_table_says():
    assert len(gs.SHAPES) == 11 and set(gs.SHAPE_FACTS) == set(gs.SHAPES)
    for shape in gs.SHAPES:
        xs, ab, As = gs.grids_of(shape)
        npairs = len(xs) * len(ab)
        nslices = -(-npairs // gs.WAVE)
        last = npairs - (nslices - 1) * gs.WAVE
        assert (len(xs), len(ab)) == shape and (npairs, nslices, last) == gs.SHAPE_FACTS[shape], shape
        assert len(set(xs)) == len(xs) and all(0 < v < 1 for v in xs) and len(set(ab)) == len(ab)
        assert min(xs) >= gs.X_RANGE[0] and max(xs) <= gs.X_RANGE[1] and min(ab) >= gs.ABETA_RANGE[0] and max(ab) <= gs.ABETA_RANGE[1] * (1 + 1e-12)
        if len(ab) > 2:
            assert np.allclose(np.diff(np.log(ab)), np.log(ab[1] / ab[0]))                  # log-spaced
            assert ab[0] == pytest.approx(gs.ABETA_RANGE[0]) and ab[-1] == pytest.approx(gs.ABETA_RANGE[1])
        assert As == list(gs.A_LIST) and 4 <= len(As) <= 6
    facts = sorted(gs.SHAPE_FACTS.values())
    assert [f[0] for f in facts] == [10, 51, 63, 64, 64, 65, 128, 129, 576, 1024, 1037]
    assert {f[1] for f in facts} == {1, 2, 3, 9, 16, 17}
    assert gs.SHAPE_FACTS[(5, 13)][2] == 1 and gs.SHAPE_FACTS[(3, 43)][2] == 1 and gs.SHAPE_FACTS[(17, 61)][2] == 13
    assert 64 % 13 and 64 % 43 and 64 % 61                                                  # nab does not divide the slice
    # (17, 61): the pairs of some x value straddle two slices
    assert any((ix * 61) // 64 != (ix * 61 + 60) // 64 for ix in range(17))
    from ballermixplus_amd.hostmodel import Grids
    assert (min(Grids.DEFAULT_ABETA), max(Grids.DEFAULT_ABETA)) == gs.ABETA_RANGE
    d = Grids(None, None, False, False, None, None)
    assert (min(d.x), max(d.x)) == pytest.approx(gs.X_RANGE)
    fx, fa = Grids('0.3', None, False, False, None, None).scan_order(), Grids(None, 7.0, False, False, None, None).scan_order()
    assert (len(fx[0]), len(fx[1]), len(fa[0]), len(fa[1])) == (1, 51, 10, 1)              # the CLI's --fixX and --fixAlpha shapes


def test_test_sites_fill_more_than_eight_chunks():
    figures = {}
    for stride in gs.STRIDES:
        t = gs.tests_of(stride)
        assert np.all(np.diff(t) == stride) and t[0] >= 0 and t[-1] < gs.N
        for lds in (True, False):
            M, J, spb, chunks, padded, last = gs.chunks_of(stride, lds)
            assert M == len(t) and chunks > 8 and M % spb != 0 and padded > chunks and padded % 8 == 0
            assert last != 0 and (J == 0 or last < J)                                       # a partial last group
            figures[(stride, lds)] = (M, J, spb, chunks, padded, last)
    print('(stride, table in LDS) -> (test sites, J, test sites per workgroup, chunks, chunks launched, test sites of the last group): %r' % figures)
    dense = gs.tests_of(1)
    (a, b), = gs.LOW
    assert dense[0] < a - 100 and dense[-1] > b + 100                                       # the dense run covers the stretch and both sides
    gen, k, nn, row = _sites('small')
    for j in gs.POS_TIES:
        assert gen[j + 1] == gen[j]
    assert np.all(np.diff(gen) >= 0) and int(np.sum(np.diff(gen) == 0)) == len(gs.POS_TIES)
    wide = {A: [len(gs.window_of(gen, i, A)[0]) for i in (0, 2000, gs.N - 1)] for A in gs.A_LIST}
    print('window sizes of the sites 0 / 2000 / N - 1 per A: %r' % wide)
    assert wide[gs.A_LIST[0]][1] == gs.N - 1 and 20 < wide[gs.A_LIST[-1]][1] < 64


def test_spb_literals_still_match_the_source():
    """The workgroup sizes gridshape.SPB was read off, by plain text match on plan_scan: a change there flags this suite."""
    with open(os.path.join(REPO, 'ballermixplus_amd', 'csrc', 'bmxscan.hip')) as f:
        src = f.read()
    want = [
        r'int spb = J \? \(s->M >= 65536 \? 128 : 4 \* J\) : \(s->M >= 65536 \? 32 : SITE_THREADS / WAVE\);',
        r'if \(J == 16 && spb < 64\) spb = 64;',
        r'spb = spb \* 3;',
        r'constexpr int SITE_THREADS = 1024;',
        r'constexpr int WAVE = 64;',
        r'blocks = \(\(cnt \+ pl\.spb - 1\) / pl\.spb \+ 7\) / 8 \* 8 \* c->nslices;',
        r'const int slice = \(int\)\(q % P\.nslices\);',
        r'c->nslices = c->NP / WAVE;',
    ]
    for pat in want:
        assert re.search(pat, src), pat
    assert gs.SPB == {1: (16, 64, 64), 5: (8, 96, 32), 20: (0, 1024 // 64, 1024 // 64)}


def test_data_sets():
    for data in ('small', 'large'):
        gen, k, nn, row = _sites(data)
        spect, props = gs.spectrum(data)
        assert len(gen) == gs.N and k.min() >= 1 and np.all(k <= nn) and sorted(set(nn.tolist())) == gs.sizes_of(data)
        assert all((int(a), int(b)) in spect for a, b in zip(k, nn))                       # every site's row has a neutral probability
        rows = sum(n + 1 for n in gs.sizes_of(data))
        assert row.max() < rows and (rows == 21 if data == 'small' else rows == 483 and rows * 64 * 8 > 160 * 1024)
        (a, b), = gs.LOW
        assert np.all(k[a:b] == gs.LOW_K) and np.all(nn[a:b] == gs.sizes_of(data)[0])
        R = _table(data, (5, 13))
        low = R[:, :, gs.row_offsets(data)[gs.sizes_of(data)[0]] + gs.LOW_K]
        print('%s: R of the stretch row %.4f .. %.4f; R elsewhere %.3f .. %.3f' % (data, low.min(), low.max(), R.min(), np.delete(R, row[a], axis=2).max()))
        assert low.max() < -0.5 and R.min() >= -1.0                            # (exactly -1 where P_sel underflows at n = 150: 1 + alpha R = 1 - alpha > 0)


def test_tie_layout():
    """The duplicate classes are where the module says they are."""
    xs, ab, As = gs.TIE_GRIDS
    nx, nab = gs.TIE_SHAPE
    npairs = nx * nab
    assert (nx, nab, npairs, len(As)) == (7, 13, 91, 6) and -(-npairs // 64) == 2
    cls = gs.class_of()
    val = lambda lin: (As[lin // npairs], xs[(lin // nab) % nx], ab[lin % nab])
    for lin in range(len(cls)):
        assert cls[lin] <= lin and val(lin) == val(cls[lin])
    assert len(set(val(c) for c in set(cls.tolist()))) == len(set(cls.tolist())) == 3 * 5 * 11     # the base grid is distinct
    m = lambda p: [int(v) for v in gs.members_of(p) if v < npairs]
    assert m(5) == [5, 11, 83, 89] and m(4) == [4, 12, 82, 90] and m(18) == [18, 24, 70, 76] and m(17) == [17, 25, 69, 77] and m(14) == [14, 66]
    assert m(56) == [56, 64] and m(57) == [57, 63] and m(0) == [0, 78] and m(31) == [31, 37]
    assert gs.members_of(14).tolist() == [14, 66, 14 + 3 * 91, 66 + 3 * 91]                # every A twice, three apart
    a, b = gs.TIE_CLASSES['same slice']
    assert a // 64 == b // 64
    for name in ('across, first copy in the higher lane', 'across, last lanes and first lane'):
        a, b = gs.TIE_CLASSES[name]
        assert a < b and a // 64 == 0 and b // 64 == 1 and a % 64 > b % 64
    assert all(abs(i - j) > 1 for i in range(6) for j in range(i + 1, 6) if As[i] == As[j]) and all(As.count(v) == 2 for v in As)
    for data in ('small', 'large'):
        R = _table(data, 'tie')
        for ix in range(nx):
            for ia in range(nab):
                p0 = int(cls[ix * nab + ia])
                assert np.array_equal(_bits(R[ix, ia]), _bits(R[p0 // nab, p0 % nab])), (ix, ia)
        flat = R.reshape(npairs, -1)
        assert len(np.unique(flat, axis=0)) == 5 * 11


def _case(data, kind, stride, windows):
    gen, k, nn, row = _sites(data)
    R = _table(data, kind)
    As = gs.grids(kind)[2]
    idx = gs.tests_of(stride)
    lo, hi = gs.windows_of(gen, idx, windows)
    S, ns = gs.surface_sums(c_oracle(), R, As, gen, row, gen[idx], lo, hi)
    # orc_scan itself, for the cross-check of decide(): everywhere but the three large shapes with whole-chromosome windows at the
    # strides 1 and 5 (the same sums twice, most of this file's run time)
    scan = c_scan(c_oracle(), R, As, gen, row, gen[idx], lo, hi) if (R.shape[0] * R.shape[1] < 512 or windows == 'ragged' or stride == 20) else None
    return R, As, idx, lo, hi, S, ns, scan


def _common(data, kind, stride, windows, S, ns, scan, idx, lo, hi, classes=None):
    nx, nab = gs.TIE_SHAPE if kind == 'tie' else kind
    best, lin, lead, tied = gs.decide(S, ns, classes)
    none = (lin < 0)
    clr = np.where(none, 0.0, best)
    nsb = np.where(none, 0, ns[np.arange(len(idx)), np.maximum(lin, 0) // (nx * nab)])
    if scan is not None:
        # the sums tell the same story as orc_scan: same first maximum, same T, same nSites; no winner: iA = ix = ia = -1, CLR 0, nSites 0
        assert np.array_equal(lin, np.where(scan[3] >= 0, (scan[3] * nx + scan[1]) * nab + scan[2], -1))
        assert np.array_equal(_bits(clr), _bits(scan[0])) and np.array_equal(nsb, scan[4])
        assert np.all(scan[1][none] == -1) and np.all(scan[2][none] == -1) and np.all(scan[3][none] == -1)
    nonempty_none = int(np.sum(none & (ns.max(axis=1) > 0)))
    listed = list(gs.TIED.get((data, kind, stride, windows), ()))
    found = np.nonzero(tied)[0].tolist()
    w = ~none
    print('%s %s stride %d %s: %d windows (%d empty, %d non-empty without a winner), nSites %d .. %d, CLR %.3g .. %.3g, smallest lead %.3e relative, '
          '%.3e absolute; below the bar: %r' % (data, kind, stride, windows, len(idx), int(np.sum(ns.max(axis=1) == 0)), nonempty_none, nsb[w].min(), nsb.max(),
                                               clr[w].min(), clr.max(), np.min(lead[w & ~tied] / best[w & ~tied]), np.min(lead[~tied]), found))
    assert found == listed, (data, kind, stride, windows, found, lead[tied], best[tied])
    assert len(found) <= 0.02 * len(idx)
    assert nonempty_none >= 5
    if windows == 'ragged':
        assert np.any(lo > hi) and np.any(lo > idx) and np.any(ns.max(axis=1) == 0)
    return best, lin, lead, tied


@pytest.mark.parametrize('data,shape,stride,windows', SMALL_CASES + LARGE_CASES)
def test_no_near_ties_and_windows_without_a_winner(data, shape, stride, windows):
    """Every compared window: the oracle's best grid point leads every other grid point, and T = 0, by more than gridshape.TIE_BAR of
    its T (and by more than gridshape.ABS_BAR); the windows that do not are listed in gridshape.TIED, at most 2 % of the case.  At
    least five non-empty windows have no grid point with T > 0."""
    R, As, idx, lo, hi, S, ns, scan = _case(data, shape, stride, windows)
    assert len(np.unique(R.reshape(shape[0] * shape[1], -1), axis=0)) == shape[0] * shape[1]      # no two grid points share a table column
    _common(data, shape, stride, windows, S, ns, scan, idx, lo, hi)


@pytest.mark.parametrize('data,kind,stride,windows', TIE_CASES)
def test_tie_grid(data, kind, stride, windows):
    """The oracle's T at duplicated grid points is bit-identical, its argmax is the first member of the winning class on every
    window, a quarter of the windows have a winning class with a member in the other slice, and outside the classes there are no
    near-ties."""
    R, As, idx, lo, hi, S, ns, scan = _case(data, kind, stride, windows)
    cls = gs.class_of()
    T = (2.0 * S).reshape(len(idx), -1)
    assert np.array_equal(_bits(T), _bits(T[:, cls]))                                      # every grid point = the first of its class, bit for bit
    best, lin, lead, tied = _common(data, kind, stride, windows, S, ns, scan, idx, lo, hi, cls)
    w = lin >= 0
    assert np.array_equal(cls[lin[w]], lin[w])                                              # the first copy wins
    npairs = gs.TIE_SHAPE[0] * gs.TIE_SHAPE[1]
    other_slice = np.array([len({(m % npairs) // 64 for m in gs.members_of(c)}) > 1 for c in lin[w]])
    same_slice = np.array([max(np.bincount([(m % npairs) // 64 for m in gs.members_of(c) if m // npairs == c // npairs], minlength=2)) > 1 for c in lin[w]])
    first_A = lin[w] // npairs
    print('tie grid: winners %d, with a copy in the other slice %d, with a copy in the same slice %d, winning A copies %r'
          % (int(w.sum()), int(other_slice.sum()), int(same_slice.sum()), np.bincount(first_A, minlength=6).tolist()))
    assert other_slice.sum() >= 0.25 * len(idx) and np.all(first_A < 3) and np.sum(first_A < len(As) - 1) >= 0.25 * len(idx)
    assert same_slice.sum() >= 5


@pytest.mark.parametrize('data', ('small', 'large'))
def test_oracle_accuracy(data):
    """The C oracle's CLR against a long-double restatement of 2 sum log1p(alpha R) at its grid point: 1e-12 relative, a thousandth
    of the 1e-9 the GPU tests allow."""
    assert np.finfo(np.longdouble).eps < 1e-18
    gen, k, nn, row = _sites(data)
    R = _table(data, (5, 13))
    As = list(gs.A_LIST)
    idx = gs.tests_of(20)[::8]
    lo, hi = gs.windows_of(gen, idx, 'all')
    clr, ix, ia, iA, ns = c_scan(c_oracle(), R, As, gen, row, gen[idx], lo, hi)
    worst = 0.0
    for j, i in enumerate(idx):
        if iA[j] < 0:
            continue
        sub, al = gs.window_of(gen, int(i), As[iA[j]], lo[j], hi[j])
        assert len(sub) == ns[j]
        T = 2 * np.sum(np.log1p(al.astype(np.longdouble) * R[ix[j], ia[j], row[sub]].astype(np.longdouble)))
        worst = max(worst, float(abs(clr[j] - T) / abs(T)))
    print('%s: C oracle vs long double, worst relative difference %.3e' % (data, worst))
    assert worst <= 1e-12
