"""The cases of tests/keyrange.py hold what they claim, proved with the oracle alone: the GPU tests must not be able to pass by never
filling the upper quarter of the exponent field, by never sending index 8189 through a packed key, or by comparing near-ties.
Every test prints the figures it measured; DESIGN.md section 6 quotes them."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import keyrange as kr
import tablespan as tb
from util import REPO, c_oracle, c_scan, c_sel_table, oracle_R, orc

from ballermixplus_amd.hostmodel import Grids

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
HIGH = tuple(kr.SETS)


@functools.lru_cache(maxsize=None)
def _grid(alist=kr.A_HIGH):
    return Grids(None, None, True, False, None, alist).scan_order()


@functools.lru_cache(maxsize=None)
def _psel(sizes):
    """P_sel[nx][nab][rows] of the sample sizes, ascending n (n <= 30: the Python oracle; the large sizes: the C oracle's restatement)."""
    xs, ab, _ = _grid()
    return np.concatenate([c_sel_table(c_oracle(), 'B2', n, 1, xs, ab) if n > kr.NSAMP else orc.sel_table('B2', n, 1, list(xs), list(ab))
                           for n in sizes], axis=2)


def _row_off(sizes):
    return dict(zip(sizes, np.concatenate(([0], np.cumsum([n + 1 for n in sizes])))[:-1].tolist()))


def _rows(sizes, k, nn):
    off = _row_off(sizes)
    return np.array([off[int(n)] + int(a) for a, n in zip(k, nn)], dtype=np.int32)


def _R(sizes, spect, props, carried):
    g, pr = [], []
    for n in sizes:
        for kk in range(n + 1):
            g.append(spect.get((kk, n), np.nan))
            pr.append(props[n])
    with np.errstate(invalid='ignore', divide='ignore'):
        R = _psel(tuple(sizes)) * np.array(pr) / np.array(g) - 1.0
    assert np.isfinite(R[:, :, np.unique(carried)]).all()
    return np.where(np.isfinite(R), R, 0.0)


@functools.lru_cache(maxsize=None)
def _high(name):
    """(genPos, count, rows, extreme row's index, R as oracle_R builds it with 0 on the rows no site carries) of a 'high' set."""
    gen, k, nn = kr.chromosome(name)
    sizes = kr.sizes_of(name)
    row = _rows(sizes, k, nn)
    e = kr.ext_row(name)
    er = _row_off(sizes)[e[1]] + e[0]
    spect, props = kr.spectrum(name, _psel(tuple(sizes))[:, :, er].max(), k, nn)
    return gen, k, row, er, _R(sizes, spect, props, row)


def _sums(R, As, gen, row, tg, gmin, gmax):
    """S[t][A][pair] and ns[t][A] of oracle/bmx_oracle.c orc_surface_sums."""
    L = c_oracle()
    L.orc_surface_sums.argtypes = [C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int64, _dp, _ip, C.c_int64, _dp, _dp, _dp, _dp, _ip]
    R = np.ascontiguousarray(R, dtype=np.float64)
    As = np.ascontiguousarray(As, dtype=np.float64)
    gen, row, tg = np.ascontiguousarray(gen), np.ascontiguousarray(row, dtype=np.int32), np.ascontiguousarray(tg)
    gmin, gmax = np.ascontiguousarray(gmin), np.ascontiguousarray(gmax)
    S = np.zeros((len(tg), len(As), R.shape[0] * R.shape[1]))
    ns = np.zeros((len(tg), len(As)), np.int32)
    L.orc_surface_sums(R.shape[0], R.shape[1], R.shape[2], R.ctypes.data_as(_dp), As.ctypes.data_as(_dp), len(As), len(gen),
                       gen.ctypes.data_as(_dp), row.ctypes.data_as(_ip), len(tg), tg.ctypes.data_as(_dp), gmin.ctypes.data_as(_dp),
                       gmax.ctypes.data_as(_dp), S.ctypes.data_as(_dp), ns.ctypes.data_as(_ip))
    return S, ns


@functools.lru_cache(maxsize=None)
def _scan_of(name, band, stride):
    """(test site indices, lo, hi, T of the winner, T of the runner-up, the oracle's scan) of one scan of a 'high' set.  The sums run
    over the sites of the largest window only (a site outside it is in no window of the scan)."""
    gen, k, row, er, R = _high(name)
    idx = kr.tests_of(stride)
    lo, hi = kr.high_windows(name, band, idx, k)
    a, b = int(lo.min()), int(hi.max()) + 1
    S, ns = _sums(R, _grid()[2], gen[a:b], row[a:b], gen[idx], gen[lo], gen[hi])
    T = 2.0 * S.reshape(len(idx), -1)
    assert np.array_equal(ns[:, 0], hi - lo)                     # every site of the index window but the test site: A = 20 cuts nothing
    lin = np.argmax(T, axis=1)
    best = T[np.arange(len(idx)), lin]
    T[np.arange(len(idx)), lin] = -np.inf
    o = c_scan(c_oracle(), R, _grid()[2], gen, row, gen[idx], lo, hi)
    assert np.array_equal(lin, o[1] * len(_grid()[1]) + o[2]) and np.allclose(best, o[0], rtol=1e-13, atol=0) and np.array_equal(o[4], hi - lo)
    return idx, lo, hi, best, T.max(axis=1), o


def test_the_recipe_is_what_the_docstring_says():
    assert ((kr.CLAMP + 131072) << kr.SHIFT) | kr.SENTINEL == 2 ** 31 - 1          # the packed key has no spare bit
    assert (1 << kr.SHIFT) - 1 == kr.SENTINEL and kr.CLAMP + 131072 == (1 << 18) - 1
    xs, ab, As = _grid()
    assert (len(xs), len(ab), As) == (10, 44, [20.0])
    base = kr.chromosome('s62')
    for name in HIGH:
        gen, k, nn = kr.chromosome(name)
        assert len(gen) == kr.N and np.all(np.diff(gen) > 0)                      # no position is tied
        assert np.array_equal(gen, base[0]) and k.min() >= 1 and np.all(k <= nn)
        assert 20.0 * (gen[-1] - gen[0]) < 1.0                                    # A = 20 cuts no site of any window
        e = kr.ext_row(name)
        share = float(np.mean((k == e[0]) & (nn == e[1])))
        assert (0.58 < share < 0.63) if name == 'large' else (0.40 < share < 0.45), share
        assert np.all(k[::50] == tb.EXT_K)
    assert np.array_equal(kr.chromosome('s200')[1], base[1])                      # 's200': the same sites
    assert sorted(set(kr.chromosome('large')[2].tolist())) == list(tb.LARGE_SIZES)
    assert _psel(tuple(tb.LARGE_SIZES)).shape[2] == 483 and 483 * 64 * 8 > 160 * 1024          # the R slice does not fit in LDS
    for s in kr.STRIDES:
        t = kr.tests_of(s)
        assert len(t) >= 32 and np.all(np.diff(t) == s) and t[0] < kr.CENTRE <= t[-1]
    gen, k, nn = kr.low_chromosome()
    assert len(gen) == kr.LOW_N == 16000 and np.all(np.diff(gen) > 0)
    assert gen[0] == 0.0 and gen[1] == 1e-20 and np.exp(-100.0 * gen[1]) == 1.0 and np.exp(-1.0 * gen[1]) == 1.0
    assert np.all(k[2:2 + kr.LOW_BLOCK] == kr.LOW_K) and not np.any(k[2 + kr.LOW_BLOCK:] == kr.LOW_K) and np.all(nn[:2] == 7)
    assert np.array_equal(gen[2:2 + kr.LOW_BLOCK], 1.0 + kr.LOW_STEP * np.arange(kr.LOW_BLOCK))
    assert not np.any(gen == kr.MIXED_POS)
    gen, k, nn = kr.wide_chromosome()
    assert np.all(np.diff(gen) > 0) and np.diff(gen).min() > 19.0 / 1e9           # a value of 1e9 and more reaches no site
    for nA in kr.WIDE_NA:
        As = kr.wide_grid(nA)
        u = list(kr.wide_useful(nA))
        assert len(As) == nA and np.array_equal(As[u], kr.WIDE_A) and np.delete(As, u).min() >= 1e9 and 10.0 <= min(kr.WIDE_A) and max(kr.WIDE_A) <= 2e5
    d = kr.wide_grid(8190, dup=True)
    assert d[5] == d[8189] and np.sum(d < 1e9) == 6
    for at in (0, 8189):
        b = kr.both_grid(at)
        assert len(b) == 8190 and b[at] == 20.0 and np.sum(b < 1e9) == 1


@pytest.mark.parametrize('name', HIGH)
def test_span(name):
    gen, k, row, er, R = _high(name)
    top = np.unravel_index(np.argmax(R), R.shape)
    bits = float(np.log2(1.0 + R.max()))
    rest = np.delete(R, er, axis=2)
    print('%s: log2(1 + max R) = %.6f, other rows %.2f, %d sites of the extreme row' % (name, bits, np.log2(1.0 + rest.max()), int(np.sum(row == er))))
    assert top[2] == er and abs(bits - (kr.SETS[name] - tb.MARGIN)) < 1e-6 and np.log2(1.0 + rest.max()) < 11
    assert int(np.argmax(np.bincount(row))) == er                                 # the most frequent row (the solo kernel's row0)


@pytest.mark.parametrize('name', HIGH)
def test_high_bands_and_margins(name):
    """Per (stride, band): E* of every window, the populations, and the runner-up margins of the compared windows."""
    found, compared = {}, 0
    for s in kr.STRIDES:
        pop = {}
        for band in kr.BANDS:
            idx, lo, hi, best, second, o = _scan_of(name, band, s)
            E = kr.e_star(best)
            got = kr.band_of(E)
            pop[band] = got.count(band)
            margin = (best - second) / best
            tied = np.nonzero(~(margin > kr.TIE_BAR))[0].tolist()
            print('%s stride %d %s (K = %d): E* %d .. %d, T %.5e .. %.5e, window sizes %d .. %d, %d of %d in the band, smallest margin %.2e, tied %r'
                  % (name, s, band, kr.K_OF[(name, band)], E.min(), E.max(), best.min(), best.max(), (hi - lo).min(), (hi - lo).max(),
                     pop[band], len(idx), margin.min(), tied))
            if band == 'outside':
                assert E.min() >= kr.OUTSIDE                      # every window of the scan must be refused
                assert E.max() < 140000                           # ... and is just past the range, not far beyond it
            else:
                assert E.max() <= kr.INSIDE[1]                    # no window that would have the scan refused, none 'between'
                compared += len(idx)
                if tied:
                    found[(name, band, s)] = tuple(tied)
                assert np.all(o[3] == 0)                          # a winner in every compared window
        assert pop['inside'] >= 30 and pop['outside'] >= 30, (name, s, pop)
        assert min(pop[r] for r in kr.RUNGS) >= 12, (name, s, pop)
        if name != 's62' or s == 1:                               # ([i - K, i + K] at stride 5 / 20: the extreme-row count varies more)
            assert min(pop[r] for r in kr.RUNGS) >= 30
    # the list of near-ties is complete, and short: at most 2 % of the set's compared windows
    print('%s: tied %r of %d compared windows' % (name, found, compared))
    assert found == {key: v for key, v in kr.TIED.items() if key[0] == name}
    assert sum(len(v) for v in found.values()) <= 0.02 * compared


@pytest.mark.parametrize('name', HIGH)
def test_oracle_accuracy(name):
    """The C oracle's CLR against a long-double restatement of 2 sum log1p(alpha R) on eight inside-band windows per set."""
    assert np.finfo(np.longdouble).eps < 1e-18
    gen, k, row, er, R = _high(name)
    worst, n = 0.0, 0
    for s in (1, 20):
        idx, lo, hi, best, second, o = _scan_of(name, 'inside', s)
        for j in (0, 9, 18, 31):
            assert kr.INSIDE[0] <= kr.e_star(o[0][j]) <= kr.INSIDE[1]
            sub = np.concatenate([np.arange(lo[j], idx[j]), np.arange(idx[j] + 1, hi[j] + 1)])
            al = np.exp(-20.0 * np.abs(gen[sub] - gen[idx[j]]))
            r = R[o[1][j], o[2][j], row[sub]].astype(np.longdouble)
            T = 2 * np.sum(np.log1p(al.astype(np.longdouble) * r))
            worst = max(worst, float(abs(o[0][j] - T) / abs(T)))
            n += 1
    print('%s: C oracle vs long double on %d inside-band windows: worst relative difference %.3e' % (name, n, worst))
    assert n == 8 and worst <= 1e-12, worst


@functools.lru_cache(maxsize=None)
def _low(name):
    gen, k, nn = kr.low_chromosome(name)
    sizes = list(kr.low_sizes(name))
    row = _rows(sizes, k, nn)
    lr = _row_off(sizes)[kr.low_row(name)[1]] + kr.low_row(name)[0]
    spect, props = kr.low_spectrum(_psel(tuple(sizes))[:, :, lr].max(), k, nn, name)
    return gen, row, lr, _R(sizes, spect, props, row)


@pytest.mark.parametrize('name', ('low', 'lowL'))
def test_low_case(name):
    """'low' and, on the sample sizes (7, 150, 160, 170) whose table does not fit in LDS, 'lowL'."""
    gen, row, lr, R = _low(name)
    if name == 'lowL':
        assert R.shape[2] == 491 and R.shape[2] * 64 * 8 > 160 * 1024                 # the R slice does not fit in LDS
        assert sorted(set(kr.low_chromosome(name)[2].tolist())) == [7] + list(tb.LARGE_SIZES) and lr == 8 + kr.LOWL_K
    As = _grid(kr.LOW_A)[2]
    assert As == [1.0, 100.0]
    low = 1.0 + R[:, :, lr]
    assert low.max() <= kr.LOW_FACTOR * (1 + 1e-9)                        # 1 + R <= 1e-6 at EVERY grid point (R + 1 rounds at 1e-16)
    # 'lowL': P_sel of (32, 150) spans 8.9e-12 over the grid, so R rounds to -1 at its far grid points; the block's alpha < 1 keeps
    # those factors 1 - alpha > 0, and only 'zero' holds an exact zero factor (asserted below)
    assert low.min() > 0 if name == 'low' else (low.min() >= 0 and np.mean(low > 0) > 0.5)
    assert np.all(R[:, :, :8] == -1.0)                                            # share 0.0: R = -1 exactly on the rows of size 7
    print('%s: 1 + R of the block row %.3e .. %.3e' % (name, low.min(), low.max()))
    L = c_oracle()
    for K in kr.LOW_KS:
        for s in kr.STRIDES:
            tg, lo, hi, kinds = kr.low_tests(s, K)
            assert np.all(np.diff(tg) > 0) and kinds[0] == 'zero' and kinds[-1] == 'mixed' and kinds.count('block') >= 32
            o = c_scan(L, R, As, gen, row, tg, lo, hi)
            assert np.all(o[0][:-1] == 0.0) and np.all(o[3][:-1] == -1) and np.all(o[4][:-1] == 0)     # 'zero' and the block: none
            assert o[3][-1] == 1 and 0.0 < o[0][-1] < 1e3 and o[4][-1] == 64                            # 'mixed': the second A wins
        tg, lo, hi, kinds = kr.low_tests(20, K)
        pick = np.array([1, len(tg) // 2, len(tg) - 2])
        with np.errstate(divide='ignore'):
            S, ns = _sums(R, As, gen, row, tg[pick], gen[lo[pick]], gen[hi[pick]])
        E = kr.e_star(2.0 * S.max(axis=2))                        # [window][A]: the best grid point's exponent
        print('%s K = %d: E* of the best grid point per A = 1 / 100: %r, window sizes %r' % (name, K, E.tolist(), ns.tolist()))
        assert np.all(ns == 2 * K)
        if K == kr.LOW_KS[0]:
            assert np.all(E > -kr.CLAMP) and np.all(E < -100000)                  # inside the clamp, near it
        else:
            assert np.all(E < -kr.CLAMP - 300)                                    # past it at either A (3400) and far past it (7000)
        if K == kr.LOW_KS[2]:
            assert np.all(E < -2 * kr.CLAMP)
    tg, lo, hi, kinds = kr.low_tests(1, kr.LOW_KS[0])
    with np.errstate(divide='ignore'):
        S, ns = _sums(R, As, gen, row, tg[[0, -1]], gen[lo[[0, -1]]], gen[hi[[0, -1]]])
    assert np.all(S[0] == -np.inf) and ns[0].tolist() == [1, 1]                   # 'zero': T = -inf at every grid point, at both A
    T = 2.0 * S[1]
    print('%s, mixed window: best T at A = 1 %.4e (E* %d, %d sites), at A = 100 %.4f (%d sites)'
          % (name, T[0].max(), kr.e_star(T[0].max()), ns[1][0], T[1].max(), ns[1][1]))
    assert T[0].max() < -3e4 and 0 < T[1].max() < 1e3 and ns[1].tolist() == [kr.LOW_N, 64]


@functools.lru_cache(maxsize=None)
def _wide():
    gen, k, nn = kr.wide_chromosome()
    cnt = {}
    for a in k.tolist():
        cnt[(a, 50)] = cnt.get((a, 50), 0) + 1
    spect = {key: v / len(k) for key, v in cnt.items()}
    R = oracle_R('B2', [50], int(k.min()), spect, {50: 1.0}, [0.3], [10.0])
    return gen, k.astype(np.int32), np.where(np.isfinite(R), R, 0.0)


def test_wide_grids_win_at_every_useful_index():
    gen, row, R = _wide()
    n = len(gen)
    lo, hi = np.zeros(n, np.int64), np.full(n, n - 1, np.int64)
    L = c_oracle()
    for nA in kr.WIDE_NA:
        o = c_scan(L, R, kr.wide_grid(nA), gen, row, gen, lo, hi)
        wins = {u: int(np.sum(o[3] == u)) for u in kr.wide_useful(nA)}
        print('wideA nA = %d: windows won per index %r, without a winner %d' % (nA, wins, int(np.sum(o[3] < 0))))
        assert min(wins.values()) >= 20 and sum(wins.values()) + int(np.sum(o[3] < 0)) == n
        few = c_scan(L, R, list(kr.WIDE_A), gen, row, gen, lo, hi)                # the values out of reach change nothing
        assert np.array_equal(np.array(kr.wide_useful(nA) + (-1,))[few[3]], o[3]) and np.array_equal(few[0], o[0])
    o = c_scan(L, R, kr.wide_grid(8190, dup=True), gen, row, gen, lo, hi)
    print('wideA dup: won at index 5: %d, at index 8189: %d' % (int(np.sum(o[3] == 5)), int(np.sum(o[3] == 8189))))
    assert np.sum(o[3] == 5) >= 20 and np.sum(o[3] == 8189) == 0                  # equal T: the lower index wins


def test_both_fields_at_their_ends():
    """'both': the winner's packed key (ec << 13) | 8189 of the inside-band windows, from the oracle's E*."""
    idx, lo, hi, best, second, o = _scan_of('s62', 'inside', 1)
    key = ((kr.e_star(best) + 131072) << kr.SHIFT) | 8189
    gap = (2 ** 31 - 1) - key
    print('both: INT32_MAX - packed key = %d .. %d (2^13 per unit of the exponent: %d .. %d below the clamp)'
          % (gap.min(), gap.max(), gap.min() >> 13, gap.max() >> 13))
    assert np.all(gap > 0) and gap.max() < (kr.CLAMP - kr.INSIDE[0] + 1) << kr.SHIFT and key.min() > 0.99 * 2 ** 31


def test_literals_still_match_the_source():
    """The clamp, the shift, the sentinel and the planner's bound, by plain text match on bmxscan.hip."""
    with open(os.path.join(REPO, 'ballermixplus_amd', 'csrc', 'bmxscan.hip')) as f:
        src = f.read()
    want = [
        (r'const int ec = min\(max\(E(\[j\])?, -%d\), %d\) \+ 131072;' % (kr.CLAMP, kr.CLAMP), 5),
        (r'bestK\[j\] = \(131072 << %d\) \| %d;' % (kr.SHIFT, kr.SENTINEL), 1),
        (r'bestK\[j\] = \(\(131072 \+ \(BMX_FREXP \? 1 : 0\)\) << %d\) \| %d;' % (kr.SHIFT, kr.SENTINEL), 1),
        (r'const int biA = bestK\[j\] & %d;' % kr.SENTINEL, 2),
        (r'const bool can_group = [^;]*&& c->nA < %d &&' % kr.SENTINEL, 1),
        (r'if \(bE >= %d \+ 131072\) \*F\.over = 1;' % kr.CLAMP, 1),
    ]
    for pat, n in want:
        assert len(re.findall(pat, src)) == n, pat
