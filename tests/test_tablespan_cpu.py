"""The inputs of tests/test_gpu_table_span.py really have the span_hi they ask for, reach the overflow they are meant to reach, are
free of near-ties, and the oracle is good on them.

The GPU tests must not be able to pass by never meeting a large factor, so the conditions are checked here, on the CPU, with the
table the oracle builds itself.  Every test prints the measured figures; they are copied into the docstring of tests/tablespan.py."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import tablespan as tb
from util import REPO, c_oracle, c_scan, c_sel_table, orc

from ballermixplus_amd.hostmodel import Grids

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)


@functools.lru_cache(maxsize=None)
def _grid(alist=tb.A_LIST):
    return Grids(None, None, True, False, None, alist).scan_order()


def _table_of(kind):
    """The data sets share two P_sel tables: 'large' has its own, every other set the one of n = 30."""
    return 'large' if kind == 'large' else 'n30'


def _psel(kind):
    return _psel_of(_table_of(kind))


@functools.lru_cache(maxsize=None)
def _psel_of(kind):
    """P_sel[nx][nab][rows] of the data set's sample sizes, ascending n (n = 30: the Python oracle, scipy's betabinom; the three
    large sizes: the C oracle's restatement of it, 150 times faster there)."""
    xs, ab, _ = _grid()
    if kind == 'large':
        return np.concatenate([c_sel_table(c_oracle(), 'B2', n, 1, xs, ab) for n in tb.LARGE_SIZES], axis=2)
    return orc.sel_table('B2', tb.NSAMP, 1, list(xs), list(ab))


def _row_off(kind):
    sizes = tb.sizes_of(kind)
    return dict(zip(sizes, np.concatenate(([0], np.cumsum([n + 1 for n in sizes])))[:-1].tolist()))


def _sel_max(kind):
    k, n = tb.ext_row(kind)
    return float(_psel(kind)[:, :, _row_off(kind)[n] + k].max())


@functools.lru_cache(maxsize=None)
def _sites(kind):
    gen, k, nn = tb.chromosome(kind)
    off = _row_off(kind)
    row = (np.array([off[int(n)] for n in tb.sizes_of(kind)])[np.searchsorted(tb.sizes_of(kind), nn)] + k).astype(np.int32)
    return gen, k, nn, row


@functools.lru_cache(maxsize=8)
def _table(kind, span):
    """R[nx][nab][rows] = P_sel prop / g - 1 as oracle_R builds it, 0 on the rows no site carries."""
    gen, k, nn, row = _sites(kind)
    spect, props = tb.spectrum(kind, span, _sel_max(kind), k, nn)
    g, pr = [], []
    for n in tb.sizes_of(kind):
        for kk in range(n + 1):
            g.append(spect.get((kk, n), np.nan))
            pr.append(props[n])
    with np.errstate(invalid='ignore', divide='ignore'):
        R = _psel(kind) * np.array(pr) / np.array(g) - 1.0
    assert np.isfinite(R[:, :, np.unique(row)]).all()
    return np.where(np.isfinite(R), R, 0.0)


def _ext(kind):
    k, n = tb.ext_row(kind)
    return _row_off(kind)[n] + k


CASES = [(p, s) for p in tb.PLACEMENTS for s in tb.SPANS] + [('low', tb.LOW_SPAN)] + [('large', s) for s in tb.LARGE_SPANS]


def test_the_recipe_is_what_the_docstring_says():
    xs, ab, As = _grid()
    assert (len(xs), len(ab), As) == (10, 44, [200.0, 1000.0, 5000.0, 100000.0])
    assert len(np.unique(_psel('rare').reshape(440, -1), axis=0)) == 440          # no two grid points share a table column
    base = _sites('rare')[0]
    figures = {}
    for kind in tb.PLACEMENTS + ('low', 'large'):
        gen, k, nn, row = _sites(kind)
        assert len(gen) == tb.N and np.all(np.diff(gen) > 0) and k.min() >= 1 and np.all(k <= nn)
        if kind != 'low':
            assert np.array_equal(gen, base)                                      # one set of positions
        assert np.all(row[::50] == _ext(kind))
        counts = np.bincount(row)
        first, second = np.sort(counts)[::-1][:2]
        top = int(np.argmax(counts))
        assert top == (_row_off(kind)[tb.NSAMP] + tb.LOW_K if kind == 'low' else _ext(kind)) and first > second
        figures[kind] = (int(counts[_ext(kind)]), int(first), int(second))
    assert 0.39 < figures['common'][0] / tb.N < 0.43
    gen, k, nn, row = _sites('run')
    assert np.all(k[tb.RUN_SITES[0]:tb.RUN_SITES[1]] == tb.EXT_K) and tb.RUN_SITES[1] - tb.RUN_SITES[0] == 64
    gen, k, nn, row = _sites('low')
    assert 0.09 < np.mean(k == tb.LOW_K) < 0.14
    for j in tb.LOW_PAIRS:
        assert gen[j + 1] - gen[j] == pytest.approx(tb.LOW_GAP, rel=1e-3) and k[j] == k[j + 1] == tb.LOW_K
        assert all(j in tb.tests_of(s) or j + 1 in tb.tests_of(s) for s in (1, 5, 20))
    assert sorted(set(_sites('large')[2].tolist())) == list(tb.LARGE_SIZES)
    assert _psel('large').shape[2] == 483 and 483 * 64 * 8 > 160 * 1024          # the R slice does not fit in LDS
    for stride in (1, 5, 20):
        t = tb.tests_of(stride)
        assert len(t) == 147 and np.all(np.diff(t) > 0) and t[0] == 0 and t[-1] == tb.N - 1
        assert np.median(np.diff(t)) == stride                                    # the planner picks J from the median gap
        assert ((t >= tb.RUN_SITES[0]) & (t < tb.RUN_SITES[1])).any() and (t < tb.RUN_SITES[0] - 8).any() and (t > tb.RUN_SITES[1] + 8).any()
    gen = base
    wide = [len(tb.window_of(gen, int(i), A)[0]) for A in As for i in (0, 1530, tb.N - 1)]
    print('sites of (extreme row, most frequent row, runner-up row): %r; window sizes at A = 200, 1000, 5000, 100000 of the sites '
          '0 / 1530 / N - 1: %r' % (figures, wide))
    assert wide[1] == tb.N - 1 and 500 < wide[7] < 1500


@pytest.mark.parametrize('kind,span', CASES)
def test_span(kind, span):
    """ceil(log2(1 + max R)) == span with at least 0.2 bit to either integer, and the maximum is the extreme row's."""
    R = _table(kind, span)
    top = np.unravel_index(np.argmax(R), R.shape)
    bits = float(np.log2(1.0 + R.max()))
    rest = np.delete(R, _ext(kind), axis=2)
    print('%s span %d: log2(1 + max R) = %.6f, other rows: log2(1 + max R) = %.2f, min R = -1 + %.3e'
          % (kind, span, bits, np.log2(1.0 + rest.max()), 1.0 + R.min()))
    assert top[2] == _ext(kind)
    assert int(np.ceil(bits)) == span and bits - np.floor(bits) >= 0.2 and np.ceil(bits) - bits >= 0.2
    assert np.log2(1.0 + rest.max()) < tb.SPANS[0] - 1
    assert span <= tb.SPAN_LIMIT
    if kind == 'low':
        low = 1.0 + R[:, :, tb.LOW_K]
        print('low: 1 + R of row (%d, %d): %.3e .. %.3e' % (tb.LOW_K, tb.NSAMP, low.min(), low.max()))
        assert 1e-7 < low.min() < 1e-6 and low.max() < 0.1        # g = 1: every factor of that row is below 1


def test_low_side_factors():
    """The smallest factor 1 + alpha R of the 'low' set: on the pairs 1e-9 apart, alpha = exp(-A 1e-9) > 1/2 (the
    span_generic = 54 branch of the grouped kernels' budget), R = -1 + 5.9e-7."""
    gen, k, nn, row = _sites('low')
    R = _table('low', tb.LOW_SPAN)
    rmin = R[:, :, row].min(axis=(0, 1))
    worst = {}
    for A in _grid()[2]:
        f = []
        for j in tb.LOW_PAIRS:
            for i, o in ((j, j + 1), (j + 1, j)):
                al = np.exp(-A * abs(gen[o] - gen[i]))
                assert al > 0.5
                f.append(1.0 + al * rmin[o])
        worst[A] = float(np.log2(min(f)))
    print('low side: log2 of the smallest factor per A %r' % (worst,))
    assert min(worst.values()) < -20 and max(worst.values()) < -13


@pytest.mark.parametrize('kind', ('common', 'run'))
def test_eight_factors_overflow(kind):
    """Some compared window's first eight entries of the extreme row, in the solo stream's order, have a factor product above
    2^1024 at A = 200 on the grid point of max R -- from span 129 on.  At span 128 the placed table cannot get there (8 x 127.5
    bits with every alpha < 1): that span is the boundary case on the safe side."""
    gen, k, nn, row = _sites(kind)
    A = _grid()[2][0]
    figures = {}
    for span in tb.SOLO_SPANS:
        if span < 128:
            continue
        R = _table(kind, span)
        rmax = R[:, :, _ext(kind)].max()
        best, count, total = -np.inf, 0, 0
        for stride in tb.STRIDES[False]:
            idx = tb.tests_of(stride)
            for i, lo, hi in zip(idx, *tb.windows_of(kind, idx)):
                al = tb.row0_stream(gen, row, _ext(kind), int(i), A, lo, hi)
                total += 1
                if len(al) < 8:
                    continue
                bits = float(np.sum(np.log2(1.0 + al[:8] * rmax)))
                best = max(best, bits)
                count += bits > 1024
        figures[span] = (round(best, 1), count, total)
        if span == 128:
            assert best < 1024
        else:
            assert count == total, (span, figures[span])         # every compared window, not merely one
    print('%s: span -> (largest log2 of the first eight row0 factors at A = 200, windows above 1024, windows) %r' % (kind, figures))


def test_grouped_budget_below_and_at_its_bound():
    """spend(SP * span) of the grouped and prepared kernels, SP = 64 / J sites per pass and test site: a pass over the run
    1500 .. 1563 seen from the first 32 sites at A = 200 and 1000 has every site in every window of the group with alpha <= 1/2
    (the span_hi branch, not span_generic) and every factor at the extreme row's.  SP * span_hi per (span, J): one pass takes
    between a sixth and all but 8 bits of the 1000-bit budget, so extraction is triggered both by accumulation and by a single pass."""
    gen = _sites('run')[0]
    run = np.arange(*tb.RUN_SITES)
    for A in (200.0, 1000.0):
        z = A * np.abs(gen[run][None, :] - gen[:tb.ENDS][:, None])
        assert z.min() > np.log(2.0) and z.max() < 18.0, (A, z.min(), z.max())
    nbits = {(span, J): (64 // J) * span for span in (40, 62) for J in (16, 8, 4)}
    print('SP * span_hi per (span, J): %r' % (nbits,))
    assert all(v <= tb.BUDGET_BITS for v in nbits.values())
    assert 500 < nbits[(40, 4)] < 1000 and 500 < nbits[(62, 4)] <= 1000 and tb.BUDGET_BITS - nbits[(62, 4)] < 62
    assert nbits[(62, 16)] < 500 and nbits[(40, 16)] < 500 and 4 * nbits[(62, 16)] < tb.BUDGET_BITS < 5 * nbits[(62, 16)]
    assert (64 // 4) * (tb.GROUP_SPAN_MAX + 1) > tb.BUDGET_BITS          # why can_group stops at 62


def _sums(R, As, gen, row, tg, gmin, gmax):
    """S[t][A][pair] and ns[t][A] of oracle/bmx_oracle.c orc_surface_sums over the sites given with a position in [gmin, gmax]."""
    L = c_oracle()
    L.orc_surface_sums.argtypes = [C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int64, _dp, _ip, C.c_int64, _dp, _dp, _dp, _dp, _ip]
    R = np.ascontiguousarray(R, dtype=np.float64)
    As = np.ascontiguousarray(As, dtype=np.float64)
    gen, row, tg = np.ascontiguousarray(gen), np.ascontiguousarray(row, dtype=np.int32), np.ascontiguousarray(tg)
    gmin, gmax = np.ascontiguousarray(gmin), np.ascontiguousarray(gmax)
    S = np.zeros((len(tg), len(As), R.shape[0] * R.shape[1]))
    ns = np.zeros((len(tg), len(As)), np.int32)
    L.orc_surface_sums(R.shape[0], R.shape[1], R.shape[2], R.ctypes.data_as(_dp), As.ctypes.data_as(_dp), len(As), len(gen),
                       gen.ctypes.data_as(_dp), row.ctypes.data_as(_ip), len(tg), tg.ctypes.data_as(_dp), gmin.ctypes.data_as(_dp), gmax.ctypes.data_as(_dp), S.ctypes.data_as(_dp),
                       ns.ctypes.data_as(_ip))
    return S, ns


@functools.lru_cache(maxsize=None)
def _other_rows(kind, alist):
    """The sums over the sites of every row but the extreme one, on the union of the test sites of all strides: the same for
    every span (only the extreme row's R moves with the span), so they are computed once per data set."""
    gen, k, nn, row = _sites(kind)
    union = np.unique(np.concatenate([tb.tests_of(s) for s in (1, 5, 20)]))
    rest = row != _ext(kind)
    lo, hi = tb.windows_of(kind, union)
    return (union,) + _sums(_table(kind, tb.LARGE_SPANS[0] if kind == 'large' else tb.LOW_SPAN), _grid(alist)[2], gen[rest], row[rest],
                            gen[union], gen[lo], gen[hi])


def _runner_up(kind, span, idx, alist=tb.A_LIST):
    """(T of the best grid point, its linear index (A, x, alpha_beta), T of the best other grid point) per test site index of
    idx, in the oracle's arithmetic: T = 2 sum log1p(alpha R), first strict maximum in (A, x, alpha_beta) order."""
    gen, k, nn, row = _sites(kind)
    union, S0, ns0 = _other_rows(kind, alist)
    pos = np.searchsorted(union, idx)
    assert np.array_equal(union[pos], idx)
    ext = row == _ext(kind)
    lo, hi = tb.windows_of(kind, idx)
    S1, ns1 = _sums(_table(kind, span), _grid(alist)[2], gen[ext], row[ext], gen[idx], gen[lo], gen[hi])
    assert np.all(ns0[pos] + ns1 > 0)                            # no empty window at any A
    T = (2.0 * (S0[pos] + S1)).reshape(len(idx), -1)
    lin = np.argmax(T, axis=1)                                   # first maximum
    best = T[np.arange(len(idx)), lin]
    T[np.arange(len(idx)), lin] = -np.inf
    return best, np.where(best > 0, lin, -1).astype(np.int32), T.max(axis=1)


def _strides(kind, span):
    return (1, 5, 20) if kind == 'low' else tb.STRIDES[span <= tb.GROUP_SPAN_MAX]


@pytest.mark.parametrize('kind,span', CASES)
def test_no_ties(kind, span):
    """Every compared window: the oracle's best grid point beats the runner-up (any other A, x, alpha_beta) by more than
    tablespan.TIE_BAR of its T, so the exact comparison of the integer fields on the GPU is not decided by rounding.  (No two grid
    points share a table column: there are no exact duplicates to except.)  Windows that fail must be listed in tablespan.TIED --
    at most 2 % of a case's windows -- and are skipped by the GPU tests."""
    strides = _strides(kind, span)
    bar = tb.TIE_BAR
    for s in strides:
        idx = tb.tests_of(s)
        clr, lin, sec = _runner_up(kind, span, idx)
        assert np.all(lin >= 0) and np.all(clr > 0)              # every window has a winner: no comparison of empty results
        margin = (clr - sec) / clr
        tied = np.nonzero(~(margin > bar))[0].tolist()
        print('%s span %d stride %d: CLR %.1f .. %.1f, smallest runner-up margin %.3e (absolute %.3e), %d windows below 1e-7, below the bar: %r'
              % (kind, span, s, clr.min(), clr.max(), margin.min(), (clr - sec).min(), int((margin <= 1e-7).sum()), tied))
        assert tied == list(tb.TIED.get((kind, span, s), ())), (kind, span, s, tied, margin[tied])
        assert len(tied) <= 0.02 * len(idx)
        assert clr.max() < tb.CLR_LIMIT                          # inside the range of the kernels' clamped product exponent


def test_no_ties_single_A():
    """The one case with a single A ('5000': of the four, the one whose windows are free of near-ties), placement 'run' at span 62."""
    idx = tb.tests_of(1)
    clr, lin, sec = _runner_up('run', 62, idx, tb.ONE_A)
    margin = (clr - sec) / clr
    tied = np.nonzero(~(margin > tb.TIE_BAR))[0].tolist()
    print('run span 62, A = 5000 alone: smallest runner-up margin %.3e, below the bar: %r' % (margin.min(), tied))
    assert np.all(lin >= 0) and tied == list(tb.TIED.get(('run', 62, 1, tb.ONE_A), ())) and len(tied) <= 0.02 * len(idx)


@pytest.mark.parametrize('span', (62, 240))
def test_oracle_accuracy(span):
    """The C oracle's CLR against a long-double restatement of 2 sum log1p(alpha R) at its grid point, on eight windows per
    placement: 1e-12 relative, a thousandth of the 1e-9 the GPU tests allow."""
    assert np.finfo(np.longdouble).eps < 1e-18
    As = _grid()[2]
    idx = np.array([0, 31, 1489, 1530, 1563, 1571, 2350, tb.N - 1])
    worst = 0.0
    for kind in tb.PLACEMENTS:
        gen, k, nn, row = _sites(kind)
        R = _table(kind, span)
        lo, hi = tb.windows_of(kind, idx)
        clr, ix, ia, iA, ns = c_scan(c_oracle(), R, As, gen, row, gen[idx], lo, hi)
        best, lin, _ = _runner_up(kind, span, idx)               # the sums behind test_no_ties tell the same story as orc_scan
        assert np.array_equal(lin, (iA * len(_grid()[0]) + ix) * len(_grid()[1]) + ia) and np.allclose(best, clr, rtol=1e-13, atol=0)
        for j, i in enumerate(idx):
            sub, al = tb.window_of(gen, int(i), As[iA[j]], lo[j], hi[j])
            assert len(sub) == ns[j]
            r = R[ix[j], ia[j], row[sub]].astype(np.longdouble)
            T = 2 * np.sum(np.log1p(al.astype(np.longdouble) * r))
            worst = max(worst, float(abs(clr[j] - T) / abs(T)))
    print('C oracle vs long double at span %d: worst relative difference %.3e' % (span, worst))
    assert worst <= 1e-12, worst


def test_literals_still_match_the_source():
    """The boundaries the spans were chosen around, by plain text match on bmxscan.hip: a boundary that moves fails here and flags
    this suite for re-shaping."""
    with open(os.path.join(REPO, 'ballermixplus_amd', 'csrc', 'bmxscan.hip')) as f:
        src = f.read()
    want = [
        (r'const bool can_group = [^;]*&& c->span_hi <= %d &&' % tb.GROUP_SPAN_MAX, 1),
        (r'if \(c->span_hi > %d\)\s*\n?\s*return fail\(BMX_E_LIMIT' % tb.SPAN_LIMIT, 1),
        (r'if \(bits \+ nbits > %d\) renorm_all\(\);' % tb.BUDGET_BITS, 2),
        (r'const int span_generic = max\(P\.span_hi, %d\);' % tb.SPAN_GENERIC, 2),
        (r'c->renorm_every = std::max\(1, std::min\(%d, %d / std::max\(c->span_hi, %d\)\)\);' % (tb.SOLO_LIM_CAP, tb.BUDGET_BITS, tb.SPAN_GENERIC), 1),
        (r'c->span_hi = std::max\(1, \(int\)std::ceil\(std::log2\(fmax\)\)\);', 1),
        (r'if \(lim < 8\) \{', 1),
        (r'const int ec = min\(max\(E, -131071\), 131071\) \+ 131072;', 2),
    ]
    for pat, n in want:
        assert len(re.findall(pat, src)) == n, pat
    assert [tb.solo_lim(s) for s in (62, 63, 100, 125, 126, 128, 160, 200, 240)] == [16, 15, 10, 8, 7, 7, 6, 5, 4]
