"""The catalogue of tests/offgrid.py really holds the windows, hulls and workspace sizes it is meant to hold, its replay IS
refine.compass (bit for bit, on analytic objectives and on the C oracle's), and the share of windows whose search path is decided by
less than offgrid.MARGIN_BAR stays under what tests/test_gpu_offgrid.py may leave out -- shown with the oracle alone, so that the GPU
tests cannot pass by never meeting these cases.  Every test prints the measured figures."""
import functools
import math
import os
import re

import numpy as np
import pytest

import gridshape as gs
import offgrid as og
from util import REPO, c_oracle, c_scan, c_sel_table

from ballermixplus_amd import refine


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ----------------------------------------------------------------------------- the oracle's objective
class Oracle:
    """T of a case's windows at arbitrary points: the C oracle's selection table (c_sel_table, combined with prop and g as
    test_gpu_refine.Problem.R combines them) and the window of gridshape.window_of (offgrid.window_at: the same predicate for a
    test position that need not be a site)."""

    def __init__(self, name):
        c = og.CASES[name]
        d = og.dataset(c.data)
        self.case, self.d = c, d
        self.xs, self.abetas, self.As = og.GRIDS[c.grid]
        self.rows = og.rows_of(c.data)
        self.tg, self.idx, self.lo, self.hi, self.is_site = og.tests_of(name)
        self.used = sorted(set(d.nn.tolist()))                                  # a size no site carries needs no table
        self.g = np.array([d.spect.get((k, n), np.nan) if n in self.used else np.nan for n in d.sizes for k in range(n + 1)])
        self.pr = np.array([d.props[n] for n in d.sizes for k in range(n + 1)])
        self.setup = og.setup_of(c.grid)
        self.cache = {}

    def psel(self, xs, abetas):
        L = c_oracle()
        return np.concatenate([c_sel_table(L, 'B2', n, 1, xs, abetas) if n in self.used else np.full((len(xs), len(abetas), n + 1), np.nan)
                               for n in self.d.sizes], axis=2)

    def R(self, x, a):
        if (x, a) not in self.cache:
            if len(self.cache) > 4096:
                self.cache.clear()
            with np.errstate(invalid='ignore', divide='ignore'):
                self.cache[(x, a)] = self.psel([x], [a])[0, 0] * self.pr / self.g - 1.0
        return self.cache[(x, a)]

    def T(self, j, A, x, a):
        if self.is_site[j]:
            sub, al = gs.window_of(self.d.gen, int(self.idx[j]), A, self.lo[j], self.hi[j])
        else:
            sub, al = og.window_at(self.d.gen, self.tg[j], A, self.lo[j], self.hi[j])
        if len(sub) == 0:
            return -math.inf
        v = float(2.0 * np.sum(np.log1p(al * self.R(x, a)[self.rows[sub]])))
        return v if math.isfinite(v) else -math.inf

    def scan(self):
        """The oracle's grid scan of the case: (clr, ix, ia, iA, ns)."""
        with np.errstate(invalid='ignore', divide='ignore'):
            R = self.psel(self.xs, self.abetas) * self.pr / self.g - 1.0
        R = np.where(np.isfinite(R), R, 0.0)
        return c_scan(c_oracle(), R, self.As, self.d.gen, self.rows, self.tg, self.lo, self.hi)

    def starts(self, scan, pick):
        """(c0 f64[n, 3], nat0, h0) of the windows `pick` from the scan's argmax."""
        clr, ix, ia, iA, ns = scan
        s = [self.setup.start(self.As[iA[j]], self.xs[ix[j]], self.abetas[ia[j]]) for j in pick]
        return tuple(np.array([v[q] for v in s]).reshape(len(pick), 3) for q in range(3))

    def replay(self, scan, pick):
        c0, nat0, h0 = self.starts(scan, pick)
        calls = [0]

        def eval_batch(c, act):
            calls[0] += 1
            nat = og.naturals(c, c0, nat0)
            return np.array([self.T(pick[q], *nat[q]) if act[q] else np.nan for q in range(len(pick))])
        st = self.setup
        r = og.replay(eval_batch, c0, st.free, st.lo, st.hi, h0)
        assert calls[0] <= 6 * refine.MAX_ROUNDS + 1
        return r, (c0, nat0, h0)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    o = Oracle(name)
    return o, o.scan()


def _sample(rows, count):
    rows = np.asarray(rows)
    return rows if len(rows) <= count else rows[np.unique(np.linspace(0, len(rows) - 1, count).astype(int))]


# ----------------------------------------------------------------------------- replay == refine.compass
def _quadratic(j, c):
    t = (8.0 + 0.01 * j, 0.21 + 0.001 * (j % 50), 1.0 + 0.02 * j)
    d = [c[k] - t[k] for k in range(3)]
    return 10.0 - (d[0] * d[0] + 40.0 * d[1] * d[1] + 0.5 * d[2] * d[2] + 1.2 * d[0] * d[2] + 3.0 * d[0] * d[1])


def _plateau(j, c):
    """Piecewise constant: whole rounds of exact ties; the first candidate in order must win them."""
    return -float(math.floor(abs(c[0] - 8.0) * 2.0) + math.floor(abs(c[1] - 0.3) * 40.0) + math.floor(abs(c[2] - (j % 7)) * 1.5))


def _hole(j, c):
    """-inf on a region that holds some starts and cuts the way of other searches."""
    if c[2] > 6.0 + 0.1 * (j % 5) or c[0] < 6.0 or 0.26 < c[1] < 0.29:
        return -math.inf
    return _quadratic(j, c)


def _hull(j, c):
    """Monotone: the maximum is a corner of the hull; the direction depends on the window."""
    return (1.0 if j % 2 else -1.0) * c[0] + (1.0 if j % 3 else -2.0) * c[1] + 0.1 * c[2]


def _nan(j, c):
    """A non-finite T counts as -inf."""
    return math.nan if c[1] > 0.4 else (math.inf if c[0] > 11.0 else _quadratic(j, c))


@pytest.mark.parametrize('grid', ('all', 'corner', 'tie', 'x', 'uv'))
@pytest.mark.parametrize('f', (_quadratic, _plateau, _hole, _hull, _nan), ids=lambda f: f.__name__.strip('_'))
def test_replay_is_compass_on_analytic_objectives(f, grid):
    """Every grid point a start (on 'corner' every start is a hull corner): coordinates, T, rounds and final steps as bits."""
    xs, ab, As = og.GRIDS[grid]
    st = og.setup_of(grid)
    pts = sorted(set((A, x, a) for A in As for x in xs for a in ab))
    s = [st.start(*p) for p in pts]
    c0, nat0, h0 = (np.array([v[q] for v in s]) for q in range(3))
    calls, inactive = [0], [0]

    def eval_batch(c, act):
        calls[0] += 1
        inactive[0] += int((~act).sum())
        return np.array([f(j, tuple(p)) for j, p in enumerate(c.tolist())])         # inactive rows hold a valid point too
    r = og.replay(eval_batch, c0, st.free, st.lo, st.hi, h0)
    assert calls[0] <= 6 * refine.MAX_ROUNDS + 1
    ties = 0
    for j in range(len(pts)):
        c, T, rounds, h = refine.compass(lambda p: f(j, p), tuple(c0[j]), st.free, st.lo, st.hi, tuple(h0[j]))
        assert np.array_equal(_bits(c), _bits(r.c[j])) and _bits(T) == _bits(r.T[j]) and rounds == r.rounds[j], (j, c, r.c[j])
        assert np.array_equal(_bits(h), _bits(r.h[j])) and _bits(refine._finite(f(j, tuple(c0[j])))) == _bits(r.T0[j])
        ties += r.margin[j] == 0.0
    print('%s on grid %s: %d starts, %d calls, %d inactive rows, rounds %d .. %d, %d windows met an exact tie, %d ended at -inf'
          % (f.__name__, grid, len(pts), calls[0], inactive[0], r.rounds.min(), r.rounds.max(), ties, int(np.isinf(r.T).sum())))
    assert np.all(r.margin >= 0.0)
    if f is _plateau:
        assert ties >= 0.5 * len(pts)
    if f is _quadratic and grid == 'all':
        assert ties == 0 and np.all(np.isfinite(r.margin))
    if f is _hull:                                    # ends on the hull in u and x where free (to the spacing of f's values)
        for k in (0, 1):
            assert not st.free[k] or np.all(np.minimum(np.abs(r.c[:, k] - st.lo[k]), np.abs(r.c[:, k] - st.hi[k])) < 1e-13)
    if f is _hole and grid == 'all':
        assert (np.isinf(r.T0) & np.isfinite(r.T)).any() and np.isinf(r.T).any()       # starts at -inf that find a way out, and that do not


def test_margin_rule():
    """The margin of single rounds, on one free coordinate (x) with a tabulated objective."""
    def run(Tc, Tm, Tp):
        vals = {0.3: Tc, 0.2: Tm, 0.4: Tp}
        r = og.replay(lambda c, act: np.array([vals[round(float(c[0, 1]), 6)]]), [[0.0, 0.3, 0.0]], (False, True, False), (0, 0.2, 0),
                      (0, 0.4, 0), [[0.0, 0.1, 0.0]], tol=(0.0, 0.0, 0.0), max_rounds=1)
        return float(r.margin[0]), float(r.c[0, 1])
    assert run(10.0, 8.0, 9.0) == (pytest.approx(0.1), 0.3)                    # no move: Tc - max T_i over max(|Tc|, |best|)
    assert run(10.0, 12.0, 11.0) == (pytest.approx(1.0 / 12.0), 0.2)            # a move: the runner-up is closer than the centre
    assert run(10.0, 12.0, 4.0) == (pytest.approx(2.0 / 12.0), 0.2)             # ... the centre is closer
    assert run(10.0, 12.0, 12.0) == (0.0, 0.2)                                   # an exact tie: the first in order wins, margin 0
    assert run(10.0, 10.0, 3.0) == (0.0, 0.3)                                    # a candidate ties the centre: no move, margin 0
    assert run(10.0, -math.inf, -math.inf) == (math.inf, 0.3)                    # comparisons against -inf do not count
    assert run(-math.inf, -math.inf, 5.0) == (math.inf, 0.4)
    assert run(-math.inf, 5.0, 4.0) == (pytest.approx(0.2), 0.2)
    assert run(10.0, -math.inf, 9.0) == (pytest.approx(0.1), 0.3)


def test_replay_is_compass_on_the_oracle():
    """small / all / ragged, every third window with a grid result, on the C oracle's objective."""
    o, scan = _oracle('small-all-ragged')
    pick = np.nonzero(scan[3] >= 0)[0][::3]
    r, (c0, nat0, h0) = o.replay(scan, pick)
    st = o.setup
    moved = 0
    for q, j in enumerate(pick.tolist()):
        f = refine.coord_objective(lambda A, x, a: o.T(j, A, x, a), tuple(c0[q]), tuple(nat0[q]))
        c, T, rounds, h = refine.compass(f, tuple(c0[q]), st.free, st.lo, st.hi, tuple(h0[q]))
        assert np.array_equal(_bits(c), _bits(r.c[q])) and _bits(T) == _bits(r.T[q]) and rounds == r.rounds[q], j
        assert np.array_equal(_bits(h), _bits(r.h[q]))
        moved += T > r.T0[q]
    print('small-all-ragged: %d windows replayed, %d moved off their start, rounds %d .. %d' % (len(pick), moved, r.rounds.min(), r.rounds.max()))
    assert len(pick) >= 40 and moved >= 20


# ----------------------------------------------------------------------------- catalogue facts
def test_row_counts_and_workspace_edge():
    from ballermixplus_amd import engine
    got = {}
    for data in og.WIDE_SIZES:
        d = og.dataset(data)
        xs, ab, As = og.GRIDS['wideA']
        m = engine.ModelArrays('B2', 1, d.sizes, d.spect, d.props, xs, ab)
        rows = m.rows_of(d.k, d.nn)
        assert np.array_equal(rows, og.rows_of(data))
        assert np.isfinite(m.g[rows]).all()                                     # every site's row has a neutral probability
        got[data] = (m.rows, (m.rows * 45 + 15) // 16 * 16)
    print('rows and workspace bytes: %r' % got)
    assert got == {'wide728': (728, 32768), 'wide729': (729, 32816), 'wide90831': (90831, 4087408)}
    assert {k: v[0] for k, v in got.items()} == og.WIDE_ROWS
    assert got['wide728'][1] <= 32 * 1024 < got['wide729'][1]                   # either side of REFINE_LDS_WS
    assert (512 << 20) // got['wide90831'][1] == 131 < og.WIDE_M                # the slab cap leaves fewer workgroups than windows
    assert got['wide90831'][0] > 65535                                          # 4-byte row indices
    a, b = og.dataset('wide728'), og.dataset('wide729')
    assert all(np.array_equal(u, v) for u, v in zip(a[:3], b[:3])) and a.spect == b.spect and a.props[300] == b.props[300] == 1.0
    for data, rows in (('small', 21), ('large', 483)):
        assert sum(n + 1 for n in og.dataset(data).sizes) == rows and rows * 45 < 32 * 1024
    gen = a.gen
    assert np.all(np.diff(gen) >= 0) and int(np.sum(np.diff(gen) == 0)) == len(og.WIDE_TIES)
    tg, idx, lo, hi, is_site = og.wide_tests(gen)
    assert len(tg) == og.WIDE_M and 90 <= int((~is_site).sum()) <= 100 and not np.isin(tg[~is_site], gen).any() and np.all(np.diff(tg) > 0)
    n5000 = [len(og.window_at(gen, t, 5000.0, 0, len(gen) - 1)[0]) for t in tg]
    print('wide: %d test positions, %d of them midpoints; sites within the cut at A = 5000: %d .. %d' % (len(tg), int((~is_site).sum()), min(n5000), max(n5000)))
    assert max(n5000) <= 200


def test_source_pins():
    """The constants the catalogue was built around, by plain text match on bmxscan.hip: a change there flags this suite."""
    with open(os.path.join(REPO, 'ballermixplus_amd', 'csrc', 'bmxscan.hip')) as f:
        src = f.read()
    for pat in (r'constexpr int REFINE_THREADS = 256;', r'constexpr int64_t REFINE_LDS_WS = 32 \* 1024;', r'constexpr int REFINE_GRID_MAX = 2048;',
                r'constexpr int REFINE_TABS = 5;', r'\(int64_t\)c->rows \* \(REFINE_TABS \* 8 \+ 4 \+ 1\) \+ 15\) / 16 \* 16;',
                r'std::min<int64_t>\(blocks, \(512LL << 20\) / ws\)', r'std::min<int64_t>\(REFINE_GRID_MAX, 8LL \* std::max\(cus, 1\)\)'):
        assert re.search(pat, src), pat
    assert len(og.tests_of('stride')[0]) == 4003 > 2048 and (4003 + 1) // 2 <= 2048


# Kinds a case's geometry cannot hold, with the count it holds instead (asserted exactly):
#   'long' (more than 512 sites in the range): a ragged window of gridshape.windows_of holds at most 2 RAGGED_R + 2 = 302 sites, and
#          a window of the wide data about 150 at the smallest A -- the 'all' cases supply the long ranges (asserted below);
#   'tie': the stride-20 test sites meet two tied positions (sites 2600 and 4000);
#   'empty', 'right': a window [i - r, i + r] of the wide data holds its site (r = 0 at a site holds the test position alone: no site
#          for T, so no grid result).
def _lacks(name):
    c = og.CASES[name]
    if c.tests == 'wide':
        return {'long': 0, 'empty': 0, 'right': 0}
    return {'long': 0, 'tie': 2} if c.tests == 20 else {'long': 0}


@pytest.mark.parametrize('name', og.RAGGED)
def test_window_kinds(name):
    g = og.geometry(name)
    count = {k: int(g[k].sum()) for k in og.KINDS}
    print('%s: %d windows, of each kind: %r' % (name, len(g['empty']), count))
    lacks = _lacks(name)
    for k in og.KINDS:
        if k in lacks:
            assert count[k] == lacks[k], (name, k, count[k])
        else:
            assert count[k] >= 5, (name, k, count[k])
    c = og.CASES[name]
    if c.tests == 'wide':
        tg, idx, lo, hi, is_site = og.tests_of(name)
        bare = is_site & (lo == idx) & (hi == idx)
        assert bare.sum() >= 5                                                  # windows that hold the test position alone
        spans = {int(r): int(np.sum((idx - lo >= r) & (hi - idx >= r) & ((idx - lo == r) | (hi - idx == r)))) for r in og.WIDE_R}
        print('wide: windows per half-width %r' % spans)
        assert all(v >= 20 for v in spans.values())


@pytest.mark.parametrize('name', [n for n, c in og.CASES.items() if c.windows == 'all'])
def test_whole_chromosome_windows_have_long_ranges(name):
    g = og.geometry(name)
    assert g['long'].sum() >= 5 and g['tie'].sum() == 2
    at_large_A = og.geometry(name, max(og.GRIDS[og.CASES[name].grid][2]))
    print('%s: %d ranges of more than 512 sites at the smallest A, %d of fewer than 256 at the largest' % (name, int(g['long'].sum()), int(at_large_A['short'].sum())))
    assert at_large_A['short'].sum() >= 5


def test_free_sets_and_corner_starts():
    for grid, free in og.FREE.items():
        st = og.setup_of(grid)
        assert st.free == free, grid
    assert sorted(og.FREE[s] for s in og.SUBSETS) == sorted(f for f in
           [(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)] if 0 < sum(f) < 3)   # every proper subset
    st = og.setup_of('corner')
    xs, ab, As = og.GRIDS['corner']
    clamped = 0
    for A in As:
        for x in xs:
            for a in ab:
                c, nat, h = st.start(A, x, a)
                for k in range(3):
                    v = [min(max(c[k] + s * h[k], st.lo[k]), st.hi[k]) for s in (-1, 1)]
                    assert (v[0] == c[k]) != (v[1] == c[k]), (A, x, a, k)       # exactly one candidate per coordinate clamps onto the centre
                    clamped += 1
    print('corner: %d starts, %d clamped candidates in round 1' % (len(As) * len(xs) * len(ab), clamped))
    assert clamped == 24


def test_tie_starts_sit_on_repeated_values():
    xs, ab, As = og.GRIDS['tie']
    for name in ('small-tie-ragged', 'small-tie-all'):
        o, scan = _oracle(name)
        clr, ix, ia, iA, ns = scan
        w = iA >= 0
        rep = {'A': int(np.sum([As.count(As[i]) > 1 for i in iA[w]])), 'x': int(np.sum([xs.count(xs[i]) > 1 for i in ix[w]])),
               'alpha_beta': int(np.sum([ab.count(ab[i]) > 1 for i in ia[w]]))}
        print('%s: %d starts, on a repeated value of %r' % (name, int(w.sum()), rep))
        assert min(rep.values()) >= 10
        # the start is the first copy, and the host Axis (sorted, distinct) still finds its step
        assert np.all(iA[w] < 3)
        st = o.setup
        for j in np.nonzero(w)[0][:20]:
            c, nat, h = st.start(As[iA[j]], xs[ix[j]], ab[ia[j]])
            assert all(v > 0 for v in h)


# ----------------------------------------------------------------------------- the share the replay may leave out
SHARE_CASES = [n for n in og.REPLAYED if n != 'wide729']       # wide729's objective is wide728's (test_row_counts_and_workspace_edge)


@pytest.mark.parametrize('name', SHARE_CASES)
def test_share_of_windows_decided_by_less_than_the_bar(name):
    """With the oracle's objective, at least offgrid.JUDGED_SHARE of a case's refined windows (a sample of 80) keep every decision of
    their search path at a margin of offgrid.MARGIN_BAR or more: the same condition tests/test_gpu_offgrid.py holds the device to.
    Also: the case has windows to refine, windows that improve and windows without a grid result."""
    o, scan = _oracle(name)
    clr, ix, ia, iA, ns = scan
    has = np.nonzero(iA >= 0)[0]
    pick = _sample(has, 80)
    r, _ = o.replay(scan, pick)
    low = int(np.sum(r.margin < og.MARGIN_BAR))
    low10 = int(np.sum(r.margin < 1e-10))
    tie = int(np.sum(r.margin == 0.0))
    improved = int(np.sum(r.T > clr[pick]))
    print('%s: %d windows, %d with a grid result, %d replayed: %d improved, smallest margin under %.0e in %d (%.0f %% kept), under 1e-10 in %d, exact ties %d, rounds %d .. %d'
          % (name, len(clr), len(has), len(pick), improved, og.MARGIN_BAR, low, 100.0 * (1 - low / len(pick)), low10, tie, r.rounds.min(), r.rounds.max()))
    assert len(pick) >= 40 and improved >= 1 and np.sum(iA < 0) >= 1
    assert 1 - low / len(pick) >= og.JUDGED_SHARE
