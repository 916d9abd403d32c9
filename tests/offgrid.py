"""Seeded inputs that walk the off-grid search kernels (refine_kernel, support_kernel, boot_kernel of bmxscan.hip) through window
geometry, hull and free-coordinate sets and workspace placement, and an exact host replay of their compass search: the input of
tests/test_offgrid_cpu.py and tests/test_gpu_offgrid.py.  numpy and the pure-Python definitions (ballermixplus_amd/refine.py);
no library call and no oracle -- the caller brings the objective.

Data.  'small' (21 table rows) and 'large' (483) are tests/gridshape.py's chromosomes, spectra and windows, unchanged.  wide(sizes)
adds one recipe for the edges of the refinement's workspace (45 bytes per table row: in LDS up to 32 KiB, beyond in a global slab):
WIDE_N = 1500 sites, all draws from ONE np.random.default_rng(WIDE_SEED) in this order:
  1. genPos = cumsum(rng.geometric(0.02, N)) / 1e6, then genPos[j + 1] = genPos[j] for j in WIDE_TIES (one triple)
  2. the sample size rng.choice(used, N); used = the sizes that sites carry
  3. the count: n where rng.random(N) < 0.5, else floor(rng.random(N) (n - 1)) + 1
  spectrum: the counts tabulated with one pseudo-count per row k = 1 .. n of the USED sizes, over N + those rows; props = the share
  of the sample size among the sites (1e-9 for a size no site carries, whose rows have no neutral probability).
  'wide728'    sizes (300, 426), used (300,): 728 rows, 45 * 728 = 32 760 -> 32 768 bytes: the LAST row count whose workspace is in LDS
  'wide729'    sizes (300, 427), used (300,): 729 rows: the FIRST in the slab.  Sites, counts, windows, g and prop of n = 300 are
               wide728's: the two models hold the same expression for every R entry a site can reach, so their results are equal
  'wide90831'  sizes 300 .. 520, all used: 90 831 rows, 4-byte row indices, a 4.09 MB workspace: the slab cap (512 MiB per launch)
               leaves 131 workgroups, fewer than the 300 windows
Test positions of the wide data: 300, every 5th site from 2 on (six of them the later site of a tie); every third of them is
moved to the midpoint between its site and the next (a test position that is no site).  Windows [i - r, i + r] with r cycling
through WIDE_R, clipped to the chromosome and moved off tied positions as gridshape.windows_of does.  r = 0 at a site is a window
that holds the test position alone: empty for T, so without a grid result.

Grids (x list, alpha_beta list, A list): GRIDS.  'all' has the three coordinates free; 'x', 'u', 'v', 'ux', 'xv', 'uv' free the
named ones (u = ln A, v = ln alpha_beta) and fix the others at 0.3 / 7.0 / 5000.0; 'corner' has two values per axis, so every start
is a hull corner and half of the first round's candidates clamp onto the centre; 'tie' repeats grid values (gridshape.tie_grids);
'wideA' goes with the wide data (its windows hold about 150 sites at A = 5000: refine_R at n = 300 .. 520 stays cheap).

CASES: name -> (data, grid, tests, windows); tests is a stride of gridshape.tests_of or 'wide', windows 'all', 'ragged' or 'wide'.

replay() runs refine.compass for M windows in lockstep on a batched objective and reports each window's smallest decision margin.
"""
import collections

import numpy as np

import gridshape as gs
from ballermixplus_amd import refine

# ----------------------------------------------------------------------------- the wide data
WIDE_SEED = 20261020
WIDE_N = 1500
WIDE_TIES = (41, 251, 611, 612, 901, 1291, 1451)  # genPos[j + 1] = genPos[j]; 611 / 612: three sites on one position
WIDE_SIZES = {'wide728': ((300, 426), (300,)), 'wide729': ((300, 427), (300,)), 'wide90831': (tuple(range(300, 521)),) * 2}
WIDE_ROWS = {'wide728': 728, 'wide729': 729, 'wide90831': 90831}
WIDE_M = 300
WIDE_R = (0, 1, 2, 63, 64, 65, 255, 256, 257)
DATA = ('small', 'large') + tuple(WIDE_SIZES)

Data = collections.namedtuple('Data', 'gen k nn sizes spect props')


def wide(sizes, used=None):
    """Data of the wide recipe: `sizes` in the model, sites drawn from `used` (default: all of them)."""
    sizes = tuple(int(n) for n in sizes)
    used = sizes if used is None else tuple(int(n) for n in used)
    rng = np.random.default_rng(WIDE_SEED)
    N = WIDE_N
    gen = np.cumsum(rng.geometric(0.02, N)) / 1e6
    for j in WIDE_TIES:
        gen[j + 1] = gen[j]
    nn = rng.choice(np.array(used, dtype=np.int64), N)
    k = np.where(rng.random(N) < 0.5, nn, (rng.random(N) * (nn - 1)).astype(np.int64) + 1)
    rows = sum(used)
    spect = {(kk, n): 1.0 / (N + rows) for n in used for kk in range(1, n + 1)}
    for a, b in zip(k.tolist(), nn.tolist()):
        spect[(a, b)] += 1.0 / (N + rows)
    props = {n: float(np.mean(nn == n)) if n in used else 1e-9 for n in sizes}
    return Data(gen, k.astype(np.int64), nn.astype(np.int64), list(sizes), spect, props)


_DATA = {}


def dataset(data):
    """Data(gen, k, nn, sizes, spect, props) of a data set name; the arrays are shared and read-only."""
    if data not in _DATA:
        if data in WIDE_SIZES:
            d = wide(*WIDE_SIZES[data])
        else:
            d = Data(*(gs.chromosome(data) + (gs.sizes_of(data),) + gs.spectrum(data)))
        for a in d[:3]:
            a.setflags(write=False)
        _DATA[data] = d
    return _DATA[data]


def rows_of(data):
    """Table row of every site: one block of n + 1 rows per sample size, ascending n (engine.ModelArrays.rows_of)."""
    d = dataset(data)
    off = dict(zip(d.sizes, np.concatenate(([0], np.cumsum([n + 1 for n in d.sizes])))[:-1].tolist()))
    return (np.array([off[int(n)] for n in d.nn]) + d.k).astype(np.int32)


def wide_tests(gen):
    """(test positions f64[M], site index i64[M], lo, hi, is_site bool[M]) of the wide data."""
    N = len(gen)
    idx = 2 + 5 * np.arange(WIDE_M, dtype=np.int64)
    mid = (np.arange(WIDE_M) % 3 == 1) & (gen[idx] != gen[np.minimum(idx + 1, N - 1)])
    tg = np.where(mid, 0.5 * (gen[idx] + gen[np.minimum(idx + 1, N - 1)]), gen[idx])
    r = np.array(WIDE_R, dtype=np.int64)[np.arange(WIDE_M) % len(WIDE_R)]
    lo, hi = np.maximum(idx - r, 0), np.minimum(idx + r, N - 1)
    for j in range(WIDE_M):                                       # never cut between two sites on one position
        while 0 < lo[j] < N and gen[lo[j] - 1] == gen[lo[j]]:
            lo[j] -= 1
        while 0 <= hi[j] < N - 1 and gen[hi[j] + 1] == gen[hi[j]]:
            hi[j] += 1
    return tg, idx, lo, hi, ~mid


# ----------------------------------------------------------------------------- grids
FIX_X, FIX_AB, FIX_A = 0.3, 7.0, 5000.0


def _subset(free):
    return (gs.x_grid(10) if 'x' in free else [FIX_X], gs.abeta_grid(51) if 'v' in free else [FIX_AB],
            list(gs.A_LIST) if 'u' in free else [FIX_A])


SUBSETS = ('x', 'u', 'v', 'ux', 'xv', 'uv')
GRIDS = {'all': gs.grids_of((5, 13)), 'corner': ([0.2, 0.4], [1.0, 100.0], [2000.0, 20000.0]), 'tie': gs.tie_grids(),
         'wideA': ([0.2, 0.3, 0.4], [1.0, 10.0, 100.0], [5000.0, 30000.0])}
GRIDS.update({name: _subset(name) for name in SUBSETS})
# free coordinates in refine.py's order (u = ln A, x, v = ln alpha_beta)
FREE = {name: ('u' in name, 'x' in name, 'v' in name) for name in SUBSETS}
FREE.update({'all': (True,) * 3, 'corner': (True,) * 3, 'tie': (True,) * 3, 'wideA': (True,) * 3})


def setup_of(grid):
    xs, ab, As = GRIDS[grid]
    return refine.Setup(As, xs, ab)


# ----------------------------------------------------------------------------- cases
Case = collections.namedtuple('Case', 'data grid tests windows')
CASES = collections.OrderedDict()
for _g in ('all', 'corner', 'tie'):
    for _w in ('ragged', 'all'):
        CASES['small-%s-%s' % (_g, _w)] = Case('small', _g, 20, _w)
CASES['large-all-ragged'] = Case('large', 'all', 20, 'ragged')
for _g in SUBSETS:
    CASES['small-%s-ragged' % _g] = Case('small', _g, 20, 'ragged')
for _d in WIDE_SIZES:
    CASES[_d] = Case(_d, 'wideA', 'wide', 'wide')
CASES['stride'] = Case('small', 'all', 1, 'ragged')
REPLAYED = tuple(n for n in CASES if n not in ('stride', 'wide90831'))          # the cases whose refinement is replayed exactly
RAGGED = tuple(n for n, c in CASES.items() if c.windows != 'all')


def tests_of(name):
    """(test positions f64[M], site index i64[M], lo i64[M], hi i64[M], is_site bool[M]) of a case.  The windows are inclusive
    index windows; 'all' is [0, N - 1] (the GPU tests hand it over as 'no index bounds')."""
    c = CASES[name]
    gen = dataset(c.data).gen
    if c.tests == 'wide':
        return wide_tests(gen)
    idx = np.arange(gs.N, dtype=np.int64) if c.tests == 1 else gs.tests_of(c.tests).astype(np.int64)
    lo, hi = gs.windows_of(gen, idx, c.windows)
    return gen[idx], idx, lo, hi, np.ones(len(idx), bool)


# alpha >= 1e-8, the reference's window, as A |g - t| <= zcut: bmx_alpha_cut(), the largest double z with exp(-z) >= 1e-8.  (Not
# -np.log(1e-8): that is 18.420680743952367, one ulp above it, and exp(-18.420680743952367) < 1e-8.  test_cutedge_cpu.py holds
# this constant to the oracle's bisection.)
ZCUT = 18.420680743952364


def window_at(gen, tg, A, lo, hi):
    """Site indices of the window of test position tg at A (alpha >= 1e-8, position != tg, lo <= index <= hi) and their alpha:
    gridshape.window_of for a test position that need not be a site."""
    al = np.exp(-A * np.abs(gen - tg))
    at = np.arange(len(gen))
    keep = (al >= 1e-8) & (gen != tg) & (at >= lo) & (at <= hi)
    return np.nonzero(keep)[0], al[keep]


KINDS = ('empty', 'right', 'tie', 'cut', 'short', 'long', 'off256')


def geometry(name, A=None):
    """bool[M] per kind of KINDS for the case's windows, from the site range [a, b] the kernels sum at A (default: the grid's
    smallest A, the widest range a search can meet), the range of sites with A |g - t| <= zcut inside [max(lo, 0), min(hi, N - 1)]:
      empty   lo > hi                               right   the window lies wholly right of the test position
      tie     two or more sites sit on the test position
      cut     lo or hi cuts the range that A alone would give
      short   1 .. 255 sites in the range          long    more than 512          off256  the range starts off a multiple of 256"""
    c = CASES[name]
    gen = dataset(c.data).gen
    tg, idx, lo, hi, _ = tests_of(name)
    A = min(GRIDS[c.grid][2]) if A is None else A
    N = len(gen)
    a0 = np.searchsorted(gen, tg - ZCUT / A, 'left')
    b0 = np.searchsorted(gen, tg + ZCUT / A, 'right') - 1
    wlo, whi = np.maximum(lo, 0), np.minimum(hi, N - 1)
    a, b = np.maximum(a0, wlo), np.minimum(b0, whi)
    n = np.maximum(b - a + 1, 0)
    empty = wlo > whi
    ties = np.searchsorted(gen, tg, 'right') - np.searchsorted(gen, tg, 'left')
    return {'empty': empty, 'right': ~empty & (gen[np.minimum(wlo, N - 1)] > tg), 'tie': ties >= 2,
            'cut': ~empty & ((wlo > a0) | (whi < b0)) & (n > 0), 'short': (n >= 1) & (n < 256), 'long': n > 512,
            'off256': (n >= 1) & (a % 256 != 0)}


# ----------------------------------------------------------------------------- the replay
def _finite(T):
    T = np.asarray(T, dtype=np.float64)
    return np.where(np.isfinite(T), T, -np.inf)


def naturals(c, c0, nat0, exp=None):
    """refine.natural_of row by row: f64[M, 3] natural (A, x, alpha_beta) of the points c of searches started at c0 / nat0.
    exp: a vectorised exp to stand in for refine.to_natural's math.exp (f64[n] -> f64[n]), the rule unchanged: a coordinate that
    equals the start's keeps the start's natural value, x is its own natural value, A = exp(u), alpha_beta = exp(v)."""
    if exp is None:
        return np.array([refine.natural_of(tuple(p), tuple(q), tuple(n)) for p, q, n in zip(c.tolist(), c0.tolist(), nat0.tolist())]).reshape(len(c), 3)
    c, c0, nat0 = (np.asarray(v, dtype=np.float64).reshape(-1, 3) for v in (c, c0, nat0))
    out = c.copy()
    out[:, [0, 2]] = np.asarray(exp(np.ascontiguousarray(c[:, [0, 2]]).ravel()), dtype=np.float64).reshape(-1, 2)
    return np.where(c == c0, nat0, out)


Replay = collections.namedtuple('Replay', 'c T T0 rounds h margin')


def replay(eval_batch, starts, free, lo, hi, h0, tol=refine.TOL, max_rounds=refine.MAX_ROUNDS):
    """refine.compass for M windows in lockstep: starts f64[M, 3] (u, x, v), h0 f64[M, 3], free / lo / hi / tol of the three
    coordinates.  eval_batch(c f64[M, 3], active bool[M]) -> T f64[M] is called once for the starts and once per direction per
    round in which some window has a candidate (at most 6 max_rounds + 1 calls); rows that are not active (the window has stopped,
    or its candidate clamps onto the centre) carry the window's centre and their T is ignored.
    Returns Replay(c, T, T0, rounds, h, margin): final coordinates, T there, T at the start, rounds, final steps and the
    smallest decision margin of the window's path.  The margin of a round with centre value Tc and candidate values T_i (in order;
    -inf values are ignored): no move: Tc - max T_i; a move to the first maximum `best`: the smaller of best - Tc and best - the
    largest other candidate; divided by max(|Tc|, |best|) (best: the largest candidate).  An exact finite tie is margin 0;
    comparisons against -inf do not count; a window that made no comparison has margin inf.
    The arithmetic of candidates, clamping and halving is refine.compass's, expression for expression."""
    c = np.array(starts, dtype=np.float64).reshape(-1, 3)
    h = np.array(h0, dtype=np.float64).reshape(-1, 3)
    M = len(c)
    fk = [k for k in range(3) if free[k]]
    Tc = _finite(eval_batch(c.copy(), np.ones(M, bool)))
    T0 = Tc.copy()
    rounds = np.zeros(M, np.int32)
    margin = np.full(M, np.inf)
    while True:
        conv = np.all([h[:, k] < tol[k] for k in fk], axis=0) if fk else np.ones(M, bool)
        run = (rounds < max_rounds) & ~conv
        if not run.any():
            break
        best, move = Tc.copy(), np.full(M, -1)
        cand_c = np.zeros((6, M))
        cand_T = np.full((6, M), -np.inf)
        for d in range(6):
            k = d // 2
            if not free[k]:
                continue
            v = np.minimum(np.maximum(c[:, k] + h[:, k] if d & 1 else c[:, k] - h[:, k], lo[k]), hi[k])
            act = run & (v != c[:, k])
            if not act.any():
                continue
            p = c.copy()
            p[act, k] = v[act]
            T = np.where(act, _finite(eval_batch(p, act)), -np.inf)
            cand_c[d], cand_T[d] = v, T
            up = act & (T > best)
            best[up], move[up] = T[up], d
        # the margins: -inf candidates (and the inactive ones, set to -inf above) take no part
        top = cand_T.max(axis=0)
        moved = move >= 0
        rest = cand_T.copy()
        rest[np.maximum(move, 0), np.arange(M)] = np.where(moved, -np.inf, rest[np.maximum(move, 0), np.arange(M)])
        other = rest.max(axis=0)
        with np.errstate(invalid='ignore'):
            m_stay = np.where(np.isfinite(top), Tc - top, np.inf)                          # Tc = -inf and no move: every T_i is -inf
            m_move = np.minimum(np.where(np.isfinite(Tc), best - Tc, np.inf), np.where(np.isfinite(other), best - other, np.inf))
            raw = np.where(moved, m_move, m_stay)
            scale = np.maximum(np.where(np.isfinite(Tc), np.abs(Tc), 0.0), np.where(np.isfinite(top), np.abs(top), 0.0))
            rel = np.where(np.isfinite(raw), raw / np.where(scale > 0, scale, 1.0), np.inf)
        margin = np.where(run, np.minimum(margin, rel), margin)
        for d in range(6):
            at = moved & (move == d)
            c[at, d // 2] = cand_c[d][at]
        Tc = np.where(moved, best, Tc)
        halve = run & ~moved
        h[halve] = h[halve] * 0.5
        rounds[run] += 1
    return Replay(c, Tc, T0, rounds, h, margin)


MARGIN_BAR = 1e-12          # a window is judged when its smallest margin is at least this
JUDGED_SHARE = 0.8          # at least this share of a case's refined windows must be judged
