"""Lattice chromosomes whose window cut falls within one ulp of a site, and the host restatement of the cut: the input of
tests/test_cutedge_cpu.py and tests/test_gpu_cut_edge.py.  numpy and the oracle's cut (orc.alpha_cut_z) only; the one figure taken
from a selection table (the largest P_sel of the loud row over the grid) is handed in by the caller.

Why.  A site belongs to a window at linkage value A when A * |g_i - t| <= zcut and g_i != t (zcut = bmx_alpha_cut(), the largest
double z with exp(-z) >= 1e-8: the reference's np.exp(-A * dist) >= 1e-8).  bmxscan.hip states that predicate in more than a dozen
places (the per-site, grouped, prepared and solo scan kernels, prep_kernel's bulk test and ragged-end bisection, the triangle
shortcut between the test sites of a group, finalize_kernel's two binary searches, the refine family's range search, the planting
range).  Random positions never put a site within an ulp of the cut, and a site AT the cut has alpha = 1e-8: it moves T by
2 log1p(1e-8 R), under the rtol 1e-9 bar unless R is large.  Here the positions are lattices, A is chosen per neighbour rank K so
that the K-th neighbour sits on the cut, and one loud row gives the sites at the cut an R the bar can see.

Positions (N = 4096 sites):
  'dyadic'   g_i = i 2^-17: every distance is exact.  A_in(K) is the largest A with A (K h) <= zcut, A_out(K) = nextafter(A_in, inf):
             the K-th neighbour of EVERY test site is in at A_in and out at A_out.
  'decimal'  g_i = fl(i 1e-5): the distances g_{t+K} - g_t take a handful of values an ulp or so apart.  A0(K) = zcut / median(d_K)
             and its neighbours one ulp down and up: the K-th neighbour is in for some windows and out for others, decided in the
             last bit.
  'runs'     'decimal' with every 50th position (25, 75, ...) held by three sites: a boundary can be a run that goes in or out
             together; a run between two test sites of a group also switches the scan kernels' triangle shortcut off.
K list: KS (around the group sizes 4 / 8 / 16, the wave and the 64-position ragged-end bisection), and A_NONE = 1e7, at which no
site is in reach of any other (A h = 76 and 100).  d_K is taken over the distinct positions, so that K counts positions in 'runs'.

Model: B_2, min count 1, the 3 x 3 grid XS x ABETAS, sample size 30 -- or (150, 160, 170) for the set that reads R from L2.
Neutral spectrum g(k, n) = prop_n P_sel(k | HOME) / (1 + LIFT) on k = 1 .. n, equal props: the selection model of the grid point HOME
(x = 0.5, alpha_beta = 0.5), by the oracle's table, lowered by LIFT = 5 %.  R is then LIFT on every row at HOME, so T(HOME) > 0 on
every window that holds a site: the scan reports only positive T, and a comparison of all-zero rows shows nothing.  (With g ~ 1 / k
a quarter of the windows at K = 1, and some up to K = 15, had no winner.  The spectrum sums to 1 / 1.05; the library does not ask
for a checksum.)  All draws from ONE np.random.default_rng(SEED) in this order: the sample size rng.integers(0, len(sizes), N);
u = rng.random(N), the count by the inverse CDF of P_sel(. | HOME).  The LOUD
row (7, n_0) (n_0 the smallest size) is then placed at every 7th site, and its neutral probability set as tablespan.spectrum sets
it: g = sel_max prop / 2^(span - 1/2), so that log2(1 + max R) = span - 1/2 -- for spans 12, 22 and 30.  At the cut alpha R is then
3e-5, 0.03 and 7: far to third order, far to eighth order, near.  Span 0: no loud row is placed.
Data sets: SETS.  Test sites: every stride-th site, strides 1, 5 and 20 (prepared J = 16, J = 8, solo), windows the whole
chromosome; index windows [t - K - e, t + K + e], e = 0, -1, 1, put the window's own bound on, inside and outside the site the cut
decides.

Measured with the committed seed (tests/test_cutedge_cpu.py asserts the conditions and prints the figures): see DESIGN.md."""
import functools

import numpy as np

from util import orc

SEED = 20261021
N = 4096
H = {'dyadic': 2.0 ** -17, 'decimal': 1e-5, 'runs': 1e-5}
LAYOUTS = ('dyadic', 'decimal', 'runs')
KS = (1, 3, 4, 7, 8, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 200)
A_NONE = 1e7
XS = [0.1, 0.3, 0.5]
ABETAS = [0.5, 20.0, 1e4]
LOUD_K, LOUD_EVERY = 7, 7
RUN_EVERY, RUN_AT, RUN_LEN = 50, 25, 3
SMALL, LARGE = (30,), (150, 160, 170)
MARGIN = 0.5                                    # log2(1 + max R) = span - MARGIN
STRIDES = (1, 5, 20)
HOME = (2, 0)                                   # (ix, ia) of the grid point the neutral spectrum is shaped after
LIFT = 0.05                                     # ... and lies below by: R = LIFT on every row but the loud one at that point
EVAL_POINT = (1, 1)                            # (ix, ia) of the fixed (x, alpha_beta) of the point evaluations
TIE_BAR = 1e-7                                  # multi-A scan: a runner-up A within TIE_BAR * T of the winner is a near-tie
TIE_CAP = 0.05                                  # ... and at most this share of a set's windows may be one
SENS_FACTOR = 100.0                             # a sensitive window moves by SENS_FACTOR * (1e-9 |T| + 1e-12) with its boundary site
QUIET_FACTOR = 10.0                             # ... the factor of the set without a loud row (test_cutedge_cpu.py says why)

# name -> (layout, span of the loud row or 0, sample sizes)
SETS = {'dyadic12': ('dyadic', 12, SMALL), 'decimal0': ('decimal', 0, SMALL), 'decimal12': ('decimal', 12, SMALL),
        'decimal22': ('decimal', 22, SMALL), 'decimal30': ('decimal', 30, SMALL), 'runs12': ('runs', 12, SMALL),
        'large12': ('decimal', 12, LARGE)}
LOUD_SETS = tuple(s for s in SETS if SETS[s][1] > 0)


def zcut():
    """The cut, from the oracle's bisection on numpy's exp -- never from a logarithm."""
    return orc.alpha_cut_z()


# ----------------------------------------------------------------------------- positions and rows
@functools.lru_cache(maxsize=None)
def positions(layout):
    i = np.arange(N, dtype=np.float64)
    if layout == 'dyadic':
        g = i * H['dyadic']
    elif layout == 'decimal':
        g = i * H['decimal']
    elif layout == 'runs':
        q = np.repeat(np.arange(N), np.where(np.arange(N) % RUN_EVERY == RUN_AT, RUN_LEN, 1))[:N]
        g = q.astype(np.float64) * H['runs']
    else:
        raise ValueError(layout)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _shape(n):
    """P_sel(k | HOME) on k = 1 .. n, by the oracle's table."""
    p = orc.sel_table('B2', int(n), 1, [XS[HOME[0]]], [ABETAS[HOME[1]]])[0, 0, 1:]
    assert np.all(p > 0) and abs(p.sum() - 1.0) < 1e-9
    return p


def base_spectrum(sizes):
    """({(k, n): g}, props): g = prop P_sel(k | HOME) / (1 + LIFT) on k = 1 .. n, equal props."""
    props = {int(n): 1.0 / len(sizes) for n in sizes}
    spect = {}
    for n in sizes:
        for k, v in zip(range(1, n + 1), _shape(n).tolist()):
            spect[(k, int(n))] = props[int(n)] * v / (1.0 + LIFT)
    return spect, props


@functools.lru_cache(maxsize=None)
def counts(sizes, loud):
    """(count i64[N], total i64[N]): drawn from base_spectrum(sizes); with `loud`, the loud row on every LOUD_EVERY-th site."""
    rng = np.random.default_rng(SEED)
    nn = np.asarray(sizes, dtype=np.int64)[rng.integers(0, len(sizes), N)]
    u = rng.random(N)
    k = np.zeros(N, dtype=np.int64)
    for n in sizes:
        cdf = np.cumsum(_shape(n))
        at = nn == n
        k[at] = 1 + np.minimum(np.searchsorted(cdf / cdf[-1], u[at], 'right'), n - 1)
    if loud:
        k[::LOUD_EVERY] = LOUD_K
        nn[::LOUD_EVERY] = sizes[0]
    k.setflags(write=False)
    nn.setflags(write=False)
    return k, nn


def loud_row(sizes):
    return (LOUD_K, int(sizes[0]))


def spectrum(sizes, span, sel_max):
    """base_spectrum with the loud row placed at `span` (0: left alone).  sel_max: the largest P_sel of the loud row over the grid
    (the oracle's sel_table('B2', n_0, 1, XS, ABETAS)[:, :, LOUD_K].max())."""
    spect, props = base_spectrum(sizes)
    if span:
        e = loud_row(sizes)
        spect[e] = float(sel_max) * props[e[1]] / 2.0 ** (span - MARGIN)
    return spect, props


def rows_of(sizes, k, nn):
    """Table row of every site: one block of n + 1 rows per sample size, ascending n (engine.ModelArrays.rows_of)."""
    sizes = sorted(int(n) for n in sizes)
    off = dict(zip(sizes, np.concatenate(([0], np.cumsum([n + 1 for n in sizes])))[:-1].tolist()))
    return (np.array([off[int(n)] for n in nn]) + k).astype(np.int32)


def dataset(name):
    """(gen f64[N], count, total, rows i32[N], sizes, span) of a data set of SETS."""
    layout, span, sizes = SETS[name]
    k, nn = counts(sizes, span > 0)
    return positions(layout), k, nn, rows_of(sizes, k, nn), sizes, span


def tests_of(stride):
    return np.arange(0, N, stride, dtype=np.int64)


def whole(idx):
    return np.zeros(len(idx), np.int64), np.full(len(idx), N - 1, np.int64)


def index_windows(idx, K, e):
    """[t - K - e, t + K + e], clipped to the chromosome."""
    idx = np.asarray(idx, dtype=np.int64)
    return np.maximum(idx - K - e, 0), np.minimum(idx + K + e, N - 1)


# ----------------------------------------------------------------------------- the A values
def d_K(layout, K):
    """The distances between a position and the K-th position after it, over the distinct positions."""
    u = np.unique(positions(layout))
    return u[K:] - u[:-K]


def A_in(K, z=None, d=None):
    """The largest A with A * d <= zcut; d = K h of 'dyadic' (exact) unless given."""
    z = zcut() if z is None else z
    d = K * H['dyadic'] if d is None else d
    A = z / d
    while A * d > z:
        A = np.nextafter(A, 0.0)
    while np.nextafter(A, np.inf) * d <= z:
        A = np.nextafter(A, np.inf)
    return float(A)


def A0(layout, K, z=None):
    z = zcut() if z is None else z
    return float(z / np.median(d_K(layout, K)))


@functools.lru_cache(maxsize=None)
def A_values(layout):
    """((K, A), ...): per K of KS the ulp-stepped A values, ascending, and (0, A_NONE) last.  'dyadic': (A_in, A_out).  Elsewhere
    A0 - 1 ulp, A0, A0 + 1 ulp and the pair that puts the MEDIAN distance on the cut as A_in / A_out put K h there (the largest A with
    A median(d_K) <= zcut and the next double): one ulp of A moves the product by less than the step between two distances, so
    without that pair the three values around A0 can leave a K with every neighbour in (K = 16: 3 090 of 4 080 distances are the
    median, five are larger)."""
    out = []
    for K in KS:
        if layout == 'dyadic':
            a = A_in(K)
            out += [(K, a), (K, float(np.nextafter(a, np.inf)))]
        else:
            a = A0(layout, K)
            m = A_in(K, d=float(np.median(d_K(layout, K))))
            out += [(K, v) for v in sorted({float(np.nextafter(a, 0.0)), a, float(np.nextafter(a, np.inf)), m, float(np.nextafter(m, np.inf))})]
    return tuple(out) + ((0, A_NONE),)


def A_list(layout):
    """The multi-A scan's list: one A per K (A_in on 'dyadic', A0 elsewhere), no ulp neighbours."""
    return [A_in(K) if layout == 'dyadic' else A0(layout, K) for K in KS]


# ----------------------------------------------------------------------------- the host restatement of the cut
def exact(z):
    """The predicate as the reference's arithmetic has it: one multiplication, one comparison."""
    return lambda A, d: A * d <= z


def by_division(z):
    """WRONG on purpose (test_cutedge_cpu.py's mutation check): a precomputed reach d_max = zcut / A."""
    return lambda A, d: d <= z / A


def reach(gen, ti, A, inside):
    """Inclusive index range (a i64[M], b i64[M]) of the sites i with inside(A, |g_i - g_ti|) around the test SITES ti -- the site
    itself is inside (d = 0), and the predicate is monotone on either side of it.  A: a scalar or f64[M]."""
    ti = np.asarray(ti, dtype=np.int64)
    tg = gen[ti]
    A = np.broadcast_to(np.asarray(A, dtype=np.float64), ti.shape)
    n = len(gen)
    guess = 18.420680743952364 / A
    a = np.minimum(np.searchsorted(gen, tg - guess, 'left'), ti)
    b = np.maximum(np.searchsorted(gen, tg + guess, 'right') - 1, ti)

    def ok(i):
        return (i >= 0) & (i < n) & inside(A, np.abs(gen[np.clip(i, 0, n - 1)] - tg))
    while True:
        m = ok(a - 1)
        if not m.any():
            break
        a = np.where(m, a - 1, a)
    while True:
        m = ~ok(a)
        if not m.any():
            break
        a = np.where(m, a + 1, a)
    while True:
        m = ok(b + 1)
        if not m.any():
            break
        b = np.where(m, b + 1, b)
    while True:
        m = ~ok(b)
        if not m.any():
            break
        b = np.where(m, b - 1, b)
    return a, b


def n_sites(gen, ti, A, inside, lo=None, hi=None):
    """nSites i64[M]: the sites in reach inside the index window [lo, hi], those on the test position excluded."""
    ti = np.asarray(ti, dtype=np.int64)
    a, b = reach(gen, ti, A, inside)
    if lo is not None:
        a, b = np.maximum(a, lo), np.minimum(b, hi)
    tl = np.searchsorted(gen, gen[ti], 'left')
    tr = np.searchsorted(gen, gen[ti], 'right') - 1
    ties = np.maximum(np.minimum(tr, b) - np.maximum(tl, a) + 1, 0)
    return np.maximum(b - a + 1, 0) - ties


def host_T(gen, rows, Rp, ti, A, inside, lo=None, hi=None):
    """(T f64[M], nSites i64[M]) at one grid point: T = 2 sum log1p(exp(-(A d)) Rp[row]) over the window, in site order; -inf where
    the window is empty.  Rp f64[rows]: the table column of the grid point."""
    ti = np.asarray(ti, dtype=np.int64)
    A = np.broadcast_to(np.asarray(A, dtype=np.float64), ti.shape)
    a, b = reach(gen, ti, A, inside)
    if lo is not None:
        a, b = np.maximum(a, lo), np.minimum(b, hi)
    W = int(max((b - a + 1).max(), 1))
    at = a[:, None] + np.arange(W)[None, :]
    j = np.clip(at, 0, len(gen) - 1)
    keep = (at <= b[:, None]) & (gen[j] != gen[ti][:, None])
    al = np.exp(-(A[:, None] * np.abs(gen[j] - gen[ti][:, None])))
    with np.errstate(divide='ignore', invalid='ignore'):
        T = 2.0 * np.sum(np.where(keep, np.log1p(al * Rp[rows[j]]), 0.0), axis=1)
    ns = keep.sum(axis=1)
    return np.where(ns > 0, T, -np.inf), ns


def boundary_sites(gen, ti, A, inside):
    """(far i64[M], near i64[M]): the farthest in-site and the nearest out-site of every window, -1 where there is none."""
    ti = np.asarray(ti, dtype=np.int64)
    tg = gen[ti]
    n = len(gen)
    a, b = reach(gen, ti, A, inside)
    far = np.where(tg - gen[a] >= gen[b] - tg, a, b)
    far = np.where(gen[far] != tg, far, -1)
    dl = np.where(a > 0, tg - gen[np.maximum(a - 1, 0)], np.inf)
    dr = np.where(b < n - 1, gen[np.minimum(b + 1, n - 1)] - tg, np.inf)
    near = np.where(dl <= dr, a - 1, b + 1)
    near = np.where(np.isfinite(np.minimum(dl, dr)), near, -1)
    return far, near


def near_ties(T):
    """bool[M] of T f64[M, nA] (one column per A, each the maximum over the pair grid, 0 where nothing is positive): the runner-up
    column lies within TIE_BAR * T of the winner."""
    s = np.sort(T, axis=1)
    best, second = s[:, -1], s[:, -2]
    return (best > 0) & (best - second <= TIE_BAR * best)
