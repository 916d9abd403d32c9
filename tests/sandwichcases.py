"""The cases of the --sandwich tests: chromosomes, models, windows, points and blocks, built on the host alone.
tests/test_sandwich_cpu.py proves with the oracle's table that the catalogue holds what it claims (window sizes, a tie inside a
block, range starts off a block boundary, regular H, no skipped site but the planned one); tests/test_gpu_sandwich.py runs the
same cases on the device.

Chromosome.  N = 3600 sites, all draws from ONE np.random.default_rng(SEED) in this order: genPos = cumsum(geometric(0.02, N)) /
1e6 (about 5e-5 between sites), then genPos[j + 1] = genPos[j] for j in TIES (runs of two, three and four sites on one position);
the sample size rng.choice(sizes, N); the count: n where rng.random(N) < 0.5, else floor(rng.random(N) (n - 1)) + 1.  Spectrum: the
counts tabulated with one pseudo-count per row k = 1 .. n; props: the share of the sample size among the sites.

Cases (name -> sizes):  'one' (100,): n = 100 alone;  'three' (60, 100, 140);  'slab' tests/offgrid.py's wide729 (729 table rows:
the first count whose workspace lies in the slab, not in LDS), its own 1 500 sites, grid and ten of its windows;  'skip': forty
sites of sizes 7 and 20 where the model gives size 7 the share 0.0, so R = -1 on its rows, and one site of size 7 stands 1e-20
from the test position: alpha = exp(-A 1e-20) = 1.0 exactly, D = 0, the site is skipped.

Grid of 'one' and 'three': A in A_LIST, x in XS, alpha_beta in ABETAS.  The cut reaches +-3.7e-3 (about 150 sites) at A = 5000,
+-2.6e-2 (about 1 050 sites) at A = 700 and the whole chromosome at A = 50.

Windows (WINDOWS: test position, lo, hi).  For every s of SIZES a test site i with the index window [i - s // 2, i - s // 2 + s]:
s sites besides the test site, cut by win_lo / win_hi and not by the cut at A <= 700; then, with no index bounds, the middle site of
the run of three (two more sites AT the test position, inside a block of every B >= 2), a position between two sites, a window at
either end of the chromosome.

Points (POINTS: A, x, alpha_beta): one on the grid (interior in every coordinate), two off it; alpha_beta <= 1e3.
Entries: every window at every point.  BLOCKS = (1, 2, 7, 64, 100, 10 ** 6).
"""
import collections
import math
import os
import re

import numpy as np

from util import REPO, oracle_R         # (first: util puts the repository on sys.path)
import offgrid as og

from ballermixplus_amd import refine, sandwich

SEED = 20261020
N = 3600
TIES = (40, 41, 42, 700, 1500, 1501, 2999)
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257)
A_LIST = (50.0, 700.0, 5000.0, 30000.0)
XS = (0.1, 0.3, 0.5)
ABETAS = (1.0, 10.0, 100.0, 1000.0)
POINTS = ((700.0, 0.3, 10.0), (50.0, 0.137, 3.3), (5210.7, 0.41, 731.0))
SLAB_POINTS = ((5000.0, 0.3, 10.0), (7000.0, 0.33, 42.0), (5000.0, 0.25, 3.3))
SKIP_POINTS = ((100.0, 0.3, 10.0),)
BLOCKS = (1, 2, 7, 64, 100, 10 ** 6)
NAMES = ('one', 'three', 'slab', 'skip')
ZCUT = og.ZCUT
TOL = 1e-12                 # the GPU comparison's bar: of |T| for T, of the sum of the absolute terms for every entry of g, H, J
R_TOL = 1e-9                # Context.refine_R against the oracle, relative on 1 + R

Case = collections.namedtuple('Case', 'name gen k nn sizes spect props rows xs abetas As tg lo hi points entries')


def header_constant(name):
    """An integer #define of include/bmxscan.h written as a literal or as `(aLL << b)`."""
    with open(os.path.join(REPO, 'include', 'bmxscan.h')) as f:
        m = re.search(r'#define\s+%s\s+\(?\s*(\d+)(?:LL)?\s*(?:<<\s*(\d+))?\s*\)?' % name, f.read())
    return int(m.group(1)) << int(m.group(2) or 0)


def _rows(sizes, k, nn):
    off = dict(zip(sizes, np.concatenate(([0], np.cumsum([n + 1 for n in sizes])))[:-1].tolist()))
    return (np.array([off[int(n)] for n in nn]) + k).astype(np.int32)


def _spectrum(sizes, k, nn):
    rows = sum(sizes)
    spect = {(kk, n): 1.0 / (len(k) + rows) for n in sizes for kk in range(1, n + 1)}
    for a, b in zip(k.tolist(), nn.tolist()):
        spect[(a, b)] += 1.0 / (len(k) + rows)
    return spect, {n: float(np.mean(nn == n)) for n in sizes}


def chromosome(sizes):
    rng = np.random.default_rng(SEED)
    gen = np.cumsum(rng.geometric(0.02, N)) / 1e6
    for j in TIES:
        gen[j + 1] = gen[j]
    nn = rng.choice(np.array(sizes, dtype=np.int64), N)
    k = np.where(rng.random(N) < 0.5, nn, (rng.random(N) * (nn - 1)).astype(np.int64) + 1)
    return gen, k.astype(np.int64), nn.astype(np.int64)


def windows(gen):
    """(tg f64[M], lo i64[M], hi i64[M]) of WINDOWS."""
    tg, lo, hi = [], [], []
    for j, s in enumerate(SIZES):
        i = 500 + 137 * j
        assert gen[i - 1] < gen[i] < gen[i + 1]
        tg.append(gen[i]); lo.append(i - s // 2); hi.append(i - s // 2 + s)
    for t in (gen[1501], 0.5 * (gen[2000] + gen[2001]), gen[5], gen[N - 3]):
        tg.append(t); lo.append(0); hi.append(N - 1)
    return np.array(tg), np.array(lo, dtype=np.int64), np.array(hi, dtype=np.int64)


def _main(name, sizes):
    gen, k, nn = chromosome(sizes)
    spect, props = _spectrum(sizes, k, nn)
    tg, lo, hi = windows(gen)
    entries = [(w, p) for w in range(len(tg)) for p in range(len(POINTS))]
    return Case(name, gen, k, nn, list(sizes), spect, props, _rows(sizes, k, nn), XS, ABETAS, A_LIST, tg, lo, hi, POINTS, entries)


def _slab():
    d = og.dataset('wide729')
    xs, ab, As = og.GRIDS['wideA']
    tg, idx, lo, hi, _ = og.wide_tests(d.gen)
    pick = np.arange(4, og.WIDE_M, 30)
    entries = [(w, p) for w in range(len(pick)) for p in range(len(SLAB_POINTS))]
    return Case('slab', d.gen, d.k, d.nn, list(d.sizes), d.spect, d.props, og.rows_of('wide729'), tuple(xs), tuple(ab), tuple(As),
                tg[pick], lo[pick], hi[pick], SLAB_POINTS, entries)


def _skip():
    sizes = (7, 20)
    n_sites = 40
    gen = np.concatenate(([0.0, 1e-20], 1e-4 * np.arange(1, n_sites - 1)))
    nn = np.full(n_sites, 20, dtype=np.int64)
    nn[1] = 7
    k = (1 + np.arange(n_sites) % 19).astype(np.int64)
    k[1] = 3
    spect, _ = _spectrum(sizes, k, nn)
    props = {7: 0.0, 20: 1.0}
    return Case('skip', gen, k, nn, list(sizes), spect, props, _rows(sizes, k, nn), (0.1, 0.3, 0.5), (1.0, 10.0, 100.0), (10.0, 100.0, 1000.0),
                np.array([0.0]), np.array([0], dtype=np.int64), np.array([n_sites - 1], dtype=np.int64), SKIP_POINTS, [(0, 0)])


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = {'one': lambda: _main('one', (100,)), 'three': lambda: _main('three', (60, 100, 140)), 'slab': _slab,
                        'skip': _skip}[name]()
        for a in _CASES[name][1:4]:
            a.setflags(write=False)
    return _CASES[name]


def setup_of(c):
    return refine.Setup(c.As, c.xs, c.abetas)


def model_of(c, eng):
    """(ModelArrays, rows) of a case for the device."""
    m = eng.ModelArrays('B2', 1, c.sizes, c.spect, c.props, c.xs, c.abetas)
    assert np.array_equal(m.rows_of(c.k, c.nn), c.rows)
    return m


def context(c, eng):
    ctx = eng.Context(0)
    ctx.set_model(model_of(c, eng), c.As)
    ctx.set_sites(c.gen, c.rows)
    ctx.set_tests(c.tg, c.lo, c.hi)
    return ctx


_TABS = {}


def oracle_tabs(c, p, hx=sandwich.HX, hv=sandwich.HV):
    """tabs[5][table rows] of point p of the case by the ORACLE's sel_table, at sandwich.shifted_points()."""
    key = (c.name, p, hx, hv)
    if key not in _TABS:
        _, x, ab = c.points[p]
        with np.errstate(all='ignore'):
            t = np.array([oracle_R('B2', c.sizes, 1, c.spect, c.props, [xx], [aa])[0, 0] for xx, aa in sandwich.shifted_points(x, ab, hx, hv)])
        t.setflags(write=False)
        _TABS[key] = t
    return _TABS[key]


def host(c, q, tabs, block, hx=sandwich.HX, hv=sandwich.HV, zcut=ZCUT):
    """host_sandwich of entry q on the five columns tabs."""
    w, p = c.entries[q]
    return sandwich.host_sandwich(c.gen, c.rows, tabs, c.points[p][0], c.tg[w], c.lo[w], c.hi[w], block, hx, hv, zcut)


def site_range(c, q, zcut=ZCUT):
    """[a, b): the sites the cut and the index window leave at entry q's A (the test position's own sites included)."""
    w, p = c.entries[q]
    A = c.points[p][0]
    lo, hi = max(int(c.lo[w]), 0), min(int(c.hi[w]), len(c.gen) - 1)
    z = A * np.abs(c.gen - c.tg[w])
    at = np.nonzero((z <= zcut) & (np.arange(len(c.gen)) >= lo) & (np.arange(len(c.gen)) <= hi))[0]
    return (int(at[0]), int(at[-1]) + 1) if len(at) else (lo, lo)


def literal(c, q, tabs, block, hx=sandwich.HX, hv=sandwich.HV, zcut=ZCUT):
    """The definition as a per-site Python loop (the check of host_sandwich): (T, g[3], H[6], J[6], nsites, nskipped, nblocks)."""
    w, p = c.entries[q]
    A, tg = float(c.points[p][0]), float(c.tg[w])
    g, H, J = [0.0] * 3, [0.0] * 6, [0.0] * 6
    T, ns, nsk = 0.0, 0, 0
    S = {}
    for i in range(max(int(c.lo[w]), 0), min(int(c.hi[w]), len(c.gen) - 1) + 1):
        gi = float(c.gen[i])
        z = A * abs(gi - tg)
        if not z <= zcut or gi == tg:
            continue
        ns += 1
        r = int(c.rows[i])
        al = math.exp(-z)
        R0 = float(tabs[0][r])
        Rx = (float(tabs[2][r]) - float(tabs[1][r])) / (2.0 * hx)
        Rv = (float(tabs[4][r]) - float(tabs[3][r])) / (2.0 * hv)
        D = 1.0 + al * R0
        if not D > 0.0:
            nsk += 1
            continue
        s = (-z * (al * R0) / D, al * Rx / D, al * Rv / D)
        if not all(math.isfinite(v) for v in s):
            nsk += 1
            continue
        T += math.log1p(al * R0)
        Sb = S.setdefault(i // block, [0.0] * 3)
        for k in range(3):
            g[k] += s[k]
            Sb[k] += s[k]
        for e, (k, l) in enumerate(sandwich.SYM):
            H[e] += s[k] * s[l]
    for Sb in S.values():
        for e, (k, l) in enumerate(sandwich.SYM):
            J[e] += Sb[k] * Sb[l]
    return (2.0 * T if ns > nsk else -math.inf), g, H, J, ns, nsk, len(S)


def replicated(c, m):
    """The case with every site standing m times at its position (np.repeat): (gen, rows, lo, hi) of the replicated array; a
    window [lo, hi] becomes [m lo, m hi + m - 1], so blocks of m are aligned with the copies."""
    return np.repeat(c.gen, m), np.repeat(c.rows, m), c.lo * m, c.hi * m + (m - 1)


def fd_error(tabs, half, g, hx, hv, alpha=1.0):
    """Information-weighted relative error of the central differences at (hx, hv) (tabs: the five columns) against those at half
    the steps (half: the five columns at (hx / 2, hv / 2)), per coordinate (x, v).  A site at distance alpha carries the
    information sum_r g_r (alpha R'_r)^2 / (1 + alpha R_r) about a coordinate (the expectation of its squared score under the
    neutral spectrum g); the error is sqrt(sum_r w_r (d_r - dhalf_r)^2 / sum_r w_r dhalf_r^2) with those weights
    w_r = g_r alpha^2 / (1 + alpha R_r), over the rows with a neutral probability."""
    out = []
    for a, b, h in ((1, 2, hx), (3, 4, hv)):
        d = (tabs[b] - tabs[a]) / (2.0 * h)
        dh = (half[b] - half[a]) / h
        ok = np.isfinite(d) & np.isfinite(dh) & np.isfinite(tabs[0]) & np.isfinite(g) & (1.0 + alpha * tabs[0] > 0.0)
        wgt = g[ok] * alpha ** 2 / (1.0 + alpha * tabs[0][ok])
        out.append(math.sqrt(float(np.sum(wgt * (d[ok] - dh[ok]) ** 2)) / float(np.sum(wgt * dh[ok] ** 2))))
    return tuple(out)


def g_of(c):
    """g f64[table rows] of the case's spectrum (NaN: no neutral probability)."""
    off = np.concatenate(([0], np.cumsum([n + 1 for n in c.sizes])))
    g = np.full(int(off[-1]), np.nan)
    for (k, n), v in c.spect.items():
        g[off[c.sizes.index(n)] + k] = v
    return g
