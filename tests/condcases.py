"""The cases of the --conditional tests: chromosomes, models, test sites and pairs, built on the host alone, the literal per-site
statement of the three-way mixture, and the planted demonstration.  test_conditional_cpu.py checks the host restatement
(ballermixplus_amd/conditional.py) against them; test_gpu_conditional.py runs the same chromosomes on the device.  The
chromosomes of `ragged` and `edges` are influencecases.py's recipes."""
import functools
import math

import numpy as np

import influencecases as ic
import powercases as pc
from util import orc

from ballermixplus_amd import conditional, influence, peaks, power, surfaces

SITE_TOL = 1e-12            # the CPU checks: |dT| <= SITE_TOL * (nsites + sum_i |term_i|) per grid point (the fit tests' per-site figure)
REL_TOL = 1e-9              # the GPU comparison: of max over the grid of 2 sum_i |term_i| of the HOST restatement
NAMES = ('ex1_B2', 'ex1_B2_fixX_fixAlpha_listA', 'ex1_B2_w50_s25', 'ragged')
COUNTS = ic.COUNTS


def zcut():
    return orc.alpha_cut_z()


def decode(lin, nx, nab):
    """(iA, ix, ia) of a linear grid index."""
    return lin // (nx * nab), (lin // nab) % nx, lin % nab


def host_pair(cat, R, t, c, lin_c, scale=False, zc=None):
    """conditional.host_cond_surface of the pair (test site t | test site c at lin_c) of a Cat on the table R."""
    zc = zcut() if zc is None else zc
    if c < 0 or lin_c < 0:
        return conditional.host_cond_surface(cat.gen, cat.rows, R, cat.As, cat.tg[t], cat.lo[t], cat.hi[t], None, 0, -1, 0.0, 0, 0, zc,
                                             scale=scale)
    iA, ix, ia = decode(int(lin_c), len(cat.xs), len(cat.ab))
    return conditional.host_cond_surface(cat.gen, cat.rows, R, cat.As, cat.tg[t], cat.lo[t], cat.hi[t], cat.tg[c], cat.lo[c], cat.hi[c],
                                         cat.As[iA], ix, ia, zc, scale=scale)


def literal_cond(genpos, rows, g_row, R, A, tg, lo, hi, tc, clo, chi, A_c, ix_c, ia_c, zc):
    """The definition as a per-site Python loop in PROBABILITY space: with g the neutral probability of the site's row,
    f = g (1 + R) and f_c = g (1 + R_c),
        term = log((1 - a) ((1 - ac) g + ac f_c) + a f) - log((1 - ac) g + ac f_c)
    (ac = 0 for a site that is not shared).  Returns (T[nA][nx][nab], nsites[nA], nshared[nA], S[nA][nx][nab] = sum |term|,
    T3[nA][nx][nab] = 2 sum (log(numerator) - log g): the three-way mixture against neutrality, L[nA] = 2 sum log1p(d_i))."""
    nx, nab = np.asarray(R).shape[:2]
    nA = len(A)
    T, S, T3 = np.full((nA, nx, nab), np.nan), np.zeros((nA, nx, nab)), np.full((nA, nx, nab), np.nan)
    ns, nsh, L = np.zeros(nA, dtype=np.int32), np.zeros(nA, dtype=np.int32), np.zeros(nA)
    first, last = max(int(lo), 0), min(int(hi), len(genpos) - 1)
    for iA in range(nA):
        acc = [[0.0] * nab for _ in range(nx)]
        acc_abs = [[0.0] * nab for _ in range(nx)]
        acc3 = [[0.0] * nab for _ in range(nx)]
        for i in range(first, last + 1):
            gi = float(genpos[i])
            z = float(A[iA]) * abs(gi - float(tg))
            if not z <= zc or gi == float(tg):
                continue
            ns[iA] += 1
            r = int(rows[i])
            g = float(g_row[r])
            a, ac, fc = math.exp(-z), 0.0, g
            if tc is not None and max(int(clo), 0) <= i <= min(int(chi), len(genpos) - 1):
                zcc = float(A_c) * abs(gi - float(tc))
                if zcc <= zc and gi != float(tc):
                    nsh[iA] += 1
                    ac = math.exp(-zcc)
                    fc = g * (1.0 + float(R[ix_c][ia_c][r]))
                    L[iA] += 2.0 * math.log1p(ac * float(R[ix_c][ia_c][r]))
            den = (1.0 - ac) * g + ac * fc
            for ix in range(nx):
                for ia in range(nab):
                    f = g * (1.0 + float(R[ix][ia][r]))
                    num = (1.0 - a) * den + a * f
                    term = math.log(num) - math.log(den)
                    acc[ix][ia] += term
                    acc_abs[ix][ia] += abs(term)
                    acc3[ix][ia] += math.log(num) - math.log(g)
        if ns[iA]:
            T[iA], S[iA], T3[iA] = 2.0 * np.array(acc), np.array(acc_abs), 2.0 * np.array(acc3)
    return T, ns, nsh, S, T3, L


# ------------------------------------------------------------------------------------------ the small chromosome (CPU)

@functools.lru_cache(maxsize=None)
def small():
    """300 sites of sample sizes 20 and 24 drawn from powercases' analytic spectrum (every row a site can stand on has g > 0), a
    3 x 2 x 3 grid, and test sites: four site positions and an off-site one, whole-chromosome windows but for one that cuts."""
    c = pc.Planted('B2', 1, (20, 24), 300, 23, [0.2, 0.5], [0.5, 5.0, 50.0], [400.0, 2000.0, 15000.0], (1, 1, 1))
    N = len(c.gen)
    c.tg = np.array([c.gen[60], c.gen[150], 0.5 * (c.gen[170] + c.gen[171]), c.gen[200], c.gen[290]])
    c.lo = np.array([0, 0, 0, 120, 0], dtype=np.int64)
    c.hi = np.array([N - 1, N - 1, N - 1, 185, N - 1], dtype=np.int64)
    return c


# ------------------------------------------------------------------------------------------------ the GPU's chromosomes

def example(name):
    return ic._example(name, [0, 400, -1])


def edges(eng, seed=4):
    """influencecases.edges' chromosome (700 sites around the off-site position 1.0, three at one position far out) with the A
    grid of the qualifying counts 0, 1, 255, 256, 257, 512, 513 around 1.0 -- boundaries one ulp tight -- and A = 1 (every site),
    and test sites: 0 the off-site position over the whole chromosome (the candidate); 1 the same position and window (a
    conditioning locus whose reach at grid A number k holds exactly COUNTS[k] sites); 2 the same position in a window that cuts
    its reach inside the first tile; 3 the position of a SITE near 1.0 (that site is never shared); 4 the triple's position; 5 a
    position out of reach of every site at every A but the last."""
    z = zcut()
    h = 5e-5
    j = np.arange(350, dtype=np.float64)
    left, right = 1.0 - (2 * j + 1) * h, 1.0 + (2 * j + 2) * h
    tY = float(right[300])
    gen = np.sort(np.concatenate([left, right, [tY, tY]]))
    tX = 1.0
    d = np.sort(np.abs(gen - tX))
    As = [ic._A_for_count(d, K, z) for K in COUNTS] + [1.0]
    N = len(gen)
    rng = np.random.default_rng(seed)
    n = 20
    k = rng.integers(1, n + 1, N)
    near = int(np.searchsorted(gen, tX)) + 3                   # a site a few places right of 1.0
    tg = np.array([tX, tX, tX, float(gen[near]), tY, 5.0])
    lo = np.array([0, 0, 300, 0, 0, 0], dtype=np.int64)
    hi = np.array([N - 1, N - 1, 420, N - 1, N - 1, N - 1], dtype=np.int64)
    order = np.argsort(tg, kind='stable')                       # test positions ascend, as the scan wants them
    assert order.tolist() == [0, 1, 2, 3, 4, 5]
    return ic._synthetic('cond_edges', eng, (n,), k, np.full(N, n), gen, As, tg, lo, hi, [0, 1, 2, 3, 4, 5])


def catalogue(eng):
    return {'ex1_B2': lambda: example('ex1_B2'),
            'ex1_B2_fixX_fixAlpha_listA': lambda: example('ex1_B2_fixX_fixAlpha_listA'),
            'ex1_B2_w50_s25': lambda: example('ex1_B2_w50_s25'),
            'ragged': lambda: ic.ragged(eng)}


def neighbours(cat):
    """The pairs of the comparison with real conditioning loci: every listed window given a test site a few rows to its right, then
    one to its left, then itself (the conditioning grid point is chosen by the test: the conditioning site's own argmax)."""
    M = len(cat.tg)
    out = []
    for pick in (lambda w, k: w + 2 + k, lambda w, k: w - 5 - k, lambda w, k: w):
        for k, w in enumerate(cat.windows):
            if 0 <= pick(w, k) < M:
                out.append((w, pick(w, k)))
    return out


def unreachable(cat):
    """(c, lin_c) of a conditioning locus that shares no site with ANY window: the first test site, held at the largest A of the
    grid, with no site of its clipped window in reach (A_c |g_i - tc| <= zcut and g_i != tc); None if there is none."""
    iA = int(np.argmax(cat.As))
    N = len(cat.gen)
    for c in range(len(cat.tg)):
        a, b = max(int(cat.lo[c]), 0), min(int(cat.hi[c]), N - 1)
        g = cat.gen[a:b + 1] if b >= a else np.zeros(0)
        if not np.any((cat.As[iA] * np.abs(g - cat.tg[c]) <= zcut()) & (g != cat.tg[c])):
            return c, iA * len(cat.xs) * len(cat.ab)
    return None


# ---------------------------------------------------------------------------------------------- the planted demonstration
DEMO_N, DEMO_SEED = 3000, 5
DEMO_GRID = ([0.35, 0.5], [5.0], [300.0, 1000.0, 3000.0])       # xs, alpha_betas, As: a --fixAlpha / --listA style grid
DEMO_POINT = (1, 0, 0)                                           # (iA, ix, ia): A = 1000, x = 0.35, alpha_beta = 5
DEMO_STEP = 5                                                    # every 5th site is a test site
DEMO_SEP = 0.0005                                                # --peaks G
DEMO_MIN = 5.0                                                   # --peakMin
DEMO_CENTRES = (1100, 1500)                                      # sites: (b) plants both, (a) the second alone
DEMO_KEYS = (power.replicate_key(11, 0, 0), power.replicate_key(11, 1, 0))


@functools.lru_cache(maxsize=None)
def demo_base():
    return pc.Planted('B2', 1, (20, 24), DEMO_N, DEMO_SEED, DEMO_GRID[0], DEMO_GRID[1], DEMO_GRID[2], DEMO_POINT)


def demo_rows(base, centres):
    """The base chromosome's rows with one locus planted after the other at the given sites (a site in reach of two loci keeps the
    later draw)."""
    rows = base.rows
    for c, key in zip(centres, DEMO_KEYS[-len(centres):]):
        rows, _ = power.planted_rows(base.gen, rows, base.model.sizes, base.model.row_off, base.R[DEMO_POINT[1], DEMO_POINT[2]], base.gw,
                                     base.A, [float(base.gen[c])], key, zcut())
    return rows


def demo(centres):
    """The host's whole chain on one planted chromosome: the plain-sum scan of every DEMO_STEP-th site, the peak call, the parents
    and the conditional maxima.  Returns a list of dicts per apex: row (track row), site, clr, parent (place in the list, -1),
    tmax, clr_cond, retained (None without a parent)."""
    base = demo_base()
    rows = demo_rows(base, centres)
    z = zcut()
    sites = np.arange(0, DEMO_N, DEMO_STEP)
    tg = base.gen[sites]
    N = DEMO_N
    surf = [surfaces.host_surface(base.gen, rows, base.R, base.As, t, 0, N - 1, z)[0] for t in tg.tolist()]
    best = [influence.scan_argmax(T)[:2] for T in surf]
    clr = np.array([b[0] for b in best])
    lin = np.array([b[1] for b in best])
    npairs = len(base.xs) * len(base.abetas)
    iA = np.where(lin >= 0, lin // npairs, -1)
    apex = peaks.call(tg, clr, DEMO_SEP, DEMO_MIN)['row'].astype(np.int64)
    par = conditional.parents(tg, clr, iA, np.array(base.As), apex, z)
    out = []
    for k, j in enumerate(apex.tolist()):
        e = {'row': j, 'site': int(sites[j]), 'clr': float(clr[j]), 'parent': int(par[k]), 'tmax': float(clr[j]), 'clr_cond': None,
             'retained': None}
        if par[k] >= 0:
            q = int(apex[par[k]])
            a, ix, ia = decode(int(lin[q]), len(base.xs), len(base.abetas))
            T = conditional.host_cond_surface(base.gen, rows, base.R, base.As, tg[j], 0, N - 1, tg[q], 0, N - 1, base.As[a], ix, ia, z)[0]
            e['clr_cond'] = influence.scan_argmax(T)[0]
            e['retained'] = e['clr_cond'] / e['tmax']
        out.append(e)
    return out
