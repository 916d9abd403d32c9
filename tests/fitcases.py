"""The cases of the --fit tests: chromosomes, models, per-row arrays, bins and listed (window, grid point) entries, built on the
host alone.  test_fit_cpu.py asks of every case that the float64 restatement stays within a tenth of the GPU tolerance of its own
long-double evaluation; test_gpu_fit.py runs the same cases on the device.  The chromosomes of `ragged` and `edges` are
influencecases.py's."""
import os
import re

import numpy as np

import cases
import influencecases as ic
from util import REPO, oracle_R, orc

from ballermixplus_amd import fit, power

TOL = 1e-12                 # the GPU comparison: |E_device - E_host| <= TOL * max(1, n_d) per cell, n_d the bin's sites
NAMES = ('ex1_B2', 'ex1_B2maf', 'ex1_B1', 'ragged', 'edges', 'lattice', 'many_sizes', 'excluded')


def header_constant(name):
    """An integer #define of include/bmxscan.h (written as a literal or as `(a << b)`)."""
    with open(os.path.join(REPO, 'include', 'bmxscan.h')) as f:
        m = re.search(r'#define\s+%s\s+\(?\s*(\d+)\s*(?:<<\s*(\d+))?\s*\)?' % name, f.read())
    return int(m.group(1)) << int(m.group(2) or 0)


class FitCase:
    """One case: cat = influencecases.Cat (chromosome, grids, test sites, context()), the model's (stat, min_count, sizes,
    row_off, g), F and edges, and entries = [(window, lin)]: the listed windows with their grid points."""

    def __init__(self, cat, stat, min_count, sizes, g, F, edges, entries, host_R=None, no_gw=()):
        self.name, self.cat, self.stat, self.min_count = cat.name, cat, stat, int(min_count)
        self.sizes = np.asarray(sorted(int(n) for n in sizes), dtype=np.int32)
        per = [2 if stat == 'B1' else int(n) + 1 for n in self.sizes]
        self.row_off = np.concatenate(([0], np.cumsum(per))).astype(np.int32)
        self.g = np.asarray(g, dtype=np.float64)
        assert len(self.g) == self.row_off[-1]
        self.F, self.edges = int(F), np.asarray(edges, dtype=np.float64)
        self.D = len(self.edges) + 1
        self.entries = [(int(w), int(l)) for w, l in entries]
        self.gw = power.allowed_rows(stat, self.min_count, self.sizes, self.row_off, self.g)
        for n in no_gw:                                 # the caller's gw admits no row of these sample sizes
            j = self.sizes.tolist().index(n)
            self.gw[self.row_off[j]:self.row_off[j + 1]] = 0.0
        self.cls = fit.classes(stat, self.sizes, self.row_off, self.F)
        self._host_R = host_R
        self.nx, self.nab = len(cat.xs), len(cat.ab)

    def R(self):
        """A selection table on the host: the oracle's, or the case's stand-in where the oracle would take minutes."""
        return self._host_R() if self._host_R is not None else self.cat.R()

    def tests(self):
        return np.array([w for w, _ in self.entries], dtype=np.int32)

    def lins(self):
        return np.array([l for _, l in self.entries], dtype=np.int32)

    def host(self, q, R, zcut=None, dtype=np.float64):
        """host_fit of entry q on the table R ((O all 0, E NaN, 0) for lin < 0, as the device answers)."""
        w, lin = self.entries[q]
        if lin < 0:
            nan = np.full((self.D, self.F), np.nan)
            return np.zeros((self.D, self.F), dtype=np.int32), nan, nan.copy(), 0
        iA, ix, ia = lin // (self.nx * self.nab), (lin // self.nab) % self.nx, lin % self.nab
        c = self.cat
        return fit.host_fit(c.gen, c.rows, self.row_off, R, self.gw, self.cls, self.F, self.edges, c.As[iA], ix, ia, c.tg[w], c.lo[w],
                            c.hi[w], orc.alpha_cut_z() if zcut is None else zcut, dtype=dtype)


def spread(cat, windows, per_window):
    """Entries: every listed window at per_window grid points spread over the grid by a fixed rule."""
    points = len(cat.As) * len(cat.xs) * len(cat.ab)
    out = []
    for w in windows:
        for k in range(per_window):
            out.append((w, (len(out) * 7919 + 13 * k + 5) % points))
    return out


def every_A(cat, windows):
    """Entries: every listed window at every A of the grid, the (x, alpha_beta) pair moving along."""
    npairs = len(cat.xs) * len(cat.ab)
    return [(w, iA * npairs + (5 * w + 11 * iA) % npairs) for w in windows for iA in range(len(cat.As))]


def _g_from_rows(rows, n_rows):
    """The neutral spectrum influencecases._synthetic gives its model: the share of the sites on every row, NaN where none is."""
    cnt = np.bincount(np.asarray(rows), minlength=n_rows).astype(np.float64)
    return np.where(cnt > 0, cnt / len(rows), np.nan)


def example(name, eng, windows, F, D, per_window=3):
    cat = ic._example(name, windows)
    opt, case, _ = cases.host_side(list(cases.ALL_CASES[name][0]))
    model = eng.ModelArrays(case.stat, case.data.minCount, case.data.sampSizes, case.neut.spect, case.neut.sampProps, case.xs, case.abetas)
    assert np.array_equal(model.rows_of(case.data.count, case.data.total), cat.rows)
    return FitCase(cat, case.stat, case.data.minCount, model.sizes, model.g, F, fit.default_edges(D, orc.alpha_cut_z()),
                   spread(cat, cat.windows, per_window))


def ragged(eng):
    cat = ic.ragged(eng)
    sizes = (12, 33, 50)
    g = _g_from_rows(cat.rows, sum(n + 1 for n in sizes))
    return FitCase(cat, 'B2', 1, sizes, g, 7, [0.3, 1.0, 2.5, 6.0, 12.0], spread(cat, cat.windows, 3) + [(cat.windows[0], -1)])


def edges(eng):
    """Qualifying counts of 0, 1, 255, 256, 257, 512 and 513 around the tile size of 256: 5 windows x 8 A = 40 entries."""
    cat = ic.edges(eng)
    return FitCase(cat, 'B2', 1, (20,), _g_from_rows(cat.rows, 21), 10, fit.default_edges(8, orc.alpha_cut_z()), every_A(cat, cat.windows))


def _synth(name, eng, stat, min_count, sizes, k, nn, gen, As, xs, ab, tg, lo, hi, windows, spect=None):
    """influencecases._synthetic with the statistic, the min count and the (x, alpha_beta) grids left to the caller."""
    N = len(gen)
    if spect is None:
        cnt = {}
        for a, b in zip(np.asarray(k).tolist(), np.asarray(nn).tolist()):
            cnt[(a, b)] = cnt.get((a, b), 0) + 1
        spect = {key: v / N for key, v in cnt.items()}
    props = {int(n): sum(v for (a, b), v in spect.items() if b == n) for n in sizes}
    model = eng.ModelArrays(stat, min_count, sizes, spect, props, xs, ab)
    rows = model.rows_of(k, nn)

    def context(e):
        ctx = e.Context(0)
        ctx.set_model(model, As)
        ctx.set_sites(gen, rows)
        ctx.set_tests(tg, lo, hi)
        return ctx

    def host_R():
        with np.errstate(divide='ignore', invalid='ignore'):
            return oracle_R(stat, sizes, min_count, spect, props, xs, ab)

    cat = ic.Cat(name, gen, rows, xs, ab, As, tg, lo, hi, windows, host_R, context)
    return cat, model


LATTICE_A = 16.0
LATTICE_EDGES = [0.5, 2.0, 3.3, 8.0, 16.0]


def lattice_positions():
    """Positions around the test position 0 whose z = 16 * |g| is exact (a power-of-two A): the lattice j / 64 on either side,
    and for every edge e the three distances e / 16, one ulp below and one ulp above it, on both sides.  Returns (gen sorted,
    {edge: (d_below, d_on, d_above)})."""
    j = np.arange(1, 80, dtype=np.float64)
    d = [j / 64.0 + 2.0 ** -20]                  # off the edges' own values
    marks = {}
    for e in LATTICE_EDGES:
        on = e / LATTICE_A
        marks[e] = (float(np.nextafter(on, 0.0)), on, float(np.nextafter(on, np.inf)))
        d.append(np.array(marks[e]))
    d = np.concatenate(d)
    return np.sort(np.concatenate([-d, d])), marks


def lattice(eng, seed=11):
    gen, _ = lattice_positions()
    rng = np.random.default_rng(seed)
    n = 16
    k = rng.integers(1, n + 1, len(gen))
    N = len(gen)
    tg = np.array([0.0, 0.0])
    lo, hi = np.array([0, N // 2 - 40], dtype=np.int64), np.array([N - 1, N // 2 + 60], dtype=np.int64)
    cat, model = _synth('lattice', eng, 'B2', 1, (n,), k, np.full(N, n), gen, [LATTICE_A, 1024.0], [0.2, 0.5], [1.0, 50.0], tg, lo, hi, [0, 1])
    return FitCase(cat, 'B2', 1, (n,), model.g, 4, LATTICE_EDGES, every_A(cat, [0, 1]))


def many_sizes(eng, seed=5):
    """More sample sizes than the device's LDS budget for the prologue sums holds: n_sizes * F * 16 > BMX_FIT_LDS_BYTES.  The
    host table of this case is a stand-in (uniform in [-0.9, 3), NaN where g is): the oracle's would take minutes, and the GPU
    test reads the device's own table."""
    F = 10
    S = header_constant('BMX_FIT_LDS_BYTES') // (F * 16) + 4
    sizes = tuple(range(5, 5 + S))
    assert len(sizes) * F * 16 > header_constant('BMX_FIT_LDS_BYTES')
    rng = np.random.default_rng(seed)
    N = 2000
    gen = np.sort(rng.uniform(0.0, 1.0, N))
    nn = rng.choice(np.array(sizes), N)
    k = np.array([rng.integers(1, h + 1) for h in nn])
    As = [30.0, 400.0]
    tg = np.array([0.25, float(gen[1000]), 0.9])
    lo, hi = np.zeros(3, dtype=np.int64), np.full(3, N - 1, dtype=np.int64)
    cat, model = _synth('many_sizes', eng, 'B2', 1, sizes, k, nn, gen, As, [0.2, 0.5], [1.0, 50.0], tg, lo, hi, [0, 1, 2])

    def stand_in():
        r = np.random.default_rng(seed + 1).uniform(-0.9, 3.0, (2, 2, model.rows))
        r[:, :, np.isnan(model.g)] = np.nan
        return r

    return FitCase(cat, 'B2', 1, sizes, model.g, F, fit.default_edges(8, orc.alpha_cut_z()), every_A(cat, [0, 1, 2]), stand_in)


def excluded(eng, seed=9):
    """B_2 with min count 2 on sample sizes 7 and 20.  A site with k = 1 stands on a row with gw = 0 (an excluded count): it is
    counted in O and its row enters no E; the rows no site stands on have gw = 0 and a NaN R (g is NaN there).  The gw of this
    case admits no row of size 7 at all, so the sites of that size have a neutral total of 0 and are skipped."""
    rng = np.random.default_rng(seed)
    N = 600
    gen = np.sort(np.round(rng.uniform(0.0, 1.0, N), 3))
    nn = np.where(rng.random(N) < 0.1, 7, 20)
    k = np.where(nn == 7, rng.integers(1, 8, N), rng.integers(1, 21, N))
    As = [25.0, 300.0]
    tg = np.array([0.5, float(gen[200])])
    lo, hi = np.zeros(2, dtype=np.int64), np.full(2, N - 1, dtype=np.int64)
    cat, model = _synth('excluded', eng, 'B2', 2, (7, 20), k, nn, gen, As, [0.2, 0.5], [1.0, 50.0], tg, lo, hi, [0, 1])
    return FitCase(cat, 'B2', 2, (7, 20), model.g, 5, [1.0, 4.0, 9.0], every_A(cat, [0, 1]), no_gw=(7,))


def catalogue(eng):
    """Every case of the GPU comparison, by name."""
    return {'ex1_B2': lambda: example('ex1_B2', eng, [0, 400, -1], 10, 8),
            'ex1_B2maf': lambda: example('ex1_B2maf', eng, [5, 380], 10, 8),
            'ex1_B1': lambda: example('ex1_B1', eng, [5, 380], 2, 6),
            'ragged': lambda: ragged(eng),
            'edges': lambda: edges(eng),
            'lattice': lambda: lattice(eng),
            'many_sizes': lambda: many_sizes(eng),
            'excluded': lambda: excluded(eng)}


def literal_fit(genpos, rows, row_off, R, gw, cls, F, edges, A, ix, ia, tg, lo, hi, zcut):
    """The definition as a per-site, per-row Python loop (the small cases' check of host_fit)."""
    import math
    D = len(edges) + 1
    O = [[0] * F for _ in range(D)]
    Es, En = [[0.0] * F for _ in range(D)], [[0.0] * F for _ in range(D)]
    skipped = 0
    for i in range(max(int(lo), 0), min(int(hi), len(genpos) - 1) + 1):
        g = float(genpos[i])
        z = float(A) * abs(g - float(tg))
        if not z <= zcut or g == float(tg):
            continue
        d = sum(1 for e in edges if z > e)
        r0 = int(rows[i])
        j = max(jj for jj in range(len(row_off) - 1) if row_off[jj] <= r0)
        a, b = int(row_off[j]), int(row_off[j + 1])
        O[d][int(cls[r0])] += 1
        alpha = math.exp(-z)
        m, tot, neu = [], 0.0, 0.0
        for r in range(a, b):
            v = float(gw[r]) * (1.0 + alpha * float(R[ix][ia][r])) if gw[r] > 0 else 0.0
            if not math.isfinite(v):
                v = 0.0
            m.append(v)
            tot += v
            neu += float(gw[r])
        if not (math.isfinite(tot) and tot > 0 and math.isfinite(neu) and neu > 0):
            skipped += 1
            continue
        for r in range(a, b):
            Es[d][int(cls[r])] += m[r - a] / tot
            En[d][int(cls[r])] += float(gw[r]) / neu
    return np.array(O, dtype=np.int32).reshape(D, F), np.array(Es).reshape(D, F), np.array(En).reshape(D, F), skipped


def chi2_quantile(p, df):
    """The p quantile of chi-square(df): scipy's where importable, else the Wilson-Hilferty formula."""
    try:
        from scipy import stats
        return float(stats.chi2.ppf(p, df))
    except ImportError:
        from statistics import NormalDist
        zq = NormalDist().inv_cdf(p)
        return df * (1.0 - 2.0 / (9.0 * df) + zq * (2.0 / (9.0 * df)) ** 0.5) ** 3


# ------------------------------------------------------------------------------------------------------- the planted case
PLANT_SEED, PLANT_F, PLANT_D = 1, 10, 8
PLANT_VALUES = (10000.0, 0.5, 1.0)          # (A, x, alpha_beta): values of ex1_B2's grids


def plant_point(cat):
    """(iA, ix, ia) of PLANT_VALUES in the grids' scan order."""
    return tuple([float(v) for v in grid].index(want) for grid, want in zip((cat.As, cat.xs, cat.ab), PLANT_VALUES))


def planted(eng):
    """ex1_B2's chromosome with every site in reach of one centre redrawn by power.planted_rows at one grid point (fixed seed):
    (FitCase with the planted rows and the one entry (centre window, planted point), the planted lin).  The fitted model must
    then pass its own chi-square and neutrality fail it."""
    base = example('ex1_B2', eng, [0], PLANT_F, PLANT_D, 1)
    cat = base.cat
    R = cat.R()
    iA, ix, ia = plant_point(cat)
    centre_row = len(cat.tg) // 2
    new, _ = power.planted_rows(cat.gen, cat.rows, base.sizes, base.row_off, R[ix, ia], base.gw, cat.As[iA], [float(cat.tg[centre_row])],
                                power.replicate_key(PLANT_SEED, 0), orc.alpha_cut_z())
    lin = (iA * base.nx + ix) * base.nab + ia
    inner = cat.context

    def context(e):
        ctx = inner(e)
        ctx.set_sites(cat.gen, new)
        ctx.set_tests(cat.tg, cat.lo, cat.hi)
        return ctx

    pc = ic.Cat('planted', cat.gen, new, cat.xs, cat.ab, cat.As, cat.tg, cat.lo, cat.hi, [centre_row], cat.R, context)
    return FitCase(pc, base.stat, base.min_count, base.sizes, base.g, PLANT_F, base.edges, [(centre_row, lin)]), lin
