"""The fixed cases of the planted-signal power analysis (ballermixplus_amd/power.py): the input of tests/test_power_cpu.py and
tests/test_gpu_power.py.  numpy, the package's pure-Python modules and the oracle; no library call.

sampler(stat)   6 000 sites of sample sizes 20 and 24 drawn from a complete analytic spectrum (1/k polymorphisms, half the mass on
                substitutions where the statistic has them), a run of 21 tied positions, a 3 x 3 x 4 grid, the planted point
                (A = 1000, x = 0.35, alpha_beta = 5) and three centres: the first site (its run of sites is clipped by the end of
                the array), a position inside the tie (its own sites are not redrawn) and an ordinary site.
large()         4 000 sites of the 221 sample sizes 300 .. 520: 90 831 table rows (4-byte rows, past the sampler's LDS staging
                cap of 3 072 rows and the histogram's 8 192), a 2 x 2 pair grid, one centre.
e2e             a neutral synth chromosome (3 000 sites, n = 100, chromosome 41), --findBal --listA 1000,3000,10000, the planted
                point (A = 1000, x = 0.5, alpha_beta = 100), thresholds 100 and 135, seed 1; the separation test takes 8
                replicates of it, the end-to-end test the first 4.
"""
import functools

import numpy as np

from util import Grids, c_oracle, c_scan, oracle_R, orc

from ballermixplus_amd import power, synth

SAMPLER_STATS = ('B2', 'B2maf', 'B1')
SAMPLER_KEY = power.replicate_key(7, 0, 0)
LARGE_KEY = power.replicate_key(7, 1, 0)


def analytic_spectrum(stat, sizes, min_count):
    """(spect {(k, n): g}, props {n: share}) with g > 0 on EVERY admissible count of the statistic and 0 mass elsewhere: equal
    shares per sample size; within a size half the mass on the substitutions (where the statistic has them) and the rest ~ 1/k on
    the polymorphic counts (folded for the MAF statistics)."""
    spect, props = {}, {}
    for n in sizes:
        p = 1.0 / len(sizes)
        props[n] = p
        if stat == 'B1':
            w = {0: 0.5, 1: 0.5}
        else:
            excl = set(orc.excluded_counts(stat, n, min_count).tolist())
            ks = [k for k in range(1, n) if k not in excl]
            if stat in ('B2maf', 'B0maf'):
                ks = [k for k in ks if k <= n // 2]
                pw = np.array([(1.0 / k + 1.0 / (n - k)) * (0.5 if 2 * k == n else 1.0) for k in ks])
            else:
                pw = np.array([1.0 / k for k in ks])
            sub = 0.5 if stat in ('B2', 'B2maf') else 0.0
            w = {k: (1.0 - sub) * v for k, v in zip(ks, (pw / pw.sum()).tolist())}
            if sub:
                w[n] = sub
        for k, v in w.items():
            spect[(k, n)] = p * v
    return spect, props


class Planted:
    """One case: model arrays, site arrays, the planted point and its centres; R (the oracle's table) on demand."""

    def __init__(self, stat, min_count, sizes, N, seed, xs, abetas, As, planted, tie=None):
        from ballermixplus_amd import engine
        rng = np.random.default_rng(seed)
        gaps = rng.geometric(0.02, N)
        if tie is not None:
            gaps[tie[0]:tie[1]] = 0
        self.gen = np.cumsum(gaps) / 1e6
        self.stat, self.min_count, self.sizes = stat, min_count, tuple(sizes)
        self.spect, self.props = analytic_spectrum(stat, sizes, min_count)
        nn = rng.choice(np.array(sizes), N)
        k = np.zeros(N, dtype=np.int64)
        for n in sizes:
            ks = sorted(a for (a, b) in self.spect if b == n)
            p = np.array([self.spect[(a, n)] for a in ks]) / self.props[n]
            at = np.nonzero(nn == n)[0]
            k[at] = rng.choice(np.array(ks), len(at), p=p / p.sum())
        self.xs, self.abetas, self.As = list(xs), list(abetas), list(As)
        self.model = engine.ModelArrays(stat, min_count, sizes, self.spect, self.props, self.xs, self.abetas)
        self.rows = self.model.rows_of(k, nn)
        self.planted = planted                       # (iA, ix, ia)
        self.A = float(self.As[planted[0]])
        self.gw = power.allowed_rows(stat, min_count, self.model.sizes, self.model.row_off, self.model.g)

    @functools.cached_property
    def R(self):
        return oracle_R(self.stat, self.sizes, self.min_count, self.spect, self.props, self.xs, self.abetas)

    def host(self, key, R=None, rows=None):
        """power.planted_rows of the case under key (R: another table than the oracle's, e.g. the device's)."""
        R = self.R if R is None else R
        return power.planted_rows(self.gen, self.rows if rows is None else rows, self.model.sizes, self.model.row_off,
                                  R[self.planted[1], self.planted[2]], self.gw, self.A, self.centres, key)

    def runs(self):
        """(first, count) of every centre, as bmx_ctx_plant_sites reports them."""
        fc = [power.reach(self.gen, c, self.A)[1:] for c in self.centres]
        return np.array([a for a, _ in fc], dtype=np.int32), np.array([b for _, b in fc], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def sampler(stat):
    c = Planted(stat, 0 if stat == 'B1' else 1, (20, 24), 6000, 11, [0.2, 0.35, 0.5], [0.5, 5.0, 50.0], [200.0, 1000.0, 5000.0, 30000.0],
                (1, 1, 1), tie=(2500, 2520))
    assert np.all(c.gen[2499:2520] == c.gen[2510]) and c.gen[2498] < c.gen[2499] and c.gen[2520] > c.gen[2519]
    c.centres = np.array([c.gen[0], c.gen[2510], c.gen[4500]])
    return c


@functools.lru_cache(maxsize=None)
def large():
    c = Planted('B2', 1, tuple(range(300, 521)), 4000, 21, [0.3, 0.5], [2.0, 20.0], [500.0, 2000.0], (1, 1, 0))
    assert c.model.rows > 65535 and c.model.rows * 16 > 48 << 10 and c.model.rows > 8192
    c.centres = np.array([c.gen[2000]])
    return c


# ------------------------------------------------------------------------------------------------ separation and end to end

E2E_N, E2E_n, E2E_CHROM = 3000, 100, 41
E2E_GRID = ['--findBal', '--listA', '1000,3000,10000']
E2E_PLANT = '1000,0.5,100'
E2E_THRESHOLDS = [100.0, 135.0]
E2E_SEED, E2E_R, SEP_R = 1, 4, 8


class E2E:
    """The end-to-end chromosome with the oracle's model: every site a test position, the default window mode."""

    def __init__(self):
        self.phys, self.gen, self.k, self.nn = synth.synth_chromosome(E2E_N, E2E_n, E2E_CHROM)
        self.spect = {(a, b): f for a, b, f in synth.spect_from_counts(self.k, self.nn)}
        self.props = {E2E_n: 1.0}
        self.xs, self.abetas, self.As = Grids(None, None, True, False, None, '1000,3000,10000').scan_order()
        self.min_count = int(self.k.min())
        self.m = orc.Model('B2', self.gen, self.k, self.nn, self.spect, self.props, self.min_count, self.xs, self.abetas, self.As)
        self.planted = power.parse_plant(E2E_PLANT, self.As, self.xs, self.abetas)
        self.A = float(self.As[self.planted[0]])
        self.sizes, self.row_off = np.array([E2E_n], dtype=np.int32), np.array([0, E2E_n + 1], dtype=np.int32)
        self.gw = power.allowed_rows('B2', self.min_count, self.sizes, self.row_off, self.m.g_row)
        self.rows_c, self.union, self.lo, self.hi, self.H, self.bound, self.D = power.plan_file(self.gen, self.A, float(min(self.As)))
        self.centre_pos = self.gen[self.rows_c]
        self.L = c_oracle()

    def scan(self, gen, rows, test_gen):
        """power.host_power's callable on the C oracle: (clr, lin, nsites)."""
        clr, ix, ia, iA, ns = c_scan(self.L, self.m.R, self.As, gen, rows, test_gen, np.zeros(len(test_gen), np.int64),
                                     np.full(len(test_gen), len(gen) - 1, np.int64))
        lin = np.where(iA >= 0, (iA.astype(np.int64) * len(self.xs) + ix) * len(self.abetas) + ia, -1).astype(np.int32)
        return clr, lin, ns

    def host(self, R, plant=True):
        """(arg, clr, lin, nsites) [R, K] of the first R replicates on the host."""
        return power.host_power(self.scan, self.gen, self.m.row, self.sizes, self.row_off,
                                self.m.R[self.planted[1], self.planted[2]], self.gw, self.A, self.centre_pos,
                                self.gen[self.union], self.lo, self.hi, E2E_SEED, R, 0, 'perm', 1, plant)

    def margins(self, R):
        """The margins of every redrawn site of the first R replicates."""
        from ballermixplus_amd import null
        out = []
        for r in range(R):
            bg = self.m.row[null.block_permutation(len(self.gen), power.background_key(E2E_SEED, r, 0), 1)]
            out.append(power.planted_rows(self.gen, bg, self.sizes, self.row_off, self.m.R[self.planted[1], self.planted[2]], self.gw,
                                          self.A, self.centre_pos, power.replicate_key(E2E_SEED, r, 0))[1])
        return np.array(out)


@functools.lru_cache(maxsize=None)
def e2e():
    return E2E()


@functools.lru_cache(maxsize=None)
def e2e_host(plant=True):
    """The 8 replicates of the separation test (the end-to-end test reads the first 4), computed once."""
    return e2e().host(SEP_R, plant)
