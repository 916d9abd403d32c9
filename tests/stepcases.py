"""The cases of the --stepwise tests: condcases.py's and influencecases.py's chromosomes with a list of apexes each, the literal
per-site statement of the K-locus nested mixture, the margins that make the device comparison decisive, and the planted
demonstration.  test_stepwise_cpu.py checks the host restatement (ballermixplus_amd/stepwise.py) against them; test_gpu_stepwise.py
runs the same chromosomes on the device."""
import functools
import math
import os

import numpy as np

import condcases as cc
import influencecases as ic

from ballermixplus_amd import influence, peaks, stepwise, surfaces

SITE_TOL = cc.SITE_TOL        # the CPU checks: |dT| <= SITE_TOL * (nsites + sum_i |term_i|) per grid point
REL_TOL = cc.REL_TOL          # the GPU comparison: of max over the grid of 2 sum_i |term_i| of the HOST restatement
D_TOL = 1e-12                 # the GPU comparison of d: of the per-site sum of absolute increments
ID_TOL = 1e-12                # the identity: of the sum of absolute terms
MARGIN = 1e-6                 # every choice of the greedy run is decided by at least this, relative
NAMES = ('small', 'edges', 'ragged', 'ex1_B2', 'ex1_B2_fixX_fixAlpha_listA', 'ex1_B2_w50_s25', 'demo1', 'demo2')
FAST = tuple(n for n in NAMES if n != 'ex1_B2')       # a surface of ex1_B2 (31 A x 510 pairs x 756 sites) takes the host a second
DEMO_C = 15.0
RAGGED_SEED = 79              # influencecases.ragged's recipe under a seed whose host run clears MARGIN (77, its default: an argmax
#                               decided by 1e-7; 78 .. 81 all pass, 79 by the most)


def zcut():
    return cc.zcut()


class Case:
    """One chromosome with its apexes: gen[N], rows[N], the grids in scan order, test sites (tg, lo, hi), apex: the test sites of
    the apexes in row order, C: the threshold; R() the host's table, context(engine) a context holding the case on the device."""

    def __init__(self, name, gen, rows, xs, ab, As, tg, lo, hi, apex, C, host_R, context):
        self.name, self.gen, self.rows = name, np.asarray(gen, dtype=np.float64), np.asarray(rows, dtype=np.int32)
        self.xs, self.ab, self.As = list(xs), list(ab), [float(a) for a in As]
        self.tg, self.lo, self.hi = np.asarray(tg, dtype=np.float64), np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
        self.apex = np.array(sorted(set(int(a) for a in apex)), dtype=np.int64)
        self.C = float(C)
        self._host_R, self._R, self.context = host_R, None, context
        self.npairs = len(self.xs) * len(self.ab)

    def R(self):
        if self._R is None:
            self._R = self._host_R()
        return self._R

    def ranges(self):
        a = self.apex
        return stepwise.site_ranges(self.gen, self.tg[a], self.lo[a], self.hi[a], min(self.As), zcut())

    def host_run(self, R=None, zc=None, **kw):
        a = self.apex
        return stepwise.host_run(self.gen, self.rows, self.R() if R is None else R, self.As, self.tg[a], self.lo[a], self.hi[a],
                                 zcut() if zc is None else zc, kw.pop('min_clr', self.C), **kw)


def _from_cat(cat, apex, C=0.0):
    return Case(cat.name, cat.gen, cat.rows, cat.xs, cat.ab, cat.As, cat.tg, cat.lo, cat.hi, apex, C, cat.R, cat.context)


def _from_planted(name, c, rows, tg, lo, hi, apex, C):
    def context(eng):
        ctx = eng.Context(0)
        ctx.set_model(c.model, c.As)
        ctx.set_sites(c.gen, rows)
        ctx.set_tests(tg, lo, hi)
        return ctx
    return Case(name, c.gen, rows, c.xs, c.abetas, c.As, tg, lo, hi, apex, C, lambda: c.R, context)


@functools.lru_cache(maxsize=None)
def demo_track(n_loci):
    """The planted demonstration's chromosome with one locus (site 1500) or two (sites 1100 and 1500): the plain-sum scan of every
    DEMO_STEP-th site on the host and its peak call at --peaks DEMO_SEP --peakMin DEMO_MIN.  Returns (rows, tg, clr, apex rows)."""
    base = cc.demo_base()
    rows = cc.demo_rows(base, cc.DEMO_CENTRES[-n_loci:])
    tg = base.gen[np.arange(0, cc.DEMO_N, cc.DEMO_STEP)]
    best = [influence.scan_argmax(surfaces.host_surface(base.gen, rows, base.R, base.As, t, 0, cc.DEMO_N - 1, zcut())[0])[0] for t in tg.tolist()]
    clr = np.array(best)
    return rows, tg, clr, peaks.call(tg, clr, cc.DEMO_SEP, cc.DEMO_MIN)['row'].astype(np.int64)


DEMO_CLI = ['--fixAlpha', '5', '--listA', '300,1000,3000', '-s', str(cc.DEMO_STEP), '--peaks', repr(cc.DEMO_SEP), '--peakMin', repr(cc.DEMO_MIN)]


def demo_files(d, n_loci=2, name='planted'):
    """The planted chromosome as files for the CLI in directory d: the input <name>.txt in the reference's four columns and the
    spectrum getSpect tabulates from it.  Returns ['-i', input, '--spect', spectrum]."""
    from ballermixplus_amd import helpers, synth
    base = cc.demo_base()
    rows = np.asarray(demo_track(n_loci)[0], dtype=np.int64)
    off = np.asarray(base.model.row_off, dtype=np.int64)
    j = np.searchsorted(off, rows, side='right') - 1
    k, nn = rows - off[j], np.asarray(base.model.sizes, dtype=np.int64)[j]
    inp, sp = os.path.join(str(d), name + '.txt'), os.path.join(str(d), name + '_spect.txt')
    synth.write_input(inp, np.rint(base.gen * 1e6).astype(np.int64), base.gen, k, nn)
    helpers.getSpect(inp, sp, False, False)
    return ['-i', inp, '--spect', sp]


def case(name, eng=None):
    """The case of that name.  eng: ballermixplus_amd.engine (the synthetic chromosomes build their model arrays with it; no
    device is touched before context())."""
    if eng is None:
        from ballermixplus_amd import engine as eng
    if name == 'small':
        c = cc.small()
        return _from_planted(name, c, c.rows, c.tg, c.lo, c.hi, range(5), 0.0)
    if name == 'edges':                 # (test sites 0 and 1 are the same window: one of them)
        return _from_cat(cc.edges(eng), [0, 2, 3, 4, 5])
    if name == 'ragged' or name.startswith('ex1'):
        cat = ic.ragged(eng, seed=RAGGED_SEED) if name == 'ragged' else cc.example(name)
        return _from_cat(cat, cat.windows)
    if name in ('demo1', 'demo2'):
        rows, tg, clr, apex = demo_track(int(name[-1]))
        N = cc.DEMO_N
        return _from_planted(name, cc.demo_base(), rows, tg, np.zeros(len(tg), dtype=np.int64), np.full(len(tg), N - 1, dtype=np.int64), apex, DEMO_C)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def host_case(name):
    """(the case, its host run with the margins of every choice) on the host's own table, computed once."""
    c = case(name)
    m = Margins(c.C)
    return c, c.host_run(watch=m.watch), m


class Margins:
    """A watch of stepwise.run(): the relative gaps that decide the run.  step: between the best and the second cur_T among the
    apexes not yet accepted, at every choice; argmax: between every surface's maximum and its runner-up grid point; stop: between
    the best cur_T and the threshold, at every choice and at the end."""

    def __init__(self, C):
        self.C, self.step, self.argmax, self.stop = float(C), [], [], []

    def watch(self, step, places, res, cur_T, accepted):
        if res is not None:
            for T in res['T']:
                v, l, second = influence.scan_argmax(T)
                if l >= 0:
                    self.argmax.append((v - second) / v)
        left = np.sort(cur_T[~accepted])[::-1]
        if len(left) and left[0] > 0:
            if len(left) > 1 and left[0] >= self.C:
                self.step.append((left[0] - left[1]) / left[0])
            if self.C > 0:
                self.stop.append(abs(left[0] - self.C) / max(left[0], self.C))

    def worst(self):
        return tuple(min(v) if v else float('inf') for v in (self.step, self.argmax, self.stop))


# ------------------------------------------------------------------------------------------------------ the literal loop

def literal_base(genpos, rows, g_row, R, A, tg, lo, hi, loci, zc):
    """The definition as a per-site Python loop in PROBABILITY space.  loci: (tc, clo, chi, A_c, ix_c, ia_c) in order of entry.
    Every site keeps an explicit list of mixture components (weight, density), [(1, g)] under neutrality; a locus that reaches the
    site with linkage a scales every weight by (1 - a) and appends (a, g (1 + R_c)).  With den = sum w f the candidate's term is
        log((1 - a) den + a f) - log(den),     f = g (1 + R).
    Returns (T[nA][nx][nab], nsites[nA], nshared[nA], S[nA][nx][nab] = sum |term|, d[N] = den / g - 1, cnt[N], weights: the
    largest |sum of a site's weights - 1|)."""
    N = len(genpos)
    comp = [[(1.0, float(g_row[int(rows[i])]))] for i in range(N)]
    cnt = np.zeros(N, dtype=np.int32)
    for tc, clo, chi, A_c, ix_c, ia_c in loci:
        for i in range(max(int(clo), 0), min(int(chi), N - 1) + 1):
            gi = float(genpos[i])
            z = float(A_c) * abs(gi - float(tc))
            if not z <= zc or gi == float(tc):
                continue
            a = math.exp(-z)
            g = float(g_row[int(rows[i])])
            comp[i] = [(w * (1.0 - a), f) for w, f in comp[i]] + [(a, g * (1.0 + float(R[ix_c][ia_c][int(rows[i])])))]
            cnt[i] += 1
    den = np.array([sum(w * f for w, f in c) for c in comp])
    weights = max(abs(sum(w for w, _ in c) - 1.0) for c in comp)
    d = den / np.array([float(g_row[int(r)]) for r in rows]) - 1.0
    nx, nab = np.asarray(R).shape[:2]
    nA = len(A)
    T, S = np.full((nA, nx, nab), np.nan), np.zeros((nA, nx, nab))
    ns, nsh = np.zeros(nA, dtype=np.int32), np.zeros(nA, dtype=np.int32)
    for iA in range(nA):
        acc = [[0.0] * nab for _ in range(nx)]
        acc_abs = [[0.0] * nab for _ in range(nx)]
        for i in range(max(int(lo), 0), min(int(hi), N - 1) + 1):
            gi = float(genpos[i])
            z = float(A[iA]) * abs(gi - float(tg))
            if not z <= zc or gi == float(tg):
                continue
            ns[iA] += 1
            nsh[iA] += 1 if cnt[i] > 0 else 0
            r = int(rows[i])
            g, a = float(g_row[r]), math.exp(-z)
            for ix in range(nx):
                for ia in range(nab):
                    term = math.log((1.0 - a) * den[i] + a * g * (1.0 + float(R[ix][ia][r]))) - math.log(den[i])
                    acc[ix][ia] += term
                    acc_abs[ix][ia] += abs(term)
        if ns[iA]:
            T[iA], S[iA] = 2.0 * np.array(acc), np.array(acc_abs)
    return T, ns, nsh, S, d, cnt, weights


def host_baseline(c, loci, R=None, zc=None):
    """(d, cnt, scale, written) of the case's chromosome after the loci (test site, lin) in order, by stepwise.host_baseline_add."""
    R = c.R() if R is None else R
    zc = zcut() if zc is None else zc
    nx, nab = len(c.xs), len(c.ab)
    d, cnt, scale = np.zeros(len(c.gen)), np.zeros(len(c.gen), dtype=np.int32), np.zeros(len(c.gen))
    written = []
    for t, lin in loci:
        iA, ix, ia = cc.decode(int(lin), nx, nab)
        written.append(stepwise.host_baseline_add(d, cnt, c.gen, c.rows, R, c.tg[t], c.lo[t], c.hi[t], c.As[iA], ix, ia, zc, scale=scale))
    return d, cnt, scale, written
