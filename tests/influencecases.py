"""The cases of the --influence tests: chromosomes, models, windows and block sizes, built on the host alone.  test_influence_cpu.py
asks of every case that the host restatement's argmax margins are wide enough for the GPU comparison to be decisive;
test_gpu_influence.py runs the same cases on the device."""
import numpy as np

import cases
from util import oracle_R, orc

from ballermixplus_amd import influence

BLOCKS = (1, 2, 3, 64, 255, 256, 257, 10 ** 6)
REL_TOL = 1e-9              # of max |T| of the window: test_gpu_surfaces.py's tolerance between surfaces_kernel and host_surface
COUNTS = (0, 1, 255, 256, 257, 512, 513)


class Cat:
    """One case: gen[N], rows[N], the grids in scan order, test sites (tg, lo, hi), the listed windows, and how to get R on the
    host (R()) and a context holding the case on the device (context(engine))."""

    def __init__(self, name, gen, rows, xs, ab, As, tg, lo, hi, windows, host_R, context):
        self.name, self.gen, self.rows = name, np.asarray(gen, dtype=np.float64), np.asarray(rows, dtype=np.int32)
        self.xs, self.ab, self.As = list(xs), list(ab), list(As)
        self.tg, self.lo, self.hi = np.asarray(tg, dtype=np.float64), np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
        self.windows = [int(w) for w in windows]
        self._host_R, self._R, self.context = host_R, None, context

    def R(self):
        if self._R is None:
            self._R = self._host_R()
        return self._R

    def host(self, w, B, R=None, zcut=None):
        return influence.host_influence(self.gen, self.rows, self.R() if R is None else R, self.As, self.tg[w], self.lo[w], self.hi[w],
                                        orc.alpha_cut_z() if zcut is None else zcut, B)


def _example(name, windows):
    opt, case, ts = cases.host_side(list(cases.ALL_CASES[name][0]))
    m = case.oracle_model()

    def context(eng):
        sel = eng.NormalizedBetaBinom(case.data, case.grid, opt.nofreq, opt.MAF, opt.nosub, device=0).bind(case.neut)
        assert np.array_equal(sel.rows, m.row)
        sel.ctx.set_tests(ts.test_gen, ts.lo, ts.hi)
        return sel.ctx

    M = len(ts)
    return Cat(name, m.genpos, m.row, case.xs, case.abetas, case.As, ts.test_gen, ts.lo, ts.hi, [w % M for w in windows], lambda: m.R,
               context)


def _synthetic(name, eng, sizes, k, nn, gen, As, tg, lo, hi, windows):
    from ballermixplus_amd.hostmodel import Grids
    N = len(gen)
    cnt = {}
    for a, b in zip(np.asarray(k).tolist(), np.asarray(nn).tolist()):
        cnt[(a, b)] = cnt.get((a, b), 0) + 1
    spect = {key: v / N for key, v in cnt.items()}
    props = {int(n): sum(v for (a, b), v in spect.items() if b == n) for n in sizes}
    xs, ab, _ = Grids(None, None, False, False, None, None).scan_order()
    model = eng.ModelArrays('B2', 1, sizes, spect, props, xs, ab)
    rows = model.rows_of(k, nn)

    def context(e):
        ctx = e.Context(0)
        ctx.set_model(model, As)
        ctx.set_sites(gen, rows)
        ctx.set_tests(tg, lo, hi)
        return ctx

    return Cat(name, gen, rows, xs, ab, As, tg, lo, hi, windows, lambda: oracle_R('B2', sizes, 1, spect, props, xs, ab), context)


def ragged(eng, seed=77):
    """test_gpu_surfaces.py's chromosome of three sample sizes with position ties, off-site and duplicated test positions and
    windows that are empty, clipped or do not contain the test position."""
    rng = np.random.default_rng(seed)
    N, sizes = 1500, (12, 33, 50)
    scale = 3e-6
    gen = np.sort(np.round(np.cumsum(rng.geometric(0.2, N)).astype(np.float64) / 3) * 3 * scale)
    nn = rng.choice(np.array(sizes), N)
    k = np.array([rng.integers(1, h + 1) for h in nn])
    As = [3.5, 200.0, 1500.0, 40000.0, 1e6, 1e8, 7e8]
    tg = gen[::7].copy()
    tg[::5] += scale * 0.37
    tg = np.sort(np.concatenate([tg, tg[:5]]))
    c = np.searchsorted(gen, tg)
    lo = np.maximum(c - 150, 0).astype(np.int64)
    hi = np.minimum(c + 151, N - 1).astype(np.int64)
    lo[::4] = np.minimum(lo[::4] + rng.integers(0, 300, len(lo[::4])), N - 1)
    hi[1::4] = np.maximum(hi[1::4] - rng.integers(0, 300, len(hi[1::4])), 0)
    lo[2], hi[2] = -5, 10 * N
    empty = np.nonzero(hi < lo)[0]
    beside = np.nonzero((hi >= lo) & ((gen[np.clip(lo, 0, N - 1)] > tg) | (gen[np.clip(hi, 0, N - 1)] < tg)))[0]
    assert len(empty) and len(beside)
    windows = [2, 0, len(tg) - 1, int(empty[0]), int(beside[0]), int(beside[-1]), 57, 101, 150]
    return _synthetic('ragged', eng, sizes, k, nn, gen, As, tg, lo, hi, windows)


def _A_for_count(d, K, zcut):
    """The largest A at which exactly the K nearest sites have A * d <= zcut (test_gpu_surfaces.py's)."""
    if K == 0:
        A = zcut / d[0]
        while A * d[0] <= zcut:
            A = np.nextafter(A, np.inf)
        return float(A)
    A = zcut / d[K - 1]
    while A * d[K - 1] > zcut:
        A = np.nextafter(A, 0.0)
    while np.nextafter(A, np.inf) * d[K - 1] <= zcut:
        A = np.nextafter(A, np.inf)
    assert A * d[K - 1] <= zcut < A * d[K]
    return float(A)


def edges(eng, seed=4):
    """test_gpu_surfaces.py's edge chromosome: 700 sites around the off-site position 1.0 and three at one position far out; A
    values for qualifying counts of 0, 1, 255, 256, 257, 512 and 513, in no particular order."""
    zcut = orc.alpha_cut_z()
    h = 5e-5
    j = np.arange(350, dtype=np.float64)
    left, right = 1.0 - (2 * j + 1) * h, 1.0 + (2 * j + 2) * h
    tY = float(right[300])
    gen = np.sort(np.concatenate([left, right, [tY, tY]]))
    tX = 1.0
    d = np.sort(np.abs(gen - tX))
    As = [_A_for_count(d, K, zcut) for K in COUNTS]
    As = [As[i] for i in (3, 0, 6, 2, 5, 1, 4)] + [1e8]
    N = len(gen)
    rng = np.random.default_rng(seed)
    n = 20
    k = rng.integers(1, n + 1, N)
    iY = int(np.searchsorted(gen, tY))
    tg = np.array([tX, tX, tY, tY, tY])
    lo = np.array([0, 340, 0, iY, 20], dtype=np.int64)
    hi = np.array([N - 1, 361, N - 1, iY + 2, 19], dtype=np.int64)
    return _synthetic('edges', eng, (n,), k, np.full(N, n), gen, As, tg, lo, hi, [0, 1, 2, 3, 4])


def catalogue(eng):
    """Every case of the GPU comparison, by name."""
    return {'ex1_B2': lambda: _example('ex1_B2', [0, 400, -1]),
            'ex1_B2_fixX_fixAlpha_listA': lambda: _example('ex1_B2_fixX_fixAlpha_listA', [0, 300, 555, -1]),
            'ragged': lambda: ragged(eng),
            'edges': lambda: edges(eng)}


NAMES = ('ex1_B2', 'ex1_B2_fixX_fixAlpha_listA', 'ragged', 'edges')


def tolerance(T):
    """The GPU comparison's absolute tolerance of one window: REL_TOL of max |T| (0 for a window without a value)."""
    T = np.asarray(T)
    return REL_TOL * float(np.nanmax(np.abs(T))) if (~np.isnan(T)).any() else 0.0
