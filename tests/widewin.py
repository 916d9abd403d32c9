"""A seeded cold-spot chromosome with a planted signal: the input of tests/test_widewin_cpu.py and
tests/test_gpu_wide_windows.py.  numpy only; the selection table of the planted signal is handed in by the caller
(oracle/bmx_oracle.py sel_table), so nothing here depends on the library under test.

Why: every other large oracle comparison of the suite runs on synth.py data -- uniform recombination rate, ~2 500 sites
on each side of a test site at A = 100, tie-free positions -- where the scan's overflow paths are never taken and the
widest windows (smallest A) never win.  Here an A = 100 window holds up to ~46 000 sites, so every stream cap of
ballermixplus_amd/csrc/bmxscan.hip (the literals below) is exceeded, and the planted signal makes the wide A the winner.

Recipe.  All draws come from ONE np.random.default_rng(SEED), in this order:
  1. gaps   = rng.geometric(1 / mean) for the N = 60 000 sites, in units of 1e-6: mean 8 (cold) everywhere except the two hot
              spots [4900, 5000) and [55000, 55100) with mean 72; then gaps[30000:30500] = 0 (a run of 500 exact ties: 501
              equal positions) and genPos = cumsum(gaps) / 1e6.
              (The chromosome's ends are cold and the hot spots short on purpose: the first and the last 64 sites must see
              >= 2 x 8192 far candidates in their one zone, which 5 000 sites at a spacing of 72 at either end cannot give --
              an A = 100 window reaches 0.184 from its test site.  Site 5000 is still where a cold region starts.)
  2. sizes  = 100 where rng.random(N) < 0.8, else rng.integers(90, 100, N)      (data set 'l2' only: two draws of N)
  3. plant  = rng.random(N) < alpha_i, alpha_i = max over the centres c of exp(-A* |g_i - g_c|), A* = 100; centres 6000, 30000 and
              30250 (inside the tie run), where the GPU tests look, and 32 and N - 33, so that the windows of the first and last
              64 sites have a winner too and are not compared as empty results
  4. count  = inverse CDF at rng.random(N) of the planted spectrum (B_2 selection table at x = 0.3, alpha_beta = 20, counts
              1 .. n_i renormalised; handed in by the caller) where plant, of the neutral spectrum g(k | n_i) elsewhere.
Neutral spectrum, given exactly (never tabulated from the draws): g(k | n) = 0.3 (1/k) / H_{n-1} for 1 <= k < n, g(n | n) = 0.7;
spect[(k, n)] = props[n] g(k | n) with props = {100: 1} ('lds') or {100: 0.8, 90 .. 99: 0.02 each} ('l2': 1 056 table rows, read
from L2, 254 moment slots).  Count 0 does not occur (minCount = 1), so every row a site can carry has a finite g.

Measured with the committed seed, 'lds' set, B_2, the oracle's own table (tests/test_widewin_cpu.py asserts the conditions and
prints these figures), over all runs of TEST_RUNS:
  A = 100: windows of 22 320 .. 46 670 sites.  Far candidates (sites of the window with alpha max_grid|R[row]| <= eps) in the larger
           zone of a test site: 18 436 .. 19 917 at eps = 0.15, 16 571 .. 18 649 at eps = 0.05 (the minimum: the first 64 sites);
           around 30000 / 30250 the smaller zone holds 19 664 (0.15) / 18 517 (0.05) at least.  Site 6000: 2 707 on the left,
           19 837 on the right at eps = 0.15.  Far candidates outside the 64 most frequent rows: 544 .. 601 in the larger zone,
           >= 521 in both zones around 30000 / 30250 (0 in the short zone near the chromosome's start: those rows have max|R| up to
           147 and turn far only 0.07 from the test site).  Oracle CLR 5 179 .. 9 064 around the three centres, 3 799 .. 5 394 on
           the other runs.  Exponent budget of clr_scan_prepared_kernel (2 + nfar far_bits per zone, nfar capped at 3 584):
           bitsR + bitsL = 1 213 .. 1 710 wherever a test site has two zones (> 900: split), 857 on the first and last sites.
  A = 250: 4 053 .. 7 831 far candidates per zone at eps = 0.15 (6 999 .. 7 831 around 30000 / 30250; the one zone of the first
           and last sites 6 837 .. 6 971): between 3 584 and 8 192.  Oracle CLR 3 381 .. 7 611 around the centres, 2 372 .. 3 000 elsewhere.
  Four of the widest windows (WIDEST: 46 668 and 3 x 46 164 sites): the best (x, alpha_beta) point at A = 100 lies 1.3e-3 .. 2.3e-3 T
           above every other; the C oracle agrees with a long-double restatement of 2 sum log1p(alpha R) to 9.2e-15 relative.
"""
import numpy as np

SEED = 20261018
N = 60000
COLD_MEAN, HOT_MEAN = 8, 72
HOT_SPOTS = ((4900, 5000), (55000, 55100))
TIE_RUN = (30000, 30500)
CENTRES = (6000, 30000, 30250)          # where the GPU tests look for the wide A to win
END_CENTRES = (32, N - 33)               # planted too, so that the first and last 64 windows have a winner to compare
A_STAR = 100.0
PLANT_X, PLANT_ABETA = 0.3, 20.0
P_SUB = 0.7

# the caps of ballermixplus_amd/csrc/bmxscan.hip these inputs are shaped to exceed (test_widewin_cpu.py matches them against the source)
P_FAR_CAP = 3584        # far sites per zone, prep_kernel
S_FAR_CAP = 8192        # ... solo kernels
FAR_CAP = 8192          # ... round-2 kernels
SER_CAP = 64            # series entries per zone
MID_CAP = 32            # sites between the test sites of a group staged in LDS
P_EPS = 0.15            # far test of the prepared kernels: alpha max|R| <= P_EPS
S_EPS = 0.05            # ... of the solo and round-2 kernels
FAR_BITS = 0.15 * 1.4427 * 1.1    # exponent bits one far site can move a product by (P.far_bits of the prepared kernels, a float)
BUDGET_BITS = 900       # both zones' far fields go into one exp only while 2 + nfar far_bits of the two zones add up to at most this
MOM_ROWS = 64           # rows with a moment slot while the R slice sits in LDS: the most frequent rows of the site array

A_LISTS = ('100', '250', '100,250,1000,5000,1000000')
RUN = 83                # test sites per run: five groups of 16 and a partial one

def run_around(centre, stride, count=RUN):
    """count site indices at the given stride around `centre`.  The library picks the group size from the MEDIAN index gap between
    the located test sites, and test sites inside the tie run all sit on one position (gap 0): a strided run around 30000
    therefore starts 70 test sites before it and ends 12 test sites inside the tie run."""
    before = count // 2 if stride == 1 or centre != TIE_RUN[0] else 70
    return centre + stride * (np.arange(count) - before)


# index runs of test sites the GPU tests use (stride 1); run_around() gives the strided ones (centres 6000 and 30000)
TEST_RUNS = {
    'c6000': np.arange(6000 - 41, 6000 + 42),
    'c30000': np.arange(30000 - 41, 30000 + 42),         # straddles the start of the tie run
    'c30250': np.arange(30250 - 41, 30250 + 42),         # wholly inside the tie run
    'first': np.arange(0, 64),
    'last': np.arange(N - 64, N),
    'edge': np.arange(5000, 5000 + RUN),                 # starts where the hot spot ends and the cold region resumes
    'straddle': np.arange(4960, 4960 + RUN),             # its third group (4992 .. 5007) lies across that edge
}
for _c in (6000, 30000):
    for _s in (5, 16):
        TEST_RUNS['c%d_s%d' % (_c, _s)] = run_around(_c, _s)
CENTRE_RUNS = ('c6000', 'c30000', 'c30250', 'c6000_s5', 'c6000_s16', 'c30000_s5', 'c30000_s16')
BOTH_ZONES = ('c30000', 'c30250', 'c30000_s5', 'c30000_s16')        # runs whose two zones are both past every cap
WIDEST = (29990, 30000, 30250, 30499)                    # four of the widest windows (tie run: 500 tied sites excluded)


def neutral(n):
    """g(k | n) for k = 0 .. n (g(0) = 0: the count does not occur)."""
    g = np.zeros(n + 1)
    k = np.arange(1, n)
    g[1:n] = (1.0 - P_SUB) * (1.0 / k) / np.sum(1.0 / k)
    g[n] = P_SUB
    return g


def sizes_and_props(kind):
    if kind == 'lds':
        return [100], {100: 1.0}
    if kind == 'l2':
        props = {n: 0.02 for n in range(90, 100)}
        props[100] = 0.8
        return list(range(90, 101)), props
    raise ValueError(kind)


def spectrum(kind):
    """{(k, n): props[n] g(k | n)} for k = 1 .. n, and props."""
    sizes, props = sizes_and_props(kind)
    spect = {}
    for n in sizes:
        g = neutral(n)
        for k in range(1, n + 1):
            spect[(k, n)] = props[n] * float(g[k])
    return spect, props


def positions(rng):
    mean = np.full(N, float(COLD_MEAN))
    for a, b in HOT_SPOTS:
        mean[a:b] = HOT_MEAN
    gaps = rng.geometric(1.0 / mean)
    gaps[TIE_RUN[0]:TIE_RUN[1]] = 0
    return np.cumsum(gaps) / 1e6


def _inverse_cdf(p, u):
    """Counts 1 .. n drawn by inverse CDF from p[1:] (renormalised) at the uniforms u."""
    c = np.cumsum(p[1:])
    c /= c[-1]
    return np.minimum(np.searchsorted(c, u, side='right'), len(c) - 1) + 1


def chromosome(kind, sel_of, seed=SEED):
    """(genPos f64[N], count i64[N], total i64[N], planted bool[N]) of data set `kind` ('lds' or 'l2').
    sel_of(n) -> the planted spectrum over k = 0 .. n (any scale; oracle sel_table('B2', n, 1, [PLANT_X], [PLANT_ABETA])[0, 0])."""
    rng = np.random.default_rng(seed)
    gen = positions(rng)
    sizes, _ = sizes_and_props(kind)
    if kind == 'l2':
        u = rng.random(N)
        other = rng.integers(90, 100, N)
        total = np.where(u < 0.8, 100, other).astype(np.int64)
    else:
        total = np.full(N, 100, dtype=np.int64)
    alpha = np.zeros(N)
    for c in CENTRES + END_CENTRES:
        alpha = np.maximum(alpha, np.exp(-A_STAR * np.abs(gen - gen[c])))
    planted = rng.random(N) < alpha
    u = rng.random(N)
    count = np.zeros(N, dtype=np.int64)
    for n in sizes:
        at = total == n
        count[at & planted] = _inverse_cdf(np.asarray(sel_of(n), dtype=np.float64), u[at & planted])
        count[at & ~planted] = _inverse_cdf(neutral(n), u[at & ~planted])
    return gen, count, total, planted


# ------------------------------------------------------------------------------------------------ the definitions of DESIGN.md

def window_of(gen, i, A, lo=0, hi=None):
    """Site indices of test site i's window at A (alpha >= 1e-8, position != the test site's, lo <= index <= hi: the
    reference's predicate) and their alpha."""
    hi = len(gen) - 1 if hi is None else hi
    t = gen[i]
    rad = 19.0 / A
    i0 = max(int(np.searchsorted(gen, t - rad, 'left')), lo)
    i1 = min(int(np.searchsorted(gen, t + rad, 'right')), hi + 1)
    g = gen[i0:i1]
    al = np.exp(-A * np.abs(g - t))
    keep = (al >= 1e-8) & (g != t)
    return np.arange(i0, i1)[keep], al[keep]


def far_counts(gen, row, rmax, frequent, i, A, eps):
    """Of test site i at A: (sites, far candidates, far candidates outside the frequent rows) of the (left, right) zone.
    A far candidate is a site of the window with alpha max_grid|R[row]| <= eps."""
    idx, al = window_of(gen, i, A)
    far = al * rmax[row[idx]] <= eps
    rare = far & ~frequent[row[idx]]
    left = gen[idx] < gen[i]
    return tuple((int(z.sum()), int((far & z).sum()), int((rare & z).sum())) for z in (left, ~left))
