"""Seeded chromosomes whose selection table has a chosen exponent range: the input of tests/test_tablespan_cpu.py and
tests/test_gpu_table_span.py.  numpy only; the one figure taken from a selection table (the largest P_sel of the extreme row over
the grid) is handed in by the caller from the oracle's own sel_table, so nothing here depends on the library under test.

Why: every scan kernel keeps a window's likelihood as a running product of factors 1 + alpha R[row] and pulls the exponent out at
intervals it derives from span_hi = ceil(log2(1 + max R)) (bmx_ctx_set_model), inside a 1000-bit budget.  Every other spectrum of
the GPU tests is tabulated from the test's own data (span_hi ~ 8), bar one point at span_hi = 84.  Here the neutral probability of
ONE row, (k, n) = (7, 30), is set so that log2(1 + max R) = span - 0.5 for a requested span: half a bit to either integer, so the
device's table (which agrees with the oracle's to 1e-12) cannot land on the other side of the ceil.

Recipe.  N = 3000 sites, n = 30, B_2, minCount 1, the default x / alpha_beta grid (10 x 44 points: 7 slices of 64 pairs) and the A
list '200,1000,5000,100000'.  All draws come from ONE np.random.default_rng(SEED), always all of them, in this order:
  1. genPos = cumsum(rng.geometric(0.3, N)) * 2e-6
  2. k      = rng.integers(1, 31, N)                      counts, uniform on 1 .. 30
  3. u      = rng.random(N)                               'common': k = 7 where u < 0.4
  4. v      = rng.random(N)                               'low': k = LOW_K where v < 0.1
  5. ti     = rng.integers(0, 3, N); w = rng.random(N)    'large': total = (150, 160, 170)[ti], k = 1 + floor(w total)
Placements of the extreme row (applied after the draws):
  'rare'    k[::50] = 7
  'common'  k[u < 0.4] = 7, then k[::50] = 7: 40 % of all sites
  'run'     as 'rare', plus k[1500:1564] = 7: a full 64-site pass with every factor at the maximum
  'low'     k[v < 0.1] = LOW_K, then as 'rare'; g(LOW_K, 30) = 1.0, so that R = P_sel - 1 reaches -1 + 5.9e-7 on that row, and the
            site pairs LOW_PAIRS (both of row LOW_K) lie 1e-9 apart: genPos[j + 1] = genPos[j] + 1e-9.  Both sites of the first and last
            pair, and the sites 1530 and 1570 of the middle two, are test sites at every stride
  'large'   sample sizes (150, 160, 170): 483 table rows, 247 KB per slice, read from L2 (the <false> kernel forms); extreme
            row (7, 150) on every 50th site
The extreme row is the most frequent row of the site array in every placement (the solo kernel's row0, moment slot 0): its planted
sites come on top of its share of the uniform counts.  In 'low' the most frequent row is (LOW_K, 30).
Spectrum: tabulated from the counts (g = share of the sites, props = share of the sample size), then spect[extreme row] =
sel_max props[n] / 2^(span - 0.5) with sel_max = max over the grid of P_sel(extreme row).  (It no longer sums to 1: the checksum of a
helper file is not the library's business.)

Test sites of a case: the first 32 sites, 83 sites at the case's stride around site 1530 (groups straddle the run 1500 .. 1563) and
the last 32 sites.  Strides 1, 5 (prepared J = 16, J = 8) and 20 (solo).  Windows: the whole chromosome, except on 'common', where
test site i gets the index window [i - 500, i + 500]: the scan kernels clamp the binary exponent of a window's product to
+-131 071 (the argmax is defined for |T| <= 1.8e5), and 1 265 sites at 2^124.5 and more take a whole-chromosome
window past that (T = 2.1e5 at span 125, 4.2e5 at span 240); 1 001 sites keep it below 1.5e5.

Measured with the committed seed and the oracle's own table (tests/test_tablespan_cpu.py asserts the conditions and prints these
figures):
  Sites of the extreme row / of the runner-up row: rare 162 / 128, common 1 265 / 83, run 223 / 126, large 64 / 15; low: 376 of (10, 30),
    151 of the extreme row.  Windows of the sites 0 / 1530 / N - 1 without index bounds: 2 999 sites at A = 200, 2 785 / 2 999 / 2 786 at
    1000, 548 / 1 163 / 535 at 5000, 36 / 60 / 26 at 100000.
  Span: log2(1 + max R) = span - 0.500000 on every set, the maximum on the extreme row; the other rows reach 2^3.8 .. 2^4.4 (n = 30) and
    2^6.3 ('large'); min R = -1 + 8e-11 (n = 30), exactly -1 on 'large'.
  Eight factors ('common' and 'run', all 294 compared windows of the strides 1 and 20, A = 200, the grid point of max R): log2 of the
    product of the first eight entries of the extreme row in the solo stream's order is at most 1 020.0 at span 128 (the placed
    table cannot overflow there: 8 x 127.5 bits, alpha < 1) and, in EVERY window, above 1 024 from span 129 on: 1 028 at 129, 1 276 at 160,
    1 596 at 200, 1 916 at 240.
  Grouped budget: SP span_hi = 160 / 320 / 640 at span 40 and 248 / 496 / 992 at span 62 for J = 16 / 8 / 4.
  Low side: 1 + R of row (10, 30) = 5.9e-7 .. 0.075; smallest factor 2^-20.3 at A = 200, 2^-19.3 at 1000, 2^-17.4 at 5000, 2^-13.3 at 100000
    (the floor is 1 - alpha = A 1e-9, not R).
  Oracle CLR: rare 1.7e3 (span 12) .. 5.3e4 (240); common 3.2e3 .. 1.47e5; run 2.4e3 .. 7.4e4; low 1.4e3 .. 1.6e3; large 3.7e3 .. 1.7e4: below
    the 1.8e5 of the kernels' exponent clamp.  Every window has a winner.
  Runner-up margins / T, smallest per set: rare 1.6e-7 (span 240) .. 1.0e-6; common 2.6e-7 (span 240, stride 1) .. 7.3e-5; run 3.1e-6 at
    span 12, and from span 40 on ONE window below the bar, site 12 (alpha_beta 6 leads 5 by 8.0e-4 of T: 7.2e-8 .. 1.1e-8), listed in TIED;
    low 9.8e-6; large 4.9e-7; 'run' at span 62 with A = 5000 alone 1.03e-7 (with 200, 1000 or 100000 alone windows fall below 1e-7).
  C oracle against a long-double restatement of 2 sum log1p(alpha R), eight windows per placement: 3.5e-15 relative at span 62,
    3.6e-15 at span 240 (asserted: 1e-12), so the GPU tests keep the project's rtol = 1e-9, atol = 1e-12.
"""
import numpy as np

SEED = 20261019
N = 3000
NSAMP = 30
EXT_K = 7
LOW_K = 10
LOW_G = 1.0
LOW_PAIRS = (5, 1529, 1570, 2990)       # genPos[j + 1] = genPos[j] + 1e-9
LOW_GAP = 1e-9
RUN_SITES = (1500, 1564)
LARGE_SIZES = (150, 160, 170)
A_LIST = '200,1000,5000,100000'
ONE_A = '5000'
MARGIN = 0.5                            # log2(1 + max R) = span - MARGIN

# 62: the last grouped span, 63: the first the planner sends to the solo kernel at any stride; 125 / 126: the solo kernel's limit is
# 8 / 7; 128: the first span_hi at which eight factors could overflow (2^128 each), 129: the first at which the placed table does;
# 240: the library's limit
SPANS = (12, 40, 62, 63, 100, 125, 126, 128, 129, 160, 200, 240)
GROUPED_SPANS = (12, 40, 62)            # can_group: span_hi <= 62
SOLO_SPANS = tuple(s for s in SPANS if s > 62)
PLACEMENTS = ('rare', 'common', 'run')
STRIDES = {True: (1, 5), False: (1, 20)}          # [span <= 62]
LOW_SPAN = 12
LARGE_SPANS = (50, 200)

# the boundaries of ballermixplus_amd/csrc/bmxscan.hip these spans are chosen around (test_tablespan_cpu.py matches them against
# the source)
GROUP_SPAN_MAX = 62     # can_group
SPAN_LIMIT = 240        # set_model
BUDGET_BITS = 1000      # spend()
SPAN_GENERIC = 54       # bits of a factor 1 - alpha, alpha < 1
SOLO_LIM_CAP = 16       # renorm_every = min(16, 1000 / max(span_hi, 54))

CENTRE = 1530
RUN = 83
ENDS = 32
COMMON_HALF = 500       # 'common': index windows [i - 500, i + 500]
CLR_LIMIT = 1.8e5       # 2 ln 2 x 131 071: the exponent clamp of the kernels' best-tracking

# Near-ties.  The GPU tests compare (x, alpha_beta, A, nSites) exactly, so every compared window's best grid point must beat the
# runner-up by more than TIE_BAR of its T in the oracle.  (With whole-chromosome windows 'common' cannot get there: T is then
# n_ext log P_sel(7 | x, alpha_beta) plus a small rest, and that term's maximum over alpha_beta lies at ~175, half way between the grid
# points 170 and 180 -- 142 of 147 windows within 1e-7 at span 62.  The index windows, cut off at either end of the chromosome
# and uneven in genetic length, do not have that symmetry.)
TIE_BAR = 1e-7
# (set, span, stride[, A list]) -> indices INTO tests_of(stride) of the windows below the bar: skipped by the GPU tests
# (test_tablespan_cpu.py asserts that the list is complete and holds at most 2 % of a case's windows).  Site 12 of 'run': alpha_beta 6
# leads alpha_beta 5 by 8e-4 of a T of 1.1e4 .. 7.3e4
TIED = {('run', s, d): (12,) for s in SPANS if s >= 40 for d in STRIDES[s <= 62]}


def tests_of(stride):
    """Site indices of a case's test sites: the first 32, 83 at `stride` around 1530, the last 32."""
    return np.concatenate([np.arange(ENDS), CENTRE + stride * (np.arange(RUN) - RUN // 2), np.arange(N - ENDS, N)])


def windows_of(kind, idx):
    """Inclusive index windows (lo i64[], hi i64[]) of the test sites idx of data set `kind`."""
    idx = np.asarray(idx, dtype=np.int64)
    if kind == 'common':
        return np.maximum(idx - COMMON_HALF, 0), np.minimum(idx + COMMON_HALF, N - 1)
    return np.zeros(len(idx), np.int64), np.full(len(idx), N - 1, np.int64)


def solo_lim(span):
    """renorm_every of bmx_ctx_set_model."""
    return max(1, min(SOLO_LIM_CAP, BUDGET_BITS // max(span, SPAN_GENERIC)))


def chromosome(kind, seed=SEED):
    """(genPos f64[N], count i64[N], total i64[N]) of data set `kind`: a placement, 'low' or 'large'."""
    rng = np.random.default_rng(seed)
    gen = np.cumsum(rng.geometric(0.3, N)) * 2e-6
    k = rng.integers(1, NSAMP + 1, N)
    u = rng.random(N)
    v = rng.random(N)
    ti = rng.integers(0, 3, N)
    w = rng.random(N)
    total = np.full(N, NSAMP, dtype=np.int64)
    if kind == 'large':
        total = np.array(LARGE_SIZES, dtype=np.int64)[ti]
        k = 1 + np.floor(w * total).astype(np.int64)
        total[::50] = LARGE_SIZES[0]
    elif kind == 'common':
        k[u < 0.4] = EXT_K
    elif kind == 'low':
        k[v < 0.1] = LOW_K
    elif kind not in ('rare', 'run'):
        raise ValueError(kind)
    k[::50] = EXT_K
    if kind == 'run':
        k[RUN_SITES[0]:RUN_SITES[1]] = EXT_K
    if kind == 'low':
        for j in LOW_PAIRS:
            gen[j + 1] = gen[j] + LOW_GAP
            k[j] = k[j + 1] = LOW_K
    return gen, k.astype(np.int64), total


def ext_row(kind):
    return (EXT_K, LARGE_SIZES[0] if kind == 'large' else NSAMP)


def sizes_of(kind):
    return list(LARGE_SIZES) if kind == 'large' else [NSAMP]


def spectrum(kind, span, sel_max, count, total):
    """({(k, n): g}, props) of data set `kind` with the extreme row placed at `span`.  sel_max: the largest P_sel of the extreme row
    over the grid (oracle sel_table('B2', n, 1, xs, abetas)[:, :, EXT_K].max())."""
    cnt = {}
    for a, b in zip(count.tolist(), total.tolist()):
        cnt[(a, b)] = cnt.get((a, b), 0) + 1
    spect = {key: c / N for key, c in cnt.items()}
    props = {n: float(np.mean(total == n)) for n in sizes_of(kind)}
    e = ext_row(kind)
    spect[e] = float(sel_max) * props[e[1]] / 2.0 ** (span - MARGIN)
    if kind == 'low':
        spect[(LOW_K, NSAMP)] = LOW_G
    return spect, props


def window_of(gen, i, A, lo=0, hi=N - 1):
    """Site indices of test site i's window at A (alpha >= 1e-8, position != the test site's, lo <= index <= hi) and their alpha."""
    al = np.exp(-A * np.abs(gen - gen[i]))
    at = np.arange(len(gen))
    keep = (al >= 1e-8) & (gen != gen[i]) & (at >= lo) & (at <= hi)
    return np.nonzero(keep)[0], al[keep]


def row0_stream(gen, row, row0, i, A, lo=0, hi=N - 1):
    """alpha of the window's row0 sites in the order the solo kernels' stream lists them: right of the test site nearest
    first, then left of it nearest first (from span 40 on every site of the extreme row is a near entry: alpha max|R| >= 1e-8 2^39)."""
    idx, al = window_of(gen, i, A, lo, hi)
    is0 = row[idx] == row0
    right = idx > i
    return np.concatenate([al[is0 & right], al[is0 & ~right][::-1]])
