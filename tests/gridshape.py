"""Seeded inputs that walk the scan kernels through grid shapes and exact argmax ties: the input of tests/test_gridshape_cpu.py
and tests/test_gpu_grid_shapes.py.  numpy only; nothing here depends on the library under test or on an oracle.

Why.  Every scan kernel puts the (x, alpha_beta) pairs on lanes, 64 per wave ('slice'): NP = pairs padded to 64, nslices = NP / 64.
The other GPU tests know four shapes (510, 440, 44 pairs and 1 pair).  SHAPES below are chosen around the slice count and the number
of real lanes of the last slice; TIE_GRIDS repeats grid values, so that whole classes of grid points have bit-identical table
columns and the promised argmax order (larger T, else smaller linear index (A, x, alpha_beta): DESIGN.md section 2) decides.

Data.  N = 4003 sites.  All draws come from ONE np.random.default_rng(SEED), always all of them, in this order:
  1. genPos = cumsum(rng.geometric(0.3, N)) * 2e-6; then genPos[j + 1] = genPos[j] for j in POS_TIES (exact ties; one triple)
  2. u = rng.random(N): the site is 'shaped' where u < SHAPED = 0.5, else neutral
  3. v = rng.random(N): the neutral count floor((n + 1)^v) clipped to 1 .. n  (density ~ 1 / k)
  4. p = rng.beta(a, a / x - a) with (x, a) = BLOCK_PARAMS[(site // 400) % 6]: blocks of 400 sites with their own (x, alpha_beta)
  5. m = rng.random(N): p -> 1 - p where m < 0.5
  6. ti = rng.integers(0, 3, N): the sample size of data set 'large' is LARGE_SIZES[ti]
  7. the shaped count rng.binomial(20, p);  8. w = rng.random(N): 'large' spreads it, floor((k + w) / 21 n); both clipped to 1 .. n
Data set 'small': n = 20 everywhere (21 table rows: the R slice lives in LDS).  Data set 'large': sample sizes (150, 160, 170), 483
rows, 247 KB per slice: read from L2 (the <false> kernel forms).
Spectrum: g tabulated from the NEUTRAL counts of all N sites (the draw of step 3, whether the site uses it or not) with one
pseudo-count per row, props = share of the sample size: the shaped half of the sites is a real excess over it, CLR up to 235
('small') and 694 ('large'), the winning A spread over the whole list.
The stretch LOW (200 sites) carries ONE row, (LOW_K, n) with n = 20 / 150, whose neutral probability is set to LOW_G = 8: R = P_sel
prop / LOW_G - 1 lies in -1 .. -0.97 there over the whole grid, so a test site well inside it has T < 0 at every grid point and
every A: the windows without a winner, which a pad lane (R = 0, product exactly 1) or a stale lane would steal.  Every case holds
at least 10 of them that are not empty (asserted: 5), the dense run about 210.

A list A_LIST: windows from a few dozen sites (150000) to the whole chromosome (200).

Test sites (site indices).  spb = test sites per workgroup in plan_scan of bmxscan.hip at M < 65536: 64 for the prepared J = 16
form, 4 J x 3 = 96 for the prepared J = 8 form with the table in LDS (twelve waves), 4 J = 32 with the table in L2, 1024 / 64 = 16
for the solo form.  The prepared and solo launches are padded to whole rounds of 8 chunks.
  dense     sites DENSE0 .. DENSE0 + 612: 613 = 9 x 64 + 37 (J = 16: ten chunks, 39 groups, the last of 5 test sites)
  stride 5  every 5th site: 801 = 8 x 96 + 33 (J = 8: nine chunks in LDS, 26 in L2; 101 groups, the last of one test site)
  stride 20 every 20th site: 201 = 12 x 16 + 9 (solo: thirteen chunks)
The dense run covers the stretch LOW and 250 / 160 sites of signal on either side.
Windows: 'all' (no index bounds) or 'ragged' (index windows around the test site, lowered start as mode 2 of the randomised
parity test: some empty, some wholly right of the test site), moved so that they never cut between two tied positions.

Window sizes of the sites 0 / 2000 / N - 1: 4002 at A = 200; 548 / 1165 / 611 at 5000; 102 / 193 / 94 at 30000; 23 / 34 / 14 at 150000.
Ragged windows: 183 / 224 / 50 of the 613 / 801 / 201 are empty.

Near-ties: with the committed seed 31 of the 74 grid cases have windows below the bar (at most 9 of 613, 8 of 801, 4 of 201: TIED),
the tie-grid cases none; the smallest lead that is compared exactly is 1.0e-7 of T.  C oracle against a long-double restatement
of 2 sum log1p(alpha R): 7.7e-15 relative.
tests/test_gridshape_cpu.py asserts all of this with the oracles alone and prints the measured figures.
"""
import numpy as np

SEED = 20261019
N = 4003
NSAMP = 20
LARGE_SIZES = (150, 160, 170)
A_LIST = (200.0, 5000.0, 30000.0, 150000.0)
POS_TIES = (7, 1203, 1204, 2600, 3999)          # genPos[j + 1] = genPos[j]; 1203 / 1204: three sites on one position
BLOCK = 400
BLOCK_PARAMS = ((0.3, 5.0), (0.12, 1.5), (0.45, 12.0), (0.2, 0.6), (0.38, 8.0), (0.08, 3.0))
LOW = ((3600, 3800),)
LOW_K = 1
SHAPED = 0.5                    # share of the sites drawn from their block's beta-binomial
LOW_G = 8.0
WAVE = 64

# pairs: (nx, nab) -- see the table in the module docstring of tests/test_gpu_grid_shapes.py
SHAPES = ((10, 1), (1, 51), (7, 9), (64, 1), (1, 64), (5, 13), (2, 64), (3, 43), (9, 64), (16, 64), (17, 61))
# (npairs, nslices, real lanes of the last slice)
SHAPE_FACTS = {(10, 1): (10, 1, 10), (1, 51): (51, 1, 51), (7, 9): (63, 1, 63), (64, 1): (64, 1, 64), (1, 64): (64, 1, 64),
               (5, 13): (65, 2, 1), (2, 64): (128, 2, 64), (3, 43): (129, 3, 1), (9, 64): (576, 9, 64), (16, 64): (1024, 16, 64),
               (17, 61): (1037, 17, 13)}
L2_SHAPES = ((5, 13), (3, 43), (9, 64), (17, 61))
VARIANT_SHAPES = ((5, 13), (9, 64), (17, 61))
PROFILE_SHAPES = ((5, 13), (3, 43), (17, 61))
SURFACE_SHAPES = ((5, 13), (16, 64), (17, 61))
REPEAT_SHAPES = ((5, 13), (17, 61))

ABETA_RANGE = (1e-3, 1e9)       # the default grid's range (hostmodel.Grids.DEFAULT_ABETA)
X_RANGE = (0.05, 0.5)           # the default grid's range

DENSE0 = 3350
DENSE_M = 613
STRIDES = (1, 5, 20)
# stride -> (plan: J (0: solo), test sites per workgroup with the table in LDS, with the table in L2)
SPB = {1: (16, 64, 64), 5: (8, 96, 32), 20: (0, 16, 16)}
RAGGED_R = 150
TIE_BAR = 1e-7

# (data set, 'grid' shape or 'tie', stride, windows) -> indices INTO tests_of(stride) of the windows whose runner-up at a different
# grid point (tie grid: in a different duplicate class) trails by no more than TIE_BAR of T in the oracle: excluded from the exact
# comparison of (x, alpha_beta, A, nSites) by the GPU tests.  tests/test_gridshape_cpu.py asserts that the list is complete and
# holds at most 2 % of a case's windows.
TIED = {('large', (5, 13), 1, 'all'): (246,),
 ('large', (17, 61), 1, 'all'): (476,),
 ('small', (1, 51), 1, 'all'): (456,),
 ('small', (1, 51), 1, 'ragged'): (191, 456),
 ('small', (1, 64), 1, 'all'): (456, 457, 459, 461),
 ('small', (1, 64), 1, 'ragged'): (173, 238, 456, 459),
 ('small', (1, 64), 5, 'ragged'): (32, 34, 41, 122, 236, 532, 535),
 ('small', (1, 64), 20, 'ragged'): (54, 126),
 ('small', (3, 43), 1, 'ragged'): (238,),
 ('small', (3, 43), 5, 'ragged'): (597,),
 ('small', (5, 13), 1, 'ragged'): (488,),
 ('small', (5, 13), 5, 'all'): (629,),
 ('small', (7, 9), 1, 'all'): (456,),
 ('small', (7, 9), 1, 'ragged'): (456,),
 ('small', (7, 9), 5, 'all'): (629,),
 ('small', (7, 9), 5, 'ragged'): (153, 342, 485),
 ('small', (9, 64), 1, 'ragged'): (121,),
 ('small', (9, 64), 5, 'all'): (629,),
 ('small', (9, 64), 5, 'ragged'): (153, 342, 551),
 ('small', (16, 64), 1, 'all'): (190,),
 ('small', (16, 64), 1, 'ragged'): (373, 466),
 ('small', (16, 64), 5, 'all'): (633, 708),
 ('small', (16, 64), 5, 'ragged'): (153, 410, 429),
 ('small', (16, 64), 20, 'all'): (177,),
 ('small', (16, 64), 20, 'ragged'): (88, 95, 102, 119),
 ('small', (17, 61), 1, 'all'): (204, 214, 218, 220, 248, 459),
 ('small', (17, 61), 1, 'ragged'): (9, 100, 110, 120, 220, 238, 248, 373, 459),
 ('small', (17, 61), 5, 'all'): (714,),
 ('small', (17, 61), 5, 'ragged'): (41, 66, 153, 189, 410, 485, 673, 714),
 ('small', (17, 61), 20, 'ragged'): (168, 189),
 ('small', (64, 1), 5, 'all'): (666,)}


def x_grid(nx):
    """nx distinct values in (0, 1), over the default grid's range."""
    if nx == 1:
        return [0.3]
    return [float(v) for v in np.linspace(X_RANGE[0], X_RANGE[1], nx)]


def abeta_grid(nab):
    """nab distinct values, log-spaced over the default grid's range."""
    if nab == 1:
        return [7.0]
    return [float(v) for v in np.logspace(np.log10(ABETA_RANGE[0]), np.log10(ABETA_RANGE[1]), nab)]


def grids_of(shape):
    """(x list, alpha_beta list, A list) of a shape."""
    return x_grid(shape[0]), abeta_grid(shape[1]), list(A_LIST)


# ----------------------------------------------------------------------------- exact ties
# Base grid: 5 x values, 11 alpha_beta values (1e-3 .. 1e5: clear of the saturated end), 3 A values; the values that win most
# windows of these data sets (x = 0.4 and 0.3, alpha_beta = 10 and 1.58) are the repeated ones.  The tie grid lists
#   x      [x0 x1 x2 x3 x4 x1 x0]                       7 values: x0 at 0 and 6, x1 at 1 and 5
#   abeta  [a0 .. a10 a5 a4]                            13 values: a5 at 5 and 11, a4 at 4 and 12
#   A      [A0 A1 A2 A0 A1 A2]                          every A twice, the copies three apart
# 91 pairs, two slices (27 real lanes in the second).  The pairs of one (x value, alpha_beta value) class, p = ix * 13 + ia:
#   (x0, a5): 5, 11, 83, 89         5 and 11 in slice 0 (the same slice), 83 and 89 in slice 1
#   (x0, a4): 4, 12, 82, 90
#   (x0, a):  ia, 78 + ia           for the unrepeated a (ia = 0 .. 3, 6 .. 10): one copy in each slice
#   (x1, a5): 18, 24, 70, 76        18 and 24 in slice 0; 70 and 76 in slice 1
#   (x1, a4): 17, 25, 69, 77
#   (x1, a):  13 + ia, 65 + ia      13 + ia in slice 0, lane 13 + ia; 65 + ia in slice 1, lane 1 + ia: the first copy in the HIGHER
#                                   lane of the LOWER slice
#   (x, a5), (x, a4) for x2, x3:    ix * 13 + (5, 11) and ix * 13 + (4, 12): both copies in one slice
#   (x4, a5): 57, 63                both in slice 0;  (x4, a4): 56, 64: lane 56 of slice 0 and lane 0 of slice 1
# Every class is repeated over A: linear index lin = iA * 91 + p, iA and iA + 3 of the same value.  class_of() gives the class
# (its smallest linear index) of every linear index; members_of(c) its members.
TIE_X_IDX = (0, 1, 2, 3, 4, 1, 0)
TIE_AB_IDX = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 5, 4)
TIE_A_IDX = (0, 1, 2, 0, 1, 2)
TIE_BASE_X = (0.4, 0.3, 0.1, 0.2, 0.5)
TIE_BASE_AB = tuple(float(v) for v in np.logspace(-3, 5, 11))
TIE_BASE_A = (200.0, 5000.0, 60000.0)
TIE_SHAPE = (len(TIE_X_IDX), len(TIE_AB_IDX))           # 7 x 13 = 91 pairs


def tie_grids():
    """(x list, alpha_beta list, A list) with repeated values."""
    return ([TIE_BASE_X[i] for i in TIE_X_IDX], [TIE_BASE_AB[i] for i in TIE_AB_IDX], [TIE_BASE_A[i] for i in TIE_A_IDX])


TIE_GRIDS = tie_grids()


def class_of():
    """i32[nA * npairs]: the smallest linear index (A, x, alpha_beta) among the grid points with the same three VALUES."""
    nx, nab = TIE_SHAPE
    first = {}
    out = np.zeros(len(TIE_A_IDX) * nx * nab, np.int32)
    for iA, a in enumerate(TIE_A_IDX):
        for ix, x in enumerate(TIE_X_IDX):
            for ia, b in enumerate(TIE_AB_IDX):
                lin = (iA * nx + ix) * nab + ia
                out[lin] = first.setdefault((a, x, b), lin)
    return out


def members_of(c):
    return np.nonzero(class_of() == c)[0]


# the classes the layout was chosen for (pairs p; with every A twice the linear indices are p, p + 3 * 91 at iA, iA + 3)
TIE_CLASSES = {
    'same slice': (5, 11),                                  # (x0, a5): lanes 5 and 11 of slice 0 (and 83, 89 in slice 1)
    'across, first copy in the higher lane': (14, 66),      # (x1, a1): lane 14 of slice 0, lane 2 of slice 1
    'across, last lanes and first lane': (56, 64),          # (x4, a4)
}


def grids(kind):
    """kind: a shape (nx, nab) or 'tie'."""
    return tie_grids() if kind == 'tie' else grids_of(kind)


# ----------------------------------------------------------------------------- data
def sizes_of(data):
    return list(LARGE_SIZES) if data == 'large' else [NSAMP]


def _draws(data, seed=SEED):
    """(genPos, count, total, neutral count): every draw of the recipe, in its order."""
    if data not in ('small', 'large'):
        raise ValueError(data)
    rng = np.random.default_rng(seed)
    gen = np.cumsum(rng.geometric(0.3, N)) * 2e-6
    for j in POS_TIES:
        gen[j + 1] = gen[j]
    u = rng.random(N)
    v = rng.random(N)
    blk = (np.arange(N) // BLOCK) % len(BLOCK_PARAMS)
    bx = np.array([b[0] for b in BLOCK_PARAMS])[blk]
    ba = np.array([b[1] for b in BLOCK_PARAMS])[blk]
    p = rng.beta(ba, ba / bx - ba)
    m = rng.random(N)
    p = np.where(m < 0.5, 1.0 - p, p)
    ti = rng.integers(0, 3, N)
    ks = rng.binomial(NSAMP, p)
    w = rng.random(N)
    total = np.array(LARGE_SIZES, dtype=np.int64)[ti] if data == 'large' else np.full(N, NSAMP, dtype=np.int64)
    if data == 'large':
        ks = np.floor((ks + w) / (NSAMP + 1) * total).astype(np.int64)      # the same shape at the larger sample size
    kn = np.clip(np.floor(np.exp(v * np.log(total + 1.0))).astype(np.int64), 1, total)
    k = np.clip(np.where(u < SHAPED, ks, kn), 1, total)
    n0 = sizes_of(data)[0]
    for a, b in LOW:
        total[a:b] = n0
        k[a:b] = LOW_K
        kn[a:b] = LOW_K
    return gen, k.astype(np.int64), total, kn.astype(np.int64)


def chromosome(data, seed=SEED):
    """(genPos f64[N], count i64[N], total i64[N]) of data set 'small' or 'large'."""
    return _draws(data, seed)[:3]


def spectrum(data, seed=SEED):
    """({(k, n): g}, props): g tabulated from the NEUTRAL counts of all sites with one pseudo-count per row (k = 1 .. n), props =
    share of the sample size; the stretches' row at LOW_G."""
    gen, k, total, kn = _draws(data, seed)
    sizes = sizes_of(data)
    rows = sum(sizes)
    spect = {(kk, n): 1.0 / (N + rows) for n in sizes for kk in range(1, n + 1)}
    for a, b in zip(kn.tolist(), total.tolist()):
        spect[(a, b)] += 1.0 / (N + rows)
    props = {n: float(np.mean(total == n)) for n in sizes}
    spect[(LOW_K, sizes[0])] = LOW_G
    return spect, props


def tests_of(stride):
    """Site indices of a plan's test sites."""
    if stride == 1:
        return np.arange(DENSE0, DENSE0 + DENSE_M)
    return np.arange(0, N, stride)


def chunks_of(stride, lds=True):
    """(test sites, J, test sites per workgroup, workgroup chunks, chunks of the padded launch, test sites of the last group)."""
    M = len(tests_of(stride))
    J, spb_lds, spb_l2 = SPB[stride]
    spb = spb_lds if lds else spb_l2
    chunks = -(-M // spb)
    return M, J, spb, chunks, -(-chunks // 8) * 8, (M % J if J else 1)


def windows_of(gen, idx, windows):
    """Inclusive index windows (lo i64[], hi i64[]) of the test sites idx: 'all' or 'ragged'."""
    idx = np.asarray(idx, dtype=np.int64)
    M = len(idx)
    if windows == 'all':
        return np.zeros(M, np.int64), np.full(M, N - 1, np.int64)
    if windows != 'ragged':
        raise ValueError(windows)
    rng = np.random.default_rng(SEED + 1 + M)
    r = RAGGED_R
    lo = np.maximum(idx - r, 0)
    hi = np.minimum(idx + r + 1, N - 1)
    lo = np.minimum(lo + rng.integers(0, 2 * r, M), N - 1)          # ragged, sometimes empty, sometimes past the test site
    hi = np.maximum(hi - rng.integers(0, r, M), 0)
    for j in range(M):                                              # never cut between two sites on one position
        while 0 < lo[j] < N and gen[lo[j] - 1] == gen[lo[j]]:
            lo[j] -= 1
        while 0 <= hi[j] < N - 1 and gen[hi[j] + 1] == gen[hi[j]]:
            hi[j] += 1
    return lo.astype(np.int64), hi.astype(np.int64)


def window_of(gen, i, A, lo=0, hi=N - 1):
    """Site indices of test site i's window at A (alpha >= 1e-8, position != the test site's, lo <= index <= hi) and their alpha."""
    al = np.exp(-A * np.abs(gen - gen[i]))
    at = np.arange(len(gen))
    keep = (al >= 1e-8) & (gen != gen[i]) & (at >= lo) & (at <= hi)
    return np.nonzero(keep)[0], al[keep]


# ----------------------------------------------------------------------------- the oracle's tables and sums (the caller brings the oracle)
def row_offsets(data):
    sizes = sizes_of(data)
    return dict(zip(sizes, np.concatenate(([0], np.cumsum([n + 1 for n in sizes])))[:-1].tolist()))


def rows_of(data):
    """Table row of every site: one block of n + 1 rows per sample size, ascending n."""
    gen, k, nn = chromosome(data)
    off = row_offsets(data)
    return (np.array([off[int(n)] for n in nn]) + k).astype(np.int32)


def table_from(psel, data):
    """R[nx][nab][rows] = P_sel prop / g - 1 as util.oracle_R builds it from the oracle's P_sel[nx][nab][rows] (blocks of ascending
    n), 0 on the rows the spectrum does not list (no site carries them)."""
    spect, props = spectrum(data)
    g, pr = [], []
    for n in sizes_of(data):
        for kk in range(n + 1):
            g.append(spect.get((kk, n), np.nan))
            pr.append(props[n])
    with np.errstate(invalid='ignore', divide='ignore'):
        R = psel * np.array(pr) / np.array(g) - 1.0
    return np.where(np.isfinite(R), R, 0.0)


def surface_sums(L, R, As, gen, row, tg, lo, hi):
    """S[t][A][pair] = sum over the window of log1p(alpha R) and ns[t][A], by oracle/bmx_oracle.c orc_surface_sums (L: the loaded
    C oracle).  T = 2 S.  The index windows [lo, hi] are handed over as position ranges: windows_of never cuts between two sites on
    one position, and an empty window (lo > hi) becomes an empty range."""
    import ctypes as C
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.orc_surface_sums.argtypes = [C.c_int, C.c_int, C.c_int, dp, dp, C.c_int, C.c_int64, dp, ip, C.c_int64, dp, dp, dp, dp, ip]
    R = np.ascontiguousarray(R, dtype=np.float64)
    As = np.ascontiguousarray(As, dtype=np.float64)
    gen, row, tg = np.ascontiguousarray(gen, dtype=np.float64), np.ascontiguousarray(row, dtype=np.int32), np.ascontiguousarray(tg, dtype=np.float64)
    lo, hi = np.asarray(lo), np.asarray(hi)
    assert np.all((lo > hi) | (gen[lo] <= gen[hi])) and not np.any((lo > hi) & (gen[lo] == gen[hi]))
    assert np.all((lo == 0) | (gen[np.maximum(lo, 1) - 1] < gen[lo])) and np.all((hi == len(gen) - 1) | (gen[np.minimum(hi, len(gen) - 2) + 1] > gen[hi]))
    gmin, gmax = np.ascontiguousarray(gen[lo]), np.ascontiguousarray(gen[hi])
    S = np.zeros((len(tg), len(As), R.shape[0] * R.shape[1]))
    ns = np.zeros((len(tg), len(As)), np.int32)
    L.orc_surface_sums(R.shape[0], R.shape[1], R.shape[2], R.ctypes.data_as(dp), As.ctypes.data_as(dp), len(As), len(gen), gen.ctypes.data_as(dp),
                       row.ctypes.data_as(ip), len(tg), tg.ctypes.data_as(dp), gmin.ctypes.data_as(dp), gmax.ctypes.data_as(dp), S.ctypes.data_as(dp),
                       ns.ctypes.data_as(ip))
    return S, ns


# A window counts as decided when its best T leads the best T of any other grid point (tie grid: of any other duplicate class),
# and the 'no winner' level T = 0, by more than TIE_BAR of T and by more than ABS_BAR.  ABS_BAR: the kernels compare running
# PRODUCTS, whose spacing near 1 is 2^-52, so a T below ~1e-15 W (W <= 4002 factors, each rounded once: 9e-13 at worst) is not
# distinguishable from 0 or from a neighbour on the device whatever its relative lead; 1e-11 is ten times that.
ABS_BAR = 1e-11


def decide(S, ns, classes=None):
    """From surface_sums: (best T f64[M], its linear index (first maximum; -1: no T > 0), lead over the runner-up and over 0,
    tied bool[M]).  classes: class_of() of a tie grid -- the runner-up is then the best grid point of another class."""
    M = S.shape[0]
    T = 2.0 * S
    T[ns == 0] = -np.inf                                          # the oracle skips an A whose window is empty
    T = T.reshape(M, -1)
    at = np.arange(M)
    lin = np.argmax(T, axis=1)
    best = T[at, lin]
    rest = T.copy()
    if classes is None:
        rest[at, lin] = -np.inf
    else:
        rest[classes[None, :] == classes[lin][:, None]] = -np.inf
    sec = np.maximum(rest.max(axis=1), 0.0)
    has = np.isfinite(best)
    win = has & (best > 0)
    lead = np.where(win, best - sec, np.where(has, -best, np.inf))     # no winner: how far below 0 the best T lies
    tied = has & ~((lead > TIE_BAR * np.abs(best)) & (lead > ABS_BAR))
    return np.where(has, best, 0.0), np.where(win, lin, -1).astype(np.int32), lead, tied
