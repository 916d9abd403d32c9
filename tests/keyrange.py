"""Cases at the ends of the scan's best key: the input of tests/test_keyrange_cpu.py and tests/test_gpu_key_range.py.  numpy only;
whatever is taken from a selection table (the largest P_sel of a row over the grid) is handed in by the caller from the oracle's
sel_table, so nothing here depends on the library under test.

Why.  Every scan kernel keeps the best grid point of a window as a key: ec = clamp(E, +-131071) + 131072 of the running product's
binary exponent E, a mantissa, and the A index.  The grouped and prepared kernels pack bestK = (ec << 13) | iA into one int
(iA = 8191 and ec = 131072: nothing beat T = 0; (262143 << 13) | 8191 == INT32_MAX: no spare bit); the solo and per-site kernels keep
ec and iA apart behind the same clamp.  finalize_kernel turns the winning key into the CLR and refuses the slot (BMX_E_LIMIT) where a
winner's ec sits AT the clamp.  Write E* = floor(T_best / (2 ln 2)) for the winner's exponent in the oracle, mantissa in [1, 2).

'high' -- the top of the exponent field.  N = 6000 sites, B_2, the default x / alpha_beta grid (10 x 44), the A list '20' (every site of
the chromosome is in reach: A |d| < 0.9), all draws from ONE np.random.default_rng(SEED) in tests/tablespan.py's order (positions
cumsum(geometric(0.3, N)) 2e-6: no two tied; counts uniform; u; v; ti; w), tablespan's 'common' placement (the extreme row (7, n) on the
sites with u < 0.4 and on every 50th) and its spectrum (log2(1 + max R) = span - 0.5).  Three sets:
  's62'    n = 30, span 62 (the last groupable one): prepared J = 16 / J = 8 at the strides 1 / 5, solo at 20
  's200'   the same sites at span 200: the one-test-site-per-wave kernels at every stride
  'large'  sample sizes (150, 160, 170), extreme row (7, 150), span 62: the <., false> forms that read R from L2
  ('large' carries its extreme row on 60 % of the sites, the other two on 43 %.)
Test sites: RUN = 32 consecutive multiples of the stride around site 3000; ONE K per (set, band), so that all windows of a scan (and
of a group) share a band.  On 's62' site i gets the index window [i - K, i + K] (52.6 bits per step of K).  On 's200' one site of
the extreme row is worth 200 bits and the number of such sites in [i - K, i + K] wanders by +-9 over a stride-20 run -- 3 750 bits,
more than the inside band holds -- so 's200' and 'large' count K in sites of the extreme row: the smallest index window with K of
them on either side of i (counted_windows; numpy on the counts alone).  Bands (conditions on E*, asserted on the oracle alone):
  'rung1' 'rung2' 'rung3'   E* within 600 of 32 768, 65 536, 98 304: ec has bit 15, bit 16, both set
  'inside'                  129 000 <= E* <= 131 060: compared with the oracle
  'outside'                 E* >= 131 080: the scan must be refused
  (between 131 060 and 131 080 nothing is asserted: the [1, 2) and the v_frexp [1/2, 1) mantissa conventions differ by one there)
A window of a band's scan that misses the band is still a window: below 131 060 it is compared like any other, from 131 080 on it
is refused; only the populations counted per band leave it out.
Measured with the committed seed and the oracle's own table (tests/test_keyrange_cpu.py asserts the conditions and prints these):
  s62    K = 607 / 1195 / 1828 / 2441 / 2480: E* 32 346 .. 33 796, 64 583 .. 65 838, 97 329 .. 99 535 (32 / 32 / 25, 32 / 32 / 22 and 32 / 26 / 13 of
         32 windows inside +-600 at the strides 1 / 5 / 20), inside 129 475 .. 130 522, outside 131 502 .. 132 542 (32 of 32 at every stride)
  s200   K = 82 / 164 / 246 / 328 / 329: rungs 32 749 .. 32 785, 65 509 .. 65 539, 98 239 .. 98 281, inside 130 967 .. 131 014, outside 131 365 ..
         131 412; windows of 339 .. 1 516 sites; every window in its band
  large  K = 276 / 549 / 822 / 1093 / 1096: rungs 32 726 .. 32 875, 65 455 .. 65 582, 98 241 .. 98 349, inside 130 843 .. 130 955, outside 131 202 ..
         131 320; windows of 911 .. 3 654 sites; every window in its band
  smallest runner-up margin / T of the compared windows outside TIED: 1.35e-7 ('large', stride 20); C oracle against long double on
  eight inside-band windows per set: 4.3e-15, 1.5e-15, 2.9e-15 relative
  low    E* of the best grid point at A = 1 / 100: -119 578 / -118 503 (K = 3000), -135 520 / -134 154 (3400), -278 978 / -273 660 (7000); 'mixed':
         E* = -32 227 at A = 1 (16 000 sites), T = 3.34 at A = 100 (64 sites)
  wideA  windows won at the five useful indices: 37 / 98 / 36 / 55 / 32 of 600, 342 without a winner, at every nA; 'dup': 32 at index 5, 0 at 8189

'low' -- the bottom.  LOW_N = 16 000 sites:  site 0 at 0.0 and site 1 at 1e-20, both of sample size 7, to which the model gives the
share 0.0 (R = -1 exactly on its rows: tests/sandwichcases.py 'skip');  LOW_BLOCK sites at 1.0 + i 2^-40 of ONE row, (10, 30), whose
neutral probability is set to g = 1e6 max P_sel(10 | 30), so that 1 + R <= 1e-6 at EVERY grid point (with g = 1.0, tablespan's
LOW_G, the oracle's table has 1 + R up to 0.075 and the whole block reaches E* = -5e4 only);  64 sites of ordinary rows at
1.25 + j 1e-3.  A list '1,100'.  Windows [t - K, t + K], K = 3000, 3400, 7000, at RUN test sites per stride around block site 8000: E* on
either side of -131 071 and far below it.  Two more windows stand in every test list, 'zero' in one group with the block's first windows:
  'zero'   test position 0.0, window [0, 1]: site 1 has alpha = exp(-A 1e-20) = 1.0 exactly and R = -1, a factor 0.0 (renorm's sticky
           exponent); T = -inf at every grid point.  (Site 0 sits at the test position and is no site of the window.)
  'mixed'  is LAST: test position 1.2825 in the ordinary stretch, window = the whole chromosome.  A = 1 (first) reaches the block
           with alpha = exp(-0.28): 1 + alpha R = 0.24, T ~ -4.5e4; A = 100 (second) reaches the ordinary stretch alone (the block is
           0.28 away: alpha = 5e-13, cut) and wins with a modest T > 0.  Nothing may stick from one A to the next.
The device must answer CLR = +0.0, lin = -1, nSites = 0 and all-zero profiles on every block and 'zero' window, without an error.
'lowL' is the same chromosome on the sample sizes (7, 150, 160, 170) -- 491 rows, which the <., false> forms read from L2: the block on
row (32, 150), the row of that size whose P_sel varies least over the grid (min / max = 8.9e-12; at its far grid points R rounds to -1
and the factor is 1 - alpha > 0), the 64 ordinary sites on the three sizes in turn.  Same windows, same E* (-119 578 / -135 520 / -278 978
at A = 1); 'mixed': E* = -32 229 at A = 1, T = 0.2476 at A = 100.

'wideA' -- the A-index field.  One grid pair (x 0.3, alpha_beta 10), WIDE_N = 600 sites as test_per_site_kernel_with_more_than_8191_A_
values, nA in 8189 .. 8192; the useful values WIDE_A stand at the indices 0, 4095, 4096, nA - 2, nA - 1, every other index holds
1e9 + 1e3 i (a reach of 1.8e-8: less than the smallest gap of 1e-6, so no site).  (On this chromosome no window is won below
A = 1e4, so the useful values are 2e4 .. 2e5, not 10 .. 2e5, and they stand in no monotone order.)  'dup' (nA = 8190) repeats the value of index
nA - 1 at index 5: the lower index must win.

'both' -- 's62' with nA = 8190 and A = 20 at index 8189 (then at index 0), the rest out of reach: a packed key within 2^13 of INT32_MAX.
"""
import numpy as np

import tablespan as tb

SEED = 20261021
LN2 = float(np.log(2.0))
CLAMP = 131071                      # bmxscan.hip: ec = min(max(E, -131071), 131071) + 131072
SHIFT = 13                          # bestK = (ec << 13) | iA
SENTINEL = 8191                     # iA of "none yet"; can_group: nA < 8191
INSIDE = (129000, 131060)
OUTSIDE = 131080
RUNGS = {'rung1': 32768, 'rung2': 65536, 'rung3': 98304}
RUNG_HALF = 600
BANDS = ('rung1', 'rung2', 'rung3', 'inside', 'outside')
TIE_BAR = 1e-7

N = 6000
NSAMP = 30
CENTRE = 3000
RUN = 32
STRIDES = (1, 5, 20)
A_HIGH = '20'
SETS = {'s62': 62, 's200': 200, 'large': 62}        # set -> span
# (set, band) -> K.  Measured with the oracle's table (tests/test_keyrange_cpu.py prints E* per scan and asserts the bands)
K_OF = {('s62', 'rung1'): 607, ('s62', 'rung2'): 1195, ('s62', 'rung3'): 1828, ('s62', 'inside'): 2441, ('s62', 'outside'): 2480,
        ('s200', 'rung1'): 82, ('s200', 'rung2'): 164, ('s200', 'rung3'): 246, ('s200', 'inside'): 328, ('s200', 'outside'): 329,
        ('large', 'rung1'): 276, ('large', 'rung2'): 549, ('large', 'rung3'): 822, ('large', 'inside'): 1093, ('large', 'outside'): 1096}
# (set, band, stride) -> indices INTO tests_of(stride) of the windows whose winner leads the runner-up by 1e-7 T or less: skipped by
# the GPU comparison (test_keyrange_cpu.py asserts that the list is complete and holds at most 2 % of a case's windows)
TIED = {('s62', 'rung1', 1): (21,), ('s62', 'rung1', 5): (17, 22),
        ('s200', 'rung3', 1): (30,), ('s200', 'inside', 1): (19,), ('s200', 'inside', 5): (2, 3), ('s200', 'rung1', 20): (31,)}
LARGE_SHARE = 0.6                   # 'large': the extreme row on 60 % of the sites

LOW_N = 16000
LOW_BLOCK = LOW_N - 2 - 64
LOW_K = tb.LOW_K
LOW_SIZES = (7, NSAMP)
LOWL_K = 32                         # 'lowL': (32, 150), the row of size 150 whose P_sel varies least over the grid (min / max = 8.9e-12)
LOW_FACTOR = 1e-6                   # 1 + R <= LOW_FACTOR on row (LOW_K, 30)
LOW_A = '1,100'
LOW_CENTRE = 8000
LOW_KS = (3000, 3400, 7000)
LOW_STEP = 2.0 ** -40
MIXED_POS = 1.2825

WIDE_N = 600
WIDE_NA = (8189, 8190, 8191, 8192)
WIDE_A = (6e4, 2e5, 2e4, 1e5, 4e4)    # at the indices wide_useful(nA), in that order


def e_star(T):
    """floor(T / (2 ln 2)): the binary exponent of exp(T / 2) with its mantissa in [1, 2)."""
    return np.floor(np.asarray(T, dtype=np.float64) / (2.0 * LN2)).astype(np.int64)


def band_of(E):
    """Per E*: 'inside', 'outside', a rung's name, 'between' (131 060 < E* < 131 080: nothing asserted) or 'other' (in range)."""
    out = []
    for e in np.asarray(E).tolist():
        name = 'outside' if e >= OUTSIDE else 'between' if e > INSIDE[1] else 'inside' if e >= INSIDE[0] else 'other'
        for r, mid in RUNGS.items():
            if abs(e - mid) <= RUNG_HALF:
                name = r
        out.append(name)
    return out


def tests_of(stride, centre=CENTRE, run=RUN):
    return centre + stride * (np.arange(run) - run // 2)


def windows_of(idx, K, n=N):
    idx = np.asarray(idx, dtype=np.int64)
    assert idx.min() - K >= 0 and idx.max() + K <= n - 1           # no window is cut off at an end of the chromosome
    return idx - K, idx + K


def counted_windows(is_ext, idx, C):
    """The smallest index window around each site of idx with C sites of the extreme row on either side of it."""
    at = np.nonzero(is_ext)[0]
    left = np.searchsorted(at, idx, side='left')           # extreme-row sites before idx
    right = np.searchsorted(at, idx, side='right')
    assert left.min() >= C and right.max() + C <= len(at)
    return at[left - C].astype(np.int64), at[right + C - 1].astype(np.int64)


def high_windows(name, band, idx, count=None):
    """(lo, hi) of the test sites idx in the scan of `band` on set `name`: [i - K, i + K], or on 's200' K extreme-row sites on either
    side (count: the set's counts)."""
    K = K_OF[(name, band)]
    if name in ('s200', 'large'):
        return counted_windows(np.asarray(count) == tb.EXT_K, np.asarray(idx), K)
    return windows_of(idx, K)


# ---------------------------------------------------------------------------------------------------------------- high
def sizes_of(name):
    return list(tb.LARGE_SIZES) if name == 'large' else [NSAMP]


def ext_row(name):
    return (tb.EXT_K, tb.LARGE_SIZES[0] if name == 'large' else NSAMP)


def chromosome(name, seed=SEED):
    """(genPos f64[N], count i64[N], total i64[N]) of set `name`: tablespan's draws and its 'common' placement at N = 6000."""
    rng = np.random.default_rng(seed)
    gen = np.cumsum(rng.geometric(0.3, N)) * 2e-6
    k = rng.integers(1, NSAMP + 1, N)
    u = rng.random(N)
    rng.random(N)
    ti = rng.integers(0, 3, N)
    w = rng.random(N)
    total = np.full(N, NSAMP, dtype=np.int64)
    if name == 'large':
        total = np.array(tb.LARGE_SIZES, dtype=np.int64)[ti]
        k = 1 + np.floor(w * total).astype(np.int64)
        total[u < LARGE_SHARE] = tb.LARGE_SIZES[0]
        total[::50] = tb.LARGE_SIZES[0]
    k[u < (LARGE_SHARE if name == 'large' else 0.4)] = tb.EXT_K
    k[::50] = tb.EXT_K
    return gen, k.astype(np.int64), total


def spectrum(name, sel_max, count, total):
    """({(k, n): g}, props) with the extreme row placed at the set's span: tablespan.spectrum's rule."""
    cnt = {}
    for a, b in zip(count.tolist(), total.tolist()):
        cnt[(a, b)] = cnt.get((a, b), 0) + 1
    spect = {key: c / len(count) for key, c in cnt.items()}
    props = {n: float(np.mean(total == n)) for n in sizes_of(name)}
    e = ext_row(name)
    spect[e] = float(sel_max) * props[e[1]] / 2.0 ** (SETS[name] - tb.MARGIN)
    return spect, props


# ----------------------------------------------------------------------------------------------------------------- low
def low_sizes(name='low'):
    """Sample sizes of 'low' (7, 30) and of 'lowL' (7, 150, 160, 170: 491 rows, read from L2)."""
    return (7,) + tuple(tb.LARGE_SIZES) if name == 'lowL' else LOW_SIZES


def low_row(name='low'):
    """(k, n) of the block's row."""
    return (LOWL_K, tb.LARGE_SIZES[0]) if name == 'lowL' else (LOW_K, NSAMP)


def low_chromosome(name='low', seed=SEED):
    """(genPos, count, total) of the 'low' case, or of 'lowL': the same positions on the large sample sizes."""
    rng = np.random.default_rng(seed + 1)
    gen = np.concatenate(([0.0, 1e-20], 1.0 + LOW_STEP * np.arange(LOW_BLOCK), 1.25 + 1e-3 * np.arange(64)))
    block_k, block_n = low_row(name)
    if name == 'lowL':
        last_n = np.array(tb.LARGE_SIZES, dtype=np.int64)[np.arange(64) % 3]
        last_k = 1 + np.floor(rng.random(64) * last_n).astype(np.int64)
    else:
        last_n = np.full(64, NSAMP, dtype=np.int64)
        last_k = rng.integers(1, NSAMP + 1, 64)
    k = np.concatenate(([2, 3], np.full(LOW_BLOCK, block_k), last_k)).astype(np.int64)
    total = np.concatenate(([7, 7], np.full(LOW_BLOCK, block_n), last_n)).astype(np.int64)
    k[2 + LOW_BLOCK:][k[2 + LOW_BLOCK:] == block_k] = block_k + 1        # the block's row stays the block's
    return gen, k, total


def low_spectrum(sel_max_low, count, total, name='low'):
    """Ordinary rows: uniform neutral probabilities prop(n) / (n + 1) (their R = (n + 1) P_sel - 1 is the signal 'mixed' finds); the
    block's row low_row(name) = (k, n): g = prop(n) sel_max_low / LOW_FACTOR; size 7: share 0.0, the other sizes equal shares."""
    sizes = low_sizes(name)[1:]
    props = {7: 0.0}
    props.update({n: 1.0 / len(sizes) for n in sizes})
    spect = {(kk, n): props[n] / (n + 1) for n in sizes for kk in range(n + 1)}
    spect.update({(kk, 7): 1.0 / 8 for kk in range(8)})
    spect[low_row(name)] = float(sel_max_low) * props[sizes[0]] / LOW_FACTOR
    return spect, props


def low_tests(stride, K):
    """(test positions, lo, hi, kinds) of one 'low' or 'lowL' scan: 'zero', RUN block windows at `stride` with half-width K, 'mixed'."""
    gen = low_chromosome()[0]
    idx = 2 + tests_of(stride, LOW_CENTRE)
    lo, hi = idx - K, idx + K
    assert lo.min() >= 2 and hi.max() < 2 + LOW_BLOCK
    tg = np.concatenate(([0.0], gen[idx], [MIXED_POS]))
    lo = np.concatenate(([0], lo, [0])).astype(np.int64)
    hi = np.concatenate(([1], hi, [LOW_N - 1])).astype(np.int64)
    return tg, lo, hi, ['zero'] + ['block'] * len(idx) + ['mixed']


# --------------------------------------------------------------------------------------------------------------- wideA
def wide_chromosome():
    rng = np.random.default_rng(5)
    n = 50
    gen = np.cumsum(rng.geometric(0.2, WIDE_N)).astype(np.float64) * 1e-6
    k = rng.integers(1, n + 1, WIDE_N)
    return gen, k.astype(np.int64), np.full(WIDE_N, n, dtype=np.int64)


def wide_useful(nA):
    return (0, 4095, 4096, nA - 2, nA - 1)


def wide_grid(nA, dup=False, values=WIDE_A):
    """The A list of nA values: `values` at wide_useful(nA), 1e9 + 1e3 i elsewhere; dup: index 5 repeats the value of index nA - 1."""
    As = 1e9 + 1e3 * np.arange(nA, dtype=np.float64)
    As[list(wide_useful(nA))] = values
    if dup:
        As[5] = As[nA - 1]
    return As


def both_grid(at):
    As = 1e9 + 1e3 * np.arange(8190, dtype=np.float64)
    As[at] = float(A_HIGH)
    return As
