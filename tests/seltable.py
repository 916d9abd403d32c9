"""Selection-table cases over statistics, minimum counts and sample sizes: the input of tests/test_seltable_cpu.py and
tests/test_gpu_seltable.py.  numpy only; nothing here depends on the library under test, and the functions that need an oracle
take it as an argument (orc: oracle/bmx_oracle.py).

Why.  Every likelihood starts from R[x][alpha_beta][row] = P_sel prop / g - 1.  bb_lut_kernel (K1) builds it on the grid, refine_R
is a second copy of the same arithmetic for every off-grid path.  The scan suites read the table back from the device and hand it
to the oracle, so a wrong table is invisible to them; the reference-made tables (tests/golden/lut_*.npz) stop at 6 excluded counts
and use a flat neutral model (g = 1, prop = 1), under which the last line of K1 is psel - 1 whatever it indexes.

Grid.  XS x ABETAS: 20 pairs, one slice of 64 lanes with 44 pad lanes; alpha_beta = 1e4 and 1e9 run the large-argument lgam
noise, 1e-3 .. 45 the small-argument branches.  One case runs the --findBal grid (BAL_XS x bal_abetas(): 450 pairs, eight slices).

Cases.  CASES lists (statistic, sample sizes, min_count, grid) with what the oracle says of each: nex, the number of counts
excluded from the support (m for B_2 and B_1, 2m - 1 for B_2,MAF, m + 1 for B_0, 2m for B_0,MAF; v1:399-433), the smallest
normalising base 1 - sum(excluded) over pairs and sizes, and how many (size, pair) have a base below WELL = 0.05.  From nex = 8 on
numpy sums the excluded probabilities with eight accumulators and the kernels stream that order; above 128 numpy splits the
array in two and the kernels do not.

Conditioning.  psel = raw / base.  An absolute error e in the excluded sum becomes e / base in psel, so a pair is held to the
plain bar BAR = 1e-12 (that of test_device_selection_table_matches_reference) where base >= WELL, to BAR / base where
TINY = 1e-6 < base < WELL, and only to 'finite where the oracle is finite' at or below TINY: there the reference itself is noise
(B_0,MAF at alpha_beta = 1e-3 has a NEGATIVE base, -3e-10).  tests/test_seltable_cpu.py asserts that every case holds at
least half of its pairs, and at least 10, to the plain bar.

Neutral model (model()).  Per sample size n a seeded positive spectrum g(k, n) = c_n u_k / (k + 1), u uniform in 0.5 .. 1.5, on EVERY
row it lists, with c_n such that the listed rows a site can carry (admissible()) sum to prop(n), as the helper file of a filtered
input does: a site drawn from g is then neutral under the model, R = 0 on average (ratios of at most 3 n within a size: span_hi
stays below 2^60); prop(n) distinct and summing to 1; up to
three rows per size are ABSENT from the spectrum (g = NaN on the device): min(3, rows - 2) of them, none under B_1 (two rows per
size, both carried by sites).  absent_rows() says which.  chromosome() never draws a count whose row is absent.
"""
import numpy as np

SEED = 20261103
XS = (0.05, 0.3, 0.5, 0.95)
ABETAS = (1e-3, 1.0, 45.0, 1e4, 1e9)
# the reference's --findBal grid (hostmodel.Grids(None, None, True, ...)): x and alpha_beta in the reference's list order
BAL_XS = tuple(.05 * i for i in range(1, 11))
WELL = 0.05
TINY = 1e-6
BAR = 1e-12
SMALL = 1e-280          # oracle values below this are compared absolutely against the block's largest value

# (statistic, sizes, min_count, grid) -> (nex, smallest base, (size, pair) below WELL, pairs in all).  The smallest base is what the
# oracle gives on the build host to two digits; None: noise around 0 (|base| < TINY).
CASES = (
    ('B2', (100,), 8, 'short'),
    ('B2', (24, 40, 100), 9, 'short'),
    ('B2maf', (100,), 5, 'short'),
    ('B2maf', (33, 40, 101), 8, 'short'),
    ('B2maf', (100,), 9, 'short'),
    ('B0', (41,), 7, 'short'),
    ('B0', (64, 100), 15, 'short'),
    ('B0maf', (33, 40), 4, 'short'),
    ('B0maf', (100,), 8, 'short'),
    ('B0maf', (101,), 12, 'short'),
    ('B1', (12, 50, 100), 1, 'short'),
    ('B2', (20,), 0, 'short'),
    ('B0', (20,), 0, 'short'),
    ('B2', (1, 2, 3), 1, 'short'),
    ('B2maf', (2, 3), 1, 'short'),
    ('B2', (400,), 1, 'short'),
    ('B2', (33, 34, 143, 171, 172), 1, 'short'),
    ('B2maf', (1001,), 70, 'short'),
    ('B0maf', (400,), 65, 'short'),
    ('B2maf', (40, 50), 5, 'bal'),
)
FACTS = {
    CASES[0]: (8, 0.50, 0, 20), CASES[1]: (9, 0.49, 0, 60), CASES[2]: (9, 0.50, 0, 20), CASES[3]: (15, 0.065, 0, 60),
    CASES[4]: (17, 0.066, 0, 20), CASES[5]: (8, 0.0029, 4, 20), CASES[6]: (16, 0.0029, 8, 40), CASES[7]: (8, 0.0021, 8, 40),
    CASES[8]: (16, 0.0025, 4, 20), CASES[9]: (24, 0.0020, 10, 20), CASES[10]: (1, 0.50, 0, 60), CASES[11]: (0, 1.0, 0, 20),
    CASES[12]: (1, 0.50, 0, 20), CASES[13]: (1, 0.50, 0, 60), CASES[14]: (1, 0.50, 0, 40), CASES[15]: (1, 0.50, 0, 20),
    CASES[16]: (1, 0.50, 0, 100), CASES[17]: (139, 0.0035, 4, 20), CASES[18]: (130, None, 10, 20),
}
REBUILD_CASES = (CASES[3], CASES[8])                                  # the model-rebuild test: three sizes, then one
REFINE_CASES = (CASES[0], CASES[3], CASES[6], CASES[8], CASES[10])    # refine_R through eval_points
E2E_CASES = (CASES[2], CASES[8], CASES[6], CASES[10])                 # scans against a table the device did not make


def case_id(case):
    return '%s-n%s-min%d%s' % (case[0], '.'.join(str(n) for n in case[1]), case[2], '-bal' if case[3] == 'bal' else '')


def bal_abetas():
    """The 45 alpha_beta values of --findBal (hostmodel.Grids.WHOLE_ABETA), restated so that this module imports nothing of the
    library; tests/test_seltable_cpu.py compares the two."""
    return tuple(float(v) for v in list(range(1, 10)) + list(range(5, 100, 5)) + list(range(100, 210, 10)) + [300, 500, 1e3, 1e4, 1e6, 1e9])


def grid_of(case):
    """(x list, alpha_beta list)."""
    if case[3] == 'bal':
        return list(BAL_XS), list(bal_abetas())
    return list(XS), list(ABETAS)


def nex_of(stat, m):
    if stat == 'B2maf':
        return m + max(m - 1, 0)
    if stat == 'B0':
        return m + 1
    if stat == 'B0maf':
        return 2 * m
    return m


def rows_per(stat, n):
    return 2 if stat == 'B1' else n + 1


def row_offsets(case):
    """{n: first row}: one block of rows per sample size, ascending n."""
    stat, sizes = case[0], sorted(case[1])
    off = np.concatenate(([0], np.cumsum([rows_per(stat, n) for n in sizes])))
    return dict(zip(sizes, off[:-1].tolist())), int(off[-1])


def admissible(stat, n, m):
    """Counts a site of sample size n can carry under `stat` with minimum count m (the reference's input filter): B_1 rows
    0 (substitution) and 1 (polymorphism)."""
    if stat == 'B1':
        return [0, 1]
    if stat == 'B2maf':
        return [k for k in range(0, n // 2 + 1) if k == 0 or k >= m]
    if stat == 'B0maf':
        return list(range(m, n // 2 + 1))
    return list(range(m, n if stat == 'B0' else n + 1))


_MODEL = {}


def model(case):
    """(spect {(k, n): g}, props {n: share}, absent {n: [k, ...]}) of a case: see the module docstring."""
    if case not in _MODEL:
        stat, sizes = case[0], sorted(case[1])
        rng = np.random.default_rng(SEED + 101 * CASES.index(case))
        w = 1.0 + rng.random(len(sizes)) + 0.25 * np.arange(len(sizes))
        props = dict(zip(sizes, (w / w.sum()).tolist()))
        spect, absent = {}, {}
        for n in sizes:
            nr = rows_per(stat, n)
            u = (0.5 + rng.random(nr)) / (1.0 + np.arange(nr))
            gone = [] if stat == 'B1' else sorted(rng.choice(nr, min(3, max(nr - 2, 0)), replace=False).tolist())
            keep = np.setdiff1d(np.arange(nr), gone)
            seen = np.intersect1d(keep, admissible(stat, n, case[2]))     # the rows a helper file made from filtered data would list
            u = u * (props[n] / u[seen].sum())
            for k in keep.tolist():
                spect[(k, n)] = float(u[k])
            absent[n] = gone
        _MODEL[case] = (spect, props, absent)
    return _MODEL[case]


def absent_rows(case):
    """Table rows whose neutral probability the spectrum does not list, ascending."""
    off = row_offsets(case)[0]
    return np.array(sorted(off[n] + k for n, ks in model(case)[2].items() for k in ks), dtype=np.int64)


def g_and_prop(case):
    """(g f64[rows] with NaN on the absent rows, prop f64[rows]) as the device's last line indexes them."""
    spect, props, _ = model(case)
    off, rows = row_offsets(case)
    g, pr = np.full(rows, np.nan), np.zeros(rows)
    for n in sorted(case[1]):
        for k in range(rows_per(case[0], n)):
            g[off[n] + k] = spect.get((k, n), np.nan)
            pr[off[n] + k] = props[n]
    return g, pr


# ----------------------------------------------------------------------------- what the oracle says (the caller brings it)
_TABLE, _BASE = {}, {}


def bases(orc, case, xs=None, abetas=None):
    """base[size][ix][ia] = 1 - sum(excluded) by the oracle's norm_base, sizes ascending."""
    key = (case, None if xs is None else (tuple(xs), tuple(abetas)))
    if key not in _BASE:
        gx, ga = grid_of(case) if xs is None else (xs, abetas)
        out = np.zeros((len(case[1]), len(gx), len(ga)))
        for j, n in enumerate(sorted(case[1])):
            excl = orc.excluded_counts(case[0], n, case[2])
            for ix, x in enumerate(gx):
                for ia, a in enumerate(ga):
                    out[j, ix, ia] = orc.norm_base(n, x, a, excl)
        out.setflags(write=False)
        _BASE[key] = out
    return _BASE[key]


def oracle_psel(orc, case):
    """P_sel[nx][nab][rows] by orc.sel_table, one block per sample size (ascending n).  Computed once per case and shared."""
    if case not in _TABLE:
        xs, ab = grid_of(case)
        with np.errstate(all='ignore'):
            t = np.concatenate([orc.sel_table(case[0], n, case[2], xs, ab) for n in sorted(case[1])], axis=2)
        t.setflags(write=False)
        _TABLE[case] = t
    return _TABLE[case]


def psel_tolerance(case, ref, base):
    """(tol f64[nx][nab][rows], judged bool[nx][nab][rows], plain bool[nx][nab][rows]) for a table compared with the oracle's `ref`:
    |difference| <= tol wherever `judged`; elsewhere (base <= TINY) only finiteness is compared.  plain: the entries of the pairs at
    the plain bar (base >= WELL)."""
    stat = case[0]
    off, rows = row_offsets(case)
    tol = np.full(ref.shape, np.inf)
    judged = np.zeros(ref.shape, bool)
    plain = np.zeros(ref.shape, bool)
    for j, n in enumerate(sorted(case[1])):
        sl = slice(off[n], off[n] + rows_per(stat, n))
        blk = np.abs(ref[:, :, sl])
        with np.errstate(all='ignore'):
            rel = np.where(base[j] >= WELL, BAR, BAR / base[j])[:, :, None]
            t = rel * blk
            top = np.max(np.where(np.isfinite(blk), blk, 0.0), axis=2, keepdims=True)
            t = np.where(blk < SMALL, rel * top, t)
            if stat == 'B1':
                # the polymorphism row is (1 - 2 p) / base with p up to 0.5: its error is that of p, not relative to 1 - 2 p
                t[:, :, 1] = rel[:, :, 0]
        ok = np.broadcast_to((base[j] > TINY)[:, :, None], blk.shape)
        tol[:, :, sl] = np.where(ok, t, np.inf)
        judged[:, :, sl] = ok
        plain[:, :, sl] = np.broadcast_to((base[j] >= WELL)[:, :, None], blk.shape)
    return tol, judged, plain


# ----------------------------------------------------------------------------- sites for the off-grid and end-to-end tests
BLOCK = 400
BLOCK_PARAMS = ((0.3, 5.0), (0.25, 1.5), (0.45, 12.0), (0.35, 0.6), (0.4, 8.0), (0.3, 3.0))
SHAPED = (0.7, 0.03, 0.5, 0.1, 0.6, 0.03)      # share of a block's sites drawn from its beta-binomial: stretches of signal between nearly neutral ones
SHAPED_B1 = 0.5                                 # B_1: the same share everywhere (see chromosome())
A_LIST = (150.0, 400.0, 1000.0, 2500.0, 6000.0, 20000.0)     # as test_multiple_sample_sizes_and_large_tables
N_E2E, N_REFINE = 3000, 400
TIE_LIMIT = 0.1                                                # share of a case's windows that may be listed as near-ties
# (the grid values x = 0.05 and 0.95 mirror each other: their table columns are equal to rounding, so every window that either of
# them wins is a near-tie by construction; BLOCK_PARAMS plants x between 0.25 and 0.45, which keeps them to the weak windows)

# refine_R: (A, x, alpha_beta) off the grid, then two exact grid points
OFF_GRID = ((150.0, 0.137, 3.3), (2000.0, 0.137, 2.5e7), (2000.0, 0.5, 3.3), (150.0, 0.5, 2.5e7), (150.0, 0.81, 3.3), (2000.0, 0.81, 2.5e7))
ON_GRID = ((150.0, 0.3, 45.0), (2000.0, 0.95, 1e4))
T_FLOOR = 1e-2          # every reference T of the refine_R test is at least this far from 0 (asserted on the CPU)

_CHROM = {}


def chromosome(case, N, seed=SEED):
    """(genPos f64[N] strictly ascending, count i64[N], total i64[N]).  One np.random.default_rng(seed + 7 N + case index); draws
    in this order: positions cumsum(geometric(1 / 60)) / 1e6; sample sizes by prop; u (shaped where u < SHAPED of the site's block of 400); per sample size
    the neutral counts from g over the admissible, listed counts; p = beta(a, a / x - a) of the site's block of 400, mirrored
    with probability one half; the shaped count binomial(n, p), folded under the MAF statistics, kept where it is admissible and
    listed, the neutral count elsewhere.  B_1: polymorphic with probability 0.9 where shaped, and shaped with probability SHAPED_B1
    everywhere: its table has two rows per size, so away from a strong signal nearly every grid point fits alike and the mirrored
    x values 0.05 / 0.95 tie to rounding -- with the stretches of the other statistics a third of its windows are near-ties."""
    key = (case, N, seed)
    if key in _CHROM:
        return _CHROM[key]
    stat, sizes, m = case[0], sorted(case[1]), case[2]
    spect, props, absent = model(case)
    rng = np.random.default_rng(seed + 7 * N + CASES.index(case))
    gen = np.cumsum(rng.geometric(1 / 60.0, N)) / 1e6
    nn = rng.choice(np.array(sizes, dtype=np.int64), N, p=np.array([props[n] for n in sizes]))
    shaped = rng.random(N) < (SHAPED_B1 if stat == 'B1' else np.array(SHAPED)[(np.arange(N) // BLOCK) % len(BLOCK_PARAMS)])
    kn = np.zeros(N, dtype=np.int64)
    ok = {}
    for n in sizes:
        ks = np.array([k for k in admissible(stat, n, m) if (k, n) in spect], dtype=np.int64)
        assert len(ks) >= 2, (case, n)
        ok[n] = set(ks.tolist())
        p = np.array([spect[(int(k), n)] for k in ks])
        at = nn == n
        kn[at] = rng.choice(ks, int(at.sum()), p=p / p.sum())
    blk = (np.arange(N) // BLOCK) % len(BLOCK_PARAMS)
    bx = np.array([b[0] for b in BLOCK_PARAMS])[blk]
    ba = np.array([b[1] for b in BLOCK_PARAMS])[blk]
    p = rng.beta(ba, ba / bx - ba)
    p = np.where(rng.random(N) < 0.5, 1.0 - p, p)
    ks = rng.binomial(nn, p)
    if stat.endswith('maf'):
        ks = np.minimum(ks, nn - ks)
    if stat == 'B1':
        ks = (rng.random(N) < 0.9).astype(np.int64)
    fine = np.array([int(k) in ok[int(n)] for k, n in zip(ks, nn)])
    k = np.where(shaped & fine, ks, kn).astype(np.int64)
    for a in (gen, k, nn):
        a.setflags(write=False)
    _CHROM[key] = (gen, k, nn)
    return _CHROM[key]


def rows_of(case, k, nn):
    off = row_offsets(case)[0]
    return (np.array([off[int(n)] for n in nn]) + k).astype(np.int32)


def e2e_tests():
    """Site indices of the two runs: dense 1000 .. 1699 and every 37th site."""
    return np.arange(1000, 1700), np.arange(0, N_E2E, 37)


def e2e_grid(orc, case):
    """(x list, alpha_beta list) of the end-to-end scan: the short grid without the alpha_beta values at which any (size, x) has a base
    below WELL -- the ill-conditioned pairs are whole alpha_beta columns (asserted), so what is left is still a product grid."""
    b = bases(orc, case)
    ill = b < WELL
    col = ill.any(axis=(0, 1))
    assert np.array_equal(ill, np.broadcast_to(col, ill.shape)), case
    return list(XS), [a for a, bad in zip(ABETAS, col) if not bad]


def e2e_table(oracle_R, case, xs, abetas):
    """R[nx][nab][rows] by util.oracle_R (the caller brings it) on the end-to-end grid, 0 on the rows the spectrum does not list (no
    site carries them)."""
    key = ('e2e', case)
    if key not in _TABLE:
        spect, props, _ = model(case)
        R = oracle_R(case[0], case[1], case[2], spect, props, xs, abetas)
        R = np.where(np.isfinite(R), R, 0.0)
        R.setflags(write=False)
        _TABLE[key] = R
    return _TABLE[key]


_TIES = {}


def e2e_ties(L, R, case, idx):
    """(tied bool[M], best T f64[M], winner's linear index i32[M], -1: none) of the whole-chromosome windows of the test sites idx
    by the rule of tests/gridshape.py, from the oracle's own surface (L: the loaded C oracle)."""
    import gridshape as gs
    key = (case, len(idx))
    if key not in _TIES:
        gen, k, nn = chromosome(case, N_E2E)
        M = len(idx)
        S, ns = gs.surface_sums(L, R, A_LIST, gen, rows_of(case, k, nn), gen[idx], np.zeros(M, np.int64), np.full(M, N_E2E - 1, np.int64))
        best, lin, lead, tied = gs.decide(S, ns)
        _TIES[key] = (tied, best, lin)
    return _TIES[key]


def table_R(case, psel):
    """R = psel prop / g - 1 as util.oracle_R writes it, from a P_sel[nx][nab][rows]."""
    g, pr = g_and_prop(case)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        return psel * pr / g - 1.0


def refine_tests():
    return np.arange(0, N_REFINE, 8)


def point_T(gen, rows, R_rows, tests, A):
    """T[t] = 2 sum log1p(alpha_i R_i) over the whole-chromosome window of every test site (alpha >= 1e-8, position != the test
    site's: v1:454-457), with R_rows f64[rows] the table of ONE grid point."""
    out = np.zeros(len(tests))
    ns = np.zeros(len(tests), dtype=np.int64)
    for j, t in enumerate(tests):
        al = np.exp(-A * np.abs(gen - gen[t]))
        keep = (al >= 1e-8) & (gen != gen[t])
        ns[j] = int(keep.sum())
        out[j] = 2.0 * np.sum(np.log1p(al[keep] * R_rows[rows[keep]]))
    return out, ns
