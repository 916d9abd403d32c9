"""Cases of tests/test_gpu_stream_scalars.py and of tests/golden/gen_stream_scalars.py: the smallest shapes at which the values
the preparation kernel hands to the prepared scan kernels as per-zone scalars (F_j of both zones, G_k / H_k of the triangle,
the triangle flag, the list budgets) can go wrong.  numpy only, apart from run(), which takes the engine from its caller.

Data.  N = 4000 sites, one np.random.default_rng(SEED + number of sample sizes), all draws always:
  genPos = cumsum(geometric(0.3)) * 2e-6 (6.7e-6 per site: +-1370 sites at A = 2000, +-18 at 150000); the sites TIE0 .. TIE0 + 39
  share ONE position (more than two whole groups of 16: t_j = t_0 = t_L there, every F_j = 1, and no triangle);
  sample size drawn from the data set's list; half of the sites carry a neutral count floor((n + 1)^v), half a binomial(n, p) with
  p from a beta of the block of 400 sites it lies in (folded at random), all clipped to 1 .. n;
  spectrum tabulated from the neutral draw of every site plus one pseudo-count per row, props = share of the sample size.
Data set 'one': n = 20 (21 rows: table in LDS).  Data set 'eleven': n = 40 .. 50 (506 rows: 259 KB per slice, read from L2).
Grid: 5 x values, 13 alpha_beta values: 65 pairs, two slices, one real lane in the second.
"""
import numpy as np

SEED = 20261020
N = 4000
TIE0, TIE_LEN = 1000, 40
SIZES = {'one': (20,), 'eleven': tuple(range(40, 51))}
BLOCK_PARAMS = ((0.3, 5.0), (0.12, 1.5), (0.45, 12.0), (0.2, 0.6), (0.38, 8.0), (0.08, 3.0))
XS = [float(v) for v in np.linspace(0.05, 0.5, 5)]
ABETAS = [float(v) for v in np.logspace(-3, 9, 13)]
A_LISTS = {'std': (2000.0, 5000.0, 30000.0, 150000.0), 'big': (100.0, 1e6, 1e8, 30000.0), 'single': (5000.0,), 'single 30000': (30000.0,), 'single 150000': (150000.0,)}
SPB = 64        # test sites per workgroup of the 16-site form below 65536 test sites

PREP = 'clr_scan_prepared_kernel<%d,%s>'
# name -> (data set, A list, test-site indices, windows, variant, profiles, kernel the plan must name)
CASES = {}


def _case(name, data, a, idx, windows='all', variant=0, profiles=0, kernel=None):
    CASES[name] = dict(data=data, a=a, idx=np.asarray(idx, dtype=np.int64), windows=windows, variant=variant, profiles=profiles, kernel=kernel)


# short last group, nvalid < J; every SNP a test site: the triangle form
_case('M=1', 'one', 'std', range(2000, 2001))        # (one test site has no gap to its neighbour: whatever plan the library picks)
for _m in (15, 16, 17, 2 * SPB + 3):
    _case('M=%d' % _m, 'one', 'std', range(2000, 2000 + _m), kernel=PREP % (16, 'true'))
_case('dense, chromosome start', 'one', 'std', range(0, 40), kernel=PREP % (16, 'true'))
_case('dense, chromosome end', 'one', 'std', range(N - 37, N), kernel=PREP % (16, 'true'))
# generic middle
_case('every 2nd', 'one', 'std', range(1401, 2001, 2), kernel=PREP % (16, 'true'))
_case('every 3rd', 'one', 'std', range(1400, 2000, 3), kernel=PREP % (16, 'true'))
_case('every 4th, J = 8', 'one', 'std', range(1402, 2602, 4), kernel=PREP % (8, 'true'))
_case('every 4th, J = 4', 'one', 'std', range(1402, 2602, 4), variant=15, kernel=PREP % (4, 'true'))
# t_j = t_0 = t_L
_case('tied run', 'one', 'std', range(TIE0 - 8, TIE0 + TIE_LEN + 8), kernel=PREP % (16, 'true'))
# F_j underflows to 0 next to A = 100; one A
_case('A to 1e8', 'one', 'big', range(2000, 2131), kernel=PREP % (16, 'true'))
_case('A to 1e8, every 3rd', 'one', 'big', range(1400, 2000, 3), kernel=PREP % (16, 'true'))
_case('single A', 'one', 'single', range(2000, 2131), kernel=PREP % (16, 'true'))
_case('single A = 30000', 'one', 'single 30000', range(2000, 2131), kernel=PREP % (16, 'true'))
_case('single A = 150000, every 2nd', 'one', 'single 150000', range(1401, 2001, 2), kernel=PREP % (16, 'true'))
# table in L2
_case('eleven sizes', 'eleven', 'std', range(2000, 2131), kernel=PREP % (16, 'false'))
_case('eleven sizes, every 2nd', 'eleven', 'std', range(1401, 2001, 2), kernel=PREP % (16, 'false'))
_case('eleven sizes, every 4th', 'eleven', 'std', range(1402, 2602, 4), kernel=PREP % (8, 'false'))
# explicit windows that cut inside a group
_case('cut windows', 'one', 'std', range(2000, 2131), windows='cut', kernel=PREP % (16, 'true'))
_case('cut windows, every 2nd', 'one', 'std', range(1401, 2001, 2), windows='cut', kernel=PREP % (16, 'true'))
_case('cut windows, every 4th', 'one', 'std', range(1402, 2602, 4), windows='cut', kernel=PREP % (8, 'true'))
# profiles on
_case('profiles', 'one', 'std', range(2000, 2131), profiles=7, kernel=PREP % (16, 'true'))
_case('profiles, every 4th', 'one', 'std', range(1402, 2602, 4), profiles=7, kernel=PREP % (8, 'true'))
_case('profiles, eleven sizes', 'eleven', 'std', range(1401, 2001, 2), profiles=7, kernel=PREP % (16, 'false'))

# a scan of several launch ranges: 2^18 sites of the library's own synthetic chromosome, every site a test site, profiles on
RANGES_N = 1 << 18
RANGES_SAMPLE = 4096      # records kept: around every launch cut, both ends, a spread; plus a digest of all records


def draws(data):
    """(genPos f64[N], count i64[N], total i64[N], neutral count i64[N])."""
    sizes = np.array(SIZES[data], dtype=np.int64)
    rng = np.random.default_rng(SEED + len(sizes))
    gen = np.cumsum(rng.geometric(0.3, N)) * 2e-6
    gen[TIE0:TIE0 + TIE_LEN] = gen[TIE0]
    total = sizes[rng.integers(0, len(sizes), N)]
    u, v = rng.random(N), rng.random(N)
    blk = (np.arange(N) // 400) % len(BLOCK_PARAMS)
    bx = np.array([b[0] for b in BLOCK_PARAMS])[blk]
    ba = np.array([b[1] for b in BLOCK_PARAMS])[blk]
    p = rng.beta(ba, ba / bx - ba)
    p = np.where(rng.random(N) < 0.5, 1.0 - p, p)
    ks = rng.binomial(total, p)
    kn = np.clip(np.floor(np.exp(v * np.log(total + 1.0))).astype(np.int64), 1, total)
    k = np.clip(np.where(u < 0.5, ks, kn), 1, total)
    return gen, k.astype(np.int64), total, kn


def spectrum(data):
    gen, k, total, kn = draws(data)
    sizes = SIZES[data]
    rows = sum(sizes)
    spect = {(kk, n): 1.0 / (N + rows) for n in sizes for kk in range(1, n + 1)}
    for a, b in zip(kn.tolist(), total.tolist()):
        spect[(a, b)] += 1.0 / (N + rows)
    return spect, {n: float(np.mean(total == n)) for n in sizes}


def windows_of(idx, windows):
    """Inclusive index windows: None, None ('all': no bounds) or bounds that differ from test site to test site, so that the
    largest start and the smallest end of a group cut through its zones (every 29th window empty)."""
    if windows == 'all':
        return None, None
    j = np.arange(len(idx))
    lo = np.maximum(idx - 300 + 37 * (j % 7), 0)
    hi = np.minimum(idx + 250 - 41 * (j % 5), N - 1)
    lo = np.where(j % 29 == 28, hi + 1, lo)
    return lo.astype(np.int64), hi.astype(np.int64)


def open_data(eng, data, a):
    """(context with the data set's model and sites, genPos, rows, the device's own table with 0 where it is not finite)."""
    gen, k, total, _ = draws(data)
    spect, props = spectrum(data)
    model = eng.ModelArrays('B2', 1, list(SIZES[data]), spect, props, XS, ABETAS)
    rows = model.rows_of(k, total)
    ctx = eng.Context(0)
    ctx.set_model(model, list(A_LISTS[a]))
    ctx.set_sites(gen, rows)
    R = ctx.fetch_lut()[1]
    assert np.isfinite(R[:, :, np.unique(rows)]).all()
    return ctx, gen, rows, np.where(np.isfinite(R), R, 0.0)


def run(ctx, gen, case):
    """Scan one case on a context of its data set: (records, plan, {profile name: array} or None)."""
    c = CASES[case]
    ctx.set_variant(c['variant'])
    ctx.set_profiles(c['profiles'])
    lo, hi = windows_of(c['idx'], c['windows'])
    ctx.set_tests(gen[c['idx']], lo, hi)
    ctx.scan()
    rec = ctx.fetch_records().copy()
    prof = {k: ctx.fetch_profile(k).copy() for k in ('A', 'x', 'abeta')} if c['profiles'] else None
    return rec, ctx.plan(), prof


def ranges_ctx(eng):
    """The context of the launch-range case (profiles on) and its positions."""
    from ballermixplus_amd import synth
    from ballermixplus_amd.hostmodel import Grids
    phys, gen, k, nn = synth.synth_chromosome(RANGES_N, 100, 3)
    spect = {(a, b): f for a, b, f in synth.spect_from_counts(k, nn)}
    xs, ab, As = Grids(None, None, False, False, None, None).scan_order()
    model = eng.ModelArrays('B2', int(k.min()), [100], spect, {100: 1.0}, xs, ab)
    ctx = eng.Context(0)
    ctx.set_model(model, As)
    rows = model.rows_of(k, nn)
    ctx.set_sites(gen, rows)
    ctx.set_profiles(7)
    ctx.set_tests(gen)
    return ctx, gen, rows, As


def ranges_sample(cuts, M):
    """Indices of the records kept of the launch-range case: 96 on either side of every cut, the first and last 128, a spread."""
    parts = [np.arange(0, 128), np.arange(M - 128, M)]
    for c in cuts:
        parts.append(np.arange(max(int(c) - 96, 0), min(int(c) + 96, M)))
    at = np.unique(np.concatenate(parts))
    rest = np.setdiff1d(np.linspace(0, M - 1, RANGES_SAMPLE).astype(np.int64), at)
    return np.unique(np.concatenate([at, rest[:max(RANGES_SAMPLE - len(at), 0)]]))


# ----------------------------------------------------------------------------- the oracle's side
def oracle(c_scan, L, R, gen, rows, case):
    """(clr, ix, ia, iA, ns) of the C oracle on table R, and the windows it leaves undecided: those whose runner-up at another
    grid point (or the level T = 0) trails by no more than 1e-7 of T (gridshape.decide, the bar of tests/test_gpu_grid_shapes.py)."""
    import gridshape as gs
    c = CASES[case]
    idx = c['idx']
    lo, hi = windows_of(idx, c['windows'])
    if lo is None:
        lo, hi = np.zeros(len(idx), np.int64), np.full(len(idx), N - 1, np.int64)
    As = A_LISTS[c['a']]
    ref = c_scan(L, R, As, gen, rows, gen[idx], lo, hi)
    lo2 = np.minimum(lo, N - 1)         # (an empty window lo = hi + 1 stays empty)
    S, ns = gs.surface_sums(L, R, As, gen, rows, gen[idx], lo2, hi)
    tied = gs.decide(S, ns)[3]
    return ref, np.nonzero(tied)[0]


def check_oracle(rec, orc, what):
    """The project's bar: every CLR finite and allclose(rtol 1e-9, atol 1e-12); (x, alpha_beta, A) and nSites equal on every window
    the oracle decides; no winner -> clr == 0, lin == -1, nsites == 0."""
    (clr, ix, ia, iA, ns), tied = orc
    nx, nab = len(XS), len(ABETAS)
    lin = np.where(iA >= 0, (iA * nx + ix) * nab + ia, -1)
    keep = np.ones(len(clr), bool)
    keep[tied] = False
    worst = float(np.max(np.abs(rec['clr'] - clr) / np.maximum(np.abs(clr), 1e-300)))
    print('%s: %d windows, %d undecided, %d without a winner, nSites %d .. %d, worst relative dCLR %.3e'
          % (what, len(clr), len(tied), int((lin < 0).sum()), ns.min(), ns.max(), worst))
    assert np.isfinite(rec['clr']).all(), what
    assert len(tied) <= max(0.02 * len(clr), 1), (what, tied)
    assert np.array_equal(rec['lin'][keep], lin[keep]), (what, np.nonzero(rec['lin'] != lin)[0][:8])
    assert np.array_equal(rec['nsites'][keep], ns[keep]), (what, np.nonzero(rec['nsites'] != ns)[0][:8])
    assert np.allclose(rec['clr'], clr, rtol=1e-9, atol=1e-12), (what, worst)
    z = (lin < 0) & keep
    assert np.all(rec['clr'][z] == 0.0) and np.all(rec['nsites'][z] == 0), what
