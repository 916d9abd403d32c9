"""Block bootstrap of each refined maximum: the definition behind --boot, its summary rules and its writers.

--refine gives a window an off-grid maximum (ballermixplus_amd/refine.py) and --support the range over which the composite
likelihood stays near it (ballermixplus_amd/support.py).  --boot says how far that maximum moves when the data move: every
replicate re-weights the chromosome's sites in blocks and repeats the refinement's search on the re-weighted objective.  The
device (boot_kernel, bmx_ctx_boot, bmx_ctx_eval_points_weighted) implements exactly the rules below; the CPU tests run them
on a host restatement of T.

Weights (a Poisson block bootstrap).  Replicate r of input file f re-weights the sites in blocks of B consecutive sites (site
index i as given to set_sites; block b = i // B; the last block may be short).  Every block draws an independent Poisson(1)
weight from a counter-based hash, on uint64 modulo 2^64:

    K        = replicate_key(S, r, f) = null.replicate_key(null.mix(S ^ SEED_DOMAIN), r, f)
    h(K, b)  = null.mix(K ^ null.mix(b))
    w(K, b)  = #{k in 0..19 : h >= THR[k]},   THR[k] = floor(2^64 * sum_{j <= k} e^-1 / j!)

A weight is a pure function of (K, b): overlapping windows of one replicate see the same resampled chromosome, and host and
device agree exactly (integer comparisons only).  At k = 20 the floor reaches 2^64 - 1, so weights lie in 0..20 and the
probabilities are Poisson(1)'s to within 2^-64 (the mass above 20, 2e-20, sits on 20).  SEED_DOMAIN separates the stream from
the permutation null's: --bootSeed 1 and --nullSeed 1 share nothing.

Objective.  T_w(A, x, alpha_beta) = 2 * sum_i w_i * log1p(alpha_i * R_i) over the sites of refine.py's T (the same window
predicate, the same R) that have w_i > 0; a site of weight 0 contributes nothing, whatever its term.  T_w = -inf when no site
of the set has w_i > 0, or when the sum is not finite.

One replicate of one window.  refine.compass on T_w from the window's refined point: centre, natural values and initial steps
of support.centre (so: the refined point, the grid start's h0), refine.TOL, refine.MAX_ROUNDS, the free coordinates and hull
of refine.Setup.  Kept per (window, replicate): the final natural (A, x, alpha_beta), T_w there, T_w at the centre (the
search's first evaluation) and the rounds run.  A replicate is ok when its final T_w is finite.

Summary of one window over its n_ok ok replicates, per free coordinate, at level L (order statistics, no interpolation: the
rule of null.threshold):
    lo, hi = the ceil((1 - L) / 2 * n_ok)-th (at least the 1st) and the ceil((1 + L) / 2 * n_ok)-th smallest replicate value
    sd     = the sample standard deviation (ddof 1) in the search's coordinate (ln A, x, ln alpha_beta)
    dT_q   = the ceil(L * n_ok)-th smallest of dT = T_w(final) - T_w(centre)   (>= 0: the search never moves downhill)
With n_ok < 2 every statistic is NA (the row keeps its CLR and n_ok).  A fixed coordinate (--fixX, --fixAlpha, a one-value
--listA) has NA ends and an NA sd.  dT_q is the bootstrap analogue of the drop --supportDrop guesses at; it is reported, not
fed back into --support.

What this is.  A bootstrap of a LOCAL search started at the refined point (a replicate whose surface has a higher maximum
elsewhere does not find it); positions, windows and test sites stay fixed; linkage disequilibrium is respected only up to a
block of B sites (B = 1 resamples sites as if they were independent) and demography not at all; percentile ends from R
replicates cannot resolve tails finer than 1 / R.  Windows that were not refined, or whose refined CLR is below --bootMin, are
not bootstrapped.
"""
import math

import numpy as np

from . import null, refine, support

_M64 = (1 << 64) - 1
SEED_DOMAIN = 0xB007B007B007B007      # seed ^ this, mixed: the bootstrap's keys are not the permutation null's
MAX_WEIGHT = 20
# floor(2^64 * Poisson(1).cdf(k)), k = 0..19 (tests/test_boot_cpu.py recomputes them with decimal)
THR = (
    6786177901268885274, 13572355802537770549, 16965444753172213186, 18096474403383694065, 18379231815936564285,
    18435783298447138329, 18445208545532234003, 18446555009401533385, 18446723317385195808, 18446742018272269410,
    18446743888360976771, 18446744058369041076, 18446744072536379768, 18446744073626175052, 18446744073704017573,
    18446744073709207074, 18446744073709531418, 18446744073709550497, 18446744073709551557, 18446744073709551613,
)
LEVEL = 0.95


def value_refusal(R, block=None, level=None, min_clr=None):
    """The message that refuses these values of --boot / --bootBlock / --bootLevel / --bootMin (None: the flag was not given),
    or None."""
    if R < 2:
        return '--boot takes a number of replicates >= 2 (0: off).'
    if block is not None and block < 1:
        return '--bootBlock must be >= 1.'
    if level is not None and not (0.0 < level < 1.0):
        return '--bootLevel takes a number L with 0 < L < 1.'
    if min_clr is not None and min_clr != min_clr:
        return '--bootMin takes a number.'
    return None


def replicate_key(seed, r, f=0):
    """The key of replicate r of input file f (file ordinal 0 for a single file)."""
    return null.replicate_key(null.mix((int(seed) & _M64) ^ SEED_DOMAIN), r, f)


def weight_of_hash(h):
    """w of a hash value (Python int) or of a uint64 array of them."""
    if isinstance(h, np.ndarray):
        h = h.astype(np.uint64, copy=False)
        w = np.zeros(h.shape, dtype=np.int32)
        for t in THR:
            w += h >= np.uint64(t)
        return w
    h = int(h) & _M64
    return sum(1 for t in THR if h >= t)


def block_weights(key, nblocks):
    """w(key, b) of the blocks b = 0 .. nblocks - 1, int32."""
    b = np.arange(int(nblocks), dtype=np.uint64)
    with np.errstate(over='ignore'):
        return weight_of_hash(null.mix(np.uint64(int(key) & _M64) ^ null.mix(b)))


def site_weights(key, N, block=1):
    """The weight of every site 0 .. N - 1 under blocks of `block` consecutive sites, int32."""
    N, B = int(N), int(block)
    if B < 1:
        raise ValueError('block size must be >= 1')
    return block_weights(key, (N + B - 1) // B)[np.arange(N, dtype=np.int64) // B]


def weighted_T(alpha, R, w):
    """T_w from the sites of one window at one point: alpha_i, R_i and w_i of the sites of refine.py's T."""
    w = np.asarray(w)
    on = w > 0
    if not on.any():
        return -math.inf
    with np.errstate(divide='ignore', invalid='ignore'):
        v = float(2.0 * np.sum(w[on] * np.log1p(np.asarray(alpha, dtype=np.float64)[on] * np.asarray(R, dtype=np.float64)[on])))
    return v if math.isfinite(v) else -math.inf


def replicate(Tw_natural, setup, grid_point, refined_point):
    """One replicate of one window on Tw_natural(A, x, abeta) -> T_w, for a window with scan argmax grid_point and refinement
    refined_point: {'A', 'x', 'abeta', 'T', 'T_centre', 'rounds', 'ok'}."""
    c, nat, h0 = support.centre(setup, grid_point, refined_point)
    first = []
    g = refine.coord_objective(Tw_natural, c, nat)

    def f(p):
        T = refine._finite(g(p))
        if not first:
            first.append(T)
        return T
    p, T, rounds, _ = refine.compass(f, c, setup.free, setup.lo, setup.hi, h0)
    A, x, ab = refine.natural_of(p, c, nat)
    return dict(A=A, x=x, abeta=ab, T=T, T_centre=first[0], rounds=rounds, ok=math.isfinite(T))


# ---------------------------------------------------------------------------------------------------------- summary

def _rank(q, n):
    """The order statistic (1-based) of null.threshold at level q among n values."""
    return min(max(math.ceil(round(q * n, 9)), 1), n)


def summarise(A, x, abeta, T, T_centre, free, level=LEVEL):
    """The summary of one window from its replicates (arrays of length R; T_centre may be None: no dT_q):
    {'lo', 'hi', 'sd': 3 floats in the order A, x, alpha_beta (NaN: NA), 'dT_q', 'n_ok'}."""
    T = np.asarray(T, dtype=np.float64)
    ok = np.isfinite(T)
    n = int(ok.sum())
    out = dict(lo=[math.nan] * 3, hi=[math.nan] * 3, sd=[math.nan] * 3, dT_q=math.nan, n_ok=n)
    if n < 2:
        return out
    for k, v in enumerate((A, x, abeta)):
        if not free[k]:
            continue
        v = np.sort(np.asarray(v, dtype=np.float64)[ok])
        out['lo'][k] = float(v[_rank((1.0 - level) / 2.0, n) - 1])
        out['hi'][k] = float(v[_rank((1.0 + level) / 2.0, n) - 1])
        out['sd'][k] = float(np.std(v if k == 1 else np.log(v), ddof=1))
    if T_centre is not None:
        dT = np.sort(T[ok] - np.asarray(T_centre, dtype=np.float64)[ok])
        out['dT_q'] = float(dT[_rank(level, n) - 1])
    return out


# ---------------------------------------------------------------------------------------------------------- output

HEADER = 'physPos\tgenPos\tCLR\tx_lo\tx_hi\ts_lo\ts_hi\tA_lo\tA_hi\tx_sd\tlns_sd\tlnA_sd\tdT_q\tn_ok\n'
REPS_HEADER = 'physPos\tgenPos\treplicate\tT\tx_hat\ts_hat\tA_hat\trounds\n'
ORDER = (1, 2, 0)                 # column order of the coordinates: x, s (alpha_beta), A


def output_name(outfile):
    return outfile + '.boot.txt'


def reps_name(outfile):
    return outfile + '.boot.reps.txt'


def _fmt(v):
    return 'NA' if v != v else repr(float(v))


def format_row(head, clr, s):
    """One line of <out>.boot.txt: head = (physPos, genPos), s = summarise()'s dict."""
    vals = [repr(float(clr))]
    for k in ORDER:
        vals += [_fmt(s['lo'][k]), _fmt(s['hi'][k])]
    vals += [_fmt(s['sd'][k]) for k in ORDER]
    vals += [_fmt(s['dT_q']), repr(int(s['n_ok']))]
    return '\t'.join(list(head) + vals) + '\n'


def na_row(head):
    return '\t'.join(list(head) + ['NA'] * 12) + '\n'


def _positions(ts, main_path):
    with open(main_path) as f:
        lines = f.readlines()
    order = ts.order if ts.na_rows else None
    return lines, (lambda j: 1 + (order[j] if order is not None else j))


def write_boot(path, main_path, ts, refined_clr, res, free, level=LEVEL):
    """<out>.boot.txt: one line per line of the main output, in its order.  The main output's NA rows, and test sites that were
    not bootstrapped, are all-NA rows.  res: fetch_boot()'s dict (None: nothing was bootstrapped)."""
    lines, pos_of = _positions(ts, main_path)
    out = [HEADER] + [na_row(l.rstrip('\n').split('\t')[:2]) for l in lines[1:]]
    for q, j in enumerate(res['window'].tolist() if res is not None else []):
        pos = pos_of(j)
        head = lines[pos].rstrip('\n').split('\t')[:2]
        s = summarise(res['A'][q], res['x'][q], res['abeta'][q], res['T'][q], res['T_centre'][q], free, level)
        out[pos] = format_row(head, refined_clr[j], s)
    with open(path, 'w') as f:
        f.writelines(out)


def write_reps(path, main_path, ts, res):
    """<out>.boot.reps.txt: every replicate of every bootstrapped window, window-major in the order of the test sites."""
    lines, pos_of = _positions(ts, main_path)
    with open(path, 'w') as f:
        f.write(REPS_HEADER)
        for q, j in enumerate(res['window'].tolist() if res is not None else []):
            head = lines[pos_of(j)].rstrip('\n').split('\t')[:2]
            for r in range(res['T'].shape[1]):
                f.write('\t'.join(head + [str(r), repr(float(res['T'][q, r])), repr(float(res['x'][q, r])),
                                          repr(float(res['abeta'][q, r])), repr(float(res['A'][q, r])),
                                          repr(int(res['rounds'][q, r]))]) + '\n')


def read_reps(path):
    """{(physPos, genPos) as printed: {'A', 'x', 'abeta', 'T': f64[R], 'rounds': i32[R]}} of a <out>.boot.reps.txt."""
    rows = {}
    with open(path) as f:
        assert f.readline() == REPS_HEADER
        for l in f:
            c = l.rstrip('\n').split('\t')
            rows.setdefault((c[0], c[1]), []).append(c[2:])
    out = {}
    for head, v in rows.items():
        assert [int(c[0]) for c in v] == list(range(len(v)))
        out[head] = dict(T=np.array([float(c[1]) for c in v]), x=np.array([float(c[2]) for c in v]),
                         abeta=np.array([float(c[3]) for c in v]), A=np.array([float(c[4]) for c in v]),
                         rounds=np.array([int(c[5]) for c in v], dtype=np.int32))
    return out


def free_of(ctx):
    """The free coordinates (A, x, alpha_beta) of ctx's model and A grid: refine.Setup's rule."""
    return refine.Setup(ctx.As, ctx.model.x, ctx.model.abeta).free


def boot_and_write(ctx, outfile, ts, R, seed, block, level, min_clr, f=0, reps=False):
    """After refine_and_write() of one file (input-file ordinal f) on ctx's selected slot: its bootstrap into
    <outfile>.boot.txt and, with reps, <outfile>.boot.reps.txt."""
    if len(ts) == 0:
        write_boot(output_name(outfile), outfile, ts, [], None, (False,) * 3, level)
        if reps:
            write_reps(reps_name(outfile), outfile, ts, None)
        return
    ctx.boot([replicate_key(seed, r, f) for r in range(R)], block, min_clr)
    res = ctx.fetch_boot()
    write_boot(output_name(outfile), outfile, ts, ctx.fetch_refined()['clr'], res, free_of(ctx), level)
    if reps:
        write_reps(reps_name(outfile), outfile, ts, res)
