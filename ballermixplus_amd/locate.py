"""Block-bootstrap position interval per peak: the definition behind --locate, its host restatements and its writers.

--peaks turns the CLR track into loci, --refine / --support / --boot say how high each maximum is and how well (x, alpha_beta,
A) are determined.  None of them says WHERE the selected site is: a peak's extent describes the shape of the track, and the
bootstrap of --boot keeps the test position fixed.  --locate gives every apex an interval of test positions: each replicate
resamples the chromosome's sites in blocks, repeats the whole grid scan around every apex, and records where the maximum of the
resampled track falls.

Why a replicate is an ordinary scan.  The weights are --boot's: an exact, host-reproducible Poisson(1) block weight per site
(boot.site_weights), integers 0..20.  An integer-weighted composite likelihood is the plain composite likelihood of a resampled
site array: repeat site i w_i times, at the same position and with the same table row, and T on that array is exactly boot.py's
T_w = 2 * sum_i w_i log1p(alpha_i R_i).  The scan kernels already handle runs of sites at one position, test positions that
are not sites, and exclude every site at the test position, so a replicate of the grid scan -- a GLOBAL argmax over (A, x,
alpha_beta) per test position, not boot.py's local search -- is one run of the unchanged scan kernels on the resampled array.
The device builds that array (bmx_ctx_resample_sites) and reduces each replicate's track to one argmax per peak
(bmx_ctx_locate_accumulate); resampled() and argmax_rows() below restate both on the host, exactly.

Track.  As in peaks.py: the rows of the main output that have a test position (its NA rows are not part of it), t = 0 .. M-1,
with the test position g_t the scan used.  K = the apexes of the peak call that are kept: all of them, or with --locateMin C
those with CLR >= C.

Search range of a peak.  The track rows s with g_a - g_s <= H and g_s - g_a <= H, a the apex's row (peaks.py's radius
predicate: these two subtractions, no other arithmetic); H = --locateSpan, default G (--peaks' separation).  Ranges of
neighbouring peaks may overlap.  The replicate test set is the sorted union of all ranges, and each peak holds an inclusive
[lo, hi] into that union (a range is a run of consecutive track rows, so it is a run of consecutive rows of the union too).

Replicate r of input file f.
    K_r  = replicate_key(S, r, f) = null.replicate_key(null.mix(S ^ SEED_DOMAIN), r, f)       (S = --locateSeed, default 1)
    w    = boot.site_weights(K_r, N, B)                                                       (B = --locateBlock, default 1)
    sites: np.repeat(genpos, w), np.repeat(rows, w) -- order kept, weight-0 sites dropped
    track: the ordinary grid scan of the union's test positions over that array, every window holding all its sites (the
           default window mode)
    argmax of a peak: the row of its range with the largest replicate CLR among the rows with a grid result; the earliest row
           wins a tie; none when no row has a result (or the resampled array is empty)
SEED_DOMAIN is this module's own: --locateSeed 1, --bootSeed 1 and --nullSeed 1 share nothing.

Summary of a peak over the n_ok replicates that have an argmax, at level L (--locateLevel, default 0.95); order statistics by
the rule of boot._rank / null.threshold, no interpolation:
    lo, hi          the ceil((1 - L) / 2 * n_ok)-th (at least the 1st) and the ceil((1 + L) / 2 * n_ok)-th smallest argmax ROW
                    (row order is position order, so the ends are rows of the main output and print as its strings)
    gen_sd          the sample standard deviation (ddof 1) of the argmax test positions
    p_apex          the share of ok replicates whose argmax is the apex row
    p_edge          the share whose argmax is the first or the last row of the range: when this is not small, H is too small
                    and the interval is censored
    CLR_lo, CLR_hi  the same two order statistics of the replicate maxima
With n_ok < 2 everything but CLR and n_ok is NA.

What this is.  A bootstrap of the GRID scan's argmax within +-H of each apex, not of a refined maximum; the test positions stay
fixed, so the interval lives on the test-site grid (-s coarsens it) and cannot be finer than it; linkage disequilibrium is
respected only up to a block of B sites (B = 1 treats sites as independent and gives intervals as narrow as that); demography
is not modelled; percentile ends from R replicates cannot resolve tails finer than 1 / R.  Window modes that count sites or
nucleotides (-w, --fixWinSize) are not defined on a resampled array and are refused.
"""
import math

import numpy as np

from . import boot, null, peaks

_M64 = (1 << 64) - 1
SEED_DOMAIN = 0x10CA7E10CA7E10CA      # seed ^ this, mixed: the keys are neither the bootstrap's nor the permutation null's
LEVEL = 0.95


def replicate_key(seed, r, f=0):
    """The key of replicate r of input file f (file ordinal 0 for a single file)."""
    return null.replicate_key(null.mix((int(seed) & _M64) ^ SEED_DOMAIN), r, f)


def value_refusal(R, block, span, level, min_clr):
    """The message that refuses these values of --locate / --locateBlock / --locateSpan / --locateLevel / --locateMin (None:
    the flag was not given), or None."""
    if R < 2:
        return '--locate takes a number of replicates >= 2 (0: off).'
    if block is not None and block < 1:
        return '--locateBlock must be >= 1.'
    if span is not None and not (math.isfinite(span) and span > 0.0):
        return '--locateSpan takes a finite number H > 0 (in the units --peaks measures in).'
    if level is not None and not (0.0 < level < 1.0):
        return '--locateLevel takes a number L with 0 < L < 1.'
    if min_clr is not None and min_clr != min_clr:
        return '--locateMin takes a number.'
    return None


# ------------------------------------------------------------------------------------------- the host restatements

def resampled(gen, rows, key, block=1):
    """The resampled chromosome of one replicate: (np.repeat(gen, w), np.repeat(rows, w)), w = boot.site_weights(key, N, block)
    -- what bmx_ctx_resample_sites builds on the device, exactly."""
    gen, rows = np.asarray(gen, dtype=np.float64), np.asarray(rows)
    w = boot.site_weights(key, len(gen), block)
    return np.repeat(gen, w), np.repeat(rows, w)


def ranges(g, apex_rows, span):
    """The search ranges of the apexes at track rows apex_rows (ascending) on the track positions g (non-decreasing):
    (union, lo, hi) -- the sorted union of the ranges as track rows (int64), and per apex the inclusive [lo, hi] into it."""
    g = np.ascontiguousarray(g, dtype=np.float64)
    a = np.ascontiguousarray(apex_rows, dtype=np.int64)
    if not len(a):
        z = np.zeros(0, dtype=np.int64)
        return z, z.copy(), z.copy()
    if not (math.isfinite(span) and span > 0.0):
        raise ValueError('the span must be finite and > 0')
    first, last = peaks._ranges(g, a, float(span))
    mark = np.zeros(len(g) + 1, dtype=np.int64)
    np.add.at(mark, first, 1)
    np.add.at(mark, last + 1, -1)
    union = np.nonzero(np.cumsum(mark[:-1]) > 0)[0].astype(np.int64)
    return union, np.searchsorted(union, first).astype(np.int64), np.searchsorted(union, last).astype(np.int64)


def argmax_rows(clr, has, lo, hi):
    """bmx_ctx_locate_accumulate on the host: per range [lo[k], hi[k]] of a replicate's track (clr; has: the row has a grid
    result) the first row of the largest clr among the rows with a result, and that clr: (row int32, -1: none; clr, 0 there)."""
    clr, has = np.asarray(clr, dtype=np.float64), np.asarray(has, dtype=bool)
    row, val = np.full(len(lo), -1, dtype=np.int32), np.zeros(len(lo), dtype=np.float64)
    for k, (a, b) in enumerate(zip(np.asarray(lo).tolist(), np.asarray(hi).tolist())):
        ok = np.nonzero(has[a:b + 1])[0]
        if len(ok):
            j = a + int(ok[int(np.argmax(clr[a:b + 1][ok]))])            # argmax: the first row of the maximum
            row[k], val[k] = j, clr[j]
    return row, val


def host_locate(scan, gen, rows, test_gen, lo, hi, keys, block=1):
    """The replicates on the host: scan(gen', rows', test_gen) -> (clr[M], has[M]) is run on every resampled array (the tests
    pass an independent host implementation of the scan).  Returns (row int32[R, K], clr f64[R, K], tracks: the R (clr, has)
    pairs, None where the resampled array is empty)."""
    R, K = len(keys), len(lo)
    row, val, tracks = np.full((R, K), -1, dtype=np.int32), np.zeros((R, K), dtype=np.float64), []
    for r, key in enumerate(keys):
        g, rw = resampled(gen, rows, key, block)
        if not len(g):
            tracks.append(None)
            continue
        clr, has = scan(g, rw, test_gen)
        tracks.append((clr, has))
        row[r], val[r] = argmax_rows(clr, has, lo, hi)
    return row, val, tracks


# ---------------------------------------------------------------------------------------------------------- summary

def summarise(arg, clr, g, apex, lo, hi, level=LEVEL):
    """The summary of one peak from its replicates: arg[R] the argmax rows (-1: none) and clr[R] the maxima, g the test position
    of every row arg may name, apex / lo / hi the peak's own row and the ends of its range (the same row numbering).
    {'lo', 'hi': rows (-1: NA), 'gen_sd', 'p_apex', 'p_edge', 'CLR_lo', 'CLR_hi': floats (NaN: NA), 'n_ok'}."""
    arg = np.asarray(arg, dtype=np.int64)
    ok = arg >= 0
    n = int(ok.sum())
    out = dict(lo=-1, hi=-1, gen_sd=math.nan, p_apex=math.nan, p_edge=math.nan, CLR_lo=math.nan, CLR_hi=math.nan, n_ok=n)
    if n < 2:
        return out
    a = np.sort(arg[ok])
    v = np.sort(np.asarray(clr, dtype=np.float64)[ok])
    i, j = boot._rank((1.0 - level) / 2.0, n) - 1, boot._rank((1.0 + level) / 2.0, n) - 1
    out.update(lo=int(a[i]), hi=int(a[j]), CLR_lo=float(v[i]), CLR_hi=float(v[j]),
               gen_sd=float(np.std(np.asarray(g, dtype=np.float64)[a], ddof=1)),
               p_apex=float(np.count_nonzero(a == int(apex))) / n,
               p_edge=float(np.count_nonzero((a == int(lo)) | (a == int(hi)))) / n)
    return out


# ---------------------------------------------------------------------------------------------------------- output

HEADER = 'physPos\tgenPos\tCLR\tlo_physPos\thi_physPos\tlo_genPos\thi_genPos\tgen_sd\tp_apex\tp_edge\tCLR_lo\tCLR_hi\tn_ok\n'
REPS_HEADER = 'physPos\tgenPos\treplicate\targ_physPos\targ_genPos\tCLR\n'


def output_name(outfile):
    return outfile + '.locate.txt'


def reps_name(outfile):
    return outfile + '.locate.reps.txt'


def _fmt(v):
    return 'NA' if v != v else repr(float(v))


def format_row(head, s, pos_of):
    """One line of <out>.locate.txt: head = the apex's (physPos, genPos, CLR) strings, s = summarise()'s dict, pos_of(row) =
    the (physPos, genPos) strings of a row."""
    if s['lo'] >= 0:
        a, b = pos_of(s['lo']), pos_of(s['hi'])
        ends = [a[0], b[0], a[1], b[1]]
    else:
        ends = ['NA'] * 4
    vals = [_fmt(s[k]) for k in ('gen_sd', 'p_apex', 'p_edge', 'CLR_lo', 'CLR_hi')]
    return '\t'.join(list(head) + ends + vals + [repr(int(s['n_ok']))]) + '\n'


def main_columns(main_path, line_of_row=None):
    """col(t): the columns of track row t in the main output (line_of_row: the line of every track row, None: row t is line
    t + 1 -- cli.call_peaks' second value)."""
    with open(main_path) as f:
        lines = f.readlines()
    at = (lambda t: int(t) + 1) if line_of_row is None else (lambda t: int(line_of_row[int(t)]))
    return lambda t: lines[at(t)].rstrip('\r\n').split('\t')


def write_locate(path, col, apex_rows, g, union, lo, hi, arg, clr, level=LEVEL):
    """<out>.locate.txt: one row per kept peak in position order.  col: main_columns(); apex_rows: the kept apexes' track rows;
    g: the track's test positions; union, lo, hi: ranges(); arg, clr: [R, K] argmax rows INTO THE UNION (-1: none) and maxima."""
    out = [HEADER]
    pos_of = lambda u: col(union[u])[:2]
    gu = np.asarray(g, dtype=np.float64)[union] if len(union) else np.zeros(0)
    for k, a in enumerate(np.asarray(apex_rows).tolist()):
        s = summarise(arg[:, k], clr[:, k], gu, int(np.searchsorted(union, a)), lo[k], hi[k], level)
        out.append(format_row(col(a)[:3], s, pos_of))
    with open(path, 'w') as f:
        f.writelines(out)


def write_reps(path, col, apex_rows, union, arg, clr):
    """<out>.locate.reps.txt: one row per (peak, ok replicate), peak-major in position order."""
    with open(path, 'w') as f:
        f.write(REPS_HEADER)
        for k, a in enumerate(np.asarray(apex_rows).tolist()):
            head = col(a)[:2]
            for r in range(arg.shape[0]):
                if arg[r, k] >= 0:
                    f.write('\t'.join(head + [str(r)] + col(union[arg[r, k]])[:2] + [repr(float(clr[r, k]))]) + '\n')


def read_locate(path):
    """The rows of a <out>.locate.txt as dicts: the position columns and CLR as printed, the statistics as floats (NaN: NA),
    n_ok as int."""
    names = HEADER.rstrip('\n').split('\t')
    rows = []
    with open(path) as f:
        assert f.readline() == HEADER
        for l in f:
            c = l.rstrip('\n').split('\t')
            d = dict(zip(names[:7], c[:7]))
            d.update({k: (math.nan if v == 'NA' else float(v)) for k, v in zip(names[7:12], c[7:12])})
            d['n_ok'] = int(c[12])
            rows.append(d)
    return rows


def read_reps(path):
    """{(physPos, genPos) as printed: {'replicate': i32[n], 'arg_physPos', 'arg_genPos': lists of strings, 'CLR': f64[n]}} of a
    <out>.locate.reps.txt."""
    out = {}
    with open(path) as f:
        assert f.readline() == REPS_HEADER
        for l in f:
            c = l.rstrip('\n').split('\t')
            d = out.setdefault((c[0], c[1]), dict(replicate=[], arg_physPos=[], arg_genPos=[], CLR=[]))
            d['replicate'].append(int(c[2]))
            d['arg_physPos'].append(c[3])
            d['arg_genPos'].append(c[4])
            d['CLR'].append(float(c[5]))
    for d in out.values():
        d['replicate'] = np.array(d['replicate'], dtype=np.int32)
        d['CLR'] = np.array(d['CLR'], dtype=np.float64)
    return out


# ---------------------------------------------------------------------------------------------------------- driver

def track_positions(ts):
    """The test position of every track row of a scan.TestSites (what the scan used, float64)."""
    return np.asarray(ts.arrays[1] if ts.arrays is not None else ts.test_gen, dtype=np.float64)


def kept_apexes(pk_rows, clr, min_clr=None):
    """The apexes (track rows, ascending) with CLR >= min_clr (None: all of them)."""
    rows = np.asarray(pk_rows, dtype=np.int64)
    return rows if min_clr is None else rows[np.asarray(clr, dtype=np.float64)[rows] >= min_clr]


def run_replicates(ctx, test_gen, lo, hi, keys, block=1, slot=None):
    """The replicates of the chromosome in ctx's selected slot on the device: per key, resample it into a spare slot, set the
    test positions, scan, reduce.  Returns (row int32[R, K] into test_gen, -1: none; clr f64[R, K]; N' of every replicate);
    the observed slot is selected again and untouched."""
    obs, N_obs = ctx.slot, getattr(ctx, 'N', 0)
    if slot is None:
        slot = getattr(ctx, '_locate_slot', None)
        if slot is None or slot == obs:
            slot = max(ctx.slot_count(), obs + 1)
        ctx._locate_slot = slot
    sizes = np.zeros(len(keys), dtype=np.int64)
    ctx.select_slot(slot)
    try:
        ctx.locate_begin(lo, hi, len(keys))
        for r, key in enumerate(keys):
            sizes[r] = ctx.resample_sites(obs, key, block)
            if sizes[r] == 0:                   # every weight is 0: the replicate has no track
                continue
            ctx.set_tests(test_gen)
            ctx.scan()
            ctx.locate_accumulate(r)
        row, clr = ctx.fetch_locate()
    finally:
        ctx.select_slot(obs)
        ctx.N = N_obs
    return row, clr, sizes


def locate_and_write(ctx, outfile, ts, called, R, seed=1, block=1, span=None, level=LEVEL, min_clr=None, f=0, reps=False):
    """After the observed scan and the peak call (`called`: cli.call_peaks' pair) of one file (input-file ordinal f) on ctx's
    selected slot: its position bootstrap into <outfile>.locate.txt and, with reps, <outfile>.locate.reps.txt.  span: H (the
    caller passes --peaks' G when --locateSpan was not given).  Returns (peaks kept, replicates with an empty resampled array)."""
    pk, line_of_row = called
    col = main_columns(outfile, line_of_row)
    z = np.zeros(0, dtype=np.int64)
    apex = z
    if len(ts) and len(pk['row']):
        obs_clr, _, _, iA, _ = ctx.fetch()
        apex = kept_apexes(pk['row'], np.where(iA >= 0, obs_clr, 0.0), min_clr)
    if not len(apex):
        e = np.zeros((R, 0))
        write_locate(output_name(outfile), col, z, z, z, z, z, e.astype(np.int32), e, level)
        if reps:
            write_reps(reps_name(outfile), col, z, z, e.astype(np.int32), e)
        return 0, 0
    g = track_positions(ts)
    union, lo, hi = ranges(g, apex, span)
    row, clr, sizes = run_replicates(ctx, g[union], lo, hi, [replicate_key(seed, r, f) for r in range(R)], block)
    write_locate(output_name(outfile), col, apex, g, union, lo, hi, row, clr, level)
    if reps:
        write_reps(reps_name(outfile), col, apex, union, row, clr)
    return len(apex), int(np.count_nonzero(sizes == 0))
