"""Planted-signal power analysis of the scan: the definition behind --power, its host restatements, its summary rules and writers.

Every other layer describes what the scan FOUND.  --power describes what it COULD have found: with this SNP density, these
sample sizes and this spectrum, how often would a locus of strength (A, x, alpha_beta) reach a given CLR threshold, and how well
would the scan place it?  The composite likelihood is itself a generative model, so the simulation needs nothing from outside:
every site within reach of a chosen position redraws its derived count from the mixture the scan fits, the positions and the
sample sizes stay the user's own, the rows are rewritten on the device (bmx_ctx_plant_sites), the neighbourhood is scanned by the
unchanged kernels, and each locus's range is reduced to its maximum (bmx_ctx_locate_accumulate, bmx_ctx_fetch_at).

Planted model.  ONE grid point (iA, ix, ia) of the run's model: --plant A,x,abeta must name grid values (float(v) == float(grid
value)).  The selection table R of the grid is resident on the device, so no selection probability is computed anew.

Admissible counts.  gw[row] = g[row] where the neutral probability g is finite and > 0 and the count is not an excluded count of
the statistic (allowed_rows; include/bmxscan.h BMX_STAT_*: B2 and B1 exclude k < minCount, B2maf also n - minCount < k < n, B0
also k = n, B0maf also k > n - minCount); 0 elsewhere.  A draw never lands on a row with gw = 0.

A site i of size block j is IN REACH of a centre c when genpos_i != c and A * |genpos_i - c| <= alpha_cut -- the scan's own window
predicate and its exclusion of the sites at the test position (alpha_cut = bmx_alpha_cut(), ALPHA_CUT below).  Such a site draws
    alpha_i = exp(-A * |genpos_i - c|)
    m_k     = max(0, gw[r] * (1 + alpha_i * R[ix][ia][r])),  r = row_off[j] + k, k over the rows of its size; non-finite: 0
    total   = sum_k m_k, in ascending k
    u_i     = (mix(K ^ mix(i)) >> 11) * 2^-53          (null.mix; i: the site's index in the source array)
    new row = the first k, ascending, whose running sum exceeds u_i * total; the last k with m_k > 0 if rounding leaves none
and keeps its row when total is not finite and > 0.  Sites out of reach of every centre keep their row; positions and sample sizes
never change.  The draw normalises by its own total, so the reference's normalisation quirks of the MAF statistics do not enter.
Centres ascend strictly with A * (c[k+1] - c[k]) > 2.000001 * alpha_cut: no site is in reach of two.

Host restatement.  planted_rows() below, with np.exp.  The device's exp (about 1 ulp) can move a running sum by about 1e-15
relative, so planted_rows also returns margin_i = min_k |u_i * total - cum_k| / total, and a site is DECIDED when its margin is
> MARGIN = 1e-12: device and host agree on every decided site.

Replicate r of input file f.
    K_r  = null.replicate_key(null.mix(S ^ SEED_DOMAIN), r, f)               (S = --powerSeed, default 1)
    background `perm` (default): the observed slot's rows are first permuted by bmx_ctx_permute_rows(K'_r, B),
               K'_r = null.replicate_key(null.mix(S ^ PERM_DOMAIN), r, f), B = --powerBlock (default 1); `obs`: rows as given
    the planted array is built into a spare slot (locate.run_replicates' choice), the union of the centres' search ranges is
    scanned, every range is reduced to (argmax row, CLR), and (grid point, nSites) are read at the argmax rows
The observed slot's rows are restored after the last replicate and the slot is selected again.  Both domains are this module's
own: --powerSeed 1 shares its stream with none of the other seeds.

Centres of a file (centres()).  g = the track's test positions (locate.track_positions).  Targets g[0] + (j + 0.5) * D, j = 0, 1,
... while <= g[-1]; a centre is the first track row at or after its target; it is dropped when it repeats or lies closer than
`bound` to the previously kept centre.  bound = H + alpha_cut / A_min + alpha_cut / A_plant (A_min: the smallest A of the grid):
beyond that distance the redrawn sites of one locus cannot enter a window scanned for another.  D = --plantEvery, default 1.05 *
bound; a smaller D is refused.  H = --powerSpan, default --peaks' G when given, else alpha_cut / A_plant.  Search ranges and
their union: locate.ranges(g, centre rows, H).

Thresholds.  --powerThreshold C[,C...]; with --nullPerm the run's own genome-wide 5 % and 1 % thresholds are added (the power step
then runs after the null).  With neither the run is refused.

Summary of a centre over its n_ok replicates that have an argmax (summarise(); order statistics by boot._rank, level 0.95, no
interpolation): CLR_lo, CLR_med, CLR_hi of the range maxima; power_C = the share whose maximum is >= C; lo, hi = the order
statistics of the argmax ROW; pos_rmse = the RMS of argmax test position minus centre position; p_edge = the share whose argmax
is the first or last row of the range; p_x, p_s, p_A, p_all = the shares whose argmax grid value (x, alpha_beta, A, all three)
is the planted one.  With n_ok < 2 everything but nReach (the sites in reach) and n_ok is NA.

What this is not.  Sites are drawn independently -- the composite likelihood's own assumption.  Real loci carry linkage
disequilibrium, so this power is an upper bound in spirit, not a coalescent simulation; demography is not modelled; the `perm`
background is exchangeable (LD survives only within a block of B sites).  Window modes that count sites or nucleotides (-w,
--fixWinSize) are refused as --locate refuses them (N does not change here, so they could be supported later).
"""
import math

import numpy as np

from . import boot, locate, null

_M64 = (1 << 64) - 1
SEED_DOMAIN = 0x9A17ED5179A17ED5      # seed ^ this, mixed: the keys of the draws
PERM_DOMAIN = 0xBAC6B0D9BAC6B0D9      # ... and of the permuted backgrounds
ALPHA_CUT = 18.420680743952364        # bmx_alpha_cut(): the largest z with exp(-z) >= 1e-8
MARGIN = 1e-12
LEVEL = 0.95
SPACING = 2.000001                    # centres lie more than SPACING * alpha_cut / A apart
STAT_NAMES = ('B2', 'B2maf', 'B0', 'B0maf', 'B1')


def replicate_key(seed, r, f=0):
    """The key of the draws of replicate r of input file f."""
    return null.replicate_key(null.mix((int(seed) & _M64) ^ SEED_DOMAIN), r, f)


def background_key(seed, r, f=0):
    """The key of the permuted background of replicate r of input file f."""
    return null.replicate_key(null.mix((int(seed) & _M64) ^ PERM_DOMAIN), r, f)


def value_refusal(R, every, span, block, background, thresholds):
    """The message that refuses these values of --power / --plantEvery / --powerSpan / --powerBlock / --powerBackground /
    --powerThreshold (None: the flag was not given), or None."""
    if R < 2:
        return '--power takes a number of replicates >= 2 (0: off).'
    if every is not None and not (math.isfinite(every) and every > 0.0):
        return '--plantEvery takes a finite spacing D > 0 (in the units of the test positions).'
    if span is not None and not (math.isfinite(span) and span > 0.0):
        return '--powerSpan takes a finite number H > 0 (in the units of the test positions).'
    if block is not None and block < 1:
        return '--powerBlock must be >= 1.'
    if background is not None and background not in ('perm', 'obs'):
        return '--powerBackground takes perm or obs.'
    if thresholds is not None:
        try:
            parse_thresholds(thresholds)
        except ValueError as e:
            return str(e)
    return None


def parse_thresholds(text):
    """--powerThreshold C[,C...] as floats, in the order given, repeats dropped."""
    out = []
    for part in str(text).split(','):
        try:
            v = float(part)
        except ValueError:
            v = math.nan
        if v != v:
            raise ValueError('--powerThreshold takes numbers C[,C...]; got %r.' % part)
        if v not in out:
            out.append(v)
    return out


def parse_plant(text, As, xs, abetas):
    """--plant A,x,abeta as grid indices (iA, ix, ia); ValueError (with the grids printed) unless each value is a grid value."""
    parts = str(text).split(',')
    grids = '\n  A: %s\n  x: %s\n  abeta: %s' % tuple(', '.join(repr(float(v)) for v in g) for g in (As, xs, abetas))
    if len(parts) != 3:
        raise ValueError('--plant takes A,x,abeta (three grid values).  The grids:' + grids)
    out = []
    for name, part, grid in zip(('A', 'x', 'abeta'), parts, (As, xs, abetas)):
        try:
            v = float(part)
        except ValueError:
            v = math.nan
        hit = [i for i, gv in enumerate(grid) if float(gv) == v]
        if not hit:
            raise ValueError('--plant: %s = %s is not a value of the grid.  The grids:%s' % (name, part, grids))
        out.append(hit[0])
    return tuple(out)


# ------------------------------------------------------------------------------------------- the host restatements

def allowed_rows(stat, min_count, sizes, row_off, g):
    """gw[rows]: g where it is finite and > 0 and the row's count is not an excluded count of the statistic, 0 elsewhere.
    The excluded counts (include/bmxscan.h BMX_STAT_*; m = min_count, n the sample size): B2 and B1 k < m; B2maf k < m and
    n - m < k < n; B0 k < m and k = n; B0maf k < m and k > n - m.  (B1 has two rows per size: 0 substitution, 1 polymorphism.)"""
    if stat not in STAT_NAMES:
        raise ValueError(stat)
    g = np.asarray(g, dtype=np.float64)
    m = int(min_count)
    gw = np.zeros(len(g), dtype=np.float64)
    for j, n in enumerate(np.asarray(sizes).tolist()):
        a, b = int(row_off[j]), int(row_off[j + 1])
        k = np.arange(b - a)
        bad = k < m
        if stat == 'B2maf':
            bad |= (k > n - m) & (k < n)
        elif stat == 'B0':
            bad |= k == n
        elif stat == 'B0maf':
            bad |= k > n - m
        v = g[a:b]
        with np.errstate(invalid='ignore'):
            ok = np.isfinite(v) & (v > 0.0) & ~bad
        gw[a:b] = np.where(ok, v, 0.0)
    return gw


def uniforms(key, idx):
    """u_i = (mix(key ^ mix(i)) >> 11) * 2^-53 of the site indices idx."""
    i = np.asarray(idx).astype(np.uint64)
    h = null.mix(np.uint64(int(key) & _M64) ^ null.mix(i))
    return (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def check_centres(centres, A, zcut=ALPHA_CUT):
    """ValueError unless the centres are finite and ascend with A * (c[k+1] - c[k]) > SPACING * zcut."""
    c = np.asarray(centres, dtype=np.float64)
    if c.ndim != 1 or not np.all(np.isfinite(c)):
        raise ValueError('the centres must be a flat list of finite positions')
    if len(c) > 1 and not np.all(A * np.diff(c) > SPACING * zcut):
        raise ValueError('the centres must ascend and lie more than twice the reach apart')
    return c


def reach(genpos, c, A, zcut=ALPHA_CUT):
    """(in reach bool[N], first, count) of one centre: the sites with A |g - c| <= zcut and g != c, and the run of sites that
    satisfy the first condition alone (what bmx_ctx_plant_sites reports: it holds the sites AT c too)."""
    g = np.asarray(genpos, dtype=np.float64)
    w = 1.001 * zcut / A + 4.0 * np.spacing(abs(c))                # a bracket that covers the run; the exact predicate decides
    a, b = int(np.searchsorted(g, c - w, side='left')), int(np.searchsorted(g, c + w, side='right'))
    far = A * np.abs(g[a:b] - c) > zcut
    first = a + int(np.count_nonzero((g[a:b] < c) & far))
    count = b - int(np.count_nonzero((g[a:b] > c) & far)) - first
    inr = np.zeros(len(g), dtype=bool)
    inr[a:b] = ~far & (g[a:b] != c)
    return inr, first, count


def planted_rows(genpos, rows, sizes, row_off, R_slice, gw, A, centres, key, zcut=ALPHA_CUT):
    """bmx_ctx_plant_sites on the host.  genpos[N] (non-decreasing), rows[N] (table rows), the model's sizes / row_off, R_slice =
    R[ix][ia][:] of the planted pair, gw = allowed_rows(), A the planted A, centres ascending, key the replicate's.  Returns
    (new_rows int32[N], margin f64[N]): margin_i = min_k |u_i total - cum_k| / total of a redrawn site, +inf of every other."""
    g = np.asarray(genpos, dtype=np.float64)
    rows = np.asarray(rows)
    off = np.asarray(row_off, dtype=np.int64)
    Rs, gw = np.asarray(R_slice, dtype=np.float64), np.asarray(gw, dtype=np.float64)
    c = check_centres(centres, A, zcut)
    new = rows.astype(np.int32).copy()
    margin = np.full(len(g), np.inf)
    block = np.searchsorted(off, rows, side='right') - 1          # the size block of every site
    for ck in c.tolist():
        inr, first, count = reach(g, ck, A, zcut)
        idx_all = first + np.nonzero(inr[first:first + count])[0]
        for j in np.unique(block[idx_all]).tolist():
            idx = idx_all[block[idx_all] == j]
            a, b = int(off[j]), int(off[j + 1])
            alpha = np.exp(-(A * np.abs(g[idx] - ck)))
            with np.errstate(invalid='ignore', over='ignore'):
                m = gw[a:b][None, :] * (1.0 + alpha[:, None] * Rs[a:b][None, :])
                m = np.where(np.isfinite(m) & (m > 0.0), m, 0.0)
            cum = np.cumsum(m, axis=1)                            # sequential, ascending k: the kernel's order
            total = cum[:, -1]
            ok = np.isfinite(total) & (total > 0.0)
            target = uniforms(key, idx) * total
            above = cum > target[:, None]
            last = (b - a - 1) - np.argmax(m[:, ::-1] > 0.0, axis=1)
            pick = np.where(above.any(axis=1), np.argmax(above, axis=1), last)
            with np.errstate(invalid='ignore', divide='ignore'):
                mg = np.min(np.abs(target[:, None] - cum), axis=1) / total
            new[idx[ok]] = (a + pick[ok]).astype(np.int32)
            margin[idx[ok]] = mg[ok]
    return new, margin


def spacing_refusal(D, bound):
    return ('--plantEvery %r is smaller than the bound %r (H + alpha_cut / A_min + alpha_cut / A_plant) below which the redrawn '
            'sites of one locus enter the windows scanned for the next.' % (float(D), float(bound)))


def centres(g, D, bound):
    """The centre rows of a track with test positions g (non-decreasing): targets g[0] + (j + 0.5) * D while <= g[-1], each
    snapped to the first row at or after it, dropped when it repeats or lies closer than `bound` to the previously kept centre.
    ValueError when D < bound."""
    g = np.asarray(g, dtype=np.float64)
    if not (math.isfinite(D) and math.isfinite(bound) and bound > 0.0):
        raise ValueError('spacing and bound must be finite and > 0')
    if D < bound:
        raise ValueError(spacing_refusal(D, bound))
    out = []
    if not len(g):
        return np.zeros(0, dtype=np.int64)
    j = 0
    while True:
        t = g[0] + (j + 0.5) * D
        if not t <= g[-1]:
            break
        row = int(np.searchsorted(g, t, side='left'))
        if not out or (row != out[-1] and not g[row] - g[out[-1]] < bound):
            out.append(row)
        j += 1
    return np.array(out, dtype=np.int64)


def bound_of(H, A_min, A_plant, zcut=ALPHA_CUT):
    return H + zcut / A_min + zcut / A_plant


def decode(lin, nx, nab):
    """(iA, ix, ia) of linear grid indices (iA * nx + ix) * nab + ia; -1 stays -1 in all three."""
    lin = np.asarray(lin, dtype=np.int64)
    ok = lin >= 0
    iA, rem = np.divmod(np.where(ok, lin, 0), nx * nab)
    ix, ia = np.divmod(rem, nab)
    return tuple(np.where(ok, v, -1).astype(np.int32) for v in (iA, ix, ia))


def host_power(scan, genpos, rows, sizes, row_off, R_slice, gw, A, centre_pos, test_gen, lo, hi, seed, R, f=0,
               background='perm', block=1, plant=True):
    """The replicates on the host: scan(gen, rows', test_gen) -> (clr[M], lin[M], nsites[M]) is run on every planted array (the
    tests pass an independent host implementation of the scan).  Returns (arg int32[R, K] into test_gen, clr f64[R, K], lin
    int32[R, K], nsites int32[R, K]).  plant=False scans the backgrounds alone (the same permutations, nothing redrawn)."""
    K = len(lo)
    arg, val = np.full((R, K), -1, dtype=np.int32), np.zeros((R, K), dtype=np.float64)
    lin, ns = np.full((R, K), -1, dtype=np.int32), np.zeros((R, K), dtype=np.int32)
    rows = np.asarray(rows)
    for r in range(R):
        bg = rows[null.block_permutation(len(rows), background_key(seed, r, f), block)] if background == 'perm' else rows
        new = planted_rows(genpos, bg, sizes, row_off, R_slice, gw, A, centre_pos, replicate_key(seed, r, f))[0] if plant else bg
        clr, l, n = scan(genpos, new, test_gen)
        arg[r], val[r] = locate.argmax_rows(clr, np.asarray(l) >= 0, lo, hi)
        got = arg[r] >= 0
        lin[r, got], ns[r, got] = np.asarray(l)[arg[r, got]], np.asarray(n)[arg[r, got]]
    return arg, val, lin, ns


# ---------------------------------------------------------------------------------------------------------- summary

def summarise(arg, clr, lin, g, centre, lo, hi, planted, nx, nab, thresholds, level=LEVEL):
    """The summary of one centre from its replicates: arg[R] the argmax rows (-1: none), clr[R] the maxima, lin[R] the linear
    grid index at the argmax; g the test position of every row arg may name; centre / lo / hi the centre's own row and the ends
    of its range (the same numbering); planted = (iA, ix, ia).  {'n_ok', 'CLR_lo', 'CLR_med', 'CLR_hi', 'power': [one per
    threshold], 'lo', 'hi': rows (-1: NA), 'pos_rmse', 'p_edge', 'p_x', 'p_s', 'p_A', 'p_all'} (NaN: NA)."""
    arg = np.asarray(arg, dtype=np.int64)
    ok = arg >= 0
    n = int(ok.sum())
    nan = math.nan
    out = dict(n_ok=n, CLR_lo=nan, CLR_med=nan, CLR_hi=nan, power=[nan] * len(thresholds), lo=-1, hi=-1, pos_rmse=nan, p_edge=nan,
               p_x=nan, p_s=nan, p_A=nan, p_all=nan)
    if n < 2:
        return out
    a = arg[ok]
    v = np.asarray(clr, dtype=np.float64)[ok]
    iA, ix, ia = decode(np.asarray(lin)[ok], nx, nab)
    sa, sv = np.sort(a), np.sort(v)
    i, h, j = (boot._rank(q, n) - 1 for q in ((1.0 - level) / 2.0, 0.5, (1.0 + level) / 2.0))
    g = np.asarray(g, dtype=np.float64)
    d = g[a] - g[int(centre)]
    sx, ss, sA = ix == planted[1], ia == planted[2], iA == planted[0]
    out.update(CLR_lo=float(sv[i]), CLR_med=float(sv[h]), CLR_hi=float(sv[j]),
               power=[float(np.count_nonzero(v >= C)) / n for C in thresholds],
               lo=int(sa[i]), hi=int(sa[j]), pos_rmse=float(np.sqrt(np.mean(d * d))),
               p_edge=float(np.count_nonzero((a == int(lo)) | (a == int(hi)))) / n,
               p_x=float(np.count_nonzero(sx)) / n, p_s=float(np.count_nonzero(ss)) / n, p_A=float(np.count_nonzero(sA)) / n,
               p_all=float(np.count_nonzero(sx & ss & sA)) / n)
    return out


# ---------------------------------------------------------------------------------------------------------- output

REPS_HEADER = 'physPos\tgenPos\treplicate\targ_physPos\targ_genPos\tCLR\tx_hat\ts_hat\tA_hat\tnSites\n'
_TAIL = ('lo_physPos', 'hi_physPos', 'lo_genPos', 'hi_genPos', 'pos_rmse', 'p_edge', 'p_x', 'p_s', 'p_A', 'p_all')


def header(thresholds):
    cols = ['physPos', 'genPos', 'nReach', 'n_ok', 'CLR_lo', 'CLR_med', 'CLR_hi'] + ['power_%r' % float(C) for C in thresholds]
    return '\t'.join(cols + list(_TAIL)) + '\n'


def output_name(outfile):
    return outfile + '.power.txt'


def reps_name(outfile):
    return outfile + '.power.reps.txt'


def _fmt(v):
    return 'NA' if v != v else repr(float(v))


def format_row(head, n_reach, s, pos_of):
    """One line of <out>.power.txt: head = the centre's (physPos, genPos) strings, s = summarise()'s dict, pos_of(row) = the
    (physPos, genPos) strings of a row."""
    if s['lo'] >= 0:
        a, b = pos_of(s['lo']), pos_of(s['hi'])
        ends = [a[0], b[0], a[1], b[1]]
    else:
        ends = ['NA'] * 4
    vals = [_fmt(s[k]) for k in ('CLR_lo', 'CLR_med', 'CLR_hi')] + [_fmt(p) for p in s['power']]
    tail = [_fmt(s[k]) for k in ('pos_rmse', 'p_edge', 'p_x', 'p_s', 'p_A', 'p_all')]
    return '\t'.join(list(head) + [repr(int(n_reach)), repr(int(s['n_ok']))] + vals + ends + tail) + '\n'


def write_power(path, col, centre_rows, n_reach, g, union, lo, hi, arg, clr, lin, planted, nx, nab, thresholds, level=LEVEL):
    """<out>.power.txt: one row per centre in position order.  col: locate.main_columns(); centre_rows: the centres' track rows;
    g: the track's test positions; union, lo, hi: locate.ranges(); arg, clr, lin: [R, K] argmax rows INTO THE UNION (-1: none),
    maxima and grid indices.  Returns the summaries."""
    out, sums = [header(thresholds)], []
    pos_of = lambda u: col(union[u])[:2]
    gu = np.asarray(g, dtype=np.float64)[union] if len(union) else np.zeros(0)
    for k, a in enumerate(np.asarray(centre_rows).tolist()):
        s = summarise(arg[:, k], clr[:, k], lin[:, k], gu, int(np.searchsorted(union, a)), lo[k], hi[k], planted, nx, nab,
                      thresholds, level)
        sums.append(s)
        out.append(format_row(col(a)[:2], n_reach[k], s, pos_of))
    with open(path, 'w') as f:
        f.writelines(out)
    return sums


def write_reps(path, col, centre_rows, union, arg, clr, lin, ns, xs, abs_, As):
    """<out>.power.reps.txt: one row per (centre, ok replicate), centre-major in position order; xs / abs_ / As: the grids'
    printed forms as the main output prints them."""
    nx, nab = len(xs), len(abs_)
    with open(path, 'w') as f:
        f.write(REPS_HEADER)
        for k, a in enumerate(np.asarray(centre_rows).tolist()):
            head = col(a)[:2]
            iA, ix, ia = decode(lin[:, k], nx, nab)
            for r in range(arg.shape[0]):
                if arg[r, k] >= 0:
                    grid = [xs[ix[r]], abs_[ia[r]], As[iA[r]]] if lin[r, k] >= 0 else ['0.0'] * 3
                    f.write('\t'.join(head + [str(r)] + col(union[arg[r, k]])[:2] + [repr(float(clr[r, k]))] + grid
                                      + [str(int(ns[r, k]))]) + '\n')


def read_power(path):
    """(thresholds as printed, rows) of a <out>.power.txt: every row a dict of its columns' strings."""
    with open(path) as f:
        names = f.readline().rstrip('\n').split('\t')
        rows = [dict(zip(names, l.rstrip('\n').split('\t'))) for l in f]
    return [n[len('power_'):] for n in names if n.startswith('power_')], rows


def read_reps(path):
    """The rows of a <out>.power.reps.txt as dicts of strings."""
    names = REPS_HEADER.rstrip('\n').split('\t')
    with open(path) as f:
        assert f.readline() == REPS_HEADER
        return [dict(zip(names, l.rstrip('\n').split('\t'))) for l in f]


# ---------------------------------------------------------------------------------------------------------- driver

def run_replicates(ctx, test_gen, lo, hi, centre_pos, planted, gw, seed, R, f=0, background='perm', block=1, slot=None,
                   timing=None):
    """The replicates of the chromosome in ctx's selected slot on the device.  Returns (arg int32[R, K] into test_gen, -1: none;
    clr f64[R, K]; lin int32[R, K]; nsites int32[R, K]; first, count int32[K]: every centre's run of sites); the observed slot
    is selected again with its rows restored.  timing: a list that receives, per replicate, the seconds of (permute, plant,
    set_tests, scan, accumulate) and the plant step's device milliseconds."""
    import time
    obs, N_obs, M_obs = ctx.slot, getattr(ctx, 'N', 0), ctx.M
    if slot is None:
        slot = getattr(ctx, '_locate_slot', None)
        if slot is None or slot == obs:
            slot = max(ctx.slot_count(), obs + 1)
        ctx._locate_slot = slot
    iA, ix, ia = planted
    K = len(lo)
    first = count = np.zeros(K, dtype=np.int32)
    lin, ns = np.full((R, K), -1, dtype=np.int32), np.zeros((R, K), dtype=np.int32)
    try:
        ctx.select_slot(slot)
        ctx.locate_begin(lo, hi, R)
        for r in range(R):
            t = [time.perf_counter()]
            if background == 'perm':
                ctx.select_slot(obs)
                ctx.permute_rows(background_key(seed, r, f), block)
                ctx.select_slot(slot)
                if timing is not None:
                    ctx.sync()
            t.append(time.perf_counter())
            first, count, _ = ctx.plant_sites(obs, replicate_key(seed, r, f), centre_pos, iA, ix, ia, gw)
            t.append(time.perf_counter())
            ctx.set_tests(test_gen)
            if timing is not None:
                ctx.plan()
            t.append(time.perf_counter())
            ctx.scan()
            if timing is not None:
                ctx.sync()
            t.append(time.perf_counter())
            ctx.locate_accumulate(r)
            t.append(time.perf_counter())
            if timing is not None:
                timing.append(tuple(np.diff(t).tolist()) + (ctx.plant_ms(),))
            row_r, _ = ctx.fetch_locate()
            _, lin[r], ns[r] = ctx.fetch_at(row_r[r])
        arg, clr = ctx.fetch_locate()
    finally:
        ctx.select_slot(obs)
        ctx.restore_rows()
        ctx.N = N_obs
        ctx.M = M_obs
    return arg, clr, lin, ns, first, count


def n_reach(genpos, centre_pos, A, zcut=ALPHA_CUT):
    """The sites in reach of every centre."""
    return np.array([int(np.count_nonzero(reach(genpos, c, A, zcut)[0])) for c in np.asarray(centre_pos).tolist()], dtype=np.int64)


def plan_file(g, A_plant, A_min, span=None, every=None, zcut=ALPHA_CUT):
    """(centre rows, union, lo, hi, H, bound, D) of a track with test positions g."""
    H = float(span) if span is not None else zcut / A_plant
    bound = bound_of(H, A_min, A_plant, zcut)
    D = float(every) if every is not None else 1.05 * bound
    rows = centres(g, D, bound)
    union, lo, hi = locate.ranges(g, rows, H)
    return rows, union, lo, hi, H, bound, D


def power_and_write(ctx, outfile, ts, genpos, model, As, planted, thresholds, R, seed=1, background='perm', block=1, span=None,
                    every=None, f=0, reps=False, line_of_row=None, grids_printed=None):
    """After the observed scan of one file (input-file ordinal f) on ctx's selected slot: its power analysis into
    <outfile>.power.txt and, with reps, <outfile>.power.reps.txt.  genpos: the file's site positions; model: its
    engine.ModelArrays; As: the A grid in scan order; planted = (iA, ix, ia); span: H (None: alpha_cut / A_plant); every: D
    (None: 1.05 * bound); grids_printed = (xs, abs_, As) as the main output prints them.  Returns (centres, mean power per
    threshold: NaN without a summarised centre)."""
    col = locate.main_columns(outfile, line_of_row)
    nx, nab = len(model.x), len(model.abeta)
    zcut = ctx._L.bmx_alpha_cut()
    A_plant = float(As[planted[0]])
    z = np.zeros(0, dtype=np.int64)
    g = locate.track_positions(ts) if len(ts) else np.zeros(0)
    rows, union, lo, hi, H, bound, D = plan_file(g, A_plant, float(min(As)), span, every, zcut)
    e = np.zeros((R, 0))
    if not len(rows):
        write_power(output_name(outfile), col, z, z, g, z, z, z, e.astype(np.int32), e, e.astype(np.int32), planted, nx, nab, thresholds)
        if reps:
            write_reps(reps_name(outfile), col, z, z, e.astype(np.int32), e, e.astype(np.int32), e.astype(np.int32), *grids_printed)
        return 0, [math.nan] * len(thresholds)
    sname = model.stat
    gw = allowed_rows(sname, model.min_count, model.sizes, model.row_off, model.g)
    arg, clr, lin, ns, _, _ = run_replicates(ctx, g[union], lo, hi, g[rows], planted, gw, seed, R, f, background, block)
    sums = write_power(output_name(outfile), col, rows, n_reach(genpos, g[rows], A_plant, zcut), g, union, lo, hi, arg, clr, lin,
                       planted, nx, nab, thresholds)
    if reps:
        write_reps(reps_name(outfile), col, rows, union, arg, clr, lin, ns, *grids_printed)
    mean = []
    for j in range(len(thresholds)):
        v = [s['power'][j] for s in sums if s['n_ok'] >= 2]
        mean.append(float(np.mean(v)) if v else math.nan)
    return len(rows), mean
