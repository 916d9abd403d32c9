"""Forward stepwise conditional selection of loci: the definition behind --stepwise, a plain host restatement, the greedy run, the
writers and the refusals.

What it answers.  --peaks G separates loci by G alone and --conditional holds each apex against ONE parent.  --stepwise asks: which
of the apexes are separate loci?  It accepts the highest apex, recomputes every other apex given all accepted loci, accepts the
best of what is left, and stops when nothing clears a threshold.  The result is the list of conditionally independent loci in
their order of entry, with the log ratio of the whole K-locus model against neutrality.

The baseline.  conditional.py's nested mixture: with baseline d_i a site follows g (1 + d_i).  Accepting a locus with (alpha_i,
R_i) gives (1 - alpha)(1 + d) + alpha (1 + R) = 1 + d + alpha (R - d), so ONE per-site array carries any number of accepted
loci.  Per slot: d[N] (all 0.0 at reset) and cnt[N] (int32, the number of accepted loci that reach the site).

Adding a locus.  A locus is a test site c (position tc, window bounds win_lo[c], win_hi[c]) held at the grid point lin_c = (iA_c *
nx + ix_c) * nab + ia_c.  Its sites are the surfaces' sites at A_c: max(win_lo[c], 0) <= i <= min(win_hi[c], N - 1), z_i = A_c *
|g_i - tc| <= zcut (that single product), g_i != tc.  Each of them gets

    d_i <- d_i + exp(-z_i) * (R[ix_c][ia_c][row_i] - d_i)      (no FMA contraction),     cnt_i <- cnt_i + 1

From d_i = 0.0 that is exp(-z_i) * R bit for bit: conditional.py's d of ONE conditioning locus.

A surface against the baseline.  conditional.host_cond_surface with d_i taken from the array:

    T_base(A, x, abeta) = 2 * sum_i log1p(u_i * (R_i - d_i)),    u_i = exp(-A |g_i - tg|) / (1.0 + d_i)

over the window's sites in increasing site index; NaN where no site qualifies at that A.  nsites[iA] is the surfaces' count,
nshared[iA] the number of those sites with cnt_i > 0.  Non-finite terms propagate as they do there.  Against the empty baseline
it is surfaces.host_surface bit for bit, after one added locus conditional.host_cond_surface of the pair.

The greedy run over the K apexes of the peak call (run()).
  1. cur_T[k], cur_lin[k]: the scan's rule (influence.scan_argmax) on every apex's surface against the empty baseline.
  2. Repeat: among the apexes not yet accepted take the largest cur_T (on an equal value the earlier row; exact FP64).  Stop if
     none has cur_lin >= 0 and cur_T >= C, or if --stepMax loci are in.  Add the apex at cur_lin; recompute cur_T, cur_lin of the
     remaining apexes.  Only those whose widest site range (site_ranges(): at the smallest A of the grid) meets the index range
     just written are recomputed: the baseline of every other apex's sites has not changed, so its numbers are the same bit for
     bit and skipping them changes no byte.
  3. After the last step every apex that was not accepted holds its maximum given ALL accepted loci.

Identity (consequence 2 of conditional.py, telescoped).  A locus' entry maximum is 2 sum_i log((1 + d'_i) / (1 + d_i)) over the
sites its addition writes, so the sum of the accepted loci's entry maxima equals 2 sum_i log1p(d_i) over the chromosome, to
rounding: the log ratio of the K-locus nested mixture against neutrality, reported as T_total.

The device (baseline_add_kernel, base_surfaces_kernel: bmx_ctx_baseline_reset / _add / _fetch, bmx_ctx_base_surfaces) keeps d and
cnt per slot; the loop over the steps is host-driven, one baseline_add plus one base_surfaces over the affected apexes per step.
host_baseline_add() and host_base_surface() below are the numpy restatement.

The CLI (--stepwise [--stepMin C] [--stepMax K] [--stepSurfaces], needs --peaks).  C defaults to --peakMin's value, else 0; K to
1000.  It runs on the observed scan after the peak call, beside --conditional.

Output.  <out>.stepwise.txt, tab-separated, floats as repr, one row per apex in position order: physPos genPos CLR (the main
output's strings), T_max (the maximum of the plain-sum surface), step (the order of acceptance, 1.., NA if not accepted), CLR_cond
x_cond s_cond A_cond nSites_cond nShared (for an accepted apex the values AT ENTRY, for the others the values given all accepted
loci; nSites_cond and nShared at A_cond; 0.0 and NA where nothing is > 0, as in <out>.conditional.txt), retained = CLR_cond /
T_max, T_total (the running sum after that step, NA if not accepted).  A file without peaks gets the header only.  With several
input files also a genome-wide stepwise.txt with a leading `file` column; the selection itself stays per file.  With
--stepSurfaces <out>.stepwise.surfaces.txt: each accepted apex's surface at entry, in the surfaces' format, in order of entry.

What this is not.  It is greedy and order-dependent: no subset search, nothing leaves once in.  Loci are held at GRID points and
never refitted once in.  The nested mixture is asymmetric: a later locus is nested inside the earlier ones, not beside them.
Sites are linked, so C is a threshold and not a test (--nullPerm's genome-wide threshold is the natural C).  It covers the
observed scan only.
"""
import numpy as np

from . import influence, surfaces

HEADER = 'physPos\tgenPos\tCLR\tT_max\tstep\tCLR_cond\tx_cond\ts_cond\tA_cond\tnSites_cond\tnShared\tretained\tT_total\n'
MAX_LOCI = 1000


def value_refusal(min_clr, max_loci):
    """The message that refuses these values of --stepMin / --stepMax, or None."""
    if min_clr is not None and min_clr != min_clr:
        return '--stepMin takes a number.'
    if max_loci is not None and max_loci < 1:
        return '--stepMax takes a number of loci >= 1.'
    return None


# ----------------------------------------------------------------------------------------------- the host restatement

def _locus_sites(g, tc, clo, chi, A_c, zcut):
    """(first index of the clipped window, the mask of the locus' sites inside it)."""
    a, b = max(int(clo), 0), min(int(chi), len(g) - 1)
    if b < a:
        return a, np.zeros(0, dtype=bool)
    gw = g[a:b + 1]
    return a, (A_c * np.abs(gw - tc) <= zcut) & (gw != tc)


def host_baseline_add(d, cnt, genpos, rows, R, tc, clo, chi, A_c, ix_c, ia_c, zcut, scale=None):
    """Add one locus to the baseline d[N], cnt[N] IN PLACE, in numpy.  (tc, clo, chi): the locus' position and inclusive site
    index window; (A_c, ix_c, ia_c): where it is held; R[nx][nab][table rows]; zcut: bmx_alpha_cut().  scale: an array [N] that
    collects |exp(-z) (R - d)| per written site (the sum of a site's absolute increments), or None.
    Returns (first, last, n_written): first > last and 0 when the locus has no site."""
    g = np.asarray(genpos, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.int64)
    a, keep = _locus_sites(g, tc, clo, chi, A_c, zcut)
    idx = a + np.nonzero(keep)[0]
    if not len(idx):
        return a, a - 1, 0
    with np.errstate(over='ignore', invalid='ignore'):
        z = A_c * np.abs(g[idx] - tc)
        inc = np.exp(-z) * (np.asarray(R, dtype=np.float64)[int(ix_c), int(ia_c), rows[idx]] - d[idx])
        if scale is not None:
            scale[idx] += np.abs(inc)
        d[idx] = d[idx] + inc
    cnt[idx] += 1
    return int(idx[0]), int(idx[-1]), len(idx)


def host_base_surface(genpos, rows, R, A, tg, lo, hi, d, cnt, zcut, scale=False):
    """The surface of one window against the baseline (d[N], cnt[N]) in numpy: conditional.host_cond_surface's body
    (surfaces.host_sided_surface) with d_i read from the array and `shared` meaning cnt_i > 0.  Returns (T[nA][nx][nab], NaN where no site qualifies; nsites[nA]; nshared[nA]) and
    with scale=True also S[nA][nx][nab] = 2 sum_i |term_i|."""
    side = lambda a, b, gw, rw, R: (np.asarray(d, dtype=np.float64)[a:b + 1], np.asarray(cnt)[a:b + 1] > 0)
    return surfaces.host_sided_surface(genpos, rows, R, A, tg, lo, hi, side, zcut, scale)


def site_ranges(genpos, tg, lo, hi, A_min, zcut):
    """Per window its widest site range: the first and last site index i of the clipped window with A_min * |g_i - tg| <= zcut
    (first > last: none).  genpos ascends; A_min is the smallest A of the grid.  int64[n] each."""
    g = np.asarray(genpos, dtype=np.float64)
    tg, lo, hi = np.atleast_1d(np.asarray(tg, dtype=np.float64)), np.atleast_1d(lo), np.atleast_1d(hi)
    first, last = np.zeros(len(tg), dtype=np.int64), np.full(len(tg), -1, dtype=np.int64)
    reach = zcut / A_min
    ok = lambda i, t: A_min * abs(float(g[i]) - t) <= zcut
    for k, t in enumerate(tg.tolist()):
        a, b = max(int(lo[k]), 0), min(int(hi[k]), len(g) - 1)
        if b < a:
            first[k], last[k] = a, a - 1
            continue
        i = min(max(int(np.searchsorted(g, t - reach, side='left')), a), b)        # near the left end: settle it with the exact predicate
        while i > a and ok(i - 1, t):
            i -= 1
        while i <= b and not ok(i, t):
            i += 1
        j = min(max(int(np.searchsorted(g, t + reach, side='right')) - 1, a), b)
        while j < b and ok(j + 1, t):
            j += 1
        while j >= a and not ok(j, t):
            j -= 1
        first[k], last[k] = (i, j) if i <= j else (a, a - 1)
    return first, last


# ------------------------------------------------------------------------------------------------------ the greedy run

def run(K, evaluate, add, ranges, min_clr=0.0, max_loci=MAX_LOCI, skip=True, watch=None):
    """The greedy run of the definition over K apexes (places 0 .. K - 1, in row order).
    evaluate(places) -> dict with tmax f64[n], lin i32[n], nsites i32[n][nA], nshared i32[n][nA] (and whatever else: T) of the
    listed places against the current baseline; add(place, lin) -> (first, last, n_written) adds that apex at lin;
    ranges = (first[K], last[K]): site_ranges() of the apexes.
    skip=False recomputes every remaining apex at every step (the brute form: the same bytes).  watch(step, places, res, cur_T,
    accepted) is called after every evaluation (step 0: the first), before the next choice.
    Returns a dict: T_max f64[K], step i32[K] (0: not accepted), T f64[K], lin i32[K], nsites i32[K][nA] and nshared i32[K][nA]
    (an accepted apex's at entry, the others' given all accepted loci), T_total f64[K] (NaN: not accepted), order (the accepted
    places), written ((first, last, n) per step), evals (surfaces computed)."""
    K = int(K)
    every = np.arange(K, dtype=np.int64)
    res = evaluate(every)
    cur_T, cur_lin = np.array(res['tmax'], dtype=np.float64), np.array(res['lin'], dtype=np.int32)
    ns, nsh = np.array(res['nsites'], dtype=np.int32), np.array(res['nshared'], dtype=np.int32)
    out = {'T_max': cur_T.copy(), 'step': np.zeros(K, dtype=np.int32), 'T_total': np.full(K, np.nan), 'order': [], 'written': [],
           'evals': K}
    accepted = np.zeros(K, dtype=bool)
    if watch is not None:
        watch(0, every, res, cur_T, accepted)
    first, last = ranges
    total = 0.0
    while len(out['order']) < max_loci:
        can = ~accepted & (cur_lin >= 0) & (cur_T >= min_clr)
        if not can.any():
            break
        k = int(np.argmax(np.where(can, cur_T, -np.inf)))          # the first maximum: the earlier row on an equal value
        accepted[k] = True
        out['order'].append(k)
        out['step'][k] = len(out['order'])
        total = total + float(cur_T[k])
        out['T_total'][k] = total
        w = add(k, int(cur_lin[k]))
        out['written'].append(tuple(int(v) for v in w))
        rest = ~accepted
        if skip:
            rest &= (first <= w[1]) & (last >= w[0]) if w[2] > 0 else False
        places = np.nonzero(rest)[0]
        if len(places):
            res = evaluate(places)
            cur_T[places], cur_lin[places] = res['tmax'], res['lin']
            ns[places], nsh[places] = res['nsites'], res['nshared']
            out['evals'] += len(places)
        if watch is not None:
            watch(len(out['order']), places, res if len(places) else None, cur_T, accepted)
    out.update(T=cur_T, lin=cur_lin, nsites=ns, nshared=nsh)
    return out


def host_run(genpos, rows, R, A, tg, lo, hi, zcut, min_clr=0.0, max_loci=MAX_LOCI, skip=True, watch=None, keep_T=False):
    """run() on the host restatement: the apexes are the windows (tg[k], lo[k], hi[k]), R[nx][nab][table rows], A the grid in scan
    order.  Returns run()'s dict with d, cnt (the final baseline) and, with keep_T, entry_T: each accepted apex's surface at
    entry, in order."""
    g = np.asarray(genpos, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    nx, nab = R.shape[:2]
    d, cnt = np.zeros(len(g)), np.zeros(len(g), dtype=np.int32)
    last_T = {}

    def evaluate(places):
        n = len(places)
        out = {'tmax': np.zeros(n), 'lin': np.zeros(n, dtype=np.int32), 'nsites': np.zeros((n, len(A)), dtype=np.int32),
               'nshared': np.zeros((n, len(A)), dtype=np.int32), 'T': np.zeros((n, len(A), nx, nab))}
        for q, k in enumerate(np.asarray(places).tolist()):
            T, ns, nsh = host_base_surface(g, rows, R, A, tg[k], lo[k], hi[k], d, cnt, zcut)
            out['T'][q], out['nsites'][q], out['nshared'][q] = T, ns, nsh
            out['tmax'][q], out['lin'][q] = influence.scan_argmax(T)[:2]
            if keep_T:
                last_T[k] = T
        return out

    entry_T = []

    def add(k, lin):
        if keep_T:
            entry_T.append(last_T[k])
        return host_baseline_add(d, cnt, g, rows, R, tg[k], lo[k], hi[k], A[lin // (nx * nab)], (lin // nab) % nx, lin % nab, zcut)

    ranges = site_ranges(g, tg, lo, hi, float(A.min()), zcut) if len(A) else (np.zeros(len(tg), dtype=np.int64),) * 2
    out = run(len(tg), evaluate, add, ranges, min_clr, max_loci, skip, watch)
    out.update(d=d, cnt=cnt)
    if keep_T:
        out['entry_T'] = entry_T
    return out


def device_run(ctx, apex_rows, ranges, min_clr=0.0, max_loci=MAX_LOCI, skip=True, entry=None):
    """run() on ctx's selected slot: baseline_reset, then per step one baseline_add and one base_surfaces over the affected
    apexes; no surface is copied back.  apex_rows: the test sites of the apexes, in row order.  entry: called as
    entry(place, lin) just before an apex is added (the CLI fetches --stepSurfaces' surface there)."""
    apex = np.asarray(apex_rows, dtype=np.int32)
    ctx.baseline_reset()

    def add(k, lin):
        if entry is not None:
            entry(k, lin)
        return ctx.baseline_add(int(apex[k]), lin)

    return run(len(apex), lambda places: ctx.base_surfaces(apex[places], want_T=False), add, ranges, min_clr, max_loci, skip)


# ---------------------------------------------------------------------------------------------------------- output

def output_name(outfile):
    return outfile + '.stepwise.txt'


def surfaces_name(outfile):
    return outfile + '.stepwise.surfaces.txt'


_num = influence._num
read_table = influence.read_table


def table_rows(phys, gen, clr, out, sel):
    """The rows of <out>.stepwise.txt.  phys, gen, clr: the main output's strings of every apex (in row order); out: run()'s
    dict; sel: the run's NormalizedBetaBinom (the grids in scan order)."""
    npairs = len(sel.grid_x) * len(sel.grid_abeta)
    rows = []
    for k in range(len(phys)):
        T_max, v, l, step = float(out['T_max'][k]), float(out['T'][k]), int(out['lin'][k]), int(out['step'][k])
        iA = l // npairs if l >= 0 else -1
        cols = [phys[k], gen[k], clr[k], repr(T_max), _num(step if step else None), repr(v)] + list(influence.grid_strings(l, sel))
        cols += [_num(int(out['nsites'][k][iA]) if l >= 0 else None), _num(int(out['nshared'][k][iA]) if l >= 0 else None),
                 _num(v / T_max if T_max > 0 else None), _num(float(out['T_total'][k]) if step else None)]
        rows.append('\t'.join(cols) + '\n')
    return rows


def write_table(path, rows):
    with open(path, 'w') as f:
        f.write(HEADER)
        f.writelines(rows)


def write_genome(path, per_file):
    """The genome-wide table of a run over several files.  per_file: (input basename, that file's rows as written).  Every
    file's rows in file order with a leading `file` column; the selection itself is per file."""
    with open(path, 'w') as f:
        f.write('file\t' + HEADER)
        for name, rows in per_file:
            f.writelines([name + '\t' + r for r in rows])


def stepwise_and_write(ctx, outfile, ts, sel, genpos, apex_rows, min_clr=0.0, max_loci=MAX_LOCI, with_surfaces=False):
    """After the observed scan of one file on ctx's selected slot and its peak call (apex_rows): the greedy run on the device and
    <outfile>.stepwise.txt (with_surfaces: also <outfile>.stepwise.surfaces.txt, each accepted apex's surface at entry, written
    as it is fetched).  genpos: the file's site positions as the slot holds them; sel: the run's NormalizedBetaBinom (the grids
    in scan order).  No surface is copied to the host without with_surfaces.
    Returns (the rows written, loci accepted, the final T_total (0.0 without a locus))."""
    apex = np.asarray(apex_rows, dtype=np.int64)
    rows, out = [], {'order': [], 'T_total': np.zeros(0)}
    f = None
    try:
        if with_surfaces:
            f = open(surfaces_name(outfile), 'w')
            f.write(surfaces.HEADER)
        if len(ts) and len(apex):
            clr = ctx.fetch()[0]
            zcut = float(ctx._L.bmx_alpha_cut())
            A_min = min(float(v) for v in sel.grid_A)
            ranges = site_ranges(genpos, np.asarray(ts.test_gen)[apex], np.asarray(ts.lo)[apex], np.asarray(ts.hi)[apex], A_min, zcut)
            phys, gen = surfaces.labels(ts, apex.tolist())
            entry = None
            if with_surfaces:
                layout = surfaces.Layout(sel.grid_A, sel.grid_x, sel.grid_abeta)

                def entry(k, lin):          # the baseline has not moved since this apex was last evaluated: its surface at entry
                    r = ctx.base_surfaces([int(apex[k])])
                    surfaces.write_blocks(f, layout, [phys[k]], [gen[k]], r['T'], r['nsites'])
            out = device_run(ctx, apex, ranges, min_clr, max_loci, entry=entry)
            rows = table_rows(phys, gen, [repr(float(v)) for v in clr[apex]], out, sel)
    finally:
        if f is not None:
            f.close()
    write_table(output_name(outfile), rows)
    total = float(out['T_total'][out['order'][-1]]) if out['order'] else 0.0
    return rows, len(out['order']), total
