"""Goodness of fit of each selected window: the observed frequency spectrum by distance from the test position against the
counts the fitted mixture and neutrality expect.  The definition behind --fit, a plain host restatement, the per-window
summary, and the writers.

What it answers.  Every other layer takes the fitted mixture at its word.  --fit asks whether the model the argmax names
describes the window's data: under alpha = exp(-A d) the excess of some frequency classes decays with distance.  A high CLR
whose spectrum does not decay that way is the signature of an artefact (a collapsed duplication, a run of mis-polarised sites, a
missing-data pattern); a peak whose observed spectrum follows the fitted curve bin by bin is a different finding.

Inputs of one window.  Test site t of the selected slot (tg, win_lo, win_hi, clipped to the chromosome) and ONE grid point
lin = (iA * nx + ix) * nab + ia (the CLI: the window's scan argmax).  A = the grid's A[iA], R = the selection table's column
R[ix][ia][:], zcut = bmx_alpha_cut().

Qualifying sites.  Exactly the surfaces' sites at that A: lo <= i <= hi, z_i = A * |g_i - tg| <= zcut, g_i != tg.  z_i is that
single product (no contraction), the expression the cut uses.

Per-row arrays over the table rows.  gw[rows] = power.allowed_rows(): the neutral probability of every admissible (count,
sample size), 0 elsewhere.  cls[rows] in [0, F) = classes(): the frequency class of the row -- for the row with local count k of
a size block of sample size n, min(F - 1, (k * F) // n) in integer arithmetic (k = n goes to the last class); B1 has two rows
per size (0 substitution, 1 polymorphism) and the class is k (F >= 2).

Distance bins.  edges[D - 1] strictly ascending, finite, > 0; bin(z) = #{k : z > edges[k]}: a site exactly on an edge belongs
to the lower bin, as the inclusive cut does; the last bin runs to the cut.  The CLI's default_edges(): D = 8, edges[k] =
(k + 1) * (zcut / 8), about one bin per decade of alpha.

Predictive distributions of a site of size block j (rows a..b) with alpha = exp(-z):
    m_r = gw[r] * (1 + alpha * R[r]) where gw[r] > 0, and 0 where gw[r] == 0 (the product is not formed there: R is NaN where g
          is); a non-finite m_r counts as 0
    tot = sum_r m_r in ascending r,  p_r = m_r / tot                      (the fitted mixture)
    q_r = gw[r] / sum_{a..b} gw                                          (neutrality)
A site whose tot, or whose neutral total, is not finite and > 0 is SKIPPED: it is counted in O and in the window's nSkipped and
adds nothing to either E.

Outputs per window, [D][F] each.  O (int32): the qualifying sites per (bin, class of the site's own row).  E_sel = sum over the
bin's sites of sum_{r in class} p_r.  E_neu = the same of q_r.  lin < 0: O all 0 and both E NaN.  So sum_c O[d] = n_d, the bin's
sites, and sum_c E[d] = n_d minus the bin's skipped sites, to rounding.

Device (fit_kernel, bmx_ctx_fit; include/bmxscan.h).  One workgroup per listed window, no atomics.  With 0 <= gw <= 1 (anything
else is refused), R >= -1 and 1e-8 <= alpha <= 1 a product m_r is non-finite exactly where R[r] is, for every site alike, and
the class sums are linear in alpha: the kernel sums gw and gw R per (size block, class) once per window and adds (Gs + alpha H) /
tot per site and cell.  host_fit() below is the plain per-site restatement the tests compare it with: O and nSkipped exactly, E
within 1e-12 * max(1, n_d) per cell.

Summary of a window (summarise(), for each of the two models independently; E = that model's expected counts).  Cells with
E >= --fitMinExp (default 5) are used.  The other cells of a bin are pooled into ONE rest cell of that bin (their O and E added);
the rest cell is used if its E >= --fitMinExp and dropped otherwise.  X2 = sum over the used cells of (O - E)^2 / E; df = used
cells - bins with a used cell (each bin's total is fixed).  nPooled = the bins whose rest cell holds a site or expectation and
was dropped under the FITTED model.  worst_bin, worst_class, worst_resid: the used cell of the fitted model with the largest
absolute Pearson residual (O - E) / sqrt(E) (the earlier cell on a tie; class `rest` for a rest cell) and that residual, signed.
A model without a used cell prints NA for its X2 and df; when the fitted model has none, everything from X2_sel on is NA.

What this is not.  Sites are linked, so X2 is a descriptive statistic, not a calibrated test; df ignores the three fitted
parameters; the fitted point is the GRID argmax of the scan, not the refined one; and the table covers the observed scan only
(no null replicate, no refinement).

Selection.  As --surfaces selects (surfaces.select): --fitMin C, with --peaks only the apexes, at most --fitMax N.

Output.  <out>.fit.txt, tab-separated, floats as repr, one row per selected window in the main output's order:
physPos genPos CLR x_hat s_hat A_hat nSites nSkipped X2_sel df_sel X2_neu df_neu nPooled worst_bin worst_class worst_resid.
With --fitDetail <out>.fit.cells.txt: physPos genPos bin z_lo z_hi class O E_sel E_neu, every cell of every selected window
(z_lo, z_hi: the bin's ends in z, 0 and zcut at the two ends).
"""
import math

import numpy as np

from . import influence, power, surfaces

HEADER = ('physPos\tgenPos\tCLR\tx_hat\ts_hat\tA_hat\tnSites\tnSkipped\tX2_sel\tdf_sel\tX2_neu\tdf_neu\tnPooled\tworst_bin\t'
          'worst_class\tworst_resid\n')
CELLS_HEADER = 'physPos\tgenPos\tbin\tz_lo\tz_hi\tclass\tO\tE_sel\tE_neu\n'
MAX_WINDOWS = surfaces.MAX_WINDOWS
MAX_CELLS = 256                 # BMX_FIT_MAX_CELLS: D * F
BINS, CLASSES, MIN_EXP = 8, 10, 5.0
HOST_WINDOWS = 1 << 14          # the writer asks for at most this many windows at a time


def value_refusal(bins, classes, min_clr, max_n, min_exp, b1=False):
    """The message that refuses these values of --fitBins / --fitClasses / --fitMin / --fitMax / --fitMinExp (None: the flag was
    not given), or None.  b1: the run's statistic is B1 (--noFreq), whose two rows per size need two classes."""
    D, F = BINS if bins is None else bins, CLASSES if classes is None else classes
    if D < 1:
        return '--fitBins takes a number of distance bins >= 1.'
    if F < 1:
        return '--fitClasses takes a number of frequency classes >= 1.'
    if b1 and F < 2:
        return '--fitClasses must be >= 2 with --noFreq: its two rows per sample size are the classes 0 and 1.'
    if D * F > MAX_CELLS:
        return '--fitBins times --fitClasses must be <= %d.' % MAX_CELLS
    if max_n is not None and max_n < 1:
        return '--fitMax takes a number of windows >= 1.'
    if min_clr is not None and min_clr != min_clr:
        return '--fitMin takes a number.'
    if min_exp is not None and not (math.isfinite(min_exp) and min_exp > 0.0):
        return '--fitMinExp takes a finite expected count > 0.'
    return None


def classes(stat, sizes, row_off, F):
    """cls[rows]: the frequency class of every table row.  Row k of the size block of sample size n: min(F - 1, (k * F) // n);
    B1 (two rows per size): k, which needs F >= 2."""
    F = int(F)
    if F < 1 or (stat == 'B1' and F < 2):
        raise ValueError('F >= 1 classes are needed (B1: F >= 2)')
    off = np.asarray(row_off, dtype=np.int64)
    cls = np.zeros(int(off[-1]), dtype=np.int32)
    for j, n in enumerate(np.asarray(sizes).tolist()):
        k = np.arange(int(off[j + 1] - off[j]), dtype=np.int64)
        cls[off[j]:off[j + 1]] = k if stat == 'B1' else np.minimum(F - 1, (k * F) // max(int(n), 1))
    return cls


def default_edges(D, zcut=power.ALPHA_CUT):
    """edges[k] = (k + 1) * (zcut / D), k = 0 .. D - 2."""
    return np.array([(k + 1) * (zcut / D) for k in range(int(D) - 1)], dtype=np.float64)


def check_edges(edges):
    e = np.asarray(edges, dtype=np.float64)
    if e.ndim != 1 or not np.all(np.isfinite(e)) or not np.all(e > 0.0) or not np.all(np.diff(e) > 0.0):
        raise ValueError('the edges must be a flat list of finite values > 0, strictly ascending')
    return e


# ----------------------------------------------------------------------------------------------- the host restatement

def qualifying(genpos, A, tg, lo, hi, zcut):
    """(site indices, z) of the window's qualifying sites at A, in increasing site index."""
    g = np.asarray(genpos, dtype=np.float64)
    a, b = max(int(lo), 0), min(int(hi), len(g) - 1)
    if b < a:
        return np.zeros(0, dtype=np.int64), np.zeros(0)
    gw_ = g[a:b + 1]
    z = float(A) * np.abs(gw_ - tg)
    keep = (z <= zcut) & (gw_ != tg)
    return a + np.nonzero(keep)[0].astype(np.int64), z[keep]


def host_fit(genpos, rows, row_off, R, gw, cls, F, edges, A, ix, ia, tg, lo, hi, zcut, dtype=np.float64):
    """The table of one window in numpy: per site the sums over the rows of its size, as power.planted_rows forms them.
    genpos[N], rows[N]: position and table row of every site; row_off[n_sizes + 1]; R[nx][nab][table rows] (Context.fetch_lut's
    R); gw, cls: the per-row arrays; edges[D - 1]; (A, ix, ia): the grid point; (tg, lo, hi): the window; zcut:
    bmx_alpha_cut().  dtype: the arithmetic of the expected counts (np.longdouble: the tests' check of the conditioning; the
    cut, the bins and the exponent's argument stay float64).  Returns (O int32[D][F], E_sel[D][F], E_neu[D][F], skipped)."""
    rows = np.asarray(rows, dtype=np.int64)
    off = np.asarray(row_off, dtype=np.int64)
    gw, cls = np.asarray(gw, dtype=np.float64), np.asarray(cls, dtype=np.int64)
    edges = check_edges(edges)
    F, D = int(F), len(edges) + 1
    Rs = np.asarray(R, dtype=np.float64)[ix, ia]
    O = np.zeros((D, F), dtype=np.int32)
    Es, En = np.zeros((D, F), dtype=dtype), np.zeros((D, F), dtype=dtype)
    idx, z = qualifying(genpos, A, tg, lo, hi, zcut)
    if not len(idx):
        return O, Es, En, 0
    bins = np.searchsorted(edges, z, side='left')                  # the number of edges below z
    np.add.at(O, (bins, cls[rows[idx]]), 1)
    block = np.searchsorted(off, rows[idx], side='right') - 1     # the size block of every site
    skipped = 0
    for j in np.unique(block).tolist():
        at = block == j
        a, b = int(off[j]), int(off[j + 1])
        alpha = np.exp(-(z[at].astype(dtype)))
        w = gw[a:b].astype(dtype)
        adm = gw[a:b] > 0.0
        Rj = np.where(adm, Rs[a:b], 0.0).astype(dtype)             # the product is not formed where gw == 0
        with np.errstate(invalid='ignore', over='ignore'):
            m = np.where(adm[None, :], w[None, :] * (1 + alpha[:, None] * Rj[None, :]), 0)
            m = np.where(np.isfinite(m), m, 0)
        tot = np.cumsum(m, axis=1)[:, -1]                          # sequential, ascending r
        neu = np.cumsum(w)[-1]
        ok = np.isfinite(tot) & (tot > 0) & bool(np.isfinite(neu) and neu > 0)
        skipped += int(np.count_nonzero(~ok))
        if not ok.any():
            continue
        p = m[ok] / tot[ok][:, None]
        q = w / neu
        bj = bins[at][ok]
        for c in np.unique(cls[a:b]).tolist():
            of = cls[a:b] == c
            np.add.at(Es[:, c], bj, np.cumsum(p[:, of], axis=1)[:, -1])
            np.add.at(En[:, c], bj, np.full(len(bj), np.cumsum(q[of])[-1], dtype=dtype))
    return O, Es, En, skipped


# ------------------------------------------------------------------------------------------------------------ summary

def chi_square(O, E, min_exp=MIN_EXP):
    """The summary rule on one model's table: O[D][F], E[D][F].  Returns a dict: X2 and df (None without a used cell), used (the
    used cells as (bin, class, O, E), class F: the bin's rest cell, in bin-major order), dropped (the bins whose rest cell holds
    a site or expectation and was dropped)."""
    O, E = np.asarray(O, dtype=np.float64), np.asarray(E, dtype=np.float64)
    D, F = O.shape
    used, dropped, bins_used = [], 0, 0
    for d in range(D):
        n0 = len(used)
        big = E[d] >= min_exp                                       # False for NaN
        for c in np.nonzero(big)[0].tolist():
            used.append((d, c, float(O[d, c]), float(E[d, c])))
        ro, re = float(O[d][~big].sum()), float(np.nansum(E[d][~big]))
        if re >= min_exp:
            used.append((d, F, ro, re))
        elif ro > 0 or re > 0:
            dropped += 1
        bins_used += len(used) > n0
    if not used:
        return {'X2': None, 'df': None, 'used': used, 'dropped': dropped}
    X2 = 0.0
    for _, _, o, e in used:
        X2 += (o - e) ** 2 / e
    return {'X2': X2, 'df': len(used) - bins_used, 'used': used, 'dropped': dropped}


def summarise(O, E_sel, E_neu, min_exp=MIN_EXP):
    """The per-window numbers of the definition: {'nSites', 'X2_sel', 'df_sel', 'X2_neu', 'df_neu', 'nPooled', 'worst_bin',
    'worst_class' (F: a rest cell), 'worst_resid'}; None where the definition says NA."""
    sel, neu = chi_square(O, E_sel, min_exp), chi_square(O, E_neu, min_exp)
    out = {'nSites': int(np.asarray(O).sum()), 'X2_sel': sel['X2'], 'df_sel': sel['df'], 'X2_neu': None, 'df_neu': None,
           'nPooled': None, 'worst_bin': None, 'worst_class': None, 'worst_resid': None}
    if sel['X2'] is None:
        return out
    best = None
    for d, c, o, e in sel['used']:
        r = (o - e) / math.sqrt(e)
        if best is None or abs(r) > abs(best[2]):
            best = (d, c, r)
    out.update(X2_neu=neu['X2'], df_neu=neu['df'], nPooled=sel['dropped'], worst_bin=best[0], worst_class=best[1], worst_resid=best[2])
    return out


# ---------------------------------------------------------------------------------------------------------- output

def output_name(outfile):
    return outfile + '.fit.txt'


def cells_name(outfile):
    return outfile + '.fit.cells.txt'


_num = influence._num


def summary_row(phys, gen, clr, grid, skipped, s, F):
    """One row of <out>.fit.txt: (phys, gen, clr) the main output's strings, grid = influence.grid_strings() of the window's
    grid point, s = summarise()'s dict."""
    wc = None if s['worst_class'] is None else ('rest' if s['worst_class'] == F else str(int(s['worst_class'])))
    cols = [phys, gen, clr] + list(grid) + [str(int(s['nSites'])), str(int(skipped))]
    cols += [_num(s[k]) for k in ('X2_sel', 'df_sel', 'X2_neu', 'df_neu', 'nPooled', 'worst_bin')]
    return '\t'.join(cols + ['NA' if wc is None else wc, _num(s['worst_resid'])]) + '\n'


def cell_rows(phys, gen, O, E_sel, E_neu, edges, zcut):
    """The rows of <out>.fit.cells.txt of one window: every cell, bin-major."""
    D, F = np.asarray(O).shape
    ends = [0.0] + [float(e) for e in edges] + [float(zcut)]
    out = []
    for d in range(D):
        head = '\t'.join([phys, gen, str(d), repr(ends[d]), repr(ends[d + 1])])
        for c in range(F):
            out.append('%s\t%d\t%d\t%s\t%s\n' % (head, c, int(O[d][c]), _num(float(E_sel[d][c])), _num(float(E_neu[d][c]))))
    return out


read_table = influence.read_table


def read_cells(path, D, F):
    """A cells file back: (physPos strings, genPos strings, O int32[n][D][F], E_sel[n][D][F], E_neu[n][D][F]) (NA: NaN)."""
    names, rows = read_table(path)
    assert '\t'.join(names) + '\n' == CELLS_HEADER
    n = len(rows) // (D * F) if D * F else 0
    val = lambda v: float('nan') if v == 'NA' else float(v)
    O = np.array([int(r[6]) for r in rows], dtype=np.int32).reshape(n, D, F)
    Es = np.array([val(r[7]) for r in rows], dtype=np.float64).reshape(n, D, F)
    En = np.array([val(r[8]) for r in rows], dtype=np.float64).reshape(n, D, F)
    first = rows[::D * F]
    return [r[0] for r in first], [r[1] for r in first], O, Es, En


def write_fit(outfile, phys, gen, clr, lin, sel, O, E_sel, E_neu, skipped, edges, zcut, min_exp=MIN_EXP, detail=False):
    """Both files from arrays held on the host (the tests' entry point; fit_and_write's inner step): one window per entry of
    phys / gen / clr (the main output's strings) / lin / O / E_sel / E_neu / skipped.  sel: the run's NormalizedBetaBinom (the
    grids in scan order)."""
    with open(output_name(outfile), 'w') as f:
        f.write(HEADER)
        _append(f, None, phys, gen, clr, lin, sel, O, E_sel, E_neu, skipped, edges, zcut, min_exp)
    if detail:
        with open(cells_name(outfile), 'w') as fc:
            fc.write(CELLS_HEADER)
            _append(None, fc, phys, gen, clr, lin, sel, O, E_sel, E_neu, skipped, edges, zcut, min_exp)


def _append(f, fc, phys, gen, clr, lin, sel, O, E_sel, E_neu, skipped, edges, zcut, min_exp):
    F = np.asarray(O).shape[2] if len(phys) else 0
    for w in range(len(phys)):
        if f:
            s = summarise(O[w], E_sel[w], E_neu[w], min_exp)
            f.write(summary_row(phys[w], gen[w], clr[w], influence.grid_strings(int(lin[w]), sel), skipped[w], s, F))
        if fc:
            fc.writelines(cell_rows(phys[w], gen[w], O[w], E_sel[w], E_neu[w], edges, zcut))


def fit_and_write(ctx, outfile, ts, sel, bins=BINS, n_classes=CLASSES, min_clr=0.0, max_n=MAX_WINDOWS, min_exp=MIN_EXP,
                  apex_rows=None, detail=False, host_windows=HOST_WINDOWS):
    """After the observed scan of one file on ctx's selected slot (and its peak call, if any): select the windows as --surfaces
    does, compute each one's table at its scan argmax and write <outfile>.fit.txt (detail: also <outfile>.fit.cells.txt).  sel:
    the run's NormalizedBetaBinom (its model and the grids in scan order).  The windows go to the device host_windows at a time,
    each batch written before the next is computed.  Returns (windows written, windows the cap dropped)."""
    model = sel.model
    nx, nab = len(model.x), len(model.abeta)
    zcut = ctx._L.bmx_alpha_cut()
    edges = default_edges(bins, zcut)
    rows, dropped = np.zeros(0, dtype=np.int64), 0
    clr = lin = np.zeros(0)
    if len(ts):
        clr, ix, ia, iA, _ = ctx.fetch()
        lin = np.where(iA >= 0, (iA.astype(np.int64) * nx + ix) * nab + ia, -1).astype(np.int32)
        rows, dropped = surfaces.select(clr, iA, min_clr, apex_rows, max_n)
    gw = power.allowed_rows(model.stat, model.min_count, model.sizes, model.row_off, model.g)
    cls = classes(model.stat, model.sizes, model.row_off, n_classes)
    fc = open(cells_name(outfile), 'w') if detail else None
    try:
        with open(output_name(outfile), 'w') as f:
            f.write(HEADER)
            if fc:
                fc.write(CELLS_HEADER)
            for k in range(0, len(rows), int(host_windows)):
                part = rows[k:k + int(host_windows)]
                O, Es, En, skipped = ctx.fit(part, lin[part], gw, cls, n_classes, edges)
                phys, gen = surfaces.labels(ts, part.tolist())
                _append(f, fc, phys, gen, [repr(float(v)) for v in clr[part]], lin[part], sel, O, Es, En, skipped, edges, zcut, min_exp)
    finally:
        if fc:
            fc.close()
    return len(rows), dropped
