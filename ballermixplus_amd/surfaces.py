"""Likelihood surfaces of selected windows: the definition behind --surfaces, a plain host restatement, the selection
rule and the writer.

Surface.  For one window (test position tg, site indices [win_lo, win_hi]) and every grid point (A, x, alpha_beta):

    T = 2 * sum_i log1p(alpha_i * R_i)     over the sites i with A * |g_i - tg| <= zcut and g_i != tg, in site order
    alpha_i = exp(-A * |g_i - tg|),  R_i = the selection table's entry of site i's (k, n) row at (x, alpha_beta)

NaN where no site qualifies at that A (the reference skips such an A, BalLeRMix+_v1.py:458-459); nSites is the number of
qualifying sites at that A.  This is the quantity the scan maximises, written as a plain sum of logs: the scan's kernels
multiply the factors instead, so the largest T of a surface agrees with the CLR column to rounding, not bit for bit.  The
device (surfaces_kernel, bmx_ctx_surfaces) computes the surfaces of a list of windows in one launch, each bitwise what
bmx_ctx_surface returns for that window; host_surface() below is the numpy restatement the tests compare both with.
The surface holds the grid's points only: it is the scan's own search space made visible, not a finer one, and it covers
the observed scan only (no null replicate, no refinement).

Selection (--surfaces [--surfaceMin C] [--surfaceMax N]).  The rows of the observed scan that have a grid result and
CLR >= C (default 0); with --peaks only the apexes among them; if more than N (default 1000) remain, the N with the highest
CLR are kept -- the earlier row wins a tie -- and the run says how many were dropped.  The kept rows are written in the
order of the main output.

Output.  <out>.surfaces.txt, tab-separated, header physPos genPos A x abeta T nSites: per selected window a block of
nA * nx * nab rows with A, then x, then abeta ascending; physPos, genPos and the grid values as the main output prints
them, T as repr (NA where NaN), nSites the window size at that A.  A run without a selected window writes the header only.
"""
import numpy as np

HEADER = 'physPos\tgenPos\tA\tx\tabeta\tT\tnSites\n'
MAX_WINDOWS = 1000
HOST_BYTES = 1 << 30            # the writer asks for at most this many bytes of surfaces at a time


def value_refusal(min_clr, max_n):
    """The message that refuses these values of --surfaceMin / --surfaceMax, or None."""
    if min_clr is not None and min_clr != min_clr:
        return '--surfaceMin takes a number.'
    if max_n is not None and max_n < 1:
        return '--surfaceMax takes a number of windows >= 1.'
    return None


def select(clr, lin, min_clr=0.0, apex_rows=None, max_n=MAX_WINDOWS):
    """The selection rule on one file's scan: clr[M], lin[M] (any array that is negative where the row has no grid result:
    the linear grid index, or iA), apex_rows = the rows of the peak call (None: no --peaks).  Returns (the selected rows,
    ascending int64; the number of rows the cap dropped)."""
    clr = np.asarray(clr, dtype=np.float64)
    ok = (np.asarray(lin) >= 0) & (clr >= min_clr)
    if apex_rows is not None:
        apex = np.zeros(len(clr), dtype=bool)
        apex[np.asarray(apex_rows, dtype=np.int64)] = True
        ok &= apex
    rows = np.nonzero(ok)[0].astype(np.int64)
    dropped = max(0, len(rows) - int(max_n))
    if dropped:
        keep = np.lexsort((rows, -clr[rows]))[:int(max_n)]         # CLR descending, the earlier row first among equals
        rows = np.sort(rows[keep])
    return rows, dropped


# ----------------------------------------------------------------------------------------------- the host restatement

def host_surface(genpos, rows, R, A, tg, lo, hi, zcut):
    """The surface of one window in numpy.  genpos[N], rows[N]: position and table row of every site; R[nx][nab][table rows]
    (Context.fetch_lut's R); A: the grid of A values in the order wanted; tg, lo, hi: test position and inclusive site
    index window; zcut: bmx_alpha_cut().  Returns (T[nA][nx][nab], NaN where no site qualifies; nsites[nA])."""
    g = np.asarray(genpos, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.int64)
    R = np.asarray(R, dtype=np.float64)
    A = np.atleast_1d(np.asarray(A, dtype=np.float64))
    a, b = max(int(lo), 0), min(int(hi), len(g) - 1)
    T = np.full((len(A),) + R.shape[:2], np.nan)
    ns = np.zeros(len(A), dtype=np.int32)
    if b < a:
        return T, ns
    gw, rw = g[a:b + 1], rows[a:b + 1]
    dist = np.abs(gw - tg)
    for i, Av in enumerate(A.tolist()):
        z = Av * dist
        keep = (z <= zcut) & (gw != tg)
        ns[i] = int(keep.sum())
        if ns[i]:
            with np.errstate(divide='ignore', invalid='ignore'):
                T[i] = 2.0 * np.sum(np.log1p(np.exp(-z[keep]) * R[:, :, rw[keep]]), axis=2)
    return T, ns


def host_sided_surface(genpos, rows, R, A, tg, lo, hi, side, zcut, scale=False):
    """The surface of one window whose sites follow g (1 + d_i) instead of neutrality, in numpy: the body that
    conditional.host_cond_surface and stepwise.host_base_surface share (the definitions are theirs).  host_surface's arguments,
    and side(a, b, gw, rw, R) -> (d f64[b - a + 1], shared bool[b - a + 1]) of the sites a .. b of the clipped window (gw, rw:
    their positions and table rows).  T = 2 sum_i log1p(u_i (R_i - d_i)), u_i = alpha_i / (1.0 + d_i), over host_surface's sites.
    Returns (T[nA][nx][nab], NaN where no site qualifies; nsites[nA]; nshared[nA]: the shared sites among them) and with
    scale=True also S[nA][nx][nab] = 2 sum_i |term_i| (0 where no site qualifies): the size of what cancels in T."""
    g = np.asarray(genpos, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.int64)
    R = np.asarray(R, dtype=np.float64)
    A = np.atleast_1d(np.asarray(A, dtype=np.float64))
    a, b = max(int(lo), 0), min(int(hi), len(g) - 1)
    T = np.full((len(A),) + R.shape[:2], np.nan)
    S = np.zeros(T.shape)
    ns, nsh = np.zeros(len(A), dtype=np.int32), np.zeros(len(A), dtype=np.int32)
    if b >= a:
        gw, rw = g[a:b + 1], rows[a:b + 1]
        d, shared = side(a, b, gw, rw, R)
        dist = np.abs(gw - tg)
        for i, Av in enumerate(A.tolist()):
            z = Av * dist
            keep = (z <= zcut) & (gw != tg)
            ns[i], nsh[i] = int(keep.sum()), int((keep & shared).sum())
            if ns[i]:
                with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
                    u = np.exp(-z[keep]) / (1.0 + d[keep])
                    term = np.log1p(u * (R[:, :, rw[keep]] - d[keep]))
                    T[i] = 2.0 * np.sum(term, axis=2)
                    S[i] = 2.0 * np.sum(np.abs(term), axis=2)
    return (T, ns, nsh, S) if scale else (T, ns, nsh)


# ---------------------------------------------------------------------------------------------------------- output

def output_name(outfile):
    return outfile + '.surfaces.txt'


def labels(ts, rows):
    """(physPos, genPos) of the given test sites as the main output prints them."""
    if ts.arrays is not None:
        phys, gen = ts.arrays[0][rows].tolist(), ts.arrays[1][rows].tolist()
    else:
        phys = [float(v) if isinstance(v, np.floating) else v for v in (ts.phys[j] for j in rows)]
        gen = [float(v) if isinstance(v, np.floating) else v for v in (ts.gen_label[j] for j in rows)]
    return [f'{p}' for p in phys], [f'{g}' for g in gen]


class Layout:
    """Ascending order of the three grids (given in the scan's order: A, x, abeta) and the printed `A x abeta` columns of a
    block's rows."""

    def __init__(self, grid_A, grid_x, grid_abeta):
        asc = lambda grid: sorted(range(len(grid)), key=lambda i: float(grid[i]))
        self.oA, self.ox, self.oab = asc(grid_A), asc(grid_x), asc(grid_abeta)
        self.shape = (len(self.oA), len(self.ox), len(self.oab))
        self.points = len(self.oA) * len(self.ox) * len(self.oab)
        self.cols = ['%s\t%s\t%s' % (f'{grid_A[i]}', f'{grid_x[j]}', f'{grid_abeta[k]}')
                     for i in self.oA for j in self.ox for k in self.oab]
        self.per_A = len(self.ox) * len(self.oab)

    def ascending(self, T):
        """T[n][nA][nx][nab] in the scan's order -> the same in ascending grid order."""
        T = np.asarray(T, dtype=np.float64).reshape((-1,) + self.shape)
        return T[:, self.oA][:, :, self.ox][:, :, :, self.oab]


def write_blocks(f, layout, phys, gen, T, ns):
    """The blocks of len(phys) windows appended to the open file f.  T[n][nA][nx][nab], ns[n][nA] in the scan's grid order."""
    T = layout.ascending(T)
    ns = np.asarray(ns).reshape(len(phys), layout.shape[0])[:, layout.oA]
    for w in range(len(phys)):
        head = '%s\t%s\t' % (phys[w], gen[w])
        vals = ['NA' if v != v else repr(v) for v in T[w].reshape(-1).tolist()]
        sizes = [str(v) for v in ns[w].tolist() for _ in range(layout.per_A)]
        f.writelines([head + c + '\t' + v + '\t' + s + '\n' for c, v, s in zip(layout.cols, vals, sizes)])


def write_surfaces(path, layout, phys, gen, T, ns):
    """A whole file from arrays held on the host (the tests' entry point)."""
    with open(path, 'w') as f:
        f.write(HEADER)
        write_blocks(f, layout, phys, gen, T, ns)


def read_surfaces(path, layout):
    """A surfaces file back: (physPos strings, genPos strings, T[n][nA][nx][nab], nsites[n][nA]) in ASCENDING grid order."""
    with open(path) as f:
        rows = [l.rstrip('\n').split('\t') for l in f.readlines()[1:]]
    n = len(rows) // layout.points if layout.points else 0
    T = np.array([float('nan') if r[5] == 'NA' else float(r[5]) for r in rows]).reshape((n,) + layout.shape)
    ns = np.array([int(r[6]) for r in rows], dtype=np.int32).reshape(n, layout.shape[0], layout.per_A)[:, :, 0]
    first = rows[::layout.points] if layout.points else []
    return [r[0] for r in first], [r[1] for r in first], T, ns


def surfaces_and_write(ctx, outfile, ts, sel, min_clr=0.0, max_n=MAX_WINDOWS, apex_rows=None, host_bytes=HOST_BYTES):
    """After the observed scan of one file on ctx's selected slot (and its peak call, if any): select the windows, compute
    their surfaces and write <outfile>.surfaces.txt.  sel: the run's NormalizedBetaBinom (the grids in scan order).
    The surfaces are fetched in batches of at most host_bytes, each written before the next is computed.
    Returns (windows written, windows the cap dropped)."""
    layout = Layout(sel.grid_A, sel.grid_x, sel.grid_abeta)
    rows, dropped = np.zeros(0, dtype=np.int64), 0
    if len(ts):
        clr, _, _, iA, _ = ctx.fetch()
        rows, dropped = select(clr, iA, min_clr, apex_rows, max_n)
    batch = max(1, int(host_bytes) // (8 * max(layout.points, 1)))
    with open(output_name(outfile), 'w') as f:
        f.write(HEADER)
        for k in range(0, len(rows), batch):
            part = rows[k:k + batch]
            T, ns = ctx.surfaces(part)
            phys, gen = labels(ts, part.tolist())
            write_blocks(f, layout, phys, gen, T, ns)
    return len(rows), dropped
