"""Delete-block jackknife of each selected window's CLR: the definition behind --influence, a plain host restatement, the
per-window summary, and the writers.

What it answers.  A composite likelihood is a sum over sites; --influence says which sites carry a window's maximum: the CLR
the window would have without each block of B consecutive sites, and the share of the maximum each block holds.

Inputs.  One window (test position tg, site indices [win_lo, win_hi], clipped to the chromosome), the model's grids in scan
order, zcut = bmx_alpha_cut(), a block size B >= 1.

Qualifying sites.  Site i qualifies at A when A * |g_i - tg| <= zcut and g_i != tg (the two IEEE operations of the scan and of
surfaces_kernel); ns(A) is their number.

Surface.  T(A, p) = 2 S(A, p), S the sum of log1p(exp(-z_i) R[row_i][p]) over the qualifying sites in increasing site index,
p = ix * nab + ia: bitwise what bmx_ctx_surfaces returns (surfaces.py).

Blocks.  Block of site i: b = i // B (--boot's rule on the index given to set_sites).  A_min is the smallest value of the A
grid; the qualifying sets are nested in A (FP multiplication is monotone), so every qualifying site qualifies at A_min.
i_first and i_last: the first and last site qualifying at A_min; the window's block range is i_first // B ... i_last // B
(empty without a qualifying site).  m_b: the sites of block b that qualify at A_min.  A block of the range with m_b = 0 is
not a block of the window (with B = 1 the apex's own site is one).

Block partial sum.  S_b(A, p): the same expression over the qualifying sites of block b, in increasing site index; n_b(A)
their number.

Full argmax.  T_max and lin* by the scan's rule on T: a candidate must be > 0, the larger value wins, on a tie the smaller
linear index lin = (iA * nx + ix) * nab + ia; all comparisons are `>`, so a NaN never wins; T_max = 0 and lin* = -1 when
nothing is > 0.

Per block of the range.  contrib_b = 2 S_b(lin*) (NaN when lin* < 0).  L_b and lin_b: maximum and index, under the same
rule, of T(A, p) - 2 S_b(A, p) over the grid points whose A still has a site left, ns(A) - n_b(A) > 0 (the reference skips
an A without sites, BalLeRMix+_v1.py:458-459, and so does this); where n_b(A) = 0 the candidate is T(A, p) itself; L_b = 0
and lin_b = -1 when nothing is > 0.

Per window (summarise(), over the blocks with m_b > 0).  nBlocks; jk_se = sqrt((nBlocks - 1) / nBlocks * sum (L_b - mean
L)^2), NA when nBlocks < 2; n_half = the fewest blocks, taken in descending order of contrib_b (the earlier block first among
equals), whose contributions add up to >= T_max / 2; share_max = max contrib_b / T_max; n_moved = #{b: lin_b != lin*}; the
drop block b1 = argmin L_b (the earliest on a tie): the physPos of its first and last site, its m_b, drop_share =
contrib_b1 / T_max, CLR_drop = L_b1 and the grid strings at lin_b1 as the main output prints them (NA when lin_b1 = -1).

It is a jackknife of the GRID maximum of the plain-sum surface, not of the refined maximum; jk_se describes how the CLR
depends on single blocks and is no calibrated standard error (blocks are not independent under LD).

Selection.  As --surfaces selects (surfaces.select): --influenceMin C, with --peaks only the apexes, at most --influenceMax N.

Output.  <out>.influence.txt, tab-separated, floats as repr, one row per selected window in the main output's order; a window
with T_max = 0 or nBlocks = 0 prints NA from nBlocks on.  With --influenceDetail <out>.influence.blocks.txt: one row per
selected window and block with m_b > 0.
"""
import math

import numpy as np

from . import surfaces

HEADER = ('physPos\tgenPos\tCLR\tT_max\tnBlocks\tjk_se\tn_half\tshare_max\tn_moved\tdrop_lo_physPos\tdrop_hi_physPos\t'
          'drop_nSites\tdrop_share\tCLR_drop\tx_drop\ts_drop\tA_drop\n')
BLOCKS_HEADER = 'physPos\tgenPos\tblock\tlo_physPos\thi_physPos\tnSites\tcontrib\tCLR_without\tx_hat\ts_hat\tA_hat\n'
MAX_WINDOWS = surfaces.MAX_WINDOWS
MAX_RESULTS = 1 << 26           # BMX_INFLUENCE_MAX_RESULTS: blocks of one bmx_ctx_influence call
HOST_BLOCKS = 1 << 22           # the writer asks for at most this many blocks at a time (24 bytes each on the host)


def value_refusal(block, min_clr, max_n):
    """The message that refuses these values of --influenceBlock / --influenceMin / --influenceMax, or None."""
    if block is not None and block < 1:
        return '--influenceBlock must be >= 1.'
    if max_n is not None and max_n < 1:
        return '--influenceMax takes a number of windows >= 1.'
    if min_clr is not None and min_clr != min_clr:
        return '--influenceMin takes a number.'
    return None


# ----------------------------------------------------------------------------------------------- the host restatement

def scan_argmax(values):
    """The scan's rule on a flat array in linear-index order: (maximum, index), (0.0, -1) when nothing is > 0; NaN never wins.
    Also returns the runner-up value among the candidates > 0 (0.0 without one)."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    ok = v > 0                      # False for NaN
    if not ok.any():
        return 0.0, -1, 0.0
    w = np.where(ok, v, -np.inf)
    lin = int(np.argmax(w))         # the first maximum: the smaller linear index on a tie
    w[lin] = -np.inf
    second = float(w.max()) if len(w) > 1 else -np.inf
    return float(v[lin]), lin, max(second, 0.0)


def host_influence(genpos, rows, R, A, tg, lo, hi, zcut, block):
    """The jackknife of one window in numpy, on surfaces.host_surface's expression.  genpos[N], rows[N], R[nx][nab][table
    rows], A: the grid in scan order, (tg, lo, hi): the window, zcut: bmx_alpha_cut(), block: B.
    Returns a dict: T_max, lin, ns_min (qualifying sites at A_min), T[nA][nx][nab], first_block, and per block of the range
    m, contrib, L, blin, margin (L_b minus the runner-up candidate, floored at 0: how far lin_b is from changing) and
    n_b[nA][blocks]; ns[nA]."""
    g = np.asarray(genpos, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.int64)
    R = np.asarray(R, dtype=np.float64)
    A = np.atleast_1d(np.asarray(A, dtype=np.float64))
    B = int(block)
    nA, npairs = len(A), R.shape[0] * R.shape[1]
    T, ns = surfaces.host_surface(g, rows, R, A, tg, lo, hi, zcut)
    T_max, lin_star, _ = scan_argmax(T)
    a, b = max(int(lo), 0), min(int(hi), len(g) - 1)
    idx = np.arange(a, b + 1, dtype=np.int64) if b >= a else np.zeros(0, dtype=np.int64)
    gw = g[idx]
    dist = np.abs(gw - tg)
    iAmin = int(np.argmin(A))
    keep_min = (A[iAmin] * dist <= zcut) & (gw != tg)
    out = {'T_max': T_max, 'lin': lin_star, 'ns_min': int(keep_min.sum()), 'T': T, 'ns': ns, 'first_block': 0,
           'n_b': np.zeros((nA, 0), dtype=np.int64)}
    if not keep_min.any():
        out.update(m=np.zeros(0, np.int32), contrib=np.zeros(0), L=np.zeros(0), blin=np.zeros(0, np.int32), margin=np.zeros(0))
        return out
    q = idx[keep_min]
    b0, b1 = int(q[0]) // B, int(q[-1]) // B
    nb = b1 - b0 + 1
    blk = idx // B - b0
    m = np.bincount(blk[keep_min], minlength=nb).astype(np.int32)
    # S_b[iA][b][pair] and n_b[iA][b]
    S = np.zeros((nA, nb, npairs))
    n_b = np.zeros((nA, nb), dtype=np.int64)
    for i, Av in enumerate(A.tolist()):
        z = Av * dist
        keep = (z <= zcut) & (gw != tg)
        if not keep.any():
            continue
        with np.errstate(divide='ignore', invalid='ignore'):
            term = np.log1p(np.exp(-z[keep]) * R[:, :, rows[idx[keep]]]).reshape(npairs, -1)
        kb = blk[keep]
        n_b[i] = np.bincount(kb, minlength=nb)
        starts = np.flatnonzero(np.r_[True, kb[1:] != kb[:-1]])         # kb is non-decreasing: one run per block
        S[i, kb[starts]] = np.add.reduceat(term, starts, axis=1).T
    Tf = T.reshape(nA, npairs)
    contrib, L, blin, margin = np.full(nb, np.nan), np.zeros(nb), np.full(nb, -1, np.int32), np.zeros(nb)
    for bb in range(nb):
        cand = np.where((n_b[:, bb] > 0)[:, None], Tf - 2.0 * S[:, bb], Tf)
        cand[(ns - n_b[:, bb]) <= 0] = np.nan           # an A without a site left is skipped
        L[bb], blin[bb], second = scan_argmax(cand)
        margin[bb] = L[bb] - second if blin[bb] >= 0 else -np.nanmax(np.where(np.isnan(cand), -np.inf, cand), initial=-np.inf)
        if lin_star >= 0:
            contrib[bb] = 2.0 * S[lin_star // npairs, bb, lin_star % npairs]
    out.update(first_block=b0, m=m, contrib=contrib, L=L, blin=blin, margin=margin, n_b=n_b)
    return out


# ------------------------------------------------------------------------------------------------------------ summary

def grid_strings(lin, sel):
    """(x, s, A) of the linear grid index as the main output prints them; NA for -1."""
    if lin < 0:
        return 'NA', 'NA', 'NA'
    nx, nab = len(sel.grid_x), len(sel.grid_abeta)
    return f'{sel.grid_x[(lin // nab) % nx]}', f'{sel.grid_abeta[lin % nab]}', f'{sel.grid_A[lin // (nx * nab)]}'


def summarise(T_max, lin, first_block, m, contrib, L, blin):
    """The per-window numbers of the definition from one window's arrays (the blocks of its range, in order).  Returns a dict
    with nBlocks and -- None where the definition says NA -- jk_se, n_half, share_max, n_moved, drop (the drop block's place in
    the range), drop_block (its number), drop_nSites, drop_share, CLR_drop, drop_lin; None for all but nBlocks when T_max = 0
    or nBlocks = 0."""
    m = np.asarray(m)
    own = np.nonzero(m > 0)[0]
    nB = len(own)
    out = {'nBlocks': nB, 'jk_se': None, 'n_half': None, 'share_max': None, 'n_moved': None, 'drop': None, 'drop_block': None,
           'drop_nSites': None, 'drop_share': None, 'CLR_drop': None, 'drop_lin': None}
    if nB == 0 or not T_max > 0:
        return out
    c = np.asarray(contrib, dtype=np.float64)[own]
    Lb = np.asarray(L, dtype=np.float64)[own]
    bl = np.asarray(blin)[own]
    if nB >= 2:
        out['jk_se'] = math.sqrt((nB - 1) / nB * float(np.sum((Lb - np.mean(Lb)) ** 2)))
    order = np.lexsort((np.arange(nB), -c))             # contrib descending, the earlier block first among equals
    run, half = 0.0, T_max / 2
    for k, j in enumerate(order.tolist()):
        run += float(c[j])
        if run >= half:
            out['n_half'] = k + 1
            break
    out['share_max'] = float(np.max(c)) / T_max
    out['n_moved'] = int(np.sum(bl != lin))
    d = int(np.argmin(Lb))                              # the first minimum
    out.update(drop=int(own[d]), drop_block=int(first_block) + int(own[d]), drop_nSites=int(m[own[d]]),
               drop_share=float(c[d]) / T_max, CLR_drop=float(Lb[d]), drop_lin=int(bl[d]))
    return out


# ---------------------------------------------------------------------------------------------------------- output

def output_name(outfile):
    return outfile + '.influence.txt'


def blocks_name(outfile):
    return outfile + '.influence.blocks.txt'


def _num(v):
    return 'NA' if v is None or v != v else (repr(float(v)) if isinstance(v, (float, np.floating)) else str(int(v)))


def block_sites(block, B, N):
    """First and last site index of block number `block` on a chromosome of N sites."""
    return block * B, min(block * B + B - 1, N - 1)


def summary_row(phys, gen, clr, T_max, s, position, B, sel):
    """One row of <out>.influence.txt: (phys, gen, clr) the main output's strings, s = summarise()'s dict, position: the
    input's physPos per site."""
    head = '%s\t%s\t%s\t%s\t' % (phys, gen, clr, repr(float(T_max)))
    if s['drop'] is None:
        return head + '\t'.join(['NA'] * 13) + '\n'
    i0, i1 = block_sites(s['drop_block'], B, len(position))
    cols = [_num(s['nBlocks']), _num(s['jk_se']), _num(s['n_half']), _num(s['share_max']), _num(s['n_moved']), f'{position[i0]}',
            f'{position[i1]}', _num(s['drop_nSites']), _num(s['drop_share']), _num(s['CLR_drop'])] + list(grid_strings(s['drop_lin'], sel))
    return head + '\t'.join(cols) + '\n'


def block_rows(phys, gen, first_block, m, contrib, L, blin, position, B, sel):
    """The rows of <out>.influence.blocks.txt of one window: its blocks with m_b > 0."""
    out = []
    for j in np.nonzero(np.asarray(m) > 0)[0].tolist():
        i0, i1 = block_sites(int(first_block) + j, B, len(position))
        out.append('\t'.join([phys, gen, str(int(first_block) + j), f'{position[i0]}', f'{position[i1]}', str(int(m[j])), _num(float(contrib[j])),
                              _num(float(L[j]))] + list(grid_strings(int(blin[j]), sel))) + '\n')
    return out


def read_table(path):
    """(header names, rows as lists of strings) of either file."""
    with open(path) as f:
        lines = f.read().split('\n')
    return lines[0].split('\t'), [l.split('\t') for l in lines[1:] if l]


def influence_and_write(ctx, outfile, ts, sel, data, block=1, min_clr=0.0, max_n=MAX_WINDOWS, apex_rows=None, detail=False,
                        host_blocks=HOST_BLOCKS):
    """After the observed scan of one file on ctx's selected slot (and its peak call, if any): select the windows as --surfaces
    does, jackknife them and write <outfile>.influence.txt (detail: also <outfile>.influence.blocks.txt).  sel: the run's
    NormalizedBetaBinom (the grids in scan order); data: the input (its `position` array names the blocks' sites).  The windows
    are given to the device in batches whose block ranges hold at most host_blocks blocks -- a window's range has at most
    1 + (its sites at A_min) / B -- each written before the next is computed.  Returns (windows written, windows the cap dropped)."""
    rows, dropped = np.zeros(0, dtype=np.int64), 0
    clr = np.zeros(0)
    if len(ts):
        clr, _, _, iA, _ = ctx.fetch()
        rows, dropped = surfaces.select(clr, iA, min_clr, apex_rows, max_n)
    position = data.position
    N, B = len(position), int(block)
    # an upper bound of a window's blocks that needs no device call: the blocks its index window touches
    lo = np.maximum(np.asarray(ts.lo, dtype=np.int64)[rows], 0) if len(rows) else np.zeros(0, dtype=np.int64)
    hi = np.minimum(np.asarray(ts.hi, dtype=np.int64)[rows], N - 1) if len(rows) else np.zeros(0, dtype=np.int64)
    bound = np.where(hi >= lo, hi // B - lo // B + 1, 0)
    fb = open(blocks_name(outfile), 'w') if detail else None
    try:
        with open(output_name(outfile), 'w') as f:
            f.write(HEADER)
            if fb:
                fb.write(BLOCKS_HEADER)
            k = 0
            while k < len(rows):
                e, total = k + 1, int(bound[k])
                while e < len(rows) and total + int(bound[e]) <= host_blocks:
                    total += int(bound[e])
                    e += 1
                part = rows[k:e]
                r = ctx.influence(part, B)
                phys, gen = surfaces.labels(ts, part.tolist())
                for w in range(len(part)):
                    a, b = int(r['offset'][w]), int(r['offset'][w + 1])
                    arrs = (r['m'][a:b], r['contrib'][a:b], r['L'][a:b], r['blin'][a:b])
                    s = summarise(float(r['T_max'][w]), int(r['lin'][w]), int(r['first_block'][w]), *arrs)
                    f.write(summary_row(phys[w], gen[w], repr(float(clr[part[w]])), r['T_max'][w], s, position, B, sel))
                    if fb:
                        fb.writelines(block_rows(phys[w], gen[w], r['first_block'][w], *arrs, position, B, sel))
                k = e
    finally:
        if fb:
            fb.close()
    return len(rows), dropped
