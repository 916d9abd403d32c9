"""Peaks of the CLR track: the definition behind --peaks, a plain host restatement of it, and the writers.

The scan prints one row per test site; --peaks turns that track into loci: one apex per locus, where the locus starts and
ends, and how deep the valleys to its neighbours are.  The device (peak_*_kernel, bmx_ctx_peaks / bmx_ctx_peaks_track)
implements exactly the rules below.  Every comparison is an exact FP64 comparison, the only arithmetic is the two
subtractions of the radius and the one multiplication of the extent's threshold, so call() below -- numpy on the host, used
by the tests and never by the product path -- and the device agree exactly: there is no tolerance anywhere in this feature.

Track.  The test sites of one file that have a scan result, in the order of the main output, t = 0 .. M-1, with the test
position g_t the scan used (the genPos column; physPos * --rec with --usePhysPos) and c_t = the CLR column (0 where no grid
point had T > 0).  NA rows of the main output are not part of the track.  Positions must be non-decreasing; a track whose
positions are not is refused (the CLI's window modes cannot produce one, the C ABI can).

Apex.  With separation G >= 0 and floor C: row t is an apex iff c_t > 0, c_t >= C, and there is no row s != t with
g_t - g_s <= G and g_s - g_t <= G (these two subtractions, no other arithmetic) that has c_s > c_t, or c_s == c_t and s < t.
Consequences:
  - a plateau yields its first row;
  - two apexes are always more than G apart;
  - G = 0 still merges rows at the same position;
  - the global maximum's first row is an apex whenever it passes C;
  - this is a local-maximum rule, NOT greedy clumping: a row that is beaten by a neighbour which is itself beaten is not an
    apex.  Clumping (PLINK-style) would hand that row its own clump once the winner's clump is removed; here it stays part
    of the slope of a higher locus.  Fewer, cleaner peaks.

Saddle.  Between two consecutive apexes a < b: the row of smallest c strictly between them, the first such row on ties;
none if b = a + 1.

Extent.  With fraction F in (0, 1] (default 0.5: the width at half maximum): the region of apex a is the maximal run of
consecutive rows lo .. hi containing a with c >= F * c_a (one multiplication, compared with >=) on every row, cut so that
it stays strictly inside the saddles on either side -- the saddle row belongs to neither region; two apexes on adjacent
rows have no saddle, and their regions end at their own rows on that side.  Regions are therefore disjoint.  An extent
describes the track's shape; it is not an interval for the selected site.

Rank.  1 for the file's highest apex; ties by row order.
"""
import os
import sys

import numpy as np

FRAC = 0.5
HEADER = ('physPos\tgenPos\tCLR\tx_hat\ts_hat\tA_hat\tnSites\trank\tstart_physPos\tend_physPos\tstart_genPos\tend_genPos\t'
          'nWindows\tsaddle_lo\tsaddle_hi\tp_site\tp_genome\n')
FIELDS = ('row', 'lo', 'hi', 'saddle_lo', 'saddle_hi')


def value_refusal(sep, min_clr, frac):
    """The message that refuses these values of --peaks / --peakMin / --peakExtent, or None."""
    if sep is None or sep != sep or not sep >= 0.0:
        return '--peaks takes a separation G >= 0 (in the units the scan measures distance in).'
    if min_clr is not None and min_clr != min_clr:
        return '--peakMin takes a number.'
    if frac is not None and not (0.0 < frac <= 1.0):
        return '--peakExtent takes a fraction F with 0 < F <= 1.'
    return None


# ----------------------------------------------------------------------------------------------- the host restatement

def _ranges(g, rows, sep):
    """lo, hi of the given rows: the lowest / highest row whose position is within sep, by bisection with the exact predicate."""
    M = len(g)
    gt = g[rows]
    a, b = np.zeros(len(rows), dtype=np.int64), rows.copy()
    while np.any(a < b):
        mid = (a + b) >> 1
        live = a < b
        ok = (gt - g[mid] <= sep) & live
        b = np.where(ok, mid, b)
        a = np.where(~ok & live, mid + 1, a)
    lo = a
    a, b = rows.copy(), np.full(len(rows), M - 1, dtype=np.int64)
    while np.any(a < b):
        mid = (a + b + 1) >> 1
        live = a < b
        ok = (g[mid] - gt <= sep) & live
        a = np.where(ok, mid, a)
        b = np.where(~ok & live, mid - 1, b)
    return lo, a


def _ahead(c):
    """prev[t]: the highest row s < t with c_s >= c_t (-1: none); nxt[t]: the lowest row s > t with c_s > c_t (M: none) --
    the nearest rows on either side that are ahead of t."""
    M = len(c)
    v = c.tolist()
    prev, nxt = [-1] * M, [M] * M
    st = []
    for t in range(M):
        x = v[t]
        while st and v[st[-1]] < x:
            nxt[st.pop()] = t
        if st:
            prev[t] = st[-1]
        st.append(t)
    return np.array(prev, dtype=np.int64), np.array(nxt, dtype=np.int64)


def apexes(g, c, sep, min_clr=0.0):
    """Rows of the apexes, ascending (int64)."""
    g, c = np.ascontiguousarray(g, dtype=np.float64), np.ascontiguousarray(c, dtype=np.float64)
    if len(g) and not np.all(g[1:] >= g[:-1]):
        raise ValueError('positions are not non-decreasing')
    rows = np.nonzero((c > 0.0) & (c >= min_clr))[0].astype(np.int64)
    if not len(rows):
        return rows
    lo, hi = _ranges(g, rows, float(sep))
    prev, nxt = _ahead(c)
    return rows[(prev[rows] < lo) & (nxt[rows] > hi)]


def saddles(c, rows):
    """sad[i + 1] = the saddle row between apex i and apex i + 1 (-1: adjacent rows); sad[0] = sad[K] = -1."""
    K = len(rows)
    sad = np.full(K + 1, -1, dtype=np.int64)
    for i in range(K - 1):
        a, b = int(rows[i]), int(rows[i + 1])
        if b > a + 1:
            sad[i + 1] = a + 1 + int(np.argmin(c[a + 1:b]))         # argmin: the first row of the minimum
    return sad


def extents(c, rows, sad, frac):
    M, K = len(c), len(rows)
    lo, hi = np.empty(K, dtype=np.int64), np.empty(K, dtype=np.int64)
    for i in range(K):
        a = int(rows[i])
        thr = float(frac) * float(c[a])
        lim_lo = 0 if i == 0 else (int(sad[i]) + 1 if sad[i] >= 0 else int(rows[i - 1]) + 1)
        lim_hi = M - 1 if i == K - 1 else (int(sad[i + 1]) - 1 if sad[i + 1] >= 0 else int(rows[i + 1]) - 1)
        below = np.nonzero(~(c[a + 1:lim_hi + 1] >= thr))[0]           # offsets from a + 1 upwards
        hi[i] = a + int(below[0]) if len(below) else lim_hi
        below = np.nonzero(~(c[lim_lo:a][::-1] >= thr))[0]              # offsets from a - 1 downwards
        lo[i] = a - int(below[0]) if len(below) else lim_lo
    return lo, hi


def call(g, c, sep, min_clr=0.0, frac=FRAC):
    """The peaks of the track (g, c): {'row', 'lo', 'hi', 'saddle_lo', 'saddle_hi'} per apex in row order (int32; saddle
    rows -1 where there is none) -- what Context.fetch_peaks returns."""
    refused = value_refusal(sep, min_clr, frac)
    if refused:
        raise ValueError(refused)
    c = np.ascontiguousarray(c, dtype=np.float64)
    if np.any(c != c):
        raise ValueError('NaN in the track')
    rows = apexes(g, c, sep, min_clr)
    sad = saddles(c, rows)
    lo, hi = extents(c, rows, sad, frac)
    out = {'row': rows, 'lo': lo, 'hi': hi, 'saddle_lo': sad[:-1], 'saddle_hi': sad[1:]}
    return {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in out.items()}


def ranks(clr_at_apexes):
    """Rank of every apex: 1 for the highest, ties by row order."""
    v = np.asarray(clr_at_apexes, dtype=np.float64)
    order = np.lexsort((np.arange(len(v)), -v))
    r = np.empty(len(v), dtype=np.int64)
    r[order] = np.arange(1, len(v) + 1)
    return r


# ---------------------------------------------------------------------------------------------------------- output

def output_name(outfile):
    return outfile + '.peaks.txt'


def read_track(main_path):
    """(lines of the main output, line index of every track row, g, c): the rows that carry a scan result (x_hat is not
    NA), their genPos and CLR columns as floats -- the values the scan used and reported, since both are printed as repr."""
    with open(main_path) as f:
        lines = f.readlines()
    idx, g, c = [], [], []
    for j in range(1, len(lines)):
        col = lines[j].rstrip('\r\n').split('\t')
        if len(col) < 7 or col[3] == 'NA':
            continue
        idx.append(j)
        g.append(float(col[1]))
        c.append(float(col[2]))
    return lines, np.array(idx, dtype=np.int64), np.array(g, dtype=np.float64), np.array(c, dtype=np.float64)


def peak_rows(lines, line_of_row, pk, pval_lines=None):
    """The rows of the peak table as lists of strings (HEADER's columns), in position order.  lines: the main output's;
    line_of_row: line index of every track row (None: row t is line t + 1); pk: call()'s / fetch_peaks()'s arrays;
    pval_lines: the lines of <out>.pval.txt (same line numbering), or None.  Every number is the text the main output
    (or the p-value file) prints."""
    at = (lambda t: int(t) + 1) if line_of_row is None else (lambda t: int(line_of_row[int(t)]))
    col = lambda t: lines[at(t)].rstrip('\r\n').split('\t')
    apex = [col(t) for t in pk['row'].tolist()]
    rk = ranks([float(a[2]) for a in apex]).tolist()
    out = []
    for i, a in enumerate(apex):
        lo, hi = col(pk['lo'][i]), col(pk['hi'][i])
        sl, sh = int(pk['saddle_lo'][i]), int(pk['saddle_hi'][i])
        p = pval_lines[at(pk['row'][i])].rstrip('\r\n').split('\t')[3:5] if pval_lines is not None else ['NA', 'NA']
        out.append(a[:7] + [str(rk[i]), lo[0], hi[0], lo[1], hi[1], str(int(pk['hi'][i]) - int(pk['lo'][i]) + 1),
                            col(sl)[2] if sl >= 0 else 'NA', col(sh)[2] if sh >= 0 else 'NA'] + p)
    return out


def write_peaks(path, main_path, pk, line_of_row=None, pval_path=None):
    """<out>.peaks.txt of one file from its main output (and its p-value file, if any).  Returns the rows written."""
    with open(main_path) as f:
        lines = f.readlines()
    pval_lines = None
    if pval_path is not None and os.path.exists(pval_path):
        with open(pval_path) as f:
            pval_lines = f.readlines()
    rows = peak_rows(lines, line_of_row, pk, pval_lines) if len(pk['row']) else []
    with open(path, 'w') as f:
        f.write(HEADER)
        f.writelines('\t'.join(r) + '\n' for r in rows)
    return rows


def write_genome(path, per_file):
    """The genome-wide table of a run over several files.  per_file: (input basename, rows of that file's table).  Every
    file's rows with a leading `file` column, sorted by CLR descending (ties: file order, then position), rank genome-wide."""
    rows = [[name] + list(r) for name, rs in per_file for r in rs]
    order = sorted(range(len(rows)), key=lambda j: -float(rows[j][3]))          # (sorted is stable)
    with open(path, 'w') as f:
        f.write('file\t' + HEADER)
        for k, j in enumerate(order):
            r = rows[j]
            f.write('\t'.join(r[:8] + [str(k + 1)] + r[9:]) + '\n')


def empty():
    return {k: np.zeros(0, dtype=np.int32) for k in FIELDS}


# ------------------------------------------------------------------------------------------- python -m ...peaks OUT.txt

def build_parser():
    import argparse
    p = argparse.ArgumentParser(prog='python -m ballermixplus_amd.peaks',
                                description='Call peaks again on an existing main output, without rescanning: writes '
                                            'OUT.txt.peaks.txt as the run itself would have (p-values from OUT.txt.pval.txt if it exists).')
    p.add_argument('output', help='main output file of a scan (7 tab-separated columns)')
    p.add_argument('--peaks', dest='peaks', type=float, required=True, help='separation G in the units of the genPos column')
    p.add_argument('--peakMin', dest='peakMin', type=float, default=0.0, help='only apexes with CLR >= C (default 0)')
    p.add_argument('--peakExtent', dest='peakExtent', type=float, default=FRAC,
                   help='extent of a peak: rows with CLR >= F * apex CLR, 0 < F <= 1 (default 0.5)')
    p.add_argument('--device', dest='device', type=int, default=0, help='GPU index (default 0)')
    return p


def main(argv=None):
    opt = build_parser().parse_args(sys.argv[1:] if argv is None else argv)
    refused = value_refusal(opt.peaks, opt.peakMin, opt.peakExtent)
    if not refused and not os.path.isfile(opt.output):
        refused = 'No such output file: %s' % opt.output
    if refused:
        print(refused)
        sys.exit(1)
    lines, idx, g, c = read_track(opt.output)
    if not lines or lines[0].split('\t')[:3] != HEADER.split('\t')[:3]:
        print('%s is not a main output of the scan (header physPos, genPos, CLR, ... expected).' % opt.output)
        sys.exit(1)
    if len(g) and not np.all(g[1:] >= g[:-1]):
        print('The genPos column of %s is not non-decreasing: peaks cannot be called on it.' % opt.output)
        sys.exit(1)
    if len(g):
        from . import engine
        ctx = engine.Context(opt.device)
        pk = ctx.peaks_track(g, c, opt.peaks, opt.peakMin, opt.peakExtent)
        ctx.close()
    else:
        pk = empty()
    rows = write_peaks(output_name(opt.output), opt.output, pk, idx, opt.output + '.pval.txt')
    print('%d peak/s -> %s' % (len(rows), output_name(opt.output)))


if __name__ == '__main__':
    main()
