"""Profile likelihoods of the CLR over A, x and alpha_beta: the host half of --profiles.

For test site t and grid value v of a parameter P in {A, x, abeta}:

    profile_P[t][v] = max(0, max of T over the other two grids at P = v)

the CLR column the same command prints at t when P is fixed to v (--listA v, --fixX repr(v), --fixAlpha v); 0 where no grid
point has T > 0, as the reference's scan (BalLeRMix+_v1.py:451).  The device computes them from the scan's own products
(bmx_ctx_set_profiles / bmx_ctx_fetch_profile) and max_v profile_P[t][v] equals the CLR bit for bit.  This module holds the
host definition on a full likelihood surface (the tests compare it with surfaces the reference made) and the writers of the
three output files.
"""
import numpy as np

# name on the command line -> (bit of bmx_ctx_set_profiles, column prefix, axis of the surface T[A][x][abeta])
KINDS = {'A': (1, 'A', 0), 'x': (2, 'x', 1), 'abeta': (4, 'abeta', 2)}
ORDER = ('A', 'x', 'abeta')


def parse(spec):
    """'A,x,abeta' -> the ordered tuple of names; ValueError on an empty list or an unknown name."""
    names = [s.strip() for s in str(spec).split(',') if s.strip()]
    if not names:
        raise ValueError('--profiles takes a comma list of A, x, abeta.')
    for n in names:
        if n not in KINDS:
            raise ValueError('--profiles: unknown profile %r (choose from A, x, abeta).' % n)
    return tuple(n for n in ORDER if n in names)


def mask(names):
    """The BMX_PL_* bit set of a parse() result."""
    m = 0
    for n in names:
        m |= KINDS[n][0]
    return m


def profiles_from_surface(T):
    """T[nA][nx][nab] (NaN: empty window) -> {'A': [nA], 'x': [nx], 'abeta': [nab]}: max(0, nanmax over the other two axes)."""
    T = np.asarray(T, dtype=np.float64)
    out = {}
    for name in ORDER:
        ax = KINDS[name][2]
        other = tuple(a for a in range(3) if a != ax)
        filled = np.where(np.isnan(T), -np.inf, T)
        out[name] = np.maximum(filled.max(axis=other), 0.0)
    return out


def output_name(outfile, name):
    return '%s.profile_%s.txt' % (outfile, name)


def write_profile(path, name, ts, prof, grid):
    """One profile file.  prof: f64 [len(ts)][len(grid)] in the order of `grid` (the scan's grid order); columns go out in
    ascending grid order, labelled as the main output prints the grid value.  The abeta file has CLR_bal (max over
    alpha_beta >= 1) and CLR_pos (max over alpha_beta < 1, on this run's x grid) at the end.  One row per row of the main
    output, in its order; rows the main output prints without a scan result (ts.na_rows) carry NA."""
    prefix = KINDS[name][1]
    grid = list(grid)
    prof = np.asarray(prof, dtype=np.float64).reshape(len(ts), len(grid))
    order = sorted(range(len(grid)), key=lambda i: grid[i])
    cols = prof[:, order]
    head = ['physPos', 'genPos'] + ['%s=%s' % (prefix, grid[i]) for i in order]
    if name == 'abeta':
        vals = np.asarray([float(grid[i]) for i in order])
        bal, pos = vals >= 1.0, vals < 1.0
        zero = np.zeros(len(ts))
        cols = np.column_stack([cols, cols[:, bal].max(axis=1) if bal.any() else zero,
                                cols[:, pos].max(axis=1) if pos.any() else zero])
        head += ['CLR_bal', 'CLR_pos']
    ncol = len(head) - 2
    if ts.arrays is not None:
        phys, gen = ts.arrays[0].tolist(), ts.arrays[1].tolist()
    else:
        phys = [float(v) if isinstance(v, np.floating) else v for v in ts.phys]
        gen = [float(v) if isinstance(v, np.floating) else v for v in ts.gen_label]
    body = ['%s\t%s\t%s\n' % (p, g, '\t'.join(map(repr, row))) for p, g, row in zip(phys, gen, cols.tolist())]
    if ts.na_rows:
        lines = [None] * (len(ts) + len(ts.na_rows))
        for pos, line in ts.na_rows.items():
            lines[pos] = '\t'.join(line.rstrip('\n').split('\t')[:2] + ['NA'] * ncol) + '\n'
        for j, pos in enumerate(ts.order):
            lines[pos] = body[j]
    else:
        lines = body
    with open(path, 'w') as f:
        f.write('\t'.join(head) + '\n')
        f.writelines(lines)


def fetch_and_write(ctx, names, outfile, ts, grids):
    """After the observed scan of one file on ctx's selected slot: fetch every requested profile and write its file.
    grids: {'A': scan-order A grid, 'x': ..., 'abeta': ...}."""
    for name in names:
        grid = grids[name]
        prof = ctx.fetch_profile(name) if len(ts) else np.zeros((0, len(grid)))
        write_profile(output_name(outfile, name), name, ts, prof, grid)
