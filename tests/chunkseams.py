"""The listed-window calls across their chunk seams: the cases of tests/test_chunkseams_cpu.py (which shows on the host that every
case crosses the seam it is named for) and tests/test_gpu_chunk_seams.py (which runs them on the device), and a host restatement of
the six rules by which bmx_ctx_surfaces, _influence, _fit, _cond_surfaces and _base_surfaces cut their list into chunks.  numpy and
the package's pure-Python modules only; nothing is read from a file.

The rules (ballermixplus_amd/csrc/bmxscan.hip; LITERALS below are matched against the sources by the CPU module):
  1. surfaces_step, bytes     BMX_SURFACES_CHUNK_BYTES / (nA * npairs * 8) windows         surfaces, influence, cond_surfaces,
                                                                                                       base_surfaces
  2. surfaces_step, threads   (0xffffffff / 256) / (nA * nsl) windows, nsl = slices of 256 pairs           the same four
  3. influence, range pass    rstep = 1 << 20 windows
  4. influence, blocks        INFL_CHUNK_BLOCKS = 1 << 22 blocks per chunk, one window if it has more
  5. fit, outputs             (64 << 20) / (D * F * 20) windows
  6. fit, workspace           BMX_SURFACES_CHUNK_BYTES / (n_sizes * (F + 1) * 24) windows, when the sums do not fit BMX_FIT_LDS_BYTES

How a case is built.  K = 13 DISTINCT test sites with short index windows (thirteen(): at most 8 sites inside [lo, hi]), among them
an empty window, a window beside its test position, test positions on position ties, an off-site one and windows clipped at both
chromosome ends.  The list of a call is tests[q] = q mod 13, and every second array (lin, cond_test, cond_lin) gives entry q the
value of the distinct entry q mod 13.  13 divides no chunk length, so every chunk's buffers hold another rotation of the 13: a
chunk that read its list from offset 0 again, or wrote its results to offset 0 again, cannot give entry q the numbers of entry
q mod 13 of a call that lists the 13 once.

Cases (name: model, calls):
  bytes      gridshape 'small', 17 x 61 pairs (5 slices of 256), 64 A: one surface 530 944 bytes, step 505.  surfaces, influence
             (block 10^6 and 3) and cond_surfaces with T at n = step + 3; cond_surfaces without T at n = 2 step + 3 (three chunks);
             base_surfaces after one baseline_add the same two ways
  threads    one pair, 16 A: bytes 2 097 152, threads 1 048 575 windows.  surfaces and cond_surfaces at n = step + 5
  range      the same model.  influence, block 10^6, at n = 2^20 + 3: the range pass cuts at 2^20, the window chunks at 1 048 575
  blocks     one pair, one A that reaches across the 700 sites of chromosome 'S', whole-chromosome windows, block 1: about 700
             blocks per window; n is the first block-rule cut plus 16
  one_window a lattice of 2^22 + 70 000 sites with one position tie at the test site, one pair, one A that reaches across it,
             block 1: [a short window, the window over every site, a short window]; the long one is a chunk of its own
  fit_out    gridshape 'small', 3 x 3 pairs, F = D = 16: step 13 107, n = step + 3
  fit_ws     resamplers.table('t90831') (221 sample sizes), F = 10, D = 25: 58 344 bytes of sums per window, past
             BMX_FIT_LDS_BYTES; workspace step 4 600 below the output step 13 421; n = step + 3.  The same 13 with F = 6 fit LDS.
"""
import numpy as np

import gridshape as gs
import resamplers as rs

K = 13
HOST_CAP = 600 * 10 ** 6

# ------------------------------------------------------------------------------------------------ the shipped literals
CHUNK_BYTES = 256 << 20          # BMX_SURFACES_CHUNK_BYTES
SURFS_THREADS = 256
LAUNCH_THREADS = 0xffffffff
RANGE_STEP = 1 << 20
INFL_CHUNK_BLOCKS = 1 << 22
INFL_BLOCKS = 8
FIT_OUT_BYTES = 64 << 20
FIT_CELL_BYTES = 20              # int32 O, two doubles E per cell
FIT_LDS_BYTES = 40 << 10         # BMX_FIT_LDS_BYTES
FIT_SUM_BYTES = 24               # Gn, Gs, H: three doubles per (size block, class or total)
# (file, regular expression): each stands once in the source
LITERALS = [
    ('include/bmxscan.h', r'#define BMX_SURFACES_CHUNK_BYTES \(256LL << 20\)'),
    ('include/bmxscan.h', r'#define BMX_FIT_LDS_BYTES \(40 << 10\)'),
    ('ballermixplus_amd/csrc/bmxscan.hip', r'constexpr int SURFS_THREADS = 256;'),
    ('ballermixplus_amd/csrc/bmxscan.hip', r'constexpr int INFL_BLOCKS = 8;'),
    # 1. and 2.
    ('ballermixplus_amd/csrc/bmxscan.hip',
     r'chunk = \(int64_t\)std::max<size_t>\(BMX_SURFACES_CHUNK_BYTES / \(\(size_t\)c->nA \* c->npairs \* sizeof\(double\)\), 1\);\s*'
     r'return std::min\(chunk, std::max<int64_t>\(\(0xffffffffLL / SURFS_THREADS\) / \(\(int64_t\)c->nA \* nsl\), 1\)\);'),
    ('ballermixplus_amd/csrc/bmxscan.hip', r'const int nsl = \(c->npairs \+ SURFS_THREADS - 1\) / SURFS_THREADS;\s*const int64_t step = surfaces_step\(c, nsl\);'),
    # 3.
    ('ballermixplus_amd/csrc/bmxscan.hip', r'const int64_t rstep = 1 << 20;'),
    ('ballermixplus_amd/csrc/bmxscan.hip', r'for \(int64_t q0 = 0; q0 < n; q0 \+= rstep\) \{'),
    # 4.
    ('ballermixplus_amd/csrc/bmxscan.hip', r'const int64_t INFL_CHUNK_BLOCKS = 1 << 22;'),
    ('ballermixplus_amd/csrc/bmxscan.hip',
     r'int64_t m = 1;\s*while \(m < step && q0 \+ m < n && c->if_off\[\(size_t\)\(q0 \+ m \+ 1\)\] - c->if_off\[\(size_t\)q0\] <= INFL_CHUNK_BLOCKS\) m\+\+;'),
    # 5. and 6.
    ('ballermixplus_amd/csrc/bmxscan.hip', r'tab = \(size_t\)c->n_sizes \* \(F \+ 1\) \* 3;'),
    ('ballermixplus_amd/csrc/bmxscan.hip', r'in_lds = tab \* sizeof\(double\) <= \(size_t\)BMX_FIT_LDS_BYTES && c->variant != 1;'),
    ('ballermixplus_amd/csrc/bmxscan.hip', r'int64_t step = std::max<int64_t>\(\(64LL << 20\) / \(int64_t\)\(cells \* 20\), 1\);'),
    ('ballermixplus_amd/csrc/bmxscan.hip',
     r'if \(!in_lds\) step = std::min\(step, std::max<int64_t>\(BMX_SURFACES_CHUNK_BYTES / \(int64_t\)\(tab \* sizeof\(double\)\), 1\)\);'),
]
# how often the byte-and-thread step is taken: listed_surfaces (the loop of bmx_ctx_surfaces, _cond_surfaces and _base_surfaces) and
# bmx_ctx_influence
LITERAL_COUNTS = {5: 2}


# ------------------------------------------------------------------------------------------------ the rules, restated
def surfaces_step(nA, npairs):
    """(windows per chunk, by rule 1, by rule 2) of bmx_ctx_surfaces, _influence, _cond_surfaces and _base_surfaces."""
    nsl = -(-npairs // SURFS_THREADS)
    by_bytes = max(CHUNK_BYTES // (nA * npairs * 8), 1)
    by_threads = max((LAUNCH_THREADS // SURFS_THREADS) // (nA * nsl), 1)
    return min(by_bytes, by_threads), by_bytes, by_threads


def even_cuts(n, step):
    """The chunk lengths of a loop `for (q0 = 0; q0 < n; q0 += step)`."""
    return [min(step, n - q0) for q0 in range(0, n, step)]


def influence_cuts(blocks, step):
    """The window chunks of bmx_ctx_influence: blocks[q] = the blocks of window q's range; at most `step` windows and at most
    INFL_CHUNK_BLOCKS blocks per chunk, one window if it has more."""
    off = np.concatenate(([0], np.cumsum(np.asarray(blocks, dtype=np.int64))))
    n, q0, out = len(blocks), 0, []
    while q0 < n:
        e = int(np.searchsorted(off, off[q0] + INFL_CHUNK_BLOCKS, side='right')) - 1        # the last e with off[e] - off[q0] <= the cap
        m = min(max(e - q0, 1), step, n - q0)
        out.append(m)
        q0 += m
    return out


def fit_step(n_sizes, F, D, variant=0):
    """(windows per chunk, by rule 5, by rule 6, sums in LDS) of bmx_ctx_fit (before its min with n)."""
    tab = n_sizes * (F + 1) * FIT_SUM_BYTES
    in_lds = tab <= FIT_LDS_BYTES and variant != 1
    out = max(FIT_OUT_BYTES // (D * F * FIT_CELL_BYTES), 1)
    ws = max(CHUNK_BYTES // tab, 1)
    return (out if in_lds else min(out, ws)), out, ws, in_lds


def block_counts(gen, tg, lo, hi, A_min, zcut, block):
    """Blocks of every window's range (influence.py): from the block of its first to the block of its last site that qualifies at
    the smallest A, 0 without one.  B = min(block, N), as the library takes it."""
    gen = np.asarray(gen)
    N = len(gen)
    B = min(int(block), max(N, 1))
    out = np.zeros(len(tg), dtype=np.int64)
    for j, (t, a, b) in enumerate(zip(np.asarray(tg).tolist(), np.asarray(lo).tolist(), np.asarray(hi).tolist())):
        a, b = max(int(a), 0), min(int(b), N - 1)
        if b < a:
            continue
        g = gen[a:b + 1]
        at = np.flatnonzero((A_min * np.abs(g - t) <= zcut) & (g != t))
        if len(at):
            out[j] = (a + int(at[-1])) // B - (a + int(at[0])) // B + 1
    return out


# ------------------------------------------------------------------------------------------------ lists
def rotation(n):
    """tests[q] = q mod 13."""
    return (np.arange(n, dtype=np.int64) % K).astype(np.int32)


def along(values13, n):
    """A second array of a list of n: entry q gets the value of the distinct entry q mod 13."""
    v = np.asarray(values13, dtype=np.int32)
    assert len(v) == K
    return v[np.arange(n, dtype=np.int64) % K]


def fit_lins(points):
    """One grid point per distinct entry by fitcases.spread's rule (one point per window), entry 9 without one."""
    v = [(j * 7919 + 5) % points for j in range(K)]
    v[9] = -1
    return np.array(v, dtype=np.int32)


def cond_partners(points):
    """(cond_test[13], cond_lin[13]): every distinct entry given its right neighbour among the 13 (the last one the first) at a
    spread grid point; entry 11 without a conditioning site, entry 2 without a grid point."""
    ct = [(j + 1) % K for j in range(K)]
    cl = [(j * 7919 + 11) % points for j in range(K)]
    ct[11], cl[2] = -1, -1
    return np.array(ct, dtype=np.int32), np.array(cl, dtype=np.int32)


def base_locus(sc):
    """(test site, lin) of the ONE locus the base_surfaces calls put into the baseline: entry 5 of the 13 (site 1203, a position
    tie) held at the smallest A of the grid, which reaches every site of its window; entry 6's window (site 1206) overlaps it."""
    assert int(np.argmin(sc.As)) == 0
    return 5, 500 % sc.npairs


# ------------------------------------------------------------------------------------------------ scenes
class Scene:
    """A model, one chromosome and the 13 distinct test sites."""

    def __init__(self, name, model, xs, abetas, As, gen, rows, tg, lo, hi, kinds):
        self.name, self.model, self.xs, self.abetas, self.As = name, model, list(xs), list(abetas), [float(a) for a in As]
        self.gen, self.rows = np.ascontiguousarray(gen, dtype=np.float64), np.ascontiguousarray(rows, dtype=np.int32)
        self.tg, self.lo, self.hi = np.asarray(tg, dtype=np.float64), np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
        self.kinds = kinds                   # {'empty': j, 'beside': j, 'tie': j, 'off_site': j, 'clipped': (j, j)}
        self.nA, self.npairs = len(self.As), len(self.xs) * len(self.abetas)
        self.points = self.nA * self.npairs

    def context(self, eng):
        ctx = eng.Context(0)
        ctx.set_model(self.model, self.As)
        ctx.set_sites(self.gen, self.rows)
        ctx.set_tests(self.tg, self.lo, self.hi)
        return ctx

    def decode(self, lin):
        nx, nab = len(self.xs), len(self.abetas)
        return lin // (nx * nab), (lin // nab) % nx, lin % nab


def thirteen(gen):
    """(tg, lo, hi, kinds) of the 13 distinct test sites of a chromosome of about 4 000 sites with gridshape.POS_TIES: windows of
    at most 8 sites around the test site.  (Sites 710 and 3300 stand where 700 and 3700 first stood: on the 17 x 61 grid a block
    of each of those two windows leaves a best grid point that leads by less than the GPU tolerance.)"""
    N = len(gen)
    site = [2, 7, 300, 710, 1000, 1203, 1206, 1500, 2000, 2003, 2600, 3300, N - 1]
    assert all(j in gs.POS_TIES for j in (7, 1203, 2600)) and N > 3400
    tg = gen[site].copy()
    lo = np.array([s - 3 for s in site], dtype=np.int64)
    hi = np.array([s + 4 for s in site], dtype=np.int64)
    tg[3] = 0.5 * (gen[710] + gen[711])                      # off-site
    lo[4], hi[4] = 1003, 1000                                # empty
    lo[7], hi[7] = 1504, 1511                                # beside its test position
    lo[0], hi[0] = -3, 5                                     # clipped at the start
    lo[12], hi[12] = N - 5, N + 10                           # ... and at the end
    return tg, lo, hi, {'empty': 4, 'beside': 7, 'tie': 1, 'off_site': 3, 'clipped': (0, 12)}


def thirteen_whole(gen):
    """The 13 of chromosome 'S' (700 sites): whole-chromosome windows but for an empty one, one beside its test position and one
    given as [-5, 10 N]."""
    N = len(gen)
    site = [3, 7, 50, 120, 200, 260, 300, 350, 420, 480, 560, 640, N - 1]
    tg = gen[site].copy()
    lo, hi = np.zeros(K, dtype=np.int64), np.full(K, N - 1, dtype=np.int64)
    tg[3] = 0.5 * (gen[120] + gen[121])
    lo[4], hi[4] = 210, 190
    lo[6], hi[6] = 400, N - 1
    lo[12], hi[12] = -5, 10 * N
    return tg, lo, hi, {'empty': 4, 'beside': 6, 'tie': 1, 'off_site': 3, 'clipped': (12, 12)}


_SCENES = {}


def _gs_model(shape):
    from ballermixplus_amd import engine
    xs, abetas = gs.x_grid(shape[0]), gs.abeta_grid(shape[1])
    spect, props = gs.spectrum('small')
    return engine.ModelArrays('B2', 1, gs.sizes_of('small'), spect, props, xs, abetas), xs, abetas


def _gs_sites(model, n=None):
    gen, k, nn = gs.chromosome('small')
    rows = model.rows_of(k, nn)
    return (gen, rows) if n is None else (gen[:n], rows[:n])


A_WIDE = (200.0, 3e6)            # from every site of a short window down to none of them


def scene(name):
    if name not in _SCENES:
        _SCENES[name] = _BUILD[name]()
    return _SCENES[name]


def _bytes_scene():
    model, xs, abetas = _gs_model((17, 61))
    gen, rows = _gs_sites(model)
    return Scene('bytes', model, xs, abetas, np.geomspace(A_WIDE[0], A_WIDE[1], 64), gen, rows, *thirteen(gen))


def _one_pair_scene():
    model, xs, abetas = _gs_model((1, 1))
    gen, rows = _gs_sites(model)
    return Scene('one_pair', model, xs, abetas, np.geomspace(A_WIDE[0], A_WIDE[1], 16), gen, rows, *thirteen(gen))


BLOCKS_A = 1000.0


def _blocks_scene():
    model, xs, abetas = _gs_model((1, 1))
    gen, rows = _gs_sites(model, 700)
    return Scene('blocks', model, xs, abetas, [BLOCKS_A], gen, rows, *thirteen_whole(gen))


LATTICE_N = (1 << 22) + 70000
LATTICE_H = 2.0 ** -30
LATTICE_A = 4096.0               # A * (N - 1) * h = (N - 1) / 2^18 = 16.27: below the cut of 18.42 from either end
LATTICE_ROWS = 400               # the rows are those of the first 400 sites of the gridshape chromosome, over and over


def lattice(N):
    """(gen, index of the test site): a uniform lattice with one position tie, at the middle."""
    gen = np.arange(N, dtype=np.float64) * LATTICE_H
    c = N // 2
    gen[c + 1] = gen[c]
    return gen, c


def _lattice_scene(N=LATTICE_N, A=LATTICE_A):
    model, xs, abetas = _gs_model((1, 1))
    _, rows = _gs_sites(model, LATTICE_ROWS)
    gen, c = lattice(N)
    site = [1000, c, N - 2000]
    tg = gen[site]
    lo, hi = np.array([997, 0, N - 2003], dtype=np.int64), np.array([1004, N - 1, N - 1996], dtype=np.int64)
    return Scene('one_window', model, xs, abetas, [A], gen, np.resize(rows, N), tg, lo, hi, {'tie': 1})


def lattice_scene(N):
    """The one-window scene on a shorter lattice with the same reach in z (the CPU module's check of the vectorised restatement)."""
    return _lattice_scene(N, LATTICE_A * (LATTICE_N - 1) / (N - 1))


def _fit_out_scene():
    model, xs, abetas = _gs_model((3, 3))
    gen, rows = _gs_sites(model)
    return Scene('fit_out', model, xs, abetas, gs.A_LIST, gen, rows, *thirteen(gen))


def _fit_ws_scene():
    t = rs.table('t90831')
    gen, rows = t.sites(4000, 3)
    gen = gen.copy()
    for j in gs.POS_TIES:
        if j + 1 < len(gen):
            gen[j + 1] = gen[j]
    return Scene('fit_ws', t.model, rs.XS, rs.ABETAS, rs.NULL_AS, gen, rows, *thirteen(gen))


_BUILD = {'bytes': _bytes_scene, 'one_pair': _one_pair_scene, 'blocks': _blocks_scene, 'one_window': _lattice_scene,
          'fit_out': _fit_out_scene, 'fit_ws': _fit_ws_scene}


def fit_arrays(sc, F, D, zcut):
    """(gw, cls, edges) of a fit call on a scene's model."""
    from ballermixplus_amd import fit, power
    m = sc.model
    # (gridshape's spectrum holds one row at LOW_G = 8, no probability: bmx_ctx_fit refuses a gw above 1)
    gw = np.minimum(power.allowed_rows('B2', 1, m.sizes, m.row_off, m.g), 1.0)
    return gw, fit.classes('B2', m.sizes, m.row_off, F), fit.default_edges(D, zcut)


# ------------------------------------------------------------------------------------------------ cases
class Call:
    """One call of a case: op in ('surfaces', 'influence', 'cond', 'base', 'fit'), its list length n, the restated chunk lengths per loop
    ({'windows': [...]} and, for influence, {'range': [...]}), the bytes of its host outputs, and the op's own arguments."""

    def __init__(self, op, n, cuts, host_bytes, **kw):
        self.op, self.n, self.cuts, self.host_bytes, self.kw = op, int(n), cuts, int(host_bytes), kw

    def __repr__(self):
        return 'Call(%s, n=%d, %s, %s)' % (self.op, self.n, self.kw, {k: (len(v), v[0]) for k, v in self.cuts.items()})


def _surf_bytes(sc, n, T=True):
    return n * sc.nA * (sc.npairs * 8 * bool(T) + 4)


def _cond_bytes(sc, n, T=True):
    return _surf_bytes(sc, n, T) + n * (sc.nA * 4 + 12)


def _infl_bytes(n, blocks):
    return n * 32 + 8 + int(blocks) * 24


def _list_blocks(sc, n, block, zcut):
    per = block_counts(sc.gen, sc.tg, sc.lo, sc.hi, min(sc.As), zcut, block)
    return per[np.arange(n) % len(per)]


def bytes_case(zcut):
    sc = scene('bytes')
    step = surfaces_step(sc.nA, sc.npairs)[0]
    n = step + 3
    calls = [Call('surfaces', n, {'windows': even_cuts(n, step)}, _surf_bytes(sc, n))]
    for block in (10 ** 6, 3):
        b = _list_blocks(sc, n, block, zcut)
        calls.append(Call('influence', n, {'range': even_cuts(n, RANGE_STEP), 'windows': influence_cuts(b, step)}, _infl_bytes(n, b.sum()), block=block))
    calls.append(Call('cond', n, {'windows': even_cuts(n, step)}, _cond_bytes(sc, n), want_T=True))
    n3 = 2 * step + 3
    calls.append(Call('cond', n3, {'windows': even_cuts(n3, step)}, _cond_bytes(sc, n3, False), want_T=False))
    calls.append(Call('base', n, {'windows': even_cuts(n, step)}, _cond_bytes(sc, n), want_T=True))
    calls.append(Call('base', n3, {'windows': even_cuts(n3, step)}, _cond_bytes(sc, n3, False), want_T=False))
    return sc, calls


def threads_case(zcut):
    sc = scene('one_pair')
    step = surfaces_step(sc.nA, sc.npairs)[0]
    n = step + 5
    return sc, [Call('surfaces', n, {'windows': even_cuts(n, step)}, _surf_bytes(sc, n)),
                Call('cond', n, {'windows': even_cuts(n, step)}, _cond_bytes(sc, n), want_T=True)]


def range_case(zcut):
    sc = scene('one_pair')
    step = surfaces_step(sc.nA, sc.npairs)[0]
    n = RANGE_STEP + 3
    b = _list_blocks(sc, n, 10 ** 6, zcut)
    return sc, [Call('influence', n, {'range': even_cuts(n, RANGE_STEP), 'windows': influence_cuts(b, step)}, _infl_bytes(n, b.sum()), block=10 ** 6)]


def blocks_case(zcut):
    sc = scene('blocks')
    step = surfaces_step(sc.nA, sc.npairs)[0]
    per = block_counts(sc.gen, sc.tg, sc.lo, sc.hi, min(sc.As), zcut, 1)
    first = influence_cuts(per[np.arange(2 * INFL_CHUNK_BLOCKS // max(int(per.max()), 1)) % K], step)[0]
    n = first + 16
    b = per[np.arange(n) % K]
    return sc, [Call('influence', n, {'range': even_cuts(n, RANGE_STEP), 'windows': influence_cuts(b, step)}, _infl_bytes(n, b.sum()), block=1)]


def one_window_case(zcut):
    sc = scene('one_window')
    step = surfaces_step(sc.nA, sc.npairs)[0]
    b = block_counts(sc.gen, sc.tg, sc.lo, sc.hi, min(sc.As), zcut, 1)
    return sc, [Call('influence', 3, {'range': even_cuts(3, RANGE_STEP), 'windows': influence_cuts(b, step)}, _infl_bytes(3, b.sum()), block=1)]


def _fit_call(sc, F, D, n=None, variant=0):
    step = fit_step(len(sc.model.sizes), F, D, variant)[0]
    n = step + 3 if n is None else n
    return Call('fit', n, {'windows': even_cuts(n, min(step, n))}, n * (F * D * FIT_CELL_BYTES + 4), F=F, D=D, variant=variant)


def fit_out_case(zcut):
    sc = scene('fit_out')
    return sc, [_fit_call(sc, 16, 16)]


def fit_ws_case(zcut):
    sc = scene('fit_ws')
    return sc, [_fit_call(sc, 10, 25), _fit_call(sc, 6, 25, n=K), _fit_call(sc, 6, 25, n=K, variant=1)]


CASES = {'bytes': bytes_case, 'threads': threads_case, 'range': range_case, 'blocks': blocks_case, 'one_window': one_window_case,
         'fit_out': fit_out_case, 'fit_ws': fit_ws_case}
# the cases whose list is the rotation of the 13 (one_window lists its three windows once)
ROTATED = ('bytes', 'threads', 'range', 'blocks', 'fit_out', 'fit_ws')


# --------------------------------------------------------------------------------- the jackknife of a 1 x 1 x 1 grid, vectorised
def host_influence_one_point(gen, rows, Rcol, A, tg, lo, hi, zcut, block):
    """influence.host_influence for ONE pair and ONE A, from the definition in ballermixplus_amd/influence.py, in array operations
    over the sites (host_influence loops over the blocks in Python: minutes for four million of them).  Rcol[table rows]: the
    pair's column of the table.  Returns its dict (T 1 x 1 x 1, ns and n_b one row)."""
    g = np.asarray(gen, dtype=np.float64)
    N, B = len(g), int(block)
    a, b = max(int(lo), 0), min(int(hi), N - 1)
    out = {'T_max': 0.0, 'lin': -1, 'ns_min': 0, 'T': np.full((1, 1, 1), np.nan), 'ns': np.zeros(1, dtype=np.int32), 'first_block': 0,
           'n_b': np.zeros((1, 0), dtype=np.int64), 'm': np.zeros(0, np.int32), 'contrib': np.zeros(0), 'L': np.zeros(0),
           'blin': np.zeros(0, np.int32), 'margin': np.zeros(0)}
    if b < a:
        return out
    gw = g[a:b + 1]
    z = float(A) * np.abs(gw - tg)
    keep = (z <= zcut) & (gw != tg)
    ns = int(keep.sum())
    if not ns:
        return out
    idx = a + np.flatnonzero(keep)
    with np.errstate(divide='ignore', invalid='ignore'):
        term = np.log1p(np.exp(-z[keep]) * np.asarray(Rcol, dtype=np.float64)[np.asarray(rows)[idx]])
    T = 2.0 * float(np.sum(term))
    b0, b1 = int(idx[0]) // B, int(idx[-1]) // B
    nb = b1 - b0 + 1
    blk = idx // B - b0
    m = np.bincount(blk, minlength=nb)
    S = np.bincount(blk, weights=term, minlength=nb)
    T_max, lin = (T, 0) if T > 0 else (0.0, -1)
    cand = np.where(m > 0, T - 2.0 * S, T)
    cand[ns - m <= 0] = np.nan                              # an A without a site left is skipped
    with np.errstate(invalid='ignore'):
        won = cand > 0
    L = np.where(won, cand, 0.0)
    margin = np.where(won, L, np.where(np.isnan(cand), np.inf, -cand))
    contrib = 2.0 * S if lin >= 0 else np.full(nb, np.nan)
    out.update(T_max=T_max, lin=lin, ns_min=ns, T=np.full((1, 1, 1), T), ns=np.array([ns], dtype=np.int32), first_block=b0,
               n_b=m[None, :].astype(np.int64), m=m.astype(np.int32), contrib=contrib, L=L, blin=np.where(won, 0, -1).astype(np.int32),
               margin=margin, abs_sum=2.0 * float(np.sum(np.abs(term))))
    return out
