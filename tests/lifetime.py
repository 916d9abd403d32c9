"""One long-lived context against fresh ones: the inputs, the host model of the context's state and the op scripts of
tests/test_lifetime_cpu.py (which proves on the host that the scripts reach what they are named for) and tests/test_gpu_lifetime.py
(which runs every script in ONE engine.Context and compares every op, bit for bit, with a context created for that one comparison).
numpy and the package's pure-Python modules only; nothing is read from a file.

Models (name: table, pairs, slices, A values, table rows, row index width):
    g3x3     gridshape 'small' (n = 20), 3 x 3 pairs, 4 A             9 pairs, 1 slice, 21 rows in LDS, 2-byte rows
    g17x61   gridshape 'small', the (17, 61) shape, 3 A               1 037 pairs, 17 slices
    g1       gridshape 'small', fixX / fixAlpha, one A                1 x 1 x 1
    l2       gridshape 'large' (150, 160, 170), (5, 13), 2 A          483 rows: the table is read from L2, the <., false> kernels
    w4       resamplers.table('t90831'), 2 x 2 pairs, 2 A             90 831 rows: 4-byte row indices
    w729     offgrid's 'wide729' and its 'wideA' grid, 3 x 3, 2 A     729 rows: the first whose refinement workspace is in the slab
HAND_MODELS is the order of the hand-written script: pairs 9 -> 1037 -> 1 -> 65 -> 4 -> 9, slices 1 -> 17 -> 1 -> 2 -> 1, A values
4 -> 3 -> 1 -> 2 -> 2 -> 4, rows 21 -> 483 -> 90 831 -> 21, row width 2 -> 4 -> 2 bytes: each goes up and down.  w729 (HAND_TAIL)
follows in a last segment of its own and in the newest walks; its chromosomes are wide729's 1 500 sites ('M', 'L') and their first
500 ('S').  It is the one table on which the compass kernels and sandwich_kernel all work in rf_slab and are cheap (w4 is left out
of the off-grid searches).

Chromosomes of every model: 'S' 700, 'M' 4 003 (w4: 4 000) and 'L' 12 009 (12 000) sites, position ties as gridshape.POS_TIES (the
gridshape ones: the first 700 sites of gridshape.chromosome, the chromosome itself, and three seeds of it laid end to end).  Test
sites: a dense run of 613 (stride 1: prepared J = 16), every 5th site (prepared J = 8) and every 20th (solo), whole-chromosome or
ragged index windows (the recipe of gridshape.windows_of for any length).  COST_CAP keeps the product test sites x window x pairs x A
of a scan small: the long chromosomes are scanned with the cheap models or ragged windows.

fit and cond_surfaces (the groups 'fit' and 'conditional') take their lists as surfaces and influence do (index_list); fit's grid
points and cond_surfaces' conditioning sites and grid points follow fixed spread rules (fit_lins, cond_lists), gw is the world's
admissible weights (capped at 1: fit_gw), cls fit.classes and edges fit.default_edges of the op's (F, D) out of FIT_SHAPES.  On
w4 (221 sample sizes) F = 7 and F = 10 keep fit's prologue sums in the workspace in device memory, everything else in LDS.

The baseline calls (group 'baseline': baseline_reset, baseline_add, baseline_fetch, base_surfaces) and the sandwich calls (group
'sandwich': sandwich, refine_R).  Slot.bl is the baseline's history: None, or the loci added since the last reset, each with the
test site (tg, lo, hi) it was formed from, its grid point and the slot's permutation at the time; drop_sites() alone clears it
(set_sites, resample_sites and plant_sites into the slot, set_model), drop_tests(), permute_rows and restore_rows do not.
baseline_add spreads its two plain numbers over the test sites and the grid's points (baseline_locus; 'M' and 'top' are the bad
forms); base_surfaces lists as surfaces does.  sandwich lists as surfaces does, at one point per entry (sandwich_points: a grid
point by the spread rule, then eval_point's off-grid point inside the hull, alternating), with a block out of SANDWICH_BLOCKS (1
and 7: a thread per block; 64 and 10 ** 6: a wave per block); its bad forms are block = 0, hx = 0, x = HX / 2 and an index M.  The
workspace of sandwich_kernel is the refinement's: in LDS up to 728 table rows, in rf_slab on w729 and w4 (ws_in_lds).

Scripts: the hand-written one and seven seeded walks.  The three walks of OLD_WALK_SEEDS were drawn before fit and cond_surfaces had
ops and stay op for op what they were (walk() draws them from _WEIGHTS); the two of NEW_WALK_SEEDS draw from _NEW_WEIGHTS, which
weights those two ops 3 each, and stay what they were as well; the two of LIST_WALK_SEEDS draw from _LIST_WEIGHTS, which also
weights the six baseline and sandwich ops, and go on to the baseline a scanned slot lacks at BASELINE_RATE.  The hand-written script
keeps its earlier ops in order: the new ones are inserted and the segment on w729 stands behind them all
(tests/test_lifetime_cpu.py pins all six earlier scripts with a sha256).

An op is (name, {argument: plain value}); every array an op needs is derived from its plain arguments and the state by the
functions at the end of this module, so that a script is a list of small tuples that can be compared and printed.
"""
import numpy as np

import gridshape as gs
import resamplers as rs
import offgrid as og

from ballermixplus_amd import locate, null, power, sandwich

INVALID, LIMIT, STATE = -1, -4, -5
NAN = 'nan'                      # a NaN argument, spelt so that two scripts compare equal; float() of it is the NaN


def _isnan(v):
    return v == NAN

CODE_NAMES = {0: 'OK', INVALID: 'BMX_E_INVALID', LIMIT: 'BMX_E_LIMIT', STATE: 'BMX_E_STATE'}

# ------------------------------------------------------------------------------------------------ op groups (one line of the list each)
GROUPS = {
    'set_model': ('set_model',),
    'set_sites': ('set_sites',),
    'set_tests': ('set_tests',),
    'select_slot': ('select_slot',),
    'set_variant': ('set_variant',),
    'set_profiles': ('set_profiles', 'fetch_profile'),
    'scan': ('scan',),
    'scan_write': ('scan_write',),
    'permute': ('permute_rows', 'restore_rows'),
    'null': ('null_begin', 'null_accumulate', 'null_fetch'),
    'offgrid': ('refine', 'refine_at_peaks', 'fetch_refined', 'support', 'fetch_support', 'boot', 'fetch_boot', 'eval_points',
                'eval_points_weighted'),
    'peaks': ('peaks', 'peaks_track', 'fetch_peaks'),
    'surfaces': ('surfaces', 'influence'),
    'fit': ('fit',),
    'conditional': ('cond_surfaces',),
    'baseline': ('baseline_reset', 'baseline_add', 'baseline_fetch', 'base_surfaces'),
    'sandwich': ('sandwich', 'refine_R'),
    'locate': ('resample_sites', 'locate_begin', 'locate_accumulate', 'fetch_locate'),
    'plant': ('plant_sites', 'fetch_at'),
    'pack_records': ('pack_records',),
}
GROUP_OF = {name: g for g, names in GROUPS.items() for name in names}
# ops that compute or return something of their own: the GPU module compares it with a clean room.  The others (select_slot,
# set_variant, set_profiles, refine_at_peaks) only set a switch; what they change shows in the ops that follow.
VARIANTS = (0, 12, 16)           # default; the round-2 grouped kernel (no profile form); solo on request
NO_PROFILE_VARIANTS = (12,)
PROFILE_SETS = (0, 7, 1, 4)
CHUNKS = (0, 64, 1000)
LISTS = (1, 3, 40)
FIT_SHAPES = ((1, 1), (7, 6), (10, 25))          # (F, D) of a fit call: on w4 the last two keep their sums in the workspace home
FIT_LDS_BYTES = 40 << 10                         # BMX_FIT_LDS_BYTES: n_sizes * (F + 1) * 24 bytes of sums fit LDS up to here
FIT_BAD = ('F', 'lin', 'gw')                     # F = 0, lin = nA * npairs, gw[0] = 1.5: all BMX_E_INVALID
SANDWICH_BLOCKS = (1, 7, 64, 10 ** 6)             # a sandwich call's block: the first two a thread per block, the others a wave
SANDWICH_WAVE_BLOCK = 64                         # SANDWICH_WAVE_BLOCK of bmxscan.hip
SANDWICH_BAD = ('block', 'hx', 'x', 'index')     # block = 0, hx = 0, x = HX / 2, an index M: all BMX_E_INVALID
BASELINE_BAD = ('test', 'lin')                   # test = M, lin = nA * npairs: both BMX_E_INVALID
REFINE_LDS_WS = 32 << 10                         # REFINE_LDS_WS: a workspace of (rows * 45 + 15) // 16 * 16 bytes is in LDS up to here
STRIDES = (1, 5, 20)
WINDOWS = ('all', 'ragged')
MAX_SLOTS = 4096
ANCHOR_SLOT = MAX_SLOTS - 1      # no script selects it: the GPU module builds its base_surfaces anchor there, at the checkpoints
COST_CAP = 3e9
# the off-grid searches build the selection probabilities of every candidate point over all table rows: with 90 831 rows a
# refinement of a hundred windows takes seconds (tests/test_gpu_offgrid.py has that table); the scripts leave them out there
SLOW_OFFGRID = ('w4',)

# ------------------------------------------------------------------------------------------------ worlds
LENGTHS = {'S': 700, 'M': gs.N, 'L': 3 * gs.N}
W4_LENGTHS = {'S': 700, 'M': 4000, 'L': 12000}
W729_LENGTHS = {'S': 500, 'M': og.WIDE_N, 'L': og.WIDE_N}          # offgrid's 1 500 sites and their first 500
DENSE_M = gs.DENSE_M
MODEL_SPECS = {
    'g3x3': ('small', (3, 3), gs.A_LIST),
    'g17x61': ('small', (17, 61), (200.0, 5000.0, 30000.0)),
    'g1': ('small', (1, 1), (5000.0,)),
    'l2': ('large', (5, 13), (5000.0, 30000.0)),
    'w4': ('t90831', (2, 2), rs.NULL_AS),
    'w729': ('wide729', (3, 3), og.GRIDS['wideA'][2]),
}
SCAN_WORLDS = ('g3x3', 'g17x61', 'g1', 'l2', 'w4')       # the worlds of the earlier scripts: three chromosomes of rising length each
HAND_MODELS = ('g3x3', 'g17x61', 'g1', 'l2', 'w4', 'g3x3')
HAND_TAIL = 'w729'               # the model of the hand-written script's last segment, appended after the earlier ops
_WORLDS = {}


class World:
    """One model: the ModelArrays, its grids, the admissible weights of plant_sites and its three chromosomes."""

    def __init__(self, name):
        from ballermixplus_amd import engine
        data, shape, As = MODEL_SPECS[name]
        self.name, self.data, self.shape, self.As = name, data, shape, [float(a) for a in As]
        self.chroms = {}
        if data == 't90831':
            t = rs.table(data)
            self.model, self.xs, self.abetas = t.model, list(rs.XS), list(rs.ABETAS)
            self.neutral = (t.sizes, t.spect, t.props)              # (sample sizes, spectrum, shares): what util.oracle_R takes
            for c, n in W4_LENGTHS.items():
                gen, rows = t.sites(n, 3)
                gen = gen.copy()
                for j in gs.POS_TIES:
                    if j + 1 < n:
                        gen[j + 1] = gen[j]
                self.chroms[c] = (_frozen(gen), _frozen(np.asarray(rows, dtype=np.int32)))
        elif data == 'wide729':
            d = og.dataset(data)
            self.xs, self.abetas = list(og.GRIDS['wideA'][0]), list(og.GRIDS['wideA'][1])
            self.model = engine.ModelArrays('B2', 1, d.sizes, d.spect, d.props, self.xs, self.abetas)
            self.neutral = (d.sizes, d.spect, d.props)
            rows = np.asarray(og.rows_of(data), dtype=np.int32)
            self.chroms['S'] = (_frozen(d.gen[:W729_LENGTHS['S']]), _frozen(rows[:W729_LENGTHS['S']]))
            self.chroms['M'] = self.chroms['L'] = (_frozen(d.gen), _frozen(rows))
        else:
            self.xs, self.abetas = gs.x_grid(shape[0]), gs.abeta_grid(shape[1])
            spect, props = gs.spectrum(data)
            self.model = engine.ModelArrays('B2', 1, gs.sizes_of(data), spect, props, self.xs, self.abetas)
            self.neutral = (gs.sizes_of(data), spect, props)
            parts, at = [], 0.0
            for j in range(3):
                gen, k, nn = gs.chromosome(data, gs.SEED + j)
                parts.append((gen + at, self.model.rows_of(k, nn)))
                at += float(gen[-1]) + 2e-6
            self.chroms['S'] = (_frozen(parts[0][0][:LENGTHS['S']]), _frozen(parts[0][1][:LENGTHS['S']]))
            self.chroms['M'] = (_frozen(parts[0][0]), _frozen(parts[0][1]))
            self.chroms['L'] = (_frozen(np.concatenate([p[0] for p in parts])), _frozen(np.concatenate([p[1] for p in parts])))
        self.gw = power.allowed_rows('B2', 1, self.model.sizes, self.model.row_off, self.model.g)
        # bmx_ctx_fit refuses a gw above 1 (no probability): gridshape's spectrum holds one row at LOW_G = 8
        self.fit_gw = _frozen(np.minimum(self.gw, 1.0))
        self.nA, self.nx, self.nab = len(self.As), len(self.xs), len(self.abetas)
        self.cost = self.nA * self.nx * self.nab


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def world(name):
    if name not in _WORLDS:
        _WORLDS[name] = World(name)
    return _WORLDS[name]


def test_index(N, stride):
    """Site indices of the test sites of a stride in a chromosome of N sites."""
    if stride == 1:
        m = min(DENSE_M, N)
        a = gs.DENSE0 if N >= gs.N else (N - m) // 2
        return np.arange(a, a + m)
    return np.arange(0, N, stride)


def windows_of(gen, idx, windows):
    """(lo, hi) i64 of gridshape.windows_of's 'ragged' recipe for a chromosome of any length; (None, None) for 'all'."""
    if windows == 'all':
        return None, None
    N, M, r = len(gen), len(idx), gs.RAGGED_R
    rng = np.random.default_rng(gs.SEED + 1 + M)
    lo = np.minimum(np.maximum(idx - r, 0) + rng.integers(0, 2 * r, M), N - 1)
    hi = np.maximum(np.minimum(idx + r + 1, N - 1) - rng.integers(0, r, M), 0)
    for j in range(M):
        while 0 < lo[j] < N and gen[lo[j] - 1] == gen[lo[j]]:
            lo[j] -= 1
        while 0 <= hi[j] < N - 1 and gen[hi[j] + 1] == gen[hi[j]]:
            hi[j] += 1
    return _frozen(lo.astype(np.int64)), _frozen(hi.astype(np.int64))


def scan_cost(w, N, stride, windows):
    M = len(test_index(N, stride))
    return float(M) * (N if windows == 'all' else 2 * gs.RAGGED_R) * w.cost


# ------------------------------------------------------------------------------------------------ arrays of an op's plain arguments
def index_list(kind, M):
    """The window lists of surfaces / influence / fit / cond_surfaces / fetch_at: 1, 3 or 40 indices into M test sites, any order, with repeats."""
    base = (np.arange(kind, dtype=np.int64) * 7919 + 5) % max(M, 1)
    if kind >= 3:
        base[-1] = base[0]                                            # a repeat
    if kind >= 40:
        base[7], base[8] = M - 1, 0
    return base.astype(np.int32)


def fit_lins(kind, points):
    """One grid point per listed window by a fixed spread rule (tests/fitcases.spread's), the second entry without one."""
    v = (np.arange(kind, dtype=np.int64) * 7919 + 5) % points
    if kind >= 3:
        v[1] = -1
    return v.astype(np.int32)


def cond_lists(tests, M, points):
    """(cond_test, cond_lin) of a cond_surfaces call: the test site three further on (mod M), every fourth entry without one; a
    spread grid point, the third entry without one."""
    ct = (np.asarray(tests, dtype=np.int64) + 3) % max(M, 1)
    ct[3::4] = -1
    cl = (np.arange(len(ct), dtype=np.int64) * 7919 + 11) % points
    if len(cl) >= 3:
        cl[2] = -1
    return ct.astype(np.int32), cl.astype(np.int32)


def fit_in_lds(w, F):
    """Whether bmx_ctx_fit keeps the prologue sums of a window of this model in LDS (else in its workspace in device memory)."""
    return len(w.model.sizes) * (F + 1) * 24 <= FIT_LDS_BYTES


def spread(j, n):
    """The fixed spread rule of index_list and fit_lins for one plain number j: an index into n things."""
    return (int(j) * 7919 + 5) % max(int(n), 1)


def baseline_locus(a, M, points):
    """(test, lin) of a baseline_add op: its plain numbers spread over the M test sites and the grid's points; the bad forms
    'M' and 'top' are the first index past either."""
    return (M if a['test'] == 'M' else spread(a['test'], M)), (points if a['lin'] == 'top' else spread(a['lin'], points))


def sandwich_points(w, kind):
    """(A, x, abeta) f64[kind] of a sandwich call: the even entries a grid point by the spread rule, the odd ones eval_point's
    off-grid point inside the hull (the grid point itself where a grid has one value, as on g1)."""
    lin = (np.arange(kind, dtype=np.int64) * 7919 + 5) % (w.nA * w.nx * w.nab)
    pts = np.array([(w.As[l // (w.nx * w.nab)], w.xs[(l // w.nab) % w.nx], w.abetas[l % w.nab]) for l in lin.tolist()], dtype=np.float64)
    pts[1::2] = eval_point(w)
    return pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()


def refine_ws(rows):
    """Bytes of the workspace of refine_kernel, support_kernel, boot_kernel and sandwich_kernel (refine_workspace's expression)."""
    return (rows * 45 + 15) // 16 * 16


def ws_in_lds(w):
    return refine_ws(w.model.rows) <= REFINE_LDS_WS


def list_cost(w, N, windows, kind):
    """COST_CAP's product for a call that lists `kind` of the slot's windows (base_surfaces, sandwich)."""
    return float(kind) * (N if windows == 'all' else 2 * gs.RAGGED_R) * w.cost


def track_of(n, seed):
    """A caller's track for peaks_track: n rows, non-decreasing positions with ties, values with exact ties and zeros."""
    rng = np.random.default_rng([77, n, seed])
    g = np.cumsum(rng.integers(0, 3, n)) * 1e-5
    c = np.round(rng.gamma(2.0, 3.0, n), 1) * (rng.random(n) < 0.8)
    return g, c


def eval_point(w):
    """One off-grid point inside the model's hull (the grid point itself where a grid has one value)."""
    A = w.As[0] if w.nA == 1 else 0.5 * (min(w.As) + max(w.As))
    x = w.xs[0] if w.nx == 1 else 0.5 * (min(w.xs) + max(w.xs)) * 1.01
    ab = w.abetas[0] if w.nab == 1 else float(np.sqrt(min(w.abetas) * max(w.abetas))) * 1.1
    return float(A), float(x), float(ab)


def locate_ranges(K, step, width):
    lo = np.arange(K, dtype=np.int32) * step
    return lo, (lo + width - 1).astype(np.int32)


def plant_centres(gen, A, n):
    """n centres on sites of the chromosome, more than SPACING reaches apart (fewer if the chromosome is too short)."""
    gap = power.SPACING * power.ALPHA_CUT / A * 1.01
    out, at = [], float(gen[len(gen) // 5])
    while len(out) < n and at < gen[-1]:
        j = int(np.searchsorted(gen, at))
        out.append(float(gen[min(j, len(gen) - 1)]))
        at = out[-1] + gap
    return np.array(out, dtype=np.float64)


def boot_keys(key, R):
    return [null.mix(int(key) + r) for r in range(R)]


# ------------------------------------------------------------------------------------------------ the state model
class Slot:
    def __init__(self):
        self.sites = None        # {'gen', 'given', 'src'}: the arrays the slot holds, as given (before any permutation)
        self.perm = None         # (key, block) while the rows are permuted
        self.tests = None        # {'tg', 'lo', 'hi', 'stride', 'windows'}
        self.seq = 0             # scans launched in the slot
        self.scan = None         # the last scan's description (results exist), see State.describe
        self.pl = 0              # the profiles the last scan computed
        self.rf = self.sp = self.bt = self.pk = self.null = self.lc = None
        self.bl = None           # the baseline: None, or the loci added since the last reset, each {'tg', 'lo', 'hi', 'lin', 'perm'}:
        #                          the locus' test site as it was, its grid point and the slot's permutation when it was added

    def rows_now(self):
        g = self.sites['given']
        return g if self.perm is None else g[null.block_permutation(len(g), self.perm[0], self.perm[1])]

    def drop_tests(self):
        self.tests = self.scan = self.rf = self.sp = self.bt = self.pk = self.null = None
        self.pl = 0

    def drop_sites(self):                # (the one place that drops the baseline; drop_tests, permute and restore do not)
        self.sites = self.perm = self.bl = None
        self.drop_tests()

    @property
    def M(self):
        return 0 if self.tests is None else len(self.tests['tg'])


class State:
    """What include/bmxscan.h says a context holds after a history of calls.  step(op) returns 0 or the error code the header
    gives the call, and -- when the call succeeds -- updates the state, the expected site arrays included.  R_of(model name)
    -> R[nx][nab][rows] is needed by plant_sites alone (the oracle's table on the host, the device's own on the GPU)."""

    def __init__(self, R_of=None):
        self.model, self.variant, self.profiles, self.at_peaks, self.infl = None, 0, 0, False, False
        self.slots, self.cur, self.R_of = {0: Slot()}, 0, R_of

    @property
    def slot(self):
        return self.slots[self.cur]

    @property
    def w(self):
        return world(self.model)

    def ready(self):
        s = self.slot
        return self.model is not None and s.sites is not None and s.tests is not None

    def describe(self):
        """Everything a fresh context needs to repeat the selected slot's scan."""
        s = self.slot
        return {'model': self.model, 'gen': s.sites['gen'], 'given': s.sites['given'], 'perm': s.perm, 'tests': s.tests,
                'variant': self.variant, 'profiles': self.profiles}

    def refined_now(self):
        s = self.slot
        return self.model is not None and s.scan is not None and s.rf is not None and s.rf['seq'] == s.seq

    def predict(self, op):
        return self.step(op, commit=False)

    def step(self, op, commit=True):
        name, a = op
        return getattr(self, '_' + name)(a, commit)

    # ---- set-up
    def _set_model(self, a, commit):
        if a['model'] not in MODEL_SPECS:            # 'bad': an A grid with a 0
            return INVALID
        if commit:
            for s in self.slots.values():
                s.drop_sites()
                s.lc = None
            self.model = a['model']
        return 0

    def _set_sites(self, a, commit):
        if self.model is None:
            return STATE
        if a['chrom'] not in LENGTHS:                # 'bad': positions that descend
            return INVALID
        if commit:
            gen, rows = self.w.chroms[a['chrom']]
            self.slot.drop_sites()
            self.slot.sites = {'gen': gen, 'given': rows, 'src': a['chrom']}
        return 0

    def _set_tests(self, a, commit):
        s = self.slot
        if s.sites is None:
            return STATE
        if a['stride'] == 0:                         # 'bad': no test site
            return INVALID
        if commit:
            gen = s.sites['gen']
            idx = test_index(len(gen), a['stride'])
            lo, hi = windows_of(gen, idx, a['windows'])
            s.drop_tests()
            s.tests = {'tg': _frozen(gen[idx]), 'lo': lo, 'hi': hi, 'stride': a['stride'], 'windows': a['windows']}
        return 0

    def _select_slot(self, a, commit):
        if not 0 <= a['slot'] < MAX_SLOTS:
            return INVALID
        if commit:
            self.slots.setdefault(a['slot'], Slot())
            self.cur = a['slot']
        return 0

    def _set_variant(self, a, commit):
        if commit:
            self.variant = a['variant']
        return 0

    def _set_profiles(self, a, commit):
        if not 0 <= a['which'] <= 7:
            return INVALID
        if commit:
            self.profiles = a['which']
            if not a['which']:
                for s in self.slots.values():
                    s.pl = 0
        return 0

    def _fetch_profile(self, a, commit):
        return 0 if self.slot.scan is not None and self.slot.pl & a['which'] else STATE

    # ---- scans
    def _scan(self, a, commit):
        if not self.ready():
            return STATE
        if self.profiles and self.variant in NO_PROFILE_VARIANTS:
            return LIMIT
        if commit:
            s = self.slot
            s.seq += 1
            s.scan = self.describe()
            s.pl = self.profiles
        return 0

    _scan_write = _scan

    def _permute_rows(self, a, commit):
        if self.slot.sites is None:
            return STATE
        if a['block'] < 1:
            return INVALID
        if commit:
            self.slot.perm = (a['key'], a['block'])
        return 0

    def _restore_rows(self, a, commit):
        if self.slot.sites is None:
            return STATE
        if commit:
            self.slot.perm = None
        return 0

    # ---- permutation null
    def _null_begin(self, a, commit):
        s = self.slot
        if s.scan is None:
            return STATE
        if commit:
            s.null = {'seq': s.seq, 'obs': s.scan, 'reps': []}
        return 0

    def _null_accumulate(self, a, commit):
        s = self.slot
        if s.null is None or s.seq == s.null['seq']:
            return STATE
        if commit:
            s.null['reps'].append(s.scan)
            s.null['seq'] = s.seq
        return 0

    def _null_fetch(self, a, commit):
        return STATE if self.slot.null is None else 0

    # ---- refinement, support, bootstrap
    def _refine_at_peaks(self, a, commit):
        if commit:
            self.at_peaks = bool(a['on'])
        return 0

    def _refine(self, a, commit):
        s = self.slot
        if self.model is None or s.scan is None:
            return STATE
        if _isnan(a['min_clr']):
            return INVALID
        if self.at_peaks and not (s.pk is not None and s.pk['kind'] == 'scan' and s.pk['seq'] == s.seq and s.pk['M'] == s.M):
            return INVALID
        if commit:
            s.rf = {'seq': s.seq, 'scan': s.scan, 'min_clr': a['min_clr'], 'perm': s.perm, 'peaks': s.pk['args'] if self.at_peaks else None}
            s.sp = s.bt = None
        return 0

    def _fetch_refined(self, a, commit):
        return STATE if self.slot.rf is None else 0

    def _support(self, a, commit):
        if not self.refined_now():
            return STATE
        if not (a['drop'] > 0.0 and np.isfinite(a['drop'])) or _isnan(a['min_clr']):
            return INVALID
        if commit:
            self.slot.sp = {'drop': a['drop'], 'min_clr': a['min_clr'], 'perm': self.slot.perm}
        return 0

    def _fetch_support(self, a, commit):         # "a new scan, refinement, set_tests / set_sites / set_model drop the results"
        return 0 if self.slot.sp is not None and self.refined_now() else STATE

    def _boot(self, a, commit):
        if not self.refined_now():
            return STATE
        if a['R'] < 1 or a['block'] < 1 or _isnan(a['min_clr']):
            return INVALID
        if commit:
            s = self.slot
            s.bt = {'seq': s.seq, 'key': a['key'], 'R': a['R'], 'block': a['block'], 'min_clr': a['min_clr'], 'perm': s.perm}
        return 0

    def _fetch_boot(self, a, commit):
        s = self.slot
        return 0 if s.bt is not None and s.bt['seq'] == s.seq else STATE

    def _eval_points(self, a, commit):
        return 0 if self.ready() else STATE

    def _eval_points_weighted(self, a, commit):
        if not self.ready():
            return STATE
        return INVALID if a['block'] < 1 else 0

    # ---- peaks
    @staticmethod
    def _peak_args_bad(a):
        v = (a['sep'], a['min_clr'], a['frac'])
        return any(_isnan(x) for x in v) or not a['sep'] >= 0.0 or not 0.0 < a['frac'] <= 1.0

    def _peaks(self, a, commit):
        s = self.slot
        if self._peak_args_bad(a) or self.model is None or s.scan is None:
            return INVALID
        if commit:
            s.pk = {'kind': 'scan', 'seq': s.seq, 'scan': s.scan, 'M': s.M, 'args': (a['sep'], a['min_clr'], a['frac'])}
        return 0

    def _peaks_track(self, a, commit):
        if self._peak_args_bad(a):
            return INVALID
        if commit:
            self.slot.pk = {'kind': 'track', 'seq': None, 'M': a['n'], 'args': (a['sep'], a['min_clr'], a['frac']), 'track': (a['n'], a['seed'])}
        return 0

    def _fetch_peaks(self, a, commit):
        return STATE if self.slot.pk is None else 0

    # ---- surfaces, influence
    def _surfaces(self, a, commit):
        if not self.ready():
            return STATE
        return INVALID if a.get('bad') else 0

    def _influence(self, a, commit):
        if a['block'] < 1:
            return INVALID
        if not self.ready():
            return STATE
        if a.get('bad'):
            return INVALID
        if commit:
            self.infl = True
        return 0

    # ---- fit, cond_surfaces: list_ready's rule (model, sites and test sites, no scan); they commit nothing
    def _fit(self, a, commit):
        if a['F'] < 1:                               # the call's own argument refusal comes before the state's
            return INVALID
        if not self.ready():
            return STATE
        return INVALID if a.get('bad') else 0

    def _cond_surfaces(self, a, commit):
        if not self.ready():
            return STATE
        return INVALID if a.get('bad') else 0

    # ---- the baseline of accepted loci: the slot's own, dropped with its sites alone
    def _baseline_reset(self, a, commit):
        if self.slot.sites is None:
            return STATE
        if commit:
            self.slot.bl = []
        return 0

    def _baseline_add(self, a, commit):
        s = self.slot
        if not self.ready() or s.bl is None:
            return STATE
        w = self.w
        test, lin = baseline_locus(a, s.M, w.nA * w.nx * w.nab)
        if test >= s.M or lin >= w.nA * w.nx * w.nab:
            return INVALID
        if commit:
            t = s.tests
            s.bl = s.bl + [{'tg': float(t['tg'][test]), 'lo': None if t['lo'] is None else int(t['lo'][test]),
                            'hi': None if t['hi'] is None else int(t['hi'][test]), 'lin': lin, 'perm': s.perm}]
        return 0

    def _baseline_fetch(self, a, commit):
        return STATE if self.slot.sites is None or self.slot.bl is None else 0

    def _base_surfaces(self, a, commit):
        if not self.ready() or self.slot.bl is None:
            return STATE
        return INVALID if a.get('bad') else 0

    # ---- sandwich, refine_R: list_ready's rule after the call's own block and steps; they commit nothing
    def _sandwich(self, a, commit):
        if a['block'] < 1 or not a.get('hx', sandwich.HX) > 0.0:
            return INVALID
        if not self.ready():
            return STATE
        return INVALID if a.get('bad') else 0

    def _refine_R(self, a, commit):
        if not self.ready():
            return STATE
        return 0 if 0.0 < a['x'] < 1.0 and a['abeta'] > 0.0 else INVALID

    # ---- derived sites
    def _source(self, a):
        """(code, source slot) of resample_sites / plant_sites' src argument, before their own argument checks."""
        if self.model is None:
            return STATE, None
        if not 0 <= a['src'] < MAX_SLOTS or a['src'] == self.cur:
            return INVALID, None
        src = self.slots.get(a['src'])
        return 0, (src if src is not None and src.sites is not None else None)

    def _resample_sites(self, a, commit):
        code, src = self._source(a)
        if code:
            return code
        if a['block'] < 1:
            return INVALID
        if src is None:
            return STATE
        if commit:
            gen, rows = locate.resampled(src.sites['gen'], src.rows_now(), a['key'], a['block'])
            self.slot.drop_sites()
            if len(gen):
                self.slot.sites = {'gen': _frozen(gen), 'given': _frozen(rows.astype(np.int32)), 'src': ('resampled', a['src'])}
        return 0

    def plant_args(self, a, src):
        w = self.w
        A = w.As[a['iA']]
        return A, plant_centres(src.sites['gen'], A, a['K'])

    def _plant_sites(self, a, commit):
        code, src = self._source(a)
        if code:
            return code
        w = self.w
        if a['K'] < 0 or not (0 <= a['iA'] < w.nA and 0 <= a['ix'] < w.nx and 0 <= a['ia'] < w.nab):
            return INVALID
        if src is None:
            return STATE
        if commit:
            A, centres = self.plant_args(a, src)
            m = w.model
            rows = src.rows_now()
            R = self.R_of(self.model)
            if len(centres) and R is not None:       # (None: a script is being generated; no code depends on a planted slot's rows)
                rows = power.planted_rows(src.sites['gen'], rows, m.sizes, m.row_off, R[a['ix'], a['ia']], w.gw, A, centres, a['key'])[0]
            self.slot.drop_sites()
            self.slot.sites = {'gen': src.sites['gen'], 'given': _frozen(np.asarray(rows, dtype=np.int32)), 'src': ('planted', a['src'])}
        return 0

    def _fetch_at(self, a, commit):
        if self.slot.scan is None:
            return STATE
        return INVALID if a.get('bad') else 0

    # ---- position bootstrap
    def _locate_begin(self, a, commit):
        if a['K'] < 1 or a['R'] < 1:
            return INVALID
        if commit:
            s = self.slot
            s.lc = {'K': a['K'], 'step': a['step'], 'width': a['width'], 'R': a['R'], 'seq': s.seq, 'acc': [],
                    'top': (a['K'] - 1) * a['step'] + a['width']}
        return 0

    def _locate_accumulate(self, a, commit):
        s = self.slot
        if s.lc is None:
            return STATE
        if not 0 <= a['r'] < s.lc['R']:
            return INVALID
        if s.scan is None or s.seq == s.lc['seq']:
            return STATE
        if s.M < s.lc['top']:
            return INVALID
        if commit:
            s.lc['acc'].append((a['r'], s.scan))
            s.lc['seq'] = s.seq
        return 0

    def _fetch_locate(self, a, commit):
        return STATE if self.slot.lc is None else 0

    def _pack_records(self, a, commit):
        total = sum(s.M for s in self.slots.values() if s.scan is not None)
        return INVALID if a.get('short') and total > 0 else 0

    def with_results(self):
        return sorted(k for k, s in self.slots.items() if s.scan is not None)


# ops whose success leaves something to compare with a clean room (GPU module) -- all but the switches
COMPARED = tuple(n for n in GROUP_OF if n not in ('select_slot', 'set_variant', 'set_profiles', 'refine_at_peaks'))


def is_compared(o, st):
    """Whether the GPU module compares something with a clean room after this (successful) op; st: the state after it."""
    if o[0] == 'set_variant':
        return st.ready()                       # the plan
    if o[0] == 'select_slot':
        return st.slot.scan is not None         # the slot's results
    return o[0] in COMPARED


# ------------------------------------------------------------------------------------------------ scripts
def op(name, **a):
    return (name, a)


PEAKS = dict(sep=2e-4, min_clr=1.0, frac=0.5)


def _prepare(chrom, stride, windows):
    return [op('set_sites', chrom=chrom), op('set_tests', stride=stride, windows=windows), op('scan')]


# after a call that drops the slot's baseline: each of the three is BMX_E_STATE until the next baseline_reset
_REFUSED_BASELINE = [op('baseline_add', test=0, lin=0), op('baseline_fetch'), op('base_surfaces', kind=1, want_T=True)]
EMPTY_LOCUS = 1                  # spread(1, 801) = 715: a ragged window of the 'M' chromosome's every-5th test sites with lo > hi


def hand_script():
    """The required transitions, in the order of their list where the state allows it (tests/test_lifetime_cpu.py finds each one
    in the script itself); the fit and cond_surfaces ops (transition 13) stand among the surfaces and influence calls of 9. and 2.,
    the baseline and sandwich ops (14. to 22.) are inserted where the earlier ops bring the state they need about."""
    K1, K2 = 0x1234567890ABCDEF, 0x0FEDCBA987654321
    s = [op('scan'), op('set_sites', chrom='S'), op('scan_write', chunk=0), op('restore_rows'), op('null_begin'), op('eval_points'),
         op('fetch_peaks'),                                                          # all refused: nothing is set
         op('baseline_reset'), op('sandwich', kind=1, block=1), op('refine_R', x=0.31, abeta=7.0),
         op('set_model', model='g3x3'),
         op('fit', kind=1, F=1, D=1), op('cond_surfaces', kind=1, want_T=True),         # refused: no sites yet
         op('baseline_add', test=0, lin=0), op('baseline_fetch'), op('base_surfaces', kind=1, want_T=True), op('sandwich', kind=3, block=7)]
    # 1. one slot long -> short -> medium, M large -> small -> larger
    #    17. a baseline at each length, fetched; 15. set_sites meets the long one: add, fetch and base_surfaces refuse until the reset
    s += _prepare('L', 5, 'all') + [op('baseline_fetch'), op('baseline_reset'), op('baseline_add', test=2, lin=5), op('baseline_fetch'),
                                    op('base_surfaces', kind=3, want_T=True), op('sandwich', kind=3, block=64)]
    s += _prepare('S', 20, 'ragged') + _REFUSED_BASELINE + [op('baseline_reset'), op('base_surfaces', kind=3, want_T=False),
                                                            op('baseline_add', test=1, lin=3), op('baseline_fetch')]
    s += _prepare('M', 5, 'ragged') + [op('baseline_reset'), op('baseline_fetch')]
    # 14. the plain chain (two loci on one test site: cnt = 2), then one locus whose window is empty: it writes nothing
    #     22. a refused op directly before a compared one of its group
    s += [op('baseline_reset'), op('baseline_add', test=7, lin=0), op('baseline_add', test=7, lin=1), op('base_surfaces', kind=40, want_T=True),
          op('base_surfaces', kind=1, want_T=False), op('baseline_fetch'), op('baseline_reset'), op('baseline_fetch'),
          op('baseline_add', test='M', lin=0), op('baseline_add', test=7, lin=2), op('baseline_add', test=0, lin='top'),
          op('baseline_add', test=EMPTY_LOCUS, lin=4), op('base_surfaces', kind=3, want_T=True, bad=True), op('base_surfaces', kind=3, want_T=True),
          op('baseline_add', test=9, lin=7)]
    #     16. that baseline (three loci, one of them empty) now meets scans, set_profiles and set_variant
    # 3. the same test sites under profiles 0 -> 7 -> 1 -> 0 and variants 0 -> 12 -> 0 (and the LIMIT refusal in between)
    s += [op('set_profiles', which=7), op('scan'), op('fetch_profile', which=2), op('set_profiles', which=1), op('scan'),
          op('fetch_profile', which=4), op('set_variant', variant=12), op('set_profiles', which=8), op('scan'),
          op('set_profiles', which=0), op('scan'), op('set_variant', variant=16), op('scan'), op('set_variant', variant=0), op('scan')]
    s += [op('base_surfaces', kind=3, want_T=True), op('baseline_fetch'),
          # 19. the plain sandwich chain on a model in LDS, all four blocks; 22. each refusal directly before a compared call
          op('sandwich', kind=40, block=1), op('sandwich', kind=1, block=7), op('sandwich', kind=3, block=0), op('sandwich', kind=1, block=64),
          op('sandwich', kind=3, block=7, hx=0.0), op('sandwich', kind=40, block=10 ** 6), op('sandwich', kind=3, block=7, bad='x'),
          op('sandwich', kind=3, block=7), op('sandwich', kind=3, block=64, bad='index'), op('sandwich', kind=3, block=64),
          op('refine_R', x=1.0, abeta=7.0), op('refine_R', x=0.31, abeta=7.0)]
    # 10. scan_write on a small M, on a larger M in another slot, then a plain scan of the first
    #     17. a second slot with a baseline of another length (700 sites against slot 0's 4 003)
    s += [op('select_slot', slot=1), op('set_sites', chrom='S'), op('set_tests', stride=20, windows='all'), op('scan_write', chunk=64),
          op('baseline_reset'), op('baseline_add', test=3, lin=8), op('baseline_add', test=4, lin=20), op('base_surfaces', kind=3, want_T=True),
          op('select_slot', slot=2), op('set_sites', chrom='M'), op('set_tests', stride=1, windows='all'), op('scan_write', chunk=1000),
          op('select_slot', slot=1), op('scan'), op('set_variant', variant=12), op('set_profiles', which=2), op('scan_write', chunk=64),
          op('set_profiles', which=0), op('scan_write', chunk=0), op('set_variant', variant=0)]
    # 11. pack_records after one of three slots has lost its results to set_tests
    s += [op('pack_records'), op('select_slot', slot=MAX_SLOTS), op('select_slot', slot=2), op('set_tests', stride=5, windows='ragged'), op('pack_records', short=True),
          op('pack_records'), op('scan')]
    # 4. permute -> scan -> resample and plant into other slots from the permuted source -> restore -> scan
    #    16. slot 0's baseline after set_tests, on permuted rows (a locus is added there) and restored ones; 21. sandwich on both
    #    15. resample_sites into slot 1 drops its baseline, the source's (slot 0) is unchanged
    s += [op('select_slot', slot=0), op('baseline_fetch'), op('base_surfaces', kind=1, want_T=True),
          op('set_tests', stride=5, windows='all'), op('base_surfaces', kind=3, want_T=True), op('scan'), op('permute_rows', key=K1, block=0),
          op('permute_rows', key=K1, block=7), op('base_surfaces', kind=3, want_T=True), op('sandwich', kind=3, block=7),
          op('baseline_add', test=11, lin=30), op('scan'),
          op('select_slot', slot=1), op('resample_sites', src=1, key=K2, block=5), op('resample_sites', src=0, key=K2, block=5)]
    s += _REFUSED_BASELINE + [op('baseline_reset'),
          op('set_tests', stride=5, windows='all'), op('base_surfaces', kind=3, want_T=True), op('scan'),
          op('select_slot', slot=3), op('plant_sites', src=0, key=K2, K=2, iA=4, ix=0, ia=0),
          op('plant_sites', src=0, key=K2, K=2, iA=3, ix=1, ia=2), op('set_tests', stride=20, windows='all'), op('scan'),
          op('fetch_at', kind=40, bad=True), op('fetch_at', kind=40),
          op('select_slot', slot=0), op('baseline_fetch'), op('restore_rows'), op('base_surfaces', kind=3, want_T=True),
          op('sandwich', kind=3, block=7), op('baseline_fetch'), op('scan')]
    # 5. two null runs on one slot, the second with fewer replicates; then set_tests and a third
    s += [op('null_accumulate'), op('null_begin'), op('null_accumulate')]
    for r in range(3):
        s += [op('permute_rows', key=K1 + r, block=3), op('scan'), op('null_accumulate')]
    s += [op('null_fetch'), op('restore_rows'), op('scan'), op('null_begin'), op('permute_rows', key=K2, block=1), op('scan'),
          op('null_accumulate'), op('null_fetch'), op('restore_rows'), op('set_tests', stride=20, windows='ragged'),
          op('base_surfaces', kind=3, want_T=False), op('baseline_add', test=13, lin=17), op('base_surfaces', kind=1, want_T=True),  # 16.
          op('null_fetch'),
          op('scan'), op('null_begin'), op('permute_rows', key=K2 + 1, block=2), op('scan'), op('null_accumulate'), op('null_fetch'),
          op('restore_rows')]
    # 6. a locate run K x R fully accumulated, then a smaller one in which one replicate is never accumulated
    s += [op('select_slot', slot=1), op('fetch_locate'), op('locate_begin', K=5, step=20, width=30, R=0),
          op('locate_begin', K=5, step=20, width=30, R=3)]
    for r in range(3):
        s += [op('resample_sites', src=0, key=K1 + 10 + r, block=5), op('set_tests', stride=5, windows='all'), op('scan'),
              op('locate_accumulate', r=r)]
    s += [op('fetch_locate'), op('locate_begin', K=2, step=15, width=40, R=2), op('locate_accumulate', r=1), op('scan'),
          op('locate_accumulate', r=2), op('locate_accumulate', r=1), op('fetch_locate')]
    # 7. refine -> new scan on permuted rows -> support / boot refuse, fetch_refined still answers -> refine -> support -> boot
    s += [op('select_slot', slot=0), op('set_tests', stride=20, windows='ragged'), op('scan'), op('fetch_refined'), op('refine', min_clr=2.0),
          op('sandwich', kind=3, block=1),                                                                  # 20. between the compass calls
          op('support', drop=1.0, min_clr=60.0), op('fetch_support'), op('permute_rows', key=K1, block=4), op('scan'),
          op('support', drop=1.0, min_clr=60.0), op('boot', key=K2, R=3, block=8, min_clr=60.0), op('fetch_refined'), op('fetch_support'),
          op('fetch_boot'), op('refine', min_clr=NAN), op('refine', min_clr=2.0), op('sandwich', kind=1, block=64), op('support', drop=0.0, min_clr=60.0),
          op('support', drop=1.0, min_clr=60.0), op('sandwich', kind=3, block=7), op('fetch_support'), op('boot', key=K2, R=3, block=0, min_clr=60.0),
          op('boot', key=K2, R=3, block=8, min_clr=60.0), op('sandwich', kind=40, block=10 ** 6), op('fetch_boot'), op('eval_points'),
          op('eval_points_weighted', key=K1, block=0),
          op('eval_points_weighted', key=K1, block=6), op('restore_rows')]
    # 8. peaks -> refine_at_peaks -> scan -> refine refuses; a peaks_track of another length does not count; peaks -> refine
    s += [op('scan'), op('peaks', sep=2e-4, min_clr=1.0, frac=0.0), op('peaks', **PEAKS), op('fetch_peaks'), op('refine_at_peaks', on=True),
          op('scan'), op('refine', min_clr=0.0), op('peaks_track', n=300, seed=1, sep=NAN, min_clr=1.0, frac=0.5),
          op('peaks_track', n=300, seed=1, **PEAKS), op('fetch_peaks'), op('refine', min_clr=0.0),
          op('peaks', **PEAKS), op('refine', min_clr=0.0), op('sandwich', kind=3, block=7), op('fetch_refined'), op('refine_at_peaks', on=False)]
    # 9. surfaces and influence with 40 windows, then 1, then again after every change of the model's shape
    #    13. fit and cond_surfaces with 40 windows, then 1, directly after surfaces and influence calls with longer and shorter lists
    #    18. base_surfaces directly after each of the four with a longer and with a shorter list
    s += [op('surfaces', kind=40), op('fit', kind=1, F=7, D=6), op('base_surfaces', kind=40, want_T=True),
          op('influence', kind=40, block=50), op('cond_surfaces', kind=1, want_T=True), op('base_surfaces', kind=3, want_T=False),
          op('fit', kind=40, F=10, D=25), op('base_surfaces', kind=1, want_T=True), op('cond_surfaces', kind=40, want_T=True),
          op('base_surfaces', kind=3, want_T=True),
          op('surfaces', kind=1, bad=True), op('surfaces', kind=1), op('base_surfaces', kind=40, want_T=False),
          op('cond_surfaces', kind=40, want_T=False), op('fit', kind=1, F=1, D=1),
          op('influence', kind=3, block=0), op('influence', kind=1, block=50), op('fit', kind=40, F=1, D=1), op('fit', kind=3, F=0, D=6),
          op('fit', kind=3, F=7, D=6), op('fit', kind=3, F=7, D=6, bad='lin'), op('fit', kind=1, F=10, D=25), op('fit', kind=40, F=7, D=6, bad='gw'),
          op('cond_surfaces', kind=3, want_T=True, bad=True), op('cond_surfaces', kind=1, want_T=False), op('cond_surfaces', kind=3, want_T=True)]
    # 2. the models, each with a scan (and the 4-byte rows between two scans on 2-byte rows); every other slot's sites are gone
    for m in HAND_MODELS[1:]:
        #    15. set_model meets slot 0's baseline; 14. and 19. the plain chains again under every model; 21. refine_R across it
        s += [op('refine_R', x=0.31, abeta=7.0), op('set_model', model='bad'), op('set_model', model=m)] + _REFUSED_BASELINE
        s += [op('select_slot', slot=2), op('set_tests', stride=5, windows='all'),
              op('select_slot', slot=0)]
        s += _prepare('M', 1, 'ragged') + [op('baseline_reset'), op('baseline_add', test=2, lin=0), op('baseline_add', test=3, lin=1),
                                          op('surfaces', kind=40), op('cond_surfaces', kind=3, want_T=False),
                                          op('base_surfaces', kind=40, want_T=m != 'g17x61'),
                                          op('influence', kind=40, block=64), op('base_surfaces', kind=1, want_T=m == 'g17x61'),
                                          op('fit', kind=3, F=1, D=1),
                                          op('influence', kind=1, block=64), op('cond_surfaces', kind=40, want_T=True),
                                          op('fit', kind=40, F=7, D=6), op('fit', kind=1, F=10, D=25), op('cond_surfaces', kind=1, want_T=False),
                                          op('baseline_fetch'), op('baseline_reset'), op('baseline_fetch'), op('baseline_add', test=5, lin=2),
                                          op('refine_R', x=0.31, abeta=7.0),
                                          op('sandwich', kind=40, block=1), op('sandwich', kind=1, block=7), op('sandwich', kind=1, block=64),
                                          op('sandwich', kind=40, block=10 ** 6),
                                          op('select_slot', slot=1)] + _prepare('S', 5, 'all')
        s += [op('set_profiles', which=4), op('permute_rows', key=K1, block=2), op('scan'), op('fetch_profile', which=1),
              op('fetch_profile', which=4), op('set_profiles', which=0)]
        if m not in SLOW_OFFGRID:
            s += [op('refine', min_clr=5.0)]
            if m != 'l2':        # (483 rows: the searches' per-candidate table makes these two the script's slowest ops)
                s += [op('support', drop=1.0, min_clr=60.0), op('boot', key=K1, R=2, block=16, min_clr=60.0)]
        s += [op('restore_rows'),
              op('select_slot', slot=4), op('select_slot', slot=MAX_SLOTS), op('resample_sites', src=1, key=K2, block=3),
              op('set_tests', stride=20, windows='all'), op('scan_write', chunk=0), op('peaks', **PEAKS), op('pack_records'),
              op('select_slot', slot=0)]
    return s + _hand_tail(K1, K2)


def _hand_tail(K1, K2):
    """The last segment, on the 729-row table: the smallest whose workspace leaves LDS, so that the compass kernels and
    sandwich_kernel meet in rf_slab (20.), and the one place where plant_sites meets a baseline (15.).  It stands after every
    earlier op; tests/test_lifetime_cpu.py cuts the script at its set_model before it takes the sha256."""
    t = [op('refine_R', x=0.31, abeta=7.0), op('set_model', model=HAND_TAIL)] + _REFUSED_BASELINE
    t += _prepare('M', 20, 'all') + [op('refine_R', x=0.31, abeta=7.0), op('baseline_reset'), op('baseline_add', test=1, lin=1),
                                       op('baseline_add', test=2, lin=2), op('base_surfaces', kind=40, want_T=True),
                                       op('base_surfaces', kind=1, want_T=False), op('baseline_fetch'), op('baseline_reset'),
                                       op('baseline_fetch'), op('baseline_add', test=1, lin=1), op('baseline_add', test=2, lin=2)]
    t += [op('refine', min_clr=5.0), op('sandwich', kind=40, block=1), op('fetch_refined'), op('support', drop=1.0, min_clr=60.0),
          op('sandwich', kind=1, block=7), op('fetch_support'), op('boot', key=K1, R=2, block=16, min_clr=60.0),
          op('sandwich', kind=1, block=64), op('fetch_boot'), op('eval_points'), op('sandwich', kind=40, block=10 ** 6), op('eval_points'),
          op('permute_rows', key=K2, block=9), op('sandwich', kind=3, block=7), op('restore_rows'), op('sandwich', kind=3, block=7)]
    t += [op('select_slot', slot=1), op('set_sites', chrom='S'), op('baseline_reset'), op('baseline_add', test=0, lin=0), op('baseline_fetch'),
          op('set_tests', stride=5, windows='all'), op('baseline_add', test=0, lin=0), op('baseline_fetch'),
          op('plant_sites', src=0, key=K2, K=0, iA=1, ix=1, ia=1)] + _REFUSED_BASELINE
    t += [op('baseline_reset'), op('set_tests', stride=20, windows='all'), op('base_surfaces', kind=3, want_T=True), op('scan'),
          op('select_slot', slot=0), op('baseline_fetch'), op('base_surfaces', kind=3, want_T=True), op('scan')]
    return t


OLD_WALK_SEEDS = (20261101, 20261102, 20261103)               # drawn before fit and cond_surfaces had ops: they stay what they were
NEW_WALK_SEEDS = (20261105, 20261110)                         # drawn from the table that also weights the two (the first two seeds
#                                                               after the earlier ones whose walk has both ops succeed twice, one of
#                                                               them on the workspace home of w4; tests/test_lifetime_cpu.py asserts it)
LIST_WALK_SEEDS = (20261506, 20266493)                        # drawn from the table that also weights the baseline and sandwich ops: the first seed
#                                                               after the earlier ones, for either tuple of LIST_WALK_MODELS, whose walk has all
#                                                               six succeed twice (tests/test_lifetime_cpu.py asserts it)
WALK_SEEDS = OLD_WALK_SEEDS + NEW_WALK_SEEDS + LIST_WALK_SEEDS
NEW_OPS = ('fit', 'cond_surfaces')
LIST_OPS = GROUPS['baseline'] + GROUPS['sandwich']
WALK_LENGTH = 88
WALK_SLOTS = (0, 1, 2)
WALK_MODELS = {20261101: ('g3x3', 'l2', 'g1', 'g17x61'), 20261102: ('w4', 'g3x3', 'g17x61', 'l2'), 20261103: ('g17x61', 'g1', 'w4', 'g3x3'),
               20261105: ('w4', 'g1', 'l2', 'g17x61'), 20261110: ('g1', 'w4', 'g3x3', 'l2')}
BAD_SHARE = 0.07                 # deliberately bad arguments; refusals by state come on top (kept with probability KEEP_REFUSED)
KEEP_REFUSED = 0.3
BASELINE_RATE = 0.4             # how often the newest walks turn to the baseline a scanned slot lacks, then to its first locus

_WEIGHTS = {'set_sites': 4, 'set_tests': 6, 'select_slot': 6, 'set_variant': 3, 'set_profiles': 4, 'fetch_profile': 5, 'scan': 14,
            'scan_write': 3, 'permute_rows': 4, 'restore_rows': 2, 'null_begin': 2, 'null_accumulate': 3, 'null_fetch': 2, 'refine': 4,
            'refine_at_peaks': 1, 'fetch_refined': 1, 'support': 2, 'fetch_support': 1, 'boot': 2, 'fetch_boot': 1, 'eval_points': 2,
            'eval_points_weighted': 2, 'peaks': 3, 'peaks_track': 2, 'fetch_peaks': 1, 'surfaces': 3, 'influence': 3,
            'resample_sites': 3, 'locate_begin': 2, 'locate_accumulate': 3, 'fetch_locate': 2, 'plant_sites': 3, 'fetch_at': 3,
            'pack_records': 3}
_NEW_WEIGHTS = dict(_WEIGHTS, fit=3, cond_surfaces=3)
_LIST_WEIGHTS = dict(_NEW_WEIGHTS, baseline_reset=2, baseline_add=4, base_surfaces=3, baseline_fetch=2, sandwich=3, refine_R=1)
LIST_WALK_MODELS = (('g3x3', 'w729', 'w4', 'g17x61'), ('w4', 'g1', 'w729', 'l2'))       # of LIST_WALK_SEEDS, in their order


def _listed_kinds(st):
    """The list lengths of a base_surfaces or sandwich op that COST_CAP's product allows on the selected slot's windows."""
    s = st.slot
    if s.sites is None or s.tests is None:
        return LISTS
    return tuple(k for k in LISTS if list_cost(st.w, len(s.sites['gen']), s.tests['windows'], k) <= COST_CAP) or LISTS[:1]


def _draw(rng, st, name):
    """One op of that name with seeded arguments; with probability BAD_SHARE an argument the header refuses."""
    bad = rng.random() < BAD_SHARE
    pick = lambda v: v[int(rng.integers(len(v)))]
    key = int(rng.integers(1, 2 ** 62))
    others = [k for k in WALK_SLOTS if k != st.cur]
    if name == 'set_sites':
        return op(name, chrom='bad' if bad else pick('SML'))
    if name == 'set_tests':
        if bad or st.slot.sites is None:
            return op(name, stride=0 if bad else 5, windows='all')
        N = len(st.slot.sites['gen'])
        ok = [(s, w) for s in STRIDES for w in WINDOWS if scan_cost(st.w, N, s, w) <= COST_CAP]
        s, w = pick(ok)
        return op(name, stride=s, windows=w)
    if name == 'select_slot':
        new = [k for k in others if k not in st.slots]          # every slot of the walk is visited early
        return op(name, slot=MAX_SLOTS if bad else new[0] if new else pick(others))
    if name == 'set_variant':
        return op(name, variant=pick(VARIANTS))
    if name == 'set_profiles':
        return op(name, which=8 if bad else pick(PROFILE_SETS))
    if name == 'fetch_profile':
        return op(name, which=pick((1, 2, 4)))
    if name == 'scan_write':
        return op(name, chunk=pick(CHUNKS))
    if name == 'permute_rows':
        return op(name, key=key, block=0 if bad else pick((1, 3, 16, 100000)))
    if name == 'refine':
        return op(name, min_clr=NAN if bad else pick((0.0, 5.0)))
    if name == 'refine_at_peaks':
        return op(name, on=not st.at_peaks)
    if name == 'support':
        return op(name, drop=0.0 if bad else 1.0, min_clr=pick((60.0, 100.0)))
    if name == 'boot':
        return op(name, key=key, R=pick((1, 3)), block=0 if bad else pick((4, 32)), min_clr=pick((60.0, 100.0)))
    if name == 'eval_points_weighted':
        return op(name, key=key, block=0 if bad else pick((1, 9)))
    if name == 'peaks':
        return op(name, sep=pick((0.0, 2e-4)), min_clr=pick((0.0, 2.0)), frac=0.0 if bad else pick((0.5, 1.0)))
    if name == 'peaks_track':
        return op(name, n=pick((0, 50, 700)), seed=int(rng.integers(100)), sep=NAN if bad else 3e-5, min_clr=1.0, frac=0.5)
    if name in ('surfaces', 'fetch_at'):
        return op(name, kind=pick(LISTS), **({'bad': True} if bad else {}))
    if name == 'influence':
        blk = 0 if bad and rng.random() < 0.5 else pick((16, 200))
        return op(name, kind=pick(LISTS), block=blk, **({'bad': True} if bad and blk else {}))
    if name == 'fit':
        F, D = pick(FIT_SHAPES)
        how = pick(FIT_BAD) if bad else None
        return op(name, kind=pick(LISTS), F=0 if how == 'F' else F, D=D, **({'bad': how} if how in ('lin', 'gw') else {}))
    if name == 'cond_surfaces':
        return op(name, kind=pick(LISTS), want_T=bool(pick((True, False))), **({'bad': True} if bad else {}))
    if name == 'baseline_add':
        how = pick(BASELINE_BAD) if bad else None
        return op(name, test='M' if how == 'test' else int(rng.integers(6)), lin='top' if how == 'lin' else int(rng.integers(50)))
    if name == 'base_surfaces':
        return op(name, kind=pick(_listed_kinds(st)), want_T=bool(pick((True, False))), **({'bad': True} if bad else {}))
    if name == 'sandwich':
        how = pick(SANDWICH_BAD) if bad else None
        return op(name, kind=pick(_listed_kinds(st)), block=0 if how == 'block' else pick(SANDWICH_BLOCKS), **({'hx': 0.0} if how == 'hx' else {}),
                  **({'bad': how} if how in ('x', 'index') else {}))
    if name == 'refine_R':
        return op(name, x=1.0 if bad else pick((0.31, 0.07)), abeta=pick((7.0, 300.0)))
    if name == 'resample_sites':
        return op(name, src=st.cur if bad else pick(others), key=key, block=pick((1, 5, 64)))
    if name == 'plant_sites':
        w = st.w
        return op(name, src=pick(others), key=key, K=pick((0, 1, 3)), iA=w.nA if bad else w.nA - 1, ix=int(rng.integers(w.nx)),
                  ia=int(rng.integers(w.nab)))
    if name == 'locate_begin':
        return op(name, K=pick((1, 4)), step=pick((3, 10)), width=pick((1, 25)), R=0 if bad else pick((1, 2, 3)))
    if name == 'locate_accumulate':
        R = st.slot.lc['R'] if st.slot.lc else 1
        return op(name, r=R if bad else int(rng.integers(R)))
    if name == 'pack_records':
        return op(name, **({'short': True} if bad else {}))
    return op(name)


def walk(seed, length=WALK_LENGTH):
    """A seeded random walk over WALK_SLOTS, generated from the state model: four models, the ops drawn by _WEIGHTS with what the
    selected slot lacks (sites, test sites, a scan) preferred, refusals kept at about one op in eight."""
    rng = np.random.default_rng([20261023, seed])
    st = State(R_of=lambda m: None)
    table = _WEIGHTS if seed in OLD_WALK_SEEDS else _NEW_WEIGHTS if seed in NEW_WALK_SEEDS else _LIST_WEIGHTS
    names, weights = list(table), np.array(list(table.values()), dtype=np.float64)
    models = WALK_MODELS[seed] if seed in WALK_MODELS else LIST_WALK_MODELS[LIST_WALK_SEEDS.index(seed)]
    ops = []
    while len(ops) < length:
        due = models[min(len(ops) * len(models) // length, len(models) - 1)]
        if st.model != due:
            new = op('set_model', model=due)
        else:
            s = st.slot
            lack = 'set_sites' if s.sites is None else 'set_tests' if s.tests is None else 'scan' if s.scan is None else None
            if lack == 'set_sites' and rng.random() < 0.3:
                lack = 'resample_sites' if rng.random() < 0.5 else 'plant_sites'
            name = lack if lack and rng.random() < 0.75 else names[int(rng.choice(len(names), p=weights / weights.sum()))]
            if name in ('refine', 'support', 'boot') and st.model in SLOW_OFFGRID:
                continue
            # the newest walks go on to the baseline a scanned slot lacks and to its first locus, at a lower rate (the earlier
            # walks never come here: their random numbers are what they were)
            if table is _LIST_WEIGHTS and lack is None and (s.bl is None or not s.bl) and rng.random() < BASELINE_RATE:
                name = 'baseline_reset' if s.bl is None else 'baseline_add'
            new = _draw(rng, st, name)
        code = st.predict(new)
        if code and new[0] != 'set_model' and not (new[1].get('bad') or rng.random() < KEEP_REFUSED or _is_bad(new)):
            continue
        ops.append(new)
        st.step(new)
    return ops


def _is_bad(o):
    a = o[1]
    return (a.get('block') == 0 or a.get('R') == 0 or a.get('stride') == 0 or a.get('chrom') == 'bad' or a.get('slot') == MAX_SLOTS
            or a.get('which') == 8 or a.get('F') == 0 or a.get('frac') == 0.0 or a.get('drop') == 0.0 or a.get('short')
            or NAN in a.values() or a.get('hx') == 0.0 or a.get('test') == 'M' or a.get('lin') == 'top' or a.get('x') == 1.0)


def scripts():
    out = {'hand': hand_script()}
    for seed in WALK_SEEDS:
        out['walk%d' % seed] = walk(seed)
    return out


def replay(ops, R_of=None):
    """[(op, code, state after)] -- the state object is the one replayed: look at it inside the loop, or use trace()."""
    st = State(R_of=R_of)
    for o in ops:
        yield o, st.step(o), st


def trace(ops):
    """Per op: (op, code, selected slot, model, sites of the slot, test sites, scans of the slot, profiles, variant)."""
    out = []
    for o, code, st in replay(ops, R_of=lambda m: None):
        s = st.slot
        out.append({'op': o, 'compared': code == 0 and is_compared(o, st), 'name': o[0], 'code': code, 'slot': st.cur, 'model': st.model, 'N': 0 if s.sites is None else len(s.sites['gen']),
                    'M': s.M, 'seq': s.seq, 'profiles': st.profiles, 'variant': st.variant, 'perm': s.perm,
                    'with_sites': sorted(k for k, v in st.slots.items() if v.sites is not None), 'with_results': st.with_results(),
                    'tests': None if s.tests is None else (s.tests['stride'], s.tests['windows'], s.M)})
    return out
