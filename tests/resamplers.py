"""Seeded inputs that walk the kernels that make the replicates (bmxscan.hip: permute_rows_kernel; resample_count_kernel,
prefix_kernel and resample_expand_kernel; plant_range_kernel, plant_kernel and plant_hist_kernel; null_count_kernel and
null_max_kernel; locate_reduce_kernel) past their launch caps, across their table-size branches and onto their tie rules: the
input of tests/test_resamplers_cpu.py (which shows on the host that every case reaches the edge it is named for) and of
tests/test_gpu_resamplers.py (which compares the device with the package's exact host restatements).  numpy and the package's
pure-Python modules only; nothing is read from a file.

Tables (statistic B_2, min count 1, the complete spectrum of powercases.analytic_spectrum, a 2 x 2 pair grid):
    t46      sizes 20, 24                     the cheap table of every large-N case
    t3072    50, 60 .. 97                     the last table plant_kernel stages in LDS (16 B x 3 072 = PLANT_LDS_BYTES)
    t3073    51, 60 .. 97                     the first it reads through L2
    t8192    40, 90 .. 155                    the last table with an LDS histogram (RS_HIST_MAX)
    t8193    41, 90 .. 155                    the first that counts with global atomics
    t9796    300 .. 330                       2-byte rows, global-atomic histogram, L2 planting
    t90831   300 .. 520                       4-byte rows
    one24    24                               one sample size: n_sizes = 1 in plant_kernel's block search
"""
import functools

import numpy as np

import powercases as pc

from ballermixplus_amd import boot, locate, null, power

# the literals of ballermixplus_amd/csrc/bmxscan.hip these inputs are shaped around (test_resamplers_cpu.py matches them against
# the source)
RS_THREADS, RS_PER, RS_HIST_MAX, RS_BLOCKS_MAX = 256, 4, 8192, 2048
RS_TILE = RS_THREADS * RS_PER
NULL_THREADS, NULL_BLOCKS_MAX = 256, 1024
PLANT_THREADS, PLANT_LDS_BYTES, PLANT_HIST_BLOCKS_MAX, PLANT_Y_MAX = 256, 48 << 10, 1024, 4096
PERM_THREADS, PERM_BLOCKS_MAX = 256, 8192
MOM_SLOTS = 254
WAVE, LOCATE_THREADS = 64, 256

XS, ABETAS = [0.3, 0.5], [2.0, 20.0]
SIZES = {
    't46': (20, 24),
    't3072': (50,) + tuple(range(60, 98)),
    't3073': (51,) + tuple(range(60, 98)),
    't8192': (40,) + tuple(range(90, 156)),
    't8193': (41,) + tuple(range(90, 156)),
    't9796': tuple(range(300, 331)),
    't90831': tuple(range(300, 521)),
    'one24': (24,),
}
ROWS = {'t46': 46, 't3072': 3072, 't3073': 3073, 't8192': 8192, 't8193': 8193, 't9796': 9796, 't90831': 90831, 'one24': 25}


class Table:
    """One model: the ModelArrays, its admissible weights, and seeded site arrays of any length drawn from its own spectrum."""

    def __init__(self, name):
        from ballermixplus_amd import engine
        self.name, self.sizes = name, SIZES[name]
        self.spect, self.props = pc.analytic_spectrum('B2', self.sizes, 1)
        self.model = engine.ModelArrays('B2', 1, self.sizes, self.spect, self.props, XS, ABETAS)
        self.gw = power.allowed_rows('B2', 1, self.model.sizes, self.model.row_off, self.model.g)

    @functools.lru_cache(maxsize=4)
    def sites(self, N, seed=1, flat=True):
        """(genpos f64[N], rows i32[N]): gaps geometric(0.02) / 1e6, sample sizes uniform, every admissible count equally likely (flat)
        -- an excess of middle frequencies against the model's neutral spectrum, so that most test sites have a grid result with a
        CLR > 0 -- or, with flat=False, counts from the spectrum itself."""
        rng = np.random.default_rng([seed, N, ROWS[self.name], int(flat)])
        gen = np.cumsum(rng.geometric(0.02, N)) / 1e6
        nn = rng.choice(np.array(self.sizes), N)
        k = np.zeros(N, dtype=np.int64)
        for n in self.sizes:
            ks = sorted(a for (a, b) in self.spect if b == n)
            p = np.ones(len(ks)) if flat else np.array([self.spect[(a, n)] for a in ks]) / self.props[n]
            at = np.nonzero(nn == n)[0]
            k[at] = rng.choice(np.array(ks), len(at), p=p / p.sum())
        rows = self.model.rows_of(k, nn)
        gen.setflags(write=False)
        rows.setflags(write=False)
        return gen, rows


@functools.lru_cache(maxsize=None)
def table(name):
    return Table(name)


def strided_tests(gen, n=200):
    """About n test positions: every len(gen) // n-th site."""
    return gen[::max(1, len(gen) // n)]


# ------------------------------------------------------------------------------------------------ 1. permutation

N_KEYS = 40
PERM_LARGE_N = PERM_BLOCKS_MAX * PERM_THREADS + 3 * PERM_THREADS + 77          # the second stride pass, with a ragged end


def perm_keys(n=N_KEYS, seed=11):
    return [null.replicate_key(seed, r, 0) for r in range(n)]


def feistel_shape(N, B):
    """(nb, h, domain) of null.block_permutation's network; h = domain = 0 when nb < 2 (the identity: no launch)."""
    nb = N // B
    if nb < 2:
        return nb, 0, 0
    h = max(4, ((nb - 1).bit_length() + 1) // 2)
    return nb, h, 1 << (2 * h)


# name: (table, N, B, number of keys, (nb, h, domain) as the issue states them)
PERM_CASES = {
    'n1': ('t46', 1, 1, 3, (1, 0, 0)),
    'n2': ('t46', 2, 1, N_KEYS, (2, 4, 256)),                  # nb = 2 and 3 in a domain of 256: long cycle walks
    'n3': ('t46', 3, 1, N_KEYS, (3, 4, 256)),
    'n5b2': ('t46', 5, 2, N_KEYS, (2, 4, 256)),                # ... with a tail of one site that does not move
    'n16': ('t46', 16, 1, 3, (16, 4, 256)),
    'n17': ('t46', 17, 1, 3, (17, 4, 256)),
    'n255': ('t46', 255, 1, 3, (255, 4, 256)),
    'n256': ('t46', 256, 1, 3, (256, 4, 256)),                 # nb = the domain: no walk
    'n257': ('t46', 257, 1, 3, (257, 5, 1024)),                # h steps from 4 to 5
    'n512b2': ('t46', 512, 2, 3, (256, 4, 256)),
    'idN': ('t46', 300, 300, 2, (1, 0, 0)),                    # B = N, N - 1, N + 5: nb < 2, the identity
    'idN-1': ('t46', 300, 299, 2, (1, 0, 0)),
    'idN+5': ('t46', 300, 305, 2, (0, 0, 0)),
    'wide3000': ('t90831', 3000, 1, 3, (3000, 6, 4096)),       # 4-byte rows
    'wide257': ('t90831', 257 * 3 + 1, 3, 3, (257, 5, 1024)),
    'largeB1': ('t46', PERM_LARGE_N, 1, 2, (PERM_LARGE_N, 11, 1 << 22)),
    'largeB7': ('t46', PERM_LARGE_N, 7, 2, (PERM_LARGE_N // 7, 10, 1 << 20)),
}
PERM_SMALL = [n for n in PERM_CASES if not n.startswith('large')]
PERM_RESTORE = ('n3', 'n257', 'idN', 'wide257', 'largeB7')     # the sample that also checks restore_rows


# ------------------------------------------------------------------------------------------------ 2. resampling

RS_SMALL_N = (1, 3, 4, 5, 1023, 1024, 1025, 2049)
RS_1024_TILES = RS_TILE * 1024                                 # exactly 1 024 tile sums for prefix_kernel
RS_2051_TILES = RS_BLOCKS_MAX * RS_TILE + 2 * RS_TILE + 5     # a second tile for workgroups 0 .. 2, more than 1 024 tile sums
RS_LARGE_B = (1, 7, 1025)
RS_TABLE_N = 5000
RS_TABLES = ('t46', 't8192', 't8193', 't9796', 't90831')


def rs_small_blocks(N):
    return sorted({1, 2, 3, 4, 5, 7, 1024, 1025, 4099, N, N + 1})


def rs_key(r, seed=5):
    return locate.replicate_key(seed, r, 0)


@functools.lru_cache(maxsize=None)
def rs_edge_keys(N, B):
    """(a key whose weight vector is all 0, a key with a weight >= 3) of an N <= 5 chromosome, found on the host."""
    key0 = key3 = None
    for r in range(200000):
        k = rs_key(r, seed=6)
        w = boot.site_weights(k, N, B)
        if key0 is None and not w.any():
            key0 = k
        if key3 is None and w.max() >= 3:
            key3 = k
        if key0 is not None and key3 is not None:
            return key0, key3
    raise AssertionError((N, B))


def rs_small_keys(N, B):
    return (rs_key(0), rs_key(1)) + (rs_edge_keys(N, B) if N <= 5 else ())


# ------------------------------------------------------------------------------------------------ 3. planting

class Plant:
    """One planting case: table, As, sites, centres, planted grid point (iA, ix, ia), key."""

    def __init__(self, tab, N, As, iA, centres, key_r=0, seed=1, shift=None, edges=False):
        self.t = table(tab)
        self.model, self.gw, self.As = self.t.model, self.t.gw, list(As)
        self.gen, self.rows = self.t.sites(N, seed)
        if shift is not None:                                          # a gap: the sites from shift[0] on move up by shift[1]
            self.gen = self.gen.copy()
            self.gen[shift[0]:] += shift[1]
        if edges:       # the block search's ends, in reach of _three's first centre: the first row a site can hold (k = 1) and the
            off = self.model.row_off                       # last row (k = n) of the first and of the last size block
            self.rows = self.rows.copy()
            self.rows[EDGE_SITES[0]:EDGE_SITES[1]] = [off[0] + 1, off[1] - 1, off[-2] + 1, off[-1] - 1]
        self.planted = (iA, 1, 1)
        self.A = float(As[iA])
        self.centres = np.asarray(centres(self.gen, power.ALPHA_CUT / self.A), dtype=np.float64)
        self.key = power.replicate_key(7, key_r, 0)

    def host(self, R, rows=None):
        """power.planted_rows on the table R[nx][nab][rows] (the oracle's or the device's)."""
        return power.planted_rows(self.gen, self.rows if rows is None else rows, self.model.sizes, self.model.row_off,
                                  R[self.planted[1], self.planted[2]], self.gw, self.A, self.centres, self.key)

    def runs(self):
        fc = [power.reach(self.gen, c, self.A)[1:] for c in self.centres]
        return np.array([a for a, _ in fc], dtype=np.int32), np.array([b for _, b in fc], dtype=np.int32)


EDGE_SITES = (701, 705)


def _three(gen, reach):
    return [gen[700], gen[2500], gen[4400]]


ZERO_GAP = (4000, 0.05)                                       # the 'zero' case's sites from 4 000 on lie 0.05 further up


def _zero_runs(gen, reach):
    """An ordinary centre, and three centres whose run holds no site: before the first site, in the middle of the gap (wider than
    twice the reach) and after the last site."""
    return [gen[0] - 3.0 * reach, gen[1500], 0.5 * (gen[ZERO_GAP[0] - 1] + gen[ZERO_GAP[0]]), gen[-1] + 3.0 * reach]


PLANT_K = 4100
PLANT_HIST_N = PLANT_HIST_BLOCKS_MAX * RS_THREADS + 300

# name: (table, N, As, iA, centres(gen, reach), replicate of the key)
PLANT_CASES = {
    't3072': ('t3072', 6000, (500.0, 1000.0), 1, _three, 0),
    't3073': ('t3073', 6000, (500.0, 1000.0), 1, _three, 0),
    't9796': ('t9796', 6000, (500.0, 1000.0), 1, _three, 0),
    'one24': ('one24', 6000, (500.0, 1000.0), 1, _three, 0),
    # 4 100 centres 4.5e-4 apart at A = 1e5 (reach 1.84e-4: about four sites a side): grid.y strides, 17 workgroups of ranges
    'k4100': ('t46', 40000, (1000.0, 1e5), 1, lambda gen, reach: gen[0] + 4.5e-4 * np.arange(PLANT_K), 0),
    # A = 3 000 (reach 6.1e-3, about 120 sites a side): three of the four centres have a run of 0 sites
    'zero': ('t46', 6000, (3000.0, 1e5), 0, _zero_runs, 0),
    # the whole chromosome in reach of one centre: the run is clipped at both ends
    'whole': ('t46', 1500, (200.0, 1000.0), 0, lambda gen, reach: [gen[750]], 0),
    # N past plant_hist_kernel's first pass; the run straddles the pass's end and is clipped by the array's
    'hist': ('t46', PLANT_HIST_N, (500.0, 1000.0), 1, lambda gen, reach: [gen[PLANT_HIST_N - 150]], 0),
}


@functools.lru_cache(maxsize=None)
def plant(name):
    tab, N, As, iA, centres, r = PLANT_CASES[name]
    return Plant(tab, N, As, iA, centres, PLANT_KEY_R.get(name, r), shift=ZERO_GAP if name == 'zero' else None,
                 edges=name in ('t3072', 't3073', 't9796'))


# the replicate index of a case's key where replicate 0 left a redrawn site undecided on the oracle's table (none did)
PLANT_KEY_R = {}


# ------------------------------------------------------------------------------------------------ 4. null accumulation

NULL_CAP = NULL_THREADS * NULL_BLOCKS_MAX                      # test sites of null_count_kernel's first pass
NULL_LARGE_M = 2 * NULL_CAP + 300
NULL_M = (1, 255, 256, 257, NULL_LARGE_M)
NULL_AS = (500.0, 2000.0)
NULL_HALF = 150                                                # half width, in sites, of a window that is not empty
NULL_MAX_ROWS = (0, NULL_CAP - 1, NULL_CAP, NULL_LARGE_M - 1)  # where the only non-empty window sits, in turn


def null_sites(M):
    """The null cases' chromosome of M sites (every site a test site): flat counts, so the tracks are not 0."""
    return table('t46').sites(M, 1, True)


def null_blocks(M):
    """(B of the replicates; the last one is the identity: B > N / 2)."""
    return (1, 3, 7, M // 2 + 1)


def null_key(r):
    return null.replicate_key(13, r, 0)


def null_windows(M, keep):
    """(lo, hi) int64[M]: [i - NULL_HALF, i + NULL_HALF] clipped for the rows in `keep`, the empty window lo = 1 > hi = 0
    elsewhere (its CLR is exactly 0, without a grid result)."""
    lo, hi = np.ones(M, dtype=np.int64), np.zeros(M, dtype=np.int64)
    keep = np.asarray(keep, dtype=np.int64)
    lo[keep] = np.maximum(keep - NULL_HALF, 0)
    hi[keep] = np.minimum(keep + NULL_HALF, M - 1)
    return lo, hi


def null_large_keep():
    """The rows of the large M with a window: every 257th (both passes of the stride, every lane), and the four corner rows."""
    return np.unique(np.concatenate([np.arange(0, NULL_LARGE_M, 257), NULL_MAX_ROWS]))


# ------------------------------------------------------------------------------------------------ 5. per-range argmax

ARG_N, ARG_POOL, ARG_SEED = 3000, 1100, 17
ARG_TOP = 1648            # the site whose position is repeated: the oracle's largest CLR of the pool by a wide margin (CPU module)
ARG_AS = (500.0, 2000.0)
ARG_CLEAR = 50
ARG_PER_WG = LOCATE_THREADS // WAVE

# (name, length, offsets of the repeated position, offsets with a result: None = all)
ARG_RANGES = (
    ('len1', 1, (0,), None),
    ('len63', 63, (20,), None),
    ('len64', 64, (63,), None),
    ('len65', 65, (64,), None),
    ('len128', 128, (5, 100), None),                           # a tie in two lanes, the earlier row in the lower lane
    ('len129', 129, (128,), None),
    ('len1000', 1000, (37, 613, 614), None),
    ('same_lane', 200, (10, 74), None),                        # 64 rows apart: one lane meets both and keeps the first
    ('lane63_lane0', 130, (63, 64), None),                     # the earlier row in lane 63, the later in lane 0
    ('adjacent', 70, (0, 1), None),                            # lanes 0 and 1
    ('three_passes', 300, (200, 264, 137), None),              # 200 and 264 share lane 8; the earliest, 137, is lane 9's third row
    ('last_two', 90, (), (88, 89)),                            # only the last two rows have a result
    ('none', 77, (), ()),                                      # no row has a result
)
ARG_KS = (1, 3, 4, 5, 1001)


class ArgTrack:
    """Test positions (unsorted, the ranges laid end to end from a row that is no multiple of 64), windows, and the ranges."""

    def __init__(self):
        self.t = table('t46')
        self.gen, self.rows = self.t.sites(ARG_N, ARG_SEED, True)
        rng = np.random.default_rng(ARG_SEED)
        others = np.nonzero(np.abs(np.arange(ARG_N) - ARG_TOP) > ARG_CLEAR)[0]      # (a track is smooth: the top's neighbours stay out)
        self.pool = rng.choice(others, ARG_POOL, replace=False)          # site indices, in random order
        site, has, lo, hi, names = [], [], [], [], []
        at = 0

        def fill(n, top=(), res=None):
            s = rng.choice(self.pool, n)
            if top:
                s[list(top)] = ARG_TOP
            h = np.ones(n, dtype=bool) if res is None else np.isin(np.arange(n), res)
            site.append(s)
            has.append(h)

        fill(37)                                                       # the first range begins at row 37
        at = 37
        for name, n, top, res in ARG_RANGES:
            if at % WAVE == 0:
                fill(3)
                at += 3
            fill(n, top, res)
            names.append(name)
            lo.append(at)
            hi.append(at + n - 1)
            at += n
        fill(50)
        at += 50
        names.append('last_row')                                       # lo = hi = M - 1
        lo.append(at - 1)
        hi.append(at - 1)
        self.site = np.concatenate(site)
        self.has = np.concatenate(has)
        self.M = at
        assert len(self.site) == self.M
        self.names = names
        self.lo, self.hi = np.array(lo, dtype=np.int32), np.array(hi, dtype=np.int32)
        self.test_gen = self.gen[self.site]
        self.win_lo = np.where(self.has, 0, 1).astype(np.int64)
        self.win_hi = np.where(self.has, ARG_N - 1, 0).astype(np.int64)
        # ranges up to K = 1001: the designed ones first, then seeded ones anywhere
        a = rng.integers(0, self.M, 1001)
        b = np.minimum(a + rng.integers(0, 260, 1001), self.M - 1)
        k = len(lo)
        self.lo_all = np.concatenate([self.lo, a[k:].astype(np.int32)])
        self.hi_all = np.concatenate([self.hi, b[k:].astype(np.int32)])

    def ranges(self, K):
        return self.lo_all[:K], self.hi_all[:K]

    def want_first(self):
        """Per designed range: the row a first-row argmax returns by design (-1: none; None: not fixed by the design)."""
        out = []
        for (name, n, top, res), a in zip(ARG_RANGES, self.lo.tolist()):
            out.append(a + min(top) if top else (-1 if res == () else None))
        return out + [None]


@functools.lru_cache(maxsize=None)
def arg_track():
    return ArgTrack()


def wave_argmax(clr, has, a, b, tie_rule):
    """locate_reduce_kernel on the host, lane for lane: the lanes stride over [a, b] and keep their first best, then the xor
    butterfly.  tie_rule 'first' is the kernel's (ov == bv && ob < best); 'any' takes the partner's on every tie and 'never'
    keeps its own: the two readings of the butterfly without `ob < best`.  Returns lane 0's row."""
    best = np.full(WAVE, -1, dtype=np.int64)
    bv = np.zeros(WAVE)
    for lane in range(WAVE):
        for t in range(a + lane, b + 1, WAVE):
            if has[t] and (best[lane] < 0 or clr[t] > bv[lane]):
                best[lane], bv[lane] = t, clr[t]
    o = WAVE // 2
    while o:
        ob, ov = best[np.arange(WAVE) ^ o], bv[np.arange(WAVE) ^ o]
        tie = {'first': (ov == bv) & (ob < best), 'any': ov == bv, 'never': np.zeros(WAVE, dtype=bool)}[tie_rule]
        take = (ob >= 0) & ((best < 0) | (ov > bv) | tie)
        best, bv = np.where(take, ob, best), np.where(take, ov, bv)
        o >>= 1
    return int(best[0])
