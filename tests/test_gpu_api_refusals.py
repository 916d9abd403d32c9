"""Every argument and state refusal of the library's resident-context entry points, pinned: the error code, the exact message,
which fault wins when a call has several, and that the refused call leaves the slot as it was (its sites, and the results of its
last scan, bit for bit).  One small context per state on the reference's first example (757 sites, every 25th a test site).
All of these return before any launch; none needs a launch to go wrong."""
import ctypes as C

import numpy as np
import pytest

import cases
from ballermixplus_amd import _lib, engine
from ballermixplus_amd._lib import BmxError

pytestmark = pytest.mark.gpu

INVALID, LIMIT, STATE = -1, -4, -5
NAN = float('nan')
SLOT_RANGE = 'slot index out of range (0..4095)'
NO_BOOT = 'no bootstrap of the slot\'s last scan: call bmx_ctx_boot after bmx_ctx_refine'
NO_PEAKS = 'no peak call on the slot: call bmx_ctx_peaks after a scan, or bmx_ctx_peaks_track'
NO_REFINEMENT = ' no refinement of the slot\'s last scan (call bmx_ctx_refine after the scan)'
POINTS = ' A > 0, 0 < x < 1 and alpha_beta > 0 (finite) at every point'
BEFORE_PLAN = 'model, sites and tests must be set before the plan exists'
AT_PEAKS = ('refine: restricted to the apexes (bmx_ctx_refine_at_peaks), but the slot has no peak call on its last scan: '
            'call bmx_ctx_peaks after the scan')


class World:
    """The example's host side, and one context per state: 'empty' (no model), 'model', 'sites', 'tests' (not scanned),
    'scanned', 'refined'.  get(): the shared context of a state (refusals leave it as it is); new(): one of the caller's own."""

    def __init__(self):
        argv, _ = cases.ALL_CASES['ex1_B2']
        opt, case, ts = cases.host_side(argv + ['-s', '25'])
        sel = engine.NormalizedBetaBinom(case.data, case.grid, opt.nofreq, opt.MAF, opt.nosub, device=0).prepare(case.neut)
        self.model, self.As, self.rows = sel.model, sel.grid_A, np.asarray(sel.rows, dtype=np.int32)
        self.gen = np.asarray(case.data.genPos, dtype=np.float64)
        self.tg, self.lo, self.hi = ts.test_gen, ts.lo, ts.hi
        self.M = len(ts.test_gen)
        self.ok = np.full(self.M, 0.5)
        self.bad = self.ok.copy()
        self.bad[3] = -1.0
        self.gw = np.ones(self.model.rows)
        self.shared = {}
        self.baseline = None

    def new(self, state):
        ctx = engine.Context(0)
        if state == 'empty':
            return ctx
        ctx.set_model(self.model, self.As)
        if state == 'model':
            return ctx
        ctx.set_sites(self.gen, self.rows)
        if state == 'sites':
            return ctx
        ctx.set_tests(self.tg, self.lo, self.hi)
        if state == 'tests':
            return ctx
        ctx.scan()
        if state == 'refined':
            ctx.refine()
        if self.baseline is None:
            self.baseline = ctx.fetch()
        return ctx

    def get(self, state):
        if state not in self.shared:
            self.shared[state] = self.new(state)
        return self.shared[state]

    def unchanged(self, ctx, state):
        """The slot answers as before the refused call."""
        if state in ('sites', 'tests', 'scanned', 'refined'):
            g, r = ctx.fetch_sites(len(self.gen))
            assert np.array_equal(g.view(np.uint64), self.gen.view(np.uint64)) and np.array_equal(r, self.rows)
        if state in ('scanned', 'refined'):
            assert ctx.M == self.M
            for a, b in zip(ctx.fetch(), self.baseline):
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope='module')
def world():
    w = World()
    yield w
    for ctx in w.shared.values():
        ctx.close()


def raw(ctx, name, *args):
    """The C entry point itself: arguments the wrapper would not pass on (NULL, a wrong size)."""
    _lib.check(getattr(ctx._L, name)(ctx._h, *args))


dp, ip, lp = _lib.as_dp, _lib.as_ip, _lib.as_lp
FAKE = C.c_void_p(256)          # a non-NULL address that a refused call never touches


def _plant(c, w, src, K=0, centre=None, grid=(0, 0, 0), gw=True):
    raw(c, 'bmx_ctx_plant_sites', src, 7, K, None if centre is None else dp(np.asarray(centre, dtype=np.float64)),
        grid[0], grid[1], grid[2], dp(w.gw) if gw else None, None, None, None)


def _i32(*v):
    return ip(np.array(v, dtype=np.int32))


def _f64(*v):
    return dp(np.array(v, dtype=np.float64))


def _key(v=1):
    return (C.c_uint64 * 1)(v)


# (id, state, call(ctx, world), code, message).  A state followed by '*' takes a context of the case's own: its calls before
# the refused one change the context (never the scan's results).
CASES = [
    # ---- scan, plan
    ('scan-empty', 'empty', lambda c, w: c.scan(), STATE, 'model, sites and tests must be set before scan'),
    ('scan-model', 'model', lambda c, w: c.scan(), STATE, 'model, sites and tests must be set before scan'),
    ('scan-sites', 'sites', lambda c, w: c.scan(), STATE, 'model, sites and tests must be set before scan'),
    ('plan-empty', 'empty', lambda c, w: c.plan(), STATE, BEFORE_PLAN),
    ('plan-sites', 'sites', lambda c, w: c.plan(), STATE, BEFORE_PLAN),
    ('launch_ranges-sites', 'sites', lambda c, w: c.launch_ranges(), STATE, BEFORE_PLAN),
    # ---- fetch*
    ('fetch-empty', 'empty', lambda c, w: c.fetch(), STATE, 'no scan results to fetch'),
    ('fetch-tests', 'tests', lambda c, w: c.fetch(), STATE, 'no scan results to fetch'),
    ('fetch_records-tests', 'tests', lambda c, w: c.fetch_records(), STATE, 'no scan results to fetch'),
    ('fetch_records-null-before-state', 'tests', lambda c, w: raw(c, 'bmx_ctx_fetch_records', None), INVALID, 'NULL argument'),
    ('fetch_records-null', 'scanned', lambda c, w: raw(c, 'bmx_ctx_fetch_records', None), INVALID, 'NULL argument'),
    ('result_ptrs-tests', 'tests', lambda c, w: c.result_ptrs(), STATE, 'no scan results: call bmx_ctx_scan after bmx_ctx_set_tests'),
    ('records-null-before-state', 'tests', lambda c, w: raw(c, 'bmx_ctx_records', None), INVALID, 'NULL argument'),
    ('records-tests', 'tests', lambda c, w: c.records(), STATE, 'no scan results: call bmx_ctx_scan after bmx_ctx_set_tests'),
    ('fetch_lut-empty', 'empty', lambda c, w: raw(c, 'bmx_ctx_fetch_lut', None, None), STATE, 'no model set'),
    ('fetch_profile-which-before-null-and-state', 'tests', lambda c, w: raw(c, 'bmx_ctx_fetch_profile', 3, None), INVALID,
     'fetch_profile: one of BMX_PL_A, BMX_PL_X, BMX_PL_ABETA'),
    ('fetch_profile-null-before-state', 'tests', lambda c, w: raw(c, 'bmx_ctx_fetch_profile', 2, None), INVALID, 'NULL argument'),
    ('fetch_profile-tests', 'tests', lambda c, w: c.fetch_profile('x'), STATE, 'the slot\'s last scan did not compute this profile'),
    ('fetch_profile-not-computed', 'scanned', lambda c, w: c.fetch_profile('A'), STATE, 'the slot\'s last scan did not compute this profile'),
    ('set_profiles-which', 'scanned', lambda c, w: c.set_profiles(8), INVALID, 'profiles: a set of BMX_PL_A, BMX_PL_X, BMX_PL_ABETA'),
    ('last_scan_ms-null', 'scanned', lambda c, w: raw(c, 'bmx_ctx_last_scan_ms', None), INVALID, 'NULL argument'),
    ('last_scan_ms-tests', 'tests', lambda c, w: c.last_scan_ms(), STATE, 'no scan has been launched'),
    # ---- copy_records, pack_records
    ('copy_records-null-before-state', 'tests', lambda c, w: raw(c, 'bmx_ctx_copy_records', None, 0), INVALID, 'NULL argument'),
    ('copy_records-state-before-size', 'tests', lambda c, w: raw(c, 'bmx_ctx_copy_records', FAKE, 0), STATE,
     'no scan results in the selected slot'),
    ('copy_records-small', 'scanned', lambda c, w: raw(c, 'bmx_ctx_copy_records', FAKE, w.M - 1), INVALID,
     'copy_records: destination too small'),
    ('pack_records-null', 'scanned', lambda c, w: raw(c, 'bmx_ctx_pack_records', None, 1, 0, None), INVALID, 'NULL argument'),
    ('pack_records-small', 'scanned', lambda c, w: raw(c, 'bmx_ctx_pack_records', FAKE, w.M - 1, 0, None), INVALID,
     'pack_records: destination too small'),
    ('pack_records-small-device', 'scanned', lambda c, w: raw(c, 'bmx_ctx_pack_records', FAKE, 0, 1, None), INVALID,
     'pack_records: destination too small'),
    # ---- permutation null
    ('permute_rows-state-before-block', 'model', lambda c, w: c.permute_rows(1, 0), STATE, 'set_sites must precede permute_rows'),
    ('permute_rows-block', 'scanned', lambda c, w: c.permute_rows(1, 0), INVALID, 'permutation block size must be >= 1'),
    ('restore_rows-model', 'model', lambda c, w: c.restore_rows(), STATE, 'set_sites must precede restore_rows'),
    ('null_begin-tests', 'tests', lambda c, w: c.null_begin(), STATE, 'null_begin needs the observed scan: call bmx_ctx_scan first'),
    ('null_accumulate-no-begin', 'scanned', lambda c, w: c.null_accumulate(), STATE, 'null_begin must precede null_accumulate'),
    ('null_accumulate-no-new-scan', 'scanned*', lambda c, w: (c.null_begin(), c.null_accumulate()), STATE,
     'null_accumulate needs a new scan (one per replicate)'),
    ('null_fetch-no-begin', 'scanned', lambda c, w: c.null_fetch(), STATE, 'null_begin must precede null_fetch'),
    # ---- surface(s)
    ('surface-null-before-state', 'empty', lambda c, w: raw(c, 'bmx_ctx_surface', 0.0, 0, 1, None, None), INVALID, 'NULL argument'),
    ('surface-model', 'model', lambda c, w: c.surface(0.0, 0, 1), STATE, 'model and sites must be set before surface'),
    ('surfaces-n-before-state', 'empty', lambda c, w: raw(c, 'bmx_ctx_surfaces', -1, None, None, None), INVALID, 'surfaces: n < 0'),
    ('surfaces-state-before-null', 'sites', lambda c, w: raw(c, 'bmx_ctx_surfaces', 2, None, None, None), STATE,
     'model, sites and tests must be set before surfaces'),
    ('surfaces-null', 'tests', lambda c, w: raw(c, 'bmx_ctx_surfaces', 2, None, None, None), INVALID, 'surfaces: NULL argument'),
    ('surfaces-null-T', 'scanned', lambda c, w: raw(c, 'bmx_ctx_surfaces', 2, _i32(0, 1), None, None), INVALID, 'surfaces: NULL argument'),
    ('surfaces-index', 'scanned', lambda c, w: c.surfaces([0, w.M, -1]), INVALID, 'surfaces: test site index out of range at entry 1'),
    ('surfaces-index-negative', 'tests', lambda c, w: c.surfaces([-1]), INVALID, 'surfaces: test site index out of range at entry 0'),
    ('surfaces_ms-null', 'scanned', lambda c, w: raw(c, 'bmx_ctx_surfaces_ms', None), INVALID, 'NULL argument'),
    ('surfaces_ms-none-yet', 'empty', lambda c, w: c.surfaces_ms(), STATE, 'no surfaces call yet'),
    # ---- eval_points(_weighted)
    ('eval_points-null-before-state', 'empty', lambda c, w: raw(c, 'bmx_ctx_eval_points', None, None, None, None, None), INVALID,
     'NULL argument'),
    ('eval_points-null-T', 'scanned', lambda c, w: raw(c, 'bmx_ctx_eval_points', dp(w.ok), dp(w.ok), dp(w.ok), None, None), INVALID,
     'NULL argument'),
    ('eval_points-sites', 'sites', lambda c, w: raw(c, 'bmx_ctx_eval_points', dp(w.bad), dp(w.ok), dp(w.ok), dp(w.ok), None), STATE,
     'model, sites and tests must be set before eval_points'),
    ('eval_points-A', 'scanned', lambda c, w: c.eval_points(w.bad, w.ok, w.ok), INVALID, 'eval_points:' + POINTS),
    ('eval_points-x', 'tests', lambda c, w: c.eval_points(w.ok, 1.0, w.ok), INVALID, 'eval_points:' + POINTS),
    ('eval_points-abeta-inf', 'scanned', lambda c, w: c.eval_points(w.ok, w.ok, float('inf')), INVALID, 'eval_points:' + POINTS),
    ('eval_points_weighted-null-before-state', 'empty',
     lambda c, w: raw(c, 'bmx_ctx_eval_points_weighted', 1, 0, None, None, None, None, None), INVALID, 'NULL argument'),
    ('eval_points_weighted-state-before-block', 'sites',
     lambda c, w: raw(c, 'bmx_ctx_eval_points_weighted', 1, 0, dp(w.ok), dp(w.ok), dp(w.ok), dp(w.ok), None), STATE,
     'model, sites and tests must be set before eval_points_weighted'),
    ('eval_points_weighted-block-before-points', 'scanned', lambda c, w: c.eval_points_weighted(1, 0, w.bad, w.ok, w.ok), INVALID,
     'eval_points_weighted: block must be >= 1'),
    ('eval_points_weighted-A', 'scanned', lambda c, w: c.eval_points_weighted(1, 1, NAN, w.ok, w.ok), INVALID,
     'eval_points_weighted:' + POINTS),
    ('eval_points_weighted-x', 'tests', lambda c, w: c.eval_points_weighted(1, 1, w.ok, w.bad, w.ok), INVALID,
     'eval_points_weighted:' + POINTS),
    # ---- refine, support, boot
    ('refine-state-before-nan', 'tests', lambda c, w: c.refine(NAN), STATE, 'refine: no scan results (scan the slot first)'),
    ('refine-empty', 'empty', lambda c, w: c.refine(), STATE, 'refine: no scan results (scan the slot first)'),
    ('refine-nan', 'scanned', lambda c, w: c.refine(NAN), INVALID, 'refine: min_clr is NaN'),
    ('refine-at-peaks-without-peaks', 'scanned*', lambda c, w: (c.refine_at_peaks(True), c.refine()), INVALID, AT_PEAKS),
    ('refine-nan-before-at-peaks', 'scanned*', lambda c, w: (c.refine_at_peaks(True), c.refine(NAN)), INVALID, 'refine: min_clr is NaN'),
    ('refine-at-peaks-of-an-older-scan', 'scanned*', lambda c, w: (c.peaks(0.0), c.scan(), c.refine_at_peaks(True), c.refine()),
     INVALID, AT_PEAKS),
    ('fetch_refined-scanned', 'scanned', lambda c, w: c.fetch_refined(), STATE,
     'no refinement of the slot\'s test sites: call bmx_ctx_refine after a scan'),
    ('support-state-before-drop', 'scanned', lambda c, w: c.support(-1.0, NAN), STATE, 'support:' + NO_REFINEMENT),
    ('support-tests', 'tests', lambda c, w: c.support(1.0), STATE, 'support:' + NO_REFINEMENT),
    ('support-refinement-of-an-older-scan', 'refined*', lambda c, w: (c.scan(), c.support(1.0)), STATE, 'support:' + NO_REFINEMENT),
    ('support-drop-before-nan', 'refined', lambda c, w: c.support(0.0, NAN), INVALID, 'support: drop must be finite and > 0'),
    ('support-drop-inf', 'refined', lambda c, w: c.support(float('inf')), INVALID, 'support: drop must be finite and > 0'),
    ('support-nan', 'refined', lambda c, w: c.support(1.0, NAN), INVALID, 'support: min_clr is NaN'),
    ('fetch_support-refined', 'refined', lambda c, w: c.fetch_support(), STATE,
     'no support intervals of the slot\'s test sites: call bmx_ctx_support after bmx_ctx_refine'),
    ('boot-state-before-keys', 'scanned', lambda c, w: raw(c, 'bmx_ctx_boot', None, 0, 0, NAN), STATE, 'boot:' + NO_REFINEMENT),
    ('boot-refinement-of-an-older-scan', 'refined*', lambda c, w: (c.scan(), c.boot([1])), STATE, 'boot:' + NO_REFINEMENT),
    ('boot-keys-before-block', 'refined', lambda c, w: raw(c, 'bmx_ctx_boot', None, 1, 0, NAN), INVALID,
     'boot: at least one replicate key is needed'),
    ('boot-R', 'refined', lambda c, w: raw(c, 'bmx_ctx_boot', _key(), 0, 1, 0.0), INVALID, 'boot: at least one replicate key is needed'),
    ('boot-block-before-nan', 'refined', lambda c, w: raw(c, 'bmx_ctx_boot', _key(), 1, 0, NAN), INVALID, 'boot: block must be >= 1'),
    ('boot-nan', 'refined', lambda c, w: c.boot([1], 1, NAN), INVALID, 'boot: min_clr is NaN'),
    ('boot_count-refined', 'refined', lambda c, w: raw(c, 'bmx_ctx_boot_count', None, None), STATE, NO_BOOT),
    ('fetch_boot-refined', 'refined', lambda c, w: c.fetch_boot(), STATE, NO_BOOT),
    ('fetch_boot-raw', 'scanned', lambda c, w: raw(c, 'bmx_ctx_fetch_boot', None, None, None, None, None, None, None), STATE, NO_BOOT),
    # ---- resample_sites, fetch_sites
    ('resample_sites-model-before-slot', 'empty', lambda c, w: raw(c, 'bmx_ctx_resample_sites', -1, 1, 0, None), STATE,
     'set_model must precede resample_sites'),
    ('resample_sites-slot-before-block', 'scanned', lambda c, w: raw(c, 'bmx_ctx_resample_sites', -1, 1, 0, None), INVALID, SLOT_RANGE),
    ('resample_sites-slot-4096', 'scanned', lambda c, w: raw(c, 'bmx_ctx_resample_sites', 4096, 1, 1, None), INVALID, SLOT_RANGE),
    ('resample_sites-same-before-block', 'scanned', lambda c, w: raw(c, 'bmx_ctx_resample_sites', 0, 1, 0, None), INVALID,
     'resample_sites: the source slot must not be the selected slot'),
    ('resample_sites-block-before-source', 'scanned', lambda c, w: raw(c, 'bmx_ctx_resample_sites', 5, 1, 0, None), INVALID,
     'resampling block size must be >= 1'),
    ('resample_sites-source-never-selected', 'scanned', lambda c, w: raw(c, 'bmx_ctx_resample_sites', 5, 1, 1, None), STATE,
     'resample_sites: the source slot has no sites'),
    ('resample_sites-source-without-sites', 'scanned*',
     lambda c, w: (c.select_slot(1), c.select_slot(0), raw(c, 'bmx_ctx_resample_sites', 1, 1, 1, None)), STATE,
     'resample_sites: the source slot has no sites'),
    ('fetch_sites-model', 'model', lambda c, w: c.fetch_sites(1), STATE, 'fetch_sites: the selected slot has no sites'),
    # ---- locate_*
    ('locate_begin-K', 'scanned', lambda c, w: raw(c, 'bmx_ctx_locate_begin', 0, _i32(0), _i32(0), 1), INVALID,
     'locate_begin: K >= 1 ranges and R >= 1 replicates are needed'),
    ('locate_begin-R-before-limit', 'scanned', lambda c, w: raw(c, 'bmx_ctx_locate_begin', 1, _i32(0), _i32(0), 0), INVALID,
     'locate_begin: K >= 1 ranges and R >= 1 replicates are needed'),
    ('locate_begin-null', 'scanned', lambda c, w: raw(c, 'bmx_ctx_locate_begin', 1, None, _i32(0), 1), INVALID,
     'locate_begin: K >= 1 ranges and R >= 1 replicates are needed'),
    ('locate_begin-limit-before-range', 'scanned', lambda c, w: raw(c, 'bmx_ctx_locate_begin', 2, _i32(0, 3), _i32(0, 2), 1 << 26), LIMIT,
     'locate_begin: more than 2^26 (peak, replicate) results'),
    ('locate_begin-range', 'scanned', lambda c, w: c.locate_begin([0, 3], [0, 2], 1), INVALID,
     'locate_begin: a range must have 0 <= lo <= hi'),
    ('locate_begin-range-negative', 'empty', lambda c, w: c.locate_begin([-1], [2], 1), INVALID,
     'locate_begin: a range must have 0 <= lo <= hi'),
    ('locate_accumulate-no-begin', 'scanned', lambda c, w: c.locate_accumulate(0), STATE, 'locate_begin must precede locate_accumulate'),
    ('locate_accumulate-index-before-state', 'scanned*', lambda c, w: (c.locate_begin([0], [0], 2), c.locate_accumulate(2)), INVALID,
     'locate_accumulate: replicate index outside [0, R)'),
    ('locate_accumulate-no-new-scan', 'scanned*', lambda c, w: (c.locate_begin([0], [w.M], 2), c.locate_accumulate(0)), STATE,
     'locate_accumulate needs a new scan (one per replicate)'),
    ('locate_accumulate-range-past-tests', 'scanned*', lambda c, w: (c.locate_begin([0], [w.M], 2), c.scan(), c.locate_accumulate(1)),
     INVALID, 'locate_accumulate: a range reaches past the slot\'s test sites'),
    ('fetch_locate-no-begin', 'scanned', lambda c, w: raw(c, 'bmx_ctx_fetch_locate', None, None), STATE,
     'locate_begin must precede fetch_locate'),
    # ---- plant_sites, fetch_at
    ('plant_sites-model-before-slot', 'empty', lambda c, w: raw(c, 'bmx_ctx_plant_sites', -1, 1, -1, None, 0, 0, 0, None, None, None, None),
     STATE, 'set_model must precede plant_sites'),
    ('plant_sites-slot-before-K', 'scanned', lambda c, w: _plant(c, w, -1, K=-1), INVALID, SLOT_RANGE),
    ('plant_sites-slot-4096', 'scanned', lambda c, w: _plant(c, w, 4096), INVALID, SLOT_RANGE),
    ('plant_sites-same-before-K', 'scanned', lambda c, w: _plant(c, w, 0, K=-1), INVALID,
     'plant_sites: the source slot must not be the selected slot'),
    ('plant_sites-K-before-grid', 'scanned', lambda c, w: _plant(c, w, 5, K=-1, grid=(-1, 0, 0)), INVALID, 'plant_sites: K must be >= 0'),
    ('plant_sites-grid-A', 'scanned', lambda c, w: _plant(c, w, 5, grid=(len(w.As), 0, 0)), INVALID,
     'plant_sites: the planted grid point lies outside the model\'s grids'),
    ('plant_sites-grid-x-before-null', 'scanned', lambda c, w: _plant(c, w, 5, K=1, grid=(0, -1, 0)), INVALID,
     'plant_sites: the planted grid point lies outside the model\'s grids'),
    ('plant_sites-grid-abeta', 'scanned', lambda c, w: _plant(c, w, 5, grid=(0, 0, len(w.model.abeta))), INVALID,
     'plant_sites: the planted grid point lies outside the model\'s grids'),
    ('plant_sites-null-centre', 'scanned', lambda c, w: _plant(c, w, 5, K=1), INVALID, 'plant_sites: centre and gw must be given'),
    ('plant_sites-null-gw', 'scanned', lambda c, w: _plant(c, w, 5, K=1, centre=[0.0], gw=False), INVALID,
     'plant_sites: centre and gw must be given'),
    ('plant_sites-centre-before-source', 'scanned', lambda c, w: _plant(c, w, 5, K=2, centre=[NAN, 1.0]), INVALID,
     'plant_sites: a centre is not finite'),
    ('plant_sites-centres-descend', 'scanned', lambda c, w: _plant(c, w, 5, K=2, centre=[1.0, 0.0]), INVALID,
     'plant_sites: the centres must ascend and lie more than twice the reach apart'),
    ('plant_sites-centres-close', 'scanned', lambda c, w: _plant(c, w, 5, K=2, centre=[0.0, 1e-300]), INVALID,
     'plant_sites: the centres must ascend and lie more than twice the reach apart'),
    ('plant_sites-source-never-selected', 'scanned', lambda c, w: _plant(c, w, 5, K=1, centre=[0.0]), STATE,
     'plant_sites: the source slot has no sites'),
    ('plant_sites-source-without-sites', 'scanned*', lambda c, w: (c.select_slot(1), c.select_slot(0), _plant(c, w, 1)), STATE,
     'plant_sites: the source slot has no sites'),
    ('plant_ms-null', 'scanned', lambda c, w: raw(c, 'bmx_ctx_plant_ms', None), INVALID, 'null argument'),
    ('plant_ms-none-yet', 'scanned', lambda c, w: c.plant_ms(), STATE, 'no plant_sites call yet'),
    ('fetch_at-state-before-list', 'tests', lambda c, w: raw(c, 'bmx_ctx_fetch_at', -1, None, None, None, None), STATE,
     'fetch_at needs a scan: call bmx_ctx_scan first'),
    ('fetch_at-n', 'scanned', lambda c, w: raw(c, 'bmx_ctx_fetch_at', -1, _i32(0), None, None, None), INVALID,
     'fetch_at: a list of test sites must be given'),
    ('fetch_at-null-before-limit', 'scanned', lambda c, w: raw(c, 'bmx_ctx_fetch_at', 0x7fffff01, None, None, None, None), INVALID,
     'fetch_at: a list of test sites must be given'),
    ('fetch_at-limit-before-index', 'scanned', lambda c, w: raw(c, 'bmx_ctx_fetch_at', 0x7fffff01, _i32(-2), None, None, None), LIMIT,
     'fetch_at: more than 2^31 indices'),
    ('fetch_at-index', 'scanned', lambda c, w: c.fetch_at([0, -1, w.M]), INVALID, 'fetch_at: a test site index outside [0, M) (or -1)'),
    ('fetch_at-index-negative', 'scanned', lambda c, w: c.fetch_at([-2]), INVALID, 'fetch_at: a test site index outside [0, M) (or -1)'),
    # ---- peaks*
    ('peaks-nan-before-state', 'empty', lambda c, w: c.peaks(NAN, 0.0, 2.0), INVALID, 'peaks: NaN argument'),
    ('peaks-nan-min_clr', 'scanned', lambda c, w: c.peaks(0.0, NAN), INVALID, 'peaks: NaN argument'),
    ('peaks-sep-before-frac', 'scanned', lambda c, w: c.peaks(-1.0, 0.0, 0.0), INVALID, 'peaks: the separation must be >= 0'),
    ('peaks-frac-before-state', 'tests', lambda c, w: c.peaks(0.0, 0.0, 1.5), INVALID, 'peaks: the extent fraction must lie in (0, 1]'),
    ('peaks-frac-zero', 'scanned', lambda c, w: c.peaks(0.0, 0.0, 0.0), INVALID, 'peaks: the extent fraction must lie in (0, 1]'),
    ('peaks-tests', 'tests', lambda c, w: c.peaks(0.0), INVALID, 'peaks: no scan results (scan the slot first)'),
    ('peaks-empty', 'empty', lambda c, w: c.peaks(0.0), INVALID, 'peaks: no scan results (scan the slot first)'),
    ('peaks_track-nan-before-M', 'scanned', lambda c, w: raw(c, 'bmx_ctx_peaks_track', -1, None, None, 0.0, 0.0, NAN), INVALID,
     'peaks_track: NaN argument'),
    ('peaks_track-sep', 'scanned', lambda c, w: c.peaks_track([0.0], [1.0], -0.5), INVALID, 'peaks_track: the separation must be >= 0'),
    ('peaks_track-frac', 'scanned', lambda c, w: c.peaks_track([0.0], [1.0], 0.0, 0.0, -1.0), INVALID,
     'peaks_track: the extent fraction must lie in (0, 1]'),
    ('peaks_track-M', 'scanned', lambda c, w: raw(c, 'bmx_ctx_peaks_track', -1, _f64(0.0), _f64(0.0), 0.0, 0.0, 0.5), INVALID,
     'peaks_track: M >= 0 rows of positions and values are needed'),
    ('peaks_track-null', 'scanned', lambda c, w: raw(c, 'bmx_ctx_peaks_track', 1, _f64(0.0), None, 0.0, 0.0, 0.5), INVALID,
     'peaks_track: M >= 0 rows of positions and values are needed'),
    ('peaks_track-nan-value', 'scanned', lambda c, w: c.peaks_track([0.0, 1.0, 0.5], [1.0, NAN, 1.0], 0.0), INVALID,
     'peaks_track: NaN value or non-finite position at row 1'),
    ('peaks_track-inf-position', 'scanned', lambda c, w: c.peaks_track([0.0, float('inf')], [1.0, 1.0], 0.0), INVALID,
     'peaks_track: NaN value or non-finite position at row 1'),
    ('peaks_track-descending', 'scanned', lambda c, w: c.peaks_track([0.0, 1.0, 0.5], [1.0, 1.0, 1.0], 0.0), INVALID,
     'peaks_track: positions are not non-decreasing at row 2'),
    ('peak_count-none', 'scanned', lambda c, w: raw(c, 'bmx_ctx_peak_count', None, None), STATE, NO_PEAKS),
    ('fetch_peaks-none', 'scanned', lambda c, w: c.fetch_peaks(), STATE, NO_PEAKS),
    ('fetch_peaks-raw', 'tests', lambda c, w: raw(c, 'bmx_ctx_fetch_peaks', None, None, None, None, None), STATE, NO_PEAKS),
    ('peaks_ms-null', 'scanned', lambda c, w: raw(c, 'bmx_ctx_peaks_ms', None), INVALID, 'NULL argument'),
    ('peaks_ms-none-yet', 'scanned', lambda c, w: c.peaks_ms(), STATE, 'no peak call yet'),
]


@pytest.mark.parametrize('state,call,code,msg', [pytest.param(*c[1:], id=c[0]) for c in CASES])
def test_refusal(world, state, call, code, msg):
    own = state.endswith('*')
    state = state.rstrip('*')
    ctx = world.new(state) if own else world.get(state)
    try:
        with pytest.raises(BmxError) as e:
            call(ctx, world)
        assert e.value.code == code
        assert str(e.value) == 'libbmxscan error %d: %s' % (code, msg)
        world.unchanged(ctx, state)
    finally:
        if own:
            ctx.close()


def test_peaks_refuses_unsorted_test_positions(world):
    """The one refusal that needs test sites of its own: the scan of unsorted test positions is sound, a peak call on it is not."""
    ctx = world.new('sites')
    order = np.arange(world.M)[::-1]
    ctx.set_tests(np.asarray(world.tg)[order], np.asarray(world.lo)[order], np.asarray(world.hi)[order])
    ctx.scan()
    before = ctx.fetch()
    with pytest.raises(BmxError) as e:
        ctx.peaks(0.0)
    assert e.value.code == INVALID and str(e.value) == 'libbmxscan error -1: peaks: the slot\'s test positions are not non-decreasing'
    for a, b in zip(ctx.fetch(), before):
        assert a.tobytes() == b.tobytes()
    ctx.close()
