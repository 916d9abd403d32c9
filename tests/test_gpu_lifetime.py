"""One long-lived context against fresh ones, across every call group (tests/lifetime.py holds the worlds, the state model and
the scripts; tests/test_lifetime_cpu.py shows on the host what the scripts reach).

Every test runs one script in ONE engine.Context that is closed only at the end.  Per op:
  * predicted to succeed: the op runs, everything it defines is fetched and compared AS BYTES (NaNs by bit pattern) with a clean
    room -- a context created for this one comparison, brought to the state by the shortest route (set_model, set_sites with the
    arrays the state model expects, permute_rows where the rows are permuted, set_tests, then only the calls the result depends on:
    scan, peaks, refine, the replicates of a null or locate run) and closed again.  No tolerance anywhere.  Clean rooms are never
    pooled or reused.  set_sites, permute_rows, restore_rows, resample_sites and plant_sites are also compared with the host
    restatements (null.block_permutation, locate.resampled, power.planted_rows on the device's own table).
  * predicted to be refused: BmxError with exactly the predicted code, and the slot's results fetched before and after are equal.
  * after every op one OTHER slot that holds results is fetched again and must be what it was when it was scanned.
  * at three checkpoints per script (one of them after the last set_model) the long-lived context's scan is compared with
    util.c_scan on the device's own table: integer fields exact outside the oracle's near-ties (gridshape.decide, at most 2 % of
    the windows), CLR within rtol 1e-9 / atol 1e-12 on every window -- so that the two contexts cannot be wrong together.  At the
    same checkpoints its fit and cond_surfaces of a 3-entry list are compared with fit.host_fit and
    conditional.host_cond_surface on the device's own table, at those features' tolerances (fitcases.TOL * max(1, n_d) per cell,
    condcases.REL_TOL of the conditional scale; integer fields exact), and its sandwich of a 3-entry list with
    sandwich.host_sandwich on the device's own five columns (Context.refine_R at sandwich.shifted_points; sandwichcases.TOL of |T|
    and of the sums of absolute terms, the counts exact).
  * the baseline calls (baseline_reset, _add, _fetch, base_surfaces): the clean room takes the model and the sites as given, resets
    and replays the loci the state model recorded, each under the permutation and on the single test site it was added with, then
    sets the permutation and the test sites of now and runs the op; d, cnt, baseline_add's three numbers and every array of
    base_surfaces are compared as bytes.  Every baseline_fetch is also compared with stepwise.host_baseline_add on the device's
    table (stepcases.D_TOL of each site's absolute increments, cnt exact).  At the three checkpoints of every script the
    long-lived context's base_surfaces of a 3-entry list after two adds is compared with stepwise.host_base_surface on the
    device's table (stepcases.REL_TOL of the scale; integer fields exact): a live baseline cannot be reset without changing its
    history, so this happens in lifetime.ANCHOR_SLOT, a slot of the same context that no script selects, on the checkpoint's
    sites and test sites.  Where a script itself calls base_surfaces with T on two loci or more (the hand-written one does, under
    every model; no walk does), the first two such calls under every model are compared in the same way, the list's first three
    entries, against the host's replay of the recorded history.
  * around every successful baseline or sandwich op the selected slot's scan results and, where the state model says they exist,
    fetch_refined, fetch_support and fetch_boot must be what they were; around a refused baseline op so must baseline_fetch; after
    every op one OTHER slot that holds a baseline has it fetched again.  The same sandwich call on permuted and on restored rows
    must differ.
"""
import collections
import time

import numpy as np
import pytest

import condcases as cc
import fitcases as fc
import gridshape as gs
import lifetime as lt
import sandwichcases as swc
import stepcases as stc
from util import c_oracle, c_scan

from ballermixplus_amd import conditional, fit, null, sandwich, stepwise

pytestmark = pytest.mark.gpu

ANCHOR_FIT = (7, 6)                  # (F, D) of the fit compared with host_fit at the checkpoints
ANCHOR_BLOCK = 7                     # block of the sandwich compared with host_sandwich there


def _zcut():
    from ballermixplus_amd import _lib
    return float(_lib.lib().bmx_alpha_cut())


def _fit_arrays(w, F, D):
    """(gw, cls, edges) of a fit call on a world's model (D = 1: no edge)."""
    m = w.model
    return w.fit_gw, fit.classes('B2', m.sizes, m.row_off, max(F, 1)), fit.default_edges(D, _zcut())


def _bytes(v):
    """Anything an op returns, as something == compares bit for bit."""
    if v is None or isinstance(v, (int, str, bytes)):
        return v
    if isinstance(v, float):
        return np.float64(v).tobytes()
    if isinstance(v, dict):
        return {k: _bytes(x) for k, x in sorted(v.items())}
    if isinstance(v, (tuple, list)):
        return tuple(_bytes(x) for x in v)
    a = np.ascontiguousarray(v)
    return (a.dtype.str, a.shape, a.tobytes())


def _differs(a, b, path=''):
    """Where two _bytes() values differ (for the assertion message)."""
    if type(a) is not type(b):
        return path + ': types'
    if isinstance(a, dict):
        return next((_differs(a[k], b[k], path + '.' + str(k)) for k in a if a[k] != b.get(k)), path + ': keys')
    if isinstance(a, tuple) and len(a) == 3 and isinstance(a[2], bytes):
        if a[:2] != b[:2]:
            return '%s: %r against %r' % (path, a[:2], b[:2])
        x, y = np.frombuffer(a[2], dtype=np.uint8), np.frombuffer(b[2], dtype=np.uint8)
        at = np.nonzero(x != y)[0]
        return '%s: %d of %d bytes differ, the first at element %d' % (path, len(at), len(x), at[0] // np.dtype(a[0]).itemsize)
    if isinstance(a, tuple):
        return next((_differs(p, q, '%s[%d]' % (path, i)) for i, (p, q) in enumerate(zip(a, b)) if p != q), path + ': length')
    return '%s: %r against %r' % (path, a, b)


_TABLES = {}


def device_table(name):
    """R[nx][nab][rows] of a model as a fresh context builds it."""
    if name not in _TABLES:
        from ballermixplus_amd import engine
        w = lt.world(name)
        ctx = engine.Context(0)
        try:
            ctx.set_model(w.model, w.As)
            R = ctx.fetch_lut()[1]
        finally:
            ctx.close()
        R.setflags(write=False)
        _TABLES[name] = R
    return _TABLES[name]


def _results(ctx, profiles):
    """Everything a scan defines: the five result arrays, the records, every profile that is on."""
    out = {'fetch': ctx.fetch(), 'records': ctx.fetch_records()}
    for bit in (1, 2, 4):
        if profiles & bit:
            out['profile%d' % bit] = ctx.fetch_profile(bit)
    return out


def _kept(snapshot, now):
    """A slot's results are what they were when it was scanned (set_profiles(0) may have released its profiles since)."""
    return {'fetch', 'records'} <= set(now) and all(now[k] == snapshot[k] for k in now)


class Runner:
    def __init__(self, tmp_path):
        from ballermixplus_amd import engine, _lib
        self.engine, self.BmxError = engine, _lib.BmxError
        self.ctx = engine.Context(0)
        self.st = lt.State(R_of=device_table)
        self.tmp, self.files = tmp_path, 0
        self.snap = {}                       # slot -> _bytes(_results) of its last scan
        self.rot = 0
        self.compared, self.refused, self.refetched = collections.Counter(), collections.Counter(), 0
        self.plans, self.kernels, self.wide_scans, self.anchors = set(), set(), 0, []
        self.rooms, self.t_rooms, self.t_anchors = 0, 0.0, 0.0
        self.slow = collections.Counter()    # (op, model) -> seconds, the op and its clean room together
        self.bl_snap, self.bl_rot, self.bl_refetched = {}, 0, 0        # slot -> _bytes of its baseline after its last baseline op
        self.bl_hosted, self.bl_most, self.bs_anchors, self.sw_anchors, self.base_anchors = 0, 0, [], [], []
        self.untouched, self.sw_seen, self.sw_last, self.sw_perm_pairs = 0, set(), {}, 0

    # ---- the arrays of an op, from its plain arguments and the state BEFORE it
    def args(self, o):
        name, a = o
        st, s = self.st, self.st.slot
        w = st.w if st.model else None
        if name == 'set_model':
            if a['model'] == 'bad':
                w0 = lt.world('g1')
                return {'model': w0.model, 'As': [5000.0, 0.0]}
            w1 = lt.world(a['model'])
            return {'model': w1.model, 'As': w1.As}
        if name == 'set_sites':
            gen, rows = (w or lt.world('g1')).chroms['S' if a['chrom'] == 'bad' else a['chrom']]
            return {'gen': gen[::-1] if a['chrom'] == 'bad' else gen, 'rows': rows}
        if name == 'set_tests':
            if a['stride'] == 0 or s.sites is None:
                return {'tg': np.zeros(0 if a['stride'] == 0 else 3), 'lo': None, 'hi': None}
            gen = s.sites['gen']
            idx = lt.test_index(len(gen), a['stride'])
            lo, hi = lt.windows_of(gen, idx, a['windows'])
            return {'tg': gen[idx], 'lo': lo, 'hi': hi}
        if name in ('surfaces', 'influence', 'fetch_at'):
            v = lt.index_list(a['kind'], s.M)
            if a.get('bad'):
                v[-1] = s.M
            return {'list': v}
        if name == 'fit':
            v = lt.index_list(a['kind'], s.M)
            points = w.nA * w.nx * w.nab
            lin = lt.fit_lins(a['kind'], points)
            gw, cls, edges = _fit_arrays(w, a['F'], a['D'])
            if a.get('bad') == 'lin':
                lin[-1] = points
            if a.get('bad') == 'gw':
                gw = gw.copy()
                gw[0] = 1.5
            return {'list': v, 'lin': lin, 'gw': gw, 'cls': cls, 'edges': edges}
        if name == 'cond_surfaces':
            v = lt.index_list(a['kind'], s.M)
            ct, cl = lt.cond_lists(v, s.M, w.nA * w.nx * w.nab)
            if a.get('bad'):
                ct[-1] = s.M
            return {'list': v, 'ct': ct, 'cl': cl}
        if name == 'baseline_add':
            test, lin = lt.baseline_locus(a, s.M, w.nA * w.nx * w.nab) if w else (0, 0)
            return {'test': test, 'lin': lin}
        if name == 'base_surfaces':
            v = lt.index_list(a['kind'], s.M)
            if a.get('bad'):
                v[-1] = s.M
            return {'list': v}
        if name == 'sandwich':
            v = lt.index_list(a['kind'], s.M)
            A, x, ab = lt.sandwich_points(w or lt.world('g1'), a['kind'])
            if a.get('bad') == 'x':
                x[-1] = sandwich.HX / 2
            if a.get('bad') == 'index':
                v[-1] = s.M
            return {'list': v, 'A': A, 'x': x, 'ab': ab}
        if name == 'plant_sites':
            src = st.slots.get(a['src'])
            have = src is not None and src.sites is not None and 0 <= a['iA'] < w.nA if w else False
            c = st.plant_args(a, src)[1] if have else np.arange(a['K'], dtype=np.float64)
            return {'centres': c, 'gw': w.gw if w else np.zeros(lt.world('g1').model.rows)}
        if name == 'peaks_track':
            return dict(zip(('gen', 'clr'), lt.track_of(a['n'], a['seed'])))
        if name in ('eval_points', 'eval_points_weighted'):
            return {'point': lt.eval_point(w) if w else (1.0, 0.3, 1.0)}
        if name == 'locate_begin':
            return dict(zip(('lo', 'hi'), lt.locate_ranges(a['K'], a['step'], a['width'])))
        if name == 'scan_write':
            self.files += 1
            return {'labels': (np.arange(s.M, dtype=np.int64) * 3 + 7, s.tests['tg'] if s.tests else np.zeros(0)),
                    'grids': ([repr(v) for v in w.xs], [repr(v) for v in w.abetas], [repr(v) for v in w.As]) if w else (['0.3'], ['1.0'], ['1.0'])}
        if name == 'pack_records':
            return {'total': sum(x.M for x in st.slots.values() if x.scan is not None)}
        return {}

    # ---- one op on one context (the long-lived one or a clean room); st: the state before the op
    def do(self, ctx, o, g, N=None, M=None, profiles=0, tag='live'):
        name, a = o
        f = lambda v: float(v)
        if name == 'set_model':
            ctx.set_model(g['model'], g['As'])
            return ctx.fetch_lut()[1]
        if name == 'set_sites':
            ctx.set_sites(g['gen'], g['rows'])
            return ctx.fetch_sites(len(g['gen']))
        if name == 'set_tests':
            ctx.set_tests(g['tg'], g['lo'], g['hi'])
            return ctx.plan(), ctx.launch_ranges()
        if name == 'select_slot':
            return ctx.select_slot(a['slot'])
        if name == 'set_variant':
            ctx.set_variant(a['variant'])
            return (ctx.plan(), ctx.launch_ranges()) if M else None
        if name == 'set_profiles':
            return ctx.set_profiles(a['which'])
        if name == 'fetch_profile':
            return ctx.fetch_profile(a['which'])
        if name == 'scan':
            ctx.scan()
            return _results(ctx, profiles)
        if name == 'scan_write':
            path = str(self.tmp / ('%s_%d.txt' % (tag, self.files)))
            ctx.scan_write(path, g['labels'][0], g['labels'][1], *g['grids'], chunk=a['chunk'])
            out = _results(ctx, profiles)
            with open(path, 'rb') as fh:
                out['file'] = fh.read()
            return out
        if name == 'permute_rows':
            ctx.permute_rows(a['key'], a['block'])
            return ctx.fetch_sites(N)
        if name == 'restore_rows':
            ctx.restore_rows()
            return ctx.fetch_sites(N)
        if name == 'null_begin':
            ctx.null_begin()
            return ctx.null_fetch()
        if name == 'null_accumulate':
            return ctx.null_accumulate(), ctx.null_fetch()
        if name == 'null_fetch':
            return ctx.null_fetch()
        if name == 'refine_at_peaks':
            return ctx.refine_at_peaks(a['on'])
        if name == 'refine':
            ctx.refine(f(a['min_clr']))
            return ctx.fetch_refined()
        if name == 'fetch_refined':
            return ctx.fetch_refined()
        if name == 'support':
            ctx.support(a['drop'], f(a['min_clr']))
            return ctx.fetch_support()
        if name == 'fetch_support':
            return ctx.fetch_support()
        if name == 'boot':
            ctx.boot(lt.boot_keys(a['key'], a['R']), a['block'], f(a['min_clr']))
            return ctx.fetch_boot()
        if name == 'fetch_boot':
            return ctx.fetch_boot()
        if name == 'eval_points':
            return ctx.eval_points(*g['point'])
        if name == 'eval_points_weighted':
            return ctx.eval_points_weighted(a['key'], a['block'], *g['point'])
        if name == 'peaks':
            return ctx.peaks(f(a['sep']), f(a['min_clr']), f(a['frac']))
        if name == 'peaks_track':
            return ctx.peaks_track(g['gen'], g['clr'], f(a['sep']), f(a['min_clr']), f(a['frac']))
        if name == 'fetch_peaks':
            return ctx.fetch_peaks()
        if name == 'surfaces':
            return ctx.surfaces(g['list'])
        if name == 'influence':
            return ctx.influence(g['list'], a['block'])
        if name == 'fit':
            return ctx.fit(g['list'], g['lin'], g['gw'], g['cls'], a['F'], g['edges'])
        if name == 'cond_surfaces':
            return ctx.cond_surfaces(g['list'], g['ct'], g['cl'], want_T=a['want_T'])
        if name == 'baseline_reset':
            ctx.baseline_reset()
            return ctx.baseline_fetch(N)
        if name == 'baseline_add':
            return ctx.baseline_add(g['test'], g['lin']), ctx.baseline_fetch(N)
        if name == 'baseline_fetch':
            return ctx.baseline_fetch(N or 0)
        if name == 'base_surfaces':
            return ctx.base_surfaces(g['list'], want_T=a['want_T'])
        if name == 'sandwich':
            return ctx.sandwich(g['list'], g['A'], g['x'], g['ab'], a['block'], hx=a.get('hx'))
        if name == 'refine_R':
            return ctx.refine_R(a['x'], a['abeta'])
        if name == 'resample_sites':
            n = ctx.resample_sites(a['src'], a['key'], a['block'])
            return n, (ctx.fetch_sites(n) if n else None)
        if name == 'plant_sites':
            out = ctx.plant_sites(a['src'], a['key'], g['centres'], a['iA'], a['ix'], a['ia'], g['gw'])
            return out, ctx.fetch_sites(N)
        if name == 'fetch_at':
            return ctx.fetch_at(g['list'])
        if name == 'locate_begin':
            ctx.locate_begin(g['lo'], g['hi'], a['R'])
            return ctx.fetch_locate()
        if name == 'locate_accumulate':
            ctx.locate_accumulate(a['r'])
            return ctx.fetch_locate()
        if name == 'fetch_locate':
            return ctx.fetch_locate()
        if name == 'pack_records':
            if a.get('short'):
                return ctx.pack_records(out=np.empty(max(g['total'] - 1, 0), dtype=self.engine._lib.RECORD_DTYPE))
            return ctx.pack_records()
        raise AssertionError(name)

    # ---- clean rooms
    def _setup(self, room, d, tests=True):
        """A fresh context up to a scan description's model, switches, sites, permutation and test sites."""
        w = lt.world(d['model'])
        room.set_model(w.model, w.As)
        room.set_variant(d['variant'])
        room.set_profiles(d['profiles'])
        room.set_sites(d['gen'], d['given'])
        if d['perm'] is not None:
            room.permute_rows(*d['perm'])
        if tests and d['tests'] is not None:
            room.set_tests(d['tests']['tg'], d['tests']['lo'], d['tests']['hi'])

    @staticmethod
    def _to_perm(room, have, want):
        if have != want:
            room.restore_rows() if want is None else room.permute_rows(*want)

    def _refined(self, room, rf):
        self._setup(room, rf['scan'])
        room.scan()
        if rf['peaks'] is not None:
            room.peaks(*rf['peaks'])
            room.refine_at_peaks(True)
        self._to_perm(room, rf['scan']['perm'], rf['perm'])
        room.refine(float(rf['min_clr']))

    def _based(self, room, o):
        """A fresh context up to the selected slot's baseline: the model, the sites as they were given, a reset, then every recorded
        locus under the permutation it was added under and on its single test site (the locus of a baseline_add op, the last, is
        left to the op itself); then the permutation and the test sites of now."""
        st, s = self.st, self.st.slot
        room.set_model(st.w.model, st.w.As)
        room.set_sites(s.sites['gen'], s.sites['given'])
        have = None
        if o[0] != 'baseline_reset':
            room.baseline_reset()
            for l in (s.bl[:-1] if o[0] == 'baseline_add' else s.bl):
                self._to_perm(room, have, l['perm'])
                have = l['perm']
                one = lambda v: None if v is None else np.array([v], dtype=np.int64)
                room.set_tests(np.array([l['tg']]), one(l['lo']), one(l['hi']))
                room.baseline_add(0, l['lin'])
        self._to_perm(room, have, s.perm)
        if s.tests is not None:
            room.set_tests(s.tests['tg'], s.tests['lo'], s.tests['hi'])

    def host_baseline(self):
        """(d, cnt, scale) of the selected slot's recorded baseline by stepwise.host_baseline_add on the device's own table; scale:
        each site's sum of absolute increments."""
        st, s = self.st, self.st.slot
        w, gen, given, R = st.w, s.sites['gen'], s.sites['given'], device_table(st.model)
        d, cnt, scale = np.zeros(len(gen)), np.zeros(len(gen), dtype=np.int32), np.zeros(len(gen))
        for l in s.bl:
            rows = given if l['perm'] is None else given[null.block_permutation(len(given), *l['perm'])]
            stepwise.host_baseline_add(d, cnt, gen, rows, R, l['tg'], 0 if l['lo'] is None else l['lo'], len(gen) - 1 if l['hi'] is None else l['hi'],
                                       w.As[l['lin'] // (w.nx * w.nab)], (l['lin'] // w.nab) % w.nx, l['lin'] % w.nab, _zcut(), scale=scale)
        return d, cnt, scale

    def anchor_baseline(self, i, o, got):
        """A baseline_fetch against the host's replay of the record (stepcases.D_TOL of each site's absolute increments, the counts
        exact); a 3-entry base_surfaces on two loci or more against stepwise.host_base_surface (stepcases.REL_TOL of the scale)."""
        st, s = self.st, self.st.slot
        if o[0] == 'baseline_fetch':
            dh, ch, scale = self.host_baseline()
            assert np.array_equal(got[1], ch), (i, o)
            err = np.abs(got[0] - dh)
            assert np.all(err <= stc.D_TOL * scale), (i, o, float(np.max(err[scale > 0] / scale[scale > 0])))
            self.bl_hosted += 1
            self.bl_most = max(self.bl_most, int(ch.max(initial=0)))
        elif o[1]['kind'] >= 3 and o[1]['want_T'] and len(s.bl) >= 2 and sum(m == st.model for _, m, _, _ in self.bs_anchors) < 2:
            dh, ch, _ = self.host_baseline()                # (the first two such calls under every model; the list's first three entries)
            w, gen, rows, t, R = st.w, s.sites['gen'], s.rows_now(), s.tests, device_table(st.model)
            worst = 0.0
            for q, j in enumerate(lt.index_list(o[1]['kind'], s.M)[:3].tolist()):
                lo, hi = (0, len(gen) - 1) if t['lo'] is None else (t['lo'][j], t['hi'][j])
                Th, nh, sh, S = stepwise.host_base_surface(gen, rows, R, w.As, t['tg'][j], lo, hi, dh, ch, _zcut(), scale=True)
                assert np.array_equal(got['nsites'][q], nh) and np.array_equal(got['nshared'][q], sh), (i, q)
                assert np.array_equal(np.isnan(got['T'][q]), np.isnan(Th)), (i, q)
                if (nh > 0).any():
                    worst = max(worst, float(np.nanmax(np.abs(got['T'][q] - Th))) / (stc.REL_TOL * float(S.max())))
            assert worst <= 1.0, (i, worst)
            self.bs_anchors.append((i, st.model, len(s.bl), worst))

    def held(self):
        """What a baseline or sandwich call must leave alone in the selected slot: its scan results and, where the state model
        says they exist, its refinement, support intervals and bootstrap."""
        st, s, out = self.st, self.st.slot, {'scan': self.fetch_now()}
        if s.rf is not None:
            out['refined'] = _bytes(self.ctx.fetch_refined())
        if st.predict(lt.op('fetch_support')) == 0:
            out['support'] = _bytes(self.ctx.fetch_support())
        if st.predict(lt.op('fetch_boot')) == 0:
            out['boot'] = _bytes(self.ctx.fetch_boot())
        return out

    def clean(self, o, g):
        """What a context created for this one comparison returns for op o (the state is the one AFTER the op)."""
        name, a = o
        st, s = self.st, self.st.slot
        room = self.engine.Context(0)
        self.rooms += 1
        N = None if s.sites is None else len(s.sites['gen'])
        kw = dict(N=N, M=s.M, profiles=st.profiles, tag='room')
        try:
            if name in ('set_model', 'peaks_track'):
                return self.do(room, o, g, **kw)
            if name in lt.GROUPS['baseline']:
                self._based(room, o)
                return self.do(room, o, g, **kw)
            if name == 'fetch_peaks' and s.pk['kind'] == 'track':
                t = lt.track_of(*s.pk['track'])
                room.peaks_track(t[0], t[1], *s.pk['args'])
                return room.fetch_peaks()
            if name in ('locate_begin', 'locate_accumulate', 'fetch_locate'):
                if st.model is not None:
                    room.set_model(st.w.model, st.w.As)
                lc = s.lc
                room.locate_begin(*lt.locate_ranges(lc['K'], lc['step'], lc['width']), lc['R'])
                for r, d in lc['acc']:
                    room.set_variant(d['variant'])
                    room.set_profiles(d['profiles'])
                    room.set_sites(d['gen'], d['given'])
                    if d['perm'] is not None:
                        room.permute_rows(*d['perm'])
                    room.set_tests(d['tests']['tg'], d['tests']['lo'], d['tests']['hi'])
                    room.scan()
                    room.locate_accumulate(r)
                return room.fetch_locate()
            if name in ('resample_sites', 'plant_sites'):
                src = st.slots[a['src']]
                room.set_model(st.w.model, st.w.As)
                room.set_sites(src.sites['gen'], src.sites['given'])
                if src.perm is not None:
                    room.permute_rows(*src.perm)
                room.select_slot(1)
                return self.do(room, (name, dict(a, src=0)), g, **kw)
            if name in ('null_begin', 'null_accumulate', 'null_fetch'):
                nl = s.null
                self._setup(room, nl['obs'])
                room.scan()
                room.null_begin()
                have, mx = nl['obs']['perm'], None
                for d in nl['reps']:
                    room.set_variant(d['variant'])
                    room.set_profiles(d['profiles'])
                    self._to_perm(room, have, d['perm'])
                    have = d['perm']
                    room.scan()
                    mx = room.null_accumulate()
                return (mx, room.null_fetch()) if name == 'null_accumulate' else room.null_fetch()
            if name in ('refine', 'fetch_refined'):
                self._refined(room, s.rf)
                return room.fetch_refined()
            if name in ('support', 'fetch_support'):
                self._refined(room, s.rf)
                self._to_perm(room, s.rf['perm'], s.sp['perm'])
                room.support(s.sp['drop'], float(s.sp['min_clr']))
                return room.fetch_support()
            if name in ('boot', 'fetch_boot'):
                self._refined(room, s.rf)
                self._to_perm(room, s.rf['perm'], s.bt['perm'])
                room.boot(lt.boot_keys(s.bt['key'], s.bt['R']), s.bt['block'], float(s.bt['min_clr']))
                return room.fetch_boot()
            if name in ('peaks', 'fetch_peaks'):
                self._setup(room, s.pk['scan'])
                room.scan()
                return room.peaks(*s.pk['args'])
            if name in ('fetch_profile', 'fetch_at'):
                self._setup(room, s.scan)
                room.scan()
                return self.do(room, o, g, **kw)
            # the ops that need the model, the slot's sites as they are now and (but for the first three) its test sites
            d = st.describe() if s.sites is not None else None
            if name == 'set_sites':
                room.set_model(st.w.model, st.w.As)
            elif name in ('permute_rows', 'restore_rows'):
                self._setup(room, dict(d, perm=self.perm_before if name == 'restore_rows' else None), tests=False)
            elif name == 'set_tests':
                self._setup(room, d, tests=False)
            elif name == 'set_variant':
                self._setup(room, dict(d, variant=0))
            else:
                assert name in ('scan', 'scan_write', 'surfaces', 'influence', 'fit', 'cond_surfaces', 'eval_points', 'eval_points_weighted',
                                'sandwich', 'refine_R'), name
                self._setup(room, d)
            return self.do(room, o, g, **kw)
        finally:
            room.close()

    # ---- the host restatements, where an op leaves site arrays
    def host_sites(self, o, got):
        s = self.st.slot
        name = o[0]
        if name in ('set_sites', 'permute_rows', 'restore_rows'):
            sites = got
        elif name == 'resample_sites':
            assert got[0] == (0 if s.sites is None else len(s.sites['gen'])), o
            sites = got[1]
        elif name == 'plant_sites':
            sites = got[1]
        else:
            return
        if sites is not None:
            assert np.array_equal(sites[0].view(np.uint64), s.sites['gen'].view(np.uint64)), o
            assert np.array_equal(sites[1], s.rows_now()), (o, int((sites[1] != s.rows_now()).sum()))

    def fetch_now(self):
        """The selected slot's last results, the profiles it computed included (None without results)."""
        s = self.st.slot
        return _bytes(_results(self.ctx, s.pl)) if s.scan is not None else None

    def anchor(self, i):
        """The long-lived context's scan against the C oracle on the device's own table."""
        st, s = self.st, self.st.slot
        w, gen, rows, t = st.w, s.sites['gen'], s.rows_now(), s.tests
        R = np.where(np.isfinite(device_table(st.model)), device_table(st.model), 0.0)
        M, N = s.M, len(gen)
        lo = np.zeros(M, np.int64) if t['lo'] is None else t['lo']
        hi = np.full(M, N - 1, np.int64) if t['hi'] is None else t['hi']
        got = self.ctx.fetch()
        ref = c_scan(c_oracle(), R, w.As, gen, rows, t['tg'], lo, hi)
        S, ns = gs.surface_sums(c_oracle(), R, w.As, gen, rows, t['tg'], lo, hi)
        tied = gs.decide(S, ns)[3]
        keep = ~tied
        worst = float(np.max(np.abs(got[0] - ref[0]) / np.maximum(np.abs(ref[0]), 1e-300)))
        print('  oracle anchor at op %d: model %s, %d sites, %d windows (%d near-ties left out of the exact comparison), variant %d, worst relative dCLR %.2e'
              % (i, st.model, N, M, int(tied.sum()), st.variant, worst))
        assert tied.sum() <= max(1, 0.02 * M)
        for q in (1, 2, 3, 4):
            assert np.array_equal(got[q][keep], ref[q][keep]), (i, q, np.nonzero(got[q] != ref[q])[0][:8])
        assert np.allclose(got[0], ref[0], rtol=1e-9, atol=1e-12), (i, worst)
        self.anchor_listed(i, w, gen, rows, t['tg'], lo, hi)
        self.anchor_base(i, w, gen, rows, t, lo, hi)
        self.anchors.append(i)

    def anchor_base(self, i, w, gen, rows, t, lo, hi):
        """base_surfaces of a 3-entry list after two adds against stepwise.host_base_surface on the device's table
        (stepcases.REL_TOL of the scale, integer fields exact; the adds' three numbers against stepwise.host_baseline_add).  A live
        baseline cannot be reset without changing its history, so the long-lived context does this in lt.ANCHOR_SLOT, which no
        script selects: the checkpoint's sites (the rows as they are now) and test sites are set there, and no recorded slot is
        touched."""
        st, ctx = self.st, self.ctx
        R, zcut, M, points, npairs = device_table(st.model), _zcut(), len(t['tg']), w.nA * w.nx * w.nab, w.nx * w.nab
        v = lt.index_list(3, M)
        dh, ch = np.zeros(len(gen)), np.zeros(len(gen), dtype=np.int32)
        ctx.select_slot(lt.ANCHOR_SLOT)
        try:
            ctx.set_sites(gen, rows)
            ctx.set_tests(t['tg'], t['lo'], t['hi'])
            ctx.baseline_reset()
            for k, j in enumerate(v[:2].tolist()):
                lin = lt.spread(k, points)
                got = ctx.baseline_add(j, lin)
                want = stepwise.host_baseline_add(dh, ch, gen, rows, R, t['tg'][j], lo[j], hi[j], w.As[lin // npairs], (lin // w.nab) % w.nx, lin % w.nab, zcut)
                assert got == want if want[2] else (got[0] > got[1] and got[2] == 0), (i, k, got, want)
            res = ctx.base_surfaces(v)
        finally:
            ctx.select_slot(st.cur)
        worst = 0.0
        for q, j in enumerate(v.tolist()):
            Th, nh, sh, S = stepwise.host_base_surface(gen, rows, R, w.As, t['tg'][j], lo[j], hi[j], dh, ch, zcut, scale=True)
            assert np.array_equal(res['nsites'][q], nh) and np.array_equal(res['nshared'][q], sh), (i, q)
            assert np.array_equal(np.isnan(res['T'][q]), np.isnan(Th)), (i, q)
            if (nh > 0).any():
                worst = max(worst, float(np.nanmax(np.abs(res['T'][q] - Th))) / (stc.REL_TOL * float(S.max())))
        assert worst <= 1.0, (i, worst)
        self.base_anchors.append((i, int(ch.sum()), int(res['nshared'].sum()), worst))
        print('  base_surfaces anchor at op %d: two loci on %d sites, %d shared sites in the three windows, worst %.2e of stepcases.REL_TOL x scale'
              % (i, int(ch.sum()), int(res['nshared'].sum()), worst))

    def anchor_listed(self, i, w, gen, rows, tg, lo, hi):
        """The long-lived context's fit and cond_surfaces of a 3-entry list against the host restatements on the device's table."""
        R, zcut, M = device_table(self.st.model), _zcut(), len(tg)
        v = lt.index_list(3, M)
        points, npairs = w.nA * w.nx * w.nab, w.nx * w.nab
        F, D = ANCHOR_FIT
        lin = lt.fit_lins(3, points)
        gw, cls, edges = _fit_arrays(w, F, D)
        O, Es, En, sk = self.ctx.fit(v, lin, gw, cls, F, edges)
        worst_fit = 0.0
        for q, (j, l) in enumerate(zip(v.tolist(), lin.tolist())):
            if l < 0:
                assert not O[q].any() and np.isnan(Es[q]).all() and np.isnan(En[q]).all() and sk[q] == 0
                continue
            hO, hEs, hEn, hsk = fit.host_fit(gen, rows, w.model.row_off, R, gw, cls, F, edges, w.As[l // npairs], (l // w.nab) % w.nx, l % w.nab,
                                             tg[j], lo[j], hi[j], zcut)
            assert np.array_equal(O[q], hO) and sk[q] == hsk, (i, q)
            bound = fc.TOL * np.maximum(1, hO.sum(axis=1))[:, None]
            worst_fit = max(worst_fit, float(np.max(np.abs(Es[q] - hEs) / bound)), float(np.max(np.abs(En[q] - hEn) / bound)))
        assert worst_fit <= 1.0, (i, worst_fit)
        ct, cl = lt.cond_lists(v, M, points)
        res = self.ctx.cond_surfaces(v, ct, cl, want_T=True)
        worst_cond = 0.0
        for q, (j, c, l) in enumerate(zip(v.tolist(), ct.tolist(), cl.tolist())):
            if c < 0 or l < 0:
                Th, nh, sh, S = conditional.host_cond_surface(gen, rows, R, w.As, tg[j], lo[j], hi[j], None, 0, -1, 0.0, 0, 0, zcut, scale=True)
            else:
                Th, nh, sh, S = conditional.host_cond_surface(gen, rows, R, w.As, tg[j], lo[j], hi[j], tg[c], lo[c], hi[c], w.As[l // npairs],
                                                              (l // w.nab) % w.nx, l % w.nab, zcut, scale=True)
            assert np.array_equal(res['nsites'][q], nh) and np.array_equal(res['nshared'][q], sh), (i, q)
            assert np.array_equal(np.isnan(res['T'][q]), np.isnan(Th)), (i, q)
            if (nh > 0).any():
                worst_cond = max(worst_cond, float(np.nanmax(np.abs(res['T'][q] - Th))) / (cc.REL_TOL * float(S.max())))
        assert worst_cond <= 1.0, (i, worst_cond)
        print('  listed anchor at op %d: fit (F %d, D %d) worst %.2e of its bound, cond_surfaces worst %.2e of its tolerance' % (i, F, D, worst_fit, worst_cond))
        # sandwich of a 3-entry list against host_sandwich on the device's own five columns: tests/test_gpu_sandwich.py's bar and scales
        pA, px, pab = lt.sandwich_points(w, 3)
        got = self.ctx.sandwich(v, pA, px, pab, ANCHOR_BLOCK)
        worst_sw = 0.0
        for q, j in enumerate(v.tolist()):
            tabs = np.array([self.ctx.refine_R(xx, aa) for xx, aa in sandwich.shifted_points(px[q], pab[q])])
            h = sandwich.host_sandwich(gen, rows, tabs, pA[q], tg[j], lo[j], hi[j], ANCHOR_BLOCK, zcut=zcut)
            assert (got['nsites'][q], got['nskipped'][q], got['nblocks'][q]) == (h['nsites'], h['nskipped'], h['nblocks']), (i, q)
            if h['nsites'] == h['nskipped']:
                assert got['T'][q] == -np.inf and not got['g'][q].any() and not got['H'][q].any() and not got['J'][q].any(), (i, q)
                continue
            for dev, ref, scale in [(got['T'][q], h['T'], abs(h['T']))] + [(got[k][q], h[k], h['abs' + k]) for k in ('g', 'H', 'J')]:
                worst_sw = max(worst_sw, float(np.max(np.abs(dev - ref) / (swc.TOL * np.asarray(scale) + 1e-300))))
        assert worst_sw <= 1.0, (i, worst_sw)
        self.sw_anchors.append((i, int(got['nsites'].sum()), worst_sw))
        print('  sandwich anchor at op %d: block %d, %d sites in the three windows, worst %.2e of sandwichcases.TOL x scale' % (i, ANCHOR_BLOCK, int(got['nsites'].sum()), worst_sw))

    def run(self, ops, anchors):
        st, ctx = self.st, self.ctx
        for i, o in enumerate(ops):
            name, a = o
            if i:
                self.slow[(ops[i - 1][0], st.model)] += time.perf_counter() - t_op
            t_op = time.perf_counter()
            want = st.predict(o)
            g = self.args(o)
            s = st.slot
            N = None if s.sites is None else len(s.sites['gen'])
            listed = lt.GROUP_OF[name] in ('baseline', 'sandwich')
            if want:
                before = self.fetch_now()
                based = name in lt.GROUPS['baseline'] and s.sites is not None and s.bl is not None
                bl_before = _bytes(ctx.baseline_fetch(N)) if based else None
                with pytest.raises(self.BmxError) as e:
                    self.do(ctx, o, g, N=N, M=s.M, profiles=st.profiles)
                assert e.value.code == want, (i, o, lt.CODE_NAMES[want], str(e.value))
                assert self.fetch_now() == before, (i, o, 'a refused call changed the results')
                assert not based or _bytes(ctx.baseline_fetch(N)) == bl_before, (i, o, 'a refused call changed the baseline')
                self.refused[want] += 1
            else:
                self.perm_before = s.perm
                after_profiles = st.profiles
                kept = self.held() if listed else None
                got = self.do(ctx, o, g, N=N if name != 'plant_sites' else len(st.slots[a['src']].sites['gen']), M=s.M, profiles=after_profiles)
                assert st.step(o) == 0
                s = st.slot
                self.host_sites(o, got)
                if listed:
                    assert self.held() == kept, (i, o, 'the call changed the results, the refinement, the support or the bootstrap')
                    self.untouched += 1
                if name in lt.GROUPS['baseline']:
                    self.bl_snap[st.cur] = _bytes(ctx.baseline_fetch(N))
                    if name in ('baseline_fetch', 'base_surfaces'):
                        self.anchor_baseline(i, o, got)
                if name == 'sandwich':
                    self.sw_seen.add(('LDS' if lt.ws_in_lds(st.w) else 'slab', 'wave' if a['block'] >= lt.SANDWICH_WAVE_BLOCK else 'thread'))
                    last = self.sw_last.get(st.cur)
                    if last is not None and last[0] == o and last[1] is s.tests and (last[2] is None) != (s.perm is None) and got['nsites'].any():
                        assert _bytes(got) != last[3], (i, o, 'the same answer on permuted and on restored rows')
                        self.sw_perm_pairs += 1
                    self.sw_last[st.cur] = (o, s.tests, s.perm, _bytes(got))
                if name == 'select_slot':
                    if s.scan is not None:
                        assert _kept(self.snap[st.cur], _bytes(_results(ctx, s.pl))), (i, o)
                elif name == 'pack_records':
                    want_rec = b''.join(self.snap[k]['records'][2] for k in st.with_results())
                    assert got.tobytes() == want_rec, (i, o)
                elif lt.is_compared(o, st):
                    t0 = time.perf_counter()
                    ref = self.clean(o, g)
                    self.t_rooms += time.perf_counter() - t0
                    assert _bytes(got) == _bytes(ref), (i, o, _differs(_bytes(got), _bytes(ref)))
                if lt.is_compared(o, st):
                    self.compared[lt.GROUP_OF[name]] += 1
                if name in ('scan', 'scan_write'):
                    pl = ctx.plan()
                    self.plans.add((pl['mode'], pl['J']))
                    self.kernels.add(pl['kernel'])
                    self.wide_scans += st.w.model.rows > 65535
                    self.snap[st.cur] = _bytes({k: v for k, v in got.items() if k != 'file'})
                    if i in anchors:
                        t0 = time.perf_counter()
                        self.anchor(i)
                        self.t_anchors += time.perf_counter() - t0
                for k in list(self.snap):
                    if st.slots[k].scan is None:
                        del self.snap[k]
            # one other slot that holds results must be what it was
            others = [k for k in st.with_results() if k != st.cur]
            if others:
                k = others[self.rot % len(others)]
                self.rot += 1
                ctx.select_slot(k)
                assert _kept(self.snap[k], _bytes(_results(ctx, st.slots[k].pl))), (i, o, 'slot %d changed' % k)
                ctx.select_slot(st.cur)
                self.refetched += 1
            # ... and one other slot that holds a baseline
            for k in list(self.bl_snap):
                if st.slots[k].bl is None:
                    del self.bl_snap[k]
            others = [k for k in sorted(self.bl_snap) if k != st.cur]
            if others:
                k = others[self.bl_rot % len(others)]
                self.bl_rot += 1
                ctx.select_slot(k)
                assert _bytes(ctx.baseline_fetch(len(st.slots[k].sites['gen']))) == self.bl_snap[k], (i, o, 'the baseline of slot %d changed' % k)
                ctx.select_slot(st.cur)
                self.bl_refetched += 1

    def close(self):
        self.ctx.close()


def _anchor_points(ops):
    """Three scans to compare with the oracle: the cheapest successful one of the first third, of the middle, and after the
    last set_model."""
    tr = lt.trace(ops)
    last_model = max(i for i, r in enumerate(tr) if r['name'] == 'set_model' and r['code'] == 0)
    scans = [(i, r) for i, r in enumerate(tr) if r['name'] == 'scan' and r['code'] == 0]
    cost = lambda r: lt.scan_cost(lt.world(r['model']), r['N'], r['tests'][0], r['tests'][1])
    third = len(ops) // 3
    parts = [[(i, r) for i, r in scans if i < third], [(i, r) for i, r in scans if third <= i < last_model],
             [(i, r) for i, r in scans if i > last_model]]
    assert all(parts), [len(p) for p in parts]
    return {min(p, key=lambda ir: cost(ir[1]))[0] for p in parts}


def _run_script(name, tmp_path):
    ops = lt.scripts()[name]
    anchors = _anchor_points(ops)
    from ballermixplus_amd import engine
    held = engine.live_bytes()
    run = Runner(tmp_path)
    t0 = time.perf_counter()
    try:
        run.run(ops, anchors)
    finally:
        run.close()
    assert engine.live_bytes() == held       # the closed context, and every clean room, gave back all it had allocated
    dt = time.perf_counter() - t0
    print('%s: %d ops in %.2f s (%.2f s in the clean rooms, %.2f s in the oracle); %d clean rooms; compared per group %s; refused %s; %d re-fetches of another slot; plans %s; 4-byte-row scans %d'
          % (name, len(ops), dt, run.t_rooms, run.t_anchors, run.rooms, dict(run.compared), {lt.CODE_NAMES[c]: n for c, n in run.refused.items()}, run.refetched,
             sorted(run.plans), run.wide_scans))
    print('  kernels: %s' % sorted(run.kernels))
    print('  baseline ops compared %d, sandwich ops compared %d; %d baseline fetches against the host (largest cnt %d), base_surfaces anchors (op, model, loci, share of the tolerance) %s; '
          'sandwich anchors (op, sites, share) %s; base_surfaces anchors at the checkpoints (op, sites written, shared sites, share) %s; %d ops left results, refinement, support and bootstrap as they were; %d re-fetches of another slot\'s baseline; '
          'sandwich workspaces and block paths %s; %d sandwich pairs on permuted and restored rows'
          % (run.compared['baseline'], run.compared['sandwich'], run.bl_hosted, run.bl_most, [(i, m, n, '%.1e' % x) for i, m, n, x in run.bs_anchors],
             [(i, n, '%.1e' % x) for i, n, x in run.sw_anchors], [(i, n, k, '%.1e' % x) for i, n, k, x in run.base_anchors], run.untouched, run.bl_refetched, sorted(run.sw_seen), run.sw_perm_pairs))
    print('  slowest (op, model): %s' % ', '.join('%s/%s %.2f s' % (k[0], k[1], v) for k, v in run.slow.most_common(8)))
    assert len(run.anchors) >= 3 and max(run.anchors) > max(i for i, o in enumerate(ops) if o[0] == 'set_model')
    # every script, the walks included: three sandwich and three base_surfaces anchors, one of either with sites to compare
    assert len(run.sw_anchors) >= 3 and any(n > 0 for _, n, _ in run.sw_anchors), run.sw_anchors
    assert len(run.base_anchors) >= 3 and any(n > 0 and shared > 0 for _, n, shared, _ in run.base_anchors), run.base_anchors
    return run


def test_hand_written_script(tmp_path):
    """The required transitions; it also meets the three default plans, a kernel that reads the table from L2 and a scan on
    4-byte row indices."""
    run = _run_script('hand', tmp_path)
    assert {(4, 16), (4, 8), (5, 1)} <= run.plans, run.plans
    assert any(k.endswith(',false>') or k.endswith('<false>') for k in run.kernels), run.kernels
    assert run.wide_scans >= 1
    # the baseline and sandwich groups: both homes of the workspace and both block paths, a count of 2 on some site, three host
    # anchors of either kind (one sandwich anchor with sites at least), the same call on permuted and restored rows
    assert run.sw_seen == {(h, p) for h in ('LDS', 'slab') for p in ('thread', 'wave')}, run.sw_seen
    assert run.bl_most >= 2 and run.bl_hosted >= 15 and run.bl_refetched >= 20
    assert len(run.bs_anchors) >= 3 and {'w4', lt.HAND_TAIL} <= {m for _, m, _, _ in run.bs_anchors}, run.bs_anchors
    assert run.sw_perm_pairs >= 2


@pytest.mark.parametrize('seed', lt.WALK_SEEDS)
def test_random_walk(seed, tmp_path):
    run = _run_script('walk%d' % seed, tmp_path)
    assert sum(run.refused.values()) >= lt.WALK_LENGTH // 16
