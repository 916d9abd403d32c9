"""Python face of the MI355X scan: the two seams of the reference's hot path.

    NormalizedBetaBinom(InputData, Grids, nofreq, MAF, nosub)       reference BalLeRMix+_v1.py:310-433, called at :793
    calcBaller(window_indice, testSite, InputData, NeutralSFS,
               NormalizedBetaBinom, Grids)                          reference BalLeRMix+_v1.py:436-507

keep their names, argument meaning and return values, but run on the GPU through
libbmxscan.so (include/bmxscan.h).  `scan_batch` is the call the CLI uses: all test
sites of a chromosome in one launch.  Nothing here computes likelihoods on the CPU.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import BmxModel

STAT_IDS = {'B2': 0, 'B2maf': 1, 'B0': 2, 'B0maf': 3, 'B1': 4}


def stat_name(nofreq, MAF, nosub):
    """The dispatch of v1:336-352."""
    if nofreq:
        return 'B1'
    if MAF:
        return 'B0maf' if nosub else 'B2maf'
    return 'B0' if nosub else 'B2'


def live_bytes():
    """(device, pinned): the bytes of device and of pinned host memory that the library's contexts of this process hold now
    (bmx_live_bytes)."""
    dev, pin = C.c_int64(), C.c_int64()
    _lib.lib().bmx_live_bytes(C.byref(dev), C.byref(pin))
    return dev.value, pin.value


class ModelArrays:
    """The bmx_model struct plus the numpy arrays that back its pointers."""

    def __init__(self, stat, min_count, sizes, spect, samp_props, xs, abetas):
        self.stat = stat
        self.sizes = _lib.i32(sorted(int(n) for n in sizes))
        per = [2 if stat == 'B1' else int(n) + 1 for n in self.sizes]
        self.row_off = _lib.i32(np.concatenate(([0], np.cumsum(per))))
        self.rows = int(self.row_off[-1])
        g = np.full(self.rows, np.nan)
        for j, n in enumerate(self.sizes.tolist()):
            for k in range(per[j]):
                v = spect.get((k, n))
                if v is not None:
                    g[self.row_off[j] + k] = v
        self.g = _lib.f64(g)
        self.prop = _lib.f64([samp_props[int(n)] for n in self.sizes])
        self.x = _lib.f64(xs)
        self.abeta = _lib.f64(abetas)
        self.min_count = int(min_count)
        self._off_of = {int(n): int(o) for n, o in zip(self.sizes, self.row_off[:-1])}
        # two models with equal keys build bit-identical device tables
        self.key = (stat, self.min_count, self.sizes.tobytes(), self.g.tobytes(), self.prop.tobytes(), self.x.tobytes(),
                    self.abeta.tobytes())
        self.c = BmxModel(STAT_IDS[stat], self.min_count, len(self.sizes), _lib.as_ip(self.sizes),
                          _lib.as_ip(self.row_off), _lib.as_dp(self.g), _lib.as_dp(self.prop),
                          len(self.x), _lib.as_dp(self.x), len(self.abeta), _lib.as_dp(self.abeta))

    def rows_of(self, count, total):
        """LUT row of every site: row_off[n] + k."""
        total = np.asarray(total)
        count = np.asarray(count)
        if total.size == 0:
            return _lib.i32(np.zeros(0, dtype=np.int64))
        lo, hi = int(total.min()), int(total.max())
        if lo < 0:
            raise KeyError(lo)
        tab = np.full(hi + 1, -1, dtype=np.int32)         # sample size -> first row; one gather instead of a sort of all sites
        for n, off in self._off_of.items():
            if 0 <= n <= hi:
                tab[n] = off
        rows = tab[total]
        if rows.min() < 0:
            raise KeyError(int(total[int(np.argmin(rows))]))
        rows += count.astype(np.int32, copy=False)
        return _lib.i32(rows)


class Context:
    """One resident scan context (one GPU).  Thin wrapper over the bmx_ctx_* calls."""

    def __init__(self, device=0):
        self._L = _lib.lib()
        self._h = C.c_void_p()
        _lib.check(self._L.bmx_ctx_create(C.byref(self._h), int(device)))
        self.device = int(device)
        self.M = 0
        self.N = 0                   # (before set_sites / set_model the library refuses with BMX_E_STATE: the wrapper must get that far)
        self.model, self.nA = None, 0
        self.slot = 0
        self._slot_M = {}
        self._locate_shape = {}      # slot -> (R, K) of its locate_begin
        self._keep = []

    def close(self):
        if self._h:
            self._L.bmx_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _key64(key):
        return C.c_uint64(int(key) & ((1 << 64) - 1))

    def _ms(self, fn):
        """A call whose one output is a double: the *_ms getters, a replicate's maximum."""
        ms = C.c_double()
        _lib.check(fn(self._h, C.byref(ms)))
        return ms.value

    def _points(self, A, x, abeta):
        """One (A, x, abeta) per test site of the selected slot: f64[M] each, scalars broadcast."""
        return tuple(_lib.f64(np.broadcast_to(np.asarray(v, dtype=np.float64), (self.M,))) for v in (A, x, abeta))

    def _sites_replaced(self):       # the library drops the slot's test sites with its sites (they were located in the old array)
        self.M = 0
        self._slot_M.pop(self.slot, None)

    def set_model(self, model, As):
        A = _lib.f64(As)
        _lib.check(self._L.bmx_ctx_set_model(self._h, C.byref(model.c), _lib.as_dp(A), len(A)))
        self.model, self.nA = model, len(A)        # (after the call: a refused one leaves the library, and so this object, as it was)
        self.As = A.copy()
        self._slot_M = {}
        self._locate_shape = {}      # a new model ends every slot's position bootstrap
        self.M = 0

    def set_sites(self, genpos, rows):
        g, r = _lib.f64(genpos), _lib.i32(rows)
        _lib.check(self._L.bmx_ctx_set_sites(self._h, len(g), _lib.as_dp(g), _lib.as_ip(r)))
        self.N = len(g)
        self._sites_replaced()

    def set_tests(self, test_gen, win_lo=None, win_hi=None):
        """Test positions and their inclusive index windows; no windows = all sites of the chromosome (the reference's default mode)."""
        t = _lib.f64(test_gen)
        if win_lo is None and win_hi is None:
            _lib.check(self._L.bmx_ctx_set_tests(self._h, len(t), _lib.as_dp(t), None, None))
        else:
            lo, hi = _lib.i64(win_lo), _lib.i64(win_hi)
            _lib.check(self._L.bmx_ctx_set_tests(self._h, len(t), _lib.as_dp(t), _lib.as_lp(lo), _lib.as_lp(hi)))
        self.M = len(t)
        self._slot_M[self.slot] = self.M

    def set_variant(self, v):
        _lib.check(self._L.bmx_ctx_set_variant(self._h, int(v)))

    def select_slot(self, k):
        """Chromosome slot k of this context (created on first use): its own site arrays, test sites and results,
        the context's one model.  set_sites / set_tests / scan / fetch* act on the selected slot."""
        _lib.check(self._L.bmx_ctx_select_slot(self._h, int(k)))
        self.slot = int(k)
        self.M = self._slot_M.get(self.slot, 0)

    def plan(self):
        """{'J', 'use_lds', 'mode', 'stream_bytes', 'kernel'} of the selected slot's scan (bmx_ctx_plan)."""
        J, ul, mode = C.c_int32(), C.c_int32(), C.c_int32()
        sb = C.c_int64()
        _lib.check(self._L.bmx_ctx_plan(self._h, C.byref(J), C.byref(ul), C.byref(mode), C.byref(sb)))
        lds = 'true' if ul.value else 'false'
        if mode.value == 5:
            name = 'clr_scan_solo_kernel<%s>' % lds
        elif mode.value == 4:
            name = 'clr_scan_prepared_kernel<%d,%s>' % (J.value, lds)
        elif mode.value >= 0:
            name = 'clr_scan_grouped_kernel<%d,%s,%d>' % (J.value, lds, mode.value)
        else:
            name = 'clr_scan_kernel<%s>' % lds
        return {'J': J.value, 'use_lds': bool(ul.value), 'mode': mode.value, 'stream_bytes': sb.value, 'kernel': name}

    def launch_ranges(self):
        """First test-site index of every launch range of the selected slot's scan (bmx_ctx_launch_ranges)."""
        n = C.c_int32()
        _lib.check(self._L.bmx_ctx_launch_ranges(self._h, None, 0, C.byref(n)))
        offs = np.zeros(max(n.value, 1), dtype=np.int64)
        _lib.check(self._L.bmx_ctx_launch_ranges(self._h, _lib.as_lp(offs), len(offs), C.byref(n)))
        return offs[:n.value]

    def pack_records(self, out=None, device_ptr=None, cap=None):
        """Records of every slot with results, slot order.  Host: returns a RECORD array.  device_ptr/cap: packs into
        that device buffer (room for cap records) and returns the count."""
        n = C.c_int64()
        if device_ptr is not None:
            _lib.check(self._L.bmx_ctx_pack_records(self._h, C.c_void_p(int(device_ptr)), int(cap), 1, C.byref(n)))
            return n.value
        total = sum(self._slot_M.values())
        rec = out if out is not None else np.empty(total, dtype=_lib.RECORD_DTYPE)
        _lib.check(self._L.bmx_ctx_pack_records(self._h, rec.ctypes.data_as(C.c_void_p), len(rec), 0, C.byref(n)))
        return rec[:n.value]

    def copy_records(self, device_ptr, cap):
        """The SELECTED slot's records into a device buffer of this GPU (room for cap records); waits for the scan."""
        if cap < self.M:
            raise ValueError('destination holds %d records, the slot has %d' % (cap, self.M))
        _lib.check(self._L.bmx_ctx_copy_records(self._h, C.c_void_p(int(device_ptr)), int(cap)))
        return self.M

    def scan(self):
        _lib.check(self._L.bmx_ctx_scan(self._h))

    def sync(self):
        _lib.check(self._L.bmx_ctx_sync(self._h))

    def last_scan_ms(self):
        return self._ms(self._L.bmx_ctx_last_scan_ms)

    def fetch(self):
        M = self.M
        clr = np.empty(M, dtype=np.float64)
        ix, ia, iA, ns = (np.empty(M, dtype=np.int32) for _ in range(4))
        _lib.check(self._L.bmx_ctx_fetch(self._h, _lib.as_dp(clr), _lib.as_ip(ix), _lib.as_ip(ia),
                                         _lib.as_ip(iA), _lib.as_ip(ns)))
        return clr, ix, ia, iA, ns

    def result_ptrs(self):
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _lib.check(self._L.bmx_ctx_result_ptrs(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def records(self):
        """Device address of the M 16-byte result records (bmx_record) of the last scan."""
        a = C.c_void_p()
        _lib.check(self._L.bmx_ctx_records(self._h, C.byref(a)))
        return a.value

    def fetch_records(self):
        """The last scan's results as a structured array (clr f8, lin i4, nsites i4)."""
        rec = np.empty(self.M, dtype=_lib.RECORD_DTYPE)
        _lib.check(self._L.bmx_ctx_fetch_records(self._h, rec.ctypes.data_as(C.c_void_p)))
        return rec

    def scan_write(self, path, phys, gen_label, xs, abs_, As, chunk=0):
        """Scan the test sites set by set_tests and append the reference's rows to `path` while scanning
        (chunks of test sites; a writer thread formats chunk i while chunk i+1 is on the device)."""
        phys, gen_label = _lib.i64(phys), _lib.f64(gen_label)
        if len(phys) != self.M or len(gen_label) != self.M:
            raise ValueError('one (physPos, genPos) label pair per test site is needed')
        pack = lambda v: b'\0'.join(s.encode() for s in v) + b'\0'
        _lib.check(self._L.bmx_ctx_scan_write(self._h, path.encode(), _lib.as_lp(phys), _lib.as_dp(gen_label), pack(xs), len(xs),
                                              pack(abs_), len(abs_), pack(As), len(As), int(chunk)))

    def permute_rows(self, key, block=1):
        """Permute the selected slot's site rows on the device: row[i] = given_row[sigma(i)], sigma =
        null.block_permutation(N, key, block).  Always from the rows given to set_sites."""
        _lib.check(self._L.bmx_ctx_permute_rows(self._h, self._key64(key), int(block)))

    def restore_rows(self):
        """Back to the rows given to set_sites."""
        _lib.check(self._L.bmx_ctx_restore_rows(self._h))

    def null_begin(self):
        """The last scan's CLR becomes the observed one; exceedance counts are zeroed."""
        _lib.check(self._L.bmx_ctx_null_begin(self._h))

    def null_accumulate(self):
        """After a replicate's scan: counts += (clr >= observed); returns the replicate's maximum CLR."""
        return self._ms(self._L.bmx_ctx_null_accumulate)

    def null_fetch(self):
        """(exceedance counts i32[M], number of accumulated replicates)."""
        counts = np.empty(self.M, dtype=np.int32)
        reps = C.c_int32()
        _lib.check(self._L.bmx_ctx_null_fetch(self._h, _lib.as_ip(counts), C.byref(reps)))
        return counts, reps.value

    PROFILES = {'A': 1, 'x': 2, 'abeta': 4}

    def set_profiles(self, which):
        """Profile likelihoods of later scans of every slot: a BMX_PL_* bit set (1 A, 2 x, 4 abeta; 0 off), one name
        ('A', 'x', 'abeta') or an iterable of names."""
        if isinstance(which, str):
            which = [which]
        if not isinstance(which, (int, np.integer)):
            which = sum(self.PROFILES[n] for n in set(which))
        _lib.check(self._L.bmx_ctx_set_profiles(self._h, int(which)))

    def fetch_profile(self, which):
        """f64 [M][n] of one profile ('A', 'x', 'abeta' or its bit) of the selected slot's last scan, the model's grid order."""
        bit = self.PROFILES[which] if isinstance(which, str) else int(which)
        n = {1: self.nA, 2: len(self.model.x), 4: len(self.model.abeta)}.get(bit, 0)
        out = np.empty((self.M, max(n, 1)), dtype=np.float64)
        _lib.check(self._L.bmx_ctx_fetch_profile(self._h, bit, _lib.as_dp(out)))
        return out[:, :n]

    def eval_points(self, A, x, abeta):
        """T (f64[M], -inf where the window is empty) and nSites (i32[M]) of every test site of the selected slot at the
        point (A[t], x[t], abeta[t]) -- the refinement's arithmetic (ballermixplus_amd/refine.py).  Scalars broadcast."""
        A, x, abeta = self._points(A, x, abeta)
        T, ns = np.empty(self.M, dtype=np.float64), np.empty(self.M, dtype=np.int32)
        _lib.check(self._L.bmx_ctx_eval_points(self._h, _lib.as_dp(A), _lib.as_dp(x), _lib.as_dp(abeta), _lib.as_dp(T),
                                               _lib.as_ip(ns)))
        return T, ns

    def refine(self, min_clr=0.0):
        """Refine the selected slot's last scan off the grid (windows with a grid result and CLR >= min_clr)."""
        _lib.check(self._L.bmx_ctx_refine(self._h, float(min_clr)))

    def fetch_refined(self):
        """The last refinement: {'clr', 'A', 'x', 'abeta': f64[M], 'nsites', 'rounds': i32[M]} (rounds -1: not refined;
        rows that did not improve carry the scan's values)."""
        M = self.M
        out = {k: np.empty(M, dtype=np.float64) for k in ('clr', 'A', 'x', 'abeta')}
        out.update({k: np.empty(M, dtype=np.int32) for k in ('nsites', 'rounds')})
        _lib.check(self._L.bmx_ctx_fetch_refined(self._h, _lib.as_dp(out['clr']), _lib.as_dp(out['A']), _lib.as_dp(out['x']),
                                                 _lib.as_dp(out['abeta']), _lib.as_ip(out['nsites']), _lib.as_ip(out['rounds'])))
        return out

    def support(self, drop, min_clr=0.0):
        """Support intervals (ballermixplus_amd/support.py) around the refined maxima of the selected slot's last refinement:
        windows with a refined CLR >= min_clr, threshold T* - drop."""
        _lib.check(self._L.bmx_ctx_support(self._h, float(drop), float(min_clr)))

    def fetch_support(self):
        """The last support intervals, per test site t, coordinate k (0: A, 1: x, 2: alpha_beta) and side (0: lo, 1: hi):
        'end' f64[M, 3, 2] (natural units; 'lo' and 'hi' are its two sides), 'witness' / 'outside' f64[M, 3, 2, 3] (natural
        A, x, alpha_beta), 'witness_T' / 'outside_T' f64[M, 3, 2], 'censored', 'rounds' (-1: not computed), 'evals' i32[M, 3, 2];
        'T_star', 'T_best' f64[M].  NaN where not computed."""
        M = self.M
        out = {k: np.empty((M, 3, 2), dtype=np.float64) for k in ('end', 'witness_T', 'outside_T')}
        out.update({k: np.empty((M, 3, 2, 3), dtype=np.float64) for k in ('witness', 'outside')})
        out.update({k: np.empty((M, 3, 2), dtype=np.int32) for k in ('censored', 'rounds', 'evals')})
        out.update({k: np.empty(M, dtype=np.float64) for k in ('T_star', 'T_best')})
        d, i = _lib.as_dp, _lib.as_ip
        _lib.check(self._L.bmx_ctx_fetch_support(self._h, d(out['end']), d(out['witness']), d(out['witness_T']), d(out['outside']),
                                                 d(out['outside_T']), i(out['censored']), d(out['T_star']), d(out['T_best']),
                                                 i(out['rounds']), i(out['evals'])))
        out['lo'], out['hi'] = out['end'][:, :, 0], out['end'][:, :, 1]
        return out

    def eval_points_weighted(self, key, block, A, x, abeta):
        """T_w (f64[M], -inf where no site of the window has a positive weight) and the sum of the weights of the window's
        sites at that A (i64[M]) of every test site of the selected slot at the point (A[t], x[t], abeta[t]), under the
        block-bootstrap weights of (key, block) -- the bootstrap's arithmetic (ballermixplus_amd/boot.py).  Scalars broadcast."""
        A, x, abeta = self._points(A, x, abeta)
        T, ws = np.empty(self.M, dtype=np.float64), np.empty(self.M, dtype=np.int64)
        _lib.check(self._L.bmx_ctx_eval_points_weighted(self._h, self._key64(key), int(block), _lib.as_dp(A),
                                                        _lib.as_dp(x), _lib.as_dp(abeta), _lib.as_dp(T), _lib.as_lp(ws)))
        return T, ws

    def boot(self, keys, block=1, min_clr=0.0):
        """Block bootstrap (ballermixplus_amd/boot.py) of the refined maxima of the selected slot's last refinement: one
        replicate per key (boot.replicate_key) for every window with a refined CLR >= min_clr."""
        k = np.array([self._key64(v).value for v in keys], dtype=np.uint64)
        _lib.check(self._L.bmx_ctx_boot(self._h, k.ctypes.data_as(C.POINTER(C.c_uint64)), len(k), int(block), float(min_clr)))

    def fetch_boot(self):
        """The last bootstrap: 'window' i32[n_sel] (the bootstrapped test sites, ascending), 'A', 'x', 'abeta', 'T',
        'T_centre' f64[n_sel, R] and 'rounds' i32[n_sel, R]; T = -inf: the replicate is not ok."""
        n, R = C.c_int64(), C.c_int32()
        _lib.check(self._L.bmx_ctx_boot_count(self._h, C.byref(n), C.byref(R)))
        n, R = n.value, R.value
        out = {'window': np.empty(n, dtype=np.int32), 'rounds': np.empty((n, R), dtype=np.int32)}
        out.update({k: np.empty((n, R), dtype=np.float64) for k in ('A', 'x', 'abeta', 'T', 'T_centre')})
        d = _lib.as_dp
        _lib.check(self._L.bmx_ctx_fetch_boot(self._h, _lib.as_ip(out['window']), d(out['A']), d(out['x']), d(out['abeta']),
                                              d(out['T']), d(out['T_centre']), _lib.as_ip(out['rounds'])))
        return out

    def slot_count(self):
        """Number of slot indices in use (highest selected slot + 1)."""
        return int(self._L.bmx_ctx_slot_count(self._h))

    def resample_sites(self, src_slot, key, block=1):
        """The selected slot receives the resampled sites of slot src_slot under the block-bootstrap weights of (key, block)
        (ballermixplus_amd/locate.py: np.repeat of positions and rows by boot.site_weights), built on the device; the slot is
        then as after set_sites of those arrays.  Returns the number of resampled sites (0: the slot has no sites)."""
        n = C.c_int64()
        _lib.check(self._L.bmx_ctx_resample_sites(self._h, int(src_slot), self._key64(key), int(block), C.byref(n)))
        self._sites_replaced()
        self.N = n.value
        return n.value

    def fetch_sites(self, N=None):
        """(genpos f64[N], rows i32[N]) of the selected slot as the device holds them; N: the slot's number of sites (default:
        that of the last set_sites / resample_sites call of this wrapper)."""
        N = int(self.N if N is None else N)
        g, r = np.empty(N, dtype=np.float64), np.empty(N, dtype=np.int32)
        _lib.check(self._L.bmx_ctx_fetch_sites(self._h, _lib.as_dp(g), _lib.as_ip(r)))
        return g, r

    def locate_begin(self, lo, hi, R):
        """Start the position bootstrap's reduction on the selected slot: one inclusive range [lo[k], hi[k]] into its test
        sites per peak, R replicates."""
        lo, hi = _lib.i32(lo), _lib.i32(hi)
        if lo.shape != hi.shape or lo.ndim != 1:
            raise ValueError('one (lo, hi) pair per peak is needed')
        _lib.check(self._L.bmx_ctx_locate_begin(self._h, len(lo), _lib.as_ip(lo), _lib.as_ip(hi), int(R)))
        self._locate_shape[self.slot] = (int(R), len(lo))

    def locate_accumulate(self, r):
        """After the scan of replicate r: per peak, the argmax row of its range and the CLR there."""
        _lib.check(self._L.bmx_ctx_locate_accumulate(self._h, int(r)))

    def fetch_locate(self):
        """(row i32[R, K], clr f64[R, K]) of the reduction begun by locate_begin: row -1 where a replicate has no argmax."""
        R, K = self._locate_shape.get(self.slot, (0, 0))       # (none: the library refuses the call)
        row, clr = np.empty((R, K), dtype=np.int32), np.empty((R, K), dtype=np.float64)
        _lib.check(self._L.bmx_ctx_fetch_locate(self._h, _lib.as_ip(row), _lib.as_dp(clr)))
        return row, clr

    def plant_sites(self, src_slot, key, centres, iA, ix, ia, gw):
        """The selected slot receives slot src_slot's positions and current rows with the sites in reach of `centres` redrawn
        from the mixture at grid point (iA, ix, ia) under `key` (ballermixplus_amd/power.py: planted_rows), built on the device;
        the slot is then as after set_sites of those arrays.  gw: power.allowed_rows' weights, one per table row.  Returns
        (first i32[K], count i32[K]: every centre's run of sites with A |g - c| <= alpha_cut; sites whose row changed)."""
        c = _lib.f64(centres)
        w = _lib.f64(gw)
        if c.ndim != 1 or w.shape != (self.model.rows,):
            raise ValueError('a flat list of centres and one weight per table row are needed')
        first, count = np.zeros(len(c), dtype=np.int32), np.zeros(len(c), dtype=np.int32)
        changed = C.c_int64()
        _lib.check(self._L.bmx_ctx_plant_sites(self._h, int(src_slot), self._key64(key), len(c), _lib.as_dp(c), int(iA), int(ix),
                                               int(ia), _lib.as_dp(w), _lib.as_ip(first), _lib.as_ip(count), C.byref(changed)))
        self._sites_replaced()
        return first, count, changed.value

    def plant_ms(self):
        """Device milliseconds of the context's last plant_sites() call."""
        return self._ms(self._L.bmx_ctx_plant_ms)

    def fetch_at(self, tests):
        """(clr f64[n], lin i32[n], nsites i32[n]) of the selected slot's last scan at the listed test sites (any order, repeats
        allowed); -1 gives (0, -1, 0).  lin: the linear grid index (iA * nx + ix) * nab + ia, -1 without a grid result."""
        t = _lib.i32(tests)
        if t.ndim != 1:
            raise ValueError('a flat list of test site indices is needed')
        clr, lin, ns = np.empty(len(t), dtype=np.float64), np.empty(len(t), dtype=np.int32), np.empty(len(t), dtype=np.int32)
        _lib.check(self._L.bmx_ctx_fetch_at(self._h, len(t), _lib.as_ip(t), _lib.as_dp(clr), _lib.as_ip(lin), _lib.as_ip(ns)))
        return clr, lin, ns

    def peaks(self, sep, min_clr=0.0, frac=0.5):
        """Call peaks (ballermixplus_amd/peaks.py) on the selected slot's last scan: separation sep in the units of the test
        positions, floor min_clr, extent fraction frac.  Returns fetch_peaks()."""
        _lib.check(self._L.bmx_ctx_peaks(self._h, float(sep), float(min_clr), float(frac)))
        return self.fetch_peaks()

    def peaks_track(self, gen, clr, sep, min_clr=0.0, frac=0.5):
        """The same kernels on a track given by the caller (positions gen non-decreasing, values clr); needs no model."""
        g, c = _lib.f64(gen), _lib.f64(clr)
        if g.shape != c.shape or g.ndim != 1:
            raise ValueError('one position per value is needed')
        _lib.check(self._L.bmx_ctx_peaks_track(self._h, len(g), _lib.as_dp(g), _lib.as_dp(c), float(sep), float(min_clr),
                                               float(frac)))
        return self.fetch_peaks()

    def fetch_peaks(self):
        """The selected slot's last peak call, per apex in row order: {'row', 'lo', 'hi', 'saddle_lo', 'saddle_hi': i32[K]}
        (lo .. hi: the extent; saddle rows -1 where there is none)."""
        n = C.c_int64()
        _lib.check(self._L.bmx_ctx_peak_count(self._h, C.byref(n), None))
        out = {k: np.empty(n.value, dtype=np.int32) for k in ('row', 'lo', 'hi', 'saddle_lo', 'saddle_hi')}
        i = _lib.as_ip
        _lib.check(self._L.bmx_ctx_fetch_peaks(self._h, i(out['row']), i(out['lo']), i(out['hi']), i(out['saddle_lo']),
                                               i(out['saddle_hi'])))
        return out

    def peaks_ms(self):
        """Device milliseconds of the context's last peak call."""
        return self._ms(self._L.bmx_ctx_peaks_ms)

    def refine_at_peaks(self, on=True):
        """Later refine() calls take only the apexes of their slot's peaks() call on the same scan (min_clr still applies)."""
        _lib.check(self._L.bmx_ctx_refine_at_peaks(self._h, 1 if on else 0))

    def surface(self, test_gen, win_lo, win_hi):
        """T[nA, nx, nab] (NaN where the window is empty) and nsites[nA] of one test site."""
        m = self.model
        T = np.empty((self.nA, len(m.x), len(m.abeta)), dtype=np.float64)
        ns = np.empty(self.nA, dtype=np.int32)
        _lib.check(self._L.bmx_ctx_surface(self._h, float(test_gen), int(win_lo), int(win_hi), _lib.as_dp(T),
                                           _lib.as_ip(ns)))
        return T, ns

    def surfaces(self, tests):
        """T[n, nA, nx, nab] (NaN where the window is empty at that A) and nsites[n, nA] of the listed test sites of the
        selected slot (indices into its test sites: any order, repeats allowed), each bitwise surface()'s."""
        m = self.model
        t = _lib.i32(tests)
        if t.ndim != 1:
            raise ValueError('a flat list of test site indices is needed')
        T = np.empty((len(t), self.nA, len(m.x), len(m.abeta)), dtype=np.float64)
        ns = np.empty((len(t), self.nA), dtype=np.int32)
        _lib.check(self._L.bmx_ctx_surfaces(self._h, len(t), _lib.as_ip(t), _lib.as_dp(T), _lib.as_ip(ns)))
        return T, ns

    def surfaces_ms(self):
        """Device milliseconds of the kernels of the context's last surfaces() call."""
        return self._ms(self._L.bmx_ctx_surfaces_ms)

    def influence(self, tests, block):
        """The delete-block jackknife (ballermixplus_amd/influence.py) of the listed test sites of the selected slot (any order,
        repeats allowed) with blocks of `block` consecutive sites.  Returns a dict: per window T_max f64[n], lin i32[n], ns_min
        i32[n], first_block i64[n], offset i64[n + 1]; per block of the windows' ranges, window w's at offset[w]:offset[w + 1],
        m i32, contrib f64, L f64, blin i32."""
        t = _lib.i32(tests)
        if t.ndim != 1:
            raise ValueError('a flat list of test site indices is needed')
        _lib.check(self._L.bmx_ctx_influence(self._h, len(t), _lib.as_ip(t), int(block)))
        n = C.c_int64()
        first, off = np.empty(len(t), dtype=np.int64), np.empty(len(t) + 1, dtype=np.int64)
        _lib.check(self._L.bmx_ctx_influence_count(self._h, C.byref(n), _lib.as_lp(first), _lib.as_lp(off)))
        nb = int(off[-1])
        out = {'T_max': np.empty(len(t)), 'lin': np.empty(len(t), dtype=np.int32), 'ns_min': np.empty(len(t), dtype=np.int32),
               'first_block': first, 'offset': off, 'm': np.empty(nb, dtype=np.int32), 'contrib': np.empty(nb), 'L': np.empty(nb),
               'blin': np.empty(nb, dtype=np.int32)}
        i, d = _lib.as_ip, _lib.as_dp
        _lib.check(self._L.bmx_ctx_fetch_influence(self._h, d(out['T_max']), i(out['lin']), i(out['ns_min']), i(out['m']),
                                                   d(out['contrib']), d(out['L']), i(out['blin'])))
        return out

    def influence_ms(self):
        """Device milliseconds of the kernels of the context's last influence() call (the surfaces' kernel among them)."""
        return self._ms(self._L.bmx_ctx_influence_ms)

    def fit(self, tests, lin, gw, cls, F, edges):
        """Observed against expected frequency spectrum by distance (ballermixplus_amd/fit.py) of the listed test sites of the
        selected slot (any order, repeats allowed), window q at the grid point lin[q] = (iA * nx + ix) * nab + ia (< 0: O all 0,
        E NaN).  gw f64[rows]: power.allowed_rows(); cls i32[rows] in [0, F): fit.classes(); edges f64[D - 1] ascending.
        Returns (O i32[n, D, F], E_sel f64[n, D, F], E_neu f64[n, D, F], skipped i32[n])."""
        t, l = _lib.i32(tests), _lib.i32(lin)
        if t.ndim != 1 or l.shape != t.shape:
            raise ValueError('a flat list of test site indices and one grid point per entry are needed')
        gw, cls, edges = _lib.f64(gw), _lib.i32(cls), _lib.f64(edges)
        if gw.shape != (self.model.rows,) or cls.shape != gw.shape or edges.ndim != 1:
            raise ValueError('gw and cls need one entry per table row, edges a flat list')
        F, D = int(F), len(edges) + 1
        shape = (len(t), D, max(F, 0))
        O, skipped = np.empty(shape, dtype=np.int32), np.empty(len(t), dtype=np.int32)
        Es, En = np.empty(shape), np.empty(shape)
        _lib.check(self._L.bmx_ctx_fit(self._h, len(t), _lib.as_ip(t), _lib.as_ip(l), _lib.as_dp(gw), _lib.as_ip(cls), F,
                                       _lib.as_dp(edges), D, _lib.as_ip(O), _lib.as_dp(Es), _lib.as_dp(En), _lib.as_ip(skipped)))
        return O, Es, En, skipped

    def fit_ms(self):
        """Device milliseconds of the kernel of the context's last fit() call."""
        return self._ms(self._L.bmx_ctx_fit_ms)

    def cond_surfaces(self, tests, cond_test, cond_lin, want_T=True):
        """Conditional surfaces (ballermixplus_amd/conditional.py) of the listed pairs on the selected slot: pair q is the window
        of test site tests[q] given the conditioning locus cond_test[q] (a test site, -1: none) held at the grid point
        cond_lin[q] = (iA * nx + ix) * nab + ia (< 0: none).  Returns a dict: T f64[n, nA, nx, nab] (None without want_T: the
        surfaces are then not copied back), nsites i32[n, nA], nshared i32[n, nA], tmax f64[n] and lin i32[n] (the scan's rule on
        each pair's T; 0 and -1 when nothing is > 0)."""
        t, ct, cl = _lib.i32(tests), _lib.i32(cond_test), _lib.i32(cond_lin)
        if t.ndim != 1 or ct.shape != t.shape or cl.shape != t.shape:
            raise ValueError('a flat list of test site indices and one conditioning site and grid point per entry are needed')
        return self._sided_surfaces(self._L.bmx_ctx_cond_surfaces, (_lib.as_ip(t), _lib.as_ip(ct), _lib.as_ip(cl)), len(t), want_T)

    def _sided_surfaces(self, call, lists, n, want_T):
        """cond_surfaces' and base_surfaces' dict, filled by `call` (their entry point) on the list(s) of n entries."""
        m = self.model
        nx, nab = (len(m.x), len(m.abeta)) if m is not None else (0, 0)        # (no model yet: the library answers BMX_E_STATE)
        out = {'T': np.empty((n, self.nA, nx, nab), dtype=np.float64) if want_T else None,
               'nsites': np.empty((n, self.nA), dtype=np.int32), 'nshared': np.empty((n, self.nA), dtype=np.int32),
               'tmax': np.empty(n, dtype=np.float64), 'lin': np.empty(n, dtype=np.int32)}
        _lib.check(call(self._h, n, *lists, _lib.as_dp(out['T']) if want_T else None, _lib.as_ip(out['nsites']),
                        _lib.as_ip(out['nshared']), _lib.as_dp(out['tmax']), _lib.as_ip(out['lin'])))
        return out

    def cond_surfaces_ms(self):
        """Device milliseconds of the kernels of the context's last cond_surfaces() call."""
        return self._ms(self._L.bmx_ctx_cond_surfaces_ms)

    def baseline_reset(self):
        """Allocate or zero the selected slot's baseline of accepted loci (ballermixplus_amd/stepwise.py): d = 0.0 and cnt = 0 for
        every site.  set_sites, resample_sites and plant_sites drop it."""
        _lib.check(self._L.bmx_ctx_baseline_reset(self._h))

    def baseline_add(self, test, lin):
        """Add the locus `test site test held at the grid point lin = (iA * nx + ix) * nab + ia` to the selected slot's
        baseline.  Returns (first, last, n_written): the first and last site index written and how many were (first > last and
        0 for a locus without a site)."""
        first, last, n = C.c_int64(), C.c_int64(), C.c_int32()
        _lib.check(self._L.bmx_ctx_baseline_add(self._h, int(test), int(lin), C.byref(first), C.byref(last), C.byref(n)))
        return first.value, last.value, n.value

    def baseline_fetch(self, N=None):
        """(d f64[N], cnt i32[N]) of the selected slot's baseline; N: the slot's number of sites (default: as fetch_sites)."""
        N = int(self.N if N is None else N)
        d, cnt = np.empty(N, dtype=np.float64), np.empty(N, dtype=np.int32)
        _lib.check(self._L.bmx_ctx_baseline_fetch(self._h, _lib.as_dp(d), _lib.as_ip(cnt)))
        return d, cnt

    def base_surfaces(self, tests, want_T=True):
        """The surfaces of the listed test sites of the selected slot (any order, repeats allowed) against its baseline of
        accepted loci (ballermixplus_amd/stepwise.py).  Returns cond_surfaces' dict: T f64[n, nA, nx, nab] (None without want_T:
        the surfaces are then not copied back), nsites i32[n, nA], nshared i32[n, nA] (the sites an accepted locus reaches),
        tmax f64[n] and lin i32[n] (the scan's rule on each window's T; 0 and -1 when nothing is > 0)."""
        t = _lib.i32(tests)
        if t.ndim != 1:
            raise ValueError('a flat list of test site indices is needed')
        return self._sided_surfaces(self._L.bmx_ctx_base_surfaces, (_lib.as_ip(t),), len(t), want_T)

    def base_surfaces_ms(self):
        """Device milliseconds of the kernels of the context's last base_surfaces() call."""
        return self._ms(self._L.bmx_ctx_base_surfaces_ms)

    def sandwich(self, tests, A, x, abeta, block=1, hx=None, hv=None):
        """The pieces of the sandwich variance (ballermixplus_amd/sandwich.py) of the listed windows of the selected slot, window
        q at the point (A[q], x[q], abeta[q]) (scalars broadcast over the list), blocks of `block` consecutive sites, steps
        hx, hv of the table's central differences (default: sandwich.HX, sandwich.HV).  Returns a dict: T f64[n], g f64[n, 3],
        H f64[n, 6] and J f64[n, 6] (uu, ux, uv, xx, xv, vv of (ln A, x, ln alpha_beta)), nsites, nskipped, nblocks i32[n]."""
        from . import sandwich
        t = _lib.i32(tests)
        if t.ndim != 1:
            raise ValueError('a flat list of test site indices is needed')
        n = len(t)
        pA, px, pab = (_lib.f64(np.broadcast_to(np.asarray(v, dtype=np.float64), (n,))) for v in (A, x, abeta))
        out = {'T': np.empty(n, dtype=np.float64), 'g': np.empty((n, 3), dtype=np.float64), 'H': np.empty((n, 6), dtype=np.float64),
               'J': np.empty((n, 6), dtype=np.float64)}
        out.update({k: np.empty(n, dtype=np.int32) for k in ('nsites', 'nskipped', 'nblocks')})
        _lib.check(self._L.bmx_ctx_sandwich(self._h, n, _lib.as_ip(t), _lib.as_dp(pA), _lib.as_dp(px), _lib.as_dp(pab), int(block),
                                            float(sandwich.HX if hx is None else hx), float(sandwich.HV if hv is None else hv),
                                            _lib.as_dp(out['T']), _lib.as_dp(out['g']), _lib.as_dp(out['H']), _lib.as_dp(out['J']),
                                            _lib.as_ip(out['nsites']), _lib.as_ip(out['nskipped']), _lib.as_ip(out['nblocks'])))
        return out

    def sandwich_ms(self):
        """Device milliseconds of the kernels of the context's last sandwich() call."""
        return self._ms(self._L.bmx_ctx_sandwich_ms)

    def refine_R(self, x, abeta):
        """R f64[table rows] at the off-grid point (x, abeta): the refinement's own arithmetic for every row of the model."""
        R = np.empty(self.model.rows if self.model is not None else 0, dtype=np.float64)   # (no model yet: BMX_E_STATE)
        _lib.check(self._L.bmx_ctx_refine_R(self._h, float(x), float(abeta), _lib.as_dp(R)))
        return R

    def fetch_lut(self):
        m = self.model
        shape = (len(m.x), len(m.abeta), m.rows)
        psel, R = np.empty(shape), np.empty(shape)
        _lib.check(self._L.bmx_ctx_fetch_lut(self._h, _lib.as_dp(psel), _lib.as_dp(R)))
        return psel, R


class Comm:
    """The library's own RCCL communicator (bmx_comm_*): one per (context, process group).  `make_id()` on rank 0, the 128 bytes
    to the other ranks by any channel, then Comm(ctx, id, rank, world) on every rank (collective)."""

    @staticmethod
    def make_id():
        buf = C.create_string_buffer(128)
        _lib.check(_lib.lib().bmx_comm_unique_id(buf))
        return buf.raw

    def __init__(self, ctx, comm_id, rank, world):
        self._L = _lib.lib()
        self._h = C.c_void_p()
        self.ctx, self.rank, self.world = ctx, int(rank), int(world)
        _lib.check(self._L.bmx_comm_create(C.byref(self._h), ctx._h, comm_id, self.rank, self.world))

    def gather_records(self, counts, root=0, out=None):
        """ONE gather of the context's packed records to `root` (ncclSend / ncclRecv inside the library, device to device).
        Root: a RECORD array of sum(counts) records, rank after rank (`out` if given); other ranks: None."""
        cnt = _lib.i64(counts)
        if len(cnt) != self.world:
            raise ValueError('one count per rank is needed')
        rec = None
        if self.rank == root:
            rec = out if out is not None else np.empty(int(cnt.sum()), dtype=_lib.RECORD_DTYPE)
        ptr = rec.ctypes.data_as(C.c_void_p) if rec is not None else None
        _lib.check(self._L.bmx_comm_gather_records(self._h, _lib.as_lp(cnt), int(root), ptr, None))
        return rec

    def close(self):
        if self._h:
            self._L.bmx_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NormalizedBetaBinom:
    """Drop-in for the reference class of the same name (v1:310-433): same constructor
    arguments; `get(x, a)` returns the per-site normalised selection probabilities.  The table
    is built by the device kernel (K1) and stays resident for calcBaller / scan_batch.
    The device table also folds in the neutral spectrum (R = P_sel*prop/g - 1), which the
    reference only supplies at calcBaller time, so the device state is created on first use
    (`bind`), when the NeutralSFS is known."""

    def __init__(self, InputData, Grids, nofreq, MAF, nosub, device=0, ctx=None):
        # ctx: an empty Context created ahead of time (the CLI brings the HIP runtime up while it parses the input)
        self._fresh_ctx = ctx
        self.stat = stat_name(nofreq, MAF, nosub)
        self.grid_x, self.grid_abeta, self.grid_A = Grids.scan_order()
        self._data = InputData
        self.site_gen = InputData.genPos          # (work-balanced sharding estimates window sizes from the site positions)
        self._device = device
        self._bound_to = None
        self.ctx = None
        self._psel = None
        self._key = {}
        for i, x in enumerate(self.grid_x):
            for j, a in enumerate(self.grid_abeta):
                self._key[(x, a)] = (i, j)

    def bind(self, NeutralSFS, reuse=None):
        """Create (once per NeutralSFS) the resident context: K1 table + site arrays in HBM.
        reuse: a Context that already holds this model and A grid (e.g. the previous chromosome's, whole-genome runs):
        its table and buffers are kept and only the site arrays are replaced."""
        if self._bound_to is NeutralSFS and self.ctx is not None:
            return self
        self.prepare(NeutralSFS)
        d = self._data
        if self.ctx is not None and self.ctx is not reuse:
            self.ctx.close()
        akey = tuple(float(a) for a in self.grid_A)
        same_dev = reuse is not None and reuse.device == self._device
        if same_dev and getattr(reuse, 'model', None) is not None and reuse.model.key == self.model.key and \
                getattr(reuse, 'A_key', None) == akey:
            self.ctx = reuse                      # same table: kept, only the site arrays are replaced
            self.ctx.model = self.model
            self.table_reused = True
        else:
            if same_dev:
                self.ctx = reuse                  # same GPU, another model (a chromosome with other sample sizes, another
                                                  # minCount, ...): the context and its buffers are kept, the table is rebuilt
            elif self._fresh_ctx is not None and self._fresh_ctx.device == self._device:
                self.ctx, self._fresh_ctx = self._fresh_ctx, None
            else:
                self.ctx = Context(self._device)
            self.ctx.set_model(self.model, self.grid_A)
            self.ctx.A_key = akey
            self.table_reused = False
        self.ctx.set_sites(d.genPos, self.rows)
        self._bound_to = NeutralSFS
        self._psel = None
        return self

    def rebind(self, NeutralSFS, ctx):
        """bind() again into ctx after another file's sites have replaced this one's there (cli.wrap_up)."""
        self._bound_to = None
        return self.bind(NeutralSFS, reuse=ctx)

    def prepare(self, NeutralSFS):
        """The host half of bind(): the bmx_model arrays and every site's table row.  No device call, so a whole-genome run
        does it for the next chromosome on a helper thread while the current one is scanned (cli.main_many)."""
        if getattr(self, '_prepared_for', self) is NeutralSFS and getattr(self, 'model', None) is not None:
            return self
        d = self._data
        if NeutralSFS is None:      # get() before any scan: neutral part is irrelevant to P_sel
            spect = {(k, int(n)): 1.0 for n in d.sampSizes for k in range(int(n) + 1)}
            props = {int(n): 1.0 for n in d.sampSizes}
        else:
            spect, props = NeutralSFS.spect, NeutralSFS.sampProps
        self.model = ModelArrays(self.stat, d.minCount, d.sampSizes, spect, props, self.grid_x, self.grid_abeta)
        self.rows = self.model.rows_of(d.count, d.total)
        self._prepared_for = NeutralSFS
        return self

    def get(self, x, a):
        """v1:362-363"""
        if self.ctx is None:
            self.bind(None)
        if self._psel is None:
            self._psel, _ = self.ctx.fetch_lut()
        i, j = self._key[(x, a)]
        return self._psel[i, j][self.rows]


def scan_stream(sel, test_gen, win_lo, win_hi, outfile, phys, gen_label, fetch=True):
    """scan_batch + the output rows appended to `outfile` while the scan runs (the reference writes as it scans,
    v1:599-608).  Returns what scan_batch returns (None with fetch=False: the file is all the caller wants)."""
    sel.ctx.set_tests(test_gen, win_lo, win_hi)
    # chunks of 64k test sites keep the first rows early on small inputs; large inputs take 256k per chunk (fewer kernel tails)
    sel.ctx.scan_write(outfile, phys, gen_label, [f'{v}' for v in sel.grid_x], [f'{v}' for v in sel.grid_abeta],
                       [f'{v}' for v in sel.grid_A], chunk=262144 if len(phys) >= (1 << 20) else 0)
    return sel.ctx.fetch() if fetch else None


def scan_batch(sel, test_gen, win_lo, win_hi):
    """All test sites at once.  Returns (clr f64[M], ix, ia, iA, nsites) with indices into the
    iteration-order grids held by `sel` (iA == -1: the reference's all-zero row)."""
    sel.ctx.set_tests(test_gen, win_lo, win_hi)
    sel.ctx.scan()
    return sel.ctx.fetch()


def calcBaller(window_indice, testSite, InputData, NeutralSFS, NormalizedBetaBinom, Grids):
    """Drop-in for v1:436-507 (one test site).  `window_indice` must be a contiguous index
    range, which is all the reference ever passes (v1:538,572,589,606).  Returns
    [T, x, abeta, A, nSites] with the grid's own Python objects, or the all-zero list."""
    w = np.asarray(window_indice)
    NormalizedBetaBinom.bind(NeutralSFS)
    clr, ix, ia, iA, ns = scan_batch(NormalizedBetaBinom, [float(testSite)], [int(w[0])], [int(w[-1])])
    if iA[0] < 0:
        return [0., 0., 0., 0., 0.]
    s = NormalizedBetaBinom
    return [float(clr[0]), s.grid_x[ix[0]], s.grid_abeta[ia[0]], s.grid_A[iA[0]], int(ns[0])]
