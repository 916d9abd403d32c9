"""Cases of tests/test_gpu_fold_tails.py, tests/test_fold_tails_cpu.py and tests/golden/gen_fold_tails.py: the smallest shapes at
which arithmetic of the prepared scan kernels that the result does not need can be skipped wrongly --
  the last block of a near list: pair steps of two neutral entries are skipped, a quad block with one or two real entries takes
  the one- or two-site form: every remainder of real entries (0 .. 3 in blocks of 4, 0 .. 7 in the pair blocks of 8 of the
  8-test-site kernel), lists of a single block, lists without any entry, a quad list past 12 x 64 entries (no budget byte left);
  the fold of a moment entry whose higher moments are exactly zero (top order K = the largest k with M_k != 0): every K from 2
  to 12, fold steps whose two entries differ in K, odd numbers of entries, a single entry, moments on one side only.  (Stopping
  the fold at K was built, measured slower and dropped -- DESIGN 4 -- the cases stay for whoever tries again.)
The data sets, the grid and the windows are those of tests/streamscalars.py (N = 4000 sites, n = 20: table in LDS; n = 40 .. 50:
table in L2; 65 grid pairs: the second slice has one real lane); what is new is the A lists: a ladder from A = 500 (zones of
2000 sites: a quad list of a thousand entries, every slot full) to 1e6 (zones of two or three sites, most lists empty), so that
a slot holds anything from hundreds of far sites (K = 12) down to one site far out (K = 2).

census() restates prep_kernel's classification (slot of a row, far / series / near, the orders a far site adds: P_D) in numpy, on
any table: it is how the A lists and test sites were chosen, and tests/test_fold_tails_cpu.py holds the choice to its counts.
numpy only, apart from run(), which takes the engine from its caller."""
import numpy as np

import streamscalars as ss

N = ss.N
A_LISTS = {
    'ladder': (500.0, 1000.0, 2000.0, 3500.0, 6000.0, 10000.0, 20000.0, 40000.0, 80000.0, 150000.0, 400000.0, 1e6),
    'steep': (3000.0, 8000.0, 15000.0, 30000.0, 60000.0, 100000.0, 250000.0, 600000.0),
}
PREP = ss.PREP
# name -> (data set, A list, test-site indices, windows, variant, profiles, kernel the plan must name)
CASES = {}


def _case(name, data, a, idx, windows='all', variant=0, profiles=0, kernel=None):
    CASES[name] = dict(data=data, a=a, idx=np.asarray(idx, dtype=np.int64), windows=windows, variant=variant, profiles=profiles, kernel=kernel)


_case('dense', 'one', 'ladder', range(2000, 2131), kernel=PREP % (16, 'true'))
_case('dense, steep', 'one', 'steep', range(2600, 2731), kernel=PREP % (16, 'true'))
_case('every 2nd', 'one', 'ladder', range(1401, 2001, 2), kernel=PREP % (16, 'true'))
_case('every 4th, J = 8', 'one', 'ladder', range(1402, 2602, 4), kernel=PREP % (8, 'true'))
_case('every 4th, J = 8, steep', 'one', 'steep', range(1403, 2603, 4), kernel=PREP % (8, 'true'))
# moments on one side only: the first / last sites of the chromosome
_case('chromosome start', 'one', 'ladder', range(0, 40), kernel=PREP % (16, 'true'))
_case('chromosome end', 'one', 'steep', range(N - 37, N), kernel=PREP % (16, 'true'))
# windows that cut the zones short
_case('cut windows', 'one', 'steep', range(2000, 2131), windows='cut', kernel=PREP % (16, 'true'))
_case('cut windows, every 4th', 'one', 'ladder', range(1402, 2602, 4), windows='cut', kernel=PREP % (8, 'true'))
# table in L2: 506 rows, 254 slots, the fold that requests its rows two entries ahead
_case('eleven sizes', 'eleven', 'ladder', range(2000, 2131), kernel=PREP % (16, 'false'))
_case('eleven sizes, every 2nd', 'eleven', 'steep', range(1401, 2001, 2), kernel=PREP % (16, 'false'))
_case('eleven sizes, every 4th', 'eleven', 'ladder', range(1402, 2602, 4), kernel=PREP % (8, 'false'))
# profiles on
_case('profiles', 'one', 'steep', range(2000, 2131), profiles=7, kernel=PREP % (16, 'true'))
_case('profiles, eleven sizes, every 4th', 'eleven', 'steep', range(1402, 2602, 4), profiles=7, kernel=PREP % (8, 'false'))


def windows_of(case):
    """(lo, hi) inclusive index windows of a case, never None."""
    c = CASES[case]
    lo, hi = ss.windows_of(c['idx'], c['windows'])
    if lo is None:
        lo, hi = np.zeros(len(c['idx']), np.int64), np.full(len(c['idx']), N - 1, np.int64)
    return lo, hi


def open_data(eng, data, a):
    """streamscalars.open_data with an A list of this module."""
    gen, k, total, _ = ss.draws(data)
    spect, props = ss.spectrum(data)
    model = eng.ModelArrays('B2', 1, list(ss.SIZES[data]), spect, props, ss.XS, ss.ABETAS)
    rows = model.rows_of(k, total)
    ctx = eng.Context(0)
    ctx.set_model(model, list(A_LISTS[a]))
    ctx.set_sites(gen, rows)
    R = ctx.fetch_lut()[1]
    assert np.isfinite(R[:, :, np.unique(rows)]).all()
    return ctx, gen, rows, np.where(np.isfinite(R), R, 0.0)


def run(ctx, gen, case):
    """Scan one case on a context of its data set: (records, plan, {profile name: array} or None)."""
    c = CASES[case]
    ctx.set_variant(c['variant'])
    ctx.set_profiles(c['profiles'])
    lo, hi = ss.windows_of(c['idx'], c['windows'])
    ctx.set_tests(gen[c['idx']], lo, hi)
    ctx.scan()
    rec = ctx.fetch_records().copy()
    prof = {k: ctx.fetch_profile(k).copy() for k in ('A', 'x', 'abeta')} if c['profiles'] else None
    return rec, ctx.plan(), prof


def oracle(c_scan, L, R, gen, rows, case):
    """streamscalars.oracle for a case of this module: the C oracle's answer and the windows it leaves undecided."""
    import gridshape as gs
    c = CASES[case]
    lo, hi = windows_of(case)
    As = A_LISTS[c['a']]
    ref = c_scan(L, R, As, gen, rows, gen[c['idx']], lo, hi)
    S, ns = gs.surface_sums(L, R, As, gen, rows, gen[c['idx']], np.minimum(lo, N - 1), hi)
    return ref, np.nonzero(gs.decide(S, ns)[3])[0]


check_oracle = ss.check_oracle


# ----------------------------------------------------------------------------- prep_kernel's classification, restated
P_EPS = 0.15                    # far: alpha max|R| <= P_EPS, in the exponent domain: A d >= log(max|R| / P_EPS)
P_D = np.array([9.029, 6.228, 4.56, 3.455, 2.67, 2.084, 1.629, 1.267, 0.972, 0.726])    # a far site adds E^k, k >= 3, while d < P_D[k - 3]
SER_DMIN = 1.629                # a far site without a slot is a series entry from here on (orders up to 8)
SER_CAP, MOM_SLOTS, MOM_SLOTS_LDS = 64, 254, 64
LN2 = 0.6931471805599453        # near entries with A d below it: the pair list
QUAD_BUDGETS = 12 * 64          # quad entries that have a budget byte in the header


def host_data(data, oracle_R):
    """(table R[nx][nab][rows] of the oracle (util.oracle_R), genPos, table row of every site) without a device: one block of
    n + 1 rows per sample size, ascending n."""
    gen, k, total, _ = ss.draws(data)
    spect, props = ss.spectrum(data)
    sizes = sorted(ss.SIZES[data])
    off = dict(zip(sizes, np.concatenate(([0], np.cumsum([n + 1 for n in sizes])))[:-1].tolist()))
    rows = (np.array([off[int(n)] for n in total]) + k).astype(np.int32)
    return oracle_R('B2', sizes, 1, spect, props, ss.XS, ss.ABETAS), gen, rows


def row_tables(R, rows, gen, As, zcut, in_lds):
    """(far threshold of every row in A d, NaN: never far; slot of every row, 255: none; slots in use per A)."""
    nrows = R.shape[2]
    cnt = np.bincount(rows, minlength=nrows)
    order = sorted(range(nrows), key=lambda r: (-cnt[r], r))[:MOM_SLOTS]
    slot = np.full(nrows, 255, np.int64)
    by_slot = [r for r in order if cnt[r] > 0]
    slot[by_slot] = np.arange(len(by_slot))
    with np.errstate(invalid='ignore', divide='ignore'):
        m = np.max(np.abs(R), axis=(0, 1))
        thr = np.where(np.isfinite(m), np.where(m <= P_EPS * 0.36, -1.0, np.maximum(np.log(m / P_EPS) * (1.0 + 1e-12) + 1e-9, -1.0)), np.nan)
    n = len(rows)
    kmom = []
    for A in As:
        nfar = 0.8 * (n - 1) / (gen[-1] - gen[0]) * zcut / A
        k = 0
        while k < len(by_slot) and cnt[by_slot[k]] / n * nfar * 11.0 > 30.0:
            k += 1
        kmom.append(min(k, MOM_SLOTS_LDS if in_lds else MOM_SLOTS))
    return thr, slot, kmom


def census(R, gen, rows, case, zcut):
    """One dict per (group, A, zone) of a case: 'J', 'K' (top orders of the zone's moment entries, in stream order),
    'n_pair', 'n_quad' (real entries), 'side' (+1 right, -1 left)."""
    c = CASES[case]
    J = int(c['kernel'].split('<')[1].split(',')[0])
    in_lds = c['kernel'].endswith('true>')
    As = A_LISTS[c['a']]
    thr, slot, kmom = row_tables(R, rows, gen, As, zcut, in_lds)
    idx = c['idx']
    lo, hi = windows_of(case)
    lo, hi = np.maximum(lo, 0), np.minimum(hi, N - 1)
    tg = gen[idx]
    center, center_hi = np.searchsorted(gen, tg, 'left'), np.searchsorted(gen, tg, 'right')
    out = []
    for tb in range(0, len(idx), J):
        nv = min(J, len(idx) - tb)
        t0, tL = tg[tb], tg[tb + nv - 1]
        lo_max, hi_min = int(lo[tb:tb + nv].max()), int(hi[tb:tb + nv].min())
        L_int, R_int = min(int(center[tb]), hi_min + 1), max(int(center_hi[tb + nv - 1]), lo_max)
        if hi_min < lo_max:
            L_int = R_int = int(center[tb])
            hi_min, lo_max = -1, N
        for iA, A in enumerate(As):
            for side in (+1, -1):
                at = np.arange(R_int, hi_min + 1) if side > 0 else np.arange(L_int - 1, lo_max - 1, -1)
                tnear, tfar = (tL, t0) if side > 0 else (t0, tL)
                bulk = A * np.abs(gen[at] - tfar) <= zcut
                at = at[:len(at) if bulk.all() else int(np.argmin(bulk))]        # the zone: the walk's sites up to the first one out of reach
                zn = A * np.abs(gen[at] - tnear)
                th, sl = thr[rows[at]], slot[rows[at]]
                with np.errstate(invalid='ignore'):
                    far = zn >= th
                    d = zn - th
                mom = far & (sl < kmom[iA])
                serx = far & ~mom & ~(d < SER_DMIN)
                ser = np.zeros(len(at), bool)
                n_ser = 0
                for b in range(0, len(at), 64):                                     # a pass of the wave takes its series entries or none
                    k = int(serx[b:b + 64].sum())
                    if n_ser + k <= SER_CAP:
                        ser[b:b + 64] = serx[b:b + 64]
                        n_ser += k
                near = ~mom & ~ser
                order = 2 + (d[:, None] < P_D[None, :]).sum(axis=1)
                K = [int(order[mom & (sl == s)].max()) for s in np.unique(sl[mom])]
                out.append(dict(J=J, side=side, K=K, n_pair=int((near & (zn < LN2)).sum()), n_quad=int((near & ~(zn < LN2)).sum())))
    return out


def tally(zones):
    """What the cases must cover, counted over a list of census() records."""
    t = dict(order={k: 0 for k in range(2, 13)}, mixed_step=0, odd_occ=0, one_occ=0, one_side=0, quad_tail={r: 0 for r in range(4)},
             pair_tail={16: {r: 0 for r in range(4)}, 8: {r: 0 for r in range(8)}}, single_block=0, empty_pair=0, empty_quad=0, long_quad=0)
    for z in zones:
        K = z['K']
        for k in K:
            t['order'][k] = t['order'].get(k, 0) + 1
        t['mixed_step'] += sum(1 for s in range(0, len(K) - 1, 2) if K[s] != K[s + 1])
        t['odd_occ'] += len(K) % 2
        t['one_occ'] += len(K) == 1
        bs = 4 if z['J'] >= 16 else 8
        if z['n_pair']:
            t['pair_tail'][16 if z['J'] >= 16 else 8][z['n_pair'] % bs] += 1
            t['single_block'] += z['n_pair'] <= bs
        else:
            t['empty_pair'] += 1
        if z['n_quad']:
            t['quad_tail'][z['n_quad'] % 4] += 1
            t['single_block'] += z['n_quad'] <= 4
            t['long_quad'] += z['n_quad'] > QUAD_BUDGETS
        else:
            t['empty_quad'] += 1
    for a, b in zip(zones[0::2], zones[1::2]):          # the two zones of one (group, A)
        t['one_side'] += bool(a['K']) != bool(b['K'])
    return t
