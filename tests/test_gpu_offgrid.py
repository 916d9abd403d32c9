"""The off-grid search kernels (refine_kernel, support_kernel, boot_kernel) on the catalogue of tests/offgrid.py: ragged, empty and
one-sided windows, test positions on ties and between sites, site ranges around the 256-thread stride, every set of free
coordinates, starts on hull corners and on repeated grid values, the workspace on either side of its LDS edge, in the capped slab
with 4-byte row indices, and workgroups that take a second window.  tests/test_offgrid_cpu.py proves with the oracle alone that
the catalogue holds these cases.

  a. the existing checkers (C oracle at 1e-9: check_refined, check_support, check_boot) on the new geometry;
  b. bit for bit: the refined CLR is eval_points at the reported point, a replicate's T and T_centre are eval_points_weighted at
     the reported point and at the refined point;
  c. refine_kernel replayed on the host: offgrid.replay (refine.compass in lockstep) on the objective ctx.eval_points must take the
     device's path -- rounds, the improved flag and the reported point.  On grid 'x' (x alone free: no exp between a coordinate
     and its natural value) every window, bit for bit.  Elsewhere a window is judged when every decision of its path had a
     margin of at least offgrid.MARGIN_BAR = 1e-12; judged windows match in rounds, flag, the bits of x, A and alpha_beta
     within 4 np.spacing and CLR within 1e-12 relative; at least offgrid.JUDGED_SHARE of a case's refined windows must be judged.
     The replay takes exp from the device (the device_exp fixture), not from the host: the two differ in the last bit at 6 % of
     the arguments, and T is so ill-conditioned in alpha_beta (1 ulp moves it by up to 1e-5 at alpha_beta = 1e9) that with the
     host's exp 2 to 8 judged windows of every case whose alpha_beta is free left the device's path, at margins up to 1e-5;
  d. boot_kernel replayed the same way from support.centre on eval_points_weighted, replicates whose centre is -inf included;
  e. weighted point evaluation at block sizes around the stride of 256 against the host restatement;
  f. the workspace: 728 against 729 table rows, slices of the capped slab, halves of a launch whose workgroups stride.
Every test prints what it measured and its wall time."""
import math
import time

import numpy as np
import pytest

import offgrid as og
import test_gpu_boot as tb
import test_gpu_support as tsup
from test_gpu_refine import Problem, _scan_refine, check_refined

from ballermixplus_amd import boot, refine, support

pytestmark = pytest.mark.gpu

CHECKED = [n for n in og.CASES if n != 'stride']
SUPPORT_BOOT = {'small-all-ragged': 64, 'small-corner-ragged': 1, 'large-all-ragged': 64, 'wide729': 1}        # case -> block size


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _ulps(a, b):
    """Distance in units in the last place of two arrays of positive finite doubles."""
    return np.abs(_bits(a).astype(np.int64) - _bits(b).astype(np.int64))


_MODEL = {}


def _model(data, grid):
    if (data, grid) not in _MODEL:
        from ballermixplus_amd import engine as eng
        d = og.dataset(data)
        xs, ab, _ = og.GRIDS[grid]
        model = eng.ModelArrays('B2', 1, d.sizes, d.spect, d.props, xs, ab)
        rows = model.rows_of(d.k, d.nn)
        assert np.array_equal(rows, og.rows_of(data)) and model.rows == og.WIDE_ROWS.get(data, model.rows)
        _MODEL[(data, grid)] = (model, rows)
    return _MODEL[(data, grid)]


@pytest.fixture(scope='module')
def open_ctx():
    """open_ctx(case name) -> the one context of the case's (data set, grid), with that model and the data set's sites in slot 0;
    every context is closed when the module ends."""
    from ballermixplus_amd import engine as eng
    made = {}

    def get(name):
        c = og.CASES[name]
        key = (c.data, c.grid)
        if key not in made:
            model, rows = _model(*key)
            ctx = eng.Context(0)
            made[key] = ctx
            ctx.set_model(model, og.GRIDS[c.grid][2])
            ctx.set_sites(og.dataset(c.data).gen, rows)
        return made[key]

    yield get
    for ctx in made.values():
        ctx.close()


@pytest.fixture(autouse=True)
def _wall_time(request):
    t0 = time.perf_counter()
    yield
    print('%s: wall time %.2f s' % (request.node.name, time.perf_counter() - t0))


def _windows(name, rows=slice(None)):
    tg, idx, lo, hi, _ = og.tests_of(name)
    return tg[rows], lo[rows], hi[rows]


def _run(ctx, name, rows=slice(None)):
    """scan -> refine of the case's windows (or of `rows` of them) on the context's selected slot."""
    tg, lo, hi = _windows(name, rows)
    if og.CASES[name].windows == 'all':
        return _scan_refine(ctx, tg, None, None)                  # no index bounds: the reference's default mode
    return _scan_refine(ctx, tg, lo, hi)


def _problem(name, rows=slice(None)):
    c = og.CASES[name]
    d = og.dataset(c.data)
    xs, ab, As = og.GRIDS[c.grid]
    tg, lo, hi = _windows(name, rows)
    return Problem('B2', 1, d.sizes, d.spect, d.props, d.gen, _model(c.data, c.grid)[1], As, xs, ab, tg, lo, hi)


def _dummy(name, M):
    xs, ab, As = og.GRIDS[og.CASES[name].grid]
    return np.full(M, As[0]), np.full(M, xs[0]), np.full(M, ab[0])


def _improved(scan, ref):
    return _bits(ref['clr']) != _bits(scan[0])


def _same_bytes(a, b, rows=slice(None)):
    return sorted(a) == sorted(b) and all(np.ascontiguousarray(a[k][rows]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in a)


def _same_search(full, part, rows, grid):
    """(scan, refined) of a full run against those of `rows` of its windows run on their own: everything the search made, byte for
    byte.  A scan's CLR may differ in its last bits between two sets of test sites (another plan or grouping; the bitwise promises
    of a scan hold within one plan), so the scan is compared as scans are (winner and nSites equal, CLR to
    1e-9), and the refined CLR byte for byte where the search improved on both scans; A, x, alpha_beta, nSites, rounds byte for
    byte on every window.  Returns (grid CLRs that differ in bits, windows improved against one scan only)."""
    (sa, ra), (sb, rb) = full, part
    xs, ab, As = (np.asarray(v, dtype=np.float64) for v in og.GRIDS[grid])
    grids = (('A', As, 3), ('x', xs, 1), ('abeta', ab, 2))
    for q in (1, 2, 3, 4):
        assert np.array_equal(sa[q][rows], sb[q]), q
    assert np.allclose(sa[0][rows], sb[0], rtol=1e-9, atol=1e-12)
    ia, ib = _improved(sa, ra)[rows], _improved(sb, rb)
    for f in ('A', 'x', 'abeta', 'nsites', 'rounds'):
        assert ra[f][rows].tobytes() == rb[f].tobytes(), f
    both = ia & ib
    assert ra['clr'][rows][both].tobytes() == rb['clr'][both].tobytes()
    # improved against one scan only: a search that stayed on its start, whose T and the scan's product-form CLR are one number
    # in two roundings -- which of them is larger hangs on the scan's last bits
    one = ia != ib
    start = np.stack([_bits(ra[f][rows]) == _bits(g[np.maximum(sa[q][rows], 0)]) for f, g, q in grids], axis=0).all(axis=0)
    assert np.all(start[one]) and np.allclose(ra['clr'][rows][one], rb['clr'][one], rtol=1e-9, atol=1e-12)
    return int(np.sum(_bits(sa[0][rows]) != _bits(sb[0]))), int(one.sum())


def _cut(ref, q):
    done = ref['rounds'] >= 0
    return float(np.quantile(ref['clr'][done], q))


def _keys(n, seed):
    return [boot.replicate_key(seed, r, 0) for r in range(n)]


# ----------------------------------------------------------------------------- b. bit for bit
def _check_refined_bits(ctx, name, scan, ref):
    imp = _improved(scan, ref)
    A, x, a = _dummy(name, len(imp))
    A[imp], x[imp], a[imp] = ref['A'][imp], ref['x'][imp], ref['abeta'][imp]
    T, ns = ctx.eval_points(A, x, a)
    assert np.array_equal(_bits(T[imp]), _bits(ref['clr'][imp])), np.nonzero(_bits(T) != _bits(ref['clr']))[0][:8]
    assert np.array_equal(ns[imp], ref['nsites'][imp])
    return int(imp.sum())


def _check_boot_bits(ctx, name, ref, res, keys, B):
    """Per key, one batched call at the final points and one at the refined points."""
    M = len(ref['clr'])
    win = res['window']
    for r, K in enumerate(keys):
        A, x, a = _dummy(name, M)
        A[win], x[win], a[win] = res['A'][:, r], res['x'][:, r], res['abeta'][:, r]
        T, _ = ctx.eval_points_weighted(K, B, A, x, a)
        assert np.array_equal(_bits(T[win]), _bits(res['T'][:, r])), (r, np.nonzero(_bits(T[win]) != _bits(res['T'][:, r]))[0][:8])
        A[win], x[win], a[win] = ref['A'][win], ref['x'][win], ref['abeta'][win]
        T, _ = ctx.eval_points_weighted(K, B, A, x, a)
        assert np.array_equal(_bits(T[win]), _bits(res['T_centre'][:, r])), r
    return len(win) * len(keys)


@pytest.mark.parametrize('name', list(og.CASES))
def test_refined_clr_is_the_point_evaluation(name, open_ctx):
    ctx = open_ctx(name)
    scan, ref = _run(ctx, name)
    n = _check_refined_bits(ctx, name, scan, ref)
    print('%s: %d windows, %d refined, %d improved: CLR and nSites are eval_points at the reported point, bit for bit' % (name, len(scan[0]), int((ref['rounds'] >= 0).sum()), n))
    assert n >= 1


# ----------------------------------------------------------------------------- a. the existing checkers
@pytest.mark.parametrize('name', CHECKED)
def test_checkers_on_the_catalogue(name, open_ctx):
    ctx = open_ctx(name)
    pb = _problem(name)
    scan, ref = _run(ctx, name)
    imp = check_refined(ctx, pb, scan, ref, max_checks=8 if name == 'wide90831' else 24)
    none = int((scan[3] < 0).sum())
    print('%s: %d windows, %d without a grid result, %d refined, %d improved, rounds up to %d' % (name, len(imp), none, int((ref['rounds'] >= 0).sum()), int(imp.sum()), ref['rounds'].max()))
    assert imp.sum() >= 1 and none >= 1
    assert np.array_equal(ref['rounds'] >= 0, scan[3] >= 0)
    if name not in SUPPORT_BOOT:
        return
    cut = _cut(ref, 0.9)
    ctx.support(support.DROP, cut)
    sup = ctx.fetch_support()
    done = tsup.check_support(ctx, pb, scan, ref, sup, max_checks=12)
    assert np.array_equal(done.any(axis=(1, 2)), (ref['rounds'] >= 0) & (ref['clr'] >= cut))
    B = SUPPORT_BOOT[name]
    keys = _keys(3, 5)
    ctx.boot(keys, B, 0.0)
    res = ctx.fetch_boot()
    assert np.array_equal(res['window'], np.nonzero(ref['rounds'] >= 0)[0])
    tb.check_boot(pb, scan, ref, res, keys, B)
    n = _check_boot_bits(ctx, name, ref, res, keys, B)
    print('%s: support of %d windows (%d ends), boot B = %d: %d replicates, %d with T = -inf; T and T_centre are eval_points_weighted bit for bit'
          % (name, int(done.any(axis=(1, 2)).sum()), int(done.sum()), B, n, int(np.isinf(res['T']).sum())))


# ----------------------------------------------------------------------------- c, d. the replays
_EXP_WORKER = """
import sys
import numpy as np
import torch
rd, wr = sys.stdin.buffer, sys.stdout.buffer
while True:
    head = rd.read(8)
    if len(head) < 8:
        break
    n = int(np.frombuffer(head, np.int64)[0])
    v = np.frombuffer(rd.read(8 * n), np.float64).copy()
    wr.write(torch.exp(torch.from_numpy(v).to('cuda:0')).cpu().numpy().tobytes())
    wr.flush()
"""


@pytest.fixture(scope='module')
def device_exp():
    """exp of a float64 array as the GPU's device library computes it: torch on the same device, in a child process of its own
    (the library's HIP runtime and torch's do not share a process once the library's came first), started once for the module and
    ended with it.  The replay needs the device's own exp between a coordinate and its natural value: the selection table is
    ill-conditioned in alpha_beta (log-gamma differences at arguments of about alpha_beta / x: one ulp of alpha_beta moves T by up
    to 1e-12 relative at 100 and 1e-5 at 1e9, measured), the host's exp differs from the device's in the last bit at 6 % of the
    arguments, and one such difference sends a search down another path at margins far above offgrid.MARGIN_BAR."""
    import subprocess
    import sys
    p = subprocess.Popen([sys.executable, '-c', _EXP_WORKER], stdin=subprocess.PIPE, stdout=subprocess.PIPE)

    def f(v):
        v = np.ascontiguousarray(v, dtype=np.float64)
        p.stdin.write(np.int64(v.size).tobytes() + v.tobytes())
        p.stdin.flush()
        out = p.stdout.read(8 * v.size)
        assert len(out) == 8 * v.size, 'the exp worker ended (exit status %r)' % p.poll()
        return np.frombuffer(out, np.float64).copy()
    assert np.allclose(f(np.array([0.0, 1.0])), [1.0, math.e], rtol=1e-15)
    yield f
    p.stdin.close()
    p.wait(timeout=60)


def _compare(what, exact, rp, nat, dev_rounds, dev_nat, dev_T, both=None):
    """rp: offgrid.Replay; nat: its final natural values; dev_*: the device's rounds, natural values [n, 3] and T of the same
    searches; both: bool[n], the searches whose reported point is to be compared (refinement: improved on both sides).
    Returns the judged share."""
    n = len(rp.rounds)
    judged = np.ones(n, bool) if exact else rp.margin >= og.MARGIN_BAR
    cmp_ = judged if both is None else judged & both
    fin = cmp_ & np.isfinite(rp.T) & np.isfinite(dev_T)
    ulp = np.zeros((n, 3), np.int64)
    ulp[fin] = _ulps(nat[fin], dev_nat[fin])
    rel = np.zeros(n)
    rel[fin] = np.abs(rp.T[fin] - dev_T[fin]) / np.abs(dev_T[fin])
    off = ~judged
    lost = int(np.sum(off & (rp.rounds != dev_rounds)))
    print('%s: %d searches, %d judged (%.1f %%), %d exact ties, smallest judged margin %.2e; unjudged searches with other rounds than the device: %d; '
          'rounds %d .. %d; worst distance of A / x / alpha_beta %r ulp, worst relative dT %.2e, %d ends at -inf'
          % (what, n, int(judged.sum()), 100.0 * judged.mean(), int((rp.margin == 0).sum()), rp.margin[judged].min() if judged.any() else math.nan, lost,
             dev_rounds.min(), dev_rounds.max(), ulp.max(axis=0).tolist(), rel.max(), int(np.isinf(dev_T).sum())))
    assert np.array_equal(rp.rounds[judged], dev_rounds[judged]), (what, np.nonzero(judged & (rp.rounds != dev_rounds))[0][:8])
    assert np.array_equal(np.isfinite(rp.T[cmp_]), np.isfinite(dev_T[cmp_])), what
    assert np.array_equal(_bits(nat[cmp_, 1]), _bits(dev_nat[cmp_, 1])), (what, 'x')
    if exact:
        assert np.array_equal(_bits(nat[cmp_]), _bits(dev_nat[cmp_])) and np.array_equal(_bits(rp.T[cmp_]), _bits(dev_T[cmp_])), what
    else:
        assert np.all(np.abs(nat[fin] - dev_nat[fin]) <= 4 * np.spacing(np.abs(dev_nat[fin]))), (what, ulp.max(axis=0))
        assert np.all(rel <= 1e-12), (what, rel.max())
    assert judged.mean() >= og.JUDGED_SHARE, (what, judged.mean())
    return judged


@pytest.mark.parametrize('name', og.REPLAYED)
def test_refine_kernel_takes_the_replays_path(name, open_ctx, device_exp):
    ctx = open_ctx(name)
    c = og.CASES[name]
    xs, ab, As = og.GRIDS[c.grid]
    st = og.setup_of(c.grid)
    scan, ref = _run(ctx, name)
    clr, ix, ia, iA, ns = scan
    M = len(clr)
    has = np.nonzero(iA >= 0)[0]
    assert np.array_equal(ref['rounds'] >= 0, iA >= 0) and len(has) >= 40
    s = [st.start(As[iA[j]], xs[ix[j]], ab[ia[j]]) for j in has]
    c0, nat0, h0 = (np.array([v[q] for v in s]) for q in range(3))
    calls = [0]

    def point(nat, act):
        A, x, a = _dummy(name, M)
        A[has[act]], x[has[act]], a[has[act]] = nat[act, 0], nat[act, 1], nat[act, 2]
        return A, x, a

    def eval_batch(p, act):
        calls[0] += 1
        return ctx.eval_points(*point(og.naturals(p, c0, nat0, device_exp), act))[0][has]
    rp = og.replay(eval_batch, c0, st.free, st.lo, st.hi, h0, refine.TOL, 256)
    nat = og.naturals(rp.c, c0, nat0, device_exp)
    exact = c.grid == 'x'
    imp_dev = _improved(scan, ref)[has]
    imp_rp = rp.T > clr[has]
    dev_nat = np.stack([ref['A'], ref['x'], ref['abeta']], axis=1)[has]
    print('%s: %d eval_points calls of %d points; improved on the device %d, in the replay %d' % (name, calls[0], M, int(imp_dev.sum()), int(imp_rp.sum())))
    judged = _compare(name, exact, rp, nat, ref['rounds'][has], dev_nat, ref['clr'][has], both=imp_dev & imp_rp)
    assert np.array_equal(imp_dev[judged], imp_rp[judged]), np.nonzero(judged & (imp_dev != imp_rp))[0][:8]
    if exact:
        ns_rp = ctx.eval_points(*point(nat, imp_rp))[1][has]
        assert np.array_equal(ns_rp[imp_rp], ref['nsites'][has][imp_rp])
        assert np.array_equal(_bits(rp.T0), _bits(ctx.eval_points(*point(nat0, np.ones(len(has), bool)))[0][has]))
    assert imp_dev.sum() >= 1


def _zero_block_keys(name, B, count, seed=7, need=3):
    """The first `count` keys of `seed` under which at least `need` non-empty windows of the case lie wholly in blocks of weight
    0 (whatever A: every site of the window has weight 0, so T_w is -inf at every point)."""
    tg, idx, lo, hi, _ = og.tests_of(name)
    N = len(og.dataset(og.CASES[name].data).gen)
    keys = []
    for r in range(1000):
        K = boot.replicate_key(seed, r, 0)
        w = np.concatenate(([0], np.cumsum(boot.site_weights(K, N, B))))
        ok = lo <= hi
        if int(np.sum(ok & (w[np.minimum(hi, N - 1) + 1] - w[np.minimum(lo, N - 1)] == 0))) >= need:
            keys.append(K)
            if len(keys) == count:
                return keys
    raise AssertionError('no such keys')


@pytest.mark.parametrize('B', (1, 64))
@pytest.mark.parametrize('name', ('small-all-ragged', 'small-corner-ragged'))
def test_boot_kernel_takes_the_replays_path(name, B, open_ctx, device_exp):
    ctx = open_ctx(name)
    c = og.CASES[name]
    xs, ab, As = og.GRIDS[c.grid]
    st = og.setup_of(c.grid)
    scan, ref = _run(ctx, name)
    clr, ix, ia, iA, ns = scan
    M = len(clr)
    keys = _zero_block_keys(name, B, 2) if B == 64 else _keys(2, 9)
    ctx.boot(keys, B, 0.0)
    res = ctx.fetch_boot()
    win = res['window']
    assert np.array_equal(win, np.nonzero(iA >= 0)[0]) and len(win) >= 40
    s = [support.centre(st, (As[iA[j]], xs[ix[j]], ab[ia[j]]), (ref['A'][j], ref['x'][j], ref['abeta'][j])) for j in win]
    c0, nat0, h0 = (np.array([v[q] for v in s]) for q in range(3))
    lost = 0
    for r, K in enumerate(keys):
        def eval_batch(p, act):
            nat = og.naturals(p, c0, nat0, device_exp)
            A, x, a = _dummy(name, M)
            A[win[act]], x[win[act]], a[win[act]] = nat[act, 0], nat[act, 1], nat[act, 2]
            return ctx.eval_points_weighted(K, B, A, x, a)[0][win]
        rp = og.replay(eval_batch, c0, st.free, st.lo, st.hi, h0, refine.TOL, 256)
        nat = og.naturals(rp.c, c0, nat0, device_exp)
        dev_nat = np.stack([res['A'][:, r], res['x'][:, r], res['abeta'][:, r]], axis=1)
        _compare('%s B = %d key %d' % (name, B, r), False, rp, nat, res['rounds'][:, r], dev_nat, res['T'][:, r])
        assert np.array_equal(_bits(rp.T0), _bits(res['T_centre'][:, r]))          # the centre is the refined point itself: no exp
        lost += int(np.isinf(res['T_centre'][:, r]).sum())
    n = _check_boot_bits(ctx, name, ref, res, keys, B)
    print('%s B = %d: %d replicates, %d with a centre at -inf, %d of them still at -inf at the end' % (name, B, n, lost, int(np.isinf(res['T']).sum())))
    if B == 64:
        assert lost >= 1


# ----------------------------------------------------------------------------- e. weighted point evaluation around the stride
def test_weighted_points_at_block_sizes_around_the_stride(open_ctx):
    """test_gpu_boot.check_weighted_points' comparison (Host.Tw at 1e-9, the weight sums exactly) at block sizes on either side of
    the 256 sites a workgroup advances by: boot_kernel carries i / B and i % B along that stride."""
    name = 'small-all-ragged'
    ctx = open_ctx(name)
    pb = _problem(name)
    tg, lo, hi = _windows(name)
    ctx.set_tests(tg, lo, hi)
    M, N = len(tg), len(pb.genpos)
    host = tb.Host(pb)
    A, x, a = tb._points(pb, M, 13)
    for B in (1, 3, 7, 64, 255, 256, 257, 1000, N + 5):
        K = boot.replicate_key(3, B % 5, 1)
        w = boot.site_weights(K, N, B)
        T, ws = ctx.eval_points_weighted(K, B, A, x, a)
        hits, worst = 0, 0.0
        for j in range(M):
            want, wsum = host.Tw(j, w, A[j], x[j], a[j])
            assert ws[j] == wsum, (B, j, ws[j], wsum)
            assert tb._close(T[j], want, 1e-9), (B, j, T[j], want)
            if math.isfinite(want):
                hits += 1
                worst = max(worst, abs(T[j] - want) / abs(want))
        print('eval_points_weighted B = %d: %d windows, %d finite, worst relative difference to the host %.2e, weight sums equal' % (B, M, hits, worst))
        assert hits >= M // 3


# ----------------------------------------------------------------------------- f. the workspace
def test_either_side_of_the_lds_edge(open_ctx):
    """728 rows (workspace in LDS) and 729 rows (in the slab): the same sites, windows, g and prop, so the same expression for every
    table entry a site reaches -- every result is equal."""
    a = _run(open_ctx('wide728'), 'wide728')
    b = _run(open_ctx('wide729'), 'wide729')
    d = [k for k in a[1] if a[1][k].tobytes() != b[1][k].tobytes()]
    print('wide728 against wide729: %d windows, %d refined, %d improved; fields that differ: %r' % (len(a[0][0]), int((a[1]['rounds'] >= 0).sum()), int(_improved(*a).sum()), d))
    assert all(np.array_equal(u, v) for u, v in zip(a[0][1:], b[0][1:])) and np.array_equal(_bits(a[0][0]), _bits(b[0][0]))
    assert _same_bytes(a[1], b[1])
    assert _improved(*a).sum() >= 20


def test_slices_of_the_capped_slab(open_ctx):
    """90 831 rows: at most 131 workgroups, so in the full run of 300 windows a workgroup takes a second and a third window with the
    first one's map, row list, tables and state in its slab; slices of 100 windows give every window a fresh workgroup."""
    name = 'wide90831'
    ctx = open_ctx(name)
    scan, ref = _run(ctx, name)
    assert (ref['rounds'] >= 0).sum() > 131
    xs, ab, As = og.GRIDS['wideA']
    point = (As[0], xs[1], ab[1])                                 # ONE point for every window: a second window finds its tables built
    T, ns = ctx.eval_points(*point)
    assert np.isfinite(T).sum() >= 250
    moved = np.zeros(2, np.int64)
    for k in range(3):
        rows = slice(100 * k, 100 * (k + 1))
        s, r = _run(ctx, name, rows)
        Tk, nsk = ctx.eval_points(*point)
        assert T[rows].tobytes() == Tk.tobytes() and np.array_equal(ns[rows], nsk), (k, np.nonzero(_bits(T[rows]) != _bits(Tk))[0][:8])
        moved += np.array(_same_search((scan, ref), (s, r), rows, 'wideA'))
    print('%s: %d windows, %d refined by at most 131 workgroups; three slices of 100 reproduce them byte for byte (%d grid CLRs differ in their last bits between the two scans, %d searches that stayed on their start count as improved against one scan only)' % (name, len(scan[0]), int((ref['rounds'] >= 0).sum()), moved[0], moved[1]))


def test_halves_of_a_striding_launch(open_ctx):
    """4 003 windows, more than the 2 048 workgroups of a launch: the full run against its two halves (slots of their own, at most
    2 002 windows each), for the refinement, point evaluation at one common point, the bootstrap (one key at the top 10 %, and ten
    keys for more tasks than workgroups) and the support intervals (top 2 %)."""
    name = 'stride'
    ctx = open_ctx(name)
    d = og.dataset('small')
    rows = _model('small', 'all')[1]
    M = len(og.tests_of(name)[0])
    half = (slice(0, (M + 1) // 2), slice((M + 1) // 2, M))

    def everything(sl, cut10, cut2):
        scan, ref = _run(ctx, name, sl)
        xs, ab, As = og.GRIDS['all']
        T, ns = ctx.eval_points(As[1], xs[2], ab[6])              # ONE point for every window: a second window finds its tables built
        out = {'ref': ref, 'point': {'T': T, 'ns': ns}}
        for tag, keys in (('boot1', _keys(1, 11)), ('boot10', _keys(10, 11))):
            ctx.boot(keys, 16, cut10 if cut10 is not None else _cut(ref, 0.9))
            out[tag] = ctx.fetch_boot()
        ctx.support(support.DROP, cut2 if cut2 is not None else _cut(ref, 0.98))
        out['support'] = ctx.fetch_support()
        return scan, out
    try:
        ctx.select_slot(0)
        scan, full = everything(slice(None), None, None)
        ref = full['ref']
        cut10, cut2 = _cut(ref, 0.9), _cut(ref, 0.98)
        n_ref, n_boot, n_sup = int((ref['rounds'] >= 0).sum()), len(full['boot10']['window']) * 10, int((full['support']['rounds'] >= 0).sum())
        print('stride: %d windows, %d refined, %d bootstrap tasks at 10 keys, %d support tasks' % (M, n_ref, n_boot, n_sup))
        assert n_ref > 2048 and n_boot > 2048 and n_sup >= 100
        _check_refined_bits(ctx, name, scan, ref)
        for k, sl in enumerate(half):
            ctx.select_slot(1 + k)
            ctx.set_sites(d.gen, rows)
            s, part = everything(sl, cut10, cut2)
            print('stride, half %d: (grid CLRs that differ in bits, windows improved against one scan only) = %r' % (k, _same_search((scan, ref), (s, part['ref']), sl, 'all')))
            assert _same_bytes(full['point'], part['point'], sl), k
            sup = {f: v for f, v in full['support'].items() if f not in ('lo', 'hi')}
            assert _same_bytes(sup, {f: part['support'][f] for f in sup}, sl), k
            for tag in ('boot1', 'boot10'):
                fw = full[tag]['window']
                at = (fw >= sl.start) & (fw < sl.stop)
                assert np.array_equal(fw[at] - sl.start, part[tag]['window']) and at.sum() >= 50, (k, tag)
                for f in ('A', 'x', 'abeta', 'T', 'T_centre', 'rounds'):
                    assert full[tag][f][at].tobytes() == part[tag][f].tobytes(), (k, tag, f)
    finally:
        ctx.select_slot(0)
