"""Block bootstrap on the GPU (--boot): weighted point evaluation against the host restatement of T_w (the C oracle's selection
table, boot.py's weights), replicates against it at the reported point, at the centre and at the compass neighbours,
determinism and independence of tasks, a planted parameter, call order and limits, and the CLI (nothing else it writes changes)."""
import math
import os

import numpy as np
import pytest

import cases
from test_gpu_refine import (REPO, Problem, _bits, _case_ctx, _cli, _engine, _last_steps, _problem_of_case, _read, _scan_refine,
                             _synth)
from util import REFT

from ballermixplus_amd import boot, refine, support
from ballermixplus_amd._lib import BmxError

pytestmark = pytest.mark.gpu

EXAMPLES = [('ex1_B2', 31), ('ex2_B2maf', 47), ('ex1_B1', 31), ('ex2_B0maf_1kb', 6)]


class Host:
    """T_w of a Problem's test sites on the host: the C oracle's R, the window predicate of the oracle, boot.py's weights."""

    def __init__(self, pb):
        self.pb = pb
        self.cache = {}
        self.idx = np.arange(len(pb.genpos))

    def terms(self, j, A, x, a):
        pb = self.pb
        if (x, a) not in self.cache:
            self.cache[(x, a)] = pb.R(x, a)[0, 0]
        d = np.abs(pb.genpos - pb.tg[j])
        al = np.exp(-A * d)
        keep = (al >= 1e-8) & (pb.genpos != pb.tg[j]) & (self.idx >= pb.lo[j]) & (self.idx <= pb.hi[j])
        sub = np.nonzero(keep)[0]
        return sub, al[sub], self.cache[(x, a)][pb.rows[sub]]

    def Tw(self, j, w, A, x, a):
        sub, al, R = self.terms(j, A, x, a)
        return boot.weighted_T(al, R, w[sub]), int(w[sub].sum())


def _close(got, want, tol):
    if not math.isfinite(want):
        return got == want
    return abs(got - want) <= tol * abs(want)


def _points(pb, M, seed):
    """Half grid points, half random off-grid points inside the hull."""
    rng = np.random.default_rng(seed)
    st = pb.setup
    A = np.asarray(pb.As)[rng.integers(0, len(pb.As), M)].astype(np.float64)
    x = np.asarray(pb.xs)[rng.integers(0, len(pb.xs), M)].astype(np.float64)
    a = np.asarray(pb.abetas)[rng.integers(0, len(pb.abetas), M)].astype(np.float64)
    off = np.arange(M) % 2 == 1
    # off the grid: A where windows hold some sites, moderate alpha_beta
    A[off] = np.exp(rng.uniform(max(st.lo[0], math.log(200.0)), min(st.hi[0], math.log(2e4)), off.sum())) if st.free[0] else A[off]
    x[off] = rng.uniform(st.lo[1], st.hi[1], off.sum()) if st.free[1] else x[off]
    a[off] = np.exp(rng.uniform(max(st.lo[2], math.log(0.5)), min(st.hi[2], math.log(500.0)), off.sum())) if st.free[2] else a[off]
    return A, x, a


def _single_weight_keys():
    """The first keys of seed 1 whose weight of block 0 is > 0 and is 0."""
    pos = zero = None
    for r in range(1000):
        K = boot.replicate_key(1, r, 0)
        w = int(boot.block_weights(K, 1)[0])
        if w > 0 and pos is None:
            pos = (K, w)
        if w == 0 and zero is None:
            zero = K
        if pos and zero is not None:
            return pos, zero
    raise AssertionError('no such keys')


def check_weighted_points(ctx, pb, seed):
    M, N = len(pb.tg), len(pb.genpos)
    host = Host(pb)
    A, x, a = _points(pb, M, seed)
    hits = 0
    for B in (1, 7, 64, N + 5):
        K = boot.replicate_key(3, B % 5, 1)
        w = boot.site_weights(K, N, B)
        T, ws = ctx.eval_points_weighted(K, B, A, x, a)
        for j in range(M):
            want, wsum = host.Tw(j, w, A[j], x[j], a[j])
            print('eval_points_weighted B=%d j=%d device %r host %r wsum %d/%d' % (B, j, T[j], want, ws[j], wsum))
            assert ws[j] == wsum, (B, j)
            assert _close(T[j], want, 1e-9), (B, j, T[j], want)
            hits += math.isfinite(want)
    assert hits >= M
    (K1, w0), K0 = _single_weight_keys()
    T0, _ = ctx.eval_points(A, x, a)
    T1, ws1 = ctx.eval_points_weighted(K1, N + 5, A, x, a)
    Tz, wsz = ctx.eval_points_weighted(K0, N + 5, A, x, a)
    assert np.all(Tz == -np.inf) and np.all(wsz == 0)
    for j in range(M):
        print('single weight %d: j=%d %r vs %r' % (w0, j, T1[j], w0 * T0[j]))
        assert _close(T1[j], w0 * T0[j], 1e-12), (j, T1[j], T0[j], w0)
    assert np.isfinite(T1).sum() > 0
    # every site at weight 1: the weighted round is the unweighted round, bit for bit, and the weight sum is nSites
    Ku = boot.replicate_key(1, 0, 0)
    assert int(boot.block_weights(Ku, 1)[0]) == 1
    Tu, nsu = ctx.eval_points(A, x, a)
    Tw, wsw = ctx.eval_points_weighted(Ku, N + 5, A, x, a)
    print('unit weight: %d points, %d finite, %d differ in bits' % (M, int(np.isfinite(Tu).sum()), int((_bits(Tw) != _bits(Tu)).sum())))
    assert np.array_equal(_bits(Tw), _bits(Tu)) and np.array_equal(wsw, nsu)


# ---------------------------------------------------------------------------------------------------- weighted point evaluation

@pytest.mark.parametrize('name,step', EXAMPLES)
def test_eval_points_weighted_reference_examples(name, step):
    opt, case, ts, sel = _case_ctx(cases.ALL_CASES[name][0])
    tg, lo, hi = ts.test_gen[::step], ts.lo[::step], ts.hi[::step]
    sel.ctx.set_tests(tg, lo, hi)
    pb = _problem_of_case(case, ts, sel)
    pb.tg, pb.lo, pb.hi = np.asarray(tg), np.asarray(lo), np.asarray(hi)
    check_weighted_points(sel.ctx, pb, 7)
    sel.ctx.close()


def test_eval_points_weighted_table_in_l2():
    ctx, gen, rows, (st, mc, sizes, spect, props, As, xs, ab) = _synth(20000, spread=30)
    tg = gen[::1250]
    lo = np.zeros(len(tg), dtype=np.int64)
    hi = np.full(len(tg), len(gen) - 1, dtype=np.int64)
    ctx.set_tests(tg, lo, hi)
    check_weighted_points(ctx, Problem(st, mc, sizes, spect, props, gen, rows, As, xs, ab, tg, lo, hi), 9)
    ctx.close()


# ---------------------------------------------------------------------------------------------------- replicates

def check_boot(pb, scan, ref, res, keys, B, max_checks=24):
    """Every (window, replicate): T >= T_centre, inside the hull, fixed coordinates kept.  A sample of them (the first and the
    last window, replicates 0 and R - 1 among them): the host's T_w at the reported point and at the centre, and no better
    compass neighbour at the last steps."""
    clr, ix, ia, iA, ns = scan
    st = pb.setup
    n, R = res['T'].shape
    assert n > 0 and R == len(keys)
    sel = (ref['rounds'] >= 0)
    assert np.array_equal(res['window'], np.nonzero(sel)[0].astype(np.int32)[:n]) or n <= sel.sum()
    assert np.all(res['T'] >= res['T_centre'])
    assert np.all(res['rounds'] >= 0)
    for k, key in enumerate(('A', 'x', 'abeta')):
        c = np.array([refine.to_coord(k, v) for v in res[key].ravel()])
        assert np.all(c >= st.lo[k] - 1e-12 * abs(st.lo[k])) and np.all(c <= st.hi[k] + 1e-12 * abs(st.hi[k])), key
        if not st.free[k]:
            assert np.array_equal(_bits(res[key]), _bits(np.repeat(ref[key][res['window']], R).reshape(n, R))), key
    host = Host(pb)
    N = len(pb.genpos)
    W = [boot.site_weights(K, N, B) for K in keys]
    pairs = [(0, 0), (0, R - 1), (n - 1, 0), (n - 1, R - 1)]
    rng = np.random.default_rng(1)
    while len(pairs) < min(max_checks, n * R):
        p = (int(rng.integers(0, n)), int(rng.integers(0, R)))
        if p not in pairs:
            pairs.append(p)
    for q, r in pairs:
        j = int(res['window'][q])
        A, x, a = res['A'][q, r], res['x'][q, r], res['abeta'][q, r]
        T, _ = host.Tw(j, W[r], A, x, a)
        Tc, _ = host.Tw(j, W[r], ref['A'][j], ref['x'][j], ref['abeta'][j])
        print('boot window %d rep %d: T %r host %r  T_centre %r host %r  rounds %d' % (j, r, res['T'][q, r], T, res['T_centre'][q, r],
                                                                                    Tc, res['rounds'][q, r]))
        assert _close(res['T'][q, r], T, 1e-9), (j, r, res['T'][q, r], T)
        assert _close(res['T_centre'][q, r], Tc, 1e-9), (j, r, res['T_centre'][q, r], Tc)
        if res['rounds'][q, r] >= refine.MAX_ROUNDS or not math.isfinite(T):
            continue
        grid = (pb.As[iA[j]], pb.xs[ix[j]], pb.abetas[ia[j]])
        c0, nat0, h0 = support.centre(st, grid, (ref['A'][j], ref['x'][j], ref['abeta'][j]))
        h = _last_steps(h0, st.free)
        c = tuple(c0[k] if v == nat0[k] else refine.to_coord(k, v) for k, v in enumerate((A, x, a)))
        for d in range(6):
            k = d // 2
            if not st.free[k]:
                continue
            v = min(max(c[k] + h[k] if d & 1 else c[k] - h[k], st.lo[k]), st.hi[k])
            if v == c[k]:
                continue
            nb = list(c)
            nb[k] = v
            Tn, _ = host.Tw(j, W[r], *refine.natural_of(tuple(nb), c0, nat0))
            assert Tn <= res['T'][q, r] + 1e-9 * abs(res['T'][q, r]), (j, r, d, Tn, res['T'][q, r])


def _keys(R, seed=1, f=0):
    return [boot.replicate_key(seed, r, f) for r in range(R)]


@pytest.mark.parametrize('name,step', [('ex1_B2', 7), ('ex2_B2maf', 9), ('ex1_B1', 7), ('ex2_B0maf_1kb', 1)])
def test_boot_reference_examples(name, step):
    opt, case, ts, sel = _case_ctx(cases.ALL_CASES[name][0])
    tg, lo, hi = ts.test_gen[::step], ts.lo[::step], ts.hi[::step]
    scan, ref = _scan_refine(sel.ctx, tg, lo, hi)
    pb = _problem_of_case(case, ts, sel)
    pb.tg, pb.lo, pb.hi = np.asarray(tg), np.asarray(lo), np.asarray(hi)
    keys = _keys(8)
    sel.ctx.boot(keys, 16, 0.0)
    res = sel.ctx.fetch_boot()
    assert np.array_equal(res['window'], np.nonzero(ref['rounds'] >= 0)[0])
    check_boot(pb, scan, ref, res, keys, 16)
    sel.ctx.close()


@pytest.mark.parametrize('stat,spread,step', [('B2', 30, 16), ('B0', 0, 1), ('B0maf', 0, 16), ('B2maf', 0, 4)])
def test_boot_synthetic_plans(stat, spread, step):
    ctx, gen, rows, (st, mc, sizes, spect, props, As, xs, ab) = _synth(20000, stat=stat, spread=spread)
    tg = gen[::step][:2000]
    lo = np.zeros(len(tg), dtype=np.int64)
    hi = np.full(len(tg), len(gen) - 1, dtype=np.int64)
    scan, ref = _scan_refine(ctx, tg, lo, hi)
    cut = float(np.quantile(ref['clr'][ref['rounds'] >= 0], 0.9))
    keys = _keys(8, seed=2)
    ctx.boot(keys, 1, cut)
    res = ctx.fetch_boot()
    assert np.array_equal(res['window'], np.nonzero((ref['rounds'] >= 0) & (ref['clr'] >= cut))[0])
    check_boot(Problem(st, mc, sizes, spect, props, gen, rows, As, xs, ab, tg, lo, hi), scan, ref, res, keys, 1, max_checks=8)
    ctx.close()


def test_boot_keeps_fixed_coordinates():
    argv = cases.ALL_CASES['ex2_B2'][0] + ['--fixX', '0.3', '--listA', '2500', '--findBal', '-s', '10']
    opt, case, ts, sel = _case_ctx(argv)
    scan, ref = _scan_refine(sel.ctx, ts.test_gen, ts.lo, ts.hi)
    sel.ctx.boot(_keys(8), 4, 0.0)
    res = sel.ctx.fetch_boot()
    assert res['T'].shape[0] > 0
    assert np.all(_bits(res['x']) == _bits(np.full(res['x'].shape, 0.3)))
    assert np.all(_bits(res['A']) == _bits(np.full(res['A'].shape, 2500.0)))
    assert np.all(res['abeta'] >= 1.0) and len(np.unique(res['abeta'])) > 1
    sel.ctx.close()


# ---------------------------------------------------------------------------------------------------- determinism, independence

def _same(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a) and sorted(a) == sorted(b)


def test_determinism_subset_single_replicate_and_profiles():
    opt, case, ts, sel = _case_ctx(cases.ALL_CASES['ex2_B2maf'][0])
    ctx = sel.ctx
    tg, lo, hi = ts.test_gen[::3], ts.lo[::3], ts.hi[::3]
    scan, ref = _scan_refine(ctx, tg, lo, hi)
    keys = _keys(8)
    ctx.boot(keys, 7, 0.0)
    a = ctx.fetch_boot()
    ctx.boot(keys, 7, 0.0)
    assert _same(a, ctx.fetch_boot())
    cut = float(np.quantile(ref['clr'][ref['rounds'] >= 0], 0.8))
    ctx.boot(keys, 7, cut)
    c = ctx.fetch_boot()
    assert 0 < len(c['window']) < len(a['window']) and np.all(ref['clr'][c['window']] >= cut)
    at = np.searchsorted(a['window'], c['window'])
    assert np.array_equal(a['window'][at], c['window'])
    for k in ('A', 'x', 'abeta', 'T', 'T_centre', 'rounds'):
        assert a[k][at].tobytes() == c[k].tobytes(), k
    for r in (0, 5, 7):
        ctx.boot([keys[r]], 7, 0.0)
        one = ctx.fetch_boot()
        assert one['T'].shape == (len(a['window']), 1)
        for k in ('A', 'x', 'abeta', 'T', 'T_centre', 'rounds'):
            assert np.ascontiguousarray(a[k][:, r]).tobytes() == one[k][:, 0].tobytes(), (k, r)
    assert len({a['T'][:, r].tobytes() for r in range(8)}) == 8        # the replicates differ
    ctx.set_profiles(7)
    _scan_refine(ctx, tg, lo, hi)
    ctx.boot(keys, 7, 0.0)
    assert _same(a, ctx.fetch_boot())
    ctx.close()


def test_call_order_and_limits():
    opt, case, ts, sel = _case_ctx(cases.ALL_CASES['ex1_B2'][0] + ['-s', '20'])
    ctx = sel.ctx
    ctx.set_tests(ts.test_gen, ts.lo, ts.hi)
    ctx.scan()
    with pytest.raises(BmxError) as e:
        ctx.boot(_keys(4), 1, 0.0)                # no refinement yet
    assert e.value.code == -5
    ctx.refine(0.0)
    n = int((ctx.fetch_refined()['rounds'] >= 0).sum())
    for keys, B in (([], 1), (_keys(4), 0)):
        with pytest.raises(BmxError) as e:
            ctx.boot(keys, B, 0.0)
        assert e.value.code == -1
    with pytest.raises(BmxError) as e:
        ctx.eval_points_weighted(1, 0, 1000.0, 0.3, 5.0)
    assert e.value.code == -1
    with pytest.raises(BmxError) as e:
        ctx.boot([1] * ((1 << 26) // n + 1), 1, 0.0)
    assert e.value.code == -4 and '--bootMin' in str(e.value)
    ctx.boot(_keys(2), 1, 0.0)
    assert ctx.fetch_boot()['T'].shape == (n, 2)
    ctx.boot(_keys(2), 1, 1e300)                   # nothing selected
    assert ctx.fetch_boot()['T'].shape == (0, 2)
    ctx.boot(_keys(2), 1, 0.0)
    ctx.scan()                                     # a new scan drops the results
    with pytest.raises(BmxError) as e:
        ctx.fetch_boot()
    assert e.value.code == -5
    ctx.close()


# ---------------------------------------------------------------------------------------------------- a planted parameter

def test_planted_parameter_moves_with_the_data():
    """tests/test_gpu_refine.py's planted data (x = 0.27 around one centre).  With 64 replicates the x_hat values differ and
    stay in the hull.  Whether the percentile interval holds the refined x_hat is printed, not asserted: a percentile interval
    need not contain its centre, and the seed was not chosen for it."""
    eng = _engine()
    from ballermixplus_amd.hostmodel import Grids
    from ballermixplus_amd import synth
    rng = np.random.default_rng(11)
    n, N, x0, a0, A0 = 100, 6000, 0.27, 40.0, 2000.0
    gen = np.cumsum(rng.uniform(0.5e-6, 1.5e-6, N))
    centre = gen[N // 2]
    ks = np.arange(1, n)
    w = 1.0 / ks
    k = rng.choice(ks, size=N, p=w / w.sum())
    k = np.where(rng.random(N) < 0.3, n, k)
    sel_p = np.exp(-A0 * np.abs(gen - centre))
    chosen = rng.random(N) < sel_p
    xx = np.where(rng.random(N) < 0.5, x0, 1 - x0)
    p = rng.beta(a0, a0 / xx - a0)
    kb = rng.binomial(n, p)
    k = np.where(chosen, kb, k)
    keep = k > 0
    gen, k = gen[keep], k[keep]
    nn = np.full(len(k), n)
    neutral = ~chosen[keep]
    spect = {(a, b): f for a, b, f in synth.spect_from_counts(k[neutral], nn[neutral])}
    for kk in set(k.tolist()):
        spect.setdefault((kk, n), 0.5 / len(k))
    xs, ab, As = Grids(None, None, False, False, None, None).scan_order()
    model = eng.ModelArrays('B2', 1, [n], spect, {n: 1.0}, xs, ab)
    ctx = eng.Context(0)
    ctx.set_model(model, As)
    ctx.set_sites(gen, model.rows_of(k, nn))
    scan, ref = _scan_refine(ctx, np.array([centre]), None, None)
    ctx.boot(_keys(64), 16, 0.0)
    res = ctx.fetch_boot()
    assert res['T'].shape == (1, 64) and np.all(np.isfinite(res['T']))
    xh = res['x'][0]
    assert len(np.unique(xh)) > 1
    assert np.all(xh >= min(xs)) and np.all(xh <= max(xs))
    s = boot.summarise(res['A'][0], xh, res['abeta'][0], res['T'][0], res['T_centre'][0], (True, True, True), 0.95)
    print('planted x = %r: refined x_hat %r, bootstrap x_lo %r x_hi %r x_sd %r dT_q %r; interval holds x_hat: %r, holds the planted '
          'x: %r' % (x0, ref['x'][0], s['lo'][1], s['hi'][1], s['sd'][1], s['dT_q'], s['lo'][1] <= ref['x'][0] <= s['hi'][1],
                     s['lo'][1] <= x0 <= s['hi'][1]))
    ctx.close()


# ---------------------------------------------------------------------------------------------------- CLI

def _rows(path):
    with open(path) as f:
        return [l.rstrip('\n').split('\t') for l in f]


def _check_boot_file(main, outfile, level, min_clr, free=(True, True, True)):
    m, b, r = _rows(main), _rows(boot.output_name(outfile)), _rows(refine.output_name(outfile))
    assert '\t'.join(b[0]) + '\n' == boot.HEADER and len(b) == len(m)
    reps = boot.read_reps(boot.reps_name(outfile))
    done = 0
    for lm, lb, lr in zip(m[1:], b[1:], r[1:]):
        assert lb[:2] == lm[:2] and len(lb) == 14
        na = lm[5] == 'NA' or lm[3:] == ['0.0'] * 4 or float(lr[2]) < min_clr
        assert (lb[2:] == ['NA'] * 12) == na, (lm, lb)
        if na:
            assert (lb[0], lb[1]) not in reps
            continue
        done += 1
        assert lb[2] == repr(float(lr[2]))
        v = reps[(lb[0], lb[1])]
        s = boot.summarise(v['A'], v['x'], v['abeta'], v['T'], None, free, level)
        want = boot.format_row(lb[:2], float(lr[2]), s).rstrip('\n').split('\t')
        assert lb[:12] == want[:12] and lb[13] == want[13], (lb, want)      # (dT_q needs T at the centre, which the file lacks)
        assert float(lb[12]) >= 0
    assert len(reps) == done
    return done


def test_cli_boot_leaves_everything_else(tmp_path):
    base = ['-i', os.path.join(REFT, 'Example2_balancing_10MYA_DAF.txt'), '--spect', os.path.join(REFT, 'HC_CEU_Neut_DAF_spect_for_B2.txt'),
            '-s', '5']
    extra = ['--refine', '--support', '--profiles', 'A,x,abeta', '--nullPerm', '3']
    plain, full, top = (str(tmp_path / n) for n in ('plain.txt', 'full.txt', 'top.txt'))
    _cli(base + ['-o', plain] + extra)
    _cli(base + ['-o', full] + extra + ['--boot', '8', '--bootBlock', '16', '--bootReps'])
    for ext in ('', '.refined.txt', '.support.txt', '.profile_A.txt', '.profile_x.txt', '.profile_abeta.txt', '.null.txt', '.pval.txt'):
        assert _read(plain + ext) == _read(full + ext), ext
    assert sorted(os.listdir(tmp_path)) == sorted(os.path.basename(p) + e for p, es in (
        (plain, ('', '.refined.txt', '.support.txt', '.profile_A.txt', '.profile_x.txt', '.profile_abeta.txt', '.null.txt', '.pval.txt')),
        (full, ('', '.refined.txt', '.support.txt', '.profile_A.txt', '.profile_x.txt', '.profile_abeta.txt', '.null.txt', '.pval.txt',
                '.boot.txt', '.boot.reps.txt'))) for e in es)
    assert _check_boot_file(full, full, 0.95, 0.0) > 10
    cut = sorted(float(l[2]) for l in _rows(refine.output_name(full))[1:] if l[5] != 'NA')[-20]
    _cli(base + ['-o', top, '--refine', '--boot', '8', '--bootBlock', '16', '--bootReps', '--bootMin', repr(cut), '--bootLevel', '0.5'])
    assert not os.path.exists(support.output_name(top))
    assert _check_boot_file(top, top, 0.5, cut) == 20
    # the same windows, the same replicates: a replicate does not depend on the other windows
    a, b = boot.read_reps(boot.reps_name(full)), boot.read_reps(boot.reps_name(top))
    for head, v in b.items():
        assert all(np.array_equal(v[k], a[head][k]) for k in v), head


def test_cli_boot_three_files(tmp_path):
    spect = os.path.join(REFT, 'HC_CEU_Neut_DAF_spect_for_B2.txt')
    third = tmp_path / 'Example3_copy_of_1.txt'
    third.write_bytes(_read(os.path.join(REFT, 'Example1_fullSweep_200kya_DAF.txt')))
    ins = [os.path.join(REFT, 'Example1_fullSweep_200kya_DAF.txt'), os.path.join(REFT, 'Example2_balancing_10MYA_DAF.txt'),
           str(third)]
    lst = tmp_path / 'inputs.txt'
    lst.write_text('\n'.join(ins) + '\n')
    d1, d2 = tmp_path / 'plain', tmp_path / 'boot'
    d1.mkdir()
    d2.mkdir()
    _cli(['--inputs', str(lst), '--spect', spect, '-o', str(d1), '-s', '9', '--refine'])
    _cli(['--inputs', str(lst), '--spect', spect, '-o', str(d2), '-s', '9', '--refine', '--boot', '4', '--bootReps', '--bootSeed', '5'])
    outs = sorted(os.listdir(d1))
    assert outs and sorted(f for f in os.listdir(d2) if '.boot.' not in f) == outs
    mains = [f for f in outs if not f.endswith('.refined.txt')]
    assert len(mains) == 3
    for f in outs:
        assert _read(d1 / f) == _read(d2 / f)
    for f in mains:
        assert _check_boot_file(str(d2 / f), str(d2 / f), 0.95, 0.0) > 5
    # files 0 and 2 hold the same data: the same windows, different keys, so different replicates
    first, last = (boot.read_reps(boot.reps_name(str(d2 / os.path.basename(p)) + '.out.txt')) for p in (ins[0], ins[2]))
    assert sorted(first) == sorted(last)
    assert any(not np.array_equal(first[h]['T'], last[h]['T']) for h in first)
