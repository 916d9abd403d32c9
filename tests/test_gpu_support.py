"""Support intervals on the GPU (--support): every computed end against the device's own point evaluation (bit for bit) and the
C oracle, the device against the definition (ballermixplus_amd/support.py) on the oracle's objective, a planted parameter, fixed
coordinates, determinism, the CLI (nothing else it writes changes), and the refinement's results unchanged."""
import hashlib
import json
import math
import os

import numpy as np
import pytest

import cases
import test_gpu_refine as tr
from util import GOLD, REFT

from ballermixplus_amd import refine, support

pytestmark = pytest.mark.gpu

REFERENCE = [('ex1_B2', 7), ('ex2_B2maf', 9), ('ex1_B1', 7), ('ex2_B0maf_1kb', 1), ('ex2_B2', 1)]
SYNTHETIC = [('B2', 30, 16), ('B0', 0, 1), ('B0maf', 0, 16), ('B2maf', 0, 4)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _run(ctx, tg, lo, hi, drop=support.DROP, min_clr=0.0):
    scan, ref = tr._scan_refine(ctx, tg, lo, hi)
    ctx.support(drop, min_clr)
    return scan, ref, ctx.fetch_support()


def _coord(k, v):
    return refine.to_coord(k, v)


def _nuis_last_steps(h0, free, k):
    """The steps of the last round of a converged nuisance search (coordinate k held) that found no move."""
    fr = [free[j] and j != k for j in range(3)]
    if not any(fr):
        return None
    J = 0
    while not all(h0[j] * 0.5 ** J < support.NUIS_TOL[j] for j in range(3) if fr[j]):
        J += 1
    return [h * 0.5 ** (J - 1) for h in h0]


def check_support(ctx, pb, scan, ref, sup, max_checks=24, drop=support.DROP):
    """All computed tasks: inside the hull, lo <= refined <= hi, witnesses' T = eval_points bit for bit, T* = the refined CLR
    where the refinement improved.  Up to max_checks tasks: the oracle at the witness and around the outside point."""
    clr, ix, ia, iA, ns = scan
    st = pb.setup
    done = sup['rounds'] >= 0
    assert done.any()
    nat = np.stack([ref['A'], ref['x'], ref['abeta']], axis=1)
    M = len(clr)
    for k in range(3):
        assert (done[:, k, :].any() if st.free[k] else not done[:, k, :].any()), k
        rows = np.nonzero(done[:, k, 0])[0]
        assert np.array_equal(rows, np.nonzero(done[:, k, 1])[0])
        assert np.all(sup['lo'][rows, k] <= nat[rows, k]) and np.all(nat[rows, k] <= sup['hi'][rows, k]), k
        for side in range(2):
            c = np.array([_coord(k, v) for v in sup['end'][rows, k, side]])
            assert np.all(c >= st.lo[k] - 1e-12 * abs(st.lo[k])) and np.all(c <= st.hi[k] + 1e-12 * abs(st.hi[k])), k
            assert np.array_equal(_bits(sup['witness'][rows, k, side, k]), _bits(sup['end'][rows, k, side]))
            # the witness's T is the device's point evaluation at its natural values, bit for bit
            pts = np.tile([1.0, 0.5, 1.0], (M, 1))
            pts[rows] = sup['witness'][rows, k, side]
            T, _ = ctx.eval_points(pts[:, 0], pts[:, 1], pts[:, 2])
            assert np.array_equal(_bits(T[rows]), _bits(sup['witness_T'][rows, k, side])), (k, side)
            assert np.all(sup['witness_T'][rows, k, side] >= sup['T_star'][rows] - drop)
    anyd = done.any(axis=(1, 2))
    T, _ = ctx.eval_points(np.where(anyd, nat[:, 0], 1.0), np.where(anyd, nat[:, 1], 0.5), np.where(anyd, nat[:, 2], 1.0))
    assert np.array_equal(_bits(T[anyd]), _bits(sup['T_star'][anyd]))
    imp = anyd & (_bits(ref['clr']) != _bits(clr))
    assert np.array_equal(_bits(sup['T_star'][imp]), _bits(ref['clr'][imp]))
    assert np.all(sup['T_best'][anyd] >= sup['T_star'][anyd])
    assert np.all(np.isnan(sup['T_star'][~anyd])) and np.all(sup['rounds'][~anyd] == -1)
    # the oracle: witnesses reach L; outside points are within END_TOL of the end, and no neighbour of their nuisance
    # solution reaches L
    tasks = [(t, k, s) for t, k, s in zip(*np.nonzero(done)) if sup['T_star'][t] - drop > 0]
    if len(tasks) > max_checks:
        tasks = [tasks[i] for i in np.linspace(0, len(tasks) - 1, max_checks).astype(int)]
    for t, k, s in tasks:
        L = sup['T_star'][t] - drop
        Tw, _ = pb.T(t, *sup['witness'][t, k, s])
        assert Tw >= L * (1 - 1e-9), (t, k, s, Tw, L)
        if sup['censored'][t, k, s]:
            assert _coord(k, sup['end'][t, k, s]) in (st.lo[k], st.hi[k]) or sup['evals'][t, k, s] >= support.MAX_WALK
            continue
        o = sup['outside'][t, k, s]
        assert sup['outside_T'][t, k, s] < L
        assert abs(_coord(k, o[k]) - _coord(k, sup['end'][t, k, s])) < support.END_TOL[k], (t, k, s)
        _, nat0, h0 = st.start(pb.As[iA[t]], pb.xs[ix[t]], pb.abetas[ia[t]])
        h = _nuis_last_steps(h0, st.free, k)
        if h is None:
            continue
        c = [_coord(j, o[j]) for j in range(3)]
        for d in range(6):
            j = d // 2
            if j == k or not st.free[j]:
                continue
            v = min(max(c[j] + h[j] if d & 1 else c[j] - h[j], st.lo[j]), st.hi[j])
            if v == c[j]:
                continue
            nb = list(c)
            nb[j] = v
            Tn, _ = pb.T(t, math.exp(nb[0]), nb[1], math.exp(nb[2]))
            assert Tn < L * (1 + 1e-9), (t, k, s, d, Tn, L)
    return done


@pytest.mark.parametrize('name,step', REFERENCE)
def test_support_reference_examples(name, step):
    opt, case, ts, sel = tr._case_ctx(cases.ALL_CASES[name][0])
    tg, lo, hi = ts.test_gen[::step], ts.lo[::step], ts.hi[::step]
    scan, ref, sup = _run(sel.ctx, tg, lo, hi)
    pb = tr._problem_of_case(case, ts, sel)
    pb.tg, pb.lo, pb.hi = np.asarray(tg), np.asarray(lo), np.asarray(hi)
    check_support(sel.ctx, pb, scan, ref, sup)
    sel.ctx.close()


@pytest.mark.parametrize('stat,spread,step', SYNTHETIC)
def test_support_synthetic_plans(stat, spread, step):
    """31 sample sizes put the workspace in the global slab; a single n keeps it in LDS."""
    ctx, gen, rows, (st, mc, sizes, spect, props, As, xs, ab) = tr._synth(20000, stat=stat, spread=spread)
    tg = gen[::step][:2000]
    lo = np.zeros(len(tg), dtype=np.int64)
    hi = np.full(len(tg), len(gen) - 1, dtype=np.int64)
    scan, ref, _ = _run(ctx, tg, lo, hi)
    cut = float(np.quantile(ref['clr'][scan[3] >= 0], 0.9))      # the top windows: the card's time goes to the checks
    ctx.support(support.DROP, cut)
    sup = ctx.fetch_support()
    pb = tr.Problem(st, mc, sizes, spect, props, gen, rows, As, xs, ab, tg, lo, hi)
    done = check_support(ctx, pb, scan, ref, sup, max_checks=8)
    assert np.array_equal(done.any(axis=(1, 2)), (ref['rounds'] >= 0) & (ref['clr'] >= cut))
    ctx.close()


def test_device_matches_definition():
    """support.py on the C oracle's objective gives the device's ends to within 2 END_TOL; a window is skipped only where the
    host run met a comparison with L closer than 1e-8 relative (a tie the two arithmetics may decide differently)."""
    checked = skipped = 0
    for name, rows in (('ex1_B2', (300, 378, 450, 520, 600, 680)), ('ex2_B2', (400, 500, 592, 700, 800, 900))):
        opt, case, ts, sel = tr._case_ctx(cases.ALL_CASES[name][0])
        pb = tr._problem_of_case(case, ts, sel)
        idx = np.array(rows)
        pb.tg, pb.lo, pb.hi = (np.asarray(v)[idx] for v in (ts.test_gen, ts.lo, ts.hi))
        scan, ref, sup = _run(sel.ctx, pb.tg, pb.lo, pb.hi)
        st = pb.setup
        for t in range(len(idx)):
            if scan[3][t] < 0:
                continue
            near = [math.inf]
            grid = (pb.As[scan[3][t]], pb.xs[scan[1][t]], pb.abetas[scan[2][t]])
            nat = (ref['A'][t], ref['x'][t], ref['abeta'][t])
            Ts = pb.T(t, *nat)[0]
            L = Ts - support.DROP

            def f(A, x, a, t=t, L=L):
                T = pb.T(t, A, x, a)[0]
                near[0] = min(near[0], abs(T - L) / abs(L))
                return T
            _, _, ends = support.support_natural(f, st, grid, nat)
            if near[0] < 1e-8:
                skipped += 1
                continue
            checked += 1
            for k in range(3):
                for s in range(2):
                    e = ends[k][s]
                    assert abs(_coord(k, e['end']) - _coord(k, sup['end'][t, k, s])) <= 2 * support.END_TOL[k], \
                        (name, t, k, s, e['end'], sup['end'][t, k, s])
                    assert bool(e['censored']) == bool(sup['censored'][t, k, s])
        sel.ctx.close()
    assert skipped <= 2 and checked >= 10


def test_planted_parameter():
    """The planted window of test_gpu_refine (x = 0.27): the x interval contains the refined x, has a width, and (at this one
    seed, as observed) contains 0.27."""
    ctx, centre = tr_planted()
    scan, ref, sup = _run(ctx, np.array([centre]), None, None)
    lo, hi = sup['lo'][0, 1], sup['hi'][0, 1]
    assert lo <= ref['x'][0] <= hi and hi > lo
    assert lo <= 0.27 <= hi, (lo, hi)
    assert sup['lo'][0, 0] <= ref['A'][0] <= sup['hi'][0, 0]
    ctx.close()


def tr_planted():
    """test_gpu_refine.test_planted_parameter's chromosome and context."""
    from ballermixplus_amd import engine as eng, synth
    from ballermixplus_amd.hostmodel import Grids
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
    return ctx, centre


def test_fixed_coordinates_are_na():
    argv = cases.ALL_CASES['ex2_B2'][0] + ['--fixX', '0.3', '--listA', '2500', '--findBal', '-s', '10']
    opt, case, ts, sel = tr._case_ctx(argv)
    scan, ref, sup = _run(sel.ctx, ts.test_gen, ts.lo, ts.hi)
    assert np.all(sup['rounds'][:, :2] == -1) and np.all(np.isnan(sup['end'][:, :2]))
    ok = (scan[3] >= 0)
    assert np.all(sup['rounds'][ok, 2] >= 0)
    assert np.all(sup['lo'][ok, 2] >= 1.0) and np.all(sup['hi'][ok, 2] >= sup['lo'][ok, 2])
    assert np.all(_bits(sup['witness'][ok, 2, :, 1]) == _bits(np.full((ok.sum(), 2), 0.3)))
    sel.ctx.close()


def test_determinism_and_window_alone():
    opt, case, ts, sel = tr._case_ctx(cases.ALL_CASES['ex2_B2maf'][0])
    ctx = sel.ctx
    scan, ref, a = _run(ctx, ts.test_gen, ts.lo, ts.hi)
    ctx.support(support.DROP, 0.0)
    b = ctx.fetch_support()
    for key in a:
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key
    cut = float(np.quantile(ref['clr'][scan[3] >= 0], 0.9))
    ctx.support(support.DROP, cut)
    c = ctx.fetch_support()
    top = (ref['rounds'] >= 0) & (ref['clr'] >= cut)
    assert np.all(c['rounds'][~top] == -1) and np.all(c['rounds'][top] >= 0)
    for key in a:
        assert np.asarray(a[key])[top].tobytes() == np.asarray(c[key])[top].tobytes(), key
    for j in np.nonzero(top)[0][:3].tolist():       # alone: the window is the slot's only test site
        _, _, d = _run(ctx, ts.test_gen[j:j + 1], ts.lo[j:j + 1], ts.hi[j:j + 1])
        for key in a:
            assert np.asarray(a[key])[j:j + 1].tobytes() == np.asarray(d[key]).tobytes(), (j, key)
    ctx.close()


def test_needs_a_refinement_of_the_last_scan():
    from ballermixplus_amd import _lib
    opt, case, ts, sel = tr._case_ctx(cases.ALL_CASES['ex1_B2'][0] + ['-s', '50'])
    ctx = sel.ctx
    ctx.set_tests(ts.test_gen, ts.lo, ts.hi)
    ctx.scan()
    with pytest.raises(_lib.BmxError):
        ctx.support(support.DROP)
    ctx.refine(0.0)
    ctx.scan()
    with pytest.raises(_lib.BmxError):
        ctx.support(support.DROP)
    ctx.refine(0.0)
    for bad in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(_lib.BmxError):
            ctx.support(bad)
    ctx.support(support.DROP)
    assert (ctx.fetch_support()['rounds'] >= 0).any()
    ctx.close()


def _refined_digest(res):
    h = hashlib.sha256()
    for k in ('clr', 'A', 'x', 'abeta', 'nsites', 'rounds'):
        h.update(np.ascontiguousarray(res[k]).tobytes())
    return h.hexdigest()


def test_refined_results_unchanged():
    """fetch_refined on test_gpu_refine's cases hashes as it did before support intervals existed
    (tests/golden/support/refined_hashes.json, recorded with the refinement's first release)."""
    with open(os.path.join(GOLD, 'support', 'refined_hashes.json')) as f:
        want = json.load(f)
    got = {}
    for name, step in REFERENCE:
        opt, case, ts, sel = tr._case_ctx(cases.ALL_CASES[name][0])
        got['%s/%d' % (name, step)] = _refined_digest(tr._scan_refine(sel.ctx, ts.test_gen[::step], ts.lo[::step],
                                                                        ts.hi[::step])[1])
        sel.ctx.close()
    for stat, spread, step in SYNTHETIC:
        ctx, gen, rows, _ = tr._synth(20000, stat=stat, spread=spread)
        tg = gen[::step][:2000]
        res = tr._scan_refine(ctx, tg, np.zeros(len(tg), dtype=np.int64), np.full(len(tg), len(gen) - 1, dtype=np.int64))[1]
        got['synth_%s_%d_%d' % (stat, spread, step)] = _refined_digest(res)
        ctx.close()
    assert got == want


# ---------------------------------------------------------------------------------------------------- CLI

def _check_support_file(main, path):
    a = [l.rstrip('\n').split('\t') for l in open(main)]
    b = [l.rstrip('\n').split('\t') for l in open(path)]
    assert len(a) == len(b) and ''.join(t + '\n' for t in ['\t'.join(b[0])]) == support.HEADER
    computed = 0
    for la, lb in zip(a[1:], b[1:]):
        assert la[:2] == lb[:2] and len(lb) == 11
        if la[3] == 'NA' or lb[2] == 'NA':
            assert lb[2:] == ['NA'] * 9
            continue
        computed += 1
        for c in range(3, 9, 2):
            assert float(lb[c]) <= float(lb[c + 1])
        assert float(lb[9]) >= float(lb[2]) * (1 - 1e-12) or float(lb[9]) >= float(lb[2])
    return computed


def test_cli_support_leaves_everything_else(tmp_path):
    base = ['-i', os.path.join(REFT, 'Example2_balancing_10MYA_MAF_nosub.txt'), '--spect',
            os.path.join(REFT, 'HC_CEU_Neut_MAF-noSub_spect_for_B0maf.txt'), '--noSub', '--MAF', '--usePhysPos', '--fixWinSize',
            '-w', '1000', '--step', '200', '--noCenter']
    plain, sup = str(tmp_path / 'plain.txt'), str(tmp_path / 'sup.txt')
    extra = ['--refine', '--profiles', 'A,x,abeta', '--nullPerm', '3']
    tr._cli(base + ['-o', plain] + extra)
    tr._cli(base + ['-o', sup] + extra + ['--support'])
    for ext in ('', '.refined.txt', '.profile_A.txt', '.profile_x.txt', '.profile_abeta.txt', '.null.txt', '.pval.txt'):
        assert tr._read(plain + ext) == tr._read(sup + ext), ext
    assert not os.path.exists(support.output_name(plain))
    lines = open(sup).readlines()
    assert any('\tNA\t' in l for l in lines[1:])        # windows without sites are NA rows
    assert _check_support_file(sup, support.output_name(sup)) > 0


def test_cli_support_three_files(tmp_path):
    spect = os.path.join(REFT, 'HC_CEU_Neut_DAF_spect_for_B2.txt')
    third = tmp_path / 'Example3_copy_of_1.txt'
    third.write_bytes(tr._read(os.path.join(REFT, 'Example1_fullSweep_200kya_DAF.txt')))
    ins = [os.path.join(REFT, 'Example1_fullSweep_200kya_DAF.txt'), os.path.join(REFT, 'Example2_balancing_10MYA_DAF.txt'),
           str(third)]
    lst = tmp_path / 'inputs.txt'
    lst.write_text('\n'.join(ins) + '\n')
    d = tmp_path / 'sup'
    d.mkdir()
    tr._cli(['--inputs', str(lst), '--spect', spect, '-o', str(d), '-s', '3', '--refine', '--support', '--supportMin', '5'])
    mains = sorted(f for f in os.listdir(d) if f.endswith('.out.txt'))
    assert len(mains) == 3
    for f in mains:
        assert os.path.exists(support.output_name(str(d / f)))
        assert _check_support_file(str(d / f), support.output_name(str(d / f))) > 0
