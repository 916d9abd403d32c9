"""Off-grid refinement on the GPU (--refine): point evaluation against the reference's own T at off-grid points, refined rows
against the C oracle at the reported point and at its compass neighbours, a planted parameter, fixed coordinates,
determinism, and the CLI (nothing else it writes changes)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
from util import GOLD, REFT, c_oracle, c_scan, c_sel_table, read_tsv

from ballermixplus_amd import refine

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RG = os.path.join(GOLD, 'refine')


def _engine():
    from ballermixplus_amd import engine
    return engine


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _case_ctx(argv):
    opt, case, ts = cases.host_side(list(argv))
    sel = _engine().NormalizedBetaBinom(case.data, case.grid, opt.nofreq, opt.MAF, opt.nosub, device=0).bind(case.neut)
    return opt, case, ts, sel


class Problem:
    """What the checks need of one scanned slot: sites, rows, the model's per-size tables for the oracle."""

    def __init__(self, stat, min_count, sizes, spect, props, genpos, rows, As, xs, abetas, tg, lo, hi):
        self.stat, self.min_count = stat, int(min_count)
        self.sizes = sorted(int(n) for n in sizes)
        self.spect, self.props = spect, props
        self.genpos = np.asarray(genpos, dtype=np.float64)
        self.rows = np.asarray(rows, dtype=np.int32)
        self.As, self.xs, self.abetas = list(As), list(xs), list(abetas)
        self.tg, self.lo, self.hi = (np.asarray(v) for v in (tg, lo, hi))
        self.setup = refine.Setup(self.As, self.xs, self.abetas)
        self.L = c_oracle()

    def R(self, x, a):
        """R[1][1][rows] of the one-value grid (x, a), by the C oracle's selection table."""
        tabs, g, pr = [], [], []
        for n in self.sizes:
            t = c_sel_table(self.L, self.stat, n, self.min_count, [x], [a])
            tabs.append(t)
            for k in range(t.shape[2]):
                g.append(self.spect.get((k, n), np.nan))
                pr.append(self.props[n])
        with np.errstate(invalid='ignore', divide='ignore'):
            return np.concatenate(tabs, axis=2) * np.array(pr) / np.array(g) - 1.0

    def T(self, j, A, x, a):
        """(CLR, nSites) of test site j at one point by the C oracle (CLR 0 where T <= 0)."""
        clr, _, _, _, ns = c_scan(self.L, self.R(x, a), [A], self.genpos, self.rows, self.tg[j:j + 1], self.lo[j:j + 1],
                                  self.hi[j:j + 1])
        return float(clr[0]), int(ns[0])


def _problem_of_case(case, ts, sel):
    m = sel.model
    return Problem(case.stat, case.data.minCount, m.sizes.tolist(), case.neut.spect, case.neut.sampProps, case.data.genPos,
                   sel.rows, case.As, case.xs, case.abetas, ts.test_gen, ts.lo, ts.hi)


def _last_steps(h0, free):
    """The steps of the last round that found no move: all steps halve together, the search stops once every free step is
    below its tolerance."""
    J = 0
    while not all(h0[k] * 0.5 ** J < refine.TOL[k] for k in range(3) if free[k]):
        J += 1
    return [h * 0.5 ** (J - 1) for h in h0]


def check_refined(ctx, pb, scan, res, max_checks=24):
    """Every row: CLR >= the grid's bitwise, unrefined rows unchanged, inside the bounds.  Up to max_checks improved rows:
    the oracle's T at the reported point and no better compass neighbour at the last steps."""
    clr, ix, ia, iA, ns = scan
    r = res
    assert np.all(r['clr'] >= clr)
    imp = _bits(r['clr']) != _bits(clr)
    assert np.all(r['rounds'][imp] >= 0)
    assert np.all(r['rounds'][iA < 0] == -1)
    same = ~imp & (iA >= 0)
    for key, grid, idx in (('A', pb.As, iA), ('x', pb.xs, ix), ('abeta', pb.abetas, ia)):
        want = np.asarray(grid, dtype=np.float64)[np.maximum(idx, 0)]
        assert np.array_equal(_bits(r[key][same]), _bits(want[same])), key
        assert np.all(np.isnan(r[key][iA < 0])), key
    assert np.array_equal(r['nsites'][~imp], ns[~imp])
    st = pb.setup
    for k, key in enumerate(('A', 'x', 'abeta')):
        c = np.array([refine.to_coord(k, v) for v in r[key][iA >= 0]])
        assert np.all(c >= st.lo[k] - 1e-12 * abs(st.lo[k])) and np.all(c <= st.hi[k] + 1e-12 * abs(st.hi[k])), key
    rows = np.nonzero(imp)[0]
    if len(rows) > max_checks:
        rows = rows[np.linspace(0, len(rows) - 1, max_checks).astype(int)]
    for j in rows.tolist():
        A, x, a = r['A'][j], r['x'][j], r['abeta'][j]
        T, n = pb.T(j, A, x, a)
        assert abs(T - r['clr'][j]) <= 1e-9 * abs(T), (j, T, r['clr'][j])
        assert n == r['nsites'][j]
        if r['rounds'][j] >= refine.MAX_ROUNDS:
            continue
        c0, nat0, h0 = st.start(pb.As[iA[j]], pb.xs[ix[j]], pb.abetas[ia[j]])
        h = _last_steps(h0, st.free)
        c = (refine.to_coord(0, A), x, refine.to_coord(2, a))
        for d in range(6):
            k = d // 2
            if not st.free[k]:
                continue
            v = min(max(c[k] + h[k] if d & 1 else c[k] - h[k], st.lo[k]), st.hi[k])
            if v == c[k]:
                continue
            nb = list(c)
            nb[k] = v
            Tn, _ = pb.T(j, math.exp(nb[0]), nb[1], math.exp(nb[2]))
            assert Tn <= r['clr'][j] * (1 + 1e-9), (j, d, Tn, r['clr'][j])
    return imp


# ---------------------------------------------------------------------------------------------------- point evaluation

@pytest.mark.parametrize('name', sorted(f[:-10] for f in os.listdir(RG) if f.endswith('.args.json')))
def test_eval_points_match_reference(name):
    with open(os.path.join(RG, name + '.args.json')) as f:
        args = json.load(f)
    args = [os.path.join(REFT, a) if a.endswith('.txt') else a for a in args]
    x, a, A = (float(args[args.index(k) + 1]) for k in ('--fixX', '--fixAlpha', '--listA'))
    opt, case, ts, sel = _case_ctx(args)
    ctx = sel.ctx
    ctx.set_tests(ts.test_gen, ts.lo, ts.hi)
    T, ns = ctx.eval_points(A, x, a)
    gold = read_tsv(os.path.join(RG, name + '.tsv'))
    assert len(gold) == len(T)
    hit = 0
    for j, row in enumerate(gold):
        want = float(row[2])
        if want > 0:            # the reference prints T where it is > 0, else an all-zero row
            hit += 1
            assert abs(T[j] - want) <= 1e-9 * want, (j, T[j], want)
            assert int(row[6]) == ns[j]
        else:
            assert not T[j] > 0, (j, T[j])
    assert hit >= 5
    ctx.close()


def test_eval_points_at_grid_points_match_surface():
    opt, case, ts, sel = _case_ctx(cases.ALL_CASES['ex1_B2'][0] + ['-s', '60'])
    ctx = sel.ctx
    ctx.set_tests(ts.test_gen, ts.lo, ts.hi)
    rng = np.random.default_rng(5)
    M = len(ts.test_gen)
    iA, ix, ia = rng.integers(0, len(case.As), M), rng.integers(0, len(case.xs), M), rng.integers(0, len(case.abetas), M)
    A = np.asarray(case.As)[iA]
    x = np.asarray(case.xs)[ix]
    a = np.asarray(case.abetas)[ia]
    T, ns = ctx.eval_points(A, x, a)
    for j in range(M):
        S, sn = ctx.surface(ts.test_gen[j], ts.lo[j], ts.hi[j])
        want = S[iA[j], ix[j], ia[j]]
        if np.isnan(want):
            assert T[j] == -np.inf and ns[j] == 0
        else:
            assert abs(T[j] - want) <= 1e-12 * abs(want), (j, T[j], want)
            assert ns[j] == sn[iA[j]]
    ctx.close()


# ---------------------------------------------------------------------------------------------------- refinement

def _synth(N, n=100, chrom=3, stat='B2', spread=0):
    """A synthetic chromosome under `stat`; spread > 0: sample sizes n - spread .. n (the table is read from L2)."""
    from ballermixplus_amd import synth
    from ballermixplus_amd.hostmodel import Grids
    eng = _engine()
    phys, gen, k, nn = synth.synth_chromosome(N, n, chrom)
    if spread:
        n2 = np.random.default_rng(chrom).integers(n - spread, n + 1, len(k))
        k = np.where(k == nn, n2, np.maximum(1, np.minimum(n2 - 1, (k * n2) // nn)))
        nn = n2
    if stat.startswith('B0'):
        keep = (k > 0) & (k < nn)
        gen, k, nn = gen[keep], k[keep], nn[keep]
    if stat.endswith('maf'):
        k = np.minimum(k, nn - k)
    spect = {(a, b): f for a, b, f in synth.spect_from_counts(k, nn)}
    sizes = sorted(set(nn.tolist()))
    props = {s_: float(sum(f for (a, b), f in spect.items() if b == s_)) for s_ in sizes}
    xs, ab, As = Grids(None, None, False, False, None, None).scan_order()
    model = eng.ModelArrays(stat, int(k.min()), sizes, spect, props, xs, ab)
    ctx = eng.Context(0)
    ctx.set_model(model, As)
    rows = model.rows_of(k, nn)
    ctx.set_sites(gen, rows)
    return ctx, gen, rows, (stat, int(k.min()), sizes, spect, props, As, xs, ab)


def _scan_refine(ctx, tg, lo, hi, min_clr=0.0):
    ctx.set_tests(tg, lo, hi)
    ctx.scan()
    scan = ctx.fetch()
    ctx.refine(min_clr)
    return scan, ctx.fetch_refined()


@pytest.mark.parametrize('name,step', [('ex1_B2', 7), ('ex2_B2maf', 9), ('ex1_B1', 7), ('ex2_B0maf_1kb', 1), ('ex2_B2', 1)])
def test_refine_reference_examples(name, step):
    opt, case, ts, sel = _case_ctx(cases.ALL_CASES[name][0])
    tg, lo, hi = ts.test_gen[::step], ts.lo[::step], ts.hi[::step]
    scan, res = _scan_refine(sel.ctx, tg, lo, hi)
    pb = _problem_of_case(case, ts, sel)
    pb.tg, pb.lo, pb.hi = np.asarray(tg), np.asarray(lo), np.asarray(hi)
    imp = check_refined(sel.ctx, pb, scan, res)
    assert imp.sum() > 0
    sel.ctx.close()


@pytest.mark.parametrize('stat,spread,step', [('B2', 30, 16), ('B0', 0, 1), ('B0maf', 0, 16), ('B2maf', 0, 4)])
def test_refine_synthetic_plans(stat, spread, step):
    """Multi-n (31 sample sizes: the table in L2), and strided test sites (sparse: the solo plan)."""
    ctx, gen, rows, (st, mc, sizes, spect, props, As, xs, ab) = _synth(20000, stat=stat, spread=spread)
    tg = gen[::step][:2000]
    lo = np.zeros(len(tg), dtype=np.int64)
    hi = np.full(len(tg), len(gen) - 1, dtype=np.int64)
    scan, res = _scan_refine(ctx, tg, lo, hi)
    pb = Problem(st, mc, sizes, spect, props, gen, rows, As, xs, ab, tg, lo, hi)
    imp = check_refined(ctx, pb, scan, res, max_checks=8)
    assert imp.sum() > 0
    ctx.close()


def test_planted_parameter():
    """About 2000 sites around one centre drawn from the folded beta-binomial at x = 0.27, alpha_beta = 40 with probability
    exp(-A0 d), neutral elsewhere: the grid can only say 0.25 or 0.30."""
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
    props = {n: 1.0}
    xs, ab, As = Grids(None, None, False, False, None, None).scan_order()
    model = eng.ModelArrays('B2', 1, [n], spect, props, xs, ab)
    ctx = eng.Context(0)
    ctx.set_model(model, As)
    ctx.set_sites(gen, model.rows_of(k, nn))
    scan, res = _scan_refine(ctx, np.array([centre]), None, None)
    assert res['clr'][0] > scan[0][0]
    assert abs(res['x'][0] - x0) < 0.01, (res['x'][0], xs[scan[1][0]])
    ctx.close()


def test_fixed_coordinates_are_kept():
    """--fixX 0.3, a one-value --listA and --findBal: the fixed coordinates are returned bit for bit, alpha_beta stays >= 1."""
    argv = cases.ALL_CASES['ex2_B2'][0] + ['--fixX', '0.3', '--listA', '2500', '--findBal', '-s', '10']
    opt, case, ts, sel = _case_ctx(argv)
    scan, res = _scan_refine(sel.ctx, ts.test_gen, ts.lo, ts.hi)
    ok = scan[3] >= 0
    assert np.all(_bits(res['x'][ok]) == _bits(np.full(ok.sum(), 0.3)))
    assert np.all(_bits(res['A'][ok]) == _bits(np.full(ok.sum(), 2500.0)))
    assert np.all(res['abeta'][ok] >= 1.0)
    assert (res['clr'] > scan[0]).sum() > 0
    sel.ctx.close()


def test_determinism_subset_and_profiles():
    opt, case, ts, sel = _case_ctx(cases.ALL_CASES['ex2_B2maf'][0])
    ctx = sel.ctx
    scan, a = _scan_refine(ctx, ts.test_gen, ts.lo, ts.hi)
    ctx.refine(0.0)
    b = ctx.fetch_refined()
    for k in a:
        assert np.array_equal(a[k].view(np.uint64) if a[k].dtype == np.float64 else a[k],
                              b[k].view(np.uint64) if b[k].dtype == np.float64 else b[k]), k
    cut = float(np.quantile(scan[0][scan[3] >= 0], 0.8))
    ctx.refine(cut)
    c = ctx.fetch_refined()
    top = (scan[3] >= 0) & (scan[0] >= cut)
    assert np.all(c['rounds'][~top] == -1) and np.all(c['rounds'][top] >= 0)
    for k in a:
        assert np.array_equal(np.asarray(a[k])[top].tobytes(), np.asarray(c[k])[top].tobytes()), k
    assert np.array_equal(_bits(c['clr'][~top]), _bits(scan[0][~top]))
    ctx.set_profiles(7)
    scan2, d = _scan_refine(ctx, ts.test_gen, ts.lo, ts.hi)
    for k in a:
        assert np.array_equal(np.asarray(a[k]).tobytes(), np.asarray(d[k]).tobytes()), k
    ctx.close()


# ---------------------------------------------------------------------------------------------------- CLI

def _cli(args):
    r = subprocess.run([sys.executable, os.path.join(REPO, 'BalLeRMixPlus_amd.py')] + args, capture_output=True, text=True,
                       timeout=900, cwd=REPO)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _read(p):
    with open(p, 'rb') as f:
        return f.read()


def _check_refined_file(main, path):
    a = open(main).readlines()
    b = open(path).readlines()
    assert len(a) == len(b) and a[0] == b[0]
    changed = 0
    for la, lb in zip(a[1:], b[1:]):
        if la == lb:
            continue
        changed += 1
        fa, fb = la.rstrip('\n').split('\t'), lb.rstrip('\n').split('\t')
        assert fa[:2] == fb[:2]
        assert float(fb[2]) > float(fa[2])
        assert fb[2] == repr(float(fb[2])) and fb[6] == repr(int(fb[6]))
    return changed


def test_cli_refine_leaves_everything_else(tmp_path):
    base = ['-i', os.path.join(REFT, 'Example2_balancing_10MYA_DAF.txt'), '--spect', os.path.join(REFT, 'HC_CEU_Neut_DAF_spect_for_B2.txt')]
    plain, ref, full, fullr, top = (str(tmp_path / n) for n in ('plain.txt', 'ref.txt', 'full.txt', 'fullr.txt', 'top.txt'))
    _cli(base + ['-o', plain])
    _cli(base + ['-o', ref, '--refine'])
    assert _read(plain) == _read(ref)
    assert _check_refined_file(ref, refine.output_name(ref)) > 0
    _cli(base + ['-o', full, '--profiles', 'A,x,abeta', '--nullPerm', '3'])
    _cli(base + ['-o', fullr, '--refine', '--profiles', 'A,x,abeta', '--nullPerm', '3'])
    for ext in ('', '.profile_A.txt', '.profile_x.txt', '.profile_abeta.txt', '.null.txt', '.pval.txt'):
        assert _read(full + ext) == _read(fullr + ext), ext
    assert _read(refine.output_name(fullr)) == _read(refine.output_name(ref))
    _cli(base + ['-o', top, '--refine', '--refineMin', '1e300'])
    assert _read(refine.output_name(top)) == _read(top)


def test_cli_refine_three_files(tmp_path):
    spect = os.path.join(REFT, 'HC_CEU_Neut_DAF_spect_for_B2.txt')
    third = tmp_path / 'Example3_copy_of_1.txt'
    third.write_bytes(_read(os.path.join(REFT, 'Example1_fullSweep_200kya_DAF.txt')))
    ins = [os.path.join(REFT, 'Example1_fullSweep_200kya_DAF.txt'), os.path.join(REFT, 'Example2_balancing_10MYA_DAF.txt'),
           str(third)]
    lst = tmp_path / 'inputs.txt'
    lst.write_text('\n'.join(ins) + '\n')
    d1, d2 = tmp_path / 'plain', tmp_path / 'ref'
    d1.mkdir()
    d2.mkdir()
    _cli(['--inputs', str(lst), '--spect', spect, '-o', str(d1), '-s', '3'])
    _cli(['--inputs', str(lst), '--spect', spect, '-o', str(d2), '-s', '3', '--refine'])
    outs = sorted(f for f in os.listdir(d1))
    assert outs and sorted(f for f in os.listdir(d2) if not f.endswith('.refined.txt')) == outs
    for f in outs:
        assert _read(d1 / f) == _read(d2 / f)
        assert _check_refined_file(str(d2 / f), refine.output_name(str(d2 / f))) > 0
