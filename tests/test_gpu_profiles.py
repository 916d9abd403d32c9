"""Profile likelihoods on the GPU (--profiles): against the reference's own likelihood surfaces and the C oracle on one-value
sub-grids, max_v profile == CLR bit for bit in every plan the default variant picks, and nothing else changes: the scan's
results, the main output, the null's files."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
from util import GOLD, REFT, c_oracle, c_scan, read_tsv

from ballermixplus_amd import profiles

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX1 = os.path.join(REFT, 'Example1_fullSweep_200kya_DAF.txt')
SPECT_B2 = os.path.join(REFT, 'HC_CEU_Neut_DAF_spect_for_B2.txt')
ALL = ('A', 'x', 'abeta')


def _engine():
    from ballermixplus_amd import engine
    return engine


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _scan_all(ctx, tg, lo=None, hi=None):
    ctx.set_tests(tg, lo, hi)
    ctx.scan()
    return ctx.fetch(), {k: ctx.fetch_profile(k) for k in ALL}


def _check_invariant(res, prof):
    clr, _, _, iA, _ = res
    for k in ALL:
        p = prof[k]
        assert p.shape[0] == len(clr)
        assert np.all(p >= 0.0), k
        assert np.array_equal(_bits(p.max(axis=1)), _bits(clr)), k
        assert np.all(p[iA < 0] == 0.0), k


def _synth_ctx(N, n=100, chrom=3, stat='B2', spread=0):
    """A synthetic chromosome under `stat` (B2, B2maf, B0maf); spread > 0: sample sizes n - spread .. n (missing data), so that
    the table is read from L2."""
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
    return ctx, gen, rows, As


def _no_profile(ctx, which):
    from ballermixplus_amd import _lib
    with pytest.raises(_lib.BmxError, match='did not compute this profile'):
        ctx.fetch_profile(which)


@pytest.mark.parametrize('name,site', [('surface_ex1_B2_site0', 0), ('surface_ex1_B2_site378', 378),
                                       ('surface_ex1_B2_site756', 756), ('surface_ex2_B2maf_bal_site592', 592),
                                       ('surface_ex2_B2maf_bal_site1183', 1183)])
def test_profiles_match_reference_surfaces(name, site):
    argv = cases.ALL_CASES['ex1_B2'][0] if 'ex1' in name else cases.ALL_CASES['ex2_B2maf_findBal'][0]
    opt, case, ts = cases.host_side(list(argv))
    sel = _engine().NormalizedBetaBinom(case.data, case.grid, False, opt.MAF, False, device=0).bind(case.neut)
    sel.ctx.set_profiles(7)
    j = site                   # every site is a test site in the default window mode
    res, prof = _scan_all(sel.ctx, ts.test_gen, ts.lo, ts.hi)
    want = profiles.profiles_from_surface(np.load(os.path.join(GOLD, name + '.npz'))['T'])
    for k in ALL:
        got = prof[k][j]
        assert np.allclose(got, want[k], rtol=1e-6, atol=1e-9), (k, got, want[k])
    _check_invariant(res, prof)
    sel.ctx.close()


def test_examples_bitwise_and_unchanged_results():
    """Example 1 at strides 1 (J = 16), 4 (J = 8) and 16 (solo): max_v profile == clr bitwise, results equal with profiles off."""
    opt, case, ts = cases.host_side(list(cases.ALL_CASES['ex1_B2'][0]))
    sel = _engine().NormalizedBetaBinom(case.data, case.grid, False, False, False, device=0).bind(case.neut)
    ctx = sel.ctx
    seen = set()
    for step in (1, 4, 16):
        tg, lo, hi = ts.test_gen[::step], ts.lo[::step], ts.hi[::step]
        ctx.set_profiles(0)
        ctx.set_tests(tg, lo, hi)
        ctx.scan()
        off = ctx.fetch()
        _no_profile(ctx, 'A')               # BMX_E_STATE: this scan ran without profiles
        ctx.set_profiles(7)
        res, prof = _scan_all(ctx, tg, lo, hi)
        p = ctx.plan()
        seen.add((p['mode'], p['J']))
        _check_invariant(res, prof)
        for a, b in zip(off, res):
            assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
        ctx.set_profiles(1)                 # one profile: the others are not there
        ctx.scan()
        assert np.array_equal(_bits(ctx.fetch_profile('A')), _bits(prof['A']))
        _no_profile(ctx, 'x')
    assert {(4, 16), (4, 8), (5, 1)} <= seen, seen
    ctx.close()


def test_large_chromosome_bitwise_ranges_and_scan_write(tmp_path):
    """1 M sites: every test site a window (J = 16, several launch ranges with profiles on), then a strided solo plan on
    unsorted test sites; scan_write gives the profiles of scan."""
    ctx, gen, rows, As = _synth_ctx(1 << 20)
    ctx.set_tests(gen)
    ctx.scan()
    off = ctx.fetch()
    ctx.set_profiles(7)
    res, prof = _scan_all(ctx, gen)
    assert ctx.plan()['kernel'] == 'clr_scan_prepared_kernel<16,true>'
    assert len(ctx.launch_ranges()) >= 2
    _check_invariant(res, prof)
    for a, b in zip(off, res):
        assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
    idx = np.arange(0, len(gen), 3)[:300000]
    ctx.set_tests(gen[idx])
    m = ctx.model
    ctx.scan_write(str(tmp_path / 'w.txt'), np.arange(len(idx)), gen[idx], [f'{v}' for v in m.x], [f'{v}' for v in m.abeta],
                   [f'{v}' for v in As], chunk=65536)
    sw = {k: ctx.fetch_profile(k) for k in ALL}
    _, pr = _scan_all(ctx, gen[idx])
    for k in ALL:
        assert np.array_equal(_bits(sw[k]), _bits(pr[k])), k
    rng = np.random.default_rng(5)
    sub = rng.permutation(np.arange(1000, len(gen) - 1000, 97))[:5000]
    res, prof = _scan_all(ctx, gen[sub])
    assert ctx.plan()['kernel'].startswith('clr_scan_solo_kernel<')
    _check_invariant(res, prof)
    ctx.close()


def test_table_in_l2_bitwise_and_unchanged_results():
    """31 sample sizes (the table is read from L2): J = 16, J = 8 and solo plans, max_v profile == clr bitwise, results equal
    with profiles off."""
    ctx, gen, rows, As = _synth_ctx(300000, chrom=11, spread=30)
    want = {1: 'clr_scan_prepared_kernel<16,false>', 4: 'clr_scan_prepared_kernel<8,false>', 16: 'clr_scan_solo_kernel<false>'}
    for step, kernel in want.items():
        tg = gen[::step]
        ctx.set_profiles(0)
        ctx.set_tests(tg)
        ctx.scan()
        off = ctx.fetch()
        assert ctx.plan()['kernel'] == kernel
        ctx.set_profiles(['A', 'x', 'abeta'])
        res, prof = _scan_all(ctx, tg)
        assert ctx.plan()['kernel'] == kernel
        _check_invariant(res, prof)
        assert np.sum(res[3] >= 0) > 0
        for a, b in zip(off, res):
            assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8)), step
    ctx.close()


@pytest.mark.parametrize('stat', ['B2', 'B2maf', 'B0maf'])
def test_sub_grid_equivalence_against_oracle(stat):
    """Column v of each profile == the C oracle's scan with that single A, x or alpha_beta, on more than 2 000 test sites:
    both sides of every launch cut, the first and last 64 test sites and a spread over the chromosome."""
    ctx, gen, rows, As = _synth_ctx(1 << 20, n=50, chrom=7, stat=stat)
    ctx.set_profiles(7)
    res, prof = _scan_all(ctx, gen)
    _check_invariant(res, prof)
    cuts = ctx.launch_ranges()
    assert len(cuts) >= 2
    M = len(gen)
    pick = set(range(64)) | set(range(M - 64, M))
    for c in cuts[1:]:
        pick |= set(range(int(c) - 16, int(c) + 16))
    pick |= set(np.linspace(0, M - 1, 2000).astype(int).tolist())
    pick = np.array(sorted(pick))
    assert len(pick) >= 2000
    _, R = ctx.fetch_lut()
    R = np.where(np.isfinite(R), R, 0.0)
    L = c_oracle()
    lo, hi = np.zeros(len(pick), np.int64), np.full(len(pick), M - 1, np.int64)
    As = np.asarray(As, dtype=np.float64)
    tg = gen[pick]
    for v in range(len(As)):
        o = c_scan(L, R, As[v:v + 1], gen, rows, tg, lo, hi)[0]
        assert np.allclose(prof['A'][pick, v], o, rtol=1e-6, atol=1e-9), ('A', v)
    for v in range(R.shape[0]):
        o = c_scan(L, R[v:v + 1], As, gen, rows, tg, lo, hi)[0]
        assert np.allclose(prof['x'][pick, v], o, rtol=1e-6, atol=1e-9), ('x', v)
    for v in range(R.shape[1]):
        o = c_scan(L, R[:, v:v + 1], As, gen, rows, tg, lo, hi)[0]
        assert np.allclose(prof['abeta'][pick, v], o, rtol=1e-6, atol=1e-9), ('abeta', v)
    ctx.close()


def _cli(args):
    r = subprocess.run([sys.executable, os.path.join(REPO, 'BalLeRMixPlus_amd.py')] + args, capture_output=True, text=True,
                       timeout=900, cwd=REPO)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _read(p):
    with open(p, 'rb') as f:
        return f.read()


def test_cli_findbal_null_and_main_output(tmp_path):
    base = ['-i', os.path.join(REFT, 'Example2_balancing_10MYA_MAF.txt'), '--spect',
            os.path.join(REFT, 'HC_CEU_Neut_MAF_spect_for_B2maf.txt'), '--MAF']
    plain, prof, both, nul = (str(tmp_path / n) for n in ('plain.txt', 'prof.txt', 'both.txt', 'null.txt'))
    _cli(base + ['-o', plain])
    _cli(base + ['-o', prof, '--profiles', 'abeta,A,x'])
    assert _read(plain) == _read(prof)
    head = open(prof + '.profile_abeta.txt').readline().rstrip('\n').split('\t')
    assert head[:2] == ['physPos', 'genPos'] and head[-2:] == ['CLR_bal', 'CLR_pos']
    rows = [l.rstrip('\n').split('\t') for l in open(prof + '.profile_abeta.txt').readlines()[1:]]
    gold = read_tsv(os.path.join(GOLD, 'e2e', 'ex2_B2maf_findBal.tsv'))
    assert len(rows) == len(gold)
    for r, g in zip(rows, gold):
        assert r[0] == g[0]
        want = float(g[2])
        assert abs(float(r[-2]) - want) <= max(1e-9, 1e-6 * abs(want)), (r, g)
    main = [l.split('\t') for l in open(prof).readlines()[1:]]
    for name in ALL:
        body = [l.rstrip('\n').split('\t') for l in open(prof + '.profile_%s.txt' % name).readlines()[1:]]
        n = len(body[0]) - 2 - (2 if name == 'abeta' else 0)
        for r, m in zip(body, main):
            assert max(float(v) for v in r[2:2 + n]) == float(m[2])
    _cli(base + ['-o', nul, '--nullPerm', '3'])
    _cli(base + ['-o', both, '--nullPerm', '3', '--profiles', 'A,x,abeta'])
    for ext in ('.pval.txt', '.null.txt'):
        assert _read(nul + ext) == _read(both + ext), ext
    for name in ALL:
        assert _read(prof + '.profile_%s.txt' % name) == _read(both + '.profile_%s.txt' % name), name


def test_cli_two_files_write_both_sets(tmp_path):
    spect = SPECT_B2
    a, b = EX1, os.path.join(REFT, 'Example2_balancing_10MYA_DAF.txt')
    out = str(tmp_path / 'o' / '{}.out')
    _cli(['-i', a + ',' + b, '--spect', spect, '-o', out, '--profiles', 'x', '-s', '3'])
    got = sorted(os.path.basename(p) for p in glob.glob(str(tmp_path / 'o' / '*.profile_*')))
    assert got == ['Example1_fullSweep_200kya_DAF.out.profile_x.txt', 'Example2_balancing_10MYA_DAF.out.profile_x.txt'], got
    for stem in ('Example1_fullSweep_200kya_DAF', 'Example2_balancing_10MYA_DAF'):
        main = read_tsv(str(tmp_path / 'o' / (stem + '.out')))
        pr = read_tsv(str(tmp_path / 'o' / (stem + '.out.profile_x.txt')))
        assert len(main) == len(pr) > 0
        for r, m in zip(pr, main):       # each file's own profiles: their maximum is that file's CLR column
            assert r[:2] == m[:2]
            assert max(float(v) for v in r[2:]) == float(m[2]), (stem, r, m)
