"""GPU parity: the HIP path, called through the C ABI, against the reference's goldens and
the oracle.  Tolerances: integer/index fields exact (ties within rounding noise excepted, see
cases.compare_rows); CLR within 1e-6 relative (BASELINE.json north_star), absolute floor 1e-9."""
import glob
import os

import numpy as np
import pytest

import cases
from util import GOLD, c_oracle, c_scan, orc, read_tsv

pytestmark = pytest.mark.gpu

LUTS = sorted(glob.glob(os.path.join(GOLD, 'lut_*.npz')))


def _engine():
    from ballermixplus_amd import engine
    return engine


@pytest.mark.parametrize('path', LUTS, ids=[os.path.basename(p)[4:-4] for p in LUTS])
def test_device_selection_table_matches_reference(path):
    """K1 (device lgamma / beta-binomial) vs NormalizedBetaBinom.normProbs of the reference.  The fixtures pin the glibc of the
    host that made them (scipy's lgam calls its log), and K1 follows the log of the host it RUNS on through LogPatch: on a host
    whose libm rounds a patched argument differently this is the test that fails first, at alpha_beta >= 1e4."""
    eng = _engine()
    stat = os.path.basename(path)[4:-4].split('_')[0]
    z = np.load(path)
    xs, ab, minc = z['x'].tolist(), z['abeta'].tolist(), int(z['minCount'])
    sizes = sorted(set(z['total'].tolist()))
    spect = {(k, n): 1.0 for n in sizes for k in range(n + 1)}
    props = {n: 1.0 for n in sizes}
    model = eng.ModelArrays(stat, minc, sizes, spect, props, xs, ab)
    ctx = eng.Context(0)
    ctx.set_model(model, [100.0])
    psel, R = ctx.fetch_lut()
    rows = model.rows_of(z['count'], z['total'])
    got = psel[:, :, rows]
    ref = z['table']
    rel = np.abs(got - ref) / np.abs(ref)
    # The large-argument lgam noise (alpha_beta >= 1e4) must be REPRODUCED, not merely
    # approximated: a 1-ulp-accurate log would already be off by 1e-5 at alpha_beta = 1e9.
    # The device log is correctly rounded; glibc's (which scipy calls) is not on ~0.015 % of the
    # arguments; the host ships those exceptions (LogPatch), so nothing beyond exp/log-of-small
    # ulp differences (amplified where normBase -> 0, e.g. B_0 at tiny alpha_beta) remains.
    assert np.nanmax(rel) < 1e-12, float(np.nanmax(rel))
    assert np.allclose(R[:, :, rows], got - 1.0, rtol=0, atol=1e-15 * np.abs(got).max() + 1e-300)
    ctx.close()


def _run_case(name, tmp_path):
    eng = _engine()
    from ballermixplus_amd import scan as scanmod
    argv, gold = cases.ALL_CASES[name]
    opt, case, ts = cases.host_side(argv)
    sel = eng.NormalizedBetaBinom(case.data, case.grid, opt.nofreq, opt.MAF, opt.nosub)
    sel.bind(case.neut)
    res = eng.scan_batch(sel, ts.test_gen, ts.lo, ts.hi)
    out = str(tmp_path / ('bmx_gpu_%s.tsv' % name))
    scanmod.write_rows(out, ts, res, sel)
    with open(out) as f:
        lines = f.readlines()[1:]
    return case, ts, lines, gold


@pytest.mark.parametrize('name', sorted(cases.ALL_CASES))
def test_scan_reproduces_golden_file(name, tmp_path):
    """Every row of every golden output file (configs 1 and 2 of BASELINE.json among them)."""
    if not os.path.exists(cases.ALL_CASES[name][1]):
        pytest.skip('fixture not generated')
    case, ts, lines, gold = _run_case(name, tmp_path)
    worst, ties = cases.compare_rows(lines, gold, rtol=1e-6, case=case, ts=ts)
    assert worst < 1e-6
    assert ties == 0 or name.endswith('B1'), ties


def test_cli_end_to_end_config1(tmp_path):
    """The drop-in command line itself, byte-compatible header and row format."""
    from ballermixplus_amd import cli
    argv, gold = cases.ALL_CASES['ex1_B2']
    out = tmp_path / 'o.txt'
    cli.main(argv + ['-o', str(out), '-s', '50'])
    got = out.read_text().splitlines()
    assert got[0] == 'physPos\tgenPos\tCLR\tx_hat\ts_hat\tA_hat\tnSites'
    ref = read_tsv(gold)[::50]
    for a, b in zip([l.split('\t') for l in got[1:]], ref):
        assert a[:2] == b[:2] and a[3:] == b[3:]
        assert abs(float(a[2]) - float(b[2])) <= 1e-6 * abs(float(b[2]))


def _synth_case(N, n, chrom=1, bal=False, listA=None):
    from ballermixplus_amd import synth
    from ballermixplus_amd.hostmodel import Grids
    phys, gen, k, nn = synth.synth_chromosome(N, n, chrom)
    spect = {(a, b): f for a, b, f in synth.spect_from_counts(k, nn)}
    props = {n: 1.0}
    grid = Grids(None, None, bal, bal, None, listA)
    return phys, gen, k, nn, spect, props, grid


@pytest.mark.parametrize('key,N,n,step,bal', [('20k', 20000, 100, 200, False), ('20k_n200_bal', 20000, 200, 400, True),
                                              ('1M', 1000000, 100, 100000, False), ('1M', 1000000, 100, 4000, False),
                                              ('1M_n200_bal', 1000000, 200, 40000, True)])
def test_synthetic_strided_windows_match_reference(key, N, n, step, bal):
    """BASELINE configs 3/5 in miniature + config 3 at full size on the windows the reference
    could afford (tests/golden/synth, produced by running the reference with -s)."""
    path = os.path.join(GOLD, 'synth', 'synth_%s_step%d.tsv' % (key, step))
    if not os.path.exists(path):
        pytest.skip('fixture not generated')
    eng = _engine()
    listA = ','.join(str(100 * i) for i in range(1, 101)) if bal else None
    phys, gen, k, nn, spect, props, grid = _synth_case(N, n, 2 if bal else 1, bal, listA)
    xs, ab, As = grid.scan_order()
    model = eng.ModelArrays('B2', int(k.min()), [n], spect, props, xs, ab)
    ctx = eng.Context(0)
    ctx.set_model(model, As)
    ctx.set_sites(gen, model.rows_of(k, nn))
    idx = np.arange(0, N, step)
    ctx.set_tests(gen[idx], np.zeros(len(idx), np.int64), np.full(len(idx), N - 1, np.int64))
    ctx.scan()
    clr, ix, ia, iA, ns = ctx.fetch()
    rows = read_tsv(path)
    assert len(rows) == len(idx)
    for j, r in enumerate(rows):
        assert int(r[0]) == phys[idx[j]]
        if r[3:6] == ['0.0', '0.0', '0.0']:
            assert iA[j] < 0
            continue
        assert (repr(xs[ix[j]]), repr(ab[ia[j]]), repr(As[iA[j]]), str(ns[j])) == (r[3], r[4], r[5], r[6]), (j, r)
        assert abs(clr[j] - float(r[2])) <= max(1e-9, 1e-6 * abs(float(r[2]))), (j, r, clr[j])
    ctx.close()


def test_full_size_properties_config3():
    """Config 3 (1M SNPs, n=100, default grid) at full size, through properties that need no
    reference run: (i) a strided subset scanned alone equals the same rows of a denser scan
    (shard invariance: what multi-GPU sharding relies on); (ii) windows fully inside a 60k-site
    sub-chromosome give the same rows (CLR to rounding) when that sub-chromosome is scanned on its own;
    (iii) the C oracle agrees on a sample of rows."""
    eng = _engine()
    N, n = 1000000, 100
    phys, gen, k, nn, spect, props, grid = _synth_case(N, n)
    xs, ab, As = grid.scan_order()
    model = eng.ModelArrays('B2', int(k.min()), [n], spect, props, xs, ab)
    rows = model.rows_of(k, nn)
    ctx = eng.Context(0)
    ctx.set_model(model, As)
    ctx.set_sites(gen, rows)
    full_lo = lambda m: np.zeros(m, np.int64)
    idx = np.arange(400000, 400000 + 8192)
    ctx.set_tests(gen[idx], full_lo(len(idx)), np.full(len(idx), N - 1, np.int64))
    ctx.scan()
    dense = [a.copy() for a in ctx.fetch()]
    # test sites are processed in groups of J consecutive entries of the test list; a shard that
    # starts on a group boundary (the multi-GPU driver deals blocks of 4096) is bit-identical
    sub = idx[2048:6144]
    ctx.set_tests(gen[sub], full_lo(len(sub)), np.full(len(sub), N - 1, np.int64))
    ctx.scan()
    shard = ctx.fetch()
    for a, b in zip(dense, shard):
        assert np.array_equal(a[2048:6144], b)
    # any other subset regroups the test sites: same argmax, CLR equal to rounding
    sub = idx[::7]
    ctx.set_tests(gen[sub], full_lo(len(sub)), np.full(len(sub), N - 1, np.int64))
    ctx.scan()
    sparse = ctx.fetch()
    for a, b in zip(dense[1:], sparse[1:]):
        assert np.array_equal(a[::7], b)
    assert np.allclose(dense[0][::7], sparse[0], rtol=1e-12, atol=0)
    # the per-site kernel (variant 2) agrees with the grouped one
    ctx.set_variant(2)
    ctx.scan()
    v2 = ctx.fetch()
    ctx.set_variant(0)
    for a, b in zip(sparse[1:], v2[1:]):
        assert np.array_equal(a, b)
    assert np.allclose(sparse[0], v2[0], rtol=1e-12, atol=0)
    # (ii) cut out [370000, 440000): all windows of idx (+-2.6k sites) lie inside
    lo_c, hi_c = 370000, 440000
    ctx2 = eng.Context(0)
    ctx2.set_model(model, As)
    ctx2.set_sites(gen[lo_c:hi_c], rows[lo_c:hi_c])
    ctx2.set_tests(gen[idx], full_lo(len(idx)), np.full(len(idx), hi_c - lo_c - 1, np.int64))
    ctx2.scan()
    cut = ctx2.fetch()
    # a different site array ranks its rows afresh for the far-field moments (which rows are summed as
    # moments is a per-array choice), so the CLR agrees to rounding, not bit for bit
    for a, b in zip(dense[1:], cut[1:]):
        assert np.array_equal(a, b)
    assert np.allclose(dense[0], cut[0], rtol=1e-10, atol=1e-13)
    # (iii) oracle on 24 rows
    L = c_oracle()
    _, R = ctx.fetch_lut()
    pick = idx[:: len(idx) // 24][:24]
    oc = c_scan(L, R, As, gen[lo_c:hi_c], rows[lo_c:hi_c], gen[pick], np.zeros(len(pick), np.int64),
                np.full(len(pick), hi_c - lo_c - 1, np.int64))
    sel = np.searchsorted(idx, pick)
    assert np.array_equal(oc[1], dense[1][sel]) and np.array_equal(oc[2], dense[2][sel])
    assert np.array_equal(oc[3], dense[3][sel]) and np.array_equal(oc[4], dense[4][sel])
    assert np.max(np.abs(oc[0] - dense[0][sel]) / np.maximum(np.abs(oc[0]), 1e-9)) < 1e-9
    ctx.close()
    ctx2.close()


def test_edge_cases():
    """Empty windows, a single site, duplicated positions (all ties excluded, v1:455), windows
    that exclude the test site's neighbourhood, and a test position off the site grid."""
    eng = _engine()
    L = c_oracle()
    n = 20
    rng = np.random.default_rng(5)
    N = 300
    gen = np.sort(np.round(rng.uniform(0, 0.02, N), 5))      # rounding creates exact ties
    k = rng.integers(1, n + 1, N)
    nn = np.full(N, n)
    from ballermixplus_amd import synth
    from ballermixplus_amd.hostmodel import Grids
    spect = {(a, b): f for a, b, f in synth.spect_from_counts(np.concatenate([k, np.arange(1, n + 1)]),
                                                               np.full(N + n, n))}
    grid = Grids(None, None, False, False, None, None)
    xs, ab, As = grid.scan_order()
    model = eng.ModelArrays('B2', 1, [n], spect, {n: 1.0}, xs, ab)
    rows = model.rows_of(k, nn)
    ctx = eng.Context(0)
    ctx.set_model(model, As)
    ctx.set_sites(gen, rows)
    tg = np.concatenate([gen[:40], [gen[0] - 1.0, gen[-1] + 1.0, 0.5 * (gen[10] + gen[11])], gen[100:110]])
    lo = np.concatenate([np.zeros(40, np.int64), [0, 0, 0], np.arange(100, 110) + 5]).astype(np.int64)
    hi = np.concatenate([np.full(40, N - 1), [N - 1, N - 1, N - 1], np.arange(100, 110) + 4]).astype(np.int64)
    hi[:5] = [0, 1, 2, 3, 4]          # tiny windows at the left edge
    ctx.set_tests(tg, lo, hi)
    ctx.scan()
    got = ctx.fetch()
    _, R = ctx.fetch_lut()
    ref = c_scan(L, R, As, gen, rows, tg, lo, hi)
    assert np.array_equal(got[4], ref[4])
    for f in (1, 2, 3):
        assert np.array_equal(got[f], ref[f])
    assert np.allclose(got[0], ref[0], rtol=1e-9, atol=1e-12)
    assert np.all(got[3][43:] == -1) and np.all(got[0][43:] == 0)      # lo > hi: empty windows
    ctx.close()


def test_abi_error_paths():
    from ballermixplus_amd import _lib, engine
    ctx = engine.Context(0)
    with pytest.raises(_lib.BmxError):
        ctx.scan()                                   # nothing set yet
    model = engine.ModelArrays('B2', 1, [10], {(k, 10): 0.1 for k in range(11)}, {10: 1.0}, [0.5], [1.0])
    ctx.set_model(model, [100.0])
    with pytest.raises(_lib.BmxError):
        ctx.set_sites([0.2, 0.1], [1, 2])            # unsorted positions
    with pytest.raises(_lib.BmxError):
        ctx.set_sites([0.1, 0.2], [1, 99])           # row outside the table
    with pytest.raises(_lib.BmxError):
        engine.Context(999)
    # a new model invalidates the site arrays set under the old one (row numbering, moment slots)
    ctx.set_sites([0.1, 0.2], [1, 2])
    ctx.set_model(model, [100.0, 1000.0])
    with pytest.raises(_lib.BmxError):
        ctx.set_tests([0.1], [0], [1])
    # ... and new sites invalidate the test sites located in the old array
    ctx.set_sites([0.1, 0.2, 0.3], [1, 2, 3])
    ctx.set_tests([0.2], [0], [2])
    ctx.scan()
    ctx.set_sites([0.1, 0.2], [1, 2])
    with pytest.raises(_lib.BmxError):
        ctx.scan()
    ctx.close()


def test_rccl_gather_path_single_rank(tmp_path):
    """The multi-GPU code path (NCCL process group, zero-copy view of the library's device
    buffers, all_gather_into_tensor, reassembly) exercised with one rank on this box: the CLI
    under BMX_FORCE_DIST=1 must write the same file as the plain single-process run."""
    import subprocess
    import sys
    from util import REPO
    argv, gold = cases.ALL_CASES['ex1_B2_w50_s25']
    outs = []
    for force in ('0', '1'):
        out = tmp_path / ('o%s.txt' % force)
        env = dict(os.environ, BMX_FORCE_DIST=force, RANK='0', WORLD_SIZE='1', LOCAL_RANK='0',
                   MASTER_ADDR='127.0.0.1', MASTER_PORT='29541')
        subprocess.run([sys.executable, os.path.join(REPO, 'BalLeRMixPlus_amd.py')] + argv + ['-o', str(out)],
                       check=True, env=env, stdout=subprocess.DEVNULL, timeout=600)
        outs.append(out.read_text())
    assert outs[0] == outs[1]
    worst, ties = cases.compare_rows(outs[1].splitlines(True)[1:], gold)
    assert worst < 1e-6 and ties == 0


@pytest.mark.parametrize('sizes,label', [((40, 50, 60), 'lds'), ((150, 160, 170), 'global-R'), ((200,), 'lds-8-wave')])
def test_multiple_sample_sizes_and_large_tables(sizes, label):
    """Ragged input: several sample sizes in one file (missing data), LUT rows = sum(n+1).
    (150,160,170) gives 483 rows = 247 KB per slice > LDS, so R is read from global memory;
    (200,) fills most of a CU's LDS and runs 8 waves per workgroup.  Dense test sites (grouped
    kernel) and strided test sites (per-site kernel) are both compared with the C oracle."""
    eng = _engine()
    L = c_oracle()
    from ballermixplus_amd.hostmodel import Grids
    rng = np.random.default_rng(11)
    N = 6000
    gen = np.cumsum(rng.geometric(1 / 60.0, N)) / 1e6
    nn = rng.choice(np.array(sizes), N)
    k = np.where(rng.random(N) < 0.6, nn, (rng.random(N) * (nn - 1)).astype(int) + 1)
    cnt = {}
    for a, b in zip(k.tolist(), nn.tolist()):
        cnt[(a, b)] = cnt.get((a, b), 0) + 1
    spect = {key: v / N for key, v in cnt.items()}
    props = {int(n): sum(v for (a, b), v in spect.items() if b == n) for n in sizes}
    grid = Grids(None, None, True, False, None, '150,400,1000,2500,6000,20000')
    xs, ab, As = grid.scan_order()
    model = eng.ModelArrays('B2', int(k.min()), sizes, spect, props, xs, ab)
    rows = model.rows_of(k, nn)
    ctx = eng.Context(0)
    ctx.set_model(model, As)
    ctx.set_sites(gen, rows)
    _, R = ctx.fetch_lut()
    Rfin = np.where(np.isfinite(R), R, 0.0)
    for idx in (np.arange(1000, 1700), np.arange(0, N, 37)):
        lo = np.zeros(len(idx), np.int64)
        hi = np.full(len(idx), N - 1, np.int64)
        ctx.set_tests(gen[idx], lo, hi)
        ctx.scan()
        got = ctx.fetch()
        ref = c_scan(L, Rfin, As, gen, rows, gen[idx], lo, hi)
        for f in (1, 2, 3, 4):
            assert np.array_equal(got[f], ref[f]), (label, f)
        assert np.allclose(got[0], ref[0], rtol=1e-9, atol=1e-12)
    ctx.close()


# kernel variants exercised by the randomised scenarios (bmx_ctx_set_variant); overridable for fuzz runs
RANDOMISED_VARIANTS = tuple(int(v) for v in os.environ.get('BMX_TEST_VARIANTS', '0,2,16,12,14,15,3,8,10').split(','))


@pytest.mark.parametrize('seed', list(range(15)))
def test_randomised_scenarios_against_oracle(seed):
    """Seeded random inputs through both kernels (grouped and per-site) vs the C oracle: random
    densities (windows from a few sites to thousands), exact position ties, several sample sizes,
    random statistic, random step, random fixed-index windows (some empty, some not containing the
    test position), off-grid and duplicated test positions, tiny and huge A values."""
    eng = _engine()
    L = c_oracle()
    from ballermixplus_amd.hostmodel import Grids
    rng = np.random.default_rng(1000 + seed)
    N = int(rng.integers(300, 4000))
    scale = 10.0 ** rng.uniform(-7.5, -4.0)
    gen = np.cumsum(rng.geometric(0.2, N)).astype(np.float64) * scale
    if seed % 3 == 0:
        gen = np.round(gen / (scale * 3)) * (scale * 3)          # exact ties
    gen = np.sort(gen)
    if seed >= 12:      # a recombination map with hot spots, cold spots and flat stretches (long runs of ties)
        rate = np.exp(rng.normal(0, 2.0, N // 50 + 1))[np.arange(N) // 50]
        rate[rng.random(N) < 0.02] = 0.0
        flat = int(rng.integers(0, max(1, N - 400)))
        rate[flat:flat + 300] = 0.0
        gen = np.cumsum(rate * rng.geometric(0.2, N)) * scale
    sizes = tuple(sorted(set(int(v) for v in rng.choice([12, 20, 33, 50, 64], int(rng.integers(1, 4))))))
    nn = rng.choice(np.array(sizes), N)
    stat = ['B2', 'B2maf', 'B0', 'B0maf', 'B1'][seed % 5]
    if stat == 'B1':
        k = (rng.random(N) < 0.3).astype(np.int64)
    elif stat.endswith('maf'):
        lo_k = 1 if stat == 'B0maf' else 0
        k = np.array([rng.integers(lo_k, n // 2 + 1) for n in nn])
    else:
        hi_k = nn - 1 if stat == 'B0' else nn
        k = np.array([rng.integers(1, h + 1) for h in hi_k])
    cnt = {}
    for a, b in zip(k.tolist(), nn.tolist()):
        cnt[(a, b)] = cnt.get((a, b), 0) + 1
    spect = {key: v / N for key, v in cnt.items()}
    props = {int(n): sum(v for (a, b), v in spect.items() if b == n) for n in sizes}
    listA = ','.join(repr(float(v)) for v in 10.0 ** rng.uniform(0.5, 9.0, int(rng.integers(2, 9))))
    grid = Grids(None, None, bool(seed % 2), False, None, listA)
    xs, ab, As = grid.scan_order()
    minc = int(k[k > 0].min()) if stat.endswith('maf') else (1 if stat == 'B1' else int(k.min()))
    model = eng.ModelArrays(stat, minc, sizes, spect, props, xs, ab)
    rows = model.rows_of(k, nn)
    ctx = eng.Context(0)
    ctx.set_model(model, As)
    ctx.set_sites(gen, rows)
    _, R = ctx.fetch_lut()
    Rfin = np.where(np.isfinite(R), R, 0.0)
    step = int(rng.integers(1, 4))
    idx = np.arange(0, N, step)
    tg = gen[idx].copy()
    off = rng.random(len(tg)) < 0.1
    tg[off] += scale * 0.37                                          # off-grid test positions
    tg = np.sort(np.concatenate([tg, tg[:5]]))                       # duplicated test positions
    M = len(tg)
    mode = seed % 4
    if mode == 0:
        lo, hi = np.zeros(M, np.int64), np.full(M, N - 1, np.int64)
    else:
        c = np.searchsorted(gen, tg)
        r = int(rng.integers(1, 200))
        lo = np.maximum(c - r, 0).astype(np.int64)
        hi = np.minimum(c + r + 1, N - 1).astype(np.int64)
        if mode == 2:
            lo = np.minimum(lo + rng.integers(0, 2 * r, M), N - 1)   # ragged, sometimes empty, sometimes past the test site
        if mode == 3:
            hi = np.maximum(hi - rng.integers(0, 2 * r, M), 0)
    ref = c_scan(L, Rfin, As, gen, rows, tg, lo, hi)
    for variant in RANDOMISED_VARIANTS:
        ctx.set_variant(variant)
        ctx.set_tests(tg, lo, hi)
        ctx.scan()
        got = ctx.fetch()
        # exact integer fields, except grid points tied within rounding noise (saturated tables)
        same = (got[1] == ref[1]) & (got[2] == ref[2]) & (got[3] == ref[3])
        assert np.array_equal(got[4][same], ref[4][same]), (seed, variant)
        assert np.allclose(got[0], ref[0], rtol=1e-9, atol=1e-12), (seed, variant)
        # A different argmax is legitimate only as a TIE: the two grid points' T agree to rounding
        # noise (saturated tables -- B_1's two rows, alpha_beta >= 1e6 at small n -- make many grid
        # points coincide).  Checked against the device's own likelihood surface of that test site.
        for t in np.nonzero(~same)[0][:6]:
            assert got[3][t] >= 0 and ref[3][t] >= 0, (seed, variant, t)
            Ts, _ = ctx.surface(tg[t], lo[t], hi[t])
            Tg, Tr = Ts[got[3][t], got[1][t], got[2][t]], Ts[ref[3][t], ref[1][t], ref[2][t]]
            assert abs(Tg - Tr) <= 1e-9 * abs(Tr) + 1e-12, (seed, variant, t, Tg, Tr)
            assert abs(got[0][t] - Tg) <= 1e-9 * abs(Tg) + 1e-12
    ctx.close()


SURF = sorted(glob.glob(os.path.join(GOLD, 'surface_*.npz')))


@pytest.mark.parametrize('path', SURF, ids=[os.path.basename(p)[8:-4] for p in SURF])
def test_device_likelihood_surface_matches_reference(path):
    """Every grid point, not just the maximum: T[A,x,a] from the device (bmx_ctx_surface) against the
    reference's calcBaller called once per grid point (tests/golden/surface_*.npz), and the scan
    kernel's maximum against the maximum of that surface."""
    eng = _engine()
    z = np.load(path)
    key = 'ex1_B2' if 'ex1_B2' in os.path.basename(path) else 'ex2_B2maf_findBal'
    argv = cases.ALL_CASES[key][0]
    opt, case, ts = cases.host_side(argv)
    sel = eng.NormalizedBetaBinom(case.data, case.grid, opt.nofreq, opt.MAF, opt.nosub).bind(case.neut)
    s = int(z['site'])
    T, ns = sel.ctx.surface(case.data.genPos[s], 0, case.data.numSites - 1)
    ref = z['T']
    pos = ~np.isnan(ref)                         # the reference reports a value only where T > 0
    assert np.all((T[~pos] <= 0) | np.isnan(T[~pos]))
    assert np.max(np.abs(T[pos] - ref[pos]) / np.abs(ref[pos])) < 1e-9
    has = pos.any(axis=(1, 2))
    assert np.array_equal(ns[has], z['nsites'][has])
    clr, ix, ia, iA, n = eng.scan_batch(sel, [case.data.genPos[s]], [0], [case.data.numSites - 1])
    flat = np.where(np.isnan(T), -np.inf, T).reshape(-1)
    best = int(np.argmax(flat))                  # first maximum in (A, x, a) order
    assert flat[best] > 0 and abs(clr[0] - flat[best]) <= 1e-12 * flat[best]
    nx, nab = len(case.xs), len(case.abetas)
    assert (int(iA[0]), int(ix[0]), int(ia[0])) == (best // (nx * nab), (best // nab) % nx, best % nab)


def test_fallback_paths_extreme_table_and_unsorted_tests():
    """(i) A neutral probability of 1e-25 makes R ~ 1e24: too wide for block-wise exponent extraction,
    the library must fall back to the per-site kernel and still agree with the oracle;
    (ii) test positions given in descending order (not what any Scan mode produces, but the ABI
    allows it) must give the same rows as the ascending call."""
    eng = _engine()
    L = c_oracle()
    from ballermixplus_amd.hostmodel import Grids
    rng = np.random.default_rng(9)
    N, n = 2500, 30
    gen = np.cumsum(rng.geometric(0.3, N)) * 2e-6
    k = rng.integers(1, n + 1, N)
    k[::50] = 7
    nn = np.full(N, n)
    cnt = {}
    for a in k.tolist():
        cnt[(a, n)] = cnt.get((a, n), 0) + 1
    spect = {key: v / N for key, v in cnt.items()}
    spect[(7, n)] = 1e-25                                  # (checksum of the helper file is not the library's business)
    grid = Grids(None, None, False, False, None, '200,1000,5000')
    xs, ab, As = grid.scan_order()
    model = eng.ModelArrays('B2', 1, [n], spect, {n: 1.0}, xs, ab)
    rows = model.rows_of(k, nn)
    ctx = eng.Context(0)
    ctx.set_model(model, As)
    ctx.set_sites(gen, rows)
    _, R = ctx.fetch_lut()
    assert np.nanmax(R) > 1e20
    Rfin = np.where(np.isfinite(R), R, 0.0)
    idx = np.arange(0, N, 2)
    lo, hi = np.zeros(len(idx), np.int64), np.full(len(idx), N - 1, np.int64)
    ref = c_scan(L, Rfin, As, gen, rows, gen[idx], lo, hi)
    ctx.set_tests(gen[idx], lo, hi)
    ctx.scan()
    got = ctx.fetch()
    for f in (1, 2, 3, 4):
        assert np.array_equal(got[f], ref[f])
    assert np.allclose(got[0], ref[0], rtol=1e-9, atol=1e-12)
    # (ii) descending test order
    ctx.set_tests(gen[idx][::-1].copy(), lo, hi)
    ctx.scan()
    rev = ctx.fetch()
    for a, b in zip(got, rev):
        assert np.array_equal(a, b[::-1])
    ctx.close()


def test_more_than_65535_lut_rows():
    """221 distinct sample sizes (300..520): 90 831 LUT rows, 4-byte row indices, R from global
    memory.  A handful of test sites against the C oracle."""
    eng = _engine()
    L = c_oracle()
    from ballermixplus_amd.hostmodel import Grids
    rng = np.random.default_rng(21)
    sizes = tuple(range(300, 521))
    N = 3000
    gen = np.cumsum(rng.geometric(0.02, N)) / 1e6
    nn = rng.choice(np.array(sizes), N)
    k = np.where(rng.random(N) < 0.5, nn, (rng.random(N) * (nn - 1)).astype(int) + 1)
    cnt = {}
    for a, b in zip(k.tolist(), nn.tolist()):
        cnt[(a, b)] = cnt.get((a, b), 0) + 1
    spect = {key: v / N for key, v in cnt.items()}
    props = {}
    for (a, b), v in spect.items():
        props[b] = props.get(b, 0.0) + v
    for n in sizes:
        props.setdefault(n, 1e-9)
    grid = Grids('0.3', None, True, False, None, '300,2000')
    xs, ab, As = grid.scan_order()
    model = eng.ModelArrays('B2', 1, sizes, spect, props, xs, ab)
    assert model.rows > 65535
    rows = model.rows_of(k, nn)
    ctx = eng.Context(0)
    ctx.set_model(model, As)
    ctx.set_sites(gen, rows)
    _, R = ctx.fetch_lut()
    Rfin = np.where(np.isfinite(R), R, 0.0)
    idx = np.arange(1000, 1100)
    lo, hi = np.zeros(len(idx), np.int64), np.full(len(idx), N - 1, np.int64)
    ctx.set_tests(gen[idx], lo, hi)
    ctx.scan()
    got = ctx.fetch()
    ref = c_scan(L, Rfin, As, gen, rows, gen[idx], lo, hi)
    for f in (1, 2, 3, 4):
        assert np.array_equal(got[f], ref[f])
    assert np.allclose(got[0], ref[0], rtol=1e-9, atol=1e-12)
    ctx.close()


def test_partial_last_group_costs_nothing_extra():
    """Performance guard: a test-site count that is not a multiple of the group size used to make
    the padding lanes of the last group walk left to index 0 (seconds on a long chromosome).  The
    kernel time for M = 16k + 5 must stay within 30 % of M = 16k, and strided scans must not fall
    off a cliff."""
    eng = _engine()
    N, n = 400000, 100
    phys, gen, k, nn, spect, props, grid = _synth_case(N, n)
    xs, ab, As = grid.scan_order()
    model = eng.ModelArrays('B2', int(k.min()), [n], spect, props, xs, ab)
    ctx = eng.Context(0)
    ctx.set_model(model, As)
    ctx.set_sites(gen, model.rows_of(k, nn))
    times = {}
    for M in (16384, 16384 + 5):
        idx = np.arange(N - M, N)                       # the LAST sites of the chromosome: longest left walk
        ctx.set_tests(gen[idx], np.zeros(M, np.int64), np.full(M, N - 1, np.int64))
        ctx.scan(); ctx.sync()
        ctx.scan(); ctx.sync()
        times[M] = ctx.last_scan_ms()
    assert times[16384 + 5] < 1.3 * times[16384] + 1.0, times
    per_window = {}
    for step in (1, 12, 40):
        idx = np.arange(0, N, step)[:8000]
        ctx.set_tests(gen[idx], np.zeros(len(idx), np.int64), np.full(len(idx), N - 1, np.int64))
        ctx.scan(); ctx.sync()
        per_window[step] = ctx.last_scan_ms() / len(idx)
    assert per_window[12] < 6 * per_window[1] and per_window[40] < 8 * per_window[1], per_window
    ctx.close()


@pytest.mark.parametrize('stat,nosub,spread', [('B2', False, 0), ('B0', True, 0), ('B1', False, 0), ('B2', False, 30)])
def test_far_field_moments_against_exact_products(stat, nosub, spread):
    """The default kernel sums far-field sites (alpha*|R| <= 0.03) as per-row moments of the log1p
    series to 8th order; variant 10 multiplies every factor 1 + alpha*R.  Same argmax and nSites on
    every window, CLR equal to 1e-11 relative (bound in DESIGN.md: 2e-15 per site at the threshold),
    for data with and without substitutions, for the two-row B_1 table and for 31 sample sizes (a
    table too large for LDS: R from L2, 254 moment slots); J = 16, 8 and 4."""
    eng = _engine()
    from ballermixplus_amd import synth
    from ballermixplus_amd.hostmodel import Grids
    N, n = 300000, 100
    phys, gen, k, nn = synth.synth_chromosome(N, n, 3)
    if nosub:
        keep = k < n
        gen, k, nn = gen[keep], k[keep], nn[keep]
        N = len(gen)
    sizes, props = [n], {n: 1.0}
    if spread:                                          # missing data: sample sizes n-spread..n, counts rescaled
        rng = np.random.default_rng(5)
        n2 = rng.integers(n - spread, n + 1, N)
        k = np.where(k == nn, n2, np.maximum(1, np.minimum(n2 - 1, (k * n2) // nn)))
        nn = n2
        sizes = sorted(set(nn.tolist()))
    if stat == 'B1':
        k = (k < n).astype(np.int64)                    # 1 = polymorphic, 0 = substitution
        cnt = {(int(a), n): float(np.mean(k == a)) for a in (0, 1)}
        minc = 1
    else:
        cnt = {(a, b): f for a, b, f in synth.spect_from_counts(k, nn)}
        minc = int(k.min())
    if spread:
        props = {int(s_): float(sum(f for (a, b), f in cnt.items() if b == s_)) for s_ in sizes}
    grid = Grids(None, None, False, False, None, None)
    xs, ab, As = grid.scan_order()
    model = eng.ModelArrays(stat, minc, sizes, cnt, props, xs, ab)
    ctx = eng.Context(0)
    ctx.set_model(model, As)
    ctx.set_sites(gen, model.rows_of(k, nn))
    for step, M in ((1, 4096), (7, 2048), (40, 1024)):
        idx = (N // 3 + step * np.arange(M)).astype(np.int64)
        lo, hi = np.zeros(M, np.int64), np.full(M, N - 1, np.int64)
        out = {}
        for variant in (10, 0):
            ctx.set_variant(variant)
            ctx.set_tests(gen[idx], lo, hi)
            ctx.scan()
            out[variant] = [a.copy() for a in ctx.fetch()]
        same = np.ones(M, bool)
        for f in (1, 2, 3):
            same &= out[0][f] == out[10][f]
        # the two-row B_1 table has grid points tied to rounding (see cases.compare_rows): there the two
        # forms may pick different ends of a tie, with the same CLR
        # (CLR is compared on EVERY window below; a few per cent of B_1's windows are such ties)
        assert same.all() or (stat == 'B1' and same.mean() > 0.95), (stat, step, same.mean())
        assert np.array_equal(out[0][4][same], out[10][4][same]), (stat, step)
        assert np.allclose(out[0][0], out[10][0], rtol=1e-11, atol=1e-13), (stat, step)
    ctx.close()


def test_grouped_kernel_at_config3_scale_against_the_reference():
    """The shipped (grouped, J = 16) kernel vs the REFERENCE at full config-3 size: each of the 250
    sites the reference scanned (tests/golden/synth/synth_1M_step4000.tsv, reference run with -s 4000)
    is embedded in a run of 16 consecutive test sites, so that it goes through a full group with bulk
    zones, pairs/quads and ragged ends -- not through the per-site kernel the strided scan uses."""
    path = os.path.join(GOLD, 'synth', 'synth_1M_step4000.tsv')
    if not os.path.exists(path):
        pytest.skip('fixture not generated')
    eng = _engine()
    N, n = 1000000, 100
    phys, gen, k, nn, spect, props, grid = _synth_case(N, n)
    xs, ab, As = grid.scan_order()
    model = eng.ModelArrays('B2', int(k.min()), [n], spect, props, xs, ab)
    ctx = eng.Context(0)
    ctx.set_model(model, As)
    ctx.set_sites(gen, model.rows_of(k, nn))
    ref_idx = np.arange(0, N, 4000)
    rows = read_tsv(path)
    assert len(rows) == len(ref_idx)
    off = np.arange(-5, 11)                                 # the reference site is the 6th of its group
    idx = np.clip(ref_idx[:, None] + off[None, :], 0, N - 1).reshape(-1)
    idx = np.unique(idx)
    ctx.set_tests(gen[idx], np.zeros(len(idx), np.int64), np.full(len(idx), N - 1, np.int64))
    ctx.scan()
    clr, ix, ia, iA, ns = ctx.fetch()
    where = np.searchsorted(idx, ref_idx)
    for j, r in zip(where, rows):
        assert int(r[0]) == phys[idx[j]]
        if r[3:6] == ['0.0', '0.0', '0.0']:
            assert iA[j] < 0
            continue
        assert (repr(xs[ix[j]]), repr(ab[ia[j]]), repr(As[iA[j]]), str(ns[j])) == (r[3], r[4], r[5], r[6]), (j, r)
        assert abs(clr[j] - float(r[2])) <= max(1e-9, 1e-6 * abs(float(r[2]))), (j, r, clr[j])
    ctx.close()
