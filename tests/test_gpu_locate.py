"""--locate on the GPU: the device's resampled site array is exactly the host restatement's, a slot resampled on the device is
bitwise a slot given the expanded arrays with set_sites (in every scan plan), a replicate is the weighted likelihood (C oracle
on the expanded arrays, boot.weighted_T on the unexpanded ones), the per-peak reduction is an exact first-row argmax, and the
CLI writes what the API computes without changing any other output."""
import os

import numpy as np
import pytest

from util import REFT, Case, c_oracle, c_scan, orc

from ballermixplus_amd import boot, locate

pytestmark = pytest.mark.gpu

EX1 = os.path.join(REFT, 'Example1_fullSweep_200kya_DAF.txt')
EX2 = os.path.join(REFT, 'Example2_balancing_10MYA_DAF.txt')
SPECT_B2 = os.path.join(REFT, 'HC_CEU_Neut_DAF_spect_for_B2.txt')
G = '0.002'                 # --peaks of the end-to-end runs (Example 2 spans 0.05 in genPos, Example 1 0.001)
FLAGS = ['--peaks', G, '--locate', '8', '--locateBlock', '16', '--locateReps']


def _engine():
    from ballermixplus_amd import engine
    return engine


def _bits(res):
    clr, ix, ia, iA, ns = res
    return (np.asarray(clr, dtype=np.float64).view(np.uint64), ix, ia, iA, ns)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b)))


def _scan(ctx, test_gen):
    ctx.set_tests(test_gen)
    ctx.scan()
    return ctx.fetch()


def _sel(path):
    eng = _engine()
    case = Case(path, SPECT_B2)
    sel = eng.NormalizedBetaBinom(case.data, case.grid, False, False, False).bind(case.neut)
    return case, sel


def _synthetic(seed, sizes, N, p_fixed, grids, fill_props=False):
    """The synthetic inputs of tests/test_gpu_null.py: (model, As, gen, rows)."""
    eng = _engine()
    from ballermixplus_amd.hostmodel import Grids
    rng = np.random.default_rng(seed)
    gen = np.cumsum(rng.geometric(0.02, N)) / 1e6
    nn = rng.choice(np.array(sizes), N)
    k = np.where(rng.random(N) < p_fixed, nn, (rng.random(N) * (nn - 1)).astype(int) + 1)
    cnt = {}
    for a, b in zip(k.tolist(), nn.tolist()):
        cnt[(a, b)] = cnt.get((a, b), 0) + 1
    spect = {key: v / N for key, v in cnt.items()}
    props = {}
    for (a, b), v in spect.items():
        props[b] = props.get(b, 0.0) + v
    if fill_props:
        for n in sizes:
            props.setdefault(n, 1e-9)
    xs, ab, As = Grids(*grids).scan_order()
    model = eng.ModelArrays('B2', int(k.min()) if not fill_props else 1, sizes, spect, props, xs, ab)
    return model, As, gen, model.rows_of(k, nn)


def _eleven_sizes():
    """20 000 sites, 11 sample sizes: the table is read from L2."""
    sizes = list(range(90, 201, 11))
    return _synthetic(5, sizes, 20000, 0.6, (None, None, False, False, None, None))


def _four_byte_rows():
    """3 000 sites, more than 65 535 table rows: the 4-byte row array."""
    out = _synthetic(21, tuple(range(300, 521)), 3000, 0.5, ('0.3', None, True, False, None, '300,2000'), fill_props=True)
    assert out[0].rows > 65535
    return out


def _check_resampled(ctx, src, gen, rows, key, B):
    n = ctx.resample_sites(src, key, B)
    w = boot.site_weights(key, len(gen), B)
    assert n == int(w.sum()) and n > 0
    g, r = ctx.fetch_sites()
    hg, hr = locate.resampled(gen, rows, key, B)
    assert np.array_equal(g.view(np.uint64), np.asarray(hg, dtype=np.float64).view(np.uint64))
    assert np.array_equal(r, np.asarray(hr, dtype=np.int32))


# ------------------------------------------------------------------------------------------------ 1. resampling is exact

@pytest.mark.parametrize('B', [1, 7, 64])
def test_resampled_sites_are_the_host_restatement(B):
    case, sel = _sel(EX1)
    ctx = sel.ctx
    gen, rows = np.asarray(case.data.genPos), np.asarray(sel.rows)
    ctx.select_slot(1)
    for key in (locate.replicate_key(3, 0, 0), locate.replicate_key(3, 1, 2)):
        _check_resampled(ctx, 0, gen, rows, key, B)
    ctx.close()


def test_resampled_sites_with_4_byte_rows_and_several_tiles():
    model, As, gen, rows = _four_byte_rows()              # 3 000 sites: three tiles of 1 024, the last one short
    ctx = _engine().Context(0)
    ctx.set_model(model, As)
    ctx.set_sites(gen, rows)
    ctx.select_slot(1)
    for key, B in ((locate.replicate_key(4, 0, 0), 1), (locate.replicate_key(4, 1, 0), 25)):
        _check_resampled(ctx, 0, gen, rows, key, B)
    ctx.close()


def test_resample_refusals_and_the_empty_replicate():
    eng = _engine()
    case, sel = _sel(EX1)
    ctx = sel.ctx
    gen, rows = np.asarray(case.data.genPos), np.asarray(sel.rows)
    key = locate.replicate_key(1, 0, 0)
    with pytest.raises(eng._lib.BmxError) as e:
        ctx.resample_sites(0, key, 1)                     # the source is the selected slot
    assert e.value.code == -1
    ctx.select_slot(1)
    with pytest.raises(eng._lib.BmxError) as e:
        ctx.resample_sites(0, key, 0)
    assert e.value.code == -1
    with pytest.raises(eng._lib.BmxError) as e:
        ctx.resample_sites(7, key, 1)                     # a slot that was never given sites
    assert e.value.code == -5
    # a 1-site chromosome and a key (chosen on the host) under which its weight is 0
    ctx.select_slot(2)
    ctx.set_sites(gen[:1], rows[:1])
    key0 = next(k for k in (locate.replicate_key(1, r, 0) for r in range(200)) if boot.site_weights(k, 1, 1)[0] == 0)
    key2 = next(k for k in (locate.replicate_key(1, r, 0) for r in range(2000)) if boot.site_weights(k, 1, 1)[0] >= 2)
    ctx.select_slot(1)
    assert ctx.resample_sites(0, key, 16) > 0            # the slot has sites ...
    assert ctx.resample_sites(2, key0, 1) == 0           # ... and loses them
    with pytest.raises(eng._lib.BmxError) as e:
        ctx.set_tests(gen[:3])
    assert e.value.code == -5
    with pytest.raises(eng._lib.BmxError) as e:
        ctx.fetch_sites(1)
    assert e.value.code == -5
    n = ctx.resample_sites(2, key2, 1)                    # the one site, repeated
    assert n == boot.site_weights(key2, 1, 1)[0] >= 2
    g, r = ctx.fetch_sites()
    assert g.tolist() == [gen[0]] * n and r.tolist() == [rows[0]] * n
    ctx.close()


# ------------------------------------------------------------------------------------------------ 2. a replicate slot is a set_sites slot

def _fresh(model, As, gen, rows, test_gen):
    c = _engine().Context(0)
    c.set_model(model, As)
    c.set_sites(gen, rows)
    got = _scan(c, test_gen)
    plan = c.plan()
    c.close()
    return got, plan


# the plan of the OBSERVED scan at each step, as tests/test_gpu_null.py asserts it, and of the replicate's scan of the same test
# positions over the resampled array (each site stands once on average, so the forms are the same)
PLANS = {1: ((4, 16), (4, 16)), 6: ((4, 8), (4, 8)), 20: ((5, 1), (5, 1))}


@pytest.mark.parametrize('step', [1, 6, 20])
def test_replicate_slot_is_a_set_sites_slot(step):
    case, sel = _sel(EX1)
    ctx = sel.ctx
    gen, rows = np.asarray(case.data.genPos), np.asarray(sel.rows)
    tg = gen[::step]
    base = _scan(ctx, tg)
    base_plan = ctx.plan()
    assert (base_plan['mode'], base_plan['J']) == PLANS[step][0], base_plan
    for r, B in enumerate((1, 16)):
        key = locate.replicate_key(3, r, 0)
        w = boot.site_weights(key, len(gen), B)[::step]
        assert np.any(w == 0) and np.any(w >= 2)          # test positions whose own site is gone, and whose site is repeated
        ctx.select_slot(1)
        assert ctx.resample_sites(0, key, B) == len(locate.resampled(gen, rows, key, B)[0])
        got = _scan(ctx, tg)
        plan = ctx.plan()
        print('step', step, 'B', B, 'replicate plan', plan)
        hg, hr = locate.resampled(gen, rows, key, B)
        want, want_plan = _fresh(sel.model, sel.grid_A, hg, hr, tg)
        assert plan == want_plan
        assert (plan['mode'], plan['J']) == PLANS[step][1], plan
        assert _same(got, want), (step, B)
        assert not _same(got, base)
        ctx.select_slot(0)
        assert _same(ctx.fetch(), base) and ctx.plan() == base_plan
    ctx.scan()
    assert _same(ctx.fetch(), base)                       # the observed slot still scans to the same bits
    ctx.close()


def test_replicate_slot_with_eleven_sample_sizes():
    model, As, gen, rows = _eleven_sizes()
    ctx = _engine().Context(0)
    ctx.set_model(model, As)
    ctx.set_sites(gen, rows)
    idx = np.arange(0, len(gen), 3)
    tg = gen[idx]
    base = _scan(ctx, tg)
    base_plan = ctx.plan()
    assert not base_plan['use_lds']
    key = locate.replicate_key(9, 0, 0)
    w = boot.site_weights(key, len(gen), 25)[idx]
    assert np.any(w == 0) and np.any(w >= 2)
    ctx.select_slot(1)
    ctx.resample_sites(0, key, 25)
    got = _scan(ctx, tg)
    plan = ctx.plan()
    assert not plan['use_lds']
    hg, hr = locate.resampled(gen, rows, key, 25)
    want, want_plan = _fresh(model, As, hg, hr, tg)
    assert plan == want_plan and _same(got, want)
    ctx.select_slot(0)
    assert _same(ctx.fetch(), base) and ctx.plan() == base_plan
    ctx.close()


# ------------------------------------------------------------------------------------------------ 3. a replicate is the weighted likelihood

class _OracleEx2:
    """The C oracle on Example 2's replicates of the end-to-end runs (seed 1, file 0, blocks of 16), computed once for the tests
    that need it: the whole track of replicate 0 (every site a test position) is kept, and any subset of its test positions is
    served from it (a test position's result does not depend on which others are scanned with it)."""

    B = 16

    def __init__(self):
        self.case = Case(EX2, SPECT_B2)
        self.m = self.case.oracle_model()
        self.L = c_oracle()
        self.gen = np.asarray(self.case.data.genPos)
        self.key0 = locate.replicate_key(1, 0, 0)
        self.g0, self.r0 = locate.resampled(self.gen, self.m.row, self.key0, self.B)
        self.track0 = self._scan(self.g0, self.r0, self.gen)

    def _scan(self, g, r, t):
        return c_scan(self.L, self.m.R, self.case.As, g, r, t, np.zeros(len(t), np.int64), np.full(len(t), len(g) - 1, np.int64))

    def scan(self, g, r, t):
        """locate.host_locate's callable: (clr, has a grid result) of the test positions t over the site arrays (g, r)."""
        if np.array_equal(g, self.g0) and np.array_equal(r, self.r0) and np.all(np.isin(t, self.gen)):
            at = np.searchsorted(self.gen, t)
            assert np.array_equal(self.gen[at], t)                    # (sites at one position share their result)
            return self.track0[0][at], self.track0[3][at] >= 0
        o = self._scan(g, r, t)
        return o[0], o[3] >= 0


@pytest.fixture(scope='module')
def oracle_ex2():
    return _OracleEx2()


def test_replicate_is_the_weighted_likelihood(oracle_ex2):
    """One replicate track of Example 2, every site a test position, against the C oracle on the expanded arrays (tests/cases.py
    compare_rows' rule: CLR within rtol = 1e-6 with an atol = 1e-9 floor; another argmax only as a tie, the oracle's T at its
    own argmax within tie_rtol = 1e-9 of ours), and the oracle's CLR against the grid maximum of boot.weighted_T on the
    UNEXPANDED sites."""
    rtol, atol, tie_rtol = 1e-6, 1e-9, 1e-9
    case, sel = _sel(EX2)
    ctx = sel.ctx
    gen = np.asarray(case.data.genPos)
    m = oracle_ex2.m
    N = len(gen)
    key, B = oracle_ex2.key0, oracle_ex2.B
    w = boot.site_weights(key, N, B)
    assert np.any(w == 0) and np.any(w >= 2)                          # test positions whose own site is gone, or repeated
    ctx.select_slot(1)
    assert ctx.resample_sites(0, key, B) == len(oracle_ex2.g0)
    tg = gen
    M = len(tg)
    clr, ix, ia, iA, ns = _scan(ctx, tg)
    o = oracle_ex2.track0
    ties = 0
    for t in range(M):
        assert abs(clr[t] - o[0][t]) <= max(atol, rtol * abs(o[0][t])), t
        if (ix[t], ia[t], iA[t]) != (o[1][t], o[2][t], o[3][t]):
            assert abs(o[0][t] - clr[t]) <= max(atol, tie_rtol * abs(clr[t])), t
            ties += 1
        else:
            assert ns[t] == o[4][t], t
    # repetition is the weighting: ten positions spread over the rows with a result
    have = np.nonzero(o[3] >= 0)[0]
    assert len(have) >= 10
    for t in have[np.linspace(0, len(have) - 1, 10).astype(int)].tolist():
        best = 0.0
        for A in case.As:
            sub, alphas = orc.window_mask(m, A, 0, N - 1, tg[t])
            for jx in range(len(case.xs)):
                for ja in range(len(case.abetas)):
                    best = max(best, boot.weighted_T(alphas[sub], m.R[jx, ja, m.row[sub]], w[sub]))
        assert best > 0 and abs(best - o[0][t]) <= 1e-12 * abs(o[0][t]), (t, best, o[0][t])
    ctx.close()


# ------------------------------------------------------------------------------------------------ 4. the reduction is exact

def _reduce_and_compare(ctx, lo, hi, scans):
    """locate_begin + one accumulate per scan of `scans` (callables that leave a new scan in the slot) against numpy."""
    ctx.locate_begin(lo, hi, len(scans))
    want_row, want_clr = [], []
    for r, launch in enumerate(scans):
        launch()
        ctx.locate_accumulate(r)
        clr, _, _, iA, _ = ctx.fetch()
        a, v = locate.argmax_rows(clr, iA >= 0, lo, hi)
        want_row.append(a)
        want_clr.append(v)
    row, clr = ctx.fetch_locate()
    assert np.array_equal(row, np.array(want_row))
    assert np.array_equal(clr.view(np.uint64), np.array(want_clr).view(np.uint64))
    return row, clr


def test_reduction_is_an_exact_first_row_argmax():
    eng = _engine()
    case, sel = _sel(EX1)
    ctx = sel.ctx
    gen = np.asarray(case.data.genPos)
    N = len(gen)
    # 300 test positions; position 120 is scanned twice (rows 120 and 121: a plateau of two equal CLRs); the last 70 lie far
    # beyond the chromosome, where no site is inside any window: rows without a grid result
    tg = gen[100:330:1][:229].copy()
    tg = np.concatenate([tg[:121], tg[120:121], tg[121:]])
    tg = np.concatenate([tg, gen[-1] + 1.0 + np.arange(70) * 1e-6])
    M = len(tg)
    assert M == 300 and tg[120] == tg[121] and np.all(np.diff(tg) >= 0)
    with pytest.raises(eng._lib.BmxError) as e:
        ctx.locate_accumulate(0)                          # no locate_begin yet
    assert e.value.code == -5
    base = _scan(ctx, tg)
    assert np.all(base[3][230:] < 0) and base[0][120] == base[0][121] and base[3][120] >= 0
    lo = np.array([0, 50, 150, 120, 240, 200, 121, 0], dtype=np.int32)
    hi = np.array([99, 160, 150, 121, 299, 260, 130, 299], dtype=np.int32)
    #              overlap  overlap one row plateau  none  partly  plateau's second row first  everything
    ctx.locate_begin(lo, hi, 2)
    with pytest.raises(eng._lib.BmxError) as e:
        ctx.locate_accumulate(0)                          # no scan since locate_begin
    assert e.value.code == -5
    with pytest.raises(eng._lib.BmxError) as e:
        ctx.locate_accumulate(2)
    assert e.value.code == -1

    def permuted():
        ctx.permute_rows(5, 3)
        ctx.scan()

    row, clr = _reduce_and_compare(ctx, lo, hi, [ctx.scan, permuted])
    assert row[0, 2] == 150 and row[0, 4] == -1 and clr[0, 4] == 0.0 and row[0, 3] == 120 and row[0, 6] >= 121
    assert not np.array_equal(row[0], row[1])
    ctx.restore_rows()
    with pytest.raises(eng._lib.BmxError) as e:
        ctx.locate_accumulate(1)                          # every accumulate takes a new scan
    assert e.value.code == -5
    # K = 1 and K = 200
    _reduce_and_compare(ctx, np.array([7], np.int32), np.array([293], np.int32), [ctx.scan])
    rng = np.random.default_rng(8)
    a = rng.integers(0, M, 200)
    b = np.minimum(a + rng.integers(0, 150, 200), M - 1)
    row, _ = _reduce_and_compare(ctx, a.astype(np.int32), b.astype(np.int32), [ctx.scan])
    assert np.any(row < 0) and np.any(row >= 0)
    with pytest.raises(eng._lib.BmxError) as e:
        ctx.locate_begin(np.array([0], np.int32), np.array([M], np.int32), 1)
        ctx.scan()
        ctx.locate_accumulate(0)                          # a range past the slot's test sites
    assert e.value.code == -1
    ctx.close()


# ------------------------------------------------------------------------------------------------ 5. end to end

def _cli(argv):
    from ballermixplus_amd import cli
    cli.main(argv)


def _api_locate(infile, f, seed=1, step=1, R=8, B=16, sep=float(G)):
    """What --peaks G --locate R --locateBlock B writes for one file, assembled from the API calls: (lines of <out>.locate.txt,
    lines of <out>.locate.reps.txt, and for test 6 the pieces: case, union positions, lo, hi, row[R, K], clr[R, K])."""
    case, sel = _sel(infile)
    ctx = sel.ctx
    gen = np.asarray(case.data.genPos)
    tg = gen[::step]
    obs = _scan(ctx, tg)
    pk = ctx.peaks(sep)
    union, lo, hi = locate.ranges(tg, pk['row'], sep)
    rows, clrs = [], []
    ctx.select_slot(1)
    for r in range(R):
        assert ctx.resample_sites(0, locate.replicate_key(seed, r, f), B) > 0
        clr, _, _, iA, _ = _scan(ctx, tg[union])
        a, v = locate.argmax_rows(clr, iA >= 0, lo, hi)
        rows.append(a)
        clrs.append(v)
    ctx.close()
    return case, tg, obs, pk, union, lo, hi, np.array(rows), np.array(clrs)


def _expected_files(main_path, api):
    case, tg, obs, pk, union, lo, hi, row, clr = api
    col = locate.main_columns(main_path)
    out, reps = [locate.HEADER], [locate.REPS_HEADER]
    for k, a in enumerate(pk['row'].tolist()):
        s = locate.summarise(row[:, k], clr[:, k], tg[union], int(np.searchsorted(union, a)), lo[k], hi[k], 0.95)
        out.append(locate.format_row(col(a)[:3], s, lambda u: col(union[u])[:2]))
        for r in range(row.shape[0]):
            if row[r, k] >= 0:
                reps.append('\t'.join(col(a)[:2] + [str(r)] + col(union[row[r, k]])[:2] + [repr(float(clr[r, k]))]) + '\n')
    return ''.join(out), ''.join(reps)


EX2_ARGV = ['-i', EX2, '--spect', SPECT_B2]


@pytest.fixture(scope='module')
def ex2_run(tmp_path_factory):
    d = tmp_path_factory.mktemp('locate')
    out = str(d / 'l.txt')
    _cli(EX2_ARGV + ['-o', out] + FLAGS)
    return d, out, _api_locate(EX2, 0)


def test_cli_writes_what_the_api_computes(ex2_run):
    d, out, api = ex2_run
    want, want_reps = _expected_files(out, api)
    assert len(api[3]['row']) >= 2                        # several peaks, or the test says little
    assert open(out + '.locate.txt').read() == want
    assert open(out + '.locate.reps.txt').read() == want_reps
    rows = locate.read_locate(out + '.locate.txt')
    assert len(rows) == len(api[3]['row']) and all(r['n_ok'] == 8 for r in rows)


def test_cli_leaves_the_other_outputs_alone_and_repeats_itself(ex2_run):
    d, out, _ = ex2_run
    plain, again, seeded = str(d / 'p.txt'), str(d / 'a.txt'), str(d / 's.txt')
    _cli(EX2_ARGV + ['-o', plain, '--peaks', G])
    _cli(EX2_ARGV + ['-o', again] + FLAGS)
    _cli(EX2_ARGV + ['-o', seeded] + FLAGS + ['--locateSeed', '2'])
    rd = lambda p: open(p, 'rb').read()
    for suffix in ('', '.peaks.txt'):
        assert rd(out + suffix) == rd(plain + suffix) == rd(again + suffix) == rd(seeded + suffix)
    assert not os.path.exists(plain + '.locate.txt')
    for suffix in ('.locate.txt', '.locate.reps.txt'):
        assert rd(out + suffix) == rd(again + suffix)
    assert rd(out + '.locate.reps.txt') != rd(seeded + '.locate.reps.txt')


def test_cli_with_refine_boot_and_null(ex2_run):
    d, out, api = ex2_run
    more = ['--peaks', G, '--refine', '--boot', '4', '--nullPerm', '3']
    a, b = str(d / 'r0.txt'), str(d / 'r1.txt')
    _cli(EX2_ARGV + ['-o', a] + more)
    _cli(EX2_ARGV + ['-o', b] + more + FLAGS[2:])
    rd = lambda p: open(p, 'rb').read()
    for suffix in ('', '.peaks.txt', '.refined.txt', '.boot.txt', '.null.txt', '.pval.txt'):
        assert rd(a + suffix) == rd(b + suffix), suffix
    assert rd(a) == rd(out)
    for suffix in ('.locate.txt', '.locate.reps.txt'):             # the locate files of the run without these flags
        assert rd(b + suffix) == rd(out + suffix), suffix
    want, want_reps = _expected_files(b, api)
    assert open(b + '.locate.txt').read() == want and open(b + '.locate.reps.txt').read() == want_reps


def test_cli_two_files_key_each_file(ex2_run, tmp_path):
    d, one, _ = ex2_run
    out = tmp_path / 'res'
    _cli(['-i', EX1 + ',' + EX2, '--spect', SPECT_B2, '-o', str(out)] + FLAGS)
    plain = tmp_path / 'plain'
    _cli(['-i', EX1 + ',' + EX2, '--spect', SPECT_B2, '-o', str(plain), '--peaks', G])
    rd = lambda p: open(p, 'rb').read()
    for i, f in enumerate((EX1, EX2)):
        name = os.path.basename(f) + '.out.txt'
        for suffix in ('', '.peaks.txt'):
            assert rd(str(out / name) + suffix) == rd(str(plain / name) + suffix)
        want, want_reps = _expected_files(str(out / name), _api_locate(f, i))
        assert open(str(out / name) + '.locate.txt').read() == want
        assert open(str(out / name) + '.locate.reps.txt').read() == want_reps
    assert rd(str(out / 'peaks.txt')) == rd(str(plain / 'peaks.txt'))
    name = os.path.basename(EX2) + '.out.txt'
    assert rd(str(out / name)) == rd(one)                                    # the same scan ...
    assert rd(str(out / name) + '.locate.reps.txt') != rd(one + '.locate.reps.txt')      # ... other replicates: file ordinal 1


# ------------------------------------------------------------------------------------------------ 6. against the oracle alone

def test_argmax_rows_against_the_oracle(ex2_run, oracle_ex2):
    """The (peak, replicate) argmax rows of the end-to-end run on Example 2 (every site a test position) against
    locate.host_locate on the C oracle: equal rows wherever the oracle's best and second-best CLR of the range differ by more
    than 1e-9 relative, CLRs within compare_rows' rtol everywhere, at most 2 % of the pairs exempted.  (The oracle alone has no
    pair that close on this input at G = 0.002, seed 1 and blocks of 16: 0 of its 56 pairs.)"""
    d, out, api = ex2_run
    case, tg, obs, pk, union, lo, hi, row, clr = api
    assert len(pk['row']) >= 2
    keys = [locate.replicate_key(1, r, 0) for r in range(8)]
    want_row, want_clr, tracks = locate.host_locate(oracle_ex2.scan, oracle_ex2.gen, oracle_ex2.m.row, tg[union], lo, hi, keys,
                                                    oracle_ex2.B)
    reps = locate.read_reps(out + '.locate.reps.txt')
    col = locate.main_columns(out)
    exempt = 0
    for k, a in enumerate(pk['row'].tolist()):
        got = reps[tuple(col(a)[:2])]
        assert got['replicate'].tolist() == list(range(8))
        for r in range(8):
            assert row[r, k] >= 0 and want_row[r, k] >= 0
            assert got['arg_genPos'][r] == col(union[row[r, k]])[1] and got['CLR'][r] == clr[r, k]      # the file holds the API's rows
            assert abs(clr[r, k] - want_clr[r, k]) <= max(1e-9, 1e-6 * abs(want_clr[r, k])), (k, r)
            c, h = tracks[r]
            v = np.sort(c[lo[k]:hi[k] + 1][h[lo[k]:hi[k] + 1]])[::-1]
            if len(v) >= 2 and v[0] - v[1] <= 1e-9 * abs(v[0]):
                exempt += 1
            else:
                assert row[r, k] == want_row[r, k], (k, r)
    assert exempt <= 0.02 * row.size
