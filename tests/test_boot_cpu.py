"""--boot without a GPU: the threshold table and the weights, the weighted host objective against the refinement's, one
replicate on the oracle's objective, the summary rules, both writers, and flag parsing and refusals (no context is created)."""
import glob
import math
import os
from decimal import ROUND_FLOOR, Decimal, getcontext

import numpy as np
import pytest

import cases
from util import REFT, orc, oracle_R, read_tsv

from ballermixplus_amd import boot, cli, null, refine, support
from ballermixplus_amd import scan as scanmod

EX1 = os.path.join(REFT, 'Example1_fullSweep_200kya_DAF.txt')
SPECT = os.path.join(REFT, 'HC_CEU_Neut_DAF_spect_for_B2.txt')


# ---------------------------------------------------------------------------------------------------- weights

def _thresholds(n):
    getcontext().prec = 80
    e1, c, f, out = Decimal(-1).exp(), Decimal(0), Decimal(1), []
    for k in range(n):
        if k:
            f *= k
        c += e1 / f
        out.append(int((c * (1 << 64)).to_integral_value(rounding=ROUND_FLOOR)))
    return out


def test_threshold_table_is_poisson_cdf():
    want = _thresholds(21)
    assert list(boot.THR) == want[:20] and len(boot.THR) == boot.MAX_WEIGHT == 20
    assert boot.THR[0] == 6786177901268885274 and boot.THR[1] == 13572355802537770549
    assert want[20] == (1 << 64) - 1 and all(a < b for a, b in zip(boot.THR, boot.THR[1:]))


def test_weight_at_and_around_each_threshold():
    assert boot.weight_of_hash(0) == 0
    assert boot.weight_of_hash((1 << 64) - 1) == 20
    for k, t in enumerate(boot.THR):
        assert boot.weight_of_hash(t - 1) == k
        assert boot.weight_of_hash(t) == k + 1
        assert boot.weight_of_hash(t + 1) == (k + 2 if k + 1 < 20 and t + 1 == boot.THR[k + 1] else k + 1)
    h = np.array([0, boot.THR[0] - 1, boot.THR[0], boot.THR[3], boot.THR[19] - 1, boot.THR[19], (1 << 64) - 1], dtype=np.uint64)
    assert boot.weight_of_hash(h).tolist() == [0, 0, 1, 4, 19, 20, 20]
    assert boot.weight_of_hash(h).tolist() == [boot.weight_of_hash(int(v)) for v in h]


def test_weights_are_the_documented_hash():
    K = boot.replicate_key(1, 0, 0)
    w = boot.block_weights(K, 50)
    for b in (0, 1, 17, 49):
        assert w[b] == boot.weight_of_hash(null.mix(K ^ null.mix(b)))


def test_weight_statistics():
    n = 10 ** 6
    w = boot.block_weights(boot.replicate_key(1, 0, 0), n)
    assert w.min() >= 0 and w.max() <= 20
    assert abs(w.mean() - 1.0) <= 5e-3         # five standard errors of a Poisson(1) mean at 10^6 draws
    for k in range(7):
        p = math.exp(-1.0) / math.factorial(k)
        assert abs((w == k).mean() - p) <= 5.0 * math.sqrt(p * (1.0 - p) / n), k


def test_keys_separate_replicates_files_seeds_and_the_null():
    N = 4000
    base = boot.site_weights(boot.replicate_key(1, 0, 0), N)
    for other in (boot.replicate_key(1, 1, 0), boot.replicate_key(1, 0, 1), boot.replicate_key(2, 0, 0)):
        assert not np.array_equal(base, boot.site_weights(other, N))
    keys = {boot.replicate_key(s, r, f) for s in (1, 2, 3) for r in range(8) for f in range(3)}
    assert len(keys) == 72
    for s in (0, 1, 7, 12345):
        assert boot.replicate_key(s, 0, 0) != null.replicate_key(s, 0, 0)
        assert boot.replicate_key(s, 3, 2) != null.replicate_key(s, 3, 2)
    assert boot.replicate_key(1, 0, 0) == null.replicate_key(null.mix(1 ^ boot.SEED_DOMAIN), 0, 0)


@pytest.mark.parametrize('N,B', [(10, 1), (10, 3), (64, 7), (100, 64), (5, 9)])
def test_block_structure(N, B):
    K = boot.replicate_key(5, 2, 1)
    w = boot.site_weights(K, N, B)
    nb = (N + B - 1) // B
    bw = boot.block_weights(K, nb)
    assert len(w) == N
    for i in range(N):
        assert w[i] == bw[i // B]
    assert len(w[(nb - 1) * B:]) == N - (nb - 1) * B       # the short last block
    with pytest.raises(ValueError):
        boot.site_weights(K, N, 0)


# ---------------------------------------------------------------------------------------------------- the host objective

class Window:
    """T and T_w of test site j by the oracle's selection table on a one-value grid (tests/test_refine_cpu.py's
    _objective construction)."""

    def __init__(self, case, ts, j):
        self.case, self.ts, self.j = case, ts, j
        self.m = case.oracle_model()
        self.sizes = sorted(set(int(n) for n in case.data.sampSizes))
        self.cache = {}

    def terms(self, A, x, a):
        d, case = self.case.data, self.case
        if (x, a) not in self.cache:
            self.cache[(x, a)] = oracle_R(case.stat, self.sizes, d.minCount, case.neut.spect, case.neut.sampProps, [x], [a])[0, 0]
        sub, alphas = orc.window_mask(self.m, A, self.ts.lo[self.j], self.ts.hi[self.j], self.ts.test_gen[self.j])
        return sub, alphas[sub], self.cache[(x, a)][self.m.row[sub]]

    def T(self, A, x, a):
        sub, al, R = self.terms(A, x, a)
        if len(sub) == 0:
            return -math.inf
        with np.errstate(divide='ignore', invalid='ignore'):
            return float(2.0 * np.sum(np.log1p(al * R)))

    def Tw(self, w):
        def f(A, x, a):
            sub, al, R = self.terms(A, x, a)
            return boot.weighted_T(al, R, np.asarray(w)[sub])
        return f


def test_weighted_objective_against_the_refinements():
    argv, gold = cases.ALL_CASES['ex1_B2']
    opt, case, ts = cases.host_side(list(argv))
    N = len(case.data.genPos)
    for j, pt in ((378, (5000.0, 0.25, 40.0)), (600, (1234.5, 0.3377, 7.25)), (100, (2e4, 0.5, 1e9))):
        W = Window(case, ts, j)
        assert W.Tw(np.ones(N, dtype=np.int32))(*pt) == refine._finite(W.T(*pt))
        w = boot.site_weights(boot.replicate_key(1, 0, 0), N, 7)
        sub, al, R = W.terms(*pt)
        with np.errstate(divide='ignore', invalid='ignore'):
            want = 2.0 * sum(float(w[i]) * float(np.log1p(a * r)) for i, a, r in zip(sub, al, R) if w[i] > 0)
        got = W.Tw(w)(*pt)
        assert math.isfinite(got) and abs(got - want) <= 1e-12 * abs(want)
        assert W.Tw(np.zeros(N, dtype=np.int32))(*pt) == -math.inf
        z = w.copy()
        z[sub] = 0                                     # positive weights outside the window only
        assert W.Tw(z)(*pt) == -math.inf
    assert boot.weighted_T([0.5, 0.5], [math.nan, 1.0], [0, 2]) == 4.0 * math.log1p(0.5)      # weight 0: nothing, whatever its term
    assert boot.weighted_T([0.5, 0.5], [-3.0, 1.0], [1, 2]) == -math.inf                       # a sum that is not finite


# ---------------------------------------------------------------------------------------------------- one replicate

@pytest.mark.parametrize('name,rows', [('ex1_B2', (378, 600)), ('ex2_B2', (592, 900)), ('ex2_B2maf', (700,))])
def test_replicate_on_oracle(name, rows):
    argv, gold = cases.ALL_CASES[name]
    opt, case, ts = cases.host_side(list(argv))
    st = refine.Setup(case.As, case.xs, case.abetas)
    ref = read_tsv(gold)
    N = len(case.data.genPos)
    for j in rows:
        r = ref[j]
        grid = (float(r[5]), float(r[3]), float(r[4]))
        W = Window(case, ts, j)
        out = refine.refine_window(W.T, st, *grid, float(r[2]))
        nat = out[1:4]
        for rep, B in ((0, 1), (1, 16)):
            Tw = W.Tw(boot.site_weights(boot.replicate_key(1, rep, 0), N, B))
            seen = []
            res = boot.replicate(lambda A, x, a: seen.append((A, x, a)) or Tw(A, x, a), st, grid, nat)
            assert seen[0] == tuple(nat)                               # starts at the refined point
            assert res['T_centre'] == Tw(*nat) and res['ok']
            assert res['T'] == Tw(res['A'], res['x'], res['abeta'])
            assert res['T'] - res['T_centre'] >= 0
            assert res['rounds'] < refine.MAX_ROUNDS
            # a compass-local optimum of T_w at the last steps that were tried
            c0, nat0, h0 = support.centre(st, grid, nat)
            f = refine.coord_objective(Tw, c0, nat0)
            c, Tc, rounds, h = refine.compass(f, c0, st.free, st.lo, st.hi, h0)
            assert refine.natural_of(c, c0, nat0) == (res['A'], res['x'], res['abeta']) and Tc == res['T']
            for d in range(6):
                k = d // 2
                v = min(max(c[k] + 2 * h[k] if d & 1 else c[k] - 2 * h[k], st.lo[k]), st.hi[k])
                if v != c[k]:
                    assert f(c[:k] + (v,) + c[k + 1:]) <= Tc


def test_replicate_keeps_fixed_coordinates():
    argv = cases.ALL_CASES['ex2_B2'][0] + ['--fixX', '0.3', '--listA', '900']
    opt, case, ts = cases.host_side(list(argv))
    st = refine.Setup(case.As, case.xs, case.abetas)
    assert st.free == (False, False, True)
    W = Window(case, ts, 592)
    grid = (900.0, 0.3, 1e6)
    out = refine.refine_window(W.T, st, *grid, W.T(*grid))
    Tw = W.Tw(boot.site_weights(boot.replicate_key(3, 0, 0), len(case.data.genPos), 4))
    seen = []
    res = boot.replicate(lambda A, x, a: seen.append((A, x, a)) or Tw(A, x, a), st, grid, out[1:4])
    assert all(p[0] == 900.0 and p[1] == 0.3 for p in seen)
    assert (res['A'], res['x']) == (900.0, 0.3)


# ---------------------------------------------------------------------------------------------------- summary

def test_summary_order_statistics():
    rng = np.random.default_rng(3)
    for n, L in ((2, 0.95), (8, 0.95), (20, 0.9), (64, 0.95), (100, 0.5), (101, 0.99)):
        x = rng.uniform(0.1, 0.4, n)
        A = np.exp(rng.uniform(5, 9, n))
        ab = np.exp(rng.uniform(0, 3, n))
        Tc = rng.uniform(10, 20, n)
        T = Tc + rng.uniform(0, 2, n)
        s = boot.summarise(A, x, ab, T, Tc, (True, True, True), L)
        klo, khi, kq = max(math.ceil(round((1 - L) / 2 * n, 9)), 1), math.ceil(round((1 + L) / 2 * n, 9)), math.ceil(round(L * n, 9))
        for k, v in enumerate((A, x, ab)):
            assert s['lo'][k] == np.sort(v)[klo - 1] and s['hi'][k] == np.sort(v)[khi - 1]
        assert s['sd'][1] == float(np.std(np.sort(x), ddof=1))
        assert abs(s['sd'][0] - np.std(np.log(A), ddof=1)) < 1e-12 and abs(s['sd'][2] - np.std(np.log(ab), ddof=1)) < 1e-12
        assert s['dT_q'] == np.sort(T - Tc)[kq - 1] and s['n_ok'] == n
    # the ranks themselves: n = 8, L = 0.95 -> 1st and 8th; n = 100, L = 0.9 -> 5th and 95th, dT at the 90th
    v = np.arange(1.0, 101.0)
    s = boot.summarise(v, v / 200, v, v, np.zeros(100), (True, True, True), 0.9)
    assert (s['lo'][0], s['hi'][0], s['dT_q']) == (5.0, 95.0, 90.0)
    s = boot.summarise(v[:8], v[:8] / 200, v[:8], v[:8], np.zeros(8), (True, True, True), 0.95)
    assert (s['lo'][0], s['hi'][0], s['dT_q']) == (1.0, 8.0, 8.0)


def test_summary_na_rules():
    one = np.array([1.0, 2.0, 3.0])
    s = boot.summarise(one, one / 10, one, np.array([5.0, -np.inf, -np.inf]), one, (True, True, True))
    assert s['n_ok'] == 1 and all(v != v for v in s['lo'] + s['hi'] + s['sd'] + [s['dT_q']])
    s = boot.summarise(one, one / 10, one, np.full(3, -np.inf), one, (True, True, True))
    assert s['n_ok'] == 0 and s['dT_q'] != s['dT_q']
    # a fixed coordinate has NA ends; non-finite replicates are left out and counted out of n_ok
    A = np.array([100.0, 1e9, 200.0, 300.0])
    x = np.full(4, 0.3)
    T = np.array([7.0, np.nan, 8.0, 9.0])
    s = boot.summarise(A, x, A, T, T - 1.0, (True, False, True), 0.5)
    assert s['n_ok'] == 3 and s['lo'][1] != s['lo'][1] and s['hi'][1] != s['hi'][1] and s['sd'][1] != s['sd'][1]
    assert (s['lo'][0], s['hi'][0]) == (100.0, 300.0) and s['dT_q'] == 1.0
    assert abs(s['sd'][0] - np.std(np.log([100.0, 200.0, 300.0]), ddof=1)) < 1e-15


# ---------------------------------------------------------------------------------------------------- writers

def _ts_with_na():
    ts = scanmod.TestSites()
    ts.add(100, 1e-4, 1e-4, 0, 5)
    ts.add_na('200\t2e-4\t0\tNA\tNA\tNA\t0\n')
    ts.add(300, 3e-4, 3e-4, 0, 5)
    ts.add(400, 4e-4, 4e-4, 0, 5)
    return ts


def _res(windows, R):
    n = len(windows)
    return {'window': np.array(windows, dtype=np.int32), 'rounds': np.full((n, R), 9, dtype=np.int32),
            'A': np.zeros((n, R)), 'x': np.zeros((n, R)), 'abeta': np.zeros((n, R)), 'T': np.zeros((n, R)),
            'T_centre': np.zeros((n, R))}


def test_writers_with_na_rows(tmp_path):
    ts = _ts_with_na()
    main = tmp_path / 'o.txt'
    main.write_text(scanmod.HEADER + '100\t0.0001\t12.5\t0.25\t40\t1000\t77\n200\t2e-4\t0\tNA\tNA\tNA\t0\n'
                    '300\t0.0003\t0.0\t0.0\t0.0\t0.0\t0.0\n400\t0.0004\t3.25\t0.5\t1000000000.0\t900\t12\n')
    res = _res([0, 2], 4)
    res['A'][0] = (1000.0, 2000.0, 500.0, 4000.0)
    res['x'][0] = (0.25, 0.5, 0.125, 0.375)
    res['abeta'][0] = (8.0, 4.0, 2.0, 16.0)
    res['T'][0] = (13.0, 14.0, 15.0, 16.0)
    res['T_centre'][0] = (12.0, 13.5, 13.0, 15.75)
    res['A'][1] = 900.0                         # A fixed; one replicate not ok
    res['x'][1] = (0.5, 0.25, 0.375, 0.4375)
    res['abeta'][1] = (1.0, 2.0, 4.0, 3.0)
    res['T'][1] = (3.5, -np.inf, 4.0, 3.75)
    res['T_centre'][1] = (3.0, -np.inf, 3.0, 3.0)
    out = tmp_path / 'o.txt.boot.txt'
    boot.write_boot(str(out), str(main), ts, np.array([13.0625, 0.0, 3.25]), res, (True, True, True), 0.5)
    got = out.read_text().splitlines(True)
    sd = lambda v: repr(float(np.std(v, ddof=1)))
    assert got[0] == boot.HEADER
    assert got[1] == '\t'.join(['100', '0.0001', '13.0625', '0.125', '0.375', '2.0', '8.0', '500.0', '2000.0',
                                sd([0.125, 0.25, 0.375, 0.5]), sd(np.log([2.0, 4.0, 8.0, 16.0])),
                                sd(np.log([500.0, 1000.0, 2000.0, 4000.0])), '0.5', '4']) + '\n'   # dT sorted: 0.25, 0.5, 1.0, 2.0; rank ceil(0.5 * 4) = 2
    assert got[2] == '200\t2e-4' + '\tNA' * 12 + '\n'
    assert got[3] == '300\t0.0003' + '\tNA' * 12 + '\n'
    boot.write_boot(str(out), str(main), ts, np.array([13.0625, 0.0, 3.25]), res, (False, True, True), 0.5)
    got = out.read_text().splitlines(True)
    assert got[4] == '\t'.join(['400', '0.0004', '3.25', '0.375', '0.5', '1.0', '4.0', 'NA', 'NA',      # n_ok = 3, L = 0.5: ranks ceil(0.75) = 1 and ceil(2.25) = 3
                                sd([0.375, 0.4375, 0.5]), sd(np.log([1.0, 3.0, 4.0])), 'NA', '0.75', '3']) + '\n'
    reps = tmp_path / 'o.txt.boot.reps.txt'
    boot.write_reps(str(reps), str(main), ts, res)
    lines = reps.read_text().splitlines(True)
    assert lines[0] == boot.REPS_HEADER and len(lines) == 1 + 8
    assert lines[1] == '100\t0.0001\t0\t13.0\t0.25\t8.0\t1000.0\t9\n'
    assert lines[6] == '400\t0.0004\t1\t-inf\t0.25\t2.0\t900.0\t9\n'
    back = boot.read_reps(str(reps))
    assert sorted(back) == [('100', '0.0001'), ('400', '0.0004')]
    assert np.array_equal(back[('400', '0.0004')]['T'], res['T'][1]) and np.array_equal(back[('100', '0.0001')]['A'], res['A'][0])
    assert boot.output_name('a/b.txt') == 'a/b.txt.boot.txt' and boot.reps_name('a/b.txt') == 'a/b.txt.boot.reps.txt'


def test_writers_without_na_rows_and_below_two_ok(tmp_path):
    ts = scanmod.TestSites()
    ts.add_many(np.array([1, 2]), np.array([1e-6, 2e-6]), np.array([1e-6, 2e-6]), np.array([0, 0]), np.array([1, 1]))
    main = tmp_path / 'o.txt'
    main.write_text(scanmod.HEADER + '1\t1e-06\t5.0\t0.3\t5\t900\t3\n2\t2e-06\t6.0\t0.3\t5\t900\t3\n')
    res = _res([1], 2)
    res['T'][0] = (6.0, -np.inf)
    boot.write_boot(str(tmp_path / 'b.txt'), str(main), ts, np.array([5.0, 6.5]), res, (True, True, True))
    assert (tmp_path / 'b.txt').read_text() == boot.HEADER + '1\t1e-06' + '\tNA' * 12 + '\n' \
        '2\t2e-06\t6.5' + '\tNA' * 10 + '\t1\n'


def test_writers_without_test_sites(tmp_path):
    ts = scanmod.TestSites()
    ts.add_na('5\t5e-06\t0\tNA\tNA\tNA\t0\n')
    main = tmp_path / 'o.txt'
    main.write_text(scanmod.HEADER + '5\t5e-06\t0\tNA\tNA\tNA\t0\n')
    boot.boot_and_write(None, str(main), ts, 8, 1, 1, 0.95, 0.0, 0, True)
    assert (tmp_path / 'o.txt.boot.txt').read_text() == boot.HEADER + '5\t5e-06' + '\tNA' * 12 + '\n'
    assert (tmp_path / 'o.txt.boot.reps.txt').read_text() == boot.REPS_HEADER


# ---------------------------------------------------------------------------------------------------- flags

def test_flags_off_by_default_and_parsed():
    opt = cli.build_parser().parse_args(['-i', EX1, '--spect', SPECT])
    assert opt.boot == 0 and not opt.bootReps and cli.boot_refusal(opt) is None
    assert opt.bootSeed is None and opt.bootBlock is None and opt.bootLevel is None and opt.bootMin is None
    opt = cli.build_parser().parse_args(['-i', EX1, '--spect', SPECT, '-o', 'o', '--refine', '--support', '--nullPerm', '3',
                                         '--boot', '100', '--bootSeed', '7', '--bootBlock', '64', '--bootLevel', '0.9',
                                         '--bootMin', '12.5', '--bootReps'])
    assert (opt.boot, opt.bootSeed, opt.bootBlock, opt.bootLevel, opt.bootMin, opt.bootReps) == (100, 7, 64, 0.9, 12.5, True)
    assert cli.refine_refusal(opt) is None and cli.support_refusal(opt) is None and cli.boot_refusal(opt) is None


@pytest.mark.parametrize('extra,env,word', [
    (['--boot', '8', '-o', 'OUT'], {}, '--boot'),                                   # needs --refine
    (['--boot', '8', '--refine'], {}, '-o'),
    (['--boot', '8', '--refine', '-o', 'OUT', '--getSpect'], {}, '--getSpect'),
    (['--boot', '8', '--refine', '-o', 'OUT', '--getConfig'], {}, '--getConfig'),
    (['--boot', '8', '--refine', '-o', 'OUT'], {'WORLD_SIZE': '2'}, 'multi-rank'),
    (['--boot', '1', '--refine', '-o', 'OUT'], {}, '--boot'),
    (['--boot', '-3', '--refine', '-o', 'OUT'], {}, '--boot'),
    (['--boot', '8', '--bootBlock', '0', '--refine', '-o', 'OUT'], {}, '--bootBlock'),
    (['--boot', '8', '--bootLevel', '1', '--refine', '-o', 'OUT'], {}, '--bootLevel'),
    (['--boot', '8', '--bootLevel', '0', '--refine', '-o', 'OUT'], {}, '--bootLevel'),
    (['--boot', '8', '--bootLevel', 'nan', '--refine', '-o', 'OUT'], {}, '--bootLevel'),
    (['--boot', '8', '--bootMin', 'nan', '--refine', '-o', 'OUT'], {}, '--bootMin'),
    (['--bootSeed', '3', '--refine', '-o', 'OUT'], {}, '--bootSeed'),
    (['--bootBlock', '3', '--refine', '-o', 'OUT'], {}, '--bootBlock'),
    (['--bootLevel', '0.9', '--refine', '-o', 'OUT'], {}, '--bootLevel'),
    (['--bootMin', '3', '--refine', '-o', 'OUT'], {}, '--bootMin'),
    (['--bootReps', '--refine', '-o', 'OUT'], {}, '--bootReps'),
])
def test_refusals(extra, env, word, tmp_path, monkeypatch, capsys):
    from ballermixplus_amd import engine
    made = []
    monkeypatch.setattr(engine, 'Context', lambda *a, **k: made.append(1))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    argv = ['-i', EX1, '--spect', SPECT] + [str(tmp_path / 'o.txt') if a == 'OUT' else a for a in extra]
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 1
    said = capsys.readouterr().out
    assert word in said and '--boot' in said
    assert not made and not glob.glob(str(tmp_path / '*'))
