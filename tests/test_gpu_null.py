"""The permutation null on the GPU: the device's row permutation is bitwise the host's (ballermixplus_amd/null.py) in every
scan plan, restoring the rows restores the scan, a permuted replicate matches the C oracle, the device accumulation matches
the host's, and the CLI writes what the API computes without changing the main output."""
import os

import numpy as np
import pytest

import cases
from util import REFT, Case, c_oracle, c_scan, read_tsv

from ballermixplus_amd import null

pytestmark = pytest.mark.gpu

EX1 = os.path.join(REFT, 'Example1_fullSweep_200kya_DAF.txt')
EX2 = os.path.join(REFT, 'Example2_balancing_10MYA_DAF.txt')
SPECT_B2 = os.path.join(REFT, 'HC_CEU_Neut_DAF_spect_for_B2.txt')


def _engine():
    from ballermixplus_amd import engine
    return engine


def _bits(res):
    clr, ix, ia, iA, ns = res
    return (np.asarray(clr, dtype=np.float64).view(np.uint64), ix, ia, iA, ns)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b)))


def _scan(ctx, test_gen, lo=None, hi=None):
    ctx.set_tests(test_gen, lo, hi)
    ctx.scan()
    return ctx.fetch()


def _host_permuted(model, As, gen, rows, sig, test_gen, lo=None, hi=None):
    eng = _engine()
    c = eng.Context(0)
    c.set_model(model, As)
    c.set_sites(gen, rows[sig])
    got = _scan(c, test_gen, lo, hi)
    c.close()
    return got


def _check_plan(sel, gen, step, want_mode, want_J, blocks=(1, 7)):
    """Observed scan, then permuted replicates against set_sites(rows[sigma]), then restore."""
    ctx = sel.ctx
    rows = np.asarray(sel.rows)
    tg = gen[::step]
    base = _scan(ctx, tg)
    plan = ctx.plan()
    assert (plan['mode'], plan['J']) == (want_mode, want_J), plan
    N = len(gen)
    for r, B in enumerate(blocks):
        key = null.replicate_key(3, r, 0)
        ctx.permute_rows(key, B)
        ctx.scan()
        got = ctx.fetch()
        want = _host_permuted(sel.model, sel.grid_A, gen, rows, null.block_permutation(N, key, B), tg)
        assert _same(got, want), (step, B)
        assert not _same(got, base)
    ctx.restore_rows()
    ctx.scan()
    assert _same(ctx.fetch(), base)
    return ctx


def _ex1_sel():
    eng = _engine()
    case = Case(EX1, SPECT_B2)
    sel = eng.NormalizedBetaBinom(case.data, case.grid, False, False, False).bind(case.neut)
    return case, sel


@pytest.mark.parametrize('step,mode,J', [(1, 4, 16), (6, 4, 8), (20, 5, 1)])
def test_device_permutation_matches_host(step, mode, J):
    """Dense prepared plan (J = 16), -s 6 (J = 8) and -s 20 (one test site per wave)."""
    case, sel = _ex1_sel()
    _check_plan(sel, np.asarray(case.data.genPos), step, mode, J)
    sel.ctx.close()


def test_device_permutation_with_eleven_sample_sizes():
    """11 sample sizes (the table is read from L2), site-based windows."""
    eng = _engine()
    from ballermixplus_amd.hostmodel import Grids
    rng = np.random.default_rng(5)
    sizes = list(range(90, 201, 11))
    assert len(sizes) == 11
    N = 20000
    gen = np.cumsum(rng.geometric(0.02, N)) / 1e6
    nn = rng.choice(np.array(sizes), N)
    k = np.where(rng.random(N) < 0.6, nn, (rng.random(N) * (nn - 1)).astype(int) + 1)
    cnt = {}
    for a, b in zip(k.tolist(), nn.tolist()):
        cnt[(a, b)] = cnt.get((a, b), 0) + 1
    spect = {key: v / N for key, v in cnt.items()}
    props = {}
    for (a, b), v in spect.items():
        props[b] = props.get(b, 0.0) + v
    xs, ab, As = Grids(None, None, False, False, None, None).scan_order()
    model = eng.ModelArrays('B2', int(k.min()), sizes, spect, props, xs, ab)
    rows = model.rows_of(k, nn)
    ctx = eng.Context(0)
    ctx.set_model(model, As)
    ctx.set_sites(gen, rows)
    idx = np.arange(0, N, 3)
    lo, hi = np.maximum(0, idx - 200), np.minimum(N - 1, idx + 201)
    base = _scan(ctx, gen[idx], lo, hi)
    assert not ctx.plan()['use_lds']
    for r, B in enumerate((1, 25)):
        key = null.replicate_key(9, r, 0)
        ctx.permute_rows(key, B)
        ctx.scan()
        want = _host_permuted(model, As, gen, rows, null.block_permutation(N, key, B), gen[idx], lo, hi)
        assert _same(ctx.fetch(), want)
    ctx.restore_rows()
    ctx.scan()
    assert _same(ctx.fetch(), base)
    ctx.close()


def test_device_permutation_with_4_byte_rows():
    """More than 65 535 LUT rows: the row32 array is permuted."""
    eng = _engine()
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
    xs, ab, As = Grids('0.3', None, True, False, None, '300,2000').scan_order()
    model = eng.ModelArrays('B2', 1, sizes, spect, props, xs, ab)
    assert model.rows > 65535
    rows = model.rows_of(k, nn)
    ctx = eng.Context(0)
    ctx.set_model(model, As)
    ctx.set_sites(gen, rows)
    idx = np.arange(1000, 1100)
    lo, hi = np.zeros(len(idx), np.int64), np.full(len(idx), N - 1, np.int64)
    base = _scan(ctx, gen[idx], lo, hi)
    key = null.replicate_key(4, 0, 0)
    ctx.permute_rows(key, 1)
    ctx.scan()
    want = _host_permuted(model, As, gen, rows, null.block_permutation(N, key, 1), gen[idx], lo, hi)
    assert _same(ctx.fetch(), want)
    ctx.restore_rows()
    ctx.scan()
    assert _same(ctx.fetch(), base)
    ctx.close()


def test_two_slots_are_permuted_independently():
    """Slot 1 holds a second chromosome (Example 1's positions with its rows reversed); permuting it leaves slot 0 alone."""
    case, sel = _ex1_sel()
    ctx = sel.ctx
    gen = np.asarray(case.data.genPos)
    r1 = np.asarray(sel.rows)
    r2 = r1[::-1].copy()
    ctx.select_slot(1)
    ctx.set_sites(gen, r2)
    base2 = _scan(ctx, gen[::2])
    ctx.select_slot(0)
    base1 = _scan(ctx, gen)
    key = null.replicate_key(8, 0, 1)
    ctx.select_slot(1)
    ctx.permute_rows(key, 1)
    ctx.scan()
    ctx.select_slot(0)
    ctx.scan()
    assert _same(ctx.fetch(), base1)                    # slot 0 keeps its rows
    ctx.select_slot(1)
    want = _host_permuted(sel.model, sel.grid_A, gen, r2, null.block_permutation(len(gen), key, 1), gen[::2])
    assert _same(ctx.fetch(), want)
    assert not _same(ctx.fetch(), base2)
    ctx.restore_rows()
    ctx.scan()
    assert _same(ctx.fetch(), base2)
    ctx.close()


def _synth_input(tmp_path, name, nosub, seed):
    from ballermixplus_amd import synth
    rng = np.random.default_rng(seed)
    N, n = 4000, 40
    phys = np.cumsum(rng.geometric(1 / 300.0, N)).astype(np.int64)
    poly = rng.integers(1, n, N)
    k = poly if nosub else np.where(rng.random(N) < 0.4, n, poly)
    path = str(tmp_path / (name + '.txt'))
    synth.write_input(path, phys, phys / 1e6, k, np.full(N, n))
    return path


@pytest.mark.parametrize('stat', ['B2', 'B2maf', 'B0maf'])
def test_permuted_replicate_matches_the_oracle(stat, tmp_path):
    """One permuted replicate of a 4 000-site chromosome against the C oracle run on the host-permuted rows."""
    eng = _engine()
    from ballermixplus_amd import helpers
    MAF, nosub = stat != 'B2', stat == 'B0maf'
    inp = _synth_input(tmp_path, stat, nosub, 40 + len(stat))
    spect = str(tmp_path / (stat + '.spect'))
    helpers.getSpect(inp, spect, MAF, nosub)
    case = Case(inp, spect, MAF=MAF, nosub=nosub)
    sel = eng.NormalizedBetaBinom(case.data, case.grid, False, MAF, nosub).bind(case.neut)
    gen = np.asarray(case.data.genPos)
    N = len(gen)
    idx = np.arange(7, N, 80)
    lo, hi = np.zeros(len(idx), np.int64), np.full(len(idx), N - 1, np.int64)
    key = null.replicate_key(1, 0, 0)
    sig = null.block_permutation(N, key, 1)
    sel.ctx.set_tests(gen[idx], lo, hi)
    sel.ctx.permute_rows(key, 1)
    sel.ctx.scan()
    clr, ix, ia, iA, ns = sel.ctx.fetch()
    m = case.oracle_model()
    o = c_scan(c_oracle(), m.R, case.As, gen, np.asarray(m.row)[sig], gen[idx], lo, hi)
    assert np.array_equal(o[1], ix) and np.array_equal(o[2], ia) and np.array_equal(o[3], iA)
    assert np.array_equal(o[4], ns)
    assert np.max(np.abs(o[0] - clr) / np.maximum(np.abs(o[0]), 1e-300)) <= 1e-6
    sel.ctx.close()


def test_accumulation_matches_the_host():
    eng = _engine()
    case, sel = _ex1_sel()
    ctx = sel.ctx
    gen = np.asarray(case.data.genPos)
    obs = _scan(ctx, gen[::2])[0]
    ctx.null_begin()
    with pytest.raises(eng._lib.BmxError) as e:
        ctx.null_accumulate()                             # no replicate scanned yet
    assert e.value.code == -5
    with pytest.raises(eng._lib.BmxError) as e:
        ctx.permute_rows(1, 0)
    assert e.value.code == -1
    counts = np.zeros(len(obs), np.int64)
    for r in range(5):
        ctx.permute_rows(null.replicate_key(7, r, 0), 1 + 2 * r)
        ctx.scan()
        clr = ctx.fetch()[0]
        m = ctx.null_accumulate()
        assert m == clr.max()
        counts += clr >= obs
    got, reps = ctx.null_fetch()
    assert reps == 5 and np.array_equal(got, counts)
    ctx.set_tests(gen[::2])                               # new test sites drop the null state
    with pytest.raises(eng._lib.BmxError) as e:
        ctx.null_fetch()
    assert e.value.code == -5
    ctx.close()


def _api_null(infile, spect, R, seed, f, step=1):
    eng = _engine()
    case = Case(infile, spect)
    sel = eng.NormalizedBetaBinom(case.data, case.grid, False, False, False).bind(case.neut)
    gen = np.asarray(case.data.genPos)
    tg = gen[::step]
    sel.ctx.set_tests(tg, np.zeros(len(tg), np.int64), np.full(len(tg), len(gen) - 1, np.int64))
    sel.ctx.scan()
    got = null.run_file(sel.ctx, R, seed, 1, f)
    sel.ctx.close()
    return got


def _read_null(path):
    lines = open(path).read().splitlines()
    assert lines[0] == 'replicate\tmaxCLR'
    return [l.split('\t') for l in lines[1:]]


def test_cli_one_file(tmp_path):
    from ballermixplus_amd import cli
    argv, _ = cases.ALL_CASES['ex1_B2']
    plain, withnull = tmp_path / 'a.txt', tmp_path / 'b.txt'
    cli.main(argv + ['-o', str(plain)])
    cli.main(argv + ['-o', str(withnull), '--nullPerm', '20', '--nullSeed', '7'])
    assert plain.read_bytes() == withnull.read_bytes()
    clr, iA, counts, maxima = _api_null(EX1, SPECT_B2, 20, 7, 0)
    rows = _read_null(str(withnull) + '.null.txt')
    assert [r[0] for r in rows] == [str(i) for i in range(20)]
    assert [float(r[1]) for r in rows] == maxima.tolist()
    pv = read_tsv(str(withnull) + '.pval.txt')
    main = read_tsv(str(withnull))
    assert len(pv) == len(main) == len(clr)
    ps = np.array([float(r[3]) for r in pv])
    pg = np.array([float(r[4]) for r in pv])
    assert np.all(ps >= 1 / 21) and np.all(ps <= 1) and np.all(pg >= 1 / 21) and np.all(pg <= 1)
    assert np.array_equal(ps, null.p_site(counts, 20)) and np.array_equal(pg, null.p_genome(clr, maxima))
    assert [r[:3] for r in pv] == [r[:3] for r in main]


def test_cli_many_files_key_each_file(tmp_path):
    from ballermixplus_amd import cli
    out = tmp_path / 'res'
    cli.main(['-i', EX1 + ',' + EX2, '--spect', SPECT_B2, '-o', str(out), '-s', '3', '--nullPerm', '4', '--nullSeed', '5'])
    per = [_api_null(f, SPECT_B2, 4, 5, i, step=3) for i, f in enumerate((EX1, EX2))]
    wrong = _api_null(EX2, SPECT_B2, 4, 5, 0, step=3)         # file 1 keyed as if it were file 0
    assert not np.array_equal(wrong[3], per[1][3])
    gmax = np.maximum(per[0][3], per[1][3])
    rows = _read_null(str(out / 'null.txt'))
    assert [float(r[1]) for r in rows] == gmax.tolist()
    for f, (clr, iA, counts, _) in zip((EX1, EX2), per):
        pv = read_tsv(str(out / (os.path.basename(f) + '.out.txt.pval.txt')))
        assert np.array_equal(np.array([float(r[3]) for r in pv]), null.p_site(counts, 4))
        assert np.array_equal(np.array([float(r[4]) for r in pv]), null.p_genome(clr, gmax))
