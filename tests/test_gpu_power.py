"""--power on the GPU: the device's planted site array is the host restatement's on every site (all are decided), a planted slot
is bitwise a slot given the same arrays with set_sites, fetch_at gathers what fetch returns, the argument checks refuse without
reaching a kernel, planting separates the range maxima from the unplanted backgrounds as the oracle says it does, and the CLI
writes what the host pipeline on the oracle scan computes without changing any other output."""
import os

import numpy as np
import pytest

import powercases as pc

from ballermixplus_amd import helpers, locate, null, power, synth

pytestmark = pytest.mark.gpu


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


def _ctx(c):
    ctx = _engine().Context(0)
    ctx.set_model(c.model, c.As)
    ctx.set_sites(c.gen, c.rows)
    return ctx


def _check_planted(ctx, c, key, src_rows, tests):
    """plant_sites from slot 0 into slot 1 under key against the host restatement on the DEVICE's table; then the slot's state."""
    N = len(c.gen)
    R = ctx.fetch_lut()[1]
    ctx.select_slot(1)
    first, count, changed = ctx.plant_sites(0, key, c.centres, *c.planted, c.gw)
    g, r = ctx.fetch_sites(N)
    want, margin = c.host(key, R=R, rows=src_rows)
    redrawn = np.isfinite(margin)
    assert redrawn.sum() > 300 and np.all(margin[redrawn] > power.MARGIN)         # every site is decided
    assert np.array_equal(g.view(np.uint64), c.gen.view(np.uint64))
    assert np.array_equal(r, want)
    hf, hc = c.runs()
    assert np.array_equal(first, hf) and np.array_equal(count, hc)
    assert changed == np.count_nonzero(want != np.asarray(src_rows)) > 100
    assert ctx.plant_ms() > 0.0
    got = _scan(ctx, tests)
    plan = ctx.plan()
    ctx.select_slot(0)
    g0, r0 = ctx.fetch_sites(N)
    assert np.array_equal(g0.view(np.uint64), c.gen.view(np.uint64)) and np.array_equal(r0, np.asarray(src_rows))    # the source is read only
    ctx.select_slot(2)                                                 # the slot's state: a set_sites slot of the fetched arrays
    ctx.set_sites(g, r)
    assert _same(_scan(ctx, tests), got) and ctx.plan() == plan
    ctx.select_slot(0)
    return got


# ------------------------------------------------------------------------------------------------ 1. sampler vs host

@pytest.mark.parametrize('stat', pc.SAMPLER_STATS)
def test_planted_rows_are_the_host_restatement(stat):
    c = pc.sampler(stat)
    assert c.model.rows * 16 <= 48 << 10                               # the table is staged in LDS
    ctx = _ctx(c)
    tests = c.gen[::7]
    base = _scan(ctx, tests)
    got = _check_planted(ctx, c, pc.SAMPLER_KEY, c.rows, tests)
    assert not _same(got, base)
    if stat == 'B2':
        # the rows the source holds NOW: a permutation included
        bkey = power.background_key(7, 0, 0)
        ctx.permute_rows(bkey, 3)
        bg = c.rows[null.block_permutation(len(c.rows), bkey, 3)]
        _check_planted(ctx, c, pc.SAMPLER_KEY, bg, tests)
        ctx.restore_rows()
        # K == 0: a plain copy
        ctx.select_slot(1)
        first, count, changed = ctx.plant_sites(0, 1, np.zeros(0), *c.planted, c.gw)
        assert len(first) == 0 and changed == 0
        g, r = ctx.fetch_sites(len(c.gen))
        assert np.array_equal(g, c.gen) and np.array_equal(r, c.rows)
        assert _same(_scan(ctx, tests), base)
        ctx.select_slot(0)
        ctx.scan()
        assert _same(ctx.fetch(), base)                                # the observed slot still scans to the same bits
    ctx.close()


# ------------------------------------------------------------------------------------------------ 2. large table

def test_planted_rows_with_4_byte_rows_and_the_table_in_l2():
    c = pc.large()
    ctx = _ctx(c)
    _check_planted(ctx, c, pc.LARGE_KEY, c.rows, c.gen[1800:2200:5])
    ctx.close()


# ------------------------------------------------------------------------------------------------ 3. fetch_at

def test_fetch_at_gathers_the_scan_results():
    eng = _engine()
    c = pc.sampler('B2')
    ctx = _ctx(c)
    with pytest.raises(eng._lib.BmxError) as e:
        ctx.fetch_at([0])                                              # before a scan
    assert e.value.code == -5
    tests = np.concatenate([c.gen[::11], c.gen[-1] + 1.0 + np.arange(5) * 1e-6])       # the last five have no grid result
    clr, ix, ia, iA, ns = _scan(ctx, tests)
    M = len(tests)
    assert np.all(iA[-5:] < 0)
    rng = np.random.default_rng(2)
    idx = np.concatenate([rng.integers(0, M, 300), [-1, M - 1, 0, -1, 5, 5]]).astype(np.int32)
    rng.shuffle(idx)
    got_clr, got_lin, got_ns = ctx.fetch_at(idx)
    lin = np.where(iA >= 0, (iA.astype(np.int64) * len(c.xs) + ix) * len(c.abetas) + ia, -1)
    ok = idx >= 0
    assert np.array_equal(got_clr[ok].view(np.uint64), clr[idx[ok]].view(np.uint64))
    assert np.array_equal(got_lin[ok], lin[idx[ok]]) and np.array_equal(got_ns[ok], ns[idx[ok]])
    assert np.all(got_clr[~ok] == 0.0) and np.all(got_lin[~ok] == -1) and np.all(got_ns[~ok] == 0) and (~ok).sum() == 2
    assert all(len(a) == 0 for a in ctx.fetch_at(np.zeros(0, dtype=np.int32)))
    for bad in ([M], [-2], [0, 1, M + 7]):
        with pytest.raises(eng._lib.BmxError) as e:
            ctx.fetch_at(bad)
        assert e.value.code == -1
    ctx.close()


# ------------------------------------------------------------------------------------------------ 4. errors

def test_plant_sites_refusals():
    eng = _engine()
    c = pc.sampler('B2')
    ctx = eng.Context(0)
    E = eng._lib.BmxError
    good = (c.centres, 1, 1, 1, c.gw)

    def refused(code, *a):
        with pytest.raises(E) as e:
            ctx.plant_sites(*a)
        assert e.value.code == code, a

    ctx.model = c.model                                                # (the wrapper checks gw's length against it)
    refused(-5, 1, 1, *good)                                           # no model
    ctx.set_model(c.model, c.As)
    ctx.select_slot(1)
    refused(-5, 0, 1, *good)                                           # a source without sites
    ctx.select_slot(0)
    ctx.set_sites(c.gen, c.rows)
    with pytest.raises(E) as e:
        ctx.plant_ms()                                                 # nothing planted yet
    assert e.value.code == -5
    refused(-1, 0, 1, *good)                                           # the source is the selected slot
    ctx.select_slot(1)
    refused(-1, -1, 1, *good)
    refused(-1, 4096, 1, *good)
    refused(-5, 7, 1, *good)                                           # a slot that was never given sites
    for pt in ((-1, 1, 1), (4, 1, 1), (1, -1, 1), (1, 3, 1), (1, 1, -1), (1, 1, 3)):
        refused(-1, 0, 1, c.centres, *pt, c.gw)
    reach = power.ALPHA_CUT / c.A
    for bad in ([0.2, 0.1], [0.1, 0.1], [0.1, 0.1 + 2.0 * reach], [0.1, np.nan], [np.inf]):
        refused(-1, 0, 1, np.array(bad), 1, 1, 1, c.gw)
    L, h = ctx._L, ctx._h
    cp = eng._lib.as_dp(np.ascontiguousarray(c.centres))
    gp = eng._lib.as_dp(c.gw)
    assert L.bmx_ctx_plant_sites(h, 0, 1, -1, cp, 1, 1, 1, gp, None, None, None) == -1       # K < 0
    assert L.bmx_ctx_plant_sites(h, 0, 1, 3, None, 1, 1, 1, gp, None, None, None) == -1      # NULL centre
    assert L.bmx_ctx_plant_sites(h, 0, 1, 3, cp, 1, 1, 1, None, None, None, None) == -1      # NULL gw
    assert L.bmx_ctx_plant_sites(h, 0, 1, 0, None, 1, 1, 1, None, None, None, None) == 0     # K == 0 needs neither
    assert L.bmx_ctx_plant_sites(h, 0, 1, 3, cp, 1, 1, 1, gp, None, None, None) == 0         # the outputs may be NULL
    g, r = ctx.fetch_sites(len(c.gen))
    assert np.array_equal(r, c.host(1, R=ctx.fetch_lut()[1])[0])
    ctx.close()


# ------------------------------------------------------------------------------------------------ 5. separation

def _e2e_ctx():
    e = pc.e2e()
    eng = _engine()
    model = eng.ModelArrays('B2', e.min_count, [pc.E2E_n], e.spect, e.props, e.xs, e.abetas)
    ctx = eng.Context(0)
    ctx.set_model(model, e.As)
    ctx.set_sites(e.gen, model.rows_of(e.k, e.nn))
    return e, model, ctx


def test_planting_separates_the_range_maxima():
    """8 replicates of the end-to-end chromosome on the perm background: every range maximum after planting is at least twice the
    same range's maximum on the same permuted background without planting (tests/test_power_cpu.py establishes the factor for
    exactly these draws with the oracle)."""
    e, model, ctx = _e2e_ctx()
    tg = e.gen[e.union]
    base = _scan(ctx, e.gen[::3])
    arg, clr, lin, ns, first, count = power.run_replicates(ctx, tg, e.lo, e.hi, e.centre_pos, e.planted, e.gw, pc.E2E_SEED, pc.SEP_R)
    assert ctx.slot == 0 and np.all(arg >= 0)
    ctx.scan()
    assert _same(ctx.fetch(), base)                                    # rows restored, test sites and plan intact
    want = pc.e2e_host(True)
    assert np.array_equal(arg, want[0]) and np.array_equal(lin, want[2]) and np.array_equal(ns, want[3])
    assert np.all(np.abs(clr - want[1]) <= 1e-6 * np.abs(want[1]))
    plain = np.zeros_like(clr)
    ctx.select_slot(3)
    ctx.set_sites(e.gen, model.rows_of(e.k, e.nn))
    for r in range(pc.SEP_R):
        ctx.permute_rows(power.background_key(pc.E2E_SEED, r, 0), 1)
        c, _, _, iA, _ = _scan(ctx, tg)
        plain[r] = locate.argmax_rows(c, iA >= 0, e.lo, e.hi)[1]
    print('planted / unplanted range maxima: min %.3f' % (clr / plain).min())
    assert np.all(plain > 0.0) and np.all(clr >= 2.0 * plain)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 6. end to end

def _cli(argv):
    from ballermixplus_amd import cli
    cli.main(argv)


@pytest.fixture(scope='module')
def e2e_run(tmp_path_factory):
    d = tmp_path_factory.mktemp('power')
    e = pc.e2e()
    inp, sp = str(d / 'in.txt'), str(d / 'spect.txt')
    synth.write_input(inp, e.phys, e.gen, e.k, e.nn)
    helpers.getSpect(inp, sp, False, False)
    base = ['-i', inp, '--spect', sp] + pc.E2E_GRID
    flags = ['--power', str(pc.E2E_R), '--plant', pc.E2E_PLANT, '--powerThreshold', ','.join(repr(C) for C in pc.E2E_THRESHOLDS),
             '--powerReps']
    out = str(d / 'p.txt')
    _cli(base + ['-o', out] + flags)
    return d, base, flags, out


def _close(a, b):
    if a == 'NA' or b == 'NA':
        return a == b
    return abs(float(a) - float(b)) <= 1e-6 * abs(float(b))


def test_cli_writes_what_the_host_pipeline_computes(e2e_run):
    d, base, flags, out = e2e_run
    e = pc.e2e()
    arg, clr, lin, ns = (a[:pc.E2E_R] for a in pc.e2e_host(True))
    col = locate.main_columns(out)
    want, want_reps = str(d / 'want.power.txt'), str(d / 'want.reps.txt')
    power.write_power(want, col, e.rows_c, power.n_reach(e.gen, e.centre_pos, e.A), e.gen, e.union, e.lo, e.hi, arg, clr, lin,
                      e.planted, len(e.xs), len(e.abetas), pc.E2E_THRESHOLDS)
    power.write_reps(want_reps, col, e.rows_c, e.union, arg, clr, lin, ns, [f'{v}' for v in e.xs], [f'{v}' for v in e.abetas],
                     [f'{v}' for v in e.As])
    thr, got = power.read_power(out + '.power.txt')
    wthr, exp = power.read_power(want)
    assert thr == wthr == [repr(C) for C in pc.E2E_THRESHOLDS] and len(got) == len(exp) == len(e.rows_c) >= 3
    approx = ('CLR_lo', 'CLR_med', 'CLR_hi')
    for a, b in zip(got, exp):
        assert list(a) == list(b)
        for name in a:
            assert _close(a[name], b[name]) if name in approx else a[name] == b[name], (name, a[name], b[name])
        assert a['n_ok'] == str(pc.E2E_R) and int(a['nReach']) > 100
    powers = [[float(r['power_' + t]) for r in got] for t in thr]
    assert 0.0 < np.mean(powers[1]) < np.mean(powers[0]) <= 1.0
    got_reps, exp_reps = power.read_reps(out + '.power.reps.txt'), power.read_reps(want_reps)
    assert len(got_reps) == len(exp_reps) == pc.E2E_R * len(e.rows_c)
    for a, b in zip(got_reps, exp_reps):
        for name in a:                                                 # argmax rows, grid values and nSites are exact
            assert _close(a[name], b[name]) if name == 'CLR' else a[name] == b[name], (name, a[name], b[name])


def test_cli_leaves_the_main_output_alone_and_repeats_itself(e2e_run, capsys):
    d, base, flags, out = e2e_run
    plain, again, seeded, obs = (str(d / n) for n in ('plain.txt', 'again.txt', 'seeded.txt', 'obs.txt'))
    _cli(base + ['-o', plain])
    _cli(base + ['-o', again] + flags)
    _cli(base + ['-o', seeded] + flags + ['--powerSeed', '2'])
    _cli(base + ['-o', obs] + flags + ['--powerBackground', 'obs'])
    rd = lambda p: open(p, 'rb').read()
    assert rd(out) == rd(plain) == rd(again) == rd(seeded) == rd(obs)
    assert not os.path.exists(plain + '.power.txt')
    for suffix in ('.power.txt', '.power.reps.txt'):
        assert rd(out + suffix) == rd(again + suffix)
    assert rd(out + '.power.reps.txt') != rd(seeded + '.power.reps.txt')
    assert rd(out + '.power.reps.txt') != rd(obs + '.power.reps.txt')
    # with --nullPerm the run's own thresholds are added, and the null's files stay what they are without --power
    n0, n1 = str(d / 'n0.txt'), str(d / 'n1.txt')
    _cli(base + ['-o', n0, '--nullPerm', '5'])
    capsys.readouterr()
    _cli(base + ['-o', n1, '--nullPerm', '5'] + flags[:4])
    said = capsys.readouterr().out
    for suffix in ('', '.null.txt', '.pval.txt'):
        assert rd(n0 + suffix) == rd(n1 + suffix), suffix
    mx = np.array([float(l.split('\t')[1]) for l in open(n1 + '.null.txt').read().splitlines()[1:]])
    thr, rows = power.read_power(n1 + '.power.txt')
    assert null.threshold(mx, 0.99) == null.threshold(mx, 0.95) and thr == [repr(null.threshold(mx, 0.95))]      # 5 replicates: one maximum
    assert 'Power: %d centre/s' % len(rows) in said and 'mean power' in said
    assert not os.path.exists(n1 + '.power.reps.txt')


def test_cli_refusals(e2e_run, capsys):
    d, base, flags, out = e2e_run
    o = ['-o', str(d / 'r.txt')]
    for argv, msg in ((base + o + ['--plant', pc.E2E_PLANT], '--plant needs --power.'),
                      (base + o + ['--power', '1', '--plant', pc.E2E_PLANT, '--powerThreshold', '5'], '--power takes a number of replicates >= 2'),
                      (base + o + ['--power', '4', '--powerThreshold', '5'], '--power needs --plant'),
                      (base + o + ['--power', '4', '--plant', pc.E2E_PLANT], '--power needs --powerThreshold'),
                      (base + ['--power', '4', '--plant', pc.E2E_PLANT, '--powerThreshold', '5'], '--power needs -o'),
                      (base + o + ['-w', '100', '--power', '4', '--plant', pc.E2E_PLANT, '--powerThreshold', '5'], 'default window mode'),
                      (base + o + ['--power', '4', '--plant', '1000,0.5,101', '--powerThreshold', '5'], 'is not a value of the grid'),
                      (base + o + ['--power', '4', '--plant', pc.E2E_PLANT, '--powerThreshold', '5', '--plantEvery', '0.01'],
                       'smaller than the bound')):
        with pytest.raises(SystemExit) as e:
            _cli(argv)
        assert e.value.code == 1
        assert msg in capsys.readouterr().out, msg
    assert not os.path.exists(str(d / 'r.txt')) and not os.path.exists(str(d / 'r.txt.power.txt'))     # refused before any scan


def test_cli_two_files_key_each_file(e2e_run, tmp_path):
    """The same chromosome twice in one run: file 0 repeats the one-file run, file 1 has other replicates (the file ordinal is part
    of the keys); with --nullPerm both files wait for the genome-wide thresholds and carry them."""
    import shutil
    d, base, flags, out = e2e_run
    twin = str(d / 'twin.txt')
    shutil.copy(base[1], twin)
    many = ['-i', base[1] + ',' + twin] + base[2:]
    res = tmp_path / 'res'
    _cli(many + ['-o', str(res)] + flags)
    rd = lambda p: open(p, 'rb').read()
    one, two = (str(res / (n + '.out.txt')) for n in ('in.txt', 'twin.txt'))
    assert rd(one) == rd(two) == rd(out)
    for suffix in ('.power.txt', '.power.reps.txt'):
        assert rd(one + suffix) == rd(out + suffix)
    assert rd(two + '.power.reps.txt') != rd(out + '.power.reps.txt')
    assert [r['physPos'] for r in power.read_power(two + '.power.txt')[1]] == [r['physPos'] for r in power.read_power(out + '.power.txt')[1]]
    nul = tmp_path / 'nul'
    _cli(many + ['-o', str(nul), '--nullPerm', '5'] + flags[:4])
    mx = np.array([float(l.split('\t')[1]) for l in open(str(nul / 'null.txt')).read().splitlines()[1:]])
    want = [repr(null.threshold(mx, 0.95))]
    for n in ('in.txt', 'twin.txt'):
        thr, rows = power.read_power(str(nul / (n + '.out.txt')) + '.power.txt')
        assert thr == want and len(rows) == len(pc.e2e().rows_c) and all(r['n_ok'] == str(pc.E2E_R) for r in rows)
        assert rd(str(nul / (n + '.out.txt'))) == rd(out)
