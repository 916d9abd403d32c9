"""The planted-signal power analysis on the host (ballermixplus_amd/power.py): the admissible counts against the oracle, the draw
against its own probabilities, the centre, summary and format rules, and -- for every fixed case tests/test_gpu_power.py uses --
that no redrawn site is undecided, that the oracle separates planted from unplanted backgrounds, and that no replicate maximum
sits on a threshold."""
import math

import numpy as np
import pytest

import powercases as pc
from util import oracle_R, orc

from ballermixplus_amd import null, power


# ------------------------------------------------------------------------------------------------ admissible counts

@pytest.mark.parametrize('stat', orc.STATS)
def test_allowed_rows_are_the_oracles_support(stat):
    for m in ((0, 1) if stat == 'B1' else (1, 2, 3)):
        sizes = np.array([7, 12, 20], dtype=np.int32)
        per = [2 if stat == 'B1' else int(n) + 1 for n in sizes]
        off = np.concatenate(([0], np.cumsum(per))).astype(np.int32)
        g = np.linspace(0.1, 0.9, off[-1])
        g[3], g[off[1] + 1] = np.nan, 0.0                            # absent from the helper file; a zero probability
        gw = power.allowed_rows(stat, m, sizes, off, g)
        for j, n in enumerate(sizes.tolist()):
            excl = set(int(k) for k in orc.excluded_counts(stat, n, m).tolist() if 0 <= k < per[j])
            for k in range(per[j]):
                r = off[j] + k
                want = 0.0 if (k in excl or not (g[r] > 0.0)) else g[r]
                assert gw[r] == want, (stat, m, n, k)


@pytest.mark.parametrize('stat', ['B2', 'B0'])
def test_total_is_the_sample_sizes_share(stat):
    """With a spectrum on every admissible count, sum_k gw (1 + alpha R) = prop(n): both mixture components are normalised on
    the same support."""
    sizes, m = (20, 24), 1
    spect, props = pc.analytic_spectrum(stat, sizes, m)
    xs, abetas = [0.2, 0.5], [0.5, 20.0]
    R = oracle_R(stat, sizes, m, spect, props, xs, abetas)
    per = [n + 1 for n in sizes]
    off = np.concatenate(([0], np.cumsum(per)))
    g = np.full(off[-1], np.nan)
    for (k, n), v in spect.items():
        g[off[sizes.index(n)] + k] = v
    gw = power.allowed_rows(stat, m, np.array(sizes), off, g)
    for ix in range(2):
        for ia in range(2):
            for alpha in (0.0, 1e-8, 0.3, 0.9, 1.0):
                for j, n in enumerate(sizes):
                    a, b = off[j], off[j + 1]
                    with np.errstate(invalid='ignore'):
                        mk = gw[a:b] * (1.0 + alpha * R[ix, ia, a:b])
                    total = np.cumsum(np.where(np.isfinite(mk) & (mk > 0), mk, 0.0))[-1]
                    assert abs(total - props[n]) <= 1e-12 * props[n], (stat, ix, ia, alpha, n, total)


# ------------------------------------------------------------------------------------------------ the draw

def test_hash_to_uniform_mapping():
    key = 0x0123456789ABCDEF
    u = power.uniforms(key, np.array([0, 1, 2 ** 31 + 5]))
    for i, v in zip((0, 1, 2 ** 31 + 5), u.tolist()):
        h = null.mix(key ^ null.mix(i))
        assert v == (h >> 11) / 2.0 ** 53 and 0.0 <= v < 1.0
    # splitmix64 of 0 and 1 (the published test vectors of the generator seeded with 0)
    assert null.mix(0) == 0xE220A8397B1DCDAF
    assert power.uniforms(0, np.array([0]))[0] == (null.mix(null.mix(0)) >> 11) * 2.0 ** -53
    big = power.uniforms(5, np.arange(200000))
    assert abs(big.mean() - 0.5) < 5 * math.sqrt(1 / 12 / 200000) and big.max() < 1.0


def test_draw_frequencies_follow_the_mixture():
    """One size (n = 20), 20 000 redrawn sites at one common distance from the centre, a fixed key: the count of every k within 5
    binomial sigma of its probability m_k / total."""
    n, N, A = 20, 20000, 1000.0
    spect, props = pc.analytic_spectrum('B2', (n,), 1)
    R = oracle_R('B2', (n,), 1, spect, props, [0.5], [20.0])[0, 0]
    off = np.array([0, n + 1])
    g = np.array([spect.get((k, n), np.nan) for k in range(n + 1)])
    gw = power.allowed_rows('B2', 1, np.array([n]), off, g)
    gen = np.concatenate(([0.0], np.full(N, 0.001)))                  # the centre's own site, then the 20 000 at distance 0.001
    rows = np.full(N + 1, n, dtype=np.int32)                          # all substitutions
    new, margin = power.planted_rows(gen, rows, np.array([n]), off, R, gw, A, [0.0], power.replicate_key(3, 0, 0))
    assert new[0] == n and margin[0] == np.inf                        # the site at the centre stays
    alpha = np.exp(-1.0)
    m = np.where(gw > 0.0, np.maximum(gw * (1.0 + alpha * np.nan_to_num(R)), 0.0), 0.0)       # (R is NaN where g is absent: k = 0)
    p = m / m.sum()
    cnt = np.bincount(new[1:], minlength=n + 1)
    assert cnt[0] == 0 and p[0] == 0.0
    for k in range(1, n + 1):
        assert abs(cnt[k] - N * p[k]) <= 5.0 * math.sqrt(N * p[k] * (1.0 - p[k])), (k, cnt[k], N * p[k])
    assert np.all(margin[1:] > power.MARGIN)


def test_sites_at_the_centre_and_out_of_reach_keep_their_rows():
    c = pc.sampler('B2')
    new, margin = c.host(pc.SAMPLER_KEY)
    first, count = c.runs()
    inr = np.zeros(len(c.gen), dtype=bool)
    for ck, a, n in zip(c.centres, first, count):
        assert a == np.nonzero(c.A * np.abs(c.gen - ck) <= power.ALPHA_CUT)[0][0]
        assert n == np.count_nonzero(c.A * np.abs(c.gen - ck) <= power.ALPHA_CUT)
        inr[a:a + n] = c.gen[a:a + n] != ck
    assert first[0] == 0 and count[0] < count[2]                      # the first centre's run is clipped
    assert np.count_nonzero(c.gen == c.centres[1]) == 21              # the tie is not redrawn
    assert np.array_equal(new[~inr], c.rows[~inr]) and np.all(margin[~inr] == np.inf)
    assert np.all(np.isfinite(margin[inr])) and np.count_nonzero(new != c.rows) > 1000
    # sample sizes never change
    blk = lambda r: np.searchsorted(c.model.row_off, r, side='right')
    assert np.array_equal(blk(new), blk(c.rows))
    assert np.all(c.gw[new[inr]] > 0.0)
    # centres too close, descending or not finite
    for bad in ([0.1, 0.1 + 2.0 * power.ALPHA_CUT / c.A], [0.2, 0.1], [math.nan]):
        with pytest.raises(ValueError):
            power.planted_rows(c.gen, c.rows, c.model.sizes, c.model.row_off, c.R[1, 1], c.gw, c.A, bad, 1)


# ------------------------------------------------------------------------------------------------ centres

def test_centre_rules():
    g = np.arange(0.0, 100.0, 0.5)
    rows = power.centres(g, 10.0, 8.0)
    assert g[rows].tolist() == [5.0, 15.0, 25.0, 35.0, 45.0, 55.0, 65.0, 75.0, 85.0, 95.0]      # targets g[0] + (j + 0.5) D
    g2 = np.array([0.0, 4.9, 5.2, 14.0, 16.0, 16.0, 40.0, 41.0, 58.0, 100.0])
    rows = power.centres(g2, 10.0, 9.5)
    # targets 5, 15, 25, ..., 95: snapped to 5.2, 16.0 (the first of the tie), 40 (for 25 and 35: a repeat), 58 (45; again for 55),
    # 100 (65 .. 95: repeats)
    assert rows.tolist() == [2, 4, 6, 8, 9]
    rows = power.centres(g2, 10.0, 10.0)
    assert rows.tolist() == [2, 4, 6, 8, 9]                            # 16.0 - 5.2 = 10.8 >= 10
    rows = power.centres(np.array([0.0, 5.0, 14.0, 30.0]), 10.0, 9.5)
    assert rows.tolist() == [1, 3]                                     # 14 lies closer than the bound to 5 and is dropped
    with pytest.raises(ValueError, match='smaller than the bound'):
        power.centres(g, 7.9, 8.0)
    assert len(power.centres(np.zeros(0), 1.0, 1.0)) == 0
    assert power.centres(np.array([1.0, 1.5]), 10.0, 1.0).tolist() == []          # the first target lies past the end
    assert power.bound_of(2.0, 100.0, 1000.0, 18.0) == 2.0 + 0.18 + 0.018
    rows, union, lo, hi, H, bound, D = power.plan_file(g, 10.0, 5.0)
    assert H == power.ALPHA_CUT / 10.0 and bound == H + power.ALPHA_CUT / 5.0 + H and D == 1.05 * bound
    assert np.all(np.diff(g[rows]) >= bound) and np.all(10.0 * np.diff(g[rows]) > power.SPACING * power.ALPHA_CUT)


def test_plant_and_threshold_parsing():
    As, xs, abetas = [100, 1000.0, 1e6], [0.05, 0.15000000000000002, 0.5], [1, 100, 1e9]
    assert power.parse_plant('1000,0.5,100', As, xs, abetas) == (1, 2, 1)
    assert power.parse_plant('1e6,0.05,1000000000', As, xs, abetas) == (2, 0, 2)
    for bad in ('1000,0.15,100', '1000,0.5', '999,0.5,100', 'a,b,c'):
        with pytest.raises(ValueError, match='A: 100.0, 1000.0, 1000000.0'):
            power.parse_plant(bad, As, xs, abetas)
    assert power.parse_thresholds('10,2.5,10') == [10.0, 2.5]
    with pytest.raises(ValueError):
        power.parse_thresholds('10,x')
    assert power.value_refusal(1, None, None, None, None, None).startswith('--power takes')
    assert power.value_refusal(2, None, None, None, None, '5') is None
    assert power.value_refusal(2, -1.0, None, None, None, None).startswith('--plantEvery')
    assert power.value_refusal(2, None, 0.0, None, None, None).startswith('--powerSpan')
    assert power.value_refusal(2, None, None, 0, None, None).startswith('--powerBlock')
    assert power.value_refusal(2, None, None, None, 'neutral', None).startswith('--powerBackground')
    assert power.value_refusal(2, None, None, None, None, 'nan').startswith('--powerThreshold')
    assert power.replicate_key(1, 0) != power.background_key(1, 0) != null.replicate_key(1, 0)


# ------------------------------------------------------------------------------------------------ summary and format

def test_summary_and_format_rules():
    nx, nab = 3, 4
    lin_of = lambda iA, ix, ia: (iA * nx + ix) * nab + ia
    planted = (1, 2, 3)
    g = np.arange(10) * 0.5
    arg = np.array([4, 6, -1, 4, 2, 9])
    clr = np.array([10.0, 30.0, 0.0, 20.0, 50.0, 40.0])
    lin = np.array([lin_of(1, 2, 3), lin_of(1, 2, 0), -1, lin_of(0, 2, 3), lin_of(1, 0, 3), lin_of(1, 2, 3)])
    s = power.summarise(arg, clr, lin, g, 4, 2, 9, planted, nx, nab, [20.0, 45.0, 5.0])
    assert s['n_ok'] == 5
    assert (s['CLR_lo'], s['CLR_med'], s['CLR_hi']) == (10.0, 30.0, 50.0)          # ranks ceil(.025 * 5) = 1, 3, ceil(4.875) = 5
    assert s['power'] == [0.8, 0.2, 1.0]                                            # >= C
    assert (s['lo'], s['hi']) == (2, 9)
    assert s['pos_rmse'] == math.sqrt((0 + 1.0 + 0 + 1.0 + 2.5 ** 2) / 5)
    assert s['p_edge'] == 0.4 and s['p_x'] == 0.8 and s['p_s'] == 0.8 and s['p_A'] == 0.8 and s['p_all'] == 0.4
    pos_of = lambda r: ('p%d' % r, 'g%d' % r)
    line = power.format_row(('100', '0.1'), 37, s, pos_of)
    assert line == '\t'.join(['100', '0.1', '37', '5', '10.0', '30.0', '50.0', '0.8', '0.2', '1.0', 'p2', 'p9', 'g2', 'g9',
                              repr(s['pos_rmse']), '0.4', '0.8', '0.8', '0.8', '0.4']) + '\n'
    assert power.header([20.0, 45.5]).split('\t')[7:9] == ['power_20.0', 'power_45.5']
    assert len(power.header([20.0, 45.0, 5.0]).split('\t')) == len(line.split('\t'))
    one = power.summarise(np.array([-1, 3]), np.array([0.0, 9.0]), np.array([-1, 0]), g, 4, 2, 9, planted, nx, nab, [1.0])
    assert one['n_ok'] == 1
    assert power.format_row(('1', '2'), 0, one, pos_of) == '\t'.join(['1', '2', '0', '1'] + ['NA'] * 14) + '\n'
    assert [a.tolist() for a in power.decode(np.array([-1, lin_of(2, 1, 3)]), nx, nab)] == [[-1, 2], [-1, 1], [-1, 3]]


def test_writers_and_readers(tmp_path):
    main = tmp_path / 'o.txt'
    main.write_text('physPos\tgenPos\tCLR\n' + ''.join('%d\t%r\t1.0\n' % (100 * t, 0.5 * t) for t in range(10)))
    from ballermixplus_amd import locate
    col = locate.main_columns(str(main))
    g = np.arange(10) * 0.5
    union = np.arange(1, 9)
    arg = np.array([[3], [5], [-1]], dtype=np.int32)                    # into the union: track rows 4 and 6
    clr = np.array([[7.0], [9.0], [0.0]])
    lin = np.array([[5], [-1], [-1]], dtype=np.int32)
    ns = np.array([[11], [0], [0]], dtype=np.int32)
    sums = power.write_power(str(main) + '.power.txt', col, [4], [17], g, union, [0], [7], arg, clr, lin, (0, 1, 1), 3, 4, [8.0])
    thr, rows = power.read_power(str(main) + '.power.txt')
    assert thr == ['8.0'] and len(rows) == 1 and sums[0]['n_ok'] == 2
    r = rows[0]
    assert (r['physPos'], r['genPos'], r['nReach'], r['n_ok'], r['power_8.0']) == ('400', '2.0', '17', '2', '0.5')
    assert (r['lo_physPos'], r['hi_physPos'], r['lo_genPos'], r['hi_genPos']) == ('400', '600', '2.0', '3.0')
    power.write_reps(str(main) + '.power.reps.txt', col, [4], union, arg, clr, lin, ns, ['0.1', '0.2', '0.3'], ['1', '2', '3', '4'],
                     ['100', '200'])
    reps = power.read_reps(str(main) + '.power.reps.txt')
    assert [d['replicate'] for d in reps] == ['0', '1']
    assert (reps[0]['arg_physPos'], reps[0]['CLR'], reps[0]['x_hat'], reps[0]['s_hat'], reps[0]['A_hat'], reps[0]['nSites']) == \
        ('400', '7.0', '0.2', '2', '100', '11')
    assert (reps[1]['x_hat'], reps[1]['nSites']) == ('0.0', '0')
    # a file without centres: the header only
    z = np.zeros(0, dtype=np.int64)
    e = np.zeros((3, 0))
    power.write_power(str(main) + '.none.txt', col, z, z, g, z, z, z, e.astype(np.int32), e, e.astype(np.int32), (0, 0, 0), 3, 4, [8.0])
    assert open(str(main) + '.none.txt').read() == power.header([8.0])


# ------------------------------------------------------------------------------------------------ the GPU file's fixed cases

@pytest.mark.parametrize('stat', pc.SAMPLER_STATS)
def test_sampler_cases_have_no_undecided_site(stat):
    c = pc.sampler(stat)
    new, margin = c.host(pc.SAMPLER_KEY)
    redrawn = np.isfinite(margin)
    assert redrawn.sum() > 1500 and np.all(margin[redrawn] > power.MARGIN), margin.min()
    assert np.count_nonzero(new != c.rows) > 500
    # ... nor on a permuted background (test 1 plants onto one as well)
    bg = c.rows[null.block_permutation(len(c.rows), power.background_key(7, 0, 0), 3)]
    assert np.all(c.host(pc.SAMPLER_KEY, rows=bg)[1] > power.MARGIN)


def test_large_case_has_no_undecided_site():
    c = pc.large()
    new, margin = c.host(pc.LARGE_KEY)
    redrawn = np.isfinite(margin)
    assert redrawn.sum() > 300 and np.all(margin[redrawn] > power.MARGIN), margin.min()
    assert np.count_nonzero(new != c.rows) > 100


def test_e2e_case_has_no_undecided_site_and_no_clr_on_a_threshold():
    e = pc.e2e()
    assert len(e.rows_c) >= 3
    margin = e.margins(pc.SEP_R)
    assert np.isfinite(margin).sum() > 1000 * pc.SEP_R and np.all(margin > power.MARGIN), margin.min()
    arg, clr, lin, ns = pc.e2e_host(True)
    assert np.all(arg >= 0)
    for C in pc.E2E_THRESHOLDS:
        assert np.all(np.abs(clr[:pc.E2E_R] - C) > 1e-6 * C)
    hit = [float(np.mean(clr[:pc.E2E_R] >= C)) for C in pc.E2E_THRESHOLDS]
    assert 0.0 < hit[1] < hit[0] <= 1.0, hit                            # thresholds that tell something


def test_oracle_separates_planted_from_unplanted_backgrounds():
    """The separation case of the GPU file with the oracle: on every replicate and centre the range maximum after planting is at
    least twice the maximum of the same range on the same permuted background without planting."""
    planted, plain = pc.e2e_host(True), pc.e2e_host(False)
    assert planted[1].shape == (pc.SEP_R, len(pc.e2e().rows_c))
    assert np.all(plain[1] > 0.0) and np.all(planted[1] >= 2.0 * plain[1]), (planted[1] / plain[1]).min()
    # the scan finds the planted strength more often than not at these centres
    iA, ix, ia = power.decode(planted[2], len(pc.e2e().xs), len(pc.e2e().abetas))
    assert np.mean(ix == pc.e2e().planted[1]) > 0.5
