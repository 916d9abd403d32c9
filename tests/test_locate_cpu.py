"""--locate without a GPU: the keys, the host restatement of the resampling, ranges and their union, the summary rules, the
writers and readers byte for byte, and every refusal of the command line."""
import glob
import math
import os

import numpy as np
import pytest

from util import REFT

from ballermixplus_amd import boot, cli, locate, null
from ballermixplus_amd import scan as scanmod

EX1 = os.path.join(REFT, 'Example1_fullSweep_200kya_DAF.txt')
SPECT = os.path.join(REFT, 'HC_CEU_Neut_DAF_spect_for_B2.txt')


# ---------------------------------------------------------------------------------------------------- keys, resampling

def test_keys_are_their_own_stream():
    for seed in (0, 1, 7, 2 ** 64 - 1):
        ks = {locate.replicate_key(seed, r, f) for r in range(4) for f in range(3)}
        assert len(ks) == 12
        for r in range(4):
            for f in range(3):
                k = locate.replicate_key(seed, r, f)
                assert k != boot.replicate_key(seed, r, f) and k != null.replicate_key(seed, r, f)
                assert k == null.replicate_key(null.mix((seed & (2 ** 64 - 1)) ^ locate.SEED_DOMAIN), r, f)
    assert locate.SEED_DOMAIN != boot.SEED_DOMAIN
    assert locate.replicate_key(1, 0) == locate.replicate_key(1, 0, 0) != locate.replicate_key(1, 0, 1)


@pytest.mark.parametrize('N,B', [(1, 1), (5, 1), (100, 7), (1000, 64), (1025, 1), (33, 100)])
def test_resampled_is_repeat_by_the_bootstrap_weights(N, B):
    rng = np.random.default_rng(N + B)
    gen = np.sort(rng.random(N))
    rows = rng.integers(0, 50, N).astype(np.int32)
    for key in (locate.replicate_key(3, 0), locate.replicate_key(3, 1, 2)):
        w = boot.site_weights(key, N, B)
        g, r = locate.resampled(gen, rows, key, B)
        assert len(g) == len(r) == int(w.sum())
        assert np.array_equal(g.view(np.uint64), np.repeat(gen, w).view(np.uint64)) and np.array_equal(r, np.repeat(rows, w))
        assert r.dtype == rows.dtype
        # order kept, weight-0 sites dropped, every kept site w times
        src = np.repeat(np.arange(N), w)
        assert np.all(np.diff(src) >= 0) and np.array_equal(np.bincount(src, minlength=N), w)
        for b in range(0, N, B):
            assert len(set(w[b:b + B].tolist())) == 1               # one weight per block


# ---------------------------------------------------------------------------------------------------- ranges

def test_ranges_overlap_and_union():
    g = np.arange(10) * 1.0                      # rows at 0, 1, ..., 9
    union, lo, hi = locate.ranges(g, [2, 4, 9], 1.5)
    assert union.tolist() == [1, 2, 3, 4, 5, 8, 9]                  # [1..3] and [3..5] overlap at row 3; [8..9]
    assert lo.tolist() == [0, 2, 5] and hi.tolist() == [2, 4, 6]
    for k, a in enumerate((2, 4, 9)):
        inside = np.nonzero(np.abs(g - g[a]) <= 1.5)[0]
        assert union[lo[k]:hi[k] + 1].tolist() == inside.tolist()


def test_range_of_one_row_and_ties_at_one_position():
    g = np.array([0.0, 1.0, 1.0, 1.0, 5.0, 9.0])
    union, lo, hi = locate.ranges(g, [4], 0.5)
    assert union.tolist() == [4] and lo.tolist() == [0] and hi.tolist() == [0]
    union, lo, hi = locate.ranges(g, [2], 0.5)                       # rows at the apex's own position belong to its range
    assert union.tolist() == [1, 2, 3] and (lo[0], hi[0]) == (0, 2)
    union, lo, hi = locate.ranges(g, [1, 4], 4.0)                    # the bound is inclusive: 5 - 1 <= 4
    assert union.tolist() == [0, 1, 2, 3, 4, 5] and lo.tolist() == [0, 1] and hi.tolist() == [4, 5]


def test_range_that_covers_the_whole_file_and_no_apexes():
    g = np.cumsum(np.random.default_rng(1).random(50))
    union, lo, hi = locate.ranges(g, [0, 20, 49], 1e9)
    assert union.tolist() == list(range(50)) and lo.tolist() == [0, 0, 0] and hi.tolist() == [49, 49, 49]
    union, lo, hi = locate.ranges(g, [], 1.0)
    assert len(union) == len(lo) == len(hi) == 0
    for bad in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError):
            locate.ranges(g, [3], bad)


def _ts_with_na():
    """Main output: NA, row, row, NA, row, row -- four track rows."""
    ts = scanmod.TestSites()
    ts.add_na('5\t5e-06\t0\tNA\tNA\tNA\t0\n')
    ts.add(10, 1e-05, 1e-05, 0, 3)
    ts.add(20, 2e-05, 2e-05, 0, 3)
    ts.add_na('25\t2.5e-05\t0\tNA\tNA\tNA\t0\n')
    ts.add(30, 3e-05, 3e-05, 0, 3)
    ts.add(40, 4e-05, 4e-05, 0, 3)
    main = (scanmod.HEADER + '5\t5e-06\t0\tNA\tNA\tNA\t0\n' + '10\t1e-05\t1.5\t0.3\t5\t900\t3\n' + '20\t2e-05\t7.25\t0.3\t5\t900\t3\n'
            + '25\t2.5e-05\t0\tNA\tNA\tNA\t0\n' + '30\t3e-05\t2.0\t0.3\t5\t900\t3\n' + '40\t4e-05\t0.0\t0\t0\t0\t0\n')
    return ts, main


def test_na_rows_are_not_part_of_the_track(tmp_path):
    ts, main = _ts_with_na()
    g = locate.track_positions(ts)
    assert g.tolist() == [1e-05, 2e-05, 3e-05, 4e-05]
    union, lo, hi = locate.ranges(g, [1], 1.5e-05)
    assert union.tolist() == [0, 1, 2]                               # the NA row at 2.5e-05 lies inside H and is no row of the range
    (tmp_path / 'o.txt').write_text(main)
    col = locate.main_columns(str(tmp_path / 'o.txt'), np.asarray(ts.order, dtype=np.int64) + 1)
    assert [col(t)[0] for t in range(4)] == ['10', '20', '30', '40']
    col = locate.main_columns(str(tmp_path / 'o.txt'))
    assert col(0)[0] == '5'                                           # (without the map: row t is line t + 1)


# ---------------------------------------------------------------------------------------------------- argmax, summary

def test_argmax_rows_first_row_wins_and_rows_without_a_result_are_skipped():
    clr = np.array([1.0, 3.0, 3.0, 9.0, 2.0, 2.0])
    has = np.array([True, True, True, False, True, True])
    row, val = locate.argmax_rows(clr, has, [0, 3, 4, 0], [2, 3, 5, 5])
    assert row.tolist() == [1, -1, 4, 1] and val.tolist() == [3.0, 0.0, 2.0, 3.0]
    assert row.dtype == np.int32


def _naive_rank(q, n):
    return min(max(math.ceil(round(q * n, 9)), 1), n)


@pytest.mark.parametrize('level', [0.95, 0.5])
def test_summary_order_statistics(level):
    rng = np.random.default_rng(11)
    R = 40
    g = np.arange(30) * 0.5
    arg = rng.integers(5, 16, R)
    arg[[3, 17]] = -1                            # two replicates without an argmax
    clr = rng.random(R) * 10
    s = locate.summarise(arg, clr, g, 10, 5, 15, level)
    ok = arg >= 0
    n = int(ok.sum())
    a, v = np.sort(arg[ok]), np.sort(clr[ok])
    i, j = _naive_rank((1 - level) / 2, n), _naive_rank((1 + level) / 2, n)
    assert n == 38 and s['n_ok'] == n
    assert (s['lo'], s['hi']) == (a[i - 1], a[j - 1]) and (s['CLR_lo'], s['CLR_hi']) == (v[i - 1], v[j - 1])
    assert s['gen_sd'] == float(np.std(g[arg[ok]], ddof=1))
    assert s['p_apex'] == np.count_nonzero(arg == 10) / n
    assert s['p_edge'] == np.count_nonzero((arg == 5) | (arg == 15)) / n
    if level == 0.95:
        assert (i, j) == (1, 38)                 # ceil(0.025 * 38) = 1, ceil(0.975 * 38) = ceil(37.05) = 38
    else:
        assert (i, j) == (10, 29)                # ceil(0.25 * 38) = 10, ceil(0.75 * 38) = 29


def test_summary_of_hand_made_replicates():
    g = np.array([0.0, 1.0, 2.0, 3.0, 4.0])
    arg = np.array([2, 2, 0, 4, 2, 3, 2, 2, 1, 2])
    clr = np.arange(10.0)
    s = locate.summarise(arg, clr, g, 2, 0, 4, 0.5)
    # sorted rows 0 1 2 2 2 2 2 2 3 4: the ceil(2.5) = 3rd and the ceil(7.5) = 8th
    assert (s['lo'], s['hi']) == (2, 2) and (s['CLR_lo'], s['CLR_hi']) == (2.0, 7.0)
    assert s['p_apex'] == 0.6 and s['p_edge'] == 0.2 and s['n_ok'] == 10
    s = locate.summarise(arg, clr, g, 2, 0, 4, 0.95)
    assert (s['lo'], s['hi']) == (0, 4)                              # ceil(0.25) = 1st, ceil(9.75) = 10th
    s = locate.summarise(np.array([3, 3]), np.array([1.0, 2.0]), g, 3, 3, 3, 0.95)     # a one-row range: apex and both edges
    assert (s['lo'], s['hi'], s['gen_sd'], s['p_apex'], s['p_edge']) == (3, 3, 0.0, 1.0, 1.0)


@pytest.mark.parametrize('arg,n_ok', [([-1, -1, -1], 0), ([-1, 2, -1], 1), ([1, -1, 2], 2)])
def test_summary_below_two_ok_is_na(arg, n_ok):
    s = locate.summarise(np.array(arg), np.array([1.0, 2.0, 3.0]), np.arange(4.0), 2, 1, 3)
    assert s['n_ok'] == n_ok
    if n_ok < 2:
        assert s['lo'] == s['hi'] == -1
        assert all(s[k] != s[k] for k in ('gen_sd', 'p_apex', 'p_edge', 'CLR_lo', 'CLR_hi'))
    else:
        assert (s['lo'], s['hi'], s['CLR_lo'], s['CLR_hi']) == (1, 2, 1.0, 3.0)
        assert s['gen_sd'] == float(np.std([1.0, 2.0], ddof=1)) and s['p_apex'] == 0.5 and s['p_edge'] == 0.5


# ---------------------------------------------------------------------------------------------------- writers, readers

def test_writer_bytes_and_readers_round_trip(tmp_path):
    ts, main = _ts_with_na()
    path = tmp_path / 'o.txt'
    path.write_text(main)
    col = locate.main_columns(str(path), np.asarray(ts.order, dtype=np.int64) + 1)
    g = locate.track_positions(ts)
    apex = np.array([1, 3])
    union, lo, hi = locate.ranges(g, apex, 1.5e-05)
    assert union.tolist() == [0, 1, 2, 3] and lo.tolist() == [0, 2] and hi.tolist() == [2, 3]
    #                 peak 0 (range rows 0..2, apex 1)   peak 1 (range rows 2..3, apex 3): one ok replicate only
    arg = np.array([[1, -1], [0, 3], [1, -1], [2, -1]], dtype=np.int32)
    clr = np.array([[7.5, 0.0], [6.25, 0.125], [8.0, 0.0], [7.0, 0.0]])
    locate.write_locate(str(tmp_path / 'l.txt'), col, apex, g, union, lo, hi, arg, clr, 0.5)
    sd = repr(float(np.std([1e-05, 2e-05, 2e-05, 3e-05], ddof=1)))
    want = (locate.HEADER
            + '20\t2e-05\t7.25\t10\t20\t1e-05\t2e-05\t' + sd + '\t0.5\t0.5\t6.25\t7.5\t4\n'
            + '40\t4e-05\t0.0\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\t1\n')
    assert (tmp_path / 'l.txt').read_text() == want
    assert locate.HEADER == ('physPos\tgenPos\tCLR\tlo_physPos\thi_physPos\tlo_genPos\thi_genPos\tgen_sd\tp_apex\tp_edge\tCLR_lo\t'
                             'CLR_hi\tn_ok\n')
    rows = locate.read_locate(str(tmp_path / 'l.txt'))
    assert [r['physPos'] for r in rows] == ['20', '40'] and rows[0]['lo_genPos'] == '1e-05' and rows[0]['hi_physPos'] == '20'
    assert rows[0]['gen_sd'] == float(sd) and rows[0]['p_edge'] == 0.5 and rows[0]['CLR_hi'] == 7.5 and rows[0]['n_ok'] == 4
    assert rows[1]['n_ok'] == 1 and rows[1]['gen_sd'] != rows[1]['gen_sd'] and rows[1]['lo_physPos'] == 'NA'
    locate.write_reps(str(tmp_path / 'r.txt'), col, apex, union, arg, clr)
    assert (tmp_path / 'r.txt').read_text() == (
        'physPos\tgenPos\treplicate\targ_physPos\targ_genPos\tCLR\n'
        '20\t2e-05\t0\t20\t2e-05\t7.5\n20\t2e-05\t1\t10\t1e-05\t6.25\n20\t2e-05\t2\t20\t2e-05\t8.0\n20\t2e-05\t3\t30\t3e-05\t7.0\n'
        '40\t4e-05\t1\t40\t4e-05\t0.125\n')
    reps = locate.read_reps(str(tmp_path / 'r.txt'))
    assert list(reps) == [('20', '2e-05'), ('40', '4e-05')]
    assert reps[('20', '2e-05')]['replicate'].tolist() == [0, 1, 2, 3] and reps[('20', '2e-05')]['CLR'].tolist() == [7.5, 6.25, 8.0, 7.0]
    assert reps[('20', '2e-05')]['arg_physPos'] == ['20', '10', '20', '30'] and reps[('40', '4e-05')]['arg_genPos'] == ['4e-05']
    assert locate.output_name('a/b.txt') == 'a/b.txt.locate.txt' and locate.reps_name('a/b.txt') == 'a/b.txt.locate.reps.txt'


def test_a_file_without_peaks_gets_the_header_only(tmp_path):
    from ballermixplus_amd import peaks
    ts, main = _ts_with_na()
    path = tmp_path / 'o.txt'
    path.write_text(main)
    n = locate.locate_and_write(None, str(path), ts, (peaks.empty(), None), 8, reps=True)
    assert n == (0, 0)
    assert (tmp_path / 'o.txt.locate.txt').read_text() == locate.HEADER
    assert (tmp_path / 'o.txt.locate.reps.txt').read_text() == locate.REPS_HEADER
    assert locate.read_locate(str(tmp_path / 'o.txt.locate.txt')) == [] and locate.read_reps(str(tmp_path / 'o.txt.locate.reps.txt')) == {}


def test_host_locate_runs_the_given_scan_on_the_resampled_arrays():
    rng = np.random.default_rng(2)
    N = 300
    gen = np.sort(rng.random(N))
    rows = rng.integers(0, 9, N)
    tg = gen[::10]
    keys = [locate.replicate_key(5, r) for r in range(3)]
    seen = []

    def scan(g, r, t):
        seen.append((g.copy(), r.copy()))
        clr = np.array([float(np.sum(r[np.abs(g - v) < 0.05])) for v in t])      # any function of the resampled array
        return clr, clr > 0

    row, val, tracks = locate.host_locate(scan, gen, rows, tg, [0, 5, 29], [9, 20, 29], keys, 4)
    assert row.shape == val.shape == (3, 3) and len(tracks) == 3
    for r, key in enumerate(keys):
        g, rw = locate.resampled(gen, rows, key, 4)
        assert np.array_equal(seen[r][0], g) and np.array_equal(seen[r][1], rw)
        a, v = locate.argmax_rows(tracks[r][0], tracks[r][1], [0, 5, 29], [9, 20, 29])
        assert np.array_equal(row[r], a) and np.array_equal(val[r], v)
    gen1 = np.array([0.5])
    key0 = next(k for k in (locate.replicate_key(1, r) for r in range(100)) if boot.site_weights(k, 1, 1)[0] == 0)
    row, val, tracks = locate.host_locate(scan, gen1, np.array([1]), gen1, [0], [0], [key0])
    assert row.tolist() == [[-1]] and tracks == [None]                # an empty resampled array: no track, no argmax


# ---------------------------------------------------------------------------------------------------- flags

def test_flags_off_by_default_and_parsed():
    opt = cli.build_parser().parse_args(['-i', EX1, '--spect', SPECT])
    assert opt.locate == 0 and not opt.locateReps and cli.locate_refusal(opt) is None
    assert opt.locateSeed is None and opt.locateBlock is None and opt.locateSpan is None and opt.locateLevel is None
    assert opt.locateMin is None
    opt = cli.build_parser().parse_args(['-i', EX1, '--spect', SPECT, '-o', 'o', '--peaks', '0.01', '--refine', '--boot', '4',
                                         '--nullPerm', '3', '--locate', '100', '--locateSeed', '7', '--locateBlock', '64',
                                         '--locateSpan', '0.02', '--locateLevel', '0.9', '--locateMin', '12.5', '--locateReps'])
    assert (opt.locate, opt.locateSeed, opt.locateBlock, opt.locateSpan, opt.locateLevel, opt.locateMin, opt.locateReps) == \
        (100, 7, 64, 0.02, 0.9, 12.5, True)
    assert cli.locate_refusal(opt) is None and cli.peaks_refusal(opt) is None and cli.boot_refusal(opt) is None


PK = ['--peaks', '0.01', '-o', 'OUT']


@pytest.mark.parametrize('extra,env,word', [
    (['--locateSeed', '3'] + PK, {}, '--locateSeed'),
    (['--locateBlock', '3'] + PK, {}, '--locateBlock'),
    (['--locateSpan', '0.1'] + PK, {}, '--locateSpan'),
    (['--locateLevel', '0.9'] + PK, {}, '--locateLevel'),
    (['--locateMin', '3'] + PK, {}, '--locateMin'),
    (['--locateReps'] + PK, {}, '--locateReps'),
    (['--locate', '1'] + PK, {}, '>= 2'),
    (['--locate', '-3'] + PK, {}, '>= 2'),
    (['--locate', '8', '-o', 'OUT'], {}, '--peaks'),
    (['--locate', '8', '-w', '50'] + PK, {}, 'window mode'),
    (['--locate', '8', '--fixWinSize', '-w', '5000'] + PK, {}, 'window mode'),
    (['--locate', '8', '--fixWinSize'] + PK, {}, 'window mode'),
    (['--locate', '8', '--getSpect'] + PK, {}, '--getSpect'),
    (['--locate', '8', '--getConfig'] + PK, {}, '--getConfig'),
    (['--locate', '8', '--peaks', '0.01'], {}, '-o'),
    (['--locate', '8'] + PK, {'WORLD_SIZE': '2'}, 'multi-rank'),
    (['--locate', '8'] + PK, {'BMX_FORCE_DIST': '1'}, 'multi-rank'),
    (['--locate', '8', '--locateBlock', '0'] + PK, {}, '--locateBlock'),
    (['--locate', '8', '--locateSpan', '0'] + PK, {}, '--locateSpan'),
    (['--locate', '8', '--locateSpan', '-1'] + PK, {}, '--locateSpan'),
    (['--locate', '8', '--locateSpan', 'inf'] + PK, {}, '--locateSpan'),
    (['--locate', '8', '--locateSpan', 'nan'] + PK, {}, '--locateSpan'),
    (['--locate', '8', '--locateLevel', '0'] + PK, {}, '--locateLevel'),
    (['--locate', '8', '--locateLevel', '1'] + PK, {}, '--locateLevel'),
    (['--locate', '8', '--locateLevel', 'nan'] + PK, {}, '--locateLevel'),
    (['--locate', '8', '--locateMin', 'nan'] + PK, {}, '--locateMin'),
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
    assert word in said and said.startswith('--locate')               # refused in this feature's name
    assert not made and not glob.glob(str(tmp_path / '*'))


def test_window_mode_refusal_says_why(capsys):
    with pytest.raises(SystemExit):
        cli.main(['-i', EX1, '--spect', SPECT, '-o', 'x', '--peaks', '0.01', '--locate', '8', '-w', '50'])
    assert 'not defined on a resampled' in capsys.readouterr().out


def test_help_and_docstring_name_the_flags():
    text = cli.build_parser().format_help()
    for flag in ('--locate', '--locateSeed', '--locateBlock', '--locateSpan', '--locateLevel', '--locateMin', '--locateReps'):
        assert flag in text and flag in cli.__doc__
