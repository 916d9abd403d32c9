"""Peak calling (--peaks) without a GPU: the host restatement of peaks.py against an O(M^2) loop written straight from the
definition on nasty tracks, the stated consequences as properties, the reference's own Example 2 as a fixture (and its
stability under the parity tolerance), the writers, flag parsing and refusals, and the stand-alone module's argument handling
up to the point where it needs a device."""
import glob
import os

import numpy as np
import pytest

from util import REFT

from ballermixplus_amd import cli, peaks

EX1 = os.path.join(REFT, 'Example1_fullSweep_200kya_DAF.txt')
SPECT = os.path.join(REFT, 'HC_CEU_Neut_DAF_spect_for_B2.txt')
EX2_OUT = os.path.join(REFT, 'output', 'Example2_B2.txt')
EX2_APEXES = {0.005: [2149, 9508, 25768, 34622, 46869], 0.02: [25768]}


# ------------------------------------------------------------------------------------------ nasty tracks and the plain loop

def nasty_track(seed, M):
    """A seeded track built to be nasty: values from a handful of levels (exact ties, plateaus, zeros), runs of equal
    positions, gaps of very different lengths."""
    rng = np.random.default_rng(seed)
    levels = np.array([0.0, 0.0, 0.5, 1.0, 1.0, 2.5, 7.0, 7.0, 12.25, 40.0])[:int(rng.integers(3, 11))]
    c = levels[rng.integers(0, len(levels), M)]
    if M and rng.random() < 0.5:           # plateaus: runs of one value
        run = rng.integers(1, 9, M)
        c = np.repeat(c, run)[:M]
    step = rng.choice([0.0, 0.0, 1e-4, 1e-3, 0.05], M) * rng.random(M)
    if M and rng.random() < 0.3:
        step[rng.integers(0, M, max(M // 50, 1))] += 1.0         # long quiet stretches
    g = np.cumsum(step) + float(rng.random())
    return np.ascontiguousarray(g), np.ascontiguousarray(c, dtype=np.float64)


def nasty_params(seed, g, c):
    """(G, C, F) of a nasty case: G from 0 to beyond the whole span, C from none to above the maximum, F up to 1."""
    rng = np.random.default_rng(seed + 77)
    span = float(g[-1] - g[0]) if len(g) else 1.0
    G = [0.0, 1e-4, 0.01, span / 7, span, 2 * span + 1][int(rng.integers(0, 6))]
    top = float(c.max()) if len(c) else 1.0
    C = [0.0, 0.0, 1.0, top, top + 1][int(rng.integers(0, 5))]
    F = [0.5, 1.0, 0.25, 0.9][int(rng.integers(0, 4))]
    return G, C, F


def brute(g, c, G, C, F):
    """The definition, sentence by sentence, in O(M^2)."""
    M = len(g)
    rows = []
    for t in range(M):
        if not (c[t] > 0 and c[t] >= C):
            continue
        beaten = False
        for s in range(M):
            if s != t and g[t] - g[s] <= G and g[s] - g[t] <= G and (c[s] > c[t] or (c[s] == c[t] and s < t)):
                beaten = True
                break
        if not beaten:
            rows.append(t)
    K = len(rows)
    sad = [-1] * (K + 1)
    for i in range(K - 1):
        best = -1
        for s in range(rows[i] + 1, rows[i + 1]):
            if best < 0 or c[s] < c[best]:
                best = s
        sad[i + 1] = best
    lo, hi = [], []
    for i, a in enumerate(rows):
        thr = F * c[a]
        floor = 0 if i == 0 else (sad[i] + 1 if sad[i] >= 0 else rows[i - 1] + 1)
        ceil = M - 1 if i == K - 1 else (sad[i + 1] - 1 if sad[i + 1] >= 0 else rows[i + 1] - 1)
        l = h = a
        while l - 1 >= floor and c[l - 1] >= thr:
            l -= 1
        while h + 1 <= ceil and c[h + 1] >= thr:
            h += 1
        lo.append(l)
        hi.append(h)
    return {'row': rows, 'lo': lo, 'hi': hi, 'saddle_lo': sad[:-1], 'saddle_hi': sad[1:]}


def same(pk, want):
    return all(np.array_equal(np.asarray(pk[k], dtype=np.int64), np.asarray(want[k], dtype=np.int64)) for k in peaks.FIELDS)


def check_properties(g, c, G, C, F, pk):
    row, lo, hi = (pk[k].astype(np.int64) for k in ('row', 'lo', 'hi'))
    sl, sh = pk['saddle_lo'].astype(np.int64), pk['saddle_hi'].astype(np.int64)
    assert np.all(np.diff(row) > 0)
    assert np.all(c[row] > 0) and np.all(c[row] >= C)
    assert np.all(g[row][1:] - g[row][:-1] > G)                      # more than G apart
    assert np.all(lo <= row) and np.all(row <= hi)                   # every apex inside its region
    assert np.all(hi[:-1] < lo[1:])                                  # regions disjoint
    assert np.all((sl < 0) | (sl < lo)) and np.all((sh < 0) | (sh > hi))      # ... and strictly inside the saddles
    assert np.array_equal(sl[1:], sh[:-1])
    assert np.all((sh[:-1] >= 0) == (row[1:] > row[:-1] + 1))
    if len(row):
        assert sl[0] == -1 and sh[-1] == -1
    for i in range(len(row)):
        assert np.all(c[lo[i]:hi[i] + 1] >= F * c[row[i]])
    if len(c) and c.max() > 0 and c.max() >= C:
        assert int(np.argmax(c)) in row.tolist()                      # the global maximum's first row


# ------------------------------------------------------------------------------------------------------- the definition

@pytest.mark.parametrize('block', range(6))
def test_host_restatement_against_the_definition(block):
    apex = 0
    for seed in range(block * 60, block * 60 + 60):
        M = [0, 1, 2, 3, 17, 64, 65, 130, 257][seed % 9]
        g, c = nasty_track(seed, M)
        G, C, F = nasty_params(seed, g, c)
        pk = peaks.call(g, c, G, C, F)
        want = brute(g, c, G, C, F)
        assert same(pk, want), (seed, M, G, C, F)
        check_properties(g, c, G, C, F, pk)
        apex += len(pk['row'])
    assert apex > 30


def test_special_cases():
    g = np.arange(10) * 0.1
    c = np.array([1., 3., 3., 3., 1., 0., 2., 2., 5., 5.])
    pk = peaks.call(g, c, 0.25, 0.0, 0.5)
    assert pk['row'].tolist() == [1, 8]                              # plateaus yield their first row; 6 is beaten by 8
    assert pk['saddle_hi'].tolist() == [5, -1] and pk['lo'].tolist() == [1, 8] and pk['hi'].tolist() == [3, 9]
    # not greedy clumping: 6 (c = 2) lies within G of 8 only, 8 is an apex, 6 is not -- and stays none when 8 is itself beaten
    c2 = c.copy()
    c2[9] = 6.0
    assert peaks.call(g, c2, 0.25)['row'].tolist() == [1, 9]
    assert peaks.call(g, c, 0.0)['row'].tolist() == [0, 1, 2, 3, 4, 6, 7, 8, 9]          # G = 0, distinct positions: every row > 0
    same_pos = np.zeros(10)
    assert peaks.call(same_pos, c, 0.0)['row'].tolist() == [8]        # G = 0 still merges rows at the same position
    assert peaks.call(g, c, 100.0)['row'].tolist() == [8]
    assert peaks.call(g, c, 0.25, 5.5)['row'].tolist() == []          # C above the maximum
    assert peaks.call(g, c, 0.25, 5.0)['row'].tolist() == [8]
    full = peaks.call(g, c, 0.25, 0.0, 1.0)                            # F = 1: the plateau of the apex
    assert full['lo'].tolist() == [1, 8] and full['hi'].tolist() == [3, 9]
    adj = peaks.call(np.arange(4.0), np.array([2., 1., 1., 2.]), 0.0, 0.0, 0.25)       # adjacent apexes: no saddle, own rows
    assert adj['row'].tolist() == [0, 1, 2, 3] and adj['saddle_hi'].tolist() == [-1, -1, -1, -1]
    assert adj['lo'].tolist() == [0, 1, 2, 3] and adj['hi'].tolist() == [0, 1, 2, 3]
    for M in (0, 1):
        e = peaks.call(np.zeros(M), np.ones(M), 1.0)
        assert e['row'].tolist() == list(range(M)) and e['lo'].tolist() == e['hi'].tolist() == list(range(M))
    with pytest.raises(ValueError):
        peaks.call(np.array([1.0, 0.5]), np.ones(2), 1.0)             # unsorted positions
    for bad in ((-1.0, 0.0, 0.5), (float('nan'), 0.0, 0.5), (1.0, float('nan'), 0.5), (1.0, 0.0, 0.0), (1.0, 0.0, 1.5),
                (1.0, 0.0, float('nan'))):
        with pytest.raises(ValueError):
            peaks.call(g, c, *bad)
    assert peaks.ranks([3.0, 7.0, 3.0, 9.0]).tolist() == [3, 2, 4, 1]


# ------------------------------------------------------------------------------------------- the reference's Example 2

def test_reference_example2_fixture():
    lines, idx, g, c = peaks.read_track(EX2_OUT)
    assert len(g) == len(lines) - 1 == 1184
    phys = np.array([int(lines[j].split('\t')[0]) for j in idx])
    for G, want in EX2_APEXES.items():
        pk = peaks.call(g, c, G, 10.0)
        assert phys[pk['row']].tolist() == want
    pk = peaks.call(g, c, 0.005, 10.0)
    top = pk['row'][peaks.ranks(c[pk['row']]) == 1][0]
    assert phys[top] == 25768 and lines[idx[top]].split('\t')[2].startswith('283.06')
    assert len(peaks.call(g, c, 0.001, 10.0)['row']) == 9
    # the sets do not move under the project's parity tolerance (1e-6 relative on the CLR): the GPU's own scan of
    # Example 2 therefore has the same apex positions (tests/test_gpu_peaks.py)
    rng = np.random.default_rng(11)
    for G in (0.005, 0.02, 0.001):
        base = peaks.call(g, c, G, 10.0)['row'].tolist()
        for _ in range(20):
            c2 = c * (1.0 + rng.uniform(-1e-6, 1e-6, len(c)))
            assert peaks.call(g, c2, G, 10.0)['row'].tolist() == base


# ---------------------------------------------------------------------------------------------------------- writers

def _main_file(path, rows):
    with open(path, 'w') as f:
        f.write('physPos\tgenPos\tCLR\tx_hat\ts_hat\tA_hat\tnSites\n')
        f.writelines('\t'.join(r) + '\n' for r in rows)


def test_writer_format_and_na_rows(tmp_path):
    rows = [['100', '0.001', '1.5', '0.3', '10', '500', '7'],
            ['150', '0.0015', '0', 'NA', 'NA', 'NA', '0'],              # an NA row: not part of the track
            ['200', '0.002', '9.25', '0.3', '10', '500', '9'],
            ['300', '0.003', '4.0', '0.4', '1', '200', '9'],
            ['400', '0.004', '0.0', '0.0', '0.0', '0.0', '0.0'],
            ['500', '0.005', '6.5', '0.5', '5', '100', '4'],
            ['600', '0.006', '6.5', '0.5', '5', '100', '4']]
    main = str(tmp_path / 'o.txt')
    _main_file(main, rows)
    lines, idx, g, c = peaks.read_track(main)
    assert idx.tolist() == [1, 3, 4, 5, 6, 7] and c.tolist() == [1.5, 9.25, 4.0, 0.0, 6.5, 6.5]
    pk = peaks.call(g, c, 0.0015, 0.0, 0.5)
    assert pk['row'].tolist() == [1, 4]
    out = peaks.write_peaks(peaks.output_name(main), main, pk, idx)
    got = open(main + '.peaks.txt').read().split('\n')
    assert got[0] + '\n' == peaks.HEADER and got[-1] == '' and len(got) == 4
    assert len(peaks.HEADER.rstrip('\n').split('\t')) == 17
    assert got[1].split('\t') == rows[2] + ['1', '200', '200', '0.002', '0.002', '1', 'NA', '0.0', 'NA', 'NA']
    assert got[2].split('\t') == rows[5] + ['2', '500', '600', '0.005', '0.006', '2', '0.0', 'NA', 'NA', 'NA']
    assert out == [l.split('\t') for l in got[1:3]]
    # p-values: the apex's columns of the p-value file, as text
    with open(main + '.pval.txt', 'w') as f:
        f.write('physPos\tgenPos\tCLR\tp_site\tp_genome\n')
        f.writelines('%s\t%s\t%s\t0.%d\t0.0%d\n' % (r[0], r[1], r[2], j + 1, j + 1) if r[3] != 'NA' else
                     '%s\t%s\t%s\tNA\tNA\n' % (r[0], r[1], r[2]) for j, r in enumerate(rows))
    peaks.write_peaks(peaks.output_name(main), main, pk, idx, main + '.pval.txt')
    got = open(main + '.peaks.txt').read().split('\n')
    assert got[1].split('\t')[15:] == ['0.3', '0.03'] and got[2].split('\t')[15:] == ['0.6', '0.06']
    # no apex: the header only
    peaks.write_peaks(peaks.output_name(main), main, peaks.call(g, c, 1.0, 100.0), idx)
    assert open(main + '.peaks.txt').read() == peaks.HEADER
    # genome-wide: every file's rows, by CLR descending, ranked again
    peaks.write_genome(str(tmp_path / 'peaks.txt'), [('a.txt', out), ('b.txt', out)])
    gw = [l.split('\t') for l in open(tmp_path / 'peaks.txt').read().split('\n')[:-1]]
    assert '\t'.join(gw[0]) + '\n' == 'file\t' + peaks.HEADER
    assert [(r[0], r[1], r[8]) for r in gw[1:]] == [('a.txt', '200', '1'), ('b.txt', '200', '2'), ('a.txt', '500', '3'), ('b.txt', '500', '4')]
    assert all(r[1:8] + r[9:] == out[0][:7] + out[0][8:] for r in gw[1:3])


# ------------------------------------------------------------------------------------------------------------ flags

def test_flags_off_by_default_and_parsed():
    opt = cli.build_parser().parse_args(['-i', EX1, '--spect', SPECT])
    assert opt.peaks is None and opt.peakMin is None and opt.peakExtent is None and not opt.atPeaks
    assert cli.peaks_refusal(opt) is None
    opt = cli.build_parser().parse_args(['-i', EX1, '--spect', SPECT, '-o', 'o', '--refine', '--support', '--boot', '8', '--nullPerm', '3',
                                         '--peaks', '0.005', '--peakMin', '10', '--peakExtent', '0.25', '--atPeaks'])
    assert (opt.peaks, opt.peakMin, opt.peakExtent, opt.atPeaks) == (0.005, 10.0, 0.25, True)
    assert cli.peaks_refusal(opt) is None
    opt = cli.build_parser().parse_args(['-i', EX1, '--spect', SPECT, '-o', 'o', '--peaks', '0'])
    assert cli.peaks_refusal(opt) is None


@pytest.mark.parametrize('extra,env,word', [
    (['--peaks', '0.01'], {}, '-o'),
    (['--peaks', '0.01', '-o', 'OUT', '--getSpect'], {}, '--getSpect'),
    (['--peaks', '0.01', '-o', 'OUT', '--getConfig'], {}, '--getConfig'),
    (['--peaks', '0.01', '-o', 'OUT'], {'WORLD_SIZE': '2'}, 'multi-rank'),
    (['--peaks', '0.01', '-o', 'OUT'], {'BMX_FORCE_DIST': '1'}, 'multi-rank'),
    (['--peaks', '-1', '-o', 'OUT'], {}, '--peaks'),
    (['--peaks', 'nan', '-o', 'OUT'], {}, '--peaks'),
    (['--peaks', '0.01', '--peakMin', 'nan', '-o', 'OUT'], {}, '--peakMin'),
    (['--peaks', '0.01', '--peakExtent', '0', '-o', 'OUT'], {}, '--peakExtent'),
    (['--peaks', '0.01', '--peakExtent', '1.01', '-o', 'OUT'], {}, '--peakExtent'),
    (['--peaks', '0.01', '--peakExtent', 'nan', '-o', 'OUT'], {}, '--peakExtent'),
    (['--peaks', '0.01', '--atPeaks', '-o', 'OUT'], {}, '--refine'),
    (['--peakMin', '3', '-o', 'OUT'], {}, '--peakMin'),
    (['--peakExtent', '0.5', '-o', 'OUT'], {}, '--peakExtent'),
    (['--atPeaks', '--refine', '-o', 'OUT'], {}, '--atPeaks'),
    # refused in this feature's name although another addition would refuse it too
    (['--peaks', '0.01', '--nullPerm', '3'], {}, '--peaks'),
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
    assert word in said and ('--peak' in said or '--atPeaks' in said)
    assert not made and not glob.glob(str(tmp_path / '*'))


@pytest.mark.parametrize('argv,word', [
    (['OUT', '--peaks', '-0.5'], '--peaks'),
    (['OUT', '--peaks', 'nan'], '--peaks'),
    (['OUT', '--peaks', '0.01', '--peakMin', 'nan'], '--peakMin'),
    (['OUT', '--peaks', '0.01', '--peakExtent', '2'], '--peakExtent'),
    (['MISSING', '--peaks', '0.01'], 'No such output file'),
    (['NOTMAIN', '--peaks', '0.01'], 'not a main output'),
    (['UNSORTED', '--peaks', '0.01'], 'non-decreasing'),
])
def test_standalone_arguments(argv, word, tmp_path, monkeypatch, capsys):
    from ballermixplus_amd import engine
    made = []
    monkeypatch.setattr(engine, 'Context', lambda *a, **k: made.append(1))
    files = {'OUT': str(tmp_path / 'o.txt'), 'MISSING': str(tmp_path / 'none.txt'), 'NOTMAIN': str(tmp_path / 'n.txt'),
             'UNSORTED': str(tmp_path / 'u.txt')}
    _main_file(files['OUT'], [['1', '0.1', '2.0', '0.3', '10', '500', '7']])
    _main_file(files['UNSORTED'], [['1', '0.2', '2.0', '0.3', '10', '500', '7'], ['2', '0.1', '2.0', '0.3', '10', '500', '7']])
    with open(files['NOTMAIN'], 'w') as f:
        f.write('replicate\tmaxCLR\n0\t1.0\n')
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(SystemExit) as e:
        peaks.main([files.get(a, a) for a in argv])
    assert e.value.code == 1
    assert word in capsys.readouterr().out
    assert not made and sorted(os.listdir(tmp_path)) == before


def test_standalone_needs_the_separation(tmp_path, capsys):
    main = str(tmp_path / 'o.txt')
    _main_file(main, [['1', '0.1', '2.0', '0.3', '10', '500', '7']])
    with pytest.raises(SystemExit) as e:
        peaks.main([main])
    assert e.value.code == 2 and '--peaks' in capsys.readouterr().err


def test_standalone_without_track_rows_writes_the_header(tmp_path, monkeypatch):
    from ballermixplus_amd import engine
    monkeypatch.setattr(engine, 'Context', lambda *a, **k: pytest.fail('no device is needed for an empty track'))
    main = str(tmp_path / 'o.txt')
    _main_file(main, [['150', '0.0015', '0', 'NA', 'NA', 'NA', '0']])
    peaks.main([main, '--peaks', '0.01'])
    assert open(main + '.peaks.txt').read() == peaks.HEADER
