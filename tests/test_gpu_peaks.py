"""Peak calling on the GPU (--peaks): the kernels against the host restatement of peaks.py -- exactly, there is no tolerance in
this feature -- on nasty uploaded tracks and after real scans, call order and errors, and the CLI: nothing else it writes
changes, the peak file is the writer fed with the host restatement, the stand-alone module reproduces it, --atPeaks restricts
the refinement (and with it support intervals and bootstrap) to the apexes without changing their rows."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_refine import REPO, _cli, _engine, _read, _synth
from test_peaks_cpu import EX2_APEXES, check_properties, nasty_params, nasty_track
from util import REFT

from ballermixplus_amd import boot, peaks, refine, support
from ballermixplus_amd._lib import BmxError

pytestmark = pytest.mark.gpu

EX2 = ['-i', os.path.join(REFT, 'Example2_balancing_10MYA_DAF.txt'), '--spect', os.path.join(REFT, 'HC_CEU_Neut_DAF_spect_for_B2.txt')]


def _same(got, want, what):
    for k in peaks.FIELDS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (what, k, got[k][:8], want[k][:8])


def _check_track(ctx, g, c, G, C, F, what):
    got = ctx.peaks_track(g, c, G, C, F)
    want = peaks.call(g, c, G, C, F)
    print('%s: M = %d, G = %r, C = %r, F = %r: %d apexes (host %d), %.3f ms' % (what, len(g), G, C, F, len(got['row']), len(want['row']),
                                                                           ctx.peaks_ms()))
    _same(got, want, what)
    return got


# ---------------------------------------------------------------------------------------------------- uploaded tracks

def test_small_nasty_tracks_match_the_host_exactly():
    ctx = _engine().Context(0)
    apex = 0
    for seed in range(240):
        M = [0, 1, 2, 3, 17, 63, 64, 65, 127, 128, 129, 257, 1000, 4097][seed % 14]
        g, c = nasty_track(seed, M)
        G, C, F = nasty_params(seed, g, c)
        pk = _check_track(ctx, g, c, G, C, F, 'seed %d' % seed)
        check_properties(g, c, G, C, F, pk)
        apex += len(pk['row'])
    assert apex > 200
    ctx.close()


@pytest.mark.parametrize('M', [200003, 1 << 20, 2500037])
def test_large_tracks_and_every_kind_of_radius(M):
    """Radii that span no full tile, exactly one tile, many tiles, more tiles than a workgroup stages and the whole track;
    M a multiple of 64 and not."""
    ctx = _engine().Context(0)
    g, c = nasty_track(M, M)
    # positions on a regular lattice make a radius' extent in rows exact: 64 rows either side is one whole tile at most
    lattice = np.arange(M) * 0.5
    rng = np.random.default_rng(M)
    smooth = np.convolve(rng.random(M + 400), np.ones(401) / 401, 'valid')[:M] + 1e-3 * rng.integers(0, 4, M)
    span = float(g[-1] - g[0])
    for what, gg, cc, G, C, F in (
            ('lattice, 20 rows', lattice, c, 10.0, 0.0, 0.5), ('lattice, one tile', lattice, c, 32.0, 1.0, 0.5),
            ('lattice, 640 rows', lattice, smooth, 320.0, 0.0, 0.9), ('lattice, 100k rows', lattice, smooth, 50000.0, 0.0, 0.99),
            ('whole track', g, c, 2 * span + 1, 0.0, 0.5), ('whole lattice', lattice, smooth, float(M), 0.0, 0.5),
            ('nasty, span / 1000', g, c, span / 1000, 1.0, 0.25), ('nasty, G = 1e-4', g, c, 1e-4, 0.0, 1.0)):
        pk = _check_track(ctx, gg, cc, G, C, F, what)
        assert len(pk['row']) >= 1
    # apexes in the first and in the last tile; one value everywhere: the first row
    c2 = smooth.copy()
    c2[3] = c2[M - 2] = 10.0
    pk = _check_track(ctx, lattice, c2, 1000.0, 0.0, 0.5, 'first and last tile')
    assert pk['row'][0] == 3 and pk['row'][-1] == M - 2
    pk = _check_track(ctx, lattice, np.ones(M), float(M), 0.0, 1.0, 'one plateau')
    assert pk['row'].tolist() == [0] and pk['hi'].tolist() == [M - 1]
    if M <= 300000:
        _check_track(ctx, lattice, c, 0.0, 0.0, 0.5, 'G = 0: every positive row')
    ctx.close()


def test_errors_and_call_order():
    eng = _engine()
    ctx = eng.Context(0)
    g, c = np.arange(5.0), np.array([1., 2., 1., 3., 1.])
    with pytest.raises(BmxError) as e:
        ctx.fetch_peaks()
    assert e.value.code == -5
    for bad in ((float('nan'), 0, 0.5), (-1.0, 0, 0.5), (1.0, float('nan'), 0.5), (1.0, 0, 0.0), (1.0, 0, 1.5), (1.0, 0, float('nan'))):
        with pytest.raises(BmxError) as e:
            ctx.peaks_track(g, c, *bad)
        assert e.value.code == -1
    for gg, cc in ((g[::-1], c), (g, np.array([1., np.nan, 1., 1., 1.])), (np.array([0., 1., np.inf, np.inf, np.inf]), c)):
        with pytest.raises(BmxError) as e:
            ctx.peaks_track(gg, cc, 1.0)
        assert e.value.code == -1
    with pytest.raises(BmxError) as e:
        ctx.peaks(1.0)                        # no scan yet
    assert e.value.code == -1 and 'scan' in str(e.value)
    assert ctx.peaks_track(g, c, 1.0)['row'].tolist() == [1, 3]
    assert ctx.peaks_track(g[:0], c[:0], 1.0)['row'].tolist() == []
    ctx.close()
    # after a scan: unsorted test positions are refused; a refinement restricted to apexes needs a peak call on that scan
    ctx, gen, rows, _ = _synth(20000)
    tg = gen[::50][:200]
    ctx.set_tests(tg[::-1].copy())
    ctx.scan()
    with pytest.raises(BmxError) as e:
        ctx.peaks(0.001)
    assert e.value.code == -1 and 'non-decreasing' in str(e.value)
    ctx.set_tests(tg)
    ctx.scan()
    ctx.refine_at_peaks(True)
    with pytest.raises(BmxError) as e:
        ctx.refine(0.0)
    assert e.value.code == -1 and 'peak' in str(e.value)
    ctx.peaks_track(g, c, 1.0)               # a track is not a peak call on the scan
    with pytest.raises(BmxError):
        ctx.refine(0.0)
    pk = ctx.peaks(0.01)                      # (test sites every ~0.0036: a few rows either side)
    assert 0 < len(pk['row']) < len(tg) // 2
    ctx.refine(0.0)
    assert np.array_equal(np.nonzero(ctx.fetch_refined()['rounds'] >= 0)[0], pk['row'])
    ctx.scan()                                # a new scan: the peak call is of the previous one
    with pytest.raises(BmxError):
        ctx.refine(0.0)
    ctx.refine_at_peaks(False)
    ctx.refine(0.0)
    assert (ctx.fetch_refined()['rounds'] >= 0).sum() > len(pk['row'])
    ctx.close()


# ---------------------------------------------------------------------------------------------------- after real scans

@pytest.mark.parametrize('N', [20000, 1000000])
def test_peaks_of_real_scans(N):
    ctx, gen, rows, _ = _synth(N)
    plans = set()
    for step in (1, 6, 20):
        tg = gen[::step]
        ctx.select_slot(0)
        ctx.set_tests(tg)
        plan = ctx.plan()
        plans.add((plan['mode'], plan['J']))
        ctx.scan()
        clr = ctx.fetch()[0]
        for G, C, F in ((0.0005, 0.0, 0.5), (0.01, float(np.quantile(clr, 0.9)), 0.25), (float(tg[-1]), 0.0, 1.0)):
            got = ctx.peaks(G, C, F)
            print('N = %d, stride %d (%s), G = %r: %d apexes, %.3f ms, scan %.2f ms' % (N, step, plan['kernel'], G, len(got['row']),
                                                                                   ctx.peaks_ms(), ctx.last_scan_ms()))
            _same(got, peaks.call(tg, clr, G, C, F), (N, step, G))
            assert len(got['row']) >= 1
        if step == 6:
            # a second slot in between: its peaks are its own, and slot 0's are still there afterwards
            keep = ctx.fetch_peaks()
            ctx.select_slot(1)
            ctx.set_sites(gen[:5000], rows[:5000])
            ctx.set_tests(gen[:5000:3])
            ctx.scan()
            _same(ctx.peaks(0.001), peaks.call(gen[:5000:3], ctx.fetch()[0], 0.001), 'slot 1')
            ctx.select_slot(0)
            _same(ctx.fetch_peaks(), keep, 'slot 0 again')
    assert plans == {(4, 16), (4, 8), (5, 1)}
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- CLI

def _lines(p):
    with open(p) as f:
        return f.readlines()


def _host_peak_file(main, G, C, F, pval=None):
    """The writer fed with the host restatement of the run's own main output."""
    lines, idx, g, c = peaks.read_track(main)
    tmp = main + '.host_peaks.txt'
    peaks.write_peaks(tmp, main, peaks.call(g, c, G, C, F), idx, pval)
    data = _read(tmp)
    os.remove(tmp)
    return data


def test_cli_peaks_on_example2(tmp_path):
    plain, pk, pn = (str(tmp_path / n) for n in ('plain.txt', 'pk.txt', 'pn.txt'))
    _cli(EX2 + ['-o', plain])
    _cli(EX2 + ['-o', pk, '--peaks', '0.005', '--peakMin', '10'])
    assert _read(plain) == _read(pk)
    assert sorted(os.listdir(tmp_path)) == ['pk.txt', 'pk.txt.peaks.txt', 'plain.txt']
    table = _read(peaks.output_name(pk))
    assert table == _host_peak_file(pk, 0.005, 10.0, 0.5)
    rows = [l.rstrip('\n').split('\t') for l in _lines(peaks.output_name(pk))]
    assert '\t'.join(rows[0]) + '\n' == peaks.HEADER
    assert [int(r[0]) for r in rows[1:]] == EX2_APEXES[0.005]
    assert [r[0] for r in rows[1:] if r[7] == '1'] == ['25768']
    main = _lines(pk)
    assert all('\t'.join(r[:7]) + '\n' in main for r in rows[1:])
    assert all(r[15:] == ['NA', 'NA'] for r in rows[1:]) and rows[1][13] == 'NA' and rows[-1][14] == 'NA'
    # the stand-alone module on that output: the same bytes
    os.remove(peaks.output_name(pk))
    r = subprocess.run([sys.executable, '-m', 'ballermixplus_amd.peaks', pk, '--peaks', '0.005', '--peakMin', '10'], capture_output=True,
                       text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stdout + r.stderr
    assert _read(peaks.output_name(pk)) == table
    for G, want in ((0.02, EX2_APEXES[0.02]), (0.001, None)):
        r = subprocess.run([sys.executable, '-m', 'ballermixplus_amd.peaks', pk, '--peaks', repr(G), '--peakMin', '10', '--peakExtent', '0.25'],
                           capture_output=True, text=True, timeout=600, cwd=REPO)
        assert r.returncode == 0, r.stdout + r.stderr
        assert _read(peaks.output_name(pk)) == _host_peak_file(pk, G, 10.0, 0.25)
        got = [int(l.split('\t')[0]) for l in _lines(peaks.output_name(pk))[1:]]
        assert got == want if want is not None else len(got) == 9
    # with the null: its files do not change, and the p columns are the apex rows of the p-value file
    _cli(EX2 + ['-o', plain, '--nullPerm', '3'])
    _cli(EX2 + ['-o', pn, '--nullPerm', '3', '--peaks', '0.005', '--peakMin', '10'])
    for ext in ('', '.null.txt', '.pval.txt'):
        assert _read(plain + ext) == _read(pn + ext), ext
    assert _read(peaks.output_name(pn)) == _host_peak_file(pn, 0.005, 10.0, 0.5, pn + '.pval.txt')
    pv = {l.split('\t')[0]: l.rstrip('\n').split('\t')[3:5] for l in _lines(pn + '.pval.txt')[1:]}
    rows = [l.rstrip('\n').split('\t') for l in _lines(peaks.output_name(pn))[1:]]
    assert len(rows) == 5 and all(r[15:] == pv[r[0]] and 'NA' not in r[15:] for r in rows)
    # a floor above every CLR: the header only
    _cli(EX2 + ['-o', pk, '--peaks', '0.005', '--peakMin', '1e9'])
    assert _read(peaks.output_name(pk)) == peaks.HEADER.encode()


def test_cli_at_peaks(tmp_path):
    every, at = (str(tmp_path / n) for n in ('every.txt', 'at.txt'))
    extra = ['-s', '3', '--refine', '--refineMin', '14', '--support', '--boot', '6', '--bootBlock', '16', '--peaks', '0.002']
    _cli(EX2 + ['-o', every] + extra)
    _cli(EX2 + ['-o', at] + extra + ['--atPeaks'])
    assert _read(every) == _read(at) and _read(peaks.output_name(every)) == _read(peaks.output_name(at))
    # without --atPeaks nothing of the refinement changes with --peaks
    ref = str(tmp_path / 'ref.txt')
    _cli(EX2 + ['-o', ref] + extra[:-2])
    for name in (refine.output_name, support.output_name, boot.output_name):
        assert _read(name(ref)) == _read(name(every)), name(ref)
    main = _lines(at)
    _, idx, g, c = peaks.read_track(at)
    apex = set((idx[peaks.call(g, c, 0.002)['row']]).tolist())
    done = {j for j in apex if float(main[j].split('\t')[2]) >= 14.0}
    assert len(apex) > len(done) >= 3
    changed = 0
    for name, other in ((refine.output_name, 'main'), (support.output_name, 'NA'), (boot.output_name, 'NA')):
        a, b = _lines(name(every)), _lines(name(at))
        assert len(a) == len(b) == len(main) and a[0] == b[0]
        for j in range(1, len(main)):
            if j in done:
                assert a[j] == b[j], (name(at), j)              # a window's search does not depend on which others are done
                changed += name is refine.output_name and b[j] != main[j]
            elif other == 'main':
                assert b[j] == main[j], j
            else:
                assert set(b[j].rstrip('\n').split('\t')[2:]) == {'NA'}, (name(at), j)
        if other == 'NA':
            assert all(b[j].split('\t')[2] != 'NA' for j in done), name(at)
    assert changed >= 1


def test_at_peaks_refines_exactly_the_apexes_above_the_floor():
    ctx, gen, rows, _ = _synth(20000)
    ctx.set_tests(gen[::2])
    ctx.scan()
    clr, _, _, iA, _ = ctx.fetch()
    cut = float(np.quantile(clr, 0.5))
    ctx.refine(cut)
    free = ctx.fetch_refined()
    pk = ctx.peaks(0.0004)
    ctx.refine_at_peaks(True)
    ctx.refine(cut)
    r = ctx.fetch_refined()
    want = pk['row'][(clr[pk['row']] >= cut) & (iA[pk['row']] >= 0)]
    assert 0 < len(want) < len(pk['row'])
    assert np.array_equal(np.nonzero(r['rounds'] >= 0)[0], want)
    for k in ('clr', 'A', 'x', 'abeta', 'nsites', 'rounds'):
        assert np.array_equal(r[k][want], free[k][want]), k
    rest = np.setdiff1d(np.arange(len(clr)), want)
    assert np.array_equal(r['clr'][rest], clr[rest])
    ctx.close()


def test_cli_three_files(tmp_path):
    spect = EX2[3]
    third = tmp_path / 'Example3_copy_of_1.txt'
    third.write_bytes(_read(os.path.join(REFT, 'Example1_fullSweep_200kya_DAF.txt')))
    ins = [os.path.join(REFT, 'Example1_fullSweep_200kya_DAF.txt'), EX2[1], str(third)]
    lst = tmp_path / 'inputs.txt'
    lst.write_text('\n'.join(ins) + '\n')
    d1, d2 = tmp_path / 'plain', tmp_path / 'peaks'
    d1.mkdir()
    d2.mkdir()
    _cli(['--inputs', str(lst), '--spect', spect, '-o', str(d1), '-s', '2', '--nullPerm', '2'])
    _cli(['--inputs', str(lst), '--spect', spect, '-o', str(d2), '-s', '2', '--nullPerm', '2', '--peaks', '0.0002', '--peakMin', '5'])
    outs = sorted(os.listdir(d1))
    assert sorted(f for f in os.listdir(d2) if 'peaks' not in f) == outs
    for f in outs:
        assert _read(d1 / f) == _read(d2 / f), f
    mains = [os.path.basename(p) + '.out.txt' for p in ins]
    merged = []
    for name, m in zip(ins, mains):
        path = str(d2 / m)
        assert _read(peaks.output_name(path)) == _host_peak_file(path, 0.0002, 5.0, 0.5, path + '.pval.txt')
        rows = [l.rstrip('\n').split('\t') for l in _lines(peaks.output_name(path))[1:]]
        assert len(rows) >= 1
        merged += [[os.path.basename(name)] + r for r in rows]
    assert len(merged) >= 10
    gw = [l.rstrip('\n').split('\t') for l in _lines(d2 / 'peaks.txt')]
    assert '\t'.join(gw[0]) + '\n' == 'file\t' + peaks.HEADER
    assert [r[8] for r in gw[1:]] == [str(k + 1) for k in range(len(merged))]
    clr = [float(r[3]) for r in gw[1:]]
    assert clr == sorted(clr, reverse=True)
    strip = lambda r: r[:8] + r[9:]
    assert sorted(map(strip, gw[1:])) == sorted(map(strip, merged))
    # files 0 and 2 hold the same data: equal CLR, file order decides
    first = [r for r in gw[1:] if r[0] in (os.path.basename(ins[0]), os.path.basename(ins[2]))]
    assert [r[0] for r in first[:2]] == [os.path.basename(ins[0]), os.path.basename(ins[2])] and strip(first[0])[1:] == strip(first[1])[1:]
