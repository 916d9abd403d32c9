"""The delete-block jackknife of a window's CLR (--influence) without a GPU: the host restatement against real deletion of the
block, the rule that skips an A without sites, the per-window summary on hand-written arrays, the files, the flags and every
refusal, the prototypes, and the argmax margins of the cases the GPU tests compare on."""
import glob
import math
import os

import numpy as np
import pytest

import influencecases as ic
from util import REFT

from ballermixplus_amd import _lib, cli, influence, surfaces

EX1 = os.path.join(REFT, 'Example1_fullSweep_200kya_DAF.txt')
SPECT = os.path.join(REFT, 'HC_CEU_Neut_DAF_spect_for_B2.txt')
ZCUT = 18.420680743952364


# ------------------------------------------------------------------------------------- the restatement against deletion

def _random_chromosome(seed, N, nrows):
    rng = np.random.default_rng(seed)
    g = np.sort(np.round(rng.uniform(0, 1.0, N), 2 if seed % 2 else 6))           # two decimals: many position ties
    rows = rng.integers(0, nrows, N)
    R = rng.uniform(-0.6, 1.5, (3, 2, nrows))
    return g, rows, R


def _brute(g, rows, R, A, tg, lo, hi, B, b):
    """L_b by deleting block b from the arrays: the scan-rule maximum of host_surface on what is left of the window."""
    a, e = max(lo, 0), min(hi, len(g) - 1)
    keep = np.ones(len(g), dtype=bool)
    keep[b * B:(b + 1) * B] = False
    inside = np.zeros(len(g), dtype=bool)
    inside[a:e + 1] = True
    sub = keep & inside
    T, ns = surfaces.host_surface(g[sub], rows[sub], R, A, tg, 0, int(sub.sum()) - 1, ZCUT)
    return influence.scan_argmax(T)[:2], T


def _abs_terms(g, rows, R, A, tg, lo, hi, lin):
    """2 sum_i |log1p term| of the window at the linear grid index lin (0 for lin < 0)."""
    if lin < 0:
        return 0.0
    npairs = R.shape[0] * R.shape[1]
    a, e = max(lo, 0), min(hi, len(g) - 1)
    z = A[lin // npairs] * np.abs(g[a:e + 1] - tg)
    keep = (z <= ZCUT) & (g[a:e + 1] != tg)
    return 2.0 * float(np.sum(np.abs(np.log1p(np.exp(-z[keep]) * R.reshape(npairs, -1)[lin % npairs][rows[a:e + 1][keep]]))))


@pytest.mark.parametrize('seed,N,nrows', [(1, 300, 13), (2, 211, 34), (3, 97, 51), (4, 300, 5)])
def test_host_influence_against_deleting_the_block(seed, N, nrows):
    g, rows, R = _random_chromosome(seed, N, nrows)
    A = [40.0, 700.0, 90.0, 5000.0]
    rng = np.random.default_rng(seed + 100)
    worst = 0.0
    for w in range(4):
        tg = float(g[rng.integers(0, N)]) if w % 2 == 0 else float(rng.uniform(0, 1))      # at a site (g == tg excluded), or off-site
        lo, hi = (0, N - 1) if w < 2 else (int(rng.integers(0, N // 2)), int(rng.integers(N // 2, N + 20)))
        for B in (1, 2, 7, N + 5):
            h = influence.host_influence(g, rows, R, A, tg, lo, hi, ZCUT, B)
            T, ns = surfaces.host_surface(g, rows, R, A, tg, lo, hi, ZCUT)
            assert np.array_equal(h['T'], T, equal_nan=True) and (h['T_max'], h['lin']) == influence.scan_argmax(T)[:2]
            assert h['ns_min'] == ns[0] == ns.max()
            assert len(h['m']) == len(h['L']) == len(h['contrib']) == len(h['blin']) == len(h['margin'])
            if B > N:
                assert len(h['m']) == 1 and h['first_block'] == 0 and h['L'][0] == 0 and h['blin'][0] == -1
            for j in range(len(h['m'])):
                b = h['first_block'] + j
                (Lb, lb), Tb = _brute(g, rows, R, A, tg, lo, hi, B, b)
                # both sides are numpy sums of the same terms: only the order differs
                scale = 1e-12 * max(_abs_terms(g, rows, R, A, tg, lo, hi, l) for l in (h['blin'][j], lb, h['lin']))
                assert abs(h['L'][j] - Lb) <= scale, (w, B, b, h['L'][j], Lb)
                worst = max(worst, abs(h['L'][j] - Lb))
                if h['margin'][j] > 2 * scale:
                    assert h['blin'][j] == lb, (w, B, b)
                if h['lin'] >= 0:
                    full = h['T'].reshape(-1)[h['lin']]
                    without = Tb.reshape(-1)[h['lin']]
                    if not np.isnan(without):
                        assert abs(h['contrib'][j] - (full - without)) <= scale
    print('largest |L_b - deletion| = %.3e' % worst)


def test_an_A_that_keeps_no_site_is_skipped():
    """The largest A holds only the three sites next to the test position, all in block 1, and carries the full maximum (the
    sites further out lower pair 0's likelihood at the small A).  Without block 1 that A has no site left: it is absent from
    block 1's candidates, and L_1 comes from the small A."""
    g = np.array([0.40, 0.42, 0.44, 0.46, 0.499, 0.5, 0.501, 0.502, 0.55, 0.58])
    rows = np.array([1, 1, 1, 1, 0, 0, 0, 0, 1, 1])
    R = np.array([[[3.0, -0.9], [-0.5, 0.2]]])         # pair 0: the near sites (row 0) raise it, the far ones lower it; pair 1: the reverse
    A = [10.0, 1000.0]                                 # A = 1000 reaches |d| <= 0.0184: sites 4, 6 and 7 (site 5 is the test position)
    h = influence.host_influence(g, rows, R, A, 0.5, 0, 9, ZCUT, 4)
    T, ns = surfaces.host_surface(g, rows, R, A, 0.5, 0, 9, ZCUT)
    assert ns.tolist() == [9, 3] and h['ns_min'] == 9
    assert h['lin'] == 2 and h['T_max'] == T[1, 0, 0] > T[0, 0, 0] > 0          # the full argmax sits at the large A
    assert h['first_block'] == 0 and h['m'].tolist() == [4, 3, 2]
    # blocks 0 and 2 have no site at the large A: their candidate there is T itself.  It wins for block 2; without block 0's four
    # lowering sites pair 0 at the small A is higher still
    assert h['L'][2] == h['T_max'] and h['blin'][2] == 2
    S0 = np.sum(np.log1p(np.exp(-10.0 * np.abs(g[:4] - 0.5)) * -0.9))
    assert h['blin'][0] == 0 and abs(h['L'][0] - (T[0, 0, 0] - 2.0 * S0)) <= 1e-14 and h['L'][0] > h['T_max']
    assert h['contrib'][0] == h['contrib'][2] == 0.0 and abs(h['contrib'][1] - h['T_max']) <= 1e-14 * h['T_max']
    # block 1: only the small A is a candidate; pair 1 without the near sites is what is left of it
    far = np.array([0, 1, 2, 3, 8, 9])
    want = 2.0 * np.sum(np.log1p(np.exp(-10.0 * np.abs(g[far] - 0.5)) * 0.2))
    assert h['blin'][1] == 1 and want > 0 and abs(h['L'][1] - want) <= 1e-14
    # were the large A a candidate of block 1, its value T - 2 S_b would be a rounding residue of either sign: give it one
    h2 = influence.host_influence(g, rows, np.array([[[3.0, -0.9]]]), A, 0.5, 0, 9, ZCUT, 4)
    assert h2['lin'] == 1 and h2['blin'][1] == -1 and h2['L'][1] == 0.0 and h2['margin'][1] > 1.0


# ---------------------------------------------------------------------------------------------------------- summarise

def test_summarise_by_hand():
    s = influence.summarise(10.0, 7, 4, [2, 0, 3, 1], [6.0, np.nan, 3.0, 1.0], [4.0, 10.0, 7.0, 9.0], [7, 7, 5, 7])
    assert s['nBlocks'] == 3                                   # the block with m = 0 is dropped
    mean = (4.0 + 7.0 + 9.0) / 3
    assert s['jk_se'] == math.sqrt(2 / 3 * ((4 - mean) ** 2 + (7 - mean) ** 2 + (9 - mean) ** 2))
    assert s['n_half'] == 1 and s['share_max'] == 0.6 and s['n_moved'] == 1
    assert (s['drop'], s['drop_block'], s['drop_nSites'], s['drop_share'], s['CLR_drop'], s['drop_lin']) == (0, 4, 2, 0.6, 4.0, 7)
    # n_half by hand: 4, 3, 3 of 12 -> 4 + 3 = 7 >= 6: two blocks; with equal contributions the earlier block is taken first
    s = influence.summarise(12.0, 0, 0, [1, 1, 1], [3.0, 4.0, 3.0], [9.0, 8.0, 9.0], [0, 0, 0])
    assert s['n_half'] == 2 and s['n_moved'] == 0 and s['drop'] == 1
    # ties of L: the earliest block is the drop block
    s = influence.summarise(12.0, 0, 10, [1, 2, 1], [5.0, 5.0, 2.0], [7.0, 7.0, 10.0], [0, 3, 0])
    assert (s['drop'], s['drop_block'], s['drop_nSites'], s['drop_lin']) == (0, 10, 1, 0) and s['n_half'] == 2
    # negative contributions: the sum may never reach half (n_half NA), shares may be negative
    s = influence.summarise(4.0, 2, 0, [1, 1], [-1.0, 1.5], [5.0, 2.5], [2, 2])
    assert s['n_half'] is None and s['share_max'] == 0.375 and s['drop'] == 1 and s['drop_share'] == 0.375
    s = influence.summarise(4.0, 2, 0, [1, 1, 1], [-1.0, 2.5, 2.5], [5.0, 1.5, 1.5], [2, 2, 2])
    assert s['n_half'] == 1 and s['drop'] == 1
    # one block: no spread
    s = influence.summarise(4.0, 2, 0, [5], [4.0], [0.0], [-1])
    assert s['nBlocks'] == 1 and s['jk_se'] is None and s['n_half'] == 1 and s['drop_lin'] == -1 and s['n_moved'] == 1
    # no block, or no maximum: NA from nBlocks on
    for s in (influence.summarise(0.0, -1, 0, [1, 1], [np.nan, np.nan], [0.0, 0.0], [-1, -1]), influence.summarise(3.0, 1, 0, [0], [0.0], [3.0], [1]),
              influence.summarise(3.0, 1, 0, [], [], [], [])):
        assert s['drop'] is None and s['jk_se'] is None and s['n_half'] is None


class _Sel:
    grid_A = [2000.0, 100.0]
    grid_x = [0.5, 0.05, 0.25]
    grid_abeta = [10, 0.01]


def test_files_headers_na_rows_and_round_trip(tmp_path):
    assert influence.HEADER.rstrip('\n').split('\t') == (
        'physPos genPos CLR T_max nBlocks jk_se n_half share_max n_moved drop_lo_physPos drop_hi_physPos drop_nSites drop_share '
        'CLR_drop x_drop s_drop A_drop').split()
    assert influence.BLOCKS_HEADER.rstrip('\n').split('\t') == 'physPos genPos block lo_physPos hi_physPos nSites contrib CLR_without x_hat s_hat A_hat'.split()
    assert influence.grid_strings(-1, _Sel) == ('NA', 'NA', 'NA')
    assert influence.grid_strings(9, _Sel) == ('0.05', '0.01', '100.0')        # lin = (1 * 3 + 1) * 2 + 1
    position = np.arange(100, 1100, 100)
    m, c, L, bl = [2, 0, 1], [0.1 + 0.2, np.nan, 1.0], [5.0, 7.0, 0.0], [9, 3, -1]
    s = influence.summarise(7.0, 3, 1, m, c, L, bl)
    row = influence.summary_row('500', '0.0005', '7.5', 7.0, s, position, 3, _Sel).rstrip('\n').split('\t')
    assert len(row) == 17 and row[:4] == ['500', '0.0005', '7.5', '7.0'] and row[4] == '2'
    assert row[9:12] == ['1000', '1000', '1'] and row[13:] == ['0.0', 'NA', 'NA', 'NA']      # block 3 = sites 9 .. 11 of 10: clipped
    assert row[7] == repr(1.0 / 7.0) and float(row[5]) == math.sqrt(0.5 * 12.5)
    na = influence.summary_row('500', '0.0005', '0.0', 0.0, influence.summarise(0.0, -1, 0, [], [], [], []), position, 3, _Sel)
    assert na == '500\t0.0005\t0.0\t0.0' + '\tNA' * 13 + '\n'
    rows = influence.block_rows('500', '0.0005', 1, m, c, L, bl, position, 3, _Sel)
    assert [r.rstrip('\n').split('\t') for r in rows] == [
        ['500', '0.0005', '1', '400', '600', '2', '0.30000000000000004', '5.0', '0.05', '0.01', '100.0'],
        ['500', '0.0005', '3', '1000', '1000', '1', '1.0', '0.0', 'NA', 'NA', 'NA']]
    path = str(tmp_path / 't.txt')
    with open(path, 'w') as f:
        f.write(influence.BLOCKS_HEADER)
        f.writelines(rows)
    head, back = influence.read_table(path)
    assert head == influence.BLOCKS_HEADER.rstrip('\n').split('\t') and [float(r[6]) for r in back] == [0.1 + 0.2, 1.0]
    assert influence.output_name('a/b.txt') == 'a/b.txt.influence.txt' and influence.blocks_name('a/b.txt') == 'a/b.txt.influence.blocks.txt'


class _FakeCtx:
    def __init__(self, clr):
        self.clr, self.calls = np.asarray(clr, dtype=np.float64), []

    def fetch(self):
        z = np.zeros(len(self.clr), dtype=np.int32)
        return self.clr, z, z, z, z

    def influence(self, tests, B):
        self.calls.append((list(tests), B))
        n = len(tests)
        return {'T_max': np.asarray(tests, dtype=np.float64), 'lin': np.zeros(n, np.int32), 'ns_min': np.ones(n, np.int32),
                'first_block': np.zeros(n, np.int64), 'offset': np.arange(n + 1, dtype=np.int64), 'm': np.ones(n, np.int32),
                'contrib': np.asarray(tests, dtype=np.float64), 'L': np.zeros(n), 'blin': np.full(n, -1, np.int32)}


def test_influence_and_write_selects_and_batches(tmp_path):
    from ballermixplus_amd import scan as scanmod
    ts = scanmod.TestSites()
    ts.add_many(np.arange(10) * 100, np.arange(10) * 1e-4, np.arange(10) * 1e-4, np.zeros(10, int), np.full(10, 9))

    class Data:
        position = np.arange(10) * 100

    ctx = _FakeCtx([1, 8, 3, 9, 0, 6, 7, 2, 5, 4])
    out = str(tmp_path / 'o.txt')
    # every window's index range touches 5 blocks of two sites: 10 blocks hold two windows
    assert influence.influence_and_write(ctx, out, ts, _Sel, Data, 2, 3.0, 5, None, True, host_blocks=10) == (5, 2)
    assert ctx.calls == [([1, 3], 2), ([5, 6], 2), ([8], 2)]
    head, rows = influence.read_table(influence.output_name(out))
    assert head[0] == 'physPos' and [r[0] for r in rows] == ['100', '300', '500', '600', '800'] and [r[3] for r in rows] == ['1.0', '3.0', '5.0', '6.0', '8.0']
    assert [r[2] for r in rows] == ['8.0', '9.0', '6.0', '7.0', '5.0'] and all(r[4] == '1' and r[5] == 'NA' for r in rows)
    assert len(influence.read_table(influence.blocks_name(out))[1]) == 5
    os.remove(influence.blocks_name(out))
    assert influence.influence_and_write(ctx, out, ts, _Sel, Data, 1, 50.0) == (0, 0)
    assert open(influence.output_name(out)).read() == influence.HEADER and not os.path.exists(influence.blocks_name(out))
    assert influence.influence_and_write(ctx, out, scanmod.TestSites(), _Sel, Data, 1, 0.0, detail=True) == (0, 0)
    assert open(influence.blocks_name(out)).read() == influence.BLOCKS_HEADER


# ------------------------------------------------------------------------------------------------ flags and refusals

def test_flags_off_by_default_and_parsed():
    opt = cli.build_parser().parse_args(['-i', EX1, '--spect', SPECT])
    assert opt.influence is False and opt.influenceDetail is False
    assert (opt.influenceBlock, opt.influenceMin, opt.influenceMax) == (None, None, None) and cli.influence_refusal(opt) is None
    opt = cli.build_parser().parse_args(['-i', EX1, '--spect', SPECT, '-o', 'o', '--influence', '--influenceBlock', '8', '--influenceMin', '2.5',
                                         '--influenceMax', '7', '--influenceDetail', '-w', '50'])
    assert (opt.influence, opt.influenceBlock, opt.influenceMin, opt.influenceMax, opt.influenceDetail) == (True, 8, 2.5, 7, True)
    assert cli.influence_refusal(opt) is None                   # every window mode is allowed
    opt = cli.build_parser().parse_args(['-i', EX1, '--spect', SPECT, '-o', 'o', '--influence', '--peaks', '0.01', '--surfaces', '--nullPerm', '2'])
    assert cli.influence_refusal(opt) is None
    assert (influence.MAX_WINDOWS, influence.MAX_RESULTS) == (1000, 1 << 26)


O = ['-o', 'OUT']
OK = ['--influence', '--influenceMin', '5'] + O
WHICH = ('--influence needs --peaks G (the jackknife of the apexes) or --influenceMin C (of the windows with CLR >= C): '
         'the jackknife of every window of a chromosome is never what is meant.')
HELPER = '--influence scans the input; it cannot be combined with --getSpect / --getConfig.'
RANKS = '--influence runs in a single process; multi-rank launches are not supported.'
NO_O = '--influence needs -o: the influence file is written next to the output.'

ROWS = [
    (['--influenceBlock', '3'] + O, {}, '--influenceBlock needs --influence.'),
    (['--influenceMin', '3'] + O, {}, '--influenceMin needs --influence.'),
    (['--influenceMax', '3'] + O, {}, '--influenceMax needs --influence.'),
    (['--influenceDetail'] + O, {}, '--influenceDetail needs --influence.'),
    (OK + ['--getSpect'], {}, HELPER),
    (OK + ['--getConfig'], {}, HELPER),
    (OK[:-2], {}, NO_O),
    (OK, {'WORLD_SIZE': '2'}, RANKS),
    (OK, {'BMX_FORCE_DIST': '1'}, RANKS),
    (['--influence'] + O, {}, WHICH),
    (['--influence', '--influenceMax', '5'] + O, {}, WHICH),
    (OK + ['--influenceBlock', '0'], {}, '--influenceBlock must be >= 1.'),
    (OK + ['--influenceBlock', '-2'], {}, '--influenceBlock must be >= 1.'),
    (OK + ['--influenceMax', '0'], {}, '--influenceMax takes a number of windows >= 1.'),
    (['--influence', '--influenceMin', 'nan'] + O, {}, '--influenceMin takes a number.'),
    # two faults: a value before the selection, the selection before helper mode and -o, -o before the ranks
    (['--influence', '--influenceBlock', '0'], {}, '--influenceBlock must be >= 1.'),
    (['--influence', '--getSpect'], {}, WHICH),
    (OK[:-2], {'WORLD_SIZE': '2'}, NO_O),
    # the other features speak first
    (['--influence', '--surfaces'] + O, {}, '--surfaces needs --peaks G (the surfaces of the apexes) or --surfaceMin C (of the windows with '
                                            'CLR >= C): the surface of every window of a chromosome is never what is meant.'),
    (['--influence', '--peaks', '0.01'], {}, '--peaks needs -o: the peak file is written next to the output.'),
    (['--influence', '--refineMin', '3'] + O, {}, '--refineMin needs --refine.'),
]


@pytest.mark.parametrize('tail,env,message', ROWS, ids=[' '.join(t) + ''.join(' %s=%s' % kv for kv in e.items()) for t, e, _ in ROWS])
def test_refusal_message(tail, env, message, tmp_path, monkeypatch, capsys):
    from ballermixplus_amd import engine
    made = []
    monkeypatch.setattr(engine, 'Context', lambda *a, **k: made.append(1))
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.delenv('BMX_FORCE_DIST', raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    argv = ['-i', EX1, '--spect', SPECT] + [str(tmp_path / 'o.txt') if a == 'OUT' else a for a in tail]
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 1
    assert capsys.readouterr().out == message + '\n'
    assert not made and not glob.glob(str(tmp_path / '*'))


def test_refused_the_same_with_several_inputs(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(['-i', EX1 + ',' + EX1, '--spect', SPECT, '-o', str(tmp_path / 'd'), '--influence'])
    assert e.value.code == 1 and capsys.readouterr().out == WHICH + '\n'
    assert not glob.glob(str(tmp_path / '*'))


def test_prototypes_of_the_new_symbols():
    for name in ('bmx_ctx_influence', 'bmx_ctx_influence_count', 'bmx_ctx_fetch_influence', 'bmx_ctx_influence_ms'):
        assert name in _lib.PROTOTYPES
        fn = getattr(_lib.lib(), name)
        assert fn.argtypes == _lib.PROTOTYPES[name][1]
    with open(os.path.join(os.path.dirname(_lib.__file__), '..', 'include', 'bmxscan.h')) as f:
        head = f.read()
    assert '#define BMX_INFLUENCE_MAX_RESULTS (1LL << 26)' in head and '#define BMX_ABI_VERSION_MINOR 5' in head
    for name in ('bmx_ctx_influence(', 'bmx_ctx_influence_count(', 'bmx_ctx_fetch_influence(', 'bmx_ctx_influence_ms('):
        assert 'int ' + name in head


# ------------------------------------------------------------------------------------------- the catalogue's margins

@pytest.mark.parametrize('name', ic.NAMES)
def test_margins_of_the_gpu_cases_are_wide(name):
    """The GPU test compares lin_b only where the host's margin exceeds twice its tolerance; that must leave nearly every block:
    at most 1 % of a case's blocks may have so small a margin."""
    from ballermixplus_amd import engine
    cat = ic.catalogue(engine)[name]()
    narrow = total = 0
    for w in cat.windows:
        for B in ic.BLOCKS:
            h = cat.host(w, B)
            tol = ic.tolerance(h['T'])
            narrow += int(np.sum(h['margin'] <= 2 * tol))
            total += len(h['margin'])
    print('%s: %d of %d blocks with a margin <= twice the tolerance' % (name, narrow, total))
    assert total > 0 and narrow <= 0.01 * total, (narrow, total)
