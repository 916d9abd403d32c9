"""--sandwich on the host: the restatement against a literal per-site loop, the analytic u-score against a numerical derivative of
the oracle's T, the identities of the definition (B = 1, replicated sites, one block), summarise() on hand-made matrices, the
`unstable` rule, the writer, the CLI's refusals, the default steps, and the margins of the catalogue of sandwichcases.py.  The
tables are the oracle's (sel_table); nothing here needs a GPU."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import sandwichcases as sc
from util import REFT, REPO, oracle_R, orc

from ballermixplus_amd import refine, sandwich


def _summary(h, c, p):
    return sandwich.summarise(h['T'], h['g'], h['H'], h['J'], sc.setup_of(c), c.points[p])


# ------------------------------------------------------------------------------------------------- the restatement

@pytest.mark.parametrize('name,block', [('one', 1), ('one', 7), ('three', 64), ('skip', 2)])
def test_host_sandwich_against_a_literal_loop(name, block):
    c = sc.case(name)
    for q in range(0, len(c.entries), 4 if name != 'skip' else 1):
        w, p = c.entries[q]
        if c.points[p][0] < 100.0 and c.hi[w] - c.lo[w] > 2000:
            continue                                        # the whole chromosome in a Python loop: the windows of 1 000 suffice
        tabs = sc.oracle_tabs(c, p)
        h = sc.host(c, q, tabs, block)
        T, g, H, J, ns, nsk, nb = sc.literal(c, q, tabs, block)
        assert (h['nsites'], h['nskipped'], h['nblocks']) == (ns, nsk, nb), (name, q)
        assert h['T'] == T or abs(h['T'] - T) <= 1e-13 * h['absT'], (name, q)
        for got, want, scale in ((h['g'], g, h['absg']), (h['H'], H, h['absH']), (h['J'], J, h['absJ'])):
            assert np.all(np.abs(got - np.array(want)) <= 1e-13 * scale), (name, q)


def test_the_u_score_is_the_derivative_of_T_in_ln_A():
    """g_u = sum of the analytic u-scores against (T(A e^h) - T(A e^-h)) / (2 h) / 2 of the oracle's T on a window the index
    bounds cut (its membership does not move with A)."""
    c = sc.case('one')
    for q in (9, 15, 21):                                   # windows of 63, 65 and 256 sites at the grid point (A = 700)
        w, p = c.entries[q]
        assert p == 0 and w in (3, 5, 7) and sc.SIZES[w] in (63, 65, 256)
        A, x, ab = c.points[p]
        tabs = sc.oracle_tabs(c, p)
        h = sc.host(c, q, tabs, 1)

        def T(Av):
            z = Av * np.abs(c.gen - c.tg[w])
            keep = (z <= sc.ZCUT) & (c.gen != c.tg[w]) & (np.arange(len(c.gen)) >= c.lo[w]) & (np.arange(len(c.gen)) <= c.hi[w])
            assert keep.sum() == h['nsites']
            return float(np.sum(np.log1p(np.exp(-z[keep]) * tabs[0][c.rows[keep]])))

        e = 1e-5
        num = (T(A * math.exp(e)) - T(A * math.exp(-e))) / (2 * e)
        print('entry %d: analytic %.12g, numerical %.12g' % (q, h['g'][0], num))
        assert abs(h['g'][0] - num) <= 1e-7 * h['absg'][0]


@pytest.mark.parametrize('name', sc.NAMES)
def test_block_one_gives_J_equal_to_H(name):
    c = sc.case(name)
    for q in range(len(c.entries)):
        h = sc.host(c, q, sc.oracle_tabs(c, c.entries[q][1]), 1)
        assert np.array_equal(h['J'], h['H']) and h['nblocks'] == h['nsites'] - h['nskipped']


def test_a_single_block_gives_J_equal_to_g_gT():
    c = sc.case('three')
    for q in (10, 28, 30):
        h = sc.host(c, q, sc.oracle_tabs(c, c.entries[q][1]), 10 ** 6)
        assert h['nblocks'] == 1
        want = np.array([h['g'][k] * h['g'][l] for k, l in sandwich.SYM])
        assert np.all(np.abs(h['J'] - want) <= 1e-13 * h['absJ'])


def test_replicated_sites():
    """Every site four times, blocks of four: J = 4 H, every eigenvalue of H^-1 J is 4, se = 2 se_naive."""
    c = sc.case('one')
    m = 4
    gen, rows, lo, hi = sc.replicated(c, m)
    for q in (9, 19, 27, 31):
        w, p = c.entries[q]
        tabs = sc.oracle_tabs(c, p)
        h = sandwich.host_sandwich(gen, rows, tabs, c.points[p][0], c.tg[w], lo[w], hi[w], m, zcut=sc.ZCUT)
        one = sc.host(c, q, tabs, 1)
        assert h['nsites'] == m * one['nsites'] and h['nblocks'] == one['nblocks']
        s = _summary(h, c, p)
        assert s['status'] == 'ok'
        assert np.all(np.abs(s['eigenvalues'] - 4.0) <= 1e-9), s['eigenvalues']
        assert abs(s['lambda_mean'] - 4.0) <= 1e-9 and abs(s['lambda_max'] - 4.0) <= 1e-9
        for k in s['kept']:
            assert abs(s['se'][k] - 2.0 * s['se_naive'][k]) <= 1e-9 * s['se'][k]


# ---------------------------------------------------------------------------------------------------------- summarise

SETUP = refine.Setup([10.0, 100.0, 1000.0], [0.1, 0.3, 0.5], [1.0, 10.0, 100.0])
INSIDE = (100.0, 0.3, 10.0)


def _six(M):
    return [M[k][l] for k, l in sandwich.SYM]


def test_summarise_on_hand_made_matrices():
    H = np.diag([4.0, 25.0, 100.0])
    s = sandwich.summarise(30.0, [0.0, 0.0, 0.0], _six(H), _six(H), SETUP, INSIDE)                   # J = H
    assert s['status'] == 'ok' and s['kept'] == (0, 1, 2) and s['on_hull'] == ()
    assert np.allclose(s['se'], [0.5, 0.2, 0.1], rtol=1e-14) and np.allclose(s['se_naive'], s['se'], rtol=1e-14)
    assert abs(s['lambda_mean'] - 1.0) <= 1e-14 and abs(s['lambda_max'] - 1.0) <= 1e-14 and abs(s['CLR_adj'] - 30.0) <= 1e-12
    assert s['grad_norm'] == 0.0
    s = sandwich.summarise(30.0, [2.0, 0.0, 0.0], _six(H), _six(4.0 * H), SETUP, INSIDE)             # J = 4 H
    assert np.allclose(s['se'], [1.0, 0.4, 0.2], rtol=1e-14) and np.allclose(s['se_naive'], [0.5, 0.2, 0.1], rtol=1e-14)
    assert abs(s['lambda_mean'] - 4.0) <= 1e-13 and abs(s['lambda_max'] - 4.0) <= 1e-13 and abs(s['CLR_adj'] - 7.5) <= 1e-12
    assert abs(s['grad_norm'] - 1.0) <= 1e-14                                                        # sqrt(2 * 2 / 4)
    # a full matrix against numpy on the same numbers
    rng = np.random.default_rng(3)
    X, Y = rng.normal(size=(40, 3)), rng.normal(size=(12, 3))
    Hf, Jf, g = X.T @ X, Y.T @ Y, rng.normal(size=3)
    s = sandwich.summarise(10.0, g, _six(Hf), _six(Jf), SETUP, INSIDE)
    Hi = np.linalg.inv(Hf)
    assert np.allclose(s['se'], np.sqrt(np.diag(Hi @ Jf @ Hi)), rtol=1e-10)
    lam = np.sort(np.linalg.eigvals(Hi @ Jf).real)
    assert abs(s['lambda_max'] - lam[-1]) <= 1e-10 * lam[-1] and abs(s['lambda_mean'] - lam.mean()) <= 1e-10 * lam[-1]
    assert abs(s['grad_norm'] - math.sqrt(g @ Hi @ g)) <= 1e-10
    # singular: a rank-one H, a zero diagonal entry, no kept coordinate
    v = np.array([1.0, 2.0, 3.0])
    for Hs in (np.outer(v, v), np.diag([1.0, 0.0, 1.0])):
        s = sandwich.summarise(10.0, g, _six(Hs), _six(Jf), SETUP, INSIDE)
        assert s['status'] == 'singular' and s['se'] == [None] * 3 and s['lambda_mean'] is None and s['CLR_adj'] is None
    one = refine.Setup([100.0], [0.3], [10.0])
    assert sandwich.summarise(10.0, g, _six(Hf), _six(Jf), one, INSIDE)['status'] == 'singular'
    # T = -inf: no CLR_adj, the rest stands
    s = sandwich.summarise(-math.inf, g, _six(Hf), _six(Jf), SETUP, INSIDE)
    assert s['status'] == 'ok' and s['CLR_adj'] is None


def test_every_coordinate_on_the_hull_or_fixed():
    rng = np.random.default_rng(4)
    X, Y = rng.normal(size=(40, 3)), rng.normal(size=(12, 3))
    Hf, Jf, g = X.T @ X, Y.T @ Y, rng.normal(size=3)
    for k in range(3):
        for end in (0, 2):
            grids = ([10.0, 100.0, 1000.0], [0.1, 0.3, 0.5], [1.0, 10.0, 100.0])
            point = list(INSIDE)
            point[k] = grids[k][end]
            s = sandwich.summarise(10.0, g, _six(Hf), _six(Jf), SETUP, tuple(point))
            rest = tuple(j for j in range(3) if j != k)
            assert s['on_hull'] == (k,) and s['kept'] == rest and s['se'][k] is None and s['se_naive'][k] is None
            at = np.ix_(rest, rest)
            Hi = np.linalg.inv(Hf[at])
            assert np.allclose([s['se'][j] for j in rest], np.sqrt(np.diag(Hi @ Jf[at] @ Hi)), rtol=1e-10)
            assert abs(s['lambda_mean'] - np.trace(Hi @ Jf[at]) / 2) <= 1e-10
        fixed = [[10.0, 100.0, 1000.0], [0.1, 0.3, 0.5], [1.0, 10.0, 100.0]]
        fixed[k] = [INSIDE[k]]
        s = sandwich.summarise(10.0, g, _six(Hf), _six(Jf), refine.Setup(*fixed), INSIDE)
        assert s['on_hull'] == () and s['kept'] == tuple(j for j in range(3) if j != k) and s['se'][k] is None
    # a refined point that came back through exp onto the hull is on it
    A_hi = math.exp(math.log(1000.0) * (1 - 1e-16))
    assert sandwich.kept_coordinates(SETUP, (A_hi, 0.3, 10.0)) == ((1, 2), (0,))


def test_the_unstable_rule():
    H = np.diag([4.0, 25.0, 100.0])
    first = sandwich.summarise(30.0, [0.0] * 3, _six(H), _six(H), SETUP, INSIDE)
    for factor, status in ((1.0, 'ok'), (1.2, 'ok'), (1.2099, 'ok'), (1.2101, 'unstable'), (0.8, 'unstable'), (0.82, 'ok')):
        second = sandwich.summarise(30.0, [0.0] * 3, _six(H), _six(factor * H), SETUP, INSIDE)         # se scales by sqrt(factor)
        rel = sandwich.fd_rel(first, second)
        assert abs(rel - abs(math.sqrt(factor) - 1.0)) <= 1e-12
        assert sandwich.status_of(first, rel) == status, factor
    sing = sandwich.summarise(30.0, [0.0] * 3, _six(np.zeros((3, 3))), _six(H), SETUP, INSIDE)
    assert sandwich.fd_rel(sing, first) is None and sandwich.status_of(sing, None) == 'singular'
    assert sandwich.fd_rel(first, sing) == math.inf and sandwich.status_of(first, math.inf) == 'unstable'
    # only one coordinate moves: the largest change counts
    second = sandwich.summarise(30.0, [0.0] * 3, _six(H), _six(np.diag([4.0, 25.0, 169.0])), SETUP, INSIDE)
    assert abs(sandwich.fd_rel(first, second) - 0.3) <= 1e-12


# ------------------------------------------------------------------------------------------------------------- writer

def _call(c, entries, block, hx, hv):
    hs = [sc.host(c, q, sc.oracle_tabs(c, c.entries[q][1], hx, hv), block, hx, hv) for q in entries]
    out = {k: np.array([h[k] for h in hs]) for k in ('T', 'g', 'H', 'J', 'nsites', 'nskipped', 'nblocks')}
    return out


def test_the_writer(tmp_path):
    c = sc.case('one')
    entries = [0, 10, 27, 28]
    first, second = _call(c, entries, 7, sandwich.HX, sandwich.HV), _call(c, entries, 7, 2 * sandwich.HX, 2 * sandwich.HV)
    points = [c.points[c.entries[q][1]] for q in entries]
    strings = [(repr(x), repr(ab), repr(A)) for A, x, ab in points]
    rows = sandwich.rows_of(['1', '2', '3', '4'], ['0.1', '0.2', '0.3', '0.4'], ['5.0', '6.0', '7.0', '8.0'], strings,
                            ['grid', 'refined', 'grid', 'refined'], points, sc.setup_of(c), first, second)
    out = str(tmp_path / 'o.txt')
    sandwich.write_sandwich(out, rows)
    names, got = sandwich.read_table(sandwich.output_name(out))
    assert '\t'.join(names) + '\n' == sandwich.HEADER and len(names) == 23 and len(got) == 4 and all(len(r) == 23 for r in got)
    assert got[0][:11] == ['1', '0.1', '5.0', '0.3', '10.0', '700.0', '0', '0', '0', 'grid', '.'] and got[0][11:] == ['NA'] * 11 + ['singular']
    r = got[1]                                  # A = 50 is the hull's lower end
    s1 = _summary({k: first[k][1] for k in first}, c, 1)
    assert r[9:11] == ['refined', 'lnA'] and r[13] == 'NA' and r[16] == 'NA' and r[22] == 'ok'
    assert r[11] == repr(s1['se'][1]) and r[12] == repr(s1['se'][2]) and r[14] == repr(s1['se_naive'][1]) and r[17] == repr(s1['lambda_mean'])
    assert r[19] == repr(float(first['T'][1]) / s1['lambda_mean']) and r[6:9] == ['63', '0', '10'] and float(r[21]) < 0.1
    assert got[2][10] == '.' and got[2][22] == 'ok' and 'NA' not in got[2]
    for r in got[1:]:
        assert float(r[17]) <= float(r[18]) * (1 + 1e-12) and float(r[11]) > 0
    # a file without a window: the header only
    empty = str(tmp_path / 'e.txt')
    sandwich.write_sandwich(empty, [])
    assert open(sandwich.output_name(empty)).read() == sandwich.HEADER


def test_a_point_too_close_to_the_ends_of_x_is_refused_before_the_file_exists(tmp_path):
    """x_hat within 2 hx of 0: ValueError, and no <out>.sandwich.txt is left behind; nothing is asked of the device."""
    class Sel:
        grid_A, grid_x, grid_abeta = [10.0, 100.0], [0.0015, 0.3], [1.0, 10.0]

    class Ctx:
        def fetch(self):
            return (np.array([5.0, 7.0]), np.array([0, 1], dtype=np.int32), np.array([0, 1], dtype=np.int32),
                    np.array([0, 1], dtype=np.int32), np.array([9, 9], dtype=np.int32))

        def sandwich(self, *a):
            raise AssertionError('the device was asked')

    out = str(tmp_path / 'o.txt')
    with pytest.raises(ValueError) as e:
        sandwich.sandwich_and_write(Ctx(), out, [0, 1], Sel, min_clr=0.0)
    assert 'sandwichStep' in str(e.value) and not os.path.exists(sandwich.output_name(out))
    assert sandwich.sandwich_and_write(Ctx(), out, [], Sel) == (0, 0) and open(sandwich.output_name(out)).read() == sandwich.HEADER


# ----------------------------------------------------------------------------------------------------------- refusals

EX1 = ['-i', os.path.join(REFT, 'Example1_fullSweep_200kya_DAF.txt'), '--spect', os.path.join(REFT, 'HC_CEU_Neut_DAF_spect_for_B2.txt')]


def _refused(args):
    from ballermixplus_amd import cli
    opt = cli.build_parser().parse_args(args)
    return cli.sandwich_refusal(opt)


def test_value_refusal_and_steps():
    assert sandwich.value_refusal(None, None, None, None) is None and sandwich.value_refusal(8, 0.0, 5, '1e-3,1e-2') is None
    assert 'sandwichBlock' in sandwich.value_refusal(0, None, None, None)
    assert 'sandwichMin' in sandwich.value_refusal(None, float('nan'), None, None)
    assert 'sandwichMax' in sandwich.value_refusal(None, None, 0, None)
    for bad in ('1e-3', '1e-3,1e-2,3', 'a,b', '0,1e-2', '1e-3,-1', 'inf,1e-2', '1e-3,nan'):
        assert 'sandwichStep' in sandwich.value_refusal(None, None, None, bad), bad
    assert sandwich.parse_step('0.002,0.02') == (0.002, 0.02)
    pts = sandwich.shifted_points(0.3, 10.0)
    rv = math.exp(sandwich.HV)
    assert pts == ((0.3, 10.0), (0.3 - sandwich.HX, 10.0), (0.3 + sandwich.HX, 10.0), (0.3, 10.0 / rv), (0.3, 10.0 * rv))


def test_cli_refusals(monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.delenv('BMX_FORCE_DIST', raising=False)
    ok = EX1 + ['-o', 'x.txt']
    assert _refused(ok) is None and _refused(ok + ['--sandwich', '--peaks', '0.001']) is None
    assert _refused(ok + ['--sandwich', '--sandwichMin', '3', '--sandwichBlock', '8', '--sandwichMax', '4', '--sandwichStep', '0.002,0.02']) is None
    for flag, val in (('--sandwichBlock', '8'), ('--sandwichMin', '1'), ('--sandwichMax', '5'), ('--sandwichStep', '1e-3,1e-2')):
        assert _refused(ok + [flag, val]) == '%s needs --sandwich.' % flag
    assert _refused(ok + ['--sandwich']).startswith('--sandwich needs --peaks G')
    assert 'sandwichBlock' in _refused(ok + ['--sandwich', '--peaks', '0.001', '--sandwichBlock', '0'])
    assert 'sandwichStep' in _refused(ok + ['--sandwich', '--peaks', '0.001', '--sandwichStep', '0,1'])
    assert 'sandwichMax' in _refused(ok + ['--sandwich', '--peaks', '0.001', '--sandwichMax', '0'])
    assert '-o' in _refused(EX1 + ['--sandwich', '--peaks', '0.001'])
    assert 'getSpect' in _refused(ok + ['--sandwich', '--peaks', '0.001', '--getSpect'])
    monkeypatch.setenv('WORLD_SIZE', '2')
    assert 'single process' in _refused(ok + ['--sandwich', '--peaks', '0.001'])
    monkeypatch.delenv('WORLD_SIZE')
    for mode in (['-w', '100'], ['--usePhysPos', '-w', '1000'], ['--fixWinSize', '-w', '50']):           # every window mode is allowed
        assert _refused(ok + ['--sandwich', '--peaks', '0.001'] + mode) is None


def test_the_command_line_is_refused_before_anything_runs(tmp_path):
    out = str(tmp_path / 'x.txt')
    bad = subprocess.run([sys.executable, os.path.join(REPO, 'BalLeRMixPlus_amd.py')] + EX1 + ['-o', out, '--sandwichBlock', '4'],
                         capture_output=True, text=True, timeout=300, cwd=REPO)
    assert bad.returncode == 1 and bad.stdout.strip() == '--sandwichBlock needs --sandwich.' and not os.path.exists(out)


# ------------------------------------------------------------------------------------------------------ default steps

def _flat_case(x, ab):
    """Five columns at (HX, HV) and at half the steps of n = 100, B_2, min count 1 under the catalogue's spectrum of 'one'."""
    c = sc.case('one')
    cols = lambda hx, hv: np.array([oracle_R('B2', c.sizes, 1, c.spect, c.props, [xx], [aa])[0, 0]
                                    for xx, aa in sandwich.shifted_points(x, ab, hx, hv)])
    return cols(sandwich.HX, sandwich.HV), cols(sandwich.HX / 2, sandwich.HV / 2), sc.g_of(c)


def test_the_default_steps():
    worst = 0.0
    for ab in (0.3, 10.0, 1e3):
        for x in (0.1, 0.3, 0.45):
            tabs, half, g = _flat_case(x, ab)
            for alpha in (1.0, 0.1):
                ex, ev = sc.fd_error(tabs, half, g, sandwich.HX, sandwich.HV, alpha)
                print('alpha_beta %g, x %g, alpha %g: error of Rx %.2e, of Rv %.2e' % (ab, x, alpha, ex, ev))
                worst = max(worst, ex, ev)
    print('worst %.2e' % worst)
    assert worst <= 1e-3
    for name in sc.NAMES:                                   # the catalogue's own points
        c = sc.case(name)
        for p in range(len(c.points)):
            e = sc.fd_error(sc.oracle_tabs(c, p), sc.oracle_tabs(c, p, sandwich.HX / 2, sandwich.HV / 2), sc.g_of(c), sandwich.HX, sandwich.HV)
            print('%s point %d: %.2e %.2e' % (name, p, *e))
            assert max(e) <= 1e-3
            assert c.points[p][2] <= 1e3


# ---------------------------------------------------------------------------------------------- the catalogue's margins

def test_the_catalogue_holds_what_it_claims():
    c = sc.case('one')
    assert len(c.gen) <= 4000 and len(sc.case('three').sizes) == 3 and c.sizes == [100]
    assert np.count_nonzero(np.diff(c.gen) == 0.0) == len(sc.TIES)
    sizes = {}
    for q, (w, p) in enumerate(c.entries):
        h = sc.host(c, q, sc.oracle_tabs(c, p), 1)
        sizes[(w, p)] = h['nsites']
    for j, s in enumerate(sc.SIZES):                        # the index windows, not the cut, at the two smaller A
        assert sizes[(j, 0)] == s and sizes[(j, 1)] == s
    assert 900 <= sizes[(9, 0)] <= 1100 and sizes[(10, 1)] == sc.N and sizes[(9, 1)] == sc.N - 3      # the run of three at the test position
    assert sizes[(8, 2)] < 257                               # ... and the cut at the largest
    # a site at the test position inside a block, range starts off a block boundary
    w = 9
    i = int(np.searchsorted(c.gen, c.tg[w]))
    assert c.gen[i] == c.gen[i + 1] == c.gen[i + 2] == c.tg[w] and any((i + 1) % B not in (0, B - 1) for B in (7, 64, 100))
    starts = [sc.site_range(c, q)[0] for q in range(len(c.entries))]
    for B in (2, 7, 64, 100):
        assert any(a % B for a in starts) and any(a % B == 0 for a in starts)
    assert max(sc.BLOCKS) > sc.N and set(sc.BLOCKS) >= {1, 2, 7, 64, 100}
    assert sc.header_constant('BMX_SANDWICH_MAX_WINDOWS') == 1 << 24 and sc.header_constant('BMX_SANDWICH_CHUNK_WINDOWS') == 1 << 18
    slab = sc.case('slab')
    rows = sum(n + 1 for n in slab.sizes)
    assert rows == 729 and (rows * 45 + 15) // 16 * 16 > 32 * 1024 >= (728 * 45 + 15) // 16 * 16


@pytest.mark.parametrize('name', sc.NAMES)
def test_the_catalogue_is_regular_and_skips_only_where_planned(name):
    c = sc.case(name)
    skipped = 0
    for q, (w, p) in enumerate(c.entries):
        for B in (1, 7):
            h = sc.host(c, q, sc.oracle_tabs(c, p), B)
            skipped += h['nskipped']
            s = _summary(h, c, p)
            if h['nsites'] - h['nskipped'] >= 8:            # (fewer used sites than 2 p + 2 cannot be asked to give a regular H)
                assert s['status'] == 'ok', (name, q, B)
                assert all(s['se'][k] > 0 and s['se_naive'][k] > 0 for k in s['kept'])
            if B == 1 and s['status'] == 'ok':
                assert abs(s['lambda_mean'] - 1.0) <= 1e-9 and all(abs(s['se'][k] - s['se_naive'][k]) <= 1e-9 * s['se'][k] for k in s['kept'])
    assert (skipped > 0) == (name == 'skip')
    if name == 'skip':
        h = sc.host(c, 0, sc.oracle_tabs(c, 0), 1)
        assert h['nskipped'] == 1 and h['nsites'] == 39 and np.all(sc.oracle_tabs(c, 0)[0][1:8] == -1.0)
    # the oracle's normalising bases of these points are all well conditioned: refine_R is held to the plain bar
    excl = orc.excluded_counts('B2', 100, 1)
    for p in range(len(c.points)):
        for x, ab in sandwich.shifted_points(c.points[p][1], c.points[p][2]):
            assert all(orc.norm_base(n, x, ab, orc.excluded_counts('B2', n, 1)) >= 0.05 for n in c.sizes)
    assert len(excl) == 1
