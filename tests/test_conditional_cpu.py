"""Conditional CLRs of neighbouring peaks on the host (--conditional): conditional.host_cond_surface against a literal per-site loop
of the three-way mixture in probability space, the two identities of the definition, the parent rule, the writer, the refusals
and the planted demonstration (one locus and its shoulders against two loci)."""
import glob
import os

import numpy as np
import pytest

import condcases as cc
from util import REFT

from ballermixplus_amd import cli, conditional, influence, surfaces

EX1 = os.path.join(REFT, 'Example1_fullSweep_200kya_DAF.txt')
SPECT = os.path.join(REFT, 'HC_CEU_Neut_DAF_spect_for_B2.txt')

# (candidate test site, conditioning test site, conditioning grid point (iA, ix, ia)) on condcases.small()
PAIRS = [(1, 0, (0, 1, 2)), (1, 3, (1, 0, 1)), (2, 1, (2, 1, 0)), (3, 1, (0, 0, 0)), (0, 4, (0, 1, 1)), (4, 2, (1, 1, 2)), (1, 1, (1, 1, 1)),
         (0, 4, (2, 0, 1))]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))


def _host(c, t, q, point, scale=False):
    iA, ix, ia = point
    return conditional.host_cond_surface(c.gen, c.rows, c.R, c.As, c.tg[t], c.lo[t], c.hi[t], c.tg[q], c.lo[q], c.hi[q], c.As[iA], ix, ia,
                                         cc.zcut(), scale=scale)


# ---------------------------------------------------------------------------------------------------- the literal loop

@pytest.mark.parametrize('t,q,point', PAIRS, ids=['%d|%d@%s' % (t, q, ''.join(map(str, p))) for t, q, p in PAIRS])
def test_restatement_against_the_literal_three_way_mixture(t, q, point):
    c = cc.small()
    assert len(c.gen) == 300 and len(set(c.sizes)) == 2
    T, ns, nsh, S = _host(c, t, q, point, scale=True)
    iA, ix, ia = point
    Tl, nl, nshl, Sl, T3, L = cc.literal_cond(c.gen, c.rows, c.model.g, c.R, c.As, c.tg[t], c.lo[t], c.hi[t], c.tg[q], c.lo[q], c.hi[q],
                                              c.As[iA], ix, ia, cc.zcut())
    assert np.array_equal(ns, nl) and np.array_equal(nsh, nshl)
    assert np.array_equal(np.isnan(T), np.isnan(Tl)) and np.array_equal(np.isnan(T).all(axis=(1, 2)), ns == 0)
    assert (ns > 0).any()
    bound = cc.SITE_TOL * (ns[:, None, None] + Sl)
    ok = ~np.isnan(T)
    worst = np.max(np.abs(T - Tl)[ok] / bound[ok])
    print('pair %d | %d: nsites %s, nshared %s, worst |dT| / bound %.3g' % (t, q, ns.tolist(), nsh.tolist(), worst))
    assert worst <= 1.0
    assert np.all(np.abs(S - 2.0 * Sl)[ok] <= bound[ok])
    # identity 2: T_cond + 2 sum log1p(d_i) is the three-way mixture against neutrality
    assert np.all(np.abs(T + L[:, None, None] - T3)[ok] <= bound[ok])


def test_some_pair_shares_sites_and_some_term_cancels():
    """The cases mean something: shared sites at every A for one pair, none for another, and a conditional surface that differs
    from the unconditional one."""
    c = cc.small()
    shared = [_host(c, t, q, p)[2] for t, q, p in PAIRS]
    assert any((s > 0).all() for s in shared) and any((s > 0).any() and (s == 0).any() for s in shared)
    T = _host(c, 1, 0, (0, 1, 2))[0]
    T0 = surfaces.host_surface(c.gen, c.rows, c.R, c.As, c.tg[1], c.lo[1], c.hi[1], cc.zcut())[0]
    assert not _same_bits(T, T0)


# ---------------------------------------------------------------------------------------------------------- identities

def test_no_conditioning_locus_is_the_surface_bit_for_bit():
    c = cc.small()
    z = cc.zcut()
    for t in range(len(c.tg)):
        T0, n0 = surfaces.host_surface(c.gen, c.rows, c.R, c.As, c.tg[t], c.lo[t], c.hi[t], z)
        # none at all
        T, ns, nsh = conditional.host_cond_surface(c.gen, c.rows, c.R, c.As, c.tg[t], c.lo[t], c.hi[t], None, 0, -1, 0.0, 0, 0, z)
        assert _same_bits(T, T0) and np.array_equal(ns, n0) and not nsh.any()
        # out of reach by distance: a position far beyond the chromosome at the largest A
        far = float(c.gen[-1]) + 10.0 * z / max(c.As)
        T, ns, nsh = conditional.host_cond_surface(c.gen, c.rows, c.R, c.As, c.tg[t], c.lo[t], c.hi[t], far, 0, len(c.gen) - 1, max(c.As), 1, 1, z)
        assert _same_bits(T, T0) and np.array_equal(ns, n0) and not nsh.any()
        # out of reach by its window: an empty one, and one that lies beside the candidate's sites
        for clo, chi in ((5, 4), (-9, -1), (len(c.gen), len(c.gen) + 7)):
            T, ns, nsh = conditional.host_cond_surface(c.gen, c.rows, c.R, c.As, c.tg[t], c.lo[t], c.hi[t], c.tg[1], clo, chi, c.As[0], 0, 0, z)
            assert _same_bits(T, T0) and np.array_equal(ns, n0) and not nsh.any()


def test_a_site_at_the_conditioning_position_is_not_shared():
    c = cc.small()
    z = cc.zcut()
    # test site 0 is a site's position: given test site 0, the candidate 1's shared sites leave that site out
    T, ns, nsh = _host(c, 1, 0, (0, 0, 0))
    g, tc = c.gen, c.tg[0]
    cand = (c.As[0] * np.abs(g - c.tg[1]) <= z) & (g != c.tg[1])
    reach = c.As[0] * np.abs(g - tc) <= z
    assert (g == tc).sum() >= 1 and cand[g == tc].all() and reach[g == tc].all()
    assert nsh[0] == int((cand & reach & (g != tc)).sum()) == int((cand & reach).sum()) - int((g == tc).sum())


# ------------------------------------------------------------------------------------------------------------- parents

def test_parents_on_hand_made_tracks():
    z = 18.0
    A = np.array([9.0, 90.0])               # reaches 2.0 and 0.2
    # rows:        0    1    2    3    4    5    6
    gen = np.array([0.0, 1.0, 1.3, 5.0, 5.3, 5.5, 9.9])
    clr = np.array([9.0, 5.0, 7.0, 4.0, 4.0, 8.0, 50.0])
    iA = np.array([1, 1, 1, 1, 1, 1, 1])
    rows = np.arange(7)
    # every reach 0.2, H = 0.4: 1-2 (0.3 apart), 3-4 (0.3), 4-5 (0.2), 3-5 (0.5: out); the highest peak (row 6) is out of span
    par = conditional.parents(gen, clr, iA, A, rows, z)
    assert par.tolist() == [-1, 2, -1, -1, 5, -1, -1]
    # ... a tie: of rows 3 and 4 (equal CLR) only the later one has the earlier as a candidate; with a wide reach at row 3
    # (A = 9: 2.0) row 3 sees row 5 and row 4 sees both: the higher CLR wins, not the nearer
    iA2 = iA.copy()
    iA2[3] = 0
    par = conditional.parents(gen, clr, iA2, A, rows, z)
    assert par.tolist() == [-1, 2, -1, 5, 5, -1, -1]
    clr3 = clr.copy()
    clr3[5] = 4.0                            # three equal rows 3, 4, 5: a chain, each the child of the earliest in span
    par = conditional.parents(gen, clr3, iA2, A, rows, z)
    assert par.tolist() == [-1, 2, -1, -1, 3, 3, -1]
    # span given: H = 5 for every pair, whatever the reaches; of the chain 1 < 2 < 0 both lower rows are children of row 0, the highest in span
    par = conditional.parents(gen, clr, iA, A, rows, z, span=5.0)
    assert par.tolist() == [-1, 0, 0, 6, 6, 6, -1]
    par = conditional.parents(gen, clr, iA, A, rows, z, span=0.3)           # |1.3 - 1.0| and |5.3 - 5.0| round above 0.3: exact FP64
    assert par.tolist() == [-1, 2 if abs(gen[2] - gen[1]) <= 0.3 else -1, -1, -1, 5, -1, -1]
    # a subset of the rows in any CLR order: places in the list, not rows
    par = conditional.parents(gen, clr, iA, A, np.array([1, 2, 5]), z, span=5.0)
    assert par.tolist() == [2, 2, -1]
    # a row without a grid result has no footprint of its own
    iA4 = iA.copy()
    iA4[1] = -1
    assert conditional.parents(gen, clr, iA4, A, rows, z).tolist() == [-1, -1, -1, -1, 5, -1, -1]
    assert conditional.parents(gen, clr, iA, A, np.zeros(0, dtype=np.int64), z).tolist() == []


def test_pair_list():
    tests, ct, cl, where = conditional.pair_list(np.array([10, 20, 30]), np.array([1, -1, 1]), np.arange(100, 140), keep=[0, 1])
    assert tests.tolist() == [10, 10, 20, 20, 20] and ct.tolist() == [-1, 20, 10, -1, -1] and cl.tolist() == [-1, 120, 110, -1, -1]
    assert where == [(0, 0, 1, 2, 3), (1, 4, -1, -1, -1)]
    assert tests.dtype == ct.dtype == cl.dtype == np.int32


# ------------------------------------------------------------------------------------------------------ writer, reader

class _Sel:
    grid_A, grid_x, grid_abeta = [100.0, 1000.0], [0.3, 0.5], [1.0, 10.0, 100.0]


def test_writer_and_reader_round_trip(tmp_path):
    apex = np.array([4, 9, 17])
    parent = np.array([1, -1, 1])
    iA_hat = np.full(20, -1)
    iA_hat[[4, 9, 17]] = [1, 0, 0]
    tests, ct, cl, where = conditional.pair_list(apex, parent, np.arange(20) % 12)
    n = len(tests)
    res = {'tmax': np.array([8.0, 2.0, 30.5, 31.0, 31.0, 0.0, 0.0, 31.0, 31.0]), 'lin': np.array([3, 7, 2, 2, 2, -1, -1, 2, 2], dtype=np.int32),
           'nsites': np.tile(np.array([[40, 12]], dtype=np.int32), (n, 1)), 'nshared': np.tile(np.array([[33, 5]], dtype=np.int32), (n, 1))}
    assert n == 9
    rows = conditional.table_rows(['100', '200', '300'], ['0.1', '0.2', '0.3'], ['7.5', '31.25', '0.5'], apex, parent, iA_hat, where, res, _Sel)
    path = str(tmp_path / 'o.txt.conditional.txt')
    assert conditional.output_name(str(tmp_path / 'o.txt')) == path
    conditional.write_table(path, rows)
    names, back = conditional.read_table(path)
    assert '\t'.join(names) + '\n' == conditional.HEADER and len(names) == 16
    assert back[0] == ['100', '0.1', '7.5', '8.0', '200', '0.2', '31.25', '5', '2.0', '0.3', '10.0', '1000.0', '12', '0.25', '30.5',
                       repr(30.5 / 31.0)]
    assert back[1] == ['200', '0.2', '31.25', '31.0'] + ['NA'] * 12
    # nothing > 0 given the parent: 0.0 and NA labels; an unconditional maximum of 0 has no ratio
    assert back[2] == ['300', '0.3', '0.5', '0.0', '200', '0.2', '31.25', '33', '0.0', 'NA', 'NA', 'NA', 'NA', 'NA', '31.0', '1.0']
    conditional.write_table(path, [])
    with open(path) as f:
        assert f.read() == conditional.HEADER


# ------------------------------------------------------------------------------------------------------------ refusals

def test_value_refusal():
    assert conditional.value_refusal(None, None) is None and conditional.value_refusal(0.01, -3.0) is None
    for bad in (0.0, -1.0, float('nan')):
        assert conditional.value_refusal(bad, None) == '--condSpan takes a distance > 0 in the units of the test positions.'
    assert conditional.value_refusal(None, float('nan')) == '--condMin takes a number.'
    assert conditional.value_refusal(0.0, float('nan')).startswith('--condSpan')


O = ['-o', 'OUT']
OK = ['--conditional', '--peaks', '0.01'] + O
WS, FD = {'WORLD_SIZE': '2'}, {'BMX_FORCE_DIST': '1'}
HELPER = '--conditional scans the input; it cannot be combined with --getSpect / --getConfig.'
RANKS = '--conditional runs in a single process; multi-rank launches are not supported.'
ROWS = [(['--condSpan', '0.01'] + O, {}, '--condSpan needs --conditional.'),
        (['--condMin', '3'] + O, {}, '--condMin needs --conditional.'),
        (['--condSurfaces'] + O, {}, '--condSurfaces needs --conditional.'),
        (['--conditional'] + O, {}, '--conditional needs --peaks G: it conditions every apex of the peak call on its neighbour.'),
        (OK + ['--condSpan', '0'], {}, '--condSpan takes a distance > 0 in the units of the test positions.'),
        (OK + ['--condSpan', 'nan'], {}, '--condSpan takes a distance > 0 in the units of the test positions.'),
        (OK + ['--condMin', 'nan'], {}, '--condMin takes a number.'),
        (OK + ['--getSpect'], {}, HELPER), (OK + ['--getConfig'], {}, HELPER),
        (OK[:-2], {}, '--conditional needs -o: the conditional file is written next to the output.'),
        (OK, WS, RANKS), (OK, FD, RANKS),
        # two faults: the value before the missing --peaks, the feature before --peaks' own refusal
        (['--conditional', '--condSpan', '-1'] + O, {}, '--condSpan takes a distance > 0 in the units of the test positions.'),
        (['--conditional', '--peaks', '-1'], {}, '--conditional needs -o: the conditional file is written next to the output.')]


@pytest.mark.parametrize('tail,env,message', ROWS, ids=[' '.join(t) + ''.join(' %s=%s' % kv for kv in e.items()) for t, e, _ in ROWS])
def test_cli_refusal_message(tail, env, message, tmp_path, monkeypatch, capsys):
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


def test_help_names_the_flags():
    text = cli.build_parser().format_help()
    for flag in ('--conditional', '--condSpan', '--condMin', '--condSurfaces'):
        assert flag in text and flag in cli.__doc__


# ------------------------------------------------------------------------------------------- the planted demonstration

def test_two_planted_loci_retain_more_than_one_locus_and_its_shoulder():
    """(a) one planted locus: the strongest apex that has a parent is a shoulder of the locus, and given the locus at its grid
    argmax next to nothing of it is left.  (b) a second locus planted 400 sites away, the footprints overlapping: its apex, given
    the first locus, keeps its CLR.  Ordering only; the two values are quoted in the README."""
    a = cc.demo(cc.DEMO_CENTRES[1:])
    b = cc.demo(cc.DEMO_CENTRES)
    shoulders = [e for e in a if e['parent'] >= 0]
    assert shoulders
    top_a = max(a, key=lambda e: e['clr'])
    shoulder = max(shoulders, key=lambda e: e['clr'])
    assert a[shoulder['parent']] is top_a and abs(top_a['site'] - cc.DEMO_CENTRES[1]) <= 4 * cc.DEMO_STEP
    assert abs(shoulder['site'] - cc.DEMO_CENTRES[1]) < 100           # a shoulder: inside the planted locus' footprint
    order = sorted(b, key=lambda e: -e['clr'])
    first, second = order[0], order[1]
    assert abs(first['site'] - cc.DEMO_CENTRES[1]) <= 4 * cc.DEMO_STEP and abs(second['site'] - cc.DEMO_CENTRES[0]) <= 4 * cc.DEMO_STEP
    assert b[second['parent']] is first
    print('(a) shoulder at site %d, CLR %r: retained %r' % (shoulder['site'], shoulder['clr'], shoulder['retained']))
    print('(b) second locus at site %d, CLR %r: retained %r' % (second['site'], second['clr'], second['retained']))
    assert second['retained'] > shoulder['retained']
