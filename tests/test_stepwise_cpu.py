"""Forward stepwise selection on the host (--stepwise): stepwise.host_base_surface and host_baseline_add against a literal per-site
loop of the K-locus nested mixture in probability space, the two bitwise anchors (no locus: the surface; one locus: the conditional
surface), the telescoped identity, the greedy run against the brute form that recomputes every apex at every step, the margins that
make the device comparison decisive, the planted demonstration, the writer and the refusals."""
import glob
import os

import numpy as np
import pytest

import condcases as cc
import stepcases as sc
from util import REFT

from ballermixplus_amd import cli, conditional, influence, stepwise, surfaces

EX1 = os.path.join(REFT, 'Example1_fullSweep_200kya_DAF.txt')
SPECT = os.path.join(REFT, 'HC_CEU_Neut_DAF_spect_for_B2.txt')

# the loci of the literal comparison on condcases.small(): (test site, grid point (iA, ix, ia)), in order of entry
LOCI = [(0, (0, 1, 2)), (3, (1, 0, 1)), (4, (2, 0, 1))]
CANDIDATES = (1, 2, 3)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))


def _lin(c, point):
    iA, ix, ia = point
    return (iA * len(c.xs) + ix) * len(c.abetas) + ia


def _baseline(c, loci):
    """(d, cnt, scale, written) of condcases.small() after the loci, by host_baseline_add."""
    d, cnt, scale = np.zeros(len(c.gen)), np.zeros(len(c.gen), dtype=np.int32), np.zeros(len(c.gen))
    written = [stepwise.host_baseline_add(d, cnt, c.gen, c.rows, c.R, c.tg[t], c.lo[t], c.hi[t], c.As[p[0]], p[1], p[2], cc.zcut(), scale=scale)
               for t, p in loci]
    return d, cnt, scale, written


# ---------------------------------------------------------------------------------------------------- the literal loop

@pytest.mark.parametrize('K', [0, 1, 2, 3])
def test_restatement_against_the_literal_k_locus_mixture(K):
    c = cc.small()
    loci = LOCI[:K]
    d, cnt, scale, written = _baseline(c, loci)
    lit_loci = [(c.tg[t], c.lo[t], c.hi[t], c.As[p[0]], p[1], p[2]) for t, p in loci]
    worst = 0.0
    for t in CANDIDATES:
        T, ns, nsh, S = stepwise.host_base_surface(c.gen, c.rows, c.R, c.As, c.tg[t], c.lo[t], c.hi[t], d, cnt, cc.zcut(), scale=True)
        Tl, nl, nshl, Sl, dl, cntl, weights = sc.literal_base(c.gen, c.rows, c.model.g, c.R, c.As, c.tg[t], c.lo[t], c.hi[t], lit_loci, cc.zcut())
        assert weights <= 1e-15 * (K + 1)           # the components of every site are a proper distribution
        assert np.array_equal(cnt, cntl) and np.array_equal(ns, nl) and np.array_equal(nsh, nshl)
        assert np.all(np.abs(d - dl) <= sc.SITE_TOL * (1.0 + scale))
        assert np.array_equal(np.isnan(T), np.isnan(Tl)) and np.array_equal(np.isnan(T).all(axis=(1, 2)), ns == 0)
        assert (ns > 0).any()
        bound = sc.SITE_TOL * (ns[:, None, None] + Sl)
        ok = ~np.isnan(T)
        worst = max(worst, float(np.max(np.abs(T - Tl)[ok] / bound[ok])))
        assert np.all(np.abs(T - Tl)[ok] <= bound[ok]) and np.all(np.abs(S - 2.0 * Sl)[ok] <= bound[ok])
        if K:
            assert (nsh > 0).any()
        else:
            assert not nsh.any() and not cnt.any() and not d.any()
    assert [w[2] > 0 for w in written] == [True] * K and (K < 2 or cnt.max() >= 2)      # some site is reached by two loci
    print('K = %d: worst |dT| / bound %.3g, sites reached %d, by more than one locus %d' % (K, worst, int((cnt > 0).sum()), int((cnt > 1).sum())))


# ------------------------------------------------------------------------------------------------------------- anchors

def test_no_locus_is_the_surface_and_one_locus_the_conditional_surface_bit_for_bit():
    c = cc.small()
    z = cc.zcut()
    N = len(c.gen)
    zero, none = np.zeros(N), np.zeros(N, dtype=np.int32)
    for t in range(len(c.tg)):
        T0, n0 = surfaces.host_surface(c.gen, c.rows, c.R, c.As, c.tg[t], c.lo[t], c.hi[t], z)
        T, ns, nsh = stepwise.host_base_surface(c.gen, c.rows, c.R, c.As, c.tg[t], c.lo[t], c.hi[t], zero, none, z)
        assert _same_bits(T, T0) and np.array_equal(ns, n0) and not nsh.any()
    for q, point in LOCI + [(1, (1, 1, 1)), (3, (0, 0, 0))]:             # (test site 3's window cuts: [120, 185])
        d, cnt, _, written = _baseline(c, [(q, point)])
        first, last, n = written[0]
        assert n == int((cnt > 0).sum()) and cnt.max() == 1 and first == int(np.nonzero(cnt)[0][0]) and last == int(np.nonzero(cnt)[0][-1])
        for t in range(len(c.tg)):
            Tc, nc, nshc = conditional.host_cond_surface(c.gen, c.rows, c.R, c.As, c.tg[t], c.lo[t], c.hi[t], c.tg[q], c.lo[q], c.hi[q],
                                                         c.As[point[0]], point[1], point[2], z)
            T, ns, nsh = stepwise.host_base_surface(c.gen, c.rows, c.R, c.As, c.tg[t], c.lo[t], c.hi[t], d, cnt, z)
            assert _same_bits(T, Tc) and np.array_equal(ns, nc) and np.array_equal(nsh, nshc), (q, point, t)


def test_a_locus_without_a_site_writes_nothing():
    c = cc.small()
    d, cnt = np.full(len(c.gen), 0.25), np.ones(len(c.gen), dtype=np.int32)
    for clo, chi in ((5, 4), (-9, -1), (len(c.gen), len(c.gen) + 7)):
        first, last, n = stepwise.host_baseline_add(d, cnt, c.gen, c.rows, c.R, c.tg[1], clo, chi, c.As[0], 0, 0, cc.zcut())
        assert first > last and n == 0
    far = float(c.gen[-1]) + 10.0 * cc.zcut() / max(c.As)
    assert stepwise.host_baseline_add(d, cnt, c.gen, c.rows, c.R, far, 0, len(c.gen) - 1, max(c.As), 1, 1, cc.zcut())[2] == 0
    assert (d == 0.25).all() and (cnt == 1).all()


def test_site_ranges_against_a_plain_mask():
    for name in ('small', 'ragged', 'edges'):
        c = sc.case(name)
        every = np.arange(len(c.tg))
        first, last = stepwise.site_ranges(c.gen, c.tg, c.lo, c.hi, min(c.As), sc.zcut())
        for k in every.tolist():
            a, b = max(int(c.lo[k]), 0), min(int(c.hi[k]), len(c.gen) - 1)
            at = a + np.nonzero(min(c.As) * np.abs(c.gen[a:b + 1] - c.tg[k]) <= sc.zcut())[0] if b >= a else np.zeros(0, dtype=np.int64)
            if len(at):
                assert (first[k], last[k]) == (at[0], at[-1]), (name, k)
            else:
                assert first[k] > last[k], (name, k)


# ------------------------------------------------------------------------------------------------------- the greedy run

@pytest.mark.parametrize('name', sc.FAST)
def test_identity_the_entry_maxima_sum_to_the_log_ratio_of_the_whole_model(name):
    c, out, _ = sc.host_case(name)
    nx, nab = len(c.xs), len(c.ab)
    d, cnt = np.zeros(len(c.gen)), np.zeros(len(c.gen), dtype=np.int32)
    total, scale = 0.0, 0.0
    for step, k in enumerate(out['order']):              # the run again, one locus at a time, with the size of every entry's sum
        t, lin = int(c.apex[k]), int(out['lin'][k])
        T, ns, nsh, S = stepwise.host_base_surface(c.gen, c.rows, c.R(), c.As, c.tg[t], c.lo[t], c.hi[t], d, cnt, sc.zcut(), scale=True)
        v, l, _ = influence.scan_argmax(T)
        assert (v, l) == (float(out['T'][k]), lin) and out['step'][k] == step + 1
        total += v
        assert total == out['T_total'][k]
        scale += float(S.reshape(-1)[lin])
        iA, ix, ia = cc.decode(lin, nx, nab)
        w = stepwise.host_baseline_add(d, cnt, c.gen, c.rows, c.R(), c.tg[t], c.lo[t], c.hi[t], c.As[iA], ix, ia, sc.zcut())
        assert w == out['written'][step]
    assert _same_bits(d, out['d']) and np.array_equal(cnt, out['cnt'])
    whole = 2.0 * float(np.sum(np.log1p(d)))
    scale += 2.0 * float(np.sum(np.abs(np.log1p(d))))
    print('%s: %d loci, T_total %r, 2 sum log1p(d) %r, |difference| / scale %.3g' % (name, len(out['order']), total, whole,
                                                                                     abs(total - whole) / scale if scale else 0.0))
    assert abs(total - whole) <= sc.ID_TOL * scale


@pytest.mark.parametrize('name', sc.FAST)
def test_the_skip_rule_changes_nothing(name):
    c, out, _ = sc.host_case(name)
    brute = c.host_run(skip=False)
    K = len(c.apex)
    n = len(out['order'])
    assert brute['evals'] == K + sum(K - s - 1 for s in range(n)) >= out['evals']
    assert brute['order'] == out['order'] and brute['written'] == out['written']
    for f in ('T_max', 'T', 'T_total', 'd'):
        assert _same_bits(brute[f], out[f]), (name, f)
    for f in ('step', 'lin', 'nsites', 'nshared', 'cnt'):
        assert np.array_equal(brute[f], out[f]), (name, f)
    print('%s: %d apexes, %d loci, %d surfaces with the skip rule, %d without' % (name, K, n, out['evals'], brute['evals']))


def test_the_skip_rule_skips_something():
    assert any(sc.host_case(n)[1]['evals'] < len(sc.host_case(n)[0].apex) * (len(sc.host_case(n)[1]['order']) + 1) - 1 for n in ('ragged', 'ex1_B2_w50_s25'))


@pytest.mark.parametrize('name', sc.NAMES)
def test_margins_every_choice_is_decided_by_more_than_rounding(name):
    c, out, m = sc.host_case(name)
    step, argmax, stop = m.worst()
    print('%s: %d apexes, accepted %s; smallest relative gap: between two apexes %.3g, between two grid points %.3g, to the threshold %.3g'
          % (name, len(c.apex), [int(c.apex[k]) for k in out['order']], step, argmax, stop))
    assert step > sc.MARGIN and argmax > sc.MARGIN and stop > sc.MARGIN
    if name != 'ex1_B2_fixX_fixAlpha_listA':            # (that grid's surfaces are all below 0: nothing is accepted)
        assert out['order']


def test_max_loci_and_threshold_stop_the_run():
    c, out, _ = sc.host_case('ragged')
    assert len(out['order']) >= 3
    two = c.host_run(max_loci=2)
    assert two['order'] == out['order'][:2] and two['written'] == out['written'][:2]
    C = float(np.sort(out['T'][out['step'] > 0])[-2]) * 0.999          # just below the second highest entry value
    high = c.host_run(min_clr=C)
    assert 1 <= len(high['order']) < len(out['order']) and high['order'] == out['order'][:len(high['order'])]
    rest = high['step'] == 0
    assert (high['T'][rest] < C).all() or (high['lin'][rest] < 0).any()
    none = c.host_run(min_clr=1e9)
    assert none['order'] == [] and not none['cnt'].any() and _same_bits(none['T'], none['T_max'])


# ------------------------------------------------------------------------------------------- the planted demonstration

def test_planted_one_locus_is_one_locus_and_two_are_two():
    """C = 15.  (a) one planted locus (site 1500): exactly one apex is accepted, within a few test sites of the plant, and every
    other apex -- the shoulders with CLRs up to 19.8 among them -- ends below C.  (b) a second locus at site 1100, the footprints
    overlapping: exactly two, in the order of their CLRs.  The numbers are quoted in the README."""
    for name, centres in (('demo1', cc.DEMO_CENTRES[1:]), ('demo2', cc.DEMO_CENTRES)):
        c, out, _ = sc.host_case(name)
        sites = c.apex * cc.DEMO_STEP
        got = [int(sites[k]) for k in out['order']]
        print('%s: apexes at sites %s, T_max %s\n   accepted %s at entry values %s, T_total %r\n   the others given all accepted loci: %s'
              % (name, sites.tolist(), [round(float(v), 3) for v in out['T_max']], got, [float(out['T'][k]) for k in out['order']],
                 float(np.nanmax(out['T_total'])), [(int(s), float(v)) for s, v, st in zip(sites, out['T'], out['step']) if not st]))
        assert len(got) == len(centres)
        for s, want in zip(got, sorted(centres, reverse=True)):          # (the locus at 1500 is the stronger one)
            assert abs(s - want) <= 4 * cc.DEMO_STEP
        rest = out['step'] == 0
        assert (out['T'][rest] < sc.DEMO_C).all() and (out['T_max'][rest] > sc.DEMO_C).any()       # a shoulder was above C and is not any more


# ------------------------------------------------------------------------------------------------------ writer, reader

class _Sel:
    grid_A, grid_x, grid_abeta = [100.0, 1000.0], [0.3, 0.5], [1.0, 10.0, 100.0]


def test_writer_and_reader_round_trip(tmp_path):
    nan = float('nan')
    out = {'T_max': np.array([8.0, 31.0, 0.5, 0.0]), 'step': np.array([2, 1, 0, 0], dtype=np.int32), 'T': np.array([2.0, 31.0, 0.0, 0.0]),
           'lin': np.array([7, 2, -1, -1], dtype=np.int32), 'T_total': np.array([33.0, 31.0, nan, nan]),
           'nsites': np.tile(np.array([[40, 12]], dtype=np.int32), (4, 1)), 'nshared': np.array([[33, 5], [0, 0], [9, 9], [0, 0]], dtype=np.int32),
           'order': [1, 0]}
    rows = stepwise.table_rows(['100', '200', '300', '400'], ['0.1', '0.2', '0.3', '0.4'], ['7.5', '31.25', '0.5', '0.0'], out, _Sel)
    path = str(tmp_path / 'o.txt.stepwise.txt')
    assert stepwise.output_name(str(tmp_path / 'o.txt')) == path and stepwise.surfaces_name('o') == 'o.stepwise.surfaces.txt'
    stepwise.write_table(path, rows)
    names, back = stepwise.read_table(path)
    assert '\t'.join(names) + '\n' == stepwise.HEADER and len(names) == 13
    assert names == 'physPos genPos CLR T_max step CLR_cond x_cond s_cond A_cond nSites_cond nShared retained T_total'.split()
    assert back[0] == ['100', '0.1', '7.5', '8.0', '2', '2.0', '0.3', '10.0', '1000.0', '12', '5', '0.25', '33.0']
    assert back[1] == ['200', '0.2', '31.25', '31.0', '1', '31.0', '0.3', '100.0', '100.0', '40', '0', '1.0', '31.0']
    # nothing > 0 given the accepted loci: 0.0 and NA labels; an unconditional maximum of 0 has no ratio
    assert back[2] == ['300', '0.3', '0.5', '0.5', 'NA', '0.0', 'NA', 'NA', 'NA', 'NA', 'NA', '0.0', 'NA']
    assert back[3] == ['400', '0.4', '0.0', '0.0', 'NA', '0.0', 'NA', 'NA', 'NA', 'NA', 'NA', 'NA', 'NA']
    stepwise.write_table(path, [])
    with open(path) as f:
        assert f.read() == stepwise.HEADER
    gpath = str(tmp_path / 'stepwise.txt')
    stepwise.write_genome(gpath, [('a.txt', rows[:2]), ('b.txt', []), ('c.txt', rows[2:3])])
    with open(gpath) as f:
        lines = f.read().split('\n')
    assert lines[0] == 'file\t' + stepwise.HEADER[:-1] and [l.split('\t')[0] for l in lines[1:4]] == ['a.txt', 'a.txt', 'c.txt']
    assert lines[1].split('\t')[1:] == back[0] and lines[4] == ''


def test_table_of_a_host_run():
    c, out, _ = sc.host_case('small')

    class Sel:
        grid_A, grid_x, grid_abeta = c.As, c.xs, c.ab
    K = len(c.apex)
    rows = [r.rstrip('\n').split('\t') for r in stepwise.table_rows(['p'] * K, ['g'] * K, ['c'] * K, out, Sel)]
    assert [r[4] for r in rows] == [str(s) for s in out['step'].tolist()]           # every apex of `small` is accepted
    first = out['order'][0]
    assert rows[first][5] == rows[first][3] and rows[first][10] == '0' and rows[first][11] == '1.0' and rows[first][12] == rows[first][3]
    last = out['order'][-1]
    assert rows[last][12] == repr(float(np.nanmax(out['T_total'])))


# ------------------------------------------------------------------------------------------------------------ refusals

def test_value_refusal():
    assert stepwise.value_refusal(None, None) is None and stepwise.value_refusal(-3.0, 1) is None
    assert stepwise.value_refusal(float('nan'), None) == '--stepMin takes a number.'
    for bad in (0, -2):
        assert stepwise.value_refusal(None, bad) == '--stepMax takes a number of loci >= 1.'
    assert stepwise.value_refusal(float('nan'), 0).startswith('--stepMin')


O = ['-o', 'OUT']
OK = ['--stepwise', '--peaks', '0.01'] + O
WS, FD = {'WORLD_SIZE': '2'}, {'BMX_FORCE_DIST': '1'}
HELPER = '--stepwise scans the input; it cannot be combined with --getSpect / --getConfig.'
RANKS = '--stepwise runs in a single process; multi-rank launches are not supported.'
ROWS = [(['--stepMin', '3'] + O, {}, '--stepMin needs --stepwise.'),
        (['--stepMax', '3'] + O, {}, '--stepMax needs --stepwise.'),
        (['--stepSurfaces'] + O, {}, '--stepSurfaces needs --stepwise.'),
        (['--stepwise'] + O, {}, '--stepwise needs --peaks G: it selects among the apexes of the peak call.'),
        (OK + ['--stepMin', 'nan'], {}, '--stepMin takes a number.'),
        (OK + ['--stepMax', '0'], {}, '--stepMax takes a number of loci >= 1.'),
        (OK + ['--stepMax', '-4'], {}, '--stepMax takes a number of loci >= 1.'),
        (OK + ['--getSpect'], {}, HELPER), (OK + ['--getConfig'], {}, HELPER),
        (OK[:-2], {}, '--stepwise needs -o: the stepwise file is written next to the output.'),
        (OK, WS, RANKS), (OK, FD, RANKS),
        # two faults: the value before the missing --peaks, the feature before --peaks' own refusal
        (['--stepwise', '--stepMax', '0'] + O, {}, '--stepMax takes a number of loci >= 1.'),
        (['--stepwise', '--peaks', '-1'], {}, '--stepwise needs -o: the stepwise file is written next to the output.')]


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
    for flag in ('--stepwise', '--stepMin', '--stepMax', '--stepSurfaces'):
        assert flag in text and flag in cli.__doc__
