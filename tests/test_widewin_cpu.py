"""The inputs of tests/test_gpu_wide_windows.py really are past the scan kernels' stream caps, and the oracle is good there.

The GPU tests must not be able to pass by never reaching the overflow paths, so the conditions are checked here, on the CPU,
from the definitions in DESIGN.md section 4 (a far candidate: a site of the window with alpha max_grid|R[row]| <= eps; a series
candidate: a far candidate whose row has no moment slot, i.e. is not among the 64 most frequent rows of the site array), with
the 'lds' data set and the table the oracle builds itself.  Every assertion message carries the measured figures; they are
copied into the docstring of tests/widewin.py."""
import functools
import os
import re

import numpy as np

import widewin as ww
from util import REPO, c_oracle, c_scan, oracle_R, orc

from ballermixplus_amd.hostmodel import Grids


@functools.lru_cache(maxsize=None)
def _lds():
    sel = functools.lru_cache(maxsize=None)(lambda n: orc.sel_table('B2', n, 1, [ww.PLANT_X], [ww.PLANT_ABETA])[0, 0])
    gen, k, nn, planted = ww.chromosome('lds', sel)
    spect, props = ww.spectrum('lds')
    xs, ab, _ = Grids(None, None, True, False, None, '100').scan_order()
    R = oracle_R('B2', [100], 1, spect, props, xs, ab)
    row = k.astype(np.int32)                       # one sample size: row = count
    rmax = np.full(R.shape[2], np.inf)
    rmax[1:] = np.abs(R[:, :, 1:]).max(axis=(0, 1))
    frequent = np.zeros(R.shape[2], dtype=bool)
    frequent[np.argsort(-np.bincount(row, minlength=R.shape[2]), kind='stable')[:ww.MOM_ROWS]] = True
    return dict(gen=gen, k=k, nn=nn, planted=planted, spect=spect, props=props, xs=xs, ab=ab, R=R, row=row, rmax=rmax,
                frequent=frequent)


@functools.lru_cache(maxsize=None)
def _counts(run, A, eps):
    """[test site][zone: left, right][sites, far candidates, series candidates]"""
    d = _lds()
    return np.array([ww.far_counts(d['gen'], d['row'], d['rmax'], d['frequent'], int(i), A, eps) for i in ww.TEST_RUNS[run]])


@functools.lru_cache(maxsize=None)
def _oracle(run, A):
    d = _lds()
    idx = ww.TEST_RUNS[run]
    return c_scan(c_oracle(), d['R'], [A], d['gen'], d['row'], d['gen'][idx], np.zeros(len(idx), np.int64),
                  np.full(len(idx), ww.N - 1, np.int64))


def test_the_recipe_is_what_the_docstring_says():
    d = _lds()
    gen, k, nn = d['gen'], d['k'], d['nn']
    assert len(gen) == ww.N and np.all(np.diff(gen) >= 0)
    a, b = ww.TIE_RUN
    assert np.all(gen[a - 1:b] == gen[a]) and gen[a - 2] < gen[a] < gen[b]       # 501 equal positions
    ties_elsewhere = int((np.diff(gen) == 0).sum()) - (b - a)
    assert ties_elsewhere == 0, ties_elsewhere                                   # geometric gaps are >= 1
    assert k.min() >= 1 and np.all(k <= nn) and np.all(nn == 100)
    assert np.isfinite(d['R'][:, :, 1:]).all()                                   # every row a site can carry has a finite g
    assert abs(sum(d['spect'].values()) - 1.0) < 1e-12
    for kind, rows in (('lds', 101), ('l2', 1056)):
        sizes, props = ww.sizes_and_props(kind)
        assert sum(n + 1 for n in sizes) == rows and abs(sum(props.values()) - 1.0) < 1e-12
    xs, ab, As = Grids(None, None, True, False, None, ww.A_LISTS[2]).scan_order()
    assert (len(xs), len(ab), len(As)) == (10, 44, 5) and 1.0 not in xs
    assert -(-len(xs) * len(ab) // 64) == 7 and len(xs) * len(ab) % 64 != 0      # 7 slices of 64 pairs, the last one partial
    for run in ww.TEST_RUNS.values():
        assert len(run) <= 96


def test_several_sample_sizes_use_the_same_draws_for_the_positions():
    sel = functools.lru_cache(maxsize=None)(lambda n: orc.sel_table('B2', n, 1, [ww.PLANT_X], [ww.PLANT_ABETA])[0, 0])
    gen, k, nn, _ = ww.chromosome('l2', sel)
    assert np.array_equal(gen, _lds()['gen'])
    assert sorted(set(nn.tolist())) == list(range(90, 101)) and 0.79 < np.mean(nn == 100) < 0.81
    assert k.min() >= 1 and np.all(k <= nn)
    # every (k, n) drawn has a neutral probability
    spect, _ = ww.spectrum('l2')
    assert all((int(a), int(b)) in spect for a, b in set(zip(k.tolist(), nn.tolist())))


def test_far_candidates_at_A_100_exceed_twice_the_largest_cap():
    """Every test site: at least one zone with >= 2 x 8192 far candidates at eps = 0.05 (round-2 and solo kernels) and at
    eps = 0.15 (prepared kernels); around 30000 / 30250 both zones."""
    need = 2 * max(ww.FAR_CAP, ww.S_FAR_CAP, ww.P_FAR_CAP)
    figures = {}
    for eps in (ww.S_EPS, ww.P_EPS):
        for run in ww.TEST_RUNS:
            far = _counts(run, 100.0, eps)[:, :, 1]
            figures[(run, eps)] = (int(far.max(axis=1).min()), int(far.max(axis=1).max()), int(far.min(axis=1).min()))
    sites = np.concatenate([_counts(run, 100.0, ww.P_EPS)[:, :, 0].sum(axis=1) for run in ww.TEST_RUNS])
    msg = 'A = 100: windows of %d .. %d sites; (run, eps): (larger zone min, max, smaller zone min) %r' % (sites.min(), sites.max(), figures)
    print(msg)
    for (run, eps), (big_min, _, small_min) in figures.items():
        assert big_min >= need, msg
        if run in ww.BOTH_ZONES:
            assert small_min >= need, msg
    for run in ('first', 'last'):                        # one zone is empty there
        assert figures[(run, ww.P_EPS)][2] == 0
    left, right = _counts('c6000', 100.0, ww.P_EPS)[41, :, 1]
    print('site 6000 at eps 0.15: %d far candidates on the left, %d on the right' % (left, right))
    assert 4 * left < right                              # an uneven pair of zones


def test_far_candidates_at_A_250_lie_between_the_prepared_cap_and_the_others():
    """Both zones strictly between 3584 and 8192 at eps = 0.15: past the prepared kernels' cap alone."""
    figures = {}
    for run in ww.TEST_RUNS:
        far = _counts(run, 250.0, ww.P_EPS)[:, :, 1]
        if run in ('first', 'last'):
            far = far.max(axis=1)                        # the one zone there is
        figures[run] = (int(far.min()), int(far.max()))
    msg = 'A = 250, eps = 0.15: far candidates per zone (min, max) %r' % (figures,)
    print(msg)
    for lo, hi in figures.values():
        assert ww.P_FAR_CAP < lo and hi < min(ww.FAR_CAP, ww.S_FAR_CAP), msg


def test_series_candidates_exceed_twice_the_cap():
    """Far candidates whose row has no moment slot: > 2 x 64 in the larger zone of every test site at A = 100 and in both zones
    around 30000 / 30250.  (The rare rows have max|R| of up to 147, so they turn far only 0.07 from the test site: the short
    zone of the sites near the chromosome's start holds none.)"""
    figures = {}
    for run in ww.TEST_RUNS:
        rare = _counts(run, 100.0, ww.P_EPS)[:, :, 2]
        figures[run] = (int(rare.max(axis=1).min()), int(rare.min(axis=1).min()))
    msg = 'A = 100, eps = 0.15: far candidates outside the %d most frequent rows, (larger zone min, smaller zone min) %r' % (ww.MOM_ROWS, figures)
    print(msg)
    for run, (big, small) in figures.items():
        assert big > 2 * ww.SER_CAP, msg
        if run in ww.BOTH_ZONES:
            assert small > 2 * ww.SER_CAP, msg


def test_exponent_budget_split_is_taken_and_not_taken():
    """clr_scan_prepared_kernel applies the two zones' far fields one after the other when bitsR + bitsL > 900, with
    bits = 2 + (int)((far sites of the zone, at most P_FAR_CAP, + its ragged end) * far_bits).  From the far candidates at A = 100,
    eps = 0.15, capped as prep_kernel caps them and without the ragged end (at most one site per test site of the group): the
    split is taken on every run with two zones and not on the first and last sites, whose one zone stays below the budget even
    with a ragged end of 16 sites."""
    fb = float(np.float32(ww.FAR_BITS))
    bits = lambda nfar: 2 + int(np.float32(nfar) * np.float32(fb))
    figures = {}
    for run in ww.TEST_RUNS:
        far = np.minimum(_counts(run, 100.0, ww.P_EPS)[:, :, 1], ww.P_FAR_CAP)
        both = [bits(a) + bits(b) for a, b in far]
        figures[run] = (min(both), max(both))
    msg = 'bitsR + bitsL at A = 100 (min, max) %r' % (figures,)
    print(msg)
    for run, (lo, hi) in figures.items():
        if run in ('first', 'last'):
            assert bits(ww.P_FAR_CAP + 16) + bits(16) <= ww.BUDGET_BITS and hi <= ww.BUDGET_BITS, msg
        else:
            assert lo > ww.BUDGET_BITS, msg


def test_groups_meet_the_mid_cap():
    """More than MID_CAP sites between the test sites of a group: at stride 5 a group of 8 spans 35 sites, and a group inside the
    tie run holds test sites that are not in each other's windows."""
    assert 5 * (8 - 1) > ww.MID_CAP
    gen = _lds()['gen']
    run = ww.TEST_RUNS['c30250']
    assert np.all(gen[run] == gen[run[0]]) and ww.TIE_RUN[0] <= run[0] and run[-1] < ww.TIE_RUN[1]
    mixed = ww.TEST_RUNS['c30000']
    assert gen[mixed[0]] < gen[mixed[-1]] == gen[ww.TIE_RUN[0]]


def test_the_wide_A_wins_around_the_centres():
    """Single-A oracle scans at A = 100 and at A = 250: a result with CLR > 1000 on every test site around the three centres (and,
    beyond what the GPU tests strictly need, on the other runs too: no comparison of theirs is one of empty results)."""
    figures = {}
    for A in (100.0, 250.0):
        for run in ww.TEST_RUNS:
            clr, _, _, iA, ns = _oracle(run, A)
            figures[(run, A)] = (float(clr.min()), float(clr.max()), int(iA.min()), int(ns.max()))
    msg = '(run, A): (CLR min, CLR max, iA min, nSites max) %r' % (figures,)
    print(msg)
    for (run, A), (cmin, cmax, iA, ns) in figures.items():
        assert iA >= 0 and cmin > 1000, msg
        assert cmax < 1.8e5                              # far inside the product exponent's range


@functools.lru_cache(maxsize=None)
def _widest_surfaces():
    d = _lds()
    m = orc.Model('B2', d['gen'], d['k'], d['nn'], d['spect'], d['props'], 1, d['xs'], d['ab'], [100.0])
    assert np.array_equal(m.R[:, :, 1:], d['R'][:, :, 1:]) and np.array_equal(m.row, d['row'])
    return m, [orc.clr_lut(m, 0, ww.N - 1, d['gen'][i], surface=True) for i in ww.WIDEST]


def test_no_ties_on_the_widest_windows():
    """The best grid point lies at least 1e-6 T above every other (x, alpha_beta) point of the same A, so the exact comparison of
    (x, alpha_beta) in the GPU tests is not decided by rounding."""
    margins, sizes = [], []
    for best, Ts, ns in _widest_surfaces()[1]:
        flat = np.sort(Ts[0].reshape(-1))
        assert flat[-1] == best[0] > 0
        margins.append(float((flat[-1] - flat[-2]) / flat[-1]))
        sizes.append(int(ns[0]))
    msg = 'widest windows %r: %r sites, runner-up margins / T %r' % (ww.WIDEST, sizes, margins)
    print(msg)
    assert min(sizes) > 46000 and min(margins) >= 1e-6, msg


def test_oracle_accuracy_on_the_widest_windows():
    """The C oracle's CLR against an extended-precision restatement of 2 sum log1p(alpha R) at its grid point: 1e-11 relative, a
    hundredth of the 1e-9 the GPU tests allow."""
    d = _lds()
    idx = np.array(ww.WIDEST)
    clr, ix, ia, iA, ns = c_scan(c_oracle(), d['R'], [100.0], d['gen'], d['row'], d['gen'][idx], np.zeros(4, np.int64),
                                 np.full(4, ww.N - 1, np.int64))
    assert np.finfo(np.longdouble).eps < 1e-18
    worst = 0.0
    for j, i in enumerate(idx):
        sub, al = ww.window_of(d['gen'], int(i), 100.0)
        assert len(sub) == ns[j]
        r = d['R'][ix[j], ia[j], d['row'][sub]].astype(np.longdouble)
        T = 2 * np.sum(np.log1p(al.astype(np.longdouble) * r))
        worst = max(worst, float(abs(clr[j] - T) / abs(T)))
        (best, _, _) = _widest_surfaces()[1][j]
        assert best[1:4] == (ix[j], ia[j], 0) and best[4] == ns[j]
    print('C oracle vs long double on the widest windows: worst relative difference %.3e' % worst)
    assert worst <= 1e-11, worst


def test_cap_literals_still_match_the_source():
    """The caps these inputs were shaped for, by plain text match on their definitions in bmxscan.hip: a change of a cap fails here
    and flags this suite for re-shaping."""
    with open(os.path.join(REPO, 'ballermixplus_amd', 'csrc', 'bmxscan.hip')) as f:
        src = f.read()
    want = [
        r'constexpr int P_FAR_CAP = P_ORDER == 16 \? 2048 : P_ORDER == 12 \? %d : 8192;' % ww.P_FAR_CAP,
        r'#define BMX_P_ORDER 12\n',
        r'constexpr double P_EPS = P_ORDER == 16 \? 0\.25 : P_ORDER == 12 \? %s : 0\.05;' % re.escape(repr(ww.P_EPS)),
        r'#define BMX_S_ORDER 8\n',
        r'#if BMX_S_ORDER == 8\nconstexpr int S_ORDER = 8, S_COPIES = 8, S_MOM = 1 \+ S_ORDER / 2, S_FAR_CAP = %d;\n// \(S_EPS = %s\)' % (ww.S_FAR_CAP, re.escape(repr(ww.S_EPS))),
        r'constexpr int FAR_CAP = %d;' % ww.FAR_CAP,
        r'constexpr int SER_CAP = %d;' % ww.SER_CAP,
        r'constexpr int MID_CAP = %d;' % ww.MID_CAP,
        r'constexpr int MOM_SLOTS_LDS = %d;' % ww.MOM_ROWS,
        r'P\.far_bits = \(float\)\(P_EPS \* 1\.4427 \* 1\.1\);',
        r'const bool split = bitsR \+ bitsL > %d;' % ww.BUDGET_BITS,
    ]
    for pat in want:
        assert len(re.findall(pat, src)) == 1, pat
