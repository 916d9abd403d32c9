"""tests/chunkseams.py on the host: the restated chunk rules are the shipped ones, every case crosses the seam it is named for, no
chunk length is a multiple of 13 (so every chunk holds another rotation of the 13 distinct entries), the 13 are distinct and hold
the window kinds they promise, the host arrays stay below 600 MB, the argmax margins of the host restatements leave at most 1 % of
the blocks undecided, and the vectorised one-point jackknife is influence.host_influence.  No GPU."""
import functools
import os
import re

import numpy as np
import pytest

import chunkseams as cs
import influencecases as ic
from util import REPO, c_oracle, c_sel_table, orc

from ballermixplus_amd import conditional, influence, surfaces

ZCUT = orc.alpha_cut_z()


@functools.lru_cache(maxsize=None)
def _R(name):
    """The oracle's table of a gridshape scene, 0 on the rows no site stands on."""
    sc = cs.scene(name)
    return cs.gs.table_from(c_sel_table(c_oracle(), 'B2', cs.gs.NSAMP, 1, sc.xs, sc.abetas), 'small')


@functools.lru_cache(maxsize=None)
def _case(name):
    return cs.CASES[name](ZCUT)


def test_the_restated_rules_are_the_shipped_ones():
    src = {}
    for k, (path, pat) in enumerate(cs.LITERALS):
        if path not in src:
            with open(os.path.join(REPO, path)) as f:
                src[path] = f.read()
        assert len(re.findall(pat, src[path])) == cs.LITERAL_COUNTS.get(k, 1), pat
    assert (cs.CHUNK_BYTES, cs.FIT_LDS_BYTES, cs.RANGE_STEP, cs.INFL_CHUNK_BLOCKS, cs.FIT_OUT_BYTES) == (256 << 20, 40 << 10, 1 << 20, 1 << 22, 64 << 20)
    assert ZCUT == pytest.approx(-np.log(1e-8), rel=1e-12)
    # the restatement on figures worked by hand
    assert cs.surfaces_step(64, 1037) == (505, 505, 52428) and cs.surfaces_step(16, 1) == (1048575, 2097152, 1048575)
    assert cs.surfaces_step(1, 1 << 26)[0] == 1 and cs.even_cuts(7, 3) == [3, 3, 1] and cs.even_cuts(6, 3) == [3, 3]
    assert cs.fit_step(1, 16, 16) == (13107, 13107, (256 << 20) // (17 * 24), True)
    assert cs.fit_step(221, 10, 25) == (4600, 13421, 4600, False) and cs.fit_step(221, 6, 25)[3] and not cs.fit_step(221, 6, 25, 1)[3]
    cap = cs.INFL_CHUNK_BLOCKS
    assert cs.influence_cuts([5, cap - 5, 1, cap + 1, 2, 3], 100) == [2, 1, 1, 2]      # full to the block, then one window with more
    assert cs.influence_cuts([1] * 10, 4) == [4, 4, 2] and cs.influence_cuts([0] * 5, 100) == [5]


@pytest.mark.parametrize('name', list(cs.CASES))
def test_every_case_crosses_its_seam(name):
    sc, calls = _case(name)
    for c in calls:
        print(name, c, '%.1f MB on the host' % (c.host_bytes / 1e6))
        assert c.host_bytes <= cs.HOST_CAP
        for loop, cuts in c.cuts.items():
            assert sum(cuts) == c.n
            if name in cs.ROTATED:
                # 13 divides no chunk length, and no chunk but the first starts on a multiple of 13: at buffer offset 0 every
                # chunk holds another entry of the 13 than the first chunk does
                assert all(m % cs.K for m in cuts[:-1]), (loop, cuts)
                starts = np.cumsum([0] + cuts[:-1])
                assert all(int(s) % cs.K for s in starts[1:]), (loop, starts)
    step, by_bytes, by_threads = cs.surfaces_step(sc.nA, sc.npairs)
    if name == 'bytes':
        assert sc.nA * sc.npairs * 8 == 530944 and -(-sc.npairs // 256) == 5 and (step, by_bytes) == (505, 505) and by_threads > step
        assert [c.cuts['windows'] for c in calls] == [[505, 3]] * 4 + [[505, 505, 3]] + [[505, 3], [505, 505, 3]]
        assert [c.kw.get('block') for c in calls[1:3]] == [10 ** 6, 3] and calls[1].cuts['range'] == [508]
        assert calls[3].kw['want_T'] and not calls[4].kw['want_T'] and 260e6 < calls[0].host_bytes < 280e6
        assert [(c.op, c.kw['want_T']) for c in calls[3:]] == [('cond', True), ('cond', False), ('base', True), ('base', False)]
    if name == 'threads':
        assert (by_bytes, by_threads, step) == (2097152, 1048575, 1048575)
        assert all(c.cuts['windows'] == [1048575, 5] for c in calls) and [c.op for c in calls] == ['surfaces', 'cond']
    if name == 'range':
        c = calls[0]
        assert c.cuts['range'] == [1 << 20, 3] and c.cuts['windows'] == [1048575, 4]        # the two seams lie one window apart
        assert c.n <= cs.INFL_CHUNK_BLOCKS                  # at most one block per window: the block rule does not cut first
    if name == 'blocks':
        c = calls[0]
        per = cs.block_counts(sc.gen, sc.tg, sc.lo, sc.hi, min(sc.As), ZCUT, 1)
        assert sc.As[0] * (sc.gen[-1] - sc.gen[0]) <= ZCUT and per.max() == 700 and sorted(per.tolist())[:2] == [0, 300]
        first = c.cuts['windows'][0]
        b = per[np.arange(c.n) % cs.K]
        assert len(c.cuts['windows']) >= 2 and first < step and 5000 < first < 8000
        assert b[:first].sum() <= cs.INFL_CHUNK_BLOCKS < b[:first + 1].sum()               # the block rule cuts, to the window
        assert c.cuts['range'] == [c.n] and b.sum() < influence.MAX_RESULTS
    if name == 'one_window':
        c = calls[0]
        b = cs.block_counts(sc.gen, sc.tg, sc.lo, sc.hi, min(sc.As), ZCUT, 1)
        assert c.cuts['windows'] == [1, 1, 1] and b[1] == cs.LATTICE_N > cs.INFL_CHUNK_BLOCKS and b[0] == b[2] == 8
        assert sc.As[0] * (sc.gen[-1] - sc.gen[0]) <= ZCUT and len(sc.gen) == (1 << 22) + 70000
        assert np.count_nonzero(np.diff(sc.gen) == 0) == 1 and sc.gen[len(sc.gen) // 2 + 1] == sc.tg[1]
        assert len(set(np.diff(sc.gen).tolist())) == 3      # the lattice step, the tie and the double step behind it
    if name == 'fit_out':
        c = calls[0]
        assert (c.kw['F'], c.kw['D']) == (16, 16) and c.cuts['windows'] == [13107, 3] and cs.fit_step(1, 16, 16)[3]
    if name == 'fit_ws':
        n_sizes = len(sc.model.sizes)
        step, out, ws, in_lds = cs.fit_step(n_sizes, 10, 25)
        assert n_sizes == 221 and n_sizes * 11 * 24 == 58344 > cs.FIT_LDS_BYTES and not in_lds
        assert ws < out and step == ws and calls[0].cuts['windows'] == [ws, 3]                 # the workspace rule binds
        assert cs.fit_step(n_sizes, 6, 25)[3] and n_sizes * 7 * 24 <= cs.FIT_LDS_BYTES
        assert [(c.n, c.kw['variant']) for c in calls[1:]] == [(cs.K, 0), (cs.K, 1)]


@pytest.mark.parametrize('name', ['bytes', 'one_pair', 'blocks', 'fit_out', 'fit_ws'])
def test_the_thirteen(name):
    sc = cs.scene(name)
    N, k = len(sc.gen), sc.kinds
    assert len(sc.tg) == cs.K and np.all(np.diff(sc.tg) > 0)
    a, b = np.maximum(sc.lo, 0), np.minimum(sc.hi, N - 1)
    inside = np.maximum(b - a + 1, 0)
    if name != 'blocks':
        assert inside.max() <= 8
    assert sc.hi[k['empty']] < sc.lo[k['empty']] and (inside > 0).sum() == cs.K - 1
    j = k['beside']
    assert sc.gen[a[j]] > sc.tg[j] or sc.gen[b[j]] < sc.tg[j]
    j = k['tie']
    assert np.count_nonzero(sc.gen == sc.tg[j]) >= 2
    assert not np.any(sc.gen == sc.tg[k['off_site']]) and sc.gen[0] < sc.tg[k['off_site']] < sc.gen[-1]
    lo_clip, hi_clip = k['clipped']
    assert sc.lo[lo_clip] < 0 and sc.hi[hi_clip] > N - 1
    # the second arrays: one entry without a grid point, one without a conditioning site, and pairs that share sites
    lins = cs.fit_lins(sc.points)
    ct, cl = cs.cond_partners(sc.points)
    assert (lins < 0).sum() == 1 and lins.max() < sc.points and (ct < 0).sum() == 1 and (cl < 0).sum() == 1 and cl.max() < sc.points
    assert len(set(zip(ct.tolist(), cl.tolist()))) == cs.K
    if name != 'blocks':
        assert cs.along(lins, 40).tolist() == [int(lins[q % 13]) for q in range(40)] and cs.rotation(40).tolist() == [q % 13 for q in range(40)]


def _argmax_margin(T):
    v, l, second = influence.scan_argmax(T)
    if l >= 0:
        return v - second
    T = np.asarray(T)
    return float(-np.nanmax(np.where(np.isnan(T), -np.inf, T), initial=-np.inf))


@pytest.mark.parametrize('name,blocks', [('bytes', (10 ** 6, 3)), ('one_pair', (10 ** 6,)), ('blocks', (1,))])
def test_the_thirteen_are_distinct_and_their_margins_decide(name, blocks):
    """On the oracle's table: the 13 surfaces differ pairwise (a rotation gone wrong cannot hide), and lin and lin_b are further
    than twice the GPU tolerance from changing on at least 99 % of the 13 x blocks."""
    sc, R = cs.scene(name), _R(name)
    seen, narrow_lin = set(), 0
    for j in range(cs.K):
        T, ns = surfaces.host_surface(sc.gen, sc.rows, R, sc.As, sc.tg[j], sc.lo[j], sc.hi[j], ZCUT)
        seen.add((T.tobytes(), ns.tobytes()))
        narrow_lin += not _argmax_margin(T) > 2 * ic.tolerance(T)
    ct, cl = cs.cond_partners(sc.points)
    shared, moved = 0, 0
    for j in range(cs.K):
        c = int(ct[j])
        if c >= 0 and cl[j] >= 0:
            iA, ix, ia = sc.decode(int(cl[j]))
            T, ns, nsh, S = conditional.host_cond_surface(sc.gen, sc.rows, R, sc.As, sc.tg[j], sc.lo[j], sc.hi[j], sc.tg[c], sc.lo[c], sc.hi[c],
                                                          sc.As[iA], ix, ia, ZCUT, scale=True)
            shared += int(nsh.max() > 0)
            narrow_lin += not _argmax_margin(T) > 2 * 1e-9 * float(S.max())
    total, narrow = 0, 0
    for B in blocks:
        for j in range(cs.K):
            h = influence.host_influence(sc.gen, sc.rows, R, sc.As, sc.tg[j], sc.lo[j], sc.hi[j], ZCUT, min(B, len(sc.gen)))
            total += len(h['m'])
            narrow += int((~(h['margin'] > 2 * ic.tolerance(h['T']))).sum())
    print('%s: %d distinct surfaces, %d pairs share sites, %d of 26 window argmaxes and %d of %d blocks within twice the tolerance'
          % (name, len(seen), shared, narrow_lin, narrow, total))
    assert len(seen) == cs.K
    assert shared >= 2
    assert total >= cs.K - 1 and narrow <= 0.01 * total and narrow_lin <= 1


def test_the_one_point_jackknife_is_host_influence():
    """On a 3 000-site lattice of the one-window recipe, every window and two block sizes."""
    sc = cs.lattice_scene(3000)
    R = _R('one_pair')
    assert np.array_equal(cs.scene('one_pair').xs, sc.xs) and np.array_equal(cs.scene('one_pair').abetas, sc.abetas)
    for j in range(3):
        for B in (1, 3, 10 ** 6):
            B = min(B, 3000)
            h = influence.host_influence(sc.gen, sc.rows, R, sc.As, sc.tg[j], sc.lo[j], sc.hi[j], ZCUT, B)
            v = cs.host_influence_one_point(sc.gen, sc.rows, R[0, 0], sc.As[0], sc.tg[j], sc.lo[j], sc.hi[j], ZCUT, B)
            assert (v['lin'], v['ns_min'], v['first_block']) == (h['lin'], h['ns_min'], h['first_block']) and np.array_equal(v['ns'], h['ns'])
            assert np.array_equal(v['m'], h['m']) and np.array_equal(v['blin'], h['blin']) and np.array_equal(v['n_b'], h['n_b'])
            tol = 1e-12 * v['abs_sum']
            assert abs(v['T_max'] - h['T_max']) <= tol and np.allclose(v['T'], h['T'], rtol=0, atol=tol)
            assert np.allclose(v['L'], h['L'], rtol=0, atol=tol) and np.allclose(v['contrib'], h['contrib'], rtol=0, atol=tol, equal_nan=True)
            assert np.allclose(v['margin'], h['margin'], rtol=0, atol=tol)
            if j == 1 and B == 1:
                # the window over every site: the two sites on the test position do not qualify and are blocks with m = 0
                assert v['ns_min'] == 2998 and len(v['m']) == 3000 and (v['m'] == 0).sum() == 2 and h['lin'] == 0


def test_the_long_window_has_a_maximum_worth_a_tolerance():
    """The whole lattice on the oracle's table: T_max > 0, so that every block has a contribution and an L_b to compare, and the
    terms do not cancel (sum |term| within a factor of 100 of T): REL_TOL of max |T| is far above the rounding of four million
    additions (2^-53 sqrt(n) sum |term|, 2e-13 of it)."""
    sc = cs.scene('one_window')
    R = _R('one_pair')
    v = cs.host_influence_one_point(sc.gen, sc.rows, R[0, 0], sc.As[0], sc.tg[1], sc.lo[1], sc.hi[1], ZCUT, 1)
    narrow = int((~(v['margin'] > 2 * ic.tolerance(v['T']))).sum())
    print('one_window: T_max %r, sum |term| %r, %d blocks, %d with m = 0, %d margins within twice the tolerance'
          % (v['T_max'], v['abs_sum'], len(v['m']), int((v['m'] == 0).sum()), narrow))
    assert v['lin'] == 0 and v['abs_sum'] <= 100 * v['T_max']
    assert len(v['m']) == cs.LATTICE_N and (v['m'] == 0).sum() == 2 and v['ns_min'] == cs.LATTICE_N - 2
    assert narrow <= 0.01 * len(v['m'])
