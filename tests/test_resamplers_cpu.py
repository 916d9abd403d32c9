"""The catalogue of tests/resamplers.py on the host: with the package's exact restatements alone (null.block_permutation,
boot.site_weights, locate.resampled, locate.argmax_rows, power.planted_rows / power.reach) and the oracle's table, every case
reaches the edge it is named for -- the launch caps, the table sizes either side of 3 072 and 8 192 rows, the Feistel shapes, the
all-zero and heavy weight vectors, decided draws, the empty-window rows and the designed ties -- and the constants the cases were
shaped around still read so in bmxscan.hip."""
import functools
import itertools
import os
import re

import numpy as np
import pytest

import resamplers as rs
from util import REPO, c_oracle, c_scan, oracle_R

from ballermixplus_amd import boot, locate, null, power


@functools.lru_cache(maxsize=None)
def _R(name):
    """The ORACLE's table of a catalogue table (the GPU module plants and scans with the device's)."""
    t = rs.table(name)
    return oracle_R('B2', t.sizes, 1, t.spect, t.props, rs.XS, rs.ABETAS)


def test_source_pins():
    """The constants the catalogue was built around, by plain text match on bmxscan.hip: a change there flags this suite."""
    with open(os.path.join(REPO, 'ballermixplus_amd', 'csrc', 'bmxscan.hip')) as f:
        src = f.read()
    for pat in (r'constexpr int RS_THREADS = %d;' % rs.RS_THREADS, r'constexpr int RS_PER = %d;' % rs.RS_PER,
                r'constexpr int RS_TILE = RS_THREADS \* RS_PER;', r'constexpr int RS_HIST_MAX = %d;' % rs.RS_HIST_MAX,
                r'constexpr int RS_BLOCKS_MAX = %d;' % rs.RS_BLOCKS_MAX, r'constexpr int NULL_THREADS = %d;' % rs.NULL_THREADS,
                r'constexpr int NULL_BLOCKS_MAX = %d;' % rs.NULL_BLOCKS_MAX, r'constexpr int PLANT_THREADS = %d;' % rs.PLANT_THREADS,
                r'constexpr int PLANT_LDS_BYTES = 48 << 10;', r'constexpr int PLANT_HIST_BLOCKS_MAX = %d;' % rs.PLANT_HIST_BLOCKS_MAX,
                r'constexpr int MOM_SLOTS = %d;' % rs.MOM_SLOTS, r'constexpr int LOCATE_THREADS = %d;' % rs.LOCATE_THREADS,
                r'constexpr int WAVE = %d;' % rs.WAVE,
                r'std::min<int64_t>\(\(s->N \+ 255\) / 256, %d\);\n        if \(s->wide_rows\) hipLaunchKernelGGL\(permute_rows_kernel<uint32_t>, dim3\(blocks\), dim3\(256\)'
                % rs.PERM_BLOCKS_MAX,
                r'\(unsigned\)std::min<int32_t>\(K, %d\)\);' % rs.PLANT_Y_MAX,
                r'const bool in_lds = \(size_t\)c->rows \* 16 <= \(size_t\)PLANT_LDS_BYTES;',
                r'Q\.use_hist = c->rows <= RS_HIST_MAX \? 1 : 0;', r'const int use_hist = c->rows <= RS_HIST_MAX \? 1 : 0;',
                r'std::min<int64_t>\(ntiles, RS_BLOCKS_MAX\)', r'std::min<int64_t>\(\(s->M \+ NULL_THREADS - 1\) / NULL_THREADS, NULL_BLOCKS_MAX\)',
                r'std::min<int64_t>\(\(N \+ RS_THREADS - 1\) / RS_THREADS, PLANT_HIST_BLOCKS_MAX\)',
                r'__launch_bounds__\(1024\) void prefix_kernel', r'const bool wide = c->rows > 65535;'):
        assert re.search(pat, src), pat
    assert rs.PLANT_LDS_BYTES == 48 << 10 and rs.RS_TILE == 1024


# ------------------------------------------------------------------------------------------------ tables

@pytest.mark.parametrize('name', sorted(rs.ROWS))
def test_table_rows(name):
    """Under B_2 the table has sum(n + 1) rows; the sizes give the counts the branches are named for."""
    t = rs.table(name)
    assert t.model.rows == sum(n + 1 for n in rs.SIZES[name]) == rs.ROWS[name]
    assert np.all(t.gw[np.isfinite(t.model.g)] > 0.0)              # a complete spectrum: every row a site can hold can be drawn
    rows = t.model.rows
    lds_plant, lds_hist, wide = rows * 16 <= rs.PLANT_LDS_BYTES, rows <= rs.RS_HIST_MAX, rows > 65535
    want = {'t46': (1, 1, 0), 't3072': (1, 1, 0), 't3073': (0, 1, 0), 't8192': (0, 1, 0), 't8193': (0, 0, 0), 't9796': (0, 0, 0),
            't90831': (0, 0, 1), 'one24': (1, 1, 0)}[name]
    assert (lds_plant, lds_hist, wide) == tuple(bool(v) for v in want)
    print(name, rows, 'rows: plant table in', 'LDS' if lds_plant else 'L2', '| histogram in', 'LDS' if lds_hist else 'global memory',
          '|', 4 if wide else 2, 'byte rows')


def test_tables_sit_on_both_sides_of_the_boundaries():
    assert rs.ROWS['t3072'] * 16 == rs.PLANT_LDS_BYTES and rs.ROWS['t3073'] == rs.ROWS['t3072'] + 1
    assert rs.ROWS['t8192'] == rs.RS_HIST_MAX and rs.ROWS['t8193'] == rs.RS_HIST_MAX + 1
    assert rs.RS_HIST_MAX < rs.ROWS['t9796'] <= 65535 < rs.ROWS['t90831']


@pytest.mark.parametrize('name,N', [(n, rs.RS_TABLE_N) for n in ('t8192', 't8193', 't9796')] + [('t9796', rs.RS_2051_TILES)])
def test_sites_occupy_more_rows_than_moment_slots(name, N):
    """More than MOM_SLOTS rows carry sites, before and after resampling: the per-row counts decide which rows get a slot."""
    gen, rows = rs.table(name).sites(N)
    occ = len(np.unique(rows))
    hr = locate.resampled(gen, rows, rs.rs_key(0), 7)[1]
    cnt, cnt_r = np.bincount(rows, minlength=rs.ROWS[name]), np.bincount(hr, minlength=rs.ROWS[name])
    order = lambda c: np.lexsort((np.arange(len(c)), -c))[:rs.MOM_SLOTS]
    print(name, N, 'occupied rows', occ, 'after resampling', len(np.unique(hr)))
    assert occ > rs.MOM_SLOTS and len(np.unique(hr)) > rs.MOM_SLOTS
    assert not np.array_equal(order(cnt), order(cnt_r))            # the ranking of the replicate is its own


# ------------------------------------------------------------------------------------------------ 1. permutation

@pytest.mark.parametrize('name', sorted(rs.PERM_CASES))
def test_permutation_shapes(name):
    tab, N, B, nk, shape = rs.PERM_CASES[name]
    assert rs.feistel_shape(N, B) == shape, rs.feistel_shape(N, B)
    nb = N // B
    keys = rs.perm_keys(nk)
    sig = null.block_permutations(N, keys, B)
    print(name, 'N', N, 'B', B, 'nb', nb, 'h', shape[1], 'domain', shape[2], 'tail', N - nb * B)
    for s in sig:
        assert np.array_equal(np.sort(s), np.arange(N))
        assert np.array_equal(s[nb * B:], np.arange(nb * B, N))    # the tail does not move
        if nb >= 2 and B > 1:
            assert np.array_equal(s[:nb * B] % B, np.arange(nb * B) % B) and np.all(s[:nb * B:B] % B == 0)       # whole blocks move
    if nb < 2:
        assert all(np.array_equal(s, np.arange(N)) for s in sig)
    else:
        assert not np.array_equal(sig[0], sig[1])                  # two keys in a row: the second is not a composition
    if N > 1000000:
        per_pass = rs.PERM_BLOCKS_MAX * rs.PERM_THREADS
        assert per_pass < N < 2 * per_pass and (N - per_pass) % rs.PERM_THREADS != 0 and N % 7 != 0
        assert np.count_nonzero(sig[0][per_pass:] != np.arange(per_pass, N)) > 800       # the second pass moves rows


def test_two_and_three_blocks_visit_every_permutation():
    """nb = 2 and nb = 3 in the 256-value domain: 40 keys give 2 of 2 and 6 of 6 block orders."""
    for name, want in (('n2', 2), ('n3', 6), ('n5b2', 2)):
        tab, N, B, nk, shape = rs.PERM_CASES[name]
        assert nk == rs.N_KEYS == 40
        seen = {tuple((s[:shape[0] * B:B] // B).tolist()) for s in null.block_permutations(N, rs.perm_keys(nk), B)}
        assert seen == set(itertools.permutations(range(shape[0]))) and len(seen) == want, seen


def test_shapes_cover_what_the_issue_names():
    shapes = {rs.PERM_CASES[n][4] for n in rs.PERM_SMALL}
    assert {s[0] for s in shapes} >= {0, 1, 2, 3, 16, 17, 255, 256, 257}
    assert (256, 4, 256) in shapes and (257, 5, 1024) in shapes      # nb = the domain; h steps to 5
    assert rs.table(rs.PERM_CASES['wide257'][0]).model.rows > 65535


# ------------------------------------------------------------------------------------------------ 2. resampling

def test_resampling_shapes():
    tiles = lambda N: (N + rs.RS_TILE - 1) // rs.RS_TILE
    assert [tiles(N) for N in rs.RS_SMALL_N] == [1, 1, 1, 1, 1, 1, 2, 3]
    assert rs.RS_SMALL_N[4:7] == (rs.RS_TILE - 1, rs.RS_TILE, rs.RS_TILE + 1)
    assert set(rs.RS_SMALL_N) >= {rs.RS_PER - 1, rs.RS_PER, rs.RS_PER + 1}               # one thread's four sites, one more, one less
    assert tiles(rs.RS_1024_TILES) == 1024 and rs.RS_1024_TILES % rs.RS_TILE == 0
    assert tiles(rs.RS_2051_TILES) == 2051 == rs.RS_BLOCKS_MAX + 3 and rs.RS_2051_TILES % rs.RS_TILE == 5
    assert tiles(rs.RS_TABLE_N) >= 3
    for N in rs.RS_SMALL_N:
        Bs = rs.rs_small_blocks(N)
        assert set(Bs) >= {1, 2, 3, 4, 5, 7, rs.RS_TILE, rs.RS_TILE + 1, 4 * rs.RS_TILE + 3, N, N + 1}
    print('tiles: small', [tiles(N) for N in rs.RS_SMALL_N], '| 1 048 576 sites', tiles(rs.RS_1024_TILES), '|', rs.RS_2051_TILES, 'sites',
          tiles(rs.RS_2051_TILES))


def test_block_crossings_inside_one_threads_sites():
    """B = 2, 3, 5: how many times a thread steps to the next block (rs_weights' `++rem == B`) within its RS_PER consecutive
    sites -- twice per thread at B = 2, once or twice at B = 3, at most once at B = 5 -- and its weight changes mid-thread."""
    N = 2049
    for B, want in ((2, {2}), (3, {1, 2}), (5, {0, 1})):
        w = boot.site_weights(rs.rs_key(0), N, B)
        i0 = np.arange(0, N - rs.RS_PER + 1, rs.RS_PER)
        steps = {int(np.count_nonzero((np.arange(a, a + rs.RS_PER) + 1) % B == 0)) for a in i0}
        assert steps == want, (B, steps)
        changes = np.array([np.count_nonzero(np.diff(w[a:a + rs.RS_PER])) for a in i0])
        assert changes.max() >= 1


@pytest.mark.parametrize('N', [n for n in rs.RS_SMALL_N if n <= 5])
def test_edge_keys_of_the_short_chromosomes(N):
    for B in rs.rs_small_blocks(N):
        key0, key3 = rs.rs_edge_keys(N, B)
        w0, w3 = boot.site_weights(key0, N, B), boot.site_weights(key3, N, B)
        assert w0.sum() == 0 and w3.max() >= 3
        assert len(locate.resampled(np.arange(N) * 1.0, np.arange(N), key0, B)[0]) == 0
    print(N, 'all-zero and heavy keys found for B in', rs.rs_small_blocks(N))


@pytest.mark.parametrize('N', [rs.RS_1024_TILES, rs.RS_2051_TILES])
def test_large_resamples_fit_and_differ(N):
    for r, B in enumerate(rs.RS_LARGE_B):
        w = boot.site_weights(rs.rs_key(r), N, B)
        tile_sums = np.add.reduceat(w, np.arange(0, N, rs.RS_TILE))
        assert 0 < w.sum() < 2 ** 31 - 1 and len(tile_sums) == (N + rs.RS_TILE - 1) // rs.RS_TILE
        print(N, 'B', B, 'resampled sites', int(w.sum()), 'tile sums', int(tile_sums.min()), '..', int(tile_sums.max()))


# ------------------------------------------------------------------------------------------------ 3. planting

@pytest.mark.parametrize('name', sorted(rs.PLANT_CASES))
def test_planting_cases_are_decided_and_reach_their_edge(name):
    """On the oracle's table: every redrawn site above power.MARGIN, at least 100 of them, and the case's own geometry."""
    c = rs.plant(name)
    N, K = len(c.gen), len(c.centres)
    want, margin = c.host(_R(c.t.name))
    redrawn = np.isfinite(margin)
    changed = np.count_nonzero(want != c.rows)
    first, count = c.runs()
    print(name, 'N', N, 'K', K, 'redrawn', int(redrawn.sum()), 'changed', changed, 'least margin %.3g' % margin[redrawn].min(),
          'longest run', int(count.max()), 'runs of 0 sites', int(np.count_nonzero(count == 0)))
    assert redrawn.sum() >= 100 and changed >= 100 and np.all(margin[redrawn] > power.MARGIN)
    assert np.all(np.isin(want, np.nonzero(c.gw > 0.0)[0]))
    power.check_centres(c.centres, c.A)
    if name in ('t3072', 't3073', 't9796'):
        # the block search's ends: redrawn sites whose source row is the first row a site can hold (k = 1) and the last row
        # (k = n) of the first and of the last size block
        off = c.model.row_off
        src = set(c.rows[redrawn].tolist())
        for j in (0, len(off) - 2):
            assert int(off[j]) + 1 in src and int(off[j + 1]) - 1 in src, j
    if name == 'one24':
        assert len(c.model.sizes) == 1
    if name == 'k4100':
        assert K == rs.PLANT_K > rs.PLANT_Y_MAX and (K + 255) // 256 == 17
        tail = slice(int(first[rs.PLANT_Y_MAX]), N)                # the sites of the centres only grid.y's stride reaches
        assert np.count_nonzero(want[tail] != c.rows[tail]) >= 5
        assert 2 <= np.median(count) <= 12 and c.centres[-1] < c.gen[-1]
    if name == 'zero':
        assert count.tolist()[0] == count.tolist()[2] == count.tolist()[3] == 0 and count[1] > 100
        assert first[0] == 0 and first[2] == rs.ZERO_GAP[0] and first[3] == N
    if name == 'whole':
        assert K == 1 and first[0] == 0 and count[0] == N              # clipped at both ends
    if name == 'hist':
        assert N == rs.PLANT_HIST_N > rs.PLANT_HIST_BLOCKS_MAX * rs.RS_THREADS and first[0] + count[0] == N
        cap = rs.PLANT_HIST_BLOCKS_MAX * rs.RS_THREADS
        assert first[0] < cap and np.count_nonzero(want[cap:] != c.rows[cap:]) >= 50          # rows change in the strided pass


# ------------------------------------------------------------------------------------------------ 4. null accumulation

def test_null_windows():
    assert rs.NULL_CAP == 262144 and rs.NULL_LARGE_M == 2 * 262144 + 300 and rs.NULL_M[1:4] == (255, 256, 257)
    M = rs.NULL_LARGE_M
    assert rs.NULL_MAX_ROWS == (0, 262143, 262144, M - 1)
    for row in rs.NULL_MAX_ROWS:
        lo, hi = rs.null_windows(M, [row])
        empty = lo > hi
        assert empty.sum() == M - 1 and not empty[row] and 0 <= lo[row] <= row <= hi[row] <= M - 1 and hi[row] - lo[row] >= rs.NULL_HALF
    lo, hi = rs.null_windows(M, [])
    assert np.all(lo > hi)                                             # the track that is 0 everywhere
    keep = rs.null_large_keep()
    assert set(rs.NULL_MAX_ROWS) <= set(keep.tolist()) and 2000 < len(keep) < 2100
    assert {int(k) % rs.NULL_THREADS for k in keep} == set(range(rs.NULL_THREADS))       # every thread of a workgroup
    assert np.any(keep < rs.NULL_CAP) and np.any((keep >= rs.NULL_CAP) & (keep < 2 * rs.NULL_CAP)) and np.any(keep >= 2 * rs.NULL_CAP)
    for M in rs.NULL_M:
        Bs = rs.null_blocks(M)
        assert M // Bs[-1] < 2 and (M < 4 or all(M // B >= 2 for B in Bs[:-1]))          # the last replicate is the identity


def test_null_corner_rows_have_a_positive_clr():
    """The one non-empty window of each placement holds a CLR > 0 on the oracle, observed and in the replicate the GPU module
    scans (key 0, B = 1): the maximum sits at that row alone."""
    t = rs.table('t46')
    gen, rows = rs.null_sites(rs.NULL_LARGE_M)
    perm = rows[null.block_permutation(len(gen), rs.null_key(0), 1)]
    L = c_oracle()
    for row in rs.NULL_MAX_ROWS:
        lo, hi = rs.null_windows(len(gen), [row])
        for what, r in (('observed', rows), ('replicate', perm)):
            clr, _, _, iA, _ = c_scan(L, _R('t46'), rs.NULL_AS, gen, r, gen[row:row + 1], lo[row:row + 1], hi[row:row + 1])
            print('row', row, what, 'oracle CLR', clr[0])
            assert iA[0] >= 0 and clr[0] > 1e-3


# ------------------------------------------------------------------------------------------------ 5. per-range argmax

def test_argmax_track_design():
    a = rs.arg_track()
    assert np.all(a.lo[:-1] % rs.WAVE != 0) and a.lo[-1] == a.hi[-1] == a.M - 1
    assert np.any(np.diff(a.test_gen) < 0) and np.any(np.diff(a.test_gen) > 0)          # unsorted
    assert sorted((a.hi - a.lo + 1).tolist()[:7]) == [1, 63, 64, 65, 128, 129, 1000]
    assert set(rs.ARG_KS) == {1, 3, 4, 5, 1001} and rs.ARG_PER_WG == 4 and len(a.lo_all) == 1001
    assert np.all(a.lo_all <= a.hi_all) and a.hi_all.max() == a.M - 1
    by = dict(zip(a.names, zip(a.lo.tolist(), a.hi.tolist())))
    top = np.nonzero(a.site == rs.ARG_TOP)[0]
    lane = lambda name, off: off % rs.WAVE                            # a lane is row - lo, modulo 64
    s, _ = by['same_lane']
    assert {s + 10, s + 74} <= set(top.tolist()) and lane('same_lane', 10) == lane('same_lane', 74)
    s, _ = by['lane63_lane0']
    assert {s + 63, s + 64} <= set(top.tolist()) and lane('', 63) == 63 and lane('', 64) == 0
    s, e = by['last_two']
    assert a.has[s:e + 1].tolist() == [False] * 88 + [True, True]
    s, e = by['none']
    assert not a.has[s:e + 1].any()
    print('M', a.M, 'ranges', len(a.lo), 'rows at the top position', len(top), 'rows without a window', int((~a.has).sum()))


def test_argmax_top_and_mutants_on_the_oracle():
    """The repeated position has the oracle's largest CLR by 1e-3 relative at least, a thousand times what the device and the
    oracle differ by (1e-6, tests/cases.py), so every designed range's maximum is the repeat; on the oracle's track the lane-for-lane restatement of the kernel equals locate.argmax_rows,
    and the butterfly without `ob < best` (either reading) returns another row on designed ranges."""
    a = rs.arg_track()
    L = c_oracle()
    clr, _, _, iA, _ = c_scan(L, _R('t46'), rs.ARG_AS, a.gen, a.rows, a.test_gen, a.win_lo, a.win_hi)
    has = iA >= 0
    assert np.array_equal(has[~a.has], np.zeros((~a.has).sum(), dtype=bool)) and np.all(clr[~a.has] == 0.0)
    top = a.site == rs.ARG_TOP
    assert has[top].all() and len(set(clr[top].tolist())) == 1
    print('oracle: top CLR', clr[top][0], 'next', clr[~top].max())
    assert clr[~top].max() < (1.0 - 1e-3) * clr[top][0]
    row, val = locate.argmax_rows(clr, has, a.lo, a.hi)
    for k, (name, want) in enumerate(zip(a.names, a.want_first())):
        if want is not None:
            assert row[k] == want, name
    lanes = {rule: [rs.wave_argmax(clr, has, int(x), int(y), rule) for x, y in zip(a.lo, a.hi)] for rule in ('first', 'any', 'never')}
    assert lanes['first'] == row.tolist()
    for rule in ('any', 'never'):
        wrong = [n for n, g, w in zip(a.names, lanes[rule], row.tolist()) if g != w]
        print('butterfly tie rule %r fails on' % rule, wrong)
        assert wrong
    lo, hi = a.ranges(1001)
    r1001 = locate.argmax_rows(clr, has, lo, hi)[0]
    assert np.any(r1001 < 0) and np.count_nonzero(r1001 >= 0) > 900 and has.mean() > 0.9
