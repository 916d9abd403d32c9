"""The kernels that make the replicates, at their edges (the catalogue is tests/resamplers.py; tests/test_resamplers_cpu.py shows
that each case reaches its edge): the device's permuted rows, resampled and planted site arrays, null counts and maxima and
per-range argmax rows against the package's host restatements.  Every comparison is integer-exact or bit for bit."""
import numpy as np
import pytest

import resamplers as rs

from ballermixplus_amd import boot, locate, null, power

pytestmark = pytest.mark.gpu

AS = (500.0, 2000.0)


def _engine():
    from ballermixplus_amd import engine
    return engine


def _bits(res):
    clr, ix, ia, iA, ns = res
    return (np.asarray(clr, dtype=np.float64).view(np.uint64), ix, ia, iA, ns)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b)))


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _scan(ctx, test_gen, lo=None, hi=None):
    ctx.set_tests(test_gen, lo, hi)
    ctx.scan()
    return ctx.fetch()


def _ctx(t, As, gen, rows):
    ctx = _engine().Context(0)
    ctx.set_model(t.model, As)
    ctx.set_sites(gen, rows)
    return ctx


def _source_untouched(ctx, gen, rows):
    ctx.select_slot(0)
    g0, r0 = ctx.fetch_sites(len(gen))
    assert np.array_equal(_u64(g0), _u64(gen)) and np.array_equal(r0, rows)


def _is_a_set_sites_slot(ctx, g, r, tests):
    """The selected slot (sites built on the device; g, r: fetched from it) against slot 2 given g, r through set_sites: the five
    result fields bit-equal, plan() equal -- the one observable of the per-row counts the device made."""
    got = _scan(ctx, tests)
    plan = ctx.plan()
    ctx.select_slot(2)
    ctx.set_sites(g, r)
    want = _scan(ctx, tests)
    assert _same(got, want) and ctx.plan() == plan, (plan, ctx.plan())
    assert np.count_nonzero(got[3] >= 0) >= 20             # (a track without results would say nothing)
    return got


# ------------------------------------------------------------------------------------------------ 1. permutation

def _check_permuted(name):
    tab, N, B, nk, shape = rs.PERM_CASES[name]
    t = rs.table(tab)
    gen, rows = t.sites(N)
    ctx = _ctx(t, AS, gen, rows)
    keys = rs.perm_keys(nk)
    sig = null.block_permutations(N, keys, B)
    moved = 0
    for key, s in zip(keys, sig):                          # every call permutes the rows GIVEN: not a composition
        ctx.permute_rows(key, B)
        g, r = ctx.fetch_sites()
        assert np.array_equal(r, rows[s]), (name, hex(key))
        assert np.array_equal(_u64(g), _u64(gen))
        moved += int(np.count_nonzero(s != np.arange(N)))
    assert (moved > 0) == (shape[0] >= 2)
    if name in rs.PERM_RESTORE:
        ctx.restore_rows()
        g, r = ctx.fetch_sites()
        assert np.array_equal(r, rows) and np.array_equal(_u64(g), _u64(gen))
    ctx.close()


@pytest.mark.parametrize('name', rs.PERM_SMALL)
def test_permuted_rows_small_shapes(name):
    """nb = 0 .. 3, 16, 17, 255, 256 (the whole domain), 257 (h = 5), tails that stay, 2- and 4-byte rows."""
    _check_permuted(name)


@pytest.mark.parametrize('name', ['largeB1', 'largeB7'])
def test_permuted_rows_past_the_launch_cap(name):
    """2 097 997 sites: the grid-stride loop's second pass, with a ragged end (and at B = 7 a tail of 6 sites)."""
    _check_permuted(name)


# ------------------------------------------------------------------------------------------------ 2. resampling

def _check_resampled(ctx, gen, rows, key, B):
    """resample_sites of slot 0 into the selected slot against locate.resampled; returns the fetched arrays (None: no sites)."""
    eng = _engine()
    n = ctx.resample_sites(0, key, B)
    w = boot.site_weights(key, len(gen), B)
    assert n == int(w.sum()), (len(gen), B, hex(key))
    if n == 0:
        with pytest.raises(eng._lib.BmxError) as e:
            ctx.fetch_sites(1)
        assert e.value.code == -5
        return None
    g, r = ctx.fetch_sites()
    hg, hr = locate.resampled(gen, rows, key, B)
    assert len(g) == n == len(hg)
    assert np.array_equal(_u64(g), _u64(hg)), (len(gen), B, hex(key))
    assert np.array_equal(r, np.asarray(hr, dtype=np.int32)), (len(gen), B, hex(key))
    return g, r


@pytest.mark.parametrize('N', rs.RS_SMALL_N)
def test_resampled_sites_small_shapes(N):
    """N at the RS_PER and tile edges, B from 1 to past N: two ordinary keys each, and for N <= 5 an all-zero weight vector and a
    weight >= 3."""
    t = rs.table('t46')
    gen, rows = t.sites(N)
    ctx = _ctx(t, AS, gen, rows)
    ctx.select_slot(1)
    empty = heavy = 0
    for B in rs.rs_small_blocks(N):
        for key in rs.rs_small_keys(N, B):
            got = _check_resampled(ctx, gen, rows, key, B)
            empty += got is None
            heavy += got is not None and boot.site_weights(key, N, B).max() >= 3
    assert N > 5 or (empty >= len(rs.rs_small_blocks(N)) and heavy >= len(rs.rs_small_blocks(N)))
    _source_untouched(ctx, gen, rows)
    ctx.close()


@pytest.mark.parametrize('r,B', list(enumerate(rs.RS_LARGE_B)))
def test_resampled_sites_1024_tiles(r, B):
    """1 048 576 sites: exactly 1 024 tile sums, one per thread of prefix_kernel."""
    t = rs.table('t46')
    gen, rows = t.sites(rs.RS_1024_TILES)
    ctx = _ctx(t, AS, gen, rows)
    ctx.select_slot(1)
    _check_resampled(ctx, gen, rows, rs.rs_key(r), B)
    _source_untouched(ctx, gen, rows)
    ctx.close()


@pytest.mark.parametrize('tab,r,B', [('t46', r, B) for r, B in enumerate(rs.RS_LARGE_B)] + [('t9796', 1, 7)])
def test_resampled_sites_2051_tiles(tab, r, B):
    """2 099 205 sites, 2 051 tiles on 2 048 workgroups: workgroups 0 .. 2 take a second tile (the block scan's and the tile sum's LDS
    are reused, the LDS histogram carries over), prefix_kernel's threads take up to three tile sums each; then the slot's state."""
    t = rs.table(tab)
    gen, rows = t.sites(rs.RS_2051_TILES)
    ctx = _ctx(t, AS, gen, rows)
    ctx.select_slot(1)
    g, r_ = _check_resampled(ctx, gen, rows, rs.rs_key(r), B)
    _is_a_set_sites_slot(ctx, g, r_, rs.strided_tests(gen))
    _source_untouched(ctx, gen, rows)
    ctx.close()


@pytest.mark.parametrize('tab', rs.RS_TABLES)
def test_resampled_sites_across_the_table_sizes(tab):
    """5 000 sites (five tiles) on tables of 46, 8 192 (the last LDS histogram), 8 193 and 9 796 (2-byte rows, global atomics) and
    90 831 rows (4-byte rows); then the slot's state, which the device's per-row counts decide."""
    t = rs.table(tab)
    gen, rows = t.sites(rs.RS_TABLE_N)
    ctx = _ctx(t, AS, gen, rows)
    for r, B in enumerate((1, 7)):
        ctx.select_slot(1)
        g, r_ = _check_resampled(ctx, gen, rows, rs.rs_key(r), B)
        _is_a_set_sites_slot(ctx, g, r_, rs.strided_tests(gen))
    _source_untouched(ctx, gen, rows)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 3. planting

@pytest.mark.parametrize('name', sorted(rs.PLANT_CASES))
def test_planted_rows(name):
    """plant_sites from slot 0 into slot 1 against power.planted_rows on the DEVICE's table (every redrawn site decided, at least
    100 of them): rows, runs and the number of changed rows; the source untouched; the slot a set_sites slot."""
    c = rs.plant(name)
    N = len(c.gen)
    ctx = _ctx(c.t, c.As, c.gen, c.rows)
    R = ctx.fetch_lut()[1]
    ctx.select_slot(1)
    first, count, changed = ctx.plant_sites(0, c.key, c.centres, *c.planted, c.gw)
    g, r = ctx.fetch_sites(N)
    want, margin = c.host(R)
    redrawn = np.isfinite(margin)
    assert redrawn.sum() >= 100 and np.all(margin[redrawn] > power.MARGIN)
    assert np.array_equal(_u64(g), _u64(c.gen))
    assert np.array_equal(r, want), np.nonzero(r != want)[0][:10]
    hf, hc = c.runs()
    assert np.array_equal(first, hf) and np.array_equal(count, hc)
    assert changed == np.count_nonzero(want != c.rows) >= 100
    assert ctx.plant_ms() > 0.0
    _is_a_set_sites_slot(ctx, g, r, rs.strided_tests(c.gen))
    _source_untouched(ctx, c.gen, c.rows)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 4. null accumulation

@pytest.mark.parametrize('M', rs.NULL_M)
def test_null_counts_and_maxima(M):
    """Every site a test site; three permuted replicates and the identity (B > N / 2: bit-equal to the observed track, so every
    count rises -- the `>=`); the large M strides null_count_kernel twice and a bit and gives null_max_kernel 1 024 partials."""
    t = rs.table('t46')
    gen, rows = rs.null_sites(M)
    ctx = _ctx(t, rs.NULL_AS, gen, rows)
    if M == rs.NULL_LARGE_M:
        lo, hi = rs.null_windows(M, rs.null_large_keep())
        obs = _scan(ctx, gen, lo, hi)
        assert np.count_nonzero(obs[0]) > 1500 and np.count_nonzero(obs[0] == 0.0) >= M - len(rs.null_large_keep())
    else:
        obs = _scan(ctx, gen)
    ctx.null_begin()
    counts = np.zeros(M, dtype=np.int64)
    Bs = rs.null_blocks(M)
    for r, B in enumerate(Bs):
        before = counts.copy()
        ctx.permute_rows(rs.null_key(r), B)
        ctx.scan()
        rep = ctx.fetch()
        m = ctx.null_accumulate()
        assert _u64([m])[0] == _u64([rep[0].max()])[0]
        counts += rep[0] >= obs[0]
        if r == len(Bs) - 1:                               # the identity
            assert _same(rep, obs) and np.array_equal(counts, before + 1)
        got, reps = ctx.null_fetch()
        assert reps == r + 1 and np.array_equal(got, counts)
    if M >= 255:
        assert counts.min() >= 1 and counts.max() == len(Bs) and len(np.unique(counts)) >= 2
    ctx.null_begin()                                       # a second begin: counts and replicates start over
    got, reps = ctx.null_fetch()
    assert reps == 0 and not got.any()
    ctx.close()


@pytest.mark.parametrize('row', rs.NULL_MAX_ROWS + (None,))
def test_null_maximum_from_one_row(row):
    """524 588 test sites, every window empty (CLR exactly 0, and 0 >= 0 counts) but one: row 0, the last row of the first pass,
    the first of the strided pass, the last row.  None: no window at all, and the maximum is 0.0."""
    M = rs.NULL_LARGE_M
    t = rs.table('t46')
    gen, rows = rs.null_sites(M)
    ctx = _ctx(t, rs.NULL_AS, gen, rows)
    lo, hi = rs.null_windows(M, [] if row is None else [row])
    obs = _scan(ctx, gen, lo, hi)
    ctx.null_begin()
    ctx.permute_rows(rs.null_key(0), 1)
    ctx.scan()
    rep = ctx.fetch()
    m = ctx.null_accumulate()
    got, reps = ctx.null_fetch()
    want = (rep[0] >= obs[0]).astype(np.int32)
    assert reps == 1 and np.array_equal(got, want)
    others = np.ones(M, dtype=bool)
    if row is None:
        assert m == 0.0 and not np.signbit(m)
    else:
        others[row] = False
        assert obs[0][row] > 0.0 and rep[0][row] > 0.0 and rep[0][row] != obs[0][row]
        assert _u64([m])[0] == _u64(rep[0][row:row + 1])[0]
    assert not rep[0][others].any() and not obs[0][others].any() and np.all(got[others] == 1)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 5. per-range argmax

def test_argmax_rows_on_designed_ties():
    """Unsorted test positions (one test site per wave), one position repeated at chosen rows of ranges that begin off the 64-row
    grid, rows without a window for rows without a result: fetch_locate against locate.argmax_rows on the fetched track."""
    a = rs.arg_track()
    ctx = _ctx(a.t, rs.ARG_AS, a.gen, a.rows)
    track = _scan(ctx, a.test_gen, a.win_lo, a.win_hi)
    assert ctx.plan()['mode'] == 5, ctx.plan()
    clr, has = track[0], track[3] >= 0
    top = a.site == rs.ARG_TOP
    assert len(np.unique(_u64(clr[top]))) == 1 and has[top].all()      # the premise: repeats are bit-equal
    assert clr[~top].max() < clr[top][0]                                # ... and the maximum of every range that holds one
    assert not has[~a.has].any() and has.mean() > 0.9

    def permuted():
        ctx.permute_rows(rs.null_key(3), 1)
        ctx.scan()

    for K in rs.ARG_KS:
        lo, hi = a.ranges(K)
        scans = [ctx.scan, permuted] if K == 1001 else [ctx.scan]
        ctx.locate_begin(lo, hi, len(scans))
        want_row, want_clr = [], []
        for r, launch in enumerate(scans):
            launch()
            ctx.locate_accumulate(r)
            t = ctx.fetch()
            assert r > 0 or _same(t, track)
            assert len(np.unique(_u64(t[0][top]))) == 1
            w = locate.argmax_rows(t[0], t[3] >= 0, lo, hi)
            want_row.append(w[0])
            want_clr.append(w[1])
        row, val = ctx.fetch_locate()
        assert np.array_equal(row, np.array(want_row)), (K, np.nonzero(row != np.array(want_row)))
        assert np.array_equal(_u64(val), _u64(np.array(want_clr)))
        ctx.restore_rows()
        if K >= len(a.lo):
            for k, (name, want) in enumerate(zip(a.names, a.want_first())):
                if want is not None:
                    assert row[0, k] == want, name
            assert row[0, len(a.lo) - 1] == a.M - 1                     # lo = hi = M - 1
    ctx.close()
