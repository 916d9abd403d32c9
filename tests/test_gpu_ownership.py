"""What a closed context leaves behind: nothing.  Every device and pinned allocation of the library is held by a buffer that
frees itself, and engine.live_bytes() (bmx_live_bytes) counts the bytes all of them hold in this process.  Each case reads the
two counters first and asks for exactly that reading after its last context is closed -- a difference, not zero: fixtures of
other modules may hold contexts of their own.

Inputs are the worlds of tests/lifetime.py: model g3x3 (21 table rows, 9 pairs, 4 A), chromosome 'S' (700 sites) and its dense
run of 613 test sites with whole-chromosome windows; l2 (483 rows) and g1 for the change of model.
"""
import ctypes as C

import numpy as np
import pytest

import lifetime as lt

pytestmark = pytest.mark.gpu

KEY = 0x1234567890ABCDEF


@pytest.fixture(scope='module')
def engine():
    from ballermixplus_amd import engine
    return engine


def _tests(w):
    gen, rows = w.chroms['S']
    idx = lt.test_index(len(gen), 1)
    assert (len(gen), len(idx)) == (700, 613)
    return gen, rows, idx


def _open(engine, name='g3x3'):
    """A context with the model, the short chromosome and its dense test sites."""
    w = lt.world(name)
    gen, rows, idx = _tests(w)
    ctx = engine.Context(0)
    ctx.set_model(w.model, w.As)
    ctx.set_sites(gen, rows)
    ctx.set_tests(gen[idx])
    return ctx


def test_created_and_closed(engine):
    held = engine.live_bytes()
    ctx = engine.Context(0)
    try:
        assert engine.live_bytes()[0] > held[0]          # the status words at least
    finally:
        ctx.close()
    assert engine.live_bytes() == held


def test_every_group_of_buffers_on_two_slots(engine):
    """Model, sites, tests, scan, refine, support, boot and a peak call on the first and on the last slot; nothing is released
    by hand before the context is closed."""
    held = engine.live_bytes()
    w = lt.world('g3x3')
    gen, rows, idx = _tests(w)
    ctx = engine.Context(0)
    try:
        ctx.set_model(w.model, w.As)
        for slot in (0, lt.MAX_SLOTS - 1):
            before = engine.live_bytes()[0]
            ctx.select_slot(slot)
            ctx.set_sites(gen, rows)
            ctx.set_tests(gen[idx])
            ctx.scan()
            ctx.refine()
            ctx.support(1.0)
            ctx.boot(lt.boot_keys(KEY, 3), block=8)
            assert ctx.peaks(**lt.PEAKS) is not None
            assert ctx.fetch_refined()['rounds'].max() >= 0 and len(ctx.fetch_boot()['window']) > 0
            assert engine.live_bytes()[0] > before
    finally:
        ctx.close()
    assert engine.live_bytes() == held


def test_scan_write_pinned_staging(engine, tmp_path):
    held = engine.live_bytes()
    w = lt.world('g3x3')
    gen, rows, idx = _tests(w)
    ctx = _open(engine)
    try:
        path = tmp_path / 'rows.txt'
        ctx.scan_write(str(path), idx, gen[idx], [repr(v) for v in w.xs], [repr(v) for v in w.abetas], [repr(v) for v in w.As], chunk=64)
        assert len(path.read_bytes().splitlines()) == len(idx)
        assert engine.live_bytes()[1] > held[1]
    finally:
        ctx.close()
    assert engine.live_bytes() == held


def test_larger_model_then_smaller(engine):
    """The context keeps the larger table's arrays for the smaller model (grow-only) and frees them when it goes."""
    held = engine.live_bytes()
    ctx = engine.Context(0)
    try:
        big = lt.world('l2')
        ctx.set_model(big.model, big.As)
        with_big = engine.live_bytes()[0]
        small = lt.world('g1')
        ctx.set_model(small.model, small.As)
        assert engine.live_bytes()[0] == with_big
        assert ctx.fetch_lut()[1].shape == (1, 1, small.model.rows)
    finally:
        ctx.close()
    assert engine.live_bytes() == held


def test_two_contexts_closed_in_opening_order(engine):
    held = engine.live_bytes()
    first = _open(engine)
    try:
        one = engine.live_bytes()[0]
        second = _open(engine)
        try:
            two = engine.live_bytes()[0]
            assert two - one == one - held[0]            # the same calls allocate the same bytes
            first.scan()
            second.scan()
            first.close()
            assert held[0] < engine.live_bytes()[0] < two
            assert np.isfinite(second.fetch()[0]).all()      # the survivor is whole
        finally:
            second.close()
    finally:
        first.close()
    assert engine.live_bytes() == held


def test_one_shot_entry_points_accepted_and_refused(engine):
    """bmx_scan and bmx_lut_build make a context of their own and take it down again, whether the call succeeds or is refused
    (an x grid outside (0, 1): validate_model), and a refusal's message survives the take-down."""
    from ballermixplus_amd import _lib
    held = engine.live_bytes()
    L = _lib.lib()
    w = lt.world('g3x3')
    gen, rows, idx = _tests(w)
    bad = engine.ModelArrays('B2', 1, *w.neutral, [1.5], w.abetas)
    M = len(idx)
    A = _lib.f64(w.As)
    g, r, t = _lib.f64(gen), _lib.i32(rows), _lib.f64(gen[idx])
    lo, hi = _lib.i64(np.zeros(M)), _lib.i64(np.full(M, len(gen) - 1))
    clr = np.full(M, np.nan)
    ix, ia, iA, ns = (np.empty(M, np.int32) for _ in range(4))
    scan = lambda m: L.bmx_scan(C.byref(m.c), _lib.as_dp(A), len(A), len(g), _lib.as_dp(g), _lib.as_ip(r), M, _lib.as_dp(t), _lib.as_lp(lo),
                                _lib.as_lp(hi), _lib.as_dp(clr), _lib.as_ip(ix), _lib.as_ip(ia), _lib.as_ip(iA), _lib.as_ip(ns), 0)
    psel, R = (np.full((w.nx, w.nab, w.model.rows), np.nan) for _ in range(2))
    lut = lambda m: L.bmx_lut_build(C.byref(m.c), _lib.as_dp(psel), _lib.as_dp(R), 0)
    for call in (scan, lut):
        assert call(w.model) == 0, L.bmx_last_error()
        assert engine.live_bytes() == held
        assert call(bad) == lt.INVALID and b'x grid must lie in (0,1)' in L.bmx_last_error()
        assert engine.live_bytes() == held
    assert np.isfinite(clr).all() and np.isfinite(R).any()           # both calls did hand their results out
