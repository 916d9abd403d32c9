"""The per-zone scalars of the prepared pipeline -- F_j of both zones, G_k / H_k and the flag of the triangle, the list budgets --
are computed ONCE per group by prep_kernel and read by the eight slice-waves as scalar loads from the stream.  They are the same
doubles from the same device functions as when every slice-wave computed them, so every result must be what it was, bit for bit:
tests/golden/stream_scalars.npz holds the records (clr bits, lin, nsites), the plan and the profiles' bits of every case of
tests/streamscalars.py as the commit before that change computed them (tests/golden/gen_stream_scalars.py).

Every case is also held to the project's bar against the C oracle fed the device's own table: (x, alpha_beta, A) and nSites equal
on every window the oracle decides (runner-up more than 1e-7 of T behind: at most 2 % are not), CLR rtol 1e-9, atol 1e-12 on all.
Each case is scanned twice on its context (two scans in a row); contexts are shared between the cases of a data set and A list,
so most cases also follow other test sites, variants and profile settings on a long-lived context."""
import hashlib
import os

import numpy as np
import pytest

import streamscalars as ss
from util import GOLD, c_oracle, c_scan

pytestmark = pytest.mark.gpu

NAMES = sorted(ss.CASES)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope='module')
def gold():
    g = np.load(os.path.join(GOLD, 'stream_scalars.npz'))
    assert list(g['names']) == NAMES            # the golden file was written for exactly these cases
    return g


@pytest.fixture(scope='module')
def opened():
    """opened(data set, A list) -> (context, genPos, rows, device table): one per module, closed at its end."""
    from ballermixplus_amd import engine as eng
    made = {}

    def get(data, a):
        if (data, a) not in made:
            made[(data, a)] = ss.open_data(eng, data, a)
        return made[(data, a)]

    yield get
    for ctx, _, _, _ in made.values():
        ctx.close()


@pytest.mark.parametrize('name', NAMES)
def test_bits_of_the_parent_and_the_oracle(name, gold, opened):
    c = ss.CASES[name]
    ctx, gen, rows, R = opened(c['data'], c['a'])
    tag = 'case%02d' % NAMES.index(name)
    orc = ss.oracle(c_scan, c_oracle(), R, gen, rows, name)
    for turn in ('first scan', 'second scan'):
        rec, plan, prof = ss.run(ctx, gen, name)
        what = '%s, %s' % (name, turn)
        assert plan['kernel'] == str(gold[tag + '_kernel']), (what, plan)
        assert c['kernel'] is None or plan['kernel'] == c['kernel'], (what, plan)
        diff = np.nonzero(_bits(rec['clr']) != gold[tag + '_clr'])[0]
        assert len(diff) == 0, (what, diff[:8], rec['clr'][diff[:4]], gold[tag + '_clr'][diff[:4]].view(np.float64))
        assert np.array_equal(rec['lin'], gold[tag + '_lin']), what
        assert np.array_equal(rec['nsites'], gold[tag + '_nsites']), what
        if c['profiles']:
            for k in ('A', 'x', 'abeta'):
                assert np.array_equal(_bits(prof[k]), gold[tag + '_prof_' + k]), (what, k)
                assert np.array_equal(_bits(prof[k].max(axis=1)), _bits(rec['clr'])), (what, k)
        ss.check_oracle(rec, orc, what)


def test_launch_ranges(gold):
    """2^18 test sites with profiles on: three launch ranges.  Every record equals the parent's (digest of all of them; the
    sampled ones array for array), and the windows on both sides of every cut meet the oracle's bar."""
    from ballermixplus_amd import engine as eng
    ctx, gen, rows, As = ss.ranges_ctx(eng)
    try:
        ctx.scan()
        rec = ctx.fetch_records()
        cuts = ctx.launch_ranges()
        assert len(cuts) >= 2 and np.array_equal(cuts, gold['ranges_cuts']), cuts
        assert ctx.plan()['kernel'] == 'clr_scan_prepared_kernel<16,true>'
        at = gold['ranges_at']
        assert np.array_equal(at, ss.ranges_sample(cuts, len(rec)))
        diff = np.nonzero(_bits(rec['clr'][at]) != gold['ranges_clr'])[0]
        assert len(diff) == 0, (at[diff[:8]],)
        assert np.array_equal(rec['lin'][at], gold['ranges_lin']) and np.array_equal(rec['nsites'][at], gold['ranges_nsites'])
        assert hashlib.sha256(rec.tobytes()).hexdigest() == str(gold['ranges_sha256'])
        assert hashlib.sha256(ctx.fetch_profile('A').tobytes()).hexdigest() == str(gold['ranges_prof_A_sha256'])
        # the oracle on 32 windows around every cut (the whole grid: 5 100 points, windows of up to a few thousand sites)
        R = ctx.fetch_lut()[1]
        R = np.where(np.isfinite(R), R, 0.0)
        pick = np.unique(np.concatenate([np.arange(max(int(c) - 16, 0), min(int(c) + 16, len(rec))) for c in cuts]))
        n = len(gen)
        clr, ix, ia, iA, ns = c_scan(c_oracle(), R, As, gen, rows, gen[pick], np.zeros(len(pick), np.int64), np.full(len(pick), n - 1, np.int64))
        nx, nab = R.shape[0], R.shape[1]
        lin = np.where(iA >= 0, (iA * nx + ix) * nab + ia, -1)
        worst = float(np.max(np.abs(rec['clr'][pick] - clr) / np.maximum(np.abs(clr), 1e-300)))
        print('launch ranges: cuts %s, %d windows against the oracle, worst relative dCLR %.3e' % (cuts.tolist(), len(pick), worst))
        assert np.array_equal(rec['lin'][pick], lin) and np.array_equal(rec['nsites'][pick], ns)
        assert np.allclose(rec['clr'][pick], clr, rtol=1e-9, atol=1e-12), worst
    finally:
        ctx.close()
