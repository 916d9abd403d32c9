"""The prepared scan kernels skip the pair steps of two neutral entries in a pair list's last block and take the one- or two-site
form for a quad list's last block with one or two real entries (prep_kernel hands them the number of neutral entries in the low
bits of the header's list lengths).  What is skipped is arithmetic of the form x * 1.0 or fma(F, +-0, c), so every result must be
what it was, bit for bit: tests/golden/fold_tails.npz holds the records (clr bits, lin, nsites), the
plan and the profiles' bits of every case of tests/foldtails.py as the commit before that change computed them
(tests/golden/gen_fold_tails.py).  What the cases cover is counted by tests/test_fold_tails_cpu.py: every remainder of real
entries in both kinds of last block, and the moment entries of every top order (a fold that stops at an entry's top order was
measured slower and is not in the library; its cases stay in the fixture).

Every case is also held to the project's bar against the C oracle fed the device's own table: (x, alpha_beta, A) and nSites equal
on every window the oracle decides (runner-up more than 1e-7 of T behind: at most 2 % are not), CLR rtol 1e-9, atol 1e-12 on all.
Each case is scanned twice on its context; contexts are shared between the cases of a data set and A list, so most cases also
follow other test sites, windows and profile settings on a long-lived context."""
import os

import numpy as np
import pytest

import foldtails as ft
from util import GOLD, c_oracle, c_scan

pytestmark = pytest.mark.gpu

NAMES = sorted(ft.CASES)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope='module')
def gold():
    g = np.load(os.path.join(GOLD, 'fold_tails.npz'))
    assert list(g['names']) == NAMES            # the golden file was written for exactly these cases
    return g


@pytest.fixture(scope='module')
def opened():
    """opened(data set, A list) -> (context, genPos, rows, device table): one per module, closed at its end."""
    from ballermixplus_amd import engine as eng
    made = {}

    def get(data, a):
        if (data, a) not in made:
            made[(data, a)] = ft.open_data(eng, data, a)
        return made[(data, a)]

    yield get
    for ctx, _, _, _ in made.values():
        ctx.close()


@pytest.mark.parametrize('name', NAMES)
def test_bits_of_the_parent_and_the_oracle(name, gold, opened):
    c = ft.CASES[name]
    ctx, gen, rows, R = opened(c['data'], c['a'])
    tag = 'case%02d' % NAMES.index(name)
    orc = ft.oracle(c_scan, c_oracle(), R, gen, rows, name)
    for turn in ('first scan', 'second scan'):
        rec, plan, prof = ft.run(ctx, gen, name)
        what = '%s, %s' % (name, turn)
        assert plan['kernel'] == str(gold[tag + '_kernel']), (what, plan)
        assert plan['kernel'] == c['kernel'], (what, plan)
        diff = np.nonzero(_bits(rec['clr']) != gold[tag + '_clr'])[0]
        assert len(diff) == 0, (what, diff[:8], rec['clr'][diff[:4]], gold[tag + '_clr'][diff[:4]].view(np.float64))
        assert np.array_equal(rec['lin'], gold[tag + '_lin']), what
        assert np.array_equal(rec['nsites'], gold[tag + '_nsites']), what
        if c['profiles']:
            for k in ('A', 'x', 'abeta'):
                assert np.array_equal(_bits(prof[k]), gold[tag + '_prof_' + k]), (what, k)
                assert np.array_equal(_bits(prof[k].max(axis=1)), _bits(rec['clr'])), (what, k)
        ft.check_oracle(rec, orc, what)
