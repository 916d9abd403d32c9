"""A census of the cases of tests/foldtails.py, on the CPU: prep_kernel's classification (slot of a row, far / series / near, the
orders a far site adds) restated in numpy on the oracle's table, and counted -- the top order of every moment entry, the real
entries in the last block of every near list.  It is a census of what tests/test_gpu_fold_tails.py exercises, not a comparison
with the device: it keeps the case set from losing a class when somebody changes an A list or a range of test sites."""
import numpy as np
import pytest

import foldtails as ft
from util import oracle_R, orc

NEED = 8        # occurrences of every class over the case set


@pytest.fixture(scope='module')
def zones():
    """{case: census records}; the oracle's table once per data set."""
    zcut = orc.alpha_cut_z()
    data = {d: ft.host_data(d, oracle_R) for d in sorted({c['data'] for c in ft.CASES.values()})}
    return {name: ft.census(*data[ft.CASES[name]['data']], name, zcut) for name in sorted(ft.CASES)}


def test_per_case_counts(zones):
    for name, zs in zones.items():
        t = ft.tally(zs)
        print('%-36s orders %s  quad tails %s  pair tails %s' % (name, list(t['order'].values()), list(t['quad_tail'].values()),
                                                                 list(t['pair_tail'][16 if zs[0]['J'] >= 16 else 8].values())))
        assert sum(t['order'].values()) > 0 and sum(t['quad_tail'].values()) > 0, name


def test_every_class_occurs(zones):
    t = ft.tally([z for zs in zones.values() for z in zs])
    print(t)
    assert sorted(t['order']) == list(range(2, 13)) and min(t['order'].values()) >= NEED, t['order']
    assert t['mixed_step'] >= NEED                      # a fold step whose two entries differ in their top order
    assert t['odd_occ'] >= NEED and t['one_occ'] >= NEED and t['one_side'] >= NEED
    assert min(t['quad_tail'].values()) >= NEED, t['quad_tail']
    assert min(t['pair_tail'][16].values()) >= NEED and min(t['pair_tail'][8].values()) >= NEED, t['pair_tail']
    assert t['single_block'] >= NEED and t['empty_pair'] >= NEED and t['empty_quad'] >= NEED and t['long_quad'] >= NEED


def test_forms(zones):
    """Both table placements and both group sizes see every fold cut and every tail on their own."""
    forms = {}
    for name, zs in zones.items():
        forms.setdefault(ft.CASES[name]['kernel'], []).extend(zs)
    assert sorted(forms) == sorted(ft.PREP % (j, l) for j in (16, 8) for l in ('true', 'false'))
    for kernel, zs in forms.items():
        t = ft.tally(zs)
        assert min(t['order'].values()) >= NEED, (kernel, t['order'])
        assert min(t['quad_tail'].values()) >= NEED, (kernel, t['quad_tail'])
        assert min(t['pair_tail'][16 if zs[0]['J'] >= 16 else 8].values()) >= NEED, (kernel, t['pair_tail'])
        assert t['mixed_step'] >= NEED and t['odd_occ'] >= NEED, kernel
