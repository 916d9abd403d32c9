"""The listed-window kernels' outputs, byte for byte: sha256 digests of the raw arrays of ctx.surfaces and ctx.influence on every
case of influencecases.py and of ctx.fit on every case of fitcases.py (both homes of the prologue sums), against
tests/golden/listed/hashes.json.  The other tests of these families compare with a host restatement to a tolerance and would
not see a changed rounding; profiles/listed_window_fold.txt names the commit whose library the file was recorded with."""
import hashlib
import json
import os

import numpy as np
import pytest

import fitcases as fc
import influencecases as ic
from test_gpu_refine import _engine
from util import GOLD

pytestmark = pytest.mark.gpu

INFLUENCE_KEYS = ('T_max', 'lin', 'ns_min', 'first_block', 'offset', 'm', 'contrib', 'L', 'blin')


def _digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def digests():
    """{'surfaces/<case>', 'influence/<case>/<block>', 'fit/<case>/<lds|global>': sha256 of the call's arrays in their order}"""
    eng = _engine()
    got = {}
    for name in ic.NAMES:
        cat = ic.catalogue(eng)[name]()
        ctx = cat.context(eng)
        got['surfaces/%s' % name] = _digest(ctx.surfaces(cat.windows))
        for B in ic.BLOCKS:
            r = ctx.influence(cat.windows, B)
            got['influence/%s/%d' % (name, B)] = _digest(r[k] for k in INFLUENCE_KEYS)
        ctx.close()
    for name in fc.NAMES:
        c = fc.catalogue(eng)[name]()
        ctx = c.cat.context(eng)
        for variant, home in ((0, 'lds'), (1, 'global')):       # (a case too large for LDS works in device memory either way)
            ctx.set_variant(variant)
            got['fit/%s/%s' % (name, home)] = _digest(ctx.fit(c.tests(), c.lins(), c.gw, c.cls, c.F, c.edges))
        ctx.close()
    return got


def test_listed_outputs_unchanged():
    with open(os.path.join(GOLD, 'listed', 'hashes.json')) as f:
        want = json.load(f)
    got = digests()
    for k in sorted(want):
        if got.get(k) != want[k]:
            print('differs: %s' % k)
    assert got == want
