"""The listed-window kernels' outputs, byte for byte: sha256 digests of the raw arrays of ctx.surfaces and ctx.influence on every
case of influencecases.py, of ctx.fit on every case of fitcases.py (both homes of the prologue sums), of ctx.cond_surfaces on
every case of condcases.py (pairs with shared sites and pairs without) and of ctx.base_surfaces on the fast cases of stepcases.py
(against the empty baseline, after one and after two loci, with the baseline itself), against tests/golden/listed/hashes.json.
The other tests of these families compare with a host restatement to a tolerance and would not see a changed rounding;
profiles/listed_window_fold.txt and profiles/listed_surfaces_fold.txt name the commits whose libraries the file was recorded with."""
import hashlib
import json
import os

import numpy as np
import pytest

import condcases as cc
import fitcases as fc
import influencecases as ic
import stepcases as sc
from test_gpu_conditional import _scan_lin
from test_gpu_refine import _engine
from util import GOLD

pytestmark = pytest.mark.gpu

INFLUENCE_KEYS = ('T_max', 'lin', 'ns_min', 'first_block', 'offset', 'm', 'contrib', 'L', 'blin')
SURFACE_KEYS = ('T', 'nsites', 'nshared', 'tmax', 'lin')         # of ctx.cond_surfaces and ctx.base_surfaces


def _digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def digests():
    """{'surfaces/<case>', 'influence/<case>/<block>', 'fit/<case>/<lds|global>', 'cond_surfaces/<case>', 'base_surfaces/<case>/<loci
    in the baseline>': sha256 of the call's arrays in their order; with loci in the baseline, baseline_fetch's d and cnt after them}"""
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
    for name in cc.NAMES:
        cat = cc.catalogue(eng)[name]()
        ctx = cat.context(eng)
        lin = _scan_lin(ctx, name, len(cat.tg))
        pairs = [(t, c, int(lin[c])) for t, c in cc.neighbours(cat)]
        far = cc.unreachable(cat)
        if far is not None:
            pairs += [(t, far[0], far[1]) for t in cat.windows]
        r = ctx.cond_surfaces(*zip(*pairs))
        got['cond_surfaces/%s' % name] = _digest(r[k] for k in SURFACE_KEYS)
        ctx.close()
    for name in sc.FAST:
        c = sc.case(name, eng)
        ctx = c.context(eng)
        apex = c.apex.astype(np.int32)
        ctx.baseline_reset()
        r = ctx.base_surfaces(apex)
        got['base_surfaces/%s/0' % name] = _digest(r[k] for k in SURFACE_KEYS)
        # the loci: the case's first apexes at their grid argmax (the scan's rule; where nothing is > 0, the highest point)
        held = np.where(r['lin'] >= 0, r['lin'], np.argmax(np.where(np.isnan(r['T']), -np.inf, r['T']).reshape(len(apex), -1), axis=1))
        for k in (1, 2):
            j = (k - 1) % len(apex)
            ctx.baseline_add(int(apex[j]), int(held[j]))
            r = ctx.base_surfaces(apex)
            got['base_surfaces/%s/%d' % (name, k)] = _digest([r[key] for key in SURFACE_KEYS] + list(ctx.baseline_fetch(len(c.gen))))
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
