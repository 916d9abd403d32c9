"""tests/lifetime.py on the host: the scripts that tests/test_gpu_lifetime.py runs in one long-lived context are deterministic, hold
every transition they are meant to hold, run every op group before every other, compare every group at least five times and meet
every error code; the state model answers a table of rows restated from include/bmxscan.h as the header does; and the site arrays
it expects after permute, restore, resample and plant are what the package's host restatements give.  The scripts from before the
baseline and sandwich calls had ops are pinned by their sha256; the fit ops reach both homes of the prologue sums, the sandwich ops
both homes of the refinement's workspace and both block paths; and every baseline a script builds is replayed on the oracle's
table with stepwise.host_baseline_add from the loci and row states the state model recorded.  No GPU."""
import collections
import hashlib
import os
import re

import numpy as np
import pytest

import lifetime as lt
from lifetime import INVALID, LIMIT, STATE, op

from ballermixplus_amd import boot, null, power


@pytest.fixture(scope='module')
def scripts():
    return lt.scripts()


def _run(ops, R_of=lambda m: None):
    """[(op, code, snapshot)] with what the detectors below look at."""
    out = []
    for o, code, st in lt.replay(ops, R_of=R_of):
        s = st.slot
        out.append((o, code, {
            'slot': st.cur, 'model': st.model, 'N': 0 if s.sites is None else len(s.sites['gen']), 'M': s.M, 'seq': s.seq,
            'profiles': st.profiles, 'variant': st.variant, 'perm': s.perm, 'tests': id(s.tests) if s.tests is not None else None,
            'with_sites': sorted(k for k, v in st.slots.items() if v.sites is not None), 'with_results': st.with_results(),
            'null_reps': None if s.null is None else len(s.null['reps']),
            'lc': None if s.lc is None else (s.lc['K'], s.lc['R'], sorted({r for r, _ in s.lc['acc']})),
            'src': None if s.sites is None else s.sites['src'],
            'perm_of': {k: v.perm for k, v in st.slots.items()}, 'compared': code == 0 and lt.is_compared(o, st),
            'bl': None if s.bl is None else len(s.bl), 'bl_of': {k: None if v.bl is None else len(v.bl) for k, v in st.slots.items()},
            'N_of': {k: 0 if v.sites is None else len(v.sites['gen']) for k, v in st.slots.items()},
            'windows': None if s.tests is None else s.tests['windows'], 'stride': None if s.tests is None else s.tests['stride']}))
    return out


def _find(run, start, pred):
    """Index of the first entry at or after `start` that satisfies pred(op, code, snapshot), or -1."""
    for i in range(start, len(run)):
        if pred(*run[i]):
            return i
    return -1


def _chain(run, preds, same_slot=True):
    """True if the entries matching preds occur in that order (others may lie between), all in one slot if same_slot."""
    for first in range(len(run)):
        if not preds[0](*run[first]):
            continue
        slot, at, ok = run[first][2]['slot'], first, True
        for p in preds[1:]:
            at = _find(run, at + 1, lambda o, c, s: p(o, c, s) and (not same_slot or s['slot'] == slot))
            if at < 0:
                ok = False
                break
        if ok:
            return True
    return False


def ok(name, **want):
    return lambda o, c, s: o[0] == name and c == 0 and all(o[1].get(k) == v for k, v in want.items())


def refused(name, code):
    return lambda o, c, s: o[0] == name and c == code


def test_scripts_are_deterministic(scripts):
    again = lt.scripts()
    assert list(again) == ['hand'] + ['walk%d' % s for s in lt.WALK_SEEDS] and len(lt.WALK_SEEDS) >= 3
    for k in scripts:
        assert scripts[k] == again[k], k
    for seed in lt.WALK_SEEDS:
        ops = scripts['walk%d' % seed]
        run = _run(ops)
        n_ref = sum(1 for _, c, _ in run if c)
        slots = {s['slot'] for _, _, s in run}
        print('walk %d: %d ops, %d refused, slots %s, models %s' % (seed, len(ops), n_ref, sorted(slots), [o[1]['model'] for o, c, _ in run if o[0] == 'set_model']))
        assert len(ops) >= 80 and len(slots) >= 3
        assert len(ops) / 16 <= n_ref <= len(ops) / 4              # about one op in eight
    assert scripts['walk%d' % lt.WALK_SEEDS[0]] != scripts['walk%d' % lt.WALK_SEEDS[1]]


# sha256 of repr() of the scripts as they were before fit and cond_surfaces had ops (the first four) and before the baseline and
# sandwich calls had (the two walks of NEW_WALK_SEEDS)
PINNED = {'hand': 'f33bfc16a490813785aa3927fc6cc387ee04f80682c52f20e7806a109c0f63c7',
          'walk20261101': '89d6ccf692b7ebab8e06591903fd5c02c22f2d2a57b0621a99922e8b96676454',
          'walk20261102': 'a98854200f3b9b65f1d4f24ba3d7086c74e6e0a2e1ac0978372af43635988381',
          'walk20261103': '09faa44244ca0223ca72b558b998e689d136af8628bb864ad61c123b5d77e497',
          'walk20261105': '3c32ffe2cdea1e8e878b8519ba1c4cd8f9004c73f6faccdc7610f9a82f8cf0e1',
          'walk20261110': 'a96bb2dba287d9d59ba463287f03ece692e04e893baa923b9468bb791910c1f7'}
DROPPERS = ('set_sites', 'resample_sites', 'plant_sites', 'set_model')      # the four calls that drop a baseline


def _tail(ops):
    """Index of the hand-written script's last segment: its set_model of the 729-row table."""
    return ops.index(op('set_model', model=lt.HAND_TAIL))


def _drops(run):
    """The successful droppers of a run that met a baseline with at least one locus (set_model: in any slot)."""
    out = []
    for i, (o, c, s) in enumerate(run):
        if i and c == 0 and o[0] in DROPPERS:
            held = run[i - 1][2]['bl_of']
            if any(held.values()) if o[0] == 'set_model' else held.get(s['slot']):
                out.append(i)
    return out


def test_the_earlier_scripts_are_what_they_were(scripts):
    """The five earlier walks op for op; the hand-written script keeps its earlier ops in order: the new ones are inserted and
    the segment on the 729-row table stands behind all of them."""
    assert set(PINNED) == {'hand'} | {'walk%d' % s for s in lt.OLD_WALK_SEEDS + lt.NEW_WALK_SEEDS}
    for k, want in PINNED.items():
        ops = scripts[k]
        if k == 'hand':
            assert sum(o[0] in lt.NEW_OPS for o in ops) >= 30 and sum(o[0] in lt.LIST_OPS for o in ops) >= 60
            cut = _tail(ops)
            assert not any(o[1].get('model') == lt.HAND_TAIL for o in ops[:cut]) and cut > max(i for i, o in enumerate(ops) if o[1].get('model') == 'w4')
            ops = [o for o in ops[:cut] if o[0] not in lt.NEW_OPS + lt.LIST_OPS]
        else:
            assert not any(o[0] in lt.LIST_OPS for o in ops)
            assert any(o[0] in lt.NEW_OPS for o in ops) == (k in ['walk%d' % s for s in lt.NEW_WALK_SEEDS])
        assert hashlib.sha256(repr(ops).encode()).hexdigest() == want, k
    for seed in lt.NEW_WALK_SEEDS:                      # the new walks draw both new ops, succeeding
        done = collections.Counter(o[0] for o, c, _ in _run(scripts['walk%d' % seed]) if c == 0)
        assert all(done[n] >= 2 for n in lt.NEW_OPS), (seed, done)
    drops = 0
    for seed in lt.LIST_WALK_SEEDS:                     # the newest draw the six baseline and sandwich ops, succeeding, on the 729-row table too
        run = _run(scripts['walk%d' % seed])
        done = collections.Counter(o[0] for o, c, _ in run if c == 0)
        assert all(done[n] >= 2 for n in lt.LIST_OPS), (seed, done)
        assert lt.HAND_TAIL in lt.LIST_WALK_MODELS[lt.LIST_WALK_SEEDS.index(seed)]
        drops += len(_drops(run))
    assert drops >= 1                                   # ... and a call that drops a baseline meets one that holds a locus


def test_worlds():
    facts = {}
    assert set(lt.MODEL_SPECS) == set(lt.SCAN_WORLDS) | {lt.HAND_TAIL}
    for name in lt.MODEL_SPECS:
        w = lt.world(name)
        pairs = w.nx * w.nab
        facts[name] = (pairs, -(-pairs // 64), w.nA, w.model.rows, 4 if w.model.rows > 65535 else 2)
        lens = [len(w.chroms[c][0]) for c in 'SML']
        if name in lt.SCAN_WORLDS:
            assert lens[1] >= 3 * lens[0] and lens[2] >= 3 * lens[0] - 100 and lens[2] >= 2.9 * lens[1], lens
        else:                                           # offgrid's wide729: its 1 500 sites and their first 500
            assert lens == [500, 1500, 1500] and facts[name] == (9, 1, 2, 729, 2)
        for c in 'SML':
            gen, rows = w.chroms[c]
            assert np.all(np.diff(gen) >= 0) and (np.diff(gen) == 0).sum() >= 1 and rows.min() >= 0 and rows.max() < w.model.rows
            assert np.all(np.isfinite(w.model.g[rows])) and np.all(w.model.g[rows] > 0)
    assert facts['g3x3'] == (9, 1, 4, 21, 2) and facts['g17x61'][:3] == (1037, 17, 3) and facts['g1'][:3] == (1, 1, 1)
    assert facts['l2'][3] == 483 and facts['w4'][3:] == (90831, 4)
    # the hand-written order: pairs, slices, A values and row width each go up and down
    for q in (0, 1, 2, 4):
        d = np.sign(np.diff([facts[m][q] for m in lt.HAND_MODELS]))
        assert (d > 0).any() and (d < 0).any(), q
    # the three plans' test sites at every length
    for N in (700, 4003, 12009):
        assert [len(lt.test_index(N, s)) for s in lt.STRIDES] == [613, -(-N // 5), -(-N // 20)]


def test_required_transitions(scripts):
    run = _run(scripts['hand'])
    names = [o[0] for o, _, _ in run]
    # 1. long -> short -> medium in one slot, M large -> small -> larger
    per = collections.defaultdict(list)
    for i, (o, c, s) in enumerate(run):
        if o[0] == 'set_sites' and c == 0:
            j = _find(run, i + 1, lambda o2, c2, s2: s2['slot'] == s['slot'] and o2[0] in ('set_tests', 'set_sites', 'set_model') and c2 == 0)
            if j >= 0 and run[j][0][0] == 'set_tests':
                per[s['slot']].append((s['N'], run[j][2]['M']))
    assert any(a[0] >= 3 * b[0] and c[0] >= 3 * b[0] and c[0] < a[0] and a[1] > b[1] < c[1]
               for v in per.values() for a, b, c in zip(v, v[1:], v[2:])), per
    # 2. every model, and no slot keeps its sites across set_model
    models = [o[1]['model'] for o, c, _ in run if o[0] == 'set_model' and c == 0]
    assert tuple(models) == lt.HAND_MODELS + (lt.HAND_TAIL,)
    for i, (o, c, s) in enumerate(run):
        if o[0] == 'set_model' and c == 0 and s['model'] != models[0] or (o[0] == 'set_model' and c == 0 and run[i - 1][2]['model'] is not None):
            assert len(run[i - 1][2]['with_sites']) >= 2 and s['with_sites'] == []
    i4 = names.index('set_model', [k for k, (o, c, _) in enumerate(run) if o[1].get('model') == 'w4'][0])
    assert _find(run, 0, ok('scan')) < i4 < _find(run, i4, lambda o, c, s: o[0] == 'scan' and c == 0 and s['model'] == 'g3x3')
    # 3. one set of test sites under profiles 0 -> 7 -> 1 -> 0 and variants 0 -> 12 -> 0
    by_tests = collections.defaultdict(list)
    for o, c, s in run:
        if o[0] == 'scan' and c == 0:
            by_tests[s['tests']].append((s['profiles'], s['variant']))

    def subseq(seq, want):
        it = iter(seq)
        return all(any(x == w for x in it) for w in want)
    assert any(subseq([p for p, _ in v], [0, 7, 1, 0]) and subseq([q for _, q in v], [0, 12, 0]) for v in by_tests.values())
    # 4. permute -> scan -> resample and plant from the permuted source -> restore -> scan
    i = _find(run, 0, ok('permute_rows'))
    src = run[i][2]['slot']
    j = _find(run, i, ok('scan'))
    r = _find(run, j, lambda o, c, s: ok('resample_sites', src=src)(o, c, s) and s['perm_of'][src] is not None)
    p = _find(run, j, lambda o, c, s: ok('plant_sites', src=src)(o, c, s) and s['perm_of'][src] is not None)
    k = _find(run, max(r, p), lambda o, c, s: ok('restore_rows')(o, c, s) and s['slot'] == src)
    assert 0 <= i < j < min(r, p) and max(r, p) < k and run[_find(run, k, ok('scan'))][2]['slot'] == src
    assert run[r][2]['slot'] != src and run[p][2]['slot'] not in (src, run[r][2]['slot'])
    # 5. two null runs, the second with fewer replicates, then set_tests and a third
    runs = [(i, s['slot'], s['null_reps']) for i, (o, c, s) in enumerate(run) if o[0] == 'null_fetch' and c == 0]
    assert len(runs) >= 3 and runs[0][1] == runs[1][1] == runs[2][1] and runs[0][2] > runs[1][2] >= 1 and runs[2][2] >= 1
    assert _find(run, runs[1][0], lambda o, c, s: ok('set_tests')(o, c, s) and s['slot'] == runs[0][1]) < runs[2][0]
    assert _find(run, runs[0][0], ok('null_begin')) < runs[1][0]
    # 6. a full K x R locate run, then a smaller one with a replicate that is never accumulated
    fl = [s['lc'] for o, c, s in run if o[0] == 'fetch_locate' and c == 0]
    assert len(fl) >= 2 and fl[0][2] == list(range(fl[0][1])) and fl[1][0] < fl[0][0] and fl[1][1] < fl[0][1]
    assert 0 < len(fl[1][2]) < fl[1][1]
    # 7. refine -> scan on permuted rows -> support, boot refuse; fetch_refined answers -> refine -> support -> boot
    assert _chain(run, [ok('refine'), ok('permute_rows'), ok('scan'), refused('support', STATE), refused('boot', STATE), ok('fetch_refined'),
                        refused('fetch_support', STATE), ok('refine'), ok('support'), ok('boot'), ok('fetch_boot')])
    # 8. peaks -> at peaks -> scan -> refine refuses; a track of another length does not count; peaks -> refine
    i = _find(run, 0, ok('peaks_track'))
    assert run[i][0][1]['n'] != run[i][2]['M'] > 0
    assert _chain(run, [ok('peaks'), ok('refine_at_peaks', on=True), ok('scan'), refused('refine', INVALID), ok('peaks_track'),
                        refused('refine', INVALID), ok('peaks'), ok('refine')])
    # 9. surfaces and influence: 40 windows, then 1, then again after every change of the model's shape
    assert _chain(run, [ok('surfaces', kind=40), ok('surfaces', kind=1)]) and _chain(run, [ok('influence', kind=40), ok('influence', kind=1)])
    segments = [i for i, (o, c, _) in enumerate(run) if o[0] == 'set_model' and c == 0] + [len(run)]     # every segment between two set_model
    cuts = segments[:-1]                                                                                  # ... but the last, on the 729-row table
    assert run[cuts[-1]][0][1]['model'] == lt.HAND_TAIL
    for a, b in zip(cuts[1:], cuts[2:]):
        part = run[a:b]
        assert _chain(part, [ok('surfaces', kind=40)]) and _chain(part, [ok('influence', kind=40), ok('influence', kind=1)]), a
    # 13. fit and cond_surfaces: 40 windows, then 1, again after every change of the model's shape, and directly after surfaces
    #     and influence calls with longer and shorter lists (the shared buffers grow and shrink)
    for name in lt.NEW_OPS:
        assert _chain(run, [ok(name, kind=40), ok(name, kind=1)]) and _chain(run, [ok(name, kind=1), ok(name, kind=40)]), name
        for a, b in zip(cuts[1:], cuts[2:]):
            assert _chain(run[a:b], [ok(name, kind=40), ok(name, kind=1)]), (name, a)
        after = {(run[i - 1][0][0], run[i - 1][0][1]['kind'], o[1]['kind']) for i, (o, c, s) in enumerate(run)
                 if o[0] == name and c == 0 and run[i - 1][1] == 0 and run[i - 1][0][0] in ('surfaces', 'influence')}
        assert {p for p, _, _ in after} == {'surfaces', 'influence'}, (name, after)
        assert any(k0 > k1 for _, k0, k1 in after) and any(k0 < k1 for _, k0, k1 in after), (name, after)
    assert {o[1]['want_T'] for o, c, _ in run if o[0] == 'cond_surfaces' and c == 0} == {True, False}
    assert {(o[1]['F'], o[1]['D']) for o, c, _ in run if o[0] == 'fit' and c == 0} == set(lt.FIT_SHAPES)
    assert {o[1].get('bad', 'F') for o, c, _ in run if o[0] == 'fit' and c == INVALID} == set(lt.FIT_BAD)
    held = lambda name, n=1, **want: (lambda o, c, s: ok(name, **want)(o, c, s) and (s['bl'] or 0) >= n)
    # 14. the plain baseline chain, again in every segment between two set_model (the last included); want_T takes both values
    chain14 = [ok('baseline_reset'), held('baseline_add', 1), held('baseline_add', 2), held('base_surfaces', 2, kind=40), held('base_surfaces', 2, kind=1),
               held('baseline_fetch', 2), ok('baseline_reset'), lambda o, c, s: ok('baseline_fetch')(o, c, s) and s['bl'] == 0]
    for a, b in zip(segments, segments[1:]):
        assert _chain(run[a:b], chain14), a
    assert {o[1]['want_T'] for o, c, _ in run if o[0] == 'base_surfaces' and c == 0} == {True, False}
    # 15. the four droppers meet a baseline with a locus in the selected slot: add, fetch and base_surfaces are BMX_E_STATE, then a
    #     reset and a compared base_surfaces; the source of the resample and of the plant keeps its own, fetched afterwards
    met = set()
    for i in _drops(run):
        o, c, s = run[i]
        slot = s['slot']
        if not run[i - 1][2]['bl_of'].get(slot):
            continue
        here = lambda p: (lambda o2, c2, s2: p(o2, c2, s2) and s2['slot'] == slot)
        jr = _find(run, i + 1, here(ok('baseline_reset')))
        js = [_find(run, i + 1, here(lambda o2, c2, s2, n=n: o2[0] == n)) for n in ('baseline_add', 'baseline_fetch', 'base_surfaces')]
        if jr < 0 or min(js) < 0 or max(js) > jr:
            continue
        assert all(run[j][1] == STATE for j in js), (i, o)
        assert _find(run, jr, here(lambda o2, c2, s2: ok('base_surfaces')(o2, c2, s2) and s2['compared'])) > jr, (i, o)
        if o[0] in ('resample_sites', 'plant_sites'):
            src, n = o[1]['src'], run[i - 1][2]['bl_of'][o[1]['src']]
            jf = _find(run, i + 1, lambda o2, c2, s2: ok('baseline_fetch')(o2, c2, s2) and s2['slot'] == src)
            assert n >= 1 and jf > i and run[jf][2]['bl'] == n, (i, o)
            assert not any(o2[0] in ('baseline_reset', 'baseline_add') and s2['slot'] == src for o2, _, s2 in run[i:jf]), (i, o)
        met.add(o[0])
    assert met == set(DROPPERS), met
    # 16. the non-droppers: set_tests to another stride and ragged windows under a baseline of two loci or more, then a compared
    #     base_surfaces and an add on the new test sites; scans, set_variant, set_profiles; the rows permuted and restored
    assert any(ok('set_tests')(o, c, s) and (s['bl'] or 0) >= 2 and s['windows'] == 'ragged' and run[i - 1][2]['slot'] == s['slot']
               and run[i - 1][2]['stride'] not in (None, s['stride']) and ok('base_surfaces')(*run[i + 1]) and run[i + 1][2]['compared']
               and ok('baseline_add')(*run[i + 2]) for i, (o, c, s) in enumerate(run[:-2]) if i)
    assert _chain(run, [held('baseline_add', 2), held('set_profiles', 2), held('scan', 2), held('set_variant', 2), held('base_surfaces', 2)])
    perm = lambda name, on: (lambda o, c, s: held(name, 2)(o, c, s) and (s['perm'] is not None) == on)
    assert _chain(run, [perm('permute_rows', True), perm('base_surfaces', True), perm('baseline_add', True), perm('restore_rows', False),
                        perm('base_surfaces', False), perm('baseline_fetch', False)])
    # 17. one slot's baseline at N long -> short -> medium, each fetched; two slots with baselines of different N at once: away, the
    #     other slot's baseline used, back, then a compared baseline_fetch and base_surfaces
    fetched = collections.defaultdict(list)
    for i, (o, c, s) in enumerate(run):
        if ok('baseline_reset')(o, c, s):
            j = _find(run, i + 1, lambda o2, c2, s2: s2['slot'] == s['slot'] and o2[0] in ('baseline_fetch', 'set_sites', 'set_model'))
            if j >= 0 and ok('baseline_fetch')(*run[j]) and (not fetched[s['slot']] or fetched[s['slot']][-1] != s['N']):
                fetched[s['slot']].append(s['N'])
    assert any(a >= 3 * b and c >= 3 * b and c < a for v in fetched.values() for a, b, c in zip(v, v[1:], v[2:])), fetched
    hit = False
    for i, (o, c, s) in enumerate(run):
        if ok('select_slot')(o, c, s) and s['bl']:
            other = [k for k, n in s['bl_of'].items() if n and k != s['slot'] and s['N_of'][k] != s['N']]
            left = max((j for j in range(i) if run[j][2]['slot'] == s['slot']), default=-1)
            used = any(lt.GROUP_OF[o2[0]] == 'baseline' and c2 == 0 and s2['slot'] in other for o2, c2, s2 in run[left + 1:i])
            e = _find(run, i + 1, lambda o2, c2, s2: o2[0] == 'select_slot')
            part = run[i + 1:e if e >= 0 else len(run)]
            hit |= bool(other) and used and _chain(part, [ok('baseline_fetch')]) and _chain(part, [ok('base_surfaces')])
    assert hit
    # 18. base_surfaces directly after surfaces, influence, fit and cond_surfaces calls with a longer and with a shorter list
    after = {(run[i - 1][0][0], run[i - 1][0][1]['kind'], o[1]['kind']) for i, (o, c, s) in enumerate(run)
             if o[0] == 'base_surfaces' and c == 0 and i and run[i - 1][1] == 0 and run[i - 1][0][0] in ('surfaces', 'influence', 'fit', 'cond_surfaces')}
    assert {p for p, _, _ in after} == {'surfaces', 'influence', 'fit', 'cond_surfaces'}, after
    assert any(k0 > k1 for _, k0, k1 in after) and any(k0 < k1 for _, k0, k1 in after), after
    # 19. the plain sandwich chain with all four blocks, in every segment: on w4 (slab, 4-byte rows), on the 729-row table and in LDS
    for a, b in zip(segments, segments[1:]):
        part = run[a:b]
        assert _chain(part, [ok('sandwich', kind=40), ok('sandwich', kind=1), ok('sandwich', kind=1), ok('sandwich', kind=40)]), a
        assert {o[1]['block'] for o, c, _ in part if o[0] == 'sandwich' and c == 0} == set(lt.SANDWICH_BLOCKS), a
    # 20. sandwich between the compass calls, on a model in LDS and on the 729-row table (there also between two eval_points)
    chain20 = [ok('refine'), ok('sandwich'), ok('fetch_refined'), ok('support'), ok('sandwich'), ok('fetch_support'), ok('boot'), ok('sandwich'),
               ok('fetch_boot')]
    assert _chain(run[segments[0]:segments[1]], chain20) and lt.ws_in_lds(lt.world(lt.HAND_MODELS[0]))
    assert _chain(run[segments[-2]:], chain20 + [ok('eval_points'), ok('sandwich'), ok('eval_points')]) and not lt.ws_in_lds(lt.world(lt.HAND_TAIL))
    # 21. sandwich on permuted rows, then the same call on the restored ones; refine_R before and after a set_model that changes the rows
    hit = 0
    for i, (o, c, s) in enumerate(run):
        if ok('sandwich')(o, c, s) and s['perm'] is not None:
            j = _find(run, i + 1, lambda o2, c2, s2: s2['slot'] == s['slot'] and o2[0] in ('sandwich', 'set_tests', 'set_sites', 'set_model') and c2 == 0)
            hit += j > i and run[j][0] == o and run[j][2]['perm'] is None and run[j][2]['tests'] == s['tests']
    assert hit >= 2
    rows_of = lambda m: lt.world(m).model.rows
    crossed = 0
    for i in segments[1:-1]:
        b = max((j for j in range(i) if run[j][0][0] == 'refine_R'), default=-1)
        a = _find(run, i, lambda o2, c2, s2: o2[0] == 'refine_R')
        crossed += b >= 0 and a > i and run[b][1] == run[a][1] == 0 and rows_of(run[b][2]['model']) != rows_of(run[a][2]['model'])
    assert crossed >= 4                                                     # 21 -> 483 -> 90 831 -> 21 -> 729
    # 22. (a refused baseline op and a refused sandwich op directly before a compared op of their group: 12. below, for all groups)
    assert {(o[1]['test'], o[1]['lin']) for o, c, _ in run if o[0] == 'baseline_add' and c == INVALID} >= {('M', 0), (0, 'top')}
    bad_sw = {'block' if o[1]['block'] == 0 else 'hx' if o[1].get('hx') == 0.0 else o[1]['bad'] for o, c, _ in run if o[0] == 'sandwich' and c == INVALID}
    assert bad_sw == set(lt.SANDWICH_BAD)
    # 10. scan_write on a small M, on a larger M in another slot, a plain scan of the first
    i = _find(run, 0, ok('scan_write'))
    j = _find(run, i + 1, ok('scan_write'))
    k = _find(run, j + 1, lambda o, c, s: ok('scan')(o, c, s) and s['slot'] == run[i][2]['slot'])
    assert run[j][2]['slot'] != run[i][2]['slot'] and run[j][2]['M'] > run[i][2]['M'] and run[k][2]['tests'] == run[i][2]['tests']
    assert {o[1]['chunk'] for o, c, _ in run if o[0] == 'scan_write' and c == 0} == set(lt.CHUNKS)
    # 11. pack_records after one of three slots has lost its results to set_tests
    hit = False
    for i, (o, c, s) in enumerate(run):
        if o[0] == 'set_tests' and c == 0 and i and len(run[i - 1][2]['with_results']) >= 3 and s['slot'] in run[i - 1][2]['with_results']:
            j = _find(run, i + 1, lambda o2, c2, s2: o2[0] in ('pack_records', 'scan') and c2 == 0)
            hit |= j >= 0 and run[j][0][0] == 'pack_records' and len(run[j][2]['with_results']) == len(run[i - 1][2]['with_results']) - 1
    assert hit
    # 12. a refused call directly before a compared op of the same group, in every group that can refuse
    seen = set()
    for ops in scripts.values():
        r = _run(ops)
        for (o1, c1, s1), (o2, c2, s2), (o3, c3, s3) in zip(r, r[1:], r[2:]):
            if c1 and s2['compared'] and lt.GROUP_OF[o1[0]] == lt.GROUP_OF[o2[0]] and (s1['slot'] == s2['slot'] or o2[0] == 'select_slot'):
                seen.add(lt.GROUP_OF[o1[0]])
            # a scan takes no argument, so what refuses one refuses the next: one switch (set_profiles) lies between the two
            if c1 and o1[0] in ('scan', 'scan_write') and o2[0] == 'set_profiles' and o3[0] == o1[0] and s3['compared'] and s1['slot'] == s3['slot']:
                seen.add(o1[0])
    assert seen >= set(lt.GROUPS) - {'set_variant'}, set(lt.GROUPS) - seen         # set_variant refuses nothing but a NULL context


def test_every_group_before_every_other_and_compared(scripts):
    have, compared, codes, per_op = set(), collections.Counter(), collections.Counter(), collections.Counter()
    for ops in scripts.values():
        seen = set()
        for o, c, s in _run(ops):
            g = lt.GROUP_OF[o[0]]
            have |= {(x, g) for x in seen}
            seen.add(g)
            codes[c] += 1
            if s['compared']:
                compared[g] += 1
                per_op[o[0]] += 1
    missing = [(x, y) for x in lt.GROUPS for y in lt.GROUPS if x != y and (x, y) not in have]
    print('compared per group:', dict(compared))
    print('compared per op:', dict(per_op))
    print('codes:', {lt.CODE_NAMES[c]: n for c, n in codes.items()})
    assert not missing, missing
    assert all(compared[g] >= 5 for g in lt.GROUPS), compared
    assert all(codes[c] >= 1 for c in (INVALID, LIMIT, STATE))
    # every op of every group is in some script, succeeding and (where it can be) refused
    used = {(o[0], c == 0) for ops in scripts.values() for o, c, _ in _run(ops)}
    assert {n for n, good in used if good} == set(lt.GROUP_OF)
    cannot_refuse = {'set_variant', 'refine_at_peaks'}          # (a NULL context apart)
    assert {n for n, good in used if not good} >= set(lt.GROUP_OF) - cannot_refuse


def test_both_homes_of_the_fit_sums_are_reached(scripts):
    """On w4 (221 sample sizes) F = 7 and F = 10 keep the prologue sums in the workspace in device memory; every other model and
    F = 1 keep them in LDS."""
    homes = collections.Counter()
    for k, ops in scripts.items():
        for o, c, s in _run(ops):
            if o[0] == 'fit' and c == 0:
                homes[(k == 'hand', lt.fit_in_lds(lt.world(s['model']), o[1]['F']))] += 1
    print('successful fit ops by (hand-written script, sums in LDS):', dict(homes))
    assert all(homes[(h, l)] >= 1 for h in (True, False) for l in (True, False)), homes
    w4 = lt.world('w4')
    assert [lt.fit_in_lds(w4, F) for F, _ in lt.FIT_SHAPES] == [True, False, False] and len(w4.model.sizes) == 221
    assert all(lt.fit_in_lds(lt.world(m), F) for m in lt.MODEL_SPECS if m != 'w4' for F, _ in lt.FIT_SHAPES)
    assert all(F * D <= 256 for F, D in lt.FIT_SHAPES)
    # the lists: one entry without a grid point, every fourth without a conditioning site, one without a conditioning grid point
    for kind in lt.LISTS:
        t = lt.index_list(kind, 613)
        lins = lt.fit_lins(kind, 36)
        ct, cl = lt.cond_lists(t, 613, 36)
        assert len(lins) == len(ct) == len(cl) == kind and lins.max() < 36 and cl.max() < 36 and ct.max() < 613 and ct.min() >= -1
        assert (lins < 0).sum() == (kind >= 3) and (cl < 0).sum() == (kind >= 3) and (ct < 0).sum() == kind // 4
        assert np.array_equal(ct[ct >= 0], ((t.astype(np.int64) + 3) % 613)[ct >= 0])


def test_both_homes_of_the_sandwich_workspace_and_both_block_paths_are_reached(scripts):
    """sandwich_kernel works in refine_workspace's workspace: in LDS up to 728 table rows, in c->rf_slab beyond (l2's 483 rows are
    in LDS, the 729 of w729 and the 90 831 of w4 in the slab); a block below SANDWICH_WAVE_BLOCK sites is one thread's, a larger
    one a wave's.  On w729 the compass kernels (refine, support, boot, eval_points) run in the same slab between the sandwich calls."""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'ballermixplus_amd', 'csrc', 'bmxscan.hip')) as f:
        src = f.read()
    for pat in (r'const int64_t ws = \(\(int64_t\)c->rows \* \(REFINE_TABS \* 8 \+ 4 \+ 1\) \+ 15\) / 16 \* 16;', r'constexpr int REFINE_TABS = 5;',
                r'constexpr int64_t REFINE_LDS_WS = 32 \* 1024;', r'P\.ws_lds = ws <= REFINE_LDS_WS;', r'constexpr int64_t SANDWICH_WAVE_BLOCK = 64;',
                r'if \(B < SANDWICH_WAVE_BLOCK\) \{', r'int lrc = launch_ws\(c, sandwich_kernel, Q, Q\.P, m\);'):
        assert re.search(pat, src), pat
    assert lt.refine_ws(728) == 32768 == lt.REFINE_LDS_WS and lt.refine_ws(729) == 32816 and lt.SANDWICH_WAVE_BLOCK == 64
    assert {m: lt.ws_in_lds(lt.world(m)) for m in lt.MODEL_SPECS} == {'g3x3': True, 'g17x61': True, 'g1': True, 'l2': True, 'w4': False, 'w729': False}
    assert [b >= lt.SANDWICH_WAVE_BLOCK for b in lt.SANDWICH_BLOCKS] == [False, False, True, True]
    seen, beside = collections.Counter(), collections.Counter()
    for k, ops in scripts.items():
        run = _run(ops)
        for i, (o, c, s) in enumerate(run):
            if o[0] == 'sandwich' and c == 0:
                lds = lt.ws_in_lds(lt.world(s['model']))
                seen[(k == 'hand', lds, o[1]['block'] >= lt.SANDWICH_WAVE_BLOCK)] += 1
                near = {run[j][0][0] for j in (i - 1, i + 1) if 0 <= j < len(run) and run[j][1] == 0}
                if not lds and near & {'refine', 'support', 'boot', 'eval_points', 'eval_points_weighted'}:
                    beside[k == 'hand'] += 1
    print('successful sandwich ops by (hand-written script, workspace in LDS, a wave per block):', dict(seen))
    print('... of them directly beside a compass launch in the slab:', dict(beside))
    assert all(seen[(h, l, wv)] >= 1 for h in (True, False) for l in (True, False) for wv in (True, False)), seen
    assert beside[True] >= 4
    # the points: x +- HX inside (0, 1) for every world and list; on g1 every point is the grid point
    from ballermixplus_amd import sandwich
    for m in lt.MODEL_SPECS:
        w = lt.world(m)
        for kind in lt.LISTS:
            A, x, ab = lt.sandwich_points(w, kind)
            assert len(A) == len(x) == len(ab) == kind and np.all(x - sandwich.HX > 0.0) and np.all(x + sandwich.HX < 1.0)
            assert np.all(A >= min(w.As)) and np.all(A <= max(w.As)) and np.all(ab >= min(w.abetas)) and np.all(ab <= max(w.abetas))
            on_grid = np.isin(A, w.As) & np.isin(x, w.xs) & np.isin(ab, w.abetas)
            assert on_grid[0::2].all() and (on_grid.all() if m == 'g1' else kind < 2 or not on_grid[1::2].any())
    assert not sandwich.HX / 2 - sandwich.HX > 0.0                          # the bad x


def _replayed(bl, gen, given, R, w, zcut):
    """(d, cnt, written per locus) of a recorded baseline on the host: stepwise.host_baseline_add with each locus' window, grid
    point and the rows in force when it was added."""
    from ballermixplus_amd import stepwise
    d, cnt, written = np.zeros(len(gen)), np.zeros(len(gen), dtype=np.int32), []
    for l in bl:
        rows = given if l['perm'] is None else given[null.block_permutation(len(given), *l['perm'])]
        lin, npairs = l['lin'], w.nx * w.nab
        written.append(stepwise.host_baseline_add(d, cnt, gen, rows, R, l['tg'], 0 if l['lo'] is None else l['lo'], len(gen) - 1 if l['hi'] is None else l['hi'],
                                                  w.As[lin // npairs], (lin // w.nab) % w.nx, lin % w.nab, zcut))
    return d, cnt, written


def _mixture(bl, gen, given, R, w, zcut):
    """(d, scale, cnt) of a recorded baseline in closed form, the loci taken in REVERSE order: locus k reaches site i with linkage
    a_ik = exp(-A_k |g_i - t_k|) and the later loci leave it the weight rest_ik = prod_{j > k} (1 - a_ij), so
    d_i = sum_k a_ik R_k[row_ik] rest_ik (the nested mixture of ballermixplus_amd/stepwise.py written out); scale: the same sum of
    absolute terms.  Shares no statement with stepwise.host_baseline_add."""
    N = len(gen)
    d, scale, rest, cnt = np.zeros(N), np.zeros(N), np.ones(N), np.zeros(N, dtype=np.int32)
    at = np.arange(N)
    for l in reversed(bl):
        rows = given if l['perm'] is None else given[null.block_permutation(N, *l['perm'])]
        lin, npairs = l['lin'], w.nx * w.nab
        z = w.As[lin // npairs] * np.abs(gen - l['tg'])
        reach = (z <= zcut) & (gen != l['tg']) & (at >= (0 if l['lo'] is None else l['lo'])) & (at <= (N - 1 if l['hi'] is None else l['hi']))
        a = np.where(reach, np.exp(-z), 0.0)
        term = a * R[(lin // w.nab) % w.nx, lin % w.nab][rows] * rest
        d, scale, rest, cnt = d + np.where(reach, term, 0.0), scale + np.where(reach, np.abs(term), 0.0), rest * (1.0 - a), cnt + reach
    return d, scale, cnt


def test_the_recorded_baselines_replay_on_the_host(scripts):
    """Every baseline history a script records, in every world (the 21-, 483-, 729- and 90 831-row tables, each on the oracle's
    table of its own spectrum), rebuilt with stepwise.host_baseline_add from the loci and row states of the state model's record,
    and compared with the closed form of the nested mixture (_mixture: another order of operations, no shared statement) at 1e-12
    of the sum of absolute terms, the counts exactly.  In the hand-written script the counts reach 2, one baseline holds loci
    formed under two row states (and differs from the one the unpermuted rows would give), one locus writes nothing."""
    from util import oracle_R
    import offgrid as og
    tables = {}

    def table(m):
        w = lt.world(m)
        if m not in tables:
            tables[m] = oracle_R('B2', w.neutral[0], 1, w.neutral[1], w.neutral[2], w.xs, w.abetas)
        return tables[m]
    most, mixed, empty, replayed, worlds, worst = 0, 0, 0, collections.Counter(), set(), 0.0
    for k, ops in scripts.items():
        for o, c, st in lt.replay(ops, R_of=lambda m: None):
            s = st.slot
            if c or lt.GROUP_OF[o[0]] != 'baseline' or not s.bl:
                continue
            w, gen, given = st.w, s.sites['gen'], s.sites['given']
            d, cnt, written = _replayed(s.bl, gen, given, table(st.model), w, og.ZCUT)
            want, scale, reached = _mixture(s.bl, gen, given, table(st.model), w, og.ZCUT)
            replayed[k] += 1
            worlds.add(st.model)
            assert np.array_equal(cnt, reached) and cnt.sum() == sum(n for _, _, n in written) and not d[cnt == 0].any(), (k, o)
            assert all((a > b and n == 0) or (a <= b and 1 <= n <= b - a + 1 and cnt[a] and cnt[b]) for a, b, n in written), (k, o, written)
            err = np.abs(d - want)
            assert np.all(err <= 1e-12 * scale), (k, o, float(np.max(err[scale > 0] / scale[scale > 0])))
            worst = max(worst, float(np.max(err[scale > 0] / scale[scale > 0], initial=0.0)))
            if k != 'hand':
                continue
            most = max(most, int(cnt.max(initial=0)))
            empty += sum(n == 0 and a > b for a, b, n in written)
            if len({l['perm'] for l in s.bl}) >= 2:
                plain = _replayed([dict(l, perm=None) for l in s.bl], gen, given, table(st.model), w, og.ZCUT)[0]
                mixed += not np.array_equal(plain, d)
    print('baselines replayed per script %s in the worlds %s, worst %.1e of the sum of absolute terms; in the hand-written script the largest cnt is %d, '
          '%d empty loci are met and %d replayed baselines hold loci formed under two row states' % (dict(replayed), sorted(worlds), worst, most, empty, mixed))
    assert set(replayed) == set(scripts) - {'walk%d' % s for s in lt.OLD_WALK_SEEDS + lt.NEW_WALK_SEEDS} and worlds == set(lt.MODEL_SPECS)
    assert replayed['hand'] >= 60 and all(replayed['walk%d' % s] >= 5 for s in lt.LIST_WALK_SEEDS)
    assert most >= 2 and empty >= 1 and mixed >= 1


def test_the_listed_calls_stay_cheap_and_no_script_selects_the_anchor_slot(scripts):
    """COST_CAP's product, extended to base_surfaces and sandwich (list_cost: list length x window x pairs x A), holds for every
    such op of every script; on the 12 009-site chromosomes the hand-written script lists ragged windows or 1 and 3 windows only.
    lifetime.ANCHOR_SLOT, where the GPU module builds its base_surfaces anchor, belongs to no script."""
    n = 0
    for k, ops in scripts.items():
        assert not any(o[0] in ('select_slot', 'resample_sites', 'plant_sites') and lt.ANCHOR_SLOT in (o[1].get('slot'), o[1].get('src')) for o in ops), k
        for o, c, s in _run(ops):
            if c == 0 and o[0] in ('base_surfaces', 'sandwich'):
                n += 1
                assert lt.list_cost(lt.world(s['model']), s['N'], s['windows'], o[1]['kind']) <= lt.COST_CAP, (k, o)
                if k == 'hand' and s['N'] >= 12000:
                    assert s['windows'] == 'ragged' or o[1]['kind'] <= 3, o
    assert n >= 80 and 0 <= lt.ANCHOR_SLOT < lt.MAX_SLOTS


G3 = op('set_model', model='g3x3')
SITES, TESTS, SCAN = op('set_sites', chrom='S'), op('set_tests', stride=5, windows='all'), op('scan')
RESET, ADD = op('baseline_reset'), op('baseline_add', test=0, lin=0)
READY = [G3, SITES, TESTS]
BASED = READY + [RESET]
SCANNED = READY + [SCAN]
REFINED = SCANNED + [op('refine', min_clr=0.0)]
PK = dict(sep=1e-4, min_clr=0.0, frac=0.5)
# (history, op, the code include/bmxscan.h gives it) -- each row one sentence of the header
HEADER_ROWS = [
    ([], SITES, STATE),                                                   # "Call order: set_model, then set_sites, then set_tests"
    ([G3], TESTS, STATE),
    ([G3, SITES], SCAN, STATE),                                           # "call order violated (e.g. scan before model/sites were set)"
    (SCANNED + [op('set_model', model='g1')], SCAN, STATE),               # "a new model discards the site and test arrays of EVERY slot"
    (SCANNED + [op('select_slot', slot=1), op('set_model', model='g1'), op('select_slot', slot=0)], op('set_tests', stride=5, windows='all'), STATE),
    (SCANNED + [SITES], SCAN, STATE),                                     # "new sites discard the slot's test sites"
    (READY, op('select_slot', slot=4096), INVALID),                       # "0 <= slot < 4096"
    (READY, op('select_slot', slot=4095), 0),
    (READY + [op('set_variant', variant=12), op('set_profiles', which=7)], SCAN, LIMIT),   # "diagnostic variants ... BMX_E_LIMIT"
    (READY + [op('set_profiles', which=1), SCAN], op('fetch_profile', which=2), STATE),      # "when that scan ran without this profile"
    (READY + [op('set_profiles', which=3), SCAN, TESTS], op('fetch_profile', which=1), STATE),  # "set_tests ... drops them"
    (READY + [op('set_profiles', which=3), SCAN], op('fetch_profile', which=2), 0),
    ([G3], op('permute_rows', key=1, block=1), STATE),
    (READY, op('permute_rows', key=1, block=0), INVALID),                 # "block < 1: BMX_E_INVALID"
    (READY, op('null_begin'), STATE),                                     # "BMX_E_STATE before a scan"
    (SCANNED + [op('null_begin')], op('null_accumulate'), STATE),         # "when no scan was launched since null_begin"
    (SCANNED + [op('null_begin'), SCAN, op('null_accumulate')], op('null_accumulate'), STATE),      # "... / the previous accumulate"
    (SCANNED + [op('null_begin'), TESTS], op('null_fetch'), STATE),       # "set_tests (and so set_sites / set_model) drops this state"
    (READY, op('refine', min_clr=0.0), STATE),                            # "BMX_E_STATE before a scan"
    (REFINED + [SCAN], op('support', drop=1.0, min_clr=0.0), STATE),      # "bmx_ctx_refine after the last scan; else BMX_E_STATE"
    (REFINED + [SCAN], op('boot', key=1, R=2, block=1, min_clr=0.0), STATE),
    (REFINED + [SCAN], op('fetch_refined'), 0),                           # only "set_tests / set_sites / set_model drop the results"
    (REFINED + [TESTS], op('fetch_refined'), STATE),
    (REFINED, op('support', drop=float('inf'), min_clr=0.0), INVALID),    # "drop finite and > 0"
    (REFINED + [op('support', drop=1.0, min_clr=0.0), SCAN], op('fetch_support'), STATE),           # "A new scan ... drop the results"
    (REFINED + [op('support', drop=1.0, min_clr=0.0), op('refine', min_clr=0.0)], op('fetch_support'), STATE),    # "... refinement ..."
    (REFINED, op('boot', key=1, R=0, block=1, min_clr=0.0), INVALID),     # "R < 1, block < 1 or a NaN min_clr: BMX_E_INVALID"
    (REFINED + [op('boot', key=1, R=2, block=1, min_clr=0.0), SCAN], op('fetch_boot'), STATE),      # "A new scan ... drop the results"
    (READY, op('eval_points_weighted', key=1, block=0), INVALID),         # "block >= 1, else BMX_E_INVALID"
    ([G3, SITES], op('surfaces', kind=1), STATE),                         # "Needs model, sites and test sites (else BMX_E_STATE), no scan"
    (READY, op('surfaces', kind=3), 0),
    (READY, op('surfaces', kind=3, bad=True), INVALID),                   # "an index outside [0, M) ... is BMX_E_INVALID"
    ([G3], op('influence', kind=1, block=0), INVALID),                    # "block < 1 ... is BMX_E_INVALID and nothing is read"
    ([G3], op('influence', kind=1, block=5), STATE),
    ([G3, SITES], op('fit', kind=1, F=7, D=6), STATE),                    # "BMX_E_STATE without model, sites and test sites"
    (READY, op('fit', kind=3, F=7, D=6), 0),                              # no scan is needed
    (SCANNED, op('fit', kind=3, F=1, D=1), 0),
    ([G3], op('fit', kind=1, F=0, D=6), INVALID),                         # "F < 1 ... BMX_E_INVALID": the call's own argument comes first
    (READY, op('fit', kind=3, F=7, D=6, bad='lin'), INVALID),             # "lin >= nA * nx * nab"
    (READY, op('fit', kind=3, F=7, D=6, bad='gw'), INVALID),              # "a gw outside [0, 1]"
    ([G3], op('fit', kind=3, F=7, D=6, bad='gw'), STATE),                 # ... which is looked at after the state
    ([G3, SITES], op('cond_surfaces', kind=1, want_T=True), STATE),       # "BMX_E_STATE without model, sites and test sites"
    (READY, op('cond_surfaces', kind=3, want_T=False), 0),
    (READY, op('cond_surfaces', kind=3, want_T=True, bad=True), INVALID),                   # "a cond_test outside [-1, M)"
    ([G3], op('baseline_reset'), STATE),                                  # baseline_reset: "BMX_E_STATE without sites"
    ([G3, SITES], op('baseline_reset'), 0),                               # ... and needs no test sites
    ([G3, SITES, RESET], ADD, STATE),                                     # baseline_add: "BMX_E_STATE without model, sites and test sites;"
    (READY, ADD, STATE),                                                  # "BMX_E_STATE without a baseline;"
    (BASED, op('baseline_add', test='M', lin=0), INVALID),                # "BMX_E_INVALID test outside [0, M);"
    (BASED, op('baseline_add', test=0, lin='top'), INVALID),              # "BMX_E_INVALID lin outside [0, nA * nx * nab)"
    ([G3, SITES, RESET], op('baseline_add', test='M', lin='top'), STATE),  # ... "in this order": the state before the arguments
    (BASED, ADD, 0),
    (READY, op('baseline_fetch'), STATE),                                 # baseline_fetch: "BMX_E_STATE without a baseline"
    ([G3, SITES, RESET], op('baseline_fetch'), 0),
    ([G3, SITES, RESET], op('base_surfaces', kind=1, want_T=True), STATE),   # base_surfaces: "BMX_E_STATE without model, sites and test sites;"
    (READY, op('base_surfaces', kind=1, want_T=True), STATE),             # "BMX_E_STATE without a baseline;"
    (READY, op('base_surfaces', kind=3, want_T=True, bad=True), STATE),   # ... which comes before
    (BASED, op('base_surfaces', kind=3, want_T=True, bad=True), INVALID),  # "BMX_E_INVALID an index outside [0, M)"
    (BASED, op('base_surfaces', kind=3, want_T=False), 0),                # against the empty baseline too
    # "bmx_ctx_set_sites, _resample_sites and _plant_sites on a slot (and a new model) drop its baseline: the calls below are then
    # BMX_E_STATE until the next reset"
    (BASED + [ADD, SITES], op('baseline_fetch'), STATE),
    (BASED + [ADD, SITES, TESTS], ADD, STATE),
    (BASED + [ADD, SITES, TESTS], op('base_surfaces', kind=1, want_T=True), STATE),
    (BASED + [ADD, SITES, RESET], op('baseline_fetch'), 0),
    (BASED + [ADD, G3], op('baseline_fetch'), STATE),
    (BASED + [ADD, G3, SITES, TESTS], ADD, STATE),
    (BASED + [ADD, op('select_slot', slot=1), SITES, op('select_slot', slot=0), op('resample_sites', src=1, key=1, block=1)], op('baseline_fetch'), STATE),
    (BASED + [ADD, op('select_slot', slot=1), SITES, op('select_slot', slot=0), op('plant_sites', src=1, key=1, K=0, iA=0, ix=0, ia=0)],
     op('baseline_fetch'), STATE),
    (BASED + [ADD, op('select_slot', slot=1), op('resample_sites', src=0, key=1, block=1), op('select_slot', slot=0)], op('baseline_fetch'), 0),   # the source keeps its own
    # "A baseline survives bmx_ctx_set_tests, scans, bmx_ctx_permute_rows and bmx_ctx_restore_rows" (and select_slot, set_variant, set_profiles)
    (BASED + [ADD, TESTS], op('baseline_fetch'), 0),
    (BASED + [ADD, op('set_tests', stride=20, windows='ragged')], ADD, 0),
    (BASED + [ADD, SCAN], op('base_surfaces', kind=3, want_T=True), 0),
    (BASED + [ADD, op('permute_rows', key=1, block=3)], op('base_surfaces', kind=3, want_T=True), 0),
    (BASED + [ADD, op('permute_rows', key=1, block=3), op('restore_rows')], op('baseline_fetch'), 0),
    (BASED + [ADD, op('select_slot', slot=1), op('select_slot', slot=0), op('set_variant', variant=16), op('set_profiles', which=1)], op('baseline_fetch'), 0),
    (BASED + [op('select_slot', slot=1)], op('baseline_fetch'), STATE),   # "on the selected slot": another slot has none
    # sandwich: "n < 0, block and the steps are refused before the state is looked at"
    ([], op('sandwich', kind=1, block=0), INVALID),                       # "block < 1"
    ([G3], op('sandwich', kind=1, block=7, hx=0.0), INVALID),             # "hx or hv not finite and > 0"
    ([G3, SITES], op('sandwich', kind=1, block=7), STATE),                # "BMX_E_STATE without model, sites and test sites"
    ([G3, SITES], op('sandwich', kind=3, block=7, bad='index'), STATE),   # ... which comes before the list's entries
    (READY, op('sandwich', kind=3, block=7, bad='index'), INVALID),       # "an index outside [0, M)"
    (READY, op('sandwich', kind=3, block=7, bad='x'), INVALID),           # "x - hx <= 0"
    (READY, op('sandwich', kind=3, block=10 ** 6), 0),                    # "Needs no scan"
    (SCANNED, op('sandwich', kind=40, block=1), 0),
    ([G3, SITES], op('refine_R', x=0.3, abeta=7.0), STATE),               # refine_R: "without model, sites and test sites BMX_E_STATE"
    ([G3], op('refine_R', x=1.0, abeta=7.0), STATE),                      # (the state is looked at first, as in bmx_ctx_eval_points)
    (READY, op('refine_R', x=1.0, abeta=7.0), INVALID),                   # "x outside (0, 1) ... is BMX_E_INVALID"
    (READY, op('refine_R', x=0.3, abeta=7.0), 0),
    (READY, op('resample_sites', src=0, key=1, block=1), INVALID),        # "src_slot == the selected slot"
    (READY + [op('select_slot', slot=1)], op('resample_sites', src=2, key=1, block=1), STATE),      # "a source without sites"
    (READY + [op('select_slot', slot=1)], op('resample_sites', src=0, key=1, block=0), INVALID),
    (READY + [op('select_slot', slot=1), op('resample_sites', src=0, key=1, block=1)], SCAN, STATE),   # "its test sites are discarded"
    ([], op('locate_begin', K=1, step=1, width=1, R=1), 0),               # needs nothing: "this state outlives set_sites / ..."
    ([op('locate_begin', K=1, step=1, width=1, R=1), G3], op('fetch_locate'), STATE),               # "a new model ends it"
    ([G3, op('locate_begin', K=1, step=1, width=1, R=1), SITES, TESTS], op('fetch_locate'), 0),
    (SCANNED + [op('locate_begin', K=1, step=1, width=1, R=2)], op('locate_accumulate', r=0), STATE),   # "no scan since locate_begin"
    (SCANNED + [op('locate_begin', K=1, step=1, width=1, R=2), SCAN], op('locate_accumulate', r=2), INVALID),
    (SCANNED + [op('locate_begin', K=2, step=100, width=100, R=2), SCAN], op('locate_accumulate', r=0), INVALID),   # "a range reaches past"
    (READY + [op('select_slot', slot=1)], op('plant_sites', src=0, key=1, K=1, iA=4, ix=0, ia=0), INVALID),   # "indices outside the grids"
    ([op('select_slot', slot=1)], op('plant_sites', src=0, key=1, K=1, iA=0, ix=0, ia=0), STATE),             # "no model"
    (READY, op('fetch_at', kind=3), STATE),                               # "before a scan the call is BMX_E_STATE"
    (SCANNED, op('fetch_at', kind=3, bad=True), INVALID),
    (READY, op('peaks', **PK), INVALID),                                  # "no scan yet ... are all BMX_E_INVALID"
    (SCANNED, op('peaks', sep=-1.0, min_clr=0.0, frac=0.5), INVALID),
    ([], op('peaks_track', n=10, seed=0, **PK), 0),                       # "Needs neither model nor sites"
    ([], op('fetch_peaks'), STATE),                                       # "BMX_E_STATE without one"
    (SCANNED + [op('peaks', **PK), TESTS], op('fetch_peaks'), STATE),     # "set_tests / set_sites / set_model drop it"
    (SCANNED + [op('refine_at_peaks', on=True)], op('refine', min_clr=0.0), INVALID),               # "else the refinement fails with BMX_E_INVALID"
    (SCANNED + [op('refine_at_peaks', on=True), op('peaks', **PK), SCAN], op('refine', min_clr=0.0), INVALID),   # "on the slot's last scan"
    (SCANNED + [op('refine_at_peaks', on=True), op('peaks', **PK)], op('refine', min_clr=0.0), 0),
    (SCANNED + [op('refine_at_peaks', on=True), op('peaks_track', n=140, seed=0, **PK)], op('refine', min_clr=0.0), INVALID),   # "must be a bmx_ctx_peaks"
    (SCANNED, op('pack_records', short=True), INVALID),
    ([], op('pack_records', short=True), 0),                              # nothing to pack: room for 0 records is enough
]


@pytest.mark.parametrize('row', range(len(HEADER_ROWS)))
def test_state_model_agrees_with_the_header(row):
    history, o, want = HEADER_ROWS[row]
    st = lt.State(R_of=lambda m: None)
    for h in history:
        assert st.step(h) == 0, h
    before = (st.cur, st.model, st.slot.seq, st.slot.M, st.slot.sites is None)
    assert st.predict(o) == want, (o, lt.CODE_NAMES[want])
    assert (st.cur, st.model, st.slot.seq, st.slot.M, st.slot.sites is None) == before        # predict changes nothing
    assert st.step(o) == want
    if want:
        assert (st.cur, st.model, st.slot.seq, st.slot.M, st.slot.sites is None) == before    # nor does a refused call


def test_expected_site_arrays_are_the_host_restatements():
    """permute -> resample and plant from the permuted source -> restore, on the oracle's table."""
    from util import oracle_R
    w = lt.world('g3x3')
    spect, props = lt.gs.spectrum('small')
    R = oracle_R('B2', lt.gs.sizes_of('small'), 1, spect, props, w.xs, w.abetas)
    st = lt.State(R_of=lambda m: R)
    K1, K2, K3 = 0xABCDEF12345, 0x5555AAAA5555, 77
    gen, rows = w.chroms['M']
    for o in (G3, op('set_sites', chrom='M'), op('permute_rows', key=K1, block=7), op('select_slot', slot=1),
              op('resample_sites', src=0, key=K2, block=5), op('select_slot', slot=2),
              op('plant_sites', src=0, key=K3, K=3, iA=3, ix=1, ia=2)):
        assert st.step(o) == 0, o
    sigma = null.block_permutation(len(rows), K1, 7)
    assert sorted(sigma.tolist()) == list(range(len(rows))) and (sigma != np.arange(len(rows))).sum() > len(rows) // 2
    permuted = rows[sigma]
    assert np.array_equal(st.slots[0].rows_now(), permuted) and np.array_equal(st.slots[0].sites['given'], rows)
    wgt = boot.site_weights(K2, len(rows), 5)
    assert wgt.min() == 0 and wgt.max() >= 3
    assert np.array_equal(st.slots[1].sites['gen'], np.repeat(gen, wgt)) and np.array_equal(st.slots[1].sites['given'], np.repeat(permuted, wgt))
    A = w.As[3]
    centres = lt.plant_centres(gen, A, 3)
    assert len(centres) == 3 and np.all(A * np.diff(centres) > power.SPACING * power.ALPHA_CUT)
    want, margin = power.planted_rows(gen, permuted, w.model.sizes, w.model.row_off, R[1, 2], w.gw, A, centres, K3)
    assert np.array_equal(st.slots[2].sites['given'], want) and np.array_equal(st.slots[2].sites['gen'], gen)
    changed = int((want != permuted).sum())
    print('planted: %d sites in reach, %d rows changed, smallest margin %.2e' % (int(np.isfinite(margin).sum()), changed, float(margin.min())))
    assert changed >= 5 and margin.min() > power.MARGIN
    assert st.step(op('select_slot', slot=0)) == 0 and st.step(op('restore_rows')) == 0
    assert np.array_equal(st.slot.rows_now(), rows)
    # the derived slots keep what they were given
    assert np.array_equal(st.slots[1].sites['given'], np.repeat(permuted, wgt)) and np.array_equal(st.slots[2].sites['given'], want)
    # an identity permutation (one block) and the lists
    assert st.step(op('permute_rows', key=K1, block=len(rows))) == 0 and np.array_equal(st.slot.rows_now(), rows)
    for kind in lt.LISTS:
        for M in (35, 613):
            v = lt.index_list(kind, M)
            assert len(v) == kind and v.min() >= 0 and v.max() < M and (kind < 3 or len(set(v.tolist())) < kind)
