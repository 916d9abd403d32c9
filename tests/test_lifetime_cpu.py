"""tests/lifetime.py on the host: the scripts that tests/test_gpu_lifetime.py runs in one long-lived context are deterministic, hold
every transition they are meant to hold, run every op group before every other, compare every group at least five times and meet
every error code; the state model answers a table of rows restated from include/bmxscan.h as the header does; and the site arrays
it expects after permute, restore, resample and plant are what the package's host restatements give.  The scripts from before fit
and cond_surfaces had ops are pinned by their sha256, and the fit ops reach both homes of the prologue sums.  No GPU."""
import collections
import hashlib

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
            'perm_of': {k: v.perm for k, v in st.slots.items()}, 'compared': code == 0 and lt.is_compared(o, st)}))
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


# sha256 of repr() of the scripts as they were before fit and cond_surfaces had ops
PINNED = {'hand': 'f33bfc16a490813785aa3927fc6cc387ee04f80682c52f20e7806a109c0f63c7',
          'walk20261101': '89d6ccf692b7ebab8e06591903fd5c02c22f2d2a57b0621a99922e8b96676454',
          'walk20261102': 'a98854200f3b9b65f1d4f24ba3d7086c74e6e0a2e1ac0978372af43635988381',
          'walk20261103': '09faa44244ca0223ca72b558b998e689d136af8628bb864ad61c123b5d77e497'}


def test_the_earlier_scripts_are_what_they_were(scripts):
    """The three earlier walks op for op; the hand-written script keeps its earlier ops in order, the new ones are inserted."""
    assert set(PINNED) == {'hand'} | {'walk%d' % s for s in lt.OLD_WALK_SEEDS}
    for k, want in PINNED.items():
        ops = scripts[k]
        if k == 'hand':
            assert sum(o[0] in lt.NEW_OPS for o in ops) >= 30
            ops = [o for o in ops if o[0] not in lt.NEW_OPS]
        else:
            assert not any(o[0] in lt.NEW_OPS for o in ops)
        assert hashlib.sha256(repr(ops).encode()).hexdigest() == want, k
    for seed in lt.NEW_WALK_SEEDS:                      # the new walks draw both new ops, succeeding
        done = collections.Counter(o[0] for o, c, _ in _run(scripts['walk%d' % seed]) if c == 0)
        assert all(done[n] >= 2 for n in lt.NEW_OPS), (seed, done)


def test_worlds():
    facts = {}
    for name in lt.MODEL_SPECS:
        w = lt.world(name)
        pairs = w.nx * w.nab
        facts[name] = (pairs, -(-pairs // 64), w.nA, w.model.rows, 4 if w.model.rows > 65535 else 2)
        lens = [len(w.chroms[c][0]) for c in 'SML']
        assert lens[1] >= 3 * lens[0] and lens[2] >= 3 * lens[0] - 100 and lens[2] >= 2.9 * lens[1], lens
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
    assert tuple(models) == lt.HAND_MODELS
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
    cuts = [i for i, (o, c, _) in enumerate(run) if o[0] == 'set_model' and c == 0] + [len(run)]
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


G3 = op('set_model', model='g3x3')
SITES, TESTS, SCAN = op('set_sites', chrom='S'), op('set_tests', stride=5, windows='all'), op('scan')
READY = [G3, SITES, TESTS]
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
