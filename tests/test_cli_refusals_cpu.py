"""Every refusal of the command line's nine additions (--power, --locate, --peaks, --surfaces, --nullPerm, --profiles, --boot,
--refine, --support), message for message: the exact line cli.main prints, that it exits with status 1, opens no device and
writes no file.  The rows with two faults fix the precedence: which message wins inside a feature, and which feature speaks
first.  (The per-feature test_refusals tables of the other files ask for a word of the message; this one asks for all of it.)"""
import glob
import os

import pytest

from util import REFT

from ballermixplus_amd import cli

EX1 = os.path.join(REFT, 'Example1_fullSweep_200kya_DAF.txt')
SPECT = os.path.join(REFT, 'HC_CEU_Neut_DAF_spect_for_B2.txt')

O = ['-o', 'OUT']                   # OUT: a file name in the test's own directory
WS, FD = {'WORLD_SIZE': '2'}, {'BMX_FORCE_DIST': '1'}


def helper(f):
    return '%s scans the input; it cannot be combined with --getSpect / --getConfig.' % f


def ranks(f):
    return '%s runs in a single process; multi-rank launches are not supported.' % f


def common(ok, flag, no_o, in_name=None):
    """The four refusals every feature shares, on a command line `ok` that runs (it ends with -o OUT): helper-file mode, no -o,
    the two signs of a multi-rank launch; in_name: the feature whose name they are refused in, when it is not the flag's own."""
    f = in_name or flag
    return [(ok + ['--getSpect'], {}, helper(f)), (ok + ['--getConfig'], {}, helper(f)), (ok[:-2], {}, no_o),
            (ok, WS, ranks(f)), (ok, FD, ranks(f))]


def orphans(flags, parent):
    return [(fl.split() + O, {}, '%s needs %s.' % (fl.split()[0], parent)) for fl in flags]


PLANT = ['--plant', '1000,0.5,100']
POWER = ['--power', '4'] + PLANT + ['--powerThreshold', '5'] + O
POWER_W = ('--power needs the default window mode (no -w, no --fixWinSize): the replicates are scanned with every window '
           'holding all sites.')
POWER_PLANT = '--power needs --plant A,x,abeta: the grid point whose mixture the sites are drawn from.'
POWER_O = '--power needs -o: the power file is written next to the output.'
LOCATE = ['--locate', '8', '--peaks', '0.01'] + O
LOCATE_W = ('--locate needs the default window mode (no -w, no --fixWinSize): windows that count sites or nucleotides are '
            'not defined on a resampled site array.')
LOCATE_PEAKS = '--locate needs --peaks G: the intervals are drawn around the apexes of the peak call.'
LOCATE_O = '--locate needs -o: the locate file is written next to the output.'
LOCATE_R = '--locate takes a number of replicates >= 2 (0: off).'
PEAKS = ['--peaks', '0.01'] + O
PEAKS_O = '--peaks needs -o: the peak file is written next to the output.'
SURF = ['--surfaces', '--surfaceMin', '5'] + O
SURF_WHICH = ('--surfaces needs --peaks G (the surfaces of the apexes) or --surfaceMin C (of the windows with CLR >= C): '
              'the surface of every window of a chromosome is never what is meant.')
SURF_O = '--surfaces needs -o: the surfaces file is written next to the output.'
NULL = ['--nullPerm', '3'] + O
NULL_R = '--nullPerm takes a number of replicates >= 1 (0: off).'
NULL_O = '--nullPerm needs -o: the null and p-value files are written next to the output.'
PROF = ['--profiles', 'A'] + O
PROF_O = '--profiles needs -o: the profile files are written next to the output.'
BOOT = ['--boot', '4', '--refine'] + O
BOOT_R = '--boot takes a number of replicates >= 2 (0: off).'
BOOT_REFINE = '--boot needs --refine: the replicates start at the refined maxima.'
BOOT_O = '--boot needs -o: the bootstrap file is written next to the output.'
REFINE = ['--refine'] + O
REFINE_O = '--refine needs -o: the refined file is written next to the output.'
SUPPORT = ['--support', '--refine'] + O
SUPPORT_REFINE = '--support needs --refine: the intervals are drawn around the refined maxima.'

ROWS = (
    # ---------------------------------------------------------------------------------------------------------- --power
    orphans(['--plant 1000,0.5,100', '--plantEvery 1', '--powerSpan 1', '--powerSeed 3', '--powerBackground obs', '--powerBlock 2',
             '--powerThreshold 5', '--powerReps'], '--power')
    + common(POWER, '--power', POWER_O)
    + [(['--power', '1'] + POWER[2:], {}, '--power takes a number of replicates >= 2 (0: off).'),
       (['--power', '4', '--powerThreshold', '5'] + O, {}, POWER_PLANT),
       (['--power', '4'] + PLANT + O, {}, '--power needs --powerThreshold C[,C...] or --nullPerm (whose genome-wide thresholds it '
                                         'then uses).'),
       (POWER + ['-w', '50'], {}, POWER_W),
       (POWER + ['--fixWinSize', '-w', '5000'], {}, POWER_W),
       (POWER + ['--fixWinSize'], {}, POWER_W),
       # two faults in the feature
       (['--power', '4', '-w', '50'] + O, {}, POWER_PLANT),                                  # no --plant, a window mode
       (['--power', '4', '--powerBlock', '0', '--powerThreshold', '5'] + O, {}, '--powerBlock must be >= 1.'),   # a value, no --plant
       (POWER[:-2] + ['--getSpect', '-w', '50'], {}, helper('--power')),                     # helper mode, window mode, no -o
       (POWER[:-2] + ['-w', '50'], WS, POWER_W),                                             # window mode, no -o, multi-rank
       (POWER[:-2], WS, POWER_O)]                                                            # no -o, multi-rank
    # --------------------------------------------------------------------------------------------------------- --locate
    + orphans(['--locateSeed 3', '--locateBlock 3', '--locateSpan 0.1', '--locateLevel 0.9', '--locateMin 3', '--locateReps'],
              '--locate')
    + common(LOCATE, '--locate', LOCATE_O)
    + [(['--locate', '1'] + LOCATE[2:], {}, LOCATE_R),
       (['--locate', '8'] + O, {}, LOCATE_PEAKS),
       (LOCATE + ['-w', '50'], {}, LOCATE_W),
       (LOCATE + ['--fixWinSize', '-w', '5000'], {}, LOCATE_W),
       (LOCATE + ['--fixWinSize'], {}, LOCATE_W),
       # two faults in the feature
       (['--locate', '8'], {}, LOCATE_PEAKS),                                                # no --peaks, no -o
       (['--locate', '8', '--getSpect'], {}, helper('--locate')),                            # helper mode, no --peaks, no -o
       (['--locate', '8', '--locateLevel', '1', '-w', '50'], {}, '--locateLevel takes a number L with 0 < L < 1.'),
       (LOCATE[:-2] + ['-w', '50'], FD, LOCATE_W)]                                           # window mode, no -o, multi-rank
    # ---------------------------------------------------------------------------------------------------------- --peaks
    + orphans(['--peakMin 3', '--peakExtent 0.5', '--atPeaks'], '--peaks')
    + common(PEAKS, '--peaks', PEAKS_O)
    + [(['--peaks', '-1'] + O, {}, '--peaks takes a separation G >= 0 (in the units the scan measures distance in).'),
       (PEAKS + ['--atPeaks'], {}, '--atPeaks needs --refine: it restricts the refinement to the apexes.'),
       # two faults in the feature
       (['--peaks', '0.01', '--atPeaks'], {}, PEAKS_O),                                      # no -o, --atPeaks without --refine
       (PEAKS + ['--atPeaks'], WS, ranks('--peaks')),                                        # multi-rank, --atPeaks without --refine
       (['--peaks', '0.01', '--peakExtent', '0', '--getConfig'], {}, '--peakExtent takes a fraction F with 0 < F <= 1.')]
    # ------------------------------------------------------------------------------------------------------- --surfaces
    + orphans(['--surfaceMin 3', '--surfaceMax 4'], '--surfaces')
    + common(SURF, '--surfaces', SURF_O)
    + [(['--surfaces'] + O, {}, SURF_WHICH),
       (SURF + ['--surfaceMax', '0'], {}, '--surfaceMax takes a number of windows >= 1.'),
       # two faults in the feature
       (['--surfaces', '--getSpect'], {}, SURF_WHICH),                                       # no selection, helper mode, no -o
       (['--surfaces', '--surfaceMax', '0'], {}, '--surfaceMax takes a number of windows >= 1.'),   # a value, no selection, no -o
       (SURF[:-2], FD, SURF_O)]                                                              # no -o, multi-rank
    # -------------------------------------------------------------------------------------------------------- --nullPerm
    + common(NULL, '--nullPerm', NULL_O)
    + [(['--nullPerm', '-1'] + O, {}, NULL_R),
       (NULL + ['--nullBlock', '0'], {}, '--nullBlock must be >= 1.'),
       # two faults in the feature
       (['--nullPerm', '-1', '--nullBlock', '0'], {}, NULL_R),
       (['--nullPerm', '3', '--nullBlock', '0', '--getSpect'], {}, '--nullBlock must be >= 1.'),
       (['--nullPerm', '3', '--getConfig'], WS, helper('--nullPerm'))]
    # -------------------------------------------------------------------------------------------------------- --profiles
    + common(PROF, '--profiles', PROF_O)
    + [(['--profiles', ','] + O, {}, '--profiles takes a comma list of A, x, abeta.'),
       (['--profiles', 'A,z'] + O, {}, "--profiles: unknown profile 'z' (choose from A, x, abeta)."),
       # two faults in the feature
       (['--profiles', 'z', '--getSpect'], {}, "--profiles: unknown profile 'z' (choose from A, x, abeta)."),
       (['--profiles', 'A'], WS, PROF_O),
       (['--profiles', 'A', '--getSpect'], FD, helper('--profiles'))]
    # ------------------------------------------------------------------------------------------------------------ --boot
    + orphans(['--bootSeed 3', '--bootBlock 3', '--bootLevel 0.9', '--bootMin 3', '--bootReps'], '--boot')
    + common(BOOT, '--boot', BOOT_O)
    + [(['--boot', '1'] + BOOT[2:], {}, BOOT_R),
       (['--boot', '-3'] + BOOT[2:], {}, BOOT_R),
       (['--boot', '4'] + O, {}, BOOT_REFINE),
       (BOOT + ['--bootBlock', '0'], {}, '--bootBlock must be >= 1.'),
       (BOOT + ['--bootLevel', '0'], {}, '--bootLevel takes a number L with 0 < L < 1.'),
       (BOOT + ['--bootLevel', '1'], {}, '--bootLevel takes a number L with 0 < L < 1.'),
       (BOOT + ['--bootLevel', 'nan'], {}, '--bootLevel takes a number L with 0 < L < 1.'),
       (BOOT + ['--bootMin', 'nan'], {}, '--bootMin takes a number.'),
       # two faults in the feature
       (['--boot', '1'] + O, {}, BOOT_R),                                                    # too few replicates, no --refine
       (['--boot', '4', '--getSpect'], {}, helper('--boot')),                                # helper mode, no --refine, no -o
       (['--boot', '4'], {}, BOOT_REFINE),                                                   # no --refine, no -o
       (['--boot', '4', '--refine', '--bootBlock', '0'], {}, BOOT_O),                        # no -o, a value
       (BOOT + ['--bootLevel', '2'], WS, ranks('--boot')),                                   # multi-rank, a value
       (BOOT + ['--bootBlock', '0', '--bootLevel', '2', '--bootMin', 'nan'], {}, '--bootBlock must be >= 1.'),
       (BOOT + ['--bootLevel', '2', '--bootMin', 'nan'], {}, '--bootLevel takes a number L with 0 < L < 1.')]
    # ---------------------------------------------------------------------------------------------------------- --refine
    + orphans(['--refineMin 3'], '--refine')
    + common(REFINE, '--refine', REFINE_O)
    + [(REFINE + ['--refineMin', 'nan'], {}, '--refineMin takes a number.'),
       # two faults in the feature
       (['--refine', '--refineMin', 'nan', '--getSpect'], {}, '--refineMin takes a number.'),
       (['--refine', '--getSpect'], WS, helper('--refine')),
       (['--refine'], FD, REFINE_O)]
    # --------------------------------------------------------------------------------------------------------- --support
    + orphans(['--supportDrop 2', '--supportMin 3'], '--support')
    + common(SUPPORT, '--support', REFINE_O, in_name='--refine')          # --support has --refine refuse these
    + [(['--support'] + O, {}, SUPPORT_REFINE),
       (SUPPORT + ['--supportDrop', '0'], {}, '--supportDrop takes a finite number > 0.'),
       (SUPPORT + ['--supportDrop', 'inf'], {}, '--supportDrop takes a finite number > 0.'),
       (SUPPORT + ['--supportDrop', 'nan'], {}, '--supportDrop takes a finite number > 0.'),
       (SUPPORT + ['--supportMin', 'nan'], {}, '--supportMin takes a number.'),
       # two faults in the feature
       (['--support', '--supportDrop', '0'] + O, {}, SUPPORT_REFINE),                        # no --refine, a value
       (SUPPORT + ['--supportDrop', '0', '--supportMin', 'nan'], {}, '--supportDrop takes a finite number > 0.'),
       (['--support', '--supportDrop', '0'], {}, SUPPORT_REFINE)]                            # no --refine, a value, no -o
    # ------------------------------------------------------------------------------------------ faults in two features
    + [(['--locate', '1', '--boot', '1'] + O, {}, LOCATE_R),
       (['--peakMin', '3', '--supportDrop', '1'] + O, {}, '--peakMin needs --peaks.'),
       (['--surfaces', '--nullPerm', '-1'] + O, {}, SURF_WHICH),
       (['--power', '4', '--locate', '1'] + O, {}, POWER_PLANT),
       (['--locate', '8', '--peaks', '-1'] + O, {}, '--peaks takes a separation G >= 0 (in the units the scan measures distance in).'),
       (['--locate', '8', '--peaks', '0.01', '--surfaces'], {}, LOCATE_O),                   # all three lack -o: --locate says so
       (['--peaks', '0.01', '--surfaces'], {}, PEAKS_O),
       (['--nullPerm', '-1', '--profiles', 'z'] + O, {}, NULL_R),
       (['--profiles', 'z', '--bootSeed', '2'] + O, {}, "--profiles: unknown profile 'z' (choose from A, x, abeta)."),
       (['--refineMin', '3', '--bootSeed', '2'] + O, {}, '--bootSeed needs --boot.'),
       (['--boot', '4', '--support'] + O, {}, BOOT_REFINE),
       (['--refine', '--refineMin', 'nan', '--supportMin', '3'] + O, {}, '--refineMin takes a number.'),
       (['--refine', '--boot', '4', '--support'], WS, BOOT_O),
       (['--refine', '--support', '--supportDrop', '0'], {}, REFINE_O),
       (POWER + ['--nullPerm', '3', '--locate', '8', '--peaks', '0.01', '--surfaces', '--profiles', 'A', '--refine', '--boot', '4',
                 '--support'], WS, ranks('--power'))]
)


@pytest.mark.parametrize('tail,env,message', ROWS, ids=[' '.join(t) + ''.join(' %s=%s' % kv for kv in e.items()) for t, e, _ in ROWS])
def test_refusal_message(tail, env, message, tmp_path, monkeypatch, capsys):
    from ballermixplus_amd import engine
    made = []
    monkeypatch.setattr(engine, 'Context', lambda *a, **k: made.append(1))
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.delenv('BMX_FORCE_DIST', raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    argv = ['-i', EX1, '--spect', SPECT] + [str(tmp_path / 'o.txt') if a == 'OUT' else a for a in tail]
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 1
    assert capsys.readouterr().out == message + '\n'
    assert not made and not glob.glob(str(tmp_path / '*'))


def test_the_table_is_complete():
    """Every feature has its orphan rows, the five common refusals, and three rows with two faults; three rows cross features."""
    said = [m for _, _, m in ROWS]
    for f in ('--power', '--locate', '--peaks', '--surfaces', '--nullPerm', '--profiles', '--boot', '--refine'):
        assert helper(f) in said and ranks(f) in said and any(m.startswith(f + ' needs -o: ') for m in said)
    owner = {'plant': 'power', 'atPeaks': 'peaks'}
    owner.update({p: f for f, p in (('power', 'power'), ('locate', 'locate'), ('peaks', 'peak'), ('surfaces', 'surface'),
                                    ('boot', 'boot'), ('refine', 'refine'), ('support', 'support'))})
    subs = 0
    for dest in vars(cli.build_parser().parse_args(['-i', EX1, '--spect', SPECT])):
        f = next((f for p, f in owner.items() if dest.startswith(p) and dest != f), None)
        if f is not None:
            assert '--%s needs --%s.' % (dest, f) in said, dest
            subs += 1
    assert subs == 8 + 6 + 3 + 2 + 5 + 1 + 2
