"""The one-file form (-i FILE -o OUT) and the several-files form (--inputs LIST -o DIR, LIST naming that one file) of the same
command line write the same per-file files, byte for byte: both run the same stages in the same order on file ordinal 0, which
keys every random stream.  Two command lines: every addition the default window mode allows at once, with --nullPerm (the
power step waits for the null's thresholds), and a shorter one without it (the power step runs with the file's stages).
The listed-window stages of the first command line (--influence, --fit, --conditional) write, amid the replicate-making stages
(boot, locate, null, power), byte for byte what they write after a scan and a peak call alone."""
import glob
import os

import pytest

import powercases as pc

from ballermixplus_amd import cli, conditional, fit, helpers, influence, synth

pytestmark = pytest.mark.gpu

POWER = ['--power', str(pc.E2E_R), '--plant', pc.E2E_PLANT, '--powerReps', '--powerSeed', '5']
THRESHOLDS = ['--powerThreshold', ','.join(repr(C) for C in pc.E2E_THRESHOLDS)]


def everything(G):
    return (['--profiles', 'A,x,abeta', '--peaks', G, '--atPeaks', '--refine', '--support', '--boot', '4', '--bootSeed', '2', '--bootReps',
             '--surfaces', '--influence', '--fit', '--conditional', '--locate', '4', '--locateSeed', '3', '--locateReps', '--nullPerm', '3',
             '--nullSeed', '4'] + POWER)


# the listed-window stages that came after --surfaces: flag -> the suffix of its file, from the module that writes it
LISTED = {'--influence': influence.output_name(''), '--fit': fit.output_name(''), '--conditional': conditional.output_name('')}


def inline_power(G):
    return ['--peaks', G, '--refine'] + POWER + THRESHOLDS


@pytest.fixture(scope='module')
def chromosome(tmp_path_factory):
    d = tmp_path_factory.mktemp('forms')
    e = pc.e2e()
    inp, sp, lst = str(d / 'in.txt'), str(d / 'spect.txt'), str(d / 'list.txt')
    synth.write_input(inp, e.phys, e.gen, e.k, e.nn)
    helpers.getSpect(inp, sp, False, False)
    with open(lst, 'w') as f:
        f.write('in.txt\n')
    return d, inp, sp, lst, repr(float(e.H))


_ONE = {}


def _one_file(chromosome, flags):
    """The one-file form of a command line, run once per module: the path of its main output."""
    d, inp, sp, lst, G = chromosome
    if flags.__name__ not in _ONE:
        os.mkdir(str(d / flags.__name__))
        out = str(d / flags.__name__ / 'one.txt')
        cli.main(['-i', inp, '-o', out, '--spect', sp] + pc.E2E_GRID + flags(G))
        _ONE[flags.__name__] = out
    return _ONE[flags.__name__]


@pytest.mark.parametrize('flags,companions', [
    (everything, {'.profile_A.txt', '.profile_x.txt', '.profile_abeta.txt', '.peaks.txt', '.refined.txt', '.support.txt', '.boot.txt',
                  '.boot.reps.txt', '.surfaces.txt', '.locate.txt', '.locate.reps.txt', '.pval.txt', '.power.txt', '.power.reps.txt',
                  '.null.txt'} | set(LISTED.values())),
    (inline_power, {'.peaks.txt', '.refined.txt', '.power.txt', '.power.reps.txt'}),
])
def test_both_forms_write_the_same_files(chromosome, flags, companions, tmp_path):
    d, inp, sp, lst, G = chromosome
    tail = ['--spect', sp] + pc.E2E_GRID + flags(G)
    out, many = _one_file(chromosome, flags), str(tmp_path / 'many')
    cli.main(['--inputs', lst, '-o', many] + tail)
    rd = lambda p: open(p, 'rb').read()
    twin = os.path.join(many, 'in.txt.out.txt')
    assert {p[len(out):] for p in glob.glob(out + '.*')} == companions
    assert rd(out) == rd(twin) and len(rd(out).splitlines()) == pc.E2E_N + 1
    for suffix in companions:
        other = os.path.join(many, 'null.txt') if suffix == '.null.txt' else twin + suffix
        assert rd(out + suffix) == rd(other), suffix
        assert len(rd(out + suffix).splitlines()) > 1, suffix              # (a header alone would compare nothing)
    # the several-files form adds only its genome-wide peak table
    assert sorted(os.listdir(many)) == sorted([os.path.basename(twin) + s for s in companions - {'.null.txt'}] + ['in.txt.out.txt', 'peaks.txt']
                                              + (['null.txt'] if '.null.txt' in companions else []))


def test_the_listed_window_stages_do_not_depend_on_the_stages_around_them(chromosome, tmp_path):
    """Each of --influence, --fit and --conditional, alone after the scan and the peak call, writes the file it writes in the
    all-stages run: boot, locate, null and power replicates before and after it leave nothing behind that these stages read."""
    d, inp, sp, lst, G = chromosome
    full = _one_file(chromosome, everything)
    rd = lambda p: open(p, 'rb').read()
    assert set(LISTED.values()) == {'.influence.txt', '.fit.txt', '.conditional.txt'}
    for flag, suffix in LISTED.items():
        out = str(tmp_path / (flag.strip('-') + '.txt'))
        cli.main(['-i', inp, '-o', out, '--spect', sp] + pc.E2E_GRID + ['--peaks', G, flag])
        assert {p[len(out):] for p in glob.glob(out + '.*')} == {'.peaks.txt', suffix}, flag
        assert len(rd(out + suffix).splitlines()) > 1, flag
        assert rd(out + suffix) == rd(full + suffix), flag
