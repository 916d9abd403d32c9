"""The one-file form (-i FILE -o OUT) and the several-files form (--inputs LIST -o DIR, LIST naming that one file) of the same
command line write the same per-file files, byte for byte: both run the same stages in the same order on file ordinal 0, which
keys every random stream.  Two command lines: every addition the default window mode allows at once, with --nullPerm (the
power step waits for the null's thresholds), and a shorter one without it (the power step runs with the file's stages)."""
import glob
import os

import pytest

import powercases as pc

from ballermixplus_amd import cli, helpers, synth

pytestmark = pytest.mark.gpu

POWER = ['--power', str(pc.E2E_R), '--plant', pc.E2E_PLANT, '--powerReps', '--powerSeed', '5']
THRESHOLDS = ['--powerThreshold', ','.join(repr(C) for C in pc.E2E_THRESHOLDS)]


def everything(G):
    return (['--profiles', 'A,x,abeta', '--peaks', G, '--atPeaks', '--refine', '--support', '--boot', '4', '--bootSeed', '2', '--bootReps',
             '--surfaces', '--locate', '4', '--locateSeed', '3', '--locateReps', '--nullPerm', '3', '--nullSeed', '4'] + POWER)


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


@pytest.mark.parametrize('flags,companions', [
    (everything, {'.profile_A.txt', '.profile_x.txt', '.profile_abeta.txt', '.peaks.txt', '.refined.txt', '.support.txt', '.boot.txt',
                  '.boot.reps.txt', '.surfaces.txt', '.locate.txt', '.locate.reps.txt', '.pval.txt', '.power.txt', '.power.reps.txt',
                  '.null.txt'}),
    (inline_power, {'.peaks.txt', '.refined.txt', '.power.txt', '.power.reps.txt'}),
])
def test_both_forms_write_the_same_files(chromosome, flags, companions, tmp_path):
    d, inp, sp, lst, G = chromosome
    tail = ['--spect', sp] + pc.E2E_GRID + flags(G)
    out, many = str(tmp_path / 'one.txt'), str(tmp_path / 'many')
    cli.main(['-i', inp, '-o', out] + tail)
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
