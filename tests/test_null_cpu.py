"""The permutation null's host half without a GPU: the permutation's exact definition (ballermixplus_amd/null.py, which the
device reproduces bit for bit), the p-value and threshold arithmetic, and the --nullPerm / --nullSeed / --nullBlock flags
with their refusals."""
import math
import os

import numpy as np
import pytest

from util import REFT

from ballermixplus_amd import null
from ballermixplus_amd.cli import build_parser

M64 = (1 << 64) - 1


def _mix_py(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _sigma_py(i, N, B, K):
    """The definition of the permutation in plain Python integers, one site at a time."""
    nb = N // B
    if nb < 2 or i >= nb * B:
        return i
    b, o = divmod(i, B)
    w = (nb - 1).bit_length()
    h = max(4, math.ceil(w / 2))
    m = (1 << h) - 1

    def feistel(x):
        L, R = x >> h, x & m
        for j in range(8):
            L, R = R, L ^ (_mix_py(R ^ _mix_py((K + j) & M64)) & m)
        return (L << h) | R

    x = feistel(b)
    while x >= nb:
        x = feistel(x)
    return x * B + o


def test_mix_known_values():
    # splitmix64's first outputs from state 0 (the generator adds the constant before mixing)
    assert null.mix(0) == 0xE220A8397B1DCDAF
    assert null.mix(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert null.mix((2 * 0x9E3779B97F4A7C15) & M64) == 0x06C45D188009454F
    for z in (1, 7, 12345678901234567, M64):
        assert null.mix(z) == _mix_py(z)
    arr = np.array([0, 1, M64], dtype=np.uint64)
    assert null.mix(arr).tolist() == [_mix_py(0), _mix_py(1), _mix_py(M64)]
    assert null.replicate_key(7, 3, 1) == _mix_py(_mix_py(_mix_py(7) ^ 3) ^ 1)


@pytest.mark.parametrize('N', [1, 2, 5, 255, 256, 257, 10 ** 5 + 3, 2 ** 20 + 7])
def test_block_permutation_is_a_bijection(N):
    key = null.replicate_key(1, 0, 0)
    for B in (1, 3, 64, N, N + 1):
        s = null.block_permutation(N, key, B)
        assert s.dtype == np.int64 and len(s) == N
        assert np.array_equal(np.sort(s), np.arange(N)), (N, B)


@pytest.mark.parametrize('N,B', [(10, 1), (257, 1), (257, 3), (1000, 64), (5, 2), (300, 7)])
def test_block_permutation_matches_the_plain_definition(N, B):
    for r in range(3):
        K = null.replicate_key(11, r, 2)
        want = [_sigma_py(i, N, B, K) for i in range(N)]
        assert null.block_permutation(N, K, B).tolist() == want


def test_tail_stays_and_blocks_keep_their_order():
    N, B = 1003, 10
    s = null.block_permutation(N, null.replicate_key(5, 1, 0), B)
    assert np.array_equal(s[1000:], np.arange(1000, N))              # N mod B sites in place
    blocks = s[:1000].reshape(100, B)
    assert np.all(blocks % B == np.arange(B))                        # each block moved whole, inner order kept
    assert np.all(np.diff(blocks, axis=1) == 1)
    assert not np.array_equal(blocks[:, 0], np.arange(0, 1000, B))    # and the blocks did move
    # fewer than two whole blocks: nothing moves
    assert np.array_equal(null.block_permutation(19, 123, 10), np.arange(19))


def test_replicate_and_file_give_different_permutations():
    N = 5000
    base = null.block_permutation(N, null.replicate_key(1, 0, 0))
    assert not np.array_equal(base, np.arange(N))
    for r, f in ((1, 0), (2, 0), (0, 1), (0, 2), (1, 1)):
        assert not np.array_equal(base, null.block_permutation(N, null.replicate_key(1, r, f)))
    assert not np.array_equal(base, null.block_permutation(N, null.replicate_key(2, 0, 0)))
    assert np.array_equal(base, null.block_permutation(N, null.replicate_key(1, 0, 0)))          # deterministic
    many = null.block_permutations(N, [null.replicate_key(1, r, 0) for r in range(3)])
    assert np.array_equal(many[0], base)


def test_marginal_uniformity():
    """N = 10, single sites, 20 000 keys: every (i, sigma(i)) cell holds 2000 +- 5 sigma."""
    S = null.block_permutations(10, [null.replicate_key(2024, r, 0) for r in range(20000)], 1)
    cells = np.stack([np.bincount(S[:, i], minlength=10) for i in range(10)])
    sd = math.sqrt(20000 * 0.1 * 0.9)
    assert np.max(np.abs(cells - 2000)) <= 5 * sd, cells


def test_p_values_and_thresholds():
    maxima = np.array([5.0, 1.0, 3.0, 2.0, 4.0, 4.0, 9.0, 0.5, 7.0, 6.0])     # R = 10
    R = len(maxima)
    counts = np.array([0, 3, 10])
    assert np.allclose(null.p_site(counts, R), [1 / 11, 4 / 11, 1.0])
    clr = np.array([10.0, 9.0, 4.0, 0.1, 4.5])
    # #{max >= clr}: 0, 1, 6 (4, 4, 5, 6, 7, 9), 10, 4
    assert np.allclose(null.p_genome(clr, maxima), np.array([1, 2, 7, 11, 5]) / 11.0)
    # ceil(q R)-th smallest: sorted 0.5 1 2 3 4 4 5 6 7 9
    assert null.threshold(maxima, 0.95) == 9.0          # 10th
    assert null.threshold(maxima, 0.9) == 7.0           # 9th
    assert null.threshold(maxima, 0.5) == 4.0           # 5th
    m20 = np.arange(20, dtype=np.float64)[::-1]
    assert null.threshold(m20, 0.95) == 18.0            # 19th of 0..19
    assert null.threshold(np.arange(100.0), 0.99) == 98.0
    with pytest.raises(ValueError):
        null.threshold([], 0.95)


def test_writers(tmp_path):
    from ballermixplus_amd import scan as scanmod
    p = tmp_path / 'n.txt'
    null.write_null(str(p), [1.5, 0.1 + 0.2])
    assert p.read_text() == 'replicate\tmaxCLR\n0\t1.5\n1\t0.30000000000000004\n'
    ts = scanmod.TestSites()
    ts.add(100, 0.1, 0.1, 0, 5)
    ts.add_na('150\t0.00015\t0\tNA\tNA\tNA\t0\n')
    ts.add(200.5, 0.2, 0.2, 1, 6)
    q = tmp_path / 'p.txt'
    null.write_pval(str(q), ts, np.array([3.25, 0.0]), np.array([0, -1]), np.array([1, 4]), np.array([1.0, 5.0, 2.0, 3.0]))
    assert q.read_text().splitlines() == ['physPos\tgenPos\tCLR\tp_site\tp_genome', '100\t0.1\t3.25\t0.4\t0.4',
                                          '150\t0.00015\t0\tNA\tNA', '200.5\t0.2\t0.0\t1.0\t1.0']


def test_null_flags_parse_with_their_defaults():
    o = build_parser().parse_args(['-i', 'x', '--spect', 'y'])
    assert (o.nullPerm, o.nullSeed, o.nullBlock) == (0, 1, 1)
    o = build_parser().parse_args(['-i', 'x', '--spect', 'y', '--nullPerm', '100', '--nullSeed', '7', '--nullBlock', '50'])
    assert (o.nullPerm, o.nullSeed, o.nullBlock) == (100, 7, 50)


def _refused(argv, capsys, monkeypatch, env=None):
    from ballermixplus_amd import cli
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 1
    return capsys.readouterr().out


def test_null_refusals(tmp_path, capsys, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.delenv('BMX_FORCE_DIST', raising=False)
    inp = os.path.join(REFT, 'Example1_fullSweep_200kya_DAF.txt')
    spect = os.path.join(REFT, 'HC_CEU_Neut_DAF_spect_for_B2.txt')
    base = ['-i', inp, '--spect', spect, '--nullPerm', '5']
    out = _refused(base, capsys, monkeypatch)
    assert '-o' in out
    out = _refused(['-i', inp, '--spect', str(tmp_path / 's.txt'), '--getSpect', '--nullPerm', '5', '-o', str(tmp_path / 'o')],
                   capsys, monkeypatch)
    assert '--getSpect' in out and not (tmp_path / 's.txt').exists()
    out = _refused(['-i', inp, '--spect', str(tmp_path / 's.txt'), '--getConfig', '--nullPerm', '5'], capsys, monkeypatch)
    assert '--getConfig' in out
    out = _refused(base + ['-o', str(tmp_path / 'o.txt')], capsys, monkeypatch, env={'WORLD_SIZE': '2', 'RANK': '0'})
    assert 'multi-rank' in out and not (tmp_path / 'o.txt').exists()
    out = _refused(base + ['-o', str(tmp_path / 'o.txt'), '--nullBlock', '0'], capsys, monkeypatch)
    assert '--nullBlock' in out
