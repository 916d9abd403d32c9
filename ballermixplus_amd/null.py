"""Permutation null of the CLR: the host half of --nullPerm.

The device permutes the (k, n) row of every site of one chromosome (bmx_ctx_permute_rows), scans each replicate with the
usual kernels and accumulates per-window exceedances and the replicate's maximum CLR (bmx_ctx_null_accumulate).  This
module holds the exact host definition of that permutation (the tests compare the device with it bit for bit), the
p-values and thresholds derived from the accumulated counts and maxima, and the writers of the two output files.

The permutation, on uint64 modulo 2^64:

    mix(z)                = splitmix64
    replicate_key(S, r, f) = mix(mix(mix(S) ^ r) ^ f)      r: replicate, f: input-file ordinal
    sigma(i; N, B, K)     : blocks of B consecutive sites, nb = N // B of them, permuted by an 8-round Feistel network on
                            2h bits (h = max(4, ceil(bit_length(nb - 1) / 2)), round function mix(R ^ mix(K + j)) & (2^h - 1))
                            with cycle walking into [0, nb); the tail of N mod B sites, and everything when nb < 2, stays
    permuted_row[i]       = row[sigma(i)]

Feistel with cycle walking is a keyed pseudorandom permutation, not an exactly uniform shuffle.  The null it gives is
exchangeability of sites (B = 1) or of blocks of B sites under the composite likelihood: LD beyond a block and demography
are not modelled, so it does not replace neutral simulations.
"""
import math

import numpy as np

_M64 = (1 << 64) - 1
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_C1 = np.uint64(0xBF58476D1CE4E5B9)
_C2 = np.uint64(0x94D049BB133111EB)
ROUNDS = 8


def _mix_arr(z):
    z = z + _GOLDEN
    z = (z ^ (z >> np.uint64(30))) * _C1
    z = (z ^ (z >> np.uint64(27))) * _C2
    return z ^ (z >> np.uint64(31))


def mix(z):
    """splitmix64 of a Python int (taken modulo 2^64) or of a uint64 array."""
    with np.errstate(over='ignore'):
        if isinstance(z, np.ndarray):
            return _mix_arr(z.astype(np.uint64, copy=False))
        return int(_mix_arr(np.array([int(z) & _M64], dtype=np.uint64))[0])


def replicate_key(seed, r, f=0):
    """The permutation key of replicate r of input file f (file ordinal 0 for a single file)."""
    return mix(mix(mix(seed) ^ (int(r) & _M64)) ^ (int(f) & _M64))


def _feistel(x, h, m, rk):
    L, R = x >> np.uint64(h), x & m
    for k in rk:
        L, R = R, L ^ (_mix_arr(R ^ k) & m)
    return (L << np.uint64(h)) | R


def block_permutations(N, keys, block=1):
    """sigma of every key in `keys`, shape (len(keys), N): row j is block_permutation(N, keys[j], block)."""
    N, B = int(N), int(block)
    if B < 1:
        raise ValueError('block size must be >= 1')
    keys = np.array([int(k) & _M64 for k in keys], dtype=np.uint64)      # (Python ints: a list of them may not fit int64)
    sig = np.tile(np.arange(N, dtype=np.int64), (len(keys), 1))
    nb = N // B
    if nb < 2:
        return sig
    h = max(4, ((nb - 1).bit_length() + 1) // 2)
    m = np.uint64((1 << h) - 1)
    with np.errstate(over='ignore'):
        rk = [_mix_arr(keys + np.uint64(j)) for j in range(ROUNDS)]          # mix(K + j): the round keys
        x = _feistel(np.tile(np.arange(nb, dtype=np.uint64), (len(keys), 1)), h, m, [k[:, None] for k in rk])
        out = x >= np.uint64(nb)
        while out.any():                         # cycle walking: each cycle of the permutation returns into [0, nb)
            kk = np.nonzero(out)[0]
            x[out] = _feistel(x[out], h, m, [k[kk] for k in rk])
            out = x >= np.uint64(nb)
    sig[:, :nb * B] = (x.astype(np.int64)[:, :, None] * B + np.arange(B, dtype=np.int64)).reshape(len(keys), nb * B)
    return sig


def block_permutation(N, key, block=1):
    """sigma as an int64 array of length N: permuted_row = row[sigma] (the device's bmx_ctx_permute_rows, bitwise)."""
    return block_permutations(N, [key], block)[0]


# ---- p-values and thresholds ----------------------------------------------------------------------------------------

def p_site(counts, R):
    """Pointwise p-value of every window: (1 + #{replicates with CLR >= observed}) / (R + 1)."""
    return (1.0 + np.asarray(counts, dtype=np.float64)) / (R + 1.0)


def p_genome(clr, maxima):
    """Genome-wide (family-wise) p-value of every window: (1 + #{r: max_r >= CLR}) / (R + 1)."""
    mx = np.sort(np.asarray(maxima, dtype=np.float64))
    R = len(mx)
    ge = R - np.searchsorted(mx, np.asarray(clr, dtype=np.float64), side='left')
    return (1.0 + ge) / (R + 1.0)


def threshold(maxima, q):
    """Genome-wide CLR threshold at level q (e.g. 0.95): the ceil(q * R)-th smallest replicate maximum."""
    mx = np.sort(np.asarray(maxima, dtype=np.float64))
    R = len(mx)
    if R == 0:
        raise ValueError('no replicates')
    k = min(max(math.ceil(round(q * R, 9)), 1), R)
    return float(mx[k - 1])


# ---- output ---------------------------------------------------------------------------------------------------------

NULL_HEADER = 'replicate\tmaxCLR\n'
PVAL_HEADER = 'physPos\tgenPos\tCLR\tp_site\tp_genome\n'


def write_null(path, maxima):
    """One row per replicate: its genome-wide maximum CLR (repr)."""
    with open(path, 'w') as f:
        f.write(NULL_HEADER)
        f.writelines('%d\t%r\n' % (r, float(v)) for r, v in enumerate(np.asarray(maxima, dtype=np.float64).tolist()))


def write_pval(path, ts, clr, iA, counts, maxima):
    """One row per row of the main output, in its order: physPos, genPos and CLR printed as the main output prints them,
    then p_site and p_genome; rows that the main output prints without a scan result (ts.na_rows) carry NA."""
    R = len(maxima)
    ps = p_site(counts, R).tolist()
    pg = p_genome(clr, maxima).tolist()
    clr = np.asarray(clr, dtype=np.float64).tolist()
    iA = np.asarray(iA).tolist()
    if ts.arrays is not None:
        phys, gen = ts.arrays[0].tolist(), ts.arrays[1].tolist()
    else:
        phys = [float(v) if isinstance(v, np.floating) else v for v in ts.phys]
        gen = [float(v) if isinstance(v, np.floating) else v for v in ts.gen_label]
    body = [f'{p}\t{g}\t{c if a >= 0 else 0.0}\t{s!r}\t{q!r}\n' for p, g, c, a, s, q in zip(phys, gen, clr, iA, ps, pg)]
    if ts.na_rows:
        lines = [None] * (len(ts) + len(ts.na_rows))
        for pos, line in ts.na_rows.items():
            lines[pos] = '\t'.join(line.rstrip('\n').split('\t')[:3]) + '\tNA\tNA\n'
        for j, pos in enumerate(ts.order):
            lines[pos] = body[j]
    else:
        lines = body
    with open(path, 'w') as f:
        f.write(PVAL_HEADER)
        f.writelines(lines)


def run_file(ctx, R, seed, block, f):
    """The null of the chromosome in ctx's selected slot, whose observed scan has just run: R replicates keyed
    replicate_key(seed, r, f).  Returns (observed clr, iA, counts[M], maxima[R]); the slot's rows are restored."""
    clr, _, _, iA, _ = ctx.fetch()
    ctx.null_begin()
    maxima = np.empty(R, dtype=np.float64)
    for r in range(R):
        ctx.permute_rows(replicate_key(seed, r, f), block)
        ctx.scan()
        maxima[r] = ctx.null_accumulate()
    counts, reps = ctx.null_fetch()
    ctx.restore_rows()
    assert reps == R
    return clr, iA, counts, maxima
