"""Writes tests/golden/fold_tails.npz: the scan records (clr as uint64 bits, lin, nsites), the plan's kernel and the profile
arrays' bits of every case of tests/foldtails.py, as the library in the tree (or the one BMX_LIB_NAME names) computes them on the
GPU.  It was run with the library of the commit BEFORE the prepared scan kernels began to shorten the last blocks of the near
lists; tests/test_gpu_fold_tails.py holds every later build to those bits.
Every case is checked against the C oracle before it is written (the bar of the GPU tests: argmax and nSites equal, CLR rtol
1e-9, atol 1e-12), so the file holds no bits the oracle does not vouch for.
    python tests/golden/gen_fold_tails.py [output.npz]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import foldtails as ft  # noqa: E402
from util import c_oracle, c_scan  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def main(out):
    from ballermixplus_amd import engine as eng
    store, ctxs = {}, {}
    names = sorted(ft.CASES)
    for name in names:
        c = ft.CASES[name]
        key = (c['data'], c['a'])
        if key not in ctxs:
            ctxs[key] = ft.open_data(eng, *key)
        ctx, gen, rows, R = ctxs[key]
        rec, plan, prof = ft.run(ctx, gen, name)
        assert c['kernel'] is None or plan['kernel'] == c['kernel'], (name, plan)
        ft.check_oracle(rec, ft.oracle(c_scan, c_oracle(), R, gen, rows, name), name)
        tag = 'case%02d' % names.index(name)
        store[tag + '_clr'] = bits(rec['clr'])
        store[tag + '_lin'] = rec['lin'].astype(np.int32)
        store[tag + '_nsites'] = rec['nsites'].astype(np.int32)
        store[tag + '_kernel'] = np.array(plan['kernel'])
        if prof:
            for k, p in prof.items():
                store[tag + '_prof_' + k] = bits(p)
        print('%-36s %-34s %4d windows, %3d without a winner, CLR up to %.4g' % (name, plan['kernel'], len(rec), int((rec['lin'] < 0).sum()), rec['clr'].max()))
    for ctx, _, _, _ in ctxs.values():
        ctx.close()
    store['names'] = np.array(names)
    np.savez_compressed(out, **store)
    print('%s: %d bytes' % (out, os.path.getsize(out)))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'fold_tails.npz'))
