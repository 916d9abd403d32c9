"""Writes tests/golden/stream_scalars.npz: the scan records (clr as uint64 bits, lin, nsites), the plan's kernel and the profile
arrays' bits of every case of tests/streamscalars.py, as the library in the tree computes them on the GPU.  It was run on the
commit BEFORE the preparation kernel began to write F_j, G_k / H_k and the list budgets into the stream; the test
tests/test_gpu_stream_scalars.py holds every later build to those bits.  Every case is checked against the C oracle before it is
written (the bar of the GPU tests: argmax and nSites equal, CLR rtol 1e-9, atol 1e-12), so the file holds no bits the oracle
does not vouch for.
    python tests/golden/gen_stream_scalars.py [output.npz]"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import streamscalars as ss  # noqa: E402
from util import c_oracle, c_scan  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def main(out):
    from ballermixplus_amd import engine as eng
    store, ctxs = {}, {}
    names = sorted(ss.CASES)
    for name in names:
        c = ss.CASES[name]
        key = (c['data'], c['a'])
        if key not in ctxs:
            ctxs[key] = ss.open_data(eng, *key)
        ctx, gen, rows, R = ctxs[key]
        rec, plan, prof = ss.run(ctx, gen, name)
        assert c['kernel'] is None or plan['kernel'] == c['kernel'], (name, plan)
        ss.check_oracle(rec, ss.oracle(c_scan, c_oracle(), R, gen, rows, name), name)
        tag = 'case%02d' % names.index(name)
        store[tag + '_clr'] = bits(rec['clr'])
        store[tag + '_lin'] = rec['lin'].astype(np.int32)
        store[tag + '_nsites'] = rec['nsites'].astype(np.int32)
        store[tag + '_kernel'] = np.array(plan['kernel'])
        if prof:
            for k, p in prof.items():
                store[tag + '_prof_' + k] = bits(p)
        print('%-28s %-34s %4d windows, %3d without a winner, CLR up to %.4g' % (name, plan['kernel'], len(rec), int((rec['lin'] < 0).sum()), rec['clr'].max()))
    for ctx, _, _, _ in ctxs.values():
        ctx.close()
    store['names'] = np.array(names)
    # several launch ranges
    ctx, gen, rows, As = ss.ranges_ctx(eng)
    ctx.scan()
    rec = ctx.fetch_records()
    cuts = ctx.launch_ranges()
    assert len(cuts) >= 2, cuts
    at = ss.ranges_sample(cuts, len(rec))
    store['ranges_cuts'] = np.asarray(cuts, dtype=np.int64)
    store['ranges_at'] = at
    store['ranges_clr'] = bits(rec['clr'][at])
    store['ranges_lin'] = rec['lin'][at].astype(np.int32)
    store['ranges_nsites'] = rec['nsites'][at].astype(np.int32)
    store['ranges_sha256'] = np.array(hashlib.sha256(rec.tobytes()).hexdigest())
    store['ranges_prof_A_sha256'] = np.array(hashlib.sha256(ctx.fetch_profile('A').tobytes()).hexdigest())
    print('launch ranges: %d test sites, cuts %s, %d records kept, plan %s' % (len(rec), cuts.tolist(), len(at), ctx.plan()['kernel']))
    ctx.close()
    np.savez_compressed(out, **store)
    print('%s: %d bytes' % (out, os.path.getsize(out)))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'stream_scalars.npz'))
