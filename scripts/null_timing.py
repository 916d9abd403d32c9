"""Cost of one permutation-null replicate (--nullPerm) against the observed scan, on the synthetic 1M-SNP chromosome of
BASELINE config 3 (n = 100, default grid, every site a test site, all-sites windows): the permute kernel, the re-done plan and
counting pass of the prepared pipeline, the scan kernel and the accumulate, per replicate; and the permute kernel alone on
10 M sites.  Usage: python scripts/null_timing.py [N] [replicates]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from ballermixplus_amd import engine, null, synth  # noqa: E402
from ballermixplus_amd.hostmodel import Grids  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
R = int(sys.argv[2]) if len(sys.argv) > 2 else 10
phys, gen, k, nn = synth.synth_chromosome(N, 100, 1)
xs, ab, As = Grids(None, None, False, False, None, None).scan_order()
sp = {(a, b): f for a, b, f in synth.spect_from_counts(k, nn)}
model = engine.ModelArrays('B2', int(k.min()), [100], sp, {100: 1.0}, xs, ab)
rows = model.rows_of(k, nn)
ctx = engine.Context(0)
ctx.set_model(model, As)
ctx.set_sites(gen, rows)
lo, hi = np.zeros(N, np.int64), np.full(N, N - 1, np.int64)


def wall(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


# observed scan: set_tests makes the plan and runs the counting pass; scan launches; sync waits for the kernels
obs_prep = wall(lambda: ctx.set_tests(gen, lo, hi))
obs_wall = wall(lambda: (ctx.scan(), ctx.sync()))
obs_kernel = ctx.last_scan_ms()
ctx.scan()
ctx.sync()
obs_kernel2 = ctx.last_scan_ms()
print('N = %d sites, M = %d test sites, default grid (%d x %d x %d), plan %s' % (N, N, len(xs), len(ab), len(As), ctx.plan()['kernel']))
print('observed: set_tests (plan + counting pass) %.1f ms | scan + sync %.1f ms (kernel %.1f ms; again %.1f ms)'
      % (obs_prep, obs_wall, obs_kernel, obs_kernel2))
ctx.null_begin()
rec = []
for r in range(R):
    key = null.replicate_key(1, r, 0)
    t_perm = wall(lambda: (ctx.permute_rows(key, 1), ctx.sync()))
    t_prep = wall(ctx.scan)             # plan + counting pass (synchronous) + asynchronous launches
    t_rest = wall(ctx.sync)
    kern = ctx.last_scan_ms()
    t_acc = wall(ctx.null_accumulate)
    rec.append((t_perm, t_prep, t_rest, kern, t_acc))
    print('replicate %2d: permute %.2f ms | scan call (re-prep + launch) %.1f ms | wait %.1f ms (scan kernel %.1f ms) | accumulate %.2f ms'
          ' | total %.1f ms' % (r, t_perm, t_prep, t_rest, kern, t_acc, t_perm + t_prep + t_rest + t_acc))
ctx.restore_rows()
a = np.array(rec[1:] if R > 1 else rec)
tot = a[:, 0] + a[:, 1] + a[:, 2] + a[:, 4]
print('median over replicates 1..%d: permute %.2f ms, scan call %.1f ms, wait %.1f ms, accumulate %.2f ms, total %.1f ms'
      % (R - 1, np.median(a[:, 0]), np.median(a[:, 1]), np.median(a[:, 2]), np.median(a[:, 4]), np.median(tot)))
print('replicate / observed scan (scan + sync): %.3f;  replicate / observed (set_tests + scan + sync): %.3f'
      % (np.median(tot) / obs_wall, np.median(tot) / (obs_prep + obs_wall)))
ctx.close()

# the permute kernel alone, 10 M sites (2-byte rows), blocks of 1 and 100 sites; 20 launches back to back
N2 = 10_000_000
phys2, gen2, k2, nn2 = synth.synth_chromosome(N2, 100, 2)
sp2 = {(a, b): f for a, b, f in synth.spect_from_counts(k2, nn2)}
model2 = engine.ModelArrays('B2', int(k2.min()), [100], sp2, {100: 1.0}, xs, ab)
ctx = engine.Context(0)
ctx.set_model(model2, As)
ctx.set_sites(gen2, model2.rows_of(k2, nn2))
ctx.permute_rows(1, 1)                   # first call: also keeps the given rows
ctx.sync()
for B in (1, 100):
    t = wall(lambda: ([ctx.permute_rows(null.replicate_key(3, r, 0), B) for r in range(20)], ctx.sync()))
    print('permute kernel, %d sites, blocks of %d: %.3f ms per launch (wall, 20 launches back to back)' % (N2, B, t / 20))
ctx.close()
