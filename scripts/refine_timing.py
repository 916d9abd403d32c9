"""Cost of the off-grid refinement (--refine) against the scan, on the synthetic 1M-SNP chromosome of BASELINE config 3 (n = 100,
default grid, every site a test site): refining every window with a grid result, and only the top 1 % of windows by grid CLR
(--refineMin at the 99th percentile); then the same chromosome with 31 sample sizes n = 70..100 (the refinement's workspace no
longer fits LDS and lives in the per-workgroup global slab).  Scan kernel time (events) and refinement wall time (refine + sync),
median of R rounds, with the mean number of compass rounds of the refined windows and how many improved; then the kernel's
registers and scratch from the assembly (`make -C ballermixplus_amd/csrc asm` first, or they are skipped).
Usage: python scripts/refine_timing.py [N] [R]"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from ballermixplus_amd import engine, synth  # noqa: E402
from ballermixplus_amd.hostmodel import Grids  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
R = int(sys.argv[2]) if len(sys.argv) > 2 else 3
phys, gen, k0, n0 = synth.synth_chromosome(N, 100, 1)
xs, ab, As = Grids(None, None, False, False, None, None).scan_order()


def context(k, nn):
    sizes = sorted(set(nn.tolist()))
    sp = {(a, b): f for a, b, f in synth.spect_from_counts(k, nn)}
    props = {s_: float(sum(f for (a, b), f in sp.items() if b == s_)) for s_ in sizes}
    model = engine.ModelArrays('B2', int(k.min()), sizes, sp, props, xs, ab)
    c = engine.Context(0)
    c.set_model(model, As)
    c.set_sites(gen, model.rows_of(k, nn))
    return c


def timed_refine(ctx, min_clr, reps):
    ms = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        ctx.refine(min_clr)
        ctx.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


n2 = np.random.default_rng(5).integers(70, 101, N)
k2 = np.where(k0 == n0, n2, np.maximum(1, np.minimum(n2 - 1, (k0 * n2) // n0)))
for label, (k, nn), reps_all in (('1 size (n = 100)', (k0, n0), R), ('31 sizes (n = 70..100)', (k2, n2), 1)):
    ctx = context(k, nn)
    ctx.set_tests(gen)
    scans = []
    for _ in range(R):
        ctx.scan()
        ctx.sync()
        scans.append(ctx.last_scan_ms())
    scan_ms = float(np.median(scans))
    clr, _, _, iA, _ = ctx.fetch()
    have = iA >= 0
    top = float(np.quantile(clr[have], 0.99))
    print('%s: M = %d test sites, %d with a grid result, scan kernels %.2f ms (plan %s)' % (label, len(gen), have.sum(), scan_ms,
                                                                                          ctx.plan()['kernel']), flush=True)
    for what, cut, reps in (('top 1 %% (CLR >= %.4g)' % top, top, R), ('every window', 0.0, reps_all)):
        ms = timed_refine(ctx, cut, reps)
        r = ctx.fetch_refined()
        done = r['rounds'] >= 0
        imp = r['clr'] > clr
        print('  refine %-28s %6d windows  %10.2f ms  x%.2f scans  %.1f rounds/window  %d improved (mean +%.4g CLR)' % (
            what, done.sum(), ms, ms / scan_ms, r['rounds'][done].mean() if done.any() else 0.0, imp.sum(),
            (r['clr'] - clr)[imp].mean() if imp.any() else 0.0), flush=True)
    ctx.close()
asm = os.path.join(ROOT, 'ballermixplus_amd', 'csrc', 'bmxscan.gfx950.s')
if os.path.exists(asm):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'kernel_resources.py')], capture_output=True, text=True).stdout
    print('\n'.join(l for l in out.splitlines() if l.startswith('kernel') or 'refine' in l))
