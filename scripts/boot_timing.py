"""Cost of the block bootstrap (--boot) against the refinement, on the synthetic 1M-SNP chromosome of refine_timing.py
(n = 100, default grid, every site a test site) and the same chromosome with 31 sample sizes n = 70..100 (the workspace in
the global slab): the top 1 % and the top 0.1 % of windows by refined CLR, REPS replicates, blocks of 1 and of 64 sites.
Refinement and bootstrap wall time (call + sync; the refinement the median of R rounds, the bootstrap one run), the time per
task, the mean rounds per task, the share of replicates that are not ok, and the ratio to REPS refinements of the same
windows re-measured in the same run -- a replicate is one more compass search of its window.  Then the kernels' registers and
scratch from the assembly (`make -C ballermixplus_amd/csrc asm` first, or they are skipped).
Usage: python scripts/boot_timing.py [N] [R] [REPS]"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from ballermixplus_amd import boot, engine, synth  # noqa: E402
from ballermixplus_amd.hostmodel import Grids  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
R = int(sys.argv[2]) if len(sys.argv) > 2 else 3
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 100
phys, gen, k0, n0 = synth.synth_chromosome(N, 100, 1)
xs, ab, As = Grids(None, None, False, False, None, None).scan_order()
keys = [boot.replicate_key(1, r, 0) for r in range(REPS)]


def context(k, nn):
    sizes = sorted(set(nn.tolist()))
    sp = {(a, b): f for a, b, f in synth.spect_from_counts(k, nn)}
    props = {s_: float(sum(f for (a, b), f in sp.items() if b == s_)) for s_ in sizes}
    model = engine.ModelArrays('B2', int(k.min()), sizes, sp, props, xs, ab)
    c = engine.Context(0)
    c.set_model(model, As)
    c.set_sites(gen, model.rows_of(k, nn))
    return c


def timed(fn, reps):
    ms = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


n2 = np.random.default_rng(5).integers(70, 101, N)
k2 = np.where(k0 == n0, n2, np.maximum(1, np.minimum(n2 - 1, (k0 * n2) // n0)))
for label, (k, nn) in (('1 size (n = 100)', (k0, n0)), ('31 sizes (n = 70..100)', (k2, n2))):
    ctx = context(k, nn)
    ctx.set_tests(gen)
    ctx.scan()
    ctx.sync()
    clr, _, _, iA, _ = ctx.fetch()
    have = iA >= 0
    print('%s: M = %d test sites, %d with a grid result, scan kernels %.2f ms (plan %s)' % (label, len(gen), have.sum(),
                                                                                          ctx.last_scan_ms(), ctx.plan()['kernel']), flush=True)
    for q in (0.99, 0.999):
        cut = float(np.quantile(clr[have], q))
        ref_ms = timed(lambda: ctx.refine(cut), R)
        ref = ctx.fetch_refined()
        win = int((ref['rounds'] >= 0).sum())
        print('  top %.1f %% (CLR >= %.4g): %6d windows  refine %9.2f ms = %.1f us per window, %.1f rounds per window' % (
            100 * (1 - q), cut, win, ref_ms, 1e3 * ref_ms / max(win, 1), ref['rounds'][ref['rounds'] >= 0].mean()), flush=True)
        for B in (1, 64):
            ms = timed(lambda: ctx.boot(keys, B, cut), 1)
            b = ctx.fetch_boot()
            tasks = b['T'].size
            print('    R = %d, B = %2d: %8d tasks  boot %10.2f ms = %.1f us per task = x%.2f of %d refinements  %.1f rounds per task  '
                  '%.2f %% of replicates not ok' % (REPS, B, tasks, ms, 1e3 * ms / max(tasks, 1), ms / (REPS * ref_ms), REPS,
                                                   b['rounds'].mean(), 100.0 * (~np.isfinite(b['T'])).mean()), flush=True)
    ctx.close()
asm = os.path.join(ROOT, 'ballermixplus_amd', 'csrc', 'bmxscan.gfx950.s')
if os.path.exists(asm):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'kernel_resources.py')], capture_output=True, text=True).stdout
    print('\n'.join(l for l in out.splitlines() if l.startswith('kernel') or 'refine' in l or 'support' in l or 'boot' in l))
