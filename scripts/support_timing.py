"""Cost of the support intervals (--support) against the scan and the refinement, on the synthetic 1M-SNP chromosome of
refine_timing.py (n = 100, default grid, every site a test site) and the same chromosome with 31 sample sizes n = 70..100 (the
workspace in the global slab): the top 1 % and the top 0.1 % of windows by refined CLR.  Scan kernel time (events), refinement
and support wall time (call + sync), median of R rounds, with the profile evaluations and compass rounds per task; then the
kernel's registers and scratch from the assembly (`make -C ballermixplus_amd/csrc asm` first, or they are skipped).
Usage: python scripts/support_timing.py [N] [R]"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from ballermixplus_amd import engine, support, synth  # noqa: E402
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
for label, (k, nn), reps in (('1 size (n = 100)', (k0, n0), R), ('31 sizes (n = 70..100)', (k2, n2), 1)):
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
    print('%s: M = %d test sites, %d with a grid result, scan kernels %.2f ms (plan %s)' % (label, len(gen), have.sum(), scan_ms,
                                                                                          ctx.plan()['kernel']), flush=True)
    for q in (0.99, 0.999):
        cut = float(np.quantile(clr[have], q))
        ref_ms = timed(lambda: ctx.refine(cut), reps)
        sup_ms = timed(lambda: ctx.support(support.DROP, cut), reps)
        s = ctx.fetch_support()
        done = s['rounds'] >= 0
        win = done.any(axis=(1, 2)).sum()
        cens = s['censored'][done].mean() if done.any() else 0.0
        worse = (s['T_best'] > s['T_star']).sum()
        print('  top %.1f %% (CLR >= %.4g): %6d windows, %6d tasks  refine %9.2f ms  support %10.2f ms = x%.1f scans = x%.1f '
              'refine  %.1f profiles and %.1f rounds per task (%.1f rounds per profile)  %.0f %% of ends censored  '
              '%d windows with T_best > T*' % (
                  100 * (1 - q), cut, win, done.sum(), ref_ms, sup_ms, sup_ms / scan_ms, sup_ms / ref_ms,
                  s['evals'][done].mean(), s['rounds'][done].mean(), s['rounds'][done].sum() / max(1, s['evals'][done].sum()),
                  100 * cens, worse), flush=True)
    ctx.close()
asm = os.path.join(ROOT, 'ballermixplus_amd', 'csrc', 'bmxscan.gfx950.s')
if os.path.exists(asm):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'kernel_resources.py')], capture_output=True, text=True).stdout
    print('\n'.join(l for l in out.splitlines() if l.startswith('kernel') or 'refine' in l or 'support' in l))
