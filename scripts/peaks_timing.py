"""Cost of the peak call (--peaks) and what --atPeaks saves, on the synthetic 1M-SNP chromosome of refine_timing.py (n = 100,
default grid, every site a test site), at separations G = 0.01, 0.05 and 0.2 (about 140, 690 and 2 760 rows either side).
Per G: the peak call's device time (bmx_ctx_peaks_ms: HIP events from its first kernel to its last, the median of R calls
after one warm-up call) next to last_scan_ms of the same scan, the number of apexes, and the same call on the host-uploaded
track (bmx_ctx_peaks_track).  Then refinement + support intervals + a bootstrap of REPS replicates of the windows with
CLR >= the Q quantile (what --refine --refineMin C --support --boot REPS run after the scan): wall time of the three calls, each
ended by a synchronise, without the restriction (once: the parent's path) and restricted to the apexes of each G, with the
number of windows done.  Then the kernels' registers and scratch from the assembly (`make -C ballermixplus_amd/csrc asm` first,
or they are skipped).
Usage: python scripts/peaks_timing.py [N] [R] [REPS] [Q]"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from ballermixplus_amd import boot, engine, support, synth  # noqa: E402
from ballermixplus_amd.hostmodel import Grids  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
R = int(sys.argv[2]) if len(sys.argv) > 2 else 9
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 100
Q = float(sys.argv[4]) if len(sys.argv) > 4 else 0.99
SEPS = (0.01, 0.05, 0.2)
phys, gen, k, nn = synth.synth_chromosome(N, 100, 1)
xs, ab, As = Grids(None, None, False, False, None, None).scan_order()
keys = [boot.replicate_key(1, r, 0) for r in range(REPS)]
sp = {(a, b): f for a, b, f in synth.spect_from_counts(k, nn)}
model = engine.ModelArrays('B2', int(k.min()), [100], sp, {100: 1.0}, xs, ab)
ctx = engine.Context(0)
ctx.set_model(model, As)
ctx.set_sites(gen, model.rows_of(k, nn))
ctx.set_tests(gen)
ctx.scan()
ctx.sync()
ctx.scan()                  # (the first scan of a process also loads the code objects)
ctx.sync()
scan_ms = ctx.last_scan_ms()
clr, _, _, iA, _ = ctx.fetch()
print('M = %d test sites, scan kernels %.2f ms (plan %s)' % (len(gen), scan_ms, ctx.plan()['kernel']), flush=True)
rows_per_unit = len(gen) / float(gen[-1] - gen[0])
for G in SEPS:
    ctx.peaks(G)
    ms = []
    for _ in range(R):
        pk = ctx.peaks(G)
        ms.append(ctx.peaks_ms())
    ctx.peaks_track(gen, clr, G)
    tr = []
    for _ in range(R):
        ctx.peaks_track(gen, clr, G)
        tr.append(ctx.peaks_ms())
    print('G = %-5g (~%5.0f rows either side): %6d apexes  peak call %7.3f ms (min %.3f, max %.3f) = %.3f %% of the scan;  uploaded track %7.3f ms'
          % (G, G * rows_per_unit, len(pk['row']), np.median(ms), min(ms), max(ms), 100 * np.median(ms) / scan_ms, np.median(tr)), flush=True)


def after_scan(cut):
    """What --refine --refineMin cut --support --boot REPS run: (wall ms of refine, support, boot; windows done)."""
    out = []
    for fn in (lambda: ctx.refine(cut), lambda: ctx.support(support.DROP, cut), lambda: ctx.boot(keys, 1, cut)):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out, int((ctx.fetch_refined()['rounds'] >= 0).sum())


cut = float(np.quantile(clr[iA >= 0], Q))
ctx.refine_at_peaks(True)
ctx.peaks(SEPS[-1])
after_scan(cut)             # warm-up of the three kernels on a few windows
print('windows with CLR >= %.4g (the %g quantile), R = %d replicates, blocks of 1 site:' % (cut, Q, REPS))
ctx.refine_at_peaks(False)
(t_ref, t_sup, t_boot), done0 = after_scan(cut)
total0 = t_ref + t_sup + t_boot
print('  every window       : %6d windows  refine %9.1f ms  support %9.1f ms  boot %10.1f ms  total %10.1f ms' % (done0, t_ref, t_sup, t_boot, total0),
      flush=True)
ctx.refine_at_peaks(True)
for G in SEPS:
    ctx.peaks(G)
    (t_ref, t_sup, t_boot), done = after_scan(cut)
    total = t_ref + t_sup + t_boot
    print('  --atPeaks, G = %-5g: %6d windows  refine %9.1f ms  support %9.1f ms  boot %10.1f ms  total %10.1f ms  = 1/%.0f of the time for 1/%.0f of the windows'
          % (G, done, t_ref, t_sup, t_boot, total, total0 / total, done0 / max(done, 1)), flush=True)
ctx.close()
asm = os.path.join(ROOT, 'ballermixplus_amd', 'csrc', 'bmxscan.gfx950.s')
if os.path.exists(asm):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'kernel_resources.py')], capture_output=True, text=True).stdout
    print('\n'.join(l for l in out.splitlines() if l.startswith('kernel') or 'peak' in l or 'refine_init' in l))
