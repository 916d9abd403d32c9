"""Cost of the profile likelihoods (--profiles) against the plain scan, on the synthetic 1M-SNP chromosome of BASELINE config 3
(n = 100, default grid): every site a test site (clr_scan_prepared_kernel<16,true>), every 4th site (<8,true>) and every 16th
site (solo plan); then the same chromosome with 31 sample sizes n = 70..100 (missing data: the table is read from L2), every site
and every 4th site (<16,false>, <8,false>).  Scan kernel time with profiles off, A only, x + abeta and all three, alternated within this process, median of R rounds; then the
kernels' registers and spills from the assembly (`make -C ballermixplus_amd/csrc asm` first, or they are skipped).
Usage: python scripts/profile_timing.py [N] [R]"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from ballermixplus_amd import engine, synth  # noqa: E402
from ballermixplus_amd.hostmodel import Grids  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
R = int(sys.argv[2]) if len(sys.argv) > 2 else 7
phys, gen, k0, n0 = synth.synth_chromosome(N, 100, 1)
xs, ab, As = Grids(None, None, False, False, None, None).scan_order()
SETS = (('off', 0), ('A', 1), ('x+abeta', 6), ('all', 7))


def context(k, nn):
    sizes = sorted(set(nn.tolist()))
    sp = {(a, b): f for a, b, f in synth.spect_from_counts(k, nn)}
    props = {s_: float(sum(f for (a, b), f in sp.items() if b == s_)) for s_ in sizes}
    model = engine.ModelArrays('B2', int(k.min()), sizes, sp, props, xs, ab)
    c = engine.Context(0)
    c.set_model(model, As)
    c.set_sites(gen, model.rows_of(k, nn))
    return c


n2 = np.random.default_rng(5).integers(70, 101, N)
k2 = np.where(k0 == n0, n2, np.maximum(1, np.minimum(n2 - 1, (k0 * n2) // n0)))
CASES = (('1 size, every site', (k0, n0), 1), ('1 size, every 4th site', (k0, n0), 4), ('1 size, every 16th site', (k0, n0), 16),
         ('31 sizes, every site', (k2, n2), 1), ('31 sizes, every 4th site', (k2, n2), 4))
ctx, cur = None, None
for label, kn, step in CASES:
    if cur is not kn:
        if ctx is not None:
            ctx.close()
        ctx, cur = context(*kn), kn
    tg = gen[::step]
    ctx.set_tests(tg)
    ms = {s: [] for s, _ in SETS}
    for r in range(R + 1):
        for s, w in SETS:
            ctx.set_profiles(w)
            ctx.scan()                  # (a changed profile set re-plans: the first scan after a switch includes that)
            ctx.sync()
            ctx.scan()
            ctx.sync()
            if r:
                ms[s].append(ctx.last_scan_ms())
    ctx.set_profiles(0)
    ctx.scan()
    plan = ctx.plan()['kernel']
    base = np.median(ms['off'])
    print('%s: M = %d test sites, plan %s, scan kernels (median of %d):' % (label, len(tg), plan, R))
    for s, _ in SETS:
        print('  profiles %-8s %8.2f ms  x%.3f' % (s, np.median(ms[s]), np.median(ms[s]) / base))
ctx.close()
asm = os.path.join(ROOT, 'ballermixplus_amd', 'csrc', 'bmxscan.gfx950.s')
if os.path.exists(asm):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'kernel_resources.py')], capture_output=True, text=True).stdout
    print('\n'.join(l for l in out.splitlines() if l.startswith('kernel') or 'clr_scan_prepared' in l or 'clr_scan_solo' in l
                    or 'finalize' in l))
