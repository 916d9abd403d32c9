"""Cost of --surfaces on the synthetic 1M-SNP chromosome of refine_timing.py (n = 100, default grid: 31 x 10 x 51 = 15 810 grid
points per window, every site a test site), for the apex windows of --peaks 0.01 among the top 1 % of the CLR.
Writes profiles/surfaces_timing.txt:
  - the scan's kernel time (last_scan_ms) and the number of selected windows;
  - bmx_ctx_surfaces_ms of ONE call over all of them (HIP events around its kernels; the median of R calls after a warm-up
    call) and the wall time of that call, per call and per window;
  - the baseline, the only way before bmx_ctx_surfaces: a loop of bmx_ctx_surface over 20 of the same windows (evenly
    spaced among them), wall time per window (the call blocks; the median of R loops after a warm-up loop);
  - the ratio of the two per-window times -- the run FAILS (exit status 1) unless the batched one is lower -- and whether
    the 20 windows agree bitwise;
  - the end-to-end time of surfaces.surfaces_and_write (selection, surfaces, formatting and the file) and the file's size;
  - surfaces_kernel's registers, LDS and scratch from `make -C ballermixplus_amd/csrc probe K=surfaces_kernel` (or from a
    saved copy of that command's output given with --probe FILE); scratch must be 0.
Every step that uses the GPU is a child process of its own under its own time limit; the first step that fails, faults or
runs out of time ends the run, and nothing more is started.
Usage: python scripts/surfaces_timing.py [N] [R] [--probe FILE]"""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

G, Q, LOOP = 0.01, 0.99, 20
LIMITS = {'kernels': 420, 'file': 420}        # seconds per GPU step


def setup(N):
    """The scanned chromosome and its selected windows: (ctx, gen, test sites, grids holder, cut, apex rows)."""
    import numpy as np
    from ballermixplus_amd import engine, scan as scanmod, synth
    from ballermixplus_amd.hostmodel import Grids
    phys, gen, k, nn = synth.synth_chromosome(N, 100, 1)
    xs, ab, As = Grids(None, None, False, False, None, None).scan_order()
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
    clr, _, _, iA, _ = ctx.fetch()
    cut = float(np.quantile(clr, Q))
    pk = ctx.peaks(G, cut)
    ts = scanmod.TestSites()
    ts.add_many(phys, gen, gen, np.zeros(N, np.int64), np.full(N, N - 1, np.int64))

    class Sel:
        grid_x, grid_abeta, grid_A = xs, ab, As
    return ctx, gen, ts, Sel, cut, pk['row']


def step_kernels(N, R):
    import numpy as np
    from ballermixplus_amd import surfaces
    ctx, gen, ts, Sel, cut, apex = setup(N)
    out = {'scan_ms': ctx.last_scan_ms(), 'M': len(gen), 'cut': cut, 'apexes': len(apex)}
    clr, _, _, iA, _ = ctx.fetch()
    rows, dropped = surfaces.select(clr, iA, cut, apex, 1 << 30)
    out['windows'] = len(rows)
    ctx.surfaces(rows)
    ms, wall = [], []
    for _ in range(R):
        t0 = time.perf_counter()
        T, ns = ctx.surfaces(rows)
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(ctx.surfaces_ms())
    out.update(batch_ms=float(np.median(ms)), batch_ms_min=min(ms), batch_ms_max=max(ms), batch_wall_ms=float(np.median(wall)))
    some = np.unique(np.linspace(0, len(rows) - 1, min(LOOP, len(rows))).astype(np.int64))
    loop = []
    for r in range(R + 1):
        t0 = time.perf_counter()
        one = [ctx.surface(gen[rows[j]], 0, N - 1) for j in some]
        loop.append((time.perf_counter() - t0) * 1e3 / len(some))
    out.update(loop_windows=len(some), loop_ms_per_window=float(np.median(loop[1:])), loop_min=min(loop[1:]), loop_max=max(loop[1:]))
    out['bitwise'] = all(np.array_equal(T[j], one[i][0], equal_nan=True) and np.array_equal(ns[j], one[i][1]) for i, j in enumerate(some))
    out['mean_sites_at_smallest_A'] = float(ns.max(axis=1).mean())
    ctx.close()
    print('RESULT ' + json.dumps(out), flush=True)


def step_file(N, R):
    from ballermixplus_amd import surfaces
    ctx, gen, ts, Sel, cut, apex = setup(N)
    with tempfile.TemporaryDirectory() as d:
        outfile = os.path.join(d, 'chr.out.txt')
        t0 = time.perf_counter()
        n, dropped = surfaces.surfaces_and_write(ctx, outfile, ts, Sel, cut, 1 << 30, apex)
        wall = (time.perf_counter() - t0) * 1e3
        size = os.path.getsize(surfaces.output_name(outfile))
    out = {'windows': n, 'file_wall_ms': wall, 'file_bytes': size, 'kernel_ms': ctx.surfaces_ms()}
    ctx.close()
    print('RESULT ' + json.dumps(out), flush=True)


def resources(saved):
    """surfaces_kernel's lines of `make probe K=surfaces_kernel`: {'VGPRs': .., 'LDS': .., 'Scratch': .., ...}."""
    if saved:
        text = open(saved).read()
    else:
        text = subprocess.run(['make', '-C', os.path.join(ROOT, 'ballermixplus_amd', 'csrc'), 'probe', 'K=surfaces_kernel'],
                              capture_output=True, text=True, timeout=900).stdout
    res = {}
    for key, pat in (('VGPRs', r' VGPRs: (\d+)'), ('SGPRs', r'TotalSGPRs: (\d+)'), ('Scratch', r'ScratchSize \[bytes/lane\]: (\d+)'),
                     ('VGPR spill', r'VGPRs Spill: (\d+)'), ('SGPR spill', r'SGPRs Spill: (\d+)'),
                     ('Occupancy', r'Occupancy \[waves/SIMD\]: (\d+)'), ('LDS', r'LDS Size \[bytes/block\]: (\d+)')):
        m = re.search(pat, text)
        if m:
            res[key] = int(m.group(1))
    return res


def child(step, N, R):
    """One GPU step in a process of its own under its time limit: its RESULT, or None (failed: the run ends)."""
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step, str(N), str(R)], capture_output=True, text=True,
                           timeout=LIMITS[step], cwd=ROOT)
    except subprocess.TimeoutExpired:
        print('step %s ran out of its %d s: nothing more is started' % (step, LIMITS[step]))
        return None
    got = [l for l in r.stdout.splitlines() if l.startswith('RESULT ')]
    if r.returncode != 0 or not got:
        print('step %s failed (exit status %d): nothing more is started\n%s' % (step, r.returncode, (r.stdout + r.stderr)[-2000:]))
        return None
    return json.loads(got[-1][7:])


def main(argv):
    if argv[:1] == ['--step']:
        return {'kernels': step_kernels, 'file': step_file}[argv[1]](int(argv[2]), int(argv[3]))
    saved = None
    if '--probe' in argv:
        i = argv.index('--probe')
        saved = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    N = int(argv[0]) if len(argv) > 0 else 1000000
    R = int(argv[1]) if len(argv) > 1 else 5
    k = child('kernels', N, R)
    if k is None:
        sys.exit(1)
    f = child('file', N, R)
    if f is None:
        sys.exit(1)
    res = resources(saved)
    W = max(k['windows'], 1)
    per_kernel, per_wall = k['batch_ms'] / W, k['batch_wall_ms'] / W
    lines = [
        'surfaces_timing.py %d %d: synthetic chromosome of %d sites (n = 100), default grid, every site a test site' % (N, R, N),
        'scan kernels %.2f ms for M = %d windows' % (k['scan_ms'], k['M']),
        'selected: the apexes of --peaks %g with CLR >= %.4g (the %g quantile): %d windows (%.0f sites in the widest window on average)'
        % (G, k['cut'], Q, k['windows'], k['mean_sites_at_smallest_A']),
        'bmx_ctx_surfaces, one call over the %d windows: kernels %.2f ms (min %.2f, max %.2f; bmx_ctx_surfaces_ms, median of %d calls), '
        'wall %.2f ms with the copy to the host' % (k['windows'], k['batch_ms'], k['batch_ms_min'], k['batch_ms_max'], R, k['batch_wall_ms']),
        '  per window: kernels %.4f ms, wall %.4f ms' % (per_kernel, per_wall),
        'baseline, a loop of bmx_ctx_surface over %d of these windows: wall %.3f ms per window (min %.3f, max %.3f; median of %d loops)'
        % (k['loop_windows'], k['loop_ms_per_window'], k['loop_min'], k['loop_max'], R),
        'ratio loop / batched per window: %.1f (wall against wall), %.1f (loop wall against batched kernels)'
        % (k['loop_ms_per_window'] / per_wall, k['loop_ms_per_window'] / per_kernel),
        'the %d windows of the loop bitwise equal to the batched call: %s' % (k['loop_windows'], 'yes' if k['bitwise'] else 'NO'),
        'end to end (selection, surfaces, formatting, <out>.surfaces.txt of %d windows, %.1f MB): %.0f ms, of which kernels %.2f ms'
        % (f['windows'], f['file_bytes'] / 1e6, f['file_wall_ms'], f['kernel_ms']),
        'surfaces_kernel (make probe K=surfaces_kernel): ' + ', '.join('%s %d' % kv for kv in res.items()),
    ]
    ok = per_wall < k['loop_ms_per_window'] and k['bitwise'] and res.get('Scratch') == 0
    lines.append('requirement (batched per-window time below the loop\'s, bitwise equal, scratch 0): %s' % ('met' if ok else 'NOT MET'))
    text = '\n'.join(lines) + '\n'
    with open(os.path.join(ROOT, 'profiles', 'surfaces_timing.txt'), 'w') as fh:
        fh.write(text)
    print(text, end='')
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main(sys.argv[1:])
