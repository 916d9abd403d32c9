"""Cost of --sandwich on the workload of surfaces_timing.py: the synthetic 1M-SNP chromosome (n = 100, default grid, every site a
test site) and the apex windows of --peaks 0.01 among the top 1 % of the CLR, each at its refined point.  Writes
profiles/sandwich_timing.txt (or --out FILE):
  - bmx_ctx_refine restricted to those apexes (bmx_ctx_refine_at_peaks), wall time of the call to the end of its kernels, and the
    rounds it took per window: the yardstick `one compass round per window`;
  - bmx_ctx_sandwich_ms of one call over the windows at B = 1 and at B = 64, the median of R calls after a warm-up call, with the
    spread and the wall time of the call with the copies;
  - bmx_ctx_boot with 100 replicates of the same windows in the same process (B = 1), wall time to the end of its kernels;
  - the only way there was before: fetch_sites, five Context.refine_R columns and sandwich.host_sandwich per window on the host
    (numpy), timed on HAND windows spread over the list, with the largest difference to the device on them in units of the tests'
    tolerance (T 1e-12 relative; g, H, J 1e-12 of the sum of the absolute terms).
The GPU work is one child process under a time limit; if it fails, faults or runs out of time nothing more is started.
Usage: python scripts/sandwich_timing.py [N] [R] [--out FILE]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

LIMIT = 540         # seconds for the GPU step
HAND = 5
TOL = 1e-12
BOOT_R = 100


def step_kernels(N, R):
    import numpy as np
    import surfaces_timing
    from ballermixplus_amd import sandwich, surfaces
    ctx, gen, ts, Sel, cut, apex = surfaces_timing.setup(N)
    clr, ix, ia, iA, _ = ctx.fetch()
    rows, dropped = surfaces.select(clr, iA, cut, apex, 1 << 30)
    zcut = float(ctx._L.bmx_alpha_cut())
    out = {'M': len(gen), 'cut': cut, 'windows': len(rows)}

    def walled(call):
        ctx.sync()
        t0 = time.perf_counter()
        call()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3

    ctx.refine_at_peaks(True)
    walled(lambda: ctx.refine(cut))
    out['refine_ms'] = float(np.median([walled(lambda: ctx.refine(cut)) for _ in range(3)]))
    ref = ctx.fetch_refined()
    done = np.nonzero(ref['rounds'] >= 0)[0]
    assert np.array_equal(done, rows)
    out['rounds'] = float(ref['rounds'][rows].mean())
    A, x, ab = ref['A'][rows], ref['x'][rows], ref['abeta'][rows]
    t = rows.astype(np.int32)
    for B in (1, 64):
        call = lambda: ctx.sandwich(t, A, x, ab, B)
        res = call()
        ms, wall = [], []
        for _ in range(R):
            t0 = time.perf_counter()
            res = call()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(ctx.sandwich_ms())
        out['sw%d' % B] = [float(np.median(ms)), min(ms), max(ms), float(np.median(wall))]
        out['blocks%d' % B] = float(res['nblocks'].mean())
    out['mean_sites'] = float(res['nsites'].mean())
    out['skipped'] = int(res['nskipped'].sum())
    keys = np.arange(1, BOOT_R + 1, dtype=np.uint64)
    out['boot_ms'] = walled(lambda: ctx.boot(keys, 1, cut))
    boot = ctx.fetch_boot()
    out['boot_tasks'] = int(len(boot['rounds'].reshape(-1))) if isinstance(boot, dict) else BOOT_R * len(rows)
    # the host route on a few windows
    t0 = time.perf_counter()
    g_dev, rows_dev = ctx.fetch_sites(N)
    out['fetch_ms'] = (time.perf_counter() - t0) * 1e3
    per, worst, same = [], 0.0, True
    for q in np.unique(np.linspace(0, len(t) - 1, HAND).astype(np.int64)).tolist():
        t0 = time.perf_counter()
        tabs = np.array([ctx.refine_R(xx, aa) for xx, aa in sandwich.shifted_points(x[q], ab[q])])
        h = sandwich.host_sandwich(g_dev, rows_dev, tabs, A[q], gen[t[q]], 0, N - 1, 64, zcut=zcut)
        per.append((time.perf_counter() - t0) * 1e3)
        same = bool(same and (h['nsites'], h['nskipped'], h['nblocks']) == (res['nsites'][q], res['nskipped'][q], res['nblocks'][q]))
        for k in ('g', 'H', 'J'):
            worst = max(worst, float(np.max(np.abs(res[k][q] - h[k]) / (TOL * h['abs' + k] + 1e-300))))
        worst = max(worst, abs(res['T'][q] - h['T']) / (TOL * abs(h['T'])))
    out.update(host_ms=float(np.median(per)), host_min=min(per), host_max=max(per), host_windows=len(per), same_counts=same, worst=worst)
    ctx.close()
    print('RESULT ' + json.dumps(out), flush=True)


def main(argv):
    if argv[:1] == ['--step']:
        return step_kernels(int(argv[1]), int(argv[2]))
    opts = {}
    if '--out' in argv:
        i = argv.index('--out')
        opts['--out'] = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    N = int(argv[0]) if len(argv) > 0 else 1000000
    R = int(argv[1]) if len(argv) > 1 else 7
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', str(N), str(R)], capture_output=True, text=True,
                           timeout=LIMIT, cwd=ROOT)
    except subprocess.TimeoutExpired:
        print('the GPU step ran out of its %d s: nothing more is started' % LIMIT)
        sys.exit(1)
    got = [l for l in p.stdout.splitlines() if l.startswith('RESULT ')]
    if p.returncode != 0 or not got:
        print('the GPU step failed (exit status %d): nothing more is started\n%s' % (p.returncode, (p.stdout + p.stderr)[-2000:]))
        sys.exit(1)
    k = json.loads(got[-1][7:])
    W = k['windows']
    per_round = k['refine_ms'] / max(k['rounds'], 1e-9)
    lines = [
        'sandwich_timing.py %d %d: synthetic chromosome of %d sites (n = 100), default grid, every site a test site' % (N, R, N),
        'windows: the apexes of --peaks 0.01 with CLR >= %.4g (the 0.99 quantile): %d windows, each at its refined point (%.0f sites per '
        'window at that A on average, %d skipped in all)' % (k['cut'], W, k['mean_sites'], k['skipped']),
        'bmx_ctx_refine of those windows (bmx_ctx_refine_at_peaks): %.2f ms wall to the end of its kernels (median of 3 calls after a warm-up), '
        '%.1f rounds per window: %.2f ms per round of the list' % (k['refine_ms'], k['rounds'], per_round)]
    for B in (1, 64):
        ms, lo, hi, wall = k['sw%d' % B]
        lines.append('bmx_ctx_sandwich, one call over the %d windows, B = %2d: kernels %.2f ms (min %.2f, max %.2f; bmx_ctx_sandwich_ms, median '
                     'of %d calls after a warm-up call), wall %.1f ms with the copies; %.1f blocks per window; %.2f compass rounds of the list'
                     % (W, B, ms, lo, hi, R, wall, k['blocks%d' % B], ms / per_round))
    lines += [
        'bmx_ctx_boot of the same windows, %d replicates, B = 1 (%d tasks): %.0f ms wall to the end of its kernels = %.0f times the sandwich call at '
        'B = 1' % (BOOT_R, k['boot_tasks'], k['boot_ms'], k['boot_ms'] / k['sw1'][0]),
        'before: fetch_sites (%.0f ms once), five refine_R columns and sandwich.host_sandwich per window on the host (numpy, one thread), B = 64: '
        '%.1f ms per window (min %.1f, max %.1f; median of %d windows spread over the list); the %d windows: %.1f s, %.0f times the call\'s wall time'
        % (k['fetch_ms'], k['host_ms'], k['host_min'], k['host_max'], k['host_windows'], W, k['host_ms'] * W / 1e3, k['host_ms'] * W / k['sw64'][3]),
        '  on those windows the three counts equal the host\'s: %s; largest |device - host| over T, g, H, J = %.2g of the tests\' tolerance '
        '(T: 1e-12 relative; g, H, J: 1e-12 of the sum of the absolute terms)' % ('yes' if k['same_counts'] else 'NO', k['worst'])]
    ok = k['same_counts'] and k['worst'] <= 1.0
    lines.append('requirement (counts equal, sums within the tolerance): %s' % ('met' if ok else 'NOT MET'))
    text = '\n'.join(lines) + '\n'
    with open(opts.get('--out') or os.path.join(ROOT, 'profiles', 'sandwich_timing.txt'), 'w') as fh:
        fh.write(text)
    print(text, end='')
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main(sys.argv[1:])
