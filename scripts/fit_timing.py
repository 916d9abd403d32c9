"""Cost of --fit on the workload of surfaces_timing.py and influence_timing.py: the synthetic 1M-SNP chromosome (n = 100, default
grid, every site a test site) and the apex windows of --peaks 0.01 among the top 1 % of the CLR.  Writes profiles/fit_timing.txt
(or --out FILE):
  - bmx_ctx_fit_ms of one call over the windows at the defaults (8 distance bins, 10 frequency classes, every window at its scan
    argmax), the median of R calls after a warm-up call, with the spread and the wall time of the call with the copies;
  - bmx_ctx_surfaces_ms of one call over the same windows in the same process, the median of R calls after a warm-up call;
  - the only way there was before: fit.host_fit per window on the host (numpy), timed on HAND windows spread over the list, with
    the largest difference between the device's table and the host's on them in units of the tests' tolerance;
  - fit_kernel's registers, LDS and scratch (the LDS form) from the compiler's resource remarks (or from a saved copy of them given
    with --probe FILE); scratch must be 0.
The GPU work is one child process under a time limit; if it fails, faults or runs out of time nothing more is started.
Usage: python scripts/fit_timing.py [N] [R] [--probe FILE] [--out FILE]"""
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

LIMIT = 540         # seconds for the GPU step
HAND = 9
TOL = 1e-12         # tests/fitcases.py TOL


def step_kernels(N, R):
    import numpy as np
    import surfaces_timing
    from ballermixplus_amd import fit, power, surfaces
    ctx, gen, ts, Sel, cut, apex = surfaces_timing.setup(N)
    clr, ix, ia, iA, _ = ctx.fetch()
    rows, dropped = surfaces.select(clr, iA, cut, apex, 1 << 30)
    m = ctx.model
    nx, nab = len(m.x), len(m.abeta)
    lin = ((iA.astype(np.int64) * nx + ix) * nab + ia)[rows].astype(np.int32)
    zcut = float(ctx._L.bmx_alpha_cut())
    gw = power.allowed_rows(m.stat, m.min_count, m.sizes, m.row_off, m.g)
    cls = fit.classes(m.stat, m.sizes, m.row_off, fit.CLASSES)
    edges = fit.default_edges(fit.BINS, zcut)
    out = {'scan_ms': ctx.last_scan_ms(), 'M': len(gen), 'cut': cut, 'windows': len(rows)}
    ctx.fit(rows, lin, gw, cls, fit.CLASSES, edges)
    ms, wall = [], []
    for _ in range(R):
        t0 = time.perf_counter()
        O, Es, En, sk = ctx.fit(rows, lin, gw, cls, fit.CLASSES, edges)
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(ctx.fit_ms())
    out.update(fit_ms=float(np.median(ms)), fit_min=min(ms), fit_max=max(ms), wall_ms=float(np.median(wall)),
               mean_sites=float(O.sum(axis=(1, 2)).mean()), skipped=int(sk.sum()))
    ctx.surfaces(rows)
    ms = []
    for _ in range(R):
        ctx.surfaces(rows)
        ms.append(ctx.surfaces_ms())
    out.update(surf_ms=float(np.median(ms)), surf_min=min(ms), surf_max=max(ms))
    _, Rtab = ctx.fetch_lut()
    _, rows_dev = ctx.fetch_sites(N)
    per, worst, same = [], 0.0, True
    for q in np.unique(np.linspace(0, len(rows) - 1, HAND).astype(np.int64)).tolist():
        t = int(rows[q])
        t0 = time.perf_counter()
        hO, hEs, hEn, hsk = fit.host_fit(gen, rows_dev, m.row_off, Rtab, gw, cls, fit.CLASSES, edges, Sel.grid_A[iA[t]], ix[t], ia[t],
                                         gen[t], 0, N - 1, zcut)
        per.append((time.perf_counter() - t0) * 1e3)
        same = bool(same and np.array_equal(hO, O[q]) and int(hsk) == int(sk[q]))
        bound = TOL * np.maximum(1, hO.sum(axis=1))[:, None]
        worst = max(worst, float(np.max(np.abs(hEs - Es[q]) / bound)), float(np.max(np.abs(hEn - En[q]) / bound)))
    out.update(host_ms=float(np.median(per)), host_min=min(per), host_max=max(per), host_windows=len(per), same_counts=same, worst=worst)
    ctx.close()
    print('RESULT ' + json.dumps(out), flush=True)


def resources(saved):
    """fit_kernel<true>'s lines of the compiler's kernel-resource-usage remarks."""
    if saved:
        text = open(saved).read()
    else:
        src = os.path.join(ROOT, 'ballermixplus_amd', 'csrc')
        text = subprocess.run([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '-O3', '--offload-arch=gfx950', '-ffp-contract=off', '-std=c++17',
                               '-DBMX_SRC_HASH="probe"', '-S', '--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-o',
                               os.devnull, os.path.join(src, 'bmxscan.hip')], capture_output=True, text=True, timeout=1800).stderr
    at = text.find('fit_kernelILb1E')
    text = text[at:text.find('Function Name', at + 1) if text.find('Function Name', at + 1) > 0 else len(text)] if at >= 0 else ''
    res = {}
    for key, pat in (('VGPRs', r' VGPRs: (\d+)'), ('SGPRs', r'TotalSGPRs: (\d+)'), ('Scratch', r'ScratchSize \[bytes/lane\]: (\d+)'),
                     ('VGPR spill', r'VGPRs Spill: (\d+)'), ('SGPR spill', r'SGPRs Spill: (\d+)'),
                     ('Occupancy', r'Occupancy \[waves/SIMD\]: (\d+)'), ('LDS', r'LDS Size \[bytes/block\]: (\d+)')):
        mt = re.search(pat, text)
        if mt:
            res[key] = int(mt.group(1))
    return res


def main(argv):
    if argv[:1] == ['--step']:
        return step_kernels(int(argv[1]), int(argv[2]))
    opts = {}
    for flag in ('--probe', '--out'):
        if flag in argv:
            i = argv.index(flag)
            opts[flag] = argv[i + 1]
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
    res = resources(opts.get('--probe'))
    W = k['windows']
    lines = [
        'fit_timing.py %d %d: synthetic chromosome of %d sites (n = 100), default grid, every site a test site' % (N, R, N),
        'selected: the apexes of --peaks 0.01 with CLR >= %.4g (the 0.99 quantile): %d windows, each at its scan argmax (%.0f qualifying '
        'sites per window on average, %d skipped)' % (k['cut'], W, k['mean_sites'], k['skipped']),
        'bmx_ctx_fit, 8 distance bins x 10 frequency classes, one call over the %d windows: kernel %.3f ms (min %.3f, max %.3f; '
        'bmx_ctx_fit_ms, median of %d calls after a warm-up call), wall %.2f ms with the copies; %.2f us per window'
        % (W, k['fit_ms'], k['fit_min'], k['fit_max'], R, k['wall_ms'], k['fit_ms'] * 1e3 / max(W, 1)),
        'bmx_ctx_surfaces, one call over the same windows in the same process: kernels %.2f ms (min %.2f, max %.2f; bmx_ctx_surfaces_ms, '
        'median of %d calls); the fit call costs %.4f of it' % (k['surf_ms'], k['surf_min'], k['surf_max'], R, k['fit_ms'] / k['surf_ms']),
        'before: fit.host_fit per window on the host (numpy, one thread): %.2f ms per window (min %.2f, max %.2f; median of %d windows '
        'spread over the list); the %d windows: %.0f ms, %.0f times the call\'s wall time'
        % (k['host_ms'], k['host_min'], k['host_max'], k['host_windows'], W, k['host_ms'] * W, k['host_ms'] * W / k['wall_ms']),
        '  on those windows O and nSkipped equal the host\'s: %s; largest |E device - E host| = %.3f of the tests\' tolerance (1e-12 * '
        'max(1, n_d) per cell)' % ('yes' if k['same_counts'] else 'NO', k['worst']),
        'fit_kernel<LDS> (kernel-resource-usage remarks): ' + ', '.join('%s %d' % kv for kv in res.items())]
    ok = res.get('Scratch') == 0 and k['same_counts'] and k['worst'] <= 1.0
    lines.append('requirement (scratch 0, counts equal, E within the tolerance): %s' % ('met' if ok else 'NOT MET'))
    text = '\n'.join(lines) + '\n'
    with open(opts.get('--out') or os.path.join(ROOT, 'profiles', 'fit_timing.txt'), 'w') as fh:
        fh.write(text)
    print(text, end='')
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main(sys.argv[1:])
