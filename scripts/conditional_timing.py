"""Cost of --conditional on the workload of surfaces_timing.py: the synthetic 1M-SNP chromosome (n = 100, default grid, every site a
test site) and the apex windows of --peaks 0.01 among the top 1 % of the CLR, every window given the NEXT apex of the list (the
first for the last) held at its scan argmax.  Writes profiles/conditional_timing.txt (or --out FILE):
  - bmx_ctx_cond_surfaces_ms of one call over the pairs, the median of R calls after a warm-up call, with the spread and the wall
    time of the call with the copies; the same list with T_out = NULL (the CLI's form: maxima only);
  - bmx_ctx_surfaces_ms of one call over the same windows in the same process, the median of R calls after a warm-up call: the
    yardstick (the per-term work differs by one subtract);
  - the only way there was before: fetch_sites + fetch_lut + conditional.host_cond_surface per pair on the host (numpy), timed on
    HAND pairs spread over the list, with the largest difference to the device on them in units of the tests' tolerance;
  - cond_surfaces_kernel's and surfaces_kernel's registers, LDS and scratch from the compiler's resource remarks (or from a saved
    copy of them given with --probe FILE); scratch must be 0.
The GPU work is one child process under a time limit; if it fails, faults or runs out of time nothing more is started.
Usage: python scripts/conditional_timing.py [N] [R] [--probe FILE] [--out FILE]"""
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
HAND = 5
REL_TOL = 1e-9      # tests/condcases.py REL_TOL


def step_kernels(N, R):
    import numpy as np
    import surfaces_timing
    from ballermixplus_amd import conditional, surfaces
    ctx, gen, ts, Sel, cut, apex = surfaces_timing.setup(N)
    clr, ix, ia, iA, _ = ctx.fetch()
    rows, dropped = surfaces.select(clr, iA, cut, apex, 1 << 30)
    m = ctx.model
    nx, nab = len(m.x), len(m.abeta)
    lin = ((iA.astype(np.int64) * nx + ix) * nab + ia).astype(np.int32)
    zcut = float(ctx._L.bmx_alpha_cut())
    t = rows.astype(np.int32)
    c = np.roll(t, -1)
    cl = lin[c]
    out = {'M': len(gen), 'cut': cut, 'windows': len(rows)}

    def timed(call, read):
        call()
        ms, wall = [], []
        for _ in range(R):
            t0 = time.perf_counter()
            r = call()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(read())
        return r, float(np.median(ms)), min(ms), max(ms), float(np.median(wall))

    res, out['cond_ms'], out['cond_min'], out['cond_max'], out['cond_wall'] = timed(lambda: ctx.cond_surfaces(t, c, cl), ctx.cond_surfaces_ms)
    bare, out['bare_ms'], out['bare_min'], out['bare_max'], out['bare_wall'] = timed(lambda: ctx.cond_surfaces(t, c, cl, want_T=False),
                                                                                    ctx.cond_surfaces_ms)
    _, out['surf_ms'], out['surf_min'], out['surf_max'], out['surf_wall'] = timed(lambda: ctx.surfaces(t), ctx.surfaces_ms)
    own = res['nshared'][np.arange(len(t)), iA[t]]
    out.update(mean_sites=float(res['nsites'].max(axis=1).mean()), mean_shared=float(own.mean()), with_shared=int((own > 0).sum()),
               same_max=bool(np.array_equal(bare['tmax'].view(np.uint64), res['tmax'].view(np.uint64)) and np.array_equal(bare['lin'], res['lin'])))
    t0 = time.perf_counter()
    g_dev, rows_dev = ctx.fetch_sites(N)
    _, Rtab = ctx.fetch_lut()
    out['fetch_ms'] = (time.perf_counter() - t0) * 1e3
    per, worst, same = [], 0.0, True
    for q in np.unique(np.linspace(0, len(t) - 1, HAND).astype(np.int64)).tolist():
        a, p = int(cl[q]) // (nx * nab), int(cl[q]) % (nx * nab)
        t0 = time.perf_counter()
        Th, nh, sh, S = conditional.host_cond_surface(g_dev, rows_dev, Rtab, Sel.grid_A, gen[t[q]], 0, N - 1, gen[c[q]], 0, N - 1,
                                                      float(Sel.grid_A[a]), p // nab, p % nab, zcut, scale=True)
        per.append((time.perf_counter() - t0) * 1e3)
        same = bool(same and np.array_equal(nh, res['nsites'][q]) and np.array_equal(sh, res['nshared'][q])
                    and np.array_equal(np.isnan(Th), np.isnan(res['T'][q])))
        worst = max(worst, float(np.nanmax(np.abs(Th - res['T'][q]))) / (REL_TOL * float(S.max())))
    out.update(host_ms=float(np.median(per)), host_min=min(per), host_max=max(per), host_pairs=len(per), same_counts=same, worst=worst)
    ctx.close()
    print('RESULT ' + json.dumps(out), flush=True)


def resources(saved, kernel):
    """The named kernel's lines of the compiler's kernel-resource-usage remarks."""
    if saved:
        text = open(saved).read()
    else:
        src = os.path.join(ROOT, 'ballermixplus_amd', 'csrc')
        text = subprocess.run([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '-O3', '--offload-arch=gfx950', '-ffp-contract=off', '-std=c++17',
                               '-DBMX_SRC_HASH="probe"', '-S', '--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-o',
                               os.devnull, os.path.join(src, 'bmxscan.hip')], capture_output=True, text=True, timeout=1800).stderr
    mt = re.search(r'Function Name: \S*\d%sE' % kernel, text)
    at = mt.start() if mt else -1
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
    res, res0 = resources(opts.get('--probe'), 'cond_surfaces_kernel'), resources(opts.get('--probe'), 'surfaces_kernel')
    W = k['windows']
    lines = [
        'conditional_timing.py %d %d: synthetic chromosome of %d sites (n = 100), default grid, every site a test site' % (N, R, N),
        'pairs: the apexes of --peaks 0.01 with CLR >= %.4g (the 0.99 quantile), each given the next apex of the list at its scan argmax: '
        '%d pairs (%.0f sites per window at its widest A on average; %.1f shared at the window\'s own scan-argmax A, %d pairs share a site '
        'there)' % (k['cut'], W, k['mean_sites'], k['mean_shared'], k['with_shared']),
        'bmx_ctx_cond_surfaces, one call over the %d pairs: kernels %.2f ms (min %.2f, max %.2f; bmx_ctx_cond_surfaces_ms, median of %d '
        'calls after a warm-up call), wall %.1f ms with the copies' % (W, k['cond_ms'], k['cond_min'], k['cond_max'], R, k['cond_wall']),
        'the same list with T_out = NULL (maxima only, the CLI\'s form): kernels %.2f ms (min %.2f, max %.2f), wall %.1f ms; tmax and lin '
        'equal the full call\'s: %s' % (k['bare_ms'], k['bare_min'], k['bare_max'], k['bare_wall'], 'yes' if k['same_max'] else 'NO'),
        'bmx_ctx_surfaces, one call over the same windows in the same process: kernels %.2f ms (min %.2f, max %.2f; bmx_ctx_surfaces_ms, '
        'median of %d calls), wall %.1f ms; cond_surfaces / surfaces = %.3f (kernels), %.3f with T_out = NULL (the argmax kernel included)'
        % (k['surf_ms'], k['surf_min'], k['surf_max'], R, k['surf_wall'], k['cond_ms'] / k['surf_ms'], k['bare_ms'] / k['surf_ms']),
        'before: fetch_sites + fetch_lut (%.0f ms once) and conditional.host_cond_surface per pair on the host (numpy, one thread): %.0f ms '
        'per pair (min %.0f, max %.0f; median of %d pairs spread over the list); the %d pairs: %.0f s, %.0f times the call\'s wall time'
        % (k['fetch_ms'], k['host_ms'], k['host_min'], k['host_max'], k['host_pairs'], W, k['host_ms'] * W / 1e3,
           k['host_ms'] * W / k['cond_wall']),
        '  on those pairs nsites, nshared and the NaN pattern equal the host\'s: %s; largest |T device - T host| = %.2g of the tests\' '
        'tolerance (1e-9 * max over the grid of 2 sum |term|)' % ('yes' if k['same_counts'] else 'NO', k['worst']),
        'cond_surfaces_kernel (kernel-resource-usage remarks): ' + ', '.join('%s %d' % kv for kv in res.items()),
        'surfaces_kernel      (kernel-resource-usage remarks): ' + ', '.join('%s %d' % kv for kv in res0.items())]
    ok = res.get('Scratch') == 0 and k['same_counts'] and k['worst'] <= 1.0 and k['same_max']
    lines.append('requirement (scratch 0, counts equal, T within the tolerance, maxima equal without T): %s' % ('met' if ok else 'NOT MET'))
    text = '\n'.join(lines) + '\n'
    with open(opts.get('--out') or os.path.join(ROOT, 'profiles', 'conditional_timing.txt'), 'w') as fh:
        fh.write(text)
    print(text, end='')
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main(sys.argv[1:])
