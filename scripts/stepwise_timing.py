"""Cost of --stepwise on the workload of surfaces_timing.py: the synthetic 1M-SNP chromosome (n = 100, default grid, every site a
test site) and the apexes of --peaks 0.01 among the top 1 % of the CLR, selected forward at C = that 0.99 quantile.  Writes
profiles/stepwise_timing.txt and profiles/stepwise_kernel_resources.txt (or --out FILE, --resources FILE):
  - the whole selection (stepwise.device_run: baseline_reset, then per step one baseline_add and one base_surfaces over the affected
    apexes), wall time, the median of R runs after a warm-up run, with the loci accepted and the surfaces computed;
  - per step: the wall time of bmx_ctx_baseline_add (the call blocks) and bmx_ctx_base_surfaces_ms of the step's call, medians over
    the steps of the last run; the first call over all apexes apart;
  - next to it, in the same process: bmx_ctx_base_surfaces and bmx_ctx_cond_surfaces (each apex given the next at its scan argmax)
    of the same list without T, bmx_ctx_*_ms, the median of R calls after a warm-up call;
  - the host route: fetch_sites + fetch_lut + stepwise.host_base_surface / host_baseline_add (numpy, one thread), timed on HAND
    windows and loci spread over the list, scaled to the run's counts; the largest difference to the device on them;
  - both kernels' registers, LDS and scratch from the compiler's resource remarks (or a saved copy: --probe FILE).
The GPU work is one child process under a time limit; if it fails, faults or runs out of time nothing more is started.
Usage: python scripts/stepwise_timing.py [N] [R] [--probe FILE] [--out FILE] [--resources FILE]"""
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
REL_TOL = 1e-9      # tests/stepcases.py REL_TOL


def step_kernels(N, R):
    import numpy as np
    import surfaces_timing
    from ballermixplus_amd import stepwise
    ctx, gen, ts, Sel, cut, apex = surfaces_timing.setup(N)
    clr, ix, ia, iA, _ = ctx.fetch()
    m = ctx.model
    nx, nab = len(m.x), len(m.abeta)
    lin = ((iA.astype(np.int64) * nx + ix) * nab + ia).astype(np.int32)
    zcut = float(ctx._L.bmx_alpha_cut())
    t = np.asarray(apex, dtype=np.int32)
    K = len(t)
    A = np.array([float(v) for v in Sel.grid_A])
    out = {'M': len(gen), 'cut': cut, 'apexes': K}
    t0 = time.perf_counter()
    ranges = stepwise.site_ranges(gen, gen[t], np.zeros(K, np.int64), np.full(K, N - 1, np.int64), float(A.min()), zcut)
    out['ranges_ms'] = (time.perf_counter() - t0) * 1e3

    log = {}
    real_add, real_base = ctx.baseline_add, ctx.base_surfaces

    def add(test, lin_):
        t0 = time.perf_counter()
        w = real_add(test, lin_)
        log['add'].append((time.perf_counter() - t0) * 1e3)
        return w

    def base(tests, want_T=True):
        r = real_base(tests, want_T=want_T)
        log['base'].append((len(tests), ctx.base_surfaces_ms()))
        return r

    ctx.baseline_add, ctx.base_surfaces = add, base
    walls = []
    for rep in range(R + 1):                    # (the first run is the warm-up)
        log['add'], log['base'] = [], []
        t0 = time.perf_counter()
        run = stepwise.device_run(ctx, t, ranges, cut, max_loci=K)
        walls.append((time.perf_counter() - t0) * 1e3)
    ctx.baseline_add, ctx.base_surfaces = real_add, real_base
    walls = walls[1:]
    steps = log['base'][1:]
    out.update(run_ms=float(np.median(walls)), run_min=min(walls), run_max=max(walls), accepted=len(run['order']), evals=int(run['evals']),
               total=float(run['T_total'][run['order'][-1]]) if run['order'] else 0.0,
               first_ms=log['base'][0][1], add_ms=float(np.median(log['add'])) if log['add'] else 0.0,
               add_max=max(log['add']) if log['add'] else 0.0, step_calls=len(steps),
               step_ms=float(np.median([s[1] for s in steps])) if steps else 0.0, step_max=max([s[1] for s in steps]) if steps else 0.0,
               step_windows=float(np.mean([s[0] for s in steps])) if steps else 0.0,
               step_sum=float(sum(s[1] for s in steps)), written=float(np.mean([w[2] for w in run['written']])) if run['written'] else 0.0)
    d_dev, cnt_dev = ctx.baseline_fetch(N)
    out['identity'] = 2.0 * float(np.sum(np.log1p(d_dev)))
    out['reached'] = int((cnt_dev > 0).sum())
    out['reached_twice'] = int((cnt_dev > 1).sum())

    def timed(call, read):
        call()
        ms = []
        for _ in range(R):
            call()
            ms.append(read())
        return float(np.median(ms)), min(ms), max(ms)

    # the same list in one call each, against the run's final baseline: base_surfaces, cond_surfaces (the next apex), surfaces
    out['base_ms'], out['base_min'], out['base_max'] = timed(lambda: ctx.base_surfaces(t, want_T=False), ctx.base_surfaces_ms)
    c = np.roll(t, -1)
    out['cond_ms'], out['cond_min'], out['cond_max'] = timed(lambda: ctx.cond_surfaces(t, c, lin[c], want_T=False), ctx.cond_surfaces_ms)
    # the host route on HAND windows and loci
    t0 = time.perf_counter()
    g_dev, rows_dev = ctx.fetch_sites(N)
    _, Rtab = ctx.fetch_lut()
    out['fetch_ms'] = (time.perf_counter() - t0) * 1e3
    per, per_add, worst, same = [], [], 0.0, True
    hand = np.unique(np.linspace(0, K - 1, HAND).astype(np.int64)).tolist()
    res = ctx.base_surfaces(t[hand])
    for j, q in enumerate(hand):
        t0 = time.perf_counter()
        Th, nh, sh, S = stepwise.host_base_surface(g_dev, rows_dev, Rtab, A, gen[t[q]], 0, N - 1, d_dev, cnt_dev, zcut, scale=True)
        per.append((time.perf_counter() - t0) * 1e3)
        same = bool(same and np.array_equal(nh, res['nsites'][j]) and np.array_equal(sh, res['nshared'][j])
                    and np.array_equal(np.isnan(Th), np.isnan(res['T'][j])))
        worst = max(worst, float(np.nanmax(np.abs(Th - res['T'][j]))) / (REL_TOL * float(S.max())))
        dh, ch = np.zeros(N), np.zeros(N, dtype=np.int32)
        l = int(lin[t[q]])
        t0 = time.perf_counter()
        stepwise.host_baseline_add(dh, ch, g_dev, rows_dev, Rtab, gen[t[q]], 0, N - 1, float(A[l // (nx * nab)]), (l // nab) % nx, l % nab, zcut)
        per_add.append((time.perf_counter() - t0) * 1e3)
    out.update(host_ms=float(np.median(per)), host_min=min(per), host_max=max(per), host_add_ms=float(np.median(per_add)), host_n=len(per),
               same_counts=same, worst=worst)
    ctx.close()
    print('RESULT ' + json.dumps(out), flush=True)


def main(argv):
    if argv[:1] == ['--step']:
        return step_kernels(int(argv[1]), int(argv[2]))
    from conditional_timing import resources
    opts = {}
    for flag in ('--probe', '--out', '--resources'):
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
    kernels = ('baseline_add_kernel', 'base_surfaces_kernel', 'cond_surfaces_kernel', 'surfaces_kernel')
    res = {name: resources(opts.get('--probe'), name) for name in kernels}
    K = k['apexes']
    host_s = (k['evals'] * k['host_ms'] + k['accepted'] * k['host_add_ms']) / 1e3
    lines = [
        'stepwise_timing.py %d %d: synthetic chromosome of %d sites (n = 100), default grid, every site a test site' % (N, R, N),
        'apexes: those of --peaks 0.01 with CLR >= %.4g (the 0.99 quantile): %d; C = the same value; no cap on the loci' % (k['cut'], K),
        'the whole selection (baseline_reset, then per step one baseline_add and one base_surfaces over the affected apexes, no surface '
        'copied back): wall %.1f ms (min %.1f, max %.1f; median of %d runs after a warm-up run); %d loci accepted, %d surfaces computed '
        '(%d + %.1f per step on average), %.0f sites written per locus; stepwise.site_ranges of the apexes on the host, once: %.1f ms'
        % (k['run_ms'], k['run_min'], k['run_max'], R, k['accepted'], k['evals'], K, k['step_windows'], k['written'], k['ranges_ms']),
        '  T_total %r; 2 sum log1p(d) on the fetched baseline %r; %d sites reached by a locus, %d by more than one'
        % (k['total'], k['identity'], k['reached'], k['reached_twice']),
        'per step (the last run): bmx_ctx_baseline_add %.3f ms wall (median over the steps, max %.3f; launch, copy of three numbers, '
        'synchronise); bmx_ctx_base_surfaces_ms %.3f ms (median over the %d steps with an affected apex, max %.3f; their sum %.1f ms); '
        'the first call over all %d apexes: %.2f ms' % (k['add_ms'], k['add_max'], k['step_ms'], k['step_calls'], k['step_max'], k['step_sum'], K,
                                                       k['first_ms']),
        'next to it, one call over the same %d windows without T, against the final baseline, in the same process (kernels, median of %d '
        'calls after a warm-up call): bmx_ctx_base_surfaces %.2f ms (min %.2f, max %.2f); bmx_ctx_cond_surfaces (each apex given the next at '
        'its scan argmax) %.2f ms (min %.2f, max %.2f); base_surfaces / cond_surfaces = %.3f'
        % (K, R, k['base_ms'], k['base_min'], k['base_max'], k['cond_ms'], k['cond_min'], k['cond_max'], k['base_ms'] / k['cond_ms']),
        'the host route: fetch_sites + fetch_lut (%.0f ms once), stepwise.host_base_surface %.0f ms per window (min %.0f, max %.0f; numpy, one '
        'thread, median of %d windows spread over the list) and host_baseline_add %.1f ms per locus; the run\'s %d surfaces and %d loci: '
        '%.0f s, %.0f times the selection\'s wall time' % (k['fetch_ms'], k['host_ms'], k['host_min'], k['host_max'], k['host_n'],
                                                           k['host_add_ms'], k['evals'], k['accepted'], host_s, host_s * 1e3 / k['run_ms']),
        '  on those windows nsites, nshared and the NaN pattern equal the host\'s: %s; largest |T device - T host| = %.2g of the tests\' '
        'tolerance (1e-9 * max over the grid of 2 sum |term|)' % ('yes' if k['same_counts'] else 'NO', k['worst'])]
    rlines = ['%-22s (kernel-resource-usage remarks): ' % name + ', '.join('%s %d' % kv for kv in res[name].items()) for name in kernels]
    ok = all(res[n].get('Scratch') == 0 for n in kernels[:2]) and k['same_counts'] and k['worst'] <= 1.0
    lines.append('requirement (scratch 0 in both kernels, counts equal, T within the tolerance): %s' % ('met' if ok else 'NOT MET'))
    text = '\n'.join(lines) + '\n'
    with open(opts.get('--out') or os.path.join(ROOT, 'profiles', 'stepwise_timing.txt'), 'w') as fh:
        fh.write(text)
    with open(opts.get('--resources') or os.path.join(ROOT, 'profiles', 'stepwise_kernel_resources.txt'), 'w') as fh:
        fh.write('\n'.join(rlines) + '\n')
    print(text + '\n'.join(rlines))
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main(sys.argv[1:])
