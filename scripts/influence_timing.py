"""Cost of --influence on the workload of surfaces_timing.py: the synthetic 1M-SNP chromosome (n = 100, default grid, every site a
test site) and the apex windows of --peaks 0.01 among the top 1 % of the CLR.  Writes profiles/influence_timing.txt (or --out FILE):
  - bmx_ctx_surfaces_ms of one call over the windows (the parent's code: the same number of log1p terms, once), the median of
    R calls after a warm-up call;
  - bmx_ctx_influence_ms of one call over the same windows in the same process at B = 1 and B = 64 (its kernels: the surfaces,
    the range search, the argmax and the blocks), the median of R calls after a warm-up call, the wall time of the call with
    the copies to the host, the number of blocks, and the ratio to the surfaces' time;
  - the only way there was before: per block one set_sites of the site array without the block (on a second slot), set_tests
    and ctx.surfaces of the window -- timed on 5 blocks of one window and extrapolated to every block of every window;
  - influence_kernel's registers, LDS and scratch from `make -C ballermixplus_amd/csrc probe K=influence_kernel` (or from a
    saved copy of that command's output given with --probe FILE); scratch must be 0.
The GPU work is one child process under a time limit; if it fails, faults or runs out of time nothing more is started.
Usage: python scripts/influence_timing.py [N] [R] [--probe FILE] [--out FILE]"""
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
BLOCKS = (1, 64)
HAND = 5


def step_kernels(N, R):
    import numpy as np
    import surfaces_timing
    from ballermixplus_amd import surfaces
    ctx, gen, ts, Sel, cut, apex = surfaces_timing.setup(N)
    clr, _, _, iA, _ = ctx.fetch()
    rows, dropped = surfaces.select(clr, iA, cut, apex, 1 << 30)
    out = {'scan_ms': ctx.last_scan_ms(), 'M': len(gen), 'cut': cut, 'windows': len(rows)}
    ctx.surfaces(rows)
    ms = []
    for _ in range(R):
        T, ns = ctx.surfaces(rows)
        ms.append(ctx.surfaces_ms())
    out.update(surf_ms=float(np.median(ms)), surf_min=min(ms), surf_max=max(ms), mean_sites=float(ns.max(axis=1).mean()))
    tmax = np.nanmax(np.where(np.isnan(T), -np.inf, T).reshape(len(rows), -1), axis=1)
    del T
    for B in BLOCKS:
        ctx.influence(rows, B)
        ms, wall = [], []
        for _ in range(R):
            t0 = time.perf_counter()
            r = ctx.influence(rows, B)
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(ctx.influence_ms())
        out['B%d' % B] = {'ms': float(np.median(ms)), 'min': min(ms), 'max': max(ms), 'wall_ms': float(np.median(wall)),
                          'blocks': int(r['offset'][-1]), 'own': int((r['m'] > 0).sum()),
                          'tmax_bitwise': bool(np.array_equal(r['T_max'], np.maximum(tmax, 0.0)))}
    # the previous alternative on one window of middling size
    sizes = r['offset'][1:] - r['offset'][:-1]
    q = int(np.argsort(sizes)[len(sizes) // 2])
    w = int(rows[q])
    _, rows_dev = ctx.fetch_sites(N)
    for B in BLOCKS:
        r = ctx.influence([w], B)
        own = np.nonzero(r['m'] > 0)[0]
        pick = own[np.unique(np.linspace(0, len(own) - 1, HAND).astype(np.int64))]
        ctx.select_slot(1)
        per, worst = [], 0.0
        for rep in range(2):            # the first pass also grows the slot's buffers
            for j in pick.tolist():
                b = int(r['first_block'][0]) + j
                t0 = time.perf_counter()
                keep = np.ones(N, dtype=bool)
                keep[b * B:(b + 1) * B] = False
                ctx.set_sites(gen[keep], rows_dev[keep])
                ctx.set_tests(gen[w:w + 1])
                Td, _ = ctx.surfaces([0])
                v = float(np.nanmax(np.where(Td > 0, Td, 0.0)))
                if rep:
                    per.append((time.perf_counter() - t0) * 1e3)
                    worst = max(worst, abs(v - float(r['L'][j])) / max(abs(v), 1e-300))
        ctx.select_slot(0)
        out['B%d' % B].update(hand_ms_per_block=float(np.median(per)), hand_blocks=len(pick), hand_rel_diff=worst)
    ctx.close()
    print('RESULT ' + json.dumps(out), flush=True)


def resources(saved):
    """influence_kernel's lines of `make probe K=influence_kernel`."""
    if saved:
        text = open(saved).read()
    else:
        text = subprocess.run(['make', '-C', os.path.join(ROOT, 'ballermixplus_amd', 'csrc'), 'probe', 'K=influence_kernel'],
                              capture_output=True, text=True, timeout=900).stdout
    res = {}
    for key, pat in (('VGPRs', r' VGPRs: (\d+)'), ('SGPRs', r'TotalSGPRs: (\d+)'), ('Scratch', r'ScratchSize \[bytes/lane\]: (\d+)'),
                     ('VGPR spill', r'VGPRs Spill: (\d+)'), ('SGPR spill', r'SGPRs Spill: (\d+)'),
                     ('Occupancy', r'Occupancy \[waves/SIMD\]: (\d+)'), ('LDS', r'LDS Size \[bytes/block\]: (\d+)')):
        m = re.search(pat, text)
        if m:
            res[key] = int(m.group(1))
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
    R = int(argv[1]) if len(argv) > 1 else 5
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
        'influence_timing.py %d %d: synthetic chromosome of %d sites (n = 100), default grid, every site a test site' % (N, R, N),
        'selected: the apexes of --peaks 0.01 with CLR >= %.4g (the 0.99 quantile): %d windows (%.0f sites in the widest window on average)'
        % (k['cut'], W, k['mean_sites']),
        'bmx_ctx_surfaces, one call over the %d windows: kernels %.2f ms (min %.2f, max %.2f; bmx_ctx_surfaces_ms, median of %d calls)'
        % (W, k['surf_ms'], k['surf_min'], k['surf_max'], R)]
    for B in BLOCKS:
        b = k['B%d' % B]
        lines += [
            'bmx_ctx_influence, B = %d, one call over the same windows in the same process: kernels %.2f ms (min %.2f, max %.2f; '
            'bmx_ctx_influence_ms, median of %d calls; the surfaces\' kernel is among them), wall %.2f ms with the copies to the host'
            % (B, b['ms'], b['min'], b['max'], R, b['wall_ms']),
            '  %d blocks in the windows\' ranges, %d of them with a qualifying site; %.4f ms per window, %.3f us per block; ratio to the '
            'surfaces\' kernel time %.2f; T_max bitwise the surfaces\' maximum: %s'
            % (b['blocks'], b['own'], b['ms'] / W, b['ms'] * 1e3 / max(b['blocks'], 1), b['ms'] / k['surf_ms'], 'yes' if b['tmax_bitwise'] else 'NO'),
            '  before: per block one set_sites of the array without it, set_tests and ctx.surfaces of the window: %.2f ms per block (wall, '
            'median of %d blocks of one window, largest relative difference to L_b %.1e); extrapolated to the %d blocks with a site: '
            '%.0f s, %.0f times the call\'s wall time'
            % (b['hand_ms_per_block'], b['hand_blocks'], b['hand_rel_diff'], b['own'], b['hand_ms_per_block'] * b['own'] / 1e3,
               b['hand_ms_per_block'] * b['own'] / b['wall_ms'])]
    lines.append('influence_kernel (make probe K=influence_kernel): ' + ', '.join('%s %d' % kv for kv in res.items()))
    ok = res.get('Scratch') == 0 and all(k['B%d' % B]['tmax_bitwise'] for B in BLOCKS)
    lines.append('requirement (scratch 0, T_max bitwise the surfaces\'): %s' % ('met' if ok else 'NOT MET'))
    text = '\n'.join(lines) + '\n'
    with open(opts.get('--out') or os.path.join(ROOT, 'profiles', 'influence_timing.txt'), 'w') as fh:
        fh.write(text)
    print(text, end='')
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main(sys.argv[1:])
