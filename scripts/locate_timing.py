"""Cost of --locate on the synthetic 1M-SNP chromosome of refine_timing.py (n = 100, default grid, every site a test site), for
the apexes of --peaks 0.01 among the top 1 % of the CLR, H = G, R replicates with blocks of B = 1 and B = 64 sites.
Writes profiles/locate_timing.txt, per B:
  - the mean wall milliseconds per replicate of resample (bmx_ctx_resample_sites), set_tests + plan, scan and accumulate, and
    their total, on the device path that locate.run_replicates drives;
  - the same loop with the replicate built on the host -- np.repeat of the chromosome by boot.site_weights, then set_sites
    (upload and validation pass) -- on the same box: the figure the device path is judged against;
  - whether the two paths give the same argmax rows and maxima (they must: bitwise);
  - the share of replicates with an empty resampled array (N' = 0) and of peaks with n_ok < R.
Every B is a child process of its own under its own time limit; the first that fails, faults or runs out of time ends the run,
and nothing more is started.
Usage: python scripts/locate_timing.py [N] [R]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

G, Q = 0.01, 0.99
BLOCKS = (1, 64)
LIMIT = 540                 # seconds per GPU step


def step(N, R, B):
    import numpy as np
    from ballermixplus_amd import boot, engine, locate, synth
    from ballermixplus_amd.hostmodel import Grids
    phys, gen, k, nn = synth.synth_chromosome(N, 100, 1)
    xs, ab, As = Grids(None, None, False, False, None, None).scan_order()
    sp = {(a, b): f for a, b, f in synth.spect_from_counts(k, nn)}
    model = engine.ModelArrays('B2', int(k.min()), [100], sp, {100: 1.0}, xs, ab)
    rows = model.rows_of(k, nn)
    ctx = engine.Context(0)
    ctx.set_model(model, As)
    ctx.set_sites(gen, rows)
    ctx.set_tests(gen)
    ctx.scan()
    ctx.sync()
    ctx.scan()                  # (the first scan of a process also loads the code objects)
    ctx.sync()
    clr = ctx.fetch()[0]
    cut = float(np.quantile(clr, Q))
    pk = ctx.peaks(G, cut)
    union, lo, hi = locate.ranges(gen, pk['row'], G)
    tg = gen[union]
    keys = [locate.replicate_key(1, r, 0) for r in range(R)]
    out = {'B': B, 'R': R, 'scan_ms': ctx.last_scan_ms(), 'cut': cut, 'K': len(lo), 'union': len(union), 'M': len(gen)}
    now = time.perf_counter
    res = {}
    for path in ('device', 'host'):
        t = np.zeros(4)
        sizes = np.zeros(R, dtype=np.int64)
        ctx.select_slot(1)
        ctx.locate_begin(lo, hi, R)
        for r, key in enumerate(keys[:1] + keys):           # (replicate 0 once more in front: warm-up, not timed)
            warm = r == 0
            r = max(r - 1, 0)
            t0 = now()
            if path == 'device':
                n = ctx.resample_sites(0, key, B)
            else:
                w = boot.site_weights(key, len(gen), B)
                g2, r2 = np.repeat(gen, w), np.repeat(rows, w)
                n = len(g2)
                if n:
                    ctx.set_sites(g2, r2)
            t1 = now()
            sizes[r] = n
            if n == 0:
                continue
            ctx.set_tests(tg)
            t2 = now()
            ctx.scan()
            ctx.sync()
            t3 = now()
            if not warm:
                ctx.locate_accumulate(r)
                t4 = now()
                t += np.array([t1 - t0, t2 - t1, t3 - t2, t4 - t3]) * 1e3
        res[path] = ctx.fetch_locate()
        ctx.select_slot(0)
        out[path] = dict(zip(('resample', 'set_tests', 'scan', 'accumulate'), (t / R).tolist()), total=float(t.sum() / R))
        out[path + '_empty'] = int(np.count_nonzero(sizes == 0))
    out['same'] = bool(np.array_equal(res['device'][0], res['host'][0])
                       and np.array_equal(res['device'][1].view(np.uint64), res['host'][1].view(np.uint64)))
    out['peaks_short'] = int(np.count_nonzero((res['device'][0] >= 0).sum(axis=0) < R))
    ctx.close()
    print('RESULT ' + json.dumps(out), flush=True)


def child(N, R, B):
    """One B in a process of its own under its time limit: its RESULT, or None (failed: the run ends)."""
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', str(N), str(R), str(B)], capture_output=True,
                           text=True, timeout=LIMIT, cwd=ROOT)
    except subprocess.TimeoutExpired:
        print('B = %d ran out of its %d s: nothing more is started' % (B, LIMIT))
        return None
    got = [l for l in r.stdout.splitlines() if l.startswith('RESULT ')]
    if r.returncode != 0 or not got:
        print('B = %d failed (exit status %d): nothing more is started\n%s' % (B, r.returncode, (r.stdout + r.stderr)[-2000:]))
        return None
    return json.loads(got[-1][7:])


def main(argv):
    if argv[:1] == ['--step']:
        return step(int(argv[1]), int(argv[2]), int(argv[3]))
    N = int(argv[0]) if len(argv) > 0 else 1000000
    R = int(argv[1]) if len(argv) > 1 else 100
    lines = ['locate_timing.py %d %d: synthetic chromosome of %d sites (n = 100), default grid, every site a test site' % (N, R, N)]
    ok = True
    for B in BLOCKS:
        k = child(N, R, B)
        if k is None:
            sys.exit(1)
        if B == BLOCKS[0]:
            lines.append('observed scan: kernels %.2f ms for M = %d windows; the apexes of --peaks %g with CLR >= %.4g (the %g quantile): '
                         '%d peaks, H = G: the union of their ranges holds %d test positions'
                         % (k['scan_ms'], k['M'], G, k['cut'], Q, k['K'], k['union']))
        lines.append('R = %d, B = %d, wall ms per replicate (mean):' % (R, B))
        for path, what in (('device', 'replicate built on the device (bmx_ctx_resample_sites)'),
                           ('host', 'replicate built on the host (np.repeat + set_sites)')):
            d = k[path]
            lines.append('  %-56s resample %8.2f  set_tests + plan %8.2f  scan %8.2f  accumulate %6.2f  total %8.2f'
                         % (what + ':', d['resample'], d['set_tests'], d['scan'], d['accumulate'], d['total']))
        lines.append('  building the replicate: host / device = %.1f; whole replicate: host / device = %.2f; same argmax rows and maxima, '
                     'bitwise: %s' % (k['host']['resample'] / k['device']['resample'], k['host']['total'] / k['device']['total'],
                                      'yes' if k['same'] else 'NO'))
        lines.append('  replicates with N\' = 0: %d of %d; peaks with n_ok < R: %d of %d' % (k['device_empty'], R, k['peaks_short'], k['K']))
        ok = ok and k['same']
    text = '\n'.join(lines) + '\n'
    with open(os.path.join(ROOT, 'profiles', 'locate_timing.txt'), 'w') as fh:
        fh.write(text)
    print(text, end='')
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main(sys.argv[1:])
