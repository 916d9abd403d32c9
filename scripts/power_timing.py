"""Cost of --power on the synthetic 1M-SNP chromosome of locate_timing.py (n = 100, default grid, every site a test site): the
planted point A = 1000, x = 0.5, alpha_beta = 100, default spacing and span, perm background with blocks of 1 site, R replicates.
Writes profiles/power_timing.txt:
  - the number of centres and the share of the chromosome's test positions the union of their ranges covers;
  - the mean wall milliseconds per replicate of permute, plant (and the device milliseconds bmx_ctx_plant_ms reports for it),
    set_tests + plan, scan and accumulate on the device path that power.run_replicates drives;
  - the plant step of the only alternative there was before -- fetch_sites, power.planted_rows in numpy, set_sites -- on the
    same box, for the first HOST_R replicates (it is slow), and the ratio;
  - whether the two paths give the same planted rows and the same argmax rows on those replicates.
The measurement is one child process under a time limit; if it fails, faults or runs out of time nothing more is started.
Usage: python scripts/power_timing.py [N] [R]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLANT = '1000,0.5,100'
HOST_R = 3
LIMIT = 540                 # seconds for the GPU step


def step(N, R):
    import numpy as np
    from ballermixplus_amd import engine, locate, power, synth
    from ballermixplus_amd.hostmodel import Grids
    phys, gen, k, nn = synth.synth_chromosome(N, 100, 1)
    xs, ab, As = Grids(None, None, False, False, None, None).scan_order()
    sp = {(a, b): f for a, b, f in synth.spect_from_counts(k, nn)}
    model = engine.ModelArrays('B2', int(k.min()), [100], sp, {100: 1.0}, xs, ab)
    rows = model.rows_of(k, nn)
    planted = power.parse_plant(PLANT, As, xs, ab)
    A = float(As[planted[0]])
    gw = power.allowed_rows('B2', model.min_count, model.sizes, model.row_off, model.g)
    ctx = engine.Context(0)
    ctx.set_model(model, As)
    ctx.set_sites(gen, rows)
    ctx.set_tests(gen)
    ctx.scan()
    ctx.sync()
    ctx.scan()                  # (the first scan of a process also loads the code objects)
    ctx.sync()
    out = {'R': R, 'M': len(gen), 'scan_ms': ctx.last_scan_ms()}
    crow, union, lo, hi, H, bound, D = power.plan_file(gen, A, float(min(As)), None, None, ctx._L.bmx_alpha_cut())
    tg, cpos = gen[union], gen[crow]
    out.update(K=len(crow), union=len(union), H=H, bound=bound, D=D)
    power.run_replicates(ctx, tg, lo, hi, cpos, planted, gw, 1, 2)              # warm-up, not timed
    timing = []
    arg, clr, lin, ns, first, count = power.run_replicates(ctx, tg, lo, hi, cpos, planted, gw, 1, R, timing=timing)
    t = np.array(timing)
    out['device'] = dict(zip(('permute', 'plant', 'set_tests', 'scan', 'accumulate'), (t[:, :5].mean(axis=0) * 1e3).tolist()),
                         plant_device_ms=float(t[:, 5].mean()), total=float(t[:, :5].sum(axis=1).mean() * 1e3))
    out['reach'] = int(power.n_reach(gen, cpos, A).sum())
    # the alternative: the rows come back, are redrawn in numpy and go up again through set_sites
    Rt = ctx.fetch_lut()[1][planted[1], planted[2]]
    host_ms, same_rows, same_arg = [], True, True
    now = time.perf_counter
    for r in range(min(HOST_R, R)):
        ctx.permute_rows(power.background_key(1, r, 0), 1)
        ctx.sync()
        t0 = now()
        g0, r0 = ctx.fetch_sites(len(gen))
        new, margin = power.planted_rows(g0, r0, model.sizes, model.row_off, Rt, gw, A, cpos, power.replicate_key(1, r, 0))
        ctx.select_slot(2)
        ctx.set_sites(g0, new)
        host_ms.append((now() - t0) * 1e3)
        ctx.set_tests(tg)
        ctx.scan()
        c2, _, _, iA2, _ = ctx.fetch()
        a2, v2 = locate.argmax_rows(c2, iA2 >= 0, lo, hi)
        same_arg = same_arg and bool(np.array_equal(a2, arg[r]) and np.array_equal(v2.view(np.uint64), clr[r].view(np.uint64)))
        ctx.select_slot(1)
        ctx.plant_sites(0, power.replicate_key(1, r, 0), cpos, *planted, gw)
        same_rows = same_rows and bool(np.array_equal(ctx.fetch_sites(len(gen))[1], new))
        out['undecided'] = out.get('undecided', 0) + int(np.count_nonzero(margin <= power.MARGIN))
        ctx.select_slot(0)
    ctx.restore_rows()
    out.update(host_plant_ms=float(np.mean(host_ms)), host_R=len(host_ms), same_rows=same_rows, same_arg=same_arg,
               power=[float(np.mean(clr >= C)) for C in (50.0, 100.0)], n_ok_short=int(np.count_nonzero((arg >= 0).sum(axis=0) < R)))
    ctx.close()
    print('RESULT ' + json.dumps(out), flush=True)


def main(argv):
    if argv[:1] == ['--step']:
        return step(int(argv[1]), int(argv[2]))
    N = int(argv[0]) if len(argv) > 0 else 1000000
    R = int(argv[1]) if len(argv) > 1 else 20
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', str(N), str(R)], capture_output=True, text=True,
                           timeout=LIMIT, cwd=ROOT)
    except subprocess.TimeoutExpired:
        print('the measurement ran out of its %d s: nothing more is started' % LIMIT)
        sys.exit(1)
    got = [l for l in r.stdout.splitlines() if l.startswith('RESULT ')]
    if r.returncode != 0 or not got:
        print('the measurement failed (exit status %d): nothing more is started\n%s' % (r.returncode, (r.stdout + r.stderr)[-2000:]))
        sys.exit(1)
    k = json.loads(got[-1][7:])
    d = k['device']
    lines = [
        'power_timing.py %d %d: synthetic chromosome of %d sites (n = 100), default grid, every site a test site' % (N, R, N),
        'observed scan: kernels %.2f ms for M = %d windows; planted point %s, H = %.6g, bound = %.6g, D = %.6g: %d centres, %d sites in '
        'reach, the union of their ranges holds %d test positions (%.1f %% of the chromosome)'
        % (k['scan_ms'], k['M'], PLANT, k['H'], k['bound'], k['D'], k['K'], k['reach'], k['union'], 100.0 * k['union'] / k['M']),
        'R = %d, perm background (blocks of 1 site), wall ms per replicate (mean):' % R,
        '  permute %7.2f  plant %7.2f (device: %.3f)  set_tests + plan %7.2f  scan %8.2f  accumulate %6.2f  total %8.2f'
        % (d['permute'], d['plant'], d['plant_device_ms'], d['set_tests'], d['scan'], d['accumulate'], d['total']),
        'the plant step on the host (fetch_sites + power.planted_rows in numpy + set_sites), mean of the first %d replicates: %.1f ms; '
        'host / device = %.1f' % (k['host_R'], k['host_plant_ms'], k['host_plant_ms'] / d['plant']),
        'same planted rows on those replicates: %s (undecided sites: %d); same argmax rows and maxima, bitwise: %s'
        % ('yes' if k['same_rows'] else 'NO', k['undecided'], 'yes' if k['same_arg'] else 'NO'),
        'share of (replicate, centre) maxima >= 50: %.3f, >= 100: %.3f; centres with n_ok < R: %d of %d'
        % (k['power'][0], k['power'][1], k['n_ok_short'], k['K']),
    ]
    text = '\n'.join(lines) + '\n'
    with open(os.path.join(ROOT, 'profiles', 'power_timing.txt'), 'w') as fh:
        fh.write(text)
    print(text, end='')
    sys.exit(0 if k['same_rows'] and k['same_arg'] else 1)


if __name__ == '__main__':
    main(sys.argv[1:])
