"""GPU tests added in round 4.

The headline workloads against the ORACLE at scale: BASELINE config 4 (whole genome, 22 chromosomes) and config 5 (8 contigs)
scanned in full exactly as bench.py scans them (ONE context, one slot per chromosome, scans launched back to back), then
>= 10 000 windows of config 4 -- >= 400 on EVERY chromosome, including the first and last 64 test sites of each and the
windows on either side of every launch-range cut -- and >= 2 000 windows over ALL 8 config-5 contigs recomputed by the plain-C
oracle (oracle/bmx_oracle.c orc_scan = calcBaller, BalLeRMix+_v1.py:436-507, in log1p form) from a selection table that
the oracle builds itself (oracle/bmx_oracle.py sel_table = NormalizedBetaBinom, v1:319-433, scipy's betabinom), never from the
GPU's own K1 table: K1 -> K2 -> finalize is checked end to end.  Bar: exact (x, alpha, A, nSites); CLR to 1e-6 relative
(1e-9 absolute floor) as north_star states; the worst relative difference is printed.
"""
import os
import sys

import numpy as np
import pytest

from util import c_oracle, c_scan, oracle_R

pytestmark = pytest.mark.gpu


def _T_at(R, As, gen, row, t, lin, npairs, nab):
    """The oracle's T of test site position t at the grid point with linear index lin, and its window size (numpy; the same
    sum as orc_scan, one grid point)."""
    iA, rem = divmod(int(lin), npairs)
    ix, ia = divmod(rem, nab)
    A = As[iA]
    rad = 19.0 / A
    i0, i1 = np.searchsorted(gen, t - rad, 'left'), np.searchsorted(gen, t + rad, 'right')
    g = gen[i0:i1]
    al = np.exp(-A * np.abs(g - t))
    keep = (al >= 1e-8) & (g != t)
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(2.0 * np.sum(np.log1p(al[keep] * R[ix, ia, row[i0:i1][keep]]))), int(keep.sum())


def _compare(name, got, want, R, As, gen, row, tpos, nx, nab):
    """got / want: (clr, ix, ia, iA, ns) of the same test sites from the GPU and from the oracle.  Returns (worst relative
    CLR difference, worst absolute one, number of rounding-noise ties).  A different argmax is accepted only where the
    oracle's own T at the GPU's grid point is within 1e-9 of the oracle's best -- a tie the reference would resolve by the
    rounding noise of its sums -- and such windows are counted and reported."""
    clr, ix, ia, iA, ns = got
    oc, ox, oa, oA, on = want
    npairs = nx * nab
    same = (ix == ox) & (ia == oa) & (iA == oA)
    ties = 0
    for j in np.where(~same)[0]:
        assert iA[j] >= 0 and oA[j] >= 0, (name, j, clr[j], oc[j])
        T, n = _T_at(R, As, gen, row, tpos[j], (iA[j] * nx + ix[j]) * nab + ia[j], npairs, nab)
        assert abs(T - oc[j]) <= 1e-9 * abs(oc[j]) and n == ns[j], (name, j, clr[j], oc[j], T, (ix[j], ia[j], iA[j]), (ox[j], oa[j], oA[j]))
        ties += 1
    assert np.array_equal(ns[same], on[same]), (name, np.where(ns != on)[0][:8])
    err = np.abs(clr - oc)
    tol = np.maximum(1e-9, 1e-6 * np.abs(oc))
    bad = np.where(~(err <= tol))[0]
    assert len(bad) == 0, (name, bad[:8], clr[bad[:8]], oc[bad[:8]])
    assert np.array_equal(oA < 0, iA < 0) or ties, name
    rel = err / np.maximum(np.abs(oc), 1e-9)
    return float(rel.max()) if len(rel) else 0.0, float(err.max()) if len(err) else 0.0, ties


def _sample(N, rng, edge, nrand, cuts):
    parts = [np.arange(0, min(edge, N)), np.arange(max(N - edge, 0), N), rng.integers(0, N, nrand)]
    for c in cuts:
        parts.append(np.arange(max(c - 32, 0), min(c + 32, N)))
    return np.unique(np.concatenate(parts))


def test_config4_every_chromosome_against_the_oracle():
    """BASELINE config 4 as bench.py runs it; 10 000+ windows over all 22 chromosomes against the C oracle, K1 -> K2 end to end."""
    import test_gpu_round2 as r2
    from ballermixplus_amd import engine as eng
    from ballermixplus_amd.hostmodel import Grids
    sizes, data, spect = r2._config4_data()
    xs, ab, As = Grids(None, None, False, False, None, None).scan_order()
    min_count = int(min(int(d[2].min()) for d in data))
    model = eng.ModelArrays('B2', min_count, [100], spect, {100: 1.0}, xs, ab)
    R = oracle_R('B2', [100], min_count, spect, {100: 1.0}, xs, ab)
    # the oracle's table against the device's (K1 is pinned by the reference's tables elsewhere; this is the same check on the
    # table this workload uses)
    ctx = eng.Context(0)
    ctx.set_model(model, As)
    Rd = ctx.fetch_lut()[1]
    ok = np.isfinite(R)
    assert np.array_equal(ok, np.isfinite(Rd)) and np.max(np.abs(Rd[ok] - R[ok]) / np.maximum(np.abs(R[ok]), 1e-300)) < 1e-9
    for c, (phys, gen, k, nn) in enumerate(data):
        N = len(gen)
        ctx.select_slot(c)
        ctx.set_sites(gen, model.rows_of(k, nn))
        ctx.set_tests(gen, np.zeros(N, np.int64), np.full(N, N - 1, np.int64))
    for c in range(len(data)):
        ctx.select_slot(c)
        ctx.scan()
    ctx.sync()
    L = c_oracle()
    total, worst, worst_abs, ties, ncuts = 0, 0.0, 0.0, 0, 0
    for c, (phys, gen, k, nn) in enumerate(data):
        N = len(gen)
        ctx.select_slot(c)
        cuts = [int(v) for v in ctx.launch_ranges()[1:]]
        ncuts += len(cuts)
        got = ctx.fetch()
        assert len(got[0]) == N
        idx = _sample(N, np.random.default_rng(4000 + c), 64, 340, cuts)
        assert len(idx) >= 400
        row = model.rows_of(k, nn)
        want = c_scan(L, R, As, gen, row, gen[idx], np.zeros(len(idx), np.int64), np.full(len(idx), N - 1, np.int64))
        w, wa, t = _compare('chr%d' % (c + 1), tuple(a[idx] for a in got), want, R, As, gen, row, gen[idx], len(xs), len(ab))
        worst, worst_abs, ties, total = max(worst, w), max(worst_abs, wa), ties + t, total + len(idx)
    ctx.close()
    assert total >= 10000 and ncuts >= 1          # chromosome 1 (3.46 M windows) does not fit one launch range
    print('config 4 vs C oracle (own table): %d windows on 22 chromosomes, %d launch-range cuts covered, worst rel dCLR %.3e, '
          'worst abs %.3e, %d rounding-noise ties' % (total, ncuts, worst, worst_abs, ties))
    assert worst < 1e-6
    assert ties == 0


def test_config5_every_contig_against_the_oracle():
    """BASELINE config 5 as bench.py runs it (8 contigs of 1.25 M SNPs, n = 200, 100 x 10 x 44 grid); 2 000+ windows over all 8
    contigs against the C oracle with the oracle's own table."""
    from ballermixplus_amd import engine as eng, synth
    from ballermixplus_amd.hostmodel import Grids
    data = [synth.synth_chromosome(1250000, 200, c + 1) for c in range(8)]
    spect = {(a, b): f for a, b, f in synth.spect_from_counts(np.concatenate([d[2] for d in data]), np.concatenate([d[3] for d in data]))}
    xs, ab, As = Grids(None, None, True, True, '100,10000,100', None).scan_order()
    assert (len(As), len(xs), len(ab)) == (100, 10, 44)
    min_count = int(min(int(d[2].min()) for d in data))
    model = eng.ModelArrays('B2', min_count, [200], spect, {200: 1.0}, xs, ab)
    R = oracle_R('B2', [200], min_count, spect, {200: 1.0}, xs, ab)
    ctx = eng.Context(0)
    ctx.set_model(model, As)
    for c, (phys, gen, k, nn) in enumerate(data):
        N = len(gen)
        ctx.select_slot(c)
        ctx.set_sites(gen, model.rows_of(k, nn))
        ctx.set_tests(gen, np.zeros(N, np.int64), np.full(N, N - 1, np.int64))
    for c in range(8):
        ctx.select_slot(c)
        ctx.scan()
    ctx.sync()
    L = c_oracle()
    total, worst, worst_abs, ties = 0, 0.0, 0.0, 0
    for c, (phys, gen, k, nn) in enumerate(data):
        N = len(gen)
        ctx.select_slot(c)
        cuts = [int(v) for v in ctx.launch_ranges()[1:]]
        got = ctx.fetch()
        idx = _sample(N, np.random.default_rng(5000 + c), 32, 200, cuts)
        row = model.rows_of(k, nn)
        want = c_scan(L, R, As, gen, row, gen[idx], np.zeros(len(idx), np.int64), np.full(len(idx), N - 1, np.int64))
        w, wa, t = _compare('contig%d' % (c + 1), tuple(a[idx] for a in got), want, R, As, gen, row, gen[idx], len(xs), len(ab))
        worst, worst_abs, ties, total = max(worst, w), max(worst_abs, wa), ties + t, total + len(idx)
    ctx.close()
    assert total >= 2000
    print('config 5 vs C oracle (own table): %d windows on 8 contigs, worst rel dCLR %.3e, worst abs %.3e, %d rounding-noise ties'
          % (total, worst, worst_abs, ties))
    assert worst < 1e-6
    assert ties == 0


def _native_rccl_gather_checks():
    """The body of test_native_rccl_gather_with_one_rank, run in a process of its own."""
    from ballermixplus_amd import _lib, engine as eng, synth
    from ballermixplus_amd.hostmodel import Grids
    xs, ab, As = Grids(None, None, False, False, None, None).scan_order()
    data = [synth.synth_chromosome(60000, 100, c + 1) for c in range(2)]
    spect = {(a, b): f for a, b, f in synth.spect_from_counts(np.concatenate([d[2] for d in data]), np.concatenate([d[3] for d in data]))}
    model = eng.ModelArrays('B2', 1, [100], spect, {100: 1.0}, xs, ab)
    ctx = eng.Context(0)
    ctx.set_model(model, As)
    for c, (phys, gen, k, nn) in enumerate(data):
        idx = np.arange(20000, 20000 + 4096 * (c + 1))
        ctx.select_slot(c)
        ctx.set_sites(gen, model.rows_of(k, nn))
        ctx.set_tests(gen[idx], np.zeros(len(idx), np.int64), np.full(len(idx), len(gen) - 1, np.int64))
        ctx.scan()
    want = ctx.pack_records()
    assert len(want) == 4096 * 3
    comm = eng.Comm(ctx, eng.Comm.make_id(), 0, 1)
    got = comm.gather_records([len(want)], root=0)
    assert np.array_equal(got, want)
    again = comm.gather_records([len(want)], root=0, out=np.empty(len(want), dtype=_lib.RECORD_DTYPE))      # buffers are reused
    assert np.array_equal(again, want)
    with pytest.raises(_lib.BmxError):           # counts must say what the context holds
        comm.gather_records([len(want) - 1], root=0)
    with pytest.raises(ValueError):
        comm.gather_records([1, 2], root=0)
    comm.close()
    ctx.close()


def test_native_rccl_gather_with_one_rank():
    """bmx_comm_*: the library's own RCCL communicator (librccl.so through dlopen, ncclCommInitRank on the context's device) and
    ONE gather of the packed records of two chromosome slots -- with a single rank the group holds no send / receive, the path
    through ncclGroupStart / ncclGroupEnd, the packing into the receive buffer and the copy to the host is the same one N ranks
    take.  (N > 1 needs N GPUs: RCCL refuses two ranks on one device.  Not run on this 1-GPU box.)
    The checks run in a fresh process, as a rank does: in the test process the library is loaded before anything imports
    torch, and a test that imports torch later brings torch's own librccl.so.1 and HIP runtime into it; dlopen("librccl.so.1")
    would then return torch's copy, bound to a HIP runtime this process never initialised (ncclCommInitRank: "no
    ROCm-capable device is detected")."""
    import subprocess
    from util import HERE
    r = subprocess.run([sys.executable, '-c', 'import sys; sys.path.insert(0, sys.argv[1]); import test_gpu_round4 as t; '
                        't._native_rccl_gather_checks(); print("native gather ok")', HERE],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'native gather ok' in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_bench_step_through_the_native_gather():
    """bench.py with BMX_NATIVE_GATHER=1 and the process group forced on for a single rank: every step's records go through
    bmx_comm_gather_records (the library's own ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd path) instead of
    torch.distributed.gather; same checksum and parity sample as the plain run."""
    import json
    import subprocess
    from util import REPO
    env = dict(os.environ, BMX_FORCE_DIST='1', BMX_NATIVE_GATHER='1', MASTER_ADDR='127.0.0.1', MASTER_PORT='29673')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'BMX_DIST_BACKEND', 'BMX_SINGLE_DEVICE'):
        env.pop(k, None)
    common = [sys.executable, os.path.join(REPO, 'bench.py'), '--steps', '2', '--warmup', '1', '--total-snps', '400000', '--no-cpu-baseline',
              '--full']
    r = subprocess.run(common, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
    assert d['config']['records_per_step'] == d['config']['windows_per_step'] and d['parity_sample']['mismatches'] == 0
    assert 'bitwise equal to the timed steps\': True' in d['config']['end_to_end_note']
    for k in ('BMX_FORCE_DIST', 'BMX_NATIVE_GATHER'):
        env.pop(k)
    r1 = subprocess.run(common, capture_output=True, text=True, timeout=600, env=env)
    assert r1.returncode == 0, r1.stderr[-2000:]
    d1 = json.loads([l for l in r1.stdout.splitlines() if l.startswith('{')][-1])
    assert d1['config']['checksum_clr'] == pytest.approx(d['config']['checksum_clr'], rel=1e-12)


def test_set_tests_without_window_bounds_means_all_sites():
    """bmx_ctx_set_tests(win_lo = win_hi = NULL): every window holds all sites of the chromosome (Scan._alpha, BalLeRMix+_v1.py:598-610;
    the bounds are written on the device) -- the records are those of explicit [0, N - 1] bounds, bit for bit, at stride 1 (groups
    of 16), stride 5 (groups of 8) and stride 40 (one test site per wave); one of the two bounds alone is refused."""
    from ballermixplus_amd import engine as eng, synth
    from ballermixplus_amd.hostmodel import Grids
    N, n = 200000, 100
    phys, gen, k, nn = synth.synth_chromosome(N, n, 3)
    spect = {(a, b): f for a, b, f in synth.spect_from_counts(k, nn)}
    xs, ab, As = Grids(None, None, False, False, None, None).scan_order()
    model = eng.ModelArrays('B2', int(k.min()), [n], spect, {n: 1.0}, xs, ab)
    ctx = eng.Context(0)
    ctx.set_model(model, As)
    ctx.set_sites(gen, model.rows_of(k, nn))
    for step, kernel in ((1, 'clr_scan_prepared_kernel<16,true>'), (5, 'clr_scan_prepared_kernel<8,true>'), (40, 'clr_scan_solo_kernel<true>')):
        idx = np.arange(1000, 150000, step)[:20000]
        ctx.set_tests(gen[idx], np.zeros(len(idx), np.int64), np.full(len(idx), N - 1, np.int64))
        assert ctx.plan()['kernel'] == kernel
        ctx.scan()
        want = ctx.fetch_records().copy()
        ctx.set_tests(gen[idx])
        ctx.scan()
        got = ctx.fetch_records()
        assert np.array_equal(got, want), step
    from ballermixplus_amd import _lib
    t = _lib.f64(gen[:16])
    with pytest.raises(Exception):
        _lib.check(ctx._L.bmx_ctx_set_tests(ctx._h, 16, _lib.as_dp(t), _lib.as_lp(np.zeros(16, np.int64)), None))
    ctx.close()
