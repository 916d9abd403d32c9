#!/usr/bin/env python3
"""Fixtures of --refine: the reference's own T at off-grid points (tests/golden/refine/).

Runs only in the build container, where the reference checkout is mounted at /root/reference.  Each run is the reference's
CLI on Example 2 with a one-value grid (--fixX, --fixAlpha, --listA) at a point that lies between grid values, near the
example's own maxima, every 24th
site (-s 24: about 50 rows), so that its CLR column is T at that point (or 0 where T <= 0).

    python tests/golden/make_refine_golden.py
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
REF_PY = os.path.join(REF, 'BalLeRMix+_v1.py')
REF_TEST = os.path.join(REF, 'test')

# name: (input, helper file, flags, (x, alpha_beta, A))
RUNS = {
    'ex2_B2_x0.47_a3.7e8_A937.5': ('Example2_balancing_10MYA_DAF.txt', 'HC_CEU_Neut_DAF_spect_for_B2.txt', [], ('0.47', '3.7e8', '937.5')),
    'ex2_B2_x0.43_a3.3_A777.7': ('Example2_balancing_10MYA_DAF.txt', 'HC_CEU_Neut_DAF_spect_for_B2.txt', [], ('0.43', '3.3', '777.7')),
    'ex2_B2maf_x0.47_a0.037_A123.4': ('Example2_balancing_10MYA_DAF.txt', 'HC_CEU_Neut_MAF_spect_for_B2maf.txt', ['--MAF'],
                                      ('0.47', '0.037', '123.4')),
}
STEP = '24'


def main():
    out = os.path.join(HERE, 'refine')
    os.makedirs(out, exist_ok=True)
    for name, (inp, spect, flags, (x, a, A)) in RUNS.items():
        args = ['-i', inp, '--spect', spect] + flags + ['--fixX', x, '--fixAlpha', a, '--listA', A, '-s', STEP]
        full = [os.path.join(REF_TEST, v) if v.endswith('.txt') else v for v in args]
        subprocess.run([sys.executable, REF_PY] + full + ['-o', os.path.join(out, name + '.tsv')], check=True,
                       stdout=subprocess.DEVNULL)
        with open(os.path.join(out, name + '.args.json'), 'w') as f:
            json.dump(args, f)
        print(name)


if __name__ == '__main__':
    main()
