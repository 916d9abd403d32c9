"""Command line of the MI355X build: every flag of the reference's main()
(BalLeRMix+_v1.py:715-802) with the same spelling, defaults and pipeline order
InputData -> NeutralSFS -> get_neut_probs -> Grids -> NormalizedBetaBinom -> Scan (v1:777-799).

Additions (do not change any reference command line):
  --device K        GPU index for a single-process run (default 0)
  -i a.txt,b.txt,... | --inputs LIST.txt     several input files (a whole genome, one file per chromosome) in ONE process
                    on one scan context: the selection table is built once (and rebuilt only when a file's sample sizes
                    or minCount differ), the next file is read while the current one is scanned, and -o names a directory
                    (created; outputs are <dir>/<input basename>.out.txt) or a pattern containing {} (replaced by the
                    input's basename without extension).  The reference handles one file per process
                    (BalLeRMix+_v1.py:777-799); looping it pays process start, HIP start-up and the table once per file.
  --nullPerm R [--nullSeed S] [--nullBlock B]     permutation null (ballermixplus_amd/null.py): after the observed scan of
                    each file, R more scans with the sites' (k, n) rows permuted on the device; writes <out>.null.txt (several
                    files: <dir>/null.txt or the -o pattern with `null`) and <out>.pval.txt next to each output file.
  --profiles A,x,abeta     profile likelihoods (ballermixplus_amd/profiles.py): per window the CLR with A, x or alpha_beta fixed
                    to each grid value, from the same scan; writes <out>.profile_A.txt / .profile_x.txt / .profile_abeta.txt
                    next to each output file.
  --refine [--refineMin C]     off-grid refinement (ballermixplus_amd/refine.py): a compass search from each window's grid argmax
                    (windows with grid CLR >= C); writes <out>.refined.txt next to each output file, the main output's format.
  --support [--supportDrop D] [--supportMin C]     with --refine: support intervals around each refined maximum
                    (ballermixplus_amd/support.py): per free coordinate, the range where the profile T stays >= T* - D
                    (windows with refined CLR >= C); writes <out>.support.txt next to each output file.
  --boot R [--bootSeed S] [--bootBlock B] [--bootLevel L] [--bootMin C] [--bootReps]     with --refine: a Poisson block
                    bootstrap of each refined maximum (ballermixplus_amd/boot.py): R replicates re-weight the sites in blocks of
                    B consecutive sites and repeat the search from the refined point (windows with refined CLR >= C); writes
                    <out>.boot.txt (percentile ends at level L, standard deviations) and with --bootReps <out>.boot.reps.txt
                    next to each output file.
  --peaks G [--peakMin C] [--peakExtent F] [--atPeaks]     peaks of the CLR track (ballermixplus_amd/peaks.py): the rows that no row
                    within distance G beats (CLR >= C), each with its extent (rows with CLR >= F * apex CLR, inside the saddles
                    to its neighbours); writes <out>.peaks.txt next to each output file (several files: also <dir>/peaks.txt or
                    the -o pattern with `peaks`, genome-wide).  --atPeaks (with --refine): refine only the apexes, and so compute
                    --support / --boot for them only.  `python -m ballermixplus_amd.peaks OUT.txt --peaks G` calls peaks again on
                    an existing output.
  --surfaces [--surfaceMin C] [--surfaceMax N]     likelihood surfaces of selected windows (ballermixplus_amd/surfaces.py): T at
                    every grid point (A, x, alpha_beta) of the observed scan's windows with CLR >= C -- with --peaks only the apexes
                    among them -- at most N of them (default 1000: the N highest CLR); needs --peaks or --surfaceMin.  Writes
                    <out>.surfaces.txt next to each output file: per window a block of rows physPos, genPos, A, x, abeta, T, nSites
                    with the grids ascending.
  --influence [--influenceBlock B] [--influenceMin C] [--influenceMax N] [--influenceDetail]     delete-block jackknife of the
                    CLR of selected windows (ballermixplus_amd/influence.py): per window, selected as --surfaces selects them
                    (CLR >= C, with --peaks only the apexes, at most N: default 1000; needs --peaks or --influenceMin), the grid
                    maximum of its surface without each block of B consecutive sites (default 1) and the share of the maximum
                    each block holds; writes <out>.influence.txt (per window: the number of blocks, the jackknife spread, how few
                    blocks hold half of the maximum, the largest share, the block whose removal costs most) and with
                    --influenceDetail <out>.influence.blocks.txt (every block) next to each output file.
  --fit [--fitBins D] [--fitClasses F] [--fitMin C] [--fitMax N] [--fitMinExp E] [--fitDetail]     goodness of fit of selected
                    windows (ballermixplus_amd/fit.py): per window, selected as --surfaces selects them (CLR >= C, with --peaks only
                    the apexes, at most N: default 1000; needs --peaks or --fitMin), the sites of the window at its scan argmax
                    counted by distance bin (D bins of z = A |g - t| up to the cut, default 8) and frequency class (F classes of
                    k / n, default 10) against the counts the fitted mixture and neutrality expect; writes <out>.fit.txt (per
                    window: the two chi-square sums over the cells with an expected count >= E, default 5, their degrees of
                    freedom and the worst cell) and with --fitDetail <out>.fit.cells.txt (every cell) next to each output file.
                    Sites are linked: the sums describe, they are no calibrated test.
  --conditional [--condSpan H] [--condMin C] [--condSurfaces]     with --peaks: are two nearby apexes two loci, or one locus and
                    its shoulder (ballermixplus_amd/conditional.py)?  Every apex gets as parent the highest apex above it within H
                    (default: the sum of the two fitted reaches, alpha_cut / A_hat each); the apex's surface is then computed
                    again with the parent's fitted model, held at its grid argmax, in place of neutrality at the sites the two
                    share, and the parent's given the apex.  Writes <out>.conditional.txt next to each output file: per apex with
                    CLR >= C (default: all) the parent, the shared sites, the conditional maximum and where it sits, the share
                    of the unconditional maximum it retains, and the same for the parent given the apex; with --condSurfaces
                    <out>.conditional.surfaces.txt (the conditional surfaces, in --surfaces' format).  One locus, not refitted;
                    sites are linked: `retained` describes, it is no test.
  --stepwise [--stepMin C] [--stepMax K] [--stepSurfaces]     with --peaks: which of the apexes are separate loci
                    (ballermixplus_amd/stepwise.py)?  Forward stepwise selection: the highest apex is accepted at its grid argmax,
                    every other apex is computed again given ALL accepted loci, the best of what is left is accepted, until
                    nothing reaches C (default: --peakMin's value, else 0) or K loci (default 1000) are in.  Writes
                    <out>.stepwise.txt next to each output file: per apex its order of entry, the conditional maximum (at entry
                    for an accepted apex, given all accepted loci for the others) and where it sits, the share of the
                    unconditional maximum it retains and the running log ratio T_total of the accepted loci against neutrality;
                    with --stepSurfaces <out>.stepwise.surfaces.txt (each accepted apex's surface at entry, in --surfaces'
                    format).  Greedy, loci held at grid points and never refitted; sites are linked: C is a threshold, not a test.
  --sandwich [--sandwichBlock B] [--sandwichMin C] [--sandwichMax N] [--sandwichStep hx,hv]     how well are x, alpha_beta and A
                    determined (ballermixplus_amd/sandwich.py)?  The sandwich (Godambe) variance H^-1 J H^-1 of selected windows of
                    the observed scan (selected as --surfaces selects) at each window's fitted point -- the refined point with
                    --refine, else the grid argmax: H from the per-site scores, J from their sums over blocks of B consecutive
                    sites (default 1).  Writes <out>.sandwich.txt next to each output file: standard errors of x, ln alpha_beta
                    and ln A with and without the linkage correction, the scale lambda by which linkage inflates the CLR, and
                    CLR / lambda.  The point is not re-optimised and the null is on the boundary: CLR_adj describes, it is no test.
  --locate R [--locateSeed S] [--locateBlock B] [--locateSpan H] [--locateLevel L] [--locateMin C] [--locateReps]     with
                    --peaks: a block-bootstrap interval for the POSITION of every apex (ballermixplus_amd/locate.py): R replicates
                    resample the sites in blocks of B consecutive sites on the device, repeat the grid scan at the test positions
                    within H of the apexes (default H = G) and record where each peak's maximum falls; writes <out>.locate.txt
                    (percentile ends at level L as rows of the main output, the spread, the share of replicates at the apex and
                    at the ends of the range) and with --locateReps <out>.locate.reps.txt next to each output file.  Default
                    window mode only (no -w, no --fixWinSize).
  --power R --plant A,x,abeta [--powerThreshold C[,C...]] [--plantEvery D] [--powerSpan H] [--powerSeed S]
  [--powerBackground perm|obs] [--powerBlock B] [--powerReps]     planted-signal power analysis (ballermixplus_amd/power.py): R
                    replicates redraw, on the device, the derived counts of the sites within reach of centres every D along the
                    track from the mixture the scan fits at the grid point A,x,abeta (on the rows permuted in blocks of B sites,
                    or on the observed rows), scan the test positions within H of the centres and compare each centre's maximum
                    with the thresholds C (with --nullPerm: also the run's genome-wide 5 % and 1 % thresholds; the power step
                    then runs after the null); writes <out>.power.txt (per centre: the power at each threshold, the spread of the
                    maxima and of their positions, how often the planted grid values are recovered) and with --powerReps
                    <out>.power.reps.txt next to each output file.  Default window mode only.
Multi-GPU: launch under `python -m torch.distributed.run --nproc-per-node N -m ballermixplus_amd.cli ...`;
test sites are sharded over the ranks (rank r computes on GPU LOCAL_RANK), rank 0 gathers the 16-byte records
(one RCCL gather) and writes the output file.  BMX_DIST_BACKEND=gloo BMX_SINGLE_DEVICE=1 lets several ranks
share GPU 0 with a CPU gather: a rehearsal of the multi-rank control flow on a 1-GPU box.

Structure: main() asks every addition's <feature>_refusal(opt) before anything is read.  main() (one file) and main_many()
(several) bring a file to its Scan in their own ways; after it both call file_stages() per file and wrap_up() once.
"""
import argparse
import os
import sys
from collections import namedtuple
from datetime import datetime

import numpy as np


def build_parser():
    """Flags, destinations, types and defaults are the reference's (v1:718-753): its command lines run unchanged.
    The help texts are this build's own wording."""
    parser = argparse.ArgumentParser(description='BalLeRMix+ B-statistic scan on AMD Instinct MI355X (libbmxscan).')
    parser.add_argument('-i', '--input', dest='infile', required=False, default=None,
                        help='input file: header line, then tab-separated physPos, genPos, derived (or minor) allele count x, sample size n')
    parser.add_argument('-o', '--output', dest='outfile', help='output file (7 tab-separated columns, one row per test site)')
    parser.add_argument('--spect', dest='spectfile', required=True,
                        help='neutral helper file to read: frequency spectrum (k n fraction) or, with --noFreq, the '
                             'substitution/polymorphism configuration. With --getSpect / --getConfig: the file to WRITE')
    parser.add_argument('--minCount', dest='minCount', default=1,
                        help='smallest allele count present in the input when rare variants were filtered out (default 1; '
                             'used as given only by the B_1 statistic, otherwise taken from the data)')
    parser.add_argument('--getSpect', dest='getSpec', action='store_true', default=False,
                        help='helper step: tabulate the (k, n) frequency spectrum of the concatenated input -i into --spect and exit (combine with --MAF / --noSub as for the scan)')
    parser.add_argument('--getConfig', dest='getConfig', action='store_true', default=False,
                        help='helper step: tabulate the substitution : polymorphism proportions per sample size of -i into --spect and exit')
    parser.add_argument('--findBal', dest='bal', action='store_true', default=False,
                        help='restrict the (x, alpha) grid to shapes typical of balancing selection')
    parser.add_argument('--findPos', dest='pos', action='store_true', default=False,
                        help='restrict the (x, alpha) grid to shapes typical of positive selection (ignored when --findBal is given, as in the reference)')
    parser.add_argument('--noFreq', dest='nofreq', action='store_true', default=False,
                        help='B_1: ignore allele frequencies; a site is a substitution (count 0) or a polymorphism (any other count)')
    parser.add_argument('--noSub', dest='nosub', action='store_true', default=False,
                        help='B_0 / B_0,MAF: the input holds polymorphic sites only, no substitutions')
    parser.add_argument('--MAF', dest='MAF', action='store_true', default=False,
                        help='B_2,MAF / B_0,MAF: fold counts to minor-allele counts (default: polarised counts, B_2)')
    parser.add_argument('--usePhysPos', action='store_true', dest='phys', default=False,
                        help='measure distances on physical positions times --rec instead of on the genPos column')
    parser.add_argument('--rec', dest='Rrate', default=1e-6, type=float,
                        help='uniform recombination rate in cM per nucleotide for --usePhysPos (default 1e-6)')
    parser.add_argument('--fixWinSize', action='store_true', dest='size', default=False,
                        help='windows of a fixed physical length; give the length in nucleotides with -w')
    parser.add_argument('-w', '--window', dest='w', type=int, default=0,
                        help='number of informative sites on either side of the test site, or with --fixWinSize the window length in nucleotides (default 0: every site with alpha >= 1e-8)')
    parser.add_argument('--noCenter', action='store_true', dest='noCenter', default=False,
                        help='with --fixWinSize: test positions every -s nucleotides instead of at informative sites')
    parser.add_argument('-s', '--step', dest='step', type=float, default=1,
                        help='test every s-th informative site, or every s nucleotides with --noCenter (default 1)')
    parser.add_argument('--fixX', dest='x', help='fix the equilibrium frequency x instead of searching the x grid')
    parser.add_argument('--fixAlpha', dest='abeta', type=float, default=None,
                        help='fix the beta-binomial alpha parameter instead of searching the alpha grid')
    parser.add_argument('--rangeA', dest='seqA', help='linkage parameter grid as <Amin>,<Amax>,<Astep> (no spaces)')
    parser.add_argument('--listA', dest='listA', help='linkage parameter grid as a comma-separated list (no spaces)')
    # additions
    parser.add_argument('--inputs', dest='inputs', default=None,
                        help='MI355X build only: a text file naming several input files, one per line (whole genome in one process); '
                             'equivalent to -i a.txt,b.txt,...; -o is then a directory or a pattern containing {}')
    parser.add_argument('--device', dest='device', type=int, default=None,
                        help='GPU index for a single-process run (MI355X build only; not allowed under torch.distributed.run, where every rank uses GPU LOCAL_RANK)')
    parser.add_argument('--nullPerm', dest='nullPerm', type=int, default=0,
                        help='MI355X build only: R > 0 scans every input R more times with the sites\' (k, n) labels permuted within '
                             'the chromosome and writes <out>.null.txt (maximum CLR of every replicate) and <out>.pval.txt '
                             '(pointwise and genome-wide p-value of every window); default 0: off')
    parser.add_argument('--nullSeed', dest='nullSeed', type=int, default=1,
                        help='MI355X build only: seed of the --nullPerm permutations (default 1)')
    parser.add_argument('--nullBlock', dest='nullBlock', type=int, default=1,
                        help='MI355X build only: --nullPerm moves blocks of this many consecutive sites intact (default 1: single sites)')
    parser.add_argument('--profiles', dest='profiles', default=None,
                        help='MI355X build only: comma list of A, x, abeta.  Writes <out>.profile_<name>.txt next to each output '
                             'file: per window the CLR with that parameter fixed to each grid value (columns in ascending grid '
                             'order; the abeta file adds CLR_bal and CLR_pos); default: off')
    parser.add_argument('--refine', dest='refine', action='store_true', default=False,
                        help='MI355X build only: polish every window\'s grid maximum off the grid (a local compass search in ln A, x '
                             'and ln alpha_beta inside the hull of the grid) and write <out>.refined.txt next to each output file: '
                             'the main output\'s rows, with CLR, x_hat, s_hat, A_hat and nSites replaced where the refined CLR is '
                             'higher; default: off')
    parser.add_argument('--refineMin', dest='refineMin', type=float, default=None,
                        help='MI355X build only, with --refine: refine only the windows whose grid CLR is >= this value')
    parser.add_argument('--support', dest='support', action='store_true', default=False,
                        help='MI355X build only, with --refine: support intervals of x, s (alpha_beta) and A around each refined '
                             'maximum -- where the profile of T stays within --supportDrop of it -- written to <out>.support.txt '
                             'next to each output file; default: off')
    parser.add_argument('--supportDrop', dest='supportDrop', type=float, default=None,
                        help='MI355X build only, with --support: the drop D in T = 2 ln(likelihood ratio) that bounds the '
                             'intervals; default: %r, the 0.95 quantile of chi-square(1)' % 3.841458820694124)
    parser.add_argument('--supportMin', dest='supportMin', type=float, default=None,
                        help='MI355X build only, with --support: only windows whose refined CLR is >= this value; '
                             'default: --refineMin\'s value, or 0')
    parser.add_argument('--boot', dest='boot', type=int, default=0,
                        help='MI355X build only, with --refine: R >= 2 bootstrap replicates of every refined maximum.  Each replicate '
                             'gives every block of --bootBlock consecutive sites a Poisson(1) weight and repeats the local search '
                             'from the refined point; <out>.boot.txt holds percentile ends and standard deviations of x, s '
                             '(alpha_beta) and A per window; default 0: off')
    parser.add_argument('--bootSeed', dest='bootSeed', type=int, default=None,
                        help='MI355X build only, with --boot: seed of the bootstrap weights (default 1; its stream is separate from '
                             '--nullSeed\'s)')
    parser.add_argument('--bootBlock', dest='bootBlock', type=int, default=None,
                        help='MI355X build only, with --boot: sites per block (default 1).  B should span the linkage disequilibrium '
                             'of the data; B = 1 resamples sites as if they were independent')
    parser.add_argument('--bootLevel', dest='bootLevel', type=float, default=None,
                        help='MI355X build only, with --boot: level L of the percentile ends and of dT_q, 0 < L < 1 (default 0.95)')
    parser.add_argument('--bootMin', dest='bootMin', type=float, default=None,
                        help='MI355X build only, with --boot: only windows whose refined CLR is >= this value; '
                             'default: --refineMin\'s value, or 0')
    parser.add_argument('--bootReps', dest='bootReps', action='store_true', default=False,
                        help='MI355X build only, with --boot: also write every replicate of every bootstrapped window to '
                             '<out>.boot.reps.txt')
    parser.add_argument('--peaks', dest='peaks', type=float, default=None,
                        help='MI355X build only: call peaks on the CLR track with separation G, in the units the scan measures '
                             'distance in (the genPos column): a row is an apex when no row within G has a higher CLR.  Writes '
                             '<out>.peaks.txt next to each output file: one row per apex with its extent, the CLR at the saddles '
                             'to its neighbours and, with --nullPerm, its p-values.  No default: G states what "one locus" means; '
                             'a window at A_hat reaches 18.42 / A_hat')
    parser.add_argument('--peakMin', dest='peakMin', type=float, default=None,
                        help='MI355X build only, with --peaks: only apexes with CLR >= this value (default 0)')
    parser.add_argument('--peakExtent', dest='peakExtent', type=float, default=None,
                        help='MI355X build only, with --peaks: a peak extends over the rows around its apex with CLR >= F * apex '
                             'CLR, 0 < F <= 1 (default 0.5: the width at half maximum)')
    parser.add_argument('--atPeaks', dest='atPeaks', action='store_true', default=False,
                        help='MI355X build only, with --peaks and --refine: refine only the apexes (--refineMin still applies); '
                             '--support and --boot follow, as they only touch refined windows')
    parser.add_argument('--surfaces', dest='surfaces', action='store_true', default=False,
                        help='MI355X build only: write the likelihood surface T(A, x, alpha_beta) of selected windows of the observed '
                             'scan -- every grid point, not only the maximum -- to <out>.surfaces.txt next to each output file '
                             '(columns physPos, genPos, A, x, abeta, T, nSites; one block per window, grids ascending).  The windows: '
                             'with --peaks the apexes, with --surfaceMin those at or above it, with both the apexes at or above it; '
                             'one of the two is required; default: off')
    parser.add_argument('--surfaceMin', dest='surfaceMin', type=float, default=None,
                        help='MI355X build only, with --surfaces: only windows with CLR >= this value (default 0)')
    parser.add_argument('--surfaceMax', dest='surfaceMax', type=int, default=None,
                        help='MI355X build only, with --surfaces: at most N windows per file, the N with the highest CLR '
                             '(default 1000)')
    parser.add_argument('--influence', dest='influence', action='store_true', default=False,
                        help='MI355X build only: delete-block jackknife of the CLR of selected windows of the observed scan: the grid '
                             'maximum of the window\'s surface without each block of --influenceBlock consecutive sites, and each '
                             'block\'s share of the maximum, summarised per window in <out>.influence.txt next to each output file.  '
                             'The windows: with --peaks the apexes, with --influenceMin those at or above it, with both the apexes '
                             'at or above it; one of the two is required; default: off')
    parser.add_argument('--influenceBlock', dest='influenceBlock', type=int, default=None,
                        help='MI355X build only, with --influence: sites per block (default 1: single SNPs).  B should span the '
                             'cluster of sites whose joint removal is in question')
    parser.add_argument('--influenceMin', dest='influenceMin', type=float, default=None,
                        help='MI355X build only, with --influence: only windows with CLR >= this value (default 0)')
    parser.add_argument('--influenceMax', dest='influenceMax', type=int, default=None,
                        help='MI355X build only, with --influence: at most N windows per file, the N with the highest CLR '
                             '(default 1000)')
    parser.add_argument('--influenceDetail', dest='influenceDetail', action='store_true', default=False,
                        help='MI355X build only, with --influence: also write every block of every selected window to '
                             '<out>.influence.blocks.txt')
    parser.add_argument('--fit', dest='fit', action='store_true', default=False,
                        help='MI355X build only: goodness of fit of selected windows of the observed scan: the sites of each window '
                             'at its scan argmax, counted by distance bin and frequency class, against the counts expected under '
                             'the fitted mixture and under neutrality, summarised per window in <out>.fit.txt next to each output '
                             'file.  The windows: with --peaks the apexes, with --fitMin those at or above it, with both the apexes '
                             'at or above it.  The chi-square sums describe (sites are linked); they are no calibrated test')
    parser.add_argument('--fitBins', dest='fitBins', type=int, default=None,
                        help='MI355X build only, with --fit: distance bins of equal width in z = A |g - t| up to the cut (default 8: '
                             'about one per decade of alpha)')
    parser.add_argument('--fitClasses', dest='fitClasses', type=int, default=None,
                        help='MI355X build only, with --fit: frequency classes min(F - 1, (k F) // n) (default 10; --noFreq: the '
                             'two classes substitution / polymorphism are 0 and 1); bins times classes at most 256')
    parser.add_argument('--fitMin', dest='fitMin', type=float, default=None,
                        help='MI355X build only, with --fit: only windows with CLR >= this value (default 0)')
    parser.add_argument('--fitMax', dest='fitMax', type=int, default=None,
                        help='MI355X build only, with --fit: at most N windows per file, the N with the highest CLR (default 1000)')
    parser.add_argument('--fitMinExp', dest='fitMinExp', type=float, default=None,
                        help='MI355X build only, with --fit: cells with an expected count below this value are pooled per bin '
                             '(default 5)')
    parser.add_argument('--fitDetail', dest='fitDetail', action='store_true', default=False,
                        help='MI355X build only, with --fit: also write every cell of every selected window to <out>.fit.cells.txt')
    parser.add_argument('--conditional', dest='conditional', action='store_true', default=False,
                        help='MI355X build only, with --peaks: conditional CLRs of neighbouring apexes of the observed scan.  Every '
                             'apex gets as parent the highest apex above it within --condSpan; its surface is computed again with '
                             'the parent\'s fitted model, held at its grid argmax and not refitted, in place of neutrality at the '
                             'sites both reach, and the parent\'s given the apex.  <out>.conditional.txt next to each output file '
                             'gives per apex the parent, the shared sites, the conditional maximum and the share of the '
                             'unconditional maximum it retains.  Sites are linked: the share describes, it is no test')
    parser.add_argument('--condSpan', dest='condSpan', type=float, default=None,
                        help='MI355X build only, with --conditional: a parent lies within this distance, in the units of the test '
                             'positions (default: the sum of the two fitted reaches alpha_cut / A_hat, so the footprints can share '
                             'a site)')
    parser.add_argument('--condMin', dest='condMin', type=float, default=None,
                        help='MI355X build only, with --conditional: only apexes with CLR >= this value get a row (parents are '
                             'still chosen among all apexes)')
    parser.add_argument('--condSurfaces', dest='condSurfaces', action='store_true', default=False,
                        help='MI355X build only, with --conditional: also write the conditional surface of every apex that has a '
                             'parent to <out>.conditional.surfaces.txt, in the format of --surfaces')
    parser.add_argument('--stepwise', dest='stepwise', action='store_true', default=False,
                        help='MI355X build only, with --peaks: forward stepwise conditional selection of the apexes of the observed '
                             'scan.  The highest apex is accepted at its grid argmax, every other apex is computed again given all '
                             'accepted loci, the best of what is left is accepted, until nothing reaches --stepMin or --stepMax loci '
                             'are in.  <out>.stepwise.txt next to each output file gives per apex its order of entry, the '
                             'conditional maximum, the share of the unconditional maximum it retains and the running log ratio of '
                             'the accepted loci against neutrality.  Greedy; loci are never refitted; the threshold is no test')
    parser.add_argument('--stepMin', dest='stepMin', type=float, default=None,
                        help='MI355X build only, with --stepwise: an apex enters only with a conditional maximum >= this value '
                             '(default: the value of --peakMin, else 0; --nullPerm\'s genome-wide threshold is the natural choice)')
    parser.add_argument('--stepMax', dest='stepMax', type=int, default=None,
                        help='MI355X build only, with --stepwise: at most this many loci are accepted per file (default 1000)')
    parser.add_argument('--stepSurfaces', dest='stepSurfaces', action='store_true', default=False,
                        help='MI355X build only, with --stepwise: also write every accepted apex\'s surface at entry to '
                             '<out>.stepwise.surfaces.txt, in the format of --surfaces')
    parser.add_argument('--sandwich', dest='sandwich', action='store_true', default=False,
                        help='MI355X build only: sandwich (Godambe) standard errors of selected windows of the observed scan.  At each '
                             'window\'s fitted point (the refined point with --refine, else the grid argmax) H is the sum of the outer '
                             'products of the per-site scores and J that of their sums over blocks of --sandwichBlock consecutive '
                             'sites; <out>.sandwich.txt next to each output file gives the standard errors of x, ln alpha_beta and '
                             'ln A from H^-1 J H^-1 and from H^-1 alone, lambda = tr(H^-1 J) / p and CLR / lambda.  Needs --peaks G '
                             '(the apexes) or --sandwichMin C.  The point is not re-optimised: the numbers describe, they are no test')
    parser.add_argument('--sandwichBlock', dest='sandwichBlock', type=int, default=None,
                        help='MI355X build only, with --sandwich: sites per block of the score sums, consecutive in the input '
                             '(default 1: J equals H)')
    parser.add_argument('--sandwichMin', dest='sandwichMin', type=float, default=None,
                        help='MI355X build only, with --sandwich: only windows with CLR >= this value (default 0)')
    parser.add_argument('--sandwichMax', dest='sandwichMax', type=int, default=None,
                        help='MI355X build only, with --sandwich: at most N windows per file, the N with the highest CLR (default 1000)')
    parser.add_argument('--sandwichStep', dest='sandwichStep', type=str, default=None,
                        help='MI355X build only, with --sandwich: hx,hv, the steps of the central differences of the selection table '
                             'in x and in ln alpha_beta (default 0.001,0.01); a second pass at twice the steps gives fd_rel')
    parser.add_argument('--locate', dest='locate', type=int, default=0,
                        help='MI355X build only, with --peaks: R >= 2 bootstrap replicates of the grid scan around every apex.  Each '
                             'replicate gives every block of --locateBlock consecutive sites a Poisson(1) weight, scans the '
                             'resampled chromosome at the test positions within --locateSpan of the apexes and records where each '
                             'peak\'s maximum falls; <out>.locate.txt holds, per apex, the percentile interval of that position (as '
                             'rows of the main output), its standard deviation, the share of replicates at the apex and at the ends '
                             'of the range, and the percentile ends of the replicate maxima; default 0: off')
    parser.add_argument('--locateSeed', dest='locateSeed', type=int, default=None,
                        help='MI355X build only, with --locate: seed of the weights (default 1; its stream is separate from '
                             '--bootSeed\'s and --nullSeed\'s)')
    parser.add_argument('--locateBlock', dest='locateBlock', type=int, default=None,
                        help='MI355X build only, with --locate: sites per block (default 1).  B should span the linkage disequilibrium '
                             'of the data; B = 1 resamples sites as if they were independent and gives intervals as narrow as that')
    parser.add_argument('--locateSpan', dest='locateSpan', type=float, default=None,
                        help='MI355X build only, with --locate: half-width H of the search range around every apex, in the units '
                             '--peaks measures in (default: --peaks\' G).  A large p_edge says H was too small')
    parser.add_argument('--locateLevel', dest='locateLevel', type=float, default=None,
                        help='MI355X build only, with --locate: level L of the percentile ends, 0 < L < 1 (default 0.95)')
    parser.add_argument('--locateMin', dest='locateMin', type=float, default=None,
                        help='MI355X build only, with --locate: only apexes with CLR >= this value (default: all apexes)')
    parser.add_argument('--locateReps', dest='locateReps', action='store_true', default=False,
                        help='MI355X build only, with --locate: also write the argmax of every replicate of every peak to '
                             '<out>.locate.reps.txt')
    parser.add_argument('--power', dest='power', type=int, default=0,
                        help='MI355X build only: planted-signal power analysis with this many replicates (>= 2; 0: off).  Every '
                             'replicate redraws the derived counts of the sites within reach of evenly spaced centres from the '
                             'mixture of the grid point --plant, scans the neighbourhoods and compares each maximum with the '
                             'thresholds; <out>.power.txt holds, per centre, the power and how well the locus is placed')
    parser.add_argument('--plant', dest='plant', type=str, default=None,
                        help='MI355X build only, with --power: the planted grid point A,x,abeta (values of the run\'s grids)')
    parser.add_argument('--plantEvery', dest='plantEvery', type=float, default=None,
                        help='MI355X build only, with --power: spacing D of the centres in the units of the test positions '
                             '(default 1.05 x the smallest spacing at which the loci do not disturb each other)')
    parser.add_argument('--powerSpan', dest='powerSpan', type=float, default=None,
                        help='MI355X build only, with --power: half-width H of the range searched around every centre (default '
                             '--peaks\' G when given, else the reach of the planted A)')
    parser.add_argument('--powerSeed', dest='powerSeed', type=int, default=None,
                        help='MI355X build only, with --power: seed of the draws (default 1; its stream is separate from the '
                             'other seeds\')')
    parser.add_argument('--powerBackground', dest='powerBackground', type=str, default=None,
                        help='MI355X build only, with --power: perm (default; the rows are permuted in blocks of --powerBlock '
                             'sites before planting) or obs (the observed rows)')
    parser.add_argument('--powerBlock', dest='powerBlock', type=int, default=None,
                        help='MI355X build only, with --power: sites per block of the perm background (default 1)')
    parser.add_argument('--powerThreshold', dest='powerThreshold', type=str, default=None,
                        help='MI355X build only, with --power: CLR thresholds C[,C...]; with --nullPerm the run\'s own genome-wide '
                             '5%% and 1%% thresholds are added')
    parser.add_argument('--powerReps', dest='powerReps', action='store_true', default=False,
                        help='MI355X build only, with --power: also write every replicate of every centre to <out>.power.reps.txt')
    return parser


# ------------------------------------------------------------------------------------------------------------ refusals
# Every <feature>_refusal(opt) returns the message that refuses the command line in that feature's name, or None when the
# feature can run or is off.  Each is the list of its checks in the order they are asked, built from the five checks below and
# the feature's own; the values of its flags are judged by <feature module>.value_refusal.  main() asks the features in a fixed
# order and prints the first message (tests/test_cli_refusals_cpu.py holds every message and the precedence).

def given(v, default):
    """The value of a flag whose parser default is None (not given), or the default."""
    return v if v is not None else default


def when(fault, message):
    return message if fault else None


def orphan(opt, feature, dests):
    """A flag of `feature` (by destination, which is its name) that was given although the feature is off."""
    for d in dests:
        if getattr(opt, d) is not None and getattr(opt, d) is not False:
            return '--%s needs %s.' % (d, feature)
    return None


def helper_mode(opt, feature):
    return when(opt.getSpec or opt.getConfig, '%s scans the input; it cannot be combined with --getSpect / --getConfig.' % feature)


def no_output(opt, feature, files):
    return when(not opt.outfile, '%s needs -o: the %s written next to the output.' % (feature, files))


def multi_rank(feature):
    return when(int(os.environ.get('WORLD_SIZE', '1')) > 1 or os.environ.get('BMX_FORCE_DIST') == '1',
                '%s runs in a single process; multi-rank launches are not supported.' % feature)


def window_mode(opt, feature, why):
    return when(opt.w != 0 or opt.size, '%s needs the default window mode (no -w, no --fixWinSize): %s' % (feature, why))


def power_refusal(opt):
    """--power / --plant* / --power*.  Whether --plant names grid values is asked once the grids are known (planted_point)."""
    if not opt.power:
        return orphan(opt, '--power', ('plant', 'plantEvery', 'powerSpan', 'powerSeed', 'powerBackground', 'powerBlock',
                                       'powerThreshold', 'powerReps'))
    from . import power
    return (power.value_refusal(opt.power, opt.plantEvery, opt.powerSpan, opt.powerBlock, opt.powerBackground, opt.powerThreshold)
            or when(opt.plant is None, '--power needs --plant A,x,abeta: the grid point whose mixture the sites are drawn from.')
            or when(opt.powerThreshold is None and not opt.nullPerm,
                    '--power needs --powerThreshold C[,C...] or --nullPerm (whose genome-wide thresholds it then uses).')
            or helper_mode(opt, '--power')
            or window_mode(opt, '--power', 'the replicates are scanned with every window holding all sites.')
            or no_output(opt, '--power', 'power file is')
            or multi_rank('--power'))


def power_span(opt):
    """--powerSpan, else --peaks' G, else None (power.py then takes the reach of the planted A)."""
    return given(opt.powerSpan, opt.peaks)


def planted_point(opt, grid):
    """(iA, ix, ia) of --plant in the grids' scan order; the run is refused, with the grids printed, unless it names grid values."""
    from . import power
    xs, abetas, As = grid.scan_order()
    try:
        planted = power.parse_plant(opt.plant, As, xs, abetas)
    except ValueError as e:
        print(e)
        sys.exit(1)
    if opt.plantEvery is not None:      # refused before anything is scanned
        A_plant = float(As[planted[0]])
        H = given(power_span(opt), power.ALPHA_CUT / A_plant)
        bound = power.bound_of(H, float(min(As)), A_plant)
        if opt.plantEvery < bound:
            print(power.spacing_refusal(opt.plantEvery, bound))
            sys.exit(1)
    return planted


def write_power(opt, ctx, sel, outfile, ts, genpos, planted, null_maxima, say, f=0):
    """<outfile>.power.txt (with --powerReps <outfile>.power.reps.txt) of one file (input-file ordinal f) whose sites are in
    ctx's selected slot; null_maxima: the genome-wide maxima of --nullPerm's replicates, or None."""
    from . import null, power
    thr = power.parse_thresholds(opt.powerThreshold) if opt.powerThreshold is not None else []
    if null_maxima is not None:
        for t in (null.threshold(null_maxima, 0.95), null.threshold(null_maxima, 0.99)):
            if t not in thr:            # (few replicates: the two levels may name one maximum)
                thr.append(t)
    line_of_row = np.asarray(ts.order, dtype=np.int64) + 1 if ts.na_rows else None
    try:
        n, mean = power.power_and_write(ctx, outfile, ts, genpos, sel.model, sel.grid_A, planted, thr, opt.power,
                                        given(opt.powerSeed, 1), opt.powerBackground or 'perm', given(opt.powerBlock, 1),
                                        power_span(opt), opt.plantEvery, f, opt.powerReps, line_of_row,
                                        ([f'{v}' for v in sel.grid_x], [f'{v}' for v in sel.grid_abeta], [f'{v}' for v in sel.grid_A]))
    except ValueError as e:
        print(e)
        sys.exit(1)
    say(f'\n{datetime.now()}. Power: {n} centre/s, {opt.power} replicates -> {power.output_name(outfile)}; mean power '
        + ', '.join('%r: %s' % (float(C), 'NA' if m != m else repr(m)) for C, m in zip(thr, mean)))


def locate_refusal(opt):
    """--locate / --locate*.  Asked before the other features' refusals, so that a command line with --locate is refused in
    --locate's name."""
    if not opt.locate:
        return orphan(opt, '--locate', ('locateSeed', 'locateBlock', 'locateSpan', 'locateLevel', 'locateMin', 'locateReps'))
    from . import locate
    return (locate.value_refusal(opt.locate, opt.locateBlock, opt.locateSpan, opt.locateLevel, opt.locateMin)
            or helper_mode(opt, '--locate')
            or when(opt.peaks is None, '--locate needs --peaks G: the intervals are drawn around the apexes of the peak call.')
            or window_mode(opt, '--locate', 'windows that count sites or nucleotides are not defined on a resampled site array.')
            or no_output(opt, '--locate', 'locate file is')
            or multi_rank('--locate'))


def write_locate(opt, ctx, outfile, ts, called, say, f=0):
    """<outfile>.locate.txt (with --locateReps <outfile>.locate.reps.txt) of one file (input-file ordinal f) whose observed scan
    and peak call (`called`) have just run on ctx's selected slot."""
    from . import locate
    n, empty = locate.locate_and_write(ctx, outfile, ts, called, opt.locate, given(opt.locateSeed, 1), given(opt.locateBlock, 1),
                                       given(opt.locateSpan, opt.peaks), given(opt.locateLevel, locate.LEVEL), opt.locateMin, f,
                                       opt.locateReps)
    say(f'\n{datetime.now()}. Position bootstrap: {n} peak/s, {opt.locate} replicates -> {locate.output_name(outfile)}')
    if empty:
        say(f'--locate: {empty} replicate/s drew weight 0 for every site and have no track.')


def surfaces_refusal(opt):
    """--surfaces / --surfaceMin / --surfaceMax."""
    if not opt.surfaces:
        return orphan(opt, '--surfaces', ('surfaceMin', 'surfaceMax'))
    from . import surfaces
    return (surfaces.value_refusal(opt.surfaceMin, opt.surfaceMax)
            or when(opt.peaks is None and opt.surfaceMin is None,
                    '--surfaces needs --peaks G (the surfaces of the apexes) or --surfaceMin C (of the windows with CLR >= C): '
                    'the surface of every window of a chromosome is never what is meant.')
            or helper_mode(opt, '--surfaces')
            or no_output(opt, '--surfaces', 'surfaces file is')
            or multi_rank('--surfaces'))


def write_surfaces(opt, ctx, sel, outfile, ts, called, say):
    """<outfile>.surfaces.txt of one file whose observed scan (and peak call: `called`, or None without --peaks) has just run
    on ctx's selected slot."""
    from . import surfaces
    n, dropped = surfaces.surfaces_and_write(ctx, outfile, ts, sel, given(opt.surfaceMin, 0.0), given(opt.surfaceMax, surfaces.MAX_WINDOWS),
                                             called[0]['row'] if called is not None else None)
    say(f'\n{datetime.now()}. Surfaces: {n} window/s -> {surfaces.output_name(outfile)}')
    if dropped:
        say(f'--surfaceMax: {dropped} more window/s qualified and were dropped (the {n} with the highest CLR are kept).')


def influence_refusal(opt):
    """--influence / --influenceBlock / --influenceMin / --influenceMax / --influenceDetail."""
    if not opt.influence:
        return orphan(opt, '--influence', ('influenceBlock', 'influenceMin', 'influenceMax', 'influenceDetail'))
    from . import influence
    return (influence.value_refusal(opt.influenceBlock, opt.influenceMin, opt.influenceMax)
            or when(opt.peaks is None and opt.influenceMin is None,
                    '--influence needs --peaks G (the jackknife of the apexes) or --influenceMin C (of the windows with CLR >= C): '
                    'the jackknife of every window of a chromosome is never what is meant.')
            or helper_mode(opt, '--influence')
            or no_output(opt, '--influence', 'influence file is')
            or multi_rank('--influence'))


def write_influence(opt, ctx, sel, outfile, ts, data, called, say):
    """<outfile>.influence.txt (with --influenceDetail <outfile>.influence.blocks.txt) of one file whose observed scan (and peak
    call: `called`, or None without --peaks) has just run on ctx's selected slot."""
    from . import influence
    B = given(opt.influenceBlock, 1)
    n, dropped = influence.influence_and_write(ctx, outfile, ts, sel, data, B, given(opt.influenceMin, 0.0),
                                               given(opt.influenceMax, influence.MAX_WINDOWS),
                                               called[0]['row'] if called is not None else None, opt.influenceDetail)
    say(f'\n{datetime.now()}. Influence: {n} window/s, blocks of {B} site/s -> {influence.output_name(outfile)}')
    if dropped:
        say(f'--influenceMax: {dropped} more window/s qualified and were dropped (the {n} with the highest CLR are kept).')


def fit_refusal(opt):
    """--fit / --fitBins / --fitClasses / --fitMin / --fitMax / --fitMinExp / --fitDetail."""
    if not opt.fit:
        return orphan(opt, '--fit', ('fitBins', 'fitClasses', 'fitMin', 'fitMax', 'fitMinExp', 'fitDetail'))
    from . import fit
    return (fit.value_refusal(opt.fitBins, opt.fitClasses, opt.fitMin, opt.fitMax, opt.fitMinExp, opt.nofreq)
            or when(opt.peaks is None and opt.fitMin is None,
                    '--fit needs --peaks G (the fit of the apexes) or --fitMin C (of the windows with CLR >= C): '
                    'the table of every window of a chromosome is never what is meant.')
            or helper_mode(opt, '--fit')
            or no_output(opt, '--fit', 'fit file is')
            or multi_rank('--fit'))


def write_fit(opt, ctx, sel, outfile, ts, called, say):
    """<outfile>.fit.txt (with --fitDetail <outfile>.fit.cells.txt) of one file whose observed scan (and peak call: `called`, or
    None without --peaks) has just run on ctx's selected slot."""
    from . import fit
    D, F = given(opt.fitBins, fit.BINS), given(opt.fitClasses, fit.CLASSES)
    n, dropped = fit.fit_and_write(ctx, outfile, ts, sel, D, F, given(opt.fitMin, 0.0), given(opt.fitMax, fit.MAX_WINDOWS),
                                   given(opt.fitMinExp, fit.MIN_EXP), called[0]['row'] if called is not None else None, opt.fitDetail)
    say(f'\n{datetime.now()}. Fit: {n} window/s, {D} distance bin/s x {F} frequency class/es -> {fit.output_name(outfile)}')
    if dropped:
        say(f'--fitMax: {dropped} more window/s qualified and were dropped (the {n} with the highest CLR are kept).')


def conditional_refusal(opt):
    """--conditional / --condSpan / --condMin / --condSurfaces."""
    if not opt.conditional:
        return orphan(opt, '--conditional', ('condSpan', 'condMin', 'condSurfaces'))
    from . import conditional
    return (conditional.value_refusal(opt.condSpan, opt.condMin)
            or when(opt.peaks is None, '--conditional needs --peaks G: it conditions every apex of the peak call on its neighbour.')
            or helper_mode(opt, '--conditional')
            or no_output(opt, '--conditional', 'conditional file is')
            or multi_rank('--conditional'))


def write_conditional(opt, ctx, sel, outfile, ts, called, say):
    """<outfile>.conditional.txt (with --condSurfaces <outfile>.conditional.surfaces.txt) of one file whose observed scan and
    peak call (`called`) have just run on ctx's selected slot."""
    from . import conditional
    n, with_parent = conditional.conditional_and_write(ctx, outfile, ts, sel, called[0]['row'], opt.condSpan, opt.condMin, opt.condSurfaces)
    say(f'\n{datetime.now()}. Conditional: {n} apex/es, {with_parent} with a parent -> {conditional.output_name(outfile)}')


def stepwise_refusal(opt):
    """--stepwise / --stepMin / --stepMax / --stepSurfaces."""
    if not opt.stepwise:
        return orphan(opt, '--stepwise', ('stepMin', 'stepMax', 'stepSurfaces'))
    from . import stepwise
    return (stepwise.value_refusal(opt.stepMin, opt.stepMax)
            or when(opt.peaks is None, '--stepwise needs --peaks G: it selects among the apexes of the peak call.')
            or helper_mode(opt, '--stepwise')
            or no_output(opt, '--stepwise', 'stepwise file is')
            or multi_rank('--stepwise'))


def write_stepwise(opt, ctx, sel, outfile, ts, data, called, say):
    """<outfile>.stepwise.txt (with --stepSurfaces <outfile>.stepwise.surfaces.txt) of one file whose observed scan and peak call
    (`called`) have just run on ctx's selected slot.  Returns the rows written (for the genome-wide table)."""
    from . import stepwise
    C = given(opt.stepMin, given(opt.peakMin, 0.0))
    rows, accepted, total = stepwise.stepwise_and_write(ctx, outfile, ts, sel, data.genPos, called[0]['row'], C,
                                                        given(opt.stepMax, stepwise.MAX_LOCI), opt.stepSurfaces)
    say(f'\n{datetime.now()}. Stepwise: {len(rows)} apex/es, {accepted} accepted (threshold {float(C)!r}), T_total {total!r} -> '
        f'{stepwise.output_name(outfile)}')
    return rows


def sandwich_refusal(opt):
    """--sandwich / --sandwichBlock / --sandwichMin / --sandwichMax / --sandwichStep."""
    if not opt.sandwich:
        return orphan(opt, '--sandwich', ('sandwichBlock', 'sandwichMin', 'sandwichMax', 'sandwichStep'))
    from . import sandwich
    return (sandwich.value_refusal(opt.sandwichBlock, opt.sandwichMin, opt.sandwichMax, opt.sandwichStep)
            or when(opt.peaks is None and opt.sandwichMin is None,
                    '--sandwich needs --peaks G (the standard errors of the apexes) or --sandwichMin C (of the windows with CLR >= C): '
                    'the variance of every window of a chromosome is never what is meant.')
            or helper_mode(opt, '--sandwich')
            or no_output(opt, '--sandwich', 'sandwich file is')
            or multi_rank('--sandwich'))


def write_sandwich(opt, ctx, sel, outfile, ts, called, say):
    """<outfile>.sandwich.txt of one file whose observed scan (its peak call: `called`, or None without --peaks; with --refine its
    refinement) has just run on ctx's selected slot."""
    from . import sandwich
    B = given(opt.sandwichBlock, 1)
    hx, hv = sandwich.parse_step(opt.sandwichStep) if opt.sandwichStep is not None else (sandwich.HX, sandwich.HV)
    try:
        n, dropped = sandwich.sandwich_and_write(ctx, outfile, ts, sel, B, given(opt.sandwichMin, 0.0), given(opt.sandwichMax, sandwich.MAX_WINDOWS),
                                                 hx, hv, called[0]['row'] if called is not None else None, bool(opt.refine))
    except ValueError as e:
        print(e)
        sys.exit(1)
    say(f'\n{datetime.now()}. Sandwich: {n} window/s, blocks of {B} site/s -> {sandwich.output_name(outfile)}')
    if dropped:
        say(f'--sandwichMax: {dropped} more window/s qualified and were dropped (the {n} with the highest CLR are kept).')


def peaks_refusal(opt):
    """--peaks / --peakMin / --peakExtent / --atPeaks.  Asked before the refusals of the features that do not need the peaks,
    so that a command line with --peaks is refused in this feature's name."""
    if opt.peaks is None:
        return orphan(opt, '--peaks', ('peakMin', 'peakExtent', 'atPeaks'))
    from . import peaks
    return (peaks.value_refusal(opt.peaks, opt.peakMin, opt.peakExtent)
            or helper_mode(opt, '--peaks')
            or no_output(opt, '--peaks', 'peak file is')
            or multi_rank('--peaks')
            or when(opt.atPeaks and not opt.refine, '--atPeaks needs --refine: it restricts the refinement to the apexes.'))


def call_peaks(opt, ctx, ts):
    """The peaks of one file whose observed scan has just run on ctx's selected slot (before anything scans the slot again):
    (peaks, line of every track row in the main output or None for line t + 1)."""
    from . import peaks
    if len(ts) == 0:
        return peaks.empty(), None
    pk = ctx.peaks(opt.peaks, given(opt.peakMin, 0.0), given(opt.peakExtent, peaks.FRAC))
    return pk, (np.asarray(ts.order, dtype=np.int64) + 1 if ts.na_rows else None)


def write_peaks(outfile, called, with_null):
    """<outfile>.peaks.txt, once all its columns are known (with the null: after its p-value file).  Returns its rows."""
    from . import peaks
    pk, line_of_row = called
    return peaks.write_peaks(peaks.output_name(outfile), outfile, pk, line_of_row, outfile + '.pval.txt' if with_null else None)


def refine_refusal(opt):
    """--refine / --refineMin."""
    if not opt.refine:
        return orphan(opt, '--refine', ('refineMin',))
    return (when(opt.refineMin is not None and opt.refineMin != opt.refineMin, '--refineMin takes a number.')
            or helper_mode(opt, '--refine')
            or no_output(opt, '--refine', 'refined file is')
            or multi_rank('--refine'))


def write_refined(opt, ctx, outfile, ts, f=0):
    """<outfile>.refined.txt (with --support <outfile>.support.txt, with --boot <outfile>.boot.txt) of one file (input-file
    ordinal f) whose observed scan has just run on ctx's selected slot."""
    from . import refine
    min_clr = given(opt.refineMin, 0.0)         # --supportMin and --bootMin fall back to it
    refine.refine_and_write(ctx, outfile, ts, min_clr)
    if opt.support:
        from . import support
        support.support_and_write(ctx, outfile, ts, given(opt.supportDrop, support.DROP), given(opt.supportMin, min_clr))
    if opt.boot:
        from . import boot
        boot.boot_and_write(ctx, outfile, ts, opt.boot, given(opt.bootSeed, 1), given(opt.bootBlock, 1), given(opt.bootLevel, boot.LEVEL),
                            given(opt.bootMin, min_clr), f, opt.bootReps)


def boot_refusal(opt):
    """--boot / --boot*.  Asked before refine_refusal, so that a command line with --boot is refused in --boot's name; the
    number of replicates is judged first, the values of the other flags last."""
    if not opt.boot:
        return orphan(opt, '--boot', ('bootSeed', 'bootBlock', 'bootLevel', 'bootMin', 'bootReps'))
    from . import boot
    return (boot.value_refusal(opt.boot)
            or helper_mode(opt, '--boot')
            or when(not opt.refine, '--boot needs --refine: the replicates start at the refined maxima.')
            or no_output(opt, '--boot', 'bootstrap file is')
            or multi_rank('--boot')
            or boot.value_refusal(opt.boot, opt.bootBlock, opt.bootLevel, opt.bootMin))


def support_refusal(opt):
    """--support / --supportDrop / --supportMin.  --refine's own refusals come first (refine_refusal)."""
    if not opt.support:
        return orphan(opt, '--support', ('supportDrop', 'supportMin'))
    from . import support
    return (when(not opt.refine, '--support needs --refine: the intervals are drawn around the refined maxima.')
            or support.value_refusal(opt.supportDrop, opt.supportMin))


def profiles_refusal(opt):
    """--profiles."""
    if opt.profiles is None:
        return None
    from . import profiles
    try:
        profiles.parse(opt.profiles)
    except ValueError as e:
        return str(e)
    return helper_mode(opt, '--profiles') or no_output(opt, '--profiles', 'profile files are') or multi_rank('--profiles')


def profile_names(opt):
    from . import profiles
    return profiles.parse(opt.profiles) if opt.profiles is not None else ()


def write_profiles(opt, ctx, sel, outfile, ts):
    """The profile files of one file whose observed scan has just run on ctx's selected slot."""
    from . import profiles
    grids = {'A': list(sel.grid_A), 'x': list(sel.grid_x), 'abeta': list(sel.grid_abeta)}
    profiles.fetch_and_write(ctx, profile_names(opt), outfile, ts, grids)


def null_refusal(opt):
    """--nullPerm / --nullBlock."""
    if not opt.nullPerm:
        return None
    return (when(opt.nullPerm < 0, '--nullPerm takes a number of replicates >= 1 (0: off).')
            or when(opt.nullBlock < 1, '--nullBlock must be >= 1.')
            or helper_mode(opt, '--nullPerm')
            or no_output(opt, '--nullPerm', 'null and p-value files are')
            or multi_rank('--nullPerm'))


def null_name(outspec, what):
    """<out>.null.txt of a one-file run; for several files <dir>/null.txt, or the -o pattern with `null` for {}."""
    return outspec.replace('{}', what) if '{}' in outspec else os.path.join(outspec, what + '.txt')


def null_of_file(opt, ctx, ts, f):
    """The null replicates of one file whose observed scan has just run on ctx's selected slot."""
    from . import null
    if len(ts) == 0:
        z = np.zeros(0)
        return z, z.astype(np.int32), z.astype(np.int32), np.full(opt.nullPerm, -np.inf)
    return null.run_file(ctx, opt.nullPerm, opt.nullSeed, opt.nullBlock, f)


# ------------------------------------------------------------------------------- the stages after a file's observed scan
# main() and main_many() differ in how a file reaches its Scan, in the names of the outputs and in the closing line; from there
# on both run file_stages() per file and wrap_up() over the files' records (the one-file form: a list of one record).

# One file's results that wait for all files: called = call_peaks()'s pair (None without --peaks), null = null_of_file()'s
# tuple (None without --nullPerm), waiting = (data, neut, sel) when the file's power step waits for the genome-wide null;
# stepwise: the rows of the file's stepwise table (None without --stepwise);
# ts: the test sites, kept only with --nullPerm (for the p-value file and the waiting power step) -- a whole genome's are large.
FileRecord = namedtuple('FileRecord', 'outfile ts called null waiting stepwise')


def file_stages(opt, ctx, sel, outfile, ts, data, neut, f, planted, say, stamp):
    """The additions' stages of one file (input-file ordinal f) whose observed scan has just run on ctx's selected slot and
    written outfile, in their order; what still needs every file's results is left to wrap_up()."""
    if opt.profiles is not None:
        write_profiles(opt, ctx, sel, outfile, ts)
        ctx.set_profiles(0)         # the observed scan's profiles only: the scans of --nullPerm, --locate and --power stay as they are
        stamp('file %d: profiles' % (f + 1))
    called = None
    if opt.peaks is not None:
        called = call_peaks(opt, ctx, ts)
        ctx.refine_at_peaks(opt.atPeaks)
        stamp('file %d: peaks' % (f + 1))
    if opt.surfaces:
        write_surfaces(opt, ctx, sel, outfile, ts, called, say)
        stamp('file %d: surfaces' % (f + 1))
    if opt.influence:
        write_influence(opt, ctx, sel, outfile, ts, data, called, say)
        stamp('file %d: influence' % (f + 1))
    if opt.fit:
        write_fit(opt, ctx, sel, outfile, ts, called, say)
        stamp('file %d: fit' % (f + 1))
    if opt.conditional:
        write_conditional(opt, ctx, sel, outfile, ts, called, say)
        stamp('file %d: conditional' % (f + 1))
    step_rows = None
    if opt.stepwise:
        step_rows = write_stepwise(opt, ctx, sel, outfile, ts, data, called, say)
        stamp('file %d: stepwise' % (f + 1))
    if opt.refine:
        write_refined(opt, ctx, outfile, ts, f)
        stamp('file %d: refine' % (f + 1))
    if opt.sandwich:
        write_sandwich(opt, ctx, sel, outfile, ts, called, say)
        stamp('file %d: sandwich' % (f + 1))
    if opt.locate:
        write_locate(opt, ctx, outfile, ts, called, say, f)
        stamp('file %d: locate' % (f + 1))
    null = None
    if opt.nullPerm:
        # per-file permutations are independent (key of file ordinal f): only the host copies of this file's observed CLR and
        # counts stay until the genome-wide maxima are known
        null = null_of_file(opt, ctx, ts, f)
        stamp('file %d: permutation null' % (f + 1))
    waiting = None
    if opt.power and opt.nullPerm:
        waiting = (data, neut, sel)         # its thresholds wait for the last file's null
    elif opt.power:
        write_power(opt, ctx, sel, outfile, ts, data.genPos, planted, None, say, f)
        stamp('file %d: power' % (f + 1))
    return FileRecord(outfile, ts if opt.nullPerm else None, called, null, waiting, step_rows)


def wrap_up(opt, ctx, records, planted, say, stamp, inputs=None):
    """What needs every file's results: the genome-wide null with the p-value files, the power steps that waited for its
    thresholds, and the peak tables (whose p-value columns come from the p-value files).  records: file_stages()'s, in file
    order, the last one's sites still in ctx.  inputs: the input files of the several-files form, which names the null file
    by null_name() and adds the genome-wide peak table; None: the one-file form (<out>.null.txt, no such table)."""
    gmax = None
    if opt.nullPerm:
        from . import null
        null_path = null_name(opt.outfile, 'null') if inputs is not None else opt.outfile + '.null.txt'
        gmax = np.full(opt.nullPerm, -np.inf)           # a replicate's genome-wide maximum: the maximum over the files
        for rec in records:
            gmax = np.maximum(gmax, rec.null[3])
        null.write_null(null_path, gmax)
        for rec in records:
            null.write_pval(rec.outfile + '.pval.txt', rec.ts, *rec.null[:3], gmax)
        say(f'\n{datetime.now()}. Permutation null: {opt.nullPerm} replicates (seed {opt.nullSeed}, blocks of {opt.nullBlock} site/s) -> {null_path}')
        say('Genome-wide CLR threshold, 5%% level: %r' % null.threshold(gmax, 0.95))
        say('Genome-wide CLR threshold, 1%% level: %r' % null.threshold(gmax, 0.99))
        stamp('permutation null')
    held = records[-1]
    for f, rec in enumerate(records):
        if rec.waiting is not None:
            data, neut, sel = rec.waiting
            if rec is not held:             # the file's sites (and its model, where it differs) go back into the context
                sel.rebind(neut, ctx)
                held = rec
            write_power(opt, ctx, sel, rec.outfile, rec.ts, data.genPos, planted, gmax, say, f)
            stamp('file %d: power' % (f + 1))
    if opt.peaks is not None:
        tables = [write_peaks(rec.outfile, rec.called, bool(opt.nullPerm)) for rec in records]
        where = opt.outfile + '.peaks.txt'
        if inputs is not None:
            from . import peaks
            where = null_name(opt.outfile, 'peaks')
            peaks.write_genome(where, [(os.path.basename(i), t) for i, t in zip(inputs, tables)])
        say(f'\n{datetime.now()}. Peaks: {sum(len(t) for t in tables)} (separation {opt.peaks!r}) -> {where}')
    if opt.stepwise and inputs is not None:
        from . import stepwise
        stepwise.write_genome(null_name(opt.outfile, 'stepwise'), [(os.path.basename(i), rec.stepwise) for i, rec in zip(inputs, records)])


def main(argv=None):
    import time
    t_start = time.time()
    stamp = (lambda what: print('[bmx cli] %-28s %.3f s' % (what, time.time() - t_start), file=sys.stderr)) \
        if os.environ.get('BMX_TRACE') else (lambda what: None)
    argv = sys.argv[1:] if argv is None else argv
    parser = build_parser()
    if len(argv) == 0:
        parser.print_help()
        sys.exit()
    opt = parser.parse_args(argv)
    if opt.infile is None and opt.inputs is None:
        parser.error('the following arguments are required: -i/--input')
    refused = power_refusal(opt) or locate_refusal(opt) or conditional_refusal(opt) or stepwise_refusal(opt) or peaks_refusal(opt) or surfaces_refusal(opt) or null_refusal(opt) or profiles_refusal(opt) or boot_refusal(opt) or refine_refusal(opt) or support_refusal(opt) or influence_refusal(opt) or fit_refusal(opt) or sandwich_refusal(opt)
    if refused:
        print(refused)
        sys.exit(1)
    files = None
    if opt.inputs is not None:
        if opt.getSpec or opt.getConfig:
            print('--inputs lists files to scan; --getSpect / --getConfig take ONE concatenated input with -i (as in the reference).')
            sys.exit(1)
        files = input_list(opt.inputs)
    elif ',' in opt.infile and not os.path.exists(opt.infile):
        files = [p for p in opt.infile.split(',') if p]
    if files is not None and not (opt.getSpec or opt.getConfig):
        return main_many(opt, files, stamp)

    from . import helpers
    if opt.getSpec:
        print('You\'ve chosen to generate site frequency spectrum...')
        print(('Concatenated input: %s \nSpectrum file: %s' % (opt.infile, opt.spectfile)))
        helpers.getSpect(opt.infile, opt.spectfile, opt.MAF, opt.nosub)
        sys.exit()
    elif opt.getConfig:
        print('You\'ve chosen to generate the substitution-polymorphism configuration...')
        print(('Concatenated input: %s \nConfiguration file: %s' % (opt.infile, opt.spectfile)))
        helpers.getConfig(opt.infile, opt.spectfile)
        sys.exit()

    from . import distributed, engine
    from .hostmodel import Grids, InputData, NeutralSFS
    from .scan import Scan

    world = distributed.World.from_env(backend=os.environ.get('BMX_DIST_BACKEND'))
    if world.distributed and opt.device is not None:
        # torch tensors of the gather and the scan context must live on the same GPU: one rank, one GPU
        print('--device cannot be combined with a multi-process launch: each rank uses GPU LOCAL_RANK.')
        sys.exit(1)
    device = opt.device if opt.device is not None else world.device_index
    verbose = world.rank == 0

    def say(*a):
        if verbose:
            print(*a)

    stamp('imports, process group')
    # The HIP runtime and the context take ~0.2 s to come up: start them now, on a helper thread, while this thread reads
    # the input and the helper file (the native calls release the GIL); engine.NormalizedBetaBinom picks the context up.
    import threading
    warm = {}

    def _warm():
        try:
            warm['ctx'] = engine.Context(device)
        except Exception as e:          # reported by the main thread where the reference-style flow creates the context
            warm['err'] = e

    warm_thread = threading.Thread(target=_warm)
    warm_thread.start()
    say(f"\n{datetime.now()}. Reading input from {opt.infile}")
    data = InputData(opt.infile, opt.nofreq, opt.MAF, opt.nosub, opt.minCount, phys=opt.phys, Rrate=opt.Rrate)
    Neutral = NeutralSFS(opt.spectfile, opt.nofreq, opt.MAF, opt.nosub)
    say(f'\n{datetime.now()}. Initializing...')
    say('Retrieving per-site neutral probabilities...')
    Neutral.get_neut_probs(data)
    grid = Grids(opt.x, opt.abeta, opt.bal, opt.pos, opt.seqA, opt.listA)
    planted = planted_point(opt, grid) if opt.power else None
    say('\nOptimizing over x= ' + ', '.join(['%g' % (x) for x in grid.x]))
    say('\n \t alpha= ' + ', '.join([str(a) for a in grid.abeta]))
    say('\n \t A= ' + ', '.join([str(A) for A in grid.A]))
    stamp('input, neutral model, grids')
    warm_thread.join()
    if 'err' in warm:
        raise warm['err']
    stamp('HIP context ready')
    pnames = profile_names(opt)
    if pnames:
        from . import profiles
        warm['ctx'].set_profiles(profiles.mask(pnames))
    Sel_Probs = engine.NormalizedBetaBinom(data, grid, opt.nofreq, opt.MAF, opt.nosub, device=device, ctx=warm['ctx'])
    say(("\n%s. Start computing likelihood ratios..." % (datetime.now())))
    # BMX_SHARD_BLOCK: test sites per shard block (default distributed.BLOCK = 4096; a multiple of 16 keeps every window's
    # arithmetic independent of the number of ranks) -- lets small inputs exercise real sharding in the tests
    runner = world.sharded_runner(block=shard_block(), balance=os.environ.get('BMX_SHARD_BALANCE') == '1') if world.distributed else None
    sc = Scan(data, Neutral, Sel_Probs, grid, opt.outfile if world.rank == 0 else None, fixSize=opt.size, r=opt.w,
              s=opt.step, phys=opt.phys, noCenter=opt.noCenter, runner=runner, verbose=verbose, keep_results=False)
    stamp('table, scan, output')
    rec = file_stages(opt, Sel_Probs.ctx, Sel_Probs, opt.outfile, sc.test_sites, data, Neutral, 0, planted, say, stamp)
    wrap_up(opt, Sel_Probs.ctx, [rec], planted, say, stamp)
    world.finish()
    say(f'\n{datetime.now()}. Pipeline finished.')


def shard_block():
    """BMX_SHARD_BLOCK: test sites per shard block of a multi-rank run (default distributed.BLOCK = 4096).  A multiple of 16
    keeps group boundaries -- hence every window's arithmetic -- independent of the number of ranks; small values let small
    inputs exercise real sharding in the tests."""
    v = os.environ.get('BMX_SHARD_BLOCK')
    if not v:
        return None
    try:
        block = int(v)
    except ValueError:
        block = 0
    if block < 16 or block % 16:
        print('BMX_SHARD_BLOCK must be a positive multiple of 16.')
        sys.exit(1)
    return block


def input_list(path):
    """The files named in an --inputs list: one per line, blank lines and lines starting with # skipped, relative names taken
    relative to the list's own directory."""
    here = os.path.dirname(os.path.abspath(path))
    with open(path) as f:
        names = [l.strip() for l in f]
    return [n if os.path.isabs(n) else os.path.join(here, n) for n in names if n and not n.startswith('#')]


def output_name(outspec, infile):
    """-o of the multi-file form: a pattern containing {} (the input's basename without extension goes there) or a directory."""
    base = os.path.basename(infile)
    if '{}' in outspec:
        return outspec.replace('{}', os.path.splitext(base)[0])
    return os.path.join(outspec, base + '.out.txt')


def main_many(opt, files, stamp=lambda what: None):
    """Several input files through the reference's stages (InputData -> NeutralSFS.get_neut_probs -> NormalizedBetaBinom ->
    Scan, BalLeRMix+_v1.py:777-799) in one process on one scan context: file i + 1 is read and given its neutral
    probabilities on a helper thread while file i is scanned and written (the native calls release the GIL)."""
    import threading
    from . import distributed, engine
    from .hostmodel import Grids, InputData, NeutralSFS
    from .scan import Scan
    if not files:
        print('No input files given.')
        sys.exit(1)
    if not opt.outfile:
        print('Several input files need -o <directory> or -o <pattern with {}>.')
        sys.exit(1)
    world = distributed.World.from_env(backend=os.environ.get('BMX_DIST_BACKEND'))
    if world.distributed and opt.device is not None:
        print('--device cannot be combined with a multi-process launch: each rank uses GPU LOCAL_RANK.')
        sys.exit(1)
    device = opt.device if opt.device is not None else world.device_index
    verbose = world.rank == 0

    def say(*a):
        if verbose:
            print(*a)

    outs = [output_name(opt.outfile, f) for f in files]
    if len(set(outs)) != len(outs):
        print('Two input files map to the same output name; give -o a pattern with {} or distinct basenames.')
        sys.exit(1)
    if world.rank == 0:
        for d in sorted(set(os.path.dirname(os.path.abspath(o)) for o in outs)):
            os.makedirs(d, exist_ok=True)
    grid = Grids(opt.x, opt.abeta, opt.bal, opt.pos, opt.seqA, opt.listA)
    planted = planted_point(opt, grid) if opt.power else None
    say('\nOptimizing over x= ' + ', '.join(['%g' % (x) for x in grid.x]))
    say('\n \t alpha= ' + ', '.join([str(a) for a in grid.abeta]))
    say('\n \t A= ' + ', '.join([str(A) for A in grid.A]))
    runner = world.sharded_runner(block=shard_block(), balance=os.environ.get('BMX_SHARD_BALANCE') == '1') if world.distributed else None
    nxt = {}

    def host_stage(i):
        try:
            data = InputData(files[i], opt.nofreq, opt.MAF, opt.nosub, opt.minCount, phys=opt.phys, Rrate=opt.Rrate)
            neut = NeutralSFS(opt.spectfile, opt.nofreq, opt.MAF, opt.nosub)
            neut.get_neut_probs(data)
            # the host half of NormalizedBetaBinom (model arrays, every site's table row) here too: no device call
            sel = engine.NormalizedBetaBinom(data, grid, opt.nofreq, opt.MAF, opt.nosub, device=device).prepare(neut)
            nxt[i] = (data, neut, sel)
        except BaseException as e:          # incl. the reference-style sys.exit() of the readers: re-raised on the main thread
            nxt[i] = e

    th = threading.Thread(target=host_stage, args=(0,))
    th.start()
    ctx = engine.Context(device)        # HIP start-up (0.2-0.3 s) while the first file is being read
    pnames = profile_names(opt)
    if pnames:
        from . import profiles
        pmask = profiles.mask(pnames)
    tables = 0
    kernel_ms = 0.0
    records = []
    for i, (infile, outfile) in enumerate(zip(files, outs)):
        th.join()
        got = nxt.pop(i)
        if isinstance(got, BaseException):
            raise got
        data, neut, sel = got
        if i + 1 < len(files):
            th = threading.Thread(target=host_stage, args=(i + 1,))
            th.start()
        say(f"\n{datetime.now()}. {infile} -> {outfile}")
        if pnames:
            ctx.set_profiles(pmask)         # (switched off after the previous file's observed scan)
        sc = Scan(data, neut, sel, grid, outfile if world.rank == 0 else None, fixSize=opt.size, r=opt.w, s=opt.step, phys=opt.phys,
                  noCenter=opt.noCenter, runner=runner, verbose=verbose, keep_results=False, reuse_ctx=ctx)
        ctx = sel.ctx
        tables += 0 if sel.table_reused else 1
        try:
            kernel_ms += ctx.last_scan_ms()
        except Exception:           # a file without test sites
            pass
        stamp('file %d of %d' % (i + 1, len(files)))
        records.append(file_stages(opt, ctx, sel, outfile, sc.test_sites, data, neut, i, planted, say, stamp))
    wrap_up(opt, ctx, records, planted, say, stamp, inputs=files)
    world.finish()
    say(f'\n{datetime.now()}. Pipeline finished: {len(files)} files, selection table built {tables} time(s), '
        f'scan kernels {kernel_ms / 1e3:.2f} s.')


if __name__ == '__main__':
    main()
    sys.stdout.flush()
    sys.stderr.flush()
    if os.environ.get('BMX_FAST_EXIT', '1') != '0':       # see BalLeRMixPlus_amd.py
        os._exit(0)
