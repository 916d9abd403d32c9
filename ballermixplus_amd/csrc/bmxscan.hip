// bmxscan.hip -- libbmxscan.so: gfx950 kernels + C ABI (include/bmxscan.h).
//
// Hot path being replaced (reference BalLeRMix+_v1.py, "v1:LINE"):
//   K1  bb_lut_kernel              <- NormalizedBetaBinom.__init__/get_raw_probs/get_*_normBase  v1:319-433
//   K2  prep_kernel + clr_scan_prepared_kernel    <- calcBaller, J = 16 / 8 test sites per wave-group (what ships for dense
//                                     test sites; round 3)                                                  v1:436-507
//       prep_solo_kernel + clr_scan_solo_kernel    <- calcBaller, one test site per wave (sparse or unsorted test sites)
//       clr_scan_grouped_kernel, clr_scan_kernel  round 2's single-kernel forms: variants 12 / 2 (cross-checks in the
//                                     tests), and the path for tables of 4 GiB and more
//       locate_kernel / finalize_kernel: test-site positions, per-slice argmax merge + nSites
//       surface_kernel             <- the full T[A,x,alpha] surface of one site (v1:449-450 wish)
//       surfaces_kernel, cond_surfaces_kernel, base_surfaces_kernel    <- the same surfaces for a list of test sites in
//                                     one launch: plain (bmx_ctx_surfaces), given one fitted neighbouring locus each
//                                     (bmx_ctx_cond_surfaces) and against a per-site baseline of any number of accepted loci
//                                     (bmx_ctx_base_surfaces); one body, listed_surface, with influence_argmax_kernel for the maxima
//       baseline_add_kernel        <- adds a locus to that baseline (bmx_ctx_baseline_*)
//       influence_kernel          <- every leave-one-block-out maximum of those surfaces (bmx_ctx_influence), with
//                                     influence_range_kernel and influence_argmax_kernel
//       fit_kernel                 <- observed against expected spectrum by distance of listed windows (bmx_ctx_fit)
//       sandwich_kernel           <- score sums, outer-product H and block-sum J of listed windows at given points
//                                     (bmx_ctx_sandwich); refine_R_kernel <- one off-grid table column (bmx_ctx_refine_R)
//
// The shipped library reads ONE environment variable, BMX_TRACE (stage messages on stderr, no effect on results).
// Tuning knobs for A/B runs (BMX_LDS_PAD, BMX_DENSE_GAP, BMX_SOLO_GAP, BMX_FORCE_J, BMX_FAR_EPS, BMX_MOM_SLOTS, BMX_SPB,
// BMX_ROWMAX_GLOBAL) exist only in the diagnostic builds (-DBMX_DIAG: `make diag|prof|count`); the scan variant is chosen with
// bmx_ctx_set_variant().
//
// K2 formulation.  For a test site t and linkage value A the reference sums, over the sites
// i of the window with alpha_i = exp(-A*|g_i - t|) >= 1e-8 and g_i != t (v1:454-457),
//     log(alpha_i*S_i + (1-alpha_i)*g_i) - log(g_i)              (v1:494-499)
// which equals log(1 + alpha_i*R[x,a][row_i]) with R = S*prop/g - 1 tabulated per (k,n) row.
// The scan keeps, per lane, the running PRODUCT  prod_i (1 + alpha_i*R)  (one FMA and one
// MUL per site and grid pair, no transcendental), pulls the binary exponent out of the product
// every few sites so it cannot over/underflow, and takes a single log per (t, A, pair).
// Lanes run over the (x, alpha_beta) pairs, so nothing is reduced across lanes until the
// final argmax.  Far from the test sites (alpha*|R| small: three quarters of a window) not even that: the sites'
// alpha^k are added to per-row moments and the product picks up exp(sum_k +-w_k F^k sum_rows R^k M_k)
// -- the log1p series with economised coefficients (order 12 on |x| <= 0.15 in the prepared kernels, order 8 on
// |x| <= 0.05 in the solo and round-2 kernels).  Since round 3 everything that does not depend on the pair -- positions,
// exp(-A d), the near / far decision, the moments, where each window ends -- is computed ONCE per group of test sites by a
// lanes-over-sites kernel (prep_kernel) and streamed through HBM to the pair-parallel waves (see "K2, prepared" below).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <dlfcn.h>
#include <errno.h>
#include <float.h>
#include <rccl/rccl.h>     // types only: the library is opened with dlopen when a gather is first asked for

#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <type_traits>
#include <string>
#include <thread>
#include <unordered_set>
#include <vector>

#include "../../include/bmxscan.h"
#include "bmx_math.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(BMX_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));       \
    } while (0)

// BMX_TRACE=1 in the environment prints one line per stage to stderr (diagnostics only)
// tuning knobs: environment variables in diagnostic builds, always absent in the shipped library
const char *diag_env(const char *name) {
#ifdef BMX_DIAG
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

bool trace_on() {
    static int on = -1;
    if (on < 0) on = getenv("BMX_TRACE") ? 1 : 0;
    return on == 1;
}
#define TRACE(...)                                   \
    do {                                             \
        if (trace_on()) {                            \
            fprintf(stderr, "[bmx] " __VA_ARGS__);   \
            fprintf(stderr, "\n");                   \
            fflush(stderr);                          \
        }                                            \
    } while (0)

constexpr int WAVE = 64;
constexpr int SCAN_THREADS = 256;             // 4 waves per workgroup (default)
constexpr int SCAN_THREADS_MAX = 512;         // 8 waves when one R slice fills most of a CU's LDS
constexpr int SCAN_THREADS_J8 = 768;          // 12 waves = 3 per SIMD: the prepared kernel's 8-test-site form (168 registers)
constexpr int SITE_THREADS = 1024;            // per-site kernel: 16 waves per workgroup, two workgroups per CU = 8 waves per SIMD
                                              // (62 VGPRs; the kernel is latency-bound per pass and lives on occupancy)
constexpr int LDS_LIMIT_BYTES = 160 * 1024;   // gfx950: 160 KiB per CU
constexpr int MOM_SLOTS = 254;                // grouped kernel: rows whose far-field sites can be summed as moments
constexpr int MOM_SLOTS_LDS = 64;             // ... of which this many are used while the R slice occupies the LDS
#ifndef BMX_PAIR_PREFETCH
#define BMX_PAIR_PREFETCH (!USE_LDS)      // pair blocks one block ahead: pays for R from global memory only (LDS: 64.22 vs 64.03 ms)
#endif
#ifndef BMX_PPAIR_PREFETCH
#define BMX_PPAIR_PREFETCH 1              // prepared kernel, pair blocks one block ahead: round 4 (no spills, 13 spare VGPRs): +0.4 % with the table in LDS too
#endif
#ifndef BMX_FOLD_RPRE
#define BMX_FOLD_RPRE (!USE_LDS)          // rows of a fold batch requested with its moments: global memory only (LDS: 64.51 vs 64.03 ms)
#endif
#ifndef BMX_FOLD_EARLY
#define BMX_FOLD_EARLY (!USE_LDS)         // prepared kernel's fold: heads and R of the next two slots requested before this step's powers
#endif
#ifndef BMX_LIST_TAILS
#define BMX_LIST_TAILS 1                  // prepared kernel's near lists: no pair step of two neutral entries, short forms for quad tails of 1 or 2
#endif
#ifndef BMX_MIDTRI
#define BMX_MIDTRI 1
#endif
#ifndef BMX_XCD_MAP
#define BMX_XCD_MAP 1     // prepared kernel: the slices of a chunk of test sites on one XCD (4.168 -> 4.205 M windows/s, HBM reads / 8)
#endif
#ifndef BMX_SOLO_XCD_MAP
#define BMX_SOLO_XCD_MAP 1     // the slices of a chunk of test sites on one XCD: the chunk's streams come out of HBM once, not eight times
#endif
#ifndef BMX_PRIV01
#define BMX_PRIV01 1
#endif
#ifndef BMX_FAR_ORDER
#define BMX_FAR_ORDER 8
#endif
constexpr int FAR_ORDER = BMX_FAR_ORDER;      // ... to this power of alpha*R (log1p series): 4, 6 or 8
#ifndef BMX_MOM_COPIES
#define BMX_MOM_COPIES 8
#endif
constexpr int MOM_COPIES = BMX_MOM_COPIES;                 // copies of the most frequent row's moments (lane % 8): fewer LDS conflicts
#ifndef BMX_QSB
#define BMX_QSB 8
#endif
#ifndef BMX_FOLD_BATCH
#define BMX_FOLD_BATCH 2
#endif
constexpr int SITE_SCR = 72;                  // per-site kernel: two lists of at most 64 sites, each padded to a multiple of four
constexpr int SCR_CAP = 80;                   // grouped kernel: entries of a wave's scratch list: up to 64 pending + 16 neutral ones (padding of the
                                              // last block of 4 or 8 and what the block loops read one block ahead -- R from global memory must
                                              // never see a stale row reference)
constexpr int MID_CAP = 32;                   // grouped kernel: sites between the test sites of a group staged in LDS (12 B each)
constexpr int FAR_CAP = 8192;                 // ... at most this many sites per zone (exponent budget: 8192 * 0.05 * 1.49 bits < 1000)
constexpr double LN2 = 0.693147180559945309417232121458;
// Far field: log1p(x) = sum_k (-1)^(k+1) w_k x^k.  To 8th order the w_k are the Taylor coefficients 1/k economised on
// [-0.05, 0.05] (Taylor polynomial of degree 24 re-expanded in Chebyshev polynomials of x/0.05, cut after T_8, constant
// term -1.9e-17 dropped): max error 8.9e-16 on the whole interval, against 2.3e-13 for the plain Taylor cut -- Taylor's
// accuracy at |x| <= 0.0296 with the far field starting 0.5 units of A*d nearer to the test sites.  Lanes that drop
// high orders (x^k/k < 2e-15) see w_k - 1/k only as |w_1 - 1| |x| + |w_2 - 1/2| x^2 + ... < 1e-17.  Lower orders: Taylor.
#if BMX_FAR_ORDER >= 8
__device__ constexpr double FAR_W[8] = {0.9999999999998467, 0.4999999999996164, 0.3333333341509627, 0.25000000122701976,
                                        0.19999882322703955, 0.16666529319200146, 0.1434841013671569, 0.12562715480255862};
#else
__device__ constexpr double FAR_W[8] = {1.0, 0.5, 0.3333333333333333, 0.25, 0.2, 0.16666666666666666, 0.14285714285714285, 0.125};
#endif

// ----------------------------------------------------------------------------- K1
struct LutParams {
    int stat, min_count, n_sizes, rows, nx, nab, NP;
    const int32_t *sizes;
    const int32_t *row_off;
    const double *g;
    const double *prop;
    const double *x;
    const double *abeta;
    double *psel;  // [nx][nab][rows]
    double *R;     // [nx][nab][rows]
    double *Rt;    // [rows][NP]   kernel layout: pair index fastest, zero padded
    bmx::LogPatch patch;   // host-libm conformance exceptions for lgam's log (bmx_math.h)
};

// One thread per (grid pair, LUT row).  The thread needs the beta-binomial pmf at the site's own
// count (folded / B_1 forms, v1:375-396) and at the counts excluded from the support
// (v1:399-433), each for b(x) and b(1-x).  All of them go through ONE inlined pmf call site
// inside nested loops: the pmf body is large, and gfx950 device-function calls from a partially
// active wave proved unusable here (hang), so nothing in this kernel is an out-of-line call.
__global__ __launch_bounds__(128) void bb_lut_kernel(LutParams P) {   // 128 threads per workgroup: room for 512 registers, no scratch
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int npairs = P.nx * P.nab;
    if (gid >= (int64_t)npairs * P.rows) return;
    int p = (int)(gid / P.rows), r = (int)(gid % P.rows);
    int ix = p / P.nab, ia = p % P.nab;
    int j = 0;
    while (j + 1 < P.n_sizes && r >= P.row_off[j + 1]) j++;
    const int n = P.sizes[j], k = r - P.row_off[j];
    const double x = P.x[ix], a = P.abeta[ia];
    const double xm = 1. - x;
    const double b1 = a / x - a, b2 = a / xm - a;                 // v1:316
    const int m = P.min_count, stat = P.stat;
    const bool maf = (stat == BMX_STAT_B2MAF || stat == BMX_STAT_B0MAF);
    int nex = m;                                                  // excluded counts, v1:399-433
    if (stat == BMX_STAT_B2MAF) nex += (m - 1 > 0 ? m - 1 : 0);
    if (stat == BMX_STAT_B0) nex += 1;
    if (stat == BMX_STAT_B0MAF) nex += m;
    // numpy's pairwise summation of the excluded probabilities, streamed (np.sum, v1:402): below 8 elements a plain loop, from 8 on
    // eight accumulators over the whole blocks of 8, combined as a tree, then the tail one by one.  That is numpy's order up to
    // 128 elements.  Above 128 numpy halves the array (first half rounded down to a multiple of 8) and sums each half this way;
    // the kernel keeps ONE run of eight accumulators (refine_R too).  Measured on the device against scipy at nex = 139 (B_2,MAF
    // n = 1001, min_count 70) and nex = 130 (B_0,MAF n = 400, min_count 65): 60 % / 75 % of the well-conditioned entries
    // bit-equal (56 .. 85 % at nex = 8 .. 24), worst relative difference 1.1e-15 / 2.2e-15 against a bar of 1e-12
    // (tests/test_gpu_seltable.py), so the split is not reproduced.
    const int nblk = nex < 8 ? 0 : nex - (nex % 8);
    double r8[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
    double res = 0.;
    double raw = 0.;
    for (int it = 0; it <= nex; ++it) {
        const bool site = (it == nex);
        int c;
        if (site) c = (stat == BMX_STAT_B1) ? n : k;              // B_1 uses pmf(n) (v1:382)
        else if (it < m) c = it;
        else if (stat == BMX_STAT_B0) c = n;
        else c = n - m + 1 + (it - m);
        const int nfold = (site && maf) ? 2 : 1;                  // pmf(k) + pmf(n-k)  (v1:389)
        double v[2];
        for (int side = 0; side < 2; ++side) {
            const double b = side ? b2 : b1;
            double pr = 0.;
            for (int f = 0; f < nfold; ++f) {
                const double q = bmx::betabinom_pmf(f ? n - c : c, n, a, b, P.patch);
                pr = f ? pr + q : q;
            }
            if (site && maf && (n % 2 == 0) && c == n / 2) pr = pr / 2;      // v1:391-392
            if (site && stat == BMX_STAT_B1) pr = (k == 0) ? pr : (1. - pr - pr);
            v[side] = pr;
        }
        const double e = 0.5 * (v[0] + v[1]);
        if (site) {
            raw = e;
        } else if (nex < 8) {
            res += e;
        } else if (it < nblk) {
            if (it < 8) r8[it] = e; else r8[it & 7] += e;
            if (it == nblk - 1)
                res = ((r8[0] + r8[1]) + (r8[2] + r8[3])) + ((r8[4] + r8[5]) + (r8[6] + r8[7]));
        } else {
            res += e;
        }
    }
    const double base = 1. - res;
    const double psel = raw / base;
    const size_t o = ((size_t)ix * P.nab + ia) * P.rows + r;
    const double R = psel * P.prop[j] / P.g[r] - 1.0;
    P.psel[o] = psel;
    P.R[o] = R;
    P.Rt[(size_t)r * P.NP + p] = R;
}

// ----------------------------------------------------------------------------- locate
__global__ void locate_kernel(const double *genpos, int64_t N, const double *test_gen, int64_t M,
                              int64_t *center, int64_t *center_hi) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= M) return;
    double v = test_gen[t];
    int64_t a = 0, b = N;
    while (a < b) {
        int64_t m = (a + b) >> 1;
        if (genpos[m] < v) a = m + 1; else b = m;
    }
    center[t] = a;  // first index with genpos >= test position
    b = N;
    while (a < b) {
        int64_t m = (a + b) >> 1;
        if (genpos[m] <= v) a = m + 1; else b = m;
    }
    center_hi[t] = a;  // first index with genpos > test position (sites in between are ties)
}

// window bounds of the all-sites mode (set_tests without bounds): every window is [0, N - 1]
__global__ void all_sites_kernel(int64_t *lo, int64_t *hi, int64_t M, int64_t N) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= M) return;
    lo[k] = 0;
    hi[k] = N - 1;
}

// index gaps between neighbouring test sites at a strided sample of all of them (set_tests: test-site density)
__global__ void gap_kernel(const int64_t *center, int64_t stride, int64_t ns, int64_t *gap) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= ns) return;
    gap[k] = center[k * stride + 1] - center[k * stride];
}

// ----------------------------------------------------------------------------- permutation null
// splitmix64: the mixer of the permutation and of its keys (ballermixplus_amd/null.py mix, bitwise)
__host__ __device__ __forceinline__ uint64_t bmx_mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// sigma(i; N, B, K) of null.block_permutation: blocks of B sites permuted by an 8-round Feistel network on 2h bits with
// cycle walking (only the first nb * B sites move; nb < 2 is the identity and never launches)
struct PermParams {
    int64_t N, B, nb;
    int h;
    uint64_t mask;
    uint64_t rk[8];        // mix(K + j), j = 0..7: the round keys, made on the host
};

__device__ __forceinline__ uint64_t feistel(uint64_t x, const PermParams &Q) {
    uint64_t L = x >> Q.h, R = x & Q.mask;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint64_t t = R;
        R = L ^ (bmx_mix64(R ^ Q.rk[j]) & Q.mask);
        L = t;
    }
    return (L << Q.h) | R;
}

// dst[i] = src[sigma(i)]: positions stay, the (k, n) rows move; grid-stride over the N sites
template <class T>
__global__ __launch_bounds__(256) void permute_rows_kernel(const T *__restrict__ src, T *__restrict__ dst, PermParams Q) {
    const int64_t moved = Q.nb * Q.B;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < Q.N; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t j = i;
        if (i < moved) {
            const int64_t b = i / Q.B;
            uint64_t x = feistel((uint64_t)b, Q);
            while (x >= (uint64_t)Q.nb) x = feistel(x, Q);      // a cycle of the permutation leads back into [0, nb)
            j = (int64_t)x * Q.B + (i - b * Q.B);
        }
        dst[i] = src[j];
    }
}

constexpr int NULL_THREADS = 256;
constexpr int NULL_BLOCKS_MAX = 1024;

__device__ __forceinline__ double block_max(double m) {
    __shared__ double wmax[NULL_THREADS / WAVE];
    for (int o = WAVE / 2; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
    if ((threadIdx.x & (WAVE - 1)) == 0) wmax[threadIdx.x / WAVE] = m;
    __syncthreads();
    m = wmax[0];
    for (int w = 1; w < NULL_THREADS / WAVE; w++) m = fmax(m, wmax[w]);
    return m;
}

// one replicate's exceedances (every test site is one thread's: no atomics) and the first pass of its maximum CLR: one
// partial per workgroup
__global__ __launch_bounds__(NULL_THREADS) void null_count_kernel(const double *__restrict__ clr, const double *__restrict__ obs,
                                                                  int32_t *__restrict__ count, int64_t M, double *__restrict__ part) {
    double m = -INFINITY;
    for (int64_t t = (int64_t)blockIdx.x * NULL_THREADS + threadIdx.x; t < M; t += (int64_t)gridDim.x * NULL_THREADS) {
        const double v = clr[t];
        count[t] += v >= obs[t] ? 1 : 0;
        m = fmax(m, v);
    }
    m = block_max(m);
    if (threadIdx.x == 0) part[blockIdx.x] = m;
}

// second pass: the maximum of the n workgroup partials (max is exact, so the result does not depend on the split)
__global__ __launch_bounds__(NULL_THREADS) void null_max_kernel(const double *__restrict__ part, int n, double *__restrict__ out) {
    double m = -INFINITY;
    for (int k = threadIdx.x; k < n; k += NULL_THREADS) m = fmax(m, part[k]);
    m = block_max(m);
    if (threadIdx.x == 0) *out = m;
}

// LUT row of a site: 2 bytes per site normally (<= 65535 rows), 4 when the table is larger
// (hundreds of distinct sample sizes).
struct RowArray {
    const uint16_t *r16;
    const uint32_t *r32;
    __device__ __forceinline__ int operator[](int64_t i) const { return r32 ? (int)r32[i] : (int)r16[i]; }
};

// ----------------------------------------------------------------------------- K2
struct ScanParams {
    const double *genpos;
    RowArray row;
    int64_t N;
    const double *Rt;  // [rows][NP]
    int rows, NP, npairs, nslices;
    const double *A;
    int nA;
    const double *test_gen;
    const int64_t *win_lo;
    const int64_t *win_hi;
    const int64_t *center;     // first index with genpos >= test position
    const int64_t *center_hi;  // first index with genpos >  test position
    int64_t M;
    double zcut;       // alpha >= 1e-8  <=>  A*d <= zcut  (v1:455)
    int renorm_every;  // per-site kernel: sites between exponent extractions
    int span_hi;       // grouped kernel: bits by which one factor 1+alpha*R can exceed 1 (>= 1)
    double rmax;       // max(0, largest finite R of the table)
    double far_eps;    // grouped kernel, FARSUM: sites with E * rowmax[row] <= far_eps go through power sums
    // [nslices][rows]: max |R| of the row over the slice's 64 pairs, rounded up (NaN for absent rows), with the
    // row's far-field moment slot in the low mantissa byte: the rank of the row among the data's rows by
    // frequency (255: not ranked); row_of_slot is the inverse, kmom[iA] says how many slots pay at A
    const double *rowmax;
    const uint8_t *kmom;
    int row_of_slot[MOM_SLOTS];
    int row0;          // per-site kernel: the most frequent row of the data (-1: none)
    int mom_slots;     // slots per wave allocated in LDS (<= MOM_SLOTS)
    int wide_tab;      // the global R table has 2^32 bytes or more
    unsigned long long *prof;   // -DBMX_PROFILE builds: cycles per kernel section, summed over waves (else unused)
    float far_bits;    // far_eps * log2(e): exponent-budget bits per far site
    int sites_per_block;
    double *part_T;    // [nslices][M]
    int32_t *part_lin;
    int32_t *part_ns;
};

__device__ __forceinline__ double readlane_f64(double v, int l) {
    int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// exp(-z) for 0 <= z < ~700, without OCML's special-case handling: n = rint(-z*log2 e),
// r = -z - n*ln2 (two-term), degree-13 Taylor polynomial (|r| <= 0.347: truncation 4e-18), ldexp.
// ~19 instructions instead of ~34; about 1 ulp, which is all alpha needs (alpha only feeds
// log-likelihood terms; the window PREDICATE never goes through this function).
// p*r + c with the constant c in a scalar register pair.  gfx950 VALU instructions take no 64-bit literals, and left to
// itself the compiler keeps every polynomial coefficient of exp_neg (called from five places) in a VGPR pair for the whole
// kernel -- 20 VGPRs of a 256-VGPR budget -- and spends a v_mov_b64 per Horner step because it selects the two-address
// v_fmac, which overwrites its addend.  The "s" constraint makes the coefficient two s_mov_b32 (scalar issue slots,
// rematerialised wherever needed) and the step one three-address v_fma_f64.
__device__ __forceinline__ double fma_sc(double p, double r, double c) {
    double o;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(o) : "v"(p), "v"(r), "s"(c));
    return o;
}

__device__ __forceinline__ double exp_neg(double z) {
    const double t = -z;
    const double n = rint(t * 1.4426950408889634);
    double r = fma(-n, 0.6931471805599453, t);
    r = fma(-n, 2.3190468138462996e-17, r);
    double p = fma_sc(1.6059043836821613e-10, r, 2.08767569878681e-09);   // 1/13!, 1/12!
    p = fma_sc(p, r, 2.505210838544172e-08);         // 1/11!
    p = fma_sc(p, r, 2.755731922398589e-07);         // 1/10!
    p = fma_sc(p, r, 2.7557319223985893e-06);        // 1/9!
    p = fma_sc(p, r, 2.48015873015873e-05);          // 1/8!
    p = fma_sc(p, r, 0.0001984126984126984);         // 1/7!
    p = fma_sc(p, r, 0.001388888888888889);          // 1/6!
    p = fma_sc(p, r, 0.008333333333333333);          // 1/5!
    p = fma_sc(p, r, 0.041666666666666664);          // 1/4!
    p = fma_sc(p, r, 0.16666666666666666);           // 1/3!
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p, (int)n);
}

// Two independent exp_neg chains, written out interleaved: a chain of 19 dependent FP64 operations runs at the FP64
// latency (~10 cycles per step for a wave on its own), two interleaved chains at nearly the issue rate.  Used where exps
// come in batches (the far-field flush: one per test site).
__device__ __forceinline__ void exp_neg2(double z0, double z1, double &o0, double &o1) {
    const double t0 = -z0, t1 = -z1;
    const double n0 = rint(t0 * 1.4426950408889634), n1 = rint(t1 * 1.4426950408889634);
    double r0 = fma(-n0, 0.6931471805599453, t0), r1 = fma(-n1, 0.6931471805599453, t1);
    r0 = fma(-n0, 2.3190468138462996e-17, r0);
    r1 = fma(-n1, 2.3190468138462996e-17, r1);
    double p0 = fma_sc(1.6059043836821613e-10, r0, 2.08767569878681e-09), p1 = fma_sc(1.6059043836821613e-10, r1, 2.08767569878681e-09);
#define BMX_STEP2(c) p0 = fma_sc(p0, r0, c); p1 = fma_sc(p1, r1, c);
    BMX_STEP2(2.505210838544172e-08)
    BMX_STEP2(2.755731922398589e-07)
    BMX_STEP2(2.7557319223985893e-06)
    BMX_STEP2(2.48015873015873e-05)
    BMX_STEP2(0.0001984126984126984)
    BMX_STEP2(0.001388888888888889)
    BMX_STEP2(0.008333333333333333)
    BMX_STEP2(0.041666666666666664)
    BMX_STEP2(0.16666666666666666)
#undef BMX_STEP2
    p0 = fma(p0, r0, 0.5); p1 = fma(p1, r1, 0.5);
    p0 = fma(p0, r0, 1.0); p1 = fma(p1, r1, 1.0);
    p0 = fma(p0, r0, 1.0); p1 = fma(p1, r1, 1.0);
    o0 = ldexp(p0, (int)n0);
    o1 = ldexp(p1, (int)n1);
}

// Pull the binary exponent out of a non-negative product; a zero product is sticky (-> -inf).
__device__ __forceinline__ void renorm(double &acc, int &E) {
    unsigned hi = (unsigned)__double2hiint(acc);
    int e = (int)((hi >> 20) & 0x7ffu);
    E = (e == 0) ? -(1 << 28) : E + (e - 1023);
    hi = (hi & 0x800fffffu) | 0x3ff00000u;
    acc = __hiloint2double((int)hi, __double2loint(acc));
}

// The same with the hardware's frexp pair (v_frexp_exp_i32_f64 / v_frexp_mant_f64): three VALU instructions instead of six.  The
// mantissa lands in [1/2, 1) -- a convention of its own: whoever compares (exponent, mantissa) pairs must take both from this
// function -- and a zero product keeps mantissa 0 with its exponent unchanged, so the comparison has to ask for a positive mantissa.
#ifndef BMX_FREXP
#define BMX_FREXP 0     // prepared kernels: measured no gain (config-3 block 4.45 vs 4.43 M windows/s), so they keep the integer form
#endif
__device__ __forceinline__ void renorm_fx(double &acc, int &E) {
    E += __builtin_amdgcn_frexp_exp(acc);
    acc = __builtin_amdgcn_frexp_mant(acc);
}

// One (E or alpha, row * 64) entry of a wave's scratch list in LDS: written lanes-over-sites, read back with a uniform
// address (LDS broadcast) by all 64 grid-pair lanes.
struct alignas(16) ScratchEnt {
    double e;
    int ro;   // row * 64
    int pad;
};

// K2, one test site per wave: sparse test sets (the reference's -s with a large step), unsorted test positions, tables whose
// dynamic range is too wide for block-wise exponent extraction; also the independent cross-check of the grouped kernel in the
// tests.  Per A and side the wave walks the window 64 sites at a time: alpha = exp(-A d) lanes-over-sites, (alpha, row) through
// the wave's LDS scratch, then every lane (grid pair) multiplies 1 + alpha R four sites per step: 2.75 vector instructions
// per site (round 1: ~6 with v_readlane broadcasts and OCML's exp).  Best grid point tracked per lane as (exponent, mantissa),
// like the grouped kernel; finalize_kernel takes the one log and counts nSites.
template <bool USE_LDS>
__global__ __launch_bounds__(SITE_THREADS) void clr_scan_kernel(ScanParams P) {
    extern __shared__ __attribute__((aligned(16))) double lds_R[];  // [rows][64] when USE_LDS, then 64 entries per wave
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nw = blockDim.x / WAVE;
    const int slice = blockIdx.x % P.nslices;   // blocks b, b+8 share an XCD: one R slice per L2
    const int64_t chunk = blockIdx.x / P.nslices;
    const int p = slice * WAVE + lane;
    const int N = (int)P.N;

    if (USE_LDS) {
        const int total = P.rows * WAVE;
        for (int idx = threadIdx.x; idx < total; idx += blockDim.x)
            lds_R[idx] = P.Rt[(size_t)(idx >> 6) * P.NP + slice * WAVE + (idx & 63)];
        __syncthreads();
    }
    // rowoff: index of the row's first value -- row * 64 in the LDS slice, row * NP in the global table (see the grouped kernel)
    const char *Rb = reinterpret_cast<const char *>(P.Rt + slice * WAVE);
    const unsigned lane8 = (unsigned)lane * 8u;
    const int rowmul = USE_LDS ? WAVE : P.wide_tab ? 1 : P.NP;      // tables of 4 GiB and more: rowoff = row, 64-bit arithmetic per load
    auto loadR = [&](int rowoff) -> double {
        if (USE_LDS) return lds_R[rowoff + lane];
        if (P.wide_tab) return *reinterpret_cast<const double *>(Rb + ((size_t)rowoff * P.NP * 8u + lane8));
        return *reinterpret_cast<const double *>(Rb + ((unsigned)rowoff * 8u + lane8));
    };
    ScratchEnt *scr = reinterpret_cast<ScratchEnt *>(lds_R + (USE_LDS ? P.rows * WAVE : 0)) + wave * SITE_SCR;
    // The most frequent row of the data (substitutions: ~70 % of the sites) stays in a register pair: its sites go through a list
    // of their own and need no R read at all -- this kernel is bound by LDS bandwidth (512 B of R per site and slice), not by
    // arithmetic, and by L2 bandwidth when the table does not fit the LDS.
    const int row0 = P.row0;
    const double R0 = row0 >= 0 ? loadR(row0 * rowmul) : 0.0;
    auto rank = [&](unsigned long long m) {
        return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    };

    const int64_t t_begin = chunk * P.sites_per_block;
    const int64_t t_end = min(t_begin + (int64_t)P.sites_per_block, P.M);
    for (int64_t t = t_begin + wave; t < t_end; t += nw) {
        const double tg = P.test_gen[t];
        const int lo = (int)max(P.win_lo[t], (int64_t)0);
        const int hi = (int)min(P.win_hi[t], (int64_t)N - 1);
        const int c = (int)P.center[t];
        double bestM = 1.0;
        int bestEc = 131072, bestA = -1;            // clamped exponent + 2^17 of the best product so far, and its A index (-1: none yet);
                                                    // not packed into one word as in the grouped kernel: this kernel takes any nA

        for (int iA = 0; iA < P.nA; ++iA) {
            const double Aval = P.A[iA];
            double acc = 1.0;
            int E = 0, since = 0;
            for (int dir = 0; dir < 2; ++dir) {
                // dir 0: indices c, c+1, ... up to hi;  dir 1: c-1, c-2, ... down to lo
                int base = dir == 0 ? max(c, lo) : min(c - 1, hi);
                int i = dir == 0 ? base + lane : base - lane;
                double g_nx = P.genpos[min(max(i, 0), N - 1)];          // the next pass's sites are requested one pass ahead
                int r_nx = (int)P.row[min(max(i, 0), N - 1)];
                while (true) {
                    const bool valid = (i >= lo) && (i <= hi);
                    const double g = g_nx;
                    const int rraw = r_nx;
                    const int inx = dir == 0 ? i + WAVE : i - WAVE;
                    g_nx = P.genpos[min(max(inx, 0), N - 1)];
                    r_nx = (int)P.row[min(max(inx, 0), N - 1)];
                    const double z = Aval * fabs(g - tg);
                    const bool in = valid && (z <= P.zcut) && (g != tg);
                    const bool beyond = valid && (z > P.zcut);
                    const unsigned long long m_in = __ballot(in);
                    if (m_in != 0ull) {
                        // two lists in the scratch: the sites of row0 at [0, n0), the others from n0r = n0 rounded up to 4 on,
                        // each padded to a multiple of four with neutral entries (alpha = 0; the row of a site of the window, so
                        // that 0*R is 0 and never 0*NaN: rows absent from the helper file hold NaN)
                        const bool is0 = in && rraw == row0;
                        const unsigned long long m0 = __ballot(is0), m1 = m_in & ~m0;
                        const int n0 = __popcll(m0), n1 = __popcll(m1), n0r = (n0 + 3) & ~3;
                        const int pad_ro = __builtin_amdgcn_readlane(rraw, __ffsll((long long)m_in) - 1) * rowmul;
                        if (in) scr[is0 ? rank(m0) : n0r + rank(m1)] = ScratchEnt{exp_neg(z), rraw * rowmul, 0};
                        if (lane < n0r - n0) scr[n0 + lane] = ScratchEnt{0.0, pad_ro, 0};
                        if (lane < 3) scr[n0r + n1 + lane] = ScratchEnt{0.0, pad_ro, 0};
                        __builtin_amdgcn_wave_barrier();
                        for (int l = 0; l < n0; l += 4) {
                            double f[4];
#pragma unroll
                            for (int u = 0; u < 4; ++u) f[u] = fma(scr[l + u].e, R0, 1.0);       // uniform address: LDS broadcast
                            acc *= (f[0] * f[1]) * (f[2] * f[3]);
                            since += 4;
                            if (since + 4 > P.renorm_every) {
                                renorm(acc, E);
                                since = 0;
                            }
                        }
                        // (no prefetch of the next step's entries, and the entry as an 8-byte + a 4-byte read rather than one 16-byte
                        // read: with 8 waves per SIMD the LDS round trips are covered by the other waves; both variants were
                        // measured slower, by 17 % and 4 %)
                        for (int l = n0r; l < n0r + n1; l += 4) {
                            double f[4];
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                const ScratchEnt en = scr[l + u];
                                f[u] = fma(en.e, loadR(en.ro), 1.0);
                            }
                            acc *= (f[0] * f[1]) * (f[2] * f[3]);
                            since += 4;
                            if (since + 4 > P.renorm_every) {
                                renorm(acc, E);
                                since = 0;
                            }
                        }
                        __builtin_amdgcn_wave_barrier();
                    }
                    if (__ballot(beyond) != 0ull || __ballot(valid) != ~0ull) break;
                    i = inx;
                }
            }
            renorm(acc, E);
            const int ec = min(max(E, -131071), 131071) + 131072;
            if (((ec > bestEc) || (ec == bestEc && acc > bestM)) && p < P.npairs) {       // strict '>' (v1:501); iA ascending
                bestM = acc;
                bestEc = ec;
                bestA = iA;
            }
        }
        // wave argmax on (exponent, mantissa), ties to the smaller linear index = the reference's first strict
        // maximum in (A, x, alpha_beta) loop order; the logarithm is finalize_kernel's
        int bE = bestEc;
        int bL = bestA < 0 ? 0x7fffffff : bestA * P.npairs + p;
        for (int off = 32; off > 0; off >>= 1) {
            const int oE = __shfl_xor(bE, off);
            const double oM = __shfl_xor(bestM, off);
            const int oL = __shfl_xor(bL, off);
            if (oE > bE || (oE == bE && (oM > bestM || (oM == bestM && oL < bL)))) { bE = oE; bestM = oM; bL = oL; }
        }
        if (lane == 0) {
            const size_t o = (size_t)slice * P.M + t;          // [slice][M]: coalesced for writer and reader
            P.part_T[o] = bestM;
            P.part_lin[o] = bL;
            P.part_ns[o] = bE;
        }
    }
}

// ----------------------------------------------------------------------------- K2, grouped
// J consecutive test sites (a "group") share one pass over the sites around them.  A lane
// still owns one (x, alpha_beta) pair but now carries J running products, one per test site.
//
//  * bulk zones: sites that lie to the right (left) of ALL J test sites and inside ALL J
//    windows.  There  exp(-A(g_i - t_j)) = exp(-A(g_i - t_last)) * exp(-A(t_last - t_j)) = E_i * F_j
//    with F_j constant for the whole zone (scalar registers), so one LDS read of R and one
//    broadcast of (E_i, row_i) feed J FMA+MUL pairs:  v = E_i*R;  acc_j *= fma(F_j, v, 1).
//    A site within the window of the farthest test site is within all of them because FP
//    subtraction and multiplication are monotone, so the reference's predicate is kept exactly.
//  * everything else (sites between the test sites, ties, the ragged window ends) goes through
//    generic passes of 64/J sites x J test sites with the reference's formula per (site, test
//    site): alpha = exp(-(A*|g_i - t_j|)) if i in window_j and A*d <= zcut and g_i != t_j.
//
// The argmax is tracked per lane on (binary exponent, mantissa) of the product -- an exact
// ordering that needs no logarithm; one log per test site is taken at the very end.
//
//  * dense test sets (every SNP a test site): the sites between the test sites are the J test sites themselves and
//    alpha_ij = exp(-A|t_i - t_j|) separates as well (G_i H_j), so that triangle runs in the pair form below.
//
// Inner-loop forms (template parameter MODE_; 3 is what ships, 0..2 stay for A/B runs):
//   0: (E_i, row_i) and alpha_ij reach the lanes by v_readlane, one site per step.
//   1: they are staged in a wave-private LDS scratch and read back with uniform-address
//      (broadcast) ds_read, and bulk sites are taken two at a time:
//          (1 + F v1)(1 + F v2) = 1 + F*(s + F*q),   s = v1 + v2,  q = v1*v2
//      i.e. 2 FMA + 1 MUL per test site per PAIR of sites (s, q shared by all J test sites).
//   2: as 1, and list entries with alpha <= 1/2 go FOUR sites per step (see the bulk loop).
//   3: as 2, and sites with alpha*max|R| <= far_eps are not multiplied at all: their alpha^k go to per-row moments.
// Measured on gfx950 (profiles/): every VALU instruction of this kernel -- FP64 or not -- costs
// ~5-6 SIMD cycles at 2 waves/SIMD and ~10 at one, so the design minimises instruction count:
// 0.81 VALU instructions per 64 evaluations in form 3 at J = 16 (1.98 in form 2), vs ~6 in the per-site kernel.
// -DBMX_PROFILE: s_memtime stamps between the sections of the grouped kernel (diagnostic builds only; the
// stamps serialise outstanding LDS/scalar loads, so the split is approximate).  Sections: 0 sites between
// the test sites, 1 zone set-up, 2 per-pass work, 3 products over the near list, 4 ragged-end masks,
// 5 fold of the moments, 6 flush (exp per test site), 7 generic walks past the zones, 8 best-tracking per A.
#ifdef BMX_PROFILE
#define PROF_MARK(k) do { const long long now_ = clock64(); prof_[k] += now_ - tprev_; tprev_ = now_; } while (0)
#else
#define PROF_MARK(k) do { } while (0)
#endif
// -DBMX_COUNT: event counters (wave-uniform adds; no stamps), summed over waves into P.prof[16..31]
#ifdef BMX_COUNT
#define CNT(k, n) do { cnt_[k] += (unsigned long long)(n); } while (0)
#else
#define CNT(k, n) do { } while (0)
#endif

template <int J, bool USE_LDS, int MODE_>
__global__ __launch_bounds__(SCAN_THREADS_MAX) void clr_scan_grouped_kernel(ScanParams P) {
#ifdef BMX_PROFILE
    long long prof_[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    long long tprev_ = clock64();
#endif
#ifdef BMX_COUNT
    unsigned long long cnt_[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
    extern __shared__ __attribute__((aligned(16))) double lds_R[];  // [rows][64] when USE_LDS, then scratch
    constexpr int SP = WAVE / J;                                    // sites per generic pass
    constexpr bool QUAD = (MODE_ >= 2);                             // MODE_ 2 = MODE 1 + quads in far passes
    constexpr bool FARSUM = (MODE_ == 3);                           // MODE_ 3 = MODE 2 + far-field moments
    constexpr int MODE = MODE_ ? 1 : 0;
    constexpr bool MIDTRI = (MODE_ >= 2) && BMX_MIDTRI;           // dense test sets: the J x J triangle between the test sites in pair form
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // provably wave-uniform: group-level scalars live in SGPRs
    const int slice = blockIdx.x % P.nslices;
    const int64_t chunk = blockIdx.x / P.nslices;
    const int p = slice * WAVE + lane;
    const int jl = lane % J, sl = lane / J;
    const int N = (int)P.N;

    if (USE_LDS) {
        const int total = P.rows * WAVE;
        for (int idx = threadIdx.x; idx < total; idx += blockDim.x)
            lds_R[idx] = P.Rt[(size_t)(idx >> 6) * P.NP + slice * WAVE + (idx & 63)];
        for (int idx = threadIdx.x; idx < P.rows; idx += blockDim.x)
            lds_R[total + idx] = P.rowmax[(size_t)slice * P.rows + idx];
        __syncthreads();
    }
    // A row is referred to by the index of its first value: row * 64 in the LDS slice, row * NP in the global table (32 bits:
    // the host checks rows * NP * 8 < 2^31), so that either load is one address addition -- scalar base + 32-bit lane offset
    // for the global one, not a 64-bit multiply-add per load
    const char *Rb = reinterpret_cast<const char *>(P.Rt + slice * WAVE);
    const unsigned lane8 = (unsigned)lane * 8u;
    const int rowmul = USE_LDS ? WAVE : P.NP;                      // (tables of 4 GiB and more go to the per-site kernel)
    auto loadR = [&](int rowoff) -> double {
        return USE_LDS ? lds_R[rowoff + lane] : *reinterpret_cast<const double *>(Rb + ((unsigned)rowoff * 8u + lane8));
    };
    // per-row max |R| of this slice (behind the R slice), then the wave-private scratch: 64 x 16 B
    // then the wave-private scratch (64 x 16 B per wave) and the wave-private moments
    const int rows_pad = (P.rows + 1) & ~1;
    const double *rowmax = USE_LDS ? lds_R + P.rows * WAVE : P.rowmax + (size_t)slice * P.rows;
    double *lds_tail = lds_R + (USE_LDS ? P.rows * WAVE + rows_pad : 0);
    ScratchEnt *scr = reinterpret_cast<ScratchEnt *>(lds_tail) + wave * SCR_CAP;
    const int mom_len = (P.mom_slots + MOM_COPIES - 1 + 3) * FAR_ORDER;   // slot 0 in MOM_COPIES copies, slots 1.., 3 spare
    double *mom = lds_tail + (blockDim.x / WAVE) * SCR_CAP * 2 + wave * mom_len;
    // ... and the sites between the group's test sites (position, row * 64): read by the generic passes of all nA iterations
    double *mid_base = lds_tail + (blockDim.x / WAVE) * (SCR_CAP * 2 + mom_len);
    if (MODE_ == 3) {
        for (int idx = lane; idx < mom_len; idx += WAVE) mom[idx] = 0.0;
        __builtin_amdgcn_wave_barrier();
    }
    double *scr_d = reinterpret_cast<double *>(scr);

    const int64_t ngroups = (P.M + J - 1) / J;
    const int64_t gpb = P.sites_per_block / J;
    const int64_t g_end = min((chunk + 1) * gpb, ngroups);
    for (int64_t grp = chunk * gpb + wave; grp < g_end; grp += blockDim.x / WAVE) {
        const int64_t tb = grp * J;
        const int nvalid = (int)min((int64_t)J, P.M - tb);
        // the lane-derived addresses of the group prologue are recomputed per group: left loop-invariant, the compiler
        // keeps them in registers across the whole kernel and, at 256 VGPRs, in scratch
        int jl_g = jl, lane_g = lane, wave_g = wave;
        asm volatile("" : "+v"(jl_g), "+v"(lane_g), "+s"(wave_g));
        double *mid_g = mid_base + wave_g * (MID_CAP + MID_CAP / 2);
        int *mid_ro = reinterpret_cast<int *>(mid_g + MID_CAP);
        const int jj = min(jl_g, nvalid - 1);
        const double tj = P.test_gen[tb + jj];
        int lo_j = (int)max(P.win_lo[tb + jj], (int64_t)0);
        int hi_j = (int)min(P.win_hi[tb + jj], (int64_t)N - 1);
        if (jl >= nvalid) { lo_j = 1; hi_j = 0; }
        const double t0 = readlane_f64(tj, 0), tL = readlane_f64(tj, J - 1);
        const int c0 = (int)P.center[tb], cU = (int)P.center_hi[tb + nvalid - 1];
        int lo_max = 0, hi_min = N - 1;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int a = __builtin_amdgcn_readlane(lo_j, j), b = __builtin_amdgcn_readlane(hi_j, j);
            if (j < nvalid) { lo_max = max(lo_max, a); hi_min = min(hi_min, b); }
        }
        int L_int = min(c0, hi_min + 1), R_int = max(cU, lo_max);
        if (hi_min < lo_max) { L_int = c0; R_int = c0; hi_min = -1; lo_max = N; }   // no bulk zone
        // the sites between the test sites are visited once per A: keep them in LDS (global latency once per group)
        const bool staged = R_int - L_int <= MID_CAP;
        if (staged && lane_g < R_int - L_int) {
            mid_g[lane_g] = P.genpos[L_int + lane_g];
            mid_ro[lane_g] = (int)P.row[L_int + lane_g] * rowmul;
        }
        __builtin_amdgcn_wave_barrier();
        // Dense test sets: the sites between the test sites ARE the J test sites (site k at t_k, positions strictly
        // increasing, every site inside every window's index bounds).  Then alpha_ij = exp(-A|t_i - t_j|) separates into
        // G_i H_j (j < i) and H_i G_j (j > i), G_k = exp(-A(t_k - t_0)), H_k = 1/G_k, and the triangle of (site, test site)
        // pairs runs in the pair form of the bulk loops instead of generic passes (see the A loop).
        bool mid_tri = false;
        if (MIDTRI) {
            const bool same = staged && (R_int - L_int == J) && nvalid == J && lo_max <= L_int && hi_min >= R_int - 1;
            if (same) {
                const double gm = mid_g[jl_g];
                const double tprev = __shfl_up(tj, 1);
                mid_tri = __ballot(!(gm == tj && (jl_g == 0 || tj > tprev))) == 0ull;
            }
        }

        // running best per test site: key = (clamped exponent + 2^17) << 13 | iA  (iA = 8191: none yet)
        double acc[J], bestM[J];
        int E[J], bestK[J];
#pragma unroll
        for (int j = 0; j < J; ++j) { bestM[j] = 1.0; bestK[j] = (131072 << 13) | 8191; }

        for (int iA = 0; iA < P.nA; ++iA) {
            const double A = P.A[iA];
            const int kmom = MODE_ == 3 ? min((int)P.kmom[iA], P.mom_slots) : 0;
            // Exponent budget: every factor 1 + alpha*R lies in [1 - alpha, max(1, 1 + Rmax)], so a
            // block of 8 sites moves log2 of a product by at most 8*span bits, span being the
            // larger of span_hi and -log2(1 - alpha_max).  The products are pulled back to [1,2)
            // before the running total could pass 1000 bits (FP64 holds +-1022).
            int bits = 0;
#pragma unroll
            for (int j = 0; j < J; ++j) { acc[j] = 1.0; E[j] = 0; }
            auto renorm_all = [&]() {
#pragma unroll
                for (int j = 0; j < J; ++j) renorm(acc[j], E[j]);
                bits = 0;
            };
            auto spend = [&](int nbits) {
                if (bits + nbits > 1000) renorm_all();
                bits += nbits;
            };
            const int span_generic = max(P.span_hi, 54);     // alpha < 1  =>  1 - alpha >= 2^-53

            // SP sites x J test sites with per-(site, test site) alpha (lane = site slot * J + test site): acc_j *= 1 + alpha R
            auto apply_pass = [&](double alpha, int rowoff, unsigned long long m_in, double *buf) {
                if (MODE == 1) {
                    buf[lane] = alpha;
                    __builtin_amdgcn_wave_barrier();
                }
                double Rpre[SP];
                if (!USE_LDS) {               // R from global memory: all rows of the pass requested at once (lanes without a site: row 0)
#pragma unroll
                    for (int s = 0; s < SP; ++s) Rpre[s] = loadR(__builtin_amdgcn_readlane(rowoff, s * J));
                }
#pragma unroll
                for (int s = 0; s < SP; ++s) {
                    if (((m_in >> (s * J)) & ((1ull << J) - 1ull)) == 0ull) continue;
                    const double R = USE_LDS ? loadR(__builtin_amdgcn_readlane(rowoff, s * J)) : Rpre[s];
                    if (MODE == 1) {
                        const double2 *a2 = reinterpret_cast<const double2 *>(buf + s * J);
#pragma unroll
                        for (int j = 0; j < J; j += 2) {
                            const double2 a = a2[j >> 1];              // uniform address: LDS broadcast
                            acc[j] *= fma(a.x, R, 1.0);
                            acc[j + 1] *= fma(a.y, R, 1.0);
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < J; ++j) acc[j] *= fma(readlane_f64(alpha, s * J + j), R, 1.0);
                    }
                }
                if (MODE == 1) __builtin_amdgcn_wave_barrier();
            };

            // one generic pass over SP sites starting at b, stepping dir; returns "all finished"
            // (site i of the lane, its position and row; lanes with inr = false carry no site)
            auto generic_core = [&](int i, bool inr, double g, int rowoff, int dir) -> bool {
                const bool inwin = inr && i >= lo_j && i <= hi_j;
                const double z = A * fabs(g - tj);
                const bool in = inwin && (z <= P.zcut) && (g != tj);
                // a lane is finished once nothing further along the walk can be in its window; an empty
                // window (lo > hi: the padding test sites of a partial last group) is finished at once --
                // without this the left walk of a partial group runs to index 0
                const bool fin = lo_j > hi_j ||
                                 (dir > 0 ? (!inr || i > hi_j || (i >= lo_j && g > tj && z > P.zcut))
                                          : (!inr || i < lo_j || (i <= hi_j && g < tj && z > P.zcut)));
                const unsigned long long m_in = __ballot(in);
                CNT(7, 1);
                if (m_in != 0ull) {
                    CNT(6, 1);
                    const double alpha = in ? exp_neg(z) : 0.0;
                    // factors of this pass lie in [1 - a_max, 1 + a_max*Rmax]; away from the test sites
                    // (every alpha <= 1/2) that is [1/2, 2^span_hi], not the 54-bit worst case
                    spend(SP * (__ballot(in && z < 0.6931471805599453) == 0ull ? max(P.span_hi, 2) : span_generic));
                    apply_pass(alpha, rowoff, m_in, scr_d);
                }
                return __ballot(fin) == ~0ull;
            };
            auto generic_pass = [&](int b, int dir, int lim, bool from_lds) -> bool {
                const int i = b + dir * sl;
                const bool inr = dir > 0 ? (i < lim) : (i > lim);
                // both loads up front: the row is needed only when some site is in a window, but waiting for
                // the ballot would put two global round trips in series
                // (two branches, not a select between an LDS and a global address: that would be a flat load)
                double g = 0.0;
                int rowoff = 0;
                if (from_lds) {
                    if (inr) { g = mid_g[i - L_int]; rowoff = mid_ro[i - L_int]; }
                } else {
                    if (inr) { g = P.genpos[i]; rowoff = (int)P.row[i] * rowmul; }
                }
                return generic_core(i, inr, g, rowoff, dir);
            };

            // bulk zone: sites i = base, base+dir, ... ; ok(i) is a prefix property along the walk
            constexpr int ZONE_DONE = -0x7fffffff;
            auto bulk_zone = [&](int base, int dir, double tnear, double tfar) -> int {
                double F[J];
                {
                    const double fv = exp_neg(A * fabs(tnear - tj));
#pragma unroll
                    for (int j = 0; j < J; ++j) F[j] = readlane_f64(fv, j);
                }
                // the site data of the NEXT pass is requested before this pass's arithmetic starts,
                // so its L2 latency hides under ~4000 cycles of FP64 work
                int i = base + dir * lane;
                double g_nx = P.genpos[min(max(i, 0), N - 1)];
                int r_nx = (int)P.row[min(max(i, 0), N - 1)];
                int nfar_tot = 0;                                  // far-field sites of this zone (FARSUM)
                double m1p = 0.0, m2p = 0.0;                       // lane-private first and second moments of slot 0
                // MODE 1: the near list is carried from pass to pass -- entries pending in scr[0 .. fill), worked off in blocks
                // of four only when the next pass would not fit behind them or the zone has ended, so the padding of the last
                // block and the set-up of the block loops are paid once per ~60 near sites, not once per pass (~15)
                int fill = 0, pend_np = 0, pend_hi = 0, pend_lo = 0, pad_ro = 0;
                bool ended = false;
                auto rank = [&](unsigned long long m) {
                    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                };
                PROF_MARK(1);
                while (true) {
                    int cnt = 0, cnt_blk = 0, inx = i;
                    bool nearl = false;
                    double Ev = 0.0;
                    int rraw = 0;
                    if (!ended) {
                    const bool ok = dir > 0 ? (i <= hi_min) : (i >= lo_max);
                    const double g = g_nx;
                    rraw = r_nx;
                    inx = i + dir * WAVE;
                    g_nx = P.genpos[min(max(inx, 0), N - 1)];
                    r_nx = (int)P.row[min(max(inx, 0), N - 1)];
                    const bool bulk = ok && (A * fabs(g - tfar) <= P.zcut);
                    const unsigned long long mb = __ballot(bulk);
                    cnt = __popcll(mb);
                    CNT(13, 1);
                    if (cnt) {
                        CNT(0, 1);
                        CNT(14, cnt);
                        Ev = bulk ? exp_neg(A * fabs(g - tnear)) : 0.0;
                        cnt_blk = cnt;                                  // sites left to the block loops
                        if (MODE == 1) {
                            // FARSUM.  A site is FAR when alpha*|R| <= far_eps for every pair of the slice and every
                            // test site (alpha = E F <= E) and its row is one of the kmom most frequent rows of the
                            // data (substitutions, singletons, ...: nearly all sites).  For those,
                            //   sum_i log1p(F v_i) = sum_k (-1)^(k+1) F^k/k * sum_rows R[row]^k M_k[row],  M_k = sum_i E_i^k,
                            // so the pass only adds E, E^2, .. E^8 to the row's moments in LDS -- lane-parallel over
                            // the sites, nothing per pair -- and the zone's end folds the moments into the product.
                            bool moml = false;
                            if (FARSUM && kmom) {
                                const double ri = rowmax[rraw];                 // row's max |R|, its moment slot in the low byte
                                const int slot = __double2loint(ri) & 0xff;
                                const double xr = Ev * ri;
                                moml = bulk && slot < kmom && xr <= P.far_eps && nfar_tot < FAR_CAP;
                                const unsigned long long mm = __ballot(moml);
                                const int nfar = __popcll(mm);
                                PROF_MARK(10);
                                if (nfar) {
                                    if (moml) {
                                        // most sites carry the most frequent row (substitutions): its moments are kept in
                                        // MOM_COPIES copies so that one ds_add_f64 does not serialise ~45 lanes on one address
                                        double *mr = mom + (slot ? slot + MOM_COPIES - 1 : (lane & (MOM_COPIES - 1))) * FAR_ORDER;   // slot 0 = copies 0..C-1
                                        // ds_add_f64 costs ~0.65 FMA slots per active lane (scripts/ubench_lds_atomic), so a
                                        // lane only adds the powers it needs: x^k/k < 2e-15 is dropped (x = E * rowmax >= |F v|)
                                        const double E2 = Ev * Ev;
                                        if (BMX_PRIV01 && slot == 0) {
                                            // the most frequent row (70 % of the sites): first and second moments -- the two every far
                                            // site adds -- in two registers of the lane, joined to the LDS copies at the fold
                                            m1p += Ev;
                                            m2p += E2;
                                        } else {
                                            atomicAdd(mr, Ev);
                                            atomicAdd(mr + 1, E2);
                                        }
                                        if (xr > 1.8e-5) {
                                            const double E3 = E2 * Ev;
                                            atomicAdd(mr + 2, E3);
                                            if (xr > 3.0e-4) {
                                                const double E4 = E2 * E2;
                                                atomicAdd(mr + 3, E4);
                                                if (FAR_ORDER >= 6 && xr > 1.6e-3) {
                                                    atomicAdd(mr + 4, E4 * Ev);
                                                    if (xr > 4.8e-3) {
                                                        atomicAdd(mr + 5, E4 * E2);
                                                        if (FAR_ORDER >= 8 && xr > 0.0105) {
                                                            atomicAdd(mr + 6, E4 * E3);
                                                            if (xr > 0.0189) atomicAdd(mr + 7, E4 * E4);
                                                        }
                                                    }
                                                }
                                            }
                                        }
                                    }
                                    PROF_MARK(11);
                                    nfar_tot += nfar;
                                    cnt_blk = cnt - nfar;
                                    CNT(5, nfar);
                                }
                            }
                            nearl = bulk && !moml;
                            PROF_MARK(2);
                        } else {
                            int rowoff = rraw * rowmul;
                            rowoff = bulk ? rowoff : __builtin_amdgcn_readlane(rowoff, 0);
                            const double e0 = readlane_f64(Ev, 0);
                            const double om = 1.0 - e0, op = fma(e0, P.rmax, 1.0);
                            const int lowbits = 1024 - ((__double2hiint(om) >> 20) & 0x7ff);
                            const int hibits = ((__double2hiint(op) >> 20) & 0x7ff) - 1022;
                            const int span8 = 8 * min(max(hibits, lowbits), 125);
                            for (int l0 = 0; l0 < cnt; l0 += 8) {
                                spend(span8);
#pragma unroll
                                for (int u = 0; u < 8; ++u) {
                                    const int l = l0 + u;           // lanes >= cnt carry Ev = 0: factor 1
                                    const double v = readlane_f64(Ev, l) * loadR(__builtin_amdgcn_readlane(rowoff, l));
#pragma unroll
                                    for (int j = 0; j < J; ++j) acc[j] *= fma(F[j], v, 1.0);
                                }
                            }
                        }
                    }
                    }
                    if (MODE == 1) {
                        if (fill > 0 && (ended || fill + cnt_blk > WAVE - 4)) {
                            CNT(1, 1);
                            CNT(4, fill);
                            // neutral entries (E = 0, the row of a site of the zone: 0*R is 0, not 0*NaN from a row absent in the
                            // helper file) behind the list: the padding of the last block and what the loops read one block ahead
                            if (lane < 16) scr[fill + lane] = ScratchEnt{0.0, pad_ro, 0};
                            __builtin_amdgcn_wave_barrier();
                            // every factor of the pending sites lies in [1 - E0, 1 + E0*Rmax], E0 the largest alpha among them
                            const int span8 = 8 * min(max(pend_hi, pend_lo), 125);
                            constexpr int BS = J >= 16 ? 4 : 8;        // sites per unrolled block
                            // Sites with alpha <= 1/2 (factors >= 1/2: the expanded product is well conditioned) are
                            // taken FOUR per step:
                            //   prod_m (1 + F v_m) = 1 + F e1 + F^2 e2 + F^3 e3 + F^4 e4   (Horner in F),
                            // e_k = elementary symmetric polynomials of v_1..v_4 shared by all J test sites:
                            // 4 FMA + 1 MUL per test site per four sites.  The near list is ordered by distance, so the
                            // entries with E > 1/2 are a prefix: they go two per step (below), rounded up to whole blocks.
                            const int npair = !QUAD ? fill : min(fill, (pend_np + BS - 1) & ~(BS - 1));
                            const int span8q = 8 * min(max(pend_hi, 2), 125);
                            PROF_MARK(9);
                            if (QUAD && npair < fill) {
                                // the R rows of the NEXT four sites are requested before this block's arithmetic, so the
                                // two dependent LDS round trips (list entry -> row) of a block hide under the previous one
                                double Rn[4], en_e[4];
#pragma unroll
                                for (int u = 0; u < 4; ++u) {
                                    const ScratchEnt en = scr[min(npair + u, SCR_CAP - 1)];
                                    en_e[u] = en.e;
                                    Rn[u] = loadR(en.ro);
                                }
                                for (int l0 = npair; l0 < fill; l0 += 4) {
                                    CNT(2, 1);
                                    spend(span8q / 2);
                                    double v[4];
#pragma unroll
                                    for (int u = 0; u < 4; ++u) v[u] = en_e[u] * Rn[u];
#pragma unroll
                                    for (int u = 0; u < 4; ++u) {
                                        const ScratchEnt en = scr[min(l0 + 4 + u, SCR_CAP - 1)];
                                        en_e[u] = en.e;
                                        Rn[u] = loadR(en.ro);
                                    }
                                    const double s01 = v[0] + v[1], q01 = v[0] * v[1];
                                    const double s23 = v[2] + v[3], q23 = v[2] * v[3];
                                    const double e1 = s01 + s23;
                                    const double e2 = fma(s01, s23, q01 + q23);
                                    const double e3 = fma(q01, s23, q23 * s01);
                                    const double e4 = q01 * q23;
#pragma unroll
                                    for (int j = 0; j < J; ++j) {
                                        double t = fma(F[j], e4, e3);
                                        t = fma(F[j], t, e2);
                                        t = fma(F[j], t, e1);
                                        acc[j] *= fma(F[j], t, 1.0);
                                        if ((j & (BMX_QSB - 1)) == BMX_QSB - 1) __builtin_amdgcn_sched_barrier(0);   // at most BMX_QSB chains in flight
                                    }
                                }
                            }
                            // (R from global memory: the rows of the NEXT block are requested before this block's arithmetic, as in
                            // the quad loop -- an L2 round trip per block would otherwise be exposed)
                            double Rp[BS], ep[BS];
                            if (BMX_PAIR_PREFETCH && npair > 0) {
#pragma unroll
                                for (int u = 0; u < BS; ++u) {
                                    const ScratchEnt en = scr[u];
                                    ep[u] = en.e;
                                    Rp[u] = loadR(en.ro);
                                }
                            }
                            for (int l0 = 0; l0 < npair; l0 += BS) {
                                CNT(3, 1);
                                spend(span8 * BS / 8);
                                double v[BS];
                                if (BMX_PAIR_PREFETCH) {
#pragma unroll
                                    for (int u = 0; u < BS; ++u) v[u] = ep[u] * Rp[u];
#pragma unroll
                                    for (int u = 0; u < BS; ++u) {
                                        const ScratchEnt en = scr[min(l0 + BS + u, SCR_CAP - 1)];
                                        ep[u] = en.e;
                                        Rp[u] = loadR(en.ro);
                                    }
                                } else {
#pragma unroll
                                for (int u = 0; u < BS; ++u) {      // lanes >= cnt carry Ev = 0: factor 1
                                    const ScratchEnt en = scr[l0 + u];     // uniform address: LDS broadcast
                                    v[u] = en.e * loadR(en.ro);
                                }
                                }
#pragma unroll
                                for (int u = 0; u < BS; u += 2) {
                                    const double sv = v[u] + v[u + 1], qv = v[u] * v[u + 1];
#pragma unroll
                                    for (int j = 0; j < J; ++j) acc[j] *= fma(F[j], fma(F[j], qv, sv), 1.0);
                                }
                            }
                            __builtin_amdgcn_wave_barrier();
                            fill = 0;
                            pend_np = 0;
                        }
                        PROF_MARK(3);
                        if (ended) break;
                        if (cnt_blk > 0) {
                            if (fill == 0) {
                                // lane 0 is the site of the pass nearest to the test sites: the largest alpha of everything pending
                                const double e0 = readlane_f64(Ev, 0);
                                const double om = 1.0 - e0, op = fma(e0, P.rmax, 1.0);
                                pend_lo = 1024 - ((__double2hiint(om) >> 20) & 0x7ff);
                                pend_hi = ((__double2hiint(op) >> 20) & 0x7ff) - 1022;
                                pad_ro = __builtin_amdgcn_readlane(rraw, 0) * rowmul;
                            }
                            const unsigned long long mn = __ballot(nearl);
                            if (nearl) scr[fill + rank(mn)] = ScratchEnt{Ev, rraw * rowmul, 0};
                            if (QUAD) pend_np += __popcll(__ballot(nearl && Ev > 0.5));
                            fill += cnt_blk;
                        }
                    }
                    base += dir * cnt;
                    if (cnt < WAVE) {
                        if (MODE != 1) break;
                        ended = true;                                  // one more turn: works off what is pending
                    }
                    i = inx;
                }
                PROF_MARK(2);
                // Ragged far end.  Beyond the zone common to all J windows, window j still holds n_j more sites.
                // When those are far-field sites (alpha |R| <= 3e-4: the log1p series to third order is exact
                // to 2e-15), the n_j grow along the order in which the windows end and all fit one pass, their
                // power sums are simply carried on from test site to test site in the flush below:
                // no generic passes at this end of the windows.
                int nrag_v = 0;                                    // lane: n_j of test site jl = lane % J
                int nrmax = 0;
                bool rag = false;
                if (FARSUM && kmom) {
                    const int ir = base + dir * lane;
                    const bool inr = ir >= 0 && ir < N;
                    const int ic = min(max(ir, 0), N - 1);
                    const double g = P.genpos[ic];
                    const int rr = (int)P.row[ic];
                    // alpha = E F needs the sites strictly beyond ALL test sites of the group (not so when the group has
                    // no common zone; a site AT a test position is not in that test site's window, v1:456), and the
                    // count below needs every window to be open already at `base`
                    bool okr = __ballot(inr && (dir > 0 ? g <= tnear : g >= tnear)) == 0ull &&
                               __ballot(dir > 0 ? lo_j > base : hi_j < base) == 0ull;
                    if (okr) {
                        // n_j = min(sites up to the window's index bound, sites with A*|g - t_j| <= zcut): the second
                        // count is a bisection over the pass's positions (the predicate falls monotonically along
                        // the walk: positions are sorted, FP subtraction and multiplication are monotone), done by
                        // every lane for its own test site -- the same predicate, bit for bit, as the scan's
                        scr_d[lane] = g;
                        __builtin_amdgcn_wave_barrier();
                        const int cnt1 = min(max(dir > 0 ? hi_j - base + 1 : base - lo_j + 1, 0), WAVE);
                        int lo_n = 0, hi_n = WAVE;                 // predicate true below lo_n, false from hi_n on
#pragma unroll
                        for (int it = 0; it < 7; ++it) {
                            const int mid = min((lo_n + hi_n) >> 1, WAVE - 1);
                            const bool pm = A * fabs(scr_d[mid] - tj) <= P.zcut;
                            const bool act = lo_n < hi_n;
                            lo_n = act && pm ? mid + 1 : lo_n;
                            hi_n = act && !pm ? mid : hi_n;
                        }
                        nrag_v = min(cnt1, lo_n);
                        __builtin_amdgcn_wave_barrier();
                        // the windows must end in walk order (t ascending to the right, descending to the left)
                        const int nb = dir > 0 ? __shfl_up(nrag_v, 1) : __shfl_down(nrag_v, 1);
                        const bool edge = dir > 0 ? jl == 0 : jl == J - 1;
                        okr = __ballot(!edge && nb > nrag_v) == 0ull;
                        nrmax = __builtin_amdgcn_readlane(nrag_v, dir > 0 ? J - 1 : 0);
                    }
                    if (okr && nrmax > 0 && nrmax < WAVE) {
                        const double Er = exp_neg(A * fabs(g - tnear));
                        const bool far3 = lane >= nrmax || Er * rowmax[rr] <= 3e-4;     // NaN (absent row): false
                        if (__ballot(far3) == ~0ull) {
                            rag = true;
                            scr[lane] = ScratchEnt{Er, rr * rowmul, 0};
                            __builtin_amdgcn_wave_barrier();
                        }
                    }
                }
                PROF_MARK(4);
                CNT(15, 1);
                if (FARSUM && (nfar_tot || rag)) {
                    CNT(8, 1);
                    CNT(11, rag ? 1 : 0);
                    // fold the moments: p_k = sum_rows M_k[row] R[row]^k, then acc_j *= exp(sum_k (-1)^(k+1) F_j^k p_k / k).
                    // |F v| <= far_eps = 0.05: 8th-order series with economised coefficients (see the flush), error < 9e-16 per
                    // site.  |sum| <= nfar_tot * far_eps * 1.03 < 422.
                    __builtin_amdgcn_wave_barrier();
                    double p[FAR_ORDER];
#pragma unroll
                    for (int k = 0; k < FAR_ORDER; ++k) p[k] = 0.0;
                    if (nfar_tot) {
                    auto fold = [&](const double (&m)[FAR_ORDER], const double R) {
                        const double R2 = R * R, R3 = R2 * R, R4 = R2 * R2;
                        p[0] = fma(m[0], R, p[0]);
                        p[1] = fma(m[1], R2, p[1]);
                        p[2] = fma(m[2], R3, p[2]);
                        p[3] = fma(m[3], R4, p[3]);
                        if constexpr (FAR_ORDER >= 6) {
                            p[4] = fma(m[4], R4 * R, p[4]);
                            p[5] = fma(m[5], R4 * R2, p[5]);
                        }
                        if constexpr (FAR_ORDER >= 8) {
                            p[6] = fma(m[6], R4 * R3, p[6]);
                            p[7] = fma(m[7], R4 * R4, p[7]);
                        }
                    };
                    {   // slot 0: its MOM_COPIES copies are read lane-parallel (copy = lane / order, moment = lane % order)
                        // and added up across lanes
                        static_assert(MOM_COPIES * FAR_ORDER <= WAVE, "slot-0 copies must fit one wave-wide read");
                        double x = 0.0;
                        if (lane < MOM_COPIES * FAR_ORDER) {
                            x = mom[lane];
                            mom[lane] = 0.0;                              // ready for the next zone
                        }
                        if (BMX_PRIV01) {
                            // lane = copy * 8 + order: the private sums are first added up over each group of eight lanes, then
                            // join the copies' first (order 0) and second (order 1) entries; the loop below sums over the copies
                            double y1 = m1p, y2 = m2p;
#pragma unroll
                            for (int off = 1; off < FAR_ORDER; off <<= 1) {
                                y1 += __shfl_xor(y1, off);
                                y2 += __shfl_xor(y2, off);
                            }
                            const int k8 = lane & (FAR_ORDER - 1);
                            x += k8 == 0 ? y1 : k8 == 1 ? y2 : 0.0;
                        }
#pragma unroll
                        for (int c = MOM_COPIES / 2; c >= 1; c >>= 1) x += __shfl_down(x, c * FAR_ORDER);
                        double m[FAR_ORDER];
#pragma unroll
                        for (int k = 0; k < FAR_ORDER; ++k) m[k] = readlane_f64(x, k);
                        if (m[0] != 0.0) fold(m, loadR(P.row_of_slot[0] * rowmul));
                    }
                    // the other slots, four at a time: all LDS reads of a batch are in flight together
                    CNT(10, kmom);
                    constexpr int FB = BMX_FOLD_BATCH;                       // slots per batch: their LDS reads are in flight together
                    for (int s0 = 1; s0 < kmom; s0 += FB) {
                        double2 m2[FB][FAR_ORDER / 2];
                        double Rs[FB];
                        if (BMX_FOLD_RPRE) {      // the batch's rows are requested together with the moments
#pragma unroll
                            for (int u = 0; u < FB; ++u) Rs[u] = loadR(P.row_of_slot[min(s0 + u, MOM_SLOTS - 1)] * rowmul);
                        }
#pragma unroll
                        for (int u = 0; u < FB; ++u) {
                            double2 *mp = reinterpret_cast<double2 *>(mom + (s0 + u + MOM_COPIES - 1) * FAR_ORDER);
#pragma unroll
                            for (int q = 0; q < FAR_ORDER / 2; ++q) m2[u][q] = mp[q];    // uniform address: LDS broadcast
                        }
#pragma unroll
                        for (int u = 0; u < FB; ++u) {
                            if (m2[u][0].x == 0.0) continue;              // no far site of this row in the zone
                            CNT(9, 1);
                            double m[FAR_ORDER];
#pragma unroll
                            for (int q = 0; q < FAR_ORDER / 2; ++q) {
                                m[2 * q] = m2[u][q].x;
                                m[2 * q + 1] = m2[u][q].y;
                            }
                            fold(m, BMX_FOLD_RPRE ? Rs[u] : loadR(P.row_of_slot[min(s0 + u, MOM_SLOTS - 1)] * rowmul));
                        }
                    }
                    // ready for the next zone: one lane-parallel sweep over the slots that may have been used
                    for (int idx = MOM_COPIES * FAR_ORDER + lane; idx < (kmom + MOM_COPIES - 1) * FAR_ORDER; idx += WAVE) mom[idx] = 0.0;
                    __builtin_amdgcn_wave_barrier();
                    }
                    PROF_MARK(5);
                    spend(2 + (int)((float)(nfar_tot + nrmax) * P.far_bits));
                    // t = p1 - f (p2/2 - f (p3/3 - ...)),  log product = f t
                    // t = w1 p1 - f (w2 p2 - f (w3 p3 - ...)),  log product = f t   (w_k: FAR_W above)
#pragma unroll
                    for (int k = 0; k < FAR_ORDER; ++k) p[k] *= FAR_W[k];
                    int l = 0;
                    double rag_e = 0.0, rag_R = 0.0;
                    if (rag) {
                        const ScratchEnt en = scr[0];
                        rag_e = en.e;
                        rag_R = loadR(en.ro);
                    }
#pragma unroll
                    for (int w = 0; w < J; w += 2) {
                        // test sites in pairs: the two exps of a pair are interleaved chains (exp_neg2), and the pair's
                        // products are final before the next pair starts (no tails of 16 exps kept in registers)
                        double arg[2];
#pragma unroll
                        for (int u = 0; u < 2; ++u) {
                            const int j = dir > 0 ? w + u : J - 1 - (w + u);
                            if (rag) {
                                const int nj = __builtin_amdgcn_readlane(nrag_v, j);
                                for (; l < nj; ++l) {                         // the ragged sites that window j adds
                                    const double v = rag_e * rag_R, v2 = v * v;
                                    const ScratchEnt en = scr[min(l + 1, WAVE - 1)];      // the next site's entry and row: one step ahead
                                    rag_e = en.e;
                                    rag_R = loadR(en.ro);
                                    p[0] += v;
                                    p[1] = fma(v2, 0.5, p[1]);
                                    p[2] = fma(v2 * v, 0.3333333333333333, p[2]);
                                }
                            }
                            const double f = F[j];
                            double t = p[FAR_ORDER - 1];
#pragma unroll
                            for (int k = FAR_ORDER - 2; k >= 0; --k) t = fma(-f, t, p[k]);
                            arg[u] = -f * t;
                        }
                        const int j0 = dir > 0 ? w : J - 1 - w, j1 = dir > 0 ? w + 1 : J - 2 - w;
                        double e0, e1;
                        exp_neg2(arg[0], arg[1], e0, e1);
                        acc[j0] *= e0;
                        acc[j1] *= e1;
                        asm volatile("" : "+v"(acc[j0]), "+v"(acc[j1]));
                    }
                    PROF_MARK(6);
                    if (rag) {
                        __builtin_amdgcn_wave_barrier();
                        return ZONE_DONE;      // every window of the group has ended: nothing left on this side
                    }
                }
                return base;
            };

            // sites between / at the test sites (and any part of the windows not covered by bulk)
            PROF_MARK(8);
            if (MIDTRI && mid_tri && A * (tL - t0) <= P.zcut) {
                // every pair is inside the cut-off (|t_i - t_j| <= tL - t0; FP subtraction and multiplication are monotone)
                const double xk = A * (tj - t0);
                double Gk, Hk;
                exp_neg2(xk, -xk, Gk, Hk);
                const int ro_k = mid_ro[jl];
                // each test site meets the other J - 1 sites once; every factor lies in [1 - alpha, 1 + alpha Rmax], alpha < 1
                spend((J - 1) * span_generic);
                double Fs[J];
                // sites i reach the test sites j < i:  alpha_ij = H_j G_i
#pragma unroll
                for (int j = 0; j < J; ++j) Fs[j] = readlane_f64(Hk, j);
                if (lane < J) scr[lane] = ScratchEnt{Gk, ro_k, 0};
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int i = 0; i < J; i += 2) {
                    const ScratchEnt en0 = scr[i], en1 = scr[i + 1];
                    const double v1 = en1.e * loadR(en1.ro);
                    if (i > 0) {
                        const double v0 = en0.e * loadR(en0.ro);
                        const double sv = v0 + v1, qv = v0 * v1;
#pragma unroll
                        for (int j = 0; j < i; ++j) acc[j] *= fma(Fs[j], fma(Fs[j], qv, sv), 1.0);
                    }
                    acc[i] *= fma(Fs[i], v1, 1.0);                    // test site i: site i + 1 only
                }
                __builtin_amdgcn_wave_barrier();
                // sites i reach the test sites j > i:  alpha_ij = G_j H_i
#pragma unroll
                for (int j = 0; j < J; ++j) Fs[j] = readlane_f64(Gk, j);
                if (lane < J) scr[lane] = ScratchEnt{Hk, ro_k, 0};
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int i = 0; i < J; i += 2) {
                    const ScratchEnt en0 = scr[i], en1 = scr[i + 1];
                    const double v0 = en0.e * loadR(en0.ro);
                    if (i + 2 < J) {
                        const double v1 = en1.e * loadR(en1.ro);
                        const double sv = v0 + v1, qv = v0 * v1;
#pragma unroll
                        for (int j = i + 2; j < J; ++j) acc[j] *= fma(Fs[j], fma(Fs[j], qv, sv), 1.0);
                    }
                    acc[i + 1] *= fma(Fs[i + 1], v0, 1.0);            // test site i + 1: site i only
                }
                __builtin_amdgcn_wave_barrier();
            } else {
                for (int b = L_int; b < R_int; b += SP) generic_pass(b, +1, R_int, staged);
            }
            PROF_MARK(0);
            // right side
            int b = bulk_zone(R_int, +1, tL, t0);
            if (b != ZONE_DONE) { CNT(12, 1); while (!generic_pass(b, +1, N, false)) { b += SP; CNT(12, 1); } }
            PROF_MARK(7);
            // left side
            b = bulk_zone(L_int - 1, -1, t0, tL);
            if (b != ZONE_DONE) { CNT(12, 1); while (!generic_pass(b, -1, -1, false)) { b -= SP; CNT(12, 1); } }
            PROF_MARK(7);

            renorm_all();
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int ec = min(max(E[j], -131071), 131071) + 131072;
                const int eb = bestK[j] >> 13;
                const bool better = (ec > eb) || (ec == eb && acc[j] > bestM[j]);
                if (better && p < P.npairs) {            // strict '>' (v1:501); iA ascending
                    bestM[j] = acc[j];
                    bestK[j] = (ec << 13) | iA;
                }
            }
        }
#pragma unroll
        // slice winner per test site: (exponent, mantissa) compared exactly, ties to the smaller linear index; the one
        // logarithm per test site is taken by finalize_kernel (no log, and none of its constants, in this kernel)
        for (int j = 0; j < J; ++j) {
            const int biA = bestK[j] & 8191;
            int bE = bestK[j] >> 13;
            double bM = bestM[j];
            int bL = biA == 8191 ? 0x7fffffff : biA * P.npairs + p;
            for (int off = 32; off > 0; off >>= 1) {
                const int oE = __shfl_xor(bE, off);
                const double oM = __shfl_xor(bM, off);
                const int oL = __shfl_xor(bL, off);
                if (oE > bE || (oE == bE && (oM > bM || (oM == bM && oL < bL)))) { bE = oE; bM = oM; bL = oL; }
            }
            if (lane == 0 && j < nvalid) {
                const size_t o = (size_t)slice * P.M + (tb + j);   // [slice][M]
                P.part_T[o] = bM;
                P.part_lin[o] = bL;
                P.part_ns[o] = bE;
            }
        }
    }
#ifdef BMX_PROFILE
    if (lane == 0 && P.prof)
        for (int k = 0; k < 12; ++k) atomicAdd(P.prof + k, (unsigned long long)prof_[k]);
#endif
#ifdef BMX_COUNT
    if (lane == 0 && P.prof)
        for (int k = 0; k < 16; ++k) atomicAdd(P.prof + 16 + k, cnt_[k]);
#endif
}

// ----------------------------------------------------------------------------- K2, prepared (round 3)
// Everything the grouped kernel did per pass of 64 sites -- loading positions and rows, exp(-A d), the near / far
// classification, the ds_add_f64 moment sums, the ragged-end counts -- is the same for all eight 64-pair slices of a group of
// test sites, and the grouped kernel did it once per slice (a quarter of its cycles, round-2 profiles).  Here it is done ONCE
// per group, by a separate lanes-over-sites kernel with a small register footprint (prep_kernel), which writes what the
// pair-parallel kernel needs as one sequential stream per group ("blob") in HBM; clr_scan_prepared_kernel -- one wave per
// (group, slice) as before -- then only multiplies, folds and flushes, reading its blob through a ring in LDS.
//
//   blob(group)  = for iA in 0..nA-1: near(iA, right), near(iA, left), far(iA, right), far(iA, left);   16-byte units,
//                  padded to a multiple of 4
//   near(zone)   = header (prep_hdr(J, first) units: 12 / 28 at J = 16):
//                    {magic | rag, n_pair, n_quad, n_occ} {n_far, n_rag, end index | ZONE_DONE, n_ser | class counts << 8} {n_j bytes}
//                    {span8 of the pair list | triangle flag << 16, 12 bytes: span8q / 8 of quad entries 0.., 64.., 128.., ...}
//                    J / 2 units: F_j = exp_neg(A |t_near - t_j|), j = 0 .. J - 1
//                    right zone only (the first of an A): J / 2 units G_k, J / 2 units H_k of the triangle (0 where the flag is 0)
//                  -- everything the eight slice-waves of a group used to recompute per A although it is the same in all of
//                  them; the consumer takes it with wave-uniform scalar loads straight from the blob, not through the ring.
//                  (Quad entries from 64 * 12 on have no budget byte: the consumer works those out itself, as before.)
//                  near list: n_pair entries with alpha > 1/2 (padded to whole blocks), then n_quad entries (multiple of 4),
//                             each (E_i f64, row offset i32), in walk order; 8 neutral guard entries (what the block loops
//                             request one block ahead).  The header's n_pair and n_quad are the padded counts; their low
//                             bits (3 / 2 at blocks of 8 / 4) hold the number of neutral entries in the list's last block
//                  ragged end (rag only): n_rag entries (E, row offset, flag) + 1 guard   (round 4: here, not behind the far field)
//   far(zone)    = moments:   n_occ entries of PREP_MOM units: (M_1, row offset) (M_2, M_3) (M_4, M_5) ...
//                  series entries: n_ser (a multiple of 4, <= 64) entries (E, row offset, order class) of far sites whose row has no
//                                  moment slot, highest class first
//   (both near lists first: the consumer multiplies, then takes ONE exp per test site for the two far fields together)
// Sizes come from a counting pass of the same code (prep_kernel<J, false>: identical predicates, no exp, no stores) run when
// the test sites are set, then an exclusive scan; the fill pass (prep_kernel<J, true>) and the consumer run per launch range.
// The far test is slice-independent now: alpha * max_grid |R[row]| <= far_eps, evaluated in the exponent domain
// (A d >= log(max|R| / far_eps), rounded up), so both passes classify from A d alone.
// Far field of the prepared kernels: log1p(x) = sum_k (-1)^(k+1) w_k x^k to order P_ORDER on |x| <= P_EPS, coefficients economised
// on that interval (scripts/far_series.py: Taylor polynomial of degree 40 re-expanded in Chebyshev polynomials of x / eps, cut after
// T_K, constant term < 3e-17 dropped).  Order 12 on [-0.15, 0.15]: max error 4.5e-16 (the round-2 kernels: order 8 on [-0.05, 0.05],
// 8.9e-16) -- the far field starts 1.1 units of A d nearer to the test sites, and the near lists, half of the scan kernel's
// instructions, lose a third of their entries.
#ifndef BMX_P_ORDER
#define BMX_P_ORDER 12
#endif
constexpr int P_ORDER = BMX_P_ORDER;
constexpr int P_COPIES = 4;                   // copies of the most frequent row's moments (lane % 4); P_COPIES * P_ORDER <= 64
static_assert(P_ORDER == 8 || P_ORDER == 12 || P_ORDER == 16, "far-field order of the prepared kernels: 8, 12 or 16");
static_assert(P_COPIES * P_ORDER <= WAVE, "slot-0 copies must fit one wave-wide read");
constexpr double P_EPS = P_ORDER == 16 ? 0.25 : P_ORDER == 12 ? 0.15 : 0.05;
constexpr int P_FAR_CAP = P_ORDER == 16 ? 2048 : P_ORDER == 12 ? 3584 : 8192;     // far sites per zone: P_FAR_CAP * P_EPS * 1.6 bits < 1000
#if BMX_P_ORDER == 16
__device__ constexpr double P_W[16] = {0.9999999999999954, 0.4999999999999791, 0.3333333333368442, 0.250000000008901, 0.19999999921757028,
                                       0.1666666652123534, 0.14285722101681053, 0.1250001188192722, 0.11110698172974029, 0.09999456222768308,
                                       0.09103227543438049, 0.08347880124963403, 0.07484961178075682, 0.06918273076087589, 0.08475562956871537,
                                       0.08074032343426385};
// a lane adds E^k (k >= 3) only while its term can exceed 2e-15: d = A d - threshold < P_D[k - 3]  (x = P_EPS exp(-d))
__device__ constexpr double P_D[14] = {9.539, 6.739, 5.071, 3.966, 3.181, 2.594, 2.14, 1.778, 1.483, 1.237, 1.03, 0.853, 0.7, 0.566};
#elif BMX_P_ORDER == 12
__device__ constexpr double P_W[12] = {0.9999999999999661, 0.49999999999988076, 0.3333333333754503, 0.25000000008463336, 0.19999998506452038,
                                       0.1666666441614055, 0.14285940976674, 0.1250028457483109, 0.11094429253027539, 0.09981580095968261,
                                       0.09676290425438011, 0.08920395582674094};
__device__ constexpr double P_D[10] = {9.029, 6.228, 4.56, 3.455, 2.67, 2.084, 1.629, 1.267, 0.972, 0.726};
#else
__device__ constexpr double P_W[8] = {0.9999999999998467, 0.4999999999996164, 0.3333333341509627, 0.25000000122701976,
                                      0.19999882322703955, 0.16666529319200146, 0.1434841013671569, 0.12562715480255862};
__device__ constexpr double P_D[6] = {7.94, 5.13, 3.462, 2.357, 1.571, 0.985};
#endif
constexpr double P_RAG_D = P_ORDER == 16 ? 6.74 : P_ORDER == 12 ? 6.23 : 5.13;     // log(P_EPS / 3e-4): the ragged end's third-order test
constexpr int PREP_GUARD = 8, PREP_MOM = 1 + P_ORDER / 2, PREP_RAG_GUARD = 1;     // a moment entry: (M_1, row) + M_2 .. M_K in pairs
// header of a zone: 4 units of integers, F_j in pairs, and with the first (right) zone of an A G_k and H_k of the triangle
constexpr int PREP_HDR_INT = 4, PREP_QB = 12;                     // PREP_QB: quad-list budgets in the header (one byte per started 64 entries)
__host__ __device__ constexpr int prep_hdr(int J, bool first) { return PREP_HDR_INT + J / 2 + (first ? J : 0); }
// Far sites of rows WITHOUT a moment slot (rare rows: fewer than ~1.3 sites per zone, so a slot's fold would cost more than it
// saves): not multiplied either -- they go into the stream as "series entries" (E, row, order class) and the scan kernel adds
// their (E R)^k to the same power sums p_k the moments feed, up to the order their alpha max|R| needs (2, 3, 5 or 8):
// 3 to 9 instructions per entry for all 16 test sites, against 24.5 in the product form.  A third of the old near lists were such sites.
constexpr double SER_DMIN = P_ORDER > 8 ? P_D[P_ORDER > 8 ? 6 : 0] : 0.0;      // order 9 and beyond below 2e-15
constexpr int SER_CAP = 64;                  // series entries per zone (buffered in prep_kernel's LDS until the zone's far part is written)
constexpr int PREP_MAGIC = 0x5a0e0000;
constexpr int RING_UNITS = 256, RING_MIRROR = 32, AUX_UNITS = 32;     // per wave: ring of 4 x 64 units + 32 mirrored + scratch
constexpr int PREP_ZONE_DONE = -0x7fffffff;
constexpr int PREP_THREADS = 256;
constexpr int PREP_THR_LDS_MAX = 4096;                                // rows whose far thresholds are staged in LDS
constexpr int64_t SOLO_GAP = 10;                                      // median gap between test sites beyond which groups stop paying (round 4, J = 8 at three waves per SIMD: 1.64 / 1.55 M, solo 1.575 / 1.574 M windows/s at stride 10 / 11)

struct PrepParams {
    const double *genpos;
    RowArray row;
    int64_t N;
    int rows, rowmul;             // consumer's row offset = row * rowmul (64: LDS slice, NP: global table)
    const double *A;
    int nA;
    const double *test_gen;       // the slot's test sites (absolute indexing: group g = test sites [g J, g J + J))
    const int64_t *win_lo, *win_hi, *center, *center_hi;
    int64_t M;
    double zcut;
    double rmax;                  // the consumer's P.rmax (list budgets)
    const double *rowthr;         // [rows]: A d from which a site of the row is far, the row's moment slot in the low byte
    int thr_in_lds;
    const uint8_t *kmom;
    const int *row_of_slot;       // [MOM_SLOTS]
    int mom_slots;
    int ser_cap;       // series entries per zone (SER_CAP; diagnostic builds: BMX_SER_CAP, 0 = none)
    int64_t g_begin, g_end;       // groups of this launch
    int32_t *blob_units;          // counting pass: [groups of the slot]
    const int64_t *blob_prefix;   // fill pass: exclusive prefix of blob_units
    int64_t prefix_base;          // ... of the launch range's first group: the arena holds the range's blobs from unit 0
    ScratchEnt *arena;
    int *status;                  // bit 0: a blob came out longer/shorter than counted, bit 1: bad header seen by the consumer
};

template <int J, bool FILL>
__global__ __launch_bounds__(PREP_THREADS) void prep_kernel(PrepParams P) {
    extern __shared__ __attribute__((aligned(16))) double lds_p[];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nw = blockDim.x / WAVE;
    const int N = (int)P.N;
    const int thr_len = P.thr_in_lds ? ((P.rows + 1) & ~1) : 0;
    if (P.thr_in_lds) {
        for (int idx = threadIdx.x; idx < P.rows; idx += blockDim.x) lds_p[idx] = P.rowthr[idx];
        __syncthreads();
    }
    // per wave: the moments of the right and of the left zone of one A (the stream holds both zones' near lists before either
    // zone's moments, so the right zone's sums wait while the left zone is walked), then 64 doubles of scratch.  P.mom_slots
    // is the largest number of slots any A uses (not the 64 / 254 the table would allow): LDS per wave decides how many waves
    // of this latency-bound kernel a CU holds.  The counting pass keeps one occupancy flag per slot (MS = 1).
    constexpr int MS = FILL ? P_ORDER : 1;
    const int mom_len = (P.mom_slots + P_COPIES - 1 + 3) * MS;
    double *mom_r = lds_p + thr_len + wave * (2 * mom_len + WAVE);
    double *mom_l = mom_r + mom_len;
    double *ragscr = mom_l + mom_len;
    // ... and (fill pass) the series entries of the two zones, kept until the zones' far parts are written
    ScratchEnt *ser_r = reinterpret_cast<ScratchEnt *>(lds_p + thr_len + nw * (2 * mom_len + WAVE)) + wave * (2 * SER_CAP);
    ScratchEnt *ser_l = ser_r + SER_CAP;
    for (int idx = lane; idx < 2 * mom_len; idx += WAVE) mom_r[idx] = 0.0;
    __builtin_amdgcn_wave_barrier();
    const int64_t grp = P.g_begin + (int64_t)blockIdx.x * nw + wave;
    if (grp >= P.g_end) return;                     // (no workgroup barrier below this line)
    auto thr_of = [&](int r) -> double {
        double v;
        if (P.thr_in_lds) v = lds_p[r]; else v = P.rowthr[r];
        return v;
    };
    auto rank = [&](unsigned long long m) {
        return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    };
    constexpr int BS = J >= 16 ? 4 : 8;             // sites per pair block of the consumer

    // group prologue: the consumer's, value for value
    const int64_t tb = grp * J;
    const int nvalid = (int)min((int64_t)J, P.M - tb);
    const int jl = lane % J;
    const int jj = min(jl, nvalid - 1);
    const double tj = P.test_gen[tb + jj];
    int lo_j = (int)max(P.win_lo[tb + jj], (int64_t)0);
    int hi_j = (int)min(P.win_hi[tb + jj], (int64_t)N - 1);
    if (jl >= nvalid) { lo_j = 1; hi_j = 0; }
    const double t0 = readlane_f64(tj, 0), tL = readlane_f64(tj, J - 1);
    const int c0 = (int)P.center[tb], cU = (int)P.center_hi[tb + nvalid - 1];
    int lo_max = 0, hi_min = N - 1;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int a = __builtin_amdgcn_readlane(lo_j, j), b = __builtin_amdgcn_readlane(hi_j, j);
        if (j < nvalid) { lo_max = max(lo_max, a); hi_min = min(hi_min, b); }
    }
    int L_int = min(c0, hi_min + 1), R_int = max(cU, lo_max);
    if (hi_min < lo_max) { L_int = c0; R_int = c0; hi_min = -1; lo_max = N; }   // no bulk zone
    // the consumer's triangle form applies to the group (its `mid_tri`): the J sites between L_int and R_int ARE the test sites
    bool mid_tri = false;
    if (BMX_MIDTRI) {
        const bool same = R_int - L_int <= MID_CAP && R_int - L_int == J && nvalid == J && lo_max <= L_int && hi_min >= R_int - 1;
        if (same) {
            const double gm = P.genpos[min(L_int + jl, N - 1)];
            const double tprev = __shfl_up(tj, 1);
            mid_tri = __ballot(!(gm == tj && (jl == 0 || tj > tprev))) == 0ull;
        }
    }

    int wpos = 0;                                   // units of the blob written (counted) so far
    ScratchEnt *out = nullptr;
    if (FILL) out = P.arena + (P.blob_prefix[grp] - P.prefix_base);

    for (int iA = 0; iA < P.nA; ++iA) {
        const double A = P.A[iA];
        const int kmom = min((int)P.kmom[iA], P.mom_slots);
        // One zone, first half: header slot, near list (pairs, then quads), guard; the far sites' moments go to `mom`; the
        // ragged end is sized.  What the second half needs comes back through the reference arguments.
        auto zone_near = [&](int base, int dir, double tnear, double tfar, double *mom, ScratchEnt *ser, int &zbase_o, int &npp_o, int &nqp_o,
                             int &nfar_o, int &base_o, double &m1p_o, double &m2p_o, int &nragv_o, int &nrmax_o, int &rag_o, double &zr_o,
                             int &rr_o, int &nser_o) {
            const bool first = dir > 0;
            const int zbase = wpos, nbase = zbase + prep_hdr(J, first);
            int n_pair = 0, n_pair_pad = 0, n_quad = 0, nfar_tot = 0, pad_ro = 0, n_ser = 0;
            // what the slice-waves no longer work out: F_j (lane j), with the first zone G_k / H_k of the triangle and its flag,
            // the exponent budgets of the pair list (from its first, largest alpha) and of every 64 quad entries
            const bool tri = first && mid_tri && A * (tL - t0) <= P.zcut;
            double e0p = 0.0;
            int qb0 = 0, qb1 = 0, qb2 = 0;
            if (FILL) {
                double *hd = reinterpret_cast<double *>(out + zbase + PREP_HDR_INT);
                const double fv = exp_neg(A * fabs(tnear - tj));
                if (lane < J) hd[lane] = fv;
                if (first) {
                    double Gk = 0.0, Hk = 0.0;
                    if (tri) {
                        const double xk = A * (tj - t0);
                        exp_neg2(xk, -xk, Gk, Hk);
                    }
                    if (lane < J) { hd[J + lane] = Gk; hd[2 * J + lane] = Hk; }
                }
            }
            bool pair_open = true, seen = false;
            double m1p = 0.0, m2p = 0.0;
            auto close_pairs = [&]() {
                n_pair_pad = (n_pair + BS - 1) & ~(BS - 1);
                if (FILL && lane < n_pair_pad - n_pair) out[nbase + n_pair + lane] = ScratchEnt{0.0, pad_ro, 0};
                pair_open = false;
            };
            int i = base + dir * lane;
            double g_nx = P.genpos[min(max(i, 0), N - 1)];
            int r_nx = (int)P.row[min(max(i, 0), N - 1)];
            while (true) {
                const bool ok = dir > 0 ? (i <= hi_min) : (i >= lo_max);
                const double g = g_nx;
                const int rraw = r_nx;
                const int inx = i + dir * WAVE;
                g_nx = P.genpos[min(max(inx, 0), N - 1)];
                r_nx = (int)P.row[min(max(inx, 0), N - 1)];
                const bool bulk = ok && (A * fabs(g - tfar) <= P.zcut);
                const int cnt = __popcll(__ballot(bulk));
                if (cnt) {
                    const double zn = A * fabs(g - tnear);
                    const double th = thr_of(rraw);
                    const int slot = __double2loint(th) & 0xff;
                    const bool farx = bulk && zn >= th && nfar_tot + n_ser < P_FAR_CAP;      // alpha max|R| <= P_EPS (NaN threshold: never)
                    const bool moml = farx && slot < kmom;
                    // a far site whose row has no moment slot: a series entry, while the zone's buffer has room for the whole pass
                    // (one that still needs more than 8 orders costs as much there as in the product: it stays near)
                    const bool serx = farx && slot >= kmom && !(zn - th < SER_DMIN);
                    const unsigned long long ms_ = __ballot(serx);
                    const bool ser_ok = n_ser + __popcll(ms_) <= P.ser_cap;
                    const bool serl = ser_ok && serx;
                    const bool nearl = bulk && !moml && !serl;
                    const bool pairl = nearl && zn < LN2;
                    const unsigned long long mm = __ballot(moml), mp = __ballot(pairl), mq = __ballot(nearl && !pairl);
                    const int nfar = __popcll(mm);
                    if (!seen) { pad_ro = __builtin_amdgcn_readlane(rraw, 0) * P.rowmul; seen = true; }   // lane 0: a site of the zone
                    double Ev = 0.0;
                    if (FILL) Ev = bulk ? exp_neg(zn) : 0.0;
                    if (nfar) {
                        if (moml) {
                            double *mr = mom + (slot ? slot + P_COPIES - 1 : (lane & (P_COPIES - 1))) * MS;
                            if (FILL) {
                                // a lane adds only the powers whose term can exceed 2e-15: x = alpha max|R| = far_eps exp(-(z - th))
                                const double d = zn - th;
                                const double E2 = Ev * Ev;
                                if (slot == 0) { m1p += Ev; m2p += E2; }
                                else { atomicAdd(mr, Ev); atomicAdd(mr + 1, E2); }
                                double Ek = E2;
#pragma unroll
                                for (int k = 3; k <= P_ORDER; ++k) {
                                    if (!(d < P_D[k - 3])) break;
                                    Ek *= Ev;
                                    atomicAdd(mr + (k - 1), Ek);
                                }
                            } else {
                                mom[(slot ? slot + P_COPIES - 1 : 0) * MS] = 1.0;      // occupancy only
                            }
                        }
                        nfar_tot += nfar;
                    }
                    if (ser_ok && ms_ != 0ull) {
                        if (FILL && serl) {
                            // order class by how far past the threshold the site lies: x = P_EPS exp(-(z - th)); order k + 1 matters while d < P_D[k - 2]
                            const double d = zn - th;
                            const int cls = !(d < P_D[0]) ? 2 : !(d < P_D[1]) ? 3 : !(d < P_D[3]) ? 5 : 8;
                            ser[n_ser + rank(ms_)] = ScratchEnt{Ev, rraw * P.rowmul, cls};
                        }
                        n_ser += __popcll(ms_);
                    }
                    if (pair_open) {
                        if (FILL && pairl) out[nbase + n_pair + rank(mp)] = ScratchEnt{Ev, rraw * P.rowmul, 0};
                        if (FILL && n_pair == 0 && mp != 0ull) e0p = readlane_f64(Ev, __ffsll((long long)mp) - 1);      // entry 0 of the list
                        n_pair += __popcll(mp);
                        if (__ballot(bulk && !(zn < LN2)) != 0ull || cnt < WAVE) close_pairs();
                    }
                    if (!pair_open) {
                        if (FILL && nearl && !pairl) out[nbase + n_pair_pad + n_quad + rank(mq)] = ScratchEnt{Ev, rraw * P.rowmul, 0};
                        if (FILL) {
                            // quad entry 64 k (at most one per pass): every factor of the 64 entries from it lies in [1/2, 1 + E Rmax]
                            const unsigned long long mz = __ballot(nearl && !pairl && ((n_quad + rank(mq)) & 63) == 0);
                            if (mz != 0ull) {
                                const int lz = __ffsll((long long)mz) - 1;
                                const int k = (n_quad + __popcll(mq & ((1ull << lz) - 1ull))) >> 6;
                                const double op = fma(readlane_f64(Ev, lz), P.rmax, 1.0);
                                const int hi = ((__builtin_amdgcn_readfirstlane(__double2hiint(op)) >> 20) & 0x7ff) - 1022;
                                const int qb = min(max(hi, 2), 125) << (8 * (k & 3));
                                if (k < 4) qb0 |= qb; else if (k < 8) qb1 |= qb; else if (k < PREP_QB) qb2 |= qb;
                            }
                        }
                        n_quad += __popcll(mq);
                    }
                }
                base += dir * cnt;
                if (cnt < WAVE) break;
                i = inx;
            }
            if (pair_open) close_pairs();
            const int n_quad_pad = (n_quad + 3) & ~3;
            if (FILL) {
                if (lane < n_quad_pad - n_quad) out[nbase + n_pair_pad + n_quad + lane] = ScratchEnt{0.0, pad_ro, 0};
                if (lane < PREP_GUARD) out[nbase + n_pair_pad + n_quad_pad + lane] = ScratchEnt{0.0, pad_ro, 0};
                int span8 = 0;
                if (n_pair > 0) {
                    const double om = 1.0 - e0p, op = fma(e0p, P.rmax, 1.0);
                    const int pend_lo = 1024 - ((__builtin_amdgcn_readfirstlane(__double2hiint(om)) >> 20) & 0x7ff);
                    const int pend_hi = ((__builtin_amdgcn_readfirstlane(__double2hiint(op)) >> 20) & 0x7ff) - 1022;
                    span8 = 8 * min(max(pend_hi, pend_lo), 125);
                }
                if (lane == 0) reinterpret_cast<int4 *>(out + zbase)[3] = int4{span8 | (tri ? 1 << 16 : 0), qb0, qb1, qb2};
            }
            wpos = nbase + n_pair_pad + n_quad_pad + PREP_GUARD;

            // ragged far end (see the grouped kernel): per-window counts n_j by bisection with the scan's own predicate
            int nrag_v = 0, nrmax = 0;
            int rag = 0;                 // bit 0: the ragged end goes into the stream; bit 1: some of its sites need more than three orders
            double zr = 0.0;
            int rr = 0;
            {   // (also where no row has a moment slot: series entries and the ragged end do not need one)
                const int ir = base + dir * lane;
                const bool inr = ir >= 0 && ir < N;
                const int ic = min(max(ir, 0), N - 1);
                const double g = P.genpos[ic];
                rr = (int)P.row[ic];
                bool okr = __ballot(inr && (dir > 0 ? g <= tnear : g >= tnear)) == 0ull &&
                           __ballot(dir > 0 ? lo_j > base : hi_j < base) == 0ull;
                if (okr) {
                    ragscr[lane] = g;
                    __builtin_amdgcn_wave_barrier();
                    const int cnt1 = min(max(dir > 0 ? hi_j - base + 1 : base - lo_j + 1, 0), WAVE);
                    int lo_n = 0, hi_n = WAVE;
#pragma unroll
                    for (int it = 0; it < 7; ++it) {
                        const int mid = min((lo_n + hi_n) >> 1, WAVE - 1);
                        const bool pm = A * fabs(ragscr[mid] - tj) <= P.zcut;
                        const bool act = lo_n < hi_n;
                        lo_n = act && pm ? mid + 1 : lo_n;
                        hi_n = act && !pm ? mid : hi_n;
                    }
                    nrag_v = min(cnt1, lo_n);
                    __builtin_amdgcn_wave_barrier();
                    const int nb = dir > 0 ? __shfl_up(nrag_v, 1) : __shfl_down(nrag_v, 1);
                    const bool edge = dir > 0 ? jl == 0 : jl == J - 1;
                    okr = __ballot(!edge && nb > nrag_v) == 0ull;
                    nrmax = __builtin_amdgcn_readlane(nrag_v, dir > 0 ? J - 1 : 0);
                }
                if (okr && nrmax > 0 && nrmax < WAVE) {
                    zr = A * fabs(g - tnear);
                    // every site of it far enough for eight orders (alpha max|R| <= 0.03; NaN threshold, absent row: false); most of
                    // the time for three (<= 3e-4).  Anything nearer: the zone ends before it and the scan kernel walks it.
                    const bool far8 = lane >= nrmax || zr >= thr_of(rr) + SER_DMIN;
                    const bool far3 = lane >= nrmax || zr >= thr_of(rr) + P_RAG_D;
                    rag = __ballot(far8) == ~0ull ? (__ballot(far3) == ~0ull ? 1 : 3) : 0;
                }
            }
            // the ragged end's entries follow the near list (the consumer walks them there, before either far field)
            if (rag) {
                if (FILL) {
                    if (lane < nrmax) out[wpos + lane] = ScratchEnt{exp_neg(zr), rr * P.rowmul, zr >= thr_of(rr) + P_RAG_D ? 0 : 1};      // 1: orders 4..8 too
                    if (lane == nrmax) out[wpos + lane] = ScratchEnt{0.0, rr * P.rowmul, 0};
                }
                wpos += nrmax + PREP_RAG_GUARD;
            }
            // (the padded counts are multiples of BS and of 4: their low bits carry the number of neutral entries in the last block)
            npp_o = n_pair_pad | (n_pair_pad - n_pair); nqp_o = n_quad_pad | (n_quad_pad - n_quad);
            zbase_o = zbase; nfar_o = nfar_tot; base_o = base; m1p_o = m1p; m2p_o = m2p;
            nragv_o = nrag_v; nrmax_o = nrmax; rag_o = rag; zr_o = zr; rr_o = rr; nser_o = n_ser;
        };
        // ... second half: the moments of the occupied slots (slot order), the ragged end's entries, and the header
        auto zone_far = [&](double *mom, const ScratchEnt *ser, int n_ser, int zbase, int pair_w, int quad_w, int nfar_tot, int base,
                            double m1p, double m2p, int nrag_v, int nrmax, int rag, double zr, int rr) {
            int n_occ = 0;
            if (nfar_tot) {
                __builtin_amdgcn_wave_barrier();
                {   // slot 0: P_COPIES copies read lane-parallel (copy = lane / order, moment = lane % order) + the private sums
                    double x = 0.0;
                    if (lane < P_COPIES * MS) {
                        x = mom[lane];
                        mom[lane] = 0.0;
                    }
                    if (FILL) {
                        double y1 = m1p, y2 = m2p;
#pragma unroll
                        for (int off = 1; off < WAVE; off <<= 1) {
                            y1 += __shfl_xor(y1, off);
                            y2 += __shfl_xor(y2, off);
                        }
                        x += lane == 0 ? y1 : lane == 1 ? y2 : 0.0;       // copy 0, orders 1 and 2
                    }
#pragma unroll
                    for (int c = P_COPIES / 2; c >= 1; c >>= 1) x += __shfl_down(x, c * MS);
                    const double m0 = readlane_f64(x, 0);
                    if (m0 != 0.0) {
                        if (FILL) {
                            double m[P_ORDER];
#pragma unroll
                            for (int k = 0; k < P_ORDER; ++k) m[k] = readlane_f64(x, k);
                            if (lane == 0) {
                                ScratchEnt *o = out + wpos;
                                o[0] = ScratchEnt{m[0], P.row_of_slot[0] * P.rowmul, 0};
                                double2 *o2 = reinterpret_cast<double2 *>(o + 1);
#pragma unroll
                                for (int q = 0; q < P_ORDER / 2; ++q) o2[q] = double2{m[2 * q + 1], 2 * q + 2 < P_ORDER ? m[2 * q + 2] : 0.0};
                            }
                        }
                        n_occ = 1;
                    }
                }
                for (int s0 = 1; s0 < kmom; s0 += WAVE) {
                    const int s = s0 + lane;
                    double m[P_ORDER];
#pragma unroll
                    for (int k = 0; k < P_ORDER; ++k) m[k] = 0.0;
                    if (s < kmom) {
                        double *ms = mom + (s + P_COPIES - 1) * MS;
#pragma unroll
                        for (int k = 0; k < MS; ++k) { m[k] = ms[k]; ms[k] = 0.0; }
                    }
                    const bool occ = m[0] != 0.0;
                    const unsigned long long mo = __ballot(occ);
                    if (FILL && occ) {
                        ScratchEnt *o = out + wpos + PREP_MOM * (n_occ + rank(mo));
                        o[0] = ScratchEnt{m[0], P.row_of_slot[s] * P.rowmul, 0};
                        double2 *o2 = reinterpret_cast<double2 *>(o + 1);
#pragma unroll
                        for (int q = 0; q < P_ORDER / 2; ++q) o2[q] = double2{m[2 * q + 1], 2 * q + 2 < P_ORDER ? m[2 * q + 2] : 0.0};
                    }
                    n_occ += __popcll(mo);
                }
                __builtin_amdgcn_wave_barrier();
                wpos += PREP_MOM * n_occ;
            }
            // series entries, sorted by class (highest first) and padded to a multiple of four with neutral entries
            const int n_ser_pad = (n_ser + 3) & ~3;
            int ser_w = n_ser_pad;
            if (n_ser) {
                if (FILL) {
                    __builtin_amdgcn_wave_barrier();
                    const ScratchEnt en = lane < n_ser ? ser[lane] : ScratchEnt{0.0, P.row_of_slot[0] * P.rowmul, 2};
                    const int cls = lane < n_ser ? en.pad : 0;
                    const unsigned long long m8 = __ballot(cls == 8), m5 = __ballot(cls == 5), m3 = __ballot(cls == 3), m2 = __ballot(cls == 2);
                    const int c8 = __popcll(m8), c5 = c8 + __popcll(m5), c3 = c5 + __popcll(m3);
                    const int dst = cls == 8 ? rank(m8) : cls == 5 ? c8 + rank(m5) : cls == 3 ? c5 + rank(m3) : cls == 2 ? c3 + rank(m2) : lane;
                    if (lane < n_ser_pad) out[wpos + dst] = en;
                    ser_w |= c8 << 8 | c5 << 16 | c3 << 24;
                    __builtin_amdgcn_wave_barrier();
                }
                wpos += n_ser_pad;
            }
            if (FILL) {
                // n_j of the J test sites as bytes (n_j < 64)
                int w = nrag_v & 0xff;
                w |= (__shfl_down(nrag_v, 1) & 0xff) << 8;
                w |= (__shfl_down(nrag_v, 2) & 0xff) << 16;
                w |= (__shfl_down(nrag_v, 3) & 0xff) << 24;
                const int w0 = __builtin_amdgcn_readlane(w, 0), w1 = __builtin_amdgcn_readlane(w, 4 % J),
                          w2 = __builtin_amdgcn_readlane(w, 8 % J), w3 = __builtin_amdgcn_readlane(w, 12 % J);
                if (lane == 0) {
                    int4 *o = reinterpret_cast<int4 *>(out + zbase);
                    o[0] = int4{PREP_MAGIC | rag, pair_w, quad_w, n_occ};
                    o[1] = int4{nfar_tot + n_ser, rag ? nrmax : 0, rag ? PREP_ZONE_DONE : base, ser_w};      // n_far: every site of the far field
                    o[2] = int4{w0, w1, w2, w3};
                }
            }
        };
        // stream order: both zones' near lists, then both zones' far fields (the consumer multiplies first and takes ONE exp
        // per test site for the two far fields together)
        int zbR, nppR, nqpR, nfR, beR, nrvR, nrmR, rrR, nsR, zbL, nppL, nqpL, nfL, beL, nrvL, nrmL, rrL, nsL;
        int ragR, ragL;
        double m1R, m2R, zrR, m1L, m2L, zrL;
        zone_near(R_int, +1, tL, t0, mom_r, ser_r, zbR, nppR, nqpR, nfR, beR, m1R, m2R, nrvR, nrmR, ragR, zrR, rrR, nsR);
        zone_near(L_int - 1, -1, t0, tL, mom_l, ser_l, zbL, nppL, nqpL, nfL, beL, m1L, m2L, nrvL, nrmL, ragL, zrL, rrL, nsL);
        zone_far(mom_r, ser_r, nsR, zbR, nppR, nqpR, nfR, beR, m1R, m2R, nrvR, nrmR, ragR, zrR, rrR);
        zone_far(mom_l, ser_l, nsL, zbL, nppL, nqpL, nfL, beL, m1L, m2L, nrvL, nrmL, ragL, zrL, rrL);
    }
    const int units = (wpos + 3) & ~3;
    if (!FILL) {
        if (lane == 0) P.blob_units[grp] = units;
    } else {
        if (lane == 0 && (int64_t)units != P.blob_prefix[grp + 1] - P.blob_prefix[grp]) atomicOr(P.status, 1);
    }
}

// exclusive prefix sums of the blob sizes (one workgroup; the array has one entry per group of test sites)
__global__ __launch_bounds__(1024) void prefix_kernel(const int32_t *u, int64_t n, int64_t *pre) {
    __shared__ int64_t part[1024];
    const int t = threadIdx.x;
    const int64_t per = (n + 1023) / 1024;
    const int64_t b = min((int64_t)t * per, n), e = min(b + per, n);
    int64_t s = 0;
    for (int64_t i = b; i < e; ++i) s += u[i];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int64_t v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int64_t run = part[t] - s;
    for (int64_t i = b; i < e; ++i) { pre[i] = run; run += u[i]; }
    if (t == 1023) pre[n] = part[1023];
}

// The ragged end's walk from entry l up to (not including) nj, as ONE asm statement: entry l comes out of the registers that hold the
// zone's ragged entries lanes-over-entries (v_readlane), its R was requested ahead (three registers, rotated), and its first three
// Taylor terms go into the zone's power sums p0..p2.  The same instructions the compiler made of the C++ loop -- but as a statement
// without control flow it no longer puts sixteen copies of a loop into the unrolled loop over the test sites, which is what made the
// register allocator spill 49 registers around them (round 3).  An LDS read may still be in flight when the statement ends: the
// caller waits for it (rag_walk_settle) before anything else may touch R2.
__device__ __forceinline__ void rag_walk_lds(int &l, int nj, int nrmax, int e_lo, int e_hi, int ro, unsigned lds_lane_addr,
                                             double &R0, double &R1, double &R2, double &p0, double &p1, double &p2) {
    int tmp;
    unsigned addr;
    double v, v2;
    const double third = 0.3333333333333333;
    asm volatile(
        "s_cmp_ge_i32 %[l], %[nj]\n\t"
        "s_cbranch_scc1 2f\n"
        "1:\n\t"
        "v_readlane_b32 vcc_lo, %[elo], %[l]\n\t"
        "v_readlane_b32 vcc_hi, %[ehi], %[l]\n\t"
        "s_add_i32 %[tmp], %[l], 3\n\t"
        "s_min_i32 %[tmp], %[tmp], %[nrmax]\n\t"
        "v_readlane_b32 %[tmp], %[ro], %[tmp]\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        "v_mul_f64 %[v], %[R0], vcc\n\t"
        "v_mov_b64 %[R0], %[R1]\n\t"
        "v_mov_b64 %[R1], %[R2]\n\t"
        "v_lshl_add_u32 %[addr], %[tmp], 3, %[lane]\n\t"
        "ds_read_b64 %[R2], %[addr]\n\t"
        "v_mul_f64 %[v2], %[v], %[v]\n\t"
        "v_add_f64 %[p0], %[p0], %[v]\n\t"
        "v_fma_f64 %[p1], %[v2], 0.5, %[p1]\n\t"
        "v_mul_f64 %[v2], %[v2], %[v]\n\t"
        "v_fma_f64 %[p2], %[v2], %[third], %[p2]\n\t"
        "s_add_i32 %[l], %[l], 1\n\t"
        "s_cmp_lt_i32 %[l], %[nj]\n\t"
        "s_cbranch_scc1 1b\n"
        "2:\n\t"
        : [l] "+s"(l), [R0] "+v"(R0), [R1] "+v"(R1), [R2] "+v"(R2), [p0] "+v"(p0), [p1] "+v"(p1), [p2] "+v"(p2),
          [tmp] "=&s"(tmp), [v] "=&v"(v), [v2] "=&v"(v2), [addr] "=&v"(addr)
        : [nj] "s"(nj), [nrmax] "s"(nrmax), [elo] "v"(e_lo), [ehi] "v"(e_hi), [ro] "v"(ro), [lane] "v"(lds_lane_addr), [third] "s"(third)
        : "vcc", "scc", "memory");
}
__device__ __forceinline__ void rag_walk_settle(double &R0, double &R1, double &R2) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(R0), "+v"(R1), "+v"(R2) : : "memory");
}
// ... the same walk with the R table in global memory / L2 (tables too large for LDS): row offsets are indices into the table
// (row * NP), the load is global_load_dwordx2 with the slice's base in a scalar pair, and the wait is on vmcnt.  Here the three R
// registers are taken in turn, RA -> RB -> RC -> RA, with the turn `ph` carried from statement to statement: the R of entry l was
// requested three entries ago and the walk waits for exactly that one (vmcnt(2): loads return in order), no register is moved.
// Same box, 262k-window blocks: 11 / 41 sample sizes per file 3.459 -> 3.504 / 2.638 -> 2.710 M windows/s.  With the table in LDS
// the same form measured 0.4-0.8 % SLOWER than the rotation (three more scalar compares and branches per statement, for a latency
// that is short there), so rag_walk_lds keeps it.
__device__ __forceinline__ void rag_walk_global(int &l, int &ph, int nj, int nrmax, int e_lo, int e_hi, int ro, unsigned lane8, const char *Rb,
                                             double &RA, double &RB, double &RC, double &p0, double &p1, double &p2) {
    int tmp;
    unsigned addr;
    double v, v2;
    const double third = 0.3333333333333333;
    asm volatile(
        "s_cmp_ge_i32 %[l], %[nj]\n\t"
        "s_cbranch_scc1 9f\n\t"
        "s_cmp_eq_u32 %[ph], 1\n\t"
        "s_cbranch_scc1 2f\n\t"
        "s_cmp_eq_u32 %[ph], 2\n\t"
        "s_cbranch_scc1 3f\n"
        "1:\n\t"
        "v_readlane_b32 vcc_lo, %[elo], %[l]\n\t"
        "v_readlane_b32 vcc_hi, %[ehi], %[l]\n\t"
        "s_add_i32 %[tmp], %[l], 3\n\t"
        "s_min_i32 %[tmp], %[tmp], %[nrmax]\n\t"
        "v_readlane_b32 %[tmp], %[ro], %[tmp]\n\t"
        "s_waitcnt vmcnt(2)\n\t"
        "v_mul_f64 %[v], %[RA], vcc\n\t"
        "v_lshl_add_u32 %[addr], %[tmp], 3, %[lane]\n\t"
        "global_load_dwordx2 %[RA], %[addr], %[base]\n\t"
        "v_mul_f64 %[v2], %[v], %[v]\n\t"
        "v_add_f64 %[p0], %[p0], %[v]\n\t"
        "v_fma_f64 %[p1], %[v2], 0.5, %[p1]\n\t"
        "v_mul_f64 %[v2], %[v2], %[v]\n\t"
        "v_fma_f64 %[p2], %[v2], %[third], %[p2]\n\t"
        "s_add_i32 %[l], %[l], 1\n\t"
        "s_mov_b32 %[ph], 1\n\t"
        "s_cmp_ge_i32 %[l], %[nj]\n\t"
        "s_cbranch_scc1 9f\n"
        "2:\n\t"
        "v_readlane_b32 vcc_lo, %[elo], %[l]\n\t"
        "v_readlane_b32 vcc_hi, %[ehi], %[l]\n\t"
        "s_add_i32 %[tmp], %[l], 3\n\t"
        "s_min_i32 %[tmp], %[tmp], %[nrmax]\n\t"
        "v_readlane_b32 %[tmp], %[ro], %[tmp]\n\t"
        "s_waitcnt vmcnt(2)\n\t"
        "v_mul_f64 %[v], %[RB], vcc\n\t"
        "v_lshl_add_u32 %[addr], %[tmp], 3, %[lane]\n\t"
        "global_load_dwordx2 %[RB], %[addr], %[base]\n\t"
        "v_mul_f64 %[v2], %[v], %[v]\n\t"
        "v_add_f64 %[p0], %[p0], %[v]\n\t"
        "v_fma_f64 %[p1], %[v2], 0.5, %[p1]\n\t"
        "v_mul_f64 %[v2], %[v2], %[v]\n\t"
        "v_fma_f64 %[p2], %[v2], %[third], %[p2]\n\t"
        "s_add_i32 %[l], %[l], 1\n\t"
        "s_mov_b32 %[ph], 2\n\t"
        "s_cmp_ge_i32 %[l], %[nj]\n\t"
        "s_cbranch_scc1 9f\n"
        "3:\n\t"
        "v_readlane_b32 vcc_lo, %[elo], %[l]\n\t"
        "v_readlane_b32 vcc_hi, %[ehi], %[l]\n\t"
        "s_add_i32 %[tmp], %[l], 3\n\t"
        "s_min_i32 %[tmp], %[tmp], %[nrmax]\n\t"
        "v_readlane_b32 %[tmp], %[ro], %[tmp]\n\t"
        "s_waitcnt vmcnt(2)\n\t"
        "v_mul_f64 %[v], %[RC], vcc\n\t"
        "v_lshl_add_u32 %[addr], %[tmp], 3, %[lane]\n\t"
        "global_load_dwordx2 %[RC], %[addr], %[base]\n\t"
        "v_mul_f64 %[v2], %[v], %[v]\n\t"
        "v_add_f64 %[p0], %[p0], %[v]\n\t"
        "v_fma_f64 %[p1], %[v2], 0.5, %[p1]\n\t"
        "v_mul_f64 %[v2], %[v2], %[v]\n\t"
        "v_fma_f64 %[p2], %[v2], %[third], %[p2]\n\t"
        "s_add_i32 %[l], %[l], 1\n\t"
        "s_mov_b32 %[ph], 0\n\t"
        "s_cmp_lt_i32 %[l], %[nj]\n\t"
        "s_cbranch_scc1 1b\n"
        "9:\n\t"
        : [l] "+s"(l), [ph] "+s"(ph), [RA] "+v"(RA), [RB] "+v"(RB), [RC] "+v"(RC), [p0] "+v"(p0), [p1] "+v"(p1), [p2] "+v"(p2),
          [tmp] "=&s"(tmp), [v] "=&v"(v), [v2] "=&v"(v2), [addr] "=&v"(addr)
        : [nj] "s"(nj), [nrmax] "s"(nrmax), [elo] "v"(e_lo), [ehi] "v"(e_hi), [ro] "v"(ro), [lane] "v"(lane8), [base] "s"(Rb), [third] "s"(third)
        : "vcc", "scc", "memory");
}
__device__ __forceinline__ void rag_walk_settle_global(double &RA, double &RB, double &RC) {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(RA), "+v"(RB), "+v"(RC) : : "memory");
}

struct PrepView {
    const ScratchEnt *arena;
    const int64_t *blob_prefix;   // the slot's exclusive prefix, indexed by absolute group
    int64_t prefix_base;          // prefix of the launch range's first group
    int64_t grp_base;             // absolute index of the launch range's first group
    int *status;
    // profile likelihoods (PL kernels only; NULL: that profile is off), keys (mantissa, clamped exponent + 2^17) of the launch
    // range: per (slice, A, test site) the best over the slice's pairs, and per (test site, pair) the best over A
    double *pl_am; int32_t *pl_ae;    // [nslices][nA][M]
    double *pl_pm; int32_t *pl_pe;    // [M][NP]
};

// Profile likelihoods: the key (mantissa m, exponent e) of a product that beats "product 1" (T = 0), or (0, 0) -- below every
// such key.  Keys are compared exactly as the best-tracking compares them; one conversion of the maximum key (key_clr, shared
// with finalize_kernel) makes the maximum of every profile equal to the CLR bit for bit.
__device__ __forceinline__ bool key_gt(int e, double m, int be, double bm) { return e > be || (e == be && m > bm); }

// J keys per lane (one per test site of the group) reduced over the wave's 64 lanes: a transposed butterfly -- at each of the
// first log2(J) steps a lane swaps half of its keys with its partner and keeps the larger of each pair (J - 1 exchanges), then a
// plain butterfly over the remaining lane bits.  Afterwards E[0]/m[0] of lane l hold the maximum of test site
// j = (l >> (6 - log2 J)), the same in all 64 / J lanes that share j.  The steps are a template recursion so that every array
// index is a constant: a runtime index would move acc[] / E[] of the whole scan loop to scratch memory.
template <int J, int H>
__device__ __forceinline__ void pl_transpose_step(int (&E)[J], double (&m)[J], int lane) {
    if constexpr (H >= 1) {
        constexpr int off = WAVE * H / J;          // keys H.. go to the partner across this lane bit
        const bool up = (lane & off) != 0;
#pragma unroll
        for (int k = 0; k < H; ++k) {
            const int se = up ? E[k] : E[k + H], ke = up ? E[k + H] : E[k];
            const double sm = up ? m[k] : m[k + H], km = up ? m[k + H] : m[k];
            const int re = __shfl_xor(se, off);
            const double rm = __shfl_xor(sm, off);
            const bool take = key_gt(re, rm, ke, km);
            E[k] = take ? re : ke;
            m[k] = take ? rm : km;
        }
        pl_transpose_step<J, H / 2>(E, m, lane);
    }
}

template <int J>
__device__ __forceinline__ void pl_wave_max(int (&E)[J], double (&m)[J], int lane) {
    pl_transpose_step<J, J / 2>(E, m, lane);
#pragma unroll
    for (int off = WAVE / J / 2; off >= 1; off >>= 1) {
        const int re = __shfl_xor(E[0], off);
        const double rm = __shfl_xor(m[0], off);
        if (key_gt(re, rm, E[0], m[0])) { E[0] = re; m[0] = rm; }
    }
}

// (groups of 8 with the table in LDS: 168 registers, so that one workgroup of twelve waves -- one R slice, twelve rings -- gives
// three waves per SIMD; the 16-test-site form needs 243 and runs two)
// PL: also the profile likelihoods' keys (V.pl_*); PL = false is the plain scan
template <int J, bool USE_LDS, bool PL = false>
__global__ __launch_bounds__((J == 8 && USE_LDS) ? SCAN_THREADS_J8 : SCAN_THREADS_MAX) void clr_scan_prepared_kernel(ScanParams P, PrepView V) {
#ifdef BMX_PROFILE
    // sections: 0 sites between the test sites, 1 zone header, 2 pair list, 3 quad list, 4 generic walks past the zones, 5 fold of the
    // moments, 6 series entries, 7 ragged end + Horner, 8 exp + apply, 9 renormalise + best-tracking, 10 group set-up, 11 winners out
    long long prof_[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    long long tprev_ = clock64();
#endif
    extern __shared__ __attribute__((aligned(16))) double lds_R[];  // [rows][64] when USE_LDS, then per wave: ring + scratch, sites between the test sites
    // farg[j] as an LLVM vector: the ragged-end walk indexes it with a wave-uniform j, which the compiler turns into GPR indexing
    // (s_set_gpr_idx_on) -- a C array indexed dynamically would live in scratch memory
    typedef double FargVec __attribute__((ext_vector_type(J)));
    constexpr int SP = WAVE / J;
    constexpr int BS = J >= 16 ? 4 : 8;
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
#if BMX_XCD_MAP
    // The slices of one chunk of test sites read the SAME blobs: put them on one XCD (workgroups go to the XCDs round-robin,
    // b % 8), next to each other in its dispatch order, so that one of them brings a blob into the XCD's L2 and the others hit.
    // (The host pads the number of chunks to a multiple of 8; padding chunks have no groups.)
    const int xcd = blockIdx.x & 7;
    const int64_t q = blockIdx.x >> 3;
    const int slice = (int)(q % P.nslices);
    const int64_t chunk = (q / P.nslices) * 8 + xcd;
#else
    const int slice = blockIdx.x % P.nslices;
    const int64_t chunk = blockIdx.x / P.nslices;
#endif
    const int p = slice * WAVE + lane;
    const int jl = lane % J, sl = lane / J;
    const int N = (int)P.N;
    const int nwv = blockDim.x / WAVE;

    if (USE_LDS) {
        const int total = P.rows * WAVE;
        for (int idx = threadIdx.x; idx < total; idx += blockDim.x)
            lds_R[idx] = P.Rt[(size_t)(idx >> 6) * P.NP + slice * WAVE + (idx & 63)];
    }
    const char *Rb = reinterpret_cast<const char *>(P.Rt + slice * WAVE);
    const unsigned lane8 = (unsigned)lane * 8u;
    const int rowmul = USE_LDS ? WAVE : P.NP;
    auto loadR = [&](int rowoff) -> double {
        return USE_LDS ? lds_R[rowoff + lane] : *reinterpret_cast<const double *>(Rb + ((unsigned)rowoff * 8u + lane8));
    };
    // LDS byte address of this lane's column of the R slice (for the hand-written ragged-end walk)
    const unsigned lds_lane_addr = (unsigned)(uintptr_t)(__attribute__((address_space(3))) double *)(lds_R + lane);
    double *lds_tail = lds_R + (USE_LDS ? P.rows * WAVE : 0);
    constexpr int WAVE_UNITS = RING_UNITS + RING_MIRROR + AUX_UNITS;
    ScratchEnt *ring = reinterpret_cast<ScratchEnt *>(lds_tail) + wave * WAVE_UNITS;
    ScratchEnt *scr = ring + RING_UNITS + RING_MIRROR;              // 32 units of wave-private scratch
    double *scr_d = reinterpret_cast<double *>(scr);
    double *mid_base = lds_tail + nwv * WAVE_UNITS * 2;
    // the ring and the scratch start out as valid neutral entries (row offset 0): whatever is read ahead of the stream is a
    // legal row reference
    for (int idx = lane; idx < WAVE_UNITS; idx += WAVE) ring[idx] = ScratchEnt{0.0, 0, 0};
    if (USE_LDS) __syncthreads(); else __builtin_amdgcn_wave_barrier();

    const int64_t ngroups = (P.M + J - 1) / J;
    const int64_t gpb = P.sites_per_block / J;
    const int64_t g_end = min((chunk + 1) * gpb, ngroups);
    for (int64_t grp = chunk * gpb + wave; grp < g_end; grp += nwv) {
        const int64_t tb = grp * J;
        const int nvalid = (int)min((int64_t)J, P.M - tb);
        int jl_g = jl, lane_g = lane, wave_g = wave;
        asm volatile("" : "+v"(jl_g), "+v"(lane_g), "+s"(wave_g));
        double *mid_g = mid_base + wave_g * (MID_CAP + MID_CAP / 2);
        int *mid_ro = reinterpret_cast<int *>(mid_g + MID_CAP);
        const int jj = min(jl_g, nvalid - 1);
        const double tj = P.test_gen[tb + jj];
        int lo_j = (int)max(P.win_lo[tb + jj], (int64_t)0);
        int hi_j = (int)min(P.win_hi[tb + jj], (int64_t)N - 1);
        if (jl >= nvalid) { lo_j = 1; hi_j = 0; }
        const int c0 = (int)P.center[tb], cU = (int)P.center_hi[tb + nvalid - 1];
        int lo_max = 0, hi_min = N - 1;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int a = __builtin_amdgcn_readlane(lo_j, j), b = __builtin_amdgcn_readlane(hi_j, j);
            if (j < nvalid) { lo_max = max(lo_max, a); hi_min = min(hi_min, b); }
        }
        int L_int = min(c0, hi_min + 1), R_int = max(cU, lo_max);
        if (hi_min < lo_max) { L_int = c0; R_int = c0; hi_min = -1; lo_max = N; }   // no bulk zone
        const bool staged = R_int - L_int <= MID_CAP;
        if (staged && lane_g < R_int - L_int) {
            mid_g[lane_g] = P.genpos[L_int + lane_g];
            mid_ro[lane_g] = (int)P.row[L_int + lane_g] * rowmul;
        }
        __builtin_amdgcn_wave_barrier();
        // (whether the triangle form applies -- the J staged sites ARE the test sites, and A (t_L - t_0) <= zcut -- is the producer's
        // word in the first header of every A; here only what keeps a corrupt word from reading unstaged sites)
        const bool tri_staged = staged && R_int - L_int == J;

        // the group's blob, streamed through the ring: `pos` units consumed, [.., staged_u) in the ring, the next 64 in flight
        // (the unit in flight is held as two doubles -- bit patterns, never arithmetic -- so that it stays in registers)
        const double2 *src = reinterpret_cast<const double2 *>(V.arena + (V.blob_prefix[V.grp_base + grp] - V.prefix_base));
        double2 *ring2 = reinterpret_cast<double2 *>(ring);
        // the zone headers' scalars (integers, F_j, G_k / H_k) do not go through the ring: they are the same for the whole wave, so
        // they come by scalar loads straight from the blob -- constant address space: the arena is written by the preceding kernel only
        typedef const __attribute__((address_space(4))) int *HdrPtr;
        typedef const __attribute__((address_space(4))) double *HdrPtr2;
        const HdrPtr ksrc = (HdrPtr)src;
        auto load_hdr = [&](int at, int4 &h0, int4 &h1, int4 &h3) {
            const HdrPtr hp = ksrc + 4 * at;
            h0 = int4{hp[0], hp[1], hp[2], hp[3]}; h1 = int4{hp[4], hp[5], hp[6], hp[7]}; h3 = int4{hp[12], hp[13], hp[14], hp[15]};
        };
        auto hdr_ok = [&](const int4 h0, const int4 h1, const int4 h3) -> bool {
            const int magic = h0.x, n_pair = h0.y & ~(BS - 1), n_quad = h0.z & ~3, n_occ = h0.w, nrmax = h1.y, ser_w = h1.w;
            const int n_ser = ser_w & 0xff, c8 = (ser_w >> 8) & 0xff, c5 = (ser_w >> 16) & 0xff, c3 = (ser_w >> 24) & 0xff;
            // (low bits of the list lengths: neutral entries in the last block -- fewer than a block, none in an empty list)
            return !((magic & ~3) != PREP_MAGIC || (magic & 3) == 2 || h0.y < 0 || h0.z < 0 || n_pair > N + 8 || n_quad > N + 8 || n_occ < 0 ||
                     (n_pair == 0 && h0.y != 0) || (n_quad == 0 && h0.z != 0) ||
                     n_occ > MOM_SLOTS || nrmax < 0 || nrmax >= WAVE || n_ser > SER_CAP || (n_ser & 3) || c8 > c5 || c5 > c3 || c3 > n_ser ||
                     (h3.x & 0xffff) > 1000 || (h3.x >> 17) != 0);
        };
        auto load_f = [&](int at, double (&F)[J]) {       // J doubles from unit `at` on
            const HdrPtr2 fp = (HdrPtr2)(ksrc + 4 * at);
#pragma unroll
            for (int j = 0; j < J; ++j) F[j] = fp[j];
        };
        int pos = 0, staged_u = 0;
        double nx_a, nx_b;
        {
            const double2 t = src[lane];
            nx_a = t.x; nx_b = t.y;
        }
        bool bad = false;
        auto stage = [&]() {
            const int slot = (staged_u >> 6) & 3;
            ring2[slot * WAVE + lane] = double2{nx_a, nx_b};
            if (slot == 0 && lane < RING_MIRROR) ring2[RING_UNITS + lane] = double2{nx_a, nx_b};   // units 0..15 again behind the ring's
            staged_u += WAVE;                                                       // end: any 16 consecutive units read without a wrap
            const double2 t = src[staged_u + lane];
            nx_a = t.x; nx_b = t.y;
            __builtin_amdgcn_wave_barrier();
        };
        // [pos, pos + 80) is in the ring.  `pos` moves by at most 64 units between two calls (a block, an entry, a guard, a
        // ragged end of < 64 sites), so one step restores the invariant
        auto need = [&]() {
            if (pos + 80 > staged_u) stage();
        };
        stage();
        stage();
        PROF_MARK(10);

        double acc[J], bestM[J];
        int E[J], bestK[J];
#pragma unroll
        for (int j = 0; j < J; ++j) {        // the product 1 (T = 0: only a larger one wins, v1:451,501) in the convention of the renormalisation
            bestM[j] = BMX_FREXP ? 0.5 : 1.0;
            bestK[j] = ((131072 + (BMX_FREXP ? 1 : 0)) << 13) | 8191;
        }

        for (int iA = 0; iA < P.nA; ++iA) {
            const double A = P.A[iA];
            int bits = 0;
#pragma unroll
            for (int j = 0; j < J; ++j) { acc[j] = 1.0; E[j] = 0; }
            auto renorm_all = [&]() {
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    if (BMX_FREXP) renorm_fx(acc[j], E[j]); else renorm(acc[j], E[j]);
                }
                bits = 0;
            };
            auto spend = [&](int nbits) {
                if (bits + nbits > 1000) renorm_all();
                bits += nbits;
            };
            const int span_generic = max(P.span_hi, 54);

            auto apply_pass = [&](double alpha, int rowoff, unsigned long long m_in, double *buf) {
                buf[lane] = alpha;
                __builtin_amdgcn_wave_barrier();
                double Rpre[SP];
                if (!USE_LDS) {
#pragma unroll
                    for (int s = 0; s < SP; ++s) Rpre[s] = loadR(__builtin_amdgcn_readlane(rowoff, s * J));
                }
#pragma unroll
                for (int s = 0; s < SP; ++s) {
                    if (((m_in >> (s * J)) & ((1ull << J) - 1ull)) == 0ull) continue;
                    const double R = USE_LDS ? loadR(__builtin_amdgcn_readlane(rowoff, s * J)) : Rpre[s];
                    const double2 *a2 = reinterpret_cast<const double2 *>(buf + s * J);
#pragma unroll
                    for (int j = 0; j < J; j += 2) {
                        const double2 a = a2[j >> 1];
                        acc[j] *= fma(a.x, R, 1.0);
                        acc[j + 1] *= fma(a.y, R, 1.0);
                    }
                }
                __builtin_amdgcn_wave_barrier();
            };
            auto generic_core = [&](int i, bool inr, double g, int rowoff, int dir) -> bool {
                const bool inwin = inr && i >= lo_j && i <= hi_j;
                const double z = A * fabs(g - tj);
                const bool in = inwin && (z <= P.zcut) && (g != tj);
                const bool fin = lo_j > hi_j ||
                                 (dir > 0 ? (!inr || i > hi_j || (i >= lo_j && g > tj && z > P.zcut))
                                          : (!inr || i < lo_j || (i <= hi_j && g < tj && z > P.zcut)));
                const unsigned long long m_in = __ballot(in);
                if (m_in != 0ull) {
                    const double alpha = in ? exp_neg(z) : 0.0;
                    spend(SP * (__ballot(in && z < 0.6931471805599453) == 0ull ? max(P.span_hi, 2) : span_generic));
                    apply_pass(alpha, rowoff, m_in, scr_d);
                }
                return __ballot(fin) == ~0ull;
            };
            auto generic_pass = [&](int b, int dir, int lim, bool from_lds) -> bool {
                const int i = b + dir * sl;
                const bool inr = dir > 0 ? (i < lim) : (i > lim);
                double g = 0.0;
                int rowoff = 0;
                if (from_lds) {
                    if (inr) { g = mid_g[i - L_int]; rowoff = mid_ro[i - L_int]; }
                } else {
                    if (inr) { g = P.genpos[i]; rowoff = (int)P.row[i] * rowmul; }
                }
                return generic_core(i, inr, g, rowoff, dir);
            };

            // One zone of the blob, first half: header and near-list products; returns where the generic walk goes on.  What
            // the far half needs later (after BOTH near lists) comes back through the references; fv: lane j holds F_j.
            // The header's integers (h0, h1, h3: units 0, 1 and 3) come from the caller, in scalar registers; F_j comes from the
            // units behind them -- computed once per group by prep_kernel, not once per slice here.
            auto zone_near = [&](auto dirk, const int4 h0, const int4 h1, const int4 h3, int &zpos_o, int &nocc_o, int &nfar_o, int &nrmax_o,
                                 int &rag_o, int &nser_o, FargVec &farg) -> int {
                constexpr int dirc = decltype(dirk)::value;       // compile-time: farg[j] and F[j] of the ragged-end walk are registers
                int nragv_o = 0;
                nocc_o = 0; nfar_o = 0; nrmax_o = 0; rag_o = 0; nser_o = 0;
                zpos_o = pos;
                if (bad) return PREP_ZONE_DONE;
                double F[J];
                load_f(pos + PREP_HDR_INT, F);
                need();
                const int magic = h0.x;
                const int n_pair = h0.y & ~(BS - 1), n_quad = h0.z & ~3, n_occ = h0.w;
                // neutral entries in each list's last block (E = 0: a factor of exactly 1)
                const int pair_pad = BMX_LIST_TAILS ? h0.y & (BS - 1) : 0, quad_pad = BMX_LIST_TAILS ? h0.z & 3 : 0;
                const int nfar_tot = h1.x, nrmax = h1.y, base_end = h1.z, ser_w = h1.w;
                const int rag = magic & 3;
                const int span8 = h3.x & 0xffff;                  // exponent budget of a pair entry, from the list's largest alpha
                if (!hdr_ok(h0, h1, h3)) {
                    bad = true;
                    return PREP_ZONE_DONE;
                }
                // n_j of this lane's test site (ragged end)
                nragv_o = (int)reinterpret_cast<const unsigned char *>(ring + ((pos + 2) & (RING_UNITS - 1)))[jl];
                nocc_o = n_occ; nfar_o = nfar_tot; nrmax_o = nrmax; rag_o = rag; nser_o = ser_w;
                pos += prep_hdr(J, dirc > 0);
                PROF_MARK(1);

                if (n_pair > 0) {
                    need();
                    double Rp[BS], ep[BS];
                    if (BMX_PPAIR_PREFETCH) {
                        const ScratchEnt *rp = ring + (pos & (RING_UNITS - 1));
#pragma unroll
                        for (int u = 0; u < BS; ++u) {
                            const ScratchEnt en = rp[u];
                            ep[u] = en.e;
                            Rp[u] = loadR(en.ro);
                        }
                    }
                    // one block; tail: the list's last block with nreal <= BS - 2 real entries.  A pair step of two neutral entries
                    // has v = +-0, so sv and qv are zeros and every factor is fma(F, +-0, 1.0) = 1.0 exactly: acc * 1.0 is skipped
                    // (a step with one real entry stays).  The tail is code of its own behind the loop, so that the loop over the
                    // whole blocks stays one basic block (a branch inside it: +1.5 % on the whole step); it asks for nothing ahead --
                    // what follows the list is the quad list's own first request, or the guard.
                    auto pair_block = [&](auto tailc, int nreal) {
                        constexpr bool tail = decltype(tailc)::value;
                        need();
                        const ScratchEnt *rp = ring + (pos & (RING_UNITS - 1));
                        spend(span8 * BS / 8);
                        double v[BS];
                        if (BMX_PPAIR_PREFETCH) {
#pragma unroll
                            for (int u = 0; u < BS; ++u) v[u] = ep[u] * Rp[u];
                            if (!tail) {
#pragma unroll
                                for (int u = 0; u < BS; ++u) {
                                    const ScratchEnt en = rp[BS + u];
                                    ep[u] = en.e;
                                    Rp[u] = loadR(en.ro);
                                }
                            }
                        } else {
#pragma unroll
                            for (int u = 0; u < BS; ++u) {
                                const ScratchEnt en = rp[u];
                                v[u] = en.e * loadR(en.ro);
                            }
                        }
#pragma unroll
                        for (int u = 0; u < BS; u += 2) {
                            if (tail && (u >= BS - 2 || (u > 0 && u >= nreal))) break;
                            const double sv = v[u] + v[u + 1], qv = v[u] * v[u + 1];
#pragma unroll
                            for (int j = 0; j < J; ++j) acc[j] *= fma(F[j], fma(F[j], qv, sv), 1.0);
                        }
                        pos += BS;
                    };
                    const int n_pair_main = pair_pad >= 2 ? n_pair - BS : n_pair;
                    for (int l0 = 0; l0 < n_pair_main; l0 += BS) pair_block(std::false_type{}, BS);
                    if (pair_pad >= 2) pair_block(std::true_type{}, BS - pair_pad);
                }
                PROF_MARK(2);
                if (n_quad > 0) {
                    need();
                    int span8q = 0;
                    double Rn[4], en_e[4];
                    {
                        const ScratchEnt *rp = ring + (pos & (RING_UNITS - 1));
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const ScratchEnt en = rp[u];
                            en_e[u] = en.e;
                            Rn[u] = loadR(en.ro);
                        }
                    }
                    // one block; tail: the list's last block with nreal = 1 or 2 real entries -- the neutral ones have v = +-0.  With
                    // v2 = v3 = +-0: s23 and q23 are zeros, so e1 = s01 + 0 = s01, e2 = fma(s01, 0, q01 + 0) = q01, e3 = fma(q01, 0, 0 s01)
                    // and e4 = q01 0 are zeros, and the chain is t = 0, t = fma(F, 0, q01) = q01, t = fma(F, q01, s01): the pair step.
                    // With v1 = +-0 as well: s01 = v0, q01 a zero, and the chain ends in t = fma(F, 0, v0) = v0.  (x + 0 = x and
                    // fma(a, 0, c) = c hold exactly for x, c != 0 whatever the zero's sign; where x or c is itself a zero only the sign
                    // of a zero can differ, and every such zero ends in fma(F, +-0, 1.0) = 1.0.)  Three real entries keep the
                    // four-site form.  Code of its own behind the loop, like the pair list's; its budget is the block's as before.
                    auto quad_block = [&](auto tailc, int l0, int nreal) {
                        constexpr bool tail = decltype(tailc)::value;
                        need();
                        const ScratchEnt *rp = ring + (pos & (RING_UNITS - 1));
                        if ((l0 & 63) == 0) {
                            // every factor of the next 64 entries lies in [1/2, 1 + e0 Rmax], e0 the first (largest) alpha among them:
                            // the producer's byte for the first PREP_QB * 64 entries; a longer list (unbounded: no room in a
                            // header of fixed size) goes on with the computation itself
                            const int k = l0 >> 6;
                            if (k < PREP_QB) {
                                span8q = 8 * (((k < 4 ? h3.y : k < 8 ? h3.z : h3.w) >> (8 * (k & 3))) & 0xff);
                            } else {
                                const double op = fma(rp[0].e, P.rmax, 1.0);
                                const int hi = ((__builtin_amdgcn_readfirstlane(__double2hiint(op)) >> 20) & 0x7ff) - 1022;
                                span8q = 8 * min(max(hi, 2), 125);
                            }
                        }
                        spend(span8q / 2);
                        if constexpr (tail) {
                            const double v0 = en_e[0] * Rn[0];
                            if (nreal == 2) {
                                const double v1 = en_e[1] * Rn[1];
                                const double s01 = v0 + v1, q01 = v0 * v1;
#pragma unroll
                                for (int j = 0; j < J; ++j) acc[j] *= fma(F[j], fma(F[j], q01, s01), 1.0);
                            } else {
#pragma unroll
                                for (int j = 0; j < J; ++j) acc[j] *= fma(F[j], v0, 1.0);
                            }
                        } else {
                            double v[4];
#pragma unroll
                            for (int u = 0; u < 4; ++u) v[u] = en_e[u] * Rn[u];
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                const ScratchEnt en = rp[4 + u];
                                en_e[u] = en.e;
                                Rn[u] = loadR(en.ro);
                            }
                            const double s01 = v[0] + v[1], q01 = v[0] * v[1];
                            const double s23 = v[2] + v[3], q23 = v[2] * v[3];
                            const double e1 = s01 + s23;
                            const double e2 = fma(s01, s23, q01 + q23);
                            const double e3 = fma(q01, s23, q23 * s01);
                            const double e4 = q01 * q23;
#pragma unroll
                            for (int j = 0; j < J; ++j) {
                                double t = fma(F[j], e4, e3);
                                t = fma(F[j], t, e2);
                                t = fma(F[j], t, e1);
                                acc[j] *= fma(F[j], t, 1.0);
                                if ((j & (BMX_QSB - 1)) == BMX_QSB - 1) __builtin_amdgcn_sched_barrier(0);
                            }
                        }
                        pos += 4;
                    };
                    const int n_quad_main = quad_pad >= 2 ? n_quad - 4 : n_quad;
                    for (int l0 = 0; l0 < n_quad_main; l0 += 4) quad_block(std::false_type{}, l0, 4);
                    if (quad_pad >= 2) quad_block(std::true_type{}, n_quad_main, 4 - quad_pad);
                }
                PROF_MARK(3);
                pos += PREP_GUARD;
                // The ragged end (< 64 entries and a guard) follows the near list in the stream: read at once, lanes over entries; the walk
                // takes an entry out of the registers and has its R loaded ahead.  Test site by test site, in the order in which the
                // windows end: its share of the entries into three sums of their own (third-order Taylor terms: these sites sit at
                // A d ~ 18.4), then the sums as they stand into farg[j].  Done HERE, where only the running products are live -- not
                // between the Horner chains of the far field, where round 3 had it and paid 49 spilled registers for it.
                if (rag) {
                    need();
                    const bool rag_hi = (rag & 2) != 0;
                    const ScratchEnt ragm = ring[(pos + lane) & (RING_UNITS - 1)];
                    double rag_R0 = loadR(__builtin_amdgcn_readlane(ragm.ro, 0));
                    double rag_R1 = loadR(__builtin_amdgcn_readlane(ragm.ro, min(1, nrmax)));
                    double rag_R2 = loadR(__builtin_amdgcn_readlane(ragm.ro, min(2, nrmax)));
                    const int nrag_v = nragv_o;
                    double r1 = 0.0, r2 = 0.0, r3 = 0.0;
                    int l = 0, ph = 0;            // the walk's position and whose turn it is among rag_R0 / rag_R1 / rag_R2
                    if (USE_LDS) {
                        // the walk itself is one asm statement per test site (rag_walk_lds): no control flow inside the unrolled loop
#pragma unroll
                        for (int w = 0; w < J; ++w) {
                            const int j = dirc > 0 ? w : J - 1 - w;
                            rag_walk_lds(l, __builtin_amdgcn_readlane(nrag_v, j), nrmax, __double2loint(ragm.e), __double2hiint(ragm.e), ragm.ro,
                                         lds_lane_addr, rag_R0, rag_R1, rag_R2, r1, r2, r3);
                            const double f = F[j];
                            farg[j] = fma(-f, fma(-f, fma(-f, r3, r2), r1), farg[j]);
                        }
                        rag_walk_settle(rag_R0, rag_R1, rag_R2);
                    } else {
#pragma unroll
                        for (int w = 0; w < J; ++w) {
                            const int j = dirc > 0 ? w : J - 1 - w;
                            rag_walk_global(l, ph, __builtin_amdgcn_readlane(nrag_v, j), nrmax, __double2loint(ragm.e), __double2hiint(ragm.e), ragm.ro,
                                            lane8, Rb, rag_R0, rag_R1, rag_R2, r1, r2, r3);
                            const double f = F[j];
                            farg[j] = fma(-f, fma(-f, fma(-f, r3, r2), r1), farg[j]);
                        }
                        rag_walk_settle_global(rag_R0, rag_R1, rag_R2);
                    }
                    // (rare) sites of the ragged end with alpha max|R| between 3e-4 and 0.03, flagged by the producer: orders 4 to 8 of each, for
                    // the test sites whose windows hold it -- apart from the walk above
                    if (rag_hi) {
                        for (int lh = 0; lh < nrmax; ++lh) {
                            if (__builtin_amdgcn_readlane(ragm.pad, lh) == 0) continue;
                            const double v = readlane_f64(ragm.e, lh) * loadR(__builtin_amdgcn_readlane(ragm.ro, lh));
#pragma unroll
                            for (int j = 0; j < J; ++j) {
                                const double u = (lh < __builtin_amdgcn_readlane(nrag_v, j)) ? F[j] * v : 0.0;
                                const double u2 = u * u;
                                double t = fma(-u, P_W[7], P_W[6]);
                                t = fma(-u, t, P_W[5]);
                                t = fma(-u, t, P_W[4]);
                                t = fma(-u, t, P_W[3]);
                                farg[j] = fma(u2 * u2, t, farg[j]);
                            }
                        }
                    }
                    pos += nrmax + PREP_RAG_GUARD;
                }
                PROF_MARK(7);
                return base_end;
            };

            // ... second half, after both zones' near lists: fold the zone's moments, walk its ragged end, and ADD the log of
            // the factor each test site's product has to pick up to farg (the exp is taken once for both zones)
            auto zone_far = [&](int zpos, int n_occ, int ser_w, int nfar_tot, FargVec &farg) {
                const int n_ser = ser_w & 0xff, ser_cls = ser_w >> 8;        // entries; cumulative class counts (8, 5, 3), 8 bits each
                if (bad || !nfar_tot) return;
                // F_j again, by a second scalar load from the zone's header (requested here, used by the Horner chains below:
                // the folds in between hide it) -- not 32 scalar registers kept across both near lists
                double F[J];
                load_f(zpos + PREP_HDR_INT, F);
                double pk[P_ORDER];
#pragma unroll
                for (int k = 0; k < P_ORDER; ++k) pk[k] = 0.0;
                // p_k += M_k R^k for one moment entry (q: its units 1.. as (M_2, M_3), (M_4, M_5), ...); powers by halving: depth log2 k
                // (Measured and dropped: stopping an entry's powers and FMAs at its top non-zero order -- a slot of few, far sites ends in
                // M_k = +0.0, 60 % of the entries at config 4 -- written by prep_kernel into the entry's first unit.  Exact, and fewer
                // instructions, but the wave-uniform branches inside the fold cost more than the skipped arithmetic: +2.0 % on the
                // whole step with a cut per unit, +1.4 % with two cuts and every unit still read up front; profiles/fold_tails_ab.txt.)
                auto fold = [&](const double m1, const double2 *q, const double R) {
                    double pw[P_ORDER + 1];
                    pw[1] = R;
#pragma unroll
                    for (int k = 2; k <= P_ORDER; ++k) pw[k] = pw[k >> 1] * pw[k - (k >> 1)];
                    pk[0] = fma(m1, R, pk[0]);
#pragma unroll
                    for (int k = 2; k <= P_ORDER; ++k) {
                        const double2 v = q[(k - 2) >> 1];
                        pk[k - 1] = fma((k & 1) ? v.y : v.x, pw[k], pk[k - 1]);
                    }
                };
                // two slots per step.  With the table in L2 / HBM the heads (M_1, row) and the R of the NEXT two are requested before this
                // step's powers (+3.4 / +4.2 % at 11 / 41 sample sizes); with the table in LDS the extra live values cost more than the
                // short latency (-0.7 %), so that form asks for its R where it needs it
                if (BMX_FOLD_EARLY && n_occ > 0) {
                    need();
                    const ScratchEnt *rp0 = ring + (pos & (RING_UNITS - 1));
                    ScratchEnt ua = rp0[0], ub = rp0[n_occ > 1 ? PREP_MOM : 0];
                    double Ra = loadR(ua.ro), Rb2 = loadR(ub.ro);
                    for (int s = 0; s < n_occ; s += 2) {
                        need();
                        const ScratchEnt *rp = ring + (pos & (RING_UNITS - 1));
                        const bool two = s + 1 < n_occ;
                        const double m1a = ua.e, m1b = ub.e, Rca = Ra, Rcb = Rb2;
                        const int na = s + 2 < n_occ ? 2 * PREP_MOM : 0, nb = s + 3 < n_occ ? 3 * PREP_MOM : na;     // (the last step: itself again)
                        ua = rp[na];
                        ub = rp[nb];
                        Ra = loadR(ua.ro);
                        Rb2 = loadR(ub.ro);
                        fold(m1a, reinterpret_cast<const double2 *>(rp + 1), Rca);
                        if (two) fold(m1b, reinterpret_cast<const double2 *>(rp + PREP_MOM + 1), Rcb);
                        pos += two ? 2 * PREP_MOM : PREP_MOM;
                    }
                }
                if (!BMX_FOLD_EARLY) {
                    for (int s = 0; s < n_occ; s += 2) {
                        need();
                        const ScratchEnt *rp = ring + (pos & (RING_UNITS - 1));
                        const bool two = s + 1 < n_occ;
                        const ScratchEnt ua = rp[0], ub = rp[two ? PREP_MOM : 0];
                        const double Ra = loadR(ua.ro), Rb2 = loadR(ub.ro);
                        fold(ua.e, reinterpret_cast<const double2 *>(rp + 1), Ra);
                        if (two) fold(ub.e, reinterpret_cast<const double2 *>(rp + PREP_MOM + 1), Rb2);
                        pos += two ? 2 * PREP_MOM : PREP_MOM;
                    }
                }
                PROF_MARK(5);
                // (round 4, measured and dropped: E by an LDS broadcast read one batch ahead instead of two v_readlane per entry: -0.7 %)
                // series entries: p_k += (E R)^k up to the order the entry's class needs.  The wave reads them all at once, lanes over
                // entries; one entry at a time then comes out of the registers (readlane) -- its R is the only load in the loop, four
                // entries ahead.  The producer sorted them by class, highest first: one branch-free loop per class (a lower-class
                // entry that rides along in the last batch of a higher class only gets more terms than it needs).
                if (n_ser > 0) {
                    need();
                    const ScratchEnt mine = ring[(pos + lane) & (RING_UNITS - 1)];
                    const int e8 = (ser_cls & 0x7f) + 3 & ~3, e5 = max(e8, ((ser_cls >> 8) & 0x7f) + 3 & ~3), e3 = max(e5, ((ser_cls >> 16) & 0x7f) + 3 & ~3);
                    double Rn[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) Rn[u] = loadR(__builtin_amdgcn_readlane(mine.ro, u));
                    auto batch = [&](auto kc, int s0) {
                        constexpr int K = decltype(kc)::value;
                        double Rc[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) Rc[u] = Rn[u];
                        const int nx = s0 + 4 < n_ser ? s0 + 4 : s0;
#pragma unroll
                        for (int u = 0; u < 4; ++u) Rn[u] = loadR(__builtin_amdgcn_readlane(mine.ro, nx + u));
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const double v = readlane_f64(mine.e, s0 + u) * Rc[u];
                            pk[0] += v;
                            if (K == 2) {
                                pk[1] = fma(v, v, pk[1]);
                            } else {
                                const double v2 = v * v;
                                pk[1] += v2;
                                pk[2] = fma(v2, v, pk[2]);
                                if (K > 3) {
                                    const double v4 = v2 * v2;
                                    pk[3] += v4;
                                    pk[4] = fma(v4, v, pk[4]);
                                    if (K > 5) {
                                        pk[5] = fma(v4, v2, pk[5]);
                                        pk[6] = fma(v4 * v2, v, pk[6]);
                                        pk[7] = fma(v4, v4, pk[7]);
                                    }
                                }
                            }
                        }
                    };
                    int s0 = 0;
                    for (; s0 < e8; s0 += 4) batch(std::integral_constant<int, 8>{}, s0);
                    for (; s0 < e5; s0 += 4) batch(std::integral_constant<int, 5>{}, s0);
                    for (; s0 < e3; s0 += 4) batch(std::integral_constant<int, 3>{}, s0);
                    for (; s0 < n_ser; s0 += 4) batch(std::integral_constant<int, 2>{}, s0);
                    pos += n_ser;
                }
                PROF_MARK(6);
#pragma unroll
                for (int k = 0; k < P_ORDER; ++k) pk[k] *= P_W[k];
                // the Horner chains of the zone's far field, one per test site, in one straight line
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    const double f = F[j];
                    double t = pk[P_ORDER - 1];
#pragma unroll
                    for (int k = P_ORDER - 2; k >= 0; --k) t = fma(-f, t, pk[k]);
                    farg[j] = fma(-f, t, farg[j]);              // exp_neg's argument: the factor is exp(f t)
                }
                PROF_MARK(7);
            };

            // sites between / at the test sites (and any part of the windows not covered by bulk)
            PROF_MARK(9);
            // the right zone's header (the left zone's is read where that zone starts: requesting either one earlier, across the
            // best-tracking or the right zone's near list, cost more scalar registers spilled than the wait it saved)
            int4 hR0, hR1, hR3, hL0, hL1, hL3;
            load_hdr(pos, hR0, hR1, hR3);
            const int posR = pos;
            const bool okR = !bad && hdr_ok(hR0, hR1, hR3);      // (zone_near sets `bad` from the same test; nothing of a bad header is used)
            // triangle: the producer's word says whether the form applies at this A, and brings G_k, H_k
            if (BMX_MIDTRI && tri_staged && okR && (hR3.x >> 16) == 1) {
                const double *gh = reinterpret_cast<const double *>(src + posR + PREP_HDR_INT + J / 2);
                const double Gk = gh[jl], Hk = gh[J + jl];
                const int ro_k = mid_ro[jl];
                spend((J - 1) * span_generic);
                double Fs[J];
                load_f(posR + PREP_HDR_INT + J, Fs);              // H_k
                if (lane < J) scr[lane] = ScratchEnt{Gk, ro_k, 0};
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int i = 0; i < J; i += 2) {
                    const ScratchEnt en0 = scr[i], en1 = scr[i + 1];
                    const double v1 = en1.e * loadR(en1.ro);
                    if (i > 0) {
                        const double v0 = en0.e * loadR(en0.ro);
                        const double sv = v0 + v1, qv = v0 * v1;
#pragma unroll
                        for (int j = 0; j < i; ++j) acc[j] *= fma(Fs[j], fma(Fs[j], qv, sv), 1.0);
                    }
                    acc[i] *= fma(Fs[i], v1, 1.0);
                }
                __builtin_amdgcn_wave_barrier();
                load_f(posR + PREP_HDR_INT + J / 2, Fs);          // G_k
                if (lane < J) scr[lane] = ScratchEnt{Hk, ro_k, 0};
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int i = 0; i < J; i += 2) {
                    const ScratchEnt en0 = scr[i], en1 = scr[i + 1];
                    const double v0 = en0.e * loadR(en0.ro);
                    if (i + 2 < J) {
                        const double v1 = en1.e * loadR(en1.ro);
                        const double sv = v0 + v1, qv = v0 * v1;
#pragma unroll
                        for (int j = i + 2; j < J; ++j) acc[j] *= fma(Fs[j], fma(Fs[j], qv, sv), 1.0);
                    }
                    acc[i + 1] *= fma(Fs[i + 1], v0, 1.0);
                }
                __builtin_amdgcn_wave_barrier();
            } else {
                for (int b = L_int; b < R_int; b += SP) generic_pass(b, +1, R_int, staged);
            }
            PROF_MARK(0);
            // right side, left side: near lists and whatever the zones do not cover
            int zposR, zposL;
            int noccR, nfarR, nrmR, nserR, noccL, nfarL, nrmL, nserL;
            int ragR, ragL;
            FargVec farg;               // per test site: minus the log of the factor its product picks up from the far fields (exp_neg's argument)
#pragma unroll
            for (int j = 0; j < J; ++j) farg[j] = 0.0;
            int b = zone_near(std::integral_constant<int, +1>{}, hR0, hR1, hR3, zposR, noccR, nfarR, nrmR, ragR, nserR, farg);
            if (b != PREP_ZONE_DONE) { while (!generic_pass(b, +1, N, false)) b += SP; }
            PROF_MARK(4);
            load_hdr(pos, hL0, hL1, hL3);
            b = zone_near(std::integral_constant<int, -1>{}, hL0, hL1, hL3, zposL, noccL, nfarL, nrmL, ragL, nserL, farg);
            if (b != PREP_ZONE_DONE) { while (!generic_pass(b, -1, -1, false)) b -= SP; }
            PROF_MARK(4);
            // the far fields of both zones: ONE exp per test site -- test sites in pairs, two interleaved exp chains, each pair
            // final before the next one starts
            if (!bad && (nfarR || ragR || nfarL || ragL)) {
                auto apply_far = [&]() {
#pragma unroll
                    for (int w = 0; w < J; w += 2) {
                        double e0, e1;
                        exp_neg2(farg[w], farg[w + 1], e0, e1);
                        acc[w] *= e0;
                        acc[w + 1] *= e1;
                        asm volatile("" : "+v"(acc[w]), "+v"(acc[w + 1]));
                        farg[w] = 0.0;
                        farg[w + 1] = 0.0;
                    }
                    PROF_MARK(8);
                };
                // exponent budget: a zone's far field moves a product by at most (sites) * far_bits bits (< 860 by P_FAR_CAP); both
                // zones in one exp only while their sum fits, else one after the other with the exponents pulled out in between
                const int bitsR = 2 + (int)((float)(nfarR + nrmR) * P.far_bits), bitsL = 2 + (int)((float)(nfarL + nrmL) * P.far_bits);
                // (one copy of each zone's code: this kernel's per-A path is about as large as the instruction cache)
                const bool split = bitsR + bitsL > 900;
                zone_far(zposR, noccR, nserR, nfarR, farg);
                if (split) {
                    spend(bitsR);
                    apply_far();
                }
                zone_far(zposL, noccL, nserL, nfarL, farg);
                spend(split ? bitsL : bitsR + bitsL);
                apply_far();
            }
            renorm_all();
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int ec = min(max(E[j], -131071), 131071) + 131072;
                const int eb = bestK[j] >> 13;
                const bool better = ((ec > eb) || (ec == eb && acc[j] > bestM[j])) && (!BMX_FREXP || acc[j] > 0.0);
                if (better && p < P.npairs) {
                    bestM[j] = acc[j];
                    bestK[j] = (ec << 13) | iA;
                }
            }
            if constexpr (PL) {
                if (V.pl_am) {
                    // A profile: this A's keys over the slice's pairs, in place (acc / E are dead until the next A sets them),
                    // counted exactly where the best-tracking above would count them
#pragma unroll
                    for (int j = 0; j < J; ++j) {
                        const int ec = min(max(E[j], -131071), 131071) + 131072;
                        const bool beats = key_gt(ec, acc[j], 131072 + (BMX_FREXP ? 1 : 0), BMX_FREXP ? 0.5 : 1.0) && (!BMX_FREXP || acc[j] > 0.0) &&
                                           p < P.npairs;
                        E[j] = beats ? ec : 0;
                        acc[j] = beats ? acc[j] : 0.0;
                    }
                    pl_wave_max<J>(E, acc, lane);
                    const int jm = lane >> (6 - __builtin_ctz(J));
                    if ((lane & (WAVE / J - 1)) == 0 && jm < nvalid) {
                        const size_t o = ((size_t)slice * P.nA + iA) * P.M + (tb + jm);
                        V.pl_am[o] = acc[0];
                        V.pl_ae[o] = E[0];
                    }
                }
            }
            if (bad) break;
        }
        PROF_MARK(9);
        if (bad && lane == 0) atomicOr(V.status, 2);
        if constexpr (PL) {
            if (V.pl_pm) {
                // x and alpha_beta profiles: each pair's best over A, before the winners' reduction below overwrites it
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    if (j < nvalid) {
                        const bool any = (bestK[j] & 8191) != 8191 && !bad;
                        const size_t o = (size_t)(tb + j) * P.NP + p;
                        V.pl_pm[o] = any ? bestM[j] : 0.0;
                        V.pl_pe[o] = any ? bestK[j] >> 13 : 0;
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int biA = bestK[j] & 8191;
            int bE = bestK[j] >> 13;
            double bM = bestM[j];
            int bL = (biA == 8191 || bad) ? 0x7fffffff : biA * P.npairs + p;
            for (int off = 32; off > 0; off >>= 1) {
                const int oE = __shfl_xor(bE, off);
                const double oM = __shfl_xor(bM, off);
                const int oL = __shfl_xor(bL, off);
                if (oE > bE || (oE == bE && (oM > bM || (oM == bM && oL < bL)))) { bE = oE; bM = oM; bL = oL; }
            }
            if (lane == 0 && j < nvalid) {
                const size_t o = (size_t)slice * P.M + (tb + j);
                P.part_T[o] = bM;
                P.part_lin[o] = bL;
                P.part_ns[o] = bE;
            }
        }
        PROF_MARK(11);
    }
#ifdef BMX_PROFILE
    if (lane == 0 && P.prof)
        for (int k = 0; k < 12; ++k) atomicAdd(P.prof + k, (unsigned long long)prof_[k]);
#endif
}

// ----------------------------------------------------------------------------- K2, prepared, one test site per wave
// Sparse test sets (the reference's -s with a large step), unsorted test positions: windows share too little for groups.
// The same split as above with J = 1: prep_solo_kernel walks each test site's window once per A -- both sides; with one
// test site the decay separates trivially (alpha_i = E_i, F = 1), so the two sides share the near lists and ONE set of
// moments -- and clr_scan_solo_kernel, one wave per (test site, slice), multiplies the near lists, folds the moments and takes
// one exp per A.  The round-2 per-site kernel did the walk (loads, exp, window test) in all eight slice waves and multiplied
// every site of the window.
//
// Round 3 read every entry back from the LDS ring with a broadcast ds_read_b128 next to the ds_read_b64 of its R: 9 LDS clocks per
// entry for each of 16 waves per CU -- the LDS pipe, not the vector unit, was the bound (8.7 cycles per VALU instruction).  Round 4:
// the sites of the most frequent row (substitutions: 70 % of the sites) need no R read at all -- that row's R sits in a register and
// their entries are the 8-byte E alone, two per broadcast read: 0.5 LDS instructions per entry instead of 2 -- and the slices of a
// chunk of test sites run on one XCD, so that a stream comes out of HBM once, not eight times.
// (Measured and dropped in round 4: the whole stream through the scalar cache -- s_load_dwordx16 from the constant address space,
// entries as scalar operands, no ring at all: 0.80 M windows/s against round 3's 1.35 M.  A wave gets one 64-byte line per ~2200
// cycles that way: the scalar cache is built for a few hot constants, not for 88 KB of stream per wave.)
//   blob(test site) = for iA:  one or more SEGMENTS, then the far field
//     segment   = header, 64 B: {magic | last, n0, n1, n_occ} {n_far, 0, 0, 0} ...
//                 n0 (a multiple of 8) entries of the most frequent row: E (8 B each)
//                 n1 (a multiple of 4) entries of the other rows: (E, row offset, 0) (16 B each); all 64-byte aligned;
//                 lists padded with neutral entries (E = 0); a segment is flushed from prep_solo_kernel's LDS staging lists
//                 whenever they fill, so any window size goes through fixed-size staging
//     far field = n_occ moment entries of 5 units: (c_1 .. c_8) (row offset), c_k = -+ w_k M_k, the series' coefficient already
//                 in (with F = 1 the far field of a row is one polynomial in R); padded to a multiple of 4 units
constexpr int SOLO_MAGIC = 0x50100000;
constexpr int SOLO_S0 = 256, SOLO_S1 = 192;        // staging lists per wave: E of the most frequent row / (E, row offset) of the others
// Far field of the solo kernels: order 8 on |x| <= 0.05 (the round-2 series).  The per-row thresholds on the device are
// those of the grouped kernels (P_EPS): a site is far here S_SHIFT = log(P_EPS / S_EPS) later.
#ifndef BMX_S_ORDER
#define BMX_S_ORDER 8
#endif
#if BMX_S_ORDER == 8
constexpr int S_ORDER = 8, S_COPIES = 8, S_MOM = 1 + S_ORDER / 2, S_FAR_CAP = 8192;
// (S_EPS = 0.05)
constexpr double S_SHIFT = P_ORDER == 16 ? 1.6095 : P_ORDER == 12 ? 1.0987 : 0.0;
__device__ constexpr double S_W[8] = {0.9999999999998467, 0.4999999999996164, 0.3333333341509627, 0.25000000122701976,
                                      0.19999882322703955, 0.16666529319200146, 0.1434841013671569, 0.12562715480255862};
__device__ constexpr double S_D[6] = {7.94, 5.13, 3.462, 2.357, 1.571, 0.985};
#else
// the prepared group kernels' series (order P_ORDER on |x| <= P_EPS): fewer near entries, longer Horner chains per occupied row
constexpr int S_ORDER = P_ORDER, S_COPIES = P_COPIES, S_MOM = 1 + S_ORDER / 2, S_FAR_CAP = P_FAR_CAP;
constexpr double S_SHIFT = 0.0;
#define S_W P_W
#define S_D P_D
#endif

template <bool FILL>
__global__ __launch_bounds__(PREP_THREADS) void prep_solo_kernel(PrepParams P) {
    extern __shared__ __attribute__((aligned(16))) double lds_p[];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nw = blockDim.x / WAVE;
    const int N = (int)P.N;
    const int thr_len = P.thr_in_lds ? ((P.rows + 1) & ~1) : 0;
    if (P.thr_in_lds) {
        for (int idx = threadIdx.x; idx < P.rows; idx += blockDim.x) lds_p[idx] = P.rowthr[idx];
        __syncthreads();
    }
    const int mom_len = (P.mom_slots + S_COPIES - 1 + 3) * S_ORDER;
    double *mom = lds_p + thr_len + wave * mom_len;
    // staging lists of the near entries (fill pass): the most frequent row's E, then the other rows' (E, row offset)
    double *st0 = lds_p + thr_len + nw * mom_len + wave * (SOLO_S0 + 2 * SOLO_S1);
    ScratchEnt *st1 = reinterpret_cast<ScratchEnt *>(st0 + SOLO_S0);
    for (int idx = lane; idx < mom_len; idx += WAVE) mom[idx] = 0.0;
    __builtin_amdgcn_wave_barrier();
    const int64_t t = P.g_begin + (int64_t)blockIdx.x * nw + wave;       // "group" = one test site
    if (t >= P.g_end) return;
    auto thr_of = [&](int r) -> double {
        double v;
        if (P.thr_in_lds) v = lds_p[r]; else v = P.rowthr[r];
        return v;
    };
    auto rank = [&](unsigned long long m) {
        return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    };
    const double tg = P.test_gen[t];
    const int lo = (int)max(P.win_lo[t], (int64_t)0);
    const int hi = (int)min(P.win_hi[t], (int64_t)N - 1);
    const int c = (int)P.center[t], ch = (int)P.center_hi[t];     // sites in [c, ch) sit AT the test position: never in its window (v1:455)
    const int row0 = P.row_of_slot[0];                            // the most frequent row of the data (its R stays in a register of the consumer)
    int wpos = 0;
    ScratchEnt *out = nullptr;
    if (FILL) out = P.arena + (P.blob_prefix[t] - P.prefix_base);

    for (int iA = 0; iA < P.nA; ++iA) {
        const double A = P.A[iA];
        const int kmom = min((int)P.kmom[iA], P.mom_slots);
        int n0 = 0, n1 = 0, nfar_tot = 0, pad_ro = 0;       // n0 / n1: entries staged for the next segment
        bool seen = false;
        double m1p = 0.0, m2p = 0.0;
        // one segment of the stream from the staging lists: header, the E of the most frequent row (padded to 8), the other rows'
        // entries (padded to 4)
        auto flush = [&](bool last, int n_occ) {
            const int n0p = (n0 + 7) & ~7, n1p = (n1 + 3) & ~3;
            if (FILL) {
                __builtin_amdgcn_wave_barrier();
                if (lane == 0) {
                    int4 *h = reinterpret_cast<int4 *>(out + wpos);
                    h[0] = int4{SOLO_MAGIC | (last ? 1 : 0), n0p, n1p, n_occ};
                    h[1] = int4{nfar_tot, 0, 0, 0};
                    h[2] = int4{0, 0, 0, 0};
                    h[3] = int4{0, 0, 0, 0};
                }
                double *o0 = reinterpret_cast<double *>(out + wpos + 4);
                for (int i = lane; i < n0p; i += WAVE) o0[i] = i < n0 ? st0[i] : 0.0;
                ScratchEnt *o1 = out + wpos + 4 + n0p / 2;
                for (int i = lane; i < n1p; i += WAVE) o1[i] = i < n1 ? st1[i] : ScratchEnt{0.0, pad_ro, 0};
                __builtin_amdgcn_wave_barrier();
            }
            wpos += 4 + n0p / 2 + n1p;
            n0 = 0;
            n1 = 0;
        };
        for (int dir = 0; dir < 2; ++dir) {
            // dir 0: indices max(ch, lo), +1, ... up to hi;  dir 1: min(c - 1, hi), -1, ... down to lo
            const int base = dir == 0 ? max(ch, lo) : min(c - 1, hi);
            int i = dir == 0 ? base + lane : base - lane;
            double g_nx = P.genpos[min(max(i, 0), N - 1)];
            int r_nx = (int)P.row[min(max(i, 0), N - 1)];
            while (true) {
                const bool valid = (i >= lo) && (i <= hi);
                const double g = g_nx;
                const int rraw = r_nx;
                const int inx = dir == 0 ? i + WAVE : i - WAVE;
                g_nx = P.genpos[min(max(inx, 0), N - 1)];
                r_nx = (int)P.row[min(max(inx, 0), N - 1)];
                const double zn = A * fabs(g - tg);
                const bool in = valid && (zn <= P.zcut) && (g != tg);
                const unsigned long long m_in = __ballot(in);
                if (m_in != 0ull) {
                    const double th0 = thr_of(rraw);
                    const int slot = __double2loint(th0) & 0xff;
                    const double th = th0 + S_SHIFT;                    // (NaN stays NaN: rows absent from the helper file are never far)
                    const bool moml = in && slot < kmom && zn >= th && nfar_tot < S_FAR_CAP;
                    const bool nearl = in && !moml;
                    const bool near0 = nearl && rraw == row0;
                    const unsigned long long mm = __ballot(moml), mn0 = __ballot(near0), mn1 = __ballot(nearl && !near0);
                    const int nfar = __popcll(mm);
                    if (!seen) { pad_ro = __builtin_amdgcn_readlane(rraw, __ffsll((long long)m_in) - 1) * P.rowmul; seen = true; }
                    double Ev = 0.0;
                    if (FILL) Ev = in ? exp_neg(zn) : 0.0;
                    if (nfar) {
                        if (moml) {
                            double *mr = mom + (slot ? slot + S_COPIES - 1 : (lane & (S_COPIES - 1))) * S_ORDER;
                            if (FILL) {
                                const double d = zn - th;
                                const double E2 = Ev * Ev;
                                if (slot == 0) { m1p += Ev; m2p += E2; }
                                else { atomicAdd(mr, Ev); atomicAdd(mr + 1, E2); }
                                double Ek = E2;
#pragma unroll
                                for (int k = 3; k <= S_ORDER; ++k) {
                                    if (!(d < S_D[k - 3])) break;
                                    Ek *= Ev;
                                    atomicAdd(mr + (k - 1), Ek);
                                }
                            } else {
                                mom[(slot ? slot + S_COPIES - 1 : 0) * S_ORDER] = 1.0;
                            }
                        }
                        nfar_tot += nfar;
                    }
                    // a pass adds at most 64 entries to either list: a segment goes out before one could overflow
                    if (n0 + WAVE > SOLO_S0 || n1 + WAVE > SOLO_S1) flush(false, 0);
                    if (FILL) {
                        if (near0) st0[n0 + rank(mn0)] = Ev;
                        if (nearl && !near0) st1[n1 + rank(mn1)] = ScratchEnt{Ev, rraw * P.rowmul, 0};
                    }
                    n0 += __popcll(mn0);
                    n1 += __popcll(mn1);
                }
                // the walk ends where the window does: its index bound, or the first site past the cut-off (positions are sorted)
                if (__ballot(valid && zn > P.zcut) != 0ull || __ballot(valid) != ~0ull) break;
                i = inx;
            }
        }
        // the moments of the occupied slots, premultiplied by the series' coefficients; they follow the last segment
        int n_occ = 0;
        bool occ0 = false;
        double x0 = 0.0;
        if (nfar_tot) {
            __builtin_amdgcn_wave_barrier();
            if (lane < S_COPIES * S_ORDER) {
                x0 = mom[lane];
                mom[lane] = 0.0;
            }
            if (FILL) {
                double y1 = m1p, y2 = m2p;
#pragma unroll
                for (int off = 1; off < WAVE; off <<= 1) {
                    y1 += __shfl_xor(y1, off);
                    y2 += __shfl_xor(y2, off);
                }
                x0 += lane == 0 ? y1 : lane == 1 ? y2 : 0.0;
            }
#pragma unroll
            for (int cc = S_COPIES / 2; cc >= 1; cc >>= 1) x0 += __shfl_down(x0, cc * S_ORDER);
            occ0 = readlane_f64(x0, 0) != 0.0;
            n_occ = occ0 ? 1 : 0;
            // count the other occupied slots first: the last segment's header carries n_occ
            for (int s0 = 1; s0 < kmom; s0 += WAVE) {
                const int sl = s0 + lane;
                const bool occ = sl < kmom && mom[(sl + S_COPIES - 1) * S_ORDER] != 0.0;
                n_occ += __popcll(__ballot(occ));
            }
        }
        flush(true, n_occ);
        if (nfar_tot) {
            int at = 0;
            if (occ0) {
                if (FILL) {
                    double m[S_ORDER];
#pragma unroll
                    for (int k = 0; k < S_ORDER; ++k) m[k] = readlane_f64(x0, k) * ((k & 1) ? -S_W[k] : S_W[k]);     // c_k = -+ w_k M_k
                    if (lane == 0) {
                        double2 *o2 = reinterpret_cast<double2 *>(out + wpos);
#pragma unroll
                        for (int q = 0; q < S_ORDER / 2; ++q) o2[q] = double2{m[2 * q], m[2 * q + 1]};
                        *reinterpret_cast<int4 *>(out + wpos + S_ORDER / 2) = int4{row0 * P.rowmul, 0, 0, 0};
                    }
                }
                at = 1;
            }
            for (int s0 = 1; s0 < kmom; s0 += WAVE) {
                const int sl = s0 + lane;
                double m[S_ORDER];
#pragma unroll
                for (int k = 0; k < S_ORDER; ++k) m[k] = 0.0;
                if (sl < kmom) {
                    double *ms = mom + (sl + S_COPIES - 1) * S_ORDER;
#pragma unroll
                    for (int k = 0; k < S_ORDER; ++k) { m[k] = ms[k]; ms[k] = 0.0; }
                }
                const bool occ = m[0] != 0.0;
                const unsigned long long mo = __ballot(occ);
                if (FILL && occ) {
#pragma unroll
                    for (int k = 0; k < S_ORDER; ++k) m[k] *= (k & 1) ? -S_W[k] : S_W[k];
                    ScratchEnt *o = out + wpos + S_MOM * (at + rank(mo));
                    double2 *o2 = reinterpret_cast<double2 *>(o);
#pragma unroll
                    for (int q = 0; q < S_ORDER / 2; ++q) o2[q] = double2{m[2 * q], m[2 * q + 1]};
                    *reinterpret_cast<int4 *>(o + S_ORDER / 2) = int4{P.row_of_slot[sl] * P.rowmul, 0, 0, 0};
                }
                at += __popcll(mo);
            }
            __builtin_amdgcn_wave_barrier();
            // (at == n_occ: both loops apply the same test to the same LDS values)
            const int far_units = (S_MOM * n_occ + 3) & ~3;            // the next header on a 64-byte boundary
            if (FILL && lane < far_units - S_MOM * n_occ) out[wpos + S_MOM * n_occ + lane] = ScratchEnt{0.0, 0, 0};
            wpos += far_units;
        }
    }
    const int units = (wpos + 3) & ~3;
    if (!FILL) {
        if (lane == 0) P.blob_units[t] = units;
    } else {
        if (lane == 0 && (int64_t)units != P.blob_prefix[t + 1] - P.blob_prefix[t]) atomicOr(P.status, 1);
    }
}

template <bool USE_LDS, bool PL = false>
__global__ __launch_bounds__(SITE_THREADS) void clr_scan_solo_kernel(ScanParams P, PrepView V) {
    extern __shared__ __attribute__((aligned(16))) double lds_R[];  // [rows][64] when USE_LDS, then one ring per wave
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nw = blockDim.x / WAVE;
#if BMX_SOLO_XCD_MAP
    // the slices of one chunk of test sites on one XCD, next to each other in its dispatch order (see the prepared kernel): every
    // slice reads all of the chunk's streams, and with this placement seven of the eight reads hit that XCD's L2
    const int xcd = blockIdx.x & 7;
    const int64_t q = blockIdx.x >> 3;
    const int slice = (int)(q % P.nslices);
    const int64_t chunk = (q / P.nslices) * 8 + xcd;
#else
    const int slice = blockIdx.x % P.nslices;
    const int64_t chunk = blockIdx.x / P.nslices;
#endif
    const int p = slice * WAVE + lane;
    if (USE_LDS) {
        const int total = P.rows * WAVE;
        for (int idx = threadIdx.x; idx < total; idx += blockDim.x)
            lds_R[idx] = P.Rt[(size_t)(idx >> 6) * P.NP + slice * WAVE + (idx & 63)];
    }
    const char *Rb = reinterpret_cast<const char *>(P.Rt + slice * WAVE);
    const unsigned lane8 = (unsigned)lane * 8u;
    auto loadR = [&](int rowoff) -> double {
        return USE_LDS ? lds_R[rowoff + lane] : *reinterpret_cast<const double *>(Rb + ((unsigned)rowoff * 8u + lane8));
    };
    constexpr int WAVE_UNITS = RING_UNITS + RING_MIRROR;
    ScratchEnt *ring = reinterpret_cast<ScratchEnt *>(lds_R + (USE_LDS ? P.rows * WAVE : 0)) + wave * WAVE_UNITS;
    double2 *ring2 = reinterpret_cast<double2 *>(ring);
    for (int idx = lane; idx < WAVE_UNITS; idx += WAVE) ring[idx] = ScratchEnt{0.0, 0, 0};
    if (USE_LDS) __syncthreads(); else __builtin_amdgcn_wave_barrier();
    const int rowmul = USE_LDS ? WAVE : P.NP;
    const double R0 = P.row0 >= 0 ? loadR(P.row0 * rowmul) : 0.0;       // the most frequent row of the data: its entries carry no row offset
    // every factor 1 + E R lies within 2^-54 .. 2^span_hi (or is exactly 0): P.renorm_every of them between two exponent extractions
    const int lim = P.renorm_every;

    const int64_t t_begin = chunk * P.sites_per_block;
    const int64_t t_end = min(t_begin + (int64_t)P.sites_per_block, P.M);
    for (int64_t t = t_begin + wave; t < t_end; t += nw) {
        // the stream of this test site through the ring, as in the prepared kernel
        const double2 *src = reinterpret_cast<const double2 *>(V.arena + (V.blob_prefix[V.grp_base + t] - V.prefix_base));
        int pos = 0, staged_u = 0;
        double nx_a, nx_b;
        {
            const double2 q0 = src[lane];
            nx_a = q0.x; nx_b = q0.y;
        }
        auto stage = [&]() {
            const int slot = (staged_u >> 6) & 3;
            ring2[slot * WAVE + lane] = double2{nx_a, nx_b};
            if (slot == 0 && lane < RING_MIRROR) ring2[RING_UNITS + lane] = double2{nx_a, nx_b};
            staged_u += WAVE;
            const double2 q0 = src[staged_u + lane];
            nx_a = q0.x; nx_b = q0.y;
            __builtin_amdgcn_wave_barrier();
        };
        auto need = [&]() {                   // [pos, pos + 80) is in the ring
            if (pos + 80 > staged_u) stage();
        };
        stage();
        stage();
        bool bad = false;
        double bestM = 0.5;                         // the product 1 = 0.5 * 2^1 in renorm_fx's convention: only a larger one wins (v1:451,501)
        int bestEc = 131072 + 1, bestA = -1;
        for (int iA = 0; iA < P.nA && !bad; ++iA) {
            double acc = 1.0;
            int E = 0, since = 0;
            int n_occ = 0, nfar = 0;
            for (;;) {
                need();
                const int4 *hp = reinterpret_cast<const int4 *>(ring + (pos & (RING_UNITS - 1)));
                const int4 h0 = hp[0], h1 = hp[1];
                const int magic = __builtin_amdgcn_readfirstlane(h0.x), n0 = __builtin_amdgcn_readfirstlane(h0.y);
                const int n1 = __builtin_amdgcn_readfirstlane(h0.z), nocc = __builtin_amdgcn_readfirstlane(h0.w);
                if ((magic & ~1) != SOLO_MAGIC || n0 < 0 || (n0 & 7) || n1 < 0 || (n1 & 3) || n0 > (int)P.N + 8 || n1 > (int)P.N + 8 || nocc < 0 || nocc > MOM_SLOTS) {
                    bad = true;
                    break;
                }
                pos += 4;
                // the most frequent row: two E per broadcast read, R in a register, eight entries per step
                for (int b = 0; b < n0; b += 8) {
                    need();
                    const double2 *ep = reinterpret_cast<const double2 *>(ring + (pos & (RING_UNITS - 1)));
                    double f[8];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const double2 e = ep[k];                       // uniform address: LDS broadcast
                        f[2 * k] = fma(e.x, R0, 1.0);
                        f[2 * k + 1] = fma(e.y, R0, 1.0);
                    }
                    if (since + 8 > lim) { renorm_fx(acc, E); since = 0; }
                    if (lim < 8) {
                        // span_hi >= 126: eight factors of up to 2^span_hi each do not fit between two exponent extractions (from
                        // 2^128 on their product alone leaves the double range) -- four, an extraction, four; lim >= 4 (set_model)
                        acc *= (f[0] * f[1]) * (f[2] * f[3]);
                        renorm_fx(acc, E);
                        acc *= (f[4] * f[5]) * (f[6] * f[7]);
                        since = 4;
                    } else {
                        acc *= ((f[0] * f[1]) * (f[2] * f[3])) * ((f[4] * f[5]) * (f[6] * f[7]));
                        since += 8;
                    }
                    pos += 4;
                }
                // the other rows: (E, row offset) per broadcast read, R from the LDS slice (or L2), four entries per step
                for (int b = 0; b < n1; b += 4) {
                    need();
                    const ScratchEnt *rp = ring + (pos & (RING_UNITS - 1));
                    double f[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const ScratchEnt en = rp[k];
                        f[k] = fma(en.e, loadR(en.ro), 1.0);
                    }
                    if (since + 4 > lim) { renorm_fx(acc, E); since = 0; }
                    acc *= (f[0] * f[1]) * (f[2] * f[3]);
                    since += 4;
                    pos += 4;
                }
                if (magic & 1) { n_occ = nocc; nfar = __builtin_amdgcn_readfirstlane(h1.x); break; }
            }
            if (bad) break;
            if (nfar) {
                // With F = 1 the series collapses per row: log factor = sum_rows sum_k c_k R^k, c_k = -+ w_k M_k premultiplied by the
                // preparation kernel -- one Horner chain in R per occupied row (both sides of the window at once)
                double tsum = 0.0;
                for (int s = 0; s < n_occ; ++s) {
                    need();
                    const ScratchEnt *rp = ring + (pos & (RING_UNITS - 1));
                    const double2 *qa = reinterpret_cast<const double2 *>(rp);
                    const int ro = reinterpret_cast<const int *>(rp + S_ORDER / 2)[0];
                    const double R = loadR(ro);
                    double hh = 0.0;
#pragma unroll
                    for (int k = S_ORDER - 1; k >= 0; --k) {
                        const double2 v = qa[k >> 1];
                        hh = fma(hh, R, (k & 1) ? v.y : v.x);
                    }
                    tsum = fma(hh, R, tsum);
                    pos += S_MOM;
                }
                pos = (pos + 3) & ~3;
                renorm_fx(acc, E);                   // |tsum| <= S_FAR_CAP * S_EPS * 1.1 < 600: 2^860 on top of [1/2, 1) is safe
                since = 0;
                acc *= exp_neg(-tsum);
            }
            renorm_fx(acc, E);
            const int ec = min(max(E, -131071), 131071) + 131072;
            if (((ec > bestEc) || (ec == bestEc && acc > bestM)) && acc > 0.0 && p < P.npairs) {       // strict '>' (v1:501); iA ascending
                bestM = acc;
                bestEc = ec;
                bestA = iA;
            }
            if constexpr (PL) {
                if (V.pl_am) {       // A profile: this A's best key over the slice's pairs (see the prepared kernel)
                    const bool beats = key_gt(ec, acc, 131072 + 1, 0.5) && acc > 0.0 && p < P.npairs;
                    int ek[1] = {beats ? ec : 0};
                    double mk[1] = {beats ? acc : 0.0};
                    pl_wave_max<1>(ek, mk, lane);
                    if (lane == 0) {
                        const size_t o = ((size_t)slice * P.nA + iA) * P.M + t;
                        V.pl_am[o] = mk[0];
                        V.pl_ae[o] = ek[0];
                    }
                }
            }
        }
        if (bad && lane == 0) atomicOr(V.status, 2);
        if constexpr (PL) {
            if (V.pl_pm) {       // x and alpha_beta profiles: this pair's best over A
                const bool any = bestA >= 0 && !bad;
                const size_t o = (size_t)t * P.NP + p;
                V.pl_pm[o] = any ? bestM : 0.0;
                V.pl_pe[o] = any ? bestEc : 0;
            }
        }
        int bE = bestEc;
        int bL = (bestA < 0 || bad) ? 0x7fffffff : bestA * P.npairs + p;
        for (int off = 32; off > 0; off >>= 1) {
            const int oE = __shfl_xor(bE, off);
            const double oM = __shfl_xor(bestM, off);
            const int oL = __shfl_xor(bL, off);
            if (oE > bE || (oE == bE && (oM > bestM || (oM == bestM && oL < bL)))) { bE = oE; bestM = oM; bL = oL; }
        }
        if (lane == 0) {
            const size_t o = (size_t)slice * P.M + t;
            P.part_T[o] = bestM;
            P.part_lin[o] = bL;
            P.part_ns[o] = bE;
        }
    }
}

// Combine the per-slice winners of a test site, take the one logarithm, and count nSites of the winning A
// (the scan kernels do not carry window sizes).  The count uses the scan's exact predicate:
// i in [lo,hi], A*|g_i - t| <= zcut, g_i != t; it is monotone on either side of the test site.
struct FinalParams {
    const double *part_T; const int32_t *part_lin; const int32_t *part_ns;
    int nslices, npairs;            // parts hold (mantissa, linear index, clamped exponent + 2^17) per slice
    int64_t M, N;
    const double *genpos, *A, *test_gen;
    const int64_t *win_lo, *win_hi, *center, *center_hi;
    double zcut;
    double *clr; int32_t *lin; int32_t *nsites;
    bmx_record *rec;   // the same three values as one 16-byte record per test site (what the multi-GPU gather moves)
    int *over;         // the slot's range word: set to 1 where a winner's exponent sits at the clamp (its CLR is past the range)
};

// A winning key (mantissa, clamped exponent + 2^17) to its CLR: the one conversion of the scan's result and of every profile entry
__device__ __forceinline__ double key_clr(double bM, int bE) {
    // kernels that normalise with v_frexp hand over mantissas in [1/2, 1): back to [1, 2), or a product just above 1 would come
    // out as LN2 + log(0.5000...) -- a difference of two numbers of size 0.69
    if (bM < 1.0) { bM *= 2.0; bE -= 1; }
    return 2.0 * ((double)(bE - 131072) * LN2 + log(bM));
}

__global__ void finalize_kernel(FinalParams F) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= F.M) return;
    double bT = 0.0;
    int bL = 0x7fffffff, bN = 0;
    double bM = 1.0;
    int bE = 131072;
    for (int s = 0; s < F.nslices; ++s) {
        const double m = F.part_T[(size_t)s * F.M + t];
        const int L = F.part_lin[(size_t)s * F.M + t];
        const int e = F.part_ns[(size_t)s * F.M + t];
        if (L != 0x7fffffff && (e > bE || (e == bE && (m > bM || (m == bM && L < bL))))) {
            bM = m;
            bE = e;
            bL = L;
        }
    }
    if (bL != 0x7fffffff) bT = key_clr(bM, bE);
    const bool none = (bL == 0x7fffffff);
    if (!none) {
        // a winner AT the clamp (ec = 131071 + 2^17) may have been cut: its CLR, and its order among such grid points, is not known
        if (bE >= 131071 + 131072) *F.over = 1;
        const double A = F.A[bL / F.npairs], tg = F.test_gen[t];
        const int64_t lo = max(F.win_lo[t], (int64_t)0), hi = min(F.win_hi[t], F.N - 1);
        // right of the test position: indices [a0, hi], predicate true on a prefix
        int64_t a0 = max(F.center_hi[t], lo), a = a0, b = hi + 1;
        while (a < b) {
            int64_t m = (a + b) >> 1;
            if (A * fabs(F.genpos[m] - tg) <= F.zcut) a = m + 1; else b = m;
        }
        int64_t cnt = max(a - a0, (int64_t)0);
        // left: indices [lo, b0], predicate true on a suffix
        int64_t b0 = min(F.center[t] - 1, hi);
        a = lo; b = b0 + 1;
        while (a < b) {
            int64_t m = (a + b) >> 1;
            if (A * fabs(F.genpos[m] - tg) <= F.zcut) b = m; else a = m + 1;
        }
        cnt += max(b0 + 1 - a, (int64_t)0);
        bN = (int)cnt;
    }
    F.clr[t] = none ? 0.0 : bT;
    F.lin[t] = none ? -1 : bL;
    F.nsites[t] = none ? 0 : bN;
    F.rec[t] = bmx_record{none ? 0.0 : bT, none ? -1 : bL, none ? 0 : bN};
}

// Profile likelihoods of one launch range: entry (t, v) of profile `kind` (0: A, 1: x, 2: alpha_beta) is the largest key over
// the slices (A) or over the pairs with that x / alpha_beta, converted by key_clr; +0.0 where no key beat T = 0.  One thread
// per entry; no atomics, so the result does not depend on the launch order.  Neighbouring threads take neighbouring keys: test
// sites fastest for A ([slice][A][t]), grid values fastest for x and alpha_beta ([t][pair], pair = ix * nab + ia).
struct PlFinalParams {
    const double *am; const int32_t *ae;       // [nslices][nA][M]
    const double *pm; const int32_t *pe;       // [M][NP]
    int kind, nslices, nA, nx, nab, NP;
    int64_t M;
    double *out;                               // [M][n] of the kind, grid order
};

__global__ void profile_finalize_kernel(PlFinalParams F) {
    const int n = F.kind == 0 ? F.nA : F.kind == 1 ? F.nx : F.nab;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= F.M * n) return;
    const int64_t t = F.kind == 0 ? i % F.M : i / n;
    const int v = (int)(F.kind == 0 ? i / F.M : i % n);
    int be = 0;
    double bm = 0.0;
    auto take = [&](double m, int e) {
        if (key_gt(e, m, be, bm)) { be = e; bm = m; }
    };
    if (F.kind == 0) {
        for (int s = 0; s < F.nslices; ++s) {
            const size_t o = ((size_t)s * F.nA + v) * F.M + t;
            take(F.am[o], F.ae[o]);
        }
    } else if (F.kind == 1) {
        const size_t o = (size_t)t * F.NP + (size_t)v * F.nab;
        for (int ia = 0; ia < F.nab; ++ia) take(F.pm[o + ia], F.pe[o + ia]);
    } else {
        const size_t o = (size_t)t * F.NP + v;
        for (int ix = 0; ix < F.nx; ++ix) take(F.pm[o + (size_t)ix * F.nab], F.pe[o + (size_t)ix * F.nab]);
    }
    F.out[(size_t)t * n + v] = be ? key_clr(bm, be) : 0.0;
}

// ----------------------------------------------------------------------------- surface
// Full likelihood surface T[iA][pair] of ONE test site (the reference keeps only the maximum and
// notes the surfaces as a wish, v1:449-450).  Deliberately a different arithmetic from the scan
// kernels -- a plain sum of log1p(alpha*R) per (A, pair) -- so that it doubles as an on-device
// cross-check of the product form.  One workgroup per (A, 64-pair slice); lanes = pairs.
struct SurfParams {
    const double *genpos; RowArray row; int64_t N;
    const double *Rt; int NP, npairs, nslices;
    const double *A; int nA;
    double tg; int64_t lo, hi;
    double zcut;
    double *T;        // [nA][npairs]
    int32_t *ns;      // [nA]
};

__global__ void surface_kernel(SurfParams S) {
    const int iA = blockIdx.x / S.nslices, slice = blockIdx.x % S.nslices;
    const int lane = threadIdx.x;
    const int p = slice * WAVE + lane;
    const double A = S.A[iA];
    double sum = 0.0;
    int ns = 0;
    for (int64_t base = S.lo; base <= S.hi; base += WAVE) {
        const int64_t i = base + lane;
        const bool valid = i <= S.hi;
        const double g = valid ? S.genpos[i] : S.tg;
        const double z = A * fabs(g - S.tg);
        const bool in = valid && z <= S.zcut && g != S.tg;
        const double alpha = in ? exp(-z) : 0.0;
        const int r = valid ? (int)S.row[i] : 0;
        const unsigned long long m = __ballot(in);
        ns += __popcll(m);
        for (unsigned long long mm = m; mm; mm &= mm - 1) {
            const int l = __ffsll((long long)mm) - 1;
            const double a_s = readlane_f64(alpha, l);
            const int r_s = __builtin_amdgcn_readlane(r, l);
            sum += log1p(a_s * S.Rt[(size_t)r_s * S.NP + p]);
        }
    }
    if (p < S.npairs) S.T[(size_t)iA * S.npairs + p] = ns ? 2.0 * sum : NAN;
    if (slice == 0 && lane == 0) S.ns[iA] = ns;
}

// ----------------------------------------------------------------------------- refinement
// Off-grid polish of each window's grid argmax (bmx_ctx_refine / bmx_ctx_eval_points; the definition, which the CPU tests run
// on a host restatement of T, is ballermixplus_amd/refine.py).  The objective at an arbitrary point (A, x, alpha_beta) is
//     T = 2 * sum_i log1p(alpha_i R_i),  alpha_i = exp(-A |g_i - t|),  over i in [win_lo, win_hi] with A |g_i - t| <= zcut, g_i != t,
//     R_i = psel(k_i, n_i | x, alpha_beta) * prop(n_i) / g(k_i, n_i) - 1          (-inf: no such site; non-finite: -inf)
// with psel computed as K1 computes it for grid points (refine_psel is K1's arithmetic, one inlined pmf call site inside loops).
// K1's LogPatch covers only the logs of the grid's arguments; off the grid the device's correctly rounded log is used as it
// is -- at most one unit in the last place of a log inside lgam, far below the 1e-9 to which the tests compare T.
// A compass search in (u = ln A, x, v = ln alpha_beta) starts at the scan's argmax.  One workgroup per window, grid-striding
// over a device-compacted list of the windows to refine.  Each round:
//   1. thread 0 lays out the <= 6 candidates (u-, u+, x-, x+, v-, v+, clamped to the grid's hull; one that clamps onto the
//      centre is skipped); wave 0 finds the site range of the smallest A among them (64-way search on genpos), once per A;
//   2. the rows that range references are marked in a byte map (plain stores of 1: no atomics) and compacted in order; the
//      R entries of the new (x, alpha_beta) candidates -- and of the centre when it changed -- are built for those rows only,
//      in LDS when the workspace fits REFINE_LDS_WS, else in a per-workgroup global slab;
//   3. threads stride over the sites ALIGNED TO THE SITE INDEX (site i goes to thread i % REFINE_THREADS, in increasing i), so
//      a point's T does not depend on the range it was summed over, on the round that summed it or on the launch;
//   4. the per-thread sums are reduced in a fixed order (xor butterfly in each wave, then the waves in order); thread 0
//      decides the move (strict '>', first in order wins ties; no move halves every step) and broadcasts it through LDS.
// No atomics: a window's result is a function of that window alone.
constexpr int REFINE_THREADS = 256;
constexpr int REFINE_WAVES = REFINE_THREADS / WAVE;
constexpr int64_t REFINE_LDS_WS = 32 * 1024;     // workspace bytes held in LDS (else the global slab)
constexpr int REFINE_TABS = 5;                   // R entries of: the centre, x-, x+, v-, v+
constexpr int REFINE_EVALS = 7;                  // T of: the centre, u-, u+, x-, x+, v-, v+
constexpr int REFINE_GRID_MAX = 2048;            // workgroups of a refinement launch (grid-stride over the windows)

// A slot's sites and its windows, as the compass, surfaces, influence and fit kernels take them (window_range, tile_site)
struct SiteView { const double *genpos; RowArray row; int64_t N; };
struct WindowView { const double *test_gen; const int64_t *win_lo, *win_hi; double zcut; };

struct RefineParams {
    int stat, min_count, n_sizes, rows;
    const int32_t *sizes, *row_off;
    const double *g, *prop;
    const double *gA, *gx, *gab;       // the model's grids
    int npairs, nab;
    const double *cu, *cv;             // ln of every grid A / alpha_beta (the host's log: a start's coordinates)
    const double *h0u, *h0x, *h0v;     // initial step at every grid value
    double lo[3], hi[3], tol[3];       // hull and tolerance of u, x, v
    int fr[3];                         // 1: the coordinate is free
    int max_rounds;
    SiteView sites; WindowView win;
    const int32_t *list; const int64_t *count;     // refine: the windows to refine; point evaluation: nullptr (all M)
    int64_t M;
    const int32_t *lin; const double *clr;         // refine: the last scan
    const double *pA, *px, *pab;                   // point evaluation: the points
    char *slab; int64_t ws_bytes; int ws_lds;      // workspace: [REFINE_TABS][rows] f64, [rows] i32 list, [rows] u8 map
    double *o_clr, *o_A, *o_x, *o_ab;
    int32_t *o_ns, *o_rounds;
};

// bmx::betabinom_pmf without a LogPatch, operation for operation, with its three log-beta terms from ONE inlined call site in
// a loop the compiler may not unroll.  (Every function of bmx_math.h is inlined; with three copies of lbeta_pos, or with
// the pmf unrolled, a loop around the pmf spans more than a branch instruction reaches and the compiler would have to jump
// with s_setpc_b64.)
__device__ __forceinline__ double refine_pmf(int k, int n, double a, double b) {
    if (k < 0 || k > n) return 0.0;
    double l0 = 0., l1 = 0., l2 = 0.;
#pragma nounroll
    for (int i = 0; i < 3; ++i) {
        const double p = i == 0 ? (double)(n - k + 1) : i == 1 ? k + a : a;
        const double q = i == 0 ? (double)(k + 1) : i == 1 ? n - k + b : b;
        const double v = bmx::cephes::lbeta_pos(p, q, bmx::LogPatch{nullptr, nullptr, 0});
        if (i == 0) l0 = v; else if (i == 1) l1 = v; else l2 = v;
    }
    const double combiln = -bmx::crlog((double)(n + 1)) - l0;
    const double lpm = combiln + l1 - l2;
    double p = exp(lpm);
    if (p < 0.0) p = 0.0;
    if (p > 1.0) p = 1.0;
    return p;
}

// R of LUT row r at (x, alpha_beta): bb_lut_kernel's arithmetic (refine_pmf for its pmf), in loops that are not unrolled.
__device__ __forceinline__ double refine_R(const RefineParams &P, int r, double x, double a) {
    int j = 0;
    while (j + 1 < P.n_sizes && r >= P.row_off[j + 1]) j++;
    const int n = P.sizes[j], k = r - P.row_off[j];
    const double xm = 1. - x;
    const double b1 = a / x - a, b2 = a / xm - a;
    const int m = P.min_count, stat = P.stat;
    const bool maf = (stat == BMX_STAT_B2MAF || stat == BMX_STAT_B0MAF);
    int nex = m;
    if (stat == BMX_STAT_B2MAF) nex += (m - 1 > 0 ? m - 1 : 0);
    if (stat == BMX_STAT_B0) nex += 1;
    if (stat == BMX_STAT_B0MAF) nex += m;
    const int nblk = nex < 8 ? 0 : nex - (nex % 8);
    double r8[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
    double res = 0.;
    double raw = 0.;
#pragma nounroll
    for (int it = 0; it <= nex; ++it) {
        const bool site = (it == nex);
        int c;
        if (site) c = (stat == BMX_STAT_B1) ? n : k;
        else if (it < m) c = it;
        else if (stat == BMX_STAT_B0) c = n;
        else c = n - m + 1 + (it - m);
        const int nfold = (site && maf) ? 2 : 1;
        double v0 = 0., v1 = 0., pr = 0.;
#pragma nounroll
        for (int sf = 0; sf < 2 * nfold; ++sf) {        // (side, fold) pairs: b(x) then b(1 - x)
            const int side = sf / nfold, f = sf % nfold;
            const double q = refine_pmf(f ? n - c : c, n, a, side ? b2 : b1);
            pr = f ? pr + q : q;
            if (f == nfold - 1) {
                if (site && maf && (n % 2 == 0) && c == n / 2) pr = pr / 2;
                if (site && stat == BMX_STAT_B1) pr = (k == 0) ? pr : (1. - pr - pr);
                if (side) v1 = pr; else v0 = pr;
            }
        }
        const double e = 0.5 * (v0 + v1);
        if (site) {
            raw = e;
        } else if (nex < 8) {
            res += e;
        } else if (it < nblk) {
            if (it < 8) r8[it] = e; else r8[it & 7] += e;
            if (it == nblk - 1)
                res = ((r8[0] + r8[1]) + (r8[2] + r8[3])) + ((r8[4] + r8[5]) + (r8[6] + r8[7]));
        } else {
            res += e;
        }
    }
    const double psel = raw / (1. - res);
    return psel * P.prop[j] / P.g[r] - 1.0;
}

// First index in [a, b) where pred holds (pred: false ... false true ... true on [a, b)), b if none.  All 64 lanes of one
// wave call it with the same arguments; 64 probes per step.
template <class F>
__device__ __forceinline__ int64_t wave_first_true(int64_t a, int64_t b, F pred) {
    const int lane = threadIdx.x % WAVE;
    while (a < b) {
        const int64_t n = b - a;
        const int64_t step = (n + WAVE - 1) / WAVE;
        const int64_t p = min(a + (int64_t)(lane + 1) * step - 1, b - 1);
        const unsigned long long m = __ballot(pred(p));
        if (!m) return b;
        const int L = __ffsll((long long)m) - 1;
        const int64_t pL = min(a + (int64_t)(L + 1) * step - 1, b - 1);
        const int64_t pP = L ? min(a + (int64_t)L * step - 1, b - 1) : a - 1;
        a = pP + 1;
        b = pL;         // pred(pL) holds: the answer is in [a, pL) or is pL
        if (a >= b) return pL;
        if (step == 1) return pL;
    }
    return b;
}

// ---- the sites of window t at one A: i in [max(win_lo, 0), min(win_hi, N - 1)] with A |g_i - tg| <= zcut and g_i != tg, stated
// once for the surfaces, influence and fit kernels.  (The scan kernels, surface_kernel -- the single-window cross-check -- and the
// compass kernels keep their own text: compass_begin and compass_round run these searches apart, and sharing them through a
// split helper moved refine_kernel's schedule and cost it time, profiles/listed_window_fold.txt.)
// All 64 lanes of a wave: the first site of the clipped window at or right of tg (ctr), and around it -- A |g_i - tg| being
// monotone on either side -- the sites [a, b) that A's cut can hold.
struct SiteRange { int64_t ctr, a, b; };
__device__ __forceinline__ SiteRange window_range(const SiteView &V, const WindowView &W, int64_t t, double tg, double A) {
    const int64_t wlo = max(W.win_lo[t], (int64_t)0), whi = min(W.win_hi[t], V.N - 1);
    const double zc = W.zcut;
    SiteRange R;
    R.ctr = wave_first_true(wlo, whi + 1, [&](int64_t i) { return V.genpos[i] >= tg; });
    R.a = wave_first_true(wlo, R.ctr, [&](int64_t i) { return A * fabs(V.genpos[i] - tg) <= zc; });
    R.b = wave_first_true(R.ctr, whi + 1, [&](int64_t i) { return !(A * fabs(V.genpos[i] - tg) <= zc); });
    return R;
}

// Site i = base + tid of a tile over [.., hi]: is it one of A's sites (`in`), and its z = A |g_i - tg|; its (alpha, row) into the
// workgroup's tile (row -1: not `in`); the term a pair p adds for the tile's entry (alpha_s, r_s >= 0)
__device__ __forceinline__ bool tile_site(const double *genpos, int64_t i, int64_t hi, double tg, double A, double zc, double &z) {
    const bool valid = i <= hi;
    const double g = valid ? genpos[i] : tg;
    z = A * fabs(g - tg);
    return valid && z <= zc && g != tg;
}
__device__ __forceinline__ void tile_store(const RowArray &row, int64_t i, bool in, double z, double *s_alpha, int *s_row) {
    s_alpha[threadIdx.x] = in ? exp(-z) : 0.0; s_row[threadIdx.x] = in ? (int)row[i] : -1;
}
__device__ __forceinline__ double tile_term(double alpha_s, int r_s, const double *Rt, int NP, int p) { return log1p(alpha_s * Rt[(size_t)r_s * NP + p]); }

__device__ const uint64_t BOOT_THR[20] = {     // floor(2^64 * Poisson(1).cdf(k)), k = 0..19 (boot.py THR)
    6786177901268885274ull, 13572355802537770549ull, 16965444753172213186ull, 18096474403383694065ull, 18379231815936564285ull,
    18435783298447138329ull, 18445208545532234003ull, 18446555009401533385ull, 18446723317385195808ull, 18446742018272269410ull,
    18446743888360976771ull, 18446744058369041076ull, 18446744072536379768ull, 18446744073626175052ull, 18446744073704017573ull,
    18446744073709207074ull, 18446744073709531418ull, 18446744073709550497ull, 18446744073709551557ull, 18446744073709551613ull};

// w(key, b) of boot.py: the number of thresholds at or below the hash (ascending table: stop at the first one above it)
__device__ __forceinline__ int boot_weight(uint64_t key, uint64_t b) {
    const uint64_t h = bmx_mix64(key ^ bmx_mix64(b));
    int w = 0;
    while (w < 20 && h >= BOOT_THR[w]) ++w;
    return w;
}

// The weight of a site in the sums of a round, carried along a thread's stride of REFINE_THREADS sites: start(i) at the thread's
// first site, then one next() per site.  count_t holds a thread's total weight inside a cut.
struct UnitWeight {                 // T: every site once (refine_kernel, support_kernel)
    using count_t = int;
    __device__ __forceinline__ void start(int64_t) {}
    __device__ __forceinline__ int next() { return 1; }
};

struct BootWeight {                 // T_w: w_i = boot_weight(key, i / B) (boot_kernel)
    using count_t = long long;
    uint64_t key, B, qB, rB;        // qB, rB: REFINE_THREADS / B and REFINE_THREADS % B
    uint64_t blk, rem;              // i / B and i % B, carried along with i: no division in the loop
    __device__ __forceinline__ void start(int64_t i) { blk = (uint64_t)i / B; rem = (uint64_t)i % B; }
    __device__ __forceinline__ int next() {
        const int w = boot_weight(key, blk);
        blk += qB; rem += rB;
        if (rem >= B) { rem -= B; blk++; }
        return w;
    }
};

struct RefineState {
    double c[3], nat[3];            // the centre: coordinates (u, x, v) and natural values (A, x, alpha_beta)
    double c0[3], nat0[3];          // the start
    double h[3];
    double Tc;
    long long nsc;                  // sites (BootWeight: total weight) inside the cut of the centre's A
    int have_c, rounds, phase, cand;
    int valid[REFINE_EVALS];        // the evaluations of the last round laid out ...
    double T[REFINE_EVALS];         // ... and their T where that round summed (for the caller's thread 0, after the round)
    double cc[REFINE_EVALS][3], cn[REFINE_EVALS][3];
    double Aev[3];                  // A of the centre, u-, u+
    int need_tab[REFINE_TABS];
    double tx[REFINE_TABS], tab_ab[REFINE_TABS];
    double built_x0, built_ab0;     // (x, alpha_beta) the centre's entries hold, for rows version built_rv0 (-1: none)
    int built_rv0;
    double rangeA;                  // the A the current range and row list were made for (0: none)
    int64_t ctr, wlo, whi, rlo, rhi;
    int nused, rv;
    double tg;
    double red[REFINE_WAVES][REFINE_EVALS];
    long long redn[REFINE_WAVES][3];
    int wtot[REFINE_WAVES];
};

__device__ __forceinline__ double refine_nat(const RefineState &S, int k, double v) {
    return v == S.c0[k] ? S.nat0[k] : (k == 1 ? v : exp(v));
}

// A workgroup's workspace, in LDS or in its slab: [REFINE_TABS][rows] f64 tables, [rows] i32 row list, [rows] u8 row map
struct CompassWs {
    double *tab; int32_t *list; uint8_t *map;
};

__device__ __forceinline__ CompassWs compass_ws(const RefineParams &P, double *lds_ws) {
    char *ws = P.ws_lds ? (char *)lds_ws : P.slab + (size_t)blockIdx.x * (size_t)P.ws_bytes;
    CompassWs W;
    W.tab = (double *)ws;
    W.list = (int32_t *)(ws + (size_t)REFINE_TABS * P.rows * sizeof(double));
    W.map = (uint8_t *)(W.list + P.rows);
    return W;
}

// Thread 0, a start: point t of a point evaluation (no steps: nothing to search) ...
__device__ __forceinline__ void compass_start_point(const RefineParams &P, RefineState &S, int64_t t) {
    S.nat0[0] = P.pA[t]; S.nat0[1] = P.px[t]; S.nat0[2] = P.pab[t];
    S.c0[0] = log(P.pA[t]); S.c0[1] = P.px[t]; S.c0[2] = log(P.pab[t]);
    S.h[0] = S.h[1] = S.h[2] = 0.0;
}

// ... or the refined point (rA, rx, rab)[t] of window t, with the grid start's own coordinate where a value is the grid's; the
// grid start's steps go to h0
__device__ __forceinline__ void compass_start_refined(const RefineParams &P, RefineState &S, int64_t t, const double *rA,
                                                      const double *rx, const double *rab, double *h0) {
    const int L = P.lin[t], iA = L / P.npairs, p = L % P.npairs, ix = p / P.nab, ia = p % P.nab;
    const double g0[3] = {P.gA[iA], P.gx[ix], P.gab[ia]}, gc[3] = {P.cu[iA], P.gx[ix], P.cv[ia]};
    S.nat0[0] = rA[t]; S.nat0[1] = rx[t]; S.nat0[2] = rab[t];
    for (int k = 0; k < 3; ++k) S.c0[k] = S.nat0[k] == g0[k] ? gc[k] : (k == 1 ? S.nat0[k] : log(S.nat0[k]));
    h0[0] = P.h0u[iA]; h0[1] = P.h0x[ix]; h0[2] = P.h0v[ia];
}

// All threads, once per window, after thread 0 set the start (S.c0, S.nat0, S.h): the centre at the start, nothing evaluated
// or built, and the window -- its bounds and the first site at or right of the test position
__device__ __forceinline__ void compass_begin(const RefineParams &P, RefineState &S, int64_t t) {
    if (threadIdx.x == 0) {
        for (int k = 0; k < 3; ++k) { S.c[k] = S.c0[k]; S.nat[k] = S.nat0[k]; }
        S.Tc = -INFINITY; S.nsc = 0; S.have_c = 0; S.rounds = 0;
        S.built_rv0 = -1; S.rangeA = 0.0; S.rv = 0; S.nused = 0;
        S.tg = P.win.test_gen[t];
        S.wlo = max(P.win.win_lo[t], (int64_t)0);
        S.whi = min(P.win.win_hi[t], P.sites.N - 1);
    }
    __syncthreads();
    if (threadIdx.x / WAVE == 0) {
        const double tg = S.tg;
        const int64_t ctr = wave_first_true(S.wlo, S.whi + 1, [&](int64_t i) { return P.sites.genpos[i] >= tg; });
        if (threadIdx.x % WAVE == 0) S.ctr = ctr;
    }
}

// One round of the compass search (steps 1-4 above) over the free coordinates fr[3], with the site weights wt: the one text of
// refine_kernel, support_kernel and boot_kernel.  All threads of the workgroup call it; false: the search has ended (converged
// or out of rounds, nothing left to evaluate) at the centre S.c / S.nat with S.Tc and S.nsc.  After a round thread 0 finds in
// S.valid[] what it evaluated and in S.T[] the values, until it lays out the next one.
template <class W>
__device__ __forceinline__ bool compass_round(const RefineParams &P, RefineState &S, const int *fr, const CompassWs &ws, W wt) {
    const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE;
    // ---- 1. the round's candidates (thread 0)
    if (tid == 0) {
        for (int e = 0; e < REFINE_EVALS; ++e) S.valid[e] = 0;
        S.valid[0] = !S.have_c;
        bool conv = true;
        for (int k = 0; k < 3; ++k)
            if (fr[k] && !(S.h[k] < P.tol[k])) conv = false;
        S.cand = S.rounds < P.max_rounds && !conv;
        if (S.cand) {
            for (int d = 0; d < 6; ++d) {
                const int k = d >> 1;
                if (!fr[k]) continue;
                const double v = min(max((d & 1) ? S.c[k] + S.h[k] : S.c[k] - S.h[k], P.lo[k]), P.hi[k]);
                if (v == S.c[k]) continue;
                S.valid[d + 1] = 1;
                for (int q = 0; q < 3; ++q) { S.cc[d + 1][q] = S.c[q]; S.cn[d + 1][q] = S.nat[q]; }
                S.cc[d + 1][k] = v;
                S.cn[d + 1][k] = refine_nat(S, k, v);
            }
        }
        bool any = false;
        for (int e = 0; e < REFINE_EVALS; ++e) any = any || S.valid[e];
        S.phase = any ? 1 : S.cand ? 2 : 0;
        S.Aev[0] = S.nat[0];
        S.Aev[1] = S.valid[1] ? S.cn[1][0] : S.nat[0];
        S.Aev[2] = S.valid[2] ? S.cn[2][0] : S.nat[0];
        S.need_tab[0] = S.valid[0] || S.valid[1] || S.valid[2];
        S.tx[0] = S.nat[1]; S.tab_ab[0] = S.nat[2];
        for (int q = 1; q < REFINE_TABS; ++q) {
            S.need_tab[q] = S.valid[q + 2];
            S.tx[q] = S.valid[q + 2] ? S.cn[q + 2][1] : S.nat[1];
            S.tab_ab[q] = S.valid[q + 2] ? S.cn[q + 2][2] : S.nat[2];
        }
    }
    __syncthreads();
    const int phase = S.phase;
    if (phase == 0) return false;
    if (phase == 2) {       // every candidate clamps onto the centre: halve
        if (tid == 0) {
            for (int k = 0; k < 3; ++k) S.h[k] *= 0.5;
            S.rounds++;
        }
        __syncthreads();
        return true;
    }
    const double tg = S.tg;
    // ---- the site range of the smallest A of the round, and the rows it references
    double Amin = S.Aev[0];
    if (S.valid[1]) Amin = min(Amin, S.Aev[1]);
    if (S.valid[2]) Amin = min(Amin, S.Aev[2]);
    if (Amin != S.rangeA) {
        if (wave == 0) {
            const double zc = P.win.zcut;
            const int64_t ctr = S.ctr;
            const int64_t a = wave_first_true(S.wlo, ctr, [&](int64_t i) { return Amin * fabs(P.sites.genpos[i] - tg) <= zc; });
            const int64_t b = wave_first_true(ctr, S.whi + 1, [&](int64_t i) { return !(Amin * fabs(P.sites.genpos[i] - tg) <= zc); });
            if (lane == 0) { S.rlo = a; S.rhi = b - 1; }
        }
        for (int r = tid; r < P.rows; r += REFINE_THREADS) ws.map[r] = 0;
        __syncthreads();
        for (int64_t i = S.rlo + tid; i <= S.rhi; i += REFINE_THREADS) ws.map[P.sites.row[i]] = 1;
        __syncthreads();
        int base = 0;
        for (int r0 = 0; r0 < P.rows; r0 += REFINE_THREADS) {
            const int r = r0 + tid;
            const bool on = r < P.rows && ws.map[r];
            const unsigned long long m = __ballot(on);
            if (lane == 0) S.wtot[wave] = __popcll(m);
            __syncthreads();
            int off = base;
            for (int q = 0; q < wave; ++q) off += S.wtot[q];
            if (on) ws.list[off + __popcll(m & ((1ull << lane) - 1ull))] = r;
            for (int q = 0; q < REFINE_WAVES; ++q) base += S.wtot[q];
            __syncthreads();
        }
        if (tid == 0) { S.nused = base; S.rangeA = Amin; S.rv++; }
        __syncthreads();
    }
    // ---- 2. R entries of the tables this round needs (the centre's only when its (x, alpha_beta) or rows changed)
    {
        int qmask = 0, nq = 0;          // the tables to build, as a bit set (an indexed array goes to scratch in boot_kernel)
        const bool keep0 = S.built_rv0 == S.rv && S.built_x0 == S.tx[0] && S.built_ab0 == S.tab_ab[0];
        for (int q = 0; q < REFINE_TABS; ++q)
            if (S.need_tab[q] && !(q == 0 && keep0)) { qmask |= 1 << q; nq++; }
        const int nu = S.nused;
        for (int it = tid; it < nq * nu; it += REFINE_THREADS) {
            int m = qmask;
            for (int j = it / nu; j > 0; --j) m &= m - 1;
            const int q = __ffs(m) - 1, r = ws.list[it % nu];
            ws.tab[(size_t)q * P.rows + r] = refine_R(P, r, S.tx[q], S.tab_ab[q]);
        }
        __syncthreads();
        if (tid == 0 && S.need_tab[0]) { S.built_rv0 = S.rv; S.built_x0 = S.tx[0]; S.built_ab0 = S.tab_ab[0]; }
    }
    // ---- 3. the (weighted) site sums, aligned to the site index; a site of weight 0 skips its loads and its exp / log1p
    double acc[REFINE_EVALS];
    typename W::count_t ns[3] = {0, 0, 0};
    for (int e = 0; e < REFINE_EVALS; ++e) acc[e] = 0.0;
    {
        int vmask = 0;
        for (int e = 0; e < REFINE_EVALS; ++e) vmask |= S.valid[e] << e;
        const double A0 = S.Aev[0], A1 = S.Aev[1], A2 = S.Aev[2], zc = P.win.zcut;
        const int64_t lo = S.rlo, hi = S.rhi;
        int64_t i = lo - (lo % REFINE_THREADS) + tid;
        if (i < lo) i += REFINE_THREADS;
        if (i <= hi) wt.start(i);
        for (; i <= hi; i += REFINE_THREADS) {
            const int wi = wt.next();
            if (wi == 0) continue;
            const double wd = (double)wi;
            const double gi = P.sites.genpos[i];
            const int r = P.sites.row[i];
            const double d = fabs(gi - tg);
            const bool same = gi == tg;
            const double z0 = A0 * d, z1 = A1 * d, z2 = A2 * d;
            const bool in0 = z0 <= zc && !same, in1 = z1 <= zc && !same, in2 = z2 <= zc && !same;
            const double a0 = exp(-z0);
            if (in0) ns[0] += wi;
            if (in1) ns[1] += wi;
            if (in2) ns[2] += wi;
            if (vmask & 1) { const double v = log1p(a0 * ws.tab[r]); if (in0) acc[0] += wd * v; }
            if (vmask & 2) { const double v = log1p(exp(-z1) * ws.tab[r]); if (in1) acc[1] += wd * v; }
            if (vmask & 4) { const double v = log1p(exp(-z2) * ws.tab[r]); if (in2) acc[2] += wd * v; }
            for (int q = 1; q < REFINE_TABS; ++q)
                if (vmask & (1 << (q + 2))) { const double v = log1p(a0 * ws.tab[(size_t)q * P.rows + r]); if (in0) acc[q + 2] += wd * v; }
        }
    }
    // ---- 4. fixed-order reduction, the decision
    for (int off = 1; off < WAVE; off <<= 1) {
        for (int e = 0; e < REFINE_EVALS; ++e) acc[e] += __shfl_xor(acc[e], off);
        for (int k = 0; k < 3; ++k) ns[k] += __shfl_xor(ns[k], off);
    }
    if (lane == 0) {
        for (int e = 0; e < REFINE_EVALS; ++e) S.red[wave][e] = acc[e];
        for (int k = 0; k < 3; ++k) S.redn[wave][k] = ns[k];
    }
    __syncthreads();
    if (tid == 0) {
        long long nk[3];
        for (int k = 0; k < 3; ++k) nk[k] = (S.redn[0][k] + S.redn[1][k]) + (S.redn[2][k] + S.redn[3][k]);
        for (int e = 0; e < REFINE_EVALS; ++e) {
            const double s = (S.red[0][e] + S.red[1][e]) + (S.red[2][e] + S.red[3][e]);
            const long long n = nk[e == 1 ? 1 : e == 2 ? 2 : 0];
            const double v = 2.0 * s;
            S.T[e] = (n > 0 && isfinite(v)) ? v : -INFINITY;
        }
        if (S.valid[0]) { S.Tc = S.T[0]; S.nsc = nk[0]; S.have_c = 1; }
        if (S.cand) {
            double best = S.Tc;
            int bi = -1;
            for (int e = 1; e < REFINE_EVALS; ++e)
                if (S.valid[e] && S.T[e] > best) { best = S.T[e]; bi = e; }
            if (bi >= 0) {
                for (int k = 0; k < 3; ++k) { S.c[k] = S.cc[bi][k]; S.nat[k] = S.cn[bi][k]; }
                S.Tc = best;
                S.nsc = nk[bi == 1 ? 1 : bi == 2 ? 2 : 0];
            } else {
                for (int k = 0; k < 3; ++k) S.h[k] *= 0.5;
            }
            S.rounds++;
        }
    }
    __syncthreads();
    return true;
}

__global__ __launch_bounds__(REFINE_THREADS) void refine_kernel(RefineParams P) {
    extern __shared__ __attribute__((aligned(16))) double lds_ws[];
    __shared__ RefineState S;
    const int tid = threadIdx.x;
    const CompassWs ws = compass_ws(P, lds_ws);
    const int64_t count = P.list ? *P.count : P.M;
    for (int64_t w = blockIdx.x; w < count; w += gridDim.x) {
        const int64_t t = P.list ? (int64_t)P.list[w] : w;
        if (tid == 0) {
            if (P.list) {           // the scan's argmax, with the host's coordinates and steps of its grid values
                const int L = P.lin[t], iA = L / P.npairs, p = L % P.npairs, ix = p / P.nab, ia = p % P.nab;
                S.nat0[0] = P.gA[iA]; S.nat0[1] = P.gx[ix]; S.nat0[2] = P.gab[ia];
                S.c0[0] = P.cu[iA]; S.c0[1] = P.gx[ix]; S.c0[2] = P.cv[ia];
                S.h[0] = P.h0u[iA]; S.h[1] = P.h0x[ix]; S.h[2] = P.h0v[ia];
            } else {
                compass_start_point(P, S, t);
            }
        }
        compass_begin(P, S, t);
        while (compass_round(P, S, P.fr, ws, UnitWeight())) {}
        if (tid == 0) {
            if (P.list) {
                if (S.Tc > P.clr[t]) {
                    P.o_clr[t] = S.Tc; P.o_A[t] = S.nat[0]; P.o_x[t] = S.nat[1]; P.o_ab[t] = S.nat[2]; P.o_ns[t] = (int32_t)S.nsc;
                }
                P.o_rounds[t] = S.rounds;
            } else {
                P.o_clr[t] = S.Tc;
                P.o_ns[t] = (int32_t)S.nsc;
            }
        }
        __syncthreads();
    }
}

// Before a refinement: every window's row is the scan's (A, x, alpha_beta of its lin; NaN without a grid result), rounds -1,
// and flag[t] = 1 for the windows to refine (lin >= 0, clr >= min_clr and, under bmx_ctx_refine_at_peaks, an apex of the slot's
// peak call: apex != nullptr).
struct RefineInitParams {
    const double *clr; const int32_t *lin, *nsites;
    const int32_t *apex;
    const double *gA, *gx, *gab;
    int npairs, nab;
    int64_t M;
    double min_clr;
    int32_t *flag;
    double *o_clr, *o_A, *o_x, *o_ab;
    int32_t *o_ns, *o_rounds;
};

__global__ void refine_init_kernel(RefineInitParams Q) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= Q.M) return;
    const int L = Q.lin[t];
    const double clr = Q.clr[t];
    Q.flag[t] = (L >= 0 && clr >= Q.min_clr && (!Q.apex || Q.apex[t])) ? 1 : 0;
    Q.o_clr[t] = clr;
    Q.o_ns[t] = Q.nsites[t];
    Q.o_rounds[t] = -1;
    if (L >= 0) {
        const int p = L % Q.npairs;
        Q.o_A[t] = Q.gA[L / Q.npairs]; Q.o_x[t] = Q.gx[p / Q.nab]; Q.o_ab[t] = Q.gab[p % Q.nab];
    } else {
        Q.o_A[t] = Q.o_x[t] = Q.o_ab[t] = NAN;
    }
}

__global__ void refine_compact_kernel(const int32_t *flag, const int64_t *pre, int64_t M, int32_t *list) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < M && flag[t]) list[pre[t]] = (int32_t)t;
}

// ----------------------------------------------------------------------------- support intervals
// Profile-likelihood support intervals around each refined maximum (bmx_ctx_support; the definition is
// ballermixplus_amd/support.py).  One task per (window, free coordinate k, side): task id (t * 3 + k) * 2 + side, side 0 the
// lower end.  One workgroup of REFINE_THREADS per task, grid-striding over a device-compacted task list, so the six tasks of a
// window run in parallel.  A task is a sequence of nuisance searches -- compass_round, the refinement's own round, over the
// task's free coordinates U.fr (coordinate k held), so a witness's T is bmx_ctx_eval_points' T at its natural values bit for
// bit.  After each round thread 0 folds the round's evaluations into T_best.  Between the searches it runs the walk /
// bisection of support.py: search 0 evaluates T* at the centre (no free coordinate), then each search is one profile P_k(t),
// started at the refined point as compass_start_refined lays it out.  No atomics: a task's result is a function of its
// window alone.
constexpr int SUPPORT_TASKS = 6;                // per window: (k, side)
constexpr int SUPPORT_MAX_WALK = 64;
constexpr int SUPPORT_ND = 11;                  // doubles per task: end, witness[3], witness T, outside[3], outside T, T*, T_best
constexpr int SUPPORT_NI = 3;                   // int32 per task: censored, rounds (-1: not computed), profile evaluations

struct SupportParams {
    RefineParams P;                             // the model, sites, windows and workspace as refine_kernel has them
    const int32_t *list; const int64_t *count;  // the tasks to run
    const double *rA, *rx, *rab;                // the refinement's natural values (the centre)
    double drop, end_tol[3];
    double *o_d; int32_t *o_i;                  // [6 M][SUPPORT_ND], [6 M][SUPPORT_NI]
};

struct SupportTask {
    int k, side, fr[3], stage, walk, censored, evals, rounds, done;
    double h0[3], d, Tstar, L, tbest;
    double in_c[3], in_n[3], in_T, out_c[3], out_n[3], out_T;
};

__global__ __launch_bounds__(REFINE_THREADS) void support_kernel(SupportParams Q) {
    extern __shared__ __attribute__((aligned(16))) double lds_ws[];
    __shared__ RefineState S;
    __shared__ SupportTask U;
    const RefineParams &P = Q.P;
    const int tid = threadIdx.x;
    const CompassWs ws = compass_ws(P, lds_ws);
    const int64_t count = *Q.count;
    for (int64_t w = blockIdx.x; w < count; w += gridDim.x) {
        const int64_t task = Q.list[w];
        const int64_t t = task / SUPPORT_TASKS;
        if (tid == 0) {
            U.k = (int)(task % SUPPORT_TASKS) / 2;
            U.side = (int)(task % 2);
            compass_start_refined(P, S, t, Q.rA, Q.rx, Q.rab, U.h0);
            for (int k = 0; k < 3; ++k) {
                S.h[k] = 0.0;
                U.fr[k] = 0;                // search 0: T* at the centre
            }
            U.d = U.h0[U.k];
            U.stage = 0; U.walk = 0; U.censored = 0; U.evals = 0; U.rounds = 0; U.done = 0;
            U.tbest = -INFINITY;
        }
        compass_begin(P, S, t);
        for (;;) {
            if (compass_round(P, S, U.fr, ws, UnitWeight())) {
                if (tid == 0)
                    for (int e = 0; e < REFINE_EVALS; ++e)
                        if (S.valid[e] && S.T[e] > U.tbest) U.tbest = S.T[e];
                continue;
            }
            // ---- the search has ended: P = S.Tc at S.c.  Walk / bisection (support.py), then the next search or the end
            if (tid == 0) {
                const int k = U.k;
                const double Tr = S.Tc;
                bool bisect = false;
                U.rounds += S.rounds;
                if (U.stage == 0) {
                    U.Tstar = Tr; U.L = Tr - Q.drop;
                    for (int q = 0; q < 3; ++q) { U.in_c[q] = S.c[q]; U.in_n[q] = S.nat[q]; }
                    U.in_T = Tr;
                    U.stage = 1;
                } else {
                    U.evals++;
                    const bool inside = Tr >= U.L;
                    if (inside) {
                        for (int q = 0; q < 3; ++q) { U.in_c[q] = S.c[q]; U.in_n[q] = S.nat[q]; }
                        U.in_T = Tr;
                        if (U.stage == 1) U.d *= 2.0;
                    } else {
                        for (int q = 0; q < 3; ++q) { U.out_c[q] = S.c[q]; U.out_n[q] = S.nat[q]; }
                        U.out_T = Tr;
                        U.stage = 2;
                    }
                    bisect = U.stage == 2;
                }
                double v = 0.0;
                if (!bisect) {
                    v = min(max(U.in_c[k] + (U.side ? U.d : -U.d), P.lo[k]), P.hi[k]);
                    if (U.walk == SUPPORT_MAX_WALK || v == U.in_c[k]) { U.censored = 1; U.done = 1; }
                    U.walk++;
                } else {
                    if (!(fabs(U.out_c[k] - U.in_c[k]) >= Q.end_tol[k])) U.done = 1;
                    v = U.in_c[k] + 0.5 * (U.out_c[k] - U.in_c[k]);
                }
                if (!U.done) {          // P_k(v), warm-started from the inside point with the grid-start steps
                    for (int q = 0; q < 3; ++q) {
                        S.c[q] = U.in_c[q]; S.nat[q] = U.in_n[q];
                        S.h[q] = U.h0[q];
                        U.fr[q] = P.fr[q] && q != k;
                    }
                    S.c[k] = v;
                    S.nat[k] = refine_nat(S, k, v);
                    S.Tc = -INFINITY; S.have_c = 0; S.rounds = 0;
                }
            }
            __syncthreads();
            if (U.done) break;
        }
        if (tid == 0) {
            double *od = Q.o_d + (size_t)task * SUPPORT_ND;
            int32_t *oi = Q.o_i + (size_t)task * SUPPORT_NI;
            od[0] = U.in_n[U.k];
            for (int q = 0; q < 3; ++q) { od[1 + q] = U.in_n[q]; od[5 + q] = U.censored ? NAN : U.out_n[q]; }
            od[4] = U.in_T;
            od[8] = U.censored ? NAN : U.out_T;
            od[9] = U.Tstar;
            od[10] = U.tbest;
            oi[0] = U.censored; oi[1] = U.rounds; oi[2] = U.evals;
        }
        __syncthreads();
    }
}

// Before the support kernel: every task not computed (NaN, rounds -1); flag[task] = 1 for the free coordinates of the windows
// that were refined with a refined CLR >= min_clr.
struct SupportInitParams {
    const double *clr; const int32_t *rounds;     // the refinement
    int fr[3];
    int64_t M;
    double min_clr;
    int32_t *flag;
    double *o_d; int32_t *o_i;
};

__global__ void support_init_kernel(SupportInitParams Q) {
    const int64_t task = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (task >= Q.M * SUPPORT_TASKS) return;
    const int64_t t = task / SUPPORT_TASKS;
    const int k = (int)(task % SUPPORT_TASKS) / 2;
    Q.flag[task] = (Q.rounds[t] >= 0 && Q.clr[t] >= Q.min_clr && Q.fr[k]) ? 1 : 0;
    for (int j = 0; j < SUPPORT_ND; ++j) Q.o_d[task * SUPPORT_ND + j] = NAN;
    Q.o_i[task * SUPPORT_NI] = 0;
    Q.o_i[task * SUPPORT_NI + 1] = -1;
    Q.o_i[task * SUPPORT_NI + 2] = 0;
}

// ----------------------------------------------------------------------------- block bootstrap
// Block bootstrap of each refined maximum (bmx_ctx_boot / bmx_ctx_eval_points_weighted; the definition is
// ballermixplus_amd/boot.py).  One task per (selected window, replicate), window-major: task q * R + r is replicate r of the
// q-th selected window, so the R tasks of a window -- the same site range, the same first-round tables -- are neighbours in
// dispatch order.  One workgroup of REFINE_THREADS per task, grid-striding over the tasks.  A task is one compass search --
// compass_round, the refinement's own round, with the weights of BootWeight -- from the refined point
// (compass_start_refined: support_kernel's centre, the grid start's steps), on
//     T_w = 2 * sum_i w_i log1p(alpha_i R_i),   w_i = boot_weight(key_r, i / B)
// over the sites of T with w_i > 0.  The weight is computed in the loop: the block index advances with the site index
// (i += REFINE_THREADS: b += REFINE_THREADS / B, carrying the remainder) so the loop has no division, and a site of weight
// 0 skips its exp / log1p (a wave skips them where its 64 consecutive sites all have weight 0: whole blocks when B >= 64).
// In place of nSites the sums carry the total weight of the sites inside each A's cut (S.nsc): T_w is -inf when it is 0.
// After a round thread 0 keeps T_w of the start (T_centre) where that round evaluated it.
// No atomics: a task's result is a function of its window and its key alone.
struct BootParams {
    RefineParams P;                             // the model, sites, windows and workspace as refine_kernel has them
    const uint64_t *keys; int R;                // one key per replicate (point evaluation: one key, R = 1)
    int64_t block;
    const int32_t *list; const int64_t *count;  // the selected windows; nullptr: point evaluation of all M at P.pA/px/pab
    const double *rA, *rx, *rab;                // the refinement's natural values (the centre)
    double *o_A, *o_x, *o_ab, *o_T, *o_Tc;      // [n_sel R]; point evaluation: o_T[M]
    int32_t *o_rounds;
    int64_t *o_wsum;                            // point evaluation: [M] (may be nullptr)
};

__global__ __launch_bounds__(REFINE_THREADS) void boot_kernel(BootParams Q) {
    extern __shared__ __attribute__((aligned(16))) double lds_ws[];
    __shared__ RefineState S;
    const RefineParams &P = Q.P;
    const int tid = threadIdx.x;
    const CompassWs ws = compass_ws(P, lds_ws);
    const int64_t count = Q.list ? *Q.count * Q.R : P.M;
    BootWeight wt;
    wt.B = (uint64_t)Q.block;
    wt.qB = REFINE_THREADS / wt.B; wt.rB = REFINE_THREADS % wt.B;
    wt.blk = wt.rem = 0;
    for (int64_t w = blockIdx.x; w < count; w += gridDim.x) {
        const int64_t t = Q.list ? (int64_t)Q.list[w / Q.R] : w;
        wt.key = Q.keys[Q.list ? w % Q.R : 0];
        if (tid == 0) {
            if (Q.list) compass_start_refined(P, S, t, Q.rA, Q.rx, Q.rab, S.h);
            else compass_start_point(P, S, t);
        }
        compass_begin(P, S, t);
        double Tcentre = -INFINITY;         // thread 0: T_w at the start, which the first summing round evaluates
        while (compass_round(P, S, P.fr, ws, wt))
            if (tid == 0 && S.valid[0]) Tcentre = S.T[0];
        if (tid == 0) {
            if (Q.list) {
                Q.o_A[w] = S.nat[0]; Q.o_x[w] = S.nat[1]; Q.o_ab[w] = S.nat[2];
                Q.o_T[w] = S.Tc; Q.o_Tc[w] = Tcentre; Q.o_rounds[w] = S.rounds;
            } else {
                Q.o_T[t] = S.Tc;
                if (Q.o_wsum) Q.o_wsum[t] = S.nsc;
            }
        }
        __syncthreads();
    }
}

// Before the bootstrap: flag[t] = 1 for the windows that were refined with a refined CLR >= min_clr.
__global__ void boot_init_kernel(const double *clr, const int32_t *rounds, int64_t M, double min_clr, int32_t *flag) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < M) flag[t] = (rounds[t] >= 0 && clr[t] >= min_clr) ? 1 : 0;
}

// ----------------------------------------------------------------------------- sandwich (Godambe) pieces of listed windows
// bmx_ctx_sandwich (the definition is ballermixplus_amd/sandwich.py).  Window q of the list is test site tests[q] at the
// caller's point (A, x, alpha_beta)[q]; the host has laid out the five (x, alpha_beta) of the table columns -- the point,
// x - hx, x + hx, alpha_beta / rv, alpha_beta * rv -- so the kernel forms no shifted point itself.  One workgroup of
// REFINE_THREADS per window, grid-striding over the list; the workspace is the compass kernels' (REFINE_TABS columns x rows, row
// list, row map; LDS or slab).  Per window:
//   1. wave 0: window_range at the point's A;
//   2. the rows the range references are marked and compacted in order (own text: compass_round's stays as it is);
//   3. the five columns of those rows by refine_R, ONE inlined call site in the strided loop;
//   4. the block pass over the blocks i / B that meet [a, b).  B < SANDWICH_WAVE_BLOCK: thread tid takes the blocks
//      b0 + tid + REFINE_THREADS k and walks each one's sites in order, adding s s^T to its H partials and, at the block's end,
//      S_b S_b^T to its J partials.  Otherwise wave w takes the blocks b0 + w + REFINE_WAVES k, its lanes stride over the block's
//      sites, and a fixed-order xor butterfly forms S_b in every lane; lane 0 adds S_b S_b^T.  Both add the products through
//      sandwich_outer, so with B = 1 (S_b = s) J is H bit for bit;
//   5. the per-thread partials (T, g[3], H[6], J[6], three counts) are reduced by an xor butterfly in each wave and the four
//      waves as (0 + 1) + (2 + 3).
// No atomics; every order is fixed by the window's range, B and the thread layout: a window's numbers depend on that window,
// its point, B and the steps alone.
constexpr int64_t SANDWICH_WAVE_BLOCK = 64;       // blocks of at least this many sites go to a wave each
constexpr int SANDWICH_VALS = 16;                 // T, g[3], H[6], J[6]

struct SandwichParams {
    RefineParams P;                       // the model, sites, windows and workspace as refine_kernel has them
    const int32_t *tests;                 // [n] the listed windows of this launch
    const double *pA, *px, *pab;          // [n] the points
    const double *pxm, *pxp, *pabm, *pabp;// [n] x - hx, x + hx, alpha_beta / rv, alpha_beta * rv
    int64_t n, B;
    double den_x, den_v;                  // 2 hx and 2 hv: the central differences' denominators
    double *T, *g, *H, *J;                // [n], [n][3], [n][6], [n][6]
    int32_t *ns, *nsk, *nb;               // [n] each
};

// M += v v^T for v = (a, b, c), in the order (uu, ux, uv, xx, xv, vv): the one expression of H's and J's products
__device__ __forceinline__ void sandwich_outer(double *M, double a, double b, double c) {
    M[0] = fma(a, a, M[0]); M[1] = fma(a, b, M[1]); M[2] = fma(a, c, M[2]);
    M[3] = fma(b, b, M[3]); M[4] = fma(b, c, M[4]); M[5] = fma(c, c, M[5]);
}

// Site i of the window: its score s into (su, sx, sv) and log1p(alpha R) into lt.  0: not one of the window's sites; 1: used;
// 2: skipped (D not > 0 or a score not finite)
__device__ __forceinline__ int sandwich_site(const RefineParams &P, const double *tab, int64_t i, double tg, double A, double den_x,
                                             double den_v, double &su, double &sx, double &sv, double &lt) {
    const double gi = P.sites.genpos[i];
    const double z = A * fabs(gi - tg);
    if (!(z <= P.win.zcut) || gi == tg) return 0;
    const int r = P.sites.row[i];
    const size_t rows = (size_t)P.rows;
    const double alpha = exp(-z);
    const double R0 = tab[r];
    const double Rx = (tab[2 * rows + r] - tab[rows + r]) / den_x;
    const double Rv = (tab[4 * rows + r] - tab[3 * rows + r]) / den_v;
    const double aR = alpha * R0;
    const double D = 1.0 + aR;
    su = -z * aR / D; sx = alpha * Rx / D; sv = alpha * Rv / D;
    lt = log1p(aR);
    return (D > 0.0 && isfinite(su) && isfinite(sx) && isfinite(sv)) ? 1 : 2;
}

__global__ __launch_bounds__(REFINE_THREADS) void sandwich_kernel(SandwichParams Q) {
    extern __shared__ __attribute__((aligned(16))) double lds_ws[];
    __shared__ int64_t s_range[2];
    __shared__ double s_px[REFINE_TABS], s_pab[REFINE_TABS];
    __shared__ int s_wtot[REFINE_WAVES];
    __shared__ int s_nused;
    __shared__ double s_red[REFINE_WAVES][SANDWICH_VALS];
    __shared__ int s_redn[REFINE_WAVES][3];
    const RefineParams &P = Q.P;
    const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE;
    const CompassWs ws = compass_ws(P, lds_ws);
    const int64_t B = Q.B;
    const double den_x = Q.den_x, den_v = Q.den_v;
    for (int64_t q = blockIdx.x; q < Q.n; q += gridDim.x) {
        const int64_t t = Q.tests[q];
        const double A = Q.pA[q], tg = P.win.test_gen[t];
        // ---- 1. the site range [a, b) of the point's A; the five (x, alpha_beta) of the columns
        if (wave == 0) {
            const SiteRange R = window_range(P.sites, P.win, t, tg, A);
            if (lane == 0) { s_range[0] = R.a; s_range[1] = R.b; }
        }
        if (tid == 0) {
            s_px[0] = Q.px[q]; s_px[1] = Q.pxm[q]; s_px[2] = Q.pxp[q]; s_px[3] = Q.px[q]; s_px[4] = Q.px[q];
            s_pab[0] = Q.pab[q]; s_pab[1] = Q.pab[q]; s_pab[2] = Q.pab[q]; s_pab[3] = Q.pabm[q]; s_pab[4] = Q.pabp[q];
        }
        for (int r = tid; r < P.rows; r += REFINE_THREADS) ws.map[r] = 0;
        __syncthreads();
        const int64_t a = s_range[0], b = s_range[1];
        // ---- 2. the rows of the range, marked (plain stores of 1) and compacted in ascending order
        for (int64_t i = a + tid; i < b; i += REFINE_THREADS) ws.map[P.sites.row[i]] = 1;
        __syncthreads();
        int base = 0;
        for (int r0 = 0; r0 < P.rows; r0 += REFINE_THREADS) {
            const int r = r0 + tid;
            const bool on = r < P.rows && ws.map[r];
            const unsigned long long m = __ballot(on);
            if (lane == 0) s_wtot[wave] = __popcll(m);
            __syncthreads();
            int off = base;
            for (int w = 0; w < wave; ++w) off += s_wtot[w];
            if (on) ws.list[off + __popcll(m & ((1ull << lane) - 1ull))] = r;
            for (int w = 0; w < REFINE_WAVES; ++w) base += s_wtot[w];
            __syncthreads();
        }
        if (tid == 0) s_nused = base;
        __syncthreads();
        // ---- 3. the five columns of those rows
        {
            const int nu = s_nused;
            for (int it = tid; it < REFINE_TABS * nu; it += REFINE_THREADS) {
                const int k = it / nu, r = ws.list[it % nu];
                ws.tab[(size_t)k * P.rows + r] = refine_R(P, r, s_px[k], s_pab[k]);
            }
        }
        __syncthreads();
        // ---- 4. the block pass: acc = T / 2, g[3], H[6], J[6]; cnt = the window's sites, the skipped ones, the blocks with a used site
        double acc[SANDWICH_VALS];
        int cnt[3] = {0, 0, 0};
        for (int e = 0; e < SANDWICH_VALS; ++e) acc[e] = 0.0;
        if (a < b) {
            const int64_t b0 = a / B, b1 = (b - 1) / B;
            if (B < SANDWICH_WAVE_BLOCK) {
                for (int64_t blk = b0 + tid; blk <= b1; blk += REFINE_THREADS) {
                    const int64_t lo = max(a, blk * B), hi = min(b, (blk + 1) * B);
                    double Su = 0.0, Sx = 0.0, Sv = 0.0;
                    int used = 0;
                    for (int64_t i = lo; i < hi; ++i) {
                        double su, sx, sv, lt;
                        const int kind = sandwich_site(P, ws.tab, i, tg, A, den_x, den_v, su, sx, sv, lt);
                        if (kind == 0) continue;
                        cnt[0]++;
                        if (kind == 2) { cnt[1]++; continue; }
                        acc[0] += lt; acc[1] += su; acc[2] += sx; acc[3] += sv;
                        sandwich_outer(acc + 4, su, sx, sv);
                        Su += su; Sx += sx; Sv += sv;
                        used++;
                    }
                    if (used) { sandwich_outer(acc + 10, Su, Sx, Sv); cnt[2]++; }
                }
            } else {
                for (int64_t blk = b0 + wave; blk <= b1; blk += REFINE_WAVES) {
                    const int64_t lo = max(a, blk * B), hi = min(b, (blk + 1) * B);
                    double Su = 0.0, Sx = 0.0, Sv = 0.0;
                    int used = 0;
                    for (int64_t i = lo + lane; i < hi; i += WAVE) {
                        double su, sx, sv, lt;
                        const int kind = sandwich_site(P, ws.tab, i, tg, A, den_x, den_v, su, sx, sv, lt);
                        if (kind == 0) continue;
                        cnt[0]++;
                        if (kind == 2) { cnt[1]++; continue; }
                        acc[0] += lt; acc[1] += su; acc[2] += sx; acc[3] += sv;
                        sandwich_outer(acc + 4, su, sx, sv);
                        Su += su; Sx += sx; Sv += sv;
                        used++;
                    }
                    for (int off = 1; off < WAVE; off <<= 1) {
                        Su += __shfl_xor(Su, off); Sx += __shfl_xor(Sx, off); Sv += __shfl_xor(Sv, off);
                        used += __shfl_xor(used, off);
                    }
                    if (lane == 0 && used) { sandwich_outer(acc + 10, Su, Sx, Sv); cnt[2]++; }
                }
            }
        }
        // ---- 5. fixed-order reduction across the workgroup
        for (int off = 1; off < WAVE; off <<= 1) {
            for (int e = 0; e < SANDWICH_VALS; ++e) acc[e] += __shfl_xor(acc[e], off);
            for (int k = 0; k < 3; ++k) cnt[k] += __shfl_xor(cnt[k], off);
        }
        if (lane == 0) {
            for (int e = 0; e < SANDWICH_VALS; ++e) s_red[wave][e] = acc[e];
            for (int k = 0; k < 3; ++k) s_redn[wave][k] = cnt[k];
        }
        __syncthreads();
        if (tid < SANDWICH_VALS) {
            const double v = (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]);
            const int nsites = (s_redn[0][0] + s_redn[1][0]) + (s_redn[2][0] + s_redn[3][0]);
            const int nskip = (s_redn[0][1] + s_redn[1][1]) + (s_redn[2][1] + s_redn[3][1]);
            if (tid == 0) Q.T[q] = nsites > nskip ? 2.0 * v : -INFINITY;
            else if (tid < 4) Q.g[q * 3 + (tid - 1)] = v;
            else if (tid < 10) Q.H[q * 6 + (tid - 4)] = v;
            else Q.J[q * 6 + (tid - 10)] = v;
        } else if (tid == SANDWICH_VALS) {
            Q.ns[q] = (s_redn[0][0] + s_redn[1][0]) + (s_redn[2][0] + s_redn[3][0]);
            Q.nsk[q] = (s_redn[0][1] + s_redn[1][1]) + (s_redn[2][1] + s_redn[3][1]);
            Q.nb[q] = (s_redn[0][2] + s_redn[1][2]) + (s_redn[2][2] + s_redn[3][2]);
        }
        __syncthreads();
    }
}

// bmx_ctx_refine_R: the off-grid column of every table row at one (x, alpha_beta), one thread per row
__global__ __launch_bounds__(REFINE_THREADS) void refine_R_kernel(RefineParams P, double x, double ab, double *out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < P.rows) out[r] = refine_R(P, r, x, ab);
}

// ----------------------------------------------------------------------------- resampled sites, position bootstrap
// bmx_ctx_resample_sites / bmx_ctx_locate_* (the definition is ballermixplus_amd/locate.py).  An integer-weighted composite
// likelihood is the plain one of the site array in which site i stands w_i times: the scan kernels run unchanged on the array
// these kernels build from a source slot's sites, with the bootstrap's weights w_i = boot_weight(key, i / B).
//   resample_count_kernel    per tile of RS_TILE consecutive source sites (one workgroup): the sum of its weights
//   prefix_kernel            the exclusive prefix of the tile sums (its last entry: N', the length of the resampled array)
//   resample_expand_kernel   per tile again: the weights once more (integer comparisons: the same), an exclusive scan of them
//                            inside the workgroup, and every site written w_i times from tile prefix + scan on; the copies of
//                            every table row are counted in an LDS histogram per workgroup (tables of up to RS_HIST_MAX rows;
//                            larger ones count with global atomics) that is added to the global counts once per workgroup
// Three launches on one stream, no workgroup waits for another.  A thread takes RS_PER consecutive sites, so the order of the
// sites is kept and a thread's block index advances without a division per site.
constexpr int RS_THREADS = 256;
constexpr int RS_PER = 4;
constexpr int RS_TILE = RS_THREADS * RS_PER;
constexpr int RS_HIST_MAX = 8192;             // rows of a workgroup's LDS histogram (32 KiB)
constexpr int RS_BLOCKS_MAX = 2048;           // workgroups of the expansion (each strides over the tiles)

// the weights of sites i0 .. i0 + RS_PER - 1 (0 past the end of the array); returns their sum
__device__ __forceinline__ int rs_weights(uint64_t key, int64_t B, int64_t N, int64_t i0, int w[RS_PER]) {
    int64_t b = i0 / B, rem = i0 - b * B;
    int wb = boot_weight(key, (uint64_t)b), sum = 0;
#pragma unroll
    for (int k = 0; k < RS_PER; k++) {
        w[k] = i0 + k < N ? wb : 0;
        sum += w[k];
        if (++rem == B) { rem = 0; ++b; wb = boot_weight(key, (uint64_t)b); }
    }
    return sum;
}

// inclusive scan of v over the workgroup's RS_THREADS threads (wave shuffles, then the wave totals through LDS); *total = the sum
__device__ __forceinline__ int rs_block_scan(int v, int *total) {
    __shared__ int wtot[RS_THREADS / WAVE];
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    for (int o = 1; o < WAVE; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    __syncthreads();                          // the previous tile's readers of wtot are done
    if (lane == WAVE - 1) wtot[wv] = v;
    __syncthreads();
    int before = 0, all = 0;
    for (int k = 0; k < RS_THREADS / WAVE; k++) {
        if (k < wv) before += wtot[k];
        all += wtot[k];
    }
    *total = all;
    return v + before;
}

__global__ __launch_bounds__(RS_THREADS) void resample_count_kernel(uint64_t key, int64_t B, int64_t N, int64_t ntiles,
                                                                    int32_t *__restrict__ tile_sum) {
    __shared__ int wsum[RS_THREADS / WAVE];
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int w[RS_PER];
        int s = rs_weights(key, B, N, tile * RS_TILE + (int64_t)threadIdx.x * RS_PER, w);
        for (int o = WAVE / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
        __syncthreads();                      // the previous tile's sum has been read
        if (lane == 0) wsum[wv] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            int total = 0;
            for (int k = 0; k < RS_THREADS / WAVE; k++) total += wsum[k];
            tile_sum[tile] = total;
        }
    }
}

struct ResampleParams {
    uint64_t key;
    int64_t B, N, ntiles, N_out;
    const double *src_gen;
    const void *src_row;
    double *dst_gen;
    void *dst_row;
    const int64_t *tile_pre;                  // [ntiles + 1]
    int32_t *cnt;                             // [rows] copies per table row (zeroed before the launch)
    int rows, use_hist;
};

template <class T>
__global__ __launch_bounds__(RS_THREADS) void resample_expand_kernel(ResampleParams Q) {
    extern __shared__ int rs_hist[];          // [rows] when use_hist
    const T *__restrict__ src_row = (const T *)Q.src_row;
    T *__restrict__ dst_row = (T *)Q.dst_row;
    if (Q.use_hist) {
        for (int r = threadIdx.x; r < Q.rows; r += RS_THREADS) rs_hist[r] = 0;
        __syncthreads();
    }
    for (int64_t tile = blockIdx.x; tile < Q.ntiles; tile += gridDim.x) {
        const int64_t i0 = tile * RS_TILE + (int64_t)threadIdx.x * RS_PER;
        int w[RS_PER], total;
        const int s = rs_weights(Q.key, Q.B, Q.N, i0, w);
        int64_t o = Q.tile_pre[tile] + (rs_block_scan(s, &total) - s);
#pragma unroll
        for (int k = 0; k < RS_PER; k++) {
            if (w[k] == 0) continue;          // (also every index past the end of the source)
            const double g = Q.src_gen[i0 + k];
            const T r = src_row[i0 + k];
            for (int j = 0; j < w[k] && o < Q.N_out; j++, o++) {       // (o < N_out always holds: the prefix is of these weights)
                Q.dst_gen[o] = g;
                dst_row[o] = r;
            }
            if ((int)r < Q.rows) {
                if (Q.use_hist) atomicAdd(&rs_hist[(int)r], w[k]);
                else atomicAdd(&Q.cnt[(int)r], w[k]);
            }
        }
    }
    if (Q.use_hist) {
        __syncthreads();
        for (int r = threadIdx.x; r < Q.rows; r += RS_THREADS)
            if (rs_hist[r]) atomicAdd(&Q.cnt[r], rs_hist[r]);
    }
}

// After a replicate's scan: per peak k (one wave), the row of its range [lo[k], hi[k]] of the slot's test sites with the largest
// CLR among the rows with a grid result (lin >= 0), the earliest such row on ties; -1 (and CLR 0) when no row has one.  Exact FP64
// comparisons; the lanes stride over the range and keep their first best, then a butterfly in which both partners apply the
// same rule.  A row is one wave's alone: no atomics.
constexpr int LOCATE_THREADS = 256;
__global__ __launch_bounds__(LOCATE_THREADS) void locate_reduce_kernel(const double *__restrict__ clr, const int32_t *__restrict__ lin,
                                                                       const int32_t *__restrict__ lo, const int32_t *__restrict__ hi, int K,
                                                                       int32_t *__restrict__ row_out, double *__restrict__ clr_out) {
    const int k = blockIdx.x * (LOCATE_THREADS / WAVE) + threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    if (k >= K) return;
    int32_t best = -1;
    double bv = 0.0;
    for (int64_t t = (int64_t)lo[k] + lane, e = hi[k]; t <= e; t += WAVE) {
        if (lin[t] < 0) continue;
        const double v = clr[t];
        if (best < 0 || v > bv) { best = (int32_t)t; bv = v; }
    }
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        const int32_t ob = __shfl_xor(best, o);
        const double ov = __shfl_xor(bv, o);
        if (ob >= 0 && (best < 0 || ov > bv || (ov == bv && ob < best))) { best = ob; bv = ov; }
    }
    if (lane == 0) { row_out[k] = best; clr_out[k] = best >= 0 ? bv : 0.0; }
}

// ----------------------------------------------------------------------------- planted sites (power analysis)
// bmx_ctx_plant_sites / bmx_ctx_fetch_at (the definition is ballermixplus_amd/power.py).  The composite likelihood is a generative
// model: a site in reach of a planted locus at c (the scan's own predicate, A |g - c| <= zcut and g != c) redraws its derived count
// from m_k = max(0, gw[r] (1 + alpha R[ix][ia][r])), r over the rows of its sample size, alpha = exp(-A |g - c|).  The slot that
// receives the array is then scanned by the unchanged kernels.
//   plant_range_kernel   per centre (one thread): the run of sites that satisfy A |g - c| <= zcut, by two binary searches with
//                        the exact predicate (rounding is monotone, so the run is contiguous and the searches are exact)
//   plant_kernel         workgroups of PLANT_THREADS over (centre, tile of its run), one site per thread: the total of m_k in
//                        ascending k, then the first k whose running sum exceeds u * total, u from the counter-based hash of the
//                        site index.  gw and the (ix, ia) slice of R are staged in LDS while 16 * rows bytes fit PLANT_LDS_BYTES
//                        (lanes of one sample size read one address: a broadcast), and are read through L2 otherwise
//   plant_hist_kernel    the sites per table row of the finished array, counted as resample_expand_kernel counts them
// A site belongs to one centre at most (the host refuses centres closer than twice the reach), so no two threads write one row.
constexpr int PLANT_THREADS = 256;
constexpr int PLANT_LDS_BYTES = 48 << 10;     // gw + R slice staged in LDS up to 3072 table rows
constexpr int PLANT_HIST_BLOCKS_MAX = 1024;

__global__ void plant_range_kernel(const double *__restrict__ g, int64_t N, const double *__restrict__ centre, int K, double A,
                                   double zcut, int32_t *__restrict__ first, int32_t *__restrict__ count) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const double c = centre[k];
    int64_t a = 0, b = N;                     // the first site that is not (below c and out of reach)
    while (a < b) {
        const int64_t mid = (a + b) >> 1;
        const double gm = g[mid];
        if (gm < c && A * fabs(gm - c) > zcut) a = mid + 1; else b = mid;
    }
    const int64_t lo = a;
    b = N;                                    // the first site from there on that is above c and out of reach
    while (a < b) {
        const int64_t mid = (a + b) >> 1;
        const double gm = g[mid];
        if (gm > c && A * fabs(gm - c) > zcut) b = mid; else a = mid + 1;
    }
    first[k] = (int32_t)lo;
    count[k] = (int32_t)(a - lo);
}

struct PlantParams {
    uint64_t key;
    const double *gen;                        // the positions (source and destination hold the same)
    const void *src_row;
    void *dst_row;
    const double *centre;
    const int32_t *first, *count;             // [K]
    int K;
    double A, zcut;
    const double *gw, *R;                     // [rows]: the admissible neutral probabilities, the planted pair's slice of the table
    const int32_t *row_off;                   // [n_sizes + 1]
    int n_sizes, rows;
    unsigned long long *changed;
};

template <class T, bool LDS>
__global__ __launch_bounds__(PLANT_THREADS) void plant_kernel(PlantParams Q) {
    extern __shared__ double plant_tab[];     // LDS: gw[rows], then R[rows]
    if (LDS) {
        for (int r = threadIdx.x; r < Q.rows; r += PLANT_THREADS) {
            plant_tab[r] = Q.gw[r];
            plant_tab[Q.rows + r] = Q.R[r];
        }
        __syncthreads();
    }
    const double *gw = LDS ? plant_tab : Q.gw;
    const double *Rs = LDS ? plant_tab + Q.rows : Q.R;
    const T *__restrict__ src_row = (const T *)Q.src_row;
    T *__restrict__ dst_row = (T *)Q.dst_row;
    for (int k = blockIdx.y; k < Q.K; k += gridDim.y) {
        const int64_t i0 = Q.first[k], n = Q.count[k];
        const double c = Q.centre[k];
        for (int64_t o = (int64_t)blockIdx.x * PLANT_THREADS + threadIdx.x; o < n; o += (int64_t)gridDim.x * PLANT_THREADS) {
            const int64_t i = i0 + o;
            const double g = Q.gen[i];
            const double z = Q.A * fabs(g - c);
            if (!(z <= Q.zcut) || g == c) continue;
            const int r0 = (int)src_row[i];
            if (r0 >= Q.rows) continue;       // (never: set_sites checked every row)
            int ja = 0, jb = Q.n_sizes - 1;   // the size block of the row: the last j with row_off[j] <= r0
            while (ja < jb) {
                const int mid = (ja + jb + 1) >> 1;
                if (Q.row_off[mid] <= r0) ja = mid; else jb = mid - 1;
            }
            const int ra = Q.row_off[ja], rb = Q.row_off[ja + 1];
            const double alpha = exp_neg(z);
            double total = 0.0;
            for (int r = ra; r < rb; r++) {
                double m = gw[r] * (1.0 + alpha * Rs[r]);
                if (!(m > 0.0) || m > DBL_MAX) m = 0.0;       // negative, NaN and infinite terms count as 0
                total += m;
            }
            if (!(total > 0.0) || total > DBL_MAX) continue;  // nothing to draw from: the row stays
            const double u = (double)(bmx_mix64(Q.key ^ bmx_mix64((uint64_t)i)) >> 11) * 0x1p-53;
            const double target = u * total;
            double cum = 0.0;
            int pick = -1, last = -1;
            for (int r = ra; r < rb; r++) {
                double m = gw[r] * (1.0 + alpha * Rs[r]);
                if (!(m > 0.0) || m > DBL_MAX) m = 0.0;
                cum += m;
                if (m > 0.0) last = r;
                if (pick < 0 && cum > target) pick = r;
            }
            if (pick < 0) pick = last;        // rounding left no k above u * total: the last k with m_k > 0
            if (pick != r0) {
                dst_row[i] = (T)pick;
                atomicAdd(Q.changed, 1ull);
            }
        }
    }
}

template <class T>
__global__ __launch_bounds__(RS_THREADS) void plant_hist_kernel(const T *__restrict__ row, int64_t N, int32_t *__restrict__ cnt, int rows,
                                                                int use_hist) {
    extern __shared__ int plant_hist[];       // [rows] when use_hist
    if (use_hist) {
        for (int r = threadIdx.x; r < rows; r += RS_THREADS) plant_hist[r] = 0;
        __syncthreads();
    }
    for (int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x; i < N; i += (int64_t)gridDim.x * RS_THREADS) {
        const int r = (int)row[i];
        if (r < rows) {
            if (use_hist) atomicAdd(&plant_hist[r], 1);
            else atomicAdd(&cnt[r], 1);
        }
    }
    if (use_hist) {
        __syncthreads();
        for (int r = threadIdx.x; r < rows; r += RS_THREADS)
            if (plant_hist[r]) atomicAdd(&cnt[r], plant_hist[r]);
    }
}

// bmx_ctx_fetch_at: the scan's results at a list of test sites (-1: the empty result)
__global__ void fetch_at_kernel(const double *__restrict__ clr, const int32_t *__restrict__ lin, const int32_t *__restrict__ ns,
                                const int32_t *__restrict__ tests, int64_t n, double *__restrict__ o_clr, int32_t *__restrict__ o_lin,
                                int32_t *__restrict__ o_ns) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int32_t t = tests[j];
    o_clr[j] = t < 0 ? 0.0 : clr[t];
    o_lin[j] = t < 0 ? -1 : lin[t];
    o_ns[j] = t < 0 ? 0 : ns[t];
}

// ----------------------------------------------------------------------------- peaks
// Peak calling on a CLR track (bmx_ctx_peaks / bmx_ctx_peaks_track; the definition is ballermixplus_amd/peaks.py): rows
// t = 0 .. M-1 with non-decreasing positions g and values c.  Every comparison is an exact FP64 comparison and the only
// arithmetic is the two subtractions of the radius predicate and the one multiplication of the extent's threshold, so the
// host restatement and these kernels agree exactly.
//   peak_tile_kernel     per tile of PEAK_TILE = 64 consecutive rows (one wave): its maximum and the first row that attains it
//   peak_apex_kernel     per row with c > 0 and c >= min_clr: its index range [lo, hi] by two binary searches on g with the exact
//                        predicate, then "is any row of the range ahead of me" -- (larger c, or equal c and a lower row) -- against
//                        the tile maxima of the tiles wholly inside the range and row by row in the two partial tiles at its ends
//   prefix_kernel + refine_compact_kernel     the apex rows in row order
//   peak_saddle_kernel   per gap between consecutive apexes (one workgroup, grid-stride): the first row of smallest c strictly inside
//   peak_extent_kernel   per apex (one wave): the run of rows with c >= frac * c_apex around it, cut inside the saddles
// Gaps and extents are very uneven in length (a chromosome has long quiet stretches): a workgroup strides over its gap and a
// wave over its extent 64 rows at a time; the imbalance between workgroups is accepted.
constexpr int PEAK_TILE = 64;
constexpr int PEAK_THREADS = 256;             // 4 tiles per workgroup
constexpr int PEAK_LDS_TILES = 1024;          // tile maxima a workgroup stages (12 KiB): 65536 rows around its own

// (value, row): `a` is ahead of `b` when its value is larger, or equal with a lower row
__device__ __forceinline__ bool peak_ahead(double av, int32_t ai, double bv, int32_t bi) { return av > bv || (av == bv && ai < bi); }

__global__ __launch_bounds__(PEAK_THREADS) void peak_tile_kernel(const double *__restrict__ c, int64_t M, double *__restrict__ tmax,
                                                                  int32_t *__restrict__ tfirst) {
    const int64_t t = (int64_t)blockIdx.x * PEAK_THREADS + threadIdx.x;
    double v = t < M ? c[t] : -INFINITY;
    int32_t i = t < M ? (int32_t)t : INT32_MAX;
    for (int off = WAVE / 2; off; off >>= 1) {
        const double ov = __shfl_xor(v, off, WAVE);
        const int32_t oi = __shfl_xor(i, off, WAVE);
        if (peak_ahead(ov, oi, v, i)) { v = ov; i = oi; }
    }
    if ((threadIdx.x & (WAVE - 1)) == 0 && t < M) { tmax[t / PEAK_TILE] = v; tfirst[t / PEAK_TILE] = i; }
}

struct PeakParams {
    const double *g, *c;
    int64_t M;
    double sep, min_clr;
    const double *tmax; const int32_t *tfirst;
    int32_t *flag;
};

__global__ __launch_bounds__(PEAK_THREADS) void peak_apex_kernel(PeakParams Q) {
    __shared__ double s_max[PEAK_LDS_TILES];
    __shared__ int32_t s_first[PEAK_LDS_TILES];
    __shared__ int s_lo, s_hi;
    const int tid = threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x * PEAK_THREADS + tid;
    const int64_t M = Q.M;
    if (tid == 0) { s_lo = INT32_MAX; s_hi = -1; }
    __syncthreads();
    double ct = 0.0;
    bool cand = false;
    if (t < M) {
        ct = Q.c[t];
        cand = ct > 0.0 && ct >= Q.min_clr;
    }
    int64_t lo = t, hi = t;
    int f0 = 0, f1 = -1;            // the tiles wholly inside [lo, hi]
    if (cand) {
        const double gt = Q.g[t];
        int64_t a = 0, b = t;       // lo: the lowest row s <= t with g_t - g_s <= sep (t itself qualifies: sep >= 0)
        while (a < b) {
            const int64_t mid = (a + b) >> 1;
            if (gt - Q.g[mid] <= Q.sep) b = mid; else a = mid + 1;
        }
        lo = a;
        a = t; b = M - 1;           // hi: the highest row s >= t with g_s - g_t <= sep
        while (a < b) {
            const int64_t mid = (a + b + 1) >> 1;
            if (Q.g[mid] - gt <= Q.sep) a = mid; else b = mid - 1;
        }
        hi = a;
        f0 = (int)((lo + PEAK_TILE - 1) / PEAK_TILE);
        f1 = hi == M - 1 ? (int)((M - 1) / PEAK_TILE) : (int)((hi + 1) / PEAK_TILE) - 1;     // the last tile ends at row M - 1
        if (f0 <= f1) { atomicMin(&s_lo, f0); atomicMax(&s_hi, f1); }
    }
    __syncthreads();
    // the tile maxima the workgroup's rows share go through LDS: the tiles its ranges cover, at most PEAK_LDS_TILES of them
    // around its own four; what lies beyond is read from memory
    const bool any = s_hi >= 0;
    const int w0 = any ? max(s_lo, (int)blockIdx.x * (PEAK_THREADS / PEAK_TILE) - PEAK_LDS_TILES / 2) : 0;
    const int w1 = any ? min(s_hi, w0 + PEAK_LDS_TILES - 1) : -1;
    for (int T = w0 + tid; T <= w1; T += PEAK_THREADS) { s_max[T - w0] = Q.tmax[T]; s_first[T - w0] = Q.tfirst[T]; }
    __syncthreads();
    if (t >= M) return;
    int apex = 0;
    if (cand) {
        const int32_t ti = (int32_t)t;
        bool beaten = false;
        // whole tiles, outwards from the row's own: a tile's maximum beats the row unless it is the row itself -- equal
        // values count only from a lower row, which is why the tiles keep the FIRST row of their maximum
        int dn = min(max((int)(t / PEAK_TILE), f0), f1), up = dn + 1;
        while (!beaten && (dn >= f0 || up <= f1)) {
            if (dn >= f0) {
                const bool in = dn >= w0 && dn <= w1;
                beaten = peak_ahead(in ? s_max[dn - w0] : Q.tmax[dn], in ? s_first[dn - w0] : Q.tfirst[dn], ct, ti);
                --dn;
            }
            if (!beaten && up <= f1) {
                const bool in = up >= w0 && up <= w1;
                beaten = peak_ahead(in ? s_max[up - w0] : Q.tmax[up], in ? s_first[up - w0] : Q.tfirst[up], ct, ti);
                ++up;
            }
        }
        // the partial tiles at the two ends (the whole range when it holds no whole tile: fewer than 127 rows)
        const int64_t e0 = f0 <= f1 ? (int64_t)f0 * PEAK_TILE - 1 : hi;
        for (int64_t s = lo; !beaten && s <= e0; ++s) beaten = s != t && peak_ahead(Q.c[s], (int32_t)s, ct, ti);
        if (f0 <= f1)
            for (int64_t s = (int64_t)(f1 + 1) * PEAK_TILE; !beaten && s <= hi; ++s) beaten = s != t && peak_ahead(Q.c[s], (int32_t)s, ct, ti);
        apex = beaten ? 0 : 1;
    }
    Q.flag[t] = apex;
}

// sad[0] = sad[K] = -1; sad[i + 1] = the saddle between apex i and apex i + 1 (-1: adjacent rows)
__global__ __launch_bounds__(PEAK_THREADS) void peak_saddle_kernel(const double *__restrict__ c, const int32_t *__restrict__ row, int64_t K,
                                                                    int32_t *__restrict__ sad) {
    __shared__ double s_v[PEAK_THREADS / WAVE];
    __shared__ int32_t s_i[PEAK_THREADS / WAVE];
    const int tid = threadIdx.x;
    if (blockIdx.x == 0 && tid == 0) { sad[0] = -1; sad[K] = -1; }
    for (int64_t i = blockIdx.x; i + 1 < K; i += gridDim.x) {
        const int64_t a = row[i], b = row[i + 1];
        double v = 0.0;
        int32_t idx = -1;           // -1: no row seen
        for (int64_t s = a + 1 + tid; s < b; s += PEAK_THREADS) {
            const double cs = c[s];
            if (idx < 0 || cs < v) { v = cs; idx = (int32_t)s; }
        }
        for (int off = WAVE / 2; off; off >>= 1) {
            const double ov = __shfl_xor(v, off, WAVE);
            const int32_t oi = __shfl_xor(idx, off, WAVE);
            if (oi >= 0 && (idx < 0 || ov < v || (ov == v && oi < idx))) { v = ov; idx = oi; }
        }
        if ((tid & (WAVE - 1)) == 0) { s_v[tid / WAVE] = v; s_i[tid / WAVE] = idx; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < PEAK_THREADS / WAVE; w++) {
                const double ov = s_v[w];
                const int32_t oi = s_i[w];
                if (oi >= 0 && (idx < 0 || ov < v || (ov == v && oi < idx))) { v = ov; idx = oi; }
            }
            sad[i + 1] = idx;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(PEAK_THREADS) void peak_extent_kernel(const double *__restrict__ c, int64_t M, const int32_t *__restrict__ row,
                                                                    const int32_t *__restrict__ sad, int64_t K, double frac,
                                                                    int32_t *__restrict__ o_lo, int32_t *__restrict__ o_hi) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t i = (int64_t)blockIdx.x * (PEAK_THREADS / WAVE) + threadIdx.x / WAVE;       // wave-uniform
    if (i >= K) return;
    const int64_t a = row[i];
    const double thr = frac * c[a];
    // the region stays strictly inside the saddles; adjacent apexes have none between them and end at their own rows
    const int64_t lim_lo = i == 0 ? 0 : (sad[i] >= 0 ? (int64_t)sad[i] + 1 : (int64_t)row[i - 1] + 1);
    const int64_t lim_hi = i == K - 1 ? M - 1 : (sad[i + 1] >= 0 ? (int64_t)sad[i + 1] - 1 : (int64_t)row[i + 1] - 1);
    int64_t hi = a;
    for (int64_t pos = a + 1;; pos += WAVE) {
        const int64_t s = pos + lane;
        const unsigned long long ok = __ballot(s <= lim_hi && c[s <= lim_hi ? s : a] >= thr);
        if (ok == ~0ULL) { hi = pos + WAVE - 1; continue; }
        hi = pos + __builtin_ctzll(~ok) - 1;
        break;
    }
    int64_t lo = a;
    for (int64_t pos = a - 1;; pos -= WAVE) {
        const int64_t s = pos - lane;
        const unsigned long long ok = __ballot(s >= lim_lo && c[s >= lim_lo ? s : a] >= thr);
        if (ok == ~0ULL) { lo = pos - WAVE + 1; continue; }
        lo = pos - __builtin_ctzll(~ok) + 1;
        break;
    }
    if (lane == 0) { o_lo[i] = (int32_t)lo; o_hi[i] = (int32_t)hi; }
}

// ----------------------------------------------------------------------------- surfaces of a list of test sites
// surface_kernel's T[iA][pair] for a LIST of test sites of the slot in one launch, plain (bmx_ctx_surfaces; the definition and the
// CLI's selection rule are ballermixplus_amd/surfaces.py), given one fitted neighbouring locus per entry (bmx_ctx_cond_surfaces,
// ballermixplus_amd/conditional.py) or against the slot's baseline of accepted loci (bmx_ctx_base_surfaces,
// ballermixplus_amd/stepwise.py).  One body, listed_surface; the three kernels differ in their SIDE alone: where the (d, shared) of
// a staged site comes from.  One workgroup of SURFS_THREADS per (listed entry q, iA, slice of SURFS_THREADS pairs); thread tid owns
// pair p = slice * SURFS_THREADS + tid.
//   1. wave 0 finds the inclusive site range of this A inside the window (window_range: a window at A = 1e8 reads a few dozen
//      positions, not the chromosome); it goes to the workgroup through LDS.
//   2. the range is walked in tiles of SURFS_THREADS sites: tile_site and tile_store put (alpha, row) of site base + tid into LDS.
//      Under a side the same thread takes the site's d and whether it is SHARED from the side and stores u = alpha / (1.0 + d) over
//      alpha and d beside it: the conditioning costs one division per site per tile.  The barriers count the `in` sites (and the
//      shared ones); every thread then adds its term over them IN INCREASING SITE INDEX (same-address LDS reads, R coalesced):
//      tile_term = log1p(alpha R) without a side, log1p(u (R - d)) under one -- a subtract more.
//   The sides:
//      NoSide (surfaces_kernel): nothing of d is compiled -- no second LDS array, no division, no shared count.
//      PairSide (cond_surfaces_kernel): entry q's conditioning locus is test site ctest[q] held at the grid point clin[q] = iA_c *
//        npairs + p_c (either < 0: none).  A site is shared iff it lies inside the conditioning site's clipped window, A_c |g_i - tc|
//        <= zcut and g_i != tc; then d = exp(-zc) R[row_i][p_c] (one exp, one gather), else d = 0.0 exactly.
//      BaselineSide (base_surfaces_kernel): d = the slot's d[i] and shared = cnt[i] > 0, two coalesced loads.
// Bit for bit, by construction and held by the tests:
//   - surfaces_kernel's sum runs over surface_kernel's sites in surface_kernel's order with surface_kernel's expression (the sites
//     outside the range are exactly those it skips): T and nSites are what bmx_ctx_surface returns for the window;
//   - with d = 0.0, u is alpha and R - 0.0 is R: a pair without a conditioning locus, or with one out of reach of every site, and a
//     window against the empty baseline are surfaces_kernel's window;
//   - baseline_add_kernel's first update of a site is exp(-z) R, PairSide's d: a window after ONE baseline_add is
//     cond_surfaces_kernel's pair (window | that locus).
// No atomics: an entry's numbers depend on that entry (and the baseline) alone.
constexpr int SURFS_THREADS = 256;

struct SurfsParams {
    SiteView sites; WindowView win;
    const double *Rt; int NP, npairs, nslices;      // nslices: slices of SURFS_THREADS pairs
    const double *A; int nA;
    const int32_t *tests;                            // the listed test sites of this launch
    double *T;        // [n][nA][npairs]
    int32_t *ns;      // [n][nA]
    int32_t *nsh;     // [n][nA]: the shared sites among ns (written under a side only)
};

// A side: begin() is the workgroup's setup for entry q, site() gives `shared` and d of site i, staged by this thread (row in s_row)
struct NoSide {
    static constexpr bool sided = false;
    struct Locus {};
    __device__ __forceinline__ Locus begin(const SurfsParams &, int64_t) const { return {}; }
};
struct PairSide {
    static constexpr bool sided = true;
    const int32_t *ctest, *clin;                     // the conditioning loci of this launch's entries
    struct Locus { double tc, Ac; int pc; int64_t clo, chi; };
    __device__ __forceinline__ Locus begin(const SurfsParams &S, int64_t q) const {
        const int32_t ct = ctest[q], cl = clin[q];
        Locus L{0.0, 0.0, 0, 0, -1};                 // (no conditioning locus: no site is inside this window)
        if (ct >= 0 && cl >= 0) {
            L.tc = S.win.test_gen[ct]; L.Ac = S.A[cl / S.npairs]; L.pc = cl % S.npairs;
            L.clo = max(S.win.win_lo[ct], (int64_t)0); L.chi = min(S.win.win_hi[ct], S.sites.N - 1);
        }
        return L;
    }
    __device__ __forceinline__ bool site(const SurfsParams &S, const Locus &L, int64_t i, bool in, const int *s_row, double &d) const {
        bool shared = false;
        d = 0.0;
        if (in && i >= L.clo && i <= L.chi) {
            const double g = S.sites.genpos[i], zc = L.Ac * fabs(g - L.tc);
            shared = zc <= S.win.zcut && g != L.tc;
            if (shared) d = exp(-zc) * S.Rt[(size_t)s_row[threadIdx.x] * S.NP + L.pc];
        }
        return shared;
    }
};
struct BaselineSide {
    static constexpr bool sided = true;
    const double *d; const int32_t *cnt;             // the slot's baseline: [N]
    struct Locus {};
    __device__ __forceinline__ Locus begin(const SurfsParams &, int64_t) const { return {}; }
    __device__ __forceinline__ bool site(const SurfsParams &, const Locus &, int64_t i, bool in, const int *, double &d_i) const {
        d_i = in ? d[i] : 0.0;
        return in && cnt[i] > 0;
    }
};

template <class Side>
__device__ __forceinline__ void listed_surface(const SurfsParams &S, const Side &side) {
    __shared__ double s_u[SURFS_THREADS];           // alpha; under a side u = alpha / (1.0 + d)
    __shared__ double s_d[SURFS_THREADS];           // (under a side only: never referenced without one, and then not allocated)
    __shared__ int s_row[SURFS_THREADS];
    __shared__ int64_t s_range[2];
    const int tid = threadIdx.x;
    const int slice = blockIdx.x % S.nslices;
    const int iA = (blockIdx.x / S.nslices) % S.nA;
    const int64_t q = blockIdx.x / S.nslices / S.nA;
    const int p = slice * SURFS_THREADS + tid;
    const bool live = p < S.npairs;                 // (p may lie beyond the padded row of R: an idle thread reads nothing)
    const int64_t t = S.tests[q];
    const double A = S.A[iA], tg = S.win.test_gen[t];
    [[maybe_unused]] const typename Side::Locus locus = side.begin(S, q);
    if (tid < WAVE) {
        const SiteRange R = window_range(S.sites, S.win, t, tg, A);
        if (tid == 0) { s_range[0] = R.a; s_range[1] = R.b - 1; }
    }
    __syncthreads();
    const int64_t rlo = s_range[0], rhi = s_range[1];
    double sum = 0.0, z;
    int ns = 0;
    [[maybe_unused]] int nsh = 0;
    for (int64_t base = rlo; base <= rhi; base += SURFS_THREADS) {
        const int64_t i = base + tid;
        const bool in = tile_site(S.sites.genpos, i, rhi, tg, A, S.win.zcut, z);
        tile_store(S.sites.row, i, in, z, s_u, s_row);
        [[maybe_unused]] bool shared = false;
        if constexpr (Side::sided) {
            double d;
            shared = side.site(S, locus, i, in, s_row, d);
            s_d[tid] = d;
            s_u[tid] = s_u[tid] / (1.0 + d);
        }
        ns += __syncthreads_count(in);
        if constexpr (Side::sided) nsh += __syncthreads_count(shared);
        if (live) {
            const int cnt = (int)min((int64_t)SURFS_THREADS, rhi - base + 1);
            for (int s = 0; s < cnt; ++s) {
                const int r_s = s_row[s];
                if constexpr (Side::sided) {
                    if (r_s >= 0) sum += log1p(s_u[s] * (S.Rt[(size_t)r_s * S.NP + p] - s_d[s]));
                } else {
                    if (r_s >= 0) sum += tile_term(s_u[s], r_s, S.Rt, S.NP, p);
                }
            }
        }
        __syncthreads();
    }
    if (live) S.T[((size_t)q * S.nA + iA) * S.npairs + p] = ns ? 2.0 * sum : NAN;
    if (slice == 0 && tid == 0) {
        S.ns[(size_t)q * S.nA + iA] = ns;
        if constexpr (Side::sided) S.nsh[(size_t)q * S.nA + iA] = nsh;
    }
}

__global__ __launch_bounds__(SURFS_THREADS) void surfaces_kernel(SurfsParams S) { listed_surface(S, NoSide{}); }
__global__ __launch_bounds__(SURFS_THREADS) void cond_surfaces_kernel(SurfsParams S, PairSide side) { listed_surface(S, side); }
__global__ __launch_bounds__(SURFS_THREADS) void base_surfaces_kernel(SurfsParams S, BaselineSide side) { listed_surface(S, side); }

// ------------------------------------------------------------------------------------ a per-site baseline of accepted loci
// bmx_ctx_baseline_* (the definition is ballermixplus_amd/stepwise.py; base_surfaces_kernel above reads it).  The slot keeps d[N]
// and cnt[N]: under the accepted loci site i follows g (1 + d_i), and cnt_i of them reach it.
//   baseline_add_kernel: the locus is test site t held at (A, column p of the table).  Wave 0 of every workgroup finds the locus'
//   site range with window_range (a few dozen probes), then the workgroups stride over the range in tiles of SURFS_THREADS sites,
//   one thread per site: tile_site's predicate, d_i <- d_i + exp(-z) (R[row_i][p] - d_i) -- from d_i = 0.0 that is exp(-z) R bit
//   for bit, cond_surfaces_kernel's d -- and cnt_i + 1.  A site is written by one thread of one workgroup: plain loads and stores.
//   Workgroup 0 also writes out[0..2] = the first and last written site and how many were written, from the range as
//   influence_range_kernel derives its o[2], o[3]: inside [a, b) every site passes the cut, and the sites [ctr, e) at the locus' own
//   position are the only ones left out (first > last: none).
constexpr int BASE_ADD_GRID_MAX = 1024;       // workgroups of a baseline_add launch (they stride over the range)

struct BaseAddParams {
    SiteView sites; WindowView win;
    const double *Rt; int NP;
    int64_t t; double A; int p;                      // the locus: its test site, and the grid point it is held at
    double *d; int32_t *cnt;                         // [N]
    int64_t *out;                                    // [3]: first, last, number written
};

__global__ __launch_bounds__(SURFS_THREADS) void baseline_add_kernel(BaseAddParams S) {
    __shared__ int64_t s_range[2];
    const int tid = threadIdx.x;
    const double A = S.A, tc = S.win.test_gen[S.t];
    if (tid < WAVE) {
        const SiteRange R = window_range(S.sites, S.win, S.t, tc, A);
        if (blockIdx.x == 0) {                       // (workgroup-uniform)
            const int64_t e = wave_first_true(R.ctr, R.b, [&](int64_t i) { return S.sites.genpos[i] > tc; });
            if (tid == 0) {
                S.out[0] = R.a < R.ctr ? R.a : e;
                S.out[1] = e < R.b ? R.b - 1 : R.ctr - 1;
                S.out[2] = (R.b - R.a) - (e - R.ctr);
            }
        }
        if (tid == 0) { s_range[0] = R.a; s_range[1] = R.b - 1; }
    }
    __syncthreads();
    const int64_t rlo = s_range[0], rhi = s_range[1];
    for (int64_t base = rlo + (int64_t)blockIdx.x * SURFS_THREADS; base <= rhi; base += (int64_t)gridDim.x * SURFS_THREADS) {
        const int64_t i = base + tid;
        double z;
        if (tile_site(S.sites.genpos, i, rhi, tc, A, S.win.zcut, z)) {
            const double d = S.d[i];
            S.d[i] = d + exp(-z) * (S.Rt[(size_t)S.sites.row[i] * S.NP + S.p] - d);
            S.cnt[i] = S.cnt[i] + 1;
        }
    }
}

// ----------------------------------------------------------- delete-block jackknife of a list of test sites' grid maxima
// bmx_ctx_influence (the definition is ballermixplus_amd/influence.py).  Per chunk of listed windows four launches on the
// context's stream: surfaces_kernel gives T and ns, influence_range_kernel every (window, A)'s site range,
// influence_argmax_kernel T_max and lin*, and influence_kernel the blocks.
//   influence_kernel: one workgroup of INFL_THREADS per (listed window, run of up to INFL_BLOCKS consecutive blocks of its
//   range); thread tid owns the pairs p = slice * INFL_THREADS + tid.  For every (iA, slice) the run's sites inside that A's
//   range are walked in tiles of INFL_THREADS sites through surfaces_kernel's helpers (tile_site, tile_store, then tile_term over
//   the `in` sites in increasing site index), the sum restarted at every block boundary: S_b has surfaces_kernel's expression by
//   construction and its order, so a block that holds every qualifying site of an A has S_b == S bitwise.  At a boundary the thread
//   forms T - 2 S_b and keeps its running best (value, lin) of that block in its own column of an LDS table; one fixed-order
//   workgroup reduction per block ends the workgroup.
// No atomics.  A block's numbers depend on its window and B alone: a run only decides which workgroup computes them.
constexpr int INFL_THREADS = 256;
constexpr int INFL_BLOCKS = 8;

// The scan's rule on (value, linear index): a candidate must be > 0 (the start is (0, -1)), the larger value wins, on a tie
// the smaller index; every comparison is false for a NaN.  l < 0: no candidate.
__device__ __forceinline__ void infl_take(double &bv, int32_t &bl, double v, int32_t l) {
    if (l >= 0 && (v > bv || (v == bv && bl >= 0 && l < bl))) { bv = v; bl = l; }
}

// The workgroup's best in thread 0's (v, l); every thread calls it.
__device__ __forceinline__ void infl_wg_best(double &v, int32_t &l, double *s_v, int32_t *s_l) {
    const int tid = threadIdx.x;
    for (int off = WAVE / 2; off; off >>= 1) {
        const double ov = __shfl_xor(v, off, WAVE);
        const int32_t ol = __shfl_xor(l, off, WAVE);
        infl_take(v, l, ov, ol);
    }
    if ((tid & (WAVE - 1)) == 0) { s_v[tid / WAVE] = v; s_l[tid / WAVE] = l; }
    __syncthreads();
    if (tid == 0)
        for (int w = 1; w < INFL_THREADS / WAVE; w++) infl_take(v, l, s_v[w], s_l[w]);
    __syncthreads();
}

struct InflRangeParams {
    SiteView sites; WindowView win;
    const double *A; int nA;
    const int32_t *tests; int64_t n;
    int64_t *rng;     // [n][nA][4]: the inclusive range of A (window_range's), the first and last QUALIFYING site (first > last: none)
};

// One wave per (listed window, A): window_range, and the end of the run of sites at the test position.
__global__ __launch_bounds__(INFL_THREADS) void influence_range_kernel(InflRangeParams S) {
    const int64_t w = (int64_t)blockIdx.x * (INFL_THREADS / WAVE) + threadIdx.x / WAVE;        // wave-uniform
    if (w >= S.n * S.nA) return;
    const int64_t t = S.tests[w / S.nA];
    const double A = S.A[w % S.nA], tg = S.win.test_gen[t];
    const SiteRange R = window_range(S.sites, S.win, t, tg, A);
    const int64_t ctr = R.ctr, a = R.a, b = R.b, e = wave_first_true(ctr, b, [&](int64_t i) { return S.sites.genpos[i] > tg; });
    if (threadIdx.x % WAVE == 0) {
        int64_t *o = S.rng + (size_t)w * 4;
        o[0] = a; o[1] = b - 1;
        o[2] = a < ctr ? a : e;                 // the sites [ctr, e) sit at the test position and do not qualify
        o[3] = e < b ? b - 1 : ctr - 1;
    }
}

// T_max and lin* of every window of a chunk: the scan's rule over T[q][lin], lin = iA * npairs + p.
__global__ __launch_bounds__(INFL_THREADS) void influence_argmax_kernel(const double *__restrict__ T, int64_t per, double *__restrict__ tmax,
                                                                         int32_t *__restrict__ lin) {
    __shared__ double s_v[INFL_THREADS / WAVE];
    __shared__ int32_t s_l[INFL_THREADS / WAVE];
    const double *Tq = T + (size_t)blockIdx.x * per;
    double v = 0.0;
    int32_t l = -1;
    for (int64_t i = threadIdx.x; i < per; i += INFL_THREADS) infl_take(v, l, Tq[i], (int32_t)i);
    infl_wg_best(v, l, s_v, s_l);
    if (threadIdx.x == 0) { tmax[blockIdx.x] = v; lin[blockIdx.x] = l; }
}

struct InflItem {
    int64_t b0, out;        // the run's first block, and where its results go in the chunk's per-block arrays
    int32_t q, pad;         // the window's place in the chunk
};

struct InflParams {
    SiteView sites; WindowView win;
    const double *Rt; int NP, npairs, nslices;
    const double *A; int nA, iAmin;
    const int32_t *tests;                               // the chunk's listed test sites
    int64_t B;
    const double *T; const int32_t *ns;                 // the chunk's surfaces: [m][nA][npairs], [m][nA]
    const int64_t *rng;                                 // [m][nA][4]
    const int32_t *lin;                                 // lin*[m]
    const InflItem *items;
    int32_t *m_out; double *contrib; double *L; int32_t *blin;
};

__global__ __launch_bounds__(INFL_THREADS) void influence_kernel(InflParams S) {
    __shared__ double s_alpha[INFL_THREADS];
    __shared__ int s_row[INFL_THREADS];
    __shared__ double s_bv[INFL_BLOCKS][INFL_THREADS];
    __shared__ int32_t s_bl[INFL_BLOCKS][INFL_THREADS];
    __shared__ double s_rv[INFL_THREADS / WAVE];
    __shared__ int32_t s_rl[INFL_THREADS / WAVE];
    const int tid = threadIdx.x;
    const InflItem it = S.items[blockIdx.x];
    const int64_t q = it.q, B = S.B;
    const int64_t *rq = S.rng + (size_t)q * S.nA * 4;
    const int64_t ifirst = rq[S.iAmin * 4 + 2], ilast = rq[S.iAmin * 4 + 3];
    const int nblk = (int)min((int64_t)INFL_BLOCKS, ilast / B - it.b0 + 1);
    const int64_t clo = max(it.b0 * B, ifirst), chi = min((it.b0 + nblk) * B - 1, ilast);      // the run's sites
    const double tg = S.win.test_gen[S.tests[q]];
    const int32_t linstar = S.lin[q];
    for (int k = 0; k < nblk; ++k) { s_bv[k][tid] = 0.0; s_bl[k][tid] = -1; }       // (a thread's own column: no barrier)
    // the thread's best T over the A's whose range the run does not reach: there n_b = 0 for every block of the run, so T itself
    // is a candidate of each of them (the rule is a total order: it may join the blocks' bests at the end)
    double ov = 0.0;
    int32_t ol = -1;
    for (int iA = 0; iA < S.nA; ++iA) {
        const double A = S.A[iA];
        const int nsA = S.ns[q * S.nA + iA];
        const int64_t lo = max(clo, rq[iA * 4]), hi = min(chi, rq[iA * 4 + 1]);
        for (int slice = 0; slice < S.nslices; ++slice) {
            const int p = slice * INFL_THREADS + tid;
            const bool live = p < S.npairs;
            const int pr = live ? p : 0;            // an idle thread follows the wave at pair 0 and keeps nothing
            const int32_t lin = iA * S.npairs + p;
            const double Tp = S.T[((size_t)q * S.nA + iA) * S.npairs + pr];
            if (lo > hi && iA != S.iAmin) {         // wave-uniform; (the run always has a site at A_min, where m_b is counted)
                if (live) {
                    if (lin == linstar)
                        for (int k = 0; k < nblk; ++k) S.contrib[it.out + k] = 2.0 * 0.0;
                    if (nsA > 0) infl_take(ov, ol, Tp, lin);
                }
                continue;
            }
            // block k of the run ends at site kend; (sum, nb) are S_b and n_b of the block being walked
            int k = 0, nb = 0;
            int64_t kend = (it.b0 + 1) * B - 1;
            double sum = 0.0, z;
            auto close = [&]() {
                if (iA == S.iAmin && slice == 0 && tid == 0) S.m_out[it.out + k] = nb;
                if (live) {
                    if (lin == linstar) S.contrib[it.out + k] = 2.0 * sum;
                    if (nsA - nb > 0) {             // the reference skips an A without sites
                        double bv = s_bv[k][tid];
                        int32_t bl = s_bl[k][tid];
                        infl_take(bv, bl, nb ? Tp - 2.0 * sum : Tp, lin);
                        s_bv[k][tid] = bv; s_bl[k][tid] = bl;
                    }
                }
                ++k; kend += B; nb = 0; sum = 0.0;
            };
            for (int64_t base = lo; base <= hi; base += INFL_THREADS) {
                const bool in = tile_site(S.sites.genpos, base + tid, hi, tg, A, S.win.zcut, z);
                tile_store(S.sites.row, base + tid, in, z, s_alpha, s_row);
                __syncthreads();
                const int cnt = (int)min((int64_t)INFL_THREADS, hi - base + 1);
                for (int s = 0; s < cnt; ++s) {
                    while (base + s > kend) close();
                    const int r_s = s_row[s];
                    if (r_s >= 0) {                 // wave-uniform: the one log1p of the kernel
                        sum += tile_term(s_alpha[s], r_s, S.Rt, S.NP, pr);
                        ++nb;
                    }
                }
                __syncthreads();
            }
            while (k < nblk) close();
        }
    }
    for (int k = 0; k < nblk; ++k) {
        double v = s_bv[k][tid];
        int32_t l = s_bl[k][tid];
        infl_take(v, l, ov, ol);
        infl_wg_best(v, l, s_rv, s_rl);
        if (tid == 0) {
            S.L[it.out + k] = v;
            S.blin[it.out + k] = l;
            if (linstar < 0) S.contrib[it.out + k] = NAN;
        }
    }
}

// ------------------------------------------------------------ goodness of fit of a list of test sites: spectrum by distance
// bmx_ctx_fit (the definition is ballermixplus_amd/fit.py; include/bmxscan.h states the entry point).  One workgroup of
// FIT_THREADS per listed window q = (test site, grid point lin).
//   1. prologue: per (size block j, class c), in ascending row order over the block's rows of that class with gw > 0,
//        Gn = sum gw,   Gs = sum gw over the rows with a finite R,   H = sum gw R over the same rows
//      with R the (ix, ia) row of the resident table [pair][rows], then per j their totals over the classes in ascending c (kept
//      at c = F).  m_r = gw (1 + alpha R) is linear in alpha, and with 0 <= gw <= 1 (the host refuses anything else), R >= -1 and
//      1e-8 <= alpha <= 1 it is non-finite exactly where R is, for every site alike: those rows count as 0 in the selected sums
//      and stay in the neutral ones.  The three tables of n_sizes * (F + 1) doubles live in LDS (LDS = true) or in the
//      window's own part of a workspace in device memory.
//   2. wave 0 finds the site range with window_range: the sites are exactly surfaces_kernel's.
//   3. the range is walked in tiles of FIT_THREADS sites: thread tid computes (bin, alpha, size block, own class, tot,
//      neutral total) of site base + tid into LDS (bin -1: not `in` by tile_site; tot = 0: the site is skipped, its tot or its neutral
//      total is not finite and > 0); then thread d * F + c owns cell (d, c) and adds the tile's sites of bin d IN INCREASING SITE
//      INDEX: same-address LDS reads of the site's numbers, neighbouring addresses of the tables across c.
// No atomics: a window's numbers are a function of that window and the per-row arrays alone.
constexpr int FIT_THREADS = 256;

struct FitParams {
    SiteView sites; WindowView win;
    const double *R; int rows, npairs;                  // the table [pair][rows]
    const double *A;
    const int32_t *row_off; int n_sizes;
    const int32_t *tests, *lin;                         // the listed windows of this launch
    const double *gw; const int32_t *cls; int F;
    const double *edges; int D;
    double *ws;                                         // [n][3][n_sizes * (F + 1)] when the tables do not live in LDS
    int32_t *O; double *Esel, *Eneu;                    // [n][D][F]
    int32_t *skipped;                                   // [n]
};

template <bool LDS>
__global__ __launch_bounds__(FIT_THREADS) void fit_kernel(FitParams S) {
    extern __shared__ double fit_tab[];                 // LDS: Gn, Gs, H
    __shared__ double s_edge[BMX_FIT_MAX_CELLS];
    __shared__ double s_alpha[FIT_THREADS], s_tot[FIT_THREADS], s_neu[FIT_THREADS];
    __shared__ int s_bin[FIT_THREADS], s_blk[FIT_THREADS], s_cls[FIT_THREADS];
    __shared__ int64_t s_range[2];
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int F = S.F, D = S.D, W = F + 1, cells = D * F, ntab = S.n_sizes * W;
    const int32_t lin = S.lin[q];
    if (lin < 0) {                                      // workgroup-uniform
        if (tid < cells) {
            S.O[q * cells + tid] = 0;
            S.Esel[q * cells + tid] = NAN;
            S.Eneu[q * cells + tid] = NAN;
        }
        if (tid == 0) S.skipped[q] = 0;
        return;
    }
    double *Gn = LDS ? fit_tab : S.ws + (size_t)q * 3 * ntab;
    double *Gs = Gn + ntab, *H = Gs + ntab;
    const double *Rs = S.R + (size_t)(lin % S.npairs) * S.rows;
    const int64_t t = S.tests[q];
    const double A = S.A[lin / S.npairs], tg = S.win.test_gen[t];
    for (int e = tid; e < S.n_sizes * F; e += FIT_THREADS) {
        const int j = e / F, c = e - j * F;
        double gn = 0.0, gs = 0.0, h = 0.0;
        for (int r = S.row_off[j]; r < S.row_off[j + 1]; ++r) {
            if (S.cls[r] != c) continue;
            const double w = S.gw[r];
            if (!(w > 0.0)) continue;
            gn += w;
            const double Rr = Rs[r];
            if (Rr - Rr == 0.0) { gs += w; h += w * Rr; }
        }
        Gn[j * W + c] = gn; Gs[j * W + c] = gs; H[j * W + c] = h;
    }
    for (int k = tid; k < D - 1; k += FIT_THREADS) s_edge[k] = S.edges[k];
    if (tid < WAVE) {
        const SiteRange R = window_range(S.sites, S.win, t, tg, A);
        if (tid == 0) { s_range[0] = R.a; s_range[1] = R.b - 1; }
    }
    __syncthreads();
    for (int j = tid; j < S.n_sizes; j += FIT_THREADS) {
        double gn = 0.0, gs = 0.0, h = 0.0;
        for (int c = 0; c < F; ++c) { gn += Gn[j * W + c]; gs += Gs[j * W + c]; h += H[j * W + c]; }
        Gn[j * W + F] = gn; Gs[j * W + F] = gs; H[j * W + F] = h;
    }
    __syncthreads();
    const int64_t rlo = s_range[0], rhi = s_range[1];
    const bool cell = tid < cells;
    const int d = tid / F, c = tid - d * F;
    int o = 0, nskip = 0;
    double es = 0.0, en = 0.0, z;
    for (int64_t base = rlo; base <= rhi; base += FIT_THREADS) {
        const bool in = tile_site(S.sites.genpos, base + tid, rhi, tg, A, S.win.zcut, z);
        int bin = -1, j = 0, own = 0;
        double alpha = 0.0, tot = 0.0, neu = 0.0;
        if (in) {
            bin = 0;
            for (int k = 0; k < D - 1; ++k) bin += z > s_edge[k] ? 1 : 0;
            const int r0 = min((int)S.sites.row[base + tid], S.rows - 1);       // (set_sites checked every row)
            int jb = S.n_sizes - 1;                     // the size block of the row: the last j with row_off[j] <= r0
            while (j < jb) {
                const int mid = (j + jb + 1) >> 1;
                if (S.row_off[mid] <= r0) j = mid; else jb = mid - 1;
            }
            own = S.cls[r0];
            alpha = exp(-z);
            tot = Gs[j * W + F] + alpha * H[j * W + F];
            neu = Gn[j * W + F];
            if (!(tot > 0.0 && tot <= DBL_MAX && neu > 0.0 && neu <= DBL_MAX)) tot = 0.0;
        }
        s_bin[tid] = bin; s_blk[tid] = j; s_cls[tid] = own;
        s_alpha[tid] = alpha; s_tot[tid] = tot; s_neu[tid] = neu;
        nskip += __syncthreads_count(in && !(tot > 0.0));
        if (cell) {
            const int cnt = (int)min((int64_t)FIT_THREADS, rhi - base + 1);
            for (int s = 0; s < cnt; ++s) {
                if (s_bin[s] != d) continue;
                o += s_cls[s] == c ? 1 : 0;
                const double tot_s = s_tot[s];
                if (tot_s > 0.0) {
                    const int k = s_blk[s] * W + c;
                    es += (Gs[k] + s_alpha[s] * H[k]) / tot_s;
                    en += Gn[k] / s_neu[s];
                }
            }
        }
        __syncthreads();
    }
    if (cell) {
        S.O[q * cells + tid] = o;
        S.Esel[q * cells + tid] = es;
        S.Eneu[q * cells + tid] = en;
    }
    if (tid == 0) S.skipped[q] = nskip;
}

// Largest double z with exp(-z) >= 1e-8 under correct rounding of exp: bisection on the host.
double compute_zcut() {
    double lo = 18.0, hi = 19.0;
    for (;;) {
        double mid = 0.5 * (lo + hi);
        if (mid == lo || mid == hi) break;
        if (exp(-mid) >= 1e-8) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace

// -DBMX_DEVICE_PROBE=<kernel instantiation>: device code of that ONE kernel and nothing else (register / spill counts and the
// assembly of a kernel under work in seconds instead of a minute; `make probe K='clr_scan_prepared_kernel<16, true>'`).  A kernel
// that is no template is always compiled: the Makefile passes -DBMX_DEVICE_PROBE_PLAIN for it and picks its lines of the report.
#ifdef BMX_DEVICE_PROBE
#ifndef BMX_DEVICE_PROBE_PLAIN
namespace {
template __global__ void BMX_DEVICE_PROBE(ScanParams, PrepView);
}
#endif
#else

// bmx_io.cpp: rows [0, n) formatted into `out` (<= 512 bytes per row); grid indices either as (ix, ia, iA) or as the
// linear index lin = (iA*nx + ix)*nab + ia (< 0: the reference's all-zero row).  Returns the bytes written, 0 on a bad index.
struct bmx_row_tables_;
extern "C" bmx_row_tables_ *bmx_row_tables_new_(const char *xs, int nx, const char *abs_, int nab, const char *As, int nA);
extern "C" void bmx_row_tables_free_(bmx_row_tables_ *t);
extern "C" int bmx_write_chunk_(FILE *f, const bmx_row_tables_ *t, int64_t n, const int64_t *phys, const double *gen, const double *clr,
                                const int32_t *ix, const int32_t *ia, const int32_t *iA, const int32_t *lin, const int32_t *nsites);
// bmx_io.cpp: the threaded host passes of set_sites / set_tests
extern "C" int bmx_validate_sites_(int64_t N, const double *genpos, const int32_t *row, int32_t rows, const double *g,
                                   uint16_t *r16, uint32_t *r32, int64_t *cnt);
extern "C" int bmx_tests_sorted_(int64_t M, const double *test_gen);

// =================================================================================== ctx
namespace {

// Bytes held by every DevBuf / PinnedBuf of the process (bmx_live_bytes)
std::atomic<int64_t> g_device_bytes{0}, g_pinned_bytes{0};

// What owns a device or host resource is never copied: contexts and slots live on the heap
struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};

// Device buffer that owns its allocation and only grows: set_sites / set_tests / surface of a long run (22 chromosomes,
// thousands of surfaces) reuse their allocations instead of paying hipMalloc/hipFree per call.  Whoever holds one frees it
// by going away; release() gives the memory back earlier.  PINNED: the same in pinned host memory.
template <class T, bool PINNED = false>
struct DevBuf : NoCopy {
    T *p = nullptr;
    size_t cap = 0;
    ~DevBuf() { release(); }
    hipError_t ensure(size_t n) {
        if (n <= cap && p) return hipSuccess;
        release();
        const size_t want = std::max<size_t>(n, 1);
        hipError_t e = PINNED ? hipHostMalloc((void **)&p, want * sizeof(T), hipHostMallocDefault) : hipMalloc((void **)&p, want * sizeof(T));
        if (e == hipSuccess) cap = want;
        live() += (int64_t)(cap * sizeof(T));
        return e;
    }
    void release() {
        if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
        live() -= (int64_t)(cap * sizeof(T));
        p = nullptr;
        cap = 0;
    }
    static std::atomic<int64_t> &live() { return PINNED ? g_pinned_bytes : g_device_bytes; }
};
using PinnedBuf = DevBuf<char, true>;   // ensure(bytes)

// Device time of an interval on a stream; ms < 0: none measured yet.  The timer owns its two events, which begin() creates
// on first use.
struct DevTimer : NoCopy {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double ms = -1.0;
    ~DevTimer() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
    hipError_t create() {
        hipError_t e = ev0 ? hipSuccess : hipEventCreate(&ev0);
        if (e == hipSuccess && !ev1) e = hipEventCreate(&ev1);
        return e;
    }
    hipError_t begin(hipStream_t s) {
        const hipError_t e = create();
        return e == hipSuccess ? hipEventRecord(ev0, s) : e;
    }
    hipError_t end(hipStream_t s) { return hipEventRecord(ev1, s); }
    hipError_t read() {         // once the caller has waited for the stream: ms = the interval
        float f = 0.f;
        const hipError_t e = hipEventElapsedTime(&f, ev0, ev1);
        if (e == hipSuccess) ms = (double)f;
        return e;
    }
    int get(double *out, const char *none_yet) const {          // the entry points' *_ms getters
        if (ms < 0) return fail(BMX_E_STATE, none_yet);
        *out = ms;
        return BMX_OK;
    }
};

// fn(t, begin, end) on T host threads over [0, n)
template <class F>
void parallel_ranges(int64_t n, int64_t grain, F fn) {
    unsigned hw = std::thread::hardware_concurrency();
    int T = (int)std::min<int64_t>(std::min<unsigned>(hw ? hw : 1, 32), n / std::max<int64_t>(grain, 1) + 1);
    if (T <= 1) { fn(0, (int64_t)0, n); return; }
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t) th.emplace_back(fn, t, n * t / T, n * (t + 1) / T);
    for (auto &x : th) x.join();
}

}  // namespace

struct ScanPlan;

// One launch range of the prepared pipeline: test sites [off, off + cnt) = groups [g0, g0 + ng), whose blobs take `units`
// 16-byte units of the arena starting at prefix `pbase`.
struct PrepRange {
    int64_t off, cnt, g0, ng, pbase, units;
};

// Everything a launch of the scan needs that does not depend on which test sites it covers.
struct ScanPlan {
    ScanParams P;
    const void *fn = nullptr;
    const void *fn_pl = nullptr;    // the same kernel with the profile likelihoods (nullptr: the plan's kernel has no such form)
    int J = 0, threads = SCAN_THREADS;
    size_t lds_bytes = 0;
    int spb = 0;            // test sites per workgroup
    int64_t range = 0;      // test sites per launch (multiple of spb): bounds the per-slice winner arrays
    bool use_lds = false;
    int mode = 3;           // inner-loop form of the grouped kernel (0..3), 4: prepared pipeline
    // prepared pipeline (mode 4): the per-group kernel's two forms and its launch shape
    const void *prep_count = nullptr, *prep_fill = nullptr;
    size_t prep_lds = 0, prep_lds_count = 0;
    int thr_in_lds = 0, prep_threads = PREP_THREADS;
};

// One chromosome of a context (a "slot"): its site arrays, its test sites, their results and the scan plan made for them.
// A context holds ONE model and any number of slots (bmx_ctx_select_slot); a whole-genome run keeps every chromosome
// resident and scans them back to back on the context's stream.
struct ChromSlot {
    int index = 0;               // the slot's number in its context
    // sites (grow-only buffers)
    bool has_sites = false;
    int64_t N = 0;
    DevBuf<double> genpos, rowmax, rowthr;
    DevBuf<uint16_t> row16;      // one of the two is used
    DevBuf<uint32_t> row32;
    bool wide_rows = false;
    DevBuf<uint8_t> kmom;        // far-field moment slots that pay at each A (set_sites)
    DevBuf<int> d_row_of_slot;
    int row_of_slot[MOM_SLOTS] = {0};
    int nslots = 0;              // rows ranked by frequency: row_of_slot[0 .. nslots)
    int kmom_max = 0;            // the most slots any A uses
    int kmom_max_ser = 0;        // ... in the prepared group kernels' table (second half of kmom)
    // tests
    bool has_tests = false;
    int64_t M = 0;
    DevBuf<double> test_gen;
    DevBuf<int64_t> win_lo, win_hi, center, center_hi;
    bool tests_sorted = false;
    int64_t test_gap = 1 << 30;  // median index gap between neighbouring test sites (strided sample of all of them)
    // results of all test sites
    bool timed = false;          // a scan has been launched since the test sites were set: results / events are valid
    DevBuf<double> clr;
    DevBuf<int32_t> lin, nsites;
    DevBuf<bmx_record> rec;
    DevTimer scan;               // the events around the last scan, created with the slot
    // plan of the scan, made once per (model, sites, tests, variant)
    bool plan_ok = false;
    int plan_variant = -1;
    ScanPlan plan;
    // prepared pipeline: blob sizes per group, their exclusive prefix, launch ranges
    bool prep_ok = false;
    DevBuf<int32_t> blob_units;
    DevBuf<int64_t> blob_prefix;
    std::vector<PrepRange> ranges;
    int plan_pl = 0;             // the context's profile set the plan (its launch ranges) was made for
    // profile likelihoods of the last scan: which ones it computed (BMX_PL_* bits), [M][nA] / [M][nx] / [M][nab] f64
    int pl_have = 0;
    DevBuf<double> pl_out[3];
    uint64_t scan_seq = 0;       // scans launched in this slot (the null's accumulate takes each replicate's scan once)
    // permutation null: the rows given to set_sites while the row arrays hold a permutation of them (bmx_ctx_permute_rows) ...
    bool has_orig = false;
    DevBuf<uint16_t> orig16;
    DevBuf<uint32_t> orig32;
    // ... and the null's state (bmx_ctx_null_begin): observed CLR, exceedance counts, workgroup maxima, replicates so far
    bool null_ok = false;
    uint64_t null_seq = 0;       // scan_seq at null_begin / the last accumulate
    int32_t null_reps = 0;
    DevBuf<double> null_obs, null_part;
    DevBuf<int32_t> null_cnt;
    // refinement of the last scan (bmx_ctx_refine): clr, A, x, alpha_beta, nSites and rounds of every test site
    bool rf_have = false;
    uint64_t rf_seq = 0;         // scan_seq of the scan that was refined
    DevBuf<double> rf_clr, rf_A, rf_x, rf_ab;
    DevBuf<int32_t> rf_ns, rf_rounds;
    // support intervals around the refined maxima (bmx_ctx_support): per task, SUPPORT_ND doubles and SUPPORT_NI int32
    bool sp_have = false;
    DevBuf<double> sp_d;
    DevBuf<int32_t> sp_i;

    // block bootstrap of the refined maxima (bmx_ctx_boot): the selected windows, and per (window, replicate) the final
    // point, T_w there and at the centre, rounds
    bool bt_have = false;
    uint64_t bt_seq = 0;         // scan_seq of the scan whose refinement was bootstrapped
    int64_t bt_nsel = 0;
    int32_t bt_R = 0;
    DevBuf<int32_t> bt_win, bt_rounds;
    DevBuf<double> bt_A, bt_x, bt_ab, bt_T, bt_Tc;

    // peaks of the last peak call on this slot (bmx_ctx_peaks / bmx_ctx_peaks_track): apex flags of the track's pk_M rows, and per
    // apex, in row order, its row, extent and (pk_sad[i], pk_sad[i + 1]) the saddles on either side
    bool pk_have = false;
    bool pk_scan = false;        // the track was the slot's scan (bmx_ctx_peaks), whose scan_seq was ...
    uint64_t pk_seq = 0;
    int64_t pk_M = 0, pk_K = 0;
    DevBuf<int32_t> pk_flag, pk_row, pk_lo, pk_hi, pk_sad;

    // position bootstrap (bmx_ctx_locate_*): the peaks' ranges into this slot's test sites and, per (replicate, peak), the argmax
    // row and its CLR.  Every replicate sets the slot's sites and test sites anew, so this state outlives them: locate_begin
    // starts it, a new model ends it.
    bool lc_ok = false;
    uint64_t lc_seq = 0;         // scan_seq at locate_begin / the last accumulate
    int32_t lc_K = 0, lc_R = 0;
    int64_t lc_M = 0;            // 1 + the highest row any range names
    DevBuf<int32_t> lc_lo, lc_hi, lc_row;
    DevBuf<double> lc_clr;

    // the baseline of accepted loci (bmx_ctx_baseline_*): per site d and the number of loci that reach it.  It belongs to the
    // sites: set_sites, resample_sites and plant_sites drop it.
    bool bl_have = false;
    DevBuf<double> bl_d;
    DevBuf<int32_t> bl_cnt;

    // the row indices: 16-bit unless the table has more than 65535 rows (wide_rows); orig: the given rows while they are permuted
    RowArray row_array() const { return RowArray{wide_rows ? nullptr : row16.p, wide_rows ? row32.p : nullptr}; }
    void *row_ptr() const { return wide_rows ? (void *)row32.p : (void *)row16.p; }
    void *orig_ptr() const { return wide_rows ? (void *)orig32.p : (void *)orig16.p; }
    size_t row_bytes(size_t n) const { return n * (wide_rows ? sizeof(uint32_t) : sizeof(uint16_t)); }
    hipError_t ensure_rows(size_t n, bool wide) {       // room for n of them in a slot without sites, about to receive them
        wide_rows = wide;
        return wide ? row32.ensure(n) : row16.ensure(n);
    }
    // what the entry points ask of the slot before they act (c: its context); each refuses with a message of its own
    bool has_results() const { return has_tests && timed; }
    bool ready_to_scan(const bmx_ctx *c) const;
    bool has_refinement_of_last_scan(const bmx_ctx *c) const;

    void release_peaks() {
        pk_have = false;
        pk_flag.release(); pk_row.release(); pk_lo.release(); pk_hi.release(); pk_sad.release();
    }
    void release_support() {
        sp_have = false;
        sp_d.release(); sp_i.release();
    }
    void release_boot() {
        bt_have = false;
        bt_win.release(); bt_rounds.release(); bt_A.release(); bt_x.release(); bt_ab.release(); bt_T.release(); bt_Tc.release();
    }
    void release_refined() {
        rf_have = false;
        rf_clr.release(); rf_A.release(); rf_x.release(); rf_ab.release(); rf_ns.release(); rf_rounds.release();
        release_support();
        release_boot();
    }
};

struct bmx_ctx {
    int device = 0;
    hipStream_t stream = nullptr, copy_stream = nullptr;
    hipEvent_t ev_done[2] = {nullptr, nullptr}, ev_copied[2] = {nullptr, nullptr};
    int variant = 0;
    // model
    bool has_model = false;
    int stat = 0, min_count = 1, n_sizes = 0, rows = 0, nx = 0, nab = 0, npairs = 0, NP = 0, nslices = 0, nA = 0;
    int renorm_every = 16, span_hi = 1;
    double rmax = 0.0;
    DevBuf<int32_t> d_sizes, d_row_off;
    DevBuf<double> d_g, d_prop, d_x, d_abeta, d_A;
    DevBuf<double> d_psel, d_R, d_Rt;
    std::vector<double> h_A, h_rowmax;   // h_rowmax: [nslices][rows] max |R| (+inf: absent row)
    DevBuf<uint64_t> d_patch_x;
    DevBuf<double> d_patch_y;
    int n_patch = 0;
    std::vector<double> h_g;
    // chromosomes
    std::vector<std::unique_ptr<ChromSlot>> slots;      // slot 0 exists from creation; empty: never selected
    ChromSlot *cur = nullptr;
    int cur_index = 0;
    DevBuf<unsigned long long> d_prof;      // -DBMX_PROFILE / -DBMX_COUNT builds
    // scratch shared by the slots (launches of one context are serialised on its stream)
    DevBuf<double> part_T;       // per-slice winners of one launch range
    DevBuf<int32_t> part_lin, part_ns;
    DevBuf<ScratchEnt> arena;    // prepared pipeline: the blobs of one launch range
    DevBuf<int> d_status;        // ... and its error bits; behind them one range word per slot ([1 + slot index], finalize_kernel)
    DevBuf<double> surf_T;
    DevBuf<int32_t> surf_ns;
    // surfaces of a list of test sites (bmx_ctx_surfaces, _cond_surfaces, _base_surfaces): the list, one chunk's outputs (T and
    // nsites; under a side the shared counts; the maxima and argmaxes when asked for), the events around bmx_ctx_surfaces' chunks
    DevBuf<double> sfs_T, sfs_tmax;
    DevBuf<int32_t> sfs_ns, sfs_list, sfs_nsh, sfs_lin;
    DevTimer sfs;
    // delete-block jackknife (bmx_ctx_influence): the site ranges of the list at A_min and of one chunk at every A, the chunk's
    // runs of blocks, T_max / lin* and per-block outputs, the events around a chunk's kernels; the last call's results on the host
    DevBuf<int64_t> if_rng1, if_rng;
    DevBuf<InflItem> if_items;
    DevBuf<double> if_tmax, if_contrib, if_L;
    DevBuf<int32_t> if_lin, if_m, if_blin;
    DevTimer ifl;
    bool if_have = false;
    std::vector<int64_t> if_first, if_off;
    std::vector<double> if_h_tmax, if_h_contrib, if_h_L;
    std::vector<int32_t> if_h_lin, if_h_ns, if_h_m, if_h_blin;
    // goodness of fit (bmx_ctx_fit): the windows' grid points, the per-row arrays and the bin edges, the workspace of the
    // windows whose prologue sums do not fit LDS, one chunk's outputs, the events around a chunk's kernel
    DevBuf<double> ft_gw, ft_edges, ft_ws, ft_Es, ft_En;
    DevBuf<int32_t> ft_lin, ft_cls, ft_O, ft_skip;
    DevTimer ft;
    // conditional surfaces (bmx_ctx_cond_surfaces): the pairs' conditioning sites and grid points, the events around a chunk's
    // kernels (everything else in the surfaces' buffers)
    DevBuf<int32_t> cs_ctest, cs_clin;
    DevTimer cs;
    // surfaces against a slot's baseline (bmx_ctx_base_surfaces): the events around a chunk's kernels; baseline_add's three numbers
    DevBuf<int64_t> bs_out;
    DevTimer bs;
    // sandwich pieces (bmx_ctx_sandwich): the list, the points with the four shifted arguments of their columns, one chunk's
    // sums and counts, the events around a chunk's kernel; the column of bmx_ctx_refine_R
    DevBuf<int32_t> sw_list, sw_cnt;
    DevBuf<double> sw_pts, sw_out, sw_R;
    DevTimer sw;
    DevBuf<int64_t> gap_sample;
    // profile likelihoods (bmx_ctx_set_profiles): the BMX_PL_* set of later scans, and the keys of one launch range
    int pl_which = 0;
    DevBuf<double> pl_am, pl_pm;
    DevBuf<int32_t> pl_ae, pl_pe;
    // refinement scratch (bmx_ctx_refine / bmx_ctx_eval_points): windows to refine, per-grid-value starts and steps, the
    // per-workgroup workspace of models whose workspace does not fit LDS, points and their results
    DevBuf<int32_t> rf_flag, rf_list, rf_pns;
    DevBuf<int64_t> rf_pre;
    DevBuf<double> rf_grid, rf_pts, rf_pT;
    DevBuf<char> rf_slab;
    DevBuf<uint64_t> bt_keys;    // bootstrap: the replicates' keys, and the weight sums of a weighted point evaluation
    DevBuf<int64_t> bt_pws;
    // peak calling (bmx_ctx_peaks*): the tile maxima, an uploaded track, the events around the last call, and the switch that
    // restricts bmx_ctx_refine to the apexes (bmx_ctx_refine_at_peaks)
    DevBuf<double> pk_tmax, pk_track;
    DevBuf<int32_t> pk_tfirst;
    DevTimer pk;
    bool rf_at_peaks = false;
    // resampled sites (bmx_ctx_resample_sites): the tile sums of the weights, their prefix, the copies per table row
    DevBuf<int32_t> rs_tsum, rs_cnt;
    DevBuf<int64_t> rs_tpre;
    // planted sites (bmx_ctx_plant_sites): the centres and their runs of sites, the admissible neutral probabilities, the number
    // of changed rows, the events around the device work of the last call; bmx_ctx_fetch_at's list and gathered results
    DevBuf<double> pw_centre, pw_gw, fa_clr;
    DevBuf<int32_t> pw_first, pw_count, fa_idx, fa_lin, fa_ns;
    DevBuf<unsigned long long> pw_changed;
    DevTimer pw;
    std::vector<double> h_x, h_ab;
    // pinned host staging of the streaming writer: two slots of (clr, lin, nsites)
    PinnedBuf h_stage[2];
    double zcut = 0;

    // the handles that are no buffers; everything else frees itself
    ~bmx_ctx() {
        for (int k = 0; k < 2; k++) {
            if (ev_done[k]) (void)hipEventDestroy(ev_done[k]);
            if (ev_copied[k]) (void)hipEventDestroy(ev_copied[k]);
        }
        if (stream) (void)hipStreamDestroy(stream);
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
    }
};

inline bool ChromSlot::ready_to_scan(const bmx_ctx *c) const { return c->has_model && has_sites && has_tests; }
inline bool ChromSlot::has_refinement_of_last_scan(const bmx_ctx *c) const {
    return c->has_model && has_results() && rf_have && rf_seq == scan_seq;
}

namespace {

// the model's arrays stay allocated for the next model, like every other buffer of the context
void free_model(bmx_ctx *c) { c->has_model = false; }
// sites / tests: the buffers stay allocated for the next chromosome; only the state is dropped
void drop_tests(ChromSlot *s) {
    s->has_tests = false;
    s->timed = false;       // results belong to the test sites they were computed for
    s->plan_ok = false;
    s->prep_ok = false;
    s->null_ok = false;     // the observed CLR and the counts belong to those test sites
    s->pl_have = 0;         // ... and so do the profiles
    s->release_refined();   // ... and the refinement
    s->pk_have = false;     // ... and the peaks
}
void drop_sites(ChromSlot *s) {
    s->has_sites = false;
    s->has_orig = false;    // new rows: nothing is permuted
    s->bl_have = false;     // ... and the baseline of accepted loci was formed from the old ones
    drop_tests(s);        // test sites were located in the old site array
}

template <class T>
int upload(DevBuf<T> &dst, const T *src, size_t n, hipStream_t s) {
    HIP_TRY(dst.ensure(n));
    if (n) HIP_TRY(hipMemcpyAsync(dst.p, src, n * sizeof(T), hipMemcpyHostToDevice, s));
    return BMX_OK;
}

// n values back to the host, now; a NULL dst is an output the caller did not ask for
template <class T>
hipError_t download(T *dst, const T *src, size_t n) {
    return dst ? hipMemcpy(dst, src, n * sizeof(T), hipMemcpyDeviceToHost) : hipSuccess;
}

// n flags -> their exclusive prefix in c->rf_pre (the count at rf_pre[n]) -> the flagged indices, ascending, in `list`.  Both only
// enqueue on the context's stream: a caller that needs the count on the host reads rf_pre[n] back and waits itself.
hipError_t flag_prefix(bmx_ctx *c, const int32_t *flag, int64_t n) {
    hipLaunchKernelGGL(prefix_kernel, dim3(1), dim3(1024), 0, c->stream, flag, n, c->rf_pre.p);
    return hipGetLastError();
}
hipError_t flag_compact(bmx_ctx *c, const int32_t *flag, int64_t n, int32_t *list) {
    hipLaunchKernelGGL(refine_compact_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, flag, (const int64_t *)c->rf_pre.p, n, list);
    return hipGetLastError();
}

// ---- shared by the entry points over windows listed by test-site index: a slot's sites and windows for their kernels ...
SiteView site_view(const ChromSlot *s) { return SiteView{s->genpos.p, s->row_array(), s->N}; }
WindowView window_view(const bmx_ctx *c, const ChromSlot *s) { return WindowView{s->test_gen.p, s->win_lo.p, s->win_hi.p, c->zcut}; }
// ... what bmx_ctx_surfaces, _influence and _fit refuse before they look at the list's entries, in their common order, `who` in
// front: n < 0, the entry point's own argument refusal (`own`, nullptr: none), the slot's state, with n > 0 a NULL argument ...
int list_ready(bmx_ctx *c, const std::string &who, int64_t n, const char *own, bool null_arg) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    if (n < 0) return fail(BMX_E_INVALID, who + ": n < 0");
    if (own) return fail(BMX_E_INVALID, who + ": " + own);
    if (!c->cur->ready_to_scan(c)) return fail(BMX_E_STATE, "model, sites and tests must be set before " + who);
    if (n > 0 && null_arg) return fail(BMX_E_INVALID, who + ": NULL argument");
    return BMX_OK;
}
// ... and the windows per launch of surfaces_kernel (nsl slices of SURFS_THREADS pairs): their surfaces within BMX_SURFACES_CHUNK_BYTES,
// their workgroups within a launch's 2^32 threads (set_model bounds nA * npairs below 2^31, so one window's always fit)
int64_t surfaces_step(const bmx_ctx *c, int nsl) {
    const int64_t chunk = (int64_t)std::max<size_t>(BMX_SURFACES_CHUNK_BYTES / ((size_t)c->nA * c->npairs * sizeof(double)), 1);
    return std::min(chunk, std::max<int64_t>((0xffffffffLL / SURFS_THREADS) / ((int64_t)c->nA * nsl), 1));
}
// ... what the listed-surface kernels and bmx_ctx_influence's first stage take of the model and the slot (the list, the outputs and
// a side are the caller's) ...
SurfsParams surfs_params(const bmx_ctx *c, const ChromSlot *s, int nsl) {
    SurfsParams S{};
    S.sites = site_view(s); S.win = window_view(c, s);
    S.Rt = c->d_Rt.p; S.NP = c->NP; S.npairs = c->npairs; S.nslices = nsl; S.A = c->d_A.p; S.nA = c->nA;
    return S;
}
// ... and everything bmx_ctx_surfaces, _cond_surfaces and _base_surfaces do with a list of n > 0 entries once their own refusals
// are past: the entries' range, surfaces_step entries per launch on one set of device buffers, per chunk `launch(S, q0, grid)` --
// the call's kernel with its side, on the chunk from entry q0 -- then influence_argmax_kernel when tmax or lin is wanted, the copies
// that were asked for (a NULL output is not copied; without T_out the surfaces never leave the device), and the chunks' kernel
// milliseconds summed into the call's timer.
template <class Launch>
int listed_surfaces(bmx_ctx *c, const std::string &who, int64_t n, const int32_t *tests, DevTimer &timer, Launch launch, double *T_out,
                    int32_t *nsites_out, int32_t *nshared_out, double *tmax_out, int32_t *lin_out) {
    ChromSlot *s = c->cur;
    for (int64_t q = 0; q < n; q++)
        if (tests[q] < 0 || tests[q] >= s->M) return fail(BMX_E_INVALID, who + ": test site index out of range at entry " + std::to_string(q));
    HIP_TRY(hipSetDevice(c->device));
    const size_t per = (size_t)c->nA * c->npairs;              // doubles of one entry's surface
    const int nsl = (c->npairs + SURFS_THREADS - 1) / SURFS_THREADS;
    const int64_t step = surfaces_step(c, nsl);
    const size_t first = (size_t)std::min<int64_t>(step, n);
    HIP_TRY(c->sfs_T.ensure(first * per));
    HIP_TRY(c->sfs_ns.ensure(first * c->nA));
    HIP_TRY(c->sfs_nsh.ensure(first * c->nA));
    HIP_TRY(c->sfs_tmax.ensure(first));
    HIP_TRY(c->sfs_lin.ensure(first));
    int rc;
    if ((rc = upload(c->sfs_list, tests, (size_t)n, c->stream))) return rc;
    SurfsParams S = surfs_params(c, s, nsl);
    S.T = c->sfs_T.p; S.ns = c->sfs_ns.p; S.nsh = c->sfs_nsh.p;
    double total = 0.0;
    for (int64_t q0 = 0; q0 < n; q0 += step) {
        const int64_t m = std::min(step, n - q0);
        S.tests = c->sfs_list.p + q0;
        HIP_TRY(timer.begin(c->stream));
        launch(S, q0, dim3((unsigned)(m * c->nA * nsl)));
        if (tmax_out || lin_out)
            hipLaunchKernelGGL(influence_argmax_kernel, dim3((unsigned)m), dim3(INFL_THREADS), 0, c->stream, (const double *)c->sfs_T.p,
                               (int64_t)per, c->sfs_tmax.p, c->sfs_lin.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(timer.end(c->stream));
        // each chunk goes back before the next is launched: one set of device buffers serves the whole list
        const hipMemcpyKind D2H = hipMemcpyDeviceToHost;
        if (T_out) HIP_TRY(hipMemcpyAsync(T_out + (size_t)q0 * per, c->sfs_T.p, (size_t)m * per * sizeof(double), D2H, c->stream));
        if (nsites_out) HIP_TRY(hipMemcpyAsync(nsites_out + (size_t)q0 * c->nA, c->sfs_ns.p, (size_t)m * c->nA * sizeof(int32_t), D2H, c->stream));
        if (nshared_out) HIP_TRY(hipMemcpyAsync(nshared_out + (size_t)q0 * c->nA, c->sfs_nsh.p, (size_t)m * c->nA * sizeof(int32_t), D2H, c->stream));
        if (tmax_out) HIP_TRY(hipMemcpyAsync(tmax_out + q0, c->sfs_tmax.p, (size_t)m * sizeof(double), D2H, c->stream));
        if (lin_out) HIP_TRY(hipMemcpyAsync(lin_out + q0, c->sfs_lin.p, (size_t)m * sizeof(int32_t), D2H, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(timer.read());
        total += timer.ms;
    }
    timer.ms = total;        // the call's figure: its chunks' kernels
    return BMX_OK;
}

int validate_model(const bmx_model *m) {
    if (!m) return fail(BMX_E_INVALID, "model is NULL");
    if (m->stat < BMX_STAT_B2 || m->stat > BMX_STAT_B1) return fail(BMX_E_INVALID, "unknown statistic id");
    if (m->n_sizes < 1 || !m->sizes || !m->row_off || !m->g || !m->prop)
        return fail(BMX_E_INVALID, "model: sizes/row_off/g/prop must be given");
    if (m->nx < 1 || m->nab < 1 || !m->x || !m->abeta) return fail(BMX_E_INVALID, "model: empty x / alpha_beta grid");
    if (m->min_count < 0) return fail(BMX_E_INVALID, "model: negative min_count");
    if (m->row_off[0] != 0) return fail(BMX_E_INVALID, "model: row_off[0] must be 0");
    for (int j = 0; j < m->n_sizes; j++) {
        int want = m->stat == BMX_STAT_B1 ? 2 : m->sizes[j] + 1;
        if (m->sizes[j] < 1 || m->row_off[j + 1] - m->row_off[j] != want)
            return fail(BMX_E_INVALID, "model: row_off does not match sizes (n+1 rows per size, 2 for B1)");
    }
    if (m->row_off[m->n_sizes] > (1 << 24)) return fail(BMX_E_LIMIT, "model: more than 2^24 LUT rows");
    for (int i = 0; i < m->nx; i++)
        if (!(m->x[i] > 0.0 && m->x[i] < 1.0)) return fail(BMX_E_INVALID, "model: x grid must lie in (0,1)");
    for (int i = 0; i < m->nab; i++)
        if (!(m->abeta[i] > 0.0)) return fail(BMX_E_INVALID, "model: alpha_beta grid must be positive");
    return BMX_OK;
}

constexpr int MAX_SLOTS = 4096;

int ensure_plan(bmx_ctx *c, ChromSlot *s);

int select_slot(bmx_ctx *c, int slot) {
    if (slot < 0 || slot >= MAX_SLOTS) return fail(BMX_E_INVALID, "slot index out of range (0..4095)");
    if ((size_t)slot >= c->slots.size()) c->slots.resize((size_t)slot + 1);
    if (!c->slots[(size_t)slot]) {
        std::unique_ptr<ChromSlot> s(new ChromSlot());
        s->index = slot;
        if (s->scan.create() != hipSuccess) return fail(BMX_E_HIP, "event creation failed");
        c->slots[(size_t)slot] = std::move(s);
    }
    c->cur = c->slots[(size_t)slot].get();
    c->cur_index = slot;
    return BMX_OK;
}

// What set_sites derives from the per-row site counts, the number of sites and the first and last position: the frequency ranking
// of the rows (moment slots), kmom, rowmax and rowthr of slot s, uploaded on the context's stream.  Shared by bmx_ctx_set_sites
// (counts from the host's validation pass) and bmx_ctx_resample_sites (counts from the device); returns with the stream idle.
int derive_row_tables(bmx_ctx *c, ChromSlot *s, const std::vector<int64_t> &cnt, int64_t N, double g_first, double g_last) {
    int rc;
    // Moment slots for the far field: rank the rows by how many sites carry them.
    // Slot s pays at a given A when the ~23 instructions saved per far site of that row outweigh
    // the ~30 instructions its term costs at the end of each zone; the expected number of far sites
    // per zone follows from the mean site density (a performance heuristic only: any choice is exact).
    // The prepared group kernels have a cheaper place than the product for a far site without a slot
    // (series entries, ~11 instructions less than the product): a second table with that gain for them
    // (measured optimum 10-12, flat: profiles/r03_series_entries.txt).
    std::vector<int> order((size_t)c->rows);
    for (int r = 0; r < c->rows; r++) order[(size_t)r] = r;
    const size_t ns = std::min((size_t)MOM_SLOTS, order.size());
    std::partial_sort(order.begin(), order.begin() + ns, order.end(),
                      [&](int a, int b) { return cnt[(size_t)a] != cnt[(size_t)b] ? cnt[(size_t)a] > cnt[(size_t)b] : a < b; });
    std::vector<uint8_t> slot((size_t)c->rows, 255);
    int nslots = 0;
    for (size_t k = 0; k < ns; k++) {
        if (cnt[(size_t)order[k]] == 0) break;
        slot[(size_t)order[k]] = (uint8_t)k;
        s->row_of_slot[k] = order[k];
        nslots = (int)k + 1;
    }
    for (int k = nslots; k < MOM_SLOTS; k++) s->row_of_slot[k] = nslots ? s->row_of_slot[0] : 0;
    s->nslots = nslots;
    const int kcap = diag_env("BMX_MOM_SLOTS") ? std::min(std::max(atoi(diag_env("BMX_MOM_SLOTS")), 0), MOM_SLOTS) : MOM_SLOTS;
    const double range = g_last - g_first;
    std::vector<uint8_t> km(2 * (size_t)c->nA, 0);            // [0, nA): solo / round-2 kernels; [nA, 2 nA): prepared group kernels
    s->kmom_max = 0;
    s->kmom_max_ser = 0;
    for (int t = 0; t < 2; t++) {
        const double gain = diag_env("BMX_KMOM_GAIN") ? atof(diag_env("BMX_KMOM_GAIN")) : t ? 11.0 : 23.0;      // (threshold experiments)
        for (int a = 0; a < c->nA; a++) {
            const double nfar = range > 0 ? 0.8 * (double)(N - 1) / range * c->zcut / c->h_A[(size_t)a] : (double)N;
            int k = 0;
            while (k < nslots && k < kcap && (double)cnt[(size_t)s->row_of_slot[k]] / (double)N * nfar * gain > 30.0) k++;
            km[(size_t)t * c->nA + a] = (uint8_t)k;
            (t ? s->kmom_max_ser : s->kmom_max) = std::max(t ? s->kmom_max_ser : s->kmom_max, k);
        }
    }
    // the kernel reads max |R| and the slot of a row with one load: the slot sits in the low mantissa
    // byte of the (rounded up) maximum; +inf becomes NaN, which never compares as far
    std::vector<double> packed(c->h_rowmax.size());
    // BMX_ROWMAX_GLOBAL (diagnostic builds): one far threshold per row for all slices (its max |R| over the whole grid) -- what a
    // classification shared by the slices would have to use; measures how many more near sites that costs
    std::vector<double> rm_src(c->h_rowmax);
    if (diag_env("BMX_ROWMAX_GLOBAL")) {
        const size_t R_ = (size_t)c->rows, S_ = rm_src.size() / R_;
        for (size_t r = 0; r < R_; r++) {
            double m = 0.0;
            bool nan = false;
            for (size_t sl = 0; sl < S_; sl++) { const double v = rm_src[sl * R_ + r]; if (v != v) nan = true; else m = std::max(m, v); }
            for (size_t sl = 0; sl < S_; sl++) if (!nan) rm_src[sl * R_ + r] = m;
        }
    }
    for (size_t k = 0; k < packed.size(); k++) {
        uint64_t bits;
        memcpy(&bits, &rm_src[k], sizeof bits);
        bits = ((bits & ~0xffull) + 0x100ull) | slot[k % (size_t)c->rows];
        memcpy(&packed[k], &bits, sizeof bits);
    }
    if ((rc = upload(s->rowmax, (const double *)packed.data(), packed.size(), c->stream))) return rc;
    if ((rc = upload(s->kmom, (const uint8_t *)km.data(), km.size(), c->stream))) return rc;
    // prepared pipeline: ONE far threshold per row for all slices, in the exponent domain -- a site of the row at
    // z = A d >= thr has alpha max_grid|R| <= far_eps (log rounded up, the low mantissa byte replaced by the row's slot
    // after rounding up once more).  Rows with max|R| <= far_eps / e are far at any distance (thr = -1); rows absent from
    // the helper file (max|R| = inf) get NaN, which never compares as far.
    const double eps = P_EPS;
    std::vector<double> thr((size_t)c->rows);
    const size_t R_ = (size_t)c->rows, S_ = c->h_rowmax.size() / std::max<size_t>(R_, 1);
    for (size_t r = 0; r < R_; r++) {
        double m = 0.0;
        for (size_t sl = 0; sl < S_; sl++) {
            const double v = c->h_rowmax[sl * R_ + r];
            m = (v != v || m != m) ? NAN : std::max(m, v);
        }
        double t = (m != m) ? INFINITY : (m <= eps * 0.36) ? -1.0 : std::log(m / eps) * (1.0 + 1e-12) + 1e-9;
        if (t < 0.0 && t != -1.0) t = std::max(t, -1.0);
        uint64_t bits;
        memcpy(&bits, &t, sizeof bits);
        if (t > 0.0) bits = ((bits & ~0xffull) + 0x100ull) | slot[r];     // rounds the threshold up; +inf becomes NaN
        else bits = (bits & ~0xffull) | slot[r];                            // negative: far at any distance either way
        memcpy(&thr[r], &bits, sizeof bits);
    }
    if ((rc = upload(s->rowthr, (const double *)thr.data(), thr.size(), c->stream))) return rc;
    if ((rc = upload(s->d_row_of_slot, (const int *)s->row_of_slot, (size_t)MOM_SLOTS, c->stream))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));     // the staging vectors go out of scope here
    return BMX_OK;
}

// A slot that receives sites derived from another slot's on the device (bmx_ctx_resample_sites, bmx_ctx_plant_sites).  The source:
// src_slot checked, src = that slot if it holds sites, else nullptr (which the caller refuses after its own argument checks) ...
int source_slot(bmx_ctx *c, const char *who, int32_t src_slot, ChromSlot *&src) {
    if (src_slot < 0 || src_slot >= MAX_SLOTS) return fail(BMX_E_INVALID, "slot index out of range (0..4095)");
    if (src_slot == c->cur_index) return fail(BMX_E_INVALID, std::string(who) + ": the source slot must not be the selected slot");
    src = (size_t)src_slot < c->slots.size() ? c->slots[(size_t)src_slot].get() : nullptr;
    if (src && !src->has_sites) src = nullptr;
    return BMX_OK;
}
// ... and the end: the n sites are in s->genpos and the slot's row array, their number per table row in c->rs_cnt.  The counts and
// the two end positions come back -- with plant_sites' number of changed rows (c->pw_changed) behind them, on the same wait --
// and everything set_sites derives from them follows on the host.
int finish_derived_sites(bmx_ctx *c, ChromSlot *s, int64_t n, unsigned long long *changed = nullptr) {
    std::vector<int32_t> cnt32((size_t)c->rows);
    double ends[2] = {0.0, 0.0};
    HIP_TRY(hipMemcpyAsync(cnt32.data(), c->rs_cnt.p, cnt32.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&ends[0], s->genpos.p, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&ends[1], s->genpos.p + (n - 1), sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (changed) HIP_TRY(hipMemcpyAsync(changed, c->pw_changed.p, sizeof(*changed), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<int64_t> cnt(cnt32.begin(), cnt32.end());
    int rc;
    if ((rc = derive_row_tables(c, s, cnt, n, ends[0], ends[1]))) return rc;
    s->N = n;
    s->has_sites = true;
    return BMX_OK;
}
}  // namespace

extern "C" {

void bmx_version(int *major, int *minor) {
    if (major) *major = BMX_ABI_VERSION_MAJOR;
    if (minor) *minor = BMX_ABI_VERSION_MINOR;
}

/* A short hash of the kernel source this binary was built from (Makefile: -DBMX_SRC_HASH): the Python shim and the
 * tests compare it with the source in the tree, so that a stale libbmxscan.so cannot be tested or benchmarked. */
#ifndef BMX_SRC_HASH
#define BMX_SRC_HASH "unknown"
#endif
const char *bmx_build_id(void) { return BMX_SRC_HASH; }

const char *bmx_last_error(void) { return g_err.c_str(); }
void bmx_set_error_(const char *msg) { g_err = msg ? msg : ""; }   // for the library's other translation units

int bmx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

double bmx_alpha_cut(void) { return compute_zcut(); }

void bmx_live_bytes(int64_t *device_bytes, int64_t *pinned_bytes) {
    if (device_bytes) *device_bytes = g_device_bytes.load();
    if (pinned_bytes) *pinned_bytes = g_pinned_bytes.load();
}

int bmx_ctx_create(bmx_ctx **out, int device) {
    if (!out) return fail(BMX_E_INVALID, "out is NULL");
    *out = nullptr;
    int n = bmx_device_count();
    if (n <= 0) return fail(BMX_E_NODEVICE, "no HIP device available (libbmxscan has no CPU fallback)");
    if (device < 0 || device >= n) return fail(BMX_E_NODEVICE, "device index out of range");
    TRACE("ctx_create: hipSetDevice(%d)", device);
    HIP_TRY(hipSetDevice(device));
    bmx_ctx *c = new bmx_ctx();
    c->device = device;
    c->zcut = compute_zcut();
    bool ok = hipStreamCreate(&c->stream) == hipSuccess && hipStreamCreate(&c->copy_stream) == hipSuccess;
    for (int k = 0; ok && k < 2; k++)
        ok = hipEventCreateWithFlags(&c->ev_done[k], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&c->ev_copied[k], hipEventDisableTiming) == hipSuccess;
    if (ok) ok = c->d_status.ensure(1 + MAX_SLOTS) == hipSuccess &&
                 hipMemset(c->d_status.p, 0, (1 + MAX_SLOTS) * sizeof(int)) == hipSuccess;
    if (ok) ok = select_slot(c, 0) == BMX_OK;
    if (!ok) {
        bmx_ctx_destroy(c);
        return fail(BMX_E_HIP, "stream/event creation failed");
    }
    TRACE("ctx_create: done");
    *out = c;
    return BMX_OK;
}

void bmx_ctx_destroy(bmx_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    delete c;
}

int bmx_ctx_set_variant(bmx_ctx *c, int variant) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    c->variant = variant;
    return BMX_OK;
}

int bmx_ctx_select_slot(bmx_ctx *c, int32_t slot) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    return select_slot(c, slot);
}

int bmx_ctx_slot_count(bmx_ctx *c) {
    if (!c) return 0;
    return (int)c->slots.size();
}

int bmx_ctx_set_model(bmx_ctx *c, const bmx_model *m, const double *A, int32_t nA) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    int rc = validate_model(m);
    if (rc) return rc;
    if (!A || nA < 1) return fail(BMX_E_INVALID, "empty A grid");
    for (int i = 0; i < nA; i++)
        if (!(A[i] > 0.0)) return fail(BMX_E_INVALID, "A grid must be positive");
    if ((int64_t)nA * m->nx * m->nab > 0x7ffffff0LL) return fail(BMX_E_LIMIT, "grid has more than 2^31 points");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    free_model(c);
    for (const auto &s : c->slots)
        if (s) { drop_sites(s.get()); s->lc_ok = false; }      // row indices and the moment slots belong to the model they were set under
    c->stat = m->stat; c->min_count = m->min_count; c->n_sizes = m->n_sizes;
    c->rows = m->row_off[m->n_sizes]; c->nx = m->nx; c->nab = m->nab; c->nA = nA;
    c->npairs = m->nx * m->nab;
    c->h_g.assign(m->g, m->g + c->rows);
    c->NP = (c->npairs + WAVE - 1) / WAVE * WAVE;
    c->nslices = c->NP / WAVE;
    if ((rc = upload(c->d_sizes, m->sizes, (size_t)m->n_sizes, c->stream))) return rc;
    if ((rc = upload(c->d_row_off, m->row_off, (size_t)m->n_sizes + 1, c->stream))) return rc;
    if ((rc = upload(c->d_g, m->g, (size_t)c->rows, c->stream))) return rc;
    if ((rc = upload(c->d_prop, m->prop, (size_t)m->n_sizes, c->stream))) return rc;
    if ((rc = upload(c->d_x, m->x, (size_t)m->nx, c->stream))) return rc;
    if ((rc = upload(c->d_abeta, m->abeta, (size_t)m->nab, c->stream))) return rc;
    if ((rc = upload(c->d_A, A, (size_t)nA, c->stream))) return rc;
    c->h_A.assign(A, A + nA);
    c->h_x.assign(m->x, m->x + m->nx);
    c->h_ab.assign(m->abeta, m->abeta + m->nab);
    size_t tab = (size_t)c->npairs * c->rows;
    HIP_TRY(c->d_psel.ensure(tab));
    HIP_TRY(c->d_R.ensure(tab));
    HIP_TRY(c->d_Rt.ensure((size_t)c->rows * c->NP));
    HIP_TRY(hipMemsetAsync(c->d_Rt.p, 0, (size_t)c->rows * c->NP * sizeof(double), c->stream));
    // host-libm conformance patch (bmx_math.h): every argument that K1 takes a log of inside lgam's
    // Stirling branch, evaluated with this host's libm and with the device's correctly rounded log
    std::vector<uint64_t> px;
    std::vector<double> py;
    {
        std::unordered_set<uint64_t> seen;        // many (k, n) give the same argument bits: check each once
        auto consider = [&](double v) {
            if (!(v >= 13.0) || !(v < 1e300)) return;     // lgam's log(x) branch starts at 13
            uint64_t vb;
            memcpy(&vb, &v, sizeof(vb));
            if (!seen.insert(vb).second) return;
            const double hl = log(v);
            if (hl != bmx::crlog(v)) {
                uint64_t b;
                memcpy(&b, &v, sizeof(b));
                if (std::find(px.begin(), px.end(), b) == px.end() && px.size() < 4096) { px.push_back(b); py.push_back(hl); }
            }
        };
        int nmax = 0;
        for (int j = 0; j < m->n_sizes; j++) nmax = std::max(nmax, m->sizes[j]);
        for (int ix = 0; ix < m->nx; ix++)
            for (int ia = 0; ia < m->nab; ia++) {
                const double a = m->abeta[ia];
                for (int side = 0; side < 2; side++) {
                    const double xx = side ? 1. - m->x[ix] : m->x[ix];
                    const double b = a / xx - a;
                    consider(a); consider(b); consider(a + b);
                    for (int j = 0; j < m->n_sizes; j++) {
                        const int n = m->sizes[j];
                        for (int k = 0; k <= n; k++) {
                            const double p1 = k + a, q1 = n - k + b;
                            consider(p1); consider(q1); consider(p1 + q1);
                        }
                    }
                }
            }
    }
    c->n_patch = (int)px.size();
    TRACE("set_model: %d libm log exceptions", c->n_patch);
    if (c->n_patch) {
        if ((rc = upload(c->d_patch_x, (const uint64_t *)px.data(), px.size(), c->stream))) return rc;
        if ((rc = upload(c->d_patch_y, (const double *)py.data(), py.size(), c->stream))) return rc;
    }
    LutParams P;
    P.patch = bmx::LogPatch{c->d_patch_x.p, c->d_patch_y.p, c->n_patch};
    P.stat = c->stat; P.min_count = c->min_count; P.n_sizes = c->n_sizes; P.rows = c->rows;
    P.nx = c->nx; P.nab = c->nab; P.NP = c->NP;
    P.sizes = c->d_sizes.p; P.row_off = c->d_row_off.p; P.g = c->d_g.p; P.prop = c->d_prop.p;
    P.x = c->d_x.p; P.abeta = c->d_abeta.p; P.psel = c->d_psel.p; P.R = c->d_R.p; P.Rt = c->d_Rt.p;
    int threads = 128;
    int blocks = (int)((tab + threads - 1) / threads);
    TRACE("set_model: launching bb_lut_kernel, %d blocks x %d, rows=%d pairs=%d", blocks, threads, c->rows, c->npairs);
    hipLaunchKernelGGL(bb_lut_kernel, dim3(blocks), dim3(threads), 0, c->stream, P);
    HIP_TRY(hipGetLastError());
    // How many sites may be multiplied between exponent extractions: every factor
    // 1 + alpha*R lies in [min(1, 1+Rmin), max(1, 1+Rmax)]; keep the product inside 2^+-1000.
    std::vector<double> hR(tab);
    HIP_TRY(hipMemcpyAsync(hR.data(), c->d_R.p, tab * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    TRACE("set_model: table built");
    double fmax = 1.0, fmin = 1.0;
    for (size_t i = 0; i < tab; i++) {
        double v = hR[i];
        if (v != v) continue;  // rows absent from the helper file
        double f = 1.0 + v;
        fmax = std::max(fmax, f);
        if (f > 0.0) fmin = std::min(fmin, f);
    }
    if (!(fmax < 1e300)) return fail(BMX_E_INVALID, "selection table overflows (a neutral probability g is 0 or tiny)");
    c->span_hi = std::max(1, (int)std::ceil(std::log2(fmax)));
    // no kernel multiplies fewer than four factors between two exponent extractions (the per-site kernel always four; the solo
    // kernel eight of the most frequent row, split four + four once renorm_every < 8): 4 x 240 bits on a mantissa below 2
    if (c->span_hi > 240)
        return fail(BMX_E_LIMIT, "selection table spans more than 2^240 (a neutral probability of ~1e-70?)");
    c->rmax = fmax - 1.0;
    {   // per slice and row: the largest |R| over the slice's pairs (grouped kernel's far-field test)
        std::vector<double> rm((size_t)c->nslices * c->rows, 0.0);
        for (int p = 0; p < c->npairs; p++)
            for (int r = 0; r < c->rows; r++) {
                const double v = std::fabs(hR[(size_t)p * c->rows + r]);
                double &m = rm[(size_t)(p / WAVE) * c->rows + r];
                m = (v != v) ? INFINITY : std::max(m, v);
            }
        c->h_rowmax.swap(rm);                 // uploaded by set_sites, with the rows' moment slots packed in
    }
    // per-site kernel: worst case per factor is max(span_hi, 54 bits for 1 - alpha) -- see the kernel
    c->renorm_every = std::max(1, std::min(16, 1000 / std::max(c->span_hi, 54)));
    c->has_model = true;
    return BMX_OK;
}

int bmx_ctx_set_sites(bmx_ctx *c, int64_t N, const double *genpos, const int32_t *row) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    if (!c->has_model) return fail(BMX_E_STATE, "set_model must precede set_sites");
    if (N < 1 || !genpos || !row) return fail(BMX_E_INVALID, "empty site arrays");
    if (N >= 0x7fffffffLL) return fail(BMX_E_LIMIT, "more than 2^31 sites in one array (scan chromosomes one at a time)");
    ChromSlot *s = c->cur;
    // One pass on the host's cores: every row index inside the table and on a (k, n) with a positive neutral probability
    // (the kernels index the LDS/L2 table with it unchecked), positions sorted and not NaN; 16-bit row indices and the
    // per-row site counts (moment slots) come out of the same pass.
    const bool wide = c->rows > 65535;
    std::vector<uint16_t> r16(wide ? 0 : (size_t)N);
    std::vector<uint32_t> r32(wide ? (size_t)N : 0);
    std::vector<int64_t> cnt((size_t)c->rows, 0);
    switch (bmx_validate_sites_(N, genpos, row, c->rows, c->h_g.data(), wide ? nullptr : r16.data(), wide ? r32.data() : nullptr, cnt.data())) {
        case 1: return fail(BMX_E_INVALID, "site row index outside the LUT");
        case 2: return fail(BMX_E_INVALID, "a site has a (count, sample size) whose neutral probability is missing or not positive");
        case 3: return fail(BMX_E_INVALID, "genetic positions must be non-decreasing");
        case 4: return fail(BMX_E_INVALID, "NaN genetic position");
        default: break;
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    drop_sites(s);
    int rc;
    if ((rc = upload(s->genpos, genpos, (size_t)N, c->stream))) return rc;
    if (wide) {
        if ((rc = upload(s->row32, (const uint32_t *)r32.data(), (size_t)N, c->stream))) return rc;
    } else {
        if ((rc = upload(s->row16, (const uint16_t *)r16.data(), (size_t)N, c->stream))) return rc;
    }
    s->wide_rows = wide;
    if ((rc = derive_row_tables(c, s, cnt, N, genpos[0], genpos[N - 1]))) return rc;
    s->N = N;
    s->has_sites = true;
    return BMX_OK;
}

int bmx_ctx_set_tests(bmx_ctx *c, int64_t M, const double *test_gen, const int64_t *win_lo,
                      const int64_t *win_hi) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->has_sites) return fail(BMX_E_STATE, "set_sites must precede set_tests");
    if (M < 1 || !test_gen) return fail(BMX_E_INVALID, "empty test-site arrays");
    if ((win_lo == nullptr) != (win_hi == nullptr)) return fail(BMX_E_INVALID, "window bounds: both arrays or neither (neither = all sites)");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    drop_tests(s);
    int rc;
    if ((rc = upload(s->test_gen, test_gen, (size_t)M, c->stream))) return rc;
    if (win_lo) {
        if ((rc = upload(s->win_lo, win_lo, (size_t)M, c->stream))) return rc;
        if ((rc = upload(s->win_hi, win_hi, (size_t)M, c->stream))) return rc;
    } else {        // the reference's default mode (v1:598-610): every window holds all sites -- nothing to copy
        HIP_TRY(s->win_lo.ensure((size_t)M));
        HIP_TRY(s->win_hi.ensure((size_t)M));
        hipLaunchKernelGGL(all_sites_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, c->stream, s->win_lo.p, s->win_hi.p, M, s->N);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(s->center.ensure((size_t)M));
    HIP_TRY(s->center_hi.ensure((size_t)M));
    HIP_TRY(s->clr.ensure((size_t)M));
    HIP_TRY(s->lin.ensure((size_t)M));
    HIP_TRY(s->nsites.ensure((size_t)M));
    HIP_TRY(s->rec.ensure((size_t)M));
    int threads = 256;
    hipLaunchKernelGGL(locate_kernel, dim3((unsigned)((M + threads - 1) / threads)), dim3(threads), 0, c->stream,
                       s->genpos.p, s->N, s->test_gen.p, M, s->center.p, s->center_hi.p);
    HIP_TRY(hipGetLastError());
    // test-site density: the median index gap between neighbouring test sites over a strided sample of ALL of them (decides
    // grouped vs per-site kernel and the group size; a chromosome whose head differs from its body is judged by its body)
    const int64_t ns = std::min<int64_t>(M - 1, 65536);
    if (ns > 0) {
        HIP_TRY(c->gap_sample.ensure((size_t)ns));
        hipLaunchKernelGGL(gap_kernel, dim3((unsigned)((ns + threads - 1) / threads)), dim3(threads), 0, c->stream,
                           s->center.p, (M - 1) / ns, ns, c->gap_sample.p);
        HIP_TRY(hipGetLastError());
    }
    // while the device locates the test sites: the grouped kernels need ascending test positions
    s->tests_sorted = bmx_tests_sorted_(M, test_gen) != 0;
    s->test_gap = 1 << 30;
    if (ns > 0) {
        std::vector<int64_t> gaps((size_t)ns);
        HIP_TRY(hipMemcpyAsync(gaps.data(), c->gap_sample.p, (size_t)ns * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        std::nth_element(gaps.begin(), gaps.begin() + gaps.size() / 2, gaps.end());
        s->test_gap = gaps[gaps.size() / 2];
    } else {
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    s->M = M;
    s->has_tests = true;
    // the plan of the scan, and for the prepared pipeline the sizes of its per-group blobs (a counting pass on the device),
    // are part of setting the test sites: bmx_ctx_scan itself only launches
    return ensure_plan(c, s);
}

}  // extern "C"

namespace {

// the dynamic-LDS limit of a kernel is set per FUNCTION and launches read it: attribute + launch pairs of different contexts
// (threads of bmx_scan_multi, a caller's own threads) must not interleave
std::mutex g_launch_mu;

// Profile likelihoods' scratch: keys of one launch range, per test site
constexpr int64_t PL_SCRATCH_BYTES = (int64_t)1 << 30;
int64_t pl_bytes_per_test(const bmx_ctx *c, int which) {
    int64_t b = 0;
    if (which & BMX_PL_A) b += 12 * (int64_t)c->nslices * c->nA;
    if (which & (BMX_PL_X | BMX_PL_ABETA)) b += 12 * (int64_t)c->NP;
    return b;
}

int plan_scan(bmx_ctx *c, ChromSlot *s, ScanPlan &pl) {
    ScanParams &P = pl.P;
    P.genpos = s->genpos.p; P.row = s->row_array(); P.N = s->N; P.Rt = c->d_Rt.p;
    P.rows = c->rows; P.NP = c->NP; P.npairs = c->npairs; P.nslices = c->nslices;
    P.A = c->d_A.p; P.nA = c->nA; P.zcut = c->zcut; P.renorm_every = c->renorm_every; P.span_hi = c->span_hi; P.rmax = c->rmax;
    {
        // 8th order: economised coefficients, valid on [-0.05, 0.05] (FAR_W); lower orders: Taylor, cut at ~6e-15
        const double eps_default = FAR_ORDER >= 8 ? 0.05 : FAR_ORDER >= 6 ? 0.0105 : 0.0016;
        double eps = diag_env("BMX_FAR_EPS") ? atof(diag_env("BMX_FAR_EPS")) : eps_default;   // accuracy experiments
        eps = std::min(std::max(eps, 0.0), FAR_ORDER >= 8 ? 0.05 : 0.035);
        P.far_eps = eps;
        P.rowmax = s->rowmax.p;
        P.kmom = s->kmom.p;
        P.prof = nullptr;
#if defined(BMX_PROFILE) || defined(BMX_COUNT)
        if (!c->d_prof.p) { HIP_TRY(c->d_prof.ensure(32)); HIP_TRY(hipMemset(c->d_prof.p, 0, 32 * sizeof(unsigned long long))); }
        P.prof = c->d_prof.p;
#endif
        for (int k = 0; k < MOM_SLOTS; k++) P.row_of_slot[k] = s->row_of_slot[k];
        P.far_bits = (float)(eps * 1.4427 * 1.03);      // |log1p(x)| <= 1.027 |x| for |x| <= 0.05
    }
    size_t lds = (size_t)c->rows * WAVE * sizeof(double);
    if (const char *pad = diag_env("BMX_LDS_PAD")) lds += (size_t)std::max(atoi(pad), 0);   // occupancy experiments
    P.row0 = s->nslots > 0 ? s->row_of_slot[0] : -1;
    P.wide_tab = (size_t)c->rows * c->NP * sizeof(double) >= ((size_t)1 << 32) ? 1 : 0;
    // Grouping pays while neighbouring test sites share most of their windows.  Measured on config 3 in round 3 with the
    // prepared kernels (windows/s x1000 for J = 16 / 8 / 4 / one test site per wave; profiles/r03_stride_table.txt): stride 1:
    // 4175/-/-/-, 2: 3133/2860/1774/1339, 4: -/2433/1677/1343, 6: -/2058/1543/1342, 8: -/1741/1474/1337, 12: -/1354/1298/1333,
    // 16: -/1157/1158/1322, 24: -/916/957/1314, 32: -/772/836/1301, 48: -/585/687/1282, 64+: 1268 ... 1174 at 200
    // -> J = 16 up to a median gap of 3 sites between test sites, 8 up to 12 (round 4: up to 9, the solo pipeline having gained 15 %),
    //    beyond that one test site per wave.
    // (The round-2 kernels, variant 12, keep their own thresholds: 16 / 8 / 4 up to 3 / 28 / 56, then the per-site kernel.)
    const int64_t gap_max = diag_env("BMX_DENSE_GAP") ? atoll(diag_env("BMX_DENSE_GAP")) : 56;
    const bool can_group = s->tests_sorted && s->test_gap <= gap_max && c->span_hi <= 62 && s->N < 0x7fffffffLL && c->nA < 8191 && !P.wide_tab;
    int J = 0;
    // variants: 0 -> prepared pipeline (round 3: per-group work done once by prep_kernel), J by test-site gap;
    //           13 / 14 / 15 -> prepared, J = 16 / 8 / 4;
    //           12 -> the round-2 grouped kernel, J by test-site gap (pairs near / quads mid / power sums far);
    //           3 -> J=8, 4 -> J=4 (same form); 10/11 -> J=16/8 without the power sums (exact products);
    //           8/9 -> J=16/8 pairs only; 5/6/7 -> J=16/8/4 readlane single-site loop; 1, 2 -> per-site kernel
    const int v = c->variant;
    const bool prep_ok = !diag_env("BMX_FAR_EPS");
    // one test site per wave, prepared (mode 5): sparse or unsorted test sites (variant 0), or on request (variant 16)
    const int64_t solo_gap = diag_env("BMX_SOLO_GAP") ? atoll(diag_env("BMX_SOLO_GAP")) : SOLO_GAP;
    const bool solo = prep_ok && !P.wide_tab && s->N < 0x7fffffffLL && (v == 16 || (v == 0 && (!can_group || s->test_gap > solo_gap)));
    const bool prepared = !solo && can_group && (v == 0 || (v >= 13 && v <= 15)) && prep_ok;
    if (can_group && !solo) {
        J = (v == 0 || v == 12 || v == 5 || v == 8 || v == 10 || v == 13) ? 16 : (v == 3 || v == 6 || v == 9 || v == 11 || v == 14) ? 8
            : (v == 4 || v == 7 || v == 15) ? 4 : 0;
        if (v == 12) J = s->test_gap <= 3 ? 16 : s->test_gap <= 28 ? 8 : 4;
        if (v == 0) J = s->test_gap <= 3 ? 16 : 8;                  // (gaps beyond SOLO_GAP never get here: solo)
        if ((v == 0 || v == 12) && diag_env("BMX_FORCE_J")) {                    // threshold experiments: 16, 8 or 4
            const int fj = atoi(diag_env("BMX_FORCE_J"));
            if (fj != 16 && fj != 8 && fj != 4) return fail(BMX_E_INVALID, "BMX_FORCE_J must be 16, 8 or 4");
            J = fj;
        }
    }
    // LDS: the prepared kernel keeps per wave a ring of the blob stream and 512 B of scratch, the round-2 grouped kernel a
    // scratch list and the moments; both the sites between the test sites; the slice's per-row max |R| only the latter
    int mom_slots = MOM_SLOTS_LDS;
    auto wave_bytes = [&](int slots) {
        if (solo) return (size_t)(RING_UNITS + RING_MIRROR) * sizeof(ScratchEnt);
        if (prepared) return (size_t)(RING_UNITS + RING_MIRROR + AUX_UNITS) * sizeof(ScratchEnt) + (size_t)MID_CAP * 12;
        return SCR_CAP * sizeof(ScratchEnt) + (size_t)(slots + MOM_COPIES - 1 + 3) * FAR_ORDER * sizeof(double) + (size_t)MID_CAP * 12;
    };
    const size_t lds_rm = (prepared || solo) ? 0 : (size_t)((c->rows + 1) & ~1) * sizeof(double);
    auto lds_need = [&](int slots) { return lds + lds_rm + (size_t)((solo ? SITE_THREADS : SCAN_THREADS_MAX) / WAVE) * wave_bytes(slots); };
    // moment slots: as many (64, 32, 16, 8, 0) as leave the R slice in LDS; when the table is too large for LDS anyway
    // (many sample sizes: the sites spread over many rows), all MOM_SLOTS.  (The prepared pipeline's moments live in
    // prep_kernel's LDS: 64 slots with the table in LDS, all of them otherwise -- the same rule, so that both forms
    // classify alike.)
    while (!prepared && !solo && mom_slots >= 8 && lds_need(mom_slots) > (size_t)LDS_LIMIT_BYTES) mom_slots /= 2;
    if (mom_slots < 8) mom_slots = 0;
    const bool fits = lds_need(mom_slots) <= (size_t)LDS_LIMIT_BYTES && !diag_env("BMX_NO_LDS");   // BMX_NO_LDS: R from L2 (A/B runs)
    if (!fits || c->variant == 1) mom_slots = MOM_SLOTS;
    P.mom_slots = mom_slots;
    // test sites per workgroup: every workgroup loads its R slice into LDS first (52 KB at n = 100, 103 KB at n = 200), so large scans
    // give each wave two groups of 16 (128 test sites per 4 waves: +0.6 % at config 3, +2 % at config 5 over 64; 256 gains nothing more)
    int spb = J ? (s->M >= 65536 ? 128 : 4 * J) : (s->M >= 65536 ? 32 : SITE_THREADS / WAVE);   // per-site kernel: >= one test site per wave
    if (J == 16 && spb < 64) spb = 64;
    if (J && diag_env("BMX_SPB")) spb = std::max(4 * J, atoi(diag_env("BMX_SPB")) / (4 * J) * (4 * J));   // experiments
    const bool use_lds = fits && c->variant != 1;
    const void *fn = nullptr;
#define PICK(K) (use_lds ? (const void *)K<true> : (const void *)K<false>)
    // inner-loop form: 0 readlane / one site per step; 1 LDS broadcast + pairs; 2 = 1 + four sites per
    // step where alpha <= 1/2; 3 = 2 + power sums where alpha*max|R| <= far_eps; 4 = 3 with the per-group work prepared
    const int mode = solo ? 5 : prepared ? 4 : (v >= 5 && v <= 7) ? 0 : (v >= 8 && v <= 9) ? 1 : (v >= 10 && v <= 11) ? 2 : 3;
#define GP2(JJ, MM) (use_lds ? (const void *)clr_scan_grouped_kernel<JJ, true, MM> : (const void *)clr_scan_grouped_kernel<JJ, false, MM>)
#define GP4(JJ) (use_lds ? (const void *)clr_scan_prepared_kernel<JJ, true> : (const void *)clr_scan_prepared_kernel<JJ, false>)
#define GPICK(JJ) (mode == 4 ? GP4(JJ) : mode == 3 ? GP2(JJ, 3) : mode == 2 ? GP2(JJ, 2) : mode == 1 ? GP2(JJ, 1) : GP2(JJ, 0))
    if (J == 8) fn = GPICK(8);
    else if (J == 16) fn = GPICK(16);
    else if (J == 4) fn = GPICK(4);
    else if (solo) fn = PICK(clr_scan_solo_kernel);
    else fn = PICK(clr_scan_kernel);
    // profile likelihoods: the prepared and solo pipelines only
#define GPL(JJ) (use_lds ? (const void *)clr_scan_prepared_kernel<JJ, true, true> : (const void *)clr_scan_prepared_kernel<JJ, false, true>)
    const void *fn_pl = nullptr;
    if (mode == 4 && J == 16) fn_pl = GPL(16);
    else if (mode == 4 && J == 8) fn_pl = GPL(8);
    else if (mode == 4 && J == 4) fn_pl = GPL(4);
    else if (solo) fn_pl = use_lds ? (const void *)clr_scan_solo_kernel<true, true> : (const void *)clr_scan_solo_kernel<false, true>;
#undef GPL
#undef GP2
#undef GP4
#undef GPICK
#undef PICK
    // One wave per SIMD issues FP64 at half rate (measured), so a workgroup whose LDS footprint
    // allows only one resident workgroup per CU gets 8 waves instead of 4.
    int threads = SCAN_THREADS;
    size_t lds_bytes = (use_lds ? lds + (J ? lds_rm : 0) : 0) + (J ? (size_t)(threads / WAVE) * wave_bytes(mom_slots) : 0);
    if (J && 2 * lds_bytes > (size_t)LDS_LIMIT_BYTES) {
        threads = SCAN_THREADS_MAX;
        lds_bytes = (use_lds ? lds + lds_rm : 0) + (size_t)(threads / WAVE) * wave_bytes(mom_slots);
        spb *= 2;
    }
    if (prepared && J == 8 && use_lds) {
        // three waves per SIMD: ONE workgroup of twelve waves per CU (its registers allow it, see the kernel), if slice + twelve rings fit
        const size_t lds12 = lds + (size_t)(SCAN_THREADS_J8 / WAVE) * wave_bytes(mom_slots);
        if (lds12 <= (size_t)LDS_LIMIT_BYTES) {
            if (threads == SCAN_THREADS_MAX) spb /= 2;
            threads = SCAN_THREADS_J8;
            lds_bytes = lds12;
            spb = spb * 3;                 // the same number of groups per wave as with four waves
        }
    }
    if (!J) {       // per-site kernels: 16 waves, the R slice (if it fits) + 1 KB of scratch list (solo: 4.3 KB of ring) per wave
        threads = SITE_THREADS;
        lds_bytes = (use_lds ? lds : 0) + (size_t)(threads / WAVE) * (solo ? wave_bytes(0) : SITE_SCR * sizeof(ScratchEnt));
    }
    if (lds_bytes > (size_t)LDS_LIMIT_BYTES) return fail(BMX_E_LIMIT, "LDS budget exceeded");
    if (lds_bytes) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    P.sites_per_block = spb;
    pl.fn = fn; pl.fn_pl = fn_pl; pl.J = solo ? 1 : J; pl.threads = threads; pl.lds_bytes = lds_bytes; pl.spb = spb; pl.use_lds = use_lds;
    pl.mode = solo ? 5 : J ? mode : -1;
    // test sites per launch: keeps the per-slice winners (16 B x slices per test site) within ~512 MB and the grid
    // within 2^31 workgroups; a multiple of the workgroup's share, so ranges cut the test sites where workgroups do
    int64_t range = std::max<int64_t>((int64_t)(512u << 20) / (16 * (int64_t)c->nslices), spb);
    range = std::min<int64_t>(range, (int64_t)0x7fffff00LL / c->nslices * spb);
    // with profile likelihoods on, also their per-range keys (12 B per slice and A, 12 B per pair) within PL_SCRATCH_BYTES
    if (const int64_t plb = pl_bytes_per_test(c, c->pl_which)) range = std::min<int64_t>(range, std::max<int64_t>(PL_SCRATCH_BYTES / plb, spb));
    range = std::max<int64_t>(range / spb, 1) * spb;
    pl.range = range;
    if (prepared || solo) {
        pl.thr_in_lds = c->rows <= PREP_THR_LDS_MAX ? 1 : 0;
        // the moment slots of prep_kernel: 64 with the table in LDS, all of them otherwise (see above) -- but no more than any A
        // uses: the moment arrays are most of that kernel's LDS, and LDS per wave decides how many of its waves a CU holds
        const int pm = std::max(1, std::min(use_lds ? MOM_SLOTS_LDS : MOM_SLOTS, (prepared && J == 16) ? s->kmom_max_ser : s->kmom_max));
        P.mom_slots = pm;
        const size_t mom_fill = solo ? (size_t)(pm + S_COPIES - 1 + 3) * S_ORDER : 2 * (size_t)(pm + P_COPIES - 1 + 3) * P_ORDER + WAVE;
        const size_t mom_count = solo ? mom_fill : 2 * (size_t)(pm + P_COPIES - 1 + 3) + WAVE;      // grouped counting pass: one flag per slot
        pl.prep_threads = mom_fill * sizeof(double) > 20480 ? PREP_THREADS / 4 : PREP_THREADS;          // (all 254 slots: 25 KB per moment array)
        const size_t thr_b = pl.thr_in_lds ? (size_t)((c->rows + 1) & ~1) * sizeof(double) : 0;
        const size_t stage_b = solo ? (size_t)(SOLO_S0 + 2 * SOLO_S1) * sizeof(double) : 2 * SER_CAP * sizeof(ScratchEnt);   // near-entry staging / series entries
        pl.prep_lds = thr_b + (size_t)(pl.prep_threads / WAVE) * (mom_fill * sizeof(double) + stage_b);
        pl.prep_lds_count = thr_b + (size_t)(pl.prep_threads / WAVE) * (mom_count * sizeof(double) + (solo ? stage_b : 0));
        P.far_bits = (float)(P_EPS * 1.4427 * 1.1);          // |log1p(x)| <= 1.09 |x| for |x| <= 0.15 (1.16 at 0.25: order 16 uses 1.2)
        if (P_ORDER == 16) P.far_bits = (float)(P_EPS * 1.4427 * 1.2);
#define PP(JJ, FF) (const void *)prep_kernel<JJ, FF>
        if (solo) {
            pl.prep_count = (const void *)prep_solo_kernel<false>;
            pl.prep_fill = (const void *)prep_solo_kernel<true>;
        } else {
            pl.prep_count = J == 16 ? PP(16, false) : J == 8 ? PP(8, false) : PP(4, false);
            pl.prep_fill = J == 16 ? PP(16, true) : J == 8 ? PP(8, true) : PP(4, true);
        }
#undef PP
        if (pl.prep_lds > (size_t)LDS_LIMIT_BYTES) return fail(BMX_E_LIMIT, "LDS budget of the preparation kernel exceeded");
        HIP_TRY(hipFuncSetAttribute(pl.prep_count, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.prep_lds_count));
        HIP_TRY(hipFuncSetAttribute(pl.prep_fill, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.prep_lds));
    }
    TRACE("scan plan: lds=%zu use_lds=%d span_hi=%d spb=%d J=%d threads=%d range=%lld mode=%d", lds_bytes, (int)use_lds, c->span_hi, spb, J, threads,
          (long long)range, pl.mode);
    return BMX_OK;
}

PrepParams prep_params(bmx_ctx *c, ChromSlot *s, const ScanPlan &pl) {
    PrepParams Q;
    Q.genpos = s->genpos.p; Q.row = pl.P.row; Q.N = s->N;
    Q.rows = c->rows; Q.rowmul = pl.use_lds ? WAVE : c->NP;
    Q.A = c->d_A.p; Q.nA = c->nA;
    Q.test_gen = s->test_gen.p; Q.win_lo = s->win_lo.p; Q.win_hi = s->win_hi.p; Q.center = s->center.p; Q.center_hi = s->center_hi.p;
    Q.M = s->M; Q.zcut = c->zcut; Q.rmax = pl.P.rmax;
    Q.rowthr = s->rowthr.p; Q.thr_in_lds = pl.thr_in_lds;
    // series entries only where they are cheaper than the product: groups of 16 (a product entry costs 1.5 instructions per test site)
    const bool series = pl.mode == 4 && pl.J == 16;
    Q.kmom = s->kmom.p + (series ? c->nA : 0); Q.row_of_slot = s->d_row_of_slot.p; Q.mom_slots = pl.P.mom_slots;
    Q.ser_cap = !series ? 0 : diag_env("BMX_SER_CAP") ? std::min(std::max(atoi(diag_env("BMX_SER_CAP")), 0), SER_CAP) : SER_CAP;
    Q.g_begin = 0; Q.g_end = 0;
    Q.blob_units = s->blob_units.p; Q.blob_prefix = s->blob_prefix.p; Q.prefix_base = 0;
    Q.arena = c->arena.p; Q.status = c->d_status.p;
    return Q;
}

// Prepared pipeline, once per (model, sites, tests, variant): the counting pass over all groups, the prefix of the blob
// sizes, and the launch ranges -- cut where the per-slice winner arrays (pl.range) or the arena would overflow.
int ensure_prep(bmx_ctx *c, ChromSlot *s) {
    ScanPlan &pl = s->plan;
    if (pl.mode < 4 || s->prep_ok) return BMX_OK;
    const int J = pl.J;
    const int64_t ngroups = (s->M + J - 1) / J;
    HIP_TRY(s->blob_units.ensure((size_t)ngroups));
    HIP_TRY(s->blob_prefix.ensure((size_t)ngroups + 1));
    PrepParams Q = prep_params(c, s, pl);
    Q.g_begin = 0; Q.g_end = ngroups;
    const int gpw = pl.prep_threads / WAVE;
    void *kargs[] = {&Q};
    {
        std::lock_guard<std::mutex> launch_lock(g_launch_mu);
        if (pl.prep_lds_count) HIP_TRY(hipFuncSetAttribute(pl.prep_count, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.prep_lds_count));
        HIP_TRY(hipLaunchKernel(pl.prep_count, dim3((unsigned)((ngroups + gpw - 1) / gpw)), dim3(pl.prep_threads), kargs, pl.prep_lds_count, c->stream));
    }
    hipLaunchKernelGGL(prefix_kernel, dim3(1), dim3(1024), 0, c->stream, (const int32_t *)s->blob_units.p, ngroups, s->blob_prefix.p);
    HIP_TRY(hipGetLastError());
    std::vector<int64_t> pre((size_t)ngroups + 1);
    HIP_TRY(hipMemcpyAsync(pre.data(), s->blob_prefix.p, pre.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    // arena budget: a quarter of what is free now (plus what the arena already holds), at most 16 GiB
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const int64_t cap_units = (int64_t)(std::min<size_t>((free_b + c->arena.cap * sizeof(ScratchEnt)) / 4, (size_t)16 << 30) / sizeof(ScratchEnt));
    const int64_t gstep = std::max<int64_t>(pl.spb / J, 1);       // groups per workgroup of the consumer
    s->ranges.clear();
    int64_t need = 0;
    for (int64_t g0 = 0; g0 < ngroups;) {
        int64_t g1 = g0;
        while (g1 < ngroups) {
            const int64_t g2 = std::min(g1 + gstep, ngroups);
            if (g1 > g0 && ((g2 - g0) * J > pl.range || pre[(size_t)g2] - pre[(size_t)g0] > cap_units)) break;
            g1 = g2;
        }
        const int64_t units = pre[(size_t)g1] - pre[(size_t)g0];
        if (units > cap_units) return fail(BMX_E_LIMIT, "prepared scan: one workgroup's share of the stream does not fit the device memory left");
        s->ranges.push_back(PrepRange{g0 * J, std::min(g1 * J, s->M) - g0 * J, g0, g1 - g0, pre[(size_t)g0], units});
        need = std::max(need, units);
        g0 = g1;
    }
    // the consumers' read-ahead runs up to five chunks past a blob's end.  A slot with permuted rows (permutation null) is
    // prepared again for every replicate and its stream size varies a little with the permutation: an arena that has to grow
    // then takes an eighth more, so that it is not re-allocated replicate after replicate (~0.4 s each at 1 M test sites)
    const size_t want = (size_t)need + 8 * WAVE;
    HIP_TRY(c->arena.ensure(s->has_orig && want > c->arena.cap ? want + want / 8 : want));
    TRACE("prepared: %lld groups, %.1f MB of blobs, %zu launch range(s), arena %.1f MB", (long long)ngroups, (double)pre[(size_t)ngroups] * 16e-6,
          s->ranges.size(), (double)c->arena.cap * 16e-6);
    s->prep_ok = true;
    return BMX_OK;
}

int ensure_plan(bmx_ctx *c, ChromSlot *s) {
    if (!s->plan_ok || s->plan_variant != c->variant || s->plan_pl != c->pl_which) {
        s->plan_ok = false;
        s->prep_ok = false;
        int rc = plan_scan(c, s, s->plan);
        if (rc) return rc;
        s->plan_ok = true;
        s->plan_variant = c->variant;
        s->plan_pl = c->pl_which;
    }
    return ensure_prep(c, s);
}

// scan + finalize of test sites [off, off + cnt) on the context's stream (asynchronous)
int launch_range(bmx_ctx *c, ChromSlot *s, ScanPlan &pl, int64_t off, int64_t cnt, const PrepRange *pr) {
    std::lock_guard<std::mutex> launch_lock(g_launch_mu);
    ScanParams P = pl.P;
    const size_t np = (size_t)cnt * c->nslices;
    HIP_TRY(c->part_T.ensure(np));
    HIP_TRY(c->part_lin.ensure(np));
    HIP_TRY(c->part_ns.ensure(np));
    P.test_gen = s->test_gen.p + off; P.win_lo = s->win_lo.p + off; P.win_hi = s->win_hi.p + off;
    P.center = s->center.p + off; P.center_hi = s->center_hi.p + off; P.M = cnt;
    P.part_T = c->part_T.p; P.part_lin = c->part_lin.p; P.part_ns = c->part_ns.p;
    const int plw = c->pl_which;
    const void *fn = plw ? pl.fn_pl : pl.fn;
    if (!fn) return fail(BMX_E_LIMIT, "profile likelihoods: this scan plan has no profile form");
    if (plw) {
        if (plw & BMX_PL_A) {
            HIP_TRY(c->pl_am.ensure((size_t)cnt * c->nslices * c->nA));
            HIP_TRY(c->pl_ae.ensure((size_t)cnt * c->nslices * c->nA));
        }
        if (plw & (BMX_PL_X | BMX_PL_ABETA)) {
            HIP_TRY(c->pl_pm.ensure((size_t)cnt * c->NP));
            HIP_TRY(c->pl_pe.ensure((size_t)cnt * c->NP));
        }
    }
    if (pl.lds_bytes) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes));
    int64_t blocks = (cnt + pl.spb - 1) / pl.spb * c->nslices;
    if (pr && (pl.mode == 5 ? BMX_SOLO_XCD_MAP : BMX_XCD_MAP)) blocks = ((cnt + pl.spb - 1) / pl.spb + 7) / 8 * 8 * c->nslices;     // chunks padded to whole XCD rounds
    if (pr) {
        // the range's blobs: filled by the per-group kernel, then consumed by one wave per (group, slice)
        if ((size_t)pr->units + 8 * WAVE > c->arena.cap) HIP_TRY(c->arena.ensure((size_t)pr->units + 8 * WAVE));
        PrepParams Q = prep_params(c, s, pl);
        Q.g_begin = pr->g0; Q.g_end = pr->g0 + pr->ng; Q.prefix_base = pr->pbase;
        const int gpw = pl.prep_threads / WAVE;
        void *qargs[] = {&Q};
        // (the dynamic-LDS limit is an attribute of the FUNCTION, shared by every slot and context; another slot's plan may have
        // lowered it since this one was made)
        if (pl.prep_lds) HIP_TRY(hipFuncSetAttribute(pl.prep_fill, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.prep_lds));
        HIP_TRY(hipLaunchKernel(pl.prep_fill, dim3((unsigned)((pr->ng + gpw - 1) / gpw)), dim3(pl.prep_threads), qargs, pl.prep_lds, c->stream));
        PrepView V;
        V.arena = c->arena.p; V.blob_prefix = s->blob_prefix.p; V.prefix_base = pr->pbase; V.grp_base = pr->g0; V.status = c->d_status.p;
        V.pl_am = (plw & BMX_PL_A) ? c->pl_am.p : nullptr; V.pl_ae = (plw & BMX_PL_A) ? c->pl_ae.p : nullptr;
        V.pl_pm = (plw & (BMX_PL_X | BMX_PL_ABETA)) ? c->pl_pm.p : nullptr; V.pl_pe = (plw & (BMX_PL_X | BMX_PL_ABETA)) ? c->pl_pe.p : nullptr;
        void *kargs[] = {&P, &V};
        HIP_TRY(hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(pl.threads), kargs, pl.lds_bytes, c->stream));
    } else {
        void *kargs[] = {&P};
        HIP_TRY(hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(pl.threads), kargs, pl.lds_bytes, c->stream));
    }
    FinalParams F;
    F.part_T = c->part_T.p; F.part_lin = c->part_lin.p; F.part_ns = c->part_ns.p;
    F.nslices = c->nslices; F.npairs = c->npairs; F.M = cnt; F.N = s->N;
    F.genpos = s->genpos.p; F.A = c->d_A.p; F.test_gen = P.test_gen; F.win_lo = P.win_lo; F.win_hi = P.win_hi;
    F.center = P.center; F.center_hi = P.center_hi; F.zcut = c->zcut;
    F.clr = s->clr.p + off; F.lin = s->lin.p + off; F.nsites = s->nsites.p + off; F.rec = s->rec.p + off;
    F.over = c->d_status.p + 1 + s->index;
    const int fthreads = 256;
    hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)((cnt + fthreads - 1) / fthreads)), dim3(fthreads), 0, c->stream, F);
    HIP_TRY(hipGetLastError());
    for (int kind = 0; kind < 3; ++kind) {
        if (!(plw & (1 << kind))) continue;
        PlFinalParams G;
        G.am = c->pl_am.p; G.ae = c->pl_ae.p; G.pm = c->pl_pm.p; G.pe = c->pl_pe.p;
        G.kind = kind; G.nslices = c->nslices; G.nA = c->nA; G.nx = c->nx; G.nab = c->nab; G.NP = c->NP; G.M = cnt;
        const int n = kind == 0 ? c->nA : kind == 1 ? c->nx : c->nab;
        G.out = s->pl_out[kind].p + (size_t)off * n;
        const int64_t items = cnt * n;
        hipLaunchKernelGGL(profile_finalize_kernel, dim3((unsigned)((items + fthreads - 1) / fthreads)), dim3(fthreads), 0, c->stream, G);
        HIP_TRY(hipGetLastError());
    }
    return BMX_OK;
}

// before the launches of a scan: the profile set it computes (the slot's profile arrays sized for it), or BMX_E_LIMIT where the
// plan's kernels have no profile form.  The slot's profiles are valid again once every range has been launched.
int begin_profiles(bmx_ctx *c, ChromSlot *s) {
    const int w = c->pl_which;
    if (w && !s->plan.fn_pl)       // refused before anything is launched: the last scan's results and profiles stay as they are
        return fail(BMX_E_LIMIT, "profile likelihoods need the prepared or solo scan kernels; this plan uses a round-2 kernel "
                                 "(a table of 4 GiB or more, 2^31 sites or more, or a diagnostic variant)");
    s->pl_have = 0;
    if (!w) return BMX_OK;
    const int n[3] = {c->nA, c->nx, c->nab};
    for (int k = 0; k < 3; ++k)
        if (w & (1 << k)) HIP_TRY(s->pl_out[k].ensure((size_t)s->M * n[k]));
    return BMX_OK;
}

// the launch ranges of a slot's scan: the prepared pipeline's own, or plain cuts of pl.range test sites
int scan_ranges(bmx_ctx *c, ChromSlot *s, std::vector<PrepRange> &out) {
    int rc = ensure_plan(c, s);
    if (rc) return rc;
    out.clear();
    if (s->plan.mode >= 4) { out = s->ranges; return BMX_OK; }
    for (int64_t off = 0; off < s->M; off += s->plan.range)
        out.push_back(PrepRange{off, std::min(s->plan.range, s->M - off), 0, 0, 0, 0});
    return BMX_OK;
}

// before the launches of a scan of slot s: its range word starts at 0
int begin_range_word(bmx_ctx *c, ChromSlot *s) {
    HIP_TRY(hipMemsetAsync(c->d_status.p + 1 + s->index, 0, sizeof(int), c->stream));
    return BMX_OK;
}

// the device-side error bits of the prepared pipeline, checked wherever results leave the library (the first reader clears them),
// and with the same read the range word of slot s -- of every slot for s == nullptr -- where it holds scan results: a winner at
// the exponent clamp is BMX_E_LIMIT every time, until that slot is scanned again
int check_status(bmx_ctx *c, const ChromSlot *s) {
    std::vector<int> st(1 + c->slots.size(), 0);
    HIP_TRY(hipMemcpy(st.data(), c->d_status.p, st.size() * sizeof(int), hipMemcpyDeviceToHost));
    if (st[0]) {
        HIP_TRY(hipMemset(c->d_status.p, 0, sizeof(int)));
        return fail(BMX_E_HIP, st[0] & 1 ? "prepared scan: a group's stream differs in size from the counting pass" : "prepared scan: bad zone header in a group's stream");
    }
    for (size_t i = 0; i < c->slots.size(); i++) {
        const ChromSlot *q = c->slots[i].get();
        if (q && (!s || s == q) && q->has_results() && st[1 + i])
            return fail(BMX_E_LIMIT, "scan: a window of slot " + std::to_string(i) + " has a CLR past the scan's range (|T| <= 2 ln 2 x 131070 = 1.817e5 per "
                                     "grid point): the slot's results are withheld until it is scanned again with narrower windows");
    }
    return BMX_OK;
}

}  // namespace

extern "C" {

int bmx_ctx_scan(bmx_ctx *c) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->ready_to_scan(c)) return fail(BMX_E_STATE, "model, sites and tests must be set before scan");
    HIP_TRY(hipSetDevice(c->device));
    std::vector<PrepRange> rs;
    int rc = scan_ranges(c, s, rs);
    if (rc) return rc;
    if ((rc = begin_profiles(c, s))) return rc;
    if ((rc = begin_range_word(c, s))) return rc;
    HIP_TRY(s->scan.begin(c->stream));
    for (const PrepRange &r : rs)
        if ((rc = launch_range(c, s, s->plan, r.off, r.cnt, s->plan.mode >= 4 ? &r : nullptr))) return rc;
    HIP_TRY(s->scan.end(c->stream));
    s->timed = true;
    s->pl_have = c->pl_which;
    s->scan_seq++;
    return BMX_OK;
}

/* What the scan of the selected slot will launch (valid once the test sites are set): group size J (0: one test site per
 * wave), 1 if the R slice is read from LDS, the inner-loop mode (4: prepared pipeline, 0..3: round-2 grouped forms, -1:
 * per-site kernel), and the bytes of the prepared stream of all test sites (0 otherwise).  Any pointer may be NULL. */
int bmx_ctx_plan(bmx_ctx *c, int32_t *J, int32_t *use_lds, int32_t *mode, int64_t *stream_bytes) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->ready_to_scan(c)) return fail(BMX_E_STATE, "model, sites and tests must be set before the plan exists");
    HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_plan(c, s);
    if (rc) return rc;
    if (J) *J = s->plan.J;
    if (use_lds) *use_lds = s->plan.use_lds ? 1 : 0;
    if (mode) *mode = s->plan.mode;
    if (stream_bytes) {
        int64_t u = 0;
        if (s->plan.mode >= 4) for (const PrepRange &r : s->ranges) u += r.units;
        *stream_bytes = u * (int64_t)sizeof(ScratchEnt);
    }
    return BMX_OK;
}

int bmx_ctx_launch_ranges(bmx_ctx *c, int64_t *offs, int32_t cap, int32_t *n_out) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->ready_to_scan(c)) return fail(BMX_E_STATE, "model, sites and tests must be set before the plan exists");
    HIP_TRY(hipSetDevice(c->device));
    std::vector<PrepRange> rs;
    int rc = scan_ranges(c, s, rs);
    if (rc) return rc;
    if (n_out) *n_out = (int32_t)rs.size();
    for (size_t i = 0; i < rs.size() && (int64_t)i < cap && offs; i++) offs[i] = rs[i].off;
    return BMX_OK;
}

int bmx_ctx_sync(bmx_ctx *c) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
#if defined(BMX_PROFILE) || defined(BMX_COUNT)
    if (c->d_prof.p) {
        unsigned long long h[32];
        HIP_TRY(hipMemcpy(h, c->d_prof.p, sizeof h, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemset(c->d_prof.p, 0, sizeof h));
#ifdef BMX_COUNT
        static const char *cn[16] = {"bulk passes with sites", "passes with a near list", "quad blocks", "pair blocks", "near-list sites",
                                     "far (moment) sites", "generic passes with sites", "generic passes", "zones folded/flushed",
                                     "fold slots non-empty", "fold slots scanned (kmom)", "ragged zones", "generic walk passes",
                                     "bulk pass iterations", "bulk sites", "zones"};
        for (int k = 0; k < 16; k++) fprintf(stderr, "[bmx count] %-28s %llu\n", cn[k], h[16 + k]);
#endif
        double tot = 0;
        for (int k = 0; k < 12; k++) tot += (double)h[k];
        static const char *nm[12] = {"between test sites", "zone set-up", "per-pass: rank, list position, tail", "near-list block loops", "ragged-end masks",
                                    "fold of moments", "flush", "generic walks past zones", "best-tracking", "near-list set-up",
                                    "per-pass: loads, exp, classify", "per-pass: moment adds"};
        static const char *np[12] = {"between test sites", "zone header", "pair lists", "quad lists", "generic walks past zones", "fold of moments",
                                    "series entries", "ragged end + Horner", "exp + apply", "renormalise + best-tracking", "group set-up", "winners out"};
        const bool prep_names = diag_env("BMX_PROF_PREPARED") != nullptr;
        if (tot > 0) for (int k = 0; k < 12; k++) fprintf(stderr, "[bmx prof] %-36s %5.1f %%\n", (prep_names ? np : nm)[k], 100.0 * (double)h[k] / tot);
    }
#endif
    return check_status(c, c->cur);
}

/* The records of every slot that holds scan results, in slot order, back to back: the whole genome's results with one
 * call (and, on a device buffer, what ONE gather then moves to the writing rank).  dst: room for `cap` records, in host
 * memory (dst_on_device = 0) or device memory of this context's GPU (1); n_out: records written.  Blocks until done. */
int bmx_ctx_pack_records(bmx_ctx *c, void *dst, int64_t cap, int32_t dst_on_device, int64_t *n_out) {
    if (!c || (!dst && cap > 0)) return fail(BMX_E_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    int64_t n = 0;
    for (const auto &s : c->slots)
        if (s && s->has_results()) n += s->M;
    if (n_out) *n_out = n;
    if (n > cap) return fail(BMX_E_INVALID, "pack_records: destination too small");
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int st = check_status(c, nullptr)) return st;        // before anything is copied: the destination may be another device's input
    int64_t at = 0;
    for (const auto &s : c->slots) {
        if (!s || !s->has_results()) continue;
        HIP_TRY(hipMemcpyAsync((bmx_record *)dst + at, s->rec.p, (size_t)s->M * sizeof(bmx_record),
                               dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
        at += s->M;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BMX_OK;
}

int bmx_ctx_copy_records(bmx_ctx *c, void *dst_device, int64_t cap) {
    if (!c || !dst_device) return fail(BMX_E_INVALID, "NULL argument");
    ChromSlot *s = c->cur;
    if (!s->has_results()) return fail(BMX_E_STATE, "no scan results in the selected slot");
    if (cap < s->M) return fail(BMX_E_INVALID, "copy_records: destination too small");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int st = check_status(c, s)) return st;
    HIP_TRY(hipMemcpyAsync(dst_device, s->rec.p, (size_t)s->M * sizeof(bmx_record), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BMX_OK;
}

int bmx_ctx_last_scan_ms(bmx_ctx *c, double *ms) {
    if (!c || !ms) return fail(BMX_E_INVALID, "NULL argument");
    ChromSlot *s = c->cur;
    if (!s->timed) return fail(BMX_E_STATE, "no scan has been launched");
    HIP_TRY(hipEventSynchronize(s->scan.ev1));
    HIP_TRY(s->scan.read());
    *ms = s->scan.ms;
    return BMX_OK;
}

int bmx_ctx_result_ptrs(bmx_ctx *c, void **d_clr, void **d_lin, void **d_nsites) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->has_results()) return fail(BMX_E_STATE, "no scan results: call bmx_ctx_scan after bmx_ctx_set_tests");
    if (d_clr) *d_clr = s->clr.p;
    if (d_lin) *d_lin = s->lin.p;
    if (d_nsites) *d_nsites = s->nsites.p;
    return BMX_OK;
}

int bmx_ctx_records(bmx_ctx *c, void **d_rec) {
    if (!c || !d_rec) return fail(BMX_E_INVALID, "NULL argument");
    ChromSlot *s = c->cur;
    if (!s->has_results()) return fail(BMX_E_STATE, "no scan results: call bmx_ctx_scan after bmx_ctx_set_tests");
    *d_rec = s->rec.p;
    return BMX_OK;
}

int bmx_ctx_fetch_records(bmx_ctx *c, bmx_record *rec) {
    if (!c || !rec) return fail(BMX_E_INVALID, "NULL argument");
    ChromSlot *s = c->cur;
    if (!s->has_results()) return fail(BMX_E_STATE, "no scan results to fetch");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int st = check_status(c, s)) return st;
    HIP_TRY(hipMemcpy(rec, s->rec.p, (size_t)s->M * sizeof(bmx_record), hipMemcpyDeviceToHost));
    return BMX_OK;
}

int bmx_ctx_fetch(bmx_ctx *c, double *clr, int32_t *ix, int32_t *ia, int32_t *iA, int32_t *nsites) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->has_results()) return fail(BMX_E_STATE, "no scan results to fetch");
    HIP_TRY(hipSetDevice(c->device));
    std::vector<int32_t> lin((size_t)s->M);
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int st = check_status(c, s)) return st;
    HIP_TRY(download(clr, s->clr.p, (size_t)s->M));
    HIP_TRY(download(nsites, s->nsites.p, (size_t)s->M));
    HIP_TRY(hipMemcpy(lin.data(), s->lin.p, (size_t)s->M * sizeof(int32_t), hipMemcpyDeviceToHost));
    const int32_t npairs = c->npairs, nab = c->nab;
    parallel_ranges(s->M, 1 << 18, [&](int, int64_t b, int64_t e) {
        for (int64_t t = b; t < e; t++) {
            const int32_t L = lin[(size_t)t];
            int32_t a = -1, bb = -1, d = -1;
            if (L >= 0) {
                d = L / npairs;
                const int32_t p = L % npairs;
                a = p / nab;
                bb = p % nab;
            }
            if (ix) ix[t] = a;
            if (ia) ia[t] = bb;
            if (iA) iA[t] = d;
        }
    });
    return BMX_OK;
}

/* ---- profile likelihoods (ballermixplus_amd/profiles.py holds the host definition and the writers) ---- */

int bmx_ctx_set_profiles(bmx_ctx *c, int32_t which) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    if (which < 0 || which > (BMX_PL_A | BMX_PL_X | BMX_PL_ABETA)) return fail(BMX_E_INVALID, "profiles: a set of BMX_PL_A, BMX_PL_X, BMX_PL_ABETA");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->pl_which = which;
    if (!which) {       // off: nothing of the profiles stays on the device
        c->pl_am.release(); c->pl_ae.release(); c->pl_pm.release(); c->pl_pe.release();
        for (const auto &s : c->slots) {
            if (!s) continue;
            s->pl_have = 0;
            for (auto &b : s->pl_out) b.release();
        }
    }
    return BMX_OK;
}

int bmx_ctx_fetch_profile(bmx_ctx *c, int32_t which, double *out) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    if (which != BMX_PL_A && which != BMX_PL_X && which != BMX_PL_ABETA) return fail(BMX_E_INVALID, "fetch_profile: one of BMX_PL_A, BMX_PL_X, BMX_PL_ABETA");
    if (!out) return fail(BMX_E_INVALID, "NULL argument");
    ChromSlot *s = c->cur;
    if (!s->has_results() || !(s->pl_have & which)) return fail(BMX_E_STATE, "the slot's last scan did not compute this profile");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int st = check_status(c, s)) return st;
    const int k = which == BMX_PL_A ? 0 : which == BMX_PL_X ? 1 : 2;
    const int n = k == 0 ? c->nA : k == 1 ? c->nx : c->nab;
    if (s->M) HIP_TRY(hipMemcpy(out, s->pl_out[k].p, (size_t)s->M * n * sizeof(double), hipMemcpyDeviceToHost));
    return BMX_OK;
}

/* ---- permutation null (ballermixplus_amd/null.py holds the host reference of the permutation) ---- */

int bmx_ctx_permute_rows(bmx_ctx *c, uint64_t key, int64_t block) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->has_sites) return fail(BMX_E_STATE, "set_sites must precede permute_rows");
    if (block < 1) return fail(BMX_E_INVALID, "permutation block size must be >= 1");
    HIP_TRY(hipSetDevice(c->device));
    const size_t N = (size_t)s->N;
    if (!s->has_orig) {         // first permutation since set_sites: keep the given rows (on the stream, after any scan reading them)
        if (s->wide_rows) HIP_TRY(s->orig32.ensure(N));
        else HIP_TRY(s->orig16.ensure(N));
        HIP_TRY(hipMemcpyAsync(s->orig_ptr(), s->row_ptr(), s->row_bytes(N), hipMemcpyDeviceToDevice, c->stream));
        s->has_orig = true;
    }
    PermParams Q;
    Q.N = s->N;
    Q.B = block;
    Q.nb = s->N / block;
    if (Q.nb < 2) {             // sigma is the identity: the rows given to set_sites
        HIP_TRY(hipMemcpyAsync(s->row_ptr(), s->orig_ptr(), s->row_bytes(N), hipMemcpyDeviceToDevice, c->stream));
    } else {
        int w = 0;
        for (uint64_t v = (uint64_t)(Q.nb - 1); v; v >>= 1) w++;
        Q.h = std::max(4, (w + 1) / 2);
        Q.mask = (1ull << Q.h) - 1;
        for (int j = 0; j < 8; j++) Q.rk[j] = bmx_mix64(key + (uint64_t)j);
        const unsigned blocks = (unsigned)std::min<int64_t>((s->N + 255) / 256, 8192);
        if (s->wide_rows) hipLaunchKernelGGL(permute_rows_kernel<uint32_t>, dim3(blocks), dim3(256), 0, c->stream, s->orig32.p, s->row32.p, Q);
        else hipLaunchKernelGGL(permute_rows_kernel<uint16_t>, dim3(blocks), dim3(256), 0, c->stream, s->orig16.p, s->row16.p, Q);
        HIP_TRY(hipGetLastError());
    }
    // the per-row site counts (moment slots, rowthr) do not change; which sites are near a test site does: the prepared
    // pipeline's counting pass and launch ranges are redone by the next scan
    s->plan_ok = false;
    s->prep_ok = false;
    return BMX_OK;
}

int bmx_ctx_restore_rows(bmx_ctx *c) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->has_sites) return fail(BMX_E_STATE, "set_sites must precede restore_rows");
    if (!s->has_orig) return BMX_OK;        // never permuted: the rows are the given ones
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(s->row_ptr(), s->orig_ptr(), s->row_bytes((size_t)s->N), hipMemcpyDeviceToDevice, c->stream));
    s->plan_ok = false;
    s->prep_ok = false;
    return BMX_OK;
}

int bmx_ctx_null_begin(bmx_ctx *c) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->has_results()) return fail(BMX_E_STATE, "null_begin needs the observed scan: call bmx_ctx_scan first");
    HIP_TRY(hipSetDevice(c->device));
    const size_t M = (size_t)s->M;
    HIP_TRY(s->null_obs.ensure(M));
    HIP_TRY(s->null_cnt.ensure(M));
    HIP_TRY(s->null_part.ensure((size_t)NULL_BLOCKS_MAX + 1));
    HIP_TRY(hipMemcpyAsync(s->null_obs.p, s->clr.p, M * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(s->null_cnt.p, 0, M * sizeof(int32_t), c->stream));
    s->null_ok = true;
    s->null_reps = 0;
    s->null_seq = s->scan_seq;
    return BMX_OK;
}

int bmx_ctx_null_accumulate(bmx_ctx *c, double *max_out) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->null_ok) return fail(BMX_E_STATE, "null_begin must precede null_accumulate");
    if (!s->timed || s->scan_seq == s->null_seq) return fail(BMX_E_STATE, "null_accumulate needs a new scan (one per replicate)");
    HIP_TRY(hipSetDevice(c->device));
    const int blocks = (int)std::min<int64_t>((s->M + NULL_THREADS - 1) / NULL_THREADS, NULL_BLOCKS_MAX);
    double *part = s->null_part.p, *mx = s->null_part.p + NULL_BLOCKS_MAX;
    hipLaunchKernelGGL(null_count_kernel, dim3(blocks), dim3(NULL_THREADS), 0, c->stream, (const double *)s->clr.p,
                       (const double *)s->null_obs.p, s->null_cnt.p, s->M, part);
    hipLaunchKernelGGL(null_max_kernel, dim3(1), dim3(NULL_THREADS), 0, c->stream, (const double *)part, blocks, mx);
    HIP_TRY(hipGetLastError());
    double m = 0.0;
    HIP_TRY(hipMemcpyAsync(&m, mx, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int st = check_status(c, s)) return st;      // the replicate's scan must have been sound (a stale prepared stream shows here)
    s->null_seq = s->scan_seq;
    s->null_reps++;
    if (max_out) *max_out = m;
    return BMX_OK;
}

int bmx_ctx_null_fetch(bmx_ctx *c, int32_t *counts, int32_t *replicates) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->null_ok) return fail(BMX_E_STATE, "null_begin must precede null_fetch");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(download(counts, s->null_cnt.p, (size_t)s->M));
    if (replicates) *replicates = s->null_reps;
    return BMX_OK;
}

int bmx_ctx_fetch_lut(bmx_ctx *c, double *psel_out, double *R_out) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    if (!c->has_model) return fail(BMX_E_STATE, "no model set");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t tab = (size_t)c->npairs * c->rows;
    HIP_TRY(download(psel_out, c->d_psel.p, tab));
    HIP_TRY(download(R_out, c->d_R.p, tab));
    return BMX_OK;
}

int bmx_ctx_surface(bmx_ctx *c, double test_gen, int64_t win_lo, int64_t win_hi, double *T_out, int32_t *nsites_out) {
    if (!c || !T_out) return fail(BMX_E_INVALID, "NULL argument");
    ChromSlot *s = c->cur;
    if (!c->has_model || !s->has_sites) return fail(BMX_E_STATE, "model and sites must be set before surface");
    HIP_TRY(hipSetDevice(c->device));
    SurfParams S;
    S.genpos = s->genpos.p; S.row = s->row_array(); S.N = s->N; S.Rt = c->d_Rt.p; S.NP = c->NP; S.npairs = c->npairs;
    S.nslices = c->nslices; S.A = c->d_A.p; S.nA = c->nA; S.tg = test_gen;
    S.lo = std::max<int64_t>(win_lo, 0); S.hi = std::min<int64_t>(win_hi, s->N - 1); S.zcut = c->zcut;
    HIP_TRY(c->surf_T.ensure((size_t)c->nA * c->npairs));
    HIP_TRY(c->surf_ns.ensure((size_t)c->nA));
    S.T = c->surf_T.p; S.ns = c->surf_ns.p;
    hipLaunchKernelGGL(surface_kernel, dim3((unsigned)(c->nA * c->nslices)), dim3(WAVE), 0, c->stream, S);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(T_out, c->surf_T.p, (size_t)c->nA * c->npairs * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (nsites_out) HIP_TRY(hipMemcpyAsync(nsites_out, c->surf_ns.p, (size_t)c->nA * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BMX_OK;
}

// The three listed-surface calls: their own refusals, then listed_surfaces.  They differ on purpose in three places, held by the
// refusal and lifetime tests: bmx_ctx_surfaces refuses a NULL T_out where the other two take it as "do not copy the surfaces
// back"; with n == 0 it leaves its milliseconds alone where the other two set theirs to 0.0; and bmx_ctx_base_surfaces refuses a
// missing baseline after list_ready and before its n == 0 return.
int bmx_ctx_surfaces(bmx_ctx *c, int64_t n, const int32_t *tests, double *T_out, int32_t *nsites_out) {
    int rc;
    if ((rc = list_ready(c, "surfaces", n, nullptr, !tests || !T_out))) return rc;
    if (n == 0) return BMX_OK;
    return listed_surfaces(c, "surfaces", n, tests, c->sfs, [&](const SurfsParams &S, int64_t, dim3 grid) {
        hipLaunchKernelGGL(surfaces_kernel, grid, dim3(SURFS_THREADS), 0, c->stream, S);
    }, T_out, nsites_out, nullptr, nullptr, nullptr);
}

int bmx_ctx_surfaces_ms(bmx_ctx *c, double *ms) {
    if (!c || !ms) return fail(BMX_E_INVALID, "NULL argument");
    return c->sfs.get(ms, "no surfaces call yet");
}

int bmx_ctx_influence(bmx_ctx *c, int64_t n, const int32_t *tests, int64_t block) {
    int rc;
    if ((rc = list_ready(c, "influence", n, block < 1 ? "block < 1" : nullptr, !tests))) return rc;
    ChromSlot *s = c->cur;
    for (int64_t q = 0; q < n; q++)
        if (tests[q] < 0 || tests[q] >= s->M) return fail(BMX_E_INVALID, "influence: test site index out of range at entry " + std::to_string(q));
    c->if_have = false;
    c->if_first.assign((size_t)n, 0);
    c->if_off.assign((size_t)n + 1, 0);
    c->if_h_tmax.assign((size_t)n, 0.0); c->if_h_lin.assign((size_t)n, -1); c->if_h_ns.assign((size_t)n, 0);
    c->if_h_m.clear(); c->if_h_contrib.clear(); c->if_h_L.clear(); c->if_h_blin.clear();
    c->ifl.ms = 0.0;
    if (n == 0) { c->if_have = true; return BMX_OK; }
    HIP_TRY(hipSetDevice(c->device));
    const int64_t B = std::min(block, std::max<int64_t>(s->N, 1));        // i / B is 0 for every site either way
    const int iAmin = (int)(std::min_element(c->h_A.begin(), c->h_A.end()) - c->h_A.begin());
    if ((rc = upload(c->sfs_list, tests, (size_t)n, c->stream))) return rc;
    // 1. every listed window's qualifying sites at A_min -> its block range and the offsets of the per-block arrays
    InflRangeParams Q;
    Q.sites = site_view(s); Q.win = window_view(c, s);
    std::vector<int64_t> h_rng((size_t)n * 4);
    const int64_t rstep = 1 << 20;
    HIP_TRY(c->if_rng1.ensure((size_t)std::min(rstep, n) * 4));
    const int wpb = INFL_THREADS / WAVE;
    for (int64_t q0 = 0; q0 < n; q0 += rstep) {
        const int64_t m = std::min(rstep, n - q0);
        Q.A = c->d_A.p + iAmin; Q.nA = 1; Q.tests = c->sfs_list.p + q0; Q.n = m; Q.rng = c->if_rng1.p;
        hipLaunchKernelGGL(influence_range_kernel, dim3((unsigned)((m + wpb - 1) / wpb)), dim3(INFL_THREADS), 0, c->stream, Q);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_rng.data() + (size_t)q0 * 4, c->if_rng1.p, (size_t)m * 4 * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    for (int64_t q = 0; q < n; q++) {
        const int64_t first = h_rng[(size_t)q * 4 + 2], last = h_rng[(size_t)q * 4 + 3];
        const bool any = first <= last;
        c->if_first[(size_t)q] = any ? first / B : 0;
        c->if_off[(size_t)q + 1] = c->if_off[(size_t)q] + (any ? last / B - first / B + 1 : 0);
        if (c->if_off[(size_t)q + 1] > BMX_INFLUENCE_MAX_RESULTS)
            return fail(BMX_E_LIMIT, "influence: more than BMX_INFLUENCE_MAX_RESULTS blocks in one call; list fewer windows");
    }
    const size_t total = (size_t)c->if_off[(size_t)n];
    c->if_h_m.assign(total, 0); c->if_h_contrib.assign(total, 0.0); c->if_h_L.assign(total, 0.0); c->if_h_blin.assign(total, -1);
    // 2. chunks of windows: as many as bmx_ctx_surfaces takes at a time, and at most INFL_CHUNK_BLOCKS blocks (one window if it has more)
    const size_t per = (size_t)c->nA * c->npairs;
    const int nsl = (c->npairs + SURFS_THREADS - 1) / SURFS_THREADS;
    const int64_t step = surfaces_step(c, nsl);
    const int64_t INFL_CHUNK_BLOCKS = 1 << 22;
    SurfsParams S = surfs_params(c, s, nsl);
    InflParams P;
    P.sites = Q.sites; P.win = Q.win; P.Rt = c->d_Rt.p; P.NP = c->NP; P.npairs = c->npairs; P.nslices = nsl;
    P.A = c->d_A.p; P.nA = c->nA; P.iAmin = iAmin; P.B = B;
    std::vector<InflItem> items;
    std::vector<int32_t> h_ns;
    double total_ms = 0.0;
    for (int64_t q0 = 0; q0 < n;) {
        int64_t m = 1;
        while (m < step && q0 + m < n && c->if_off[(size_t)(q0 + m + 1)] - c->if_off[(size_t)q0] <= INFL_CHUNK_BLOCKS) m++;
        const int64_t o0 = c->if_off[(size_t)q0], nb = c->if_off[(size_t)(q0 + m)] - o0;
        items.clear();
        for (int64_t q = 0; q < m; q++) {
            const int64_t cnt = c->if_off[(size_t)(q0 + q + 1)] - c->if_off[(size_t)(q0 + q)];
            for (int64_t k = 0; k < cnt; k += INFL_BLOCKS)
                items.push_back(InflItem{c->if_first[(size_t)(q0 + q)] + k, c->if_off[(size_t)(q0 + q)] - o0 + k, (int32_t)q, 0});
        }
        HIP_TRY(c->sfs_T.ensure((size_t)m * per));
        HIP_TRY(c->sfs_ns.ensure((size_t)m * c->nA));
        HIP_TRY(c->if_rng.ensure((size_t)m * c->nA * 4));
        HIP_TRY(c->if_tmax.ensure((size_t)m));
        HIP_TRY(c->if_lin.ensure((size_t)m));
        HIP_TRY(c->if_items.ensure(items.size()));
        HIP_TRY(c->if_m.ensure((size_t)nb));
        HIP_TRY(c->if_contrib.ensure((size_t)nb));
        HIP_TRY(c->if_L.ensure((size_t)nb));
        HIP_TRY(c->if_blin.ensure((size_t)nb));
        if (!items.empty())
            HIP_TRY(hipMemcpyAsync(c->if_items.p, items.data(), items.size() * sizeof(InflItem), hipMemcpyHostToDevice, c->stream));
        S.tests = c->sfs_list.p + q0; S.T = c->sfs_T.p; S.ns = c->sfs_ns.p;
        Q.A = c->d_A.p; Q.nA = c->nA; Q.tests = S.tests; Q.n = m; Q.rng = c->if_rng.p;
        P.tests = S.tests; P.T = c->sfs_T.p; P.ns = c->sfs_ns.p; P.rng = c->if_rng.p; P.lin = c->if_lin.p; P.items = c->if_items.p;
        P.m_out = c->if_m.p; P.contrib = c->if_contrib.p; P.L = c->if_L.p; P.blin = c->if_blin.p;
        HIP_TRY(c->ifl.begin(c->stream));
        hipLaunchKernelGGL(surfaces_kernel, dim3((unsigned)(m * c->nA * nsl)), dim3(SURFS_THREADS), 0, c->stream, S);
        hipLaunchKernelGGL(influence_range_kernel, dim3((unsigned)((m * c->nA + wpb - 1) / wpb)), dim3(INFL_THREADS), 0, c->stream, Q);
        hipLaunchKernelGGL(influence_argmax_kernel, dim3((unsigned)m), dim3(INFL_THREADS), 0, c->stream, (const double *)c->sfs_T.p,
                           (int64_t)per, c->if_tmax.p, c->if_lin.p);
        if (!items.empty())
            hipLaunchKernelGGL(influence_kernel, dim3((unsigned)items.size()), dim3(INFL_THREADS), 0, c->stream, P);
        HIP_TRY(hipGetLastError());
        HIP_TRY(c->ifl.end(c->stream));
        h_ns.resize((size_t)m * c->nA);
        HIP_TRY(hipMemcpyAsync(c->if_h_tmax.data() + q0, c->if_tmax.p, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(c->if_h_lin.data() + q0, c->if_lin.p, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(h_ns.data(), c->sfs_ns.p, (size_t)m * c->nA * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        if (nb) {
            HIP_TRY(hipMemcpyAsync(c->if_h_m.data() + o0, c->if_m.p, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(c->if_h_contrib.data() + o0, c->if_contrib.p, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(c->if_h_L.data() + o0, c->if_L.p, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(c->if_h_blin.data() + o0, c->if_blin.p, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(c->ifl.read());
        total_ms += c->ifl.ms;
        for (int64_t q = 0; q < m; q++) c->if_h_ns[(size_t)(q0 + q)] = h_ns[(size_t)q * c->nA + iAmin];
        q0 += m;
    }
    c->ifl.ms = total_ms;        // the call's figure: its chunks' kernels, the surfaces among them
    c->if_have = true;
    return BMX_OK;
}

int bmx_ctx_influence_count(bmx_ctx *c, int64_t *n_windows, int64_t *first_block, int64_t *offset) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    if (!c->if_have) return fail(BMX_E_STATE, "no influence call yet");
    const size_t n = c->if_first.size();
    if (n_windows) *n_windows = (int64_t)n;
    if (first_block) std::copy(c->if_first.begin(), c->if_first.end(), first_block);
    if (offset) std::copy(c->if_off.begin(), c->if_off.end(), offset);
    return BMX_OK;
}

int bmx_ctx_fetch_influence(bmx_ctx *c, double *t_max, int32_t *lin, int32_t *ns_min, int32_t *m, double *contrib, double *L,
                            int32_t *block_lin) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    if (!c->if_have) return fail(BMX_E_STATE, "no influence call yet");
    if (t_max) std::copy(c->if_h_tmax.begin(), c->if_h_tmax.end(), t_max);
    if (lin) std::copy(c->if_h_lin.begin(), c->if_h_lin.end(), lin);
    if (ns_min) std::copy(c->if_h_ns.begin(), c->if_h_ns.end(), ns_min);
    if (m) std::copy(c->if_h_m.begin(), c->if_h_m.end(), m);
    if (contrib) std::copy(c->if_h_contrib.begin(), c->if_h_contrib.end(), contrib);
    if (L) std::copy(c->if_h_L.begin(), c->if_h_L.end(), L);
    if (block_lin) std::copy(c->if_h_blin.begin(), c->if_h_blin.end(), block_lin);
    return BMX_OK;
}

int bmx_ctx_influence_ms(bmx_ctx *c, double *ms) {
    if (!c || !ms) return fail(BMX_E_INVALID, "NULL argument");
    if (!c->if_have) return fail(BMX_E_STATE, "no influence call yet");
    *ms = c->ifl.ms;
    return BMX_OK;
}

int bmx_ctx_fit(bmx_ctx *c, int64_t n, const int32_t *tests, const int32_t *lin, const double *gw, const int32_t *cls, int32_t F,
                const double *edges, int32_t D, int32_t *O_out, double *Esel_out, double *Eneu_out, int32_t *skipped_out) {
    const bool cells_ok = F >= 1 && D >= 1 && (int64_t)D * F <= BMX_FIT_MAX_CELLS;
    int rc = list_ready(c, "fit", n, cells_ok ? nullptr : "F >= 1, D >= 1 and D * F <= BMX_FIT_MAX_CELLS are needed",
                        !tests || !lin || !gw || !cls || (D > 1 && !edges) || !O_out || !Esel_out || !Eneu_out);
    if (rc) return rc;
    ChromSlot *s = c->cur;
    if (n > 0) {
        for (int32_t k = 0; k + 1 < D; k++)
            if (!(edges[k] - edges[k] == 0.0) || !(edges[k] > (k ? edges[k - 1] : 0.0)))
                return fail(BMX_E_INVALID, "fit: the edges must be finite, > 0 and strictly ascending");
        for (int r = 0; r < c->rows; r++) {
            if (cls[r] < 0 || cls[r] >= F) return fail(BMX_E_INVALID, "fit: a class outside [0, F) at row " + std::to_string(r));
            if (!(gw[r] >= 0.0 && gw[r] <= 1.0)) return fail(BMX_E_INVALID, "fit: gw outside [0, 1] at row " + std::to_string(r));
        }
    }
    const int64_t points = (int64_t)c->nA * c->npairs;
    for (int64_t q = 0; q < n; q++) {
        if (tests[q] < 0 || tests[q] >= s->M) return fail(BMX_E_INVALID, "fit: test site index out of range at entry " + std::to_string(q));
        if (lin[q] >= points) return fail(BMX_E_INVALID, "fit: grid point outside the model's grids at entry " + std::to_string(q));
    }
    c->ft.ms = 0.0;
    if (n == 0) return BMX_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t cells = (size_t)D * F, tab = (size_t)c->n_sizes * (F + 1) * 3;       // doubles of one window's prologue sums
    const bool in_lds = tab * sizeof(double) <= (size_t)BMX_FIT_LDS_BYTES && c->variant != 1;
    // a chunk's outputs stay at or below 64 MiB, its workspace (if any) at or below BMX_SURFACES_CHUNK_BYTES
    int64_t step = std::max<int64_t>((64LL << 20) / (int64_t)(cells * 20), 1);
    if (!in_lds) step = std::min(step, std::max<int64_t>(BMX_SURFACES_CHUNK_BYTES / (int64_t)(tab * sizeof(double)), 1));
    step = std::min(step, n);
    if ((rc = upload(c->sfs_list, tests, (size_t)n, c->stream))) return rc;
    if ((rc = upload(c->ft_lin, lin, (size_t)n, c->stream))) return rc;
    if ((rc = upload(c->ft_gw, gw, (size_t)c->rows, c->stream))) return rc;
    if ((rc = upload(c->ft_cls, cls, (size_t)c->rows, c->stream))) return rc;
    if ((rc = upload(c->ft_edges, edges, (size_t)(D - 1), c->stream))) return rc;
    HIP_TRY(c->ft_O.ensure((size_t)step * cells));
    HIP_TRY(c->ft_Es.ensure((size_t)step * cells));
    HIP_TRY(c->ft_En.ensure((size_t)step * cells));
    HIP_TRY(c->ft_skip.ensure((size_t)step));
    if (!in_lds) HIP_TRY(c->ft_ws.ensure((size_t)step * tab));
    FitParams P;
    P.sites = site_view(s); P.win = window_view(c, s);
    P.R = c->d_R.p; P.rows = c->rows; P.npairs = c->npairs; P.A = c->d_A.p;
    P.row_off = c->d_row_off.p; P.n_sizes = c->n_sizes;
    P.gw = c->ft_gw.p; P.cls = c->ft_cls.p; P.F = F; P.edges = c->ft_edges.p; P.D = D;
    P.ws = in_lds ? nullptr : c->ft_ws.p;
    P.O = c->ft_O.p; P.Esel = c->ft_Es.p; P.Eneu = c->ft_En.p; P.skipped = c->ft_skip.p;
    double total = 0.0;
    for (int64_t q0 = 0; q0 < n; q0 += step) {
        const int64_t m = std::min(step, n - q0);
        P.tests = c->sfs_list.p + q0; P.lin = c->ft_lin.p + q0;
        HIP_TRY(c->ft.begin(c->stream));
        if (in_lds) hipLaunchKernelGGL(fit_kernel<true>, dim3((unsigned)m), dim3(FIT_THREADS), tab * sizeof(double), c->stream, P);
        else hipLaunchKernelGGL(fit_kernel<false>, dim3((unsigned)m), dim3(FIT_THREADS), 0, c->stream, P);
        HIP_TRY(hipGetLastError());
        HIP_TRY(c->ft.end(c->stream));
        HIP_TRY(hipMemcpyAsync(O_out + (size_t)q0 * cells, c->ft_O.p, (size_t)m * cells * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(Esel_out + (size_t)q0 * cells, c->ft_Es.p, (size_t)m * cells * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(Eneu_out + (size_t)q0 * cells, c->ft_En.p, (size_t)m * cells * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (skipped_out)
            HIP_TRY(hipMemcpyAsync(skipped_out + q0, c->ft_skip.p, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(c->ft.read());
        total += c->ft.ms;
    }
    c->ft.ms = total;        // the call's figure: its chunks' kernels
    return BMX_OK;
}

int bmx_ctx_fit_ms(bmx_ctx *c, double *ms) {
    if (!c || !ms) return fail(BMX_E_INVALID, "NULL argument");
    return c->ft.get(ms, "no fit call yet");
}

int bmx_ctx_cond_surfaces(bmx_ctx *c, int64_t n, const int32_t *tests, const int32_t *cond_test, const int32_t *cond_lin, double *T_out,
                          int32_t *nsites_out, int32_t *nshared_out, double *tmax_out, int32_t *lin_out) {
    int rc;
    if ((rc = list_ready(c, "cond_surfaces", n, nullptr, !tests || !cond_test || !cond_lin))) return rc;
    if (n == 0) { c->cs.ms = 0.0; return BMX_OK; }
    ChromSlot *s = c->cur;
    const size_t per = (size_t)c->nA * c->npairs;
    // the conditioning entries up to the first test site index out of range: listed_surfaces refuses that entry, in its place in
    // the order of one pass over the entries, and nothing has touched the device by then
    int64_t q = 0;
    for (; q < n && tests[q] >= 0 && tests[q] < s->M; q++) {
        if (cond_test[q] < -1 || cond_test[q] >= s->M)
            return fail(BMX_E_INVALID, "cond_surfaces: conditioning test site index out of range at entry " + std::to_string(q));
        if (cond_lin[q] >= 0 && (size_t)cond_lin[q] >= per)
            return fail(BMX_E_INVALID, "cond_surfaces: conditioning grid index out of range at entry " + std::to_string(q));
    }
    if (q == n) {
        HIP_TRY(hipSetDevice(c->device));
        if ((rc = upload(c->cs_ctest, cond_test, (size_t)n, c->stream))) return rc;
        if ((rc = upload(c->cs_clin, cond_lin, (size_t)n, c->stream))) return rc;
    }
    return listed_surfaces(c, "cond_surfaces", n, tests, c->cs, [&](const SurfsParams &S, int64_t q0, dim3 grid) {
        hipLaunchKernelGGL(cond_surfaces_kernel, grid, dim3(SURFS_THREADS), 0, c->stream, S, PairSide{c->cs_ctest.p + q0, c->cs_clin.p + q0});
    }, T_out, nsites_out, nshared_out, tmax_out, lin_out);
}

int bmx_ctx_cond_surfaces_ms(bmx_ctx *c, double *ms) {
    if (!c || !ms) return fail(BMX_E_INVALID, "NULL argument");
    return c->cs.get(ms, "no cond_surfaces call yet");
}

int bmx_ctx_baseline_reset(bmx_ctx *c) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->has_sites) return fail(BMX_E_STATE, "sites must be set before baseline_reset");
    HIP_TRY(hipSetDevice(c->device));
    s->bl_have = false;
    HIP_TRY(s->bl_d.ensure((size_t)s->N));
    HIP_TRY(s->bl_cnt.ensure((size_t)s->N));
    HIP_TRY(hipMemsetAsync(s->bl_d.p, 0, (size_t)s->N * sizeof(double), c->stream));          // (all bits 0: 0.0)
    HIP_TRY(hipMemsetAsync(s->bl_cnt.p, 0, (size_t)s->N * sizeof(int32_t), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    s->bl_have = true;
    return BMX_OK;
}

int bmx_ctx_baseline_add(bmx_ctx *c, int32_t test, int32_t lin, int64_t *first, int64_t *last, int32_t *n_written) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->ready_to_scan(c)) return fail(BMX_E_STATE, "model, sites and tests must be set before baseline_add");
    if (!s->bl_have) return fail(BMX_E_STATE, "baseline_add: no baseline (bmx_ctx_baseline_reset) on this slot's sites");
    if (test < 0 || test >= s->M) return fail(BMX_E_INVALID, "baseline_add: test site index out of range");
    if (lin < 0 || (int64_t)lin >= (int64_t)c->nA * c->npairs) return fail(BMX_E_INVALID, "baseline_add: grid index out of range");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->bs_out.ensure(3));
    BaseAddParams P;
    P.sites = site_view(s); P.win = window_view(c, s);
    P.Rt = c->d_Rt.p; P.NP = c->NP;
    P.t = test; P.A = c->h_A[(size_t)(lin / c->npairs)]; P.p = lin % c->npairs;
    P.d = s->bl_d.p; P.cnt = s->bl_cnt.p; P.out = c->bs_out.p;
    const int64_t grid = std::min<int64_t>(std::max<int64_t>((s->N + SURFS_THREADS - 1) / SURFS_THREADS, 1), BASE_ADD_GRID_MAX);
    hipLaunchKernelGGL(baseline_add_kernel, dim3((unsigned)grid), dim3(SURFS_THREADS), 0, c->stream, P);
    HIP_TRY(hipGetLastError());
    int64_t out[3] = {0, -1, 0};
    HIP_TRY(hipMemcpyAsync(out, c->bs_out.p, sizeof(out), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (first) *first = out[0];
    if (last) *last = out[1];
    if (n_written) *n_written = (int32_t)out[2];
    return BMX_OK;
}

int bmx_ctx_baseline_fetch(bmx_ctx *c, double *d_out, int32_t *cnt_out) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->has_sites || !s->bl_have) return fail(BMX_E_STATE, "baseline_fetch: no baseline (bmx_ctx_baseline_reset) on this slot's sites");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(download(d_out, (const double *)s->bl_d.p, (size_t)s->N));
    HIP_TRY(download(cnt_out, (const int32_t *)s->bl_cnt.p, (size_t)s->N));
    return BMX_OK;
}

int bmx_ctx_base_surfaces(bmx_ctx *c, int64_t n, const int32_t *tests, double *T_out, int32_t *nsites_out, int32_t *nshared_out,
                          double *tmax_out, int32_t *lin_out) {
    int rc;
    if ((rc = list_ready(c, "base_surfaces", n, nullptr, !tests))) return rc;
    ChromSlot *s = c->cur;
    if (!s->bl_have) return fail(BMX_E_STATE, "base_surfaces: no baseline (bmx_ctx_baseline_reset) on this slot's sites");
    if (n == 0) { c->bs.ms = 0.0; return BMX_OK; }
    return listed_surfaces(c, "base_surfaces", n, tests, c->bs, [&](const SurfsParams &S, int64_t, dim3 grid) {
        hipLaunchKernelGGL(base_surfaces_kernel, grid, dim3(SURFS_THREADS), 0, c->stream, S, BaselineSide{s->bl_d.p, s->bl_cnt.p});
    }, T_out, nsites_out, nshared_out, tmax_out, lin_out);
}

int bmx_ctx_base_surfaces_ms(bmx_ctx *c, double *ms) {
    if (!c || !ms) return fail(BMX_E_INVALID, "NULL argument");
    return c->bs.get(ms, "no base_surfaces call yet");
}

}  // extern "C"

/* ---- refinement (ballermixplus_amd/refine.py holds the definition: bounds, initial steps, the compass search) ---- */

namespace {

// The model's part of a refinement launch: grids, each grid value's coordinate and initial step, hull, free coordinates
// (uploaded into c->rf_grid: cu[nA], cv[nab], h0u[nA], h0x[nx], h0v[nab]).
int refine_setup(bmx_ctx *c, ChromSlot *s, RefineParams &P, int max_rounds) {
    const int nA = c->nA, nx = c->nx, nab = c->nab;
    std::vector<double> cu(nA), cv(nab), h0u(nA), h0x(nx), h0v(nab);
    for (int i = 0; i < nA; i++) cu[i] = std::log(c->h_A[i]);
    for (int i = 0; i < nab; i++) cv[i] = std::log(c->h_ab[i]);
    auto axis = [&](const std::vector<double> &vals, std::vector<double> &h0, int k) {
        std::vector<double> S(vals);
        std::sort(S.begin(), S.end());
        S.erase(std::unique(S.begin(), S.end()), S.end());
        P.fr[k] = S.size() >= 2;
        P.lo[k] = S.front();
        P.hi[k] = S.back();
        for (size_t i = 0; i < vals.size(); i++) {
            const size_t p = (size_t)(std::lower_bound(S.begin(), S.end(), vals[i]) - S.begin());
            double h = INFINITY;
            if (p > 0) h = std::min(h, S[p] - S[p - 1]);
            if (p + 1 < S.size()) h = std::min(h, S[p + 1] - S[p]);
            h0[i] = S.size() >= 2 ? 0.5 * h : 0.0;
        }
    };
    axis(cu, h0u, 0);
    axis(c->h_x, h0x, 1);
    axis(cv, h0v, 2);
    P.tol[0] = 1e-4; P.tol[1] = 1e-5; P.tol[2] = 1e-4;
    std::vector<double> all;
    for (auto *v : {&cu, &cv, &h0u, &h0x, &h0v}) all.insert(all.end(), v->begin(), v->end());
    int rc;
    if ((rc = upload(c->rf_grid, (const double *)all.data(), all.size(), c->stream))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));      // `all` goes out of scope here
    const double *d = c->rf_grid.p;
    P.cu = d; P.cv = d + nA; P.h0u = d + nA + nab; P.h0x = d + 2 * nA + nab; P.h0v = d + 2 * nA + nab + nx;
    P.stat = c->stat; P.min_count = c->min_count; P.n_sizes = c->n_sizes; P.rows = c->rows;
    P.sizes = c->d_sizes.p; P.row_off = c->d_row_off.p; P.g = c->d_g.p; P.prop = c->d_prop.p;
    P.gA = c->d_A.p; P.gx = c->d_x.p; P.gab = c->d_abeta.p; P.npairs = c->npairs; P.nab = nab;
    P.max_rounds = max_rounds;
    P.sites = site_view(s); P.win = window_view(c, s);
    P.M = s->M;
    P.list = nullptr; P.count = nullptr; P.lin = nullptr; P.clr = nullptr; P.pA = P.px = P.pab = nullptr;
    P.o_A = P.o_x = P.o_ab = nullptr; P.o_rounds = nullptr;
    return BMX_OK;
}

// Workspace (LDS or slab) of a launch of refine_kernel or support_kernel over `work` workgroups at most: the workgroups to launch
int refine_workspace(bmx_ctx *c, RefineParams &P, int64_t work, int64_t &blocks_out) {
    const int64_t ws = ((int64_t)c->rows * (REFINE_TABS * 8 + 4 + 1) + 15) / 16 * 16;
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    int64_t blocks = std::min<int64_t>(std::max<int64_t>(work, 1), std::min<int64_t>(REFINE_GRID_MAX, 8LL * std::max(cus, 1)));
    P.ws_bytes = ws;
    P.ws_lds = ws <= REFINE_LDS_WS;
    if (!P.ws_lds) {
        blocks = std::max<int64_t>(1, std::min<int64_t>(blocks, (512LL << 20) / ws));
        HIP_TRY(c->rf_slab.ensure((size_t)(blocks * ws)));
        P.slab = c->rf_slab.p;
    } else {
        P.slab = nullptr;
    }
    blocks_out = blocks;
    return BMX_OK;
}

// ... and the launch of a kernel that works in it (refine_kernel, support_kernel, boot_kernel) with its parameters Q, whose
// RefineParams are P
template <class Params>
int launch_ws(bmx_ctx *c, void (*kernel)(Params), Params &Q, RefineParams &P, int64_t work) {
    int64_t blocks = 0;
    int rc = refine_workspace(c, P, work, blocks);
    if (rc) return rc;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(REFINE_THREADS), P.ws_lds ? (size_t)P.ws_bytes : 0, c->stream, Q);
    HIP_TRY(hipGetLastError());
    return BMX_OK;
}

// The points of a point evaluation (bmx_ctx_eval_points, bmx_ctx_eval_points_weighted): one (A, x, abeta) per test site of the
// slot, checked; then, with the stream idle, P set up for them, the points in c->rf_pts and room for a value each in c->rf_pT
int upload_points(bmx_ctx *c, const char *who, const double *A, const double *x, const double *abeta, RefineParams &P) {
    ChromSlot *s = c->cur;
    const int64_t M = s->M;
    for (int64_t t = 0; t < M; t++)
        if (!(A[t] > 0.0) || !(x[t] > 0.0 && x[t] < 1.0) || !(abeta[t] > 0.0) || !std::isfinite(A[t]) || !std::isfinite(abeta[t]))
            return fail(BMX_E_INVALID, std::string(who) + ": A > 0, 0 < x < 1 and alpha_beta > 0 (finite) at every point");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int rc = refine_setup(c, s, P, 0);
    if (rc) return rc;
    HIP_TRY(c->rf_pts.ensure((size_t)3 * M));
    const double *src[3] = {A, x, abeta};
    for (int k = 0; k < 3; k++)
        HIP_TRY(hipMemcpyAsync(c->rf_pts.p + k * M, src[k], (size_t)M * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c->rf_pT.ensure((size_t)M));
    P.pA = c->rf_pts.p; P.px = c->rf_pts.p + M; P.pab = c->rf_pts.p + 2 * M;
    return BMX_OK;
}

}  // namespace

extern "C" {

int bmx_ctx_eval_points(bmx_ctx *c, const double *A, const double *x, const double *abeta, double *T_out, int32_t *nsites_out) {
    if (!c || !A || !x || !abeta || !T_out) return fail(BMX_E_INVALID, "NULL argument");
    ChromSlot *s = c->cur;
    if (!s->ready_to_scan(c)) return fail(BMX_E_STATE, "model, sites and tests must be set before eval_points");
    const int64_t M = s->M;
    RefineParams P;
    int rc = upload_points(c, "eval_points", A, x, abeta, P);
    if (rc) return rc;
    HIP_TRY(c->rf_pns.ensure((size_t)M));
    P.o_clr = c->rf_pT.p; P.o_ns = c->rf_pns.p;
    if ((rc = launch_ws(c, refine_kernel, P, P, M))) return rc;
    HIP_TRY(hipMemcpyAsync(T_out, c->rf_pT.p, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (nsites_out) HIP_TRY(hipMemcpyAsync(nsites_out, c->rf_pns.p, (size_t)M * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BMX_OK;
}

int bmx_ctx_refine(bmx_ctx *c, double min_clr) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!c->has_model || !s->has_results()) return fail(BMX_E_STATE, "refine: no scan results (scan the slot first)");
    if (min_clr != min_clr) return fail(BMX_E_INVALID, "refine: min_clr is NaN");
    if (c->rf_at_peaks && !(s->pk_have && s->pk_scan && s->pk_seq == s->scan_seq && s->pk_M == s->M))
        return fail(BMX_E_INVALID, "refine: restricted to the apexes (bmx_ctx_refine_at_peaks), but the slot has no peak call on its last scan: "
                                   "call bmx_ctx_peaks after the scan");
    HIP_TRY(hipSetDevice(c->device));
    const int64_t M = s->M;
    RefineParams P;
    int rc = refine_setup(c, s, P, 256);
    if (rc) return rc;
    HIP_TRY(s->rf_clr.ensure((size_t)M)); HIP_TRY(s->rf_A.ensure((size_t)M)); HIP_TRY(s->rf_x.ensure((size_t)M));
    HIP_TRY(s->rf_ab.ensure((size_t)M)); HIP_TRY(s->rf_ns.ensure((size_t)M)); HIP_TRY(s->rf_rounds.ensure((size_t)M));
    HIP_TRY(c->rf_flag.ensure((size_t)M));
    HIP_TRY(c->rf_pre.ensure((size_t)M + 1));
    HIP_TRY(c->rf_list.ensure((size_t)M));
    RefineInitParams Q;
    Q.clr = s->clr.p; Q.lin = s->lin.p; Q.nsites = s->nsites.p;
    Q.apex = c->rf_at_peaks ? s->pk_flag.p : nullptr;
    Q.gA = c->d_A.p; Q.gx = c->d_x.p; Q.gab = c->d_abeta.p; Q.npairs = c->npairs; Q.nab = c->nab;
    Q.M = M; Q.min_clr = min_clr; Q.flag = c->rf_flag.p;
    Q.o_clr = s->rf_clr.p; Q.o_A = s->rf_A.p; Q.o_x = s->rf_x.p; Q.o_ab = s->rf_ab.p; Q.o_ns = s->rf_ns.p; Q.o_rounds = s->rf_rounds.p;
    hipLaunchKernelGGL(refine_init_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, c->stream, Q);
    HIP_TRY(hipGetLastError());
    HIP_TRY(flag_prefix(c, c->rf_flag.p, M));
    HIP_TRY(flag_compact(c, c->rf_flag.p, M, c->rf_list.p));
    P.list = c->rf_list.p; P.count = c->rf_pre.p + M;
    P.lin = s->lin.p; P.clr = s->clr.p;
    P.o_clr = s->rf_clr.p; P.o_A = s->rf_A.p; P.o_x = s->rf_x.p; P.o_ab = s->rf_ab.p; P.o_ns = s->rf_ns.p; P.o_rounds = s->rf_rounds.p;
    if ((rc = launch_ws(c, refine_kernel, P, P, M))) return rc;
    s->rf_have = true;
    s->rf_seq = s->scan_seq;
    s->release_support();
    s->release_boot();
    return BMX_OK;
}

int bmx_ctx_fetch_refined(bmx_ctx *c, double *clr, double *A, double *x, double *abeta, int32_t *nsites, int32_t *rounds) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->rf_have) return fail(BMX_E_STATE, "no refinement of the slot's test sites: call bmx_ctx_refine after a scan");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t M = (size_t)s->M;
    HIP_TRY(download(clr, s->rf_clr.p, M)); HIP_TRY(download(A, s->rf_A.p, M)); HIP_TRY(download(x, s->rf_x.p, M));
    HIP_TRY(download(abeta, s->rf_ab.p, M)); HIP_TRY(download(nsites, s->rf_ns.p, M)); HIP_TRY(download(rounds, s->rf_rounds.p, M));
    return BMX_OK;
}

int bmx_ctx_support(bmx_ctx *c, double drop, double min_clr) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->has_refinement_of_last_scan(c))
        return fail(BMX_E_STATE, "support: no refinement of the slot's last scan (call bmx_ctx_refine after the scan)");
    if (!(drop > 0.0) || !std::isfinite(drop)) return fail(BMX_E_INVALID, "support: drop must be finite and > 0");
    if (min_clr != min_clr) return fail(BMX_E_INVALID, "support: min_clr is NaN");
    const int64_t M = s->M, nt = M * SUPPORT_TASKS;
    if (nt > INT32_MAX) return fail(BMX_E_LIMIT, "support: more than 2^31 tasks");
    HIP_TRY(hipSetDevice(c->device));
    SupportParams Q;
    int rc = refine_setup(c, s, Q.P, 256);
    if (rc) return rc;
    const double tol[3] = {1e-3, 1e-4, 1e-3};       // support.py: NUIS_TOL, END_TOL
    for (int k = 0; k < 3; k++) { Q.P.tol[k] = tol[k]; Q.end_tol[k] = tol[k]; }
    Q.drop = drop;
    HIP_TRY(s->sp_d.ensure((size_t)nt * SUPPORT_ND));
    HIP_TRY(s->sp_i.ensure((size_t)nt * SUPPORT_NI));
    HIP_TRY(c->rf_flag.ensure((size_t)nt));
    HIP_TRY(c->rf_pre.ensure((size_t)nt + 1));
    HIP_TRY(c->rf_list.ensure((size_t)nt));
    SupportInitParams I;
    I.clr = s->rf_clr.p; I.rounds = s->rf_rounds.p;
    for (int k = 0; k < 3; k++) I.fr[k] = Q.P.fr[k];
    I.M = M; I.min_clr = min_clr; I.flag = c->rf_flag.p; I.o_d = s->sp_d.p; I.o_i = s->sp_i.p;
    hipLaunchKernelGGL(support_init_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, c->stream, I);
    HIP_TRY(hipGetLastError());
    HIP_TRY(flag_prefix(c, c->rf_flag.p, nt));
    HIP_TRY(flag_compact(c, c->rf_flag.p, nt, c->rf_list.p));
    Q.P.lin = s->lin.p; Q.P.clr = s->clr.p;
    Q.list = c->rf_list.p; Q.count = c->rf_pre.p + nt;
    Q.rA = s->rf_A.p; Q.rx = s->rf_x.p; Q.rab = s->rf_ab.p;
    Q.o_d = s->sp_d.p; Q.o_i = s->sp_i.p;
    if ((rc = launch_ws(c, support_kernel, Q, Q.P, nt))) return rc;
    s->sp_have = true;
    return BMX_OK;
}

int bmx_ctx_fetch_support(bmx_ctx *c, double *end, double *witness, double *witness_T, double *outside, double *outside_T,
                          int32_t *censored, double *T_star, double *T_best, int32_t *rounds, int32_t *evals) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->sp_have || !s->has_refinement_of_last_scan(c))      // a new scan drops them, as it drops the bootstrap
        return fail(BMX_E_STATE, "no support intervals of the slot's test sites: call bmx_ctx_support after bmx_ctx_refine");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t M = (size_t)s->M, nt = M * SUPPORT_TASKS;
    std::vector<double> d(nt * SUPPORT_ND);
    std::vector<int32_t> iv(nt * SUPPORT_NI);
    HIP_TRY(hipMemcpy(d.data(), s->sp_d.p, d.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(iv.data(), s->sp_i.p, iv.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t q = 0; q < nt; q++) {
        const double *od = &d[q * SUPPORT_ND];
        const int32_t *oi = &iv[q * SUPPORT_NI];
        if (end) end[q] = od[0];
        for (int j = 0; j < 3; j++) {
            if (witness) witness[q * 3 + j] = od[1 + j];
            if (outside) outside[q * 3 + j] = od[5 + j];
        }
        if (witness_T) witness_T[q] = od[4];
        if (outside_T) outside_T[q] = od[8];
        if (censored) censored[q] = oi[0];
        if (rounds) rounds[q] = oi[1];
        if (evals) evals[q] = oi[2];
    }
    for (size_t t = 0; t < M; t++) {
        double ts = NAN, tb = NAN;
        for (size_t q = t * SUPPORT_TASKS; q < (t + 1) * SUPPORT_TASKS; q++) {
            if (iv[q * SUPPORT_NI + 1] < 0) continue;
            if (ts != ts) ts = d[q * SUPPORT_ND + 9];
            if (tb != tb || d[q * SUPPORT_ND + 10] > tb) tb = d[q * SUPPORT_ND + 10];
        }
        if (T_star) T_star[t] = ts;
        if (T_best) T_best[t] = tb;
    }
    return BMX_OK;
}

}  // extern "C"

/* ---- block bootstrap (ballermixplus_amd/boot.py holds the definition: weights, objective, one replicate) ---- */

extern "C" {

int bmx_ctx_eval_points_weighted(bmx_ctx *c, uint64_t key, int64_t block, const double *A, const double *x, const double *abeta,
                                 double *T_out, int64_t *wsum_out) {
    if (!c || !A || !x || !abeta || !T_out) return fail(BMX_E_INVALID, "NULL argument");
    ChromSlot *s = c->cur;
    if (!s->ready_to_scan(c)) return fail(BMX_E_STATE, "model, sites and tests must be set before eval_points_weighted");
    if (block < 1) return fail(BMX_E_INVALID, "eval_points_weighted: block must be >= 1");
    const int64_t M = s->M;
    BootParams Q;
    int rc = upload_points(c, "eval_points_weighted", A, x, abeta, Q.P);
    if (rc) return rc;
    HIP_TRY(c->bt_pws.ensure((size_t)M));
    HIP_TRY(c->bt_keys.ensure(1));
    HIP_TRY(hipMemcpyAsync(c->bt_keys.p, &key, sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    Q.keys = c->bt_keys.p; Q.R = 1; Q.block = block;
    Q.list = nullptr; Q.count = nullptr; Q.rA = Q.rx = Q.rab = nullptr;
    Q.o_A = Q.o_x = Q.o_ab = Q.o_Tc = nullptr; Q.o_rounds = nullptr;
    Q.o_T = c->rf_pT.p; Q.o_wsum = c->bt_pws.p;
    if ((rc = launch_ws(c, boot_kernel, Q, Q.P, M))) return rc;
    HIP_TRY(hipMemcpyAsync(T_out, c->rf_pT.p, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (wsum_out) HIP_TRY(hipMemcpyAsync(wsum_out, c->bt_pws.p, (size_t)M * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));     // (also: `key` leaves scope here)
    return BMX_OK;
}

int bmx_ctx_boot(bmx_ctx *c, const uint64_t *keys, int32_t R, int64_t block, double min_clr) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->has_refinement_of_last_scan(c))
        return fail(BMX_E_STATE, "boot: no refinement of the slot's last scan (call bmx_ctx_refine after the scan)");
    if (!keys || R < 1) return fail(BMX_E_INVALID, "boot: at least one replicate key is needed");
    if (block < 1) return fail(BMX_E_INVALID, "boot: block must be >= 1");
    if (min_clr != min_clr) return fail(BMX_E_INVALID, "boot: min_clr is NaN");
    HIP_TRY(hipSetDevice(c->device));
    const int64_t M = s->M;
    s->release_boot();
    BootParams Q;
    int rc = refine_setup(c, s, Q.P, 256);
    if (rc) return rc;
    // the selection: its count is needed on the host to size the results (this waits for the refinement)
    HIP_TRY(c->rf_flag.ensure((size_t)M));
    HIP_TRY(c->rf_pre.ensure((size_t)M + 1));
    HIP_TRY(s->bt_win.ensure((size_t)M));
    hipLaunchKernelGGL(boot_init_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, c->stream, (const double *)s->rf_clr.p,
                       (const int32_t *)s->rf_rounds.p, M, min_clr, c->rf_flag.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(flag_prefix(c, c->rf_flag.p, M));
    HIP_TRY(flag_compact(c, c->rf_flag.p, M, s->bt_win.p));
    int64_t nsel = 0;
    HIP_TRY(hipMemcpyAsync(&nsel, c->rf_pre.p + M, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (nsel * (int64_t)R > BMX_BOOT_MAX_RESULTS)
        return fail(BMX_E_LIMIT, "boot: " + std::to_string(nsel) + " windows x " + std::to_string(R) + " replicates exceed " +
                    std::to_string((long long)BMX_BOOT_MAX_RESULTS) + " results: raise --bootMin (min_clr) or lower the replicates");
    const size_t nt = (size_t)nsel * (size_t)R;
    HIP_TRY(s->bt_A.ensure(nt)); HIP_TRY(s->bt_x.ensure(nt)); HIP_TRY(s->bt_ab.ensure(nt));
    HIP_TRY(s->bt_T.ensure(nt)); HIP_TRY(s->bt_Tc.ensure(nt)); HIP_TRY(s->bt_rounds.ensure(nt));
    if ((rc = upload(c->bt_keys, keys, (size_t)R, c->stream))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));       // the caller's keys may go away after the call
    s->bt_nsel = nsel; s->bt_R = R; s->bt_seq = s->scan_seq;
    if (nt) {
        Q.P.lin = s->lin.p; Q.P.clr = s->clr.p;
        Q.keys = c->bt_keys.p; Q.R = R; Q.block = block;
        Q.list = s->bt_win.p; Q.count = c->rf_pre.p + M;
        Q.rA = s->rf_A.p; Q.rx = s->rf_x.p; Q.rab = s->rf_ab.p;
        Q.o_A = s->bt_A.p; Q.o_x = s->bt_x.p; Q.o_ab = s->bt_ab.p; Q.o_T = s->bt_T.p; Q.o_Tc = s->bt_Tc.p;
        Q.o_rounds = s->bt_rounds.p; Q.o_wsum = nullptr;
        if ((rc = launch_ws(c, boot_kernel, Q, Q.P, (int64_t)nt))) return rc;
    }
    s->bt_have = true;
    return BMX_OK;
}

int bmx_ctx_boot_count(bmx_ctx *c, int64_t *n_sel, int32_t *R) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->bt_have || s->bt_seq != s->scan_seq)
        return fail(BMX_E_STATE, "no bootstrap of the slot's last scan: call bmx_ctx_boot after bmx_ctx_refine");
    if (n_sel) *n_sel = s->bt_nsel;
    if (R) *R = s->bt_R;
    return BMX_OK;
}

int bmx_ctx_fetch_boot(bmx_ctx *c, int32_t *window, double *A, double *x, double *abeta, double *T, double *T_centre,
                       int32_t *rounds) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->bt_have || s->bt_seq != s->scan_seq)
        return fail(BMX_E_STATE, "no bootstrap of the slot's last scan: call bmx_ctx_boot after bmx_ctx_refine");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t n = (size_t)s->bt_nsel, nt = n * (size_t)s->bt_R;
    if (!nt) return BMX_OK;
    HIP_TRY(download(window, s->bt_win.p, n));
    HIP_TRY(download(A, s->bt_A.p, nt)); HIP_TRY(download(x, s->bt_x.p, nt)); HIP_TRY(download(abeta, s->bt_ab.p, nt));
    HIP_TRY(download(T, s->bt_T.p, nt)); HIP_TRY(download(T_centre, s->bt_Tc.p, nt)); HIP_TRY(download(rounds, s->bt_rounds.p, nt));
    return BMX_OK;
}

/* ---- sandwich (Godambe) pieces of listed windows (ballermixplus_amd/sandwich.py holds the definition) ---- */

int bmx_ctx_sandwich(bmx_ctx *c, int64_t n, const int32_t *tests, const double *A, const double *x, const double *abeta, int64_t block,
                     double hx, double hv, double *T_out, double *g_out, double *H_out, double *J_out, int32_t *nsites_out,
                     int32_t *nskipped_out, int32_t *nblocks_out) {
    int rc;
    const bool steps_ok = std::isfinite(hx) && hx > 0.0 && std::isfinite(hv) && hv > 0.0;
    const char *own = block < 1 ? "block < 1" : steps_ok ? nullptr : "the steps hx and hv must be finite and > 0";
    if ((rc = list_ready(c, "sandwich", n, own, !tests || !A || !x || !abeta))) return rc;
    if (n > BMX_SANDWICH_MAX_WINDOWS) return fail(BMX_E_LIMIT, "sandwich: more than BMX_SANDWICH_MAX_WINDOWS windows in one call");
    if (n == 0) { c->sw.ms = 0.0; return BMX_OK; }
    ChromSlot *s = c->cur;
    const double rv = std::exp(hv);                 // the C library's exp, once: the four shifted points are the host's
    // the five (x, alpha_beta) of entry q's columns, as every pass below forms them
    auto shifted = [&](int64_t q, double &xm, double &xp, double &am, double &ap) {
        xm = x[q] - hx; xp = x[q] + hx; am = abeta[q] / rv; ap = abeta[q] * rv;
    };
    for (int64_t q = 0; q < n; q++) {               // the whole list is judged before anything is launched or written
        if (tests[q] < 0 || tests[q] >= s->M) return fail(BMX_E_INVALID, "sandwich: test site index out of range at entry " + std::to_string(q));
        if (!(A[q] > 0.0) || !std::isfinite(A[q]) || !(abeta[q] > 0.0) || !std::isfinite(abeta[q]))
            return fail(BMX_E_INVALID, "sandwich: A and alpha_beta must be finite and > 0 at entry " + std::to_string(q));
        double xm, xp, am, ap;
        shifted(q, xm, xp, am, ap);
        if (!(xm > 0.0) || !(xp < 1.0))
            return fail(BMX_E_INVALID, "sandwich: 0 < x - hx and x + hx < 1 are needed at entry " + std::to_string(q));
        if (!(am > 0.0) || !std::isfinite(ap))
            return fail(BMX_E_INVALID, "sandwich: alpha_beta / exp(hv) and alpha_beta * exp(hv) must be finite and > 0 at entry " + std::to_string(q));
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    SandwichParams Q;
    if ((rc = refine_setup(c, s, Q.P, 0))) return rc;
    // chunks of at most BMX_SANDWICH_CHUNK_WINDOWS windows: list, points and outputs of one chunk on the host and on the device
    const int64_t step = std::min<int64_t>(BMX_SANDWICH_CHUNK_WINDOWS, n);
    std::vector<double> pts;                        // [7][step]: A, x, abeta, x - hx, x + hx, abeta / rv, abeta * rv
    try {
        pts.resize((size_t)7 * step);
    } catch (const std::bad_alloc &) {
        return fail(BMX_E_LIMIT, "sandwich: no host memory for one chunk's points");
    }
    HIP_TRY(c->sw_out.ensure((size_t)step * SANDWICH_VALS));
    HIP_TRY(c->sw_cnt.ensure((size_t)step * 3));
    HIP_TRY(c->sw_list.ensure((size_t)step));
    HIP_TRY(c->sw_pts.ensure((size_t)step * 7));
    Q.B = std::min(block, std::max<int64_t>(s->N, 1));           // i / B is 0 for every site either way
    Q.den_x = 2.0 * hx; Q.den_v = 2.0 * hv;
    Q.T = c->sw_out.p; Q.g = Q.T + step; Q.H = Q.g + 3 * step; Q.J = Q.H + 6 * step;
    Q.ns = c->sw_cnt.p; Q.nsk = Q.ns + step; Q.nb = Q.nsk + step;
    Q.tests = c->sw_list.p;
    const double *d = c->sw_pts.p;
    Q.pA = d; Q.px = d + step; Q.pab = d + 2 * step; Q.pxm = d + 3 * step; Q.pxp = d + 4 * step; Q.pabm = d + 5 * step; Q.pabp = d + 6 * step;
    const double ms_before = c->sw.ms;
    double total = 0.0;
    auto run = [&]() -> int {
        const hipMemcpyKind D2H = hipMemcpyDeviceToHost, H2D = hipMemcpyHostToDevice;
        for (int64_t q0 = 0; q0 < n; q0 += step) {
            const int64_t m = std::min(step, n - q0);
            for (int64_t q = 0; q < m; q++) {
                double xm, xp, am, ap;
                shifted(q0 + q, xm, xp, am, ap);
                const double row[7] = {A[q0 + q], x[q0 + q], abeta[q0 + q], xm, xp, am, ap};
                for (int k = 0; k < 7; k++) pts[(size_t)k * step + q] = row[k];
            }
            HIP_TRY(hipMemcpyAsync(c->sw_list.p, tests + q0, (size_t)m * sizeof(int32_t), H2D, c->stream));
            HIP_TRY(hipMemcpyAsync(c->sw_pts.p, pts.data(), pts.size() * sizeof(double), H2D, c->stream));
            Q.n = m;
            HIP_TRY(c->sw.begin(c->stream));
            int lrc = launch_ws(c, sandwich_kernel, Q, Q.P, m);
            if (lrc) return lrc;
            HIP_TRY(c->sw.end(c->stream));
            // each chunk goes back before the next is launched (and before its points are overwritten on the host)
            if (T_out) HIP_TRY(hipMemcpyAsync(T_out + q0, Q.T, (size_t)m * sizeof(double), D2H, c->stream));
            if (g_out) HIP_TRY(hipMemcpyAsync(g_out + q0 * 3, Q.g, (size_t)m * 3 * sizeof(double), D2H, c->stream));
            if (H_out) HIP_TRY(hipMemcpyAsync(H_out + q0 * 6, Q.H, (size_t)m * 6 * sizeof(double), D2H, c->stream));
            if (J_out) HIP_TRY(hipMemcpyAsync(J_out + q0 * 6, Q.J, (size_t)m * 6 * sizeof(double), D2H, c->stream));
            if (nsites_out) HIP_TRY(hipMemcpyAsync(nsites_out + q0, Q.ns, (size_t)m * sizeof(int32_t), D2H, c->stream));
            if (nskipped_out) HIP_TRY(hipMemcpyAsync(nskipped_out + q0, Q.nsk, (size_t)m * sizeof(int32_t), D2H, c->stream));
            if (nblocks_out) HIP_TRY(hipMemcpyAsync(nblocks_out + q0, Q.nb, (size_t)m * sizeof(int32_t), D2H, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            HIP_TRY(c->sw.read());
            total += c->sw.ms;
        }
        return BMX_OK;
    };
    rc = run();
    c->sw.ms = rc ? ms_before : total;      // the call's figure: its chunks' kernels; a failed call leaves the last good one
    return rc;
}

int bmx_ctx_sandwich_ms(bmx_ctx *c, double *ms) {
    if (!c || !ms) return fail(BMX_E_INVALID, "NULL argument");
    return c->sw.get(ms, "no sandwich call yet");
}

int bmx_ctx_refine_R(bmx_ctx *c, double x, double abeta, double *R_out) {
    if (!c || !R_out) return fail(BMX_E_INVALID, "NULL argument");
    ChromSlot *s = c->cur;
    if (!s->ready_to_scan(c)) return fail(BMX_E_STATE, "model, sites and tests must be set before refine_R");
    if (!(x > 0.0 && x < 1.0) || !(abeta > 0.0) || !std::isfinite(abeta))
        return fail(BMX_E_INVALID, "refine_R: 0 < x < 1 and alpha_beta > 0 (finite) are needed");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    RefineParams P;
    int rc = refine_setup(c, s, P, 0);
    if (rc) return rc;
    HIP_TRY(c->sw_R.ensure((size_t)c->rows));
    hipLaunchKernelGGL(refine_R_kernel, dim3((unsigned)((c->rows + REFINE_THREADS - 1) / REFINE_THREADS)), dim3(REFINE_THREADS), 0, c->stream, P, x, abeta,
                       c->sw_R.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(R_out, c->sw_R.p, (size_t)c->rows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BMX_OK;
}

/* ---- resampled sites and the position bootstrap (ballermixplus_amd/locate.py holds the definition) ---- */

int bmx_ctx_resample_sites(bmx_ctx *c, int32_t src_slot, uint64_t key, int64_t block, int64_t *N_out) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    if (!c->has_model) return fail(BMX_E_STATE, "set_model must precede resample_sites");
    ChromSlot *src = nullptr, *s = c->cur;
    int rc = source_slot(c, "resample_sites", src_slot, src);
    if (rc) return rc;
    if (block < 1) return fail(BMX_E_INVALID, "resampling block size must be >= 1");
    if (!src) return fail(BMX_E_STATE, "resample_sites: the source slot has no sites");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    drop_sites(s);
    if (N_out) *N_out = 0;
    const int64_t N = src->N, ntiles = (N + RS_TILE - 1) / RS_TILE;
    HIP_TRY(c->rs_tsum.ensure((size_t)ntiles));
    HIP_TRY(c->rs_tpre.ensure((size_t)ntiles + 1));
    HIP_TRY(c->rs_cnt.ensure((size_t)c->rows));
    const unsigned blocks = (unsigned)std::min<int64_t>(ntiles, RS_BLOCKS_MAX);
    hipLaunchKernelGGL(resample_count_kernel, dim3(blocks), dim3(RS_THREADS), 0, c->stream, key, block, N, ntiles, c->rs_tsum.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(prefix_kernel, dim3(1), dim3(1024), 0, c->stream, (const int32_t *)c->rs_tsum.p, ntiles, c->rs_tpre.p);
    HIP_TRY(hipGetLastError());
    int64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, c->rs_tpre.p + ntiles, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (total >= 0x7fffffffLL) return fail(BMX_E_LIMIT, "resample_sites: more than 2^31 resampled sites");
    if (total < 1) return BMX_OK;             // every weight is 0: the slot stays without sites
    const bool wide = src->wide_rows;
    HIP_TRY(s->genpos.ensure((size_t)total));
    HIP_TRY(s->ensure_rows((size_t)total, wide));
    HIP_TRY(hipMemsetAsync(c->rs_cnt.p, 0, (size_t)c->rows * sizeof(int32_t), c->stream));
    ResampleParams Q;
    Q.key = key; Q.B = block; Q.N = N; Q.ntiles = ntiles; Q.N_out = total;
    Q.src_gen = src->genpos.p;
    Q.src_row = src->row_ptr();
    Q.dst_gen = s->genpos.p;
    Q.dst_row = s->row_ptr();
    Q.tile_pre = c->rs_tpre.p;
    Q.cnt = c->rs_cnt.p;
    Q.rows = c->rows;
    Q.use_hist = c->rows <= RS_HIST_MAX ? 1 : 0;
    const size_t lds = Q.use_hist ? (size_t)c->rows * sizeof(int) : 0;
    if (wide) hipLaunchKernelGGL(resample_expand_kernel<uint32_t>, dim3(blocks), dim3(RS_THREADS), lds, c->stream, Q);
    else hipLaunchKernelGGL(resample_expand_kernel<uint16_t>, dim3(blocks), dim3(RS_THREADS), lds, c->stream, Q);
    HIP_TRY(hipGetLastError());
    if ((rc = finish_derived_sites(c, s, total))) return rc;
    if (N_out) *N_out = total;
    return BMX_OK;
}

int bmx_ctx_fetch_sites(bmx_ctx *c, double *genpos_out, int32_t *row_out) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->has_sites) return fail(BMX_E_STATE, "fetch_sites: the selected slot has no sites");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t N = (size_t)s->N;
    HIP_TRY(download(genpos_out, s->genpos.p, N));
    if (row_out) {
        if (s->wide_rows) {
            HIP_TRY(hipMemcpy(row_out, s->row32.p, N * sizeof(uint32_t), hipMemcpyDeviceToHost));
        } else {
            std::vector<uint16_t> r16(N);
            HIP_TRY(hipMemcpy(r16.data(), s->row16.p, N * sizeof(uint16_t), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < N; i++) row_out[i] = (int32_t)r16[i];
        }
    }
    return BMX_OK;
}

int bmx_ctx_locate_begin(bmx_ctx *c, int32_t K, const int32_t *lo, const int32_t *hi, int32_t R) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    if (K < 1 || R < 1 || !lo || !hi) return fail(BMX_E_INVALID, "locate_begin: K >= 1 ranges and R >= 1 replicates are needed");
    if ((int64_t)K * R > BMX_LOCATE_MAX_RESULTS) return fail(BMX_E_LIMIT, "locate_begin: more than 2^26 (peak, replicate) results");
    int64_t top = 0;
    for (int32_t k = 0; k < K; k++) {
        if (lo[k] < 0 || hi[k] < lo[k]) return fail(BMX_E_INVALID, "locate_begin: a range must have 0 <= lo <= hi");
        top = std::max<int64_t>(top, (int64_t)hi[k] + 1);
    }
    ChromSlot *s = c->cur;
    HIP_TRY(hipSetDevice(c->device));
    s->lc_ok = false;
    const size_t n = (size_t)K * (size_t)R;
    int rc;
    if ((rc = upload(s->lc_lo, lo, (size_t)K, c->stream))) return rc;
    if ((rc = upload(s->lc_hi, hi, (size_t)K, c->stream))) return rc;
    HIP_TRY(s->lc_row.ensure(n));
    HIP_TRY(s->lc_clr.ensure(n));
    HIP_TRY(hipMemsetAsync(s->lc_row.p, 0xff, n * sizeof(int32_t), c->stream));      // -1: no argmax (a replicate never accumulated)
    HIP_TRY(hipMemsetAsync(s->lc_clr.p, 0, n * sizeof(double), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));       // lo / hi are the caller's
    s->lc_ok = true;
    s->lc_K = K;
    s->lc_R = R;
    s->lc_M = top;
    s->lc_seq = s->scan_seq;
    return BMX_OK;
}

int bmx_ctx_locate_accumulate(bmx_ctx *c, int32_t r) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->lc_ok) return fail(BMX_E_STATE, "locate_begin must precede locate_accumulate");
    if (r < 0 || r >= s->lc_R) return fail(BMX_E_INVALID, "locate_accumulate: replicate index outside [0, R)");
    if (!s->has_results() || s->scan_seq == s->lc_seq)
        return fail(BMX_E_STATE, "locate_accumulate needs a new scan (one per replicate)");
    if (s->M < s->lc_M) return fail(BMX_E_INVALID, "locate_accumulate: a range reaches past the slot's test sites");
    HIP_TRY(hipSetDevice(c->device));
    const int per = LOCATE_THREADS / WAVE;
    hipLaunchKernelGGL(locate_reduce_kernel, dim3((unsigned)((s->lc_K + per - 1) / per)), dim3(LOCATE_THREADS), 0, c->stream,
                       (const double *)s->clr.p, (const int32_t *)s->lin.p, (const int32_t *)s->lc_lo.p, (const int32_t *)s->lc_hi.p,
                       (int)s->lc_K, s->lc_row.p + (size_t)r * s->lc_K, s->lc_clr.p + (size_t)r * s->lc_K);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int st = check_status(c, s)) return st;      // the replicate's scan must have been sound
    s->lc_seq = s->scan_seq;
    return BMX_OK;
}

int bmx_ctx_fetch_locate(bmx_ctx *c, int32_t *row_out, double *clr_out) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->lc_ok) return fail(BMX_E_STATE, "locate_begin must precede fetch_locate");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t n = (size_t)s->lc_K * (size_t)s->lc_R;
    HIP_TRY(download(row_out, s->lc_row.p, n));
    HIP_TRY(download(clr_out, s->lc_clr.p, n));
    return BMX_OK;
}

/* ---- planted sites: the power analysis (ballermixplus_amd/power.py holds the definition) ---- */

int bmx_ctx_plant_sites(bmx_ctx *c, int32_t src_slot, uint64_t key, int32_t K, const double *centre, int32_t iA, int32_t ix,
                        int32_t ia, const double *gw, int32_t *first_out, int32_t *count_out, int64_t *changed_out) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    if (!c->has_model) return fail(BMX_E_STATE, "set_model must precede plant_sites");
    ChromSlot *src = nullptr, *s = c->cur;
    int rc = source_slot(c, "plant_sites", src_slot, src);
    if (rc) return rc;
    if (K < 0) return fail(BMX_E_INVALID, "plant_sites: K must be >= 0");
    if (iA < 0 || iA >= c->nA || ix < 0 || ix >= c->nx || ia < 0 || ia >= c->nab)
        return fail(BMX_E_INVALID, "plant_sites: the planted grid point lies outside the model's grids");
    if (K > 0 && (!centre || !gw)) return fail(BMX_E_INVALID, "plant_sites: centre and gw must be given");
    const double A = c->h_A[(size_t)iA];
    for (int32_t k = 0; k < K; k++) {
        if (!(centre[k] - centre[k] == 0.0)) return fail(BMX_E_INVALID, "plant_sites: a centre is not finite");
        if (k + 1 < K && !(A * (centre[k + 1] - centre[k]) > 2.000001 * c->zcut))
            return fail(BMX_E_INVALID, "plant_sites: the centres must ascend and lie more than twice the reach apart");
    }
    if (!src) return fail(BMX_E_STATE, "plant_sites: the source slot has no sites");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    drop_sites(s);
    if (changed_out) *changed_out = 0;
    const int64_t N = src->N;
    const bool wide = src->wide_rows;
    HIP_TRY(s->genpos.ensure((size_t)N));
    HIP_TRY(s->ensure_rows((size_t)N, wide));
    HIP_TRY(c->rs_cnt.ensure((size_t)c->rows));
    HIP_TRY(c->pw_changed.ensure(1));
    std::vector<int32_t> first((size_t)K), count((size_t)K);
    if (K > 0) {
        if ((rc = upload(c->pw_centre, centre, (size_t)K, c->stream))) return rc;
        if ((rc = upload(c->pw_gw, gw, (size_t)c->rows, c->stream))) return rc;
        HIP_TRY(c->pw_first.ensure((size_t)K));
        HIP_TRY(c->pw_count.ensure((size_t)K));
    }
    HIP_TRY(c->pw.begin(c->stream));
    HIP_TRY(hipMemcpyAsync(s->genpos.p, src->genpos.p, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(s->row_ptr(), src->row_ptr(), s->row_bytes((size_t)N), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->pw_changed.p, 0, sizeof(unsigned long long), c->stream));
    HIP_TRY(hipMemsetAsync(c->rs_cnt.p, 0, (size_t)c->rows * sizeof(int32_t), c->stream));
    if (K > 0) {
        hipLaunchKernelGGL(plant_range_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, c->stream, (const double *)src->genpos.p, N,
                           (const double *)c->pw_centre.p, (int)K, A, c->zcut, c->pw_first.p, c->pw_count.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(first.data(), c->pw_first.p, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(count.data(), c->pw_count.p, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));     // the longest run sizes the grid
        int64_t longest = 0;
        for (int32_t k = 0; k < K; k++) {
            if (first[(size_t)k] < 0 || count[(size_t)k] < 0 || (int64_t)first[(size_t)k] + count[(size_t)k] > N)
                return fail(BMX_E_HIP, "plant_sites: a run of sites lies outside the array");
            longest = std::max<int64_t>(longest, count[(size_t)k]);
        }
        if (longest > 0) {
            PlantParams Q;
            Q.key = key;
            Q.gen = src->genpos.p;
            Q.src_row = src->row_ptr(); Q.dst_row = s->row_ptr();
            Q.centre = c->pw_centre.p; Q.first = c->pw_first.p; Q.count = c->pw_count.p; Q.K = K;
            Q.A = A; Q.zcut = c->zcut;
            Q.gw = c->pw_gw.p;
            Q.R = c->d_R.p + ((size_t)ix * c->nab + ia) * (size_t)c->rows;
            Q.row_off = c->d_row_off.p; Q.n_sizes = c->n_sizes; Q.rows = c->rows;
            Q.changed = c->pw_changed.p;
            const bool in_lds = (size_t)c->rows * 16 <= (size_t)PLANT_LDS_BYTES;
            const size_t lds = in_lds ? (size_t)c->rows * 16 : 0;
            const dim3 grid((unsigned)std::min<int64_t>((longest + PLANT_THREADS - 1) / PLANT_THREADS, 65535), (unsigned)std::min<int32_t>(K, 4096));
            if (wide) {
                if (in_lds) hipLaunchKernelGGL((plant_kernel<uint32_t, true>), grid, dim3(PLANT_THREADS), lds, c->stream, Q);
                else hipLaunchKernelGGL((plant_kernel<uint32_t, false>), grid, dim3(PLANT_THREADS), lds, c->stream, Q);
            } else {
                if (in_lds) hipLaunchKernelGGL((plant_kernel<uint16_t, true>), grid, dim3(PLANT_THREADS), lds, c->stream, Q);
                else hipLaunchKernelGGL((plant_kernel<uint16_t, false>), grid, dim3(PLANT_THREADS), lds, c->stream, Q);
            }
            HIP_TRY(hipGetLastError());
        }
    }
    {   // the sites per table row of the finished array
        const int use_hist = c->rows <= RS_HIST_MAX ? 1 : 0;
        const size_t lds = use_hist ? (size_t)c->rows * sizeof(int) : 0;
        const unsigned blocks = (unsigned)std::min<int64_t>((N + RS_THREADS - 1) / RS_THREADS, PLANT_HIST_BLOCKS_MAX);
        if (wide) hipLaunchKernelGGL(plant_hist_kernel<uint32_t>, dim3(blocks), dim3(RS_THREADS), lds, c->stream, (const uint32_t *)s->row32.p, N,
                                     c->rs_cnt.p, c->rows, use_hist);
        else hipLaunchKernelGGL(plant_hist_kernel<uint16_t>, dim3(blocks), dim3(RS_THREADS), lds, c->stream, (const uint16_t *)s->row16.p, N,
                                c->rs_cnt.p, c->rows, use_hist);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(c->pw.end(c->stream));
    unsigned long long changed = 0;
    if ((rc = finish_derived_sites(c, s, N, &changed))) return rc;
    HIP_TRY(c->pw.read());          // (that call has waited for the stream)
    for (int32_t k = 0; k < K; k++) {
        if (first_out) first_out[k] = first[(size_t)k];
        if (count_out) count_out[k] = count[(size_t)k];
    }
    if (changed_out) *changed_out = (int64_t)changed;
    return BMX_OK;
}

int bmx_ctx_plant_ms(bmx_ctx *c, double *ms) {
    if (!c || !ms) return fail(BMX_E_INVALID, "null argument");
    return c->pw.get(ms, "no plant_sites call yet");
}

int bmx_ctx_fetch_at(bmx_ctx *c, int64_t n, const int32_t *tests, double *clr, int32_t *lin, int32_t *nsites) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->has_results()) return fail(BMX_E_STATE, "fetch_at needs a scan: call bmx_ctx_scan first");
    if (n < 0 || (n > 0 && !tests)) return fail(BMX_E_INVALID, "fetch_at: a list of test sites must be given");
    if (n > 0x7fffff00LL) return fail(BMX_E_LIMIT, "fetch_at: more than 2^31 indices");
    for (int64_t j = 0; j < n; j++)
        if (tests[j] < -1 || (int64_t)tests[j] >= s->M) return fail(BMX_E_INVALID, "fetch_at: a test site index outside [0, M) (or -1)");
    if (n == 0) return BMX_OK;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = upload(c->fa_idx, tests, (size_t)n, c->stream))) return rc;
    HIP_TRY(c->fa_clr.ensure((size_t)n));
    HIP_TRY(c->fa_lin.ensure((size_t)n));
    HIP_TRY(c->fa_ns.ensure((size_t)n));
    hipLaunchKernelGGL(fetch_at_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const double *)s->clr.p,
                       (const int32_t *)s->lin.p, (const int32_t *)s->nsites.p, (const int32_t *)c->fa_idx.p, n, c->fa_clr.p, c->fa_lin.p,
                       c->fa_ns.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(download(clr, c->fa_clr.p, (size_t)n)); HIP_TRY(download(lin, c->fa_lin.p, (size_t)n)); HIP_TRY(download(nsites, c->fa_ns.p, (size_t)n));
    return BMX_OK;
}

}  // extern "C"

/* ---- peaks (ballermixplus_amd/peaks.py holds the definition: apex, saddle, extent) ---- */

namespace {

int peaks_check(const char *who, double sep, double min_clr, double frac) {
    if (sep != sep || min_clr != min_clr || frac != frac) return fail(BMX_E_INVALID, std::string(who) + ": NaN argument");
    if (!(sep >= 0.0)) return fail(BMX_E_INVALID, std::string(who) + ": the separation must be >= 0");
    if (!(frac > 0.0 && frac <= 1.0)) return fail(BMX_E_INVALID, std::string(who) + ": the extent fraction must lie in (0, 1]");
    return BMX_OK;
}

// The peak call on a device-resident track (g, clr: M rows, positions non-decreasing) into the slot's peak state.  Blocks.
int peaks_run(bmx_ctx *c, ChromSlot *s, const double *g, const double *clr, int64_t M, double sep, double min_clr, double frac) {
    if (M > 0x7fffff00LL) return fail(BMX_E_LIMIT, "peaks: more than 2^31 rows");
    s->pk_have = false;
    int64_t K = 0;
    HIP_TRY(c->pk.begin(c->stream));
    if (M > 0) {
        const int64_t tiles = (M + PEAK_TILE - 1) / PEAK_TILE;
        HIP_TRY(c->pk_tmax.ensure((size_t)tiles));
        HIP_TRY(c->pk_tfirst.ensure((size_t)tiles));
        HIP_TRY(s->pk_flag.ensure((size_t)M));
        HIP_TRY(c->rf_pre.ensure((size_t)M + 1));
        const unsigned nb = (unsigned)((M + PEAK_THREADS - 1) / PEAK_THREADS);
        hipLaunchKernelGGL(peak_tile_kernel, dim3(nb), dim3(PEAK_THREADS), 0, c->stream, clr, M, c->pk_tmax.p, c->pk_tfirst.p);
        HIP_TRY(hipGetLastError());
        PeakParams Q;
        Q.g = g; Q.c = clr; Q.M = M; Q.sep = sep; Q.min_clr = min_clr;
        Q.tmax = c->pk_tmax.p; Q.tfirst = c->pk_tfirst.p; Q.flag = s->pk_flag.p;
        hipLaunchKernelGGL(peak_apex_kernel, dim3(nb), dim3(PEAK_THREADS), 0, c->stream, Q);
        HIP_TRY(hipGetLastError());
        // the apexes in row order: the order is part of the result, so a prefix sum and not an atomic counter
        HIP_TRY(flag_prefix(c, s->pk_flag.p, M));
        HIP_TRY(hipMemcpyAsync(&K, c->rf_pre.p + M, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));       // the number of apexes sizes their arrays
        HIP_TRY(s->pk_row.ensure((size_t)K)); HIP_TRY(s->pk_lo.ensure((size_t)K)); HIP_TRY(s->pk_hi.ensure((size_t)K));
        HIP_TRY(s->pk_sad.ensure((size_t)K + 1));
        if (K > 0) {
            HIP_TRY(flag_compact(c, s->pk_flag.p, M, s->pk_row.p));
            const unsigned ng = (unsigned)std::min<int64_t>(std::max<int64_t>(K - 1, 1), 1 << 20);
            hipLaunchKernelGGL(peak_saddle_kernel, dim3(ng), dim3(PEAK_THREADS), 0, c->stream, clr, (const int32_t *)s->pk_row.p, K, s->pk_sad.p);
            HIP_TRY(hipGetLastError());
            const int per = PEAK_THREADS / WAVE;
            hipLaunchKernelGGL(peak_extent_kernel, dim3((unsigned)((K + per - 1) / per)), dim3(PEAK_THREADS), 0, c->stream, clr, M,
                               (const int32_t *)s->pk_row.p, (const int32_t *)s->pk_sad.p, K, frac, s->pk_lo.p, s->pk_hi.p);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(c->pk.end(c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(c->pk.read());
    s->pk_M = M; s->pk_K = K;
    s->pk_have = true;
    s->pk_scan = false;
    return BMX_OK;
}

}  // namespace

extern "C" {

int bmx_ctx_peaks(bmx_ctx *c, double sep, double min_clr, double frac) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    int rc = peaks_check("peaks", sep, min_clr, frac);
    if (rc) return rc;
    ChromSlot *s = c->cur;
    if (!c->has_model || !s->has_results()) return fail(BMX_E_INVALID, "peaks: no scan results (scan the slot first)");
    if (!s->tests_sorted) return fail(BMX_E_INVALID, "peaks: the slot's test positions are not non-decreasing");
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = peaks_run(c, s, s->test_gen.p, s->clr.p, s->M, sep, min_clr, frac))) return rc;
    s->pk_scan = true;
    s->pk_seq = s->scan_seq;
    return BMX_OK;
}

int bmx_ctx_peaks_track(bmx_ctx *c, int64_t M, const double *gen, const double *clr, double sep, double min_clr, double frac) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    int rc = peaks_check("peaks_track", sep, min_clr, frac);
    if (rc) return rc;
    if (M < 0 || (M > 0 && (!gen || !clr))) return fail(BMX_E_INVALID, "peaks_track: M >= 0 rows of positions and values are needed");
    for (int64_t t = 0; t < M; t++) {
        if (clr[t] != clr[t] || !std::isfinite(gen[t])) return fail(BMX_E_INVALID, "peaks_track: NaN value or non-finite position at row " + std::to_string(t));
        if (t && !(gen[t] >= gen[t - 1])) return fail(BMX_E_INVALID, "peaks_track: positions are not non-decreasing at row " + std::to_string(t));
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(c->pk_track.ensure((size_t)2 * (size_t)M));
    if (M) {
        HIP_TRY(hipMemcpyAsync(c->pk_track.p, gen, (size_t)M * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->pk_track.p + M, clr, (size_t)M * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));       // the caller's arrays may go away; the call's timing starts after the upload
    }
    return peaks_run(c, c->cur, c->pk_track.p, c->pk_track.p + M, M, sep, min_clr, frac);
}

int bmx_ctx_peak_count(bmx_ctx *c, int64_t *n_peaks, int64_t *M) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->pk_have) return fail(BMX_E_STATE, "no peak call on the slot: call bmx_ctx_peaks after a scan, or bmx_ctx_peaks_track");
    if (n_peaks) *n_peaks = s->pk_K;
    if (M) *M = s->pk_M;
    return BMX_OK;
}

int bmx_ctx_fetch_peaks(bmx_ctx *c, int32_t *row, int32_t *lo, int32_t *hi, int32_t *saddle_lo, int32_t *saddle_hi) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    ChromSlot *s = c->cur;
    if (!s->pk_have) return fail(BMX_E_STATE, "no peak call on the slot: call bmx_ctx_peaks after a scan, or bmx_ctx_peaks_track");
    const size_t K = (size_t)s->pk_K;
    if (!K) return BMX_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(download(row, s->pk_row.p, K)); HIP_TRY(download(lo, s->pk_lo.p, K)); HIP_TRY(download(hi, s->pk_hi.p, K));
    HIP_TRY(download(saddle_lo, s->pk_sad.p, K)); HIP_TRY(download(saddle_hi, s->pk_sad.p + 1, K));
    return BMX_OK;
}

int bmx_ctx_peaks_ms(bmx_ctx *c, double *ms) {
    if (!c || !ms) return fail(BMX_E_INVALID, "NULL argument");
    return c->pk.get(ms, "no peak call yet");
}

int bmx_ctx_refine_at_peaks(bmx_ctx *c, int32_t on) {
    if (!c) return fail(BMX_E_INVALID, "ctx is NULL");
    c->rf_at_peaks = on != 0;
    return BMX_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------- RCCL gather
// librccl.so through dlopen: only these entry points, resolved once
struct RcclApi {
    void *handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    std::string error;
};

struct bmx_comm {
    bmx_ctx *ctx = nullptr;
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1;
    DevBuf<bmx_record> send, recv;
};

namespace {

RcclApi *rccl_api() {
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            api.handle = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (api.handle) break;
        }
        if (!api.handle) { api.error = std::string("librccl.so cannot be opened: ") + dlerror(); return; }
        auto sym = [&](const char *n) -> void * {
            void *f = dlsym(api.handle, n);
            if (!f && api.error.empty()) api.error = std::string("librccl.so lacks ") + n;
            return f;
        };
        api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(sym("ncclGetUniqueId"));
        api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(sym("ncclCommInitRank"));
        api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(sym("ncclCommDestroy"));
        api.GroupStart = reinterpret_cast<decltype(api.GroupStart)>(sym("ncclGroupStart"));
        api.GroupEnd = reinterpret_cast<decltype(api.GroupEnd)>(sym("ncclGroupEnd"));
        api.Send = reinterpret_cast<decltype(api.Send)>(sym("ncclSend"));
        api.Recv = reinterpret_cast<decltype(api.Recv)>(sym("ncclRecv"));
        api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(sym("ncclGetErrorString"));
    });
    return &api;
}

#define RCCL_TRY(api, expr)                                                                                        \
    do {                                                                                                           \
        ncclResult_t r_ = (expr);                                                                                  \
        if (r_ != ncclSuccess) return fail(BMX_E_HIP, std::string(#expr) + ": " + (api)->GetErrorString(r_));      \
    } while (0)

}  // namespace

extern "C" {

int bmx_comm_unique_id(char *id) {
    if (!id) return fail(BMX_E_INVALID, "id is NULL");
    RcclApi *api = rccl_api();
    if (!api->error.empty()) return fail(BMX_E_HIP, api->error);
    static_assert(sizeof(ncclUniqueId) == BMX_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
    ncclUniqueId u;
    RCCL_TRY(api, api->GetUniqueId(&u));
    memcpy(id, &u, sizeof u);
    return BMX_OK;
}

int bmx_comm_create(bmx_comm **out, bmx_ctx *c, const char *id, int32_t rank, int32_t world) {
    if (!out || !c || !id) return fail(BMX_E_INVALID, "NULL argument");
    *out = nullptr;
    if (world < 1 || rank < 0 || rank >= world) return fail(BMX_E_INVALID, "rank / world out of range");
    RcclApi *api = rccl_api();
    if (!api->error.empty()) return fail(BMX_E_HIP, api->error);
    HIP_TRY(hipSetDevice(c->device));
    ncclUniqueId u;
    memcpy(&u, id, sizeof u);
    ncclComm_t comm = nullptr;
    RCCL_TRY(api, api->CommInitRank(&comm, world, u, rank));
    bmx_comm *cm = new bmx_comm();
    cm->ctx = c; cm->comm = comm; cm->rank = rank; cm->world = world;
    *out = cm;
    return BMX_OK;
}

void bmx_comm_destroy(bmx_comm *cm) {
    if (!cm) return;
    (void)hipSetDevice(cm->ctx->device);
    RcclApi *api = rccl_api();
    if (cm->comm && api->CommDestroy) (void)api->CommDestroy(cm->comm);
    delete cm;
}

int bmx_comm_gather_records(bmx_comm *cm, const int64_t *counts, int32_t root, bmx_record *dst_host, void **d_out) {
    if (!cm || !counts) return fail(BMX_E_INVALID, "NULL argument");
    if (root < 0 || root >= cm->world) return fail(BMX_E_INVALID, "root out of range");
    RcclApi *api = rccl_api();
    bmx_ctx *c = cm->ctx;
    HIP_TRY(hipSetDevice(c->device));
    int64_t total = 0, my_off = 0;
    for (int r = 0; r < cm->world; r++) {
        if (counts[r] < 0) return fail(BMX_E_INVALID, "negative record count");
        if (r < cm->rank) my_off += counts[r];
        total += counts[r];
    }
    const int64_t mine = counts[cm->rank];
    const bool is_root = cm->rank == root;
    // this rank's records, packed: straight into the root's receive buffer at the rank's own offset, or into the send buffer
    bmx_record *pack_to = nullptr;
    if (is_root) {
        HIP_TRY(cm->recv.ensure((size_t)total));
        pack_to = cm->recv.p + my_off;
    } else {
        HIP_TRY(cm->send.ensure((size_t)mine));
        pack_to = cm->send.p;
    }
    int64_t n = 0;
    int rc = bmx_ctx_pack_records(c, pack_to, mine, 1, &n);
    if (rc) return rc;
    if (n != mine) return fail(BMX_E_INVALID, "gather_records: counts[rank] differs from the records this context holds");
    // one group: the root posts a receive per peer (each at that rank's offset), every peer one send
    RCCL_TRY(api, api->GroupStart());
    if (is_root) {
        int64_t off = 0;
        for (int r = 0; r < cm->world; r++) {
            if (r != root && counts[r] > 0)
                RCCL_TRY(api, api->Recv(cm->recv.p + off, (size_t)counts[r] * sizeof(bmx_record), ncclChar, r, cm->comm, c->stream));
            off += counts[r];
        }
    } else if (mine > 0) {
        RCCL_TRY(api, api->Send(cm->send.p, (size_t)mine * sizeof(bmx_record), ncclChar, root, cm->comm, c->stream));
    }
    RCCL_TRY(api, api->GroupEnd());
    if (is_root && dst_host && total > 0)
        HIP_TRY(hipMemcpyAsync(dst_host, cm->recv.p, (size_t)total * sizeof(bmx_record), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (d_out) *d_out = is_root ? (void *)cm->recv.p : nullptr;
    return BMX_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------- streaming output
// The reference writes each row as soon as calcBaller returns it (BalLeRMix+_v1.py:599-608).  Here the test sites are
// scanned in chunks on the context's stream; chunk i's results travel to pinned host memory on a second stream and are
// formatted and appended to the output file by a writer thread while chunk i+1 is being scanned.
#include <condition_variable>
#include <deque>
#include <mutex>

extern "C" int bmx_ctx_scan_write(bmx_ctx *c, const char *path, const int64_t *phys, const double *gen,
                                  const char *xs, int nx, const char *abs_, int nab, const char *As, int nA, int64_t chunk) {
    if (!c || !path || !phys || !gen || !xs || !abs_ || !As) return fail(BMX_E_INVALID, "NULL argument");
    ChromSlot *s = c->cur;
    if (!c->has_model || !s->has_sites || !s->has_tests) return fail(BMX_E_STATE, "model, sites and tests must be set before scan");
    if (nx != c->nx || nab != c->nab || nA != c->nA) return fail(BMX_E_INVALID, "printed grids do not match the model's grids");
    HIP_TRY(hipSetDevice(c->device));
    std::vector<PrepRange> rs;
    int rc = scan_ranges(c, s, rs);
    if (rc) return rc;
    if ((rc = begin_profiles(c, s))) return rc;
    if ((rc = begin_range_word(c, s))) return rc;
    ScanPlan &pl = s->plan;
    // chunks: the prepared pipeline's launch ranges as they are (their blobs were sized per range); otherwise `chunk` test
    // sites at a time (0: 65536; whole workgroups, which keeps every result bit-identical to bmx_ctx_scan)
    std::vector<PrepRange> chunks;
    if (pl.mode >= 4) {
        // a prepared range is cut further into chunks of whole workgroups: each chunk's groups are a sub-range of the
        // range's blobs (same arena, same prefix base), so nothing has to be re-planned
        if (chunk <= 0) chunk = 65536;
        chunk = std::max<int64_t>(chunk / pl.spb, 1) * pl.spb;
        for (const PrepRange &r : rs)
            for (int64_t o = 0; o < r.cnt; o += chunk) {
                PrepRange q = r;
                q.off = r.off + o;
                q.cnt = std::min(chunk, r.cnt - o);
                chunks.push_back(q);
            }
    } else {
        if (chunk <= 0) chunk = 65536;
        chunk = std::min<int64_t>(std::max<int64_t>(chunk / pl.spb, 1) * pl.spb, pl.range);
        for (int64_t off = 0; off < s->M; off += chunk) chunks.push_back(PrepRange{off, std::min(chunk, s->M - off), 0, 0, 0, 0});
    }
    int64_t chunk_max = 1;
    for (const PrepRange &q : chunks) chunk_max = std::max(chunk_max, q.cnt);
    const size_t slot_bytes = (size_t)chunk_max * 16;
    for (PinnedBuf &h : c->h_stage) HIP_TRY(h.ensure(slot_bytes));
    bmx_row_tables_ *tabs = bmx_row_tables_new_(xs, nx, abs_, nab, As, nA);
    FILE *f = fopen(path, "a");
    if (!f) {
        bmx_row_tables_free_(tabs);
        return fail(BMX_E_INVALID, std::string("cannot open ") + path + ": " + strerror(errno));
    }
    struct Job { int slot; int64_t off, cnt; };
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Job> jobs;
    bool slot_free[2] = {true, true}, done = false;
    int werr = 0;                  // 1: event wait failed, 2: formatting/writing failed
    std::string wmsg;              // the writer thread's own message (bmx_last_error is thread-local)
    std::thread writer([&]() {
        (void)hipSetDevice(c->device);
        for (;;) {
            Job j;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !jobs.empty() || done; });
                if (jobs.empty()) return;
                j = jobs.front();
                jobs.pop_front();
            }
            int e = 0;
            std::string msg;
            if (hipEventSynchronize(c->ev_copied[j.slot]) != hipSuccess) e = 1;
            if (!e && !werr) {
                const char *base = c->h_stage[j.slot].p;
                const double *hclr = (const double *)base;
                const int32_t *hlin = (const int32_t *)(base + (size_t)chunk_max * 8);
                const int32_t *hns = (const int32_t *)(base + (size_t)chunk_max * 12);
                if (bmx_write_chunk_(f, tabs, j.cnt, phys + j.off, gen + j.off, hclr, nullptr, nullptr, nullptr, hlin, hns)) {
                    e = 2;
                    msg = bmx_last_error();       // set on THIS thread by bmx_write_chunk_
                }
            }
            {
                std::lock_guard<std::mutex> lk(mu);
                if (e && !werr) { werr = e; wmsg = msg; }
                slot_free[j.slot] = true;
            }
            cv.notify_all();
        }
    });
    bool all_launched = false;
    auto finish = [&](int code, const std::string &msg) {
        {
            std::lock_guard<std::mutex> lk(mu);
            done = true;
        }
        cv.notify_all();
        writer.join();
        (void)hipStreamSynchronize(c->stream);
        (void)hipStreamSynchronize(c->copy_stream);
        const bool wfail = fclose(f) != 0;
        bmx_row_tables_free_(tabs);
        s->timed = all_launched && !werr && !code;     // results are fetchable only when every chunk was scanned
        if (s->timed) s->scan_seq++;
        s->pl_have = s->timed ? c->pl_which : 0;
        if (code) return fail(code, msg);
        if (werr == 1) return fail(BMX_E_HIP, "streaming writer: waiting for a result copy failed");
        if (werr == 2) return fail(BMX_E_INVALID, std::string("streaming writer: ") + wmsg);
        if (wfail) return fail(BMX_E_INVALID, "write failed");
        return check_status(c, s);
    };
#define STREAM_TRY(expr)                                                                                  \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return finish(BMX_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
    STREAM_TRY(s->scan.begin(c->stream));
    size_t k = 0;
    bool stopped = false;
    for (; k < chunks.size(); ++k) {
        const PrepRange &q = chunks[k];
        const int slot = (int)(k & 1);
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return slot_free[slot]; });
            if (werr) { stopped = true; break; }
            slot_free[slot] = false;
        }
        if (pl.mode >= 4) {
            // the chunk's groups within its range: fill + consume exactly those
            PrepRange sub = q;
            sub.g0 = q.off / pl.J;
            sub.ng = (q.cnt + pl.J - 1) / pl.J;
            if ((rc = launch_range(c, s, pl, q.off, q.cnt, &sub))) return finish(rc, g_err);
        } else if ((rc = launch_range(c, s, pl, q.off, q.cnt, nullptr))) return finish(rc, g_err);
        STREAM_TRY(hipEventRecord(c->ev_done[slot], c->stream));
        STREAM_TRY(hipStreamWaitEvent(c->copy_stream, c->ev_done[slot], 0));
        char *base = c->h_stage[slot].p;
        STREAM_TRY(hipMemcpyAsync(base, s->clr.p + q.off, (size_t)q.cnt * 8, hipMemcpyDeviceToHost, c->copy_stream));
        STREAM_TRY(hipMemcpyAsync(base + (size_t)chunk_max * 8, s->lin.p + q.off, (size_t)q.cnt * 4, hipMemcpyDeviceToHost, c->copy_stream));
        STREAM_TRY(hipMemcpyAsync(base + (size_t)chunk_max * 12, s->nsites.p + q.off, (size_t)q.cnt * 4, hipMemcpyDeviceToHost, c->copy_stream));
        STREAM_TRY(hipEventRecord(c->ev_copied[slot], c->copy_stream));
        {
            std::lock_guard<std::mutex> lk(mu);
            jobs.push_back(Job{slot, q.off, q.cnt});
        }
        cv.notify_all();
    }
    STREAM_TRY(s->scan.end(c->stream));
#undef STREAM_TRY
    all_launched = !stopped;
    return finish(BMX_OK, "");
}

namespace {
// The context of a one-shot entry point: destroyed at the end of the call, with the thread's error text as the call left it
struct OneShotCtx {
    bmx_ctx *c = nullptr;
    ~OneShotCtx() {
        const std::string keep = g_err;
        bmx_ctx_destroy(c);
        g_err = keep;
    }
};
}  // namespace

extern "C" {

int bmx_lut_build(const bmx_model *m, double *psel_out, double *R_out, int device) {
    OneShotCtx own;
    int rc = bmx_ctx_create(&own.c, device);
    const double A1 = 1.0;
    if (!rc) rc = bmx_ctx_set_model(own.c, m, &A1, 1);
    if (!rc) rc = bmx_ctx_fetch_lut(own.c, psel_out, R_out);
    return rc;
}

int bmx_scan(const bmx_model *m, const double *A, int32_t nA, int64_t N, const double *genpos,
             const int32_t *row, int64_t M, const double *test_gen, const int64_t *win_lo,
             const int64_t *win_hi, double *clr, int32_t *ix, int32_t *ia, int32_t *iA,
             int32_t *nsites, int device) {
    OneShotCtx own;
    int rc = bmx_ctx_create(&own.c, device);
    if (!rc) rc = bmx_ctx_set_model(own.c, m, A, nA);
    if (!rc) rc = bmx_ctx_set_sites(own.c, N, genpos, row);
    if (!rc) rc = bmx_ctx_set_tests(own.c, M, test_gen, win_lo, win_hi);
    if (!rc) rc = bmx_ctx_scan(own.c);
    if (!rc) rc = bmx_ctx_fetch(own.c, clr, ix, ia, iA, nsites);
    return rc;
}


/* bmx_scan on several GPUs of this node, inside the library (no torch, no process group): one host thread and one context
 * per entry of `devices` (NULL: 0 .. n_devices-1; an index may repeat -- two contexts on one GPU), test sites dealt to the
 * workers in blocks of 4096 consecutive test sites round-robin -- the sharding of ballermixplus_amd/distributed.py, so every
 * row is bitwise what one GPU computes -- and each worker's results copied into the caller's buffers. */
int bmx_scan_multi(const bmx_model *m, const double *A, int32_t nA, int64_t N, const double *genpos,
                   const int32_t *row, int64_t M, const double *test_gen, const int64_t *win_lo,
                   const int64_t *win_hi, double *clr, int32_t *ix, int32_t *ia, int32_t *iA,
                   int32_t *nsites, int32_t n_devices, const int32_t *devices) {
    if (n_devices < 1 || n_devices > 64) return fail(BMX_E_INVALID, "n_devices must be 1..64");
    if (M < 1 || !test_gen || !win_lo || !win_hi) return fail(BMX_E_INVALID, "empty test-site arrays");
    constexpr int64_t BLOCK = 4096;
    const int64_t nblk = (M + BLOCK - 1) / BLOCK;
    std::vector<int> rcs((size_t)n_devices, BMX_OK);
    std::vector<std::string> msgs((size_t)n_devices);
    auto work = [&](int w) {
        // this worker's test sites: blocks w, w + n, w + 2n, ...
        std::vector<int64_t> idx;
        for (int64_t b = w; b < nblk; b += n_devices)
            for (int64_t t = b * BLOCK; t < std::min((b + 1) * BLOCK, M); ++t) idx.push_back(t);
        if (idx.empty()) return;
        const size_t n = idx.size();
        std::vector<double> tg(n), c_(n);
        std::vector<int64_t> lo(n), hi(n);
        std::vector<int32_t> x_(n), a_(n), A_(n), ns_(n);
        for (size_t i = 0; i < n; ++i) { tg[i] = test_gen[idx[i]]; lo[i] = win_lo[idx[i]]; hi[i] = win_hi[idx[i]]; }
        OneShotCtx own;
        int rc = bmx_ctx_create(&own.c, devices ? devices[w] : w);
        if (!rc) rc = bmx_ctx_set_model(own.c, m, A, nA);
        if (!rc) rc = bmx_ctx_set_sites(own.c, N, genpos, row);
        if (!rc) rc = bmx_ctx_set_tests(own.c, (int64_t)n, tg.data(), lo.data(), hi.data());
        if (!rc) rc = bmx_ctx_scan(own.c);
        if (!rc) rc = bmx_ctx_fetch(own.c, c_.data(), x_.data(), a_.data(), A_.data(), ns_.data());
        if (rc) msgs[(size_t)w] = bmx_last_error();          // this thread's message
        rcs[(size_t)w] = rc;
        if (rc) return;
        for (size_t i = 0; i < n; ++i) {
            const int64_t t = idx[i];
            if (clr) clr[t] = c_[i];
            if (ix) ix[t] = x_[i];
            if (ia) ia[t] = a_[i];
            if (iA) iA[t] = A_[i];
            if (nsites) nsites[t] = ns_[i];
        }
    };
    std::vector<std::thread> th;
    for (int w = 0; w < n_devices; ++w) th.emplace_back(work, w);
    for (auto &t : th) t.join();
    for (int w = 0; w < n_devices; ++w)
        if (rcs[(size_t)w]) return fail(rcs[(size_t)w], "worker " + std::to_string(w) + ": " + msgs[(size_t)w]);
    return BMX_OK;
}

}  // extern "C"

#endif  // BMX_DEVICE_PROBE
