/* bmxscan.h -- C ABI of libbmxscan.so, the MI355X (gfx950) composite-likelihood scan.
 *
 * The reference (bioXiaoheng/BallerMixPlus, BalLeRMix+_v1.py) is a single Python
 * script with no FFI of its own; the seam this library drops into is the pair of
 * Python calls on its hot path:
 *
 *   NormalizedBetaBinom(InputData, Grids, nofreq, MAF, nosub)      BalLeRMix+_v1.py:793 (class at :310-433)
 *   calcBaller(window_indice, testSite, InputData, NeutralSFS,
 *              NormalizedBetaBinom, Grids) -> [T, x, abeta, A, nSites]
 *                                                                   BalLeRMix+_v1.py:539,573,590,606 (def at :436-507)
 *
 * Every entry point is extern "C", takes plain pointers and sizes, never throws,
 * never exits the process and retains no caller memory after it returns.
 * Return value: 0 on success, a negative BMX_E_* code otherwise; the message is
 * available from bmx_last_error() (thread-local).  All host buffers are
 * caller-allocated, C-contiguous, native endian.  There is NO CPU fallback: when
 * no HIP device is usable every compute entry point fails with BMX_E_NODEVICE.
 */
#ifndef BMXSCAN_H
#define BMXSCAN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BMX_ABI_VERSION_MAJOR 1
#define BMX_ABI_VERSION_MINOR 5

enum {
    BMX_OK = 0,
    BMX_E_INVALID = -1,   /* bad argument (null pointer, size, unsorted positions, ...) */
    BMX_E_NODEVICE = -2,  /* no usable HIP device / device index out of range */
    BMX_E_HIP = -3,       /* a HIP runtime call failed; see bmx_last_error() */
    BMX_E_LIMIT = -4,     /* a documented limit was exceeded (2^24 LUT rows, 2^31 sites, 2^31 grid points, a CLR past the scan's range) */
    BMX_E_STATE = -5      /* call order violated (e.g. scan before model/sites were set) */
};

/* Which B statistic the selection table is built for.
 * Replaces the (nofreq, MAF, nosub) flag triple of NormalizedBetaBinom.__init__
 * (BalLeRMix+_v1.py:319, dispatch at :336-352). */
enum {
    BMX_STAT_B2 = 0,     /* default                      v1:351-352, normBase :399-404 */
    BMX_STAT_B2MAF = 1,  /* --MAF                        v1:344-345, :389-392, :406-413 */
    BMX_STAT_B0 = 2,     /* --noSub                      v1:348-349, :419-425 */
    BMX_STAT_B0MAF = 3,  /* --noSub --MAF                v1:341-342, :427-433 */
    BMX_STAT_B1 = 4      /* --noFreq                     v1:337-338, :378-383, :415-417 */
};

/* The model the grid search runs over.  It carries what calcBaller reads from
 * InputData / NeutralSFS / Grids, re-indexed by LUT row instead of by site:
 * a site with derived count k and sample size sizes[j] maps to row
 * row_off[j] + k  (B1: k in {0,1}).  rows = row_off[n_sizes]. */
typedef struct bmx_model {
    int32_t stat;            /* BMX_STAT_* */
    int32_t min_count;       /* InputData.minCount (v1:59,74) */
    int32_t n_sizes;         /* number of distinct sample sizes (InputData.sampSizes, v1:76) */
    const int32_t *sizes;    /* [n_sizes] sample sizes n */
    const int32_t *row_off;  /* [n_sizes+1] first LUT row of each size */
    const double *g;         /* [rows] neutral probability NeutralSFS.spect[(k,n)] (v1:208,292);
                                NaN for (k,n) absent from the helper file (never referenced by a site) */
    const double *prop;      /* [n_sizes] NeutralSFS.sampProps[n] (v1:212-214,304) */
    int32_t nx;              /* grids in the reference's ITERATION order: list(set(Grids.x)) etc. */
    const double *x;         /* [nx]   (v1:473) */
    int32_t nab;
    const double *abeta;     /* [nab]  (v1:474) */
} bmx_model;

/* One result row as the multi-GPU gather moves it (16 bytes): CLR, linear grid index
 * (iA*nx + ix)*nab + ia (-1: no grid point had T > 0) and nSites -- Tmax[0], Tmax[1:4], Tmax[4] of
 * calcBaller's return value (BalLeRMix+_v1.py:451,502,507). */
typedef struct bmx_record {
    double clr;
    int32_t lin;
    int32_t nsites;
} bmx_record;

/* ---- library-level queries -------------------------------------------------------- */
void bmx_version(int *major, int *minor);
/* Hash of the kernel/host sources this binary was built from (first 16 hex digits of their SHA-256, set by the
 * Makefile): the Python shim refuses a library whose id differs from the sources next to it. */
const char *bmx_build_id(void);
const char *bmx_last_error(void);
/* Number of visible HIP devices (0 when none / no driver). */
int bmx_device_count(void);
/* The window cut-off in the exponent domain: largest double z with exp(-z) >= 1e-8, so that the
 * reference's predicate `np.exp(-A*dist) >= 1e-8` (BalLeRMix+_v1.py:454-455) is `A*dist <= z`. */
double bmx_alpha_cut(void);
/* Diagnostic: the bytes of device memory and of pinned host memory that the contexts and communicators of this process hold
 * right now, summed over all of them and all devices.  Every allocation of the library is counted, at the size asked for;
 * what the runtime itself or other libraries hold is not.  After the last context is destroyed both are what they were
 * before the first was created.  Either pointer may be NULL; takes no context and never fails. */
void bmx_live_bytes(int64_t *device_bytes, int64_t *pinned_bytes);

/* ---- one-shot entry points (host buffers in, host buffers out) ---------------------- */

/* Replaces NormalizedBetaBinom.__init__ (BalLeRMix+_v1.py:319-359) + get() (:362-363).
 * Runs the device lgamma / beta-binomial kernel and returns, for every grid pair
 * and LUT row,
 *     psel_out[ix][ia][row] = normProbs[(x,a)] value of a site on that row      (optional, may be NULL)
 *     R_out   [ix][ia][row] = psel * prop(n) / g(k,n) - 1                       (optional, may be NULL)
 * so that calcBaller's mixture log-ratio of one site is log1p(alpha * R) (v1:494-499). */
int bmx_lut_build(const bmx_model *m, double *psel_out, double *R_out, int device);

/* Replaces the calcBaller call of every Scan mode (BalLeRMix+_v1.py:539,573,590,606).
 *   A[nA]        linkage grid in iteration order list(set(Grids.A))                    (v1:453)
 *   genpos[N]    InputData.genPos, non-decreasing;  row[N] LUT row of each site
 *   test_gen[M]  genetic position of each test site (testSite argument, v1:436)
 *   win_lo/hi[M] inclusive index bounds of window_indice (0, N-1 for the default mode)
 * Outputs, length M:  clr = Tmax[0];  ix/ia/iA = indices of x_hat / alpha_hat / A_hat in the
 * grids passed in;  nsites = Tmax[4].  iA == -1 (with clr = 0, ix = ia = -1, nsites = 0)
 * means no grid point had T > 0: the reference prints its all-zero initial row (v1:451). */
int bmx_scan(const bmx_model *m, const double *A, int32_t nA, int64_t N, const double *genpos,
             const int32_t *row, int64_t M, const double *test_gen, const int64_t *win_lo,
             const int64_t *win_hi, double *clr, int32_t *ix, int32_t *ia, int32_t *iA,
             int32_t *nsites, int device);

/* bmx_scan on several GPUs of this node, inside the library (no Python, no torch, no process group): one host thread and
 * one context per entry of devices[n_devices] (NULL: GPUs 0 .. n_devices-1; an index may repeat), test sites dealt to the
 * workers in blocks of 4096 consecutive test sites round-robin, each worker's results copied into the caller's buffers.
 * Every output row is bitwise what bmx_scan returns on one GPU (a window's arithmetic never depends on the sharding). */
int bmx_scan_multi(const bmx_model *m, const double *A, int32_t nA, int64_t N, const double *genpos,
                   const int32_t *row, int64_t M, const double *test_gen, const int64_t *win_lo,
                   const int64_t *win_hi, double *clr, int32_t *ix, int32_t *ia, int32_t *iA,
                   int32_t *nsites, int32_t n_devices, const int32_t *devices);

/* ---- resident-context entry points ------------------------------------------------- */
/* Same computation split so that inputs stay resident in HBM across scans (one context per
 * process per GPU; the multi-GPU driver shards test sites across processes).
 * A context holds ONE model (selection table + A grid) and any number of chromosome SLOTS, each with its own site
 * arrays, test sites and results: the reference runs one input file per process (BalLeRMix+_v1.py:777-799); a
 * whole-genome run here selects slot k, sets chromosome k's sites and test sites, and scans the slots back to back on
 * the context's stream with the table built once.  Slot 0 exists from creation and is selected; set_sites, set_tests,
 * scan, fetch*, records, result_ptrs, last_scan_ms, scan_write, surface, surfaces and plan act on the selected slot. */
typedef struct bmx_ctx bmx_ctx;

int bmx_ctx_create(bmx_ctx **out, int device);
void bmx_ctx_destroy(bmx_ctx *c);
/* Build the selection table on the device (K1) and keep it resident.  Call order: set_model, then
 * set_sites, then set_tests; a new model discards the site and test arrays of EVERY slot (their
 * row indices belong to the old one), and new sites discard the slot's test sites (located in the old array).
 * The table's bit pattern follows the HOST's libm: scipy evaluates lgam's log with glibc's log, which is not correctly
 * rounded on ~0.015 % of arguments, so set_model evaluates this host's log on every argument the table build will use
 * and ships the exceptions to the device (bmx_math.h LogPatch).  The device table is therefore a function of the
 * model AND of the host library -- by design: it reproduces what scipy computes on this box. */
int bmx_ctx_set_model(bmx_ctx *c, const bmx_model *m, const double *A, int32_t nA);
/* Copy the site arrays of one chromosome to the device (and rank its rows by frequency for the scan
 * kernel's far-field moments). */
int bmx_ctx_set_sites(bmx_ctx *c, int64_t N, const double *genpos, const int32_t *row);
/* Copy test sites + window bounds to the device (and locate each test site).  win_lo == win_hi == NULL: every window
 * holds all sites of the chromosome, [0, N - 1] -- the reference's default mode (Scan._alpha, BalLeRMix+_v1.py:598-610);
 * the bounds are then written on the device, nothing is copied. */
int bmx_ctx_set_tests(bmx_ctx *c, int64_t M, const double *test_gen, const int64_t *win_lo,
                      const int64_t *win_hi);
/* Launch the scan (K2 + argmax finalisation) on the context's stream; asynchronous.
 * CLR range: the scan compares grid points by the binary exponent E and the mantissa of the window's likelihood ratio and keeps
 * E clamped to +-131071.  A winner AT the upper clamp may have been cut, so the argmax and the CLR are defined for E <= 131070,
 * |T| <= 2 ln 2 x 131070 = 1.817e5 per (window, A, grid point).  If any window of a scan has its winner at the clamp, that
 * slot's results are not handed out by the calls that return a scan: bmx_ctx_sync (on the selected slot), bmx_ctx_fetch, bmx_ctx_fetch_records,
 * bmx_ctx_fetch_profile, bmx_ctx_pack_records (any slot it packs), bmx_ctx_copy_records, bmx_ctx_scan_write (the rows it
 * appended are then not to be used), bmx_ctx_null_accumulate, bmx_ctx_locate_accumulate, bmx_scan and bmx_scan_multi return
 * BMX_E_LIMIT naming the range -- every time, until the slot is scanned again; other slots are unaffected.  Below neutral the
 * clamp is harmless: nothing with T <= 0 can win, and such a window comes out as "none" (clr +0.0, indices -1, nsites 0).
 * The off-grid calls (surface, surfaces, eval_points, ...) are plain sums and have no such limit.
 * NOT checked: bmx_ctx_result_ptrs and bmx_ctx_records (device addresses; nothing is read), and the calls that work on a
 * finished scan of the selected slot -- bmx_ctx_fetch_at, bmx_ctx_peaks, bmx_ctx_refine and what is built on them.  They read
 * the clamped clr / lin / nsites of a refused slot as they stand: call bmx_ctx_sync after the scan first, and go on only
 * where it returns BMX_OK. */
int bmx_ctx_scan(bmx_ctx *c);
/* Block until the stream is idle.  BMX_E_LIMIT if the selected slot's last scan left the CLR range (bmx_ctx_scan). */
int bmx_ctx_sync(bmx_ctx *c);
/* Milliseconds the last bmx_ctx_scan spent in the scan kernel(s), from HIP events
 * recorded on the context's stream (valid after bmx_ctx_sync). */
int bmx_ctx_last_scan_ms(bmx_ctx *c, double *ms);
/* Copy results of the last scan to host buffers of length M. */
int bmx_ctx_fetch(bmx_ctx *c, double *clr, int32_t *ix, int32_t *ia, int32_t *iA, int32_t *nsites);
/* Device addresses of the last scan's results: clr f64[M], lin i32[M] (linear grid index
 * (iA*nx + ix)*nab + ia, or -1), nsites i32[M].  Valid until the next set_tests/destroy;
 * used for the RCCL gather without a host round trip. */
int bmx_ctx_result_ptrs(bmx_ctx *c, void **d_clr, void **d_lin, void **d_nsites);
/* The same results as one array of M bmx_record: device address (for a single RCCL gather to the
 * writing rank) and host copy.  Valid until the next set_tests/destroy. */
int bmx_ctx_records(bmx_ctx *c, void **d_rec);
int bmx_ctx_fetch_records(bmx_ctx *c, bmx_record *rec);
/* Scan and stream: the rows of `scores.write(...)` (BalLeRMix+_v1.py:599-608) are appended to `path`
 * while the scan is still running.  Test sites go to the device `chunk` at a time (0: 65536; rounded to
 * whole workgroups, which keeps every result bit-identical to bmx_ctx_scan); each chunk's results are copied
 * to pinned host memory on a second stream and formatted/written by a host thread while the next chunk is
 * scanned.  phys[M], gen[M]: the first two columns of each row; xs/abs_/As: the grids' printed forms as for
 * bmx_write_rows (they must have the model's nx/nab/nA entries).  Results stay fetchable afterwards. */
int bmx_ctx_scan_write(bmx_ctx *c, const char *path, const int64_t *phys, const double *gen,
                       const char *xs, int nx, const char *abs_, int nab, const char *As, int nA, int64_t chunk);
/* Copy the resident tables back: psel/R as in bmx_lut_build (either may be NULL). */
int bmx_ctx_fetch_lut(bmx_ctx *c, double *psel_out, double *R_out);
/* Full likelihood surface of ONE test site: T_out[nA][nx][nab] = T(A, x, alpha_beta) in the grids'
 * iteration order (NaN where the window of that A is empty -- the reference `continue`s there,
 * BalLeRMix+_v1.py:458-459), nsites_out[nA] = window size per A (may be NULL).  The reference only
 * keeps the maximum and lists the surfaces as future work (v1:449-450).  Computed as a plain sum of
 * log1p(alpha*R), independently of the scan kernels' product form. */
int bmx_ctx_surface(bmx_ctx *c, double test_gen, int64_t win_lo, int64_t win_hi, double *T_out,
                    int32_t *nsites_out);
/* Surfaces of n test sites of the selected slot (indices into its M test sites, any order, repeats allowed):
 * T_out[n][nA][nx][nab] in the model's grid iteration order (NaN where the window at that A is empty),
 * nsites_out[n][nA] (may be NULL).  Each window bitwise what bmx_ctx_surface gives for its
 * (test_gen, win_lo, win_hi).  Needs model, sites and test sites (else BMX_E_STATE), no scan; an index outside
 * [0, M) or a NULL tests/T_out with n > 0 is BMX_E_INVALID; n == 0 succeeds and writes nothing.  Leaves scan
 * results, profiles, refinement, support, bootstrap, peak and null state of every slot untouched.  Blocks.
 * The list is processed in chunks of as many windows as keep the device output buffer at or below
 * BMX_SURFACES_CHUNK_BYTES (one window where a single surface is larger); each chunk is copied back before the
 * next is launched, so the device memory held does not grow with n.
 * These two entry points arrived without a bump of BMX_ABI_VERSION_MINOR (as the profile, refinement, support, bootstrap and
 * peak groups did): version 1.5 does not say whether a binary has them; look the symbol up (dlsym) to find out. */
#define BMX_SURFACES_CHUNK_BYTES (256LL << 20)
int bmx_ctx_surfaces(bmx_ctx *c, int64_t n, const int32_t *tests, double *T_out, int32_t *nsites_out);
/* Milliseconds the last bmx_ctx_surfaces spent in its kernels (HIP events on the context's stream). */
int bmx_ctx_surfaces_ms(bmx_ctx *c, double *ms);
/* Delete-block jackknife of the grid maximum of n test sites of the selected slot (listed as for bmx_ctx_surfaces: any order,
 * repeats allowed); the definition is ballermixplus_amd/influence.py.  Block of site i: i / block.  A window's block range runs
 * from the block of its first to the block of its last site that qualifies at the smallest A of the grid (empty without one).
 * Per window: T_max and lin* = the scan's argmax rule on the window's surface (bitwise bmx_ctx_surfaces'; lin = (iA * nx + ix) *
 * nab + ia, -1 and T_max 0 when nothing is > 0) and the number of qualifying sites at the smallest A.  Per block b of the range:
 * m = its qualifying sites at the smallest A, contrib = 2 S_b(lin*) (NaN when lin* < 0), L and lin = maximum and argmax, under
 * the same rule, of T - 2 S_b over the grid points whose A keeps a site outside the block (0 and -1 when nothing is > 0).
 * The results stay in the context until the next call: bmx_ctx_influence_count gives the number of listed windows, every
 * window's first block and the exclusive prefix offset[n + 1] of the windows' blocks in the per-block arrays;
 * bmx_ctx_fetch_influence copies t_max[n], lin[n], ns_min[n] and m, contrib, L, block_lin [offset[n]] (any pointer may be NULL).
 * A NULL context, n < 0, block < 1, a NULL list with n > 0 or an index outside [0, M) is BMX_E_INVALID and nothing is read;
 * without model, sites and test sites BMX_E_STATE; more than BMX_INFLUENCE_MAX_RESULTS blocks in one call BMX_E_LIMIT (list
 * fewer windows per call); count / fetch / ms before a successful call BMX_E_STATE.  n == 0 succeeds.  No atomics: a window's
 * numbers depend on that window and `block` alone.  Uses the surfaces' buffers and its own; leaves sites, test sites, scan
 * results, records, profiles, refinement, bootstrap, peak and null state of every slot untouched.  Blocks.
 * bmx_ctx_influence_ms: milliseconds the last call spent in its kernels (the surfaces' kernel among them).
 * Added without a bump of BMX_ABI_VERSION_MINOR, as the groups above: look the symbols up to find out. */
#define BMX_INFLUENCE_MAX_RESULTS (1LL << 26)
int bmx_ctx_influence(bmx_ctx *c, int64_t n, const int32_t *tests, int64_t block);
int bmx_ctx_influence_count(bmx_ctx *c, int64_t *n_windows, int64_t *first_block, int64_t *offset);
int bmx_ctx_fetch_influence(bmx_ctx *c, double *t_max, int32_t *lin, int32_t *ns_min, int32_t *m, double *contrib, double *L,
                            int32_t *block_lin);
int bmx_ctx_influence_ms(bmx_ctx *c, double *ms);
/* Goodness of fit of n test sites of the selected slot (listed as for bmx_ctx_surfaces: any order, repeats allowed): the observed
 * frequency spectrum by distance bin against the counts expected under ONE grid point per window and under neutrality; the
 * definition is ballermixplus_amd/fit.py.  Window q is test site tests[q] (tg, win_lo, win_hi) with the grid point lin[q] =
 * (iA * nx + ix) * nab + ia.  Its sites are the surfaces' sites at that A: win_lo <= i <= win_hi, z_i = A * |g_i - tg| <=
 * bmx_alpha_cut() (that single product), g_i != tg.
 *   gw[rows]   the caller's: the neutral probability (0 <= gw <= 1) of every admissible (count, sample size), 0 elsewhere
 *              (power.allowed_rows);  cls[rows] in [0, F): the frequency class of every table row
 *   edges[D-1] strictly ascending, finite, > 0;  bin(z) = #{k : z > edges[k]} (a site on an edge belongs to the lower bin; the
 *              last bin runs to the cut)
 *   for a site of size block j with rows a..b, alpha = exp(-z), R = the table's column of (ix, ia):
 *       m_r = gw[r] * (1 + alpha * R[r]) where gw[r] > 0, else 0 (the product is not formed: R is NaN where g is); a non-finite
 *       m_r counts as 0;  tot = sum_r m_r, p_r = m_r / tot;  neutral: q_r = gw[r] / sum_{a..b} gw
 *   O_out[n][D][F]     the sites per (bin, class of the site's own row)
 *   Esel_out[n][D][F]  sum over the bin's sites of sum_{r in class} p_r;   Eneu_out[n][D][F] the same of q_r
 *   skipped_out[n] (may be NULL): the sites whose tot or neutral total is not finite and > 0: counted in O, added to neither E
 * lin[q] < 0: O all 0, both E NaN, skipped 0.
 * fit_kernel: one workgroup of 256 per listed window, no atomics; a window's numbers depend on that window and the per-row
 * arrays alone (bitwise the same alone, in a list, or twice).  With 0 <= gw <= 1, R >= -1 and 0 < alpha <= 1 a product m_r is
 * non-finite exactly where R[r] is, whatever alpha: such a row is left out of the selected sums for every site (it stays in the
 * neutral ones), and the class sums are linear in alpha.  The prologue forms, per (size block j, class c) and in ascending
 * row order, Gn = sum gw, Gs = sum gw over the rows with a finite R and H = sum gw R over the same rows, and their totals over
 * the classes in ascending c; a site then adds (Gs[j][c] + alpha H[j][c]) / tot, tot = Gs[j][.] + alpha H[j][.], and Gn[j][c] /
 * Gn[j][.] to the cells of its bin, the sites of a cell in increasing site index.  The sums are staged in LDS while n_sizes *
 * (F + 1) * 24 bytes fit BMX_FIT_LDS_BYTES and in a per-window workspace in device memory past it (also with
 * bmx_ctx_set_variant(c, 1), for cross-checks).
 * BMX_E_INVALID and nothing is written: a NULL context, n < 0, a NULL tests / lin / gw / cls / edges (D > 1) / O_out / Esel_out /
 * Eneu_out with n > 0, an index outside [0, M), lin >= nA * nx * nab, F < 1, D < 1, D * F > BMX_FIT_MAX_CELLS, an edge that is
 * not finite, not > 0 or not above the one before, a cls outside [0, F), a gw outside [0, 1] (NaN included).  BMX_E_STATE
 * without model, sites and test sites: n < 0, F < 1, D < 1 and D * F > BMX_FIT_MAX_CELLS are refused before the state is looked
 * at (as bmx_ctx_influence's block < 1), every other argument after it; bmx_ctx_fit_ms (milliseconds the last call spent in its kernels) before a successful call
 * is BMX_E_STATE.  n == 0 succeeds.  Blocks.  Leaves sites, test sites, scan results, records, profiles, refinement, support,
 * bootstrap, peak, null, influence and locate state of every slot untouched.
 * Added without a bump of BMX_ABI_VERSION_MINOR, as the groups above: look the symbols up to find out. */
#define BMX_FIT_MAX_CELLS 256            /* D * F */
#define BMX_FIT_LDS_BYTES (40 << 10)     /* the prologue's sums of one window in LDS up to here */
int bmx_ctx_fit(bmx_ctx *c, int64_t n, const int32_t *tests, const int32_t *lin, const double *gw, const int32_t *cls, int32_t F,
                const double *edges, int32_t D, int32_t *O_out, double *Esel_out, double *Eneu_out,
                int32_t *skipped_out /* [n], may be NULL */);
int bmx_ctx_fit_ms(bmx_ctx *c, double *ms);
/* Conditional surfaces of n PAIRS on the selected slot: the surface of a candidate window given one fitted neighbouring locus;
 * the definition is ballermixplus_amd/conditional.py.  Pair q: the window of test site tests[q] (tg, win_lo, win_hi) and the
 * conditioning locus cond_test[q] (a test site of the same slot: position tc and its own window bounds) held at the grid point
 * cond_lin[q] = (iA_c * nx + ix_c) * nab + ia_c.  The candidate's sites at A are the surfaces' sites.  One of them is SHARED
 * iff max(win_lo[c], 0) <= i <= min(win_hi[c], N - 1), zc_i = A_c * |g_i - tc| <= bmx_alpha_cut() (that single product) and
 * g_i != tc; then d_i = exp(-zc_i) * R[ix_c][ia_c][row_i], for every other site d_i = 0.0 exactly (also with cond_test < 0 or
 * cond_lin < 0: no conditioning locus).  With alpha_i = exp(-A |g_i - tg|) and u_i = alpha_i / (1.0 + d_i),
 *     T_cond(A, x, abeta) = 2 * sum_i log1p(u_i * (R_i - d_i))      over the candidate's sites in increasing site index,
 * NaN where no site qualifies at that A.
 *   T_out[n][nA][nx][nab]  (may be NULL: the surfaces are then not copied back)
 *   nsites_out[n][nA]      the surfaces' count (may be NULL);   nshared_out[n][nA]  the shared sites among them (may be NULL)
 *   tmax_out[n], lin_out[n]  the scan's rule on each pair's T_cond (may be NULL): a value must be > 0, the larger wins, a tie
 *                          goes to the smaller linear index, NaN never wins; 0 and -1 when nothing is > 0
 * With every d_i == 0.0, u_i == alpha_i and R_i - 0.0 == R_i: T_cond, nsites, tmax and lin are then bitwise bmx_ctx_surfaces'
 * (and its argmax), nshared 0.  cond_surfaces_kernel: one workgroup of 256 per (pair, A, slice of 256 grid pairs), no atomics;
 * a pair's numbers depend on that pair alone (bitwise the same alone, in a list, or twice).  Chunked as bmx_ctx_surfaces:
 * device output at or below BMX_SURFACES_CHUNK_BYTES, each chunk copied back before the next launch.
 * BMX_E_INVALID and nothing is written: a NULL context, n < 0, a NULL tests / cond_test / cond_lin with n > 0, a tests index
 * outside [0, M), a cond_test outside [-1, M), a cond_lin >= nA * nx * nab.  BMX_E_STATE without model, sites and test sites;
 * bmx_ctx_cond_surfaces_ms (milliseconds the last call spent in its kernels) before a successful call is BMX_E_STATE.
 * n == 0 succeeds.  Blocks.  Uses the surfaces' device buffers and its own; leaves sites, test sites, scan results, records,
 * profiles, refinement, support, bootstrap, peak, null, influence, fit and locate state of every slot untouched.
 * Added without a bump of BMX_ABI_VERSION_MINOR, as the groups above: look the symbols up to find out. */
int bmx_ctx_cond_surfaces(bmx_ctx *c, int64_t n, const int32_t *tests, const int32_t *cond_test, const int32_t *cond_lin,
                          double *T_out /* [n][nA][nx][nab], may be NULL */, int32_t *nsites_out /* [n][nA], may be NULL */,
                          int32_t *nshared_out /* [n][nA], may be NULL */, double *tmax_out /* [n], may be NULL */,
                          int32_t *lin_out /* [n], may be NULL */);
int bmx_ctx_cond_surfaces_ms(bmx_ctx *c, double *ms);
/* A per-site BASELINE of any number of accepted loci on the selected slot, and the surfaces of n listed windows against it: the
 * device side of forward stepwise selection; the definition is ballermixplus_amd/stepwise.py.  The slot keeps d[N] (double) and
 * cnt[N] (int32): under the accepted loci site i follows g (1 + d_i), and cnt_i of them reach it.
 * bmx_ctx_baseline_reset: allocates the two arrays for the slot's N sites, or zeroes them (d = 0.0, cnt = 0).  BMX_E_INVALID: a
 *   NULL context; BMX_E_STATE without sites.  bmx_ctx_set_sites, _resample_sites and _plant_sites on a slot (and a new model)
 *   drop its baseline: the calls below are then BMX_E_STATE until the next reset.  Nothing else does: a baseline survives
 *   bmx_ctx_set_tests, scans, bmx_ctx_permute_rows and bmx_ctx_restore_rows (and bmx_ctx_select_slot away and back), and each
 *   locus keeps the d formed from the rows in force when it was added.
 * bmx_ctx_baseline_add: adds the locus "test site `test` held at the grid point lin = (iA_c * nx + ix_c) * nab + ia_c".  Its sites
 *   are the surfaces' sites at A_c: max(win_lo, 0) <= i <= min(win_hi, N - 1), z_i = A_c * |g_i - tc| <= bmx_alpha_cut() (that
 *   single product), g_i != tc.  Each of them gets
 *       d_i <- d_i + exp(-z_i) * (R[ix_c][ia_c][row_i] - d_i)        (no FMA contraction),   cnt_i <- cnt_i + 1;
 *   from d_i = 0.0 that is exp(-z_i) * R bit for bit: bmx_ctx_cond_surfaces' d.  *first, *last: the first and last site written,
 *   *n_written: how many (each may be NULL); a locus without a site writes nothing and returns first > last, n_written 0.
 *   baseline_add_kernel: one thread per site of the locus' range, plain loads and stores, no atomics.  Refusals, in this order:
 *   BMX_E_INVALID a NULL context; BMX_E_STATE without model, sites and test sites; BMX_E_STATE without a baseline; BMX_E_INVALID
 *   test outside [0, M); BMX_E_INVALID lin outside [0, nA * nx * nab).  A refused call writes nothing.
 * bmx_ctx_baseline_fetch: d_out[N], cnt_out[N] (either may be NULL).  BMX_E_INVALID: a NULL context; BMX_E_STATE without a
 *   baseline.
 * bmx_ctx_base_surfaces: window q is test site tests[q] (tg, win_lo, win_hi); its sites at A are the surfaces' sites.  With
 *   alpha_i = exp(-A |g_i - tg|) and u_i = alpha_i / (1.0 + d_i),
 *       T_base(A, x, abeta) = 2 * sum_i log1p(u_i * (R_i - d_i))      over the window's sites in increasing site index,
 *   NaN where no site qualifies at that A: bmx_ctx_cond_surfaces' expression with d read from the baseline.
 *     T_out[n][nA][nx][nab]  (may be NULL: the surfaces are then not copied back)
 *     nsites_out[n][nA]      the surfaces' count (may be NULL);   nshared_out[n][nA]  the sites among them with cnt_i > 0 (may be NULL)
 *     tmax_out[n], lin_out[n]  the scan's rule on each window's T_base (may be NULL), as bmx_ctx_cond_surfaces gives them
 *   Against the empty baseline T_base, nsites, tmax and lin are bitwise bmx_ctx_surfaces' (and its argmax) and nshared is 0; after
 *   ONE bmx_ctx_baseline_add they are bitwise bmx_ctx_cond_surfaces' of the pairs (window | that locus), nshared included.
 *   base_surfaces_kernel: one workgroup of 256 per (window, A, slice of 256 grid pairs), no atomics; a window's numbers depend on
 *   that window and the baseline alone (bitwise the same alone, in a list, or twice).  Chunked as bmx_ctx_surfaces: device output
 *   at or below BMX_SURFACES_CHUNK_BYTES, each chunk copied back before the next launch.  Refusals, in this order: BMX_E_INVALID
 *   a NULL context; BMX_E_INVALID n < 0; BMX_E_STATE without model, sites and test sites; BMX_E_INVALID a NULL tests with n > 0;
 *   BMX_E_STATE without a baseline; BMX_E_INVALID an index outside [0, M).  Nothing is written on refusal.  n == 0 succeeds.
 *   bmx_ctx_base_surfaces_ms (milliseconds the last call spent in its kernels) before a successful call is BMX_E_STATE.
 * All block.  They use the surfaces' device buffers and their own; apart from the selected slot's baseline they leave sites, test
 * sites, scan results, records, profiles, refinement, support, bootstrap, peak, null, influence, fit, conditional, sandwich and
 * locate state of every slot untouched.
 * Added without a bump of BMX_ABI_VERSION_MINOR, as the groups above: look the symbols up to find out. */
int bmx_ctx_baseline_reset(bmx_ctx *c);
int bmx_ctx_baseline_add(bmx_ctx *c, int32_t test, int32_t lin, int64_t *first /* may be NULL */, int64_t *last /* may be NULL */,
                         int32_t *n_written /* may be NULL */);
int bmx_ctx_baseline_fetch(bmx_ctx *c, double *d_out /* [N], may be NULL */, int32_t *cnt_out /* [N], may be NULL */);
int bmx_ctx_base_surfaces(bmx_ctx *c, int64_t n, const int32_t *tests, double *T_out /* [n][nA][nx][nab], may be NULL */,
                          int32_t *nsites_out /* [n][nA], may be NULL */, int32_t *nshared_out /* [n][nA], may be NULL */,
                          double *tmax_out /* [n], may be NULL */, int32_t *lin_out /* [n], may be NULL */);
int bmx_ctx_base_surfaces_ms(bmx_ctx *c, double *ms);
/* The pieces of the sandwich (Godambe) variance H^-1 J H^-1 of n listed windows on the selected slot, each at a point the caller
 * gives; the definition is ballermixplus_amd/sandwich.py.  Window q: test site tests[q] (tg, win_lo, win_hi) at (A[q], x[q],
 * abeta[q]).  Its sites are the surfaces' sites at that A: z_i = A * |g_i - tg| <= bmx_alpha_cut(), g_i != tg.  Coordinates
 * (u, x, v) = (ln A, x, ln alpha_beta).  With alpha_i = exp(-z_i), R(row | x, abeta) the off-grid table entry bmx_ctx_refine_R
 * returns, rv = exp(hv) (the host's exp, once per call),
 *     R_i = R(row_i | x, abeta),  Rx_i = (R(row_i | x + hx, abeta) - R(row_i | x - hx, abeta)) / (2 hx),
 *     Rv_i = (R(row_i | x, abeta * rv) - R(row_i | x, abeta / rv)) / (2 hv),  D_i = 1 + alpha_i R_i,
 *     s_i = (-z_i alpha_i R_i / D_i, alpha_i Rx_i / D_i, alpha_i Rv_i / D_i).
 * A site whose D_i is not > 0 or whose s_i is not finite is SKIPPED: counted in nsites and nskipped, it enters no sum.
 *   T_out[n]        2 * sum log1p(alpha_i R_i) over the used sites; -inf without one
 *   g_out[n][3]     sum s_i
 *   H_out[n][6]     sum s_i s_i^T, as (uu, ux, uv, xx, xv, vv)
 *   J_out[n][6]     sum over the blocks b = i / block (the site index in the slot's array) of S_b S_b^T, S_b = the sum of s_i over
 *                   the block's used sites in this window; the same six entries
 *   nsites_out[n]   the window's sites at A (the surfaces' count), nskipped_out[n] the skipped among them,
 *   nblocks_out[n]  the blocks with a used site
 * Every output may be NULL.  An empty window: T = -inf, the counts 0, g, H and J all 0.0.
 * sandwich_kernel: one workgroup of 256 per window, the workspace of the refinement's kernels (five table columns of the rows the
 * window references, in LDS or in a slab), blocks of fewer than 64 sites one thread each, larger ones one wave each; no atomics,
 * every sum in a fixed order: a window's 16 doubles depend on that window, its point, block, hx and hv alone (bitwise the same
 * alone, in a list, twice, in any order), and with block = 1 J is H bit for bit.  At most BMX_SANDWICH_CHUNK_WINDOWS windows per
 * launch: the list is judged as a whole first, then each chunk's points are formed and uploaded, its kernel runs and its outputs
 * are copied back before the next chunk, so host and device hold one chunk's arrays whatever n is.
 * BMX_E_INVALID and nothing is written: a NULL context, n < 0, block < 1, hx or hv not finite and > 0, a NULL tests / A / x /
 * abeta with n > 0, an index outside [0, M), an A or abeta not finite and > 0, x - hx <= 0 or x + hx >= 1, abeta / rv or
 * abeta * rv not finite and > 0.  BMX_E_STATE without model, sites and test sites (n < 0, block and the steps are refused before
 * the state is looked at); BMX_E_LIMIT for n > BMX_SANDWICH_MAX_WINDOWS.  n == 0 succeeds.  Blocks.  Needs no scan; leaves
 * sites, test sites, scan results, records, profiles, refinement, support, bootstrap, peak, null, influence, fit and locate
 * state of every slot untouched.  bmx_ctx_sandwich_ms (milliseconds the last call spent in its kernels) before a successful
 * call is BMX_E_STATE.
 * bmx_ctx_refine_R: R_out[rows] = R(row | x, abeta) of every table row of the model, the refinement's off-grid arithmetic
 * (refine_R; NaN for a row without a neutral probability), one thread per row.  bmx_ctx_eval_points' argument rules: a NULL
 * argument, x outside (0, 1) or abeta not finite and > 0 is BMX_E_INVALID, without model, sites and test sites BMX_E_STATE.
 * Blocks.
 * Added without a bump of BMX_ABI_VERSION_MINOR, as the groups above: look the symbols up to find out. */
#define BMX_SANDWICH_MAX_WINDOWS (1LL << 24)
#define BMX_SANDWICH_CHUNK_WINDOWS (1LL << 18)
int bmx_ctx_sandwich(bmx_ctx *c, int64_t n, const int32_t *tests, const double *A, const double *x, const double *abeta,
                     int64_t block, double hx, double hv, double *T_out /* [n] */, double *g_out /* [n][3] */,
                     double *H_out /* [n][6] */, double *J_out /* [n][6] */, int32_t *nsites_out /* [n] */,
                     int32_t *nskipped_out /* [n] */, int32_t *nblocks_out /* [n] */);
int bmx_ctx_sandwich_ms(bmx_ctx *c, double *ms);
int bmx_ctx_refine_R(bmx_ctx *c, double x, double abeta, double *R_out /* [rows] */);
/* Choose the scan kernel variant (0 = default). For A/B measurements only. */
int bmx_ctx_set_variant(bmx_ctx *c, int variant);
/* Select (creating it on first use) chromosome slot `slot`, 0 <= slot < 4096. */
int bmx_ctx_select_slot(bmx_ctx *c, int32_t slot);
/* Number of slot indices in use (highest selected slot + 1). */
int bmx_ctx_slot_count(bmx_ctx *c);
/* The records of every slot that holds scan results, in slot order, back to back: the whole genome's rows with one
 * call -- to host memory (dst_on_device = 0), or to device memory of this context's GPU (1), where ONE gather then
 * moves them to the writing rank.  dst: room for `cap` records; *n_out (may be NULL): records written.  Blocks. */
int bmx_ctx_pack_records(bmx_ctx *c, void *dst, int64_t cap, int32_t dst_on_device, int64_t *n_out);
/* The SELECTED slot's M records to device memory of this context's GPU (room for `cap` >= M records), device to device on the
 * context's stream; blocks until done.  What a sharded run gathers per input file when the context also holds other slots. */
int bmx_ctx_copy_records(bmx_ctx *c, void *dst_device, int64_t cap);
/* What the scan of the selected slot launches (valid once its test sites are set): *J = test sites per wave-group (0: one
 * test site per wave), *use_lds = 1 if the R slice is read from LDS, *mode = 4 prepared pipeline (prep_kernel +
 * clr_scan_prepared_kernel), 5 prepared pipeline with one test site per wave (prep_solo_kernel + clr_scan_solo_kernel, *J = 1:
 * sparse or unsorted test sites), 0..3 the round-2 grouped forms, -1 the round-2 per-site kernel; *stream_bytes = bytes of the prepared
 * per-group streams of all test sites (0 otherwise).  Any pointer may be NULL. */
int bmx_ctx_plan(bmx_ctx *c, int32_t *J, int32_t *use_lds, int32_t *mode, int64_t *stream_bytes);
/* Where the selected slot's scan is cut into launches: offs[i] = index of the first test site of launch range i (offs[0] = 0;
 * range i ends where range i + 1 begins, the last one at M).  At most `cap` entries are written; *n_out = number of ranges.
 * A window's result must not depend on the cut -- the parity tests recompute the windows on either side of every cut
 * independently.  Valid once the test sites are set. */
int bmx_ctx_launch_ranges(bmx_ctx *c, int64_t *offs, int32_t cap, int32_t *n_out);

/* ---- permutation null (opt-in; the CLI's --nullPerm) ------------------------------------------------------------------
 * A null distribution of the CLR on the user's own sites: the (k, n) rows of the selected slot's sites are permuted on the
 * device while positions, windows, test sites and the selection table stay; each replicate is scanned with bmx_ctx_scan and
 * its exceedances and maximum are accumulated on the device.  Under the composite likelihood's assumption that sites (or
 * blocks of sites) are exchangeable; LD beyond a block and demography are not modelled.
 *
 * permute_rows: row[i] = given_row[sigma(i)], sigma the keyed block permutation of ballermixplus_amd/null.py
 * (block_permutation: blocks of `block` consecutive sites moved intact by an 8-round Feistel network with cycle walking over
 * the N / block whole blocks, the N mod block tail in place).  A pseudorandom permutation, not an exactly uniform shuffle.
 * The first call after set_sites keeps the given rows on the device (2 or 4 bytes per site); later calls permute those, not
 * the previous permutation.  restore_rows: back to the rows given to set_sites (nothing to do if never permuted).  Both are
 * asynchronous on the context's stream and make the next scan redo its plan and the prepared pipeline's counting pass.
 * block < 1: BMX_E_INVALID.  set_sites drops the kept rows. */
int bmx_ctx_permute_rows(bmx_ctx *c, uint64_t key, int64_t block);
int bmx_ctx_restore_rows(bmx_ctx *c);
/* The selected slot's last scan results become the observed CLR and the M exceedance counts are zeroed (12 bytes per test
 * site).  BMX_E_STATE before a scan; set_tests (and so set_sites / set_model) drops this state. */
int bmx_ctx_null_begin(bmx_ctx *c);
/* After the scan of one replicate: counts[t] += (clr[t] >= observed clr[t]); *max_out (may be NULL) = the maximum CLR over
 * the slot's M test sites (two-pass reduction: deterministic, no atomics).  Blocks.  BMX_E_STATE without null_begin or when no
 * scan was launched since null_begin / the previous accumulate. */
int bmx_ctx_null_accumulate(bmx_ctx *c, double *max_out);
/* counts[M] (may be NULL): exceedances per test site; *replicates (may be NULL): accumulates since null_begin.  Blocks. */
int bmx_ctx_null_fetch(bmx_ctx *c, int32_t *counts, int32_t *replicates);

/* ---- profile likelihoods (opt-in; the CLI's --profiles) -----------------------------------------------------------------
 * For test site t and grid value v of a parameter P in {A, x, alpha_beta}: profile_P[t][v] = max(0, the largest T over the
 * other two grids with P = v) -- the CLR the scan reports at t when P is fixed to v (0 where no grid point has T > 0).  The
 * kernels compare the exact (mantissa, exponent) keys of the products and convert each maximum with the conversion of the
 * CLR, so max_v profile_P[t][v] == clr[t] bit for bit.
 *
 * set_profiles: the set (0: off, the default) that later scans of every slot compute, bmx_ctx_scan and bmx_ctx_scan_write
 * alike.  Off releases every profile buffer.  While on, a slot holds 8 * (nA + nx + nab) bytes per test site and the scan's
 * launch ranges are kept short enough for the keys of one range to fit 1 GiB.  Plans on the round-2 kernels (tables of 4 GiB
 * or more, 2^31 sites or more, diagnostic variants) have no profile form: their scan fails with BMX_E_LIMIT.
 * fetch_profile: one BMX_PL_* of the selected slot's last scan, f64 [M][n] with n = nA, nx or nab, the model's grid order.
 * Blocks.  BMX_E_STATE when that scan ran without this profile; set_tests (and so set_sites / set_model) drops them. */
enum { BMX_PL_A = 1, BMX_PL_X = 2, BMX_PL_ABETA = 4 };
int bmx_ctx_set_profiles(bmx_ctx *c, int32_t which);
int bmx_ctx_fetch_profile(bmx_ctx *c, int32_t which, double *out);

/* ---- off-grid refinement of each window's maximum (opt-in; the CLI's --refine; ballermixplus_amd/refine.py) --------------
 * A deterministic compass search in (ln A, x, ln alpha_beta) from the scan's argmax, on the exact T of the reference at
 * arbitrary parameter values (the selection probabilities of each candidate are computed on the device as the table's are).
 * A coordinate is free when the model's grid has two or more distinct values of it; the search stays inside the hull of the
 * grid.  A refined row is reported only where its T is strictly greater than the scan's CLR, so the refined CLR is >= the
 * scan's bit for bit.  Each window's result depends on that window alone.  A local polish, not a global optimiser. */
/* T at a caller-given point per test site of the selected slot (the refinement's arithmetic): A/x/abeta[M], T_out[M]
 * (-inf where the window at that A is empty), nsites_out[M] (may be NULL).  Blocks. */
int bmx_ctx_eval_points(bmx_ctx *c, const double *A, const double *x, const double *abeta, double *T_out, int32_t *nsites_out);
/* Refine the selected slot's last scan (windows with lin >= 0 and clr >= min_clr); asynchronous on the context's stream.
 * BMX_E_STATE before a scan.  set_tests / set_sites / set_model drop the results. */
int bmx_ctx_refine(bmx_ctx *c, double min_clr);
/* M rows: clr, A, x, abeta, nsites of the refined (or unchanged) result; rounds[t] = -1 not refined, else rounds run.  Blocks.
 * Rows without a grid result carry NaN in A, x and abeta.  Any pointer may be NULL. */
int bmx_ctx_fetch_refined(bmx_ctx *c, double *clr, double *A, double *x, double *abeta, int32_t *nsites, int32_t *rounds);

/* ---- support intervals around each refined maximum (opt-in; the CLI's --support; ballermixplus_amd/support.py) -----------
 * Per window and free coordinate k (0: A, 1: x, 2: alpha_beta), the range over which the profile of T -- T maximised over the
 * other free coordinates by the refinement's compass search with k held -- stays >= T* - drop, T* being T at the refined point.
 * Each end is found by a doubling walk from the refined point and a bisection to a fixed tolerance.  Each window's result
 * depends on that window alone.  The profile searches are local, so an interval may be narrower than the true one. */
/* Support intervals of the windows of the selected slot's last refinement (bmx_ctx_refine after the last scan; else
 * BMX_E_STATE) with a refined CLR >= min_clr; drop finite and > 0.  Asynchronous on the context's stream.  A new scan,
 * refinement, set_tests / set_sites / set_model drop the results. */
int bmx_ctx_support(bmx_ctx *c, double drop, double min_clr);
/* Per task q = (t * 3 + k) * 2 + side (side 0: the lower end, 1: the upper end), M * 6 of each:
 *   end[q] (natural units), witness[q * 3 + j] (the inside point at the end: A, x, alpha_beta) and witness_T[q] (its T),
 *   outside[q * 3 + j] / outside_T[q] (the nearest point found outside; NaN when censored), censored[q] (1: the end sits on
 *   the grid's hull), rounds[q] (compass rounds run; -1: not computed -- window not refined, below min_clr, or k fixed),
 *   evals[q] (profile evaluations).
 * Per test site t (M of each): T_star[t] (T at the refined point) and T_best[t] (the largest T any profile search of the window
 * saw, T* included); NaN where nothing was computed.  Blocks.  Any pointer may be NULL. */
int bmx_ctx_fetch_support(bmx_ctx *c, double *end, double *witness, double *witness_T, double *outside, double *outside_T,
                          int32_t *censored, double *T_star, double *T_best, int32_t *rounds, int32_t *evals);

/* ---- block bootstrap of each refined maximum (opt-in; the CLI's --boot; ballermixplus_amd/boot.py) ----------------------
 * Replicate r re-weights the sites in blocks of `block` consecutive sites (block b = site index / block) with Poisson(1)
 * weights w(key_r, b) in 0..20 drawn from a counter-based hash by integer comparisons, and repeats the refinement's compass
 * search from the refined point on T_w = 2 * sum_i w_i log1p(alpha_i R_i) over the sites of T that have w_i > 0 (-inf: no such
 * site, or a sum that is not finite).  Centre, initial steps, tolerances, rounds, free coordinates and hull are those of the
 * support intervals' centre and of the refinement.  One workgroup per (window, replicate); a result depends on its window
 * and its key alone.  A local search: a replicate does not find a higher maximum elsewhere on its surface. */
/* T_w at a caller-given point per test site of the selected slot under the weights of (key, block): A/x/abeta[M], T_out[M],
 * wsum_out[M] (may be NULL) = the sum of the weights of the window's sites at that A.  block >= 1, else BMX_E_INVALID.
 * Blocks. */
int bmx_ctx_eval_points_weighted(bmx_ctx *c, uint64_t key, int64_t block, const double *A, const double *x, const double *abeta,
                                 double *T_out, int64_t *wsum_out);
/* Bootstrap the windows of the selected slot's last refinement (bmx_ctx_refine after the last scan; else BMX_E_STATE) that were
 * refined and have a refined CLR >= min_clr: R replicates each, replicate r under keys[r].  R < 1, block < 1 or a NaN min_clr:
 * BMX_E_INVALID.  At most BMX_BOOT_MAX_RESULTS (window, replicate) results (44 bytes each on the device): more is BMX_E_LIMIT,
 * to be met with a higher min_clr (the CLI's --bootMin) or fewer replicates.  The call waits for the refinement to learn the
 * number of selected windows; the bootstrap itself is asynchronous on the context's stream.  A new scan, refinement,
 * set_tests / set_sites / set_model drop the results. */
#define BMX_BOOT_MAX_RESULTS (1LL << 26)
int bmx_ctx_boot(bmx_ctx *c, const uint64_t *keys, int32_t R, int64_t block, double min_clr);
/* *n_sel (may be NULL) = the number of windows of the last bootstrap, *R (may be NULL) = its replicates.  BMX_E_STATE
 * without one. */
int bmx_ctx_boot_count(bmx_ctx *c, int64_t *n_sel, int32_t *R);
/* window[n_sel]: the bootstrapped test sites, ascending.  Per (window q, replicate r) at q * R + r, n_sel * R of each: the final
 * point A, x, abeta (natural units), T (T_w there; -inf: the replicate is not ok), T_centre (T_w at the refined point, the
 * search's first evaluation) and rounds (compass rounds run).  Blocks.  Any pointer may be NULL. */
int bmx_ctx_fetch_boot(bmx_ctx *c, int32_t *window, double *A, double *x, double *abeta, double *T, double *T_centre,
                       int32_t *rounds);

/* ---- resampled sites and the position bootstrap (opt-in; the CLI's --locate; ballermixplus_amd/locate.py) ----------------
 * An integer-weighted composite likelihood is the plain one of the site array in which site i stands w_i times, at its position
 * and with its table row.  So a bootstrap replicate of the whole grid scan -- a global argmax per test position, not a local
 * search -- is bmx_ctx_scan on a resampled site array: the scan kernels run unchanged (they already handle runs of sites at one
 * position, test positions that are no site, and exclude every site at the test position).  These entry points build that
 * array on the device and reduce each replicate's track to one argmax per peak.  They arrived without a bump of
 * BMX_ABI_VERSION_MINOR, as the groups above did: look the symbols up to find out whether a binary has them. */
/* The SELECTED slot receives the resampled sites of slot src_slot: site i of src_slot w(key, i / block) times (the bootstrap's
 * weights, 0..20), order kept, weight-0 sites dropped -- np.repeat(genpos, w), np.repeat(row, w).  Built on the device (tile
 * sums of the weights, a prefix of the sums, an expansion that also counts the copies per table row; no workgroup waits for
 * another); the counts and the two end positions come back to the host, which derives from them what bmx_ctx_set_sites derives
 * from the host arrays.  Afterwards the selected slot is in exactly the state bmx_ctx_set_sites leaves for the expanded arrays
 * (its test sites are discarded); src_slot is read only and keeps its sites, test sites, results and every other state.  The
 * rows taken are the ones src_slot holds now (a permutation by bmx_ctx_permute_rows included).  *N_out (may be NULL) = the
 * number of resampled sites N'.  N' == 0 is BMX_OK and leaves the selected slot without sites; N' >= 2^31 - 1 is BMX_E_LIMIT
 * (the slot is left without sites); src_slot == the selected slot, a slot index out of range or block < 1 is BMX_E_INVALID; a
 * source without sites is BMX_E_STATE.  Blocks. */
int bmx_ctx_resample_sites(bmx_ctx *c, int32_t src_slot, uint64_t key, int64_t block, int64_t *N_out);
/* The selected slot's site arrays as the device holds them: genpos_out[N], row_out[N] (table rows as int32); either may be
 * NULL.  BMX_E_STATE without sites.  Blocks. */
int bmx_ctx_fetch_sites(bmx_ctx *c, double *genpos_out, int32_t *row_out);
/* The position bootstrap's reduction, on the selected slot (the replicates' slot).  locate_begin: K >= 1 peaks with inclusive
 * ranges lo[k] <= hi[k] into the slot's test sites (ranges may overlap), R >= 1 replicates; every result starts as (row -1,
 * CLR 0).  At most BMX_LOCATE_MAX_RESULTS (peak, replicate) results (12 bytes each on the device), else BMX_E_LIMIT.  Every
 * replicate sets the slot's sites and test sites anew, so this state outlives set_sites / resample_sites / set_tests; a new
 * locate_begin or a new model ends it.
 * locate_accumulate: after the scan of replicate r (0 <= r < R), one wave per peak reduces the scan's results over the peak's
 * range to (row, CLR): the row with the largest CLR among the rows with a grid result (lin >= 0), the earliest such row on
 * equality, exact FP64 comparisons; (-1, 0) when no row of the range has a grid result.  BMX_E_STATE without locate_begin or
 * when no scan was launched since locate_begin / the previous accumulate; BMX_E_INVALID when a range reaches past the slot's
 * test sites.  Blocks, and checks the scan's device status as null_accumulate does.
 * fetch_locate: row_out[R][K] (indices into the slot's test sites) and clr_out[R][K]; either may be NULL.  Blocks. */
#define BMX_LOCATE_MAX_RESULTS (1LL << 26)
int bmx_ctx_locate_begin(bmx_ctx *c, int32_t K, const int32_t *lo, const int32_t *hi, int32_t R);
int bmx_ctx_locate_accumulate(bmx_ctx *c, int32_t r);
int bmx_ctx_fetch_locate(bmx_ctx *c, int32_t *row_out, double *clr_out);

/* ---- planted sites: the power analysis (opt-in; the CLI's --power; ballermixplus_amd/power.py holds the definition) -------
 * The composite likelihood is a generative model.  A site i in reach of a planted locus at position c -- the scan's own
 * predicate A |g_i - c| <= bmx_alpha_cut() and its exclusion g_i != c -- redraws its derived count from the mixture the scan
 * fits at ONE grid point (iA, ix, ia) of the model:
 *     m_k = max(0, gw[r] * (1 + alpha_i * R[ix][ia][r])),  r = row_off[j] + k over the rows of the site's sample size j,
 *     alpha_i = exp(-A |g_i - c|);  a non-finite m_k counts as 0;  total = sum_k m_k in ascending k;
 *     u_i = (mix(key ^ mix(i)) >> 11) * 2^-53  (splitmix64, i the site's index);
 *     the new row is the first k whose running sum exceeds u_i * total (the last k with m_k > 0 if rounding leaves none);
 *     total not finite or not > 0: the row stays.
 * gw[rows] is the caller's: the neutral probability of every admissible (count, sample size), 0 elsewhere.  Positions and sample
 * sizes never change.  The array is then scanned by the unchanged kernels.  These entry points arrived without a bump of
 * BMX_ABI_VERSION_MINOR, as the groups above did: look the symbols up to find out whether a binary has them. */
/* The SELECTED slot receives src_slot's positions and the rows src_slot holds now (a permutation by bmx_ctx_permute_rows
 * included), with the sites in reach of centre[0 .. K) redrawn under key.  Afterwards the selected slot is in exactly the state
 * bmx_ctx_set_sites leaves for those arrays (its test sites are discarded); src_slot is read only.  first_out[k] / count_out[k]
 * (may be NULL): the run of sites with A |g_i - c_k| <= bmx_alpha_cut() (it holds the sites AT c_k, which are not redrawn);
 * *changed_out (may be NULL): the sites whose row changed.  K == 0 succeeds and copies the source.  src_slot == the selected
 * slot, indices outside the grids or the slots, K < 0, a centre that is not finite, centres that do not ascend with
 * A (c[k+1] - c[k]) > 2.000001 bmx_alpha_cut() (no site is in reach of two), and a NULL gw or centre with K > 0 are
 * BMX_E_INVALID; no model, or a source without sites, is BMX_E_STATE.  Blocks. */
int bmx_ctx_plant_sites(bmx_ctx *c, int32_t src_slot, uint64_t key, int32_t K, const double *centre, int32_t iA, int32_t ix,
                        int32_t ia, const double *gw /* [rows] */, int32_t *first_out, int32_t *count_out /* [K], may be NULL */,
                        int64_t *changed_out /* may be NULL */);
/* Milliseconds the last bmx_ctx_plant_sites spent on the device, the two copies of the arrays included (HIP events). */
int bmx_ctx_plant_ms(bmx_ctx *c, double *ms);
/* The selected slot's last scan results at tests[n] (indices into its M test sites, any order, repeats allowed), gathered on
 * the device: clr, lin (linear grid index, -1: none) and nsites, any of which may be NULL.  An index of -1 gives (0, -1, 0);
 * other indices outside [0, M) are BMX_E_INVALID; before a scan the call is BMX_E_STATE; n == 0 succeeds.  Blocks. */
int bmx_ctx_fetch_at(bmx_ctx *c, int64_t n, const int32_t *tests, double *clr, int32_t *lin, int32_t *nsites);

/* ---- peaks of the CLR track (opt-in; the CLI's --peaks; ballermixplus_amd/peaks.py holds the definition) ------------------
 * The track: rows t = 0 .. M-1 with non-decreasing positions g and values c.  Row t is an APEX iff c_t > 0, c_t >= min_clr and no
 * other row s with g_t - g_s <= sep and g_s - g_t <= sep has c_s > c_t, or c_s == c_t and s < t (a local-maximum rule, not greedy
 * clumping).  Between consecutive apexes the SADDLE is the first row of smallest c strictly between them (none when they are
 * adjacent rows).  The EXTENT of an apex a is the maximal run of rows around it with c >= frac * c_a, cut strictly inside the
 * saddles on either side (adjacent apexes end at their own rows).  Exact FP64 comparisons throughout: the host restatement in
 * peaks.py gives the same rows.  Errors of this group: a NaN argument, sep < 0, frac outside (0, 1], no scan yet, unsorted
 * positions, and a refinement restricted to apexes without a peak call on the slot's last scan are all BMX_E_INVALID. */
/* Peaks of the selected slot's last scan: g = its test positions, c = its CLR.  Blocks. */
int bmx_ctx_peaks(bmx_ctx *c, double sep, double min_clr, double frac);
/* The same kernels on a track given by the caller: gen[M], clr[M] (M >= 0; no NaN value, finite non-decreasing positions).
 * Needs neither model nor sites; the result replaces the selected slot's peak call.  Blocks. */
int bmx_ctx_peaks_track(bmx_ctx *c, int64_t M, const double *gen, const double *clr, double sep, double min_clr, double frac);
/* *n_peaks (may be NULL) = the number of apexes of the selected slot's last peak call, *M (may be NULL) = the rows of its track.
 * BMX_E_STATE without one; set_tests / set_sites / set_model drop it. */
int bmx_ctx_peak_count(bmx_ctx *c, int64_t *n_peaks, int64_t *M);
/* Per apex, in row order, n_peaks of each: its row, the first and last row of its extent, and the saddle rows below and above it
 * (-1: none -- the end of the track, or the neighbouring apex is the adjacent row).  Any pointer may be NULL. */
int bmx_ctx_fetch_peaks(bmx_ctx *c, int32_t *row, int32_t *lo, int32_t *hi, int32_t *saddle_lo, int32_t *saddle_hi);
/* Milliseconds of the context's last peak call on the device, first kernel to last (HIP events on the context's stream; the
 * eight-byte read-back of the apex count that sizes the results lies in between). */
int bmx_ctx_peaks_ms(bmx_ctx *c, double *ms);
/* on != 0: later bmx_ctx_refine calls of this context refine only the windows that are apexes of their slot's peak call, which must
 * be a bmx_ctx_peaks on the slot's last scan (else the refinement fails with BMX_E_INVALID); min_clr applies on top.  Support
 * intervals and bootstrap follow, as they only touch refined windows.  Off by default. */
int bmx_ctx_refine_at_peaks(bmx_ctx *c, int32_t on);

/* ---- the final gather over RCCL, inside the library (north_star: "only a final RCCL gather over xGMI") --
 * One process per GPU, each with its own context.  Rank 0 makes an id (bmx_comm_unique_id: 128 bytes) and hands it to the other
 * ranks by whatever channel the caller has (MPI, a file, a socket, torch's store); every rank then calls bmx_comm_create with
 * its context -- collectively, like ncclCommInitRank.  librccl.so is opened when the first of these functions is called
 * (dlopen): a program that never gathers never loads it.  No torch, no Python. */
typedef struct bmx_comm bmx_comm;
#define BMX_COMM_ID_BYTES 128
int bmx_comm_unique_id(char *id /* BMX_COMM_ID_BYTES */);
int bmx_comm_create(bmx_comm **out, bmx_ctx *c, const char *id, int32_t rank, int32_t world);
void bmx_comm_destroy(bmx_comm *cm);
/* ONE gather of the records of every slot of the communicator's context that holds results (slot order, as
 * bmx_ctx_pack_records) to rank `root`: the packed bmx_record buffers move device to device in one group of ncclSend /
 * ncclRecv on the context's stream -- every peer has its own xGMI link to the root, nothing goes to the other ranks.
 * counts[world]: the number of records of every rank (each rank knows them all: test sites are dealt deterministically).
 * On the root, dst_host (may be NULL) receives all records, rank after rank, and *d_out (may be NULL) the device address of
 * the same array (valid until the next gather or bmx_comm_destroy); other ranks ignore both.  Collective; blocks until done. */
int bmx_comm_gather_records(bmx_comm *cm, const int64_t *counts, int32_t root, bmx_record *dst_host, void **d_out);

/* ---- input ingest (host only) ------------------------------ */
/* Native reader of the 4-column input that InputData.readCounts / readPolyCalls parse line by
 * line in Python (BalLeRMix+_v1.py:80-131): header skipped, tab-separated physPos, genPos, k, n.
 * bmx_input_count returns the number of data lines; bmx_input_parse fills caller-allocated arrays
 * of that length: phys = int(float(col0)), coord = float(col[pos_col]) (pos_col 0: physical,
 * 1: genetic), k = int(col2), n = int(col3).  Bit-identical to the Python parse (strtod). */
int bmx_input_count(const char *path, int64_t *n_out);
int bmx_input_parse(const char *path, int64_t N, int pos_col, int64_t *phys, double *coord,
                    int64_t *k, int64_t *n);

/* ---- output (host only) ------------------------------------- */
/* Appends M result rows to `path` in the reference's format (BalLeRMix+_v1.py:607), floats printed
 * exactly as Python's repr().  xs/abs/As: the grids' printed forms, '\0'-separated, in grid order.
 * iA[t] < 0 writes the all-zero row (v1:451).  Integer physPos only (the --noCenter mode prints a
 * float there and stays in Python). */
int bmx_write_rows(const char *path, int64_t M, const int64_t *phys, const double *gen, const double *clr,
                   const int32_t *ix, const int32_t *ia, const int32_t *iA, const int32_t *nsites,
                   const char *xs, int nx, const char *abs_, int nab, const char *As, int nA);
/* The same rows from 16-byte records as a sharded run gathers them on the writing rank: per_rank[r] = the records of rank
 * r's test sites in its own order, test sites dealt to the `world` ranks in blocks of `block` consecutive test sites
 * round-robin.  world = 1 (block: any value >= 1): M records in output order.  Appends to `path`. */
int bmx_write_records(const char *path, int64_t M, const int64_t *phys, const double *gen,
                      const bmx_record *const *per_rank, int32_t world, int64_t block,
                      const char *xs, int nx, const char *abs_, int nab, const char *As, int nA);
/* repr(v) as Python prints it, into buf (>= 32 bytes); returns the length. */
int bmx_py_repr(double v, char *buf);

#ifdef __cplusplus
}
#endif
#endif /* BMXSCAN_H */
