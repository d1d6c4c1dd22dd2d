/*
 * pbbi.h -- C ABI of libpbbi.so, the MI355X (gfx950) ensemble-HMC hot path.
 *
 * Drop-in boundary.  The reference (Anton-Le/PhysicsBasedBayesianInference) has
 * no FFI layer: its boundary is the Python class API of src/{ensemble,
 * integrator,HMC,potential}.py.  Each entry point below replaces the arithmetic
 * behind one of those methods (cited as file:line relative to the reference
 * root) and is what a ctypes binding in those files would call -- see
 * INTEGRATION.md for the stub a maintainer would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only; no exceptions cross the ABI.
 *   - Every function returns an int status (PBBI_OK = 0, negative = error
 *     class); pbbi_last_error() returns a thread-local message for the last
 *     failure on the calling thread.
 *   - State arrays are DEVICE pointers owned by the caller (e.g.
 *     torch.Tensor.data_ptr()); the library never frees or retains them past
 *     the call.  Layout: (D, N) "ensemble-major" -- element (d, n) at
 *     [d*ldn + n], chain index n fastest, ldn >= N.  This is the reference's
 *     np.zeros((numDimensions, numParticles)) C-order layout
 *     (src/ensemble.py:40-41).  Element type is the potential handle's dtype.
 *   - `mass` is a device array of N elements or NULL (= all ones, the
 *     reference default src/ensemble.py:42; NULL also selects the division-free
 *     fast path, which is exact for unit mass).
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *     Calls are asynchronous with respect to the host.
 *   - Potential handles are immutable after creation; the library is
 *     re-entrant; one handle may be used from several streams.
 *   - There is NO CPU fallback: every entry point launches HIP kernels on the
 *     handle's device and fails with PBBI_ERR_HIP if that is impossible.
 *
 * RNG contract (device "philox" mode; pbbi_hmc_run, pbbi_philox_*)
 *   Philox-4x32-10, key = (seed_lo32, seed_hi32),
 *   counter = (chain_lo32, block, iteration_lo32, stream | chain_hi24 << 8),
 *   where `chain` is the GLOBAL chain index (chain0 + n), so results do not
 *   depend on how the ensemble is sharded over GPUs.
 *   Standard normals: one block serves the four dims d, d+4, d+8, d+12 of a group of 16
 *     (block = ((dim>>4)<<2) | (dim&3), slot = (dim>>2)&3) through two SINGLE-PRECISION
 *     Box-Muller transforms, (x0,x1) -> slots 0,1 and (x2,x3) -> slots 2,3:
 *       u1 = a*2^-32 + 2^-33 in (0,1],  u2 = (b>>8)*2^-24,  r = sqrtf(-2 ln u1),
 *       z_even = r*cos(2 pi u2),  z_odd = r*sin(2 pi u2),  widened to the array dtype.
 *     The device evaluates log2/sqrt/sin/cos on its transcendental unit; draws are
 *     reproducible bit for bit on the device (pbbi_philox_normal returns exactly what
 *     pbbi_hmc_run draws), exact N(0,1) on a 2^-24-relative grid with tails to 6.7 sigma.
 *   Flag PBBI_DRAW_F64 (stream bit PBBI_STREAM_DRAW_F64 of pbbi_philox_normal): DOUBLE-PRECISION Box-Muller,
 *     the counterpart of the reference's float64 draws (src/ensemble.py:72-74,88-91).  Two blocks per four
 *     dims: slots 0,1 from block blk, slots 2,3 from block blk | 0x80000000.  With w1 = x1:x0, w2 = x3:x2:
 *       u1 = ((w1 >> 12) + 0.5) * 2^-52 in (0,1);   k2 = w2 >> 11,  angle 2 pi k2 2^-53 = (pi/2)(n + y),
 *       n = (k2 + 2^50) >> 51,  y = (k2 - n 2^51) 2^-51 in [-1/2, 1/2)   (integer arithmetic, exact);
 *       r = sqrt(-2 ln u1), ln by fdlibm's e_log.c scheme (s = f/(2+f), Lg1..Lg7, Horner with fma);
 *       sin / cos((pi/2) y) by Taylor polynomials in y^2 (9 / 10 terms, fma), rotated by n & 3;
 *       z_even = r cos(angle),  z_odd = r sin(angle).
 *     Only +, -, *, /, sqrt, fma in a fixed order: the device's variates and the oracle's are THE SAME BITS
 *     (csrc/pbbi_rng.h, oracle/pbbi_oracle.c); exact N(0,1) on a 2^-52 grid with tails to 8.57 sigma.
 *   Metropolis uniform of a chain: block = 0xFFFFFFFF, stream = PBBI_STREAM_UNIFORM,
 *     u = ((x1:x0)>>11) * 2^-53 in [0,1).
 *   Predictive replicates (pbbi_predictive_glm; csrc/glm_sample_dev.h, restated in NumPy with SciPy's distribution
 *     functions by tests/glm_predictive_ref.py): stream = PBBI_STREAM_PREDICTIVE.  The block of (draw t, observation i,
 *     index b) is counter (chain = i, block = b, iteration = t), t = s * N + n the global draw index (S * N <= 2^32), so a
 *     replicate depends on (seed, t, i) alone.  The uniform of a block: u = ((x1:x0 >> 11) + 0.5) * 2^-53 in double arithmetic, never 0 (and 1 only for
 *     the one k = 2^53 - 1, where the sum rounds up: every sampler below is defined at u = 1); the
 *     normal of a block: the FIRST normal (z_even) of the double-precision Box-Muller above.  eta = x_i . w_t + o_i.
 *     Every sampler is exact; none is replaced by a normal approximation:
 *       gaussian     y = eta + exp(theta) / sqrt(a_i) * z,  z the normal of block 0.
 *       poisson, logistic (binomial n_i), negbinomial (mean mu = exp(eta), shape phi = exp(theta), p = phi / (phi + mu)):
 *                    inversion of the uniform of block 0 over the support enumerated from the mode outwards: m, m + 1, m - 1,
 *                    m + 2, m - 2, ..., points outside the support skipped; y = the first point at which the accumulated
 *                    mass reaches u (cum >= u).  m = floor(mu); min(n, floor((n + 1) p)); max(0, floor((phi - 1) mu / phi)).
 *                    The mass at m from glm_lgamma, its neighbours by the one-division ratio recurrences f(k + 1) / f(k) =
 *                    mu / (k + 1); (n - k) r / (k + 1), r = exp(eta); (k + phi) q / (k + 1), q = mu / (mu + phi), and their
 *                    inverses.  The walk ends when the terms on both sides are 0 and returns the last point visited that had
 *                    positive mass.  n_i = 1: y = 1 if u < p, else 0, without a walk.  O(sigma) steps per value: a
 *                    distribution whose VARIANCE is above 2^20 (mu; n p (1 - p); mu + mu^2 / phi) is NOT SERVED and gives
 *                    NaN, as does a walk longer than 2^20 rounds (only a shape phi -> 0 gets there); a rejection sampler for
 *                    large means would be a different stream number.
 *       ordinal      inversion of the uniform of block 0 over the K cumulative probabilities sigma(kappa_j - eta) in category
 *                    order: y = the first category whose cumulative probability is >= u.
 *       gamma        shape alpha = exp(theta), mean mu = exp(eta).  Marsaglia-Tsang: d = alpha - 1/3 (alpha + 2/3 when
 *                    alpha < 1), c = 1 / sqrt(9 d); attempt j = 0, 1, ... takes z = the normal of block 2j and u = the uniform
 *                    of block 2j + 1, v = (1 + c z)^3, and accepts if v > 0 and log u < z^2 / 2 + d - d v + d log v;
 *                    y = d v mu / alpha, times u'^(1 / alpha) with u' the uniform of block 0x80000000 when alpha < 1.  After
 *                    64 attempts the value is NaN.
 *     A non-finite eta or mean gives NaN.
 *   The integer part is bit-identical to oracle/pbbi_oracle.c; the single-precision
 *   transcendental part agrees with the host mirror to ~1e-6 absolute.
 */
#ifndef PBBI_H
#define PBBI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBBI_VERSION 103 /* major*100 + minor */

enum { PBBI_OK = 0, PBBI_ERR_INVALID = -1, PBBI_ERR_UNSUPPORTED = -2, PBBI_ERR_HIP = -3 };
enum { PBBI_F64 = 0, PBBI_F32 = 1 };
/* method: the two Integrator subclasses, src/integrator.py:94,126 */
enum { PBBI_LEAPFROG = 0, PBBI_STORMER_VERLET = 1 };
/* flags */
enum {
    /* reproduce src/HMC.py:176: a rejected chain's stored momentum is its OLD POSITION.
     * Without the flag the stored momentum of a rejected chain is the drawn momentum. */
    PBBI_COMPAT_P_FROM_OLDQ = 1,
    /* Opt-in throughput form: integrate in kick-drift-kick form with fused
     * multiply-adds (state q and the half-step velocity; 2 instead of 7 fp64 instructions per
     * element-step for the updates, no acceleration array).  Algebraically the reference's
     * velocity-Verlet (src/integrator.py:105-120); results agree to ~1e-13 relative instead of bit
     * for bit, accept masks as before.  Honoured by the two-lane Rosenbrock kernel (config C3) and
     * by the multi-lane / multi-wave harmonic, diagonal-Gaussian and Rosenbrock kernels (D <= 256); the MFMA kernels always
     * integrate this way, the other chain-per-lane kernels ignore it.  Stormer-Verlet under the flag
     * is the same recurrence without the closing half kick and with one more drift (honoured by the
     * separable kernel up to D = 256 and the in-wave Rosenbrock kernel up to D = 128). */
    PBBI_KDK_FMA = 2,
    /* Accept test at the temperature of the momentum draw: ratio = exp((oldH - newH) / kT) instead of
     * the reference's exp(oldH - newH) (src/HMC.py:115 has no beta although src/ensemble.py:88 draws p at
     * kB*T; the two agree only for T = 1/kB).  With the flag the chains sample exp(-U(q)/kT): the
     * canonical ensemble at that temperature.  kT is pbbi_hmc_run's argument; uploaded-draw iterations
     * state it through pbbi_hmc_iter_kt.  Without the flag (default) the reference's test is kept. */
    PBBI_BETA_ACCEPT = 4,
    /* Per-chain trajectory lengths (pbbi_hmc_iter_dyn / pbbi_hmc_run_dyn; SURVEY 8f row 2 -- planned in
     * the reference's WeekPlan.md:16-17, not a reference feature).  PBBI_PER_CHAIN_STEPS: chain n takes
     * its OWN number of leapfrog steps L_n in [1, L] -- steps_in[n] (uploaded draws) or
     * 1 + floor(u * L) with u from PBBI_STREAM_STEPS (in-kernel draws); lengths drawn independently of
     * the state keep the HMC kernel valid, and a fixed length's resonances go away chain by chain.
     * PBBI_UTURN_STOP: a chain stops after the first step j at which (q_j - q_0) . p_j < 0 (the
     * no-U-turn criterion), at most L (or L_n) steps; steps_out[n] records where.  Stopping at the
     * U-turn alone is NOT a reversible kernel: the flag is for measuring trajectory lengths during
     * warm-up (HMC.adaptTrajectoryLength), not for the recorded run.  Lanes of finished chains are
     * masked out; a wave leaves the loop when its last chain has. */
    PBBI_PER_CHAIN_STEPS = 8,
    PBBI_UTURN_STOP = 16,
    /* Momenta drawn in DOUBLE precision (pbbi_hmc_run / pbbi_hmc_run_dyn, every kernel family): the
     * counterpart of the reference's float64 normals (src/ensemble.py:72-74,88-91).  See "RNG contract":
     * bit-identical to oracle/pbbi_oracle.c, 52-bit radius / 53-bit angle, tails to 8.57 sigma.  Costs
     * ~2.5x the vector instructions of the default single-precision draw (the C2 headline: see DESIGN.md). */
    PBBI_DRAW_F64 = 32
};
enum { PBBI_STREAM_MOMENTUM = 0, PBBI_STREAM_POSITION = 1, PBBI_STREAM_UNIFORM = 2, PBBI_STREAM_STEPS = 3,
       PBBI_STREAM_SWAP = 4, /* replica-exchange uniforms (pbbi_replica_exchange) */
       PBBI_STREAM_RESAMPLE = 5, /* the stage uniform of systematic resampling (pbbi_smc_resample_systematic) */
       PBBI_STREAM_PREDICTIVE = 6, /* posterior predictive replicates (pbbi_predictive_glm; "Predictive replicates" above) */
       /* OR-ed into pbbi_philox_normal's rng_stream: the draw PBBI_DRAW_F64 selects in pbbi_hmc_run */
       PBBI_STREAM_DRAW_F64 = 0x100 };

typedef struct pbbi_potential pbbi_potential; /* opaque */

typedef struct {
    char name[128];
    char arch[64];
    int compute_units;
    int64_t hbm_bytes;
    int lds_bytes_per_block;
    int clock_khz;
} pbbi_devinfo;

/* ---- library ------------------------------------------------------------- */
int pbbi_version(void);
const char* pbbi_last_error(void);
int pbbi_device_count(int* count_out);
int pbbi_device_info(int device, pbbi_devinfo* out);

/* ---- potentials ----------------------------------------------------------
 * "potential" in the reference is any callable q(D,) -> scalar with a gradient
 * callable (D,) -> (D,) (src/integrator.py:73, src/HMC.py:102).  A GPU kernel
 * cannot call Python, so the closed forms the reference exercises are handles.
 * All parameter arrays are HOST pointers (float64), copied at creation.
 *   harmonic   U = 0.5*dot(k, q**2)                     src/potential.py:18-27
 *   gauss_diag U = 0.5*dot(prec*(q-mu), q-mu) + cst
 *   gauss_dense U = 0.5*dot(x, P x) + cst, x = q-mu, grad = P x with P symmetric
 *              (= -multivariate_normal.logpdf, src/tests/test_HMC.py:49,125).
 *              `precision` is D x D row-major and MUST be symmetric.
 *              (fp64 HMC iterations: D <= 128 on the register-resident MFMA kernel with P in LDS, 128 < D <= 256 on
 *              the same kernel with P streamed through LDS, beyond -- and fp32 -- one fused GEMM per leapfrog step.)
 *   rosenbrock U = sum_{i<D-1} [b (q_{i+1}-q_i^2)^2 + (a-q_i)^2] / s
 *              (defined by this build).
 * mean may be NULL (= 0).
 */
int pbbi_potential_create_harmonic(int D, const double* springConsts, int dtype, int device,
                                   pbbi_potential** out);
int pbbi_potential_create_gauss_diag(int D, const double* mean, const double* prec, double cst,
                                     int dtype, int device, pbbi_potential** out);
int pbbi_potential_create_gauss_dense(int D, const double* mean, const double* precision,
                                      double cst, int dtype, int device, pbbi_potential** out);
int pbbi_potential_create_rosenbrock(int D, double a, double b, double s, int dtype, int device,
                                     pbbi_potential** out);
/* User-defined potential -- the counterpart of the reference's arbitrary Python callables
 * (`potential=` / `gradient=` of src/HMC.py:35-60, src/integrator.py:36-59).  The two functions
 * are stated in C++ (contract in physicsbasedbayesianinference_amd/custom.py and
 * csrc/pbbi_custom.h), compiled by hipcc for gfx950 into a plugin shared object whose kernels
 * have them inlined; `plugin_path` names that file.  `params` (host, float64, may be NULL when
 * n_params == 0) is copied to the device in the handle's dtype and passed to both functions:
 * model constants, or the data set of a Bayesian model. */
int pbbi_potential_create_custom(const char* plugin_path, int D, const double* params, int n_params,
                                 int dtype, int device, pbbi_potential** out);
/* Generalised linear model with a Gaussian prior -- the likelihood as two matrix products shared by all chains,
 * on the fp64 matrix cores (csrc/kernels_glm.hip):
 *     U(w) = sum_i [ b(x_i . w) - y_i (x_i . w) ] + 0.5 prior_precision |w|^2   over the M rows x_i of X,
 *     logistic: b = softplus (y in {0, 1});   poisson: b = exp (y = counts, log link).
 * X (M x D row-major) and y (M) are HOST pointers, copied at creation (X into MFMA fragment order).  fp64 and
 * 1 <= D <= 128 only (otherwise PBBI_ERR_UNSUPPORTED); M >= 1; prior_precision >= 0.  The handle serves the
 * evaluations, the integrators, pbbi_hmc_iter / _iter_kt and pbbi_hmc_run (Leapfrog and Stormer-Verlet, always in
 * kick-drift-kick form); per-chain trajectory lengths and GIST return PBBI_ERR_UNSUPPORTED. */
enum { PBBI_GLM_LOGISTIC = 0, PBBI_GLM_POISSON = 1 };
int pbbi_potential_create_glm(int D, int64_t M, const double* X, const double* y, int family,
                              double prior_precision, int dtype, int device, pbbi_potential** out);
/* The fragment image pbbi_potential_create_glm uploads, on the HOST (touches no device): *len_out <- its length in
 * doubles; with `out` non-NULL (out_len >= that length) the image itself.  Per block of 16 observations b, with
 * DP = D padded to 16 / 32 / 64 / 128, KS = DP/4, NT = DP/16, lane = 0..63, e = 0, 1:
 *     P1[s2][lane][e]    = X[16b + (lane & 15)][4 (2 s2 + e) + (lane >> 4)]            s2 < KS/2
 *     P2[r2][t][lane][e] = X[16b + 4 (2 r2 + e) + (lane >> 4)][16 t + (lane & 15)]     r2 < 2, t < NT
 * (P1 then P2, 32 DP doubles per block), zero padded; the block count is padded to a multiple of 4. */
int pbbi_glm_pack_design(int D, int64_t M, const double* X, double* out, int64_t out_len, int64_t* len_out);
/* The full model: observation weights a_i, offsets o_i, binomial trials n_i and a prior per coefficient,
 *     U(w) = sum_i a_i [ n_i b(eta_i) - y_i eta_i ] + 0.5 sum_d lam_d (w_d - mu_d)^2,    eta_i = x_i . w + o_i,
 *     grad U = X^T r + lam (.) (w - mu),    r_i = a_i [ n_i b'(eta_i) - y_i ].
 * weights / offset / trials: host pointers to M doubles, NULL = all 1 / all 0 / all 1; weights finite and >= 0 (a
 * row of weight 0 contributes exactly 0 to U and the gradient, even where b(eta_i) overflows), offset finite (for
 * Poisson rates typically log(exposure)), trials integers >= 1 and logistic only (y_i = successes, integers in
 * [0, n_i]; Poisson y = counts).  prior_precision: D doubles, each finite and >= 0 (0 = a flat coordinate), required;
 * prior_mean: D doubles or NULL = 0.  Violations return PBBI_ERR_INVALID with a message before anything is
 * allocated.  The handle runs the same kernels and serves the same calls as one of pbbi_potential_create_glm (whose
 * model is the case weights = trials = 1, offset = 0, lam_d = prior_precision, mu = 0, on kernels of its own whose
 * arithmetic this entry does not touch); the device keeps c_i = a_i n_i, d_i = a_i y_i and o_i. */
int pbbi_potential_create_glm_ex(int D, int64_t M, const double* X, const double* y, int family,
                                 const double* weights, const double* offset, const double* trials,
                                 const double* prior_precision, const double* prior_mean, int dtype, int device,
                                 pbbi_potential** out);
/* The three observation streams pbbi_potential_create_glm_ex uploads, on the HOST (touches no device, checks the
 * same rules): *len_out <- their total length in doubles, 3 * 16 * (blocks of 16 observations padded to a multiple of
 * 4); with `out` non-NULL (out_len >= that length) c | d | o, each stream zero padded past M. */
int pbbi_glm_pack_observations(int64_t M, int family, const double* y, const double* weights, const double* offset,
                               const double* trials, double* out, int64_t out_len, int64_t* len_out);
/* K-class (multinomial logistic / softmax) regression, every class with coefficients and a Gaussian prior shared by
 * the classes (csrc/kernels_glm_softmax.hip):
 *     U(W) = sum_i [ logsumexp_k(eta_ik) - eta_{i,y_i} ] + 0.5 sum_k sum_d lam_d W_kd^2,    eta_ik = x_i . W_k.
 * The handle's dimension is K*D: one chain is the K coefficient vectors class-major, w[k*D + d].  X (M x D row-major),
 * y (M labels as doubles, integers in [0, K)) and prior_precision (D values, finite and >= 0) are HOST pointers,
 * checked (PBBI_ERR_INVALID) and copied at creation.  fp64 only; each class is padded to Dc = 16, 32 or 64 rows and
 * 2 <= K <= 8, K * Dc <= 128 (D <= 16 for K <= 8, D <= 32 for K <= 4, D <= 64 for K = 2), otherwise
 * PBBI_ERR_UNSUPPORTED.  The handle is a GLM handle of family PBBI_GLM_SOFTMAX: it serves what those serve and
 * refuses what they refuse (per-chain trajectory lengths, GIST).  pbbi_potential_create_glm / _glm_ex do not accept
 * this family. */
enum { PBBI_GLM_SOFTMAX = 2 };
int pbbi_potential_create_glm_softmax(int D, int K, int64_t M, const double* X, const double* y,
                                      const double* prior_precision /* D values */, int dtype, int device,
                                      pbbi_potential** out);
/* host only, no GPU: the padded class size, the tile count and (row_map != NULL) the external row of each of the
   NT*16 internal rows, -1 for padding */
int pbbi_glm_softmax_layout(int D, int K, int* Dc_out, int* NT_out, int32_t* row_map);
/* The three families with a free dispersion, on the full model's kernel frame (csrc/kernels_glm.hip, FAM = 3, 4, 5 of
 * k_glm<NT, FAM, true>).  theta is the LOG-dispersion, a_i >= 0 observation weights, o_i offsets, eta_i = x_i . w + o_i;
 * constants that depend on neither w nor theta are dropped:
 *     gaussian     sigma = exp(theta), tau = exp(-2 theta), y real:
 *                  U_i = a_i [ 0.5 tau (y_i - eta_i)^2 + theta ]
 *     negbinomial  NB2, log link: mu_i = exp(eta_i), phi = exp(theta), Var = mu + mu^2 / phi, y non-negative integers:
 *                  U_i = a_i [ lgamma(phi) - lgamma(y_i + phi) - phi theta - y_i eta_i + (y_i + phi) logaddexp(eta_i, theta) ]
 *     gamma        log link: mu_i = exp(eta_i), shape alpha = exp(theta), Var = mu^2 / alpha, y > 0; with z_i = eta_i - log y_i
 *                  U_i = a_i [ lgamma(alpha) - alpha theta + alpha (z_i + exp(-z_i)) ]      (the dropped constant: + a_i log y_i)
 *                  alpha held at 1 is exponential regression
 *     U = sum_i U_i + 0.5 sum_d lam_d (w_d - mu_d)^2  [ + 0.5 lam_theta (theta - m_theta)^2  when theta is sampled ]
 * sample != 0: theta is the LAST component of the chain's state, the handle's dimension is D + 1 and lam / mu hold D + 1
 * entries (the last: precision and mean of theta's Gaussian prior; mu may be NULL = 0); `theta` is ignored.
 * sample == 0: the dispersion is held at exp(theta) (theta finite), the state is w alone (dimension D), lam / mu hold D
 * entries.  The design image on the device is that of [X | 0] at the padded state dimension: the theta row meets a
 * zero column, so eta does not see it; its gradient, sum_i dU_i / dtheta, is reduced per chain in the kernel.  The
 * device keeps c_i = a_i, d_i = y_i (raw, not a_i y_i; gamma: d_i = log y_i, taken once on the host -- the kernel needs
 * nothing else of y) and o_i; a row of weight 0 contributes exactly 0.  weights /
 * offset: M doubles or NULL = all 1 / all 0.  fp64 only; the state dimension (D + 1 when sampled) is at most 128 for
 * gaussian and gamma and at most 64 for negbinomial, whose kernel for 65 .. 128 rows cannot be built without register
 * spills to memory and is not shipped (PBBI_ERR_UNSUPPORTED).  Violations of the value rules return PBBI_ERR_INVALID before
 * anything is allocated.  The handle is a GLM handle (same calls served and refused); pbbi_describe_run names the
 * family.  pbbi_potential_create_glm / _glm_ex do not accept these families. */
enum { PBBI_GLM_GAUSSIAN = 3, PBBI_GLM_NEGBINOMIAL = 4, PBBI_GLM_GAMMA = 5 };
int pbbi_potential_create_glm_dispersion(int D, int64_t M, const double* X, const double* y, int family,
                                         const double* weights, const double* offset, const double* lam,
                                         const double* mu, int sample, double theta, int dtype, int device,
                                         pbbi_potential** out);
/* The three observation streams pbbi_potential_create_glm_dispersion uploads, on the HOST (touches no device, checks the
 * same rules): *len_out <- their total length, as for pbbi_glm_pack_observations; with `out` non-NULL c = a | d = y | o
 * (gamma: d = log y), each stream zero padded past M. */
int pbbi_glm_pack_observations_dispersion(int64_t M, int family, const double* y, const double* weights,
                                          const double* offset, double* out, int64_t out_len, int64_t* len_out);
/* Ordinal (cumulative-logit, proportional-odds) regression with sampled cutpoints, on the full model's kernel frame
 * (csrc/kernels_glm.hip, FAM = 6 of k_glm<NT, FAM, true>).  Categories y_i in {0 .. K-1}, 2 <= K <= 8, cutpoints kappa_1 < .. <
 * kappa_{K-1} with kappa_0 = -inf and kappa_K = +inf, observation weights a_i >= 0, offsets o_i, eta_i = x_i . w + o_i:
 *     P(y_i = k) = sigma(kappa_{k+1} - eta_i) - sigma(kappa_k - eta_i)
 * X carries NO intercept column: the cutpoints are the intercepts (a column of ones is not identified against them; X is not
 * tested for one).  The chain's state is [w (D rows); zeta (K - 1 rows)], the cutpoint rows LAST and unconstrained:
 *     zeta_1 = kappa_1,  zeta_j = log(kappa_j - kappa_{j-1}) (j >= 2),  so  kappa_j = zeta_1 + sum_{m = 2 .. j} exp(zeta_m)
 * and the ordering holds by construction.  The priors are Gaussian on these rows -- lam / mu hold D + K - 1 entries, the last
 * K - 1 the precision and mean of zeta_1 and of the log-gaps (mu may be NULL = 0) -- and stated on zeta, so there is no Jacobian
 * term.  With sp = softplus and Delta_k = kappa_{k+1} - kappa_k = exp(zeta_{k+1}), an observation of category k has
 *     U_i = a_i [ sp(eta_i - kappa_{k+1}) + sp(kappa_k - eta_i) - log(1 - exp(-Delta_k)) ]
 * (sigma(b) - sigma(a) = sigma(b) sigma(-a) (1 - exp(-(b - a))): no logarithm of a difference of two sigmoids), the terms of an
 * infinite cutpoint absent: k = 0 keeps the first softplus, k = K - 1 the second, neither has the last term.
 *     U = sum_i U_i + 0.5 sum_d lam_d (s_d - mu_d)^2  over the D + K - 1 rows s of the state.
 * K = 2 is logistic regression with intercept -kappa_1.  The handle's dimension is D + K - 1.  The design image on the device
 * is that of [X | 0] at the padded state dimension; the device keeps c_i = a_i, d_i = y_i (the category) and o_i, and the
 * weighted category counts A_k = sum_{i: y_i = k} a_i behind the prior table; a row of weight 0 contributes exactly 0, a
 * category without observations is allowed.  Checked before anything is allocated, with the observation's index in the message
 * (PBBI_ERR_INVALID): y integers in [0, K), weights finite and >= 0, offsets finite, lam finite and >= 0, 2 <= K <= 8.  fp64
 * only; the state dimension D + K - 1 is at most 64: the kernel for 65 .. 128 rows cannot be built without register spills to
 * memory and is not shipped (PBBI_ERR_UNSUPPORTED).  The handle is a GLM handle: per-
 * chain lengths and GIST are refused; pbbi_potential_set_metric_diag, pbbi_pointwise_glm (whose fitted mean is the expected
 * category sum_j sigma(eta - kappa_j)), pbbi_loglik_glm and pbbi_potential_set_likelihood_power are served;
 * pbbi_describe_run names the family.  Random effects on this family are not built: the hierarchical entries answer
 * PBBI_ERR_UNSUPPORTED for family 6. */
enum { PBBI_GLM_ORDINAL = 6 };
/* pbbi_potential_create_glm_ordinal(D, K, M, X, y, weights, offset, lam, mu, dtype, device, out) and its host-only packer
 * pbbi_glm_pack_observations_ordinal are declared in pbbi_glm_ordinal.h (included at the end). */
/* Hierarchical priors with sampled group scales (random effects, a learned ridge penalty) on the full model's kernel frame
 * (csrc/kernels_glm.hip, k_glm<NT, FAM, true, GLM_HIER_CENTRED>); families logistic and poisson, weights a_i, trials n_i, offsets o_i
 * and eta_i = x_i . w + o_i as for pbbi_potential_create_glm_ex.  groups[d] is -1 (coefficient d keeps the fixed prior
 * {prior[d], prior_mean[d]}) or a group index j in 0 .. J-1; the members of group j share the unknown scale sigma_j =
 * exp(t_j), w_d | t_j ~ N(mu_d, sigma_j^2), t_j ~ N(m_tj, 1 / lam_tj) (the centred parametrisation, sampled on the log scale):
 *     U(w, t) = sum_i a_i [ n_i b(eta_i) - y_i eta_i ]
 *             + 0.5 sum_{d: groups_d < 0} lam_d (w_d - mu_d)^2
 *             + sum_j [ 0.5 exp(-2 t_j) S_j + n_j t_j + 0.5 lam_tj (t_j - m_tj)^2 ]
 *     S_j = sum_{d: groups_d = j} (w_d - mu_d)^2,   n_j = #{d: groups_d = j}
 *     dU/dw_d = (likelihood) + exp(-2 t_j) (w_d - mu_d)   for groups_d = j
 *     dU/dt_j = n_j - exp(-2 t_j) S_j + lam_tj (t_j - m_tj)
 * State: rows 0 .. D-1 the coefficients, rows D .. D+J-1 t_0 .. t_{J-1}; the handle's dimension is D + J.  The design image
 * on the device is that of [X | 0] at the padded dimension of D + J, so eta does not see the t rows.  prior: D doubles (the
 * entries of grouped coefficients are ignored), prior_mean: D doubles or NULL = 0, log_scale_prior: J pairs (m_tj, lam_tj),
 * lam_tj >= 0.  1 <= J <= 4 (else PBBI_ERR_UNSUPPORTED) and every index 0 .. J-1 must be used; fp64 only; D + J <= 64 for
 * both families: their kernels for 65 .. 128 rows cannot be built without register spills to memory and are not shipped
 * (PBBI_ERR_UNSUPPORTED).  Violations of the value rules return PBBI_ERR_INVALID before anything is
 * allocated.  The handle is a GLM handle (same calls served and refused: no per-chain trajectory lengths, no GIST). */
int pbbi_potential_create_glm_hier(int D, int64_t M, const double* X, const double* y, int family, const double* weights,
                                   const double* offset, const double* trials, const double* prior,
                                   const double* prior_mean, const int32_t* groups, int J, const double* log_scale_prior,
                                   int dtype, int device, pbbi_potential** out);
/* ... with a choice of parametrisation.  PBBI_HIER_CENTRED is pbbi_potential_create_glm_hier exactly (same kernel, same
 * bits).  PBBI_HIER_NONCENTRED (k_glm<NT, FAM, true, GLM_HIER_NC>) samples z_d in place of w_d on the grouped rows:
 *     rows 0 .. D-1: groups_d < 0 holds w_d as above; groups_d = j holds z_d, w_d = mu_d + exp(t_j) z_d, z_d ~ N(0, 1)
 *     rows D .. D+J-1: t_j as above
 *     U(z, t)  = L(w(z, t)) + 0.5 sum_{fixed} lam_d (w_d - mu_d)^2 + 0.5 sum_{grouped} z_d^2 + sum_j 0.5 lam_tj (t_j - m_tj)^2
 *     dU/dz_d  = exp(t_j) gL_d + z_d,   gL = X^T r at w(z, t)       (grouped rows)
 *     dU/dw_d  = gL_d + lam_d (w_d - mu_d)                          (fixed rows)
 *     dU/dt_j  = exp(t_j) sum_{d in j} gL_d z_d + lam_tj (t_j - m_tj)
 * with L the likelihood sum above.  It is the same posterior in other coordinates: U_nc(z, t) = U_c(w(z, t), t) - sum_j n_j
 * t_j, the n_j t_j being the Jacobian of (w, t) -> (z, t).  Choose it when a level has few observations (the centred
 * posterior is then a funnel in (w, t) whose neck no single step size serves); with many observations per level the
 * centred form mixes better.  States, samples and running statistics of such a handle are in sampler coordinates (z on
 * the grouped rows).  The scaling runs inside the kernel on a copy of the state; the table of pbbi_glm_pack_prior_groups
 * is the same.  All rules above apply; D + J <= 64 for both families; any other `parametrisation` is PBBI_ERR_INVALID. */
#define PBBI_HIER_CENTRED 0
#define PBBI_HIER_NONCENTRED 1
int pbbi_potential_create_glm_hier_ex(int D, int64_t M, const double* X, const double* y, int family, const double* weights,
                                      const double* offset, const double* trials, const double* prior,
                                      const double* prior_mean, const int32_t* groups, int J, const double* log_scale_prior,
                                      int parametrisation, int dtype, int device, pbbi_potential** out);
/* The prior table pbbi_potential_create_glm_hier uploads and the kernel keeps in LDS, on the HOST (touches no device, checks
 * the same rules): out <- lam (DP) | mu (DP) with DP = D + J padded to 16, 32, 64 or 128 -- a fixed row {lam_d, mu_d}, a
 * member of group j {-(j + 1), mu_d} (a negative lam slot names the group whose exp(-2 t_j) is the row's precision), row
 * D + j {lam_tj, m_tj}, zeros past D + J; n_out <- n_0 .. n_{J-1}. */
int pbbi_glm_pack_prior_groups(int D, int J, const double* prior, const double* prior_mean, const int32_t* groups,
                               const double* log_scale_prior, double* out, double* n_out);
/* Random effects for the dispersion families: the likelihood of pbbi_potential_create_glm_dispersion (gaussian, negbinomial;
 * theta the LOG-dispersion, weights a_i >= 0, offsets o_i, eta_i = x_i . w + o_i) under the priors of
 * pbbi_potential_create_glm_hier_ex (csrc/kernels_glm.hip, k_glm<NT, FAM, true, GLM_HIER_CENTRED / GLM_HIER_NC> with FAM = 3, 4)
 * -- the linear mixed model with unknown residual sigma, its held-sigma form with weights 1 / sigma_i^2 (eight schools),
 * NB2 counts with a random intercept per site:
 *     gaussian     U_i = a_i [ 0.5 exp(-2 theta) (y_i - eta_i)^2 + theta ]
 *     negbinomial  U_i = a_i [ lgamma(phi) - lgamma(y_i + phi) - phi theta - y_i eta_i + (y_i + phi) logaddexp(eta_i, theta) ],
 *                  phi = exp(theta)
 *     centred:     U = sum_i U_i + 0.5 sum_{d: groups_d < 0} lam_d (w_d - mu_d)^2
 *                    + sum_j [ 0.5 exp(-2 t_j) S_j + n_j t_j + 0.5 lam_tj (t_j - m_tj)^2 ]
 *                    + 0.5 lam_theta (theta - m_theta)^2                        (the last term only when theta is sampled)
 *     noncentred:  grouped rows hold z_d, w_d = mu_d + exp(t_j) z_d;  U_nc(z, t, theta) = U_c(w(z, t), t, theta) - sum_j n_j t_j
 * State: rows 0 .. D-1 the coefficients (z_d on grouped rows when non-centred), rows D .. D+J-1 t_0 .. t_{J-1}, and with
 * sample != 0 row D+J theta, the LAST row; the handle's dimension is D + J + (sample ? 1 : 0).  sample == 0: the dispersion
 * is held at exp(theta) (theta finite) and the state is [w; t].  The design image on the device is that of [X | 0] at the
 * padded state dimension, so eta sees neither the t rows nor the theta row.
 * Arguments: X, y, family, weights, offset with the rules of pbbi_potential_create_glm_dispersion (y finite; negbinomial: non-
 * negative integers; weights finite >= 0 or NULL; offset finite or NULL; X finite); prior (D doubles, the entries of grouped
 * coefficients ignored), prior_mean (D doubles or NULL = 0), groups (D entries, -1 or 0 .. J-1, every index used), J (1 .. 4,
 * else PBBI_ERR_UNSUPPORTED), log_scale_prior (J pairs (m_tj, lam_tj >= 0)) and parametrisation with the rules of
 * pbbi_potential_create_glm_hier_ex; log_dispersion_prior: the pair (m_theta, lam_theta >= 0) when sample != 0 (`theta` is then
 * ignored), NULL when sample == 0 (a held dispersion has no prior: non-NULL is PBBI_ERR_INVALID).  Families logistic and
 * poisson are PBBI_ERR_INVALID here (they are pbbi_potential_create_glm_hier / _hier_ex).  Violations of the value rules return
 * PBBI_ERR_INVALID before anything is allocated; fp32, or D + J + (sample ? 1 : 0) above
 * pbbi_glm_hier_dispersion_max_dim(family, parametrisation), PBBI_ERR_UNSUPPORTED.  A kernel is shipped only if it builds
 * without register spills to memory; all twelve of 16, 32 and 64 rows do, and there is none at 128 rows (64 for both
 * families and both parametrisations).  The handle is a GLM handle (same calls served and refused: no per-chain trajectory
 * lengths, no GIST); pbbi_describe_run names the family, the dispersion row or held value, the groups and the parametrisation.
 * Not served: structured group priors (a penalty matrix) for these families. */
int pbbi_potential_create_glm_hier_dispersion(int D, int64_t M, const double* X, const double* y, int family,
                                              const double* weights, const double* offset, const double* prior,
                                              const double* prior_mean, const int32_t* groups, int J,
                                              const double* log_scale_prior, int parametrisation, int sample, double theta,
                                              const double* log_dispersion_prior, int dtype, int device, pbbi_potential** out);
/* The prior table pbbi_potential_create_glm_hier_dispersion uploads and its kernel keeps in LDS, on the HOST (touches no
 * device, checks the same rules): out <- lam (DP) | mu (DP) with DP = D + J + (sample ? 1 : 0) padded to 16, 32, 64 or 128 --
 * rows 0 .. D+J-1 as pbbi_glm_pack_prior_groups writes them, row D + J {lam_theta, m_theta} when sample != 0 (a fixed row: its
 * lam slot is >= 0), zeros past the state; n_out <- n_0 .. n_{J-1}. */
int pbbi_glm_pack_prior_groups_dispersion(int D, int J, const double* prior, const double* prior_mean, const int32_t* groups,
                                          const double* log_scale_prior, int sample, const double* log_dispersion_prior,
                                          double* out, double* n_out);
/* The largest state dimension D + J + (sample ? 1 : 0) pbbi_potential_create_glm_hier_dispersion serves for a family
 * (PBBI_GLM_GAUSSIAN, PBBI_GLM_NEGBINOMIAL) and parametrisation; 0 for any other argument.  Returns the number, not a status. */
int pbbi_glm_hier_dispersion_max_dim(int family, int parametrisation);
/* Structured group priors: the centred model of pbbi_potential_create_glm_hier with a symmetric positive semi-definite
 * matrix in each group's quadratic form (k_glm<NT, FAM, true, GLM_HIER_Q>) -- random walks (RW1 / RW2), difference penalties
 * of splines, ICAR / CAR effects, any correlated effect given by a precision matrix, the smoothing parameter sampled.  With
 * d_j = (w_d - mu_d) over the members of group j in increasing column order,
 *     w_j - mu_j | t_j ~ N(0, exp(2 t_j) Q_j^-)                (Q_j possibly rank deficient, r_j = rank(Q_j))
 *     U(w, t) = sum_i a_i [ n_i b(eta_i) - y_i eta_i ]
 *             + 0.5 sum_{d: groups_d < 0} lam_d (w_d - mu_d)^2
 *             + sum_j [ 0.5 exp(-2 t_j) d_j^T Q_j d_j + r_j t_j + 0.5 lam_tj (t_j - m_tj)^2 ]
 *     dU/dw (members of j) = (likelihood) + exp(-2 t_j) Q_j d_j
 *     dU/dt_j              = r_j - exp(-2 t_j) d_j^T Q_j d_j + lam_tj (t_j - m_tj)
 * Q_j = I, r_j = n_j is the model of pbbi_potential_create_glm_hier.  All arguments up to log_scale_prior are that
 * function's, with its rules.  penalty: a (D x D) row-major matrix in COEFFICIENT indexing -- Q_j on the rows and columns
 * of the members of group j, the identity on the members of an exchangeable group, zero on fixed rows and between
 * different groups; entries finite, each block symmetric (max|Q - Q^T| <= 1e-12 max|Q|; (Q + Q^T) / 2 is used), positive
 * semi-definite (smallest eigenvalue >= -1e-10 x the largest) and not zero.  rank: J values, rank[j] an integer in 1 ..
 * n_j.  Violations return PBBI_ERR_INVALID before anything is allocated; D + J > 64 or fp32 PBBI_ERR_UNSUPPORTED.  The
 * device keeps the (DP x DP) image of pbbi_glm_pack_penalty, resident in LDS for the whole launch (8 DP^2 bytes), and the
 * ranks in the n_j slots of the prior table; Q (w - mu) is one more fp64 MFMA product per gradient evaluation.  The handle
 * is a GLM handle (same calls served and refused); pbbi_describe_run names the kernel.  Not served: the non-centred
 * parametrisation, structure across groups, sampled structure (a CAR rho), D + J > 64. */
int pbbi_potential_create_glm_hier_q(int D, int64_t M, const double* X, const double* y, int family, const double* weights,
                                     const double* offset, const double* trials, const double* prior,
                                     const double* prior_mean, const int32_t* groups, int J, const double* log_scale_prior,
                                     const double* penalty, const double* rank, int dtype, int device, pbbi_potential** out);
/* The image of the penalty pbbi_potential_create_glm_hier_q uploads, on the HOST (touches no device; checks only D >= 1,
 * 1 <= J <= 4, D + J <= 128): *len_out <- its length DP * DP in doubles, DP = D + J padded to 16 / 32 / 64 / 128; with
 * `out` non-NULL (out_len >= that length) the image: one block per 16 rows of Q, each in the order of P1 of
 * pbbi_glm_pack_design with the rows of Q in the role of observations,
 *     out[((t * DP/8 + s2) * 64 + lane) * 2 + e] = Q[16 t + (lane & 15)][4 (2 s2 + e) + (lane >> 4)]     t < DP/16, s2 < DP/8
 * with (Q + Q^T) / 2 for Q; rows and columns >= D are zero. */
int pbbi_glm_pack_penalty(int D, int J, const double* penalty, double* out, int64_t out_len, int64_t* len_out);
/* What a GLM handle says about T = S * N draws of its state, per observation, reduced over the draws on the device
 * (csrc/kernels_glm_pointwise.hip: eta = X W for 16 draws at a time on the fp64 matrix cores, from the first copy of the
 * packed design image).  ll_it = minus the per-observation term of the handle's potential at draw t -- the log-likelihood of
 * observation i WITHOUT the terms that depend on no parameter (a log C(n, y); -a lgamma(y + 1); -a/2 log 2 pi; gamma: -a log y), which the
 * caller adds -- and exactly 0 for an observation of weight 0.  Outputs, each (M) doubles on the device or NULL:
 *     lse_out[i]  = log sum_t exp(ll_it)          (lppd_i = lse_i - log T + the constant of observation i)
 *     mean_out[i] = mean_t ll_it
 *     var_out[i]  = the unbiased variance over t of ll_it (the WAIC penalty of observation i); needs S * N >= 2
 *     mu_out[i]   = mean_t of the fitted mean: sigmoid(eta_it) (logistic, per trial), exp(eta_it) (poisson, negbinomial, gamma),
 *                   eta_it (gaussian), eta_it = x_i . w_t + o_i -- for every observation, whatever its weight
 * samples_sdn: S contiguous (Dt, N) slabs of doubles (the pbbi_sample_moments convention) on the handle's device, Dt >= the
 * handle's state dimension; rows past it are ignored.  The draws are on the NATURAL scale: for a non-centred handle (w; t),
 * not (z; t).  Only the coefficient rows are read as coefficients: the log-scales of a hierarchical handle do not enter, a
 * sampled log-dispersion is read from its own row, a held one comes from the handle.  ranges: 0 = the library chooses how
 * many ranges the draws are cut into, >= 1 (<= 65535) fixes it; the ranges are merged in index order without atomics, so for
 * a given `ranges` the results are bit for bit the same from run to run.  A draw with ll_it = -inf leaves lse_i to the other
 * draws and makes mean_i and var_i non-finite; a NaN draw makes every output of the observations it reaches NaN.
 * Served: the handles of pbbi_potential_create_glm, _glm_ex, _glm_dispersion, _glm_hier, _glm_hier_ex, _glm_hier_q and
 * _glm_hier_dispersion.  A softmax handle and a handle that is no GLM handle: PBBI_ERR_UNSUPPORTED.  NULL handle or samples,
 * S < 1, N < 1, Dt below the state dimension, var_out with S * N < 2, ranges outside 0 .. 65535: PBBI_ERR_INVALID.  Every
 * rule is checked before the device is touched. */
int pbbi_pointwise_glm(const pbbi_potential* pot, const void* samples_sdn, int S, int Dt, int64_t N, int ranges,
                       double* lse_out, double* mean_out, double* var_out, double* mu_out, void* stream);
/* The argument rules of pbbi_pointwise_glm alone, on the HOST (touches no device), for a handle described by value: handle = 0
 * (NULL), 1 (a GLM handle of `family` with state dimension `state_dim`) or 2 (a handle of another kind); `samples` is only
 * compared with NULL; want_var != 0: var_out is asked for.  Returns what pbbi_pointwise_glm would return before it launches. */
int pbbi_pointwise_glm_check(int handle, int family, int state_dim, const void* samples, int S, int Dt, int64_t N,
                             int ranges, int want_var);
/* The likelihood energy of each of S * N draws of a GLM handle's state (csrc/kernels_glm_loglik.hip: a wave keeps 16 draws in
 * registers and walks the observation blocks, eta = X W on the fp64 matrix cores from the first copy of the packed design image):
 *     ulik_out[s * N + n] = sum_i U_i(draw n of slab s)            (S * N doubles on the device)
 * the likelihood part of the handle's potential -- minus the log-likelihood WITHOUT the terms that depend on no parameter (see
 * pbbi_pointwise_glm), which the caller adds -- with no prior term, no group-scale term and no prior of theta.  An observation of
 * weight 0 adds exactly 0, whatever its linear predictor is.  samples_sdn, Dt and the rows that are read: as for
 * pbbi_pointwise_glm (natural scale; only the coefficient rows are read as coefficients, the other rows change no bit; a sampled
 * log-dispersion is read from its own row, a held one comes from the handle).  The likelihood is ALWAYS at power 1: on a handle
 * tempered by pbbi_potential_set_likelihood_power the streams as built are read.  ranges: the observation blocks are cut into
 * `ranges` (0 = the library chooses, else 1 .. 65535; more ranges than blocks leave empty ones) so that few draws still fill the
 * device; a second kernel adds the partials in index order, without atomics: for a given `ranges` the result is bit for bit the
 * same from run to run.  A draw with log-likelihood -inf gives +inf, a NaN draw NaN, for that draw only.
 * Served: the handles pbbi_pointwise_glm serves, in the shapes the handles themselves are shipped in (no kernel reserves scratch
 * memory).  Rules, in this order, all before the device is touched: NULL handle, NULL samples, NULL ulik_out, S < 1, N < 1,
 * ranges outside 0 .. 65535: PBBI_ERR_INVALID; a handle that is no GLM handle, a softmax handle, an unknown family:
 * PBBI_ERR_UNSUPPORTED; Dt below the state dimension: PBBI_ERR_INVALID. */
int pbbi_loglik_glm(const pbbi_potential* pot, const void* samples_sdn, int S, int Dt, int64_t N, int ranges,
                    double* ulik_out, void* stream);
/* Those rules alone, on the HOST, for a handle described by value (as pbbi_pointwise_glm_check); the pointers are only compared
 * with NULL. */
int pbbi_loglik_glm_check(int handle, int family, int state_dim, const void* samples, const void* ulik_out, int S, int Dt,
                          int64_t N, int ranges);
/* Posterior predictive replicates of a GLM handle, drawn on the device (csrc/kernels_glm_predictive.hip: pbbi_loglik_glm's
 * frame -- a wave keeps 16 draws in registers and walks the observation blocks, eta on the fp64 matrix cores -- with the
 * family samplers of the RNG contract's section "Predictive replicates" in the lane).  For each of the S * N draws t = s * N + n
 * and each observation i one replicate y_rep ~ p(y | draw t), reduced per draw over the observations of weight a_i != 0:
 *     stats_out[k * S * N + t], k =    0  sum of (y_rep - centre)          1  sum of (y_rep - centre)^2
 *                                      2  min y_rep      3  max y_rep      4  number of y_rep <= cut
 *                                      5  sum of log f(y_rep_i | draw t)   6  sum of log f(y_i | draw t)
 * 5 and 6 are the full proper log densities by one code path, the terms pbbi_pointwise_glm leaves to its caller included
 * (log C(n, y); -lgamma(y + 1); the Gaussian constant; -log y), UNWEIGHTED except for the Gaussian family, where a_i is a
 * precision weight (variance sigma^2 / a_i); in the other families a weight changes no replicate's distribution.
 * aux: the image y | n | a on the device -- three runs of 16 * ceil(M / 64) * 4 doubles, zero padded: the response, the
 * binomial trials (1 elsewhere) and the weight.  The handle's own streams are not read, except its offset (0 for a handle of
 * pbbi_potential_create_glm); a likelihood power on the handle changes nothing.  samples_sdn, Dt, the rows that are read and
 * `ranges` (over the observation blocks): as for pbbi_loglik_glm.
 * yrep_out: NULL (keep = 0), or a (keep, M) matrix on the device that receives the replicates of draws t < keep; a row with
 * a_i = 0 is NaN there.  Neither the statistics nor yrep_out depend on `ranges`, on the order tiles run in or on whether yrep_out
 * is given -- a replicate is a function of (seed, t, i) -- except that the SUMS (0, 1, 5, 6) add their ranges in index order, so
 * another `ranges` may change their last bits (integer-valued sums are exact); for a given `ranges` every bit repeats.
 * A non-finite eta or mean gives a NaN replicate; so does a DISCRETE replicate whose distribution has variance above 2^20,
 * which is not served (the inversion walks O(sigma) points per value), and a Gamma value none of whose 64 attempts accepts.  A
 * NaN replicate makes statistics 0, 1, 2, 3 and 5 of its own draw NaN, and no other draw's.
 * Rules, in this order, the first nine those of pbbi_loglik_glm without its output: NULL handle, NULL samples, S < 1, N < 1,
 * ranges outside 0 .. 65535: PBBI_ERR_INVALID; a handle that is no GLM handle, a softmax handle, an unknown family:
 * PBBI_ERR_UNSUPPORTED; Dt below the state dimension; NULL aux; NULL stats_out; S * N > 2^32; keep outside 0 .. S * N; keep > 0
 * without yrep_out or yrep_out with keep = 0; centre or cut not finite; keep * M > 2^28: PBBI_ERR_INVALID.  All before the device
 * is touched.  Shipped: the 22 shapes of pbbi_loglik_glm; none reserves scratch memory. */
int pbbi_predictive_glm(const pbbi_potential* pot, const void* samples_sdn, int S, int Dt, int64_t N, uint64_t seed,
                        const double* aux, double centre, double cut, int ranges, double* stats_out, int64_t keep,
                        double* yrep_out, void* stream);
/* Those rules alone but the last (it needs the handle's M), on the HOST, for a handle described by value (as
 * pbbi_pointwise_glm_check); the pointers are only compared with NULL; yrep_given != 0: yrep_out is given. */
int pbbi_predictive_glm_check(int handle, int family, int state_dim, const void* samples, const void* aux,
                              const void* stats_out, int S, int Dt, int64_t N, int ranges, int64_t keep, int yrep_given,
                              double centre, double cut);
/* The likelihood power of a GLM handle: the handle's potential becomes -log [ p(w) L(w)^beta ] (prior terms untouched), the path
 * from the prior (beta -> 0) to the posterior (beta = 1) of likelihood-tempered SMC.  Raising the likelihood to the power beta is
 * multiplying every observation weight a_i by beta, so no kernel changes: a small kernel writes c <- beta c0 on the handle's
 * observation streams (and d <- beta d0 where d holds a_i y_i: logistic and poisson; the dispersion families keep d = y raw).  The
 * streams as built are copied on the first call and kept.  1.0 * x is exact: at beta = 1 the handle is bit for bit the untouched one.
 * beta_dev != NULL: the kernel reads beta from that device double (a fixed schedule needs no host read; the getter then
 * reports NaN, and the value is not checked); beta_dev == NULL: the host value `beta`, finite and > 0.
 * Every kernel that reads the streams sees the power: pbbi_hmc_iter / pbbi_hmc_run, pbbi_integrate, pbbi_potential_eval,
 * pbbi_energy, pbbi_weights_ratio, pbbi_pointwise_glm.  pbbi_loglik_glm does not (see there).  The power lives on the HANDLE, like
 * the metric: samplers that share a handle share its power, and setting it is ordered only against work on `stream`.
 * Rules, in this order: NULL handle: PBBI_ERR_INVALID; a handle that is no GLM handle, a softmax handle, a handle of
 * pbbi_potential_create_glm (it has no streams: build the model with pbbi_potential_create_glm_ex): PBBI_ERR_UNSUPPORTED with the
 * reason; a host beta that is not finite and > 0: PBBI_ERR_INVALID. */
int pbbi_potential_set_likelihood_power(pbbi_potential* pot, double beta, const double* beta_dev, void* stream);
/* *beta_out <- the power as last set from the host, NaN when it was last read from the device, 1 on a handle never tempered. */
int pbbi_potential_get_likelihood_power(const pbbi_potential* pot, double* beta_out);
/* The rules of pbbi_potential_set_likelihood_power alone, on the HOST, by value: handle as for pbbi_pointwise_glm_check, has_streams
 * != 0: the handle keeps observation streams, beta_on_device != 0: beta_dev is given (beta is then not read). */
int pbbi_likelihood_power_check(int handle, int family, int has_streams, double beta, int beta_on_device);
/* A diagonal metric (mass matrix) on a GLM handle or on a user-defined one (pbbi_potential_create_custom).  With m_d > 0 for each of the D = pbbi_potential_dim(pot) rows of the state
 * -- coefficients, group log-scales and a sampled log-dispersion alike; for a softmax handle the K D rows, class-major -- and
 * the per-chain mass m_n of a call (1 where the call passes none), row d of chain n has mass m_n m_d:
 *     draw    p_d = sqrt(m_n m_d kT) z_d     (z_d: the Philox normals drawn without a metric, same counters, same precision rule)
 *     velocity v_d = p_d / (m_n m_d),   kick v_d -= c h g_d / (m_n m_d),   drift q_d += h v_d
 *     kinetic energy K = 0.5 sum_d p_d^2 / (m_n m_d)
 * in every call that integrates or weighs momenta on the handle: pbbi_hmc_iter(_kt) with in-kernel or uploaded draws,
 * pbbi_hmc_run, compat and non-compat stores, pbbi_leapfrog and pbbi_stormer_verlet (v_out is the velocity above), pbbi_energy,
 * pbbi_weights_ratio, and everything built on them (tempered SMC, the tempering ladder).  pbbi_potential_eval does not see it.
 * A metric of all ones reproduces the handle without one bit for bit.  The device keeps the table {m_d, 1 / m_d} of
 * pbbi_glm_pack_metric and the kernels (the METRIC instantiations of k_glm and k_glm_softmax) hold it in LDS for the launch; a
 * handle without a metric launches the kernels it always has.
 * A user-defined handle keeps the same table in its own dtype (fp64 or fp32), in the same two fields of the handle as a GLM
 * handle; the METRIC instantiations of its plugin's kernels (csrc/pbbi_custom.h) read it at wave-uniform addresses.  The same
 * model holds there with the per-chain mass dividing the kinetic sum last, K = 0.5 (sum_d p_d^2 / m_d) / m_n, in every mode
 * the plugin serves: Leapfrog, Stormer-Verlet and PBBI_KDK_FMA, fused runs, the redraw of a rejected chain.  A register
 * kernel whose METRIC twin would need scratch memory where it needs none is not launched with a metric: the workspace
 * kernels serve that shape instead, and pbbi_describe_run says so.  No shape is refused.
 * The metric lives on the HANDLE because pbbi_hmc_run's signature is fixed: two samplers that share a handle share the metric,
 * and setting it is not ordered against launches in flight on other streams -- synchronise first.
 * mass_diag: D doubles on the host, every one finite and > 0 (else PBBI_ERR_INVALID); NULL removes the metric.  D must equal
 * pbbi_potential_dim(pot) (PBBI_ERR_INVALID).  A handle of any other kind (harmonic, diagonal or dense Gaussian, Rosenbrock), or
 * a GLM handle whose METRIC kernel is not shipped (it would spill registers to memory): PBBI_ERR_UNSUPPORTED with the reason.
 * Per-chain trajectory lengths and GIST stay refused on GLM and user-defined handles with or without a metric. */
int pbbi_potential_set_metric_diag(pbbi_potential* pot, const double* mass_diag, int D);
/* Copies the handle's metric into out (D = pbbi_potential_dim(pot) doubles, out_len >= D; out may be NULL).  *has_out <- 1 when
 * the handle carries a metric, 0 when it does not (out is then left alone).  A handle that is neither a GLM nor a user-defined
 * handle has none. */
int pbbi_potential_get_metric_diag(const pbbi_potential* pot, double* out, int out_len, int* has_out);
/* pbbi_glm_pack_metric, the host-only packer and checker of that table, is declared in pbbi_glm_metric.h (included at the end). */
/* A dense metric (mass matrix) on a GLM handle.  With M symmetric positive definite over the D = pbbi_potential_dim(pot) rows of
 * the state (a sampled log-dispersion among them), M = L L^T (L lower, positive diagonal), C = M^-1 and the per-chain mass m_n of
 * a call, chain n has the mass matrix m_n M:
 *     draw    p = sqrt(m_n kT) L z           (z: the Philox normals drawn without a metric, same counters, same precision rule)
 *     velocity v = C p / m_n,   kick v -= c h C g / m_n,   drift q += h v
 *     kinetic energy K = 0.5 p^T C p / m_n = 0.5 p . v
 * in every call the diagonal metric serves (above); uploaded momenta are p as given, v_out is the velocity above,
 * pbbi_potential_eval does not see it.  The natural choice is the posterior precision (the Hessian at the mode): every
 * frequency of a Gaussian posterior is then 1, whatever the correlation between its rows.  The dense identity reproduces the
 * handle without a metric bit for bit.  The device keeps the three images of pbbi_glm_pack_metric_dense (pbbi_glm_metric.h); the
 * dense-metric instantiations of k_glm hold C in LDS for the launch (8 DP^2 bytes) and form C g on the fp64 matrix cores.
 * A handle carries at most ONE metric: setting either kind removes the other, and NULL to either entry removes whichever is
 * there.  Like the diagonal one it lives on the handle: two samplers that share a handle share the metric.
 * M: (D x D) doubles on the host, row-major, under the rules of pbbi_glm_pack_metric_dense (PBBI_ERR_INVALID); D must equal
 * pbbi_potential_dim(pot).  Served: the handles of pbbi_potential_create_glm, _glm_ex and _glm_dispersion, float64, state
 * dimension <= 64.  Every other handle -- no GLM handle, softmax, ordinal, hierarchical, a wider state -- is refused with
 * PBBI_ERR_UNSUPPORTED and the reason, before the device is touched. */
int pbbi_potential_set_metric_dense(pbbi_potential* pot, const double* M, int D);
/* Copies the handle's dense metric, as it was given, into out (D x D doubles, out_len >= D^2; out may be NULL).  *has_out <- 1
 * when the handle carries a dense metric, 0 when it does not -- a handle with a diagonal metric answers 0 here, and one with a
 * dense metric answers 0 to pbbi_potential_get_metric_diag. */
int pbbi_potential_get_metric_dense(const pbbi_potential* pot, double* out, int64_t out_len, int* has_out);
int pbbi_potential_destroy(pbbi_potential* pot);
int pbbi_potential_dim(const pbbi_potential* pot);
int pbbi_potential_dtype(const pbbi_potential* pot);
int pbbi_potential_device(const pbbi_potential* pot);

/* potential(q[:, n]) and gradient(q[:, n]) for every chain.
 * U_out: N elements or NULL; grad_out: (D, N) with stride ldn or NULL.
 * Replaces the user callables the reference invokes per chain
 * (src/integrator.py:73, src/HMC.py:102,111,114). */
int pbbi_potential_eval(const pbbi_potential* pot, const void* q, int64_t N, int64_t ldn,
                        void* U_out, void* grad_out, void* stream);

/* ---- integrators ---------------------------------------------------------
 * Leapfrog.integrate() src/integrator.py:95-123 / StormerVerlet.integrate()
 * src/integrator.py:127-165, over the whole ensemble, in place on q and p.
 * L = numSteps = int(finalTime/stepSize), computed by the host
 * (src/integrator.py:51).  v_out: optional (D, N) receiving Integrator.v.
 */
int pbbi_integrate(const pbbi_potential* pot, int method, void* q, void* p, const void* mass,
                   void* v_out, int64_t N, int64_t ldn, double h, int L, void* stream);
int pbbi_leapfrog(const pbbi_potential* pot, void* q, void* p, const void* mass, int64_t N,
                  int64_t ldn, double h, int L, void* stream);
int pbbi_stormer_verlet(const pbbi_potential* pot, void* q, void* p, const void* mass, int64_t N,
                        int64_t ldn, double h, int L, void* stream);

/* ---- energies ------------------------------------------------------------
 * H = 0.5*dot(p,p)/mass + potential(q) per chain          src/HMC.py:100-102
 * pbbi_energy: H_out (N) and/or weight_out (N) = exp(-H)  (HMC.getWeights :86-104)
 * pbbi_weights_ratio: exp(oldH - newH)                    (HMC.getWeightsRatio :106-116)
 */
int pbbi_energy(const pbbi_potential* pot, const void* q, const void* p, const void* mass,
                int64_t N, int64_t ldn, void* H_out, void* weight_out, void* stream);
int pbbi_weights_ratio(const pbbi_potential* pot, const void* newQ, const void* newP,
                       const void* oldQ, const void* oldP, const void* mass, int64_t N,
                       int64_t ldn, void* ratio_out, void* stream);

/* ---- fused HMC iteration -------------------------------------------------
 * One pass of the body of HMC.getSamples' loop, src/HMC.py:154-179, fused:
 * integrate -> energies -> ratio -> reject mask -> select -> store.
 *   q_in  (D,N) chain state;  p_in (D,N) freshly drawn momentum;  u_in (N) uniforms
 *   q_out (D,N) <- samples_hmc[:,:,i]   (may alias q_in)
 *   p_out (D,N) <- momentum_hmc[:,:,i]  (may alias p_in; may be NULL)
 *   ratio_out (N) optional; reject_out (N bytes, 1 = rejected) optional.
 * Parity mode: the host uploads the NumPy RandomState stream into p_in / u_in.
 */
int pbbi_hmc_iter(const pbbi_potential* pot, int method, const void* q_in, const void* p_in,
                  const void* u_in, const void* mass, void* q_out, void* p_out, void* ratio_out,
                  uint8_t* reject_out, int64_t N, int64_t ldn, double h, int L, int flags,
                  void* stream);

/* pbbi_hmc_iter for momenta drawn at kT = boltzmannConst*temperature (src/ensemble.py:88): identical
 * to it unless flags has PBBI_BETA_ACCEPT, which needs kT for its accept test. */
int pbbi_hmc_iter_kt(const pbbi_potential* pot, int method, const void* q_in, const void* p_in,
                     const void* u_in, const void* mass, void* q_out, void* p_out, void* ratio_out,
                     uint8_t* reject_out, int64_t N, int64_t ldn, double h, int L, int flags, double kT,
                     void* stream);

/* S iterations of the same loop with momentum and uniforms drawn in-kernel
 * (RNG contract above): iteration i uses draw index iter0+i, chain n uses the
 * global index chain0+n, p = sqrt(mass*kT) * z  (src/ensemble.py:88-91 with
 * kT = boltzmannConst*temperature).
 *   q_state (D,N; stride ldn): in = current positions, out = positions after S iterations
 *   samples_out (S, D, N) dense slabs <- samples_hmc   (device layout is S-major;
 *               the reference's (D,N,S) is a permuted view of it); NULL = burn-in: the S
 *               iterations only advance q_state (momenta_out must then be NULL too)
 *   momenta_out (S, D, N) or NULL;  reject_out (S, N) bytes or NULL;
 *   ratio_out (S, N) or NULL.
 * iter0 + S must not exceed 2^32: the Philox counter carries 32 iteration bits, a larger index
 * would repeat the draws of iteration (index mod 2^32) and is refused (PBBI_ERR_INVALID).  Runs
 * that must not share draws (a warm-up and the sampling that follows) use different seeds.
 * The run is the unit of work: consecutive iterations may share one launch, and the dense-Gaussian paths
 * keep the gradient of the chain's current position between iterations (the loop of src/HMC.py:150-179
 * evaluates it again at the top of every iteration, src/integrator.py:105-108).  Neither changes a
 * result: a run of S iterations equals S runs of one iteration bit for bit.
 */
int pbbi_hmc_run(const pbbi_potential* pot, int method, void* q_state, const void* mass,
                 void* samples_out, void* momenta_out, uint8_t* reject_out, void* ratio_out,
                 int64_t N, int64_t ldn, double h, int L, int S, int flags, uint64_t seed,
                 uint64_t iter0, uint64_t chain0, double kT, void* stream);

/* What pbbi_hmc_run would do with these arguments, in words, written to out (NUL-terminated, truncated to
 * out_len): the kernel family, whether the run carries the gradient between iterations and -- if not -- why
 * (e.g. the dense D = 128 path carries below N = 2^32 / (16 D) = 2 097 152 chains per call only: beyond, the
 * two carried slabs pass the 32-bit buffer offsets), and how many iterations one launch covers.  Nothing is
 * launched. */
int pbbi_describe_run(const pbbi_potential* pot, int method, int64_t N, int64_t ldn, int L, int S, int flags,
                      char* out, int out_len);

/* pbbi_hmc_iter_kt / pbbi_hmc_run with per-chain trajectory lengths (flags PBBI_PER_CHAIN_STEPS,
 * PBBI_UTURN_STOP above).  steps_in (N int32, device; iter only): the chains' step counts, each in
 * [0, L]; NULL = L for every chain.  steps_out (N, or (S, N) for run; may be NULL): the steps each
 * chain took.  Leapfrog only.  Served by the chain-per-lane kernels (harmonic, diagonal Gaussian,
 * Rosenbrock: fp64, D <= 32, reference operation order whatever PBBI_KDK_FMA says, bit-exact with the
 * oracle) and by the dense MFMA kernels (fp64, D <= 256, both flags: the 16-chain tile keeps stepping while
 * one of its chains is live; the U-turn quantity is formed from the kernel's kick-drift-kick values, so a
 * chain whose (q - q_0) . v passes zero within rounding may stop one step apart from a reference-order
 * run); with PBBI_PER_CHAIN_STEPS alone (no U-turn stop) and PBBI_KDK_FMA also by the multi-lane kernels --
 * harmonic / diagonal Gaussian 32 < D <= 256, Rosenbrock 32 < D <= 128, kick-drift-kick form, ~1e-13 from the
 * reference order like every PBBI_KDK_FMA path; other paths return PBBI_ERR_UNSUPPORTED. */
int pbbi_hmc_iter_dyn(const pbbi_potential* pot, int method, const void* q_in, const void* p_in,
                      const void* u_in, const void* mass, const int32_t* steps_in, void* q_out, void* p_out,
                      void* ratio_out, uint8_t* reject_out, int32_t* steps_out, int64_t N, int64_t ldn,
                      double h, int L, int flags, double kT, void* stream);
int pbbi_hmc_run_dyn(const pbbi_potential* pot, int method, void* q_state, const void* mass,
                     void* samples_out, void* momenta_out, uint8_t* reject_out, void* ratio_out,
                     int32_t* steps_out, int64_t N, int64_t ldn, double h, int L, int S, int flags,
                     uint64_t seed, uint64_t iter0, uint64_t chain0, double kT, void* stream);

/* ---- a reversible per-chain dynamic trajectory length: the self-tuning no-U-turn sampler ------------
 * ("no u-turn sampling" is planned in the reference, references/PhysicsBasedHMC_SoHPC2022_WeekPlan.md:16-17;
 * PBBI_UTURN_STOP alone only measures, see above.)  GIST (Bou-Rabee, Carpenter & Marsden 2024): with
 * tau(q, p) = the number of leapfrog steps until (q_j - q_0) . p_j < 0 first holds, at most Lmax,
 *     tau_f = tau(q, p);    L uniform on 1..tau_f  (1 + floor(u tau_f), u from PBBI_STREAM_STEPS);
 *     (q', p') = L steps from (q, p);    tau_b = tau(q', -p');
 *     accept with probability min(1, exp((H - H')/kT_or_1) * tau_f / tau_b * [L <= tau_b]).
 * Every chain adapts its length to where it is, and the chain still leaves exp(-H) invariant: the length is a
 * Gibbs draw whose density enters the Metropolis ratio at both ends.  One iteration is three masked
 * trajectories (forward search, proposal, backward search: the per-chain-length kernels of
 * pbbi_hmc_iter_dyn, so the same potentials / sizes are served: elementwise D <= 32, dense fp64 D <= 256, other
 * handles return PBBI_ERR_UNSUPPORTED) plus an accept kernel; momenta are drawn by pbbi_philox_normal's
 * kernel for the same counters as pbbi_hmc_run (PBBI_DRAW_F64 honoured), the Metropolis uniform is the
 * chain's PBBI_STREAM_UNIFORM draw.  Arguments as pbbi_hmc_run (samples_out required); tau_out (S, 3, N)
 * int32 or NULL receives tau_f, L, tau_b; ratio_out the full acceptance ratio.  flags: PBBI_COMPAT_P_FROM_OLDQ,
 * PBBI_BETA_ACCEPT, PBBI_DRAW_F64.  Restated in oracle/pbbi_oracle.c::oracle_hmc_iter_gist. */
int pbbi_hmc_run_gist(const pbbi_potential* pot, void* q_state, const void* mass, void* samples_out,
                      void* momenta_out, uint8_t* reject_out, void* ratio_out, int32_t* tau_out, int64_t N,
                      int64_t ldn, double h, int Lmax, int S, int flags, uint64_t seed, uint64_t iter0,
                      uint64_t chain0, double kT, void* stream);

/* ---- tempering: replica exchange between temperature rungs ----------------------------
 * The reference draws momenta at kB*T (src/ensemble.py:88) and plans canonical / micro-canonical ensembles
 * (references/PhysicsBasedHMC_SoHPC2022_WeekPlan.md:25-27; Ensemble.setWeights, src/ensemble.py:52-61, is
 * commented out).  A temperature LADDER: the ensemble's N = R*Nr chains form R rungs -- rung r = chains
 * [r*Nr, (r+1)*Nr), sampled at kT_r by pbbi_hmc_run(..., PBBI_BETA_ACCEPT, kT_r) on its block of the state --
 * and this call is the exchange step between them, on the device, one launch after the energy evaluation:
 * for r = parity, parity + 2, ... chain n of rung r and chain n of rung r+1 swap POSITIONS with probability
 *     min(1, exp((beta_r - beta_{r+1}) (U(q_r) - U(q_{r+1})))),   beta_r = 1 / kT_r,
 * which leaves prod_r exp(-beta_r U(q_r)) invariant; hot rungs cross barriers, swaps carry the crossings down
 * to the rung at kT = 1.  betas: R doubles on the DEVICE.  The uniform of a pair is the lower chain's
 * (global index chain0 + r*Nr + n) draw of PBBI_STREAM_SWAP for `iter`, u53 like the Metropolis uniform.
 * swapped_out: ((R-1), Nr) bytes or NULL (rows of the other parity are left alone). */
int pbbi_replica_exchange(const pbbi_potential* pot, void* q, int64_t Nr, int R, int64_t ldn, const double* betas,
                          int parity, uint64_t seed, uint64_t iter, uint64_t chain0, uint8_t* swapped_out,
                          void* stream);

/* ---- RNG (device Philox stream) -------------------------------------------
 * out[d*ldn+n] = scale * z(dim d, chain chain0+n); scale_per_chain (N) overrides
 * scale when non-NULL.  Device-mode counterpart of Ensemble.setPosition /
 * setMomentum (src/ensemble.py:63-93).  dtype of out/scale_per_chain = `dtype`. */
int pbbi_philox_normal(uint64_t seed, int rng_stream, uint64_t iter, uint64_t chain0, int D,
                       int64_t N, int64_t ldn, double scale, const void* scale_per_chain,
                       int dtype, int device, void* out, void* stream);
int pbbi_philox_uniform(uint64_t seed, uint64_t iter, uint64_t chain0, int64_t N, int dtype,
                        int device, void* out, void* stream);
/* out[n] = 1 + floor(u * L) capped at L, u = the PBBI_STREAM_STEPS uniform of chain chain0+n (block
 * 0xFFFFFFFF, same 53-bit construction as the Metropolis uniform): what PBBI_PER_CHAIN_STEPS draws. */
int pbbi_philox_steps(uint64_t seed, uint64_t iter, uint64_t chain0, int64_t N, int L, int device,
                      int32_t* out, void* stream);

/* ---- layout helper --------------------------------------------------------
 * (S, D, N) device slabs -> the reference's (D, N, S) S-fastest array
 * (src/HMC.py:136-145,178-179).  Both device pointers, same dtype. */
int pbbi_transpose_sdn_to_dns(const void* src_sdn, void* dst_dns, int S, int D, int64_t N,
                              int dtype, int device, void* stream);

/* ---- streaming statistics (the sample sink) -----------------------
 * Per-dimension mean and (biased) variance over all S*N draws of (S, D, N) device slabs,
 * without moving the samples off the GPU: mean_out[d], var_out[d] (D elements each, dtype of
 * the slabs; accumulated in fp64, two deterministic stages, no atomics).  The reference only
 * returns the (D, N, S) array (src/HMC.py:136-183); at C2 scale that is 6.7 GB per 100 draws.
 * Accuracy: the sums run about each dimension's first value, so with kappa = |mean| / sd the variance is within
 * (1e-12 + 64 * 2^-53 * kappa) of itself and the mean within 1e-12 * max(|mean|, sd), whatever the offset (floats: + 2^-23). */
int pbbi_sample_moments(const void* samples_sdn, int S, int D, int64_t N, int dtype, int device,
                        void* mean_out, void* var_out, void* stream);

/* Per-CHAIN mean and unbiased variance over the S draws of each (dim, chain): chain_mean_out and
 * chain_var_out are (D, N) device arrays (stride N) in the slabs' dtype, accumulated in fp64
 * (sums about the chain's first draw).  The ingredients of the Gelman-Rubin statistic across the ensemble's chains
 * (HMC.rhat in the Python layer); S >= 2. */
int pbbi_chain_moments(const void* samples_sdn, int S, int D, int64_t N, int dtype, int device,
                       void* chain_mean_out, void* chain_var_out, void* stream);

/* Ensemble-averaged autocovariance of the chains' draws at lags 0..T (T <= PBBI_MAX_LAG):
 *   acov_out[t*D + d] = mean_n (1/S) sum_{s < S-t} (x[s,d,n] - m[d,n]) (x[s+t,d,n] - m[d,n]),
 * m = chain_mean (D, N) from pbbi_chain_moments.  acov_out: (T+1, D) DOUBLES on the device (fp64
 * accumulation, deterministic two-stage reduction over the chains).  chain_mean is in the slabs' dtype: for float slabs
 * a first pass takes each chain's mean of x - m in fp64 and the sums are centred on m plus that, not on the rounded m.
 * The ingredient of the effective sample size of the ensemble (HMC.ess in the Python layer). */
#define PBBI_MAX_LAG 32
int pbbi_chain_autocov(const void* samples_sdn, const void* chain_mean, int S, int D, int64_t N, int T,
                       int dtype, int device, double* acov_out, void* stream);

/* Covariance matrix of all S*N draws: cov_out[i*D + j] = mean((x_i - mean_i)(x_j - mean_j)), D x D
 * DOUBLES on the device, row-major, symmetric; `mean` (D doubles on the device) is subtracted before
 * the products (give the output of pbbi_sample_moments converted to double, or any shift: the result
 * is then the second moment about that point). */
int pbbi_sample_covariance(const void* samples_sdn, int S, int D, int64_t N, int dtype, int device,
                           const double* mean, double* cov_out, void* stream);

/* ---- running statistics: the same quantities merged across chunks on the device -------------
 * A long run yields its draws chunk by chunk ((c, D, N) slabs, HMC.sampleChunks); the four calls above need every
 * draw resident.  Here a device-resident state of DOUBLES is updated by one pass over each chunk and can be
 * finalised at any time; only one chunk is ever resident.  T = the largest lag kept, 0 <= T <= PBBI_MAX_LAG.
 *
 * State, per (dim, chain) (arrays of D*N, chain axis fastest): the shift c = the chain's first draw (y_s = x_s - c),
 * s1 = sum y_s, A_t = sum_{s>=t} y_s y_{s-t} (t = 0..T), the last T and the first T values of y; per ensemble: a
 * shift vector (D; the first slab's mean over the chains), e = sum (x - shift) (D) and the D x D sum of
 * (x - shift)(x - shift)^T.  pbbi_stats_state_len: *doubles_out = (3T + 3) D N + 2 D + D^2 (host only, no device
 * needed): a lag that is not asked for costs no state and no traffic.
 *
 * pbbi_stats_accumulate: adds the c draws of slabs_sdn ((c, D, N), fp64 or fp32 by `dtype`) to `state`, in draw
 *   order.  S_before = the draws the state already holds, given by the CALLER (nothing is read back);
 *   S_before == 0 starts the state (no reset call: whatever the buffer held is overwritten or never read).  Each
 *   draw goes through ONE update (explicit fma for the lagged products), so the per-chain state after S draws is
 *   bit-identical however the S draws were cut into chunks; the D x D sum is accumulated in 16 x 16 tiles over
 *   slices of the chunk and added in a fixed order (deterministic for a given cut; cuts agree to rounding).
 * pbbi_stats_finalize: from a state of S_total draws, with m_n the mean of chain n and delta = s1 / S_total,
 *     sum_{s=t}^{S-1} (x_s - m)(x_{s-t} - m) = A_t - delta (2 s1 - head_t - tail_t) + (S - t) delta^2      (t < S)
 *   (head_t / tail_t = the sum of the first / last t values of y; lags t >= S are exactly 0), reduced over the
 *   chains in two fixed-order stages without atomics.  Outputs are device DOUBLES, any of them may be NULL:
 *     mean_out, var_out (D): as pbbi_sample_moments (var biased, over all S*N draws);
 *     cov_out (D x D): as pbbi_sample_covariance about the mean;
 *     acov_out ((T+1) x D): pbbi_chain_autocov's definition, the 1/S included;
 *     w_out (D): the mean over chains of the unbiased chain variances;  bvar_out (D): the biased variance over
 *     chains of the chain means;  chain_mean_out, chain_var_out (D x N): as pbbi_chain_moments.
 *   mean, var, W, bvar, acov and the per-chain outputs come from the per-chain state alone (bit-stable under
 *   re-chunking); only cov uses the tile sums.  The state is left unchanged: finalise, continue, finalise again.
 * PBBI_ERR_INVALID before any launch: T out of range, c < 1, S_before < 0, a NULL state or slab pointer, an unknown
 * dtype, S_total < 1, S_total < 2 with w_out or chain_var_out given. */
int pbbi_stats_state_len(int D, int64_t N, int T, int64_t* doubles_out);
int pbbi_stats_accumulate(double* state, int D, int64_t N, int T, int64_t S_before, const void* slabs_sdn, int c,
                          int dtype, int device, void* stream);
int pbbi_stats_finalize(const double* state, int D, int64_t N, int T, int64_t S_total, int device, double* mean_out,
                        double* var_out, double* cov_out, double* acov_out, double* w_out, double* bvar_out,
                        double* chain_mean_out, double* chain_var_out, void* stream);

/* ---- running histogram: quantiles and marginal shapes of a long run, one chunk resident -------
 * What no moment yields: per dimension a histogram of `bins` equal bins (PBBI_HIST_MIN_BINS <= bins <=
 * PBBI_HIST_MAX_BINS), pooled over all chains and all draws, accumulated chunk by chunk from the same (c, D, N) slabs
 * as the running statistics.  Every accumulated quantity is an integer count or an exact extreme, so the state after
 * a run is bit-identical however the run was cut into chunks and from run to run.
 *
 * State: D * (bins + 8) words of 8 bytes (pbbi_hist_state_len; host only, no device needed).  Six arrays of D words,
 * then the counts:
 *     lo (D) | hi (D) | inv = bins / (hi - lo) (D) | min (D) | max (D)      doubles
 *     nan (D)                                                               unsigned 64-bit: the NaNs, in no bin
 *     counts (D x (bins + 2))                                               unsigned 64-bit
 *   min / max run over every non-NaN value seen, infinities included (+inf / -inf while there is none).
 * The bin of a value x (converted to double first) of dimension d:
 *     x < lo: bin 0;   x >= hi: bin bins + 1;   else bin 1 + min((int64)floor((x - lo) * inv), bins - 1)
 *   (so -inf lands in bin 0 and +inf in bin bins + 1; the product is not contracted with anything).
 *
 * pbbi_hist_set_range: the explicit range.  lo, hi: HOST arrays of D doubles, lo_d < hi_d, both and their difference
 *   finite.  Writes the header (inv computed on the host in double) and zeroes the counts and nan, min = +inf, max =
 *   -inf.  Waits for the stream once (the header leaves a host buffer).
 * pbbi_hist_accumulate: adds the c draws of slabs_sdn ((c, D, N), fp64 or fp32 by `dtype`) to `state`.  Nothing is
 *   read back.  auto_range = 0 uses the range in the state.  auto_range = 1 (S_before must be 0) starts the state
 *   from this chunk on the device, whatever the buffer held: with a_d, b_d the smallest and largest FINITE value of
 *   the chunk in dimension d (0, 0 if there is none),
 *       span = b - a;  lo = a - margin * span;  hi = b + margin * span;   if !(hi > lo):  lo = a - 0.5, hi = a + 0.5
 *   in this order of operations, then zeroes the counts and counts the chunk in the same call.  margin is ignored
 *   with auto_range = 0.  S_before is only checked (the counts carry no draw index).
 * There is no finalise entry: the state is read once by the caller, quantiles are host arithmetic on the counts.
 * PBBI_ERR_INVALID before any launch: D < 1, N < 1, bins out of range, c < 1, S_before < 0, a NULL state, slab or
 * range pointer, an unknown dtype, lo >= hi or a non-finite bound (or difference), margin < 0 or not finite,
 * auto_range with S_before > 0. */
#define PBBI_HIST_MIN_BINS 16
#define PBBI_HIST_MAX_BINS 4096
int pbbi_hist_state_len(int D, int bins, int64_t* words_out);
int pbbi_hist_set_range(void* state, int D, int bins, const double* lo, const double* hi, int device, void* stream);
int pbbi_hist_accumulate(void* state, int D, int64_t N, int bins, int64_t S_before, const void* slabs_sdn, int c,
                         int dtype, int auto_range, double margin, int device, void* stream);

/* ---- ensemble weights ----------------------------------------------
 * Normalised canonical weights of an ensemble from its per-chain Hamiltonians (pbbi_energy),
 *     w_n = exp(-beta (H_n - H_min)) / sum_m exp(-beta (H_m - H_min)),
 * the normalised form of HMC.getWeights (src/HMC.py:86-104; the reference's commented-out
 * Ensemble.setWeights, src/ensemble.py:52-61) -- computed on the device in three steps so that a
 * SHARDED ensemble can all-reduce the two scalars in between (MIN of *min_out, SUM of *sum_out; both
 * are device doubles):
 *   pbbi_reduce_min        *min_out = min_n x[n]  (NaNs are skipped; +inf for N == 0)
 *   pbbi_canonical_weights w_out[n] = exp(-beta (H[n] - *hmin)),  *sum_out = sum_n w_out[n]
 *   pbbi_scale_inverse     w[n] /= *sum
 * Reductions are two-stage and deterministic (no atomics).  x / H / w are of `dtype`. */
int pbbi_reduce_min(const void* x, int64_t N, int dtype, int device, double* min_out, void* stream);
int pbbi_canonical_weights(const void* H, int64_t N, double beta, const double* hmin, int dtype,
                           int device, void* w_out, double* sum_out, void* stream);
int pbbi_scale_inverse(void* w, int64_t N, const double* sum, int dtype, int device, void* stream);

/* ---- tempered sequential Monte Carlo (physicsbasedbayesianinference_amd/smc.py) ----------------
 * The population steps between the HMC moves of an SMC sampler on the path pi_beta ~ exp(-beta U(q)), stage 0 a
 * reference N(m, sigma^2 I).  U is the (N) output of pbbi_potential_eval (dtype of the state); logw (N), betas,
 * sums and log Z are DOUBLES on the device.  Every sum is an fp64 online log-sum-exp, reduced in two deterministic
 * stages (no atomics).  Non-finite log weights are zero weights.  W_n = exp(logw_n) / sum exp(logw) (logw NULL =
 * uniform).  With q given (stage 1) the incremental log weight of a coefficient c carries the reference term:
 *     l_n = -c U_n + |q_n - m|^2 / (2 sigma^2) + (D/2) log(2 pi sigma^2)        (m = ref_mean, D doubles or NULL = 0)
 * and without q it is l_n = -c U_n.  N >= 1; offsets are 64-bit; ldn >= N.
 *
 * pbbi_smc_ess_scan: one pass over the particles for K candidate coefficients coefs[k] (device doubles):
 *   out[3k] = log sum_n W_n w_n,  out[3k+1] = log sum_n W_n w_n^2,  out[3k+2] = (sum W w)^2 / sum W w^2 (the ESS
 *   as a fraction of N; 0 when no weight is left), out[3K] = log sum_n exp(logw_n).  out: 3K+1 device doubles.
 * pbbi_smc_next_beta: betas[0] = the current beta, betas[1] <- the next one, both on the device.  Searches
 *   dbeta in (0, 1 - beta] for the ESS fraction = target_ess: one pass over a log-spaced grid of 64 candidates in
 *   [1e-8, 1] (1 - beta); with q (stage 1, ESS not monotone) the search starts at the grid's maximiser and, when
 *   even that is below the target, takes it and sets the warning; then 6 passes of 64 interior points each
 *   narrow the bracket to 1/65 (final width <= 6e-12 (1 - beta)).  The result is the bracket's lower end (the
 *   side whose ESS >= target); when all of (0, 1 - beta] is feasible betas[1] = 1.0 exactly.  Fixed passes, no
 *   host round trip.  info_out (2 device doubles or NULL): the warning flag (1.0 / 0.0), the final bracket width.
 * pbbi_smc_reweight: logw_n += l_n with c = betas[1] - betas[0]; stage_out (2 device doubles or NULL) <- the
 *   log-evidence increment log sum W w and the ESS fraction of the updated weights; *logz += the increment
 *   (logz: one device double or NULL).
 * pbbi_smc_resample_systematic: systematic resampling with ONE uniform per stage, in fixed point:
 *   ticks_n = floor(exp(logw_n - max logw) 2^32) (0 for non-finite logw), C = inclusive prefix sum of the ticks
 *   (uint64, exact), T = C_{N-1};  u = ((x1:x0) >> 11) 2^-53 with (x0, x1) the first two words of the Philox block
 *   0xFFFFFFFF of stream PBBI_STREAM_RESAMPLE, iter = stage, chain 0;  uT = floor(k T / 2^53), k the 53-bit integer;
 *   ancestor a_j = the smallest n with C_n > floor((j T + uT) / N), all in exact 128-bit integer arithmetic.
 *   Ancestors do not depend on launch shape or summation order.  A particle below 2^-32 of the largest weight
 *   gets no offspring.  q_out[:, j] = q_in[:, a_j] (q_out must not overlap q_in), logw <- 0.  ess / threshold:
 *   with ess (a device double, e.g. stage_out + 1) given, the call resamples only when *ess < threshold and is
 *   otherwise the identity (q_out = q_in, a_j = j, logw kept) -- a decision taken on the device.  Optional:
 *   ancestors_out (N int32), ticks_out (N uint64), resampled_out (1 byte).  All weights zero: with status_out
 *   (one device int32) the call writes PBBI_ERR_INVALID there, returns PBBI_OK and copies q_in (no host sync);
 *   without it the call waits for the stream and returns PBBI_ERR_INVALID.  N < 2^31, stage < 2^32. */
int pbbi_smc_ess_scan(const void* U, const double* logw, const void* q, const double* ref_mean, double ref_std,
                      int64_t N, int64_t ldn, int D, int K, const double* coefs, int dtype, int device, double* out,
                      void* stream);
int pbbi_smc_next_beta(const void* U, const double* logw, const void* q, const double* ref_mean, double ref_std,
                       int64_t N, int64_t ldn, int D, double target_ess, double* betas, double* info_out, int dtype,
                       int device, void* stream);
int pbbi_smc_reweight(const void* U, const void* q, const double* ref_mean, double ref_std, int64_t N, int64_t ldn,
                      int D, const double* betas, double* logw, double* logz, double* stage_out, int dtype, int device,
                      void* stream);
int pbbi_smc_resample_systematic(double* logw, int64_t N, uint64_t seed, uint64_t stage, const void* q_in,
                                 void* q_out, int64_t ldn, int D, const double* ess, double threshold,
                                 int32_t* ancestors_out, uint64_t* ticks_out, uint8_t* resampled_out,
                                 int32_t* status_out, int dtype, int device, void* stream);

#ifdef __cplusplus
}
#endif
#include "pbbi_glm_metric.h"
#include "pbbi_glm_ordinal.h"
/* pbbi_glm_hessian(pot, q, ranges, hess_out, stream): the Hessian of a GLM handle's potential at one state (posterior mode,
 * Laplace approximation), and its host-only twin pbbi_glm_hessian_check */
#include "pbbi_glm_hessian.h"
#endif /* PBBI_H */
