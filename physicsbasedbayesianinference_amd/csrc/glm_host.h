// glm_host.h -- the host side of the GLM potentials that calls no HIP function (glm_host.cpp): which kernels are shipped,
// the argument rules of the create entries and the packers of what they upload.  Plain C++: no HIP header here, so the
// translation unit links into a stand-alone program (glm_asan_driver.cpp) as well as into libpbbi.so.
#pragma once
#include <stdint.h>

#include <string>

#include "pbbi.h"

int pbbi_fail(int code, const std::string& msg);  // pbbi_api.hip

// The kind of a GLM handle (pbbi_potential::glm_variant): set once by the builder of its create entry, read by the
// launch switch of kernels_glm.hip, the routing and pbbi_describe_run.
enum GlmVariant {
    GLM_V_PLAIN = 0,            // pbbi_potential_create_glm:                 k_glm<NT, FAM, false>
    GLM_V_FULL = 1,             // pbbi_potential_create_glm_ex:              k_glm<NT, FAM, true>
    GLM_V_SOFTMAX = 2,          // pbbi_potential_create_glm_softmax:         k_glm_softmax<NTc, K>
    GLM_V_DISPERSION = 3,       // pbbi_potential_create_glm_dispersion:      k_glm<NT, FAM, true>, FAM = 3, 4, 5
    GLM_V_HIER = 4,             // pbbi_potential_create_glm_hier / _hier_ex: k_glm<NT, FAM, true, GLM_HIER_CENTRED>
    GLM_V_HIER_NC = 5,          // pbbi_potential_create_glm_hier_ex:         k_glm<NT, FAM, true, GLM_HIER_NC>
    GLM_V_HIER_Q = 6,           // pbbi_potential_create_glm_hier_q:          k_glm<NT, FAM, true, GLM_HIER_Q>
    GLM_V_HIER_DISPERSION = 7,  // pbbi_potential_create_glm_hier_dispersion: FAM = 3, 4 with GLM_HIER_CENTRED / GLM_HIER_NC
                                //   (which of the two: pbbi_potential::glm_hier_nc)
    GLM_V_ORDINAL = 8,          // pbbi_potential_create_glm_ordinal:         k_glm<NT, PBBI_GLM_ORDINAL, true>
};
enum { GLM_TERM_WEIGHTS = 1, GLM_TERM_OFFSET = 2, GLM_TERM_TRIALS = 4, GLM_TERM_PRIOR_VECTOR = 8, GLM_TERM_PRIOR_MEAN = 16,
       GLM_TERM_PRIOR_FLAT = 32 };

// The families by the shape of their link: the canonical ones (b(eta) alone) and the ones with a dispersion theta.  The one
// statement of both, for the rules of glm_host.cpp and for the kernels' `if constexpr` (glm_family_dev.h, kernels_glm.hip).
constexpr bool glm_disp(int fam) { return fam == PBBI_GLM_GAUSSIAN || fam == PBBI_GLM_NEGBINOMIAL || fam == PBBI_GLM_GAMMA; }
constexpr bool glm_canonical(int fam) { return fam == PBBI_GLM_LOGISTIC || fam == PBBI_GLM_POISSON; }
// the families' names as the error texts and pbbi_describe_run write them: the one table
constexpr const char* glm_family_name(int fam) {
    constexpr const char* names[] = {"logistic", "poisson", "softmax", "gaussian", "negbinomial", "gamma", "ordinal"};
    return fam >= 0 && fam < (int)(sizeof(names) / sizeof(names[0])) ? names[fam] : "unknown";
}

// The ordinal family's widest shipped kernel, in padded rows: the state is the coefficients and the K - 1 cutpoint rows.  At 128
// rows the kernel reserves 292 bytes of scratch per lane even with all 512 registers (the full model's kernel there already fills
// the file, and the walk adds the cutpoints, the G terms and seven accumulators) and is not shipped
// (profiles/glm_ordinal_resources.txt).
constexpr int GLM_ORDINAL_MAX_ROWS = 64;

// The largest state dimension (every sampled row: coefficients, group log-scales, a sampled log-dispersion) the kernels of a
// variant serve for a family; 0 = nothing shipped.  The one statement of it: the create entries and the launch read this.
int glm_max_dim(int variant, int family);
// ... and glm_max_dim's sibling for the diagonal metric (METRIC = true of k_glm): the largest PADDED row count (16, 32, 64, 128;
// 0 = none) at which the METRIC twin of k_glm<NT, family, rich, hier> builds without scratch at its parent's waves per SIMD
// (profiles/glm_metric_resources.txt).  hier: 0 none, 1 centred, 2 non-centred, 3 structured group priors (GLM_HIER_* of
// kernels_glm.hip).  As built, every METRIC twin of k_glm does where its parent does, so these are glm_max_dim's numbers; the rule
// stays a statement of its own so that a twin that stops fitting is taken out here and nowhere else.  constexpr: the launch
// switch instantiates by it, pbbi_potential_set_metric_diag refuses by it.
constexpr int glm_metric_max_rows(int family, bool rich, int hier) {
    const bool canonical = family == PBBI_GLM_LOGISTIC || family == PBBI_GLM_POISSON;
    if (hier != 0) return 64;
    if (!rich) return canonical ? 128 : 0;
    if (family == PBBI_GLM_ORDINAL) return GLM_ORDINAL_MAX_ROWS;
    return family == PBBI_GLM_NEGBINOMIAL ? 64 : 128;
}
// ... and of k_glm_softmax<Dc / 16, K>: every shape of glm_softmax_layout but the one with Dc = 64 rows per class (K = 2), whose
// METRIC twin reserves 36 bytes of scratch per lane
constexpr bool glm_softmax_metric_ships(int Dc, int K) { return Dc * K <= 128 && Dc < 64; }
// the same question asked of a handle: the largest state dimension its variant's METRIC kernels serve (0 = none).  dp = the
// handle's glm_DP (softmax: the padded class size Dc), K its classes (softmax only)
int glm_metric_max_dim(int variant, int family, int hier_nc, int dp, int K);
// ---- the diagonal metric's table: {m_d, 1 / m_d} of the DP = glm_padded_dim(D) rows, {1, 1} past D (2 DP doubles)
int glm_check_metric(int D, const double* mass_diag);  // every entry finite and > 0
void glm_pack_metric(int D, const double* mass_diag, double* out);
// ... and glm_metric_max_rows' sibling for the dense metric (METRIC = GLM_METRIC_DENSE of k_glm): the largest PADDED row count (16,
// 32, 64; 0 = none) at which the dense twin of k_glm<NT, family, rich, hier> builds without scratch at its parent's waves per SIMD
// (profiles/glm_dense_metric_resources.txt).  The C image alone is 8 DP^2 bytes of LDS, 128 KiB at 128 rows: nothing there.  The
// hierarchical kernels and the ordinal family are not built with it.  constexpr: the launch switch instantiates by it,
// pbbi_potential_set_metric_dense refuses by it.
constexpr int glm_dense_metric_max_rows(int family, bool rich, int hier) {
    if (hier != 0) return 0;
    if (glm_canonical(family)) return 64;
    return rich && glm_disp(family) ? 64 : 0;
}
// the same question asked of a handle: the largest state dimension its variant's dense-metric kernels serve (0 = none)
int glm_dense_metric_max_dim(int variant, int family);
// ---- the dense metric: a (D x D) symmetric positive-definite mass matrix M = L L^T, C = M^-1.  glm_check_metric_dense: 1 <= D <=
// 64 (PBBI_ERR_UNSUPPORTED), every entry finite, max|M - M^T| <= 1e-12 max|M| (the penalty's rule; (M + M^T) / 2 is used), the
// Cholesky factorisation completes with every pivot > 0 (PBBI_ERR_INVALID) -- in that order.  glm_pack_metric_dense: three (DP x
// DP) images, DP = glm_padded_dim(D), in the first product's A-fragment order (the penalty's writer): C, L and M, each the
// identity on the padding rows and columns; 3 DP^2 doubles.
int glm_check_metric_dense(int D, const double* M);
int64_t glm_metric_dense_len(int D);
void glm_pack_metric_dense(int D, const double* M, double* out);

// ---- the design matrix
int glm_padded_dim(int D);                   // 16, 32, 64 or 128
int64_t glm_blocks_padded(int64_t M);        // blocks of 16 observations, padded to a multiple of 4
int64_t glm_image_len(int D, int64_t M);     // doubles of the fragment image of an M x D design matrix
void glm_pack(int D, int64_t M, const double* X, double* out);
void glm_pack_dp(int D, int DP, int64_t M, const double* X, double* out);  // ... of [X | 0] at a padded dimension DP >= D
int glm_check_design(int D, int64_t M, const double* X);                   // every entry finite
// ---- the observation streams (glm_obs_len(M) doubles) and the prior vectors
int64_t glm_obs_len(int64_t M);
int glm_check_obs(int64_t M, int family, const double* y, const double* weights, const double* offset, const double* trials);
void glm_pack_obs(int64_t M, const double* y, const double* weights, const double* offset, const double* trials, double* out);
int glm_check_prior(int D, const double* lam, const double* mu);
int glm_check_obs_disp(int64_t M, int family, const double* y, const double* weights, const double* offset);
void glm_pack_obs_disp(int64_t M, int family, const double* y, const double* weights, const double* offset, double* out);
// ---- the ordinal family: the shape rule (K, and D + K - 1 against glm_max_dim), the observation rules, the streams a | y | o with
// the weighted category counts A_k (8 doubles, 0 past K), and the prior table lam (DP) | mu (DP) | A_k (8) | A_k as built (8)
int glm_check_ordinal_shape(int D, int K);
int glm_check_obs_ordinal(int64_t M, int K, const double* y, const double* weights, const double* offset);
void glm_pack_obs_ordinal(int64_t M, int K, const double* y, const double* weights, const double* offset, double* out,
                          double* counts_out);
// ---- hierarchical priors: the table the kernels keep in LDS, the log-dispersion's pair, the penalty image
int glm_check_hier(int D, int J, const double* lam, const double* mu, const int32_t* groups, const double* tprior);
void glm_pack_prior_groups(int D, int J, const double* lam, const double* mu, const int32_t* groups, const double* tprior,
                           double* out, double* n_out);
int glm_check_hier_disp_theta(int sample, double theta, const double* dprior);
void glm_pack_prior_groups_disp(int D, int J, const double* lam, const double* mu, const int32_t* groups, const double* tprior,
                                int sample, const double* dprior, double* out, double* n_out);
int glm_check_penalty(int D, int J, const int32_t* groups, const double* penalty, const double* rank);
int64_t glm_penalty_image_len(int D, int J);  // doubles of the fragment image of the (DP x DP) penalty
void glm_pack_penalty(int D, int J, const double* penalty, double* out);
// ---- pointwise log-likelihood over draws (kernels_glm_pointwise.hip): every argument rule of pbbi_pointwise_glm.  handle: 0 =
// NULL, 1 = a GLM handle (family, state_dim its own), 2 = a handle of another kind
extern const char* const GLM_POINTWISE_RULE;
int glm_check_pointwise(int handle, int family, int state_dim, const void* sdn, int S, int Dt, int64_t N, int ranges,
                        bool want_var);
// ---- the likelihood energy of each draw (kernels_glm_loglik.hip): every argument rule of pbbi_loglik_glm, `handle` as above
int glm_check_loglik(int handle, int family, int state_dim, const void* sdn, const void* out, int S, int Dt, int64_t N,
                     int ranges);
// ---- posterior predictive replicates (kernels_glm_predictive.hip): every argument rule of pbbi_predictive_glm that needs no
// handle, `handle` as above -- glm_check_draws' first, then aux, stats_out, S * N <= 2^32, keep, centre, cut -- and the one that
// needs the handle's M (keep * M <= 2^28), which the entry checks right after them
int glm_check_predictive(int handle, int family, int state_dim, const void* sdn, const void* aux, const void* stats_out, int S,
                         int Dt, int64_t N, int ranges, int64_t keep, bool yrep_given, double centre, double cut);
int glm_check_predictive_keep(int64_t keep, int64_t M);
// ---- the Hessian at one state (kernels_glm_hessian.hip): every argument rule of pbbi_glm_hessian, `handle` as above;
// hierarchical: the handle has group log-scales (every GLM_V_HIER* variant)
extern const char* const GLM_HESSIAN_RULE;
int glm_check_hessian(int handle, int family, bool hierarchical, const void* q, const void* out, int ranges);
// ---- the likelihood power: every argument rule of pbbi_potential_set_likelihood_power.  has_streams: the handle keeps the
// c | d | o streams (every GLM handle but the plain model's and the softmax's); beta is read only when it comes from the host
extern const char* const GLM_POWER_RULE;
int glm_check_power(int handle, int family, bool has_streams, double beta, bool beta_on_device);
// ---- K-class softmax regression
extern const char* const GLM_SOFTMAX_RULE;
int glm_softmax_layout(int D, int K, int* Dc_out, int* NT_out, int32_t* row_map);
int glm_softmax_check(int D, int K, int64_t M, const double* X, const double* y, const double* lam);
