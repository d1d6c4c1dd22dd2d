// glm_host.cpp -- the host side of the GLM potentials that calls no HIP function: which kernels are shipped, the argument
// rules of the create entries, and the packers that lay the design matrix, the observation streams, the prior table and the
// penalty out the way k_glm and k_glm_softmax read them (kernels_glm.hip and kernels_glm_softmax.hip describe the layouts
// from the device's side).  Plain C++, built once for libpbbi.so and once more, sanitized, with glm_asan_driver.cpp.
#include "glm_host.h"

#include <cmath>
#include <cstring>
#include <vector>

// An instantiation ships only if it builds without scratch (profiles/glm_*_resources.txt).  The frame's widest kernel has 128
// rows.  The full model's kernels at 128 rows already fill the register file, so nothing built on them has one there: not the
// negative binomial (the constants of its exp, log and two series), not the hierarchical priors in any form (172 and 180 bytes
// of scratch per lane for the centred ones), not the dispersion families with random effects.  The softmax kernels' shapes
// are a rule on (D, K): glm_softmax_layout.
int glm_max_dim(int variant, int family) {
    switch (variant) {
        case GLM_V_PLAIN:
        case GLM_V_FULL: return glm_canonical(family) ? 128 : 0;
        case GLM_V_DISPERSION:
            return family == PBBI_GLM_GAUSSIAN || family == PBBI_GLM_GAMMA ? 128 : family == PBBI_GLM_NEGBINOMIAL ? 64 : 0;
        case GLM_V_HIER:
        case GLM_V_HIER_NC:
        case GLM_V_HIER_Q: return glm_canonical(family) ? 64 : 0;
        // (random effects for the Gamma family are not built)
        case GLM_V_HIER_DISPERSION: return family == PBBI_GLM_GAUSSIAN || family == PBBI_GLM_NEGBINOMIAL ? 64 : 0;
        case GLM_V_ORDINAL: return family == PBBI_GLM_ORDINAL ? GLM_ORDINAL_MAX_ROWS : 0;
    }
    return 0;
}

// The diagonal metric: glm_metric_max_rows (glm_host.h) by variant, as a state dimension like glm_max_dim.  A METRIC kernel exists
// only where its parent does, so the answer is never above glm_max_dim's.
int glm_metric_max_dim(int variant, int family, int hier_nc, int dp, int K) {
    int rows = 0;
    switch (variant) {
        case GLM_V_PLAIN: rows = glm_metric_max_rows(family, false, 0); break;
        case GLM_V_FULL:
        case GLM_V_DISPERSION:
        case GLM_V_ORDINAL: rows = glm_metric_max_rows(family, true, 0); break;
        case GLM_V_HIER: rows = glm_metric_max_rows(family, true, 1); break;
        case GLM_V_HIER_NC: rows = glm_metric_max_rows(family, true, 2); break;
        case GLM_V_HIER_Q: rows = glm_metric_max_rows(family, true, 3); break;
        case GLM_V_HIER_DISPERSION: rows = glm_metric_max_rows(family, true, hier_nc ? 2 : 1); break;
        case GLM_V_SOFTMAX: return glm_softmax_metric_ships(dp, K) ? 128 : 0;
    }
    const int parent = glm_max_dim(variant, family);
    return rows < parent ? rows : parent;
}

int glm_check_metric(int D, const double* mass_diag) {
    if (D < 1 || D > 128) return pbbi_fail(PBBI_ERR_INVALID, "metric: need 1 <= D <= 128 (D = " + std::to_string(D) + ")");
    if (!mass_diag) return pbbi_fail(PBBI_ERR_INVALID, "mass_diag is NULL");
    for (int d = 0; d < D; ++d)
        if (!(std::isfinite(mass_diag[d]) && mass_diag[d] > 0.0))
            return pbbi_fail(PBBI_ERR_INVALID, "mass_diag must be finite and > 0 (row " + std::to_string(d) + ")");
    return PBBI_OK;
}

// {m_d, 1 / m_d} per row, the 16-byte entries the kernels stage into LDS; {1, 1} on the padding rows, whose momenta are zero
void glm_pack_metric(int D, const double* mass_diag, double* out) {
    const int DP = glm_padded_dim(D);
    for (int d = 0; d < DP; ++d) {
        out[2 * d] = d < D ? mass_diag[d] : 1.0;
        out[2 * d + 1] = d < D ? 1.0 / mass_diag[d] : 1.0;
    }
}

// the exported packer and checker (include/pbbi.h): the table's length first (out = NULL), the checks before anything is written
int pbbi_glm_pack_metric(int D, const double* mass_diag, double* out, int64_t out_len, int64_t* len_out) {
    if (D < 1 || D > 128) return pbbi_fail(PBBI_ERR_INVALID, "metric: need 1 <= D <= 128 (D = " + std::to_string(D) + ")");
    const int64_t len = 2 * (int64_t)glm_padded_dim(D);
    if (len_out) *len_out = len;
    if (!out) return PBBI_OK;
    if (int rc = glm_check_metric(D, mass_diag)) return rc;
    if (out_len < len) return pbbi_fail(PBBI_ERR_INVALID, "out is shorter than the metric table");
    glm_pack_metric(D, mass_diag, out);
    return PBBI_OK;
}

// ---- the fragment image of X ------------------------------------------------------------------------------------
int glm_padded_dim(int D) { return D <= 16 ? 16 : D <= 32 ? 32 : D <= 64 ? 64 : 128; }
int64_t glm_blocks_padded(int64_t M) { return ((M + 15) / 16 + 3) / 4 * 4; }
int64_t glm_image_len(int D, int64_t M) { return glm_blocks_padded(M) * (int64_t)glm_padded_dim(D) * 32; }

// X (M x D, row-major) -> per block of 16 observations P1 [KS/2][64][2] then P2 [2][NT][64][2] (see the top of
// kernels_glm.hip), zero padded to DP columns and to a multiple of 4 blocks.
void glm_pack(int D, int64_t M, const double* X, double* out) { glm_pack_dp(D, glm_padded_dim(D), M, X, out); }
// the first product's A fragments of block b, P1[s2][lane][e] = at(16 b + (lane & 15), 4 (2 s2 + e) + (lane >> 4)): the one
// statement of that order, for the design (glm_pack_dp) and for the penalty of the structured group priors (glm_pack_penalty)
template <class At>
static void glm_pack_p1(int KS, int64_t b, const At& at, double* P1) {
    for (int l = 0; l < 64; ++l) {
        const int lo = l & 15, hi = l >> 4;
        for (int s2 = 0; s2 < KS / 2; ++s2)
            for (int e = 0; e < 2; ++e)
                P1[((size_t)s2 * 64 + l) * 2 + e] = at(16 * b + lo, 4 * (2 * s2 + e) + hi);
    }
}
// a (DP x DP) matrix as the A operand of a product with the state: DP / 16 blocks of 16 rows, each in that order -- the penalty of
// the structured group priors and the three images of the dense metric
template <class At>
static void glm_pack_square(int DP, const At& at, double* out) {
    const int KS = DP / 4;
    for (int b = 0; b < DP / 16; ++b) glm_pack_p1(KS, b, at, out + (size_t)b * KS * 64);
}
// ... at a padded dimension DP >= D of the caller's: the image of [X | 0]
void glm_pack_dp(int D, int DP, int64_t M, const double* X, double* out) {
    const int NT = DP / 16, KS = DP / 4;
    const int64_t nbp = glm_blocks_padded(M);
    const int64_t blk_len = (int64_t)DP * 32;
    std::memset(out, 0, sizeof(double) * (size_t)(nbp * blk_len));
    auto at = [&](int64_t i, int d) -> double { return (i < M && d < D) ? X[(size_t)i * D + d] : 0.0; };
    for (int64_t b = 0; b < (M + 15) / 16; ++b) {
        double* P1 = out + b * blk_len;
        double* P2 = P1 + (int64_t)KS * 64;
        glm_pack_p1(KS, b, at, P1);
        for (int l = 0; l < 64; ++l) {
            const int lo = l & 15, hi = l >> 4;
            for (int r2 = 0; r2 < 2; ++r2)
                for (int t = 0; t < NT; ++t)
                    for (int e = 0; e < 2; ++e)
                        P2[(((size_t)r2 * NT + t) * 64 + l) * 2 + e] = at(16 * b + 4 * (2 * r2 + e) + hi, 16 * t + lo);
        }
    }
}

int glm_check_design(int D, int64_t M, const double* X) {
    for (int64_t i = 0; i < M * D; ++i)
        if (!std::isfinite(X[i])) return pbbi_fail(PBBI_ERR_INVALID, "X must be finite");
    return PBBI_OK;
}

// ---- the full model's observation streams and prior vectors -----------------------------------------------------
int64_t glm_obs_len(int64_t M) { return 3 * glm_blocks_padded(M) * 16; }

// Every rule of the full model's per-observation arguments (NULL = the default: weights 1, offset 0, trials 1).
int glm_check_obs(int64_t M, int family, const double* y, const double* weights, const double* offset,
                  const double* trials) {
    if (M < 1) return pbbi_fail(PBBI_ERR_INVALID, "M must be >= 1");
    if (!glm_canonical(family)) return pbbi_fail(PBBI_ERR_INVALID, "unknown GLM family");
    if (!y) return pbbi_fail(PBBI_ERR_INVALID, "y is NULL");
    if (trials && family != PBBI_GLM_LOGISTIC)
        return pbbi_fail(PBBI_ERR_INVALID, "trials belong to the logistic (binomial) family only");
    for (int64_t i = 0; i < M; ++i) {
        auto at = [i] { return " (observation " + std::to_string(i) + ")"; };
        const double n = trials ? trials[i] : 1.0;
        if (!std::isfinite(n) || n < 1.0 || n != std::floor(n))
            return pbbi_fail(PBBI_ERR_INVALID, "trials must be integers >= 1" + at());
        if (!std::isfinite(y[i]) || y[i] < 0.0 || y[i] != std::floor(y[i]))
            return pbbi_fail(PBBI_ERR_INVALID, "y must hold non-negative integers" + at());
        if (family == PBBI_GLM_LOGISTIC && y[i] > n)
            return pbbi_fail(PBBI_ERR_INVALID, "logistic: y must not exceed the trials" + at());
        if (weights && !(std::isfinite(weights[i]) && weights[i] >= 0.0))
            return pbbi_fail(PBBI_ERR_INVALID, "weights must be finite and >= 0" + at());
        if (offset && !std::isfinite(offset[i]))
            return pbbi_fail(PBBI_ERR_INVALID, "offset must be finite" + at());
    }
    return PBBI_OK;
}

// c = a n | d = a y | o, each zero padded to the image's block count (glm_obs_len(M) doubles).
void glm_pack_obs(int64_t M, const double* y, const double* weights, const double* offset, const double* trials,
                  double* out) {
    const int64_t len = glm_blocks_padded(M) * 16;
    std::memset(out, 0, sizeof(double) * (size_t)(3 * len));
    for (int64_t i = 0; i < M; ++i) {
        const double a = weights ? weights[i] : 1.0;
        out[i] = a * (trials ? trials[i] : 1.0);
        out[len + i] = a * y[i];
        out[2 * len + i] = offset ? offset[i] : 0.0;
    }
}

int glm_check_prior(int D, const double* lam, const double* mu) {
    if (!lam) return pbbi_fail(PBBI_ERR_INVALID, "prior_precision is NULL");
    for (int d = 0; d < D; ++d) {
        if (!(std::isfinite(lam[d]) && lam[d] >= 0.0))
            return pbbi_fail(PBBI_ERR_INVALID, "prior_precision must be finite and >= 0 (coefficient " + std::to_string(d) + ")");
        if (mu && !std::isfinite(mu[d]))
            return pbbi_fail(PBBI_ERR_INVALID, "prior_mean must be finite (coefficient " + std::to_string(d) + ")");
    }
    return PBBI_OK;
}

// ---- the dispersion families ------------------------------------------------------------------------------------
int glm_check_obs_disp(int64_t M, int family, const double* y, const double* weights, const double* offset) {
    if (M < 1) return pbbi_fail(PBBI_ERR_INVALID, "M must be >= 1");
    if (!glm_disp(family)) return pbbi_fail(PBBI_ERR_INVALID, "unknown dispersion family (gaussian = 3, negbinomial = 4)");
    if (!y) return pbbi_fail(PBBI_ERR_INVALID, "y is NULL");
    for (int64_t i = 0; i < M; ++i) {
        auto at = [i] { return " (observation " + std::to_string(i) + ")"; };
        if (!std::isfinite(y[i])) return pbbi_fail(PBBI_ERR_INVALID, "y must be finite" + at());
        if (family == PBBI_GLM_NEGBINOMIAL && (y[i] < 0.0 || y[i] != std::floor(y[i])))
            return pbbi_fail(PBBI_ERR_INVALID, "negbinomial: y must hold non-negative integers" + at());
        if (family == PBBI_GLM_GAMMA && !(y[i] > 0.0)) return pbbi_fail(PBBI_ERR_INVALID, "gamma: y must be > 0" + at());
        if (weights && !(std::isfinite(weights[i]) && weights[i] >= 0.0))
            return pbbi_fail(PBBI_ERR_INVALID, "weights must be finite and >= 0" + at());
        if (offset && !std::isfinite(offset[i]))
            return pbbi_fail(PBBI_ERR_INVALID, "offset must be finite" + at());
    }
    return PBBI_OK;
}

// c = a | d = y (raw; gamma: log y, all its kernels need of y) | o, each zero padded to the image's block count
// (glm_obs_len(M) doubles).  The caller has run glm_check_obs_disp: a Gamma family's y is > 0.
void glm_pack_obs_disp(int64_t M, int family, const double* y, const double* weights, const double* offset, double* out) {
    const int64_t len = glm_blocks_padded(M) * 16;
    std::memset(out, 0, sizeof(double) * (size_t)(3 * len));
    for (int64_t i = 0; i < M; ++i) {
        out[i] = weights ? weights[i] : 1.0;
        out[len + i] = family == PBBI_GLM_GAMMA ? std::log(y[i]) : y[i];
        out[2 * len + i] = offset ? offset[i] : 0.0;
    }
}

// ---- the ordinal family -----------------------------------------------------------------------------------------
int glm_check_ordinal_shape(int D, int K) {
    if (D < 1) return pbbi_fail(PBBI_ERR_INVALID, "D must be >= 1");
    if (K < 2 || K > 8)
        return pbbi_fail(PBBI_ERR_INVALID, "ordinal: the number of categories K must be 2 .. 8 (K = " + std::to_string(K) + ")");
    const int top = glm_max_dim(GLM_V_ORDINAL, PBBI_GLM_ORDINAL);
    if (D + K - 1 > top)
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, "ordinal: the state dimension (coefficients + K - 1 cutpoint rows) must be <= " +
                                                   std::to_string(top) + " (" + std::to_string(D + K - 1) + ")");
    return PBBI_OK;
}

int glm_check_obs_ordinal(int64_t M, int K, const double* y, const double* weights, const double* offset) {
    if (M < 1) return pbbi_fail(PBBI_ERR_INVALID, "M must be >= 1");
    if (K < 2 || K > 8)
        return pbbi_fail(PBBI_ERR_INVALID, "ordinal: the number of categories K must be 2 .. 8 (K = " + std::to_string(K) + ")");
    if (!y) return pbbi_fail(PBBI_ERR_INVALID, "y is NULL");
    for (int64_t i = 0; i < M; ++i) {
        auto at = [i] { return " (observation " + std::to_string(i) + ")"; };
        if (!(std::isfinite(y[i]) && y[i] >= 0.0 && y[i] < (double)K && y[i] == std::floor(y[i])))
            return pbbi_fail(PBBI_ERR_INVALID, "ordinal: y must hold integer categories in [0, K)" + at());
        if (weights && !(std::isfinite(weights[i]) && weights[i] >= 0.0))
            return pbbi_fail(PBBI_ERR_INVALID, "weights must be finite and >= 0" + at());
        if (offset && !std::isfinite(offset[i]))
            return pbbi_fail(PBBI_ERR_INVALID, "offset must be finite" + at());
    }
    return PBBI_OK;
}

// c = a | d = y (the category) | o, each zero padded to the image's block count (glm_obs_len(M) doubles); counts_out[k] = A_k =
// the sum of the weights of category k, 8 doubles, 0 past K.  The caller has run glm_check_obs_ordinal.
void glm_pack_obs_ordinal(int64_t M, int K, const double* y, const double* weights, const double* offset, double* out,
                          double* counts_out) {
    (void)K;
    const int64_t len = glm_blocks_padded(M) * 16;
    std::memset(out, 0, sizeof(double) * (size_t)(3 * len));
    for (int k = 0; k < 8; ++k) counts_out[k] = 0.0;
    for (int64_t i = 0; i < M; ++i) {
        const double a = weights ? weights[i] : 1.0;
        out[i] = a;
        out[len + i] = y[i];
        out[2 * len + i] = offset ? offset[i] : 0.0;
        counts_out[(int)y[i]] += a;
    }
}

// ---- the hierarchical prior -------------------------------------------------------------------------------------
// Every rule of the hierarchical prior's arguments: groups (D entries, -1 or 0 .. J-1, every index used), the fixed rows'
// {lam, mu}, the J pairs (mean, precision) of the log-scales.
int glm_check_hier(int D, int J, const double* lam, const double* mu, const int32_t* groups, const double* tprior) {
    if (D < 1) return pbbi_fail(PBBI_ERR_INVALID, "D must be >= 1");
    if (J < 1 || J > 4)
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, "hierarchical prior: the number of groups J must be 1 .. 4 (J = " +
                                                   std::to_string(J) + ")");
    if (!groups) return pbbi_fail(PBBI_ERR_INVALID, "groups is NULL");
    if (!lam) return pbbi_fail(PBBI_ERR_INVALID, "prior_precision is NULL");
    if (!tprior) return pbbi_fail(PBBI_ERR_INVALID, "log_scale_prior is NULL");
    int count[4] = {0, 0, 0, 0};
    for (int d = 0; d < D; ++d) {
        if (groups[d] < -1 || groups[d] >= J)
            return pbbi_fail(PBBI_ERR_INVALID, "groups must hold -1 (fixed prior) or a group index 0 .. J-1 (coefficient " +
                                                   std::to_string(d) + ": " + std::to_string(groups[d]) + ", J = " +
                                                   std::to_string(J) + ")");
        if (groups[d] >= 0) ++count[groups[d]];
        // a grouped coefficient's fixed precision is not used
        if (groups[d] < 0 && !(std::isfinite(lam[d]) && lam[d] >= 0.0))
            return pbbi_fail(PBBI_ERR_INVALID, "prior_precision must be finite and >= 0 (coefficient " + std::to_string(d) + ")");
        if (mu && !std::isfinite(mu[d]))
            return pbbi_fail(PBBI_ERR_INVALID, "prior_mean must be finite (coefficient " + std::to_string(d) + ")");
    }
    for (int j = 0; j < J; ++j) {
        if (count[j] == 0)
            return pbbi_fail(PBBI_ERR_INVALID, "every group index 0 .. J-1 must be used (group " + std::to_string(j) +
                                                   " has no coefficient)");
        if (!std::isfinite(tprior[2 * j]) || !(std::isfinite(tprior[2 * j + 1]) && tprior[2 * j + 1] >= 0.0))
            return pbbi_fail(PBBI_ERR_INVALID, "log_scale_prior must hold J pairs (finite mean, finite precision >= 0) "
                                               "(group " + std::to_string(j) + ")");
    }
    return PBBI_OK;
}

// The table the hierarchical kernels stage into plds, lam (DP) | mu (DP) with DP = glm_padded_dim(D + J): a fixed row its
// {lam_d, mu_d}, a member of group j {-(j + 1), mu_d}, row D + j {lam_tj, m_tj}, zeros past D + J; n_out[j] = the members
// of group j.  The caller has run glm_check_hier.
void glm_pack_prior_groups(int D, int J, const double* lam, const double* mu, const int32_t* groups, const double* tprior,
                           double* out, double* n_out) {
    const int DP = glm_padded_dim(D + J);
    std::memset(out, 0, sizeof(double) * (size_t)(2 * DP));
    for (int j = 0; j < J; ++j) n_out[j] = 0.0;
    for (int d = 0; d < D; ++d) {
        out[d] = groups[d] < 0 ? lam[d] : -(double)(groups[d] + 1);
        out[DP + d] = mu ? mu[d] : 0.0;
        if (groups[d] >= 0) n_out[groups[d]] += 1.0;
    }
    for (int j = 0; j < J; ++j) {
        out[D + j] = tprior[2 * j + 1];
        out[DP + D + j] = tprior[2 * j];
    }
}

// ---- random effects for the dispersion families -----------------------------------------------------------------
// Every rule of the log-dispersion's arguments: sampled, a pair (finite mean, finite precision >= 0) is required; held, theta
// must be finite and there is no prior to give.
int glm_check_hier_disp_theta(int sample, double theta, const double* dprior) {
    if (sample) {
        if (!dprior) return pbbi_fail(PBBI_ERR_INVALID, "log_dispersion_prior is NULL (a sampled dispersion needs its pair (mean, precision))");
        if (!std::isfinite(dprior[0]) || !(std::isfinite(dprior[1]) && dprior[1] >= 0.0))
            return pbbi_fail(PBBI_ERR_INVALID, "log_dispersion_prior must be (finite mean, finite precision >= 0)");
    } else {
        if (dprior) return pbbi_fail(PBBI_ERR_INVALID, "log_dispersion_prior belongs to a sampled dispersion only: a held one has no prior");
        if (!std::isfinite(theta))
            return pbbi_fail(PBBI_ERR_INVALID, "a held dispersion must be finite and > 0 (theta = its logarithm)");
    }
    return PBBI_OK;
}

// The table of glm_pack_prior_groups at DP = glm_padded_dim(D + J + (sample ? 1 : 0)), with theta's {lam_theta, m_theta} at row
// D + J when it is sampled (a fixed row: a non-negative lam slot) and zeros past the state.  The caller has run glm_check_hier
// and glm_check_hier_disp_theta.
void glm_pack_prior_groups_disp(int D, int J, const double* lam, const double* mu, const int32_t* groups, const double* tprior,
                                int sample, const double* dprior, double* out, double* n_out) {
    const int DP = glm_padded_dim(D + J + (sample ? 1 : 0)), DPh = glm_padded_dim(D + J);
    std::vector<double> tab((size_t)2 * DPh);
    glm_pack_prior_groups(D, J, lam, mu, groups, tprior, tab.data(), n_out);  // the one statement of the codes
    std::memset(out, 0, sizeof(double) * (size_t)(2 * DP));
    for (int d = 0; d < D + J; ++d) {
        out[d] = tab[(size_t)d];
        out[DP + d] = tab[(size_t)DPh + d];
    }
    if (sample) {
        out[D + J] = dprior[1];
        out[DP + D + J] = dprior[0];
    }
}

// ---- structured group priors ------------------------------------------------------------------------------------
int64_t glm_penalty_image_len(int D, int J) { const int64_t DP = glm_padded_dim(D + J); return DP * DP; }

// The eigenvalues of a symmetric n x n matrix (row-major in a, destroyed) by cyclic Jacobi rotations, into ev.  n <= 63 here.
static void glm_sym_eigenvalues(int n, std::vector<double>& a, std::vector<double>& ev) {
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < n; ++k) (i == k ? diag : off) += a[(size_t)i * n + k] * a[(size_t)i * n + k];
        if (off <= 1e-30 * diag || off == 0.0) break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = a[(size_t)p * n + q];
                if (apq == 0.0) continue;
                const double theta = (a[(size_t)q * n + q] - a[(size_t)p * n + p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; ++k) {  // columns p, q
                    const double akp = a[(size_t)k * n + p], akq = a[(size_t)k * n + q];
                    a[(size_t)k * n + p] = c * akp - s * akq;
                    a[(size_t)k * n + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {  // rows p, q
                    const double apk = a[(size_t)p * n + k], aqk = a[(size_t)q * n + k];
                    a[(size_t)p * n + k] = c * apk - s * aqk;
                    a[(size_t)q * n + k] = s * apk + c * aqk;
                }
            }
    }
    ev.resize((size_t)n);
    for (int i = 0; i < n; ++i) ev[(size_t)i] = a[(size_t)i * n + i];
}

// Every rule of the penalty of the structured group priors: a (D x D) row-major matrix in coefficient indexing, finite,
// zero on fixed rows and between different groups, each group's block symmetric to 1e-12 of its largest entry, positive
// semi-definite (smallest eigenvalue >= -1e-10 x the largest) and not zero; rank[j] an integer in 1 .. n_j.  The caller has
// run glm_check_hier.
int glm_check_penalty(int D, int J, const int32_t* groups, const double* penalty, const double* rank) {
    if (!penalty) return pbbi_fail(PBBI_ERR_INVALID, "penalty is NULL");
    if (!rank) return pbbi_fail(PBBI_ERR_INVALID, "penalty_rank is NULL");
    for (int a = 0; a < D; ++a)
        for (int b = 0; b < D; ++b) {
            const double v = penalty[(size_t)a * D + b];
            if (!std::isfinite(v))
                return pbbi_fail(PBBI_ERR_INVALID, "penalty must be finite (entry " + std::to_string(a) + ", " + std::to_string(b) + ")");
            if (v != 0.0 && (groups[a] < 0 || groups[a] != groups[b]))
                return pbbi_fail(PBBI_ERR_INVALID, "penalty must be zero on fixed rows and between different groups (entry " +
                                                       std::to_string(a) + ", " + std::to_string(b) + ")");
        }
    for (int j = 0; j < J; ++j) {
        std::vector<int> idx;
        for (int d = 0; d < D; ++d)
            if (groups[d] == j) idx.push_back(d);
        const int n = (int)idx.size();
        const std::string grp = " (group " + std::to_string(j) + ")";
        double big = 0.0, asym = 0.0;
        std::vector<double> blk((size_t)n * n);
        for (int a = 0; a < n; ++a)
            for (int b = 0; b < n; ++b) {
                const double v = penalty[(size_t)idx[a] * D + idx[b]], vt = penalty[(size_t)idx[b] * D + idx[a]];
                big = std::fmax(big, std::fabs(v));
                asym = std::fmax(asym, std::fabs(v - vt));
                blk[(size_t)a * n + b] = 0.5 * (v + vt);
            }
        if (big == 0.0) return pbbi_fail(PBBI_ERR_INVALID, "penalty must not be the zero matrix" + grp);
        if (asym > 1e-12 * big) return pbbi_fail(PBBI_ERR_INVALID, "penalty must be symmetric" + grp);
        std::vector<double> ev;
        glm_sym_eigenvalues(n, blk, ev);
        double lo = ev[0], hi = ev[0];
        for (double v : ev) { lo = std::fmin(lo, v); hi = std::fmax(hi, v); }
        if (!(hi > 0.0) || lo < -1e-10 * hi)
            return pbbi_fail(PBBI_ERR_INVALID, "penalty must be positive semi-definite" + grp);
        if (!std::isfinite(rank[j]) || rank[j] != std::floor(rank[j]) || rank[j] < 1.0 || rank[j] > (double)n)
            return pbbi_fail(PBBI_ERR_INVALID, "penalty_rank must be an integer in 1 .. n_j" + grp);
    }
    return PBBI_OK;
}

// The image of the (DP x DP) penalty the kernel keeps in LDS, DP = glm_padded_dim(D + J): DP / 16 blocks of 16 rows, each in
// the first product's A-fragment order (glm_pack_p1), (Q + Q^T) / 2 on rows and columns < D and zero beyond.
void glm_pack_penalty(int D, int J, const double* penalty, double* out) {
    const int DP = glm_padded_dim(D + J);
    auto at = [&](int64_t i, int d) -> double {
        return (i < D && d < D) ? 0.5 * (penalty[(size_t)i * D + d] + penalty[(size_t)d * D + i]) : 0.0;
    };
    glm_pack_square(DP, at, out);
}

// ---- the dense metric ---------------------------------------------------------------------------------------------
int glm_dense_metric_max_dim(int variant, int family) {
    int rows = 0;
    switch (variant) {
        case GLM_V_PLAIN: rows = glm_dense_metric_max_rows(family, false, 0); break;
        case GLM_V_FULL:
        case GLM_V_DISPERSION: rows = glm_dense_metric_max_rows(family, true, 0); break;
        default: return 0;  // softmax, ordinal and every hierarchical variant: no dense-metric kernel is built
    }
    const int parent = glm_max_dim(variant, family);
    return rows < parent ? rows : parent;
}

// The lower Cholesky factor of the symmetric (D x D) matrix a (row-major) into l (zero above the diagonal); false where a pivot
// is not > 0 (or not a number): the matrix is not positive definite.
static bool glm_cholesky(int D, const std::vector<double>& a, std::vector<double>& l) {
    l.assign((size_t)D * D, 0.0);
    for (int j = 0; j < D; ++j) {
        double piv = a[(size_t)j * D + j];
        for (int k = 0; k < j; ++k) piv -= l[(size_t)j * D + k] * l[(size_t)j * D + k];
        if (!(piv > 0.0) || !std::isfinite(piv)) return false;
        const double ljj = std::sqrt(piv);
        l[(size_t)j * D + j] = ljj;
        for (int i = j + 1; i < D; ++i) {
            double s = a[(size_t)i * D + j];
            for (int k = 0; k < j; ++k) s -= l[(size_t)i * D + k] * l[(size_t)j * D + k];
            l[(size_t)i * D + j] = s / ljj;
        }
    }
    return true;
}

// (M + M^T) / 2 of the caller's matrix
static std::vector<double> glm_symmetrised(int D, const double* M) {
    std::vector<double> a((size_t)D * D);
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) a[(size_t)i * D + j] = 0.5 * (M[(size_t)i * D + j] + M[(size_t)j * D + i]);
    return a;
}

// the dense metric's rule on the dimension, stated once for the checker and for the packer's length call
static int glm_check_metric_dense_dim(int D) {
    if (D < 1 || D > 64)
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, "dense metric: need 1 <= D <= 64 (D = " + std::to_string(D) + "): the kernels keep the "
                                               "(DP x DP) inverse in LDS, 8 DP^2 bytes");
    return PBBI_OK;
}

int glm_check_metric_dense(int D, const double* M) {
    if (int rc = glm_check_metric_dense_dim(D)) return rc;
    if (!M) return pbbi_fail(PBBI_ERR_INVALID, "dense metric: M is NULL");
    double big = 0.0, asym = 0.0;
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) {
            const double v = M[(size_t)i * D + j];
            if (!std::isfinite(v))
                return pbbi_fail(PBBI_ERR_INVALID, "dense metric: M must be finite (entry " + std::to_string(i) + ", " + std::to_string(j) + ")");
            big = std::fmax(big, std::fabs(v));
            asym = std::fmax(asym, std::fabs(v - M[(size_t)j * D + i]));
        }
    if (asym > 1e-12 * big) return pbbi_fail(PBBI_ERR_INVALID, "dense metric: M must be symmetric (max|M - M^T| <= 1e-12 max|M|)");
    std::vector<double> l;
    if (!glm_cholesky(D, glm_symmetrised(D, M), l))
        return pbbi_fail(PBBI_ERR_INVALID, "dense metric: M must be positive definite (the Cholesky factorisation met a pivot <= 0)");
    return PBBI_OK;
}

int64_t glm_metric_dense_len(int D) { return 3 * (int64_t)glm_padded_dim(D) * glm_padded_dim(D); }

// C = M^-1 | L | M, each (DP x DP) in the first product's A-fragment order (glm_pack_square), the identity on rows and columns >=
// D.  The caller has run glm_check_metric_dense.  C from the factor: column j of L^-1 by forward substitution, C = L^-T L^-1.
void glm_pack_metric_dense(int D, const double* M, double* out) {
    const int DP = glm_padded_dim(D);
    const std::vector<double> a = glm_symmetrised(D, M);
    std::vector<double> l, li((size_t)D * D, 0.0), c((size_t)D * D, 0.0);
    glm_cholesky(D, a, l);
    for (int j = 0; j < D; ++j)
        for (int i = j; i < D; ++i) {
            double s = i == j ? 1.0 : 0.0;
            for (int k = j; k < i; ++k) s -= l[(size_t)i * D + k] * li[(size_t)k * D + j];
            li[(size_t)i * D + j] = s / l[(size_t)i * D + i];
        }
    for (int i = 0; i < D; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = 0.0;
            for (int k = i; k < D; ++k) s += li[(size_t)k * D + i] * li[(size_t)k * D + j];
            c[(size_t)i * D + j] = c[(size_t)j * D + i] = s;
        }
    const std::vector<double>* src[3] = {&c, &l, &a};
    for (int m = 0; m < 3; ++m) {
        const std::vector<double>& v = *src[m];
        auto at = [&](int64_t i, int d) -> double { return (i < D && d < D) ? v[(size_t)i * D + d] : (i == d ? 1.0 : 0.0); };
        glm_pack_square(DP, at, out + (size_t)m * DP * DP);
    }
}

// the exported packer and checker (include/pbbi_glm_metric.h): the images' length first (out = NULL), the checks before anything
// is written
int pbbi_glm_pack_metric_dense(int D, const double* M, double* out, int64_t out_len, int64_t* len_out) {
    if (int rc = glm_check_metric_dense_dim(D)) return rc;
    const int64_t len = glm_metric_dense_len(D);
    if (len_out) *len_out = len;
    if (!out) return PBBI_OK;
    if (int rc = glm_check_metric_dense(D, M)) return rc;
    if (out_len < len) return pbbi_fail(PBBI_ERR_INVALID, "out is shorter than the dense metric's images");
    glm_pack_metric_dense(D, M, out);
    return PBBI_OK;
}

// ---- pointwise log-likelihood over draws ------------------------------------------------------------------------
const char* const GLM_POINTWISE_RULE = "pbbi_pointwise_glm serves the handles of pbbi_potential_create_glm, _glm_ex, "
                                       "_glm_dispersion, _glm_hier, _glm_hier_ex, _glm_hier_q and _glm_hier_dispersion "
                                       "(families logistic, poisson, gaussian, negbinomial, gamma; float64)";

// The rules of the two entries that take draws, in the order both state them.  Each entry has one rule of its own, at its own
// place: pbbi_loglik_glm's output (out_null: never set by pbbi_pointwise_glm, whose four outputs are all optional) and
// pbbi_pointwise_glm's var_out (want_var: never set by pbbi_loglik_glm).  `entry` is what pbbi_loglik_glm puts before the rules
// on the handle's kind ("pbbi_loglik_glm: "); pbbi_pointwise_glm puts nothing there.
static int glm_check_draws(const char* entry, int handle, int family, int state_dim, const void* sdn, bool out_null, int S,
                           int Dt, int64_t N, int ranges, bool want_var) {
    if (handle == 0) return pbbi_fail(PBBI_ERR_INVALID, "potential handle is NULL");
    if (!sdn) return pbbi_fail(PBBI_ERR_INVALID, "samples is NULL");
    if (out_null) return pbbi_fail(PBBI_ERR_INVALID, "ulik_out is NULL");
    if (S < 1) return pbbi_fail(PBBI_ERR_INVALID, "S must be >= 1 (S = " + std::to_string(S) + ")");
    if (N < 1) return pbbi_fail(PBBI_ERR_INVALID, "N must be >= 1 (N = " + std::to_string(N) + ")");
    if (want_var && S == 1 && N == 1)  // S * N < 2 without forming the product
        return pbbi_fail(PBBI_ERR_INVALID, "var_out needs at least two draws (S * N = 1): pass NULL");
    if (ranges < 0 || ranges > 65535)
        return pbbi_fail(PBBI_ERR_INVALID, "ranges must be 0 (the library chooses) or 1 .. 65535 (ranges = " +
                                               std::to_string(ranges) + ")");
    if (handle != 1)
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, std::string(entry) + "not a GLM handle: " + GLM_POINTWISE_RULE);
    if (family == PBBI_GLM_SOFTMAX)
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, std::string(entry) + "a softmax handle is not served: " + GLM_POINTWISE_RULE);
    if (!glm_canonical(family) && !glm_disp(family) && family != PBBI_GLM_ORDINAL)
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, std::string(entry) + "unknown GLM family: " + GLM_POINTWISE_RULE);
    if (Dt < state_dim)
        return pbbi_fail(PBBI_ERR_INVALID, "Dt must be at least the handle's state dimension (Dt = " + std::to_string(Dt) +
                                               ", state dimension " + std::to_string(state_dim) + ")");
    return PBBI_OK;
}

int glm_check_pointwise(int handle, int family, int state_dim, const void* sdn, int S, int Dt, int64_t N, int ranges,
                        bool want_var) {
    return glm_check_draws("", handle, family, state_dim, sdn, false, S, Dt, N, ranges, want_var);
}

// ---- the likelihood energy of each draw -------------------------------------------------------------------------
int glm_check_loglik(int handle, int family, int state_dim, const void* sdn, const void* out, int S, int Dt, int64_t N,
                     int ranges) {
    return glm_check_draws("pbbi_loglik_glm: ", handle, family, state_dim, sdn, out == nullptr, S, Dt, N, ranges, false);
}

// ---- posterior predictive replicates ----------------------------------------------------------------------------
// The rules pbbi_predictive_glm shares with the two entries above first (glm_check_draws: no output rule, no var_out), then its own.
int glm_check_predictive(int handle, int family, int state_dim, const void* sdn, const void* aux, const void* stats_out, int S,
                         int Dt, int64_t N, int ranges, int64_t keep, bool yrep_given, double centre, double cut) {
    if (int rc = glm_check_draws("pbbi_predictive_glm: ", handle, family, state_dim, sdn, false, S, Dt, N, ranges, false)) return rc;
    if (!aux) return pbbi_fail(PBBI_ERR_INVALID, "aux is NULL");
    if (!stats_out) return pbbi_fail(PBBI_ERR_INVALID, "stats_out is NULL");
    const int64_t two32 = (int64_t)1 << 32;
    if (N > two32 || (int64_t)S * N > two32)  // S < 2^31 and N <= 2^32: the product is below 2^63
        return pbbi_fail(PBBI_ERR_INVALID, "S * N must be <= 2^32: the draw index is the 32-bit iteration word of the counter "
                                           "(S = " + std::to_string(S) + ", N = " + std::to_string(N) + ")");
    if (keep < 0 || keep > (int64_t)S * N)
        return pbbi_fail(PBBI_ERR_INVALID, "keep must be in 0 .. S * N (keep = " + std::to_string(keep) + ")");
    if ((keep > 0) != yrep_given)
        return pbbi_fail(PBBI_ERR_INVALID, keep > 0 ? "keep > 0 needs yrep_out" : "yrep_out needs keep > 0: pass NULL");
    if (!std::isfinite(centre)) return pbbi_fail(PBBI_ERR_INVALID, "centre must be finite");
    if (!std::isfinite(cut)) return pbbi_fail(PBBI_ERR_INVALID, "cut must be finite");
    return PBBI_OK;
}

int glm_check_predictive_keep(int64_t keep, int64_t M) {
    const int64_t cap = (int64_t)1 << 28;
    if (keep > 0 && (keep > cap || keep * M > cap))
        return pbbi_fail(PBBI_ERR_INVALID, "keep * M must be <= 2^28 values of yrep_out (keep = " + std::to_string(keep) +
                                               ", M = " + std::to_string(M) + ")");
    return PBBI_OK;
}

// ---- the Hessian at one state -----------------------------------------------------------------------------------
const char* const GLM_HESSIAN_RULE = "pbbi_glm_hessian serves the handles of pbbi_potential_create_glm, _glm_ex and "
                                     "_glm_dispersion (families logistic, poisson, gaussian, negbinomial, gamma; float64; "
                                     "theta sampled or held)";

// The rules of pbbi_glm_hessian, in the order it states them: the arguments first, then the handle's kind.
int glm_check_hessian(int handle, int family, bool hierarchical, const void* q, const void* out, int ranges) {
    const std::string entry = "pbbi_glm_hessian: ";
    if (handle == 0) return pbbi_fail(PBBI_ERR_INVALID, "potential handle is NULL");
    if (!q) return pbbi_fail(PBBI_ERR_INVALID, "q is NULL");
    if (!out) return pbbi_fail(PBBI_ERR_INVALID, "hess_out is NULL");
    if (ranges < 0 || ranges > 65535)
        return pbbi_fail(PBBI_ERR_INVALID, "ranges must be 0 (the library chooses) or 1 .. 65535 (ranges = " +
                                               std::to_string(ranges) + ")");
    if (handle != 1) return pbbi_fail(PBBI_ERR_UNSUPPORTED, entry + "not a GLM handle: " + GLM_HESSIAN_RULE);
    if (family == PBBI_GLM_SOFTMAX)
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, entry + "a softmax handle is not served: " + GLM_HESSIAN_RULE);
    if (family == PBBI_GLM_ORDINAL)
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, entry + "an ordinal handle is not served: " + GLM_HESSIAN_RULE);
    if (hierarchical)
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, entry + "a hierarchical handle (sampled group scales) is not served: " +
                                                   GLM_HESSIAN_RULE);
    if (!glm_canonical(family) && !glm_disp(family))
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, entry + "unknown GLM family: " + GLM_HESSIAN_RULE);
    return PBBI_OK;
}

// ---- the likelihood power ---------------------------------------------------------------------------------------
const char* const GLM_POWER_RULE = "a likelihood power is served on the handles that keep observation streams: "
                                   "pbbi_potential_create_glm_ex, _glm_dispersion, _glm_hier, _glm_hier_ex, _glm_hier_q and "
                                   "_glm_hier_dispersion (a plain model is built as _glm_ex with weights 1 for it)";

int glm_check_power(int handle, int family, bool has_streams, double beta, bool beta_on_device) {
    if (handle == 0) return pbbi_fail(PBBI_ERR_INVALID, "potential handle is NULL");
    if (handle != 1) return pbbi_fail(PBBI_ERR_UNSUPPORTED, std::string("not a GLM handle: ") + GLM_POWER_RULE);
    if (family == PBBI_GLM_SOFTMAX)
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, std::string("a softmax handle has no observation weights: ") + GLM_POWER_RULE);
    if (!has_streams)
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, std::string("a handle of pbbi_potential_create_glm has no observation streams: ") +
                                                   GLM_POWER_RULE);
    if (!beta_on_device && !(std::isfinite(beta) && beta > 0.0))
        return pbbi_fail(PBBI_ERR_INVALID, "the likelihood power must be finite and > 0 (beta = " + std::to_string(beta) +
                                               "); a power read from the device is not checked");
    return PBBI_OK;
}

// ---- K-class softmax regression ---------------------------------------------------------------------------------
const char* const GLM_SOFTMAX_RULE = "softmax GLM: float64, 2 <= K <= 8 classes, each padded to Dc = 16, 32 or 64 rows with "
                                     "K * Dc <= 128 (D <= 16 for K <= 8, D <= 32 for K <= 4, D <= 64 for K = 2)";

// The padded class size and the tile count of a (D, K) model, and the external row of each of the NT * 16 internal
// rows (-1 = padding).
int glm_softmax_layout(int D, int K, int* Dc_out, int* NT_out, int32_t* row_map) {
    if (D < 1 || K < 2 || K > 8 || D > 64) return pbbi_fail(PBBI_ERR_UNSUPPORTED, GLM_SOFTMAX_RULE);
    const int Dc = glm_padded_dim(D);
    if (K * Dc > 128) return pbbi_fail(PBBI_ERR_UNSUPPORTED, GLM_SOFTMAX_RULE);
    if (Dc_out) *Dc_out = Dc;
    if (NT_out) *NT_out = K * Dc / 16;
    if (row_map)
        for (int k = 0; k < K; ++k)
            for (int d = 0; d < Dc; ++d) row_map[k * Dc + d] = d < D ? k * D + d : -1;
    return PBBI_OK;
}

int glm_softmax_check(int D, int K, int64_t M, const double* X, const double* y, const double* lam) {
    if (!X || !y) return pbbi_fail(PBBI_ERR_INVALID, "X / y is NULL");
    if (!lam) return pbbi_fail(PBBI_ERR_INVALID, "prior_precision is NULL");
    if (M < 1) return pbbi_fail(PBBI_ERR_INVALID, "M must be >= 1");
    if (D < 1) return pbbi_fail(PBBI_ERR_INVALID, "D must be >= 1");
    if (K < 2) return pbbi_fail(PBBI_ERR_INVALID, "softmax GLM: at least two classes");
    for (int64_t i = 0; i < M; ++i)
        if (!(std::isfinite(y[i]) && y[i] >= 0.0 && y[i] < (double)K && y[i] == std::floor(y[i])))
            return pbbi_fail(PBBI_ERR_INVALID, "labels must be integers in [0, K) (observation " + std::to_string(i) + ")");
    for (int64_t i = 0; i < M * D; ++i)
        if (!std::isfinite(X[i])) return pbbi_fail(PBBI_ERR_INVALID, "X must be finite (row " + std::to_string(i / D) + ")");
    return glm_check_prior(D, lam, nullptr);
}
