// glm_family_dev.h -- the family arithmetic of the GLM kernels (gfx950), stated once: the per-observation energy term U_i of
// each family with its derivatives, psi and log Gamma, what a dispersion family forms once per chain, the fitted mean and the
// rule that selects a row of weight 0 out; the ordinal family's cutpoints, link and expected category.  k_glm (kernels_glm.hip, kernels_glm_metric.hip) takes U_i, dU_i/deta and
// dU_i/dtheta; the kernels that take draws (k_glm_pw, k_glm_ll; glm_draws_dev.h) call the same functions with want_u and keep
// U_i alone -- the compiler drops the derivatives they do not read, and -ffp-contract=off keeps what is left operation for
// operation, so the three kernels agree on U_i bit for bit by construction.  glm_disp() and glm_canonical() are glm_host.h's.
#pragma once
#include "pbbi_internal.h"

// b(eta) - y eta and b'(eta) - y of one observation
template <int FAM>
__device__ __forceinline__ void glm_link(double eta, double yv, bool want_u, double& resid, double& uterm) {
    if constexpr (FAM == PBBI_GLM_LOGISTIC) {
        const double e = exp(-fabs(eta));
        const double inv = 1.0 / (1.0 + e);
        resid = (eta >= 0.0 ? inv : e * inv) - yv;
        uterm = 0.0;
        if (want_u) uterm = ((eta > 0.0 ? eta : 0.0) + log1p(e)) - yv * eta;
    } else {
        const double e = exp(eta);
        resid = e - yv;
        uterm = e - yv * eta;
    }
}

// the full model's c b(eta) - d eta and c b'(eta) - d
template <int FAM>
__device__ __forceinline__ void glm_link_rich(double eta, double cv, double dv, bool want_u, double& resid,
                                              double& uterm) {
    if constexpr (FAM == PBBI_GLM_LOGISTIC) {
        const double e = exp(-fabs(eta));
        const double inv = 1.0 / (1.0 + e);
        resid = cv * (eta >= 0.0 ? inv : e * inv) - dv;
        uterm = 0.0;
        if (want_u) uterm = cv * ((eta > 0.0 ? eta : 0.0) + log1p(e)) - dv * eta;
    } else {
        const double e = exp(eta);
        resid = cv * e - dv;
        uterm = cv * e - dv * eta;
    }
}

// psi and log Gamma for x > 0: the recurrences psi(x) = psi(x + 1) - 1/x and lgamma(x) = lgamma(x + 1) - log x, two steps
// at a time (one division per pair, at most three pairs), up to an argument >= 6, then the asymptotic series: psi
// through x^-14 (the first term left out is 3617 / (8160 x^16): 1.6e-13 at 6), Stirling's through x^-13 (3617 / (122400
// x^15): 6e-14 at 6).  The library's lgamma, inlined once per accumulator register, costs these kernels their registers.
__device__ __forceinline__ double glm_psi(double x) {
    double acc = 0.0;
    while (x < 6.0) {
        acc -= (2.0 * x + 1.0) / (x * (x + 1.0));  // 1/x + 1/(x + 1)
        x += 2.0;
    }
    const double r = 1.0 / x, r2 = r * r;
    const double tail = r2 * (1.0 / 12 - r2 * (1.0 / 120 - r2 * (1.0 / 252 - r2 * (1.0 / 240 - r2 * (1.0 / 132 -
                        r2 * (691.0 / 32760 - r2 * (1.0 / 12)))))));
    return acc + ((log(x) - 0.5 * r) - tail);
}
__device__ __forceinline__ double glm_lgamma(double x) {
    double prod = 1.0;
    while (x < 6.0) {
        prod *= x * (x + 1.0);
        x += 2.0;
    }
    const double r = 1.0 / x, r2 = r * r;
    const double tail = r * (1.0 / 12 - r2 * (1.0 / 360 - r2 * (1.0 / 1260 - r2 * (1.0 / 1680 - r2 * (1.0 / 1188 -
                        r2 * (691.0 / 360360 - r2 * (1.0 / 156)))))));
    return ((((x - 0.5) * log(x) - x) + 0.91893853320467274178) + tail) - log(prod);
}

// what a dispersion family forms once per chain and gradient evaluation
//   gaussian:     a = tau = exp(-2 theta)
//   negbinomial:  a = phi = exp(theta), b = psi(phi), c = lgamma(phi) (an evaluation that wants U only)
//   gamma:        a = alpha = exp(theta), b = psi(alpha) - theta - 1, c = lgamma(alpha) - alpha theta (wants U only)
struct GlmDispChain { double theta, a, b, c; };

template <int FAM>
__device__ __forceinline__ GlmDispChain glm_disp_chain(double theta, bool want_u) {
    GlmDispChain k{theta, 0.0, 0.0, 0.0};
    if constexpr (FAM == PBBI_GLM_GAUSSIAN) {
        k.a = exp(-2.0 * theta);
    } else if constexpr (FAM == PBBI_GLM_GAMMA) {
        k.a = exp(theta);
        k.b = (glm_psi(k.a) - theta) - 1.0;
        if (want_u) k.c = glm_lgamma(k.a) - k.a * theta;
    } else {
        static_assert(FAM == PBBI_GLM_NEGBINOMIAL, "a dispersion family");
        k.a = exp(theta);
        k.b = glm_psi(k.a);
        if (want_u) k.c = glm_lgamma(k.a);
    }
    return k;
}

// the dispersion families' U_i, dU_i/deta and dU_i/dtheta (cv = a_i, yv = y_i; gamma: yv = log y_i, the stream its packer writes)
template <int FAM>
__device__ __forceinline__ void glm_link_disp(double eta, double cv, double yv, const GlmDispChain& k, bool want_u,
                                              double& resid, double& uterm, double& tterm) {
    if constexpr (FAM == PBBI_GLM_GAUSSIAN) {
        const double r = yv - eta;
        const double tr = k.a * r;
        const double trr = tr * r;  // tau (y - eta)^2
        resid = -(cv * tr);
        tterm = cv * (1.0 - trr);
        uterm = cv * (0.5 * trr + k.theta);
    } else if constexpr (FAM == PBBI_GLM_GAMMA) {
        // z = eta - log y: U_i = a [lgamma(alpha) - alpha theta + alpha (z + exp(-z))], one exp per observation.  An exp(-z) that
        // overflows makes the chain's energy inf / NaN and the proposal is rejected, as for Poisson's exp(eta).
        const double z = eta - yv;
        const double e = exp(-z);
        const double ze = z + e;
        resid = cv * (k.a * (1.0 - e));
        tterm = cv * (k.a * (k.b + ze));
        uterm = cv * (k.c + k.a * ze);
    } else {
        static_assert(FAM == PBBI_GLM_NEGBINOMIAL, "a dispersion family");
        // z = eta - theta: s = sigmoid(z), sp = softplus(z); logaddexp(eta, theta) = theta + sp, so
        // -phi theta - y eta + (y + phi) logaddexp = (y + phi) sp - y z
        const double z = eta - k.theta;
        const double e = exp(-fabs(z));
        const double ope = 1.0 + e;  // in [1, 2]: log(ope) is log1p(e) to 1.2e-16 ABSOLUTE, which is what sp needs, and
        const double inv = 1.0 / ope;  // keeps these kernels to one logarithm's constants
        const double s = z >= 0.0 ? inv : e * inv;
        const double s1 = z >= 0.0 ? e * inv : inv;  // 1 - s
        const double sp = (z > 0.0 ? z : 0.0) + log(ope);
        const double yp = yv + k.a;
        resid = cv * (yp * s - yv);
        tterm = cv * (k.a * (((k.b - glm_psi(yp)) + sp) - s) + yv * s1);
        uterm = 0.0;
        if (want_u) uterm = cv * (((k.c - glm_lgamma(yp)) + yp * sp) - yv * z);
    }
}

// ---- second derivatives: what k_glm_hess (kernels_glm_hessian.hip) takes.  New functions beside the ones above, which they do
// not call: k_glm, k_glm_pw and k_glm_ll read none of these.
//
// psi'(x) for x > 0, in the style of glm_psi: the recurrence psi'(x) = psi'(x + 1) + 1/x^2, two steps at a time (one division
// per pair), then the asymptotic series 1/x + 1/(2x^2) + sum B_2k / x^(2k+1) through x^-15.  The first term left out is
// 3617 / (510 x^17): 4.2e-13 at 6, 7.1e-17 at 10.  The Hessian takes psi' in differences (psi'(phi) - psi'(y + phi)) whose size
// is far below either term, so the recurrence runs up to an argument >= 10 (>= 6 would leave 2e-12 of the term); at most five
// pairs.  glm_psi_far is psi by the same recurrence to >= 10 (first term left out of glm_psi's series: 3617 / (8160 x^16),
// 4.4e-17 at 10), for the same reason: dU/dtheta's own psi difference is differentiated here.
__device__ __forceinline__ double glm_trigamma(double x) {
    double acc = 0.0;
    while (x < 10.0) {
        const double x1 = x + 1.0, den = x * x1;
        acc += (x * x + x1 * x1) / (den * den);  // 1/x^2 + 1/(x + 1)^2
        x += 2.0;
    }
    const double r = 1.0 / x, r2 = r * r;
    const double tail = r2 * (1.0 / 6 - r2 * (1.0 / 30 - r2 * (1.0 / 42 - r2 * (1.0 / 30 - r2 * (5.0 / 66 -
                        r2 * (691.0 / 2730 - r2 * (7.0 / 6)))))));
    return acc + (r + r2 * 0.5 + r * tail);
}
__device__ __forceinline__ double glm_psi_far(double x) {
    double acc = 0.0;
    while (x < 10.0) {
        acc -= (2.0 * x + 1.0) / (x * (x + 1.0));
        x += 2.0;
    }
    const double r = 1.0 / x, r2 = r * r;
    const double tail = r2 * (1.0 / 12 - r2 * (1.0 / 120 - r2 * (1.0 / 252 - r2 * (1.0 / 240 - r2 * (1.0 / 132 -
                        r2 * (691.0 / 32760 - r2 * (1.0 / 12)))))));
    return acc + ((log(x) - 0.5 * r) - tail);
}

// h = d2U_i/deta2 of the canonical families (cv = a_i n_i): c sigma (1 - sigma), c exp(eta)
template <int FAM>
__device__ __forceinline__ double glm_hess_rich(double eta, double cv) {
    if constexpr (FAM == PBBI_GLM_LOGISTIC) {
        const double e = exp(-fabs(eta));
        const double inv = 1.0 / (1.0 + e);
        return cv * ((e * inv) * inv);
    } else {
        return cv * exp(eta);
    }
}

// what a dispersion family's second derivatives form once per evaluation
//   gaussian:     a = tau = exp(-2 theta)
//   negbinomial:  a = phi = exp(theta), b = psi(phi), c = phi psi'(phi)
//   gamma:        a = alpha = exp(theta), b = (psi(alpha) - theta - 1) + (alpha psi'(alpha) - 1)
template <int FAM>
__device__ __forceinline__ GlmDispChain glm_hess_chain(double theta) {
    GlmDispChain k{theta, 0.0, 0.0, 0.0};
    if constexpr (FAM == PBBI_GLM_GAUSSIAN) {
        k.a = exp(-2.0 * theta);
    } else if constexpr (FAM == PBBI_GLM_GAMMA) {
        k.a = exp(theta);
        k.b = ((glm_psi_far(k.a) - theta) - 1.0) + (k.a * glm_trigamma(k.a) - 1.0);
    } else {
        static_assert(FAM == PBBI_GLM_NEGBINOMIAL, "a dispersion family");
        k.a = exp(theta);
        k.b = glm_psi_far(k.a);
        k.c = k.a * glm_trigamma(k.a);
    }
    return k;
}

// the dispersion families' h = d2U_i/deta2, kx = d2U_i/deta dtheta and tt = d2U_i/dtheta2 (cv = a_i, yv = y_i; gamma: log y_i)
//   gaussian     e = y - eta:  h = a tau,  kx = 2 a tau e,  tt = 2 a tau e^2
//   negbinomial  s = sigma(eta - theta), sp = softplus(eta - theta), yp = y + phi:
//                h = a yp s (1 - s),  kx = a [phi s - yp s (1 - s)],
//                tt = a { phi [psi(phi) - psi(yp) + sp - s] + phi [phi psi'(phi) - phi psi'(yp)] - phi s^2 + y s (1 - s) }
//   gamma        z = eta - log y:  h = a alpha exp(-z),  kx = a alpha (1 - exp(-z)),
//                tt = a alpha [ (psi(alpha) - theta - 1 + z + exp(-z)) + alpha psi'(alpha) - 1 ]
template <int FAM>
__device__ __forceinline__ void glm_hess_disp(double eta, double cv, double yv, const GlmDispChain& k, double& h, double& kx,
                                              double& tt) {
    if constexpr (FAM == PBBI_GLM_GAUSSIAN) {
        const double r = yv - eta;
        const double tr = k.a * r;
        h = cv * k.a;
        kx = cv * (2.0 * tr);
        tt = cv * (2.0 * (tr * r));
    } else if constexpr (FAM == PBBI_GLM_GAMMA) {
        const double z = eta - yv;
        const double e = exp(-z);
        h = cv * (k.a * e);
        kx = cv * (k.a * (1.0 - e));
        tt = cv * (k.a * (k.b + (z + e)));
    } else {
        static_assert(FAM == PBBI_GLM_NEGBINOMIAL, "a dispersion family");
        const double z = eta - k.theta;
        const double e = exp(-fabs(z));
        const double ope = 1.0 + e;
        const double inv = 1.0 / ope;
        const double s = z >= 0.0 ? inv : e * inv;
        const double ss1 = (e * inv) * inv;  // s (1 - s)
        const double sp = (z > 0.0 ? z : 0.0) + log(ope);
        const double yp = yv + k.a;
        h = cv * (yp * ss1);
        kx = cv * (k.a * s - yp * ss1);
        tt = cv * (((k.a * (((k.b - glm_psi_far(yp)) + sp) - s) + k.a * (k.c - k.a * glm_trigamma(yp))) - k.a * (s * s)) +
                   yv * ss1);
    }
}

// ---- ordinal (cumulative-logit) regression: K ordered categories, cutpoints kappa_1 < .. < kappa_{K-1} carried by the chain as
// zeta_1 = kappa_1, zeta_m = log(kappa_m - kappa_{m-1}) (include/pbbi.h has the model).  What a chain forms once per gradient
// evaluation from its K - 1 zeta rows z[0 .. K-2] (z[j] = zeta_{j+1}; entries past K - 1 are not read), before the likelihood walk:
//   kap[j] = kappa_{j+1};  G[m] = -log(1 - exp(-Delta_m)) = -log(-expm1(-Delta_m)) of the interior category m, 1 <= m <= K - 2,
//   whose width is Delta_m = exp(z[m]) (an evaluation that wants U only)
// and after it, where the cutpoints' gradient is assembled (glm_ord_widths: held across the walk they would cost its registers):
//   gap[m] = Delta_m;  iem[m] = 1 / expm1(Delta_m)
// Entries past the model's are SELECTED to finite constants (kap: the last cutpoint again; gap 1; iem, G 0), never multiplied
// out, so a padding row's content reaches nothing.  km1 = K - 1, as the double the category stream is compared with.
struct GlmOrdChain { double kap[7], G[7], km1; };
struct GlmOrdAcc { double c[7]; };  // this lane's share of sum_i dU_i/dkappa_{j+1}, j = 0 .. 6

__device__ __forceinline__ GlmOrdChain glm_ord_chain(const double (&z)[7], int K, bool want_u) {
    GlmOrdChain k;
    k.km1 = (double)(K - 1);
    k.kap[0] = z[0];
    k.G[0] = 0.0;
#pragma unroll
    for (int m = 1; m < 7; ++m) {
        const bool in = m < K - 1;  // wave-uniform
        const double d = in ? exp(z[m]) : 1.0;
        k.kap[m] = in ? k.kap[m - 1] + d : k.kap[m - 1];
        k.G[m] = 0.0;
        if (want_u) k.G[m] = in ? -log(-expm1(-d)) : 0.0;
    }
    return k;
}
__device__ __forceinline__ void glm_ord_widths(const double (&z)[7], int K, double (&gap)[7], double (&iem)[7]) {
    gap[0] = 1.0;
    iem[0] = 0.0;
#pragma unroll
    for (int m = 1; m < 7; ++m) {
        const bool in = m < K - 1;
        gap[m] = in ? exp(z[m]) : 1.0;
        iem[m] = in ? 1.0 / expm1(gap[m]) : 0.0;
    }
}

// U_i, dU_i/deta and the two sigmoid terms of one observation of category yv (cv = a_i):
//   U_i = a [ sp(eta - kappa_{k+1}) + sp(kappa_k - eta) + G_k ],  s_hi = sigma(eta - kappa_{k+1}),  s_lo = sigma(kappa_k - eta)
// the term of an infinite cutpoint absent (k = 0: no s_lo; k = K - 1: no s_hi).  The observation's two cutpoints are selected
// out of the chain's by the category; two exp per observation, two log more where U is wanted.
// t_hi = a s_hi is what dU/dkappa_{k+1} loses, t_lo = a s_lo what dU/dkappa_k gains.
__device__ __forceinline__ void glm_link_ord(double eta, double cv, double yv, const GlmOrdChain& k, bool want_u, double& resid,
                                             double& uterm, double& t_hi, double& t_lo) {
    double khi = k.kap[0], klo = k.kap[0];
#pragma unroll
    for (int j = 1; j < 7; ++j) {
        khi = (yv == (double)j) ? k.kap[j] : khi;        // kappa_{k+1} of category j is kap[j]
        klo = (yv == (double)(j + 1)) ? k.kap[j] : klo;  // kappa_k of category j + 1 is kap[j]
    }
    const bool has_hi = yv < k.km1, has_lo = yv > 0.0;
    const double a = eta - khi, b = klo - eta;
    const double ea = exp(-fabs(a)), eb = exp(-fabs(b));
    const double oa = 1.0 + ea, ob = 1.0 + eb;  // in [1, 2]: log(oa) is log1p(ea) to 1.2e-16 ABSOLUTE, which is what sp needs (as
    const double ia = 1.0 / oa, ib = 1.0 / ob;  // for the negative binomial), and keeps these kernels to one logarithm's constants
    const double s_hi = has_hi ? (a >= 0.0 ? ia : ea * ia) : 0.0;
    const double s_lo = has_lo ? (b >= 0.0 ? ib : eb * ib) : 0.0;
    t_hi = cv * s_hi;
    t_lo = cv * s_lo;
    resid = cv * (s_hi - s_lo);
    uterm = 0.0;
    if (want_u) {
        double Gk = 0.0;
#pragma unroll
        for (int j = 1; j < 7; ++j) Gk = (yv == (double)j) ? k.G[j] : Gk;
        const double sp_hi = has_hi ? (a > 0.0 ? a : 0.0) + log(oa) : 0.0;
        const double sp_lo = has_lo ? (b > 0.0 ? b : 0.0) + log(ob) : 0.0;
        uterm = cv * ((sp_hi + sp_lo) + Gk);
    }
}

// the ordinal family's fitted mean: the expected category sum_{j = 1 .. K-1} P(y >= j) = sum_j sigma(eta - kappa_j)
__device__ __forceinline__ double glm_mean_ord(double eta, const GlmOrdChain& k) {
    double m = 0.0;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const double a = eta - k.kap[j];
        const double e = exp(-fabs(a));
        const double inv = 1.0 / (1.0 + e);
        m += ((double)j < k.km1) ? (a >= 0.0 ? inv : e * inv) : 0.0;
    }
    return m;
}

// the fitted mean of one observation: the sigmoid as glm_link_rich forms it, eta (gaussian), exp(eta) (every log link:
// poisson, negbinomial, gamma)
template <int FAM>
__device__ __forceinline__ double glm_mean(double eta) {
    if constexpr (FAM == PBBI_GLM_LOGISTIC) {
        const double e = exp(-fabs(eta));
        const double inv = 1.0 / (1.0 + e);
        return eta >= 0.0 ? inv : e * inv;
    } else if constexpr (FAM == PBBI_GLM_GAUSSIAN) {
        return eta;
    } else {
        return exp(eta);
    }
}

// Does the row have weight?  A row without adds exactly nothing, whatever b() gave: its terms are SELECTED out, not multiplied
// (0 * inf is NaN).  The streams are c = a n, d = a y (canonical families) and c = a, d = y (dispersion families; gamma: d = log y; ordinal: d = the category).
template <int FAM>
__device__ __forceinline__ bool glm_row_on(double cv, double dv) {
    if constexpr (glm_disp(FAM) || FAM == PBBI_GLM_ORDINAL) return cv != 0.0;
    else return !(cv == 0.0 && dv == 0.0);
}
