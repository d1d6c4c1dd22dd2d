// glm_sample_dev.h -- the family samplers of the posterior predictive kernel (gfx950): one replicate y_rep ~ p(y | draw) of one
// observation, and the full proper log density of a value under the same draw.  Device side of the section "Predictive
// replicates" of the RNG contract in include/pbbi.h, which defines every sampler to the operation; tests/glm_predictive_ref.py
// restates it in NumPy with SciPy's own distribution functions.  k_glm_pp (kernels_glm_predictive.hip) is the one caller.
//
// Counters: the block of (draw t, observation i, index b) is rng_block(seed, PBBI_STREAM_PREDICTIVE, iter = t, chain = i, b),
// so a replicate depends on (seed, t, i) alone.  Every sampler is exact: inversion of one uniform for the discrete families
// (over the support enumerated from the mode outwards, O(sigma) steps), Box-Muller for the Gaussian, Marsaglia-Tsang for the
// Gamma.  A non-finite linear predictor or mean gives NaN; so does a discrete distribution whose variance is above
// GLM_PP_MAX_VAR = 2^20 (the enumeration would keep a lane, and with it its wave, busy for thousands of steps per value).
#pragma once
#include "glm_draws_dev.h"
#include "pbbi_rng.h"

constexpr uint32_t GLM_STREAM_PREDICTIVE = 6u;  // PBBI_STREAM_PREDICTIVE
constexpr double GLM_PP_MAX_VAR = 1048576.0;    // 2^20
constexpr int GLM_PP_GAMMA_TRIES = 64;
constexpr int GLM_PP_MAX_STEPS = 1 << 20;

struct GlmPpKey { uint64_t seed, t, i; };

// the uniform of a block: ((x1:x0 >> 11) + 0.5) 2^-53, never 0 (1 only where the sum rounds up from 2^53 - 1/2)
__device__ __forceinline__ double glm_pp_uniform(const GlmPpKey& k, uint32_t blk) {
    const PhiloxOut x = rng_block(k.seed, GLM_STREAM_PREDICTIVE, k.t, k.i, blk);
    const uint64_t w = ((uint64_t)x.x1 << 32) | x.x0;
    return ((double)(w >> 11) + 0.5) * 0x1.0p-53;
}
// the first normal of box_muller_f64 on a block
__device__ __forceinline__ double glm_pp_normal(const GlmPpKey& k, uint32_t blk) {
    double zc, zs;
    box_muller_f64(rng_block(k.seed, GLM_STREAM_PREDICTIVE, k.t, k.i, blk), zc, zs);
    return zc;
}

// Inversion over the integers lo = 0 .. hi from the mode m (mass f_m > 0 there): m, m+1, m-1, m+2, m-2, ..., points outside
// the support skipped; the first point at which the accumulated mass reaches u.  up(k) = f(k+1) / f(k), dn(k) = f(k-1) / f(k).
// Ends when the terms on both sides are 0 (or past the support) with the last point visited that had positive mass.
template <class Up, class Dn>
__device__ __forceinline__ double glm_pp_invert(double u, double m, double f_m, double hi, Up&& up, Dn&& dn) {
    double cum = f_m, last = m;
    if (cum >= u) return m;
    double ku = m, kd = m, fu = f_m, fd = f_m;
    // GLM_PP_MAX_STEPS rounds: a thousand standard deviations at the variance cap; only a negative binomial of tiny shape, whose
    // tail falls off like 1 / k, can get there (probability ~ shape), and gives NaN
    for (int round = 0; round < GLM_PP_MAX_STEPS; ++round) {
        bool any = false;
        if (ku < hi && fu > 0.0) {
            fu *= up(ku);
            ku += 1.0;
            if (fu > 0.0) {
                cum += fu; last = ku; any = true;
                if (cum >= u) return ku;
            }
        }
        if (kd > 0.0 && fd > 0.0) {
            fd *= dn(kd);
            kd -= 1.0;
            if (fd > 0.0) {
                cum += fd; last = kd; any = true;
                if (cum >= u) return kd;
            }
        }
        if (!any) return last;
    }
    return __builtin_nan("");
}

// what the samplers form once per draw beside GlmDrawChain: the Gaussian's sigma, the Gamma's d and c
struct GlmPpChain { double sig, d, c; };
template <int FAM>
__device__ __forceinline__ GlmPpChain glm_pp_chain([[maybe_unused]] const GlmDrawChain<FAM>& dk) {
    GlmPpChain k{0.0, 0.0, 0.0};
    if constexpr (FAM == PBBI_GLM_GAUSSIAN) k.sig = exp(dk.theta);
    if constexpr (FAM == PBBI_GLM_GAMMA) {
        k.d = dk.a < 1.0 ? dk.a + 2.0 / 3.0 : dk.a - 1.0 / 3.0;
        k.c = 1.0 / sqrt(9.0 * k.d);
    }
    return k;
}

// One replicate of observation i at draw t: eta includes the offset, nv the binomial trials, av the weight (read by the
// Gaussian alone, as a precision weight).
template <int FAM>
__device__ __forceinline__ double glm_pp_sample(const GlmPpKey& key, double eta, double nv, double av,
                                                [[maybe_unused]] const GlmDrawChain<FAM>& dk,
                                                [[maybe_unused]] const GlmPpChain& pk) {
    const double nan = __builtin_nan("");
    if (!(fabs(eta) <= 1.7976931348623157e308)) return nan;  // +-inf, NaN
    if constexpr (FAM == PBBI_GLM_GAUSSIAN) {
        return eta + pk.sig / sqrt(av) * glm_pp_normal(key, 0u);
    } else if constexpr (FAM == PBBI_GLM_POISSON) {
        const double mu = exp(eta);
        if (!(mu <= GLM_PP_MAX_VAR)) return nan;
        const double u = glm_pp_uniform(key, 0u);
        const double m = floor(mu);
        const double f_m = exp((m * eta - mu) - glm_lgamma(m + 1.0));
        return glm_pp_invert(u, m, f_m, 0x1.0p62, [&](double k) { return mu / (k + 1.0); }, [&](double k) { return k / mu; });
    } else if constexpr (FAM == PBBI_GLM_LOGISTIC) {
        const double p = glm_mean<PBBI_GLM_LOGISTIC>(eta);
        const double u = glm_pp_uniform(key, 0u);
        if (nv == 1.0) return u < p ? 1.0 : 0.0;
        const double e = exp(-fabs(eta));
        const double q1 = 1.0 / (1.0 + e);                         // max(p, 1 - p)
        if (!(nv * (p * (eta >= 0.0 ? e * q1 : q1)) <= GLM_PP_MAX_VAR)) return nan;
        double m = floor((nv + 1.0) * p);
        m = m > nv ? nv : m;
        const double spl = log1p(e);                               // log p = min(eta, 0) - spl, log(1 - p) = -max(eta, 0) - spl
        const double lp = (eta < 0.0 ? eta : 0.0) - spl, lq = -(eta > 0.0 ? eta : 0.0) - spl;
        const double f_m = exp(((glm_lgamma(nv + 1.0) - glm_lgamma(m + 1.0)) - glm_lgamma((nv - m) + 1.0)) + (m * lp + (nv - m) * lq));
        const double r = exp(eta);                                 // the odds p / (1 - p)
        return glm_pp_invert(u, m, f_m, nv, [&](double k) { return ((nv - k) * r) / (k + 1.0); },
                             [&](double k) { return k / (((nv - k) + 1.0) * r); });
    } else if constexpr (FAM == PBBI_GLM_NEGBINOMIAL) {
        const double mu = exp(eta), phi = dk.a;
        if (!(mu + mu * (mu / phi) <= GLM_PP_MAX_VAR) || !(phi > 0.0)) return nan;
        const double u = glm_pp_uniform(key, 0u);
        double m = floor(((phi - 1.0) * mu) / phi);
        m = m > 0.0 ? m : 0.0;
        const double z = eta - dk.theta;
        const double spl = log1p(exp(-fabs(z)));
        const double lp = -(z > 0.0 ? z : 0.0) - spl, lq = (z < 0.0 ? z : 0.0) - spl;  // log p, log(1 - p): p = phi / (phi + mu)
        const double q = mu / (mu + phi);
        const double f_m = exp(((glm_lgamma(m + phi) - dk.c) - glm_lgamma(m + 1.0)) + (phi * lp + m * lq));
        return glm_pp_invert(u, m, f_m, 0x1.0p62, [&](double k) { return ((k + phi) * q) / (k + 1.0); },
                             [&](double k) { return k / (((k - 1.0) + phi) * q); });
    } else if constexpr (FAM == PBBI_GLM_ORDINAL) {
        const double u = glm_pp_uniform(key, 0u);
        double y = dk.km1;
#pragma unroll
        for (int j = 6; j >= 0; --j) {  // the first category whose cumulative probability sigma(kappa_{j+1} - eta) reaches u
            const double a = dk.kap[j] - eta;
            const double e = exp(-fabs(a));
            const double inv = 1.0 / (1.0 + e);
            const double cdf = a >= 0.0 ? inv : e * inv;
            y = ((double)j < dk.km1 && cdf >= u) ? (double)j : y;
        }
        return (dk.kap[0] == dk.kap[0] && dk.kap[6] == dk.kap[6]) ? y : nan;  // kap accumulates: a NaN cutpoint reaches kap[6]
    } else {
        static_assert(FAM == PBBI_GLM_GAMMA, "a family of glm_draw_dispatch");
        const double alpha = dk.a, mu = exp(eta);
        if (!(mu <= 1.7976931348623157e308) || !(alpha > 0.0) || !(alpha <= 1.7976931348623157e308)) return nan;
        double y = nan;
        for (int j = 0; j < GLM_PP_GAMMA_TRIES; ++j) {
            const double zn = glm_pp_normal(key, 2u * (uint32_t)j);
            const double t = 1.0 + pk.c * zn;
            const double v = t * t * t;
            if (!(v > 0.0)) continue;
            const double uu = glm_pp_uniform(key, 2u * (uint32_t)j + 1u);
            if (log(uu) < ((0.5 * (zn * zn) + pk.d) - pk.d * v) + pk.d * log(v)) {
                y = ((pk.d * v) * mu) / alpha;
                break;
            }
        }
        if (alpha < 1.0) y *= exp(log(glm_pp_uniform(key, 0x80000000u)) / alpha);
        return y;
    }
}

// log f(y | draw) of one value: minus the energy term of glm_draw_uterm at unit weight, plus the term that depends on no
// parameter, which the samplers of k_glm drop (log C(n, y); -lgamma(y + 1); the Gaussian constant; -log y).  Unweighted, except
// for the Gaussian family, whose weight is a precision weight: N(eta, sigma^2 / a).  (a - 1) theta and log a are an exact 0 at a = 1.
template <int FAM>
__device__ __forceinline__ double glm_pp_logpdf(double yv, double eta, double nv, double av, const GlmDrawChain<FAM>& dk) {
    if constexpr (FAM == PBBI_GLM_LOGISTIC) {
        const double lc = (glm_lgamma(nv + 1.0) - glm_lgamma(yv + 1.0)) - glm_lgamma((nv - yv) + 1.0);
        return lc - glm_draw_uterm<FAM>(eta, nv, yv, dk);
    } else if constexpr (FAM == PBBI_GLM_POISSON) {
        return -glm_draw_uterm<FAM>(eta, 1.0, yv, dk) - glm_lgamma(yv + 1.0);
    } else if constexpr (FAM == PBBI_GLM_GAUSSIAN) {
        return ((av - 1.0) * dk.theta + 0.5 * log(av)) - glm_draw_uterm<FAM>(eta, av, yv, dk) - 0.91893853320467274178;
    } else if constexpr (FAM == PBBI_GLM_NEGBINOMIAL) {
        return -glm_draw_uterm<FAM>(eta, 1.0, yv, dk) - glm_lgamma(yv + 1.0);
    } else if constexpr (FAM == PBBI_GLM_GAMMA) {
        const double ly = log(yv);
        return -glm_draw_uterm<FAM>(eta, 1.0, ly, dk) - ly;
    } else {
        return -glm_draw_uterm<FAM>(eta, 1.0, yv, dk);
    }
}
