// glm_asan_driver.cpp -- glm_host.cpp under AddressSanitizer + UndefinedBehaviorSanitizer (test infrastructure, CPU only).
// The packers and checkers compute indices into buffers the caller sized: every one of them is driven here over heap buffers
// of EXACTLY the documented length (one element more or less is a report), at the dimensions where the padding changes (D = 1,
// 16, 17, 64, 65, 128 as far as each function's rule allows; M = 1, 16, 65; J = 1 and 4; a sampled and a held dispersion; the
// softmax shapes (1, 2), (16, 8), (17, 4), (64, 2); a penalty on a group of one and on the largest group there is).  Built
// together with glm_host.cpp by `make asan_check`; prints "asan ok" and exits 0 when the sanitizers stayed silent (they abort
// the process otherwise) and every call returned what its arguments deserve.  tests/test_glm_host_asan.py runs it.
#include <cmath>
#include <cstdio>
#include <memory>

#include "glm_host.h"

static std::string g_error;
int pbbi_fail(int code, const std::string& msg) {
    g_error = msg;
    return code;
}

template <class T>
using Buf = std::unique_ptr<T[]>;
static Buf<double> dbuf(int64_t n, double fill, double step = 0.0) {  // exactly n elements (n = 0: a valid empty block)
    Buf<double> p(new double[(size_t)n]);
    for (int64_t i = 0; i < n; ++i) p[(size_t)i] = fill + step * (double)(i % 7);
    return p;
}

static int bad = 0;
#define EXPECT(cond)                                                                  \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::printf("line %d: %s failed (%s)\n", __LINE__, #cond, g_error.c_str()); \
            ++bad;                                                                    \
        }                                                                             \
    } while (0)

static const int DS[] = {1, 16, 17, 64, 65, 128};
static const int64_t MS[] = {1, 16, 65};

static void design_and_observations() {
    for (int D : DS)
        for (int64_t M : MS) {
            Buf<double> X = dbuf(M * D, 0.25, 0.5);
            EXPECT(glm_check_design(D, M, X.get()) == PBBI_OK);
            EXPECT(glm_image_len(D, M) == glm_blocks_padded(M) * glm_padded_dim(D) * 32);
            Buf<double> img = dbuf(glm_image_len(D, M), -1.0);
            glm_pack(D, M, X.get(), img.get());
            EXPECT(img[0] == X[0]);  // P1[0][0][0] = X[0][0]
            // [X | 0] at every padded dimension that holds D (the hierarchical and dispersion handles' images)
            for (int DP = glm_padded_dim(D); DP <= 128; DP *= 2) {
                Buf<double> wide = dbuf(glm_blocks_padded(M) * DP * 32, -1.0);
                glm_pack_dp(D, DP, M, X.get(), wide.get());
                EXPECT(wide[0] == X[0]);
            }
        }
    for (int64_t M : MS) {
        Buf<double> y = dbuf(M, 1.0), w = dbuf(M, 0.5, 0.25), o = dbuf(M, -0.5, 0.125), n = dbuf(M, 2.0);
        Buf<double> out = dbuf(glm_obs_len(M), -1.0);
        for (int opt = 0; opt < 2; ++opt) {  // every optional argument given, every one NULL
            const double *wp = opt ? w.get() : nullptr, *op = opt ? o.get() : nullptr, *np = opt ? n.get() : nullptr;
            EXPECT(glm_check_obs(M, PBBI_GLM_LOGISTIC, y.get(), wp, op, np) == PBBI_OK);
            EXPECT(glm_check_obs(M, PBBI_GLM_POISSON, y.get(), wp, op, nullptr) == PBBI_OK);
            glm_pack_obs(M, y.get(), wp, op, np, out.get());
            EXPECT(out[(size_t)(glm_obs_len(M) / 3 + M - 1)] == (opt ? w[(size_t)(M - 1)] : 1.0));  // d = a y, y = 1
            EXPECT(glm_check_obs_disp(M, PBBI_GLM_GAUSSIAN, y.get(), wp, op) == PBBI_OK);
            EXPECT(glm_check_obs_disp(M, PBBI_GLM_NEGBINOMIAL, y.get(), wp, op) == PBBI_OK);
            glm_pack_obs_disp(M, PBBI_GLM_NEGBINOMIAL, y.get(), wp, op, out.get());
            EXPECT(out[(size_t)(glm_obs_len(M) - 1)] == 0.0);  // the offsets' padding
            EXPECT(out[(size_t)(glm_obs_len(M) / 3 + M - 1)] == 1.0);  // d = y (raw), y = 1
            EXPECT(glm_check_obs_disp(M, PBBI_GLM_GAMMA, y.get(), wp, op) == PBBI_OK);
            glm_pack_obs_disp(M, PBBI_GLM_GAMMA, y.get(), wp, op, out.get());
            EXPECT(out[(size_t)(glm_obs_len(M) / 3 + M - 1)] == 0.0);  // gamma: d = log y, y = 1
            EXPECT(out[(size_t)(glm_obs_len(M) / 3 + M)] == 0.0 && out[(size_t)(glm_obs_len(M) - 1)] == 0.0);  // padding
        }
        y[(size_t)(M - 1)] = 3.0;  // the LAST observation is the one found: above its trials, and no integer for the counts
        EXPECT(glm_check_obs(M, PBBI_GLM_LOGISTIC, y.get(), nullptr, nullptr, n.get()) == PBBI_ERR_INVALID);
        y[(size_t)(M - 1)] = 0.5;
        EXPECT(glm_check_obs_disp(M, PBBI_GLM_NEGBINOMIAL, y.get(), nullptr, nullptr) == PBBI_ERR_INVALID);
        EXPECT(glm_check_obs_disp(M, PBBI_GLM_GAMMA, y.get(), nullptr, nullptr) == PBBI_OK);  // gamma: any y > 0
        for (double v : {0.0, -1.0, (double)NAN, (double)INFINITY}) {  // ... and nothing else; the LAST observation is named
            y[(size_t)(M - 1)] = v;
            EXPECT(glm_check_obs_disp(M, PBBI_GLM_GAMMA, y.get(), nullptr, nullptr) == PBBI_ERR_INVALID);
            EXPECT(g_error.find("(observation " + std::to_string(M - 1) + ")") != std::string::npos);
            EXPECT((g_error.find("gamma: y must be > 0") != std::string::npos) == std::isfinite(v));
        }
        EXPECT(glm_check_obs_disp(M, 7, y.get(), nullptr, nullptr) == PBBI_ERR_INVALID);
        // the ordinal family: categories 0 .. K-1 in turn, exactly-sized streams and the 8 weighted category counts
        for (int K : {2, 5, 8}) {
            Buf<double> cat = dbuf(M, 0.0), counts = dbuf(8, -1.0);
            double want[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int64_t i = 0; i < M; ++i) {
                cat[(size_t)i] = (double)(i % K);
                want[i % K] += w[(size_t)i];
            }
            EXPECT(glm_check_obs_ordinal(M, K, cat.get(), w.get(), o.get()) == PBBI_OK);
            EXPECT(glm_check_obs_ordinal(M, K, cat.get(), nullptr, nullptr) == PBBI_OK);
            glm_pack_obs_ordinal(M, K, cat.get(), w.get(), o.get(), out.get(), counts.get());
            EXPECT(out[0] == w[0] && out[(size_t)(glm_obs_len(M) / 3 + M - 1)] == (double)((M - 1) % K));  // c = a, d = the category
            EXPECT(out[(size_t)(glm_obs_len(M) - 1)] == 0.0);  // the offsets' padding
            for (int k = 0; k < 8; ++k) EXPECT(counts[(size_t)k] == want[k]);  // (same order of additions; 0 past K)
            for (double v : {-1.0, (double)K, 0.5, (double)NAN, (double)INFINITY}) {  // the LAST observation is named
                cat[(size_t)(M - 1)] = v;
                EXPECT(glm_check_obs_ordinal(M, K, cat.get(), nullptr, nullptr) == PBBI_ERR_INVALID);
                EXPECT(g_error.find("integer categories in [0, K) (observation " + std::to_string(M - 1) + ")") != std::string::npos);
            }
            cat[(size_t)(M - 1)] = 0.0;
            w[(size_t)(M - 1)] = -0.5;
            EXPECT(glm_check_obs_ordinal(M, K, cat.get(), w.get(), nullptr) == PBBI_ERR_INVALID);
            EXPECT(g_error.find("weights must be finite and >= 0 (observation " + std::to_string(M - 1) + ")") != std::string::npos);
            w[(size_t)(M - 1)] = 0.5 + 0.25 * (double)(M - 1);
            o[(size_t)(M - 1)] = (double)INFINITY;
            EXPECT(glm_check_obs_ordinal(M, K, cat.get(), nullptr, o.get()) == PBBI_ERR_INVALID);
            o[(size_t)(M - 1)] = 0.0;
        }
        EXPECT(glm_check_obs_ordinal(M, 1, y.get(), nullptr, nullptr) == PBBI_ERR_INVALID);
        EXPECT(glm_check_obs_ordinal(M, 9, y.get(), nullptr, nullptr) == PBBI_ERR_INVALID);
        EXPECT(glm_check_obs_ordinal(M, 3, nullptr, nullptr, nullptr) == PBBI_ERR_INVALID);
    }
    for (int D : DS) {
        Buf<double> lam = dbuf(D, 0.5, 0.5), mu = dbuf(D, -1.0, 0.5);
        EXPECT(glm_check_prior(D, lam.get(), mu.get()) == PBBI_OK);
        EXPECT(glm_check_prior(D, lam.get(), nullptr) == PBBI_OK);
        lam[(size_t)(D - 1)] = -1.0;
        EXPECT(glm_check_prior(D, lam.get(), mu.get()) == PBBI_ERR_INVALID);
    }
}

// groups of a D-coefficient model with J groups: coefficient d in group d % (J + 1) - 1 (so -1, fixed, comes round too) once
// every group has a member; group 0 alone where D < J + 1 leaves no room for that
static Buf<int32_t> groups_of(int D, int J) {
    Buf<int32_t> g(new int32_t[(size_t)D]);
    for (int d = 0; d < D; ++d) g[(size_t)d] = D >= J + 1 ? d % (J + 1) - 1 : d % J;
    return g;
}

static void hierarchical_tables() {
    const int JS[] = {1, 4};
    for (int D : DS)
        for (int J : JS) {
            Buf<double> lam = dbuf(D, 0.5, 0.5), mu = dbuf(D, -1.0, 0.5), tprior = dbuf(2 * J, 0.25, 0.25);
            Buf<int32_t> groups = groups_of(D, J);
            const int rc = glm_check_hier(D, J, lam.get(), mu.get(), groups.get(), tprior.get());
            EXPECT(rc == (D >= J ? PBBI_OK : PBBI_ERR_INVALID));  // fewer coefficients than groups: one is unused
            if (rc != PBBI_OK) continue;
            for (int sample = 0; sample < 2; ++sample) {
                const int Dt = D + J + sample;
                if (Dt > 128) continue;  // the packers' own limit (the entries refuse it before they pack)
                const int DP = glm_padded_dim(Dt);
                Buf<double> dprior = dbuf(2, 0.5), nj = dbuf(J, -1.0);
                EXPECT(glm_check_hier_disp_theta(sample, 0.25, sample ? dprior.get() : nullptr) == PBBI_OK);
                EXPECT(glm_check_hier_disp_theta(sample, 0.25, sample ? nullptr : dprior.get()) == PBBI_ERR_INVALID);
                Buf<double> tab = dbuf(2 * DP, -7.0);
                glm_pack_prior_groups_disp(D, J, lam.get(), mu.get(), groups.get(), tprior.get(), sample, dprior.get(), tab.get(),
                                           nj.get());
                EXPECT(tab[(size_t)(D + J - 1)] == tprior[(size_t)(2 * J - 1)]);         // lam of t_{J-1}
                EXPECT(tab[(size_t)(DP + D + J - 1)] == tprior[(size_t)(2 * J - 2)]);    // its mean
                if (sample) EXPECT(tab[(size_t)(D + J)] == dprior[1] && tab[(size_t)(DP + D + J)] == dprior[0]);
                if (!sample) {  // the table of the logistic / poisson handles is the same one without theta
                    Buf<double> plain = dbuf(2 * DP, -7.0);
                    glm_pack_prior_groups(D, J, lam.get(), mu.get(), groups.get(), tprior.get(), plain.get(), nj.get());
                    for (int i = 0; i < 2 * DP; ++i) EXPECT(plain[(size_t)i] == tab[(size_t)i]);
                    double members = 0.0;
                    for (int j = 0; j < J; ++j) members += nj[(size_t)j];
                    EXPECT(members >= (double)J && members <= (double)D);
                }
            }
        }
}

// a first-order random walk (RW1, rank n - 1; [1] for n = 1) on every group's coefficients, zero elsewhere
static Buf<double> rw1_penalty(int D, int J, const int32_t* groups, double* rank) {
    Buf<double> Q = dbuf((int64_t)D * D, 0.0);
    for (int j = 0; j < J; ++j) {
        int prev = -1, n = 0;
        for (int d = 0; d < D; ++d) {
            if (groups[d] != j) continue;
            if (prev >= 0) {
                Q[(size_t)prev * D + prev] += 1.0; Q[(size_t)d * D + d] += 1.0;
                Q[(size_t)prev * D + d] -= 1.0; Q[(size_t)d * D + prev] -= 1.0;
            }
            prev = d; ++n;
        }
        if (n == 1) Q[(size_t)prev * D + prev] = 1.0;
        rank[j] = n == 1 ? 1.0 : (double)(n - 1);
    }
    return Q;
}

static void penalties() {
    // {D, J}: one group of one; 16 and 17 coefficients in 1 and 4 groups; four groups of one; the largest group the kernels
    // serve (D + J <= 64: 63 coefficients, all in one group -- the eigenvalue routine's largest matrix); the most rows with J = 4
    const int shapes[][2] = {{1, 1}, {16, 1}, {16, 4}, {17, 1}, {17, 4}, {4, 4}, {63, 1}, {60, 4}};
    for (const auto& sh : shapes) {
        const int D = sh[0], J = sh[1];
        Buf<int32_t> groups = groups_of(D, J);
        if (D == 63) for (int d = 0; d < D; ++d) groups[(size_t)d] = 0;
        Buf<double> rank = dbuf(J, 0.0);
        Buf<double> Q = rw1_penalty(D, J, groups.get(), rank.get());
        EXPECT(glm_check_penalty(D, J, groups.get(), Q.get(), rank.get()) == PBBI_OK);
        EXPECT(glm_penalty_image_len(D, J) == (int64_t)glm_padded_dim(D + J) * glm_padded_dim(D + J));
        Buf<double> img = dbuf(glm_penalty_image_len(D, J), -1.0);
        glm_pack_penalty(D, J, Q.get(), img.get());
        EXPECT(img[0] == Q[0]);
        Q[(size_t)D * D - 1] = -1.0;  // the LAST entry: indefinite (or non-zero on a fixed row)
        EXPECT(glm_check_penalty(D, J, groups.get(), Q.get(), rank.get()) == PBBI_ERR_INVALID);
    }
    // the packer alone serves up to D + J = 128
    for (int D : {65, 124, 127}) {
        const int J = D == 127 ? 1 : 4;
        Buf<double> Q = dbuf((int64_t)D * D, 0.5, 0.25), img = dbuf(glm_penalty_image_len(D, J), -1.0);
        glm_pack_penalty(D, J, Q.get(), img.get());
        EXPECT(img[0] == Q[0]);
    }
}

static void softmax_shapes() {
    const int shapes[][2] = {{1, 2}, {16, 8}, {17, 4}, {64, 2}};
    for (const auto& sh : shapes)
        for (int64_t M : MS) {
            const int D = sh[0], K = sh[1];
            int Dc = 0, NT = 0;
            EXPECT(glm_softmax_layout(D, K, &Dc, &NT, nullptr) == PBBI_OK);
            EXPECT(Dc == glm_padded_dim(D) && NT == K * Dc / 16);
            Buf<int32_t> rows(new int32_t[(size_t)NT * 16]);
            EXPECT(glm_softmax_layout(D, K, nullptr, nullptr, rows.get()) == PBBI_OK);
            EXPECT(rows[(size_t)NT * 16 - 1] == (D == Dc ? K * D - 1 : -1));
            Buf<double> X = dbuf(M * D, 0.25, 0.5), y = dbuf(M, (double)(K - 1)), lam = dbuf(D, 0.5);
            EXPECT(glm_softmax_check(D, K, M, X.get(), y.get(), lam.get()) == PBBI_OK);
            y[(size_t)(M - 1)] = (double)K;
            EXPECT(glm_softmax_check(D, K, M, X.get(), y.get(), lam.get()) == PBBI_ERR_INVALID);
        }
    EXPECT(glm_softmax_layout(17, 8, nullptr, nullptr, nullptr) == PBBI_ERR_UNSUPPORTED);
    EXPECT(glm_softmax_layout(65, 2, nullptr, nullptr, nullptr) == PBBI_ERR_UNSUPPORTED);
}

// every rule of pbbi_pointwise_glm's arguments, in the order the checker states them; `samples` is only compared with NULL
static void pointwise_rules() {
    Buf<double> s = dbuf(1, 0.0);
    const void* p = s.get();
    const int fams[] = {PBBI_GLM_LOGISTIC, PBBI_GLM_POISSON, PBBI_GLM_GAUSSIAN, PBBI_GLM_NEGBINOMIAL};
    for (int fam : fams) {
        EXPECT(glm_check_pointwise(1, fam, 5, p, 3, 5, 150, 0, true) == PBBI_OK);
        EXPECT(glm_check_pointwise(1, fam, 5, p, 1, 7, 1, 1, false) == PBBI_OK);   // one draw without the variance; Dt > D
        EXPECT(glm_check_pointwise(1, fam, 128, p, 1, 128, 2, 65535, true) == PBBI_OK);
    }
    EXPECT(glm_check_pointwise(0, PBBI_GLM_LOGISTIC, 5, p, 3, 5, 150, 0, true) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("handle is NULL") != std::string::npos);
    EXPECT(glm_check_pointwise(1, PBBI_GLM_LOGISTIC, 5, nullptr, 3, 5, 150, 0, true) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("samples is NULL") != std::string::npos);
    EXPECT(glm_check_pointwise(1, PBBI_GLM_LOGISTIC, 5, p, 0, 5, 150, 0, true) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("S must be >= 1") != std::string::npos);
    EXPECT(glm_check_pointwise(1, PBBI_GLM_LOGISTIC, 5, p, 3, 5, 0, 0, true) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("N must be >= 1") != std::string::npos);
    EXPECT(glm_check_pointwise(1, PBBI_GLM_LOGISTIC, 5, p, 1, 5, 1, 0, true) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("at least two draws") != std::string::npos);
    EXPECT(glm_check_pointwise(1, PBBI_GLM_LOGISTIC, 5, p, 3, 5, 150, -1, true) == PBBI_ERR_INVALID);
    EXPECT(glm_check_pointwise(1, PBBI_GLM_LOGISTIC, 5, p, 3, 5, 150, 65536, true) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("ranges must be") != std::string::npos);
    EXPECT(glm_check_pointwise(1, PBBI_GLM_LOGISTIC, 5, p, 3, 4, 150, 0, true) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("state dimension") != std::string::npos);
    EXPECT(glm_check_pointwise(1, PBBI_GLM_SOFTMAX, 6, p, 3, 6, 150, 0, true) == PBBI_ERR_UNSUPPORTED);
    EXPECT(g_error.find("softmax") != std::string::npos && g_error.find(GLM_POINTWISE_RULE) != std::string::npos);
    EXPECT(glm_check_pointwise(2, 0, 5, p, 3, 5, 150, 0, true) == PBBI_ERR_UNSUPPORTED);
    EXPECT(g_error.find("not a GLM handle") != std::string::npos && g_error.find(GLM_POINTWISE_RULE) != std::string::npos);
    EXPECT(glm_check_pointwise(1, 99, 5, p, 3, 5, 150, 0, true) == PBBI_ERR_UNSUPPORTED);
    // S * N is formed in 64 bits
    EXPECT(glm_check_pointwise(1, PBBI_GLM_LOGISTIC, 5, p, 2000000000, 5, (int64_t)1 << 40, 0, true) == PBBI_OK);
}

// every rule of pbbi_loglik_glm's arguments, in the order the checker states them; the pointers are only compared with NULL
static void loglik_rules() {
    Buf<double> s = dbuf(1, 0.0), o = dbuf(1, 0.0);
    const void *p = s.get(), *u = o.get();
    for (int fam : {(int)PBBI_GLM_LOGISTIC, (int)PBBI_GLM_POISSON, (int)PBBI_GLM_GAUSSIAN, (int)PBBI_GLM_NEGBINOMIAL}) {
        EXPECT(glm_check_loglik(1, fam, 5, p, u, 3, 5, 150, 0) == PBBI_OK);
        EXPECT(glm_check_loglik(1, fam, 5, p, u, 1, 7, 1, 1) == PBBI_OK);  // one draw; Dt > D
        EXPECT(glm_check_loglik(1, fam, 128, p, u, 1, 128, 2, 65535) == PBBI_OK);
    }
    EXPECT(glm_check_loglik(0, PBBI_GLM_LOGISTIC, 5, nullptr, nullptr, 0, 4, 0, -1) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("handle is NULL") != std::string::npos);
    EXPECT(glm_check_loglik(1, PBBI_GLM_LOGISTIC, 5, nullptr, nullptr, 0, 4, 0, -1) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("samples is NULL") != std::string::npos);
    EXPECT(glm_check_loglik(1, PBBI_GLM_LOGISTIC, 5, p, nullptr, 0, 4, 0, -1) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("ulik_out is NULL") != std::string::npos);
    EXPECT(glm_check_loglik(1, PBBI_GLM_LOGISTIC, 5, p, u, 0, 4, 0, -1) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("S must be >= 1") != std::string::npos);
    EXPECT(glm_check_loglik(1, PBBI_GLM_LOGISTIC, 5, p, u, 3, 4, 0, -1) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("N must be >= 1") != std::string::npos);
    EXPECT(glm_check_loglik(1, PBBI_GLM_LOGISTIC, 5, p, u, 3, 4, 150, -1) == PBBI_ERR_INVALID);
    EXPECT(glm_check_loglik(1, PBBI_GLM_LOGISTIC, 5, p, u, 3, 4, 150, 65536) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("ranges must be") != std::string::npos);
    EXPECT(glm_check_loglik(2, 0, 5, p, u, 3, 4, 150, 0) == PBBI_ERR_UNSUPPORTED);
    EXPECT(g_error.find("not a GLM handle") != std::string::npos && g_error.find(GLM_POINTWISE_RULE) != std::string::npos);
    EXPECT(glm_check_loglik(1, PBBI_GLM_SOFTMAX, 6, p, u, 3, 4, 150, 0) == PBBI_ERR_UNSUPPORTED);
    EXPECT(g_error.find("softmax") != std::string::npos);
    EXPECT(glm_check_loglik(1, 99, 5, p, u, 3, 4, 150, 0) == PBBI_ERR_UNSUPPORTED);
    EXPECT(glm_check_loglik(1, PBBI_GLM_LOGISTIC, 5, p, u, 3, 4, 150, 0) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("state dimension") != std::string::npos);
    EXPECT(glm_check_loglik(1, PBBI_GLM_LOGISTIC, 5, p, u, 2000000000, 5, (int64_t)1 << 40, 0) == PBBI_OK);
}

// the rules pbbi_predictive_glm adds to those it shares (above), in the order the checker states them
static void predictive_rules() {
    Buf<double> s = dbuf(1, 0.0);
    const void* p = s.get();
    const double nan = std::nan("");
    EXPECT(glm_check_predictive(1, PBBI_GLM_POISSON, 5, p, p, p, 3, 5, 150, 0, 0, false, 1.5, 0.0) == PBBI_OK);
    EXPECT(glm_check_predictive(1, PBBI_GLM_ORDINAL, 9, p, p, p, 1, 9, (int64_t)1 << 32, 65535, 450, true, -1.5, 2.0) == PBBI_OK);
    EXPECT(glm_check_predictive(1, PBBI_GLM_SOFTMAX, 6, p, nullptr, nullptr, 3, 6, 150, 0, -1, true, nan, nan) == PBBI_ERR_UNSUPPORTED);
    EXPECT(g_error.find("pbbi_predictive_glm: a softmax handle") != std::string::npos);
    EXPECT(glm_check_predictive(1, PBBI_GLM_POISSON, 5, p, nullptr, nullptr, 3, 5, (int64_t)1 << 32, 0, -1, true, nan, nan) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("aux is NULL") != std::string::npos);
    EXPECT(glm_check_predictive(1, PBBI_GLM_POISSON, 5, p, p, nullptr, 3, 5, (int64_t)1 << 32, 0, -1, true, nan, nan) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("stats_out is NULL") != std::string::npos);
    EXPECT(glm_check_predictive(1, PBBI_GLM_POISSON, 5, p, p, p, 3, 5, (int64_t)1 << 32, 0, -1, true, nan, nan) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("S * N must be <= 2^32") != std::string::npos);
    EXPECT(glm_check_predictive(1, PBBI_GLM_POISSON, 5, p, p, p, 2000000000, 5, (int64_t)1 << 40, 0, 0, false, 0.0, 0.0) == PBBI_ERR_INVALID);
    EXPECT(glm_check_predictive(1, PBBI_GLM_POISSON, 5, p, p, p, 3, 5, 150, 0, 451, true, nan, nan) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("keep must be in") != std::string::npos);
    EXPECT(glm_check_predictive(1, PBBI_GLM_POISSON, 5, p, p, p, 3, 5, 150, 0, 5, false, nan, nan) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("keep > 0 needs yrep_out") != std::string::npos);
    EXPECT(glm_check_predictive(1, PBBI_GLM_POISSON, 5, p, p, p, 3, 5, 150, 0, 0, true, nan, nan) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("yrep_out needs keep > 0") != std::string::npos);
    EXPECT(glm_check_predictive(1, PBBI_GLM_POISSON, 5, p, p, p, 3, 5, 150, 0, 0, false, nan, nan) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("centre must be finite") != std::string::npos);
    EXPECT(glm_check_predictive(1, PBBI_GLM_POISSON, 5, p, p, p, 3, 5, 150, 0, 0, false, 0.0, INFINITY) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("cut must be finite") != std::string::npos);
    EXPECT(glm_check_predictive_keep(0, (int64_t)1 << 40) == PBBI_OK && glm_check_predictive_keep(1 << 14, 1 << 14) == PBBI_OK);
    EXPECT(glm_check_predictive_keep((1 << 14) + 1, 1 << 14) == PBBI_ERR_INVALID && g_error.find("keep * M") != std::string::npos);
    EXPECT(glm_check_predictive_keep((int64_t)1 << 40, (int64_t)1 << 40) == PBBI_ERR_INVALID);   // no overflow of the product
}

// every rule of pbbi_glm_hessian's arguments, in the order the checker states them; the pointers are only compared with NULL
static void hessian_rules() {
    Buf<double> s = dbuf(1, 0.0), o = dbuf(1, 0.0);
    const void *q = s.get(), *h = o.get();
    for (int fam : {(int)PBBI_GLM_LOGISTIC, (int)PBBI_GLM_POISSON, (int)PBBI_GLM_GAUSSIAN, (int)PBBI_GLM_NEGBINOMIAL, (int)PBBI_GLM_GAMMA})
        for (int ranges : {0, 1, 65535}) EXPECT(glm_check_hessian(1, fam, false, q, h, ranges) == PBBI_OK);
    EXPECT(glm_check_hessian(0, PBBI_GLM_SOFTMAX, true, nullptr, nullptr, -1) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("handle is NULL") != std::string::npos);
    EXPECT(glm_check_hessian(2, PBBI_GLM_SOFTMAX, true, nullptr, nullptr, -1) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("q is NULL") != std::string::npos);
    EXPECT(glm_check_hessian(2, PBBI_GLM_SOFTMAX, true, q, nullptr, -1) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("hess_out is NULL") != std::string::npos);
    EXPECT(glm_check_hessian(2, PBBI_GLM_SOFTMAX, true, q, h, -1) == PBBI_ERR_INVALID);
    EXPECT(glm_check_hessian(2, PBBI_GLM_SOFTMAX, true, q, h, 65536) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("ranges must be") != std::string::npos);
    EXPECT(glm_check_hessian(2, PBBI_GLM_SOFTMAX, true, q, h, 0) == PBBI_ERR_UNSUPPORTED);
    EXPECT(g_error.find("not a GLM handle") != std::string::npos && g_error.find(GLM_HESSIAN_RULE) != std::string::npos);
    EXPECT(glm_check_hessian(1, PBBI_GLM_SOFTMAX, true, q, h, 0) == PBBI_ERR_UNSUPPORTED);
    EXPECT(g_error.find("softmax") != std::string::npos);
    EXPECT(glm_check_hessian(1, PBBI_GLM_ORDINAL, true, q, h, 0) == PBBI_ERR_UNSUPPORTED);
    EXPECT(g_error.find("ordinal") != std::string::npos);
    EXPECT(glm_check_hessian(1, PBBI_GLM_LOGISTIC, true, q, h, 0) == PBBI_ERR_UNSUPPORTED);
    EXPECT(g_error.find("hierarchical") != std::string::npos && g_error.find(GLM_HESSIAN_RULE) != std::string::npos);
    EXPECT(glm_check_hessian(1, 99, false, q, h, 0) == PBBI_ERR_UNSUPPORTED);
    EXPECT(g_error.find("unknown GLM family") != std::string::npos);
}

// every rule of pbbi_potential_set_likelihood_power, in the checker's order
static void power_rules() {
    for (int fam : {(int)PBBI_GLM_LOGISTIC, (int)PBBI_GLM_POISSON, (int)PBBI_GLM_GAUSSIAN, (int)PBBI_GLM_NEGBINOMIAL}) {
        EXPECT(glm_check_power(1, fam, true, 1.0, false) == PBBI_OK && glm_check_power(1, fam, true, 1e-300, false) == PBBI_OK);
        EXPECT(glm_check_power(1, fam, true, (double)NAN, true) == PBBI_OK);  // read from the device: not checked
    }
    EXPECT(glm_check_power(0, PBBI_GLM_SOFTMAX, false, -1.0, false) == PBBI_ERR_INVALID);
    EXPECT(g_error.find("handle is NULL") != std::string::npos);
    EXPECT(glm_check_power(2, PBBI_GLM_SOFTMAX, false, -1.0, false) == PBBI_ERR_UNSUPPORTED);
    EXPECT(g_error.find("not a GLM handle") != std::string::npos && g_error.find(GLM_POWER_RULE) != std::string::npos);
    EXPECT(glm_check_power(1, PBBI_GLM_SOFTMAX, false, -1.0, false) == PBBI_ERR_UNSUPPORTED);
    EXPECT(g_error.find("softmax") != std::string::npos);
    EXPECT(glm_check_power(1, PBBI_GLM_LOGISTIC, false, -1.0, false) == PBBI_ERR_UNSUPPORTED);
    EXPECT(g_error.find("no observation streams") != std::string::npos);
    for (double v : {0.0, -1.0, (double)NAN, (double)INFINITY}) {
        EXPECT(glm_check_power(1, PBBI_GLM_LOGISTIC, true, v, false) == PBBI_ERR_INVALID);
        EXPECT(g_error.find("finite and > 0") != std::string::npos);
    }
}

// the diagonal metric's table: 2 * glm_padded_dim(D) doubles, {m_d, 1 / m_d} then {1, 1}; the last entry is the one found
static void metric_tables() {
    for (int D : DS) {
        const int64_t len = 2 * (int64_t)glm_padded_dim(D);
        int64_t n = -1;
        EXPECT(pbbi_glm_pack_metric(D, nullptr, nullptr, 0, &n) == PBBI_OK && n == len);
        Buf<double> m = dbuf(D, 0.75, 0.5), out = dbuf(len, -1.0);
        EXPECT(pbbi_glm_pack_metric(D, m.get(), out.get(), len, &n) == PBBI_OK && n == len);
        EXPECT(out[0] == 0.75 && out[1] == 1.0 / 0.75);
        EXPECT(out[(size_t)(2 * D - 2)] == m[(size_t)(D - 1)] && out[(size_t)(2 * D - 1)] == 1.0 / m[(size_t)(D - 1)]);
        EXPECT(out[(size_t)(len - 2)] == (D == glm_padded_dim(D) ? m[(size_t)(D - 1)] : 1.0));
        EXPECT(pbbi_glm_pack_metric(D, m.get(), out.get(), len - 1, &n) == PBBI_ERR_INVALID);
        EXPECT(pbbi_glm_pack_metric(D, nullptr, out.get(), len, &n) == PBBI_ERR_INVALID);
        for (double v : {0.0, -1.0, (double)NAN, (double)INFINITY}) {
            m[(size_t)(D - 1)] = v;
            EXPECT(pbbi_glm_pack_metric(D, m.get(), out.get(), len, &n) == PBBI_ERR_INVALID);
            EXPECT(g_error.find("finite and > 0") != std::string::npos);
        }
    }
    EXPECT(pbbi_glm_pack_metric(0, nullptr, nullptr, 0, nullptr) == PBBI_ERR_INVALID);
    EXPECT(pbbi_glm_pack_metric(129, nullptr, nullptr, 0, nullptr) == PBBI_ERR_INVALID);
    // which METRIC kernels ship: where their parents do, but for the softmax kernel at 64 rows per class
    EXPECT(glm_metric_max_dim(GLM_V_PLAIN, PBBI_GLM_LOGISTIC, 0, 128, 0) == 128 && glm_metric_max_dim(GLM_V_SOFTMAX, PBBI_GLM_SOFTMAX, 0, 16, 8) == 128);
    for (int v : {GLM_V_HIER, GLM_V_HIER_NC, GLM_V_HIER_Q})
        EXPECT(glm_metric_max_dim(v, PBBI_GLM_LOGISTIC, 0, 64, 0) == 64 && glm_metric_max_dim(v, PBBI_GLM_GAUSSIAN, 0, 64, 0) == 0);
    EXPECT(glm_metric_max_dim(GLM_V_DISPERSION, PBBI_GLM_NEGBINOMIAL, 0, 64, 0) == 64 && glm_metric_max_dim(99, PBBI_GLM_LOGISTIC, 0, 16, 0) == 0);
    EXPECT(glm_metric_max_dim(GLM_V_DISPERSION, PBBI_GLM_GAMMA, 0, 128, 0) == 128 && glm_metric_max_dim(GLM_V_HIER_DISPERSION, PBBI_GLM_GAMMA, 0, 64, 0) == 0);
    EXPECT(glm_metric_max_dim(GLM_V_SOFTMAX, PBBI_GLM_SOFTMAX, 0, 64, 2) == 0 && glm_metric_max_dim(GLM_V_SOFTMAX, PBBI_GLM_SOFTMAX, 0, 32, 4) == 128);
}

// the dense metric's images: 3 DP^2 doubles, C | L | M in A-fragment order, over an exactly-sized (D x D) matrix and an exactly-
// sized output; the first entry of each image is its [0][0], the last (lane 63, e = 1 of the last K-step pair of the last block)
// its [DP - 1][DP - 1]
static void dense_metric_images() {
    for (int D : {1, 5, 16, 17, 33, 64}) {
        const int DP = glm_padded_dim(D);
        const int64_t len = 3 * (int64_t)DP * DP;
        int64_t n = -1;
        EXPECT(pbbi_glm_pack_metric_dense(D, nullptr, nullptr, 0, &n) == PBBI_OK && n == len && glm_metric_dense_len(D) == len);
        // tridiagonal, diagonally dominant: 2 + (i % 3) on the diagonal, -0.5 beside it
        Buf<double> M = dbuf((int64_t)D * D, 0.0);
        for (int i = 0; i < D; ++i) {
            M[(size_t)i * D + i] = 2.0 + (double)(i % 3);
            if (i + 1 < D) M[(size_t)i * D + i + 1] = M[(size_t)(i + 1) * D + i] = -0.5;
        }
        EXPECT(glm_check_metric_dense(D, M.get()) == PBBI_OK);
        Buf<double> out = dbuf(len, -7.0);
        EXPECT(pbbi_glm_pack_metric_dense(D, M.get(), out.get(), len, &n) == PBBI_OK && n == len);
        const size_t sq = (size_t)DP * DP;
        EXPECT(out[2 * sq] == 2.0 && out[sq] == std::sqrt(2.0));
        const double last = D == DP ? M[(size_t)D * D - 1] : 1.0;
        EXPECT(out[3 * sq - 1] == last);
        if (D < DP) EXPECT(out[sq - 1] == 1.0 && out[2 * sq - 1] == 1.0);  // the identity on the padding
        for (int64_t i = 0; i < len; ++i)
            if (!std::isfinite(out[(size_t)i]) || out[(size_t)i] == -7.0) { EXPECT(!"an entry of the images was left unwritten"); break; }
        EXPECT(pbbi_glm_pack_metric_dense(D, M.get(), out.get(), len - 1, &n) == PBBI_ERR_INVALID && g_error.find("shorter") != std::string::npos);
        EXPECT(pbbi_glm_pack_metric_dense(D, nullptr, out.get(), len, &n) == PBBI_ERR_INVALID);
        // the rules, in their order: finite, symmetric, positive definite
        const double keep = M[(size_t)D * D - 1];
        M[(size_t)D * D - 1] = NAN;
        EXPECT(glm_check_metric_dense(D, M.get()) == PBBI_ERR_INVALID && g_error.find("finite") != std::string::npos);
        M[(size_t)D * D - 1] = -keep;
        EXPECT(glm_check_metric_dense(D, M.get()) == PBBI_ERR_INVALID && g_error.find("positive definite") != std::string::npos);
        M[(size_t)D * D - 1] = keep;
        if (D > 1) {
            M[1] += 1e-6;
            EXPECT(glm_check_metric_dense(D, M.get()) == PBBI_ERR_INVALID && g_error.find("symmetric") != std::string::npos);
            M[1] -= 1e-6;
        }
        EXPECT(glm_check_metric_dense(D, M.get()) == PBBI_OK);
    }
    EXPECT(pbbi_glm_pack_metric_dense(0, nullptr, nullptr, 0, nullptr) == PBBI_ERR_UNSUPPORTED);
    EXPECT(pbbi_glm_pack_metric_dense(65, nullptr, nullptr, 0, nullptr) == PBBI_ERR_UNSUPPORTED && glm_check_metric_dense(65, nullptr) == PBBI_ERR_UNSUPPORTED);
    // which dense-metric kernels ship: the plain and full models and the dispersion families up to 64 rows, nothing else
    EXPECT(glm_dense_metric_max_dim(GLM_V_PLAIN, PBBI_GLM_LOGISTIC) == 64 && glm_dense_metric_max_dim(GLM_V_FULL, PBBI_GLM_POISSON) == 64);
    for (int f : {PBBI_GLM_GAUSSIAN, PBBI_GLM_NEGBINOMIAL, PBBI_GLM_GAMMA}) EXPECT(glm_dense_metric_max_dim(GLM_V_DISPERSION, f) == 64);
    for (int v : {(int)GLM_V_SOFTMAX, (int)GLM_V_HIER, (int)GLM_V_HIER_NC, (int)GLM_V_HIER_Q, (int)GLM_V_HIER_DISPERSION, (int)GLM_V_ORDINAL, 99})
        for (int f = 0; f < 7; ++f) EXPECT(glm_dense_metric_max_dim(v, f) == 0);
    EXPECT(glm_dense_metric_max_rows(PBBI_GLM_ORDINAL, true, 0) == 0 && glm_dense_metric_max_rows(PBBI_GLM_LOGISTIC, true, 1) == 0);
}

int main() {
    metric_tables();
    dense_metric_images();
    design_and_observations();
    hierarchical_tables();
    penalties();
    softmax_shapes();
    pointwise_rules();
    loglik_rules();
    predictive_rules();
    hessian_rules();
    power_rules();
    // what is shipped (the one statement the entries and the launch read)
    EXPECT(glm_max_dim(GLM_V_PLAIN, PBBI_GLM_LOGISTIC) == 128 && glm_max_dim(GLM_V_FULL, PBBI_GLM_POISSON) == 128);
    EXPECT(glm_max_dim(GLM_V_DISPERSION, PBBI_GLM_GAUSSIAN) == 128 && glm_max_dim(GLM_V_DISPERSION, PBBI_GLM_NEGBINOMIAL) == 64);
    for (int v : {GLM_V_HIER, GLM_V_HIER_NC, GLM_V_HIER_Q})
        EXPECT(glm_max_dim(v, PBBI_GLM_LOGISTIC) == 64 && glm_max_dim(v, PBBI_GLM_POISSON) == 64 && glm_max_dim(v, PBBI_GLM_GAUSSIAN) == 0);
    EXPECT(glm_max_dim(GLM_V_HIER_DISPERSION, PBBI_GLM_GAUSSIAN) == 64 && glm_max_dim(GLM_V_HIER_DISPERSION, PBBI_GLM_LOGISTIC) == 0);
    // the Gamma family: the Gaussian's shapes without random effects, and on no other frame
    EXPECT(glm_max_dim(GLM_V_DISPERSION, PBBI_GLM_GAMMA) == 128 && glm_max_dim(GLM_V_HIER_DISPERSION, PBBI_GLM_GAMMA) == 0);
    EXPECT(glm_max_dim(GLM_V_FULL, PBBI_GLM_GAMMA) == 0 && glm_max_dim(GLM_V_HIER, PBBI_GLM_GAMMA) == 0);
    EXPECT(glm_disp(PBBI_GLM_GAMMA) && !glm_canonical(PBBI_GLM_GAMMA) && std::string(glm_family_name(PBBI_GLM_GAMMA)) == "gamma");
    EXPECT(glm_max_dim(GLM_V_SOFTMAX, PBBI_GLM_SOFTMAX) == 0 && glm_max_dim(99, PBBI_GLM_LOGISTIC) == 0);
    // the ordinal family: 64 rows on its own variant, with the metric where it ships, and on no other frame
    EXPECT(glm_max_dim(GLM_V_ORDINAL, PBBI_GLM_ORDINAL) == 64 && GLM_ORDINAL_MAX_ROWS == 64);
    EXPECT(glm_max_dim(GLM_V_ORDINAL, PBBI_GLM_LOGISTIC) == 0 && glm_max_dim(GLM_V_FULL, PBBI_GLM_ORDINAL) == 0);
    EXPECT(glm_max_dim(GLM_V_DISPERSION, PBBI_GLM_ORDINAL) == 0 && glm_max_dim(GLM_V_HIER, PBBI_GLM_ORDINAL) == 0);
    EXPECT(glm_max_dim(GLM_V_HIER_DISPERSION, PBBI_GLM_ORDINAL) == 0);
    EXPECT(glm_metric_max_dim(GLM_V_ORDINAL, PBBI_GLM_ORDINAL, 0, 64, 8) == 64 && glm_metric_max_rows(PBBI_GLM_ORDINAL, true, 0) == 64);
    EXPECT(!glm_disp(PBBI_GLM_ORDINAL) && !glm_canonical(PBBI_GLM_ORDINAL) && std::string(glm_family_name(PBBI_GLM_ORDINAL)) == "ordinal");
    EXPECT(glm_check_ordinal_shape(60, 5) == PBBI_OK && glm_check_ordinal_shape(57, 8) == PBBI_OK && glm_check_ordinal_shape(1, 2) == PBBI_OK);
    EXPECT(glm_check_ordinal_shape(61, 5) == PBBI_ERR_UNSUPPORTED && g_error.find("<= 64 (65)") != std::string::npos);
    EXPECT(glm_check_ordinal_shape(5, 1) == PBBI_ERR_INVALID && glm_check_ordinal_shape(5, 9) == PBBI_ERR_INVALID);
    EXPECT(glm_check_ordinal_shape(0, 3) == PBBI_ERR_INVALID);
    if (bad) {
        std::printf("%d expectation(s) failed\n", bad);
        return 1;
    }
    std::printf("asan ok\n");
    return 0;
}
