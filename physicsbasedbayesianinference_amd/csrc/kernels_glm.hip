// kernels_glm.hip -- generalised linear models whose likelihood runs on the fp64 matrix cores (gfx950).
//
//   U(w) = sum_i [ b(x_i.w) - y_i (x_i.w) ] + 0.5 lam |w|^2,   grad U = X^T (b'(eta) - y) + lam w,   eta = X w
// over the M rows x_i of the design matrix X (M x D).  For an ENSEMBLE of chains these are two matrix products
// shared by all of them -- eta = X W and g = X^T R with W, R of one column per chain -- so the data set is read
// once per 64 chains instead of once per chain (the user-source plugin path, custom.LOGISTIC_REGRESSION_SOURCE).
//
// Layout.  One wave owns 16 chains and keeps q, the half-step velocity vh and the gradient accumulator in
// registers in the layout of kernels_dense_dev.h: element s of a lane is row 4s + g, g = lane >> 4, chain =
// lane & 15.  X travels through LDS in blocks of 16 observations, pre-swizzled on the host (glm_pack) into the
// A-fragment order of v_mfma_f64_16x16x4_f64 -- twice, once per product:
//   P1[s2][lane][e]     = X[16b + (lane & 15)][4 (2 s2 + e) + (lane >> 4)]       eta tile   = X_b (16 x DP) . W
//   P2[r2][t][lane][e]  = X[16b + 4 (2 r2 + e) + (lane >> 4)][16 t + (lane & 15)] g tile t += X_b^T (DP x 16) . R_b
// (e = the two halves of one 16-byte LDS read).  The first product's B operand of K-step s is q[s] as it sits
// (B[k = lane >> 4][j = lane & 15] = W[4s + g][chain]).  Its result has C/D map col = lane & 15, row =
// (lane >> 4) + 4 reg: register r of the eta tile holds the observations {4r + g} of the lane's own chain --
// exactly the B operand of the K-step of the SECOND product that sums over those four observations.  The link
// function is applied in place on the four accumulator values and they go straight back into the matrix pipe: no
// cross-lane movement, no LDS round trip.  The second product's C/D rows (lane >> 4) + 4 r' of tile t are rows
// 16t + 4r' + g: the state layout again.
//
// Padding.  Rows of the last block past M are zeros in the image, but b(0) and b'(0) are not zero (log 2 and 1/2,
// 1 and 1): both the residual and the energy term of an observation >= M are masked.  Columns D <= d < DP are
// zeros in the image; the state arrays are addressed through bounded descriptors (pbbi_buf.h), so rows d >= D
// load 0 and their stores are dropped.
//
// One launch is one HMC iteration (or one integrate(), or one evaluation): kick-drift-kick with fused
// multiply-adds like the other MFMA kernels, ONE call site of the gradient inside a loop over the trajectory's
// evaluations whose kick / drift coefficients say which update follows it.  Nothing is carried between the
// iterations of a run, so a run of S iterations is S launches and equals S runs of one bit for bit by
// construction.
//
// The full model (RICH = true; handles of pbbi_potential_create_glm_ex):
//   U(w) = sum_i a_i [ n_i b(eta_i) - y_i eta_i ] + 0.5 sum_d lam_d (w_d - mu_d)^2,   eta_i = x_i.w + o_i
// with observation weights a_i, binomial trials n_i and offsets o_i.  The device sees c_i = a_i n_i, d_i = a_i y_i
// and o_i: three streams of one value per observation that travel through LDS beside the X chunk where the plain
// model stages y alone (U_i = c_i b(eta_i) - d_i eta_i, r_i = c_i b'(eta_i) - d_i).  An observation with c_i = d_i
// = 0 is SELECTED out like one past M -- its b(eta_i) may have overflowed and 0 * inf is NaN.  lam_d and mu_d sit in
// LDS for the whole launch (2 DP doubles, loaded once): KS more values per lane in registers would push the DP =
// 128 kernels into scratch, and they are read KS times per gradient next to M DP / 8 MFMAs.  The plain model's
// instantiations (RICH = false) hold none of this: their code is what it was before the full model existed.
//
// The dispersion families (FAM = PBBI_GLM_GAUSSIAN, PBBI_GLM_NEGBINOMIAL of k_glm<NT, FAM, true>; handles of
// pbbi_potential_create_glm_dispersion) add a parameter that is no coefficient of X: theta, the log-dispersion, which
// enters every observation's link and whose gradient is a sum over observations per chain (include/pbbi.h has the model).
// Sampled, theta is row D of the state (D = the coefficient count): the image is that of [X | 0], so eta does not see the
// row, while the momentum draw, kick, drift, stores and the {lam, mu} prior in plds treat it like any other.  Once per
// gradient evaluation the lane that owns row D (s = D >> 2, g = D & 3) contributes its q[s] to a chain_sum, the other
// three lane groups contribute 0 (adding zeros is exact), and every lane of the chain has theta; the per-chain
// quantities (tau; phi, psi(phi), lgamma(phi)) are formed there, once.  Each lane accumulates dU_i/dtheta of its
// observations next to usum, and chain_sum of that goes into the gradient accumulator at (s, g) before the kick and the
// evaluation's store.  Held, theta comes from the kernel arguments (a wave-uniform switch, no further instantiations)
// and the state is w alone.  The streams are c = a, d = y (raw), o; a row with c = 0 is selected out.
//
// Hierarchical priors (HIER = GLM_HIER_CENTRED of k_glm<NT, FAM, true, HIER>, FAM logistic / poisson; handles of
// pbbi_potential_create_glm_hier; include/pbbi.h has the model): a block of coefficients shares the prior scale exp(t_j),
// and t_0 .. t_{J-1} (J <= 4) are rows D .. D+J-1 of the state, behind zero columns of the image like theta above.  The
// likelihood walk is the full model's.  The {lam, mu} table in plds carries the grouping -- a member of group j has
// -(j + 1) in its lam slot (lam >= 0 otherwise), row D + j the Gaussian prior of t_j -- followed by four entries {n_j, 0}.
// Once per gradient evaluation, after glm_grad: each lane sums (q - mu)^2 of its rows per group; a lane owns at most one
// t row (they are consecutive, a lane's rows 4 apart) and contributes its q to that t_j's chain_sum, 0 to the others';
// tau_j = exp(-2 t_j) is formed once; n_j - tau_j S_j goes into the gradient accumulator at the owner's register.  Kick,
// evaluation store and energy use tau_j where a fixed row uses its lam (glm_hier_lam: four selects on the value read).
//
// The non-centred parametrisation (HIER = GLM_HIER_NC; handles of pbbi_potential_create_glm_hier_ex): a grouped row of the
// state holds z_d with w_d = mu_d + sig_j z_d, sig_j = exp(t_j), and z_d ~ N(0, 1) a priori; fixed rows and t rows are as
// above, and so is the table in plds (its {n_j, 0} tail is not staged).  Before glm_grad: the t_j are broadcast as above,
// sig_j is formed once, and the first product's B operand is a scaled copy weff of the state (grouped ? fma(sig_j, q, mu) :
// q -- compile-time-indexed selects on the sign-coded lam slot); q is not touched.  After it, gL = X^T r at w(z, t) sits in
// gacc: each lane sums gL_d z_d of its rows per group, sig_j chain_sum(...) = dU/dt_j's likelihood part goes to the owner's
// register, and grouped rows of gacc are multiplied by sig_j (dU/dz_d = sig_j gL_d + z_d).  Kick, evaluation store and
// energy give a grouped row precision 1 and mean 0 (glm_nc_prior: its mu slot is the mean of w and must not enter the prior
// of z).  No n_j t_j in U: U_nc(z, t) = U_c(w(z, t), t) - sum_j n_j t_j, the Jacobian of the change of variables.
//
// Structured group priors (HIER = GLM_HIER_Q; handles of pbbi_potential_create_glm_hier_q): the centred model with a
// symmetric PSD matrix in each group's quadratic form, w_j - mu_j | t_j ~ N(0, exp(2 t_j) Q_j^-) -- random walks, ICAR,
// difference penalties; Q_j = I is the model above.  The host lays the J blocks out as one (D x D) matrix in coefficient
// indexing (identity on exchangeable groups, zero on fixed rows and between groups) and packs it with the FIRST product's
// A-fragment writer, one block per 16 rows of Q (glm_pack_penalty): 8 DP^2 bytes that sit in LDS behind plds for the whole
// launch.  Once per gradient evaluation, after glm_grad: dq[s] = member ? q[s] - mu : 0 (a SELECT on the sign of the lam
// slot, so a t row or a diverged fixed row never meets a zero of Q as 0 * inf) is the B operand of K-step s exactly as q[s]
// is for X_b . W, and tile t of Q . dq comes out with register r = row 16t + 4r + g: the state layout, no movement.  Tile by
// tile the lane adds dq . (Q dq) of its rows to its group sums and tau_j (Q dq) into gacc for member rows, so one tile of
// the product is live at a time.  dU/dt_j = r_j - tau_j S_j with r_j = rank(Q_j) in the table's {n_j, 0} slot; kick, store
// and energy apply {lam, mu} to fixed and t rows only (a second select on the sign), the energy adds 0.5 sum_j tau_j S_j.
//
// Random effects for the dispersion families (FAM = 3, 4 with HIER = GLM_HIER_CENTRED / GLM_HIER_NC; handles of
// pbbi_potential_create_glm_hier_dispersion): the two paragraphs above composed.  The state is [w; t_0 .. t_{J-1}; theta], theta
// LAST when it is sampled (row trow = trow0 + J) and from the arguments when it is held; the table in plds is lam (DP) | mu
// (DP) | n_j with DP the padded D + J + sampled, the theta row a fixed row {lam_theta, m_theta} behind a zero column of the
// image.  Per evaluation: theta is broadcast and glm_disp_chain formed BEFORE glm_grad, whatever HIER is; the t rows are
// broadcast as above (a lane owns at most one t row; for J = 4 the lane group of t_0 owns theta too, one register on -- the two
// broadcasts select on their own (s, g) and share nothing); chain_sum(tsum) goes into gacc at theta's owner LAST, after the
// non-centred branch has taken G[j] from gacc and scaled its grouped rows (the theta row is fixed, so either order is exact;
// this one keeps the dispersion kernels' sequence of operations).  Nothing else is new: weff leaves the theta row as q, S_j and
// G_j select on the group codes and never see it, kick / store / energy give it its {lam, mu} like any fixed row.
#include <cmath>
#include <cstring>
#include <type_traits>

#include "kernels_dense_dev.h"
#include "pbbi_chain.h"

static int64_t glm_blocks_padded(int64_t M);

namespace {

struct GlmPrm {
    const double* img;  // nbp blocks of 2 * KS * 64 doubles (P1 then P2), nbp = blocks padded to a multiple of 4
    const double* y;    // nbp * 16, zero padded
    const double* q_in;
    const double* p_in;
    const double* u_in;
    const double* mass;
    double* q_out;
    double* p_out;
    double* v_out;
    double* ratio_out;
    uint8_t* reject_out;
    double* U_out;     // modes 2..4
    double* grad_out;  // mode 2
    double* w_out;     // mode 3
    int64_t N, ldn_in, ldn_out, M;
    double h, lam, kT;
    int L, D, flags, rng, mode, method, nb;
    uint64_t seed, iter, chain0;
};
// the full model's kernel arguments (the plain kernels keep theirs as they are)
struct GlmPrmRich : GlmPrm {
    const double* obs;    // c | d | o, each obs_stride = nbp * 16 doubles, zero padded
    const double* prior;  // lam (DP) | mu (DP), zero padded past D
    int64_t obs_stride;
};
// the dispersion families' kernel arguments (the full model's kernels keep theirs as they are)
struct GlmPrmDisp : GlmPrmRich {
    double theta;  // the held log-dispersion (trow < 0)
    int trow;      // the state row of theta when it is sampled, -1 when it is held
};
// the hierarchical prior's kernel arguments (the full model's kernels keep theirs as they are)
struct GlmPrmHier : GlmPrmRich {  // prior: lam (DP) | mu (DP) | n_j (4, the members of each group, 0 past J)
    int trow0;     // the state row of t_0 (= the coefficient count); t_j is row trow0 + j
    int J;         // groups, 1 .. 4
};
// random effects for the dispersion families: the hierarchical prior's arguments plus theta; trow0 + J == trow when sampled
struct GlmPrmHierDisp : GlmPrmHier {
    double theta;  // the held log-dispersion (trow < 0)
    int trow;      // the state row of theta when it is sampled (the LAST row), -1 when it is held
};
// structured group priors: ... | r_j = rank(Q_j) in the n_j slots
struct GlmPrmHierQ : GlmPrmHier {
    const double* qimg;  // the (DP x DP) penalty in the first product's A-fragment order, DP / 16 blocks of DP * 16 doubles
};
constexpr bool glm_disp(int fam) { return fam == PBBI_GLM_GAUSSIAN || fam == PBBI_GLM_NEGBINOMIAL; }
// HIER of k_glm: no hierarchical prior, the centred parametrisation (the chain holds w_d), the non-centred one (z_d), the
// centred one with a penalty matrix in each group's quadratic form
enum { GLM_HIER_NONE = 0, GLM_HIER_CENTRED = 1, GLM_HIER_NC = 2, GLM_HIER_Q = 3 };
template <int FAM, bool RICH, int HIER = GLM_HIER_NONE>
struct GlmArgs {
    using type = std::conditional_t<HIER == GLM_HIER_Q, GlmPrmHierQ,
                                    std::conditional_t<HIER != GLM_HIER_NONE, std::conditional_t<glm_disp(FAM), GlmPrmHierDisp, GlmPrmHier>, GlmPrm>>;
};
template <int FAM>
struct GlmArgs<FAM, true, GLM_HIER_NONE> { using type = std::conditional_t<glm_disp(FAM), GlmPrmDisp, GlmPrmRich>; };
enum { GLM_HMC = 0, GLM_INTEGRATE = 1, GLM_EVAL = 2, GLM_ENERGY = 3, GLM_RATIO = 4 };

template <int NT>
struct GlmCfg {
    static constexpr int KS = 4 * NT;
    static constexpr int CB = NT >= 4 ? 1 : 4 / NT;    // observation blocks per staged chunk
    static constexpr int BLKV = NT * 256;              // 16-byte elements per block (P1 + P2)
    static constexpr int CHV = CB * BLKV;              // ... per chunk
    static constexpr int PER_THREAD = CHV / BLOCK;     // = CB * NT
    static_assert(CHV % BLOCK == 0, "whole 16-byte elements per thread");
    static constexpr int OBS = CB * 16;                // observations per chunk
    static_assert(3 * OBS <= BLOCK, "one thread per staged value of c | d | o");
};

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
struct GlmDispChain { double theta, a, b, c; };

template <int FAM>
__device__ __forceinline__ GlmDispChain glm_disp_chain(double theta, bool want_u) {
    GlmDispChain k{theta, 0.0, 0.0, 0.0};
    if constexpr (FAM == PBBI_GLM_GAUSSIAN) {
        k.a = exp(-2.0 * theta);
    } else {
        k.a = exp(theta);
        k.b = glm_psi(k.a);
        if (want_u) k.c = glm_lgamma(k.a);
    }
    return k;
}

// the dispersion families' U_i, dU_i/deta and dU_i/dtheta (cv = a_i, yv = y_i)
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
    } else {
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

// hierarchical prior: the precision of a row from the lam slot of its plds entry -- lam >= 0 is a fixed row's own,
// -(j + 1) marks a member of group j, whose precision is tau_j = exp(-2 t_j) of this chain
__device__ __forceinline__ double glm_hier_lam(double x, const double (&tau)[4]) {
    double r = x;
    r = (x == -1.0) ? tau[0] : r;
    r = (x == -2.0) ? tau[1] : r;
    r = (x == -3.0) ? tau[2] : r;
    r = (x == -4.0) ? tau[3] : r;
    return r;
}

// non-centred hierarchical prior: the {precision, mean} of a row's prior in the SAMPLED coordinate.  A grouped row (lam
// slot < 0) holds z_d ~ N(0, 1): its mu slot is the mean of w_d, which enters weff and not this prior.
__device__ __forceinline__ v2f64 glm_nc_prior(v2f64 pm) {
    const bool grouped = pm.x < 0.0;
    return v2f64{grouped ? 1.0 : pm.x, grouped ? 0.0 : pm.y};
}

// gacc[t][r] (row 16t + 4r + g) = sum_i X[i][row] (b'(eta_i) - y_i) for the wave's 16 chains, usum = this lane's
// share of sum_i b(eta_i) - y_i eta_i (observations {4r + g} of every block; chain_sum completes it).
// Every wave of the workgroup takes part in the staging: one chunk of CB blocks is in LDS while the next waits
// in registers (fetched before the MFMAs of the current one, written after the barrier that ends its reads).
// RICH: ylds holds the chunk's c | d | o (OBS values each); thread j < 3 OBS stages value j % OBS of stream j / OBS.
// Dispersion families: dk = the chain's theta-derived values, tsum = this lane's share of sum_i dU_i/dtheta.
template <int NT, int FAM, bool RICH, int HIER = GLM_HIER_NONE>
__device__ __forceinline__ void glm_grad(const typename GlmArgs<FAM, RICH, HIER>::type& prm, v2f64* __restrict__ lds,
                                         double* __restrict__ ylds, int lane, int g, const double (&q)[4 * NT], v4f64 (&gacc)[NT],
                                         double& usum, bool want_u, [[maybe_unused]] const GlmDispChain& dk,
                                         [[maybe_unused]] double& tsum) {
    using C = GlmCfg<NT>;
    constexpr int KS = C::KS;
    const v2f64* __restrict__ src = reinterpret_cast<const v2f64*>(prm.img);
    const int nch = (prm.nb + C::CB - 1) / C::CB;
    v2f64 tmp[C::PER_THREAD];
    double ytmp = 0.0;
    const double* __restrict__ osrc = nullptr;  // RICH: this thread's value of chunk 0
    if constexpr (RICH)
        if (threadIdx.x < 3 * C::OBS) osrc = prm.obs + (threadIdx.x / C::OBS) * prm.obs_stride + threadIdx.x % C::OBS;
#pragma unroll
    for (int j = 0; j < C::PER_THREAD; ++j) tmp[j] = src[threadIdx.x + j * BLOCK];
    if constexpr (RICH) {
        if (osrc) ytmp = osrc[0];
    } else {
        if (threadIdx.x < C::CB * 16) ytmp = prm.y[threadIdx.x];
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) gacc[t] = v4f64{0.0, 0.0, 0.0, 0.0};
    usum = 0.0;
    if constexpr (glm_disp(FAM)) tsum = 0.0;
    for (int ch = 0; ch < nch; ++ch) {
        __syncthreads();  // everybody has finished reading the previous chunk
#pragma unroll
        for (int j = 0; j < C::PER_THREAD; ++j) lds[threadIdx.x + j * BLOCK] = tmp[j];
        if constexpr (RICH) {
            if (osrc) ylds[threadIdx.x] = ytmp;
        } else {
            if (threadIdx.x < C::CB * 16) ylds[threadIdx.x] = ytmp;
        }
        __syncthreads();
        if (ch + 1 < nch) {
            const v2f64* nsrc = src + (size_t)(ch + 1) * C::CHV;
#pragma unroll
            for (int j = 0; j < C::PER_THREAD; ++j) tmp[j] = nsrc[threadIdx.x + j * BLOCK];
            if constexpr (RICH) {
                if (osrc) ytmp = osrc[(size_t)(ch + 1) * C::OBS];
            } else {
                if (threadIdx.x < C::CB * 16) ytmp = prm.y[(size_t)(ch + 1) * (C::CB * 16) + threadIdx.x];
            }
        }
#pragma unroll
        for (int bi = 0; bi < C::CB; ++bi) {
            const int blk = ch * C::CB + bi;
            if (C::CB > 1 && blk >= prm.nb) break;
            const v2f64* __restrict__ P1 = lds + bi * C::BLKV + lane;
            const v2f64* __restrict__ P2 = P1 + (KS / 2) * 64;
            // eta tile: 16 observations x 16 chains, K = DP
            v4f64 eta = v4f64{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s2 = 0; s2 < KS / 2; ++s2) {
                const v2f64 A = P1[s2 * 64];
                eta = __builtin_amdgcn_mfma_f64_16x16x4f64(A.x, q[2 * s2], eta, 0, 0, 0);
                eta = __builtin_amdgcn_mfma_f64_16x16x4f64(A.y, q[2 * s2 + 1], eta, 0, 0, 0);
            }
            // link function in place: register r = observations {4r + g} of this lane's chain
            double res[4];
            const int64_t obs0 = (int64_t)blk * 16 + g;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool ok = obs0 + 4 * r < prm.M;
                double rr, ut;
                if constexpr (glm_disp(FAM)) {
                    const int i = bi * 16 + 4 * r + g;
                    const double cv = ylds[i], yv = ylds[C::OBS + i], ov = ylds[2 * C::OBS + i];
                    double tt;
                    glm_link_disp<FAM>(eta[r] + ov, cv, yv, dk, want_u, rr, ut, tt);
                    const bool on = ok && cv != 0.0;  // weight 0: exactly nothing
                    res[r] = on ? rr : 0.0;
                    usum += on ? ut : 0.0;
                    tsum += on ? tt : 0.0;
                } else if constexpr (RICH) {
                    const int i = bi * 16 + 4 * r + g;
                    const double cv = ylds[i], dv = ylds[C::OBS + i], ov = ylds[2 * C::OBS + i];
                    glm_link_rich<FAM>(eta[r] + ov, cv, dv, want_u, rr, ut);
                    const bool on = ok && !(cv == 0.0 && dv == 0.0);  // weight 0: exactly nothing, whatever b() gave
                    res[r] = on ? rr : 0.0;
                    usum += on ? ut : 0.0;
                } else {
                    glm_link<FAM>(eta[r], ylds[bi * 16 + 4 * r + g], want_u, rr, ut);
                    res[r] = ok ? rr : 0.0;
                    usum += ok ? ut : 0.0;
                }
            }
            // g tiles += X_b^T . R_b: K-step r sums over the observations register r holds
#pragma unroll
            for (int r2 = 0; r2 < 2; ++r2)
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const v2f64 A = P2[(r2 * NT + t) * 64];
                    gacc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(A.x, res[2 * r2], gacc[t], 0, 0, 0);
                    gacc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(A.y, res[2 * r2 + 1], gacc[t], 0, 0, 0);
                }
        }
    }
}

// Waves per SIMD: two up to DP = 32, except the negative binomial at DP = 32 -- the constants of its exp, log and two
// series sit in vector registers beside the state (the scalar file is full), and held to 256 registers it spills; at DP
// = 128 it spills even with all 512 and is not instantiated (glm_build_disp refuses that shape).
// Likewise the non-centred logistic kernel at DP = 32: q, its scaled copy and the link's constants need 12 bytes of scratch
// at 256 registers.  The structured group priors (GLM_HIER_Q) keep the centred kernels' counts: all six build without scratch
// at them (profiles/glm_hier_penalty_resources.txt).
// The dispersion families with a hierarchical prior (centred and non-centred) need no case of their own: all twelve build without
// scratch at their families' counts (profiles/glm_hier_dispersion_resources.txt).
constexpr int glm_waves_per_simd(int NT, int fam, int hier) {
    return (NT <= 2 && !(NT == 2 && (fam == PBBI_GLM_NEGBINOMIAL || (hier == GLM_HIER_NC && fam == PBBI_GLM_LOGISTIC)))) ? 2 : 1;
}
// TWIN: k_glm_softmax of kernels_glm_softmax.hip restates this frame (ghost waves and ragged tail, momentum first, the
// kick / drift schedule of the evaluation loop, the five modes, the accept epilogue).  A fix to either belongs in both.
template <int NT, int FAM, bool RICH, int HIER = GLM_HIER_NONE>
__global__ void __launch_bounds__(BLOCK, glm_waves_per_simd(NT, FAM, HIER)) k_glm(typename GlmArgs<FAM, RICH, HIER>::type prm) {
    static_assert(RICH || !glm_disp(FAM), "the dispersion families live on the full model's frame");
    static_assert(HIER == GLM_HIER_NONE || RICH, "the hierarchical prior lives on the full model's frame");
    static_assert(HIER != GLM_HIER_Q || !glm_disp(FAM), "structured group priors: logistic and poisson only");
    using C = GlmCfg<NT>;
    constexpr int KS = C::KS;
    constexpr int DP = 16 * NT;
    __shared__ __attribute__((aligned(16))) v2f64 lds[C::CHV];
    __shared__ double ylds[(RICH ? 3 : 1) * C::CB * 16];
    constexpr bool HAS_NJ = HIER == GLM_HIER_CENTRED || HIER == GLM_HIER_Q;
    // RICH: {lam, mu} of each row (else unused); centred HIER: then {n_j, 0}; HIER_Q: then the penalty's fragments (8 DP^2 bytes)
    __shared__ __attribute__((aligned(16))) v2f64 plds[RICH ? DP + (HAS_NJ ? 4 : 0) + (HIER == GLM_HIER_Q ? DP * DP / 2 : 0) : 1];
    if constexpr (RICH) {
        for (int i = threadIdx.x; i < DP; i += BLOCK) plds[i] = v2f64{prm.prior[i], prm.prior[DP + i]};
        if constexpr (HAS_NJ)
            if (threadIdx.x < 4) plds[DP + threadIdx.x] = v2f64{prm.prior[2 * DP + threadIdx.x], 0.0};
        if constexpr (HIER == GLM_HIER_Q) {
            const v2f64* __restrict__ qsrc = reinterpret_cast<const v2f64*>(prm.qimg);
            for (int i = threadIdx.x; i < DP * DP / 2; i += BLOCK) plds[DP + 4 + i] = qsrc[i];
        }
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4;
    const int c = lane & 15;
    const int D = prm.D;
    const int mode = prm.mode;

    // every wave takes part in the staging barriers: one past the end of the ensemble recomputes the last tile
    // with its stores masked
    int64_t n0 = ((int64_t)blockIdx.x * 4 + wave) * CHAINS_PER_WAVE;  // wave-uniform
    bool ghost = false;
    if (n0 >= prm.N) {
        ghost = true;
        n0 = (prm.N - 1) / CHAINS_PER_WAVE * CHAINS_PER_WAVE;
    }
    const int64_t left = prm.N - n0;
    const bool valid = !ghost && c < left;
    const int cc = c < left ? c : (int)left - 1;  // ragged tail: compute on a clamped chain
    const uint32_t ld_in = 8u * (uint32_t)prm.ldn_in, ld_out = 8u * (uint32_t)prm.ldn_out;
    const uint32_t vin = (uint32_t)g * ld_in + 8u * (uint32_t)cc, s4in = 4u * ld_in;
    const uint32_t vout = (uint32_t)g * ld_out + 8u * (uint32_t)cc, s4out = 4u * ld_out;
    const __amdgpu_buffer_rsrc_t qin = rows_of<false>(prm.q_in, n0, D, prm.ldn_in, prm.N);
    const __amdgpu_buffer_rsrc_t pin = rows_of<false>(prm.p_in, n0, D, prm.ldn_in, prm.N);
    const __amdgpu_buffer_rsrc_t qout = rows_of<false>(prm.q_out, n0, D, prm.ldn_out, prm.N);
    const __amdgpu_buffer_rsrc_t pout = rows_of<false>(prm.p_out, n0, D, prm.ldn_out, prm.N);
    const bool have_pout = (prm.p_out != nullptr);
    const double m = prm.mass ? prm.mass[n0 + cc] : 1.0;
    const double minv = prm.mass ? 1.0 / m : 1.0;
    const bool traj = (mode == GLM_HMC || mode == GLM_INTEGRATE);
    const bool rng = (mode == GLM_HMC) && prm.rng;
    const uint64_t chain = prm.chain0 + (uint64_t)(n0 + cc);

    double q[KS], vh[KS];
    v4f64 gacc[NT];
    // ---- momentum first (vh holds p until the division by the mass below)
    double u = 0.0;
    if (rng) {
        const double pstd = sqrt(m * prm.kT);  // src/ensemble.py:88
#pragma unroll
        for (int k = 0; k < NT; ++k) {  // block k: rows 16k + 4*slot + g
            double z[4];
            rng_normal4d(prm.seed, PBBI_STREAM_MOMENTUM, prm.iter, chain, (uint32_t)((k << 2) | g),
                         (prm.flags & PBBI_DRAW_F64) != 0, z);
#pragma unroll
            for (int sl = 0; sl < 4; ++sl) vh[4 * k + sl] = (16 * k + 4 * sl + g < D) ? z[sl] * pstd : 0.0;
        }
        u = rng_uniform(prm.seed, prm.iter, chain);
        if (have_pout && !(prm.flags & PBBI_COMPAT_P_FROM_OLDQ) && valid) {
            // non-compat: a rejected chain reports its drawn momentum; park the draw now
#pragma unroll
            for (int s = 0; s < KS; ++s) store_row(pout, vout, s4out, s, vh[s]);
        }
    } else if (mode != GLM_EVAL) {
#pragma unroll
        for (int s = 0; s < KS; ++s) vh[s] = load_row(pin, vin, s4in, s);
        if (mode == GLM_HMC) u = prm.u_in[n0 + cc];
    } else {
#pragma unroll
        for (int s = 0; s < KS; ++s) vh[s] = 0.0;
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) q[s] = load_row(qin, vin, s4in, s);
    double pp_old = 0.0;
#pragma unroll
    for (int s = 0; s < KS; ++s) pp_old = fma(vh[s], vh[s], pp_old);
    if (traj) {
#pragma unroll
        for (int s = 0; s < KS; ++s) vh[s] *= minv;  // v = p/m
    }

    // ---- the trajectory as a list of gradient evaluations, each followed by a kick of ck and a drift of hd:
    //   Leapfrog        e = 0: h/2, h    e = 1 .. L-1: h, h    e = L: h/2, 0          (L = 0: one evaluation, no update)
    //   Stormer-Verlet  e = 0: h/2, h    e = 1 .. L:   h, h    e = L+1 (HMC only): 0, 0 -- U at the last position;
    //                   (q_{n+1} - q_n)/h = vh is the velocity it returns (src/integrator.py:142-163)
    const bool sv = prm.method == PBBI_STORMER_VERLET;
    const int L = prm.L;
    int nev = 1;
    if (traj) nev = sv ? L + 1 + (mode == GLM_HMC ? 1 : 0) : L + 1;
    const double lam = prm.lam;
    const double h = prm.h;
    double U_old = 0.0, U_new = 0.0;
    [[maybe_unused]] double htau[4];  // centred HIER, HIER_Q: tau_j = exp(-2 t_j) of the evaluation in hand (its store follows the loop)
    for (int e = 0; e < nev; ++e) {
        double ck = 0.0, hd = 0.0;
        if (traj) {
            if (sv) {
                if (e <= L) { ck = e == 0 ? 0.5 * h : h; hd = h; }
            } else if (L >= 1) {
                ck = (e == 0 || e == L) ? 0.5 * h : h;
                hd = e < L ? h : 0.0;
            }
        }
        ck *= minv;
        const bool want_u = (e == 0 || e == nev - 1) && mode != GLM_INTEGRATE;
        double usum;
        // the dispersion families: theta to every lane of the chain and what is formed from it, before the likelihood walk
        [[maybe_unused]] int ts = -1, tg = 0;
        [[maybe_unused]] GlmDispChain dk{};
        [[maybe_unused]] double tsum = 0.0;
        if constexpr (glm_disp(FAM)) {
            // theta: the owner of its row contributes q[s], everybody else 0 (exact); held: from the arguments
            ts = prm.trow >> 2, tg = prm.trow & 3;  // trow = -1: no s matches
            double th = 0.0;
#pragma unroll
            for (int s = 0; s < KS; ++s) th = (s == ts) ? q[s] : th;
            th = chain_sum(g == tg ? th : 0.0);
            if (prm.trow < 0) th = prm.theta;
            dk = glm_disp_chain<FAM>(th, want_u);
        }
        if constexpr (HIER == GLM_HIER_NC) {
            // The chain holds z_d on a grouped row: w_d = mu_d + sig_j z_d is what the likelihood sees.  The t_j reach
            // every lane of the chain as below (the owner contributes, the others add exact zeros); weff, the B operand
            // of the first product, is a scaled COPY of the state -- q itself is what the drift, the stores and the prior
            // work on, and scaling in place and back is not exact.
            const int jo = (g - prm.trow0) & 3;
            const int so = (prm.trow0 + jo) >> 2;
            double th = 0.0;
#pragma unroll
            for (int s = 0; s < KS; ++s) th = (s == so) ? q[s] : th;
            double sig[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sig[j] = 1.0;
                if (j < prm.J) sig[j] = exp(chain_sum(jo == j ? th : 0.0));
            }
            double weff[KS];
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const v2f64 pm = plds[4 * s + g];
                weff[s] = (pm.x < 0.0) ? fma(glm_hier_lam(pm.x, sig), q[s], pm.y) : q[s];
            }
            glm_grad<NT, FAM, RICH, HIER>(prm, lds, ylds, lane, g, weff, gacc, usum, want_u, dk, tsum);
            // dU/dt_j = sig_j sum_{d in j} gL_d z_d (this lane's rows here, the chain's below) goes to the owner's
            // register; dU/dz_d = sig_j gL_d (the priors' parts come with the rows below)
            double G[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const v2f64 pm = plds[4 * s + g];
                const double gz = gacc[s >> 2][s & 3] * q[s];
#pragma unroll
                for (int j = 0; j < 4; ++j) G[j] += (pm.x == -(double)(j + 1)) ? gz : 0.0;
            }
            double gown = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < prm.J) {
                    const double gt = chain_sum(G[j]) * sig[j];
                    gown = (jo == j) ? gt : gown;
                }
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double lx = plds[4 * (4 * t + r) + g].x;
                    const double gs = (lx < 0.0) ? gacc[t][r] * glm_hier_lam(lx, sig) : gacc[t][r];
                    gacc[t][r] = gs + ((4 * t + r == so) ? gown : 0.0);
                }
        } else {
            glm_grad<NT, FAM, RICH, HIER>(prm, lds, ylds, lane, g, q, gacc, usum, want_u, dk, tsum);
        }
        if constexpr (glm_disp(FAM)) {
            // dU/dtheta's likelihood part at theta's owner -- after the non-centred branch has read and scaled gacc
            tsum = chain_sum(tsum);
            tsum = (g == tg) ? tsum : 0.0;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) gacc[t][r] += (4 * t + r == ts) ? tsum : 0.0;
        }
        [[maybe_unused]] double hnt = 0.0;  // centred HIER: sum_j n_j t_j; HIER_Q: sum_j r_j t_j
        if constexpr (HIER == GLM_HIER_CENTRED) {
            // The t rows are J <= 4 consecutive rows, so a lane (rows 4s + g) owns at most one: row trow0 + jo, register
            // so.  It contributes that q to the chain sum of t_jo and 0 to the others' (exact); every lane of the chain
            // then has t_j and forms tau_j.  Groups past J stay at t = 0, S = 0 and meet no row.
            const int jo = (g - prm.trow0) & 3;
            const int so = (prm.trow0 + jo) >> 2;
            // S_j = sum over the members of group j of (w - mu)^2: this lane's rows here, the chain's below
            double S[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const v2f64 pm = plds[4 * s + g];
                const double dq = q[s] - pm.y;
                const double dq2 = dq * dq;
#pragma unroll
                for (int j = 0; j < 4; ++j) S[j] += (pm.x == -(double)(j + 1)) ? dq2 : 0.0;
            }
            double th = 0.0;
#pragma unroll
            for (int s = 0; s < KS; ++s) th = (s == so) ? q[s] : th;
            // dU/dt_j = n_j - tau_j S_j (the t prior's part comes with the row's {lam, mu} like any fixed row's)
            double gown = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                htau[j] = 1.0;
                if (j < prm.J) {
                    const double tj = chain_sum(jo == j ? th : 0.0);
                    const double nj = plds[DP + j].x;
                    htau[j] = exp(-2.0 * tj);
                    const double gt = nj - htau[j] * chain_sum(S[j]);
                    gown = (jo == j) ? gt : gown;
                    hnt = fma(nj, tj, hnt);
                }
            }
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) gacc[t][r] += (4 * t + r == so) ? gown : 0.0;
        }
        [[maybe_unused]] double hqs = 0.0;  // HIER_Q: sum_j tau_j S_j, S_j = d_j^T Q_j d_j
        if constexpr (HIER == GLM_HIER_Q) {
            // t_j to every lane of the chain and tau_j, as in the centred branch -- before the product, whose rows want tau
            const int jo = (g - prm.trow0) & 3;
            const int so = (prm.trow0 + jo) >> 2;
            double th = 0.0;
#pragma unroll
            for (int s = 0; s < KS; ++s) th = (s == so) ? q[s] : th;
            double tj[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                htau[j] = 1.0;
                tj[j] = 0.0;
                if (j < prm.J) {
                    tj[j] = chain_sum(jo == j ? th : 0.0);
                    htau[j] = exp(-2.0 * tj[j]);
                }
            }
            // the B operand: w - mu on member rows, an exact 0 SELECTED everywhere else (fixed, t and padding rows)
            double dq[KS];
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const v2f64 pm = plds[4 * s + g];
                dq[s] = (pm.x < 0.0) ? q[s] - pm.y : 0.0;
            }
            // Q dq tile by tile: register r of tile t is row 16t + 4r + g of this lane's chain.  Consumed at once: the
            // lane's share of S_j and tau_j (Q dq) into the gradient of member rows.
            const v2f64* __restrict__ QA = plds + (DP + 4) + lane;
            double S[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                v4f64 qd = v4f64{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int s2 = 0; s2 < KS / 2; ++s2) {
                    const v2f64 A = QA[(t * (KS / 2) + s2) * 64];
                    qd = __builtin_amdgcn_mfma_f64_16x16x4f64(A.x, dq[2 * s2], qd, 0, 0, 0);
                    qd = __builtin_amdgcn_mfma_f64_16x16x4f64(A.y, dq[2 * s2 + 1], qd, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double lx = plds[4 * (4 * t + r) + g].x;
                    const double dqd = dq[4 * t + r] * qd[r];
#pragma unroll
                    for (int j = 0; j < 4; ++j) S[j] += (lx == -(double)(j + 1)) ? dqd : 0.0;
                    gacc[t][r] = (lx < 0.0) ? fma(glm_hier_lam(lx, htau), qd[r], gacc[t][r]) : gacc[t][r];
                }
            }
            // dU/dt_j = r_j - tau_j S_j (the t prior's part comes with the row's {lam, mu})
            double gown = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < prm.J) {
                    const double Sj = chain_sum(S[j]);
                    const double rj = plds[DP + j].x;
                    const double gt = rj - htau[j] * Sj;
                    gown = (jo == j) ? gt : gown;
                    hnt = fma(rj, tj[j], hnt);
                    hqs = fma(htau[j], Sj, hqs);
                }
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) gacc[t][r] += (4 * t + r == so) ? gown : 0.0;
        }
        if (want_u) {
            double qq = 0.0;
            if constexpr (HIER == GLM_HIER_NC) {
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    const v2f64 pm = glm_nc_prior(plds[4 * s + g]);
                    const double dq = q[s] - pm.y;
                    qq = fma(pm.x * dq, dq, qq);
                }
                U_new = chain_sum(usum) + 0.5 * chain_sum(qq);  // no n_j t_j: the Jacobian of w -> z took it
            } else if constexpr (HIER == GLM_HIER_CENTRED) {
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    const v2f64 pm = plds[4 * s + g];
                    const double dq = q[s] - pm.y;
                    qq = fma(glm_hier_lam(pm.x, htau) * dq, dq, qq);
                }
                U_new = (chain_sum(usum) + 0.5 * chain_sum(qq)) + hnt;
            } else if constexpr (HIER == GLM_HIER_Q) {
#pragma unroll
                for (int s = 0; s < KS; ++s) {  // fixed and t rows; the members' quadratic forms are in hqs
                    const v2f64 pm = plds[4 * s + g];
                    const double dq = q[s] - pm.y;
                    qq = (pm.x < 0.0) ? qq : fma(pm.x * dq, dq, qq);
                }
                U_new = (chain_sum(usum) + 0.5 * (chain_sum(qq) + hqs)) + hnt;
            } else if constexpr (RICH) {
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    const v2f64 pm = plds[4 * s + g];
                    const double dq = q[s] - pm.y;
                    qq = fma(pm.x * dq, dq, qq);
                }
                U_new = chain_sum(usum) + 0.5 * chain_sum(qq);
            } else {
#pragma unroll
                for (int s = 0; s < KS; ++s) qq = fma(q[s], q[s], qq);
                U_new = chain_sum(usum) + (0.5 * lam) * chain_sum(qq);
            }
            if (e == 0) U_old = U_new;
        }
        if (mode == GLM_EVAL) break;  // the gradient stays in gacc
        // an evaluation for U alone is followed by no update (a product 0 * inf would turn an overflowed
        // gradient, whose energy rejects the proposal, into a NaN momentum)
        if (!(traj && (sv ? e <= L : L >= 1))) continue;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int s = 4 * t + r;
                double gt;
                if constexpr (HIER == GLM_HIER_NC) {
                    const v2f64 pm = glm_nc_prior(plds[4 * s + g]);
                    gt = fma(pm.x, q[s] - pm.y, gacc[t][r]);
                } else if constexpr (HIER == GLM_HIER_CENTRED) {
                    const v2f64 pm = plds[4 * s + g];
                    gt = fma(glm_hier_lam(pm.x, htau), q[s] - pm.y, gacc[t][r]);
                } else if constexpr (HIER == GLM_HIER_Q) {
                    const v2f64 pm = plds[4 * s + g];  // a member's prior part is in gacc already
                    gt = (pm.x < 0.0) ? gacc[t][r] : fma(pm.x, q[s] - pm.y, gacc[t][r]);
                } else if constexpr (RICH) {
                    const v2f64 pm = plds[4 * s + g];
                    gt = fma(pm.x, q[s] - pm.y, gacc[t][r]);
                } else {
                    gt = fma(lam, q[s], gacc[t][r]);
                }
                vh[s] = fma(-gt, ck, vh[s]);
                q[s] = fma(vh[s], hd, q[s]);
            }
    }

    if (mode == GLM_EVAL) {
        if (prm.grad_out && valid) {
            const __amdgpu_buffer_rsrc_t gout = rows_of<false>(prm.grad_out, n0, D, prm.ldn_out, prm.N);
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int s = 4 * t + r;
                    double gt;
                    if constexpr (HIER == GLM_HIER_NC) {
                        const v2f64 pm = glm_nc_prior(plds[4 * s + g]);
                        gt = fma(pm.x, q[s] - pm.y, gacc[t][r]);
                    } else if constexpr (HIER == GLM_HIER_CENTRED) {
                        const v2f64 pm = plds[4 * s + g];
                        gt = fma(glm_hier_lam(pm.x, htau), q[s] - pm.y, gacc[t][r]);
                    } else if constexpr (HIER == GLM_HIER_Q) {
                        const v2f64 pm = plds[4 * s + g];
                        gt = (pm.x < 0.0) ? gacc[t][r] : fma(pm.x, q[s] - pm.y, gacc[t][r]);
                    } else if constexpr (RICH) {
                        const v2f64 pm = plds[4 * s + g];
                        gt = fma(pm.x, q[s] - pm.y, gacc[t][r]);
                    } else {
                        gt = fma(lam, q[s], gacc[t][r]);
                    }
                    store_row(gout, vout, s4out, s, gt);
                }
        }
        if (prm.U_out && valid && g == 0) prm.U_out[n0 + c] = U_old;
        return;
    }
    if (mode == GLM_ENERGY || mode == GLM_RATIO) {
        const double H = 0.5 * chain_sum(pp_old) / m + U_old;
        if (valid && g == 0) {
            if (mode == GLM_ENERGY) {
                if (prm.U_out) prm.U_out[n0 + c] = H;
                if (prm.w_out) prm.w_out[n0 + c] = exp(-H);
            } else {
                prm.U_out[n0 + c] = exp(prm.U_out[n0 + c] - H);
            }
        }
        return;
    }
    if (mode == GLM_INTEGRATE) {  // in place q, p; optional Integrator.v
        if (valid) {
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                store_row(qout, vout, s4out, s, q[s]);
                store_row(pout, vout, s4out, s, prm.mass ? vh[s] * m : vh[s]);
            }
            if (prm.v_out) {
                const __amdgpu_buffer_rsrc_t vo = rows_of<false>(prm.v_out, n0, D, prm.ldn_out, prm.N);
#pragma unroll
                for (int s = 0; s < KS; ++s) store_row(vo, vout, s4out, s, vh[s]);
            }
        }
        return;
    }

    // ---- energies, ratio, decision (src/HMC.py:109-115,166-173)
    double pp_new = 0.0;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        if (prm.mass) vh[s] *= m;  // p = v*m; vh now holds p
        pp_new = fma(vh[s], vh[s], pp_new);
    }
    const double oldH = 0.5 * chain_sum(pp_old) / m + U_old;
    const double newH = 0.5 * chain_sum(pp_new) / m + U_new;
    const double ratio = exp((oldH - newH) * pbbi_accept_beta(prm.flags, prm.kT));
    const bool reject = metropolis_reject(ratio, u);
    const bool compat = (prm.flags & PBBI_COMPAT_P_FROM_OLDQ) != 0;
    bool store_p = have_pout;
    if (reject) {  // fetch the old point again instead of keeping it live through the trajectory
#pragma unroll
        for (int s = 0; s < KS; ++s) q[s] = load_row(qin, vin, s4in, s);  // :175
        if (compat) {  // :176  p <- oldQ
#pragma unroll
            for (int s = 0; s < KS; ++s) vh[s] = q[s];
        } else if (rng) {
            store_p = false;  // the parked draw stays
        } else if (have_pout) {
#pragma unroll
            for (int s = 0; s < KS; ++s) vh[s] = load_row(pin, vin, s4in, s);
        }
    }
    if (valid) {
#pragma unroll
        for (int s = 0; s < KS; ++s) store_row(qout, vout, s4out, s, q[s]);  // :178
        if (store_p) {
#pragma unroll
            for (int s = 0; s < KS; ++s) store_row(pout, vout, s4out, s, vh[s]);  // :179
        }
    }
    if (valid && g == 0) {
        if (prm.ratio_out) prm.ratio_out[n0 + c] = ratio;
        if (prm.reject_out) prm.reject_out[n0 + c] = reject ? 1 : 0;
    }
}

int glm_check(const pbbi_potential* pot, int64_t ld) {
    if (pot->dtype != PBBI_F64 || pot->glm_DP == 0 || !pot->d_glm_img)
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, "GLM kernels: fp64, D <= 128");
    if ((int64_t)pot->glm_DP * ld >= ((int64_t)1 << 29))
        return pbbi_fail(PBBI_ERR_UNSUPPORTED,
                         "GLM kernels address a lane's rows with 32-bit offsets: padded D * leading stride must "
                         "be < 2^29 elements; shard the ensemble");
    return PBBI_OK;
}

GlmPrm glm_prm(const pbbi_potential* pot) {
    GlmPrm prm{};
    prm.img = (const double*)pot->d_glm_img;
    prm.y = (const double*)pot->d_glm_y;
    prm.M = pot->glm_M;
    prm.nb = (int)((pot->glm_M + 15) / 16);
    prm.lam = pot->glm_lam;
    prm.D = pot->D;
    prm.kT = 1.0;
    return prm;
}

int glm_launch(const pbbi_potential* pot, const GlmPrm& prm, hipStream_t stream) {
    const dim3 grid((unsigned)((prm.N + CHAINS_PER_WG - 1) / CHAINS_PER_WG)), block(BLOCK);
    const bool rich = pot->d_glm_obs != nullptr;  // handle of pbbi_potential_create_glm_ex
    GlmPrmRich rprm{};
    static_cast<GlmPrm&>(rprm) = prm;
    rprm.obs = (const double*)pot->d_glm_obs;
    rprm.prior = (const double*)pot->d_glm_prior;
    rprm.obs_stride = glm_blocks_padded(pot->glm_M) * 16;
    const bool disp = glm_disp(pot->glm_family);  // handle of pbbi_potential_create_glm_dispersion or _glm_hier_dispersion
    const bool hd = disp && pot->glm_hier_J > 0;  // ... the latter
    GlmPrmDisp dprm{};
    static_cast<GlmPrmRich&>(dprm) = rprm;
    dprm.theta = pot->glm_theta;
    dprm.trow = pot->glm_trow;
    if (disp && pot->glm_family == PBBI_GLM_NEGBINOMIAL && pot->glm_DP > 64)
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, "negbinomial: no kernel at a padded state dimension of 128 (internal)");
#define GLM_DISP_CASE(NT_, FAM_)                                                                            \
    if (disp && !hd && pot->glm_DP == 16 * NT_ && pot->glm_family == FAM_)                                  \
        hipLaunchKernelGGL((k_glm<NT_, FAM_, true>), grid, block, 0, stream, dprm);
    GLM_DISP_CASE(1, PBBI_GLM_GAUSSIAN) GLM_DISP_CASE(2, PBBI_GLM_GAUSSIAN) GLM_DISP_CASE(4, PBBI_GLM_GAUSSIAN)
    GLM_DISP_CASE(8, PBBI_GLM_GAUSSIAN)
    GLM_DISP_CASE(1, PBBI_GLM_NEGBINOMIAL) GLM_DISP_CASE(2, PBBI_GLM_NEGBINOMIAL) GLM_DISP_CASE(4, PBBI_GLM_NEGBINOMIAL)
#undef GLM_DISP_CASE
    const bool nc = pot->glm_hier_J > 0 && pot->glm_hier_nc && !hd;  // handle of pbbi_potential_create_glm_hier_ex, non-centred
    const bool hq = pot->glm_hier_J > 0 && pot->d_glm_qimg;   // handle of pbbi_potential_create_glm_hier_q
    const bool hier = pot->glm_hier_J > 0 && !nc && !hq && !hd;  // handle of pbbi_potential_create_glm_hier
    GlmPrmHier hprm{};
    static_cast<GlmPrmRich&>(hprm) = rprm;
    hprm.trow0 = pot->D - pot->glm_hier_J - (hd && pot->glm_trow >= 0 ? 1 : 0);  // a sampled theta is the last row, behind the t rows
    hprm.J = pot->glm_hier_J;
    if (hier && pot->glm_DP > glm_hier_max_dim(pot->glm_family))
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, "hierarchical prior: no kernel at this padded state dimension (internal)");
#define GLM_HIER_CASE(NT_, FAM_)                                                                            \
    if (hier && pot->glm_DP == 16 * NT_ && pot->glm_family == FAM_)                                         \
        hipLaunchKernelGGL((k_glm<NT_, FAM_, true, GLM_HIER_CENTRED>), grid, block, 0, stream, hprm);
    GLM_HIER_CASE(1, PBBI_GLM_LOGISTIC) GLM_HIER_CASE(2, PBBI_GLM_LOGISTIC) GLM_HIER_CASE(4, PBBI_GLM_LOGISTIC)
    GLM_HIER_CASE(1, PBBI_GLM_POISSON) GLM_HIER_CASE(2, PBBI_GLM_POISSON) GLM_HIER_CASE(4, PBBI_GLM_POISSON)
#undef GLM_HIER_CASE
    if (nc && pot->glm_DP > glm_hier_nc_max_dim(pot->glm_family))
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, "non-centred hierarchical prior: no kernel at this padded state dimension (internal)");
#define GLM_NC_CASE(NT_, FAM_)                                                                              \
    if (nc && pot->glm_DP == 16 * NT_ && pot->glm_family == FAM_)                                           \
        hipLaunchKernelGGL((k_glm<NT_, FAM_, true, GLM_HIER_NC>), grid, block, 0, stream, hprm);
    GLM_NC_CASE(1, PBBI_GLM_LOGISTIC) GLM_NC_CASE(2, PBBI_GLM_LOGISTIC) GLM_NC_CASE(4, PBBI_GLM_LOGISTIC)
    GLM_NC_CASE(1, PBBI_GLM_POISSON) GLM_NC_CASE(2, PBBI_GLM_POISSON) GLM_NC_CASE(4, PBBI_GLM_POISSON)
#undef GLM_NC_CASE
    GlmPrmHierQ qprm{};
    static_cast<GlmPrmHier&>(qprm) = hprm;
    qprm.qimg = (const double*)pot->d_glm_qimg;
    if (hq && pot->glm_DP > glm_hier_q_max_dim(pot->glm_family))
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, "structured group priors: no kernel at this padded state dimension (internal)");
#define GLM_HQ_CASE(NT_, FAM_)                                                                              \
    if (hq && pot->glm_DP == 16 * NT_ && pot->glm_family == FAM_)                                           \
        hipLaunchKernelGGL((k_glm<NT_, FAM_, true, GLM_HIER_Q>), grid, block, 0, stream, qprm);
    GLM_HQ_CASE(1, PBBI_GLM_LOGISTIC) GLM_HQ_CASE(2, PBBI_GLM_LOGISTIC) GLM_HQ_CASE(4, PBBI_GLM_LOGISTIC)
    GLM_HQ_CASE(1, PBBI_GLM_POISSON) GLM_HQ_CASE(2, PBBI_GLM_POISSON) GLM_HQ_CASE(4, PBBI_GLM_POISSON)
#undef GLM_HQ_CASE
    GlmPrmHierDisp hdprm{};
    static_cast<GlmPrmHier&>(hdprm) = hprm;
    hdprm.theta = pot->glm_theta;
    hdprm.trow = pot->glm_trow;
    if (hd && pot->glm_DP > glm_hier_disp_max_dim(pot->glm_family, pot->glm_hier_nc ? PBBI_HIER_NONCENTRED : PBBI_HIER_CENTRED))
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, "random effects for the dispersion families: no kernel at this padded state dimension (internal)");
#define GLM_HD_CASE(NT_, FAM_)                                                                              \
    if (hd && pot->glm_DP == 16 * NT_ && pot->glm_family == FAM_) {                                         \
        if (pot->glm_hier_nc)                                                                               \
            hipLaunchKernelGGL((k_glm<NT_, FAM_, true, GLM_HIER_NC>), grid, block, 0, stream, hdprm);       \
        else                                                                                                \
            hipLaunchKernelGGL((k_glm<NT_, FAM_, true, GLM_HIER_CENTRED>), grid, block, 0, stream, hdprm);  \
    }
    GLM_HD_CASE(1, PBBI_GLM_GAUSSIAN) GLM_HD_CASE(2, PBBI_GLM_GAUSSIAN) GLM_HD_CASE(4, PBBI_GLM_GAUSSIAN)
    GLM_HD_CASE(1, PBBI_GLM_NEGBINOMIAL) GLM_HD_CASE(2, PBBI_GLM_NEGBINOMIAL) GLM_HD_CASE(4, PBBI_GLM_NEGBINOMIAL)
#undef GLM_HD_CASE
#define GLM_CASE(NT_, RICH_, PRM_)                                                                          \
    if (!disp && !hier && !nc && !hq && pot->glm_DP == 16 * NT_ && rich == RICH_) {                                \
        if (pot->glm_family == PBBI_GLM_LOGISTIC)                                                           \
            hipLaunchKernelGGL((k_glm<NT_, PBBI_GLM_LOGISTIC, RICH_>), grid, block, 0, stream, PRM_);       \
        else                                                                                                \
            hipLaunchKernelGGL((k_glm<NT_, PBBI_GLM_POISSON, RICH_>), grid, block, 0, stream, PRM_);        \
    }
    GLM_CASE(1, false, prm) GLM_CASE(2, false, prm) GLM_CASE(4, false, prm) GLM_CASE(8, false, prm)
    GLM_CASE(1, true, rprm) GLM_CASE(2, true, rprm) GLM_CASE(4, true, rprm) GLM_CASE(8, true, rprm)
#undef GLM_CASE
    PBBI_HIP(hipGetLastError());
    return PBBI_OK;
}

}  // namespace

// ---- host side: the fragment image of X ------------------------------------------------------------------
int glm_padded_dim(int D) { return D <= 16 ? 16 : D <= 32 ? 32 : D <= 64 ? 64 : 128; }
static int64_t glm_blocks_padded(int64_t M) { return ((M + 15) / 16 + 3) / 4 * 4; }
int64_t glm_image_len(int D, int64_t M) { return glm_blocks_padded(M) * (int64_t)glm_padded_dim(D) * 32; }

// X (M x D, row-major) -> per block of 16 observations P1 [KS/2][64][2] then P2 [2][NT][64][2] (see the top of
// the file), zero padded to DP columns and to a multiple of 4 blocks.  Host only.
static void glm_pack_dp(int D, int DP, int64_t M, const double* X, double* out);
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
// ... at a padded dimension DP >= D of the caller's: the image of [X | 0]
static void glm_pack_dp(int D, int DP, int64_t M, const double* X, double* out) {
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

int glm_build(pbbi_potential* pot, int64_t M, const double* X, const double* y, int family, double lam) {
    const int D = pot->D;
    if (D > 128 || pot->dtype != PBBI_F64)
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, "GLM potentials run on the fp64 matrix-core kernels: float64 and "
                                               "D <= 128 only (D = " + std::to_string(D) + ")");
    std::vector<double> img((size_t)glm_image_len(D, M));
    glm_pack(D, M, X, img.data());
    std::vector<double> yp((size_t)glm_blocks_padded(M) * 16, 0.0);
    std::memcpy(yp.data(), y, sizeof(double) * (size_t)M);
    PBBI_HIP(hipMalloc(&pot->d_glm_img, img.size() * sizeof(double)));
    PBBI_HIP(hipMalloc(&pot->d_glm_y, yp.size() * sizeof(double)));
    PBBI_HIP(hipMemcpy(pot->d_glm_img, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice));
    PBBI_HIP(hipMemcpy(pot->d_glm_y, yp.data(), yp.size() * sizeof(double), hipMemcpyHostToDevice));
    pot->glm_DP = glm_padded_dim(D);
    pot->glm_M = M;
    pot->glm_family = family;
    pot->glm_lam = lam;
    return PBBI_OK;
}

// ---- host side: the full model's observation streams and prior vectors ------------------------------------
int64_t glm_obs_len(int64_t M) { return 3 * glm_blocks_padded(M) * 16; }

// Every rule of the full model's per-observation arguments (NULL = the default: weights 1, offset 0, trials 1).
int glm_check_obs(int64_t M, int family, const double* y, const double* weights, const double* offset,
                  const double* trials) {
    if (M < 1) return pbbi_fail(PBBI_ERR_INVALID, "M must be >= 1");
    if (family != PBBI_GLM_LOGISTIC && family != PBBI_GLM_POISSON)
        return pbbi_fail(PBBI_ERR_INVALID, "unknown GLM family");
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

// c = a n | d = a y | o, each zero padded to the image's block count (glm_obs_len(M) doubles).  Host only.
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

// the caller has run glm_check_obs and glm_check_prior
int glm_build_ex(pbbi_potential* pot, int64_t M, const double* X, const double* y, int family, const double* weights,
                 const double* offset, const double* trials, const double* lam, const double* mu) {
    const int D = pot->D;
    if (D > 128 || pot->dtype != PBBI_F64)
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, "GLM potentials run on the fp64 matrix-core kernels: float64 and "
                                               "D <= 128 only (D = " + std::to_string(D) + ")");
    const int DP = glm_padded_dim(D);
    std::vector<double> img((size_t)glm_image_len(D, M));
    glm_pack(D, M, X, img.data());
    std::vector<double> obs((size_t)glm_obs_len(M));
    glm_pack_obs(M, y, weights, offset, trials, obs.data());
    std::vector<double> prior((size_t)2 * DP, 0.0);  // lam | mu, zeros past D
    bool flat = true, centred = true, one = true;
    for (int d = 0; d < D; ++d) {
        prior[d] = lam[d];
        prior[DP + d] = mu ? mu[d] : 0.0;
        flat = flat && lam[d] == 0.0;
        one = one && lam[d] == lam[0];
        centred = centred && prior[DP + d] == 0.0;
    }
    PBBI_HIP(hipMalloc(&pot->d_glm_img, img.size() * sizeof(double)));
    PBBI_HIP(hipMalloc(&pot->d_glm_obs, obs.size() * sizeof(double)));
    PBBI_HIP(hipMalloc(&pot->d_glm_prior, prior.size() * sizeof(double)));
    PBBI_HIP(hipMemcpy(pot->d_glm_img, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice));
    PBBI_HIP(hipMemcpy(pot->d_glm_obs, obs.data(), obs.size() * sizeof(double), hipMemcpyHostToDevice));
    PBBI_HIP(hipMemcpy(pot->d_glm_prior, prior.data(), prior.size() * sizeof(double), hipMemcpyHostToDevice));
    pot->glm_DP = DP;
    pot->glm_M = M;
    pot->glm_family = family;
    pot->glm_lam = one ? lam[0] : 0.0;  // (the full model's kernels read d_glm_prior)
    pot->glm_terms = (weights ? GLM_TERM_WEIGHTS : 0) | (offset ? GLM_TERM_OFFSET : 0) | (trials ? GLM_TERM_TRIALS : 0) |
                     (one ? 0 : GLM_TERM_PRIOR_VECTOR) | (centred ? 0 : GLM_TERM_PRIOR_MEAN) | (flat ? GLM_TERM_PRIOR_FLAT : 0);
    return PBBI_OK;
}

// ---- host side: the dispersion families ------------------------------------------------------------------------
int glm_check_obs_disp(int64_t M, int family, const double* y, const double* weights, const double* offset) {
    if (M < 1) return pbbi_fail(PBBI_ERR_INVALID, "M must be >= 1");
    if (!glm_disp(family)) return pbbi_fail(PBBI_ERR_INVALID, "unknown dispersion family (gaussian = 3, negbinomial = 4)");
    if (!y) return pbbi_fail(PBBI_ERR_INVALID, "y is NULL");
    for (int64_t i = 0; i < M; ++i) {
        auto at = [i] { return " (observation " + std::to_string(i) + ")"; };
        if (!std::isfinite(y[i])) return pbbi_fail(PBBI_ERR_INVALID, "y must be finite" + at());
        if (family == PBBI_GLM_NEGBINOMIAL && (y[i] < 0.0 || y[i] != std::floor(y[i])))
            return pbbi_fail(PBBI_ERR_INVALID, "negbinomial: y must hold non-negative integers" + at());
        if (weights && !(std::isfinite(weights[i]) && weights[i] >= 0.0))
            return pbbi_fail(PBBI_ERR_INVALID, "weights must be finite and >= 0" + at());
        if (offset && !std::isfinite(offset[i]))
            return pbbi_fail(PBBI_ERR_INVALID, "offset must be finite" + at());
    }
    return PBBI_OK;
}

// c = a | d = y (raw) | o, each zero padded to the image's block count (glm_obs_len(M) doubles).  Host only.
void glm_pack_obs_disp(int64_t M, const double* y, const double* weights, const double* offset, double* out) {
    const int64_t len = glm_blocks_padded(M) * 16;
    std::memset(out, 0, sizeof(double) * (size_t)(3 * len));
    for (int64_t i = 0; i < M; ++i) {
        out[i] = weights ? weights[i] : 1.0;
        out[len + i] = y[i];
        out[2 * len + i] = offset ? offset[i] : 0.0;
    }
}

// the caller has run glm_check_obs_disp and glm_check_prior (over pot->D entries); pot->D = Dx + (sample ? 1 : 0)
int glm_build_disp(pbbi_potential* pot, int Dx, int64_t M, const double* X, const double* y, int family,
                   const double* weights, const double* offset, const double* lam, const double* mu, int sample,
                   double theta) {
    const int Dt = pot->D;
    if (Dt > 128 || pot->dtype != PBBI_F64)
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, "GLM potentials run on the fp64 matrix-core kernels: float64 and a state "
                                               "dimension <= 128 only (" + std::to_string(Dt) + ")");
    // k_glm<8, PBBI_GLM_NEGBINOMIAL, true> cannot be built without scratch (the full model's DP = 128 kernel already
    // fills all 512 registers) and is not shipped
    if (family == PBBI_GLM_NEGBINOMIAL && Dt > 64)
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, "negbinomial: the state dimension (coefficients + 1 for a sampled dispersion) "
                                               "must be <= 64: its kernel at 65 .. 128 does not fit the register file (" +
                                                   std::to_string(Dt) + ")");
    const int DP = glm_padded_dim(Dt);
    const int64_t nbp = glm_blocks_padded(M);
    std::vector<double> img((size_t)(nbp * DP * 32));
    glm_pack_dp(Dx, DP, M, X, img.data());  // [X | 0]: the theta row meets a zero column
    std::vector<double> obs((size_t)glm_obs_len(M));
    glm_pack_obs_disp(M, y, weights, offset, obs.data());
    std::vector<double> prior((size_t)2 * DP, 0.0);  // lam | mu over the Dt state rows, zeros past them
    for (int d = 0; d < Dt; ++d) {
        prior[d] = lam[d];
        prior[DP + d] = mu ? mu[d] : 0.0;
    }
    PBBI_HIP(hipMalloc(&pot->d_glm_img, img.size() * sizeof(double)));
    PBBI_HIP(hipMalloc(&pot->d_glm_obs, obs.size() * sizeof(double)));
    PBBI_HIP(hipMalloc(&pot->d_glm_prior, prior.size() * sizeof(double)));
    PBBI_HIP(hipMemcpy(pot->d_glm_img, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice));
    PBBI_HIP(hipMemcpy(pot->d_glm_obs, obs.data(), obs.size() * sizeof(double), hipMemcpyHostToDevice));
    PBBI_HIP(hipMemcpy(pot->d_glm_prior, prior.data(), prior.size() * sizeof(double), hipMemcpyHostToDevice));
    pot->glm_DP = DP;
    pot->glm_M = M;
    pot->glm_family = family;
    pot->glm_lam = 0.0;  // (these kernels read d_glm_prior)
    pot->glm_terms = (weights ? GLM_TERM_WEIGHTS : 0) | (offset ? GLM_TERM_OFFSET : 0);
    pot->glm_trow = sample ? Dx : -1;
    pot->glm_theta = sample ? 0.0 : theta;
    return PBBI_OK;
}

// ---- host side: the hierarchical prior -------------------------------------------------------------------------
// the largest state dimension (coefficients + groups) each family's hierarchical kernels serve: k_glm<8, FAM, true, GLM_HIER_CENTRED>
// cannot be built without scratch for either family (the full model's DP = 128 kernels already fill the register file;
// 172 and 180 bytes per lane) and is not shipped
int glm_hier_max_dim(int family) { return (family == PBBI_GLM_LOGISTIC || family == PBBI_GLM_POISSON) ? 64 : 0; }
// ... the non-centred kernels k_glm<NT, FAM, true, GLM_HIER_NC>: NT = 1, 2, 4 build without scratch for both families (the
// scaled copy of the state costs KS more registers beside q; profiles/glm_hier_nc_resources.txt)
int glm_hier_nc_max_dim(int family) { return (family == PBBI_GLM_LOGISTIC || family == PBBI_GLM_POISSON) ? 64 : 0; }

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
// of group j.  The caller has run glm_check_hier.  Host only.
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

// ---- host side: random effects for the dispersion families -----------------------------------------------------------
// The largest state dimension (coefficients + groups + 1 for a sampled dispersion) the kernels k_glm<NT, FAM, true, HIER> with
// FAM = gaussian / negbinomial and HIER = GLM_HIER_CENTRED / GLM_HIER_NC serve; 0 = nothing served.  An instantiation ships
// only if it builds without scratch: all twelve of NT = 1, 2, 4 do (profiles/glm_hier_dispersion_resources.txt).  There is no
// kernel at 128 rows for either parent's hierarchical form.
int glm_hier_disp_max_dim(int family, int parametrisation) {
    if (!glm_disp(family)) return 0;
    if (parametrisation != PBBI_HIER_CENTRED && parametrisation != PBBI_HIER_NONCENTRED) return 0;
    return 64;
}

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
// and glm_check_hier_disp_theta.  Host only.
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

// the caller has run glm_check_obs_disp, glm_check_hier and glm_check_hier_disp_theta; pot->D = Dx + J + (sample ? 1 : 0)
int glm_build_hier_disp(pbbi_potential* pot, int Dx, int64_t M, const double* X, const double* y, int family,
                        const double* weights, const double* offset, const double* lam, const double* mu,
                        const int32_t* groups, int J, const double* tprior, int parametrisation, int sample, double theta,
                        const double* dprior) {
    const int Dt = pot->D;
    const int dmax = glm_hier_disp_max_dim(family, parametrisation);
    if (pot->dtype != PBBI_F64 || Dt > dmax)
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, "random effects for the dispersion families: float64 and a state dimension "
                                               "(coefficients + groups + 1 for a sampled dispersion) <= " + std::to_string(dmax) +
                                                   " only (" + std::to_string(Dt) + ")");
    const int DP = glm_padded_dim(Dt);
    const int64_t nbp = glm_blocks_padded(M);
    std::vector<double> img((size_t)(nbp * DP * 32));
    glm_pack_dp(Dx, DP, M, X, img.data());  // [X | 0]: the t rows and the theta row meet zero columns
    std::vector<double> obs((size_t)glm_obs_len(M));
    glm_pack_obs_disp(M, y, weights, offset, obs.data());
    std::vector<double> prior((size_t)2 * DP + 4, 0.0);  // lam | mu | n_j
    double* nj = prior.data() + 2 * DP;
    glm_pack_prior_groups_disp(Dx, J, lam, mu, groups, tprior, sample, dprior, prior.data(), nj);
    for (int j = 0; j < 4; ++j) pot->glm_hier_n[j] = nj[j];
    PBBI_HIP(hipMalloc(&pot->d_glm_img, img.size() * sizeof(double)));
    PBBI_HIP(hipMalloc(&pot->d_glm_obs, obs.size() * sizeof(double)));
    PBBI_HIP(hipMalloc(&pot->d_glm_prior, prior.size() * sizeof(double)));
    PBBI_HIP(hipMemcpy(pot->d_glm_img, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice));
    PBBI_HIP(hipMemcpy(pot->d_glm_obs, obs.data(), obs.size() * sizeof(double), hipMemcpyHostToDevice));
    PBBI_HIP(hipMemcpy(pot->d_glm_prior, prior.data(), prior.size() * sizeof(double), hipMemcpyHostToDevice));
    pot->glm_DP = DP;
    pot->glm_M = M;
    pot->glm_family = family;
    pot->glm_lam = 0.0;  // (these kernels read d_glm_prior)
    pot->glm_terms = (weights ? GLM_TERM_WEIGHTS : 0) | (offset ? GLM_TERM_OFFSET : 0);
    pot->glm_hier_J = J;
    pot->glm_hier_nc = parametrisation == PBBI_HIER_NONCENTRED ? 1 : 0;
    pot->glm_trow = sample ? Dx + J : -1;
    pot->glm_theta = sample ? 0.0 : theta;
    return PBBI_OK;
}

// ---- host side: structured group priors ----------------------------------------------------------------------------
// the largest state dimension the kernels k_glm<NT, FAM, true, GLM_HIER_Q> serve: NT = 1, 2, 4 build without scratch for both
// families (profiles/glm_hier_penalty_resources.txt); there is no centred kernel at 128 rows to extend
int glm_hier_q_max_dim(int family) { return (family == PBBI_GLM_LOGISTIC || family == PBBI_GLM_POISSON) ? 64 : 0; }

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
// the first product's A-fragment order (glm_pack_p1), (Q + Q^T) / 2 on rows and columns < D and zero beyond.  Host only.
void glm_pack_penalty(int D, int J, const double* penalty, double* out) {
    const int DP = glm_padded_dim(D + J), KS = DP / 4;
    auto at = [&](int64_t i, int d) -> double {
        return (i < D && d < D) ? 0.5 * (penalty[(size_t)i * D + d] + penalty[(size_t)d * D + i]) : 0.0;
    };
    for (int b = 0; b < DP / 16; ++b) glm_pack_p1(KS, b, at, out + (size_t)b * KS * 64);
}

// the caller has run glm_check_obs and glm_check_hier (and glm_check_penalty where penalty is given); pot->D = Dx + J.
// penalty != NULL: the structured group priors (centred only), rank[j] into the table's n_j slots.
int glm_build_hier(pbbi_potential* pot, int Dx, int64_t M, const double* X, const double* y, int family,
                   const double* weights, const double* offset, const double* trials, const double* lam, const double* mu,
                   const int32_t* groups, int J, const double* tprior, int parametrisation, const double* penalty,
                   const double* rank) {
    const int Dt = pot->D;
    const bool nc = parametrisation == PBBI_HIER_NONCENTRED;
    const int dmax = penalty ? glm_hier_q_max_dim(family) : nc ? glm_hier_nc_max_dim(family) : glm_hier_max_dim(family);
    if (pot->dtype != PBBI_F64 || Dt > dmax)
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, "hierarchical GLM potentials: float64 and a state dimension (coefficients + "
                                               "groups) <= " + std::to_string(dmax) + " only (" +
                                                   std::to_string(Dt) + ")");
    const int DP = glm_padded_dim(Dt);
    const int64_t nbp = glm_blocks_padded(M);
    std::vector<double> img((size_t)(nbp * DP * 32));
    glm_pack_dp(Dx, DP, M, X, img.data());  // [X | 0]: the t rows meet zero columns
    std::vector<double> obs((size_t)glm_obs_len(M));
    glm_pack_obs(M, y, weights, offset, trials, obs.data());
    std::vector<double> prior((size_t)2 * DP + 4, 0.0);  // lam | mu | n_j
    double* nj = prior.data() + 2 * DP;
    glm_pack_prior_groups(Dx, J, lam, mu, groups, tprior, prior.data(), nj);
    for (int j = 0; j < 4; ++j) pot->glm_hier_n[j] = nj[j];
    if (penalty) {
        for (int j = 0; j < J; ++j) nj[j] = pot->glm_hier_rank[j] = rank[j];  // r_j t_j: the normaliser of a rank-r_j Gaussian
        std::vector<double> qimg((size_t)glm_penalty_image_len(Dx, J));
        glm_pack_penalty(Dx, J, penalty, qimg.data());
        PBBI_HIP(hipMalloc(&pot->d_glm_qimg, qimg.size() * sizeof(double)));
        PBBI_HIP(hipMemcpy(pot->d_glm_qimg, qimg.data(), qimg.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    PBBI_HIP(hipMalloc(&pot->d_glm_img, img.size() * sizeof(double)));
    PBBI_HIP(hipMalloc(&pot->d_glm_obs, obs.size() * sizeof(double)));
    PBBI_HIP(hipMalloc(&pot->d_glm_prior, prior.size() * sizeof(double)));
    PBBI_HIP(hipMemcpy(pot->d_glm_img, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice));
    PBBI_HIP(hipMemcpy(pot->d_glm_obs, obs.data(), obs.size() * sizeof(double), hipMemcpyHostToDevice));
    PBBI_HIP(hipMemcpy(pot->d_glm_prior, prior.data(), prior.size() * sizeof(double), hipMemcpyHostToDevice));
    pot->glm_DP = DP;
    pot->glm_M = M;
    pot->glm_family = family;
    pot->glm_lam = 0.0;  // (these kernels read d_glm_prior)
    pot->glm_terms = (weights ? GLM_TERM_WEIGHTS : 0) | (offset ? GLM_TERM_OFFSET : 0) | (trials ? GLM_TERM_TRIALS : 0);
    pot->glm_hier_J = J;
    pot->glm_hier_nc = nc ? 1 : 0;
    return PBBI_OK;
}

int glm_hmc_iter(const IterArgs& a) {
    if (int rc = glm_check(a.pot, a.ldn_in > a.ldn_out ? a.ldn_in : a.ldn_out)) return rc;
    if (pbbi_dyn(a)) return pbbi_fail(PBBI_ERR_UNSUPPORTED, "GLM potentials: fixed trajectory lengths only");
    if (a.fuse_S > 1) return pbbi_fail(PBBI_ERR_INVALID, "the GLM kernel takes one iteration per launch (internal)");
    if (a.N == 0) return PBBI_OK;
    GlmPrm prm = glm_prm(a.pot);
    prm.q_in = (const double*)a.q_in;
    prm.p_in = (const double*)a.p_in;
    prm.u_in = (const double*)a.u_in;
    prm.mass = (const double*)a.mass;
    prm.q_out = (double*)a.q_out;
    prm.p_out = (double*)a.p_out;
    prm.ratio_out = (double*)a.ratio_out;
    prm.reject_out = a.reject_out;
    prm.N = a.N; prm.ldn_in = a.ldn_in; prm.ldn_out = a.ldn_out;
    prm.h = a.h; prm.kT = a.kT; prm.L = a.L; prm.flags = a.flags; prm.rng = a.rng;
    prm.mode = GLM_HMC; prm.method = a.method;
    prm.seed = a.seed; prm.iter = a.iter; prm.chain0 = a.chain0;
    return glm_launch(a.pot, prm, a.stream);
}

int glm_integrate(const IntegrateArgs& a) {
    if (int rc = glm_check(a.pot, a.ldn)) return rc;
    if (a.N == 0) return PBBI_OK;
    GlmPrm prm = glm_prm(a.pot);
    prm.q_in = (const double*)a.q;
    prm.p_in = (const double*)a.p;
    prm.mass = (const double*)a.mass;
    prm.q_out = (double*)a.q;
    prm.p_out = (double*)a.p;
    prm.v_out = (double*)a.v_out;
    prm.N = a.N; prm.ldn_in = a.ldn; prm.ldn_out = a.ldn;
    prm.h = a.h; prm.L = a.L; prm.mode = GLM_INTEGRATE; prm.method = a.method;
    return glm_launch(a.pot, prm, a.stream);
}

static int glm_eval_launch(const EvalArgs& a, int mode) {
    if (int rc = glm_check(a.pot, a.ldn)) return rc;
    if (a.N == 0) return PBBI_OK;
    GlmPrm prm = glm_prm(a.pot);
    prm.q_in = (const double*)a.q;
    prm.p_in = (const double*)a.p;
    prm.mass = (const double*)a.mass;
    prm.U_out = (double*)a.U_out;
    prm.grad_out = (double*)a.grad_out;
    prm.w_out = (double*)a.w_out;
    prm.N = a.N; prm.ldn_in = a.ldn; prm.ldn_out = a.ldn;
    prm.mode = mode;
    return glm_launch(a.pot, prm, a.stream);
}
int glm_eval(const EvalArgs& a) { return glm_eval_launch(a, GLM_EVAL); }
int glm_energy(const EvalArgs& a) { return glm_eval_launch(a, a.ratio_finish ? GLM_RATIO : GLM_ENERGY); }
