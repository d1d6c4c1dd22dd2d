// kernels_glm.hip -- generalised linear models whose likelihood runs on the fp64 matrix cores (gfx950).
//
//   U(w) = sum_i [ b(x_i.w) - y_i (x_i.w) ] + 0.5 lam |w|^2,   grad U = X^T (b'(eta) - y) + lam w,   eta = X w
// over the M rows x_i of the design matrix X (M x D).  For an ENSEMBLE of chains these are two matrix products
// shared by all of them -- eta = X W and g = X^T R with W, R of one column per chain -- so the data set is read
// once per 64 chains instead of once per chain (the user-source plugin path, custom.LOGISTIC_REGRESSION_SOURCE).
//
// Layout.  One wave owns 16 chains and keeps q, the half-step velocity vh and the gradient accumulator in
// registers in the layout of kernels_dense_dev.h: element s of a lane is row 4s + g, g = lane >> 4, chain =
// lane & 15.  X travels through LDS in blocks of 16 observations, pre-swizzled on the host (glm_pack, glm_host.cpp) into the
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
// The dispersion families (FAM = PBBI_GLM_GAUSSIAN, PBBI_GLM_NEGBINOMIAL, PBBI_GLM_GAMMA of k_glm<NT, FAM, true>; handles of
// pbbi_potential_create_glm_dispersion) add a parameter that is no coefficient of X: theta, the log-dispersion, which
// enters every observation's link and whose gradient is a sum over observations per chain (include/pbbi.h has the model).
// Sampled, theta is row D of the state (D = the coefficient count): the image is that of [X | 0], so eta does not see the
// row, while the momentum draw, kick, drift, stores and the {lam, mu} prior in plds treat it like any other.  Once per
// gradient evaluation the lane that owns row D (s = D >> 2, g = D & 3) contributes its q[s] to a chain_sum, the other
// three lane groups contribute 0 (adding zeros is exact), and every lane of the chain has theta; the per-chain
// quantities (tau; phi, psi(phi), lgamma(phi); alpha, psi(alpha) - theta - 1, lgamma(alpha) - alpha theta) are formed there, once.  Each lane accumulates dU_i/dtheta of its
// observations next to usum, and chain_sum of that goes into the gradient accumulator at (s, g) before the kick and the
// evaluation's store.  Held, theta comes from the kernel arguments (a wave-uniform switch, no further instantiations)
// and the state is w alone.  The streams are c = a, d = y (raw; gamma: log y, taken once on the host), o; a row with c = 0 is
// selected out.
//
// Ordinal regression (FAM = PBBI_GLM_ORDINAL of k_glm<NT, FAM, true>; handles of pbbi_potential_create_glm_ordinal; include/pbbi.h
// has the model): K ordered categories, the K - 1 cutpoints carried as rows crow0 .. crow0 + K - 2 of the state -- zeta_1 = kappa_1,
// then the log-gaps -- behind zero columns of the image like theta above, with Gaussian priors in the {lam, mu} table.  Once per
// gradient evaluation the rows reach every lane of the chain (glm_ord_rows: a lane group owns one of them, two for K - 1 > 4) and
// kappa_j and, where U is wanted, G_k = -log(1 - exp(-Delta_k)) are formed (glm_ord_chain).  In the walk the streams are c = a, d =
// the category, o; the observation's two cutpoints are SELECTED out of the lane's kappa registers by its category, U_i = a [sp(eta
// - kappa_{k+1}) + sp(kappa_k - eta) + G_k] (glm_link_ord), and the two sigmoid terms go into seven cutpoint accumulators beside
// usum.  After it: chain_sum of each, the A_k / expm1(Delta_k) parts (A_k, the weighted category counts, follow the table in plds
// as the n_j do), the chain rule to zeta, and the results into gacc at the owning registers.  One wave per SIMD at every size; no
// kernel at 128 rows (profiles/glm_ordinal_resources.txt).
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
// A-fragment writer, one block per 16 rows of Q (glm_pack_penalty, glm_host.cpp): 8 DP^2 bytes that sit in LDS behind plds for the whole
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
//
// This file holds the device code, the kernel-argument structs, glm_check, the launch switch and the entry points.  Which
// shapes ship, the argument rules and the packers are glm_host.cpp (no HIP there); the builders that upload what the packers
// make are pbbi_api.hip's; glm_args.h fills the arguments that come from a call.  The family arithmetic (glm_link, glm_link_rich,
// glm_link_disp, glm_disp_chain, glm_psi, glm_lgamma) is glm_family_dev.h's, shared with the kernels that take draws.
#include <cmath>
#include <type_traits>

#include "glm_args.h"
#include "glm_family_dev.h"
#include "kernels_dense_dev.h"
#include "pbbi_chain.h"

int glm_launch_metric(const pbbi_potential* pot, const void* glm_prm, hipStream_t stream);  // glm_prm: a GlmPrm of this file
int glm_launch_metric_dense(const pbbi_potential* pot, const void* glm_prm, hipStream_t stream);  // (kernels_glm_dense_metric.hip)

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
// the ordinal family's kernel arguments (the full model's kernels keep theirs as they are); prior: lam (DP) | mu (DP) | A_k (8,
// the weighted category counts sum_{i: y_i = k} a_i, 0 past K)
struct GlmPrmOrd : GlmPrmRich {
    int crow0;  // the state row of zeta_1 (= the coefficient count); zeta_{j+1} is row crow0 + j
    int K;      // categories, 2 .. 8
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
// HIER of k_glm: no hierarchical prior, the centred parametrisation (the chain holds w_d), the non-centred one (z_d), the
// centred one with a penalty matrix in each group's quadratic form
enum { GLM_HIER_NONE = 0, GLM_HIER_CENTRED = 1, GLM_HIER_NC = 2, GLM_HIER_Q = 3 };
template <int FAM, bool RICH, int HIER = GLM_HIER_NONE>
struct GlmArgs {
    using type = std::conditional_t<HIER == GLM_HIER_Q, GlmPrmHierQ,
                                    std::conditional_t<HIER != GLM_HIER_NONE, std::conditional_t<glm_disp(FAM), GlmPrmHierDisp, GlmPrmHier>, GlmPrm>>;
};
template <int FAM>
struct GlmArgs<FAM, true, GLM_HIER_NONE> {
    using type = std::conditional_t<glm_disp(FAM), GlmPrmDisp, std::conditional_t<FAM == PBBI_GLM_ORDINAL, GlmPrmOrd, GlmPrmRich>>;
};
// what a family forms once per chain and gradient evaluation, and what a lane accumulates beside usum for the rows that are no
// coefficients of X: theta's (a double) or the cutpoints' (GlmOrdAcc)
template <int FAM> using GlmFamChain = std::conditional_t<FAM == PBBI_GLM_ORDINAL, GlmOrdChain, GlmDispChain>;
template <int FAM> using GlmFamAcc = std::conditional_t<FAM == PBBI_GLM_ORDINAL, GlmOrdAcc, double>;
// the diagonal metric's kernel arguments (METRIC = true of k_glm): the arguments of the same kernel without one, plus the table
template <class Prm>
struct GlmPrmMetric : Prm {
    const double* metric;  // {m_d, 1 / m_d} of each of the DP rows, {1, 1} past D (glm_pack_metric, glm_host.cpp)
};
// the dense metric's (METRIC = GLM_METRIC_DENSE of k_glm): the same arguments plus the three images
template <class Prm>
struct GlmPrmMetricDense : Prm {
    const double* dimg;  // C = M^-1 | L | M, each (DP x DP) in the first product's A-fragment order (glm_pack_metric_dense, glm_host.cpp)
};
// METRIC of k_glm: no metric, the diagonal one, the dense one.  (ints, not an unnamed enum: they are compared in the kernels'
// signature, an unnamed type there enters the mangled name, and the host and device passes number unnamed types differently --
// the host would register a name the code object does not hold)
constexpr int GLM_METRIC_NONE = 0, GLM_METRIC_DIAG = 1, GLM_METRIC_DENSE = 2;
template <int FAM, bool RICH, int HIER, int METRIC>
using GlmKernelArgs = std::conditional_t<METRIC == GLM_METRIC_DENSE, GlmPrmMetricDense<typename GlmArgs<FAM, RICH, HIER>::type>,
                                         std::conditional_t<METRIC == GLM_METRIC_DIAG, GlmPrmMetric<typename GlmArgs<FAM, RICH, HIER>::type>,
                                                            typename GlmArgs<FAM, RICH, HIER>::type>>;
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

// the ordinal family's K - 1 cutpoint rows to every lane of the chain: lane group g owns zeta row jo in register so and, for
// K - 1 > 4, row jo + 4 one register on; the owner contributes its q to that row's chain_sum, everybody else an exact 0
template <int KS>
__device__ __forceinline__ void glm_ord_rows(const double (&q)[KS], int jo, int so, int K, double (&z)[7]) {
    double th0 = 0.0, th1 = 0.0;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        th0 = (s == so) ? q[s] : th0;
        th1 = (s == so + 1) ? q[s] : th1;
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        z[j] = 0.0;
        if (j < K - 1) z[j] = chain_sum(jo == (j & 3) ? (j < 4 ? th0 : th1) : 0.0);  // rows past K - 1 are not summed
    }
}

// gacc[t][r] (row 16t + 4r + g) = sum_i X[i][row] (b'(eta_i) - y_i) for the wave's 16 chains, usum = this lane's
// share of sum_i b(eta_i) - y_i eta_i (observations {4r + g} of every block; chain_sum completes it).
// Every wave of the workgroup takes part in the staging: one chunk of CB blocks is in LDS while the next waits
// in registers (fetched before the MFMAs of the current one, written after the barrier that ends its reads).
// RICH: ylds holds the chunk's c | d | o (OBS values each); thread j < 3 OBS stages value j % OBS of stream j / OBS.
// Dispersion families: dk = the chain's theta-derived values, tsum = this lane's share of sum_i dU_i/dtheta.
// Ordinal family: dk = the chain's cutpoints and what is formed from them, tsum.c[j] = this lane's share of sum_i dU_i/dkappa_{j+1}.
template <int NT, int FAM, bool RICH, int HIER = GLM_HIER_NONE>
__device__ __forceinline__ void glm_grad(const typename GlmArgs<FAM, RICH, HIER>::type& prm, v2f64* __restrict__ lds,
                                         double* __restrict__ ylds, int lane, int g, const double (&q)[4 * NT], v4f64 (&gacc)[NT],
                                         double& usum, bool want_u, [[maybe_unused]] const GlmFamChain<FAM>& dk,
                                         [[maybe_unused]] GlmFamAcc<FAM>& tsum) {
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
    if constexpr (FAM == PBBI_GLM_ORDINAL) {
#pragma unroll
        for (int j = 0; j < 7; ++j) tsum.c[j] = 0.0;
    }
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
                } else if constexpr (FAM == PBBI_GLM_ORDINAL) {
                    const int i = bi * 16 + 4 * r + g;
                    const double cv = ylds[i], yv = ylds[C::OBS + i], ov = ylds[2 * C::OBS + i];
                    double thi, tlo;
                    glm_link_ord(eta[r] + ov, cv, yv, dk, want_u, rr, ut, thi, tlo);
                    const bool on = ok && cv != 0.0;  // weight 0: exactly nothing
                    res[r] = on ? rr : 0.0;
                    usum += on ? ut : 0.0;
                    // category k loses a s_hi from dU/dkappa_{k+1} and gains a s_lo in dU/dkappa_k (absent terms are 0)
                    thi = on ? thi : 0.0;
                    tlo = on ? tlo : 0.0;
#pragma unroll
                    for (int j = 0; j < 7; ++j)
                        tsum.c[j] += (yv == (double)j) ? -thi : (yv == (double)(j + 1)) ? tlo : 0.0;
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
// = 128 it spills even with all 512 and is not instantiated (glm_max_dim of glm_host.cpp says so to the create entry and to the launch).
// Likewise the non-centred logistic kernel at DP = 32: q, its scaled copy and the link's constants need 12 bytes of scratch
// at 256 registers.  The structured group priors (GLM_HIER_Q) keep the centred kernels' counts: all six build without scratch
// at them (profiles/glm_hier_penalty_resources.txt).
// The dispersion families with a hierarchical prior (centred and non-centred) need no case of their own: all twelve build without
// scratch at their families' counts (profiles/glm_hier_dispersion_resources.txt).
// The Gamma family runs at the Gaussian's counts, DP = 128 included (profiles/glm_gamma_resources.txt).
// The dense metric's twins run at their parents' counts but for the Poisson kernels at DP = 64: those parents reach two waves by
// register count under a bound of one, and their dense twins, left at that bound, take 285 registers; asked for two they build in
// 254 without scratch (profiles/glm_dense_metric_resources.txt).
constexpr int glm_waves_per_simd(int NT, int fam, int hier, int metric = GLM_METRIC_NONE) {
    if (metric == GLM_METRIC_DENSE && NT == 4 && fam == PBBI_GLM_POISSON) return 2;
    if (fam == PBBI_GLM_ORDINAL) return 1;  // at the logistic's two waves the 16- and 32-row kernels reserve 212 / 324 bytes of scratch
    return (NT <= 2 && !(NT == 2 && (fam == PBBI_GLM_NEGBINOMIAL || (hier == GLM_HIER_NC && fam == PBBI_GLM_LOGISTIC)))) ? 2 : 1;
}
// TWIN: k_glm_softmax of kernels_glm_softmax.hip restates this frame (ghost waves and ragged tail, momentum first, the
// kick / drift schedule of the evaluation loop, the five modes, the accept epilogue).  A fix to either belongs in both.
//
// The diagonal metric (METRIC = true; a handle that carries one, pbbi_potential_set_metric_diag): row d of chain n has mass
// m_n m_d.  The table {m_d, 1 / m_d} sits in LDS for the launch (mlds, DP entries of 16 bytes beside plds, loaded once before
// the first barrier; entry 4s + g is register s of the lane, the indexing of the {lam, mu} reads) and is read where it is
// used -- KS more values per lane in registers would cost the DP = 64 and 128 kernels theirs.  It enters the draw (p = z sqrt(m_n
// m_d kT)), the velocity (v = p / (m_n m_d)), the kick (ck / m_d), p = v m_n m_d at the end and both kinetic energies (sum p^2 /
// m_d, then / m_n); the drift, the gradient and U never see it.  Every one of these is today's operation with one more factor, so
// a table of ones multiplies by exactly 1.0 and the run is today's bit for bit.  METRIC = GLM_METRIC_NONE: nothing of it is compiled.
//
// The dense metric (METRIC = GLM_METRIC_DENSE; pbbi_potential_set_metric_dense): chain n has the mass matrix m_n M, M = L L^T, C =
// M^-1 (include/pbbi.h has the model).  vh stays the velocity.  C sits in LDS behind plds for the launch (clds, 8 DP^2 bytes in the
// first product's A-fragment order, like the penalty of GLM_HIER_Q); L and M are used once per iteration and their fragments are
// read straight from memory.  A state register is the B operand of a K-step as it sits and tile t of the product comes out with
// register r = row 16t + 4r + g, so no value moves between lanes:
//   draw      p = L (z sqrt(m_n kT))      into gacc (dead before the first gradient), then vh
//   velocity  C p into gacc; pp = sum p_s (C p)_s is formed THERE, where both are in hand; vh = (C p) / m_n
//   kick      the rows' gradients (likelihood and prior) go into gacc in place; C g tile by tile with gacc as the B operand, the
//             four registers of the tile kicked and drifted at once -- one output tile is live at a time
//   the end   p = m_n (M v) into gacc (dead after the last kick); pp = sum p_s (m_n v_s), C p = m_n v being what v is
// The kinetic energy is 0.5 pp / m_n as without a metric.  With M = I every product is exact and every other operation is the one
// of the kernel without a metric on the same values: the dense identity reproduces it bit for bit.  Padding rows: the images are
// the identity there, their momenta, gradients and velocities are exact zeros.
template <int KS, class Bop>
__device__ __forceinline__ v4f64 glm_square_tile(const v2f64* __restrict__ A, int t, const Bop& b) {  // A: the image + lane
    v4f64 acc = v4f64{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s2 = 0; s2 < KS / 2; ++s2) {
        const v2f64 a = A[(t * (KS / 2) + s2) * 64];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b(2 * s2), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, b(2 * s2 + 1), acc, 0, 0, 0);
    }
    return acc;
}
template <int NT, int FAM, bool RICH, int HIER = GLM_HIER_NONE, int METRIC_KIND = GLM_METRIC_NONE>
__global__ void __launch_bounds__(BLOCK, glm_waves_per_simd(NT, FAM, HIER, METRIC_KIND)) k_glm(GlmKernelArgs<FAM, RICH, HIER, METRIC_KIND> prm) {
    constexpr bool METRIC = METRIC_KIND == GLM_METRIC_DIAG;  // (the diagonal metric's statements below read as they always have)
    constexpr bool DENSE = METRIC_KIND == GLM_METRIC_DENSE;
    static_assert(!DENSE || (HIER == GLM_HIER_NONE && FAM != PBBI_GLM_ORDINAL && NT <= 4), "the dense metric: no hierarchical prior, not the ordinal family, DP <= 64");
    static_assert(RICH || !glm_disp(FAM), "the dispersion families live on the full model's frame");
    static_assert(HIER == GLM_HIER_NONE || RICH, "the hierarchical prior lives on the full model's frame");
    static_assert(HIER != GLM_HIER_Q || !glm_disp(FAM), "structured group priors: logistic and poisson only");
    static_assert(FAM != PBBI_GLM_ORDINAL || (RICH && HIER == GLM_HIER_NONE), "the ordinal family: the full model's frame, no random effects");
    using C = GlmCfg<NT>;
    constexpr int KS = C::KS;
    constexpr int DP = 16 * NT;
    __shared__ __attribute__((aligned(16))) v2f64 lds[C::CHV];
    __shared__ double ylds[(RICH ? 3 : 1) * C::CB * 16];
    constexpr bool HAS_NJ = HIER == GLM_HIER_CENTRED || HIER == GLM_HIER_Q;
    // RICH: {lam, mu} of each row (else unused); centred HIER: then {n_j, 0}; HIER_Q: then the penalty's fragments (8 DP^2 bytes)
    // METRIC: behind all of that the metric's table {m_d, 1 / m_d}, DP entries (mlds below) -- one array, so that a kernel without
    // a metric declares exactly what it always has
    // ordinal family: then {A_k, 0}, 8 entries
    constexpr bool ORD = FAM == PBBI_GLM_ORDINAL;
    constexpr int PL = RICH ? DP + (HAS_NJ ? 4 : 0) + (HIER == GLM_HIER_Q ? DP * DP / 2 : 0) + (ORD ? 8 : 0) : 0;
    // DENSE: behind plds the C image instead (clds below), DP^2 / 2 entries
    constexpr int ML = METRIC ? DP : DENSE ? DP * DP / 2 : 0;
    __shared__ __attribute__((aligned(16))) v2f64 plds[PL + ML > 0 ? PL + ML : 1];
    if constexpr (RICH) {
        for (int i = threadIdx.x; i < DP; i += BLOCK) plds[i] = v2f64{prm.prior[i], prm.prior[DP + i]};
        if constexpr (HAS_NJ)
            if (threadIdx.x < 4) plds[DP + threadIdx.x] = v2f64{prm.prior[2 * DP + threadIdx.x], 0.0};
        if constexpr (ORD)
            if (threadIdx.x < 8) plds[DP + threadIdx.x] = v2f64{prm.prior[2 * DP + threadIdx.x], 0.0};
        if constexpr (HIER == GLM_HIER_Q) {
            const v2f64* __restrict__ qsrc = reinterpret_cast<const v2f64*>(prm.qimg);
            for (int i = threadIdx.x; i < DP * DP / 2; i += BLOCK) plds[DP + 4 + i] = qsrc[i];
        }
        if constexpr (!METRIC && !DENSE) __syncthreads();
    }
    [[maybe_unused]] v2f64* const mlds = plds + PL;
    if constexpr (METRIC) {
        const v2f64* __restrict__ msrc = reinterpret_cast<const v2f64*>(prm.metric);
        for (int i = threadIdx.x; i < DP; i += BLOCK) mlds[i] = msrc[i];
        __syncthreads();
    }
    if constexpr (DENSE) {
        const v2f64* __restrict__ csrc = reinterpret_cast<const v2f64*>(prm.dimg);
        for (int i = threadIdx.x; i < DP * DP / 2; i += BLOCK) mlds[i] = csrc[i];
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
            for (int sl = 0; sl < 4; ++sl) {
                if constexpr (METRIC) {
                    const double pstd_d = sqrt((m * mlds[4 * (4 * k + sl) + g].x) * prm.kT);
                    vh[4 * k + sl] = (16 * k + 4 * sl + g < D) ? z[sl] * pstd_d : 0.0;
                } else {
                    vh[4 * k + sl] = (16 * k + 4 * sl + g < D) ? z[sl] * pstd : 0.0;
                }
            }
        }
        if constexpr (DENSE) {  // p = L (z sqrt(m_n kT)), L's fragments from memory
            const v2f64* __restrict__ LA = reinterpret_cast<const v2f64*>(prm.dimg) + DP * DP / 2 + lane;
#pragma unroll
            for (int t = 0; t < NT; ++t) gacc[t] = glm_square_tile<KS>(LA, t, [&](int s) { return vh[s]; });
#pragma unroll
            for (int s = 0; s < KS; ++s) vh[s] = gacc[s >> 2][s & 3];
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
    if constexpr (DENSE) {  // C p into gacc while p is the operand; sum_s p_s (C p)_s
#pragma unroll
        for (int t = 0; t < NT; ++t) gacc[t] = glm_square_tile<KS>(mlds + lane, t, [&](int s) { return vh[s]; });
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        if constexpr (METRIC) pp_old = fma(vh[s] * mlds[4 * s + g].y, vh[s], pp_old);  // sum_d p_d^2 / m_d
        else if constexpr (DENSE) pp_old = fma(vh[s], gacc[s >> 2][s & 3], pp_old);
        else pp_old = fma(vh[s], vh[s], pp_old);
    }
    // (the sum is FORMED here: left to the compiler it is sunk to the accept test, and the drawn momenta and the table's
    //  entries stay in registers across the whole trajectory -- 388 bytes of scratch at DP = 128)
    if constexpr (METRIC || DENSE) pp_old = vgpr_fresh(pp_old);
    if (traj) {
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            if constexpr (METRIC) vh[s] *= minv * mlds[4 * s + g].y;  // v = p / (m_n m_d)
            else if constexpr (DENSE) vh[s] = gacc[s >> 2][s & 3] * minv;  // v = C p / m_n
            else vh[s] *= minv;  // v = p/m
        }
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
        [[maybe_unused]] GlmFamChain<FAM> dk{};
        [[maybe_unused]] GlmFamAcc<FAM> tsum{};
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
        // the ordinal family: the K - 1 cutpoint rows to every lane of the chain.  They are consecutive rows crow0 + j, a lane's rows
        // 4 apart: lane group g owns zeta row jo = (g - crow0) & 3 in register so and, for K - 1 > 4, row jo + 4 one register on.
        // The owner contributes its q to that row's chain_sum, everybody else an exact 0; rows past K - 1 are not summed.
        [[maybe_unused]] int ojo = 0, oso = -1;
        if constexpr (ORD) {
            ojo = (g - prm.crow0) & 3;
            oso = (prm.crow0 + ojo) >> 2;
            double z[7];
            glm_ord_rows<KS>(q, ojo, oso, prm.K, z);
            dk = glm_ord_chain(z, prm.K, want_u);
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
        if constexpr (ORD) {
            // dU/dkappa_{j+1}: the chain's sum of the lanes' shares, plus A_{j+1} / expm1(Delta_{j+1}) - A_j / expm1(Delta_j) from
            // the G terms of the interior categories (an empty category is SELECTED out: its width may have underflowed to 0).
            // Then the chain rule to zeta, dU/dzeta_1 = sum_j dU/dkappa_j, dU/dzeta_m = Delta_{m-1} sum_{j >= m} dU/dkappa_j, into
            // gacc at the owning register of each row (the prior's part comes with the row's {lam, mu} like any fixed row's).
            // (the rows are read again and the widths formed here: q has not moved since the broadcast before the walk)
            double z[7], gap[7], iem[7];
            glm_ord_rows<KS>(q, ojo, oso, prm.K, z);
            glm_ord_widths(z, prm.K, gap, iem);
            double ai[8];
            ai[0] = 0.0;
#pragma unroll
            for (int m = 1; m < 7; ++m) {
                const double A = plds[DP + m].x;
                ai[m] = (A != 0.0) ? A * iem[m] : 0.0;  // (iem is 0 past the interior categories)
            }
            ai[7] = 0.0;
            double suf = 0.0, gown0 = 0.0, gown1 = 0.0;
#pragma unroll
            for (int j = 6; j >= 0; --j) {
                if (j < prm.K - 1) suf += chain_sum(tsum.c[j]) + (ai[j + 1] - ai[j]);
                const double gz = (j < prm.K - 1) ? (j == 0 ? suf : gap[j] * suf) : 0.0;
                if (j < 4) gown0 = (ojo == j) ? gz : gown0;
                else gown1 = (ojo == j - 4) ? gz : gown1;
            }
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) gacc[t][r] += (4 * t + r == oso) ? gown0 : (4 * t + r == oso + 1) ? gown1 : 0.0;
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
            // (the product below is glm_square_tile's, the form the dense metric shares; it stays written out here so that these
            // kernels keep the code they have)
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
        // METRIC: the table is READ here, through a copy of the lane's index the compiler cannot see through -- the values
        // read for the velocity above would otherwise stay in registers across the gradient
        [[maybe_unused]] int gm = g;
        if constexpr (METRIC) gm = vgpr_fresh(g);
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
                if constexpr (DENSE) {
                    gacc[t][r] = gt;  // the row's whole gradient in place: the B operand of C g below
                } else {
                    if constexpr (METRIC) vh[s] = fma(-gt, ck * mlds[4 * s + gm].y, vh[s]);  // (ck != 0 here: no 0 * inf)
                    else vh[s] = fma(-gt, ck, vh[s]);
                    q[s] = fma(vh[s], hd, q[s]);
                }
            }
        if constexpr (DENSE) {  // C g tile by tile, the tile's four rows kicked and drifted at once
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const v4f64 cg = glm_square_tile<KS>(mlds + lane, t, [&](int s) { return gacc[s >> 2][s & 3]; });
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int s = 4 * t + r;
                    vh[s] = fma(-cg[r], ck, vh[s]);
                    q[s] = fma(vh[s], hd, q[s]);
                }
            }
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
        if constexpr (DENSE) {  // p = m_n (M v), M's fragments from memory
            const v2f64* __restrict__ MA = reinterpret_cast<const v2f64*>(prm.dimg) + DP * DP + lane;
#pragma unroll
            for (int t = 0; t < NT; ++t) gacc[t] = glm_square_tile<KS>(MA, t, [&](int s) { return vh[s]; });
        }
        if (valid) {
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                store_row(qout, vout, s4out, s, q[s]);
                if constexpr (DENSE) store_row(pout, vout, s4out, s, prm.mass ? gacc[s >> 2][s & 3] * m : gacc[s >> 2][s & 3]);
                else if constexpr (METRIC) store_row(pout, vout, s4out, s, (prm.mass ? vh[s] * m : vh[s]) * mlds[4 * s + vgpr_fresh(g)].x);
                else store_row(pout, vout, s4out, s, prm.mass ? vh[s] * m : vh[s]);
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
    [[maybe_unused]] int ge = g;
    if constexpr (METRIC) ge = vgpr_fresh(g);  // (read again, as at the kick)
    if constexpr (DENSE) {  // M v into gacc while v is the operand
        const v2f64* __restrict__ MA = reinterpret_cast<const v2f64*>(prm.dimg) + DP * DP + lane;
#pragma unroll
        for (int t = 0; t < NT; ++t) gacc[t] = glm_square_tile<KS>(MA, t, [&](int s) { return vh[s]; });
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        if constexpr (DENSE) {  // p = m_n (M v) and C p = m_n v: sum_s p_s (C p)_s; vh now holds p
            const double cp = prm.mass ? vh[s] * m : vh[s];
            vh[s] = prm.mass ? gacc[s >> 2][s & 3] * m : gacc[s >> 2][s & 3];
            pp_new = fma(vh[s], cp, pp_new);
            continue;
        }
        if (prm.mass) vh[s] *= m;  // p = v*m; vh now holds p
        if constexpr (METRIC) {
            const v2f64 md = mlds[4 * s + ge];
            vh[s] *= md.x;  // p = v m_n m_d
            pp_new = fma(vh[s] * md.y, vh[s], pp_new);
        } else {
            pp_new = fma(vh[s], vh[s], pp_new);
        }
    }
    const double oldH = 0.5 * chain_sum(pp_old) / m + U_old;
    double newH = 0.5 * chain_sum(pp_new) / m + U_new;
    // ordinal: a trajectory that diverged -- a width exp(zeta) that overflowed, inf - inf in a cutpoint, a NaN momentum behind
    // them -- ends in a NaN energy, and a NaN ratio is ACCEPTED (metropolis_reject).  The widths are exponentials of the state,
    // so the step that rejects a fifth of the proposals is close to the one that diverges, and a chain that accepted a NaN never
    // leaves it: here a NaN energy is an infinite one, a rejected proposal.
    if constexpr (FAM == PBBI_GLM_ORDINAL) newH = (newH == newH) ? newH : __builtin_inf();
    // dense metric: a gradient row that overflowed at the last evaluation is an infinite momentum and an infinite energy in the
    // kernels without a product (rejected); through C g it meets the zeros of the image as 0 * inf, a NaN in every row of the chain,
    // a NaN energy and an ACCEPTED proposal.  A NaN energy is an infinite one here too: the proposal is rejected as it is there,
    // with the ratio 0 it has there.
    if constexpr (DENSE) newH = (newH == newH) ? newH : __builtin_inf();
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

// the full model's part of the arguments, which every kernel but the plain model's takes
template <class Prm>
Prm glm_prm_rich(const pbbi_potential* pot, const GlmPrm& prm) {
    Prm r{};
    static_cast<GlmPrm&>(r) = prm;
    r.obs = (const double*)pot->d_glm_obs;
    r.prior = (const double*)pot->d_glm_prior;
    r.obs_stride = glm_blocks_padded(pot->glm_M) * 16;
    return r;
}
// ... and the hierarchical prior's: the t rows follow the coefficients, a sampled theta is the last row, behind them
template <class Prm>
Prm glm_prm_hier(const pbbi_potential* pot, const GlmPrm& prm) {
    Prm r = glm_prm_rich<Prm>(pot, prm);
    r.trow0 = pot->D - pot->glm_hier_J - (pot->glm_trow >= 0 ? 1 : 0);
    r.J = pot->glm_hier_J;
    return r;
}

// One case per variant of handle (glm_host.h), each building the one argument struct its kernels take.  A variant, family or
// padded dimension with no shipped kernel launches nothing and is PBBI_ERR_UNSUPPORTED.
template <int GLM_METRIC_PASS>  // GLM_METRIC_NONE / _DIAG / _DENSE: the one kind of kernel this pass instantiates
int glm_launch_pass(const pbbi_potential* pot, const GlmPrm& prm, hipStream_t stream) {
    const dim3 grid((unsigned)((prm.N + CHAINS_PER_WG - 1) / CHAINS_PER_WG)), block(BLOCK);
    const int NT = pot->glm_DP / 16, fam = pot->glm_family;
    bool done = false;
// a handle without a metric launches the kernel it always has; one with a metric the METRIC twin of the same case, which
// takes the same arguments plus the table (the dense metric: plus the images), where that twin is shipped
#define GLM_CASE(NT_, FAM_, RICH_, HIER_, PRM_)                                                             \
    if (NT == NT_ && fam == FAM_) {                                                                         \
        if constexpr (GLM_METRIC_PASS == GLM_METRIC_NONE) {                                                 \
            hipLaunchKernelGGL((k_glm<NT_, FAM_, RICH_, HIER_>), grid, block, 0, stream, PRM_);             \
            done = true;                                                                                    \
        } else if constexpr (GLM_METRIC_PASS == GLM_METRIC_DIAG) {                                          \
            if constexpr (16 * NT_ <= glm_metric_max_rows(FAM_, RICH_, HIER_)) {                            \
                GlmPrmMetric<std::decay_t<decltype(PRM_)>> am{};                                            \
                static_cast<std::decay_t<decltype(PRM_)>&>(am) = PRM_;                                      \
                am.metric = (const double*)pot->d_glm_metric;                                               \
                hipLaunchKernelGGL((k_glm<NT_, FAM_, RICH_, HIER_, GLM_METRIC_DIAG>), grid, block, 0, stream, am); \
                done = true;                                                                                \
            }                                                                                               \
        } else if constexpr (16 * NT_ <= glm_dense_metric_max_rows(FAM_, RICH_, HIER_)) {                   \
            GlmPrmMetricDense<std::decay_t<decltype(PRM_)>> ad{};                                           \
            static_cast<std::decay_t<decltype(PRM_)>&>(ad) = PRM_;                                          \
            ad.dimg = (const double*)pot->d_glm_metric_dense;                                               \
            hipLaunchKernelGGL((k_glm<NT_, FAM_, RICH_, HIER_, GLM_METRIC_DENSE>), grid, block, 0, stream, ad); \
            done = true;                                                                                    \
        }                                                                                                   \
    }
// (K_ is the case list's kernel of the variant in hand.  The lists keep the order they have always had: it is the order in which
// the kernels are instantiated and laid out in the code object.)
    if (pot->D <= glm_max_dim(pot->glm_variant, fam)) switch (pot->glm_variant) {
        case GLM_V_DISPERSION: {
            GlmPrmDisp a = glm_prm_rich<GlmPrmDisp>(pot, prm);
            a.theta = pot->glm_theta;
            a.trow = pot->glm_trow;
#define K_(NT_, FAM_) GLM_CASE(NT_, FAM_, true, GLM_HIER_NONE, a)
            K_(1, PBBI_GLM_GAUSSIAN) K_(2, PBBI_GLM_GAUSSIAN) K_(4, PBBI_GLM_GAUSSIAN) K_(8, PBBI_GLM_GAUSSIAN)
            K_(1, PBBI_GLM_NEGBINOMIAL) K_(2, PBBI_GLM_NEGBINOMIAL) K_(4, PBBI_GLM_NEGBINOMIAL)
            K_(1, PBBI_GLM_GAMMA) K_(2, PBBI_GLM_GAMMA) K_(4, PBBI_GLM_GAMMA) K_(8, PBBI_GLM_GAMMA)
#undef K_
        } break;
        case GLM_V_ORDINAL: {
            GlmPrmOrd a = glm_prm_rich<GlmPrmOrd>(pot, prm);
            a.K = pot->glm_K;
            a.crow0 = pot->D - (pot->glm_K - 1);
#define K_(NT_) GLM_CASE(NT_, PBBI_GLM_ORDINAL, true, GLM_HIER_NONE, a)
            K_(1) K_(2) K_(4)
#undef K_
        } break;
        case GLM_V_HIER: {
            const GlmPrmHier a = glm_prm_hier<GlmPrmHier>(pot, prm);
#define K_(NT_, FAM_) GLM_CASE(NT_, FAM_, true, GLM_HIER_CENTRED, a)
            K_(1, PBBI_GLM_LOGISTIC) K_(2, PBBI_GLM_LOGISTIC) K_(4, PBBI_GLM_LOGISTIC)
            K_(1, PBBI_GLM_POISSON) K_(2, PBBI_GLM_POISSON) K_(4, PBBI_GLM_POISSON)
#undef K_
        } break;
        case GLM_V_HIER_NC: {
            const GlmPrmHier a = glm_prm_hier<GlmPrmHier>(pot, prm);
#define K_(NT_, FAM_) GLM_CASE(NT_, FAM_, true, GLM_HIER_NC, a)
            K_(1, PBBI_GLM_LOGISTIC) K_(2, PBBI_GLM_LOGISTIC) K_(4, PBBI_GLM_LOGISTIC)
            K_(1, PBBI_GLM_POISSON) K_(2, PBBI_GLM_POISSON) K_(4, PBBI_GLM_POISSON)
#undef K_
        } break;
        case GLM_V_HIER_Q: {
            GlmPrmHierQ a = glm_prm_hier<GlmPrmHierQ>(pot, prm);
            a.qimg = (const double*)pot->d_glm_qimg;
#define K_(NT_, FAM_) GLM_CASE(NT_, FAM_, true, GLM_HIER_Q, a)
            K_(1, PBBI_GLM_LOGISTIC) K_(2, PBBI_GLM_LOGISTIC) K_(4, PBBI_GLM_LOGISTIC)
            K_(1, PBBI_GLM_POISSON) K_(2, PBBI_GLM_POISSON) K_(4, PBBI_GLM_POISSON)
#undef K_
        } break;
        case GLM_V_HIER_DISPERSION: {
            GlmPrmHierDisp a = glm_prm_hier<GlmPrmHierDisp>(pot, prm);
            a.theta = pot->glm_theta;
            a.trow = pot->glm_trow;
#define K_(NT_, FAM_)                                                                                       \
    if (pot->glm_hier_nc) {                                                                                 \
        GLM_CASE(NT_, FAM_, true, GLM_HIER_NC, a)                                                           \
    } else {                                                                                                \
        GLM_CASE(NT_, FAM_, true, GLM_HIER_CENTRED, a)                                                      \
    }
            K_(1, PBBI_GLM_GAUSSIAN) K_(2, PBBI_GLM_GAUSSIAN) K_(4, PBBI_GLM_GAUSSIAN)
            K_(1, PBBI_GLM_NEGBINOMIAL) K_(2, PBBI_GLM_NEGBINOMIAL) K_(4, PBBI_GLM_NEGBINOMIAL)
#undef K_
        } break;
#define K_(NT_, RICH_, PRM_) \
    GLM_CASE(NT_, PBBI_GLM_LOGISTIC, RICH_, GLM_HIER_NONE, PRM_) GLM_CASE(NT_, PBBI_GLM_POISSON, RICH_, GLM_HIER_NONE, PRM_)
        case GLM_V_PLAIN: {
            K_(1, false, prm) K_(2, false, prm) K_(4, false, prm) K_(8, false, prm)
        } break;
        case GLM_V_FULL: {
            const GlmPrmRich a = glm_prm_rich<GlmPrmRich>(pot, prm);
            K_(1, true, a) K_(2, true, a) K_(4, true, a) K_(8, true, a)
        } break;
#undef K_
    }
#undef GLM_CASE
    if (!done) return pbbi_fail(PBBI_ERR_UNSUPPORTED, "GLM kernels: no kernel is shipped for this handle's variant, family and "
                                                      "padded state dimension");
    PBBI_HIP(hipGetLastError());
    return PBBI_OK;
}
#ifndef PBBI_GLM_METRIC_TU
// the existing case lists here, the METRIC lists in a translation unit of their own (kernels_glm_metric.hip, see the end)
int glm_launch(const pbbi_potential* pot, const GlmPrm& prm, hipStream_t stream) {
    if (pot->d_glm_metric_dense) return glm_launch_metric_dense(pot, &prm, stream);
    if (!pot->d_glm_metric) return glm_launch_pass<GLM_METRIC_NONE>(pot, prm, stream);
    return glm_launch_metric(pot, &prm, stream);
}

template <class Args>
int glm_run(const Args& a, int mode) {
    if (a.N == 0) return PBBI_OK;
    GlmPrm prm = glm_prm(a.pot);
    glm_fill(prm, a, mode);
    return glm_launch(a.pot, prm, a.stream);
}

#endif  // !PBBI_GLM_METRIC_TU

}  // namespace

// The METRIC instantiations are compiled from this same file as a second translation unit (kernels_glm_metric.hip defines
// PBBI_GLM_METRIC_TU and includes it): with both lists in one module the compiler lays the kernels without a metric out
// differently -- 15 of the 53 move by a register or two although their code is the same text -- and the kernels of a handle
// without a metric must stay what they are.  That unit holds the METRIC case lists and this entry, nothing else.
// The dense metric's instantiations are a third unit for the same reason (kernels_glm_dense_metric.hip defines PBBI_GLM_METRIC_TU
// as 2): the diagonal metric's kernels stay what they are too.
#if defined(PBBI_GLM_METRIC_TU) && PBBI_GLM_METRIC_TU == 2
int glm_launch_metric_dense(const pbbi_potential* pot, const void* glm_prm, hipStream_t stream) {
    return glm_launch_pass<GLM_METRIC_DENSE>(pot, *static_cast<const GlmPrm*>(glm_prm), stream);
}
#elif defined(PBBI_GLM_METRIC_TU)
int glm_launch_metric(const pbbi_potential* pot, const void* glm_prm, hipStream_t stream) {
    return glm_launch_pass<GLM_METRIC_DIAG>(pot, *static_cast<const GlmPrm*>(glm_prm), stream);
}
#else

int glm_hmc_iter(const IterArgs& a) {
    if (int rc = glm_check(a.pot, a.ldn_in > a.ldn_out ? a.ldn_in : a.ldn_out)) return rc;
    if (int rc = glm_check_iter(a)) return rc;
    return glm_run(a, GLM_HMC);
}
int glm_integrate(const IntegrateArgs& a) {
    if (int rc = glm_check(a.pot, a.ldn)) return rc;
    return glm_run(a, GLM_INTEGRATE);
}
int glm_eval(const EvalArgs& a) {
    if (int rc = glm_check(a.pot, a.ldn)) return rc;
    return glm_run(a, GLM_EVAL);
}
int glm_energy(const EvalArgs& a) {
    if (int rc = glm_check(a.pot, a.ldn)) return rc;
    return glm_run(a, a.ratio_finish ? GLM_RATIO : GLM_ENERGY);
}
#endif  // PBBI_GLM_METRIC_TU
