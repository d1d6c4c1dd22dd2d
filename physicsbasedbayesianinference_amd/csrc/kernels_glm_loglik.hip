// kernels_glm_loglik.hip -- the likelihood energy of each of S * N draws of a GLM handle's state (gfx950):
//   ulik[s * N + n] = sum_i U_i(draw)
// the likelihood part of k_glm's U (kernels_glm.hip) -- minus the log-likelihood with the constants k_i dropped as k_glm
// drops them -- without the prior, the group-scale terms or theta's prior.  It is what a likelihood-tempered SMC sampler
// (smc.LikelihoodTemperedSMC) weighs its particles by at every stage: an M x D x T product on the fp64 matrix cores.
// The same file holds the kernel that scales a handle's observation streams by a likelihood power
// (pbbi_potential_set_likelihood_power): pi_beta(w) ~ p(w) L(w)^beta is the full model with every weight a_i times beta.
//
// No header is shared with kernels_glm.hip or kernels_glm_pointwise.hip and neither is touched: glm_link, glm_link_rich,
// glm_link_disp and glm_lgamma are RESTATED below operation for operation (ll_link, ll_lgamma), as pw_link restates them
// (tests/test_glm_loglik.py holds ulik + prior to the U of pbbi_potential_eval on the same draws).  The plain model is the full
// model's formula at c = 1, d = y, o = 0 (1 * x and x + 0 are exact), a runtime choice of what is staged.
//
// Loop order: k_glm_pw's turned round.  A wave owns ONE tile of 16 consecutive draws (chains n0 .. n0 + 15 of one (Dt, N)
// slab): the B operand of K-step s -- row 4s + g, chain lane & 15, KS = DP / 4 doubles per lane -- is loaded once and stays
// in registers for the whole walk, and the per-draw constants (exp(-2 theta), or phi and lgamma(phi)) are formed once.  The four
// waves of a workgroup (64 draws) walk the same observation blocks: LLB blocks of 16 observations at a time, their
// first-product fragments P1 of the packed design image (glm_pack, glm_host.cpp; P2 is not read) and their c | d | o values
// staged through LDS between two barriers and shared by the four waves, as k_glm stages X.  The eta tile comes out with
// register r = observations {4r + g} of the lane's own draw; the link runs in the lane, which adds its terms in block order
// into ONE double; at the end the four g groups are summed by two __shfl_xor steps (16, then 32).  blockIdx.y cuts the
// (padded) observation blocks into `ranges`, so that a small population still fills the chip; k_glm_ll_merge adds the
// partials [ranges][S * N] in index order: no atomics, and for a given `ranges` every bit is the same from run to run.
//
// Rows.  Only rows below the coefficient count Dx are loaded as coefficients; rows Dx .. DP-1 of the B operand are an exact 0 (a
// SELECT on the row index, the address clamped to a valid row), so a t row at +-inf or a sampled theta changes no bit.  A sampled
// theta is read from its own row (trow), a held one comes from the handle.  Draws are on the natural scale.
// Padding rows: the image is padded to a multiple of 4 blocks; a row i >= M is SELECTED out (in the plain model it has c = 1,
// d = 0, eta = 0 and would add log 2 or 1).  A row of weight 0 (c = d = 0; dispersion families: c = 0) adds exactly 0 whatever
// b(eta) gave: a select, not a product, so a NaN there does not reach the sum.  Tail tile of a slab: lanes past N compute on a
// clamped chain and write nothing; a wave whose tile is past the last one does the same (it still meets every barrier).
// Non-finite draws stay in their own column of the product: ll = -inf gives +inf, a NaN gives NaN, for that draw only.
//
// Shipped: NT = DP / 16 in {1, 2, 4, 8} for logistic, poisson and gaussian, {1, 2, 4} for negbinomial -- the shapes the handles
// themselves are shipped in (glm_max_dim).  None reserves scratch (profiles/glm_loglik_resources.txt).
#include <cmath>

#include "pbbi_internal.h"

namespace {

typedef double ll_v4 __attribute__((ext_vector_type(4)));
typedef double ll_v2 __attribute__((ext_vector_type(2)));

constexpr int LL_BLOCK = 256;  // 4 waves, one tile of 16 draws each

// observation blocks staged per barrier pair: 32 KiB of fragments at NT = 4 and 8
template <int NT> struct LlStage { static constexpr int LB = NT <= 4 ? 4 : 2; };

struct LlPrm {
    const double* img;   // the packed design image; block b starts at b * blk_len, P1 first
    const double* c;     // per-observation streams, zero padded to the image's blocks; c == nullptr: the plain model, d = y
    const double* d;
    const double* o;
    const double* sdn;   // S slabs (Dt, N)
    double* part;        // [ranges][S * N]
    int64_t M, N, blk_len, ntile, tiles;  // ntile = tiles per slab, tiles = S * ntile
    int64_t slab_len;    // Dt * N
    int64_t nblk;        // blocks of the image (a multiple of 4)
    int64_t total;       // S * N
    double theta;        // the held log-dispersion
    int Dx;              // coefficient rows
    int trow;            // the state row of a sampled theta, -1: held (or no dispersion)
    int ranges;
};

// log Gamma for x > 0 as kernels_glm.hip's glm_lgamma states it
__device__ __forceinline__ double ll_lgamma(double x) {
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

// per draw: gaussian a = tau = exp(-2 theta); negbinomial a = phi = exp(theta), c = lgamma(phi) (glm_disp_chain)
struct LlDraw { double theta, a, c; };

template <int FAM>
__device__ __forceinline__ LlDraw ll_draw(double theta) {
    LlDraw k{theta, 0.0, 0.0};
    if constexpr (FAM == PBBI_GLM_GAUSSIAN) {
        k.a = exp(-2.0 * theta);
    } else if constexpr (FAM == PBBI_GLM_NEGBINOMIAL) {
        k.a = exp(theta);
        k.c = ll_lgamma(k.a);
    }
    return k;
}

// the energy term of k_glm of one observation at one draw; `on` = the row has weight
template <int FAM>
__device__ __forceinline__ double ll_link(double eta, double cv, double dv, const LlDraw& k, bool& on) {
    if constexpr (FAM == PBBI_GLM_LOGISTIC) {  // glm_link_rich: c ((eta > 0 ? eta : 0) + log1p(e)) - d eta
        const double e = exp(-fabs(eta));
        on = !(cv == 0.0 && dv == 0.0);
        return cv * ((eta > 0.0 ? eta : 0.0) + log1p(e)) - dv * eta;
    } else if constexpr (FAM == PBBI_GLM_POISSON) {  // c e - d eta
        const double e = exp(eta);
        on = !(cv == 0.0 && dv == 0.0);
        return cv * e - dv * eta;
    } else if constexpr (FAM == PBBI_GLM_GAUSSIAN) {  // glm_link_disp: c (0.5 tau r^2 + theta), d = y
        const double r = dv - eta;
        const double tr = k.a * r;
        const double trr = tr * r;
        on = cv != 0.0;
        return cv * (0.5 * trr + k.theta);
    } else {  // c (lgamma(phi) - lgamma(y + phi) + (y + phi) softplus(z) - y z), z = eta - theta
        const double z = eta - k.theta;
        const double e = exp(-fabs(z));
        const double ope = 1.0 + e;
        const double sp = (z > 0.0 ? z : 0.0) + log(ope);
        const double yp = dv + k.a;
        on = cv != 0.0;
        return cv * (((k.c - ll_lgamma(yp)) + yp * sp) - dv * z);
    }
}

template <int NT, int FAM>
__global__ void __launch_bounds__(LL_BLOCK) k_glm_ll(LlPrm prm) {
    constexpr int KS = 4 * NT;
    constexpr int LB = LlStage<NT>::LB;
    constexpr int P1V = (KS / 2) * 64;  // 16-byte elements of one block's P1
    constexpr bool DISP = FAM == PBBI_GLM_GAUSSIAN || FAM == PBBI_GLM_NEGBINOMIAL;
    __shared__ __attribute__((aligned(16))) ll_v2 lds[LB * P1V];
    __shared__ double olds[3 * LB * 16];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4;
    const int c = lane & 15;

    // ---- the wave's tile of 16 draws: the B operand and the per-draw constants, once
    const int64_t t_own = (int64_t)blockIdx.x * 4 + wave;
    const bool tile_ok = t_own < prm.tiles;
    const int64_t t = tile_ok ? t_own : prm.tiles - 1;  // past the last tile: compute on it, write nothing
    const int64_t slab = t / prm.ntile, n0 = (t - slab * prm.ntile) * 16;
    const int64_t left = prm.N - n0;
    const bool valid = tile_ok && c < left;
    const int64_t chain = n0 + (c < left ? c : left - 1);  // ragged tail: compute on a clamped chain
    const double* __restrict__ col = prm.sdn + slab * prm.slab_len + chain;
    const int Dx = prm.Dx;
    double q[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int row = 4 * s + g;
        const double v = col[(int64_t)(row < Dx ? row : Dx - 1) * prm.N];
        q[s] = row < Dx ? v : 0.0;
    }
    [[maybe_unused]] LlDraw dk{0.0, 0.0, 0.0};
    if constexpr (DISP) dk = ll_draw<FAM>(prm.trow >= 0 ? col[(int64_t)prm.trow * prm.N] : prm.theta);

    // ---- the walk over this range's observation blocks, LB at a time
    const int64_t nstage = prm.nblk / LB;
    const int64_t s0 = nstage * (int64_t)blockIdx.y / prm.ranges, s1 = nstage * ((int64_t)blockIdx.y + 1) / prm.ranges;
    double acc = 0.0;
    for (int64_t sg = s0; sg < s1; ++sg) {
        const int64_t blk0 = sg * LB;
        __syncthreads();  // the previous stage has been read
#pragma unroll
        for (int bi = 0; bi < LB; ++bi) {
            const ll_v2* __restrict__ src = reinterpret_cast<const ll_v2*>(prm.img + (blk0 + bi) * prm.blk_len);
            for (int i = threadIdx.x; i < P1V; i += LL_BLOCK) lds[bi * P1V + i] = src[i];
        }
        if (threadIdx.x < 3 * LB * 16) {
            const int st = threadIdx.x / (LB * 16), i = threadIdx.x % (LB * 16);
            const int64_t at = blk0 * 16 + i;
            double v;
            if (prm.c) v = (st == 0 ? prm.c : st == 1 ? prm.d : prm.o)[at];
            else v = st == 0 ? 1.0 : st == 1 ? prm.d[at] : 0.0;
            olds[threadIdx.x] = v;
        }
        __syncthreads();
#pragma unroll
        for (int bi = 0; bi < LB; ++bi) {
            const ll_v2* __restrict__ P1 = lds + bi * P1V + lane;
            ll_v4 eta = ll_v4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s2 = 0; s2 < KS / 2; ++s2) {
                const ll_v2 A = P1[s2 * 64];
                eta = __builtin_amdgcn_mfma_f64_16x16x4f64(A.x, q[2 * s2], eta, 0, 0, 0);
                eta = __builtin_amdgcn_mfma_f64_16x16x4f64(A.y, q[2 * s2 + 1], eta, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = bi * 16 + 4 * r + g;
                bool on;
                const double u = ll_link<FAM>(eta[r] + olds[2 * LB * 16 + i], olds[i], olds[LB * 16 + i], dk, on);
                // weight 0 and the image's padding rows: exactly nothing, whatever b() gave
                acc += (on && blk0 * 16 + i < prm.M) ? u : 0.0;
            }
        }
    }
    // ---- the four g groups of the lane's draw, in a fixed order
    acc += __shfl_xor(acc, 16, 64);
    acc += __shfl_xor(acc, 32, 64);
    if (valid && g == 0) prm.part[(int64_t)blockIdx.y * prm.total + slab * prm.N + chain] = acc;
}

// the ranges of one draw in index order
__global__ void __launch_bounds__(256) k_glm_ll_merge(const double* __restrict__ part, int64_t total, int ranges,
                                                       double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    double s = part[i];
    for (int r = 1; r < ranges; ++r) s += part[(int64_t)r * total + i];
    out[i] = s;
}

// c <- beta c0 (and d <- beta d0 where d holds a y) over the streams' padded length; beta from the device when beta_dev is given
__global__ void __launch_bounds__(256) k_glm_power(const double* __restrict__ obs0, double* __restrict__ obs, int64_t len,
                                                    int scale_d, double beta, const double* __restrict__ beta_dev) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    const double b = beta_dev ? *beta_dev : beta;
    obs[i] = b * obs0[i];
    if (scale_d) obs[len + i] = b * obs0[len + i];
}

}  // namespace

extern "C" int pbbi_loglik_glm_check(int handle, int family, int state_dim, const void* sdn, const void* out, int S, int Dt,
                                     int64_t N, int ranges) {
    return glm_check_loglik(handle, family, state_dim, sdn, out, S, Dt, N, ranges);
}

extern "C" int pbbi_loglik_glm(const pbbi_potential* pot, const void* sdn, int S, int Dt, int64_t N, int ranges,
                               double* ulik_out, void* stream) {
    // every rule, before the device is touched (glm_host.cpp)
    if (int rc = glm_check_loglik(pot ? (pot->kind == KIND_GLM ? 1 : 2) : 0, pot ? pot->glm_family : 0, pot ? pot->D : 0, sdn,
                                  ulik_out, S, Dt, N, ranges))
        return rc;
    if (pot->dtype != PBBI_F64 || pot->glm_DP == 0 || !pot->d_glm_img)
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, "pbbi_loglik_glm: a built fp64 GLM handle");
    DeviceGuard guard(pot->device);
    if (!guard.ok) return pbbi_fail(PBBI_ERR_HIP, "pbbi_loglik_glm: cannot select the handle's device");
    hipStream_t st = (hipStream_t)stream;
    const int NT = pot->glm_DP / 16, fam = pot->glm_family;
    const int64_t M = pot->glm_M, nblk = glm_blocks_padded(M), olen = nblk * 16;

    LlPrm prm{};
    prm.img = (const double*)pot->d_glm_img;
    if (pot->glm_variant == GLM_V_PLAIN) {
        prm.c = nullptr; prm.d = (const double*)pot->d_glm_y; prm.o = nullptr;
    } else {  // the likelihood at power 1: a tempered handle keeps its streams as built
        prm.c = (const double*)(pot->d_glm_obs0 ? pot->d_glm_obs0 : pot->d_glm_obs); prm.d = prm.c + olen; prm.o = prm.d + olen;
    }
    prm.sdn = (const double*)sdn;
    prm.M = M; prm.N = N;
    prm.blk_len = (int64_t)pot->glm_DP * 32;
    prm.ntile = (N + 15) / 16;
    prm.tiles = (int64_t)S * prm.ntile;
    prm.slab_len = (int64_t)Dt * N;
    prm.total = (int64_t)S * N;
    prm.nblk = nblk;
    prm.theta = pot->glm_theta;
    prm.trow = pot->glm_trow;
    prm.Dx = pot->D - pot->glm_hier_J - (pot->glm_trow >= 0 ? 1 : 0);
    const int64_t groups = (prm.tiles + 3) / 4;
    if (groups > 0x7fffffff) return pbbi_fail(PBBI_ERR_UNSUPPORTED, "pbbi_loglik_glm: more than 2^31 workgroups of 64 draws");
    if (ranges == 0) {  // enough workgroups for the chip, at least one stage of blocks per range, at most 64 ranges
        const int64_t nstage = nblk / (NT <= 4 ? 4 : 2);
        int64_t r = (1024 + groups - 1) / groups;
        if (r > nstage) r = nstage;
        ranges = (int)(r < 1 ? 1 : r > 64 ? 64 : r);
    }
    prm.ranges = ranges;

    double* part = nullptr;
    PBBI_HIP(hipMallocAsync((void**)&part, sizeof(double) * (size_t)ranges * (size_t)prm.total, st));
    prm.part = part;
    const dim3 grid((unsigned)groups, (unsigned)ranges), block(LL_BLOCK);
    bool done = false;
#define LL_CASE(NT_, FAM_)                                                              \
    if (NT == NT_ && fam == FAM_) {                                                     \
        hipLaunchKernelGGL((k_glm_ll<NT_, FAM_>), grid, block, 0, st, prm);             \
        done = true;                                                                    \
    }
    LL_CASE(1, PBBI_GLM_LOGISTIC) LL_CASE(2, PBBI_GLM_LOGISTIC) LL_CASE(4, PBBI_GLM_LOGISTIC) LL_CASE(8, PBBI_GLM_LOGISTIC)
    LL_CASE(1, PBBI_GLM_POISSON) LL_CASE(2, PBBI_GLM_POISSON) LL_CASE(4, PBBI_GLM_POISSON) LL_CASE(8, PBBI_GLM_POISSON)
    LL_CASE(1, PBBI_GLM_GAUSSIAN) LL_CASE(2, PBBI_GLM_GAUSSIAN) LL_CASE(4, PBBI_GLM_GAUSSIAN) LL_CASE(8, PBBI_GLM_GAUSSIAN)
    LL_CASE(1, PBBI_GLM_NEGBINOMIAL) LL_CASE(2, PBBI_GLM_NEGBINOMIAL) LL_CASE(4, PBBI_GLM_NEGBINOMIAL)
#undef LL_CASE
    if (done)
        hipLaunchKernelGGL(k_glm_ll_merge, dim3((unsigned)((prm.total + 255) / 256)), dim3(256), 0, st, (const double*)part,
                           prm.total, ranges, ulik_out);
    const hipError_t launched = hipGetLastError();
    PBBI_HIP(hipFreeAsync(part, st));
    if (!done) return pbbi_fail(PBBI_ERR_UNSUPPORTED, "pbbi_loglik_glm: no kernel is shipped for this handle's family and "
                                                      "padded state dimension");
    PBBI_HIP(launched);
    return PBBI_OK;
}

// ---- the likelihood power of a handle with observation streams
static int power_handle_kind(const pbbi_potential* pot) { return pot ? (pot->kind == KIND_GLM ? 1 : 2) : 0; }
static int power_has_streams(const pbbi_potential* pot) {
    return pot && pot->kind == KIND_GLM && pot->glm_variant != GLM_V_PLAIN && pot->glm_variant != GLM_V_SOFTMAX &&
           pot->d_glm_obs != nullptr;
}

extern "C" int pbbi_likelihood_power_check(int handle, int family, int has_streams, double beta, int beta_on_device) {
    return glm_check_power(handle, family, has_streams != 0, beta, beta_on_device != 0);
}

extern "C" int pbbi_potential_set_likelihood_power(pbbi_potential* pot, double beta, const double* beta_dev, void* stream) {
    if (int rc = glm_check_power(power_handle_kind(pot), pot ? pot->glm_family : 0, power_has_streams(pot), beta,
                                 beta_dev != nullptr))
        return rc;
    DeviceGuard guard(pot->device);
    if (!guard.ok) return pbbi_fail(PBBI_ERR_HIP, "pbbi_potential_set_likelihood_power: cannot select the handle's device");
    hipStream_t st = (hipStream_t)stream;
    const int64_t len = glm_blocks_padded(pot->glm_M) * 16;
    if (!pot->d_glm_obs0) {  // the streams as built, kept from the first tempering on
        void* keep = nullptr;
        PBBI_HIP(hipMalloc(&keep, sizeof(double) * (size_t)(3 * len)));
        const hipError_t e = hipMemcpyAsync(keep, pot->d_glm_obs, sizeof(double) * (size_t)(3 * len), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) {
            (void)hipFree(keep);
            return pbbi_fail(PBBI_ERR_HIP, std::string("pbbi_potential_set_likelihood_power: ") + hipGetErrorString(e));
        }
        pot->d_glm_obs0 = keep;
    }
    const int scale_d = (pot->glm_family == PBBI_GLM_LOGISTIC || pot->glm_family == PBBI_GLM_POISSON) ? 1 : 0;
    hipLaunchKernelGGL(k_glm_power, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st, (const double*)pot->d_glm_obs0,
                       (double*)pot->d_glm_obs, len, scale_d, beta, beta_dev);
    PBBI_HIP(hipGetLastError());
    pot->glm_power = beta_dev ? NAN : beta;
    return PBBI_OK;
}

extern "C" int pbbi_potential_get_likelihood_power(const pbbi_potential* pot, double* beta_out) {
    if (!pot) return pbbi_fail(PBBI_ERR_INVALID, "potential handle is NULL");
    if (!beta_out) return pbbi_fail(PBBI_ERR_INVALID, "beta_out is NULL");
    *beta_out = pot->d_glm_obs0 ? pot->glm_power : 1.0;  // never tempered: 1
    return PBBI_OK;
}
