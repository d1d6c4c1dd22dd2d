// kernels_glm_loglik.hip -- the likelihood energy of each of S * N draws of a GLM handle's state (gfx950):
//   ulik[s * N + n] = sum_i U_i(draw)
// the likelihood part of k_glm's U (kernels_glm.hip) -- minus the log-likelihood with the constants k_i dropped as k_glm
// drops them -- without the prior, the group-scale terms or theta's prior.  It is what a likelihood-tempered SMC sampler
// (smc.LikelihoodTemperedSMC) weighs its particles by at every stage: an M x D x T product on the fp64 matrix cores.
// The same file holds the kernel that scales a handle's observation streams by a likelihood power
// (pbbi_potential_set_likelihood_power): pi_beta(w) ~ p(w) L(w)^beta is the full model with every weight a_i times beta.
//
// U_i is formed by the functions k_glm itself calls: glm_link_rich / glm_link_disp of glm_family_dev.h with want_u
// (glm_draw_uterm; tests/test_glm_loglik.py holds ulik + prior to the U of pbbi_potential_eval on the same draws).  What this
// kernel shares with k_glm_pw (kernels_glm_pointwise.hip) -- the common arguments, the tile of draws, the B operand, the staging,
// the eta tile, and on the host the filler, the preflight and the (NT, family) dispatch -- is glm_draws_dev.h; the plain model
// is a runtime choice of what is staged (there).
//
// Loop order: k_glm_pw's turned round.  A wave owns ONE tile of 16 consecutive draws (chains n0 .. n0 + 15 of one (Dt, N)
// slab): the B operand of K-step s -- row 4s + g, chain lane & 15, KS = DP / 4 doubles per lane -- is loaded once and stays
// in registers for the whole walk, and the per-draw constants (exp(-2 theta), phi and lgamma(phi), or the Gamma's) are formed once.  The four
// waves of a workgroup (64 draws) walk the same observation blocks: LLB blocks of 16 observations at a time, their
// first-product fragments P1 of the packed design image (glm_pack, glm_host.cpp; P2 is not read) and their c | d | o values
// staged through LDS between two barriers and shared by the four waves, as k_glm stages X.  The eta tile comes out with
// register r = observations {4r + g} of the lane's own draw; the link runs in the lane, which adds its terms in block order
// into ONE double; at the end the four g groups are summed by two __shfl_xor steps (16, then 32).  blockIdx.y cuts the
// (padded) observation blocks into `ranges`, so that a small population still fills the chip; k_glm_ll_merge adds the
// partials [ranges][S * N] in index order: no atomics, and for a given `ranges` every bit is the same from run to run.
//
// Rows.  Rows Dx .. DP-1 of the B operand are an exact 0 (glm_draw_load), so a t row at +-inf or a sampled theta changes no bit.
// A sampled theta is read from its own row (trow), a held one comes from the handle.  Draws are on the natural scale.
// Padding rows: the image is padded to a multiple of 4 blocks; a row i >= M is SELECTED out (in the plain model it has c = 1,
// d = 0, eta = 0 and would add log 2 or 1).  A row of weight 0 (c = d = 0; dispersion families: c = 0) adds exactly 0 whatever
// b(eta) gave: a select, not a product, so a NaN there does not reach the sum.  Tail tile of a slab: lanes past N compute on a
// clamped chain and write nothing; a wave whose tile is past the last one does the same (it still meets every barrier).
// Non-finite draws stay in their own column of the product: ll = -inf gives +inf, a NaN gives NaN, for that draw only.
//
// Shipped: the 22 shapes of glm_draw_dispatch.  None reserves scratch (profiles/glm_loglik_resources.txt, the Gamma's four in
// profiles/glm_gamma_resources.txt, the ordinal family's three in profiles/glm_ordinal_resources.txt).
#include <cmath>

#include "glm_draws_dev.h"

namespace {

constexpr int LL_BLOCK = GLM_DRAW_BLOCK;  // 4 waves, one tile of 16 draws each

// observation blocks staged per barrier pair: 32 KiB of fragments at NT = 4 and 8
template <int NT> struct LlStage { static constexpr int LB = NT <= 4 ? 4 : 2; };

struct LlPrm : GlmDrawPrm {
    double* part;   // [ranges][S * N]
    int64_t nblk;   // blocks of the image (a multiple of 4)
    int64_t total;  // S * N
};

template <int NT, int FAM>
__global__ void __launch_bounds__(LL_BLOCK) k_glm_ll(LlPrm prm) {
    constexpr int KS = 4 * NT;
    constexpr int LB = LlStage<NT>::LB;
    constexpr int P1V = (KS / 2) * 64;  // 16-byte elements of one block's P1
    __shared__ __attribute__((aligned(16))) glm_v2 lds[LB * P1V];
    __shared__ double olds[3 * LB * 16];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4;
    const int c = lane & 15;

    // ---- the wave's tile of 16 draws: the B operand and the per-draw constants, once
    const int64_t t_own = (int64_t)blockIdx.x * 4 + wave;
    const bool tile_ok = t_own < prm.tiles;
    const int64_t t = tile_ok ? t_own : prm.tiles - 1;  // past the last tile: compute on it, write nothing
    const GlmDrawTile tile = glm_draw_tile(prm, t, c);
    const bool valid = tile_ok && tile.valid;
    double q[KS];
    glm_draw_load<KS>(prm, tile.col, g, q);
    const GlmDrawChain<FAM> dk = glm_draw_disp<FAM>(prm, tile.col);

    // ---- the walk over this range's observation blocks, LB at a time
    const int64_t nstage = prm.nblk / LB;
    const int64_t s0 = nstage * (int64_t)blockIdx.y / prm.ranges, s1 = nstage * ((int64_t)blockIdx.y + 1) / prm.ranges;
    double acc = 0.0;
    for (int64_t sg = s0; sg < s1; ++sg) {
        const int64_t blk0 = sg * LB;
        __syncthreads();  // the previous stage has been read
        glm_draw_stage<LB, P1V>(prm, blk0, lds, olds);
        __syncthreads();
#pragma unroll
        for (int bi = 0; bi < LB; ++bi) {
            const glm_v4 eta = glm_draw_eta<KS>(lds + bi * P1V + lane, q);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = bi * 16 + 4 * r + g;
                const double cv = olds[i], dv = olds[LB * 16 + i];
                const double u = glm_draw_uterm<FAM>(eta[r] + olds[2 * LB * 16 + i], cv, dv, dk);
                // weight 0 and the image's padding rows: exactly nothing, whatever b() gave
                acc += (glm_row_on<FAM>(cv, dv) && blk0 * 16 + i < prm.M) ? u : 0.0;
            }
        }
    }
    // ---- the four g groups of the lane's draw, in a fixed order
    acc += __shfl_xor(acc, 16, 64);
    acc += __shfl_xor(acc, 32, 64);
    if (valid && g == 0) prm.part[(int64_t)blockIdx.y * prm.total + tile.slab * prm.N + tile.chain] = acc;
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

// the ordinal family's weighted category counts, which its gradient reads beside the streams: A_k <- beta A_k as built
// (tail: 8 current values, then the 8 as built -- the end of the handle's prior table)
__global__ void __launch_bounds__(64) k_glm_power_counts(double* __restrict__ tail, double beta, const double* __restrict__ beta_dev) {
    if (threadIdx.x < 8) tail[threadIdx.x] = (beta_dev ? *beta_dev : beta) * tail[8 + threadIdx.x];
}

}  // namespace

extern "C" int pbbi_loglik_glm_check(int handle, int family, int state_dim, const void* sdn, const void* out, int S, int Dt,
                                     int64_t N, int ranges) {
    return glm_check_loglik(handle, family, state_dim, sdn, out, S, Dt, N, ranges);
}

// the launches of pbbi_loglik_glm, after glm_draw_entry's preflight
static int ll_run(const pbbi_potential* pot, const void* sdn, int S, int Dt, int64_t N, int ranges, double* ulik_out,
                  hipStream_t st) {
    const int NT = pot->glm_DP / 16;
    LlPrm prm{};
    glm_draw_fill(prm, pot, sdn, S, Dt, N, true);  // the likelihood at power 1: a tempered handle's streams as built
    prm.total = (int64_t)S * N;
    prm.nblk = glm_blocks_padded(pot->glm_M);
    const int64_t groups = (prm.tiles + 3) / 4;
    if (groups > 0x7fffffff) return pbbi_fail(PBBI_ERR_UNSUPPORTED, "pbbi_loglik_glm: more than 2^31 workgroups of 64 draws");
    if (ranges == 0) {  // enough workgroups for the chip, at least one stage of blocks per range, at most 64 ranges
        const int64_t nstage = prm.nblk / (NT <= 4 ? 4 : 2);
        int64_t r = (1024 + groups - 1) / groups;
        if (r > nstage) r = nstage;
        ranges = (int)(r < 1 ? 1 : r > 64 ? 64 : r);
    }
    prm.ranges = ranges;

    double* part = nullptr;
    PBBI_HIP(hipMallocAsync((void**)&part, sizeof(double) * (size_t)ranges * (size_t)prm.total, st));
    prm.part = part;
    const dim3 grid((unsigned)groups, (unsigned)ranges), block(LL_BLOCK);
    const bool done = glm_draw_dispatch(NT, pot->glm_family, [&](auto nt, auto fam) {
        hipLaunchKernelGGL((k_glm_ll<decltype(nt)::value, decltype(fam)::value>), grid, block, 0, st, prm);
    });
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

extern "C" int pbbi_loglik_glm(const pbbi_potential* pot, const void* sdn, int S, int Dt, int64_t N, int ranges,
                               double* ulik_out, void* stream) {
    return glm_draw_entry(
        "pbbi_loglik_glm", pot,
        [&](int handle, int family, int state_dim) {
            return glm_check_loglik(handle, family, state_dim, sdn, ulik_out, S, Dt, N, ranges);
        },
        [&] { return ll_run(pot, sdn, S, Dt, N, ranges, ulik_out, (hipStream_t)stream); });
}

// ---- the likelihood power of a handle with observation streams
static int power_has_streams(const pbbi_potential* pot) {
    return pot && pot->kind == KIND_GLM && pot->glm_variant != GLM_V_PLAIN && pot->glm_variant != GLM_V_SOFTMAX &&
           pot->d_glm_obs != nullptr;
}

extern "C" int pbbi_likelihood_power_check(int handle, int family, int has_streams, double beta, int beta_on_device) {
    return glm_check_power(handle, family, has_streams != 0, beta, beta_on_device != 0);
}

extern "C" int pbbi_potential_set_likelihood_power(pbbi_potential* pot, double beta, const double* beta_dev, void* stream) {
    if (int rc = glm_check_power(glm_handle_kind(pot), pot ? pot->glm_family : 0, power_has_streams(pot), beta,
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
    if (pot->glm_variant == GLM_V_ORDINAL)
        hipLaunchKernelGGL(k_glm_power_counts, dim3(1), dim3(64), 0, st, (double*)pot->d_glm_prior + 2 * pot->glm_DP, beta, beta_dev);
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
