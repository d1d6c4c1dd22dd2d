// kernels_glm_pointwise.hip -- what a GLM handle says about T draws of its state, per observation, reduced over the draws on
// the device (gfx950): log sum_t exp(ll_it), the mean and the unbiased variance of ll_it over the draws, and the mean of the
// fitted mean -- the lppd, the WAIC penalty and the posterior predictive mean without an M x T matrix anywhere.
//
// ll_it is minus the per-observation energy term of k_glm (kernels_glm.hip), formed by the functions k_glm itself calls:
// glm_link_rich / glm_link_disp of glm_family_dev.h with want_u (glm_draw_uterm), the fitted mean by glm_mean beside them
// (tests/test_glm_pointwise.py holds sum_i mean_i to the U of pbbi_potential_eval on the same draws).  What this kernel shares
// with k_glm_ll (kernels_glm_loglik.hip) -- the common arguments, the tile of draws, the B operand, the staging, the eta tile, and
// on the host the filler, the preflight and the (NT, family) dispatch -- is glm_draws_dev.h; the plain model is a runtime choice
// of what is staged (there).
//
// Loop order: k_glm's, inverted.  A workgroup owns OB = 2 blocks of 16 observations: their first-product fragments P1 of the
// packed design image (glm_pack, glm_host.cpp; the second copy P2 is not read) and their c | d | o values are staged into LDS
// ONCE.  Its four waves then walk tiles of 16 consecutive draws (chains n0 .. n0 + 15 of one (Dt, N) slab) of the workgroup's
// draw range, wave w the tiles t0 + w, t0 + w + 4, ...: no barrier inside the walk.  The B operand of K-step s is row 4s + g,
// chain lane & 15 of the slab, loaded as it lies (the state layout of the samplers' output); the eta tile comes out with
// register r = observations {4r + g} of the lane's own draw.  The link and the accumulation run in the lane, which keeps 5
// doubles per observation across the whole walk:
//   m, s      the running maximum of ll and sum_t exp(ll_t - m): one exp per value; no fmax (a NaN must reach s)
//   mean, M2  Welford's recurrence; the count n is the lane's, one division per tile
//   mu        the sum of the fitted mean
// At the end of the walk: one butterfly over the 16 lanes that share g (Chan's merge for (n, mean, M2), the max-shifted merge
// for (m, s)), one merge of the four waves through LDS in wave order, and the partial of (draw range, observation) goes to
// the workspace.  k_glm_pw_merge folds the ranges in index order: no atomics, and for a given number of ranges every bit of
// the result is the same from run to run.
//
// Rows.  Rows Dx .. DP-1 of the B operand are an exact 0 (glm_draw_load), so the log-scales of a hierarchical handle or a
// sampled theta never meet the image's zero columns as 0 * inf.  A sampled theta is read from its own row (trow); a held one
// comes from the handle.  Draws are on the natural scale: a non-centred handle is served with (w; t) as the caller converted
// them.  Tail tile of a slab: lanes past N compute on a clamped chain and accumulate nothing.
//
// A row of weight 0 (c = d = 0, dispersion families: c = 0) has ll = 0 exactly, selected as in k_glm; its fitted mean is
// formed like any other row's.  Non-finite draws: ll = -inf leaves lse finite and makes mean and variance non-finite; a NaN
// reaches all four outputs.
#include <cmath>

#include "glm_draws_dev.h"

namespace {

constexpr int PW_BLOCK = GLM_DRAW_BLOCK;
constexpr int PW_OB = 2;       // observation blocks per workgroup
constexpr int PW_OBS = PW_OB * 16;
constexpr int PW_NV = 6;       // doubles of a partial: n, mean, M2, m, s, mu

struct PwPrm : GlmDrawPrm {
    double* part;  // [ranges][groups * PW_OBS][PW_NV]
};

// (m, s) <- (m, s) + one value x: s = sum exp(. - m).  x == m covers -inf beside -inf (the difference would be NaN); a NaN x
// compares false twice and reaches s through the exp.
__device__ __forceinline__ void pw_lse_add(double& m, double& s, double x) {
    const double e = (x == m) ? 1.0 : exp(-fabs(x - m));
    if (x > m) {
        s = s * e + 1.0;
        m = x;
    } else {
        s += e;
    }
}
// (ma, sa) <- (ma, sa) merged with (mb, sb)
__device__ __forceinline__ void pw_lse_merge(double& ma, double& sa, double mb, double sb) {
    const double m = ma > mb ? ma : mb;  // m, unlike s, is never NaN
    const double fa = (ma == m) ? 1.0 : exp(ma - m);
    const double fb = (mb == m) ? 1.0 : exp(mb - m);
    sa = sa * fa + sb * fb;
    ma = m;
}
// Chan's merge of (na, mean, M2) with (nb, .., ..); an empty side is SELECTED out
__device__ __forceinline__ void pw_chan_merge(double na, double& mean_a, double& M2a, double nb, double mean_b, double M2b) {
    const double n = na + nb;
    const double w = n > 0.0 ? nb / n : 0.0;
    const double delta = mean_b - mean_a;
    const double mean = mean_a + delta * w;
    const double M2 = (M2a + M2b) + (delta * delta) * (na * w);
    const bool ea = na == 0.0, eb = nb == 0.0;
    mean_a = eb ? mean_a : ea ? mean_b : mean;
    M2a = eb ? M2a : ea ? M2b : M2;
}

template <int NT, int FAM>
__global__ void __launch_bounds__(PW_BLOCK) k_glm_pw(PwPrm prm) {
    constexpr int KS = 4 * NT;
    constexpr int P1V = (KS / 2) * 64;  // 16-byte elements of one block's P1
    __shared__ __attribute__((aligned(16))) glm_v2 lds[PW_OB * P1V];
    __shared__ double olds[3 * PW_OBS];
    __shared__ double red[4 * PW_OBS * PW_NV];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4;
    const int c = lane & 15;
    const int64_t blk0 = (int64_t)blockIdx.x * PW_OB;  // the image is padded to a multiple of 4 blocks: blk0 + 1 is inside it

    // ---- stage the group's fragments and values once
    glm_draw_stage<PW_OB, P1V>(prm, blk0, lds, olds);
    __syncthreads();
    double cv[PW_OB][4], dv[PW_OB][4], ov[PW_OB][4];
#pragma unroll
    for (int bi = 0; bi < PW_OB; ++bi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = bi * 16 + 4 * r + g;
            cv[bi][r] = olds[i]; dv[bi][r] = olds[PW_OBS + i]; ov[bi][r] = olds[2 * PW_OBS + i];
        }

    double am[PW_OB][4], as[PW_OB][4], amean[PW_OB][4], aM2[PW_OB][4], amu[PW_OB][4];
#pragma unroll
    for (int bi = 0; bi < PW_OB; ++bi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            am[bi][r] = -INFINITY; as[bi][r] = 0.0; amean[bi][r] = 0.0; aM2[bi][r] = 0.0; amu[bi][r] = 0.0;
        }
    double n = 0.0;

    // ---- the walk over this range's draw tiles
    const int64_t t0 = prm.tiles * (int64_t)blockIdx.y / prm.ranges, t1 = prm.tiles * ((int64_t)blockIdx.y + 1) / prm.ranges;
    for (int64_t t = t0 + wave; t < t1; t += 4) {
        const GlmDrawTile tile = glm_draw_tile(prm, t, c);
        const bool valid = tile.valid;
        double q[KS];
        glm_draw_load<KS>(prm, tile.col, g, q);
        const GlmDrawChain<FAM> dk = glm_draw_disp<FAM>(prm, tile.col);
        const double ninv = 1.0 / (n + 1.0);
#pragma unroll
        for (int bi = 0; bi < PW_OB; ++bi) {
            const glm_v4 eta = glm_draw_eta<KS>(lds + bi * P1V + lane, q);
            if (valid) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double e = eta[r] + ov[bi][r];
                    const double mu = glm_draw_mean<FAM>(e, dk);
                    double ll = -glm_draw_uterm<FAM>(e, cv[bi][r], dv[bi][r], dk);
                    ll = glm_row_on<FAM>(cv[bi][r], dv[bi][r]) ? ll : 0.0;  // weight 0: exactly nothing, whatever b() gave
                    pw_lse_add(am[bi][r], as[bi][r], ll);
                    const double delta = ll - amean[bi][r];
                    amean[bi][r] += delta * ninv;
                    aM2[bi][r] += delta * (ll - amean[bi][r]);
                    amu[bi][r] += mu;
                }
            }
        }
        n += valid ? 1.0 : 0.0;
    }

    // ---- the 16 lanes of each g row, then the four waves in wave order
#pragma unroll
    for (int bi = 0; bi < PW_OB; ++bi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double nn = n;
#pragma unroll
            for (int mask = 1; mask < 16; mask <<= 1) {
                const double nb = __shfl_xor(nn, mask, 64);
                const double mean_b = __shfl_xor(amean[bi][r], mask, 64), M2b = __shfl_xor(aM2[bi][r], mask, 64);
                const double mb = __shfl_xor(am[bi][r], mask, 64), sb = __shfl_xor(as[bi][r], mask, 64);
                const double mub = __shfl_xor(amu[bi][r], mask, 64);
                // the lower lane of a pair is "a" on both sides, so both lanes hold the same bits
                const bool lo = (lane & mask) == 0;
                double ma_ = lo ? amean[bi][r] : mean_b, M2a_ = lo ? aM2[bi][r] : M2b;
                pw_chan_merge(lo ? nn : nb, ma_, M2a_, lo ? nb : nn, lo ? mean_b : amean[bi][r], lo ? M2b : aM2[bi][r]);
                double lm = lo ? am[bi][r] : mb, ls = lo ? as[bi][r] : sb;
                pw_lse_merge(lm, ls, lo ? mb : am[bi][r], lo ? sb : as[bi][r]);
                amu[bi][r] = lo ? amu[bi][r] + mub : mub + amu[bi][r];
                amean[bi][r] = ma_; aM2[bi][r] = M2a_; am[bi][r] = lm; as[bi][r] = ls;
                nn += nb;
            }
            if (c == 0) {
                double* dst = red + ((size_t)wave * PW_OBS + (bi * 16 + 4 * r + g)) * PW_NV;
                dst[0] = nn; dst[1] = amean[bi][r]; dst[2] = aM2[bi][r]; dst[3] = am[bi][r]; dst[4] = as[bi][r];
                dst[5] = amu[bi][r];
            }
        }
    __syncthreads();
    if (threadIdx.x < PW_OBS) {
        const double* a = red + (size_t)threadIdx.x * PW_NV;
        double nn = a[0], mean = a[1], M2 = a[2], m = a[3], s = a[4], mu = a[5];
        for (int w = 1; w < 4; ++w) {
            const double* b = red + ((size_t)w * PW_OBS + threadIdx.x) * PW_NV;
            pw_chan_merge(nn, mean, M2, b[0], b[1], b[2]);
            pw_lse_merge(m, s, b[3], b[4]);
            mu += b[5];
            nn += b[0];
        }
        double* dst = prm.part + (((size_t)blockIdx.y * gridDim.x + blockIdx.x) * PW_OBS + threadIdx.x) * PW_NV;
        dst[0] = nn; dst[1] = mean; dst[2] = M2; dst[3] = m; dst[4] = s; dst[5] = mu;
    }
}

// the ranges of one observation in index order; lse = m + log s, var = M2 / (n - 1)
__global__ void __launch_bounds__(256) k_glm_pw_merge(const double* __restrict__ part, int64_t M, int64_t stride, int ranges,
                                                       double* lse_out, double* mean_out, double* var_out, double* mu_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const double* a = part + (size_t)i * PW_NV;
    double nn = a[0], mean = a[1], M2 = a[2], m = a[3], s = a[4], mu = a[5];
    for (int r = 1; r < ranges; ++r) {
        const double* b = part + ((size_t)r * stride + i) * PW_NV;
        pw_chan_merge(nn, mean, M2, b[0], b[1], b[2]);
        pw_lse_merge(m, s, b[3], b[4]);
        mu += b[5];
        nn += b[0];
    }
    if (lse_out) lse_out[i] = m + log(s);
    if (mean_out) mean_out[i] = mean;
    if (var_out) var_out[i] = M2 / (nn - 1.0);
    if (mu_out) mu_out[i] = mu / nn;
}

}  // namespace

extern "C" int pbbi_pointwise_glm_check(int handle, int family, int state_dim, const void* sdn, int S, int Dt, int64_t N,
                                        int ranges, int want_var) {
    return glm_check_pointwise(handle, family, state_dim, sdn, S, Dt, N, ranges, want_var != 0);
}

// the launches of pbbi_pointwise_glm, after glm_draw_entry's preflight
static int pw_run(const pbbi_potential* pot, const void* sdn, int S, int Dt, int64_t N, int ranges, double* lse_out,
                  double* mean_out, double* var_out, double* mu_out, hipStream_t st) {
    const int64_t M = pot->glm_M, nb = (M + 15) / 16, groups = (nb + PW_OB - 1) / PW_OB;
    PwPrm prm{};
    glm_draw_fill(prm, pot, sdn, S, Dt, N, false);
    if (ranges == 0) {  // enough workgroups for the chip, at least one tile per wave of a range, at most 64 ranges
        int64_t r = (2048 + groups - 1) / groups;
        if (r > prm.tiles / 4) r = prm.tiles / 4;
        ranges = (int)(r < 1 ? 1 : r > 64 ? 64 : r);
    }
    prm.ranges = ranges;

    double* part = nullptr;
    PBBI_HIP(hipMallocAsync((void**)&part, sizeof(double) * (size_t)ranges * (size_t)groups * PW_OBS * PW_NV, st));
    prm.part = part;
    const dim3 grid((unsigned)groups, (unsigned)ranges), block(PW_BLOCK);
    const bool done = glm_draw_dispatch(pot->glm_DP / 16, pot->glm_family, [&](auto nt, auto fam) {
        hipLaunchKernelGGL((k_glm_pw<decltype(nt)::value, decltype(fam)::value>), grid, block, 0, st, prm);
    });
    if (done)
        hipLaunchKernelGGL(k_glm_pw_merge, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, (const double*)part, M,
                           groups * PW_OBS, ranges, lse_out, mean_out, var_out, mu_out);
    const hipError_t launched = hipGetLastError();
    PBBI_HIP(hipFreeAsync(part, st));
    if (!done) return pbbi_fail(PBBI_ERR_UNSUPPORTED, "pbbi_pointwise_glm: no kernel is shipped for this handle's family and "
                                                      "padded state dimension");
    PBBI_HIP(launched);
    return PBBI_OK;
}

extern "C" int pbbi_pointwise_glm(const pbbi_potential* pot, const void* sdn, int S, int Dt, int64_t N, int ranges,
                                  double* lse_out, double* mean_out, double* var_out, double* mu_out, void* stream) {
    return glm_draw_entry(
        "pbbi_pointwise_glm", pot,
        [&](int handle, int family, int state_dim) {
            return glm_check_pointwise(handle, family, state_dim, sdn, S, Dt, N, ranges, var_out != nullptr);
        },
        [&] { return pw_run(pot, sdn, S, Dt, N, ranges, lse_out, mean_out, var_out, mu_out, (hipStream_t)stream); });
}
