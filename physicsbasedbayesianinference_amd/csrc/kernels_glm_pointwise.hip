// kernels_glm_pointwise.hip -- what a GLM handle says about T draws of its state, per observation, reduced over the draws on
// the device (gfx950): log sum_t exp(ll_it), the mean and the unbiased variance of ll_it over the draws, and the mean of the
// fitted mean -- the lppd, the WAIC penalty and the posterior predictive mean without an M x T matrix anywhere.
//
// ll_it is minus the per-observation energy term of k_glm (kernels_glm.hip): glm_link / glm_link_rich / glm_link_disp with
// want_u.  That file is not touched and shares no header with this one: the link formulas and glm_lgamma are RESTATED below,
// operation for operation (pw_link, pw_lgamma; tests/test_glm_pointwise.py holds sum_i mean_i to the U of pbbi_potential_eval on the
// same draws).  The plain model is the full model's formula at c = 1, d = y, o = 0, which is the plain formula bit for bit
// (1 * x and x + 0 are exact), so the model is a runtime choice of what is staged, not an instantiation.
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
// Rows.  Only rows below the coefficient count Dx are loaded as coefficients; rows Dx .. DP-1 of the B operand are an exact 0
// (a SELECT on the row index, the address clamped to a valid row), so the log-scales of a hierarchical handle or a sampled
// theta -- which sit behind zero columns of the image -- never meet those zeros as 0 * inf.  A sampled theta is read from
// its own row (trow); a held one comes from the handle.  Draws are on the natural scale: a non-centred handle is served with
// (w; t) as the caller converted them.  Tail tile of a slab: lanes past N compute on a clamped chain and accumulate nothing.
//
// A row of weight 0 (c = d = 0, dispersion families: c = 0) has ll = 0 exactly, selected as in k_glm; its fitted mean is
// formed like any other row's.  Non-finite draws: ll = -inf leaves lse finite and makes mean and variance non-finite; a NaN
// reaches all four outputs.
#include <cmath>

#include "pbbi_internal.h"

namespace {

typedef double pw_v4 __attribute__((ext_vector_type(4)));
typedef double pw_v2 __attribute__((ext_vector_type(2)));

constexpr int PW_BLOCK = 256;  // 4 waves
constexpr int PW_OB = 2;       // observation blocks per workgroup
constexpr int PW_OBS = PW_OB * 16;
constexpr int PW_NV = 6;       // doubles of a partial: n, mean, M2, m, s, mu

struct PwPrm {
    const double* img;   // the packed design image; block b starts at b * blk_len, P1 first
    const double* c;     // per-observation streams, zero padded to the image's blocks; c == nullptr: the plain model, d = y
    const double* d;
    const double* o;
    const double* sdn;   // S slabs (Dt, N)
    double* part;        // [ranges][groups * PW_OBS][PW_NV]
    int64_t M, N, blk_len, ntile, tiles;  // ntile = tiles per slab, tiles = S * ntile
    int64_t slab_len;    // Dt * N
    double theta;        // the held log-dispersion
    int Dx;              // coefficient rows
    int trow;            // the state row of a sampled theta, -1: held (or no dispersion)
    int ranges;
};

// log Gamma for x > 0 as kernels_glm.hip's glm_lgamma states it
__device__ __forceinline__ double pw_lgamma(double x) {
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
struct PwDraw { double theta, a, c; };

template <int FAM>
__device__ __forceinline__ PwDraw pw_draw(double theta) {
    PwDraw k{theta, 0.0, 0.0};
    if constexpr (FAM == PBBI_GLM_GAUSSIAN) {
        k.a = exp(-2.0 * theta);
    } else if constexpr (FAM == PBBI_GLM_NEGBINOMIAL) {
        k.a = exp(theta);
        k.c = pw_lgamma(k.a);
    }
    return k;
}

// ll = -(the energy term of k_glm) and the fitted mean of one observation at one draw; `on` = the row has weight
template <int FAM>
__device__ __forceinline__ void pw_link(double eta, double cv, double dv, const PwDraw& k, double& ll, double& mu, bool& on) {
    if constexpr (FAM == PBBI_GLM_LOGISTIC) {  // glm_link_rich: c ((eta > 0 ? eta : 0) + log1p(e)) - d eta
        const double e = exp(-fabs(eta));
        const double inv = 1.0 / (1.0 + e);
        mu = eta >= 0.0 ? inv : e * inv;
        ll = -(cv * ((eta > 0.0 ? eta : 0.0) + log1p(e)) - dv * eta);
        on = !(cv == 0.0 && dv == 0.0);
    } else if constexpr (FAM == PBBI_GLM_POISSON) {  // c e - d eta
        const double e = exp(eta);
        mu = e;
        ll = -(cv * e - dv * eta);
        on = !(cv == 0.0 && dv == 0.0);
    } else if constexpr (FAM == PBBI_GLM_GAUSSIAN) {  // glm_link_disp: c (0.5 tau r^2 + theta), d = y
        const double r = dv - eta;
        const double tr = k.a * r;
        const double trr = tr * r;
        mu = eta;
        ll = -(cv * (0.5 * trr + k.theta));
        on = cv != 0.0;
    } else {  // c (lgamma(phi) - lgamma(y + phi) + (y + phi) softplus(z) - y z), z = eta - theta
        const double z = eta - k.theta;
        const double e = exp(-fabs(z));
        const double ope = 1.0 + e;
        const double sp = (z > 0.0 ? z : 0.0) + log(ope);
        const double yp = dv + k.a;
        mu = exp(eta);
        ll = -(cv * (((k.c - pw_lgamma(yp)) + yp * sp) - dv * z));
        on = cv != 0.0;
    }
}

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
    constexpr bool DISP = FAM == PBBI_GLM_GAUSSIAN || FAM == PBBI_GLM_NEGBINOMIAL;
    __shared__ __attribute__((aligned(16))) pw_v2 lds[PW_OB * P1V];
    __shared__ double olds[3 * PW_OBS];
    __shared__ double red[4 * PW_OBS * PW_NV];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4;
    const int c = lane & 15;
    const int64_t blk0 = (int64_t)blockIdx.x * PW_OB;  // the image is padded to a multiple of 4 blocks: blk0 + 1 is inside it

    // ---- stage the group's fragments and values once
#pragma unroll
    for (int bi = 0; bi < PW_OB; ++bi) {
        const pw_v2* __restrict__ src = reinterpret_cast<const pw_v2*>(prm.img + (blk0 + bi) * prm.blk_len);
        for (int i = threadIdx.x; i < P1V; i += PW_BLOCK) lds[bi * P1V + i] = src[i];
    }
    if (threadIdx.x < 3 * PW_OBS) {
        const int st = threadIdx.x / PW_OBS, i = threadIdx.x % PW_OBS;
        const int64_t at = blk0 * 16 + i;
        double v;
        if (prm.c) v = (st == 0 ? prm.c : st == 1 ? prm.d : prm.o)[at];
        else v = st == 0 ? 1.0 : st == 1 ? prm.d[at] : 0.0;
        olds[threadIdx.x] = v;
    }
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
    const int Dx = prm.Dx;
    for (int64_t t = t0 + wave; t < t1; t += 4) {
        const int64_t slab = t / prm.ntile, n0 = (t - slab * prm.ntile) * 16;
        const int64_t left = prm.N - n0;
        const bool valid = c < left;
        const int64_t chain = n0 + (valid ? c : left - 1);  // ragged tail: compute on a clamped chain
        const double* __restrict__ col = prm.sdn + slab * prm.slab_len + chain;
        double q[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int row = 4 * s + g;
            const double v = col[(int64_t)(row < Dx ? row : Dx - 1) * prm.N];
            q[s] = row < Dx ? v : 0.0;
        }
        [[maybe_unused]] PwDraw dk{0.0, 0.0, 0.0};
        if constexpr (DISP) dk = pw_draw<FAM>(prm.trow >= 0 ? col[(int64_t)prm.trow * prm.N] : prm.theta);
        const double ninv = 1.0 / (n + 1.0);
#pragma unroll
        for (int bi = 0; bi < PW_OB; ++bi) {
            const pw_v2* __restrict__ P1 = lds + bi * P1V + lane;
            pw_v4 eta = pw_v4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s2 = 0; s2 < KS / 2; ++s2) {
                const pw_v2 A = P1[s2 * 64];
                eta = __builtin_amdgcn_mfma_f64_16x16x4f64(A.x, q[2 * s2], eta, 0, 0, 0);
                eta = __builtin_amdgcn_mfma_f64_16x16x4f64(A.y, q[2 * s2 + 1], eta, 0, 0, 0);
            }
            if (valid) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    double ll, mu;
                    bool on;
                    pw_link<FAM>(eta[r] + ov[bi][r], cv[bi][r], dv[bi][r], dk, ll, mu, on);
                    ll = on ? ll : 0.0;  // weight 0: exactly nothing, whatever b() gave
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

extern "C" int pbbi_pointwise_glm(const pbbi_potential* pot, const void* sdn, int S, int Dt, int64_t N, int ranges,
                                  double* lse_out, double* mean_out, double* var_out, double* mu_out, void* stream) {
    // every rule, before the device is touched (glm_host.cpp)
    if (int rc = glm_check_pointwise(pot ? (pot->kind == KIND_GLM ? 1 : 2) : 0, pot ? pot->glm_family : 0, pot ? pot->D : 0,
                                     sdn, S, Dt, N, ranges, var_out != nullptr))
        return rc;
    if (pot->dtype != PBBI_F64 || pot->glm_DP == 0 || !pot->d_glm_img)
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, "pbbi_pointwise_glm: a built fp64 GLM handle");
    DeviceGuard guard(pot->device);
    if (!guard.ok) return pbbi_fail(PBBI_ERR_HIP, "pbbi_pointwise_glm: cannot select the handle's device");
    hipStream_t st = (hipStream_t)stream;
    const int NT = pot->glm_DP / 16, fam = pot->glm_family;
    const int64_t M = pot->glm_M, nb = (M + 15) / 16, groups = (nb + PW_OB - 1) / PW_OB;
    const int64_t olen = glm_blocks_padded(M) * 16;

    PwPrm prm{};
    prm.img = (const double*)pot->d_glm_img;
    if (pot->glm_variant == GLM_V_PLAIN) {
        prm.c = nullptr; prm.d = (const double*)pot->d_glm_y; prm.o = nullptr;
    } else {
        prm.c = (const double*)pot->d_glm_obs; prm.d = prm.c + olen; prm.o = prm.d + olen;
    }
    prm.sdn = (const double*)sdn;
    prm.M = M; prm.N = N;
    prm.blk_len = (int64_t)pot->glm_DP * 32;
    prm.ntile = (N + 15) / 16;
    prm.tiles = (int64_t)S * prm.ntile;
    prm.slab_len = (int64_t)Dt * N;
    prm.theta = pot->glm_theta;
    prm.trow = pot->glm_trow;
    prm.Dx = pot->D - pot->glm_hier_J - (pot->glm_trow >= 0 ? 1 : 0);
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
    bool done = false;
#define PW_CASE(NT_, FAM_)                                                              \
    if (NT == NT_ && fam == FAM_) {                                                     \
        hipLaunchKernelGGL((k_glm_pw<NT_, FAM_>), grid, block, 0, st, prm);             \
        done = true;                                                                    \
    }
    PW_CASE(1, PBBI_GLM_LOGISTIC) PW_CASE(2, PBBI_GLM_LOGISTIC) PW_CASE(4, PBBI_GLM_LOGISTIC) PW_CASE(8, PBBI_GLM_LOGISTIC)
    PW_CASE(1, PBBI_GLM_POISSON) PW_CASE(2, PBBI_GLM_POISSON) PW_CASE(4, PBBI_GLM_POISSON) PW_CASE(8, PBBI_GLM_POISSON)
    PW_CASE(1, PBBI_GLM_GAUSSIAN) PW_CASE(2, PBBI_GLM_GAUSSIAN) PW_CASE(4, PBBI_GLM_GAUSSIAN) PW_CASE(8, PBBI_GLM_GAUSSIAN)
    PW_CASE(1, PBBI_GLM_NEGBINOMIAL) PW_CASE(2, PBBI_GLM_NEGBINOMIAL) PW_CASE(4, PBBI_GLM_NEGBINOMIAL)
#undef PW_CASE
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
