// kernels_glm_hessian.hip -- the Hessian of a GLM handle's potential at ONE state q (gfx950):
//   H = d2U/dq2 = X^T Lambda(eta) X + diag(lam)        [ + the theta row and column of a sampled log-dispersion ]
// U the potential pbbi_potential_eval differentiates, prior included; n x n row-major, n the handle's state dimension.  It is
// what a Newton step to the posterior mode, the Laplace approximation and a curvature metric need (laplace.py): M * D^2 fp64
// flops on the matrix cores over the design image the handle already keeps.
//
// Operands.  The eta tile of a block of 16 observations is P1 x w with w in all 16 columns of the B operand (glm_draw_eta of
// glm_draws_dev.h with a "draw" of stride 1): lane (g, c) = (lane >> 4, lane & 15) then holds eta of observation 4r + g in
// register r, the same value in every c.  That is the lane map of the P2 fragment of K-step r (glm_pack, glm_host.cpp: lane
// (g, c) holds X[16b + 4r + g][16t + c]), so tile (t, u) of X^T Lambda X is
//     mfma_f64_16x16x4( P2[r][t], h[4r + g] * P2[r][u] )    summed over r and the blocks,
// both operands from the second copy of the image: no cross-lane movement.  Only tiles t <= u are formed, and of a diagonal
// tile only the entries a <= b are read (x_a (h x_b) and x_b (h x_a) round differently): the merge mirrors them, so H is
// symmetric bit for bit.  H_w,theta = sum_i k_i x_i is one more product per tile row whose B operand is k in every column (the
// gradient's second product is the template); H_theta,theta is a sum in the lane.
//
// Waves.  A workgroup of four waves takes a stage of four blocks at a time.  First each wave forms eta and the second
// derivatives h | k of ONE of the four blocks (glm_hess_rich / glm_hess_disp of glm_family_dev.h) and leaves them in LDS (128
// doubles); after a barrier each wave accumulates ITS tile rows over all four blocks, reading the P2 fragments from the image
// (L1 / L2 serve the four waves' shared reads).  The tile rows are split so that no wave needs scratch: at NT = DP / 16 = 8,
// wave w owns rows w and 7 - w -- 9 of the 36 tiles, 36 accumulator doubles per lane, whichever w --, at NT <= 4 wave w owns
// row w (waves past NT form eta only).  The slot of a tile in the wave's accumulators is static; which (t, u) it holds is
// wave-uniform arithmetic on w, so the column fragment is loaded by address, not picked from a register array.
//
// Ranges.  blockIdx.x owns a range of stages and writes its partial image [DP * DP | DP | 1 (+ 7 pad)] to a workspace;
// k_glm_hess_merge folds the ranges in index order, without atomics, adds lam on the diagonal and mirrors: for a given `ranges`
// every bit is the same from run to run, and a range without a stage writes exact zeros.
//
// Rows.  A row of weight 0 (glm_row_on) and the image's padding rows (i >= M) have h = k = tt SELECTED to 0, so an exp(eta) that
// overflowed there reaches nothing.  The streams are read as they are: a handle tempered by pbbi_potential_set_likelihood_power
// gives the tempered Hessian.  The B operand of eta holds an exact 0 past the coefficient rows (glm_draw_load), so a sampled
// theta -- which sits behind a zero column of the image -- does not enter eta.
//
// Shipped: logistic, poisson, gaussian and gamma at NT = 1, 2, 4, 8, negbinomial at NT = 1, 2, 4 (the shapes the handles are
// shipped in); none reserves scratch (profiles/glm_hessian_resources.txt).
#include <cmath>

#include "glm_draws_dev.h"

namespace {

constexpr int HS_BLOCK = GLM_DRAW_BLOCK;  // 4 waves

struct HsPrm : GlmDrawPrm {
    double* part;  // [ranges][plen]
    int64_t nblk;  // blocks of the image (a multiple of 4)
    int64_t plen;  // DP * DP + DP + 8
};

template <int NT, int FAM>
__global__ void __launch_bounds__(HS_BLOCK) k_glm_hess(HsPrm prm) {
    constexpr int KS = 4 * NT, DP = 16 * NT;
    constexpr int NS = NT == 8 ? 9 : NT;  // tile slots of a wave
    constexpr int NR = NT == 8 ? 2 : 1;   // tile rows of a wave
    __shared__ double hl[2 * 64];         // h | k of the stage's 64 observations
    __shared__ double tl[4];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4;
    const int c = lane & 15;
    const bool sampled = prm.trow >= 0;

    // ---- the state: w in all 16 columns of eta's B operand, and what the family forms once
    double q[KS];
    glm_draw_load<KS>(prm, prm.sdn, g, q);
    [[maybe_unused]] GlmDispChain dk{0.0, 0.0, 0.0, 0.0};
    if constexpr (glm_disp(FAM)) dk = glm_hess_chain<FAM>(sampled ? prm.sdn[prm.trow] : prm.theta);

    // ---- the wave's tile rows: slots 0 .. n0 - 1 are tiles (t0, t0 + s), the rest (NT = 8) tiles (t1, t1 + s - n0)
    const int t0 = wave < NT ? wave : NT - 1;
    const int t1 = NT - 1 - t0;
    const int n0 = wave < NT ? NT - wave : 0;
    const int nslot = NT == 8 ? NS : n0;

    glm_v4 acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = glm_v4{0.0, 0.0, 0.0, 0.0};
    glm_v4 acck[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) acck[j] = glm_v4{0.0, 0.0, 0.0, 0.0};
    double tt_acc = 0.0;

    const int64_t nstage = prm.nblk / 4;
    const int64_t s0 = nstage * (int64_t)blockIdx.x / prm.ranges, s1 = nstage * ((int64_t)blockIdx.x + 1) / prm.ranges;
    for (int64_t sg = s0; sg < s1; ++sg) {
        {  // eta and the second derivatives of the wave's own block of the stage
            const int64_t blk = sg * 4 + wave;
            const glm_v4 eta = glm_draw_eta<KS>(reinterpret_cast<const glm_v2*>(prm.img + blk * prm.blk_len) + lane, q);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t i = blk * 16 + 4 * r + g;
                const double cv = prm.c ? prm.c[i] : 1.0, dv = prm.d[i], ov = prm.c ? prm.o[i] : 0.0;
                double h, kx = 0.0, tt = 0.0;
                if constexpr (glm_disp(FAM)) glm_hess_disp<FAM>(eta[r] + ov, cv, dv, dk, h, kx, tt);
                else h = glm_hess_rich<FAM>(eta[r] + ov, cv);
                const bool on = glm_row_on<FAM>(cv, dv) && i < prm.M;  // weight 0, padding rows: exactly nothing
                tt_acc += on ? tt : 0.0;
                if (c == 0) {
                    hl[wave * 16 + 4 * r + g] = on ? h : 0.0;
                    hl[64 + wave * 16 + 4 * r + g] = on ? kx : 0.0;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int bi = 0; bi < 4; ++bi) {
            const glm_v2* __restrict__ P2 = reinterpret_cast<const glm_v2*>(prm.img + (sg * 4 + bi) * prm.blk_len + KS * 64) + lane;
#pragma unroll
            for (int r2 = 0; r2 < 2; ++r2) {
                const double h0 = hl[bi * 16 + 8 * r2 + g], h1 = hl[bi * 16 + 8 * r2 + 4 + g];
                const glm_v2 A0 = P2[(r2 * NT + t0) * 64];
                glm_v2 A1 = A0;
                if constexpr (NR == 2) A1 = P2[(r2 * NT + t1) * 64];
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    if (s < nslot) {  // wave-uniform
                        const bool first = s < n0;
                        const int u = first ? t0 + s : t1 + (s - n0);
                        const glm_v2 B = P2[(r2 * NT + u) * 64];
                        const glm_v2 A = first ? A0 : A1;
                        acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(A.x, h0 * B.x, acc[s], 0, 0, 0);
                        acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(A.y, h1 * B.y, acc[s], 0, 0, 0);
                    }
                }
                if constexpr (glm_disp(FAM)) {
                    if (sampled && nslot > 0) {
                        const double k0 = hl[64 + bi * 16 + 8 * r2 + g], k1 = hl[64 + bi * 16 + 8 * r2 + 4 + g];
                        acck[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(A0.x, k0, acck[0], 0, 0, 0);
                        acck[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(A0.y, k1, acck[0], 0, 0, 0);
                        if constexpr (NR == 2) {
                            acck[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(A1.x, k0, acck[1], 0, 0, 0);
                            acck[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(A1.y, k1, acck[1], 0, 0, 0);
                        }
                    }
                }
            }
        }
        __syncthreads();  // hl has been read
    }

    // ---- the partial image of this range: register rr of lane (g, c) is entry (16 t + 4 rr + g, 16 u + c)
    double* __restrict__ out = prm.part + (int64_t)blockIdx.x * prm.plen;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (s < nslot) {
            const bool first = s < n0;
            const int t = first ? t0 : t1;
            const int u = first ? t0 + s : t1 + (s - n0);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) out[(16 * t + 4 * rr + g) * DP + 16 * u + c] = acc[s][rr];
        }
    }
    if constexpr (glm_disp(FAM)) {
        if (sampled && nslot > 0 && c == 0) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                out[DP * DP + 16 * t0 + 4 * rr + g] = acck[0][rr];
                if constexpr (NR == 2) out[DP * DP + 16 * t1 + 4 * rr + g] = acck[1][rr];
            }
        }
        // theta-theta: the four g groups of a wave, then the four waves, in a fixed order
        tt_acc += __shfl_xor(tt_acc, 16, 64);
        tt_acc += __shfl_xor(tt_acc, 32, 64);
        if (lane == 0) tl[wave] = tt_acc;
        __syncthreads();
        if (threadIdx.x == 0) out[DP * DP + DP] = ((tl[0] + tl[1]) + tl[2]) + tl[3];
    }
}

// H[a][b] of the n x n output: the ranges of its entry of the partial image in index order, lam on the diagonal.  (a, b) and
// (b, a) read the same entry -- the one with the smaller row -- so the output is symmetric bit for bit.
__global__ void __launch_bounds__(256) k_glm_hess_merge(const double* __restrict__ part, int64_t plen, int ranges, int DP, int n,
                                                         int trow, const double* __restrict__ lam_vec, double lam,
                                                         double* __restrict__ out) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * n) return;
    const int a = idx / n, b = idx - a * n;
    int at;
    if (a == trow || b == trow) at = a == b ? DP * DP + DP : DP * DP + (a == trow ? b : a);
    else at = a <= b ? a * DP + b : b * DP + a;
    double s = part[at];
    for (int r = 1; r < ranges; ++r) s += part[(int64_t)r * plen + at];
    if (a == b) s += lam_vec ? lam_vec[a] : lam;
    out[idx] = s;
}

// The (NT, family) switch of the shipped shapes: the families with a likelihood in closed second derivatives, NT = 8 not for
// the negative binomial (its handles stop at 64 rows).  false: no kernel is shipped for the pair.
template <class Launch>
bool hess_dispatch(int NT, int fam, Launch&& launch) {
    auto tiles = [&](auto f) {
        constexpr int FAM = decltype(f)::value;
        switch (NT) {
            case 1: launch(std::integral_constant<int, 1>{}, f); return true;
            case 2: launch(std::integral_constant<int, 2>{}, f); return true;
            case 4: launch(std::integral_constant<int, 4>{}, f); return true;
            case 8:
                if constexpr (FAM != PBBI_GLM_NEGBINOMIAL) {
                    launch(std::integral_constant<int, 8>{}, f);
                    return true;
                }
        }
        return false;
    };
    switch (fam) {
        case PBBI_GLM_LOGISTIC: return tiles(std::integral_constant<int, PBBI_GLM_LOGISTIC>{});
        case PBBI_GLM_POISSON: return tiles(std::integral_constant<int, PBBI_GLM_POISSON>{});
        case PBBI_GLM_GAUSSIAN: return tiles(std::integral_constant<int, PBBI_GLM_GAUSSIAN>{});
        case PBBI_GLM_NEGBINOMIAL: return tiles(std::integral_constant<int, PBBI_GLM_NEGBINOMIAL>{});
        case PBBI_GLM_GAMMA: return tiles(std::integral_constant<int, PBBI_GLM_GAMMA>{});
    }
    return false;
}

}  // namespace

extern "C" int pbbi_glm_hessian_check(int handle, int family, int hierarchical, const void* q, const void* hess_out, int ranges) {
    return glm_check_hessian(handle, family, hierarchical != 0, q, hess_out, ranges);
}

// the launches of pbbi_glm_hessian, after glm_draw_entry's preflight
static int hess_run(const pbbi_potential* pot, const void* q, int ranges, double* hess_out, hipStream_t st) {
    const int DP = pot->glm_DP, NT = DP / 16, n = pot->D;
    HsPrm prm{};
    glm_draw_fill(prm, pot, q, 1, n, 1, false);  // one "draw" of stride 1; the streams as the handle samples with them
    prm.nblk = glm_blocks_padded(pot->glm_M);
    prm.plen = (int64_t)DP * DP + DP + 8;
    if (ranges == 0) {  // two workgroups per compute unit of the largest part, at least one stage per range
        const int64_t nstage = prm.nblk / 4;
        ranges = (int)(nstage < 512 ? nstage : 512);
    }
    prm.ranges = ranges;

    double* part = nullptr;
    PBBI_HIP(hipMallocAsync((void**)&part, sizeof(double) * (size_t)ranges * (size_t)prm.plen, st));
    prm.part = part;
    const bool done = hess_dispatch(NT, pot->glm_family, [&](auto nt, auto fam) {
        hipLaunchKernelGGL((k_glm_hess<decltype(nt)::value, decltype(fam)::value>), dim3((unsigned)ranges), dim3(HS_BLOCK), 0, st,
                           prm);
    });
    if (done) {
        const bool plain = pot->glm_variant == GLM_V_PLAIN;
        hipLaunchKernelGGL(k_glm_hess_merge, dim3((unsigned)((n * n + 255) / 256)), dim3(256), 0, st, (const double*)part, prm.plen,
                           ranges, DP, n, prm.trow, plain ? (const double*)nullptr : (const double*)pot->d_glm_prior, pot->glm_lam,
                           hess_out);
    }
    const hipError_t launched = hipGetLastError();
    PBBI_HIP(hipFreeAsync(part, st));
    if (!done) return pbbi_fail(PBBI_ERR_UNSUPPORTED, "pbbi_glm_hessian: no kernel is shipped for this handle's family and "
                                                      "padded state dimension");
    PBBI_HIP(launched);
    return PBBI_OK;
}

extern "C" int pbbi_glm_hessian(const pbbi_potential* pot, const void* q, int ranges, double* hess_out, void* stream) {
    return glm_draw_entry(
        "pbbi_glm_hessian", pot,
        [&](int handle, int family, int) {
            return glm_check_hessian(handle, family, pot && pot->glm_hier_J > 0, q, hess_out, ranges);
        },
        [&] { return hess_run(pot, q, ranges, hess_out, (hipStream_t)stream); });
}
