// glm_draws_dev.h -- what the two kernels that take T draws of a GLM handle's state share (gfx950): k_glm_pw
// (kernels_glm_pointwise.hip: per observation, reduced over the draws) and k_glm_ll (kernels_glm_loglik.hip: per draw, summed
// over the observations).  Both form eta tiles of 16 observations x 16 draws from the first-product fragments P1 of the packed
// design image (glm_pack, glm_host.cpp; the second copy P2 is not read) and the draws as they lie in the samplers' output, and
// apply the family's energy term in the lane; they differ in which of the two they keep in registers and which they walk.
//
// Device side: the common kernel arguments, the tile of 16 draws, the B operand, the staging of observation blocks into LDS,
// the eta tile and the energy term -- glm_link_rich / glm_link_disp of glm_family_dev.h with want_u, the functions k_glm calls.
// The plain model is the full model's formula at c = 1, d = y, o = 0, which is the plain formula bit for bit (1 * x and x + 0
// are exact), so the model is a runtime choice of what is staged, not an instantiation.
// Host side: the filler of the common arguments, the preflight of an entry and the (NT, family) dispatch of the 22 shipped
// shapes -- NT = DP / 16 in {1, 2, 4, 8} for logistic, poisson, gaussian and gamma, {1, 2, 4} for negbinomial and ordinal: the shapes the
// handles themselves are shipped in (glm_max_dim).
#pragma once
#include <cmath>
#include <type_traits>

#include "glm_family_dev.h"

typedef double glm_v4 __attribute__((ext_vector_type(4)));
typedef double glm_v2 __attribute__((ext_vector_type(2)));

constexpr int GLM_DRAW_BLOCK = 256;  // 4 waves

struct GlmDrawPrm {
    const double* img;   // the packed design image; block b starts at b * blk_len, P1 first
    const double* c;     // per-observation streams, zero padded to the image's blocks; c == nullptr: the plain model, d = y
    const double* d;
    const double* o;
    const double* sdn;   // S slabs (Dt, N)
    int64_t M, N, blk_len, ntile, tiles;  // ntile = tiles per slab, tiles = S * ntile
    int64_t slab_len;    // Dt * N
    double theta;        // the held log-dispersion
    int Dx;              // coefficient rows
    int trow;            // the state row of a sampled theta, -1: held (or no dispersion)
    int ranges;
    int K;               // ordinal family: categories; the K - 1 cutpoint rows are rows Dx .. Dx + K - 2 of a draw (else 0)
};

// Tile t of 16 consecutive draws (chains n0 .. n0 + 15 of one (Dt, N) slab) as lane c = lane & 15 sees it.  Ragged tail of a
// slab: a lane past N computes on a clamped chain and is not `valid`.
struct GlmDrawTile {
    int64_t slab, chain;
    bool valid;
    const double* __restrict__ col;  // row 0 of the lane's draw; row r is col[r * N]
};
__device__ __forceinline__ GlmDrawTile glm_draw_tile(const GlmDrawPrm& prm, int64_t t, int c) {
    const int64_t slab = t / prm.ntile, n0 = (t - slab * prm.ntile) * 16;
    const int64_t left = prm.N - n0;
    const bool valid = c < left;
    const int64_t chain = n0 + (valid ? c : left - 1);
    return GlmDrawTile{slab, chain, valid, prm.sdn + slab * prm.slab_len + chain};
}

// The B operand of K-step s: row 4s + g of the lane's draw, loaded as it lies.  Only rows below the coefficient count Dx are
// loaded as coefficients; rows Dx .. DP-1 are an exact 0 (a SELECT on the row index, the address clamped to a valid row), so the
// log-scales of a hierarchical handle or a sampled theta -- which sit behind zero columns of the image -- never meet those zeros
// as 0 * inf.
template <int KS>
__device__ __forceinline__ void glm_draw_load(const GlmDrawPrm& prm, const double* __restrict__ col, int g, double (&q)[KS]) {
    const int Dx = prm.Dx;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int row = 4 * s + g;
        const double v = col[(int64_t)(row < Dx ? row : Dx - 1) * prm.N];
        q[s] = row < Dx ? v : 0.0;
    }
}

// What a dispersion family forms once per draw (glm_disp_chain with want_u): a sampled theta is read from its own row (trow), a
// held one comes from the handle.  The canonical families form nothing.
// The ordinal family forms its cutpoints (glm_ord_chain with want_u) from the K - 1 rows behind the coefficients, read as they lie.
template <int FAM>
using GlmDrawChain = std::conditional_t<FAM == PBBI_GLM_ORDINAL, GlmOrdChain, GlmDispChain>;
template <int FAM>
__device__ __forceinline__ GlmDrawChain<FAM> glm_draw_disp(const GlmDrawPrm& prm, const double* __restrict__ col) {
    if constexpr (FAM == PBBI_GLM_ORDINAL) {
        double z[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const bool in = j < prm.K - 1;  // the address clamped to a row of the draw
            const double v = col[(int64_t)(prm.Dx + (in ? j : 0)) * prm.N];
            z[j] = in ? v : 0.0;
        }
        return glm_ord_chain(z, prm.K, true);
    } else if constexpr (glm_disp(FAM)) {
        return glm_disp_chain<FAM>(prm.trow >= 0 ? col[(int64_t)prm.trow * prm.N] : prm.theta, true);
    } else {
        return GlmDispChain{0.0, 0.0, 0.0, 0.0};
    }
}

// Blocks blk0 .. blk0 + NB - 1 of 16 observations into LDS, by the whole workgroup: their P1 fragments (P1V 16-byte elements
// each) and their c | d | o values (olds: three runs of NB * 16); the plain model stages c = 1, d = y, o = 0.  The image and the
// streams are padded to a multiple of 4 blocks, so NB <= 4 blocks from a multiple of NB are inside them.  The caller places the
// barriers.
template <int NB, int P1V>
__device__ __forceinline__ void glm_draw_stage(const GlmDrawPrm& prm, int64_t blk0, glm_v2* lds, double* olds) {
    static_assert(3 * NB * 16 <= GLM_DRAW_BLOCK, "one thread per staged value of c | d | o");
#pragma unroll
    for (int bi = 0; bi < NB; ++bi) {
        const glm_v2* __restrict__ src = reinterpret_cast<const glm_v2*>(prm.img + (blk0 + bi) * prm.blk_len);
        for (int i = threadIdx.x; i < P1V; i += GLM_DRAW_BLOCK) lds[bi * P1V + i] = src[i];
    }
    if (threadIdx.x < 3 * NB * 16) {
        const int st = threadIdx.x / (NB * 16), i = threadIdx.x % (NB * 16);
        const int64_t at = blk0 * 16 + i;
        double v;
        if (prm.c) v = (st == 0 ? prm.c : st == 1 ? prm.d : prm.o)[at];
        else v = st == 0 ? 1.0 : st == 1 ? prm.d[at] : 0.0;
        olds[threadIdx.x] = v;
    }
}

// The eta tile of one staged block (P1 = its fragments + lane): register r = observations {4r + g} of the lane's own draw
template <int KS>
__device__ __forceinline__ glm_v4 glm_draw_eta(const glm_v2* __restrict__ P1, const double (&q)[KS]) {
    glm_v4 eta = glm_v4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s2 = 0; s2 < KS / 2; ++s2) {
        const glm_v2 A = P1[s2 * 64];
        eta = __builtin_amdgcn_mfma_f64_16x16x4f64(A.x, q[2 * s2], eta, 0, 0, 0);
        eta = __builtin_amdgcn_mfma_f64_16x16x4f64(A.y, q[2 * s2 + 1], eta, 0, 0, 0);
    }
    return eta;
}

// The energy term of k_glm of one observation at one draw -- minus its log-likelihood with the constants k_i dropped -- by the
// functions k_glm calls; the residual and dU_i/dtheta are not read and the compiler drops them
template <int FAM>
__device__ __forceinline__ double glm_draw_uterm(double eta, double cv, double dv, [[maybe_unused]] const GlmDrawChain<FAM>& dk) {
    [[maybe_unused]] double resid, tterm, tlo;
    double uterm;
    if constexpr (FAM == PBBI_GLM_ORDINAL) glm_link_ord(eta, cv, dv, dk, true, resid, uterm, tterm, tlo);
    else if constexpr (glm_disp(FAM)) glm_link_disp<FAM>(eta, cv, dv, dk, true, resid, uterm, tterm);
    else glm_link_rich<FAM>(eta, cv, dv, true, resid, uterm);
    return uterm;
}

// ---- the host side of the two entries ----------------------------------------------------------------------------------------
// handle: 0 = NULL, 1 = a GLM handle, 2 = a handle of another kind (glm_check_pointwise, glm_check_loglik, glm_check_power)
inline int glm_handle_kind(const pbbi_potential* pot) { return pot ? (pot->kind == KIND_GLM ? 1 : 2) : 0; }

// An entry that takes draws: its argument rules (`rules(handle, family, state_dim)`: glm_host.cpp, before the device is
// touched), the handle's own state, its device made current, then `body()`.  `entry` is the entry's name in the error texts.
template <class Rules, class Body>
int glm_draw_entry(const char* entry, const pbbi_potential* pot, Rules&& rules, Body&& body) {
    if (int rc = rules(glm_handle_kind(pot), pot ? pot->glm_family : 0, pot ? pot->D : 0)) return rc;
    if (pot->dtype != PBBI_F64 || pot->glm_DP == 0 || !pot->d_glm_img)
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, std::string(entry) + ": a built fp64 GLM handle");
    DeviceGuard guard(pot->device);
    if (!guard.ok) return pbbi_fail(PBBI_ERR_HIP, std::string(entry) + ": cannot select the handle's device");
    return body();
}

// The common arguments from the handle and the draws (S slabs of (Dt, N)); `ranges` is the entry's.  as_built: read the streams
// as the handle was built, whatever likelihood power it carries now (d_glm_obs0, kept from the first tempering on).  That is
// pbbi_loglik_glm's reading -- the likelihood at power 1 is what a tempered sampler weighs by -- while pbbi_pointwise_glm reads
// d_glm_obs, the streams the handle samples with: deliberate, and the behaviour both entries have always had.
inline void glm_draw_fill(GlmDrawPrm& prm, const pbbi_potential* pot, const void* sdn, int S, int Dt, int64_t N, bool as_built) {
    const int64_t olen = glm_blocks_padded(pot->glm_M) * 16;
    prm.img = (const double*)pot->d_glm_img;
    if (pot->glm_variant == GLM_V_PLAIN) {
        prm.c = nullptr; prm.d = (const double*)pot->d_glm_y; prm.o = nullptr;
    } else {
        prm.c = (const double*)(as_built && pot->d_glm_obs0 ? pot->d_glm_obs0 : pot->d_glm_obs);
        prm.d = prm.c + olen; prm.o = prm.d + olen;
    }
    prm.sdn = (const double*)sdn;
    prm.M = pot->glm_M; prm.N = N;
    prm.blk_len = (int64_t)pot->glm_DP * 32;
    prm.ntile = (N + 15) / 16;
    prm.tiles = (int64_t)S * prm.ntile;
    prm.slab_len = (int64_t)Dt * N;
    prm.theta = pot->glm_theta;
    prm.trow = pot->glm_trow;
    prm.K = pot->glm_variant == GLM_V_ORDINAL ? pot->glm_K : 0;
    prm.Dx = pot->D - pot->glm_hier_J - (pot->glm_trow >= 0 ? 1 : 0) - (prm.K ? prm.K - 1 : 0);
}

// the fitted mean of one observation at one draw: glm_mean of glm_family_dev.h; the ordinal family's is the expected category
template <int FAM>
__device__ __forceinline__ double glm_draw_mean(double eta, [[maybe_unused]] const GlmDrawChain<FAM>& dk) {
    if constexpr (FAM == PBBI_GLM_ORDINAL) return glm_mean_ord(eta, dk);
    else return glm_mean<FAM>(eta);
}

// The (NT, family) switch of the shipped shapes: launch(NT, FAM) with both as std::integral_constant, so the entry names its
// kernel template as k<decltype(nt)::value, decltype(fam)::value>.  false: no kernel is shipped for the pair.
template <class Launch>
bool glm_draw_dispatch(int NT, int fam, Launch&& launch) {
    auto tiles = [&](auto f) {
        constexpr int FAM = decltype(f)::value;
        switch (NT) {
            case 1: launch(std::integral_constant<int, 1>{}, f); return true;
            case 2: launch(std::integral_constant<int, 2>{}, f); return true;
            case 4: launch(std::integral_constant<int, 4>{}, f); return true;
            case 8:
                if constexpr (FAM != PBBI_GLM_NEGBINOMIAL && (FAM != PBBI_GLM_ORDINAL || GLM_ORDINAL_MAX_ROWS >= 128)) {
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
        case PBBI_GLM_ORDINAL: return tiles(std::integral_constant<int, PBBI_GLM_ORDINAL>{});
    }
    return false;
}
