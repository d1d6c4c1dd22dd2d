// kernels_glm_predictive.hip -- posterior predictive replicates of a GLM handle, drawn in the kernel (gfx950): for each of
// S * N draws of the handle's state and each observation one replicate y_rep ~ p(y | draw), reduced per draw to seven test
// statistics over the observations (pbbi_predictive_glm, include/pbbi.h has the table), with the replicates of the first
// `keep` draws written out on request.  No M x T matrix exists unless it is asked for.
//
// The frame is k_glm_ll's (kernels_glm_loglik.hip), unchanged: a wave owns ONE tile of 16 draws -- the B operand and the
// per-draw constants in registers -- and walks the observation blocks, LB at a time, whose P1 fragments the four waves of a
// workgroup share through LDS; blockIdx.y cuts the (padded) blocks into `ranges`; k_glm_pp_merge folds the partials
// [ranges][7][S * N] in index order, without atomics.  Everything that frame is made of is glm_draws_dev.h's.  What is staged
// beside P1 differs: instead of the handle's c | d streams the caller's `aux` image y | n | a (response, binomial trials,
// weight; zero padded like the streams, so glm_draw_stage stages it as it stages c | d | o), and the handle's offset o.
//
// Per (draw t, observation i): eta + o_i, one replicate by glm_pp_sample (glm_sample_dev.h: counters (seed, t, i) alone, so
// neither the tile order nor `ranges` nor `keep` reaches a replicate), its log density and the observed value's by the same
// function, and the lane's share of the seven statistics.  A row of weight 0 and the image's padding rows are SELECTED out of
// all seven (a NaN there reaches nothing); in yrep_out a row of weight 0 is NaN.  At the end the four g groups of a draw are
// folded by two __shfl_xor steps, sums added, min and max taken.  A NaN replicate is carried as a flag beside the sums (fmin
// and fmax drop a NaN) and makes statistics 0, 1, 2, 3 and 5 of its own draw NaN.
//
// Shipped: the 22 shapes of glm_draw_dispatch; none reserves scratch (profiles/glm_predictive_resources.txt).
#include <cmath>

#include "glm_sample_dev.h"

namespace {

constexpr int PP_BLOCK = GLM_DRAW_BLOCK;
constexpr int PP_STATS = 7;

template <int NT> struct PpStage { static constexpr int LB = NT <= 4 ? 4 : 2; };

struct PpPrm : GlmDrawPrm {  // c | d | o of the base: the aux runs y | n | a
    const double* off;   // the handle's offset stream, nullptr: 0
    double* part;        // [ranges][7][S * N]
    double* yrep;        // (keep, M) or nullptr
    int64_t nblk, total, keep;
    uint64_t seed;
    double centre, cut;
};

template <int NT, int FAM>
__global__ void __launch_bounds__(PP_BLOCK) k_glm_pp(PpPrm prm) {
    constexpr int KS = 4 * NT;
    constexpr int LB = PpStage<NT>::LB;
    constexpr int P1V = (KS / 2) * 64;
    __shared__ __attribute__((aligned(16))) glm_v2 lds[LB * P1V];
    __shared__ double olds[3 * LB * 16];
    __shared__ double offs[LB * 16];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4;
    const int c = lane & 15;

    const int64_t t_own = (int64_t)blockIdx.x * 4 + wave;
    const bool tile_ok = t_own < prm.tiles;
    const int64_t t = tile_ok ? t_own : prm.tiles - 1;
    const GlmDrawTile tile = glm_draw_tile(prm, t, c);
    const bool valid = tile_ok && tile.valid;
    double q[KS];
    glm_draw_load<KS>(prm, tile.col, g, q);
    const GlmDrawChain<FAM> dk = glm_draw_disp<FAM>(prm, tile.col);
    const GlmPpChain pk = glm_pp_chain<FAM>(dk);
    const int64_t draw = tile.slab * prm.N + tile.chain;  // the global draw index s * N + n
    const bool writes = valid && prm.yrep != nullptr && draw < prm.keep;
    double* __restrict__ yrow = prm.yrep + (writes ? draw : 0) * prm.M;
    const double nan = __builtin_nan(""), inf = __builtin_inf();

    const int64_t nstage = prm.nblk / LB;
    const int64_t s0 = nstage * (int64_t)blockIdx.y / prm.ranges, s1 = nstage * ((int64_t)blockIdx.y + 1) / prm.ranges;
    double sum1 = 0.0, sum2 = 0.0, mn = inf, mx = -inf, cnt = 0.0, lrep = 0.0, lobs = 0.0;
    bool bad = false;
    for (int64_t sg = s0; sg < s1; ++sg) {
        const int64_t blk0 = sg * LB;
        __syncthreads();
        glm_draw_stage<LB, P1V>(prm, blk0, lds, olds);
        if (threadIdx.x < LB * 16) offs[threadIdx.x] = prm.off ? prm.off[blk0 * 16 + threadIdx.x] : 0.0;
        __syncthreads();
#pragma unroll 1
        for (int bi = 0; bi < LB; ++bi) {
            const glm_v4 eta4 = glm_draw_eta<KS>(lds + bi * P1V + lane, q);
#pragma unroll 1
            for (int r = 0; r < 4; ++r) {
                const int i = bi * 16 + 4 * r + g;
                const int64_t row = blk0 * 16 + i;
                const double yv = olds[i], nv = olds[LB * 16 + i], av = olds[2 * LB * 16 + i];
                const double eta = (r == 0 ? eta4[0] : r == 1 ? eta4[1] : r == 2 ? eta4[2] : eta4[3]) + offs[i];
                const bool on = av != 0.0 && row < prm.M;
                const GlmPpKey key{prm.seed, (uint64_t)draw, (uint64_t)row};
                // a row that is off draws nothing: its lane waits for the wave's slowest either way
                const double yr = on ? glm_pp_sample<FAM>(key, eta, nv, av, dk, pk) : nan;
                if (writes && row < prm.M) yrow[row] = yr;
                const double lr = glm_pp_logpdf<FAM>(yr, eta, nv, av, dk);
                const double lo = glm_pp_logpdf<FAM>(yv, eta, nv, av, dk);
                const bool isn = yr != yr;
                const double dc = yr - prm.centre;
                bad = bad || (on && isn);
                sum1 += on ? dc : 0.0;
                sum2 += on ? dc * dc : 0.0;
                mn = (on && yr < mn) ? yr : mn;
                mx = (on && yr > mx) ? yr : mx;
                cnt += (on && yr <= prm.cut) ? 1.0 : 0.0;
                lrep += on ? lr : 0.0;
                lobs += on ? lo : 0.0;
            }
        }
    }
    // ---- the four g groups of the lane's draw, in a fixed order
#pragma unroll
    for (int sh = 16; sh <= 32; sh *= 2) {
        sum1 += __shfl_xor(sum1, sh, 64);
        sum2 += __shfl_xor(sum2, sh, 64);
        cnt += __shfl_xor(cnt, sh, 64);
        lrep += __shfl_xor(lrep, sh, 64);
        lobs += __shfl_xor(lobs, sh, 64);
        const double m2 = __shfl_xor(mn, sh, 64), x2 = __shfl_xor(mx, sh, 64);
        mn = m2 < mn ? m2 : mn;
        mx = x2 > mx ? x2 : mx;
        const int b2 = __shfl_xor((int)bad, sh, 64);  // every lane takes part: not behind the ||
        bad = bad || b2 != 0;
    }
    if (valid && g == 0) {
        double* __restrict__ p = prm.part + (int64_t)blockIdx.y * PP_STATS * prm.total + draw;
        p[0] = bad ? nan : sum1;
        p[prm.total] = bad ? nan : sum2;
        p[2 * prm.total] = bad ? nan : mn;
        p[3 * prm.total] = bad ? nan : mx;
        p[4 * prm.total] = cnt;
        p[5 * prm.total] = bad ? nan : lrep;
        p[6 * prm.total] = lobs;
    }
}

// the ranges of one statistic of one draw in index order: sums added, min and max taken, a NaN kept
__global__ void __launch_bounds__(256) k_glm_pp_merge(const double* __restrict__ part, int64_t total, int ranges,
                                                       double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= PP_STATS * total) return;
    const int k = (int)(i / total);
    double s = part[i];
    for (int r = 1; r < ranges; ++r) {
        const double v = part[(int64_t)r * PP_STATS * total + i];
        if (k == 2) s = (v < s || v != v) ? v : s;
        else if (k == 3) s = (v > s || v != v) ? v : s;
        else s += v;
    }
    out[i] = s;
}

}  // namespace

extern "C" int pbbi_predictive_glm_check(int handle, int family, int state_dim, const void* sdn, const void* aux,
                                         const void* stats_out, int S, int Dt, int64_t N, int ranges, int64_t keep,
                                         int yrep_given, double centre, double cut) {
    return glm_check_predictive(handle, family, state_dim, sdn, aux, stats_out, S, Dt, N, ranges, keep, yrep_given != 0, centre,
                                cut);
}

static int pp_run(const pbbi_potential* pot, const void* sdn, int S, int Dt, int64_t N, uint64_t seed, const double* aux,
                  double centre, double cut, int ranges, double* stats_out, int64_t keep, double* yrep_out, hipStream_t st) {
    const int NT = pot->glm_DP / 16;
    PpPrm prm{};
    glm_draw_fill(prm, pot, sdn, S, Dt, N, true);
    const int64_t olen = glm_blocks_padded(pot->glm_M) * 16;
    prm.off = prm.c ? prm.o : nullptr;  // the plain model has none
    prm.c = aux; prm.d = aux + olen; prm.o = aux + 2 * olen;
    prm.total = (int64_t)S * N;
    prm.nblk = glm_blocks_padded(pot->glm_M);
    prm.keep = keep;
    prm.yrep = yrep_out;
    prm.seed = seed;
    prm.centre = centre;
    prm.cut = cut;
    const int64_t groups = (prm.tiles + 3) / 4;
    if (groups > 0x7fffffff) return pbbi_fail(PBBI_ERR_UNSUPPORTED, "pbbi_predictive_glm: more than 2^31 workgroups of 64 draws");
    if (ranges == 0) {  // as pbbi_loglik_glm chooses
        const int64_t nstage = prm.nblk / (NT <= 4 ? 4 : 2);
        int64_t r = (1024 + groups - 1) / groups;
        if (r > nstage) r = nstage;
        ranges = (int)(r < 1 ? 1 : r > 64 ? 64 : r);
    }
    prm.ranges = ranges;

    double* part = nullptr;
    PBBI_HIP(hipMallocAsync((void**)&part, sizeof(double) * (size_t)ranges * PP_STATS * (size_t)prm.total, st));
    prm.part = part;
    const dim3 grid((unsigned)groups, (unsigned)ranges), block(PP_BLOCK);
    const bool done = glm_draw_dispatch(NT, pot->glm_family, [&](auto nt, auto fam) {
        hipLaunchKernelGGL((k_glm_pp<decltype(nt)::value, decltype(fam)::value>), grid, block, 0, st, prm);
    });
    if (done)
        hipLaunchKernelGGL(k_glm_pp_merge, dim3((unsigned)((PP_STATS * prm.total + 255) / 256)), dim3(256), 0, st,
                       (const double*)part, prm.total, ranges, stats_out);
    const hipError_t launched = hipGetLastError();
    PBBI_HIP(hipFreeAsync(part, st));
    if (!done) return pbbi_fail(PBBI_ERR_UNSUPPORTED, "pbbi_predictive_glm: no kernel is shipped for this handle's family and "
                                                      "padded state dimension");
    PBBI_HIP(launched);
    return PBBI_OK;
}

extern "C" int pbbi_predictive_glm(const pbbi_potential* pot, const void* sdn, int S, int Dt, int64_t N, uint64_t seed,
                                   const double* aux, double centre, double cut, int ranges, double* stats_out, int64_t keep,
                                   double* yrep_out, void* stream) {
    return glm_draw_entry(
        "pbbi_predictive_glm", pot,
        [&](int handle, int family, int state_dim) {
            if (int rc = glm_check_predictive(handle, family, state_dim, sdn, aux, stats_out, S, Dt, N, ranges, keep,
                                              yrep_out != nullptr, centre, cut))
                return rc;
            return glm_check_predictive_keep(keep, pot->glm_M);  // a GLM handle from here on
        },
        [&] {
            return pp_run(pot, sdn, S, Dt, N, seed, aux, centre, cut, ranges, stats_out, keep, yrep_out, (hipStream_t)stream);
        });
}
