// kernels_glm_softmax.hip -- K-class (multinomial logistic / softmax) regression on the fp64 matrix cores (gfx950).
//
//   U(W) = sum_i [ logsumexp_k(eta_ik) - eta_{i,y_i} ] + 0.5 sum_k sum_d lam_d W_kd^2,   eta_ik = x_i . W_k,
//   dU/dW_k = sum_i (softmax_k(eta_i) - [y_i == k]) x_i + lam (.) W_k,                    y_i in {0 .. K-1}
// The sampler sees one vector of K D numbers per chain, class-major (w[k D + d]).  The chain frame is that of
// kernels_glm.hip (k_glm): 16 chains per wave, 4 waves per workgroup, ghost waves and a clamped ragged tail, q, the
// half-step velocity and the gradient accumulator in registers (element s of a lane is INTERNAL row 4s + g), X staged
// through LDS in the image glm_pack makes of an M x D matrix at DP = Dc, kick-drift-kick with one call site of the
// gradient, five modes, the accept test of pbbi_chain.h.  What is new:
//
// Internal layout.  Every class is padded to Dc = 16, 32 or 64 rows and owns the NTc = Dc / 16 tiles k NTc ..
// k NTc + NTc - 1 of the chain's state; NT = K NTc <= 8.  Internal row k Dc + d is external row k D + d for d < D.
// The K linear predictors of an observation are K eta tiles X_b . W_k: the SAME A fragments of X (each read from
// LDS once, s2 outer, k inner) against class k's rows, and under the MFMA's C/D map they land in the SAME lane.  The
// softmax over the classes is therefore in-lane arithmetic on K accumulator values, and each class's residual is
// already the B operand of X_b^T . R_k, which goes into class k's gradient tiles.  The K eta chains are independent
// of each other and interleave in the matrix pipe.
//
// Padding.  Rows d >= D of a class load 0 and are never stored.  A bounded descriptor alone cannot do that: the
// natural address of a padded row of class k is a real row of class k + 1.  The accessors below therefore decide per
// lane: a lane whose row is padding READS a row that certainly exists (the first row of its group of four, or row 0
// when the whole group is padding) and discards the value, and its store is not issued at all.  The descriptor is
// bounded over the K D external rows on top of that.
//
// Draws.  The in-kernel momentum must be the draw of a (K D, N) state: the normal of external row r is slot
// (r % 16) / 4 of block rng_block_of_dim(r).  The four elements of a tile are the rows r0 + 4e, r0 = k D + 16 tc + g:
// they lie in the block of r0 and, when k D is no multiple of 16, in the next block of the same r % 4 -- two Philox
// blocks per tile there instead of one, the same numbers.
//
// An observation >= M is masked out of the residual and of the energy (softmax(0) = 1 / K, log K).
#include <cmath>
#include <type_traits>

#include "glm_args.h"
#include "kernels_dense_dev.h"
#include "pbbi_chain.h"

int glm_softmax_launch_metric(const pbbi_potential* pot, const void* smx_prm, hipStream_t stream);  // smx_prm: a SmxPrm of this file

namespace {

struct SmxPrm {
    const double* img;    // nbp blocks of 32 Dc doubles (P1 then P2), nbp = blocks padded to a multiple of 4
    const double* y;      // labels as doubles, nbp * 16, zero padded
    const double* prior;  // lam, Dc values, zero padded past D
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
    double h, kT;
    int L, D, flags, rng, mode, method, nb;  // D: coefficients per class
    uint64_t seed, iter, chain0;
};
// the diagonal metric's kernel arguments (METRIC = true of k_glm_softmax): the same arguments plus the table
struct SmxPrmMetric : SmxPrm {
    const double* metric;  // {m, 1 / m} of each INTERNAL row (class k padded to Dc rows; {1, 1} on padding), K Dc entries or more
};
enum { SMX_HMC = 0, SMX_INTEGRATE = 1, SMX_EVAL = 2, SMX_ENERGY = 3, SMX_RATIO = 4 };

template <int NTc>
struct SmxCfg {
    static constexpr int KSc = 4 * NTc;                  // K-steps (elements of a lane) per class
    static constexpr int CB = NTc >= 4 ? 1 : 4 / NTc;    // observation blocks per staged chunk
    static constexpr int BLKV = NTc * 256;               // 16-byte elements per block (P1 + P2)
    static constexpr int CHV = CB * BLKV;                // ... per chunk
    static constexpr int PER_THREAD = CHV / BLOCK;       // = CB * NTc
    static_assert(CHV % BLOCK == 0, "whole 16-byte elements per thread");
};

// Element s of a lane: class s / KSc, row d = 4 (s % KSc) + g of that class, external row k D + d.
// voff = this lane's offset (8 (g ld + cc)), v0 = the offset of row 0 of its group (8 cc), ld8 = 8 ld.
template <int NTc>
__device__ __forceinline__ double smx_load(__amdgpu_buffer_rsrc_t base, uint32_t voff, uint32_t v0, uint32_t ld8, int s,
                                           int g, int D) {
    constexpr int KSc = 4 * NTc;
    const int k = s / KSc, d0 = 4 * (s % KSc);
    D = sgpr_fresh(D);  // (the row offset is formed next to its access, not held in a scalar register from the top)
    const bool ok = d0 + g < D;  // d0 >= D: no lane is
    const uint32_t soff = d0 < D ? (uint32_t)(k * D + d0) * sgpr_fresh(ld8) : 0u;
    const double t = buf_load<double>(base, ok ? voff : v0, soff);
    return ok ? t : 0.0;
}
template <int NTc>
__device__ __forceinline__ void smx_store(__amdgpu_buffer_rsrc_t base, uint32_t voff, uint32_t ld8, int s, int g, int D,
                                          double val) {
    constexpr int KSc = 4 * NTc;
    const int k = s / KSc, d0 = 4 * (s % KSc);
    D = sgpr_fresh(D);
    if (d0 + g < D) buf_store(base, voff, (uint32_t)(k * D + d0) * sgpr_fresh(ld8), val);
}

// gacc[k NTc + t][r] (class k, row 16t + 4r + g) = sum_i X[i][row] (softmax_k(eta_i) - [y_i == k]) for the wave's 16
// chains, usum = this lane's share of sum_i logsumexp(eta_i) - eta_{i, y_i}.  Staging as in kernels_glm.hip: one chunk of
// CB blocks is in LDS while the next waits in registers.
template <int NTc, int K>
__device__ __forceinline__ void smx_grad(const SmxPrm& prm, v2f64* __restrict__ lds, double* __restrict__ ylds, int lane,
                                         int g, const double (&q)[4 * NTc * K], v4f64 (&gacc)[NTc * K], double& usum,
                                         bool want_u) {
    using C = SmxCfg<NTc>;
    constexpr int KSc = C::KSc;
    const v2f64* __restrict__ src = reinterpret_cast<const v2f64*>(prm.img);
    const int nch = (prm.nb + C::CB - 1) / C::CB;
    v2f64 tmp[C::PER_THREAD];
    double ytmp = 0.0;
#pragma unroll
    for (int j = 0; j < C::PER_THREAD; ++j) tmp[j] = src[threadIdx.x + j * BLOCK];
    if (threadIdx.x < C::CB * 16) ytmp = prm.y[threadIdx.x];
#pragma unroll
    for (int t = 0; t < NTc * K; ++t) gacc[t] = v4f64{0.0, 0.0, 0.0, 0.0};
    usum = 0.0;
    for (int ch = 0; ch < nch; ++ch) {
        __syncthreads();  // everybody has finished reading the previous chunk
#pragma unroll
        for (int j = 0; j < C::PER_THREAD; ++j) lds[threadIdx.x + j * BLOCK] = tmp[j];
        if (threadIdx.x < C::CB * 16) ylds[threadIdx.x] = ytmp;
        __syncthreads();
        if (ch + 1 < nch) {
            const v2f64* nsrc = src + (size_t)(ch + 1) * C::CHV;
#pragma unroll
            for (int j = 0; j < C::PER_THREAD; ++j) tmp[j] = nsrc[threadIdx.x + j * BLOCK];
            if (threadIdx.x < C::CB * 16) ytmp = prm.y[(size_t)(ch + 1) * (C::CB * 16) + threadIdx.x];
        }
#pragma unroll
        for (int bi = 0; bi < C::CB; ++bi) {
            const int blk = ch * C::CB + bi;
            if (C::CB > 1 && blk >= prm.nb) break;
            const v2f64* __restrict__ P1 = lds + bi * C::BLKV + lane;
            const v2f64* __restrict__ P2 = P1 + (KSc / 2) * 64;
            // K eta tiles, each 16 observations x 16 chains: every fragment of X read once, used by all classes
            v4f64 eta[K];
#pragma unroll
            for (int k = 0; k < K; ++k) eta[k] = v4f64{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s2 = 0; s2 < KSc / 2; ++s2) {
                const v2f64 A = P1[s2 * 64];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    eta[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(A.x, q[k * KSc + 2 * s2], eta[k], 0, 0, 0);
                    eta[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(A.y, q[k * KSc + 2 * s2 + 1], eta[k], 0, 0, 0);
                }
            }
            // softmax in place: register r of every class = observations {4r + g} of this lane's chain
            const int64_t obs0 = (int64_t)blk * 16 + g;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool ok = obs0 + 4 * r < prm.M;
                const double yv = ylds[bi * 16 + 4 * r + g];
                double m = eta[0][r];
#pragma unroll
                for (int k = 1; k < K; ++k) m = eta[k][r] > m ? eta[k][r] : m;
                double eta_y = 0.0, Z = 0.0;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    eta_y = yv == (double)k ? eta[k][r] : eta_y;
                    const double e = exp(eta[k][r] - m);
                    eta[k][r] = e;
                    Z += e;
                }
                const double inv = 1.0 / Z;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const double rr = eta[k][r] * inv - (yv == (double)k ? 1.0 : 0.0);
                    eta[k][r] = ok ? rr : 0.0;
                }
                if (want_u) usum += ok ? (m + log(Z)) - eta_y : 0.0;
            }
            // class k's g tiles += X_b^T . R_k: K-step r sums over the observations register r holds
#pragma unroll
            for (int r2 = 0; r2 < 2; ++r2)
#pragma unroll
                for (int t = 0; t < NTc; ++t) {
                    const v2f64 A = P2[(r2 * NTc + t) * 64];
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        gacc[k * NTc + t] = __builtin_amdgcn_mfma_f64_16x16x4f64(A.x, eta[k][2 * r2], gacc[k * NTc + t], 0, 0, 0);
                        gacc[k * NTc + t] = __builtin_amdgcn_mfma_f64_16x16x4f64(A.y, eta[k][2 * r2 + 1], gacc[k * NTc + t], 0, 0, 0);
                    }
                }
        }
    }
}

// TWIN: the frame below (ghost waves and ragged tail, momentum first, the kick / drift schedule of the evaluation loop,
// the five modes, the accept epilogue) restates k_glm of kernels_glm.hip, which must keep compiling to what it compiles
// to.  A fix to either frame belongs in both.
//
// The diagonal metric (METRIC = true) is k_glm's, statement for statement: the table {m, 1 / m} in LDS for the launch (mlds, one
// 16-byte entry per INTERNAL row, loaded once before the first barrier; entry 4s + g is register s of the lane), read where it is
// used, one more factor in the draw, the velocity, the kick, p = v m and both kinetic energies.  A table of ones multiplies by
// exactly 1.0.  METRIC = false: nothing of it is compiled.
template <int NTc, int K, bool METRIC = false>
__global__ void __launch_bounds__(BLOCK, NTc * K <= 2 ? 2 : 1) k_glm_softmax(std::conditional_t<METRIC, SmxPrmMetric, SmxPrm> prm) {
    using C = SmxCfg<NTc>;
    constexpr int NT = NTc * K;
    constexpr int KS = 4 * NT;
    constexpr int KSc = C::KSc;
    constexpr int Dc = 16 * NTc;
    static_assert(K >= 2 && K <= 8 && NT <= 8, "2 <= K <= 8 classes of Dc = 16, 32 or 64 rows, K * Dc <= 128");
    __shared__ __attribute__((aligned(16))) v2f64 lds[C::CHV];
    __shared__ double ylds[C::CB * 16];
    // lam of each row of a class, zero past D; METRIC: behind it the metric's table, one 16-byte entry per internal row (mlds below)
    __shared__ __attribute__((aligned(METRIC ? 16 : 8))) double plds[Dc + (METRIC ? 32 * NTc * K : 0)];
    for (int i = threadIdx.x; i < Dc; i += BLOCK) plds[i] = prm.prior[i];
    [[maybe_unused]] v2f64* const mlds = reinterpret_cast<v2f64*>(plds + Dc);  // (Dc doubles: a multiple of 16 bytes)
    if constexpr (METRIC) {
        const v2f64* __restrict__ msrc = reinterpret_cast<const v2f64*>(prm.metric);
        for (int i = threadIdx.x; i < 16 * NTc * K; i += BLOCK) mlds[i] = msrc[i];
    }
    __syncthreads();
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
    const uint32_t v0 = 8u * (uint32_t)cc;
    const uint32_t vin = (uint32_t)g * ld_in + v0, vout = (uint32_t)g * ld_out + v0;
    const __amdgpu_buffer_rsrc_t qin = rows_of<false>(prm.q_in, n0, K * D, prm.ldn_in, prm.N);
    const __amdgpu_buffer_rsrc_t pin = rows_of<false>(prm.p_in, n0, K * D, prm.ldn_in, prm.N);
    const __amdgpu_buffer_rsrc_t qout = rows_of<false>(prm.q_out, n0, K * D, prm.ldn_out, prm.N);
    const __amdgpu_buffer_rsrc_t pout = rows_of<false>(prm.p_out, n0, K * D, prm.ldn_out, prm.N);
    const bool have_pout = (prm.p_out != nullptr);
    const double m = prm.mass ? prm.mass[n0 + cc] : 1.0;
    const double minv = prm.mass ? 1.0 / m : 1.0;
    const bool traj = (mode == SMX_HMC || mode == SMX_INTEGRATE);
    const bool rng = (mode == SMX_HMC) && prm.rng;
    const uint64_t chain = prm.chain0 + (uint64_t)(n0 + cc);

    double q[KS], vh[KS];
    v4f64 gacc[NT];
    // ---- momentum first (vh holds p until the division by the mass below)
    double u = 0.0;
    if (rng) {
        const double pstd = sqrt(m * prm.kT);  // src/ensemble.py:88
        const bool f64 = (prm.flags & PBBI_DRAW_F64) != 0;
#pragma unroll
        for (int t = 0; t < NT; ++t) {  // element e of the tile: external row r0 + 4e
            const int k = t / NTc, tc = t % NTc;
            const int r0 = k * D + 16 * tc + g;
            const uint32_t blk = rng_block_of_dim(r0);
            const int j = (r0 >> 2) & 3;  // slot of element 0; elements past slot 3 are in the next block of r0 % 4
            double z[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            {
                double za[4];
                rng_normal4d(prm.seed, PBBI_STREAM_MOMENTUM, prm.iter, chain, blk, f64, za);
#pragma unroll
                for (int i = 0; i < 4; ++i) z[i] = za[i];
            }
            // wave-uniform: no lane needs the next block when the class starts on a block boundary (j == 0 everywhere),
            // nor when the tile's last live element (emax, lane group 0's) stays within slot 3 for the largest j
            const int off = (k * D) & 15;
            const int jmax = off + 3 >= 12 ? 3 : (off + 3) >> 2;
            const int live = D - 16 * tc;  // live rows of this tile (<= 0: all padding)
            const int emax = live >= 16 ? 3 : (live + 3) / 4 - 1;
            if (off != 0 && live > 0 && jmax + emax >= 4) {
                double zb[4];
                rng_normal4d(prm.seed, PBBI_STREAM_MOMENTUM, prm.iter, chain, blk + 4u, f64, zb);
#pragma unroll
                for (int i = 0; i < 4; ++i) z[4 + i] = zb[i];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double ze = j == 0 ? z[e] : j == 1 ? z[e + 1] : j == 2 ? z[e + 2] : z[e + 3];
                if constexpr (METRIC) {
                    const double pstd_d = sqrt((m * mlds[4 * (4 * t + e) + g].x) * prm.kT);
                    vh[4 * t + e] = (16 * tc + 4 * e + g < D) ? ze * pstd_d : 0.0;
                } else {
                    vh[4 * t + e] = (16 * tc + 4 * e + g < D) ? ze * pstd : 0.0;
                }
            }
        }
        u = rng_uniform(prm.seed, prm.iter, chain);
        if (have_pout && !(prm.flags & PBBI_COMPAT_P_FROM_OLDQ) && valid) {
            // non-compat: a rejected chain reports its drawn momentum; park the draw now
#pragma unroll
            for (int s = 0; s < KS; ++s) smx_store<NTc>(pout, vout, ld_out, s, g, D, vh[s]);
        }
    } else if (mode != SMX_EVAL) {
#pragma unroll
        for (int s = 0; s < KS; ++s) vh[s] = smx_load<NTc>(pin, vin, v0, ld_in, s, g, D);
        if (mode == SMX_HMC) u = prm.u_in[n0 + cc];
    } else {
#pragma unroll
        for (int s = 0; s < KS; ++s) vh[s] = 0.0;
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) q[s] = smx_load<NTc>(qin, vin, v0, ld_in, s, g, D);
    double pp_old = 0.0;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        if constexpr (METRIC) pp_old = fma(vh[s] * mlds[4 * s + g].y, vh[s], pp_old);  // sum_d p_d^2 / m_d
        else pp_old = fma(vh[s], vh[s], pp_old);
    }
    // (the sum is FORMED here: left to the compiler it is sunk to the accept test, and the drawn momenta and the table's
    //  entries stay in registers across the whole trajectory -- 388 bytes of scratch at DP = 128)
    if constexpr (METRIC) pp_old = vgpr_fresh(pp_old);
    if (traj) {
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            if constexpr (METRIC) vh[s] *= minv * mlds[4 * s + g].y;  // v = p / (m_n m_d)
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
    if (traj) nev = sv ? L + 1 + (mode == SMX_HMC ? 1 : 0) : L + 1;
    const double h = prm.h;
    double U_old = 0.0, U_new = 0.0;
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
        const bool want_u = (e == 0 || e == nev - 1) && mode != SMX_INTEGRATE;
        double usum;
        smx_grad<NTc, K>(prm, lds, ylds, lane, g, q, gacc, usum, want_u);
        if (want_u) {
            double qq = 0.0;
#pragma unroll
            for (int s = 0; s < KS; ++s) qq = fma(plds[4 * (s % KSc) + g] * q[s], q[s], qq);
            U_new = chain_sum(usum) + 0.5 * chain_sum(qq);
            if (e == 0) U_old = U_new;
        }
        if (mode == SMX_EVAL) break;  // the gradient stays in gacc
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
                const double gt = fma(plds[4 * (s % KSc) + g], q[s], gacc[t][r]);
                if constexpr (METRIC) vh[s] = fma(-gt, ck * mlds[4 * s + gm].y, vh[s]);  // (ck != 0 here: no 0 * inf)
                else vh[s] = fma(-gt, ck, vh[s]);
                q[s] = fma(vh[s], hd, q[s]);
            }
    }

    if (mode == SMX_EVAL) {
        if (prm.grad_out && valid) {
            const __amdgpu_buffer_rsrc_t gout = rows_of<false>(prm.grad_out, n0, K * D, prm.ldn_out, prm.N);
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int s = 4 * t + r;
                    smx_store<NTc>(gout, vout, ld_out, s, g, D, fma(plds[4 * (s % KSc) + g], q[s], gacc[t][r]));
                }
        }
        if (prm.U_out && valid && g == 0) prm.U_out[n0 + c] = U_old;
        return;
    }
    if (mode == SMX_ENERGY || mode == SMX_RATIO) {
        const double H = 0.5 * chain_sum(pp_old) / m + U_old;
        if (valid && g == 0) {
            if (mode == SMX_ENERGY) {
                if (prm.U_out) prm.U_out[n0 + c] = H;
                if (prm.w_out) prm.w_out[n0 + c] = exp(-H);
            } else {
                prm.U_out[n0 + c] = exp(prm.U_out[n0 + c] - H);
            }
        }
        return;
    }
    if (mode == SMX_INTEGRATE) {  // in place q, p; optional Integrator.v
        if (valid) {
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                smx_store<NTc>(qout, vout, ld_out, s, g, D, q[s]);
                if constexpr (METRIC) smx_store<NTc>(pout, vout, ld_out, s, g, D, (prm.mass ? vh[s] * m : vh[s]) * mlds[4 * s + vgpr_fresh(g)].x);
                else smx_store<NTc>(pout, vout, ld_out, s, g, D, prm.mass ? vh[s] * m : vh[s]);
            }
            if (prm.v_out) {
                const __amdgpu_buffer_rsrc_t vo = rows_of<false>(prm.v_out, n0, K * D, prm.ldn_out, prm.N);
#pragma unroll
                for (int s = 0; s < KS; ++s) smx_store<NTc>(vo, vout, ld_out, s, g, D, vh[s]);
            }
        }
        return;
    }

    // ---- energies, ratio, decision (src/HMC.py:109-115,166-173)
    double pp_new = 0.0;
    [[maybe_unused]] int ge = g;
    if constexpr (METRIC) ge = vgpr_fresh(g);  // (read again, as at the kick)
#pragma unroll
    for (int s = 0; s < KS; ++s) {
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
    const double newH = 0.5 * chain_sum(pp_new) / m + U_new;
    const double ratio = exp((oldH - newH) * pbbi_accept_beta(prm.flags, prm.kT));
    const bool reject = metropolis_reject(ratio, u);
    const bool compat = (prm.flags & PBBI_COMPAT_P_FROM_OLDQ) != 0;
    bool store_p = have_pout;
    if (reject) {  // fetch the old point again instead of keeping it live through the trajectory
#pragma unroll
        for (int s = 0; s < KS; ++s) q[s] = smx_load<NTc>(qin, vin, v0, ld_in, s, g, D);  // :175
        if (compat) {  // :176  p <- oldQ
#pragma unroll
            for (int s = 0; s < KS; ++s) vh[s] = q[s];
        } else if (rng) {
            store_p = false;  // the parked draw stays
        } else if (have_pout) {
#pragma unroll
            for (int s = 0; s < KS; ++s) vh[s] = smx_load<NTc>(pin, vin, v0, ld_in, s, g, D);
        }
    }
    if (valid) {
#pragma unroll
        for (int s = 0; s < KS; ++s) smx_store<NTc>(qout, vout, ld_out, s, g, D, q[s]);  // :178
        if (store_p) {
#pragma unroll
            for (int s = 0; s < KS; ++s) smx_store<NTc>(pout, vout, ld_out, s, g, D, vh[s]);  // :179
        }
    }
    if (valid && g == 0) {
        if (prm.ratio_out) prm.ratio_out[n0 + c] = ratio;
        if (prm.reject_out) prm.reject_out[n0 + c] = reject ? 1 : 0;
    }
}

int smx_check(const pbbi_potential* pot, int64_t ld) {
    if (pot->dtype != PBBI_F64 || pot->glm_K < 2 || !pot->d_glm_img || !pot->d_glm_prior)
        return pbbi_fail(PBBI_ERR_UNSUPPORTED, GLM_SOFTMAX_RULE);
    if ((int64_t)(pot->D + 4) * ld >= ((int64_t)1 << 29))
        return pbbi_fail(PBBI_ERR_UNSUPPORTED,
                         "GLM kernels address a lane's rows with 32-bit offsets: rows * leading stride must "
                         "be < 2^29 elements; shard the ensemble");
    return PBBI_OK;
}

SmxPrm smx_prm(const pbbi_potential* pot) {
    SmxPrm prm{};
    prm.img = (const double*)pot->d_glm_img;
    prm.y = (const double*)pot->d_glm_y;
    prm.prior = (const double*)pot->d_glm_prior;
    prm.M = pot->glm_M;
    prm.nb = (int)((pot->glm_M + 15) / 16);
    prm.D = pot->D / pot->glm_K;
    prm.kT = 1.0;
    return prm;
}

template <bool METRIC>
int smx_launch_pass(const pbbi_potential* pot, const SmxPrm& prm0, hipStream_t stream) {
    std::conditional_t<METRIC, SmxPrmMetric, SmxPrm> prm{};
    static_cast<SmxPrm&>(prm) = prm0;
    if constexpr (METRIC) prm.metric = (const double*)pot->d_glm_metric;
    const dim3 grid((unsigned)((prm.N + CHAINS_PER_WG - 1) / CHAINS_PER_WG)), block(BLOCK);
    const int NTc = pot->glm_DP / 16, K = pot->glm_K;
    bool done = false;
#define SMX_CASE(NTC_, K_)                                                                 \
    if (NTc == NTC_ && K == K_) {                                                          \
        if constexpr (!METRIC || glm_softmax_metric_ships(16 * NTC_, K_)) {                \
            hipLaunchKernelGGL((k_glm_softmax<NTC_, K_, METRIC>), grid, block, 0, stream, prm); \
            done = true;                                                                   \
        }                                                                                  \
    }
    SMX_CASE(1, 2) SMX_CASE(1, 3) SMX_CASE(1, 4) SMX_CASE(1, 5) SMX_CASE(1, 6) SMX_CASE(1, 7) SMX_CASE(1, 8)
    SMX_CASE(2, 2) SMX_CASE(2, 3) SMX_CASE(2, 4)
    SMX_CASE(4, 2)
#undef SMX_CASE
    if (!done) return pbbi_fail(PBBI_ERR_UNSUPPORTED, GLM_SOFTMAX_RULE);
    PBBI_HIP(hipGetLastError());
    return PBBI_OK;
}
#ifndef PBBI_GLM_METRIC_TU
// the existing case list here, the METRIC list in a translation unit of its own (kernels_glm_softmax_metric.hip, as for k_glm:
// kernels_glm.hip says why); a handle without a metric launches the kernel it always has
int smx_launch(const pbbi_potential* pot, const SmxPrm& prm, hipStream_t stream) {
    if (!pot->d_glm_metric) return smx_launch_pass<false>(pot, prm, stream);
    return glm_softmax_launch_metric(pot, &prm, stream);
}

template <class Args>
int smx_run(const Args& a, int mode) {
    if (a.N == 0) return PBBI_OK;
    SmxPrm prm = smx_prm(a.pot);
    glm_fill(prm, a, mode);
    return smx_launch(a.pot, prm, a.stream);
}

#endif  // !PBBI_GLM_METRIC_TU

}  // namespace

#ifdef PBBI_GLM_METRIC_TU
int glm_softmax_launch_metric(const pbbi_potential* pot, const void* smx_prm, hipStream_t stream) {
    return smx_launch_pass<true>(pot, *static_cast<const SmxPrm*>(smx_prm), stream);
}
#else

int glm_softmax_hmc_iter(const IterArgs& a) {
    if (int rc = smx_check(a.pot, a.ldn_in > a.ldn_out ? a.ldn_in : a.ldn_out)) return rc;
    if (int rc = glm_check_iter(a)) return rc;
    return smx_run(a, SMX_HMC);
}
int glm_softmax_integrate(const IntegrateArgs& a) {
    if (int rc = smx_check(a.pot, a.ldn)) return rc;
    return smx_run(a, SMX_INTEGRATE);
}
int glm_softmax_eval(const EvalArgs& a) {
    if (int rc = smx_check(a.pot, a.ldn)) return rc;
    return smx_run(a, SMX_EVAL);
}
int glm_softmax_energy(const EvalArgs& a) {
    if (int rc = smx_check(a.pot, a.ldn)) return rc;
    return smx_run(a, a.ratio_finish ? SMX_RATIO : SMX_ENERGY);
}
#endif  // PBBI_GLM_METRIC_TU
