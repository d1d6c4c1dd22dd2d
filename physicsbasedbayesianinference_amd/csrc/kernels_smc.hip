// kernels_smc.hip -- the cross-chain steps of tempered sequential Monte Carlo (include/pbbi.h, "tempered SMC";
// DESIGN.md 4.9): the ESS of candidate temperatures, the device-side choice of the next one, the reweighting with
// the log-evidence increment, and systematic resampling of the (D, N) state.
//
// Every sum is an fp64 log-sum-exp pair (max, sum) accumulated online, reduced in two deterministic stages (a
// fixed number of partials per N, merged in a fixed order; no atomics).  The resampler's cumulative weights are
// integers (fixed-point ticks, 64-bit prefix sums), so its ancestors do not depend on launch shape or on the
// order of any floating-point sum.
#include "pbbi_internal.h"
#include "pbbi_rng.h"

namespace {

constexpr int SMC_BLOCK = 256;
constexpr int SCAN_K = 64;          // candidates per scan block (64 lanes x 4 particle groups)
constexpr int NB_GRID = 64;         // candidates per next_beta pass
constexpr int NB_REFINE = 6;        // K-section passes after the log-spaced one: bracket / 65^6
constexpr double NB_LOG_LO = 1e-8;  // the log grid spans [1e-8, 1] * (1 - beta)
constexpr int RS_TILE = 1024;       // particles per block of the tick / prefix-scan kernels (256 x 4)
constexpr int TICK_BITS = 32;       // ticks_n = floor(exp(logw_n - max) * 2^32)

inline size_t esize(int dtype) { return dtype == PBBI_F64 ? 8 : 4; }

// ---- online log-sum-exp pairs -----------------------------------------------------------------------------
// A non-finite term (NaN, -inf, +inf) has zero weight.
__device__ __forceinline__ void lse_add(double& m, double& s, double a) {
    if (!(a > -INFINITY && a < INFINITY)) return;
    if (a > m) {
        s = s * exp(m - a) + 1.0;
        m = a;
    } else {
        s += exp(a - m);
    }
}
__device__ __forceinline__ void lse_merge(double& m, double& s, double m2, double s2) {
    if (!(s2 > 0.0)) return;
    if (!(s > 0.0)) { m = m2; s = s2; return; }
    if (m2 > m) {
        s = s * exp(m - m2) + s2;
        m = m2;
    } else {
        s += s2 * exp(m2 - m);
    }
}
__device__ __forceinline__ double lse_log(double m, double s) { return s > 0.0 ? m + log(s) : -INFINITY; }

int n_parts(int64_t N, int64_t per_block, int cap) {  // partial count: a function of N alone
    const int64_t b = (N + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// ---- stage-1 reference term r_n = |q_n - m|^2 / (2 sigma^2) + (D/2) log(2 pi sigma^2) ------------------------
template <typename T>
__global__ __launch_bounds__(SMC_BLOCK) void k_smc_ref(const T* __restrict__ q, int64_t N, int64_t ldn, int D,
                                                       const double* __restrict__ mean, double inv2s2, double cst,
                                                       double* __restrict__ r) {
    const int64_t n = (int64_t)blockIdx.x * SMC_BLOCK + threadIdx.x;
    if (n >= N) return;
    double acc = 0.0;
    for (int d = 0; d < D; ++d) {
        const double x = (double)q[(int64_t)d * ldn + n] - (mean ? mean[d] : 0.0);
        acc += x * x;
    }
    r[n] = acc * inv2s2 + cst;
}

// ---- ESS scan: per candidate c_k, l_n = r_n - c_k U_n, a_n = logw_n + l_n, b_n = logw_n + 2 l_n ------------------
// Slot K is the normaliser log sum exp(logw).  part[((slot * n_part) + block) * 4 + {m_a, s_a, m_b, s_b}].
template <typename T>
__global__ __launch_bounds__(SMC_BLOCK) void k_scan_partial(const T* __restrict__ U, const double* __restrict__ logw,
                                                            const double* __restrict__ ref, int64_t N, int K,
                                                            const double* __restrict__ coef, int n_part,
                                                            double* __restrict__ part) {
    __shared__ double sU[SMC_BLOCK], sR[SMC_BLOCK], sL[SMC_BLOCK];
    __shared__ double red[4][SCAN_K][4];
    const int tid = threadIdx.x, k = tid & (SCAN_K - 1), g = tid >> 6;
    const int slot = blockIdx.y * SCAN_K + k;
    const bool live = slot <= K;
    const double c = slot < K ? coef[slot] : 0.0;
    double ma = -INFINITY, sa = 0.0, mb = -INFINITY, sb = 0.0;
    for (int64_t base = (int64_t)blockIdx.x * SMC_BLOCK; base < N; base += (int64_t)n_part * SMC_BLOCK) {
        __syncthreads();
        const int64_t n = base + tid;
        if (n < N) {
            sU[tid] = (double)U[n];
            sR[tid] = ref ? ref[n] : 0.0;
            sL[tid] = logw ? logw[n] : 0.0;
        }
        __syncthreads();
        const int cnt = (int)((N - base) < SMC_BLOCK ? (N - base) : SMC_BLOCK);
        if (live) {
            for (int i = g; i < cnt; i += 4) {
                if (slot == K) { lse_add(ma, sa, sL[i]); continue; }
                const double l = sR[i] - c * sU[i];
                lse_add(ma, sa, sL[i] + l);
                lse_add(mb, sb, sL[i] + 2.0 * l);
            }
        }
    }
    red[g][k][0] = ma; red[g][k][1] = sa; red[g][k][2] = mb; red[g][k][3] = sb;
    __syncthreads();
    if (g == 0 && live) {
        for (int j = 1; j < 4; ++j) {  // fixed order
            lse_merge(ma, sa, red[j][k][0], red[j][k][1]);
            lse_merge(mb, sb, red[j][k][2], red[j][k][3]);
        }
        double* o = part + ((size_t)slot * n_part + blockIdx.x) * 4;
        o[0] = ma; o[1] = sa; o[2] = mb; o[3] = sb;
    }
}

// out[3k] = log sum W w, out[3k+1] = log sum W w^2, out[3k+2] = (sum W w)^2 / sum W w^2; out[3K] = log sum exp(logw)
__global__ void k_scan_final(const double* __restrict__ part, int n_part, int K, double* __restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > K) return;
    double m0 = -INFINITY, s0 = 0.0;
    const double* pn = part + (size_t)K * n_part * 4;
    for (int i = 0; i < n_part; ++i) lse_merge(m0, s0, pn[4 * i], pn[4 * i + 1]);
    const double lnorm = lse_log(m0, s0);
    if (k == K) { out[3 * K] = lnorm; return; }
    double ma = -INFINITY, sa = 0.0, mb = -INFINITY, sb = 0.0;
    const double* p = part + (size_t)k * n_part * 4;
    for (int i = 0; i < n_part; ++i) {
        lse_merge(ma, sa, p[4 * i], p[4 * i + 1]);
        lse_merge(mb, sb, p[4 * i + 2], p[4 * i + 3]);
    }
    const double la = lse_log(ma, sa) - lnorm, lb = lse_log(mb, sb) - lnorm;
    const double ess = exp(2.0 * la - lb);
    out[3 * k] = la;
    out[3 * k + 1] = lb;
    out[3 * k + 2] = ess == ess ? ess : 0.0;  // no weight at all: ESS 0
}

// ---- next beta: bracket search on the device ----------------------------------------------------------------
// st[0] lo, st[1] hi, st[2] done, st[3] warn, st[4] chosen (lo of the final bracket)
__global__ void k_nb_init(const double* __restrict__ betas, double* __restrict__ coef) {
    const int i = threadIdx.x;
    const double room = 1.0 - betas[0];
    // log-spaced: 1e-8 * room .. room
    coef[i] = room * exp(log(NB_LOG_LO) * (double)(NB_GRID - 1 - i) / (double)(NB_GRID - 1));
    if (i == NB_GRID - 1) coef[i] = room;
}

__global__ void k_nb_step(const double* __restrict__ res, double* __restrict__ coef, double* __restrict__ st,
                          const double* __restrict__ betas, int pass, int stage1, double target) {
    if (threadIdx.x != 0) return;
    const double room = 1.0 - betas[0];
    if (pass == 0) {
        st[2] = 0.0; st[3] = 0.0;
        // the log grid: start after the maximiser (stage 1, ESS not monotone) or at 0 (later stages)
        int a = 0;
        if (stage1)
            for (int i = 1; i < NB_GRID; ++i)
                if (res[3 * i + 2] > res[3 * a + 2]) a = i;
        if (res[3 * a + 2] < target) {
            if (stage1) { st[4] = coef[a]; st[3] = 1.0; st[2] = 1.0; st[0] = st[1] = coef[a]; }
            else { st[0] = 0.0; st[1] = coef[0]; }
        } else {
            int i = a;
            while (i + 1 < NB_GRID && res[3 * (i + 1) + 2] >= target) ++i;
            if (i == NB_GRID - 1) { st[4] = room; st[2] = 1.0; st[0] = st[1] = room; }  // the whole way to beta = 1
            else { st[0] = coef[i]; st[1] = coef[i + 1]; }
        }
    } else if (st[2] == 0.0) {
        // interior points lo + (hi - lo) (j + 1) / (K + 1): the first one below the target closes the bracket
        const double lo = st[0], hi = st[1];
        int j = 0;
        while (j < NB_GRID && res[3 * j + 2] >= target) ++j;
        st[0] = j == 0 ? lo : coef[j - 1];
        st[1] = j == NB_GRID ? hi : coef[j];
    }
    if (st[2] == 0.0) {
        const double lo = st[0], w = st[1] - st[0];
        for (int j = 0; j < NB_GRID; ++j) coef[j] = lo + w * (double)(j + 1) / (double)(NB_GRID + 1);
    }
}

__global__ void k_nb_finish(const double* __restrict__ st, double* __restrict__ betas, double* __restrict__ info) {
    if (threadIdx.x != 0) return;
    const double d = st[2] != 0.0 ? st[4] : st[0];
    const double b = betas[0] + d;
    betas[1] = (d >= 1.0 - betas[0] || b >= 1.0) ? 1.0 : b;
    if (info) { info[0] = st[3]; info[1] = st[1] - st[0]; }
}

// ---- reweight --------------------------------------------------------------------------------------------------
// part[block * 6 + {m_old, s_old, m_new, s_new, m_new2, s_new2}]
template <typename T>
__global__ __launch_bounds__(SMC_BLOCK) void k_rw_partial(const T* __restrict__ U, const double* __restrict__ ref,
                                                          int64_t N, const double* __restrict__ betas,
                                                          double* __restrict__ logw, double* __restrict__ part) {
    __shared__ double red[6][SMC_BLOCK];
    const double c = betas[1] - betas[0];
    double m0 = -INFINITY, s0 = 0.0, m1 = -INFINITY, s1 = 0.0, m2 = -INFINITY, s2 = 0.0;
    for (int64_t n = (int64_t)blockIdx.x * SMC_BLOCK + threadIdx.x; n < N; n += (int64_t)gridDim.x * SMC_BLOCK) {
        const double lw = logw[n];
        const double l = (ref ? ref[n] : 0.0) - c * (double)U[n];
        const double nw = lw + l;
        lse_add(m0, s0, lw);
        lse_add(m1, s1, nw);
        lse_add(m2, s2, 2.0 * nw);
        logw[n] = nw == nw ? nw : -INFINITY;
    }
    const int t = threadIdx.x;
    red[0][t] = m0; red[1][t] = s0; red[2][t] = m1; red[3][t] = s1; red[4][t] = m2; red[5][t] = s2;
    __syncthreads();
    for (int s = SMC_BLOCK / 2; s > 0; s >>= 1) {
        if (t < s)
            for (int j = 0; j < 6; j += 2) {
                double m = red[j][t], v = red[j + 1][t];
                lse_merge(m, v, red[j][t + s], red[j + 1][t + s]);
                red[j][t] = m; red[j + 1][t] = v;
            }
        __syncthreads();
    }
    if (t < 6) part[(size_t)blockIdx.x * 6 + t] = red[t][0];
}

// stage_out[0] = log sum W w (the log-evidence increment), stage_out[1] = ESS / N of the updated weights
__global__ void k_rw_final(const double* __restrict__ part, int n_part, double N, double* __restrict__ logz,
                           double* __restrict__ stage_out) {
    if (threadIdx.x != 0) return;
    double m0 = -INFINITY, s0 = 0.0, m1 = -INFINITY, s1 = 0.0, m2 = -INFINITY, s2 = 0.0;
    for (int i = 0; i < n_part; ++i) {
        const double* p = part + (size_t)i * 6;
        lse_merge(m0, s0, p[0], p[1]);
        lse_merge(m1, s1, p[2], p[3]);
        lse_merge(m2, s2, p[4], p[5]);
    }
    const double l1 = lse_log(m1, s1);
    const double dz = l1 - lse_log(m0, s0);
    const double ess = exp(2.0 * l1 - lse_log(m2, s2)) / N;
    if (stage_out) { stage_out[0] = dz; stage_out[1] = ess == ess ? ess : 0.0; }
    if (logz) *logz += dz;
}

// ---- systematic resampling in fixed point ------------------------------------------------------------------------
__global__ __launch_bounds__(SMC_BLOCK) void k_rs_max(const double* __restrict__ logw, int64_t N,
                                                      double* __restrict__ part) {
    __shared__ double r[SMC_BLOCK];
    double m = -INFINITY;
    for (int64_t n = (int64_t)blockIdx.x * SMC_BLOCK + threadIdx.x; n < N; n += (int64_t)gridDim.x * SMC_BLOCK) {
        const double v = logw[n];
        if (v > m && v < INFINITY) m = v;  // NaN / +inf: zero weight
    }
    r[threadIdx.x] = m;
    __syncthreads();
    for (int s = SMC_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s && r[threadIdx.x + s] > r[threadIdx.x]) r[threadIdx.x] = r[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = r[0];
}

// inclusive scan of 256 values in LDS (Hillis-Steele), integers: exact and order-free
__device__ __forceinline__ uint64_t block_scan_incl(uint64_t v, uint64_t* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < SMC_BLOCK; o <<= 1) {
        const uint64_t add = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    const uint64_t r = sh[t];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(SMC_BLOCK) void k_rs_ticks(const double* __restrict__ logw, int64_t N,
                                                        const double* __restrict__ mpart, int n_mpart,
                                                        uint64_t* __restrict__ ticks, uint64_t* __restrict__ bsum) {
    __shared__ double smax;
    __shared__ uint64_t sh[SMC_BLOCK];
    if (threadIdx.x == 0) {
        double m = -INFINITY;
        for (int i = 0; i < n_mpart; ++i) m = mpart[i] > m ? mpart[i] : m;
        smax = m;
    }
    __syncthreads();
    const double M = smax;
    uint64_t acc = 0;
    const int64_t b0 = (int64_t)blockIdx.x * RS_TILE;
    for (int e = 0; e < RS_TILE / SMC_BLOCK; ++e) {
        const int64_t n = b0 + e * SMC_BLOCK + threadIdx.x;
        if (n >= N) break;
        const double v = logw[n];
        uint64_t tk = 0;
        if (M > -INFINITY && v > -INFINITY && v < INFINITY)
            tk = (uint64_t)(exp(v - M) * (double)(1ull << TICK_BITS));  // truncation = floor, <= 2^32
        ticks[n] = tk;
        acc += tk;
    }
    const uint64_t tot = block_scan_incl(acc, sh);
    if (threadIdx.x == SMC_BLOCK - 1) bsum[blockIdx.x] = tot;
}

// ctl[0] = T (total ticks), ctl[1] = floor(u T), ctl[2] = 1 if this call resamples, ctl[3] = 1 if T == 0
__global__ __launch_bounds__(SMC_BLOCK) void k_rs_top(uint64_t* __restrict__ bsum, int n_blk, uint64_t seed,
                                                      uint64_t stage, const double* __restrict__ ess, double thr,
                                                      uint64_t* __restrict__ ctl, int32_t* __restrict__ status,
                                                      uint8_t* __restrict__ resampled) {
    __shared__ uint64_t sh[SMC_BLOCK];
    uint64_t carry = 0;
    for (int c0 = 0; c0 < n_blk; c0 += SMC_BLOCK) {  // exclusive scan of the block sums, in place
        const int i = c0 + threadIdx.x;
        const uint64_t v = i < n_blk ? bsum[i] : 0;
        const uint64_t inc = block_scan_incl(v, sh);
        if (i < n_blk) bsum[i] = carry + inc - v;
        const uint64_t last = sh[SMC_BLOCK - 1];  // (block_scan_incl leaves sh intact after its final barrier)
        __syncthreads();
        carry += last;
    }
    if (threadIdx.x == 0) {
        const uint64_t T = carry;
        // the stage uniform: block 0xFFFFFFFF of PBBI_STREAM_RESAMPLE at iter = stage, chain 0; k = 53 bits
        const PhiloxOut x = rng_block(seed, (uint32_t)PBBI_STREAM_RESAMPLE, stage, 0, 0xFFFFFFFFu);
        const uint64_t k = (((uint64_t)x.x1 << 32) | x.x0) >> 11;
        const uint64_t hi = __umul64hi(k, T), lo = k * T;
        ctl[0] = T;
        ctl[1] = (hi << 11) | (lo >> 53);  // floor(k T / 2^53) < T
        const bool want = !ess || !(*ess >= thr);
        const bool empty = T == 0;
        ctl[2] = (want && !empty) ? 1 : 0;
        ctl[3] = empty ? 1 : 0;
        if (status) *status = (want && empty) ? PBBI_ERR_INVALID : PBBI_OK;
        if (resampled) *resampled = (want && !empty) ? 1 : 0;
    }
}

__global__ __launch_bounds__(SMC_BLOCK) void k_rs_scan(const uint64_t* __restrict__ ticks, int64_t N,
                                                       const uint64_t* __restrict__ boff, uint64_t* __restrict__ cdf) {
    __shared__ uint64_t sh[SMC_BLOCK];
    constexpr int E = RS_TILE / SMC_BLOCK;
    const int64_t n0 = (int64_t)blockIdx.x * RS_TILE + (int64_t)threadIdx.x * E;
    uint64_t v[E], acc = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        v[e] = n0 + e < N ? ticks[n0 + e] : 0;
        acc += v[e];
    }
    uint64_t run = block_scan_incl(acc, sh) - acc + boff[blockIdx.x];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        run += v[e];
        if (n0 + e < N) cdf[n0 + e] = run;
    }
}

// 128-bit a * b as (hi, lo)
__device__ __forceinline__ void mul128(uint64_t a, uint64_t b, uint64_t& hi, uint64_t& lo) {
    hi = __umul64hi(a, b);
    lo = a * b;
}

// ancestor of output j: the smallest n with C_n N > j T + floor(u T)  (<=> C_n > floor((j T + floor(u T)) / N))
__device__ __forceinline__ int64_t rs_search(const uint64_t* __restrict__ cdf, int64_t N, int64_t j, uint64_t T,
                                             uint64_t uT) {
    uint64_t phi, plo;
    mul128((uint64_t)j, T, phi, plo);
    plo += uT;
    phi += plo < uT ? 1 : 0;
    int64_t lo = 0, hi = N - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        uint64_t chi, clo;
        mul128(cdf[mid], (uint64_t)N, chi, clo);
        if (chi > phi || (chi == phi && clo > plo)) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

template <typename T> struct Vec;
template <> struct Vec<double> { using type = double2; static constexpr int n = 2; };
template <> struct Vec<float> { using type = float4; static constexpr int n = 4; };

// VEC consecutive outputs per thread: ancestors by per-output search (a one-hot weight spreads over all threads),
// then q_out[:, j] = q_in[:, a_j] down the D rows, one VEC-wide store per row where the row is aligned
template <typename T>
__global__ __launch_bounds__(SMC_BLOCK) void k_rs_gather(const uint64_t* __restrict__ cdf, int64_t N,
                                                         const uint64_t* __restrict__ ctl, const T* __restrict__ q_in,
                                                         T* __restrict__ q_out, int64_t ldn, int D, int vec_ok,
                                                         int32_t* __restrict__ anc_out, double* __restrict__ logw) {
    using V = typename Vec<T>::type;
    constexpr int W = Vec<T>::n;
    const int64_t j0 = ((int64_t)blockIdx.x * SMC_BLOCK + threadIdx.x) * W;
    if (j0 >= N) return;
    const bool res = ctl[2] != 0;
    const uint64_t TT = ctl[0], uT = ctl[1];
    int64_t a[W];
#pragma unroll
    for (int i = 0; i < W; ++i) {
        const int64_t j = j0 + i;
        a[i] = j < N ? (res ? rs_search(cdf, N, j, TT, uT) : j) : 0;
        if (j < N) {
            if (anc_out) anc_out[j] = (int32_t)a[i];
            if (res) logw[j] = 0.0;
        }
    }
    const bool full = vec_ok && j0 + W <= N;
    for (int d = 0; d < D; ++d) {
        const T* src = q_in + (int64_t)d * ldn;
        T* dst = q_out + (int64_t)d * ldn;
        T v[W];
#pragma unroll
        for (int i = 0; i < W; ++i) v[i] = src[a[i]];
        if (full) {
            V pk;
            __builtin_memcpy(&pk, v, sizeof(V));
            *reinterpret_cast<V*>(dst + j0) = pk;
        } else {
#pragma unroll
            for (int i = 0; i < W; ++i)
                if (j0 + i < N) dst[j0 + i] = v[i];
        }
    }
}

int check_dtype(int dtype) {
    return (dtype == PBBI_F64 || dtype == PBBI_F32) ? PBBI_OK : pbbi_fail(PBBI_ERR_INVALID, "unknown dtype");
}

// r_n into ws when q is given (stage 1), else nullptr
int ref_term(const void* q, const double* mean, double sigma, int64_t N, int64_t ldn, int D, int dtype, Scratch& ws,
             double** r_out) {
    *r_out = nullptr;
    if (!q) return PBBI_OK;
    if (!(sigma > 0.0)) return pbbi_fail(PBBI_ERR_INVALID, "ref_std must be > 0");
    if (D < 1 || ldn < N) return pbbi_fail(PBBI_ERR_INVALID, "bad D / ldn");
    double* r = (double*)ws.get((size_t)N * 8);
    if (!r) return pbbi_fail(PBBI_ERR_HIP, "hipMallocAsync failed");
    const double inv2s2 = 1.0 / (2.0 * sigma * sigma), cst = 0.5 * D * log(2.0 * M_PI * sigma * sigma);
    const dim3 grid((unsigned)((N + SMC_BLOCK - 1) / SMC_BLOCK));
    if (dtype == PBBI_F64)
        hipLaunchKernelGGL(k_smc_ref<double>, grid, dim3(SMC_BLOCK), 0, ws.st, (const double*)q, N, ldn, D, mean,
                           inv2s2, cst, r);
    else
        hipLaunchKernelGGL(k_smc_ref<float>, grid, dim3(SMC_BLOCK), 0, ws.st, (const float*)q, N, ldn, D, mean,
                           inv2s2, cst, r);
    *r_out = r;
    return PBBI_OK;
}

int scan_launch(const void* U, const double* logw, const double* r, int64_t N, int K, const double* coef, int dtype,
                double* part, int n_part, double* out, hipStream_t st) {
    const dim3 grid((unsigned)n_part, (unsigned)((K + 1 + SCAN_K - 1) / SCAN_K));
    if (dtype == PBBI_F64)
        hipLaunchKernelGGL(k_scan_partial<double>, grid, dim3(SMC_BLOCK), 0, st, (const double*)U, logw, r, N, K,
                           coef, n_part, part);
    else
        hipLaunchKernelGGL(k_scan_partial<float>, grid, dim3(SMC_BLOCK), 0, st, (const float*)U, logw, r, N, K,
                           coef, n_part, part);
    hipLaunchKernelGGL(k_scan_final, dim3((unsigned)((K + 1 + 63) / 64)), dim3(64), 0, st, part, n_part, K, out);
    return PBBI_OK;
}

constexpr int SCAN_PARTS = 256;

}  // namespace

extern "C" {

int pbbi_smc_ess_scan(const void* U, const double* logw, const void* q, const double* ref_mean, double ref_std,
                      int64_t N, int64_t ldn, int D, int K, const double* coefs, int dtype, int device, double* out,
                      void* stream) {
    if (int rc = check_dtype(dtype)) return rc;
    if (N < 1 || K < 1) return pbbi_fail(PBBI_ERR_INVALID, "need N >= 1 and K >= 1");
    if (!U || !coefs || !out) return pbbi_fail(PBBI_ERR_INVALID, "U / coefs / out is NULL");
    DeviceGuard guard(device);
    hipStream_t st = (hipStream_t)stream;
    Scratch ws(st);
    double* r = nullptr;
    if (int rc = ref_term(q, ref_mean, ref_std, N, ldn, D, dtype, ws, &r)) return rc;
    const int n_part = n_parts(N, SMC_BLOCK, SCAN_PARTS);
    double* part = (double*)ws.get((size_t)(K + 1) * n_part * 4 * 8);
    if (!part) return pbbi_fail(PBBI_ERR_HIP, "hipMallocAsync failed");
    scan_launch(U, logw, r, N, K, coefs, dtype, part, n_part, out, st);
    PBBI_HIP(hipGetLastError());
    return PBBI_OK;
}

int pbbi_smc_next_beta(const void* U, const double* logw, const void* q, const double* ref_mean, double ref_std,
                       int64_t N, int64_t ldn, int D, double target_ess, double* betas, double* info_out, int dtype,
                       int device, void* stream) {
    if (int rc = check_dtype(dtype)) return rc;
    if (N < 1) return pbbi_fail(PBBI_ERR_INVALID, "need N >= 1");
    if (!(target_ess > 0.0 && target_ess < 1.0)) return pbbi_fail(PBBI_ERR_INVALID, "target_ess must be in (0, 1)");
    if (!U || !betas) return pbbi_fail(PBBI_ERR_INVALID, "U / betas is NULL");
    DeviceGuard guard(device);
    hipStream_t st = (hipStream_t)stream;
    Scratch ws(st);
    double* r = nullptr;
    if (int rc = ref_term(q, ref_mean, ref_std, N, ldn, D, dtype, ws, &r)) return rc;
    const int n_part = n_parts(N, SMC_BLOCK, SCAN_PARTS);
    double* part = (double*)ws.get((size_t)(NB_GRID + 1) * n_part * 4 * 8);
    double* coef = (double*)ws.get(NB_GRID * 8);
    double* res = (double*)ws.get((3 * NB_GRID + 1) * 8);
    double* sst = (double*)ws.get(8 * 8);
    if (!part || !coef || !res || !sst) return pbbi_fail(PBBI_ERR_HIP, "hipMallocAsync failed");
    hipLaunchKernelGGL(k_nb_init, dim3(1), dim3(NB_GRID), 0, st, (const double*)betas, coef);
    for (int pass = 0; pass <= NB_REFINE; ++pass) {
        scan_launch(U, logw, r, N, NB_GRID, coef, dtype, part, n_part, res, st);
        hipLaunchKernelGGL(k_nb_step, dim3(1), dim3(64), 0, st, (const double*)res, coef, sst, (const double*)betas,
                           pass, q ? 1 : 0, target_ess);
    }
    hipLaunchKernelGGL(k_nb_finish, dim3(1), dim3(64), 0, st, (const double*)sst, betas, info_out);
    PBBI_HIP(hipGetLastError());
    return PBBI_OK;
}

int pbbi_smc_reweight(const void* U, const void* q, const double* ref_mean, double ref_std, int64_t N, int64_t ldn,
                      int D, const double* betas, double* logw, double* logz, double* stage_out, int dtype, int device,
                      void* stream) {
    if (int rc = check_dtype(dtype)) return rc;
    if (N < 1) return pbbi_fail(PBBI_ERR_INVALID, "need N >= 1");
    if (!U || !betas || !logw) return pbbi_fail(PBBI_ERR_INVALID, "U / betas / logw is NULL");
    DeviceGuard guard(device);
    hipStream_t st = (hipStream_t)stream;
    Scratch ws(st);
    double* r = nullptr;
    if (int rc = ref_term(q, ref_mean, ref_std, N, ldn, D, dtype, ws, &r)) return rc;
    const int n_part = n_parts(N, SMC_BLOCK, SCAN_PARTS);
    double* part = (double*)ws.get((size_t)n_part * 6 * 8);
    if (!part) return pbbi_fail(PBBI_ERR_HIP, "hipMallocAsync failed");
    if (dtype == PBBI_F64)
        hipLaunchKernelGGL(k_rw_partial<double>, dim3(n_part), dim3(SMC_BLOCK), 0, st, (const double*)U, r, N, betas,
                           logw, part);
    else
        hipLaunchKernelGGL(k_rw_partial<float>, dim3(n_part), dim3(SMC_BLOCK), 0, st, (const float*)U, r, N, betas,
                           logw, part);
    hipLaunchKernelGGL(k_rw_final, dim3(1), dim3(64), 0, st, (const double*)part, n_part, (double)N, logz, stage_out);
    PBBI_HIP(hipGetLastError());
    return PBBI_OK;
}

int pbbi_smc_resample_systematic(double* logw, int64_t N, uint64_t seed, uint64_t stage, const void* q_in,
                                 void* q_out, int64_t ldn, int D, const double* ess, double threshold,
                                 int32_t* ancestors_out, uint64_t* ticks_out, uint8_t* resampled_out,
                                 int32_t* status_out, int dtype, int device, void* stream) {
    if (int rc = check_dtype(dtype)) return rc;
    if (N < 1 || N > INT32_MAX || D < 1 || ldn < N)
        return pbbi_fail(PBBI_ERR_INVALID, "need 1 <= N < 2^31, D >= 1, ldn >= N");
    if (stage > UINT32_MAX) return pbbi_fail(PBBI_ERR_INVALID, "stage must be < 2^32");
    if (!logw || !q_in || !q_out) return pbbi_fail(PBBI_ERR_INVALID, "logw / q_in / q_out is NULL");
    const size_t es = esize(dtype);
    const char *a0 = (const char*)q_in, *b0 = (const char*)q_out;
    const size_t span = ((size_t)(D - 1) * (size_t)ldn + (size_t)N) * es;
    if (a0 < b0 + span && b0 < a0 + span) return pbbi_fail(PBBI_ERR_INVALID, "q_out must not overlap q_in");
    DeviceGuard guard(device);
    hipStream_t st = (hipStream_t)stream;
    Scratch ws(st);
    const int n_mpart = n_parts(N, SMC_BLOCK, SCAN_PARTS);
    const int64_t n_blk = (N + RS_TILE - 1) / RS_TILE;
    double* mpart = (double*)ws.get((size_t)n_mpart * 8);
    uint64_t* ticks = ticks_out ? ticks_out : (uint64_t*)ws.get((size_t)N * 8);
    uint64_t* cdf = (uint64_t*)ws.get((size_t)N * 8);
    uint64_t* bsum = (uint64_t*)ws.get((size_t)n_blk * 8);
    uint64_t* ctl = (uint64_t*)ws.get(4 * 8);
    int32_t* status = status_out ? status_out : (int32_t*)ws.get(4);
    if (!mpart || !ticks || !cdf || !bsum || !ctl || !status) return pbbi_fail(PBBI_ERR_HIP, "hipMallocAsync failed");
    hipLaunchKernelGGL(k_rs_max, dim3(n_mpart), dim3(SMC_BLOCK), 0, st, (const double*)logw, N, mpart);
    hipLaunchKernelGGL(k_rs_ticks, dim3((unsigned)n_blk), dim3(SMC_BLOCK), 0, st, (const double*)logw, N,
                       (const double*)mpart, n_mpart, ticks, bsum);
    hipLaunchKernelGGL(k_rs_top, dim3(1), dim3(SMC_BLOCK), 0, st, bsum, (int)n_blk, seed, stage, ess, threshold, ctl,
                       status, resampled_out);
    hipLaunchKernelGGL(k_rs_scan, dim3((unsigned)n_blk), dim3(SMC_BLOCK), 0, st, (const uint64_t*)ticks, N,
                       (const uint64_t*)bsum, cdf);
    const int W = dtype == PBBI_F64 ? 2 : 4;
    const int vec_ok = (ldn % W == 0) && ((uintptr_t)q_out % 16 == 0);
    const dim3 grid((unsigned)((N + (int64_t)SMC_BLOCK * W - 1) / ((int64_t)SMC_BLOCK * W)));
    if (dtype == PBBI_F64)
        hipLaunchKernelGGL(k_rs_gather<double>, grid, dim3(SMC_BLOCK), 0, st, (const uint64_t*)cdf, N,
                           (const uint64_t*)ctl, (const double*)q_in, (double*)q_out, ldn, D, vec_ok, ancestors_out,
                           logw);
    else
        hipLaunchKernelGGL(k_rs_gather<float>, grid, dim3(SMC_BLOCK), 0, st, (const uint64_t*)cdf, N,
                           (const uint64_t*)ctl, (const float*)q_in, (float*)q_out, ldn, D, vec_ok, ancestors_out,
                           logw);
    PBBI_HIP(hipGetLastError());
    if (!status_out) {  // synchronous form: report an all-zero weight vector as the call's status
        int32_t h = 0;
        PBBI_HIP(hipMemcpyAsync(&h, status, 4, hipMemcpyDeviceToHost, st));
        PBBI_HIP(hipStreamSynchronize(st));
        if (h != PBBI_OK) return pbbi_fail(PBBI_ERR_INVALID, "every resampling weight is zero (non-finite logw)");
    }
    return PBBI_OK;
}

}  // extern "C"
