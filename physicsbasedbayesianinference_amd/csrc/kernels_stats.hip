// kernels_stats.hip -- the running statistics sink (include/pbbi.h, "running statistics"): a
// device-resident state that one pass over each chunk's (c, D, N) slabs updates and that can be finalised at any
// time into what pbbi_sample_moments / pbbi_chain_moments / pbbi_chain_autocov / pbbi_sample_covariance return for
// the whole run.  Only one chunk is ever resident.
//
// State (doubles; M = D*N; the per-(dim, chain) arrays hold element (d, n) at d*N + n: chain axis fastest):
//     [0,        M)             c      the chain's first accumulated draw (the shift); y_s = x_s - c
//     [M,        2M)            s1     sum_s y_s
//     [2M,       (3+T)M)        A_t    sum_{s>=t} y_s y_{s-t},  t = 0..T
//     [(3+T)M,   (3+2T)M)       win_k  y_{S-1-k}, k = 0..T-1 (the last T values, newest first; 0 where S <= k)
//     [(3+2T)M,  (3+3T)M)       head_k y_k,       k = 0..T-1 (the first T values; written once, while S <= T)
//     then per ensemble:        shift (D) | e = sum (x - shift) (D) | P = sum (x - shift)(x - shift)^T (D*D, the
//                               16x16 tiles on and above the diagonal)
// = (3T + 3) D N + 2 D + D^2 doubles (pbbi_stats_state_len): a lag that was not asked for has no state.
#include "pbbi_internal.h"

namespace {

struct StatsLayout {
    int64_t M, s1, A, win, head, shift, e, P, len;
    StatsLayout(int D, int64_t N, int T) {
        M = (int64_t)D * N;
        s1 = M;
        A = 2 * M;
        win = (3 + (int64_t)T) * M;
        head = (3 + 2 * (int64_t)T) * M;
        shift = (3 + 3 * (int64_t)T) * M;
        e = shift + D;
        P = e + D;
        len = P + (int64_t)D * D;
    }
};

// sum of v over the 256 threads of a block, in a fixed order; every thread of the block calls it
__device__ inline double block_sum(double v, double* r) {
    r[threadIdx.x] = v;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) r[threadIdx.x] += r[threadIdx.x + k];
        __syncthreads();
    }
    const double s = r[0];
    __syncthreads();
    return s;
}

// THE per-draw update of one chain's state (the only one): shifted value, sum, window, lagged products.  Draws go
// through it one after the other in draw order, so the state after S draws does not depend on how they were cut
// into chunks.  Lags past T (TW > T) are computed in registers and never stored.
template <int TW>
__device__ __forceinline__ double stats_step(double v, double c, double& s1, double (&a)[TW + 1], double (&w)[TW + 1]) {
    const double y = v - c;
    s1 += y;
#pragma unroll
    for (int t = TW; t > 0; --t) w[t] = w[t - 1];
    w[0] = y;
#pragma unroll
    for (int t = 0; t <= TW; ++t) a[t] = fma(y, w[t], a[t]);
    return y;
}

// one thread per (dim, chain), lanes along the chain axis: loads the chain's state (or starts it when S0 == 0),
// runs the chunk's c draws through stats_step, stores the state.  TW >= T: the compile-time size of the register
// window and of the lag sums.
template <typename X, int TW>
__global__ void __launch_bounds__(256) k_stats_accumulate(double* __restrict__ st, const X* __restrict__ x, int c,
                                                          int D, int64_t N, int T, int64_t S0) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;  // (no barrier in this kernel)
    const int64_t M = (int64_t)D * N, i = (int64_t)blockIdx.y * N + n;
    double* A = st + 2 * M + i;
    double* win = st + (3 + (int64_t)T) * M + i;
    double* head = st + (3 + 2 * (int64_t)T) * M + i;
    const X* xp = x + i;
    double a[TW + 1], w[TW + 1], shift, s1;
    if (S0 == 0) {
        shift = (double)xp[0];
        s1 = 0.0;
#pragma unroll
        for (int t = 0; t <= TW; ++t) { a[t] = 0.0; w[t] = 0.0; }
    } else {
        shift = st[i];
        s1 = st[M + i];
#pragma unroll
        for (int t = 0; t <= TW; ++t) {
            a[t] = t <= T ? A[(int64_t)t * M] : 0.0;
            w[t] = t < T ? win[(int64_t)t * M] : 0.0;
        }
    }
    int s = 0;
    for (; s + 4 <= c; s += 4) {  // four loads in flight, then the four updates in order
        X v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = xp[(int64_t)(s + k) * M];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double y = stats_step<TW>((double)v[k], shift, s1, a, w);
            const int64_t sg = S0 + s + k;
            if (sg < T) head[sg * M] = y;
        }
    }
    for (; s < c; ++s) {
        const double y = stats_step<TW>((double)xp[(int64_t)s * M], shift, s1, a, w);
        const int64_t sg = S0 + s;
        if (sg < T) head[sg * M] = y;
    }
    if (S0 == 0) st[i] = shift;
    st[M + i] = s1;
#pragma unroll
    for (int t = 0; t <= TW; ++t) {
        if (t <= T) A[(int64_t)t * M] = a[t];
        if (t < T) win[(int64_t)t * M] = w[t];
    }
}

// the ensemble shift: shift[d] = mean over the chains of the first slab (block d; fixed order)
template <typename X>
__global__ void __launch_bounds__(256) k_stats_shift(const X* __restrict__ x, int64_t N, double* __restrict__ shift) {
    __shared__ double r[256];
    const int d = blockIdx.x;
    double s = 0.0;
    for (int64_t n = threadIdx.x; n < N; n += 256) s += (double)x[(int64_t)d * N + n];
    const double tot = block_sum(s, r);
    if (threadIdx.x == 0) shift[d] = tot / (double)N;
}

// k_cov_partial's scheme (pbbi_api.hip) on one chunk: a 16x16 tile of sum_m (x_i - shift_i)(x_j - shift_j) over a
// slice of the chunk's c*N draws, tiles on and above the diagonal; the diagonal tiles also sum x_i - shift_i
template <typename X>
__global__ void __launch_bounds__(256) k_stats_cov_partial(const X* __restrict__ x, const double* __restrict__ shift,
                                                           int c, int D, int64_t N, int chunks,
                                                           double* __restrict__ part /* [chunks][D][D] */,
                                                           double* __restrict__ epart /* [chunks][D] */) {
    const int ti = blockIdx.y, tj = blockIdx.z;
    if (tj < ti) return;  // (block-uniform: no thread of the block reaches a barrier)
    const int li = threadIdx.x >> 4, lj = threadIdx.x & 15;
    const int64_t Mt = (int64_t)c * N;
    const int64_t per = ((Mt + chunks - 1) / chunks + 63) / 64 * 64;
    const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < Mt ? lo + per : Mt;
    __shared__ double xi[16][65], xj[16][65];
    const bool sums = ti == tj && lj == 0;
    double acc = 0.0, esum = 0.0;
    for (int64_t m0 = lo; m0 < hi; m0 += 64) {
        for (int k = threadIdx.x; k < 16 * 64; k += 256) {  // rows of the two tiles, 64 draws each
            const int row = k >> 6, cc = k & 63;
            const int64_t m = m0 + cc;
            double a = 0.0, b = 0.0;
            if (m < hi) {
                const int64_t s = m / N, n = m - s * N;
                const int di = ti * 16 + row, dj = tj * 16 + row;
                if (di < D) a = (double)x[(s * D + di) * N + n] - shift[di];
                if (dj < D) b = (double)x[(s * D + dj) * N + n] - shift[dj];
            }
            xi[row][cc] = a;
            xj[row][cc] = b;
        }
        __syncthreads();
#pragma unroll 16
        for (int cc = 0; cc < 64; ++cc) acc = fma(xi[li][cc], xj[lj][cc], acc);
        if (sums)
            for (int cc = 0; cc < 64; ++cc) esum += xi[li][cc];
        __syncthreads();
    }
    const int i = ti * 16 + li, j = tj * 16 + lj;
    if (i < D && j < D) part[((size_t)blockIdx.x * D + i) * D + j] = acc;
    if (sums && i < D) epart[(size_t)blockIdx.x * D + i] = esum;
}

// P += the chunk partials, e += theirs, each in a fixed order (first: the state starts here)
__global__ void k_stats_cov_add(const double* __restrict__ part, const double* __restrict__ epart, int chunks, int D,
                                int first, double* __restrict__ e, double* __restrict__ P) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < D) {
        double s = 0.0;
        for (int k = 0; k < chunks; ++k) s += epart[(size_t)k * D + idx];
        e[idx] = (first ? 0.0 : e[idx]) + s;
    }
    if (idx >= D * D) return;
    const int i = idx / D, j = idx - i * D;
    if ((j >> 4) < (i >> 4)) return;  // tiles below the diagonal are not kept
    double s = 0.0;
    for (int k = 0; k < chunks; ++k) s += part[((size_t)k * D + i) * D + j];
    P[idx] = (first ? 0.0 : P[idx]) + s;
}

// ---- finalisation -----------------------------------------------------------------------------------------------
// Stage 1 over the chains: block (b, d) forms, for its 256 chains, the chain mean m = c + s1/S and the centred lag sums
//     C_t = A_t - delta (2 s1 - head_t - tail_t) + (S - t) delta^2,  delta = s1/S,  t < S   (0 for t >= S),
// head_t / tail_t the sums of the first / last t values of y, and sums them over the block lag by lag.
// part: [blocks][D][T+2], slots 0..T = sum C_t, slot T+1 = sum m.  The state is only read.
__global__ void __launch_bounds__(256) k_stats_chain_final(const double* __restrict__ st, int D, int64_t N, int T,
                                                           int64_t S, double* __restrict__ chain_mean,
                                                           double* __restrict__ chain_var, double* __restrict__ part) {
    __shared__ double r[256];
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int d = blockIdx.y;
    const bool valid = n < N;  // the work is guarded, the barriers are not
    const int64_t M = (int64_t)D * N, i = (int64_t)d * N + (valid ? n : 0);
    const double* A = st + 2 * M + i;
    const double* win = st + (3 + (int64_t)T) * M + i;
    const double* head = st + (3 + 2 * (int64_t)T) * M + i;
    double* out = part + ((size_t)blockIdx.x * D + d) * (T + 2);
    double s1 = 0.0, delta = 0.0, m = 0.0;
    if (valid) {
        s1 = st[M + i];
        delta = s1 / (double)S;
        m = st[i] + delta;
        if (chain_mean) chain_mean[i] = m;
    }
    const double msum = block_sum(m, r);
    if (threadIdx.x == 0) out[T + 1] = msum;
    double hs = 0.0, ts = 0.0;
    for (int t = 0; t <= T; ++t) {
        double Ct = 0.0;
        if (valid && t < S) {
            if (t > 0) {
                hs += head[(int64_t)(t - 1) * M];
                ts += win[(int64_t)(t - 1) * M];
            }
            Ct = A[(int64_t)t * M] - delta * (2.0 * s1 - hs - ts) + (double)(S - t) * (delta * delta);
            if (t == 0 && chain_var) chain_var[i] = Ct / (double)(S - 1);
        }
        const double csum = block_sum(Ct, r);
        if (threadIdx.x == 0) out[t] = csum;
    }
}

// Stage 2: the block partials of one (slot, dim) in block order.  tot: [T+2][D] (slot T+1 holds the MEAN, not the sum)
__global__ void k_stats_final_sums(const double* __restrict__ part, int n_blocks, int D, int64_t N, int T, int64_t S,
                                   double* __restrict__ tot, double* __restrict__ mean, double* __restrict__ acov,
                                   double* __restrict__ W) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;  // slot*D + d
    if (idx >= (T + 2) * D) return;
    const int slot = idx / D, d = idx - slot * D;
    double s = 0.0;
    for (int b = 0; b < n_blocks; ++b) s += part[((size_t)b * D + d) * (T + 2) + slot];
    if (slot == T + 1) {
        s = s / (double)N;
        if (mean) mean[d] = s;
    } else {
        if (acov) acov[idx] = s / ((double)S * (double)N);
        if (slot == 0 && W) W[d] = s / ((double)(S - 1) * (double)N);
    }
    tot[idx] = s;
}

// the chain means about the ensemble mean: block partials of sum_n (m_n - mean_d)^2
__global__ void __launch_bounds__(256) k_stats_dev_partial(const double* __restrict__ st, int D, int64_t N, int64_t S,
                                                           const double* __restrict__ mean /* tot slot T+1 */,
                                                           double* __restrict__ part2 /* [blocks][D] */) {
    __shared__ double r[256];
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int d = blockIdx.y;
    const int64_t M = (int64_t)D * N;
    double q = 0.0;
    if (n < N) {
        const int64_t i = (int64_t)d * N + n;
        const double dev = st[i] + st[M + i] / (double)S - mean[d];
        q = dev * dev;
    }
    const double s = block_sum(q, r);
    if (threadIdx.x == 0) part2[(size_t)blockIdx.x * D + d] = s;
}

// bvar = the biased variance over chains of the chain means; var = within + between, over all S*N draws
__global__ void k_stats_final_var(const double* __restrict__ part2, int n_blocks, int D, int64_t N, int64_t S,
                                  const double* __restrict__ c0 /* tot slot 0 */, double* __restrict__ var,
                                  double* __restrict__ bvar) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    double s = 0.0;
    for (int b = 0; b < n_blocks; ++b) s += part2[(size_t)b * D + d];
    const double bv = s / (double)N;
    if (bvar) bvar[d] = bv;
    if (var) var[d] = c0[d] / ((double)S * (double)N) + bv;
}

// cov = P / count - (e / count)(e / count)^T; tiles below the diagonal mirror the upper ones
__global__ void k_stats_cov_out(const double* __restrict__ e, const double* __restrict__ P, int D, double count,
                                double* __restrict__ cov) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= D * D) return;
    const int i = idx / D, j = idx - i * D;
    int pi = i, pj = j;
    if ((j >> 4) < (i >> 4)) { pi = j; pj = i; }
    cov[idx] = P[(size_t)pi * D + pj] / count - (e[i] / count) * (e[j] / count);
}

template <typename X, int TW>
void launch_accumulate(double* st, const void* x, int c, int D, int64_t N, int T, int64_t S0, hipStream_t s) {
    const dim3 grid((unsigned)((N + 255) / 256), (unsigned)D), block(256);
    hipLaunchKernelGGL((k_stats_accumulate<X, TW>), grid, block, 0, s, st, (const X*)x, c, D, N, T, S0);
}

template <typename X>
void route_accumulate(double* st, const void* x, int c, int D, int64_t N, int T, int64_t S0, hipStream_t s) {
    if (T == 0) launch_accumulate<X, 0>(st, x, c, D, N, T, S0, s);
    else if (T <= 4) launch_accumulate<X, 4>(st, x, c, D, N, T, S0, s);
    else if (T <= 8) launch_accumulate<X, 8>(st, x, c, D, N, T, S0, s);
    else if (T <= 16) launch_accumulate<X, 16>(st, x, c, D, N, T, S0, s);
    else launch_accumulate<X, PBBI_MAX_LAG>(st, x, c, D, N, T, S0, s);
}

int check_shape(int D, int64_t N, int T) {
    if (D < 1 || N < 1) return pbbi_fail(PBBI_ERR_INVALID, "D and N must be >= 1");
    if (D > 65535) return pbbi_fail(PBBI_ERR_INVALID, "D must be <= 65535");
    if (T < 0 || T > PBBI_MAX_LAG) return pbbi_fail(PBBI_ERR_INVALID, "T must be in [0, PBBI_MAX_LAG]");
    return PBBI_OK;
}

}  // namespace

extern "C" {

int pbbi_stats_state_len(int D, int64_t N, int T, int64_t* doubles_out) {
    if (const int rc = check_shape(D, N, T)) return rc;
    if (!doubles_out) return pbbi_fail(PBBI_ERR_INVALID, "doubles_out is NULL");
    *doubles_out = StatsLayout(D, N, T).len;
    return PBBI_OK;
}

int pbbi_stats_accumulate(double* state, int D, int64_t N, int T, int64_t S_before, const void* slabs_sdn, int c,
                          int dtype, int device, void* stream) {
    if (const int rc = check_shape(D, N, T)) return rc;
    if (c < 1) return pbbi_fail(PBBI_ERR_INVALID, "c must be >= 1");
    if (S_before < 0) return pbbi_fail(PBBI_ERR_INVALID, "S_before must be >= 0");
    if (!state) return pbbi_fail(PBBI_ERR_INVALID, "state is NULL");
    if (!slabs_sdn) return pbbi_fail(PBBI_ERR_INVALID, "slabs is NULL");
    if (dtype != PBBI_F64 && dtype != PBBI_F32) return pbbi_fail(PBBI_ERR_INVALID, "unknown dtype");
    DeviceGuard guard(device);
    hipStream_t st = (hipStream_t)stream;
    const StatsLayout lay(D, N, T);
    const int first = S_before == 0;
    // the per-(dim, chain) state
    if (dtype == PBBI_F64) route_accumulate<double>(state, slabs_sdn, c, D, N, T, S_before, st);
    else route_accumulate<float>(state, slabs_sdn, c, D, N, T, S_before, st);
    // the ensemble sums, shifted by the first slab's mean over the chains
    if (first) {
        if (dtype == PBBI_F64)
            hipLaunchKernelGGL(k_stats_shift<double>, dim3((unsigned)D), dim3(256), 0, st, (const double*)slabs_sdn, N,
                               state + lay.shift);
        else
            hipLaunchKernelGGL(k_stats_shift<float>, dim3((unsigned)D), dim3(256), 0, st, (const float*)slabs_sdn, N,
                               state + lay.shift);
    }
    const int tiles = (D + 15) / 16;
    const int64_t Mt = (int64_t)c * N;
    int chunks = (int)(Mt / 4096 > 0 ? (Mt / 4096 > 1024 ? 1024 : Mt / 4096) : 1);
    const int max_chunks = tiles * tiles >= 64 ? 64 : 1024 / (tiles * tiles);
    if (chunks > max_chunks) chunks = max_chunks;
    double* part = nullptr;
    PBBI_HIP(hipMallocAsync((void**)&part, sizeof(double) * (size_t)chunks * D * ((size_t)D + 1), st));
    double* epart = part + (size_t)chunks * D * D;
    const dim3 grid((unsigned)chunks, (unsigned)tiles, (unsigned)tiles), block(256);
    if (dtype == PBBI_F64)
        hipLaunchKernelGGL(k_stats_cov_partial<double>, grid, block, 0, st, (const double*)slabs_sdn,
                           (const double*)(state + lay.shift), c, D, N, chunks, part, epart);
    else
        hipLaunchKernelGGL(k_stats_cov_partial<float>, grid, block, 0, st, (const float*)slabs_sdn,
                           (const double*)(state + lay.shift), c, D, N, chunks, part, epart);
    hipLaunchKernelGGL(k_stats_cov_add, dim3((unsigned)(((int64_t)D * D + 255) / 256)), dim3(256), 0, st,
                       (const double*)part, (const double*)epart, chunks, D, first, state + lay.e, state + lay.P);
    PBBI_HIP(hipGetLastError());
    PBBI_HIP(hipFreeAsync(part, st));
    return PBBI_OK;
}

int pbbi_stats_finalize(const double* state, int D, int64_t N, int T, int64_t S_total, int device, double* mean_out,
                        double* var_out, double* cov_out, double* acov_out, double* w_out, double* bvar_out,
                        double* chain_mean_out, double* chain_var_out, void* stream) {
    if (const int rc = check_shape(D, N, T)) return rc;
    if (S_total < 1) return pbbi_fail(PBBI_ERR_INVALID, "S_total must be >= 1");
    if (S_total < 2 && (w_out || chain_var_out))
        return pbbi_fail(PBBI_ERR_INVALID, "the unbiased chain variances need S_total >= 2");
    if (!state) return pbbi_fail(PBBI_ERR_INVALID, "state is NULL");
    DeviceGuard guard(device);
    hipStream_t st = (hipStream_t)stream;
    const StatsLayout lay(D, N, T);
    if (cov_out)
        hipLaunchKernelGGL(k_stats_cov_out, dim3((unsigned)(((int64_t)D * D + 255) / 256)), dim3(256), 0, st,
                           state + lay.e, state + lay.P, D, (double)S_total * (double)N, cov_out);
    if (mean_out || var_out || acov_out || w_out || bvar_out || chain_mean_out || chain_var_out) {
        const int n_blocks = (int)((N + 255) / 256);
        const size_t n_part = (size_t)n_blocks * D * (T + 2), n_tot = (size_t)(T + 2) * D, n_part2 = (size_t)n_blocks * D;
        double* part = nullptr;
        PBBI_HIP(hipMallocAsync((void**)&part, sizeof(double) * (n_part + n_tot + n_part2), st));
        double *tot = part + n_part, *part2 = tot + n_tot;
        const dim3 grid((unsigned)n_blocks, (unsigned)D), block(256);
        hipLaunchKernelGGL(k_stats_chain_final, grid, block, 0, st, state, D, N, T, S_total, chain_mean_out,
                           chain_var_out, part);
        hipLaunchKernelGGL(k_stats_final_sums, dim3((unsigned)((n_tot + 255) / 256)), dim3(256), 0, st,
                           (const double*)part, n_blocks, D, N, T, S_total, tot, mean_out, acov_out, w_out);
        if (var_out || bvar_out) {
            hipLaunchKernelGGL(k_stats_dev_partial, grid, block, 0, st, state, D, N, S_total,
                               (const double*)(tot + (size_t)(T + 1) * D), part2);
            hipLaunchKernelGGL(k_stats_final_var, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, st,
                               (const double*)part2, n_blocks, D, N, S_total, (const double*)tot, var_out, bvar_out);
        }
        PBBI_HIP(hipGetLastError());
        PBBI_HIP(hipFreeAsync(part, st));
    }
    PBBI_HIP(hipGetLastError());
    return PBBI_OK;
}

}  // extern "C"
