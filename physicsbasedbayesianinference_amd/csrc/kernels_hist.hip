// kernels_hist.hip -- the running histogram sink (include/pbbi.h, "running histogram"): per dimension a
// histogram of `bins` equal bins pooled over all chains and draws, two tail bins, the extreme values and a NaN count, updated
// by one pass over each chunk's (c, D, N) slabs.  Every accumulated quantity is an integer count or an exact minimum / maximum:
// the state after a run does not depend on how the run was cut into chunks, on the launch shape or on the order in which the
// atomic additions arrive.  The state layout, the argument rules and the launch shape are hist_host.h's.
//
// The bin of a value x (converted to double first), with lo, hi and inv = bins / (hi - lo) of its dimension:
//     x != x:   no bin, nan += 1
//     x <  lo:  bin 0          x >= hi:  bin bins + 1          else  bin 1 + min(floor((x - lo) * inv), bins - 1)
#include "hist_host.h"
#include "pbbi_internal.h"

namespace {

constexpr int HIST_THREADS = 256;

// The order of the extremes is total: -0.0 sorts below +0.0, so a minimum or maximum has the same bits whichever order its
// candidates arrive in.
__device__ __forceinline__ double hist_min(double a, double b) { return (b < a || (b == a && signbit(b))) ? b : a; }
__device__ __forceinline__ double hist_max(double a, double b) { return (b > a || (b == a && !signbit(b))) ? b : a; }

// f(value as double) for every element of a workgroup's slice: draws [s_lo, s_hi) of dimension d, chains [n_lo, n_hi).  Each
// row is read with 16-byte loads from its first 16-byte boundary on (a row of an odd N starts 8 bytes off it; fp32 rows 4, 8 or
// 12), four loads in flight per lane; the elements before that boundary and after the last whole vector are read one by one.
template <typename X, typename F>
__device__ __forceinline__ void hist_for_each(const X* __restrict__ x, int D, int64_t N, int d, int s_lo, int s_hi, int64_t n_lo,
                                              int64_t n_hi, F&& f) {
    constexpr int V = 16 / (int)sizeof(X);
    typedef X Vec __attribute__((ext_vector_type(V)));
    const int64_t len = n_hi - n_lo;
    const int tid = threadIdx.x;
    for (int s = s_lo; s < s_hi; ++s) {
        const X* row = x + ((int64_t)s * D + d) * N + n_lo;
        int64_t head = (int64_t)((0 - (uintptr_t)row / sizeof(X)) & (uintptr_t)(V - 1));
        if (head > len) head = len;
        const int64_t nvec = (len - head) / V, tail0 = head + nvec * V;
        const Vec* vp = reinterpret_cast<const Vec*>(row + head);
        int64_t i = tid;
        for (; i + 3 * HIST_THREADS < nvec; i += 4 * HIST_THREADS) {
            Vec v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = vp[i + k * HIST_THREADS];
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int j = 0; j < V; ++j) f((double)v[k][j]);
        }
        for (; i < nvec; i += HIST_THREADS) {
            const Vec v = vp[i];
#pragma unroll
            for (int j = 0; j < V; ++j) f((double)v[j]);
        }
        if (tid < head) f((double)row[tid]);
        if (tail0 + tid < len) f((double)row[tail0 + tid]);
    }
}

// the slice of this workgroup (hist_host.h: HistShape)
struct HistSlice {
    int d, s_lo, s_hi;
    int64_t n_lo, n_hi, part;  // part: the slot of this workgroup's {min, max} pair
    __device__ HistSlice(int c, int64_t N, int rows_per_block) {
        d = blockIdx.z;
        const int64_t s0 = (int64_t)blockIdx.y * rows_per_block;  // < c (hist_launch_shape)
        s_lo = (int)s0;
        s_hi = s0 + rows_per_block < c ? (int)(s0 + rows_per_block) : c;
        n_lo = (int64_t)blockIdx.x * HIST_COLS;
        n_hi = n_lo + HIST_COLS < N ? n_lo + HIST_COLS : N;
        part = ((int64_t)d * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    }
};

// {min, max} over the workgroup, written by thread 0 to part[0], part[1]; every thread of the block calls it
__device__ __forceinline__ void hist_block_extremes(double mn, double mx, double* __restrict__ part) {
    __shared__ double r[2][HIST_THREADS / 64];
    for (int o = 32; o > 0; o >>= 1) {
        mn = hist_min(mn, __shfl_xor(mn, o));
        mx = hist_max(mx, __shfl_xor(mx, o));
    }
    if ((threadIdx.x & 63) == 0) {
        r[0][threadIdx.x >> 6] = mn;
        r[1][threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < HIST_THREADS / 64; ++w) {
            mn = hist_min(mn, r[0][w]);
            mx = hist_max(mx, r[1][w]);
        }
        part[0] = mn;
        part[1] = mx;
    }
}

// auto range, pass 1: the finite minimum and maximum of each workgroup's slice (+inf / -inf where it holds no finite value)
template <typename X>
__global__ void __launch_bounds__(HIST_THREADS) k_hist_finite_extremes(const X* __restrict__ x, int c, int D, int64_t N,
                                                                        int rows_per_block, double* __restrict__ part) {
    const HistSlice sl(c, N, rows_per_block);
    double mn = INFINITY, mx = -INFINITY;
    hist_for_each(x, D, N, sl.d, sl.s_lo, sl.s_hi, sl.n_lo, sl.n_hi, [&](double v) {
        if (fabs(v) < INFINITY) {  // (false for a NaN)
            mn = hist_min(mn, v);
            mx = hist_max(mx, v);
        }
    });
    hist_block_extremes(mn, mx, part + 2 * sl.part);
}

// the {min, max} partials of dimension blockIdx.x over its per_dim workgroups; every thread of the block calls it, thread 0
// holds the result
__device__ __forceinline__ void hist_merge_partials(const double* __restrict__ part, int64_t per_dim, double& mn, double& mx) {
    __shared__ double r[2][HIST_THREADS];
    const double* p = part + 2 * (int64_t)blockIdx.x * per_dim;
    mn = INFINITY;
    mx = -INFINITY;
    for (int64_t i = threadIdx.x; i < per_dim; i += HIST_THREADS) {
        mn = hist_min(mn, p[2 * i]);
        mx = hist_max(mx, p[2 * i + 1]);
    }
    r[0][threadIdx.x] = mn;
    r[1][threadIdx.x] = mx;
    __syncthreads();
    for (int k = HIST_THREADS / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) {
            r[0][threadIdx.x] = hist_min(r[0][threadIdx.x], r[0][threadIdx.x + k]);
            r[1][threadIdx.x] = hist_max(r[1][threadIdx.x], r[1][threadIdx.x + k]);
        }
        __syncthreads();
    }
    mn = r[0][0];
    mx = r[1][0];
}

// auto range, pass 2 (block d): a, b = the finite extremes of the first chunk (0, 0 without a finite value);
//     span = b - a;  lo = a - margin * span;  hi = b + margin * span;  !(hi > lo):  lo = a - 0.5, hi = a + 0.5
// writes the header of dimension d and zeroes its counts: the state starts here, whatever the buffer held.  (A span or a margin
// times it that overflows gives lo = -inf, hi = +inf, inv = 0: every finite value then lands in bin `bins`.)
__global__ void __launch_bounds__(HIST_THREADS) k_hist_auto_range(double* __restrict__ st, int D, int bins, double margin,
                                                                  const double* __restrict__ part, int64_t per_dim) {
    const HistLayout lay(D, bins);
    const int d = blockIdx.x;
    double a, b;
    hist_merge_partials(part, per_dim, a, b);
    if (threadIdx.x == 0) {
        if (a > b) a = b = 0.0;
        const double span = b - a;
        double lo = a - margin * span, hi = b + margin * span;
        if (!(hi > lo)) {
            lo = a - 0.5;
            hi = a + 0.5;
        }
        st[lay.lo + d] = lo;
        st[lay.hi + d] = hi;
        st[lay.inv + d] = (double)bins / (hi - lo);
        st[lay.min + d] = INFINITY;
        st[lay.max + d] = -INFINITY;
        st[lay.nan + d] = 0.0;  // the all-zero word
    }
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(st) + lay.counts + (int64_t)d * lay.stride;
    for (int k = threadIdx.x; k < bins + 2; k += HIST_THREADS) counts[k] = 0ull;
}

// The counting pass.  A workgroup owns one dimension and a slice of (draws x chains) of at most 2^31 values (hist_host.h: no
// 32-bit counter can wrap), counts it into bins + 2 counters in LDS with LDS atomics and adds its non-zero counters to the
// 64-bit counts of the state: integer additions, which commute, so the sums do not depend on the order of arrival.  The NaN
// count goes the same way; the extremes over all non-NaN values (infinities included) leave as one pair per workgroup.
template <typename X>
__global__ void __launch_bounds__(HIST_THREADS) k_hist_count(double* __restrict__ st, const X* __restrict__ x, int c, int D,
                                                              int64_t N, int bins, int rows_per_block,
                                                              double* __restrict__ part) {
    extern __shared__ unsigned int cnt[];  // bins + 2
    const HistLayout lay(D, bins);
    const HistSlice sl(c, N, rows_per_block);
    for (int k = threadIdx.x; k < bins + 2; k += HIST_THREADS) cnt[k] = 0u;
    __syncthreads();
    const double lo = st[lay.lo + sl.d], hi = st[lay.hi + sl.d], inv = st[lay.inv + sl.d];
    const double top = (double)(bins - 1);
    double mn = INFINITY, mx = -INFINITY;
    unsigned int nan = 0u;
    hist_for_each(x, D, N, sl.d, sl.s_lo, sl.s_hi, sl.n_lo, sl.n_hi, [&](double v) {
        if (v != v) {
            ++nan;
            return;
        }
        mn = hist_min(mn, v);
        mx = hist_max(mx, v);
        int k;
        if (v < lo) k = 0;
        else if (v >= hi) k = bins + 1;
        else {
            const double f = floor((v - lo) * inv);  // >= 0 here; a NaN (inv = 0 of an overflowed range) takes the last bin
            k = 1 + (f < top ? (int)f : bins - 1);
        }
        atomicAdd(&cnt[k], 1u);
    });
    __syncthreads();
    unsigned long long* words = reinterpret_cast<unsigned long long*>(st);
    unsigned long long* counts = words + lay.counts + (int64_t)sl.d * lay.stride;
    for (int k = threadIdx.x; k < bins + 2; k += HIST_THREADS) {
        const unsigned int n = cnt[k];
        if (n) atomicAdd(&counts[k], (unsigned long long)n);
    }
    for (int o = 32; o > 0; o >>= 1) nan += __shfl_xor(nan, o);
    if ((threadIdx.x & 63) == 0 && nan) atomicAdd(&words[lay.nan + sl.d], (unsigned long long)nan);
    hist_block_extremes(mn, mx, part + 2 * sl.part);
}

// min / max of the state (block d) <- with the chunk's partials
__global__ void __launch_bounds__(HIST_THREADS) k_hist_merge_extremes(double* __restrict__ st, int D, int bins,
                                                                      const double* __restrict__ part, int64_t per_dim) {
    const HistLayout lay(D, bins);
    const int d = blockIdx.x;
    double mn, mx;
    hist_merge_partials(part, per_dim, mn, mx);
    if (threadIdx.x == 0) {
        st[lay.min + d] = hist_min(st[lay.min + d], mn);
        st[lay.max + d] = hist_max(st[lay.max + d], mx);
    }
}

template <typename X>
void launch_chunk(double* st, const X* x, int c, int D, int64_t N, int bins, bool auto_range, double margin,
                  const HistShape& shape, double* part, hipStream_t s) {
    const dim3 grid((unsigned)shape.col_chunks, (unsigned)shape.row_chunks, (unsigned)D), block(HIST_THREADS);
    const int64_t per_dim = shape.per_dim();
    if (auto_range) {
        hipLaunchKernelGGL(k_hist_finite_extremes<X>, grid, block, 0, s, x, c, D, N, shape.rows_per_block, part);
        hipLaunchKernelGGL(k_hist_auto_range, dim3((unsigned)D), block, 0, s, st, D, bins, margin, (const double*)part, per_dim);
    }
    hipLaunchKernelGGL(k_hist_count<X>, grid, block, sizeof(unsigned int) * (size_t)(bins + 2), s, st, x, c, D, N, bins,
                       shape.rows_per_block, part);
    hipLaunchKernelGGL(k_hist_merge_extremes, dim3((unsigned)D), block, 0, s, st, D, bins, (const double*)part, per_dim);
}

}  // namespace

extern "C" {

int pbbi_hist_state_len(int D, int bins, int64_t* words_out) {
    if (const int rc = hist_check_shape(D, bins)) return rc;
    if (!words_out) return pbbi_fail(PBBI_ERR_INVALID, "words_out is NULL");
    *words_out = HistLayout(D, bins).len;
    return PBBI_OK;
}

int pbbi_hist_set_range(void* state, int D, int bins, const double* lo, const double* hi, int device, void* stream) {
    if (const int rc = hist_check_range(state, D, bins, lo, hi)) return rc;
    DeviceGuard guard(device);
    hipStream_t st = (hipStream_t)stream;
    const HistLayout lay(D, bins);
    std::vector<double> header((size_t)lay.counts);
    hist_pack_header(D, bins, lo, hi, header.data());
    PBBI_HIP(hipMemcpyAsync(state, header.data(), sizeof(double) * header.size(), hipMemcpyHostToDevice, st));
    PBBI_HIP(hipMemsetAsync((double*)state + lay.counts, 0, sizeof(double) * (size_t)(lay.len - lay.counts), st));
    PBBI_HIP(hipStreamSynchronize(st));  // the header leaves a host buffer of this call
    return PBBI_OK;
}

int pbbi_hist_accumulate(void* state, int D, int64_t N, int bins, int64_t S_before, const void* slabs_sdn, int c, int dtype,
                         int auto_range, double margin, int device, void* stream) {
    if (const int rc = hist_check_accumulate(state, D, N, bins, S_before, slabs_sdn, c, dtype, auto_range, margin)) return rc;
    HistShape shape;
    if (const int rc = hist_launch_shape(D, N, c, &shape)) return rc;
    DeviceGuard guard(device);
    hipStream_t st = (hipStream_t)stream;
    double* part = nullptr;  // one {min, max} pair per workgroup
    PBBI_HIP(hipMallocAsync((void**)&part, sizeof(double) * 2 * (size_t)D * (size_t)shape.per_dim(), st));
    if (dtype == PBBI_F64)
        launch_chunk<double>((double*)state, (const double*)slabs_sdn, c, D, N, bins, auto_range != 0, margin, shape, part, st);
    else
        launch_chunk<float>((double*)state, (const float*)slabs_sdn, c, D, N, bins, auto_range != 0, margin, shape, part, st);
    PBBI_HIP(hipGetLastError());
    PBBI_HIP(hipFreeAsync(part, st));
    return PBBI_OK;
}

}  // extern "C"
