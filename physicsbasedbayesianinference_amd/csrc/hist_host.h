// hist_host.h -- the host side of the running histogram sink that calls no HIP function (hist_host.cpp): the layout of the
// device state, the argument rules of the pbbi_hist_* entries, the header an explicit range uploads and the launch shape with
// its counter-wrap bound.  Plain C++: no HIP header here (kernels_hist.hip holds the kernels and the launches).
#pragma once
#include <stdint.h>

#include <string>

#include "pbbi.h"

int pbbi_fail(int code, const std::string& msg);  // pbbi_api.hip

// The state: D * (bins + 8) words of 8 bytes.  Six header arrays of D words each, then the counts, (bins + 2) per dimension:
//     lo | hi | inv = bins / (hi - lo) | min | max          doubles
//     nan                                                   unsigned 64-bit
//     counts[d][0 .. bins + 1]                              unsigned 64-bit; bin 0 = below lo, bin bins + 1 = at or above hi
struct HistLayout {  // (constexpr: the kernels build it too)
    int64_t lo, hi, inv, min, max, nan, counts, stride, len;
    constexpr HistLayout(int D, int bins)
        : lo(0), hi(D), inv(2 * (int64_t)D), min(3 * (int64_t)D), max(4 * (int64_t)D), nan(5 * (int64_t)D),
          counts(6 * (int64_t)D), stride((int64_t)bins + 2), len((int64_t)D * ((int64_t)bins + 8)) {}
};
enum { HIST_HEADER_ARRAYS = 6 };

// The slice of one workgroup: one dimension, HIST_COLS chains of rows_per_block draws.  A workgroup counts in 32-bit LDS
// counters, so the values it can see are bounded: rows_per_block <= HIST_MAX_ROWS and
//     HIST_MAX_ROWS * HIST_COLS = 2^18 * 2^13 = 2^31 < 2^32:  no counter can wrap, whatever c and N are.
enum { HIST_COLS = 8192, HIST_MAX_ROWS = 1 << 18, HIST_TARGET_BLOCKS = 2048 };
struct HistShape {
    int64_t col_chunks;  // grid.x: slices of HIST_COLS chains
    int rows_per_block;  // draws of the chunk per workgroup
    int row_chunks;      // grid.y
    int64_t per_dim() const { return col_chunks * row_chunks; }  // workgroups (and min / max partials) per dimension
};

int hist_check_shape(int D, int bins);  // D in [1, 65535], bins in [PBBI_HIST_MIN_BINS, PBBI_HIST_MAX_BINS]
// every rule of pbbi_hist_set_range: shape, pointers, lo_d < hi_d, both finite and hi_d - lo_d finite
int hist_check_range(const void* state, int D, int bins, const double* lo, const double* hi);
// the header an explicit range uploads: HIST_HEADER_ARRAYS * D words (lo | hi | inv | min = +inf | max = -inf | nan = 0)
void hist_pack_header(int D, int bins, const double* lo, const double* hi, double* out);
// every rule of pbbi_hist_accumulate
int hist_check_accumulate(const void* state, int D, int64_t N, int bins, int64_t S_before, const void* slabs, int c, int dtype,
                          int auto_range, double margin);
// the grid for a chunk: about HIST_TARGET_BLOCKS workgroups where the chunk has the work, rows_per_block <= HIST_MAX_ROWS
int hist_launch_shape(int D, int64_t N, int c, HistShape* out);
