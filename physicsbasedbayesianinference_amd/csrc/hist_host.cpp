// hist_host.cpp -- the host side of the running histogram sink that calls no HIP function (hist_host.h): argument rules, the
// explicit range's header, the launch shape.  Everything here runs before any launch and on a machine without a GPU.
#include "hist_host.h"

#include <cmath>
#include <limits>

int hist_check_shape(int D, int bins) {
    if (D < 1) return pbbi_fail(PBBI_ERR_INVALID, "D must be >= 1");
    if (D > 65535) return pbbi_fail(PBBI_ERR_INVALID, "D must be <= 65535");
    if (bins < PBBI_HIST_MIN_BINS || bins > PBBI_HIST_MAX_BINS)
        return pbbi_fail(PBBI_ERR_INVALID, "bins must be in [PBBI_HIST_MIN_BINS, PBBI_HIST_MAX_BINS]");
    return PBBI_OK;
}

int hist_check_range(const void* state, int D, int bins, const double* lo, const double* hi) {
    if (const int rc = hist_check_shape(D, bins)) return rc;
    if (!state) return pbbi_fail(PBBI_ERR_INVALID, "state is NULL");
    if (!lo || !hi) return pbbi_fail(PBBI_ERR_INVALID, "lo or hi is NULL");
    for (int d = 0; d < D; ++d) {
        if (!std::isfinite(lo[d]) || !std::isfinite(hi[d]))
            return pbbi_fail(PBBI_ERR_INVALID, "lo and hi must be finite (dimension " + std::to_string(d) + ")");
        if (!(lo[d] < hi[d])) return pbbi_fail(PBBI_ERR_INVALID, "lo must be < hi (dimension " + std::to_string(d) + ")");
        if (!std::isfinite(hi[d] - lo[d]))
            return pbbi_fail(PBBI_ERR_INVALID, "hi - lo must be finite (dimension " + std::to_string(d) + ")");
    }
    return PBBI_OK;
}

void hist_pack_header(int D, int bins, const double* lo, const double* hi, double* out) {
    const HistLayout lay(D, bins);
    const double inf = std::numeric_limits<double>::infinity();
    for (int d = 0; d < D; ++d) {
        out[lay.lo + d] = lo[d];
        out[lay.hi + d] = hi[d];
        out[lay.inv + d] = (double)bins / (hi[d] - lo[d]);
        out[lay.min + d] = inf;
        out[lay.max + d] = -inf;
        out[lay.nan + d] = 0.0;  // the all-zero word: an unsigned 64-bit 0
    }
}

int hist_check_accumulate(const void* state, int D, int64_t N, int bins, int64_t S_before, const void* slabs, int c, int dtype,
                          int auto_range, double margin) {
    if (const int rc = hist_check_shape(D, bins)) return rc;
    if (N < 1) return pbbi_fail(PBBI_ERR_INVALID, "N must be >= 1");
    if (c < 1) return pbbi_fail(PBBI_ERR_INVALID, "c must be >= 1");
    if (S_before < 0) return pbbi_fail(PBBI_ERR_INVALID, "S_before must be >= 0");
    if (!state) return pbbi_fail(PBBI_ERR_INVALID, "state is NULL");
    if (!slabs) return pbbi_fail(PBBI_ERR_INVALID, "slabs is NULL");
    if (dtype != PBBI_F64 && dtype != PBBI_F32) return pbbi_fail(PBBI_ERR_INVALID, "unknown dtype");
    if (auto_range != 0 && auto_range != 1) return pbbi_fail(PBBI_ERR_INVALID, "auto_range must be 0 or 1");
    if (auto_range) {
        if (S_before > 0) return pbbi_fail(PBBI_ERR_INVALID, "auto_range starts a state: S_before must be 0");
        if (!(margin >= 0.0) || !std::isfinite(margin)) return pbbi_fail(PBBI_ERR_INVALID, "margin must be finite and >= 0");
    }
    HistShape shape;
    return hist_launch_shape(D, N, c, &shape);
}

int hist_launch_shape(int D, int64_t N, int c, HistShape* out) {
    const int64_t col_chunks = (N + HIST_COLS - 1) / HIST_COLS;
    if (col_chunks > 0x7fffffff) return pbbi_fail(PBBI_ERR_INVALID, "N is beyond the launch grid");
    const int64_t per_row = (int64_t)D * col_chunks;  // workgroups when each takes every draw of its columns
    int64_t row_chunks = (HIST_TARGET_BLOCKS + per_row - 1) / per_row;
    if (row_chunks > c) row_chunks = c;
    int64_t rows = (c + row_chunks - 1) / row_chunks;
    if (rows > HIST_MAX_ROWS) rows = HIST_MAX_ROWS;  // the counter-wrap bound (hist_host.h)
    out->col_chunks = col_chunks;
    out->rows_per_block = (int)rows;
    out->row_chunks = (int)((c + rows - 1) / rows);  // <= max(HIST_TARGET_BLOCKS, 2^31 / HIST_MAX_ROWS) = 8192
    return PBBI_OK;
}
