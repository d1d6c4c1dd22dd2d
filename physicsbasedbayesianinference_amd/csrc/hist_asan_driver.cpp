// hist_asan_driver.cpp -- hist_host.cpp under AddressSanitizer + UndefinedBehaviorSanitizer (test infrastructure, CPU only).
// The header packer writes into a buffer the caller sized and the range check reads two the caller sized: they are driven here
// over heap buffers of EXACTLY the documented length at D = 1, 3, 17, 128 and bins = 16, 100, 4096.  Every rejection of the
// argument rules is asked for once, and the launch shape is held to its promises over a sweep of (D, N, c) up to the largest
// values the entries accept: the counter-wrap bound rows_per_block * HIST_COLS <= 2^31, a grid within the launch limits, and
// slices that cover the chunk.  Built together with hist_host.cpp by `make hist_asan_check` (a prerequisite of `make
// asan_check`); prints "hist asan ok" and exits 0 when the sanitizers stayed silent and every call returned what its arguments
// deserve.  tests/test_running_hist_host.py runs it.
#include <cmath>
#include <cstdio>
#include <limits>
#include <memory>

#include "hist_host.h"

static std::string g_error;
int pbbi_fail(int code, const std::string& msg) {
    g_error = msg;
    return code;
}

static int bad = 0;
#define EXPECT(cond)                                                                  \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::printf("line %d: %s failed (%s)\n", __LINE__, #cond, g_error.c_str()); \
            ++bad;                                                                    \
        }                                                                             \
    } while (0)

static void layout_and_header() {
    for (int D : {1, 3, 17, 128})
        for (int bins : {16, 100, 4096}) {
            const HistLayout lay(D, bins);
            EXPECT(lay.len == (int64_t)D * (bins + 8) && lay.counts == (int64_t)HIST_HEADER_ARRAYS * D);
            EXPECT(lay.counts + D * lay.stride == lay.len);
            std::unique_ptr<double[]> lo(new double[D]), hi(new double[D]), out(new double[(size_t)lay.counts]);
            for (int d = 0; d < D; ++d) {
                lo[d] = -1.0 - d;
                hi[d] = 2.0 + 0.5 * d;
            }
            int dummy = 0;
            EXPECT(hist_check_range(&dummy, D, bins, lo.get(), hi.get()) == PBBI_OK);
            hist_pack_header(D, bins, lo.get(), hi.get(), out.get());
            for (int d = 0; d < D; ++d) {
                EXPECT(out[lay.lo + d] == lo[d] && out[lay.hi + d] == hi[d]);
                EXPECT(out[lay.inv + d] == (double)bins / (hi[d] - lo[d]));
                EXPECT(out[lay.min + d] == INFINITY && out[lay.max + d] == -INFINITY && out[lay.nan + d] == 0.0);
            }
            // one bad entry, in the last place
            const double keep = hi[D - 1];
            for (double v : {lo[D - 1], lo[D - 1] - 1.0, (double)INFINITY, (double)NAN, std::numeric_limits<double>::max()}) {
                hi[D - 1] = v;
                if (v == std::numeric_limits<double>::max()) lo[D - 1] = -v;  // finite bounds, an infinite difference
                EXPECT(hist_check_range(&dummy, D, bins, lo.get(), hi.get()) == PBBI_ERR_INVALID);
            }
            hi[D - 1] = keep;
            lo[D - 1] = -INFINITY;
            EXPECT(hist_check_range(&dummy, D, bins, lo.get(), hi.get()) == PBBI_ERR_INVALID);
            EXPECT(hist_check_range(nullptr, D, bins, lo.get(), hi.get()) == PBBI_ERR_INVALID);
            EXPECT(hist_check_range(&dummy, D, bins, nullptr, hi.get()) == PBBI_ERR_INVALID);
            EXPECT(hist_check_range(&dummy, D, bins, lo.get(), nullptr) == PBBI_ERR_INVALID);
        }
    for (int bins : {15, 4097, 0, -1}) EXPECT(hist_check_shape(3, bins) == PBBI_ERR_INVALID);
    for (int D : {0, -1, 65536}) EXPECT(hist_check_shape(D, 64) == PBBI_ERR_INVALID);
    EXPECT(hist_check_shape(65535, 4096) == PBBI_OK);
}

static void accumulate_rules() {
    int s = 0;
    const void* p = &s;
    EXPECT(hist_check_accumulate(p, 3, 5, 16, 0, p, 2, PBBI_F64, 0, 1.0) == PBBI_OK);
    EXPECT(hist_check_accumulate(p, 3, 5, 16, 7, p, 2, PBBI_F32, 0, -1.0) == PBBI_OK);  // margin is not read without auto_range
    EXPECT(hist_check_accumulate(p, 3, 5, 16, 0, p, 2, PBBI_F64, 1, 0.0) == PBBI_OK);
    EXPECT(hist_check_accumulate(p, 0, 5, 16, 0, p, 2, PBBI_F64, 0, 1.0) == PBBI_ERR_INVALID);
    EXPECT(hist_check_accumulate(p, 3, 0, 16, 0, p, 2, PBBI_F64, 0, 1.0) == PBBI_ERR_INVALID);
    EXPECT(hist_check_accumulate(p, 3, 5, 15, 0, p, 2, PBBI_F64, 0, 1.0) == PBBI_ERR_INVALID);
    EXPECT(hist_check_accumulate(p, 3, 5, 4097, 0, p, 2, PBBI_F64, 0, 1.0) == PBBI_ERR_INVALID);
    EXPECT(hist_check_accumulate(p, 3, 5, 16, -1, p, 2, PBBI_F64, 0, 1.0) == PBBI_ERR_INVALID);
    EXPECT(hist_check_accumulate(p, 3, 5, 16, 0, p, 0, PBBI_F64, 0, 1.0) == PBBI_ERR_INVALID);
    EXPECT(hist_check_accumulate(nullptr, 3, 5, 16, 0, p, 2, PBBI_F64, 0, 1.0) == PBBI_ERR_INVALID);
    EXPECT(hist_check_accumulate(p, 3, 5, 16, 0, nullptr, 2, PBBI_F64, 0, 1.0) == PBBI_ERR_INVALID);
    EXPECT(hist_check_accumulate(p, 3, 5, 16, 0, p, 2, 7, 0, 1.0) == PBBI_ERR_INVALID);
    EXPECT(hist_check_accumulate(p, 3, 5, 16, 0, p, 2, PBBI_F64, 2, 1.0) == PBBI_ERR_INVALID);
    EXPECT(hist_check_accumulate(p, 3, 5, 16, 1, p, 2, PBBI_F64, 1, 1.0) == PBBI_ERR_INVALID);
    EXPECT(hist_check_accumulate(p, 3, 5, 16, 0, p, 2, PBBI_F64, 1, -0.5) == PBBI_ERR_INVALID);
    EXPECT(hist_check_accumulate(p, 3, 5, 16, 0, p, 2, PBBI_F64, 1, NAN) == PBBI_ERR_INVALID);
    EXPECT(hist_check_accumulate(p, 3, 5, 16, 0, p, 2, PBBI_F64, 1, INFINITY) == PBBI_ERR_INVALID);
    EXPECT(hist_check_accumulate(p, 3, ((int64_t)1 << 45), 16, 0, p, 2, PBBI_F64, 0, 1.0) == PBBI_ERR_INVALID);  // past the grid
}

static void launch_shapes() {
    const int64_t NS[] = {1, 5, 257, HIST_COLS - 1, HIST_COLS, HIST_COLS + 1, 65536, (int64_t)1 << 30, ((int64_t)1 << 43)};
    const int CS[] = {1, 2, 40, 50, 2047, 2048, 2049, HIST_MAX_ROWS, HIST_MAX_ROWS + 1, std::numeric_limits<int>::max()};
    for (int D : {1, 3, 128, 2048, 65535})
        for (int64_t N : NS)
            for (int c : CS) {
                HistShape g;
                EXPECT(hist_launch_shape(D, N, c, &g) == PBBI_OK);
                EXPECT(g.col_chunks >= 1 && g.col_chunks <= 0x7fffffff && g.col_chunks * HIST_COLS >= N &&
                       (g.col_chunks - 1) * HIST_COLS < N);
                EXPECT(g.rows_per_block >= 1 && g.rows_per_block <= HIST_MAX_ROWS);
                EXPECT((int64_t)g.rows_per_block * HIST_COLS <= ((int64_t)1 << 31));  // no 32-bit counter can wrap
                EXPECT(g.row_chunks >= 1 && g.row_chunks <= 65535);
                EXPECT((int64_t)g.row_chunks * g.rows_per_block >= c && (int64_t)(g.row_chunks - 1) * g.rows_per_block < c);
                EXPECT(g.per_dim() == g.col_chunks * g.row_chunks);
            }
    HistShape g;
    EXPECT(hist_launch_shape(128, 65536, 50, &g) == PBBI_OK && g.col_chunks == 8 && g.row_chunks == 2 && g.rows_per_block == 25);
}

int main() {
    layout_and_header();
    accumulate_rules();
    launch_shapes();
    if (bad) {
        std::printf("%d checks failed\n", bad);
        return 1;
    }
    std::printf("hist asan ok\n");
    return 0;
}
