// pbbi_internal.h -- shared between the translation units of libpbbi.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "glm_host.h"
#include "pbbi.h"

enum { KIND_HARMONIC = 0, KIND_GAUSS_DIAG = 1, KIND_GAUSS_DENSE = 2, KIND_ROSENBROCK = 3, KIND_CUSTOM = 4, KIND_GLM = 5 };

// layout version of the structs a user-potential plugin (pbbi_custom.h) shares with libpbbi.so
#define PBBI_PLUGIN_ABI 5  /* 4: plugins honour IterArgs::fuse_* (several iterations of a run per call); 5: they serve the
                              diagonal metric of the handle (d_glm_metric) and export pbbi_plugin_hmc_route */

struct IterArgs;
struct IntegrateArgs;
struct EvalArgs;

struct pbbi_potential {
    int kind;
    int D;
    int dtype;
    int device;
    double cst, a, b, s;
    void* d_mean;  // D elements (dtype) or nullptr
    void* d_prec;  // D elements (harmonic / diag) or D*D row-major (dense)
    // dense Gaussian, register-resident MFMA path (D <= 128):
    int DP;        // D padded to a multiple of 16 (0 = path not available)
    void* d_frag;  // DP*DP elements: precision in MFMA A-fragment order
    void* d_mean_pad;  // DP elements, zero padded
    bool zero_mean;    // every mean entry is exactly 0 (x = q, no subtraction needed)
    // dense Gaussian, streaming GEMM path (D > 128, or fp32): kernels_big.hip
    int DPAD_big;      // D padded to a multiple of 128 (0 = path not built)
    void* d_big_PT;    // DPAD x DPAD, P transposed ([k][i]), zero padded, handle dtype
    void* d_big_mu;    // DPAD, zero padded
    // user-defined potential (KIND_CUSTOM): kernels live in a plugin .so built by custom.py
    void* plugin;      // dlopen handle
    void* d_params;    // n_params elements (dtype) handed to the user's functions, or nullptr
    int n_params;
    int (*plugin_hmc_iter)(const IterArgs*);
    int (*plugin_integrate)(const IntegrateArgs*);
    int (*plugin_eval)(const EvalArgs*, int mode);
    // dense Gaussian, the same kernel with P streamed through the LDS (128 < D <= 256, fp64): kernels_dstream.hip
    int DPS;           // D padded to 192 or 256 (0 = path not available)
    void* d_sfrag;     // DPS*DPS elements: precision in the order the stream consumes it
    void* d_smean;     // DPS elements, zero padded
    // generalised linear model (KIND_GLM), kernels_glm.hip.  (Appended: plugins built against the fields above keep working.)
    int glm_DP;        // D padded to 16, 32, 64 or 128 (0 = not a built GLM handle)
    int glm_family;    // PBBI_GLM_*
    int64_t glm_M;     // observations
    double glm_lam;    // prior precision
    void* d_glm_img;   // X in MFMA A-fragment order, blocks of 16 observations (glm_pack)
    void* d_glm_y;     // y, zero padded to the blocks of the image
    // the full model (pbbi_potential_create_glm_ex); all zero / NULL on a handle of pbbi_potential_create_glm.  (Appended.)
    void* d_glm_obs;   // c = a n | d = a y | o, each zero padded to the blocks of the image (glm_pack_obs)
    void* d_glm_prior; // lam (glm_DP) | mu (glm_DP), zeros past D
    int glm_terms;     // GLM_TERM_*: what pbbi_describe_run names
    // softmax regression (pbbi_potential_create_glm_softmax), kernels_glm_softmax.hip.  (Appended.)  D = glm_K * (coefficients
    // per class), glm_DP = the padded class size Dc, d_glm_y the labels, d_glm_prior lam (Dc values, zeros past D)
    int glm_K;         // classes
    // the dispersion families (pbbi_potential_create_glm_dispersion), FAM = 3, 4, 5 of k_glm<NT, FAM, true>.  (Appended.)  D =
    // the state dimension (coefficients + the theta row when sampled), d_glm_obs = a | y | o, d_glm_prior covers the theta row
    int glm_trow;      // the state row of theta (= the coefficient count) when it is sampled, -1 when it is held
    double glm_theta;  // the held log-dispersion
    // the hierarchical prior (pbbi_potential_create_glm_hier), k_glm<NT, FAM, true, GLM_HIER_CENTRED>.  (Appended.)  D = coefficients +
    // glm_hier_J, the t rows last; d_glm_prior is the table of glm_pack_prior_groups
    int glm_hier_J;        // groups
    double glm_hier_n[4];  // members of each group
    // ... in the non-centred parametrisation (pbbi_potential_create_glm_hier_ex), k_glm<NT, FAM, true, GLM_HIER_NC>.  (Appended.)
    int glm_hier_nc;       // 1: the grouped rows of the state hold z_d, w_d = mu_d + exp(t_j) z_d
    // ... with structured group priors (pbbi_potential_create_glm_hier_q), k_glm<NT, FAM, true, GLM_HIER_Q>.  (Appended.)
    void* d_glm_qimg;      // the (glm_DP x glm_DP) penalty in A-fragment order (glm_pack_penalty)
    double glm_hier_rank[4];  // rank(Q_j), what the table's n_j slots hold on such a handle
    // random effects for the dispersion families (pbbi_potential_create_glm_hier_dispersion) add no field: glm_family 3 / 4 with
    // glm_hier_J > 0, D = coefficients + glm_hier_J + (glm_trow >= 0), glm_trow the LAST row, d_glm_prior the table of
    // glm_pack_prior_groups_disp, d_glm_obs = a | y | o
    // which of these kinds of handle this is.  (Appended.)  The one record of it: no other field is asked for the kind.
    int glm_variant;       // GlmVariant (glm_host.h), set by the builder of the create entry
    // the diagonal metric (pbbi_potential_set_metric_diag).  (Appended.)  NULL / NULL on a handle without one, which launches the
    // kernels it always has.  GLM and user-defined (KIND_CUSTOM) handles carry one, in these same two fields
    void* d_glm_metric;       // {m_d, 1 / m_d} per row in the kernel's row order (glm_pack_metric; softmax: the internal rows);
                              // KIND_CUSTOM: D + 8 pairs in the handle's dtype, ones past row D (the plugin kernels, pbbi_custom.h)
    double* glm_metric_diag;  // the D entries as given, on the host (pbbi_potential_get_metric_diag)
    // KIND_CUSTOM: which of the plugin's kernels serves an HMC call on the handle as it is now (pbbi_describe_run).  (Appended.)
    int (*plugin_hmc_route)(const pbbi_potential*, int method, int flags, int unit_mass);
    // the likelihood power (pbbi_potential_set_likelihood_power, kernels_glm_loglik.hip).  (Appended.)  NULL on a handle that was
    // never tempered, which then runs the bits it always has
    void* d_glm_obs0;   // d_glm_obs as built (power 1); d_glm_obs itself then holds c = beta c0 (| d = beta d0)
    double glm_power;   // the power as set from the host; NaN when it was read from the device
    // the dense metric (pbbi_potential_set_metric_dense).  (Appended.)  NULL / NULL on a handle without one; a handle carries at
    // most one metric, so these two and the two of the diagonal metric above are never set together
    void* d_glm_metric_dense;   // C = M^-1 | L | M, three (glm_DP x glm_DP) images in A-fragment order (glm_pack_metric_dense)
    double* glm_metric_dense;   // the D x D entries as given, on the host (pbbi_potential_get_metric_dense)
};

// ---- error plumbing ---------------------------------------------------------
void pbbi_set_error(const std::string& msg);
int pbbi_fail(int code, const std::string& msg);

#define PBBI_HIP(expr)                                                                          \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess)                                                                   \
            return pbbi_fail(PBBI_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

struct DeviceGuard {  // make the handle's device current for the duration of a call
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) { ok = false; return; }
        if (prev != dev && hipSetDevice(dev) != hipSuccess) ok = false;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// PBBI_BETA_ACCEPT: factor on (oldH - newH) in the accept test.  1.0 (exact: the product then has the
// bits of the difference) reproduces src/HMC.py:115; 1/kT is the test that matches the momentum draw
// of src/ensemble.py:88.
__host__ __device__ inline double pbbi_accept_beta(int flags, double kT) {
    return (flags & PBBI_BETA_ACCEPT) ? 1.0 / kT : 1.0;
}

int pbbi_num_cus(int device);  // compute units of a device (cached), pbbi_api.hip
// ---- launch descriptors passed between api and kernel TUs ---------------------
struct IterArgs {
    const pbbi_potential* pot;
    int method;
    const void* q_in;
    const void* p_in;  // nullptr in RNG mode
    const void* u_in;  // nullptr in RNG mode
    const void* mass;
    void* q_out;
    void* p_out;
    void* ratio_out;
    uint8_t* reject_out;
    int64_t N, ldn_in, ldn_out;
    double h;
    int L;
    int flags;
    // RNG mode
    int rng;
    uint64_t seed, iter, chain0;
    double kT;
    hipStream_t stream;
    // scratch arena lent by pbbi_hmc_run (all its iterations run on one stream, one after the other):
    // paths that need device scratch carve it from here instead of allocating every iteration, and
    // report the bytes they asked for through scratch_used (how the first iteration sizes the arena)
    void* scratch;
    size_t scratch_bytes;
    size_t* scratch_used;
    // Fused run (pbbi_hmc_run on a path that keeps the chain on chip across iterations, see
    // pbbi_fused_iterations): fuse_S > 1 makes this ONE call cover draw indices iter .. iter+fuse_S-1.
    // Iteration k of the call writes position slab fuse_slab0 + k of fuse_q_base (D*N elements each,
    // stride N; modulo 2 when fuse_wrap2: a burn-in's two scratch slabs), p_out + k*D*N,
    // ratio_out + k*N, reject_out + k*N; q_in / ldn_in feed iteration 0 only.
    int fuse_S;
    int fuse_wrap2;
    int64_t fuse_slab0;
    void* fuse_q_base;
    // per-chain trajectory lengths (PBBI_PER_CHAIN_STEPS / PBBI_UTURN_STOP, pbbi_hmc_*_dyn)
    const int32_t* steps_in;  // uploaded mode; nullptr = L
    int32_t* steps_out;       // optional
    // gradient carried across the iterations of a run (dense MFMA kernel, kernels_dense.hip CARRY):
    // carry = 1 first iteration (forms and stores g(q_0)), 2 later ones; carry_g = [2][D][N] doubles,
    // carry_sel = [N] bytes, zeroed before iteration 0
    int carry;
    void* carry_g;
    uint8_t* carry_sel;
    // routing decisions a run takes ONCE for all its iterations (pbbi_hmc_run): PBBI_ROUTE_* bits
    int route_hint;
};
#define PBBI_ROUTE_NO_DENSE_STREAM 1  /* 128 < D <= 256 dense Gaussian: stay on the GEMM path (kernels_big.hip) */
inline bool pbbi_dyn(const IterArgs& a) { return (a.flags & (PBBI_PER_CHAIN_STEPS | PBBI_UTURN_STOP)) != 0; }

struct IntegrateArgs {
    const pbbi_potential* pot;
    int method;
    void* q;
    void* p;
    const void* mass;
    void* v_out;
    int64_t N, ldn;
    double h;
    int L;
    hipStream_t stream;
};

struct EvalArgs {
    const pbbi_potential* pot;
    const void* q;
    const void* p;     // energy only
    const void* mass;  // energy only
    int64_t N, ldn;
    void* U_out;     // potential (eval) or H (energy)
    void* grad_out;  // eval only
    void* w_out;     // energy only: exp(-H)
    int ratio_finish;  // energy only: U_out[n] = exp(U_out[n] - H)   (src/HMC.py:115)
    hipStream_t stream;
};

// Device scratch for one call: from the arena an IterArgs lends, else stream-ordered allocations.
#include <vector>
struct Scratch {
    hipStream_t st;
    char* base = nullptr;
    size_t cap = 0, off = 0, total = 0;
    size_t* used = nullptr;
    std::vector<void*> owned;
    explicit Scratch(hipStream_t s) : st(s) {}
    explicit Scratch(const IterArgs& a)
        : st(a.stream), base((char*)a.scratch), cap(a.scratch ? a.scratch_bytes : 0), used(a.scratch_used) {}
    void* get(size_t bytes) {
        bytes = ((bytes ? bytes : 16) + 255) / 256 * 256;
        total += bytes;
        if (base && off + bytes <= cap) {
            void* p = base + off;
            off += bytes;
            return p;
        }
        void* p = nullptr;
        if (hipMallocAsync(&p, bytes, st) != hipSuccess) return nullptr;
        owned.push_back(p);
        return p;
    }
    ~Scratch() {
        for (void* p : owned) (void)hipFreeAsync(p, st);
        if (used) *used = total;
    }
};

// chain-per-lane kernels (harmonic / diagonal Gaussian / Rosenbrock), kernels_lane.hip
int lane_hmc_iter(const IterArgs& a);
int lane_integrate(const IntegrateArgs& a);
int lane_eval(const EvalArgs& a);
int lane_energy(const EvalArgs& a);
// Rosenbrock 16 < D <= 32, Leapfrog: two lanes per chain (config C3), kernels_lane2.hip
bool lane2_applies(const IterArgs& a);
int lane2_hmc_iter(const IterArgs& a);
// how many consecutive iterations of pbbi_hmc_run one call of route_hmc may cover for these arguments
// (1 = the path has no fused form); lane_fused_iterations: kernels_lane.hip
int lane_fused_iterations(const IterArgs& a);
const char* lane_route_name(const IterArgs& a);  // the kernel family lane_hmc_iter picks (pbbi_describe_run)
// per-chain trajectory lengths (k_lane_dyn_hmc: elementwise potentials, fp64, D <= 32, Leapfrog)
int lane_dyn_hmc_iter(const IterArgs& a);
// one GIST iteration fused into one launch (k_lane_gist_hmc; pbbi_hmc_run_gist): elementwise potentials, fp64, D <= 32
bool lane_gist_applies(const pbbi_potential* pot);
int lane_gist_iter(const IterArgs& a);
// harmonic / diagonal Gaussian, 16 < D <= 256, PBBI_KDK_FMA: 16-dim parts in the waves of a workgroup, kernels_sepn.hip
bool sepn_applies(const IterArgs& a);
int sepn_hmc_iter(const IterArgs& a);
// ... and in the reference's operation order (bit-exact), PBBI_KDK_FMA not set
bool sepx_applies(const IterArgs& a);
int sepx_hmc_iter(const IterArgs& a);
// Rosenbrock, 32 < D <= 256, PBBI_KDK_FMA, same layout with boundary exchange through LDS, kernels_rosn.hip
bool rosn_applies(const IterArgs& a);
int rosn_hmc_iter(const IterArgs& a);
// Rosenbrock, 32 < D <= 64 (128), PBBI_KDK_FMA: 4 (8) lanes of one wave per chain, kernels_rosg.hip
bool rosg_applies(const IterArgs& a);
int rosg_hmc_iter(const IterArgs& a);
// ... and in the reference's operation order (bit-exact), 32 < D <= 128, PBBI_KDK_FMA not set
bool rosgx_applies(const IterArgs& a);
int rosgx_hmc_iter(const IterArgs& a);
// the same potentials for D > 64 and for fp32: chain state in a device workspace, kernels_stream.hip
int stream_hmc_iter(const IterArgs& a);
int stream_integrate(const IntegrateArgs& a);
int stream_eval(const EvalArgs& a);
int stream_energy(const EvalArgs& a);
// dense-precision Gaussian, MFMA register-resident (D <= 128), kernels_dense.hip
#define PBBI_CARRY_MAX_BYTES (((uint64_t)1 << 32) - ((uint64_t)1 << 20))  /* carried dense slabs: 2 * DP * N * 8 below this */
int dense_hmc_iter(const IterArgs& a);
bool dense_carry_applies(const IterArgs& a);  // may a run on these arguments carry the gradient?
int dense_fused_iterations(const IterArgs& a);
bool big_carry_applies(const IterArgs& a);     // the same for the GEMM path (kernels_big.hip)
void big_carry_bytes(const pbbi_potential* pot, int64_t N, size_t* g_bytes, size_t* sel_bytes);  // iterations one launch may cover (carried runs)
int dense_integrate(const IntegrateArgs& a);
int dense_eval(const EvalArgs& a);
int dense_energy(const EvalArgs& a);
int dense_build_fragments(pbbi_potential* pot, const double* precision_host, const double* mean_host);
// dense-precision Gaussian, 128 < D <= 256, fp64: the register-resident kernel with P streamed, kernels_dstream.hip
int dense_stream_build(pbbi_potential* pot, const double* precision_host, const double* mean_host);
bool dense_stream_applies(const IterArgs& a);
bool dense_stream_carry_applies(const IterArgs& a);
int dense_stream_fused_iterations(const IterArgs& a);
int dense_stream_hmc_iter(const IterArgs& a);
bool dense_stream_integrate_applies(const IntegrateArgs& a);
int dense_stream_integrate(const IntegrateArgs& a);
// dense-precision Gaussian, streaming MFMA GEMM per step (D > 128, fp64 / fp32), kernels_big.hip
int big_hmc_iter(const IterArgs& a);
int big_integrate(const IntegrateArgs& a);
int big_eval(const EvalArgs& a);
int big_energy(const EvalArgs& a);
int big_build(pbbi_potential* pot, const double* precision_host, const double* mean_host);
// generalised linear models, likelihood on the fp64 matrix cores (fp64, D <= 128), kernels_glm.hip; what of their host side
// calls no HIP function (shipped shapes, argument rules, packers) is glm_host.h, the builders are pbbi_api.hip's
int glm_hmc_iter(const IterArgs& a);
int glm_integrate(const IntegrateArgs& a);
int glm_eval(const EvalArgs& a);
int glm_energy(const EvalArgs& a);
// K-class softmax regression on the same frame (fp64, K * Dc <= 128), kernels_glm_softmax.hip
int glm_softmax_hmc_iter(const IterArgs& a);
int glm_softmax_integrate(const IntegrateArgs& a);
int glm_softmax_eval(const EvalArgs& a);
int glm_softmax_energy(const EvalArgs& a);
