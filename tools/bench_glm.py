"""GLM potentials (csrc/kernels_glm.hip) against the user-source plugin path on the same data, one GPU.

Bayesian logistic regression at two shapes, pbbi_hmc_run with in-kernel single-precision draws, L = 10, K
iterations per timed window.  GLM(X, y) and logistic_regression_posterior(X, y) are timed in ONE process,
alternating, five repeats each after warming both.  Writes both series, the ratio and the share of the
78.6 TFLOP/s fp64 MFMA peak (executed 4 M DP flop per chain-gradient, algorithmic 4 M D beside it) to
profiles/glm_bench.json.

--model rich benchmarks the full model (observation weights, offsets, binomial trials, a prior per coefficient:
the RICH instantiations of k_glm) against the plain model on the same X, alternating in one process; with
--custom also the full model as a CustomPotential (what its users had before).  That record goes to
profiles/glm_model_bench.json under the key given by --label.

--model softmax times SoftmaxGLM (csrc/kernels_glm_softmax.hip) against the same model as a CustomPotential, alternating
in one process, at (M = 256, D = 5, K = 3, N = 65 536), (M = 256, D = 16, K = 8, N = 65 536) and (M = 16 384, D = 16,
K = 8, N = 16 384), and writes profiles/glm_softmax_bench.json (executed 4 M K Dc flop per chain-gradient).  The plugin
at K D = 128 is two orders of magnitude slower, so each side has its own window length: SOFTMAX_SHAPES gives per shape
the iterations per pbbi_hmc_run call (the slabs of the sample buffer), the iterations per timed window of each side
(about a second of the softmax path), the repeats and the warm-up; --K / --repeats / --warmup override them.  All
figures are host-clock rates over whole windows of pbbi_hmc_run calls, not kernel times.

--model dispersion times DispersionGLM(family="negbinomial", dispersion="sample") (FAM = 4 of k_glm<NT, FAM, true>) against
the same model as a CustomPotential, alternating in one process, at (M = 256, D = 15, N = 65 536) and (M = 16 384, D = 63,
N = 16 384) -- state dimensions 16 and 64 -- and writes profiles/glm_dispersion_bench.json (executed 4 M DP flop per
chain-gradient).  Window lengths per side as for --model softmax (DISPERSION_SHAPES).

--model hier times HierarchicalGLM (k_glm<NT, FAM, true, GLM_HIER_CENTRED>: logistic, sampled group scales) against the same model as a
CustomPotential (how it ran before) and against a fixed-prior GLM of the same X and state dimension ([X | 0], the group
precisions held at their true values), all three alternating in one process with the same data, starts and step size, at
(M = 256, D = 14 + J = 2, N = 65 536) and (M = 16 384, D = 60 + J = 4, N = 16 384), and writes profiles/glm_hier_bench.json
with the accept rates of all sides.  Window lengths per side as for --model softmax (HIER_SHAPES).

--model hier --parametrisation noncentred times the non-centred HierarchicalGLM (k_glm<NT, FAM, true, GLM_HIER_NC>) against
the centred kernel on the same data (started at the same points in its own coordinates) and against the same non-centred
model as a CustomPotential, all three alternating in one process, at the two shapes above, and writes
profiles/glm_hier_nc_bench.json (HIER_NC_SHAPES: each parametrisation has the step size that suits its geometry; the cost
of a step does not depend on it).

--model hierq times HierarchicalGLM with structured group priors (k_glm<NT, FAM, true, GLM_HIER_Q>: logistic, an RW2 penalty on
every group) against HierarchicalGLM with the same groups and no penalty (the centred kernel it extends) and against the same
structured model as a CustomPotential, all three alternating in one process, at the two shapes of --model hier, and writes
profiles/glm_hier_penalty_bench.json: the project's criterion (the slowest repeat of the kernel beats the fastest of the plugin)
and the ratio to the centred kernel next to what the MFMA counts predict, 1 + (DP^2 / 64) / (M DP / 32) = 1 + DP / (2 M).

--model gamma times DispersionGLM's three families (gaussian, gamma, negbinomial; FAM = 3, 5, 4 of k_glm<NT, FAM, true>) beside
each other at the shapes of --model dispersion and writes profiles/glm_gamma_bench.json: what each family's link costs on the
same frame.

--model ordinal times OrdinalGLM (K = 5; FAM = 6 of k_glm<NT, FAM, true>) beside the full logistic model at the same padded state
dimension (16 and 64), alternating in one process at M, N and step sizes of --model dispersion, and writes
profiles/glm_ordinal_bench.json: what the ordinal link -- two exp per observation, the select chains, the K - 1 per-chain
reductions -- costs on the same kernel frame.  --model logistic times the logistic side alone (--out FILE); run on another build
of the library (the parent commit's) its file is what --model ordinal --baseline FILE merges into the record.

--model hierdisp times HierarchicalDispersionGLM(family="negbinomial", dispersion="sample") in both parametrisations (k_glm<NT,
4, true, GLM_HIER_CENTRED / GLM_HIER_NC>) against the centred model as a CustomPotential and against DispersionGLM of [X | 0]
with the group scales held at their true values -- the parent kernel at the same padded shape, so that ratio is the cost of
the prior -- all four alternating in one process, at (M = 256, D = 13, J = 2, N = 65 536) and (M = 16 384, D = 59, J = 4, N = 16
384): 16 and 64 rows with theta the last.  It writes profiles/glm_hier_dispersion_bench.json (HIER_DISP_SHAPES).

--model pointwise times pbbi_pointwise_glm (csrc/kernels_glm_pointwise.hip: lse, mean, variance of the pointwise
log-likelihood and the mean fitted mean of all M observations over S x N draws) on the plain logistic model against the
same four vectors from torch ops on the same device (chunked matmul, the link elementwise, logsumexp / mean / var over the
draws: pointwise_torch), alternating in one process, at the two shapes of SHAPES with --slabs 8 slabs of N draws.  It
writes profiles/glm_pointwise_bench.json.

--model loglik times pbbi_loglik_glm (csrc/kernels_glm_loglik.hip: the likelihood energy of each of the S x N draws, both
launches, ranges = 0) on the plain logistic model against the same vector from torch ops on the same device (chunked matmul, the
link elementwise, a sum over the observations: loglik_torch), alternating in one process, at the same two shapes and slabs.  It
writes profiles/glm_loglik_bench.json.

--model predictive times pbbi_predictive_glm (csrc/kernels_glm_predictive.hip: one Poisson replicate per draw and observation
and the seven per-draw statistics) against the same statistics from torch.poisson and torch ops over chunks of draws
(predictive_torch), alternating in one process after two warm-up calls, at the two shapes of SHAPES with --slabs 8 slabs of N
draws; and the kernel alone with the means scaled up, for the cost of the inversion's O(sigma) walk.  It writes
profiles/glm_predictive_bench.json.

usage: tools/bench_glm.py [--shape small|large|all] [--K 32] [--repeats 5] [--glm-only] [--out FILE]
       tools/bench_glm.py --model rich [--custom] [--label NAME] [--shape ...]
       tools/bench_glm.py --model softmax [--shape k3|k8|k8large|all]
       tools/bench_glm.py --model dispersion [--shape small|large|all]
       tools/bench_glm.py --model gamma [--shape small|large|all]
       tools/bench_glm.py --model ordinal [--shape small|large|all] [--baseline FILE]
       tools/bench_glm.py --model logistic [--shape small|large|all] [--build NAME] --out FILE
       tools/bench_glm.py --model hierq [--shape small|large|all]
       tools/bench_glm.py --model hierdisp [--shape small|large|all]
       tools/bench_glm.py --model pointwise [--shape small|large|all] [--slabs 8] [--repeats 5]
       tools/bench_glm.py --model loglik [--shape small|large|all] [--slabs 8] [--repeats 5]
       tools/bench_glm.py --model predictive [--shape small|large|all] [--slabs 8] [--repeats 5]
       tools/bench_glm.py --model hier [--parametrisation centred|noncentred] [--shape small|large|all]  (noncentred: also mid)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import physicsbasedbayesianinference_amd as P  # noqa: E402
from physicsbasedbayesianinference_amd import _lib, glm  # noqa: E402
from physicsbasedbayesianinference_amd.custom import logistic_regression_posterior  # noqa: E402

PEAK_F64_MFMA = 78.6e12
SHAPES = {"small": dict(M=256, D=16, N=65536, h=0.2), "large": dict(M=16384, D=64, N=16384, h=0.16)}


def problem(M, D, seed=0):
    rs = np.random.RandomState(seed)
    X = rs.standard_normal((M, D)) / np.sqrt(D)
    w = rs.standard_normal(D)
    y = (rs.uniform(size=M) < 1.0 / (1.0 + np.exp(-(X @ w)))).astype(np.float64)
    return X, y, w, rs


# the full model as user source: prm = [M, X, c, d, o, lam(D), mu(D)], c = a n, d = a y
RICH_LOGISTIC_SOURCE = """
template <class Q>
PBBI_FN T potential(const Q& q, int D, const T* prm) {
    const int M = (int)prm[0];
    const T *X = prm + 1, *c = X + (long)M * D, *d = c + M, *o = d + M, *lam = o + M, *mu = lam + D;
    T s = 0;
    for (int i = 0; i < M; ++i) {
        if (c[i] == 0 && d[i] == 0) continue;
        T z = o[i];
        for (int j = 0; j < D; ++j) z += X[i * D + j] * q[j];
        s += c[i] * ((z > 0 ? z : T(0)) + log1p(exp(-fabs(z)))) - d[i] * z;
    }
    T r = 0;
    for (int j = 0; j < D; ++j) r += lam[j] * (q[j] - mu[j]) * (q[j] - mu[j]);
    return s + T(0.5) * r;
}
template <class Q, class G>
PBBI_FN void gradient(const Q& q, G& g, int D, const T* prm) {
    const int M = (int)prm[0];
    const T *X = prm + 1, *c = X + (long)M * D, *d = c + M, *o = d + M, *lam = o + M, *mu = lam + D;
    for (int j = 0; j < D; ++j) g[j] = lam[j] * (q[j] - mu[j]);
    for (int i = 0; i < M; ++i) {
        if (c[i] == 0 && d[i] == 0) continue;
        T z = o[i];
        for (int j = 0; j < D; ++j) z += X[i * D + j] * q[j];
        const T w = c[i] / (T(1) + exp(-z)) - d[i];
        for (int j = 0; j < D; ++j) g[j] += w * X[i * D + j];
    }
}
"""


def rich_problem(M, D, seed=0):
    """problem()'s X with weights from {0, 0.5, 1, 3}, offsets ~ N(0, 0.3), trials in 1..20, a flat intercept and
    precisions from {0.5, 4} on the slopes around a prior mean ~ N(0, 0.5)."""
    X, _, w, rs = problem(M, D, seed)
    a = rs.choice([0.0, 0.5, 1.0, 3.0], size=M)
    o = 0.3 * rs.standard_normal(M)
    n = rs.randint(1, 21, size=M).astype(np.float64)
    y = rs.binomial(n.astype(int), 1.0 / (1.0 + np.exp(-(X @ w + o)))).astype(np.float64)
    lam = np.r_[0.0, rs.choice([0.5, 4.0], size=D - 1)]
    mu = 0.5 * rs.standard_normal(D)
    return dict(X=X, y=y, weights=a, offset=o, trials=n, prior_precision=lam, prior_mean=mu), w, rs


def bench_rich(name, M, D, N, h, L, K, repeats, warm, custom):
    """Plain and full model (and the full model through CustomPotential) alternating in one process.  The full
    model's posterior is ~sqrt(mean a n) narrower than the plain one's: its step size is scaled by that, so both
    run L steps per iteration at comparable accept rates (the cost per step does not depend on h)."""
    kw, w, rs = rich_problem(M, D)
    hr = h / np.sqrt(np.mean(kw["weights"] * kw["trials"]))
    q0 = np.ascontiguousarray(w[:, None] + 0.1 * rs.standard_normal((D, N)))
    yp = (kw["y"] > 0.5 * kw["trials"]).astype(np.float64)
    runners = {"plain": Runner(P.GLM(kw["X"], yp), D, N, q0, h, L, K), "rich": Runner(P.GLM(**kw), D, N, q0, hr, L, K)}
    if custom:
        from physicsbasedbayesianinference_amd.custom import CustomPotential
        prm = np.concatenate([[float(M)], kw["X"].ravel(), kw["weights"] * kw["trials"], kw["weights"] * kw["y"],
                              kw["offset"], kw["prior_precision"], kw["prior_mean"]])
        runners["custom"] = Runner(CustomPotential(D, RICH_LOGISTIC_SOURCE, prm), D, N, q0, hr, L, K)
    for r in runners.values():
        r.go(warm)
    torch.cuda.synchronize()
    series = {k: [] for k in runners}
    for i in range(repeats):
        for k, r in runners.items():   # alternating
            series[k].append(r.timed())
            print(f"# {name} repeat {i} {k}: {series[k][-1]:.4f} s", flush=True)
    out = dict(shape=name, M=M, D=D, DP=glm.padded_dim(D), chains=N, L=L, K=K, h=dict(plain=h, rich=hr),
               accept_rate={k: 1.0 - float(r.rej.float().mean().item()) for k, r in runners.items()})
    for k, ts in series.items():
        out[k + "_seconds"] = ts
        out[k + "_step_chain_per_s"] = [K * L * N / t for t in ts]
    med = {k: float(np.median(ts)) for k, ts in series.items()}
    out["rich_over_plain_time_median"] = med["rich"] / med["plain"]
    if custom:
        out["custom_over_rich_time_median"] = med["custom"] / med["rich"]
    return out


# K-class softmax regression as user source: prm = [M, K, X, y, lam(D)]; the state is the K coefficient vectors class-major
SOFTMAX_SOURCE = """
template <class Q>
PBBI_FN T potential(const Q& q, int DT, const T* prm) {
    const int M = (int)prm[0], K = (int)prm[1];
    const int D = DT / K;
    const T* X = prm + 2;
    const T* y = X + (long)M * D;
    const T* lam = y + M;
    T s = 0;
    for (int i = 0; i < M; ++i) {
        T z[16]; T m = 0;
        for (int k = 0; k < K; ++k) {
            T a = 0;
            for (int j = 0; j < D; ++j) a += X[i * D + j] * q[k * D + j];
            z[k] = a; if (k == 0 || a > m) m = a;
        }
        T Z = 0;
        for (int k = 0; k < K; ++k) Z += exp(z[k] - m);
        s += (m + log(Z)) - z[(int)y[i]];
    }
    T r = 0;
    for (int k = 0; k < K; ++k) for (int j = 0; j < D; ++j) r += lam[j] * q[k * D + j] * q[k * D + j];
    return s + T(0.5) * r;
}
template <class Q, class G>
PBBI_FN void gradient(const Q& q, G& g, int DT, const T* prm) {
    const int M = (int)prm[0], K = (int)prm[1];
    const int D = DT / K;
    const T* X = prm + 2;
    const T* y = X + (long)M * D;
    const T* lam = y + M;
    for (int k = 0; k < K; ++k) for (int j = 0; j < D; ++j) g[k * D + j] = lam[j] * q[k * D + j];
    for (int i = 0; i < M; ++i) {
        T z[16]; T m = 0;
        for (int k = 0; k < K; ++k) {
            T a = 0;
            for (int j = 0; j < D; ++j) a += X[i * D + j] * q[k * D + j];
            z[k] = a; if (k == 0 || a > m) m = a;
        }
        T Z = 0;
        for (int k = 0; k < K; ++k) { z[k] = exp(z[k] - m); Z += z[k]; }
        for (int k = 0; k < K; ++k) {
            const T w = z[k] / Z - (k == (int)y[i] ? T(1) : T(0));
            for (int j = 0; j < D; ++j) g[k * D + j] += w * X[i * D + j];
        }
    }
}
"""
# per_call: iterations per pbbi_hmc_run call; window: iterations per timed window of each side; warm: unrecorded iterations
SOFTMAX_SHAPES = {
    "k3": dict(M=256, D=5, classes=3, N=65536, h=0.2, per_call=32, window=dict(softmax=640, plugin=64), repeats=5, warm=4),
    "k8": dict(M=256, D=16, classes=8, N=65536, h=0.2, per_call=8, window=dict(softmax=256, plugin=8), repeats=5, warm=4),
    "k8large": dict(M=16384, D=16, classes=8, N=16384, h=0.02, per_call=2, window=dict(softmax=20, plugin=2), repeats=3,
                    warm=2),
}


def softmax_problem(M, D, K, seed=0):
    rs = np.random.RandomState(seed)
    X = rs.standard_normal((M, D)) / np.sqrt(D)
    X[:, 0] = 1.0
    W = rs.standard_normal((K, D))
    eta = X @ W.T
    g = -np.log(-np.log(rs.uniform(size=eta.shape)))     # Gumbel-max: y ~ softmax(eta)
    y = np.argmax(eta + g, axis=1).astype(np.float64)
    return X, y, W.ravel(), rs


def bench_softmax(name, M, D, classes, N, h, L, per_call, window, repeats, warm):
    """SoftmaxGLM and the same model through CustomPotential alternating in one process.  A window is window[side]
    iterations in pbbi_hmc_run calls of per_call (Runner.go never asks for more slabs than its buffers hold)."""
    from physicsbasedbayesianinference_amd.custom import CustomPotential
    X, y, w, rs = softmax_problem(M, D, classes)
    DT = classes * D
    q0 = np.ascontiguousarray(w[:, None] + 0.1 * rs.standard_normal((DT, N)))
    prm = np.concatenate([[float(M), float(classes)], X.ravel(), y, np.ones(D)])
    runners = {"softmax": Runner(P.SoftmaxGLM(X, y, classes=classes), DT, N, q0, h, L, per_call, window["softmax"]),
               "plugin": Runner(CustomPotential(DT, SOFTMAX_SOURCE, prm), DT, N, q0, h, L, per_call, window["plugin"])}
    for r in runners.values():
        r.go(warm)
    torch.cuda.synchronize()
    series = {k: [] for k in runners}
    for i in range(repeats):
        for k, r in runners.items():   # alternating
            series[k].append(r.timed())
            print(f"# {name} repeat {i} {k}: {series[k][-1]:.4f} s", flush=True)
    Dc, NT, _ = glm.softmax_layout(D, classes)
    grads = L + 1
    out = dict(shape=name, M=M, D=D, classes=classes, Dc=Dc, NT=NT, chains=N, L=L, h=h, iterations_per_call=per_call,
               iterations_per_window=dict(window), repeats=repeats, warmup_iterations=warm,
               timing="host clock over whole windows of pbbi_hmc_run calls (synchronised before and after)",
               accept_rate={k: 1.0 - float(r.rej.float().mean().item()) for k, r in runners.items()})
    per_it = {}
    for k, ts in series.items():
        out[k + "_seconds"] = ts
        out[k + "_step_chain_per_s"] = [window[k] * L * N / t for t in ts]
        per_it[k] = np.array(ts) / window[k]          # seconds per iteration
    flop_it = 4.0 * M * classes * Dc * grads * N
    out["softmax_executed_tflops"] = [flop_it / t / 1e12 for t in per_it["softmax"]]
    out["softmax_share_of_fp64_mfma_peak_executed"] = float(flop_it / np.median(per_it["softmax"]) / PEAK_F64_MFMA)
    out["ratio_median"] = float(np.median(per_it["plugin"]) / np.median(per_it["softmax"]))
    out["ratio_worst_case"] = float(per_it["plugin"].min() / per_it["softmax"].max())
    out["softmax_faster_by_the_medians"] = bool(np.median(per_it["softmax"]) < np.median(per_it["plugin"]))
    return out


# negative-binomial regression with a sampled log-dispersion as user source: prm = [M, X, a, y, o, lam(D + 1), mu(D + 1)];
# the state is (w, theta)
NEGBINOMIAL_SOURCE = """
PBBI_FN T nb_psi(T x) {
    T a = 0;
    while (x < T(6)) { a -= T(1) / x; x += T(1); }
    const T r = T(1) / x, r2 = r * r;
    return a + log(x) - T(0.5) * r - r2 * (T(1) / 12 - r2 * (T(1) / 120 - r2 * (T(1) / 252 - r2 * (T(1) / 240
           - r2 * (T(1) / 132 - r2 * (T(691) / 32760 - r2 * (T(1) / 12)))))));
}
template <class Q>
PBBI_FN T potential(const Q& q, int DT, const T* prm) {
    const int M = (int)prm[0], D = DT - 1;
    const T *X = prm + 1, *a = X + (long)M * D, *y = a + M, *o = y + M, *lam = o + M, *mu = lam + DT;
    const T th = q[D], phi = exp(th), lgphi = lgamma(phi);
    T s = 0;
    for (int i = 0; i < M; ++i) {
        if (a[i] == 0) continue;
        T z = o[i];
        for (int j = 0; j < D; ++j) z += X[i * D + j] * q[j];
        const T d = z - th, sp = (d > 0 ? d : T(0)) + log1p(exp(-fabs(d)));
        s += a[i] * (lgphi - lgamma(y[i] + phi) + (y[i] + phi) * sp - y[i] * d);
    }
    T r = 0;
    for (int j = 0; j < DT; ++j) r += lam[j] * (q[j] - mu[j]) * (q[j] - mu[j]);
    return s + T(0.5) * r;
}
template <class Q, class G>
PBBI_FN void gradient(const Q& q, G& g, int DT, const T* prm) {
    const int M = (int)prm[0], D = DT - 1;
    const T *X = prm + 1, *a = X + (long)M * D, *y = a + M, *o = y + M, *lam = o + M, *mu = lam + DT;
    const T th = q[D], phi = exp(th), psi_phi = nb_psi(phi);
    for (int j = 0; j < DT; ++j) g[j] = lam[j] * (q[j] - mu[j]);
    T gt = 0;
    for (int i = 0; i < M; ++i) {
        if (a[i] == 0) continue;
        T z = o[i];
        for (int j = 0; j < D; ++j) z += X[i * D + j] * q[j];
        const T d = z - th, e = exp(-fabs(d)), inv = T(1) / (T(1) + e);
        const T sg = d >= 0 ? inv : e * inv, sg1 = d >= 0 ? e * inv : inv, sp = (d > 0 ? d : T(0)) + log1p(e);
        const T w = a[i] * ((y[i] + phi) * sg - y[i]);
        gt += a[i] * (phi * (psi_phi - nb_psi(y[i] + phi) + sp - sg) + y[i] * sg1);
        for (int j = 0; j < D; ++j) g[j] += w * X[i * D + j];
    }
    g[D] += gt;
}
"""
# as SOFTMAX_SHAPES; D + 1 = 16 and 64: the last row of the DP = 16 and DP = 64 kernels is theta's
DISPERSION_SHAPES = {
    "small": dict(M=256, D=15, N=65536, h=0.05, per_call=32, window=dict(dispersion=256, plugin=32), repeats=5, warm=4),
    "large": dict(M=16384, D=63, N=16384, h=0.006, per_call=4, window=dict(dispersion=16, plugin=4), repeats=3, warm=2),
}


def dispersion_problem(M, D, seed=0):
    """Over-dispersed counts: X with an intercept column, offsets ~ N(0, 0.3), weights from {0.5, 1, 3}, phi = 2."""
    rs = np.random.RandomState(seed)
    X = rs.standard_normal((M, D)) / np.sqrt(D)
    X[:, 0] = 1.0
    w = 0.7 * rs.standard_normal(D)
    a = rs.choice([0.5, 1.0, 3.0], size=M)
    o = 0.3 * rs.standard_normal(M)
    phi = 2.0
    y = rs.poisson(rs.gamma(phi, np.exp(X @ w + o) / phi)).astype(np.float64)
    return dict(X=X, y=y, weights=a, offset=o), np.r_[w, np.log(phi)], rs


def bench_dispersion(name, M, D, N, h, L, per_call, window, repeats, warm):
    """DispersionGLM and the same model through CustomPotential alternating in one process, same data, starts, step size
    and draws."""
    from physicsbasedbayesianinference_amd.custom import CustomPotential
    kw, wt, rs = dispersion_problem(M, D)
    DT = D + 1
    q0 = np.ascontiguousarray(wt[:, None] + 0.05 * rs.standard_normal((DT, N)))
    prior = (0.0, 0.25)
    prm = np.concatenate([[float(M)], kw["X"].ravel(), kw["weights"], kw["y"], kw["offset"], np.r_[np.ones(D), prior[1]],
                          np.r_[np.zeros(D), prior[0]]])
    pot = P.DispersionGLM(family="negbinomial", dispersion="sample", log_dispersion_prior=prior, **kw)
    runners = {"dispersion": Runner(pot, DT, N, q0, h, L, per_call, window["dispersion"]),
               "plugin": Runner(CustomPotential(DT, NEGBINOMIAL_SOURCE, prm), DT, N, q0, h, L, per_call, window["plugin"])}
    for r in runners.values():
        r.go(warm)
    torch.cuda.synchronize()
    series = {k: [] for k in runners}
    for i in range(repeats):
        for k, r in runners.items():   # alternating
            series[k].append(r.timed())
            print(f"# {name} repeat {i} {k}: {series[k][-1]:.4f} s", flush=True)
    DP = glm.padded_dim(DT)
    grads = L + 1
    out = dict(shape=name, M=M, D=D, state_dimension=DT, DP=DP, chains=N, L=L, h=h, iterations_per_call=per_call,
               iterations_per_window=dict(window), repeats=repeats, warmup_iterations=warm,
               timing="host clock over whole windows of pbbi_hmc_run calls (synchronised before and after)",
               accept_rate={k: 1.0 - float(r.rej.float().mean().item()) for k, r in runners.items()})
    per_it = {}
    for k, ts in series.items():
        out[k + "_seconds"] = ts
        out[k + "_step_chain_per_s"] = [window[k] * L * N / t for t in ts]
        per_it[k] = np.array(ts) / window[k]          # seconds per iteration
    flop_it = 4.0 * M * DP * grads * N
    out["dispersion_executed_tflops"] = [flop_it / t / 1e12 for t in per_it["dispersion"]]
    out["dispersion_share_of_fp64_mfma_peak_executed"] = float(flop_it / np.median(per_it["dispersion"]) / PEAK_F64_MFMA)
    out["ratio_median"] = float(np.median(per_it["plugin"]) / np.median(per_it["dispersion"]))
    out["ratio_worst_case"] = float(per_it["plugin"].min() / per_it["dispersion"].max())  # fastest plugin over slowest kernel
    out["slowest_dispersion_beats_fastest_plugin"] = bool(per_it["dispersion"].max() < per_it["plugin"].min())
    return out

def bench_gamma(name, M, D, N, h, L, per_call, window, repeats, warm):
    """The three dispersion families of DispersionGLM (sampled dispersion) alternating in one process after warm-up: the same
    X, weights, offsets, starts, step size and draws; y from each family's own model at the same linear predictor (sigma = 0.5,
    phi = 2, alpha = 2).  No plugin side: what is measured is the cost of each family's link on the same kernel frame."""
    kw, wt, rs = dispersion_problem(M, D)
    DT = D + 1
    q0 = np.ascontiguousarray(wt[:, None] + 0.05 * rs.standard_normal((DT, N)))
    eta = kw["X"] @ wt[:D] + kw["offset"]
    ys = {"gaussian": eta + 0.5 * rs.standard_normal(M), "negbinomial": kw["y"],
          "gamma": np.maximum(rs.gamma(2.0, np.exp(eta) / 2.0), 1e-6)}
    theta0 = {"gaussian": np.log(0.5), "negbinomial": np.log(2.0), "gamma": np.log(2.0)}
    prior = (0.0, 0.25)
    W = window["dispersion"]
    runners = {}
    for fam in ("gaussian", "gamma", "negbinomial"):
        q = q0.copy()
        q[D] += theta0[fam] - wt[D]
        pot = P.DispersionGLM(**dict(kw, y=ys[fam]), family=fam, dispersion="sample", log_dispersion_prior=prior)
        runners[fam] = Runner(pot, DT, N, q, h, L, per_call, W)
    for r in runners.values():
        r.go(warm)
    torch.cuda.synchronize()
    series = {k: [] for k in runners}
    for i in range(repeats):
        for k, r in runners.items():   # alternating
            series[k].append(r.timed())
            print(f"# {name} repeat {i} {k}: {series[k][-1]:.4f} s", flush=True)
    DP = glm.padded_dim(DT)
    out = dict(shape=name, M=M, D=D, state_dimension=DT, DP=DP, chains=N, L=L, h=h, iterations_per_call=per_call,
               iterations_per_window=W, repeats=repeats, warmup_iterations=warm,
               timing="host clock over whole windows of pbbi_hmc_run calls (synchronised before and after)",
               accept_rate={k: 1.0 - float(r.rej.float().mean().item()) for k, r in runners.items()})
    flop_it = 4.0 * M * DP * (L + 1) * N
    med = {}
    for k, ts in series.items():
        out[k + "_seconds"] = ts
        out[k + "_step_chain_per_s"] = [W * L * N / t for t in ts]
        med[k] = float(np.median(ts))
        out[k + "_executed_tflops_median"] = flop_it * W / med[k] / 1e12
    out["gamma_over_gaussian_time_median"] = med["gamma"] / med["gaussian"]
    out["negbinomial_over_gamma_time_median"] = med["negbinomial"] / med["gamma"]
    out["gamma_lies_between"] = bool(med["gaussian"] <= med["gamma"] <= med["negbinomial"])
    return out


ORDINAL_K = 5


def ordinal_problem(M, D, seed=0):
    """Ordered categories (K = 5) from D covariates (no intercept column), offsets ~ N(0, 0.3), weights from {0.5, 1, 3}; and, for
    the logistic side, the same X widened by K - 1 further covariates to the ordinal model's state dimension with the response
    cut in two at the middle category."""
    K = ORDINAL_K
    rs = np.random.RandomState(seed)
    X = rs.standard_normal((M, D)) / np.sqrt(D)
    w = 0.7 * rs.standard_normal(D)
    zeta = np.r_[-1.2, np.full(K - 2, -0.2)]
    kappa = np.cumsum(np.r_[zeta[0], np.exp(zeta[1:])])
    a = rs.choice([0.5, 1.0, 3.0], size=M)
    o = 0.3 * rs.standard_normal(M)
    y = ((rs.logistic(size=M) + X @ w + o)[:, None] > kappa[None, :]).sum(axis=1).astype(np.float64)
    Xl = np.hstack([X, rs.standard_normal((M, K - 1)) / np.sqrt(D)])
    return dict(X=X, y=y, weights=a, offset=o), dict(X=Xl, y=(y >= 2).astype(np.float64), weights=a, offset=o), np.r_[w, zeta], rs


def ordinal_runners(M, D, N, h, L, per_call, W, sides):
    """The runners of --model ordinal / logistic: OrdinalGLM (K = 5, state dimension D + 4) and the full logistic model at the
    same padded state dimension, same weights, offsets, starts and draws."""
    kwo, kwl, wt, rs = ordinal_problem(M, D)
    DT = D + ORDINAL_K - 1
    q0 = np.ascontiguousarray(wt[:, None] + 0.05 * rs.standard_normal((DT, N)))
    runners = {}
    if "ordinal" in sides:
        runners["ordinal"] = Runner(P.OrdinalGLM(categories=ORDINAL_K, **kwo), DT, N, q0, h, L, per_call, W)
    if "logistic" in sides:
        ql = q0.copy()
        ql[D:] = 0.05 * rs.standard_normal((ORDINAL_K - 1, N))
        runners["logistic"] = Runner(P.GLM(family="logistic", **kwl), DT, N, ql, h, L, per_call, W)
    return runners, DT


def bench_ordinal(name, M, D, N, h, L, per_call, window, repeats, warm, sides=("ordinal", "logistic"), baseline=None):
    """OrdinalGLM (K = 5) and the full logistic model at the same padded state dimension alternating in one process after warm-up
    (M, N, h and the window lengths are --model dispersion's; D is 4 less, so that the state dimensions are its 16 and 64).  No
    plugin side: what is measured is the cost of the ordinal link -- two exp, the select chains and the K - 1 reductions -- on the
    same kernel frame.  sides = ("logistic",): that side alone (--model logistic), which run on another build of the library
    gives the record `baseline` -- then merged here as logistic_baseline_*, with the ordinal kernel's time over it."""
    W = window["dispersion"]
    runners, DT = ordinal_runners(M, D - (ORDINAL_K - 2), N, h, L, per_call, W, sides)
    for r in runners.values():
        r.go(warm)
    torch.cuda.synchronize()
    series = {k: [] for k in runners}
    for i in range(repeats):
        for k, r in runners.items():   # alternating
            series[k].append(r.timed())
            print(f"# {name} repeat {i} {k}: {series[k][-1]:.4f} s", flush=True)
    DP = glm.padded_dim(DT)
    out = dict(shape=name, M=M, D=DT - (ORDINAL_K - 1), categories=ORDINAL_K, state_dimension=DT, DP=DP, chains=N, L=L, h=h,
               iterations_per_call=per_call, iterations_per_window=W, repeats=repeats, warmup_iterations=warm,
               timing="host clock over whole windows of pbbi_hmc_run calls (synchronised before and after)",
               accept_rate={k: 1.0 - float(r.rej.float().mean().item()) for k, r in runners.items()})
    flop_it = 4.0 * M * DP * (L + 1) * N
    med = {}
    for k, ts in series.items():
        out[k + "_seconds"] = ts
        out[k + "_step_chain_per_s"] = [W * L * N / t for t in ts]
        med[k] = float(np.median(ts))
        out[k + "_executed_tflops_median"] = flop_it * W / med[k] / 1e12
    if "ordinal" in med and "logistic" in med:
        out["ordinal_over_logistic_time_median"] = med["ordinal"] / med["logistic"]
    if baseline is not None and "ordinal" in med:
        out["logistic_baseline_seconds"] = baseline["logistic_seconds"]
        out["logistic_baseline_build"] = baseline.get("build", "another build of the library")
        out["ordinal_over_logistic_baseline_time_median"] = med["ordinal"] / float(np.median(baseline["logistic_seconds"]))
    return out


# negative-binomial regression with sampled group scales and a sampled log-dispersion as user source (centred): prm = [M, D, J, X,
# a, y, o, lam(DT), mu(DT), groups(D)], the state (w, t, theta); nb_psi is NEGBINOMIAL_SOURCE's
HIER_NEGBINOMIAL_SOURCE = NEGBINOMIAL_SOURCE[:NEGBINOMIAL_SOURCE.index("template <class Q>")] + """
template <class Q>
PBBI_FN T potential(const Q& q, int DT, const T* prm) {
    const int M = (int)prm[0], D = (int)prm[1], J = (int)prm[2];
    const T *X = prm + 3, *a = X + (long)M * D, *y = a + M, *o = y + M, *lam = o + M, *mu = lam + DT, *grp = mu + DT;
    const T th = q[D + J], phi = exp(th), lgphi = lgamma(phi);
    T s = 0;
    for (int i = 0; i < M; ++i) {
        if (a[i] == 0) continue;
        T z = o[i];
        for (int j = 0; j < D; ++j) z += X[i * D + j] * q[j];
        const T d = z - th, sp = (d > 0 ? d : T(0)) + log1p(exp(-fabs(d)));
        s += a[i] * (lgphi - lgamma(y[i] + phi) + (y[i] + phi) * sp - y[i] * d);
    }
    T r = 0;
    for (int j = 0; j < D; ++j) {
        const int k = (int)grp[j];
        const T e = q[j] - mu[j];
        if (k < 0) { r += lam[j] * e * e; } else { r += exp(-2 * q[D + k]) * e * e; s += q[D + k]; }
    }
    for (int j = D; j < DT; ++j) r += lam[j] * (q[j] - mu[j]) * (q[j] - mu[j]);
    return s + T(0.5) * r;
}
template <class Q, class G>
PBBI_FN void gradient(const Q& q, G& g, int DT, const T* prm) {
    const int M = (int)prm[0], D = (int)prm[1], J = (int)prm[2];
    const T *X = prm + 3, *a = X + (long)M * D, *y = a + M, *o = y + M, *lam = o + M, *mu = lam + DT, *grp = mu + DT;
    const T th = q[D + J], phi = exp(th), psi_phi = nb_psi(phi);
    for (int j = D; j < DT; ++j) g[j] = lam[j] * (q[j] - mu[j]);
    for (int j = 0; j < D; ++j) {
        const int k = (int)grp[j];
        const T e = q[j] - mu[j];
        if (k < 0) { g[j] = lam[j] * e; } else { const T tau = exp(-2 * q[D + k]); g[j] = tau * e; g[D + k] += T(1) - tau * e * e; }
    }
    T gt = 0;
    for (int i = 0; i < M; ++i) {
        if (a[i] == 0) continue;
        T z = o[i];
        for (int j = 0; j < D; ++j) z += X[i * D + j] * q[j];
        const T d = z - th, e = exp(-fabs(d)), inv = T(1) / (T(1) + e);
        const T sg = d >= 0 ? inv : e * inv, sg1 = d >= 0 ? e * inv : inv, sp = (d > 0 ? d : T(0)) + log1p(e);
        const T w = a[i] * ((y[i] + phi) * sg - y[i]);
        gt += a[i] * (phi * (psi_phi - nb_psi(y[i] + phi) + sp - sg) + y[i] * sg1);
        for (int j = 0; j < D; ++j) g[j] += w * X[i * D + j];
    }
    g[D + J] += gt;
}
"""
# as DISPERSION_SHAPES; D + J + 1 = 16 and 64: theta is the last row of the DP = 16 and DP = 64 kernels, the t rows before it
HIER_DISP_SHAPES = {
    "small": dict(M=256, D=13, J=2, N=65536, h=0.05, per_call=32,
                  window=dict(centred=256, noncentred=256, plugin=32, parent=256), repeats=5, warm=4),
    "large": dict(M=16384, D=59, J=4, N=16384, h=0.006, per_call=4,
                  window=dict(centred=16, noncentred=16, plugin=4, parent=16), repeats=3, warm=2),
}


def bench_hier_dispersion(name, M, D, J, N, h, L, per_call, window, repeats, warm):
    """HierarchicalDispersionGLM (centred and non-centred), the centred model through CustomPotential and DispersionGLM of
    [X | 0] with the scales held alternating in one process: same data, step size and draws, the same starts in natural
    coordinates (the non-centred side starts at from_natural of them)."""
    from physicsbasedbayesianinference_amd.custom import CustomPotential
    kw, wt, rs = dispersion_problem(M, D)
    nfix = (D - 2) % J + 2
    groups = np.r_[np.full(nfix, -1), np.arange(D - nfix) % J]
    t = np.log(np.array([np.std(wt[:D][groups == j]) for j in range(J)]))     # scales that fit the coefficients drawn
    DT = D + J + 1
    tprior, dprior = (-0.5, 1.0), (0.0, 0.25)
    q0 = np.ascontiguousarray(np.r_[wt[:D], t, wt[D]][:, None] + 0.05 * rs.standard_normal((DT, N)))
    lam, mu = np.r_[np.ones(D), np.full(J, tprior[1]), dprior[1]], np.r_[np.zeros(D), np.full(J, tprior[0]), dprior[0]]
    prm = np.concatenate([[float(M), float(D), float(J)], kw["X"].ravel(), kw["weights"], kw["y"], kw["offset"], lam, mu,
                          groups.astype(float)])
    hd = dict(family="negbinomial", groups=groups, dispersion="sample", log_dispersion_prior=dprior, log_scale_prior=tprior,
              prior_precision=1.0, **kw)
    cen = P.HierarchicalDispersionGLM(**hd)
    ncp = P.HierarchicalDispersionGLM(parametrisation="noncentred", **hd)
    lam_held = np.r_[np.where(groups < 0, 1.0, np.exp(-2.0 * t)[np.maximum(groups, 0)]), np.full(J, tprior[1])]
    parent = P.DispersionGLM(np.hstack([kw["X"], np.zeros((M, J))]), kw["y"], family="negbinomial", dispersion="sample",
                             log_dispersion_prior=dprior, prior_precision=lam_held, prior_mean=mu[:D + J],
                             weights=kw["weights"], offset=kw["offset"])
    assert parent.numDimensions == DT == cen.numDimensions == ncp.numDimensions
    runners = {"centred": Runner(cen, DT, N, q0, h, L, per_call, window["centred"]),
               "noncentred": Runner(ncp, DT, N, np.ascontiguousarray(ncp.from_natural(q0)), h, L, per_call, window["noncentred"]),
               "plugin": Runner(CustomPotential(DT, HIER_NEGBINOMIAL_SOURCE, prm), DT, N, q0, h, L, per_call, window["plugin"]),
               "parent": Runner(parent, DT, N, q0, h, L, per_call, window["parent"])}
    for r in runners.values():
        r.go(warm)
    torch.cuda.synchronize()
    series = {k: [] for k in runners}
    for i in range(repeats):
        for k, r in runners.items():   # alternating
            series[k].append(r.timed())
            print(f"# {name} repeat {i} {k}: {series[k][-1]:.4f} s", flush=True)
    DP = glm.padded_dim(DT)
    grads = L + 1
    out = dict(shape=name, family="negbinomial", M=M, D=D, J=J, state_dimension=DT, DP=DP, chains=N, L=L, h=h,
               iterations_per_call=per_call, iterations_per_window=dict(window), repeats=repeats, warmup_iterations=warm,
               timing="host clock over whole windows of pbbi_hmc_run calls (synchronised before and after)",
               accept_rate={k: 1.0 - float(r.rej.float().mean().item()) for k, r in runners.items()})
    per_it = {}
    for k, ts in series.items():
        out[k + "_seconds"] = ts
        out[k + "_step_chain_per_s"] = [window[k] * L * N / t_ for t_ in ts]
        per_it[k] = np.array(ts) / window[k]          # seconds per iteration
    flop_it = 4.0 * M * DP * grads * N
    for k in ("centred", "noncentred"):
        out[k + "_share_of_fp64_mfma_peak_executed"] = float(flop_it / np.median(per_it[k]) / PEAK_F64_MFMA)
        out[k + "_over_parent_median"] = float(np.median(per_it[k]) / np.median(per_it["parent"]))   # the cost of the prior
    out["plugin_over_centred_median"] = float(np.median(per_it["plugin"]) / np.median(per_it["centred"]))
    out["plugin_over_centred_worst_case"] = float(per_it["plugin"].min() / per_it["centred"].max())
    return out


# the hierarchical model as user source: prm = [M, D, X, c, d, o, lam(D + J), mu(D + J), groups(D)], c = a n, d = a y
HIER_LOGISTIC_SOURCE = """
template <class Q>
PBBI_FN T potential(const Q& q, int DT, const T* prm) {
    const int M = (int)prm[0], D = (int)prm[1];
    const T *X = prm + 2, *c = X + (long)M * D, *d = c + M, *o = d + M, *lam = o + M, *mu = lam + DT, *grp = mu + DT;
    T s = 0;
    for (int i = 0; i < M; ++i) {
        if (c[i] == 0 && d[i] == 0) continue;
        T z = o[i];
        for (int j = 0; j < D; ++j) z += X[i * D + j] * q[j];
        s += c[i] * ((z > 0 ? z : T(0)) + log1p(exp(-fabs(z)))) - d[i] * z;
    }
    T r = 0;
    for (int j = 0; j < D; ++j) {
        const int k = (int)grp[j];
        const T e = q[j] - mu[j];
        if (k < 0) { r += lam[j] * e * e; } else { r += exp(-2 * q[D + k]) * e * e; s += q[D + k]; }
    }
    for (int j = D; j < DT; ++j) r += lam[j] * (q[j] - mu[j]) * (q[j] - mu[j]);
    return s + T(0.5) * r;
}
template <class Q, class G>
PBBI_FN void gradient(const Q& q, G& g, int DT, const T* prm) {
    const int M = (int)prm[0], D = (int)prm[1];
    const T *X = prm + 2, *c = X + (long)M * D, *d = c + M, *o = d + M, *lam = o + M, *mu = lam + DT, *grp = mu + DT;
    for (int j = D; j < DT; ++j) g[j] = lam[j] * (q[j] - mu[j]);
    for (int j = 0; j < D; ++j) {
        const int k = (int)grp[j];
        const T e = q[j] - mu[j];
        if (k < 0) { g[j] = lam[j] * e; } else { const T tau = exp(-2 * q[D + k]); g[j] = tau * e; g[D + k] += T(1) - tau * e * e; }
    }
    for (int i = 0; i < M; ++i) {
        if (c[i] == 0 && d[i] == 0) continue;
        T z = o[i];
        for (int j = 0; j < D; ++j) z += X[i * D + j] * q[j];
        const T w = c[i] / (T(1) + exp(-z)) - d[i];
        for (int j = 0; j < D; ++j) g[j] += w * X[i * D + j];
    }
}
"""
# as SOFTMAX_SHAPES; D + J = 16 and 64: the t rows are the last rows of the DP = 16 and DP = 64 kernels
HIER_SHAPES = {
    "small": dict(M=256, D=14, J=2, N=65536, h=0.12, per_call=32, window=dict(hier=256, plugin=32, fixed=256), repeats=5, warm=4),
    "large": dict(M=16384, D=60, J=4, N=16384, h=0.04, per_call=4, window=dict(hier=16, plugin=4, fixed=16), repeats=3, warm=2),
}


def hier_problem(M, D, J, seed=0):
    """rich_problem()'s recipe (weights, offsets, binomial trials) with the first D % J + 2 coefficients under a fixed
    prior of precision 1 and the others in J equal groups of scale exp(t_j), t_j in [-1, 0]."""
    rs = np.random.RandomState(seed)
    X = rs.standard_normal((M, D)) / np.sqrt(D)
    nfix = (D - 2) % J + 2
    groups = np.r_[np.full(nfix, -1), np.arange(D - nfix) % J]
    t = rs.uniform(-1.0, 0.0, size=J)
    w = np.where(groups < 0, 1.0, np.exp(t)[np.maximum(groups, 0)]) * rs.standard_normal(D)
    a = rs.choice([0.0, 0.5, 1.0, 3.0], size=M)
    o = 0.3 * rs.standard_normal(M)
    n = rs.randint(1, 21, size=M).astype(np.float64)
    y = rs.binomial(n.astype(int), 1.0 / (1.0 + np.exp(-(X @ w + o)))).astype(np.float64)
    return dict(X=X, y=y, weights=a, offset=o, trials=n, groups=groups), w, t, rs


def bench_hier(name, M, D, J, N, h, L, per_call, window, repeats, warm):
    """HierarchicalGLM, the same model through CustomPotential and a fixed-prior GLM of [X | 0] alternating in one process:
    same data, starts, step size and draws."""
    from physicsbasedbayesianinference_amd.custom import CustomPotential
    kw, w, t, rs = hier_problem(M, D, J)
    DT = D + J
    tprior = (-0.5, 1.0)
    q0 = np.ascontiguousarray(np.r_[w, t][:, None] + 0.05 * rs.standard_normal((DT, N)))
    groups = kw["groups"]
    prm = np.concatenate([[float(M), float(D)], kw["X"].ravel(), kw["weights"] * kw["trials"], kw["weights"] * kw["y"],
                          kw["offset"], np.r_[np.ones(D), np.full(J, tprior[1])], np.r_[np.zeros(D), np.full(J, tprior[0])],
                          groups.astype(float)])
    lam_fixed = np.r_[np.where(groups < 0, 1.0, np.exp(-2.0 * t)[np.maximum(groups, 0)]), np.full(J, tprior[1])]
    fixed = P.GLM(np.hstack([kw["X"], np.zeros((M, J))]), kw["y"], prior_precision=lam_fixed,
                  prior_mean=np.r_[np.zeros(D), np.full(J, tprior[0])], weights=kw["weights"], offset=kw["offset"],
                  trials=kw["trials"])
    pot = P.HierarchicalGLM(log_scale_prior=tprior, prior_precision=1.0, **kw)
    runners = {"hier": Runner(pot, DT, N, q0, h, L, per_call, window["hier"]),
               "plugin": Runner(CustomPotential(DT, HIER_LOGISTIC_SOURCE, prm), DT, N, q0, h, L, per_call, window["plugin"]),
               "fixed": Runner(fixed, DT, N, q0, h, L, per_call, window["fixed"])}
    for r in runners.values():
        r.go(warm)
    torch.cuda.synchronize()
    series = {k: [] for k in runners}
    for i in range(repeats):
        for k, r in runners.items():   # alternating
            series[k].append(r.timed())
            print(f"# {name} repeat {i} {k}: {series[k][-1]:.4f} s", flush=True)
    DP = glm.padded_dim(DT)
    grads = L + 1
    out = dict(shape=name, M=M, D=D, J=J, state_dimension=DT, DP=DP, chains=N, L=L, h=h, iterations_per_call=per_call,
               iterations_per_window=dict(window), repeats=repeats, warmup_iterations=warm,
               timing="host clock over whole windows of pbbi_hmc_run calls (synchronised before and after)",
               accept_rate={k: 1.0 - float(r.rej.float().mean().item()) for k, r in runners.items()})
    per_it = {}
    for k, ts in series.items():
        out[k + "_seconds"] = ts
        out[k + "_step_chain_per_s"] = [window[k] * L * N / t_ for t_ in ts]
        per_it[k] = np.array(ts) / window[k]          # seconds per iteration
    flop_it = 4.0 * M * DP * grads * N
    out["hier_executed_tflops"] = [flop_it / t_ / 1e12 for t_ in per_it["hier"]]
    out["hier_share_of_fp64_mfma_peak_executed"] = float(flop_it / np.median(per_it["hier"]) / PEAK_F64_MFMA)
    out["ratio_median"] = float(np.median(per_it["plugin"]) / np.median(per_it["hier"]))
    out["ratio_worst_case"] = float(per_it["plugin"].min() / per_it["hier"].max())  # fastest plugin over slowest kernel
    out["slowest_hier_beats_fastest_plugin"] = bool(per_it["hier"].max() < per_it["plugin"].min())
    out["hier_over_fixed_median"] = float(np.median(per_it["hier"]) / np.median(per_it["fixed"]))   # recorded, not gated
    return out


# the non-centred hierarchical model as user source: prm as for HIER_LOGISTIC_SOURCE; a grouped row of the state holds z_j
# with w_j = mu_j + exp(t_k) z_j
HIER_NC_LOGISTIC_SOURCE = """
template <class Q>
PBBI_FN T coef(const Q& q, int j, const T* mu, const T* grp, const T* sig) {
    const int k = (int)grp[j];
    return k < 0 ? q[j] : mu[j] + sig[k] * q[j];
}
template <class Q>
PBBI_FN T potential(const Q& q, int DT, const T* prm) {
    const int M = (int)prm[0], D = (int)prm[1];
    const T *X = prm + 2, *c = X + (long)M * D, *d = c + M, *o = d + M, *lam = o + M, *mu = lam + DT, *grp = mu + DT;
    T sig[4] = {1, 1, 1, 1};
    for (int k = 0; k < DT - D; ++k) sig[k] = exp(q[D + k]);
    T s = 0;
    for (int i = 0; i < M; ++i) {
        if (c[i] == 0 && d[i] == 0) continue;
        T z = o[i];
        for (int j = 0; j < D; ++j) z += X[i * D + j] * coef(q, j, mu, grp, sig);
        s += c[i] * ((z > 0 ? z : T(0)) + log1p(exp(-fabs(z)))) - d[i] * z;
    }
    T r = 0;
    for (int j = 0; j < D; ++j) {
        const T e = q[j] - mu[j];
        if ((int)grp[j] < 0) { r += lam[j] * e * e; } else { r += q[j] * q[j]; }
    }
    for (int j = D; j < DT; ++j) r += lam[j] * (q[j] - mu[j]) * (q[j] - mu[j]);
    return s + T(0.5) * r;
}
template <class Q, class G>
PBBI_FN void gradient(const Q& q, G& g, int DT, const T* prm) {
    const int M = (int)prm[0], D = (int)prm[1];
    const T *X = prm + 2, *c = X + (long)M * D, *d = c + M, *o = d + M, *lam = o + M, *mu = lam + DT, *grp = mu + DT;
    T sig[4] = {1, 1, 1, 1};
    for (int k = 0; k < DT - D; ++k) sig[k] = exp(q[D + k]);
    for (int j = 0; j < D; ++j) g[j] = 0;
    for (int i = 0; i < M; ++i) {
        if (c[i] == 0 && d[i] == 0) continue;
        T z = o[i];
        for (int j = 0; j < D; ++j) z += X[i * D + j] * coef(q, j, mu, grp, sig);
        const T w = c[i] / (T(1) + exp(-z)) - d[i];
        for (int j = 0; j < D; ++j) g[j] += w * X[i * D + j];
    }
    for (int j = D; j < DT; ++j) g[j] = lam[j] * (q[j] - mu[j]);
    for (int j = 0; j < D; ++j) {
        const int k = (int)grp[j];
        if (k < 0) { g[j] += lam[j] * (q[j] - mu[j]); } else { g[D + k] += sig[k] * g[j] * q[j]; g[j] = sig[k] * g[j] + q[j]; }
    }
}
"""
# as HIER_SHAPES, with a step size per parametrisation (h: centred, as there; h_nc: non-centred)
HIER_NC_SHAPES = {
    "small": dict(M=256, D=14, J=2, N=65536, h=0.12, h_nc=0.08, per_call=32,
                  window=dict(noncentred=1024, centred=1024, plugin=64), repeats=5, warm=4),
    "large": dict(M=16384, D=60, J=4, N=16384, h=0.04, h_nc=0.02, per_call=4,
                  window=dict(noncentred=48, centred=48, plugin=4), repeats=3, warm=2),
    # DP = 32, where the non-centred logistic kernel runs one wave per SIMD and the centred one two (not part of "all")
    "mid": dict(M=2048, D=28, J=4, N=32768, h=0.06, h_nc=0.03, per_call=16,
                window=dict(noncentred=256, centred=256, plugin=16), repeats=5, warm=4),
}


def hier_nc_setup(M, D, J, N):
    """hier_problem's data as the keyword arguments of HierarchicalGLM, prm of the user source, and the starts of bench_hier
    in natural coordinates."""
    kw, w, t, rs = hier_problem(M, D, J)
    tprior = (-0.5, 1.0)
    q0 = np.ascontiguousarray(np.r_[w, t][:, None] + 0.05 * rs.standard_normal((D + J, N)))
    prm = np.concatenate([[float(M), float(D)], kw["X"].ravel(), kw["weights"] * kw["trials"], kw["weights"] * kw["y"],
                          kw["offset"], np.r_[np.ones(D), np.full(J, tprior[1])], np.r_[np.zeros(D), np.full(J, tprior[0])],
                          kw["groups"].astype(float)])
    return dict(log_scale_prior=tprior, prior_precision=1.0, **kw), prm, q0


def bench_hier_nc(name, M, D, J, N, h, h_nc, L, per_call, window, repeats, warm):
    """The non-centred HierarchicalGLM, the centred one and the non-centred model through CustomPotential alternating in one
    process: same data and draws, the same starting points (each in its own coordinates)."""
    from physicsbasedbayesianinference_amd.custom import CustomPotential
    kw, prm, q0c = hier_nc_setup(M, D, J, N)
    DT = D + J
    pot = P.HierarchicalGLM(parametrisation="noncentred", **kw)
    q0 = np.ascontiguousarray(pot.from_natural(q0c))
    runners = {"noncentred": Runner(pot, DT, N, q0, h_nc, L, per_call, window["noncentred"]),
               "centred": Runner(P.HierarchicalGLM(**kw), DT, N, q0c, h, L, per_call, window["centred"]),
               "plugin": Runner(CustomPotential(DT, HIER_NC_LOGISTIC_SOURCE, prm), DT, N, q0, h_nc, L, per_call, window["plugin"])}
    for r in runners.values():
        r.go(warm)
    torch.cuda.synchronize()
    series = {k: [] for k in runners}
    for i in range(repeats):
        for k, r in runners.items():   # alternating
            series[k].append(r.timed())
            print(f"# {name} repeat {i} {k}: {series[k][-1]:.4f} s", flush=True)
    DP = glm.padded_dim(DT)
    grads = L + 1
    out = dict(shape=name, M=M, D=D, J=J, state_dimension=DT, DP=DP, chains=N, L=L, h=dict(centred=h, noncentred=h_nc, plugin=h_nc),
               iterations_per_call=per_call, iterations_per_window=dict(window), repeats=repeats, warmup_iterations=warm,
               timing="host clock over whole windows of pbbi_hmc_run calls (synchronised before and after)",
               accept_rate={k: 1.0 - float(r.rej.float().mean().item()) for k, r in runners.items()})
    per_it = {}
    for k, ts in series.items():
        out[k + "_seconds"] = ts
        out[k + "_step_chain_per_s"] = [window[k] * L * N / t_ for t_ in ts]
        per_it[k] = np.array(ts) / window[k]          # seconds per iteration
    flop_it = 4.0 * M * DP * grads * N
    out["noncentred_executed_tflops"] = [flop_it / t_ / 1e12 for t_ in per_it["noncentred"]]
    out["noncentred_share_of_fp64_mfma_peak_executed"] = float(flop_it / np.median(per_it["noncentred"]) / PEAK_F64_MFMA)
    out["ratio_median"] = float(np.median(per_it["plugin"]) / np.median(per_it["noncentred"]))
    out["ratio_worst_case"] = float(per_it["plugin"].min() / per_it["noncentred"].max())  # fastest plugin over slowest kernel
    out["slowest_noncentred_beats_fastest_plugin"] = bool(per_it["noncentred"].max() < per_it["plugin"].min())
    out["noncentred_over_centred_median"] = float(np.median(per_it["noncentred"]) / np.median(per_it["centred"]))  # reported, not gated
    return out


# the structured model as user source: prm = [M, D, X, c, d, o, lam(D + J), mu(D + J), groups(D), Q(D x D), rank(J)], Q in
# coefficient indexing (zero between groups)
HIERQ_LOGISTIC_SOURCE = """
template <class Q>
PBBI_FN T potential(const Q& q, int DT, const T* prm) {
    const int M = (int)prm[0], D = (int)prm[1];
    const T *X = prm + 2, *c = X + (long)M * D, *d = c + M, *o = d + M, *lam = o + M, *mu = lam + DT, *grp = mu + DT;
    const T *P = grp + D, *rank = P + (long)D * D;
    T s = 0;
    for (int i = 0; i < M; ++i) {
        if (c[i] == 0 && d[i] == 0) continue;
        T z = o[i];
        for (int j = 0; j < D; ++j) z += X[i * D + j] * q[j];
        s += c[i] * ((z > 0 ? z : T(0)) + log1p(exp(-fabs(z)))) - d[i] * z;
    }
    T r = 0;
    for (int j = 0; j < D; ++j) {
        const int k = (int)grp[j];
        const T e = q[j] - mu[j];
        if (k < 0) { r += lam[j] * e * e; continue; }
        T pe = 0;
        for (int l = 0; l < D; ++l) if ((int)grp[l] == k) pe += P[j * D + l] * (q[l] - mu[l]);
        r += exp(-2 * q[D + k]) * e * pe;
    }
    for (int j = D; j < DT; ++j) { r += lam[j] * (q[j] - mu[j]) * (q[j] - mu[j]); s += rank[j - D] * q[j]; }
    return s + T(0.5) * r;
}
template <class Q, class G>
PBBI_FN void gradient(const Q& q, G& g, int DT, const T* prm) {
    const int M = (int)prm[0], D = (int)prm[1];
    const T *X = prm + 2, *c = X + (long)M * D, *d = c + M, *o = d + M, *lam = o + M, *mu = lam + DT, *grp = mu + DT;
    const T *P = grp + D, *rank = P + (long)D * D;
    for (int j = D; j < DT; ++j) g[j] = rank[j - D] + lam[j] * (q[j] - mu[j]);
    for (int j = 0; j < D; ++j) {
        const int k = (int)grp[j];
        const T e = q[j] - mu[j];
        if (k < 0) { g[j] = lam[j] * e; continue; }
        T pe = 0;
        for (int l = 0; l < D; ++l) if ((int)grp[l] == k) pe += P[j * D + l] * (q[l] - mu[l]);
        const T tau = exp(-2 * q[D + k]);
        g[j] = tau * pe;
        g[D + k] -= tau * e * pe;
    }
    for (int i = 0; i < M; ++i) {
        if (c[i] == 0 && d[i] == 0) continue;
        T z = o[i];
        for (int j = 0; j < D; ++j) z += X[i * D + j] * q[j];
        const T w = c[i] / (T(1) + exp(-z)) - d[i];
        for (int j = 0; j < D; ++j) g[j] += w * X[i * D + j];
    }
}
"""
# as HIER_SHAPES (the same data and groups); h: the exchangeable side, h_q: the structured sides (an RW2 penalty's largest
# eigenvalue is 16: the stiffest direction is four times as stiff)
HIERQ_SHAPES = {
    "small": dict(M=256, D=14, J=2, N=65536, h=0.12, h_q=0.03, per_call=32,
                  window=dict(hierq=1024, hier=1024, plugin=32), repeats=5, warm=4),
    "large": dict(M=16384, D=60, J=4, N=16384, h=0.04, h_q=0.01, per_call=4,
                  window=dict(hierq=48, hier=48, plugin=4), repeats=3, warm=2),
}


def bench_hierq(name, M, D, J, N, h, h_q, L, per_call, window, repeats, warm):
    """HierarchicalGLM with an RW2 penalty on every group, the same groups without a penalty (the centred kernel) and the
    structured model through CustomPotential alternating in one process: same data, starts and draws."""
    from physicsbasedbayesianinference_amd.custom import CustomPotential
    kw, prm0, q0 = hier_nc_setup(M, D, J, N)
    DT = D + J
    groups = kw["groups"]
    penalty = {j: P.HierarchicalGLM.random_walk_penalty(int(np.sum(groups == j)), 2) for j in range(J)}
    pot = P.HierarchicalGLM(penalty=penalty, **kw)
    full = np.zeros((D, D))
    for j in range(J):
        idx = np.flatnonzero(groups == j)
        full[np.ix_(idx, idx)] = penalty[j]
    prm = np.concatenate([prm0, full.ravel(), np.asarray(pot.penalty_rank, dtype=np.float64)])
    runners = {"hierq": Runner(pot, DT, N, q0, h_q, L, per_call, window["hierq"]),
               "hier": Runner(P.HierarchicalGLM(**kw), DT, N, q0, h, L, per_call, window["hier"]),
               "plugin": Runner(CustomPotential(DT, HIERQ_LOGISTIC_SOURCE, prm), DT, N, q0, h_q, L, per_call, window["plugin"])}
    for r in runners.values():
        r.go(warm)
    torch.cuda.synchronize()
    series = {k: [] for k in runners}
    for i in range(repeats):
        for k, r in runners.items():   # alternating
            series[k].append(r.timed())
            print(f"# {name} repeat {i} {k}: {series[k][-1]:.4f} s", flush=True)
    DP = glm.padded_dim(DT)
    grads = L + 1
    out = dict(shape=name, M=M, D=D, J=J, state_dimension=DT, DP=DP, chains=N, L=L, h=dict(hierq=h_q, hier=h, plugin=h_q),
               penalty="RW2 on every group", penalty_rank=[int(r) for r in pot.penalty_rank],
               iterations_per_call=per_call, iterations_per_window=dict(window), repeats=repeats, warmup_iterations=warm,
               timing="host clock over whole windows of pbbi_hmc_run calls (synchronised before and after)",
               accept_rate={k: 1.0 - float(r.rej.float().mean().item()) for k, r in runners.items()})
    per_it = {}
    for k, ts in series.items():
        out[k + "_seconds"] = ts
        out[k + "_step_chain_per_s"] = [window[k] * L * N / t_ for t_ in ts]
        per_it[k] = np.array(ts) / window[k]          # seconds per iteration
    flop_it = (4.0 * M * DP + 2.0 * DP * DP) * grads * N
    out["hierq_executed_tflops"] = [flop_it / t_ / 1e12 for t_ in per_it["hierq"]]
    out["hierq_share_of_fp64_mfma_peak_executed"] = float(flop_it / np.median(per_it["hierq"]) / PEAK_F64_MFMA)
    out["ratio_median"] = float(np.median(per_it["plugin"]) / np.median(per_it["hierq"]))
    out["ratio_worst_case"] = float(per_it["plugin"].min() / per_it["hierq"].max())  # fastest plugin over slowest kernel
    out["slowest_hierq_beats_fastest_plugin"] = bool(per_it["hierq"].max() < per_it["plugin"].min())
    out["hierq_over_hier_median"] = float(np.median(per_it["hierq"]) / np.median(per_it["hier"]))
    out["hierq_over_hier_range"] = [float(per_it["hierq"].min() / per_it["hier"].max()), float(per_it["hierq"].max() / per_it["hier"].min())]
    out["hierq_over_hier_predicted_by_mfma_count"] = 1.0 + DP / (2.0 * M)   # (DP^2 / 64) / (M DP / 32) more MFMAs per gradient
    return out


class Runner:
    def __init__(self, pot, D, N, q0, h, L, K, window=None):
        # K: slabs of the sample / reject buffers = the most iterations one pbbi_hmc_run call may record;
        # window: iterations per timed window (default K: one call)
        self.pot, self.D, self.N, self.h, self.L, self.K = pot, D, N, h, L, K
        self.window = K if window is None else window
        self.q0 = torch.from_numpy(q0).to("cuda")
        self.q = self.q0.clone()
        self.samples = torch.empty((K, D, N), dtype=torch.float64, device="cuda")
        self.rej = torch.empty((K, N), dtype=torch.uint8, device="cuda")
        self.it = 0

    def go(self, S):
        """S iterations, in calls of at most K: iteration i of a call is written to slab i of the K-slab buffers."""
        st = torch.cuda.current_stream().cuda_stream
        while S > 0:
            n = min(S, self.K)
            _lib.call("pbbi_hmc_run", self.pot.handle, _lib.LEAPFROG, self.q.data_ptr(), None, self.samples.data_ptr(),
                      None, self.rej.data_ptr(), None, self.N, self.N, self.h, self.L, n, _lib.COMPAT_P_FROM_OLDQ, 7,
                      self.it, 0, 1.0, st)
            self.it += n
            S -= n

    def timed(self):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.go(self.window)
        torch.cuda.synchronize()
        return time.perf_counter() - t0


def pointwise_torch(X, y, sdn, chunk):
    """The baseline of --model pointwise: the same four (M,) vectors from torch ops on the same device -- matmul over chunks
    of `chunk` draws (an M x chunk matrix at a time), the logistic link elementwise, logsumexp / mean / var over the draws
    of a chunk, the chunks merged at the end (Chan's formula on the (chunks, M) stacks; every chunk has as many draws)."""
    S, D, N = sdn.shape
    parts = []
    for s in range(S):
        for n0 in range(0, N, chunk):
            eta = X @ sdn[s, :, n0:n0 + chunk]
            ll = y[:, None] * eta - torch.nn.functional.softplus(eta)
            parts.append((torch.logsumexp(ll, dim=1), ll.mean(dim=1), ll.var(dim=1, unbiased=False) * ll.shape[1],
                          torch.sigmoid(eta).mean(dim=1)))
    n = min(chunk, N)
    lse, mean, m2, mu = (torch.stack(v) for v in zip(*parts))
    grand = mean.mean(dim=0)
    M2 = m2.sum(dim=0) + n * ((mean - grand) ** 2).sum(dim=0)
    return torch.logsumexp(lse, dim=0), grand, M2 / (len(parts) * n - 1), mu.mean(dim=0)


def bench_pointwise(name, M, D, N, S, repeats, warm):
    """pbbi_pointwise_glm against pointwise_torch on S slabs of N draws of the plain logistic model, alternating in one
    process; both sides produce lse, mean, var and mu of all M observations over all S * N draws."""
    from physicsbasedbayesianinference_amd import _device
    X, y, w, rs = problem(M, D)
    pot = P.GLM(X, y)
    sdn = torch.from_numpy(np.ascontiguousarray(w[None, :, None] + 0.3 * rs.standard_normal((S, D, N)))).to("cuda:0")
    Xd, yd = torch.from_numpy(X).to("cuda:0"), torch.from_numpy(y).to("cuda:0")
    chunk = N
    while M * chunk > 2 ** 25 and chunk % 2 == 0:     # an M x chunk matrix of at most 256 MiB (N is a power of two)
        chunk //= 2
    out = torch.empty((4, M), dtype=torch.float64, device="cuda:0")
    st = _device.stream_ptr(0)

    def kernel():
        _lib.call("pbbi_pointwise_glm", pot.handle, sdn.data_ptr(), S, D, N, 0, out[0].data_ptr(), out[1].data_ptr(),
                  out[2].data_ptr(), out[3].data_ptr(), st)
        return out

    def baseline():
        return pointwise_torch(Xd, yd, sdn, chunk)

    sides = {"kernel": kernel, "torch": baseline}
    for _ in range(warm):
        got = [torch.stack(list(f())).cpu().numpy() for f in sides.values()]
    agree = float(np.max(np.abs(got[0] - got[1]) / np.maximum(1.0, np.abs(got[1]))))
    series = {k: [] for k in sides}
    for i in range(repeats):
        for k, f in sides.items():   # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            series[k].append(time.perf_counter() - t0)
            print(f"# {name} repeat {i} {k}: {series[k][-1]:.5f} s", flush=True)
    tk, tt = np.array(series["kernel"]), np.array(series["torch"])
    DP, T = glm.padded_dim(D), S * N
    return dict(shape=name, M=M, D=D, DP=DP, slabs=S, chains=N, draws=T, torch_chunk=chunk, kernel_seconds=series["kernel"],
                torch_seconds=series["torch"], kernel_values_per_s=float(M * T / np.median(tk)),
                kernel_executed_tflops=float(2.0 * M * DP * T / np.median(tk) / 1e12),
                ratio_median=float(np.median(tt) / np.median(tk)), ratio_worst_case=float(tt.min() / tk.max()),
                max_rel_difference_kernel_vs_torch=agree)


def loglik_torch(X, y, sdn, chunk):
    """The baseline of --model loglik: the same (S, N) vector from torch ops on the same device -- matmul over chunks of
    `chunk` draws (an M x chunk matrix at a time), the logistic link elementwise, a sum over the observations."""
    S, D, N = sdn.shape
    out = torch.empty((S, N), dtype=torch.float64, device=sdn.device)
    for s in range(S):
        for n0 in range(0, N, chunk):
            eta = X @ sdn[s, :, n0:n0 + chunk]
            out[s, n0:n0 + chunk] = (torch.nn.functional.softplus(eta) - y[:, None] * eta).sum(dim=0)
    return out


def bench_loglik(name, M, D, N, S, repeats, warm):
    """pbbi_loglik_glm (both launches, ranges = 0) against loglik_torch on S slabs of N draws of the plain logistic model,
    alternating in one process; both sides produce the likelihood energy of all S * N draws.  A timed window is several calls
    (at least a quarter of a second) and one synchronisation; times are per call."""
    from physicsbasedbayesianinference_amd import _device
    X, y, w, rs = problem(M, D)
    pot = P.GLM(X, y)
    sdn = torch.from_numpy(np.ascontiguousarray(w[None, :, None] + 0.3 * rs.standard_normal((S, D, N)))).to("cuda:0")
    Xd, yd = torch.from_numpy(X).to("cuda:0"), torch.from_numpy(y).to("cuda:0")
    chunk = N
    while M * chunk > 2 ** 25 and chunk % 2 == 0:     # an M x chunk matrix of at most 256 MiB (N is a power of two)
        chunk //= 2
    out = torch.empty((S, N), dtype=torch.float64, device="cuda:0")
    st = _device.stream_ptr(0)

    def kernel():
        _lib.call("pbbi_loglik_glm", pot.handle, sdn.data_ptr(), S, D, N, 0, out.data_ptr(), st)
        return out

    def baseline():
        return loglik_torch(Xd, yd, sdn, chunk)

    sides = {"kernel": kernel, "torch": baseline}
    for _ in range(warm):
        got = [f().cpu().numpy() for f in sides.values()]
    agree = float(np.max(np.abs(got[0] - got[1])) / max(1.0, float(np.max(np.abs(got[1])))))
    # one call is a millisecond or ten: a timed window is `calls` calls back to back and one synchronisation, at least a
    # quarter of a second of the faster side (sized from one timed call after the warm-up); the seconds recorded are per call
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kernel()
    torch.cuda.synchronize()
    calls = max(1, int(np.ceil(0.25 / (time.perf_counter() - t0))))
    series = {k: [] for k in sides}
    for i in range(repeats):
        for k, f in sides.items():   # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                f()
            torch.cuda.synchronize()
            series[k].append((time.perf_counter() - t0) / calls)
            print(f"# {name} repeat {i} {k}: {series[k][-1]:.6f} s per call ({calls} calls)", flush=True)
    tk, tt = np.array(series["kernel"]), np.array(series["torch"])
    DP, T = glm.padded_dim(D), S * N
    # (the rates are over CALL time: both launches and the stream-ordered allocation and release of the partials, not kernel time)
    return dict(shape=name, M=M, D=D, DP=DP, slabs=S, chains=N, draws=T, torch_chunk=chunk, calls_per_window=calls,
                kernel_seconds=series["kernel"],
                torch_seconds=series["torch"], kernel_median_seconds=float(np.median(tk)), torch_median_seconds=float(np.median(tt)),
                kernel_range_seconds=[float(tk.min()), float(tk.max())], torch_range_seconds=[float(tt.min()), float(tt.max())],
                kernel_values_per_s_over_call_time=float(M * T / np.median(tk)),
                kernel_executed_tflops_over_call_time=float(2.0 * M * DP * T / np.median(tk) / 1e12),
                ratio_median=float(np.median(tt) / np.median(tk)), ratio_worst_case=float(tt.min() / tk.max()),
                max_rel_difference_kernel_vs_torch=agree)


def predictive_torch(X, y, sdn, chunk, centre, cut):
    """The baseline of --model predictive: the same seven per-draw statistics from torch ops on the same device -- matmul over
    chunks of `chunk` draws (an M x chunk matrix at a time), torch.poisson for the replicates, the Poisson log density of the
    replicates and of y elementwise, reductions over the observations."""
    S, D, N = sdn.shape
    out = torch.empty((7, S, N), dtype=torch.float64, device=sdn.device)
    lgy = torch.lgamma(y + 1.0)[:, None]
    for s in range(S):
        for n0 in range(0, N, chunk):
            eta = X @ sdn[s, :, n0:n0 + chunk]
            mu = eta.exp()
            rep = torch.poisson(mu)
            d = rep - centre
            o = out[:, s, n0:n0 + chunk]
            o[0], o[1], o[2], o[3] = d.sum(dim=0), (d * d).sum(dim=0), rep.amin(dim=0), rep.amax(dim=0)
            o[4] = (rep <= cut).sum(dim=0)
            o[5] = (rep * eta - mu - torch.lgamma(rep + 1.0)).sum(dim=0)
            o[6] = (y[:, None] * eta - mu - lgy).sum(dim=0)
    return out


def bench_predictive(name, M, D, N, S, repeats, warm):
    """pbbi_predictive_glm (both launches, ranges = 0, no yrep_out) against predictive_torch on S slabs of N draws of the plain
    Poisson model, alternating in one process after `warm` calls of each; both sides produce the seven statistics of all S * N
    draws.  A timed window is several calls (at least a quarter of a second) and one synchronisation; times are per call.  The
    replicates differ (two generators), so the sides are held together by statistic 6, which draws nothing, and by the means of
    statistic 0 over all draws.  `kernel_ns_per_value_by_mean_shift`: the kernel alone with every mean multiplied by exp(shift) --
    what the O(sigma) walk of the inversion costs as the means grow."""
    from physicsbasedbayesianinference_amd import _device
    rs = np.random.RandomState(0)
    X = rs.standard_normal((M, D)) / np.sqrt(D)
    w = 0.5 * rs.standard_normal(D)
    y = rs.poisson(np.exp(X @ w + 1.0)).astype(np.float64)
    X = np.ascontiguousarray(np.c_[X[:, :D - 1], np.ones(M)])      # the last column an intercept; its coefficient 1
    w[D - 1] = 1.0
    pot = P.GLM(X, y, family="poisson")
    sdn = torch.from_numpy(np.ascontiguousarray(w[None, :, None] + 0.1 * rs.standard_normal((S, D, N)))).to("cuda:0")
    Xd, yd = torch.from_numpy(X).to("cuda:0"), torch.from_numpy(y).to("cuda:0")
    chunk = N
    while M * chunk > 2 ** 25 and chunk % 2 == 0:     # an M x chunk matrix of at most 256 MiB (N is a power of two)
        chunk //= 2
    T, centre, cut = S * N, float(y.mean()), 0.0
    aux = torch.from_numpy(glm._predictive_aux(pot)[0]).to("cuda:0")
    out = torch.empty((7, T), dtype=torch.float64, device="cuda:0")
    st = _device.stream_ptr(0)

    def kernel(draws=sdn):
        _lib.call("pbbi_predictive_glm", pot.handle, draws.data_ptr(), S, D, N, 1, aux.data_ptr(), centre, cut, 0, out.data_ptr(),
                  0, None, st)
        return out

    def baseline():
        return predictive_torch(Xd, yd, sdn, chunk, centre, cut).reshape(7, T)

    def window(f, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls

    sides = {"kernel": kernel, "torch": baseline}
    for _ in range(warm):
        got = [f().cpu().numpy() for f in sides.values()]
    agree = float(np.max(np.abs(got[0][6] - got[1][6])) / max(1.0, float(np.max(np.abs(got[1][6])))))
    mean_rep = [float(centre + g[0].mean() / M) for g in got]
    calls = max(1, int(np.ceil(0.25 / window(kernel, 1))))
    series = {k: [] for k in sides}
    for i in range(repeats):
        for k, f in sides.items():   # alternating
            series[k].append(window(f, calls))
            print(f"# {name} repeat {i} {k}: {series[k][-1]:.6f} s per call ({calls} calls)", flush=True)
    tk, tt = np.array(series["kernel"]), np.array(series["torch"])
    eta_max = float((Xd @ sdn[0]).max().item())
    by_shift = {}
    for shift in (0.0, 2.0, 4.0, 8.0):      # the intercept's coefficient moved: means times 1, 7.4, 55, 2981
        moved = sdn.clone()
        moved[:, D - 1, :] += shift
        kernel(moved)
        ts = [window(lambda: kernel(moved), max(1, calls // 4)) for _ in range(3)]
        by_shift["%g" % shift] = dict(largest_fitted_mean=float(np.exp(eta_max + shift)), ns_per_value=float(np.median(ts) / (M * T) * 1e9),
                                      nan_draws=int(torch.isnan(out[0]).sum().item()))
    return dict(shape=name, family="poisson", M=M, D=D, DP=glm.padded_dim(D), slabs=S, chains=N, draws=T, torch_chunk=chunk,
                calls_per_window=calls, kernel_seconds=series["kernel"], torch_seconds=series["torch"],
                kernel_median_seconds=float(np.median(tk)), torch_median_seconds=float(np.median(tt)),
                kernel_range_seconds=[float(tk.min()), float(tk.max())], torch_range_seconds=[float(tt.min()), float(tt.max())],
                kernel_ns_per_value=float(np.median(tk) / (M * T) * 1e9), torch_ns_per_value=float(np.median(tt) / (M * T) * 1e9),
                largest_fitted_mean=float(np.exp(eta_max)), kernel_ns_per_value_by_mean_shift=by_shift,
                ratio_median=float(np.median(tt) / np.median(tk)), ratio_worst_case=float(tt.min() / tk.max()),
                mean_replicate_kernel_and_torch=mean_rep, max_rel_difference_loglik_obs_kernel_vs_torch=agree)


def bench_shape(name, M, D, N, h, L, K, repeats, warm, glm_only):
    X, y, w, rs = problem(M, D)
    q0 = np.ascontiguousarray(w[:, None] + 0.3 * rs.standard_normal((D, N)))
    runners = {"glm": Runner(P.GLM(X, y), D, N, q0, h, L, K)}
    if not glm_only:
        runners["plugin"] = Runner(logistic_regression_posterior(X, y), D, N, q0, h, L, K)
    for r in runners.values():
        r.go(warm)
    torch.cuda.synchronize()
    series = {k: [] for k in runners}
    for i in range(repeats):
        for k, r in runners.items():   # alternating
            series[k].append(r.timed())
            print(f"# {name} repeat {i} {k}: {series[k][-1]:.4f} s", flush=True)
    DP = glm.padded_dim(D)
    grads = L + 1                       # per iteration and chain: g(q_0) and one per step
    out = dict(shape=name, M=M, D=D, DP=DP, chains=N, L=L, K=K, h=h,
               accept_rate={k: 1.0 - float(r.rej.float().mean().item()) for k, r in runners.items()})
    for k, ts in series.items():
        out[k + "_seconds"] = ts
        out[k + "_step_chain_per_s"] = [K * L * N / t for t in ts]
    tg = np.array(series["glm"])
    out["glm_executed_tflops"] = [4.0 * M * DP * grads * N * K / t / 1e12 for t in tg]
    out["glm_algorithmic_tflops"] = [4.0 * M * D * grads * N * K / t / 1e12 for t in tg]
    out["glm_share_of_fp64_mfma_peak_executed"] = float(4.0 * M * DP * grads * N * K / np.median(tg) / PEAK_F64_MFMA)
    out["glm_share_of_fp64_mfma_peak_algorithmic"] = float(4.0 * M * D * grads * N * K / np.median(tg) / PEAK_F64_MFMA)
    if "plugin" in series:
        tp = np.array(series["plugin"])
        out["ratio_median"] = float(np.median(tp) / np.median(tg))
        out["ratio_worst_case"] = float(tp.min() / tg.max())   # fastest plugin repeat over slowest GLM repeat
        out["slowest_glm_beats_fastest_plugin"] = bool(tg.max() < tp.min())
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all")
    ap.add_argument("--K", type=int, default=None, help="iterations per window (default 32; --model softmax: per shape)")
    ap.add_argument("--L", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=None, help="default 5 (--model softmax: per shape)")
    ap.add_argument("--warmup", type=int, default=None, help="default 4 (--model softmax: per shape)")
    ap.add_argument("--glm-only", action="store_true")
    ap.add_argument("--model", default="plain", choices=["plain", "rich", "softmax", "dispersion", "gamma", "hier", "hierq", "hierdisp",
                                                         "pointwise", "loglik", "predictive", "ordinal", "logistic"])
    ap.add_argument("--baseline", default=None, help="--model ordinal: the output file of --model logistic run on another build "
                                                     "of the library (the parent commit's), merged into the record")
    ap.add_argument("--build", default=None, help="--model logistic: a name for the build measured, kept in the record")
    ap.add_argument("--slabs", type=int, default=8, help="--model pointwise / loglik / predictive: slabs of N draws")
    ap.add_argument("--parametrisation", default="centred", choices=["centred", "noncentred"],
                    help="--model hier: noncentred times the non-centred kernel against the centred one and the plugin")
    ap.add_argument("--custom", action="store_true", help="--model rich: also the full model as a CustomPotential")
    ap.add_argument("--label", default="rich_vs_plain", help="--model rich: key of the record in the output file")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.model in ("pointwise", "loglik", "predictive"):
        bench_pw = {"pointwise": bench_pointwise, "loglik": bench_loglik, "predictive": bench_predictive}[a.model]
        a.out = a.out or os.path.join(ROOT, "profiles", "glm_%s_bench.json" % a.model)
        names = list(SHAPES) if a.shape == "all" else [a.shape]
        results = []
        if os.path.exists(a.out) and a.shape != "all":   # one shape per call: keep the other's record
            with open(a.out) as f:
                results = [r for r in json.load(f)["results"] if r["shape"] not in names]
        for n in names:
            sh = SHAPES[n]
            res = bench_pw(n, sh["M"], sh["D"], sh["N"], a.slabs, 5 if a.repeats is None else a.repeats,
                           2 if a.warmup is None else a.warmup)
            print(json.dumps(res))
            results.append(res)
            with open(a.out, "w") as f:
                json.dump(dict(device=_lib.device_info(0)["name"], peak_fp64_mfma_flops=PEAK_F64_MFMA,
                               results=sorted(results, key=lambda r: r["shape"], reverse=True)), f, indent=1)
                f.write("\n")
        sys.exit(0)
    if a.model in ("softmax", "dispersion", "gamma", "hier", "hierq", "hierdisp", "ordinal", "logistic"):
        table, fn, side = {"softmax": (SOFTMAX_SHAPES, bench_softmax, "softmax"),
                           "dispersion": (DISPERSION_SHAPES, bench_dispersion, "dispersion"),
                           "gamma": (DISPERSION_SHAPES, bench_gamma, "gamma"),
                           "ordinal": (DISPERSION_SHAPES, bench_ordinal, "ordinal"),
                           "logistic": (DISPERSION_SHAPES, bench_ordinal, "logistic"),
                           "hier": (HIER_SHAPES, bench_hier, "hier"),
                           "hierq": (HIERQ_SHAPES, bench_hierq, "hierq"),
                           "hierdisp": (HIER_DISP_SHAPES, bench_hier_dispersion, "centred")}[a.model]
        stem = {"hierq": "hier_penalty", "hierdisp": "hier_dispersion"}.get(a.model, a.model)
        if a.model == "hier" and a.parametrisation == "noncentred":
            table, fn, side, stem = HIER_NC_SHAPES, bench_hier_nc, "noncentred", "hier_nc"
        a.out = a.out or os.path.join(ROOT, "profiles", "glm_%s_bench.json" % stem)
        names = [n for n in table if n != "mid"] if a.shape == "all" else [a.shape]
        results = []
        if os.path.exists(a.out) and a.shape != "all":   # one shape per call: keep the others' records
            with open(a.out) as f:
                results = [r for r in json.load(f)["results"] if r["shape"] not in names]
        for n in names:
            cfg = dict(table[n])
            if a.K is not None:        # one window length for both sides, one call per window
                cfg["per_call"], cfg["window"] = a.K, {k: a.K for k in cfg["window"]}
            if a.repeats is not None:
                cfg["repeats"] = a.repeats
            if a.warmup is not None:
                cfg["warm"] = a.warmup
            if a.model == "logistic":
                cfg["sides"] = ("logistic",)
            if a.model == "ordinal" and a.baseline:
                with open(a.baseline) as f:
                    cfg["baseline"] = [r for r in json.load(f)["results"] if r["shape"] == n][0]
            res = fn(n, L=a.L, **cfg)
            if a.model == "logistic" and a.build:
                res["build"] = a.build
            print(json.dumps(res))
            results.append(res)
            with open(a.out, "w") as f:
                json.dump(dict(device=_lib.device_info(0)["name"], peak_fp64_mfma_flops=PEAK_F64_MFMA,
                               results=sorted(results, key=lambda r: r["shape"])), f, indent=1)
                f.write("\n")
        sys.exit(0)
    a.K = 32 if a.K is None else a.K
    a.repeats = 5 if a.repeats is None else a.repeats
    a.warmup = 4 if a.warmup is None else a.warmup
    names = list(SHAPES) if a.shape == "all" else [a.shape]
    if a.model == "rich":
        a.out = a.out or os.path.join(ROOT, "profiles", "glm_model_bench.json")
        doc = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                doc = json.load(f)
        doc["device"] = _lib.device_info(0)["name"]
        rec = {r["shape"]: r for r in doc.get(a.label, [])}
        for n in names:
            res = bench_rich(n, L=a.L, K=a.K, repeats=a.repeats, warm=a.warmup, custom=a.custom, **SHAPES[n])
            print(json.dumps(res))
            rec[n] = res
            doc[a.label] = [rec[k] for k in sorted(rec, reverse=True)]
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")
        sys.exit(0)
    a.out = a.out or os.path.join(ROOT, "profiles", "glm_bench.json")
    results = []
    if os.path.exists(a.out) and a.shape != "all":   # one shape per call: keep the other's record
        with open(a.out) as f:
            results = [r for r in json.load(f)["results"] if r["shape"] not in names]
    for n in names:
        res = bench_shape(n, L=a.L, K=a.K, repeats=a.repeats, warm=a.warmup, glm_only=a.glm_only, **SHAPES[n])
        print(json.dumps(res))
        results.append(res)
        with open(a.out, "w") as f:
            json.dump(dict(device=_lib.device_info(0)["name"], peak_fp64_mfma_flops=PEAK_F64_MFMA,
                           results=sorted(results, key=lambda r: r["shape"], reverse=True)), f, indent=1)
            f.write("\n")
