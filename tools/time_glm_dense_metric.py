#!/usr/bin/env python3
"""What the dense metric costs a GLM run, and what it buys: tools/time_glm_metric.py's protocol with a third variant.

usage: tools/time_glm_dense_metric.py [--M 4096] [--D 64] [--N 65536] [--L 10] [--S 10] [--reps 9] [--out FILE] [--label NAME]
       tools/time_glm_dense_metric.py --ess [--N 4096] [--S 400] [--out FILE]

Timing: one pbbi_hmc_run (logistic, M x D, N chains, L steps, S iterations) on the same handle with a dense metric (R diag(30^((d +
0.5) / D)) R^T, R random orthogonal), with the diagonal metric 30^((d + 0.5) / D) and without a metric, alternating in one process.
Each timing is a pair of device events around the one call, after a warm-up call of each kind.  Printed (and appended to --out):
one JSON line with the median, minimum and maximum of the `reps` timings of each kind in milliseconds, the run-to-run spread (max
- min over the median) and the ratios of medians.  With PBBI_LIB naming a build without pbbi_potential_set_metric_dense (the
parent commit's) the dense variant is left out, so the same script times that build's two kinds; --label names the build in the
result line ("head" by default, e.g. "parent" for such a run -- never a path).

--ess: a logistic model whose D = 16 columns are pairwise correlated 0.95 (M = 2048); fit = pot.laplace(); then the same budget of
S iterations at simulTime 1.5 under fit.metric and under fit.dense_metric, each after its own adaptStepSize, from fit.sample(N):
the minimum over rows of RunningStats.ess() per gradient evaluation (S N (numSteps + 1) of them).  Needs a GPU: there is no CPU
path."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DENSE_NAMES = ("pbbi_potential_set_metric_dense", "pbbi_potential_get_metric_dense", "pbbi_glm_pack_metric_dense")


def dense_metric(D, seed=3):
    rs = np.random.RandomState(1000 * seed + D)
    R, _ = np.linalg.qr(rs.standard_normal((D, D)))
    M = (R * 30.0 ** ((np.arange(D) + 0.5) / D)) @ R.T
    return 0.5 * (M + M.T)


def load():
    """The package on the library in use; a library without the dense entries is bound without them (and has no dense variant)."""
    import torch  # noqa: F401  (first: the library binds to the HIP runtime torch has loaded)
    import physicsbasedbayesianinference_amd as P
    from physicsbasedbayesianinference_amd import _lib as lib
    has_dense = hasattr(ctypes.CDLL(lib.LIB_PATH), DENSE_NAMES[0])
    if not has_dense:
        for n in DENSE_NAMES:
            lib.PROTOTYPES.pop(n, None)
            lib.HOST_PACKER_PROTOTYPES.pop(n, None)
    lib.load()
    return P, lib, has_dense


def emit(res, out):
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def timing(a):
    import torch
    P, lib, has_dense = load()
    from physicsbasedbayesianinference_amd import _device as d
    rs = np.random.RandomState(3)
    X = rs.standard_normal((a.M, a.D)) / np.sqrt(a.D)
    w = rs.standard_normal(a.D)
    y = (rs.uniform(size=a.M) < 1.0 / (1.0 + np.exp(-X @ w))).astype(np.float64)
    pot = P.GLM(X, y)
    q0 = d.as_device(np.ascontiguousarray(w[:, None] + 0.1 * rs.standard_normal((a.D, a.N))), 0, np.float64)
    reject = d.empty((a.S, a.N), np.uint8, 0)
    diag = 30.0 ** ((np.arange(a.D) + 0.5) / a.D)
    dptr = ctypes.POINTER(ctypes.c_double)

    def set_kind(k):
        lib.call("pbbi_potential_set_metric_diag", pot.handle, None, 0)
        if k == "diag":
            lib.call("pbbi_potential_set_metric_diag", pot.handle, diag.ctypes.data_as(dptr), a.D)
        elif k == "dense":
            m = dense_metric(a.D)
            lib.call("pbbi_potential_set_metric_dense", pot.handle, m.ctypes.data_as(dptr), a.D)

    def run():
        q = q0.clone()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        lib.call("pbbi_hmc_run", pot.handle, lib.LEAPFROG, q.data_ptr(), None, None, None, reject.data_ptr(), None, a.N, a.N,
                 a.h, a.L, a.S, lib.DRAW_F64, 7, 0, 0, 1.0, d.stream_ptr(0))
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), 1.0 - float(reject.float().mean())

    kinds = ["plain", "diag"] + (["dense"] if has_dense else [])
    times, accept = {k: [] for k in kinds}, {}
    for rep in range(-1, a.reps):                       # rep -1: the warm-up of each kind
        for k in kinds:
            set_kind(k)
            ms, acc = run()
            if rep >= 0:
                times[k].append(ms)
            accept[k] = acc

    def summary(v):
        return dict(median=statistics.median(v), min=min(v), max=max(v), spread=(max(v) - min(v)) / statistics.median(v))

    med = {k: statistics.median(times[k]) for k in kinds}
    emit(dict(tool="time_glm_dense_metric", library=a.label or ("PBBI_LIB" if os.environ.get("PBBI_LIB") else "head"), device=torch.cuda.get_device_name(0),
              M=a.M, D=a.D, N=a.N, L=a.L, S=a.S, h=a.h, reps=a.reps, ms={k: summary(times[k]) for k in kinds},
              diag_over_plain=med["diag"] / med["plain"], dense_over_diag=med["dense"] / med["diag"] if has_dense else None,
              dense_over_plain=med["dense"] / med["plain"] if has_dense else None, accept=accept), a.out)


def ess(a):
    import torch
    from scipy.constants import k as kB
    P, lib, has_dense = load()
    D, M, rho = 16, 2048, 0.95
    rs = np.random.RandomState(7)
    cov = np.full((D, D), rho) + (1.0 - rho) * np.eye(D)
    X = rs.standard_normal((M, D)) @ np.linalg.cholesky(cov).T / np.sqrt(D)
    w = rs.standard_normal(D)
    y = (rs.uniform(size=M) < 1.0 / (1.0 + np.exp(-X @ w))).astype(np.float64)
    pot = P.GLM(X, y)
    fit = pot.laplace()
    sd = fit.stderr
    corr = fit.covariance / np.outer(sd, sd)
    res = dict(tool="time_glm_dense_metric --ess", device=torch.cuda.get_device_name(0), M=M, D=D, N=a.N, S=a.S, simulTime=1.5,
               column_correlation=rho, posterior_correlation_max=float(np.max(np.abs(corr - np.eye(D)))),
               hessian_condition=float(np.linalg.cond(fit.hessian)),
               diag_preconditioned_condition=float(np.linalg.cond(fit.hessian / np.sqrt(np.outer(fit.metric, fit.metric)))))
    for kind, metric in (("diag", fit.metric), ("dense", fit.dense_metric)):
        hmc = P.HMC(P.Ensemble(D, a.N), 1.5, 0.1, None, potential=pot, rng="philox", seed=11, verbose=False, compat=False,
                    draw_f64=True)
        hmc.setMassMatrix(metric)
        start = fit.sample(a.N, seed=5)
        h = hmc.adaptStepSize(1 / kB, 1.0, start=start)
        stats = hmc.sampleStats(a.S, 50, 1 / kB, 1.0, burn_in=20, max_lag=32, start=start)
        e = stats.ess()
        grads = a.S * a.N * (hmc.integrator.numSteps + 1)
        res[kind] = dict(step=h, numSteps=int(hmc.integrator.numSteps), accept=hmc.acceptRate, ess_min=float(np.min(e)),
                         ess_max=float(np.max(e)), gradient_evaluations=grads, ess_min_per_gradient=float(np.min(e)) / grads,
                         ess_truncated=bool(np.any(stats.ess_truncated)))
    res["dense_over_diag"] = res["dense"]["ess_min_per_gradient"] / res["diag"]["ess_min_per_gradient"]
    pot.set_metric(None)
    emit(res, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ess", action="store_true")
    ap.add_argument("--M", type=int, default=4096)
    ap.add_argument("--D", type=int, default=64)
    ap.add_argument("--N", type=int, default=None)
    ap.add_argument("--L", type=int, default=10)
    ap.add_argument("--S", type=int, default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--h", type=float, default=0.02)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default=None, help='what the result line calls the library in use ("head"; "parent" with PBBI_LIB)')
    a = ap.parse_args()
    if a.ess:
        a.N, a.S = a.N or 4096, a.S or 400
        ess(a)
    else:
        a.N, a.S = a.N or 65536, a.S or 10
        timing(a)


if __name__ == "__main__":
    main()
