#!/usr/bin/env python3
"""Time one pbbi_glm_hessian call (k_glm_hess + k_glm_hess_merge) at M = 10^6 observations and D = 16, 64, 128 against
X.T @ (h[:, None] * X) in fp64 torch on the same device, and write both to profiles/glm_hessian_time.txt.

usage: python tools/time_glm_hessian.py [--M 1000000] [--reps 30] [--out profiles/glm_hessian_time.txt]

Needs a GPU: there is no host path.  Each figure is the mean of `reps` back-to-back calls between two device events after
`warmup` calls of the same shape (the window is a few hundred ms per shape), taken twice, alternating the two sides, so the
spread between the two takes shows beside the figure.  The flop count is the algorithm's, M * D^2 multiply-adds = 2 M D^2 (the
library forms only the upper tiles, torch a full GEMM; both are charged the full product).  The torch side is given h
ready-made; the library's time includes forming eta and h from the design image.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glm_hessian_time.txt"))
    args = ap.parse_args()
    import torch
    from physicsbasedbayesianinference_amd import GLM, _lib
    from physicsbasedbayesianinference_amd._device import stream_ptr
    if not torch.cuda.is_available():
        raise SystemExit("time_glm_hessian.py needs a GPU")
    M = args.M
    lines = ["pbbi_glm_hessian (logistic, full model, ranges = 0) against torch X.T @ (h[:, None] * X), fp64, M = %d, device %s"
             % (M, _lib.device_info(0)["name"]),
             "ms per call: mean of %d calls between device events after %d warm-up calls; two takes each, alternating" % (
                 args.reps, args.warmup),
             "%5s %22s %22s %14s %14s %12s" % ("D", "library ms (take 1, 2)", "torch ms (take 1, 2)", "library TF/s", "torch TF/s",
                                              "max rel diff")]

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.reps

    for D in (16, 64, 128):
        rs = np.random.RandomState(D)
        X = rs.standard_normal((M, D)) / np.sqrt(D)
        w = rs.standard_normal(D)
        y = (rs.uniform(size=M) < 1 / (1 + np.exp(-(X @ w)))).astype(float)
        pot = GLM(X, y, "logistic", prior_precision=1.0, weights=np.ones(M))
        dev = torch.device("cuda", pot.device)
        qd = torch.from_numpy(w).to(dev)
        out = torch.empty((D, D), dtype=torch.float64, device=dev)
        st = stream_ptr(pot.device)
        Xd = torch.from_numpy(X).to(dev)
        s = torch.sigmoid(Xd @ qd)
        hd = s * (1 - s)
        ref = [None]

        def lib():
            _lib.call("pbbi_glm_hessian", pot.handle, qd.data_ptr(), 0, out.data_ptr(), st)

        def tor():
            ref[0] = Xd.T @ (hd[:, None] * Xd)

        t_lib, t_tor = [], []
        for _ in range(2):
            t_lib.append(timed(lib))
            t_tor.append(timed(tor))
        diff = float(((out - torch.eye(D, dtype=torch.float64, device=dev) - ref[0]).abs().max() / ref[0].abs().max()).item())
        flops = 2.0 * M * D * D
        lines.append("%5d %22s %22s %14.2f %14.2f %12.2e" % (D, "%.3f, %.3f" % tuple(t_lib), "%.3f, %.3f" % tuple(t_tor),
                                                             flops / (min(t_lib) * 1e-3) / 1e12, flops / (min(t_tor) * 1e-3) / 1e12,
                                                             diff))
        print(lines[-1], flush=True)
        del pot, Xd, hd, s
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
