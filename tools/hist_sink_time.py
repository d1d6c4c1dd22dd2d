"""What the running histogram sink (stats.RunningHistogram, csrc/kernels_hist.hip) costs, one GPU.

Config C2 (dense-precision Gaussian, D = 128, 65 536 chains, fp64, L = 10), two measurements:

  1. the bare `update` on a resident chunk of c = 50 draws (c D N 8 bytes = 3.36 GB): seconds per call (median of
     `repeats` groups of `calls` back-to-back calls) and GB/s of the slab, beside the 8 TB/s DESIGN.md 4.8 reckons with.
     Three fillings of the same slab: Gaussian draws (the range covers them, as from_moments would set it), the same
     with the range from the first chunk (`margin` = 1: the draws sit in the middle third of the bins), and a constant
     (every lane of every wave adds to ONE counter);
  2. HMC.sampleStats(max_lag=0) with and without hist=, alternating in ONE process, `repeats` times each after warming
     both: the share of the run the sink costs.

Writes profiles/hist_sink_time.json.

usage: tools/hist_sink_time.py [--iterations 1000] [--chunk 50] [--repeats 3] [--calls 5] [--chains 65536] [--dim 128]
                               [--bins 2048] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from scipy.constants import k as kB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import physicsbasedbayesianinference_amd as P  # noqa: E402
from physicsbasedbayesianinference_amd import _lib  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def precision_matrix(d):
    A = np.random.RandomState(0).standard_normal((d, d))
    Pm = np.linalg.inv(A @ A.T / d + np.eye(d))
    return 0.5 * (Pm + Pm.T)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def bare_update(label, slab, make, repeats, calls):
    """Seconds per update of `slab` into the histogram make() returns (started by one update that is not timed)."""
    h = make().update(slab)
    per_call = []
    for _ in range(repeats):
        t, _ = timed(lambda: [h.update(slab) for _ in range(calls)])
        per_call.append(t / calls)
    med = float(np.median(per_call))
    nbytes = slab.numel() * slab.element_size()
    res = dict(filling=label, seconds_per_update=per_call, median_s=med, slab_bytes=nbytes, slab_GBps=nbytes / med / 1e9,
               fraction_of_8TBps=nbytes / med / HBM_BYTES_PER_S, ms_at_8TBps=nbytes / HBM_BYTES_PER_S * 1e3)
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--bins", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hist_sink_time.json"))
    a = ap.parse_args()
    D, N, S, c, bins = a.dim, a.chains, a.iterations, a.chunk, a.bins
    record = dict(device=_lib.device_info(0)["name"], hbm_bytes_per_s_assumed=HBM_BYTES_PER_S, D=D, chains=N, chunk=c,
                  bins=bins)

    # 1. the bare update on a resident chunk
    slab = torch.empty((c, D, N), dtype=torch.float64, device="cuda")
    slab.normal_(generator=torch.Generator(device="cuda").manual_seed(1))
    covered = lambda: P.RunningHistogram.from_moments(np.zeros(D), np.ones(D), N, width=6.0, bins=bins, device=0)
    auto = lambda: P.RunningHistogram(D, N, bins=bins, device=0)
    bare = [bare_update("gaussian, range of 6 sigma either side", slab, covered, a.repeats, a.calls),
            bare_update("gaussian, range from the first chunk (margin 1)", slab, auto, a.repeats, a.calls)]
    slab.fill_(2.5)
    bare.append(bare_update("constant (one counter per dimension)", slab, auto, a.repeats, a.calls))
    record["bare_update"] = bare
    del slab
    torch.cuda.empty_cache()

    # 2. the share of a run
    pot = P.GaussianDense(None, precision=precision_matrix(D), const=0.0)
    hmc = P.HMC(P.Ensemble(D, N), 1.0, 0.1, None, potential=pot, rng="philox", seed=1, verbose=False)
    T0, qStd = 1 / kB, 1.0
    new_hist = lambda: P.RunningHistogram(D, N, bins=bins, device=0)
    with_hist = lambda n: hmc.sampleStats(n, c, T0, qStd, max_lag=0, seed=1, hist=new_hist())
    without = lambda n: hmc.sampleStats(n, c, T0, qStd, max_lag=0, seed=1)
    timed(lambda: with_hist(2 * c))                                             # warm both (code objects, pool)
    timed(lambda: without(2 * c))
    series = dict(hist=[], plain=[])
    for i in range(a.repeats):                                                  # alternating
        t, _ = timed(lambda: with_hist(S))
        series["hist"].append(t)
        rate_hist = hmc.acceptRate
        t, _ = timed(lambda: without(S))
        series["plain"].append(t)
        print(f"# repeat {i}: with hist {series['hist'][-1]:.4f} s, without {series['plain'][-1]:.4f} s", flush=True)
        assert rate_hist == hmc.acceptRate                                      # the same draws
    hist_s, plain_s = float(np.median(series["hist"])), float(np.median(series["plain"]))
    chunks = -(-S // c)
    record["sample_stats"] = dict(iterations=S, max_lag=0, with_hist_seconds=series["hist"], without_seconds=series["plain"],
                                  with_hist_median_s=hist_s, without_median_s=plain_s,
                                  share_of_the_run=(hist_s - plain_s) / hist_s, overhead_fraction=hist_s / plain_s - 1.0,
                                  overhead_ms_per_chunk=(hist_s - plain_s) / chunks * 1e3,
                                  run_ms_per_chunk_without=plain_s / chunks * 1e3, accept_rate=rate_hist)
    print(json.dumps(record["sample_stats"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
