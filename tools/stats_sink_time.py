"""What the running statistics sink (stats.RunningStats, csrc/kernels_stats.hip) costs a long run, one GPU.

Config C2 (dense-precision Gaussian, D = 128, 65 536 chains, fp64, L = 10): 1000 iterations in chunks of 50 through
HMC.sampleStats, against the same loop -- one pbbi_hmc_run per chunk into one reused slab, the reject count summed on
the device, one read-back at the end -- without the sink.  The two alternate in ONE process, `repeats` times each after
warming both, for max_lag 0, 8 and 32.  Next to the measured overhead the record holds the byte model: a chunk moves
its slab once (c D N 8 bytes) for the per-chain pass and the per-chain state about (4 T + 6) D N 8 bytes; the D x D
tile sums read the slab again per tile pair.  Writes profiles/stats_sink_time.json.

usage: tools/stats_sink_time.py [--iterations 1000] [--chunk 50] [--lags 0,8,32] [--repeats 3] [--chains 65536]
                                [--dim 128] [--out FILE]
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
from physicsbasedbayesianinference_amd._device import empty, stream_ptr  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def precision_matrix(d):
    A = np.random.RandomState(0).standard_normal((d, d))
    Pm = np.linalg.inv(A @ A.T / d + np.eye(d))
    return 0.5 * (Pm + Pm.T)


def run_without_sink(hmc, S, chunk, temperature, qStd, seed=1):
    """sampleStats' loop with the accumulation taken out."""
    pot, ens = hmc._pot, hmc.ensemble
    D, N = ens.numDimensions, ens.numParticles
    dev, st = pot.device, stream_ptr(pot.device)
    md = hmc._mass()
    mptr = md.data_ptr() if md is not None else None
    q = empty((D, N), pot.dtype, dev)
    _lib.call("pbbi_philox_normal", seed, hmc._position_stream(), 0, 0, D, N, N, float(qStd), None, pot._dt, dev,
              q.data_ptr(), st)
    samples, reject = empty((chunk, D, N), pot.dtype, dev), empty((chunk, N), np.uint8, dev)
    n_rej, done = None, 0
    while done < S:
        c = min(chunk, S - done)
        _lib.call("pbbi_hmc_run", pot.handle, hmc.integrator.method_id, q.data_ptr(), mptr, samples.data_ptr(), None,
                  reject.data_ptr(), None, N, N, float(hmc.stepSize), hmc.integrator.numSteps, c, hmc._flags(), seed,
                  done, 0, float(kB * temperature), st)
        r = reject[:c].sum(dtype=torch.int64)
        n_rej = r if n_rej is None else n_rej + r
        done += c
    return 1.0 - float(n_rej.item()) / (S * N)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--lags", default="0,8,32")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stats_sink_time.json"))
    a = ap.parse_args()
    D, N, S, c = a.dim, a.chains, a.iterations, a.chunk
    pot = P.GaussianDense(None, precision=precision_matrix(D), const=0.0)
    hmc = P.HMC(P.Ensemble(D, N), 1.0, 0.1, None, potential=pot, rng="philox", seed=1, verbose=False)
    T0, qStd = 1 / kB, 1.0
    results = []
    for T in [int(t) for t in a.lags.split(",")]:
        with_sink = lambda: hmc.sampleStats(S, c, T0, qStd, max_lag=T, seed=1)
        without = lambda: run_without_sink(hmc, S, c, T0, qStd)
        timed(lambda: hmc.sampleStats(2 * c, c, T0, qStd, max_lag=T, seed=1))   # warm both (code objects, pool)
        timed(lambda: run_without_sink(hmc, 2 * c, c, T0, qStd))
        series = dict(sink=[], plain=[])
        for i in range(a.repeats):                                              # alternating
            t, rs = timed(with_sink)
            series["sink"].append(t)
            rate_sink = hmc.acceptRate
            t, rate_plain = timed(without)
            series["plain"].append(t)
            print(f"# max_lag {T} repeat {i}: sink {series['sink'][-1]:.4f} s, plain {series['plain'][-1]:.4f} s", flush=True)
        assert rate_sink == rate_plain, (rate_sink, rate_plain)                 # the same draws
        sink, plain = float(np.median(series["sink"])), float(np.median(series["plain"]))
        chunks = -(-S // c)
        slab, state = c * D * N * 8, (4 * T + 6) * D * N * 8
        tiles = (D + 15) // 16
        cov_reads = tiles * (tiles + 1) // 2 * 2 * 16 * c * N * 8               # every tile pair reads its 2 x 16 rows
        res = dict(max_lag=T, D=D, chains=N, iterations=S, chunk=c, sink_seconds=series["sink"],
                   plain_seconds=series["plain"], sink_median_s=sink, plain_median_s=plain,
                   overhead_fraction=sink / plain - 1.0, overhead_ms_per_chunk=(sink - plain) / chunks * 1e3,
                   sampling_ms_per_chunk=plain / chunks * 1e3, hoped_overhead_fraction=0.05,
                   times_the_hoped_overhead=(sink / plain - 1.0) / 0.05, state_bytes=rs.state_bytes,
                   model=dict(slab_bytes_per_chunk=slab, chain_state_bytes_per_chunk=state,
                              covariance_slab_reads_per_chunk=cov_reads,
                              chain_pass_ms_at_8TBps=(slab + state) / HBM_BYTES_PER_S * 1e3,
                              covariance_ms_at_8TBps_if_from_hbm=cov_reads / HBM_BYTES_PER_S * 1e3),
                   accept_rate=rate_sink, rhat_max=float(rs.rhat().max()),
                   ess_min=float(rs.ess().min()) if S >= 4 else None)
        print(json.dumps(res), flush=True)
        results.append(res)
        del rs
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=_lib.device_info(0)["name"], hbm_bytes_per_s_assumed=HBM_BYTES_PER_S,
                           results=results), f, indent=1)
            f.write("\n")
