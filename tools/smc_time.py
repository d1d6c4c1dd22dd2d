#!/usr/bin/env python3
"""Timing of tempered SMC at C2's shape: D = 128 dense Gaussian, N = 65 536, moves = 5.

Prints one JSON line: the resample gather's bandwidth at N = 2^20 (bytes 2 D N w + 12 N over the whole
pbbi_smc_resample_systematic call, as a fraction of 8 TB/s), the share of stage time outside pbbi_hmc_run, and the
host syncs per stage (adaptive and fixed schedule).  For per-kernel times run it under
`rocprofv3 --kernel-trace --stats -- python tools/smc_time.py`."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    import physicsbasedbayesianinference_amd as P
    from physicsbasedbayesianinference_amd import _lib
    from physicsbasedbayesianinference_amd._device import stream_ptr
    from physicsbasedbayesianinference_amd.smc import TemperedSMC
    st = stream_ptr(0)
    out = {}
    # gather bandwidth, N = 2^20, D = 128, fp64
    N, D = 1 << 20, 128
    qi = torch.randn((D, N), dtype=torch.float64, device="cuda:0")
    qo = torch.empty_like(qi)
    lw = torch.randn(N, dtype=torch.float64, device="cuda:0")
    status = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    ts = []
    for i in range(6):
        lw.normal_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _lib.call("pbbi_smc_resample_systematic", lw.data_ptr(), N, 1, i, qi.data_ptr(), qo.data_ptr(), N, D, None,
                  1.0, None, None, None, status.data_ptr(), _lib.F64, 0, st)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    t = float(np.median(ts[1:]))
    byts = 2 * D * N * 8 + 12 * N
    out["resample_call_ms_N2^20_D128"] = t * 1e3
    out["resample_frac_of_8TBs"] = byts / t / 8e12
    # C2-shaped run: stage time outside pbbi_hmc_run
    A = np.random.RandomState(0).standard_normal((D, D))
    pot = P.GaussianDense(None, cov=np.eye(D) + 0.1 * A @ A.T / D)
    N = 65536
    for label, betas in (("adaptive", None), ("fixed", np.geomspace(0.3, 1.0, 10))):
        smc = TemperedSMC(pot, D, N, 1.0, 0.1, qStd=1.2, moves=5, betas=betas, seed=1)
        smc.run(device_output=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        smc.run(device_output=True)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        S = smc.nstages
        # the HMC moves alone, same shape and count
        q = torch.randn((D, N), dtype=torch.float64, device="cuda:0")
        rej = torch.empty((5, N), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for s in range(S):
            _lib.call("pbbi_hmc_run", pot.handle, _lib.LEAPFROG, q.data_ptr(), None, None, None, rej.data_ptr(), None,
                      N, N, 0.1, 10, 5, smc.flags, 1, s * 5, 0, 1.0, st)
        torch.cuda.synchronize()
        hmc = time.perf_counter() - t1
        out[label] = dict(stages=S, ms_per_stage=total / S * 1e3, hmc_ms_per_stage=hmc / S * 1e3,
                          share_outside_hmc=max(0.0, 1.0 - hmc / total), host_syncs_per_stage=smc.host_syncs / S,
                          logZ=smc.logZ)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
