"""What one pbbi_sample_moments call costs on the chunk shape tools/hist_sink_time.py builds, one GPU.

A resident (c, D, N) = (50, 128, 65 536) fp64 slab of Gaussian draws (3.36 GB, read once): `launches` calls after
`warmup`, each timed between two events on the stream; prints one JSON line with the median, the spread and the GB/s of
the slab.  PBBI_LIB selects the library, so the same script times another build of it (DESIGN.md 4.8 compares the
sums about the first value with the sums about zero they replaced).

usage: tools/sample_moments_time.py [--launches 20] [--warmup 5] [--chunk 50] [--chains 65536] [--dim 128] [--mean 0.0]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from physicsbasedbayesianinference_amd import _lib  # noqa: E402
from physicsbasedbayesianinference_amd._device import stream_ptr  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--mean", type=float, default=0.0)
    a = ap.parse_args()
    c, D, N = a.chunk, a.dim, a.chains
    _lib.load()
    slab = torch.empty((c, D, N), dtype=torch.float64, device="cuda")
    slab.normal_(generator=torch.Generator(device="cuda").manual_seed(1))
    slab += a.mean
    mean, var = (torch.empty(D, dtype=torch.float64, device="cuda") for _ in range(2))
    st = stream_ptr(0)
    call = lambda: _lib.call("pbbi_sample_moments", slab.data_ptr(), c, D, N, _lib.F64, 0, mean.data_ptr(),
                             var.data_ptr(), st)
    for _ in range(a.warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.launches):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        call()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    nbytes = slab.numel() * slab.element_size()
    med = float(np.median(ms))
    print(json.dumps(dict(library=_lib.LIB_PATH, device=_lib.device_info(0)["name"], shape=[c, D, N], slab_bytes=nbytes,
                          launches=a.launches, median_ms=med, min_ms=float(min(ms)), max_ms=float(max(ms)),
                          slab_GBps=nbytes / med / 1e6, mean=float(mean.mean()), var=float(var.mean()))), flush=True)
