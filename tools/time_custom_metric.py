#!/usr/bin/env python3
"""What the diagonal metric costs a user-defined potential in the register kernels: one pbbi_hmc_run of the quartic chain of
tests/custom_sources.py (D = 16, N = 262 144 chains, L = 10, S = 16 iterations: one fused launch; tools/bench_custom.py's
shapes) on the same handle with a non-trivial metric and without one, alternating in one process, in reference order and in
kick-drift-kick form (PBBI_KDK_FMA).

usage: tools/time_custom_metric.py [--D 16] [--N 262144] [--L 10] [--S 16] [--reps 9] [--out FILE]

Each timing is a pair of device events around the one call, after a warm-up call of each kind (code objects load on the first
launch).  Printed: one JSON line with the median, minimum and maximum of the `reps` timings of each kind in milliseconds, the
run-to-run spread (max - min over the median) and the metric's cost as a ratio of medians.  On a build whose CustomPotential
has no set_metric only the no-metric timing is taken ("metric_ms": null), so the same script measures the commit before the
metric.  Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", type=int, default=16)
    ap.add_argument("--N", type=int, default=262144)
    ap.add_argument("--L", type=int, default=10)
    ap.add_argument("--S", type=int, default=16)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--h", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from custom_sources import QUARTIC
    from physicsbasedbayesianinference_amd import _device as d, _lib as lib
    from physicsbasedbayesianinference_amd.custom import CustomPotential
    lib.load()
    pot = CustomPotential(a.D, QUARTIC, [1.0, 0.5])
    q0 = d.as_device(np.zeros((a.D, a.N)), 0, np.float64)
    samples = d.empty((a.S, a.D, a.N), np.float64, 0)
    reject = d.empty((a.S, a.N), np.uint8, 0)
    metric = 30.0 ** ((np.arange(a.D) + 0.5) / a.D)
    has_metric = hasattr(pot, "set_metric")

    def run(flags):
        q = q0.clone()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        lib.call("pbbi_hmc_run", pot.handle, lib.LEAPFROG, q.data_ptr(), None, samples.data_ptr(), None, reject.data_ptr(), None,
                 a.N, a.N, a.h, a.L, a.S, flags, 7, 0, 0, 1.0, d.stream_ptr(0))
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), 1.0 - float(reject.float().mean())

    def summary(v):
        return dict(median=statistics.median(v), min=min(v), max=max(v), spread=(max(v) - min(v)) / statistics.median(v))

    kinds = ["plain", "metric"] if has_metric else ["plain"]
    res = dict(tool="time_custom_metric", device=torch.cuda.get_device_name(0), D=a.D, N=a.N, L=a.L, S=a.S, h=a.h, reps=a.reps)
    for form, flags in (("reference_order", 0), ("kdk_fma", lib.KDK_FMA)):
        times, accept = {k: [] for k in kinds}, {}
        for rep in range(-1, a.reps):                       # rep -1: the warm-up of each kind
            for k in kinds:
                if has_metric:
                    pot.set_metric(metric if k == "metric" else None)
                ms, acc = run(flags)
                if rep >= 0:
                    times[k].append(ms)
                accept[k] = acc
        res[form] = dict(plain_ms=summary(times["plain"]), metric_ms=summary(times["metric"]) if has_metric else None,
                         metric_over_plain=(statistics.median(times["metric"]) / statistics.median(times["plain"]))
                         if has_metric else None, accept=accept)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
