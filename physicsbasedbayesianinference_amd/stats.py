"""RunningStats -- the sample sink merged across chunks on the device (include/pbbi.h "running statistics",
csrc/kernels_stats.hip).

`HMC.sampleMoments`, `sampleCovariance`, `rhat` and `ess` need every draw of the run resident; a long run yields
its draws chunk by chunk (`HMC.sampleChunks`).  A RunningStats holds a device-resident fp64 state that one pass
over each chunk updates, and returns the same quantities, with the same definitions, for everything it has seen:

    rs = RunningStats(D, N, max_lag=32)
    for s_view, _ in hmc.sampleChunks(1000, 50, 1 / kB, 1.0, stats=rs): pass      # or rs.update(s_view) yourself
    mean, cov = rs.covariance(); rhat = rs.rhat(); ess = rs.ess()
    rs = hmc.sampleStats(1000, 50, 1 / kB, 1.0)                                   # the same without a host sync per chunk

Everything but the covariance is formed from per-chain state whose update runs draw by draw in draw order, so it
is bit-identical however the run was cut into chunks.  The host formulas of R-hat and the effective sample size
live here and are shared with the one-shot `HMC.rhat` / `HMC.ess`.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._device import default_device, dev, stream_ptr, to_numpy, torch

__all__ = ["RunningStats", "state_len", "rhat_from_moments", "ess_from_autocov"]

MAX_LAG = 32  # PBBI_MAX_LAG


def rhat_from_moments(W, bvar, S, N):
    """Gelman-Rubin R from W = mean_n var_s (unbiased chain variances) and bvar = the biased variance over the N
    chains of the chain means, S draws per chain:  R = sqrt(((S-1)/S W + B/S) / W)."""
    B_over_S = bvar * N / (N - 1.0)
    return np.sqrt(((S - 1.0) / S * W + B_over_S) / W)


def ess_from_autocov(g, bvar, S, N, T):
    """Multi-chain effective sample size (BDA3 11.5; Stan's ess) from g[t, d] = mean_n gamma_t,n (lags 0..T, the
    1/S form) and bvar as in rhat_from_moments: rho_t = 1 - (W - g_t) / var+, summed in pairs up to the first
    negative pair (Geyer's initial monotone sequence).  Returns (ess (D,), truncated (D,) bool: the sum was cut by
    T, not by a negative pair)."""
    D = g.shape[1]
    W = g[0] * S / (S - 1.0)
    var_plus = W * (S - 1.0) / S + bvar * N / (N - 1.0)
    rho = 1.0 - (W[None, :] - g) / var_plus[None, :]
    rho[0] = 1.0
    ess = np.empty(D)
    truncated = np.zeros(D, dtype=bool)
    for d in range(D):
        tau, prev, cut = -1.0, np.inf, False
        for t in range(0, T, 2):
            pair = rho[t, d] + rho[t + 1, d]
            if pair < 0.0:
                cut = True
                break
            pair = min(pair, prev)                         # Geyer's initial monotone sequence
            tau += 2.0 * pair
            prev = pair
        truncated[d] = not cut
        ess[d] = N * S / max(tau, 1.0 / np.log10(max(N * S, 10)))
    return ess, truncated


def state_len(D, N, max_lag):
    """Doubles of the device state: (3 T + 3) D N + 2 D + D^2 (pbbi_stats_state_len; needs no GPU)."""
    out = C.c_int64(0)
    try:
        _lib.call("pbbi_stats_state_len", int(D), int(N), int(max_lag), C.byref(out))
    except _lib.PbbiError as e:
        raise ValueError(str(e)) from None
    return int(out.value)


class RunningStats:
    """Running mean, variance, covariance, R-hat and ESS ingredients of an ensemble of N chains in D dimensions,
    accumulated on the device chunk by chunk.  max_lag (0..32) is the largest autocovariance lag kept (ess needs
    it; 0 keeps none): the state is (3 max_lag + 3) D N + 2 D + D^2 doubles (`state_bytes`)."""

    def __init__(self, D, N, max_lag=32, device=None):
        D, N, max_lag = int(D), int(N), int(max_lag)
        if D < 1 or N < 1:
            raise ValueError("D and N must be >= 1")
        if not 0 <= max_lag <= MAX_LAG:
            raise ValueError(f"max_lag must be in [0, {MAX_LAG}]")
        self.D, self.N, self.max_lag = D, N, max_lag
        self._len = state_len(D, N, max_lag)
        self.device = default_device() if device is None else int(device)
        self._state = torch().empty((self._len,), dtype=torch().float64, device=dev(self.device))
        self._count = 0
        self.ess_truncated = None

    @property
    def count(self):
        """Draws per chain accumulated so far."""
        return self._count

    @property
    def state_bytes(self):
        return 8 * self._len

    def _slabs(self, samples):
        """The (c, D, N) contiguous slabs behind `samples`: a (D, N, c) view of such slabs (what getSamples(
        device_output=True) and sampleChunks yield) is taken back without a copy, a contiguous (c, D, N) tensor is
        used as it is (where D == N == c make both readings possible, this one), any other (D, N, c) tensor is copied."""
        t = torch()
        if not isinstance(samples, t.Tensor):
            raise TypeError("samples must be a torch tensor on the device (a (D, N, c) view or (c, D, N) slabs)")
        if samples.dtype not in (t.float64, t.float32):
            raise TypeError("sample slabs must be float64 or float32")
        if samples.dim() != 3:
            raise ValueError("samples must be (D, N, c) or (c, D, N)")
        if not samples.is_cuda or samples.device.index != self.device:
            raise ValueError(f"samples must live on device {self.device}")
        D, N = self.D, self.N
        if tuple(samples.shape[:2]) == (D, N) and samples.permute(2, 0, 1).is_contiguous():
            sdn = samples.permute(2, 0, 1)
        elif tuple(samples.shape[1:]) == (D, N) and samples.is_contiguous():
            sdn = samples
        elif tuple(samples.shape[:2]) == (D, N):
            sdn = samples.permute(2, 0, 1).contiguous()
        else:
            raise ValueError(f"samples of shape {tuple(samples.shape)} are neither ({D}, {N}, c) nor (c, {D}, {N})")
        if sdn.shape[0] < 1:
            raise ValueError("a chunk holds at least one draw")
        return sdn

    def update(self, samples):
        """Accumulate one chunk: a (D, N, c) device view or (c, D, N) slabs, float64 or float32.  One pass over the
        chunk on the current stream; nothing is read back.  Returns self."""
        sdn = self._slabs(samples)
        code = _lib.F64 if sdn.dtype == torch().float64 else _lib.F32
        c = int(sdn.shape[0])
        _lib.call("pbbi_stats_accumulate", self._state.data_ptr(), self.D, self.N, self.max_lag, self._count,
                  sdn.data_ptr(), c, code, self.device, stream_ptr(self.device))
        self._count += c
        return self

    def finalize(self, chain_moments=False):
        """Every finalised quantity as NumPy float64 arrays: mean, var (D,), cov (D, D), acov (max_lag+1, D), bvar
        (D,), and W (D,) when count >= 2; with chain_moments also chain_mean and (count >= 2) chain_var, (D, N).
        The state is left as it is: a run can be finalised, continued and finalised again."""
        names = ["mean", "var", "cov", "acov", "W", "bvar"] + (["chain_mean", "chain_var"] if chain_moments else [])
        if self._count < 2:                                  # the unbiased chain variances need two draws
            names = [k for k in names if k not in ("W", "chain_var")]
        return self._finalize(*names)

    def _finalize(self, *names):
        """The named outputs of pbbi_stats_finalize (device doubles -> NumPy); the others are not computed."""
        if self._count < 1:
            raise ValueError("nothing accumulated yet")
        t = torch()
        D, N, T = self.D, self.N, self.max_lag
        shapes = dict(mean=(D,), var=(D,), cov=(D, D), acov=(T + 1, D), W=(D,), bvar=(D,), chain_mean=(D, N),
                      chain_var=(D, N))
        out = {k: t.empty(shapes[k], dtype=t.float64, device=dev(self.device)) for k in names}
        ptrs = [out[k].data_ptr() if k in out else None for k in shapes]
        _lib.call("pbbi_stats_finalize", self._state.data_ptr(), D, N, T, self._count, self.device, *ptrs,
                  stream_ptr(self.device))
        return {k: to_numpy(v) for k, v in out.items()}

    def moments(self):
        """(mean (D,), variance (D,)) over every draw of every chain, as HMC.sampleMoments (biased variance)."""
        r = self._finalize("mean", "var")
        return r["mean"], r["var"]

    def covariance(self):
        """(mean (D,), covariance (D, D)) over every draw of every chain, as HMC.sampleCovariance."""
        r = self._finalize("mean", "cov")
        return r["mean"], r["cov"]

    def rhat(self):
        """Gelman-Rubin potential scale reduction per dimension across the N chains, as HMC.rhat."""
        S, N = self._count, self.N
        if S < 2 or N < 2:
            raise ValueError("rhat needs at least 2 draws and 2 chains")
        r = self._finalize("W", "bvar")
        return rhat_from_moments(r["W"], r["bvar"], S, N)

    def ess(self, max_lag=None):
        """Effective sample size per dimension of the N chains x count draws, as HMC.ess, from min(max_lag,
        count - 2) lags (max_lag: at most the one the state was built with, the default); sets ess_truncated."""
        S, N = self._count, self.N
        if S < 4 or N < 2:
            raise ValueError("ess needs at least 4 draws and 2 chains")
        max_lag = self.max_lag if max_lag is None else int(max_lag)
        if max_lag > self.max_lag:
            raise ValueError(f"this RunningStats keeps lags up to {self.max_lag}")
        T = int(min(max_lag, MAX_LAG, S - 2))
        if T < 0:
            raise ValueError("max_lag must be >= 0")
        r = self._finalize("acov", "bvar")
        ess, self.ess_truncated = ess_from_autocov(r["acov"][:T + 1], r["bvar"], S, N, T)
        return ess
