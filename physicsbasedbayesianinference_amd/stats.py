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

RunningHistogram is the second sink, for what no moment yields: quantiles (credible intervals, medians) and the shape
of each marginal, from per-dimension histograms of integer counts accumulated from the same chunks
(csrc/kernels_hist.hip):

    h = RunningHistogram(D, N, bins=2048)                       # the first chunk sets the range, on the device
    rs = hmc.sampleStats(1000, 50, 1 / kB, 1.0, hist=h)
    lo95, hi95 = h.interval(0.95); med = h.median()             # within one bin width (h.resolution) of the sorted draws
"""
import ctypes as C

import numpy as np

from . import _lib
from ._device import default_device, dev, stream_ptr, to_numpy, torch

__all__ = ["RunningStats", "state_len", "rhat_from_moments", "ess_from_autocov", "RunningHistogram", "hist_state_len",
           "quantiles_from_counts", "quantile_bins", "range_from_moments", "chunk_slabs"]

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


def chunk_slabs(samples, D, N, device):
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
    if not samples.is_cuda or samples.device.index != device:
        raise ValueError(f"samples must live on device {device}")
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

    def update(self, samples):
        """Accumulate one chunk: a (D, N, c) device view or (c, D, N) slabs, float64 or float32.  One pass over the
        chunk on the current stream; nothing is read back.  Returns self."""
        sdn = chunk_slabs(samples, self.D, self.N, self.device)
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


# ---- the running histogram: quantiles and marginal shapes (include/pbbi.h "running histogram", csrc/kernels_hist.hip) ----

MIN_BINS, MAX_BINS = 16, 4096  # PBBI_HIST_MIN_BINS, PBBI_HIST_MAX_BINS


def hist_state_len(D, bins):
    """8-byte words of the device state: D (bins + 8) (pbbi_hist_state_len; needs no GPU)."""
    out = C.c_int64(0)
    try:
        _lib.call("pbbi_hist_state_len", int(D), int(bins), C.byref(out))
    except _lib.PbbiError as e:
        raise ValueError(str(e)) from None
    return int(out.value)


def range_from_moments(mean, var, width=8.0):
    """(lo, hi) = mean -/+ width * sqrt(var) per dimension: an explicit range from a pilot run's moments."""
    mean, var = np.atleast_1d(np.asarray(mean, dtype=np.float64)), np.atleast_1d(np.asarray(var, dtype=np.float64))
    if mean.shape != var.shape or mean.ndim != 1:
        raise ValueError("mean and var must be vectors of one length")
    if not width > 0 or not np.all(var > 0):
        raise ValueError("width and every variance must be > 0")
    half = float(width) * np.sqrt(var)
    return mean - half, mean + half


def _count_tables(counts, probs):
    """(counts (D, B) uint64, probs (Q,), n (D,) float64, cum (D, B) float64, k (Q, D): the first bin with cum_k >= p n)."""
    counts = np.asarray(counts, dtype=np.uint64)
    if counts.ndim != 2 or counts.shape[1] < 3:
        raise ValueError("counts must be (D, bins + 2)")
    probs = np.atleast_1d(np.asarray(probs, dtype=np.float64))
    if probs.ndim != 1 or np.any(np.isnan(probs)):
        raise ValueError("probs must be a vector of numbers")
    cum = np.cumsum(counts, axis=1, dtype=np.uint64).astype(np.float64)
    n = cum[:, -1]
    k = np.empty((probs.size, counts.shape[0]), dtype=np.int64)
    for d in range(counts.shape[0]):
        k[:, d] = np.minimum(np.searchsorted(cum[d], probs * n[d], side="left"), counts.shape[1] - 1)
    return counts, probs, n, cum, k


def quantile_bins(counts, probs):
    """(Q, D) the bin each quantile falls in (0 and bins + 1 are the tails): the first k with cum_k >= p * n."""
    return _count_tables(counts, probs)[4]


def quantiles_from_counts(counts, lo, hi, min, max, probs):
    """THE quantile rule of a histogram state, (Q, D): counts (D, bins + 2) with the two tail bins, lo / hi / min / max
    (D,).  Per dimension n = sum(counts); p <= 0 gives min, p >= 1 gives max; otherwise r = p n, k = the first bin
    with cum_k >= r, f = (r - cum_{k-1}) / counts_k and q = a + f (b - a) with [a, b] = [lo + (k-1) w, lo + k w]
    for an interior bin (w = (hi - lo) / bins; the upper end of the last one is hi), [min, lo] for k = 0 and
    [hi, max] for k = bins + 1, both ends clipped into [min, max].  In an interior bin q is within w of the
    ceil(r)-th smallest accumulated draw, which lies in the same bin.  An infinite end of a tail bin is returned as
    that infinity; a dimension without a count gives NaN."""
    counts, probs, n, cum, k = _count_tables(counts, probs)
    D, bins = counts.shape[0], counts.shape[1] - 2
    lo, hi, mn, mx = (np.broadcast_to(np.asarray(v, dtype=np.float64), (D,)) for v in (lo, hi, min, max))
    w = (hi - lo) / bins
    q = np.empty((probs.size, D))
    dd = np.arange(D)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i, p in enumerate(probs):
            ki = k[i]
            a = np.where(ki == 0, mn, np.where(ki == bins + 1, hi, lo + (ki - 1) * w))
            b = np.where(ki == 0, lo, np.where(ki == bins + 1, mx, np.where(ki == bins, hi, lo + ki * w)))
            a, b = np.clip(a, mn, mx), np.clip(b, mn, mx)
            below = np.where(ki > 0, cum[dd, np.maximum(ki - 1, 0)], 0.0)
            f = (p * n - below) / counts[dd, ki].astype(np.float64)
            qi = np.minimum(np.maximum(a + f * (b - a), a), b)   # (rounding must not carry it past an end)
            qi = np.where(np.isinf(a), a, np.where(np.isinf(b), b, qi))
            qi = np.where(p <= 0.0, mn, np.where(p >= 1.0, mx, qi))
            q[i] = np.where(n > 0, qi, np.nan)
    return q


class RunningHistogram:
    """Per-dimension histograms of an ensemble of N chains in D dimensions, pooled over chains and draws and
    accumulated on the device chunk by chunk: credible intervals, medians and marginal densities of a run that is
    never resident.  `bins` (16..4096) equal bins between lo and hi plus two tail bins, the exact minimum and maximum
    and a NaN count; the state is D (bins + 8) 8-byte words (`state_bytes`).  lo / hi (vectors of D, or scalars)
    give the range; without them the first chunk sets it on the device: its finite minimum and maximum widened by
    `margin` spans on either side.  Counts are integers: the state is the same bit for bit however the run is cut.

    The device state is allocated by the first update; until then (and in `merge`) the object is host arithmetic."""

    def __init__(self, D, N, bins=2048, lo=None, hi=None, margin=1.0, device=None):
        D, N, bins, margin = int(D), int(N), int(bins), float(margin)
        if D < 1 or N < 1:
            raise ValueError("D and N must be >= 1")
        if not MIN_BINS <= bins <= MAX_BINS:
            raise ValueError(f"bins must be in [{MIN_BINS}, {MAX_BINS}]")
        if (lo is None) != (hi is None):
            raise ValueError("give both lo and hi, or neither")
        if not margin >= 0.0 or not np.isfinite(margin):
            raise ValueError("margin must be finite and >= 0")
        self.D, self.N, self.bins, self.margin = D, N, bins, margin
        self._range = None
        if lo is not None:
            lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, dtype=np.float64), (D,)))
            hi = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, dtype=np.float64), (D,)))
            with np.errstate(over="ignore"):
                if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo < hi)
                        and np.all(np.isfinite(hi - lo))):
                    raise ValueError("lo and hi must be finite with lo < hi in every dimension")
            self._range = (lo, hi)
        self._len = hist_state_len(D, bins)
        self.device = default_device() if device is None else int(device)
        self._state = None          # (D (bins + 8),) int64 on the device, from the first update on
        self._count = 0
        self._merged = None         # what merge() added: counts, nan, min, max on the host
        self._cache = None

    @classmethod
    def from_moments(cls, mean, var, N, width=8.0, bins=2048, device=None):
        """An explicit range of mean -/+ width * sqrt(var) per dimension (e.g. RunningStats.moments() of a pilot run)."""
        lo, hi = range_from_moments(mean, var, width)
        return cls(lo.size, N, bins=bins, lo=lo, hi=hi, device=device)

    @property
    def count(self):
        """Draws per chain accumulated by update (what merge added is not in it)."""
        return self._count

    @property
    def state_bytes(self):
        return 8 * self._len

    def prepare(self):
        """Allocate the device state now and, with an explicit range, upload it (one wait for the stream); update
        does this itself on its first call.  Returns self."""
        if self._state is None:
            t = torch()
            self._state = t.empty((self._len,), dtype=t.int64, device=dev(self.device))
            if self._range is not None:
                lo, hi = self._range
                _lib.call("pbbi_hist_set_range", self._state.data_ptr(), self.D, self.bins,
                          lo.ctypes.data_as(_lib._dp), hi.ctypes.data_as(_lib._dp), self.device, stream_ptr(self.device))
        return self

    def update(self, samples):
        """Accumulate one chunk: a (D, N, c) device view or (c, D, N) slabs, float64 or float32, as
        RunningStats.update.  Queued on the current stream; nothing is read back.  Returns self."""
        sdn = chunk_slabs(samples, self.D, self.N, self.device)
        code = _lib.F64 if sdn.dtype == torch().float64 else _lib.F32
        c = int(sdn.shape[0])
        self.prepare()
        auto = 1 if (self._range is None and self._count == 0) else 0
        _lib.call("pbbi_hist_accumulate", self._state.data_ptr(), self.D, self.N, self.bins, self._count,
                  sdn.data_ptr(), c, code, auto, self.margin, self.device, stream_ptr(self.device))
        self._count += c
        self._cache = None
        return self

    def read(self):
        """The one read-back, as NumPy arrays: counts (D, bins + 2) uint64 (bin 0 below lo, bin bins + 1 at or above
        hi), lo, hi, min, max (D,) float64, nan (D,) uint64 -- the device state plus whatever merge added."""
        if self._cache is not None:
            return self._cache
        D, B = self.D, self.bins + 2
        if self._count > 0:
            words = to_numpy(self._state)
            head = words[:6 * D].reshape(6, D)
            lo, hi, _, mn, mx = (head[i].view(np.float64).copy() for i in range(5))
            nan = head[5].view(np.uint64).copy()
            counts = words[6 * D:].view(np.uint64).reshape(D, B).copy()
        elif self._range is not None:
            lo, hi = self._range[0].copy(), self._range[1].copy()
            mn, mx = np.full(D, np.inf), np.full(D, -np.inf)
            nan, counts = np.zeros(D, dtype=np.uint64), np.zeros((D, B), dtype=np.uint64)
        else:
            raise ValueError("nothing accumulated yet: the first chunk sets the range")
        if self._merged is not None:
            m = self._merged
            counts, nan = counts + m["counts"], nan + m["nan"]
            mn, mx = np.minimum(mn, m["min"]), np.maximum(mx, m["max"])
        self._cache = dict(counts=counts, lo=lo, hi=hi, min=mn, max=mx, nan=nan)
        return self._cache

    def merge(self, other):
        """Add another histogram of the same D and bins and bit-equal lo and hi (another run, another rank): a
        RunningHistogram or what its read() returned.  Counts and NaN counts add, min and max combine; the sum is
        kept on the host and shows in read() and everything built on it.  Returns self."""
        theirs = other.read() if isinstance(other, RunningHistogram) else other
        mine = self.read()
        counts = np.asarray(theirs["counts"], dtype=np.uint64)
        if counts.shape != mine["counts"].shape:
            raise ValueError(f"counts of shape {counts.shape} do not match D = {self.D}, bins = {self.bins}")
        for k in ("lo", "hi"):
            v = np.ascontiguousarray(theirs[k], dtype=np.float64)
            if v.shape != (self.D,) or v.tobytes() != np.ascontiguousarray(mine[k]).tobytes():
                raise ValueError(f"histograms merge only with bit-equal ranges ({k} differs)")
        add = dict(counts=counts, nan=np.asarray(theirs["nan"], dtype=np.uint64),
                   min=np.asarray(theirs["min"], dtype=np.float64), max=np.asarray(theirs["max"], dtype=np.float64))
        if self._merged is not None:
            m = self._merged
            add = dict(counts=m["counts"] + add["counts"], nan=m["nan"] + add["nan"],
                       min=np.minimum(m["min"], add["min"]), max=np.maximum(m["max"], add["max"]))
        self._merged, self._cache = add, None
        return self

    def quantiles(self, probs):
        """(Q, D) quantiles of each dimension over every accumulated draw (quantiles_from_counts: within one bin width
        of the order statistic wherever `clipped` is false)."""
        r = self.read()
        return quantiles_from_counts(r["counts"], r["lo"], r["hi"], r["min"], r["max"], probs)

    def interval(self, level=0.95):
        """(2, D): the central credible interval, quantiles (1 - level) / 2 and (1 + level) / 2."""
        level = float(level)
        if not 0.0 < level < 1.0:
            raise ValueError("level must be in (0, 1)")
        return self.quantiles([(1.0 - level) / 2.0, (1.0 + level) / 2.0])

    def median(self):
        return self.quantiles([0.5])[0]

    def clipped(self, probs):
        """(Q, D) bool: the quantile fell in a tail bin (below lo, or at or above hi), where only [min, lo] or
        [hi, max] bounds it.  p <= 0 and p >= 1 are min and max themselves and never clipped."""
        probs = np.atleast_1d(np.asarray(probs, dtype=np.float64))
        k = quantile_bins(self.read()["counts"], probs)
        return ((k == 0) | (k == self.bins + 1)) & ((probs > 0.0) & (probs < 1.0))[:, None]

    @property
    def resolution(self):
        """(D,) the bin widths (hi - lo) / bins: the error bound of an unclipped quantile."""
        r = self.read()
        return (r["hi"] - r["lo"]) / self.bins

    def density(self):
        """(edges (D, bins + 1), density (D, bins)): counts of the interior bins over (all counted draws x bin width),
        so each row integrates to the fraction of the draws inside [lo, hi)."""
        r = self.read()
        w = (r["hi"] - r["lo"]) / self.bins
        edges = r["lo"][:, None] + np.arange(self.bins + 1)[None, :] * w[:, None]
        edges[:, -1] = r["hi"]
        n = r["counts"].sum(axis=1, dtype=np.uint64).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            dens = r["counts"][:, 1:-1].astype(np.float64) / (n * w)[:, None]
        return edges, dens
