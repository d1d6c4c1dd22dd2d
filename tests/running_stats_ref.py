"""Shared by test_running_stats.py (GPU) and test_running_stats_host.py (CPU): the AR(1) test data, the reference
statistics in NumPy longdouble straight from the definitions of include/pbbi.h, and a NumPy restatement of the
arithmetic of pbbi_stats_accumulate / pbbi_stats_finalize (shifted sums, head, window, the correction formula).
Also shared with test_sample_diagnostics.py (GPU) and test_sample_moments_host.py (CPU): the same draws moved away
from the origin (ladder), a tolerance per dimension that is relative to the dimension's own spread (tolerances), and a
NumPy restatement of k_moments_partial / k_moments_final."""
import functools

import numpy as np

S_TOTAL = 40
CUTS = ([40], [1] * 40, [3, 1, 7, 29], [33, 7])
PER_CHAIN = ("mean", "var", "W", "bvar", "acov", "chain_mean", "chain_var")   # bit-stable under re-chunking


@functools.lru_cache(maxsize=None)
def ar1(D, N, S=S_TOTAL, seed=20240611):
    """(S, D, N) float64 AR(1) chains: phi = 0.6, unit innovation variance, a common mean of 3 and a per-chain
    offset ~ N(0, 0.25).  Deliberately not centred: a wrong shift correction shows.  Read-only."""
    rs = np.random.RandomState(seed)
    phi = 0.6
    x = np.empty((S, D, N))
    x[0] = rs.standard_normal((D, N)) / np.sqrt(1.0 - phi * phi)
    for s in range(1, S):
        x[s] = phi * x[s - 1] + rs.standard_normal((D, N))
    x += 3.0 + 0.5 * rs.standard_normal((1, D, N))
    x.setflags(write=False)
    return x


def reference(x, T):
    """The finalised quantities of (S, D, N) draws in longdouble, from the definitions: mean / var (biased) over all
    S*N draws, cov (biased), per-chain mean and unbiased variance, W = their mean over chains, bvar = the biased
    variance over chains of the chain means, acov[t, d] = mean_n (1/S) sum_{s<S-t} (x_s - m_n)(x_{s+t} - m_n) (0
    for t >= S).  W and chain_var are absent for S < 2."""
    xl = np.asarray(x, dtype=np.longdouble)
    S, D, N = xl.shape
    flat = xl.transpose(1, 0, 2).reshape(D, S * N)
    mean = flat.mean(1)
    fc = flat - mean[:, None]
    cm = xl.mean(0)
    xc = xl - cm[None]
    acov = np.zeros((T + 1, D), dtype=np.longdouble)
    for t in range(min(T + 1, S)):
        acov[t] = (xc[:S - t] * xc[t:]).sum(0).mean(1) / S
    out = dict(mean=mean, var=(fc * fc).mean(1), cov=fc @ fc.T / (S * N), acov=acov, chain_mean=cm,
               bvar=((cm - cm.mean(1, keepdims=True)) ** 2).mean(1))
    if S >= 2:
        out["chain_var"] = (xc * xc).sum(0) / (S - 1)
        out["W"] = out["chain_var"].mean(1)
    return out


def tolerance(ref):
    """1e-12 * max(1, max |reference|) of that quantity."""
    return 1e-12 * max(1.0, float(np.max(np.abs(ref))))


# ---- off-centre draws and a tolerance per dimension (test_sample_moments_host.py, test_sample_diagnostics.py) ----

# (offset, scale) of dimension d % 6: |mean| / sd from ~1 up to ~1e9
RUNGS = ((0.0, 1.0), (1e3, 1.0), (-1e4, 1e-2), (299792.458, 1e-3), (1e6, 1e-3), (1e8, 1.0))
F32_RUNGS = RUNGS[:2]            # what a float can carry: 24 bits hold 1e3 +- 1 to 6e-5
CONSTANT = 299792.458            # the value of a dimension that never moves


def _rescaled(D, N, rungs):
    x = ar1(D, N)
    out = np.empty_like(x)
    for d in range(D):
        off, scale = rungs[d % len(rungs)]
        out[:, d, :] = off + scale * (x[:, d, :] - 3.0)
    return out


@functools.lru_cache(maxsize=None)
def ladder(D, N):
    """(S, D, N) float64: dimension d of ar1(D, N) mapped to off_r + scale_r * (x - 3), r = d % 6 (RUNGS).  Sums of
    x and x*x taken about zero lose (mean / sd)^2 * 2^-53 of the variance: everything, from rung 3 on.  Read-only."""
    out = _rescaled(D, N, RUNGS)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ladder_f32(D, N):
    """The float32 variant, rungs (0, 1) and (1e3, 1) only; the reference of float32 slabs is reference() of these
    rounded values (it widens them to longdouble itself).  Read-only."""
    out = _rescaled(D, N, F32_RUNGS).astype(np.float32)
    out.setflags(write=False)
    return out


def with_constant(x):
    """x with one more dimension that holds CONSTANT (rounded to x's dtype) in every draw of every chain."""
    S, D, N = x.shape
    return np.concatenate([x, np.full((S, 1, N), CONSTANT, dtype=x.dtype)], axis=1)


def rel(kappa):
    """The relative tolerance of a second moment at kappa = |mean| / spread: 1e-12 (the bar these sums of at most
    12 000 terms are held to) + 64 * 2^-53 * kappa (2^-53 * kappa is what rounding ONE stored mean of size |mean| to
    a double does to a spread of size sd; 64 is the margin).  Linear in kappa; sums about zero err with kappa^2."""
    return 1e-12 + 64.0 * 2.0 ** -53 * np.asarray(kappa, dtype=np.float64)


def tolerances(ref, f32_outputs=()):
    """{key: array of absolute tolerances, shaped like (or broadcasting to) ref[key]} for every key of reference(),
    from the reference itself: kappa_d = |mean_d| / sqrt(var_d), kappa_b = |mean_d| / sqrt(bvar_d).  Keys named in
    f32_outputs are delivered as floats and get 2^-23 |ref| on top."""
    f = lambda a: np.asarray(a, dtype=np.float64)
    mean, var, bvar = f(np.abs(ref["mean"])), f(ref["var"]), f(ref["bvar"])
    sd = np.sqrt(var)
    kd, kb = mean / sd, mean / np.sqrt(bvar)
    tol = dict(mean=1e-12 * np.maximum(mean, sd), var=rel(kd) * var, bvar=rel(kb) * bvar,
               acov=np.broadcast_to((rel(kd) * f(ref["acov"][0]))[None, :], ref["acov"].shape),
               cov=rel(np.maximum(kd[:, None], kd[None, :])) * np.sqrt(var[:, None] * var[None, :]))
    tol["chain_mean"] = np.broadcast_to(tol["mean"][:, None], ref["chain_mean"].shape)
    if "W" in ref:
        tol["W"] = rel(kd) * f(ref["W"])
        tol["chain_var"] = rel(kd)[:, None] * f(ref["chain_var"])
    for k in f32_outputs:
        tol[k] = tol[k] + 2.0 ** -23 * np.abs(f(ref[k]))
    return tol, kd, kb


def worst_ratio(got, ref, tol):
    """max over the entries of |got - ref| / tol (0 where both the error and the tolerance are 0); a NaN or an
    infinity in got gives inf."""
    err = np.abs(np.asarray(got, dtype=np.longdouble) - ref).astype(np.float64)
    tol = np.broadcast_to(tol, err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / tol)
    ratio = np.where(np.isfinite(ratio), ratio, np.inf)
    return float(np.max(ratio)) if ratio.size else 0.0


def numpy_sample_moments(x, about_zero=False, chunks=64, threads=256):
    """k_moments_partial / k_moments_final (csrc/pbbi_api.hip) in float64 NumPy, rounding where the kernels round:
    row d's S*N draws in `chunks` slices, thread k of a slice's block adds y = x - shift_d and the rounded product
    y*y of elements k, k + 256, ... in turn, the 256 thread sums go through the halving tree, the slice sums are
    added in slice order, then mean = shift + s1/count, var = s2/count - (s1/count)^2.  shift_d = x[0, d, 0];
    about_zero=True restates the arithmetic this replaced (shift = 0).  Returns (mean, var) as float64."""
    S, D, N = x.shape
    flat = np.asarray(x, dtype=np.float64).transpose(1, 0, 2).reshape(D, S * N)       # element s*N + n of row d
    total = S * N
    per = -(-total // chunks)
    shift = np.zeros(D) if about_zero else flat[:, 0].copy()
    y = flat - shift[:, None]
    s1, s2 = np.zeros(D), np.zeros(D)
    for ch in range(chunks):
        lo, hi = ch * per, min(ch * per + per, total)
        r1, r2 = np.zeros((D, threads)), np.zeros((D, threads))
        for j in range(lo, hi, threads):
            seg = y[:, j:min(j + threads, hi)]
            r1[:, :seg.shape[1]] += seg
            r2[:, :seg.shape[1]] += seg * seg
        w = threads // 2
        while w:
            r1[:, :w] += r1[:, w:2 * w]
            r2[:, :w] += r2[:, w:2 * w]
            w //= 2
        s1, s2 = s1 + r1[:, 0], s2 + r2[:, 0]
    m1 = s1 / total
    return shift + m1, s2 / total - m1 * m1


def diagnostics_reference(ref, S, N, T):
    """(rhat, ess, ess_truncated, smallest |rho_2k + rho_2k+1| up to the cut) from the longdouble quantities through
    the project's own host formulas (stats.rhat_from_moments / stats.ess_from_autocov)."""
    from physicsbasedbayesianinference_amd.stats import ess_from_autocov, rhat_from_moments
    rhat = rhat_from_moments(ref["W"], ref["bvar"], S, N)
    g = ref["acov"][:T + 1]
    ess, trunc = ess_from_autocov(g.copy(), ref["bvar"], S, N, T)
    W = g[0] * S / (S - 1.0)                                  # the pairs as ess_from_autocov forms them
    rho = 1.0 - (W[None, :] - g) / (W * (S - 1.0) / S + ref["bvar"] * N / (N - 1.0))[None, :]
    rho[0] = 1.0
    guard = np.inf
    for d in range(g.shape[1]):
        for t in range(0, T, 2):
            pair = rho[t, d] + rho[t + 1, d]
            guard = min(guard, abs(float(pair)))
            if pair < 0.0:
                break
    return rhat, ess, trunc, guard


def distance(got, ref):
    return float(np.max(np.abs(np.asarray(got, dtype=np.longdouble) - ref)))


class NumpyRunningStats:
    """What the device kernels compute, in float64 NumPy, draw by draw (products and sums rounded separately where
    the kernel fuses them)."""

    def __init__(self, D, N, T):
        self.D, self.N, self.T, self.S = D, N, T, 0

    def update(self, slabs):
        T = self.T
        for v in np.asarray(slabs, dtype=np.float64):
            if self.S == 0:
                self.c = v.copy()
                self.s1 = np.zeros_like(v)
                self.A = np.zeros((T + 1,) + v.shape)
                self.win = np.zeros((T,) + v.shape)          # win[k] = y_{S-1-k}
                self.head = np.zeros((T,) + v.shape)         # head[k] = y_k
                self.shift = v.mean(1)
                self.e = np.zeros(self.D)
                self.P = np.zeros((self.D, self.D))
            y = v - self.c
            self.s1 = self.s1 + y
            w = np.concatenate([y[None], self.win])          # w[t] = y_{s-t}
            self.A = self.A + y[None] * w
            self.win = w[:T]
            if self.S < T:
                self.head[self.S] = y
            z = v - self.shift[:, None]
            self.e = self.e + z.sum(1)
            self.P = self.P + z @ z.T
            self.S += 1
        return self

    def finalize(self):
        S, N, T = self.S, self.N, self.T
        delta = self.s1 / S
        cm = self.c + delta
        C = np.zeros((T + 1, self.D, N))
        hs, ts = np.zeros_like(delta), np.zeros_like(delta)
        for t in range(min(T + 1, S)):                       # lags t >= S stay exactly 0: the formula is not evaluated
            if t > 0:
                hs = hs + self.head[t - 1]
                ts = ts + self.win[t - 1]
            C[t] = self.A[t] - delta * (2.0 * self.s1 - hs - ts) + (S - t) * (delta * delta)
        mean = cm.sum(1) / N
        bvar = ((cm - mean[:, None]) ** 2).sum(1) / N
        out = dict(mean=mean, bvar=bvar, var=C[0].sum(1) / (S * N) + bvar, acov=C.sum(2) / (S * N), chain_mean=cm,
                   cov=self.P / (S * N) - np.outer(self.e / (S * N), self.e / (S * N)))
        if S >= 2:
            out["chain_var"] = C[0] / (S - 1)
            out["W"] = C[0].sum(1) / ((S - 1) * N)
        return out


def cut_slabs(x, cut):
    """The consecutive (c, D, N) chunks of x for a list of chunk lengths."""
    edges = np.concatenate([[0], np.cumsum(cut)])
    return [x[a:b] for a, b in zip(edges[:-1], edges[1:])]
