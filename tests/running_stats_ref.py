"""Shared by test_running_stats.py (GPU) and test_running_stats_host.py (CPU): the AR(1) test data, the reference
statistics in NumPy longdouble straight from the definitions of include/pbbi.h, and a NumPy restatement of the
arithmetic of pbbi_stats_accumulate / pbbi_stats_finalize (shifted sums, head, window, the correction formula)."""
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
