"""A NumPy restatement of the section "Predictive replicates" of the RNG contract (include/pbbi.h): the Philox blocks
(vectorised), the uniform, and the enumeration of a discrete support from the mode.  Helper of test_glm_predictive_host.py
and test_glm_predictive.py; no test lives here.

What is NOT taken from the device's code: the masses of the discrete families come from scipy.stats.poisson / binom / nbinom
(the device uses glm_lgamma at the mode and ratio recurrences), the cumulative probabilities of the ordinal family from
scipy.special.expit, the Gaussian's normal from the oracle's double-precision draw (oracle/pbbi_oracle.c, the same bits as the
device), the Gamma from a direct restatement with NumPy's log, sin and cos.  eta is computed in longdouble from the host copy
of the draws and rounded once.

Every replicate is evaluated at eta and at eta +- 1e-10 max(1, |eta|), and likewise at a sampled theta +- 1e-10 max(1,
|theta|).  A value on which the evaluations disagree -- the uniform sits within ~1e-10 of a step of the distribution function,
or the mode changes -- is UNDECIDED and left out of comparisons; for the continuous families the decision is the Gamma's
accepted attempt (the Gaussian has none).  Expected share ~1e-9; `MAX_UNDECIDED` = 0.1 % is the cap the tests assert."""
import numpy as np
from scipy import special, stats

LD = np.longdouble
STREAM_PREDICTIVE = 6
MAX_VAR = float(1 << 20)
GAMMA_TRIES = 64
MAX_UNDECIDED = 1e-3
EPS = 1e-10
U32 = np.uint64(0xFFFFFFFF)


# ---- Philox-4x32-10 and the counters of the contract, vectorised -----------------------------------------------------------
def philox(c0, c1, c2, c3, k0, k1):
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & U32 for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & U32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & U32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & U32, (k1 + np.uint64(0xBB67AE85)) & U32
    return c0, c1, c2, c3


def block(seed, t, i, blk):
    """The block of (draw t, observation i, index blk): counter (chain = i, block, iteration = t, stream | chain_hi24 << 8)."""
    t, i, blk = np.broadcast_arrays(np.asarray(t, dtype=np.uint64), np.asarray(i, dtype=np.uint64), np.asarray(blk, dtype=np.uint64))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox(i & U32, blk, t & U32, np.uint64(STREAM_PREDICTIVE) | ((i >> np.uint64(32)) << np.uint64(8)),
                  seed & 0xFFFFFFFF, seed >> 32)


def uniform(seed, t, i, blk=0):
    x0, x1, _, _ = block(seed, t, i, blk)
    return (((x1 << np.uint64(32)) | x0) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 + 2.0 ** -54


def normal_np(seed, t, i, blk=0):
    """The first normal of the double-precision Box-Muller, restated with NumPy's log, cos: agrees with the device to a few
    ulp, not to the bit."""
    x0, x1, x2, x3 = block(seed, t, i, blk)
    u1 = ((((x1 << np.uint64(32)) | x0) >> np.uint64(12)).astype(np.float64) + 0.5) * 2.0 ** -52
    k2 = ((x3 << np.uint64(32)) | x2) >> np.uint64(11)
    n = (k2 + np.uint64(1 << 50)) >> np.uint64(51)
    y = (k2.astype(np.int64) - (n << np.uint64(51)).astype(np.int64)).astype(np.float64) * 2.0 ** -51
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(0.5 * np.pi * (n.astype(np.float64) + y))


def normal_oracle(seed, t, i):
    """The same for block 0, from the oracle: element (dim 0, chain i) of iteration t of the stream's double-precision draw.
    t, i: broadcastable integer arrays; one oracle call per distinct t over the range of i."""
    from oracle import oracle as orc
    t, i = np.broadcast_arrays(np.asarray(t, dtype=np.int64), np.asarray(i, dtype=np.int64))
    out = np.empty(t.shape)
    lo, hi = int(i.min()), int(i.max())
    for tv in np.unique(t):
        z = orc.philox_normal(int(seed), STREAM_PREDICTIVE | 0x100, int(tv), lo, 1, hi - lo + 1)[0]
        sel = t == tv
        out[sel] = z[i[sel] - lo]
    return out


# ---- the samplers ----------------------------------------------------------------------------------------------------------
def _pmf(family, k, eta, theta, n):
    with np.errstate(over="ignore", invalid="ignore"):
        if family == "poisson":
            return stats.poisson.pmf(k, np.exp(eta))
        if family == "logistic":
            return stats.binom.pmf(k, n, special.expit(eta))
        phi = np.exp(theta)
        return stats.nbinom.pmf(k, phi, special.expit(theta - eta))        # p = phi / (phi + mu)


def _mode_var(family, eta, theta, n):
    with np.errstate(over="ignore", invalid="ignore"):
        if family == "poisson":
            mu = np.exp(eta)
            return np.floor(mu), mu
        if family == "logistic":
            p = special.expit(eta)
            return np.minimum(n, np.floor((n + 1.0) * p)), n * p * (1.0 - p)
        mu, phi = np.exp(eta), np.exp(theta)
        return np.maximum(0.0, np.floor(((phi - 1.0) * mu) / phi)), mu + mu * (mu / phi)


def discrete(family, u, eta, theta=0.0, n=1.0, batch=1 << 18):
    """Inversion over the support enumerated from the mode outwards (m, m+1, m-1, ...), masses from SciPy, accumulated in the
    contract's order in double.  Flat arrays (theta, n broadcast); NaN where the contract gives NaN."""
    u, eta, theta, n = (a.ravel() for a in np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (u, eta, theta, n))))
    y = np.full(eta.shape, np.nan)
    m, var = _mode_var(family, eta, theta, n)
    todo = np.flatnonzero(np.isfinite(eta) & (var <= MAX_VAR))
    if family == "logistic":        # n = 1: u < p, no walk
        one = todo[n[todo] == 1.0]
        y[one] = (u[one] < special.expit(eta[one])).astype(np.float64)
        todo = todo[n[todo] != 1.0]
    if todo.size > 1 and np.ptp(eta[todo]) == 0.0 and np.ptp(theta[todo]) == 0.0 and np.ptp(n[todo]) == 0.0:
        # one distribution for all: its walk once, as wide as it gets, then the first cell that reaches each u
        e0, t0, n0, m0, h = eta[todo[0]], theta[todo[0]], n[todo[0]], m[todo[0]], 64
        while True:
            j = np.arange(2 * h + 1)
            k = m0 + np.where(j % 2 == 1, (j + 1) // 2, -(j // 2)).astype(np.float64)
            f = _pmf(family, k, e0, t0, n0)
            f = np.where(np.isfinite(f), f, 0.0)
            if (f[-1] == 0.0 and f[-2] == 0.0) or h >= 1 << 22:
                break
            h *= 4
        cum = np.cumsum(f)
        at = np.searchsorted(cum, u[todo], side="left")
        lastpos = f.size - 1 - int(np.argmax(f[::-1] > 0.0))
        y[todo] = k[np.minimum(at, lastpos)]
        return y
    half = np.maximum(8, np.ceil(5.0 * np.sqrt(np.where(var <= MAX_VAR, np.maximum(var, 1.0), 1.0)))).astype(np.int64)
    while todo.size:
        # values of like width together, `batch` cells at a time
        order = todo[np.argsort(half[todo], kind="stable")]
        again, pos = [], 0
        while pos < order.size:
            h = int(half[order[pos]])
            take = max(1, batch // (2 * h + 1))
            sel = order[pos:pos + take]
            sel = sel[half[sel] <= 2 * h]
            pos += sel.size
            h = int(half[sel].max())
            j = np.arange(2 * h + 1)
            delta = np.where(j % 2 == 1, (j + 1) // 2, -(j // 2)).astype(np.float64)       # 0, +1, -1, +2, -2, ...
            k = m[sel, None] + delta[None, :]
            f = _pmf(family, k, eta[sel, None], theta[sel, None], n[sel, None])
            f = np.where(np.isfinite(f), f, 0.0)
            cum = np.cumsum(f, axis=1)                                                      # sequential, in the walk's order
            hit = cum >= u[sel, None]
            first = np.argmax(hit, axis=1)
            found = hit[np.arange(sel.size), first]
            y[sel[found]] = k[found, first[found]]
            # not found: the walk is over if the terms on both sides have reached 0 (or left the support), else it is wider
            edge_dead = (f[:, -1] == 0.0) & (f[:, -2] == 0.0)
            over = ~found & edge_dead
            if over.any():
                lastpos = f.shape[1] - 1 - np.argmax(f[:, ::-1] > 0.0, axis=1)
                y[sel[over]] = k[over, lastpos[over]]
            wider = sel[~found & ~edge_dead]
            half[wider] *= 4
            again.append(wider)
        todo = np.concatenate(again) if again else np.empty(0, dtype=np.int64)
    return y


def ordinal(u, eta, kap):
    """kap: (K - 1, ...) cutpoints broadcast against eta.  The first category whose cumulative probability reaches u."""
    cdf = special.expit(kap - eta[None])
    y = np.argmax(cdf >= u[None], axis=0).astype(np.float64)
    y = np.where(np.any(cdf >= u[None], axis=0), y, float(kap.shape[0]))
    return np.where(np.isfinite(eta) & np.all(np.isfinite(kap), axis=0), y, np.nan)


def gamma(seed, t, i, eta, theta):
    """(y, attempt): Marsaglia-Tsang as the contract states it; attempt = the accepted one, -1: none of the 64."""
    eta, theta, t, i = np.broadcast_arrays(np.asarray(eta, dtype=np.float64), np.asarray(theta, dtype=np.float64), t, i)
    alpha = np.exp(theta)
    d = np.where(alpha < 1.0, alpha + 2.0 / 3.0, alpha - 1.0 / 3.0)
    c = 1.0 / np.sqrt(9.0 * d)
    y, att = np.full(eta.shape, np.nan), np.full(eta.shape, -1)
    left = np.isfinite(eta) & np.isfinite(np.exp(eta)) & (alpha > 0) & np.isfinite(alpha)
    for j in range(GAMMA_TRIES):
        ix = np.nonzero(left)
        if not ix[0].size:
            break
        z = normal_np(seed, t[ix], i[ix], 2 * j)
        v = (1.0 + c[ix] * z) ** 3
        uu = uniform(seed, t[ix], i[ix], 2 * j + 1)
        with np.errstate(invalid="ignore", divide="ignore"):
            ok = (v > 0) & (np.log(uu) < 0.5 * z * z + d[ix] - d[ix] * v + d[ix] * np.log(v))
        got = tuple(a[ok] for a in ix)
        y[got] = d[got] * v[ok] * np.exp(eta[got]) / alpha[got]
        att[got] = j
        left[got] = False
    small = alpha < 1.0
    if small.any():
        y[small] *= uniform(seed, t[small], i[small], 0x80000000) ** (1.0 / alpha[small])
    return y, att


# ---- a model's replicates ---------------------------------------------------------------------------------------------------
def linear_predictor(sp, W):
    """eta (M, T) in longdouble from the natural-scale draws W (Dt, T), rounded once to double."""
    X, o = np.asarray(sp["X"]).astype(LD), np.asarray(sp["o"]).astype(LD)
    return np.asarray(X @ np.asarray(W).astype(LD)[:sp["Dx"]] + o[:, None], dtype=np.float64)


def _once(sp, seed, eta, theta, kap, t, i):
    """(value, decision): the replicates (M, T) at this eta / theta; `decision` is what must agree between evaluations."""
    fam = sp["family"]
    n, a = np.asarray(sp["n"], dtype=np.float64)[:, None], np.asarray(sp["a"], dtype=np.float64)[:, None]
    if fam == "gaussian":
        with np.errstate(divide="ignore"):
            y = eta + np.exp(theta) / np.sqrt(a) * normal_oracle(seed, t, i)
        return y, np.zeros(eta.shape)
    if fam == "gamma":
        return gamma(seed, t, i, eta, theta)
    u = uniform(seed, t, i)
    if fam == "ordinal":
        y = ordinal(u, eta, kap)
    else:
        th = np.broadcast_to(theta, eta.shape)
        y = discrete(fam, u, eta, th, np.broadcast_to(n, eta.shape)).reshape(eta.shape)
    return y, y


def replicates(sp, W, seed, kap=None):
    """(yrep (T, M), undecided (T, M)) of a spec of test_glm_pointwise.py (`spec_of`) and natural-scale draws W (Dt, T), draw t
    = column t.  Rows of weight 0 are NaN and decided.  kap: the ordinal family's (K - 1, T) cutpoints."""
    eta = linear_predictor(sp, W)
    M, T = eta.shape
    t, i = np.arange(T)[None, :], np.arange(M)[:, None]
    sampled = sp.get("trow", -1) >= 0
    theta = np.asarray(W, dtype=np.float64)[sp["trow"]][None, :] if sampled else (0.0 if sp.get("theta") is None else float(sp["theta"]))
    theta = np.asarray(theta, dtype=np.float64)
    kp = None if kap is None else np.asarray(kap, dtype=np.float64)[:, None, :]
    y, dec = _once(sp, seed, eta, theta, kp, t, i)
    de = EPS * np.maximum(1.0, np.abs(eta))
    trials = [] if sp["family"] == "gaussian" else [(eta + de, theta), (eta - de, theta)]      # the Gaussian decides nothing
    if sampled and trials:
        dt = EPS * np.maximum(1.0, np.abs(theta))
        trials += [(eta, theta + dt), (eta, theta - dt)]
    und = np.zeros(eta.shape, dtype=bool)
    for e2, t2 in trials:
        d2 = _once(sp, seed, e2, t2, kp, t, i)[1]
        und |= ~((d2 == dec) | (np.isnan(d2) & np.isnan(dec)))
    off = np.asarray(sp["a"]) == 0.0
    y[off], und[off] = np.nan, False
    return np.ascontiguousarray(y.T), np.ascontiguousarray(und.T)


def fixed(family, seed, T, M, **par):
    """T x M values at fixed parameters (identical rows, identical draws): the design of the distribution tests.  par: mu
    (poisson), n and p (binomial), mu and phi (negbinomial), mu and alpha (gamma), mu and sigma (gaussian), eta and kap (ordinal)."""
    t, i = np.arange(T)[:, None], np.arange(M)[None, :]
    if family == "gaussian":
        return par["mu"] + par["sigma"] * normal_oracle(seed, t, i)
    if family == "gamma":
        return gamma(seed, t, i, np.log(par["mu"]), np.log(par["alpha"]))[0]
    u = uniform(seed, t + 0 * i, i + 0 * t)
    if family == "ordinal":
        kap = np.asarray(par["kap"], dtype=np.float64)
        return ordinal(u.ravel(), np.full(u.size, float(par["eta"])), np.repeat(kap[:, None], u.size, axis=1)).reshape(T, M)
    if family == "logistic":
        eta = np.log(par["p"]) - np.log1p(-par["p"])
        return discrete(family, u, eta, 0.0, float(par["n"])).reshape(T, M)
    return discrete(family, u, np.log(par["mu"]), np.log(par.get("phi", 1.0))).reshape(T, M)


# ---- goodness of fit: what both the helper and the device's replicates are held to --------------------------------------------
def gof_pvalue(family, y, **par):
    """Chi-square on the pmf with cells of expected count >= 20 (discrete families), Kolmogorov-Smirnov on the cdf (gamma,
    gaussian), of a sample y at the parameters of `fixed`."""
    y = np.asarray(y, dtype=np.float64).ravel()
    assert np.all(np.isfinite(y))
    if family == "gaussian":
        return stats.kstest(y, stats.norm(par["mu"], par["sigma"]).cdf).pvalue
    if family == "gamma":
        return stats.kstest(y, stats.gamma(par["alpha"], scale=par["mu"] / par["alpha"]).cdf).pvalue
    if family == "ordinal":
        cdf = np.r_[special.expit(np.asarray(par["kap"], dtype=np.float64) - par["eta"]), 1.0]
        pmf = np.diff(np.r_[0.0, cdf])
    else:
        dist = (stats.poisson(par["mu"]) if family == "poisson" else stats.binom(par["n"], par["p"]) if family == "logistic"
                else stats.nbinom(par["phi"], par["phi"] / (par["phi"] + par["mu"])))
        top = int(max(y.max(), dist.ppf(1.0 - 1e-12))) + 1
        pmf = dist.pmf(np.arange(top + 1))
        pmf = np.r_[pmf, max(0.0, 1.0 - pmf.sum())]           # the far tail, one cell
    assert y.min() >= 0 and np.all(y == np.floor(y))
    obs = np.bincount(y.astype(np.int64), minlength=pmf.size).astype(np.float64)
    assert obs.size == pmf.size, "a value beyond every cell"
    exp = pmf * y.size
    # merge neighbouring cells from the left until each holds an expected count >= 20; the remainder joins the last cell
    cells_o, cells_e, co, ce = [], [], 0.0, 0.0
    for o, e in zip(obs, exp):
        co, ce = co + o, ce + e
        if ce >= 20.0:
            cells_o.append(co); cells_e.append(ce); co, ce = 0.0, 0.0
    if cells_o:
        cells_o[-1] += co; cells_e[-1] += ce
    o, e = np.array(cells_o), np.array(cells_e)
    assert o.size >= 2
    chi2 = float(np.sum((o - e) ** 2 / e))
    return float(stats.chi2.sf(chi2, o.size - 1))
