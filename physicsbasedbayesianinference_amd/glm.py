"""Generalised linear models as potentials whose likelihood runs on the fp64 matrix cores.

    U(w) = sum_i [ b(x_i . w) - y_i (x_i . w) ] + 0.5 prior_precision |w|^2

over the M rows x_i of the design matrix X: -log posterior of the weights of a GLM with canonical link
and a N(0, I / prior_precision) prior.  `family="logistic"`: b = softplus, y in {0, 1} (the model of
custom.logistic_regression_posterior); `family="poisson"`: b = exp, y counts.

With any of `weights`, `offset`, `trials`, `prior_mean` or a `(D,)` vector of prior precisions the model is

    U(w) = sum_i a_i [ n_i b(eta_i) - y_i eta_i ] + 0.5 sum_d lam_d (w_d - mu_d)^2,   eta_i = x_i . w + o_i

a_i observation weights (>= 0; a row of weight 0 is held out exactly), o_i offsets (Poisson: log exposure),
n_i binomial trials (logistic only; y_i successes out of n_i), lam_d >= 0 a precision per coefficient (0 = flat)
around the prior mean mu_d.  It runs on kernels of its own (the `RICH` instantiations of k_glm); the plain
model above keeps its kernels and its arithmetic.

For an ensemble the model is two matrix products shared by all chains (eta = X W, g = X^T (b'(eta) - y)
+ prior_precision W with W the (D, N) state), which csrc/kernels_glm.hip runs on the MFMA units with X
staged through LDS -- the data set is read once per 64 chains, not once per chain.  float64, D <= 128.

`SoftmaxGLM` is the categorical family on the same frame (csrc/kernels_glm_softmax.hip): K-class softmax regression,
every class with its own coefficient vector, the chain's state the K vectors class-major.

`DispersionGLM` serves the three families with a free dispersion on the full model's frame: Gaussian regression with
unknown noise, negative-binomial (NB2) counts and Gamma regression with a log link (positive, right-skewed responses;
shape 1 is exponential regression), the log-dispersion either sampled as the last component of the chain's state or
held at a given value.

`HierarchicalGLM` is the full model with hierarchical priors: blocks of coefficients (random intercepts, random slopes,
a ridge penalty of unknown strength) share a prior scale that is sampled, on the log scale, as a further row of the state.  With `penalty=` a group's prior is structured: a symmetric positive semi-definite matrix Q_j
in its quadratic form (random walks, difference penalties of splines, ICAR), Q_j (w - mu) one more product on the matrix cores.

`HierarchicalDispersionGLM` is the product of the two: the likelihood of `DispersionGLM` under the priors of `HierarchicalGLM`
-- the linear mixed model with unknown residual sigma, eight schools, negative-binomial counts with random intercepts.

`pot.pointwise(samples)` (every class but `SoftmaxGLM`) puts the draws to use on the device (csrc/kernels_glm_pointwise.hip):
per observation the log pointwise predictive density, the WAIC penalty and the posterior predictive mean, reduced over all
draws of a (D, N, S) device view without forming an M x T matrix; a second potential on held-out data takes the same draws.

`pot.predictive(samples)` draws one replicate data set per draw in the kernel (csrc/kernels_glm_predictive.hip) and returns per-draw
test statistics and posterior predictive p-values (a `PredictiveResult`).
`pot.loglik(samples)` is the total log-likelihood of each draw (csrc/kernels_glm_loglik.hip), `pot.sample_prior(N)` exact draws
from a proper prior and `pot.set_likelihood_power(beta)` the potential of p(w) L(w)^beta: the three pieces of
`smc.LikelihoodTemperedSMC`, which tempers from the prior to the posterior and returns the log marginal likelihood.
"""
import contextlib
import ctypes as C

import numpy as np

from . import _lib
from .potential import Potential, _Metric, _dptr  # (_Metric: the mixin lives in potential.py)
from .laplace import laplace as _laplace           # (bound on GLM and DispersionGLM alone)

__all__ = ["GLM", "SoftmaxGLM", "DispersionGLM", "OrdinalGLM", "HierarchicalGLM", "HierarchicalDispersionGLM", "HIER_DISP_MAX_DIM",
           "pack_prior_groups_dispersion", "FAMILIES", "DISPERSION_FAMILIES", "HIER_MAX_DIM",
           "HIER_NC_MAX_DIM", "HIER_PARAMETRISATIONS", "HIER_MAX_GROUPS", "pack_design", "pack_observations", "pack_observations_dispersion", "pack_prior_groups",
           "pack_observations_ordinal", "DISPERSION_MAX_DIM", "ORDINAL_MAX_DIM", "ORDINAL_MAX_CATEGORIES",
           "HIER_Q_MAX_DIM", "pack_penalty", "pack_metric", "pack_metric_dense", "padded_dim", "softmax_layout", "PointwiseResult", "pointwise_constants", "PredictiveResult"]

FAMILIES = {"logistic": _lib.GLM_LOGISTIC, "poisson": _lib.GLM_POISSON}
DISPERSION_FAMILIES = {"gaussian": _lib.GLM_GAUSSIAN, "negbinomial": _lib.GLM_NEGBINOMIAL,
                       "gamma": _lib.GLM_GAMMA}   # DispersionGLM; HierarchicalDispersionGLM serves those of HIER_DISP_MAX_DIM
MAX_DIM = 128
# the largest state dimension (coefficients + 1 for a sampled dispersion) of each dispersion family: the negative
# binomial's kernel at a padded dimension of 128 does not fit the register file and is not shipped; the Gamma family's does
# (profiles/glm_gamma_resources.txt)
DISPERSION_MAX_DIM = {"gaussian": 128, "negbinomial": 64, "gamma": 128}
# the largest state dimension (coefficients + groups) of HierarchicalGLM: neither family's kernel at a padded dimension
# of 128 can be built without register spills to memory, and neither is shipped
HIER_MAX_DIM = {"logistic": 64, "poisson": 64}
# ... in the non-centred parametrisation (k_glm<NT, FAM, true, GLM_HIER_NC>): the scaled copy of the state costs KS more
# registers, and the kernels at 64 rows still build without scratch for both families
HIER_NC_MAX_DIM = {"logistic": 64, "poisson": 64}
# ... with a penalty matrix (k_glm<NT, FAM, true, GLM_HIER_Q>, centred only): the kernels at 16, 32 and 64 rows build without
# scratch for both families; there is no centred kernel at 128 rows to extend
HIER_Q_MAX_DIM = {"logistic": 64, "poisson": 64}
# the largest state dimension (coefficients + groups + 1 for a sampled dispersion) of HierarchicalDispersionGLM, by family and
# parametrisation: a kernel is shipped only if it builds without register spills to memory -- all twelve of 16, 32 and 64
# rows do (profiles/glm_hier_dispersion_resources.txt), and neither parent has a hierarchical kernel at 128 rows.  The library
# states it (pbbi_glm_hier_dispersion_max_dim); this mirrors it.
HIER_DISP_MAX_DIM = {"gaussian": {"centred": 64, "noncentred": 64}, "negbinomial": {"centred": 64, "noncentred": 64}}
HIER_PARAMETRISATIONS = {"centred": _lib.HIER_CENTRED, "noncentred": _lib.HIER_NONCENTRED}
HIER_MAX_GROUPS = 4


def padded_dim(D):
    """Rows of the chain state the kernels work on: D padded to 16, 32, 64 or 128."""
    D = int(D)
    if not 1 <= D <= MAX_DIM:
        raise ValueError(f"GLM potentials serve 1 <= D <= {MAX_DIM} (D = {D})")
    return 16 if D <= 16 else 32 if D <= 32 else 64 if D <= 64 else 128


def _iptr(arr):
    return arr.ctypes.data_as(C.POINTER(C.c_int32))


def _exp(x):
    """exp of a torch tensor or of a NumPy array, in its own array type."""
    return x.exp() if hasattr(x, "exp") and not isinstance(x, np.ndarray) else np.exp(x)


@contextlib.contextmanager
def _host_errors():
    """Whatever a host packer of libpbbi.so refuses (any RuntimeError) is a ValueError: a bad argument."""
    try:
        yield
    except RuntimeError as e:
        raise ValueError(str(e)) from None


@contextlib.contextmanager
def _device_errors():
    """What a device entry refuses about its arguments (INVALID, UNSUPPORTED) is a ValueError; every other failure stays."""
    try:
        yield
    except _lib.PbbiError as e:
        if e.code in (_lib.ERR_INVALID, _lib.ERR_UNSUPPORTED):
            raise ValueError(str(e)) from None
        raise


def _pack(name, scalars, arrays, also=()):
    """The protocol of the host packers `name(*scalars, *arrays, out, out_len, &len, *also)`: one call with NULL arrays for
    the length, one that fills a fresh array; `also` are further output arrays.  Returns the filled (flat) array."""
    n = C.c_int64()
    _lib.call(name, *scalars, *[None] * len(arrays), None, 0, C.byref(n), *[None] * len(also))
    out = np.empty(n.value, dtype=np.float64)
    _lib.call(name, *scalars, *[_dptr(v) for v in arrays], _dptr(out), out.size, C.byref(n), *[_dptr(v) for v in also])
    return out


def pack_metric(diag):
    """The table {m_d, 1 / m_d} a GLM handle with a diagonal metric keeps on the device and its kernel in LDS, computed
    (and checked: every entry finite and > 0) on the host by libpbbi.so (no GPU involved): array (DP, 2), {1, 1} on the
    padding rows."""
    m = np.ascontiguousarray(diag, dtype=np.float64)
    if m.ndim != 1 or m.size < 1:
        raise ValueError("the metric must be a vector of D >= 1 masses")
    return _pack("pbbi_glm_pack_metric", (m.size,), (m,)).reshape(-1, 2)


def pack_metric_dense(M):
    """The three images a GLM handle with a dense metric keeps on the device, computed (and checked: D <= 64, finite,
    symmetric to 1e-12 of the largest entry, positive definite) on the host by libpbbi.so (no GPU involved): array (3, DP
    DP / 2, 64, 2) -- C = inv(M), the lower Cholesky factor L and M itself, each padded with the identity to DP rows and
    laid out like pack_penalty's image, [t * DP / 8 + s2][lane][e] = A[16 t + (lane & 15)][4 (2 s2 + e) + (lane >> 4)]."""
    m = np.ascontiguousarray(M, dtype=np.float64)
    if m.ndim != 2 or m.shape[0] != m.shape[1] or m.shape[0] < 1:
        raise ValueError("the dense metric must be a (D, D) matrix, D >= 1")
    with _host_errors():
        return _pack("pbbi_glm_pack_metric_dense", (m.shape[0],), (m,)).reshape(3, -1, 64, 2)


def pack_design(X):
    """The MFMA fragment image of X that the handle keeps on the device, computed on the host by
    libpbbi.so (no GPU involved): array (blocks, 2, DP/4 * 64) -- per block of 16 observations the
    A fragments of the product X_b . W ([:, 0], as [DP/8][64 lanes][2]) and of X_b^T . R ([:, 1], as
    [2][DP/16][64 lanes][2]); layout in include/pbbi.h.  The block count is padded to a multiple of 4."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] < 1:
        raise ValueError("X must be (M, D) with M >= 1")
    M, D = X.shape
    DP = padded_dim(D)
    return _pack("pbbi_glm_pack_design", (D, M), (X,)).reshape(-1, 2, DP * 16)


def pack_observations(y, family="logistic", weights=None, offset=None, trials=None):
    """The three per-observation streams the handle of the full model keeps on the device, computed (and
    checked) on the host by libpbbi.so: array (3, L) -- c = weights * trials, d = weights * y and the
    offset, each zero padded to L = 16 * (blocks of 16 observations, padded to a multiple of 4)."""
    _known_family(family, FAMILIES)
    y = np.ascontiguousarray(y, dtype=np.float64)
    if y.ndim != 1 or y.size < 1:
        raise ValueError("y must be 1-D with at least one entry")
    M = y.size
    vec = [None if v is None else _vector(v, M, name, "M") for v, name in
           ((weights, "weights"), (offset, "offset"), (trials, "trials"))]
    with _host_errors():
        return _pack("pbbi_glm_pack_observations", (M, FAMILIES[family]), (y, *vec)).reshape(3, -1)


def pack_observations_dispersion(y, family="negbinomial", weights=None, offset=None):
    """The three per-observation streams a DispersionGLM handle keeps on the device, computed (and checked) on the host
    by libpbbi.so: array (3, L) -- c = weights, d = y (raw, not weights * y; family "gamma": log y, which is all its
    kernels need of y) and the offset, each zero padded to L as for `pack_observations`.  "gamma" requires y > 0.
    `HierarchicalDispersionGLM` keeps the same streams."""
    _known_family(family, DISPERSION_FAMILIES)
    y = np.ascontiguousarray(y, dtype=np.float64)
    if y.ndim != 1 or y.size < 1:
        raise ValueError("y must be 1-D with at least one entry")
    M = y.size
    vec = [None if v is None else _vector(v, M, name, "M") for v, name in ((weights, "weights"), (offset, "offset"))]
    with _host_errors():
        return _pack("pbbi_glm_pack_observations_dispersion", (M, DISPERSION_FAMILIES[family]), (y, *vec)).reshape(3, -1)


def pack_observations_ordinal(y, categories, weights=None, offset=None):
    """The three per-observation streams an OrdinalGLM handle keeps on the device, computed (and checked) on the host by
    libpbbi.so, and the weighted category counts: ((3, L) array, (8,) array) -- c = weights, d = y (the category) and the
    offset, each zero padded to L as for `pack_observations`; A_k = the sum of the weights of category k, 0 past `categories`."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    if y.ndim != 1 or y.size < 1:
        raise ValueError("y must be 1-D with at least one entry")
    M, K = y.size, int(categories)
    vec = [None if v is None else _vector(v, M, name, "M") for v, name in ((weights, "weights"), (offset, "offset"))]
    counts = np.empty(8, dtype=np.float64)
    with _host_errors():
        return _pack("pbbi_glm_pack_observations_ordinal", (M, K), (y, *vec), also=(counts,)).reshape(3, -1), counts


def _known_family(family, table):
    if family not in table:
        raise ValueError("family must be one of %s (got %r)" % (sorted(table), family))


def _vector(v, n, name, letter):
    v = np.asarray(v, dtype=np.float64)
    if v.ndim != 1 or v.size != n:
        raise ValueError("%s must be 1-D with %s = %d entries (shape %s)" % (name, letter, n, v.shape))
    if not np.all(np.isfinite(v)):
        raise ValueError("%s must be finite" % name)
    return np.ascontiguousarray(v)


def _design_shape(X, y):
    """(X, y, M, D) as contiguous float64: X 2-D with at least one row and one column, y 1-D with one entry per row."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("X must be 2-D: (M, D) with at least one row and one column")
    M, D = X.shape
    y = np.asarray(y, dtype=np.float64)
    if y.ndim != 1 or y.size != M:
        raise ValueError("X has %d rows, y must be 1-D with as many entries (shape %s)" % (M, y.shape))
    return np.ascontiguousarray(X), np.ascontiguousarray(y), M, D


def _design(X, y):
    """The rule for X and y of every GLM class: `_design_shape`, and both finite."""
    X, y, M, D = _design_shape(X, y)
    if not np.all(np.isfinite(X)) or not np.all(np.isfinite(y)):
        raise ValueError("X and y must be finite")
    return X, y, M, D


def _obs_vectors(weights, offset, M):
    """`weights` ((M,), finite, >= 0) and `offset` ((M,), finite) checked, None where not given."""
    if weights is not None:
        weights = _vector(weights, M, "weights", "M")
        if not np.all(weights >= 0):
            raise ValueError("weights must be >= 0")
    if offset is not None:
        offset = _vector(offset, M, "offset", "M")
    return weights, offset


def _precision_vector(prior_precision, D):
    """`prior_precision`, a scalar or a (D,) vector of finite values >= 0, as the (D,) vector."""
    lam = np.asarray(prior_precision, dtype=np.float64)
    if lam.ndim == 0:
        if not np.isfinite(lam):
            raise ValueError("prior_precision must be finite and >= 0")
        lam = np.full(D, float(lam))
    else:
        lam = _vector(lam, D, "prior_precision", "D")
    if not np.all(lam >= 0):
        raise ValueError("every prior_precision must be >= 0")
    return lam


def _float64_only(dtype):
    if np.dtype(dtype) != np.dtype("float64"):
        raise ValueError("GLM potentials are float64 only")


def _validate(X, y, family, prior_precision, dtype, prior_mean=None, weights=None, offset=None, trials=None):
    # `_design`, with the family asked for between its shape and its value checks: the order this function has always had
    _design_shape(X, y)
    _known_family(family, FAMILIES)
    X, y, M, D = _design(X, y)
    weights, offset = _obs_vectors(weights, offset, M)
    if trials is not None:
        if family != "logistic":
            raise ValueError("trials belong to the logistic (binomial) family only")
        trials = _vector(trials, M, "trials", "M")
        if not (np.all(trials >= 1) and np.all(trials == np.floor(trials))):
            raise ValueError("trials must hold integers >= 1")
    if family == "logistic":
        if trials is None and not np.all((y == 0) | (y == 1)):
            raise ValueError("logistic: y must be 0 or 1 (or successes out of `trials`)")
        if trials is not None and not (np.all(y >= 0) and np.all(y <= trials) and np.all(y == np.floor(y))):
            raise ValueError("logistic: y must hold integers with 0 <= y <= trials")
    if family == "poisson" and not (np.all(y >= 0) and np.all(y == np.floor(y))):
        raise ValueError("poisson: y must hold non-negative integers")
    lam = np.asarray(prior_precision, dtype=np.float64)
    if lam.ndim == 0:
        lam = float(lam)
        if not (np.isfinite(lam) and lam >= 0):
            raise ValueError("prior_precision must be a finite scalar >= 0 (or a (D,) vector of such)")
    else:
        lam = _vector(lam, D, "prior_precision", "D")
        if not np.all(lam >= 0):
            raise ValueError("every prior_precision must be >= 0")
    if prior_mean is not None:
        prior_mean = _vector(prior_mean, D, "prior_mean", "D")
    if D > MAX_DIM:
        raise ValueError(f"GLM potentials serve D <= {MAX_DIM} (D = {D})")
    _float64_only(dtype)
    return X, y, lam, prior_mean, weights, offset, trials


class PointwiseResult:
    """What `pointwise` returns: per observation (NumPy (M,) arrays) `lppd_i` (the log pointwise predictive density, log
    mean_t p(y_i | draw t)), `mean_ll_i` (mean_t log p(y_i | draw t)), `p_waic_i` (the unbiased variance over the draws of
    log p(y_i | draw t): the WAIC penalty; NaN with a single draw) and `mu_i` (the posterior mean of E[y_i], times the
    trials for binomial data); `T` the number of draws; and the scalars `lppd`, `p_waic`, `waic = -2 (lppd - p_waic)`."""

    def __init__(self, lppd_i, mean_ll_i, p_waic_i, mu_i, T):
        self.lppd_i, self.mean_ll_i, self.p_waic_i, self.mu_i, self.T = lppd_i, mean_ll_i, p_waic_i, mu_i, int(T)

    @property
    def lppd(self):
        return float(np.sum(self.lppd_i))

    @property
    def p_waic(self):
        return float(np.sum(self.p_waic_i))

    @property
    def waic(self):
        return -2.0 * (self.lppd - self.p_waic)

    def __repr__(self):
        return "PointwiseResult(M=%d, T=%d, lppd=%.6g, p_waic=%.6g, waic=%.6g)" % (self.lppd_i.size, self.T, self.lppd,
                                                                                 self.p_waic, self.waic)


class PredictiveResult:
    """What `predictive` returns.  Per draw, (N, S) NumPy arrays of the test statistics of that draw's replicate data set y_rep
    (over the observations of weight != 0): `mean`, `var` (the population variance), `min`, `max`, `frac_le_cut` (the share of
    y_rep <= cut), `loglik_rep` = log p(y_rep | draw) and `loglik_obs` = log p(y | draw) (full proper log densities).
    `observed`: a dict of the same statistics of the data y themselves ("mean", "var", "min", "max", "frac_le_cut").
    `yrep`: the replicates of the first `keep` draws, (keep, M) with NaN on rows of weight 0, or None.  `T`: the number of draws."""

    NAMES = ("mean", "var", "min", "max", "frac_le_cut")

    def __init__(self, mean, var, min, max, frac_le_cut, loglik_rep, loglik_obs, observed, yrep=None):
        self.mean, self.var, self.min, self.max, self.frac_le_cut = mean, var, min, max, frac_le_cut
        self.loglik_rep, self.loglik_obs, self.observed, self.yrep = loglik_rep, loglik_obs, dict(observed), yrep
        self.T = int(np.size(mean))

    def pvalue(self, name):
        """The posterior predictive p-value of a statistic: the share of draws with T(y_rep) >= T(y), `name` one of "mean",
        "var", "min", "max", "frac_le_cut"; for "loglik" the discrepancy is the log density itself, which depends on the
        draw: the share of draws with log p(y_rep | draw) <= log p(y | draw).  Draws whose statistic is NaN count as not
        meeting the condition."""
        if name == "loglik":
            return float(np.mean(self.loglik_rep <= self.loglik_obs))
        if name not in self.NAMES:
            raise ValueError("pvalue: unknown statistic %r (one of %s, \"loglik\")" % (name, ", ".join(map(repr, self.NAMES))))
        return float(np.mean(getattr(self, name) >= self.observed[name]))

    def __repr__(self):
        return "PredictiveResult(T=%d, %s)" % (self.T, ", ".join("p_%s=%.3g" % (n, self.pvalue(n)) for n in self.NAMES))


def _predictive_aux(pot):
    """(aux, on): the image y | n | a of pbbi_predictive_glm -- three runs zero padded to a multiple of 64 observations -- and
    the mask of the rows of weight != 0."""
    y = np.asarray(pot.y, dtype=np.float64).ravel()
    M = y.size
    a = np.ones(M) if pot.weights is None else np.asarray(pot.weights, dtype=np.float64)
    n = np.ones(M) if pot.trials is None else np.asarray(pot.trials, dtype=np.float64)
    aux = np.zeros((3, (M + 63) // 64 * 64))
    aux[0, :M], aux[1, :M], aux[2, :M] = y, n, a
    return aux, a != 0.0


def _predictive(self, samples, seed=0, keep=0, cut=0.0, ranges=0):
    """Posterior predictive checks, drawn on the device (csrc/kernels_glm_predictive.hip): for every draw one replicate data set
    y_rep ~ p(y | draw) at the potential's own design, reduced in the kernel to per-draw test statistics -- no M x T matrix
    unless `keep` asks for one.

        r = pot.predictive(s[:, :, 500:])                # r.pvalue("var"), r.pvalue("max"), r.pvalue("frac_le_cut"): zeros
        y_new = GLM(X_new, dummy_y).predictive(s, keep=200).yrep       # replicates at new inputs, (200, len(X_new))

    `samples` as for `pointwise`.  `seed`: the replicate of (draw t, observation i) is a function of (seed, t, i) alone (the
    RNG contract of include/pbbi.h, stream PBBI_STREAM_PREDICTIVE), t counted over the draws of THIS call in the order slab,
    chain.  `keep`: the replicates of the first `keep` draws (in that order) come back as `yrep`, (keep, M).  `cut`: the
    threshold of `frac_le_cut` (0: the share of zeros of count data).  `ranges` as for `loglik`.  The samplers are exact
    (inversion from the mode for the count families, Marsaglia-Tsang for the gamma); a DISCRETE replicate whose distribution
    has a variance above 2^20 is not served and is NaN, as is one with a non-finite linear predictor, and a NaN replicate makes
    its own draw's mean, var, min, max and loglik_rep NaN.  Weights: a row of weight 0 takes no part (NaN in `yrep`); otherwise
    a weight changes a replicate's distribution only for the gaussian family, where it is a precision weight (variance
    sigma^2 / a_i); the log densities are unweighted but for that.  Returns a `PredictiveResult`."""
    from . import _device
    sdn, S, Dt, N = _pointwise_slabs(self, samples)
    M, T, keep = self.y.size, S * N, int(keep)
    aux, on = _predictive_aux(self)
    n_on = int(np.count_nonzero(on))
    if not n_on:
        raise ValueError("predictive: every observation has weight 0")
    yo = np.asarray(self.y, dtype=np.float64).ravel()[on]
    centre = float(np.mean(yo))
    aux_d = _device.as_device(aux, self.device, np.float64)
    stats = _device.empty((7, T), np.float64, self.device)
    if 0 < keep <= T and keep * M > 1 << 28:       # (the library's own rule, before the buffer is asked for)
        raise ValueError("predictive: keep * M must be <= 2^28 values of yrep (keep = %d, M = %d)" % (keep, M))
    yrep = _device.empty((keep, M), np.float64, self.device) if 0 < keep <= T else None
    with _device_errors():
        _lib.call("pbbi_predictive_glm", self.handle, sdn.data_ptr(), S, Dt, N, int(seed) & 0xFFFFFFFFFFFFFFFF,
                  aux_d.data_ptr(), centre, float(cut), int(ranges), stats.data_ptr(), keep,
                  yrep.data_ptr() if yrep is not None else None, _device.stream_ptr(self.device))
    s = _device.to_numpy(stats)
    per = lambda v: np.ascontiguousarray(v.reshape(S, N).T)      # (N, S), as `loglik`
    d1 = s[0] / n_on
    observed = dict(mean=centre, var=float(np.mean((yo - centre) ** 2)), min=float(yo.min()), max=float(yo.max()),
                    frac_le_cut=float(np.mean(yo <= float(cut))))
    return PredictiveResult(per(centre + d1), per(s[1] / n_on - d1 * d1), per(s[2]), per(s[3]), per(s[4] / n_on), per(s[5]),
                            per(s[6]), observed, None if yrep is None else _device.to_numpy(yrep))


def _lgamma(x):
    import math
    return np.array([math.lgamma(v) for v in np.asarray(x, dtype=np.float64).ravel()]).reshape(np.shape(x))


def pointwise_constants(family, y, weights=None, trials=None):
    """k_i: the part of observation i's log-likelihood that depends on no parameter, which the kernels drop and `pointwise`
    adds on the host -- a_i log C(n_i, y_i) (logistic), -a_i lgamma(y_i + 1) (poisson, negbinomial), -a_i / 2 log 2 pi
    (gaussian), -a_i log y_i (gamma), 0 (ordinal: nothing is dropped); a_i the weights (the likelihood of observation i enters to the power a_i)."""
    y = np.asarray(y, dtype=np.float64)
    a = np.ones_like(y) if weights is None else np.asarray(weights, dtype=np.float64)
    if family == "logistic":
        n = np.ones_like(y) if trials is None else np.asarray(trials, dtype=np.float64)
        return a * (_lgamma(n + 1.0) - _lgamma(y + 1.0) - _lgamma(n - y + 1.0))
    if family in ("poisson", "negbinomial"):
        return -a * _lgamma(y + 1.0)
    if family == "gaussian":
        return -0.5 * np.log(2.0 * np.pi) * a
    if family == "gamma":
        return -a * np.log(y)
    if family == "ordinal":
        return np.zeros_like(y)
    raise ValueError("pointwise_constants: unknown family %r" % (family,))


def _pointwise_slabs(pot, samples):
    """(sdn, S, Dt, N): contiguous (S, Dt, N) float64 slabs on the potential's device holding `samples` on the natural scale --
    a (D, N, S) device view of such slabs (getSamples(device_output=True), also sliced along S) without a copy."""
    from . import _device
    t = _device.torch()
    natural = pot.parametrisation != "centred"

    def rows(Dt):
        if Dt < pot.numDimensions:
            raise ValueError("samples have %d rows, the potential's state has %d" % (Dt, pot.numDimensions))

    if isinstance(samples, t.Tensor):
        if samples.dim() == 2:
            samples = samples.unsqueeze(2)
        if samples.dim() != 3 or samples.dtype != t.float64:
            raise ValueError("samples must be a float64 (D, N, S) device view or a NumPy (Dt, N, S) / (Dt, T) array")
        if not samples.is_cuda or samples.device.index != pot.device:
            raise ValueError("samples must live on device %d" % pot.device)
        rows(samples.shape[0])
        if natural:
            samples = pot.to_natural(samples)
        sdn = samples.permute(2, 0, 1)
        if not sdn.is_contiguous():
            sdn = sdn.contiguous()
    else:
        q = np.asarray(samples, dtype=np.float64)
        if q.ndim == 2:
            q = q[:, :, None]
        if q.ndim != 3:
            raise ValueError("samples must be (Dt, N, S) or (Dt, T)")
        rows(q.shape[0])
        if natural:
            q = pot.to_natural(q)
        sdn = _device.as_device(np.ascontiguousarray(np.transpose(q, (2, 0, 1))), pot.device, np.float64)
    S, Dt, N = (int(v) for v in sdn.shape)
    if S < 1 or N < 1:
        raise ValueError("samples hold no draw")
    return sdn, S, Dt, N


def _pointwise(self, samples, ranges=0):
    """Per-observation log-likelihood statistics over posterior draws, reduced on the device (csrc/kernels_glm_pointwise.hip):
    the log pointwise predictive density, WAIC and the posterior predictive mean, without an M x T matrix anywhere.

        s = hmc.getSamples(2000, device_output=True)             # (D, N, S) device view
        r = pot.pointwise(s[:, :, 500:])                          # burn-in dropped; r.waic, r.lppd, r.p_waic, r.mu_i
        held = GLM(X_new, y_new).pointwise(s[:, :, 500:]).lppd    # held-out log predictive density of the same draws
        mu = GLM(X_new, np.zeros(len(X_new))).pointwise(s).mu_i   # the fitted mean at new X (a dummy response)

    `samples`: the (D, N, S) device view of getSamples(device_output=True) (any slice along S; no copy), or a NumPy array
    (Dt, N, S) or (Dt, T), in the SAMPLER's coordinates: `to_natural` is applied where the potential has one.  Rows past the
    state dimension are ignored.  `ranges`: 0 lets the library choose into how many ranges the draws are cut; >= 1 fixes it
    (for a given value the result is bit for bit reproducible).  Returns a `PointwiseResult`.  An observation of weight 0 has
    log-likelihood 0 exactly (it adds nothing to lppd and WAIC); its `mu_i` is formed like any other's."""
    from . import _device
    sdn, S, Dt, N = _pointwise_slabs(self, samples)
    M, T = self.y.size, S * N
    out = _device.empty((4, M), np.float64, self.device)
    ptr = [out[k].data_ptr() for k in range(4)]
    with _device_errors():
        _lib.call("pbbi_pointwise_glm", self.handle, sdn.data_ptr(), S, Dt, N, int(ranges), ptr[0], ptr[1],
                  ptr[2] if T >= 2 else None, ptr[3], _device.stream_ptr(self.device))
    lse, mean, var, mu = _device.to_numpy(out)
    k = pointwise_constants(self.family, self.y, self.weights, self.trials)
    if self.trials is not None:
        mu = mu * self.trials
    return PointwiseResult(lse - np.log(T) + k, mean + k, var if T >= 2 else np.full(M, np.nan), mu, T)


def _loglik(self, samples, ranges=0, device_output=False):
    """The total log-likelihood of every draw, on the device (csrc/kernels_glm_loglik.hip): (N, S), log p(y | draw) with the
    constants `pointwise_constants` of the observations added -- no prior term.  `samples` as for `pointwise`: the (D, N, S)
    device view of getSamples(device_output=True) (no copy), a (D, N) state, or NumPy arrays, in the SAMPLER's coordinates
    (`to_natural` is applied where the potential has one).  `ranges`: 0 lets the library choose into how many ranges the
    observations are cut; >= 1 fixes it (for a given value the result is bit for bit reproducible).  The likelihood is at power
    1 whatever `likelihood_power` is.  `device_output=True` keeps the result on the device (a float64 tensor)."""
    from . import _device
    if not isinstance(samples, _device.torch().Tensor):
        # uploaded BEFORE `to_natural`: host and device input then go through the same torch ops and give the same bits
        q = np.ascontiguousarray(samples, dtype=np.float64)
        if q.ndim not in (2, 3):
            raise ValueError("samples must be (Dt, N, S) or (Dt, T)")
        samples = _device.as_device(q, self.device, np.float64)
    sdn, S, Dt, N = _pointwise_slabs(self, samples)
    out = _device.empty((S, N), np.float64, self.device)
    pot = self._power_target(build=False)
    with _device_errors():
        _lib.call("pbbi_loglik_glm", pot.handle, sdn.data_ptr(), S, Dt, N, int(ranges), out.data_ptr(),
                  _device.stream_ptr(self.device))
    k = float(np.sum(pointwise_constants(self.family, self.y, self.weights, self.trials)))
    ll = (k - out).t()
    return ll if device_output else _device.to_numpy(ll.contiguous())


def _prior_layout(pot):
    """(mean, precision, names, D, J, groups) of the rows of the state: what `sample_prior` draws from; the precision of a
    grouped coefficient is NaN (its scale is exp(t_j))."""
    D, J, groups = pot.numCoefficients, pot.numGroups, pot.groups
    lam = np.full(D, float(pot.prior_precision)) if np.ndim(pot.prior_precision) == 0 else np.array(pot.prior_precision, float)
    mu = np.zeros(D) if pot.prior_mean is None else np.asarray(pot.prior_mean, dtype=np.float64)
    names = ["prior_precision[%d]" % d for d in range(D)]
    if groups is not None:
        lam = np.where(groups >= 0, np.nan, lam)
    mean, prec = [mu], [lam]
    if J:
        tp = np.asarray(pot.log_scale_prior, dtype=np.float64)
        mean.append(tp[:, 0]); prec.append(tp[:, 1])
        names += ["log_scale_prior[%d]" % j for j in range(J)]
    if pot.sampled:
        m_t, l_t = pot.log_dispersion_prior
        mean.append([m_t]); prec.append([l_t])
        names.append("log_dispersion_prior")
    if pot.cutpoint_prior is not None:
        cp = np.asarray(pot.cutpoint_prior, dtype=np.float64)
        mean.append(cp[:, 0]); prec.append(cp[:, 1])
        names += ["cutpoint_prior[%d]" % j for j in range(cp.shape[0])]
    return np.concatenate(mean), np.concatenate(prec), names, D, J, groups


def _sample_prior(self, N, seed=0, draw_f64=True):
    """N exact draws from the prior, in SAMPLER coordinates: a (numDimensions, N) float64 device tensor.  Standard normals z from
    the device Philox stream (pbbi_philox_normal, PBBI_STREAM_POSITION, iteration 0, chain index n; `draw_f64`: the
    double-precision draw) transformed with torch ops on the device: a fixed row is mu_d + z / sqrt(lam_d); t_j and a sampled
    theta are drawn from their (mean, precision) priors; a grouped row is mu_d + exp(t_j) z_d (centred) or z_d (non-centred).
    Raises ValueError naming the row when the prior is improper: a precision of 0 on a row that uses it, or a `penalty=` group
    (structured priors, rank deficient or not, are not served)."""
    from . import _device
    t = _device.torch()
    N = int(N)
    if N < 1:
        raise ValueError("sample_prior: N must be >= 1")
    if self.penalty is not None:
        j = [j for j, Q in enumerate(self.penalty) if Q is not None][0]
        raise ValueError("sample_prior: group %d has a structured prior (penalty[%d]), which is not served" % (j, j))
    mean, prec, names, D, J, groups = _prior_layout(self)
    for d, name in enumerate(names):
        if prec[d] == 0.0:
            raise ValueError("sample_prior: the prior of row %d is improper (%s = 0)" % (d, name))
    Dn, dev = self.numDimensions, self.device
    z = _device.empty((Dn, N), np.float64, dev)
    stream = _lib.STREAM_POSITION | (_lib.STREAM_DRAW_F64 if draw_f64 else 0)
    _lib.call("pbbi_philox_normal", int(seed), stream, 0, 0, Dn, N, N, 1.0, None, _lib.F64, dev, z.data_ptr(),
              _device.stream_ptr(dev))
    grouped = np.zeros(Dn, dtype=bool) if groups is None else np.r_[groups >= 0, np.zeros(Dn - D, dtype=bool)]
    sd = np.where(grouped, 1.0, 1.0 / np.sqrt(np.where(grouped, 1.0, prec)))
    mean_d = _device.as_device(np.ascontiguousarray(mean), dev, np.float64)
    sd_d = _device.as_device(np.ascontiguousarray(sd), dev, np.float64)
    q = mean_d[:, None] + z * sd_d[:, None]        # every row that has a (mean, precision) prior of its own
    if grouped.any():
        rows = np.flatnonzero(grouped)
        rows_d = t.as_tensor(rows, device=q.device)
        if self.parametrisation == "centred":
            trow = t.as_tensor(D + np.asarray(groups)[rows].astype(np.int64), device=q.device)
            q[rows_d] = mean_d[rows_d][:, None] + q[trow].exp() * z[rows_d]
        else:
            q[rows_d] = z[rows_d]
    return q


class _GLMBase(Potential):
    """What the six GLM classes share: the layout of the chain's state, declared.  Its rows are `numCoefficients` coefficients
    (`groups`: the prior group of each, or None), `numGroups` group log-scales, one log-dispersion if `sampled`, and one row per
    entry of `cutpoint_prior`.  `_prior_layout`, `pointwise`, `loglik`, `sample_prior` and smc.py read these attributes; a
    class sets on its instances the ones in which it differs from the defaults here."""

    kind = "glm"
    trials = None
    groups = None
    numGroups = 0
    sampled = False
    cutpoint_prior = None
    penalty = None
    parametrisation = "centred"

    def __getattr__(self, name):      # (asked only for what the instance and its classes do not have)
        if name == "numCoefficients":
            return self.numDimensions
        raise AttributeError(name)


class _Tempered:
    """The likelihood power of a GLM potential (pbbi_potential_set_likelihood_power): the potential becomes
    -log [ p(w) L(w)^beta ], the prior-to-posterior path of `smc.LikelihoodTemperedSMC`.  It lives on the handle: every sampler
    that shares the potential shares it (as it shares the metric).  `loglik` always reports the likelihood at power 1.

    The exception is a plain `GLM` (no weights, offsets, trials or prior vectors): its handle keeps no observation streams and
    is NEVER tempered.  There only the cached full-model twin `pot._power_target()` carries the power -- `pot(q)`, `pot.handle`
    and any sampler built on `pot` itself stay at power 1 whatever `pot.likelihood_power` reports; sample the tempered model
    through the twin, as `smc.LikelihoodTemperedSMC` does."""

    loglik = _loglik
    sample_prior = _sample_prior

    def _power_target(self, build=True):
        return self

    def set_likelihood_power(self, beta, beta_dev=None):
        """beta: finite and > 0 (1 restores the potential bit for bit).  `beta_dev`: the address of a device double to read beta
        from instead (no host value is involved; `likelihood_power` then reports NaN).  On a plain `GLM` the power is set on the
        twin `_power_target()` alone (see the class text): the plain handle stays at power 1."""
        from . import _device
        if beta_dev is None and not (np.isfinite(beta) and float(beta) > 0.0):
            raise ValueError("the likelihood power must be finite and > 0 (got %r)" % (beta,))
        pot = self._power_target()
        with _device_errors():
            _lib.call("pbbi_potential_set_likelihood_power", pot.handle, float(beta), beta_dev, _device.stream_ptr(self.device))

    @property
    def likelihood_power(self):
        """The power as last set from the host (1.0 when never set; NaN when it was last read from the device); for a plain `GLM`
        the power of its twin."""
        out = C.c_double(1.0)
        _lib.call("pbbi_potential_get_likelihood_power", self._power_target(build=False).handle, C.byref(out))
        return out.value


class GLM(_Tempered, _Metric, _GLMBase):
    """-log posterior of the weights of a generalised linear model (see the module text).

        pot = GLM(X, y, family="logistic", prior_precision=1.0)
        pot = GLM(X, counts, family="poisson", offset=np.log(exposure), weights=w,
                  prior_precision=np.r_[0.0, np.full(D - 1, 4.0)])          # flat intercept, tight slopes
        HMC(Ensemble(D, N), 1.0, 0.1, None, potential=pot, rng="philox").getSamples(...)

    `prior_precision` is a scalar or a (D,) vector, `prior_mean` a (D,) vector (default 0); `weights`, `offset` and
    `trials` are (M,) vectors (defaults 1, 0, 1; `trials` with family="logistic" only).  With none of them and a
    scalar precision the potential is the plain model on its own kernels.

    Works wherever a Potential does (HMC in both rng modes, Leapfrog / StormerVerlet, TemperedSMC,
    TemperingLadder).  Arguments are checked on the host before anything touches the GPU."""

    pointwise = _pointwise
    predictive = _predictive
    laplace = _laplace

    def __init__(self, X, y, family="logistic", prior_precision=1.0, prior_mean=None, weights=None, offset=None,
                 trials=None, dtype="float64", device=None):
        X, y, lam, mu, a, o, n = _validate(X, y, family, prior_precision, dtype, prior_mean, weights, offset, trials)
        super().__init__(X.shape[1], dtype, device)
        self.X, self.y, self.family, self.prior_precision = X, y, family, lam
        self.prior_mean, self.weights, self.offset, self.trials = mu, a, o, n
        M, D = X.shape
        self._plain = all(v is None for v in (mu, a, o, n)) and isinstance(lam, float)
        self._twin = None
        if self._plain:
            _lib.call("pbbi_potential_create_glm", D, M, _dptr(X), _dptr(y),
                      FAMILIES[family], lam, self._dt, self.device, C.byref(self._handle))
        else:
            lam_d = np.full(D, lam) if isinstance(lam, float) else lam
            _lib.call("pbbi_potential_create_glm_ex", D, M, _dptr(X), _dptr(y), FAMILIES[family], _dptr(a), _dptr(o),
                      _dptr(n), _dptr(lam_d), _dptr(mu), self._dt, self.device, C.byref(self._handle))

    def _power_target(self, build=True):
        """The potential whose handle carries the likelihood power: this one, or -- the plain model's handle keeps no observation
        streams -- its full-model twin (weights = 1: the same U to rounding, on the full model's kernels), built and cached when
        the potential is first tempered; the twin inherits the metric."""
        if not self._plain:
            return self
        if self._twin is None:
            if not build:
                return self
            self._twin = GLM(self.X, self.y, self.family, self.prior_precision, weights=np.ones(self.y.size),
                             dtype=self.dtype, device=self.device)
            m = self.metric
            if m is not None:
                self._twin.set_metric(m)
        return self._twin

    def set_metric(self, diag):
        super().set_metric(diag)
        if self._twin is not None:
            self._twin.set_metric(diag)


def softmax_layout(D, K):
    """(Dc, NT, row_map) of a K-class model with D coefficients per class, from libpbbi.so (host only, no GPU):
    the padded class size, the number of 16-row tiles of a chain's state in the kernel, and for each of the NT * 16
    internal rows the row of the (K * D, N) state it holds (-1: padding, loads 0 and is never stored).  Class k owns
    internal rows k * Dc .. k * Dc + Dc - 1.  Raises ValueError outside the supported shapes."""
    D, K = int(D), int(K)
    Dc, NT = C.c_int(), C.c_int()
    with _host_errors():
        _lib.call("pbbi_glm_softmax_layout", D, K, C.byref(Dc), C.byref(NT), None)
        row_map = np.empty(NT.value * 16, dtype=np.int32)
        _lib.call("pbbi_glm_softmax_layout", D, K, C.byref(Dc), C.byref(NT), _iptr(row_map))
    return Dc.value, NT.value, row_map


class SoftmaxGLM(_Metric, _GLMBase):
    """-log posterior of the coefficients of K-class (multinomial logistic / softmax) regression:

        U(W) = sum_i [ logsumexp_k(x_i . W_k) - x_i . W_{y_i} ] + 0.5 sum_k sum_d lam_d W_kd^2,   y_i in {0 .. K-1}

        pot = SoftmaxGLM(X, y, classes=None, prior_precision=1.0)      # classes default: int(max(y)) + 1
        hmc = HMC(Ensemble(pot.numDimensions, N), 1.0, 0.1, None, potential=pot, rng="philox")
        W = pot.coefficients(samples)                                  # (K * D, ...) -> (K, D, ...), a view

    All K classes carry coefficients; the Gaussian prior identifies them.  The sampler sees one vector of
    `classes * D` numbers per chain, class-major: w[k * D + d].  `prior_precision` is a scalar or a (D,) vector of
    finite values >= 0, shared by the classes.  A precision of ZERO on a column leaves the posterior improper along
    the direction that shifts that column's coefficient in every class together: the softmax does not see that
    direction, so only the prior can hold it.

    Supported shapes: 2 <= classes <= 8, each class padded to Dc = 16, 32 or 64 rows, classes * Dc <= 128 (D <= 16
    for classes <= 8, D <= 32 for classes <= 4, D <= 64 for classes = 2); float64 only.  Not served: observation
    weights, offsets, multinomial counts, a prior mean, a pinned reference class, classes > 8, per-chain trajectory
    lengths and GIST (they raise as for `GLM`); nothing (U, gradient) is carried between iterations.

    Works wherever `GLM` does (HMC in both rng modes, Leapfrog / StormerVerlet, TemperedSMC, TemperingLadder,
    sampleStats).  Arguments are checked on the host before anything touches the GPU."""

    def __init__(self, X, y, classes=None, prior_precision=1.0, dtype="float64", device=None):
        X, y, M, D = _design(X, y)
        if not (np.all(y >= 0) and np.all(y == np.floor(y))):
            raise ValueError("labels must be integers >= 0")
        K = int(y.max()) + 1 if classes is None else int(classes)
        if classes is not None and K != classes:
            raise ValueError("classes must be an integer")
        if K < 2:
            raise ValueError("softmax regression needs classes >= 2 (classes = %d)" % K)
        if not np.all(y < K):
            raise ValueError("labels must be < classes = %d" % K)
        lam = _precision_vector(prior_precision, D)
        softmax_layout(D, K)   # the shape rule, stated once: in libpbbi.so (host only); raises ValueError
        _float64_only(dtype)
        super().__init__(K * D, dtype, device)
        self.X, self.y, self.classes, self.prior_precision = X, y, K, lam
        self.family = "softmax"
        _lib.call("pbbi_potential_create_glm_softmax", D, K, M, _dptr(X), _dptr(y), _dptr(lam), self._dt, self.device,
                  C.byref(self._handle))

    def pointwise(self, samples, ranges=0):
        """Not built for the softmax family (GLM, DispersionGLM, HierarchicalGLM and HierarchicalDispersionGLM have it)."""
        raise ValueError("not built")

    def coefficients(self, samples):
        """(K * D, ...) -> (K, D, ...): the leading axis of a state, sample or gradient array split by class (a view
        wherever the array allows one)."""
        D = self.numDimensions // self.classes
        return samples.reshape((self.classes, D) + tuple(samples.shape[1:]))


def _validate_dispersion(X, y, family, weights, offset):
    """X, y and the per-observation vectors of a dispersion family, checked: (X, y, weights, offset) as float64 arrays."""
    _known_family(family, DISPERSION_FAMILIES)
    X, y, M, D = _design(X, y)
    if family == "negbinomial" and not (np.all(y >= 0) and np.all(y == np.floor(y))):
        raise ValueError("negbinomial: y must hold non-negative integers")
    if family == "gamma" and not np.all(y > 0):
        raise ValueError("gamma: y must be > 0")
    return (X, y) + _obs_vectors(weights, offset, M)


def _dispersion_args(dispersion, log_dispersion_prior):
    """`dispersion` and `log_dispersion_prior` checked: (sample, held value or None, theta, prior pair or None)."""
    sample = isinstance(dispersion, str)
    if sample:
        if dispersion != "sample":
            raise ValueError('dispersion must be "sample" or a float > 0 (got %r)' % (dispersion,))
        m_t, l_t = (0.0, 0.25) if log_dispersion_prior is None else _pair(log_dispersion_prior)
        if not (np.isfinite(m_t) and np.isfinite(l_t) and l_t >= 0):
            raise ValueError("log_dispersion_prior must be (mean, precision) with a finite mean and a finite precision >= 0")
        theta = 0.0
    else:
        if log_dispersion_prior is not None:
            raise ValueError("log_dispersion_prior belongs to dispersion=\"sample\" only: a held dispersion has no prior")
        try:
            disp = float(dispersion)
        except (TypeError, ValueError):
            raise ValueError('dispersion must be "sample" or a float > 0 (got %r)' % (dispersion,)) from None
        if not (np.isfinite(disp) and disp > 0):
            raise ValueError("a held dispersion must be finite and > 0 (got %r)" % (dispersion,))
        theta = float(np.log(disp))
    return sample, (None if sample else disp), theta, ((m_t, l_t) if sample else None)


class DispersionGLM(_Tempered, _Metric, _GLMBase):
    """-log posterior of a GLM whose family has a free dispersion, with theta = log(dispersion):

        gaussian     y_i ~ N(eta_i, sigma^2 / a_i), sigma = exp(theta):
                     U_i = a_i [ 0.5 exp(-2 theta) (y_i - eta_i)^2 + theta ]
        negbinomial  y_i ~ NB2(mu_i = exp(eta_i), phi = exp(theta)), Var = mu + mu^2 / phi, y non-negative integers:
                     U_i = a_i [ lgamma(phi) - lgamma(y_i + phi) - phi theta - y_i eta_i + (y_i + phi) logaddexp(eta_i, theta) ]
        gamma        y_i ~ Gamma(shape alpha = exp(theta), mean mu_i = exp(eta_i)), Var = mu^2 / alpha, y > 0; z_i = eta_i - log y_i:
                     U_i = a_i [ lgamma(alpha) - alpha theta + alpha (z_i + exp(-z_i)) ]
        U = sum_i U_i + 0.5 sum_d lam_d (w_d - mu_d)^2 + 0.5 lam_theta (theta - m_theta)^2,    eta_i = x_i . w + o_i

    (constants that depend on neither w nor theta dropped; the theta prior only when theta is sampled).

        pot = DispersionGLM(X, counts, family="negbinomial", dispersion="sample", log_dispersion_prior=(0.0, 0.25))
        hmc = HMC(Ensemble(pot.numDimensions, N), 1.0, 0.05, None, potential=pot, rng="philox")
        w, phi = pot.split(samples)             # (D, ...) coefficients and exp(theta): sigma resp. phi
        pot = DispersionGLM(X, y, family="gaussian", dispersion=0.7)      # sigma held at 0.7: the state is w alone
        pot = DispersionGLM(X, cost, family="gamma", offset=np.log(exposure))   # positive, right-skewed data; the shape sampled
        pot = DispersionGLM(X, duration, family="gamma", dispersion=1.0)  # shape 1: exponential regression

    `dispersion="sample"`: theta is the LAST component of the chain's state, numDimensions == D + 1, and
    `log_dispersion_prior=(mean, precision >= 0)` is theta's Gaussian prior (default (0, 0.25); precision 0 = flat in
    theta, p(sigma) proportional to 1 / sigma).  `dispersion=` a float > 0: sigma, phi resp. alpha is held there, numDimensions
    == D, and `log_dispersion_prior` must not be given.  `prior_precision` is a scalar or a (D,) vector, `prior_mean` a
    (D,) vector (default 0), `weights` (>= 0; a row of weight 0 is held out exactly) and `offset` (M,) vectors.

    Shapes: float64; the state dimension is at most 128 for "gaussian" and "gamma" and at most 64 for "negbinomial" (the
    negative binomial's kernel for 65 .. 128 rows cannot be built without register spills to memory and is not shipped).
    As with phi, a large alpha means little dispersion.  The device keeps log y for "gamma" (the kernels need nothing else
    of y); an exp(-z_i) that overflows rejects the proposal, like Poisson's exp(eta).

    Works wherever `GLM` does (HMC in both rng modes, Leapfrog / StormerVerlet, TemperedSMC, TemperingLadder,
    sampleStats); per-chain trajectory lengths and GIST raise as for `GLM`.  Arguments are checked on the host before
    anything touches the GPU.  It runs on csrc/kernels_glm.hip (FAM = 3, 4, 5 of k_glm<NT, FAM, true>)."""

    pointwise = _pointwise
    predictive = _predictive
    laplace = _laplace

    def __init__(self, X, y, family="negbinomial", dispersion="sample", log_dispersion_prior=None, prior_precision=1.0,
                 prior_mean=None, weights=None, offset=None, dtype="float64", device=None):
        X, y, weights, offset = _validate_dispersion(X, y, family, weights, offset)
        M, D = X.shape
        sample, disp, theta, tprior = _dispersion_args(dispersion, log_dispersion_prior)
        lam = _precision_vector(prior_precision, D)
        mu = np.zeros(D) if prior_mean is None else _vector(prior_mean, D, "prior_mean", "D")
        Dt = D + 1 if sample else D
        if Dt > DISPERSION_MAX_DIM[family]:
            raise ValueError("DispersionGLM(family=%r) serves a state dimension (coefficients%s) <= %d (got %d)"
                             % (family, " + 1 for the sampled dispersion" if sample else "", DISPERSION_MAX_DIM[family], Dt))
        _float64_only(dtype)
        super().__init__(Dt, dtype, device)
        self.X, self.y, self.family, self.weights, self.offset = X, y, family, weights, offset
        self.prior_precision, self.prior_mean = lam, mu
        self.sampled = sample
        self.dispersion = "sample" if sample else disp
        self.log_dispersion_prior = tprior
        self.numCoefficients = D
        lam_t = np.ascontiguousarray(np.r_[lam, tprior[1]] if sample else lam)
        mu_t = np.ascontiguousarray(np.r_[mu, tprior[0]] if sample else mu)
        _lib.call("pbbi_potential_create_glm_dispersion", D, M, _dptr(X), _dptr(y), DISPERSION_FAMILIES[family],
                  _dptr(weights), _dptr(offset), _dptr(lam_t), _dptr(mu_t), int(sample), theta, self._dt, self.device,
                  C.byref(self._handle))

    def split(self, samples):
        """(numDimensions, ...) -> (w, dispersion): the (D, ...) coefficients (a view wherever the array allows one) and
        exp(theta) -- sigma for "gaussian", phi for "negbinomial", the shape alpha for "gamma" -- of shape (...); held: the
        constant itself."""
        D = self.numCoefficients
        if not self.sampled:
            return samples, self.dispersion
        theta = samples[D]
        return samples[:D], _exp(theta)


ORDINAL_MAX_CATEGORIES = 8
# the largest state dimension (coefficients + K - 1 cutpoint rows) an ordinal kernel is shipped for (glm_max_dim of
# csrc/glm_host.cpp, profiles/glm_ordinal_resources.txt)
ORDINAL_MAX_DIM = 64


def _cutpoint_prior(v, K):
    """`cutpoint_prior` checked: a (K - 1, 2) array of (mean, precision) -- row 0 of zeta_1 = kappa_1, rows 1 .. K-2 of the
    log-gaps.  Given as ((m1, l1), (mg, lg)): one pair for the first cutpoint and one for every log-gap; or (K - 1, 2)."""
    a = np.asarray(v, dtype=np.float64)
    if a.shape == (2, 2) and K - 1 != 2:      # (K = 3: the two readings agree)
        a = np.vstack([a[:1], np.repeat(a[1:], K - 2, axis=0)])
    if a.shape != (K - 1, 2):
        raise ValueError("cutpoint_prior must be ((mean, precision) of the first cutpoint, (mean, precision) of the log-gaps) "
                         "or a (K - 1, 2) array of such pairs (K - 1 = %d; shape %s)" % (K - 1, a.shape))
    if not (np.all(np.isfinite(a)) and np.all(a[:, 1] >= 0)):
        raise ValueError("cutpoint_prior must hold finite means and finite precisions >= 0")
    return a


class OrdinalGLM(_Tempered, _Metric, _GLMBase):
    """-log posterior of ordinal (cumulative-logit, proportional-odds) regression: ordered categories y_i in {0 .. K-1} -- Likert
    items, grades, severity scores -- with cutpoints kappa_1 < .. < kappa_{K-1} (kappa_0 = -inf, kappa_K = +inf):

        P(y_i = k) = sigma(kappa_{k+1} - eta_i) - sigma(kappa_k - eta_i),    eta_i = x_i . w + o_i

        pot = OrdinalGLM(X, stars)                          # categories = max(y) + 1
        hmc = HMC(Ensemble(pot.numDimensions, N), 1.0, 0.05, None, potential=pot, rng="philox")
        w, kappa = pot.split(samples)                       # (D, ...) coefficients, (K - 1, ...) ordered cutpoints
        q0 = pot.unconstrain(w0, kappa0)                    # starting values from the natural scale

    X carries NO intercept column: the cutpoints are the intercepts (a column of ones is not identified against them; X is
    not tested for one).  The chain's state is [w (D rows); zeta (K - 1 rows)], numDimensions == D + K - 1, the cutpoint rows
    last and unconstrained: zeta_1 = kappa_1, zeta_j = log(kappa_j - kappa_{j-1}), so the ordering holds by construction.
    The priors are Gaussian on these rows and stated on zeta (no Jacobian term): `cutpoint_prior` is ((mean, precision) of
    the first cutpoint, (mean, precision) of every log-gap), default ((0, 0.1), (0, 1)) -- kappa_1 ~ N(0, 10), each gap
    log-normal around 1 -- or a (K - 1, 2) array of pairs, one per row.  `categories=None` takes int(max(y)) + 1; 2 <= K <= 8,
    and a category without observations is allowed.  `prior_precision` is a scalar or a (D,) vector, `prior_mean` a (D,)
    vector (default 0), `weights` (>= 0; a row of weight 0 is held out exactly) and `offset` (M,) vectors.  K = 2 is logistic
    regression with intercept -kappa_1.

    `pointwise` reports the expected category sum_j P(y_i >= j) as `mu_i`.  Works wherever `GLM` does (HMC in both rng modes,
    Leapfrog / StormerVerlet, the diagonal metric and `adaptMassMatrix`, `loglik`, `LikelihoodTemperedSMC`); per-chain
    trajectory lengths and GIST raise as for `GLM`; random effects are not built for this family.  float64; the state
    dimension is at most ORDINAL_MAX_DIM.  It runs on csrc/kernels_glm.hip (FAM = 6 of k_glm<NT, FAM, true>)."""

    family = "ordinal"
    pointwise = _pointwise
    predictive = _predictive

    def __init__(self, X, y, categories=None, prior_precision=1.0, prior_mean=None, weights=None, offset=None,
                 cutpoint_prior=((0.0, 0.1), (0.0, 1.0)), dtype="float64", device=None):
        X, y, M, D = _design(X, y)
        K = int(np.max(y)) + 1 if categories is None else int(categories)
        if categories is None and K < 2:
            K = 2
        if not 2 <= K <= ORDINAL_MAX_CATEGORIES:
            raise ValueError("OrdinalGLM serves 2 <= categories <= %d (got %d)" % (ORDINAL_MAX_CATEGORIES, K))
        if not (np.all(y >= 0) and np.all(y < K) and np.all(y == np.floor(y))):
            raise ValueError("ordinal: y must hold integer categories in [0, %d)" % K)
        weights, offset = _obs_vectors(weights, offset, M)
        lam = _precision_vector(prior_precision, D)
        mu = np.zeros(D) if prior_mean is None else _vector(prior_mean, D, "prior_mean", "D")
        cp = _cutpoint_prior(cutpoint_prior, K)
        Dt = D + K - 1
        if Dt > ORDINAL_MAX_DIM:
            raise ValueError("OrdinalGLM serves a state dimension (coefficients + categories - 1) <= %d (got %d)"
                             % (ORDINAL_MAX_DIM, Dt))
        _float64_only(dtype)
        super().__init__(Dt, dtype, device)
        self.X, self.y, self.weights, self.offset = X, y, weights, offset
        self.prior_precision, self.prior_mean = lam, mu
        self.categories, self.cutpoint_prior, self.numCoefficients = K, cp, D
        lam_t = np.ascontiguousarray(np.r_[lam, cp[:, 1]])
        mu_t = np.ascontiguousarray(np.r_[mu, cp[:, 0]])
        _lib.call("pbbi_potential_create_glm_ordinal", D, K, M, _dptr(X), _dptr(y), _dptr(weights), _dptr(offset), _dptr(lam_t),
                  _dptr(mu_t), self._dt, self.device, C.byref(self._handle))

    def split(self, samples):
        """(numDimensions, ...) -> (w, cutpoints): the (D, ...) coefficients (a view wherever the array allows one) and the
        (K - 1, ...) cutpoints on the natural, ordered scale: kappa_j = zeta_1 + sum_{m = 2 .. j} exp(zeta_m)."""
        D = self.numCoefficients
        z = samples[D:self.numDimensions]
        if isinstance(z, np.ndarray):
            return samples[:D], np.cumsum(np.concatenate([z[:1], np.exp(z[1:])], axis=0), axis=0)
        from . import _device
        t = _device.torch()
        return samples[:D], t.cumsum(t.cat([z[:1], z[1:].exp()], dim=0), dim=0)

    def unconstrain(self, w, cutpoints):
        """The inverse of `split`, for starting values: (D, ...) coefficients and (K - 1, ...) strictly increasing cutpoints ->
        the (numDimensions, ...) state [w; kappa_1; log(kappa_j - kappa_{j-1})] (NumPy)."""
        w, k = np.asarray(w, dtype=np.float64), np.asarray(cutpoints, dtype=np.float64)
        if w.shape[0] != self.numCoefficients or k.shape[0] != self.categories - 1 or w.shape[1:] != k.shape[1:]:
            raise ValueError("unconstrain: w must be (%d, ...) and cutpoints (%d, ...) with the same trailing shape"
                             % (self.numCoefficients, self.categories - 1))
        gaps = np.diff(k, axis=0)
        if not (np.all(np.isfinite(k)) and np.all(gaps > 0)):
            raise ValueError("unconstrain: the cutpoints must be finite and strictly increasing")
        return np.concatenate([w, k[:1], np.log(gaps)], axis=0)


def _pair(v):
    try:
        a, b = v
        return float(a), float(b)
    except (TypeError, ValueError):
        raise ValueError("log_dispersion_prior must be a pair (mean, precision)") from None


def _groups_vector(groups, D):
    g = np.asarray(groups)
    if g.ndim != 1 or g.size != D:
        raise ValueError("groups must be 1-D with D = %d entries (shape %s)" % (D, g.shape))
    if g.dtype.kind not in "iu":
        gf = np.asarray(g, dtype=np.float64)
        if not (np.all(np.isfinite(gf)) and np.all(gf == np.floor(gf))):
            raise ValueError("groups must hold integers: -1 (fixed prior) or a group index")
        g = gf
    g = g.astype(np.int64)
    if np.any(g < -1):
        raise ValueError("groups must hold -1 (fixed prior) or a group index >= 0 (got %d)" % g.min())
    J = int(g.max()) + 1
    if J < 1:
        raise ValueError("groups names no group (all -1): that model is GLM")
    if J > HIER_MAX_GROUPS:
        raise ValueError("at most %d groups are served (group index %d)" % (HIER_MAX_GROUPS, J - 1))
    missing = [j for j in range(J) if not np.any(g == j)]
    if missing:
        raise ValueError("every group index 0 .. %d must be used (unused: %s)" % (J - 1, missing))
    return np.ascontiguousarray(g, dtype=np.int32), J


def _log_scale_prior(v, J):
    a = np.asarray(v, dtype=np.float64)
    if a.shape == (2,):
        a = np.tile(a, (J, 1))
    if a.shape != (J, 2):
        raise ValueError("log_scale_prior must be one pair (mean, precision) or J = %d pairs (shape %s)" % (J, a.shape))
    if not (np.all(np.isfinite(a)) and np.all(a[:, 1] >= 0)):
        raise ValueError("log_scale_prior: finite means and finite precisions >= 0")
    return np.ascontiguousarray(a)


def _hier_prior(D, groups, log_scale_prior, prior_precision, prior_mean):
    """groups (int32), J, the (J, 2) log-scale priors, lam (D,) with 0 at the grouped coefficients, mu (D,)."""
    groups, J = _groups_vector(groups, D)
    try:
        tp = _log_scale_prior(log_scale_prior, J)
    except (TypeError, ValueError) as e:
        raise ValueError(str(e) if "log_scale_prior" in str(e) else
                         "log_scale_prior must be one pair (mean, precision) or J pairs") from None
    lam = np.asarray(prior_precision, dtype=np.float64)
    if lam.ndim == 0:
        lam = np.full(D, float(lam))
    elif lam.ndim != 1 or lam.size != D:
        raise ValueError("prior_precision must be a scalar or 1-D with D = %d entries (shape %s)" % (D, lam.shape))
    lam = np.where(groups >= 0, 0.0, lam)          # the entries of grouped coefficients are ignored
    if not (np.all(np.isfinite(lam)) and np.all(lam >= 0)):
        raise ValueError("every prior_precision of an ungrouped coefficient must be finite and >= 0")
    mu = np.zeros(D) if prior_mean is None else _vector(prior_mean, D, "prior_mean", "D")
    return groups, J, tp, np.ascontiguousarray(lam), mu


def _hier_args(parametrisation, groups):
    """The two arguments both hierarchical constructors ask for before they look at the data."""
    if not isinstance(parametrisation, str) or parametrisation not in HIER_PARAMETRISATIONS:
        raise ValueError("parametrisation must be \"centred\" or \"noncentred\" (got %r)" % (parametrisation,))
    if groups is None:
        raise ValueError("groups is required: a (D,) vector of -1 (fixed prior) or group indices 0 .. J-1")


def pack_prior_groups(groups, log_scale_prior=(0.0, 1.0), prior_precision=1.0, prior_mean=None):
    """The prior table a HierarchicalGLM handle keeps on the device and its kernel in LDS, computed (and checked) on the
    host by libpbbi.so: (table, n) -- table (2, DP) with DP = padded_dim(D + J): row 0 the `lam` slots (a fixed
    coefficient's precision, -(j + 1) for a member of group j, the precision of t_j's prior at D + j), row 1 the means
    (mu_d, the mean of t_j's prior at D + j), zeros past D + J; n (J,) the members of each group."""
    D = np.asarray(groups).size
    groups, J, tp, lam, mu = _hier_prior(D, groups, log_scale_prior, prior_precision, prior_mean)
    DP = padded_dim(D + J)
    out, n = np.empty(2 * DP, dtype=np.float64), np.empty(J, dtype=np.float64)
    with _host_errors():
        _lib.call("pbbi_glm_pack_prior_groups", D, J, _dptr(lam), _dptr(mu), _iptr(groups), _dptr(tp), _dptr(out), _dptr(n))
    return out.reshape(2, DP), n


def _penalty_blocks(penalty, penalty_rank, groups, J):
    """(blocks, ranks, full): the J checked and symmetrised matrices (None for an exchangeable group), the J ranks (n_j for an
    exchangeable group) and the (D, D) matrix in coefficient indexing the C ABI takes (identity on exchangeable groups, zero
    on fixed rows and between groups) -- or (None, None, None) when no group has a penalty."""
    if penalty is None:
        if penalty_rank is not None:
            raise ValueError("penalty_rank belongs to a penalty: none is given")
        return None, None, None
    if isinstance(penalty, dict):
        for j in penalty:
            if not (isinstance(j, (int, np.integer)) and 0 <= j < J):
                raise ValueError("penalty is given for group %r, which is not used (groups 0 .. %d)" % (j, J - 1))
        blocks = [penalty.get(j) for j in range(J)]
    else:
        try:
            blocks = list(penalty)
        except TypeError:
            raise ValueError("penalty must be a dict {group: matrix} or a length-J sequence with None for exchangeable "
                             "groups") from None
        if len(blocks) != J:
            raise ValueError("penalty must have one entry per group used, J = %d (got %d): None for an exchangeable group"
                             % (J, len(blocks)))
    if isinstance(penalty_rank, dict):
        for j in penalty_rank:
            if not (isinstance(j, (int, np.integer)) and 0 <= j < J):
                raise ValueError("penalty_rank is given for group %r, which is not used (groups 0 .. %d)" % (j, J - 1))
        given = [penalty_rank.get(j) for j in range(J)]
    elif penalty_rank is None:
        given = [None] * J
    else:
        try:
            given = list(penalty_rank)
        except TypeError:
            raise ValueError("penalty_rank must be a dict {group: rank} or a length-J sequence") from None
        if len(given) != J:
            raise ValueError("penalty_rank must have one entry per group used, J = %d (got %d)" % (J, len(given)))
    if all(b is None for b in blocks):
        if any(r is not None for r in given):
            raise ValueError("penalty_rank belongs to a penalty: none is given")
        return None, None, None
    D = groups.size
    full = np.zeros((D, D))
    ranks = np.zeros(J, dtype=np.int64)
    out = []
    for j in range(J):
        idx = np.flatnonzero(groups == j)
        n = idx.size
        if blocks[j] is None:
            if given[j] is not None:
                raise ValueError("penalty_rank[%d] is given for a group without a penalty" % j)
            full[idx, idx] = 1.0
            ranks[j] = n
            out.append(None)
            continue
        try:
            Q = np.array(blocks[j], dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("penalty[%d] must be an (n_j, n_j) matrix of numbers" % j) from None
        if Q.shape != (n, n):
            raise ValueError("penalty[%d] must be (n_j, n_j) = (%d, %d), ordered as the members of the group by column "
                             "(shape %s)" % (j, n, n, Q.shape))
        if not np.all(np.isfinite(Q)):
            raise ValueError("penalty[%d] must be finite" % j)
        big = float(np.max(np.abs(Q)))
        if big == 0.0:
            raise ValueError("penalty[%d] is the zero matrix: no prior at all" % j)
        if float(np.max(np.abs(Q - Q.T))) > 1e-12 * big:
            raise ValueError("penalty[%d] must be symmetric (max|Q - Q^T| <= 1e-12 max|Q|)" % j)
        Q = 0.5 * (Q + Q.T)
        ev = np.linalg.eigvalsh(Q)
        if not (ev[-1] > 0.0 and ev[0] >= -1e-10 * ev[-1]):
            raise ValueError("penalty[%d] must be positive semi-definite (smallest eigenvalue %.3g, largest %.3g)"
                             % (j, ev[0], ev[-1]))
        if given[j] is None:
            r = int(np.sum(ev > 1e-10 * ev[-1]))
        else:
            r = given[j]
            if isinstance(r, (bool, np.bool_)) or not isinstance(r, (int, np.integer, float, np.floating)) \
                    or not np.isfinite(r) or r != int(r) or not 1 <= int(r) <= n:
                raise ValueError("penalty_rank[%d] must be an integer in 1 .. n_j = %d (got %r)" % (j, n, r))
            r = int(r)
        full[np.ix_(idx, idx)] = Q
        ranks[j] = r
        out.append(Q)
    return out, ranks, np.ascontiguousarray(full)


def pack_penalty(penalty, J):
    """The image of the penalty a HierarchicalGLM handle with structured group priors keeps on the device and its kernel in
    LDS, computed on the host by libpbbi.so (no GPU involved).  `penalty` is the (D, D) matrix in coefficient indexing (Q_j on
    the members of group j, the identity on an exchangeable group, zero on fixed rows and between groups), `J` the number of
    groups.  Returns an array (DP/16, DP/8, 64, 2) with DP = padded_dim(D + J): per block t of 16 rows of Q the A fragments of
    the product Q_t . (w - mu) in the order of `pack_design`'s first product, [s2][lane][e] = Q[16 t + (lane & 15)][4 (2 s2 +
    e) + (lane >> 4)]; rows and columns >= D are zero."""
    Q = np.ascontiguousarray(penalty, dtype=np.float64)
    if Q.ndim != 2 or Q.shape[0] != Q.shape[1] or Q.shape[0] < 1:
        raise ValueError("penalty must be a square (D, D) matrix (shape %s)" % (Q.shape,))
    D, J = Q.shape[0], int(J)
    if not 1 <= J <= HIER_MAX_GROUPS:
        raise ValueError("J must be 1 .. %d (got %d)" % (HIER_MAX_GROUPS, J))
    DP = padded_dim(D + J)
    return _pack("pbbi_glm_pack_penalty", (D, J), (Q,)).reshape(DP // 16, DP // 8, 64, 2)


class HierarchicalGLM(_Tempered, _Metric, _GLMBase):
    """-log posterior of a GLM (family "logistic" or "poisson", the full model of `GLM`: weights a_i, trials n_i,
    offsets o_i, eta_i = x_i . w + o_i) in which blocks of coefficients share a prior scale that is sampled:

        U(w, t) = sum_i a_i [ n_i b(eta_i) - y_i eta_i ]
                + 0.5 sum_{d: groups_d < 0} lam_d (w_d - mu_d)^2
                + sum_j [ 0.5 exp(-2 t_j) S_j + n_j t_j + 0.5 lam_tj (t_j - m_tj)^2 ]
        S_j = sum_{d: groups_d = j} (w_d - mu_d)^2,    n_j = #{d: groups_d = j}

    i.e. w_d | t_j ~ N(mu_d, sigma_j^2) with sigma_j = exp(t_j) and t_j ~ N(m_tj, 1 / lam_tj): random intercepts per
    school or batch (one-hot columns of X in one group), random slopes, a ridge penalty of unknown strength.

        groups = np.r_[-1, -1, np.zeros(12, int)]                    # two fixed coefficients, twelve random intercepts
        pot = HierarchicalGLM(X, y, family="logistic", groups=groups, log_scale_prior=(0.0, 1.0))
        hmc = HMC(Ensemble(pot.numDimensions, N), 1.0, 0.05, None, potential=pot, rng="philox")
        w, scales = pot.split(samples)                               # (D, ...) coefficients, (J, ...) sigma_j = exp(t_j)
        pot = HierarchicalGLM.with_random_intercepts(X, y, labels)   # appends the one-hot columns itself

    `groups` is a (D,) vector of -1 (the coefficient keeps its fixed prior `prior_precision` / `prior_mean`, as in
    `GLM`) or a group index 0 .. J-1; every index must be used, 1 <= J <= 4.  The chain's state has D + J rows: the
    coefficients, then t_0 .. t_{J-1}; numDimensions == D + J.  `log_scale_prior` is one pair (mean, precision >= 0)
    for all groups or J pairs.  The `prior_precision` entries of grouped coefficients are IGNORED (their precision is
    exp(-2 t_j)); their `prior_mean` entries are used.  `weights`, `offset`, `trials` as for `GLM`.

    That is the CENTRED parametrisation (`parametrisation="centred"`, the default), sampled on the log scale.  Where the
    data say little about a group's coefficients (few observations per level, a weak likelihood) the posterior is a funnel:
    small t_j with all members near their means is a narrow neck no single step size serves, and the chains under-sample
    it.  `parametrisation="noncentred"` cures it: on a grouped row the chain holds z_d in place of w_d,

        w_d = mu_d + exp(t_j) z_d,    z_d ~ N(0, 1) a priori
        U(z, t) = sum_i a_i [ n_i b(eta_i) - y_i eta_i ]  (at w(z, t))
                + 0.5 sum_{d: groups_d < 0} lam_d (w_d - mu_d)^2 + 0.5 sum_{d: groups_d >= 0} z_d^2
                + sum_j 0.5 lam_tj (t_j - m_tj)^2

    the same posterior in other coordinates: U_nc(z, t) = U_c(w(z, t), t) - sum_j n_j t_j, the n_j t_j being the Jacobian
    of the change of variables.  Fixed rows and the t rows are as above.  Which to choose: weak data per level (few
    observations, random intercepts of small groups) -- non-centred; many observations per level -- centred (there the
    likelihood pins w_d, and z_d = (w_d - mu_d) exp(-t_j) is what becomes a funnel).  The scaling runs inside the kernel,
    on a copy of the state (k_glm<NT, FAM, true, GLM_HIER_NC>).  The sampler's states, `getSamples`' output, `sampleStats`
    and `RunningStats` of a non-centred potential are in SAMPLER coordinates (z on the grouped rows); `to_natural` maps
    them to (w; t), `from_natural` back, and `split` returns w and the scales on the natural scale for both forms.

    Structured group priors (`penalty=`, centred only).  The priors above are exchangeable: independent members.  With a
    symmetric positive semi-definite matrix Q_j in the quadratic form of group j,

        w_j - mu_j | t_j ~ N(0, exp(2 t_j) Q_j^-),    d_j = (w_d - mu_d) over the members of j in increasing column order
        U(w, t) = ... + sum_j [ 0.5 exp(-2 t_j) d_j^T Q_j d_j + r_j t_j + 0.5 lam_tj (t_j - m_tj)^2 ],    r_j = rank(Q_j)

    the same class serves penalised splines and additive models (a difference penalty, the smoothing parameter sampled),
    random-walk effects over time, ICAR spatial effects and any correlated effect given by a precision matrix:

        groups = np.r_[-1, np.zeros(12, int)]                                              # an intercept, twelve months
        pot = HierarchicalGLM(X, y, groups=groups, penalty={0: HierarchicalGLM.random_walk_penalty(12, 2)})
        pot = HierarchicalGLM.with_random_intercepts(X, y, region, penalty=HierarchicalGLM.icar_penalty(adjacency))

    `penalty` is a dict {j: Q_j} or a length-J sequence with None for the groups that stay exchangeable (Q_j = I, r_j = n_j:
    the model above exactly); Q_j is (n_j, n_j), finite, symmetric to 1e-12 of its largest entry (it is then symmetrised),
    positive semi-definite (smallest eigenvalue >= -1e-10 of the largest) and not zero.  It may be rank deficient (an
    improper prior, as RW2 and ICAR are: the data or a fixed row must then pin the null space).  `penalty_rank` gives r_j
    (same forms, an integer in 1 .. n_j); by default it is the number of eigenvalues above 1e-10 of the largest
    (`numpy.linalg.eigvalsh`).  `penalty=None`, or None for every group, is the exchangeable model on the kernels and with
    the bits it always had.  `pot.penalty` (the J symmetrised matrices or None) and `pot.penalty_rank` are kept.  Helpers, all
    on the host: `HierarchicalGLM.random_walk_penalty(n, order)`, `HierarchicalGLM.icar_penalty(adjacency)`, and
    `glm.pack_penalty` (the image the kernel keeps in LDS).  Q_j (w - mu) is one more product on the matrix cores per
    gradient evaluation (k_glm<NT, FAM, true, GLM_HIER_Q>), the matrix resident in LDS; D + J <= 64 (`HIER_Q_MAX_DIM`).
    Not served with a penalty: `parametrisation="noncentred"` (it would need w = mu + exp(t) L^-T z with Q = L L^T),
    structure across groups, sampled structure such as the rho of a proper CAR prior.

    Not served: a per-group choice of parametrisation, sampled group scales on `SoftmaxGLM` (for the families of
    `DispersionGLM` they are `HierarchicalDispersionGLM`), more than 4 groups, group means as parameters, per-chain trajectory lengths and GIST (they raise as for `GLM`).  Shapes:
    float64; D + J <= 64 for both families and both parametrisations (`HIER_MAX_DIM`, `HIER_NC_MAX_DIM`: the kernels for
    65 .. 128 rows cannot be built without register spills to memory and are not shipped).

    Works wherever `GLM` does (HMC in both rng modes, Leapfrog / StormerVerlet, TemperedSMC, TemperingLadder,
    sampleStats).  Arguments are checked on the host before anything touches the GPU.  It runs on csrc/kernels_glm.hip
    (k_glm<NT, FAM, true, HIER>)."""

    pointwise = _pointwise
    predictive = _predictive

    def __init__(self, X, y, family="logistic", groups=None, log_scale_prior=(0.0, 1.0), prior_precision=1.0,
                 prior_mean=None, weights=None, offset=None, trials=None, dtype="float64", device=None,
                 parametrisation="centred", penalty=None, penalty_rank=None):
        _hier_args(parametrisation, groups)
        # X, y and the per-observation vectors: GLM's rules (the prior is checked below, with the groups)
        X, y, _, _, a, o, n = _validate(X, y, family, 0.0, dtype, None, weights, offset, trials)
        M, D = X.shape
        groups, J, tp, lam, mu = _hier_prior(D, groups, log_scale_prior, prior_precision, prior_mean)
        Qs, ranks, Qfull = _penalty_blocks(penalty, penalty_rank, groups, J)
        if Qs is not None and parametrisation != "centred":
            raise ValueError("penalty is served by parametrisation=\"centred\" only (the non-centred form of a structured "
                             "prior, w = mu + exp(t) L^-T z, is not built)")
        dmax = (HIER_Q_MAX_DIM if Qs is not None else HIER_NC_MAX_DIM if parametrisation == "noncentred" else HIER_MAX_DIM)[family]
        if D + J > dmax:
            raise ValueError("HierarchicalGLM(family=%r) serves a state dimension (coefficients + groups) <= %d (got %d + %d)"
                             % (family, dmax, D, J))
        self._set_hier_state(D + J, dtype, device, parametrisation, X, y, family, a, o, n, lam, mu, groups, tp, Qs, ranks)
        model = (D, M, _dptr(X), _dptr(y), FAMILIES[family], _dptr(a), _dptr(o), _dptr(n), _dptr(lam), _dptr(mu), _iptr(groups),
                 J, _dptr(tp))
        where = (self._dt, self.device, C.byref(self._handle))
        if Qs is not None:
            rk = np.ascontiguousarray(ranks, dtype=np.float64)
            _lib.call("pbbi_potential_create_glm_hier_q", *model, _dptr(Qfull), _dptr(rk), *where)
        elif parametrisation == "centred":    # the entry point, and so the kernel, every call had before the keyword existed
            _lib.call("pbbi_potential_create_glm_hier", *model, *where)
        else:
            _lib.call("pbbi_potential_create_glm_hier_ex", *model, HIER_PARAMETRISATIONS[parametrisation], *where)

    def _set_hier_state(self, Dt, dtype, device, parametrisation, X, y, family, weights, offset, trials, lam, mu, groups, tp,
                        penalty=None, ranks=None):
        """Potential's own state (Dt rows) and the attributes every hierarchical potential carries."""
        Potential.__init__(self, Dt, dtype, device)
        self.parametrisation = parametrisation
        self.X, self.y, self.family = X, y, family
        self.weights, self.offset, self.trials = weights, offset, trials
        self.prior_precision, self.prior_mean = lam, mu
        self.groups, self.log_scale_prior = groups, tp
        self.numCoefficients, self.numGroups = groups.size, tp.shape[0]
        self.levels = None
        self.penalty, self.penalty_rank = penalty, ranks

    def _scale_and_mean(self, q):
        """(exp(t) of each row's group, mu) shaped to broadcast against q[:D], in q's own array type; and the grouped mask."""
        D, J = self.numCoefficients, self.numGroups
        grouped = np.asarray(self.groups) >= 0
        idx = np.where(grouped, self.groups, 0).astype(np.int64)
        mu = np.asarray(self.prior_mean, dtype=np.float64).reshape((D,) + (1,) * (q.ndim - 1))
        mask = grouped.reshape(mu.shape)
        if isinstance(q, np.ndarray):
            return np.exp(q[D:D + J])[idx], mu, mask, np.where
        import torch
        dev = dict(device=q.device)
        return (q[D:D + J].exp()[torch.as_tensor(idx, **dev)], torch.as_tensor(mu, dtype=q.dtype, **dev),
                torch.as_tensor(mask, **dev), torch.where)

    def to_natural(self, q):
        """A sampler state (numDimensions, ...) -> (w; t), the centred state: w_d = mu_d + exp(t_j) z_d on the grouped rows
        of a non-centred potential, everything else as it is.  NumPy arrays and torch tensors (device tensors with torch
        ops) of any trailing shape; a new array.  The identity (a copy) for "centred"."""
        out = q.copy() if isinstance(q, np.ndarray) else q.clone()
        if self.parametrisation == "centred":
            return out
        D = self.numCoefficients
        sig, mu, mask, where = self._scale_and_mean(q)
        out[:D] = where(mask, mu + sig * q[:D], q[:D])
        return out

    def from_natural(self, qc):
        """The inverse of `to_natural`: (w; t) -> the sampler's state, z_d = (w_d - mu_d) exp(-t_j) on the grouped rows of
        a non-centred potential.  A new array; the identity (a copy) for "centred"."""
        out = qc.copy() if isinstance(qc, np.ndarray) else qc.clone()
        if self.parametrisation == "centred":
            return out
        D = self.numCoefficients
        sig, mu, mask, where = self._scale_and_mean(qc)
        out[:D] = where(mask, (qc[:D] - mu) / sig, qc[:D])
        return out

    def split(self, samples):
        """(numDimensions, ...) -> (w, scales): the (D, ...) coefficients (a view wherever the array allows one) and the
        (J, ...) group scales sigma_j = exp(t_j), on the natural scale for both parametrisations ("noncentred": through
        `to_natural`); NumPy arrays and device tensors alike."""
        D = self.numCoefficients
        if self.parametrisation != "centred":
            samples = self.to_natural(samples)
        t = samples[D:D + self.numGroups]
        return samples[:D], _exp(t)

    @staticmethod
    def random_intercept_design(X, labels, groups=None):
        """([X | onehot(labels)], groups, levels) on the host: one column per distinct label (sorted), all in one new
        group after those of `groups` (default: every column of X fixed)."""
        X = np.asarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise ValueError("X must be 2-D: (M, D)")
        M, D = X.shape
        labels = np.asarray(labels)
        if labels.ndim != 1 or labels.size != M:
            raise ValueError("labels must be 1-D with M = %d entries (shape %s)" % (M, labels.shape))
        levels, idx = np.unique(labels, return_inverse=True)
        base = np.full(D, -1, dtype=np.int64) if groups is None else np.asarray(groups).astype(np.int64)
        if base.ndim != 1 or base.size != D:
            raise ValueError("groups must be 1-D with D = %d entries (shape %s)" % (D, base.shape))
        new = int(base.max()) + 1 if base.size and base.max() >= 0 else 0
        onehot = np.zeros((M, levels.size))
        onehot[np.arange(M), idx] = 1.0
        return np.hstack([X, onehot]), np.r_[base, np.full(levels.size, new, dtype=np.int64)], levels

    @staticmethod
    def random_walk_penalty(n, order=1):
        """D^T D of the order-th difference matrix D ((n - order, n)): the precision structure of a first- or second-order
        random walk over n ordered levels (RW1 / RW2), the difference penalty of a P-spline.  (n, n), banded, rank n - order:
        constants (and for order 2 linear trends) are not penalised."""
        if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)):
            raise ValueError("random_walk_penalty: n must be an integer (got %r)" % (n,))
        if order not in (1, 2) or isinstance(order, (bool, np.bool_)):
            raise ValueError("random_walk_penalty: order must be 1 or 2 (got %r)" % (order,))
        if n <= order:
            raise ValueError("random_walk_penalty: n must be > order (n = %d, order = %d)" % (n, order))
        Dm = np.diff(np.eye(int(n)), n=int(order), axis=0)
        return Dm.T @ Dm

    @staticmethod
    def icar_penalty(adjacency):
        """diag(A 1) - A for a symmetric 0/1 adjacency matrix A with zero diagonal: the intrinsic conditional autoregressive
        (ICAR) structure over the nodes of a graph.  (n, n), rank n - (number of connected components).  Asymmetric
        adjacencies, other entries than 0 and 1, self-loops and isolated nodes raise ValueError."""
        A = np.asarray(adjacency, dtype=np.float64)
        if A.ndim != 2 or A.shape[0] != A.shape[1] or A.shape[0] < 2:
            raise ValueError("icar_penalty: adjacency must be a square (n, n) matrix with n >= 2 (shape %s)" % (A.shape,))
        if not np.all((A == 0.0) | (A == 1.0)):
            raise ValueError("icar_penalty: adjacency must hold 0 and 1 only")
        if not np.array_equal(A, A.T):
            raise ValueError("icar_penalty: adjacency must be symmetric")
        if np.any(np.diag(A) != 0.0):
            raise ValueError("icar_penalty: adjacency must have a zero diagonal")
        deg = A.sum(axis=1)
        if np.any(deg == 0.0):
            raise ValueError("icar_penalty: node %d is isolated (no neighbour): give it a group of its own or drop it"
                             % int(np.flatnonzero(deg == 0.0)[0]))
        return np.diag(deg) - A

    @classmethod
    def with_random_intercepts(cls, X, y, labels, penalty=None, penalty_rank=None, **kw):
        """The model with one random intercept per distinct value of `labels` (M,): a one-hot column per level is
        appended to X and those columns form one new group, after any groups given in `kw` (whose `groups`,
        `prior_precision` and `prior_mean` vectors cover the columns of X; the new columns get mean 0).  Built on the
        host; `pot.levels` keeps the sorted label values, in the order of the appended columns.  `parametrisation` and
        every other keyword of the constructor pass through: few observations per level want "noncentred".  `penalty` (and
        `penalty_rank`) is the matrix Q of the NEW group, (levels, levels) in the order of the sorted label values -- e.g.
        `icar_penalty(adjacency)` over regions, `random_walk_penalty(levels, 1)` over ordered periods (centred only)."""
        Xh, groups, levels = cls.random_intercept_design(X, labels, kw.pop("groups", None))
        D, K = np.asarray(X).shape[1], levels.size
        for name, fill in (("prior_precision", 0.0), ("prior_mean", 0.0)):
            v = kw.get(name)
            if v is not None and np.ndim(v) == 1:
                kw[name] = np.r_[_vector(v, D, name, "D"), np.full(K, fill)]
        if penalty is not None:
            kw["penalty"] = {int(groups[-1]): penalty}
            if penalty_rank is not None:
                kw["penalty_rank"] = {int(groups[-1]): penalty_rank}
        elif penalty_rank is not None:
            raise ValueError("penalty_rank belongs to a penalty: none is given")
        pot = cls(Xh, y, groups=groups, **kw)
        pot.levels = levels
        return pot


def pack_prior_groups_dispersion(groups, log_scale_prior=(0.0, 1.0), prior_precision=1.0, prior_mean=None, dispersion="sample",
                                 log_dispersion_prior=None):
    """The prior table a HierarchicalDispersionGLM handle keeps on the device and its kernel in LDS, computed (and checked) on
    the host by libpbbi.so: (table, n) -- table (2, DP) with DP = padded_dim(D + J + sampled): rows 0 .. D+J-1 as in
    `pack_prior_groups`, and with a sampled dispersion row D + J holds theta's prior (its precision in row 0 of the table,
    its mean in row 1); zeros past the state; n (J,) the members of each group."""
    D = np.asarray(groups).size
    groups, J, tp, lam, mu = _hier_prior(D, groups, log_scale_prior, prior_precision, prior_mean)
    sample, _, _, dprior = _dispersion_args(dispersion, log_dispersion_prior)
    DP = padded_dim(D + J + int(sample))
    dp = np.ascontiguousarray(dprior, dtype=np.float64) if sample else None
    out, n = np.empty(2 * DP, dtype=np.float64), np.empty(J, dtype=np.float64)
    with _host_errors():
        _lib.call("pbbi_glm_pack_prior_groups_dispersion", D, J, _dptr(lam), _dptr(mu), _iptr(groups), _dptr(tp), int(sample),
                  _dptr(dp), _dptr(out), _dptr(n))
    return out.reshape(2, DP), n


class HierarchicalDispersionGLM(HierarchicalGLM):
    """-log posterior of a GLM with a free dispersion (family "gaussian" or "negbinomial", the likelihood of `DispersionGLM`:
    theta = log(dispersion), weights a_i, offsets o_i, eta_i = x_i . w + o_i) in which blocks of coefficients share a sampled
    prior scale (the priors of `HierarchicalGLM`): the linear mixed model with unknown residual sigma, its held-sigma form with
    weights 1 / sigma_i^2, over-dispersed counts with a random intercept per site or batch.

        gaussian     U_i = a_i [ 0.5 exp(-2 theta) (y_i - eta_i)^2 + theta ]
        negbinomial  U_i = a_i [ lgamma(phi) - lgamma(y_i + phi) - phi theta - y_i eta_i + (y_i + phi) logaddexp(eta_i, theta) ]
        centred:     U = sum_i U_i + 0.5 sum_{d: groups_d < 0} lam_d (w_d - mu_d)^2
                       + sum_j [ 0.5 exp(-2 t_j) S_j + n_j t_j + 0.5 lam_tj (t_j - m_tj)^2 ]
                       + 0.5 lam_theta (theta - m_theta)^2                     (the last term only when theta is sampled)
        noncentred:  grouped rows hold z_d, w_d = mu_d + exp(t_j) z_d;  U_nc(z, t, theta) = U_c(w(z, t), t, theta) - sum_j n_j t_j

        pot = HierarchicalDispersionGLM(X, y, family="gaussian", groups=groups, dispersion="sample",
                                        log_dispersion_prior=(0.0, 0.25), log_scale_prior=(0.0, 1.0))
        w, scales, dispersion = pot.split(samples)        # natural scale for both parametrisations
        pot = HierarchicalDispersionGLM.with_random_intercepts(X, y, school, family="gaussian", parametrisation="noncentred")
        # eight schools: y_i ~ N(mu + b_i, sigma_i^2) with sigma_i known
        pot = HierarchicalDispersionGLM.with_random_intercepts(np.ones((8, 1)), y8, np.arange(8), family="gaussian",
                                                               dispersion=1.0, weights=1 / sigma8**2,
                                                               parametrisation="noncentred")

    The chain's state: rows 0 .. D-1 the coefficients (z on the grouped rows of a non-centred potential), rows D .. D+J-1
    t_0 .. t_{J-1}, and with `dispersion="sample"` theta as the LAST row; numDimensions == D + J + (1 if sampled else 0).  With
    `dispersion=` a float > 0 the state is [w; t].  `groups`, `log_scale_prior`, `prior_precision`, `prior_mean` and
    `parametrisation` are `HierarchicalGLM`'s, `dispersion`, `log_dispersion_prior`, `weights` and `offset` `DispersionGLM`'s,
    each with its rules.  `to_natural` / `from_natural` map between the sampler's state and (w; t; theta) -- the theta row passes
    through -- and `split` returns (w, scales, dispersion) on the natural scale for both parametrisations.

    Shapes: float64, 1 <= J <= 4, D + J + sampled <= 64 for both families and both parametrisations (`HIER_DISP_MAX_DIM`; a
    kernel is shipped only if it builds without register spills to memory, and there is none at 65 .. 128 rows).  Not built:
    `penalty=` (structured group priors for these families), more than 4 groups, per-chain trajectory lengths and GIST (they
    raise as for `GLM`).

    Works wherever `GLM` does (HMC in both rng modes, Leapfrog / StormerVerlet, TemperedSMC, TemperingLadder, sampleStats).
    Arguments are checked on the host before anything touches the GPU.  It runs on csrc/kernels_glm.hip (k_glm<NT, FAM, true,
    HIER> with FAM = 3, 4)."""

    def __init__(self, X, y, family="gaussian", groups=None, dispersion="sample", log_dispersion_prior=None,
                 log_scale_prior=(0.0, 1.0), prior_precision=1.0, prior_mean=None, weights=None, offset=None,
                 parametrisation="centred", penalty=None, penalty_rank=None, dtype="float64", device=None):
        if family in FAMILIES:
            raise ValueError("HierarchicalDispersionGLM serves the families %s; family=%r with sampled group scales is "
                             "HierarchicalGLM" % (sorted(HIER_DISP_MAX_DIM), family))
        if penalty is not None or penalty_rank is not None:
            raise ValueError("penalty= (structured group priors) is not built for HierarchicalDispersionGLM: it is served by "
                             "HierarchicalGLM (families logistic and poisson) only")
        _hier_args(parametrisation, groups)
        if family in DISPERSION_FAMILIES and family not in HIER_DISP_MAX_DIM:
            raise ValueError("HierarchicalDispersionGLM serves the families %s: random effects for family=%r are not built "
                             "(DispersionGLM serves it)" % (sorted(HIER_DISP_MAX_DIM), family))
        X, y, a, o = _validate_dispersion(X, y, family, weights, offset)
        M, D = X.shape
        sample, disp, theta, dprior = _dispersion_args(dispersion, log_dispersion_prior)
        groups, J, tp, lam, mu = _hier_prior(D, groups, log_scale_prior, prior_precision, prior_mean)
        Dt = D + J + int(sample)
        dmax = HIER_DISP_MAX_DIM[family][parametrisation]
        if Dt > dmax:
            raise ValueError("HierarchicalDispersionGLM(family=%r, parametrisation=%r) serves a state dimension (coefficients + "
                             "groups%s) <= %d (got %d): a kernel is shipped only if it builds without register spills to memory"
                             % (family, parametrisation, " + 1 for the sampled dispersion" if sample else "", dmax, Dt))
        _float64_only(dtype)
        self._set_hier_state(Dt, dtype, device, parametrisation, X, y, family, a, o, None, lam, mu, groups, tp)
        self.sampled = sample
        self.dispersion = "sample" if sample else disp
        self.log_dispersion_prior = dprior
        dp = np.ascontiguousarray(dprior, dtype=np.float64) if sample else None
        _lib.call("pbbi_potential_create_glm_hier_dispersion", D, M, _dptr(X), _dptr(y), DISPERSION_FAMILIES[family], _dptr(a),
                  _dptr(o), _dptr(lam), _dptr(mu), _iptr(groups), J, _dptr(tp),
                  HIER_PARAMETRISATIONS[parametrisation], int(sample), theta, _dptr(dp), self._dt, self.device,
                  C.byref(self._handle))

    def split(self, samples):
        """(numDimensions, ...) -> (w, scales, dispersion): the (D, ...) coefficients and the (J, ...) group scales sigma_j =
        exp(t_j) as `HierarchicalGLM.split` returns them (natural scale for both parametrisations), and exp(theta) -- sigma for
        "gaussian", phi for "negbinomial" -- of shape (...); held: the constant itself."""
        w, scales = super().split(samples)
        if not self.sampled:
            return w, scales, self.dispersion
        theta = samples[self.numCoefficients + self.numGroups]
        return w, scales, _exp(theta)
