"""Generalised linear models as potentials whose likelihood runs on the fp64 matrix cores.

    U(w) = sum_i [ b(x_i . w) - y_i (x_i . w) ] + 0.5 prior_precision |w|^2

over the M rows x_i of the design matrix X: -log posterior of the weights of a GLM with canonical link
and a N(0, I / prior_precision) prior.  `family="logistic"`: b = softplus, y in {0, 1} (the model of
custom.logistic_regression_posterior); `family="poisson"`: b = exp, y counts.

For an ensemble the model is two matrix products shared by all chains (eta = X W, g = X^T (b'(eta) - y)
+ prior_precision W with W the (D, N) state), which csrc/kernels_glm.hip runs on the MFMA units with X
staged through LDS -- the data set is read once per 64 chains, not once per chain.  float64, D <= 128.
"""
import ctypes as C

import numpy as np

from . import _lib
from .potential import Potential, _dptr

__all__ = ["GLM", "FAMILIES", "pack_design", "padded_dim"]

FAMILIES = {"logistic": _lib.GLM_LOGISTIC, "poisson": _lib.GLM_POISSON}
MAX_DIM = 128


def padded_dim(D):
    """Rows of the chain state the kernels work on: D padded to 16, 32, 64 or 128."""
    D = int(D)
    if not 1 <= D <= MAX_DIM:
        raise ValueError(f"GLM potentials serve 1 <= D <= {MAX_DIM} (D = {D})")
    return 16 if D <= 16 else 32 if D <= 32 else 64 if D <= 64 else 128


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
    n = C.c_int64()
    _lib.call("pbbi_glm_pack_design", D, M, None, None, 0, C.byref(n))
    out = np.empty(n.value, dtype=np.float64)
    _lib.call("pbbi_glm_pack_design", D, M, _dptr(X), _dptr(out), out.size, C.byref(n))
    return out.reshape(-1, 2, DP * 16)


def _validate(X, y, family, prior_precision, dtype):
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("X must be 2-D: (M, D)")
    M, D = X.shape
    if M < 1 or D < 1:
        raise ValueError("X must have at least one row and one column")
    y = np.asarray(y, dtype=np.float64)
    if y.ndim != 1 or y.size != M:
        raise ValueError("X has %d rows, y must be 1-D with as many entries (shape %s)" % (M, y.shape))
    if family not in FAMILIES:
        raise ValueError("family must be one of %s (got %r)" % (sorted(FAMILIES), family))
    if not np.all(np.isfinite(X)) or not np.all(np.isfinite(y)):
        raise ValueError("X and y must be finite")
    if family == "logistic" and not np.all((y == 0) | (y == 1)):
        raise ValueError("logistic: y must be 0 or 1")
    if family == "poisson" and not (np.all(y >= 0) and np.all(y == np.floor(y))):
        raise ValueError("poisson: y must hold non-negative integers")
    lam = float(prior_precision)
    if not (np.isfinite(lam) and lam >= 0):
        raise ValueError("prior_precision must be a finite scalar >= 0")
    if D > MAX_DIM:
        raise ValueError(f"GLM potentials serve D <= {MAX_DIM} (D = {D})")
    if np.dtype(dtype) != np.dtype("float64"):
        raise ValueError("GLM potentials are float64 only")
    return np.ascontiguousarray(X), np.ascontiguousarray(y), lam


class GLM(Potential):
    """-log posterior of the weights of a generalised linear model (see the module text).

        pot = GLM(X, y, family="logistic", prior_precision=1.0)
        HMC(Ensemble(D, N), 1.0, 0.1, None, potential=pot, rng="philox").getSamples(...)

    Works wherever a Potential does (HMC in both rng modes, Leapfrog / StormerVerlet, TemperedSMC,
    TemperingLadder).  Arguments are checked on the host before anything touches the GPU."""

    kind = "glm"

    def __init__(self, X, y, family="logistic", prior_precision=1.0, dtype="float64", device=None):
        X, y, lam = _validate(X, y, family, prior_precision, dtype)
        super().__init__(X.shape[1], dtype, device)
        self.X, self.y, self.family, self.prior_precision = X, y, family, lam
        _lib.call("pbbi_potential_create_glm", X.shape[1], X.shape[0], _dptr(X), _dptr(y),
                  FAMILIES[family], lam, self._dt, self.device, C.byref(self._handle))
