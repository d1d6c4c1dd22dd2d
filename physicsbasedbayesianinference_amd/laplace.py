"""Posterior mode and Laplace approximation of a GLM potential: `GLM.laplace` and `DispersionGLM.laplace`.

    fit = pot.laplace()                       # damped Newton to the mode; fit.mode, fit.stderr, fit.log_evidence
    hmc.setMassMatrix(fit.metric)             # a metric from the curvature before the first draw
    hmc.setMassMatrix(fit.dense_metric)       # ... or the dense one: correlated rows as well as badly scaled ones
    hmc.getSamples(S, T, 0.0, rng="philox", start=fit.sample(N, spread=1.5))   # chains over-dispersed around the mode

The hot path is the Hessian X^T Lambda(eta) X of the potential at one state, on the fp64 matrix cores over the design image the
handle already keeps (pbbi_glm_hessian, csrc/kernels_glm_hessian.hip).  The Newton loop is host plumbing: per iteration one
Hessian launch, one pbbi_potential_eval of one chain (U and the gradient) and one small copy to the host, where the n x n
Cholesky factor is taken (n <= 128); the line search evaluates its 16 trial steps as 16 chains of one more evaluation.
"""
import numpy as np

from . import _lib

__all__ = ["LaplaceResult", "laplace"]

_LOG_2PI = float(np.log(2.0 * np.pi))
ARMIJO = 1e-4       # sufficient decrease: U(w + t d) <= U(w) + ARMIJO t g.d
HALVINGS = 16       # trial steps t = 2^-j, j = 0 .. 15, one chain each
RIDGE0, RIDGE_UP, RIDGE_TRIES = 1e-6, 10.0, 24


class LaplaceResult:
    """What `laplace` returns.  `mode` (n,) in the sampler's coordinates (coefficients, then a sampled log-dispersion);
    `hessian` (n, n) of the potential there; `U` the potential there; `converged`, `iterations` (Newton steps taken) and
    `decrement` (the last Newton decrement, -g.d / 2).  Derived, all on the host in float64:

        covariance    hessian^-1
        stderr        sqrt(diag(covariance))
        metric        1 / diag(covariance): what HMC.setMassMatrix takes
        dense_metric  (hessian + hessian^T) / 2: the dense metric HMC.setMassMatrix takes (GLM, DispersionGLM up to 64 rows)
        log_evidence  the Laplace log p(y)
        sample(N)     N draws of N(mode, spread^2 covariance) as a device tensor

    Built by hand -- LaplaceResult(mode, hessian, U, prior_precision=..., prior_names=..., constant=...) -- it serves the same
    algebra; `sample` needs `device`."""

    def __init__(self, mode, hessian, U, converged=True, iterations=0, decrement=0.0, prior_precision=None, prior_names=None,
                 constant=0.0, power=1.0, device=None):
        self.mode = np.array(mode, dtype=np.float64).ravel()
        n = self.mode.size
        self.hessian = np.array(hessian, dtype=np.float64).reshape(n, n)
        self.U = float(U)
        self.converged, self.iterations, self.decrement = bool(converged), int(iterations), float(decrement)
        self.prior_precision = None if prior_precision is None else np.array(prior_precision, dtype=np.float64).ravel()
        self.prior_names = list(prior_names) if prior_names is not None else ["row %d" % d for d in range(n)]
        self.constant, self.power, self.device = float(constant), float(power), device
        self._chol = None

    def _factor(self):
        """L with hessian = L L^T; ValueError where the Hessian is not positive definite (no mode was found)."""
        if self._chol is None:
            try:
                self._chol = np.linalg.cholesky(self.hessian)
            except np.linalg.LinAlgError:
                raise ValueError("the Hessian is not positive definite: no Laplace approximation at this point "
                                 "(converged = %r)" % self.converged) from None
        return self._chol

    @property
    def covariance(self):
        L = self._factor()
        Li = np.linalg.solve(L, np.eye(L.shape[0]))
        C = Li.T @ Li
        return 0.5 * (C + C.T)

    @property
    def stderr(self):
        return np.sqrt(np.diag(self.covariance))

    @property
    def metric(self):
        return 1.0 / np.diag(self.covariance)

    @property
    def dense_metric(self):
        """The Hessian, symmetrised: the posterior precision of the approximation, what HMC.setMassMatrix takes as a DENSE
        metric -- it removes the correlation between rows as well as their scales (`metric` removes the scales alone)."""
        return 0.5 * (self.hessian + self.hessian.T)

    @property
    def log_evidence(self):
        """log p(y) ~ -U(mode) + sum_i k_i + 1/2 sum_rows log(lam_row / 2 pi) + n/2 log 2 pi - 1/2 log det H: the joint density
        at the mode -- the constants k_i the kernels drop (glm.pointwise_constants) and the normalisers of the rows' Gaussian
        priors put back -- times the Gaussian integral around it.  This is the convention of
        smc.LikelihoodTemperedSMC.logML: the evidence of the model with its PROPER prior, constants included, so the two
        numbers can be held side by side.  ValueError naming the row where a prior precision is 0 (an improper prior has no
        evidence), and where the potential carried a likelihood power other than 1 when it was evaluated."""
        if self.prior_precision is None:
            raise ValueError("log_evidence: the result carries no prior (prior_precision=)")
        if self.power != 1.0:
            raise ValueError("log_evidence: the potential was evaluated at likelihood power %r, not 1" % (self.power,))
        for d, name in enumerate(self.prior_names):
            if self.prior_precision[d] == 0.0:
                raise ValueError("log_evidence: the prior of row %d is improper (%s = 0)" % (d, name))
        n = self.mode.size
        logdet = 2.0 * float(np.sum(np.log(np.diag(self._factor()))))
        return (-self.U + self.constant + 0.5 * float(np.sum(np.log(self.prior_precision / (2.0 * np.pi))))
                + 0.5 * n * _LOG_2PI - 0.5 * logdet)

    def sample(self, N, seed=0, spread=1.0):
        """(n, N) float64 device tensor q = mode + spread L^-T z with hessian = L L^T: draws of N(mode, spread^2 covariance),
        e.g. over-dispersed starting states for HMC's start=.  z are standard normals from the device Philox stream
        (pbbi_philox_normal, PBBI_STREAM_POSITION with the double-precision draw, iteration 0, chain index n -- as
        `sample_prior` draws), transformed with torch ops on the device."""
        from . import _device
        t = _device.torch()
        N = int(N)
        if N < 1:
            raise ValueError("sample: N must be >= 1")
        if self.device is None:
            raise ValueError("sample: the result carries no device (device=)")
        n, dev = self.mode.size, self.device
        L = self._factor()
        z = _device.empty((n, N), np.float64, dev)
        _lib.call("pbbi_philox_normal", int(seed), _lib.STREAM_POSITION | _lib.STREAM_DRAW_F64, 0, 0, n, N, N, 1.0, None,
                  _lib.F64, dev, z.data_ptr(), _device.stream_ptr(dev))
        Lt = _device.as_device(np.ascontiguousarray(L.T), dev, np.float64)
        mode = _device.as_device(self.mode, dev, np.float64)
        # (the solver returns a column-major result: made row-major, the layout every entry that takes a (D, N) state reads)
        return (mode[:, None] + float(spread) * t.linalg.solve_triangular(Lt, z, upper=True)).contiguous()

    def __repr__(self):
        return "LaplaceResult(n=%d, U=%.6g, converged=%r, iterations=%d, decrement=%.3g)" % (
            self.mode.size, self.U, self.converged, self.iterations, self.decrement)


def _hessian_into(pot, q_dev, out_dev, ranges):
    from . import _device
    from .glm import _device_errors
    with _device_errors():
        _lib.call("pbbi_glm_hessian", pot.handle, q_dev.data_ptr(), int(ranges), out_dev.data_ptr(), _device.stream_ptr(pot.device))


def hessian(pot, q, ranges=0):
    """The (n, n) Hessian of the potential at the state q (n,), from the device (pbbi_glm_hessian), as a NumPy array."""
    from . import _device
    n = pot.numDimensions
    q = np.ascontiguousarray(q, dtype=np.float64).ravel()
    if q.size != n:
        raise ValueError("q must hold the %d rows of the state" % n)
    out = _device.empty((n, n), np.float64, pot.device)
    _hessian_into(pot, _device.as_device(q, pot.device, np.float64), out, ranges)
    return _device.to_numpy(out)


def laplace(self, start=None, max_iter=50, tol=1e-12, ranges=0):
    """The posterior mode by a damped Newton iteration and the Laplace approximation around it: a `LaplaceResult`.

    Per iteration the device forms the Hessian H (pbbi_glm_hessian: X^T Lambda X on the matrix cores) and U with its gradient
    g (pbbi_potential_eval of one chain); one small copy brings the three to the host.  There H is factored (Cholesky), the
    step is d = -H^-1 g and the Newton decrement -g.d / 2.  The iteration stops with converged=True when the decrement is
    <= `tol`, without taking that step.  Otherwise the 16 trial points w + 2^-j d, j = 0 .. 15, are evaluated as 16 chains of
    one more pbbi_potential_eval and the largest step with U(w + t d) <= U(w) + 1e-4 t g.d is taken.  If H has no Cholesky
    factor or no trial step passes, rho I is added to H -- rho from 1e-6 max diag(H), times 10 on each failure, back to 0
    after a step (the families with a sampled log-dispersion are not jointly convex).  `max_iter` steps taken, a non-finite U,
    or a ridge that never helps end the iteration with converged=False; nothing is raised.

    On linearly separable logistic data with a flat prior there is no mode: the steps walk out along a ray, U and the
    decrement fall like exp(-k), and a decrement <= 1e-12 is eventually met (after some 30 steps) far from the origin; such
    a fit shows in `stderr`.  A proper prior (prior_precision > 0) has a mode.

    `start`: (n,) in the sampler's coordinates, finite; default zeros.  `ranges` as for pbbi_glm_hessian (0: the library
    chooses; a fixed value makes every bit reproducible).  The potential is evaluated as it is: with a likelihood power set
    the result is the tempered mode, and its `log_evidence` raises."""
    from . import _device
    from .glm import _prior_layout, pointwise_constants
    n, dev = self.numDimensions, self.device
    if start is None:
        w = np.zeros(n)
    else:
        w = np.array(start, dtype=np.float64).ravel()
        if w.size != n:
            raise ValueError("start must hold the %d rows of the state, got %d" % (n, w.size))
        if not np.all(np.isfinite(w)):
            raise ValueError("start must be finite")
    max_iter = int(max_iter)
    stream = _device.stream_ptr(dev)
    buf = _device.empty((n * n + n + 1,), np.float64, dev)      # H | g | U: one copy per iteration
    Hd, gd, Ud = buf[:n * n], buf[n * n:n * n + n], buf[n * n + n:]
    Uj_d = _device.empty((HALVINGS,), np.float64, dev)
    steps = 0.5 ** np.arange(HALVINGS)

    H, U, dec = np.full((n, n), np.nan), float("nan"), float("nan")
    converged, it = False, 0
    while True:
        qd = _device.as_device(w, dev, np.float64)
        _hessian_into(self, qd, Hd, ranges)
        _lib.call("pbbi_potential_eval", self.handle, qd.data_ptr(), 1, 1, Ud.data_ptr(), gd.data_ptr(), stream)
        host = _device.to_numpy(buf)
        H, g, U = host[:n * n].reshape(n, n).copy(), host[n * n:n * n + n].copy(), float(host[-1])
        if not (np.isfinite(U) and np.all(np.isfinite(g)) and np.all(np.isfinite(H))):
            break
        rho, moved = 0.0, False
        for _ in range(RIDGE_TRIES):
            try:
                L = np.linalg.cholesky(H + rho * np.eye(n) if rho else H)
            except np.linalg.LinAlgError:
                L = None
            if L is not None:
                d = -np.linalg.solve(L.T, np.linalg.solve(L, g))
                gd_dot = float(g @ d)
                dec = -0.5 * gd_dot
                if dec <= tol:
                    converged = rho == 0.0      # with a ridge the point is stationary but H is not positive definite
                    break
                if it >= max_iter:
                    break
                Q = w[:, None] + d[:, None] * steps[None, :]
                Qd = _device.as_device(Q, dev, np.float64)
                _lib.call("pbbi_potential_eval", self.handle, Qd.data_ptr(), HALVINGS, HALVINGS, Uj_d.data_ptr(), None, stream)
                Uj = _device.to_numpy(Uj_d)
                ok = np.isfinite(Uj) & (Uj <= U + ARMIJO * steps * gd_dot)
                if ok.any():
                    w = Q[:, int(np.argmax(ok))].copy()
                    it += 1
                    moved = True
                    break
            scale = float(np.max(np.abs(np.diag(H)))) or 1.0
            rho = RIDGE0 * scale if rho == 0.0 else RIDGE_UP * rho
        if not moved:
            break

    _, prec, names, _, _, _ = _prior_layout(self)
    # the handle that was evaluated is this potential's own: a plain GLM's stays at power 1 whatever its twin carries
    power = self.likelihood_power if self._power_target(build=False) is self else 1.0
    k = float(np.sum(pointwise_constants(self.family, self.y, self.weights, self.trials)))
    return LaplaceResult(w, H, U, converged, it, dec, prior_precision=prec, prior_names=names, constant=k, power=power,
                         device=dev)
