"""Tempered sequential Monte Carlo: the ensemble as ONE population, with the model evidence.

The reference plans "further development of SMC" (references/PhysicsBasedHMC_SoHPC2022_WeekPlan.md:39) and keeps
ensemble weights exp(-beta H) it never uses (src/ensemble.py:52-61, src/HMC.py:86-104).  Here N particles move
along the path pi_beta ~ exp(-beta U(q)) from a reference N(qMean, qStd^2 I) (stage 0) to beta = 1:

  per stage:  U = eval(q);  choose beta' (pbbi_smc_next_beta: the ESS of the incremental weights = target_ess);
              reweight and accumulate log Z (pbbi_smc_reweight);  resample when the ESS of the accumulated weights
              is below resample_threshold (pbbi_smc_resample_systematic, decided on the device);
              `moves` HMC iterations at kT = 1 / beta' (pbbi_hmc_run, PBBI_BETA_ACCEPT).

Stage 1 is importance sampling from the reference: qStd must make the reference WIDER than exp(-beta_1 U).  The step
size stays the same at every stage: in the kT form leapfrog stability is h sqrt(lambda_max) < 2 whatever kT is, and
the sqrt(kT) of the momentum already widens the moves with the distribution.
"""
import numpy as np

from . import _lib
from ._device import as_device, empty, stream_ptr, synchronize, to_numpy
from .integrator import resolve_potential

__all__ = ["TemperedSMC", "LikelihoodTemperedSMC"]

_METHODS = {"leapfrog": _lib.LEAPFROG, "stormer_verlet": _lib.STORMER_VERLET, "stormerverlet": _lib.STORMER_VERLET}


class TemperedSMC:
    """N particles tempered from a Gaussian reference to exp(-U).

        smc = TemperedSMC(potential, D, N, simulTime=1.0, stepSize=0.1, qStd=3.0)
        q = smc.run()                 # (D, N) equally weighted particles at beta = 1
        smc.logZ                      # log of the integral of exp(-U(q)) dq

    `betas` (increasing, ending at 1) fixes the schedule and skips the search; without it every stage reads back
    one double (the next beta, the kT of its moves).  After run(): `logZ`, `betas` (the stages' betas),
    `ess` (ESS / N of the accumulated weights after each reweighting), `acceptRates` (per stage), `resampled`
    (per stage, bool), `warnings` (list of str), `host_syncs` (device-to-host reads during the stage loop),
    `ancestors` (per stage, device int32 arrays, with record_ancestors=True), `state` (the final device state)."""

    def __init__(self, potential, numDimensions, numParticles, simulTime, stepSize, qStd, qMean=None, moves=5,
                 target_ess=0.5, resample_threshold=0.5, betas=None, method="leapfrog", seed=0, kdk_fma=True,
                 draw_f64=False, record_ancestors=False, max_stages=1000):
        self.D, self.N = int(numDimensions), int(numParticles)
        if self.D < 1 or self.N < 1:
            raise ValueError("numDimensions and numParticles must be >= 1")
        if not (0.0 < float(target_ess) < 1.0):
            raise ValueError("target_ess must lie in (0, 1)")
        if not (0.0 <= float(resample_threshold) <= 1.0):
            raise ValueError("resample_threshold must lie in [0, 1]")
        if not (float(qStd) > 0.0):
            raise ValueError("qStd must be > 0")
        if int(moves) < 1:
            raise ValueError("moves must be >= 1")
        if not (float(stepSize) > 0.0 and float(simulTime) > 0.0):
            raise ValueError("stepSize and simulTime must be > 0")
        if str(method).lower() not in _METHODS:
            raise ValueError(f"method must be one of {sorted(_METHODS)}")
        if betas is not None:
            b = np.asarray(betas, dtype=np.float64)
            if b.ndim != 1 or b.size < 1 or not np.all(np.isfinite(b)) or b[0] <= 0.0 or np.any(np.diff(b) <= 0.0) \
                    or b[-1] != 1.0:
                raise ValueError("betas must increase strictly from a value > 0 to exactly 1")
            betas = b
        self.qMean = None if qMean is None else np.ascontiguousarray(qMean, dtype=np.float64).ravel()
        if self.qMean is not None and self.qMean.size != self.D:
            raise ValueError("qMean must have numDimensions entries")
        self.fixed_betas = betas
        self.simulTime, self.stepSize, self.qStd = float(simulTime), float(stepSize), float(qStd)
        self.numSteps = max(1, int(self.simulTime / self.stepSize))     # src/integrator.py:51
        self.moves, self.target_ess = int(moves), float(target_ess)
        self.resample_threshold, self.seed = float(resample_threshold), int(seed)
        self.method = _METHODS[str(method).lower()]
        self.draw_f64 = bool(draw_f64)
        self.flags = _lib.BETA_ACCEPT | (_lib.KDK_FMA if kdk_fma else 0) | (_lib.DRAW_F64 if draw_f64 else 0)
        self.record_ancestors = bool(record_ancestors)
        self.max_stages = int(max_stages) if betas is None else int(betas.size)
        self.pot = resolve_potential(potential, "potential", self.D)
        if self.pot.numDimensions != self.D:
            raise ValueError(f"potential has D={self.pot.numDimensions}, sampler has D={self.D}")
        self.logZ = self.betas = self.ess = self.acceptRates = self.resampled = self.state = None
        self.warnings, self.ancestors, self.host_syncs = [], [], 0

    def run(self, device_output=False):
        import torch
        pot, D, N, dev, dt = self.pot, self.D, self.N, self.pot.device, self.pot.dtype
        st = stream_ptr(dev)
        if self.max_stages + self.moves * self.max_stages > 2 ** 32:
            raise ValueError("too many stages for the 32-bit Philox iteration counter")
        q = empty((D, N), dt, dev)
        q_alt = empty((D, N), dt, dev)
        pos_stream = _lib.STREAM_POSITION | (_lib.STREAM_DRAW_F64 if self.draw_f64 else 0)
        _lib.call("pbbi_philox_normal", self.seed, pos_stream, 0, 0, D, N, N, self.qStd, None, pot._dt, dev,
                  q.data_ptr(), st)
        mean = None
        if self.qMean is not None:
            mean = as_device(self.qMean, dev, np.float64)
            q += mean.to(q.dtype)[:, None]
        mean_ptr = mean.data_ptr() if mean is not None else None
        S = self.max_stages
        betas = torch.zeros(S + 1, dtype=torch.float64, device=q.device)
        if self.fixed_betas is not None:
            betas[1:] = torch.from_numpy(self.fixed_betas).to(q.device)
        info = torch.zeros((S, 2), dtype=torch.float64, device=q.device)       # warning flag, bracket width
        rec = torch.zeros((S, 2), dtype=torch.float64, device=q.device)        # log Z increment, ESS / N
        logz = torch.zeros(1, dtype=torch.float64, device=q.device)
        logw = torch.zeros(N, dtype=torch.float64, device=q.device)
        resampled = torch.zeros(S + 1, dtype=torch.uint8, device=q.device)
        status = torch.zeros(S + 1, dtype=torch.int32, device=q.device)
        n_rej = torch.zeros(S, dtype=torch.float64, device=q.device)
        U = empty((N,), dt, dev)
        reject = empty((self.moves, N), np.uint8, dev)
        anc = empty((N,), np.int32, dev)
        self.ancestors, self.warnings, self.host_syncs = [], [], 0
        t, q = self._stages(st, q, q_alt, mean_ptr, betas, info, rec, logz, logw, resampled, status, n_rej, U, reject,
                            anc)
        synchronize(dev)
        self._raise_on_status(status, t + 1)
        self.nstages = t
        self.betas = to_numpy(betas[1:t + 1]).copy()
        self.logZ = float(to_numpy(logz)[0])
        r = to_numpy(rec[:t])
        self.logZ_increments, self.ess = r[:, 0].copy(), r[:, 1].copy()
        self.resampled = to_numpy(resampled[:t + 1]).astype(bool)
        self.acceptRates = 1.0 - to_numpy(n_rej[:t]) / (self.moves * N)
        if self.fixed_betas is None and to_numpy(info[0, 0]) != 0.0:
            self.warnings.append("stage 1: even the best beta of the log grid leaves the ESS below target_ess "
                                 "(the reference is too narrow or too far from the target: widen qStd)")
        self.state = q
        return q if device_output else to_numpy(q)

    def _stages(self, st, q, q_alt, mean_ptr, betas, info, rec, logz, logw, resampled, status, n_rej, U, reject, anc):
        """The stage loop and the closing resample: launches only, plus -- adaptive schedule -- the one read of the
        next beta per stage.  Returns (stages, final state)."""
        pot, D, N, dev, S = self.pot, self.D, self.N, self.pot.device, self.max_stages
        b8 = 8
        t, beta = 0, 0.0
        while True:
            if t >= S:
                raise RuntimeError(f"TemperedSMC: beta did not reach 1 within max_stages={S} stages")
            qarg = q.data_ptr() if t == 0 else None
            _lib.call("pbbi_potential_eval", pot.handle, q.data_ptr(), N, N, U.data_ptr(), None, st)
            bptr = betas.data_ptr() + t * b8
            if self.fixed_betas is None:
                _lib.call("pbbi_smc_next_beta", U.data_ptr(), logw.data_ptr(), qarg, mean_ptr, self.qStd, N, N, D,
                          self.target_ess, bptr, info.data_ptr() + t * 2 * b8, pot._dt, dev, st)
            _lib.call("pbbi_smc_reweight", U.data_ptr(), qarg, mean_ptr, self.qStd, N, N, D, bptr, logw.data_ptr(),
                      logz.data_ptr(), rec.data_ptr() + t * 2 * b8, pot._dt, dev, st)
            a_out = empty((N,), np.int32, dev) if self.record_ancestors else anc
            _lib.call("pbbi_smc_resample_systematic", logw.data_ptr(), N, self.seed, t, q.data_ptr(), q_alt.data_ptr(),
                      N, D, rec.data_ptr() + (t * 2 + 1) * b8, self.resample_threshold, a_out.data_ptr(), None,
                      resampled.data_ptr() + t, status.data_ptr() + 4 * t, pot._dt, dev, st)
            if self.record_ancestors:
                self.ancestors.append(a_out)
            q, q_alt = q_alt, q
            if self.fixed_betas is None:
                prev, beta = beta, float(betas[t + 1].item())        # the one device -> host read of the stage
                self.host_syncs += 1
                if not beta > prev:
                    self._raise_on_status(status, t + 1)
                    raise RuntimeError(f"TemperedSMC: stage {t + 1} could not raise beta above {prev!r} (the ESS of "
                                       "every step is below target_ess: particles of extreme U, e.g. diverged moves)")
            else:
                beta = float(self.fixed_betas[t])
            _lib.call("pbbi_hmc_run", pot.handle, self.method, q.data_ptr(), None, None, None, reject.data_ptr(), None,
                      N, N, self.stepSize, self.numSteps, self.moves, self.flags, self.seed, t * self.moves, 0,
                      1.0 / beta, st)
            n_rej[t] += reject.sum()
            t += 1
            if beta == 1.0:
                break
        # the final weights (a stage without a resample leaves them unequal): one more resample at stage index t,
        # the identity when they are equal already
        a_out = empty((N,), np.int32, dev) if self.record_ancestors else anc
        _lib.call("pbbi_smc_resample_systematic", logw.data_ptr(), N, self.seed, t, q.data_ptr(), q_alt.data_ptr(), N,
                  D, None, 1.0, a_out.data_ptr(), None, resampled.data_ptr() + t, status.data_ptr() + 4 * t, pot._dt,
                  dev, st)
        if self.record_ancestors:
            self.ancestors.append(a_out)
        return t, q_alt

    @staticmethod
    def _raise_on_status(status, upto):
        st_h = to_numpy(status[:upto])
        if np.any(st_h != _lib.OK):
            raise _lib.PbbiError(int(st_h[st_h != _lib.OK][0]),
                                 f"every resampling weight was zero at stage {int(np.argmax(st_h != _lib.OK))}")


class LikelihoodTemperedSMC:
    """N particles tempered from the PRIOR of a GLM potential to its posterior along pi_beta(w) ~ p(w) L(w)^beta: the log
    marginal likelihood of the model.

        smc = LikelihoodTemperedSMC(pot, 4096, simulTime=1.0, stepSize=0.05)
        q = smc.run()                 # (numDimensions, N) equally weighted posterior particles, sampler coordinates
        smc.logML                     # log p(y): compare two models by the difference

    Stage 0 is an exact draw from the prior (`pot.sample_prior`, which must be proper); the incremental weight of a stage is
    dbeta * loglik (`pbbi_loglik_glm` on the particles, natural coordinates) through the population kernels of `TemperedSMC`
    with no reference term; the moves are HMC at kT = 1 on the potential with its likelihood power set to the stage's beta
    from the device (`pbbi_potential_set_likelihood_power`), restored to 1 when run() leaves.  The power lives on the handle:
    do not run another sampler on the same potential meanwhile.  A plain `GLM` is tempered on its full-model twin.

    `betas` (increasing, from a value > 0 to exactly 1) fixes the schedule: no host read inside the loop; without it every
    stage reads back one double.  After run(): `logML` (= `logZ` + the likelihood's constants sum_i k_i), `logZ`, `betas`,
    `ess`, `acceptRates`, `resampled`, `ancestors` (record_ancestors=True), `host_syncs`, `state`."""

    def __init__(self, potential, numParticles, simulTime, stepSize, moves=5, target_ess=0.5, resample_threshold=0.5,
                 betas=None, method="leapfrog", seed=0, record_ancestors=False, max_stages=1000, kdk_fma=True,
                 draw_f64=True):
        from . import glm
        if isinstance(potential, glm.SoftmaxGLM) or not isinstance(potential, glm._Tempered):
            raise ValueError("LikelihoodTemperedSMC serves GLM, DispersionGLM, HierarchicalGLM and HierarchicalDispersionGLM "
                             "potentials (got %s)" % type(potential).__name__)
        self.N = int(numParticles)
        if self.N < 1:
            raise ValueError("numParticles must be >= 1")
        if not (0.0 < float(target_ess) < 1.0):
            raise ValueError("target_ess must lie in (0, 1)")
        if not (0.0 <= float(resample_threshold) <= 1.0):
            raise ValueError("resample_threshold must lie in [0, 1]")
        if int(moves) < 1:
            raise ValueError("moves must be >= 1")
        if not (float(stepSize) > 0.0 and float(simulTime) > 0.0):
            raise ValueError("stepSize and simulTime must be > 0")
        if str(method).lower() not in _METHODS:
            raise ValueError(f"method must be one of {sorted(_METHODS)}")
        if betas is not None:
            b = np.asarray(betas, dtype=np.float64)
            if b.ndim != 1 or b.size < 1 or not np.all(np.isfinite(b)) or b[0] <= 0.0 or np.any(np.diff(b) <= 0.0) \
                    or b[-1] != 1.0:
                raise ValueError("betas must increase strictly from a value > 0 to exactly 1")
            betas = b
        elif int(max_stages) < 1:
            raise ValueError("max_stages must be >= 1")
        self.pot, self.D = potential, potential.numDimensions
        self.fixed_betas = betas
        self.simulTime, self.stepSize = float(simulTime), float(stepSize)
        self.numSteps = max(1, int(self.simulTime / self.stepSize))
        self.moves, self.target_ess = int(moves), float(target_ess)
        self.resample_threshold, self.seed = float(resample_threshold), int(seed)
        self.method = _METHODS[str(method).lower()]
        self.draw_f64 = bool(draw_f64)
        self.flags = (_lib.KDK_FMA if kdk_fma else 0) | (_lib.DRAW_F64 if draw_f64 else 0)
        self.record_ancestors = bool(record_ancestors)
        self.max_stages = int(max_stages) if betas is None else int(betas.size)
        self.logML = self.logZ = self.betas = self.ess = self.acceptRates = self.resampled = self.state = None
        self.ancestors, self.host_syncs = [], 0

    def run(self, device_output=False):
        import torch
        from .glm import pointwise_constants
        pot, D, N, dev = self.pot, self.D, self.N, self.pot.device
        st = stream_ptr(dev)
        S = self.max_stages
        if self.moves * S > 2 ** 32:      # stage t draws iterations t * moves .. (t + 1) * moves - 1; the resampler's stage <= S
            raise ValueError("too many stages for the 32-bit Philox iteration counter")
        q = pot.sample_prior(N, seed=self.seed, draw_f64=self.draw_f64)      # raises on an improper prior
        q_alt = empty((D, N), np.float64, dev)
        target = pot._power_target()                                           # (a plain GLM: its full-model twin)
        betas = torch.zeros(S + 1, dtype=torch.float64, device=q.device)       # betas[0] = 0: the prior
        if self.fixed_betas is not None:
            betas[1:] = torch.from_numpy(self.fixed_betas).to(q.device)
        info = torch.zeros((S, 2), dtype=torch.float64, device=q.device)
        rec = torch.zeros((S, 2), dtype=torch.float64, device=q.device)        # log Z increment, ESS / N
        logz = torch.zeros(1, dtype=torch.float64, device=q.device)
        logw = torch.zeros(N, dtype=torch.float64, device=q.device)
        resampled = torch.zeros(S + 1, dtype=torch.uint8, device=q.device)
        status = torch.zeros(S + 1, dtype=torch.int32, device=q.device)
        n_rej = torch.zeros(S, dtype=torch.float64, device=q.device)
        U = empty((N,), np.float64, dev)
        reject = empty((self.moves, N), np.uint8, dev)
        anc = empty((N,), np.int32, dev)
        self.ancestors, self.host_syncs = [], 0
        try:
            t, q = self._stages(st, q, q_alt, target, betas, info, rec, logz, logw, resampled, status, n_rej, U, reject, anc)
        finally:
            _lib.call("pbbi_potential_set_likelihood_power", target.handle, 1.0, None, st)
        synchronize(dev)
        TemperedSMC._raise_on_status(status, t + 1)
        self.nstages = t
        self.betas = to_numpy(betas[1:t + 1]).copy()
        self.logZ = float(to_numpy(logz)[0])
        k = pointwise_constants(pot.family, pot.y, pot.weights, pot.trials)
        self.logML = self.logZ + float(np.sum(k))
        r = to_numpy(rec[:t])
        self.logZ_increments, self.ess = r[:, 0].copy(), r[:, 1].copy()
        self.resampled = to_numpy(resampled[:t + 1]).astype(bool)
        self.acceptRates = 1.0 - to_numpy(n_rej[:t]) / (self.moves * N)
        self.state = q
        return q if device_output else to_numpy(q)

    def _stages(self, st, q, q_alt, target, betas, info, rec, logz, logw, resampled, status, n_rej, U, reject, anc):
        """The stage loop and the closing resample: launches only, plus -- adaptive schedule -- the one read of the next
        beta per stage.  Returns (stages, final state)."""
        pot, D, N, dev, S = self.pot, self.D, self.N, self.pot.device, self.max_stages
        noncentred = pot.parametrisation != "centred"
        b8, t, beta = 8, 0, 0.0
        while True:
            if t >= S:
                raise RuntimeError(f"LikelihoodTemperedSMC: beta did not reach 1 within max_stages={S} stages")
            qn = pot.to_natural(q) if noncentred else q
            _lib.call("pbbi_loglik_glm", target.handle, qn.data_ptr(), 1, D, N, 0, U.data_ptr(), st)
            bptr = betas.data_ptr() + t * b8
            if self.fixed_betas is None:
                _lib.call("pbbi_smc_next_beta", U.data_ptr(), logw.data_ptr(), None, None, 1.0, N, N, D,
                          self.target_ess, bptr, info.data_ptr() + t * 2 * b8, _lib.F64, dev, st)
            _lib.call("pbbi_smc_reweight", U.data_ptr(), None, None, 1.0, N, N, D, bptr, logw.data_ptr(),
                      logz.data_ptr(), rec.data_ptr() + t * 2 * b8, _lib.F64, dev, st)
            a_out = empty((N,), np.int32, dev) if self.record_ancestors else anc
            _lib.call("pbbi_smc_resample_systematic", logw.data_ptr(), N, self.seed, t, q.data_ptr(), q_alt.data_ptr(),
                      N, D, rec.data_ptr() + (t * 2 + 1) * b8, self.resample_threshold, a_out.data_ptr(), None,
                      resampled.data_ptr() + t, status.data_ptr() + 4 * t, _lib.F64, dev, st)
            if self.record_ancestors:
                self.ancestors.append(a_out)
            q, q_alt = q_alt, q
            if self.fixed_betas is None:
                prev, beta = beta, float(betas[t + 1].item())        # the one device -> host read of the stage
                self.host_syncs += 1
                if not beta > prev:
                    TemperedSMC._raise_on_status(status, t + 1)
                    raise RuntimeError(f"LikelihoodTemperedSMC: stage {t + 1} could not raise beta above {prev!r} (the "
                                       "ESS of every step is below target_ess: particles of extreme likelihood)")
            else:
                beta = float(self.fixed_betas[t])
            _lib.call("pbbi_potential_set_likelihood_power", target.handle, 0.0, betas.data_ptr() + (t + 1) * b8, st)
            _lib.call("pbbi_hmc_run", target.handle, self.method, q.data_ptr(), None, None, None, reject.data_ptr(),
                      None, N, N, self.stepSize, self.numSteps, self.moves, self.flags, self.seed, t * self.moves, 0,
                      1.0, st)
            n_rej[t] += reject.sum()
            t += 1
            if beta == 1.0:
                break
        a_out = empty((N,), np.int32, dev) if self.record_ancestors else anc
        _lib.call("pbbi_smc_resample_systematic", logw.data_ptr(), N, self.seed, t, q.data_ptr(), q_alt.data_ptr(), N,
                  D, None, 1.0, a_out.data_ptr(), None, resampled.data_ptr() + t, status.data_ptr() + 4 * t, _lib.F64,
                  dev, st)
        if self.record_ancestors:
            self.ancestors.append(a_out)
        return t, q_alt
