"""The host side of the per-draw log-likelihood, the likelihood power and likelihood-tempered SMC (no GPU): the ABI, every
argument rule in the order include/pbbi.h states it, the improper priors `sample_prior` refuses and the arguments
`LikelihoodTemperedSMC` refuses.  Potentials are made without a device (`__new__` and the attributes the code reads), as
test_glm_hier_dispersion.hostpot does."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"pbbi_loglik_glm", "pbbi_loglik_glm_check", "pbbi_potential_set_likelihood_power",
         "pbbi_potential_get_likelihood_power", "pbbi_likelihood_power_check"}


def test_loglik_abi_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pbbi.h")).read()
    assert re.search(r"\bint\s+pbbi_loglik_glm\s*\(const pbbi_potential\* pot, const void\* samples_sdn, int S, int Dt, "
                     r"int64_t N, int ranges,\s*double\* ulik_out, void\* stream\);", hdr)
    assert re.search(r"\bint\s+pbbi_potential_set_likelihood_power\s*\(pbbi_potential\* pot, double beta, "
                     r"const double\* beta_dev, void\* stream\);", hdr)
    assert re.search(r"\bint\s+pbbi_potential_get_likelihood_power\s*\(const pbbi_potential\* pot, double\* beta_out\);", hdr)
    from physicsbasedbayesianinference_amd import _lib
    assert NAMES <= set(_lib.PROTOTYPES)
    assert len(_lib.PROTOTYPES["pbbi_loglik_glm"]) == 8 and len(_lib.PROTOTYPES["pbbi_potential_set_likelihood_power"]) == 4
    lib = _lib.load()
    for name in NAMES:
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name]
    assert lib.pbbi_version() == 103
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert NAMES <= set(re.findall(r"\bT (pbbi_[a-z0-9_]+)", out))
    assert not any(n.startswith("pbbi_glm_") for n in NAMES)      # outside the census of test_glm_abi_errors.py
    import physicsbasedbayesianinference_amd as P
    for cls in (P.GLM, P.DispersionGLM, P.HierarchicalGLM, P.HierarchicalDispersionGLM):
        for m in ("loglik", "sample_prior", "set_likelihood_power"):
            assert callable(getattr(cls, m))
        assert isinstance(cls.likelihood_power, property)
    assert P.LikelihoodTemperedSMC is P.smc.LikelihoodTemperedSMC
    assert "kernels_glm_loglik.hip" in open(os.path.join(ROOT, "physicsbasedbayesianinference_amd", "csrc", "Makefile")).read()


def test_loglik_rejects_bad_arguments_without_a_device():
    """Code and text of every rule, in the header's order: each case breaks every LATER rule too, so the answer names the
    first rule broken."""
    from physicsbasedbayesianinference_amd import _lib
    lib = _lib.load()
    buf = (C.c_double * 4)()
    ptr = C.addressof(buf)
    assert lib.pbbi_loglik_glm(None, ptr, 3, 5, 150, 0, ptr, None) == _lib.ERR_INVALID
    assert "handle is NULL" in _lib.last_error()
    good = dict(handle=1, family=_lib.GLM_LOGISTIC, state_dim=5, samples=ptr, out=ptr, S=3, Dt=5, N=150, ranges=0)

    def rc(**kw):
        a = dict(good, **kw)
        return lib.pbbi_loglik_glm_check(a["handle"], a["family"], a["state_dim"], a["samples"], a["out"], a["S"], a["Dt"],
                                         a["N"], a["ranges"])

    assert rc() == _lib.OK and rc(ranges=7) == _lib.OK and rc(ranges=65535) == _lib.OK and rc(Dt=9) == _lib.OK
    assert rc(S=1, N=1) == _lib.OK
    for fam in (_lib.GLM_POISSON, _lib.GLM_GAUSSIAN, _lib.GLM_NEGBINOMIAL):
        assert rc(family=fam) == _lib.OK
    order = [(dict(handle=0), _lib.ERR_INVALID, "handle is NULL"),
             (dict(samples=None), _lib.ERR_INVALID, "samples is NULL"),
             (dict(out=None), _lib.ERR_INVALID, "ulik_out is NULL"),
             (dict(S=0), _lib.ERR_INVALID, "S must be >= 1"),
             (dict(N=0), _lib.ERR_INVALID, "N must be >= 1"),
             (dict(ranges=65536), _lib.ERR_INVALID, "ranges must be"),
             (dict(handle=2), _lib.ERR_UNSUPPORTED, "not a GLM handle"),
             (dict(family=_lib.GLM_SOFTMAX), _lib.ERR_UNSUPPORTED, "softmax"),
             (dict(family=99), _lib.ERR_UNSUPPORTED, "unknown GLM family"),
             (dict(Dt=4), _lib.ERR_INVALID, "state dimension")]
    for i, (kw, code, text) in enumerate(order):
        assert rc(**kw) == code, kw
        assert text in _lib.last_error(), (kw, _lib.last_error())
        later = {}
        for k2, _, _ in order[i + 1:]:
            later.update({k: v for k, v in k2.items() if k not in later})      # (handle, family: the earliest later rule)
        later.update(kw)
        assert rc(**later) == code and text in _lib.last_error(), (kw, later, _lib.last_error())
    assert rc(S=-3) == _lib.ERR_INVALID and rc(N=-1) == _lib.ERR_INVALID and rc(ranges=-1) == _lib.ERR_INVALID
    assert rc(S=2000000000, N=1 << 40) == _lib.OK      # S * N is formed in 64 bits


def test_power_rejects_bad_arguments_without_a_device():
    from physicsbasedbayesianinference_amd import _lib
    lib = _lib.load()
    assert lib.pbbi_potential_set_likelihood_power(None, 0.5, None, None) == _lib.ERR_INVALID
    assert "handle is NULL" in _lib.last_error()
    out = C.c_double(7.0)
    assert lib.pbbi_potential_get_likelihood_power(None, C.byref(out)) == _lib.ERR_INVALID and out.value == 7.0

    def rc(handle=1, family=_lib.GLM_LOGISTIC, has_streams=1, beta=0.25, on_device=0):
        return lib.pbbi_likelihood_power_check(handle, family, has_streams, beta, on_device)

    assert rc() == _lib.OK and rc(beta=1.0) == _lib.OK and rc(beta=1e-300) == _lib.OK and rc(beta=3.0) == _lib.OK
    for fam in (_lib.GLM_POISSON, _lib.GLM_GAUSSIAN, _lib.GLM_NEGBINOMIAL):
        assert rc(family=fam) == _lib.OK
    assert rc(beta=float("nan"), on_device=1) == _lib.OK       # read from the device: the host value is not looked at
    # in the header's order; each case breaks the later rules too
    assert rc(handle=0, family=_lib.GLM_SOFTMAX, has_streams=0, beta=-1.0) == _lib.ERR_INVALID
    assert "handle is NULL" in _lib.last_error()
    assert rc(handle=2, family=_lib.GLM_SOFTMAX, has_streams=0, beta=-1.0) == _lib.ERR_UNSUPPORTED
    assert "not a GLM handle" in _lib.last_error() and "_glm_hier_dispersion" in _lib.last_error()
    assert rc(family=_lib.GLM_SOFTMAX, has_streams=0, beta=-1.0) == _lib.ERR_UNSUPPORTED
    assert "softmax" in _lib.last_error()
    assert rc(has_streams=0, beta=-1.0) == _lib.ERR_UNSUPPORTED
    assert "no observation streams" in _lib.last_error() and "pbbi_potential_create_glm_ex" in _lib.last_error()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert rc(beta=bad) == _lib.ERR_INVALID
        assert "finite and > 0" in _lib.last_error()


def fake(cls, **attrs):
    pot = cls.__new__(cls)
    for k, v in attrs.items():
        setattr(pot, k, v)
    return pot


def test_sample_prior_refuses_improper_priors():
    """Each kind of improper prior, named by its row, before anything touches a device."""
    import physicsbasedbayesianinference_amd as P
    base = dict(device=0, prior_mean=None)
    # a flat coefficient: scalar and vector precisions
    with pytest.raises(ValueError, match=r"row 0 is improper \(prior_precision\[0\] = 0\)"):
        fake(P.GLM, numDimensions=3, prior_precision=0.0, **base).sample_prior(8)
    with pytest.raises(ValueError, match=r"row 2 is improper \(prior_precision\[2\] = 0\)"):
        fake(P.GLM, numDimensions=3, prior_precision=np.array([1.0, 2.0, 0.0]), **base).sample_prior(8)
    # a flat log-dispersion
    with pytest.raises(ValueError, match=r"row 2 is improper \(log_dispersion_prior = 0\)"):
        fake(P.DispersionGLM, numDimensions=3, numCoefficients=2, prior_precision=np.ones(2), sampled=True,
             log_dispersion_prior=(0.0, 0.0), **base).sample_prior(8)
    hier = dict(numDimensions=5, numCoefficients=3, numGroups=2, groups=np.array([-1, 0, 1], dtype=np.int32), penalty=None,
                parametrisation="centred", **base)
    # a flat fixed row; the (ignored, zero) precision of a grouped row is NOT one
    with pytest.raises(ValueError, match=r"row 0 is improper \(prior_precision\[0\] = 0\)"):
        fake(P.HierarchicalGLM, prior_precision=np.zeros(3), log_scale_prior=np.array([[0.0, 1.0], [0.0, 1.0]]),
             **hier).sample_prior(8)
    # a flat log-scale
    with pytest.raises(ValueError, match=r"row 4 is improper \(log_scale_prior\[1\] = 0\)"):
        fake(P.HierarchicalGLM, prior_precision=np.array([1.0, 0.0, 0.0]),
             log_scale_prior=np.array([[0.0, 1.0], [0.0, 0.0]]), **hier).sample_prior(8)
    # a structured prior, full rank or not
    with pytest.raises(ValueError, match=r"group 1 has a structured prior \(penalty\[1\]\)"):
        fake(P.HierarchicalGLM, prior_precision=np.array([1.0, 0.0, 0.0]), log_scale_prior=np.array([[0.0, 1.0], [0.0, 1.0]]),
             **dict(hier, penalty=[None, np.eye(1)])).sample_prior(8)
    # the hierarchical-dispersion class: theta's row is the last
    with pytest.raises(ValueError, match=r"row 5 is improper \(log_dispersion_prior = 0\)"):
        fake(P.HierarchicalDispersionGLM, prior_precision=np.array([1.0, 0.0, 0.0]), sampled=True,
             log_dispersion_prior=(0.0, 0.0), log_scale_prior=np.array([[0.0, 1.0], [0.0, 1.0]]),
             **dict(hier, numDimensions=6)).sample_prior(8)
    with pytest.raises(ValueError, match="N must be >= 1"):
        fake(P.GLM, numDimensions=3, prior_precision=1.0, **base).sample_prior(0)
    assert not hasattr(P.SoftmaxGLM, "sample_prior")


def test_likelihood_tempered_smc_rejects_bad_arguments():
    import physicsbasedbayesianinference_amd as P
    pot = fake(P.GLM, numDimensions=3, device=0)
    ok = dict(numParticles=64, simulTime=1.0, stepSize=0.1)
    smc = P.LikelihoodTemperedSMC(pot, **ok)
    assert smc.numSteps == 10 and smc.moves == 5 and smc.logML is None and smc.host_syncs == 0
    assert P.LikelihoodTemperedSMC(pot, betas=[0.1, 0.5, 1.0], **ok).max_stages == 3
    for kw in (dict(numParticles=0), dict(target_ess=0.0), dict(target_ess=1.0), dict(resample_threshold=1.5), dict(moves=0),
               dict(stepSize=0.0), dict(simulTime=-1.0), dict(method="euler"), dict(betas=[0.5, 0.4, 1.0]), dict(betas=[0.0, 1.0]),
               dict(betas=[0.5, 0.9]), dict(betas=[[0.5, 1.0]]), dict(betas=[0.5, float("nan"), 1.0]), dict(max_stages=0)):
        with pytest.raises(ValueError):
            P.LikelihoodTemperedSMC(pot, **dict(ok, **kw))
    for other in (fake(P.SoftmaxGLM, numDimensions=6, device=0), fake(P.StandardGaussian, numDimensions=3, device=0), None,
                  lambda q: 0.0):
        with pytest.raises(ValueError, match="LikelihoodTemperedSMC serves"):
            P.LikelihoodTemperedSMC(other, **ok)
    with pytest.raises(ValueError, match="finite and > 0"):
        fake(P.GLM, numDimensions=3, device=0, _plain=False, _twin=None).set_likelihood_power(0.0)
