"""Host side of the GLM Hessian and the Laplace approximation (no GPU): the order of pbbi_glm_hessian's rejections through its
by-value twin pbbi_glm_hessian_check, the binding of the two entries, where `laplace` is bound, the algebra of a hand-made
LaplaceResult, and start= on the parity path of HMC.

The two entries are declared in include/pbbi_glm_hessian.h (which pbbi.h includes) and bound under _lib.HESSIAN_PROTOTYPES, beside
ORDINAL_PROTOTYPES and for its reason: tests/test_glm_abi_errors.py reads every pbbi_glm_* name of _lib.PROTOTYPES as a create /
pack entry whose rejections it spells out, and tests/test_host_logic.py holds _lib.PROTOTYPES equal to the names of pbbi.h alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from physicsbasedbayesianinference_amd import _lib, glm, laplace

INVALID, UNSUPPORTED = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
PTR = C.c_void_p(64)        # only compared with NULL


def check(handle, family, hier, q, out, ranges):
    rc = _lib.load().pbbi_glm_hessian_check(handle, family, hier, q, out, ranges)
    return rc, (_lib.last_error() if rc else "")


# every argument wrong at once, then mended one rule at a time: each call must stop at the FIRST rule it still breaks
SEQUENCE = [
    ((0, _lib.GLM_SOFTMAX, 1, None, None, -1), INVALID, "potential handle is NULL"),
    ((2, _lib.GLM_SOFTMAX, 1, None, None, -1), INVALID, "q is NULL"),
    ((2, _lib.GLM_SOFTMAX, 1, PTR, None, -1), INVALID, "hess_out is NULL"),
    ((2, _lib.GLM_SOFTMAX, 1, PTR, PTR, -1), INVALID, "ranges must be 0 (the library chooses) or 1 .. 65535 (ranges = -1)"),
    ((2, _lib.GLM_SOFTMAX, 1, PTR, PTR, 65536), INVALID, "ranges must be 0 (the library chooses) or 1 .. 65535 (ranges = 65536)"),
    ((2, _lib.GLM_SOFTMAX, 1, PTR, PTR, 0), UNSUPPORTED, "pbbi_glm_hessian: not a GLM handle: "),
    ((1, _lib.GLM_SOFTMAX, 1, PTR, PTR, 0), UNSUPPORTED, "pbbi_glm_hessian: a softmax handle is not served: "),
    ((1, _lib.GLM_ORDINAL, 1, PTR, PTR, 0), UNSUPPORTED, "pbbi_glm_hessian: an ordinal handle is not served: "),
    ((1, _lib.GLM_LOGISTIC, 1, PTR, PTR, 0), UNSUPPORTED, "pbbi_glm_hessian: a hierarchical handle (sampled group scales) is not served: "),
    ((1, 99, 0, PTR, PTR, 0), UNSUPPORTED, "pbbi_glm_hessian: unknown GLM family: "),
]


@pytest.mark.parametrize("args, code, text", SEQUENCE, ids=[s[2][:40] for s in SEQUENCE])
def test_rule_order(args, code, text):
    rc, msg = check(*args)
    assert rc == code and msg.startswith(text), (rc, msg)
    if code == UNSUPPORTED:
        assert msg.endswith("theta sampled or held)") and "_glm_dispersion" in msg        # the stated rule


@pytest.mark.parametrize("family", [_lib.GLM_LOGISTIC, _lib.GLM_POISSON, _lib.GLM_GAUSSIAN, _lib.GLM_NEGBINOMIAL, _lib.GLM_GAMMA])
@pytest.mark.parametrize("ranges", [0, 1, 65535])
def test_valid_calls_pass(family, ranges):
    assert check(1, family, 0, PTR, PTR, ranges) == (_lib.OK, "")


def test_symbols_are_bound_and_exported():
    assert sorted(_lib.HESSIAN_PROTOTYPES) == ["pbbi_glm_hessian", "pbbi_glm_hessian_check"]
    assert [len(_lib.HESSIAN_PROTOTYPES[n]) for n in sorted(_lib.HESSIAN_PROTOTYPES)] == [5, 6]
    lib = _lib.load()
    for n, argtypes in _lib.HESSIAN_PROTOTYPES.items():
        assert getattr(lib, n).argtypes == argtypes
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert set(_lib.HESSIAN_PROTOTYPES) <= set(re.findall(r"\bT (pbbi_[a-z0-9_]+)", out))
    hdr = open(os.path.join(ROOT, "include", "pbbi_glm_hessian.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(pbbi_[a-z0-9_]+)\s*\(", hdr))) == sorted(_lib.HESSIAN_PROTOTYPES)
    assert '#include "pbbi_glm_hessian.h"' in open(os.path.join(ROOT, "include", "pbbi.h")).read()
    assert lib.pbbi_version() == 103


def test_laplace_is_bound_on_two_classes_only():
    has = {c.__name__ for c in (glm.GLM, glm.SoftmaxGLM, glm.DispersionGLM, glm.OrdinalGLM, glm.HierarchicalGLM,
                                glm.HierarchicalDispersionGLM) if hasattr(c, "laplace")}
    assert has == {"GLM", "DispersionGLM"}
    assert glm.GLM.laplace is laplace.laplace and glm.DispersionGLM.laplace is laplace.laplace
    import physicsbasedbayesianinference_amd as P
    assert "LaplaceResult" in P.__all__ and P.LaplaceResult is laplace.LaplaceResult


# ---- LaplaceResult from a hand-made (mode, H, U): H = [[2, 1], [1, 3]], det 5, inverse [[3, -1], [-1, 2]] / 5
H2 = np.array([[2.0, 1.0], [1.0, 3.0]])


def hand_made(**kw):
    return laplace.LaplaceResult([0.5, -1.0], H2, 1.25, prior_precision=[4.0, 0.25], prior_names=["prior_precision[0]",
                                 "log_dispersion_prior"], constant=-0.75, **kw)


def test_result_algebra():
    fit = hand_made()
    assert np.allclose(fit.covariance, np.array([[3.0, -1.0], [-1.0, 2.0]]) / 5.0, rtol=0, atol=1e-15)
    assert np.array_equal(fit.covariance, fit.covariance.T)
    assert np.allclose(fit.stderr, np.sqrt([0.6, 0.4]), rtol=1e-15)
    assert np.allclose(fit.metric, [5.0 / 3.0, 2.5], rtol=1e-15)
    assert fit.converged and fit.iterations == 0 and fit.U == 1.25
    # -U + k + 1/2 [log(4 / 2pi) + log(0.25 / 2pi)] + (2 / 2) log 2pi - 1/2 log 5  =  -1.25 - 0.75 + 1/2 log(1) - 1/2 log 5
    assert abs(fit.log_evidence - (-2.0 - 0.5 * np.log(5.0))) <= 1e-14


def test_improper_row_raises_with_its_name():
    fit = laplace.LaplaceResult([0.0, 0.0], H2, 0.0, prior_precision=[1.0, 0.0], prior_names=["prior_precision[0]",
                                "log_dispersion_prior"])
    with pytest.raises(ValueError, match=r"the prior of row 1 is improper \(log_dispersion_prior = 0\)"):
        fit.log_evidence
    assert np.all(np.isfinite(fit.stderr))            # the rest of the algebra does not need a proper prior


def test_tempered_result_has_no_evidence():
    with pytest.raises(ValueError, match="likelihood power 0.5"):
        hand_made(power=0.5).log_evidence
    with pytest.raises(ValueError, match="likelihood power nan"):
        hand_made(power=float("nan")).log_evidence


def test_indefinite_hessian_raises_on_use():
    fit = laplace.LaplaceResult([0.0, 0.0], [[1.0, 2.0], [2.0, 1.0]], 0.0, converged=False)
    with pytest.raises(ValueError, match="not positive definite"):
        fit.covariance


def test_start_with_numpy_rng_raises():
    """The rule is stated before anything is allocated, so it is reached without a device."""
    from physicsbasedbayesianinference_amd import HMC
    hmc = HMC.__new__(HMC)
    hmc._pot = type("P", (), {"numDimensions": 2})()
    hmc.ensemble = type("E", (), {"numDimensions": 2, "numParticles": 4})()
    hmc.rng, hmc.seed = "numpy", 0
    with pytest.raises(ValueError, match="start needs rng='philox'"):
        hmc.getSamples(3, 1.0, 1.0, start=np.zeros((2, 4)))
    with pytest.raises(ValueError, match="start needs rng='philox'"):
        hmc.getSamples(3, 1.0, 1.0, rng="numpy", start=np.zeros((2, 4)))
