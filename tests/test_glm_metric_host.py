"""The diagonal metric of the GLM handles, host side (no device): the packer and checker pbbi_glm_pack_metric of
csrc/glm_host.cpp, the three ABI entries in the header, the ctypes table and the library's dynamic symbols, and the shrinkage
of HMC.adaptMassMatrix against hand values.  The kernels' side is tests/test_glm_metric.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"pbbi_potential_set_metric_diag", "pbbi_potential_get_metric_diag", "pbbi_glm_pack_metric"}


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_metric_abi_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pbbi.h")).read()
    assert '#include "pbbi_glm_metric.h"' in hdr     # the host-only packer's declaration: a part of pbbi.h in a file of its own
    hdr += open(os.path.join(ROOT, "include", "pbbi_glm_metric.h")).read()
    for n in NAMES:
        assert re.search(r"\bint %s\s*\(" % n, hdr), n
    assert "share the metric" in hdr           # two samplers that share a handle share the metric: said where it is declared
    from physicsbasedbayesianinference_amd import _lib, glm
    table = {**_lib.PROTOTYPES, **_lib.HOST_PACKER_PROTOTYPES}
    assert NAMES <= set(table)
    assert [len(table[n]) for n in sorted(NAMES)] == [5, 4, 3]     # pack_metric, get_metric_diag, set_metric_diag
    assert "pack_metric" in glm.__all__
    for cls in (glm.GLM, glm.SoftmaxGLM, glm.DispersionGLM, glm.HierarchicalGLM, glm.HierarchicalDispersionGLM):
        assert callable(getattr(cls, "set_metric")) and isinstance(getattr(cls, "metric"), property), cls
    _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert NAMES <= set(re.findall(r"\bT (pbbi_[a-z0-9_]+)", out))


@pytest.mark.parametrize("D", [1, 5, 16, 17, 33, 64, 65, 128])
def test_pack_metric_layout_padding_and_length_protocol(D):
    """{m_d, 1 / m_d} in 16-byte entries, {1, 1} on the rows past D up to the padded dimension; the length comes first
    (out = NULL), a short buffer is refused and left alone; callable without a device."""
    from physicsbasedbayesianinference_amd import _lib, glm
    L = _lib.load()
    DP = 16 if D <= 16 else 32 if D <= 32 else 64 if D <= 64 else 128
    m = 30.0 ** ((np.arange(D) + 0.5) / D)
    n = C.c_int64(-1)
    assert L.pbbi_glm_pack_metric(D, None, None, 0, C.byref(n)) == _lib.OK and n.value == 2 * DP
    assert L.pbbi_glm_pack_metric(D, None, None, 0, None) == _lib.OK          # len_out is optional
    out = np.full(2 * DP, -7.0)
    assert L.pbbi_glm_pack_metric(D, _dptr(m), _dptr(out), out.size, C.byref(n)) == _lib.OK and n.value == 2 * DP
    tab = out.reshape(DP, 2)
    assert np.array_equal(tab[:D, 0], m) and np.array_equal(tab[:D, 1], 1.0 / m)
    assert np.all(tab[D:] == 1.0)
    assert np.array_equal(glm.pack_metric(m), tab)
    short = np.full(2 * DP - 1, -7.0)
    assert L.pbbi_glm_pack_metric(D, _dptr(m), _dptr(short), short.size, C.byref(n)) == _lib.ERR_INVALID
    assert "shorter" in _lib.last_error() and np.all(short == -7.0) and n.value == 2 * DP
    assert L.pbbi_glm_pack_metric(D, None, _dptr(out), out.size, C.byref(n)) == _lib.ERR_INVALID
    assert "NULL" in _lib.last_error()


def test_pack_metric_ones_table_is_exactly_ones():
    from physicsbasedbayesianinference_amd import glm
    assert np.all(glm.pack_metric(np.ones(50)) == 1.0)


@pytest.mark.parametrize("bad", [0.0, -1.0, -0.0, np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("D,where", [(1, 0), (17, 0), (17, 16), (128, 77)])
def test_pack_metric_rejects_entries_that_are_no_mass(D, where, bad):
    from physicsbasedbayesianinference_amd import _lib
    L = _lib.load()
    m = np.linspace(1.0, 3.0, D)
    m[where] = bad
    out = np.full(256, -7.0)
    n = C.c_int64(0)
    assert L.pbbi_glm_pack_metric(D, _dptr(m), _dptr(out), out.size, C.byref(n)) == _lib.ERR_INVALID
    assert "finite and > 0" in _lib.last_error() and f"row {where}" in _lib.last_error()
    assert np.all(out == -7.0)                                               # nothing written


@pytest.mark.parametrize("D", [0, -3, 129])
def test_pack_metric_rejects_dimensions_no_kernel_has(D):
    from physicsbasedbayesianinference_amd import _lib
    n = C.c_int64(-1)
    assert _lib.load().pbbi_glm_pack_metric(D, None, None, 0, C.byref(n)) == _lib.ERR_INVALID and n.value == -1


def test_regularized_variance_against_hand_values():
    """Stan's shrinkage n / (n + 5) var + 1e-3 * 5 / (n + 5): n = 5 halves the estimate and adds 5e-4; n = 95 keeps 95 % and
    adds 5e-5; a zero variance still gives a finite mass."""
    from physicsbasedbayesianinference_amd.HMC import regularized_variance
    assert regularized_variance(2.0, 5) == pytest.approx(1.0 + 5e-4, rel=1e-15)
    assert regularized_variance(1.0, 95) == pytest.approx(0.95 + 5e-5, rel=1e-15)
    got = regularized_variance(np.array([0.0, 1e-4, 4.0]), 45)
    assert np.allclose(got, [1e-4, 0.9e-4 + 1e-4, 3.6 + 1e-4], rtol=1e-14, atol=0.0)
    assert np.all(np.isfinite(1.0 / got))


def test_mass_matrix_entries_refuse_a_potential_without_one():
    """HMC.setMassMatrix / massMatrix / adaptMassMatrix forward to the potential's set_metric; a potential class without
    that entry is a ValueError before anything else happens (no handle is needed to find out)."""
    from physicsbasedbayesianinference_amd.HMC import HMC

    class _NoMetric:
        pass

    h = HMC.__new__(HMC)
    h._pot = _NoMetric()
    with pytest.raises(ValueError, match="GLM potentials only"):
        h.setMassMatrix(np.ones(3))
    with pytest.raises(ValueError, match="GLM potentials only"):
        h.massMatrix
