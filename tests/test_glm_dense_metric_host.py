"""The dense metric of the GLM handles, host side (no device): the packer and checker pbbi_glm_pack_metric_dense of
csrc/glm_host.cpp, the three ABI entries in the headers, the ctypes tables and the library's dynamic symbols, the shrinkage of
HMC.adaptMassMatrix(dense=True) against hand values and LaplaceResult.dense_metric.  The kernels' side is
tests/test_glm_dense_metric.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"pbbi_potential_set_metric_dense", "pbbi_potential_get_metric_dense"}
PACKER = "pbbi_glm_pack_metric_dense"
DIMS = [1, 5, 16, 17, 33, 64]


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def dense_metric_of(D, seed=3):
    """M = R diag(30^((d + 0.5) / D)) R^T with R a seeded random orthogonal matrix: fully dense, condition number < 30,
    symmetric to the last bit, and with no symmetry of its own that a wrong row mapping could hide behind."""
    rs = np.random.RandomState(1000 * seed + D)
    R, _ = np.linalg.qr(rs.standard_normal((D, D)))
    M = (R * 30.0 ** ((np.arange(D) + 0.5) / D)) @ R.T
    return 0.5 * (M + M.T)




def _padded(A, DP):
    out = np.eye(DP)
    out[:A.shape[0], :A.shape[1]] = A
    return out


def decode(img, DP):
    """One (DP x DP) image back into the matrix by the lane maps the kernel walks it with: K-step pair s2 of tile t holds, in
    lane l and half e, A[16 t + (l & 15)][4 (2 s2 + e) + (l >> 4)] -- and, pushed through an emulation of the product, tile t
    of A b lands in register r of lane l as row 16 t + 4 r + (l >> 4) of chain l & 15."""
    KS, NT = DP // 4, DP // 16
    frag = img.reshape(NT, KS // 2, 64, 2)
    lane = np.arange(64)
    g, c = lane >> 4, lane & 15
    A = np.full((DP, DP), np.nan)
    for t in range(NT):
        for s2 in range(KS // 2):
            for e in range(2):
                A[16 * t + c, 4 * (2 * s2 + e) + g] = frag[t, s2, :, e]
    # the product as the MFMA forms it: D[i = g + 4 r][j = c] += sum_k A[i][k] B[k][j], the A operand of a lane being
    # A[i = l & 15][k = l >> 4] and the B operand B[k = l >> 4][j = l & 15] -- with B = integer state registers, exact
    rs = np.random.RandomState(DP)
    B = rs.randint(-4, 5, size=(DP, 16)).astype(np.float64)
    q = np.stack([B[4 * s + g, c] for s in range(KS)])             # the state layout: register s of a lane is row 4 s + g
    out = np.zeros((DP, 16))
    for t in range(NT):
        acc = np.zeros((64, 4))
        for s in range(KS):
            a = frag[t, s // 2, :, s % 2]                          # per lane: A[16 t + (l & 15)][4 s + (l >> 4)]
            Amat, Bmat = np.zeros((16, 4)), np.zeros((4, 16))
            Amat[c, g] = a
            Bmat[g, c] = q[s]
            Dm = Amat @ Bmat
            for r in range(4):
                acc[:, r] += Dm[g + 4 * r, c]
        for r in range(4):
            out[16 * t + 4 * r + g, c] = acc[:, r]
    assert np.allclose(out, A @ B, rtol=1e-13, atol=1e-13)
    return A


def test_dense_metric_abi_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pbbi.h")).read()
    own = open(os.path.join(ROOT, "include", "pbbi_glm_metric.h")).read()
    for n in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % n, hdr), n
    assert re.search(r"\bint %s\s*\(" % PACKER, own) and '#include "pbbi_glm_metric.h"' in hdr
    assert "at most ONE metric" in hdr
    from physicsbasedbayesianinference_amd import _lib, glm
    assert ENTRIES <= set(_lib.PROTOTYPES) and PACKER in _lib.HOST_PACKER_PROTOTYPES and PACKER not in _lib.PROTOTYPES
    assert [len(_lib.PROTOTYPES[n]) for n in sorted(ENTRIES)] == [4, 3] and len(_lib.HOST_PACKER_PROTOTYPES[PACKER]) == 5
    assert "pack_metric_dense" in glm.__all__
    lib = _lib.load()
    assert lib.pbbi_version() == 103
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert ENTRIES | {PACKER} <= set(re.findall(r"\bT (pbbi_[a-z0-9_]+)", out))
    for n in ENTRIES:
        assert getattr(lib, n).argtypes == _lib.PROTOTYPES[n]
    assert getattr(lib, PACKER).argtypes == _lib.HOST_PACKER_PROTOTYPES[PACKER]


@pytest.mark.parametrize("D", DIMS)
def test_pack_length_protocol_and_short_buffer(D):
    from physicsbasedbayesianinference_amd import _lib, glm
    lib = _lib.load()
    DP = glm.padded_dim(D)
    assert DP == (16 if D <= 16 else 32 if D <= 32 else 64)
    n = C.c_int64(-1)
    assert lib.pbbi_glm_pack_metric_dense(D, None, None, 0, C.byref(n)) == _lib.OK and n.value == 3 * DP * DP
    M = dense_metric_of(D)
    short = np.full(3 * DP * DP - 1, -7.0)
    assert lib.pbbi_glm_pack_metric_dense(D, _dptr(M), _dptr(short), short.size, C.byref(n)) == _lib.ERR_INVALID
    assert "shorter" in _lib.last_error() and np.all(short == -7.0) and n.value == 3 * DP * DP
    full = np.full(3 * DP * DP, -7.0)
    assert lib.pbbi_glm_pack_metric_dense(D, None, _dptr(full), full.size, C.byref(n)) == _lib.ERR_INVALID
    assert "NULL" in _lib.last_error() and np.all(full == -7.0)
    assert lib.pbbi_glm_pack_metric_dense(D, _dptr(M), _dptr(full), full.size, None) == _lib.OK
    assert np.array_equal(full.reshape(3, -1, 64, 2), glm.pack_metric_dense(M))


@pytest.mark.parametrize("D", DIMS)
def test_images_are_the_inverse_the_factor_and_the_matrix(D):
    """Decoded by the lane maps: inv(M) to 1e-12 relative, cholesky(M) likewise, M itself exactly -- each with the identity on
    the padding rows and columns."""
    from physicsbasedbayesianinference_amd import glm
    DP = glm.padded_dim(D)
    M = dense_metric_of(D)
    img = glm.pack_metric_dense(M)
    assert img.shape == (3, DP * DP // 128, 64, 2)
    Cd, Ld, Md = (decode(img[m], DP) for m in range(3))
    assert np.array_equal(Md, _padded(M, DP))
    Ci, Lc = _padded(np.linalg.inv(M), DP), _padded(np.linalg.cholesky(M), DP)
    assert np.max(np.abs(Cd - Ci)) <= 1e-12 * np.max(np.abs(Ci))
    assert np.max(np.abs(Ld - Lc)) <= 1e-12 * np.max(np.abs(Lc))
    assert np.array_equal(Ld, np.tril(Ld)) and np.all(np.diag(Ld) > 0.0) and np.array_equal(Cd, Cd.T)
    # an asymmetry inside the rule is symmetrised: (M + M^T) / 2 is what is packed
    if D > 1:
        A = M.copy()
        A[0, 1] += 1e-13 * np.max(np.abs(M))
        assert np.array_equal(decode(glm.pack_metric_dense(A)[2], DP), _padded(0.5 * (A + A.T), DP))


def test_rejections_code_text_and_order():
    from physicsbasedbayesianinference_amd import _lib, glm
    lib = _lib.load()

    def refuse(D, M):
        out = np.full(3 * 64 * 64, -7.0)
        n = C.c_int64(-1)
        rc = lib.pbbi_glm_pack_metric_dense(D, _dptr(M) if M is not None else None, _dptr(out), out.size, C.byref(n))
        assert rc != _lib.OK and np.all(out == -7.0)
        return rc, _lib.last_error()

    # D = 65 comes first: refused whatever the matrix holds, even with out = NULL
    bad65 = np.full((65, 65), np.nan)
    rc, msg = refuse(65, bad65)
    assert rc == _lib.ERR_UNSUPPORTED and "1 <= D <= 64" in msg and "D = 65" in msg
    assert lib.pbbi_glm_pack_metric_dense(65, None, None, 0, None) == _lib.ERR_UNSUPPORTED
    assert lib.pbbi_glm_pack_metric_dense(0, None, None, 0, None) == _lib.ERR_UNSUPPORTED
    M = dense_metric_of(5)
    # NaN before asymmetry before definiteness
    A = M.copy()
    A[3, 4] = np.nan
    A[0, 1] += 1.0
    A[2, 2] = -50.0
    rc, msg = refuse(5, A)
    assert rc == _lib.ERR_INVALID and "finite" in msg and "entry 3, 4" in msg
    A[3, 4] = np.inf
    assert refuse(5, A)[1].find("finite") >= 0
    A[3, 4] = M[3, 4]
    rc, msg = refuse(5, A)
    assert rc == _lib.ERR_INVALID and "symmetric" in msg and "1e-12" in msg
    A[0, 1] = M[0, 1]
    rc, msg = refuse(5, A)                       # indefinite
    assert rc == _lib.ERR_INVALID and "positive definite" in msg
    v = np.array([1.0, 2.0, -1.0, 0.5, 3.0])
    rc, msg = refuse(5, np.outer(v, v))          # singular (rank one)
    assert rc == _lib.ERR_INVALID and "positive definite" in msg
    rc, msg = refuse(5, np.zeros((5, 5)))
    assert rc == _lib.ERR_INVALID and "positive definite" in msg
    # the Python packer: every refusal is a ValueError; pack_metric keeps refusing 2-D input with its own message
    for bad in (A, np.outer(v, v), np.ones((3, 4)), np.ones(3)):
        with pytest.raises(ValueError):
            glm.pack_metric_dense(bad)
    with pytest.raises(ValueError, match="vector of D >= 1 masses"):
        glm.pack_metric(M)


def test_regularized_covariance_against_hand_values():
    from physicsbasedbayesianinference_amd.HMC import regularized_covariance, regularized_variance
    cov = np.array([[4.0, 1.0], [1.0, 9.0]])
    got = regularized_covariance(cov, 95)           # n / (n + 5) = 0.95, 1e-3 * 5 / 100 = 5e-5 on the diagonal
    assert np.allclose(got, [[3.80005, 0.95], [0.95, 8.55005]], rtol=1e-15, atol=0)
    got = regularized_covariance(cov, 5)
    assert np.allclose(got, [[2.0005, 0.5], [0.5, 4.5005]], rtol=1e-15, atol=0)
    assert np.array_equal(np.diag(regularized_covariance(cov, 25)), regularized_variance(np.diag(cov), 25))
    asym = np.array([[1.0, 0.25], [0.75, 1.0]])     # symmetrised
    assert np.array_equal(regularized_covariance(asym, 95), regularized_covariance(asym.T, 95))
    with pytest.raises(ValueError):
        regularized_covariance(np.ones(3), 10)


def test_dense_metric_of_a_hand_built_laplace_result():
    from physicsbasedbayesianinference_amd.laplace import LaplaceResult
    H = np.array([[2.0, 0.5, 0.0], [0.5 + 1e-15, 3.0, -1.0], [0.0, -1.0, 4.0]])
    fit = LaplaceResult(np.zeros(3), H, 0.0)
    assert np.array_equal(fit.dense_metric, 0.5 * (H + H.T)) and np.array_equal(fit.dense_metric, fit.dense_metric.T)
    assert np.allclose(np.linalg.inv(fit.dense_metric), fit.covariance, rtol=1e-13)
    assert np.allclose(1.0 / np.diag(np.linalg.inv(fit.dense_metric)), fit.metric, rtol=1e-13)
    fit.dense_metric[0, 0] = 99.0                   # a fresh array each time: the result's Hessian is not touched
    assert fit.hessian[0, 0] == 2.0
