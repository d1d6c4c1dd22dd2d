"""Softmax regression (glm.SoftmaxGLM, csrc/kernels_glm_softmax.hip): K-class multinomial logistic regression whose K
eta tiles and K gradient tile groups run on the fp64 MFMA units, the softmax in lane.

The oracle side is the user-source mechanism, as in tests/test_glm.py: `orc.pot_custom(complete_source(SOFTMAX_SOURCE),
K * D, prm)` with prm = [M, K, X.ravel(), y, lam (D values)].

Tolerance: 1e-10 relative to max(1, max|.|) -- tests/test_glm.py's figure for these models (the MFMA sums run in another
order than the oracle's loops); reject masks are compared for equality.  Every HMC comparison first requires the ORACLE's
reject fraction to lie strictly inside (0, 1) by the margins stated at the test: a mask of all-accept proves nothing.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10

SOFTMAX_SOURCE = """
template <class Q>
PBBI_FN T potential(const Q& q, int DT, const T* prm) {
    const int M = (int)prm[0], K = (int)prm[1];
    const int D = DT / K;
    const T* X = prm + 2;
    const T* y = X + (long)M * D;
    const T* lam = y + M;
    T s = 0;
    for (int i = 0; i < M; ++i) {
        T z[16]; T m = 0;
        for (int k = 0; k < K; ++k) {
            T a = 0;
            for (int j = 0; j < D; ++j) a += X[i * D + j] * q[k * D + j];
            z[k] = a; if (k == 0 || a > m) m = a;
        }
        T Z = 0;
        for (int k = 0; k < K; ++k) Z += exp(z[k] - m);
        s += (m + log(Z)) - z[(int)y[i]];
    }
    T r = 0;
    for (int k = 0; k < K; ++k) for (int j = 0; j < D; ++j) r += lam[j] * q[k * D + j] * q[k * D + j];
    return s + T(0.5) * r;
}
template <class Q, class G>
PBBI_FN void gradient(const Q& q, G& g, int DT, const T* prm) {
    const int M = (int)prm[0], K = (int)prm[1];
    const int D = DT / K;
    const T* X = prm + 2;
    const T* y = X + (long)M * D;
    const T* lam = y + M;
    for (int k = 0; k < K; ++k) for (int j = 0; j < D; ++j) g[k * D + j] = lam[j] * q[k * D + j];
    for (int i = 0; i < M; ++i) {
        T z[16]; T m = 0;
        for (int k = 0; k < K; ++k) {
            T a = 0;
            for (int j = 0; j < D; ++j) a += X[i * D + j] * q[k * D + j];
            z[k] = a; if (k == 0 || a > m) m = a;
        }
        T Z = 0;
        for (int k = 0; k < K; ++k) { z[k] = exp(z[k] - m); Z += z[k]; }
        for (int k = 0; k < K; ++k) {
            const T w = z[k] / Z - (k == (int)y[i] ? T(1) : T(0));
            for (int j = 0; j < D; ++j) g[k * D + j] += w * X[i * D + j];
        }
    }
}
"""

# (M, D, K, N, h, L)
CASES = {
    "A": (37, 5, 3, 131, 0.3, 8),      # NT = 3 (odd); D % 4 != 0: padded rows beside a live class, draws straddle blocks;
                                       # ragged last observation block, ragged last wave, ghost waves
    "B": (64, 16, 8, 67, 0.3, 8),      # NT = 8, the register-heaviest instantiation; no padding anywhere; whole blocks
    "C": (203, 20, 4, 131, 0.2, 10),   # Dc = 32: two tiles per class, NT = 8
    "D": (100, 40, 2, 67, 0.3, 10),    # Dc = 64: four tiles per class, K = 2
}
ALL = sorted(CASES)


def problem(M, D, K, seed=11):
    rs = np.random.RandomState(seed)
    X = rs.standard_normal((M, D)) / np.sqrt(D); X[:, 0] = 1.0
    W = rs.standard_normal((K, D))
    eta = X @ W.T
    p = np.exp(eta - eta.max(1, keepdims=True)); p /= p.sum(1, keepdims=True)
    y = np.array([rs.choice(K, p=pi) for pi in p], dtype=np.float64)
    return X, y, W.ravel(), rs


def lam_of(D):
    return np.r_[0.25, np.ones(D - 1)]


def draws(case, mass=False, kT=1.0):
    """X, y, lam, then -- in this order from the problem's own stream -- q, p0, u; p = p0 sqrt(mass kT)."""
    M, D, K, N, h, L = CASES[case]
    X, y, w, rs = problem(M, D, K)
    q = np.ascontiguousarray(w[:, None] + 0.3 * rs.standard_normal((K * D, N)))
    p0 = rs.standard_normal((K * D, N))
    u = rs.uniform(size=N)
    m = 1.0 + (np.arange(N) % 3) * 0.5 if mass else None
    p = np.ascontiguousarray(p0 * np.sqrt((m if mass else 1.0) * kT))
    return X, y, lam_of(D), q, p, u, m


def softmax_params(X, y, K, lam):
    return np.concatenate([[float(X.shape[0]), float(K)], X.ravel(), y, lam])


@functools.lru_cache(maxsize=None)
def oracle_pot(case):
    from physicsbasedbayesianinference_amd import custom
    M, D, K = CASES[case][:3]
    X, y, w, rs = problem(M, D, K)
    return orc.pot_custom(custom.complete_source(SOFTMAX_SOURCE), K * D, softmax_params(X, y, K, lam_of(D)))


@functools.lru_cache(maxsize=None)
def device_pot(case):
    import physicsbasedbayesianinference_amd as pkg
    M, D, K = CASES[case][:3]
    X, y, w, rs = problem(M, D, K)
    return pkg.SoftmaxGLM(X, y, classes=K, prior_precision=lam_of(D))


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape
    assert np.all(np.isfinite(b)), "oracle value not finite"
    assert np.all(np.isfinite(a)), "device value not finite"
    return float(np.max(np.abs(a - b))) / max(1.0, float(np.max(np.abs(b))))


def check(name, a, b, tol=TOL):
    e = rel(a, b)
    print(f"{name}: {e:.3e}")
    assert e <= tol, (name, e)


# ------------------------------------------------------------------------------------------------ CPU
def test_softmax_abi_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pbbi.h")).read()
    assert re.search(r"\bpbbi_potential_create_glm_softmax\s*\(", hdr)
    assert re.search(r"\bpbbi_glm_softmax_layout\s*\(", hdr)
    assert "PBBI_GLM_SOFTMAX = 2" in hdr
    import physicsbasedbayesianinference_amd as pkg
    from physicsbasedbayesianinference_amd import _lib, glm
    assert _lib.GLM_SOFTMAX == 2
    assert {"pbbi_potential_create_glm_softmax", "pbbi_glm_softmax_layout"} <= set(_lib.PROTOTYPES)
    assert pkg.SoftmaxGLM is glm.SoftmaxGLM and "SoftmaxGLM" in pkg.__all__
    assert issubclass(pkg.SoftmaxGLM, pkg.Potential) and pkg.SoftmaxGLM.kind == "glm"
    lib = _lib.load()
    assert lib.pbbi_version() == 103
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (pbbi_[a-z0-9_]+)", out))
    assert {"pbbi_potential_create_glm_softmax", "pbbi_glm_softmax_layout"} <= exported


LAYOUT_OK = [CASES[c][1:3] for c in ALL] + [(16, 8), (32, 4), (64, 2), (17, 4), (1, 2)]


@pytest.mark.parametrize("D,K", LAYOUT_OK)
def test_softmax_layout_is_a_bijection(D, K):
    from physicsbasedbayesianinference_amd import glm
    Dc, NT, row_map = glm.softmax_layout(D, K)
    assert Dc == glm.padded_dim(D) and NT == K * Dc // 16 and NT <= 8
    assert row_map.dtype == np.int32 and row_map.shape == (NT * 16,)
    live = row_map[row_map >= 0]
    assert np.array_equal(np.sort(live), np.arange(K * D)) and np.all(row_map[row_map < 0] == -1)
    for k in range(K):   # class k's rows lie in class k's tiles, in order, padding behind them
        mine = row_map[k * Dc:(k + 1) * Dc]
        assert np.array_equal(mine[:D], k * D + np.arange(D)) and np.all(mine[D:] == -1)


@pytest.mark.parametrize("D,K", [(17, 5), (33, 3), (65, 2), (16, 9), (5, 1)])
def test_softmax_layout_refuses_other_shapes(D, K):
    from physicsbasedbayesianinference_amd import _lib, glm
    with pytest.raises(ValueError, match="K \\* Dc <= 128"):
        glm.softmax_layout(D, K)
    Dc, NT = C.c_int(), C.c_int()
    assert _lib.load().pbbi_glm_softmax_layout(D, K, C.byref(Dc), C.byref(NT), None) == _lib.ERR_UNSUPPORTED


def test_softmax_rejects_bad_arguments_on_the_host():
    from physicsbasedbayesianinference_amd import SoftmaxGLM
    rs = np.random.RandomState(0)
    X = rs.standard_normal((10, 3))
    y = (np.arange(10) % 3).astype(float)
    bad = [
        dict(X=X, y=y + 0.5),                                          # labels not integral
        dict(X=X, y=y - 1.0),                                          # ... negative
        dict(X=X, y=y, classes=2),                                     # ... >= classes
        dict(X=X, y=np.zeros(10), classes=1),                          # classes < 2
        dict(X=X, y=np.zeros(10)),                                     # (default: max(y) + 1 = 1)
        dict(X=X, y=y, classes=9),                                     # shapes outside the rule
        dict(X=rs.standard_normal((10, 17)), y=y, classes=5),
        dict(X=rs.standard_normal((10, 33)), y=y, classes=3),
        dict(X=rs.standard_normal((10, 65)), y=(np.arange(10) % 2).astype(float)),
        dict(X=np.where(np.arange(30).reshape(10, 3) == 4, np.inf, X), y=y),   # X not finite
        dict(X=np.where(np.arange(30).reshape(10, 3) == 7, np.nan, X), y=y),
        dict(X=X, y=np.where(np.arange(10) == 2, np.nan, y)),
        dict(X=X, y=y, prior_precision=-1.0),                          # precision negative / NaN
        dict(X=X, y=y, prior_precision=np.nan),
        dict(X=X, y=y, prior_precision=np.r_[1.0, -1.0, 1.0]),
        dict(X=X, y=y, prior_precision=np.r_[1.0, np.nan, 1.0]),
        dict(X=X, y=y, prior_precision=np.ones(4)),                    # ... of the wrong length
        dict(X=X, y=y, prior_precision=np.ones((3, 1))),
        dict(X=X.ravel(), y=y),                                        # X not 2-D, y of another length
        dict(X=X, y=y[:9]),
        dict(X=X, y=y, dtype="float32"),                               # fp64 only
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            SoftmaxGLM(**kw)


def test_softmax_c_entry_checks_before_the_gpu():
    """The C entry point returns its argument errors without a device: INVALID for the data, UNSUPPORTED for the shape
    rule (with a message that states it) and for fp32; the two older creation calls keep refusing family 2."""
    from physicsbasedbayesianinference_amd import _lib
    L = _lib.load()
    dp = C.POINTER(C.c_double)
    ptr = lambda a: a.ctypes.data_as(dp)
    X, y, lam = np.ones((4, 3)), np.array([0.0, 1.0, 2.0, 1.0]), np.ones(3)
    h = C.c_void_p()
    create = L.pbbi_potential_create_glm_softmax
    for yy in (y + 0.5, y - 1.0, y + 1.0):
        assert create(3, 3, 4, ptr(X), ptr(yy), ptr(lam), _lib.F64, 0, C.byref(h)) == _lib.ERR_INVALID and not h
    assert create(3, 1, 4, ptr(X), ptr(np.zeros(4)), ptr(lam), _lib.F64, 0, C.byref(h)) == _lib.ERR_INVALID
    assert create(3, 3, 4, ptr(X * np.inf), ptr(y), ptr(lam), _lib.F64, 0, C.byref(h)) == _lib.ERR_INVALID
    assert create(3, 3, 4, ptr(X), ptr(y), ptr(-lam), _lib.F64, 0, C.byref(h)) == _lib.ERR_INVALID
    assert create(3, 3, 4, ptr(X), ptr(y), ptr(lam * np.nan), _lib.F64, 0, C.byref(h)) == _lib.ERR_INVALID
    assert create(3, 3, 4, ptr(X), ptr(y), ptr(lam), _lib.F32, 0, C.byref(h)) == _lib.ERR_UNSUPPORTED and not h
    X17 = np.ones((4, 17))
    assert create(17, 5, 4, ptr(X17), ptr(y), ptr(np.ones(17)), _lib.F64, 0, C.byref(h)) == _lib.ERR_UNSUPPORTED
    assert "K * Dc <= 128" in _lib.last_error() and not h
    assert create(3, 9, 4, ptr(X), ptr(y), ptr(lam), _lib.F64, 0, C.byref(h)) == _lib.ERR_UNSUPPORTED
    assert L.pbbi_potential_create_glm(3, 4, ptr(X), ptr(y), 2, 1.0, _lib.F64, 0, C.byref(h)) == _lib.ERR_INVALID
    assert L.pbbi_potential_create_glm_ex(3, 4, ptr(X), ptr(y), 2, None, None, None, ptr(lam), None, _lib.F64, 0,
                                          C.byref(h)) == _lib.ERR_INVALID


def _mfma(A, B, Cacc):
    """v_mfma_f64_16x16x4_f64 on per-lane operands: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15];
    register r of lane l of C/D is element (row (l >> 4) + 4 r, column l & 15)."""
    tile = A.reshape(4, 16).T @ B.reshape(4, 16)   # [i][j]
    lane = np.arange(64)
    for r in range(4):
        Cacc[:, r] += tile[(lane >> 4) + 4 * r, lane & 15]


@pytest.mark.parametrize("case", ["A", "C"])
def test_softmax_walk_feeds_every_class(case):
    """The kernel's walk replayed in NumPy on the packed image and the row map (small integers: every sum is exact): K eta
    tiles from the same P1 fragments, then each class's gradient tiles from P2, equal X @ W_k and X.T @ R_k."""
    from physicsbasedbayesianinference_amd import glm
    M, D, K = CASES[case][:3]
    rs = np.random.RandomState(1000 * M + D)
    X = rs.randint(-9, 10, size=(M, D)).astype(np.float64)
    W = rs.randint(-9, 10, size=(K * D, 16)).astype(np.float64)      # the (K D, N) state of 16 chains
    R = rs.randint(-9, 10, size=(K, M, 16)).astype(np.float64)
    Dc, NT, row_map = glm.softmax_layout(D, K)
    NTc, KSc = Dc // 16, Dc // 4
    img = glm.pack_design(X)
    nb = (M + 15) // 16
    assert img.shape == ((nb + 3) // 4 * 4, 2, Dc * 16)
    lane = np.arange(64)
    g, c = lane >> 4, lane & 15
    Wi = np.where(row_map[:, None] >= 0, W[np.maximum(row_map, 0)], 0.0)     # internal rows: padding loads 0
    q = np.stack([Wi[4 * s + g, c] for s in range(K * KSc)])       # element s of a lane is internal row 4s + g
    Rp = np.zeros((K, 16 * nb, 16))
    Rp[:, :M] = R
    gacc = np.zeros((NT, 64, 4))
    for b in range(nb):
        P1 = img[b, 0].reshape(KSc // 2, 64, 2)
        P2 = img[b, 1].reshape(2, NTc, 64, 2)
        eta = np.zeros((K, 64, 4))
        for s2 in range(KSc // 2):          # every fragment read once, used by all K classes
            for k in range(K):
                for e in range(2):
                    _mfma(P1[s2, :, e], q[k * KSc + 2 * s2 + e], eta[k])
        for k in range(K):
            ref = np.zeros((16 * nb, 16))
            ref[:M] = X @ W[k * D:(k + 1) * D]
            for r in range(4):
                assert np.array_equal(eta[k][:, r], ref[16 * b + 4 * r + g, c])
        for r2 in range(2):
            for t in range(NTc):
                for k in range(K):
                    for e in range(2):
                        _mfma(P2[r2, t, :, e], Rp[k, 16 * b + 4 * (2 * r2 + e) + g, c], gacc[k * NTc + t])
    got = np.zeros((K * D, 16))
    for t in range(NT):
        for r in range(4):
            rows = row_map[16 * t + 4 * r + g]
            ok = rows >= 0
            assert not gacc[t][~ok, r].any()                         # padded rows collect zeros (and are never stored)
            got[rows[ok], c[ok]] = gacc[t][ok, r]
    for k in range(K):
        assert np.array_equal(got[k * D:(k + 1) * D], X.T @ R[k])


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def P():
    import physicsbasedbayesianinference_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def lib():
    from physicsbasedbayesianinference_amd import _lib
    _lib.load()
    return _lib


def _dev():
    from physicsbasedbayesianinference_amd import _device
    return _device


def padded(arr, ldn):
    """(D, N) host array -> device tensor with leading stride ldn > N (the tail holds a poison value)."""
    import torch
    D, N = arr.shape
    t = torch.full((D, ldn), 1e300, dtype=torch.float64, device="cuda:0")
    t[:, :N] = torch.from_numpy(np.ascontiguousarray(arr)).to("cuda:0")
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL)
def test_softmax_eval_matches_oracle(P, lib, case):
    import torch
    d = _dev()
    M, D, K, N, h, L = CASES[case]
    X, y, lam, q, p, u, m = draws(case)
    pot, op = device_pot(case), oracle_pot(case)
    assert pot.numDimensions == K * D and pot.classes == K
    Uo, go = orc.potential(op, q, want_grad=True)
    ldn = N + 5
    qd = padded(q, ldn)
    U = torch.full((N,), -7.0, dtype=torch.float64, device="cuda:0")
    gd = torch.full((K * D, ldn), -7.0, dtype=torch.float64, device="cuda:0")
    lib.call("pbbi_potential_eval", pot.handle, qd.data_ptr(), N, ldn, U.data_ptr(), gd.data_ptr(), d.stream_ptr(0))
    torch.cuda.synchronize()
    check(f"U {case}", U.cpu().numpy(), Uo)
    check(f"grad {case}", gd[:, :N].cpu().numpy(), go)
    assert np.all(gd[:, N:].cpu().numpy() == -7.0), "stores past N"
    assert np.array_equal(qd[:, :N].cpu().numpy(), q) and np.all(qd[:, N:].cpu().numpy() == 1e300)
    # the class API (ldn == N) and the view by class
    check("call", pot(q), Uo)
    gq = pot.gradient(q)
    check("gradient", gq, go)
    Wk = pot.coefficients(gq)
    assert Wk.shape == (K, D, N) and np.shares_memory(Wk, gq) and np.array_equal(Wk[K - 1, D - 1], gq[K * D - 1])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL)
@pytest.mark.parametrize("method", ["Leapfrog", "Stormer-Verlet"])
@pytest.mark.parametrize("mass", [False, True])
@pytest.mark.parametrize("kt", [False, True])
def test_softmax_uploaded_draw_iteration_matches_oracle(P, lib, case, method, mass, kt):
    """Every run's ORACLE reject fraction must lie in [0.05, 0.9]."""
    import torch
    d = _dev()
    M, D, K, N, h, L = CASES[case]
    kT = 2.0 if kt else 1.0
    X, y, lam, q, p, u, m = draws(case, mass, kT)
    pot, op = device_pot(case), oracle_pot(case)
    DT = K * D
    qd, pd, ud = (d.as_device(a, 0, np.float64) for a in (q, p, u))
    md = d.as_device(m, 0, np.float64) if mass else None
    qo, po = d.empty((DT, N), np.float64, 0), d.empty((DT, N), np.float64, 0)
    ratio, rej = d.empty((N,), np.float64, 0), d.empty((N,), np.uint8, 0)
    mi = 0 if method == "Leapfrog" else 1
    args = [pot.handle, mi, qd.data_ptr(), pd.data_ptr(), ud.data_ptr(), md.data_ptr() if mass else None, qo.data_ptr(),
            po.data_ptr(), ratio.data_ptr(), rej.data_ptr(), N, N, h, L]
    if kt:
        lib.call("pbbi_hmc_iter_kt", *args, lib.COMPAT_P_FROM_OLDQ | lib.BETA_ACCEPT, kT, d.stream_ptr(0))
    else:
        lib.call("pbbi_hmc_iter", *args, lib.COMPAT_P_FROM_OLDQ, d.stream_ptr(0))
    torch.cuda.synchronize()
    r_o, rej_o = orc.hmc_iter(op, method, q, p, u, m, h, L, beta=1.0 / kT)
    frac = rej_o.mean()
    print("reject fraction", frac)
    assert np.all(np.isfinite(r_o)) and 0.05 <= frac <= 0.9
    grej = d.to_numpy(rej).astype(bool)
    print("mask mismatches", int((grej != rej_o).sum()), "ratio err", rel(d.to_numpy(ratio), r_o))
    assert np.array_equal(grej, rej_o)
    check("q", d.to_numpy(qo), q)
    check("p", d.to_numpy(po), p)
    check("ratio", d.to_numpy(ratio), r_o)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL)
def test_softmax_philox_run_matches_oracle(P, lib, case):
    """pbbi_hmc_run, PBBI_DRAW_F64: the oracle draws its own momenta of the (K D, N) state (no device draw is replayed).
    The oracle's overall reject fraction must lie in [0.05, 0.6]."""
    import torch
    d = _dev()
    M, D, K, N, h, L = CASES[case]
    X, y, lam, q, p, u, m = draws(case)
    pot, op = device_pot(case), oracle_pot(case)
    DT, S = K * D, 3
    seed, iter0, chain0 = 17, 3, 1000003
    ldn = N + 5
    qd = padded(q, ldn)
    samples, momenta = d.empty((S, DT, N), np.float64, 0), d.empty((S, DT, N), np.float64, 0)
    rej, ratio = d.empty((S, N), np.uint8, 0), d.empty((S, N), np.float64, 0)
    flags = lib.COMPAT_P_FROM_OLDQ | lib.DRAW_F64
    lib.call("pbbi_hmc_run", pot.handle, 0, qd.data_ptr(), None, samples.data_ptr(), momenta.data_ptr(), rej.data_ptr(),
             ratio.data_ptr(), N, ldn, h, L, S, flags, seed, iter0, chain0, 1.0, d.stream_ptr(0))
    torch.cuda.synchronize()
    so, mo, rejo, ro = orc.hmc_run_philox(op, "Leapfrog", q, None, h, L, S, seed, iter0, chain0, 1.0,
                                          compat=orc.COMPAT_P_FROM_OLDQ | orc.DRAW_F64)
    frac = rejo.mean()
    print("reject fraction", frac, rejo.mean(axis=1))
    assert all(np.all(np.isfinite(a)) for a in (so, mo, ro)) and 0.05 <= frac <= 0.6
    assert np.array_equal(d.to_numpy(rej).astype(bool), rejo)
    check("samples", d.to_numpy(samples), so)
    check("momenta", d.to_numpy(momenta), mo)
    check("ratio", d.to_numpy(ratio), ro)
    check("final state", qd[:, :N].cpu().numpy(), q)
    assert np.all(qd[:, N:].cpu().numpy() == 1e300)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["A", "C"])
def test_softmax_single_precision_draw_is_mapped_row_for_row(P, lib, case):
    """One pbbi_hmc_run of S = 1 (f32 draw) equals, bit for bit, pbbi_hmc_iter fed with pbbi_philox_normal(seed, momentum
    stream, iter, chain0, K D, N) and pbbi_philox_uniform: the kernel's draw is the draw of a (K D, N) state.  Without
    PBBI_COMPAT_P_FROM_OLDQ as well: a rejected chain then reports the drawn momentum itself."""
    import torch
    from test_gpu_parity import device_normal, device_uniform
    d = _dev()
    M, D, K, N, h, L = CASES[case]
    X, y, lam, q, p, u, m = draws(case)
    pot = device_pot(case)
    DT = K * D
    seed, it, chain0 = 23, 5, 77
    z = np.ascontiguousarray(device_normal(lib, seed, lib.STREAM_MOMENTUM, it, chain0, DT, N))
    uu = device_uniform(lib, seed, it, chain0, N)
    for flags in (lib.COMPAT_P_FROM_OLDQ, 0):
        qd = d.as_device(q, 0, np.float64)
        s1, m1 = d.empty((1, DT, N), np.float64, 0), d.empty((1, DT, N), np.float64, 0)
        r1, a1 = d.empty((1, N), np.uint8, 0), d.empty((1, N), np.float64, 0)
        lib.call("pbbi_hmc_run", pot.handle, 0, qd.data_ptr(), None, s1.data_ptr(), m1.data_ptr(), r1.data_ptr(),
                 a1.data_ptr(), N, N, h, L, 1, flags, seed, it, chain0, 1.0, d.stream_ptr(0))
        q2, pd, ud = (d.as_device(a, 0, np.float64) for a in (q, z, uu))
        qo, po = d.empty((DT, N), np.float64, 0), d.empty((DT, N), np.float64, 0)
        a2, r2 = d.empty((N,), np.float64, 0), d.empty((N,), np.uint8, 0)
        lib.call("pbbi_hmc_iter", pot.handle, 0, q2.data_ptr(), pd.data_ptr(), ud.data_ptr(), None, qo.data_ptr(),
                 po.data_ptr(), a2.data_ptr(), r2.data_ptr(), N, N, h, L, flags, d.stream_ptr(0))
        torch.cuda.synchronize()
        assert np.array_equal(d.to_numpy(s1)[0], d.to_numpy(qo))
        assert np.array_equal(d.to_numpy(m1)[0], d.to_numpy(po))
        assert np.array_equal(d.to_numpy(a1)[0], d.to_numpy(a2))
        assert np.array_equal(d.to_numpy(r1)[0], d.to_numpy(r2))
        rj = d.to_numpy(r2).astype(bool)
        assert 0 < rj.sum() < N
        if flags == 0:
            assert np.array_equal(d.to_numpy(m1)[0][:, rj], z[:, rj])


@pytest.mark.gpu
def test_softmax_run_fused_bit_identically(P, lib):
    """A run of S = 7 equals seven runs of one bit for bit; the burn-in form ends in the same state.  Case A, masses."""
    import torch
    d = _dev()
    M, D, K, N, h, L = CASES["A"]
    X, y, lam, q0, p, u, m = draws("A", mass=True)
    pot = device_pot("A")
    DT, S, seed, chain0, iter0 = K * D, 7, 8, 5, 2
    md = d.as_device(m, 0, np.float64)
    st = d.stream_ptr(0)

    def run(s_per_call, record=True):
        qd = d.as_device(q0, 0, np.float64)
        samples, momenta = d.empty((S, DT, N), np.float64, 0), d.empty((S, DT, N), np.float64, 0)
        reject, ratio = d.empty((S, N), np.uint8, 0), d.empty((S, N), np.float64, 0)
        for i in range(0, S, s_per_call):
            lib.call("pbbi_hmc_run", pot.handle, 0, qd.data_ptr(), md.data_ptr(),
                     samples[i].data_ptr() if record else None, momenta[i].data_ptr() if record else None,
                     reject[i].data_ptr() if record else None, ratio[i].data_ptr() if record else None,
                     N, N, h, L, min(s_per_call, S - i), lib.COMPAT_P_FROM_OLDQ, seed, iter0 + i, chain0, 1.0, st)
        torch.cuda.synchronize()
        return tuple(d.to_numpy(a) for a in (samples, momenta, reject, ratio, qd))

    one, each = run(S), run(1)
    for a, b in zip(one, each):
        assert np.array_equal(a, b)
    assert np.all(np.isfinite(one[0])) and 0.02 < one[2].mean() < 0.98
    assert np.array_equal(run(S, record=False)[4], one[4])


@pytest.mark.gpu
def test_softmax_integrators_and_energies_match_oracle(P, lib):
    """Leapfrog / StormerVerlet(...).integrate() of the class API, pbbi_energy and pbbi_weights_ratio.  Case A, masses."""
    import torch
    d = _dev()
    M, D, K, N, h, L = CASES["A"]
    X, y, lam, q0, p0, u, m = draws("A", mass=True)
    pot, op = device_pot("A"), oracle_pot("A")
    DT = K * D
    for cls, method in ((P.Leapfrog, "Leapfrog"), (P.StormerVerlet, "Stormer-Verlet")):
        q, p = q0.copy(), p0.copy()
        ens = P.Ensemble(DT, N)
        ens.mass = m.copy()
        ens.q[...] = q
        ens.p[...] = p
        integ = cls(ens, h, h * L + 0.5 * h, pot.gradient)
        assert integ.numSteps == L
        qd, pd = integ.integrate()
        v = orc.integrate(op, method, q, p, m, h, L)
        check(method + " q", np.asarray(qd), q)
        check(method + " p", np.asarray(pd), p)
        check(method + " v", np.asarray(integ.v), v)
    rs = np.random.RandomState(5)
    q2 = np.ascontiguousarray(q0 + 0.1 * rs.standard_normal(q0.shape))
    p2 = np.ascontiguousarray(rs.standard_normal(p0.shape))
    qd, pd, q2d, p2d, md = (d.as_device(a, 0, np.float64) for a in (q0, p0, q2, p2, m))
    H, wgt, ratio = (d.empty((N,), np.float64, 0) for _ in range(3))
    st = d.stream_ptr(0)
    lib.call("pbbi_energy", pot.handle, qd.data_ptr(), pd.data_ptr(), md.data_ptr(), N, N, H.data_ptr(), wgt.data_ptr(), st)
    lib.call("pbbi_weights_ratio", pot.handle, q2d.data_ptr(), p2d.data_ptr(), qd.data_ptr(), pd.data_ptr(), md.data_ptr(),
             N, N, ratio.data_ptr(), st)
    torch.cuda.synchronize()
    wo, Ho = orc.weights(op, q0, p0, m)
    check("H", d.to_numpy(H), Ho)
    check("w", d.to_numpy(wgt), wo)
    check("weights_ratio", d.to_numpy(ratio), orc.weights_ratio(op, q2, p2, q0, p0, m))


@pytest.mark.gpu
@pytest.mark.parametrize("rng,N", [("philox", 256), ("numpy", 96)])
def test_softmax_agrees_with_the_plugin_path(P, rng, N):
    """HMC through the class API on SoftmaxGLM(X, y) and on the same model as a CustomPotential: equal masks."""
    from scipy.constants import k as kB
    from physicsbasedbayesianinference_amd.custom import CustomPotential
    M, D, K = CASES["A"][:3]
    X, y, w, rs = problem(M, D, K)
    out = []
    for pot in (P.SoftmaxGLM(X, y), CustomPotential(K * D, SOFTMAX_SOURCE, softmax_params(X, y, K, np.ones(D)))):
        assert pot.numDimensions == 15
        np.random.seed(99)
        hmc = P.HMC(P.Ensemble(15, N), 2.4, 0.3, None, potential=pot, rng=rng, seed=13, verbose=False)
        s, m = hmc.getSamples(6, 1 / kB, 1.0)
        out.append((np.asarray(s), np.asarray(m), np.asarray(hmc.reject_masks)))
    assert np.array_equal(out[0][2], out[1][2])
    assert 0.02 < out[1][2].mean() < 0.9
    check("samples", out[0][0], out[1][0])
    check("momenta", out[0][1], out[1][1])


@pytest.mark.gpu
def test_softmax_through_the_classes_and_unsupported_calls(P, lib):
    from scipy.constants import k as kB
    from physicsbasedbayesianinference_amd.smc import TemperedSMC
    d = _dev()
    M, D, K = CASES["A"][:3]
    X, y, w, rs = problem(M, D, K)
    pot = P.SoftmaxGLM(X, y)
    assert pot.classes == 3 and pot.numDimensions == 15
    smc = TemperedSMC(pot, 15, 1024, 1.0, 0.2, 2.0, seed=3)
    q = smc.run()
    assert smc.betas[-1] == 1.0 and np.isfinite(smc.logZ)
    assert np.all(np.isfinite(np.asarray(q.cpu() if hasattr(q, "cpu") else q)))
    from physicsbasedbayesianinference_amd.tempering import TemperingLadder, geometric_ladder
    ladder = TemperingLadder(pot, 15, 64, geometric_ladder(4.0, 3), simulTime=1.0, stepSize=0.2, seed=5)
    x = np.asarray(ladder.run(numSamples=3, qStd=1.0, swap_every=1, burn_in=2))
    assert x.shape == (15, 64, 3) and np.all(np.isfinite(x))
    hmc = P.HMC(P.Ensemble(15, 256), 2.4, 0.3, None, potential=pot, rng="philox", seed=13, verbose=False)
    st = hmc.sampleStats(8, 4, 1 / kB, 1.0, max_lag=2)
    assert isinstance(st, P.RunningStats) and st.count == 8 and 0.0 < hmc.acceptRate <= 1.0
    text = hmc.describeRun()
    print(text)
    assert "k_glm_softmax" in text and "K = 3" in text and "padded to 16" in text
    assert "iterations per launch: up to 1" in text
    with pytest.raises(lib.PbbiError) as e:
        hmc.getSamplesGIST(2, 1 / kB, 1.0)
    assert e.value.code == lib.ERR_UNSUPPORTED
    N, S = 64, 2
    qd = d.as_device(np.ascontiguousarray(w[:, None] + 0.3 * rs.standard_normal((15, N))), 0, np.float64)
    samples = d.empty((S, 15, N), np.float64, 0)
    L = lib.load()
    rc = L.pbbi_hmc_run_dyn(pot.handle, 0, qd.data_ptr(), None, samples.data_ptr(), None, None, None, None, N, N, 0.1, 4,
                            S, lib.COMPAT_P_FROM_OLDQ | lib.PER_CHAIN_STEPS, 1, 0, 0, 1.0, d.stream_ptr(0))
    assert rc == lib.ERR_UNSUPPORTED, lib.last_error()
    rc = L.pbbi_hmc_run_gist(pot.handle, qd.data_ptr(), None, samples.data_ptr(), None, None, None, None, N, N, 0.1, 4, S,
                             lib.COMPAT_P_FROM_OLDQ, 1, 0, 0, 1.0, d.stream_ptr(0))
    assert rc == lib.ERR_UNSUPPORTED, lib.last_error()
    p, u = d.as_device(rs.standard_normal((15, N)), 0, np.float64), d.as_device(rs.uniform(size=N), 0, np.float64)
    rc = L.pbbi_hmc_iter_dyn(pot.handle, 0, qd.data_ptr(), p.data_ptr(), u.data_ptr(), None, None, samples.data_ptr(), None,
                             None, None, None, N, N, 0.1, 4, lib.PER_CHAIN_STEPS, 1.0, d.stream_ptr(0))
    assert rc == lib.ERR_UNSUPPORTED, lib.last_error()
