"""GLM potentials (physicsbasedbayesianinference_amd/glm.py, csrc/kernels_glm.hip): logistic and Poisson regression
whose likelihood runs as two fp64 MFMA products per gradient.

The oracle side is always the user-source mechanism: `orc.pot_custom(complete_source(SOURCE), D, prm)` with
prm = [M, X.ravel(), y, lambda] -- custom.LOGISTIC_REGRESSION_SOURCE is the oracle's statement of the logistic model,
POISSON_SOURCE below the same text with exp(z) - y z and weight exp(z) - y.

Tolerance: 1e-10 relative to max(1, max|.|) -- the project's figure for softplus models (the MFMA sums run in another
order than the oracle's loops); reject masks are compared for equality.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10

POISSON_SOURCE = """
template <class Q>
PBBI_FN T potential(const Q& q, int D, const T* prm) {
    const int M = (int)prm[0];
    const T* X = prm + 1;
    const T* y = X + (long)M * D;
    const T lam = y[M];
    T s = 0;
    for (int i = 0; i < M; ++i) {
        T z = 0;
        for (int j = 0; j < D; ++j) z += X[i * D + j] * q[j];
        s += exp(z) - y[i] * z;
    }
    T r = 0;
    for (int j = 0; j < D; ++j) r += q[j] * q[j];
    return s + (T(0.5) * lam) * r;
}
template <class Q, class G>
PBBI_FN void gradient(const Q& q, G& g, int D, const T* prm) {
    const int M = (int)prm[0];
    const T* X = prm + 1;
    const T* y = X + (long)M * D;
    const T lam = y[M];
    for (int j = 0; j < D; ++j) g[j] = lam * q[j];
    for (int i = 0; i < M; ++i) {
        T z = 0;
        for (int j = 0; j < D; ++j) z += X[i * D + j] * q[j];
        const T w = exp(z) - y[i];
        for (int j = 0; j < D; ++j) g[j] += w * X[i * D + j];
    }
}
"""


def problem(family, M, D, seed):
    rs = np.random.RandomState(seed)
    X = rs.standard_normal((M, D)) / np.sqrt(D)
    w = rs.standard_normal(D)
    eta = X @ w
    if family == "logistic":
        y = (rs.uniform(size=M) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    else:
        y = rs.poisson(np.exp(eta)).astype(np.float64)
    return X, y, w, rs


def start(w, N, rs):
    return np.ascontiguousarray(w[:, None] + 0.3 * rs.standard_normal((w.size, N)))


def oracle_pot(family, X, y, lam=1.0):
    from physicsbasedbayesianinference_amd import custom
    src = custom.LOGISTIC_REGRESSION_SOURCE if family == "logistic" else POISSON_SOURCE
    prm = np.concatenate([[float(X.shape[0])], X.ravel(), y, [float(lam)]])
    return orc.pot_custom(custom.complete_source(src), X.shape[1], prm)


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
def test_glm_abi_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pbbi.h")).read()
    assert re.search(r"\bpbbi_potential_create_glm\s*\(", hdr)
    assert "PBBI_GLM_LOGISTIC = 0" in hdr and "PBBI_GLM_POISSON = 1" in hdr
    from physicsbasedbayesianinference_amd import _lib
    assert "pbbi_potential_create_glm" in _lib.PROTOTYPES
    lib = _lib.load()
    assert lib.pbbi_version() == 103
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (pbbi_[a-z0-9_]+)", out))
    assert {"pbbi_potential_create_glm", "pbbi_glm_pack_design"} <= exported


def test_glm_rejects_bad_arguments_on_the_host():
    from physicsbasedbayesianinference_amd import GLM
    rs = np.random.RandomState(0)
    X = rs.standard_normal((10, 3))
    yb = (rs.uniform(size=10) < 0.5).astype(float)
    yc = rs.poisson(2.0, 10).astype(float)
    bad = [
        dict(X=X.ravel(), y=yb),                                   # X not 2-D
        dict(X=X[None], y=yb),
        dict(X=X, y=yb[:9]),                                       # y of another length
        dict(X=X, y=yb.reshape(10, 1)),
        dict(X=X, y=yb, family="gaussian"),                        # family unknown
        dict(X=X, y=yb + 0.5),                                     # logistic y not in {0, 1}
        dict(X=X, y=yc + 2.0, family="logistic"),
        dict(X=X, y=-yc - 1.0, family="poisson"),                  # poisson y < 0
        dict(X=X, y=yc + 0.25, family="poisson"),                  # ... not integral
        dict(X=X, y=yb, prior_precision=-1.0),                     # precision < 0
        dict(X=X, y=yb, prior_precision=np.nan),
        dict(X=rs.standard_normal((10, 129)), y=yb),               # D > 128
        dict(X=np.where(np.arange(30).reshape(10, 3) == 4, np.inf, X), y=yb),   # not finite
        dict(X=np.where(np.arange(30).reshape(10, 3) == 7, np.nan, X), y=yb),
        dict(X=X, y=np.where(np.arange(10) == 2, np.nan, yb)),
        dict(X=X, y=yb, dtype="float32"),                          # fp64 only
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            GLM(**kw)


def _mfma(A, B, Cacc):
    """v_mfma_f64_16x16x4_f64 on per-lane operands: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15];
    register r of lane l of C/D is element (row (l >> 4) + 4 r, column l & 15)."""
    tile = A.reshape(4, 16).T @ B.reshape(4, 16)   # [i][j]
    lane = np.arange(64)
    for r in range(4):
        Cacc[:, r] += tile[(lane >> 4) + 4 * r, lane & 15]


@pytest.mark.parametrize("M", [1, 16, 203])
@pytest.mark.parametrize("D", [1, 5, 16, 50, 128])
def test_pack_design_feeds_both_products(M, D):
    """The packed image, pushed through a NumPy emulation of the MFMA lane maps exactly as the kernel walks it,
    reproduces X @ W and X.T @ R (integer-valued inputs: every sum is exact)."""
    from physicsbasedbayesianinference_amd import glm
    rs = np.random.RandomState(1000 * M + D)
    X = rs.randint(-9, 10, size=(M, D)).astype(np.float64)
    W = rs.randint(-9, 10, size=(D, 16)).astype(np.float64)
    R = rs.randint(-9, 10, size=(M, 16)).astype(np.float64)
    DP = glm.padded_dim(D)
    KS, NT = DP // 4, DP // 16
    img = glm.pack_design(X)
    nb = (M + 15) // 16
    assert img.shape == ((nb + 3) // 4 * 4, 2, DP * 16)
    assert not img[nb:].any()
    lane = np.arange(64)
    g, c = lane >> 4, lane & 15
    Wp = np.zeros((DP, 16))
    Wp[:D] = W
    Rp = np.zeros((16 * nb, 16))
    Rp[:M] = R
    q = np.stack([Wp[4 * s + g, c] for s in range(KS)])      # state layout: element s of a lane is row 4s + g
    eta_ref, g_ref = np.zeros((16 * nb, 16)), np.zeros((DP, 16))
    eta_ref[:M] = X @ W
    g_ref[:D] = X.T @ R
    gacc = np.zeros((NT, 64, 4))
    for b in range(nb):
        P1 = img[b, 0].reshape(KS // 2, 64, 2)
        P2 = img[b, 1].reshape(2, NT, 64, 2)
        eta = np.zeros((64, 4))
        for s2 in range(KS // 2):
            for e in range(2):
                _mfma(P1[s2, :, e], q[2 * s2 + e], eta)
        for r in range(4):   # register r = observations {4r + g} of the lane's chain
            assert np.array_equal(eta[:, r], eta_ref[16 * b + 4 * r + g, c])
        res = np.stack([Rp[16 * b + 4 * r + g, c] for r in range(4)])
        for r2 in range(2):
            for t in range(NT):
                for e in range(2):
                    _mfma(P2[r2, t, :, e], res[2 * r2 + e], gacc[t])
    for t in range(NT):
        for r in range(4):   # rows 16t + 4r + g: the state layout again
            assert np.array_equal(gacc[t][:, r], g_ref[16 * t + 4 * r + g, c])


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
@pytest.mark.parametrize("family", ["logistic", "poisson"])
@pytest.mark.parametrize("M,D", [(1, 1), (40, 5), (203, 5), (512, 16), (1000, 50), (4096, 128)])
def test_glm_eval_matches_oracle(P, lib, family, M, D):
    import torch
    d = _dev()
    X, y, w, rs = problem(family, M, D, 7 * M + D)
    pot = P.GLM(X, y, family=family, prior_precision=1.0)
    op = oracle_pot(family, X, y)
    for N in (1, 17, 1003):
        q = start(w, N, rs)
        Uo, go = orc.potential(op, q, want_grad=True)
        ldn = N + 7
        qd = padded(q, ldn)
        U = torch.full((N,), -7.0, dtype=torch.float64, device="cuda:0")
        gd = torch.full((D, ldn), -7.0, dtype=torch.float64, device="cuda:0")
        lib.call("pbbi_potential_eval", pot.handle, qd.data_ptr(), N, ldn, U.data_ptr(), gd.data_ptr(), d.stream_ptr(0))
        torch.cuda.synchronize()
        check(f"U {family} {M}x{D} N={N}", U.cpu().numpy(), Uo)
        check(f"grad {family} {M}x{D} N={N}", gd[:, :N].cpu().numpy(), go)
        assert np.all(gd[:, N:].cpu().numpy() == -7.0), "stores past N"
    # the class API (ldn == N), U and gradient separately
    q = start(w, 33, rs)
    Uo, go = orc.potential(op, q, want_grad=True)
    check("call", pot(q), Uo)
    check("gradient", pot.gradient(q), go)


@pytest.mark.gpu
def test_glm_softplus_tails_and_energies(P, lib):
    """|eta| up to 40: U finite, gradient within tolerance; energy / weights_ratio against the oracle."""
    import torch
    d = _dev()
    M, D, N = 203, 5, 257
    X, y, w, rs = problem("logistic", M, D, 5)
    X = X * (40.0 / np.max(np.abs(X @ w)))
    pot = P.GLM(X, y)
    op = oracle_pot("logistic", X, y)
    q = np.ascontiguousarray(np.repeat(w[:, None], N, 1) * np.linspace(-1.0, 1.0, N)[None, :])
    assert 39.0 < np.max(np.abs(X @ q)) <= 40.0 + 1e-9
    Uo, go = orc.potential(op, q, want_grad=True)
    U, gq = pot.value_and_gradient(q)
    assert np.all(np.isfinite(U))
    check("tails U", U, Uo)
    check("tails grad", gq, go)
    # energies
    X, y, w, rs = problem("poisson", 300, 8, 6)
    pot, op = P.GLM(X, y, family="poisson"), oracle_pot("poisson", X, y)
    N = 1003
    q, q2 = start(w, N, rs), start(w, N, rs)
    p, p2 = rs.standard_normal((8, N)), rs.standard_normal((8, N))
    m = 1.0 + (np.arange(N) % 3) * 0.5
    qd, pd, q2d, p2d, md = (d.as_device(a, 0, np.float64) for a in (q, p, q2, p2, m))
    H, wgt, ratio = (d.empty((N,), np.float64, 0) for _ in range(3))
    st = d.stream_ptr(0)
    lib.call("pbbi_energy", pot.handle, qd.data_ptr(), pd.data_ptr(), md.data_ptr(), N, N, H.data_ptr(), wgt.data_ptr(), st)
    lib.call("pbbi_weights_ratio", pot.handle, q2d.data_ptr(), p2d.data_ptr(), qd.data_ptr(), pd.data_ptr(), md.data_ptr(),
             N, N, ratio.data_ptr(), st)
    torch.cuda.synchronize()
    wo, Ho = orc.weights(op, q, p, m)
    check("H", d.to_numpy(H), Ho)
    check("w", d.to_numpy(wgt), wo)
    ro = orc.weights_ratio(op, q2, p2, q, p, m)
    check("weights_ratio", d.to_numpy(ratio), ro)


ITER_CASES = [("logistic", 512, 16, 300, 0.4, 10), ("logistic", 203, 5, 300, 0.45, 8),
              ("poisson", 300, 8, 300, 0.1, 10)]


@pytest.mark.gpu
@pytest.mark.parametrize("family,M,D,N,h,L", ITER_CASES)
@pytest.mark.parametrize("method", ["Leapfrog", "Stormer-Verlet"])
@pytest.mark.parametrize("mass", [False, True])
@pytest.mark.parametrize("kt", [False, True])
def test_glm_uploaded_draw_iteration_matches_oracle(P, lib, family, M, D, N, h, L, method, mass, kt):
    import torch
    d = _dev()
    X, y, w, rs = problem(family, M, D, 11)
    pot, op = P.GLM(X, y, family=family), oracle_pot(family, X, y)
    N = N + 3  # ragged
    kT = 2.0 if kt else 1.0
    m = 1.0 + (np.arange(N) % 3) * 0.5 if mass else None
    q = start(w, N, rs)
    p = np.ascontiguousarray(rs.standard_normal((D, N)) * np.sqrt((m if mass else 1.0) * kT))
    u = rs.uniform(size=N)
    qd, pd, ud = (d.as_device(a, 0, np.float64) for a in (q, p, u))
    md = d.as_device(m, 0, np.float64) if mass else None
    qo, po = d.empty((D, N), np.float64, 0), d.empty((D, N), np.float64, 0)
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
    assert np.all(np.isfinite(r_o)) and 0.0 < frac < 1.0  # both outcomes occur, or equal masks say nothing
    grej = d.to_numpy(rej).astype(bool)
    print("mask mismatches", int((grej != rej_o).sum()), "ratio err", rel(d.to_numpy(ratio), r_o))
    assert np.array_equal(grej, rej_o)
    check("q", d.to_numpy(qo), q)
    check("p", d.to_numpy(po), p)
    check("ratio", d.to_numpy(ratio), r_o)


RUN_CASES = [("logistic", 512, 16, 300, 0.4, 10, 3), ("logistic", 203, 5, 300, 0.45, 8, 3),
             ("logistic", 1000, 50, 200, 0.25, 10, 5), ("logistic", 4096, 128, 100, 0.2, 10, 5),
             ("poisson", 300, 8, 300, 0.1, 10, 3), ("poisson", 1000, 50, 200, 0.12, 10, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("family,M,D,N,h,L,S", RUN_CASES)
def test_glm_philox_run_matches_oracle(P, lib, family, M, D, N, h, L, S):
    """pbbi_hmc_run, PBBI_DRAW_F64: the oracle draws its own momenta (no device draw is replayed)."""
    import torch
    d = _dev()
    X, y, w, rs = problem(family, M, D, 21)
    pot, op = P.GLM(X, y, family=family), oracle_pot(family, X, y)
    seed, iter0, chain0 = 17, 3, 1000003
    q = start(w, N, rs)
    ldn = N + 5
    qd = padded(q, ldn)
    samples, momenta = d.empty((S, D, N), np.float64, 0), d.empty((S, D, N), np.float64, 0)
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


@pytest.mark.gpu
@pytest.mark.parametrize("family,method", [("logistic", 0), ("logistic", 1), ("poisson", 0)])
def test_glm_run_fused_bit_identically(P, lib, family, method):
    """One run of S = 21 equals 21 runs of one, bit for bit; the burn-in form ends in the same state."""
    import torch
    d = _dev()
    M, D = (203, 5) if family == "logistic" else (300, 8)
    X, y, w, rs = problem(family, M, D, 31)
    pot = P.GLM(X, y, family=family)
    N, L, S, seed, chain0, iter0 = 777, 4, 21, 8, 5, 2
    h = 0.45 if family == "logistic" else 0.1
    m = 1.0 + (np.arange(N) % 3) * 0.5
    md = d.as_device(m, 0, np.float64)
    st = d.stream_ptr(0)
    q0 = start(w, N, rs)

    def run(s_per_call, record=True):
        qd = d.as_device(q0, 0, np.float64)
        samples, momenta = d.empty((S, D, N), np.float64, 0), d.empty((S, D, N), np.float64, 0)
        reject, ratio = d.empty((S, N), np.uint8, 0), d.empty((S, N), np.float64, 0)
        for i in range(0, S, s_per_call):
            lib.call("pbbi_hmc_run", pot.handle, method, qd.data_ptr(), md.data_ptr(),
                     samples[i].data_ptr() if record else None, momenta[i].data_ptr() if record else None,
                     reject[i].data_ptr() if record else None, ratio[i].data_ptr() if record else None,
                     N, N, h, L, min(s_per_call, S - i), lib.COMPAT_P_FROM_OLDQ, seed, iter0 + i, chain0, 1.0, st)
        torch.cuda.synchronize()
        return tuple(d.to_numpy(a) for a in (samples, momenta, reject, ratio, qd))

    one, each = run(S), run(1)
    for a, b in zip(one, each):
        assert np.array_equal(a, b)
    assert 0.02 < one[2].mean() < 0.98
    assert np.array_equal(run(S, record=False)[4], one[4])


@pytest.mark.gpu
@pytest.mark.parametrize("rng,N", [("philox", 4096), ("numpy", 96)])
def test_glm_agrees_with_the_plugin_path(P, rng, N):
    """HMC through the class API on GLM(X, y) and on logistic_regression_posterior(X, y): same draws, equal masks."""
    from scipy.constants import k as kB
    from physicsbasedbayesianinference_amd.custom import logistic_regression_posterior
    X, y, w, rs = problem("logistic", 256, 16, 41)
    out = []
    for pot in (P.GLM(X, y), logistic_regression_posterior(X, y)):
        np.random.seed(99)
        hmc = P.HMC(P.Ensemble(16, N), 4.0, 0.4, None, potential=pot, rng=rng, seed=13, verbose=False)
        s, m = hmc.getSamples(6, 1 / kB, 1.0)
        out.append((np.asarray(s), np.asarray(m), np.asarray(hmc.reject_masks)))
    assert np.array_equal(out[0][2], out[1][2])
    assert 0.02 < out[1][2].mean() < 0.9
    check("samples", out[0][0], out[1][0])
    check("momenta", out[0][1], out[1][1])


@pytest.mark.gpu
def test_glm_unsupported_calls(P, lib):
    import ctypes as C
    d = _dev()
    X, y, w, rs = problem("logistic", 40, 5, 1)
    pot = P.GLM(X, y)
    N, S = 64, 2
    q = d.as_device(start(w, N, rs), 0, np.float64)
    samples = d.empty((S, 5, N), np.float64, 0)
    L = lib.load()
    rc = L.pbbi_hmc_run_dyn(pot.handle, 0, q.data_ptr(), None, samples.data_ptr(), None, None, None, None, N, N, 0.1, 4,
                            S, lib.COMPAT_P_FROM_OLDQ | lib.PER_CHAIN_STEPS, 1, 0, 0, 1.0, d.stream_ptr(0))
    assert rc == lib.ERR_UNSUPPORTED, lib.last_error()
    rc = L.pbbi_hmc_run_gist(pot.handle, q.data_ptr(), None, samples.data_ptr(), None, None, None, None, N, N, 0.1, 4, S,
                             lib.COMPAT_P_FROM_OLDQ, 1, 0, 0, 1.0, d.stream_ptr(0))
    assert rc == lib.ERR_UNSUPPORTED, lib.last_error()
    p, u = d.as_device(rs.standard_normal((5, N)), 0, np.float64), d.as_device(rs.uniform(size=N), 0, np.float64)
    rc = L.pbbi_hmc_iter_dyn(pot.handle, 0, q.data_ptr(), p.data_ptr(), u.data_ptr(), None, None, samples.data_ptr(), None,
                             None, None, None, N, N, 0.1, 4, lib.PER_CHAIN_STEPS, 1.0, d.stream_ptr(0))
    assert rc == lib.ERR_UNSUPPORTED, lib.last_error()
    # creation: D = 129 and fp32
    dp = C.POINTER(C.c_double)
    Xb, yb = np.zeros((4, 129)), np.zeros(4)
    h = C.c_void_p()
    rc = L.pbbi_potential_create_glm(129, 4, Xb.ctypes.data_as(dp), yb.ctypes.data_as(dp), 0, 1.0, lib.F64, 0, C.byref(h))
    assert rc == lib.ERR_UNSUPPORTED and "128" in lib.last_error() and not h
    rc = L.pbbi_potential_create_glm(5, 40, X.ctypes.data_as(dp), y.ctypes.data_as(dp), 0, 1.0, lib.F32, 0, C.byref(h))
    assert rc == lib.ERR_UNSUPPORTED and not h
    # describe_run names the kernel and the iterations per launch
    buf = C.create_string_buffer(1024)
    lib.call("pbbi_describe_run", pot.handle, 0, N, N, 4, S, lib.COMPAT_P_FROM_OLDQ, buf, 1024)
    text = buf.value.decode()
    assert "k_glm" in text and "iterations per launch: up to 1" in text


@pytest.mark.gpu
def test_glm_integrators_match_oracle(P, lib):
    """pbbi_leapfrog / pbbi_stormer_verlet / pbbi_integrate (v_out) in place, with masses."""
    import torch
    d = _dev()
    X, y, w, rs = problem("logistic", 203, 5, 51)
    pot, op = P.GLM(X, y), oracle_pot("logistic", X, y)
    N, h, L = 131, 0.2, 7
    m = 1.0 + (np.arange(N) % 3) * 0.5
    for method in ("Leapfrog", "Stormer-Verlet"):
        q, p = start(w, N, rs), np.ascontiguousarray(rs.standard_normal((5, N)))
        qd, pd, md = (d.as_device(a, 0, np.float64) for a in (q, p, m))
        vd = d.empty((5, N), np.float64, 0)
        lib.call("pbbi_integrate", pot.handle, 0 if method == "Leapfrog" else 1, qd.data_ptr(), pd.data_ptr(), md.data_ptr(),
                 vd.data_ptr(), N, N, h, L, d.stream_ptr(0))
        torch.cuda.synchronize()
        v = orc.integrate(op, method, q, p, m, h, L)
        check(method + " q", d.to_numpy(qd), q)
        check(method + " p", d.to_numpy(pd), p)
        check(method + " v", d.to_numpy(vd), v)


@pytest.mark.gpu
@pytest.mark.parametrize("ragged", [0, 5])
def test_glm_full_size_run_vs_oracle(P, lib, ragged):
    """The timed shape M = 16 384, D = 64, N = 16 384: sixteen 16-chain groups (first and last tile, a tile boundary,
    random groups) replayed on the oracle from the device's draws for the same counters."""
    import torch
    from test_gpu_fullsize import GROUP, chain_groups
    from test_gpu_parity import device_normal, device_uniform
    d = _dev()
    M, D, S, h, L, seed = 16384, 64, 3, 0.16, 10, 5
    N = 16384 - ragged
    X, y, w, rs = problem("logistic", M, D, 61)
    pot, op = P.GLM(X, y), oracle_pot("logistic", X, y)
    q0 = start(w, N, rs)
    qd = d.as_device(q0, 0, np.float64)
    samples, momenta = d.empty((S, D, N), np.float64, 0), d.empty((S, D, N), np.float64, 0)
    rej = d.empty((S, N), np.uint8, 0)
    flags = lib.COMPAT_P_FROM_OLDQ | lib.DRAW_F64
    lib.call("pbbi_hmc_run", pot.handle, 0, qd.data_ptr(), None, samples.data_ptr(), momenta.data_ptr(), rej.data_ptr(),
             None, N, N, h, L, S, flags, seed, 0, 0, 1.0, d.stream_ptr(0))
    torch.cuda.synchronize()
    grej = d.to_numpy(rej).astype(bool)
    print("device reject fraction", grej.mean())
    # sixteen groups; the random ones are picked (by seed) where the device saw a rejection, the oracle must confirm it
    starts = set(chain_groups(N, 8, 64, 3))
    hit = np.flatnonzero(grej.any(axis=0))
    pick = np.random.RandomState(4).permutation(hit)
    for n in pick:
        if len(starts) >= 16:
            break
        starts.add(int(min(max(n - 3, 0), N - GROUP)))
    n_rej = 0
    for g0 in sorted(starts):
        sl = slice(g0, g0 + GROUP)
        q = np.ascontiguousarray(q0[:, sl])
        for i in range(S):
            p = np.ascontiguousarray(device_normal(lib, seed, lib.STREAM_MOMENTUM | lib.STREAM_DRAW_F64, i, g0, D, GROUP))
            u = device_uniform(lib, seed, i, g0, GROUP)
            ratio, r = orc.hmc_iter(op, "Leapfrog", q, p, u, None, h, L)
            assert np.all(np.isfinite(ratio)) and np.all(np.isfinite(q)) and np.all(np.isfinite(p))
            assert np.array_equal(grej[i, sl], r), (g0, i)
            check(f"q[{g0}] it {i}", samples[i, :, sl].cpu().numpy(), q)
            check(f"p[{g0}] it {i}", momenta[i, :, sl].cpu().numpy(), p)
            n_rej += int(r.sum())
        assert np.array_equal(qd[:, sl].cpu().numpy(), samples[S - 1, :, sl].cpu().numpy())
    assert n_rej >= 1


@pytest.mark.gpu
def test_tempered_smc_accepts_a_glm_target(P):
    from physicsbasedbayesianinference_amd.smc import TemperedSMC
    X, y, w, rs = problem("logistic", 203, 5, 71)
    smc = TemperedSMC(P.GLM(X, y), 5, 2048, 1.0, 0.2, 2.0, seed=3)
    q = smc.run()
    assert smc.betas[-1] == 1.0 and np.isfinite(smc.logZ)
    assert np.all(np.isfinite(np.asarray(q.cpu() if hasattr(q, "cpu") else q)))
