"""The Gamma family of glm.DispersionGLM (family="gamma", PBBI_GLM_GAMMA = 5 of k_glm<NT, FAM, true>), the part that needs no
GPU: the header and the library, the packer, the constructors' refusals, and the yardstick the GPU tests of test_glm_gamma.py
are held to.  theta = log(alpha) is the log-dispersion, alpha the shape, mu_i = exp(eta_i), Var = mu^2 / alpha:

    U_i = a_i [ lgamma(alpha) - alpha log alpha + alpha (eta_i + y_i exp(-eta_i)) - alpha log y_i ]        eta_i = x_i . w + o_i
    U   = sum_i U_i + 0.5 sum_d lam_d (w_d - mu_d)^2 + 0.5 lam_theta (theta - m_theta)^2      (theta prior only when sampled)

so that log p(y_i | .) = -U_i / a_i - log y_i.  The kernels form it from z_i = eta_i - log y_i, with log y taken once on the
host; the oracle side below states it in the NATURAL form above, from y itself.

The oracle side is the user-source mechanism of test_glm_model.py, `orc.pot_custom(complete_source(SOURCE), Dt, prm)`, with
this file's own C++ statement of the model: prm = [M, sampled, held theta, X.ravel(), a, y, o, lam(Dt), mu(Dt)]; it carries
its own psi (recurrence up to 10, eight series terms) and skips rows of weight 0 by a branch.

The data: weights from {0, 0.5, 1, 3} with at least one 0, offsets ~ N(0, 0.3), theta in [-0.5, 1.5], y drawn from the model
and clipped so that |eta_i - log y_i| < 8 at the truth.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from test_glm_dispersion import THETA_PRIOR, start  # noqa: F401  (start: (Dt, N) states around (w, theta))
from test_glm_model import rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_DIM = 128     # the state dimension glm_max_dim(GLM_V_DISPERSION, PBBI_GLM_GAMMA) states: the Gaussian's

SOURCE = """
PBBI_FN T gm_psi(T x) {
    T a = 0;
    while (x < T(10)) { a -= T(1) / x; x += T(1); }
    const T r = T(1) / x, r2 = r * r;
    return a + log(x) - T(0.5) * r
           - r2 * (T(1) / 12 - r2 * (T(1) / 120 - r2 * (T(1) / 252 - r2 * (T(1) / 240 - r2 * (T(1) / 132
           - r2 * (T(691) / 32760 - r2 * (T(1) / 12 - r2 * (T(3617) / 8160))))))));
}
template <class Q>
PBBI_FN T potential(const Q& q, int DT, const T* prm) {
    const int M = (int)prm[0], smp = (int)prm[1];
    const int D = DT - smp;
    const T* X = prm + 3;
    const T* a = X + (long)M * D;
    const T* y = a + M;
    const T* o = y + M;
    const T* lam = o + M;
    const T* mu = lam + DT;
    const T th = smp ? q[D] : prm[2];
    const T alpha = exp(th);
    T s = 0;
    for (int i = 0; i < M; ++i) {
        if (a[i] == 0) continue;                // weight 0: the row is not there
        T e = o[i];
        for (int j = 0; j < D; ++j) e += X[i * D + j] * q[j];
        s += a[i] * (lgamma(alpha) - alpha * log(alpha) + alpha * (e + y[i] * exp(-e)) - alpha * log(y[i]));
    }
    T r = 0;
    for (int j = 0; j < DT; ++j) r += lam[j] * (q[j] - mu[j]) * (q[j] - mu[j]);
    return s + T(0.5) * r;
}
template <class Q, class G>
PBBI_FN void gradient(const Q& q, G& g, int DT, const T* prm) {
    const int M = (int)prm[0], smp = (int)prm[1];
    const int D = DT - smp;
    const T* X = prm + 3;
    const T* a = X + (long)M * D;
    const T* y = a + M;
    const T* o = y + M;
    const T* lam = o + M;
    const T* mu = lam + DT;
    const T th = smp ? q[D] : prm[2];
    const T alpha = exp(th);
    const T psi_alpha = gm_psi(alpha);
    for (int j = 0; j < DT; ++j) g[j] = lam[j] * (q[j] - mu[j]);
    T gt = 0;
    for (int i = 0; i < M; ++i) {
        if (a[i] == 0) continue;
        T e = o[i];
        for (int j = 0; j < D; ++j) e += X[i * D + j] * q[j];
        const T ye = y[i] * exp(-e);
        const T w = a[i] * alpha * (T(1) - ye);
        gt += a[i] * alpha * (psi_alpha - log(alpha) - T(1) + e + ye - log(y[i]));
        for (int j = 0; j < D; ++j) g[j] += w * X[i * D + j];
    }
    if (smp) g[D] += gt;
}
"""


def problem(M, D, seed):
    """The data of every Gamma test: weights from {0, 0.5, 1, 3} with at least one 0 (M > 1), offsets ~ N(0, 0.3), lam_d from
    {0, 0.5, 4} with lam_0 = 0, mu_d ~ N(0, 0.5), a true theta in [-0.5, 1.5], y from Gamma(alpha, scale mu / alpha) clipped to
    |eta - log y| < 8.  Returns the keyword arguments of DispersionGLM (without the dispersion mode), the true (w, theta) and
    the generator."""
    rs = np.random.RandomState(seed)
    X = rs.standard_normal((M, D)) / np.sqrt(D)
    w = 0.7 * rs.standard_normal(D)
    theta = rs.uniform(-0.5, 1.5)
    a = rs.choice([0.0, 0.5, 1.0, 3.0], size=M)
    if M > 1:
        a[rs.randint(M)] = 0.0
    else:
        a[:] = 3.0
    o = 0.3 * rs.standard_normal(M)
    eta = X @ w + o
    alpha = np.exp(theta)
    y = np.clip(rs.gamma(alpha, np.exp(eta) / alpha), np.exp(eta - 7.9), np.exp(eta + 7.9))
    assert np.all(y > 0) and np.all(np.abs(eta - np.log(y)) < 8.0)
    lam = rs.choice([0.0, 0.5, 4.0], size=D)
    lam[0] = 0.0
    mu = 0.5 * rs.standard_normal(D)
    return dict(X=X, y=y, family="gamma", weights=a, offset=o, prior_precision=lam, prior_mean=mu), w, theta, rs


def make(P, kw, sampled, theta=None):
    if sampled:
        return P.DispersionGLM(dispersion="sample", log_dispersion_prior=THETA_PRIOR, **kw)
    return P.DispersionGLM(dispersion=float(np.exp(theta)), **kw)


def oracle_pot(kw, sampled, theta=None, keep=None, theta_prior=THETA_PRIOR):
    """The oracle's potential of the data `kw`; held: at log-dispersion theta; keep = a row mask."""
    from physicsbasedbayesianinference_amd import custom
    X, y, a, o = kw["X"], kw["y"], kw.get("weights"), kw.get("offset")
    M, D = X.shape
    a = np.ones(M) if a is None else a
    o = np.zeros(M) if o is None else o
    if keep is not None:
        X, y, a, o = X[keep], y[keep], a[keep], o[keep]
    lam = np.broadcast_to(np.asarray(kw["prior_precision"], float), (D,))
    mu = np.zeros(D) if kw.get("prior_mean") is None else kw["prior_mean"]
    if sampled:
        lam, mu = np.r_[lam, theta_prior[1]], np.r_[mu, theta_prior[0]]
    th = 0.0 if sampled else float(np.log(np.exp(theta)))    # the class takes exp(theta) and the library its logarithm
    prm = np.concatenate([[float(X.shape[0]), float(sampled), th], X.ravel(), a, y, o, lam, mu])
    return orc.pot_custom(custom.complete_source(SOURCE), D + int(sampled), prm)


# ------------------------------------------------------------------------------------------------ 1: header and library
def test_gamma_header_and_library():
    hdr = open(os.path.join(ROOT, "include", "pbbi.h")).read()
    assert re.search(r"PBBI_GLM_GAMMA\s*=\s*5\b", hdr)
    assert re.search(r"PBBI_GLM_GAUSSIAN\s*=\s*3\b", hdr) and re.search(r"PBBI_GLM_NEGBINOMIAL\s*=\s*4\b", hdr)
    from physicsbasedbayesianinference_amd import _lib, glm
    assert _lib.GLM_GAMMA == 5
    assert glm.DISPERSION_FAMILIES["gamma"] == 5 and sorted(glm.DISPERSION_FAMILIES) == ["gamma", "gaussian", "negbinomial"]
    assert glm.DISPERSION_MAX_DIM["gamma"] == MAX_DIM
    assert sorted(glm.FAMILIES) == ["logistic", "poisson"]         # GLM keeps accepting exactly what it accepts
    assert sorted(glm.HIER_DISP_MAX_DIM) == ["gaussian", "negbinomial"]
    lib = _lib.load()
    assert lib.pbbi_version() == 103
    # no new export: the family goes through the entries the dispersion families have
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (pbbi_[a-z0-9_]+)", out))
    assert {"pbbi_potential_create_glm_dispersion", "pbbi_glm_pack_observations_dispersion"} <= exported
    assert not [n for n in exported if "gamma" in n]
    for par in (_lib.HIER_CENTRED, _lib.HIER_NONCENTRED):          # random effects for Gamma are not built
        assert lib.pbbi_glm_hier_dispersion_max_dim(_lib.GLM_GAMMA, par) == 0
        assert lib.pbbi_glm_hier_dispersion_max_dim(_lib.GLM_GAUSSIAN, par) == 64


# ------------------------------------------------------------------------------------------------ 2: packing
@pytest.mark.parametrize("M", [1, 16, 203])
def test_gamma_pack_observations(M):
    from physicsbasedbayesianinference_amd import _lib, glm
    kw, _, _, rs = problem(M, 3, 100 * M + 5)
    y, a, o = kw["y"], kw["weights"], kw["offset"]
    length = ((M + 15) // 16 + 3) // 4 * 4 * 16
    out = glm.pack_observations_dispersion(y, "gamma", weights=a, offset=o)
    assert out.shape == (3, length) == glm.pack_observations_dispersion(y, "gaussian", weights=a, offset=o).shape
    assert np.array_equal(out[0, :M], a) and np.array_equal(out[2, :M], o)
    assert np.all(np.abs(out[1, :M] - np.log(y)) <= np.spacing(np.abs(np.log(y))))      # d = log y, to the last place
    assert not out[:, M:].any()
    out = glm.pack_observations_dispersion(y, "gamma")                 # the defaults: weights 1, offset 0
    assert out.shape == (3, length)
    assert np.array_equal(out[0, :M], np.ones(M)) and not out[2].any() and not out[:, M:].any()
    assert np.all(np.abs(out[1, :M] - np.log(y)) <= np.spacing(np.abs(np.log(y))))
    # the helper refuses what the constructor refuses
    last = np.arange(M) == M - 1
    for bad in (0.0, -1.0, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            glm.pack_observations_dispersion(np.where(last, bad, y), "gamma")
    for bad in (dict(weights=-np.ones(M)), dict(offset=np.full(M, np.inf)), dict(weights=np.ones(M + 1))):
        with pytest.raises(ValueError):
            glm.pack_observations_dispersion(y, "gamma", **bad)
    # ... and the C entry says which rule and which observation
    lib = _lib.load()
    n = C.c_int64()
    buf = np.empty(3 * length)
    ptr = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    assert lib.pbbi_glm_pack_observations_dispersion(M, 5, ptr(y), None, None, ptr(buf), buf.size, C.byref(n)) == _lib.OK
    assert n.value == 3 * length and np.array_equal(buf.reshape(3, -1), out)
    for bad, text in ((0.0, "gamma: y must be > 0"), (-2.5, "gamma: y must be > 0"), (np.nan, "y must be finite"),
                      (np.inf, "y must be finite")):
        yb = np.ascontiguousarray(np.where(last, bad, y))
        rc = lib.pbbi_glm_pack_observations_dispersion(M, 5, ptr(yb), None, None, ptr(buf), buf.size, C.byref(n))
        assert rc == _lib.ERR_INVALID
        assert _lib.last_error().endswith("%s (observation %d)" % (text, M - 1)), _lib.last_error()
    rc = lib.pbbi_glm_pack_observations_dispersion(M, 7, ptr(y), None, None, ptr(buf), buf.size, C.byref(n))
    assert rc == _lib.ERR_INVALID and "unknown dispersion family (gaussian = 3, negbinomial = 4)" in _lib.last_error()


# ------------------------------------------------------------------------------------------------ 3: constructors
def test_gamma_constructor_refuses_on_the_host():
    from physicsbasedbayesianinference_amd import GLM, DispersionGLM, HierarchicalDispersionGLM, _lib
    rs = np.random.RandomState(0)
    M, D = 10, 3
    X = rs.standard_normal((M, D))
    y = rs.gamma(2.0, 1.0, M)
    at2 = np.arange(M) == 2
    ga = dict(X=X, y=y, family="gamma")
    bad = [dict(ga, y=np.where(at2, 0.0, y)), dict(ga, y=np.where(at2, -1.0, y)), dict(ga, y=-y),      # y > 0
           dict(ga, y=np.where(at2, np.nan, y)), dict(ga, y=np.where(at2, np.inf, y)),                # ... and finite
           dict(ga, weights=np.where(at2, -0.5, 1.0)), dict(ga, offset=np.where(at2, np.nan, 0.0)),
           dict(ga, dispersion=0.0), dict(ga, dispersion=-1.0), dict(ga, dispersion="fit"),
           dict(ga, dispersion=2.0, log_dispersion_prior=(0.0, 0.25)), dict(ga, dtype="float32"),
           dict(ga, family="student"), dict(ga, family="inverse-gaussian")]
    for kw in bad:
        with pytest.raises(ValueError):
            DispersionGLM(**kw)
    with pytest.raises(ValueError, match="gamma: y must be > 0"):
        DispersionGLM(**dict(ga, y=np.where(at2, 0.0, y)))
    # a state dimension one above the cap, the theta row included
    with pytest.raises(ValueError, match=str(MAX_DIM)):
        DispersionGLM(X=np.ones((4, MAX_DIM)), y=np.ones(4), family="gamma")
    with pytest.raises(ValueError, match=str(MAX_DIM)):
        DispersionGLM(X=np.ones((4, MAX_DIM + 1)), y=np.ones(4), family="gamma", dispersion=1.0)
    # random effects, and the canonical model's class, do not serve the family: a ValueError that says so
    with pytest.raises(ValueError, match="gamma"):
        HierarchicalDispersionGLM(X, y, family="gamma", groups=np.array([-1, 0, 0]))
    with pytest.raises(ValueError):
        GLM(X, y, family="gamma")
    # the C entries, before anything is allocated: the dimension rule of _glm_dispersion, UNSUPPORTED from _glm_hier_dispersion
    lib = _lib.load()
    ptr = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    handle = C.c_void_p()
    wide, ones = np.ones((4, MAX_DIM)), np.ones(4)
    lam = np.ones(MAX_DIM + 1)
    rc = lib.pbbi_potential_create_glm_dispersion(MAX_DIM, 4, ptr(wide), ptr(ones), 5, None, None, ptr(lam), None, 1, 0.0,
                                                  _lib.F64, 0, C.byref(handle))
    assert rc == _lib.ERR_UNSUPPORTED and not handle.value and str(MAX_DIM) in _lib.last_error()
    yb = np.ascontiguousarray(np.where(at2, 0.0, y))
    rc = lib.pbbi_potential_create_glm_dispersion(D, M, ptr(X), ptr(yb), 5, None, None, ptr(lam), None, 1, 0.0, _lib.F64, 0,
                                                  C.byref(handle))
    assert rc == _lib.ERR_INVALID and not handle.value and "gamma: y must be > 0 (observation 2)" in _lib.last_error()
    groups = np.array([-1, 0, 0], dtype=np.int32)
    tp, dp = np.array([0.0, 1.0]), np.array([0.0, 0.25])
    rc = lib.pbbi_potential_create_glm_hier_dispersion(D, M, ptr(X), ptr(y), 5, None, None, ptr(lam), None,
                                                       groups.ctypes.data_as(C.POINTER(C.c_int32)), 1, ptr(tp), _lib.HIER_CENTRED,
                                                       1, 0.0, ptr(dp), _lib.F64, 0, C.byref(handle))
    assert rc == _lib.ERR_UNSUPPORTED and not handle.value and "gamma" in _lib.last_error()


# ------------------------------------------------------------------------------------------------ 4: the yardstick
def scipy_U(kw, q, sampled, theta):
    """U from scipy.stats.gamma.logpdf: -sum a_i logpdf(y_i; alpha, scale = mu_i / alpha) - sum a_i log y_i + the priors."""
    from scipy import stats
    X, y, a, o = kw["X"], kw["y"], kw["weights"], kw["offset"]
    D = X.shape[1]
    th = q[D] if sampled else theta
    alpha, mu = np.exp(th), np.exp(X @ q[:D] + o)
    U = -np.sum(a * stats.gamma.logpdf(y, alpha, scale=mu / alpha)) - np.sum(a * np.log(y))
    U += 0.5 * np.sum(kw["prior_precision"] * (q[:D] - kw["prior_mean"]) ** 2)
    if sampled:
        U += 0.5 * THETA_PRIOR[1] * (th - THETA_PRIOR[0]) ** 2
    return U


@pytest.mark.parametrize("sampled", [True, False])
def test_gamma_oracle_source_is_pinned(sampled):
    """The yardstick, not the feature: the oracle's U equals the SciPy density within 1e-12 relative and its gradient central
    differences within 1e-6, at M = 40, D = 5."""
    M, D, N = 40, 5, 12
    kw, w, theta, rs = problem(M, D, 5)
    q = start(w, theta, N, rs, sampled=sampled)
    op = oracle_pot(kw, sampled, theta)
    U, g = orc.potential(op, q, want_grad=True)
    Us = np.array([scipy_U(kw, q[:, n], sampled, theta) for n in range(N)])
    e = float(np.max(np.abs(U - Us) / np.maximum(1.0, np.abs(Us))))
    print("U against SciPy", e)
    assert e <= 1e-12
    h = 1e-5
    fd = np.empty_like(g)
    for j in range(q.shape[0]):
        qp, qm = q.copy(), q.copy()
        qp[j] += h
        qm[j] -= h
        fd[j] = (orc.potential(op, qp) - orc.potential(op, qm)) / (2 * h)
    e = rel(g, fd)
    print("gradient against central differences", e)
    assert e <= 1e-6
    assert g.shape[0] == D + int(sampled)


def test_gamma_pointwise_constant_is_minus_a_log_y():
    """log p(y_i | .) = -U_i / a_i - log y_i: pointwise_constants("gamma", ...) is -a_i log y_i, 0 on a row of weight 0."""
    from scipy import stats
    from scipy.special import gammaln
    from physicsbasedbayesianinference_amd import glm
    kw, w, theta, _ = problem(40, 5, 5)
    y, a = kw["y"], kw["weights"]
    k = glm.pointwise_constants("gamma", y, a)
    assert np.array_equal(k, -a * np.log(y)) and np.any(a == 0.0) and np.all(k[a == 0.0] == 0.0)
    assert np.array_equal(glm.pointwise_constants("gamma", y), -np.log(y))
    eta, alpha = kw["X"] @ w + kw["offset"], np.exp(theta)
    z = eta - np.log(y)
    Ui = a * (gammaln(alpha) - alpha * theta + alpha * (z + np.exp(-z)))
    full = a * stats.gamma.logpdf(y, alpha, scale=np.exp(eta) / alpha)
    assert np.max(np.abs((k - Ui) - full) / np.maximum(1.0, np.abs(full))) <= 1e-12
