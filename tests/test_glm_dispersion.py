"""The GLM families with a free dispersion (glm.DispersionGLM, csrc/kernels_glm.hip: FAM = 3, 4 of k_glm<NT, FAM, true>).
theta is the log-dispersion, a_i observation weights, o_i offsets, eta_i = x_i . w + o_i:

    gaussian     U_i = a_i [ 0.5 tau (y_i - eta_i)^2 + theta ],                                  tau = exp(-2 theta)
    negbinomial  U_i = a_i [ lgamma(phi) - lgamma(y_i + phi) - phi theta - y_i eta_i + (y_i + phi) logaddexp(eta_i, theta) ]
    U = sum_i U_i + 0.5 sum_d lam_d (w_d - mu_d)^2 + 0.5 lam_theta (theta - m_theta)^2           phi = exp(theta)

sampled: theta is the last component of the state and has the last entry of lam / mu; held: theta is a constant, the
state is w alone and the theta prior is absent.

The oracle side is the user-source mechanism of test_glm_model.py, `orc.pot_custom(complete_source(SOURCE), Dt, prm)`,
with this file's own C++ statement of the model: prm = [M, family, sampled, held theta, X.ravel(), a, y, o, lam(Dt),
mu(Dt)]; it carries its own psi (recurrence up to 10, eight series terms) and skips rows of weight 0 by a branch.

Tolerance: that file's `rel` / `check` with TOL = 1e-10 relative to max(1, max|oracle|); reject masks are compared for
equality under its `decisive` preconditions (asserted on the oracle's values).  Step sizes and seeds of the sampling
tests were chosen on the CPU from the oracle alone, so that the reject fraction lies in [0.1, 0.9] and no accept test is
closer than 1e-8.  The data keeps theta in [-1.5, 2.5], negative-binomial counts below 200 and |eta| < 6.

Shapes: the negative binomial's kernel at a padded state dimension of 128 is not shipped (it cannot be built without
scratch), so its largest state dimension is 64 (D = 63 sampled, D = 64 held); the Gaussian goes to 128.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from test_glm_model import N_EVAL, check, decisive, device_eval, padded, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOURCE = """
PBBI_FN T dg_psi(T x) {
    T a = 0;
    while (x < T(10)) { a -= T(1) / x; x += T(1); }
    const T r = T(1) / x, r2 = r * r;
    return a + log(x) - T(0.5) * r
           - r2 * (T(1) / 12 - r2 * (T(1) / 120 - r2 * (T(1) / 252 - r2 * (T(1) / 240 - r2 * (T(1) / 132
           - r2 * (T(691) / 32760 - r2 * (T(1) / 12 - r2 * (T(3617) / 8160))))))));
}
PBBI_FN T dg_softplus(T z) { return (z > 0 ? z : T(0)) + log1p(exp(-fabs(z))); }
PBBI_FN T dg_sigmoid(T z) { return z >= 0 ? T(1) / (T(1) + exp(-z)) : exp(z) / (T(1) + exp(z)); }
template <class Q>
PBBI_FN T potential(const Q& q, int DT, const T* prm) {
    const int M = (int)prm[0], fam = (int)prm[1], smp = (int)prm[2];
    const int D = DT - smp;
    const T* X = prm + 4;
    const T* a = X + (long)M * D;
    const T* y = a + M;
    const T* o = y + M;
    const T* lam = o + M;
    const T* mu = lam + DT;
    const T th = smp ? q[D] : prm[3];
    const T phi = exp(th), tau = exp(-2 * th);
    T s = 0;
    for (int i = 0; i < M; ++i) {
        if (a[i] == 0) continue;                // weight 0: the row is not there
        T z = o[i];
        for (int j = 0; j < D; ++j) z += X[i * D + j] * q[j];
        if (fam == 0) {
            s += a[i] * (T(0.5) * tau * (y[i] - z) * (y[i] - z) + th);
        } else {
            const T lae = (z > th ? z : th) + log1p(exp(-fabs(z - th)));
            s += a[i] * (lgamma(phi) - lgamma(y[i] + phi) - phi * th - y[i] * z + (y[i] + phi) * lae);
        }
    }
    T r = 0;
    for (int j = 0; j < DT; ++j) r += lam[j] * (q[j] - mu[j]) * (q[j] - mu[j]);
    return s + T(0.5) * r;
}
template <class Q, class G>
PBBI_FN void gradient(const Q& q, G& g, int DT, const T* prm) {
    const int M = (int)prm[0], fam = (int)prm[1], smp = (int)prm[2];
    const int D = DT - smp;
    const T* X = prm + 4;
    const T* a = X + (long)M * D;
    const T* y = a + M;
    const T* o = y + M;
    const T* lam = o + M;
    const T* mu = lam + DT;
    const T th = smp ? q[D] : prm[3];
    const T phi = exp(th), tau = exp(-2 * th);
    const T psi_phi = fam == 0 ? T(0) : dg_psi(phi);
    for (int j = 0; j < DT; ++j) g[j] = lam[j] * (q[j] - mu[j]);
    T gt = 0;
    for (int i = 0; i < M; ++i) {
        if (a[i] == 0) continue;
        T z = o[i];
        for (int j = 0; j < D; ++j) z += X[i * D + j] * q[j];
        T w;
        if (fam == 0) {
            w = -a[i] * tau * (y[i] - z);
            gt += a[i] * (T(1) - tau * (y[i] - z) * (y[i] - z));
        } else {
            const T sg = dg_sigmoid(z - th);
            w = a[i] * ((y[i] + phi) * sg - y[i]);
            gt += a[i] * phi * (psi_phi - dg_psi(y[i] + phi) + dg_softplus(z - th) + y[i] * (T(1) - sg) / phi - sg);
        }
        for (int j = 0; j < D; ++j) g[j] += w * X[i * D + j];
    }
    if (smp) g[D] += gt;
}
"""
FAM_ID = {"gaussian": 0, "negbinomial": 1}
THETA_PRIOR = (0.3, 0.25)


def problem(family, M, D, seed):
    """The data of every GPU test: weights from {0, 0.5, 1, 3} with at least one 0 (M > 1), offsets ~ N(0, 0.3), lam_d
    from {0, 0.5, 4} with lam_0 = 0, mu_d ~ N(0, 0.5), a true theta in [-0.5, 1.5]; negative-binomial counts from the
    gamma-Poisson mixture, cut at 200.  Returns the keyword arguments of DispersionGLM (without the dispersion mode),
    the true (w, theta) and the generator."""
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
    if family == "gaussian":
        y = eta + np.exp(theta) * rs.standard_normal(M)
    else:
        phi = np.exp(theta)
        y = np.minimum(rs.poisson(rs.gamma(phi, np.exp(eta) / phi)), 200).astype(np.float64)
    lam = rs.choice([0.0, 0.5, 4.0], size=D)
    lam[0] = 0.0
    mu = 0.5 * rs.standard_normal(D)
    return dict(X=X, y=y, family=family, weights=a, offset=o, prior_precision=lam, prior_mean=mu), w, theta, rs


def start(w, theta, N, rs, spread=0.3, sampled=True):
    """(Dt, N) states around (w, theta); theta stays in [-1.5, 2.5]."""
    q = w[:, None] + spread * rs.standard_normal((w.size, N))
    if sampled:
        q = np.vstack([q, np.clip(theta + spread * rs.standard_normal((1, N)), -1.5, 2.5)])
    return np.ascontiguousarray(q)


def make(P, kw, sampled, theta=None):
    if sampled:
        return P.DispersionGLM(dispersion="sample", log_dispersion_prior=THETA_PRIOR, **kw)
    return P.DispersionGLM(dispersion=float(np.exp(theta)), **kw)


def oracle_pot(kw, sampled, theta=None, keep=None, theta_prior=THETA_PRIOR):
    """The oracle's potential of the data `kw`; held: at log-dispersion theta; keep = a row mask."""
    from physicsbasedbayesianinference_amd import custom
    X, y, a, o = kw["X"], kw["y"], kw["weights"], kw["offset"]
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
    prm = np.concatenate([[float(X.shape[0]), float(FAM_ID[kw["family"]]), float(sampled), th], X.ravel(), a, y, o, lam, mu])
    return orc.pot_custom(custom.complete_source(SOURCE), D + int(sampled), prm)


# ------------------------------------------------------------------------------------------------ CPU
def test_dispersion_abi_declared_bound_and_exported():
    names = {"pbbi_potential_create_glm_dispersion", "pbbi_glm_pack_observations_dispersion"}
    hdr = open(os.path.join(ROOT, "include", "pbbi.h")).read()
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
    assert re.search(r"PBBI_GLM_GAUSSIAN\s*=\s*3\b", hdr) and re.search(r"PBBI_GLM_NEGBINOMIAL\s*=\s*4\b", hdr)
    import physicsbasedbayesianinference_amd as pkg
    from physicsbasedbayesianinference_amd import _lib, glm
    assert pkg.DispersionGLM is glm.DispersionGLM and "DispersionGLM" in pkg.__all__
    assert pkg.pack_observations_dispersion is glm.pack_observations_dispersion
    assert "pack_observations_dispersion" in pkg.__all__
    assert (_lib.GLM_GAUSSIAN, _lib.GLM_NEGBINOMIAL) == (3, 4)
    assert names <= set(_lib.PROTOTYPES)
    assert sorted(glm.FAMILIES) == ["logistic", "poisson"]         # GLM keeps accepting exactly what it accepts
    lib = _lib.load()
    assert lib.pbbi_version() == 103
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert names <= set(re.findall(r"\bT (pbbi_[a-z0-9_]+)", out))


@pytest.mark.parametrize("family", ["gaussian", "negbinomial"])
@pytest.mark.parametrize("M", [1, 16, 203])
def test_pack_observations_dispersion_matches_numpy(M, family):
    from physicsbasedbayesianinference_amd import glm
    kw, _, _, rs = problem(family, M, 3, 100 * M + len(family))
    y, a, o = kw["y"], kw["weights"], kw["offset"]
    length = ((M + 15) // 16 + 3) // 4 * 4 * 16
    out = glm.pack_observations_dispersion(y, family, weights=a, offset=o)
    assert out.shape == (3, length)
    assert np.array_equal(out[0, :M], a) and np.array_equal(out[1, :M], y) and np.array_equal(out[2, :M], o)   # d = y, raw
    assert not out[:, M:].any()
    out = glm.pack_observations_dispersion(y, family)                 # the defaults: weights 1, offset 0
    assert out.shape == (3, length)
    assert np.array_equal(out[0, :M], np.ones(M)) and np.array_equal(out[1, :M], y) and not out[2].any()
    assert not out[:, M:].any()
    # the helper refuses what the constructor refuses
    for bad in (dict(weights=-np.ones(M)), dict(weights=np.full(M, np.nan)), dict(offset=np.full(M, np.inf)),
                dict(weights=np.ones(M + 1)), dict(offset=np.zeros((M, 1)))):
        with pytest.raises(ValueError):
            glm.pack_observations_dispersion(y, family, **bad)
    with pytest.raises(ValueError):
        glm.pack_observations_dispersion(np.where(np.arange(M) == 0, np.nan, y), family)
    with pytest.raises(ValueError):
        glm.pack_observations_dispersion(y, "poisson")
    with pytest.raises(ValueError):
        glm.pack_observations_dispersion(np.abs(y) + 0.5, "negbinomial")
    with pytest.raises(ValueError):
        glm.pack_observations_dispersion(-np.abs(y) - 1.0, "negbinomial")


def test_dispersion_rejects_bad_arguments_on_the_host():
    from physicsbasedbayesianinference_amd import GLM, DispersionGLM
    rs = np.random.RandomState(0)
    M, D = 10, 3
    X = rs.standard_normal((M, D))
    yc = rs.poisson(2.0, M).astype(float)
    yr = rs.standard_normal(M)
    ones, at2 = np.ones(M), np.arange(M) == 2
    nb, ga = dict(X=X, y=yc, family="negbinomial"), dict(X=X, y=yr, family="gaussian")
    bad = [
        dict(nb, X=X[:9]), dict(nb, X=X.ravel()), dict(ga, y=yr.reshape(M, 1)),                    # shapes
        dict(nb, weights=ones[:9]), dict(nb, weights=ones.reshape(1, M)), dict(ga, offset=np.zeros(M + 1)),
        dict(ga, offset=0.0), dict(nb, prior_precision=np.ones(D + 1)), dict(nb, prior_precision=np.ones((D, 1))),
        dict(ga, prior_mean=np.zeros(D - 1)), dict(ga, prior_mean=0.0), dict(nb, log_dispersion_prior=(0.0,)),
        dict(nb, log_dispersion_prior=0.25),
        dict(ga, X=np.where(np.arange(D) == 1, np.nan, X)), dict(ga, y=np.where(at2, np.inf, yr)),  # finite values
        dict(nb, weights=np.where(at2, np.nan, ones)), dict(nb, weights=np.where(at2, np.inf, ones)),
        dict(ga, offset=np.where(at2, np.nan, 0.0)), dict(ga, offset=np.where(at2, -np.inf, 0.0)),
        dict(nb, prior_precision=np.array([1.0, np.nan, 1.0])), dict(nb, prior_precision=np.inf),
        dict(nb, prior_mean=np.array([0.0, np.nan, 0.0])), dict(nb, log_dispersion_prior=(np.nan, 0.25)),
        dict(nb, log_dispersion_prior=(0.0, np.inf)),
        dict(nb, weights=np.where(at2, -0.5, ones)),                                               # weights >= 0
        dict(nb, y=yc + 0.25), dict(nb, y=-yc - 1.0), dict(nb, y=yr),                              # negbinomial y: counts
        dict(nb, dispersion=0.0), dict(nb, dispersion=-1.0), dict(ga, dispersion=np.inf),          # dispersion > 0, finite
        dict(ga, dispersion=np.nan), dict(ga, dispersion="fit"), dict(ga, dispersion=None),
        dict(nb, prior_precision=-1.0), dict(nb, prior_precision=np.array([1.0, -1.0, 1.0])),      # precisions >= 0
        dict(nb, log_dispersion_prior=(0.0, -0.1)),
        dict(nb, dispersion=2.0, log_dispersion_prior=(0.0, 0.25)),                                # a prior with a held theta
        dict(ga, dispersion=0.5, log_dispersion_prior=(0.0, 0.0)),
        dict(nb, dtype="float32"), dict(ga, dtype="float32"),                                      # float64 only
        dict(nb, family="poisson"), dict(nb, family="logistic"), dict(ga, family="student"),
        # the state dimension: 128 for the Gaussian, 64 for the negative binomial, the theta row included
        dict(X=np.ones((4, 128)), y=np.zeros(4), family="gaussian"),
        dict(X=np.ones((4, 129)), y=np.zeros(4), family="gaussian", dispersion=1.0),
        dict(X=np.ones((4, 64)), y=np.zeros(4), family="negbinomial"),
        dict(X=np.ones((4, 65)), y=np.zeros(4), family="negbinomial", dispersion=1.0),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            DispersionGLM(**kw)
        print("refused:", sorted(set(kw) - {"X", "y"}))
    with pytest.raises(ValueError, match="64"):
        DispersionGLM(X=np.ones((4, 64)), y=np.zeros(4), family="negbinomial")
    for family in ("negbinomial", "gaussian"):          # GLM goes on refusing the families it does not serve
        with pytest.raises(ValueError):
            GLM(X, yc, family=family)


def _scipy_terms(kw, q, sampled, theta):
    """U and the likelihood part of it, from the SciPy expressions of the model."""
    from scipy.special import gammaln
    X, y, a, o = kw["X"], kw["y"], kw["weights"], kw["offset"]
    D = X.shape[1]
    th = q[D] if sampled else theta
    eta = X @ q[:D] + o
    if kw["family"] == "gaussian":
        Ui = a * (0.5 * np.exp(-2 * th) * (y - eta) ** 2 + th)
    else:
        phi = np.exp(th)
        Ui = a * (gammaln(phi) - gammaln(y + phi) - phi * th - y * eta + (y + phi) * np.logaddexp(eta, th))
    U = Ui.sum() + 0.5 * np.sum(kw["prior_precision"] * (q[:D] - kw["prior_mean"]) ** 2)
    if sampled:
        U += 0.5 * THETA_PRIOR[1] * (th - THETA_PRIOR[0]) ** 2
    return U


@pytest.mark.parametrize("family", ["gaussian", "negbinomial"])
@pytest.mark.parametrize("sampled", [True, False])
def test_dispersion_oracle_source_is_pinned(family, sampled):
    """The yardstick, not the feature: the oracle's U equals the SciPy expressions (gammaln, logaddexp) within 1e-12
    relative and its gradient central differences within 1e-6, at M = 40, D = 5."""
    M, D, N = 40, 5, 12
    kw, w, theta, rs = problem(family, M, D, 5)
    q = start(w, theta, N, rs, sampled=sampled)
    op = oracle_pot(kw, sampled, theta)
    U, g = orc.potential(op, q, want_grad=True)
    Us = np.array([_scipy_terms(kw, q[:, n], sampled, theta) for n in range(N)])
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


@pytest.mark.parametrize("D", [3, 4, 5, 6, 15, 16])
def test_pack_design_zero_column_hides_theta(D):
    """A NumPy replay of the first product on the image the handle keeps, pack_design([X | 0]): the theta row D sits in
    lane group g = D & 3 at K-step s = D >> 2, meets a zero column, and eta = X w whatever theta is."""
    from physicsbasedbayesianinference_amd import glm
    M = 37
    rs = np.random.RandomState(D)
    X = rs.standard_normal((M, D))
    Dt = D + 1
    DP = glm.padded_dim(Dt)
    img = glm.pack_design(np.hstack([X, np.zeros((M, 1))]))
    assert img.shape == (4, 2, DP * 16)
    nb, KS = (M + 15) // 16, DP // 4
    lane = np.arange(64)
    g, c = lane >> 4, lane & 15
    s_t, g_t = D >> 2, D & 3
    assert 4 * s_t + g_t == D and s_t < KS
    etas = []
    for theta in (-1.5, 0.7, 2.5):
        w = rs.standard_normal(Dt) if theta == -1.5 else w
        w[D] = theta
        # the state as the kernel holds it: element s of a lane is row 4 s + g (16 chains: all the same vector here)
        qreg = np.zeros((KS, 64))
        for s in range(KS):
            rows = 4 * s + g
            qreg[s] = np.where(rows < Dt, w[np.minimum(rows, Dt - 1)], 0.0)
        # theta as the kernel reads it: the owner lanes contribute q[s_t], the others 0, summed over the four groups
        contrib = np.where(g == g_t, qreg[s_t], 0.0)
        assert np.array_equal(contrib.reshape(4, 16).sum(axis=0), np.full(16, theta))
        eta = np.zeros((M,))
        for b in range(nb):
            P1 = img[b, 0].reshape(KS // 2, 64, 2)
            acc = np.zeros((16, 16))                       # [observation][chain]
            for s in range(KS):
                A = P1[s // 2, :, s % 2]                   # A[i = lane & 15][k = lane >> 4]
                for ln in range(64):
                    acc[c[ln], :] += A[ln] * qreg[s, (g[ln] << 4) + np.arange(16)]
                if s == s_t:                               # theta's K-step: its column of the image is zero
                    assert not A[g == g_t].any()
            n = min(16, M - 16 * b)
            eta[16 * b:16 * b + n] = acc[:n, 0]
        etas.append(eta)
        assert np.allclose(eta, X @ w[:D], rtol=0, atol=1e-12)
    assert np.array_equal(etas[0], etas[1]) and np.array_equal(etas[0], etas[2])


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


N_DISP = 100   # six full wave tiles and one of 4 chains; the second workgroup has one ghost wave

# (M, D): theta in each of the four lane groups (D = 4 .. 7), in the last row of a tile (15), alone in the second tile
# (16), at the DP = 64 / 128 boundary (63, 64) and in the last row of the largest kernel (127); M = 1, a ragged last
# block, several chunks
EVAL_SHAPES = [(1, 4), (40, 5), (40, 6), (40, 7), (203, 15), (203, 16), (1000, 63), (1000, 64), (203, 127)]
EVAL_CASES = [(f, s, M, D) for f in ("gaussian", "negbinomial") for s in (True, False) for (M, D) in EVAL_SHAPES
              if D + int(s) <= (128 if f == "gaussian" else 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("family,sampled,M,D", EVAL_CASES)
def test_dispersion_eval_matches_oracle(P, lib, family, sampled, M, D):
    kw, w, theta, rs = problem(family, M, D, 7 * M + D)
    assert M == 1 or (kw["weights"] == 0).any()
    pot, op = make(P, kw, sampled, theta), oracle_pot(kw, sampled, theta)
    assert pot.numDimensions == D + int(sampled)
    q = start(w, theta, N_DISP, rs, sampled=sampled)
    Uo, go = orc.potential(op, q, want_grad=True)
    U, g = device_eval(lib, pot, q)
    check(f"U {family} {M}x{D}", U, Uo)
    check(f"grad {family} {M}x{D}", g, go)
    if sampled:
        check("theta row", g[D], go[D])
    check("call", pot(q), Uo)                           # the class API (ldn == N)
    check("gradient", pot.gradient(q), go)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["gaussian", "negbinomial"])
@pytest.mark.parametrize("M,D", [(40, 5), (203, 15), (203, 16)])
def test_dispersion_held_equals_sampled(P, lib, family, M, D):
    """Device against device: at theta = theta0 the held model is the sampled one without its theta prior and row."""
    kw, w, theta0, rs = problem(family, M, D, 3 * M + D)
    q = start(w, theta0, N_DISP, rs, sampled=False)
    held, smp = make(P, kw, False, theta0), make(P, kw, True)
    th = float(np.log(np.exp(theta0)))                  # the held model's theta: log of the dispersion it was given
    Uh, gh = device_eval(lib, held, q)
    Us, gs = device_eval(lib, smp, np.ascontiguousarray(np.vstack([q, np.full((1, N_DISP), th)])))
    check("U", Uh, Us - 0.5 * THETA_PRIOR[1] * (th - THETA_PRIOR[0]) ** 2)
    check("grad", gh, gs[:D])


@pytest.mark.gpu
def test_dispersion_gaussian_equals_linear_regression(P, lib):
    """Through existing code: gaussian, held sigma, no weights -- energy differences and the gradient are those of
    linear_regression_posterior(X, y - o, sigma^2) on the dense kernels (its constant differs)."""
    M, D, sigma = 203, 16, 0.7
    kw, w, _, rs = problem("gaussian", M, D, 17)
    kw["weights"] = None
    pot = P.DispersionGLM(dispersion=sigma, **kw)
    ref = P.linear_regression_posterior(kw["X"], kw["y"] - kw["offset"], sigma ** 2, prior_precision=kw["prior_precision"],
                                        prior_mean=kw["prior_mean"])
    q = start(w, 0.0, N_DISP, rs, sampled=False)
    U, g = device_eval(lib, pot, q)
    Ur, gr = device_eval(lib, ref, q)
    check("U differences", U[1:] - U[0], Ur[1:] - Ur[0])
    check("grad", g, gr)


@pytest.mark.gpu
@pytest.mark.parametrize("sampled", [True, False])
def test_dispersion_zero_weight_under_overflow(P, lib, sampled):
    """negbinomial: a weight-0 row with eta = 800, and a weight-0 row in the ragged last block, are not there."""
    M, D = 33, 3
    kw, w, theta, rs = problem("negbinomial", M, D, 9)
    q = start(w, theta, N_DISP, rs, spread=0.01, sampled=sampled)
    hot, last = 5, M - 1
    kw["X"][hot] = 800.0 * w / (w @ w)
    kw["weights"][[hot, last]] = 0.0
    kw["weights"][[hot + 1, last - 1]] = 3.0
    eta = kw["X"] @ q[:D] + kw["offset"][:, None]
    assert np.all(np.abs(eta[hot] - 800.0) < 30.0)
    keep = np.ones(M, bool)
    keep[[hot, last]] = False
    Uo, go = orc.potential(oracle_pot(kw, sampled, theta, keep), q, want_grad=True)
    U, g = device_eval(lib, make(P, kw, sampled, theta), q)
    assert np.all(np.isfinite(U)) and np.all(np.isfinite(g))
    check("U", U, Uo)
    check("grad", g, go)


# family, M, D, h (Leapfrog), h (Stormer-Verlet), L -- N = 303, theta sampled; both h from the oracle alone (see the
# module text): at each the reject fraction lies in [0.1, 0.9] for all four combinations of mass and kT
ITER_CASES = [("gaussian", 40, 5, 0.2, 0.12, 8), ("gaussian", 203, 16, 0.08, 0.06, 8),
              ("negbinomial", 40, 5, 0.6, 0.3, 8), ("negbinomial", 203, 16, 0.32, 0.12, 8)]


def iter_inputs(family, M, D, mass, kt):
    kw, w, theta, rs = problem(family, M, D, 11)
    N = 303
    kT = 2.0 if kt else 1.0
    m = 1.0 + (np.arange(N) % 3) * 0.5 if mass else None
    q = start(w, theta, N, rs, spread=0.1)
    p = np.ascontiguousarray(rs.standard_normal((D + 1, N)) * np.sqrt((m if mass else 1.0) * kT))
    u = rs.uniform(size=N)
    return kw, N, kT, m, q, p, u


@pytest.mark.gpu
@pytest.mark.parametrize("family,M,D,h_lf,h_sv,L", ITER_CASES)
@pytest.mark.parametrize("method", ["Leapfrog", "Stormer-Verlet"])
@pytest.mark.parametrize("mass", [False, True])
@pytest.mark.parametrize("kt", [False, True])
def test_dispersion_uploaded_draw_iteration_matches_oracle(P, lib, family, M, D, h_lf, h_sv, L, method, mass, kt):
    import torch
    h = h_lf if method == "Leapfrog" else h_sv
    d = _dev()
    kw, N, kT, m, q, p, u = iter_inputs(family, M, D, mass, kt)
    Dt = D + 1
    pot, op = make(P, kw, True), oracle_pot(kw, True)
    qd, pd, ud = (d.as_device(a, 0, np.float64) for a in (q, p, u))
    md = d.as_device(m, 0, np.float64) if mass else None
    qo, po = d.empty((Dt, N), np.float64, 0), d.empty((Dt, N), np.float64, 0)
    ratio, rej = d.empty((N,), np.float64, 0), d.empty((N,), np.uint8, 0)
    mi = 0 if method == "Leapfrog" else 1
    args = [pot.handle, mi, qd.data_ptr(), pd.data_ptr(), ud.data_ptr(), md.data_ptr() if mass else None, qo.data_ptr(),
            po.data_ptr(), ratio.data_ptr(), rej.data_ptr(), N, N, h, L]
    flags = lib.COMPAT_P_FROM_OLDQ | lib.BETA_ACCEPT
    if kt:
        lib.call("pbbi_hmc_iter_kt", *args, flags, kT, d.stream_ptr(0))
    else:
        lib.call("pbbi_hmc_iter", *args, flags, d.stream_ptr(0))
    torch.cuda.synchronize()
    r_o, rej_o = orc.hmc_iter(op, method, q, p, u, m, h, L, beta=1.0 / kT)
    decisive(r_o, u, rej_o, 0.1, 0.9)
    grej = d.to_numpy(rej).astype(bool)
    print("mask mismatches", int((grej != rej_o).sum()), "ratio err", rel(d.to_numpy(ratio), r_o))
    assert np.array_equal(grej, rej_o)
    check("q", d.to_numpy(qo), q)
    check("p", d.to_numpy(po), p)
    check("ratio", d.to_numpy(ratio), r_o)


# family, sampled, M, D, N, h, L -- S = 6
RUN_CASES = [("gaussian", True, 203, 16, 300, 0.08, 8), ("negbinomial", True, 203, 16, 300, 0.3, 8),
             ("negbinomial", False, 40, 5, 300, 0.5, 8), ("gaussian", True, 203, 127, 100, 0.08, 6)]
RUN_SEED, RUN_ITER0, RUN_CHAIN0, RUN_S = 17, 3, 1000003, 6


@pytest.mark.gpu
@pytest.mark.parametrize("family,sampled,M,D,N,h,L", RUN_CASES)
def test_dispersion_philox_run_matches_oracle(P, lib, family, sampled, M, D, N, h, L):
    """pbbi_hmc_run, PBBI_DRAW_F64: the oracle draws its own momenta of the (Dt, N) state (no device draw is replayed)."""
    import torch
    d = _dev()
    kw, w, theta, rs = problem(family, M, D, 21)
    q = start(w, theta, N, rs, spread=0.1, sampled=sampled)
    pot = make(P, kw, sampled, theta)
    Dt, S = D + int(sampled), RUN_S
    ldn = N + 5
    qd = padded(q, ldn)
    samples, momenta = d.empty((S, Dt, N), np.float64, 0), d.empty((S, Dt, N), np.float64, 0)
    rej, ratio = d.empty((S, N), np.uint8, 0), d.empty((S, N), np.float64, 0)
    flags = lib.COMPAT_P_FROM_OLDQ | lib.DRAW_F64
    lib.call("pbbi_hmc_run", pot.handle, 0, qd.data_ptr(), None, samples.data_ptr(), momenta.data_ptr(), rej.data_ptr(),
             ratio.data_ptr(), N, ldn, h, L, S, flags, RUN_SEED, RUN_ITER0, RUN_CHAIN0, 1.0, d.stream_ptr(0))
    torch.cuda.synchronize()
    so, mo, rejo, ro = orc.hmc_run_philox(oracle_pot(kw, sampled, theta), "Leapfrog", q, None, h, L, S, RUN_SEED, RUN_ITER0,
                                          RUN_CHAIN0, 1.0, compat=orc.COMPAT_P_FROM_OLDQ | orc.DRAW_F64)
    u = np.stack([orc.philox_uniform(RUN_SEED, RUN_ITER0 + i, RUN_CHAIN0, N) for i in range(S)])
    assert np.all(np.isfinite(so)) and np.all(np.isfinite(mo))
    decisive(ro, u, rejo, 0.1, 0.9)
    assert np.array_equal(d.to_numpy(rej).astype(bool), rejo)
    check("samples", d.to_numpy(samples), so)
    check("momenta", d.to_numpy(momenta), mo)
    check("ratio", d.to_numpy(ratio), ro)
    check("final state", qd[:, :N].cpu().numpy(), q)
    assert np.all(qd[:, N:].cpu().numpy() == 1e300), "stores past N"


@pytest.mark.gpu
@pytest.mark.parametrize("family,sampled,method", [("gaussian", True, 0), ("negbinomial", True, 1), ("negbinomial", False, 0)])
def test_dispersion_run_equals_runs_of_one_bit_for_bit(P, lib, family, sampled, method):
    import torch
    d = _dev()
    M, D, h = (203, 16, 0.06) if family == "gaussian" else (203, 16, 0.15)
    kw, w, theta, rs = problem(family, M, D, 31)
    pot = make(P, kw, sampled, theta)
    Dt = D + int(sampled)
    N, L, S, seed, chain0, iter0 = 333, 4, 7, 8, 5, 2
    m = 1.0 + (np.arange(N) % 3) * 0.5
    md = d.as_device(m, 0, np.float64)
    st = d.stream_ptr(0)
    q0 = start(w, theta, N, rs, spread=0.1, sampled=sampled)

    def run(s_per_call):
        qd = d.as_device(q0, 0, np.float64)
        samples, momenta = d.empty((S, Dt, N), np.float64, 0), d.empty((S, Dt, N), np.float64, 0)
        reject, ratio = d.empty((S, N), np.uint8, 0), d.empty((S, N), np.float64, 0)
        for i in range(0, S, s_per_call):
            lib.call("pbbi_hmc_run", pot.handle, method, qd.data_ptr(), md.data_ptr(), samples[i].data_ptr(),
                     momenta[i].data_ptr(), reject[i].data_ptr(), ratio[i].data_ptr(), N, N, h, L,
                     min(s_per_call, S - i), lib.COMPAT_P_FROM_OLDQ, seed, iter0 + i, chain0, 1.0, st)
        torch.cuda.synchronize()
        return tuple(d.to_numpy(a) for a in (samples, momenta, reject, ratio, qd))

    one, each = run(S), run(1)
    for a, b in zip(one, each):
        assert np.array_equal(a, b)
    assert np.all(np.isfinite(one[0])) and 0.0 < one[2].mean() < 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["gaussian", "negbinomial"])
def test_dispersion_integrators_match_oracle(P, family):
    """Leapfrog / StormerVerlet(...).integrate() of the class API, theta sampled, with per-chain masses."""
    M, D, N, h, L = 203, 5, N_EVAL, 0.02, 7
    kw, w, theta, rs = problem(family, M, D, 51)
    pot, op = make(P, kw, True), oracle_pot(kw, True)
    Dt = D + 1
    m = 1.0 + (np.arange(N) % 3) * 0.5
    for cls, method in ((P.Leapfrog, "Leapfrog"), (P.StormerVerlet, "Stormer-Verlet")):
        q, p = start(w, theta, N, rs, spread=0.1), np.ascontiguousarray(rs.standard_normal((Dt, N)))
        ens = P.Ensemble(Dt, N)
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


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["gaussian", "negbinomial"])
def test_dispersion_through_the_classes(P, lib, family):
    """HMC.getSamples in both rng modes, sampleStats, TemperedSMC and pbbi_describe_run take a DispersionGLM; split
    returns the coefficients and exp(theta); GIST refuses it as it refuses GLM."""
    from scipy.constants import k as kB
    from physicsbasedbayesianinference_amd.smc import TemperedSMC
    M, D, N, S = 203, 5, 200, 4
    kw, w, theta, rs = problem(family, M, D, 71)
    pot, held = make(P, kw, True), make(P, kw, False, theta)
    assert pot.numDimensions == D + 1 and held.numDimensions == D and pot.sampled and not held.sampled
    assert pot.log_dispersion_prior == THETA_PRIOR and held.log_dispersion_prior is None
    for rng in ("philox", "numpy"):
        np.random.seed(5)
        hmc = P.HMC(P.Ensemble(D + 1, N), 0.4, 0.05, None, potential=pot, rng=rng, seed=13, verbose=False)
        s, m = hmc.getSamples(S, 1 / kB, 0.3)
        s, m = np.asarray(s), np.asarray(m)
        assert s.shape == (D + 1, N, S) and np.all(np.isfinite(s)) and np.all(np.isfinite(m))
        coef, disp = pot.split(s)
        assert coef.shape == (D, N, S) and disp.shape == (N, S)
        assert np.array_equal(coef, s[:D]) and np.array_equal(disp, np.exp(s[D])) and np.all(disp > 0)
    sh, _ = P.HMC(P.Ensemble(D, N), 0.4, 0.05, None, potential=held, rng="philox", seed=13, verbose=False).getSamples(S, 1 / kB, 0.3)
    coef, disp = held.split(np.asarray(sh))
    assert coef.shape == (D, N, S) and disp == pytest.approx(np.exp(theta), rel=1e-15)
    stats = P.HMC(P.Ensemble(D + 1, N), 0.4, 0.05, None, potential=pot, rng="philox", seed=13,
                  verbose=False).sampleStats(8, 4, 1 / kB, 0.3, burn_in=2, max_lag=2)
    mean, var = stats.moments()[:2]
    mean, var = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (mean, var))
    assert mean.shape[0] == D + 1 and np.all(np.isfinite(mean)) and np.all(np.isfinite(var))
    errs = []
    plain = P.GLM(kw["X"], np.minimum(np.abs(np.floor(kw["y"])), 1.0))
    for target, dim in ((pot, D + 1), (plain, D)):
        with pytest.raises(lib.PbbiError) as e:
            P.HMC(P.Ensemble(dim, 64), 0.8, 0.1, None, potential=target, rng="philox", seed=13,
                  verbose=False).getSamplesGIST(2, 1 / kB, 1.0)
        errs.append((e.value.code, str(e.value)))
    assert errs[0] == errs[1] and errs[0][0] == lib.ERR_UNSUPPORTED
    smc = TemperedSMC(pot, D + 1, 2048, 0.5, 0.2, 0.05, seed=3)
    q = smc.run()
    assert smc.betas[-1] == 1.0 and np.isfinite(smc.logZ)
    assert np.all(np.isfinite(np.asarray(q.cpu() if hasattr(q, "cpu") else q)))
    buf = C.create_string_buffer(1024)
    lib.call("pbbi_describe_run", pot.handle, 0, 64, 64, 4, 2, lib.COMPAT_P_FROM_OLDQ, buf, 1024)
    text = buf.value.decode()
    print(text)
    assert "k_glm" in text and family in text and "sampled" in text and "iterations per launch: up to 1" in text
    lib.call("pbbi_describe_run", held.handle, 0, 64, 64, 4, 2, lib.COMPAT_P_FROM_OLDQ, buf, 1024)
    assert family in buf.value.decode() and "held" in buf.value.decode()


@pytest.mark.gpu
def test_dispersion_gaussian_known_answer(P):
    """Linear regression with unknown noise under flat priors in w and theta (p(sigma) proportional to 1 / sigma): E[w] is
    the least-squares solution and sigma^2 is scaled inverse-chi-square, E[theta] = 0.5 [log(RSS / 2) - psi((M - D) / 2)].
    4096 independent chains from dispersed starts, step size from adaptStepSize, 300 iterations of L = 10 of burn-in; the
    mean over the chains of the final state matches both within 5 standard errors (sd over the chains / sqrt(N))."""
    from scipy.constants import k as kB
    from scipy.special import digamma
    M, D, N = 40, 3, 4096
    rs = np.random.RandomState(123)
    X = rs.standard_normal((M, D))
    y = X @ np.array([0.5, -1.0, 0.25]) + 0.6 * rs.standard_normal(M)
    pot = P.DispersionGLM(X, y, family="gaussian", dispersion="sample", log_dispersion_prior=(0.0, 0.0), prior_precision=0.0)
    w_ls = np.linalg.lstsq(X, y, rcond=None)[0]
    rss = float(np.sum((y - X @ w_ls) ** 2))
    theta_exact = 0.5 * (np.log(rss / 2.0) - digamma((M - D) / 2.0))
    # dispersed: the starts are N(0, 0.2^2), twice the posterior's standard deviations (0.07 .. 0.12) wide and five to ten of
    # them away from its mean.  (A NumPy replay of this sampler shows that a cloud of 0.5 leaves the chains that start with
    # sigma far below their residuals stuck -- one fixed step size, every proposal rejected -- whatever computes U.)
    q_std = 0.2
    warm = P.HMC(P.Ensemble(D + 1, N), 0.5, 0.05, None, potential=pot, rng="philox", seed=2024, verbose=False)
    h = warm.adaptStepSize(1 / kB, q_std)
    assert 1e-3 < h < 1.0, h
    hmc = P.HMC(P.Ensemble(D + 1, N), 10.5 * h, h, None, potential=pot, rng="philox", seed=2024, verbose=False)
    assert hmc.integrator.numSteps == 10
    s, _ = hmc.getSamples(1, 1 / kB, q_std, burn_in=300)
    last = np.asarray(s)[:, :, 0]
    mean, se = last.mean(axis=1), last.std(axis=1, ddof=1) / np.sqrt(N)
    exact = np.r_[w_ls, theta_exact]
    print("step", h, "accept", hmc.acceptRate, "mean", mean, "exact", exact, "deviation / se", (mean - exact) / se)
    assert np.all(np.isfinite(last))
    assert np.all(np.abs(mean - exact) <= 5.0 * se)
