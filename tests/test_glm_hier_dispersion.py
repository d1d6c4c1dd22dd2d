"""Random effects for the dispersion families (glm.HierarchicalDispersionGLM, csrc/kernels_glm.hip: k_glm<NT, FAM, true, HIER>
with FAM = 3, 4 and HIER = GLM_HIER_CENTRED / GLM_HIER_NC): the likelihood of DispersionGLM under the priors of HierarchicalGLM,
eta_i = x_i . w + o_i, weights a_i >= 0, theta the log-dispersion:

    gaussian     U_i = a_i [ 0.5 exp(-2 theta) (y_i - eta_i)^2 + theta ]
    negbinomial  U_i = a_i [ lgamma(phi) - lgamma(y_i + phi) - phi theta - y_i eta_i + (y_i + phi) logaddexp(eta_i, theta) ]
    centred:     U = sum_i U_i + 0.5 sum_{d fixed} lam_d (w_d - mu_d)^2
                   + sum_j [ 0.5 exp(-2 t_j) S_j + n_j t_j + 0.5 lam_tj (t_j - m_tj)^2 ] + 0.5 lam_theta (theta - m_theta)^2
    noncentred:  grouped rows hold z_d, w_d = mu_d + exp(t_j) z_d;  U_nc(z, t, theta) = U_c(w(z, t), t, theta) - sum_j n_j t_j

State: rows 0 .. D-1 the coefficients, rows D .. D+J-1 the t_j, row D+J theta when it is sampled (the theta prior only then).

The oracle side is `orc.pot_custom(complete_source(SOURCE), DT, prm)` with this file's own C++ statement of the model, both
parametrisations: prm = [M, D, J, family, sampled, held theta, noncentred, X.ravel(), a, y, o, lam(DT), mu(DT), groups(D)].  It
carries its own psi (recurrence up to 10, eight series terms, as test_glm_dispersion.py does) and skips rows of weight 0 by a
branch.  It is pinned below against a NumPy / SciPy statement (gammaln, digamma) and, non-centred against centred, through the
change of variables.

Tolerance: `check` / `rel` of test_glm_model.py, TOL = 1e-10 relative to max(1, max|oracle|).  Reject masks are compared for
equality under that file's `decisive` preconditions, asserted on the ORACLE's values: reject fraction within [0.1, 0.9] and no
accept test closer than 1e-8.  Those are conditions, not measurements: the step sizes and seeds of ITER_CASES and RUN_CASES were
chosen on the CPU from the oracle alone so that they hold (reject fractions over the eight combinations of integrator, mass
and kT at N = 303, and of the S = 3 runs, are listed beside the tables).

Data: the recipe of test_glm_dispersion.problem plus test_glm_hier.problem -- weights from {0, 0.5, 1, 3} with at least one 0
(M > 1), offsets ~ N(0, 0.3), lam_d from {0, 0.5, 4} with lam_0 = 0, mu_d ~ N(0, 0.5), groups from {-1, 0 .. J-1} with every
value present, log-scale priors all different with one flat.  theta stays in [-1.5, 2.5], every t_j in [-2, 2], |eta| < 6
(asserted at w(z, t)), negative-binomial counts are cut at 200.

Shapes: all twelve kernels (NT = 1, 2, 4; both families; both parametrisations) build without scratch, so
glm.HIER_DISP_MAX_DIM is 64 throughout and the negative binomial runs every shape the Gaussian does.
"""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from test_glm_dispersion import THETA_PRIOR
from test_glm_hier import t_priors
from test_glm_model import check, decisive, device_eval, padded, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOURCE = """
PBBI_FN T hd_psi(T x) {
    T a = 0;
    while (x < T(10)) { a -= T(1) / x; x += T(1); }
    const T r = T(1) / x, r2 = r * r;
    return a + log(x) - T(0.5) * r
           - r2 * (T(1) / 12 - r2 * (T(1) / 120 - r2 * (T(1) / 252 - r2 * (T(1) / 240 - r2 * (T(1) / 132
           - r2 * (T(691) / 32760 - r2 * (T(1) / 12 - r2 * (T(3617) / 8160))))))));
}
PBBI_FN T hd_softplus(T z) { return (z > 0 ? z : T(0)) + log1p(exp(-fabs(z))); }
PBBI_FN T hd_sigmoid(T z) { return z >= 0 ? T(1) / (T(1) + exp(-z)) : exp(z) / (T(1) + exp(z)); }
// w_j of the state q: a fixed row holds it; a grouped row holds it (centred) or z_j (non-centred)
template <class Q>
PBBI_FN T hd_coef(const Q& q, int j, int nc, const T* mu, const T* grp, const T* sig) {
    const int k = (int)grp[j];
    return (nc && k >= 0) ? mu[j] + sig[k] * q[j] : q[j];
}
template <class Q>
PBBI_FN T potential(const Q& q, int DT, const T* prm) {
    const int M = (int)prm[0], D = (int)prm[1], J = (int)prm[2], fam = (int)prm[3], smp = (int)prm[4], nc = (int)prm[6];
    const T* X = prm + 7;
    const T* a = X + (long)M * D;
    const T* y = a + M;
    const T* o = y + M;
    const T* lam = o + M;
    const T* mu = lam + DT;
    const T* grp = mu + DT;
    T sig[4] = {1, 1, 1, 1}, tau[4] = {1, 1, 1, 1};
    for (int k = 0; k < J; ++k) { sig[k] = exp(q[D + k]); tau[k] = exp(-2 * q[D + k]); }
    const T th = smp ? q[D + J] : prm[5];
    const T phi = exp(th), tth = exp(-2 * th);
    T s = 0;
    for (int i = 0; i < M; ++i) {
        if (a[i] == 0) continue;                // weight 0: the row is not there
        T z = o[i];
        for (int j = 0; j < D; ++j) z += X[i * D + j] * hd_coef(q, j, nc, mu, grp, sig);
        if (fam == 0) {
            s += a[i] * (T(0.5) * tth * (y[i] - z) * (y[i] - z) + th);
        } else {
            const T lae = (z > th ? z : th) + log1p(exp(-fabs(z - th)));
            s += a[i] * (lgamma(phi) - lgamma(y[i] + phi) - phi * th - y[i] * z + (y[i] + phi) * lae);
        }
    }
    T r = 0;
    for (int j = 0; j < D; ++j) {
        const int k = (int)grp[j];
        const T e = q[j] - mu[j];
        if (k < 0) {
            r += lam[j] * e * e;
        } else if (nc) {
            r += q[j] * q[j];                   // z ~ N(0, 1): mu is the mean of w and has no part here
        } else {
            r += tau[k] * e * e;
            s += q[D + k];                      // n_j t_j, one t_j per member
        }
    }
    for (int j = D; j < DT; ++j) r += lam[j] * (q[j] - mu[j]) * (q[j] - mu[j]);      // the t rows and the theta row
    return s + T(0.5) * r;
}
template <class Q, class G>
PBBI_FN void gradient(const Q& q, G& g, int DT, const T* prm) {
    const int M = (int)prm[0], D = (int)prm[1], J = (int)prm[2], fam = (int)prm[3], smp = (int)prm[4], nc = (int)prm[6];
    const T* X = prm + 7;
    const T* a = X + (long)M * D;
    const T* y = a + M;
    const T* o = y + M;
    const T* lam = o + M;
    const T* mu = lam + DT;
    const T* grp = mu + DT;
    T sig[4] = {1, 1, 1, 1}, tau[4] = {1, 1, 1, 1};
    for (int k = 0; k < J; ++k) { sig[k] = exp(q[D + k]); tau[k] = exp(-2 * q[D + k]); }
    const T th = smp ? q[D + J] : prm[5];
    const T phi = exp(th), tth = exp(-2 * th);
    const T psi_phi = fam == 0 ? T(0) : hd_psi(phi);
    for (int j = 0; j < D; ++j) g[j] = 0;       // gL = dL/dw first
    T gt = 0;
    for (int i = 0; i < M; ++i) {
        if (a[i] == 0) continue;
        T z = o[i];
        for (int j = 0; j < D; ++j) z += X[i * D + j] * hd_coef(q, j, nc, mu, grp, sig);
        T w;
        if (fam == 0) {
            w = -a[i] * tth * (y[i] - z);
            gt += a[i] * (T(1) - tth * (y[i] - z) * (y[i] - z));
        } else {
            const T sg = hd_sigmoid(z - th);
            w = a[i] * ((y[i] + phi) * sg - y[i]);
            gt += a[i] * phi * (psi_phi - hd_psi(y[i] + phi) + hd_softplus(z - th) + y[i] * (T(1) - sg) / phi - sg);
        }
        for (int j = 0; j < D; ++j) g[j] += w * X[i * D + j];
    }
    for (int j = D; j < DT; ++j) g[j] = lam[j] * (q[j] - mu[j]);
    if (smp) g[D + J] += gt;
    for (int j = 0; j < D; ++j) {
        const int k = (int)grp[j];
        const T e = q[j] - mu[j];
        if (k < 0) {
            g[j] += lam[j] * e;
        } else if (nc) {
            g[D + k] += sig[k] * g[j] * q[j];
            g[j] = sig[k] * g[j] + q[j];
        } else {
            g[D + k] += T(1) - tau[k] * e * e;
            g[j] += tau[k] * e;
        }
    }
}
"""
FAMILY = ("gaussian", "negbinomial")
FAM_ID = {"gaussian": 0, "negbinomial": 1}
PARAMS = ("centred", "noncentred")
N_HD = 100     # six full wave tiles and one of 4 chains; the second workgroup has one ghost wave


def problem(family, M, D, J, seed):
    """The data of every test (the module text has the recipe).  Returns the keyword arguments of HierarchicalDispersionGLM
    without the dispersion mode and the parametrisation, the true (w, t, theta) and the generator."""
    rs = np.random.RandomState(seed)
    X = rs.standard_normal((M, D)) / np.sqrt(D)
    w = 0.7 * rs.standard_normal(D)
    t = rs.uniform(-0.5, 0.5, size=J)
    theta = rs.uniform(-0.5, 1.5)
    a = rs.choice([0.0, 0.5, 1.0, 3.0], size=M)
    if M > 1:
        a[rs.randint(M)] = 0.0
    else:
        a[:] = 3.0
    o = 0.3 * rs.standard_normal(M)
    eta = X @ w + o
    assert np.all(np.abs(eta) < 6.0)
    if family == "gaussian":
        y = eta + np.exp(theta) * rs.standard_normal(M)
    else:
        phi = np.exp(theta)
        y = np.minimum(rs.poisson(rs.gamma(phi, np.exp(eta) / phi)), 200).astype(np.float64)
    lam = rs.choice([0.0, 0.5, 4.0], size=D)
    lam[0] = 0.0
    mu = 0.5 * rs.standard_normal(D)
    assert D >= J + 1
    groups = rs.randint(-1, J, size=D)
    groups[rs.permutation(D)[:J + 1]] = np.arange(-1, J)
    assert set(groups) == set(range(-1, J))
    kw = dict(X=X, y=y, family=family, groups=groups, log_scale_prior=t_priors(J), weights=a, offset=o, prior_precision=lam,
              prior_mean=mu)
    return kw, w, t, theta, rs


def hostpot(kw, parametrisation, sampled):
    """A HierarchicalDispersionGLM with the attributes of `kw` and no device: what to_natural / from_natural / split read."""
    from physicsbasedbayesianinference_amd import HierarchicalDispersionGLM as H
    fake = H.__new__(H)
    groups = np.asarray(kw["groups"])
    fake.numCoefficients, fake.numGroups = groups.size, int(groups.max()) + 1
    fake.groups = groups.astype(np.int32)
    fake.prior_mean = np.zeros(groups.size) if kw.get("prior_mean") is None else np.asarray(kw["prior_mean"], float)
    fake.parametrisation = parametrisation
    fake.sampled = bool(sampled)
    fake.dispersion = "sample" if sampled else 1.7
    return fake


def natural_start(kw, w, t, theta, N, rs, spread, sampled):
    """(D + J + sampled, N) states around (w; t; theta) in NATURAL coordinates, within the data bounds of the module text."""
    q = w[:, None] + spread * rs.standard_normal((w.size, N))
    tq = np.clip(t[:, None] + spread * rs.standard_normal((t.size, N)), -2.0, 2.0)
    rows = [q, tq]
    if sampled:
        rows.append(np.clip(theta + spread * rs.standard_normal((1, N)), -1.5, 2.5))
    qc = np.ascontiguousarray(np.vstack(rows))
    assert np.all(np.abs(kw["X"] @ qc[:w.size] + kw["offset"][:, None]) < 6.0)
    return qc


def start(kw, par, w, t, theta, N, rs, spread=0.3, sampled=True):
    """... in SAMPLER coordinates: z on the grouped rows of a non-centred potential (from_natural)."""
    qc = natural_start(kw, w, t, theta, N, rs, spread, sampled)
    return np.ascontiguousarray(hostpot(kw, par, sampled).from_natural(qc))


def model_params(kw, par, sampled, theta=None):
    """prm of SOURCE and the state dimension."""
    X, y, a, o = kw["X"], kw["y"], kw["weights"], kw["offset"]
    M, D = X.shape
    a = np.ones(M) if a is None else a
    o = np.zeros(M) if o is None else o
    groups = np.asarray(kw["groups"])
    J = int(groups.max()) + 1
    tp = np.broadcast_to(np.asarray(kw["log_scale_prior"], float), (J, 2))
    lam = np.r_[np.broadcast_to(np.asarray(kw["prior_precision"], float), (D,)), tp[:, 1]]
    mu = np.r_[np.zeros(D) if kw.get("prior_mean") is None else kw["prior_mean"], tp[:, 0]]
    if sampled:
        lam, mu = np.r_[lam, THETA_PRIOR[1]], np.r_[mu, THETA_PRIOR[0]]
    th = 0.0 if sampled else float(np.log(np.exp(theta)))     # the class takes exp(theta) and the library its logarithm
    head = [float(M), float(D), float(J), float(FAM_ID[kw["family"]]), float(sampled), th, float(par == "noncentred")]
    return np.concatenate([head, X.ravel(), a, y, o, lam, mu, groups.astype(float)]), D + J + int(sampled)


def oracle_pot(kw, par, sampled, theta=None):
    from physicsbasedbayesianinference_amd import custom
    prm, DT = model_params(kw, par, sampled, theta)
    return orc.pot_custom(custom.complete_source(SOURCE), DT, prm)


def make(P, kw, par, sampled, theta=None):
    if sampled:
        return P.HierarchicalDispersionGLM(dispersion="sample", log_dispersion_prior=THETA_PRIOR, parametrisation=par, **kw)
    return P.HierarchicalDispersionGLM(dispersion=float(np.exp(theta)), parametrisation=par, **kw)


def members(kw):
    groups = np.asarray(kw["groups"])
    return np.array([np.sum(groups == j) for j in range(int(groups.max()) + 1)], dtype=float)


def numpy_model(kw, qc, sampled, theta):
    """(U, gradient) of the CENTRED model at one natural state qc from NumPy and SciPy (gammaln, digamma)."""
    from scipy.special import digamma, expit, gammaln
    X, y, a, o = kw["X"], kw["y"], kw["weights"], kw["offset"]
    D = X.shape[1]
    groups, tp = np.asarray(kw["groups"]), np.asarray(kw["log_scale_prior"], float)
    J = int(groups.max()) + 1
    lam, mu = kw["prior_precision"], kw["prior_mean"]
    w, t = qc[:D], qc[D:D + J]
    th = qc[D + J] if sampled else theta
    eta = X @ w + o
    if kw["family"] == "gaussian":
        tau = np.exp(-2 * th)
        Ui = a * (0.5 * tau * (y - eta) ** 2 + th)
        de = -a * tau * (y - eta)
        dth = np.sum(a * (1.0 - tau * (y - eta) ** 2))
    else:
        phi = np.exp(th)
        Ui = a * (gammaln(phi) - gammaln(y + phi) - phi * th - y * eta + (y + phi) * np.logaddexp(eta, th))
        s = expit(eta - th)
        de = a * ((y + phi) * s - y)
        dth = np.sum(a * (phi * (digamma(phi) - digamma(y + phi) + np.logaddexp(0.0, eta - th) - s) + y * (1.0 - s)))
    U = Ui.sum()
    g = np.zeros(qc.size)
    g[:D] = X.T @ de
    fixed = groups < 0
    U += 0.5 * np.sum(lam[fixed] * (w[fixed] - mu[fixed]) ** 2)
    g[:D][fixed] += lam[fixed] * (w[fixed] - mu[fixed])
    for j in range(J):
        mem = groups == j
        e = w[mem] - mu[mem]
        tau_j = np.exp(-2 * t[j])
        U += 0.5 * tau_j * np.sum(e ** 2) + mem.sum() * t[j] + 0.5 * tp[j, 1] * (t[j] - tp[j, 0]) ** 2
        g[:D][mem] += tau_j * e
        g[D + j] = mem.sum() - tau_j * np.sum(e ** 2) + tp[j, 1] * (t[j] - tp[j, 0])
    if sampled:
        U += 0.5 * THETA_PRIOR[1] * (th - THETA_PRIOR[0]) ** 2
        g[D + J] = dth + THETA_PRIOR[1] * (th - THETA_PRIOR[0])
    return U, g


def natural_np(kw, q):
    """The closed form of to_natural, written out; the theta row (and anything else past the t rows) passes through."""
    groups, mu = np.asarray(kw["groups"]), kw["prior_mean"]
    D = groups.size
    out = q.copy()
    for d in range(D):
        if groups[d] >= 0:
            out[d] = mu[d] + np.exp(q[D + groups[d]]) * q[d]
    return out


def from_centred(kw, q, Uc, gc):
    """(U, gradient) of the non-centred model at q from the centred model's at to_natural(q): the Jacobian term and the chain
    rule.  A theta row is common to both."""
    groups = np.asarray(kw["groups"])
    D, nj = groups.size, members(kw)
    J = nj.size
    U = Uc - nj @ q[D:D + J]
    g = gc.copy()
    g[D:D + J] -= nj.reshape((J,) + (1,) * (gc.ndim - 1))
    for d in range(D):
        j = groups[d]
        if j >= 0:
            e = np.exp(q[D + j])
            g[d] = e * gc[d]
            g[D + j] += gc[d] * e * q[d]
    return U, g


# M, D, J, sampled: the smallest shapes at which ownership of the t rows and the theta row can go wrong
SHAPES = [(1, 2, 1, True),                        # the smallest
          (40, 5, 2, True), (40, 5, 2, False),    # general
          (40, 11, 4, True),                      # theta is row 15, the last of a tile; J = 4: t_0 and theta share a lane group
          (203, 12, 4, True),                     # the t rows end the first tile, theta is alone in the second (DP = 32)
          (203, 14, 4, True),                     # the t rows straddle the tile boundary
          (203, 28, 3, True), (203, 29, 3, False),      # 32 rows exactly
          (1000, 59, 4, True), (1000, 60, 4, False)]    # 64 rows exactly


def shipped(family, par, D, J, sampled):
    try:
        from physicsbasedbayesianinference_amd import glm
        return D + J + int(sampled) <= glm.HIER_DISP_MAX_DIM[family][par]
    except (ImportError, AttributeError, KeyError):       # the names do not exist: the CPU tests say so
        return True


# ------------------------------------------------------------------------------------------------ CPU
NAMES = {"pbbi_potential_create_glm_hier_dispersion", "pbbi_glm_pack_prior_groups_dispersion",
         "pbbi_glm_hier_dispersion_max_dim"}


def test_hd_abi_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pbbi.h")).read()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
    import physicsbasedbayesianinference_amd as pkg
    from physicsbasedbayesianinference_amd import _lib, glm
    assert pkg.HierarchicalDispersionGLM is glm.HierarchicalDispersionGLM and "HierarchicalDispersionGLM" in pkg.__all__
    assert NAMES <= set(_lib.PROTOTYPES)
    assert len(_lib.PROTOTYPES["pbbi_potential_create_glm_hier_dispersion"]) == 19
    lib = _lib.load()
    assert lib.pbbi_version() == 103
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert NAMES <= set(re.findall(r"\bT (pbbi_[a-z0-9_]+)", out))
    sig = inspect.signature(glm.HierarchicalDispersionGLM.__init__)
    assert sig.parameters["parametrisation"].default == "centred" and sig.parameters["dispersion"].default == "sample"
    # the library states what ships, glm.HIER_DISP_MAX_DIM mirrors it
    assert sorted(glm.HIER_DISP_MAX_DIM) == ["gaussian", "negbinomial"]
    for family in FAMILY:
        assert sorted(glm.HIER_DISP_MAX_DIM[family]) == ["centred", "noncentred"]
        for par in PARAMS:
            got = lib.pbbi_glm_hier_dispersion_max_dim(glm.DISPERSION_FAMILIES[family], glm.HIER_PARAMETRISATIONS[par])
            assert got == glm.HIER_DISP_MAX_DIM[family][par], (family, par, got)
    assert glm.HIER_DISP_MAX_DIM["gaussian"] == {"centred": 64, "noncentred": 64}       # all six Gaussian kernels must ship
    for fam, par in ((0, 0), (1, 1), (3, 2), (4, -1), (2, 0)):
        assert lib.pbbi_glm_hier_dispersion_max_dim(fam, par) == 0
    # the parents keep serving exactly what they served
    assert sorted(glm.FAMILIES) == ["logistic", "poisson"] and sorted(glm.HIER_MAX_DIM) == ["logistic", "poisson"]


def test_hd_rejects_bad_arguments_on_the_host():
    from physicsbasedbayesianinference_amd import HierarchicalDispersionGLM as H, HierarchicalGLM, _lib, glm
    rs = np.random.RandomState(0)
    M, D = 10, 4
    X = rs.standard_normal((M, D))
    yc = rs.poisson(2.0, M).astype(float)
    yr = rs.standard_normal(M)
    ones, at2 = np.ones(M), np.arange(M) == 2
    g = np.array([-1, 0, 0, 1])
    ga = dict(X=X, y=yr, family="gaussian", groups=g)
    nb = dict(X=X, y=yc, family="negbinomial", groups=g, parametrisation="noncentred")
    dmax = glm.HIER_DISP_MAX_DIM
    bad = [
        # the families of HierarchicalGLM point there; unknown ones are unknown
        (dict(ga, family="logistic", y=(yc > 1).astype(float)), "HierarchicalGLM"), (dict(nb, family="poisson"), "HierarchicalGLM"),
        (dict(ga, family="student"), "family"),
        # structured group priors are not built
        (dict(ga, penalty={0: np.eye(2)}), "not built"), (dict(nb, penalty=[np.eye(2), None]), "not built"),
        (dict(ga, penalty_rank={0: 1}), "not built"),
        # the parametrisation
        (dict(ga, parametrisation="non-centered"), "parametrisation"), (dict(ga, parametrisation=1), "parametrisation"),
        (dict(ga, parametrisation=None), "parametrisation"),
        # every rule of HierarchicalGLM's prior arguments
        (dict(ga, groups=g[:3]), "groups"), (dict(ga, groups=None), "groups"), (dict(ga, groups=np.array([-2, 0, 0, 1])), "-1"),
        (dict(ga, groups=np.array([-1, 0, 0, 2])), "must be used"), (dict(ga, groups=np.array([-1, 0.5, 0, 1])), "integers"),
        (dict(ga, groups=np.full(D, -1)), "GLM"),
        (dict(ga, X=np.ones((M, 6)), groups=np.array([-1, 0, 1, 2, 3, 4])), "at most 4"),
        (dict(ga, prior_precision=-1.0), "prior_precision"), (dict(ga, prior_precision=np.ones(D + 1)), "prior_precision"),
        (dict(nb, prior_precision=np.array([np.nan, 1.0, 1.0, 1.0])), "prior_precision"),
        (dict(ga, prior_mean=np.zeros(D - 1)), "prior_mean"), (dict(nb, prior_mean=np.array([0.0, np.nan, 0.0, 0.0])), "prior_mean"),
        (dict(ga, log_scale_prior=(0.0, -0.1)), "log_scale_prior"), (dict(ga, log_scale_prior="wide"), "log_scale_prior"),
        (dict(nb, log_scale_prior=np.zeros((3, 2))), "log_scale_prior"), (dict(nb, log_scale_prior=(np.nan, 1.0)), "log_scale_prior"),
        # every rule of DispersionGLM's data and dispersion arguments
        (dict(ga, X=X[:9]), "rows"), (dict(ga, X=X.ravel()), "2-D"), (dict(ga, y=yr.reshape(M, 1)), "1-D"),
        (dict(ga, X=np.where(np.arange(D) == 1, np.nan, X)), "finite"), (dict(ga, y=np.where(at2, np.inf, yr)), "finite"),
        (dict(nb, y=yc + 0.25), "negbinomial"), (dict(nb, y=-yc - 1.0), "negbinomial"),
        (dict(nb, weights=ones[:9]), "weights"), (dict(nb, weights=np.where(at2, -0.5, ones)), "weights"),
        (dict(nb, weights=np.where(at2, np.nan, ones)), "weights"), (dict(ga, offset=np.zeros(M + 1)), "offset"),
        (dict(ga, offset=np.where(at2, np.inf, 0.0)), "offset"),
        (dict(nb, dispersion=0.0), "dispersion"), (dict(nb, dispersion=-1.0), "dispersion"), (dict(ga, dispersion=np.inf), "dispersion"),
        (dict(ga, dispersion=np.nan), "dispersion"), (dict(ga, dispersion="fit"), "dispersion"), (dict(ga, dispersion=None), "dispersion"),
        (dict(nb, log_dispersion_prior=(0.0,)), "log_dispersion_prior"), (dict(nb, log_dispersion_prior=0.25), "log_dispersion_prior"),
        (dict(nb, log_dispersion_prior=(np.nan, 0.25)), "log_dispersion_prior"),
        (dict(nb, log_dispersion_prior=(0.0, -0.1)), "log_dispersion_prior"),
        # a prior with a held dispersion
        (dict(nb, dispersion=2.0, log_dispersion_prior=(0.0, 0.25)), "held dispersion has no prior"),
        (dict(ga, dispersion=0.5, log_dispersion_prior=(0.0, 0.0)), "held dispersion has no prior"),
        # float32
        (dict(ga, dtype="float32"), "float64"), (dict(nb, dtype="float32"), "float64"),
    ]
    # D + J + sampled above HIER_DISP_MAX_DIM: one past it sampled, one past it held, for every family and parametrisation
    for family in FAMILY:
        for par in PARAMS:
            m = dmax[family][par]
            base = dict(y=np.zeros(4), family=family, parametrisation=par)
            bad.append((dict(base, X=np.ones((4, m - 1)), groups=np.arange(m - 1) % 2 - 1), "state dimension"))             # + 1 + 1
            bad.append((dict(base, X=np.ones((4, m - 3)), groups=np.arange(m - 3) % 4, dispersion=1.0), "state dimension"))  # + 4
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            H(**kw)
        print("refused:", sorted(set(kw) - {"X", "y"}), msg)
    with pytest.raises(ValueError, match="not built"):
        H.with_random_intercepts(X, yr, np.arange(M) % 3, penalty=np.eye(3))
    with pytest.raises(ValueError, match="parametrisation"):
        H.with_random_intercepts(X, yr, np.arange(M) % 3, parametrisation="nc")
    for family in FAMILY:                            # HierarchicalGLM goes on refusing the families it does not serve
        with pytest.raises(ValueError, match="family"):
            HierarchicalGLM(X, yc, family=family, groups=g)

    # the C entry points state the same rules with their codes (host only: nothing here reaches a device)
    L = _lib.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    tp = np.array([0.0, 1.0] * 4)
    h = C.c_void_p()
    ys, gi = np.zeros(4), np.ascontiguousarray(g, np.int32)
    pr = np.array([0.0, 0.25])

    def ptr(a, kind=dp):
        return None if a is None else np.ascontiguousarray(a).ctypes.data_as(kind)

    def create(Dn=4, Xn=None, y=ys, fam=3, w=None, o=None, lam=None, mu=None, groups=gi, J=2, tpr=tp, par=0, sample=1, theta=0.0,
               dprior=pr, dtype=_lib.F64):
        Xn = np.ones((4, Dn)) if Xn is None else Xn
        lam = np.ones(Dn) if lam is None else lam
        keep = [np.ascontiguousarray(v) for v in (Xn, y, lam, tpr)]     # alive across the call
        rc = L.pbbi_potential_create_glm_hier_dispersion(Dn, 4, ptr(keep[0]), ptr(keep[1]), fam, ptr(w), ptr(o), ptr(keep[2]),
                                                         ptr(mu), ptr(groups, ip), J, ptr(keep[3]), par, sample, theta,
                                                         ptr(dprior), dtype, 0, C.byref(h))
        return rc, _lib.last_error()

    INV, UNS = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    cases = [
        (dict(par=2), INV, "parametrisation"), (dict(par=-1), INV, "parametrisation"),
        (dict(fam=0), INV, "pbbi_potential_create_glm_hier"), (dict(fam=1), INV, "pbbi_potential_create_glm_hier"),
        (dict(fam=2), INV, "family"), (dict(fam=7), INV, "family"),
        (dict(J=0), UNS, "1 .. 4"), (dict(J=5), UNS, "1 .. 4"), (dict(J=3), INV, "must be used"),
        (dict(groups=np.array([-2, 0, 0, 1], np.int32)), INV, "groups"), (dict(groups=None), INV, "groups"),
        (dict(lam=np.array([-1.0, 1, 1, 1])), INV, "prior_precision"), (dict(mu=np.array([np.inf, 0, 0, 0])), INV, "prior_mean"),
        (dict(tpr=np.array([0.0, -1.0] * 4)), INV, "log_scale_prior"), (dict(tpr=np.array([np.nan, 1.0] * 4)), INV, "log_scale_prior"),
        (dict(y=np.array([0.0, np.nan, 0, 0])), INV, "y must be finite"), (dict(fam=4, y=np.array([0.0, 1.5, 0, 0])), INV, "negbinomial"),
        (dict(w=np.array([1.0, -1, 1, 1])), INV, "weights"), (dict(o=np.array([0.0, np.inf, 0, 0])), INV, "offset"),
        (dict(Xn=np.where(np.arange(16).reshape(4, 4) == 5, np.nan, 1.0)), INV, "X must be finite"),
        (dict(dprior=None), INV, "log_dispersion_prior"), (dict(dprior=np.array([0.0, -0.5])), INV, "log_dispersion_prior"),
        (dict(dprior=np.array([np.inf, 0.5])), INV, "log_dispersion_prior"),
        (dict(sample=0, theta=0.3), INV, "held one has no prior"), (dict(sample=0, theta=np.nan, dprior=None), INV, "held dispersion"),
        (dict(dtype=_lib.F32), UNS, "float64"),
    ]
    for fam, family in ((3, "gaussian"), (4, "negbinomial")):
        for par, pname in enumerate(PARAMS):
            m = dmax[family][pname]
            gb = np.r_[np.zeros(m - 2, dtype=np.int32), np.int32(1)]
            cases.append((dict(fam=fam, par=par, Dn=m - 1, groups=gb), UNS, "<= %d" % m))     # m - 1 + 2 + 1 rows
    for kwargs, code, msg in cases:
        rc, err = create(**kwargs)
        print("C refused:", sorted(kwargs), rc, err)
        assert rc == code and msg in err and not h, (kwargs, rc, err)
    # the packing entry refuses what the builder refuses
    out, n = np.empty(256), np.empty(4)
    rc = L.pbbi_glm_pack_prior_groups_dispersion(4, 2, ptr(np.ones(4)), None, ptr(gi, ip), ptr(tp), 1, None, ptr(out), ptr(n))
    assert rc == INV and "log_dispersion_prior" in _lib.last_error()
    rc = L.pbbi_glm_pack_prior_groups_dispersion(4, 2, ptr(np.ones(4)), None, ptr(gi, ip), ptr(tp), 0, ptr(pr), ptr(out), ptr(n))
    assert rc == INV and "held one has no prior" in _lib.last_error()
    rc = L.pbbi_glm_pack_prior_groups_dispersion(4, 3, ptr(np.ones(4)), None, ptr(gi, ip), ptr(tp), 1, ptr(pr), ptr(out), ptr(n))
    assert rc == INV and "must be used" in _lib.last_error()
    rc = L.pbbi_glm_pack_prior_groups_dispersion(4, 2, ptr(np.ones(4)), None, ptr(gi, ip), ptr(tp), 1, ptr(pr), None, ptr(n))
    assert rc == INV
    for kw in (dict(dispersion=2.0, log_dispersion_prior=(0.0, 1.0)), dict(log_dispersion_prior=(0.0, -1.0)),
               dict(log_scale_prior=(0.0, -1.0)), dict(prior_precision=-1.0)):
        with pytest.raises(ValueError):
            glm.pack_prior_groups_dispersion(g, **kw)


@pytest.mark.parametrize("D,J,sampled", sorted({s[1:] for s in SHAPES} | {(3, 1, True), (15, 1, True), (15, 1, False), (13, 2, True)}))
def test_hd_pack_prior_groups_dispersion_matches_numpy(D, J, sampled):
    from physicsbasedbayesianinference_amd import glm
    rs = np.random.RandomState(13 * D + J + int(sampled))
    groups = rs.randint(-1, J, size=D)
    groups[rs.permutation(D)[:J + 1]] = np.arange(-1, J)
    lam, mu, tp = rs.choice([0.0, 0.5, 4.0], size=D), rs.standard_normal(D), t_priors(J)
    DT = D + J + int(sampled)
    DP = glm.padded_dim(DT)
    disp = dict(dispersion="sample", log_dispersion_prior=THETA_PRIOR) if sampled else dict(dispersion=0.8)
    table, nj = glm.pack_prior_groups_dispersion(groups, tp, lam, mu, **disp)
    assert table.shape == (2, DP) and nj.shape == (J,)
    fixed = groups < 0
    assert np.array_equal(table[0, :D][fixed], lam[fixed])                               # a fixed row: its own precision
    assert np.array_equal(table[0, :D][~fixed], -(groups[~fixed] + 1.0))                 # a member of group j: -(j + 1)
    assert np.array_equal(table[1, :D], mu)
    assert np.array_equal(table[0, D:D + J], tp[:, 1]) and np.array_equal(table[1, D:D + J], tp[:, 0])      # the t rows
    if sampled:
        assert table[0, D + J] == THETA_PRIOR[1] and table[1, D + J] == THETA_PRIOR[0]   # the theta row, a FIXED row
        assert table[0, D + J] >= 0.0
    assert not table[:, DT:].any()                                                       # zeros past D + J + sampled
    assert np.array_equal(nj, [np.sum(groups == j) for j in range(J)])
    # rows 0 .. D+J-1 are the parent's table
    ptab, pn = glm.pack_prior_groups(groups, tp, lam, mu)
    assert np.array_equal(ptab[:, :D + J], table[:, :D + J]) and np.array_equal(pn, nj)
    # the defaults of the class: theta's prior (0, 0.25)
    if sampled:
        table, _ = glm.pack_prior_groups_dispersion(groups, tp, lam, mu)
        assert table[0, D + J] == 0.25 and table[1, D + J] == 0.0


@pytest.mark.parametrize("family", FAMILY)
@pytest.mark.parametrize("sampled", [True, False])
def test_hd_oracle_source_is_pinned(family, sampled):
    """The yardstick, not the feature: SOURCE (centred) against the NumPy / SciPy statement of the model, U within 1e-12 and
    the gradient within 1e-9 relative (SciPy's digamma against the source's own series), and SOURCE (non-centred) against the
    centred one through the change of variables, at M = 40, D = 5, J = 2, N = 12."""
    M, D, J, N = 40, 5, 2, 12
    kw, w, t, theta, rs = problem(family, M, D, J, 5)
    assert (kw["weights"] == 0).any() and kw["prior_precision"][0] == 0.0
    qc = natural_start(kw, w, t, theta, N, rs, 0.3, sampled)
    DT = D + J + int(sampled)
    Uo, go = orc.potential(oracle_pot(kw, "centred", sampled, theta), qc, want_grad=True)
    assert go.shape == (DT, N)
    ref = [numpy_model(kw, qc[:, n], sampled, theta) for n in range(N)]
    Us, gs = np.array([r[0] for r in ref]), np.stack([r[1] for r in ref], axis=1)
    e = float(np.max(np.abs(Uo - Us) / np.maximum(1.0, np.abs(Us))))
    print("U against NumPy / SciPy", e)
    assert e <= 1e-12
    e = rel(go, gs)
    print("gradient against NumPy / SciPy", e)
    assert e <= 1e-9
    q = np.ascontiguousarray(hostpot(kw, "noncentred", sampled).from_natural(qc))
    assert not np.array_equal(q, qc)
    Un, gn = orc.potential(oracle_pot(kw, "noncentred", sampled, theta), q, want_grad=True)
    Ut, gt = from_centred(kw, q, *orc.potential(oracle_pot(kw, "centred", sampled, theta), natural_np(kw, q), want_grad=True))
    e = float(np.max(np.abs(Un - Ut) / np.maximum(1.0, np.abs(Ut))))
    print("non-centred U against the centred source", e)
    assert e <= 1e-12
    e = rel(gn, gt)
    print("non-centred gradient against the centred source's by the chain rule", e)
    assert e <= 1e-11


@pytest.mark.parametrize("par", PARAMS)
@pytest.mark.parametrize("D,J,sampled", sorted({s[1:] for s in SHAPES}))
def test_hd_lane_walk_replay(D, J, sampled, par):
    """A NumPy replay of what a wave does with the packed table: lane (g, c), register s holds row 4 s + g.  Which (s, g) owns
    each t row and the theta row; what each chain sum returns (t_j and theta reach all four lane groups; with a held theta no
    lane contributes and the argument is used); the group sums S_j (centred) or the sums of gacc * q and the scaling of the
    grouped rows (non-centred); chain_sum(tsum) into theta's owner LAST.  With stand-ins for gL = X^T r and for the lanes'
    shares of dU/dtheta they reproduce the prior part of U and the whole gradient of the closed form."""
    from physicsbasedbayesianinference_amd import glm
    rs = np.random.RandomState(7 * D + J + int(sampled))
    nc = par == "noncentred"
    g_of = rs.randint(-1, J, size=D)
    g_of[rs.permutation(D)[:J + 1]] = np.arange(-1, J)
    lam, mu, tp = rs.choice([0.0, 0.5, 4.0], size=D), rs.standard_normal(D), t_priors(J)
    disp = dict(dispersion="sample", log_dispersion_prior=THETA_PRIOR) if sampled else dict(dispersion=0.8)
    table, nj = glm.pack_prior_groups_dispersion(g_of, tp, lam, mu, **disp)
    DT = D + J + int(sampled)
    DP = glm.padded_dim(DT)
    KS = DP // 4
    theta = rs.uniform(-1.5, 2.5)
    state = np.r_[rs.standard_normal(D), rs.uniform(-2, 2, J), [theta] if sampled else []]
    gL = np.r_[rs.standard_normal(D), np.zeros(DP - D)]     # zero on the t rows, the theta row and the padding: [X | 0]
    tshare = rs.standard_normal(64)                         # each lane's share of sum_i dU_i / dtheta
    lane = np.arange(64)
    g, c = lane >> 4, lane & 15
    rows = np.stack([4 * s + g for s in range(KS)])
    q = np.where(rows < DT, state[np.minimum(rows, DT - 1)], 0.0)
    plam, pmu = table[0][rows], table[1][rows]

    def chain_sum(x):
        return np.tile(x.reshape(4, 16).sum(axis=0), 4)
    # theta: ts = trow >> 2, tg = trow & 3 (arithmetic shift: trow = -1 gives ts = -1, which no register matches)
    trow = D + J if sampled else -1
    ts, tg = trow >> 2, trow & 3
    th = np.zeros(64)
    for s in range(KS):
        th = np.where(s == ts, q[s], th)
    th = chain_sum(np.where(g == tg, th, 0.0))
    if trow < 0:
        assert not th.any()
        th = np.full(64, theta)
    assert np.array_equal(th, np.full(64, theta))
    # the t rows: a lane owns at most one
    trow0 = D
    jo = (g - trow0) & 3
    so = (trow0 + jo) >> 2
    for j in range(J):
        owners = {(int(s), int(gg)) for s in range(KS) for gg in range(4) if 4 * s + gg == D + j}
        assert owners == {(int(so[ln]), int(g[ln])) for ln in lane if jo[ln] == j}, (j, owners)
    if sampled:
        assert (ts, tg) == ((D + J) >> 2, (D + J) & 3) and ts < KS
        if J == 4:      # theta shares its lane group with t_0, one register on
            own0 = lane[jo == 0]
            assert np.all(g[own0] == tg) and np.all(so[own0] + 1 == ts)
    tq = np.array([q[so[ln], ln] if so[ln] < KS else 0.0 for ln in lane])
    tj = np.zeros((4, 64))
    for j in range(J):
        tj[j] = chain_sum(np.where(jo == j, tq, 0.0))
        assert np.array_equal(tj[j], np.full(64, state[D + j]))
    sig, tau = np.exp(tj), np.exp(-2.0 * tj)
    gacc = gL[rows].copy()
    if nc:
        sel = plam.copy()
        for j in range(4):
            sel = np.where(plam == -(j + 1.0), sig[j][None, :], sel)
        weff = np.where(plam < 0.0, sel * q + pmu, q)
        w_true = np.where(g_of < 0, state[:D], mu + np.exp(state[D:D + J][np.maximum(g_of, 0)]) * state[:D])
        for s in range(KS):
            for ln in range(0, 64, 16):
                row = 4 * s + g[ln]
                want = w_true[row] if row < D else (state[row] if row < DT else 0.0)    # t rows and theta row: q as it is
                assert abs(weff[s, ln] - want) <= 1e-15 * max(1.0, abs(want)), (row, weff[s, ln], want)
        G = np.zeros((4, 64))
        for s in range(KS):
            for j in range(4):
                G[j] += np.where(plam[s] == -(j + 1.0), gacc[s] * q[s], 0.0)
        gown = np.zeros(64)
        for j in range(J):
            gown = np.where(jo == j, chain_sum(G[j]) * sig[j], gown)
        gacc = np.where(plam < 0.0, gacc * sel, gacc)
        prec, mean = np.where(plam < 0.0, 1.0, plam), np.where(plam < 0.0, 0.0, pmu)
        hnt = 0.0
    else:
        S = np.zeros((4, 64))
        for s in range(KS):
            for j in range(4):
                S[j] += np.where(plam[s] == -(j + 1.0), (q[s] - pmu[s]) ** 2, 0.0)
        gown, hnt = np.zeros(64), np.zeros(64)
        for j in range(J):
            gown = np.where(jo == j, nj[j] - tau[j] * chain_sum(S[j]), gown)
            hnt = hnt + nj[j] * tj[j]
        prec = plam.copy()
        for j in range(4):
            prec = np.where(plam == -(j + 1.0), tau[j][None, :], prec)
        mean = pmu
    for s in range(KS):
        gacc[s] += np.where(s == so, gown, 0.0)
    # chain_sum(tsum) at theta's owner, after the scaling above
    tsum = np.where(g == tg, chain_sum(tshare), 0.0)
    for s in range(KS):
        gacc[s] += np.where(s == ts, tsum, 0.0)
    U = 0.5 * chain_sum(np.sum(prec * (q - mean) ** 2, axis=0)) + hnt
    grad = prec * (q - mean) + gacc
    # closed form
    x, tt = state[:D], state[D:D + J]
    fixed = g_of < 0
    Uc = 0.5 * np.sum(lam[fixed] * (x[fixed] - mu[fixed]) ** 2) + 0.5 * np.sum(tp[:, 1] * (tt - tp[:, 0]) ** 2)
    gc = np.zeros(DT)
    gc[:D][fixed] = gL[:D][fixed] + lam[fixed] * (x[fixed] - mu[fixed])
    for j in range(J):
        mem = g_of == j
        if nc:
            Uc += 0.5 * np.sum(x[mem] ** 2)
            gc[:D][mem] = np.exp(tt[j]) * gL[:D][mem] + x[mem]
            gc[D + j] = np.exp(tt[j]) * np.sum(gL[:D][mem] * x[mem]) + tp[j, 1] * (tt[j] - tp[j, 0])
        else:
            e = x[mem] - mu[mem]
            Uc += 0.5 * np.exp(-2 * tt[j]) * np.sum(e ** 2) + mem.sum() * tt[j]
            gc[:D][mem] = gL[:D][mem] + np.exp(-2 * tt[j]) * e
            gc[D + j] = mem.sum() - np.exp(-2 * tt[j]) * np.sum(e ** 2) + tp[j, 1] * (tt[j] - tp[j, 0])
    per_chain = tshare.reshape(4, 16).sum(axis=0)
    if sampled:
        Uc += 0.5 * THETA_PRIOR[1] * (theta - THETA_PRIOR[0]) ** 2
    assert np.allclose(U, Uc, rtol=1e-13, atol=1e-13)
    for s in range(KS):
        for ln in range(64):
            row = 4 * s + g[ln]
            want = gc[row] if row < DT else 0.0
            if sampled and row == D + J:
                want = per_chain[c[ln]] + THETA_PRIOR[1] * (theta - THETA_PRIOR[0])
            assert abs(grad[s, ln] - want) <= 1e-12 * max(1.0, abs(want)), (row, ln, grad[s, ln], want)


@pytest.mark.parametrize("D,J,sampled", [(5, 2, True), (5, 2, False), (59, 4, True)])
def test_hd_to_natural_from_natural_split(D, J, sampled):
    import torch
    rs = np.random.RandomState(D + J)
    groups = rs.randint(-1, J, size=D)
    groups[rs.permutation(D)[:J + 1]] = np.arange(-1, J)
    kw = dict(groups=groups, prior_mean=0.5 * rs.standard_normal(D))
    nc, ce = hostpot(kw, "noncentred", sampled), hostpot(kw, "centred", sampled)
    DT = D + J + int(sampled)
    for shape in ((DT,), (DT, 11, 3)):
        q = rs.standard_normal(shape)
        q[D:D + J] = rs.uniform(-1, 1, q[D:D + J].shape)
        keep = q.copy()
        nat = nc.to_natural(q)
        assert nat is not q and np.array_equal(q, keep) and nat.shape == q.shape
        assert np.allclose(nat, natural_np(kw, q), rtol=1e-15, atol=0)
        fixed = groups < 0
        assert np.array_equal(nat[:D][fixed], q[:D][fixed]) and np.array_equal(nat[D:], q[D:])     # t rows and theta pass through
        back = nc.from_natural(nat)
        e = rel(back, q)      # four roundings on a grouped row, as in test_glm_hier_noncentred.py: below 1e-15 of max(1, max|q|)
        print("round trip", shape, e)
        assert e <= 1e-15 and back is not nat and np.array_equal(back[D:], q[D:])
        tq = torch.from_numpy(q)
        tn, tb = nc.to_natural(tq), nc.from_natural(torch.from_numpy(nat))
        assert isinstance(tn, torch.Tensor) and isinstance(tb, torch.Tensor) and tn.data_ptr() != tq.data_ptr()
        assert np.allclose(tn.numpy(), nat, rtol=1e-12, atol=1e-12) and np.allclose(tb.numpy(), back, rtol=1e-12, atol=1e-12)
        for pot, wq in ((nc, nat), (ce, q)):
            w, sc, dv = pot.split(q)
            assert w.shape == (D,) + shape[1:] and sc.shape == (J,) + shape[1:]
            assert np.array_equal(w, wq[:D]) and np.array_equal(sc, np.exp(q[D:D + J]))
            if sampled:
                assert dv.shape == shape[1:] and np.array_equal(dv, np.exp(q[D + J]))
            else:
                assert dv == 1.7
            w, sc, dv = pot.split(tq)
            assert isinstance(w, torch.Tensor) and isinstance(sc, torch.Tensor) and np.allclose(w.numpy(), wq[:D], rtol=1e-12, atol=1e-12)
            assert (isinstance(dv, torch.Tensor) and np.allclose(dv.numpy(), np.exp(q[D + J]), rtol=1e-14)) if sampled else dv == 1.7
        for f in (ce.to_natural, ce.from_natural):          # centred: the identity, as new arrays
            out = f(q)
            assert out is not q and np.array_equal(out, q) and torch.equal(f(tq), tq)


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


EVAL_CASES = [(f, p) + s for f in FAMILY for p in PARAMS for s in SHAPES if shipped(f, p, *s[1:])]


@pytest.mark.gpu
@pytest.mark.parametrize("family,par,M,D,J,sampled", EVAL_CASES)
def test_hd_eval_matches_oracle(P, lib, family, par, M, D, J, sampled):
    kw, w, t, theta, rs = problem(family, M, D, J, 7 * M + D)
    assert (M == 1 or (kw["weights"] == 0).any()) and kw["prior_precision"][0] == 0.0
    pot, op = make(P, kw, par, sampled, theta), oracle_pot(kw, par, sampled, theta)
    DT = D + J + int(sampled)
    assert pot.numDimensions == DT and pot.numCoefficients == D and pot.numGroups == J and pot.sampled == sampled
    assert pot.parametrisation == par and np.array_equal(pot.groups, kw["groups"]) and pot.levels is None
    q = start(kw, par, w, t, theta, N_HD, rs, sampled=sampled)
    Uo, go = orc.potential(op, q, want_grad=True)
    U, g = device_eval(lib, pot, q)                    # a padded leading stride, nothing stored past N
    tag = f"{family} {par} {M}x{D}+{J}+{int(sampled)}"
    check("U " + tag, U, Uo)
    check("grad " + tag, g, go)
    check("t rows", g[D:D + J], go[D:D + J])
    if sampled:
        check("theta row", g[D + J], go[D + J])
    check("call", pot(q), Uo)                          # the class API (ldn == N)
    check("gradient", pot.gradient(q), go)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILY)
@pytest.mark.parametrize("M,D,J,sampled", [(40, 5, 2, True), (203, 14, 4, True), (203, 29, 3, False)])
def test_hd_noncentred_device_against_centred_device(P, lib, family, M, D, J, sampled):
    """The non-centred kernel at q against the centred kernel at to_natural(q): U differs by the Jacobian term sum_j n_j t_j,
    the gradients are related by the chain rule; the theta row is common."""
    kw, w, t, theta, rs = problem(family, M, D, J, 3 * M + D)
    pot, cen = make(P, kw, "noncentred", sampled, theta), make(P, kw, "centred", sampled, theta)
    q = start(kw, "noncentred", w, t, theta, N_HD, rs, sampled=sampled)
    qc = pot.to_natural(q)
    assert np.allclose(qc, natural_np(kw, q), rtol=1e-15, atol=0) and np.array_equal(cen.to_natural(q), q)
    U, g = device_eval(lib, pot, q)
    Uc, gc = device_eval(lib, cen, np.ascontiguousarray(qc))
    Ut, gt = from_centred(kw, q, Uc, gc)
    check("U", U, Ut)
    check("grad", g, gt)
    check("t rows", g[D:D + J], gt[D:D + J])
    if sampled:
        check("theta row", g[D + J], gt[D + J])


# family, parametrisation, M, D, J, h (Leapfrog), h (Stormer-Verlet), L -- N = 303, theta sampled.  Reject fractions from the
# oracle over the four combinations of mass and kT (Leapfrog; Stormer-Verlet); the closest accept test of all 64 is 8.8e-5:
#   gaussian centred         0.18 .. 0.39;  0.34 .. 0.45
#   gaussian noncentred      0.19 .. 0.45;  0.35 .. 0.49
#   negbinomial centred      0.19 .. 0.43;  0.23 .. 0.33
#   negbinomial noncentred   0.17 .. 0.34;  0.28 .. 0.38
ITER_CASES = [("gaussian", "centred", 40, 5, 2, 0.17, 0.17, 8), ("gaussian", "noncentred", 40, 5, 2, 0.17, 0.17, 8),
              ("negbinomial", "centred", 40, 5, 2, 0.35, 0.25, 8), ("negbinomial", "noncentred", 40, 5, 2, 0.3, 0.25, 8)]
ITER_SEED = 11


def iter_inputs(family, par, M, D, J, mass, kt):
    kw, w, t, theta, rs = problem(family, M, D, J, ITER_SEED)
    N = 303
    kT = 2.0 if kt else 1.0
    m = 1.0 + (np.arange(N) % 3) * 0.5 if mass else None
    q = start(kw, par, w, t, theta, N, rs, spread=0.1)
    p = np.ascontiguousarray(rs.standard_normal((D + J + 1, N)) * np.sqrt((m if mass else 1.0) * kT))
    u = rs.uniform(size=N)
    return kw, theta, N, kT, m, q, p, u


@pytest.mark.gpu
@pytest.mark.parametrize("family,par,M,D,J,h_lf,h_sv,L", ITER_CASES)
@pytest.mark.parametrize("method", ["Leapfrog", "Stormer-Verlet"])
@pytest.mark.parametrize("mass", [False, True])
@pytest.mark.parametrize("kt", [False, True])
def test_hd_uploaded_draw_iteration_matches_oracle(P, lib, family, par, M, D, J, h_lf, h_sv, L, method, mass, kt):
    import torch
    h = h_lf if method == "Leapfrog" else h_sv
    d = _dev()
    kw, theta, N, kT, m, q, p, u = iter_inputs(family, par, M, D, J, mass, kt)
    Dt = D + J + 1
    pot, op = make(P, kw, par, True), oracle_pot(kw, par, True)
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


# family, parametrisation, M, D, J, sampled, N, h, L -- S = 3: two 32-row and two 64-row cases.  Reject fractions from the
# oracle: 0.19, 0.38, 0.25, 0.25; the closest accept test is 2.5e-4
RUN_CASES = [("gaussian", "noncentred", 203, 28, 3, True, 300, 0.07, 8), ("negbinomial", "centred", 203, 29, 3, False, 300, 0.25, 8),
             ("gaussian", "centred", 1000, 60, 4, False, 200, 0.2, 8), ("negbinomial", "noncentred", 1000, 59, 4, True, 200, 0.11, 8)]
RUN_SEED, RUN_ITER0, RUN_CHAIN0, RUN_S, RUN_DATA = 17, 3, 1000003, 3, 21


@pytest.mark.gpu
@pytest.mark.parametrize("family,par,M,D,J,sampled,N,h,L", RUN_CASES)
def test_hd_philox_run_matches_oracle(P, lib, family, par, M, D, J, sampled, N, h, L):
    """pbbi_hmc_run, PBBI_DRAW_F64: the oracle draws its own momenta of the whole state (no device draw is replayed)."""
    import torch
    d = _dev()
    kw, w, t, theta, rs = problem(family, M, D, J, RUN_DATA)
    q = start(kw, par, w, t, theta, N, rs, spread=0.1, sampled=sampled)
    pot = make(P, kw, par, sampled, theta)
    Dt, S = D + J + int(sampled), RUN_S
    assert glm_rows(Dt) == (32 if M == 203 else 64)
    ldn = N + 5
    qd = padded(q, ldn)
    samples, momenta = d.empty((S, Dt, N), np.float64, 0), d.empty((S, Dt, N), np.float64, 0)
    rej, ratio = d.empty((S, N), np.uint8, 0), d.empty((S, N), np.float64, 0)
    flags = lib.COMPAT_P_FROM_OLDQ | lib.DRAW_F64
    lib.call("pbbi_hmc_run", pot.handle, 0, qd.data_ptr(), None, samples.data_ptr(), momenta.data_ptr(), rej.data_ptr(),
             ratio.data_ptr(), N, ldn, h, L, S, flags, RUN_SEED, RUN_ITER0, RUN_CHAIN0, 1.0, d.stream_ptr(0))
    torch.cuda.synchronize()
    so, mo, rejo, ro = orc.hmc_run_philox(oracle_pot(kw, par, sampled, theta), "Leapfrog", q, None, h, L, S, RUN_SEED, RUN_ITER0,
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


def glm_rows(Dt):
    from physicsbasedbayesianinference_amd import glm
    return glm.padded_dim(Dt)


@pytest.mark.gpu
@pytest.mark.parametrize("method", [0, 1])
def test_hd_run_equals_runs_of_one_bit_for_bit(P, lib, method):
    """A run of S = 9 equals 9 runs of one, bit for bit; the burn-in form (samples_out = NULL) ends in the same state."""
    import torch
    d = _dev()
    family, par, M, D, J, sampled, h = (("gaussian", "noncentred", 203, 14, 4, True, 0.04) if method == 0 else
                                        ("negbinomial", "centred", 203, 29, 3, False, 0.03))
    kw, w, t, theta, rs = problem(family, M, D, J, 31)
    pot = make(P, kw, par, sampled, theta)
    Dt = D + J + int(sampled)
    N, L, S, seed, chain0, iter0 = 333, 4, 9, 8, 5, 2
    m = 1.0 + (np.arange(N) % 3) * 0.5
    md = d.as_device(m, 0, np.float64)
    st = d.stream_ptr(0)
    q0 = start(kw, par, w, t, theta, N, rs, spread=0.1, sampled=sampled)

    def run(s_per_call, record=True):
        qd = d.as_device(q0, 0, np.float64)
        samples, momenta = d.empty((S, Dt, N), np.float64, 0), d.empty((S, Dt, N), np.float64, 0)
        reject, ratio = d.empty((S, N), np.uint8, 0), d.empty((S, N), np.float64, 0)
        for i in range(0, S, s_per_call):
            lib.call("pbbi_hmc_run", pot.handle, method, qd.data_ptr(), md.data_ptr(), samples[i].data_ptr() if record else None,
                     momenta[i].data_ptr() if record else None, reject[i].data_ptr(), ratio[i].data_ptr(), N, N, h, L,
                     min(s_per_call, S - i), lib.COMPAT_P_FROM_OLDQ, seed, iter0 + i, chain0, 1.0, st)
        torch.cuda.synchronize()
        return tuple(d.to_numpy(a) for a in (samples, momenta, reject, ratio, qd))

    one, each, burn = run(S), run(1), run(S, record=False)
    for a, b in zip(one, each):
        assert np.array_equal(a, b)
    assert np.array_equal(one[4], burn[4]) and np.array_equal(one[2], burn[2]) and np.array_equal(one[3], burn[3])
    assert np.array_equal(one[4], one[0][-1])
    assert np.all(np.isfinite(one[0])) and 0.0 < one[2].mean() < 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILY)
@pytest.mark.parametrize("par", PARAMS)
def test_hd_integrators_match_oracle(P, lib, family, par):
    """pbbi_leapfrog / pbbi_stormer_verlet / pbbi_integrate (v_out) in place, with masses."""
    import torch
    d = _dev()
    M, D, J, N, h, L = 203, 14, 4, 131, 0.02, 7
    kw, w, t, theta, rs = problem(family, M, D, J, 51)
    pot, op = make(P, kw, par, True), oracle_pot(kw, par, True)
    Dt = D + J + 1
    m = 1.0 + (np.arange(N) % 3) * 0.5
    for method in ("Leapfrog", "Stormer-Verlet"):
        for entry in ("pbbi_integrate", "pbbi_leapfrog" if method == "Leapfrog" else "pbbi_stormer_verlet"):
            q, p = start(kw, par, w, t, theta, N, rs, spread=0.1), np.ascontiguousarray(rs.standard_normal((Dt, N)))
            qd, pd, md = (d.as_device(a, 0, np.float64) for a in (q, p, m))
            vd = d.empty((Dt, N), np.float64, 0)
            if entry == "pbbi_integrate":
                lib.call(entry, pot.handle, 0 if method == "Leapfrog" else 1, qd.data_ptr(), pd.data_ptr(), md.data_ptr(),
                         vd.data_ptr(), N, N, h, L, d.stream_ptr(0))
            else:
                lib.call(entry, pot.handle, qd.data_ptr(), pd.data_ptr(), md.data_ptr(), N, N, h, L, d.stream_ptr(0))
            torch.cuda.synchronize()
            v = orc.integrate(op, method, q, p, m, h, L)
            check(entry + " q", d.to_numpy(qd), q)
            check(entry + " p", d.to_numpy(pd), p)
            if entry == "pbbi_integrate":
                check(entry + " v", d.to_numpy(vd), v)


@pytest.mark.gpu
@pytest.mark.parametrize("rng,N", [("philox", 1024), ("numpy", 96)])
def test_hd_through_the_classes(P, lib, rng, N):
    """HMC(...).getSamples on the non-centred HierarchicalDispersionGLM and on the same model as a CustomPotential of SOURCE:
    equal masks, samples and momenta to TOL; split returns the right shapes and the natural scale."""
    from scipy.constants import k as kB
    M, D, J, S = 203, 12, 4, 4
    kw, w, t, theta, rs = problem("gaussian", M, D, J, 71)
    pot = make(P, kw, "noncentred", True)
    prm, DT = model_params(kw, "noncentred", True)
    plug = P.CustomPotential(DT, SOURCE, prm)
    out = []
    for target in (pot, plug):
        np.random.seed(5)
        hmc = P.HMC(P.Ensemble(DT, N), 0.3, 0.03, None, potential=target, rng=rng, seed=13, verbose=False)
        s, m = hmc.getSamples(S, 1 / kB, 0.3)
        out.append((np.asarray(s), np.asarray(m), np.asarray(hmc.reject_masks)))
    (s, m, r), (s2, m2, r2) = out
    assert s.shape == (DT, N, S) and np.all(np.isfinite(s)) and np.all(np.isfinite(m))
    print("reject fraction", r.mean())
    assert 0.0 < r.mean() < 1.0
    assert np.array_equal(r, r2)
    check("samples", s, s2)
    check("momenta", m, m2)
    coef, scales, sigma = pot.split(s)
    assert coef.shape == (D, N, S) and scales.shape == (J, N, S) and sigma.shape == (N, S)
    assert np.array_equal(scales, np.exp(s[D:D + J])) and np.array_equal(sigma, np.exp(s[D + J]))
    assert np.array_equal(coef, pot.to_natural(s)[:D]) and np.allclose(coef, natural_np(kw, s)[:D], rtol=1e-15, atol=0)


@pytest.mark.gpu
def test_hd_smc_and_unsupported_calls(P, lib):
    """TemperedSMC accepts the potential; per-chain lengths and GIST are refused as on every GLM handle; describeRun names
    the kernel, the family, the dispersion and the parametrisation."""
    from physicsbasedbayesianinference_amd.smc import TemperedSMC
    d = _dev()
    M, D, J, N, S = 203, 5, 2, 64, 2
    kw, w, t, theta, rs = problem("negbinomial", M, D, J, 81)
    pot = P.HierarchicalDispersionGLM.with_random_intercepts(
        kw["X"], kw["y"], np.arange(M) % 3, family="negbinomial", groups=kw["groups"], log_scale_prior=(0.0, 4.0),
        prior_precision=kw["prior_precision"], prior_mean=kw["prior_mean"], weights=kw["weights"], offset=kw["offset"],
        dispersion="sample", log_dispersion_prior=THETA_PRIOR, parametrisation="noncentred")
    Dt = D + 3 + J + 1 + 1
    assert pot.numDimensions == Dt and pot.numGroups == J + 1 and list(pot.levels) == [0, 1, 2] and pot.sampled
    assert pot.parametrisation == "noncentred" and pot.numCoefficients == D + 3
    smc = TemperedSMC(pot, Dt, 2048, 0.25, 0.05, 0.05, betas=[0.3, 0.6, 1.0], seed=3)
    q = smc.run()
    assert smc.betas[-1] == 1.0 and np.isfinite(smc.logZ)
    assert np.all(np.isfinite(np.asarray(q.cpu() if hasattr(q, "cpu") else q)))
    L = lib.load()
    qd = d.as_device(0.1 * rs.standard_normal((Dt, N)), 0, np.float64)
    samples = d.empty((S, Dt, N), np.float64, 0)
    rc = L.pbbi_hmc_run_dyn(pot.handle, 0, qd.data_ptr(), None, samples.data_ptr(), None, None, None, None, N, N, 0.1, 4,
                            S, lib.COMPAT_P_FROM_OLDQ | lib.PER_CHAIN_STEPS, 1, 0, 0, 1.0, d.stream_ptr(0))
    assert rc == lib.ERR_UNSUPPORTED, lib.last_error()
    rc = L.pbbi_hmc_run_gist(pot.handle, qd.data_ptr(), None, samples.data_ptr(), None, None, None, None, N, N, 0.1, 4, S,
                             lib.COMPAT_P_FROM_OLDQ, 1, 0, 0, 1.0, d.stream_ptr(0))
    assert rc == lib.ERR_UNSUPPORTED, lib.last_error()
    buf = C.create_string_buffer(2048)
    lib.call("pbbi_describe_run", pot.handle, 0, N, N, 4, S, lib.COMPAT_P_FROM_OLDQ, buf, 2048)
    text = buf.value.decode()
    print(text)
    assert "k_glm" in text and "negbinomial" in text and "non-centred" in text and "GLM_HIER_NC" in text
    assert "log-dispersion sampled: state row %d" % (Dt - 1) in text and "iterations per launch: up to 1" in text
    held = make(P, kw, "centred", False, theta)
    lib.call("pbbi_describe_run", held.handle, 0, N, N, 4, S, lib.COMPAT_P_FROM_OLDQ, buf, 2048)
    text = buf.value.decode()
    print(text)
    assert "negbinomial" in text and "log-dispersion held at" in text and "GLM_HIER_CENTRED" in text and "centred:" in text


@pytest.mark.gpu
@pytest.mark.parametrize("par", PARAMS)
def test_hd_eight_schools_from_the_golden_data(P, lib, par):
    """y_i ~ N(mu + b_i, sigma_i^2) with sigma_i known, b_i ~ N(0, exp(2 t)): the held-sigma form with weights 1 / sigma_i^2, as
    the class text writes it, on tests/golden/eight_schools.data.json; U and gradient against the oracle and, by hand, the
    closed form of U at one state."""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "eight_schools.data.json")) as f:
        data = json.load(f)
    y8, s8 = np.array(data["y"], float), np.array(data["sigma"], float)
    pot = P.HierarchicalDispersionGLM.with_random_intercepts(np.ones((8, 1)), y8, np.arange(8), family="gaussian", dispersion=1.0,
                                                             weights=1 / s8 ** 2, parametrisation=par, prior_precision=0.0,
                                                             log_scale_prior=(0.0, 0.04))
    assert pot.numDimensions == 10 and pot.numCoefficients == 9 and pot.numGroups == 1 and not pot.sampled
    assert list(pot.levels) == list(range(8))
    kw = dict(X=pot.X, y=y8, family="gaussian", groups=pot.groups, log_scale_prior=(0.0, 0.04), weights=1 / s8 ** 2,
              offset=np.zeros(8), prior_precision=np.zeros(9), prior_mean=np.zeros(9))
    rs = np.random.RandomState(8)
    qc = np.ascontiguousarray(np.vstack([4.0 + rs.standard_normal((1, N_HD)), 5.0 * rs.standard_normal((8, N_HD)),
                                         rs.uniform(0.0, 2.0, (1, N_HD))]))
    q = np.ascontiguousarray(pot.from_natural(qc))
    Uo, go = orc.potential(oracle_pot(kw, par, False, 0.0), q, want_grad=True)
    U, g = device_eval(lib, pot, q)
    check("U eight schools " + par, U, Uo)
    check("grad eight schools " + par, g, go)
    mu, b, t = qc[0, 0], qc[1:9, 0], qc[9, 0]
    hand = np.sum(0.5 * (y8 - mu - b) ** 2 / s8 ** 2) + 0.5 * np.exp(-2 * t) * np.sum(b ** 2) + 0.5 * 0.04 * t ** 2 + \
        (8 * t if par == "centred" else 0.0)
    assert abs(U[0] - hand) <= 1e-12 * max(1.0, abs(hand)), (U[0], hand)
    w, scales, sigma = pot.split(q)
    assert sigma == 1.0 and np.allclose(w, qc[:9], rtol=1e-13, atol=1e-13) and np.array_equal(scales, np.exp(qc[9:10]))
