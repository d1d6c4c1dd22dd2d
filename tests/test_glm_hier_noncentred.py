"""The non-centred parametrisation of the hierarchical prior (glm.HierarchicalGLM(parametrisation="noncentred"),
csrc/kernels_glm.hip: k_glm<NT, FAM, true, GLM_HIER_NC>).  The model, data and table are those of test_glm_hier.py; the
state differs on the grouped rows, which hold z_d with w_d = mu_d + exp(t_j) z_d:

    U(z, t) = L(w(z, t)) + 0.5 sum_{fixed} lam_d (w_d - mu_d)^2 + 0.5 sum_{grouped} z_d^2 + sum_j 0.5 lam_tj (t_j - m_tj)^2
    dU/dz_d = exp(t_j) gL_d + z_d,    dU/dw_d = gL_d + lam_d (w_d - mu_d),    dU/dt_j = exp(t_j) sum_{d in j} gL_d z_d + lam_tj (t_j - m_tj)

with L the likelihood sum and gL = X^T r at w(z, t).  It is the centred posterior in other coordinates:
U_nc(z, t) = U_c(w(z, t), t) - sum_j n_j t_j.

The oracle side is this file's own C++ statement of that model (SOURCE_NC) on the prm layout of test_glm_hier.SOURCE,
through `orc.pot_custom(complete_source(SOURCE_NC), D + J, prm)`: potential and gradient written out, rows of weight 0
skipped by a branch.  It is pinned against NumPy, central differences and the centred oracle below.

Tolerance: `check` of test_glm_model.py, TOL = 1e-10 relative to max(1, max|oracle|); reject masks are compared for
equality under `decisive` (reject fraction in [0.1, 0.9], no accept test closer than 1e-8, asserted on the oracle's values).
States are built in natural coordinates by test_glm_hier.start and mapped with from_natural, so every t_j stays in [-2, 2]
and |eta| < 6 at w(z, t); both are asserted.

Step sizes and seeds of the sampling tests, chosen on the CPU from the oracle alone (reject fractions at N = 303 over the
four combinations of mass and kT; the closest accept test of all of them is 4.1e-4):
    iteration  logistic 40 x 5+2:   Leapfrog h = 0.15 (0.19 .. 0.40), Stormer-Verlet h = 0.15 (0.33 .. 0.56), L = 8, seed 11
    iteration  poisson 203 x 15+2:  Leapfrog h = 0.1 (0.22 .. 0.49), Stormer-Verlet h = 0.1 (0.42 .. 0.63), L = 8, seed 11
    philox run logistic 203 x 15+2, N = 300: h = 0.12, L = 8 (reject fraction 0.24); poisson 1000 x 60+4, N = 200: h = 0.07,
               L = 8 (0.22); seed 17, first iteration 3, first chain 1000003, data seed 21
The known answer (the funnel's neck): h = 0.4, L = 6, S = 30 as the issue states them, confirmed with the oracle: on that
target, from that start, under the in-kernel draw's contract with the seeds 2024 .. 2029 it accepts 0.971 .. 0.972 of the
proposals and the largest deviation of the statistics is 2.4 standard errors (seed 2024, the test's: 1.7).

Shapes: all six kernels (NT = 1, 2, 4, both families) build without scratch, so glm.HIER_NC_MAX_DIM is 64 for both families
and the largest shape is D + J = 64.
"""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from test_glm_hier import interleaved, model_params, oracle_pot, problem, start, t_priors
from test_glm_model import LINKS, check, decisive, device_eval, padded, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOURCE_NC = """
PBBI_FN T b0(T z) { return %(b0)s; }
PBBI_FN T b1(T z) { return %(b1)s; }
// w_j of the state q: a fixed row holds it, a grouped row holds z_j
template <class Q>
PBBI_FN T coef(const Q& q, int j, int D, const T* mu, const T* grp, const T* sig) {
    const int k = (int)grp[j];
    return k < 0 ? q[j] : mu[j] + sig[k] * q[j];
}
template <class Q>
PBBI_FN T potential(const Q& q, int DT, const T* prm) {
    const int M = (int)prm[0], D = (int)prm[1];
    const T* X = prm + 2;
    const T* c = X + (long)M * D;
    const T* d = c + M;
    const T* o = d + M;
    const T* lam = o + M;
    const T* mu = lam + DT;
    const T* grp = mu + DT;
    T sig[4] = {1, 1, 1, 1};
    for (int k = 0; k < DT - D; ++k) sig[k] = exp(q[D + k]);
    T s = 0;
    for (int i = 0; i < M; ++i) {
        if (c[i] == 0 && d[i] == 0) continue;   // weight 0: the row is not there
        T z = o[i];
        for (int j = 0; j < D; ++j) z += X[i * D + j] * coef(q, j, D, mu, grp, sig);
        s += c[i] * b0(z) - d[i] * z;
    }
    T r = 0;
    for (int j = 0; j < D; ++j) {
        if ((int)grp[j] < 0) {
            const T e = q[j] - mu[j];
            r += lam[j] * e * e;
        } else {
            r += q[j] * q[j];                     // z ~ N(0, 1): mu is the mean of w and has no part here
        }
    }
    for (int j = D; j < DT; ++j) r += lam[j] * (q[j] - mu[j]) * (q[j] - mu[j]);
    return s + T(0.5) * r;
}
template <class Q, class G>
PBBI_FN void gradient(const Q& q, G& g, int DT, const T* prm) {
    const int M = (int)prm[0], D = (int)prm[1];
    const T* X = prm + 2;
    const T* c = X + (long)M * D;
    const T* d = c + M;
    const T* o = d + M;
    const T* lam = o + M;
    const T* mu = lam + DT;
    const T* grp = mu + DT;
    T sig[4] = {1, 1, 1, 1};
    for (int k = 0; k < DT - D; ++k) sig[k] = exp(q[D + k]);
    for (int j = 0; j < D; ++j) g[j] = 0;           // gL first
    for (int i = 0; i < M; ++i) {
        if (c[i] == 0 && d[i] == 0) continue;
        T z = o[i];
        for (int j = 0; j < D; ++j) z += X[i * D + j] * coef(q, j, D, mu, grp, sig);
        const T w = c[i] * b1(z) - d[i];
        for (int j = 0; j < D; ++j) g[j] += w * X[i * D + j];
    }
    for (int j = D; j < DT; ++j) g[j] = lam[j] * (q[j] - mu[j]);
    for (int j = 0; j < D; ++j) {
        const int k = (int)grp[j];
        if (k < 0) {
            g[j] += lam[j] * (q[j] - mu[j]);
        } else {
            g[D + k] += sig[k] * g[j] * q[j];
            g[j] = sig[k] * g[j] + q[j];
        }
    }
}
"""
FAMILY = ("logistic", "poisson")


def oracle_nc(kw):
    from physicsbasedbayesianinference_amd import custom
    prm, DT = model_params(kw)
    return orc.pot_custom(custom.complete_source(SOURCE_NC % LINKS[kw["family"]]), DT, prm)


def hostpot(kw, parametrisation="noncentred"):
    """A HierarchicalGLM with the attributes of `kw` and no device: what to_natural / from_natural / split read."""
    from physicsbasedbayesianinference_amd import HierarchicalGLM as H
    fake = H.__new__(H)
    groups = np.asarray(kw["groups"])
    fake.numCoefficients, fake.numGroups = groups.size, int(groups.max()) + 1
    fake.groups = groups.astype(np.int32)
    fake.prior_mean = np.zeros(groups.size) if kw.get("prior_mean") is None else np.asarray(kw["prior_mean"], float)
    fake.parametrisation = parametrisation
    return fake


def nc_start(kw, w, t, N, rs, spread=0.3):
    """(D + J, N) sampler states: test_glm_hier.start in natural coordinates, mapped by from_natural; the data bounds of
    the issue are asserted at w(z, t)."""
    qc = start(w, t, N, rs, spread)
    D = w.size
    assert np.all(np.abs(qc[D:]) <= 2.0) and np.all(np.abs(kw["X"] @ qc[:D] + kw["offset"][:, None]) < 6.0)
    return np.ascontiguousarray(hostpot(kw).from_natural(qc))


def natural_np(kw, q):
    """The closed form of to_natural, written out."""
    groups, mu = np.asarray(kw["groups"]), kw["prior_mean"]
    D = groups.size
    out = q.copy()
    for d in range(D):
        if groups[d] >= 0:
            out[d] = mu[d] + np.exp(q[D + groups[d]]) * q[d]
    return out


def numpy_U_nc(kw, q):
    """U of one state from the NumPy statement of the non-centred model."""
    X, y, a, o, n = kw["X"], kw["y"], kw["weights"], kw["offset"], kw["trials"]
    M, D = X.shape
    n = np.ones(M) if n is None else n
    groups, tp = np.asarray(kw["groups"]), np.asarray(kw["log_scale_prior"], float)
    w, t = natural_np(kw, q)[:D], q[D:]
    eta = X @ w + o
    b = np.logaddexp(0.0, eta) if kw["family"] == "logistic" else np.exp(eta)
    U = np.sum(a * (n * b - y * eta))
    fixed = groups < 0
    U += 0.5 * np.sum(kw["prior_precision"][fixed] * (w[fixed] - kw["prior_mean"][fixed]) ** 2)
    U += 0.5 * np.sum(q[:D][~fixed] ** 2)
    return U + 0.5 * np.sum(tp[:, 1] * (t - tp[:, 0]) ** 2)


def members(kw):
    groups = np.asarray(kw["groups"])
    return np.array([np.sum(groups == j) for j in range(int(groups.max()) + 1)], dtype=float)


def from_centred(kw, q, Uc, gc):
    """(U, gradient) of the non-centred model at q from the centred model's at to_natural(q): the Jacobian term and the
    chain rule."""
    groups = np.asarray(kw["groups"])
    D, nj = groups.size, members(kw)
    U = Uc - nj @ q[D:]
    g = gc.copy()
    g[D:] -= nj[:, None]
    for d in range(D):
        j = groups[d]
        if j >= 0:
            e = np.exp(q[D + j])
            g[d] = e * gc[d]
            g[D + j] += gc[d] * e * q[d]
    return U, g


# ------------------------------------------------------------------------------------------------ CPU
def test_nc_abi_declared_bound_and_exported():
    name = "pbbi_potential_create_glm_hier_ex"
    hdr = open(os.path.join(ROOT, "include", "pbbi.h")).read()
    assert re.search(r"\b%s\s*\(" % name, hdr)
    assert re.search(r"#define\s+PBBI_HIER_CENTRED\s+0\b", hdr) and re.search(r"#define\s+PBBI_HIER_NONCENTRED\s+1\b", hdr)
    from physicsbasedbayesianinference_amd import HierarchicalGLM, _lib, glm
    assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name]) == len(_lib.PROTOTYPES["pbbi_potential_create_glm_hier"]) + 1
    assert (_lib.HIER_CENTRED, _lib.HIER_NONCENTRED) == (0, 1)
    lib = _lib.load()
    assert lib.pbbi_version() == 103
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert {name, "pbbi_potential_create_glm_hier"} <= set(re.findall(r"\bT (pbbi_[a-z0-9_]+)", out))
    sig = inspect.signature(HierarchicalGLM.__init__)
    assert sig.parameters["parametrisation"].default == "centred"
    assert HierarchicalGLM.parametrisation == "centred"
    assert sorted(glm.HIER_NC_MAX_DIM) == ["logistic", "poisson"]
    assert all(16 <= glm.HIER_NC_MAX_DIM[f] <= glm.HIER_MAX_DIM[f] for f in FAMILY)


def test_nc_rejects_bad_arguments_on_the_host():
    from physicsbasedbayesianinference_amd import HierarchicalGLM, _lib, glm
    rs = np.random.RandomState(0)
    M, D = 10, 4
    X = rs.standard_normal((M, D))
    yb = rs.randint(0, 2, M).astype(float)
    yc = rs.poisson(2.0, M).astype(float)
    ones, at2 = np.ones(M), np.arange(M) == 2
    g = np.array([-1, 0, 0, 1])
    lo = dict(X=X, y=yb, family="logistic", groups=g, parametrisation="noncentred")
    po = dict(X=X, y=yc, family="poisson", groups=g, parametrisation="noncentred")
    nmax = glm.HIER_NC_MAX_DIM
    bad = [
        # the keyword itself
        (dict(lo, parametrisation="non-centered"), "parametrisation"), (dict(lo, parametrisation=1), "parametrisation"),
        (dict(lo, parametrisation=None), "parametrisation"),
        # a state dimension above HIER_NC_MAX_DIM
        (dict(po, X=np.ones((4, nmax["poisson"])), y=np.zeros(4), groups=np.zeros(nmax["poisson"], int)), "state dimension"),
        (dict(lo, X=np.ones((4, nmax["logistic"] - 3)), y=np.zeros(4), groups=np.arange(nmax["logistic"] - 3) % 4), "state dimension"),
        # float32
        (dict(lo, dtype="float32"), "float64"), (dict(po, dtype="float32"), "float64"),
        # one representative of each rejection HierarchicalGLM makes
        (dict(lo, groups=g[:3]), "groups"), (dict(lo, groups=None), "groups"), (dict(lo, groups=np.array([-2, 0, 0, 1])), "-1"),
        (dict(lo, groups=np.array([-1, 0, 0, 2])), "must be used"), (dict(lo, groups=np.array([-1, 0.5, 0, 1])), "integers"),
        (dict(lo, groups=np.full(D, -1)), "GLM"),
        (dict(lo, X=np.ones((M, 6)), groups=np.array([-1, 0, 1, 2, 3, 4])), "at most 4"),
        (dict(lo, prior_precision=-1.0), "prior_precision"), (dict(lo, prior_mean=np.zeros(D - 1)), "prior_mean"),
        (dict(lo, log_scale_prior=(0.0, -0.1)), "log_scale_prior"), (dict(lo, log_scale_prior="wide"), "log_scale_prior"),
        (dict(lo, family="gaussian"), "family"),
        (dict(lo, X=X[:9]), "rows"), (dict(lo, X=np.where(np.arange(D) == 1, np.nan, X)), "finite"),
        (dict(lo, y=yb + 0.5), "logistic"), (dict(po, y=yc + 0.25), "poisson"),
        (dict(lo, weights=np.where(at2, -0.5, ones)), "weights"), (dict(po, offset=np.zeros(M + 1)), "offset"),
        (dict(po, trials=ones), "trials"), (dict(lo, trials=0.5 * ones), "trials"),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            HierarchicalGLM(**kw)
        print("refused:", sorted(set(kw) - {"X", "y"}), msg)
    with pytest.raises(ValueError, match="parametrisation"):
        HierarchicalGLM.with_random_intercepts(X, yb, np.arange(M) % 3, parametrisation="nc")
    # the C entry point states the same rules (host only: nothing here reaches a device)
    L = _lib.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    tp = np.array([0.0, 1.0] * 4)
    h = C.c_void_p()
    Xs, ys, gi = np.ones((4, 4)), np.zeros(4), np.ascontiguousarray(g, np.int32)

    def create(par, Dn=4, Xn=Xs, groups=gi, J=2, fam=0, dtype=_lib.F64):
        rc = L.pbbi_potential_create_glm_hier_ex(Dn, 4, Xn.ctypes.data_as(dp), ys.ctypes.data_as(dp), fam, None, None, None,
                                                 np.ones(Dn).ctypes.data_as(dp), None, groups.ctypes.data_as(ip), J,
                                                 tp.ctypes.data_as(dp), par, dtype, 0, C.byref(h))
        return rc, _lib.last_error()
    for par in (2, -1):
        rc, err = create(par)
        assert rc == _lib.ERR_INVALID and "parametrisation" in err and not h, (rc, err)
    for fam, family in enumerate(FAMILY):
        Dn = nmax[family] - 1
        gb2 = np.r_[np.zeros(Dn - 1, dtype=np.int32), np.int32(1)]
        rc, err = create(_lib.HIER_NONCENTRED, Dn, np.ones((4, Dn)), gb2, 2, fam)
        assert rc == _lib.ERR_UNSUPPORTED and "<= %d" % nmax[family] in err and not h, (rc, err)
        rc, err = create(_lib.HIER_NONCENTRED, fam=fam, dtype=_lib.F32)
        assert rc == _lib.ERR_UNSUPPORTED and "float64" in err and not h, (rc, err)
        rc, err = create(_lib.HIER_NONCENTRED, fam=fam, J=3)
        assert rc == _lib.ERR_INVALID and "must be used" in err and not h, (rc, err)
    rc, err = create(_lib.HIER_NONCENTRED, fam=3)
    assert rc == _lib.ERR_INVALID and not h, (rc, err)


@pytest.mark.parametrize("D,J", [(14, 2), (60, 4)])
def test_nc_to_natural_from_natural_split(D, J):
    import torch
    rs = np.random.RandomState(D + J)
    kw = dict(groups=interleaved(D, J), prior_mean=0.5 * rs.standard_normal(D))
    nc, ce = hostpot(kw), hostpot(kw, "centred")
    # The round trip z -> w = mu + sig z -> (w - mu) / sig rounds four times: its absolute error is at most (eps / 2) (3 |z| +
    # |w| / sig), and |w| / sig <= |mu| / sig + |z|.  With mu ~ N(0, 1/4) and t in [-1, 1] that is below 2.5e-15 for |z| <= 4,
    # and relative to max(1, max |q|) -- the measure `rel` of every comparison here -- below the 1e-15 of the issue.
    for shape in ((D + J,), (D + J, 11, 3)):
        q = rs.standard_normal(shape)
        q[D:] = rs.uniform(-1, 1, q[D:].shape)
        keep = q.copy()
        nat = nc.to_natural(q)
        assert nat is not q and np.array_equal(q, keep) and nat.shape == q.shape
        assert np.allclose(nat, natural_np(kw, q), rtol=1e-15, atol=0)     # the closed form, row by row
        fixed = kw["groups"] < 0
        assert np.array_equal(nat[:D][fixed], q[:D][fixed]) and np.array_equal(nat[D:], q[D:])
        back = nc.from_natural(nat)
        e = rel(back, q)
        print("round trip", shape, e)
        assert e <= 1e-15 and back is not nat
        assert rel(nc.to_natural(nc.from_natural(q)), q) <= 1e-15
        # tensors come back as tensors, with the same numbers
        tq = torch.from_numpy(q)
        tn, tb = nc.to_natural(tq), nc.from_natural(torch.from_numpy(nat))
        assert isinstance(tn, torch.Tensor) and isinstance(tb, torch.Tensor) and tn.data_ptr() != tq.data_ptr()
        assert np.allclose(tn.numpy(), nat, rtol=1e-12, atol=1e-12) and np.allclose(tb.numpy(), back, rtol=1e-12, atol=1e-12)
        # split: natural scale for both forms
        w, sc = nc.split(q)
        assert w.shape == (D,) + shape[1:] and sc.shape == (J,) + shape[1:]
        assert np.array_equal(w, nat[:D]) and np.array_equal(sc, np.exp(q[D:]))
        w, sc = nc.split(tq)
        assert isinstance(w, torch.Tensor) and isinstance(sc, torch.Tensor) and torch.equal(w, tn[:D])
        # centred: the identity, as new arrays
        for f in (ce.to_natural, ce.from_natural):
            out = f(q)
            assert out is not q and np.array_equal(out, q)
            assert torch.equal(f(tq), tq)
        w, sc = ce.split(q)
        assert np.array_equal(w, q[:D]) and np.array_equal(sc, np.exp(q[D:]))


@pytest.mark.parametrize("family", FAMILY)
def test_nc_oracle_source_is_pinned(family):
    """The yardstick, not the feature: SOURCE_NC against NumPy, central differences of its own U, and the centred oracle
    of test_glm_hier through the Jacobian term and the chain rule, at M = 40, D = 5, J = 2, N = 12."""
    M, D, J, N = 40, 5, 2, 12
    kw, w, t, rs = problem(family, M, D, J, 5)
    q = nc_start(kw, w, t, N, rs)
    op = oracle_nc(kw)
    U, g = orc.potential(op, q, want_grad=True)
    assert g.shape[0] == D + J
    Us = np.array([numpy_U_nc(kw, q[:, n]) for n in range(N)])
    e = float(np.max(np.abs(U - Us) / np.maximum(1.0, np.abs(Us))))
    print("U against NumPy", e)
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
    Uc, gc = orc.potential(oracle_pot(kw), hostpot(kw).to_natural(q), want_grad=True)
    Ut, gt = from_centred(kw, q, Uc, gc)
    e = float(np.max(np.abs(U - Ut) / np.maximum(1.0, np.abs(Ut))))
    print("U against the centred oracle", e)
    assert e <= 1e-12
    e = rel(g, gt)
    print("gradient against the centred oracle's by the chain rule", e)
    assert e <= 1e-11


@pytest.mark.parametrize("D,J", [(3, 1), (5, 2), (14, 2), (15, 2), (16, 1), (28, 4), (60, 4)])
def test_nc_lane_walk_replay(D, J):
    """A NumPy replay of what a wave of the non-centred kernel does with the packed table: lane (g, c), register s holds
    row 4 s + g.  The owner compare and chain sum that hand t_j to all four lane groups; the select that builds weff from
    the sign-coded lam slot; the per-lane sums of gacc * q per group with their chain sum, scaled by sig_j into the owner's
    register; the scaling of the grouped rows of gacc; the {precision, mean} select of the prior.  With an arbitrary
    stand-in for gL = X^T r they reproduce the prior part of U and the whole gradient of the closed form."""
    from physicsbasedbayesianinference_amd import glm
    rs = np.random.RandomState(7 * D + J)
    g_of = rs.randint(-1, J, size=D)
    g_of[rs.permutation(D)[:J + 1]] = np.arange(-1, J)
    lam, mu, tp = rs.choice([0.0, 0.5, 4.0], size=D), rs.standard_normal(D), t_priors(J)
    table, nj = glm.pack_prior_groups(g_of, tp, lam, mu)
    DT, DP = D + J, glm.padded_dim(D + J)
    KS = DP // 4
    state = np.r_[rs.standard_normal(D), rs.uniform(-2, 2, J)]
    gL = np.r_[rs.standard_normal(D), np.zeros(DP - D)]          # zero on the t rows and the padding: the image of [X | 0]
    lane = np.arange(64)
    g = lane >> 4
    rows = np.stack([4 * s + g for s in range(KS)])
    q = np.where(rows < DT, state[np.minimum(rows, DT - 1)], 0.0)
    plam, pmu = table[0][rows], table[1][rows]

    def chain_sum(x):
        return np.tile(x.reshape(4, 16).sum(axis=0), 4)
    jo = (g - D) & 3
    so = (D + jo) >> 2
    th = np.array([q[so[ln], ln] if so[ln] < KS else 0.0 for ln in range(64)])
    sig = np.ones((4, 64))
    for j in range(J):
        tj = chain_sum(np.where(jo == j, th, 0.0))
        assert np.array_equal(tj, np.full(64, state[D + j]))
        sig[j] = np.exp(tj)
    # weff: grouped ? fma(sig_j, q, mu) : q
    sel = plam.copy()
    for j in range(4):
        sel = np.where(plam == -(j + 1.0), sig[j][None, :], sel)
    weff = np.where(plam < 0.0, sel * q + pmu, q)
    w_true = np.where(g_of < 0, state[:D], mu + np.exp(state[D:][np.maximum(g_of, 0)]) * state[:D])
    for s in range(KS):
        for ln in range(0, 64, 16):
            row = 4 * s + g[ln]
            want = w_true[row] if row < D else (state[row] if row < DT else 0.0)
            assert abs(weff[s, ln] - want) <= 1e-15 * max(1.0, abs(want)), (row, weff[s, ln], want)
    assert np.array_equal(q, np.where(rows < DT, state[np.minimum(rows, DT - 1)], 0.0))      # q itself is untouched
    # after the products: gacc = gL in the state layout
    gacc = gL[rows]
    G = np.zeros((4, 64))
    for s in range(KS):
        for j in range(4):
            G[j] += np.where(plam[s] == -(j + 1.0), gacc[s] * q[s], 0.0)
    gown = np.zeros(64)
    for j in range(J):
        gown = np.where(jo == j, chain_sum(G[j]) * sig[j], gown)
    gacc = np.where(plam < 0.0, gacc * sel, gacc)
    for s in range(KS):
        gacc[s] += np.where(s == so, gown, 0.0)
    # the prior in the sampled coordinate: a grouped row has precision 1 and mean 0
    prec, mean = np.where(plam < 0.0, 1.0, plam), np.where(plam < 0.0, 0.0, pmu)
    U = 0.5 * chain_sum(np.sum(prec * (q - mean) ** 2, axis=0))
    grad = prec * (q - mean) + gacc
    # closed form
    z, tt = state[:D], state[D:]
    fixed = g_of < 0
    Uc = 0.5 * np.sum(lam[fixed] * (z[fixed] - mu[fixed]) ** 2) + 0.5 * np.sum(z[~fixed] ** 2) + \
        0.5 * np.sum(tp[:, 1] * (tt - tp[:, 0]) ** 2)
    gc = np.zeros(DT)
    gc[:D][fixed] = gL[:D][fixed] + lam[fixed] * (z[fixed] - mu[fixed])
    for j in range(J):
        mem = g_of == j
        gc[:D][mem] = np.exp(tt[j]) * gL[:D][mem] + z[mem]
        gc[D + j] = np.exp(tt[j]) * np.sum(gL[:D][mem] * z[mem]) + tp[j, 1] * (tt[j] - tp[j, 0])
    assert np.allclose(U, Uc, rtol=1e-13, atol=1e-13)
    for s in range(KS):
        for ln in range(0, 64, 16):
            row = 4 * s + g[ln]
            want = gc[row] if row < DT else 0.0
            assert abs(grad[s, ln] - want) <= 1e-12 * max(1.0, abs(want)), (row, grad[s, ln], want)


KA_D, KA_N, KA_H, KA_L, KA_S, KA_SEED = 6, 4096, 0.4, 6, 30, 2024
KA_TP = np.array([(0.2, 0.25), (-0.3, 0.25)])
KA_GROUPS = np.array([0, 1, 0, 1, 0, 1])
KA_MU = np.array([0.5, -0.25, 1.0, 0.0, -1.5, 0.75])
PHI_M1 = 0.158655                      # Phi(-1)


def known_answer_kw():
    return dict(X=np.zeros((1, KA_D)), y=np.zeros(1), family="poisson", groups=KA_GROUPS, log_scale_prior=KA_TP,
                prior_mean=KA_MU, weights=None, offset=None, trials=None, prior_precision=1.0)


def known_answer_start():
    """Every chain at the point z = 0, t = m."""
    return np.ascontiguousarray(np.tile(np.r_[np.zeros(KA_D), KA_TP[:, 0]][:, None], (1, KA_N)))


def known_answer_check(q):
    """The statistics of the issue (its list gives 6 + 6 + 2 + 2 + 2 = 18 of them), each within 5 exact standard errors (the chains are independent): mean z_d against
    0 (SE 1/sqrt(N)), var z_d against 1 (sqrt(2/N)), mean t_j against m_j (2/sqrt(N)), var t_j against 4 (4 sqrt(2/N)), the
    share of chains with t_j < m_j - 2 against Phi(-1) (binomial SE) -- the neck.  Returns the largest deviation."""
    N = q.shape[1]
    z, t, m = q[:KA_D], q[KA_D:], KA_TP[:, 0]
    dev = np.r_[np.abs(z.mean(axis=1)) * np.sqrt(N),
                np.abs(z.var(axis=1, ddof=1) - 1.0) / np.sqrt(2.0 / N),
                np.abs(t.mean(axis=1) - m) / (2.0 / np.sqrt(N)),
                np.abs(t.var(axis=1, ddof=1) - 4.0) / (4.0 * np.sqrt(2.0 / N)),
                np.abs((t < (m - 2.0)[:, None]).mean(axis=1) - PHI_M1) / np.sqrt(PHI_M1 * (1.0 - PHI_M1) / N)]
    assert dev.size == 2 * KA_D + 6
    print("deviations in standard errors:", np.round(dev, 2))
    assert np.all(dev <= 5.0), dev
    return float(dev.max())


def test_nc_known_answer_bounds_hold_for_fresh_draws():
    for seed in (KA_SEED, KA_SEED + 1):
        rs = np.random.RandomState(seed)
        known_answer_check(np.vstack([rs.standard_normal((KA_D, KA_N)), KA_TP[:, 0, None] + 2.0 * rs.standard_normal((2, KA_N))]))


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


def nc_pot(P, kw):
    return P.HierarchicalGLM(parametrisation="noncentred", **kw)


N_HIER = 100   # six full wave tiles and one of 4 chains; the second workgroup has one ghost wave


def eval_shapes(family):
    try:
        from physicsbasedbayesianinference_amd import glm
        dmax = glm.HIER_NC_MAX_DIM[family]
    except (ImportError, AttributeError, KeyError):      # the names do not exist: the CPU tests say so
        return [(1, 3, 1, "drawn")]
    shapes = [(1, 3, 1, "drawn"), (40, 5, 2, "drawn"), (40, 14, 2, "drawn"), (40, 15, 2, "drawn"), (203, 16, 1, "drawn"),
              (203, 28, 4, "drawn"), (1000, 60, 4, "drawn"), (203, 60, 4, "single"), (203, 16, 4, "all")]
    return [s for s in shapes if s[1] + s[2] <= dmax]


def eval_problem(family, M, D, J, how):
    kw, w, t, rs = problem(family, M, D, J, 7 * M + D)
    if how == "single":
        kw["groups"] = interleaved(D, J, single=True)
        assert np.sum(kw["groups"] == J - 1) == 1
    elif how == "all":
        kw["groups"] = interleaved(D, J, all_grouped=True)
        assert not (kw["groups"] < 0).any()
    return kw, w, t, rs


@pytest.mark.gpu
@pytest.mark.parametrize("family,M,D,J,how", [(f,) + s for f in FAMILY for s in eval_shapes(f)])
def test_nc_eval_matches_oracle(P, lib, family, M, D, J, how):
    kw, w, t, rs = eval_problem(family, M, D, J, how)
    assert M == 1 or (kw["weights"] == 0).any()
    pot, op = nc_pot(P, kw), oracle_nc(kw)
    assert pot.numDimensions == D + J and pot.numCoefficients == D and pot.numGroups == J
    assert pot.parametrisation == "noncentred" and np.array_equal(pot.groups, kw["groups"])
    q = nc_start(kw, w, t, N_HIER, rs)
    Uo, go = orc.potential(op, q, want_grad=True)
    U, g = device_eval(lib, pot, q)
    check(f"U {family} {M}x{D}+{J} {how}", U, Uo)
    check(f"grad {family} {M}x{D}+{J} {how}", g, go)
    check("t rows", g[D:], go[D:])
    check("call", pot(q), Uo)                           # the class API (ldn == N)
    check("gradient", pot.gradient(q), go)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILY)
@pytest.mark.parametrize("M,D,J", [(40, 5, 2), (203, 15, 2), (203, 28, 4)])
def test_nc_device_against_centred_device(P, lib, family, M, D, J):
    """The non-centred kernel at q against the existing centred kernel at to_natural(q): U differs by the Jacobian term
    sum_j n_j t_j, the gradients are related by the chain rule."""
    kw, w, t, rs = problem(family, M, D, J, 3 * M + D)
    pot, cen = nc_pot(P, kw), P.HierarchicalGLM(**kw)
    assert cen.parametrisation == "centred"
    q = nc_start(kw, w, t, N_HIER, rs)
    qc = pot.to_natural(q)
    assert np.allclose(qc, natural_np(kw, q), rtol=1e-15, atol=0) and np.array_equal(cen.to_natural(q), q)
    U, g = device_eval(lib, pot, q)
    Uc, gc = device_eval(lib, cen, np.ascontiguousarray(qc))
    Ut, gt = from_centred(kw, q, Uc, gc)
    check("U", U, Ut)
    check("grad", g, gt)
    check("z and fixed rows", g[:D], gt[:D])
    check("t rows", g[D:], gt[D:])


# family, M, D, J, h (Leapfrog), h (Stormer-Verlet), L -- N = 303; the shapes of test_glm_hier.ITER_CASES, both h from the
# oracle alone (the module text has the reject fractions)
ITER_CASES = [("logistic", 40, 5, 2, 0.15, 0.15, 8), ("poisson", 203, 15, 2, 0.1, 0.1, 8)]
ITER_SEED = 11


def iter_inputs(family, M, D, J, mass, kt):
    kw, w, t, rs = problem(family, M, D, J, ITER_SEED)
    N = 303
    kT = 2.0 if kt else 1.0
    m = 1.0 + (np.arange(N) % 3) * 0.5 if mass else None
    q = nc_start(kw, w, t, N, rs, spread=0.1)
    p = np.ascontiguousarray(rs.standard_normal((D + J, N)) * np.sqrt((m if mass else 1.0) * kT))
    u = rs.uniform(size=N)
    return kw, N, kT, m, q, p, u


@pytest.mark.gpu
@pytest.mark.parametrize("family,M,D,J,h_lf,h_sv,L", ITER_CASES)
@pytest.mark.parametrize("method", ["Leapfrog", "Stormer-Verlet"])
@pytest.mark.parametrize("mass", [False, True])
@pytest.mark.parametrize("kt", [False, True])
def test_nc_uploaded_draw_iteration_matches_oracle(P, lib, family, M, D, J, h_lf, h_sv, L, method, mass, kt):
    import torch
    h = h_lf if method == "Leapfrog" else h_sv
    d = _dev()
    kw, N, kT, m, q, p, u = iter_inputs(family, M, D, J, mass, kt)
    Dt = D + J
    pot, op = nc_pot(P, kw), oracle_nc(kw)
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


# family, M, D, J, N, h, L -- S = 3; the shapes of test_glm_hier.RUN_CASES
RUN_CASES = [("logistic", 203, 15, 2, 300, 0.12, 8), ("poisson", 1000, 60, 4, 200, 0.07, 8)]
RUN_SEED, RUN_ITER0, RUN_CHAIN0, RUN_S, RUN_DATA = 17, 3, 1000003, 3, 21


@pytest.mark.gpu
@pytest.mark.parametrize("family,M,D,J,N,h,L", RUN_CASES)
def test_nc_philox_run_matches_oracle(P, lib, family, M, D, J, N, h, L):
    """pbbi_hmc_run, PBBI_DRAW_F64: the oracle draws its own momenta of the (D + J, N) state (no device draw is replayed)."""
    import torch
    d = _dev()
    kw, w, t, rs = problem(family, M, D, J, RUN_DATA)
    q = nc_start(kw, w, t, N, rs, spread=0.1)
    pot = nc_pot(P, kw)
    Dt, S = D + J, RUN_S
    ldn = N + 5
    qd = padded(q, ldn)
    samples, momenta = d.empty((S, Dt, N), np.float64, 0), d.empty((S, Dt, N), np.float64, 0)
    rej, ratio = d.empty((S, N), np.uint8, 0), d.empty((S, N), np.float64, 0)
    flags = lib.COMPAT_P_FROM_OLDQ | lib.DRAW_F64
    lib.call("pbbi_hmc_run", pot.handle, 0, qd.data_ptr(), None, samples.data_ptr(), momenta.data_ptr(), rej.data_ptr(),
             ratio.data_ptr(), N, ldn, h, L, S, flags, RUN_SEED, RUN_ITER0, RUN_CHAIN0, 1.0, d.stream_ptr(0))
    torch.cuda.synchronize()
    so, mo, rejo, ro = orc.hmc_run_philox(oracle_nc(kw), "Leapfrog", q, None, h, L, S, RUN_SEED, RUN_ITER0, RUN_CHAIN0, 1.0,
                                          compat=orc.COMPAT_P_FROM_OLDQ | orc.DRAW_F64)
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
@pytest.mark.parametrize("method", [0, 1])
def test_nc_run_equals_runs_of_one_bit_for_bit(P, lib, method):
    """A run of S = 21 equals 21 runs of one, bit for bit; the burn-in form (samples_out = NULL) ends in the same state."""
    import torch
    d = _dev()
    family, M, D, J, h = ("logistic", 203, 15, 2, 0.06) if method == 0 else ("poisson", 203, 28, 4, 0.03)
    kw, w, t, rs = problem(family, M, D, J, 31)
    pot = nc_pot(P, kw)
    Dt = D + J
    N, L, S, seed, chain0, iter0 = 333, 4, 21, 8, 5, 2
    m = 1.0 + (np.arange(N) % 3) * 0.5
    md = d.as_device(m, 0, np.float64)
    st = d.stream_ptr(0)
    q0 = nc_start(kw, w, t, N, rs, spread=0.1)

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
def test_nc_integrators_match_oracle(P, lib, family):
    """pbbi_leapfrog / pbbi_stormer_verlet / pbbi_integrate (v_out) in place, with masses."""
    import torch
    d = _dev()
    M, D, J, N, h, L = 203, 15, 2, 131, 0.02, 7
    kw, w, t, rs = problem(family, M, D, J, 51)
    pot, op = nc_pot(P, kw), oracle_nc(kw)
    Dt = D + J
    m = 1.0 + (np.arange(N) % 3) * 0.5
    for method in ("Leapfrog", "Stormer-Verlet"):
        for entry in ("pbbi_integrate", "pbbi_leapfrog" if method == "Leapfrog" else "pbbi_stormer_verlet"):
            q, p = nc_start(kw, w, t, N, rs, spread=0.1), np.ascontiguousarray(rs.standard_normal((Dt, N)))
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
@pytest.mark.parametrize("rng,N", [("philox", 4096), ("numpy", 96)])
def test_nc_through_the_classes(P, lib, rng, N):
    """HMC(...).getSamples on the non-centred HierarchicalGLM and on the same model as a CustomPotential of SOURCE_NC: equal
    masks, samples and momenta to TOL; split returns the natural scale."""
    from scipy.constants import k as kB
    M, D, J, S = 203, 15, 2, 4
    kw, w, t, rs = problem("logistic", M, D, J, 71)
    pot = nc_pot(P, kw)
    prm, DT = model_params(kw)
    plug = P.CustomPotential(DT, SOURCE_NC % LINKS["logistic"], prm)
    out = []
    for target in (pot, plug):
        np.random.seed(5)
        hmc = P.HMC(P.Ensemble(DT, N), 0.45, 0.05, None, potential=target, rng=rng, seed=13, verbose=False)
        s, m = hmc.getSamples(S, 1 / kB, 0.3)
        out.append((np.asarray(s), np.asarray(m), np.asarray(hmc.reject_masks)))
    (s, m, r), (s2, m2, r2) = out
    assert s.shape == (DT, N, S) and np.all(np.isfinite(s)) and np.all(np.isfinite(m))
    print("reject fraction", r.mean())
    assert 0.0 < r.mean() < 1.0
    assert np.array_equal(r, r2)
    check("samples", s, s2)
    check("momenta", m, m2)
    coef, scales = pot.split(s)
    assert coef.shape == (D, N, S) and scales.shape == (J, N, S) and np.array_equal(scales, np.exp(s[D:]))
    assert np.array_equal(coef, pot.to_natural(s)[:D]) and np.allclose(coef, natural_np(kw, s)[:D], rtol=1e-15, atol=0)


@pytest.mark.gpu
def test_nc_smc_and_unsupported_calls(P, lib):
    """TemperedSMC accepts the potential; per-chain lengths and GIST are refused as on every GLM handle; describeRun
    names the kernel and the form."""
    from physicsbasedbayesianinference_amd.smc import TemperedSMC
    d = _dev()
    M, D, J, N, S = 203, 5, 2, 64, 2
    kw, w, t, rs = problem("logistic", M, D, J, 81)
    pot = P.HierarchicalGLM.with_random_intercepts(kw["X"], kw["y"], np.arange(M) % 3, family="logistic", groups=kw["groups"],
                                                   log_scale_prior=(0.0, 4.0), prior_precision=kw["prior_precision"],
                                                   prior_mean=kw["prior_mean"], weights=kw["weights"], offset=kw["offset"],
                                                   trials=kw["trials"], parametrisation="noncentred")
    Dt = D + 3 + J + 1
    assert pot.numDimensions == Dt and pot.numGroups == J + 1 and list(pot.levels) == [0, 1, 2]
    assert pot.parametrisation == "noncentred"
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
    p, u = d.as_device(rs.standard_normal((Dt, N)), 0, np.float64), d.as_device(rs.uniform(size=N), 0, np.float64)
    rc = L.pbbi_hmc_iter_dyn(pot.handle, 0, qd.data_ptr(), p.data_ptr(), u.data_ptr(), None, None, samples.data_ptr(), None,
                             None, None, None, N, N, 0.1, 4, lib.PER_CHAIN_STEPS, 1.0, d.stream_ptr(0))
    assert rc == lib.ERR_UNSUPPORTED, lib.last_error()
    buf = C.create_string_buffer(1024)
    lib.call("pbbi_describe_run", pot.handle, 0, N, N, 4, S, lib.COMPAT_P_FROM_OLDQ, buf, 1024)
    text = buf.value.decode()
    print(text)
    assert "k_glm" in text and "non-centred" in text and "iterations per launch: up to 1" in text


@pytest.mark.gpu
def test_nc_known_answer_the_funnels_neck(P, lib):
    """X = 0, one observation: the likelihood is constant, and in the sampled coordinates the target is exactly z_d ~ N(0, 1),
    t_j ~ N(m_j, 4), all independent -- in the centred form a funnel (the scale prior has sd 2) that no single step size
    serves.  N = 4096 chains start at the point z = 0, t = m; after 30 iterations of Leapfrog (h = 0.4, L = 6) with the
    in-kernel draw each chain's final state is tested against the 22 moments and tail shares of known_answer_check.  The
    oracle on this target with these values accepts 0.97 of the proposals (the module text has the figures)."""
    import torch
    d = _dev()
    kw = known_answer_kw()
    pot = P.HierarchicalGLM(kw["X"], kw["y"], family="poisson", groups=KA_GROUPS, log_scale_prior=KA_TP, prior_mean=KA_MU,
                            parametrisation="noncentred")
    q0 = known_answer_start()
    N = KA_N
    qd = d.as_device(q0, 0, np.float64)
    rej = d.empty((KA_S, N), np.uint8, 0)
    lib.call("pbbi_hmc_run", pot.handle, 0, qd.data_ptr(), None, None, None, rej.data_ptr(), None, N, N, KA_H, KA_L, KA_S,
             lib.COMPAT_P_FROM_OLDQ, KA_SEED, 0, 0, 1.0, d.stream_ptr(0))
    torch.cuda.synchronize()
    acc = 1.0 - float(d.to_numpy(rej).mean())
    q = d.to_numpy(qd)
    print("accept rate", acc)
    assert np.all(np.isfinite(q)) and not np.array_equal(q, q0)
    assert 0.9 <= acc < 1.0, acc
    known_answer_check(q)
