"""Hierarchical priors with sampled group scales (glm.HierarchicalGLM, csrc/kernels_glm.hip: k_glm<NT, FAM, true, true>).
Families logistic and poisson, the full model of GLM (weights a_i, trials n_i, offsets o_i, eta_i = x_i . w + o_i);
groups_d is -1 (fixed prior) or a group index j, and the members of group j share the scale exp(t_j):

    U(w, t) = sum_i a_i [ n_i b(eta_i) - y_i eta_i ] + 0.5 sum_{d: groups_d < 0} lam_d (w_d - mu_d)^2
            + sum_j [ 0.5 exp(-2 t_j) S_j + n_j t_j + 0.5 lam_tj (t_j - m_tj)^2 ],    S_j = sum_{d in j} (w_d - mu_d)^2

State rows 0 .. D-1 are the coefficients, rows D .. D+J-1 are t_0 .. t_{J-1}.

The oracle side is the user-source mechanism of test_glm_dispersion.py, `orc.pot_custom(complete_source(SOURCE), D + J,
prm)`, with this file's own C++ statement of the model: prm = [M, D, X.ravel(), c, d, o, lam(D + J), mu(D + J),
groups(D)], c = a n, d = a y, potential and gradient written out, rows of weight 0 skipped by a branch.

Tolerance: `rel` / `check` of test_glm_model.py with TOL = 1e-10 relative to max(1, max|oracle|); reject masks are
compared for equality under its `decisive` preconditions (asserted on the oracle's values).  Step sizes and seeds of
the sampling tests were chosen on the CPU from the oracle alone, so that the reject fraction lies in [0.1, 0.9] and no
accept test is closer than 1e-8.  The data keeps every t_j in [-2, 2] and |eta| < 6.

Shapes: neither family's kernel at a padded state dimension of 128 is shipped (it cannot be built without scratch), so
glm.HIER_MAX_DIM is 64 for both and the largest shape is D + J = 64.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from test_glm_model import LINKS, check, decisive, device_eval, padded, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOURCE = """
PBBI_FN T b0(T z) { return %(b0)s; }
PBBI_FN T b1(T z) { return %(b1)s; }
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
    T s = 0;
    for (int i = 0; i < M; ++i) {
        if (c[i] == 0 && d[i] == 0) continue;   // weight 0: the row is not there
        T z = o[i];
        for (int j = 0; j < D; ++j) z += X[i * D + j] * q[j];
        s += c[i] * b0(z) - d[i] * z;
    }
    T r = 0;
    for (int j = 0; j < D; ++j) {
        const int k = (int)grp[j];
        const T e = q[j] - mu[j];
        if (k < 0) {
            r += lam[j] * e * e;
        } else {
            r += exp(-2 * q[D + k]) * e * e;
            s += q[D + k];                        // the normaliser of N(mu, exp(2 t)): n_j t_j in all
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
    for (int j = D; j < DT; ++j) g[j] = lam[j] * (q[j] - mu[j]);
    for (int j = 0; j < D; ++j) {
        const int k = (int)grp[j];
        const T e = q[j] - mu[j];
        if (k < 0) {
            g[j] = lam[j] * e;
        } else {
            const T tau = exp(-2 * q[D + k]);
            g[j] = tau * e;
            g[D + k] += T(1) - tau * e * e;
        }
    }
    for (int i = 0; i < M; ++i) {
        if (c[i] == 0 && d[i] == 0) continue;
        T z = o[i];
        for (int j = 0; j < D; ++j) z += X[i * D + j] * q[j];
        const T w = c[i] * b1(z) - d[i];
        for (int j = 0; j < D; ++j) g[j] += w * X[i * D + j];
    }
}
"""
FAMILY = ("logistic", "poisson")


def t_priors(J):
    """J pairs (mean, precision) of the log-scales: all different, one flat."""
    return np.array([(0.3, 1.0), (-0.2, 4.0), (0.1, 0.0), (0.0, 0.5)][:J])


def problem(family, M, D, J, seed):
    """The data recipe of test_glm_dispersion.problem: weights from {0, 0.5, 1, 3} with at least one 0 (M > 1), offsets
    ~ N(0, 0.3), lam_d from {0, 0.5, 4} with lam_0 = 0, mu_d ~ N(0, 0.5); binomial trials in 1 .. 20 for logistic.  The
    groups are drawn from {-1, 0 .. J-1} with every value present; true t_j in [-0.5, 0.5].  Returns the keyword
    arguments of HierarchicalGLM, the true (w, t) and the generator."""
    rs = np.random.RandomState(seed)
    X = rs.standard_normal((M, D)) / np.sqrt(D)
    w = 0.7 * rs.standard_normal(D)
    t = rs.uniform(-0.5, 0.5, size=J)
    a = rs.choice([0.0, 0.5, 1.0, 3.0], size=M)
    if M > 1:
        a[rs.randint(M)] = 0.0
    else:
        a[:] = 3.0
    o = 0.3 * rs.standard_normal(M)
    eta = X @ w + o
    assert np.all(np.abs(eta) < 6.0)
    if family == "logistic":
        n = rs.randint(1, 21, size=M).astype(np.float64)
        y = rs.binomial(n.astype(int), 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    else:
        n = None
        y = rs.poisson(np.exp(eta)).astype(np.float64)
    lam = rs.choice([0.0, 0.5, 4.0], size=D)
    lam[0] = 0.0
    mu = 0.5 * rs.standard_normal(D)
    assert D >= J + 1
    groups = rs.randint(-1, J, size=D)
    groups[rs.permutation(D)[:J + 1]] = np.arange(-1, J)
    kw = dict(X=X, y=y, family=family, groups=groups, log_scale_prior=t_priors(J), weights=a, offset=o, trials=n,
              prior_precision=lam, prior_mean=mu)
    return kw, w, t, rs


def start(w, t, N, rs, spread=0.3):
    """(D + J, N) states around (w, t); every t_j stays in [-2, 2]."""
    q = w[:, None] + spread * rs.standard_normal((w.size, N))
    tq = np.clip(t[:, None] + spread * rs.standard_normal((t.size, N)), -2.0, 2.0)
    return np.ascontiguousarray(np.vstack([q, tq]))


def model_params(kw):
    """prm of SOURCE for the keyword arguments `kw`."""
    X, y, a, o, n = kw["X"], kw["y"], kw["weights"], kw["offset"], kw["trials"]
    M, D = X.shape
    a = np.ones(M) if a is None else a
    o = np.zeros(M) if o is None else o
    n = np.ones(M) if n is None else n
    groups = np.asarray(kw["groups"])
    J = int(groups.max()) + 1
    tp = np.broadcast_to(np.asarray(kw["log_scale_prior"], float), (J, 2))
    lam = np.broadcast_to(np.asarray(kw["prior_precision"], float), (D,))
    mu = np.zeros(D) if kw.get("prior_mean") is None else kw["prior_mean"]
    return np.concatenate([[float(M), float(D)], X.ravel(), a * n, a * y, o, np.r_[lam, tp[:, 1]], np.r_[mu, tp[:, 0]],
                           groups.astype(float)]), D + J


def oracle_pot(kw):
    from physicsbasedbayesianinference_amd import custom
    prm, DT = model_params(kw)
    return orc.pot_custom(custom.complete_source(SOURCE % LINKS[kw["family"]]), DT, prm)


def numpy_U(kw, q):
    """U of one state from the NumPy statement of the model."""
    X, y, a, o, n = kw["X"], kw["y"], kw["weights"], kw["offset"], kw["trials"]
    M, D = X.shape
    n = np.ones(M) if n is None else n
    groups, tp = np.asarray(kw["groups"]), np.asarray(kw["log_scale_prior"], float)
    J = int(groups.max()) + 1
    w, t = q[:D], q[D:]
    eta = X @ w + o
    b = np.logaddexp(0.0, eta) if kw["family"] == "logistic" else np.exp(eta)
    U = np.sum(a * (n * b - y * eta))
    fixed = groups < 0
    U += 0.5 * np.sum(kw["prior_precision"][fixed] * (w[fixed] - kw["prior_mean"][fixed]) ** 2)
    for j in range(J):
        mem = groups == j
        S = np.sum((w[mem] - kw["prior_mean"][mem]) ** 2)
        U += 0.5 * np.exp(-2 * t[j]) * S + mem.sum() * t[j] + 0.5 * tp[j, 1] * (t[j] - tp[j, 0]) ** 2
    return U


# ------------------------------------------------------------------------------------------------ CPU
def test_hier_abi_declared_bound_and_exported():
    names = {"pbbi_potential_create_glm_hier", "pbbi_glm_pack_prior_groups"}
    hdr = open(os.path.join(ROOT, "include", "pbbi.h")).read()
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
    import physicsbasedbayesianinference_amd as pkg
    from physicsbasedbayesianinference_amd import _lib, glm
    assert pkg.HierarchicalGLM is glm.HierarchicalGLM and "HierarchicalGLM" in pkg.__all__
    assert pkg.pack_prior_groups is glm.pack_prior_groups and "pack_prior_groups" in pkg.__all__
    assert names <= set(_lib.PROTOTYPES)
    assert sorted(glm.HIER_MAX_DIM) == ["logistic", "poisson"] and all(64 <= v <= 128 for v in glm.HIER_MAX_DIM.values())
    assert sorted(glm.FAMILIES) == ["logistic", "poisson"]
    lib = _lib.load()
    assert lib.pbbi_version() == 103
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert names <= set(re.findall(r"\bT (pbbi_[a-z0-9_]+)", out))


def test_hier_rejects_bad_arguments_on_the_host():
    from physicsbasedbayesianinference_amd import HierarchicalGLM, glm
    rs = np.random.RandomState(0)
    M, D = 10, 4
    X = rs.standard_normal((M, D))
    yb = rs.randint(0, 2, M).astype(float)
    yc = rs.poisson(2.0, M).astype(float)
    ones, at2 = np.ones(M), np.arange(M) == 2
    g = np.array([-1, 0, 0, 1])
    lo, po = dict(X=X, y=yb, family="logistic", groups=g), dict(X=X, y=yc, family="poisson", groups=g)
    bad = [
        # groups
        (dict(lo, groups=g[:3]), "groups"), (dict(lo, groups=np.r_[g, 0]), "groups"), (dict(lo, groups=g.reshape(2, 2)), "groups"),
        (dict(lo, groups=None), "groups"), (dict(lo, groups=np.array([-1, 0, 0, 4])), "groups"),
        (dict(lo, groups=np.array([-2, 0, 0, 1])), "-1"), (dict(lo, groups=np.array([-1, 0, 0, 2])), "must be used"),
        (dict(lo, groups=np.array([-1, 1, 1, 1])), "must be used"), (dict(lo, groups=np.array([-1, 0.5, 0, 1])), "integers"),
        (dict(lo, groups=np.full(D, -1)), "GLM"),
        (dict(X=np.ones((M, 6)), y=yb, groups=np.array([-1, 0, 1, 2, 3, 4])), "at most 4"),                   # J = 5
        # D + J above HIER_MAX_DIM
        (dict(X=np.ones((4, 64)), y=np.zeros(4), family="poisson", groups=np.zeros(64, int)), "state dimension"),
        (dict(X=np.ones((4, 61)), y=np.zeros(4), family="logistic", groups=np.arange(61) % 4), "state dimension"),
        (dict(X=np.ones((4, 129)), y=np.zeros(4), family="poisson", groups=np.zeros(129, int)), "D <="),
        # precisions
        (dict(lo, prior_precision=-1.0), "prior_precision"), (dict(lo, prior_precision=np.array([-1.0, 1, 1, 1])), "prior_precision"),
        (dict(lo, prior_precision=np.array([np.nan, 1, 1, 1])), "prior_precision"), (dict(lo, prior_precision=np.inf), "prior_precision"),
        (dict(lo, prior_precision=np.ones(D + 1)), "prior_precision"), (dict(lo, prior_precision=np.ones((D, 1))), "prior_precision"),
        (dict(lo, prior_mean=np.zeros(D - 1)), "prior_mean"), (dict(lo, prior_mean=np.array([0, np.nan, 0, 0])), "prior_mean"),
        # log_scale_prior
        (dict(lo, log_scale_prior=(0.0,)), "log_scale_prior"), (dict(lo, log_scale_prior=0.25), "log_scale_prior"),
        (dict(lo, log_scale_prior=[(0, 1), (0, 1), (0, 1)]), "log_scale_prior"), (dict(lo, log_scale_prior=(0.0, -0.1)), "log_scale_prior"),
        (dict(lo, log_scale_prior=(np.nan, 1.0)), "log_scale_prior"), (dict(lo, log_scale_prior=[(0, 1), (0, np.inf)]), "log_scale_prior"),
        (dict(lo, log_scale_prior="wide"), "log_scale_prior"),
        # dtype and family
        (dict(lo, dtype="float32"), "float64"), (dict(po, dtype="float32"), "float64"),
        (dict(lo, family="gaussian"), "family"), (dict(lo, family="negbinomial"), "family"),
        # every rejection GLM makes for X, y, weights, offset and trials
        (dict(lo, X=X[:9]), "rows"), (dict(lo, X=X.ravel()), "2-D"), (dict(lo, y=yb.reshape(M, 1)), "1-D"),
        (dict(lo, X=np.where(np.arange(D) == 1, np.nan, X)), "finite"), (dict(po, y=np.where(at2, np.inf, yc)), "finite"),
        (dict(lo, y=yb + 0.5), "logistic"), (dict(lo, y=yc + 2.0), "logistic"), (dict(po, y=yc + 0.25), "poisson"),
        (dict(po, y=-yc - 1.0), "poisson"),
        (dict(lo, weights=ones[:9]), "weights"), (dict(lo, weights=ones.reshape(1, M)), "weights"),
        (dict(lo, weights=np.where(at2, np.nan, ones)), "weights"), (dict(lo, weights=np.where(at2, -0.5, ones)), "weights"),
        (dict(po, offset=np.zeros(M + 1)), "offset"), (dict(po, offset=0.0), "offset"), (dict(po, offset=np.where(at2, np.inf, 0.0)), "offset"),
        (dict(po, trials=ones), "trials"), (dict(lo, trials=ones[:9]), "trials"), (dict(lo, trials=0.5 * ones), "trials"),
        (dict(lo, trials=np.where(at2, 0.0, ones)), "trials"), (dict(lo, y=3 * yb, trials=2 * ones), "trials"),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            HierarchicalGLM(**kw)
        print("refused:", sorted(set(kw) - {"X", "y"}), msg)
    # the entries of grouped coefficients are ignored: a value no fixed row may have passes there
    lam, n = glm.pack_prior_groups(g, prior_precision=np.array([1.0, np.nan, -3.0, np.inf]))
    assert np.array_equal(lam[0, :D + 2], [1.0, -1.0, -1.0, -2.0, 1.0, 1.0]) and np.array_equal(n, [2.0, 1.0])
    # the C entry points state the same rules (host only: nothing here reaches a device)
    from physicsbasedbayesianinference_amd import _lib
    L = _lib.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lamv, tp, out, nout = np.ones(D), np.array([0.0, 1.0] * 5), np.zeros(256), np.zeros(4)

    def pack(groups, J, lam=lamv, tpv=tp, Dn=D):
        gi = np.ascontiguousarray(groups, dtype=np.int32)
        return L.pbbi_glm_pack_prior_groups(Dn, J, lam.ctypes.data_as(dp), None, gi.ctypes.data_as(ip), tpv.ctypes.data_as(dp),
                                            out.ctypes.data_as(dp), nout.ctypes.data_as(dp)), _lib.last_error()
    assert pack(g, 2)[0] == _lib.OK
    for args, code, msg in (((g, 5), _lib.ERR_UNSUPPORTED, "1 .. 4"), ((g, 0), _lib.ERR_UNSUPPORTED, "1 .. 4"),
                            ((g, 3), _lib.ERR_INVALID, "must be used"), (([-1, 0, 0, 2], 2), _lib.ERR_INVALID, "0 .. J-1"),
                            (([-2, 0, 0, 1], 2), _lib.ERR_INVALID, "0 .. J-1"),
                            ((g, 2, np.array([-1.0, 1, 1, 1])), _lib.ERR_INVALID, "prior_precision"),
                            ((g, 2, lamv, np.array([0.0, -1.0, 0.0, 1.0])), _lib.ERR_INVALID, "log_scale_prior"),
                            ((np.zeros(128, int), 1, np.ones(128), tp, 128), _lib.ERR_UNSUPPORTED, "<= 128")):
        rc, err = pack(*args)
        assert rc == code and msg in err, (rc, err)
    h = C.c_void_p()
    Xb, yb2, gb = np.ones((4, 63)), np.zeros(4), np.zeros(63, dtype=np.int32)
    for fam in (0, 1):
        rc = L.pbbi_potential_create_glm_hier(63, 4, Xb.ctypes.data_as(dp), yb2.ctypes.data_as(dp), fam, None, None, None,
                                              np.ones(63).ctypes.data_as(dp), None, gb.ctypes.data_as(ip), 2,
                                              tp.ctypes.data_as(dp), _lib.F64, 0, C.byref(h))
        assert rc == _lib.ERR_INVALID and "must be used" in _lib.last_error() and not h
        gb2 = np.r_[np.zeros(62, dtype=np.int32), np.int32(1)]
        rc = L.pbbi_potential_create_glm_hier(63, 4, Xb.ctypes.data_as(dp), yb2.ctypes.data_as(dp), fam, None, None, None,
                                              np.ones(63).ctypes.data_as(dp), None, gb2.ctypes.data_as(ip), 2,
                                              tp.ctypes.data_as(dp), _lib.F64, 0, C.byref(h))
        assert rc == _lib.ERR_UNSUPPORTED and "<= 64" in _lib.last_error() and not h
        rc = L.pbbi_potential_create_glm_hier(4, 4, Xb.ctypes.data_as(dp), yb2.ctypes.data_as(dp), fam, None, None, None,
                                              np.ones(4).ctypes.data_as(dp), None, np.ascontiguousarray(g, np.int32).ctypes.data_as(ip),
                                              2, tp.ctypes.data_as(dp), _lib.F32, 0, C.byref(h))
        assert rc == _lib.ERR_UNSUPPORTED and "float64" in _lib.last_error() and not h
    rc = L.pbbi_potential_create_glm_hier(4, 4, Xb.ctypes.data_as(dp), yb2.ctypes.data_as(dp), 3, None, None, None,
                                          np.ones(4).ctypes.data_as(dp), None, np.ascontiguousarray(g, np.int32).ctypes.data_as(ip), 2,
                                          tp.ctypes.data_as(dp), _lib.F64, 0, C.byref(h))
    assert rc == _lib.ERR_INVALID and not h


def interleaved(D, J, single=False, all_grouped=False):
    """Groups cycling with an odd period P (J + 1 or J + 2): -1, 0, 1, .. J-1 (, J-1).  Rows of one residue mod P step
    through the four lane groups (row & 3) and, from D = 60, through several 16-row tiles.  Optionally the last group is
    cut to a single member, or no coefficient is left ungrouped."""
    P = J + 1 if J % 2 == 0 else J + 2
    g = np.minimum(np.arange(D) % P, J) - 1
    if all_grouped:
        g[g < 0] = 0
    if single:
        g[np.flatnonzero(g == J - 1)[1:]] = 0 if all_grouped or J > 1 else -1
    return g


PACK_CASES = [(D, J, False, False) for D in (3, 14, 15, 16, 60) for J in (1, 2, 4) if D >= J + 1] + \
             [(14, 2, True, False), (60, 4, True, False), (16, 4, False, True), (60, 2, False, True), (3, 1, False, True)]


@pytest.mark.parametrize("D,J,single,all_grouped", PACK_CASES)
def test_pack_prior_groups_matches_numpy(D, J, single, all_grouped):
    from physicsbasedbayesianinference_amd import glm
    rs = np.random.RandomState(100 * D + J)
    g = interleaved(D, J, single, all_grouped)
    lam, mu, tp = rs.choice([0.0, 0.5, 4.0], size=D), rs.standard_normal(D), t_priors(J)
    table, n = glm.pack_prior_groups(g, tp, lam, mu)
    DP = glm.padded_dim(D + J)
    assert table.shape == (2, DP) and n.shape == (J,)
    want = np.zeros((2, DP))
    want[0, :D] = np.where(g < 0, lam, -(g + 1.0))
    want[1, :D] = mu
    want[0, D:D + J], want[1, D:D + J] = tp[:, 1], tp[:, 0]
    assert np.array_equal(table, want)
    assert np.array_equal(n, [np.sum(g == j) for j in range(J)])
    if single:
        assert n[J - 1] == 1
    if all_grouped:
        assert not (g < 0).any()
    rows = np.flatnonzero(g == 0)
    if len(rows) >= 5:              # one group's rows in all four lane groups; at D = 60 in more than one 16-row tile
        assert set(rows & 3) == {0, 1, 2, 3}
        assert D < 60 or len(set(rows >> 4)) > 1
    one, _ = glm.pack_prior_groups(g, tuple(tp[0]), lam, mu)      # one pair serves all groups
    assert np.array_equal(one[:, D:D + J], np.tile(tp[0][::-1, None], (1, J)))


@pytest.mark.parametrize("D,J", [(3, 1), (5, 2), (14, 2), (15, 2), (16, 1), (28, 4), (60, 4)])
def test_hier_lane_walk_replay(D, J):
    """A NumPy replay of what a wave does with the packed table: lane (g, c), register s holds row 4 s + g; the owner
    compare and the chain sum that hand t_j to all four lane groups, the per-lane group sums and their chain sum, the
    select of tau_j by the sign of the lam slot.  It reproduces the prior part of U and of the gradient from the closed
    form, t rows included, and the image of [X | 0] keeps the likelihood's gradient at exactly 0 on rows D .. D+J-1."""
    from physicsbasedbayesianinference_amd import glm
    rs = np.random.RandomState(7 * D + J)
    g_of = rs.randint(-1, J, size=D)
    g_of[rs.permutation(D)[:J + 1]] = np.arange(-1, J)
    lam, mu, tp = rs.choice([0.0, 0.5, 4.0], size=D), rs.standard_normal(D), t_priors(J)
    table, nj = glm.pack_prior_groups(g_of, tp, lam, mu)
    DT, DP = D + J, glm.padded_dim(D + J)
    KS = DP // 4
    state = np.r_[rs.standard_normal(D), rs.uniform(-2, 2, J)]
    lane = np.arange(64)
    g, c = lane >> 4, lane & 15
    q = np.zeros((KS, 64))
    for s in range(KS):
        rows = 4 * s + g
        q[s] = np.where(rows < DT, state[np.minimum(rows, DT - 1)], 0.0)
    plam = np.stack([table[0, 4 * s + g] for s in range(KS)])
    pmu = np.stack([table[1, 4 * s + g] for s in range(KS)])

    def chain_sum(x):
        return np.tile(x.reshape(4, 16).sum(axis=0), 4)
    # broadcast: a lane owns at most one t row, row D + jo in register so
    jo = (g - D) & 3
    so = (D + jo) >> 2
    th = np.array([q[so[ln], ln] if so[ln] < KS else 0.0 for ln in range(64)])
    t = np.zeros((4, 64))
    tau = np.ones((4, 64))
    for j in range(J):
        t[j] = chain_sum(np.where(jo == j, th, 0.0))
        assert np.array_equal(t[j], np.full(64, state[D + j]))
        tau[j] = np.exp(-2.0 * t[j])
    # group sums
    S = np.zeros((4, 64))
    for s in range(KS):
        dq2 = (q[s] - pmu[s]) ** 2
        for j in range(4):
            S[j] += np.where(plam[s] == -(j + 1.0), dq2, 0.0)
    gacc = np.zeros((KS, 64))               # the likelihood's gradient: exactly 0 on the t rows (below), 0 here throughout
    hnt = np.zeros(64)
    gown = np.zeros(64)
    for j in range(J):
        Sj = chain_sum(S[j])
        gown = np.where(jo == j, nj[j] - tau[j] * Sj, gown)
        hnt += nj[j] * t[j]
    for s in range(KS):
        gacc[s] += np.where(s == so, gown, 0.0)
    # precision of each row by the select; energy and gradient
    prec = plam.copy()
    for j in range(4):
        prec = np.where(plam == -(j + 1.0), tau[j][None, :], prec)
    qq = np.sum(prec * (q - pmu) ** 2, axis=0)
    U = 0.5 * chain_sum(qq) + hnt
    grad = prec * (q - pmu) + gacc
    # closed form
    w, tt = state[:D], state[D:]
    fixed = g_of < 0
    Uc = 0.5 * np.sum(lam[fixed] * (w[fixed] - mu[fixed]) ** 2)
    gc = np.zeros(DT)
    gc[:D][fixed] = lam[fixed] * (w[fixed] - mu[fixed])
    for j in range(J):
        mem = g_of == j
        Sj = np.sum((w[mem] - mu[mem]) ** 2)
        Uc += 0.5 * np.exp(-2 * tt[j]) * Sj + mem.sum() * tt[j] + 0.5 * tp[j, 1] * (tt[j] - tp[j, 0]) ** 2
        gc[:D][mem] = np.exp(-2 * tt[j]) * (w[mem] - mu[mem])
        gc[D + j] = mem.sum() - np.exp(-2 * tt[j]) * Sj + tp[j, 1] * (tt[j] - tp[j, 0])
    assert np.allclose(U, Uc, rtol=1e-13, atol=1e-13)
    for s in range(KS):
        for ln in range(0, 64, 16):
            row = 4 * s + g[ln]
            want = gc[row] if row < DT else 0.0
            assert abs(grad[s, ln] - want) <= 1e-12 * max(1.0, abs(want)), (row, grad[s, ln], want)
    # the second product on the image of [X | 0]: the g tile's rows D .. D+J-1 meet zero columns whatever the residuals
    M = 37
    X = rs.standard_normal((M, D))
    img = glm.pack_design(np.hstack([X, np.zeros((M, J))]))
    NT = DP // 16
    for b in range((M + 15) // 16):
        P1 = img[b, 0].reshape(KS // 2, 64, 2)
        P2 = img[b, 1].reshape(2, NT, 64, 2)
        for j in range(J):
            row = D + j
            assert not P1[(row >> 2) // 2, g == (row & 3), (row >> 2) % 2].any()         # eta does not see t_j
            assert not P2[:, row >> 4, c == (row & 15), :].any()                          # nor does X^T r reach its row


@pytest.mark.parametrize("family", FAMILY)
def test_hier_oracle_source_is_pinned(family):
    """The yardstick, not the feature: the oracle's U equals the NumPy statement of the model within 1e-12 relative and
    its gradient central differences of its own U within 1e-6 (step 1e-5), at M = 40, D = 5, J = 2."""
    M, D, J, N = 40, 5, 2, 12
    kw, w, t, rs = problem(family, M, D, J, 5)
    q = start(w, t, N, rs)
    op = oracle_pot(kw)
    U, g = orc.potential(op, q, want_grad=True)
    Us = np.array([numpy_U(kw, q[:, n]) for n in range(N)])
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
    assert g.shape[0] == D + J


def test_with_random_intercepts_builds_the_design_on_the_host():
    from physicsbasedbayesianinference_amd import HierarchicalGLM as H
    rs = np.random.RandomState(3)
    M, D = 30, 3
    X = rs.standard_normal((M, D))
    labels = rs.choice(["c", "a", "d", "b"], size=M)
    labels[:4] = ["a", "b", "c", "d"]
    Xh, groups, levels = H.random_intercept_design(X, labels)
    assert list(levels) == ["a", "b", "c", "d"]
    onehot = (labels[:, None] == np.array(["a", "b", "c", "d"])[None, :]).astype(float)
    assert np.array_equal(Xh, np.hstack([X, onehot])) and np.array_equal(groups, [-1, -1, -1, 0, 0, 0, 0])
    # it composes with groups of the caller's: the new group comes after them
    Xh2, groups2, levels2 = H.random_intercept_design(X, np.array([7, 3, 7] * 10), groups=[-1, 0, 1])
    assert list(levels2) == [3, 7] and np.array_equal(groups2, [-1, 0, 1, 2, 2]) and Xh2.shape == (M, D + 2)
    assert np.array_equal(Xh2[:, D:], np.stack([np.array([0.0, 1.0, 0.0] * 10), np.array([1.0, 0.0, 1.0] * 10)], axis=1))
    with pytest.raises(ValueError):
        H.random_intercept_design(X, labels[:-1])
    with pytest.raises(ValueError):
        H.random_intercept_design(X, labels, groups=[-1, 0])
    # the composed arguments reach the constructor's host checks (which run before the device is touched): four groups,
    # the caller's vectors extended over the new columns -- and poisson takes no trials
    with pytest.raises(ValueError, match="trials"):
        H.with_random_intercepts(X, np.zeros(M), labels, groups=[0, 1, 2], log_scale_prior=[(0, 1)] * 4,
                                 prior_precision=np.ones(D), family="poisson", trials=np.ones(M),
                                 prior_mean=np.r_[np.zeros(D - 1), 1.0])
    with pytest.raises(ValueError, match="log_scale_prior"):      # J = 4 here: three pairs are one too few
        H.with_random_intercepts(X, np.zeros(M), labels, groups=[0, 1, 2], log_scale_prior=[(0, 1)] * 3, family="poisson")
    # split: the shapes it promises, on arrays of any trailing shape (the class method needs no device)
    fake = H.__new__(H)
    fake.numCoefficients, fake.numGroups = 5, 2
    s = rs.standard_normal((7, 11, 3))
    w, sc = H.split(fake, s)
    assert w.shape == (5, 11, 3) and sc.shape == (2, 11, 3)
    assert np.array_equal(w, s[:5]) and np.array_equal(sc, np.exp(s[5:7]))
    w, sc = H.split(fake, s[:, 0, 0])
    assert w.shape == (5,) and sc.shape == (2,)
    import torch
    w, sc = H.split(fake, torch.from_numpy(s))
    assert isinstance(sc, torch.Tensor) and tuple(sc.shape) == (2, 11, 3) and np.array_equal(sc.numpy(), np.exp(s[5:7]))


KA_D, KA_N, KA_SEED, KA_H, KA_L, KA_S = 6, 4096, 11, 0.25, 8, 30
KA_TP = np.array([(0.2, 16.0), (-0.3, 16.0)])
KA_GROUPS = np.array([0, 1, 0, 1, 0, 1])
KA_MU = np.array([0.5, -0.25, 1.0, 0.0, -1.5, 0.75])


def known_answer_draws(seed):
    """(D + J, N) draws from the prior: t_j ~ N(m_tj, 1/16), w_d | t ~ N(mu_d, exp(2 t_j))."""
    rs = np.random.RandomState(seed)
    t = KA_TP[:, 0, None] + 0.25 * rs.standard_normal((2, KA_N))
    w = KA_MU[:, None] + np.exp(t[KA_GROUPS]) * rs.standard_normal((KA_D, KA_N))
    return np.ascontiguousarray(np.vstack([w, t]))


def known_answer_check(q):
    """The bounds of the issue, exact because the chains are independent: mean(t_j) within 5 x 0.25 / sqrt(N) of m_tj,
    var(t_j) within 5 x sqrt(2 / N) / 16 of 1/16, mean(w_d) within 5 standard errors of mu_d with Var w_d = exp(2 m_tj +
    1/8)."""
    N = q.shape[1]
    t, w = q[KA_D:], q[:KA_D]
    dev_t = np.abs(t.mean(axis=1) - KA_TP[:, 0]) / (0.25 / np.sqrt(N))
    dev_v = np.abs(t.var(axis=1, ddof=1) - 1 / 16) / (np.sqrt(2.0 / N) / 16)
    sd_w = np.sqrt(np.exp(2 * KA_TP[KA_GROUPS, 0] + 1 / 8))
    dev_w = np.abs(w.mean(axis=1) - KA_MU) / (sd_w / np.sqrt(N))
    print("deviations in standard errors: mean t", dev_t, "var t", dev_v, "mean w", dev_w)
    assert np.all(dev_t <= 5.0) and np.all(dev_v <= 5.0) and np.all(dev_w <= 5.0)


def test_hier_known_answer_bounds_hold_for_fresh_prior_draws():
    known_answer_check(known_answer_draws(KA_SEED))
    known_answer_check(known_answer_draws(KA_SEED + 1))


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


N_HIER = 100   # six full wave tiles and one of 4 chains; the second workgroup has one ghost wave


def eval_shapes(family):
    from physicsbasedbayesianinference_amd import glm
    shapes = [(1, 3, 1), (40, 5, 2), (40, 14, 2), (40, 15, 2), (203, 16, 1), (203, 28, 4), (1000, 60, 4)]
    if glm.HIER_MAX_DIM[family] > 64:
        shapes.append((203, glm.HIER_MAX_DIM[family] - 4, 4))
    return shapes


def _eval_cases():
    try:
        return [(f,) + s for f in FAMILY for s in eval_shapes(f)]
    except (ImportError, AttributeError):      # the names do not exist: the CPU tests say so
        return [(f, 1, 3, 1) for f in FAMILY]


@pytest.mark.gpu
@pytest.mark.parametrize("family,M,D,J", _eval_cases())
def test_hier_eval_matches_oracle(P, lib, family, M, D, J):
    kw, w, t, rs = problem(family, M, D, J, 7 * M + D)
    assert M == 1 or (kw["weights"] == 0).any()
    pot, op = P.HierarchicalGLM(**kw), oracle_pot(kw)
    assert pot.numDimensions == D + J and pot.numCoefficients == D and pot.numGroups == J
    assert np.array_equal(pot.groups, kw["groups"])
    q = start(w, t, N_HIER, rs)
    assert np.all(np.abs(q[D:]) <= 2.0) and np.all(np.abs(kw["X"] @ q[:D] + kw["offset"][:, None]) < 6.0)
    Uo, go = orc.potential(op, q, want_grad=True)
    U, g = device_eval(lib, pot, q)
    check(f"U {family} {M}x{D}+{J}", U, Uo)
    check(f"grad {family} {M}x{D}+{J}", g, go)
    check("t rows", g[D:], go[D:])
    check("call", pot(q), Uo)                           # the class API (ldn == N)
    check("gradient", pot.gradient(q), go)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILY)
@pytest.mark.parametrize("M,D,J", [(40, 5, 2), (203, 15, 2), (203, 28, 4)])
def test_hier_held_equals_fixed(P, lib, family, M, D, J):
    """Device against device, the new kernel against the existing RICH one: at states whose t rows hold constants c_j the
    gradient rows < D are those of GLM with exp(-2 c_j) on the grouped coefficients, and U differs by sum_j [n_j c_j +
    0.5 lam_tj (c_j - m_tj)^2]."""
    kw, w, t, rs = problem(family, M, D, J, 3 * M + D)
    cj = np.array([0.4, -1.1, 1.7, -0.3])[:J]
    q = start(w, t, N_HIER, rs)
    q[D:] = cj[:, None]
    groups, tp = kw["groups"], kw["log_scale_prior"]
    lam = np.where(groups < 0, kw["prior_precision"], np.exp(-2.0 * cj)[np.maximum(groups, 0)])
    fixed = P.GLM(kw["X"], kw["y"], family=family, prior_precision=lam, prior_mean=kw["prior_mean"], weights=kw["weights"],
                  offset=kw["offset"], trials=kw["trials"])
    Uh, gh = device_eval(lib, P.HierarchicalGLM(**kw), q)
    Uf, gf = device_eval(lib, fixed, np.ascontiguousarray(q[:D]))
    nj = np.array([np.sum(groups == j) for j in range(J)])
    check("U", Uh, Uf + np.sum(nj * cj + 0.5 * tp[:, 1] * (cj - tp[:, 0]) ** 2))
    check("grad", gh[:D], gf)


# family, M, D, J, h (Leapfrog), h (Stormer-Verlet), L -- N = 303; both h from the oracle alone (see the module text): at
# each the reject fraction lies in [0.1, 0.9] for all four combinations of mass and kT
ITER_CASES = [("logistic", 40, 5, 2, 0.2, 0.15, 8), ("poisson", 203, 15, 2, 0.18, 0.05, 8)]
ITER_SEED = 11


def iter_inputs(family, M, D, J, mass, kt):
    kw, w, t, rs = problem(family, M, D, J, ITER_SEED)
    N = 303
    kT = 2.0 if kt else 1.0
    m = 1.0 + (np.arange(N) % 3) * 0.5 if mass else None
    q = start(w, t, N, rs, spread=0.1)
    p = np.ascontiguousarray(rs.standard_normal((D + J, N)) * np.sqrt((m if mass else 1.0) * kT))
    u = rs.uniform(size=N)
    return kw, N, kT, m, q, p, u


@pytest.mark.gpu
@pytest.mark.parametrize("family,M,D,J,h_lf,h_sv,L", ITER_CASES)
@pytest.mark.parametrize("method", ["Leapfrog", "Stormer-Verlet"])
@pytest.mark.parametrize("mass", [False, True])
@pytest.mark.parametrize("kt", [False, True])
def test_hier_uploaded_draw_iteration_matches_oracle(P, lib, family, M, D, J, h_lf, h_sv, L, method, mass, kt):
    import torch
    h = h_lf if method == "Leapfrog" else h_sv
    d = _dev()
    kw, N, kT, m, q, p, u = iter_inputs(family, M, D, J, mass, kt)
    Dt = D + J
    pot, op = P.HierarchicalGLM(**kw), oracle_pot(kw)
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


# family, M, D, J, N, h, L -- S = 3
RUN_CASES = [("logistic", 203, 15, 2, 300, 0.16, 8), ("poisson", 1000, 60, 4, 200, 0.2, 8)]
RUN_SEED, RUN_ITER0, RUN_CHAIN0, RUN_S, RUN_DATA = 17, 3, 1000003, 3, 21


@pytest.mark.gpu
@pytest.mark.parametrize("family,M,D,J,N,h,L", RUN_CASES)
def test_hier_philox_run_matches_oracle(P, lib, family, M, D, J, N, h, L):
    """pbbi_hmc_run, PBBI_DRAW_F64: the oracle draws its own momenta of the (D + J, N) state (no device draw is replayed)."""
    import torch
    d = _dev()
    kw, w, t, rs = problem(family, M, D, J, RUN_DATA)
    q = start(w, t, N, rs, spread=0.1)
    pot = P.HierarchicalGLM(**kw)
    Dt, S = D + J, RUN_S
    ldn = N + 5
    qd = padded(q, ldn)
    samples, momenta = d.empty((S, Dt, N), np.float64, 0), d.empty((S, Dt, N), np.float64, 0)
    rej, ratio = d.empty((S, N), np.uint8, 0), d.empty((S, N), np.float64, 0)
    flags = lib.COMPAT_P_FROM_OLDQ | lib.DRAW_F64
    lib.call("pbbi_hmc_run", pot.handle, 0, qd.data_ptr(), None, samples.data_ptr(), momenta.data_ptr(), rej.data_ptr(),
             ratio.data_ptr(), N, ldn, h, L, S, flags, RUN_SEED, RUN_ITER0, RUN_CHAIN0, 1.0, d.stream_ptr(0))
    torch.cuda.synchronize()
    so, mo, rejo, ro = orc.hmc_run_philox(oracle_pot(kw), "Leapfrog", q, None, h, L, S, RUN_SEED, RUN_ITER0, RUN_CHAIN0, 1.0,
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
def test_hier_run_equals_runs_of_one_bit_for_bit(P, lib, method):
    """A run of S = 21 equals 21 runs of one, bit for bit; the burn-in form (samples_out = NULL) ends in the same state."""
    import torch
    d = _dev()
    family, M, D, J, h = ("logistic", 203, 15, 2, 0.06) if method == 0 else ("poisson", 203, 28, 4, 0.03)
    kw, w, t, rs = problem(family, M, D, J, 31)
    pot = P.HierarchicalGLM(**kw)
    Dt = D + J
    N, L, S, seed, chain0, iter0 = 333, 4, 21, 8, 5, 2
    m = 1.0 + (np.arange(N) % 3) * 0.5
    md = d.as_device(m, 0, np.float64)
    st = d.stream_ptr(0)
    q0 = start(w, t, N, rs, spread=0.1)

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
def test_hier_integrators_match_oracle(P, lib, family):
    """pbbi_leapfrog / pbbi_stormer_verlet / pbbi_integrate (v_out) in place, with masses."""
    import torch
    d = _dev()
    M, D, J, N, h, L = 203, 15, 2, 131, 0.02, 7
    kw, w, t, rs = problem(family, M, D, J, 51)
    pot, op = P.HierarchicalGLM(**kw), oracle_pot(kw)
    Dt = D + J
    m = 1.0 + (np.arange(N) % 3) * 0.5
    for method in ("Leapfrog", "Stormer-Verlet"):
        for entry in ("pbbi_integrate", "pbbi_leapfrog" if method == "Leapfrog" else "pbbi_stormer_verlet"):
            q, p = start(w, t, N, rs, spread=0.1), np.ascontiguousarray(rs.standard_normal((Dt, N)))
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
def test_hier_through_the_classes(P, lib, rng, N):
    """HMC(...).getSamples on a HierarchicalGLM and on the same model as a CustomPotential (how it ran before): equal
    masks, samples and momenta to TOL."""
    from scipy.constants import k as kB
    M, D, J, S = 203, 15, 2, 4
    kw, w, t, rs = problem("logistic", M, D, J, 71)
    pot = P.HierarchicalGLM(**kw)
    prm, DT = model_params(kw)
    plug = P.CustomPotential(DT, SOURCE % LINKS["logistic"], prm)
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


@pytest.mark.gpu
def test_hier_smc_and_unsupported_calls(P, lib):
    """TemperedSMC accepts the potential; per-chain lengths and GIST are refused as on every GLM handle; describeRun
    names the kernel."""
    from physicsbasedbayesianinference_amd.smc import TemperedSMC
    d = _dev()
    M, D, J, N, S = 203, 5, 2, 64, 2
    kw, w, t, rs = problem("logistic", M, D, J, 81)
    pot = P.HierarchicalGLM.with_random_intercepts(kw["X"], kw["y"], np.arange(M) % 3, family="logistic", groups=kw["groups"],
                                                   log_scale_prior=(0.0, 4.0), prior_precision=kw["prior_precision"],
                                                   prior_mean=kw["prior_mean"], weights=kw["weights"], offset=kw["offset"],
                                                   trials=kw["trials"])
    Dt = D + 3 + J + 1
    assert pot.numDimensions == Dt and pot.numGroups == J + 1 and list(pot.levels) == [0, 1, 2]
    # a fixed, short schedule: kT = 1 / beta stays below 4, so the moves (5 steps of 0.05) keep every t_j near its start
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
    assert "k_glm" in text and "hierarchical" in text and "iterations per launch: up to 1" in text
    hmc = P.HMC(P.Ensemble(Dt, N), 0.45, 0.05, None, potential=pot, rng="philox", seed=13, verbose=False)
    if hasattr(hmc, "describeRun"):
        assert "k_glm" in hmc.describeRun(S)


@pytest.mark.gpu
def test_hier_known_answer_the_prior(P, lib):
    """X = 0, one observation: the likelihood is constant and the posterior is the prior.  N = 4096 chains start from prior
    draws (NumPy), so they are stationary from the first iteration; after 30 iterations with the philox draw each chain's
    final state is tested against the prior's moments within the exact standard errors (known_answer_check).  The step
    size gives an accept rate in [0.6, 0.95] (chosen on the CPU with the oracle)."""
    import torch
    d = _dev()
    pot = P.HierarchicalGLM(np.zeros((1, KA_D)), np.zeros(1), family="poisson", groups=KA_GROUPS, log_scale_prior=KA_TP,
                            prior_mean=KA_MU)
    q0 = known_answer_draws(KA_SEED)
    N, Dt = KA_N, KA_D + 2
    qd = d.as_device(q0, 0, np.float64)
    rej = d.empty((KA_S, N), np.uint8, 0)
    lib.call("pbbi_hmc_run", pot.handle, 0, qd.data_ptr(), None, None, None, rej.data_ptr(), None, N, N, KA_H, KA_L, KA_S,
             lib.COMPAT_P_FROM_OLDQ, 2024, 0, 0, 1.0, d.stream_ptr(0))
    torch.cuda.synchronize()
    acc = 1.0 - float(d.to_numpy(rej).mean())
    q = d.to_numpy(qd)
    print("accept rate", acc)
    assert np.all(np.isfinite(q)) and 0.6 <= acc <= 0.95, acc
    assert not np.array_equal(q, q0)
    known_answer_check(q)
