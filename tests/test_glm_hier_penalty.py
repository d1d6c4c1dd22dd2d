"""Structured group priors (glm.HierarchicalGLM(penalty=...), csrc/kernels_glm.hip: k_glm<NT, FAM, true, GLM_HIER_Q>).
The centred hierarchical model with a symmetric PSD matrix in each group's quadratic form; d_j = (w_d - mu_d) over the
members of group j in increasing column order, r_j = rank(Q_j):

    U(w, t) = sum_i a_i [ n_i b(eta_i) - y_i eta_i ] + 0.5 sum_{d: groups_d < 0} lam_d (w_d - mu_d)^2
            + sum_j [ 0.5 exp(-2 t_j) d_j^T Q_j d_j + r_j t_j + 0.5 lam_tj (t_j - m_tj)^2 ]

The oracle side is the user-source mechanism, `orc.pot_custom(complete_source(SOURCE), D + J, prm)`, with this file's own
C++ statement of the model: prm = [M, D, X.ravel(), c, d, o, lam(D + J), mu(D + J), groups(D), Q(D x D), rank(J)], Q the
full matrix in coefficient indexing (identity on exchangeable groups), potential and gradient written out.

Tolerance: `rel` / `check` of test_glm_model.py, 1e-10 relative to max(1, max|oracle|); reject masks are compared for
equality under its `decisive` preconditions (asserted on the oracle's values).  Step sizes and seeds of the sampling tests
were chosen on the CPU from the oracle alone.  The data keeps |eta| < 6, every t_j in [-2, 2] and |Q| entries <= 10.

Penalties: RW2 (rank n - 2), ICAR on a ring (rank n - 1), a dense full-rank A^T A / n + 0.1 I, None (identity); which group
gets which rotates with `mix`, every problem has at least one fixed row.  A group too small for a kind (RW2 needs 3 members, a
ring 3) gets the dense matrix.
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
    const T* P = grp + D;
    const T* rank = P + (long)D * D;
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
            T pe = 0;                             // row j of Q (w - mu), over the members of j's group
            for (int l = 0; l < D; ++l)
                if ((int)grp[l] == k) pe += P[j * D + l] * (q[l] - mu[l]);
            r += exp(-2 * q[D + k]) * e * pe;
        }
    }
    for (int j = D; j < DT; ++j) {
        r += lam[j] * (q[j] - mu[j]) * (q[j] - mu[j]);
        s += rank[j - D] * q[j];                  // the normaliser of a rank-r_j Gaussian of scale exp(t_j)
    }
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
    const T* P = grp + D;
    const T* rank = P + (long)D * D;
    for (int j = D; j < DT; ++j) g[j] = rank[j - D] + lam[j] * (q[j] - mu[j]);
    for (int j = 0; j < D; ++j) {
        const int k = (int)grp[j];
        const T e = q[j] - mu[j];
        if (k < 0) {
            g[j] = lam[j] * e;
        } else {
            T pe = 0;
            for (int l = 0; l < D; ++l)
                if ((int)grp[l] == k) pe += P[j * D + l] * (q[l] - mu[l]);
            const T tau = exp(-2 * q[D + k]);
            g[j] = tau * pe;
            g[D + k] -= tau * e * pe;
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
KINDS = ("rw2", "icar", "dense", None)


def t_priors(J):
    """J pairs (mean, precision) of the log-scales: all different, one flat."""
    return np.array([(0.3, 1.0), (-0.2, 4.0), (0.1, 0.0), (0.0, 0.5)][:J])


def ring(n):
    A = np.zeros((n, n))
    i = np.arange(n)
    A[i, (i + 1) % n] = A[(i + 1) % n, i] = 1.0
    return A


def make_penalty(kind, n, rs):
    """(Q or None, rank) of one group of n members; a group too small for `kind` gets the dense full-rank matrix."""
    from physicsbasedbayesianinference_amd import HierarchicalGLM as H
    if kind is None:
        return None, n
    if kind == "rw2" and n >= 3:
        return H.random_walk_penalty(n, 2), n - 2
    if kind == "icar" and n >= 3:
        return H.icar_penalty(ring(n)), n - 1
    A = rs.standard_normal((n, n))
    return A.T @ A / n + 0.1 * np.eye(n), n


def problem(family, M, D, J, seed, mix=0, identity=False):
    """The data recipe of test_glm_hier.problem (weights from {0, 0.5, 1, 3} with at least one 0 for M > 1, offsets ~ N(0,
    0.3), lam_d from {0, 0.5, 4} with lam_0 = 0, mu_d ~ N(0, 0.5), binomial trials in 1 .. 20 for logistic, groups from
    {-1, 0 .. J-1} with every value present, so at least one fixed row) plus the penalties: group j gets KINDS[(j + mix) %
    4], or np.eye for every group with `identity`.  Returns the keyword arguments of HierarchicalGLM, the true (w, t) and
    the generator."""
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
    assert (groups < 0).any()
    penalty, rank = [], []
    for j in range(J):
        nj = int(np.sum(groups == j))
        Q, r = (np.eye(nj), nj) if identity else make_penalty(KINDS[(j + mix) % 4], nj, rs)
        assert Q is None or np.max(np.abs(Q)) <= 10.0
        penalty.append(Q)
        rank.append(None if Q is None else r)   # an exchangeable group takes no rank: it is n_j
    kw = dict(X=X, y=y, family=family, groups=groups, log_scale_prior=t_priors(J), weights=a, offset=o, trials=n,
              prior_precision=lam, prior_mean=mu, penalty=penalty, penalty_rank=rank)
    return kw, w, t, rs


def start(w, t, N, rs, spread=0.3):
    """(D + J, N) states around (w, t); every t_j stays in [-2, 2]."""
    q = w[:, None] + spread * rs.standard_normal((w.size, N))
    tq = np.clip(t[:, None] + spread * rs.standard_normal((t.size, N)), -2.0, 2.0)
    return np.ascontiguousarray(np.vstack([q, tq]))


def ranks(kw):
    """r_j of every group: the given rank, n_j for an exchangeable group."""
    groups = np.asarray(kw["groups"])
    return np.array([int(np.sum(groups == j)) if r is None else r for j, r in enumerate(kw["penalty_rank"])])


def full_penalty(kw):
    """The (D, D) matrix in coefficient indexing: Q_j on its group's rows and columns, the identity on exchangeable groups."""
    groups = np.asarray(kw["groups"])
    D = groups.size
    P = np.zeros((D, D))
    for j, Q in enumerate(kw["penalty"]):
        idx = np.flatnonzero(groups == j)
        P[np.ix_(idx, idx)] = np.eye(idx.size) if Q is None else Q
    return P


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
                           groups.astype(float), full_penalty(kw).ravel(), ranks(kw).astype(float)]), D + J


def oracle_pot(kw):
    from physicsbasedbayesianinference_amd import custom
    prm, DT = model_params(kw)
    return orc.pot_custom(custom.complete_source(SOURCE % LINKS[kw["family"]]), DT, prm)


def numpy_U(kw, q):
    """U of one state from the NumPy statement of the model, group by group on the (n_j, n_j) matrices."""
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
        dj = w[mem] - kw["prior_mean"][mem]
        Q = np.eye(mem.sum()) if kw["penalty"][j] is None else kw["penalty"][j]
        U += 0.5 * np.exp(-2 * t[j]) * (dj @ Q @ dj) + ranks(kw)[j] * t[j] + 0.5 * tp[j, 1] * (t[j] - tp[j, 0]) ** 2
    return U


# ------------------------------------------------------------------------------------------------ CPU
def test_penalty_abi_declared_bound_and_exported():
    names = {"pbbi_potential_create_glm_hier_q", "pbbi_glm_pack_penalty"}
    hdr = open(os.path.join(ROOT, "include", "pbbi.h")).read()
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
    from physicsbasedbayesianinference_amd import _lib, glm
    assert names <= set(_lib.PROTOTYPES)
    assert "pack_penalty" in glm.__all__ and "HIER_Q_MAX_DIM" in glm.__all__
    assert glm.HIER_Q_MAX_DIM == {"logistic": 64, "poisson": 64}
    lib = _lib.load()
    assert lib.pbbi_version() == 103
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert names <= set(re.findall(r"\bT (pbbi_[a-z0-9_]+)", out))


def test_penalty_rejects_bad_arguments_on_the_host():
    from physicsbasedbayesianinference_amd import HierarchicalGLM as H, _lib
    rs = np.random.RandomState(0)
    M, D = 10, 6
    X = rs.standard_normal((M, D))
    yb = rs.randint(0, 2, M).astype(float)
    g = np.array([-1, 0, 0, 0, 1, 1])
    Q3, Q2 = H.random_walk_penalty(3, 1), np.array([[2.0, -1.0], [-1.0, 2.0]])
    lo = dict(X=X, y=yb, family="logistic", groups=g)
    asym = Q3.copy()
    asym[0, 1] += 1e-6
    bad = [
        (dict(lo, penalty={0: np.eye(2)}), r"penalty\[0\].*\(3, 3\)"), (dict(lo, penalty={0: np.eye(3).ravel()}), r"penalty\[0\]"),
        (dict(lo, penalty={1: np.eye(3)}), r"penalty\[1\]"), (dict(lo, penalty=[Q3]), "penalty must have one entry per group"),
        (dict(lo, penalty=[Q3, Q2, Q2]), "penalty must have one entry per group"), (dict(lo, penalty=3.0), "penalty must be a dict"),
        (dict(lo, penalty={0: np.where(np.eye(3) > 0, np.nan, 0.0)}), r"penalty\[0\] must be finite"),
        (dict(lo, penalty={1: np.array([[1.0, np.inf], [np.inf, 1.0]])}), r"penalty\[1\] must be finite"),
        (dict(lo, penalty={0: asym}), r"penalty\[0\] must be symmetric"),
        (dict(lo, penalty={1: np.array([[1.0, 2.0], [2.0, 1.0]])}), r"penalty\[1\] must be positive semi-definite"),
        (dict(lo, penalty={0: -Q3}), r"penalty\[0\] must be positive semi-definite"),
        (dict(lo, penalty={0: np.zeros((3, 3))}), r"penalty\[0\] is the zero matrix"),
        (dict(lo, penalty={2: Q2}), "penalty is given for group 2, which is not used"),
        (dict(lo, penalty={-1: Q2}), "penalty is given for group -1, which is not used"),
        (dict(lo, penalty={0: Q3}, penalty_rank={0: 0}), r"penalty_rank\[0\]"), (dict(lo, penalty={0: Q3}, penalty_rank={0: 4}), r"penalty_rank\[0\]"),
        (dict(lo, penalty={0: Q3}, penalty_rank={0: 1.5}), r"penalty_rank\[0\]"), (dict(lo, penalty={0: Q3}, penalty_rank={0: "two"}), r"penalty_rank\[0\]"),
        (dict(lo, penalty={0: Q3}, penalty_rank={1: 2}), r"penalty_rank\[1\] is given for a group without a penalty"),
        (dict(lo, penalty={0: Q3}, penalty_rank={3: 2}), "penalty_rank is given for group 3"),
        (dict(lo, penalty={0: Q3}, penalty_rank=[2]), "penalty_rank must have one entry per group"),
        (dict(lo, penalty_rank={0: 2}), "penalty_rank belongs to a penalty"), (dict(lo, penalty=[None, None], penalty_rank=[2, None]), "penalty_rank belongs to a penalty"),
        (dict(lo, penalty={0: Q3}, parametrisation="noncentred"), "penalty is served by parametrisation=\"centred\" only"),
        (dict(X=np.ones((4, 61)), y=np.zeros(4), family="poisson", groups=np.arange(61) % 4, penalty={0: np.eye(16)}), "state dimension"),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            H(**kw)
        print("refused:", sorted(set(kw) - {"X", "y"}), msg)
    with pytest.raises(ValueError, match="penalty_rank belongs to a penalty"):
        H.with_random_intercepts(X, yb, np.arange(M) % 3, penalty_rank=2)
    with pytest.raises(ValueError, match=r"penalty\[0\].*\(3, 3\)"):       # the new group of three levels is group 0 here
        H.with_random_intercepts(X, yb, np.arange(M) % 3, penalty=np.eye(4))
    with pytest.raises(ValueError, match=r"penalty\[1\].*\(3, 3\)"):       # ... and group 1 after one of the caller's
        H.with_random_intercepts(X, yb, np.arange(M) % 3, groups=[-1, 0, 0, 0, -1, -1], penalty=np.eye(2))
    # penalty=None (or None for every group) constructs the object attributes the class had before: the host checks pass and
    # the first thing that fails without a GPU is the device (the same for both spellings, after the same host work)
    import torch
    if not torch.cuda.is_available():
        for extra in (dict(), dict(penalty=None), dict(penalty=[None, None]), dict(penalty={})):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                H(**dict(lo, **extra))
        with pytest.raises(RuntimeError, match="no CPU fallback"):         # a valid penalty passes every host check too
            H(**dict(lo, penalty={0: Q3, 1: Q2}, penalty_rank={0: 2}))
    # the C entry point states the same rules (host only: every refusal comes before anything is allocated)
    L = _lib.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    gi = np.ascontiguousarray(g, dtype=np.int32)
    tp, lam = np.array([0.0, 1.0] * 4), np.ones(D)
    good = np.zeros((D, D))
    good[1:4, 1:4], good[4:, 4:] = Q3, Q2
    rank = np.array([2.0, 2.0])

    def create(pen, rk, dtype=_lib.F64, Dn=D, groups=gi, Xn=X, J=2, lamv=lam):
        h = C.c_void_p()
        pen = None if pen is None else np.ascontiguousarray(pen)
        rc = L.pbbi_potential_create_glm_hier_q(Dn, Xn.shape[0], Xn.ctypes.data_as(dp), yb[:Xn.shape[0]].ctypes.data_as(dp), 0, None,
                                                None, None, lamv.ctypes.data_as(dp), None, groups.ctypes.data_as(ip), J,
                                                tp.ctypes.data_as(dp), None if pen is None else pen.ctypes.data_as(dp),
                                                None if rk is None else rk.ctypes.data_as(dp), dtype, 0, C.byref(h))
        assert not h
        return rc, _lib.last_error()

    def at(i, k, v):
        out = good.copy()
        out[i, k] = v
        return out
    neg = good.copy()
    neg[4:, 4:] = [[1.0, 2.0], [2.0, 1.0]]
    zero = good.copy()
    zero[4:, 4:] = 0.0
    for pen, rk, code, msg in ((None, rank, _lib.ERR_INVALID, "penalty is NULL"), (good, None, _lib.ERR_INVALID, "penalty_rank is NULL"),
                               (at(1, 2, np.nan), rank, _lib.ERR_INVALID, "penalty must be finite"),
                               (at(0, 0, 1.0), rank, _lib.ERR_INVALID, "zero on fixed rows"), (at(1, 4, 0.5), rank, _lib.ERR_INVALID, "between different groups"),
                               (at(1, 2, -1.0 + 1e-6), rank, _lib.ERR_INVALID, "penalty must be symmetric"),
                               (neg, rank, _lib.ERR_INVALID, "penalty must be positive semi-definite"), (zero, rank, _lib.ERR_INVALID, "zero matrix"),
                               (good, np.array([2.0, 3.0]), _lib.ERR_INVALID, "penalty_rank"), (good, np.array([0.0, 2.0]), _lib.ERR_INVALID, "penalty_rank"),
                               (good, np.array([1.5, 2.0]), _lib.ERR_INVALID, "penalty_rank"),
                               (good, rank, _lib.ERR_UNSUPPORTED, "float64")):
        rc, err = create(pen, rk, dtype=_lib.F32 if msg == "float64" else _lib.F64)
        assert rc == code and msg in err, (rc, err, msg)
    Db = 63
    rc, err = create(np.eye(Db), np.array([62.0, 1.0]), Dn=Db, groups=np.r_[np.zeros(62, np.int32), np.int32(1)], Xn=np.ones((4, Db)),
                     lamv=np.ones(Db))
    assert rc == _lib.ERR_UNSUPPORTED and "<= 64" in err, (rc, err)
    n = C.c_int64()
    assert L.pbbi_glm_pack_penalty(D, 2, None, None, 0, C.byref(n)) == _lib.OK and n.value == 16 * 16
    assert L.pbbi_glm_pack_penalty(60, 4, None, None, 0, C.byref(n)) == _lib.OK and n.value == 64 * 64
    out = np.zeros(256)
    for args, msg in (((D, 0, good.ctypes.data_as(dp), out.ctypes.data_as(dp), 256, None), "1 <= J <= 4"),
                      ((D, 2, None, out.ctypes.data_as(dp), 256, None), "penalty is NULL"),
                      ((D, 2, good.ctypes.data_as(dp), out.ctypes.data_as(dp), 255, None), "shorter")):
        assert L.pbbi_glm_pack_penalty(*args) == _lib.ERR_INVALID and msg in _lib.last_error(), _lib.last_error()


def test_penalty_helpers_known_answers():
    from physicsbasedbayesianinference_amd import HierarchicalGLM as H
    for n in (3, 5, 12):
        Q1 = H.random_walk_penalty(n, 1)
        want = 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
        want[0, 0] = want[-1, -1] = 1.0
        assert np.array_equal(Q1, want) and np.array_equal(Q1, H.random_walk_penalty(n))
        assert not (Q1 @ np.ones(n)).any() and np.linalg.matrix_rank(Q1) == n - 1
        Q2 = H.random_walk_penalty(n, 2)
        assert np.array_equal(Q2, Q2.T) and not np.triu(Q2, 3).any()                   # pentadiagonal
        assert not (Q2 @ np.ones(n)).any() and not (Q2 @ np.arange(n)).any() and np.linalg.matrix_rank(Q2) == n - 2
        if n >= 5:
            assert np.array_equal(Q2[2, :5], [1.0, -4.0, 6.0, -4.0, 1.0]) and np.array_equal(Q2[0, :3], [1.0, -2.0, 1.0])
            assert np.array_equal(Q2[1, :4], [-2.0, 5.0, -4.0, 1.0])
    for args in ((2, 2), (1, 1), (5, 3), (5, 0), (4.0, 1), (True, 1)):
        with pytest.raises(ValueError, match="random_walk_penalty"):
            H.random_walk_penalty(*args)
    n = 7
    Q = H.icar_penalty(ring(n))
    assert np.array_equal(np.diag(Q), np.full(n, 2.0)) and np.array_equal(Q, Q.T) and not (Q @ np.ones(n)).any()
    assert np.array_equal(Q[0], [2.0, -1.0, 0, 0, 0, 0, -1.0]) and np.linalg.matrix_rank(Q) == n - 1
    two = np.zeros((7, 7))
    two[:3, :3], two[3:, 3:] = ring(3), ring(4)
    Q = H.icar_penalty(two)
    assert np.linalg.matrix_rank(Q) == 7 - 2 and not (Q @ np.ones(7)).any() and not Q[:3, 3:].any()
    assert not (Q @ np.r_[np.ones(3), np.zeros(4)]).any()                              # one null vector per component
    path = np.eye(4, k=1) + np.eye(4, k=-1)
    assert np.array_equal(H.icar_penalty(path), H.random_walk_penalty(4, 1))            # a path graph is RW1
    iso = ring(5)
    iso[4, :] = iso[:, 4] = 0.0
    asym = ring(5)
    asym[0, 1] = 0.0
    loop = ring(5)
    loop[2, 2] = 1.0
    for A, msg in ((iso, "isolated"), (asym, "symmetric"), (loop, "zero diagonal"), (2.0 * ring(5), "0 and 1"), (np.ones((3, 4)), "square"),
                   (np.ones(4), "square")):
        with pytest.raises(ValueError, match=msg):
            H.icar_penalty(A)


def _mfma(A, B, Cacc):
    """v_mfma_f64_16x16x4_f64 on per-lane operands: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15];
    register r of lane l of C/D is element (row (l >> 4) + 4 r, column l & 15)."""
    tile = A.reshape(4, 16).T @ B.reshape(4, 16)   # [i][j]
    lane = np.arange(64)
    for r in range(4):
        Cacc[:, r] += tile[(lane >> 4) + 4 * r, lane & 15]


@pytest.mark.parametrize("D,J", [(3, 1), (14, 2), (15, 2), (16, 1), (28, 4), (60, 4)])
def test_pack_penalty_lane_walk_replay(D, J):
    """The packed image, pushed through a NumPy emulation of the MFMA lane maps exactly as the kernel walks it (tile t, K-step
    s with register dq[s] as the B operand), reproduces Q @ d in the state layout on integer data (every sum exact).  The B
    operand holds NON-ZERO values on the t rows and the padding rows here: rows and columns >= D of the image are zero, so
    they neither contribute nor receive anything."""
    from physicsbasedbayesianinference_amd import glm
    rs = np.random.RandomState(31 * D + J)
    A = rs.randint(-3, 4, size=(D, D)).astype(np.float64)
    Q = A + A.T                                              # symmetric integers: (Q + Q^T) / 2 is Q exactly
    DP = glm.padded_dim(D + J)
    KS, NT = DP // 4, DP // 16
    img = glm.pack_penalty(Q, J)
    assert img.shape == (NT, KS // 2, 64, 2)
    lane = np.arange(64)
    g, c = lane >> 4, lane & 15
    # the image itself, entry by entry
    Qp = np.zeros((DP, DP))
    Qp[:D, :D] = Q
    for t in range(NT):
        for s2 in range(KS // 2):
            for e in range(2):
                assert np.array_equal(img[t, s2, :, e], Qp[16 * t + c, 4 * (2 * s2 + e) + g])
    # not symmetric on input: the image is that of (Q + Q^T) / 2
    assert np.array_equal(glm.pack_penalty(2.0 * A, J), img)
    dfull = rs.randint(-9, 10, size=(DP, 16)).astype(np.float64)      # rows >= D non-zero on purpose
    assert dfull[D:D + J].any()
    dq = np.stack([dfull[4 * s + g, c] for s in range(KS)])
    want = np.zeros((DP, 16))
    want[:D] = Q @ dfull[:D]
    for t in range(NT):
        qd = np.zeros((64, 4))
        for s2 in range(KS // 2):
            for e in range(2):
                _mfma(img[t, s2, :, e], dq[2 * s2 + e], qd)
        for r in range(4):                                   # register r of tile t = row 16t + 4r + g: the state layout
            assert np.array_equal(qd[:, r], want[16 * t + 4 * r + g, c])
    assert not want[D:].any()


@pytest.mark.parametrize("family", FAMILY)
def test_penalty_oracle_source_is_pinned(family):
    """The yardstick, not the feature: the oracle's U equals the NumPy statement of the model within 1e-12 relative and its
    gradient central differences of its own U within 1e-6 (step 1e-5), at M = 40, D = 14, J = 4 (all four kinds)."""
    M, D, J, N = 40, 14, 4, 12
    kw, w, t, rs = problem(family, M, D, J, 5)
    assert sum(Q is None for Q in kw["penalty"]) == 1
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


# known answer, the prior alone: one group of KA_D members with the dense full-rank Q = L L^T, a proper prior on t, all
# observation weights 0.  z = exp(-t) L^T (w - mu) is N(0, I) under the model whatever t does, t ~ N(m_t, 1 / lam_t).
KA_D, KA_N, KA_SEED, KA_H, KA_L, KA_BURN = 6, 4096, 11, 0.25, 8, 30
KA_TP = np.array([(0.2, 16.0)])
KA_MU = np.array([0.5, -0.25, 1.0, 0.0, -1.5, 0.75])
KA_AUTO = 1.5   # margin for autocorrelation, see known_answer_check


def known_answer_Q():
    rs = np.random.RandomState(3)
    A = rs.standard_normal((KA_D, KA_D))
    Q = A.T @ A / KA_D + 0.1 * np.eye(KA_D)
    return Q, np.linalg.cholesky(Q)


def known_answer_draws(seed):
    """(D + 1, N) i.i.d. draws from the prior: t ~ N(m_t, 1/16), w = mu + exp(t) L^-T z, z ~ N(0, I)."""
    rs = np.random.RandomState(seed)
    _, Lc = known_answer_Q()
    t = KA_TP[0, 0] + 0.25 * rs.standard_normal((1, KA_N))
    w = KA_MU[:, None] + np.exp(t) * np.linalg.solve(Lc.T, rs.standard_normal((KA_D, KA_N)))
    return np.ascontiguousarray(np.vstack([w, t]))


def known_answer_check(q, margin=1.0):
    """Bounds from the direct i.i.d. sampling distribution at the same sample count N, as
    test_hier_known_answer_bounds_hold_for_fresh_prior_draws sets them: the mean of each z component within 5 / sqrt(N) of 0,
    its variance within 5 sqrt(2 / N) of 1, mean(t) within 5 x 0.25 / sqrt(N) of m_t, var(t) within 5 sqrt(2 / N) / 16 of
    1/16.  The chains are independent of each other, and each STARTS from an i.i.d. prior draw, so the ensemble at any
    iteration is an i.i.d. sample of the prior if the kernel leaves it invariant: autocorrelation along a chain does not
    enter an across-chain moment.  `margin` (KA_AUTO = 1.5 on the device) widens the 5 standard errors for what is left:
    the fourth-moment estimate of var's own error and the rejected proposals' ties."""
    N = q.shape[1]
    _, Lc = known_answer_Q()
    t, w = q[KA_D:], q[:KA_D]
    z = np.exp(-t) * (Lc.T @ (w - KA_MU[:, None]))
    dev = dict(mean_z=np.abs(z.mean(axis=1)) / (1.0 / np.sqrt(N)),
               var_z=np.abs(z.var(axis=1, ddof=1) - 1.0) / np.sqrt(2.0 / N),
               mean_t=np.abs(t.mean(axis=1) - KA_TP[:, 0]) / (0.25 / np.sqrt(N)),
               var_t=np.abs(t.var(axis=1, ddof=1) - 1 / 16) / (np.sqrt(2.0 / N) / 16))
    print("deviations in standard errors:", {k: np.round(v, 2) for k, v in dev.items()})
    for k, v in dev.items():
        assert np.all(v <= 5.0 * margin), (k, v)


def test_penalty_known_answer_bounds_hold_for_fresh_prior_draws():
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


N_EVAL = 37   # two full wave tiles and one of 5 chains (a ragged tail); the workgroup's fourth wave is a ghost
EVAL_SHAPES = [(1, 2, 1), (40, 5, 2), (203, 15, 2), (203, 28, 4), (512, 60, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILY)
@pytest.mark.parametrize("M,D,J", EVAL_SHAPES)
def test_penalty_eval_matches_oracle(P, lib, family, M, D, J):
    mix = {(1, 2, 1): 2, (40, 5, 2): 0, (203, 15, 2): 1}.get((M, D, J), 0) + (2 if family == "poisson" and J == 2 else 0)
    kw, w, t, rs = problem(family, M, D, J, 7 * M + D, mix=mix)
    pot, op = P.HierarchicalGLM(**kw), oracle_pot(kw)
    assert pot.numDimensions == D + J and pot.numCoefficients == D and pot.numGroups == J
    assert np.array_equal(pot.penalty_rank, ranks(kw))
    for Q, Qk in zip(pot.penalty, kw["penalty"]):
        assert (Q is None and Qk is None) or np.allclose(Q, Qk, rtol=0, atol=1e-15)
    q = start(w, t, N_EVAL, rs)
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
@pytest.mark.parametrize("M,D,J", [(40, 5, 2), (203, 28, 4)])
def test_penalty_identity_equals_exchangeable(P, lib, family, M, D, J):
    """Device against device: with np.eye for every group the new kernel computes the model of HierarchicalGLM(penalty=None),
    the parent's kernel, to the tolerance (the summation orders differ: not bit for bit)."""
    kw, w, t, rs = problem(family, M, D, J, 3 * M + D, identity=True)
    q = start(w, t, N_EVAL, rs)
    plain = {k: v for k, v in kw.items() if k not in ("penalty", "penalty_rank")}
    new, old = P.HierarchicalGLM(**kw), P.HierarchicalGLM(**plain)
    assert old.penalty is None and old.penalty_rank is None and new.penalty is not None
    buf = C.create_string_buffer(2048)
    for pot, named in ((new, True), (old, False)):
        lib.call("pbbi_describe_run", pot.handle, 0, N_EVAL, N_EVAL, 4, 2, lib.COMPAT_P_FROM_OLDQ, buf, 2048)
        assert ("GLM_HIER_Q" in buf.value.decode()) == named
    Un, gn = device_eval(lib, new, q)
    Uo, go = device_eval(lib, old, q)
    check("U", Un, Uo)
    check("grad", gn, go)


# family, M, D, J, mix, h (Leapfrog), h (Stormer-Verlet), L -- N = 101; both h from the oracle alone (see the module text): at
# each the reject fraction lies in [0.1, 0.9] for all four combinations of mass and kT
ITER_CASES = [("logistic", 40, 5, 2, 0, 0.25, 0.15, 8), ("poisson", 203, 28, 4, 0, 0.2, 0.07, 8), ("logistic", 512, 60, 4, 1, 0.22, 0.1, 6)]
ITER_SEED, ITER_N = 11, 101


def iter_inputs(family, M, D, J, mix, mass, kt):
    kw, w, t, rs = problem(family, M, D, J, ITER_SEED, mix=mix)
    N = ITER_N
    kT = 2.0 if kt else 1.0
    m = 1.0 + (np.arange(N) % 3) * 0.5 if mass else None
    q = start(w, t, N, rs, spread=0.1)
    p = np.ascontiguousarray(rs.standard_normal((D + J, N)) * np.sqrt((m if mass else 1.0) * kT))
    u = rs.uniform(size=N)
    return kw, N, kT, m, q, p, u


@pytest.mark.gpu
@pytest.mark.parametrize("family,M,D,J,mix,h_lf,h_sv,L", ITER_CASES)
@pytest.mark.parametrize("method", ["Leapfrog", "Stormer-Verlet"])
@pytest.mark.parametrize("mass", [False, True])
@pytest.mark.parametrize("kt", [False, True])
def test_penalty_uploaded_draw_iteration_matches_oracle(P, lib, family, M, D, J, mix, h_lf, h_sv, L, method, mass, kt):
    import torch
    h = h_lf if method == "Leapfrog" else h_sv
    d = _dev()
    kw, N, kT, m, q, p, u = iter_inputs(family, M, D, J, mix, mass, kt)
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


# family, M, D, J, mix, N, h, L -- S = 3
RUN_CASES = [("logistic", 203, 15, 2, 0, 150, 0.2, 8), ("poisson", 512, 60, 4, 0, 100, 0.2, 6)]
RUN_SEED, RUN_ITER0, RUN_CHAIN0, RUN_S, RUN_DATA = 17, 3, 1000003, 3, 21


@pytest.mark.gpu
@pytest.mark.parametrize("family,M,D,J,mix,N,h,L", RUN_CASES)
def test_penalty_philox_run_matches_oracle(P, lib, family, M, D, J, mix, N, h, L):
    """pbbi_hmc_run, PBBI_DRAW_F64: the oracle draws its own momenta of the (D + J, N) state (no device draw is replayed)."""
    import torch
    d = _dev()
    kw, w, t, rs = problem(family, M, D, J, RUN_DATA, mix=mix)
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
def test_penalty_run_equals_runs_of_one_bit_for_bit(P, lib, method):
    """A run of S = 9 equals 9 runs of one, bit for bit; the burn-in form (samples_out = NULL) ends in the same state."""
    import torch
    d = _dev()
    family, M, D, J, h = ("logistic", 203, 15, 2, 0.06) if method == 0 else ("poisson", 203, 28, 4, 0.03)
    kw, w, t, rs = problem(family, M, D, J, 31)
    pot = P.HierarchicalGLM(**kw)
    Dt = D + J
    N, L, S, seed, chain0, iter0 = 133, 4, 9, 8, 5, 2
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
def test_penalty_integrators_match_oracle(P, lib, family):
    """pbbi_leapfrog / pbbi_stormer_verlet / pbbi_integrate (v_out) in place, with masses."""
    import torch
    d = _dev()
    M, D, J, N, h, L = 203, 28, 4, 67, 0.02, 7
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
def test_penalty_through_the_classes(P, lib, rng, N):
    """HMC(...).getSamples on the structured potential and on the same model as a CustomPotential (how it had to be written
    before): equal masks, samples and momenta to the tolerance; split returns w and exp(t)."""
    from scipy.constants import k as kB
    M, D, J, S = 203, 15, 2, 3
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
    assert np.array_equal(coef, s[:D])


@pytest.mark.gpu
def test_penalty_smc_ladder_and_unsupported_calls(P, lib):
    """with_random_intercepts(..., penalty=icar) samples; TemperedSMC and TemperingLadder accept the potential; per-chain
    lengths and GIST are refused as on every GLM handle; pbbi_describe_run names the kernel."""
    from scipy.constants import k as kB
    from physicsbasedbayesianinference_amd.smc import TemperedSMC
    from physicsbasedbayesianinference_amd.tempering import TemperingLadder
    d = _dev()
    M, D, J, N, S = 203, 5, 2, 64, 2
    kw, w, t, rs = problem("logistic", M, D, J, 81)
    K = 5
    icar = P.HierarchicalGLM.icar_penalty(ring(K))
    pot = P.HierarchicalGLM.with_random_intercepts(kw["X"], kw["y"], np.arange(M) % K, family="logistic", groups=kw["groups"],
                                                   log_scale_prior=(0.0, 4.0), prior_precision=kw["prior_precision"],
                                                   prior_mean=kw["prior_mean"], weights=kw["weights"], offset=kw["offset"],
                                                   trials=kw["trials"], penalty=icar)
    Dt = D + K + J + 1
    assert pot.numDimensions == Dt and pot.numGroups == J + 1 and list(pot.levels) == list(range(K))
    assert pot.penalty[:J] == [None] * J and np.array_equal(pot.penalty[J], icar)
    assert list(pot.penalty_rank[:J]) == [int(np.sum(kw["groups"] == j)) for j in range(J)] and pot.penalty_rank[J] == K - 1
    hmc = P.HMC(P.Ensemble(Dt, N), 0.45, 0.03, None, potential=pot, rng="philox", seed=13, verbose=False)
    s, _ = hmc.getSamples(4, 1 / kB, 0.3)
    s = np.asarray(s)
    assert s.shape == (Dt, N, 4) and np.all(np.isfinite(s)) and np.asarray(hmc.reject_masks).mean() < 1.0
    coef, scales = pot.split(s)
    assert coef.shape == (D + K, N, 4) and np.array_equal(scales, np.exp(s[D + K:]))
    # a fixed, short schedule: kT = 1 / beta stays below 4, so the moves (5 steps of 0.05) keep every t_j near its start
    smc = TemperedSMC(pot, Dt, 2048, 0.25, 0.05, 0.05, betas=[0.3, 0.6, 1.0], seed=3)
    q = smc.run()
    assert smc.betas[-1] == 1.0 and np.isfinite(smc.logZ)
    assert np.all(np.isfinite(np.asarray(q.cpu() if hasattr(q, "cpu") else q)))
    ladder = TemperingLadder(pot, Dt, 64, [1.0, 1.5, 2.25], simulTime=0.15, stepSize=0.03, seed=5)
    x = np.asarray(ladder.run(numSamples=3, qStd=0.2, swap_every=1, burn_in=2))
    assert x.shape == (Dt, 64, 3) and np.all(np.isfinite(x))
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
    buf = C.create_string_buffer(2048)
    lib.call("pbbi_describe_run", pot.handle, 0, N, N, 4, S, lib.COMPAT_P_FROM_OLDQ, buf, 2048)
    text = buf.value.decode()
    print(text)
    assert "k_glm" in text and "GLM_HIER_Q" in text and "hierarchical" in text and "iterations per launch: up to 1" in text


@pytest.mark.gpu
def test_penalty_known_answer_the_prior(P, lib):
    """All observation weights 0: the posterior is the prior.  N = 4096 chains start from i.i.d. prior draws (NumPy), so the
    ensemble is stationary from the first iteration; after KA_BURN iterations with the philox draw the final states are
    tested as z = exp(-t) L^T (w - mu) and t against the prior's moments (known_answer_check, margin KA_AUTO).  The step size
    gives an accept rate in [0.6, 0.95] (chosen on the CPU with the oracle)."""
    import torch
    d = _dev()
    Q, _ = known_answer_Q()
    M = 4
    X = np.random.RandomState(1).standard_normal((M, KA_D))
    pot = P.HierarchicalGLM(X, np.ones(M), family="poisson", groups=np.zeros(KA_D, int), log_scale_prior=KA_TP,
                            prior_mean=KA_MU, weights=np.zeros(M), penalty={0: Q})
    assert pot.penalty_rank[0] == KA_D
    q0 = known_answer_draws(KA_SEED)
    N = KA_N
    qd = d.as_device(q0, 0, np.float64)
    rej = d.empty((KA_BURN, N), np.uint8, 0)
    lib.call("pbbi_hmc_run", pot.handle, 0, qd.data_ptr(), None, None, None, rej.data_ptr(), None, N, N, KA_H, KA_L, KA_BURN,
             lib.COMPAT_P_FROM_OLDQ, 2024, 0, 0, 1.0, d.stream_ptr(0))
    torch.cuda.synchronize()
    acc = 1.0 - float(d.to_numpy(rej).mean())
    q = d.to_numpy(qd)
    print("accept rate", acc)
    assert np.all(np.isfinite(q)) and 0.6 <= acc <= 0.95, acc
    assert not np.array_equal(q, q0)
    known_answer_check(q, margin=KA_AUTO)
