"""The full GLM model (glm.py, csrc/kernels_glm.hip, the RICH instantiations of k_glm): observation weights a_i,
offsets o_i, binomial trials n_i and a prior per coefficient,

    U(w) = sum_i a_i [ n_i b(eta_i) - y_i eta_i ] + 0.5 sum_d lam_d (w_d - mu_d)^2,    eta_i = x_i . w + o_i.

The oracle side is the user-source mechanism, `orc.pot_custom(complete_source(SOURCE), D, prm)`, with this file's own
statement of the model: prm = [M, X.ravel(), c, d, o, lam(D), mu(D)], c = a n, d = a y (formed here with NumPy), a
row with c = d = 0 skipped by a branch.

Tolerance: 1e-10 relative to max(1, max|oracle|) -- the project's figure for these models, the `rel` / `check` of
test_glm.py; reject masks are compared for equality.  Step sizes and seeds of the sampling tests were chosen on the
CPU, from the oracle alone, so that both outcomes occur and no chain's accept test rests on rounding; both
preconditions are asserted on the oracle's values.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10

SOURCE = """
PBBI_FN T b0(T z) { return %(b0)s; }
PBBI_FN T b1(T z) { return %(b1)s; }
template <class Q>
PBBI_FN T potential(const Q& q, int D, const T* prm) {
    const int M = (int)prm[0];
    const T* X = prm + 1;
    const T* c = X + (long)M * D;
    const T* d = c + M;
    const T* o = d + M;
    const T* lam = o + M;
    const T* mu = lam + D;
    T s = 0;
    for (int i = 0; i < M; ++i) {
        if (c[i] == 0 && d[i] == 0) continue;   // weight 0: the row is not there
        T z = o[i];
        for (int j = 0; j < D; ++j) z += X[i * D + j] * q[j];
        s += c[i] * b0(z) - d[i] * z;
    }
    T r = 0;
    for (int j = 0; j < D; ++j) r += lam[j] * (q[j] - mu[j]) * (q[j] - mu[j]);
    return s + T(0.5) * r;
}
template <class Q, class G>
PBBI_FN void gradient(const Q& q, G& g, int D, const T* prm) {
    const int M = (int)prm[0];
    const T* X = prm + 1;
    const T* c = X + (long)M * D;
    const T* d = c + M;
    const T* o = d + M;
    const T* lam = o + M;
    const T* mu = lam + D;
    for (int j = 0; j < D; ++j) g[j] = lam[j] * (q[j] - mu[j]);
    for (int i = 0; i < M; ++i) {
        if (c[i] == 0 && d[i] == 0) continue;
        T z = o[i];
        for (int j = 0; j < D; ++j) z += X[i * D + j] * q[j];
        const T w = c[i] * b1(z) - d[i];
        for (int j = 0; j < D; ++j) g[j] += w * X[i * D + j];
    }
}
"""
LINKS = {"logistic": dict(b0="(z > 0 ? z : T(0)) + log1p(exp(-fabs(z)))", b1="T(1) / (T(1) + exp(-z))"),
         "poisson": dict(b0="exp(z)", b1="exp(z)")}


def problem(family, M, D, seed):
    """The data of every GPU test: weights from {0, 0.5, 1, 3} with at least one 0, offsets ~ N(0, 0.3), trials in
    1..20 (logistic), lam_d from {0, 0.5, 4} with lam_0 = 0, mu_d ~ N(0, 0.5)."""
    rs = np.random.RandomState(seed)
    X = rs.standard_normal((M, D)) / np.sqrt(D)
    w = rs.standard_normal(D)
    a = rs.choice([0.0, 0.5, 1.0, 3.0], size=M)
    a[rs.randint(M)] = 0.0
    o = 0.3 * rs.standard_normal(M)
    eta = X @ w + o
    if family == "logistic":
        n = rs.randint(1, 21, size=M).astype(np.float64)
        y = rs.binomial(n.astype(int), 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    else:
        n = None
        y = rs.poisson(np.exp(eta)).astype(np.float64)
    lam = rs.choice([0.0, 0.5, 4.0], size=D)
    lam[0] = 0.0
    mu = 0.5 * rs.standard_normal(D)
    return dict(X=X, y=y, family=family, weights=a, offset=o, trials=n, prior_precision=lam, prior_mean=mu), w, rs


def start(w, N, rs, spread=0.3):
    return np.ascontiguousarray(w[:, None] + spread * rs.standard_normal((w.size, N)))


def oracle_pot(kw, keep=None):
    """The oracle's potential of the data `kw` (the keyword arguments of GLM); keep = a row mask."""
    from physicsbasedbayesianinference_amd import custom
    X, y, a, o, n = kw["X"], kw["y"], kw["weights"], kw["offset"], kw["trials"]
    n = np.ones_like(y) if n is None else n
    c, d = a * n, a * y
    if keep is not None:
        X, c, d, o = X[keep], c[keep], d[keep], o[keep]
    prm = np.concatenate([[float(X.shape[0])], X.ravel(), c, d, o, kw["prior_precision"], kw["prior_mean"]])
    return orc.pot_custom(custom.complete_source(SOURCE % LINKS[kw["family"]]), X.shape[1], prm)


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


def decisive(ratio, u, rej, lo, hi):
    """The two preconditions of a mask comparison, on the oracle's values: both outcomes occur (reject fraction in
    [lo, hi]) and no chain's accept test is decided by rounding."""
    frac = float(np.mean(rej))
    margin = float(np.min(np.abs(ratio - u) / np.maximum(1.0, ratio)))
    print("reject fraction", frac, "closest accept test", margin)
    assert np.all(np.isfinite(ratio))
    assert lo <= frac <= hi, frac
    assert margin > 1e-8, margin


# ------------------------------------------------------------------------------------------------ CPU
def test_glm_model_abi_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pbbi.h")).read()
    assert re.search(r"\bpbbi_potential_create_glm_ex\s*\(", hdr)
    assert re.search(r"\bpbbi_glm_pack_observations\s*\(", hdr)
    from physicsbasedbayesianinference_amd import _lib
    assert {"pbbi_potential_create_glm_ex", "pbbi_glm_pack_observations"} <= set(_lib.PROTOTYPES)
    lib = _lib.load()
    assert lib.pbbi_version() == 103
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (pbbi_[a-z0-9_]+)", out))
    assert {"pbbi_potential_create_glm_ex", "pbbi_glm_pack_observations", "pbbi_potential_create_glm"} <= exported


@pytest.mark.parametrize("family", ["logistic", "poisson"])
@pytest.mark.parametrize("M", [1, 16, 203])
def test_pack_observations_matches_numpy(M, family):
    from physicsbasedbayesianinference_amd import glm
    kw, _, rs = problem(family, M, 3, 100 * M + len(family))
    y, a, o, n = kw["y"], kw["weights"], kw["offset"], kw["trials"]
    length = ((M + 15) // 16 + 3) // 4 * 4 * 16     # ceil(ceil(M / 16) / 4) * 4 * 16
    out = glm.pack_observations(y, family, weights=a, offset=o, trials=n)
    assert out.shape == (3, length)
    assert np.array_equal(out[0, :M], a * (n if n is not None else 1.0))
    assert np.array_equal(out[1, :M], a * y)
    assert np.array_equal(out[2, :M], o)
    assert not out[:, M:].any()
    # the defaults: weights 1, offset 0, trials 1
    y1 = np.minimum(y, 1.0) if family == "logistic" else y
    out = glm.pack_observations(y1, family)
    assert out.shape == (3, length)
    assert np.array_equal(out[0, :M], np.ones(M)) and np.array_equal(out[1, :M], y1) and not out[2].any()
    assert not out[:, M:].any()
    # the helper checks what the constructor of the handle checks
    with pytest.raises(ValueError):
        glm.pack_observations(y, family, weights=-np.ones(M))
    with pytest.raises(ValueError):
        glm.pack_observations(y + 21.0, "logistic", trials=np.full(M, 20.0))
    with pytest.raises(ValueError):
        glm.pack_observations(y, "poisson", trials=np.ones(M))


def test_glm_model_rejects_bad_arguments_on_the_host():
    from physicsbasedbayesianinference_amd import GLM
    rs = np.random.RandomState(0)
    M, D = 10, 3
    X = rs.standard_normal((M, D))
    n = rs.randint(1, 6, size=M).astype(float)
    yb = np.floor(rs.uniform(size=M) * (n + 1))
    yc = rs.poisson(2.0, M).astype(float)
    ones, at2 = np.ones(M), np.arange(M) == 2
    bad = [
        dict(X=X, y=yb, trials=n[:9]),                                     # shapes (M,)
        dict(X=X, y=yb, trials=n.reshape(M, 1)),
        dict(X=X, y=yc, family="poisson", weights=ones[:9]),
        dict(X=X, y=yc, family="poisson", weights=ones.reshape(1, M)),
        dict(X=X, y=yc, family="poisson", offset=np.zeros(M + 1)),
        dict(X=X, y=yc, family="poisson", offset=0.0),
        dict(X=X, y=yb, trials=n, prior_precision=np.ones(D + 1)),         # shapes (D,)
        dict(X=X, y=yb, trials=n, prior_precision=np.ones((D, 1))),
        dict(X=X, y=yb, trials=n, prior_mean=np.zeros(D - 1)),
        dict(X=X, y=yb, trials=n, prior_mean=0.0),
        dict(X=X, y=yb, trials=n, weights=np.where(at2, np.nan, ones)),    # all values finite
        dict(X=X, y=yb, trials=n, weights=np.where(at2, np.inf, ones)),
        dict(X=X, y=yc, family="poisson", offset=np.where(at2, np.nan, 0.0)),
        dict(X=X, y=yc, family="poisson", offset=np.where(at2, -np.inf, 0.0)),
        dict(X=X, y=yb, trials=np.where(at2, np.inf, n)),
        dict(X=X, y=yb, trials=n, prior_precision=np.array([1.0, np.nan, 1.0])),
        dict(X=X, y=yb, trials=n, prior_precision=np.array([1.0, np.inf, 1.0])),
        dict(X=X, y=yb, trials=n, prior_mean=np.array([0.0, np.nan, 0.0])),
        dict(X=X, y=yb, trials=n, weights=np.where(at2, -0.5, ones)),      # weights >= 0
        dict(X=X, y=yb, trials=n + 0.5),                                   # trials integral
        dict(X=X, y=np.zeros(M), trials=np.where(at2, 0.0, n)),            # ... and >= 1
        dict(X=X, y=yc, family="poisson", trials=ones),                    # ... and only with logistic
        dict(X=X, y=np.where(at2, n + 1.0, yb), trials=n),                 # 0 <= y <= trials
        dict(X=X, y=np.where(at2, -1.0, yb), trials=n),
        dict(X=X, y=np.where(at2, 0.5, yb), trials=n),                     # ... integral
        dict(X=X, y=np.full(M, 2.0), weights=ones),                        # without trials y stays in {0, 1}
        dict(X=X, y=-yc - 1.0, family="poisson", offset=np.zeros(M)),      # Poisson y as now
        dict(X=X, y=yc + 0.25, family="poisson", weights=ones),
        dict(X=X, y=yb, trials=n, prior_precision=np.array([1.0, -1.0, 1.0])),   # each precision >= 0
        dict(X=X, y=yb, trials=n, family="gaussian"),
        dict(X=X, y=yb, trials=n, dtype="float32"),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            GLM(**kw)
        print("refused:", sorted(set(kw) - {"X", "y"}))


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


def device_eval(lib, pot, q, pad=7):
    """pbbi_potential_eval on a padded leading stride: U (N,), gradient (D, N); nothing is stored past N."""
    import torch
    D, N = q.shape
    ldn = N + pad
    qd = padded(q, ldn)
    U = torch.full((N,), -7.0, dtype=torch.float64, device="cuda:0")
    gd = torch.full((D, ldn), -7.0, dtype=torch.float64, device="cuda:0")
    lib.call("pbbi_potential_eval", pot.handle, qd.data_ptr(), N, ldn, U.data_ptr(), gd.data_ptr(), _dev().stream_ptr(0))
    torch.cuda.synchronize()
    assert np.all(gd[:, N:].cpu().numpy() == -7.0), "stores past N"
    return U.cpu().numpy(), gd[:, :N].cpu().numpy()


N_EVAL = 83   # five full wave tiles and one of 3 chains; the second workgroup has two ghost waves


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["logistic", "poisson"])
@pytest.mark.parametrize("M,D", [(1, 1), (40, 5), (203, 5), (1000, 50), (4096, 128)])
def test_glm_model_eval_matches_oracle(P, lib, family, M, D):
    kw, w, rs = problem(family, M, D, 7 * M + D)
    assert (kw["weights"] == 0).any() and kw["prior_precision"][0] == 0
    pot, op = P.GLM(**kw), oracle_pot(kw)
    q = start(w, N_EVAL, rs)
    Uo, go = orc.potential(op, q, want_grad=True)
    U, g = device_eval(lib, pot, q)
    check(f"U {family} {M}x{D}", U, Uo)
    check(f"grad {family} {M}x{D}", g, go)
    # the class API (ldn == N)
    check("call", pot(q), Uo)
    check("gradient", pot.gradient(q), go)


@pytest.mark.gpu
def test_glm_model_equals_the_plain_path_on_expanded_data(P, lib):
    """Device against device: weights and trials are replicated rows of the plain model."""
    M, D = 40, 5
    rs = np.random.RandomState(3)
    X = rs.standard_normal((M, D)) / np.sqrt(D)
    w = rs.standard_normal(D)
    n = rs.randint(1, 5, size=M)
    a = rs.randint(1, 4, size=M)
    y = rs.binomial(n, 1.0 / (1.0 + np.exp(-(X @ w))))
    rows, ys = [], []
    for i in range(M):
        for _ in range(a[i]):                       # per weight copy: y_i ones and n_i - y_i zeros
            rows += [i] * n[i]
            ys += [1.0] * y[i] + [0.0] * (n[i] - y[i])
    X_rep, y_rep = X[rows], np.array(ys)
    assert X_rep.shape[0] == int((a * n).sum()) and y_rep.sum() == (a * y).sum()
    q = start(w, N_EVAL, rs)
    rich = P.GLM(X, y.astype(float), trials=n.astype(float), weights=a.astype(float), prior_precision=1.0)
    plain = P.GLM(X_rep, y_rep, prior_precision=1.0)
    U, g = device_eval(lib, rich, q)
    Up, gp = device_eval(lib, plain, q)
    check("U compact vs expanded", U, Up)
    check("grad compact vs expanded", g, gp)
    # all-default vectors, a constant lam_d and mu = 0: the plain model on the other kernels
    for family in ("logistic", "poisson"):
        yv = np.minimum(y, 1).astype(float) if family == "logistic" else y.astype(float)
        rich = P.GLM(X, yv, family=family, weights=np.ones(M), offset=np.zeros(M), prior_precision=np.full(D, 1.5),
                     prior_mean=np.zeros(D), **(dict(trials=np.ones(M)) if family == "logistic" else {}))
        plain = P.GLM(X, yv, family=family, prior_precision=1.5)
        U, g = device_eval(lib, rich, q)
        Up, gp = device_eval(lib, plain, q)
        check("U defaults vs plain " + family, U, Up)
        check("grad defaults vs plain " + family, g, gp)


@pytest.mark.gpu
def test_glm_model_zero_weight_under_overflow(P, lib):
    """Poisson: a weight-0 row whose exp(eta) is inf, and a weight-0 row in the ragged last block, are not there."""
    M, D = 33, 3
    kw, w, rs = problem("poisson", M, D, 9)
    q = start(w, N_EVAL, rs, spread=0.01)
    hot, last = 5, M - 1
    kw["X"][hot] = 800.0 * w / (w @ w)
    kw["weights"][[hot, last]] = 0.0
    kw["weights"][[hot + 1, last - 1]] = 3.0
    eta = kw["X"] @ q + kw["offset"][:, None]
    assert np.all(np.abs(eta[hot] - 800.0) < 30.0)
    with np.errstate(over="ignore"):
        assert np.all(np.isinf(np.exp(eta[hot])))
    keep = np.ones(M, bool)
    keep[[hot, last]] = False
    Uo, go = orc.potential(oracle_pot(kw, keep), q, want_grad=True)
    U, g = device_eval(lib, P.GLM(**kw), q)
    assert np.all(np.isfinite(U)) and np.all(np.isfinite(g))
    check("U", U, Uo)
    check("grad", g, go)


@pytest.mark.gpu
def test_glm_model_energies_match_oracle(P, lib):
    """pbbi_energy / pbbi_weights_ratio (the kernel's energy and ratio modes) with per-chain masses."""
    import torch
    d = _dev()
    kw, w, rs = problem("poisson", 300, 8, 6)
    pot, op = P.GLM(**kw), oracle_pot(kw)
    N = N_EVAL
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
    check("weights_ratio", d.to_numpy(ratio), orc.weights_ratio(op, q2, p2, q, p, m))


# family, M, D, h, L -- N = 303
ITER_CASES = [("logistic", 203, 5, 0.12, 8), ("logistic", 512, 16, 0.1, 10), ("poisson", 300, 8, 0.06, 10)]


def iter_inputs(family, M, D, mass, kt):
    kw, w, rs = problem(family, M, D, 11)
    N = 303
    kT = 2.0 if kt else 1.0
    m = 1.0 + (np.arange(N) % 3) * 0.5 if mass else None
    q = start(w, N, rs, spread=0.1)
    p = np.ascontiguousarray(rs.standard_normal((D, N)) * np.sqrt((m if mass else 1.0) * kT))
    u = rs.uniform(size=N)
    return kw, N, kT, m, q, p, u


@pytest.mark.gpu
@pytest.mark.parametrize("family,M,D,h,L", ITER_CASES)
@pytest.mark.parametrize("method", ["Leapfrog", "Stormer-Verlet"])
@pytest.mark.parametrize("mass", [False, True])
@pytest.mark.parametrize("kt", [False, True])
def test_glm_model_uploaded_draw_iteration_matches_oracle(P, lib, family, M, D, h, L, method, mass, kt):
    import torch
    d = _dev()
    kw, N, kT, m, q, p, u = iter_inputs(family, M, D, mass, kt)
    pot, op = P.GLM(**kw), oracle_pot(kw)
    qd, pd, ud = (d.as_device(a, 0, np.float64) for a in (q, p, u))
    md = d.as_device(m, 0, np.float64) if mass else None
    qo, po = d.empty((D, N), np.float64, 0), d.empty((D, N), np.float64, 0)
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
    decisive(r_o, u, rej_o, 1.0 / N, 1.0 - 1.0 / N)     # 0 < reject fraction < 1
    grej = d.to_numpy(rej).astype(bool)
    print("mask mismatches", int((grej != rej_o).sum()), "ratio err", rel(d.to_numpy(ratio), r_o))
    assert np.array_equal(grej, rej_o)
    check("q", d.to_numpy(qo), q)
    check("p", d.to_numpy(po), p)
    check("ratio", d.to_numpy(ratio), r_o)


# family, M, D, N, h, L -- S = 3; the last two are the register-heavy instantiations (DP = 64, 128)
RUN_CASES = [("logistic", 203, 5, 300, 0.12, 8), ("poisson", 300, 8, 300, 0.12, 10),
             ("logistic", 1000, 50, 200, 0.12, 10), ("logistic", 4096, 128, 100, 0.12, 10)]
RUN_SEED, RUN_ITER0, RUN_CHAIN0, RUN_S = 17, 3, 1000003, 3


def run_inputs(family, M, D, N):
    kw, w, rs = problem(family, M, D, 21)
    return kw, start(w, N, rs, spread=0.1)


def run_oracle(kw, q, h, L):
    """orc.hmc_run_philox on q (in place) and the two preconditions, from the oracle's own uniforms."""
    N = q.shape[1]
    so, mo, rejo, ro = orc.hmc_run_philox(oracle_pot(kw), "Leapfrog", q, None, h, L, RUN_S, RUN_SEED, RUN_ITER0,
                                          RUN_CHAIN0, 1.0, compat=orc.COMPAT_P_FROM_OLDQ | orc.DRAW_F64)
    u = np.stack([orc.philox_uniform(RUN_SEED, RUN_ITER0 + i, RUN_CHAIN0, N) for i in range(RUN_S)])
    assert np.all(np.isfinite(so)) and np.all(np.isfinite(mo))
    decisive(ro, u, rejo, 0.05, 0.6)
    return so, mo, rejo, ro


@pytest.mark.gpu
@pytest.mark.parametrize("family,M,D,N,h,L", RUN_CASES)
def test_glm_model_philox_run_matches_oracle(P, lib, family, M, D, N, h, L):
    """pbbi_hmc_run, PBBI_DRAW_F64: the oracle draws its own momenta (no device draw is replayed)."""
    import torch
    d = _dev()
    kw, q = run_inputs(family, M, D, N)
    pot = P.GLM(**kw)
    S = RUN_S
    ldn = N + 5
    qd = padded(q, ldn)
    samples, momenta = d.empty((S, D, N), np.float64, 0), d.empty((S, D, N), np.float64, 0)
    rej, ratio = d.empty((S, N), np.uint8, 0), d.empty((S, N), np.float64, 0)
    flags = lib.COMPAT_P_FROM_OLDQ | lib.DRAW_F64
    lib.call("pbbi_hmc_run", pot.handle, 0, qd.data_ptr(), None, samples.data_ptr(), momenta.data_ptr(), rej.data_ptr(),
             ratio.data_ptr(), N, ldn, h, L, S, flags, RUN_SEED, RUN_ITER0, RUN_CHAIN0, 1.0, d.stream_ptr(0))
    torch.cuda.synchronize()
    so, mo, rejo, ro = run_oracle(kw, q, h, L)
    assert np.array_equal(d.to_numpy(rej).astype(bool), rejo)
    check("samples", d.to_numpy(samples), so)
    check("momenta", d.to_numpy(momenta), mo)
    check("ratio", d.to_numpy(ratio), ro)
    check("final state", qd[:, :N].cpu().numpy(), q)
    assert np.all(qd[:, N:].cpu().numpy() == 1e300), "stores past N"


@pytest.mark.gpu
@pytest.mark.parametrize("family,method", [("logistic", 0), ("logistic", 1), ("poisson", 0)])
def test_glm_model_run_equals_runs_of_one_bit_for_bit(P, lib, family, method):
    import torch
    d = _dev()
    M, D, h = (203, 5, 0.12) if family == "logistic" else (300, 8, 0.06)
    kw, w, rs = problem(family, M, D, 31)
    pot = P.GLM(**kw)
    N, L, S, seed, chain0, iter0 = 333, 4, 7, 8, 5, 2
    m = 1.0 + (np.arange(N) % 3) * 0.5
    md = d.as_device(m, 0, np.float64)
    st = d.stream_ptr(0)
    q0 = start(w, N, rs, spread=0.1)

    def run(s_per_call):
        qd = d.as_device(q0, 0, np.float64)
        samples, momenta = d.empty((S, D, N), np.float64, 0), d.empty((S, D, N), np.float64, 0)
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
def test_glm_model_integrators_match_oracle(P):
    """Leapfrog / StormerVerlet(...).integrate() of the class API on a rich GLM, with per-chain masses."""
    M, D, N, h, L = 203, 5, N_EVAL, 0.05, 7
    kw, w, rs = problem("logistic", M, D, 51)
    pot, op = P.GLM(**kw), oracle_pot(kw)
    m = 1.0 + (np.arange(N) % 3) * 0.5
    for cls, method in ((P.Leapfrog, "Leapfrog"), (P.StormerVerlet, "Stormer-Verlet")):
        q, p = start(w, N, rs, spread=0.1), np.ascontiguousarray(rs.standard_normal((D, N)))
        ens = P.Ensemble(D, N)
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
def test_glm_model_through_the_classes(P, lib):
    """HMC(..., rng="philox").getSamples, TemperedSMC and pbbi_describe_run take a rich GLM; GIST refuses it as it
    refuses the plain one."""
    from scipy.constants import k as kB
    from physicsbasedbayesianinference_amd.smc import TemperedSMC
    kw, w, rs = problem("logistic", 203, 5, 71)
    pot, plain = P.GLM(**kw), P.GLM(kw["X"], np.minimum(kw["y"], 1.0))
    for name in ("weights", "offset", "trials", "prior_precision", "prior_mean"):
        assert np.array_equal(getattr(pot, name), kw[name])
        assert getattr(plain, name) is None or name == "prior_precision"
    assert plain.prior_precision == 1.0
    hmc = P.HMC(P.Ensemble(5, 200), 0.8, 0.1, None, potential=pot, rng="philox", seed=13, verbose=False)
    s, m = hmc.getSamples(4, 1 / kB, 1.0)
    assert np.asarray(s).shape == (5, 200, 4) and np.all(np.isfinite(np.asarray(s))) and np.all(np.isfinite(np.asarray(m)))
    errs = []
    for target in (pot, plain):
        with pytest.raises(lib.PbbiError) as e:
            P.HMC(P.Ensemble(5, 64), 0.8, 0.1, None, potential=target, rng="philox", seed=13,
                  verbose=False).getSamplesGIST(2, 1 / kB, 1.0)
        errs.append((e.value.code, str(e.value)))
    assert errs[0] == errs[1] and errs[0][0] == lib.ERR_UNSUPPORTED
    smc = TemperedSMC(pot, 5, 2048, 1.0, 0.2, 2.0, seed=3)
    q = smc.run()
    assert smc.betas[-1] == 1.0 and np.isfinite(smc.logZ)
    assert np.all(np.isfinite(np.asarray(q.cpu() if hasattr(q, "cpu") else q)))
    buf = C.create_string_buffer(1024)
    lib.call("pbbi_describe_run", pot.handle, 0, 64, 64, 4, 2, lib.COMPAT_P_FROM_OLDQ, buf, 1024)
    text = buf.value.decode()
    print(text)
    assert "k_glm" in text and "iterations per launch: up to 1" in text
    assert all(term in text for term in ("weights", "offset", "trials", "per-coefficient prior precision", "prior mean"))
    lib.call("pbbi_describe_run", plain.handle, 0, 64, 64, 4, 2, lib.COMPAT_P_FROM_OLDQ, buf, 1024)
    assert "plain model" in buf.value.decode() and "weights" not in buf.value.decode()
