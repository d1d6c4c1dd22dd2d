"""The Gamma family of glm.DispersionGLM on the device (family="gamma", FAM = 5 of k_glm<NT, FAM, true>, its METRIC twin, k_glm_pw
and k_glm_ll), with the CPU pins of what the GPU tests lean on.  The model, the oracle's C++ statement of it in the natural
form, the data generator and the CPU-only tests are test_glm_gamma_host.py's.

Tolerance: test_glm_model.py's `rel` / `check` with TOL = 1e-10 relative to max(1, max|oracle|); reject masks are compared for
equality under its `decisive` preconditions (asserted on the oracle's values inside each test).  Step sizes and seeds of the
sampling tests were chosen on the CPU from the oracle alone, so that the reject fraction lies in [0.1, 0.9] and no accept
test is closer than 1e-8 (test_gamma_sampling_cases_are_decisive runs every one of them without a GPU).

Shapes: the Gamma kernels ship at every padded dimension the Gaussian's do, so the largest state dimension is 128 (D = 127
sampled, D = 128 held) and test_glm_dispersion.py's EVAL_SHAPES are used whole.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import test_glm_evidence as t_ev
import test_glm_frame as F
import test_glm_metric as t_metric
import test_glm_pointwise as t_pw
import test_glm_power as t_power
from oracle import oracle as orc
from test_glm_dispersion import EVAL_SHAPES, N_DISP, THETA_PRIOR, start
from test_glm_gamma_host import MAX_DIM, make, oracle_pot, problem
from test_glm_model import check, decisive, device_eval, padded, rel

LD = np.longdouble
EVAL_CASES = [(s, M, D) for s in (True, False) for (M, D) in EVAL_SHAPES if D + int(s) <= MAX_DIM]

# M, D, h (Leapfrog), h (Stormer-Verlet), L -- N = 303, theta sampled: at each h the reject fraction lies in [0.1, 0.9] for all
# four combinations of mass and kT
ITER_CASES = [(40, 5, 0.3, 0.1, 8), (203, 16, 0.15, 0.1, 8)]
# sampled, M, D, N, h, L -- S = 6; the last is the largest shipped state dimension
RUN_CASES = [(True, 203, 16, 300, 0.12, 8), (False, 40, 5, 300, 0.35, 8), (True, 203, 127, 100, 0.12, 6)]
RUN_SEED, RUN_ITER0, RUN_CHAIN0, RUN_S = 17, 3, 1000003, 6
# M, D, (h Leapfrog, h Stormer-Verlet), L of the metric's cases (theta sampled; N, masses, kT and counters are test_glm_frame's)
METRIC_CASES = {5: (40, (0.35, 0.15), 8), 16: (203, (0.2, 0.1), 8)}
METRIC_ROWS = [("Leapfrog", True, False), ("Stormer-Verlet", False, True)]     # (method, PBBI_BETA_ACCEPT, compat)
UNIT_H = 0.7      # ... times these steps where the same handle runs with the unit metric


# ---- inputs and oracle sides, computed once and left unchanged -------------------------------------------------------------
def iter_inputs(M, D, mass, kt):
    kw, w, theta, rs = problem(M, D, 11)
    N = 303
    kT = 2.0 if kt else 1.0
    m = 1.0 + (np.arange(N) % 3) * 0.5 if mass else None
    q = start(w, theta, N, rs, spread=0.1)
    p = np.ascontiguousarray(rs.standard_normal((D + 1, N)) * np.sqrt((m if mass else 1.0) * kT))
    u = rs.uniform(size=N)
    return kw, N, kT, m, q, p, u


@functools.lru_cache(maxsize=None)
def iter_oracle(M, D, h, L, method, mass, kt):
    kw, N, kT, m, q, p, u = iter_inputs(M, D, mass, kt)
    r_o, rej_o = orc.hmc_iter(oracle_pot(kw, True), method, q, p, u, m, h, L, beta=1.0 / kT)
    return F._frozen(q=q, p=p, ratio=r_o, rej=rej_o, u=u)


def run_inputs(sampled, M, D, N):
    kw, w, theta, rs = problem(M, D, 21)
    return kw, theta, start(w, theta, N, rs, spread=0.1, sampled=sampled)


@functools.lru_cache(maxsize=None)
def run_oracle(sampled, M, D, N, h, L):
    kw, theta, q = run_inputs(sampled, M, D, N)
    so, mo, rejo, ro = orc.hmc_run_philox(oracle_pot(kw, sampled, theta), "Leapfrog", q, None, h, L, RUN_S, RUN_SEED, RUN_ITER0,
                                          RUN_CHAIN0, 1.0, compat=orc.COMPAT_P_FROM_OLDQ | orc.DRAW_F64)
    u = np.stack([orc.philox_uniform(RUN_SEED, RUN_ITER0 + i, RUN_CHAIN0, N) for i in range(RUN_S)])
    return F._frozen(samples=so, momenta=mo, rej=rejo, ratio=ro, u=u, q=q)


def metric_inputs(D):
    M = METRIC_CASES[D][0]
    kw, w, theta, rs = problem(M, D, 41)
    return kw, start(w, theta, F.N, rs, spread=0.1)


@functools.lru_cache(maxsize=None)
def metric_ref(D, method, beta, compat):
    """test_glm_metric.py's restatement of pbbi_hmc_run under the metric metric_of(Dt), on this file's oracle."""
    M, hs, L = METRIC_CASES[D]
    kw, q = metric_inputs(D)
    q = q.copy()
    s, p, rej, ratio, u = t_metric.r_run(oracle_pot(kw, True), method, q, F.MASS, t_metric.metric_of(D + 1),
                                         hs[F.METHODS.index(method)], L, F.S_RUN, F.SEED, F.ITER0, F.CHAIN0, F.KT, beta, compat)
    return F._frozen(samples=s, momenta=p, rej=rej, ratio=ratio, u=u, q=q)


def pw_case(M, sampled):
    """(kw, theta, spec, slabs (S, Dt, N)) of the draw kernels' tests: D = 5, test_glm_pointwise.py's N and S."""
    kw, w, theta, rs = problem(M, 5, t_pw.DATA_SEED)
    held = None if sampled else float(np.log(np.exp(theta)))
    sp = t_pw.spec_of("gamma", kw, 5, 5 if sampled else -1, held)
    sdn = np.ascontiguousarray(np.stack([start(w, theta, t_pw.N, rs, spread=0.1, sampled=sampled) for _ in range(t_pw.S)]))
    return kw, theta, sp, sdn


def gamma_ref_ll(sp, W):
    """(ll, mu), each (M, T) longdouble, of the draws W (Dt, T) in the natural form of the density -- without the constant
    -a_i log y_i, exactly 0 on a row of weight 0; log Gamma in double (scipy), promoted, as test_glm_pointwise.py does."""
    X, a, y, o = (np.asarray(sp[k]).astype(LD) for k in ("X", "a", "y", "o"))
    Wl = np.asarray(W).astype(LD)
    eta = X @ Wl[:sp["Dx"]] + o[:, None]
    th = Wl[sp["trow"]][None, :] if sp["trow"] >= 0 else LD(sp["theta"])
    alpha = np.exp(th) + 0 * eta
    ll = -a[:, None] * (t_pw.gammaln_ld(alpha) - alpha * np.log(alpha) + alpha * (eta + y[:, None] * np.exp(-eta))
                        - alpha * np.log(y)[:, None])
    ll[np.asarray(sp["a"]) == 0.0] = 0
    return ll, np.exp(eta)


@functools.lru_cache(maxsize=None)
def pw_ref(M, sampled):
    _, _, sp, sdn = pw_case(M, sampled)
    ll, mu = gamma_ref_ll(sp, t_pw.flat(sdn))
    return t_pw.ref_stats(ll, mu) + (ll.sum(axis=0),)


# ---- the evidence's and the known answer's truths --------------------------------------------------------------------------
EV_ALPHA = 2.0


def evidence_problem():
    """M = 20 observations, an intercept and one covariate, offsets, weights 1; prior N(mu_d, 1 / lam_d) with lam = 4: the
    posterior is about a third as wide as the prior, which a Gauss-Hermite rule on the prior's scale resolves at order 150."""
    rs = np.random.RandomState(29)
    M = 20
    X = np.c_[np.ones(M), rs.standard_normal(M)]
    o = 0.3 * rs.standard_normal(M)
    eta = X @ np.array([0.4, -0.6]) + o
    y = rs.gamma(EV_ALPHA, np.exp(eta) / EV_ALPHA)
    return dict(X=X, y=y, family="gamma", offset=o, prior_precision=np.array([4.0, 4.0]), prior_mean=np.array([0.2, -0.1]))


def evidence_truth(kw, order):
    """log of the integral of N(w; mu, diag(1 / lam)) prod_i Gamma(y_i | alpha, mean exp(eta_i)) dw by a tensor Gauss-Hermite
    rule in longdouble (w_d = mu_d + sqrt(2 / lam_d) x)."""
    from scipy.special import gammaln
    x, wq = np.polynomial.hermite.hermgauss(order)
    keep = wq > 1e-300
    x, lw = x[keep].astype(LD), np.log(wq[keep].astype(LD))
    X, y, o = (kw[k].astype(LD) for k in ("X", "y", "offset"))
    lam, mu = kw["prior_precision"].astype(LD), kw["prior_mean"].astype(LD)
    g0, g1 = np.meshgrid(x, x, indexing="ij")
    W = np.stack([mu[0] + np.sqrt(2 / lam[0]) * g0.ravel(), mu[1] + np.sqrt(2 / lam[1]) * g1.ravel()])
    LW = np.add.outer(lw, lw).ravel()
    eta = X @ W + o[:, None]
    a = LD(EV_ALPHA)
    ll = (a * np.log(a) - LD(gammaln(EV_ALPHA)) + (a - 1) * np.log(y)[:, None] - a * (eta + y[:, None] * np.exp(-eta))).sum(axis=0)
    v = LW + ll
    m = v.max()
    return float(m + np.log(np.sum(np.exp(v - m))) - np.log(LD(np.pi)))


def known_answer_problem():
    """Intercept only, alpha held (at 1: exponential regression), weights a_i > 0: exp(-w) ~ Gamma(alpha A, rate alpha S), A =
    sum a_i, S = sum a_i y_i.  alpha A = 24: the posterior's sd is 0.21 around a mean near 0, so starts of N(0, 0.3^2) are
    dispersed (1.5 sd wide) and none sits where exp(-w) makes the one fixed step size unstable (a NumPy replay of this sampler
    leaves no chain stuck for any step from 0.05 to 0.33; at alpha A = 80 it left a handful, whatever computes U)."""
    rs = np.random.RandomState(77)
    M, alpha = 30, 1.0
    a = rs.choice([0.5, 1.0], size=M)
    y = rs.gamma(alpha, 1.0 / alpha, size=M)
    return np.ones((M, 1)), y, a, alpha


# ------------------------------------------------------------------------------------------------ CPU pins
def test_gamma_sampling_cases_are_decisive():
    """Every step size of this file on the oracle alone: both outcomes occur and no accept test hangs on rounding."""
    for M, D, h_lf, h_sv, L in ITER_CASES:
        for method, h in (("Leapfrog", h_lf), ("Stormer-Verlet", h_sv)):
            for mass in (False, True):
                for kt in (False, True):
                    o = iter_oracle(M, D, h, L, method, mass, kt)
                    print(M, D, method, mass, kt)
                    decisive(o["ratio"], o["u"], o["rej"], 0.1, 0.9)
    for case in RUN_CASES:
        o = run_oracle(*case)
        print(case)
        assert np.all(np.isfinite(o["samples"])) and np.all(np.isfinite(o["momenta"]))
        decisive(o["ratio"], o["u"], o["rej"], 0.1, 0.9)
    for D in METRIC_CASES:
        for row in METRIC_ROWS:
            o = metric_ref(D, *row)
            t_metric._margin(str((D,) + row), o["ratio"], o["u"])
            assert 0.1 <= o["rej"].mean() <= 0.9
            # the unit-metric run of the same case (device against device on the GPU) stays finite and decides both ways
            M, hs, L = METRIC_CASES[D]
            kw, q = metric_inputs(D)
            me, b, c = row
            s, _, rej, ratio, _ = t_metric.r_run(oracle_pot(kw, True), me, q.copy(), F.MASS, None, UNIT_H * hs[F.METHODS.index(me)],
                                                 L, F.S_RUN, F.SEED, F.ITER0, F.CHAIN0, F.KT, b, c)
            assert np.all(np.isfinite(s)) and np.all(np.isfinite(ratio)) and 0.05 < rej.mean() < 0.95


def test_gamma_truths_are_what_they_claim():
    kw = evidence_problem()
    t1, t2 = evidence_truth(kw, 150), evidence_truth(kw, 300)
    print("evidence truth", t1, t2)
    assert abs(t1 - t2) < 1e-8
    # the conjugate posterior of the intercept, against a grid: mean and variance of w
    from scipy.special import digamma, polygamma
    X, y, a, alpha = known_answer_problem()
    A, S = a.sum(), (a * y).sum()
    w = np.linspace(-3.0, 4.0, 400001)
    lp = -alpha * (A * w + S * np.exp(-w))          # sum_i a_i alpha (-(w - log y_i) - y_i exp(-w)) + const
    p = np.exp(lp - lp.max())
    p /= p.sum()
    mean = float((p * w).sum())
    var = float((p * (w - mean) ** 2).sum())
    assert abs(mean - (np.log(alpha * S) - digamma(alpha * A))) < 1e-9
    assert abs(var - polygamma(1, alpha * A)) < 1e-9
    # the draw kernels' reference is the SciPy density minus the constant, weights with zeros included
    from scipy import stats
    from physicsbasedbayesianinference_amd import glm
    _, _, sp, sdn = pw_case(40, True)
    Wd = t_pw.flat(sdn)[:, :7]
    ll, mu = (np.asarray(v, dtype=np.float64) for v in gamma_ref_ll(sp, Wd))
    al = np.exp(Wd[5])[None, :]
    full = sp["a"][:, None] * stats.gamma.logpdf(sp["y"][:, None], al, scale=mu / al)
    k = glm.pointwise_constants("gamma", sp["y"], sp["a"])
    check("k (scipy)", np.broadcast_to(k[:, None], ll.shape), full - ll)
    for M in (40, 203):
        for sampled in (True, False):
            assert all(np.all(np.isfinite(v)) for v in pw_ref(M, sampled))


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


@pytest.mark.gpu
@pytest.mark.parametrize("sampled,M,D", EVAL_CASES)
def test_gamma_eval_matches_oracle(P, lib, sampled, M, D):
    kw, w, theta, rs = problem(M, D, 7 * M + D)
    assert M == 1 or (kw["weights"] == 0).any()
    pot, op = make(P, kw, sampled, theta), oracle_pot(kw, sampled, theta)
    assert pot.numDimensions == D + int(sampled)
    q = start(w, theta, N_DISP, rs, sampled=sampled)
    Uo, go = orc.potential(op, q, want_grad=True)
    U, g = device_eval(lib, pot, q)
    check(f"U gamma {M}x{D}", U, Uo)
    check(f"grad gamma {M}x{D}", g, go)
    if sampled:
        check("theta row", g[D], go[D])
    check("call", pot(q), Uo)                           # the class API (ldn == N)
    check("gradient", pot.gradient(q), go)


@pytest.mark.gpu
@pytest.mark.parametrize("M,D", [(40, 5), (203, 15), (203, 16)])
def test_gamma_held_equals_sampled(P, lib, M, D):
    """Device against device: at theta = theta0 the held model is the sampled one without its theta prior and row."""
    kw, w, theta0, rs = problem(M, D, 3 * M + D)
    q = start(w, theta0, N_DISP, rs, sampled=False)
    held, smp = make(P, kw, False, theta0), make(P, kw, True)
    th = float(np.log(np.exp(theta0)))                  # the held model's theta: log of the dispersion it was given
    Uh, gh = device_eval(lib, held, q)
    Us, gs = device_eval(lib, smp, np.ascontiguousarray(np.vstack([q, np.full((1, N_DISP), th)])))
    check("U", Uh, Us - 0.5 * THETA_PRIOR[1] * (th - THETA_PRIOR[0]) ** 2)
    check("grad", gh, gs[:D])


@pytest.mark.gpu
@pytest.mark.parametrize("c", [1000.0, 1e-3])
@pytest.mark.parametrize("sampled", [True, False])
def test_gamma_units_do_not_matter(P, lib, sampled, c):
    """(c y, offset + log c) is the same model: U (the dropped constant a_i log y_i does not enter it) and the gradient."""
    M, D = 203, 16
    kw, w, theta, rs = problem(M, D, 13)
    q = start(w, theta, N_DISP, rs, sampled=sampled)
    U, g = device_eval(lib, make(P, kw, sampled, theta), q)
    kc = dict(kw, y=c * kw["y"], offset=kw["offset"] + np.log(c))
    Uc, gc = device_eval(lib, make(P, kc, sampled, theta), q)
    check(f"U c={c}", Uc, U)
    check(f"grad c={c}", gc, g)


EXPONENTIAL_SOURCE = """
template <class Q>
PBBI_FN T potential(const Q& q, int D, const T* prm) {
    const int M = (int)prm[0];
    const T* X = prm + 1;
    const T* a = X + (long)M * D;
    const T* y = a + M;
    const T* o = y + M;
    const T* lam = o + M;
    const T* mu = lam + D;
    T s = 0;
    for (int i = 0; i < M; ++i) {
        if (a[i] == 0) continue;
        T e = o[i];
        for (int j = 0; j < D; ++j) e += X[i * D + j] * q[j];
        s += a[i] * (e + y[i] * exp(-e) - log(y[i]));          // -log[ (1 / mu) exp(-y / mu) ] - log y
    }
    T r = 0;
    for (int j = 0; j < D; ++j) r += lam[j] * (q[j] - mu[j]) * (q[j] - mu[j]);
    return s + T(0.5) * r;
}
template <class Q, class G>
PBBI_FN void gradient(const Q& q, G& g, int D, const T* prm) {
    const int M = (int)prm[0];
    const T* X = prm + 1;
    const T* a = X + (long)M * D;
    const T* y = a + M;
    const T* o = y + M;
    const T* lam = o + M;
    const T* mu = lam + D;
    for (int j = 0; j < D; ++j) g[j] = lam[j] * (q[j] - mu[j]);
    for (int i = 0; i < M; ++i) {
        if (a[i] == 0) continue;
        T e = o[i];
        for (int j = 0; j < D; ++j) e += X[i * D + j] * q[j];
        const T w = a[i] * (T(1) - y[i] * exp(-e));
        for (int j = 0; j < D; ++j) g[j] += w * X[i * D + j];
    }
}
"""


@pytest.mark.gpu
def test_gamma_shape_one_is_exponential_regression(P, lib):
    from physicsbasedbayesianinference_amd import custom
    M, D = 203, 16
    kw, w, _, rs = problem(M, D, 19)
    kw["y"] = np.clip(rs.exponential(np.exp(kw["X"] @ w + kw["offset"])), 1e-3, None)
    pot = P.DispersionGLM(dispersion=1.0, **kw)
    prm = np.concatenate([[float(M)], kw["X"].ravel(), kw["weights"], kw["y"], kw["offset"], kw["prior_precision"], kw["prior_mean"]])
    op = orc.pot_custom(custom.complete_source(EXPONENTIAL_SOURCE), D, prm)
    q = start(w, 0.0, N_DISP, rs, sampled=False)
    Uo, go = orc.potential(op, q, want_grad=True)
    U, g = device_eval(lib, pot, q)
    check("U exponential", U, Uo)
    check("grad exponential", g, go)


@pytest.mark.gpu
@pytest.mark.parametrize("sampled", [True, False])
def test_gamma_zero_weight_under_overflow(P, lib, sampled):
    """A weight-0 row with eta = -800, whose exp(-z) overflows, and a weight-0 row in the ragged last block, are not there."""
    M, D = 33, 3
    kw, w, theta, rs = problem(M, D, 9)
    q = start(w, theta, N_DISP, rs, spread=0.01, sampled=sampled)
    hot, last = 5, M - 1
    kw["X"][hot] = -800.0 * w / (w @ w)
    kw["weights"][[hot, last]] = 0.0
    kw["weights"][[hot + 1, last - 1]] = 3.0
    eta = kw["X"] @ q[:D] + kw["offset"][:, None]
    assert np.all(np.abs(eta[hot] + 800.0) < 30.0)
    with np.errstate(over="ignore"):
        assert np.all(np.isinf(np.exp(-(eta[hot] - np.log(kw["y"][hot])))))
    keep = np.ones(M, bool)
    keep[[hot, last]] = False
    Uo, go = orc.potential(oracle_pot(kw, sampled, theta, keep), q, want_grad=True)
    U, g = device_eval(lib, make(P, kw, sampled, theta), q)
    assert np.all(np.isfinite(U)) and np.all(np.isfinite(g))
    check("U", U, Uo)
    check("grad", g, go)


@pytest.mark.gpu
@pytest.mark.parametrize("M,D,h_lf,h_sv,L", ITER_CASES)
@pytest.mark.parametrize("method", ["Leapfrog", "Stormer-Verlet"])
@pytest.mark.parametrize("mass", [False, True])
@pytest.mark.parametrize("kt", [False, True])
def test_gamma_uploaded_draw_iteration_matches_oracle(P, lib, M, D, h_lf, h_sv, L, method, mass, kt):
    import torch
    h = h_lf if method == "Leapfrog" else h_sv
    d = _dev()
    kw, N, kT, m, q, p, u = iter_inputs(M, D, mass, kt)
    o = iter_oracle(M, D, h, L, method, mass, kt)
    decisive(o["ratio"], o["u"], o["rej"], 0.1, 0.9)
    Dt = D + 1
    pot = make(P, kw, True)
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
    grej = d.to_numpy(rej).astype(bool)
    print("mask mismatches", int((grej != o["rej"]).sum()), "ratio err", rel(d.to_numpy(ratio), o["ratio"]))
    assert np.array_equal(grej, o["rej"])
    check("q", d.to_numpy(qo), o["q"])
    check("p", d.to_numpy(po), o["p"])
    check("ratio", d.to_numpy(ratio), o["ratio"])


@pytest.mark.gpu
@pytest.mark.parametrize("sampled,M,D,N,h,L", RUN_CASES)
def test_gamma_philox_run_matches_oracle(P, lib, sampled, M, D, N, h, L):
    """pbbi_hmc_run, PBBI_DRAW_F64: the oracle draws its own momenta of the (Dt, N) state (no device draw is replayed)."""
    import torch
    d = _dev()
    kw, theta, q = run_inputs(sampled, M, D, N)
    o = run_oracle(sampled, M, D, N, h, L)
    assert np.all(np.isfinite(o["samples"])) and np.all(np.isfinite(o["momenta"]))
    decisive(o["ratio"], o["u"], o["rej"], 0.1, 0.9)
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
    assert np.array_equal(d.to_numpy(rej).astype(bool), o["rej"])
    check("samples", d.to_numpy(samples), o["samples"])
    check("momenta", d.to_numpy(momenta), o["momenta"])
    check("ratio", d.to_numpy(ratio), o["ratio"])
    check("final state", qd[:, :N].cpu().numpy(), o["q"])
    assert np.all(qd[:, N:].cpu().numpy() == 1e300), "stores past N"


@pytest.mark.gpu
@pytest.mark.parametrize("sampled,method", [(True, 0), (True, 1), (False, 1)])
def test_gamma_run_equals_runs_of_one_bit_for_bit(P, lib, sampled, method):
    import torch
    d = _dev()
    M, D, h = 203, 16, 0.1
    kw, w, theta, rs = problem(M, D, 31)
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
@pytest.mark.parametrize("D", sorted(METRIC_CASES))
def test_gamma_metric_run_vs_restatement(P, lib, D):
    """pbbi_hmc_run on a Gamma handle with a diagonal metric against test_glm_metric.py's restatement (S = 3, kT = 2.5, per-chain
    masses, PBBI_DRAW_F64, leading stride N + 5); a metric of ones is the handle without one bit for bit."""
    M, hs, L = METRIC_CASES[D]
    kw, q0 = metric_inputs(D)
    pot = make(P, kw, True)
    fresh = make(P, kw, True)
    pot.set_metric(t_metric.metric_of(D + 1))
    assert np.array_equal(pot.metric, t_metric.metric_of(D + 1)) and fresh.metric is None
    for method, beta, compat in METRIC_ROWS:
        o = metric_ref(D, method, beta, compat)
        t_metric._margin(str((D, method)), o["ratio"], o["u"])
        h = hs[F.METHODS.index(method)]
        gs, gm, grej, gratio, gq, gpad = F._device_run(lib, pot, method, q0, F.MASS, h, L, F.S_RUN,
                                                       t_metric._flags(lib, beta, compat), F.KT, pad=5)
        tag = f"gamma D={D} {method}"
        assert np.array_equal(grej, o["rej"]), tag
        check(tag + " samples", gs, o["samples"])
        check(tag + " momenta", gm, o["momenta"])
        check(tag + " ratio", gratio, o["ratio"])
        check(tag + " final state", gq, o["q"])
        assert np.all(gpad == F.POISON), tag
    # (without the metric every row is lighter: UNIT_H of the step keeps every chain finite, see the CPU pin)
    want = [F._device_run(lib, fresh, me, q0, F.MASS, UNIT_H * hs[F.METHODS.index(me)], L, F.S_RUN, t_metric._flags(lib, b, c),
                          F.KT, pad=5) for me, b, c in METRIC_ROWS]
    assert all(np.all(np.isfinite(w[0])) for w in want)
    assert any(w[2].any() for w in want) and not all(w[2].all() for w in want)
    pot.set_metric(np.ones(D + 1))
    for (me, b, c), w in zip(METRIC_ROWS, want):
        got = F._device_run(lib, pot, me, q0, F.MASS, UNIT_H * hs[F.METHODS.index(me)], L, F.S_RUN, t_metric._flags(lib, b, c),
                            F.KT, pad=5)
        for tag, a, r in zip(("samples", "momenta", "reject", "ratio", "state", "padding"), got, w):
            assert np.array_equal(a, r), (D, me, tag)


@pytest.mark.gpu
def test_gamma_adapt_mass_matrix(P, lib):
    from scipy.constants import k as kB
    kw, w, theta, _ = problem(203, 5, 41)
    pot = make(P, kw, True)
    hmc = P.HMC(P.Ensemble(6, 512), 1.0, 0.05, None, potential=pot, rng="philox", seed=4, verbose=False, compat=False,
                draw_f64=True)
    m = hmc.adaptMassMatrix(1 / kB, 0.3, windows=(25, 50))
    print("adapted metric", m, "step", hmc.stepSize)
    assert m.shape == (6,) and np.all(np.isfinite(m)) and np.all(m > 0)
    assert np.array_equal(m, pot.metric) and np.isfinite(hmc.stepSize) and hmc.stepSize > 0


@pytest.mark.gpu
@pytest.mark.parametrize("sampled", [True, False])
@pytest.mark.parametrize("M", [40, 203])
def test_gamma_pointwise_and_loglik_match_reference(P, lib, M, sampled):
    """k_glm_pw and k_glm_ll against the longdouble NumPy reduction of the natural-form density, a weight-0 row included."""
    kw, theta, sp, sdn = pw_case(M, sampled)
    lse, mean, var, mu, ulik = pw_ref(M, sampled)
    pot = make(P, kw, sampled, theta)
    got = t_pw.device_pointwise(lib, pot, sdn)
    t_pw.check_all(f"gamma M={M}", got, (lse, mean, var, mu))
    zero = sp["a"] == 0.0
    assert zero.any()
    assert np.all(got[1][zero] == 0.0) and np.all(got[2][zero] == 0.0) and np.all(got[3][zero] != 0.0)
    T = t_pw.N * t_pw.S
    k = -sp["a"].astype(LD) * np.log(sp["y"].astype(LD))
    host = np.ascontiguousarray(sdn.transpose(1, 2, 0))
    r = pot.pointwise(host)
    assert r.T == T
    check("lppd_i", r.lppd_i, lse - np.log(LD(T)) + k)
    check("p_waic_i", r.p_waic_i, var)
    check("mu_i", r.mu_i, mu)
    ref = (k.sum() + ulik).reshape(t_pw.S, t_pw.N).T
    a = pot.loglik(host)
    assert a.shape == (t_pw.N, t_pw.S)
    check("loglik", a, ref)
    pot.set_likelihood_power(0.25)                       # the likelihood is reported at power 1 while the handle is tempered
    assert t_power.same_bits(pot.loglik(host), a)
    check("pointwise sees the power", pot.pointwise(host).mean_ll_i - k, 0.25 * mean)


@pytest.mark.gpu
@pytest.mark.parametrize("beta", t_power.BETAS)
@pytest.mark.parametrize("sampled", [True, False])
def test_gamma_power_equals_fresh_handle_with_scaled_weights(P, lib, sampled, beta):
    kw, w, theta, rs = problem(203, 8, t_power.SEED)
    q0 = start(w, theta, 37, rs, spread=0.1, sampled=sampled)
    tempered = make(P, kw, sampled, theta)
    never = t_power.run(lib, tempered, q0)
    tempered.set_likelihood_power(beta)
    assert tempered.likelihood_power == beta
    a = t_power.run(lib, tempered, q0)
    b = t_power.run(lib, make(P, dict(kw, weights=beta * kw["weights"]), sampled, theta), q0)
    assert np.array_equal(a[1], b[1])
    check(f"run gamma beta={beta}", a[0], b[0])
    assert not t_power.same_bits(a[0], never[0])
    tempered.set_likelihood_power(1.0)
    c = t_power.run(lib, tempered, q0)
    assert t_power.same_bits(c[0], never[0]) and np.array_equal(c[1], never[1])


@pytest.mark.gpu
def test_gamma_sample_prior_is_the_stated_transform(P, lib):
    rs = np.random.RandomState(2)
    M, N, seed = 12, 50, 9
    X = rs.standard_normal((M, 4))
    y = rs.gamma(2.0, 1.0, M)
    lam, mu, dp = np.array([1.0, 4.0, 0.25, 2.0]), np.array([0.5, -1.0, 0.0, 2.0]), (0.1, 2.0)
    for pot, sampled in ((P.DispersionGLM(X, y, family="gamma", dispersion="sample", log_dispersion_prior=dp, prior_precision=lam,
                                          prior_mean=mu), True),
                         (P.DispersionGLM(X, y, family="gamma", dispersion=1.5, prior_precision=lam, prior_mean=mu), False)):
        q = pot.sample_prior(N, seed=seed)
        assert q.is_cuda and tuple(q.shape) == (pot.numDimensions, N)
        z = t_ev.normals(lib, seed, pot.numDimensions, N)
        ref = np.empty_like(z)
        for d in range(4):
            ref[d] = mu[d] + z[d] / np.sqrt(lam[d])
        if sampled:
            ref[4] = dp[0] + z[4] / np.sqrt(dp[1])
        err = np.max(np.abs(q.cpu().numpy() - ref) / np.maximum(1.0, np.abs(ref)))
        print("sample_prior", sampled, err)
        assert err < 1e-14
    with pytest.raises(ValueError):
        P.DispersionGLM(X, y, family="gamma", dispersion=1.5, prior_precision=0.0).sample_prior(N)


@pytest.mark.gpu
def test_gamma_evidence(P):
    """LikelihoodTemperedSMC.logML of a 2-D model with the shape held against the quadrature, test_smc.py's 8-seed rule."""
    kw = evidence_problem()
    zs = t_ev.evidence(P, lambda: P.DispersionGLM(dispersion=EV_ALPHA, **kw), simulTime=1.0, stepSize=0.1, moves=5)
    t_ev.rule(zs, evidence_truth(kw, 150))


@pytest.mark.gpu
def test_gamma_known_answer(P):
    """Intercept only, alpha held, flat prior: exp(-w) ~ Gamma(alpha A, rate alpha S), so E[w] = log(alpha S) - psi(alpha A) and
    Var[w] = trigamma(alpha A).  4096 independent chains, step size from adaptStepSize, 300 iterations of L = 10 of burn-in; the
    mean over the chains of the final state is within 5 standard errors (sd over the chains / sqrt(N)), their variance within
    5 standard errors of trigamma, SE = var sqrt((kurtosis - (N - 3) / (N - 1)) / N) -- var sqrt(2 / (N - 1)) for a normal sample,
    inflated by the sample's own kurtosis."""
    from scipy.constants import k as kB
    from scipy.special import digamma, polygamma
    X, y, a, alpha = known_answer_problem()
    N = 4096
    A, S = a.sum(), (a * y).sum()
    mean_exact, var_exact = np.log(alpha * S) - digamma(alpha * A), float(polygamma(1, alpha * A))
    pot = P.DispersionGLM(X, y, family="gamma", dispersion=alpha, prior_precision=0.0, weights=a)
    q_std = 0.3
    warm = P.HMC(P.Ensemble(1, N), 0.5, 0.05, None, potential=pot, rng="philox", seed=2024, verbose=False)
    h = warm.adaptStepSize(1 / kB, q_std)
    assert 1e-3 < h < 1.0, h
    hmc = P.HMC(P.Ensemble(1, N), 10.5 * h, h, None, potential=pot, rng="philox", seed=2024, verbose=False)
    assert hmc.integrator.numSteps == 10
    s, _ = hmc.getSamples(1, 1 / kB, q_std, burn_in=300)
    last = np.asarray(s)[0, :, 0]
    assert np.all(np.isfinite(last))
    mean, var = last.mean(), last.var(ddof=1)
    kurt = float(np.mean((last - mean) ** 4) / np.mean((last - mean) ** 2) ** 2)
    se_mean = np.sqrt(var / N)
    se_var = var * np.sqrt((kurt - (N - 3) / (N - 1)) / N)
    print("step", h, "accept", hmc.acceptRate, "mean", mean, "exact", mean_exact, "deviation / se", (mean - mean_exact) / se_mean,
          "var", var, "exact", var_exact, "deviation / se", (var - var_exact) / se_var, "kurtosis", kurt)
    assert abs(mean - mean_exact) <= 5.0 * se_mean
    assert abs(var - var_exact) <= 5.0 * se_var


@pytest.mark.gpu
def test_gamma_through_the_classes(P, lib):
    """HMC.getSamples in both rng modes, sampleStats, TemperedSMC and pbbi_describe_run take a Gamma DispersionGLM; split
    returns the coefficients and alpha = exp(theta); GIST refuses it as it refuses GLM."""
    from scipy.constants import k as kB
    from physicsbasedbayesianinference_amd.smc import TemperedSMC
    M, D, N, S = 203, 5, 200, 4
    kw, w, theta, rs = problem(M, D, 71)
    pot, held = make(P, kw, True), make(P, kw, False, theta)
    assert pot.numDimensions == D + 1 and held.numDimensions == D and pot.sampled and not held.sampled
    assert pot.log_dispersion_prior == THETA_PRIOR and held.log_dispersion_prior is None and pot.family == "gamma"
    for rng in ("philox", "numpy"):
        np.random.seed(5)
        hmc = P.HMC(P.Ensemble(D + 1, N), 0.4, 0.05, None, potential=pot, rng=rng, seed=13, verbose=False)
        s, m = hmc.getSamples(S, 1 / kB, 0.3)
        s, m = np.asarray(s), np.asarray(m)
        assert s.shape == (D + 1, N, S) and np.all(np.isfinite(s)) and np.all(np.isfinite(m))
        coef, alpha = pot.split(s)
        assert coef.shape == (D, N, S) and alpha.shape == (N, S)
        assert np.array_equal(coef, s[:D]) and np.array_equal(alpha, np.exp(s[D])) and np.all(alpha > 0)
    sh, _ = P.HMC(P.Ensemble(D, N), 0.4, 0.05, None, potential=held, rng="philox", seed=13, verbose=False).getSamples(S, 1 / kB, 0.3)
    coef, alpha = held.split(np.asarray(sh))
    assert coef.shape == (D, N, S) and alpha == pytest.approx(np.exp(theta), rel=1e-15)
    stats = P.HMC(P.Ensemble(D + 1, N), 0.4, 0.05, None, potential=pot, rng="philox", seed=13,
                  verbose=False).sampleStats(8, 4, 1 / kB, 0.3, burn_in=2, max_lag=2)
    mean, var = stats.moments()[:2]
    mean, var = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (mean, var))
    assert mean.shape[0] == D + 1 and np.all(np.isfinite(mean)) and np.all(np.isfinite(var))
    errs = []
    plain = P.GLM(kw["X"], np.minimum(np.floor(kw["y"]), 1.0))
    for target, dim in ((pot, D + 1), (plain, D)):
        with pytest.raises(lib.PbbiError) as e:
            P.HMC(P.Ensemble(dim, 64), 0.8, 0.1, None, potential=target, rng="philox", seed=13,
                  verbose=False).getSamplesGIST(2, 1 / kB, 1.0)
        errs.append((e.value.code, str(e.value)))
    assert errs[0] == errs[1] and errs[0][0] == lib.ERR_UNSUPPORTED
    smc = TemperedSMC(pot, D + 1, 2048, 0.5, 0.05, 0.05, seed=3)
    q = smc.run()
    assert smc.betas[-1] == 1.0 and np.isfinite(smc.logZ)
    assert np.all(np.isfinite(np.asarray(q.cpu() if hasattr(q, "cpu") else q)))
    buf = C.create_string_buffer(1024)
    lib.call("pbbi_describe_run", pot.handle, 0, 64, 64, 4, 2, lib.COMPAT_P_FROM_OLDQ, buf, 1024)
    text = buf.value.decode()
    print(text)
    assert "k_glm" in text and "gamma" in text and "sampled" in text and "iterations per launch: up to 1" in text
    lib.call("pbbi_describe_run", held.handle, 0, 64, 64, 4, 2, lib.COMPAT_P_FROM_OLDQ, buf, 1024)
    assert "gamma" in buf.value.decode() and "held" in buf.value.decode()
