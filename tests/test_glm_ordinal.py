"""Ordinal (cumulative-logit) regression on the device: glm.OrdinalGLM (FAM = 6 of k_glm<NT, FAM, true>, its METRIC twin, k_glm_pw
and k_glm_ll), with the CPU pins of what the GPU tests lean on.  The model, the oracle's C++ statement of it in the natural
form, the data generator, the sampling cases and the CPU-only tests are test_glm_ordinal_host.py's.

Tolerance: test_glm_model.py's `rel` / `check` with TOL = 1e-10 relative to max(1, max|oracle|); reject masks are compared for
equality under its `decisive` preconditions (asserted on the oracle's values inside each test).  Step sizes and seeds of the
sampling tests were chosen on the CPU from the oracle alone (test_ordinal_sampling_cases_are_decisive of the host file runs
every one of them without a GPU).

Shapes of the evaluation: N = 303 chains (a ragged last tile), M in {1, 40, 203} (a single row; 203 is no multiple of 16 and
does not fill the padding to 4 blocks), and (D, K) in
    (5, 2)   one cutpoint row                      (5, 5)   four rows: every lane group owns one
    (14, 5)  the cutpoint rows 14 .. 17 straddle the 16-row tile boundary and the lane-group wrap
    (16, 8)  seven rows: one lane group owns two   (MAX_DIM - 4, 5)  the largest shipped state dimension
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
from test_glm_model import check, decisive, device_eval, padded, rel
from test_glm_ordinal_host import (ITER_CASES, MAX_DIM, METRIC_CASES, METRIC_ROWS, RUN_CASES, RUN_CHAIN0, RUN_ITER0, RUN_S,
                                   RUN_SEED, UNIT_H, iter_inputs, iter_oracle, iter_step, make, metric_inputs, metric_ref, numpy_U,
                                   oracle_pot, probabilities, problem, run_inputs, run_oracle, start, table)

LD = np.longdouble
N_EVAL = 303
EVAL_SHAPES = [(5, 2), (5, 5), (14, 5), (16, 8), (MAX_DIM - 4, 5)]
EVAL_CASES = [(M, D, K) for M in (1, 40, 203) for (D, K) in EVAL_SHAPES]


# ---- the draw kernels' reference, computed once and left unchanged ---------------------------------------------------------
def pw_case(M):
    """(kw, slabs (S, Dt, N)) of the draw kernels' tests: D = 5, K = 5, test_glm_pointwise.py's N and S."""
    kw, w, zeta, rs = problem(M, 5, 5, t_pw.DATA_SEED)
    sdn = np.ascontiguousarray(np.stack([start(w, zeta, t_pw.N, rs, spread=0.1) for _ in range(t_pw.S)]))
    return kw, sdn


def ordinal_ref_ll(kw, W):
    """(ll, mu), each (M, T) longdouble, of the draws W (Dt, T): a_i log P(y_i), exactly 0 on a row of weight 0, and the expected
    category -- both from the category probabilities themselves."""
    p, mean = probabilities(kw, W)
    a = kw["weights"]
    ll = a[:, None].astype(LD) * np.log(p)
    ll[a == 0.0] = 0
    return ll, mean


@functools.lru_cache(maxsize=None)
def pw_ref(M):
    kw, sdn = pw_case(M)
    ll, mu = ordinal_ref_ll(kw, t_pw.flat(sdn))
    return t_pw.ref_stats(ll, mu) + (ll.sum(axis=0),)


# ---- the evidence's and the known answer's problems ------------------------------------------------------------------------
EV_CUT = np.array([[-0.6, 4.0], [0.2, 4.0]])      # (mean, precision) of zeta_1 and of the one log-gap
EV_ORDER = 64


def evidence_problem():
    """M = 20 observations of K = 3 categories, one covariate, offsets, weights 1: the state has 3 rows.  Every prior has
    precision 4 (sd 0.5) around a value near the truth, so the posterior is about half as wide as the prior and a Gauss-Hermite
    rule on the prior's scale resolves it."""
    rs = np.random.RandomState(29)
    M = 20
    X = rs.standard_normal((M, 1))
    o = 0.3 * rs.standard_normal(M)
    eta = X[:, 0] * 0.8 + o
    kappa = np.array([-0.6, -0.6 + np.exp(0.2)])
    y = ((rs.logistic(size=M) + eta)[:, None] > kappa[None, :]).sum(axis=1).astype(np.float64)
    assert sorted(set(y)) == [0.0, 1.0, 2.0]
    return dict(X=X, y=y, categories=3, offset=o, prior_precision=np.array([4.0]), prior_mean=np.array([0.5]), cutpoint_prior=EV_CUT)


def evidence_truth(kw, order):
    """log of the integral of the prior N(state; mu, diag(1 / lam)) times prod_i P(y_i | state) over the 3 rows of the state, by
    a tensor Gauss-Hermite rule in longdouble on the prior's scale (state_s = mu_s + sqrt(2 / lam_s) x)."""
    x, wq = np.polynomial.hermite.hermgauss(order)
    keep = wq > 1e-300
    x, lw = x[keep].astype(LD), np.log(wq[keep].astype(LD))
    lam, mu = (v.astype(LD) for v in table(kw))
    g = np.meshgrid(x, x, x, indexing="ij")
    W = np.stack([mu[s] + np.sqrt(2 / lam[s]) * g[s].ravel() for s in range(3)])
    LW = (lw[:, None, None] + lw[None, :, None] + lw[None, None, :]).ravel()
    p, _ = probabilities(dict(kw, weights=None), W)
    with np.errstate(divide="ignore"):      # (the outermost nodes: a probability that underflows weighs nothing)
        v = LW + np.log(p).sum(axis=0)
    m = v.max()
    return float(m + np.log(np.sum(np.exp(v - m))) - LD(1.5) * np.log(LD(np.pi)))


def known_answer_problem():
    """K = 2: M = 60 binary responses from two covariates and a cutpoint; flat priors on the cutpoint / the intercept, N(0, 1)
    on the coefficients."""
    rs = np.random.RandomState(77)
    M = 60
    X = rs.standard_normal((M, 2))
    y = (rs.logistic(size=M) + X @ np.array([0.8, -0.5]) > 0.3).astype(np.float64)
    assert 10 < y.sum() < M - 10
    return X, y


# ------------------------------------------------------------------------------------------------ CPU pins
def test_ordinal_truths_are_what_they_claim():
    kw = evidence_problem()
    t1, t2 = evidence_truth(kw, EV_ORDER), evidence_truth(kw, EV_ORDER + 32)
    print("evidence truth", t1, t2)
    assert abs(t1 - t2) < 1e-8
    # the draw kernels' reference: finite, the expected category inside [0, K - 1], a weight-0 row exactly 0, and the column sums
    # of a_i log P are minus the oracle's likelihood energy (its U under a flat prior)
    for M in (40, 203):
        kw, sdn = pw_case(M)
        lse, mean, var, mu, tot = pw_ref(M)
        assert all(np.all(np.isfinite(v)) for v in (lse, mean, var, mu, tot))
        assert np.all(mu >= 0) and np.all(mu <= 4) and (kw["weights"] == 0).any() and np.all(mean[kw["weights"] == 0] == 0)
        flat_kw = dict(kw, prior_precision=np.zeros(5), cutpoint_prior=np.zeros((4, 2)))
        U = orc.potential(oracle_pot(flat_kw), t_pw.flat(sdn))
        check("column sums against the oracle", -np.asarray(tot, dtype=np.float64), U)


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
@pytest.mark.parametrize("M,D,K", EVAL_CASES)
def test_ordinal_eval_matches_oracle(P, lib, M, D, K):
    kw, w, zeta, rs = problem(M, D, K, 7 * M + D + K)
    a, y, lam = kw["weights"], kw["y"], table(kw)[0]
    assert M == 1 or (a == 0).any()
    assert M < 40 or K == 2 or min(np.sum(y == k) for k in range(K)) == 0          # one category has no observation
    assert M < 40 or ((lam == 0).any() and (lam > 0).any())
    pot, op = make(P, kw), oracle_pot(kw)
    assert pot.numDimensions == D + K - 1 and pot.categories == K
    q = start(w, zeta, N_EVAL, rs)
    Uo, go = orc.potential(op, q, want_grad=True)
    U, g = device_eval(lib, pot, q)
    check(f"U ordinal {M}x{D} K={K}", U, Uo)
    check(f"grad ordinal {M}x{D} K={K}", g, go)
    check("cutpoint rows", g[D:], go[D:])
    check("call", pot(q), Uo)                           # the class API (ldn == N)
    check("gradient", pot.gradient(q), go)


@pytest.mark.gpu
@pytest.mark.parametrize("M,D", [(40, 5), (203, 15), (203, 16)])
def test_ordinal_two_categories_is_logistic_regression(P, lib, M, D):
    """Device against device: OrdinalGLM(categories=2) at [w; kappa] is GLM([1 | X], logistic) at [-kappa; w] -- U and the
    gradient, the sign flipped on the kappa row -- with flat priors on kappa and the intercept."""
    kw, w, zeta, rs = problem(M, D, 2, 3 * M + D)
    kw["cutpoint_prior"] = np.zeros((1, 2))
    q = start(w, zeta, N_EVAL, rs)
    Uo, go = device_eval(lib, make(P, kw), q)
    X1 = np.c_[np.ones(M), kw["X"]]
    logit = P.GLM(X1, kw["y"], family="logistic", weights=kw["weights"], offset=kw["offset"],
                  prior_precision=np.r_[0.0, kw["prior_precision"]], prior_mean=np.r_[0.0, kw["prior_mean"]])
    Ul, gl = device_eval(lib, logit, np.ascontiguousarray(np.vstack([-q[D:], q[:D]])))
    check("U", Uo, Ul)
    check("grad w", go[:D], gl[1:])
    check("grad kappa", go[D], -gl[0])


@pytest.mark.gpu
@pytest.mark.parametrize("M,D,K", [(40, 5, 5), (203, 14, 5), (203, 16, 8)])
def test_ordinal_translation_invariance(P, lib, M, D, K):
    """Device only.  A column of ones in X (a probe: the model is not identified with one) with a flat prior, a flat prior on
    zeta_1: shifting every cutpoint by c is shifting that coefficient by c, so g[zeta_1] = -g[w_ones]."""
    kw, w, zeta, rs = problem(M, D, K, 5 * M + D + K)
    ones = D - 1
    kw["X"][:, ones] = 1.0
    kw["prior_precision"][ones] = 0.0
    kw["cutpoint_prior"][0, 1] = 0.0
    U, g = device_eval(lib, make(P, kw), start(w, zeta, N_EVAL, rs))
    assert np.all(np.isfinite(U)) and np.max(np.abs(g[D])) > 1e-3
    check("g[zeta_1] = -g[w_ones]", g[D], -g[ones])


@pytest.mark.gpu
def test_ordinal_zero_weight_under_overflow(P, lib):
    """A weight-0 row with eta = -800 (whose category probability underflows to 0 in the natural form) and a weight-0 row in
    the ragged last block are not there."""
    M, D, K = 33, 3, 5
    kw, w, zeta, rs = problem(M, D, K, 9)
    q = start(w, zeta, N_EVAL, rs, spread=0.01)
    hot, last = 5, M - 1
    kw["X"][hot] = -800.0 * w / (w @ w)
    kw["y"][hot] = K - 1.0
    kw["weights"][[hot, last]] = 0.0
    kw["weights"][[hot + 1, last - 1]] = 3.0
    keep = np.ones(M, bool)
    keep[[hot, last]] = False
    Uo, go = orc.potential(oracle_pot(kw, keep), q, want_grad=True)
    U, g = device_eval(lib, make(P, kw), q)
    assert np.all(np.isfinite(U)) and np.all(np.isfinite(g))
    check("U", U, Uo)
    check("grad", g, go)


@pytest.mark.gpu
@pytest.mark.parametrize("M,D,K,h_lf,h_sv,L", ITER_CASES)
@pytest.mark.parametrize("method", ["Leapfrog", "Stormer-Verlet"])
@pytest.mark.parametrize("mass", [False, True])
@pytest.mark.parametrize("kt", [False, True])
def test_ordinal_uploaded_draw_iteration_matches_oracle(P, lib, M, D, K, h_lf, h_sv, L, method, mass, kt):
    import torch
    h = iter_step(method, mass, h_lf, h_sv)
    d = _dev()
    kw, N, kT, m, q, p, u = iter_inputs(M, D, K, mass, kt)
    o = iter_oracle(M, D, K, h, L, method, mass, kt)
    decisive(o["ratio"], o["u"], o["rej"], 0.1, 0.9)
    Dt = D + K - 1
    pot = make(P, kw)
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
@pytest.mark.parametrize("M,D,K,N,h,L", RUN_CASES)
def test_ordinal_philox_run_matches_oracle(P, lib, M, D, K, N, h, L):
    """pbbi_hmc_run, PBBI_DRAW_F64: the oracle draws its own momenta of the (Dt, N) state (no device draw is replayed)."""
    import torch
    d = _dev()
    kw, q = run_inputs(M, D, K, N)
    o = run_oracle(M, D, K, N, h, L)
    assert np.all(np.isfinite(o["samples"])) and np.all(np.isfinite(o["momenta"]))
    decisive(o["ratio"], o["u"], o["rej"], 0.1, 0.9)
    pot = make(P, kw)
    Dt, S = D + K - 1, RUN_S
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
@pytest.mark.parametrize("D,K", sorted(METRIC_CASES))
def test_ordinal_metric_run_vs_restatement(P, lib, D, K):
    """pbbi_hmc_run on an ordinal handle with a diagonal metric against test_glm_metric.py's restatement (S = 3, kT = 2.5,
    per-chain masses, PBBI_DRAW_F64, leading stride N + 5); a metric of ones is the handle without one bit for bit."""
    M, hs, L = METRIC_CASES[(D, K)]
    Dt = D + K - 1
    kw, q0 = metric_inputs(D, K)
    pot, fresh = make(P, kw), make(P, kw)
    pot.set_metric(t_metric.metric_of(Dt))
    assert np.array_equal(pot.metric, t_metric.metric_of(Dt)) and fresh.metric is None
    for method, beta, compat in METRIC_ROWS:
        o = metric_ref(D, K, method, beta, compat)
        t_metric._margin(str((D, K, method)), o["ratio"], o["u"])
        h = hs[F.METHODS.index(method)]
        gs, gm, grej, gratio, gq, gpad = F._device_run(lib, pot, method, q0, F.MASS, h, L, F.S_RUN,
                                                       t_metric._flags(lib, beta, compat), F.KT, pad=5)
        tag = f"ordinal D={D} K={K} {method}"
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
    pot.set_metric(np.ones(Dt))
    for (me, b, c), w in zip(METRIC_ROWS, want):
        got = F._device_run(lib, pot, me, q0, F.MASS, UNIT_H * hs[F.METHODS.index(me)], L, F.S_RUN, t_metric._flags(lib, b, c),
                            F.KT, pad=5)
        for tag, a, r in zip(("samples", "momenta", "reject", "ratio", "state", "padding"), got, w):
            assert np.array_equal(a, r), (D, K, me, tag)


@pytest.mark.gpu
def test_ordinal_adapt_mass_matrix(P, lib):
    from scipy.constants import k as kB
    kw, w, zeta, _ = problem(203, 5, 5, 41)
    # (a proper posterior: this data's category 0 is empty and its zeta_1 has a flat prior, so kappa_1 would drift to -inf)
    assert np.sum(kw["y"] == 0) == 0 and kw["cutpoint_prior"][0, 1] == 0.0
    kw["cutpoint_prior"][:, 1] = np.maximum(kw["cutpoint_prior"][:, 1], 1.0)
    pot = make(P, kw)
    hmc = P.HMC(P.Ensemble(9, 512), 1.0, 0.05, None, potential=pot, rng="philox", seed=4, verbose=False, compat=False,
                draw_f64=True)
    m = hmc.adaptMassMatrix(1 / kB, 0.3, windows=(25, 50))
    print("adapted metric", m, "step", hmc.stepSize)
    assert m.shape == (9,) and np.all(np.isfinite(m)) and np.all(m > 0)
    assert np.array_equal(m, pot.metric) and np.isfinite(hmc.stepSize) and hmc.stepSize > 0


@pytest.mark.gpu
@pytest.mark.parametrize("M", [40, 203])
def test_ordinal_pointwise_and_loglik_match_reference(P, lib, M):
    """k_glm_pw and k_glm_ll against the longdouble NumPy reduction of a_i log P(y_i), a weight-0 row included; mu_i is the
    expected category; loglik is the column sums of the pointwise reference."""
    kw, sdn = pw_case(M)
    lse, mean, var, mu, tot = pw_ref(M)
    pot = make(P, kw)
    got = t_pw.device_pointwise(lib, pot, sdn)
    t_pw.check_all(f"ordinal M={M}", got, (lse, mean, var, mu))
    zero = kw["weights"] == 0.0
    assert zero.any()
    assert np.all(got[1][zero] == 0.0) and np.all(got[2][zero] == 0.0) and np.all(got[3][zero] != 0.0)
    T = t_pw.N * t_pw.S
    host = np.ascontiguousarray(sdn.transpose(1, 2, 0))
    r = pot.pointwise(host)
    assert r.T == T
    check("lppd_i", r.lppd_i, lse - np.log(LD(T)))
    check("p_waic_i", r.p_waic_i, var)
    check("mu_i", r.mu_i, mu)
    ref = tot.reshape(t_pw.S, t_pw.N).T
    a = pot.loglik(host)
    assert a.shape == (t_pw.N, t_pw.S)
    check("loglik", a, ref)
    pot.set_likelihood_power(0.25)                       # the likelihood is reported at power 1 while the handle is tempered
    assert t_power.same_bits(pot.loglik(host), a)
    check("pointwise sees the power", pot.pointwise(host).mean_ll_i, 0.25 * mean)


@pytest.mark.gpu
@pytest.mark.parametrize("beta", t_power.BETAS)
@pytest.mark.parametrize("D,K", [(5, 5), (16, 8)])
def test_ordinal_power_is_prior_plus_beta_times_likelihood(P, lib, D, K, beta):
    """U = U_prior + beta U_lik and its gradient -- the cutpoints' included, whose A_k / expm1(Delta_k) part scales with the
    weights -- against the longdouble NumPy value and the oracle on weights beta a_i; from the host and from a device double."""
    import torch
    kw, w, zeta, rs = problem(203, D, K, t_power.SEED)
    q = start(w, zeta, 37, rs, spread=0.1)
    pot = make(P, kw)
    assert pot.likelihood_power == 1.0
    U1, g1 = pot.value_and_gradient(q)
    pot.set_likelihood_power(beta)
    assert pot.likelihood_power == beta
    U, g = pot.value_and_gradient(q)
    flat = dict(kw, prior_precision=np.zeros(D), cutpoint_prior=np.zeros((K - 1, 2)))
    Ulik = numpy_U(flat, q)
    Uprior = numpy_U(kw, q) - Ulik
    check(f"U beta={beta}", U, Uprior + LD(beta) * Ulik)
    Uo, go = orc.potential(oracle_pot(dict(kw, weights=beta * kw["weights"])), q, want_grad=True)
    check(f"U beta={beta} (oracle)", U, Uo)
    check(f"grad beta={beta} (oracle)", g, go)
    pot2 = make(P, kw)
    bdev = torch.tensor([beta], dtype=torch.float64, device="cuda:0")
    pot2.set_likelihood_power(0.0, beta_dev=bdev.data_ptr())
    U2, g2 = pot2.value_and_gradient(q)
    assert t_power.same_bits(U, U2) and t_power.same_bits(g, g2) and np.isnan(pot2.likelihood_power)
    pot.set_likelihood_power(1.0)
    U3, g3 = pot.value_and_gradient(q)
    assert t_power.same_bits(U3, U1) and t_power.same_bits(g3, g1)


@pytest.mark.gpu
def test_ordinal_sample_prior_is_the_stated_transform(P, lib):
    rs = np.random.RandomState(2)
    M, N, seed, K = 12, 50, 9, 4
    X = rs.standard_normal((M, 3))
    y = (np.arange(M) % K).astype(np.float64)
    lam, mu = np.array([1.0, 4.0, 0.25]), np.array([0.5, -1.0, 0.0])
    cp = np.array([[-0.5, 2.0], [0.1, 1.0], [0.3, 4.0]])
    pot = P.OrdinalGLM(X, y, prior_precision=lam, prior_mean=mu, cutpoint_prior=cp)
    q = pot.sample_prior(N, seed=seed)
    assert q.is_cuda and tuple(q.shape) == (6, N)
    z = t_ev.normals(lib, seed, 6, N)
    ref = np.r_[mu, cp[:, 0]][:, None] + z / np.sqrt(np.r_[lam, cp[:, 1]])[:, None]
    err = np.max(np.abs(q.cpu().numpy() - ref) / np.maximum(1.0, np.abs(ref)))
    print("sample_prior", err)
    assert err < 1e-14
    with pytest.raises(ValueError, match="cutpoint_prior"):
        P.OrdinalGLM(X, y, cutpoint_prior=((0.0, 0.0), (0.0, 1.0))).sample_prior(N)


@pytest.mark.gpu
def test_ordinal_evidence(P):
    """LikelihoodTemperedSMC.logML of the 3-row model against the quadrature, test_glm_evidence.py's 8-seed rule and particle
    count."""
    kw = evidence_problem()
    zs = t_ev.evidence(P, lambda: P.OrdinalGLM(**kw), simulTime=1.0, stepSize=0.1, moves=5)
    t_ev.rule(zs, evidence_truth(kw, EV_ORDER))


@pytest.mark.gpu
def test_ordinal_known_answer(P):
    """K = 2 against the shipped logistic GLM on the same data: the posterior means of -kappa_1 (the intercept) and of w agree.
    4096 independent chains each, step size from adaptStepSize, 300 iterations of L = 10 of burn-in, the final state of every
    chain: the chains are independent, so each run's effective sample size is its number of chains and the standard error of
    the difference of the two means is sqrt(var_1 / N + var_2 / N) from the runs' own variances.  Margin: 4 standard errors."""
    from scipy.constants import k as kB
    X, y = known_answer_problem()
    M, N = y.size, 4096
    ordinal = P.OrdinalGLM(X, y, categories=2, prior_precision=1.0, cutpoint_prior=np.zeros((1, 2)))
    logit = P.GLM(np.c_[np.ones(M), X], y, family="logistic", prior_precision=np.array([0.0, 1.0, 1.0]))
    finals = []
    for pot, seed in ((ordinal, 2024), (logit, 4048)):
        warm = P.HMC(P.Ensemble(3, N), 0.5, 0.05, None, potential=pot, rng="philox", seed=seed, verbose=False)
        h = warm.adaptStepSize(1 / kB, 0.3)
        assert 1e-3 < h < 1.0, h
        hmc = P.HMC(P.Ensemble(3, N), 10.5 * h, h, None, potential=pot, rng="philox", seed=seed, verbose=False)
        assert hmc.integrator.numSteps == 10
        s, _ = hmc.getSamples(1, 1 / kB, 0.3, burn_in=300)
        last = np.asarray(s)[:, :, 0]
        assert np.all(np.isfinite(last))
        print("step", h, "accept", hmc.acceptRate)
        finals.append(last)
    w_o, kappa = ordinal.split(finals[0])
    a = np.vstack([-kappa, w_o])                        # (intercept, w) of the ordinal run
    b = finals[1]
    se = np.sqrt(a.var(axis=1, ddof=1) / N + b.var(axis=1, ddof=1) / N)
    dev = (a.mean(axis=1) - b.mean(axis=1)) / se
    print("means", a.mean(axis=1), b.mean(axis=1), "deviation / se", dev)
    assert np.all(np.abs(dev) <= 4.0)


@pytest.mark.gpu
def test_ordinal_through_the_classes(P, lib):
    """HMC.getSamples in both rng modes and both methods, with and without a metric, sampleStats and pbbi_describe_run take an
    OrdinalGLM; split returns the coefficients and the ordered cutpoints; GIST refuses it as it refuses GLM."""
    from scipy.constants import k as kB
    M, D, K, N, S = 203, 5, 5, 200, 4
    Dt = D + K - 1
    kw, w, zeta, rs = problem(M, D, K, 71)
    pot = make(P, kw)
    assert pot.numDimensions == Dt and pot.numCoefficients == D and pot.family == "ordinal"
    for metric in (None, np.linspace(0.5, 2.0, Dt)):
        pot.set_metric(metric)
        for rng, method in (("philox", "Leapfrog"), ("numpy", "Leapfrog"), ("philox", "Stormer-Verlet")):
            np.random.seed(5)
            hmc = P.HMC(P.Ensemble(Dt, N), 0.4, 0.05, None, potential=pot, rng=rng, seed=13, verbose=False, method=method)
            s, m = hmc.getSamples(S, 1 / kB, 0.3)
            s, m = np.asarray(s), np.asarray(m)
            assert s.shape == (Dt, N, S) and np.all(np.isfinite(s)) and np.all(np.isfinite(m))
            assert 0.0 < hmc.acceptRate <= 1.0
            coef, kappa = pot.split(s)
            assert coef.shape == (D, N, S) and kappa.shape == (K - 1, N, S)
            assert np.array_equal(coef, s[:D]) and np.all(np.diff(kappa, axis=0) > 0)
            check("unconstrain", pot.unconstrain(coef, kappa), s)
    pot.set_metric(None)
    stats = P.HMC(P.Ensemble(Dt, N), 0.4, 0.05, None, potential=pot, rng="philox", seed=13,
                  verbose=False).sampleStats(8, 4, 1 / kB, 0.3, burn_in=2, max_lag=2)
    mean, var = stats.moments()[:2]
    mean, var = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (mean, var))
    assert mean.shape[0] == Dt and np.all(np.isfinite(mean)) and np.all(np.isfinite(var))
    errs = []
    plain = P.GLM(kw["X"], np.minimum(kw["y"], 1.0))
    for target, dim in ((pot, Dt), (plain, D)):
        with pytest.raises(lib.PbbiError) as e:
            P.HMC(P.Ensemble(dim, 64), 0.8, 0.1, None, potential=target, rng="philox", seed=13,
                  verbose=False).getSamplesGIST(2, 1 / kB, 1.0)
        errs.append((e.value.code, str(e.value)))
    assert errs[0] == errs[1] and errs[0][0] == lib.ERR_UNSUPPORTED
    buf = C.create_string_buffer(2048)
    lib.call("pbbi_describe_run", pot.handle, 0, 64, 64, 4, 2, lib.COMPAT_P_FROM_OLDQ, buf, 2048)
    text = buf.value.decode()
    print(text)
    assert "k_glm" in text and "ordinal" in text and "5 categories" in text and "iterations per launch: up to 1" in text
    # the default categories and the default priors
    auto = P.OrdinalGLM(kw["X"], kw["y"])
    assert auto.categories == int(kw["y"].max()) + 1
    assert np.array_equal(auto.cutpoint_prior[0], [0.0, 0.1]) and np.all(auto.cutpoint_prior[1:] == np.array([0.0, 1.0]))
