"""Posterior predictive replicates and their per-draw statistics, drawn in the kernel (csrc/kernels_glm_predictive.hip,
csrc/glm_sample_dev.h, pbbi_predictive_glm, `predictive` of the GLM classes).

References.  (1) The replicates: glm_predictive_ref.py, the NumPy restatement of the RNG contract's section "Predictive
replicates" with SciPy's masses; discrete values must agree EXACTLY wherever the reference is decided (see there: at most 0.1 %
of a case may be undecided, asserted), continuous ones to test_glm.py's TOL = 1e-10 relative to max(1, max|reference|).
(2) The statistics: recomputed in longdouble from the device's OWN replicates (log Gamma in double, promoted, as
test_glm_pointwise.py does), TOL through `check`; min, max and the count exactly.  (3) The distribution: the chi-square / KS
bound p >= 1e-6 of test_glm_predictive_host.py on the device's replicates.  (4) End to end: posterior predictive p-values of
the variance of well and badly specified count models.

Problems: the kinds of test_glm_pointwise.py (M = 203 .. 300, N = 150, S = 3: a ragged last tile, weights with zeros, trials
1 .. 20, NT = 1, 2, 4, 8), `hier_nc`, and the ordinal and gamma draw cases of their own test files."""
import functools

import numpy as np
import pytest

import glm_predictive_ref as R
import test_glm_gamma as t_gamma
import test_glm_ordinal as t_ord
import test_glm_ordinal_host as t_ordh
import test_glm_pointwise as t_pw
from test_glm import check
from test_glm_predictive_host import DIST_CASES, DIST_IDS, DIST_M, DIST_SEED, DIST_T, P_MIN

LD = np.longdouble
N, S = t_pw.N, t_pw.S
T = N * S
SEED = 77
PAD, GUARD = t_pw.PAD, t_pw.GUARD
NAN_BITS = t_pw.NAN_BITS
COUNT_FAMILIES = ("poisson", "logistic", "negbinomial", "ordinal")
NAMES = sorted(t_pw.KINDS) + ["hier_nc", "ordinal", "gamma_sampled", "gamma_held"]


# ---- the problems: (make, spec, slabs in sampler coordinates, natural-scale draws (Dt, T), cutpoints or None) --------------------
@functools.lru_cache(maxsize=None)
def case(name):
    kap = None
    if name == "ordinal":
        kw, sdn = t_ord.pw_case(203)
        sp = t_pw.spec_of("ordinal", kw, 5)
        sp["K"] = kw["categories"]
        make = lambda P: t_ordh.make(P, kw)
        W = t_pw.flat(sdn)
        kap = np.cumsum(np.concatenate([W[5:6], np.exp(W[6:5 + sp["K"] - 1])], axis=0), axis=0)
    elif name.startswith("gamma"):
        sampled = name == "gamma_sampled"
        kw, theta, sp, sdn = t_gamma.pw_case(203, sampled)
        make = lambda P: t_gamma.make(P, kw, sampled, theta)
        W = t_pw.flat(sdn)
    else:
        make, sp, sdn, _ = t_pw.kind(name)
        W = t_pw.flat(np.stack([t_pw.t_nc.natural_np(sp["kw"], q) for q in sdn]) if name == "hier_nc" else sdn)
    return make, sp, sdn, W, kap


@functools.lru_cache(maxsize=None)
def reference(name):
    """(yrep (T, M), undecided (T, M)) of the case at SEED: computed once, shared, never written to."""
    _, sp, _, W, kap = case(name)
    y, und = R.replicates(sp, W, SEED, kap)
    y.setflags(write=False)
    und.setflags(write=False)
    return y, und


def host_samples(sdn):
    return np.ascontiguousarray(np.asarray(sdn).transpose(1, 2, 0))      # (Dt, N, S)


def per_draw(a):
    return np.asarray(a).T.ravel()                                       # (N, S) -> draw t = s * N + n


def logpdf_ld(sp, W, Y, kap):
    """log f(Y[t, i] | draw t) (T, M) in longdouble: the full proper density, unweighted -- but for the Gaussian, whose weight
    is a precision weight."""
    X, o, n, a = (np.asarray(sp[k]).astype(LD) for k in ("X", "o", "n", "a"))
    Wl = np.asarray(W).astype(LD)
    eta = (X @ Wl[:sp["Dx"]] + o[:, None]).T
    Y = np.asarray(Y).astype(LD)
    fam = sp["family"]
    th = (Wl[sp["trow"]][:, None] if sp.get("trow", -1) >= 0 else LD(0.0 if sp.get("theta") is None else sp["theta"])) + 0 * eta
    g = t_pw.gammaln_ld
    with np.errstate(invalid="ignore", divide="ignore"):
        if fam == "logistic":
            return g(n + 1)[None] - g(Y + 1) - g(n[None] - Y + 1) + Y * eta - n[None] * np.logaddexp(LD(0), eta)
        if fam == "poisson":
            return Y * eta - np.exp(eta) - g(Y + 1)
        if fam == "gaussian":
            return -LD(0.5) * np.log(2 * LD(np.pi)) - th + LD(0.5) * np.log(a)[None] - LD(0.5) * a[None] * np.exp(-2 * th) * (Y - eta) ** 2
        if fam == "negbinomial":
            phi, z = np.exp(th), eta - th
            return g(Y + phi) - g(phi) - g(Y + 1) - (Y + phi) * np.logaddexp(LD(0), z) + Y * z
        if fam == "gamma":
            al = np.exp(th)
            return al * th - al * eta + (al - 1) * np.log(Y) - al * Y * np.exp(-eta) - g(al)
        kp = np.asarray(kap).astype(LD).T                                        # (T, K - 1)
        cdf = np.concatenate([np.zeros(eta.shape + (1,), LD), 1 / (1 + np.exp(-(kp[:, None, :] - eta[:, :, None]))),
                              np.ones(eta.shape + (1,), LD)], axis=2)
        pk = np.diff(cdf, axis=2)
        return np.log(np.take_along_axis(pk, np.nan_to_num(Y, nan=0.0).astype(int)[:, :, None], axis=2)[:, :, 0])


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


def device_predictive(lib, pot, sdn, seed=SEED, centre=0.0, cut=0.0, ranges=0, keep=0):
    """(stats (7, T), yrep (keep, M) or None) of pbbi_predictive_glm on (S, Dt, N) NATURAL-scale host slabs, inside the NaN
    canary: a guard behind the slabs, and both outputs in the middle of longer NaN-filled arrays that must keep their bits."""
    import torch
    from physicsbasedbayesianinference_amd import _device, glm
    s, Dt, n = sdn.shape
    M, Tn = pot.y.size, s * n
    buf = torch.full((sdn.size + GUARD,), float("nan"), dtype=torch.float64, device="cuda:0")
    buf[:sdn.size] = torch.from_numpy(np.array(sdn).ravel()).to("cuda:0")
    aux = torch.from_numpy(glm._predictive_aux(pot)[0]).to("cuda:0")
    stats = torch.full((7 * Tn + 2 * PAD,), float("nan"), dtype=torch.float64, device="cuda:0")
    yrep = torch.full((keep * M + 2 * PAD,), float("nan"), dtype=torch.float64, device="cuda:0")
    lib.call("pbbi_predictive_glm", pot.handle, buf.data_ptr(), s, Dt, n, seed, aux.data_ptr(), centre, cut, ranges,
             stats[PAD:].data_ptr(), keep, yrep[PAD:].data_ptr() if keep else None, _device.stream_ptr(0))
    torch.cuda.synchronize()
    sb, yb = stats.cpu().numpy(), yrep.cpu().numpy()
    assert np.all(sb.view(np.int64)[:PAD] == NAN_BITS) and np.all(sb.view(np.int64)[PAD + 7 * Tn:] == NAN_BITS), "stats_out"
    assert np.all(yb.view(np.int64)[:PAD] == NAN_BITS) and np.all(yb.view(np.int64)[PAD + keep * M:] == NAN_BITS), "yrep_out"
    assert np.all(buf[sdn.size:].cpu().numpy().view(np.int64) == NAN_BITS), "the guard behind the slabs was written"
    return sb[PAD:PAD + 7 * Tn].reshape(7, Tn).copy(), (yb[PAD:PAD + keep * M].reshape(keep, M).copy() if keep else None)


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_replicates_match_the_reference(P, name):
    """1. `yrep` of every draw against the restated contract; weight-0 rows are NaN."""
    make, sp, sdn, W, kap = case(name)
    yref, und = reference(name)
    print("undecided %s: %d of %d" % (name, und.sum(), und.size))
    assert und.mean() <= R.MAX_UNDECIDED
    r = make(P).predictive(host_samples(sdn), seed=SEED, keep=T)
    assert r.yrep.shape == (T, sp["y"].size) and r.T == T and r.mean.shape == (N, S)
    off = sp["a"] == 0.0
    assert np.all(np.isnan(r.yrep[:, off])) and np.all(np.isfinite(r.yrep[:, ~off])) and np.all(np.isfinite(yref[:, ~off]))
    ok = ~und & ~off[None, :]
    if sp["family"] in COUNT_FAMILIES:
        bad = np.argwhere(ok & (r.yrep != yref))
        assert bad.size == 0, (name, len(bad), bad[:5], r.yrep[tuple(bad[:5].T)], yref[tuple(bad[:5].T)])
    else:
        check("yrep " + name, r.yrep[ok], yref[ok])


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_statistics_are_those_of_the_devices_own_replicates(P, name):
    """2. All seven against the longdouble recomputation from the device's yrep; min, max and the count exactly."""
    make, sp, sdn, W, kap = case(name)
    pot = make(P)
    cut = 1.0 if sp["family"] in COUNT_FAMILIES else float(np.median(sp["y"]))
    r = pot.predictive(host_samples(sdn), seed=SEED, keep=T, cut=cut)
    on = sp["a"] != 0.0
    Y = r.yrep[:, on].astype(LD)
    mean = Y.mean(axis=1)
    check("mean", per_draw(r.mean), mean)
    check("var", per_draw(r.var), ((Y - mean[:, None]) ** 2).mean(axis=1))
    assert np.array_equal(per_draw(r.min), r.yrep[:, on].min(axis=1)) and np.array_equal(per_draw(r.max), r.yrep[:, on].max(axis=1))
    assert np.array_equal(per_draw(r.frac_le_cut), (r.yrep[:, on] <= cut).sum(axis=1).astype(np.float64) / on.sum())
    check("loglik_rep", per_draw(r.loglik_rep), logpdf_ld(sp, W, r.yrep, kap)[:, on].sum(axis=1))
    yobs = np.broadcast_to(np.asarray(sp["y"], dtype=np.float64)[None, :], r.yrep.shape)
    check("loglik_obs", per_draw(r.loglik_obs), logpdf_ld(sp, W, yobs, kap)[:, on].sum(axis=1))
    yo = np.asarray(sp["y"])[on]
    assert r.observed["mean"] == pytest.approx(yo.mean(), rel=1e-14) and r.observed["var"] == pytest.approx(yo.var(), rel=1e-12)
    assert r.observed["min"] == yo.min() and r.observed["max"] == yo.max() and r.observed["frac_le_cut"] == np.mean(yo <= cut)
    assert 0.0 <= r.pvalue("var") <= 1.0 and 0.0 <= r.pvalue("loglik") <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["poisson_full", "binomial_trials", "negbinomial_sampled", "gaussian_sampled", "logistic128",
                                  "ordinal", "gamma_sampled"])
def test_geometry_does_not_reach_the_replicates(P, lib, name):
    """3. yrep bit-identical across ranges and across keep; integer-valued statistics of the count families at centre 0
    bit-identical across ranges; the same call twice gives the same bits throughout."""
    make, sp, sdn, W, kap = case(name)
    pot = make(P)
    nat = W.reshape(W.shape[0], S, N).transpose(1, 0, 2)
    s1, y1 = device_predictive(lib, pot, nat, ranges=1, keep=T)
    s3, y3 = device_predictive(lib, pot, nat, ranges=3, keep=T)
    s3b, y3b = device_predictive(lib, pot, nat, ranges=3, keep=T)
    s0, _ = device_predictive(lib, pot, nat, ranges=3, keep=0)
    _, yk = device_predictive(lib, pot, nat, ranges=0, keep=7)
    assert same_bits(y1, y3) and same_bits(y3, y3b) and same_bits(s3, s3b) and same_bits(s3, s0) and same_bits(yk, y1[:7])
    assert same_bits(s1[2:5], s3[2:5])
    if sp["family"] in COUNT_FAMILIES:
        assert same_bits(s1[:2], s3[:2])
    for k in (0, 1, 5, 6):
        check("statistic %d across ranges" % k, s3[k], s1[k].astype(LD))


@functools.lru_cache(maxsize=None)
def unit_case(family):
    """Unit weights, so that statistic 6 is pot.loglik: (make, slabs)."""
    if family in ("logistic", "poisson"):
        X, y, w, rs = t_pw.t_plain.problem(family, 203, 5, t_pw.DATA_SEED)
        return (lambda P: P.GLM(X, y, family=family)), t_pw._slabs(lambda k: t_pw.t_plain.start(w, k, rs))
    if family == "ordinal":
        kw, sdn = t_ord.pw_case(203)
        kw = dict(kw, weights=None)
        return (lambda P: P.OrdinalGLM(**kw)), sdn
    if family == "gamma":
        kw, theta, _, sdn = t_gamma.pw_case(203, True)
        kw = dict(kw, weights=None)
        return (lambda P: t_gamma.make(P, kw, True, theta)), sdn
    kw, w, theta, rs = t_pw.t_disp.problem(family, 40, 5, t_pw.DATA_SEED)
    kw = dict(kw, weights=None)
    return ((lambda P: t_pw.t_disp.make(P, kw, True, theta)),
            t_pw._slabs(lambda k: t_pw.t_disp.start(w, theta, k, rs, spread=0.1, sampled=True)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["logistic", "poisson", "gaussian", "negbinomial", "gamma", "ordinal", "logistic17", "logistic50",
                                  "logistic128"])
def test_observed_loglik_is_the_shipped_loglik(P, name):
    """4. Statistic 6 against pot.loglik(samples) of the same draws, on unit weights."""
    make, sdn = (case(name)[0], case(name)[2]) if name[-1].isdigit() else unit_case(name)
    pot = make(P)
    assert pot.weights is None or np.all(pot.weights == 1.0)
    host = host_samples(sdn)
    ll = pot.loglik(host)
    check("loglik_obs " + name, pot.predictive(host, seed=SEED).loglik_obs, ll.astype(LD))


def dist_problem(P, family, par):
    """4096 identical rows, 64 identical draws at the parameters of the host test: (pot, samples (Dt, 64, 1))."""
    X, one = np.ones((DIST_M, 1)), np.ones(DIST_M)
    rep = lambda *rows: np.repeat(np.array(rows, dtype=np.float64)[:, None, None], DIST_T, axis=1)
    if family == "poisson":
        return P.GLM(X, one, family="poisson"), rep(np.log(par["mu"]))
    if family == "logistic":
        return P.GLM(X, one, family="logistic", trials=np.full(DIST_M, float(par["n"]))), rep(np.log(par["p"]) - np.log1p(-par["p"]))
    if family == "ordinal":
        kap = np.array(par["kap"])
        return P.OrdinalGLM(X, one, categories=kap.size + 1), rep(par["eta"], kap[0], *np.log(np.diff(kap)))
    disp = dict(negbinomial="phi", gamma="alpha", gaussian="sigma")[family]
    pot = P.DispersionGLM(X, one, family=family, dispersion=float(par[disp]))
    return pot, rep(par["mu"] if family == "gaussian" else np.log(par["mu"]))


@pytest.mark.gpu
@pytest.mark.parametrize("family,par", DIST_CASES, ids=DIST_IDS)
def test_device_replicates_follow_the_exact_distribution(P, family, par):
    """5. The host test's bound on the device's own values; beside it they are the reference's (the enumeration from a mode
    well away from 0 included: Poisson 180, the negative binomials).  The reference here decides nothing, so values may differ
    in the share that may be undecided: expected ~1e-9, cap 0.1 %."""
    pot, samples = dist_problem(P, family, par)
    r = pot.predictive(samples, seed=DIST_SEED, keep=DIST_T)
    assert r.yrep.shape == (DIST_T, DIST_M) and np.all(np.isfinite(r.yrep))
    p = R.gof_pvalue(family, r.yrep, **par)
    print("p-value %s %s: %.3g" % (family, par, p))
    assert p >= P_MIN
    ref = R.fixed(family, DIST_SEED, DIST_T, DIST_M, **par)
    if family in COUNT_FAMILIES:
        assert np.mean(r.yrep != ref) <= R.MAX_UNDECIDED
    else:
        differ = np.abs(r.yrep - ref) > 1e-10 * max(1.0, np.abs(ref).max())
        assert np.mean(differ) <= R.MAX_UNDECIDED


@pytest.mark.gpu
def test_edges_nan_draws_the_variance_cap_and_refusals(P, lib):
    """6. A NaN coefficient poisons its own draw's statistics 0, 1, 2, 3, 5 (and 6) only; a mean beyond the variance cap gives
    NaN; the refusals are ValueErrors.  Every direct call here runs inside the NaN canary."""
    make, sp, sdn, W, _ = case("poisson_full")
    pot = make(P)
    nat = np.array(W.reshape(W.shape[0], S, N).transpose(1, 0, 2))
    clean, yc = device_predictive(lib, pot, nat, keep=T)
    nat[1, 2, 7] = np.nan                                                    # draw t = N + 7
    X, o, on = sp["X"], sp["o"], sp["a"] != 0.0
    u = nat[2, :, 11].copy()
    top = int(np.argmax(np.where(on, X @ u, -np.inf)))
    nat[2, :, 11] = u * (np.log(2.0 ** 20 * 1.5) - o[top]) / (X @ u)[top]     # draw 2 N + 11: a mean of 1.5 * 2^20 on one row
    got, yg = device_predictive(lib, pot, nat, keep=T)
    t_nan, t_cap = N + 7, 2 * N + 11
    assert np.all(np.isnan(got[[0, 1, 2, 3, 5, 6], t_nan])) and np.all(np.isnan(yg[t_nan, on]))
    assert np.all(np.isnan(got[[0, 1, 2, 3, 5], t_cap])) and np.isfinite(got[6, t_cap]) and np.isnan(yg[t_cap, top])
    eta_cap = X @ nat[2, :, 11] + o
    assert np.array_equal(np.isnan(yg[t_cap]), ~on | (eta_cap > np.log(2.0 ** 20)))
    rest = np.ones(T, dtype=bool)
    rest[[t_nan, t_cap]] = False
    assert same_bits(got[:, rest], clean[:, rest]) and same_bits(yg[rest], yc[rest])
    host = host_samples(sdn)
    for kw, text in ((dict(keep=T + 1), "keep must be in"), (dict(keep=-1), "keep must be in"), (dict(cut=float("nan")), "cut must be finite"),
                     (dict(ranges=65536), "ranges must be")):
        with pytest.raises(ValueError, match=text):
            pot.predictive(host, **kw)
    with pytest.raises(ValueError, match="rows"):
        pot.predictive(host[:3])
    assert not hasattr(P.SoftmaxGLM, "predictive")


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------
E2E_M, E2E_CHAINS, E2E_SEED = 256, 2048, 3      # E2E_SEED: chosen on the CPU (test_end_to_end_bands_hold_for_the_reference_alone)


def e2e_data(seed=E2E_SEED):
    """(X, y_poisson, y_overdispersed): an intercept and two covariates, means around 5; negative-binomial counts of shape 0.5."""
    rs = np.random.RandomState(seed)
    X = np.c_[np.ones(E2E_M), 0.5 * rs.standard_normal((E2E_M, 2))]
    mu = np.exp(X @ np.array([1.5, 0.4, -0.3]))
    return X, rs.poisson(mu).astype(np.float64), rs.negative_binomial(0.5, 0.5 / (0.5 + mu)).astype(np.float64)


def laplace_draws(X, y, family, n, rs):
    """n draws from the normal approximation at the posterior mode (prior precision 1), on the CPU: what stands in for HMC when
    the bands are checked with the reference alone.  negbinomial: theta = log phi is a further row (prior N(0, 1))."""
    from scipy import optimize, special
    D = X.shape[1]

    def U(q):
        eta = X @ q[:D]
        if family == "poisson":
            return np.sum(np.exp(eta) - y * eta) + 0.5 * q @ q
        phi = np.exp(q[D])
        return -np.sum(special.gammaln(y + phi) - special.gammaln(phi) + phi * q[D] + y * eta - (y + phi) * np.logaddexp(eta, q[D])) + 0.5 * q @ q

    q0 = np.zeros(D + (family != "poisson"))
    q0[0] = np.log(y.mean() + 0.1)
    mode = optimize.minimize(U, q0, method="BFGS", options=dict(gtol=1e-8)).x
    h, H = 1e-4, np.empty((mode.size, mode.size))
    for a in range(mode.size):
        for b in range(mode.size):
            ea, eb = h * np.eye(mode.size)[a], h * np.eye(mode.size)[b]
            H[a, b] = (U(mode + ea + eb) - U(mode + ea - eb) - U(mode - ea + eb) + U(mode - ea - eb)) / (4 * h * h)
    return mode[:, None] + np.linalg.cholesky(np.linalg.inv(0.5 * (H + H.T))) @ rs.standard_normal((mode.size, n))


def reference_pvalue_var(X, y, family, W, seed):
    sp = dict(family=family, X=X, y=y, a=np.ones(y.size), o=np.zeros(y.size), n=np.ones(y.size), Dx=X.shape[1],
              trow=X.shape[1] if family == "negbinomial" else -1, theta=None)
    eta = R.linear_predictor(sp, W)
    th = np.asarray(W)[sp["trow"]][None, :] if sp["trow"] >= 0 else 0.0
    yrep = R.discrete(family, R.uniform(seed, np.arange(W.shape[1])[None, :], np.arange(y.size)[:, None]), eta, th).reshape(eta.shape)
    return float(np.mean(yrep.var(axis=0) >= y.var()))


def test_end_to_end_bands_hold_for_the_reference_alone():
    """The data seed is chosen so that the reference ALONE -- Laplace draws and the NumPy samplers, 256 draws -- is inside the
    bands the GPU test asserts, with room: (0.1, 0.9) where the model is right, 0 where it is wrong."""
    X, y_p, y_nb = e2e_data()
    rs = np.random.RandomState(1)
    p_right = reference_pvalue_var(X, y_p, "poisson", laplace_draws(X, y_p, "poisson", 256, rs), 11)
    p_wrong = reference_pvalue_var(X, y_nb, "poisson", laplace_draws(X, y_nb, "poisson", 256, rs), 11)
    p_fixed = reference_pvalue_var(X, y_nb, "negbinomial", laplace_draws(X, y_nb, "negbinomial", 256, rs), 11)
    print("reference p-values of the variance: poisson on poisson %.3f, poisson on negbinomial %.3f, negbinomial on negbinomial %.3f"
          % (p_right, p_wrong, p_fixed))
    assert 0.1 < p_right < 0.9 and p_wrong == 0.0 and 0.1 < p_fixed < 0.9


def posterior_draws(P, pot, step, L):
    """One draw per chain at the end of a short run.  Trajectories of about a quarter period of the stiffest direction (the
    intercept: curvature ~ sum of the fitted means), so that 200 iterations forget the start."""
    from scipy.constants import k as kB
    hmc = P.HMC(P.Ensemble(pot.numDimensions, E2E_CHAINS), L * step, step, None, potential=pot, rng="philox", seed=5, verbose=False)
    s, _ = hmc.getSamples(200, 1 / kB, 0.1, device_output=True)
    return s[:, :, -1:]


@pytest.mark.gpu
def test_end_to_end_the_variance_check_tells_the_models_apart(P):
    """7. Poisson data under the Poisson model: pvalue("var") inside (0.05, 0.95); over-dispersed counts (negative binomial,
    phi = 0.5) under the Poisson model: < 0.01; under the negative-binomial model: inside (0.05, 0.95).  M = 256, 2048 chains."""
    X, y_p, y_nb = e2e_data()
    right = P.GLM(X, y_p, family="poisson")
    p_right = right.predictive(posterior_draws(P, right, 0.02, 3), seed=1).pvalue("var")
    wrong = P.GLM(X, y_nb, family="poisson")
    p_wrong = wrong.predictive(posterior_draws(P, wrong, 0.02, 3), seed=1).pvalue("var")
    fixed = P.DispersionGLM(X, y_nb, family="negbinomial")
    r = fixed.predictive(posterior_draws(P, fixed, 0.04, 4), seed=1)
    print("p-values of the variance: %.3f, %.4f, %.3f" % (p_right, p_wrong, r.pvalue("var")))
    assert 0.05 < p_right < 0.95
    assert p_wrong < 0.01
    assert 0.05 < r.pvalue("var") < 0.95
    assert np.all(np.isfinite(r.var)) and r.var.shape == (E2E_CHAINS, 1)
