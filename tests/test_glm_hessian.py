"""The Hessian of a GLM potential at one state on the device (csrc/kernels_glm_hessian.hip, pbbi_glm_hessian; laplace.hessian).

Reference: the U_i of include/pbbi.h differentiated in closed form (the formulas of include/pbbi_glm_hessian.h, written out
again here), evaluated in `numpy.longdouble`; psi, psi' and the whole per-observation d2U_i/dtheta2 of the negative binomial and
the Gamma family, and their sums over the observations, in mpmath at 50 digits.  The closed forms themselves are held against
mpmath.diff of U_i (test_closed_forms_against_mpmath_diff; no GPU).

Bound, entrywise:  |H - H_ref|_ab <= TOL * scale_ab,  scale_ab = sum_i |d2U_i| |x_ia| |x_ib| + |prior_ab|  (the theta row and
column with |k_i| |x_ia| resp. |d2U_i/dtheta2|).

TOL is measured, not chosen: the same closed form in plain float64 NumPy (scipy's digamma / polygamma) against the reference
over exactly the inputs of this file, the largest ratio |H_f64 - H_ref| / scale over every entry of every case, times 16 for
the device's different summation order and exp:

    MEASURED_RATIO = 2.0e-15   (1.95e-15, at negbinomial_sampled_d2's theta-theta entry; the other cases 1e-16 .. 8e-16.
                                `python tests/test_glm_hessian.py` prints them; test_tolerance_is_the_measured_one holds it)
    TOL            = 16 * MEASURED_RATIO = 3.2e-14

Inputs are drawn with |eta| <= 3 and |theta| <= 1, so the link does not amplify the rounding of eta beyond what the float64
evaluation shows.  Shapes: the smallest that reach each way the kernel can go wrong (CASES).
"""
import functools

import numpy as np
import pytest

LD = np.longdouble
MEASURED_RATIO = 2.0e-15
TOL = 16 * MEASURED_RATIO

# name: (class, family, D, M, what it reaches)
CASES = {
    "logistic_plain_d3": ("GLM", "logistic", 3, 17, "one tile, block boundary"),
    "poisson_full_d17": ("GLM", "poisson", 17, 100, "off-diagonal tile; weight 0, offset, prior vector with a 0, prior mean"),
    "logistic_trials_d128": ("GLM", "logistic", 128, 70, "all 36 tile pairs, the wave split"),
    "poisson_plain_d33": ("GLM", "poisson", 33, 1, "padding to 64"),
    "gaussian_sampled_d15": ("DispersionGLM", "gaussian", 15, 40, "theta closes a tile"),
    "gaussian_sampled_d16": ("DispersionGLM", "gaussian", 16, 40, "theta alone in a tile"),
    "gaussian_held_d5": ("DispersionGLM", "gaussian", 5, 40, "theta from the handle"),
    "negbinomial_sampled_d63": ("DispersionGLM", "negbinomial", 63, 70, "state 64"),
    "negbinomial_sampled_d2": ("DispersionGLM", "negbinomial", 2, 40, "a small state"),
    "gamma_sampled_d127": ("DispersionGLM", "gamma", 127, 70, "state 128"),
    "gamma_held_d4": ("DispersionGLM", "gamma", 4, 40, "shape held at 1.0"),
}


@functools.lru_cache(maxsize=None)
def problem(name):
    """The model of a case as plain arrays and the state q it is evaluated at: |eta| <= 3, |theta| <= 1."""
    cls, family, D, M, _ = CASES[name]
    rs = np.random.RandomState(sorted(CASES).index(name) + 11)
    X = rs.standard_normal((M, D))
    w = rs.standard_normal(D)
    o = np.zeros(M)
    full = name == "poisson_full_d17"
    if full:
        o = rs.uniform(-0.5, 0.5, M)
    w *= 2.5 / np.max(np.abs(X @ w))               # |x.w| <= 2.5, |o| <= 0.5
    eta = X @ w + o
    a = np.ones(M)
    ntr = None
    sampled = cls == "DispersionGLM" and "sampled" in name
    held = {"gaussian_held_d5": 0.7, "gamma_held_d4": 1.0}.get(name)
    theta = rs.uniform(-1.0, 1.0) if sampled else (np.log(held) if held is not None else 0.0)
    n = D + (1 if sampled else 0)
    lam, mu = np.full(n, 1.0), np.zeros(n)
    if family == "logistic":
        if "trials" in name:
            ntr = rs.randint(1, 6, M).astype(float)
        y = rs.binomial((ntr if ntr is not None else np.ones(M)).astype(int), 1.0 / (1.0 + np.exp(-eta))).astype(float)
    elif family in ("poisson", "negbinomial"):
        y = rs.poisson(np.exp(eta)).astype(float)
    elif family == "gaussian":
        y = eta + np.exp(theta) * rs.standard_normal(M)
    else:
        y = np.exp(eta) * rs.gamma(2.0, 0.5, M)
    if full:
        a = rs.uniform(0.5, 2.0, M)
        a[7] = 0.0
        lam = rs.uniform(0.5, 3.0, n)
        lam[2] = 0.0
        mu = rs.uniform(-0.3, 0.3, n)
    if cls == "DispersionGLM":
        a = rs.uniform(0.5, 2.0, M)
        lam = rs.uniform(0.5, 3.0, n)
    q = np.r_[w, theta] if sampled else w.copy()
    plain = cls == "GLM" and not full and ntr is None
    return dict(cls=cls, family=family, X=X, y=y, a=a, ntr=ntr, o=o, lam=lam, mu=mu, sampled=sampled, theta=theta, held=held,
                q=q, plain=plain, full=full)


def build(p):
    from physicsbasedbayesianinference_amd import DispersionGLM, GLM
    if p["cls"] == "GLM":
        if p["plain"]:
            return GLM(p["X"], p["y"], p["family"], prior_precision=float(p["lam"][0]))
        return GLM(p["X"], p["y"], p["family"], prior_precision=p["lam"], prior_mean=p["mu"] if p["full"] else None,
                   weights=p["a"], offset=p["o"] if p["full"] else None, trials=p["ntr"])
    D = p["X"].shape[1]
    if p["sampled"]:
        return DispersionGLM(p["X"], p["y"], p["family"], dispersion="sample", log_dispersion_prior=(0.1, float(p["lam"][D])),
                             prior_precision=p["lam"][:D], weights=p["a"])
    return DispersionGLM(p["X"], p["y"], p["family"], dispersion=p["held"], prior_precision=p["lam"], weights=p["a"])


# ---- the closed forms -------------------------------------------------------------------------------------------------------
def _sigmoid(z):
    return 1 / (1 + np.exp(-z))


def second_derivatives(p, q, T):
    """(h, k, tt, tt_sum, tt_abs): per observation d2U_i/deta2, d2U_i/deta dtheta, d2U_i/dtheta2 in the NumPy type T, and the
    sum and absolute sum of the last over the observations -- in mpmath at 50 digits when T is longdouble and the family has
    psi terms, else in T."""
    X, y, a, o = (np.asarray(v, dtype=T) for v in (p["X"], p["y"], p["a"], p["o"]))
    D = X.shape[1]
    w = np.asarray(q[:D], dtype=T)
    theta = T(q[D]) if p["sampled"] else T(p["theta"])
    eta = X @ w + o
    fam = p["family"]
    zero = np.zeros_like(eta)
    if fam == "logistic":
        c = a * (np.asarray(p["ntr"], dtype=T) if p["ntr"] is not None else 1)
        s = _sigmoid(eta)
        return c * s * (1 - s), zero, zero, T(0), T(0)
    if fam == "poisson":
        return a * np.exp(eta), zero, zero, T(0), T(0)
    if fam == "gaussian":
        tau, e = np.exp(-2 * theta), y - eta
        tt = 2 * a * tau * e * e
        return a * tau + zero, 2 * a * tau * e, tt, np.sum(tt), np.sum(np.abs(tt))
    if fam == "negbinomial":
        phi, s = np.exp(theta), _sigmoid(eta - theta)
        h = a * (y + phi) * s * (1 - s)
        k = a * (phi * s - (y + phi) * s * (1 - s))
    else:
        alpha, z = np.exp(theta), eta - np.log(y)
        h = a * alpha * np.exp(-z)
        k = a * alpha * (1 - np.exp(-z))
    if T is LD:
        import mpmath as mp
        with mp.workdps(50):
            th = mp.mpf(float(theta)) + mp.mpf(float(theta - LD(float(theta))))
            terms = []
            for i in range(eta.size):
                et = mp.mpf(float(eta[i])) + mp.mpf(float(eta[i] - LD(float(eta[i]))))
                yi, ai = mp.mpf(float(y[i])), mp.mpf(float(a[i]))
                if fam == "negbinomial":
                    ph = mp.exp(th)
                    z = et - th
                    si = 1 / (1 + mp.exp(-z))
                    sp = mp.log(1 + mp.exp(z))
                    terms.append(ai * (ph * (mp.digamma(ph) - mp.digamma(yi + ph) + sp - si)
                                       + ph * ph * (mp.polygamma(1, ph) - mp.polygamma(1, yi + ph)) - ph * si * si
                                       + yi * si * (1 - si)))
                else:
                    al = mp.exp(th)
                    z = et - mp.log(yi)
                    terms.append(ai * al * (mp.digamma(al) - th - 1 + z + mp.exp(-z) + al * mp.polygamma(1, al) - 1))
            tt = np.array([LD(float(t)) + LD(float(t - mp.mpf(float(t)))) for t in terms], dtype=LD)
            tot, tab = mp.fsum(terms), mp.fsum([abs(t) for t in terms])
            return h, k, tt, LD(float(tot)) + LD(float(tot - mp.mpf(float(tot)))), LD(float(tab))
    from scipy.special import digamma, polygamma
    if fam == "negbinomial":
        sp = np.logaddexp(0.0, eta - theta)
        tt = a * (phi * (digamma(phi) - digamma(y + phi) + sp - s) + phi * phi * (polygamma(1, phi) - polygamma(1, y + phi))
                  - phi * s * s + y * s * (1 - s))
    else:
        tt = a * alpha * (digamma(alpha) - theta - 1 + z + np.exp(-z) + alpha * polygamma(1, alpha) - 1)
    return h, k, tt, np.sum(tt), np.sum(np.abs(tt))


def assemble(p, q, T):
    """(H, scale): the n x n Hessian at q in the type T and the bound's scale."""
    h, k, _, tt_sum, tt_abs = second_derivatives(p, q, T)
    X = np.asarray(p["X"], dtype=T)
    D = X.shape[1]
    n = D + (1 if p["sampled"] else 0)
    lam = np.asarray(p["lam"], dtype=T)
    H, sc = np.zeros((n, n), dtype=T), np.zeros((n, n), dtype=T)
    H[:D, :D] = X.T @ (h[:, None] * X)
    sc[:D, :D] = np.abs(X).T @ (np.abs(h)[:, None] * np.abs(X))
    if p["sampled"]:
        H[:D, D] = H[D, :D] = X.T @ k
        sc[:D, D] = sc[D, :D] = np.abs(X).T @ np.abs(k)
        H[D, D], sc[D, D] = tt_sum, tt_abs
    H[np.diag_indices(n)] += lam
    sc[np.diag_indices(n)] += np.abs(lam)
    return H, sc


@functools.lru_cache(maxsize=None)
def reference(name):
    p = problem(name)
    return assemble(p, p["q"], LD)


def float64_ratio(name):
    """The largest |H_f64 - H_ref| / scale of a case: what plain float64 arithmetic makes of the same closed form."""
    p = problem(name)
    H, sc = reference(name)
    H64, _ = assemble(p, p["q"], np.float64)
    return float(np.max(np.abs(H64.astype(LD) - H) / sc))


def ratio(H, name):
    Href, sc = reference(name)
    return float(np.max(np.abs(np.asarray(H, dtype=LD) - Href) / sc))


# ---- no GPU: the reference itself -------------------------------------------------------------------------------------------
def test_tolerance_is_the_measured_one():
    worst = max(float64_ratio(name) for name in CASES)
    print("float64 closed form against the reference: largest ratio %.3g (recorded %.3g, TOL %.3g)" % (worst, MEASURED_RATIO, TOL))
    assert worst <= MEASURED_RATIO
    assert worst >= MEASURED_RATIO / 4, "the recorded ratio is stale: measure again"


@pytest.mark.parametrize("name", ["logistic_trials_d128", "poisson_full_d17", "gaussian_sampled_d15", "negbinomial_sampled_d2",
                                  "gamma_sampled_d127"])
def test_closed_forms_against_mpmath_diff(name):
    import mpmath as mp
    p = problem(name)
    h, k, tt, _, _ = second_derivatives(p, p["q"], LD)
    X, D = p["X"], p["X"].shape[1]
    eta = X @ p["q"][:D] + p["o"]
    theta0 = p["q"][D] if p["sampled"] else p["theta"]
    fam = p["family"]
    with mp.workdps(50):
        for i in (0, 3, len(eta) - 1):
            yi, ai = mp.mpf(float(p["y"][i])), mp.mpf(float(p["a"][i]))
            ni = mp.mpf(float(p["ntr"][i])) if p["ntr"] is not None else mp.mpf(1)

            def U(e, th):
                if fam == "logistic":
                    return ai * (ni * mp.log(1 + mp.exp(e)) - yi * e)
                if fam == "poisson":
                    return ai * (mp.exp(e) - yi * e)
                if fam == "gaussian":
                    return ai * (mp.mpf(0.5) * mp.exp(-2 * th) * (yi - e) ** 2 + th)
                if fam == "negbinomial":
                    ph = mp.exp(th)
                    return ai * (mp.loggamma(ph) - mp.loggamma(yi + ph) - ph * th - yi * e
                                 + (yi + ph) * (th + mp.log(1 + mp.exp(e - th))))
                al, z = mp.exp(th), e - mp.log(yi)
                return ai * (mp.loggamma(al) - al * th + al * (z + mp.exp(-z)))
            pt = (mp.mpf(float(eta[i])), mp.mpf(float(theta0)))
            for got, order in ((h[i], (2, 0)), (k[i], (1, 1)), (tt[i], (0, 2))):
                want = float(mp.diff(U, pt, order))
                assert abs(float(got) - want) <= 1e-9 * max(1.0, abs(want)), (name, i, order, float(got), want)


# ---- on the device ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_hessian(name, ranges):
    from physicsbasedbayesianinference_amd import laplace
    p = problem(name)
    pot = build(p)
    return laplace.hessian(pot, p["q"], ranges=ranges)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("ranges", [0, 1, 5])
@pytest.mark.parametrize("name", sorted(CASES))
def test_hessian_within_bound(name, ranges):
    H = device_hessian(name, ranges)
    r = ratio(H, name)
    print("%s ranges=%d: largest |H - H_ref| / scale = %.3g (TOL %.3g)" % (name, ranges, r, TOL))
    assert np.array_equal(bits(H), bits(H.T)), "H is not symmetric bit for bit"
    assert r <= TOL


@pytest.mark.gpu
def test_empty_ranges_add_exact_zeros():
    H = device_hessian("logistic_plain_d3", 9)      # M = 17: 4 padded blocks, one stage, 8 empty ranges
    r = ratio(H, "logistic_plain_d3")
    print("ranges=9 at M=17: %.3g" % r)
    assert r <= TOL
    assert np.array_equal(bits(H), bits(device_hessian("logistic_plain_d3", 1)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["poisson_full_d17", "negbinomial_sampled_d63"])
def test_same_ranges_same_bits(name):
    from physicsbasedbayesianinference_amd import laplace
    p = problem(name)
    pot = build(p)
    for ranges in (0, 2):
        assert np.array_equal(bits(laplace.hessian(pot, p["q"], ranges)), bits(laplace.hessian(pot, p["q"], ranges)))


@pytest.mark.gpu
def test_weight_zero_row_with_overflowing_eta_adds_exactly_nothing():
    from physicsbasedbayesianinference_amd import GLM, laplace
    p = problem("poisson_full_d17")
    rs = np.random.RandomState(5)
    X1 = np.vstack([p["X"], rs.standard_normal((1, p["X"].shape[1]))])
    kw = dict(prior_precision=p["lam"], prior_mean=p["mu"])
    with_row = GLM(X1, np.r_[p["y"], 3.0], "poisson", weights=np.r_[p["a"], 0.0], offset=np.r_[p["o"], 800.0], **kw)
    without = GLM(p["X"], p["y"], "poisson", weights=p["a"], offset=p["o"], **kw)
    for ranges in (0, 1):
        H1, H0 = laplace.hessian(with_row, p["q"], ranges), laplace.hessian(without, p["q"], ranges)
        assert np.all(np.isfinite(H1))
        assert np.array_equal(bits(H1), bits(H0))


@pytest.mark.gpu
def test_central_differences_of_the_gradient():
    """A cap on truncation error (step 1e-5: h^2 f''' / 6 ~ 1e-11 relative, rounding 1e-16 / 1e-5), not a precision claim."""
    name = "logistic_plain_d3"
    p = problem(name)
    pot = build(p)
    H = device_hessian(name, 0)
    _, sc = reference(name)
    n, step = p["q"].size, 1e-5
    Q = np.repeat(p["q"][:, None], 2 * n, axis=1)
    for b in range(n):
        Q[b, 2 * b] += step
        Q[b, 2 * b + 1] -= step
    g = pot.gradient(Q)
    fd = np.stack([(g[:, 2 * b] - g[:, 2 * b + 1]) / (2 * step) for b in range(n)], axis=1)
    err = float(np.max(np.abs(fd - H) / sc.astype(np.float64)))
    print("central differences: %.3g" % err)
    assert err <= 1e-6


@pytest.mark.gpu
def test_handles_refused_on_the_device_entry():
    from physicsbasedbayesianinference_amd import HierarchicalGLM, OrdinalGLM, SoftmaxGLM, StandardGaussian, _lib, laplace
    rs = np.random.RandomState(0)
    X = rs.standard_normal((20, 3))
    pots = [SoftmaxGLM(X, rs.randint(0, 3, 20).astype(float), classes=3), OrdinalGLM(X, rs.randint(0, 3, 20).astype(float), 3),
            HierarchicalGLM(X, rs.randint(0, 2, 20).astype(float), groups=[0, 0, -1]), StandardGaussian(3)]
    for pot in pots:
        with pytest.raises((_lib.PbbiError, ValueError)) as e:
            laplace.hessian(pot, np.zeros(pot.numDimensions))
        assert "pbbi_glm_hessian" in str(e.value), str(e.value)


if __name__ == "__main__":
    for nm in sorted(CASES):
        print("%-28s %.3g" % (nm, float64_ratio(nm)))
    print("largest: %.3g" % max(float64_ratio(nm) for nm in CASES))
