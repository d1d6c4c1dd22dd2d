"""The dense metric of the GLM kernels (METRIC = GLM_METRIC_DENSE of k_glm, pbbi_potential_set_metric_dense): chain n has the mass
matrix m_n M, M = L L^T, C = M^-1 -- p = sqrt(m_n kT) L z, v = C p / m_n, the kick -c h C g / m_n, K = 0.5 p^T C p / m_n.

The reference is a NumPy restatement, below, of test_glm_metric.py's restatement (r_integrate, r_hamiltonian, r_hmc_iter, r_run:
the oracle's loop with the masses replaced) with the matrix in place of the diagonal; U and grad U from oracle.potential, the
draws from oracle.philox_normal / philox_uniform.  test_dense_restatement_is_the_diagonal_one_at_a_diagonal_matrix holds it to
that file's restatement first, which that file holds to the oracle.

Handles, starts, step sizes and conventions are test_glm_frame.py's (N = 150, seed 4, iteration 1, chain0 = 2^32 - 70, MASS, kT =
2.5, S = 3, both methods), tolerance test_glm.check (rel <= 1e-10), masks equal with no chain excluded.  The metric of a handle
is test_glm_dense_metric_host.dense_metric_of(Dt) = R diag(30^((d + 0.5) / Dt)) R^T, R a seeded random orthogonal matrix: fully
dense, condition number < 30, no symmetry a wrong row mapping could hide behind."""
import ctypes as C
import functools

import numpy as np
import pytest

import test_glm_dispersion as t_disp
import test_glm_frame as F
import test_glm_gamma as t_gamma
import test_glm_metric as TM
from oracle import oracle as orc
from test_glm import check     # rel <= TOL = 1e-10, both of that file
from test_glm_dense_metric_host import dense_metric_of
from test_glm_metric import _flags, _margin, metric_of

N, SEED, ITER0, CHAIN0, MASS, KT, S_RUN, METHODS = F.N, F.SEED, F.ITER0, F.CHAIN0, F.MASS, F.KT, F.S_RUN, F.METHODS
# name -> (device factory, oracle potential, the (Dt, >= N) start), (h Leapfrog, h Stormer-Verlet), L
FRAME_NAMES = ["logistic", "logistic17", "logistic50", "poisson_full", "gaussian_sampled", "negbinomial_held"]
NAMES = FRAME_NAMES + ["logistic64", "gamma"]
ITER_NAMES = ["logistic", "gaussian_sampled"]
CANARY_NAMES = ["logistic", "logistic17", "logistic50"]
_BUILT, _DEVICE = {}, {}


def _kind(name):
    if name not in _BUILT:
        if name in FRAME_NAMES:
            _BUILT[name] = F._kind(name) + (F.KINDS[name]["h"], F.KINDS[name]["L"])
        elif name == "logistic64":                                   # no padding row at all
            dev, op, q = F._plain(64)
            q.setflags(write=False)
            _BUILT[name] = (dev, op, q, (0.22, 0.22), 8)
        else:                                                        # gamma, theta sampled: as test_glm_gamma builds its own
            kw, q = t_gamma.metric_inputs(5)
            q.setflags(write=False)
            _, hs, L = t_gamma.METRIC_CASES[5]
            _BUILT[name] = ((lambda P: t_gamma.make(P, kw, True)), t_gamma.oracle_pot(kw, True), q, hs, L)
    return _BUILT[name]


def _q0(name, n=N):
    return np.array(_kind(name)[2][:, :n], order="C")      # (a copy: the restatement works in place)


RUN_ROWS = [(me, b, c) for me in METHODS for b in (False, True) for c in (False, True)]
RUN_CASES = [("run", name) + row for name in NAMES for row in RUN_ROWS]
ITER_CASES = [("iter", name, me) for name in ITER_NAMES for me in METHODS]
# case -> step size where the handle's own leaves an accept test within 1e-7 of its uniform or no chain of either outcome
# (test_dense_metric_cases_are_decisive picks these)
STEP = {}


def _h(case):
    return STEP.get(case, _kind(case[1])[3][METHODS.index(case[2])])


# ---- the restatement ------------------------------------------------------------------------------------------------
def _m(q, mass):
    return np.ones(q.shape[1]) if mass is None else np.asarray(mass, float)


def _accel(op, q, Cm, m):
    return -(Cm @ orc.potential(op, np.ascontiguousarray(q), want_grad=True)[1]) / m     # -C g / m_n


def d_integrate(op, method, q, p, mass, Md, h, L):
    """TM.r_integrate with v = C p / m_n, a = -C g / m_n and p = m_n M v at the end; in place on q, p (D, N); returns v."""
    Cm, m = np.linalg.inv(Md), _m(q, mass)
    h2 = h * h
    v = (Cm @ p) / m
    if method == "Leapfrog":
        a = _accel(op, q, Cm, m)
        for _ in range(L):
            q += (v * h + (0.5 * a) * h2)
            an = _accel(op, q, Cm, m)
            v += (0.5 * (a + an)) * h
            a = an
    else:
        qpast = q.copy()
        a = _accel(op, q, Cm, m)
        q[:] = (q + v * h) + (0.5 * a) * h2
        for _ in range(L):
            a = _accel(op, q, Cm, m)
            cur = q.copy()
            q[:] = (2 * cur - qpast) + a * h2
            qpast = cur
        v = (q - qpast) / h
    p[:] = (Md @ v) * m
    return v


def d_hamiltonian(op, q, p, mass, Md):
    """0.5 p^T C p / m_n + U(q)."""
    Cm = np.linalg.inv(Md)
    return 0.5 * np.sum(p * (Cm @ p), axis=0) / _m(q, mass) + orc.potential(op, np.ascontiguousarray(q))


def d_hmc_iter(op, method, q, p, u, mass, Md, h, L, compat, beta=1.0):
    """TM.r_hmc_iter on the two functions above."""
    oq, opp = q.copy(), p.copy()
    d_integrate(op, method, q, p, mass, Md, h, L)
    oldH = d_hamiltonian(op, oq, opp, mass, Md)
    newH = d_hamiltonian(op, q, -p, mass, Md)
    with np.errstate(over="ignore"):
        ratio = np.exp((oldH - newH) * beta)
    rej = u > np.minimum(1.0, ratio)
    q[:, rej] = oq[:, rej]
    p[:, rej] = (oq if compat else opp)[:, rej]
    return ratio, rej


def d_draw(Md, mass, kT, seed, it, chain0, D, n):
    """p = sqrt(m_n kT) L z, z the Philox normals of the double-precision draw."""
    z = orc.philox_normal(seed, orc.STREAM_MOMENTUM | orc.STREAM_DRAW_F64, it, chain0, D, n)
    m = np.ones(n) if mass is None else np.asarray(mass, float)
    return np.ascontiguousarray((np.linalg.cholesky(Md) @ z) * np.sqrt(m * kT))


def d_run(op, method, q, mass, Md, h, L, S, seed, iter0, chain0, kT, beta_accept, compat):
    """TM.r_run with the draw above."""
    D, n = q.shape
    out = [np.empty((S, D, n)), np.empty((S, D, n)), np.empty((S, n), bool), np.empty((S, n)), np.empty((S, n))]
    for i in range(S):
        p = d_draw(Md, mass, kT, seed, iter0 + i, chain0, D, n)
        u = orc.philox_uniform(seed, iter0 + i, chain0, n)
        ratio, rej = d_hmc_iter(op, method, q, p, u, mass, Md, h, L, compat, 1.0 / kT if beta_accept else 1.0)
        out[0][i], out[1][i], out[2][i], out[3][i], out[4][i] = q, p, rej, ratio, u
    return out


@functools.lru_cache(maxsize=None)
def _ref(case):
    """The restatement's result of a case under the handle's dense metric, computed once and left unchanged."""
    name = case[1]
    _, op, _, _, L = _kind(name)
    h = _h(case)
    q = _q0(name)
    Md = dense_metric_of(q.shape[0])
    if case[0] == "run":
        _, _, method, beta, compat = case
        s, p, rej, ratio, u = d_run(op, method, q, MASS, Md, h, L, S_RUN, SEED, ITER0, CHAIN0, KT, beta, compat)
        return F._frozen(samples=s, momenta=p, rej=rej, ratio=ratio, u=u, q=q)
    _, _, method = case
    p_in = d_draw(Md, MASS, KT, SEED, ITER0, CHAIN0, q.shape[0], N)
    u = orc.philox_uniform(SEED, ITER0, CHAIN0, N)
    p = p_in.copy()
    ratio, rej = d_hmc_iter(op, method, q, p, u, MASS, Md, h, L, False, 1.0 / KT)
    return F._frozen(q=q, p=p, p_in=p_in, rej=rej, ratio=ratio, u=u)


# ---- CPU --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["logistic", "gaussian_sampled"])
def test_dense_restatement_is_the_diagonal_one_at_a_diagonal_matrix(name):
    """With M = diag(m_d) the restatement above agrees with test_glm_metric's to 1e-12 on q, p, v, H and ratio, both methods,
    compat and non-compat, beta = 1 and 1 / 2.5, masks equal; and its run (the draw L z = sqrt(m_d) z) likewise."""
    _, op, _, hs, L = _kind(name)
    q0 = _q0(name, 40)
    Dt = q0.shape[0]
    mass, md = MASS[:40], metric_of(Dt)
    Md = np.diag(md)
    p0 = d_draw(Md, mass, KT, SEED, ITER0, CHAIN0, Dt, 40)
    check(f"{name} draw", p0, orc.philox_normal(SEED, orc.STREAM_MOMENTUM | orc.STREAM_DRAW_F64, ITER0, CHAIN0, Dt, 40)
          * np.sqrt(TM._mass2(q0, mass, md) * KT), tol=1e-12)
    u = orc.philox_uniform(SEED, ITER0, CHAIN0, 40)
    check(f"{name} H", d_hamiltonian(op, q0, p0, mass, Md), TM.r_hamiltonian(op, q0, p0, mass, md), tol=1e-12)
    for mi, method in enumerate(METHODS):
        h = hs[mi]
        q, p, rq, rp = q0.copy(), p0.copy(), q0.copy(), p0.copy()
        v, rv = d_integrate(op, method, q, p, mass, Md, h, L), TM.r_integrate(op, method, rq, rp, mass, md, h, L)
        for tag, a, b in (("q", q, rq), ("p", p, rp), ("v", v, rv)):
            check(f"{name} {method} integrate {tag}", a, b, tol=1e-12)
        for compat in (False, True):
            for beta in (1.0, 1.0 / KT):
                q, p, rq, rp = q0.copy(), p0.copy(), q0.copy(), p0.copy()
                ratio, rej = d_hmc_iter(op, method, q, p, u, mass, Md, h, L, compat, beta)
                rratio, rrej = TM.r_hmc_iter(op, method, rq, rp, u, mass, md, h, L, compat, beta)
                assert np.array_equal(rej, rrej), (name, method, compat, beta)
                for tag, a, b in (("q", q, rq), ("p", p, rp), ("ratio", ratio, rratio)):
                    check(f"{name} {method} compat={compat} beta={beta:.1f} iter {tag}", a, b, tol=1e-12)
    q, rq = q0.copy(), q0.copy()
    got = d_run(op, "Leapfrog", q, mass, Md, hs[0], L, S_RUN, SEED, ITER0, CHAIN0, KT, True, False)
    want = TM.r_run(op, "Leapfrog", rq, mass, md, hs[0], L, S_RUN, SEED, ITER0, CHAIN0, KT, True, False)
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[4], want[4])
    for tag, a, b in (("samples", got[0], want[0]), ("momenta", got[1], want[1]), ("ratio", got[3], want[3]), ("state", q, rq)):
        check(f"{name} run {tag}", a, b, tol=1e-12)


@pytest.mark.parametrize("name", NAMES)
def test_dense_metric_cases_are_decisive(name):
    """The restatement alone, for every case of the GPU tests below: every value finite, no accept test within 1e-7 (relative
    to max(1, ratio)) of its uniform, and a reject fraction strictly between 0 and 1 -- so that "masks are equal" is a fair
    demand on the device at 1e-10."""
    for case in (c for c in RUN_CASES + ITER_CASES if c[1] == name):
        o = _ref(case)
        assert all(np.all(np.isfinite(v)) for k, v in o.items() if k in ("samples", "momenta", "q", "p")), case
        _margin(str(case), o["ratio"], o["u"])
        assert 0 < int(o["rej"].sum()) < o["rej"].size, (case, int(o["rej"].sum()))
    Md = dense_metric_of(_q0(name).shape[0])
    ev = np.linalg.eigvalsh(Md)
    assert np.array_equal(Md, Md.T) and 1.0 < ev[0] and ev[-1] < 30.0 and np.all(Md != 0.0)
    off = Md - np.diag(np.diag(Md))
    assert Md.shape[0] == 1 or np.max(np.abs(off)) > 0.05 * np.max(np.diag(Md))     # dense in earnest


# ---- the statistical case: two predictors with posterior correlation 0.99 ------------------------------------------------
G_N, G_H, G_L, G_S = 4096, 0.5, 4, 4
G_LAM, G_SIGMA, G_RHO = 0.01, 0.7, 0.99
G_T = 1.5          # adaptMassMatrix's trajectory length (test_glm_metric.G_T says why)


@functools.lru_cache(maxsize=None)
def _gauss():
    """Gaussian family, sigma held, M = 64, D = 3: X = Q A with Q orthonormal and A^T A / sigma^2 + lam I = H the inverse of
    [[1, rho, 0], [rho, 1, 0], [0, 0, 1]] -- unit posterior scales, rows 0 and 1 correlated 0.99.  The posterior is N(mu,
    H^-1) exactly."""
    rs = np.random.RandomState(31)
    Q, _ = np.linalg.qr(rs.standard_normal((64, 3)))
    S = np.array([[1.0, G_RHO, 0.0], [G_RHO, 1.0, 0.0], [0.0, 0.0, 1.0]])
    A = np.linalg.cholesky(np.linalg.inv(S) - G_LAM * np.eye(3)).T * G_SIGMA
    X = np.ascontiguousarray(Q @ A)
    y = X @ np.array([0.8, -0.3, 0.05]) + G_SIGMA * rs.standard_normal(64)
    kw = dict(X=X, y=y, family="gaussian", weights=None, offset=None, prior_precision=G_LAM, prior_mean=None)
    H = X.T @ X / G_SIGMA ** 2 + G_LAM * np.eye(3)
    H = 0.5 * (H + H.T)
    cov = np.linalg.inv(H)
    mu = cov @ (X.T @ y) / G_SIGMA ** 2
    sd = np.sqrt(np.diag(cov))
    assert abs(cov[0, 1] / (sd[0] * sd[1]) - G_RHO) < 1e-9 and np.allclose(sd, 1.0, rtol=1e-9)
    q0 = np.ascontiguousarray(mu[:, None] + np.linalg.cholesky(cov) @ rs.standard_normal((3, G_N)))     # a stationary start
    q0.setflags(write=False)
    return kw, H, cov, mu, q0


def _gauss_op():
    return t_disp.oracle_pot(_gauss()[0], False, float(np.log(G_SIGMA)))


def _gauss_pot(P):
    return t_disp.make(P, _gauss()[0], False, float(np.log(G_SIGMA)))


@functools.lru_cache(maxsize=None)
def _gauss_cpu(dense):
    """The restatement at the GPU test's sizes: reject masks, ratios and uniforms of G_S iterations of G_N chains under M = H
    (dense) or under the best diagonal metric 1 / diag(H^-1)."""
    kw, H, cov, mu, q0 = _gauss()
    q = q0.copy()
    if dense:
        _, _, rej, ratio, u = d_run(_gauss_op(), "Leapfrog", q, None, H, G_H, G_L, G_S, SEED, ITER0, 0, 1.0, False, False)
    else:
        _, _, rej, ratio, u = TM.r_run(_gauss_op(), "Leapfrog", q, None, 1.0 / np.diag(cov), G_H, G_L, G_S, SEED, ITER0, 0, 1.0,
                                       False, False)
    return rej, ratio, u


def test_correlated_gaussian_on_the_restatement():
    """The model is what it claims (the oracle's potential is 0.5 (w - mu)^T H (w - mu) + const), and on the CPU alone: with M
    = H the restatement accepts >= 0.9 and no accept test is within 1e-7 of its uniform; with the best diagonal metric
    h omega_max = 0.5 / sqrt(1 - 0.99) = 5 > 2 and it accepts <= 0.05."""
    kw, H, cov, mu, q0 = _gauss()
    op = _gauss_op()
    U, g = orc.potential(op, np.ascontiguousarray(q0[:, :50]), want_grad=True)
    U0 = orc.potential(op, np.ascontiguousarray(mu[:, None]))[0]
    d = q0[:, :50] - mu[:, None]
    check("gradient", g, H @ d, tol=1e-9)
    check("U", U - U0, 0.5 * np.sum(d * (H @ d), axis=0), tol=1e-9)
    rej, ratio, u = _gauss_cpu(True)
    _margin("correlated gaussian, M = H", ratio, u)
    assert 1.0 - rej.mean() >= 0.9, 1.0 - rej.mean()
    rej_d = _gauss_cpu(False)[0]
    assert 1.0 - rej_d.mean() <= 0.05, 1.0 - rej_d.mean()
    assert abs(G_H / np.sqrt(1.0 - G_RHO) - 5.0) < 1e-12


# ---- GPU --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def P():
    import physicsbasedbayesianinference_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def lib():
    from physicsbasedbayesianinference_amd import _lib
    _lib.load()
    return _lib


def _fresh(P, name):
    """The handle of a kind WITHOUT a metric (this file's own: test_glm_frame's are left alone)."""
    if ("fresh", name) not in _DEVICE:
        _DEVICE[("fresh", name)] = _kind(name)[0](P)
    return _DEVICE[("fresh", name)]


def _mpot(P, name, M=None):
    """A second handle of the kind, carrying dense_metric_of(Dt) or the matrix / vector given."""
    if name not in _DEVICE:
        _DEVICE[name] = _kind(name)[0](P)
    pot = _DEVICE[name]
    pot.set_metric(dense_metric_of(pot.numDimensions) if M is None else M)
    return pot


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_dense_metric_run_vs_restatement(P, lib, name):
    """1: pbbi_hmc_run on a handle with a dense metric, S = 3, kT = 2.5, MASS, PBBI_DRAW_F64, leading stride N + 5: {Leapfrog,
    Stormer-Verlet} x {0, PBBI_BETA_ACCEPT} x {non-compat, PBBI_COMPAT_P_FROM_OLDQ} against the restatement -- samples,
    momenta (the parked draw sqrt(m_n kT) L z of a rejected non-compat chain among them), ratios, the final state within TOL;
    masks equal; padding columns untouched.  The handle reports its metric back, 2-D."""
    pot, L = _mpot(P, name), _kind(name)[4]
    assert np.array_equal(pot.metric, dense_metric_of(pot.numDimensions)) and pot.metric.ndim == 2
    for case in (c for c in RUN_CASES if c[1] == name):
        _, _, method, beta, compat = case
        o = _ref(case)
        _margin(str(case), o["ratio"], o["u"])
        gs, gm, grej, gratio, gq, gpad = F._device_run(lib, pot, method, _q0(name), MASS, _h(case), L, S_RUN,
                                                       _flags(lib, beta, compat), KT, pad=5)
        tag = f"{name} {method} beta_accept={beta} compat={compat}"
        print(tag, "mask mismatches", int((grej != o["rej"]).sum()), "rejected", int(grej.sum()))
        assert np.array_equal(grej, o["rej"]), tag
        check(tag + " samples", gs, o["samples"])
        check(tag + " momenta", gm, o["momenta"])
        check(tag + " ratio", gratio, o["ratio"])
        check(tag + " final state", gq, o["q"])
        assert np.all(gpad == F.POISON), tag


@pytest.mark.gpu
@pytest.mark.parametrize("name", ITER_NAMES)
def test_dense_metric_uploaded_draws_vs_restatement(P, lib, name):
    """2a: pbbi_hmc_iter_kt with uploaded momenta (p as given) and uniforms, PBBI_BETA_ACCEPT at kT = 2.5, non-compat, both
    methods: masks equal, q, p, ratio within TOL, a rejected chain's p_out is its p_in bit for bit."""
    pot, L = _mpot(P, name), _kind(name)[4]
    for case in (c for c in ITER_CASES if c[1] == name):
        method = case[2]
        o = _ref(case)
        _margin(str(case), o["ratio"], o["u"])
        rj = o["rej"]
        gq, gp, gratio, grej = F._device_iter(lib, pot, method, _q0(name), o["p_in"], o["u"], MASS, _h(case), L,
                                              lib.BETA_ACCEPT, KT)
        tag = f"{name} {method}"
        assert np.array_equal(grej, rj) and 0 < rj.sum() < N, tag
        check(tag + " q", gq, o["q"])
        check(tag + " p", gp, o["p"])
        check(tag + " ratio", gratio, o["ratio"])
        assert np.array_equal(gp[:, rj], o["p_in"][:, rj]) and np.array_equal(gq[:, rj], _q0(name)[:, rj]), tag


@pytest.mark.gpu
@pytest.mark.parametrize("name", ITER_NAMES)
def test_dense_metric_integrate_and_energies_vs_restatement(P, lib, name):
    """2b: pbbi_leapfrog, pbbi_stormer_verlet (q, p in place), pbbi_integrate's v_out (v = C p / m_n), pbbi_energy (H and
    exp(-H)) and pbbi_weights_ratio against the restatement under the dense metric, with MASS; pbbi_potential_eval does not
    see the metric."""
    import torch
    d = F._dev()
    pot, op, L = _mpot(P, name), _kind(name)[1], _kind(name)[4]
    q0 = _q0(name)
    Dt = q0.shape[0]
    Md = dense_metric_of(Dt)
    p0 = np.array(_ref(("iter", name, "Leapfrog"))["p_in"])
    mdev, st = d.as_device(MASS, 0, np.float64), d.stream_ptr(0)
    ends = {}
    for mi, method in enumerate(METHODS):
        h = _kind(name)[3][mi]
        q, p = q0.copy(), p0.copy()
        v = d_integrate(op, method, q, p, MASS, Md, h, L)
        ends[method] = (q, p)
        qd, pd = d.as_device(q0, 0, np.float64), d.as_device(p0, 0, np.float64)
        lib.call("pbbi_leapfrog" if method == "Leapfrog" else "pbbi_stormer_verlet", pot.handle, qd.data_ptr(),
                 pd.data_ptr(), mdev.data_ptr(), N, N, h, L, st)
        torch.cuda.synchronize()
        check(f"{name} {method} q", d.to_numpy(qd), q)
        check(f"{name} {method} p", d.to_numpy(pd), p)
        qd, pd, vd = d.as_device(q0, 0, np.float64), d.as_device(p0, 0, np.float64), d.empty((Dt, N), np.float64, 0)
        lib.call("pbbi_integrate", pot.handle, orc.METHODS[method], qd.data_ptr(), pd.data_ptr(), mdev.data_ptr(),
                 vd.data_ptr(), N, N, h, L, st)
        torch.cuda.synchronize()
        check(f"{name} {method} v", d.to_numpy(vd), v)
        check(f"{name} {method} p (integrate)", d.to_numpy(pd), p)
    H0 = d_hamiltonian(op, q0, p0, MASS, Md)
    qd, pd = d.as_device(q0, 0, np.float64), d.as_device(p0, 0, np.float64)
    Hd, wd = d.empty((N,), np.float64, 0), d.empty((N,), np.float64, 0)
    lib.call("pbbi_energy", pot.handle, qd.data_ptr(), pd.data_ptr(), mdev.data_ptr(), N, N, Hd.data_ptr(), wd.data_ptr(), st)
    torch.cuda.synchronize()
    check(f"{name} H", d.to_numpy(Hd), H0)
    assert np.max(np.abs(d.to_numpy(wd) / np.exp(-H0) - 1.0)) <= 1e-10 * max(1.0, np.max(np.abs(H0)))
    q1, p1 = ends["Leapfrog"]
    H1 = d_hamiltonian(op, q1, p1, MASS, Md)
    nq, npd = d.as_device(q1, 0, np.float64), d.as_device(p1, 0, np.float64)
    rd = d.empty((N,), np.float64, 0)
    lib.call("pbbi_weights_ratio", pot.handle, nq.data_ptr(), npd.data_ptr(), qd.data_ptr(), pd.data_ptr(), mdev.data_ptr(),
             N, N, rd.data_ptr(), st)
    torch.cuda.synchronize()
    check(f"{name} weights ratio", d.to_numpy(rd), np.exp(H0 - H1))
    U, g = orc.potential(op, q0, want_grad=True)
    Ud, gd = d.empty((N,), np.float64, 0), d.empty((Dt, N), np.float64, 0)
    lib.call("pbbi_potential_eval", pot.handle, qd.data_ptr(), N, N, Ud.data_ptr(), gd.data_ptr(), st)
    torch.cuda.synchronize()
    check(f"{name} U", d.to_numpy(Ud), U)
    check(f"{name} gradient", d.to_numpy(gd), g)


ID_ROWS = [("Leapfrog", True, False), ("Stormer-Verlet", False, True)]


def _h_id(name, method):
    """The step of a handle WITHOUT a metric.  The gamma handle's steps are test_glm_gamma's for its metric; with the unit metric
    that file runs the same handle at UNIT_H times them (at the full step chains diverge to NaN, which equals nothing)."""
    return (t_gamma.UNIT_H if name == "gamma" else 1.0) * _kind(name)[3][METHODS.index(method)]


@pytest.mark.parametrize("name", NAMES)
def test_identity_cases_are_finite_and_decisive(name):
    """The restatement alone, with M = I, for the rows of the bit-for-bit test below: every value finite (a NaN equals nothing,
    itself included), both outcomes occur over the rows, no accept test within 1e-7 of its uniform."""
    _, op, _, _, L = _kind(name)
    n_rej = n_all = 0
    for me, b, c in ID_ROWS:
        q = _q0(name)
        s, p, rej, ratio, u = d_run(op, me, q, MASS, np.eye(q.shape[0]), _h_id(name, me), L, S_RUN, SEED, ITER0, CHAIN0, KT, b, c)
        assert np.all(np.isfinite(s)) and np.all(np.isfinite(p)) and np.all(np.isfinite(q)), (name, me)
        _margin(f"identity {name} {me}", ratio, u)
        n_rej, n_all = n_rej + int(rej.sum()), n_all + rej.size
    assert 0 < n_rej < n_all, (name, n_rej, n_all)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_dense_identity_is_the_handle_without_a_metric_bit_for_bit(P, lib, name):
    """3: device against device: the dense identity's products are exact and every other operation is the kernel's without a
    metric on the same values -- samples, momenta, masks, ratios, the state and the padding bit for bit, both methods, compat
    and not.  4: dense diag(m_d) agrees with the shipped diagonal-metric run of the same handle within TOL, masks equal."""
    fresh, L, hs = _fresh(P, name), _kind(name)[4], _kind(name)[3]
    assert fresh.metric is None
    Dt = fresh.numDimensions
    want = [F._device_run(lib, fresh, me, _q0(name), MASS, _h_id(name, me), L, S_RUN, _flags(lib, b, c), KT, pad=5)
            for me, b, c in ID_ROWS]
    assert any(w[2].any() for w in want) and not all(w[2].all() for w in want)
    assert all(np.all(np.isfinite(a)) for w in want for a in (w[0], w[1], w[3], w[4])), name
    pot = _mpot(P, name)
    changed = F._device_run(lib, pot, "Leapfrog", _q0(name), MASS, _h_id(name, "Leapfrog"), L, S_RUN, _flags(lib, True, False), KT, pad=5)
    assert not np.array_equal(changed[0], want[0][0])                     # the metric in place does change the run
    pot = _mpot(P, name, np.eye(Dt))
    assert np.array_equal(pot.metric, np.eye(Dt))
    for (me, b, c), w in zip(ID_ROWS, want):
        got = F._device_run(lib, pot, me, _q0(name), MASS, _h_id(name, me), L, S_RUN, _flags(lib, b, c), KT, pad=5)
        for tag, a, r in zip(("samples", "momenta", "reject", "ratio", "state", "padding"), got, w):
            assert np.array_equal(a, r), (name, me, tag)
    md = metric_of(Dt)
    pot.set_metric(md)                                                    # the diagonal one takes the dense one's place
    assert np.array_equal(pot.metric, md)
    diag = [F._device_run(lib, pot, me, _q0(name), MASS, hs[METHODS.index(me)], L, S_RUN, _flags(lib, b, c), KT, pad=5)
            for me, b, c in ID_ROWS]
    pot.set_metric(np.diag(md))
    assert np.array_equal(pot.metric, np.diag(md))
    for (me, b, c), w in zip(ID_ROWS, diag):
        got = F._device_run(lib, pot, me, _q0(name), MASS, hs[METHODS.index(me)], L, S_RUN, _flags(lib, b, c), KT, pad=5)
        assert np.array_equal(got[2], w[2]), (name, me)
        for tag, a, r in zip(("samples", "momenta", "reject", "ratio", "state"), got, w):
            if tag != "reject":
                check(f"{name} {me} dense diag vs diagonal {tag}", a, r)
    pot.set_metric(None)
    assert pot.metric is None


CANARY_N = 37


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("name", CANARY_NAMES)
def test_dense_metric_state_inside_a_canary_allocation(P, lib, name, pad):
    """5: N = 37 chains (two full tiles and a ragged one of 5, a ghost wave) under the dense metric, the state, momentum and
    output arrays rows [1, 1 + D) of (D + 18, ldn) allocations full of NaN: pbbi_integrate with v_out and one
    pbbi_hmc_iter_kt (non-compat, masses).  A padded row d >= D loads 0, meets the identity of the images and its store is
    dropped: results within TOL of the restatement, every element outside the blocks keeps its NaN bits, the inputs are
    unchanged -- no canary reaches a result through a product."""
    import torch
    d = F._dev()
    n = CANARY_N
    pot, op, L = _mpot(P, name), _kind(name)[1], _kind(name)[4]
    q0 = _q0(name, n)
    Dt, ldn = q0.shape[0], n + pad
    Md, mass = dense_metric_of(Dt), MASS[:n]
    empty_block = np.full((Dt, n), np.nan)
    mdev, st = d.as_device(mass, 0, np.float64), d.stream_ptr(0)
    p0 = d_draw(Md, mass, KT, SEED, ITER0, CHAIN0, Dt, n)
    u = orc.philox_uniform(SEED, ITER0, CHAIN0, n)
    for mi, method in enumerate(METHODS):
        h = _kind(name)[3][mi]
        q, p = q0.copy(), p0.copy()
        v = d_integrate(op, method, q, p, mass, Md, h, L)
        (qt, qp), (pt, pp), (vt, vp) = F._canary(q0, ldn), F._canary(p0, ldn), F._canary(empty_block, ldn)
        lib.call("pbbi_integrate", pot.handle, orc.METHODS[method], qp, pp, mdev.data_ptr(), vp, n, ldn, h, L, st)
        torch.cuda.synchronize()
        check(method + " integrate q", F._canary_result(qt, Dt, n), q)
        check(method + " integrate p", F._canary_result(pt, Dt, n), p)
        check(method + " integrate v", F._canary_result(vt, Dt, n), v)
        q, p = q0.copy(), p0.copy()
        ratio, rej = d_hmc_iter(op, method, q, p, u, mass, Md, h, L, False, 1.0 / KT)
        _margin(f"canary {name} {method}", ratio, u)
        (qt, qp), (pt, pp) = F._canary(q0, ldn), F._canary(p0, ldn)
        (qot, qop), (pot_, pop) = F._canary(empty_block, ldn), F._canary(empty_block, ldn)
        ud, ro, rj = d.as_device(u, 0, np.float64), d.empty((n,), np.float64, 0), d.empty((n,), np.uint8, 0)
        lib.call("pbbi_hmc_iter_kt", pot.handle, orc.METHODS[method], qp, pp, ud.data_ptr(), mdev.data_ptr(), qop, pop,
                 ro.data_ptr(), rj.data_ptr(), n, ldn, h, L, lib.BETA_ACCEPT, KT, st)
        torch.cuda.synchronize()
        assert np.array_equal(d.to_numpy(rj).astype(bool), rej), method
        check(method + " iter q", F._canary_result(qot, Dt, n), q)
        check(method + " iter p", F._canary_result(pot_, Dt, n), p)
        check(method + " iter ratio", d.to_numpy(ro), ratio)
        assert np.array_equal(F._canary_result(qt, Dt, n), q0) and np.array_equal(F._canary_result(pt, Dt, n), p0)


@pytest.mark.gpu
def test_dense_metric_refusals_and_description(P, lib):
    """6: softmax, ordinal, hierarchical and non-GLM handles and a state wider than 64 rows are refused with
    PBBI_ERR_UNSUPPORTED and the rule, a wrong D and a matrix that is no mass matrix with PBBI_ERR_INVALID, and the handle is
    left as it was; setting the dense metric removes the diagonal one and back, and each get_ answers has = 0 for the other
    kind; describeRun() names the dense metric, and only when there is one; rng="numpy" is a ValueError naming rng="philox";
    adaptMassMatrix(dense=True) is a ValueError where the potential refuses."""
    from scipy.constants import k as kB
    import test_glm_softmax as t_soft
    raw = lib.load()

    def dp(a):
        return a.ctypes.data_as(C.POINTER(C.c_double))

    rs = np.random.RandomState(5)
    X = rs.standard_normal((20, 3))
    refused = [(t_soft.device_pot("A"), "no dense-metric kernel is built for softmax, ordinal and hierarchical"),
               (P.OrdinalGLM(X, rs.randint(0, 3, 20).astype(float), 3), "no dense-metric kernel is built for softmax, ordinal and hierarchical"),
               (F._pot(P, "hier"), "no dense-metric kernel is built for softmax, ordinal and hierarchical"),
               (F._pot(P, "hier_penalty"), "no dense-metric kernel is built for softmax, ordinal and hierarchical"),
               (F._pot(P, "hier_disp_nc"), "no dense-metric kernel is built for softmax, ordinal and hierarchical"),
               (P.StandardGaussian(4), "GLM handles only"),
               (F._pot(P, "logistic128"), "served up to 64")]
    for target, text in refused:
        Dt = target.numDimensions
        eye = np.eye(Dt)
        assert raw.pbbi_potential_set_metric_dense(target.handle, dp(eye), Dt) == lib.ERR_UNSUPPORTED, text
        assert text in lib.last_error(), (text, lib.last_error())
        has = C.c_int(7)
        lib.call("pbbi_potential_get_metric_dense", target.handle, None, 0, C.byref(has))
        assert has.value == 0
        if hasattr(target, "set_metric"):
            with pytest.raises(lib.PbbiError) as e:
                target.set_metric(eye)
            assert e.value.code == lib.ERR_UNSUPPORTED and target.metric is None
    hier = F._pot(P, "hier")
    hh = P.HMC(P.Ensemble(hier.numDimensions, 64), 0.8, 0.1, None, potential=hier, rng="philox", seed=13, verbose=False)
    with pytest.raises(ValueError, match="dense metric"):
        hh.adaptMassMatrix(1 / kB, 1.0, dense=True)
    assert hier.metric is None
    pot = _mpot(P, "logistic")
    D = pot.numDimensions
    Md = dense_metric_of(D)
    for bad_D in (D - 1, D + 1):
        v = np.eye(bad_D)
        assert raw.pbbi_potential_set_metric_dense(pot.handle, dp(v), bad_D) == lib.ERR_INVALID
        assert "state dimension" in lib.last_error()
        with pytest.raises(ValueError):
            pot.set_metric(v)
    for bad, text in ((np.nan, "finite"), (-100.0, "positive definite")):
        v = Md.copy()
        v[D - 1, D - 1] = bad
        assert raw.pbbi_potential_set_metric_dense(pot.handle, dp(v), D) == lib.ERR_INVALID and text in lib.last_error()
    v = Md.copy()
    v[0, 1] += 1e-3
    assert raw.pbbi_potential_set_metric_dense(pot.handle, dp(v), D) == lib.ERR_INVALID and "symmetric" in lib.last_error()
    assert np.array_equal(pot.metric, Md)
    # one metric at a time, and each get_ answers for its own kind only
    has_diag, has_dense = C.c_int(7), C.c_int(7)
    lib.call("pbbi_potential_get_metric_diag", pot.handle, None, 0, C.byref(has_diag))
    lib.call("pbbi_potential_get_metric_dense", pot.handle, None, 0, C.byref(has_dense))
    assert (has_diag.value, has_dense.value) == (0, 1)
    hmc = P.HMC(P.Ensemble(D, 64), 0.8, 0.1, None, potential=pot, rng="philox", seed=13, verbose=False)
    other = P.HMC(P.Ensemble(D, 32), 0.8, 0.1, None, potential=pot, rng="philox", seed=14, verbose=False)
    assert np.array_equal(hmc.massMatrix, Md) and np.array_equal(other.massMatrix, Md)
    text = hmc.describeRun()
    print(text)
    assert "k_glm" in text and "dense metric" in text and "diagonal metric" not in text
    with pytest.raises(ValueError, match='rng="philox"'):
        hmc.getSamples(2, 1 / kB, 1.0, rng="numpy")
    out = np.empty((D, D))
    lib.call("pbbi_potential_get_metric_dense", pot.handle, dp(out), out.size, C.byref(has_dense))
    assert np.array_equal(out, Md)
    assert raw.pbbi_potential_get_metric_dense(pot.handle, dp(out), out.size - 1, C.byref(has_dense)) == lib.ERR_INVALID
    other.setMassMatrix(metric_of(D))
    lib.call("pbbi_potential_get_metric_diag", pot.handle, None, 0, C.byref(has_diag))
    lib.call("pbbi_potential_get_metric_dense", pot.handle, None, 0, C.byref(has_dense))
    assert (has_diag.value, has_dense.value) == (1, 0) and np.array_equal(hmc.massMatrix, metric_of(D))
    text = hmc.describeRun()
    assert "diagonal metric" in text and "dense metric" not in text
    other.setMassMatrix(Md)
    assert np.array_equal(hmc.massMatrix, Md) and "dense metric" in hmc.describeRun()
    other.setMassMatrix(None)
    assert hmc.massMatrix is None and "dense metric" not in hmc.describeRun() and "diagonal metric" not in hmc.describeRun()
    lib.call("pbbi_potential_get_metric_dense", pot.handle, None, 0, C.byref(has_dense))
    assert has_dense.value == 0


@pytest.mark.gpu
def test_dense_metric_is_what_makes_correlated_predictors_sampleable(P, lib):
    """7: two predictors with posterior correlation 0.99, h = 0.5, L = 4, N = 4096.  With M = H the device's reject masks of
    the first iterations are the restatement's and both accept >= 0.9; with the best diagonal metric 1 / diag(H^-1), h
    omega_max = 5 and both accept <= 0.05.  From fit.sample(N), after 10 iterations under M = fit.dense_metric, the mean and
    the covariance over the N chains of the last iteration are mu and H^-1 within 5 standard errors of N independent draws
    (se(mean_d) = sqrt(S_dd / N), se(cov_ij) = sqrt((S_ii S_jj + S_ij^2) / N), S = H^-1 exactly, not the sample's)."""
    from scipy.constants import k as kB
    kw, H, cov, mu, q0 = _gauss()
    pot = _gauss_pot(P)
    assert pot.numDimensions == 3 and pot.metric is None
    pot.set_metric(1.0 / np.diag(cov))
    rej_d = F._device_run(lib, pot, "Leapfrog", np.array(q0), None, G_H, G_L, G_S, lib.DRAW_F64, 1.0, chain0=0)[2]
    pot.set_metric(H)
    rej = F._device_run(lib, pot, "Leapfrog", np.array(q0), None, G_H, G_L, G_S, lib.DRAW_F64, 1.0, chain0=0)[2]
    cpu, cpu_d = _gauss_cpu(True)[0], _gauss_cpu(False)[0]
    print(f"acceptance: M = H {1 - rej.mean():.4f} (restatement {1 - cpu.mean():.4f}), best diagonal {1 - rej_d.mean():.4f} "
          f"(restatement {1 - cpu_d.mean():.4f}); mask mismatches {int((rej != cpu).sum())}")
    assert np.array_equal(rej, cpu)
    assert 1.0 - rej.mean() >= 0.9 and 1.0 - cpu.mean() >= 0.9
    assert 1.0 - rej_d.mean() <= 0.05 and 1.0 - cpu_d.mean() <= 0.05
    fit = pot.laplace()
    check("laplace mode", fit.mode, mu, tol=1e-8)
    check("laplace Hessian", fit.dense_metric, H, tol=1e-8)
    hmc = P.HMC(P.Ensemble(3, G_N), G_H * G_L, G_H, None, potential=pot, rng="philox", seed=SEED, verbose=False, compat=False,
                draw_f64=True)
    hmc.setMassMatrix(fit.dense_metric)
    s, _ = hmc.getSamples(10, 1 / kB, 1.0, start=fit.sample(G_N))          # (D, N, S)
    last = np.ascontiguousarray(np.asarray(s)[:, :, -1])
    assert last.shape == (3, G_N) and hmc.acceptRate >= 0.9
    got_mean, got_cov = last.mean(axis=1), np.cov(last)
    se_mean = np.sqrt(np.diag(cov) / G_N)
    se_cov = np.sqrt((np.outer(np.diag(cov), np.diag(cov)) + cov ** 2) / G_N)
    print("mean error / se", (got_mean - mu) / se_mean, "covariance error / se", (got_cov - cov) / se_cov)
    assert np.all(np.abs(got_mean - mu) <= 5.0 * se_mean)
    assert np.all(np.abs(got_cov - cov) <= 5.0 * se_cov)


@pytest.mark.gpu
def test_adapt_mass_matrix_dense_recovers_the_precision(P, lib):
    """8: from a cold start (the unit metric, qStd = 1) adaptMassMatrix(dense=True, windows=(25, 50, 100)) returns M with the
    eigenvalues of H^-1 M inside [0.5, 2] -- the factor-2 band of the diagonal test, Stan's shrinkage included -- leaves
    stepSize / numSteps set, and the ensemble then accepts >= 0.6."""
    from scipy.constants import k as kB
    kw, H, cov, mu, _ = _gauss()
    pot = _gauss_pot(P)
    hmc = P.HMC(P.Ensemble(3, G_N), G_T, 0.01, None, potential=pot, rng="philox", seed=SEED, verbose=False, compat=False,
                draw_f64=True)
    M = hmc.adaptMassMatrix(1 / kB, 1.0, windows=(25, 50, 100), dense=True)
    ev = np.sort(np.linalg.eigvals(cov @ M).real)
    print("adapted metric", M, "eigenvalues of H^-1 M", ev, "step", hmc.stepSize, hmc.integrator.numSteps)
    assert M.shape == (3, 3) and np.array_equal(M, pot.metric) and np.array_equal(M, hmc.massMatrix)
    assert ev[0] >= 0.5 and ev[-1] <= 2.0, ev
    assert hmc.integrator.numSteps == max(1, int(hmc.simulTime / hmc.stepSize)) and hmc.integrator.stepSize == hmc.stepSize
    hmc.getSamples(20, 1 / kB, 1.0)
    print("accept", hmc.acceptRate)
    assert hmc.acceptRate >= 0.6
