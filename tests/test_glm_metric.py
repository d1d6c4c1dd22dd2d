"""The diagonal metric of the GLM kernels (METRIC = true of k_glm and k_glm_softmax, pbbi_potential_set_metric_diag): row d
of chain n has mass m_n m_d in the draw, the velocity, the kick and the kinetic energy.

The reference is a NumPy restatement, below, of one HMC iteration and of integrate() with those masses: the oracle's loop
(oracle/pbbi_oracle.c leapfrog_chain, stormer_verlet_chain, oracle_hmc_iter_dyn, oracle_hmc_run_philox -- the reference's
src/HMC.py:154-179 and src/integrator.py) with m replaced by m_n m_d, U and grad U from oracle.potential, the draws from
oracle.philox_normal / philox_uniform.  test_restatement_is_the_oracle_at_unit_metric holds it to the oracle first.

Handles, starts, step sizes and conventions are test_glm_frame.py's: N = 150 (nine full wave tiles, one of 6 chains, two ghost
waves in the last workgroup), seed 4, iteration 1, chain0 = 2^32 - 70, MASS = 1 + 0.5 (n % 3), tolerance test_glm.TOL = 1e-10
through its check, masks equal with no chain excluded.  The metric of a handle is geometric over [1, 30] across the state,
30^((d + 0.5) / Dt): a distinct value per row, none a power of two, so a wrong row mapping cannot cancel, and frequencies only
fall, so the files' own step sizes stay stable."""
import ctypes as C
import functools

import numpy as np
import pytest

import test_glm_dispersion as t_disp
import test_glm_frame as F
from oracle import oracle as orc
from test_glm import check     # rel <= TOL = 1e-10, both of that file

N, SEED, ITER0, CHAIN0, MASS, KT, S_RUN, METHODS = F.N, F.SEED, F.ITER0, F.CHAIN0, F.MASS, F.KT, F.S_RUN, F.METHODS
NAMES = ["logistic", "logistic17", "logistic50", "logistic128", "poisson_full", "gaussian_sampled", "negbinomial_held",
         "hier", "hier_nc", "hier_penalty", "hier_disp_nc", "softmax"]
FRAMES = ["logistic", "softmax"]      # one handle of each twin for tests 2 and 3
# (method, PBBI_BETA_ACCEPT, PBBI_COMPAT_P_FROM_OLDQ): all at kT = 2.5, with MASS, PBBI_DRAW_F64
RUN_ROWS = [(me, b, c) for me in METHODS for b in (False, True) for c in (False, True)]
RUN_CASES = [("run", name) + row for name in NAMES for row in RUN_ROWS]
ITER_CASES = [("iter", name, me) for name in FRAMES for me in METHODS]
# case -> step size where the handle's own (test_glm_frame.KINDS) leaves an accept test within 1e-7 of its uniform
# (test_metric_cases_are_decisive picks these)
STEP = {}


def metric_of(Dt):
    return 30.0 ** ((np.arange(Dt) + 0.5) / Dt)


def _h(case):
    return STEP.get(case, F.KINDS[case[1]]["h"][METHODS.index(case[2])])


# ---- the restatement ------------------------------------------------------------------------------------------------
def _mass2(q, mass, md):
    """m_n m_d as a (D, N) array."""
    D, n = q.shape
    m = np.ones(n) if mass is None else np.asarray(mass, float)
    d = np.ones(D) if md is None else np.asarray(md, float)
    return d[:, None] * m[None, :]


def _accel(op, q, M):
    return -orc.potential(op, np.ascontiguousarray(q), want_grad=True)[1] / M       # getAccel: -gradient / mass


def r_integrate(op, method, q, p, mass, md, h, L):
    """integrate() in place on q, p (D, N); returns v (Integrator.v)."""
    M = _mass2(q, mass, md)
    h2 = h * h
    v = p / M
    if method == "Leapfrog":
        a = _accel(op, q, M)
        for _ in range(L):
            q += (v * h + (0.5 * a) * h2)
            an = _accel(op, q, M)
            v += (0.5 * (a + an)) * h
            a = an
    else:
        qpast = q.copy()
        a = _accel(op, q, M)
        q[:] = (q + v * h) + (0.5 * a) * h2
        for _ in range(L):
            a = _accel(op, q, M)
            cur = q.copy()
            q[:] = (2 * cur - qpast) + a * h2
            qpast = cur
        v = (q - qpast) / h
    p[:] = v * M
    return v


def r_hamiltonian(op, q, p, mass, md):
    """0.5 sum_d p_d^2 / (m_n m_d) + U(q); the sum runs over d in order, the per-chain mass divides it last (the oracle's
    0.5 * pp / m when m_d = 1)."""
    D, n = q.shape
    m = np.ones(n) if mass is None else np.asarray(mass, float)
    d = np.ones(D) if md is None else np.asarray(md, float)
    pp = np.zeros(n)
    for k in range(D):
        pp += p[k] * p[k] / d[k]
    return 0.5 * pp / m + orc.potential(op, np.ascontiguousarray(q))


def r_hmc_iter(op, method, q, p, u, mass, md, h, L, compat, beta=1.0):
    """One getSamples iteration in place on q (state) and p (drawn momentum); returns (ratio, reject mask)."""
    oq, opp = q.copy(), p.copy()
    r_integrate(op, method, q, p, mass, md, h, L)
    oldH = r_hamiltonian(op, oq, opp, mass, md)
    newH = r_hamiltonian(op, q, -p, mass, md)
    with np.errstate(over="ignore"):
        ratio = np.exp((oldH - newH) * beta)
    rej = u > np.minimum(1.0, ratio)                     # False where the ratio is NaN
    q[:, rej] = oq[:, rej]
    p[:, rej] = (oq if compat else opp)[:, rej]
    return ratio, rej


def r_run(op, method, q, mass, md, h, L, S, seed, iter0, chain0, kT, beta_accept, compat):
    """S iterations with the Philox contract (double-precision draw), q (D, N) the state, updated in place: samples and
    momenta (S, D, N), reject (S, N), ratio (S, N), and the uniforms."""
    D, n = q.shape
    pstd = np.sqrt(_mass2(q, mass, md) * kT)
    out = [np.empty((S, D, n)), np.empty((S, D, n)), np.empty((S, n), bool), np.empty((S, n)), np.empty((S, n))]
    for i in range(S):
        p = orc.philox_normal(seed, orc.STREAM_MOMENTUM | orc.STREAM_DRAW_F64, iter0 + i, chain0, D, n) * pstd
        u = orc.philox_uniform(seed, iter0 + i, chain0, n)
        ratio, rej = r_hmc_iter(op, method, q, p, u, mass, md, h, L, compat, 1.0 / kT if beta_accept else 1.0)
        out[0][i], out[1][i], out[2][i], out[3][i], out[4][i] = q, p, rej, ratio, u
    return out


@functools.lru_cache(maxsize=None)
def _ref(case):
    """The restatement's result of a case under the handle's metric, computed once and left unchanged."""
    name = case[1]
    op, L, h = F._kind(name)[1], F.KINDS[name]["L"], _h(case)
    q = F._q0(name)
    md = metric_of(q.shape[0])
    if case[0] == "run":
        _, _, method, beta, compat = case
        s, p, rej, ratio, u = r_run(op, method, q, MASS, md, h, L, S_RUN, SEED, ITER0, CHAIN0, KT, beta, compat)
        return F._frozen(samples=s, momenta=p, rej=rej, ratio=ratio, u=u, q=q)
    _, _, method = case
    p_in = np.ascontiguousarray(orc.philox_normal(SEED, orc.STREAM_MOMENTUM | orc.STREAM_DRAW_F64, ITER0, CHAIN0,
                                                  q.shape[0], N) * np.sqrt(_mass2(q, MASS, md) * KT))
    u = orc.philox_uniform(SEED, ITER0, CHAIN0, N)
    p = p_in.copy()
    ratio, rej = r_hmc_iter(op, method, q, p, u, MASS, md, h, L, False, 1.0 / KT)
    return F._frozen(q=q, p=p, p_in=p_in, rej=rej, ratio=ratio, u=u)


def _margin(tag, ratio, u):
    assert np.all(np.isfinite(ratio)) and np.all(np.isfinite(u)), tag
    margin = float(np.min(np.abs(ratio - u) / np.maximum(1.0, ratio)))
    print(f"{tag}: reject fraction {float(np.mean(u > np.minimum(1.0, ratio))):.3f}, closest accept test {margin:.2e}")
    assert margin >= 1e-7, (tag, margin)


# ---- CPU --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["logistic", "hier_nc", "softmax"])
def test_restatement_is_the_oracle_at_unit_metric(name):
    """With m_d = 1 and per-chain masses the restatement agrees with oracle.hmc_iter and oracle.integrate to 1e-12 on q, p
    (and v) and ratio, both methods, compat and non-compat, beta = 1 and 1 / 2.5; masks equal.  With m_d = None likewise."""
    op, L = F._kind(name)[1], F.KINDS[name]["L"]
    q0 = F._q0(name, 40)
    Dt = q0.shape[0]
    mass = MASS[:40]
    p0 = np.ascontiguousarray(orc.philox_normal(SEED, orc.STREAM_MOMENTUM | orc.STREAM_DRAW_F64, ITER0, CHAIN0, Dt, 40,
                                                np.sqrt(mass * KT)))
    u = orc.philox_uniform(SEED, ITER0, CHAIN0, 40)
    for mi, method in enumerate(METHODS):
        h = F.KINDS[name]["h"][mi]
        for md in (np.ones(Dt), None):
            q, p = q0.copy(), p0.copy()
            v = orc.integrate(op, method, q, p, mass, h, L)
            rq, rp = q0.copy(), p0.copy()
            rv = r_integrate(op, method, rq, rp, mass, md, h, L)
            for tag, a, b in (("q", rq, q), ("p", rp, p), ("v", rv, v)):
                check(f"{name} {method} integrate {tag}", a, b, tol=1e-12)
            for compat in (0, orc.COMPAT_P_FROM_OLDQ):
                for beta in (1.0, 1.0 / KT):
                    q, p = q0.copy(), p0.copy()
                    ratio, rej = orc.hmc_iter(op, method, q, p, u, mass, h, L, compat=compat, beta=beta)
                    rq, rp = q0.copy(), p0.copy()
                    rratio, rrej = r_hmc_iter(op, method, rq, rp, u, mass, md, h, L, bool(compat), beta)
                    assert np.array_equal(rrej, rej) and 0 < rej.sum() < 40, (name, method, compat, beta, rej.sum())
                    for tag, a, b in (("q", rq, q), ("p", rp, p), ("ratio", rratio, ratio)):
                        check(f"{name} {method} compat={compat} beta={beta:.1f} iter {tag}", a, b, tol=1e-12)


def test_restatement_run_is_the_oracle_at_unit_metric():
    """... and its run is oracle.hmc_run_philox (the draw, the uniforms, the parked momentum of a rejected chain)."""
    name = "logistic"
    op, L, h = F._kind(name)[1], F.KINDS[name]["L"], F.KINDS[name]["h"][0]
    for beta, compat in ((False, False), (True, True)):
        q, rq = F._q0(name, 40), F._q0(name, 40)
        flags = orc.DRAW_F64 | (orc.BETA_ACCEPT if beta else 0) | (orc.COMPAT_P_FROM_OLDQ if compat else 0)
        s, p, rej, ratio = orc.hmc_run_philox(op, "Leapfrog", q, MASS[:40], h, L, S_RUN, SEED, ITER0, CHAIN0, KT, compat=flags)
        rs, rp, rrej, rratio, _ = r_run(op, "Leapfrog", rq, MASS[:40], np.ones(q.shape[0]), h, L, S_RUN, SEED, ITER0, CHAIN0, KT,
                                        beta, compat)
        assert np.array_equal(rrej, rej) and rej.any()
        for tag, a, b in (("samples", rs, s), ("momenta", rp, p), ("ratio", rratio, ratio), ("state", rq, q)):
            check(f"run beta={beta} compat={compat} {tag}", a, b, tol=1e-12)


def test_metric_cases_are_decisive():
    """The restatement alone, for every case of the GPU tests below: every value finite and no accept test within 1e-7
    (relative to max(1, ratio)) of its uniform, so that "masks are equal" is a fair demand on the device at 1e-10.  Both
    outcomes occur on every handle."""
    for name in NAMES:
        n_rej = n_all = 0
        for case in (c for c in RUN_CASES + ITER_CASES if c[1] == name):
            o = _ref(case)
            assert all(np.all(np.isfinite(v)) for k, v in o.items() if k in ("samples", "momenta", "q", "p")), case
            _margin(str(case), o["ratio"], o["u"])
            n_rej += int(o["rej"].sum())
            n_all += o["rej"].size
        assert 0 < n_rej < n_all, (name, n_rej, n_all)
    md = metric_of(7)
    assert len(set(md)) == 7 and md[0] > 1.0 and md[-1] < 30.0 and not np.any(np.log2(md) == np.round(np.log2(md)))
    assert np.allclose(md[1:] / md[:-1], 30.0 ** (1.0 / 7), rtol=1e-14)


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


_MPOTS = {}


def _mpot(P, name):
    """A handle of its own per kind (test_glm_frame's are left without a metric), carrying metric_of(Dt)."""
    if name not in _MPOTS:
        if name == "softmax":         # (test_glm_softmax.device_pot caches ONE handle per case: make a private one its way)
            import test_glm_softmax as t_soft
            M, D, K = t_soft.CASES["A"][:3]
            X, y, _, _ = t_soft.problem(M, D, K)
            _MPOTS[name] = P.SoftmaxGLM(X, y, classes=K, prior_precision=t_soft.lam_of(D))
        else:
            _MPOTS[name] = F._kind(name)[0](P)
    pot = _MPOTS[name]
    pot.set_metric(metric_of(pot.numDimensions))
    return pot


def _flags(lib, beta, compat):
    return lib.DRAW_F64 | (lib.BETA_ACCEPT if beta else 0) | (lib.COMPAT_P_FROM_OLDQ if compat else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_metric_run_vs_restatement(P, lib, name):
    """pbbi_hmc_run on a handle with a metric, S = 3, kT = 2.5, MASS, PBBI_DRAW_F64, leading stride N + 5: {Leapfrog,
    Stormer-Verlet} x {0, PBBI_BETA_ACCEPT} x {non-compat, PBBI_COMPAT_P_FROM_OLDQ} against the restatement -- samples,
    momenta (the parked draw z sqrt(m_n m_d kT) of a rejected non-compat chain among them), ratios, the final state within
    TOL; masks equal; padding columns untouched.  The handle reports its metric back."""
    pot, L = _mpot(P, name), F.KINDS[name]["L"]
    assert np.array_equal(pot.metric, metric_of(pot.numDimensions))
    for case in (c for c in RUN_CASES if c[1] == name):
        _, _, method, beta, compat = case
        o = _ref(case)
        _margin(str(case), o["ratio"], o["u"])
        gs, gm, grej, gratio, gq, gpad = F._device_run(lib, pot, method, F._q0(name), MASS, _h(case), L, S_RUN,
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
@pytest.mark.parametrize("name", FRAMES)
def test_metric_uploaded_draws_vs_restatement(P, lib, name):
    """pbbi_hmc_iter_kt with uploaded momenta (z sqrt(m_n m_d kT)) and uniforms, PBBI_BETA_ACCEPT at kT = 2.5, non-compat,
    both methods: masks equal, q, p, ratio within TOL, a rejected chain's p_out is its p_in bit for bit; without p_out,
    ratio_out and reject_out the same q_out bit for bit."""
    pot, L = _mpot(P, name), F.KINDS[name]["L"]
    for case in (c for c in ITER_CASES if c[1] == name):
        method = case[2]
        o = _ref(case)
        _margin(str(case), o["ratio"], o["u"])
        rj = o["rej"]
        gq, gp, gratio, grej = F._device_iter(lib, pot, method, F._q0(name), o["p_in"], o["u"], MASS, _h(case), L,
                                              lib.BETA_ACCEPT, KT)
        tag = f"{name} {method}"
        assert np.array_equal(grej, rj) and 0 < rj.sum() < N, tag
        check(tag + " q", gq, o["q"])
        check(tag + " p", gp, o["p"])
        check(tag + " ratio", gratio, o["ratio"])
        assert np.array_equal(gp[:, rj], o["p_in"][:, rj]) and np.array_equal(gq[:, rj], F._q0(name)[:, rj]), tag
        q_only = F._device_iter(lib, pot, method, F._q0(name), o["p_in"], o["u"], MASS, _h(case), L, lib.BETA_ACCEPT, KT,
                                outputs=False)[0]
        assert np.array_equal(q_only, gq), tag


@pytest.mark.gpu
@pytest.mark.parametrize("name", FRAMES)
def test_metric_integrate_and_energies_vs_restatement(P, lib, name):
    """pbbi_leapfrog, pbbi_stormer_verlet (q, p in place), pbbi_integrate's v_out (Integrator.v = p / (m_n m_d)), pbbi_energy
    (H and exp(-H)) and pbbi_weights_ratio against the restatement under the metric, with MASS."""
    import torch
    d = F._dev()
    pot, op, L = _mpot(P, name), F._kind(name)[1], F.KINDS[name]["L"]
    q0 = F._q0(name)
    Dt = q0.shape[0]
    md = metric_of(Dt)
    p0 = np.array(_ref(("iter", name, "Leapfrog"))["p_in"])
    mdev, st = d.as_device(MASS, 0, np.float64), d.stream_ptr(0)
    ends = {}
    for mi, method in enumerate(METHODS):
        h = F.KINDS[name]["h"][mi]
        q, p = q0.copy(), p0.copy()
        v = r_integrate(op, method, q, p, MASS, md, h, L)
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
    H0 = r_hamiltonian(op, q0, p0, MASS, md)
    qd, pd = d.as_device(q0, 0, np.float64), d.as_device(p0, 0, np.float64)
    Hd, wd = d.empty((N,), np.float64, 0), d.empty((N,), np.float64, 0)
    lib.call("pbbi_energy", pot.handle, qd.data_ptr(), pd.data_ptr(), mdev.data_ptr(), N, N, Hd.data_ptr(), wd.data_ptr(), st)
    torch.cuda.synchronize()
    check(f"{name} H", d.to_numpy(Hd), H0)
    assert np.max(np.abs(d.to_numpy(wd) / np.exp(-H0) - 1.0)) <= 1e-10 * max(1.0, np.max(np.abs(H0)))
    q1, p1 = ends["Leapfrog"]
    H1 = r_hamiltonian(op, q1, p1, MASS, md)
    nq, npd = d.as_device(q1, 0, np.float64), d.as_device(p1, 0, np.float64)
    rd = d.empty((N,), np.float64, 0)
    lib.call("pbbi_weights_ratio", pot.handle, nq.data_ptr(), npd.data_ptr(), qd.data_ptr(), pd.data_ptr(), mdev.data_ptr(),
             N, N, rd.data_ptr(), st)
    torch.cuda.synchronize()
    check(f"{name} weights ratio", d.to_numpy(rd), np.exp(H0 - H1))
    # pbbi_potential_eval does not see the metric
    U, g = orc.potential(op, q0, want_grad=True)
    Ud, gd = d.empty((N,), np.float64, 0), d.empty((Dt, N), np.float64, 0)
    lib.call("pbbi_potential_eval", pot.handle, qd.data_ptr(), N, N, Ud.data_ptr(), gd.data_ptr(), st)
    torch.cuda.synchronize()
    check(f"{name} U", d.to_numpy(Ud), U)
    check(f"{name} gradient", d.to_numpy(gd), g)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_ones_metric_is_the_handle_without_one_bit_for_bit(P, lib, name):
    """Device against device: a metric of all ones multiplies by exactly 1.0 and reproduces the no-metric pbbi_hmc_run bit
    for bit (samples, momenta, masks, ratios, the state), both methods, compat and not; after set_metric(None) the handle
    equals a fresh handle bit for bit again, and reports no metric."""
    fresh, L = F._pot(P, name), F.KINDS[name]["L"]
    assert fresh.metric is None
    pot = _mpot(P, name)
    rows = [("Leapfrog", True, False), ("Stormer-Verlet", False, True)]
    want = [F._device_run(lib, fresh, me, F._q0(name), MASS, F.KINDS[name]["h"][METHODS.index(me)], L, S_RUN,
                          _flags(lib, b, c), KT, pad=5) for me, b, c in rows]
    assert any(w[2].any() for w in want) and not all(w[2].all() for w in want)
    with_metric = F._device_run(lib, pot, "Leapfrog", F._q0(name), MASS, F.KINDS[name]["h"][0], L, S_RUN, _flags(lib, True, False),
                                KT, pad=5)
    assert not np.array_equal(with_metric[0], want[0][0])                 # the metric in place does change the run
    for setting in ("ones", None):
        pot.set_metric(np.ones(pot.numDimensions) if setting == "ones" else None)
        assert (pot.metric is None) if setting is None else np.array_equal(pot.metric, np.ones(pot.numDimensions))
        for (me, b, c), w in zip(rows, want):
            got = F._device_run(lib, pot, me, F._q0(name), MASS, F.KINDS[name]["h"][METHODS.index(me)], L, S_RUN,
                                _flags(lib, b, c), KT, pad=5)
            for tag, a, r in zip(("samples", "momenta", "reject", "ratio", "state", "padding"), got, w):
                assert np.array_equal(a, r), (name, setting, me, tag)


CANARY_N = 37


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("name", ["logistic", "logistic17", "logistic50", "softmax"])
def test_metric_state_inside_a_canary_allocation(P, lib, name, pad):
    """N = 37 chains (two full tiles and a ragged one of 5, a ghost wave) under the metric, the state, momentum and output
    arrays rows [1, 1 + D) of (D + 18, ldn) allocations full of NaN: pbbi_integrate with v_out and one pbbi_hmc_iter_kt
    (non-compat, masses).  A padded row d >= D loads 0 and its store is dropped: results within TOL of the restatement,
    every element outside the blocks keeps its NaN bits, the inputs are unchanged."""
    import torch
    d = F._dev()
    n = CANARY_N
    pot, op, L = _mpot(P, name), F._kind(name)[1], F.KINDS[name]["L"]
    q0 = F._q0(name, n)
    Dt, ldn = q0.shape[0], n + pad
    md, mass = metric_of(Dt), MASS[:n]
    empty_block = np.full((Dt, n), np.nan)
    mdev, st = d.as_device(mass, 0, np.float64), d.stream_ptr(0)
    p0 = np.ascontiguousarray(orc.philox_normal(SEED, orc.STREAM_MOMENTUM | orc.STREAM_DRAW_F64, ITER0, CHAIN0, Dt, n)
                              * np.sqrt(_mass2(q0, mass, md) * KT))
    u = orc.philox_uniform(SEED, ITER0, CHAIN0, n)
    for mi, method in enumerate(METHODS):
        h = F.KINDS[name]["h"][mi]
        q, p = q0.copy(), p0.copy()
        v = r_integrate(op, method, q, p, mass, md, h, L)
        (qt, qp), (pt, pp), (vt, vp) = F._canary(q0, ldn), F._canary(p0, ldn), F._canary(empty_block, ldn)
        lib.call("pbbi_integrate", pot.handle, orc.METHODS[method], qp, pp, mdev.data_ptr(), vp, n, ldn, h, L, st)
        torch.cuda.synchronize()
        check(method + " integrate q", F._canary_result(qt, Dt, n), q)
        check(method + " integrate p", F._canary_result(pt, Dt, n), p)
        check(method + " integrate v", F._canary_result(vt, Dt, n), v)
        q, p = q0.copy(), p0.copy()
        ratio, rej = r_hmc_iter(op, method, q, p, u, mass, md, h, L, False, 1.0 / KT)
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
def test_metric_refusals_and_description(P, lib):
    """A handle that is no GLM handle is refused (PBBI_ERR_UNSUPPORTED; HMC.setMassMatrix: ValueError); a wrong D and an
    entry that is no mass are PBBI_ERR_INVALID and leave the metric as it was; per-chain lengths and GIST stay refused
    with a metric set, with the messages they have without one; describeRun() names the metric, and only when there is
    one; two samplers on one potential share it."""
    from scipy.constants import k as kB
    pot = _mpot(P, "logistic")
    D = pot.numDimensions
    md = metric_of(D)
    gauss = P.StandardGaussian(D)
    one = np.ones(D)
    assert lib.load().pbbi_potential_set_metric_diag(gauss.handle, one.ctypes.data_as(C.POINTER(C.c_double)), D) == lib.ERR_UNSUPPORTED
    assert "GLM handles only" in lib.last_error()
    has = C.c_int(7)
    lib.call("pbbi_potential_get_metric_diag", gauss.handle, None, 0, C.byref(has))
    assert has.value == 0
    hg = P.HMC(P.Ensemble(D, 64), 0.8, 0.1, None, potential=gauss, rng="philox", seed=13, verbose=False)
    with pytest.raises(ValueError):
        hg.setMassMatrix(one)
    with pytest.raises(ValueError):
        hg.adaptMassMatrix(1 / kB, 1.0)
    for bad_D in (D - 1, D + 1):
        v = np.ones(bad_D)
        assert lib.load().pbbi_potential_set_metric_diag(pot.handle, v.ctypes.data_as(C.POINTER(C.c_double)), bad_D) == lib.ERR_INVALID
        assert "state dimension" in lib.last_error()
        with pytest.raises(ValueError):
            pot.set_metric(v)
    for bad in (0.0, -2.0, np.nan, np.inf):
        v = md.copy()
        v[D - 1] = bad
        assert lib.load().pbbi_potential_set_metric_diag(pot.handle, v.ctypes.data_as(C.POINTER(C.c_double)), D) == lib.ERR_INVALID
        assert "finite and > 0" in lib.last_error()
    assert np.array_equal(pot.metric, md)
    hmc = P.HMC(P.Ensemble(D, 64), 0.8, 0.1, None, potential=pot, rng="philox", seed=13, verbose=False)
    other = P.HMC(P.Ensemble(D, 32), 0.8, 0.1, None, potential=pot, rng="philox", seed=14, verbose=False)
    assert np.array_equal(hmc.massMatrix, md) and np.array_equal(other.massMatrix, md)
    text = hmc.describeRun()
    print(text)
    assert "k_glm" in text and "diagonal metric" in text and "iterations per launch: up to 1" in text
    plain = F._pot(P, "logistic")
    errs = []
    for target in (pot, plain):
        h = P.HMC(P.Ensemble(D, 64), 0.8, 0.1, None, potential=target, rng="philox", seed=13, verbose=False)
        with pytest.raises(lib.PbbiError) as e:
            h.getSamplesGIST(2, 1 / kB, 1.0)
        errs.append((e.value.code, str(e.value)))
        import torch
        d = F._dev()
        q = d.as_device(F._q0("logistic", 64), 0, np.float64)
        steps = torch.full((64,), 3, dtype=torch.int32, device="cuda:0")
        out = d.empty((1, D, 64), np.float64, 0)
        rc = lib.load().pbbi_hmc_run_dyn(target.handle, 0, q.data_ptr(), None, steps.data_ptr(), out.data_ptr(), None, None, None,
                                         64, 64, 0.1, 8, 1, lib.PER_CHAIN_STEPS, SEED, ITER0, 0, 1.0, d.stream_ptr(0))
        errs.append((rc, lib.last_error()))
    assert errs[0] == errs[2] and errs[1] == errs[3]
    assert errs[0][0] == lib.ERR_UNSUPPORTED and errs[1][0] == lib.ERR_UNSUPPORTED
    other.setMassMatrix(None)
    assert hmc.massMatrix is None and "diagonal metric" not in hmc.describeRun()
    # the one METRIC kernel that did not ship (softmax at 64 rows per class: it reserves scratch) is refused with the reason
    import test_glm_softmax as t_soft
    wide = t_soft.device_pot("D")                       # D = 40, K = 2: Dc = 64
    with pytest.raises(lib.PbbiError) as e:
        wide.set_metric(np.ones(wide.numDimensions))
    assert e.value.code == lib.ERR_UNSUPPORTED and "not shipped" in str(e.value) and wide.metric is None


# ---- what the feature is for ------------------------------------------------------------------------------------------
# Gaussian family, sigma = 1 held, M = 64, D = 3, orthogonal columns of norms 1 : 10 : 100, prior precision 0.01: the posterior is
# N(mean_d, s_d^2) with s_d = 1 / sqrt(|x_d|^2 + 0.01) = 0.995, 0.09999, 0.0099999995 (s_min <= 0.01, s_max about 1).
G_N, G_H, G_L, G_S = 4096, 0.5, 8, 4
G_LAM = 0.01
# adaptMassMatrix's trajectory length (simulTime).  On a Gaussian whose metric is right every row turns by the angle T per
# iteration: near pi / 2 a draw forgets its start at once, near pi it is its own mirror image (q' = -q) and |q_d| is forgotten
# only through the Metropolis step -- rows that start 10 and 100 standard deviations out (qStd = 1) then bias the pooled
# variances for hundreds of iterations.  1.5 is the first (at simulTime 4.0 the adapted step gave three steps, 3.3 rad, and the
# middle row's variance came out 1.149 times the exact one).
G_T = 1.5


@functools.lru_cache(maxsize=None)
def _gauss():
    rs = np.random.RandomState(29)
    Q, _ = np.linalg.qr(rs.standard_normal((64, 3)))
    X = np.ascontiguousarray(Q * np.array([1.0, 10.0, 100.0]))
    w = np.array([0.8, -0.3, 0.05])
    y = X @ w + rs.standard_normal(64)
    kw = dict(X=X, y=y, family="gaussian", weights=None, offset=None, prior_precision=G_LAM, prior_mean=None)
    prec = np.sum(X * X, axis=0) + G_LAM
    assert np.max(np.abs(X.T @ X - np.diag(np.sum(X * X, axis=0)))) < 1e-10
    s = 1.0 / np.sqrt(prec)
    mean = (X.T @ y) / prec
    assert s.min() <= 0.01 and 0.9 < s.max() < 1.0
    q0 = np.ascontiguousarray(mean[:, None] + s[:, None] * rs.standard_normal((3, G_N)))     # a stationary start
    q0.setflags(write=False)
    return kw, mean, s, q0


@functools.lru_cache(maxsize=None)
def _gauss_cpu_rate():
    """The restatement at the GPU test's sizes with the exact metric: the acceptance rate over G_S iterations of N chains."""
    kw, mean, s, q0 = _gauss()
    op = t_disp.oracle_pot(kw, False, 0.0)
    q = q0.copy()
    _, _, rej, ratio, u = r_run(op, "Leapfrog", q, None, 1.0 / s ** 2, G_H, G_L, G_S, SEED, ITER0, 0, 1.0, False, False)
    _margin("gaussian exact metric", ratio, u)
    return 1.0 - float(rej.mean())


def _gauss_device_rate(lib, pot, q0):
    rej = F._device_run(lib, pot, "Leapfrog", np.array(q0), None, G_H, G_L, G_S, lib.DRAW_F64, 1.0, chain0=0)[2]
    return 1.0 - float(rej.mean())


def test_gaussian_scheme_recovers_the_metric_in_numpy():
    """The windows of test 7c are chosen here, without a device: Stan's shrinkage alone, applied to the EXACT variances with
    the last window's n = 100 draws, is within a factor 2 of 1 / s_d^2 in every row (the stiff row: 1e-4 -> 1.43e-4), and
    stays so when the pooled variance is off by 10 % either way -- five times the 2 % sampling error of 4096 chains.  A last
    window of 25 draws would not do (2.5e-4), which is why the windows end with 100."""
    from physicsbasedbayesianinference_amd.HMC import regularized_variance
    _, _, s, _ = _gauss()
    for off in (0.9, 1.0, 1.1):
        m = 1.0 / regularized_variance(off * s ** 2, 100)
        assert np.all(m * s ** 2 < 2.0) and np.all(m * s ** 2 > 0.5), (off, m * s ** 2)
    assert (1.0 / regularized_variance(s ** 2, 25) * s ** 2).min() < 0.5


@pytest.mark.gpu
def test_metric_is_what_makes_the_scaled_gaussian_sampleable(P, lib):
    """7a: with the exact metric m_d = 1 / s_d^2 every row has h omega = 0.5 at h = 0.5 and the acceptance rate clears the
    restatement's own rate at the same sizes minus 3 binomial standard errors.  7b: without a metric the stiff row has
    h omega = 50, leapfrog grows by more than 10^3 per step, and the acceptance rate is below 0.01 -- on the code
    before the metric too, which is the point."""
    kw, mean, s, q0 = _gauss()
    pot = t_disp.make(P, kw, False, 0.0)
    assert pot.numDimensions == 3 and pot.metric is None
    bare = _gauss_device_rate(lib, pot, q0)
    pot.set_metric(1.0 / s ** 2)
    exact = _gauss_device_rate(lib, pot, q0)
    cpu = _gauss_cpu_rate()
    floor = cpu - 3.0 * np.sqrt(cpu * (1.0 - cpu) / (G_S * G_N))
    print(f"acceptance: exact metric {exact:.4f} (restatement {cpu:.4f}, floor {floor:.4f}), no metric {bare:.5f}")
    assert exact >= floor      # measured on MI355X: 0.9693 (the restatement's own rate 0.9693, floor 0.9653)
    assert bare < 0.01         # measured: 0.00000 -- not one of 16 384 proposals


@pytest.mark.gpu
def test_adapt_mass_matrix_recovers_the_scales_and_the_moments(P, lib):
    """7c: adaptMassMatrix from the unit metric (windows 25, 100) returns m_d within a factor 2 of 1 / s_d^2 in every row --
    the true values span four decades -- and leaves stepSize / numSteps set.  7d: a sampleStats run after it gives
    posterior means within 5 standard errors (from the run's own ESS) of the closed form and variances within 15 %."""
    from scipy.constants import k as kB
    kw, mean, s, _ = _gauss()
    pot = t_disp.make(P, kw, False, 0.0)
    hmc = P.HMC(P.Ensemble(3, G_N), G_T, 0.01, None, potential=pot, rng="philox", seed=SEED, verbose=False, compat=False,
                draw_f64=True)
    m = hmc.adaptMassMatrix(1 / kB, 1.0, windows=(25, 100))
    print("adapted metric", m, "exact", 1.0 / s ** 2, "ratio", m * s ** 2, "step", hmc.stepSize, hmc.integrator.numSteps)
    assert np.array_equal(m, pot.metric) and np.array_equal(m, hmc.massMatrix)
    assert np.all(m * s ** 2 < 2.0) and np.all(m * s ** 2 > 0.5), m * s ** 2      # measured: 1.048, 1.043, 0.701
    assert hmc.integrator.numSteps == max(1, int(hmc.simulTime / hmc.stepSize)) and hmc.integrator.stepSize == hmc.stepSize
    stats = hmc.sampleStats(60, 20, 1 / kB, 1.0, burn_in=40, max_lag=16)
    got_mean, got_var = stats.moments()
    ess = stats.ess()
    se = s / np.sqrt(ess)
    print("accept", hmc.acceptRate, "ess", ess, "mean error / se", (got_mean - mean) / se, "var ratio", got_var / s ** 2)
    assert hmc.acceptRate > 0.5
    assert np.all(np.abs(got_mean - mean) <= 5.0 * se)               # measured: 0.31, 0.72, 0.42 standard errors
    assert np.all(np.abs(got_var / s ** 2 - 1.0) <= 0.15)            # measured: 0.997, 0.999, 1.003
