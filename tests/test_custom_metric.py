"""The diagonal metric of a user-defined potential (METRIC = true of the plugin kernels, csrc/pbbi_custom.h;
pbbi_potential_set_metric_diag on a KIND_CUSTOM handle): row d of chain n has mass m_n m_d in the draw, the velocity, the
kick, the stored momentum and the kinetic energy.

The reference is test_glm_metric.py's NumPy restatement (r_integrate, r_hamiltonian, r_hmc_iter, r_run -- held to the oracle
at unit metric there) around orc.pot_custom(source, D, prm): the same C++ source compiled for the host.  Conventions are
test_glm_frame.py's: seed 4, iteration 1, chain0 = 2^32 - 70, kT = 2.5, MASS = 1 + 0.5 (n % 3), PBBI_DRAW_F64, the metric
30^((d + 0.5) / D), tolerance test_glm.TOL = 1e-10 through its check, masks equal with no chain excluded.

Source: QUARTIC of custom_sources.py with prm = [1.5, 0.75], L = 9 (test_custom_potential_polynomial_bit_exact's), N = 300 (a
ragged last block for the 256-chain and the 64-chain workgroups), and the dimensions that reach every path of the plugin:
D = 11 (register kernels, both forms, a partial first draw group), D = 21 (register kernel in kick-drift-kick form with a
partial second draw group; workspace kernels in reference order with a tail batch of 5 rows), D = 40 (workspace kernels)."""
import ctypes as C
import functools

import numpy as np
import pytest

import test_glm_frame as F
import test_glm_metric as M
from custom_sources import QUARTIC
from oracle import oracle as orc
from test_glm import check     # rel <= TOL = 1e-10, both of that file

N, SEED, ITER0, CHAIN0, KT, METHODS = 300, F.SEED, F.ITER0, F.CHAIN0, F.KT, F.METHODS
MASS = 1.0 + 0.5 * (np.arange(N) % 3)
PRM = [1.5, 0.75]
L, S_RUN = 9, 4
DIMS = (11, 21, 40)
# the step size per dimension: test_custom_potential_polynomial_bit_exact's holds in all three (the CPU test below: every
# accept test decisive, rejects and accepts in every case; Leapfrog rejects 1 to 7 of 1200, Stormer-Verlet 28 to 118)
STEP = {11: 0.07, 21: 0.07, 40: 0.07}
# (method, PBBI_KDK_FMA, PBBI_BETA_ACCEPT, PBBI_COMPAT_P_FROM_OLDQ); the restatement of a row does not depend on the form
RUN_ROWS = [(me, k, b, c) for me, k in (("Leapfrog", False), ("Leapfrog", True), ("Stormer-Verlet", False))
            for b in (False, True) for c in (False, True)]
ITER_ROWS = [("Leapfrog", False), ("Leapfrog", True), ("Stormer-Verlet", False)]
FUSED_S = 18     # one fused call of 16 iterations and one of 2
CANARY_N = 37
metric_of = M.metric_of


@functools.lru_cache(maxsize=None)
def _op(D):
    return orc.pot_custom(QUARTIC, D, PRM)


@functools.lru_cache(maxsize=None)
def _q0(D, n=N):
    q = np.ascontiguousarray(np.random.RandomState(100 + D).standard_normal((D, N))[:, :n])
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def _ref_run(D, method, beta, compat, S=S_RUN):
    """The restatement's run under metric_of(D), computed once and left unchanged."""
    q = np.array(_q0(D))
    s, p, rej, ratio, u = M.r_run(_op(D), method, q, MASS, metric_of(D), STEP[D], L, S, SEED, ITER0, CHAIN0, KT, beta, compat)
    return F._frozen(samples=s, momenta=p, rej=rej, ratio=ratio, u=u, q=q)


@functools.lru_cache(maxsize=None)
def _upload(D, n=N):
    """Uploaded draws of test 4: z sqrt(m_n m_d kT) and the Philox uniforms with every fourth forced to reject."""
    p = np.ascontiguousarray(orc.philox_normal(SEED, orc.STREAM_MOMENTUM | orc.STREAM_DRAW_F64, ITER0, CHAIN0, D, n)
                             * np.sqrt(M._mass2(_q0(D, n), MASS[:n], metric_of(D)) * KT))
    u = orc.philox_uniform(SEED, ITER0, CHAIN0, n)
    u[::4] = 1.5
    p.setflags(write=False)
    u.setflags(write=False)
    return p, u


@functools.lru_cache(maxsize=None)
def _ref_ends(D):
    """Where the restatement's Leapfrog integrate() under metric_of(D) ends from (_q0, the uploaded momenta): q1, p1."""
    q, p = np.array(_q0(D)), np.array(_upload(D)[0])
    M.r_integrate(_op(D), "Leapfrog", q, p, MASS, metric_of(D), STEP[D], L)
    q.setflags(write=False)
    p.setflags(write=False)
    return q, p


@functools.lru_cache(maxsize=None)
def _ref_iter(D, method, n=N):
    p_in, u = _upload(D, n)
    q, p = np.array(_q0(D, n)), np.array(p_in)
    ratio, rej = M.r_hmc_iter(_op(D), method, q, p, u, MASS[:n], metric_of(D), STEP[D], L, False, 1.0 / KT)
    return F._frozen(q=q, p=p, ratio=ratio, rej=rej)


# ---- CPU --------------------------------------------------------------------------------------------------------------
def test_custom_metric_cases_are_decisive():
    """Test 2.  The restatement alone, for every case of the GPU tests below: every value finite, no accept test within 1e-7
    (relative to max(1, ratio)) of its uniform -- so "masks are equal, no chain excluded" is a fair demand at 1e-10 -- and
    rejects and accepts in every case."""
    for D in DIMS:
        for method in METHODS:
            for beta in (False, True):
                for compat in (False, True):
                    o = _ref_run(D, method, beta, compat)
                    tag = f"run D={D} {method} beta={beta} compat={compat}"
                    assert np.all(np.isfinite(o["samples"])) and np.all(np.isfinite(o["momenta"])), tag
                    M._margin(tag, o["ratio"], o["u"])
                    assert 0 < o["rej"].sum() < o["rej"].size, tag
            o = _ref_iter(D, method)
            tag = f"iter D={D} {method}"
            M._margin(tag, o["ratio"], _upload(D)[1])
            assert 0 < o["rej"].sum() < N and not o["rej"][1::4].all(), tag
    for method in METHODS:
        M._margin(f"canary {method}", _ref_iter(11, method, CANARY_N)["ratio"], _upload(11, CANARY_N)[1])
    o = _ref_run(11, "Leapfrog", True, False, FUSED_S)
    M._margin("fused", o["ratio"], o["u"])
    assert 0 < o["rej"].sum() < o["rej"].size
    g = _gauss_cpu()
    assert 0.5 < g["rate"] < 1.0


def _lambda_and_schools():
    """The two traced callables of test 10: the three-row Gaussian as a lambda, and the centred eight schools model."""
    from physicsbasedbayesianinference_amd import trace as jnp
    from physicsbasedbayesianinference_amd.models import eight_schools_potential
    prec, mean = 1.0 / G_SCALES ** 2, G_MEAN
    return (lambda q: 0.5 * jnp.sum(prec * (q - mean) ** 2)), eight_schools_potential(centered=True)


def test_custom_metric_plugins_build_for_gfx950():
    """The seven plugins of the GPU tests below compile for gfx950 here, without a GPU (hipcc cross-compiles), METRIC kernels
    and all -- and travel to the GPU machine in the in-tree cache, so that the -m gpu run does not spend its time in hipcc."""
    from concurrent.futures import ThreadPoolExecutor
    from physicsbasedbayesianinference_amd import trace as jnp
    from physicsbasedbayesianinference_amd.custom import compile_plugin
    fn, schools = _lambda_and_schools()
    jobs = [(QUARTIC, "float64", D) for D in DIMS] + [(QUARTIC, "float32", 7), (GAUSS3, "float64", 3),
            (jnp.plan_potential(fn, D=3, prefer="source")["source"], "float64", 3),
            (jnp.plan_potential(schools, D=10)["source"], "float64", 10)]
    with ThreadPoolExecutor(4) as pool:
        for so in pool.map(lambda j: compile_plugin(j[0], j[1], D=j[2]), jobs):
            assert so.endswith(".so")


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


@functools.lru_cache(maxsize=None)
def _pot(D):
    """One handle (and one plugin) per dimension for all tests; each test sets the metric it needs."""
    from physicsbasedbayesianinference_amd.custom import CustomPotential
    return CustomPotential(D, QUARTIC, PRM)


def _mpot(D):
    pot = _pot(D)
    pot.set_metric(metric_of(D))
    return pot


def _flags(lib, kdk, beta, compat):
    return (lib.DRAW_F64 | (lib.KDK_FMA if kdk else 0) | (lib.BETA_ACCEPT if beta else 0)
            | (lib.COMPAT_P_FROM_OLDQ if compat else 0))


def _run_outputs(lib, pot, D):
    """pbbi_hmc_run, S = 4, leading stride N + 5, for every row of RUN_ROWS: {row: (samples, momenta, reject, ratio, state,
    padding)}."""
    return {row: F._device_run(lib, pot, row[0], np.array(_q0(D)), MASS, STEP[D], L, S_RUN, _flags(lib, *row[1:]), KT, pad=5)
            for row in RUN_ROWS}


def _integrate(lib, pot, method, q0, p0, mass, h, want_v=True):
    import torch
    d = F._dev()
    Dt, n = q0.shape
    qd, pd, vd = d.as_device(np.array(q0), 0, np.float64), d.as_device(np.array(p0), 0, np.float64), d.empty((Dt, n), np.float64, 0)
    md = d.as_device(mass, 0, np.float64)
    lib.call("pbbi_integrate", pot.handle, orc.METHODS[method], qd.data_ptr(), pd.data_ptr(), md.data_ptr(),
             vd.data_ptr() if want_v else None, n, n, float(h), L, d.stream_ptr(0))
    torch.cuda.synchronize()
    return d.to_numpy(qd), d.to_numpy(pd), d.to_numpy(vd)


def _energy(lib, pot, q, p, mass):
    import torch
    d = F._dev()
    n = q.shape[1]
    qd, pd, md = (d.as_device(np.array(a), 0, np.float64) for a in (q, p, mass))
    Hd, wd = d.empty((n,), np.float64, 0), d.empty((n,), np.float64, 0)
    lib.call("pbbi_energy", pot.handle, qd.data_ptr(), pd.data_ptr(), md.data_ptr(), n, n, Hd.data_ptr(), wd.data_ptr(),
             d.stream_ptr(0))
    torch.cuda.synchronize()
    return d.to_numpy(Hd), d.to_numpy(wd)


def _weights_ratio(lib, pot, nq, np_, oq, op, mass):
    import torch
    d = F._dev()
    n = nq.shape[1]
    a, b, c, e, md = (d.as_device(np.array(x), 0, np.float64) for x in (nq, np_, oq, op, mass))
    rd = d.empty((n,), np.float64, 0)
    lib.call("pbbi_weights_ratio", pot.handle, a.data_ptr(), b.data_ptr(), c.data_ptr(), e.data_ptr(), md.data_ptr(), n, n,
             rd.data_ptr(), d.stream_ptr(0))
    torch.cuda.synchronize()
    return d.to_numpy(rd)


def _upload_outputs(lib, pot, D):
    """Test 4's calls on a handle: one pbbi_hmc_iter_kt per row of ITER_ROWS with uploaded p, u (PBBI_BETA_ACCEPT, non-compat),
    pbbi_integrate with v_out per method, pbbi_energy and pbbi_weights_ratio: {tag: arrays}."""
    p_in, u = _upload(D)
    q0 = _q0(D)
    out = {}
    for method, kdk in ITER_ROWS:
        out["iter", method, kdk] = F._device_iter(lib, pot, method, q0, p_in, u, MASS, STEP[D], L,
                                                  lib.BETA_ACCEPT | (lib.KDK_FMA if kdk else 0), KT)
    for method in METHODS:
        out["integrate", method] = _integrate(lib, pot, method, q0, p_in, MASS, STEP[D])
    out["energy"] = _energy(lib, pot, q0, p_in, MASS)
    q1, p1 = _ref_ends(D)
    out["ratio"] = (_weights_ratio(lib, pot, q1, p1, q0, p_in, MASS),)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("D", DIMS)
def test_custom_metric_run_vs_restatement(P, lib, D):
    """Test 1.  pbbi_hmc_run on a custom handle with a metric, S = 4, kT = 2.5, MASS, PBBI_DRAW_F64, leading stride N + 5:
    {Leapfrog, Leapfrog with PBBI_KDK_FMA, Stormer-Verlet} x {0, PBBI_BETA_ACCEPT} x {non-compat, compat} against the
    restatement -- samples, momenta (the redrawn z sqrt(m_n m_d kT) of a rejected non-compat chain among them), ratios, the
    final state within TOL; masks equal; padding columns untouched; rejects and accepts in every case."""
    pot = _mpot(D)
    assert np.array_equal(pot.metric, metric_of(D))
    got = _run_outputs(lib, pot, D)
    for row in RUN_ROWS:
        method, kdk, beta, compat = row
        o = _ref_run(D, method, beta, compat)
        gs, gm, grej, gratio, gq, gpad = got[row]
        tag = f"D={D} {method} kdk={kdk} beta_accept={beta} compat={compat}"
        print(tag, "mask mismatches", int((grej != o["rej"]).sum()), "rejected", int(grej.sum()))
        assert np.array_equal(grej, o["rej"]) and 0 < grej.sum() < grej.size, tag
        check(tag + " samples", gs, o["samples"])
        check(tag + " momenta", gm, o["momenta"])
        check(tag + " ratio", gratio, o["ratio"])
        check(tag + " final state", gq, o["q"])
        assert np.all(gpad == F.POISON), tag


@pytest.mark.gpu
def test_custom_metric_fused_call_boundary(P, lib):
    """Test 3.  D = 11, S = 18 with in-kernel draws: one fused call of 16 iterations and one of 2 (the carried potential
    energy crosses both) equal 18 runs of S = 1 bit for bit, device against device, with the metric set; the last slab
    agrees with the restatement at TOL."""
    D = 11
    pot = _mpot(D)
    flags = _flags(lib, False, True, False)
    assert "iterations per launch: up to 16" in _describe(lib, pot, FUSED_S, flags)
    gs, gm, grej, gratio, gq, _ = F._device_run(lib, pot, "Leapfrog", np.array(_q0(D)), MASS, STEP[D], L, FUSED_S, flags, KT)
    q = np.array(_q0(D))
    for i in range(FUSED_S):
        s1, m1, rej1, ratio1, q, _ = F._device_run(lib, pot, "Leapfrog", q, MASS, STEP[D], L, 1, flags, KT, iter0=ITER0 + i)
        assert np.array_equal(s1[0], gs[i]) and np.array_equal(m1[0], gm[i]), i
        assert np.array_equal(rej1[0], grej[i]) and np.array_equal(ratio1[0], gratio[i]), i
    assert np.array_equal(q, gq)
    o = _ref_run(D, "Leapfrog", True, False, FUSED_S)
    assert np.array_equal(grej, o["rej"]) and 0 < grej.sum() < grej.size
    check("fused last slab", gs[-1], o["samples"][-1])
    check("fused last momenta", gm[-1], o["momenta"][-1])
    check("fused ratios", gratio, o["ratio"])


@pytest.mark.gpu
@pytest.mark.parametrize("D", DIMS)
def test_custom_metric_uploaded_integrate_energy_vs_restatement(P, lib, D):
    """Test 4.  One pbbi_hmc_iter_kt per form with uploaded momenta and uniforms (u[::4] = 1.5 forces rejects): masks equal,
    q, p, ratio within TOL, a rejected chain's p_out is its p_in bit for bit.  pbbi_integrate with v_out (v = p / (m_n m_d)),
    pbbi_energy (H and exp(-H)) and pbbi_weights_ratio against r_integrate / r_hamiltonian."""
    pot, op, md = _mpot(D), _op(D), metric_of(D)
    got = _upload_outputs(lib, pot, D)
    p_in, u = _upload(D)
    q0 = _q0(D)
    for method, kdk in ITER_ROWS:
        o = _ref_iter(D, method)
        gq, gp, gratio, grej = got["iter", method, kdk]
        tag = f"D={D} {method} kdk={kdk}"
        assert np.array_equal(grej, o["rej"]) and grej[::4].all() and 0 < grej.sum() < N, tag
        check(tag + " q", gq, o["q"])
        check(tag + " p", gp, o["p"])
        check(tag + " ratio", gratio, o["ratio"])
        assert np.array_equal(gp[:, grej], p_in[:, grej]) and np.array_equal(gq[:, grej], q0[:, grej]), tag
    ends = {}
    for method in METHODS:
        q, p = np.array(q0), np.array(p_in)
        v = M.r_integrate(op, method, q, p, MASS, md, STEP[D], L)
        ends[method] = (q, p)
        gq, gp, gv = got["integrate", method]
        check(f"D={D} {method} integrate q", gq, q)
        check(f"D={D} {method} integrate p", gp, p)
        check(f"D={D} {method} integrate v", gv, v)
    H0 = M.r_hamiltonian(op, np.array(q0), np.array(p_in), MASS, md)
    gH, gw = got["energy"]
    check(f"D={D} H", gH, H0)
    assert np.max(np.abs(gw / np.exp(-H0) - 1.0)) <= 1e-10 * max(1.0, np.max(np.abs(H0)))
    H1 = M.r_hamiltonian(op, *(np.array(a) for a in _ref_ends(D)), MASS, md)
    check(f"D={D} weights ratio", got["ratio"][0], np.exp(H0 - H1))


@pytest.mark.gpu
@pytest.mark.parametrize("D", DIMS)
def test_custom_ones_metric_is_the_handle_without_one_bit_for_bit(P, lib, D):
    """Test 5.  Device against device: with set_metric(ones) every output of tests 1 and 4 is array_equal to the same call on
    the handle without a metric (each use multiplies by exactly 1.0), and after set_metric(None) again; the metric in
    place does change the run."""
    pot = _pot(D)
    pot.set_metric(None)
    assert pot.metric is None
    want_run, want_up = _run_outputs(lib, pot, D), _upload_outputs(lib, pot, D)
    assert any(w[2].any() for w in want_run.values())
    pot.set_metric(metric_of(D))
    assert not np.array_equal(_run_outputs(lib, pot, D)[RUN_ROWS[0]][0], want_run[RUN_ROWS[0]][0])
    for setting in ("ones", None):
        pot.set_metric(np.ones(D) if setting == "ones" else None)
        assert (pot.metric is None) if setting is None else np.array_equal(pot.metric, np.ones(D))
        for want, got in ((want_run, _run_outputs(lib, pot, D)), (want_up, _upload_outputs(lib, pot, D))):
            for key in want:
                for i, (a, r) in enumerate(zip(got[key], want[key])):
                    assert np.array_equal(a, r), (D, setting, key, i)


@pytest.mark.gpu
def test_custom_metric_fp32(P, lib):
    """Test 6.  CustomPotential(7, QUARTIC, [1.0, 0.5], dtype="float32") with a metric: integrate() against r_integrate at
    2e-5 (test_custom_potential_fp32_and_errors' tolerance and inputs)."""
    from physicsbasedbayesianinference_amd.custom import CustomPotential
    D, n = 7, 100
    pot32, op = CustomPotential(D, QUARTIC, [1.0, 0.5], dtype="float32"), orc.pot_custom(QUARTIC, D, [1.0, 0.5])
    md = metric_of(D)
    pot32.set_metric(md)
    assert np.array_equal(pot32.metric, md)
    rs = np.random.RandomState(2)
    q = rs.standard_normal((D, n)).astype(np.float32).astype(np.float64)
    p = (rs.standard_normal((D, n)) * np.sqrt(md)[:, None]).astype(np.float32).astype(np.float64)
    for cls, method in ((P.Leapfrog, "Leapfrog"), (P.StormerVerlet, "Stormer-Verlet")):
        ens = P.Ensemble(D, n)
        ens.q, ens.p = q.copy(), p.copy()
        qi, pi = cls(ens, 0.05, 0.5 + 1e-6, pot32).integrate()
        q2, p2 = q.copy(), p.copy()
        M.r_integrate(op, method, q2, p2, None, md, 0.05, 10)
        for tag, a, b in (("q", qi, q2), ("p", pi, p2)):
            err = float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))
            print(f"fp32 {method} {tag}: {err:.2e}")
            assert err <= 2e-5, (method, tag, err)


@pytest.mark.gpu
def test_custom_metric_state_inside_a_canary_allocation(P, lib):
    """Test 7.  D = 11, N = 37 (a ragged block of every kernel), leading dimension 42, the state, momentum and output arrays
    rows [1, 1 + D) of (D + 18, ldn) allocations full of NaN: pbbi_integrate with v_out and one pbbi_hmc_iter_kt (non-compat,
    masses) per method.  Results within TOL of the restatement, every element outside the blocks keeps its NaN bits, the
    inputs are unchanged."""
    import torch
    d = F._dev()
    D, n, ldn = 11, CANARY_N, CANARY_N + 5
    pot, op, md, mass, h = _mpot(D), _op(D), metric_of(D), MASS[:CANARY_N], STEP[11]
    q0 = np.array(_q0(D, n))
    p0, u = (np.array(a) for a in _upload(D, n))
    empty_block = np.full((D, n), np.nan)
    mdev, st = d.as_device(mass, 0, np.float64), d.stream_ptr(0)
    for method in METHODS:
        q, p = q0.copy(), p0.copy()
        v = M.r_integrate(op, method, q, p, mass, md, h, L)
        (qt, qp), (pt, pp), (vt, vp) = F._canary(q0, ldn), F._canary(p0, ldn), F._canary(empty_block, ldn)
        lib.call("pbbi_integrate", pot.handle, orc.METHODS[method], qp, pp, mdev.data_ptr(), vp, n, ldn, h, L, st)
        torch.cuda.synchronize()
        check(method + " integrate q", F._canary_result(qt, D, n), q)
        check(method + " integrate p", F._canary_result(pt, D, n), p)
        check(method + " integrate v", F._canary_result(vt, D, n), v)
        o = _ref_iter(D, method, n)
        (qt, qp), (pt, pp) = F._canary(q0, ldn), F._canary(p0, ldn)
        (qot, qop), (pot_, pop) = F._canary(empty_block, ldn), F._canary(empty_block, ldn)
        ud, ro, rj = d.as_device(u, 0, np.float64), d.empty((n,), np.float64, 0), d.empty((n,), np.uint8, 0)
        lib.call("pbbi_hmc_iter_kt", pot.handle, orc.METHODS[method], qp, pp, ud.data_ptr(), mdev.data_ptr(), qop, pop,
                 ro.data_ptr(), rj.data_ptr(), n, ldn, h, L, lib.BETA_ACCEPT, KT, st)
        torch.cuda.synchronize()
        assert np.array_equal(d.to_numpy(rj).astype(bool), o["rej"]), method
        check(method + " iter q", F._canary_result(qot, D, n), o["q"])
        check(method + " iter p", F._canary_result(pot_, D, n), o["p"])
        check(method + " iter ratio", d.to_numpy(ro), o["ratio"])
        assert np.array_equal(F._canary_result(qt, D, n), q0) and np.array_equal(F._canary_result(pt, D, n), p0)


def _describe(lib, pot, S, flags, n=N):
    buf = C.create_string_buffer(4096)
    lib.call("pbbi_describe_run", pot.handle, orc.METHODS["Leapfrog"], n, n, L, S, flags, buf, len(buf))
    return buf.value.decode()


@pytest.mark.gpu
def test_custom_metric_entries_refusals_and_description(P, lib):
    """Test 8.  A wrong D and the entries 0, -2, NaN, inf are PBBI_ERR_INVALID with the messages of the GLM handles and leave
    the metric as it was; get_metric_diag round-trips; describeRun() names the metric only while one is set; per-chain
    lengths and GIST stay refused with the same code and message with and without a metric; pbbi_potential_eval does not see
    the metric."""
    from scipy.constants import k as kB
    import torch
    d = F._dev()
    D = 11
    pot, md = _mpot(D), metric_of(D)
    setter = lib.load().pbbi_potential_set_metric_diag
    for bad_D in (D - 1, D + 1):
        v = np.ones(bad_D)
        assert setter(pot.handle, v.ctypes.data_as(C.POINTER(C.c_double)), bad_D) == lib.ERR_INVALID
        assert "state dimension" in lib.last_error()
        with pytest.raises(ValueError):
            pot.set_metric(v)
    for bad in (0.0, -2.0, np.nan, np.inf):
        v = md.copy()
        v[D - 1] = bad
        assert setter(pot.handle, v.ctypes.data_as(C.POINTER(C.c_double)), D) == lib.ERR_INVALID
        assert "finite and > 0" in lib.last_error()
    out, has = np.zeros(D), C.c_int(0)
    lib.call("pbbi_potential_get_metric_diag", pot.handle, out.ctypes.data_as(C.POINTER(C.c_double)), D, C.byref(has))
    assert has.value == 1 and np.array_equal(out, md) and np.array_equal(pot.metric, md)
    hmc = P.HMC(P.Ensemble(D, 64), 0.8, 0.1, None, potential=pot, rng="philox", seed=13, verbose=False)
    other = P.HMC(P.Ensemble(D, 32), 0.8, 0.1, None, potential=pot, rng="philox", seed=14, verbose=False)
    assert np.array_equal(hmc.massMatrix, md) and np.array_equal(other.massMatrix, md)
    text = hmc.describeRun()
    print(text)
    assert "user-potential plugin" in text and "diagonal metric" in text and "register kernel" in text
    wide = _mpot(40)
    wtext = _describe(lib, wide, 4, lib.DRAW_F64)
    print(wtext)
    assert "diagonal metric" in wtext and "workspace kernel" in wtext and "spill" not in wtext
    q0 = np.array(_q0(D))
    U0, g0 = pot.value_and_gradient(q0)
    errs = []
    for with_metric in (True, False):
        pot.set_metric(md if with_metric else None)
        h = P.HMC(P.Ensemble(D, 64), 0.8, 0.1, None, potential=pot, rng="philox", seed=13, verbose=False)
        with pytest.raises(lib.PbbiError) as e:
            h.getSamplesGIST(2, 1 / kB, 1.0)
        errs.append((e.value.code, str(e.value)))
        q = d.as_device(q0[:, :64], 0, np.float64)
        steps = torch.full((64,), 3, dtype=torch.int32, device="cuda:0")
        out_s = d.empty((1, D, 64), np.float64, 0)
        rc = lib.load().pbbi_hmc_run_dyn(pot.handle, 0, q.data_ptr(), None, steps.data_ptr(), out_s.data_ptr(), None, None,
                                         None, 64, 64, 0.1, 8, 1, lib.PER_CHAIN_STEPS, SEED, ITER0, 0, 1.0, d.stream_ptr(0))
        errs.append((rc, lib.last_error()))
    assert errs[0] == errs[2] and errs[1] == errs[3]
    assert errs[0][0] == lib.ERR_UNSUPPORTED and errs[1][0] == lib.ERR_UNSUPPORTED
    assert hmc.massMatrix is None and "diagonal metric" not in hmc.describeRun()
    U1, g1 = pot.value_and_gradient(q0)
    assert np.array_equal(U0, U1) and np.array_equal(g0, g1)
    U_or, g_or = orc.potential(_op(D), q0, want_grad=True)
    assert np.array_equal(U0, U_or) and np.array_equal(g0, g_or)


# ---- what the feature is for ------------------------------------------------------------------------------------------
# A three-row Gaussian as C++ source, U = 0.5 sum_d prec_d (q_d - mean_d)^2, prm = means | precisions, posterior scales
# s = (1, 0.1, 0.01); sizes and steps are test_glm_metric.py's (N = 4096, h = 0.5, L = 8, S = 4, a stationary start).
GAUSS3 = '''
template <class Q>
PBBI_FN T potential(const Q& q, int D, const T* prm) {
    T s = 0;
    for (int j = 0; j < D; ++j) { const T d = q[j] - prm[j]; s += prm[D + j] * (d * d); }
    return T(0.5) * s;
}
template <class Q, class G>
PBBI_FN void gradient(const Q& q, G& g, int D, const T* prm) {
    for (int j = 0; j < D; ++j) g[j] = prm[D + j] * (q[j] - prm[j]);
}
'''
G_N, G_H, G_L, G_S, G_T = M.G_N, M.G_H, M.G_L, M.G_S, M.G_T
G_SCALES = np.array([1.0, 0.1, 0.01])
G_MEAN = np.array([0.8, -0.3, 0.05])
G_PRM = np.concatenate([G_MEAN, 1.0 / G_SCALES ** 2])


@functools.lru_cache(maxsize=None)
def _gauss_q0():
    q0 = np.ascontiguousarray(G_MEAN[:, None] + G_SCALES[:, None] * np.random.RandomState(29).standard_normal((3, G_N)))
    q0.setflags(write=False)
    return q0


@functools.lru_cache(maxsize=None)
def _gauss_cpu():
    """The restatement at the GPU test's sizes with the exact metric: the acceptance rate over G_S iterations of G_N chains,
    and one uploaded iteration for the lambda's comparison."""
    op = orc.pot_custom(GAUSS3, 3, G_PRM)
    q = np.array(_gauss_q0())
    _, _, rej, ratio, u = M.r_run(op, "Leapfrog", q, None, 1.0 / G_SCALES ** 2, G_H, G_L, G_S, SEED, ITER0, 0, 1.0, False, False)
    M._margin("gaussian exact metric", ratio, u)
    return dict(rate=1.0 - float(rej.mean()))


@pytest.mark.gpu
def test_custom_metric_is_what_makes_the_scaled_gaussian_sampleable(P, lib):
    """Test 9.  With the exact metric m_d = 1 / s_d^2 every row has h omega = 0.5 at h = 0.5 and the device's acceptance rate
    clears the restatement's own rate at the same sizes minus 3 binomial standard errors; without a metric the stiff row
    has h omega = 50 and the rate is below 0.01.  adaptMassMatrix from the unit metric (windows 25, 100, simulTime 1.5)
    returns m_d s_d^2 within (0.5, 2) in every row (test_gaussian_scheme_recovers_the_metric_in_numpy derives the bound)
    and leaves stepSize / numSteps consistent."""
    from scipy.constants import k as kB
    from physicsbasedbayesianinference_amd.custom import CustomPotential
    pot = CustomPotential(3, GAUSS3, G_PRM)
    s, q0 = G_SCALES, _gauss_q0()

    def rate():
        rej = F._device_run(lib, pot, "Leapfrog", np.array(q0), None, G_H, G_L, G_S, lib.DRAW_F64, 1.0, chain0=0)[2]
        return 1.0 - float(rej.mean())
    bare = rate()
    pot.set_metric(1.0 / s ** 2)
    exact = rate()
    cpu = _gauss_cpu()["rate"]
    floor = cpu - 3.0 * np.sqrt(cpu * (1.0 - cpu) / (G_S * G_N))
    print(f"acceptance: exact metric {exact:.4f} (restatement {cpu:.4f}, floor {floor:.4f}), no metric {bare:.5f}")
    assert exact >= floor
    assert bare < 0.01
    pot.set_metric(None)
    hmc = P.HMC(P.Ensemble(3, G_N), G_T, 0.01, None, potential=pot, rng="philox", seed=SEED, verbose=False, compat=False,
                draw_f64=True)
    m = hmc.adaptMassMatrix(1 / kB, 1.0, windows=(25, 100))
    print("adapted metric", m, "exact", 1.0 / s ** 2, "ratio", m * s ** 2, "step", hmc.stepSize, hmc.integrator.numSteps)
    assert np.array_equal(m, pot.metric) and np.array_equal(m, hmc.massMatrix)
    assert np.all(m * s ** 2 < 2.0) and np.all(m * s ** 2 > 0.5), m * s ** 2
    assert hmc.integrator.numSteps == max(1, int(hmc.simulTime / hmc.stepSize)) and hmc.integrator.stepSize == hmc.stepSize


@pytest.mark.gpu
def test_custom_metric_through_a_lambda(P, lib):
    """Test 10.  trace_potential(lambda, D = 3, prefer="source") carries set_metric and one uploaded iteration under the metric
    equals the hand-written source's (TOL, masks equal); the same lambda without prefer resolves to a descriptor and
    HMC.setMassMatrix raises ValueError; models.eight_schools_potential(centered=True) accepts adaptMassMatrix (N = 1024,
    windows 25, 50) and returns ten finite positive masses that are not all equal."""
    from scipy.constants import k as kB
    from physicsbasedbayesianinference_amd import trace as jnp
    from physicsbasedbayesianinference_amd.custom import CustomPotential
    md = 1.0 / G_SCALES ** 2
    fn, schools = _lambda_and_schools()
    traced = jnp.trace_potential(fn, D=3, prefer="source")
    assert traced.kind == "custom" and hasattr(traced, "set_metric")
    hand = CustomPotential(3, GAUSS3, G_PRM)
    n = 300
    q0 = np.array(_gauss_q0()[:, :n])
    p0 = np.ascontiguousarray(orc.philox_normal(SEED, orc.STREAM_MOMENTUM | orc.STREAM_DRAW_F64, ITER0, 0, 3, n)
                              * np.sqrt(M._mass2(q0, MASS, md) * KT))
    u = orc.philox_uniform(SEED, ITER0, 0, n)
    outs = []
    for pot in (traced, hand):
        pot.set_metric(md)
        outs.append(F._device_iter(lib, pot, "Leapfrog", q0, p0, u, MASS, G_H, G_L, lib.BETA_ACCEPT, KT))
    assert np.array_equal(outs[0][3], outs[1][3])
    for tag, a, b in zip(("q", "p", "ratio"), outs[0], outs[1]):
        check("lambda " + tag, a, b)
    q, p = q0.copy(), p0.copy()
    ratio, rej = M.r_hmc_iter(orc.pot_custom(GAUSS3, 3, G_PRM), "Leapfrog", q, p, u, MASS, md, G_H, G_L, False, 1.0 / KT)
    M._margin("lambda", ratio, u)
    assert np.array_equal(outs[1][3], rej)
    check("hand-written q", outs[1][0], q)
    check("hand-written ratio", outs[1][2], ratio)
    traced.set_metric(None)
    plain = P.HMC(P.Ensemble(3, 64), 1.0, 0.1, None, potential=fn, rng="philox", seed=3, verbose=False)
    assert not hasattr(plain._pot, "set_metric")
    with pytest.raises(ValueError, match="GLM potentials only"):
        plain.setMassMatrix(np.ones(3))
    # (simulTime 0.5 from a start of spread 0.5 at target 0.9: measured to finish for seeds 2, 3 and 4.  The sampling test's
    #  simulTime 1.5 / step 0.015 and a start of spread 1 do not: dual averaging probes steps of ten times the first one, a
    #  chain in the funnel's neck overflows to a NaN ratio, which the reference's accept rule takes, and the window's pooled
    #  variance is then not finite -- adaptMassMatrix raises FloatingPointError, as it says it does.)
    hmc = P.HMC(P.Ensemble(10, 1024), 0.5, 0.002, None, potential=schools, rng="philox",
                seed=2, verbose=False, kdk_fma=False)
    assert hmc._pot.kind == "custom"
    m = hmc.adaptMassMatrix(1 / kB, 0.5, windows=(25, 50), target=0.9)
    print("eight schools (centred) adapted metric", m)
    assert m.shape == (10,) and np.all(np.isfinite(m)) and np.all(m > 0.0) and len(set(m.tolist())) > 1
    hmc._pot.set_metric(None)
