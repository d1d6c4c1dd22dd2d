"""The kernel routes the suite had stopped reaching, each held to the oracle for an accept/reject step, and the census
of who holds which.

route_hmc / lane_hmc_iter send one API call to one of about fifteen kernel families (potential, D, dtype, integrator,
PBBI_KDK_FMA).  When a faster family took over a range of D, the tests written for the old one kept their shapes and
now run the new kernel; the old kernel still serves the sizes next to that range.  Every test here therefore says
which family it means -- route_of (test_gpu_parity.py: pbbi_describe_run's text) is asserted on the test's own
arguments before anything is launched -- and sits on the smallest shapes at which only that family is left.

Census: family (as lane_route_name / route_hmc / pbbi_describe_run name it) -> the test that holds its HMC step to
the oracle.  "F64_RUNS <row>" is test_gpu_parity.test_hmc_run_with_f64_draws_vs_host_only_oracle[<row>], whose rows
assert their route; the other entries are witnessed by test_census_witnesses below, on the named test's shape.

  k_lane_hmc            D <= 16: F64_RUNS lane_diag8; Rosenbrock, Stormer-Verlet, reference order, D = 12 .. 64
                        (all that is left for DMAX 32 / 64): test_lane_rosenbrock_stormer_verlet_* here
  k_ros2_hmc            reference order: F64_RUNS lane2_ros32_exact, test_rosenbrock_two_lane_kernel_bitexact;
                        kick-drift-kick: F64_RUNS lane2_ros32_kdk, lane2_ros24_kdk_mass
  k_sep_hmc             F64_RUNS sepn_diag64_kdk, test_separable_multilane_kdk
  k_sep_exact_hmc       F64_RUNS sepx_diag64_exact, test_streaming_lane_path_bit_exact (its three rows with
                        16 < D <= 256), test_separable_multiwave_reference_order_bitexact
  k_rosg_hmc            F64_RUNS rosg_ros64_kdk, test_rosenbrock_kdk_stormer_verlet (the only Stormer-Verlet form)
  k_rosg_exact_hmc      F64_RUNS rosgx_ros64_exact, test_streaming_lane_path_bit_exact[rosenbrock-70]
  k_rosn_hmc            F64_RUNS rosn_ros200_kdk
  k_stream_hmc  fp64    Rosenbrock: F64_RUNS stream_ros300, test_streaming_lane_path_bit_exact (128 Stormer-Verlet,
                        257); separable (D > 256 only): F64_RUNS stream_diag300, test_streaming_lane_path_bit_exact
                        (257 / 300), test_stream_kdk_flag_changes_nothing here
  k_stream_hmc  fp32    F64_RUNS stream_diag12_f32 (diagonal, Leapfrog, unit masses); harmonic, Rosenbrock, masses
                        and Stormer-Verlet: test_stream_fp32_hmc_iter_vs_fp64_oracle here
  k_dense_hmc           F64_RUNS dense*, test_dense_inplace_kick.py
  streamed P            F64_RUNS dstream_dense200, test_big_dense_getsamples_vs_oracle,
                        test_gpu_fullsize.test_dense_stream_strided_state_and_small_ensembles
  kernels_big   fp64    L >= 1 (D > 256 only): test_gemm_fp64_* here; L = 0: test_big_dense_hmc_iter_methods_vs_oracle
  kernels_big   fp32    F64_RUNS gemm_dense256_f32, test_big_wide_tile_fp32_vs_oracle, test_c5_shape_fp32_vs_fp64_oracle
  k_glm                 test_glm.test_glm_uploaded_draw_iteration_matches_oracle, test_glm_philox_run_matches_oracle
                        (every GLM handle takes this family: route_hmc's first line; test_glm_unsupported_calls
                        reads the name from pbbi_describe_run)
  plugins               F64_RUNS custom_quartic9 (registers), custom_quartic48 (workspace),
                        test_custom_potential_polynomial_bit_exact
  k_lane_dyn_hmc        test_per_chain_steps_lane_kernels_bitexact[diag5 / diag30 / harm3 / ros12]
  k_ros2_hmc<DYN>       test_per_chain_steps_lane_kernels_bitexact[ros20 / ros32]
  k_sep_hmc<DYN>        test_per_chain_steps_multilane_kdk_kernels[diag-*]
  k_rosg_hmc<DYN>       test_per_chain_steps_multilane_kdk_kernels[ros-*]
  dense kernels, per-chain lengths (pbbi_describe_run has no name of its own for them: "k_dense_hmc" / "streamed P"
                        with the carry switched off): test_per_chain_steps_dense_kernel, test_uturn_stop_dense_kernel

No family is left without a test.  Everywhere N = 150 (a full 128-chain tile and a ragged one; two full waves and a
ragged one) and the Philox counters are seed 4, iteration 1, chain0 = 2^32 - 70, so the chain counter carries into
its high word inside the ensemble.  Runs with PBBI_DRAW_F64 are drawn by the oracle itself (oracle.hmc_run_philox);
uploaded momenta and uniforms are the oracle's double-precision draws for the same counters.
"""
import numpy as np
import pytest

from oracle import oracle as orc
from test_gpu_parity import RTOL_DENSE, route_of, scaled_err

pytestmark = pytest.mark.gpu

N, SEED, ITER0, CHAIN0 = 150, 4, 1, 2 ** 32 - 70
MASS = 1.0 + 0.5 * (np.arange(N) % 3)
METHODS = ["Leapfrog", "Stormer-Verlet"]
F64 = orc.STREAM_DRAW_F64


@pytest.fixture(scope="module")
def P():
    import physicsbasedbayesianinference_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def lib():
    from physicsbasedbayesianinference_amd import _lib
    _lib.load()
    return _lib


_POTS = {}


def _problem(P, kind, D, dtype="float64"):
    """One device potential and one oracle potential per (kind, D, dtype) for the whole module; returns them and
    the point the chains start around."""
    key = (kind, D, dtype)
    if key not in _POTS:
        rs = np.random.RandomState(D)
        if kind == "dense":   # precision inv(A A^T / D + I); D = 384 has zero mean (the ZMEAN instantiation)
            A = rs.standard_normal((D, D))
            Pm = np.linalg.inv(A @ A.T / D + np.eye(D))
            Pm = 0.5 * (Pm + Pm.T)
            mu = np.zeros(D) if D == 384 else 0.5 * rs.standard_normal(D)
            _POTS[key] = (P.GaussianDense(None if D == 384 else mu, precision=Pm, const=0.1, dtype=dtype),
                          orc.pot_gauss_dense(mu, Pm, 0.1), mu)
        elif kind == "harmonic":
            k = rs.uniform(0.5, 2.0, D)
            _POTS[key] = (P.Harmonic(k, dtype=dtype), orc.pot_harmonic(k), np.zeros(D))
        elif kind == "diag":
            mu, prec = rs.standard_normal(D), rs.uniform(0.5, 2.0, D)
            _POTS[key] = (P.GaussianDiag(mu, prec=prec, const=0.25, dtype=dtype), orc.pot_gauss_diag(mu, prec, 0.25),
                          np.zeros(D))
        else:
            _POTS[key] = (P.Rosenbrock(D, dtype=dtype), orc.pot_rosenbrock(D), np.ones(D))
    return _POTS[key]


def _start(D, centre, scale):
    return np.ascontiguousarray(orc.philox_normal(SEED, orc.STREAM_POSITION | F64, ITER0, CHAIN0, D, N, scale)
                                + centre[:, None])


def _draws(D, mass):
    """The oracle's double-precision momentum and uniform draws of iteration ITER0 (uploaded to pbbi_hmc_iter)."""
    p = orc.philox_normal(SEED, orc.STREAM_MOMENTUM | F64, ITER0, CHAIN0, D, N, np.sqrt(MASS) if mass else 1.0)
    return np.ascontiguousarray(p), orc.philox_uniform(SEED, ITER0, CHAIN0, N)


def _iter(lib, pot, method, q, p, u, m, h, L, flags, npdt=np.float64):
    """One pbbi_hmc_iter on host arrays in the handle's dtype; returns q, p, ratio as float64 and the reject mask."""
    import torch
    from physicsbasedbayesianinference_amd._device import as_device, empty, stream_ptr, to_numpy
    D, n = q.shape
    qd, pd, ud = (as_device(x, 0, npdt) for x in (q, p, u))
    md = as_device(m, 0, npdt) if m is not None else None
    qo, po = empty((D, n), npdt, 0), empty((D, n), npdt, 0)
    ro, rj = empty((n,), npdt, 0), empty((n,), np.uint8, 0)
    lib.call("pbbi_hmc_iter", pot.handle, orc.METHODS[method], qd.data_ptr(), pd.data_ptr(), ud.data_ptr(),
             md.data_ptr() if md is not None else None, qo.data_ptr(), po.data_ptr(), ro.data_ptr(), rj.data_ptr(),
             n, n, float(h), int(L), flags, stream_ptr(0))
    torch.cuda.synchronize()
    return (to_numpy(qo).astype(np.float64), to_numpy(po).astype(np.float64), to_numpy(ro).astype(np.float64),
            to_numpy(rj).astype(bool))


def _run(lib, pot, method, q0, m, h, L, S, flags, per_call=None, burn=0, pad=0):
    """pbbi_hmc_run of S iterations from q0 (fp64): `per_call` iterations per call, the first `burn` of them as a
    burn-in call that records nothing, q_state with `pad` extra columns of leading stride.  Returns samples,
    momenta, reject, ratio of the recorded iterations, the final q_state and its padding columns."""
    import torch
    from physicsbasedbayesianinference_amd._device import as_device, empty, stream_ptr, to_numpy
    D, n = q0.shape
    qd = torch.full((D, n + pad), 7.25, dtype=torch.float64, device="cuda")
    qd[:, :n] = as_device(q0, 0, np.float64)
    md = as_device(m, 0, np.float64) if m is not None else None
    R = S - burn
    samples, momenta = empty((R, D, n), np.float64, 0), empty((R, D, n), np.float64, 0)
    reject, ratio = empty((R, n), np.uint8, 0), empty((R, n), np.float64, 0)
    mp, st = md.data_ptr() if md is not None else None, stream_ptr(0)
    if burn:
        lib.call("pbbi_hmc_run", pot.handle, orc.METHODS[method], qd.data_ptr(), mp, None, None, None, None, n, n + pad,
                 h, L, burn, flags, SEED, ITER0, CHAIN0, 1.0, st)
    per_call = per_call or R
    for i in range(0, R, per_call):
        lib.call("pbbi_hmc_run", pot.handle, orc.METHODS[method], qd.data_ptr(), mp, samples[i].data_ptr(),
                 momenta[i].data_ptr(), reject[i].data_ptr(), ratio[i].data_ptr(), n, n + pad, h, L, min(per_call, R - i),
                 flags, SEED, ITER0 + burn + i, CHAIN0, 1.0, st)
    torch.cuda.synchronize()
    return (to_numpy(samples), to_numpy(momenta), to_numpy(reject).astype(bool), to_numpy(ratio),
            to_numpy(qd[:, :n].contiguous()), to_numpy(qd[:, n:].contiguous()))


def _clear(u, ratio, margin):
    """Chains whose decision is not within `margin` of a tie: |log u - log min(1, ratio)| > margin."""
    with np.errstate(divide="ignore"):
        return np.abs(np.log(u) - np.minimum(0.0, np.log(ratio))) > margin


# ---- (a) the GEMM path in fp64: D > 256 ---------------------------------------------------------------------------
# D = 257: rows padded to 384, the last 128-row tile has one valid row, the second block of the p^2 column sums
# (n_sq = ceil(D / 256) = 2, first met at this size) holds one row; 300: both ragged; 384: whole tiles, zero mean.
GEMM_D = [257, 300, 384]
GEMM_L, GEMM_S = 3, 5
GEMM_H = {"Leapfrog": 0.5, "Stormer-Verlet": 0.08}
# The reject rates of the five-iteration runs with masses, from the CPU oracle on these seeds and problems: Leapfrog
# 0.311 / 0.363 / 0.441 at D = 257 / 300 / 384, Stormer-Verlet 0.329 / 0.380 / 0.425; the smallest
# |log u - log min(1, ratio)| over all six is 4.5e-4, far from a tie at the 1e-8 the log ratios are held to.
# (Re-check both on the CPU when a seed or a shape changes.)
RUN_BAND = (0.15, 0.6)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("D", GEMM_D)
def test_gemm_fp64_hmc_iter_vs_oracle(P, lib, D, method):
    """pbbi_hmc_iter on kernels_big.hip in fp64 (run_hmc<double>: k_big_gemm<double, EPI_KDK, .>, k_big_sq_partial
    with two row blocks, k_big_decide, k_big_select), uploaded p and u, with and without masses, both values of
    PBBI_COMPAT_P_FROM_OLDQ: masks equal, q and p within the dense tolerance, log ratios within 1e-8.  A single
    iteration from the over-dispersed start rejects 31 % .. 75 % on the oracle (the nearest tie is 9e-4 away), so
    the band here only asks that dozens of chains take either branch; RUN_BAND applies to the runs below."""
    pot, op, mu = _problem(P, "dense", D)
    h, q0 = GEMM_H[method], _start(D, mu, 1.0)
    for mass in (False, True):
        m = MASS if mass else None
        p0, u = _draws(D, mass)
        for compat in (lib.COMPAT_P_FROM_OLDQ, 0):
            tag = f"D={D} {method} mass={mass} compat={compat}"
            assert "kernels_big" in route_of(lib, pot, N, GEMM_L, 1, compat, method), tag
            gq, gp, gratio, grej = _iter(lib, pot, method, q0, p0, u, m, h, GEMM_L, compat)
            q, p = q0.copy(), p0.copy()
            ratio, rej = orc.hmc_iter(op, method, q, p, u, m, h, GEMM_L, compat=compat)
            eq, ep = scaled_err(gq, q), scaled_err(gp, p)
            el = float(np.max(np.abs(np.log(gratio) - np.log(ratio))))
            print(f"{tag}: reject {grej.mean():.3f}, scaled error q {eq:.2e} p {ep:.2e}, log ratio {el:.2e}")
            assert np.array_equal(grej, rej), tag
            assert eq <= RTOL_DENSE and ep <= RTOL_DENSE, (tag, eq, ep)
            assert el < 1e-8, (tag, el)
            assert 0.15 <= rej.mean() <= 0.85, (tag, rej.mean())


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("D", GEMM_D)
def test_gemm_fp64_run_vs_oracle(P, lib, D, method):
    """pbbi_hmc_run, S = 5, PBBI_DRAW_F64, with masses, against oracle.hmc_run_philox: masks equal, samples and
    momenta within 1e-10 (what the suite gave this path's five-iteration run when F64_RUNS' dense-200 row still ran
    on it), q_state the last slab.  Leapfrog carries the gradient (k_big_first_kick and the kept x.g sums in
    iterations 1 .. 4), Stormer-Verlet forms it every iteration."""
    pot, op, mu = _problem(P, "dense", D)
    h, q0 = GEMM_H[method], _start(D, mu, 1.0)
    flags = lib.COMPAT_P_FROM_OLDQ | lib.DRAW_F64
    d = route_of(lib, pot, N, GEMM_L, GEMM_S, flags, method)
    assert "kernels_big" in d and ("carried between iterations: yes" in d) == (method == "Leapfrog"), d
    gs, gm, gr, _, gq, _ = _run(lib, pot, method, q0, MASS, h, GEMM_L, GEMM_S, flags)
    q = q0.copy()
    os_, om, orj, _ = orc.hmc_run_philox(op, method, q, MASS, h, GEMM_L, GEMM_S, SEED, ITER0, CHAIN0, 1.0,
                                        compat=orc.COMPAT_P_FROM_OLDQ | orc.DRAW_F64)
    es, em = scaled_err(gs, os_), scaled_err(gm, om)
    print(f"D={D} {method}: reject {gr.mean():.3f}, scaled error samples {es:.2e} momenta {em:.2e}")
    assert np.array_equal(gr, orj)
    assert es <= 1e-10 and em <= 1e-10, (es, em)
    assert np.array_equal(gq, gs[GEMM_S - 1])
    assert RUN_BAND[0] <= gr.mean() <= RUN_BAND[1], gr.mean()


@pytest.mark.parametrize("D", GEMM_D)
def test_gemm_fp64_run_identities_on_the_device(P, lib, D):
    """Bit equality on the device, Leapfrog, with masses: one run of 5 == 5 runs of 1 (iterations 1 .. 4 of the
    former start from k_big_first_kick and the kept x.g sums, every one of the latter from its own GEMM); a burn-in
    of 2 plus 3 recorded == the last 3 of the run of 5; the run whose q_state has leading stride N + 10 == the
    contiguous run, its ten padding columns unchanged."""
    pot, _, mu = _problem(P, "dense", D)
    h, q0 = GEMM_H["Leapfrog"], _start(D, mu, 1.0)
    flags = lib.COMPAT_P_FROM_OLDQ | lib.DRAW_F64
    for s, ldn in ((GEMM_S, N), (1, N), (2, N), (3, N), (GEMM_S, N + 10)):
        assert "kernels_big" in route_of(lib, pot, N, GEMM_L, s, flags, "Leapfrog", ldn=ldn), (s, ldn)
    one = _run(lib, pot, "Leapfrog", q0, MASS, h, GEMM_L, GEMM_S, flags)
    assert RUN_BAND[0] <= one[2].mean() <= RUN_BAND[1], one[2].mean()
    each = _run(lib, pot, "Leapfrog", q0, MASS, h, GEMM_L, GEMM_S, flags, per_call=1)
    for a, b in zip(one, each):
        assert np.array_equal(a, b)
    burnt = _run(lib, pot, "Leapfrog", q0, MASS, h, GEMM_L, GEMM_S, flags, burn=2)
    for a, b in zip(one[:4], burnt[:4]):
        assert np.array_equal(a[2:], b)
    assert np.array_equal(one[4], burnt[4])
    strided = _run(lib, pot, "Leapfrog", q0, MASS, h, GEMM_L, GEMM_S, flags, pad=10)
    for a, b in zip(one[:5], strided[:5]):
        assert np.array_equal(a, b)
    assert strided[5].shape == (D, 10) and np.all(strided[5] == 7.25)


# ---- (b) k_stream_hmc, fp64, separable: only D > 256 is left to it -----------------------------------------------
def test_stream_kdk_flag_changes_nothing(P, lib):
    """Diagonal Gaussian, D = 300: the workspace kernel has one operation order, so a run with PBBI_KDK_FMA (which
    HMC(rng="philox") sets by default) equals the run without it bit for bit, and both equal the oracle's."""
    D, h, L, S = 300, 0.1, 6, 5
    pot, op, _ = _problem(P, "diag", D)
    q0 = _start(D, np.zeros(D), 1.0)
    flags = lib.COMPAT_P_FROM_OLDQ | lib.DRAW_F64
    for f in (flags, flags | lib.KDK_FMA):
        assert "k_stream_hmc" in route_of(lib, pot, N, L, S, f, "Leapfrog"), f
    plain = _run(lib, pot, "Leapfrog", q0, MASS, h, L, S, flags)
    kdk = _run(lib, pot, "Leapfrog", q0, MASS, h, L, S, flags | lib.KDK_FMA)
    for a, b in zip(plain, kdk):
        assert np.array_equal(a, b)
    q = q0.copy()
    os_, om, orj, _ = orc.hmc_run_philox(op, "Leapfrog", q, MASS, h, L, S, SEED, ITER0, CHAIN0, 1.0,
                                        compat=orc.COMPAT_P_FROM_OLDQ | orc.DRAW_F64)
    assert np.array_equal(plain[2], orj) and np.array_equal(plain[0], os_) and np.array_equal(plain[1], om)


# ---- (c) k_stream_hmc in fp32 ---------------------------------------------------------------------------------------
def _r32(x):
    return np.ascontiguousarray(np.asarray(x).astype(np.float32).astype(np.float64))


def _fp32_inputs(kind, D):
    """float32-representable q, p, u (p scaled by sqrt(MASS); MASS is representable as it is)."""
    rs = np.random.RandomState(1000 + D)
    z = rs.standard_normal((D, N))
    q = _r32(1.0 + 0.1 * z) if kind == "rosenbrock" else _r32(z)
    return q, _r32(rs.standard_normal((D, N)) * np.sqrt(MASS)), _r32(rs.uniform(size=N))


def _fma32(a, b, c):
    """fma in float32: the product of two float32 is exact in float64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _rosenbrock_accel32(q, m, a=1.0, b=100.0, s=20.0):
    """-gradient / mass with every array float32: the oracle's Rosenbrock gradient (pbbi_oracle.c pot_grad: constants
    pre-combined in double, t_i = fma(-q_i, q_i, q_{i+1}), g_i += fma(c1 q_i, t_i, -(c2 (a - q_i))), g_{i+1} += c3 t_i)."""
    f = np.float32
    inv_s = 1.0 / s
    c1, c2, c3 = f((-4.0 * b) * inv_s), f(2.0 * inv_s), f((2.0 * b) * inv_s)
    t = _fma32(-q[:-1], q[:-1], q[1:])
    g = np.zeros_like(q)
    g[1:] = c3 * t
    g[:-1] += _fma32(c1 * q[:-1], t, -(c2 * (f(a) - q[:-1])))
    return -g / m


def rosenbrock_proposal32(method, q, p, m, h, L):
    """The reference's Leapfrog / Stormer-Verlet recurrences (restated in pbbi_oracle.c leapfrog_chain /
    stormer_verlet_chain) on the Rosenbrock potential in NumPy with every array float32.  Returns q_L, p_L."""
    f = np.float32
    q, p, m, h = q.astype(f), p.astype(f), m.astype(f), f(h)
    h2 = h * h
    v = p / m
    if method == "Leapfrog":
        acc = _rosenbrock_accel32(q, m)
        for _ in range(L):
            q = q + (v * h + (f(0.5) * acc) * h2)
            nxt = _rosenbrock_accel32(q, m)
            v = v + (f(0.5) * (acc + nxt)) * h
            acc = nxt
    else:
        past = q
        q = (q + v * h) + (f(0.5) * _rosenbrock_accel32(q, m)) * h2
        for _ in range(L):
            q, past = (f(2) * q - past) + _rosenbrock_accel32(q, m) * h2, q
        v = (q - past) / h
    assert q.dtype == f and v.dtype == f
    return q.astype(np.float64), (v * m).astype(np.float64)


# (D, method) -> scaled distance (q, p) of rosenbrock_proposal32 from the fp64 oracle on _fp32_inputs, h = 0.01,
# L = 5, measured on the CPU.  The test's tolerance is 4 x these (see its docstring).
ROSENBROCK_FP32_BASELINE = {
    (20, "Leapfrog"): (1.897e-07, 1.072e-07), (20, "Stormer-Verlet"): (9.169e-07, 1.081e-05),
    (80, "Leapfrog"): (1.933e-07, 1.845e-07), (80, "Stormer-Verlet"): (9.525e-07, 1.002e-05),
}


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("kind,D", [("harmonic", 20), ("harmonic", 80), ("diag", 80), ("rosenbrock", 20), ("rosenbrock", 80)])
def test_stream_fp32_hmc_iter_vs_fp64_oracle(P, lib, kind, D, method):
    """k_stream_hmc<float> (every chain-per-lane potential in fp32, at any D), pbbi_hmc_iter with uploaded
    float32-representable q, p, u, with masses, against the fp64 oracle: decisions equal wherever
    |log u - log min(1, ratio)| > 1e-2 (more than half the chains are that clear), state compared on the chains
    that agree.  Harmonic / diagonal (h = 0.5, L = 5: 1 % .. 73 % rejections on the oracle): 3e-5 scaled, the
    suite's value for this kernel (F64_RUNS stream_diag12_f32).

    Rosenbrock (start 1 + 0.1 z, h = 0.01, L = 5): the tolerance comes from the reference's own single-precision
    error, not from the kernel.  rosenbrock_proposal32 restates the trajectory in NumPy float32; its scaled distance
    from the fp64 oracle on these inputs is the baseline (recomputed here and checked against the table):
        D = 20  Leapfrog        q 1.897e-07  p 1.072e-07        D = 20  Stormer-Verlet  q 9.169e-07  p 1.081e-05
        D = 80  Leapfrog        q 1.933e-07  p 1.845e-07        D = 80  Stormer-Verlet  q 9.525e-07  p 1.002e-05
    (Stormer-Verlet's momentum is a backward difference divided by h = 0.01, which amplifies the rounding of q a
    hundredfold.)  The kernel may fuse multiply-adds and take a reciprocal where NumPy divides, a few ulp per
    operation, so the tolerance is 4 x the baseline of the case: q 7.6e-07 / 3.7e-06 / 7.7e-07 / 3.8e-06 and
    p 4.3e-07 / 4.3e-05 / 7.4e-07 / 4.0e-05 in the order above."""
    pot, op, _ = _problem(P, kind, D, "float32")
    ros = kind == "rosenbrock"
    h, L = (0.01, 5) if ros else (0.5, 5)
    q0, p0, u = _fp32_inputs(kind, D)
    assert "k_stream_hmc" in route_of(lib, pot, N, L, 1, lib.COMPAT_P_FROM_OLDQ, method)
    q, p = q0.copy(), p0.copy()
    ratio, rej = orc.hmc_iter(op, method, q, p, u, MASS, h, L)
    if ros:
        q32, p32 = rosenbrock_proposal32(method, q0, p0, MASS, h, L)
        base = (scaled_err(np.where(rej, q0, q32), q), scaled_err(np.where(rej, q0, p32), p))
        print(f"{kind} D={D} {method}: float32 restatement vs fp64 oracle: q {base[0]:.3e} p {base[1]:.3e}")
        assert np.allclose(base, ROSENBROCK_FP32_BASELINE[(D, method)], rtol=2e-3, atol=0), base
        tol_q, tol_p = (4.0 * b for b in ROSENBROCK_FP32_BASELINE[(D, method)])
    else:
        tol_q = tol_p = 3e-5
    gq, gp, _, grej = _iter(lib, pot, method, q0, p0, u, MASS, h, L, lib.COMPAT_P_FROM_OLDQ, np.float32)
    clear = _clear(u, ratio, 1e-2)
    same = grej == rej
    eq, ep = scaled_err(gq[:, same], q[:, same]), scaled_err(gp[:, same], p[:, same])
    print(f"{kind} D={D} {method}: reject {grej.mean():.3f}, clear {clear.mean():.3f}, agree {same.mean():.3f}, "
          f"scaled error q {eq:.3e} (tolerance {tol_q:.1e}) p {ep:.3e} (tolerance {tol_p:.1e})")
    assert clear.sum() > N // 2
    assert np.array_equal(grej[clear], rej[clear])
    assert eq <= tol_q and ep <= tol_p, (eq, tol_q, ep, tol_p)


# ---- (d) k_lane_hmc: Rosenbrock, Stormer-Verlet, reference order ------------------------------------------------
# D = 12 (DMAX 16), 24 (DMAX 32), 48 and 64 (DMAX 64, ragged and full).  Separable 17 .. 64 went to k_sep_exact_hmc
# and Rosenbrock with Leapfrog to k_ros2_hmc / k_rosg_exact_hmc, so this is all that still reaches DMAX 32 / 64.
LANE_D = [12, 24, 48, 64]
LANE_H, LANE_L, LANE_S = 0.02, 6, 5


@pytest.mark.parametrize("D", LANE_D)
def test_lane_rosenbrock_stormer_verlet_hmc_iter_bitexact(P, lib, D):
    """pbbi_hmc_iter, with and without masses, both values of PBBI_COMPAT_P_FROM_OLDQ: bit for bit the oracle's
    q, p and masks (12 % .. 45 % rejections on the oracle)."""
    pot, op, one = _problem(P, "rosenbrock", D)
    q0 = _start(D, one, 0.1)
    for mass in (False, True):
        m = MASS if mass else None
        p0, u = _draws(D, mass)
        for compat in (lib.COMPAT_P_FROM_OLDQ, 0):
            tag = f"D={D} mass={mass} compat={compat}"
            assert "k_lane_hmc" in route_of(lib, pot, N, LANE_L, 1, compat, "Stormer-Verlet"), tag
            gq, gp, gratio, grej = _iter(lib, pot, "Stormer-Verlet", q0, p0, u, m, LANE_H, LANE_L, compat)
            q, p = q0.copy(), p0.copy()
            ratio, rej = orc.hmc_iter(op, "Stormer-Verlet", q, p, u, m, LANE_H, LANE_L, compat=compat)
            assert np.array_equal(grej, rej), tag
            assert np.array_equal(gq, q) and np.array_equal(gp, p), tag
            assert np.max(np.abs(np.log(gratio) - np.log(ratio))) < 1e-8, tag
            assert 0.05 < rej.mean() < 0.6, (tag, rej.mean())


@pytest.mark.parametrize("mass", [False, True])
@pytest.mark.parametrize("D", LANE_D)
def test_lane_rosenbrock_stormer_verlet_run_bitexact(P, lib, D, mass):
    """pbbi_hmc_run, S = 5, PBBI_DRAW_F64, bit for bit oracle.hmc_run_philox (which rejects 10 % / 19 % / 32 % /
    40 % at D = 12 / 24 / 48 / 64 without masses and stays finite); one run of 5 == 5 runs of 1."""
    pot, op, one = _problem(P, "rosenbrock", D)
    q0, m = _start(D, one, 0.1), (MASS if mass else None)
    flags = lib.COMPAT_P_FROM_OLDQ | lib.DRAW_F64
    for s in (LANE_S, 1):
        assert "k_lane_hmc" in route_of(lib, pot, N, LANE_L, s, flags, "Stormer-Verlet"), s
    run = _run(lib, pot, "Stormer-Verlet", q0, m, LANE_H, LANE_L, LANE_S, flags)
    q = q0.copy()
    os_, om, orj, _ = orc.hmc_run_philox(op, "Stormer-Verlet", q, m, LANE_H, LANE_L, LANE_S, SEED, ITER0, CHAIN0, 1.0,
                                        compat=orc.COMPAT_P_FROM_OLDQ | orc.DRAW_F64)
    assert np.array_equal(run[2], orj)
    assert np.array_equal(run[0], os_) and np.array_equal(run[1], om)
    assert np.array_equal(run[4], run[0][LANE_S - 1])
    assert np.isfinite(os_).all() and np.isfinite(om).all()
    assert 0.05 < orj.mean() < 0.6, orj.mean()
    each = _run(lib, pot, "Stormer-Verlet", q0, m, LANE_H, LANE_L, LANE_S, flags, per_call=1)
    for a, b in zip(run, each):
        assert np.array_equal(a, b)


# ---- the census's witnesses for the tests that carry no route assertion of their own ---------------------------
CENSUS = [
    # family, (kind, D) of the named test's potential, method, flags beyond compat, the test
    ("k_ros2_hmc: Rosenbrock 16 < D <= 32, two lanes per chain, reference", ("rosenbrock", 17), "Leapfrog", "",
     "test_rosenbrock_two_lane_kernel_bitexact"),
    ("k_sep_hmc:", ("harmonic", 17), "Stormer-Verlet", "kdk", "test_separable_multilane_kdk"),
    ("k_sep_exact_hmc", ("diag", 17), "Stormer-Verlet", "", "test_separable_multiwave_reference_order_bitexact"),
    ("k_rosg_hmc:", ("rosenbrock", 20), "Stormer-Verlet", "kdk", "test_rosenbrock_kdk_stormer_verlet"),
    ("k_rosg_hmc:", ("rosenbrock", 100), "Stormer-Verlet", "kdk", "test_rosenbrock_kdk_stormer_verlet"),
    ("k_lane_dyn_hmc", ("diag", 5), "Leapfrog", "steps", "test_per_chain_steps_lane_kernels_bitexact"),
    ("k_lane_dyn_hmc", ("rosenbrock", 12), "Leapfrog", "uturn", "test_per_chain_steps_lane_kernels_bitexact"),
    ("k_ros2_hmc<DYN>", ("rosenbrock", 20), "Leapfrog", "steps", "test_per_chain_steps_lane_kernels_bitexact"),
    ("k_sep_hmc<DYN>", ("diag", 40), "Leapfrog", "steps kdk", "test_per_chain_steps_multilane_kdk_kernels"),
    ("k_rosg_hmc<DYN>", ("rosenbrock", 64), "Leapfrog", "steps kdk", "test_per_chain_steps_multilane_kdk_kernels"),
    ("k_rosg_hmc<DYN>", ("rosenbrock", 128), "Leapfrog", "steps kdk", "test_per_chain_steps_multilane_kdk_kernels"),
]


@pytest.mark.parametrize("family,problem,method,extra,test", CENSUS, ids=[f"{r[4]}-{r[1][0]}{r[1][1]}" for r in CENSUS])
def test_census_witnesses(P, lib, family, problem, method, extra, test):
    """The tests the census names without a route assertion of their own sit on the family it says (nothing is
    launched: the shapes are theirs, at the edge of the family's range)."""
    pot, _, _ = _problem(P, *problem)
    flags = lib.COMPAT_P_FROM_OLDQ | (lib.KDK_FMA if "kdk" in extra else 0) | \
        (lib.PER_CHAIN_STEPS if "steps" in extra else 0) | (lib.UTURN_STOP if "uturn" in extra else 0)
    assert family in route_of(lib, pot, 333, 9, 1, flags, method), test
