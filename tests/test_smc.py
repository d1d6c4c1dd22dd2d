"""Tempered SMC (smc.py, csrc/kernels_smc.hip).

CPU: argument validation, the ABI table, and a NumPy restatement of the fixed-point systematic resampler (its
offspring counts obey floor(N W_n) <= o_n <= ceil(N W_n) on the tick weights).
GPU: every kernel against the NumPy restatement written here (resample bit for bit from the device's ticks; ESS scan
and reweight to 1e-13; next_beta within the bracket), a whole run replayed on the CPU oracle, and the log-evidence of
four targets whose normalising constant is known.
"""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMC_SYMBOLS = ["pbbi_smc_ess_scan", "pbbi_smc_next_beta", "pbbi_smc_reweight", "pbbi_smc_resample_systematic"]


# ---------------------------------------------------------------- NumPy restatement of the resampler
def np_ticks(logw):
    lw = np.asarray(logw, dtype=np.float64)
    fin = np.isfinite(lw)
    out = np.zeros(lw.shape, dtype=np.uint64)
    if fin.any():
        m = lw[fin].max()
        out[fin] = np.floor(np.exp(lw[fin] - m) * 2.0 ** 32).astype(np.uint64)
    return out


def stage_k(seed, stage):
    """The 53-bit integer of the stage uniform: block 0xFFFFFFFF of PBBI_STREAM_RESAMPLE (5), iter = stage, chain 0."""
    from oracle import oracle as orc
    x = orc.philox_raw([0, 0xFFFFFFFF, stage & 0xFFFFFFFF, 5], [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
    return ((x[1] << 32) | x[0]) >> 11


def np_ancestors(ticks, k):
    """a_j = the smallest n with C_n > floor((j T + floor(k T / 2^53)) / N), exactly (uint64 throughout)."""
    ticks = np.asarray(ticks, dtype=np.uint64)
    N = ticks.size
    C = np.cumsum(ticks, dtype=np.uint64)
    T = int(C[-1])
    assert T > 0
    uT = (int(k) * T) >> 53
    a, b = T // N, T % N                                  # j T + uT = j a N + (j b + uT)
    j = np.arange(N, dtype=np.uint64)
    pos = j * np.uint64(a) + (j * np.uint64(b) + np.uint64(uT)) // np.uint64(N)
    return np.searchsorted(C, pos, side="right").astype(np.int64)


def weight_cases(N, rng):
    lw = rng.standard_normal(N)
    one = np.full(N, -np.inf)
    one[rng.integers(N)] = 0.0
    spread = rng.uniform(-1e3, 0.0, N)
    holes = rng.standard_normal(N) * 3.0
    holes[rng.random(N) < 0.2] = -np.inf
    holes[rng.random(N) < 0.1] = np.nan
    peaked = rng.standard_normal(N) * 40.0
    return {"uniform": np.zeros(N), "random": lw, "one_hot": one, "spread1e3": spread, "holes": holes,
            "peaked": peaked}


# ---------------------------------------------------------------- CPU
def test_smc_symbols_in_table_and_exported():
    from physicsbasedbayesianinference_amd import _lib
    for name in SMC_SYMBOLS:
        assert name in _lib.PROTOTYPES, name
    hdr = open(os.path.join(ROOT, "include", "pbbi.h")).read()
    assert all(name + "(" in hdr for name in SMC_SYMBOLS)
    assert re.search(r"PBBI_STREAM_RESAMPLE\s*=\s*5", hdr) and _lib.STREAM_RESAMPLE == 5
    _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (pbbi_[a-z0-9_]+)", out))
    assert set(SMC_SYMBOLS) <= exported


@pytest.mark.parametrize("kw", [dict(target_ess=0.0), dict(target_ess=1.0), dict(target_ess=1.5), dict(qStd=0.0),
                                dict(qStd=-1.0), dict(moves=0), dict(betas=[0.5, 0.2, 1.0]), dict(betas=[0.1, 0.5]),
                                dict(betas=[0.0, 1.0]), dict(betas=[0.3, 0.3, 1.0]), dict(resample_threshold=1.5),
                                dict(method="rk4"), dict(qMean=[0.0, 1.0])])
def test_tempered_smc_rejects_bad_arguments(kw):
    from physicsbasedbayesianinference_amd.smc import TemperedSMC
    args = dict(simulTime=1.0, stepSize=0.1, qStd=2.0)
    args.update(kw)
    with pytest.raises(ValueError):
        TemperedSMC(None, 3, 100, **args)


@pytest.mark.parametrize("N", [1, 5, 1000, 65531])
def test_fixed_point_systematic_offspring_bounds(N):
    rng = np.random.default_rng(N)
    for name, lw in weight_cases(N, rng).items():
        ticks = np_ticks(lw)
        if ticks.sum() == 0:
            continue
        for stage in (0, 7):
            a = np_ancestors(ticks, stage_k(11, stage))
            assert np.all(np.diff(a) >= 0) and a.min() >= 0 and a.max() < N
            o = np.bincount(a, minlength=N)
            assert np.all(o[ticks == 0] == 0), name
            NW = [(N * int(t), int(ticks.sum())) for t in ticks]       # N W_n as an exact fraction
            lo = np.array([n // d for n, d in NW])
            hi = np.array([-(-n // d) for n, d in NW])
            assert np.all(lo <= o) and np.all(o <= hi), name


# ---------------------------------------------------------------- GPU
def _dev(arr, dtype=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=dtype)).to("cuda:0")


def _st():
    from physicsbasedbayesianinference_amd._device import stream_ptr
    return stream_ptr(0)


def _resample(lib, lw, q, stage, seed=3, dt=None):
    import torch
    N = lw.size
    D = q.shape[0]
    dt = dt or (lib.F64 if q.dtype == np.float64 else lib.F32)
    lwd = _dev(lw)
    qi, qo = _dev(q, q.dtype), torch.empty(q.shape, dtype=torch.float64 if q.dtype == np.float64 else torch.float32,
                                           device="cuda:0")
    anc = torch.empty(N, dtype=torch.int32, device="cuda:0")
    ticks = torch.empty(N, dtype=torch.int64, device="cuda:0")
    rs = torch.zeros(1, dtype=torch.uint8, device="cuda:0")
    lib.call("pbbi_smc_resample_systematic", lwd.data_ptr(), N, seed, stage, qi.data_ptr(), qo.data_ptr(), N, D, None,
             1.0, anc.data_ptr(), ticks.data_ptr(), rs.data_ptr(), None, dt, 0, _st())
    return (anc.cpu().numpy().astype(np.int64), ticks.cpu().numpy().view(np.uint64), qo.cpu().numpy(),
            lwd.cpu().numpy(), int(rs.item()))


@pytest.fixture(scope="module")
def lib():
    from physicsbasedbayesianinference_amd import _lib
    _lib.load()
    return _lib


@pytest.mark.gpu
@pytest.mark.parametrize("N,D", [(1, 8), (5, 1), (1000, 128), (65536, 8), (65531, 200), (2 ** 20 + 3, 1)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_resample_matches_numpy_restatement(lib, N, D, dtype):
    rng = np.random.default_rng(N + D)
    q = rng.standard_normal((D, N)).astype(dtype)
    for i, (name, lw) in enumerate(weight_cases(N, rng).items()):
        if np_ticks(lw).sum() == 0:
            continue
        if N > 70000 and name not in ("one_hot", "holes", "spread1e3"):
            continue
        anc, ticks, qo, lw_after, rs = _resample(lib, lw, q, stage=i)
        ref_t = np_ticks(lw)
        diff = np.abs(ticks.astype(np.int64) - ref_t.astype(np.int64))
        assert diff.max() <= 1, name
        a_ref = np_ancestors(ticks, stage_k(3, i))
        assert np.array_equal(anc, a_ref), name
        assert np.array_equal(qo, q[:, a_ref]), name
        assert rs == 1 and np.all(lw_after == 0.0)


@pytest.mark.gpu
def test_resample_rejects_all_zero_weights(lib):
    lw = np.full(100, -np.inf)
    lw[3] = np.nan
    with pytest.raises(lib.PbbiError):
        _resample(lib, lw, np.zeros((2, 100)), 0)


@pytest.mark.gpu
def test_resample_keeps_state_when_ess_is_high(lib):
    import torch
    N, D = 777, 3
    q = np.random.default_rng(0).standard_normal((D, N))
    lw = _dev(np.random.default_rng(1).standard_normal(N) * 0.1)
    qi, qo = _dev(q), torch.empty((D, N), dtype=torch.float64, device="cuda:0")
    ess = _dev([0.9])
    anc = torch.empty(N, dtype=torch.int32, device="cuda:0")
    rs = torch.ones(1, dtype=torch.uint8, device="cuda:0")
    before = lw.cpu().numpy()
    lib.call("pbbi_smc_resample_systematic", lw.data_ptr(), N, 1, 0, qi.data_ptr(), qo.data_ptr(), N, D, ess.data_ptr(),
             0.5, anc.data_ptr(), None, rs.data_ptr(), None, lib.F64, 0, _st())
    assert int(rs.item()) == 0 and np.array_equal(anc.cpu().numpy(), np.arange(N))
    assert np.array_equal(qo.cpu().numpy(), q) and np.array_equal(lw.cpu().numpy(), before)


def np_lse(x):
    x = x[np.isfinite(x)]
    if x.size == 0:
        return -np.inf
    m = x.max()
    return m + np.log(np.sum(np.exp(x - m)))


def np_ref_term(q, mean, sigma):
    D = q.shape[0]
    acc = np.zeros(q.shape[1])
    for d in range(D):
        x = q[d] - mean[d]
        acc = acc + x * x
    return acc * (1.0 / (2.0 * sigma * sigma)) + 0.5 * D * np.log(2.0 * np.pi * sigma * sigma)


def np_scan(U, logw, r, c):
    l = r - c * U
    a, b = logw + l, logw + 2.0 * l
    ln = np_lse(logw)
    la, lb = np_lse(a) - ln, np_lse(b) - ln
    return la, lb, np.exp(2 * la - lb)


def rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ess_scan_and_reweight_match_logsumexp(lib, dtype):
    import torch
    rng = np.random.default_rng(5)
    D, N, sigma = 6, 70001, 2.5
    q = rng.standard_normal((D, N)).astype(dtype) * 2
    U = (0.5 * (q.astype(np.float64) ** 2).sum(0) + rng.standard_normal(N)).astype(dtype)
    U[7] = np.nan
    logw = rng.standard_normal(N) * 2.0
    logw[11] = -np.inf
    mean = rng.standard_normal(D)
    coefs = np.geomspace(1e-6, 3.0, 70)
    dt = lib.F64 if dtype == np.float64 else lib.F32
    Ud, qd, lwd, md, cd = _dev(U, dtype), _dev(q, dtype), _dev(logw), _dev(mean), _dev(coefs)
    K = coefs.size
    for with_q in (False, True):
        out = torch.empty(3 * K + 1, dtype=torch.float64, device="cuda:0")
        lib.call("pbbi_smc_ess_scan", Ud.data_ptr(), lwd.data_ptr(), qd.data_ptr() if with_q else None, md.data_ptr(),
                 sigma, N, N, D, K, cd.data_ptr(), dt, 0, out.data_ptr(), _st())
        o = out.cpu().numpy()
        r = np_ref_term(q.astype(np.float64), mean, sigma) if with_q else np.zeros(N)
        Uf = U.astype(np.float64)
        assert rel(o[3 * K], np_lse(logw)) < 1e-13
        for k in range(K):
            la, lb, ess = np_scan(Uf, logw, r, coefs[k])
            assert rel(o[3 * k], la) < 1e-13 and rel(o[3 * k + 1], lb) < 1e-13, k
            assert abs(o[3 * k + 2] - ess) < 1e-12 * max(ess, 1e-300) + 1e-300, k
        # reweight with c = betas[1] - betas[0]
        betas = _dev([0.25, 0.25 + 0.01])
        lw2 = _dev(logw)
        logz = _dev([1.5])
        so = torch.zeros(2, dtype=torch.float64, device="cuda:0")
        lib.call("pbbi_smc_reweight", Ud.data_ptr(), qd.data_ptr() if with_q else None, md.data_ptr(), sigma, N, N, D,
                 betas.data_ptr(), lw2.data_ptr(), logz.data_ptr(), so.data_ptr(), dt, 0, _st())
        c = (0.25 + 0.01) - 0.25
        new = logw + (r - c * Uf)
        new[~np.isfinite(new)] = -np.inf
        got = lw2.cpu().numpy()
        assert np.array_equal(np.isfinite(got), np.isfinite(new))
        fin = np.isfinite(new)
        assert np.array_equal(got[fin], new[fin])
        dz = np_lse(new) - np_lse(logw)
        ess = np.exp(2 * np_lse(new) - np_lse(2 * new)) / N
        s = so.cpu().numpy()
        assert rel(s[0], dz) < 1e-13 and abs(s[1] - ess) < 1e-12
        assert rel(float(logz.item()), 1.5 + dz) < 1e-13


def np_cess(U, logw, dbeta):
    return np_scan(U, logw, np.zeros_like(U), dbeta)[2]


@pytest.mark.gpu
def test_next_beta_matches_numpy_bisection_and_clamps(lib):
    import torch
    rng = np.random.default_rng(9)
    N = 50000
    U = rng.standard_normal(N) * 30 + 100.0
    logw = rng.standard_normal(N) * 0.3
    Ud, lwd = _dev(U), _dev(logw)
    for beta0, rho in ((0.0, 0.5), (0.37, 0.5), (0.6, 0.9), (0.1, 0.2)):
        betas = _dev([beta0, -1.0])
        info = torch.zeros(2, dtype=torch.float64, device="cuda:0")
        lib.call("pbbi_smc_next_beta", Ud.data_ptr(), lwd.data_ptr(), None, None, 1.0, N, N, 1, rho, betas.data_ptr(),
                 info.data_ptr(), lib.F64, 0, _st())
        got = betas.cpu().numpy()[1]
        lo, hi = 0.0, 1.0 - beta0
        if np_cess(U, logw, hi) >= rho:
            assert got == 1.0
            continue
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if np_cess(U, logw, mid) >= rho:
                lo = mid
            else:
                hi = mid
        assert abs((got - beta0) - lo) < 1e-10, (beta0, rho, got - beta0, lo)
        assert info.cpu().numpy()[1] < 1e-10
    # nothing left to choose: an almost flat U takes the whole way to 1 exactly
    Uf = _dev(np.full(N, 3.0) + rng.standard_normal(N) * 1e-9)
    betas = _dev([0.3, -1.0])
    lib.call("pbbi_smc_next_beta", Uf.data_ptr(), lwd.data_ptr(), None, None, 1.0, N, N, 1, 0.5, betas.data_ptr(),
             None, lib.F64, 0, _st())
    assert betas.cpu().numpy()[1] == 1.0


@pytest.mark.gpu
def test_whole_run_replays_on_the_oracle(lib):
    """D = 4 diagonal Gaussian, N = 1000, reference operation order and double-precision draws: the CPU oracle with
    the recorded betas, kT = 1/beta and BETA_ACCEPT, plus this file's reweight / resample, gives the same ancestors,
    the same final q bit for bit and log Z to 1e-12."""
    import physicsbasedbayesianinference_amd as P
    from oracle import oracle as orc
    from physicsbasedbayesianinference_amd.smc import TemperedSMC
    D, N, seed, qStd, h, T, moves = 4, 1000, 21, 4.0, 0.2, 1.0, 3
    mu, prec = np.array([0.5, -1.0, 0.0, 2.0]), np.array([1.0, 2.0, 0.5, 4.0])
    pot = P.GaussianDiag(mu, prec=prec, const=0.0)
    smc = TemperedSMC(pot, D, N, T, h, qStd, moves=moves, target_ess=0.3, seed=seed, kdk_fma=False, draw_f64=True,
                      record_ancestors=True)
    qdev = smc.run()
    betas = smc.betas
    assert 3 <= betas.size <= 12 and betas[-1] == 1.0
    # the initial draw, as run() makes it
    import torch
    q0 = torch.empty((D, N), dtype=torch.float64, device="cuda:0")
    lib.call("pbbi_philox_normal", seed, lib.STREAM_POSITION | lib.STREAM_DRAW_F64, 0, 0, D, N, N, qStd, None,
             lib.F64, 0, q0.data_ptr(), _st())
    q = q0.cpu().numpy().copy()
    opot = orc.pot_gauss_diag(mu, prec)
    logw, logz, b_old = np.zeros(N), 0.0, 0.0
    L = max(1, int(T / h))
    for t, beta in enumerate(betas):
        U = orc.potential(opot, q)
        r =np_ref_term(q, np.zeros(D), qStd) if t == 0 else np.zeros(N)
        c = beta - b_old
        new = logw + (r - c * U)
        logz += np_lse(new) - np_lse(logw)
        logw = new
        ess = np.exp(2 * np_lse(logw) - np_lse(2 * logw)) / N
        if ess < 0.5:
            a = np_ancestors(np_ticks(logw), stage_k(seed, t))
            q = q[:, a].copy()
            logw = np.zeros(N)
        else:
            a = np.arange(N)
        assert np.array_equal(smc.ancestors[t].cpu().numpy(), a), t
        orc.hmc_run_philox(opot, "Leapfrog", q, None, h, L, moves, seed, iter0=t * moves, chain0=0, kT=1.0 / beta,
                           compat=lib.BETA_ACCEPT | lib.DRAW_F64, want_momenta=False)
        b_old = beta
    a = np_ancestors(np_ticks(logw), stage_k(seed, betas.size))
    assert np.array_equal(smc.ancestors[-1].cpu().numpy(), a)
    q = q[:, a]
    assert np.array_equal(qdev, q)
    assert abs(smc.logZ - logz) < 1e-12
    assert smc.host_syncs == betas.size


def _mixture():
    from physicsbasedbayesianinference_amd import trace as jnp
    a, b, sig, wa = np.array([-4.0, 0.0]), np.array([4.0, 0.0]), 0.6, 0.7

    def potential(q):
        la = np.log(wa) - 0.5 * jnp.sum((q - a) ** 2) / sig ** 2
        lb = np.log(1.0 - wa) - 0.5 * jnp.sum((q - b) ** 2) / sig ** 2
        return -jnp.logaddexp(la, lb)
    return potential


@pytest.mark.gpu
@pytest.mark.parametrize("target", ["dense8", "dense128", "rosenbrock", "mixture"])
def test_log_evidence_of_known_targets(target):
    import physicsbasedbayesianinference_amd as P
    from physicsbasedbayesianinference_amd.smc import TemperedSMC
    if target == "dense8":
        A = np.random.RandomState(1).standard_normal((8, 8))
        pot, D, N, kw, truth = P.GaussianDense(None, cov=A @ A.T / 8 + 0.5 * np.eye(8)), 8, 4096, \
            dict(simulTime=1.0, stepSize=0.2, qStd=4.0), 0.0
    elif target == "dense128":
        # the MFMA kernel at C2's size, with a covariance an isotropic reference can cover: C2's own Sigma (eigenvalues
        # 1 .. 4.8) leaves an exact stage-1 log ESS of at most -15 for ANY reference N(0, s I)
        A = np.random.RandomState(0).standard_normal((128, 128))
        pot, D, N, kw, truth = P.GaussianDense(None, cov=np.eye(128) + 0.1 * A @ A.T / 128), 128, 65536, \
            dict(simulTime=1.0, stepSize=0.1, qStd=1.2), 0.0
    elif target == "rosenbrock":
        # chain-per-lane family.  h sqrt(lambda_max) < 2 over the hot stages' support (lambda ~ 40 x^2 along the
        # ridge, |x| up to ~ 100): h = 0.002.  The stage-1 warning is expected here
        pot, D, N, kw, truth = P.Rosenbrock(2, 1.0, 100.0, 20.0), 2, 16384, \
            dict(simulTime=0.2, stepSize=0.002, qStd=25.0, qMean=[1.0, 10.0]), np.log(2 * np.pi)
        # the documented limit: no Gaussian reference covers the target's exponential tail along the ridge, so the
        # stage-1 weights have unbounded variance and the search warns (the evidence scatters by ~1.7 over seeds)
    else:
        pot, D, N, kw, truth = _mixture(), 2, 16384, dict(simulTime=1.0, stepSize=0.1, qStd=8.0), \
            np.log(2 * np.pi * 0.6 ** 2)
    zs, lefts = [], []
    for seed in range(8):
        smc = TemperedSMC(pot, D, N, seed=seed, **kw)
        q = smc.run()
        assert smc.betas[-1] == 1.0 and np.all(np.diff(smc.betas) > 0)
        zs.append(smc.logZ)
        if target == "rosenbrock":
            assert smc.warnings and "stage 1" in smc.warnings[0]
        if target == "mixture":
            assert not smc.warnings
            lefts.append((q[0] < 0).mean())
    zs = np.array(zs)
    print(target, zs.mean() - truth, zs.std(ddof=1), smc.betas.size)
    assert abs(zs.mean() - truth) < 3 * zs.std(ddof=1) / np.sqrt(8) + 0.01, (zs, truth)
    if target == "mixture":
        assert abs(np.mean(lefts) - 0.7) < 0.03, lefts


def _count_syncs(monkeypatch, smc):
    """Run smc with torch's synchronisation detector on around the stage loop; returns the syncs it reported."""
    import warnings
    import torch
    from physicsbasedbayesianinference_amd.smc import TemperedSMC
    inner = TemperedSMC._stages

    def watched(self, *a, **k):
        torch.cuda.set_sync_debug_mode("warn")
        try:
            return inner(self, *a, **k)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    monkeypatch.setattr(TemperedSMC, "_stages", watched)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        q = smc.run()
    hits = [f"{x.filename}:{x.lineno}: {x.message}" for x in w if "called a synchronizing" in str(x.message)]
    return q, hits


@pytest.mark.gpu
def test_host_syncs_per_stage(monkeypatch):
    """A fixed schedule runs its stage loop without one device synchronisation; the adaptive schedule has exactly
    one per stage (the read of the next beta)."""
    import physicsbasedbayesianinference_amd as P
    from physicsbasedbayesianinference_amd.smc import TemperedSMC
    smc = TemperedSMC(P.StandardGaussian(3), 3, 4096, 1.0, 0.2, qStd=3.0, betas=np.geomspace(0.15, 1.0, 8))
    q, n_fixed = _count_syncs(monkeypatch, smc)
    assert q.shape == (3, 4096) and n_fixed == [], n_fixed
    assert np.array_equal(smc.betas, np.geomspace(0.15, 1.0, 8))
    # Z of exp(-|q|^2 / 2) over R^3 is (2 pi)^(3/2)
    assert abs(smc.logZ - 1.5 * np.log(2 * np.pi)) < 0.1
    smc = TemperedSMC(P.StandardGaussian(3), 3, 4096, 1.0, 0.2, qStd=3.0)
    _, n_adaptive = _count_syncs(monkeypatch, smc)
    assert smc.nstages >= 2 and len(n_adaptive) == smc.nstages, n_adaptive


@pytest.mark.gpu
def test_next_beta_stage1_matches_numpy_restatement(lib):
    """Stage 1 (q given): the reference term, the log grid, the search from its maximiser, and the warning when even
    the best beta is below the target -- against a NumPy restatement."""
    import torch
    rng = np.random.default_rng(17)
    N = 50000
    for D, prec, sigma, rho in ((3, np.array([1.0, 1.5, 2.0]), 2.0, 0.5), (3, np.array([1.0, 1.5, 2.0]), 2.0, 0.3),
                                (20, np.linspace(1.0, 20.0, 20), 2.0, 0.5)):
        m = rng.standard_normal(D) * 0.3
        mu = rng.standard_normal(D) * 0.2
        q = m[:, None] + sigma * rng.standard_normal((D, N))
        U = 0.5 * (prec[:, None] * (q - mu[:, None]) ** 2).sum(0)
        r = np_ref_term(q, m, sigma)
        grid = np.exp(np.log(1e-8) * (63 - np.arange(64)) / 63.0)
        grid[-1] = 1.0
        ess = np.array([np_scan(U, np.zeros(N), r, c)[2] for c in grid])
        betas = _dev([0.0, -1.0])
        info = torch.zeros(2, dtype=torch.float64, device="cuda:0")
        Ud, qd, md = _dev(U), _dev(q), _dev(m)      # held: the kernels run after the call returns
        lib.call("pbbi_smc_next_beta", Ud.data_ptr(), None, qd.data_ptr(), md.data_ptr(), sigma, N, N, D, rho,
                 betas.data_ptr(), info.data_ptr(), lib.F64, 0, _st())
        got, inf = betas.cpu().numpy()[1], info.cpu().numpy()
        a = int(np.argmax(ess))
        if ess[a] < rho:
            assert inf[0] == 1.0 and abs(got - grid[a]) < 1e-12 * grid[a], (D, got, grid[a])
            continue
        assert inf[0] == 0.0
        i = a
        while i + 1 < 64 and ess[i + 1] >= rho:
            i += 1
        assert i < 63
        # the documented refinement: 6 passes of 64 interior points, the first one below the target closes the bracket
        lo, hi = grid[i], grid[i + 1]
        for _ in range(6):
            pts = lo + (hi - lo) * np.arange(1, 65) / 65.0
            e = np.array([np_scan(U, np.zeros(N), r, c)[2] for c in pts])
            j = int(np.argmax(e < rho)) if np.any(e < rho) else 64
            lo, hi = (lo if j == 0 else pts[j - 1]), (hi if j == 64 else pts[j])
        assert abs(got - lo) < 1e-10, (D, rho, got, lo)
        # and it is a crossing within the reported final width
        assert np_scan(U, np.zeros(N), r, got)[2] >= rho - 1e-12
        assert np_scan(U, np.zeros(N), r, got + inf[1])[2] < rho + 1e-12
        assert 0.0 < inf[1] < 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_resample_with_leading_stride(lib, dtype):
    """ldn > N (and ldn not a multiple of the vector width): the gather's scalar tail, padding left alone."""
    import torch
    N, D, ldn = 1003, 7, 1030
    rng = np.random.default_rng(2)
    qfull = rng.standard_normal((D, ldn)).astype(dtype)
    lw = rng.standard_normal(N) * 2.0
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    qi = _dev(qfull, dtype)
    qo = torch.full((D, ldn), -7.0, dtype=tdt, device="cuda:0")
    anc = torch.empty(N, dtype=torch.int32, device="cuda:0")
    ticks = torch.empty(N, dtype=torch.int64, device="cuda:0")
    lib.call("pbbi_smc_resample_systematic", _dev(lw).data_ptr(), N, 5, 4, qi.data_ptr(), qo.data_ptr(), ldn, D, None,
             1.0, anc.data_ptr(), ticks.data_ptr(), None, None, lib.F64 if dtype == np.float64 else lib.F32, 0, _st())
    a_ref = np_ancestors(ticks.cpu().numpy().view(np.uint64), stage_k(5, 4))
    assert np.array_equal(anc.cpu().numpy(), a_ref)
    out = qo.cpu().numpy()
    assert np.array_equal(out[:, :N], qfull[:, :N][:, a_ref])
    assert np.all(out[:, N:] == -7.0)
