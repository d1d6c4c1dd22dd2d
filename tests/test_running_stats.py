"""Running statistics on the device (stats.RunningStats, HMC.sampleStats, csrc/kernels_stats.hip).

AR(1) chains from a fixed seed (running_stats_ref.ar1: phi = 0.6, mean 3, per-chain offsets -- not centred), 40
draws cut as [40], [1]*40, [3, 1, 7, 29] and [33, 7].  The reference is NumPy longdouble from the definitions of
include/pbbi.h; the tolerance of every finalised quantity is 1e-12 * max(1, max|reference|).  The per-chain
quantities have at most 40 terms and the ensemble sums at most S*N = 12 000 (n 2^-53 ~ 1.3e-12 worst case; a
fixed-order blocked sum stays far below).  Everything formed from the per-chain state must be identical bit for bit
under re-chunking; cov only agrees within the tolerance.  The one-shot device functions are held to the same reference
at the same tolerance on the first case; test_sample_diagnostics.py holds both sinks away from the origin."""
import ctypes as C

import numpy as np
import pytest

from running_stats_ref import CUTS, PER_CHAIN, S_TOTAL, ar1, cut_slabs, distance, reference, tolerance

pytestmark = pytest.mark.gpu

# (D, N, max_lag): N = 257 / 300 span two blocks of the chain reduction with a tail, D = 17 is one past a covariance
# tile, N = 1 has no second chain, max_lag = 32 with [3, 1, 7, 29] fills the head and the window over three chunks
CASES = [(17, 257, 5), (1, 1, 5), (3, 300, 32), (3, 5, 32), (1, 256, 0), (3, 300, 1), (17, 5, 32)]


@pytest.fixture(scope="module")
def P():
    import physicsbasedbayesianinference_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def lib():
    from physicsbasedbayesianinference_amd import _lib
    _lib.load()
    return _lib


def _dev(a, dtype=None):
    import torch
    return torch.tensor(np.array(a), dtype=dtype or torch.float64, device="cuda")   # (a writable copy)


def _run(P, x, cut, T, dtype=None):
    D, N = x.shape[1:]
    rs = P.RunningStats(D, N, max_lag=T, device=0)
    for slab in cut_slabs(x, cut):
        rs.update(_dev(slab, dtype))
    return rs


def _check(got, ref, label):
    assert sorted(got) == sorted(ref)
    for k in sorted(ref):
        dist, tol = distance(got[k], ref[k]), tolerance(ref[k])
        print(f"{label} {k}: |got - numpy| = {dist:.3e} (tolerance {tol:.3e})")
        assert dist <= tol, (label, k, dist, tol)


def _one_shot_distances(lib, x, T, ref):
    """The one-shot device functions on the same draws, held to the same reference at the same tolerance."""
    import torch
    from physicsbasedbayesianinference_amd._device import stream_ptr
    S, D, N = x.shape
    xd, st = _dev(x), stream_ptr(0)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
    mean, var, cm, cv, acov, cov = new(D), new(D), new(D, N), new(D, N), new(T + 1, D), new(D, D)
    lib.call("pbbi_sample_moments", xd.data_ptr(), S, D, N, lib.F64, 0, mean.data_ptr(), var.data_ptr(), st)
    lib.call("pbbi_chain_moments", xd.data_ptr(), S, D, N, lib.F64, 0, cm.data_ptr(), cv.data_ptr(), st)
    lib.call("pbbi_chain_autocov", xd.data_ptr(), cm.data_ptr(), S, D, N, T, lib.F64, 0, acov.data_ptr(), st)
    lib.call("pbbi_sample_covariance", xd.data_ptr(), S, D, N, lib.F64, 0, mean.data_ptr(), cov.data_ptr(), st)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in dict(mean=mean, var=var, chain_mean=cm, chain_var=cv, acov=acov, cov=cov).items()}
    _check(got, {k: ref[k] for k in got}, "one-shot")


@pytest.mark.parametrize("D,N,T", CASES)
def test_chunking_invariance_and_numpy(P, lib, D, N, T):
    x = ar1(D, N)
    ref = reference(x, T)
    if (D, N, T) == CASES[0]:
        _one_shot_distances(lib, x, T, ref)
    first = None
    for cut in CUTS:
        rs = _run(P, x, cut, T)
        assert rs.count == S_TOTAL and rs.state_bytes == 8 * ((3 * T + 3) * D * N + 2 * D + D * D)
        got = rs.finalize(chain_moments=True)
        _check(got, ref, f"D={D} N={N} T={T} cut={cut if len(cut) < 5 else '[1]*40'}")
        mean, var = rs.moments()
        mean2, cov = rs.covariance()
        assert np.array_equal(mean, got["mean"]) and np.array_equal(var, got["var"]) and np.array_equal(mean2, mean)
        assert np.array_equal(cov, got["cov"]) and np.array_equal(cov, cov.T)
        diag = dict(got)
        if N >= 2:
            diag["rhat"] = rs.rhat()
            diag["ess"] = rs.ess()
            diag["ess_truncated"] = rs.ess_truncated
        if first is None:
            first = diag
            continue
        for k in PER_CHAIN + (("rhat", "ess", "ess_truncated") if N >= 2 else ()):
            assert np.array_equal(diag[k], first[k]), (k, cut)      # identical bits
        assert distance(diag["cov"], first["cov"].astype(np.longdouble)) <= tolerance(ref["cov"])


def test_rhat_and_ess_follow_the_hmc_methods(P):
    """Same return conventions and the same numbers (to rounding) as HMC.rhat / HMC.ess on the resident draws, the
    same ess_truncated marker, T_eff = min(max_lag, S - 2) lags."""
    D, N = 3, 300
    x = ar1(D, N)
    hmc = P.HMC(P.Ensemble(D, N), 1.0, 0.1, None, potential=P.StandardGaussian(D), verbose=False)
    dns = _dev(x).permute(1, 2, 0)
    rs = P.RunningStats(D, N, max_lag=32, device=0).update(dns)       # the (D, N, S) view itself
    assert np.allclose(rs.rhat(), hmc.rhat(dns), rtol=1e-12, atol=0)
    for lag in (None, 32, 7, 2):
        want = hmc.ess(dns) if lag is None else hmc.ess(dns, max_lag=lag)
        got = rs.ess() if lag is None else rs.ess(max_lag=lag)
        assert got.shape == (D,) and got.dtype == np.float64
        assert np.allclose(got, want, rtol=1e-9, atol=0), (lag, got, want)
        assert np.array_equal(rs.ess_truncated, hmc.ess_truncated)
    short = P.RunningStats(D, N, max_lag=32, device=0).update(_dev(x[:6]))
    assert np.allclose(short.ess(), hmc.ess(_dev(x[:6]).permute(1, 2, 0)), rtol=1e-9, atol=0)   # T_eff = 4
    with pytest.raises(ValueError):
        P.RunningStats(D, N, max_lag=4, device=0).update(dns).ess(max_lag=5)


@pytest.mark.parametrize("S", [1, 2, 3])
def test_short_runs(P, S):
    """Fewer draws than lags (max_lag = 5): lags t >= S are exactly 0, the others match NumPy; rhat / ess raise the
    ValueErrors of the HMC methods."""
    D, N, T = 3, 5, 5
    x = ar1(D, N)[:S]
    ref = reference(x, T)
    hmc = P.HMC(P.Ensemble(D, N), 1.0, 0.1, None, potential=P.StandardGaussian(D), verbose=False)
    dns = _dev(x).permute(1, 2, 0)
    for cut in ([S], [1] * S):
        rs = _run(P, x, cut, T)
        got = rs.finalize(chain_moments=True)
        assert ("W" in got) == (S >= 2) and ("chain_var" in got) == (S >= 2)
        _check(got, ref, f"S={S} cut={cut}")
        assert np.all(got["acov"][S:] == 0.0)
        pairs = [(rs.ess, lambda: hmc.ess(dns))] + ([(rs.rhat, lambda: hmc.rhat(dns))] if S < 2 else [])
        for mine_fn, theirs_fn in pairs:
            with pytest.raises(ValueError) as mine:
                mine_fn()
            with pytest.raises(ValueError) as theirs:
                theirs_fn()
            assert str(mine.value) == str(theirs.value)
        if S >= 2:
            assert np.allclose(rs.rhat(), hmc.rhat(dns), rtol=1e-12, atol=0)
    one_chain = _run(P, ar1(3, 1), [S_TOTAL], T)
    for fn in (one_chain.rhat, one_chain.ess):
        with pytest.raises(ValueError):
            fn()
    with pytest.raises(ValueError):
        P.RunningStats(D, N, max_lag=T, device=0).moments()          # nothing accumulated


def test_fp32_slabs(P):
    """The same draws rounded to fp32, accumulated from fp32 slabs into the fp64 state: compared with NumPy on the
    rounded values, at the same tolerance; re-chunking still changes no bit."""
    import torch
    D, N, T = 17, 257, 5
    x32 = ar1(D, N).astype(np.float32)
    ref = reference(x32.astype(np.float64), T)
    first = None
    for cut in CUTS:
        got = _run(P, x32, cut, T, dtype=torch.float32).finalize(chain_moments=True)
        _check(got, ref, f"fp32 cut={cut if len(cut) < 5 else '[1]*40'}")
        first = first or got
        for k in PER_CHAIN:
            assert np.array_equal(got[k], first[k]), (k, cut)


def test_finalize_continue_finalize(P):
    """Finalising leaves the state alone: 20 draws, finalise, 20 more, finalise = one pass over the 40."""
    D, N, T = 3, 300, 32
    x = ar1(D, N)
    rs = P.RunningStats(D, N, max_lag=T, device=0).update(_dev(x[:20]))
    _check(rs.finalize(chain_moments=True), reference(x[:20], T), "after 20")
    rs.rhat(), rs.ess(), rs.covariance()
    again = rs.update(_dev(x[20:])).finalize(chain_moments=True)
    once = _run(P, x, [40], T).finalize(chain_moments=True)
    for k in PER_CHAIN:
        assert np.array_equal(again[k], once[k]), k
    assert distance(again["cov"], once["cov"].astype(np.longdouble)) <= tolerance(reference(x, T)["cov"])


def test_update_accepts_views_and_slabs(P):
    import torch
    D, N = 3, 5
    x = ar1(D, N)
    slabs = _dev(x)                                                   # (c, D, N)
    want = P.RunningStats(D, N, 5, device=0).update(slabs).finalize(True)
    for form in (slabs.permute(1, 2, 0), slabs.permute(1, 2, 0).contiguous()):   # the view, and a (D, N, c) copy
        got = P.RunningStats(D, N, 5, device=0).update(form).finalize(True)
        for k in want:
            assert np.array_equal(got[k], want[k]), k
    rs = P.RunningStats(D, N, 5, device=0)
    with pytest.raises(TypeError):
        rs.update(x)                                                  # a NumPy array
    with pytest.raises(TypeError):
        rs.update(slabs.to(torch.float16))
    with pytest.raises(ValueError):
        rs.update(_dev(ar1(3, 300)))                                  # another ensemble's shape
    with pytest.raises(ValueError):
        rs.update(slabs[:0])                                          # c < 1
    with pytest.raises(ValueError):
        rs.update(slabs.cpu())
    assert rs.count == 0


def test_c_abi_validation_on_the_device(lib):
    """PBBI_ERR_INVALID with a message, before anything is launched, with real device buffers as the other arguments."""
    import torch
    from physicsbasedbayesianinference_amd._device import stream_ptr
    D, N, T = 3, 5, 5
    n = C.c_int64(0)
    lib.call("pbbi_stats_state_len", D, N, T, C.byref(n))
    state = torch.full((n.value,), 7.0, dtype=torch.float64, device="cuda")
    x, out = _dev(ar1(D, N)[:2]), torch.zeros(D * N, dtype=torch.float64, device="cuda")
    L, st = lib.load(), stream_ptr(0)
    bad_acc = [(state.data_ptr(), D, N, 33, 0, x.data_ptr(), 2, lib.F64, 0, st),
               (state.data_ptr(), D, N, T, 0, x.data_ptr(), 0, lib.F64, 0, st),
               (state.data_ptr(), D, N, T, 0, None, 2, lib.F64, 0, st),
               (state.data_ptr(), D, N, T, 0, x.data_ptr(), 2, 9, 0, st)]
    for args in bad_acc:
        assert L.pbbi_stats_accumulate(*args) == lib.ERR_INVALID and lib.last_error()
    o = out.data_ptr()
    for S, w, cv in ((0, None, None), (1, o, None), (1, None, o)):
        assert L.pbbi_stats_finalize(state.data_ptr(), D, N, T, S, 0, o, None, None, None, w, None, None, cv,
                                     st) == lib.ERR_INVALID and lib.last_error()
    assert L.pbbi_stats_finalize(state.data_ptr(), D, N, 33, 4, 0, o, None, None, None, None, None, None, None,
                                 st) == lib.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((state == 7.0).all()) and bool((out == 0.0).all())   # nothing ran


def test_sample_stats_against_get_samples(P):
    """HMC.sampleStats (24 iterations in chunks of 5, no host synchronisation between them) against
    RunningStats.update on the resident draws of getSamples(24, rng="philox") for the same seed: identical bits for
    everything but cov; the same accept rate; sampleChunks(stats=rs) feeds the same state; burn_in=4 equals the
    last 20 draws of a run of 24 -- the state after four iterations is the one getSamples(24) itself passes
    through, so its draws 4..23 are what a run started there with iter0 shifted by 4 records."""
    from scipy.constants import k as kB
    D, N, S, chunk, T = 3, 300, 24, 5, 8
    rs0 = np.random.RandomState(5)
    pot = P.GaussianDiag(rs0.standard_normal(D), prec=rs0.uniform(0.5, 2.0, D), const=0.0)
    hmc = P.HMC(P.Ensemble(D, N), 1.0, 0.1, None, potential=pot, rng="philox", seed=11, verbose=False)
    view, _ = hmc.getSamples(S, 1 / kB, 1.0, device_output=True)
    rate, masks = hmc.acceptRate, hmc.reject_masks
    ref = reference(view.permute(2, 0, 1).cpu().numpy(), T)
    want = P.RunningStats(D, N, max_lag=T, device=0).update(view)
    wf = want.finalize(chain_moments=True)
    _check(wf, ref, "getSamples view")

    def same(rs, target, label):
        got = rs.finalize(chain_moments=True)
        for k in PER_CHAIN:
            assert np.array_equal(got[k], target[k]), (label, k)
        tol = tolerance(np.asarray(target["cov"], dtype=np.longdouble))
        assert distance(got["cov"], target["cov"].astype(np.longdouble)) <= tol, label

    rs = hmc.sampleStats(S, chunk, 1 / kB, 1.0, max_lag=T)
    assert isinstance(rs, P.RunningStats) and rs.count == S and rs.max_lag == T
    assert hmc.acceptRate == rate and 0.0 < rate < 1.0
    same(rs, wf, "sampleStats")
    assert np.array_equal(rs.rhat(), want.rhat()) and np.array_equal(rs.ess(), want.ess())

    fed = P.RunningStats(D, N, max_lag=T, device=0)
    seen = sum(s.shape[2] for s, _ in hmc.sampleChunks(S, chunk, 1 / kB, 1.0, stats=fed))
    assert seen == S and fed.count == S and hmc.acceptRate == rate
    same(fed, wf, "sampleChunks(stats=)")

    tail = P.RunningStats(D, N, max_lag=T, device=0).update(view[:, :, 4:]).finalize(chain_moments=True)
    burned = hmc.sampleStats(S - 4, chunk, 1 / kB, 1.0, burn_in=4, max_lag=T)
    assert burned.count == S - 4
    same(burned, tail, "burn_in=4")
    assert hmc.acceptRate == 1.0 - float(masks[4:].mean())
