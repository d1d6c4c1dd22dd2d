"""Running statistics (stats.py, csrc/kernels_stats.hip), the checks that need no GPU: the documented
state size, argument validation through the C ABI (every check comes before any launch), and the accumulate /
finalise arithmetic itself -- a NumPy restatement run over the four cuts against the longdouble reference."""
import ctypes as C

import numpy as np
import pytest

from running_stats_ref import CUTS, PER_CHAIN, NumpyRunningStats, ar1, cut_slabs, distance, reference, tolerance


@pytest.fixture(scope="module")
def lib():
    from physicsbasedbayesianinference_amd import _lib
    _lib.load()
    return _lib


@pytest.mark.parametrize("D,N,T", [(1, 1, 0), (3, 5, 5), (17, 257, 32), (128, 65536, 8), (128, 65536, 32)])
def test_state_len_is_the_documented_function(lib, D, N, T):
    from physicsbasedbayesianinference_amd import stats
    out = C.c_int64(-1)
    lib.call("pbbi_stats_state_len", D, N, T, C.byref(out))
    assert out.value == (3 * T + 3) * D * N + 2 * D + D * D
    assert stats.state_len(D, N, T) == out.value


def test_state_len_rejects_bad_arguments(lib):
    from physicsbasedbayesianinference_amd import stats
    out = C.c_int64(0)
    for D, N, T in ((3, 5, 33), (3, 5, -1), (0, 5, 4), (3, 0, 4)):
        assert lib.load().pbbi_stats_state_len(D, N, T, C.byref(out)) == lib.ERR_INVALID
        assert lib.last_error()
        with pytest.raises(ValueError):
            stats.state_len(D, N, T)
    assert lib.load().pbbi_stats_state_len(3, 5, 4, None) == lib.ERR_INVALID


def test_c_abi_rejects_invalid_arguments_before_any_launch(lib):
    """Pointers that are never dereferenced stand in for device buffers: every call below must fail in its argument
    checks (this machine may have no GPU at all)."""
    L = lib.load()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)

    def acc(**k):
        a = dict(state=p, D=3, N=5, T=5, S_before=0, slabs=p, c=2, dtype=lib.F64, device=0, stream=None)
        a.update(k)                                          # (keeps the positions)
        return L.pbbi_stats_accumulate(*a.values())

    for bad in (dict(T=33), dict(T=-1), dict(c=0), dict(slabs=None), dict(state=None), dict(dtype=7),
                dict(S_before=-1), dict(D=0), dict(N=0)):
        assert acc(**bad) == lib.ERR_INVALID, bad
        assert lib.last_error()

    def fin(**k):
        a = dict(state=p, D=3, N=5, T=5, S=4, device=0, mean=p, var=None, cov=None, acov=None, W=None, bvar=None,
                 chain_mean=None, chain_var=None, stream=None)
        a.update(k)
        return L.pbbi_stats_finalize(*a.values())

    for bad in (dict(T=33), dict(S=0), dict(S=1, W=p), dict(S=1, chain_var=p), dict(state=None), dict(D=0)):
        assert fin(**bad) == lib.ERR_INVALID, bad
        assert lib.last_error()


def test_python_rejects_invalid_arguments_without_a_device():
    from physicsbasedbayesianinference_amd.stats import RunningStats
    for kw in (dict(D=3, N=5, max_lag=33), dict(D=3, N=5, max_lag=-1), dict(D=0, N=5), dict(D=3, N=0)):
        with pytest.raises(ValueError):
            RunningStats(device=0, **kw)


@pytest.mark.parametrize("D,N,T", [(3, 5, 32), (2, 7, 5), (1, 1, 1), (2, 3, 0)])
def test_numpy_restatement_of_the_arithmetic_matches_longdouble(D, N, T):
    """Shifted sums, head, window and the correction formula, over the four cuts of 40 draws (a head and a window
    that fill over three chunks at T = 32 with [3, 1, 7, 29]; chunks of one draw): every finalised quantity within
    1e-12 max(1, max|ref|) of the longdouble definitions, and everything but cov identical under re-chunking."""
    x = ar1(D, N)
    ref = reference(x, T)
    first = None
    for cut in CUTS:
        rs = NumpyRunningStats(D, N, T)
        for slab in cut_slabs(x, cut):
            rs.update(slab)
        got = rs.finalize()
        assert sorted(got) == sorted(ref)
        for k in ref:
            assert distance(got[k], ref[k]) <= tolerance(ref[k]), (k, cut, distance(got[k], ref[k]))
        if first is None:
            first = got
        for k in PER_CHAIN:
            assert np.array_equal(got[k], first[k]), (k, cut)


@pytest.mark.parametrize("S", [1, 2, 3])
def test_numpy_restatement_short_runs(S):
    """Fewer draws than lags: lags t >= S are exactly 0 (the formula is not evaluated there), the others match."""
    D, N, T = 3, 5, 5
    x = ar1(D, N)[:S]
    ref = reference(x, T)
    got = NumpyRunningStats(D, N, T).update(x).finalize()
    assert sorted(got) == sorted(ref) and ("W" in got) == (S >= 2)
    assert np.all(got["acov"][S:] == 0.0)
    for k in ref:
        assert distance(got[k], ref[k]) <= tolerance(ref[k]), (k, distance(got[k], ref[k]))


def test_rhat_and_ess_host_formulas():
    """The formulas HMC.rhat / HMC.ess and RunningStats share: R-hat of identical chain means is sqrt((S-1)/S); an
    AR(1) autocovariance gives ESS = N S (1 - phi) / (1 + phi) up to the truncation of the Geyer sum."""
    from physicsbasedbayesianinference_amd.stats import ess_from_autocov, rhat_from_moments
    assert np.allclose(rhat_from_moments(np.array([2.0]), np.array([0.0]), 10, 4), np.sqrt(0.9))
    S, N, T, phi = 4000, 8, 32, 0.8
    g = (phi ** np.arange(T + 1))[:, None] * np.ones((1, 2))
    ess, trunc = ess_from_autocov(g, np.zeros(2), S, N, T)
    assert trunc.all()                                       # phi^t stays positive: the sum is cut by T
    assert np.allclose(ess, N * S * (1 - phi) / (1 + phi), rtol=1e-2)
