"""k_dense_hmc with the interior kicks accumulated in the MFMA's C operand (kernels_dense_dev.h: matvec_inplace,
momentum kept in gradient units w = vh / (-h/m)).

The shapes are the smallest at which the step loop can go wrong: N = 53 is three full 16-chain tiles and a ragged
one in ONE workgroup (four of its eight waves return early); D = 128 / 100 / 96 / 64 / 33 are the full tile, padded
rows with skipped K-steps, and the one-pass six-tile kernel; L = 1 has no in-place trip, L = 2 one, L = 3 two back
to back; 3 iterations per pbbi_hmc_run read the carried gradient twice.

Against the oracle: reject masks equal, positions and momenta within the dense path's 1e-11 (scaled).  With
PBBI_DRAW_F64 the oracle draws its own momenta (oracle.hmc_run_philox); the single-precision draw is replayed from
pbbi_philox_normal / pbbi_philox_uniform, which return the in-kernel draws bit for bit (the host restatement of the
hardware's single-precision log / sin / cos agrees to 5e-6 only, test_gpu_parity.test_philox_device_matches_oracle).

The step sizes of the rejection cases were found with the oracle on the CPU (same problem, same counters, all four
of draw precision x mean): of a 48-point geometric grid on [0.05, 2.5], the step whose four rates (3 iterations x 53
chains each) lie nearest to 37.5 %; the oracle's rates at the chosen steps are 32-43 %.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import oracle as orc
from test_gpu_fullsize import _stress_problem
from test_gpu_parity import device_normal, device_uniform, scaled_err

pytestmark = pytest.mark.gpu

TOL = 1e-11
N, S, SEED, ITER0, CHAIN0 = 53, 3, 17, 4, 29
METHODS = ["Leapfrog", "Stormer-Verlet"]
MASS = np.random.RandomState(5).uniform(0.5, 2.0, N)  # per-chain masses from [0.5, 2]

# (D, method, L, masses) -> step size with 25-50 % rejections (see the module docstring)
H_REJECT = {
    (128, "Leapfrog", 1, False): 0.717, (128, "Leapfrog", 1, True): 0.717, (128, "Leapfrog", 2, False): 0.559,
    (128, "Leapfrog", 2, True): 0.559, (128, "Leapfrog", 3, False): 0.514, (128, "Leapfrog", 3, True): 0.514,
    (128, "Stormer-Verlet", 1, False): 0.125, (128, "Stormer-Verlet", 1, True): 0.136, (128, "Stormer-Verlet", 2, False): 0.106,
    (128, "Stormer-Verlet", 2, True): 0.115, (128, "Stormer-Verlet", 3, False): 0.097, (128, "Stormer-Verlet", 3, True): 0.106,
    (100, "Leapfrog", 1, False): 0.717, (100, "Leapfrog", 1, True): 0.78, (100, "Leapfrog", 2, False): 0.607,
    (100, "Leapfrog", 2, True): 0.607, (100, "Leapfrog", 3, False): 0.559, (100, "Leapfrog", 3, True): 0.607,
    (100, "Stormer-Verlet", 1, False): 0.136, (100, "Stormer-Verlet", 1, True): 0.148, (100, "Stormer-Verlet", 2, False): 0.115,
    (100, "Stormer-Verlet", 2, True): 0.125, (100, "Stormer-Verlet", 3, False): 0.106, (100, "Stormer-Verlet", 3, True): 0.115,
}


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


def _problem(P, D, zero_mean):
    """One device potential and one oracle potential per (D, mean) for the whole module."""
    key = (D, zero_mean)
    if key not in _POTS:
        Pm, mu = _stress_problem(D, zero_mean)
        _POTS[key] = (P.GaussianDense(None if zero_mean else mu, precision=Pm, const=0.25),
                      orc.pot_gauss_dense(mu, Pm, 0.25), mu)
    return _POTS[key]


def _run(lib, pot, method, q0, m, h, L, S_, flags, iter0=ITER0, per_call=None):
    import torch
    from physicsbasedbayesianinference_amd._device import as_device, empty, stream_ptr, to_numpy
    D, n = q0.shape
    qd = as_device(q0, 0, np.float64)
    md = as_device(m, 0, np.float64) if m is not None else None
    samples, momenta = empty((S_, D, n), np.float64, 0), empty((S_, D, n), np.float64, 0)
    reject, ratio = empty((S_, n), np.uint8, 0), empty((S_, n), np.float64, 0)
    per_call = per_call or S_
    for i in range(0, S_, per_call):
        lib.call("pbbi_hmc_run", pot.handle, orc.METHODS[method], qd.data_ptr(), md.data_ptr() if md is not None else None,
                 samples[i].data_ptr(), momenta[i].data_ptr(), reject[i].data_ptr(), ratio[i].data_ptr(), n, n, h, L,
                 min(per_call, S_ - i), flags, SEED, iter0 + i, CHAIN0, 1.0, stream_ptr(0))
    torch.cuda.synchronize()
    return to_numpy(samples), to_numpy(momenta), to_numpy(reject).astype(bool), to_numpy(ratio), to_numpy(qd)


def _against_oracle(P, lib, D, method, L, h, band=None):
    """masses x mean x draw precision at one (D, method, L, h); returns nothing, asserts everything."""
    for mass in (False, True):
        m = MASS if mass else None
        hh = h if h is not None else H_REJECT[(D, method, L, mass)]
        for zero_mean in (True, False):
            pot, op, mu = _problem(P, D, zero_mean)
            for f64 in (True, False):
                tag = f"D={D} {method} L={L} mass={mass} zero_mean={zero_mean} f64={f64} h={hh}"
                flags = lib.COMPAT_P_FROM_OLDQ | (lib.DRAW_F64 if f64 else 0)
                if f64:
                    q0 = orc.philox_normal(SEED, orc.STREAM_POSITION | orc.STREAM_DRAW_F64, ITER0, CHAIN0, D, N, 1.0)
                else:
                    q0 = device_normal(lib, SEED, lib.STREAM_POSITION, ITER0, CHAIN0, D, N, 1.0)
                q0 = np.ascontiguousarray(q0 + mu[:, None])
                gs, gm, gr, _, gq = _run(lib, pot, method, q0, m, hh, L, S, flags)
                q = q0.copy()
                if f64:
                    os_, om, orj, _ = orc.hmc_run_philox(op, method, q, m, hh, L, S, SEED, ITER0, CHAIN0, 1.0,
                                                        compat=orc.COMPAT_P_FROM_OLDQ | orc.DRAW_F64)
                else:
                    os_, om, orj = np.empty_like(gs), np.empty_like(gm), np.empty_like(gr)
                    pstd = np.sqrt(m) if mass else np.ones(N)
                    for i in range(S):
                        p = device_normal(lib, SEED, lib.STREAM_MOMENTUM, ITER0 + i, CHAIN0, D, N, 1.0, pstd)
                        u = device_uniform(lib, SEED, ITER0 + i, CHAIN0, N)
                        _, orj[i] = orc.hmc_iter(op, method, q, p, u, m, hh, L)
                        os_[i], om[i] = q, p
                es, em = scaled_err(gs, os_), scaled_err(gm, om)
                print(f"{tag}: reject {gr.mean():.3f}, scaled error q {es:.2e} p {em:.2e}")
                assert np.array_equal(gr, orj), tag
                assert es <= TOL and em <= TOL, (tag, es, em)
                assert np.array_equal(gq, gs[S - 1]), tag
                if band is not None:
                    assert band[0] <= gr.mean() <= band[1], (tag, gr.mean())


@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("D", [128, 100, 96, 64, 33])
def test_inplace_kick_vs_oracle(P, lib, D, method, L):
    _against_oracle(P, lib, D, method, L, 0.1)


@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("D", [128, 100])
def test_inplace_kick_vs_oracle_with_rejections(P, lib, D, method, L):
    """The same grid at a step size that rejects 25-50 % of the proposals: the reject path is really taken."""
    _against_oracle(P, lib, D, method, L, None, band=(0.25, 0.50))


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("D", [128, 100])
def test_run_of_7_equals_7_runs_of_1(P, lib, D, method, L):
    """One run of 7 iterations (6 of them read the carried gradient) == 7 runs of one (each forms its own), bit
    for bit, with masses: the last trip's gradient is what a fresh mat-vec at that position produces."""
    pot, _, mu = _problem(P, D, False)
    q0 = np.ascontiguousarray(orc.philox_normal(SEED, orc.STREAM_POSITION | orc.STREAM_DRAW_F64, ITER0, CHAIN0, D, N, 1.0)
                              + mu[:, None])
    h = H_REJECT[(D, method, L, True)]
    one = _run(lib, pot, method, q0, MASS, h, L, 7, 0)
    each = _run(lib, pot, method, q0, MASS, h, L, 7, 0, per_call=1)
    for a, b in zip(one, each):
        assert np.array_equal(a, b)
    assert 0.1 < one[2].mean() < 0.6  # the selector both stays and flips


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("D", [128, 33])
def test_integrate_vs_oracle(P, lib, D, method, L):
    """pbbi_integrate (MODE 1): q, p in place and Integrator.v, with and without masses, zero and non-zero mean."""
    import torch
    from physicsbasedbayesianinference_amd._device import as_device, empty, stream_ptr, to_numpy
    h = 0.1
    rs = np.random.RandomState(100 * D + L)
    for mass in (False, True):
        m = MASS if mass else None
        for zero_mean in (True, False):
            pot, op, mu = _problem(P, D, zero_mean)
            q = rs.standard_normal((D, N)) + mu[:, None]
            p = rs.standard_normal((D, N)) * (np.sqrt(MASS) if mass else 1.0)
            qd, pd = as_device(q, 0, np.float64), as_device(p, 0, np.float64)
            md = as_device(m, 0, np.float64) if mass else None
            vd = empty((D, N), np.float64, 0)
            lib.call("pbbi_integrate", pot.handle, orc.METHODS[method], qd.data_ptr(), pd.data_ptr(),
                     md.data_ptr() if mass else None, vd.data_ptr(), N, N, h, L, stream_ptr(0))
            torch.cuda.synchronize()
            qo, po = np.ascontiguousarray(q), np.ascontiguousarray(p)
            vo = orc.integrate(op, method, qo, po, m, h, L)
            errs = [scaled_err(to_numpy(a), b) for a, b in ((qd, qo), (pd, po), (vd, vo))]
            print(f"D={D} {method} L={L} mass={mass} zero_mean={zero_mean}: scaled errors q, p, v = {errs}")
            assert max(errs) <= TOL, errs


# ---- the paths this change leaves alone: per-chain trajectory lengths (DYN) and streamed P (D = 192) ------------
def run_left_alone(P, lib, which):
    """The runs recorded in tests/golden/inplace_kick_<which>.npz by the build before this change."""
    import torch
    from physicsbasedbayesianinference_amd._device import as_device, empty, stream_ptr, to_numpy
    D, L, h = (100, 5, 0.45) if which == "dyn" else (192, 3, 0.3)
    Pm, mu = _stress_problem(D, False)
    pot = P.GaussianDense(mu, precision=Pm, const=0.25)
    q0 = np.random.RandomState(D).standard_normal((D, N)) + mu[:, None]
    qd, md = as_device(q0, 0, np.float64), as_device(MASS, 0, np.float64)
    samples = empty((S, D, N), np.float64, 0)
    reject, ratio = empty((S, N), np.uint8, 0), empty((S, N), np.float64, 0)
    out = {}
    if which == "dyn":
        steps = torch.full((S, N), -1, dtype=torch.int32, device="cuda")
        lib.call("pbbi_hmc_run_dyn", pot.handle, 0, qd.data_ptr(), md.data_ptr(), samples.data_ptr(), None,
                 reject.data_ptr(), ratio.data_ptr(), steps.data_ptr(), N, N, h, L, S,
                 lib.PER_CHAIN_STEPS | lib.UTURN_STOP, SEED, ITER0, CHAIN0, 1.0, stream_ptr(0))
        torch.cuda.synchronize()
        out["steps"] = to_numpy(steps)
    else:
        lib.call("pbbi_hmc_run", pot.handle, 0, qd.data_ptr(), md.data_ptr(), samples.data_ptr(), None,
                 reject.data_ptr(), ratio.data_ptr(), N, N, h, L, S, 0, SEED, ITER0, CHAIN0, 1.0, stream_ptr(0))
        torch.cuda.synchronize()
    out.update(samples=to_numpy(samples), reject=to_numpy(reject), ratio=to_numpy(ratio))
    return out


@pytest.mark.parametrize("which", ["dyn", "d192"])
def test_paths_left_alone_are_bit_identical_to_the_recording(P, lib, which):
    got = run_left_alone(P, lib, which)
    with np.load(os.path.join(GOLDEN, f"inplace_kick_{which}.npz")) as z:
        assert sorted(z.files) == sorted(got)
        for k in z.files:
            assert np.array_equal(z[k], got[k]), k
    if which == "dyn":  # the lengths really differ from chain to chain
        assert len(np.unique(got["steps"])) > 2
    assert 0.02 < got["reject"].mean() < 0.9
