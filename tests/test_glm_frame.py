"""The chain frame of the GLM kernels (csrc/kernels_glm.hip k_glm and its restated twin k_glm_softmax of
csrc/kernels_glm_softmax.hip) held to the oracle on the paths the project's own samplers take.

The eight test_glm*.py files hold the likelihood and the prior of every model to the oracle, all of them through one
configuration of the frame: PBBI_COMPAT_P_FROM_OLDQ | PBBI_DRAW_F64, Leapfrog, no masses, kT = 1, all four outputs, the
state at the base of its own allocation.  smc.TemperedSMC, tempering.TemperingLadder and HMC(compat=False) /
HMC(beta_accept=True) / HMC(draw_f64=False) call the kernels in other ways.  This file is the census of those ways.

Census: frame feature (the lines are k_glm's; k_glm_softmax has the same ones) -> the test that asserts it.

  pstd = sqrt(m kT), the in-kernel draw with masses and / or kT != 1   test_frame_run_flags_vs_oracle (every handle),
                                                                        test_frame_single_precision_draw_is_mapped_row_for_row
  the non-compat "park the draw now" store                             test_frame_run_flags_vs_oracle (the rejected
                                                                        chains' momenta are the oracle's Philox draw)
  store_p = false for a rejected chain under rng                       test_frame_run_flags_vs_oracle
  the non-compat, non-rng reload of p_in for a rejected chain          test_frame_uploaded_noncompat_vs_oracle
  have_pout == false with non-compat and rng                           test_frame_smc_shaped_call_vs_oracle,
                                                                        test_frame_ladder_shaped_call_vs_oracle
  have_pout == false, non-compat, uploaded draws                       test_frame_uploaded_noncompat_vs_oracle (second call)
  Stormer-Verlet's extra evaluation (nev = L + 2) with in-kernel draws test_frame_run_flags_vs_oracle (every handle: U_new,
                                                                        htau, dk, tsum of the last position feed the ratio)
  the accept test at 1 / kT (PBBI_BETA_ACCEPT) and at 1 with kT != 1   test_frame_run_flags_vs_oracle,
                                                                        test_frame_smc_shaped_call_vs_oracle (kT = 2, 50)
  rng_normal4d block index (k << 2) | g, single precision, NT = 2, 4, 8 test_frame_single_precision_draw_is_mapped_row_for_row
  ghost waves and the clamped tail, N < 16, a sub-ensemble whose       test_frame_ladder_shaped_call_vs_oracle (Nr = 1, 15,
  neighbours are live data, a base that is not 16-chain aligned         17, 37, 65 inside a (D, 3 Nr) array)
  the bounded descriptors: a padded row loads 0 and its store is       test_frame_state_inside_a_canary_allocation
  dropped, whatever lies behind the state
  the ladder as the class runs it (runs per rung, exchanges, rates)    test_frame_ladder_replayed_on_the_oracle
  every mask comparison above is fair: no accept test within 1e-7      test_frame_cases_are_decisive (CPU, the oracle alone)

Everywhere N = 150 (nine full 16-chain wave tiles and one of 6; the last workgroup has two ghost waves),
the Philox counters are seed 4, iteration 1, chain0 = 2^32 - 70 (the chain counter carries into its high word inside the
ensemble) and MASS = 1 + 0.5 (n % 3), the conventions of test_route_coverage.py.  Tolerance: test_glm.py's TOL = 1e-10
relative to max(1, max|oracle|) through its `rel` / `check`; masks are compared for equality with no chain excluded;
device against device is compared bit for bit.  (The largest error any case here showed on an MI355X is 5.0e-13, the
ratio of the full-model Poisson run; no case needed a figure of its own.)  Step sizes: each handle's own test file's (the first rows of its
ITER_CASES); where a hot kT or this file's start needed another one it was picked on the CPU by
test_frame_cases_are_decisive and stands in STEP.
"""
import functools

import numpy as np
import pytest

import test_glm as t_plain
import test_glm_dispersion as t_disp
import test_glm_hier as t_hier
import test_glm_hier_dispersion as t_hd
import test_glm_hier_noncentred as t_nc
import test_glm_hier_penalty as t_pen
import test_glm_model as t_model
import test_glm_softmax as t_soft
from oracle import oracle as orc
from test_glm import check     # rel <= TOL = 1e-10, both of that file

N, SEED, ITER0, CHAIN0 = 150, 4, 1, 2 ** 32 - 70
MASS = 1.0 + 0.5 * (np.arange(N) % 3)
METHODS = ["Leapfrog", "Stormer-Verlet"]
KT = 2.5
S_RUN = 3
NQ = 207          # columns of every handle's start: the widest call is the ladder of 3 x 69
DATA_SEED = 11    # the seed of every test file's ITER_CASES data


# ---- the table of handles -------------------------------------------------------------------------------------------
def _plain(D):
    X, y, w, rs = t_plain.problem("logistic", 203, D, DATA_SEED)
    return (lambda P: P.GLM(X, y)), t_plain.oracle_pot("logistic", X, y), t_plain.start(w, NQ, rs)


def _poisson_full():
    kw, w, rs = t_model.problem("poisson", 300, 8, DATA_SEED)
    return (lambda P: P.GLM(**kw)), t_model.oracle_pot(kw), t_model.start(w, NQ, rs, spread=0.1)


def _dispersion(family, sampled):
    kw, w, theta, rs = t_disp.problem(family, 40, 5, DATA_SEED)
    return ((lambda P: t_disp.make(P, kw, sampled, theta)), t_disp.oracle_pot(kw, sampled, theta),
            t_disp.start(w, theta, NQ, rs, spread=0.1, sampled=sampled))


def _hier(noncentred):
    kw, w, t, rs = t_hier.problem("logistic", 40, 5, 2, DATA_SEED)
    if noncentred:
        return (lambda P: t_nc.nc_pot(P, kw)), t_nc.oracle_nc(kw), t_nc.nc_start(kw, w, t, NQ, rs, spread=0.1)
    return (lambda P: P.HierarchicalGLM(**kw)), t_hier.oracle_pot(kw), t_hier.start(w, t, NQ, rs, spread=0.1)


def _penalty():
    kw, w, t, rs = t_pen.problem("logistic", 40, 5, 2, DATA_SEED, mix=0)
    return (lambda P: P.HierarchicalGLM(**kw)), t_pen.oracle_pot(kw), t_pen.start(w, t, NQ, rs, spread=0.1)


def _hier_dispersion(par):
    kw, w, t, theta, rs = t_hd.problem("gaussian", 40, 5, 2, DATA_SEED)
    return ((lambda P: t_hd.make(P, kw, par, True)), t_hd.oracle_pot(kw, par, True),
            t_hd.start(kw, par, w, t, theta, NQ, rs, spread=0.1))


def _softmax():
    M, D, K = t_soft.CASES["A"][:3]
    X, y, w, rs = t_soft.problem(M, D, K)
    q = np.ascontiguousarray(w[:, None] + 0.3 * rs.standard_normal((K * D, NQ)))
    return (lambda P: t_soft.device_pot("A")), t_soft.oracle_pot("A"), q


# handle -> how it is made, its file's step sizes (Leapfrog, Stormer-Verlet) and trajectory length
KINDS = {
    "logistic": dict(make=lambda: _plain(5), h=(0.45, 0.45), L=8),                       # test_glm.ITER_CASES, M = 203
    "poisson_full": dict(make=_poisson_full, h=(0.06, 0.06), L=10),                      # test_glm_model, M = 300, D = 8
    "gaussian_sampled": dict(make=lambda: _dispersion("gaussian", True), h=(0.2, 0.12), L=8),
    "negbinomial_held": dict(make=lambda: _dispersion("negbinomial", False), h=(0.6, 0.3), L=8),
    "hier": dict(make=lambda: _hier(False), h=(0.2, 0.15), L=8),
    "hier_nc": dict(make=lambda: _hier(True), h=(0.15, 0.15), L=8),
    "hier_penalty": dict(make=_penalty, h=(0.25, 0.15), L=8),
    "hier_disp": dict(make=lambda: _hier_dispersion("centred"), h=(0.17, 0.17), L=8),
    "hier_disp_nc": dict(make=lambda: _hier_dispersion("noncentred"), h=(0.17, 0.17), L=8),
    "softmax": dict(make=_softmax, h=(0.3, 0.3), L=8),                                   # test_glm_softmax.CASES["A"]
    "logistic17": dict(make=lambda: _plain(17), h=(0.4, 0.4), L=8),                      # NT = 2
    "logistic50": dict(make=lambda: _plain(50), h=(0.25, 0.25), L=8),                    # NT = 4
    "logistic128": dict(make=lambda: _plain(128), h=(0.2, 0.2), L=8),                    # NT = 8
}
FRAMES = ("logistic", "softmax")          # one handle of each twin takes the full product of test 2
_BUILT, _DEVICE = {}, {}


def _kind(name):
    """(device factory, oracle potential, the (Dt, NQ) start) of a handle, made once per module."""
    if name not in _BUILT:
        dev, op, q = KINDS[name]["make"]()
        q.setflags(write=False)
        _BUILT[name] = (dev, op, q)
    return _BUILT[name]


def _pot(P, name):
    if name not in _DEVICE:
        _DEVICE[name] = _kind(name)[0](P)
    return _DEVICE[name]


def _q0(name, n=N, lo=0):
    return np.ascontiguousarray(_kind(name)[2][:, lo:lo + n])


# ---- the cases of tests 2 to 5, and the step size of each -----------------------------------------------------------
# run rows: (PBBI_BETA_ACCEPT, method, masses, kT), all without PBBI_COMPAT_P_FROM_OLDQ
FULL_ROWS = [(b, me, ma, kT) for b in (False, True) for me in METHODS for ma in (False, True) for kT in (1.0, KT)]
# every handle sees non-compat (all four), Stormer-Verlet, masses, and kT != 1 with PBBI_BETA_ACCEPT; the first has all
FOUR_ROWS = [(True, "Stormer-Verlet", True, KT), (False, "Leapfrog", True, 1.0), (True, "Leapfrog", False, KT),
             (False, "Stormer-Verlet", False, 1.0)]
RUN_CASES = [("run", name) + row for name in KINDS for row in (FULL_ROWS if name in FRAMES else FOUR_ROWS)]
ITER_NAMES = ["logistic", "gaussian_sampled", "hier_nc", "softmax"]
ITER_CASES = [("iter", name, b, me) for name in ITER_NAMES for b in (False, True) for me in METHODS]
SMC_NAMES = ["logistic", "negbinomial_held", "hier", "hier_disp_nc", "softmax"]
SMC_BETAS = [0.02, 0.5]
SMC_CASES = [("smc", name, beta) for name in SMC_NAMES for beta in SMC_BETAS]
LADDER_NAMES = ["logistic", "hier_nc", "logistic50", "softmax"]
LADDER_NR = [1, 15, 17, 37, 65]
LADDER_R, LADDER_KT, LADDER_S = 3, 1.7, 4
LADDER_CASES = [("ladder", name, nr) for name in LADDER_NAMES for nr in LADDER_NR]
CANARY_NAMES = ["logistic", "logistic17", "logistic50"]      # D = 5, 17, 50: none a multiple of 16
CANARY_CASES = [("iter", name, False, me) for name in CANARY_NAMES for me in METHODS]   # test 6's iteration is test 3's
ALL_CASES = RUN_CASES + ITER_CASES + [c for c in CANARY_CASES if c not in ITER_CASES] + SMC_CASES + LADDER_CASES

# case -> step size, where the file's own does not give a decisive case (test_frame_cases_are_decisive picked these)
STEP = {
    ('run', 'poisson_full', False, 'Leapfrog', True, 1.0): 0.084,
    ('run', 'negbinomial_held', True, 'Stormer-Verlet', True, 2.5): 0.42,
    ('run', 'negbinomial_held', False, 'Leapfrog', True, 1.0): 0.84,
    ('run', 'hier', False, 'Leapfrog', True, 1.0): 0.28,
    ('run', 'softmax', False, 'Leapfrog', False, 1.0): 0.42,
    ('run', 'softmax', False, 'Leapfrog', True, 1.0): 0.6,
    ('run', 'softmax', True, 'Leapfrog', False, 1.0): 0.42,
    ('run', 'softmax', True, 'Leapfrog', False, 2.5): 0.42,
    ('run', 'softmax', True, 'Leapfrog', True, 1.0): 0.6,
    ('run', 'softmax', True, 'Leapfrog', True, 2.5): 0.42,
    ('run', 'logistic17', False, 'Leapfrog', True, 1.0): 0.56,
    ('run', 'logistic50', True, 'Stormer-Verlet', True, 2.5): 0.175,
    ('run', 'logistic50', False, 'Leapfrog', True, 1.0): 0.5,
    ('run', 'logistic50', True, 'Leapfrog', False, 2.5): 0.35,
    ('run', 'logistic128', False, 'Leapfrog', True, 1.0): 0.56,
    ('iter', 'logistic', False, 'Leapfrog'): 0.63,
    ('iter', 'softmax', False, 'Leapfrog'): 0.6,
    ('iter', 'softmax', True, 'Leapfrog'): 0.6,
    ('iter', 'logistic17', False, 'Leapfrog'): 0.56,
    ('iter', 'logistic50', False, 'Leapfrog'): 0.7,
    ('smc', 'softmax', 0.02): 0.42,
    ('smc', 'softmax', 0.5): 0.42,
    ('ladder', 'logistic50', 1): 0.35,
    ('ladder', 'logistic50', 15): 0.35,
    ('ladder', 'logistic50', 17): 0.35,
    ('ladder', 'logistic50', 37): 0.5,
    ('ladder', 'logistic50', 65): 0.35,
    ('ladder', 'softmax', 1): 0.42,
    ('ladder', 'softmax', 15): 0.42,
    ('ladder', 'softmax', 17): 0.42,
    ('ladder', 'softmax', 37): 0.42,
    ('ladder', 'softmax', 65): 0.42,
}


def _method(case):
    return case[3] if case[0] in ("run", "iter") else "Leapfrog"


def _h(case):
    return STEP.get(case, KINDS[case[1]]["h"][METHODS.index(_method(case))])


def _frozen(**arrays):
    for a in arrays.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def _uniforms(n, chain0, S):
    return np.stack([orc.philox_uniform(SEED, ITER0 + i, chain0, n) for i in range(S)])


@functools.lru_cache(maxsize=None)
def _oracle(case):
    """The oracle's result of a case, computed once and left unchanged: ratio, u, rej (what the decision rests on) and
    the values the device is compared with."""
    name = case[1]
    op, L, h = _kind(name)[1], KINDS[name]["L"], _h(case)
    if case[0] == "run":
        _, _, beta, method, mass, kT = case
        q, m = _q0(name), (MASS if mass else None)
        flags = orc.DRAW_F64 | (orc.BETA_ACCEPT if beta else 0)
        s, p, rej, ratio = orc.hmc_run_philox(op, method, q, m, h, L, S_RUN, SEED, ITER0, CHAIN0, kT, compat=flags)
        return _frozen(samples=s, momenta=p, rej=rej, ratio=ratio, q=q, u=_uniforms(N, CHAIN0, S_RUN))
    if case[0] == "iter":
        _, _, beta, method = case
        kT = KT if beta else 1.0
        q = _q0(name)
        p_in = np.ascontiguousarray(orc.philox_normal(SEED, orc.STREAM_MOMENTUM | orc.STREAM_DRAW_F64, ITER0, CHAIN0,
                                                      q.shape[0], N, np.sqrt(MASS * kT)))
        u = orc.philox_uniform(SEED, ITER0, CHAIN0, N)
        p = p_in.copy()
        ratio, rej = orc.hmc_iter(op, method, q, p, u, MASS, h, L, compat=0, beta=1.0 / kT)
        return _frozen(q=q, p=p, p_in=p_in, rej=rej, ratio=ratio, u=u, kT=kT)
    if case[0] == "smc":
        q = _q0(name)
        s, _, rej, ratio = orc.hmc_run_philox(op, "Leapfrog", q, None, h, L, S_RUN, SEED, ITER0, CHAIN0, 1.0 / case[2],
                                              compat=orc.DRAW_F64 | orc.BETA_ACCEPT, want_momenta=False)
        return _frozen(samples=s, rej=rej, ratio=ratio, q=q, u=_uniforms(N, CHAIN0, S_RUN))
    nr = case[2]
    q = _q0(name, nr, nr)     # rung 1 of the (Dt, 3 nr) array
    s, _, rej, ratio = orc.hmc_run_philox(op, "Leapfrog", q, None, h, L, LADDER_S, SEED, ITER0, nr, LADDER_KT,
                                          compat=orc.DRAW_F64 | orc.BETA_ACCEPT, want_momenta=False)
    return _frozen(samples=s, rej=rej, ratio=ratio, q=q, u=_uniforms(nr, nr, LADDER_S))


def _decisive(tag, ratio, u, rej=None, values=()):
    """The preconditions of a mask comparison, on the oracle's values: everything finite, both outcomes occur (reject
    fraction in [0.1, 0.9]; skipped for the swap decisions, rej = None) and no accept test is closer than 1e-7."""
    assert all(np.all(np.isfinite(v)) for v in (ratio, u) + tuple(values)), tag
    margin = float(np.min(np.abs(ratio - u) / np.maximum(1.0, ratio)))
    frac = None if rej is None else float(np.mean(rej))
    print(f"{tag}: reject fraction {frac}, closest accept test {margin:.2e}")
    assert rej is None or 0.1 <= frac <= 0.9, (tag, frac)
    assert margin >= 1e-7, (tag, margin)


# ---- test 8's ladder and its replay on the oracle --------------------------------------------------------------------
REPLAY = dict(name="logistic", Nr=69, R=3, kT_max=4.0, simulTime=3.0, stepSize=0.4, qStd=1.0, S=2, B=2, k=2)


def _swap_uniform(seed, it, chain):
    """The PBBI_STREAM_SWAP (4) uniform of a chain, from the oracle's Philox block (pbbi_oracle.c rng_block, u53)."""
    x = orc.philox_raw([chain & 0xFFFFFFFF, 0xFFFFFFFF, it & 0xFFFFFFFF, 4 | ((chain >> 32) << 8)],
                       [seed & 0xFFFFFFFF, seed >> 32])
    return float(((x[1] << 32) | x[0]) >> 11) * 2.0 ** -53


def _ladder_replay(q_start):
    """TemperingLadder.run (tempering.py) restated on the oracle from the start `q_start` (D, R Nr): per stretch one
    hmc_run_philox per rung on its columns (chain0 = r Nr, the rung's kT, step size and length), then one exchange
    (even pairs, odd pairs, alternating).  Returns the state, rung 0's recorded samples (D, Nr, S), swapRates,
    acceptRates and the decisions [(tag, ratio, u, rej or None)] the masks rest on."""
    c = REPLAY
    op = _kind(c["name"])[1]
    Nr, R, S, B, k = c["Nr"], c["R"], c["S"], c["B"], c["k"]
    kTs = float(c["kT_max"]) ** (np.arange(R) / (R - 1.0))
    hs = c["stepSize"] * np.sqrt(kTs / kTs[0])
    Ls = [max(1, int(c["simulTime"] / h)) for h in hs]
    q = np.ascontiguousarray(q_start).copy()
    D = q.shape[0]
    rec = np.empty((S, D, Nr))
    n_rej, n_swap, n_tries = np.zeros(R), np.zeros(R - 1), np.zeros(R - 1)
    decisions = []
    it = done = sweep = 0
    total = B + S
    while it < total:
        n = min(k, total - it, (B - it) if it < B else total)
        recording = it >= B
        for r in range(R):
            qr = np.ascontiguousarray(q[:, r * Nr:(r + 1) * Nr])
            s, _, rej, ratio = orc.hmc_run_philox(op, "Leapfrog", qr, None, float(hs[r]), Ls[r], n, SEED, it, r * Nr,
                                                  float(kTs[r]), compat=orc.DRAW_F64 | orc.BETA_ACCEPT, want_momenta=False)
            u = np.stack([orc.philox_uniform(SEED, it + i, r * Nr, Nr) for i in range(n)])
            decisions.append((f"replay it {it} rung {r}", ratio, u, rej))
            assert np.all(np.isfinite(s))
            q[:, r * Nr:(r + 1) * Nr] = qr
            n_rej[r] += rej.sum()
            if recording and r == 0:
                rec[done:done + n] = s
        it += n
        if recording:
            done += n
        parity = sweep & 1
        U = orc.potential(op, q)
        pairs = [(r, lo) for r in range(parity, R - 1, 2) for lo in range(r * Nr, (r + 1) * Nr)]
        sr = np.array([np.exp((1.0 / kTs[r] - 1.0 / kTs[r + 1]) * (U[lo] - U[lo + Nr])) for r, lo in pairs])
        su = np.array([_swap_uniform(SEED, sweep, lo) for _, lo in pairs])
        decisions.append((f"replay sweep {sweep}", sr, su, None))
        sw = orc.replica_exchange(op, q, Nr, R, 1.0 / kTs, parity, SEED, sweep, 0)
        assert np.array_equal(sw[parity:R - 1:2].ravel(), su < sr), "the swap uniforms are not the oracle's"
        n_swap += sw.sum(axis=1)
        n_tries[parity:R - 1:2] += Nr
        sweep += 1
    return (q, np.ascontiguousarray(rec.transpose(1, 2, 0)), n_swap / np.maximum(n_tries, 1),
            1.0 - n_rej / (total * Nr), decisions, (kTs, hs, Ls))


def _check_replay_decisions(decisions):
    rejs = [d[3] for d in decisions if d[3] is not None]
    for tag, ratio, u, rej in decisions:
        _decisive(tag, ratio, u, None)
    frac = float(np.mean(np.concatenate([r.ravel() for r in rejs])))
    assert 0.1 <= frac <= 0.9, frac


# ---- test 1: CPU -----------------------------------------------------------------------------------------------------
def test_frame_cases_are_decisive():
    """The oracle alone, for every case of tests 2 to 5 and the ladder of test 8: every value finite, the reject
    fraction in [0.1, 0.9] and min |ratio - u| >= 1e-7 max(1, ratio) over all chains and iterations.  Given these,
    "reject masks are equal" is a fair demand on the device at 1e-10 and no chain is ever excluded."""
    for case in ALL_CASES:
        o = _oracle(case)
        _decisive(str(case), o["ratio"], o["u"], o["rej"], [v for k, v in o.items() if k in ("samples", "momenta", "q", "p")])
    c = REPLAY
    start = orc.philox_normal(SEED, orc.STREAM_POSITION, 0, 0, _kind(c["name"])[2].shape[0], c["R"] * c["Nr"], c["qStd"])
    decisions = _ladder_replay(start)[4]
    assert sum(d[3] is None for d in decisions) == 2 and len(decisions) == 2 * (c["R"] + 1)
    _check_replay_decisions(decisions)


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def P():
    import physicsbasedbayesianinference_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def lib():
    from physicsbasedbayesianinference_amd import _lib
    _lib.load()
    return _lib


def _dev():
    from physicsbasedbayesianinference_amd import _device
    return _device


POISON = 7.25


def _device_run(lib, pot, method, q0, m, h, L, S, flags, kT, chain0=CHAIN0, pad=0, iter0=ITER0):
    """pbbi_hmc_run with all four outputs from q0 (Dt, n), the state with `pad` extra columns of leading stride.
    Returns samples, momenta, reject, ratio, the final state and its padding columns."""
    import torch
    d = _dev()
    Dt, n = q0.shape
    qd = torch.full((Dt, n + pad), POISON, dtype=torch.float64, device="cuda:0")
    qd[:, :n] = d.as_device(q0, 0, np.float64)
    md = d.as_device(m, 0, np.float64) if m is not None else None
    samples, momenta = d.empty((S, Dt, n), np.float64, 0), d.empty((S, Dt, n), np.float64, 0)
    reject, ratio = d.empty((S, n), np.uint8, 0), d.empty((S, n), np.float64, 0)
    lib.call("pbbi_hmc_run", pot.handle, orc.METHODS[method], qd.data_ptr(), md.data_ptr() if md is not None else None,
             samples.data_ptr(), momenta.data_ptr(), reject.data_ptr(), ratio.data_ptr(), n, n + pad, float(h), int(L), S,
             flags, SEED, iter0, chain0, float(kT), d.stream_ptr(0))
    torch.cuda.synchronize()
    return (d.to_numpy(samples), d.to_numpy(momenta), d.to_numpy(reject).astype(bool), d.to_numpy(ratio),
            qd[:, :n].contiguous().cpu().numpy(), qd[:, n:].contiguous().cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(KINDS))
def test_frame_run_flags_vs_oracle(P, lib, name):
    """pbbi_hmc_run against oracle.hmc_run_philox, S = 3, PBBI_DRAW_F64, all four outputs, leading stride N + 5, never
    PBBI_COMPAT_P_FROM_OLDQ: the full product {0, PBBI_BETA_ACCEPT} x {Leapfrog, Stormer-Verlet} x {no masses, MASS} x
    kT {1, 2.5} on one handle of each twin, FOUR_ROWS on every other handle.  Masks equal; samples, momenta, ratio and
    the final state within TOL; the padding columns unchanged.  On the oracle's side a rejected chain's recorded
    momentum is its Philox draw times sqrt(m kT) -- the parked-draw rule, checked rather than repeated."""
    pot, L = _pot(P, name), KINDS[name]["L"]
    n_rej = 0
    for case in (c for c in RUN_CASES if c[1] == name):
        _, _, beta, method, mass, kT = case
        o = _oracle(case)
        _decisive(str(case), o["ratio"], o["u"], o["rej"])
        m = MASS if mass else None
        Dt = o["q"].shape[0]
        for i in range(S_RUN):     # the parked draw, from the oracle's generator
            z = orc.philox_normal(SEED, orc.STREAM_MOMENTUM | orc.STREAM_DRAW_F64, ITER0 + i, CHAIN0, Dt, N,
                                  np.sqrt((MASS if mass else np.ones(N)) * kT))
            rj = o["rej"][i]
            assert np.array_equal(o["momenta"][i][:, rj], z[:, rj]), case
            assert not np.any(np.all(o["momenta"][i][:, ~rj] == z[:, ~rj], axis=0)), case
        flags = lib.DRAW_F64 | (lib.BETA_ACCEPT if beta else 0)
        gs, gm, grej, gratio, gq, gpad = _device_run(lib, pot, method, _q0(name), m, _h(case), L, S_RUN, flags, kT, pad=5)
        tag = f"{name} beta_accept={beta} {method} mass={mass} kT={kT}"
        print(tag, "mask mismatches", int((grej != o["rej"]).sum()))
        assert np.array_equal(grej, o["rej"]), tag
        check(tag + " samples", gs, o["samples"])
        check(tag + " momenta", gm, o["momenta"])
        check(tag + " ratio", gratio, o["ratio"])
        check(tag + " final state", gq, o["q"])
        assert gpad.shape == (Dt, 5) and np.all(gpad == POISON), tag
        n_rej += int(grej.sum())
    assert n_rej > 0


def _device_iter(lib, pot, method, q, p, u, m, h, L, flags, kT, outputs=True):
    """pbbi_hmc_iter (kT = 1) / pbbi_hmc_iter_kt on host arrays; without `outputs` p_out, ratio_out and reject_out are
    NULL.  Returns q_out, p_out, ratio, reject."""
    import torch
    d = _dev()
    Dt, n = q.shape
    qd, pd, ud = (d.as_device(np.array(a), 0, np.float64) for a in (q, p, u))     # (the oracle's arrays are read-only)
    md = d.as_device(m, 0, np.float64) if m is not None else None
    qo, po = d.empty((Dt, n), np.float64, 0), d.empty((Dt, n), np.float64, 0)
    ro, rj = d.empty((n,), np.float64, 0), d.empty((n,), np.uint8, 0)
    args = [pot.handle, orc.METHODS[method], qd.data_ptr(), pd.data_ptr(), ud.data_ptr(),
            md.data_ptr() if md is not None else None, qo.data_ptr(),
            po.data_ptr() if outputs else None, ro.data_ptr() if outputs else None, rj.data_ptr() if outputs else None,
            n, n, float(h), int(L)]
    if kT == 1.0:
        lib.call("pbbi_hmc_iter", *args, flags, d.stream_ptr(0))
    else:
        lib.call("pbbi_hmc_iter_kt", *args, flags, float(kT), d.stream_ptr(0))
    torch.cuda.synchronize()
    if not outputs:
        return d.to_numpy(qo), None, None, None
    return d.to_numpy(qo), d.to_numpy(po), d.to_numpy(ro), d.to_numpy(rj).astype(bool)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ITER_NAMES)
def test_frame_uploaded_noncompat_vs_oracle(P, lib, name):
    """pbbi_hmc_iter with flags = 0 and pbbi_hmc_iter_kt with PBBI_BETA_ACCEPT at kT = 2.5, both methods, with masses,
    uploaded momenta (the oracle's double-precision draw times sqrt(m kT)) and uniforms, against oracle.hmc_iter(...,
    compat=0, beta=1/kT): masks equal, q, p, ratio within TOL, and a rejected chain's p_out is its p_in, bit for bit.
    A second call without p_out, ratio_out and reject_out gives the same q_out bit for bit."""
    pot, L = _pot(P, name), KINDS[name]["L"]
    for case in (c for c in ITER_CASES if c[1] == name):
        _, _, beta, method = case
        o = _oracle(case)
        _decisive(str(case), o["ratio"], o["u"], o["rej"])
        rj = o["rej"]
        assert np.array_equal(o["p"][:, rj], o["p_in"][:, rj]) and np.array_equal(o["q"][:, rj], _q0(name)[:, rj])
        flags = lib.BETA_ACCEPT if beta else 0
        gq, gp, gratio, grej = _device_iter(lib, pot, method, _q0(name), o["p_in"], o["u"], MASS, _h(case), L, flags, o["kT"])
        tag = f"{name} beta_accept={beta} {method}"
        print(tag, "mask mismatches", int((grej != rj).sum()))
        assert np.array_equal(grej, rj), tag
        check(tag + " q", gq, o["q"])
        check(tag + " p", gp, o["p"])
        check(tag + " ratio", gratio, o["ratio"])
        assert np.array_equal(gp[:, rj], o["p_in"][:, rj]), tag
        assert np.array_equal(gq[:, rj], _q0(name)[:, rj]), tag
        q_only = _device_iter(lib, pot, method, _q0(name), o["p_in"], o["u"], MASS, _h(case), L, flags, o["kT"], outputs=False)[0]
        assert np.array_equal(q_only, gq), tag


@pytest.mark.gpu
@pytest.mark.parametrize("name", SMC_NAMES)
def test_frame_smc_shaped_call_vs_oracle(P, lib, name):
    """The call of smc.TemperedSMC._stages: samples, momenta and ratio NULL, only reject, in place on a state of leading
    stride N, PBBI_BETA_ACCEPT | PBBI_DRAW_F64, kT = 1 / beta for beta = 0.02 and 0.5, three moves.  The final state
    (TOL) and the masks are oracle.hmc_run_philox's."""
    import torch
    d = _dev()
    pot, L = _pot(P, name), KINDS[name]["L"]
    for case in (c for c in SMC_CASES if c[1] == name):
        o = _oracle(case)
        _decisive(str(case), o["ratio"], o["u"], o["rej"])
        qd = d.as_device(_q0(name), 0, np.float64)
        reject = d.empty((S_RUN, N), np.uint8, 0)
        lib.call("pbbi_hmc_run", pot.handle, lib.LEAPFROG, qd.data_ptr(), None, None, None, reject.data_ptr(), None, N, N,
                 _h(case), L, S_RUN, lib.BETA_ACCEPT | lib.DRAW_F64, SEED, ITER0, CHAIN0, 1.0 / case[2], d.stream_ptr(0))
        torch.cuda.synchronize()
        grej = d.to_numpy(reject).astype(bool)
        print(case, "mask mismatches", int((grej != o["rej"]).sum()))
        assert np.array_equal(grej, o["rej"]), case
        check(f"{case} final state", d.to_numpy(qd), o["q"])


@pytest.mark.gpu
@pytest.mark.parametrize("nr", LADDER_NR)
@pytest.mark.parametrize("name", LADDER_NAMES)
def test_frame_ladder_shaped_call_vs_oracle(P, lib, name, nr):
    """One (Dt, 3 Nr) device array, the layout of tempering.TemperingLadder; only rung 1 is run, the way run() runs it:
    the pointer advanced by Nr elements, N = Nr, leading stride 3 Nr, chain0 = Nr, kT = 1.7, its flags
    (PBBI_BETA_ACCEPT | PBBI_KDK_FMA, with PBBI_DRAW_F64), samples and reject only.  Nr = 1, 15, 17, 37, 65: a base
    that is not 16-chain aligned, every class of tail length, fewer chains than a tile -- the clamped tail of rung 1
    lies against live columns of rung 2.  Rung 1 and its samples are the oracle's, rungs 0 and 2 are bit-unchanged."""
    import torch
    d = _dev()
    case = ("ladder", name, nr)
    o = _oracle(case)
    _decisive(str(case), o["ratio"], o["u"], o["rej"])
    pot, L = _pot(P, name), KINDS[name]["L"]
    q_all = _q0(name, LADDER_R * nr)
    Dt = q_all.shape[0]
    qd = d.as_device(q_all, 0, np.float64)
    samples, reject = d.empty((LADDER_S, Dt, nr), np.float64, 0), d.empty((LADDER_S, nr), np.uint8, 0)
    lib.call("pbbi_hmc_run", pot.handle, lib.LEAPFROG, qd.data_ptr() + nr * 8, None, samples.data_ptr(), None,
             reject.data_ptr(), None, nr, LADDER_R * nr, _h(case), L, LADDER_S,
             lib.BETA_ACCEPT | lib.KDK_FMA | lib.DRAW_F64, SEED, ITER0, nr, LADDER_KT, d.stream_ptr(0))
    torch.cuda.synchronize()
    gq, grej = d.to_numpy(qd), d.to_numpy(reject).astype(bool)
    assert np.array_equal(grej, o["rej"])
    check("samples", d.to_numpy(samples), o["samples"])
    check("rung 1", gq[:, nr:2 * nr], o["q"])
    assert np.array_equal(gq[:, :nr], q_all[:, :nr]) and np.array_equal(gq[:, 2 * nr:], q_all[:, 2 * nr:])


CANARY_ROWS = 18


def _canary(arr, ldn):
    """A (Dt + 18, ldn) device allocation of NaN with `arr` (Dt, n), or nothing, in rows [1, 1 + Dt); returns the
    tensor and the pointer of row 1."""
    import torch
    Dt, n = arr.shape
    t = torch.full((Dt + CANARY_ROWS, ldn), float("nan"), dtype=torch.float64, device="cuda:0")
    t[1:1 + Dt, :n] = torch.from_numpy(np.array(arr)).to("cuda:0")
    return t, t.data_ptr() + ldn * 8


def _canary_result(t, Dt, n, written=True):
    """The (Dt, n) block of a canary allocation, after asserting that every other element is still the NaN it was."""
    import torch
    nan_bits = torch.full((1,), float("nan"), dtype=torch.float64).view(torch.int64).item()
    bits = t.view(torch.int64).cpu().numpy().copy()
    block = t[1:1 + Dt, :n].cpu().numpy().copy()
    if written:
        bits[1:1 + Dt, :n] = nan_bits
    assert np.all(bits == nan_bits), "a store outside the state"
    return block


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("name", CANARY_NAMES)
def test_frame_state_inside_a_canary_allocation(P, lib, name, pad):
    """pbbi_potential_eval with the gradient, pbbi_integrate with v_out and one pbbi_hmc_iter (flags = 0, masses) whose
    state, momentum and output arrays are rows [1, 1 + D) of (D + 18, ldn) allocations full of NaN, D = 5, 17, 50 (none a
    multiple of 16), ldn = N and N + 5.  The bounded descriptors promise that a padded row d >= D loads 0 and that its
    store is dropped: a load that was not clipped shows as NaN in a result (all are compared with the oracle at TOL), a
    store that was not dropped shows in the canary (every element outside the block keeps its NaN bit pattern).  All
    accesses stay inside the test's own allocations."""
    import torch
    d = _dev()
    pot, op, L = _pot(P, name), _kind(name)[1], KINDS[name]["L"]
    q0 = _q0(name)
    Dt, ldn = q0.shape[0], N + pad
    empty_block = np.full((Dt, N), np.nan)
    md = d.as_device(MASS, 0, np.float64)
    st = d.stream_ptr(0)
    # evaluation
    Uo, go = orc.potential(op, q0, want_grad=True)
    (qt, qp), (gt, gp) = _canary(q0, ldn), _canary(empty_block, ldn)
    U = d.empty((N,), np.float64, 0)
    lib.call("pbbi_potential_eval", pot.handle, qp, N, ldn, U.data_ptr(), gp, st)
    torch.cuda.synchronize()
    check("U", d.to_numpy(U), Uo)
    check("gradient", _canary_result(gt, Dt, N), go)
    assert np.array_equal(_canary_result(qt, Dt, N), q0)
    for method in METHODS:
        case = ("iter", name, False, method)
        o, h = _oracle(case), _h(case)
        _decisive(str(case), o["ratio"], o["u"], o["rej"])
        p0, u = o["p_in"], o["u"]
        # integration, in place
        q, p = q0.copy(), p0.copy()
        v = orc.integrate(op, method, q, p, MASS, h, L)
        (qt, qp), (pt, pp), (vt, vp) = _canary(q0, ldn), _canary(p0, ldn), _canary(empty_block, ldn)
        lib.call("pbbi_integrate", pot.handle, orc.METHODS[method], qp, pp, md.data_ptr(), vp, N, ldn, h, L, st)
        torch.cuda.synchronize()
        check(method + " integrate q", _canary_result(qt, Dt, N), q)
        check(method + " integrate p", _canary_result(pt, Dt, N), p)
        check(method + " integrate v", _canary_result(vt, Dt, N), v)
        # one iteration
        q, p, ratio, rej = o["q"], o["p"], o["ratio"], o["rej"]
        (qt, qp), (pt, pp) = _canary(q0, ldn), _canary(p0, ldn)
        (qot, qop), (pot_, pop) = _canary(empty_block, ldn), _canary(empty_block, ldn)
        ud, ro, rj = d.as_device(np.array(u), 0, np.float64), d.empty((N,), np.float64, 0), d.empty((N,), np.uint8, 0)
        lib.call("pbbi_hmc_iter", pot.handle, orc.METHODS[method], qp, pp, ud.data_ptr(), md.data_ptr(), qop, pop,
                 ro.data_ptr(), rj.data_ptr(), N, ldn, h, L, 0, st)
        torch.cuda.synchronize()
        assert np.array_equal(d.to_numpy(rj).astype(bool), rej), method
        check(method + " iter q", _canary_result(qot, Dt, N), q)
        check(method + " iter p", _canary_result(pot_, Dt, N), p)
        check(method + " iter ratio", d.to_numpy(ro), ratio)
        assert np.array_equal(_canary_result(qt, Dt, N), q0) and np.array_equal(_canary_result(pt, Dt, N), p0)


# handle -> Leapfrog step size at which the host mirror of the single-precision draw rejects 9 % .. 76 % in both settings
F32_H = {"logistic17": 0.56, "logistic50": 0.6, "logistic128": 0.45, "hier": 0.28}


@pytest.mark.gpu
@pytest.mark.parametrize("mass,kT", [(True, 1.0), (False, KT)], ids=["mass", "kT2.5"])
@pytest.mark.parametrize("name", list(F32_H))
def test_frame_single_precision_draw_is_mapped_row_for_row(P, lib, name, mass, kT):
    """k_glm's counterpart of test_softmax_single_precision_draw_is_mapped_row_for_row at NT = 2, 4, 8 (and NT = 1 on
    the hierarchical handle): one pbbi_hmc_run of S = 1 WITHOUT PBBI_DRAW_F64 equals, bit for bit, one pbbi_hmc_iter(_kt)
    fed with pbbi_philox_normal(momentum stream, single precision) times sqrt(m kT) and pbbi_philox_uniform for the same
    counters -- q, p, ratio and mask; non-compat, so a rejected chain reports the drawn momentum itself.  Device against
    device: the kernel's block index (k << 2) | g is the draw of a (Dt, N) state."""
    from test_gpu_parity import device_normal, device_uniform
    pot, L = _pot(P, name), KINDS[name]["L"]
    q0 = _q0(name)
    Dt = q0.shape[0]
    m = MASS if mass else None
    h = F32_H[name]
    z = device_normal(lib, SEED, lib.STREAM_MOMENTUM, ITER0, CHAIN0, Dt, N)
    assert np.array_equal(z, z.astype(np.float32)), "not the single-precision draw"
    p_in = np.ascontiguousarray(z * np.sqrt((MASS if mass else 1.0) * kT))
    u = device_uniform(lib, SEED, ITER0, CHAIN0, N)
    flags = lib.BETA_ACCEPT if kT != 1.0 else 0
    gs, gm, grej, gratio, gq, _ = _device_run(lib, pot, "Leapfrog", q0, m, h, L, 1, flags, kT)
    iq, ip, iratio, irej = _device_iter(lib, pot, "Leapfrog", q0, p_in, u, m, h, L, flags, kT)
    assert np.array_equal(grej[0], irej)
    assert 0 < irej.sum() < N
    assert np.array_equal(gs[0], iq) and np.array_equal(gq, iq)
    assert np.array_equal(gm[0], ip)
    assert np.array_equal(gratio[0], iratio)
    assert np.array_equal(gm[0][:, irej], p_in[:, irej])


@pytest.mark.gpu
def test_frame_ladder_replayed_on_the_oracle(P, lib):
    """TemperingLadder(GLM, kTs = geometric_ladder(4, 3), 69 chains per rung, draw_f64=True).run(numSamples=2, burn_in=2,
    swap_every=2) replayed with oracle.hmc_run_philox per rung and oracle.replica_exchange: the state and the recorded
    samples within TOL, swapRates and acceptRates equal.  The start is the one draw the replay takes from the device
    (run() draws it in single precision, which the host mirrors to 5e-6 only): pbbi_philox_normal with run()'s own
    arguments.  Every accept and swap decision of the replay is at least 1e-7 from a tie."""
    from physicsbasedbayesianinference_amd.tempering import TemperingLadder, geometric_ladder
    from test_gpu_parity import device_normal
    c = REPLAY
    pot = _pot(P, c["name"])
    D = pot.numDimensions
    ladder = TemperingLadder(pot, D, c["Nr"], geometric_ladder(c["kT_max"], c["R"]), c["simulTime"], c["stepSize"],
                             seed=SEED, draw_f64=True)
    got = ladder.run(numSamples=c["S"], qStd=c["qStd"], burn_in=c["B"], swap_every=c["k"])
    start = device_normal(lib, SEED, lib.STREAM_POSITION, 0, 0, D, c["R"] * c["Nr"], c["qStd"])
    state, rec, swap_rates, accept_rates, decisions, (kTs, hs, Ls) = _ladder_replay(start)
    assert np.array_equal(ladder.kTs, kTs) and np.array_equal(ladder.stepSizes, hs) and list(ladder.numSteps) == Ls
    _check_replay_decisions(decisions)
    print("accept rates", accept_rates, "swap rates", swap_rates)
    check("state", _dev().to_numpy(ladder.state), state)
    check("samples", np.asarray(got), rec)
    assert np.array_equal(ladder.swapRates, swap_rates)
    assert np.array_equal(ladder.acceptRates, accept_rates)
