"""Ordinal (cumulative-logit) regression, glm.OrdinalGLM (PBBI_GLM_ORDINAL = 6 of k_glm<NT, FAM, true>), the part that needs no
GPU: the header and the library, the packer, the refusals, the class's layout, and the yardstick the GPU tests of
test_glm_ordinal.py are held to.  Categories y_i in {0 .. K-1}, cutpoints kappa_1 < .. < kappa_{K-1}, kappa_0 = -inf, kappa_K =
+inf, the chain's state [w (D); zeta (K - 1)] with zeta_1 = kappa_1 and zeta_j = log(kappa_j - kappa_{j-1}):

    P(y_i = k) = sigma(kappa_{k+1} - eta_i) - sigma(kappa_k - eta_i)                       eta_i = x_i . w + o_i
    U = -sum_i a_i log P(y_i) + 0.5 sum_s lam_s (state_s - mu_s)^2          (all D + K - 1 rows; the prior is stated on zeta)

The oracle side is the user-source mechanism of test_glm_model.py, `orc.pot_custom(complete_source(SOURCE), Dt, prm)`, with
this file's own C++ statement of the model in the NATURAL form above -- the logarithm of a difference of two sigmoids (mirrored
in the upper tail, where both round to 1: the same difference, and without it the yardstick itself is off by up to 5e-5 in U
where the sampling cases go), rows of weight 0 skipped by a branch: prm = [M, K, X.ravel(), a, y, o, lam(Dt), mu(Dt)].  The kernels form U_i from two softplus
terms and -log(1 - exp(-Delta_k)) instead; nothing of that algebra is restated here.

The data: weights from {0, 0.5, 1, 3} with at least one 0, offsets ~ N(0, 0.3), lam from {0, 0.5, 4} over all D + K - 1 rows
with lam_0 = 0, y drawn from the model; for K >= 3 one interior-or-edge category is emptied (its observations moved to a
neighbour), so A_k = 0 occurs.  (K = 2 keeps both categories: with one empty the response would be constant.)

The sampling cases of test_glm_ordinal.py live here, so that test_ordinal_sampling_cases_are_decisive runs every one of them on
the oracle alone: step sizes and seeds were chosen on the CPU so that the reject fraction lies in [0.1, 0.9] and no accept
test is closer than 1e-8.
"""
import ctypes as C
import functools
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import test_glm_frame as F
import test_glm_metric as t_metric
from oracle import oracle as orc
from test_glm_model import decisive, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
MAX_DIM = 64      # the state dimension glm_max_dim(GLM_V_ORDINAL, PBBI_GLM_ORDINAL) states (profiles/glm_ordinal_resources.txt)

SOURCE = """
PBBI_FN T og_sig(T x) { return x >= 0 ? T(1) / (T(1) + exp(-x)) : exp(x) / (T(1) + exp(x)); }
// P(y = k) = sigma(hi) - sigma(lo), hi = kappa_{k+1} - eta, lo = kappa_k - eta: taken as it stands in the lower tail and as the
// same difference mirrored, sigma(-lo) - sigma(-hi), in the upper one, where both sigmoids round to 1 and their difference is lost
PBBI_FN T og_prob(int k, int K, T hi, T lo) {
    if (k == 0) return og_sig(hi);
    if (k == K - 1) return og_sig(-lo);
    return hi + lo <= 0 ? og_sig(hi) - og_sig(lo) : og_sig(-lo) - og_sig(-hi);
}
template <class Q>
PBBI_FN T potential(const Q& q, int DT, const T* prm) {
    const int M = (int)prm[0], K = (int)prm[1];
    const int D = DT - (K - 1);
    const T* X = prm + 2;
    const T* a = X + (long)M * D;
    const T* y = a + M;
    const T* o = y + M;
    const T* lam = o + M;
    const T* mu = lam + DT;
    T kap[8];
    kap[0] = q[D];
    for (int j = 1; j < K - 1; ++j) kap[j] = kap[j - 1] + exp(q[D + j]);
    T s = 0;
    for (int i = 0; i < M; ++i) {
        if (a[i] == 0) continue;                // weight 0: the row is not there
        T e = o[i];
        for (int j = 0; j < D; ++j) e += X[i * D + j] * q[j];
        const int k = (int)y[i];
        s -= a[i] * log(og_prob(k, K, k < K - 1 ? kap[k] - e : T(0), k > 0 ? kap[k - 1] - e : T(0)));
    }
    T r = 0;
    for (int j = 0; j < DT; ++j) r += lam[j] * (q[j] - mu[j]) * (q[j] - mu[j]);
    return s + T(0.5) * r;
}
template <class Q, class G>
PBBI_FN void gradient(const Q& q, G& g, int DT, const T* prm) {
    const int M = (int)prm[0], K = (int)prm[1];
    const int D = DT - (K - 1);
    const T* X = prm + 2;
    const T* a = X + (long)M * D;
    const T* y = a + M;
    const T* o = y + M;
    const T* lam = o + M;
    const T* mu = lam + DT;
    T kap[8], gk[8];
    kap[0] = q[D];
    for (int j = 1; j < K - 1; ++j) kap[j] = kap[j - 1] + exp(q[D + j]);
    for (int j = 0; j < 8; ++j) gk[j] = 0;
    for (int j = 0; j < DT; ++j) g[j] = lam[j] * (q[j] - mu[j]);
    for (int i = 0; i < M; ++i) {
        if (a[i] == 0) continue;
        T e = o[i];
        for (int j = 0; j < D; ++j) e += X[i * D + j] * q[j];
        const int k = (int)y[i];
        const T hi = k < K - 1 ? kap[k] - e : T(0), lo = k > 0 ? kap[k - 1] - e : T(0);
        const T P = og_prob(k, K, hi, lo);
        const T dhi = k < K - 1 ? og_sig(hi) * og_sig(-hi) : T(0);   // the logistic density at the two cutpoints
        const T dlo = k > 0 ? og_sig(lo) * og_sig(-lo) : T(0);
        const T w = a[i] * (dhi - dlo) / P;                          // dU_i / deta
        for (int j = 0; j < D; ++j) g[j] += w * X[i * D + j];
        if (k < K - 1) gk[k] -= a[i] * dhi / P;                      // dU_i / dkappa_{k+1}
        if (k > 0) gk[k - 1] += a[i] * dlo / P;                      // dU_i / dkappa_k
    }
    T suffix = 0;
    for (int j = K - 2; j >= 0; --j) {                               // kappa_m depends on zeta_1 and on every gap up to m
        suffix += gk[j];
        g[D + j] += j == 0 ? suffix : exp(q[D + j]) * suffix;
    }
}
"""


def problem(M, D, K, seed, empty=True):
    """The data of every ordinal test.  Returns the keyword arguments of OrdinalGLM, the true (w, zeta) and the generator."""
    rs = np.random.RandomState(seed)
    X = rs.standard_normal((M, D)) / np.sqrt(D)
    w = 0.7 * rs.standard_normal(D)
    zeta = np.r_[rs.uniform(-1.5, -0.5), rs.normal(-0.2, 0.3, K - 2)]
    kappa = np.cumsum(np.r_[zeta[0], np.exp(zeta[1:])])
    a = rs.choice([0.0, 0.5, 1.0, 3.0], size=M)
    if M > 1:
        a[rs.randint(M)] = 0.0
    else:
        a[:] = 3.0
    o = 0.3 * rs.standard_normal(M)
    eta = X @ w + o
    y = (rs.logistic(size=M) + eta)[:, None] > kappa[None, :]
    y = y.sum(axis=1).astype(np.float64)
    if empty and K >= 3:
        gone = float(rs.randint(K))
        y[y == gone] = gone - 1.0 if gone > 0 else 1.0
    lam = rs.choice([0.0, 0.5, 4.0], size=D + K - 1)
    lam[0] = 0.0
    mu = np.r_[0.5 * rs.standard_normal(D), zeta + 0.3 * rs.standard_normal(K - 1)]
    kw = dict(X=X, y=y, categories=K, weights=a, offset=o, prior_precision=lam[:D], prior_mean=mu[:D],
              cutpoint_prior=np.c_[mu[D:], lam[D:]])
    return kw, w, zeta, rs


def start(w, zeta, N, rs, spread=0.3):
    """(D + K - 1, N) states around (w, zeta)."""
    c = np.r_[w, zeta]
    return np.ascontiguousarray(c[:, None] + spread * rs.standard_normal((c.size, N)))


def make(P, kw):
    return P.OrdinalGLM(**kw)


def table(kw):
    """(lam, mu) over the D + K - 1 rows of the state."""
    cp = np.asarray(kw["cutpoint_prior"], dtype=np.float64)
    return np.r_[kw["prior_precision"], cp[:, 1]], np.r_[kw["prior_mean"], cp[:, 0]]


def oracle_pot(kw, keep=None):
    """The oracle's potential of the data `kw`; keep = a row mask."""
    from physicsbasedbayesianinference_amd import custom
    X, y, K = kw["X"], kw["y"], kw["categories"]
    M, D = X.shape
    a = np.ones(M) if kw.get("weights") is None else kw["weights"]
    o = np.zeros(M) if kw.get("offset") is None else kw["offset"]
    if keep is not None:
        X, y, a, o = X[keep], y[keep], a[keep], o[keep]
    lam, mu = table(kw)
    prm = np.concatenate([[float(X.shape[0]), float(K)], X.ravel(), a, y, o, lam, mu])
    return orc.pot_custom(custom.complete_source(SOURCE), D + K - 1, prm)


def probabilities(kw, W):
    """(P(y_i | draw t) (M, T), expected category (M, T)) in longdouble from the category probabilities of the draws W (Dt, T)."""
    X, y, K = kw["X"].astype(LD), kw["y"].astype(int), kw["categories"]
    M, D = X.shape
    o = np.zeros(M, LD) if kw.get("offset") is None else kw["offset"].astype(LD)
    Wl = np.asarray(W).astype(LD)
    eta = X @ Wl[:D] + o[:, None]
    kappa = np.cumsum(np.concatenate([Wl[D:D + 1], np.exp(Wl[D + 1:D + K - 1])], axis=0), axis=0)       # (K - 1, T)
    cdf = np.ones((K + 1,) + eta.shape, LD)                      # cdf[k] = P(y < k): 0, sigma(kappa_1 - eta), .., 1
    cdf[0] = 0
    for j in range(K - 1):
        cdf[j + 1] = 1 / (1 + np.exp(-(kappa[j][None, :] - eta)))
    pk = np.diff(cdf, axis=0)                                     # (K, M, T)
    mean = sum(k * pk[k] for k in range(K))
    return np.take_along_axis(pk, y[None, :, None], axis=0)[0], mean


def numpy_U(kw, q):
    a = np.ones(kw["y"].size) if kw.get("weights") is None else kw["weights"]
    p, _ = probabilities(kw, q)
    lam, mu = table(kw)
    lik = -(a[:, None].astype(LD) * np.where(a[:, None] == 0, 0, np.log(p))).sum(axis=0)
    return lik + LD(0.5) * (lam[:, None].astype(LD) * (q.astype(LD) - mu[:, None].astype(LD)) ** 2).sum(axis=0)


# ---- the sampling cases of test_glm_ordinal.py: inputs and oracle sides, computed once and left unchanged ------------------
# M, D, K, h (Leapfrog: without, with per-chain masses), h (Stormer-Verlet: likewise), L -- N = 303, kT = 1 and ITER_KT.  The
# step is held where the ORACLE is accurate: its natural form loses the difference of two sigmoids where a trajectory takes an
# interior category's probability far down (up to 1e-8 in U at kT = 2 and the steps that reject half the chains), so the
# temperature is modest and the heavier chains, which move less, take a larger step to reject at all.
ITER_CASES = [(40, 5, 5, (0.14, 0.14), (0.08, 0.08), 8), (203, 16, 8, (0.125, 0.135), (0.08, 0.08), 8)]
ITER_KT = 1.25
ORACLE_TOL = 1e-13    # the oracle's own U against longdouble NumPy where the cases end up: a thousandth of the tests' TOL
# M, D, K, N, h, L -- S = 6; the last is the largest shipped state dimension
RUN_CASES = [(203, 16, 8, 300, 0.05, 8), (203, MAX_DIM - 4, 5, 100, 0.15, 6)]
RUN_SEED, RUN_ITER0, RUN_CHAIN0, RUN_S = 17, 3, 1000003, 6
# (D, K): M, (h Leapfrog, h Stormer-Verlet), L of the metric's cases (N, masses, kT and counters are test_glm_frame's)
METRIC_CASES = {(5, 5): (40, (0.7, 0.3), 8), (16, 8): (203, (0.5, 0.2), 8)}
METRIC_ROWS = [("Leapfrog", True, False), ("Stormer-Verlet", False, True)]     # (method, PBBI_BETA_ACCEPT, compat)
UNIT_H = 0.3      # ... times these steps where the same handle runs with the unit metric


def iter_inputs(M, D, K, mass, kt):
    kw, w, zeta, rs = problem(M, D, K, 11)
    N = 303
    kT = ITER_KT if kt else 1.0
    m = 1.0 + (np.arange(N) % 3) * 0.5 if mass else None
    q = start(w, zeta, N, rs, spread=0.1)
    p = np.ascontiguousarray(rs.standard_normal((D + K - 1, N)) * np.sqrt((m if mass else 1.0) * kT))
    u = rs.uniform(size=N)
    return kw, N, kT, m, q, p, u


@functools.lru_cache(maxsize=None)
def iter_oracle(M, D, K, h, L, method, mass, kt):
    kw, N, kT, m, q, p, u = iter_inputs(M, D, K, mass, kt)
    r_o, rej_o = orc.hmc_iter(oracle_pot(kw), method, q, p, u, m, h, L, beta=1.0 / kT)
    return F._frozen(q=q, p=p, ratio=r_o, rej=rej_o, u=u)


def iter_step(method, mass, h_lf, h_sv):
    return (h_lf if method == "Leapfrog" else h_sv)[int(mass)]


def oracle_accuracy(kw, q):
    """The oracle's U at the states q against the longdouble NumPy evaluation, relative to max(1, |U|)."""
    U, Un = orc.potential(oracle_pot(kw), np.ascontiguousarray(q)), numpy_U(kw, q)
    assert np.all(np.isfinite(U))
    return float(np.max(np.abs(U - Un) / np.maximum(1.0, np.abs(Un))))


def run_inputs(M, D, K, N):
    kw, w, zeta, rs = problem(M, D, K, 21)
    return kw, start(w, zeta, N, rs, spread=0.1)


@functools.lru_cache(maxsize=None)
def run_oracle(M, D, K, N, h, L):
    kw, q = run_inputs(M, D, K, N)
    so, mo, rejo, ro = orc.hmc_run_philox(oracle_pot(kw), "Leapfrog", q, None, h, L, RUN_S, RUN_SEED, RUN_ITER0, RUN_CHAIN0, 1.0,
                                          compat=orc.COMPAT_P_FROM_OLDQ | orc.DRAW_F64)
    u = np.stack([orc.philox_uniform(RUN_SEED, RUN_ITER0 + i, RUN_CHAIN0, N) for i in range(RUN_S)])
    return F._frozen(samples=so, momenta=mo, rej=rejo, ratio=ro, u=u, q=q)


def metric_inputs(D, K):
    M = METRIC_CASES[(D, K)][0]
    kw, w, zeta, rs = problem(M, D, K, 41)
    return kw, start(w, zeta, F.N, rs, spread=0.1)


@functools.lru_cache(maxsize=None)
def metric_ref(D, K, method, beta, compat):
    """test_glm_metric.py's restatement of pbbi_hmc_run under the metric metric_of(Dt), on this file's oracle."""
    M, hs, L = METRIC_CASES[(D, K)]
    kw, q = metric_inputs(D, K)
    q = q.copy()
    s, p, rej, ratio, u = t_metric.r_run(oracle_pot(kw), method, q, F.MASS, t_metric.metric_of(D + K - 1),
                                         hs[F.METHODS.index(method)], L, F.S_RUN, F.SEED, F.ITER0, F.CHAIN0, F.KT, beta, compat)
    return F._frozen(samples=s, momenta=p, rej=rej, ratio=ratio, u=u, q=q)


# ------------------------------------------------------------------------------------------------ 1: header and library
def test_ordinal_header_and_library():
    hdr = open(os.path.join(ROOT, "include", "pbbi.h")).read()
    assert re.search(r"PBBI_GLM_ORDINAL\s*=\s*6\b", hdr)
    # the two entries' declarations: a part of pbbi.h in a file of its own, bound from a table of its own -- the census of
    # test_glm_abi_errors.py spells out the rejections of PROTOTYPES' GLM entries, this file those of these two (below)
    assert '#include "pbbi_glm_ordinal.h"' in hdr
    own = open(os.path.join(ROOT, "include", "pbbi_glm_ordinal.h")).read()
    from physicsbasedbayesianinference_amd import _lib, glm
    assert sorted(_lib.ORDINAL_PROTOTYPES) == ["pbbi_glm_pack_observations_ordinal", "pbbi_potential_create_glm_ordinal"]
    for n in _lib.ORDINAL_PROTOTYPES:
        assert re.search(r"\bint %s\s*\(" % n, own) and n not in _lib.PROTOTYPES, n
    assert [len(_lib.ORDINAL_PROTOTYPES[n]) for n in sorted(_lib.ORDINAL_PROTOTYPES)] == [9, 12]
    import physicsbasedbayesianinference_amd as P
    assert _lib.GLM_ORDINAL == 6 and glm.ORDINAL_MAX_DIM == MAX_DIM and glm.ORDINAL_MAX_CATEGORIES == 8
    assert P.OrdinalGLM is glm.OrdinalGLM and "OrdinalGLM" in P.__all__
    assert sorted(glm.FAMILIES) == ["logistic", "poisson"] and "ordinal" not in glm.DISPERSION_FAMILIES
    lib = _lib.load()
    assert lib.pbbi_version() == 103
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (pbbi_[a-z0-9_]+)", out))
    assert {"pbbi_potential_create_glm_ordinal", "pbbi_glm_pack_observations_ordinal"} <= exported
    for n, argtypes in _lib.ORDINAL_PROTOTYPES.items():
        assert getattr(lib, n).argtypes == argtypes, n          # bound by load()


# ------------------------------------------------------------------------------------------------ 1a: the entries' rejections
# The census of test_glm_abi_errors.py, for the two entries of this family: every rejection statement in the order the entry
# makes it, each with one call that breaks that rule alone (code and exact text); every adjacent pair broken in one call reports
# the EARLIER one; one fully valid call.  Steps, options and the shared statements are that file's.
import test_glm_abi_errors as E  # noqa: E402

CENSUS_SPECS = {
    "potential_create_glm_ordinal": [("D", "i"), ("K", "i"), ("M", "l"), ("X", "D"), ("y", "D"), ("weights", "D"), ("offset", "D"),
                                     ("prior_precision", "D"), ("prior_mean", "D")] + E._END,
    "glm_pack_observations_ordinal": [("M", "l"), ("K", "i"), ("y", "D"), ("weights", "D"), ("offset", "D"), ("out", "B"),
                                      ("out_len", "l"), ("len_out", "L"), ("counts_out", "B")],
}
CENSUS_VALID = {
    "potential_create_glm_ordinal": dict(D=2, K=3, M=3, X=E.X2, y=E.A(0, 1, 2), weights=None, offset=None,
                                         prior_precision=E.A(1, 1, 1, 1), prior_mean=None, **E._DEV),
    "glm_pack_observations_ordinal": dict(M=3, K=3, y=E.A(0, 1, 2), weights=None, offset=None, out=192, out_len=192, counts_out=8),
}
# glm_check_obs_ordinal on the valid call's K = 3
OBS_ORD = [
    ("M < 1", dict(M=0), E.INVALID, "M must be >= 1"),
    ("K > 8", dict(K=9), E.INVALID, "ordinal: the number of categories K must be 2 .. 8 (K = 9)"),
    ("K < 2", dict(K=1), E.INVALID, "ordinal: the number of categories K must be 2 .. 8 (K = 1)", dict(alt=True)),
    ("y value", dict(y=E.A(3, 1, 2)), E.INVALID, "ordinal: y must hold integer categories in [0, K) (observation 0)"),
    ("weights", dict(weights=E.A(-1, 1, 1)), E.INVALID, "weights must be finite and >= 0 (observation 0)"),
    ("offset", dict(offset=E.A(E.NAN, 0, 0)), E.INVALID, "offset must be finite (observation 0)"),
]
CENSUS = {
    "potential_create_glm_ordinal": [
        E.XY_NULL, E.XY_NULL_Y,
        ("D < 1", dict(D=0), E.INVALID, "D must be >= 1"),
        *OBS_ORD,
        ("X finite", dict(X=np.full((3, 2), E.NAN)), E.INVALID, "X must be finite"),
        ("float32", dict(dtype=E._lib.F32), E.UNSUPPORTED, "GLM potentials run on the fp64 matrix-core kernels: float64 only"),
        ("state > cap", dict(D=MAX_DIM - 1, X=np.ones((3, MAX_DIM - 1)), prior_precision=np.ones(MAX_DIM + 1)), E.UNSUPPORTED,
         "ordinal: the state dimension (coefficients + K - 1 cutpoint rows) must be <= %d (%d)" % (MAX_DIM, MAX_DIM + 1)),
        E.after(E.PRIOR[0], pair=dict(D=MAX_DIM - 1, X=np.ones((3, MAX_DIM - 1)), prior_precision=None)),
        *E.PRIOR[1:], E.OUT_NULL,
        ("unknown dtype", dict(dtype=7), E.INVALID, "unknown dtype"),
    ],
    "glm_pack_observations_ordinal": [
        OBS_ORD[0], OBS_ORD[1], OBS_ORD[2],
        ("y NULL", dict(y=None), E.INVALID, "y is NULL"),
        E.after(OBS_ORD[3], pair=False), *OBS_ORD[4:],   # no y is NULL and no category
        ("short out", dict(out_len=191), E.INVALID, "out is shorter than the three streams"),
    ],
}
CENSUS_SINGLES = [(entry, step) for entry, seq in CENSUS.items() for step in seq]
CENSUS_PAIRS = []
for _entry, _seq in CENSUS.items():
    _chain = [st for st in _seq if not E._opts(st).get("alt")]
    CENSUS_PAIRS += [(_entry, a, b) for a, b in zip(_chain, _chain[1:]) if E._opts(b).get("pair") is not False]


def census_call(entry, kw):
    """-> (return code, pbbi_last_error()), the arguments laid out as test_glm_abi_errors.call lays them out; a handle that was
    made is destroyed."""
    from physicsbasedbayesianinference_amd import _lib
    lib = _lib.load()
    args, keep, handle = [], [], None
    for name, kind in CENSUS_SPECS[entry]:
        v = kw.get(name)
        if kind in "il":
            args.append(int(v))
        elif kind in "DB":
            if v is None:
                args.append(None)
                continue
            keep.append(np.zeros(int(v)) if kind == "B" else np.ascontiguousarray(v, dtype=np.float64))
            args.append(keep[-1].ctypes.data_as(_lib._dp))
        elif kind == "H":
            handle = C.c_void_p() if v else None
            args.append(C.byref(handle) if v else None)
        else:           # L
            keep.append(C.c_int64())
            args.append(C.byref(keep[-1]))
    rc = getattr(lib, "pbbi_" + entry)(*args)
    msg = lib.pbbi_last_error().decode()
    if handle is not None and handle.value:
        assert rc == _lib.OK
        assert lib.pbbi_potential_destroy(handle) == _lib.OK
    return rc, msg


@pytest.mark.parametrize("entry,step", CENSUS_SINGLES, ids=[f"{e}-{st[0]}" for e, st in CENSUS_SINGLES])
def test_ordinal_each_rejection_alone(entry, step):
    _, wrong, code, text = step[:4]
    assert census_call(entry, dict(CENSUS_VALID[entry], **wrong)) == (code, text)


@pytest.mark.parametrize("entry,first,second", CENSUS_PAIRS, ids=[f"{e}-{a[0]}+{b[0]}" for e, a, b in CENSUS_PAIRS])
def test_ordinal_the_earlier_of_two_faults_is_reported(entry, first, second):
    opts = E._opts(second)
    both = dict(CENSUS_VALID[entry], **opts["pair"]) if "pair" in opts else dict(CENSUS_VALID[entry], **second[1], **first[1])
    if "pair" not in opts:
        assert not set(first[1]) & set(second[1]), "the two single calls change the same argument: give the pair its own call"
    assert census_call(entry, both) == (first[2], opts.get("pair_text", first[3]))


@pytest.mark.parametrize("entry", sorted(CENSUS_VALID))
def test_ordinal_a_valid_call_passes_every_check(entry):
    from physicsbasedbayesianinference_amd import _lib
    rc, msg = census_call(entry, CENSUS_VALID[entry])
    if entry.startswith("potential_create_"):
        assert rc == _lib.OK or (rc == E.HIP and msg.startswith("hipGetDeviceCount(&count): ")), (rc, msg)
    else:
        assert rc == _lib.OK, msg
    assert set(CENSUS) == set(CENSUS_VALID) == set(CENSUS_SPECS) == {n[5:] for n in _lib.ORDINAL_PROTOTYPES}


# ------------------------------------------------------------------------------------------------ 2: packing
@pytest.mark.parametrize("M", [1, 16, 203])
def test_ordinal_pack_observations(M):
    from physicsbasedbayesianinference_amd import _lib, glm
    K = 5
    kw, _, _, rs = problem(M, 3, K, 100 * M + 5)
    y, a, o = kw["y"], kw["weights"], kw["offset"]
    length = ((M + 15) // 16 + 3) // 4 * 4 * 16
    out, counts = glm.pack_observations_ordinal(y, K, weights=a, offset=o)
    assert out.shape == (3, length) and counts.shape == (8,)
    assert np.array_equal(out[0, :M], a) and np.array_equal(out[1, :M], y) and np.array_equal(out[2, :M], o)
    assert not out[:, M:].any()
    want = np.array([a[y == k].sum() for k in range(8)])
    assert np.allclose(counts, want, rtol=1e-15, atol=0) and not counts[K:].any()
    if M > 16:
        assert (want[:K] == 0).any()                                    # the emptied category
    out, counts = glm.pack_observations_ordinal(y, K)                   # the defaults: weights 1, offset 0
    assert np.array_equal(out[0, :M], np.ones(M)) and not out[2].any() and not out[:, M:].any()
    assert np.array_equal(counts, np.array([float((y == k).sum()) for k in range(8)]))
    # the helper refuses what the constructor refuses
    last = np.arange(M) == M - 1
    for bad in (-1.0, float(K), 1.5, np.nan, np.inf):
        with pytest.raises(ValueError):
            glm.pack_observations_ordinal(np.where(last, bad, y), K)
    for bad in (dict(weights=-np.ones(M)), dict(offset=np.full(M, np.inf)), dict(weights=np.ones(M + 1))):
        with pytest.raises(ValueError):
            glm.pack_observations_ordinal(y, K, **bad)
    for badK in (1, 9):
        with pytest.raises(ValueError):
            glm.pack_observations_ordinal(np.zeros(M), badK)
    # ... and the C entry says which rule and which observation
    lib = _lib.load()
    n = C.c_int64()
    buf, cnt = np.empty(3 * length), np.empty(8)
    ptr = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    assert lib.pbbi_glm_pack_observations_ordinal(M, K, None, None, None, None, 0, C.byref(n), None) == _lib.OK
    assert n.value == 3 * length
    assert lib.pbbi_glm_pack_observations_ordinal(M, K, ptr(y), None, None, ptr(buf), buf.size, C.byref(n), ptr(cnt)) == _lib.OK
    assert np.array_equal(buf.reshape(3, -1), out) and np.array_equal(cnt, counts)
    assert lib.pbbi_glm_pack_observations_ordinal(M, K, ptr(y), None, None, ptr(buf), buf.size, C.byref(n), None) == _lib.OK
    for bad in (-1.0, float(K), 0.5, np.nan):
        yb = np.ascontiguousarray(np.where(last, bad, y))
        rc = lib.pbbi_glm_pack_observations_ordinal(M, K, ptr(yb), None, None, ptr(buf), buf.size, C.byref(n), ptr(cnt))
        assert rc == _lib.ERR_INVALID
        assert _lib.last_error().endswith("y must hold integer categories in [0, K) (observation %d)" % (M - 1)), _lib.last_error()
    wb = np.ascontiguousarray(np.where(last, -0.5, 1.0))
    rc = lib.pbbi_glm_pack_observations_ordinal(M, K, ptr(y), ptr(wb), None, ptr(buf), buf.size, C.byref(n), ptr(cnt))
    assert rc == _lib.ERR_INVALID and _lib.last_error().endswith("weights must be finite and >= 0 (observation %d)" % (M - 1))
    ob = np.ascontiguousarray(np.where(last, np.inf, 0.0))
    rc = lib.pbbi_glm_pack_observations_ordinal(M, K, ptr(y), None, ptr(ob), ptr(buf), buf.size, C.byref(n), ptr(cnt))
    assert rc == _lib.ERR_INVALID and _lib.last_error().endswith("offset must be finite (observation %d)" % (M - 1))
    rc = lib.pbbi_glm_pack_observations_ordinal(M, K, ptr(y), None, None, ptr(buf), buf.size - 1, C.byref(n), ptr(cnt))
    assert rc == _lib.ERR_INVALID and "shorter" in _lib.last_error()
    for badK in (1, 9):
        rc = lib.pbbi_glm_pack_observations_ordinal(M, badK, ptr(np.zeros(M)), None, None, ptr(buf), buf.size, C.byref(n), None)
        assert rc == _lib.ERR_INVALID and "K must be 2 .. 8" in _lib.last_error()


# ------------------------------------------------------------------------------------------------ 3: refusals
def test_ordinal_refuses_on_the_host():
    from physicsbasedbayesianinference_amd import GLM, HierarchicalGLM, OrdinalGLM, _lib
    rs = np.random.RandomState(0)
    M, D, K = 12, 3, 4
    X = rs.standard_normal((M, D))
    y = (np.arange(M) % K).astype(np.float64)
    at2 = np.arange(M) == 2
    og = dict(X=X, y=y)
    bad = [dict(og, y=np.where(at2, -1.0, y)), dict(og, y=np.where(at2, 1.5, y)), dict(og, y=np.where(at2, np.nan, y)),
           dict(og, categories=3), dict(og, categories=1), dict(og, categories=9), dict(og, y=np.where(at2, 8.0, y)),
           dict(og, weights=np.where(at2, -0.5, 1.0)), dict(og, weights=np.where(at2, np.inf, 1.0)),
           dict(og, offset=np.where(at2, np.nan, 0.0)), dict(og, prior_precision=-1.0), dict(og, prior_precision=np.inf),
           dict(og, cutpoint_prior=((0.0, -1.0), (0.0, 1.0))), dict(og, cutpoint_prior=((0.0, 1.0), (np.nan, 1.0))),
           dict(og, cutpoint_prior=np.ones((K, 2))), dict(og, cutpoint_prior=(0.0, 1.0)), dict(og, dtype="float32"),
           dict(og, X=X[:, 0]), dict(og, y=y[:-1])]
    for kw in bad:
        with pytest.raises(ValueError):
            OrdinalGLM(**kw)
    with pytest.raises(ValueError, match=r"integer categories in \[0, 4\)"):
        OrdinalGLM(**dict(og, y=np.where(at2, 4.0, y), categories=4))
    # a state dimension one above the cap, the cutpoint rows included
    with pytest.raises(ValueError, match=str(MAX_DIM)):
        OrdinalGLM(X=np.ones((4, MAX_DIM - 1)), y=np.array([0.0, 1.0, 2.0, 1.0]))
    # the other classes do not serve the family
    with pytest.raises(ValueError):
        GLM(X, y, family="ordinal")
    with pytest.raises(ValueError):
        HierarchicalGLM(X, y, family="ordinal", groups=np.array([-1, 0, 0]))
    # the C entries, before anything is allocated: each value rule with its message, the shape rule, and UNSUPPORTED from the
    # hierarchical entries
    lib = _lib.load()
    ptr = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    handle = C.c_void_p()
    lam = np.ones(D + K - 1)

    def create(D_=D, K_=K, X_=X, y_=y, a_=None, o_=None, lam_=lam, mu_=None, dtype=_lib.F64):
        keep = [np.ascontiguousarray(v, dtype=np.float64) if v is not None else None for v in (X_, y_, a_, o_, lam_, mu_)]
        rc = lib.pbbi_potential_create_glm_ordinal(D_, K_, y_.size, *[ptr(v) for v in keep], dtype, 0, C.byref(handle))
        return rc, _lib.last_error()

    for kwargs, code, text in (
            (dict(y_=np.where(at2, 4.0, y)), _lib.ERR_INVALID, "ordinal: y must hold integer categories in [0, K) (observation 2)"),
            (dict(y_=np.where(at2, -1.0, y)), _lib.ERR_INVALID, "ordinal: y must hold integer categories in [0, K) (observation 2)"),
            (dict(y_=np.where(at2, 0.5, y)), _lib.ERR_INVALID, "ordinal: y must hold integer categories in [0, K) (observation 2)"),
            (dict(a_=np.where(at2, -0.5, 1.0)), _lib.ERR_INVALID, "weights must be finite and >= 0 (observation 2)"),
            (dict(a_=np.where(at2, np.nan, 1.0)), _lib.ERR_INVALID, "weights must be finite and >= 0 (observation 2)"),
            (dict(o_=np.where(at2, np.inf, 0.0)), _lib.ERR_INVALID, "offset must be finite (observation 2)"),
            (dict(lam_=np.where(np.arange(D + K - 1) == D + 1, -1.0, 1.0)), _lib.ERR_INVALID,
             "prior_precision must be finite and >= 0 (coefficient %d)" % (D + 1)),
            (dict(lam_=np.where(np.arange(D + K - 1) == 1, np.inf, 1.0)), _lib.ERR_INVALID,
             "prior_precision must be finite and >= 0 (coefficient 1)"),
            (dict(K_=1, y_=np.zeros(M)), _lib.ERR_INVALID, "K must be 2 .. 8 (K = 1)"),
            (dict(K_=9), _lib.ERR_INVALID, "K must be 2 .. 8 (K = 9)"),
            (dict(dtype=_lib.F32), _lib.ERR_UNSUPPORTED, "float64"),
            (dict(D_=MAX_DIM - K + 2, X_=np.ones((M, MAX_DIM - K + 2)), lam_=np.ones(MAX_DIM + 1)), _lib.ERR_UNSUPPORTED,
             "must be <= %d (%d)" % (MAX_DIM, MAX_DIM + 1))):
        rc, msg = create(**kwargs)
        assert rc == code and not handle.value and text in msg, (kwargs.keys(), rc, msg)
    groups = np.array([-1, 0, 0], dtype=np.int32)
    gp = groups.ctypes.data_as(C.POINTER(C.c_int32))
    tp, dp = np.array([0.0, 1.0]), np.array([0.0, 0.25])
    rc = lib.pbbi_potential_create_glm_hier(D, M, ptr(X), ptr(y), 6, None, None, None, ptr(lam), None, gp, 1, ptr(tp), _lib.F64, 0,
                                            C.byref(handle))
    assert rc == _lib.ERR_UNSUPPORTED and not handle.value and "ordinal" in _lib.last_error()
    rc = lib.pbbi_potential_create_glm_hier_dispersion(D, M, ptr(X), ptr(y), 6, None, None, ptr(lam), None, gp, 1, ptr(tp),
                                                       _lib.HIER_CENTRED, 1, 0.0, ptr(dp), _lib.F64, 0, C.byref(handle))
    assert rc == _lib.ERR_UNSUPPORTED and not handle.value and "ordinal" in _lib.last_error()


# ------------------------------------------------------------------------------------------------ 4: the class
def test_ordinal_class_layout_round_trip_and_defaults():
    from physicsbasedbayesianinference_amd import glm
    sig = inspect.signature(glm.OrdinalGLM.__init__)
    assert list(sig.parameters)[1:9] == ["X", "y", "categories", "prior_precision", "prior_mean", "weights", "offset",
                                         "cutpoint_prior"]
    assert sig.parameters["categories"].default is None and sig.parameters["prior_precision"].default == 1.0
    assert sig.parameters["cutpoint_prior"].default == ((0.0, 0.1), (0.0, 1.0))
    for base in (glm._Tempered, glm.GLM.__mro__[2], glm.Potential):      # the mix-ins DispersionGLM has
        assert issubclass(glm.OrdinalGLM, base) and issubclass(glm.DispersionGLM, base)
    assert glm.OrdinalGLM.kind == "glm" and glm.OrdinalGLM.family == "ordinal"
    # the default pair per kind of row, spread over the K - 1 rows; arrays of K - 1 pairs taken as given
    for K in range(2, 9):
        cp = glm._cutpoint_prior(((0.0, 0.1), (0.0, 1.0)), K)
        assert cp.shape == (K - 1, 2) and tuple(cp[0]) == (0.0, 0.1) and np.all(cp[1:] == np.array([0.0, 1.0]))
        given = np.c_[np.arange(K - 1.0), 1.0 + np.arange(K - 1.0)]
        if K != 3:
            assert np.array_equal(glm._cutpoint_prior(given, K), given)
    # split / unconstrain on an instance that owns no handle (the arithmetic touches no device)
    D, K, N, S = 3, 5, 7, 2
    pot = object.__new__(glm.OrdinalGLM)
    pot.numCoefficients, pot.categories, pot.numDimensions = D, K, D + K - 1
    rs = np.random.RandomState(3)
    q = rs.standard_normal((D + K - 1, N, S))
    w, kappa = pot.split(q)
    assert w.shape == (D, N, S) and kappa.shape == (K - 1, N, S) and np.array_equal(w, q[:D])
    assert np.all(np.diff(kappa, axis=0) > 0) and np.array_equal(kappa[0], q[D])
    assert np.allclose(kappa[2], q[D] + np.exp(q[D + 1]) + np.exp(q[D + 2]), rtol=1e-15)
    back = pot.unconstrain(w, kappa)
    assert back.shape == q.shape and np.max(np.abs(back - q)) < 1e-12
    with pytest.raises(ValueError):
        pot.unconstrain(w, kappa[::-1])
    with pytest.raises(ValueError):
        pot.unconstrain(w[:-1], kappa)
    # the prior's layout, which sample_prior and LikelihoodTemperedSMC read
    pot.prior_precision, pot.prior_mean = np.array([1.0, 2.0, 3.0]), np.array([0.1, 0.2, 0.3])
    pot.cutpoint_prior = glm._cutpoint_prior(((-0.5, 0.1), (0.25, 1.0)), K)
    mean, prec, names, Dn, J, groups = glm._prior_layout(pot)
    assert np.array_equal(mean, [0.1, 0.2, 0.3, -0.5, 0.25, 0.25, 0.25]) and np.array_equal(prec, [1, 2, 3, 0.1, 1, 1, 1])
    assert Dn == D and J == 0 and groups is None and names[D:] == ["cutpoint_prior[%d]" % j for j in range(K - 1)]
    assert np.array_equal(glm.pointwise_constants("ordinal", np.array([0.0, 2.0]), np.array([1.0, 3.0])), np.zeros(2))


# ------------------------------------------------------------------------------------------------ 5: the yardstick
@pytest.mark.parametrize("D,K", [(5, 2), (5, 5), (16, 8)])
def test_ordinal_oracle_source_is_pinned(D, K):
    """The yardstick, not the feature: the oracle's U equals a longdouble NumPy evaluation of the category probabilities
    within 1e-12 relative and its gradient central differences within 1e-6, at M = 40."""
    M, N = 40, 12
    kw, w, zeta, rs = problem(M, D, K, 5)
    q = start(w, zeta, N, rs)
    op = oracle_pot(kw)
    U, g = orc.potential(op, q, want_grad=True)
    Un = numpy_U(kw, q)
    e = float(np.max(np.abs(U - Un) / np.maximum(1.0, np.abs(Un))))
    print("U against NumPy", e)
    assert e <= 1e-12
    h = 1e-5
    fd = np.empty_like(g)
    for j in range(q.shape[0]):
        qp, qm = q.copy(), q.copy()
        qp[j] += h
        qm[j] -= h
        fd[j] = (orc.potential(op, qp) - orc.potential(op, qm)) / (2 * h)
    e = rel(g, fd)
    print("gradient against central differences", e)
    assert e <= 1e-6
    assert g.shape[0] == D + K - 1
    p, mean = probabilities(kw, q)
    assert np.all(p > 0) and np.all(p <= 1) and np.all(mean >= 0) and np.all(mean <= K - 1)


def test_ordinal_sampling_cases_are_decisive():
    """Every sampling case of test_glm_ordinal.py on the oracle alone: both outcomes occur and no accept test hangs on rounding."""
    for M, D, K, h_lf, h_sv, L in ITER_CASES:
        for method in ("Leapfrog", "Stormer-Verlet"):
            for mass in (False, True):
                for kt in (False, True):
                    h = iter_step(method, mass, h_lf, h_sv)
                    o = iter_oracle(M, D, K, h, L, method, mass, kt)
                    print(M, D, K, method, mass, kt)
                    decisive(o["ratio"], o["u"], o["rej"], 0.1, 0.9)
                    # ... and the yardstick is accurate where EVERY proposal ends (u = 0 accepts them all)
                    kw, N, kT, m, q, p, u = iter_inputs(M, D, K, mass, kt)
                    orc.hmc_iter(oracle_pot(kw), method, q, p, np.zeros(N), m, h, L, beta=1.0 / kT)
                    e = oracle_accuracy(kw, q)
                    print("oracle's own error at the proposals", e)
                    assert e <= ORACLE_TOL
    for case in RUN_CASES:
        o = run_oracle(*case)
        print(case)
        assert np.all(np.isfinite(o["samples"])) and np.all(np.isfinite(o["momenta"]))
        decisive(o["ratio"], o["u"], o["rej"], 0.1, 0.9)
        e = oracle_accuracy(run_inputs(*case[:4])[0], np.concatenate(list(o["samples"]), axis=1))
        print("oracle's own error at the samples", e)
        assert e <= ORACLE_TOL
    for (D, K) in METRIC_CASES:
        for row in METRIC_ROWS:
            o = metric_ref(D, K, *row)
            t_metric._margin(str((D, K) + row), o["ratio"], o["u"])
            assert 0.1 <= o["rej"].mean() <= 0.9
            e = oracle_accuracy(metric_inputs(D, K)[0], np.concatenate(list(o["samples"]), axis=1))
            print("oracle's own error at the samples", e)
            assert e <= ORACLE_TOL
            # the unit-metric run of the same case (device against device on the GPU) stays finite and decides both ways
            M, hs, L = METRIC_CASES[(D, K)]
            kw, q = metric_inputs(D, K)
            me, b, c = row
            s, _, rej, ratio, _ = t_metric.r_run(oracle_pot(kw), me, q.copy(), F.MASS, None, UNIT_H * hs[F.METHODS.index(me)], L,
                                                 F.S_RUN, F.SEED, F.ITER0, F.CHAIN0, F.KT, b, c)
            assert np.all(np.isfinite(s)) and np.all(np.isfinite(ratio)) and 0.05 < rej.mean() < 0.95
