"""The host side of the posterior predictive kernel (no GPU): the ABI, every argument rule of pbbi_predictive_glm in the order
include/pbbi.h states it, `PredictiveResult.pvalue`, and the reference helper glm_predictive_ref.py held to SciPy's exact
distributions -- so that what the GPU tests compare the device with is itself a sampler of the right law.

Distribution bound: p >= 1e-6 on a fixed seed, for a chi-square on the pmf with cells of expected count >= 20 (discrete
families) or Kolmogorov-Smirnov on the cdf (gamma, gaussian) over 2^18 values.  That is a false-alarm rate -- a correct
sampler fails a case once in a million seeds -- not a measurement; a wrong mode, a skipped point or an off-by-one fails it by
hundreds of orders of magnitude at this sample size."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import glm_predictive_ref as R
import test_glm_pointwise as t_pw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"pbbi_predictive_glm", "pbbi_predictive_glm_check"}
P_MIN = 1e-6
DIST_T, DIST_M, DIST_SEED = 64, 4096, 2024          # 2^18 values: 64 identical draws x 4096 identical rows

# family, the parameters of glm_predictive_ref.fixed
DIST_CASES = [("poisson", dict(mu=0.3)), ("poisson", dict(mu=7.5)), ("poisson", dict(mu=180.0)),
              ("logistic", dict(n=12, p=0.1)), ("logistic", dict(n=12, p=0.5)),
              ("negbinomial", dict(mu=6.0, phi=0.4)), ("negbinomial", dict(mu=40.0, phi=5.0)),
              ("gamma", dict(mu=2.0, alpha=0.5)), ("gamma", dict(mu=2.0, alpha=3.0)),
              ("gaussian", dict(mu=1.0, sigma=2.0)),
              ("ordinal", dict(eta=0.3, kap=[-1.0, -0.2, 0.5, 1.7]))]          # K = 5
DIST_IDS = ["%s-%s" % (f, "-".join("%s%s" % (k, v) for k, v in p.items() if k != "kap")) for f, p in DIST_CASES]


def test_predictive_abi_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pbbi.h")).read()
    assert re.search(r"\bint\s+pbbi_predictive_glm\s*\(const pbbi_potential\* pot, const void\* samples_sdn, int S, int Dt, "
                     r"int64_t N, uint64_t seed,\s*const double\* aux, double centre, double cut, int ranges, "
                     r"double\* stats_out, int64_t keep,\s*double\* yrep_out, void\* stream\);", hdr)
    assert re.search(r"PBBI_STREAM_PREDICTIVE = 6\b", hdr)
    from physicsbasedbayesianinference_amd import _lib
    assert NAMES <= set(_lib.PROTOTYPES) and _lib.STREAM_PREDICTIVE == 6 == R.STREAM_PREDICTIVE
    assert len(_lib.PROTOTYPES["pbbi_predictive_glm"]) == 14 and len(_lib.PROTOTYPES["pbbi_predictive_glm_check"]) == 14
    lib = _lib.load()
    for name in NAMES:
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert NAMES <= set(re.findall(r"\bT (pbbi_[a-z0-9_]+)", out))
    assert not any(n.startswith("pbbi_glm_") for n in NAMES)      # outside the census of test_glm_abi_errors.py
    import physicsbasedbayesianinference_amd as P
    for cls in (P.GLM, P.DispersionGLM, P.OrdinalGLM, P.HierarchicalGLM, P.HierarchicalDispersionGLM):
        assert callable(cls.predictive) and callable(cls.pointwise)
    assert not hasattr(P.SoftmaxGLM, "predictive")
    assert P.PredictiveResult is P.glm.PredictiveResult and "PredictiveResult" in P.__all__
    mk = open(os.path.join(ROOT, "physicsbasedbayesianinference_amd", "csrc", "Makefile")).read()
    assert "kernels_glm_predictive.hip" in mk and "glm_sample_dev.h" in mk


def test_predictive_rejects_bad_arguments_without_a_device():
    """Code and text of every rule, in the header's order: each case breaks every LATER rule too, so the answer names the
    first rule broken."""
    from physicsbasedbayesianinference_amd import _lib
    lib = _lib.load()
    buf = (C.c_double * 4)()
    ptr = C.addressof(buf)
    assert lib.pbbi_predictive_glm(None, ptr, 3, 5, 150, 0, ptr, 0.0, 0.0, 0, ptr, 0, None, None) == _lib.ERR_INVALID
    assert "handle is NULL" in _lib.last_error()
    good = dict(handle=1, family=_lib.GLM_POISSON, state_dim=5, samples=ptr, aux=ptr, stats=ptr, S=3, Dt=5, N=150, ranges=0,
                keep=0, yrep=0, centre=1.5, cut=0.0)

    def rc(**kw):
        a = dict(good, **kw)
        return lib.pbbi_predictive_glm_check(a["handle"], a["family"], a["state_dim"], a["samples"], a["aux"], a["stats"],
                                             a["S"], a["Dt"], a["N"], a["ranges"], a["keep"], a["yrep"], a["centre"], a["cut"])

    assert rc() == _lib.OK and rc(ranges=7) == _lib.OK and rc(Dt=9) == _lib.OK and rc(S=1, N=1) == _lib.OK
    assert rc(keep=450, yrep=1) == _lib.OK and rc(keep=1, yrep=1) == _lib.OK and rc(cut=-3.5, centre=-1e300) == _lib.OK
    assert rc(S=1, N=1 << 32) == _lib.OK and rc(S=1 << 16, N=1 << 16) == _lib.OK
    for fam in (_lib.GLM_LOGISTIC, _lib.GLM_GAUSSIAN, _lib.GLM_NEGBINOMIAL, _lib.GLM_GAMMA, _lib.GLM_ORDINAL):
        assert rc(family=fam) == _lib.OK
    nan = float("nan")
    order = [(dict(handle=0), _lib.ERR_INVALID, "handle is NULL"),
             (dict(samples=None), _lib.ERR_INVALID, "samples is NULL"),
             (dict(S=0), _lib.ERR_INVALID, "S must be >= 1"),
             (dict(N=0), _lib.ERR_INVALID, "N must be >= 1"),
             (dict(ranges=65536), _lib.ERR_INVALID, "ranges must be"),
             (dict(handle=2), _lib.ERR_UNSUPPORTED, "not a GLM handle"),
             (dict(family=_lib.GLM_SOFTMAX), _lib.ERR_UNSUPPORTED, "softmax"),
             (dict(family=99), _lib.ERR_UNSUPPORTED, "unknown GLM family"),
             (dict(Dt=4), _lib.ERR_INVALID, "state dimension"),
             (dict(aux=None), _lib.ERR_INVALID, "aux is NULL"),
             (dict(stats=None), _lib.ERR_INVALID, "stats_out is NULL"),
             (dict(keep=-1), _lib.ERR_INVALID, "keep must be in 0 .. S * N"),
             (dict(yrep=1), _lib.ERR_INVALID, "yrep_out needs keep > 0"),
             (dict(centre=nan), _lib.ERR_INVALID, "centre must be finite"),
             (dict(cut=nan), _lib.ERR_INVALID, "cut must be finite")]
    for i, (kw, code, text) in enumerate(order):
        assert rc(**kw) == code, kw
        msg = _lib.last_error()
        assert text in msg, (kw, msg)
        if code == _lib.ERR_UNSUPPORTED:       # the rule is in the text
            assert "pbbi_predictive_glm: " in msg and "serves the handles of" in msg and "_glm_hier_dispersion" in msg
        later = {}
        for k2, _, _ in order[i + 1:]:
            later.update({k: v for k, v in k2.items() if k not in later})
        later.update(kw)
        assert rc(**later) == code and text in _lib.last_error(), (kw, later, _lib.last_error())
    # the rules that have two sides, and S * N <= 2^32 (between stats_out and keep)
    assert rc(keep=451, yrep=1) == _lib.ERR_INVALID and "keep must be in" in _lib.last_error()
    assert rc(keep=5, yrep=0) == _lib.ERR_INVALID and "keep > 0 needs yrep_out" in _lib.last_error()
    for bad in (float("inf"), -float("inf")):
        assert rc(centre=bad) == _lib.ERR_INVALID and rc(cut=bad) == _lib.ERR_INVALID
    assert rc(S=1, N=(1 << 32) + 1) == _lib.ERR_INVALID and "S * N must be <= 2^32" in _lib.last_error()
    assert rc(S=3, N=1 << 31, keep=-1, centre=nan) == _lib.ERR_INVALID and "S * N must be <= 2^32" in _lib.last_error()
    assert rc(S=3, N=1 << 31, stats=None) == _lib.ERR_INVALID and "stats_out is NULL" in _lib.last_error()
    assert rc(S=2000000000, N=1 << 40) == _lib.ERR_INVALID and "2^32" in _lib.last_error()      # formed in 64 bits


def test_predictive_result_pvalue():
    from physicsbasedbayesianinference_amd import PredictiveResult
    v = np.arange(12.0).reshape(4, 3)                              # (N, S)
    obs = dict(mean=3.0, var=100.0, min=-1.0, max=5.5, frac_le_cut=11.0)
    r = PredictiveResult(mean=v, var=v, min=v, max=v, frac_le_cut=v, loglik_rep=v - 6.0, loglik_obs=np.zeros((4, 3)), observed=obs)
    assert r.T == 12 and r.yrep is None
    assert r.pvalue("mean") == 9 / 12 and r.pvalue("var") == 0.0 and r.pvalue("min") == 1.0 and r.pvalue("max") == 6 / 12
    assert r.pvalue("frac_le_cut") == 1 / 12
    assert r.pvalue("loglik") == 7 / 12                            # loglik_rep <= loglik_obs
    w = v.copy()
    w[0, 0] = np.nan                                               # a NaN draw meets no condition
    assert PredictiveResult(w, w, w, w, w, w, w, obs).pvalue("min") == 11 / 12
    with pytest.raises(ValueError, match="unknown statistic"):
        r.pvalue("median")
    assert "p_var=0" in repr(r)


def test_reference_counters_are_the_contracts():
    """The helper's Philox is the oracle's, its uniform is never 0, and its restated normal is the oracle's to a few ulp."""
    from oracle import oracle as orc
    ctr, key = [5, 7, 9, 6 | (3 << 8)], [123, 456]
    assert [int(x) for x in R.philox(*ctr, *key)] == orc.philox_raw(ctr, key)
    seed = (456 << 32) | 123
    x = R.block(seed, 9, (3 << 32) | 5, 7)                         # chain's high bits go beside the stream number
    assert [int(v) for v in x] == orc.philox_raw(ctr, key)
    t, i = np.arange(6)[:, None], np.arange(300)[None, :]
    u = R.uniform(seed, t, i)
    assert u.min() > 0.0 and u.max() <= 1.0 and abs(u.mean() - 0.5) < 0.03
    assert np.max(np.abs(R.normal_np(seed, t, i) - R.normal_oracle(seed, t, i))) < 1e-14


@pytest.mark.parametrize("family,par", DIST_CASES, ids=DIST_IDS)
def test_reference_samples_the_exact_distribution(family, par):
    y = R.fixed(family, DIST_SEED, DIST_T, DIST_M, **par)
    assert y.shape == (DIST_T, DIST_M)
    p = R.gof_pvalue(family, y, **par)
    print("p-value %s %s: %.3g" % (family, par, p))
    assert p >= P_MIN


def test_reference_enumeration_is_the_plain_inverse_where_both_are_defined():
    """The walk from the mode is a permutation of the support: with every cell visited it must give each value its exact mass.
    Checked without sampling: the u-measure of each value, read off a fine grid of u, equals SciPy's pmf."""
    u = (np.arange(200000) + 0.5) / 200000
    for fam, eta, theta, n, dist in [("poisson", np.log(7.5), 0.0, 1.0, R.stats.poisson(7.5)),
                                     ("logistic", np.log(0.3 / 0.7), 0.0, 12.0, R.stats.binom(12, 0.3)),
                                     ("negbinomial", np.log(6.0), np.log(0.4), 1.0, R.stats.nbinom(0.4, 0.4 / 6.4))]:
        y = R.discrete(fam, u, np.full(u.size, eta), theta, n)
        share = np.bincount(y.astype(int)) / u.size
        assert np.max(np.abs(share - dist.pmf(np.arange(share.size)))) < 2.0 / u.size * 2
    # n = 1: u < p
    y = R.discrete("logistic", u, np.full(u.size, np.log(0.3 / 0.7)), 0.0, 1.0)
    assert np.array_equal(y, (u < R.special.expit(np.log(0.3 / 0.7))).astype(float))
    # beyond the variance cap, and a non-finite eta: NaN
    assert np.isnan(R.discrete("poisson", [0.5, 0.5], [np.log(2.0 ** 20 + 4.0), np.inf])).all()
    assert R.discrete("poisson", [0.5], [np.log(2.0 ** 20 - 4.0)])[0] > 1e6


@pytest.mark.parametrize("name", ["binomial_trials", "poisson_full", "negbinomial_sampled", "gaussian_sampled"])
def test_reference_leaves_almost_nothing_undecided(name):
    """The cap the GPU tests rely on: at most 0.1 % of a case's values undecided (expected ~1e-9)."""
    _, sp, sdn, _ = t_pw.kind(name)
    y, und = R.replicates(sp, t_pw.flat(sdn), seed=5)
    on = sp["a"] != 0.0
    assert y.shape == (t_pw.S * t_pw.N, sp["y"].size) and np.all(np.isnan(y[:, ~on])) and np.all(np.isfinite(y[:, on]))
    print("undecided %s: %d of %d" % (name, und.sum(), und.size))
    assert und.mean() <= R.MAX_UNDECIDED
    if sp["family"] != "gaussian":
        assert np.all(y[:, on] == np.floor(y[:, on])) and y[:, on].min() >= 0
    if sp["family"] == "logistic":
        assert np.all(y[:, on] <= sp["n"][on][None, :])
