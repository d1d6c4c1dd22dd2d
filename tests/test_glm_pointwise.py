"""Pointwise log-likelihood over posterior draws, reduced on the device (csrc/kernels_glm_pointwise.hip,
pbbi_pointwise_glm, `pointwise` of GLM / DispersionGLM / HierarchicalGLM / HierarchicalDispersionGLM).

Reference: NumPy in `longdouble` on the host copy of the same draws -- eta = X W + o, the link and the four reductions
(max-shifted log-sum-exp, two-pass mean and unbiased variance, the mean of the fitted mean) all in longdouble; only
log Gamma is evaluated in double (scipy.special.gammaln, absolute error ~1e-13 at the counts used here) and promoted.  The
data are the problem generators of the existing GLM test files, imported as test_glm_frame.py imports them.

Tolerance: test_glm.py's TOL = 1e-10 relative to max(1, max|reference|), through its `check`, for all four outputs; the
variance met it as it stands (the kernel accumulates it with Welford's recurrence and merges with Chan's formula), so no
figure of its own was needed.  Bit-for-bit claims are compared on the int64 view.

Every device call of this file runs inside a NaN canary: the slabs are followed by a NaN guard region in the same
allocation and the (M,) outputs sit in the middle of longer NaN-filled arrays whose other elements must keep their bits.
"""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import test_glm as t_plain
import test_glm_dispersion as t_disp
import test_glm_hier as t_hier
import test_glm_hier_noncentred as t_nc
import test_glm_model as t_model
from test_glm import check     # rel <= TOL = 1e-10 relative to max(1, max|reference|)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
N, S = 150, 3          # nine full 16-draw tiles and one of 6 per slab
DATA_SEED = 11         # the seed of every GLM test file's ITER_CASES data
PAD, GUARD = 32, 4096  # NaN elements on each side of an output, behind the slabs


# ---- the reference ---------------------------------------------------------------------------------------------------
def spec_of(family, kw, Dx, trow=-1, theta=None):
    """What the kernel sees of a model: X, the streams c | d | o, the coefficient count, where theta is."""
    X, y = kw["X"], kw["y"]
    M = y.size
    a = np.ones(M) if kw.get("weights") is None else kw["weights"]
    o = np.zeros(M) if kw.get("offset") is None else kw["offset"]
    n = np.ones(M) if kw.get("trials") is None else kw["trials"]
    return dict(family=family, X=X, y=y, a=a, o=o, n=n, Dx=Dx, trow=trow, theta=theta)


def gammaln_ld(x):
    from scipy.special import gammaln
    return gammaln(np.asarray(x, dtype=np.float64)).astype(LD)


def ref_ll(sp, W):
    """(ll, mu), each (M, T) longdouble, of the natural-scale draws W (Dt, T): ll without the constants k_i, exactly 0 on a
    row of weight 0."""
    X, a, y, n, o = (np.asarray(sp[k]).astype(LD) for k in ("X", "a", "y", "n", "o"))
    Wl = np.asarray(W).astype(LD)
    eta = X @ Wl[:sp["Dx"]] + o[:, None]
    fam = sp["family"]
    if fam in ("gaussian", "negbinomial"):
        th = Wl[sp["trow"]][None, :] if sp["trow"] >= 0 else LD(sp["theta"])
    if fam == "logistic":
        ll = (a * y)[:, None] * eta - (a * n)[:, None] * np.logaddexp(LD(0), eta)
        mu = 1 / (1 + np.exp(-eta))
    elif fam == "poisson":
        ll = (a * y)[:, None] * eta - a[:, None] * np.exp(eta)
        mu = np.exp(eta)
    elif fam == "gaussian":
        r = y[:, None] - eta
        ll = -a[:, None] * (LD(0.5) * np.exp(-2 * th) * r * r + th)
        mu = eta
    else:
        phi = np.exp(th) + 0 * eta
        z = eta - th
        ll = -a[:, None] * (gammaln_ld(phi) - gammaln_ld(y[:, None] + phi) + (y[:, None] + phi) * np.logaddexp(LD(0), z)
                            - y[:, None] * z)
        mu = np.exp(eta)
    ll[np.asarray(sp["a"]) == 0.0] = 0
    return ll, mu


def ref_stats(ll, mu):
    """lse, mean, unbiased variance (NaN for one draw), mean fitted mean: max-shifted and two-pass, in longdouble."""
    T = ll.shape[1]
    m = ll.max(axis=1)
    lse = m + np.log(np.sum(np.exp(ll - m[:, None]), axis=1))
    mean = ll.sum(axis=1) / T
    var = ((ll - mean[:, None]) ** 2).sum(axis=1) / (T - 1) if T > 1 else np.full(ll.shape[0], np.nan, dtype=LD)
    return lse, mean, var, mu.sum(axis=1) / T


def flat(sdn):
    """(S, Dt, N) slabs -> (Dt, S * N): the draws in the order slab-major, chain-minor."""
    return np.concatenate(list(sdn), axis=1)


def reference(sp, sdn):
    return ref_stats(*ref_ll(sp, flat(sdn)))


def constants_ref(sp):
    """k_i from log Gamma directly."""
    a, y, n = sp["a"], sp["y"], sp["n"]
    from scipy.special import gammaln
    if sp["family"] == "logistic":
        return a * (gammaln(n + 1) - gammaln(y + 1) - gammaln(n - y + 1))
    if sp["family"] == "gaussian":
        return -0.5 * a * np.log(2 * np.pi)
    return -a * gammaln(y + 1)


# ---- the table of kinds: how the handle is made, what the kernel sees of it, S slabs of natural-scale draws -----------
def _slabs(one, n=N, s=S):
    return np.ascontiguousarray(np.stack([one(n) for _ in range(s)]))


def _plain(D, M=203, family="logistic", n=N, s=S):
    X, y, w, rs = t_plain.problem(family, M, D, DATA_SEED)
    kw = dict(X=X, y=y)
    return (lambda P: P.GLM(X, y, family=family)), spec_of(family, kw, D), _slabs(lambda k: t_plain.start(w, k, rs), n, s)


def _full(family, M, D):
    kw, w, rs = t_model.problem(family, M, D, DATA_SEED)
    return (lambda P: P.GLM(**kw)), spec_of(family, kw, D), _slabs(lambda k: t_model.start(w, k, rs, spread=0.1))


def _dispersion(family, sampled):
    kw, w, theta, rs = t_disp.problem(family, 40, 5, DATA_SEED)
    held = None if sampled else float(np.log(np.exp(theta)))   # the class takes exp(theta) and the library its logarithm
    return ((lambda P: t_disp.make(P, kw, sampled, theta)), spec_of(family, kw, 5, 5 if sampled else -1, held),
            _slabs(lambda k: t_disp.start(w, theta, k, rs, spread=0.1, sampled=sampled)))


def _hier():
    kw, w, t, rs = t_hier.problem("logistic", 40, 5, 2, DATA_SEED)
    return (lambda P: P.HierarchicalGLM(**kw)), spec_of("logistic", kw, 5), _slabs(lambda k: t_hier.start(w, t, k, rs, spread=0.1))


def _hier_nc():
    """The slabs are in SAMPLER coordinates (z on the grouped rows): `pointwise` converts, the reference uses natural_np."""
    kw, w, t, rs = t_hier.problem("logistic", 40, 5, 2, DATA_SEED)
    sp = spec_of("logistic", kw, 5)
    sp["kw"] = kw
    return (lambda P: t_nc.nc_pot(P, kw)), sp, _slabs(lambda k: t_nc.nc_start(kw, w, t, k, rs, spread=0.1))


KINDS = {
    "logistic": lambda: _plain(5),                               # plain, M = 203, D = 5
    "poisson_full": lambda: _full("poisson", 300, 8),            # offsets, weights with zeros
    "binomial_trials": lambda: _full("logistic", 203, 5),        # trials in 1 .. 20, weights with zeros
    "gaussian_sampled": lambda: _dispersion("gaussian", True),
    "negbinomial_held": lambda: _dispersion("negbinomial", False),
    "negbinomial_sampled": lambda: _dispersion("negbinomial", True),
    "hier": _hier,
    "logistic17": lambda: _plain(17),                            # NT = 2
    "logistic50": lambda: _plain(50),                            # NT = 4
    "logistic128": lambda: _plain(128),                          # NT = 8
}


@functools.lru_cache(maxsize=None)
def kind(name):
    """(make, spec, slabs, reference): built once, shared, never written to."""
    make, sp, sdn = (_hier_nc if name == "hier_nc" else KINDS[name])()
    nat = np.stack([t_nc.natural_np(sp["kw"], q) for q in sdn]) if name == "hier_nc" else sdn
    ref = reference(sp, nat)
    sdn.setflags(write=False)
    for r in ref:
        r.setflags(write=False)
    return make, sp, sdn, ref


def stability_case():
    """Plain logistic, M = 203, D = 5: the draws are multiples a_t w of one direction, scaled so that observation i0 has
    ll_t = -a_t with a_t from 1200 to 2800 -- near -2000, spread 1600 -- and every exp(ll_t) underflows in double."""
    X, y, w, rs = t_plain.problem("logistic", 203, 5, DATA_SEED)
    p = X @ w
    i0 = int(np.argmax(np.abs(p)))
    sign = -1.0 if (y[i0] == 1.0) == (p[i0] > 0) else 1.0     # push observation i0 to the wrong side
    a = np.linspace(1200.0, 2800.0, N * S)[rs.permutation(N * S)]
    W = (sign / abs(p[i0])) * w[:, None] * a[None, :]
    sdn = np.ascontiguousarray(W.reshape(5, S, N).transpose(1, 0, 2))
    return X, y, i0, sdn, spec_of("logistic", dict(X=X, y=y), 5)


def overflow_case():
    """The full Poisson model with one draw (slab 1, chain 7) whose eta reaches 800 on the rows it points at."""
    make, sp, sdn, _ = kind("poisson_full")
    sdn = sdn.copy()
    X, o = sp["X"], sp["o"]
    u = sdn[1, :, 7]
    top = int(np.argmax(np.where(sp["a"] != 0.0, X @ u, -np.inf)))     # ... among the rows that have weight
    big = u * (800.0 - o[top]) / (X @ u)[top]      # eta = 800 on the row the draw points at most
    sdn[1, :, 7] = big
    return make, sp, sdn, X @ big + o


# ------------------------------------------------------------------------------------------------ CPU
def test_pointwise_abi_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pbbi.h")).read()
    assert re.search(r"\bint\s+pbbi_pointwise_glm\s*\(const pbbi_potential\* pot, const void\* samples_sdn, int S, int Dt, "
                     r"int64_t N, int ranges,\s*double\* lse_out, double\* mean_out, double\* var_out, double\* mu_out, "
                     r"void\* stream\);", hdr)
    from physicsbasedbayesianinference_amd import _lib
    assert len(_lib.PROTOTYPES["pbbi_pointwise_glm"]) == 11 and "pbbi_pointwise_glm_check" in _lib.PROTOTYPES
    lib = _lib.load()
    assert lib.pbbi_pointwise_glm.argtypes == _lib.PROTOTYPES["pbbi_pointwise_glm"]      # bound by load()
    assert lib.pbbi_version() == 103
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (pbbi_[a-z0-9_]+)", out))
    assert {"pbbi_pointwise_glm", "pbbi_pointwise_glm_check"} <= exported
    import physicsbasedbayesianinference_amd as P
    for cls in (P.GLM, P.DispersionGLM, P.HierarchicalGLM, P.HierarchicalDispersionGLM, P.SoftmaxGLM):
        assert callable(getattr(cls, "pointwise"))


def test_pointwise_rejects_bad_arguments_without_a_device():
    """Code and text of every rule; the entry point itself answers for a NULL handle before it touches a device, the
    rules that need a handle are asked of the same checker by value (pbbi_pointwise_glm_check)."""
    import ctypes as C
    from physicsbasedbayesianinference_amd import _lib
    lib = _lib.load()
    buf = (C.c_double * 4)()
    ptr = C.addressof(buf)
    assert lib.pbbi_pointwise_glm(None, ptr, 3, 5, 150, 0, None, None, None, None, None) == _lib.ERR_INVALID
    assert "handle is NULL" in _lib.last_error()
    good = dict(handle=1, family=_lib.GLM_LOGISTIC, state_dim=5, samples=ptr, S=3, Dt=5, N=150, ranges=0, want_var=1)

    def rc(**kw):
        a = dict(good, **kw)
        return lib.pbbi_pointwise_glm_check(a["handle"], a["family"], a["state_dim"], a["samples"], a["S"], a["Dt"], a["N"],
                                            a["ranges"], a["want_var"])

    assert rc() == _lib.OK and rc(ranges=7) == _lib.OK and rc(Dt=9) == _lib.OK
    assert rc(S=1, N=1, want_var=0) == _lib.OK
    for fam in (_lib.GLM_POISSON, _lib.GLM_GAUSSIAN, _lib.GLM_NEGBINOMIAL):
        assert rc(family=fam) == _lib.OK
    cases = [(dict(handle=0), _lib.ERR_INVALID, "handle is NULL"),
             (dict(samples=None), _lib.ERR_INVALID, "samples is NULL"),
             (dict(S=0), _lib.ERR_INVALID, "S must be >= 1"),
             (dict(S=-3), _lib.ERR_INVALID, "S must be >= 1"),
             (dict(N=0), _lib.ERR_INVALID, "N must be >= 1"),
             (dict(S=1, N=1), _lib.ERR_INVALID, "at least two draws"),
             (dict(ranges=-1), _lib.ERR_INVALID, "ranges must be"),
             (dict(ranges=65536), _lib.ERR_INVALID, "ranges must be"),
             (dict(Dt=4), _lib.ERR_INVALID, "state dimension"),
             (dict(family=_lib.GLM_SOFTMAX, state_dim=6, Dt=6), _lib.ERR_UNSUPPORTED, "softmax"),
             (dict(handle=2), _lib.ERR_UNSUPPORTED, "not a GLM handle")]
    for kw, code, text in cases:
        assert rc(**kw) == code, kw
        msg = _lib.last_error()
        assert text in msg, (kw, msg)
        if code == _lib.ERR_UNSUPPORTED:   # the rule is in the text
            assert "pbbi_pointwise_glm serves the handles of" in msg and "_glm_hier_dispersion" in msg
    import physicsbasedbayesianinference_amd as P
    with pytest.raises(ValueError, match="not built"):
        P.SoftmaxGLM.pointwise(None, None)


@pytest.mark.parametrize("name", ["binomial_trials", "poisson_full", "gaussian_sampled", "negbinomial_sampled"])
def test_pointwise_constants_against_scipy(name):
    """a_i log p(y_i | .) of scipy.stats minus the reference's ll is k_i, the same at every draw: trials and weights
    (with zeros) included."""
    from scipy import stats
    from physicsbasedbayesianinference_amd import glm
    _, sp, sdn, _ = kind(name)
    W = flat(sdn)[:, :7]
    ll, mu = (np.asarray(v, dtype=np.float64) for v in ref_ll(sp, W))
    a, y, n = sp["a"], sp["y"], sp["n"]
    fam = sp["family"]
    if fam == "logistic":
        full = stats.binom.logpmf(y[:, None], n[:, None], mu)
    elif fam == "poisson":
        full = stats.poisson.logpmf(y[:, None], mu)
    elif fam == "gaussian":
        full = stats.norm.logpdf(y[:, None], mu, np.exp(W[sp["trow"]])[None, :])
    else:
        phi = np.exp(W[sp["trow"]])[None, :]
        full = stats.nbinom.logpmf(y[:, None], phi, phi / (phi + mu))
    k = glm.pointwise_constants(fam, y, a, n if fam == "logistic" else None)
    assert np.any(a == 0.0) and np.all(k[a == 0.0] == 0.0)
    check(f"k {name} (scipy)", np.broadcast_to(k[:, None], ll.shape), a[:, None] * full - ll)
    check(f"k {name} (lgamma)", k, constants_ref(sp))
    assert np.all(glm.pointwise_constants("logistic", np.array([0.0, 1.0])) == 0.0)   # Bernoulli: log C(1, y) = 0


def test_pointwise_result_arithmetic():
    from scipy.special import logsumexp
    from physicsbasedbayesianinference_amd.glm import PointwiseResult
    rs = np.random.RandomState(3)
    ll = -np.abs(rs.standard_normal((6, 40))) * 3.0
    lppd_i = logsumexp(ll, axis=1) - np.log(40)
    p_i = ll.var(axis=1, ddof=1)
    r = PointwiseResult(lppd_i, ll.mean(axis=1), p_i, np.zeros(6), 40)
    assert r.T == 40
    assert r.lppd == pytest.approx(np.sum(np.log(np.mean(np.exp(ll), axis=1))), rel=1e-13)
    assert r.p_waic == pytest.approx(float(np.sum(p_i)), rel=1e-15)
    assert r.waic == pytest.approx(-2.0 * (r.lppd - r.p_waic), rel=1e-15)
    assert "waic" in repr(r)


@pytest.mark.parametrize("name", sorted(KINDS) + ["hier_nc"])
def test_pointwise_reference_is_finite(name):
    _, sp, sdn, ref = kind(name)
    assert sdn.shape[0] == S and sdn.shape[2] == N
    for v in ref:
        assert v.dtype == LD and np.all(np.isfinite(v))
    assert np.all(ref[2] >= 0)


def test_pointwise_special_cases_are_what_they_claim():
    """The stability case underflows a naive evaluation and its reference is finite; the overflow case has rows on both
    sides of exp's range and none near the edge."""
    X, y, i0, sdn, sp = stability_case()
    ll, mu = ref_ll(sp, flat(sdn))
    row = np.asarray(ll[i0], dtype=np.float64)
    assert row.max() - row.min() > 800 and -2900 < row.min() and row.max() < -1100 and abs(np.median(row) + 2000) < 200
    with np.errstate(divide="ignore"):
        assert np.log(np.sum(np.exp(row))) == -np.inf
    assert all(np.all(np.isfinite(v)) for v in ref_stats(ll, mu))
    _, sp, sdn, eta = overflow_case()
    assert 799.9 < eta.max() < 803.0 and not np.any((eta > 690) & (eta <= 720))
    assert np.sum((eta > 720) & (sp["a"] != 0.0)) >= 1 and np.sum(eta < 30) >= 3
    lse = reference(sp, sdn)[0]
    assert np.all(np.isfinite(lse))


# ------------------------------------------------------------------------------------------------ GPU
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


NAN_BITS = np.array([np.nan]).view(np.int64)[0]


def device_pointwise(lib, pot, sdn, ranges=0, want_var=True):
    """The four (M,) outputs of pbbi_pointwise_glm on (S, Dt, N) host slabs, called inside the NaN canary."""
    import torch
    d = _dev()
    s, Dt, n = sdn.shape
    M = pot.y.size
    buf = torch.full((sdn.size + GUARD,), float("nan"), dtype=torch.float64, device="cuda:0")
    buf[:sdn.size] = torch.from_numpy(np.array(sdn).ravel()).to("cuda:0")
    out = torch.full((4, M + 2 * PAD), float("nan"), dtype=torch.float64, device="cuda:0")
    ptr = [out[k, PAD:].data_ptr() for k in range(4)]
    lib.call("pbbi_pointwise_glm", pot.handle, buf.data_ptr(), s, Dt, n, ranges, ptr[0], ptr[1],
             ptr[2] if want_var else None, ptr[3], d.stream_ptr(0))
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    bits = host.view(np.int64)
    assert np.all(bits[:, :PAD] == NAN_BITS) and np.all(bits[:, PAD + M:] == NAN_BITS), "stores outside [0, M)"
    if not want_var:
        assert np.all(bits[2] == NAN_BITS), "var_out = NULL was written"
    assert np.all(buf[sdn.size:].cpu().numpy().view(np.int64) == NAN_BITS), "the guard behind the slabs was written"
    return host[:, PAD:PAD + M].copy()


def check_all(name, got, ref, want_var=True):
    for k, what in enumerate(("lse", "mean", "var", "mu")):
        if what == "var" and not want_var:
            continue
        check(f"{what} {name}", got[k], ref[k])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(KINDS))
def test_pointwise_every_kind_matches_reference(P, lib, name):
    make, sp, sdn, ref = kind(name)
    pot = make(P)
    got = device_pointwise(lib, pot, sdn)
    check_all(name, got, ref)
    zero = sp["a"] == 0.0
    if zero.any():     # weight 0: ll = 0 exactly, and the fitted mean is formed all the same
        assert np.all(np.abs(got[0][zero] - np.log(float(N * S))) < 1e-14)     # log(T), to the last bit of the device's log
        assert np.all(got[1][zero] == 0.0) and np.all(got[2][zero] == 0.0)
        assert np.all(got[3][zero] != 0.0)


@pytest.mark.gpu
def test_pointwise_hier_log_scale_rows_do_not_matter(P, lib):
    make, sp, sdn, ref = kind("hier")
    pot = make(P)
    a = device_pointwise(lib, pot, sdn)
    inf = sdn.copy()
    inf[:, 5:, :] = np.inf
    inf[0, 6, ::2] = -np.inf
    b = device_pointwise(lib, pot, inf)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    wide = np.concatenate([sdn, np.full((S, 3, N), np.nan)], axis=1)     # Dt > the state dimension: ignored rows
    c = device_pointwise(lib, pot, wide)
    assert np.array_equal(a.view(np.int64), c.view(np.int64))


@pytest.mark.gpu
def test_pointwise_noncentred_through_the_method(P, lib):
    """Sampler coordinates in, as a NumPy array and as the (D, N, S) device view; natural-scale reference."""
    import torch
    make, sp, sdn, ref = kind("hier_nc")
    pot = make(P)
    k = constants_ref(sp)
    T = N * S
    for samples in (np.ascontiguousarray(sdn.transpose(1, 2, 0)),
                    torch.from_numpy(np.array(sdn)).to("cuda:0").permute(1, 2, 0)):
        r = pot.pointwise(samples)
        assert r.T == T
        check("nc lppd_i", r.lppd_i, ref[0] - np.log(LD(T)) + k)
        check("nc mean_ll_i", r.mean_ll_i, ref[1] + k)
        check("nc p_waic_i", r.p_waic_i, ref[2])
        check("nc mu_i", r.mu_i, ref[3] * sp["n"])
        assert r.waic == pytest.approx(-2.0 * (r.lppd - r.p_waic))
    # the centred handle of the same data on the natural-scale draws: the same likelihood
    nat = np.stack([t_nc.natural_np(sp["kw"], q) for q in sdn])
    rc = P.HierarchicalGLM(**sp["kw"]).pointwise(np.ascontiguousarray(nat.transpose(1, 2, 0)))
    check("centred == noncentred", rc.lppd_i, r.lppd_i)
    with pytest.raises(ValueError):
        pot.pointwise(np.zeros((3, 10)))        # fewer rows than the state


@pytest.mark.gpu
@pytest.mark.parametrize("M", [5, 16, 203])
def test_pointwise_draw_count_and_tail_shapes(P, lib, M):
    X, y, w, rs = t_plain.problem("logistic", M, 5, DATA_SEED)
    pot = P.GLM(X, y)
    sp = spec_of("logistic", dict(X=X, y=y), 5)
    for n in (1, 15, 17, 37, 65):
        for s in (1, 2):
            sdn = _slabs(lambda k: t_plain.start(w, k, rs), n, s)
            want_var = n * s >= 2
            got = device_pointwise(lib, pot, sdn, want_var=want_var)
            check_all(f"M={M} N={n} S={s}", got, reference(sp, sdn), want_var)
    with pytest.raises(lib.PbbiError) as e:     # one draw and a variance asked for
        device_pointwise(lib, pot, _slabs(lambda k: t_plain.start(w, k, rs), 1, 1))
    assert e.value.code == lib.ERR_INVALID


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["logistic", "poisson_full"])
def test_pointwise_ranges(P, lib, name):
    make, sp, sdn, ref = kind(name)
    pot = make(P)
    for ranges in (1, 2, 7):
        a = device_pointwise(lib, pot, sdn, ranges=ranges)
        b = device_pointwise(lib, pot, sdn, ranges=ranges)
        check_all(f"{name} ranges={ranges}", a, ref)
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), ranges
    many = device_pointwise(lib, pot, sdn, ranges=64)      # more ranges than tiles: empty ranges merge as nothing
    check_all(f"{name} ranges=64", many, ref)


@pytest.mark.gpu
def test_pointwise_lse_is_stable(P, lib):
    X, y, i0, sdn, sp = stability_case()
    ref = reference(sp, sdn)
    got = device_pointwise(lib, P.GLM(X, y), sdn)
    assert np.isfinite(got[0][i0]) and got[0][i0] < -1100
    check_all("stability", got, ref)


@pytest.mark.gpu
def test_pointwise_non_finite_draws(P, lib):
    make, sp, sdn, eta = overflow_case()
    ref = reference(sp, sdn)          # longdouble holds exp(800): every reference value is finite
    got = device_pointwise(lib, make(P), sdn)
    hit = (eta > 720) & (sp["a"] != 0.0)
    calm = eta < 30
    assert hit.sum() >= 1 and calm.sum() >= 3
    check("lse, overflowed draw", got[0], ref[0])
    assert not np.any(np.isfinite(got[1][hit])) and not np.any(np.isfinite(got[2][hit]))
    check("mean, calm rows", got[1][calm], ref[1][calm])      # (rows in between: exp(eta)^2 leaves double's range)
    check("var, calm rows", got[2][calm], ref[2][calm])
    check("mu, calm rows", got[3][calm], ref[3][calm])
    zero = sp["a"] == 0.0
    assert np.all(got[1][zero] == 0.0) and np.all(got[2][zero] == 0.0)
    # a column of NaN coefficients: every output of every row (no row of this handle has weight 0)
    make, sp, sdn, _ = kind("logistic")
    bad = sdn.copy()
    bad[2, :, 140] = np.nan
    got = device_pointwise(lib, make(P), bad)
    assert np.all(np.isnan(got))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["logistic", "poisson_full", "gaussian_held"])
def test_pointwise_device_against_device(P, lib, name):
    """sum_i mean_i = -mean_t (U_t - prior_t): U from pbbi_potential_eval on the same draws, the prior on the host.
    gaussian_held: a dispersion family (held: the state is the coefficients, under the full model's Gaussian prior)."""
    make, sp, sdn = _dispersion("gaussian", False) if name == "gaussian_held" else kind(name)[:3]
    pot = make(P)
    W = flat(sdn)
    if name == "logistic":
        prior = 0.5 * np.sum(W * W, axis=0)
    else:
        prior = 0.5 * np.sum(pot.prior_precision[:, None] * (W - pot.prior_mean[:, None]) ** 2, axis=0)
    U = pot(np.ascontiguousarray(W))
    got = device_pointwise(lib, pot, sdn)
    check(f"sum mean {name}", np.sum(got[1]), -np.mean(U - prior))


@pytest.mark.gpu
def test_pointwise_end_to_end_waic(P, lib):
    from scipy.constants import k as kB
    X, _, w, rs = t_plain.problem("logistic", 406, 5, DATA_SEED)
    y = (rs.uniform(size=406) < 1.0 / (1.0 + np.exp(-3.0 * (X @ w)))).astype(np.float64)     # a signal worth fitting
    Xt, yt, Xh, yh = X[:203], y[:203], X[203:], y[203:]
    out = {}
    for label, Xa, Xb in (("fit", Xt, Xh), ("null", np.ones((203, 1)), np.ones((203, 1)))):
        pot, held = P.GLM(Xa, yt), P.GLM(Xb, yh)
        hmc = P.HMC(P.Ensemble(Xa.shape[1], 256), 0.8, 0.1, None, potential=pot, rng="philox", seed=13, verbose=False)
        s, _ = hmc.getSamples(40, 1 / kB, 1.0, device_output=True)
        assert tuple(s.shape) == (Xa.shape[1], 256, 40)
        keep = s[:, :, 20:]
        sdn = keep.permute(2, 0, 1).cpu().numpy()
        T = 20 * 256
        for which, p, Xs, ys in (("train", pot, Xa, yt), ("held", held, Xb, yh)):
            r = p.pointwise(keep)
            ref = reference(spec_of("logistic", dict(X=Xs, y=ys), Xs.shape[1]), sdn)
            assert r.T == T
            check(f"{label} {which} lppd_i", r.lppd_i, ref[0] - np.log(LD(T)))
            check(f"{label} {which} p_waic_i", r.p_waic_i, ref[2])
            check(f"{label} {which} mu_i", r.mu_i, ref[3])
            out[label, which] = (r, float(-2 * (np.sum(ref[0] - np.log(LD(T))) - np.sum(ref[2]))))
            assert r.waic == pytest.approx(out[label, which][1], rel=1e-9)
    assert out["fit", "train"][1] < out["null", "train"][1]              # the reference's ordering
    assert out["fit", "train"][0].waic < out["null", "train"][0].waic    # ... and the device's
    assert out["fit", "held"][0].lppd > out["null", "held"][0].lppd
