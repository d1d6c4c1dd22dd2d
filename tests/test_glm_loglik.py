"""The likelihood energy of each draw on the device (csrc/kernels_glm_loglik.hip, pbbi_loglik_glm, `loglik` of GLM /
DispersionGLM / HierarchicalGLM / HierarchicalDispersionGLM): ulik[s, n] = sum_i U_i(draw), no prior term.

Reference: test_glm_pointwise.ref_ll -- NumPy in `longdouble` on the host copy of the same draws (log Gamma alone in double),
exactly 0 on a row of weight 0 -- summed over the observations in longdouble.  The data are the generators of the existing GLM
test files (the kinds of test_glm_pointwise.py plus a held Gaussian dispersion, a penalty handle and the two
hierarchical-dispersion parametrisations).

Tolerance: test_glm.py's TOL = 1e-10 relative to max(1, max|reference|), through its `check`.  Bit-for-bit claims are compared
on the int64 view.  Every device call runs inside a NaN canary: the slabs are followed by a NaN guard region in the same
allocation and the (S * N) output sits in the middle of a longer NaN-filled array whose other elements must keep their bits.

A NaN offset cannot be put on a handle (the create entries refuse a non-finite offset), so "a NaN on a row of weight 0" is
made where it can arise, inside the kernel: finite inputs (an offset of 1e308 and a product x . w of 1e308 on the weight-0 rows
alone) whose sum is eta = +inf there, so that c * b(eta) = 0 * inf = NaN before the select, in the logistic and in the Poisson
family alike.
"""
import functools

import numpy as np
import pytest

import test_glm_dispersion as t_disp
import test_glm_hier as t_hier
import test_glm_hier_dispersion as t_hd
import test_glm_hier_noncentred as t_nc
import test_glm_hier_penalty as t_pen
import test_glm_model as t_model
import test_glm_pointwise as t_pw
from test_glm import TOL, check, problem, rel  # noqa: F401  (rel: through check)

LD = np.longdouble
N, S = t_pw.N, t_pw.S
DATA_SEED = t_pw.DATA_SEED
PAD, GUARD = 32, 4096
NAN_BITS = np.array([np.nan]).view(np.int64)[0]


def ref_ulik(sp, nat):
    """(S, N) longdouble: minus the summed reference log-likelihood of the natural-scale slabs (S, Dt, N)."""
    ll, _ = t_pw.ref_ll(sp, t_pw.flat(nat))
    return (-ll.sum(axis=0)).reshape(nat.shape[0], nat.shape[2])


def _gaussian_held():
    kw, w, theta, rs = t_disp.problem("gaussian", 40, 5, DATA_SEED)
    return ((lambda P: t_disp.make(P, kw, False, theta)), t_pw.spec_of("gaussian", kw, 5, -1, float(np.log(np.exp(theta)))),
            t_pw._slabs(lambda k: t_disp.start(w, theta, k, rs, spread=0.1, sampled=False)))


def _penalty():
    kw, w, t, rs = t_pen.problem("poisson", 40, 5, 2, DATA_SEED)
    return (lambda P: P.HierarchicalGLM(**kw)), t_pw.spec_of("poisson", kw, 5), t_pw._slabs(lambda k: t_pen.start(w, t, k, rs, 0.1))


def _hier_disp(family, par, sampled):
    """Slabs in SAMPLER coordinates; the spec carries kw and par for natural_np."""
    kw, w, t, theta, rs = t_hd.problem(family, 40, 5, 2, DATA_SEED)
    sp = t_pw.spec_of(family, kw, 5, 7 if sampled else -1, None if sampled else float(np.log(np.exp(theta))))
    sp["hd_kw"] = kw
    return ((lambda P: t_hd.make(P, kw, par, sampled, theta)), sp,
            t_pw._slabs(lambda k: t_hd.start(kw, par, w, t, theta, k, rs, spread=0.1, sampled=sampled)))


EXTRA = {
    "gaussian_held": _gaussian_held,
    "penalty": _penalty,
    "hd_gaussian_c": lambda: _hier_disp("gaussian", "centred", True),
    "hd_negbinomial_nc": lambda: _hier_disp("negbinomial", "noncentred", False),
}
ALL_KINDS = sorted(t_pw.KINDS) + ["hier_nc"] + sorted(EXTRA)


@functools.lru_cache(maxsize=None)
def kind(name):
    """(make, spec, slabs in sampler coordinates, natural-scale slabs, reference ulik (S, N)): built once, never written to."""
    if name in EXTRA:
        make, sp, sdn = EXTRA[name]()
        nat = np.stack([t_hd.natural_np(sp["hd_kw"], q) for q in sdn]) if name == "hd_negbinomial_nc" else sdn
    else:
        make, sp, sdn, _ = t_pw.kind(name)
        nat = np.stack([t_nc.natural_np(sp["kw"], q) for q in sdn]) if name == "hier_nc" else sdn
    ref = ref_ulik(sp, nat)
    ref.setflags(write=False)
    return make, sp, sdn, nat, ref


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", ALL_KINDS)
def test_loglik_reference_is_finite(name):
    _, sp, sdn, nat, ref = kind(name)
    assert ref.dtype == LD and ref.shape == (S, N) and np.all(np.isfinite(ref))


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


def device_ulik(lib, pot, nat, ranges=0):
    """(S, N) of pbbi_loglik_glm on (S, Dt, N) natural-scale host slabs, called inside the NaN canary."""
    import torch
    s, Dt, n = nat.shape
    buf = torch.full((nat.size + GUARD,), float("nan"), dtype=torch.float64, device="cuda:0")
    buf[:nat.size] = torch.from_numpy(np.array(nat).ravel()).to("cuda:0")
    out = torch.full((s * n + 2 * PAD,), float("nan"), dtype=torch.float64, device="cuda:0")
    lib.call("pbbi_loglik_glm", pot.handle, buf.data_ptr(), s, Dt, n, ranges, out[PAD:].data_ptr(), _dev().stream_ptr(0))
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    bits = host.view(np.int64)
    assert np.all(bits[:PAD] == NAN_BITS) and np.all(bits[PAD + s * n:] == NAN_BITS), "stores outside [0, S * N)"
    assert np.all(buf[nat.size:].cpu().numpy().view(np.int64) == NAN_BITS), "the guard behind the slabs was written"
    return host[PAD:PAD + s * n].reshape(s, n).copy()


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL_KINDS)
def test_loglik_every_kind_matches_reference(P, lib, name):
    """Every served kind of handle; logistic / logistic17 / logistic50 / logistic128 are NT = 1, 2, 4, 8 (D = 5, 17, 50, 128)."""
    make, sp, sdn, nat, ref = kind(name)
    check(name, device_ulik(lib, make(P), nat), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [5, 20, 40, 100])
def test_loglik_tile_counts(P, lib, D):
    """NT = 1, 2, 4, 8 for logistic at D = 5, 20, 40, 100, on the full model (weights with zeros, offsets, trials)."""
    kw, w, rs = t_model.problem("logistic", 203, D, DATA_SEED)
    sdn = t_pw._slabs(lambda k: t_model.start(w, k, rs, spread=0.1), 37, 2)
    check(f"D={D}", device_ulik(lib, P.GLM(**kw), sdn), ref_ulik(t_pw.spec_of("logistic", kw, D), sdn))


@pytest.mark.gpu
@pytest.mark.parametrize("M", [5, 16, 203])
def test_loglik_draw_count_tail_and_padding_rows(P, lib, M):
    """N in {1, 15, 17, 37, 65} x S in {1, 2}; M = 5 and 203 put padding rows inside a block and inside the 4-block padding.  At a
    zero draw the plain model is M log 2 exactly: a padding row (c = 1, d = 0, eta = 0) must not add its log 2."""
    X, y, w, rs = problem("logistic", M, 5, DATA_SEED)
    pot = P.GLM(X, y)
    sp = t_pw.spec_of("logistic", dict(X=X, y=y), 5)
    for n in (1, 15, 17, 37, 65):
        for s in (1, 2):
            sdn = t_pw._slabs(lambda k: t_pw.t_plain.start(w, k, rs), n, s)
            check(f"M={M} N={n} S={s}", device_ulik(lib, pot, sdn), ref_ulik(sp, sdn))
    zero = np.zeros((2, 5, 17))
    got = device_ulik(lib, pot, zero)
    check(f"M={M} zero draw", got, np.full((2, 17), M * np.log(LD(2))))
    Xp, yp, _, _ = problem("poisson", M, 5, DATA_SEED)
    check(f"M={M} zero draw, poisson", device_ulik(lib, P.GLM(Xp, yp, family="poisson"), zero), np.full((2, 17), float(M)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["logistic", "poisson_full", "logistic128"])
def test_loglik_ranges(P, lib, name):
    """ranges 1, 2, 7 and more than there are blocks (M = 203: 16 blocks; M = 300: 20): two runs bit-equal, every value within
    TOL of the reference and so of each other."""
    make, sp, sdn, nat, ref = kind(name)
    pot = make(P)
    for ranges in (0, 1, 2, 7, 64):
        a = device_ulik(lib, pot, nat, ranges=ranges)
        b = device_ulik(lib, pot, nat, ranges=ranges)
        check(f"{name} ranges={ranges}", a, ref)
        assert same_bits(a, b), ranges


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["logistic", "poisson"])
def test_loglik_weight_zero_rows(P, lib, family):
    """The model with its weight-0 rows deleted gives the same values within TOL; a non-finite term on such a row (see the
    module text) changes no bit."""
    kw, w, rs = t_model.problem(family, 203, 8, DATA_SEED)
    a = kw["weights"]
    assert np.sum(a == 0.0) >= 2
    sdn = t_pw._slabs(lambda k: t_model.start(w, k, rs, spread=0.1), 37, 2)
    full = device_ulik(lib, P.GLM(**kw), sdn)
    keep = a != 0.0
    cut = {k: (v[keep] if isinstance(v, np.ndarray) and v.shape[:1] == (203,) else v) for k, v in kw.items()}
    check(f"{family}: rows deleted", device_ulik(lib, P.GLM(**cut), sdn), full)
    check(f"{family}: reference", full, ref_ulik(t_pw.spec_of(family, kw, 8), sdn))
    # a NaN on the weight-0 rows, for BOTH families (module text): one more column that is 1 on those rows and 0 elsewhere, its
    # coefficient 1e308 in every draw, and an offset of 1e308 there -- eta = 1e308 + 1e308 = inf on those rows alone, so c * b(eta)
    # is 0 * inf = NaN before the select; on every other row the column adds 0 * 1e308 = 0 exactly and no bit changes
    o = np.zeros(203) if kw.get("offset") is None else kw["offset"]
    Xh = np.hstack([kw["X"], (~keep)[:, None].astype(np.float64)])
    hot = dict(kw, X=Xh, offset=np.where(keep, o, 1e308), prior_precision=np.r_[kw["prior_precision"], 1.0],
               prior_mean=np.r_[kw["prior_mean"], 0.0])
    sdn_h = np.concatenate([sdn, np.full((2, 1, 37), 1e308)], axis=1)
    with np.errstate(over="ignore", invalid="ignore"):
        eta = Xh @ sdn_h[0] + hot["offset"][:, None]
        assert np.all(np.isposinf(eta[~keep])) and np.all(np.isfinite(eta[keep])) and np.all(np.isnan(0.0 * eta[~keep]))
    assert same_bits(device_ulik(lib, P.GLM(**hot), sdn_h), full)


@pytest.mark.gpu
def test_loglik_other_rows_do_not_matter(P, lib):
    """t rows at +-inf and extra rows past the state change no bit."""
    make, sp, sdn, nat, ref = kind("hier")
    pot = make(P)
    a = device_ulik(lib, pot, nat)
    inf = nat.copy()
    inf[:, 5:, :] = np.inf
    inf[0, 6, ::2] = -np.inf
    assert same_bits(a, device_ulik(lib, pot, inf))
    wide = np.concatenate([nat, np.full((S, 3, N), np.nan)], axis=1)
    assert same_bits(a, device_ulik(lib, pot, wide))


@pytest.mark.gpu
def test_loglik_non_finite_draws(P, lib):
    """ll = -inf gives +inf and a NaN draw gives NaN, for that draw only: every other draw keeps its bits."""
    make, sp, sdn, eta = t_pw.overflow_case()          # the full Poisson model, draw (slab 1, chain 7) with eta = 800
    pot = make(P)
    clean = device_ulik(lib, pot, t_pw.kind("poisson_full")[2])
    got = device_ulik(lib, pot, sdn)
    assert got[1, 7] == np.inf
    mask = np.ones(got.shape, bool)
    mask[1, 7] = False
    assert same_bits(got[mask], clean[mask])
    bad = np.array(t_pw.kind("poisson_full")[2])
    bad[2, :, 140] = np.nan
    got = device_ulik(lib, pot, bad)
    assert np.isnan(got[2, 140])
    mask = np.ones(got.shape, bool)
    mask[2, 140] = False
    assert same_bits(got[mask], clean[mask])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["logistic", "poisson_full", "gaussian_held"])
def test_loglik_device_against_device(P, lib, name):
    """ulik + prior (NumPy) = U of pbbi_potential_eval on the same draws, on the plain and the full model and on a dispersion
    family (held: the state is the coefficients, under the full model's Gaussian prior)."""
    make, sp, sdn, nat, _ = kind(name)
    pot = make(P)
    W = t_pw.flat(nat)
    if name == "logistic":
        prior = 0.5 * np.sum(W * W, axis=0)
    else:
        prior = 0.5 * np.sum(pot.prior_precision[:, None] * (W - pot.prior_mean[:, None]) ** 2, axis=0)
    U = pot(np.ascontiguousarray(W))
    check(f"ulik + prior {name}", device_ulik(lib, pot, nat).ravel() + prior, U)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["binomial_trials", "hier_nc", "hd_negbinomial_nc", "gaussian_sampled"])
def test_loglik_through_the_method(P, lib, name):
    """`pot.loglik`: sampler coordinates in (non-centred input goes through to_natural), the constants k_i added, (N, S) out;
    the (D, N, S) device view and the NumPy array agree bit for bit, device_output keeps the same bits on the device."""
    import torch
    make, sp, sdn, nat, ref = kind(name)
    pot = make(P)
    k = np.sum(t_pw.constants_ref(sp).astype(LD))
    host = np.ascontiguousarray(np.array(sdn).transpose(1, 2, 0))
    view = torch.from_numpy(np.array(sdn)).to("cuda:0").permute(1, 2, 0)
    a, b = pot.loglik(host), pot.loglik(view)
    assert a.shape == (N, S) and same_bits(a, b)     # (host input is uploaded before to_natural: the same torch ops)
    check(f"loglik {name}", a, (k - ref).T)
    d = pot.loglik(view, device_output=True)
    assert d.is_cuda and tuple(d.shape) == (N, S) and same_bits(d.cpu().numpy(), b)
    check(f"loglik {name} ranges=3", pot.loglik(host, ranges=3), (k - ref).T)
    one = pot.loglik(host[:, :, 0])
    assert one.shape == (N, 1) and same_bits(one[:, 0], a[:, 0])
    with pytest.raises(ValueError):
        pot.loglik(np.zeros((3, 10)))        # fewer rows than the state


@pytest.mark.gpu
def test_loglik_refuses_softmax_and_other_handles(P, lib):
    import torch
    rs = np.random.RandomState(0)
    X = rs.standard_normal((20, 3))
    buf = torch.zeros(64, dtype=torch.float64, device="cuda:0")
    for pot in (P.SoftmaxGLM(X, rs.randint(0, 3, 20).astype(float)), P.StandardGaussian(3)):
        with pytest.raises(lib.PbbiError) as e:
            lib.call("pbbi_loglik_glm", pot.handle, buf.data_ptr(), 1, pot.numDimensions, 4, 0, buf.data_ptr(), None)
        assert e.value.code == lib.ERR_UNSUPPORTED
    assert not hasattr(P.SoftmaxGLM, "loglik")
