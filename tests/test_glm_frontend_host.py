"""The Python front end of the GLM classes (glm.py), held to a census recorded from the commit before its argument checks and
its state layout were stated once: no GPU, no device.

`_lib.call` is replaced by a function that records and returns for the `pbbi_potential_create*` entries and forwards every
other name to the library (the host packers run on the CPU), so with `device=0` every constructor runs to its end.  Per route
the census keeps the entry called, every scalar argument, a SHA-256 of what every pointer argument points to (lengths from
ENTRIES below, which follows include/pbbi.h), `vars(pot)` without the handle and what `_prior_layout(pot)` returns; per
rejection row the exception's type and its full text.  tests/golden/glm_frontend_census.json is that census of the PARENT's
glm.py (`python tests/test_glm_frontend_host.py --record OUT --glm PARENT_GLM_PY`, which also lists the `raise` lines no row
reached); the test replays it on the code as it is.  The one difference allowed is WORDING: `_validate` took over the text the
other three statements of the X rule already shared.
"""
import contextlib
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glm_frontend_census.json")

_OLD_X = ("X must be 2-D: (M, D)", "X must have at least one row and one column")
_NEW_X = "X must be 2-D: (M, D) with at least one row and one column"
WORDING = {"GLM: X 1-D": (_OLD_X[0], _NEW_X), "GLM: X without rows": (_OLD_X[1], _NEW_X)}     # row -> (parent's text, today's)

# the arguments of every create entry, in order: a name alone is a scalar; (name, length) a const double* of that many entries
# (the length a function of the call's scalars), (name, length, "i") a const int32_t*; "handle" is the out-pointer
_M, _D, _MD = (lambda s: s["M"]), (lambda s: s["D"]), (lambda s: s["M"] * s["D"])
_TP, _GR = ("log_scale_prior", lambda s: 2 * s["J"]), ("groups", _D, "i")
_XY, _END = ["D", "M", ("X", _MD), ("y", _M), "family"], ["dtype", "device", "handle"]
_OBS = [("weights", _M), ("offset", _M), ("trials", _M)]
_HIER = _XY + _OBS + [("prior_precision", _D), ("prior_mean", _D), _GR, "J", _TP]
ENTRIES = {
    "pbbi_potential_create_glm": _XY + ["prior_precision"] + _END,
    "pbbi_potential_create_glm_ex": _XY + _OBS + [("prior_precision", _D), ("prior_mean", _D)] + _END,
    "pbbi_potential_create_glm_softmax": ["D", "K", "M", ("X", _MD), ("y", _M), ("prior_precision", _D)] + _END,
    "pbbi_potential_create_glm_dispersion": _XY + _OBS[:2] + [("prior_precision", lambda s: s["D"] + s["sample"]),
                                                              ("prior_mean", lambda s: s["D"] + s["sample"]), "sample",
                                                              "theta"] + _END,
    "pbbi_potential_create_glm_ordinal": ["D", "K", "M", ("X", _MD), ("y", _M)] + _OBS[:2] + [
        ("prior_precision", lambda s: s["D"] + s["K"] - 1), ("prior_mean", lambda s: s["D"] + s["K"] - 1)] + _END,
    "pbbi_potential_create_glm_hier": _HIER + _END,
    "pbbi_potential_create_glm_hier_ex": _HIER + ["parametrisation"] + _END,
    "pbbi_potential_create_glm_hier_q": _HIER + [("penalty", lambda s: s["D"] * s["D"]), ("penalty_rank", lambda s: s["J"])] + _END,
    "pbbi_potential_create_glm_hier_dispersion": _XY + _OBS[:2] + [("prior_precision", _D), ("prior_mean", _D), _GR, "J", _TP,
                                                                   "parametrisation", "sample", "theta",
                                                                   ("log_dispersion_prior", lambda s: 2)] + _END,
}


def _sha(data):
    return hashlib.sha256(data).hexdigest()


def _enc(v):
    """A value of vars(pot) or of _prior_layout's tuple as JSON: arrays as dtype, shape and hash, sequences item by item."""
    if isinstance(v, np.ndarray):
        return {"dtype": str(v.dtype), "shape": list(v.shape), "sha256": _sha(np.ascontiguousarray(v).tobytes())}
    if isinstance(v, (list, tuple)):
        return [_enc(x) for x in v]
    return repr(v)


@contextlib.contextmanager
def recorded_creates(calls):
    """`_lib.call` records the create entries into `calls` (the pointers read while their arrays are alive) and makes no handle."""
    from physicsbasedbayesianinference_amd import _lib
    real = _lib.call

    def call(name, *args):
        if not name.startswith("pbbi_potential_create"):
            return real(name, *args)
        spec = ENTRIES[name]
        assert len(spec) == len(args), name
        scalars = {a: v for a, v in zip(spec, args) if isinstance(a, str) and a != "handle"}
        rec = {"entry": name}
        for a, v in zip(spec, args):
            if a == "handle":
                continue
            if isinstance(a, str):
                rec[a] = repr(v) if isinstance(v, float) else int(v)
            elif v is None:
                rec[a[0]] = None
            else:
                size = a[1](scalars) * (4 if a[2:] == ("i",) else 8)
                rec[a[0]] = _sha(C.string_at(C.cast(v, C.c_void_p).value, size))
        calls.append(rec)

    _lib.call = call
    try:
        yield
    finally:
        _lib.call = real


def _data():
    rs = np.random.RandomState(0)
    M, D = 12, 3
    d = dict(M=M, D=D, X=rs.standard_normal((M, D)), yb=(rs.uniform(size=M) < 0.5).astype(float),
             yc=rs.poisson(2.0, M).astype(float), yr=rs.standard_normal(M), ones=np.ones(M), at2=np.arange(M) == 2)
    d["yp"] = np.exp(d["yr"])
    d["w"] = rs.uniform(0.5, 2.0, M)
    d["w"][5] = 0.0
    d["o"] = 0.3 * rs.standard_normal(M)
    d["n"] = rs.randint(1, 5, M).astype(float)
    d["yn"] = np.minimum(d["yc"], d["n"])
    d["lam"], d["mu"] = np.array([0.0, 0.5, 4.0]), np.array([0.1, -0.2, 0.3])
    d["labels"] = np.array(list("abcabcabcabd"))
    d["g"], d["g2"] = np.array([-1, 0, 0]), np.array([0, 1, 1])
    return type("Data", (), d)


def routes(glm):
    """name -> a function that builds the potential (device 0, under `recorded_creates`)."""
    d = _data()
    X, lam, mu, w, o = d.X, d.lam, d.mu, d.w, d.o
    H, HD = glm.HierarchicalGLM, glm.HierarchicalDispersionGLM
    full = dict(prior_precision=lam, prior_mean=mu, weights=w, offset=o)
    out = {
        "GLM plain": lambda: glm.GLM(X, d.yb, device=0),
        "GLM plain poisson": lambda: glm.GLM(X, d.yc, "poisson", 0.25, device=0),
        "GLM full": lambda: glm.GLM(X, d.yn, "logistic", trials=d.n, device=0, **full),
        "GLM offset alone": lambda: glm.GLM(X, d.yc, "poisson", 2.0, offset=o, device=0),
        "SoftmaxGLM": lambda: glm.SoftmaxGLM(X, np.arange(d.M) % 3.0, device=0),
        "SoftmaxGLM classes and precisions": lambda: glm.SoftmaxGLM(X, np.arange(d.M) % 3.0, classes=4, prior_precision=lam, device=0),
        "DispersionGLM gaussian": lambda: glm.DispersionGLM(X, d.yr, "gaussian", device=0),
        "DispersionGLM negbinomial": lambda: glm.DispersionGLM(X, d.yc, log_dispersion_prior=(0.5, 2.0), device=0, **full),
        "DispersionGLM gamma": lambda: glm.DispersionGLM(X, d.yp, "gamma", weights=w, offset=o, device=0),
        "DispersionGLM held": lambda: glm.DispersionGLM(X, d.yr, "gaussian", dispersion=0.7, prior_precision=lam, device=0),
        "HierarchicalGLM centred": lambda: H(X, d.yn, groups=d.g, trials=d.n, device=0, **full),
        "HierarchicalGLM noncentred": lambda: H(X, d.yc, "poisson", groups=d.g2, log_scale_prior=((0.0, 1.0), (0.5, 2.0)),
                                                parametrisation="noncentred", offset=o, device=0),
        "HierarchicalGLM penalty": lambda: H(X, d.yb, groups=d.g2, penalty={1: H.random_walk_penalty(2, 1)}, device=0),
        "HierarchicalGLM penalty rank": lambda: H(X, d.yb, groups=d.g, penalty=[np.array([[2.0, -1.0], [-1.0, 2.0]])],
                                                  penalty_rank=[1], prior_mean=mu, device=0),
        "HierarchicalGLM random intercepts": lambda: H.with_random_intercepts(X, d.yb, d.labels, prior_precision=lam, groups=d.g,
                                                                              device=0),
        "HierarchicalGLM random intercepts penalty": lambda: H.with_random_intercepts(
            X, d.yc, d.labels, family="poisson", penalty=H.random_walk_penalty(4, 2), penalty_rank=2, prior_mean=mu, device=0),
        "HierarchicalDispersionGLM random intercepts": lambda: HD.with_random_intercepts(
            X, d.yr, d.labels, parametrisation="noncentred", dispersion=1.5, weights=w, device=0),
    }
    for K in (2, 5, 8):
        y = np.arange(d.M) % float(K)
        out["OrdinalGLM K=%d" % K] = lambda y=y: glm.OrdinalGLM(X, y, device=0, **full)
        cp = np.c_[0.1 * np.arange(K - 1.0), 0.5 + np.arange(K - 1.0)]
        out["OrdinalGLM K=%d cutpoint rows" % K] = lambda y=y, K=K, cp=cp: glm.OrdinalGLM(X, y, categories=K, cutpoint_prior=cp, device=0)
    for family, y in (("gaussian", d.yr), ("negbinomial", d.yc)):
        for par in ("centred", "noncentred"):
            for disp in ("sample", 0.7):
                kw = dict(family=family, groups=d.g2 if par == "centred" else d.g, parametrisation=par, dispersion=disp, device=0)
                if disp == "sample":
                    kw.update(full, log_dispersion_prior=(0.25, 0.5))
                out["HierarchicalDispersionGLM %s %s %s" % (family, par, disp)] = lambda y=y, kw=kw: HD(X, y, **kw)
    return out


def rejections(glm):
    """name -> a function that must raise: at least one row per `raise` of glm.py that is reachable without a device, and some
    rows with two faults, which say which is reported."""
    d = _data()
    M, D, X, at2, ones, nan, inf = d.M, d.D, d.X, d.at2, d.ones, np.nan, np.inf
    H, HD = glm.HierarchicalGLM, glm.HierarchicalDispersionGLM
    rows = {}

    def over(cls, base, table):
        for name, kw in table.items():
            rows["%s: %s" % (cls.__name__, name)] = lambda kw=dict(base, **kw): cls(device=0, **kw)

    def each(prefix, fn, table):
        for name, args in table.items():
            kw = isinstance(args[-1], dict)              # a trailing dict holds the keywords
            rows["%s: %s" % (prefix, name)] = lambda a=args[:-1] if kw else args, kw=args[-1] if kw else {}: fn(*a, **kw)

    xy = {"X 1-D": dict(X=X[:, 0]), "X without rows": dict(X=np.ones((0, D)), y=np.ones(0)),
          "X without columns": dict(X=np.ones((M, 0))), "y short": dict(y=np.zeros(M - 1)), "y 2-D": dict(y=np.zeros((M, 1))),
          "X nan": dict(X=np.where(at2[:, None], nan, X)), "y inf": dict(y=np.where(at2, inf, 0.0))}
    obs = {"weights short": dict(weights=ones[:-1]), "weights nan": dict(weights=np.where(at2, nan, ones)),
           "weights negative": dict(weights=np.where(at2, -0.5, ones)), "offset 2-D": dict(offset=np.zeros((M, 1))),
           "offset inf": dict(offset=np.where(at2, inf, 0.0)),
           "weights negative + offset inf": dict(weights=-ones, offset=np.full(M, inf))}
    lam = {"precision inf": dict(prior_precision=inf), "precision nan": dict(prior_precision=nan),
           "precision negative": dict(prior_precision=-1.0), "precision short": dict(prior_precision=np.ones(D + 1)),
           "precision 2-D": dict(prior_precision=np.ones((D, 1))), "precision entry nan": dict(prior_precision=np.array([1.0, nan, 1.0])),
           "precision entry negative": dict(prior_precision=np.array([1.0, -1.0, 1.0]))}
    mean = {"mean short": dict(prior_mean=np.zeros(D - 1)), "mean nan": dict(prior_mean=np.array([0.0, nan, 0.0]))}
    f32 = {"float32": dict(dtype="float32"), "float16": dict(dtype="float16")}

    # ---- GLM
    over(glm.GLM, dict(X=X, y=d.yb), {        # (two rows with a misshapen X, those of WORDING, and no more)
        **{k: v for k, v in xy.items() if k != "X without columns"}, **obs, **lam, **mean, **f32,
        "family": dict(family="probit"), "trials with poisson": dict(y=d.yc, family="poisson", trials=d.n),
        "trials fractional": dict(trials=np.where(at2, 1.5, ones)), "trials zero": dict(trials=np.where(at2, 0.0, ones)),
        "trials nan": dict(trials=np.where(at2, nan, ones)), "y not 0/1": dict(y=np.where(at2, 2.0, d.yb)),
        "y above trials": dict(y=d.n + 1.0, trials=d.n), "y fractional of trials": dict(y=np.where(at2, 0.5, 0.0), trials=d.n),
        "poisson y negative": dict(y=-d.yc - 1.0, family="poisson"), "poisson y fractional": dict(y=d.yc + 0.5, family="poisson"),
        "D > 128": dict(X=np.ones((M, 129))),
        "y short + family": dict(y=d.yb[:-1], family="probit"),
        "family + X nan": dict(family="probit", X=np.full((M, D), nan)), "X nan + weights negative": dict(X=np.full((M, D), nan), weights=-ones),
        "weights negative + y not 0/1": dict(weights=-ones, y=d.yc + 2.0), "y not 0/1 + precision negative": dict(y=d.yc + 2.0, prior_precision=-1.0),
        "precision negative + mean short": dict(prior_precision=-1.0, prior_mean=np.zeros(1)),
        "mean short + D > 128": dict(X=np.ones((M, 129)), prior_mean=np.zeros(1)),
        "D > 128 + float32": dict(X=np.ones((M, 129)), dtype="float32")})
    # ---- SoftmaxGLM
    y3 = np.arange(M) % 3.0
    over(glm.SoftmaxGLM, dict(X=X, y=y3), {
        **xy, **lam, **f32, "labels negative": dict(y=-y3), "labels fractional": dict(y=y3 + 0.5), "classes fractional": dict(classes=2.5),
        "classes 1": dict(y=np.zeros(M), classes=1), "classes None of one class": dict(y=np.zeros(M)), "label >= classes": dict(classes=2),
        "classes 9": dict(classes=9), "D = 17 with 8 classes": dict(X=np.ones((M, 17)), classes=8),
        "X nan + labels negative": dict(X=np.full((M, D), nan), y=-y3), "label >= classes + precision negative": dict(classes=2, prior_precision=-1.0),
        "precision negative + classes 9": dict(prior_precision=-1.0, classes=9), "classes 9 + float32": dict(classes=9, dtype="float32")})
    rows["SoftmaxGLM: pointwise"] = lambda: object.__new__(glm.SoftmaxGLM).pointwise(np.zeros((9, 2)))
    # ---- DispersionGLM
    disp = {"dispersion word": dict(dispersion="fit"), "dispersion None": dict(dispersion=None), "dispersion zero": dict(dispersion=0.0),
            "dispersion inf": dict(dispersion=inf), "dispersion prior one number": dict(log_dispersion_prior=(0.0,)),
            "dispersion prior scalar": dict(log_dispersion_prior=0.25), "dispersion prior nan": dict(log_dispersion_prior=(nan, 0.25)),
            "dispersion prior negative": dict(log_dispersion_prior=(0.0, -0.1)),
            "dispersion held with a prior": dict(dispersion=2.0, log_dispersion_prior=(0.0, 0.25)),
            "dispersion word + its prior": dict(dispersion="fit", log_dispersion_prior=(nan, 0.25))}
    over(glm.DispersionGLM, dict(X=X, y=d.yc), {
        **xy, **obs, **lam, **mean, **f32, **disp, "family": dict(family="poisson"),
        "negbinomial y negative": dict(y=-d.yc - 1.0), "negbinomial y fractional": dict(y=d.yc + 0.25),
        "gamma y zero": dict(family="gamma", y=np.where(at2, 0.0, d.yp)),
        "negbinomial state 65": dict(X=np.ones((M, 64))), "negbinomial held state 65": dict(X=np.ones((M, 65)), dispersion=1.0),
        "gaussian state 129": dict(X=np.ones((M, 128)), y=d.yr, family="gaussian"),
        "gamma state 129": dict(X=np.ones((M, 128)), y=d.yp, family="gamma"),
        "family + X 1-D": dict(family="poisson", X=X[:, 0]), "X nan + y fractional": dict(X=np.full((M, D), nan), y=d.yc + 0.25),
        "y fractional + weights negative": dict(y=d.yc + 0.25, weights=-ones), "offset inf + dispersion word": dict(offset=np.full(M, inf), dispersion="fit"),
        "dispersion zero + precision negative": dict(dispersion=0.0, prior_precision=-1.0),
        "mean short + state 65": dict(X=np.ones((M, 64)), prior_mean=np.zeros(1)), "state 65 + float32": dict(X=np.ones((M, 64)), dtype="float32")})
    # ---- OrdinalGLM
    y4 = np.arange(M) % 4.0
    over(glm.OrdinalGLM, dict(X=X, y=y4), {
        **xy, **obs, **lam, **mean, **f32, "categories 1": dict(categories=1), "categories 9": dict(categories=9),
        "y = 8": dict(y=np.where(at2, 8.0, y4)), "category >= categories": dict(categories=3), "y negative": dict(y=-y4),
        "y fractional": dict(y=y4 + 0.5), "cutpoint precision negative": dict(cutpoint_prior=((0.0, -1.0), (0.0, 1.0))),
        "cutpoint mean nan": dict(cutpoint_prior=((0.0, 1.0), (nan, 1.0))), "cutpoint K rows": dict(cutpoint_prior=np.ones((4, 2))),
        "cutpoint one pair": dict(cutpoint_prior=(0.0, 1.0)), "state 65": dict(X=np.ones((M, 62))),
        "X nan + categories 9": dict(X=np.full((M, D), nan), categories=9), "y fractional + weights negative": dict(y=y4 + 0.5, weights=-ones),
        "offset inf + precision negative": dict(offset=np.full(M, inf), prior_precision=-1.0),
        "mean short + cutpoint one pair": dict(prior_mean=np.zeros(1), cutpoint_prior=(0.0, 1.0)),
        "cutpoint one pair + state 65": dict(cutpoint_prior=(0.0, 1.0), X=np.ones((M, 62))), "state 65 + float32": dict(X=np.ones((M, 62)), dtype="float32")})
    og = object.__new__(glm.OrdinalGLM)
    og.numCoefficients, og.categories, og.numDimensions = D, 4, D + 3
    each("OrdinalGLM.unconstrain", og.unconstrain, {
        "w short": (np.zeros(D - 1), np.arange(3.0)), "cutpoints short": (np.zeros(D), np.arange(2.0)),
        "trailing shapes": (np.zeros((D, 2)), np.zeros((3, 3))), "not increasing": (np.zeros(D), np.array([0.0, 2.0, 1.0])),
        "cutpoint inf": (np.zeros(D), np.array([0.0, 1.0, inf]))})
    # ---- the hierarchical priors, shared by HierarchicalGLM and HierarchicalDispersionGLM
    Q2 = np.array([[1.0, -1.0], [-1.0, 1.0]])
    prior = {"parametrisation word": dict(parametrisation="non-centered"), "parametrisation None": dict(parametrisation=None),
             "groups None": dict(groups=None), "groups short": dict(groups=d.g[:2]), "groups fractional": dict(groups=np.array([-1, 0.5, 0])),
             "groups nan": dict(groups=np.array([-1, nan, 0])), "groups -2": dict(groups=np.array([-2, 0, 0])),
             "groups all -1": dict(groups=np.full(D, -1)), "groups 5": dict(X=np.ones((M, 6)), groups=np.array([-1, 0, 1, 2, 3, 4])),
             "groups unused index": dict(groups=np.array([-1, 0, 2])), "scale prior negative": dict(log_scale_prior=(0.0, -0.1)),
             "scale prior word": dict(log_scale_prior="wide"), "scale prior 3 pairs": dict(log_scale_prior=np.zeros((3, 2))),
             "scale prior nan": dict(log_scale_prior=(nan, 1.0)), "scale prior None": dict(log_scale_prior=None),
             "precision negative": dict(prior_precision=-1.0), "precision short": dict(prior_precision=np.ones(D + 1)),
             "precision 2-D": dict(prior_precision=np.ones((D, 1))), "precision of a fixed row nan": dict(prior_precision=np.array([nan, 1.0, 1.0])),
             "precision of a grouped row nan": dict(prior_precision=np.array([1.0, nan, -1.0])),
             "groups short + scale prior negative": dict(groups=d.g[:2], log_scale_prior=(0.0, -0.1)),
             "scale prior negative + precision negative": dict(log_scale_prior=(0.0, -0.1), prior_precision=-1.0),
             "precision negative + mean short": dict(prior_precision=-1.0, prior_mean=np.zeros(1))}
    xyh = {k: v for k, v in xy.items() if k not in ("X 1-D", "X without rows", "X without columns")}
    over(H, dict(X=X, y=d.yb, groups=d.g), {
        **xyh, **obs, **mean, **f32, **prior, "family": dict(family="gaussian"),
        "trials with poisson": dict(y=d.yc, family="poisson", trials=d.n), "y not 0/1": dict(y=d.yc + 2.0),
        "state 65": dict(X=np.ones((M, 64)), groups=np.r_[-np.ones(62, int), 0, 0]),
        "noncentred state 65": dict(X=np.ones((M, 64)), groups=np.r_[-np.ones(62, int), 0, 0], parametrisation="noncentred"),
        "penalty state 65": dict(X=np.ones((M, 64)), groups=np.r_[-np.ones(62, int), 0, 0], penalty=[Q2]),
        "penalty noncentred": dict(penalty=[Q2], parametrisation="noncentred"),
        "rank without penalty": dict(penalty_rank=[1]), "rank with None penalties": dict(penalty=[None], penalty_rank=[1]),
        "penalty of an unused group": dict(penalty={1: Q2}), "penalty no sequence": dict(penalty=3.0),
        "penalty two entries": dict(penalty=[Q2, Q2]), "rank of an unused group": dict(penalty=[Q2], penalty_rank={"a": 1}),
        "rank no sequence": dict(penalty=[Q2], penalty_rank=1), "rank two entries": dict(penalty=[Q2], penalty_rank=[1, 1]),
        "rank of an exchangeable group": dict(groups=d.g2, penalty={1: Q2}, penalty_rank={0: 1}),
        "penalty of words": dict(penalty=[[["a", "b"], ["c", "d"]]]), "penalty 3 x 3": dict(penalty=[np.eye(3)]),
        "penalty nan": dict(penalty=[np.full((2, 2), nan)]), "penalty zero": dict(penalty=[np.zeros((2, 2))]),
        "penalty asymmetric": dict(penalty=[np.array([[1.0, 0.5], [0.0, 1.0]])]),
        "penalty indefinite": dict(penalty=[np.array([[1.0, 2.0], [2.0, 1.0]])]), "rank 3 of 2": dict(penalty=[Q2], penalty_rank=[3]),
        "rank fractional": dict(penalty=[Q2], penalty_rank=[1.5]), "rank True": dict(penalty=[Q2], penalty_rank=[True]),
        "parametrisation word + groups None": dict(parametrisation="x", groups=None), "groups None + y short": dict(groups=None, y=d.yb[:-1]),
        "y short + groups short": dict(y=d.yb[:-1], groups=d.g[:2]), "float32 + groups short": dict(dtype="float32", groups=d.g[:2]),
        "mean short + penalty nan": dict(prior_mean=np.zeros(1), penalty=[np.full((2, 2), nan)]),
        "penalty noncentred + state 65": dict(X=np.ones((M, 64)), groups=np.r_[-np.ones(62, int), 0, 0], penalty=[Q2], parametrisation="noncentred")})
    each("HierarchicalGLM.with_random_intercepts", H.with_random_intercepts, {
        "rank without penalty": (X, d.yb, d.labels, dict(penalty_rank=1, device=0)),
        "labels short": (X, d.yb, d.labels[:-1], dict(device=0)), "X 1-D": (X[:, 0], d.yb, d.labels, dict(device=0)),
        "groups short": (X, d.yb, d.labels, dict(groups=d.g[:2], device=0)),
        "precision short": (X, d.yb, d.labels, dict(prior_precision=np.ones(D + 1), device=0))})
    each("HierarchicalGLM.random_walk_penalty", H.random_walk_penalty, {
        "n fractional": (4.0,), "n True": (True,), "order 3": (5, 3), "order True": (5, True), "n = order": (2, 2)})
    each("HierarchicalGLM.icar_penalty", H.icar_penalty, {
        "not square": (np.ones((2, 3)),), "one node": (np.zeros((1, 1)),), "entries": (np.array([[0.0, 2.0], [2.0, 0.0]]),),
        "asymmetric": (np.array([[0.0, 1.0], [0.0, 0.0]]),), "self-loop": (np.array([[1.0, 1.0], [1.0, 0.0]]),),
        "isolated node": (np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]]),)})
    # ---- HierarchicalDispersionGLM
    over(HD, dict(X=X, y=d.yr, groups=d.g), {
        **xy, **obs, **mean, **f32, **prior, **disp, "family of HierarchicalGLM": dict(family="logistic", y=d.yb),
        "family gamma": dict(family="gamma", y=d.yp), "family": dict(family="student"), "penalty": dict(penalty={0: np.eye(2)}),
        "penalty_rank": dict(penalty_rank={0: 1}), "negbinomial y fractional": dict(family="negbinomial", y=d.yc + 0.25),
        "state 65": dict(X=np.ones((M, 63)), groups=np.r_[-np.ones(62, int), 0]),
        "held state 65": dict(X=np.ones((M, 64)), groups=np.r_[-np.ones(63, int), 0], dispersion=1.0, family="negbinomial", y=d.yc,
                              parametrisation="noncentred"),
        "family of HierarchicalGLM + penalty": dict(family="poisson", penalty={0: np.eye(2)}), "penalty + parametrisation word": dict(penalty=[Q2], parametrisation="x"),
        "parametrisation word + groups None": dict(parametrisation="x", groups=None), "groups None + family gamma": dict(groups=None, family="gamma"),
        "family gamma + X 1-D": dict(family="gamma", X=X[:, 0]), "family + X 1-D": dict(family="student", X=X[:, 0]),
        "X 1-D + groups short": dict(X=X[:, 0], groups=d.g[:2]), "weights negative + dispersion word": dict(weights=-ones, dispersion="fit"),
        "dispersion word + groups short": dict(dispersion="fit", groups=d.g[:2]), "mean short + state 65": dict(X=np.ones((M, 63)), groups=np.r_[-np.ones(62, int), 0], prior_mean=np.zeros(1)),
        "state 65 + float32": dict(X=np.ones((M, 63)), groups=np.r_[-np.ones(62, int), 0], dtype="float32")})
    # ---- the packers and the layout
    each("padded_dim", glm.padded_dim, {"0": (0,), "129": (129,)})
    each("pack_metric", glm.pack_metric, {"2-D": (np.ones((2, 2)),), "empty": (np.ones(0),), "negative": (np.array([1.0, -1.0]),),
                                          "nan": (np.array([nan, 1.0]),), "129": (np.ones(129),)})
    each("pack_design", glm.pack_design, {"1-D": (np.ones(3),), "no rows": (np.ones((0, 3)),), "no columns": (np.ones((3, 0)),),
                                          "129 columns": (np.ones((2, 129)),), "nan": (np.full((2, 2), nan),)})
    each("pack_observations", glm.pack_observations, {
        "family": (d.yb, "probit"), "y 2-D": (np.zeros((M, 1)),), "y empty": (np.zeros(0),), "weights short": (d.yb, dict(weights=ones[:-1])),
        "trials nan": (d.yb, dict(trials=np.where(at2, nan, ones))), "y = 2": (np.where(at2, 2.0, d.yb),),
        "weights negative": (d.yb, dict(weights=-ones)), "poisson y fractional": (d.yc + 0.5, "poisson"),
        "trials with poisson": (d.yc, "poisson", dict(trials=d.n)), "trials zero": (d.yb, dict(trials=np.zeros(M))),
        "family + y empty": (np.zeros(0), "probit"), "y empty + weights short": (np.zeros(0), dict(weights=ones))})
    each("pack_observations_dispersion", glm.pack_observations_dispersion, {
        "family": (d.yc, "poisson"), "y 2-D": (np.zeros((M, 1)),), "offset short": (d.yc, dict(offset=ones[:-1])),
        "y fractional": (d.yc + 0.25,), "gamma y zero": (np.zeros(M), "gamma"), "weights negative": (d.yc, dict(weights=-ones)),
        "gaussian y nan": (np.where(at2, nan, d.yr), "gaussian")})
    each("pack_observations_ordinal", glm.pack_observations_ordinal, {
        "y 2-D": (np.zeros((M, 1)), 4), "y empty": (np.zeros(0), 4), "weights 2-D": (y4, 4, dict(weights=np.ones((M, 1)))),
        "y = K": (y4, 3), "K = 1": (np.zeros(M), 1), "K = 9": (y4, 9), "offset inf": (y4, 4, dict(offset=np.where(at2, inf, 0.0))),
        "K words": (y4, "four")})
    each("pack_prior_groups", glm.pack_prior_groups, {
        "groups all -1": (np.full(D, -1),), "scale prior negative": (d.g, (0.0, -0.1)), "precision negative": (d.g, (0.0, 1.0), -1.0),
        "mean short": (d.g, dict(prior_mean=np.zeros(1))), "129 rows": (np.r_[-np.ones(128, int), 0],)})
    each("pack_prior_groups_dispersion", glm.pack_prior_groups_dispersion, {
        "groups 2-D": (np.zeros((D, 1), int),), "dispersion word": (d.g, dict(dispersion="fit")),
        "dispersion prior negative": (d.g, dict(log_dispersion_prior=(0.0, -1.0))), "128 rows sampled": (np.r_[-np.ones(126, int), 0],),
        "groups -2 + dispersion word": (np.array([-2, 0, 0]), dict(dispersion="fit"))})
    each("pack_penalty", glm.pack_penalty, {"not square": (np.ones((2, 3)), 1), "1-D": (np.ones(3), 1), "J = 0": (np.eye(3), 0),
                                            "J = 5": (np.eye(3), 5), "128 rows": (np.eye(128), 1), "nan": (np.full((3, 3), nan), 1),
                                            "not square + J = 0": (np.ones((2, 3)), 0)})
    each("softmax_layout", glm.softmax_layout, {"K = 9": (3, 9), "K = 1": (3, 1), "D = 0": (0, 3), "D = 65": (65, 2), "D = 17, K = 8": (17, 8)})
    each("pointwise_constants", glm.pointwise_constants, {"family": ("softmax", d.yb)})
    # ---- methods of potentials that were built (no handle: whatever passes these checks goes on to the device)
    with recorded_creates([]):
        plain = glm.GLM(X, d.yb, device=0)
        flat = glm.GLM(X, d.yb, prior_precision=np.array([1.0, 0.0, 1.0]), device=0)
        hier = H(X, d.yb, groups=d.g, log_scale_prior=(0.0, 0.0), device=0)
        pen = H(X, d.yb, groups=d.g2, penalty={1: Q2}, device=0)
        hd = HD(X, d.yr, groups=d.g, log_dispersion_prior=(0.0, 0.0), parametrisation="noncentred", device=0)
        ordinal = glm.OrdinalGLM(X, y4, cutpoint_prior=((0.0, 1.0), (0.0, 0.0)), device=0)
        dg = glm.DispersionGLM(X, d.yc, prior_precision=0.0, device=0)
    each("set_likelihood_power", plain.set_likelihood_power, {"zero": (0.0,), "nan": (nan,), "inf": (inf,), "negative": (-1.0,)})
    each("sample_prior", lambda pot, N: pot.sample_prior(N), {
        "N = 0": (plain, 0), "penalty": (pen, 4), "N = 0 + penalty": (pen, 0), "flat coefficient": (flat, 4), "flat group scale": (hier, 4),
        "flat dispersion": (hd, 4), "flat log-gap": (ordinal, 4), "flat coefficients": (dg, 4)})
    import torch
    each("pointwise", lambda pot, s: pot.pointwise(s), {
        "1-D": (plain, np.zeros(3)), "rows": (hd, np.zeros((4, 2))), "4-D": (ordinal, np.zeros((6, 2, 2, 2))),
        "float32 tensor": (plain, torch.zeros((3, 2, 2), dtype=torch.float32)), "4-D tensor": (plain, torch.zeros((3, 2, 2, 2), dtype=torch.float64)),
        "host tensor": (plain, torch.zeros((3, 2), dtype=torch.float64))})
    each("loglik", lambda pot, s: pot.loglik(s), {"1-D": (plain, np.zeros(3)), "4-D": (hier, np.zeros((4, 2, 2, 2)))})
    return rows


def census(glm):
    out = {"routes": {}, "rejections": {}}
    for name, make in routes(glm).items():
        calls = []
        with recorded_creates(calls):
            pot = make()
        state = {k: _enc(v) for k, v in sorted(vars(pot).items()) if k != "_handle"}
        layout = _enc(glm._prior_layout(pot)) if isinstance(pot, glm._Tempered) else None
        out["routes"][name] = {"calls": calls, "vars": state, "prior_layout": layout}
    for name, row in rejections(glm).items():
        try:
            with recorded_creates([]):
                row()
        except Exception as e:  # noqa: BLE001 -- the type is what is recorded
            out["rejections"][name] = {"type": type(e).__name__, "message": str(e)}
        else:
            out["rejections"][name] = {"type": None, "message": None}
    return json.loads(json.dumps(out))


def test_glm_frontend_census():
    from physicsbasedbayesianinference_amd import glm
    with open(FIXTURE) as f:
        want = json.load(f)
    for row, (old, new) in WORDING.items():
        assert want["rejections"][row] == {"type": "ValueError", "message": old}
        want["rejections"][row]["message"] = new
    got = census(glm)
    for part in ("routes", "rejections"):
        assert sorted(got[part]) == sorted(want[part])
        for name in want[part]:
            assert got[part][name] == want[part][name], (part, name)
    assert len(want["rejections"]) >= 400 and sum(r["type"] is None for r in want["rejections"].values()) <= 4


def _load(path):
    """glm.py at `path` as a module of the package (its relative imports resolve to the package as it is)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("physicsbasedbayesianinference_amd._glm_census", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True, help="the JSON file to write")
    ap.add_argument("--glm", required=True, help="the glm.py to take the census of")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    path, seen = os.path.abspath(a.glm), set()
    glm = _load(path)

    def tracer(frame, event, arg):
        if frame.f_code.co_filename != path:
            return None
        if event == "line":
            seen.add(frame.f_lineno)
        return tracer

    sys.settrace(tracer)
    result = census(glm)
    sys.settrace(None)
    with open(a.record, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    import ast
    source = open(path).read()
    for no in sorted({n.lineno for n in ast.walk(ast.parse(source)) if isinstance(n, ast.Raise)} - seen):
        print("not reached: %s:%d: %s" % (os.path.basename(path), no, source.splitlines()[no - 1].strip()))
    print("%d routes, %d rejection rows" % (len(result["routes"]), len(result["rejections"])))
