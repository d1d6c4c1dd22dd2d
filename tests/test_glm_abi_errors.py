"""A census of what the C ABI's GLM entries reject (CPU only: every argument check runs before a device is asked for).

glm.py checks everything before it calls the library, so nothing else holds the library's OWN rejections: the seven
pbbi_potential_create_glm* entries and the seven host-side pbbi_glm_pack_* / _layout entries are called here directly
through _lib.load().  For every entry, SEQUENCES lists its rejection statements in the order the entry makes them, each with
one call that breaks that rule alone; the return code and the exact pbbi_last_error() text are literals recorded from the
library as it stood before the host-side refactor (PBBI_LIB selects the build under test).  Three things are asserted:

  * every statement, alone: its code and text;
  * every adjacent pair of the sequence, both broken in one call: the EARLIER one is reported (the order is part of the ABI
    -- a caller that fixes what it is told meets the faults in this order);
  * one fully valid call per entry.  A create entry then asks for the device: PBBI_OK with a handle (destroyed here) where
    there is a GPU, PBBI_ERR_HIP from hipGetDeviceCount where there is none -- either shows that every check passed.

Not reachable through these entries, hence absent: `y is NULL` of glm_check_obs / _disp behind the create entries' own
`X / y is NULL`; `D must be >= 1` of new_handle behind any entry with a check of D; `unknown dtype` behind any `float64
only`; the family rule of the hierarchical dimension check behind glm_check_obs; new_handle's device range (it needs the
device count)."""
import ctypes as C

import numpy as np
import pytest

from physicsbasedbayesianinference_amd import _lib

INVALID, UNSUPPORTED, HIP = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED, _lib.ERR_HIP
NAN, INF = float("nan"), float("inf")


def A(*v):
    return np.array(v, dtype=np.float64)


# ---- how each entry is called: (argument, kind) in the C order.  i int, l int64, d double, D doubles or NULL, G int32s or
# NULL, H the handle's out pointer (True) or NULL (None), B an out buffer of that many doubles or NULL (None), L / I / R
# optional int64 / int / int32 out pointers (always NULL here except L).
_HIER_HEAD = [("D", "i"), ("M", "l"), ("X", "D"), ("y", "D"), ("family", "i"), ("weights", "D"), ("offset", "D")]
_HIER_TAIL = [("prior_precision", "D"), ("prior_mean", "D"), ("groups", "G"), ("J", "i"), ("log_scale_prior", "D")]
_END = [("dtype", "i"), ("device", "i"), ("out", "H")]
SPECS = {
    "potential_create_glm": _HIER_HEAD[:5] + [("prior_precision", "d")] + _END,
    "potential_create_glm_ex": _HIER_HEAD + [("trials", "D"), ("prior_precision", "D"), ("prior_mean", "D")] + _END,
    "potential_create_glm_softmax": [("D", "i"), ("K", "i"), ("M", "l"), ("X", "D"), ("y", "D"), ("prior_precision", "D")] + _END,
    "potential_create_glm_dispersion": _HIER_HEAD + [("prior_precision", "D"), ("prior_mean", "D"), ("sample", "i"),
                                                     ("theta", "d")] + _END,
    "potential_create_glm_hier": _HIER_HEAD + [("trials", "D")] + _HIER_TAIL + _END,
    "potential_create_glm_hier_ex": _HIER_HEAD + [("trials", "D")] + _HIER_TAIL + [("parametrisation", "i")] + _END,
    "potential_create_glm_hier_q": _HIER_HEAD + [("trials", "D")] + _HIER_TAIL + [("penalty", "D"), ("rank", "D")] + _END,
    "potential_create_glm_hier_dispersion": _HIER_HEAD + _HIER_TAIL + [("parametrisation", "i"), ("sample", "i"), ("theta", "d"),
                                                                       ("log_dispersion_prior", "D")] + _END,
    "glm_pack_design": [("D", "i"), ("M", "l"), ("X", "D"), ("out", "B"), ("out_len", "l"), ("len_out", "L")],
    "glm_pack_observations": [("M", "l"), ("family", "i"), ("y", "D"), ("weights", "D"), ("offset", "D"), ("trials", "D"),
                              ("out", "B"), ("out_len", "l"), ("len_out", "L")],
    "glm_pack_observations_dispersion": [("M", "l"), ("family", "i"), ("y", "D"), ("weights", "D"), ("offset", "D"),
                                         ("out", "B"), ("out_len", "l"), ("len_out", "L")],
    "glm_softmax_layout": [("D", "i"), ("K", "i"), ("Dc_out", "I"), ("NT_out", "I"), ("row_map", "R")],
    "glm_pack_prior_groups": [("D", "i"), ("J", "i")] + _HIER_TAIL[:3] + [("log_scale_prior", "D"), ("out", "B"), ("n_out", "B")],
    "glm_pack_prior_groups_dispersion": [("D", "i"), ("J", "i")] + _HIER_TAIL[:3] + [
        ("log_scale_prior", "D"), ("sample", "i"), ("log_dispersion_prior", "D"), ("out", "B"), ("n_out", "B")],
    "glm_pack_penalty": [("D", "i"), ("J", "i"), ("penalty", "D"), ("out", "B"), ("out_len", "l"), ("len_out", "L")],
}


def call(entry, kw):
    """-> (return code, pbbi_last_error()); a handle that was made is destroyed."""
    lib = _lib.load()
    args, keep, handle = [], [], None
    for name, kind in SPECS[entry]:
        v = kw.get(name)
        if kind in "il":
            args.append(int(v))
        elif kind == "d":
            args.append(float(v))
        elif kind in "DGB":
            if v is None:
                args.append(None)
                continue
            a = (np.zeros(int(v)) if kind == "B" else
                 np.ascontiguousarray(v, dtype=np.int32 if kind == "G" else np.float64))
            keep.append(a)
            args.append(a.ctypes.data_as(C.POINTER(C.c_int32) if kind == "G" else _lib._dp))
        elif kind == "H":
            handle = C.c_void_p() if v else None
            args.append(C.byref(handle) if v else None)
        elif kind == "L":
            keep.append(C.c_int64())
            args.append(C.byref(keep[-1]))
        else:
            args.append(None)
    rc = getattr(lib, "pbbi_" + entry)(*args)
    msg = lib.pbbi_last_error().decode()
    if handle is not None and handle.value:
        assert rc == _lib.OK
        assert lib.pbbi_potential_destroy(handle) == _lib.OK
    return rc, msg


# ---- one valid call per entry: 3 observations, 2 or 3 coefficients
X2 = np.array([[0.5, -1.0], [1.5, 0.25], [-0.75, 2.0]])
X3 = np.array([[0.5, -1.0, 1.0], [1.5, 0.25, 1.0], [-0.75, 2.0, 1.0]])
RW1 = np.array([[1.0, -1.0, 0.0], [-1.0, 1.0, 0.0], [0.0, 0.0, 0.0]])     # coefficients 0, 1 in group 0, coefficient 2 fixed
_DEV = dict(dtype=_lib.F64, device=0, out=True)
_HIER = dict(D=3, M=3, X=X3, y=A(0, 1, 1), family=_lib.GLM_LOGISTIC, weights=None, offset=None, trials=None,
             prior_precision=A(1, 1, 1), prior_mean=None, groups=[0, 0, -1], J=1, log_scale_prior=A(0, 1), **_DEV)
VALID = {
    "potential_create_glm": dict(D=2, M=3, X=X2, y=A(0, 1, 1), family=_lib.GLM_LOGISTIC, prior_precision=1.0, **_DEV),
    "potential_create_glm_ex": dict(D=2, M=3, X=X2, y=A(0, 1, 1), family=_lib.GLM_LOGISTIC, weights=None, offset=None,
                                    trials=None, prior_precision=A(1, 1), prior_mean=None, **_DEV),
    "potential_create_glm_softmax": dict(D=2, K=3, M=3, X=X2, y=A(0, 1, 2), prior_precision=A(1, 1), **_DEV),
    "potential_create_glm_dispersion": dict(D=2, M=3, X=X2, y=A(0.5, 1, 2), family=_lib.GLM_GAUSSIAN, weights=None,
                                            offset=None, prior_precision=A(1, 1, 1), prior_mean=None, sample=1, theta=0.0, **_DEV),
    "potential_create_glm_hier": _HIER,
    "potential_create_glm_hier_ex": dict(_HIER, parametrisation=_lib.HIER_NONCENTRED),
    "potential_create_glm_hier_q": dict(_HIER, penalty=RW1, rank=A(1)),
    "potential_create_glm_hier_dispersion": dict(
        {k: v for k, v in _HIER.items() if k != "trials"}, y=A(0.5, 1, 2), family=_lib.GLM_GAUSSIAN,
        parametrisation=_lib.HIER_CENTRED, sample=1, theta=0.0, log_dispersion_prior=A(0, 1)),
    "glm_pack_design": dict(D=2, M=3, X=X2, out=4 * 16 * 32, out_len=4 * 16 * 32),
    "glm_pack_observations": dict(M=3, family=_lib.GLM_LOGISTIC, y=A(0, 1, 1), weights=None, offset=None, trials=None,
                                  out=192, out_len=192),
    "glm_pack_observations_dispersion": dict(M=3, family=_lib.GLM_GAUSSIAN, y=A(0.5, 1, 2), weights=None, offset=None,
                                             out=192, out_len=192),
    "glm_softmax_layout": dict(D=2, K=3),
    "glm_pack_prior_groups": dict(D=3, J=1, prior_precision=A(1, 1, 1), prior_mean=None, groups=[0, 0, -1],
                                  log_scale_prior=A(0, 1), out=32, n_out=1),
    "glm_pack_prior_groups_dispersion": dict(D=3, J=1, prior_precision=A(1, 1, 1), prior_mean=None, groups=[0, 0, -1],
                                             log_scale_prior=A(0, 1), sample=1, log_dispersion_prior=A(0, 1), out=32, n_out=1),
    "glm_pack_penalty": dict(D=3, J=1, penalty=RW1, out=256, out_len=256),
}

# ---- the rejection statements.  A step is (what is wrong, the arguments that make it wrong, code, text[, options]):
#   alt=True        a second condition of a statement already in the sequence: checked alone, no part of the pairs
#   pair=dict(...)  the arguments that break this rule AND the previous one of the sequence, where the two single calls
#                   cannot simply be merged (both faults sit in the same argument); pair_text: what the earlier rule then says
#   pair=False      this rule and the previous one cannot both be broken in one call (why: in the step's name)
GLM_RULE = "GLM potentials run on the fp64 matrix-core kernels: float64 and D <= 128 only"
XY_NULL = ("X is NULL", dict(X=None), INVALID, "X / y is NULL")
XY_NULL_Y = ("y is NULL", dict(y=None), INVALID, "X / y is NULL", dict(alt=True))
OUT_NULL = ("out is NULL", dict(out=None), INVALID, "out pointer is NULL")
HIER64 = dict(D=64, X=np.ones((3, 64)), prior_precision=np.ones(64), groups=[0] * 64)

# glm_check_obs, as far as an entry that has checked y reaches it
OBS = [
    ("M < 1", dict(M=0), INVALID, "M must be >= 1"),
    ("family", dict(family=_lib.GLM_GAUSSIAN), INVALID, "unknown GLM family"),
    ("trials for poisson", dict(family=_lib.GLM_POISSON, trials=A(1, 1, 1)), INVALID,
     "trials belong to the logistic (binomial) family only", dict(pair=dict(family=_lib.GLM_GAUSSIAN, trials=A(1, 1, 1)))),
    ("trials value", dict(trials=A(0.5, 1, 1)), INVALID, "trials must be integers >= 1 (observation 0)",
     dict(pair=dict(family=_lib.GLM_POISSON, trials=A(0.5, 1, 1)))),
    ("y value", dict(y=A(-1, 1, 1)), INVALID, "y must hold non-negative integers (observation 0)"),
    ("y above the trials", dict(y=A(2, 1, 1)), INVALID, "logistic: y must not exceed the trials (observation 0)",
     dict(pair=dict(y=A(1.5, 1, 1)))),
    ("weights", dict(weights=A(-1, 1, 1)), INVALID, "weights must be finite and >= 0 (observation 0)"),
    ("offset", dict(offset=A(NAN, 0, 0)), INVALID, "offset must be finite (observation 0)"),
]
# glm_check_obs_disp
OBS_DISP = [
    ("M < 1", dict(M=0), INVALID, "M must be >= 1"),
    ("family", dict(family=7), INVALID, "unknown dispersion family (gaussian = 3, negbinomial = 4)"),
    ("y finite", dict(y=A(NAN, 1, 2)), INVALID, "y must be finite (observation 0)"),
    ("negbinomial y", dict(family=_lib.GLM_NEGBINOMIAL, y=A(0.5, 1, 2)), INVALID,
     "negbinomial: y must hold non-negative integers (observation 0)", dict(pair=dict(family=_lib.GLM_NEGBINOMIAL, y=A(NAN, 1, 2)))),
    ("weights", dict(weights=A(-1, 1, 1)), INVALID, "weights must be finite and >= 0 (observation 0)"),
    ("offset", dict(offset=A(NAN, 0, 0)), INVALID, "offset must be finite (observation 0)"),
]
PRIOR = [
    ("prior_precision NULL", dict(prior_precision=None), INVALID, "prior_precision is NULL"),
    ("prior_precision value (no call has it NULL and wrong)", dict(prior_precision=A(-1, 1, 1)), INVALID,
     "prior_precision must be finite and >= 0 (coefficient 0)", dict(pair=False)),
    ("prior_mean", dict(prior_mean=A(INF, 0, 0)), INVALID, "prior_mean must be finite (coefficient 0)"),
]
# glm_check_hier on the valid call's groups [0, 0, -1]
HIER = [
    ("D < 1", dict(D=0), INVALID, "D must be >= 1"),
    ("J", dict(J=5), UNSUPPORTED, "hierarchical prior: the number of groups J must be 1 .. 4 (J = 5)"),
    ("J low", dict(J=0), UNSUPPORTED, "hierarchical prior: the number of groups J must be 1 .. 4 (J = 0)", dict(alt=True)),
    ("groups NULL", dict(groups=None), INVALID, "groups is NULL"),
    ("prior_precision NULL", dict(prior_precision=None), INVALID, "prior_precision is NULL"),
    ("log_scale_prior NULL", dict(log_scale_prior=None), INVALID, "log_scale_prior is NULL"),
    ("group index", dict(groups=[1, 0, -1]), INVALID,
     "groups must hold -1 (fixed prior) or a group index 0 .. J-1 (coefficient 0: 1, J = 1)"),
    ("prior_precision of a fixed row", dict(prior_precision=A(1, 1, -1)), INVALID,
     "prior_precision must be finite and >= 0 (coefficient 2)",
     dict(pair=dict(groups=[0, 0, -2], prior_precision=A(1, 1, -1)),
          pair_text="groups must hold -1 (fixed prior) or a group index 0 .. J-1 (coefficient 2: -2, J = 1)")),
    ("prior_mean", dict(prior_mean=A(0, 0, INF)), INVALID, "prior_mean must be finite (coefficient 2)"),
    ("a group without a coefficient", dict(J=2, log_scale_prior=A(0, 1, 0, 1)), INVALID,
     "every group index 0 .. J-1 must be used (group 1 has no coefficient)"),
    ("log_scale_prior value", dict(log_scale_prior=A(0, -1)), INVALID,
     "log_scale_prior must hold J pairs (finite mean, finite precision >= 0) (group 0)",
     dict(pair=dict(J=2, log_scale_prior=A(0, 1, 0, -1)))),
    ("log_scale_prior mean", dict(log_scale_prior=A(INF, 1)), INVALID,
     "log_scale_prior must hold J pairs (finite mean, finite precision >= 0) (group 0)", dict(alt=True)),
]
# glm_check_hier_disp_theta
THETA = [
    ("log_dispersion_prior NULL", dict(log_dispersion_prior=None), INVALID,
     "log_dispersion_prior is NULL (a sampled dispersion needs its pair (mean, precision))"),
    ("log_dispersion_prior value (no call has it NULL and wrong)", dict(log_dispersion_prior=A(0, -1)), INVALID,
     "log_dispersion_prior must be (finite mean, finite precision >= 0)", dict(pair=False)),
    ("log_dispersion_prior with a held dispersion (no call samples and holds)", dict(sample=0), INVALID,
     "log_dispersion_prior belongs to a sampled dispersion only: a held one has no prior", dict(pair=False)),
]
HELD_NAN = ("held theta", dict(sample=0, log_dispersion_prior=None, theta=NAN), INVALID,
            "a held dispersion must be finite and > 0 (theta = its logarithm)",
            dict(pair=dict(sample=0, theta=NAN)))
PARAM = ("parametrisation", dict(parametrisation=2), INVALID,
         "parametrisation must be PBBI_HIER_CENTRED (0) or PBBI_HIER_NONCENTRED (1)")
X_FINITE = ("X finite", dict(X=np.full((3, 3), NAN)), INVALID, "X must be finite")
HIER_F64 = ("float32", dict(dtype=_lib.F32), UNSUPPORTED, "hierarchical GLM potentials are float64 only")
HIER_F64_ALT = ("unknown dtype", dict(dtype=7), UNSUPPORTED, "hierarchical GLM potentials are float64 only", dict(alt=True))
SMX_RULE = ("softmax GLM: float64, 2 <= K <= 8 classes, each padded to Dc = 16, 32 or 64 rows with K * Dc <= 128 (D <= 16 for "
            "K <= 8, D <= 32 for K <= 4, D <= 64 for K = 2)")
SMX_WIDE = dict(D=17, K=8, X=np.ones((3, 17)), prior_precision=np.ones(17))
Q64 = dict(HIER64, penalty=np.eye(64), rank=A(64))


def penalty_with(Q, a, b, v):
    Q = Q.copy()
    Q[a, b] = v
    return Q


def after(step, **options):
    """The step with the pair options that fit ANOTHER predecessor than the one its list gives it."""
    return step[:4] + ((options,) if options else ())


SEQUENCES = {
    "potential_create_glm": [
        XY_NULL, XY_NULL_Y,
        ("M < 1", dict(M=0), INVALID, "M must be >= 1"),
        ("family", dict(family=_lib.GLM_GAUSSIAN), INVALID, "unknown GLM family"),
        ("prior_precision", dict(prior_precision=-1.0), INVALID, "prior_precision must be >= 0"),
        ("prior_precision NaN", dict(prior_precision=NAN), INVALID, "prior_precision must be >= 0", dict(alt=True)),
        ("float32", dict(dtype=_lib.F32), UNSUPPORTED, GLM_RULE),
        ("D > 128", dict(D=129, X=np.ones((3, 129))), UNSUPPORTED, GLM_RULE, dict(alt=True)),
        OUT_NULL,
        ("D < 1", dict(D=0), INVALID, "D must be >= 1"),
        ("unknown dtype", dict(dtype=7), INVALID, "unknown dtype"),
    ],
    "potential_create_glm_ex": [
        XY_NULL, XY_NULL_Y,
        ("D < 1", dict(D=0), INVALID, "D must be >= 1"),
        *OBS,
        ("float32", dict(dtype=_lib.F32), UNSUPPORTED, GLM_RULE),
        ("D > 128", dict(D=129, X=np.ones((3, 129)), prior_precision=np.ones(129)), UNSUPPORTED, GLM_RULE, dict(alt=True)),
        *PRIOR, OUT_NULL,
        ("unknown dtype", dict(dtype=7), INVALID, "unknown dtype"),
    ],
    "potential_create_glm_softmax": [
        XY_NULL, XY_NULL_Y,
        ("prior_precision NULL", dict(prior_precision=None), INVALID, "prior_precision is NULL"),
        ("M < 1", dict(M=0), INVALID, "M must be >= 1"),
        ("D < 1", dict(D=0), INVALID, "D must be >= 1"),
        ("K < 2", dict(K=1), INVALID, "softmax GLM: at least two classes"),
        ("labels", dict(y=A(3, 1, 2)), INVALID, "labels must be integers in [0, K) (observation 0)"),
        ("X finite", dict(X=np.full((3, 2), NAN)), INVALID, "X must be finite (row 0)"),
        ("prior_precision value", dict(prior_precision=A(-1, 1)), INVALID, "prior_precision must be finite and >= 0 (coefficient 0)"),
        ("float32", dict(dtype=_lib.F32), UNSUPPORTED, "softmax GLM potentials are float64 only"),
        ("K > 8", dict(K=9), UNSUPPORTED, SMX_RULE),
        ("K * Dc > 128", SMX_WIDE, UNSUPPORTED, SMX_RULE, dict(alt=True)),
        OUT_NULL,
    ],
    "potential_create_glm_dispersion": [
        XY_NULL, XY_NULL_Y,
        ("D < 1", dict(D=0), INVALID, "D must be >= 1"),
        *OBS_DISP,
        ("X finite", dict(X=np.full((3, 2), NAN)), INVALID, "X must be finite"),
        ("held theta", dict(sample=0, theta=NAN), INVALID, "a held dispersion must be finite and > 0 (theta = its logarithm)"),
        ("float32", dict(dtype=_lib.F32), UNSUPPORTED,
         "GLM potentials run on the fp64 matrix-core kernels: float64 and a state dimension (coefficients + 1 for a sampled "
         "dispersion) <= 128 only"),
        ("state > 128", dict(D=128, X=np.ones((3, 128)), prior_precision=np.ones(129)), UNSUPPORTED,
         "GLM potentials run on the fp64 matrix-core kernels: float64 and a state dimension (coefficients + 1 for a sampled "
         "dispersion) <= 128 only", dict(alt=True)),
        ("negbinomial state > 64", dict(family=_lib.GLM_NEGBINOMIAL, y=A(0, 1, 2), D=64, X=np.ones((3, 64)), prior_precision=np.ones(65)),
         UNSUPPORTED, "negbinomial: the state dimension (coefficients + 1 for a sampled dispersion) must be <= 64: its kernel "
         "at 65 .. 128 does not fit the register file"),
        after(PRIOR[0], pair=dict(family=_lib.GLM_NEGBINOMIAL, y=A(0, 1, 2), D=64, X=np.ones((3, 64)), prior_precision=None)),
        *PRIOR[1:], OUT_NULL,
        ("unknown dtype", dict(dtype=7), INVALID, "unknown dtype"),
    ],
    "potential_create_glm_hier": [
        XY_NULL, XY_NULL_Y, *HIER, *OBS, X_FINITE, HIER_F64, HIER_F64_ALT,
        ("state > 64", HIER64, UNSUPPORTED,
         "hierarchical prior: the state dimension (coefficients + groups) must be <= 64 for this family (65)"),
        OUT_NULL,
    ],
    "potential_create_glm_hier_ex": [
        PARAM, XY_NULL, XY_NULL_Y, *HIER, *OBS, X_FINITE, HIER_F64, HIER_F64_ALT,
        ("state > 64", HIER64, UNSUPPORTED,
         "hierarchical prior (non-centred): the state dimension (coefficients + groups) must be <= 64 for this family (65)"),
        ("state > 64, centred", dict(HIER64, parametrisation=_lib.HIER_CENTRED), UNSUPPORTED,
         "hierarchical prior: the state dimension (coefficients + groups) must be <= 64 for this family (65)", dict(alt=True)),
        OUT_NULL,
    ],
    "potential_create_glm_hier_q": [
        XY_NULL, XY_NULL_Y, *HIER, *OBS, X_FINITE,
        ("penalty NULL", dict(penalty=None), INVALID, "penalty is NULL"),
        ("penalty_rank NULL", dict(rank=None), INVALID, "penalty_rank is NULL"),
        ("penalty finite", dict(penalty=penalty_with(RW1, 0, 0, NAN)), INVALID, "penalty must be finite (entry 0, 0)"),
        ("penalty on a fixed row", dict(penalty=penalty_with(RW1, 0, 2, 1.0)), INVALID,
         "penalty must be zero on fixed rows and between different groups (entry 0, 2)",
         dict(pair=dict(penalty=penalty_with(RW1, 0, 2, NAN)), pair_text="penalty must be finite (entry 0, 2)")),
        ("zero penalty", dict(penalty=np.zeros((3, 3))), INVALID, "penalty must not be the zero matrix (group 0)",
         dict(pair=dict(penalty=penalty_with(np.zeros((3, 3)), 0, 2, 1.0)))),
        ("asymmetric penalty (a zero block is symmetric)", dict(penalty=np.array([[1, -1, 0], [-0.5, 1, 0], [0, 0, 0.0]])), INVALID,
         "penalty must be symmetric (group 0)", dict(pair=False)),
        ("indefinite penalty", dict(penalty=np.array([[1, -2, 0], [-2, 1, 0], [0, 0, 0.0]])), INVALID,
         "penalty must be positive semi-definite (group 0)", dict(pair=dict(penalty=np.array([[1, -3, 0], [-1, 1, 0], [0, 0, 0.0]])))),
        ("penalty_rank value", dict(rank=A(3)), INVALID, "penalty_rank must be an integer in 1 .. n_j (group 0)"),
        ("penalty_rank fraction", dict(rank=A(1.5)), INVALID, "penalty_rank must be an integer in 1 .. n_j (group 0)", dict(alt=True)),
        HIER_F64, HIER_F64_ALT,
        ("state > 64", Q64, UNSUPPORTED,
         "structured group priors: the state dimension (coefficients + groups) must be <= 64 (65)"),
        OUT_NULL,
    ],
    "potential_create_glm_hier_dispersion": [
        PARAM, XY_NULL, XY_NULL_Y,
        ("family", dict(family=_lib.GLM_LOGISTIC), INVALID,
         "the family must be gaussian (3) or negbinomial (4): logistic and poisson with sampled group scales are "
         "pbbi_potential_create_glm_hier / _hier_ex"),
        ("family poisson", dict(family=_lib.GLM_POISSON), INVALID,
         "the family must be gaussian (3) or negbinomial (4): logistic and poisson with sampled group scales are "
         "pbbi_potential_create_glm_hier / _hier_ex", dict(alt=True)),
        *HIER, *OBS_DISP, X_FINITE, *THETA, HELD_NAN, HIER_F64, HIER_F64_ALT,
        ("state > 64", dict(D=63, X=np.ones((3, 63)), prior_precision=np.ones(63), groups=[0] * 63), UNSUPPORTED,
         "random effects for the dispersion families (gaussian, centred): the state dimension (coefficients + groups + 1 for a "
         "sampled dispersion) must be <= 64 (65): a kernel is shipped only if it builds without register spills to memory, "
         "and there is none at 65 .. 128 rows"),
        ("state > 64, negbinomial, non-centred, held",
         dict(D=64, X=np.ones((3, 64)), prior_precision=np.ones(64), groups=[0] * 64, family=_lib.GLM_NEGBINOMIAL, y=A(0, 1, 2),
              parametrisation=_lib.HIER_NONCENTRED, sample=0, log_dispersion_prior=None), UNSUPPORTED,
         "random effects for the dispersion families (negbinomial, non-centred): the state dimension (coefficients + groups + 1 "
         "for a sampled dispersion) must be <= 64 (65): a kernel is shipped only if it builds without register spills to "
         "memory, and there is none at 65 .. 128 rows", dict(alt=True)),
        OUT_NULL,
    ],
    "glm_pack_design": [
        ("D < 1", dict(D=0), INVALID, "need 1 <= D <= 128 and M >= 1"),
        ("D > 128", dict(D=129), INVALID, "need 1 <= D <= 128 and M >= 1", dict(alt=True)),
        ("M < 1", dict(M=0), INVALID, "need 1 <= D <= 128 and M >= 1", dict(alt=True)),
        ("X NULL", dict(X=None), INVALID, "X is NULL"),
        ("short out", dict(out_len=4 * 16 * 32 - 1), INVALID, "out is shorter than the image"),
    ],
    "glm_pack_observations": [
        OBS[0], OBS[1],
        ("y NULL", dict(y=None), INVALID, "y is NULL"),
        after(OBS[2]), *OBS[3:],
        ("short out", dict(out_len=191), INVALID, "out is shorter than the three streams"),
    ],
    "glm_pack_observations_dispersion": [
        OBS_DISP[0], OBS_DISP[1],
        ("y NULL", dict(y=None), INVALID, "y is NULL"),
        after(OBS_DISP[2], pair=False), *OBS_DISP[3:],   # no y is NULL and not finite
        ("short out", dict(out_len=191), INVALID, "out is shorter than the three streams"),
    ],
    "glm_softmax_layout": [
        ("K > 8", dict(K=9), UNSUPPORTED, SMX_RULE),
        ("K < 2", dict(K=1), UNSUPPORTED, SMX_RULE, dict(alt=True)),
        ("D < 1", dict(D=0), UNSUPPORTED, SMX_RULE, dict(alt=True)),
        ("D > 64", dict(D=65, K=2), UNSUPPORTED, SMX_RULE, dict(alt=True)),
        ("K * Dc > 128 (K > 8 is refused before Dc is formed)", dict(D=17, K=8), UNSUPPORTED, SMX_RULE, dict(pair=False)),
    ],
    "glm_pack_prior_groups": [
        *HIER,
        ("state > 128", dict(D=128, prior_precision=np.ones(128), groups=[0] * 128), UNSUPPORTED,
         "hierarchical prior: coefficients + groups must be <= 128 (129)"),
        ("out NULL", dict(out=None), INVALID, "out / n_out is NULL"),
        ("n_out NULL", dict(n_out=None), INVALID, "out / n_out is NULL", dict(alt=True)),
    ],
    "glm_pack_prior_groups_dispersion": [
        *HIER, *THETA,
        ("state > 128", dict(D=127, prior_precision=np.ones(127), groups=[0] * 127), UNSUPPORTED,
         "hierarchical prior: coefficients + groups + 1 for a sampled dispersion must be <= 128 (129)"),
        ("out NULL", dict(out=None), INVALID, "out / n_out is NULL"),
        ("n_out NULL", dict(n_out=None), INVALID, "out / n_out is NULL", dict(alt=True)),
    ],
    "glm_pack_penalty": [
        ("D < 1", dict(D=0), INVALID, "need D >= 1, 1 <= J <= 4 and D + J <= 128"),
        ("J < 1", dict(J=0), INVALID, "need D >= 1, 1 <= J <= 4 and D + J <= 128", dict(alt=True)),
        ("J > 4", dict(J=5), INVALID, "need D >= 1, 1 <= J <= 4 and D + J <= 128", dict(alt=True)),
        ("D + J > 128", dict(D=128), INVALID, "need D >= 1, 1 <= J <= 4 and D + J <= 128", dict(alt=True)),
        ("penalty NULL", dict(penalty=None), INVALID, "penalty is NULL"),
        ("short out", dict(out_len=255), INVALID, "out is shorter than the image"),
    ],
}


def _opts(step):
    return step[4] if len(step) > 4 else {}


SINGLES = [(entry, step) for entry, seq in SEQUENCES.items() for step in seq]
PAIRS = []
for _entry, _seq in SEQUENCES.items():
    _chain = [s for s in _seq if not _opts(s).get("alt")]
    PAIRS += [(_entry, a, b) for a, b in zip(_chain, _chain[1:]) if _opts(b).get("pair") is not False]


@pytest.mark.parametrize("entry,step", SINGLES, ids=[f"{e[17:] or e}-{s[0]}" if e.startswith("potential_create_") else
                                                     f"{e}-{s[0]}" for e, s in SINGLES])
def test_each_rejection_alone(entry, step):
    _, wrong, code, text = step[:4]
    assert call(entry, dict(VALID[entry], **wrong)) == (code, text)


@pytest.mark.parametrize("entry,first,second", PAIRS, ids=[f"{e}-{a[0]}+{b[0]}" for e, a, b in PAIRS])
def test_the_earlier_of_two_faults_is_reported(entry, first, second):
    """Both rules broken in one call: the entry reports the one it checks first."""
    opts = _opts(second)
    both = dict(VALID[entry], **opts["pair"]) if "pair" in opts else dict(VALID[entry], **second[1], **first[1])
    if "pair" not in opts:
        assert not set(first[1]) & set(second[1]), "the two single calls change the same argument: give the pair its own call"
    assert call(entry, both) == (first[2], opts.get("pair_text", first[3]))


@pytest.mark.parametrize("entry", sorted(VALID))
def test_a_valid_call_passes_every_check(entry):
    rc, msg = call(entry, VALID[entry])
    if entry.startswith("potential_create_"):
        assert rc == _lib.OK or (rc == HIP and msg.startswith("hipGetDeviceCount(&count): ")), (rc, msg)
    else:
        assert rc == _lib.OK, msg


def test_the_census_covers_every_entry():
    lib_entries = {n[5:] for n in _lib.PROTOTYPES if n.startswith("pbbi_potential_create_glm") or n.startswith("pbbi_glm_")}
    assert set(SEQUENCES) == set(VALID) == set(SPECS) == lib_entries - {"glm_hier_dispersion_max_dim"}
    lib = _lib.load()
    dims = {(f, p): lib.pbbi_glm_hier_dispersion_max_dim(f, p) for f in range(6) for p in range(3)}
    assert dims == {(f, p): (64 if f in (_lib.GLM_GAUSSIAN, _lib.GLM_NEGBINOMIAL) and p in (0, 1) else 0)
                    for f in range(6) for p in range(3)}

