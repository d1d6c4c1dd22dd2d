// glm_args.h -- the part of k_glm's and k_glm_softmax's kernel arguments that comes from a call: GlmPrm and SmxPrm name these
// members alike, so one filler per kind of call serves both.  `mode` is the kernel's own GLM_* / SMX_* constant.  Members a call
// does not name keep what glm_prm / smx_prm gave them from the handle (kT = 1 outside an HMC iteration).
#pragma once
#include "pbbi_internal.h"

// what no GLM kernel serves
inline int glm_check_iter(const IterArgs& a) {
    if (pbbi_dyn(a)) return pbbi_fail(PBBI_ERR_UNSUPPORTED, "GLM potentials: fixed trajectory lengths only");
    if (a.fuse_S > 1) return pbbi_fail(PBBI_ERR_INVALID, "the GLM kernel takes one iteration per launch (internal)");
    return PBBI_OK;
}

template <class Prm>
void glm_fill(Prm& prm, const IterArgs& a, int mode) {
    prm.q_in = (const double*)a.q_in;
    prm.p_in = (const double*)a.p_in;
    prm.u_in = (const double*)a.u_in;
    prm.mass = (const double*)a.mass;
    prm.q_out = (double*)a.q_out;
    prm.p_out = (double*)a.p_out;
    prm.ratio_out = (double*)a.ratio_out;
    prm.reject_out = a.reject_out;
    prm.N = a.N; prm.ldn_in = a.ldn_in; prm.ldn_out = a.ldn_out;
    prm.h = a.h; prm.kT = a.kT; prm.L = a.L; prm.flags = a.flags; prm.rng = a.rng;
    prm.mode = mode; prm.method = a.method;
    prm.seed = a.seed; prm.iter = a.iter; prm.chain0 = a.chain0;
}

template <class Prm>
void glm_fill(Prm& prm, const IntegrateArgs& a, int mode) {  // in place
    prm.q_in = (const double*)a.q;
    prm.p_in = (const double*)a.p;
    prm.mass = (const double*)a.mass;
    prm.q_out = (double*)a.q;
    prm.p_out = (double*)a.p;
    prm.v_out = (double*)a.v_out;
    prm.N = a.N; prm.ldn_in = a.ldn; prm.ldn_out = a.ldn;
    prm.h = a.h; prm.L = a.L; prm.mode = mode; prm.method = a.method;
}

template <class Prm>
void glm_fill(Prm& prm, const EvalArgs& a, int mode) {
    prm.q_in = (const double*)a.q;
    prm.p_in = (const double*)a.p;
    prm.mass = (const double*)a.mass;
    prm.U_out = (double*)a.U_out;
    prm.grad_out = (double*)a.grad_out;
    prm.w_out = (double*)a.w_out;
    prm.N = a.N; prm.ldn_in = a.ldn; prm.ldn_out = a.ldn;
    prm.mode = mode;
}
