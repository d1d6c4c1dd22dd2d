// pbbi_chain.h -- what the HMC kernels share: the accept test and the slab bookkeeping of a fused run.
// The end of an iteration (re-read the old position, report a momentum, store, record) and the parameter
// structs stay with each kernel: moved into a shared inlined template, or with a kernel argument moved, hipcc
// allocates these kernels differently (scratch in the C3 kernel; profiles/chain_frame_resources.txt).
#pragma once
#include "pbbi_internal.h"

// mask = u > min(1, ratio); a NaN ratio compares False and the proposal is ACCEPTED (src/HMC.py:168-173).
// The one line of the sampler whose exact form decides parity with the reference.
template <typename T>
__device__ __forceinline__ bool metropolis_reject(T ratio, T u) {
    return (ratio == ratio) && (u > (ratio < T(1) ? ratio : T(1)));
}

// Where the iterations of a fused run put their results (pbbi_hmc_run, IterArgs::fuse_*): iteration k of the
// launch writes position slab (slab0 + k), modulo 2 for a burn-in's two scratch slabs, momentum slab k,
// ratio / reject rows k.
struct ChainRun {
    int S;            // iterations in this launch (1: plain pbbi_hmc_iter semantics)
    int wrap2;        // position slabs alternate between slab 0 and 1 of q_base (burn-in)
    int64_t slab0;    // index of the first iteration's position slab
    int64_t slab;     // elements per slab (D * N)
    double* q_base;   // slab 0 of the position slabs
};

inline ChainRun chain_run(const IterArgs& a) {
    const int64_t slab = (int64_t)a.pot->D * a.N;
    if (a.fuse_S > 1) return ChainRun{a.fuse_S, a.fuse_wrap2, a.fuse_slab0, slab, (double*)a.fuse_q_base};
    return ChainRun{1, 0, 0, slab, (double*)a.q_out};  // a single iteration is a run of one whose only "slab" is q_out
}
