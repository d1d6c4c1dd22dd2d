/* pbbi_glm_metric.h -- part of pbbi.h (which includes it): the host-only entry of the diagonal metric of the GLM handles
 * (pbbi_potential_set_metric_diag, pbbi.h).  It stands in a file of its own because it is bound and tested apart from the entries
 * of pbbi.h: it touches no device and creates no handle, its rules are those of the table alone (tests/test_glm_metric_host.py),
 * and physicsbasedbayesianinference_amd/_lib.py lists it under HOST_PACKER_PROTOTYPES. */
#ifndef PBBI_GLM_METRIC_H
#define PBBI_GLM_METRIC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The table pbbi_potential_set_metric_diag uploads, on the HOST (touches no device), and the check of its entries: *len_out <-
 * its length 2 DP in doubles, DP = D padded to 16 / 32 / 64 / 128 (1 <= D <= 128); with `out` non-NULL (out_len >= that
 * length) the table out[2 d] = m_d, out[2 d + 1] = 1 / m_d for d < D and {1, 1} for D <= d < DP -- the 16-byte entries the
 * kernels read.  An entry that is zero, negative, NaN or infinite: PBBI_ERR_INVALID, nothing written. */
int pbbi_glm_pack_metric(int D, const double* mass_diag, double* out, int64_t out_len, int64_t* len_out);

#ifdef __cplusplus
}
#endif
#endif /* PBBI_GLM_METRIC_H */
