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

/* The images pbbi_potential_set_metric_dense uploads, on the HOST (touches no device), and the check of the matrix.  M: (D x D)
 * row-major, the mass matrix.  Rules, in this order: 1 <= D <= 64 (PBBI_ERR_UNSUPPORTED: the kernels keep a (DP x DP) image in
 * LDS); every entry finite; symmetric, max|M - M^T| <= 1e-12 max|M| -- (M + M^T) / 2 is what is used; positive definite: the
 * Cholesky factorisation M = L L^T completes with every pivot > 0 (each PBBI_ERR_INVALID, nothing written).
 * *len_out <- the length 3 DP^2 in doubles, DP = D padded to 16 / 32 / 64; with `out` non-NULL (out_len >= that length) three
 * (DP x DP) images, C = M^-1, then L, then M, each the identity on rows and columns >= D and each laid out like the image of
 * pbbi_glm_pack_penalty (pbbi.h): one block per 16 rows, in the order of P1 of pbbi_glm_pack_design with the rows of the matrix
 * in the role of observations,
 *     out[m DP^2 + ((t * DP/8 + s2) * 64 + lane) * 2 + e] = A_m[16 t + (lane & 15)][4 (2 s2 + e) + (lane >> 4)]
 * for t < DP/16, s2 < DP/8 and A_0 = C, A_1 = L, A_2 = M. */
int pbbi_glm_pack_metric_dense(int D, const double* M, double* out, int64_t out_len, int64_t* len_out);

#ifdef __cplusplus
}
#endif
#endif /* PBBI_GLM_METRIC_H */
