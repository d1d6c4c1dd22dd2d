/* pbbi_glm_ordinal.h -- part of pbbi.h (which includes it, and has the model beside PBBI_GLM_ORDINAL): the two entries of
 * ordinal (cumulative-logit) regression.  They stand in a file of their own because they are bound and tested apart from the
 * entries of pbbi.h, as pbbi_glm_metric.h's is: the order of their rejections is spelt out in tests/test_glm_ordinal_host.py, and
 * physicsbasedbayesianinference_amd/_lib.py lists them under ORDINAL_PROTOTYPES. */
#ifndef PBBI_GLM_ORDINAL_H
#define PBBI_GLM_ORDINAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The handle of the model stated in pbbi.h: lam / mu hold D + K - 1 entries, the last K - 1 the precision and mean of zeta_1 and
 * of the log-gaps (mu may be NULL = 0); the handle's dimension is D + K - 1.  X (M x D row-major), y (M categories as doubles),
 * weights / offset (M doubles or NULL = all 1 / all 0) are HOST pointers, checked and copied at creation. */
int pbbi_potential_create_glm_ordinal(int D, int K, int64_t M, const double* X, const double* y, const double* weights,
                                      const double* offset, const double* lam /* D + K - 1 */, const double* mu /* or NULL */,
                                      int dtype, int device, pbbi_potential** out);
/* The three observation streams pbbi_potential_create_glm_ordinal uploads, on the HOST (touches no device, checks the same
 * rules): *len_out <- their total length, as for pbbi_glm_pack_observations; with `out` non-NULL c = a | d = y | o, each stream
 * zero padded past M, and (counts_out != NULL) the 8 weighted category counts A_k, 0 past K. */
int pbbi_glm_pack_observations_ordinal(int64_t M, int K, const double* y, const double* weights, const double* offset,
                                       double* out, int64_t out_len, int64_t* len_out, double* counts_out);

#ifdef __cplusplus
}
#endif
#endif /* PBBI_GLM_ORDINAL_H */
