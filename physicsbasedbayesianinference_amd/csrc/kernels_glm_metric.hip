// kernels_glm_metric.hip -- the METRIC = GLM_METRIC_DIAG instantiations of k_glm (the diagonal metric of a GLM handle), compiled
// from kernels_glm.hip as a translation unit of their own: the device code, the case lists and the reason are there.
#define PBBI_GLM_METRIC_TU 1
#include "kernels_glm.hip"
