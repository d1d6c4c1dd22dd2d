// kernels_glm_dense_metric.hip -- the METRIC = GLM_METRIC_DENSE instantiations of k_glm (the dense metric of a GLM handle),
// compiled from kernels_glm.hip as a translation unit of their own: the device code, the case lists and the reason are there.
#define PBBI_GLM_METRIC_TU 2
#include "kernels_glm.hip"
