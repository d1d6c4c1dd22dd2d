// kernels_glm_softmax_metric.hip -- the METRIC = true instantiations of k_glm_softmax, compiled from kernels_glm_softmax.hip as
// a translation unit of their own (kernels_glm.hip says why).
#define PBBI_GLM_METRIC_TU 1
#include "kernels_glm_softmax.hip"
