"""Host side of the diagonal metric of user-defined potentials: where the mixin lives, and what the plugin's METRIC
kernels cost -- from hipcc's own resource remarks of a cross-compile, no GPU."""
import os

import pytest

from custom_sources import QUARTIC


def test_metric_mixin_lives_in_potential_and_custom_potentials_carry_it():
    from physicsbasedbayesianinference_amd import custom, glm, potential
    assert glm._Metric is potential._Metric
    assert issubclass(custom.CustomPotential, potential._Metric)
    assert callable(custom.CustomPotential.set_metric) and isinstance(custom.CustomPotential.metric, property)
    for cls in (glm.GLM, glm.SoftmaxGLM, glm.DispersionGLM, glm.HierarchicalGLM):
        assert issubclass(cls, potential._Metric)
    for cls in (potential.Harmonic, potential.GaussianDiag, potential.GaussianDense, potential.Rosenbrock):
        assert not hasattr(cls, "set_metric")


def test_plugin_abi_is_5():
    from physicsbasedbayesianinference_amd import custom
    with open(os.path.join(custom._CSRC, "pbbi_internal.h")) as f:
        assert "#define PBBI_PLUGIN_ABI 5 " in f.read()


SMALL = '''
template <class Q>
PBBI_FN T potential(const Q& q, int D, const T* prm) {
    T s = 0;
    for (int j = 0; j < D; ++j) s += prm[0] * (q[j] * q[j]);
    return T(0.5) * s;
}
template <class Q, class G>
PBBI_FN void gradient(const Q& q, G& g, int D, const T* prm) {
    for (int j = 0; j < D; ++j) g[j] = prm[0] * q[j];
}
'''


def test_plugin_with_metric_kernels_cross_compiles():
    """plugin_source of a small source still builds with hipcc --offload-arch=gfx950 on a machine without a GPU, through
    compile_plugin, in both dtypes, and exports the route query of ABI 5."""
    from physicsbasedbayesianinference_amd.custom import compile_plugin, plugin_source
    assert "pbbi_custom.h" in plugin_source(SMALL, "float64", 3)
    for dtype in ("float64", "float32"):
        so = compile_plugin(SMALL, dtype, D=3)
        assert os.path.exists(so)
        with open(so, "rb") as f:
            blob = f.read()
        assert b"pbbi_plugin_hmc_route" in blob and b"pbbi_plugin_hmc_iter" in blob


@pytest.mark.parametrize("D", [11, 16])
def test_metric_register_kernels_need_no_scratch(D):
    """hipcc's resource remarks (-Rpass-analysis=kernel-resource-usage, the file compile_plugin(remarks=True) keeps) of the
    quartic plugin at D = 11 and D = 16, fp64: every METRIC register kernel -- k_custom_reg_hmc in reference order and in
    kick-drift-kick form, k_custom_reg_integrate -- reserves no scratch memory, and each has its parent beside it.  (A twin
    that did would not be launched: the plugin asks its code object and falls back to the workspace kernels.)"""
    from physicsbasedbayesianinference_amd.custom import plugin_resources
    res = plugin_resources(QUARTIC, "float64", D)
    twins = [k for k in res if k.startswith("k_custom_reg_") and k.endswith(",1>")]
    # reference order: method x unit mass; kick-drift-kick form: Leapfrog x unit mass
    assert len([k for k in twins if k.startswith("k_custom_reg_hmc<")]) == 6
    assert len([k for k in twins if k.startswith("k_custom_reg_integrate<")]) == 4
    for k in twins:
        parent = k[:-3] + ",0>"
        print(k, res[k], "parent", res[parent])
        assert res[k]["scratch"] == 0, (k, res[k])
    assert all(v["scratch"] == 0 for k, v in res.items() if k.startswith("k_custom_reg_"))
