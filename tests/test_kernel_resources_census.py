"""Resource guard for the census kernels (CPU test, as test_kernel_resources: the gfx950 code
objects' own metadata). DESIGN §4.4b sizes the two bitmap passes' grid at four 256-thread
workgroups a CU so that the whole grid is resident at once; that needs <= 128 VGPRs and <= 40 KB
of LDS a workgroup. None of the kernels may spill: the passes' inner loop is a gather per set bit."""
import pytest

from test_kernel_resources import _per_cu, kernels  # noqa: F401  (kernels: the module's fixture)

# kernel -> workgroups a CU the launch arithmetic relies on (the per-rank kernels: any)
EXPECT = {
    "14k_census_countE": 4,
    "15k_census_behindE": 4,
    "12k_census_refE": 1,
    "15k_census_finishE": 1,
}


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_census_kernel_resources(kernels, name):  # noqa: F811
    hits = {n: k for n, k in kernels.items() if name in n}
    assert hits, f"{name}: no such kernel in the library"
    for n, k in hits.items():
        assert k.get("private_segment_fixed_size", 0) == 0, f"{n}: {k['private_segment_fixed_size']} B of scratch"
        got = _per_cu(k)
        assert got >= EXPECT[name], (f"{n}: {got} workgroups a CU (VGPRs {k.get('vgpr_count')}, "
                                     f"LDS {k.get('group_segment_fixed_size')} B), the design assumes "
                                     f"{EXPECT[name]}")
