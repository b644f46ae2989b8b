"""Resource guard for the timeline kernels (CPU test, as test_kernel_resources_census: the gfx950
code objects' own metadata). DESIGN §4.4c launches the bitmap pass on the census's grid of four
256-thread workgroups a CU; none of the kernels may spill."""
import pytest

from test_kernel_resources import _per_cu, kernels  # noqa: F401  (kernels: the module's fixture)

# kernel -> workgroups a CU the launch arithmetic relies on (the per-rank and one-wave kernels: any)
EXPECT = {
    "10k_tl_beginE": 1,
    "10k_tl_countE": 4,
    "11k_tl_finishE": 1,
}


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_timeline_kernel_resources(kernels, name):  # noqa: F811
    hits = {n: k for n, k in kernels.items() if name in n}
    assert hits, f"{name}: no such kernel in the library"
    for n, k in hits.items():
        assert k.get("private_segment_fixed_size", 0) == 0, f"{n}: {k['private_segment_fixed_size']} B of scratch"
        got = _per_cu(k)
        assert got >= EXPECT[name], (f"{n}: {got} workgroups a CU (VGPRs {k.get('vgpr_count')}, "
                                     f"LDS {k.get('group_segment_fixed_size')} B), the design assumes "
                                     f"{EXPECT[name]}")
