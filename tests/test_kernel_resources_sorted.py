"""Occupancy guard for the sorted-tile lookupN(3) kernel (CPU test, as test_kernel_resources:
the gfx950 code object's own metadata). DESIGN §4.2 relies on k_lookupn_sorted<256, 3> running
four 4-wave workgroups a CU like the lean kernel it replaced as the default; the larger shapes are
A/B variants that need at least one workgroup (16 waves at <= 128 VGPRs) and two."""
import pytest

from test_kernel_resources import _per_cu, kernels  # noqa: F401  (kernels: the module's fixture)

EXPECT = {
    "k_lookupn_sortedILi256ELi3E": 4,
    "k_lookupn_sortedILi512ELi3E": 2,
    "k_lookupn_sortedILi1024ELi3E": 1,
}


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_sorted_kernel_occupancy(kernels, name):  # noqa: F811
    hits = {n: k for n, k in kernels.items() if name in n}
    assert hits, f"{name}: no such kernel in the library"
    for n, k in hits.items():
        got = _per_cu(k)
        assert got >= EXPECT[name], (f"{n}: {got} workgroups a CU (VGPRs {k.get('vgpr_count')}, "
                                     f"LDS {k.get('group_segment_fixed_size')} B), the design assumes "
                                     f"{EXPECT[name]}")
