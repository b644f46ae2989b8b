"""Resource guard for the side-summary kernels (CPU test, as test_kernel_resources: the gfx950 code
objects' own metadata). Neither kernel waits for another workgroup, so no residency is assumed; the
row sweep's inner loop is three 16-byte loads and sixteen byte tests a lane, which must stay in
registers: no scratch, and at least the eight 256-thread workgroups a CU its grid is sized for
(k_side_cross is launched 16 a CU, two rounds of them)."""
import pytest

from test_kernel_resources import _per_cu, kernels  # noqa: F401  (kernels: the module's fixture)

EXPECT = {
    "9k_side_ckE": 8,
    "12k_side_crossE": 8,
}


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_side_summary_kernel_resources(kernels, name):  # noqa: F811
    hits = {n: k for n, k in kernels.items() if name in n}
    assert hits, f"{name}: no such kernel in the library"
    for n, k in hits.items():
        assert k.get("private_segment_fixed_size", 0) == 0, f"{n}: {k['private_segment_fixed_size']} B of scratch"
        assert k.get("group_segment_fixed_size", 0) == 0, f"{n}: uses LDS"
        got = _per_cu(k)
        assert got >= EXPECT[name], f"{n}: {got} workgroups a CU (VGPRs {k.get('vgpr_count')})"
