"""Occupancy guard for the ticketed sorted-tile kernel (CPU test, as test_kernel_resources_sorted:
the gfx950 code object's own metadata). The launcher sizes k_lookupn_sorted_ticket<256, 3>'s grid
from the occupancy query and DESIGN §4.2 relies on four 4-wave workgroups a CU, like the strided
kernel it shares its tile body with: at most 128 VGPRs and no scratch."""
from test_kernel_resources import _per_cu, kernels  # noqa: F401  (kernels: the module's fixture)

NAME = "k_lookupn_sorted_ticketILi256ELi3E"


def test_ticket_kernel_resources(kernels):  # noqa: F811
    hits = {n: k for n, k in kernels.items() if NAME in n}
    assert len(hits) == 1, f"{NAME}: {len(hits)} such kernels in the library"
    for n, k in hits.items():
        assert _per_cu(k) >= 4, (n, k.get("vgpr_count"), k.get("group_segment_fixed_size"))
        assert k.get("vgpr_count", 0) + k.get("agpr_count", 0) <= 128, n
        assert k.get("private_segment_fixed_size", 0) == 0, n
        assert k.get("vgpr_spill_count", 0) == 0, n
