"""Resource guard for the ring-checksum kernels (CPU test, as test_kernel_resources: the gfx950
code objects' own metadata). k_rck_scan and k_rck_verify run one wave a local node and k_rck_build
one 256-thread workgroup a view to build; no workgroup waits for another, so no residency is
assumed. Their grids are sized by the work (NL / 4 workgroups, one a listed view), and the design
counts on the most a CU can hold of 256-thread workgroups, eight (32 wave slots): the built object
has 25, 23 and 44 VGPRs, far under the 64 that eight workgroups allow. The gather loops (a status
byte per set deviation bit) and the build's copies must stay in registers: no scratch. Only the
build uses LDS: three 256-word arrays (absent words, deleted-bytes scan, shifts), 3,072 bytes."""
import pytest

from test_kernel_resources import _per_cu, kernels  # noqa: F401  (kernels: the module's fixture)

EXPECT = {  # kernel: (workgroups a CU, LDS bytes)
    "10k_rck_scanE": (8, 0),
    "12k_rck_verifyE": (8, 0),
    "11k_rck_buildE": (8, 3072),
}


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_ring_checksum_kernel_resources(kernels, name):  # noqa: F811
    hits = {n: k for n, k in kernels.items() if name in n}
    assert hits, f"{name}: no such kernel in the library"
    per_cu, lds = EXPECT[name]
    for n, k in hits.items():
        assert k.get("private_segment_fixed_size", 0) == 0, f"{n}: {k['private_segment_fixed_size']} B of scratch"
        assert k.get("group_segment_fixed_size", 0) == lds, f"{n}: {k.get('group_segment_fixed_size')} B of LDS"
        got = _per_cu(k)
        assert got >= per_cu, f"{n}: {got} workgroups a CU (VGPRs {k.get('vgpr_count')})"
