"""Code-generation guards for the MerkleMap kernels (CPU: hipcc cross-compiles gfx950 without a GPU): no scratch, no SGPR hazard,
the hashing kernels within the 128 VGPRs the path-check kernels hold to, and the tree kernels they run beside still at their
occupancy."""
import pytest

import device_build as device
import isa_lint

KERNELS = ["k_mm_check", "k_mm_diff", "k_mm_gather", "k_mm_leaves", "k_mm_level", "k_mm_cap", "k_mm_get", "k_mm_verify"]
HASHING = ["k_mm_leaves", "k_mm_level", "k_mm_verify"]


@pytest.fixture(scope="module")
def device_build():
    return device.cross_compile()


def _one(remarks, fragment):
    found = [k for n, k in remarks.items() if fragment in n]
    assert len(found) == 1, (fragment, found)
    return found[0]


@pytest.mark.parametrize("fragment", KERNELS)
def test_no_scratch(device_build, fragment):
    k = _one(device_build[0], fragment)
    print(fragment, k)
    assert k["ScratchSize"] == 0, k


def test_no_sgpr_hazard(device_build):
    asm = device_build[1]
    names = isa_lint.parse_functions(asm)
    for fragment in KERNELS:
        assert sum(fragment in n for n in names) == 1, fragment
    assert isa_lint.sgpr_hazards(asm, only=KERNELS) == []


@pytest.mark.parametrize("fragment", HASHING)
def test_hashing_kernels_hold_the_path_checks_budget(device_build, fragment):
    assert _one(device_build[0], fragment)["VGPRs"] <= 128


def test_neighbours_keep_their_occupancy(device_build):
    """the kernels the maps run beside and reuse code from: the leaf kernel's five waves per SIMD, the path check's and the
    update level's 128 VGPRs"""
    remarks = device_build[0]
    assert _one(remarks, "k_hash_leaves")["Occupancy"] == 5
    assert _one(remarks, "k_mt_verify")["VGPRs"] <= 128
    assert _one(remarks, "k_mu_fast_level")["VGPRs"] <= 128
