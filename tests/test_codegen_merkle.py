"""Code-generation guards for the stand-alone Merkle kernels (CPU: hipcc cross-compiles gfx950 without a GPU): no scratch, no
SGPR hazard, the transpose tile's padded size, and the tree kernels they run beside still at their occupancy."""
import pytest

import device_build as device
import isa_lint

KERNELS = ["k_mt_transpose", "k_mt_paths", "k_mt_verify"]


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


def test_tile_and_occupancy(device_build):
    """the transpose tile is 32 rows of 33 words (the odd stride that keeps the transposed ds_read_b64 free of bank conflicts);
    the path check holds the proof verifier's query kernel's budget (at most 128 VGPRs); the leaf kernel the trees reuse keeps
    its five waves per SIMD"""
    remarks = device_build[0]
    assert _one(remarks, "k_mt_transpose")["LDS Size"] == 32 * 33 * 8
    assert _one(remarks, "k_mt_verify")["VGPRs"] <= 128
    assert _one(remarks, "k_hash_leaves")["Occupancy"] == 5
