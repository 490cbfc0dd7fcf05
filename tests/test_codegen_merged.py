"""Code-generation guards for the merged middle of Poseidon (CPU: hipcc cross-compiles gfx950 without a GPU).  test_codegen.py
covers every kernel by fragment; this names k_merged_middle, the test entry point built like the hash kernels, so that a rename
cannot drop it, and the tree kernel that test_codegen.py does not list."""
import pytest

import device_build as device
import isa_lint


@pytest.fixture(scope="module")
def device_build():
    return device.cross_compile()


def _kernels(info, fragment):
    found = [info[n] for n in info if fragment in n]
    assert found, fragment
    return found


@pytest.mark.parametrize("fragment", ["k_merged_middle", "k_merkle_topEP"])
def test_five_waves_within_102_vgprs_without_scratch(device_build, fragment):
    for k in _kernels(device_build[0], fragment):
        assert k["ScratchSize"] == 0, k
        assert k["VGPRs"] + k.get("AGPRs", 0) <= 102 and k["Occupancy"] >= 5, k


def test_the_build_has_no_sgpr_hazard(device_build):
    asm = device_build[1]
    assert any("k_merged_middle" in f for f in isa_lint.parse_functions(asm))
    assert isa_lint.sgpr_hazards(asm) == []
