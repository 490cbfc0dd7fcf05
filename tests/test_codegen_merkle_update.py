"""Code-generation guards for the leaf-update kernels (CPU: hipcc cross-compiles gfx950 without a GPU): no scratch, no SGPR hazard,
and the kernels that hash within the path check's budget of 128 VGPRs."""
import pytest

import device_build as device
import isa_lint

KERNELS = ["k_mu_leaves", "k_mu_fast_leaf", "k_mu_fast_level", "k_mu_gather", "k_mu_step", "k_mu_roots"]
HASHING = ["k_mu_leaves", "k_mu_fast_level", "k_mu_step"]


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
    k = _one(device_build[0], fragment)
    assert k["VGPRs"] + k.get("AGPRs", 0) <= 128 and k["Occupancy"] >= 4, k
