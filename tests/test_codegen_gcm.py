"""Code-generation guards for the AES-GCM batch kernels (CPU: hipcc cross-compiles gfx950 without a GPU): each exists once, no
SGPR hazard, no scratch, registers within 256, LDS within what DESIGN.md section 9k states, their figures printed and pinned to
what the build gives, and the kernels they were built beside keep theirs."""
import pytest

import device_build as device
import isa_lint
from test_codegen_pcipher import FIGURES as PCIPHER
from test_codegen_schnorr import _one

# DESIGN.md section 9k's table: mangled-name fragment -> (VGPRs + AGPRs, waves per SIMD, LDS bytes per workgroup)
FIGURES = {"k_gcm_setup": (44, 8, 1024), "k_gcm_ctrILb1E": (35, 8, 1024), "k_gcm_ctrILb0E": (35, 8, 1024), "k_gcm_ghashILi1E": (74, 3, 16384),
           "k_gcm_ghashILi64E": (52, 8, 1280), "k_aes_encrypt_blocks": (35, 8, 1024), "k_bytes_to_words": (11, 8, 0)}
KERNELS = list(FIGURES)


@pytest.fixture(scope="module")
def device_build():
    return device.cross_compile()


@pytest.mark.parametrize("fragment", KERNELS)
def test_figures(device_build, fragment):
    k = _one(device_build[0], fragment)
    print("%s: VGPRs %d, AGPRs %d, ScratchSize %d, Occupancy %d, LDS %d" % (fragment, k["VGPRs"], k.get("AGPRs", 0), k["ScratchSize"], k["Occupancy"], k.get("LDS Size", 0)))
    assert k["ScratchSize"] == 0 and k["VGPRs"] + k.get("AGPRs", 0) <= 256, k
    assert k.get("LDS Size", 0) <= FIGURES[fragment][2], k
    assert (k["VGPRs"] + k.get("AGPRs", 0), k["Occupancy"], k.get("LDS Size", 0)) == FIGURES[fragment], k


def test_each_exists_once_and_has_no_sgpr_hazard(device_build):
    asm = device_build[1]
    names = isa_lint.parse_functions(asm)
    for fragment in KERNELS:
        assert sum(fragment in n for n in names) == 1, fragment
    assert isa_lint.sgpr_hazards(asm, only=KERNELS) == []


def test_neighbours_keep_their_figures(device_build):
    remarks = device_build[0]
    for fragment, want in PCIPHER.items():
        k = _one(remarks, fragment)
        assert (k["VGPRs"] + k.get("AGPRs", 0), k["ScratchSize"], k["Occupancy"]) == (want[0], 0, want[1]), (fragment, k)
    assert _one(remarks, "k_hash_leaves")["Occupancy"] == 5
    q = _one(remarks, "k_vfy_queries")
    assert (q["VGPRs"] + q.get("AGPRs", 0), q["ScratchSize"]) == (92, 0), q
