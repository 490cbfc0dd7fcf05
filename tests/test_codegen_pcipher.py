"""Code-generation guards for the Poseidon-cipher batch kernels (CPU: hipcc cross-compiles gfx950 without a GPU): each exists
once, no SGPR hazard, no scratch, no LDS, registers within 256, their figures printed and pinned to what the build gives (DESIGN.md
section 9j records them and says which live values hold them below k_hash_leaves' five waves), and the kernels they were built
beside keep theirs."""
import pytest

import device_build as device
import isa_lint
from test_codegen_elgamal import SCHNORR
from test_codegen_schnorr import ECWITNESS, _one

KERNELS = ["k_pcipher_encrypt", "k_pcipher_decrypt"]
# DESIGN.md section 9j's table: kernel -> (VGPRs + AGPRs, waves per SIMD)
FIGURES = {"k_pcipher_encrypt": (121, 4), "k_pcipher_decrypt": (127, 4)}


@pytest.fixture(scope="module")
def device_build():
    return device.cross_compile()


@pytest.mark.parametrize("fragment", KERNELS)
def test_figures(device_build, fragment):
    k = _one(device_build[0], fragment)
    print("%s: VGPRs %d, AGPRs %d, ScratchSize %d, Occupancy %d" % (fragment, k["VGPRs"], k.get("AGPRs", 0), k["ScratchSize"], k["Occupancy"]))
    assert k["ScratchSize"] == 0 and k.get("LDS Size", 0) == 0 and k["VGPRs"] + k.get("AGPRs", 0) <= 256, k
    assert (k["VGPRs"] + k.get("AGPRs", 0), k["Occupancy"]) == FIGURES[fragment], k


def test_no_sgpr_hazard(device_build):
    asm = device_build[1]
    names = isa_lint.parse_functions(asm)
    for fragment in KERNELS:
        assert sum(fragment in n for n in names) == 1, fragment
    assert isa_lint.sgpr_hazards(asm, only=KERNELS) == []


def test_neighbours_keep_their_figures(device_build):
    remarks = device_build[0]
    for fragment, want in SCHNORR.items():
        k = _one(remarks, fragment)
        assert (k["VGPRs"] + k.get("AGPRs", 0), k["ScratchSize"], k["Occupancy"]) == (want[0], 0, want[1]), (fragment, k)
    assert _one(remarks, "k_hash_leaves")["Occupancy"] == 5
    q = _one(remarks, "k_vfy_queries")
    assert (q["VGPRs"] + q.get("AGPRs", 0), q["ScratchSize"]) == (92, 0), q
    for inst, want in ECWITNESS.items():
        k = _one(remarks, "k_ecwitness" + inst)
        assert (k["VGPRs"], k["ScratchSize"], k["Occupancy"]) == want, (inst, k)
