"""Code-generation guards for the ElGamal batch kernels (CPU: hipcc cross-compiles gfx950 without a GPU): each exists once, no
SGPR hazard, no scratch, their register figures printed and held to the budget tests/test_codegen_schnorr.py holds the ladder
kernels to (DESIGN.md section 9i records the figures), and the kernels they were built beside keep theirs."""
import pytest

import device_build as device
import isa_lint
from test_codegen_schnorr import ECWITNESS, _one

KERNELS = ["k_ec_decompress_batch", "k_ec_encode_binary", "k_elgamal_encrypt", "k_elgamal_decrypt", "k_hashed_elgamal_encrypt", "k_hashed_elgamal_decrypt",
           "k_ec_scalar_bits"]
# DESIGN.md section 9g's table: kernel -> (VGPRs, waves per SIMD)
SCHNORR = {"k_ec_mul_batch": (162, 3), "k_schnorr_sign": (184, 2), "k_schnorr_verify": (175, 2)}


@pytest.fixture(scope="module")
def device_build():
    return device.cross_compile()


@pytest.mark.parametrize("fragment", KERNELS)
def test_figures(device_build, fragment):
    """one thread per item at 64 threads per block: a square root's or a ladder's temporaries fit in registers (no scratch) within
    the budget of 256, two waves per SIMD or more"""
    k = _one(device_build[0], fragment)
    print("%s: VGPRs %d, AGPRs %d, ScratchSize %d, Occupancy %d" % (fragment, k["VGPRs"], k.get("AGPRs", 0), k["ScratchSize"], k["Occupancy"]))
    assert k["ScratchSize"] == 0 and k["VGPRs"] + k.get("AGPRs", 0) <= 256 and k["Occupancy"] >= 2, k
    assert k.get("LDS Size", 0) == 0


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
