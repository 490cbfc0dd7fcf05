"""Code-generation guards for the ecGFp5 batch kernels (CPU: hipcc cross-compiles gfx950 without a GPU): each exists once, no
SGPR hazard, no scratch, their register figures printed and held to the budget of DESIGN.md section 9g, and the kernels they were
built beside keep the figures their own tests and DESIGN.md section 9d record."""
import pytest

import device_build as device
import isa_lint

KERNELS = ["k_ec_mul_batch", "k_schnorr_sign", "k_schnorr_verify"]
# DESIGN.md section 9d's table: instantiation -> (VGPRs, scratch bytes per lane, waves per SIMD)
ECWITNESS = {"ILb0ELb0E": (249, 0, 2), "ILb0ELb1E": (252, 0, 2), "ILb1ELb0E": (256, 1280, 2), "ILb1ELb1E": (256, 1296, 2)}


@pytest.fixture(scope="module")
def device_build():
    return device.cross_compile()


def _one(remarks, fragment):
    found = [k for n, k in remarks.items() if fragment in n]
    assert len(found) == 1, (fragment, found)
    return found[0]


@pytest.mark.parametrize("fragment", KERNELS + ["k_ec_scalar_muladd"])
def test_figures(device_build, fragment):
    """one thread per item at 64 threads per block: a ladder's accumulator, addend and temporaries fit in registers (no scratch)
    within k_ecwitness's budget of 256, two waves per SIMD or more"""
    k = _one(device_build[0], fragment)
    print("%s: VGPRs %d, AGPRs %d, ScratchSize %d, Occupancy %d" % (fragment, k["VGPRs"], k.get("AGPRs", 0), k["ScratchSize"], k["Occupancy"]))
    assert k["ScratchSize"] == 0 and k["VGPRs"] + k.get("AGPRs", 0) <= 256 and k["Occupancy"] >= 2, k


def test_no_sgpr_hazard(device_build):
    asm = device_build[1]
    names = isa_lint.parse_functions(asm)
    for fragment in KERNELS:
        assert sum(fragment in n for n in names) == 1, fragment
    assert isa_lint.sgpr_hazards(asm, only=KERNELS) == []


def test_neighbours_keep_their_figures(device_build):
    remarks = device_build[0]
    assert _one(remarks, "k_hash_leaves")["Occupancy"] == 5
    q = _one(remarks, "k_vfy_queries")
    assert (q["VGPRs"] + q.get("AGPRs", 0), q["ScratchSize"]) == (92, 0), q
    for inst, want in ECWITNESS.items():
        k = _one(remarks, "k_ecwitness" + inst)
        assert (k["VGPRs"], k["ScratchSize"], k["Occupancy"]) == want, (inst, k)
