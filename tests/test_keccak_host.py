"""CPU checks of the Keccak configuration (hasher="keccak"): the native hasher against the Python restatement of
tests/keccak_ref.py (itself pinned by the published Keccak-256 vectors), the blob's HASH section, and the code generation of the
Keccak kernels (gfx950 cross-compile)."""
import ctypes as C
import random
import struct

import numpy as np
import pytest

import device_build
import keccak_circuits
import keccak_ref
import oracle_lib

P = 0xFFFFFFFF00000001
HASH_TAG = 0x48534148  # csrc/circuit.h BLOB_HASH_TAG


def test_python_restatement_against_the_published_vectors():
    assert keccak_ref.keccak256(b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    assert keccak_ref.keccak256(b"abc").hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"
    # the word-level sponge and the digest packing against the byte-level definition
    rnd = random.Random(1)
    for n in (4, 17, 34, 135):
        words = [rnd.randrange(P) for _ in range(n)]
        h = keccak_ref.hash_no_pad(np.array(words, dtype=np.uint64))
        assert keccak_ref.digest_bytes(h) == keccak_ref.keccak256(struct.pack("<%dQ" % n, *words))[:25]
    l, r = (keccak_ref.hash_no_pad(np.array([rnd.randrange(P) for _ in range(9)], dtype=np.uint64)) for _ in range(2))
    assert keccak_ref.digest_bytes(keccak_ref.two_to_one(l, r)) == keccak_ref.keccak256(keccak_ref.digest_bytes(l) + keccak_ref.digest_bytes(r))[:25]


def _in_range(h):
    return all(w < (1 << 56) for w in h[:3]) and h[3] < (1 << 32)


@pytest.mark.parametrize("n", [4, 16, 17, 18, 33, 34, 35, 84, 135, 139])
def test_native_hash_no_pad_equals_the_restatement(pkg, n):
    rnd = random.Random(n)
    for case in range(4):
        words = [rnd.randrange(P) for _ in range(n)] if case else [P - 1] * n
        got = pkg.keccak_native.hash_no_pad(words)
        assert got == [int(w) for w in keccak_ref.hash_no_pad(np.array(words, dtype=np.uint64))]
        assert _in_range(got)


def test_native_two_to_one_equals_the_restatement(pkg):
    rnd = random.Random(7)
    digests = [[rnd.randrange(1 << 56), rnd.randrange(1 << 56), rnd.randrange(1 << 56), rnd.randrange(1 << 32)] for _ in range(32)]
    digests += [[(1 << 56) - 1] * 3 + [(1 << 32) - 1], [0, 0, 0, 0]]
    for l, r in zip(digests, digests[1:] + digests[:1]):
        got = pkg.keccak_native.two_to_one(l, r)
        assert got == [int(w) for w in keccak_ref.two_to_one(np.array(l, dtype=np.uint64), np.array(r, dtype=np.uint64))]
        assert _in_range(got)


@pytest.mark.parametrize("name", ["gf_mul", "aes_gcm_13", "zk", "public_inputs"])
def test_blob_hash_section(pkg, name):
    """A Poseidon blob is what it always was, whichever entry built it; the Keccak blob is that blob plus the HASH section."""
    poseidon, _ = keccak_circuits.build(pkg, name, 1)
    keccak, pws = keccak_circuits.build(keccak_circuits.KeccakPkg(pkg), name, 1)
    assert keccak.blob == poseidon.blob + struct.pack("<II", HASH_TAG, 1)
    assert poseidon.info["hasher"] == "poseidon" and keccak.info["hasher"] == "keccak"
    assert {k: v for k, v in keccak.info.items() if k != "hasher"} == {k: v for k, v in poseidon.info.items() if k != "hasher"}
    # the frozen oracle (Poseidon only) still loads the Keccak blob and generates its witness
    oc = oracle_lib.OracleCircuit(keccak.blob)
    st, _ = oc.generate_witness(pws[0].map, 1 << 22)
    assert st == 0
    with pytest.raises(pkg.P2Error):
        pkg.CircuitData(poseidon.blob + struct.pack("<II", HASH_TAG, 2))
    with pytest.raises(pkg.P2Error):
        pkg.CircuitData(keccak.blob + b"\0")


def test_builder_entries_agree(pkg):
    """p2_builder_new and p2_builder_new_config(0, 0) build byte-identical blobs; an unknown hasher is an error."""
    L = pkg.lib()

    def blob_of(h):
        b = pkg.CircuitBuilder.__new__(pkg.CircuitBuilder)
        b._h = h
        lut = b.gf_2_8_mul_lut()
        x, y = b.add_virtual_byte_target_unsafe(), b.add_virtual_byte_target_unsafe()
        b.gf_2_8_mul(lut, x, y)
        return b.build().blob

    assert blob_of(L.p2_builder_new()) == blob_of(L.p2_builder_new_config(0, 0))
    assert blob_of(L.p2_builder_new_zk()) == blob_of(L.p2_builder_new_config(1, 0))
    assert not L.p2_builder_new_config(0, 2)
    with pytest.raises(pkg.P2Error):
        pkg.CircuitBuilder(hasher="sha256")


def test_host_verifier_reason_is_registered(pkg):
    assert pkg.VERIFY_REASONS["hash word out of range"] == pkg.VERIFY_NON_CANONICAL
    for f in ("p2_builder_new_config", "p2_native_keccak_hash_no_pad", "p2_native_keccak_two_to_one", "p2_gpu_merkle_cap_hasher"):
        assert f in pkg.lib()._p2_signatures and hasattr(pkg.lib(), f)


# The Keccak kernels as the implementation settled (gfx950, this ROCm's hipcc): the tree kernels hold five waves per SIMD (at
# most 102 VGPRs) without scratch, the verifier's and the compressor's hold four (at most 128).
TREE_KERNELS = ["k_kc_leaves", "k_kc_fri_leaves", "k_kc_level"]
VERIFY_KERNELS = ["k_kcv_range", "k_kcv_queries", "k_kcc_merkle"]
PINNED_FRAGMENTS = ["k_hash_leaves", "k_hash_fri_leaves", "k_merkle_level", "k_quotient", "k_ntt_r16", "k_pow", "k_challenger", "k_vfy_", "k_cmp_",
                    "k_finish", "k_proof_segments"]


def test_keccak_kernels_cross_compile_without_scratch():
    info, asm = device_build.cross_compile()
    for fragment, vgprs, waves in [(k, 102, 5) for k in TREE_KERNELS] + [(k, 128, 4) for k in VERIFY_KERNELS]:
        names = [n for n in info if fragment in n]
        assert len(names) == 1, (fragment, names)
        k = info[names[0]]
        assert k["ScratchSize"] == 0, (fragment, k)
        assert k["VGPRs"] + k.get("AGPRs", 0) <= vgprs and k["Occupancy"] >= waves, (fragment, k)
        assert not any(p in names[0] for p in PINNED_FRAGMENTS), names[0]  # the name fragments the other codegen tests select by
    # the rounds are 32-bit logic: chi as v_bfi_b32, rho as v_alignbit_b32
    body = asm[asm.index("k_kc_leaves"):]
    body = body[:body.index(".Lfunc_end")]
    assert body.count("v_bfi_b32") >= 50 and body.count("v_alignbit_b32") >= 48, (body.count("v_bfi_b32"), body.count("v_alignbit_b32"))
