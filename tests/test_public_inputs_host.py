"""Public inputs on the host (no GPU): registration, the blob's public-input section and its validation, the proof layout with
the public-input trailer, the in-circuit hash as the CPU oracle's witness computes it, and the new kernel's code generation."""
import ctypes as C
import struct

import pytest

import device_build as device
import isa_lint
import pi_circuits
import verify_layout

KS = [1, 7, 8, 9, 17]  # around the sponge rate (8); 7 and more also hold a duplicate, a constant and two computed targets


def test_num_public_inputs_and_proof_layout(pkg):
    for k in KS:
        data, _, _, _ = pi_circuits.small(pkg, k)
        assert data.num_public_inputs == k
        info = dict(data.info)
        assert info["num_public_inputs"] == k
        body = dict(info, proof_bytes=info["proof_bytes"] - (8 + 8 * k))
        verify_layout.sections(body)  # asserts that the layout without the trailer is the proof body exactly
    twin, _, _, _ = pi_circuits.small(pkg, 9, register=False)
    assert twin.num_public_inputs == 0
    verify_layout.sections(twin.info)  # no trailer


def test_zero_public_inputs_leave_the_blob_as_it_was(pkg):
    """A circuit without public inputs ends at blind_zrows (no section), and building it twice gives the same bytes."""
    a, _, _, _ = pi_circuits.small(pkg, 9, register=False)
    b, _, _, _ = pi_circuits.small(pkg, 9, register=False)
    assert a.blob == b.blob
    assert struct.pack("<I", pi_circuits.PI_TAG) not in a.blob[-64:]
    with_pi, _, _, _ = pi_circuits.small(pkg, 9)
    assert with_pi.blob != a.blob
    assert with_pi.info["degree_bits"] >= a.info["degree_bits"]


def test_blob_section_holds_the_slots_in_registration_order(pkg):
    data, _, _, pis = pi_circuits.small(pkg, 17)
    _, slots = pi_circuits.pi_section(data.blob, 17)
    assert len(slots) == 17 and max(slots) < data.info["num_slots"]
    # equal targets share a slot, different targets do not
    for i in range(17):
        for j in range(17):
            assert (slots[i] == slots[j]) == (pis[i] == pis[j]), (i, j)


@pytest.mark.parametrize("k", KS)
def test_oracle_witness_puts_the_public_input_hash_on_the_gate_row(pkg, orc, k):
    """The oracle (which reads version-4 blobs and ignores what follows blind_zrows) generates the witness of a circuit with
    public inputs; the PublicInputGate row's wires 0..3 hold hash_no_pad of the values, as both native hashes compute it."""
    data, pws, vals, pis = pi_circuits.small(pkg, k)
    oc = orc.OracleCircuit(data.blob)
    n = 1 << data.info["degree_bits"]
    row = pi_circuits.pi_gate_row(oc, n)
    for pw, want in zip(pws, vals):
        st, wires = oc.generate_witness(pw.map, data.info["num_wires"] * n)
        assert st == 0
        # computed targets are routed wires: their witness values are the ones computed on the host
        for t, v in zip(pis, want):
            if t >> 63:
                assert pi_circuits.target_value(wires, n, t) == v
        h = (C.c_uint64 * 4)()
        orc.lib().orc_hash_no_pad((C.c_uint64 * len(want))(*want), len(want), h)
        assert [wires[c * n + row] for c in range(4)] == list(h)
        assert list(h) == pkg.poseidon_native.hash_n_to_m_no_pad(want, 4)


def _info_rc(pkg, blob):
    info = pkg.api._Info()
    return pkg.lib().p2_blob_info(bytes(blob), len(blob), C.byref(info))


def test_malformed_public_input_sections_are_rejected(pkg):
    data, _, _, _ = pi_circuits.small(pkg, 9)
    blob = data.blob
    off, _ = pi_circuits.pi_section(blob, 9)
    assert _info_rc(pkg, blob) == 0
    L = pkg.lib()
    cases = {
        "truncated": blob[:-1],
        "truncated inside the count": blob[: off + 6],
        "tag only": blob[: off + 4],
        "slot out of range": blob[:-4] + struct.pack("<I", data.info["num_slots"]),
        "slot 2^32-1": blob[:-4] + b"\xff\xff\xff\xff",
        "bytes after the section": blob + b"\0",
        "wrong tag": blob[:off] + struct.pack("<I", pi_circuits.PI_TAG ^ 1) + blob[off + 4:],
        "count zero": blob[: off + 4] + struct.pack("<Q", 0),
        "count larger than the bytes": blob[: off + 4] + struct.pack("<Q", 1 << 40) + blob[off + 12:],
    }
    for name, bad in cases.items():
        assert _info_rc(pkg, bad) != 0, name
        assert L.p2_last_error(), name
    # a blob that ends at blind_zrows parses as it always did
    assert _info_rc(pkg, blob[:off]) == 0


def test_register_public_input_rejects_an_unknown_target(pkg):
    b = pkg.CircuitBuilder()
    b.add_virtual_target()
    with pytest.raises(pkg.P2Error):
        b.register_public_input(1000)


def test_public_inputs_read_from_a_proof_trailer(pkg):
    """p2_proof_public_inputs / CircuitData.public_inputs parse the trailer (u64 k || k values) after the proof body."""
    data, _, vals, _ = pi_circuits.small(pkg, 9)
    pb, k = data.proof_bytes, 9
    proof = bytearray(pb)
    struct.pack_into("<%dQ" % (k + 1), proof, pb - 8 * (k + 1), k, *vals[0])
    assert data.public_inputs(bytes(proof)) == vals[0]
    bad = bytearray(proof)
    struct.pack_into("<Q", bad, pb - 8 * (k + 1), k + 1)
    with pytest.raises(pkg.P2Error, match="wrong number of public inputs"):
        data.public_inputs(bytes(bad))
    with pytest.raises(pkg.P2Error):
        data.public_inputs(bytes(proof[:-1]))
    twin, _, _, _ = pi_circuits.small(pkg, 9, register=False)
    assert twin.public_inputs(bytes(twin.proof_bytes)) == []


def test_host_verifier_checks_the_trailer_with_the_shape(pkg):
    """On a well-shaped all-zero proof (sibling counts right), a wrong count word is a SHAPE verdict, a value >= p a
    NON_CANONICAL one, and with both right the verifier gets past the parse (and rejects the zero proof later)."""
    data, _, _, _ = pi_circuits.small(pkg, 7)
    k, pb = 7, data.proof_bytes
    secs = verify_layout.sections(dict(data.info, proof_bytes=pb - 8 * (k + 1)))
    base = bytearray(pb)
    for name, (off, nbytes, kind) in secs.items():
        if kind == "count":
            base[off] = secs[name.replace("_count", "_siblings")][1] // 32
    vd = (C.c_uint64 * 68)()
    L = pkg.lib()

    def reason(proof):
        assert L.p2_verify(data.blob, len(data.blob), vd, 68, bytes(proof), len(proof)) == 4
        return L.p2_last_error().decode()

    assert reason(base) == "wrong number of public inputs"  # count word 0
    assert pkg.VERIFY_REASONS[reason(base)] == pkg.VERIFY_SHAPE
    good = bytearray(base)
    struct.pack_into("<Q", good, pb - 8 * (k + 1), k)
    assert reason(good) not in ("wrong number of public inputs", "non-canonical field element", "proof truncated")
    bad = bytearray(good)
    struct.pack_into("<Q", bad, pb - 8, pi_circuits.P)  # last value = p
    assert reason(bad) == "non-canonical field element"


@pytest.fixture(scope="module")
def device_build():
    return device.cross_compile()


def test_pi_hash_kernel_cross_compiles_without_scratch(device_build):
    info, asm = device_build
    names = [n for n in info if "k_pi_hash" in n]
    assert names
    for fragment in ("k_pi_hash", "k_challenger", "k_quotient", "k_vfy_unpack", "k_vfy_transcript", "k_vfy_vanishing"):
        for n in (n for n in info if fragment in n):
            k = info[n]
            assert k["ScratchSize"] == 0, (n, k)
            assert k["VGPRs"] + k.get("AGPRs", 0) <= 128, (n, k)
    funcs = isa_lint.parse_functions(asm)
    pi = {name: blocks for name, blocks in funcs.items() if "k_pi_hash" in name}
    assert pi and sum(len(b[1]) for blocks in pi.values() for b in blocks) > 100
    assert isa_lint.sgpr_hazards(asm) == []


# The kernels public inputs touch, with the VGPRs each had before the feature (gfx950, this ROCm's hipcc): the PublicInputGate
# term, the transcript's hash and the trailer checks must not cost a register anywhere.
VGPRS_BEFORE = {"k_quotientILb0ELb1E": 128, "k_quotientILb1ELb0E": 121, "k_challenger": 93, "k_vfy_unpack": 8, "k_vfy_transcript": 96,
                "k_vfy_vanishing": 76, "k_vfy_queries": 92, "k_vfy_finish": 6, "k_finish": 4, "k_proof_segments": 8}


def test_touched_kernels_keep_their_register_counts(device_build):
    info, _ = device_build
    for fragment, vgprs in VGPRS_BEFORE.items():
        names = [n for n in info if fragment in n]
        assert len(names) == 1, (fragment, names)
        k = info[names[0]]
        assert k["VGPRs"] + k.get("AGPRs", 0) == vgprs and k["ScratchSize"] == 0, (fragment, k)


def test_register_public_input_rejects_wires_that_do_not_exist(pkg):
    """Wire targets are (row, column): the row must be a gate the builder already has, the column a routed wire."""
    b = pkg.CircuitBuilder()
    x, y = b.add_virtual_target(), b.add_virtual_target()
    xy = b.mul(x, y)  # a routed wire of ArithmeticGate row 0
    assert xy >> 63
    b.register_public_input(xy)
    row, col = (xy & ~(1 << 63)) >> 8, xy & 0xFF
    for bad in ((row + 5, col), (row, 80), (row, 134)):
        with pytest.raises(pkg.P2Error, match="register_public_input"):
            b.register_public_input((1 << 63) | (bad[0] << 8) | bad[1])
    assert b.build().num_public_inputs == 1


def test_blob_form_of_the_trailer_parser(pkg):
    """p2_proof_public_inputs (blob + proof, for callers without a handle) reads what CircuitData.public_inputs reads."""
    data, _, vals, _ = pi_circuits.small(pkg, 8)
    pb, k = data.proof_bytes, 8
    proof = bytearray(pb)
    struct.pack_into("<%dQ" % (k + 1), proof, pb - 8 * (k + 1), k, *vals[1])
    out, n = (C.c_uint64 * k)(), C.c_size_t()
    L = pkg.lib()
    assert L.p2_proof_public_inputs(data.blob, len(data.blob), bytes(proof), pb, out, k, C.byref(n)) == 0
    assert n.value == k and list(out) == vals[1] == data.public_inputs(bytes(proof))
    assert L.p2_proof_public_inputs(data.blob, len(data.blob), bytes(proof), pb, out, k - 1, C.byref(n)) != 0  # cap < k
    assert L.p2_proof_public_inputs(data.blob, len(data.blob), bytes(proof), pb - 1, out, k, C.byref(n)) != 0
    assert L.p2_circuit_public_inputs(None, bytes(proof), pb, out, k, C.byref(n)) != 0
