"""The Schnorr gadget on the host: verify_schnorr_signature through p2_host_witness with ec_gate on and off -- an honest
signature gives a witness, each tampering a failed one whose fault names a target -- R' against tests/schnorr_ref.py, and the
circuit's size.  No device, and no proof here: the CPU oracle does not know the bit hints of split_le (witness op LIMB), so proofs of
this circuit are made on the GPU and pinned by the replay of tests/proof_ref.py (tests/test_gpu_schnorr.py)."""
import pytest

import schnorr_cases as sc
import schnorr_ref as ref

ec, P, N = ref.ec, ref.P, ref.N
MSG_LEN = 5


@pytest.fixture(scope="module", params=(True, False), ids=("ec_gate", "arithmetic"))
def circuit(pkg, request):
    return sc.SignatureCircuit(pkg, MSG_LEN, request.param)


def test_an_honest_signature_gives_a_witness_and_the_references_r(pkg, circuit):
    m = sc.message(MSG_LEN)
    pk = ref.g_mul_gen(sc.RAND_SK)
    for k in (sc.RAND_K, 0):
        vals, st, f = pkg.host_witness(circuit.data.blob, circuit.witness(pk, m, ref.sign(sc.RAND_SK, m, k)), circuit.r)
        assert st == 0 and f.kind == "NONE", f
        assert vals == ec.as_fields(ref.g_mul_gen(k))


def test_each_tampering_gives_a_failed_witness_that_names_a_target(pkg, circuit):
    m = sc.message(MSG_LEN)
    pk, other = ref.g_mul_gen(sc.RAND_SK), ref.g_mul_gen(2)
    cases = {c[0]: c for c in sc.tampered(pk, m, ref.sign(sc.RAND_SK, m, sc.RAND_K), other)}
    for label in ("s bit", "other key", "e word 0 bit", "e word 1 bit", "e word 2 bit", "e word 3 bit", "msg word bit", "s = n", "pk off the curve"):
        _, pk_c, m_c, sig_c, _ = cases[label]
        _, st, f = pkg.host_witness(circuit.data.blob, circuit.witness(pk_c, m_c, sig_c))
        assert st == 1 and f.kind == "GENERATOR_CONFLICT" and f.target is not None, (label, f)
        print("%s: %s" % (label, f))
    # a bit of s that is not a bit, and a missing challenge word
    w = circuit.witness(pk, m, ref.sign(sc.RAND_SK, m, sc.RAND_K))
    bad = dict(w)
    bad[circuit.sig[0][7]] = 2
    assert pkg.host_witness(circuit.data.blob, bad)[1] == 1
    del w[circuit.sig[1][2]]
    _, st, f = pkg.host_witness(circuit.data.blob, w)
    assert st == 2 and f.kind == "NOT_SET" and f.target == circuit.sig[1][2], f


def test_what_the_gadget_leaves_to_the_native_verifier(pkg, circuit):
    """s + n names the same R': the circuit takes it, p2_schnorr_verify calls it malformed"""
    m = sc.message(MSG_LEN)
    pk = ref.g_mul_gen(sc.RAND_SK)
    s, e = ref.sign(sc.RAND_SK, m, sc.RAND_K)
    assert pkg.host_witness(circuit.data.blob, circuit.witness(pk, m, (s + N, e)))[1] == 0
    assert pkg.schnorr.verify(pk, m, (s + N, e)) == 2


def test_gadget_rows(pkg):
    """The table of DESIGN.md section 9g.  With the gate: 640 EcStepGate rows, 3 Poseidon rows (25 words) and the arithmetic
    rows of two affine conversions, one point addition, the curve check of pk, 320 + 256 booleanity checks and four 64-bit
    sums: above 2^9 = 512 by the step rows alone, below 2^10."""
    rows = {}
    for ec_gate in (True, False):
        c = sc.SignatureCircuit(pkg, MSG_LEN, ec_gate)
        info = c.data.info
        rows[ec_gate] = (c.gates - c.gates_before, info["degree_bits"])
        print("verify_schnorr_signature, msg_len %d, ec_gate=%s: %d gates from the gadget, %d in all, degree_bits %d, %d ops, %d levels"
              % (MSG_LEN, ec_gate, c.gates - c.gates_before, c.gates, info["degree_bits"], info["num_ops"], info["num_levels"]))
    assert rows[True][1] == 10 and 640 < rows[True][0] < 1024
    assert rows[False][1] == ROWS_BITS_WITHOUT_THE_GATE


# without the gate s G is 320 mixed additions of constant multiples and e (-pk) 320 doublings and mixed additions in arithmetic
# gates: 13282 rows in all, as the build gives them
ROWS_BITS_WITHOUT_THE_GATE = 14


def test_constant_and_public_keys(pkg):
    """pk as a constant point and as public inputs: the same statement"""
    m = sc.message(3)
    pk = ref.g_mul_gen(sc.RAND_SK)
    sig = ref.sign(sc.RAND_SK, m, sc.RAND_K)
    b = pkg.CircuitBuilder(ec_gate=True)
    msg_t, sig_t = b.add_virtual_target_arr(3), b.add_virtual_schnorr_signature_target()
    b.verify_schnorr_signature(b.constant_point(pk), msg_t, sig_t)
    data = b.build()
    pw = pkg.PartialWitness()
    pw.set_target_arr(msg_t, m)
    pw.set_schnorr_signature_target(sig_t, sig)
    assert pkg.host_witness(data.blob, pw)[1] == 0
    pw.map[msg_t[0]] ^= 1
    assert pkg.host_witness(data.blob, pw)[1] == 1
    c = sc.SignatureCircuit(pkg, 3, True, public=True)
    assert c.data.num_public_inputs == 13 and pkg.host_witness(c.data.blob, c.witness(pk, m, sig))[1] == 0
    with pytest.raises(pkg.P2Error):
        b.verify_schnorr_signature(c.pk[:9], msg_t, sig_t)
