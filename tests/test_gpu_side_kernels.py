"""GPU tests (pytest -m gpu) of the polynomial-side kernels that run on lazy sums and power tables: k_perm_chunks, k_zeta_tabs /
k_zeta_pows, k_eval_polys_refs, k_fri_alpha_pows / k_fri_compose, and the one-walk instantiation of k_quotient.

Three layers: whole proofs in batches of three against the CPU oracle byte for byte, on circuits small enough to take seconds
and shaped to reach every path of these kernels; the opening-point power tables alone (p2_gpu_zeta_pows) against powers computed
in Python; and the device self-test of the lazy compositions (p2_selftest_lazy_device), which draws the non-canonical
intermediates that no proof reaches by chance (probability 2^-32 per value on random data)."""
import ctypes as C
import random

import pytest

import circuits
from edge_circuits import chain_ops as _chain, chain_value as _chain_value

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001
POW2_GEN = 7277203076849721926  # of order 2^32


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.fail("-m gpu tests need a GPU: the HIP path has no CPU fallback")
    return pkg


# ---------------------------------------------------------------------------------------------- whole proofs
def _padded(pkg, luts, n_ops, seeds):
    """`luts` small lookup tables (0: none, 1: the S-box, 2: S-box and the one-bit right shift) next to an arithmetic chain that
    sets the number of rows; the chain's end value is asserted in the witness."""
    b = pkg.CircuitBuilder()
    x, y = b.add_virtual_target(), b.add_virtual_target()
    out = _chain(b, x, y, n_ops)
    byte = shifted = None
    if luts >= 1:
        byte = b.add_virtual_byte_target(b.sbox_lut())
    if luts >= 2:
        xs = [b.add_virtual_byte_target_unsafe() for _ in range(16)]
        shifted = (xs, b.right_shift_one(b.u8_unit_right_shift_lut(), xs))
    data = b.build()
    pws = []
    for seed in seeds:
        r = random.Random(seed)
        xv, yv = r.randrange(P), r.randrange(P)
        pw = pkg.PartialWitness()
        pw.set_target(x, xv)
        pw.set_target(y, yv)
        pw.set_target(out, _chain_value(xv, yv, n_ops))
        if byte is not None:
            pw.set_target(byte, r.randrange(256))
        if shifted is not None:
            vals = [r.randrange(256) for _ in range(16)]
            exp, carry = [], 0
            for v in vals:
                exp.append((v >> 1) | (carry << 7))
                carry = v & 1
            for t, v in zip(shifted[0], vals):
                pw.set_byte_target(t, v)
            for t, v in zip(shifted[1], exp):
                pw.set_byte_target(t, v)
        pws.append(pw)
    return data, pws


def _batch_of_three_matches_the_oracle(orc, data, pws):
    """Three different witnesses in one batch (the batch strides of every buffer show), each proof equal to the oracle's."""
    assert len(pws) == 3
    oc = orc.OracleCircuit(data.blob)
    assert data.verifier_data() == oc.verifier_data()
    proofs, status = data.prove_batch(pws)
    assert status == [0, 0, 0]
    assert len({bytes(p) for p in proofs}) == 3  # three different proofs: a stride of zero could not pass
    for pw, proof in zip(pws, proofs):
        ost, ref = oc.prove(pw.map)
        assert ost == 0 and proof == ref
        data.verify(proof)


def test_routed_only_circuit_of_64_rows(gpu, orc):
    """No lookup table, n = 2^6 < 256: one entry in the high power table, the evaluation kernel's tail loop only, one chunk of
    rows in every kernel that walks 256 rows per workgroup."""
    data, pws = _padded(gpu, 0, 90, [1, 2, 3])
    assert data.info["degree_bits"] == 6 and data.info["num_luts"] == 0
    _batch_of_three_matches_the_oracle(orc, data, pws)


def test_one_lookup_table_1024_rows(gpu, orc):
    """One table, n = 2^10 = 4 x 256: the four-row trip of the evaluation kernel runs (once, with an empty tail), four entries in
    the high power table, both lookup views in the quotient."""
    data, pws = _padded(gpu, 1, 1400, [4, 5, 6])
    assert data.info["degree_bits"] == 10 and data.info["num_luts"] == 1
    _batch_of_three_matches_the_oracle(orc, data, pws)


def test_two_lookup_tables_256_rows(gpu, orc):
    """Two tables, n = 2^8: exactly one workgroup of rows, tail loop only, the last partial lookup polynomials shorter than the
    others (26 = 3 * 7 + 5 table slots, 40 = 5 * 7 + 5 looking slots)."""
    data, pws = _padded(gpu, 2, 380, [7, 8, 9])
    assert data.info["degree_bits"] == 8 and data.info["num_luts"] == 2
    _batch_of_three_matches_the_oracle(orc, data, pws)


def test_poseidon_gate_circuit(gpu, orc):
    """PoseidonGate rows: 135 live wire columns, the two-walk quotient (untouched) next to the new permutation, opening and FRI
    kernels."""
    data, pws, _, _ = circuits.poseidon_encrypt(gpu, 3, [21, 22, 23])
    _batch_of_three_matches_the_oracle(orc, data, pws)


def test_smallest_aes_gcm_circuit(gpu, orc):
    """AES-GCM-128 at the smallest plaintext length the builder accepts: the flagship circuit's shape (three tables, one-walk
    quotient, 2^13 rows)."""
    r = random.Random(31)
    keys = [(bytes(r.randrange(256) for _ in range(16)), bytes(r.randrange(256) for _ in range(12)), b"") for _ in range(3)]
    data, pws, _ = circuits.encrypt(gpu, 4, 0, False, keys=keys)
    _batch_of_three_matches_the_oracle(orc, data, pws)


# ---------------------------------------------------------------------------------------------- power tables
def _e2_mul(x, y):
    return ((x[0] * y[0] + 7 * x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)


def _e2_pow(x, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = _e2_mul(r, x)
        x = _e2_mul(x, x)
        e >>= 1
    return r


def _e2_inv(x):
    return _e2_pow(x, P * P - 2)


@pytest.fixture(scope="module")
def random_z():
    r = random.Random(0x2E7A)
    return (r.randrange(P), r.randrange(P))


@pytest.mark.parametrize("bits", [0, 1, 7, 8, 9, 14])
@pytest.mark.parametrize("which", ["one", "x", "minus_one_both", "random"])
def test_zeta_power_tables(gpu, random_z, which, bits):
    """z^i for i < n at the four opening points (z, g z and their inverses) against powers computed in Python: n below, at and
    above the 256 entries of the low table (one high entry; exactly one; two; 64), i = 0, and bases whose powers are 1, have a
    zero component, or sit at the top of the field."""
    z = {"one": (1, 0), "x": (0, 1), "minus_one_both": (P - 1, P - 1), "random": random_z}[which]
    n = 1 << bits
    g = pow(POW2_GEN, (1 << 32) >> bits, P)
    out = (C.c_uint64 * (8 * n))()
    assert gpu.lib().p2_gpu_zeta_pows((C.c_uint64 * 2)(*z), n, out, 0) == 0, gpu.lib().p2_last_error()
    got = list(out)
    gz = _e2_mul(z, (g, 0))
    for k, base in enumerate([z, gz, _e2_inv(z), _e2_inv(gz)]):
        assert _e2_mul(base, [z, gz, _e2_inv(z), _e2_inv(gz)][k ^ 2]) == (1, 0)
        want, cur = [], (1, 0)
        for _ in range(n):
            want.append(cur)
            cur = _e2_mul(cur, base)
        for i in {0, n - 1, n // 2, min(n - 1, 255), min(n - 1, 256), min(n - 1, 257)}:
            assert want[i] == _e2_pow(base, i)  # the running product is the power
        assert got[2 * k * n:(2 * k + 1) * n] == [w[0] for w in want], (k, "c0")
        assert got[(2 * k + 1) * n:(2 * k + 2) * n] == [w[1] for w in want], (k, "c1")


def test_zeta_power_tables_reject_bad_arguments(gpu):
    out = (C.c_uint64 * 64)()
    assert gpu.lib().p2_gpu_zeta_pows((C.c_uint64 * 2)(1, 0), 0, out, 0) != 0
    assert gpu.lib().p2_gpu_zeta_pows((C.c_uint64 * 2)(1, 0), 3, out, 0) != 0
    assert gpu.lib().p2_gpu_zeta_pows((C.c_uint64 * 2)(P, 0), 4, out, 0) != 0


# ---------------------------------------------------------------------------------------------- lazy compositions
def test_device_selftest_of_the_lazy_compositions(gpu):
    """2^20 threads x 16 draws: the permutation term and product step, the table-slot and looking-slot steps of the one-walk
    quotient with their closing terms, the exact dot product with a uniform factor, the table-power multiply, and sub / add
    under their operand contracts, each against the textbook canonical evaluation, on operands from {0, 1, 2^32 - 1, 2^32, p - 1, p, p + 1, 2^64 - 1, zero limbs, random} that stay non-canonical wherever the contract
    allows; the planted violations (a non-canonical subtrahend, two non-canonical summands) must show, or they count."""
    assert gpu.lib().p2_selftest_lazy_device(0x1A27, 1 << 20, 0) == 0
