"""EcStepGate on the host: the shared constraint evaluator (base field and GF(p^2)) against a Python restatement tied to the
affine group law of oracle/oracle_ecgfp5.py, the host twin of the ECSTEP witness op against ec.g_mul, the sizes of the three
ecgfp5 circuits with the gate, and the resources of the new kernels.  Everything compared is a field element or a status."""
import ctypes as C
import random

import pytest

import device_build as device
import ec_circuits as K
from ec_circuits import ec

P = K.P
N = ec.GROUP_ORDER


def _wire_row(t):
    return (t & ~(1 << 63)) >> 8


# ------------------------------------------------------------------------------------------ the restatement itself
def test_restated_formulas_are_the_group_law():
    r = random.Random(31)
    G = ec.generator()
    cases = [(K.random_point(r), K.random_point(r)) for _ in range(4)]
    cases += [(ec.NEUTRAL, G), (G, ec.NEUTRAL), (G, G), (G, ec.g_neg(G)), (ec.NEUTRAL, ec.NEUTRAL)]
    for p, q in cases:
        acc = K.projective(p, r) if p != ec.NEUTRAL else K.NEUTRAL_PROJ
        for bit in (0, 1):
            w = K.row(acc, q, bit)
            assert K.constraints(w) == [0] * 40
            out = tuple(tuple(w[K.OUT + 5 * j + i] for i in range(5)) for j in range(4))
            want = ec.g_add(ec.g_add(p, p), q if bit else ec.NEUTRAL)
            assert K.affine(out) == want, (p, q, bit)


# ------------------------------------------------------------------------------------------ 1. the evaluator
def _host_base(pkg, rows):
    n = len(rows)
    buf = (C.c_uint64 * (80 * n))(*[v for w in rows for v in w])
    out = (C.c_uint64 * (40 * n))()
    assert pkg.lib().p2_host_ecstep_constraints(buf, n, out) == 0, pkg.lib().p2_last_error()
    return [list(out[40 * i:40 * i + 40]) for i in range(n)]


def _ext_reference(a, b):
    """The 40 constraints at the wires a + b X of GF(p)[X]/(X^2 - 7), from the base-field restatement alone: every constraint
    is a polynomial of degree <= 6 in the wires, so c(a + b t) is one of degree <= 6 in t -- interpolated through t = 0..6 and
    reduced with t^2 = 7."""
    ys = [K.constraints([(x + t * y) % P for x, y in zip(a, b)]) for t in range(7)]
    res = []
    for k in range(40):
        coef = [0] * 7
        for j in range(7):
            num, den = [1], 1   # prod_{m != j} (t - m) / (j - m)
            for m in range(7):
                if m == j:
                    continue
                num = [(-m * num[0]) % P] + [(num[i - 1] - m * num[i]) % P for i in range(1, len(num))] + [num[-1]]
                den = den * (j - m) % P
            s = ys[j][k] * pow(den, P - 2, P) % P
            for i in range(7):
                coef[i] = (coef[i] + s * num[i]) % P
        res.append(((coef[0] + 7 * coef[2] + 49 * coef[4] + 343 * coef[6]) % P, (coef[1] + 7 * coef[3] + 49 * coef[5]) % P))
    return res


def test_constraint_evaluator_base_field(pkg):
    rows = K.vectors()
    got = _host_base(pkg, rows)
    for i, w in enumerate(rows):
        assert got[i] == K.constraints(w), i
    assert got[0] == got[1] == got[2] == [0] * 40          # satisfying rows, bit 0, 1 and 2
    for i in range(3, 11):
        assert any(got[i]), i                                 # random rows and the rows with one wire moved
    assert got[12] == [0] * 40                               # all wires 0: X = Z = U = T = 0 everywhere
    bad = (C.c_uint64 * 80)(*([P] + [0] * 79))
    assert pkg.lib().p2_host_ecstep_constraints(bad, 1, (C.c_uint64 * 40)()) != 0


def test_constraint_evaluator_extension_field(pkg):
    r = random.Random(8)
    rows = K.vectors()
    imag = [[0] * 80, [r.randrange(P) for _ in range(80)]]
    for i, a in enumerate(rows):
        for b in imag:
            buf = (C.c_uint64 * 160)(*[v for pair in zip(a, b) for v in pair])
            out = (C.c_uint64 * 80)()
            assert pkg.lib().p2_host_ecstep_constraints_ext(buf, 1, out) == 0, pkg.lib().p2_last_error()
            got = [(out[2 * k], out[2 * k + 1]) for k in range(40)]
            if not any(b):
                assert got == [(c, 0) for c in K.constraints(a)], i
            else:
                assert got == _ext_reference(a, b), i


# ------------------------------------------------------------------------------------------ 2. the host twin
@pytest.fixture(scope="module")
def three_steps(pkg):
    return K.steps_circuit(pkg, 3)


def test_three_step_circuit_against_the_oracle(pkg, three_steps):
    data, bits, base, rows = three_steps
    r = random.Random(4)
    outs = [t for mid, out in rows for t in mid + out]
    for q in (K.random_point(r), ec.generator(), ec.NEUTRAL):
        for k in range(8):
            bv = [(k >> 2) & 1, (k >> 1) & 1, k & 1]
            pw = pkg.PartialWitness()
            pw.set_target_arr(bits, bv)
            pw.set_point_target(base, q)
            vals, st, fault = pkg.host_witness(data.blob, pw, outs)
            assert st == 0 and fault.kind == "NONE"
            want = [v for mid, out in K.chain(bv, q) for v in K.flat(mid) + K.flat(out)]
            assert vals == want                                  # the projective values of pdbl / padd_mixed
            final = tuple(tuple(vals[-20 + 5 * j + i] for i in range(5)) for j in range(4))
            assert K.affine(final) == ec.g_mul(k, q)


def test_conflict_and_missing_operand(pkg, three_steps):
    data, bits, base, rows = three_steps
    q = K.random_point(random.Random(6))
    honest = K.chain([1, 0, 1], q)
    pw = pkg.PartialWitness()
    pw.set_target_arr(bits, [1, 0, 1])
    pw.set_point_target(base, q)
    wrong_t = rows[1][1][7]                      # an `out` coefficient of the second row
    pw.set_target(wrong_t, (K.flat(honest[1][1])[7] + 1) % P)
    _, st, fault = pkg.host_witness(data.blob, pw, [])
    assert st == 1 and fault.kind == "GENERATOR_CONFLICT" and fault.op_kind == "ECSTEP"
    assert fault.gate_row == _wire_row(wrong_t) and fault.computed == K.flat(honest[1][1])[7] and fault.found == (fault.computed + 1) % P
    # the same value is no conflict
    pw = pkg.PartialWitness()
    pw.set_target_arr(bits, [1, 0, 1])
    pw.set_point_target(base, q)
    pw.set_target(wrong_t, K.flat(honest[1][1])[7])
    assert pkg.host_witness(data.blob, pw, [])[1] == 0
    # a missing Q coefficient: no row runs
    pw = pkg.PartialWitness()
    pw.set_target_arr(bits, [1, 0, 1])
    pw.set_target_arr(base[:3] + base[4:], (list(q[0]) + list(q[1]))[:3] + (list(q[0]) + list(q[1]))[4:])
    vals, st, fault = pkg.host_witness(data.blob, pw, [rows[0][0][0]])
    assert st == 2 and vals == [pkg.VALUE_UNSET] and fault.kind == "NOT_SET" and fault.target == base[3]


SCALARS = [0, 1, 2, N - 1, N, 2**320 - 1]


@pytest.mark.parametrize("base_kind", ["generator_constant", "point_input", "neutral_input"])
def test_multiply_point_with_the_gate_against_the_oracle(pkg, base_kind):
    r = random.Random(12)
    G = ec.generator()
    if base_kind == "generator_constant":
        data, k_t, base_t, res_t = K.multiply_circuit(pkg, constant_base=G)
        q = G
    else:
        data, k_t, base_t, res_t = K.multiply_circuit(pkg)
        q = K.random_point(r) if base_kind == "point_input" else ec.NEUTRAL
    assert data.info["degree_bits"] == 9
    for k in SCALARS + [r.getrandbits(320), r.randrange(N)]:
        pw = pkg.PartialWitness()
        pw.set_biguint320_target(k_t, k)
        if base_t is not None:
            pw.set_point_target(base_t, q)
        vals, st, fault = pkg.host_witness(data.blob, pw, res_t)
        assert st == 0 and fault.kind == "NONE", (k, fault.kind)
        assert (tuple(vals[:5]), tuple(vals[5:])) == ec.g_mul(k, q), k


def test_op_kind_numbers_and_load_checks(pkg):
    assert pkg.OP_KINDS.index("ECSTEP") == 7
    data, bits, base, rows = K.steps_circuit(pkg, 2)
    info = data.info
    # an unhinted row has no generator: two ops fewer, and its mid / out wires are still targets a witness can set
    plain, _, _, prow = K.steps_circuit(pkg, 2, hinted=False)
    assert plain.info["num_ops"] == info["num_ops"] - 2
    pw = pkg.PartialWitness()
    pw.set_target(prow[0][0][0], 5)
    assert pkg.host_witness(plain.blob, pw, [prow[0][0][0]])[0] == [5]
    with pytest.raises(pkg.P2Error):
        pkg.CircuitBuilder().ec_step([0] * 19, [0] * 10, 0)


# ------------------------------------------------------------------------------------------ 3. sizes
PARENT_NUM_GATES = {"public_key": 6977, "elgamal": 14820, "hashed_elgamal": 14804}   # builder.num_gates() before this gate existed


def test_circuit_sizes_with_and_without_the_gate(pkg):
    def builders(ec_gate):
        b = pkg.CircuitBuilder(ec_gate=ec_gate)
        b.public_key(b.add_secret_key())
        yield "public_key", b
        b = pkg.CircuitBuilder(ec_gate=ec_gate)
        b.elgamal_encrypt(b.add_virtual_point_target(), b.add_virtual_biguint320_target(), b.add_virtual_point_target())
        yield "elgamal", b
        b = pkg.CircuitBuilder(ec_gate=ec_gate)
        b.hashed_elgamal_encrypt(b.add_virtual_point_target(), b.add_virtual_biguint320_target(), b.add_virtual_target_arr(5))
        yield "hashed_elgamal", b

    for name, b in builders(False):
        assert b.num_gates() == PARENT_NUM_GATES[name], name
    bound = {"public_key": 10, "elgamal": 11, "hashed_elgamal": 11}
    for name, b in builders(True):
        gates = b.num_gates()
        info = b.build().info
        print("%s with the gate: %d gates before build, degree_bits %d, %d ops, %d levels" % (name, gates, info["degree_bits"], info["num_ops"], info["num_levels"]))
        assert info["degree_bits"] <= bound[name], name


# ------------------------------------------------------------------------------------------ 4. codegen
def test_new_kernels_exist_outside_the_pinned_names_and_do_not_spill():
    remarks = device.cross_compile()[0]
    pinned = ("k_quotient", "k_vfy_vanishing", "k_witnessILb")
    for fragment in ("k_ecstep_post", "k_vfy_ecvanishing", "k_ecstep_selftest"):
        found = {n: v for n, v in remarks.items() if fragment in n}
        assert len(found) == 1, fragment
        for n, k in found.items():
            assert not any(p in n for p in pinned), n
            print("%s: VGPRs %d, AGPRs %d, ScratchSize %d, Occupancy %d" % (fragment, k["VGPRs"], k.get("AGPRs", 0), k["ScratchSize"], k["Occupancy"]))
            assert k["ScratchSize"] == 0, (n, k)
    for inst in ("ILb0ELb0E", "ILb0ELb1E", "ILb1ELb0E", "ILb1ELb1E"):
        found = {n: v for n, v in remarks.items() if "k_ecwitness" + inst in n}
        assert len(found) == 1, inst
        for n, k in found.items():
            assert "k_witnessILb" not in n
            print("k_ecwitness%s: VGPRs %d, ScratchSize %d, Occupancy %d" % (inst, k["VGPRs"], k["ScratchSize"], k["Occupancy"]))
    # witness_ecstep_op is a function of its own (__noinline__), not a kernel: the compiler prints no remark for it, its
    # registers and stack are counted in the k_ecwitness figures above; its symbol is in the assembly
    assert "witness_ecstep_op" in device.cross_compile()[1]
    for k in (v for n, v in remarks.items() if "k_witness_check" in n):
        assert k["ScratchSize"] == 0, k
