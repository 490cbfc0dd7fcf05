"""EcStepGate: a plain-Python restatement of its 40 constraint polynomials, generic over the field the wires live in (Quintic;
BASE agrees with the affine oracle's helpers, oracle/oracle_ecgfp5.py: f_mul, f_add, f_sub), the rows and vectors the tests
share, and the circuits built with the gate.

Wire layout of a row (csrc/circuit.h EG_*): acc X|Z|U|T (0..19), Q x|u (20..29), bit (30), mid (31..50), out (51..70)."""
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import oracle_ecgfp5 as ec  # noqa: E402

P = ec.P
B1 = 263
ACC, Q, BIT, MID, OUT, WIRES = 0, 20, 30, 31, 51, 71


class Quintic:
    """GF(q)[z]/(z^5 - 3) over a base field given by its add, sub and mul and the embedding of a small integer: what the gate's
    formulas need, so that they read the same over GF(p) (BASE) and over GF(p^2) (tests/vanishing_ref.py)."""

    def __init__(self, add, sub, mul, const):
        self.add, self.sub, self.mul, self.const = add, sub, mul, const

    def f_add(self, a, b):
        return tuple(self.add(x, y) for x, y in zip(a, b))

    def f_sub(self, a, b):
        return tuple(self.sub(x, y) for x, y in zip(a, b))

    def f_mul(self, a, b):
        c = [self.const(0)] * 9
        for i in range(5):
            for j in range(5):
                c[i + j] = self.add(c[i + j], self.mul(a[i], b[j]))
        three = self.const(3)
        return tuple(self.add(c[k], self.mul(three, c[k + 5])) if k + 5 < 9 else c[k] for k in range(5))

    def f_small(self, a, k):
        return tuple(self.mul(x, self.const(k)) for x in a)

    def mul_bz(self, a, k=B1):
        """a * (k z)"""
        return (self.mul(a[4], self.const(3 * k)),) + tuple(self.mul(a[i], self.const(k)) for i in range(4))


BASE = Quintic(lambda x, y: (x + y) % P, lambda x, y: (x - y) % P, lambda x, y: x * y % P, lambda k: k % P)


def mul_bz(a, k=B1):
    """a * (k z) in GF(p)[z]/(z^5 - 3)"""
    return BASE.mul_bz(a, k)


def _tail(F, t1, t2, t3, t4, t5, t6):
    t7 = F.f_add(F.mul_bz(t2), t1)
    t8 = F.f_mul(t4, t7)
    w9 = F.f_add(F.mul_bz(t5, 2 * B1), F.f_small(t7, 2))
    z = F.f_sub(t8, F.f_mul(t3, w9))
    t = F.f_sub(F.f_small(t8, 2), z)
    d = F.f_sub(F.f_mul(F.f_add(F.f_small(t3, 2), t4), F.f_add(t5, t7)), t8)
    return F.mul_bz(d), z, F.f_mul(t6, F.f_sub(F.mul_bz(t2), t1)), t


def double(p, F=BASE):
    """2 p for p = (X, Z, U, T): the unified addition of ecgfp5.h with both operands equal"""
    X, Z, U, T = p
    return _tail(F, F.f_mul(X, X), F.f_mul(Z, Z), F.f_mul(U, U), F.f_mul(T, T), F.f_small(F.f_mul(X, Z), 2), F.f_small(F.f_mul(U, T), 2))


def add_mixed(p, qx, qu, F=BASE):
    """p + (qx, qu), the second operand affine (Z2 = T2 = 1)"""
    X, Z, U, T = p
    return _tail(F, F.f_mul(X, qx), Z, F.f_mul(U, qu), T, F.f_add(F.f_mul(Z, qx), X), F.f_add(F.f_mul(T, qu), U))


def _point(w, first):
    return tuple(tuple(w[first + 5 * j + i] for i in range(5)) for j in range(4))


def constraints(w, F=BASE):
    """The 40 constraint values of one row of (at least 71) wires: 0..19 mid - 2 acc, 20..39 out - (mid + bit Q).  Over GF(p)
    unless F names another base field for the wires."""
    acc, mid, out = _point(w, ACC), _point(w, MID), _point(w, OUT)
    bit = w[BIT]
    qx = tuple(F.mul(bit, v) for v in w[Q:Q + 5])
    qu = tuple(F.mul(bit, v) for v in w[Q + 5:Q + 10])
    res = []
    for have, want in ((mid, double(acc, F)), (out, add_mixed(mid, qx, qu, F))):
        for h, x in zip(have, want):
            res.extend(F.f_sub(h, x))
    return res


def row(acc, q, bit):
    """A satisfying row of 80 wires for acc = (X, Z, U, T), q = (x, u) and any field element `bit`."""
    mid = double(acc)
    out = add_mixed(mid, tuple(bit * v % P for v in q[0]), tuple(bit * v % P for v in q[1]))
    w = [v for c in acc for v in c] + list(q[0]) + list(q[1]) + [bit] + [v for c in mid for v in c] + [v for c in out for v in c]
    return w + [0] * (80 - len(w))


def affine(p):
    """(x, u) of a projective (X, Z, U, T)"""
    return (ec.f_mul(p[0], ec.f_inv(p[1])), ec.f_mul(p[2], ec.f_inv(p[3])))


def projective(g, r):
    """some projective form of the group element g = (x, u): random non-zero scalings of both fractions"""
    lam = tuple(r.randrange(1, P) for _ in range(5))
    mu = tuple(r.randrange(1, P) for _ in range(5))
    return (ec.f_mul(g[0], lam), lam, ec.f_mul(g[1], mu), mu)


def random_point(r):
    return ec.g_mul(r.randrange(1, ec.GROUP_ORDER), ec.generator())


def vectors():
    """Rows of 80 wires for the evaluator tests: satisfying rows for bit 0, 1 and 2, random rows, a satisfying row with one
    wire moved, all wires p - 1, all wires 0."""
    r = random.Random(2024)
    rows = []
    for bit in (0, 1, 2):
        rows.append(row(projective(random_point(r), r), random_point(r), bit))
    for _ in range(3):
        rows.append([r.randrange(P) for _ in range(80)])
    for col in (3, 24, 30, 40, 70):
        w = list(rows[1])
        w[col] = (w[col] + 1) % P
        rows.append(w)
    rows.append([P - 1] * 80)
    rows.append([0] * 80)
    return rows


NEUTRAL_PROJ = (ec.ZERO, ec.ONE, ec.ZERO, ec.ONE)


def chain(bits, q):
    """The (mid, out) pairs of the rows of acc <- 2 acc + bit q from the neutral element, most significant bit first."""
    acc, steps = NEUTRAL_PROJ, []
    for b in bits:
        mid = double(acc)
        acc = add_mixed(mid, tuple(b * v % P for v in q[0]), tuple(b * v % P for v in q[1]))
        steps.append((mid, acc))
    return steps


def flat(p):
    return [v for c in p for v in c]


# ------------------------------------------------------------------------------------------ circuits
def steps_circuit(pkg, nbits, hinted=True, constant_base=None, **kw):
    """nbits EcStepGate rows from the neutral element, bits given most significant first (plain targets, not made boolean);
    the base a point input, or the constant `constant_base`.  Returns (data, bit targets, base targets or None, [(mid, out)
    targets per row])."""
    b = pkg.CircuitBuilder(**kw)
    bits = b.add_virtual_target_arr(nbits)
    if constant_base is None:
        base = b.add_virtual_target_arr(10)
        q = base
    else:
        base = None
        q = [b.constant(v) for v in list(constant_base[0]) + list(constant_base[1])]
    zero, one = b.zero(), b.one()
    acc = [zero] * 5 + [one] + [zero] * 4 + [zero] * 5 + [one] + [zero] * 4
    rows = []
    for i in range(nbits):
        mid, out = b.ec_step(acc, q, bits[i], hinted)
        rows.append((mid, out))
        acc = out
    return b.build(), bits, base, rows


def multiply_circuit(pkg, constant_base=None, **kw):
    """multiply_point with the gate switched on: 320 boolean scalar bits times a point input or a constant.
    Returns (data, scalar targets, base targets or None, result targets)."""
    b = pkg.CircuitBuilder(ec_gate=True, **kw)
    k_t = b.add_virtual_biguint320_target()
    if constant_base is None:
        base = b.add_virtual_target_arr(10)   # no membership check: the tests multiply (0, 0) too
        res = b.multiply_point(k_t, base)
    else:
        base = None
        res = b.multiply_point(k_t, b.constant_point(constant_base))
    return b.build(), k_t, base, res


def public_key(pkg, seeds, ec_gate=True, **kw):
    b = pkg.CircuitBuilder(ec_gate=ec_gate, **kw)
    sk_t = b.add_secret_key()
    pk_t = b.public_key(sk_t)
    data = b.build()
    pws, cases = [], []
    for seed in seeds:
        sk = pkg.ECGFP5SecretKey.rand(seed)
        pw = pkg.PartialWitness()
        pw.set_secret_key_target(sk_t, sk)
        pws.append(pw)
        cases.append((sk, ec.g_mul(sk.value, ec.generator())))
    return data, pws, (sk_t, pk_t), cases


def elgamal(pkg, seeds, ec_gate=True, **kw):
    """The ciphertext targets are left to the witness run: the tests read them back."""
    E = pkg.ecgfp5
    b = pkg.CircuitBuilder(ec_gate=ec_gate, **kw)
    pk_t = b.add_virtual_point_target()
    nonce_t = b.add_virtual_biguint320_target()
    msg_t = b.add_virtual_point_target()
    ct_t = b.elgamal_encrypt(pk_t, nonce_t, msg_t)
    data = b.build()
    pws, cases = [], []
    for seed in seeds:
        pk = pkg.ECGFP5SecretKey.rand(3 * seed).public_key()
        msg = E.new_rand_from_subgroup(3 * seed + 1)
        nonce = E.random_scalar(3 * seed + 2)
        pw = pkg.PartialWitness()
        pw.set_point_target(pk_t, pk)
        pw.set_point_target(msg_t, msg)
        pw.set_biguint320_target(nonce_t, nonce)
        pws.append(pw)
        cases.append((pk, msg, nonce))
    return data, pws, (pk_t, nonce_t, msg_t, ct_t), cases


def hashed_elgamal(pkg, seeds, ec_gate=True, **kw):
    E = pkg.ecgfp5
    b = pkg.CircuitBuilder(ec_gate=ec_gate, **kw)
    pk_t = b.add_virtual_point_target()
    nonce_t = b.add_virtual_biguint320_target()
    msg_t = b.add_virtual_target_arr(5)
    ct_t = b.hashed_elgamal_encrypt(pk_t, nonce_t, msg_t)
    data = b.build()
    pws, cases = [], []
    for seed in seeds:
        r = random.Random(seed)
        pk = pkg.ECGFP5SecretKey.rand(3 * seed).public_key()
        msg = tuple(r.randrange(P) for _ in range(5))
        nonce = E.random_scalar(3 * seed + 2)
        pw = pkg.PartialWitness()
        pw.set_point_target(pk_t, pk)
        pw.set_target_arr(msg_t, msg)
        pw.set_biguint320_target(nonce_t, nonce)
        pws.append(pw)
        cases.append((pk, msg, nonce))
    return data, pws, (pk_t, nonce_t, msg_t, ct_t), cases
