"""Shared inputs of the Schnorr tests: directed scalars, keys and nonces, messages over the sponge-block boundaries, every
tampering class with the status it must get, and the signature circuit.  Signatures come from tests/schnorr_ref.py (the oracle's
curve and hash); expected statuses come by construction -- the reference signs, the case tampers."""
import random

import schnorr_ref as ref

ec = ref.ec
P, N = ref.P, ref.N
M64, M320 = (1 << 64) - 1, (1 << 320) - 1
# the sponge input is 20 + msg_len words and crosses a rate block at 24 and 32
MSG_LENS = (0, 1, 3, 4, 5, 11, 12, 13)

_r = random.Random(0x5c4)
RAND_SK, RAND_K = _r.randrange(1, N), _r.randrange(1, N)
RAND_SCALARS = [_r.getrandbits(320) for _ in range(3)]
# operands of (a b + c) mod n
DIRECTED = [0, 1, 2, N - 1, N, N + 1, M320, (1 << 256) - 1, M64, M64 << 64, M64 << 256, sum(M64 << (128 * i) for i in range(3))] + RAND_SCALARS


def muladd_triples():
    """every directed operand in every position against a few partners, and the random triples"""
    out = []
    for x in DIRECTED:
        out += [(x, M320, N - 1), (N - 1, x, M320), (M320, N + 1, x), (x, x, x)]
    out.append(tuple(RAND_SCALARS))
    return out


def message(n, seed=0):
    r = random.Random(1000 * seed + n)
    return [r.randrange(P) for _ in range(n)]


def flip(w):
    """w with one bit flipped, still below p"""
    return next(w ^ (1 << b) for b in range(64) if (w ^ (1 << b)) < P)


def point_outside_the_group():
    """On the curve, x a square: the other root of the generator's x^2 + (a - 1/u^2) x + b = 0 (the roots multiply to b)"""
    x, u = ec.generator()
    other = (ec.f_mul(ec.B, ec.f_inv(x)), u)
    assert ec.f_mul(ec.f_mul(u, u), ec.f_add(ec.f_add(ec.f_mul(other[0], other[0]), ec.f_mul(ec.A, other[0])), ec.B)) == other[0] and not ec.in_group(other)
    return other


def with_word(pt, coord, i, w):
    c = list(pt[coord])
    c[i] = w
    return (tuple(c), pt[1]) if coord == 0 else (pt[0], tuple(c))


def tampered(pk, msg, sig, other_pk):
    """[(label, pk, msg, sig, status)] around one honest signature (first, status 0)"""
    s, e = sig
    out = [("honest", pk, msg, sig, 0), ("s bit", pk, msg, (s ^ 1 if (s ^ 1) < N else s ^ 2, e), 1), ("other key", other_pk, msg, sig, 1)]
    for i in range(4):
        out.append(("e word %d bit" % i, pk, msg, (s, e[:i] + (flip(e[i]),) + e[i + 1:]), 1))
    out += [("s = n", pk, msg, (N, e), 2), ("s + n", pk, msg, (s + N, e), 2), ("s = 2^320 - 1", pk, msg, (M320, e), 2)]
    for i, w in ((0, P), (3, M64)):
        out.append(("e word %d not canonical" % i, pk, msg, (s, e[:i] + (w,) + e[i + 1:]), 2))
    if msg:
        j = len(msg) - 1
        out.append(("msg word bit", pk, msg[:j] + [flip(msg[j])], sig, 1))
        out.append(("msg word not canonical", pk, [P] + msg[1:], sig, 2))
        out.append(("last msg word not canonical", pk, msg[:j] + [M64], sig, 2))
    out += [("pk.x word not canonical", with_word(pk, 0, 4, M64), msg, sig, 2), ("pk.u word not canonical", with_word(pk, 1, 0, P), msg, sig, 2),
            ("pk off the curve", with_word(pk, 0, 0, (pk[0][0] + 1) % P), msg, sig, 2), ("pk outside the group", point_outside_the_group(), msg, sig, 2),
            ("pk neutral", ec.NEUTRAL, msg, sig, 2)]
    return out


def k0_signature(sk, msg):
    """the k = 0 signature: s = e sk with e = H((0,0) | pk | msg); no signer emits it, the verifier accepts it"""
    return ref.sign(sk, msg, 0)


class SignatureCircuit:
    """pk and a message of msg_len words (public inputs when `public`), a private signature, verify_schnorr_signature"""

    def __init__(self, pkg, msg_len, ec_gate, public=False):
        b = pkg.CircuitBuilder(ec_gate=ec_gate)
        self.pk, self.msg = b.add_virtual_point_target(), b.add_virtual_target_arr(msg_len)
        if public:
            b.register_public_inputs(self.pk + self.msg)
        self.sig = b.add_virtual_schnorr_signature_target()
        self.gates_before = b.num_gates()
        self.r = b.verify_schnorr_signature(self.pk, self.msg, self.sig)
        self.gates = b.num_gates()
        self.pkg, self.data = pkg, b.build()

    def witness(self, pk, msg, sig):
        pw = self.pkg.PartialWitness()
        pw.set_point_target(self.pk, pk)
        pw.set_target_arr(self.msg, msg)
        pw.set_schnorr_signature_target(self.sig, sig)
        return pw.map
