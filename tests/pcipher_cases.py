"""Shared inputs of the Poseidon-cipher tests: keys, nonces and messages from a fixed seed, the directed decryption items with
the status each must get, and the sealed-message circuit.  Nothing here calls the library under test except the circuit builder,
which takes it as `pkg`.  A cipher key is used as its ten words, so the undirected keys are random words, not curve points."""
import random

import pcipher_ref as ref

P = ref.P
M64 = (1 << 64) - 1
SEED = 0x9C19


def fq(r):
    return tuple(r.randrange(P) for _ in range(5))


def item(r, l):
    """(ks, nonce, msg): a key of two random Fq elements, a nonce of two words, l random elements"""
    return (fq(r), fq(r)), (r.randrange(P), r.randrange(P)), [fq(r) for _ in range(l)]


def items(count, l, seed=SEED):
    r = random.Random(seed * 4099 + l)
    return [item(r, l) for _ in range(count)]


def flat(elems):
    return [w for e in elems for w in e]


def with_word(elems, i, j, value):
    out = [tuple(e) for e in elems]
    out[i] = out[i][:j] + (value,) + out[i][j + 1:]
    return out


def directed_decrypt(l):
    """[(label, ks, nonce, ct, status, message or None)] for one call with length l in 4, 5, 6, 1, 2: only the rows that make
    sense at that length.  Every expectation is asserted on the reference first."""
    r = random.Random(SEED + 77 + l)
    ks, nonce, msg = item(r, l)
    good = ref.encrypt(ks, msg, nonce)
    out = [("good", ks, nonce, good, 0, msg)]
    for j in range(5):
        out.append(("tag word %d off by one" % j, ks, nonce, with_word(good, len(good) - 1, j, (good[-1][j] + 1) % P), 1, None))
    if l % 3:
        padded = msg + [ref.ZERO] * (ref.pad3(l) - l)
        dirty = ref.encrypt_padded(ks, with_word(padded, len(padded) - 1, 3, 1), nonce, l)
        # the reference's rule: padding is looked at only when l > 3
        out.append(("non-zero last padding element", ks, nonce, dirty, 1 if l > 3 else 0, None if l > 3 else msg))
        if l % 3 == 1:
            dirty = ref.encrypt_padded(ks, with_word(padded, len(padded) - 2, 0, P - 1), nonce, l)
            out.append(("non-zero first padding element", ks, nonce, dirty, 1 if l > 3 else 0, None if l > 3 else msg))
    if l in (5, 6):
        ks4, nonce4, msg4 = item(r, 4)
        out.append(("a ciphertext of l = 4 opened as l = %d" % l, ks4, nonce4, ref.encrypt(ks4, msg4, nonce4), 1, None))
    bad_ks = (with_word(list(ks), 0, 2, P)[0], ks[1])
    out.append(("ks word = p", bad_ks, nonce, good, 2, None))
    out.append(("ks word = 2^64 - 1", (ks[0], with_word(list(ks), 1, 4, M64)[1]), nonce, good, 2, None))
    out.append(("nonce word = p", ks, (nonce[0], P), good, 2, None))
    out.append(("nonce word = 2^64 - 1", ks, (M64, nonce[1]), good, 2, None))
    out.append(("ct word = p", ks, nonce, with_word(good, 0, 0, P), 2, None))
    out.append(("ct word = 2^64 - 1", ks, nonce, with_word(good, len(good) - 2, 4, M64), 2, None))
    out.append(("tag word = p", ks, nonce, with_word(good, len(good) - 1, 1, P), 2, None))
    out.append(("good again", ks, nonce, good, 0, msg))
    for label, k, n, ct, st, m in out:
        if st != 2:
            assert ref.decrypt(k, ct, n, l) == m, label
        assert (m is None) == (st != 0)
    return out


class SealedCircuit:
    """"this ciphertext decrypts, under the secret key of this public key, to that message": public_key(sk) tied to pk,
    ks = multiply_point(sk, R), m = poseidon_decrypt(ks, nonce, ct); pk, R, nonce and ct are public inputs."""

    def __init__(self, pkg, ec_gate, L=3):
        b = pkg.CircuitBuilder(ec_gate=ec_gate)
        self.L = L
        self.sk = b.add_secret_key()
        self.pk, self.R = b.add_virtual_point_target(), b.add_virtual_point_target()
        self.nonce, self.ct = b.add_virtual_target_arr(2), b.add_virtual_target_arr(5 * (L + 1))
        b.register_public_inputs(self.pk + self.R + self.nonce + self.ct)
        self.derived_pk = b.public_key(self.sk)
        for x, y in zip(self.derived_pk, self.pk):
            b.connect(x, y)
        self.ks = b.multiply_point(self.sk, self.R)
        self.out = b.poseidon_decrypt(self.ks, self.nonce, self.ct)
        self.gates = b.num_gates()
        self.pkg, self.data = pkg, b.build()

    def witness(self, sk, pk, R, nonce, ct):
        pw = self.pkg.PartialWitness()
        pw.set_biguint320_target(self.sk, sk)
        pw.set_point_target(self.pk, pk)
        pw.set_point_target(self.R, R)
        pw.set_target_arr(self.nonce, list(nonce))
        pw.set_target_arr(self.ct, flat(ct))
        return pw.map
