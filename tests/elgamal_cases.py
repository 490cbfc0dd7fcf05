"""Shared inputs of the ElGamal tests: directed scalars and points with the status they must get, encode_binary inputs whose
first decodable attempt is known by construction (tests/elgamal_ref.py classifies the pad rows), the undirected items from a fixed
seed, and the decryption circuits.  Nothing here calls the library under test except the circuit builders, which take it as
`pkg`."""
import random

import elgamal_ref as ref
import schnorr_cases as sc

ec = ref.ec
P, N = ref.P, ref.N
M32, M64, M320 = ref.M32, (1 << 64) - 1, (1 << 320) - 1
ATTEMPTS = 16
SEED = 0xE16A

_r = random.Random(SEED)
RAND_SK, RAND_K, RAND_M = _r.randrange(1, N), _r.randrange(1, N), _r.randrange(1, N)
SCALARS = (0, 1, 2, N - 1)            # n is malformed; n - 1 is the largest scalar taken


def random_pads(r, attempts=ATTEMPTS):
    return [[r.getrandbits(32) for _ in range(5)] for _ in range(attempts)]


def undirected(count, seed=SEED):
    """[(limbs, pads)]: `count` random messages with ATTEMPTS random pad rows each"""
    r = random.Random(seed)
    return [(tuple(r.getrandbits(32) for _ in range(5)), random_pads(r)) for _ in range(count)]


def classified_rows(limbs, r, want_fail, want_ok):
    """random pad rows for `limbs`, sorted by the reference into those that decode and those that do not"""
    fail, ok = [], []
    while len(fail) < want_fail or len(ok) < want_ok:
        row = [r.getrandbits(32) for _ in range(5)]
        w = ref.attempt_word(limbs, row)
        if any(v >= P for v in w):
            continue
        (ok if ref.decodes(w) else fail).append(row)
    return fail[:want_fail], ok[:want_ok]


def encode_directed():
    """[(label, limbs, pads, attempt the reference takes)]: ATTEMPTS stands for none"""
    r = random.Random(SEED + 1)
    out = []
    for label, limbs in (("limbs zero", (0,) * 5), ("limbs all ones", (M32,) * 5), ("random limbs", tuple(r.getrandbits(32) for _ in range(5)))):
        fail, ok = classified_rows(limbs, r, ATTEMPTS, 1)
        for first in (0, 7, ATTEMPTS - 1, ATTEMPTS):
            out.append(("%s, attempt %d" % (label, first), limbs, fail[:first] + ok + fail[first:ATTEMPTS - 1] if first < ATTEMPTS else fail, first))
    # a pad word of 2^32 - 1 over a non-zero limb makes a word not below p: skipped although the row's other words are those of
    # the row that decodes, which follows
    limbs = (5, 0, 7, 0, 9)
    fail, ok = classified_rows(limbs, r, ATTEMPTS, 1)
    skipped = [M32] + ok[0][1:]
    out.append(("pad word 2^32 - 1 over a non-zero limb", limbs, [skipped, fail[0]] + ok + fail[1:ATTEMPTS - 2], 2))
    # over a zero limb the same pad word gives p - 1, canonical: that attempt is tried
    limbs0 = (0, 5, 7, 0, 9)
    rows = []
    while len(rows) < 2:                                  # one row that decodes with pad 2^32 - 1 on the zero limb, one that does not
        row = [M32] + [r.getrandbits(32) for _ in range(4)]
        if ref.decodes(ref.attempt_word(limbs0, row)) == (len(rows) == 1):
            rows.append(row)
    fail0, _ = classified_rows(limbs0, r, ATTEMPTS - 2, 0)
    out.append(("pad word 2^32 - 1 over a zero limb", limbs0, rows + fail0, 1))
    for _, limbs, pads, first in out:
        assert len(pads) == ATTEMPTS and ref.first_attempt(limbs, pads) == first
    return out


def point_off_the_curve():
    g = ec.generator()
    return sc.with_word(g, 0, 0, (g[0][0] + 1) % P)


def bad_points():
    """[(label, point)]: each must get status 2"""
    g = ec.generator()
    return [("word = p", sc.with_word(g, 0, 2, P)), ("word = 2^64 - 1", sc.with_word(g, 1, 4, M64)), ("outside the group", sc.point_outside_the_group()),
            ("off the curve", point_off_the_curve()), ("x = 0, u != 0", (ec.ZERO, g[1])), ("x != 0, u = 0", (g[0], ec.ZERO))]


def good_points():
    return [ec.generator(), ref.g_mul_gen(RAND_M), ec.NEUTRAL]


def words5(k):
    return [(k >> (64 * i)) & M64 for i in range(5)]


def flat_point(p):
    return list(p[0]) + list(p[1])


def message5(seed):
    r = random.Random(SEED + 100 + seed)
    return tuple(r.randrange(P) for _ in range(5))


class DecryptCircuit:
    """public_key(sk) tied to pk, msg = elgamal_decrypt(sk, c0, c1) tied to msg; pk, c0, c1 and msg are public inputs when
    `public`.  hashed=True: the hashed cipher, ciphertext and message of five words."""

    def __init__(self, pkg, ec_gate, hashed=False, public=True):
        b = pkg.CircuitBuilder(ec_gate=ec_gate)
        self.hashed = hashed
        self.sk = b.add_secret_key()
        self.pk, self.c0 = b.add_virtual_point_target(), b.add_virtual_point_target()
        if hashed:
            self.c1, self.msg = b.add_virtual_target_arr(5), b.add_virtual_target_arr(5)
        else:
            self.c1, self.msg = b.add_virtual_point_target(), b.add_virtual_target_arr(10)
        if public:
            b.register_public_inputs(self.pk + self.c0 + self.c1 + self.msg)
        self.derived_pk = b.public_key(self.sk)
        for x, y in zip(self.derived_pk, self.pk):
            b.connect(x, y)
        self.out = (b.hashed_elgamal_decrypt if hashed else b.elgamal_decrypt)(self.sk, self.c0, self.c1)
        for x, y in zip(self.out, self.msg):
            b.connect(x, y)
        self.gates = b.num_gates()
        self.pkg, self.data = pkg, b.build()

    def witness(self, sk, pk, c0, c1, msg=None):
        """msg=None leaves the message to the witness run (the tests read self.out back)"""
        pw = self.pkg.PartialWitness()
        pw.set_biguint320_target(self.sk, sk)
        pw.set_point_target(self.pk, pk)
        pw.set_point_target(self.c0, c0)
        if self.hashed:
            pw.set_target_arr(self.c1, c1)
        else:
            pw.set_point_target(self.c1, c1)
        if msg is not None:
            pw.set_target_arr(self.msg, list(msg) if self.hashed else flat_point(msg))
        return pw.map
