"""What tests/test_vanishing_ref_host.py and tests/test_gpu_vanishing.py share: the circuits, opening sets that
tests/vanishing_ref.py alone makes valid (every opening but the quotient's and every challenge drawn, the left side evaluated in
Python, chunks 1..7 of the quotient openings drawn, chunk 0 solved), their single-coordinate perturbations with Python's verdict
on each, and the two hooks (p2_vanishing_terms, p2_gpu_vanishing_flags) behind one calling convention."""
import ctypes as C
import random

import circuits
import ec_circuits
import ghash_circuits
import pi_circuits
import proof_ref
import vanishing_ref as V

P = proof_ref.P
NAMES = ("arithmetic", "mix_columns", "aes_gcm", "ghash_mul", "small_table", "sbox_table", "poseidon_encrypt", "public_inputs",
         "ec_steps", "hashed_elgamal")
LOOKUP_NAMES = ("mix_columns", "aes_gcm", "ghash_mul", "small_table", "sbox_table")
EC_NAMES = ("ec_steps", "hashed_elgamal")
SMALLEST_TABLE = 1      # pair: the smallest table the builder accepts (it refuses an empty one); one row of 26 slots, 25 of them padding
VERDICT_CODE = {0: V.HOLDS, 5: V.FAILS, 4: V.IN_SUBGROUP}       # P2_VERIFY_OK, _VANISHING, _ZETA_IN_SUBGROUP
_built = {}


def _small_table(pkg):
    b = pkg.CircuitBuilder()
    lut = b.add_lookup_table_from_pairs([(3, 5)])
    x = b.add_virtual_target()
    b.add_lookup_from_index(x, lut)
    return b.build()


def build(pkg, name):
    """(info, blob, vanishing_ref.Circuit, CircuitData) of the named circuit, built once per process"""
    if name not in _built:
        if name == "arithmetic":
            data = circuits.arithmetic_only(pkg, [(3, 4, 5, 47)])[0]
        elif name == "mix_columns":
            data = circuits.mix_columns(pkg, circuits.random_states(3, 1))[0]
        elif name == "aes_gcm":
            data = circuits.encrypt(pkg, 4, 0, False)[0]
        elif name == "ghash_mul":
            data = ghash_circuits.mul(pkg)[0]
        elif name == "small_table":
            data = _small_table(pkg)
        elif name == "sbox_table":
            data = circuits.assert_byte(pkg, [7])[0]
        elif name == "poseidon_encrypt":
            data = circuits.poseidon_encrypt(pkg, 3, [1])[0]
        elif name == "public_inputs":
            data = pi_circuits.small(pkg, 3)[0]
        elif name == "ec_steps":
            data = ec_circuits.steps_circuit(pkg, 2)[0]
        elif name == "hashed_elgamal":
            data = ec_circuits.hashed_elgamal(pkg, [1])[0]
        else:
            raise KeyError(name)
        info = dict(data.info)
        _built[name] = (info, data.blob, V.Circuit(data.blob, info), data)
    return _built[name]


class Case:
    """one opening set with its challenges and public-inputs hash"""

    def __init__(self, o, ch, pi_hash, label=""):
        self.o, self.ch, self.pi_hash, self.label = o, ch, list(pi_hash), label

    def copy(self, label):
        return Case({k: list(v) for k, v in self.o.items()}, {k: list(v) for k, v in self.ch.items()}, self.pi_hash, label)

    def row(self):
        """the 16 challenge words of the hooks: betas gammas deltas[8] alphas zeta"""
        return self.ch["betas"] + self.ch["gammas"] + (self.ch["deltas"] or [0] * 8) + self.ch["alphas"] + list(self.ch["zeta"])


def solved(name, circ, fill, seed):
    """fill: "random", or a value every opening but the quotient's takes.  Challenges and quotient chunks 1..7 are random."""
    r = random.Random(seed)
    elem = (lambda: (r.randrange(P), r.randrange(P))) if fill == "random" else (lambda: (fill, fill))
    o = {k: [elem() for _ in range(circ.counts[k])] for k in V.OPEN if k != "quotient"}
    betas, gammas = [r.randrange(P) for _ in range(2)], [r.randrange(P) for _ in range(2)]
    ch = dict(betas=betas, gammas=gammas, deltas=betas + gammas + [r.randrange(P) for _ in range(4)] if circ.lookups else [],
              alphas=[r.randrange(P) for _ in range(2)], zeta=[r.randrange(P), r.randrange(P)])
    o["quotient"] = [(r.randrange(P), r.randrange(P)) for _ in range(circ.counts["quotient"])]
    pi_hash = [r.randrange(1, P) for _ in range(4)] if name == "public_inputs" else [0] * 4
    V.solve_quotient(circ, o, ch, pi_hash)
    return Case(o, ch, pi_hash, "solved %s" % fill)


def sweep(circ, base, second_every=7):
    """base with one coordinate increased by 1 mod p: the first coordinate of every element of every open_* section and the
    second of every `second_every`-th element (counted through the sections in OPEN's order)"""
    out, count = [], 0
    for name in V.OPEN:
        for e in range(circ.counts[name]):
            for coord in (0, 1):
                if coord == 0 or count % second_every == 0:
                    c = base.copy("%s[%d].%d + 1" % (name, e, coord))
                    v = list(c.o[name][e])
                    v[coord] = (v[coord] + 1) % P
                    c.o[name][e] = tuple(v)
                    out.append(c)
            count += 1
    return out


def python_verdict(circ, case):
    return V.verdict(circ, case.o, case.ch, case.pi_hash)


def host(pkg, info, blob, case):
    """p2_vanishing_terms -> (verdict, [terms], [(left, right)] per challenge)"""
    L = pkg.lib()
    buf = V.put_openings(info, case.o)
    cap = 1024
    terms, n, sides, verdict = (C.c_uint64 * (2 * cap))(), C.c_size_t(), (C.c_uint64 * 8)(), C.c_int(-1)
    rc = L.p2_vanishing_terms(blob, len(blob), buf, len(buf), (C.c_uint64 * 16)(*case.row()), (C.c_uint64 * 4)(*case.pi_hash), terms, cap,
                              C.byref(n), sides, C.byref(verdict))
    assert rc == 0, L.p2_last_error().decode()
    t = [(terms[2 * k], terms[2 * k + 1]) for k in range(n.value)]
    s = [((sides[4 * i], sides[4 * i + 1]), (sides[4 * i + 2], sides[4 * i + 3])) for i in range(2)]
    return VERDICT_CODE[verdict.value], t, s


def gpu_flags(pkg, data, info, cases):
    """p2_gpu_vanishing_flags on one batch -> [flags]"""
    L = pkg.lib()
    B = len(cases)
    bufs = b"".join(V.put_openings(info, c.o) for c in cases)
    rows = (C.c_uint64 * (16 * B))(*[w for c in cases for w in c.row()])
    hashes = (C.c_uint64 * (4 * B))(*[w for c in cases for w in c.pi_hash])
    flags = (C.c_uint32 * B)(*([0xFFFFFFFF] * B))
    rc = L.p2_gpu_vanishing_flags(data.gpu(), B, bufs, rows, hashes, flags)
    assert rc == 0, L.p2_last_error().decode()
    return list(flags)


def flags_verdict(f):
    """VF_ZETA = 8 (the kernel goes on past it, so VF_VANISH may come with it), VF_VANISH = 16"""
    assert f & ~24 == 0, f
    return V.IN_SUBGROUP if f & 8 else V.FAILS if f & 16 else V.HOLDS
