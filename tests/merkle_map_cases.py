"""Shared by the MerkleMap tests (CPU and GPU): the value of a key, the D = 64 key list, the tampered proof set with the statuses
a verifier must give, the checks of a map against tests/merkle_map_ref.py, and the gadget circuits."""
import functools

import merkle_map_ref as ref

P = ref.P
VALUE_LENS = (0, 1, 3, 4, 8)          # a set; noop leaves up to the last one (3); the first hashed one (4); a second sponge block (8)
# D = 64: the ends of the key space and of its halves, a pair that differs only in bit 0 and one that differs only in bit 63
KEYS_64 = [0, 1, 1 << 63, (1 << 63) + 1, P - 1, 0x1234567890ABCDE0, 0x1234567890ABCDE1, 0x0FEDCBA987654321, 0x8FEDCBA987654321]


def value_of(key, value_len, tag=0):
    """canonical words that depend on the key; p - 1 and 0 are among them for value_len >= 2"""
    words = [(0x9E3779B97F4A7C15 * ((key + 1) % P) * (w + 1) + 7 * tag + w) % P for w in range(value_len)]
    if value_len >= 2:
        words[0], words[-1] = P - 1, 0
    return words


@functools.lru_cache(maxsize=None)
def model(keys, key_bits, cap_height, value_len):
    """the reference map of a key tuple, computed once"""
    return ref.Map({k: value_of(k, value_len) for k in keys}, key_bits, cap_height, value_len)


def entries(m):
    keys = list(m.entries)
    return keys, [m.entries[k] for k in keys]


def check_map(mm, m, queries):
    """cap, len and every queried proof of `mm` (a pkg.MerkleMap) are the reference's"""
    assert mm.cap == m.cap
    assert len(mm) == len(m.entries)
    assert mm.get_batch(queries) == [m.proof(k) for k in queries]


def tampered(m, key):
    """[(label, key, proof, cap, status)] around the proof of `key`, which must have a sibling and a value word"""
    present, value, sibs = m.proof(key)
    cap = m.cap
    out = [("the proof itself", key, (present, value, sibs), cap, 0)]
    bump = lambda w: (w + 1) % P                              # noqa: E731
    s2 = [list(h) for h in sibs]
    s2[len(s2) // 2][1] = bump(s2[len(s2) // 2][1])
    out.append(("a wrong sibling", key, (present, value, s2), cap, 1))
    s3 = [list(h) for h in sibs]
    s3[0][3] = P
    out.append(("a sibling word that is p", key, (present, value, s3), cap, 2))
    if present:
        v2 = list(value)
        v2[0] = bump(v2[0])
        out.append(("a wrong value", key, (present, v2, sibs), cap, 1))
        v3 = list(value)
        v3[-1] = (1 << 64) - 1
        out.append(("a value word that is 2^64 - 1", key, (present, v3, sibs), cap, 2))
    out.append(("the other flag", key, (1 - present, value, sibs), cap, 1))
    out.append(("a flag of 2", key, (2, value, sibs), cap, 2))
    # (the absence proofs of two empty neighbours are the same proof: the reference's walk says which case this is)
    out.append(("a neighbour's key", key ^ 1, (present, value, sibs), cap, 0 if ref.walk(key ^ 1, (present, value, sibs), cap, m.depth) else 1))
    if m.D < 64:
        out.append(("a key of 2^D", key | (1 << m.D), (present, value, sibs), cap, 2))
    else:
        out.append(("a key of p", P, (present, value, sibs), cap, 2))
    c2 = [list(h) for h in cap]
    c2[key >> m.depth][2] = bump(c2[key >> m.depth][2])
    out.append(("a wrong cap entry", key, (present, value, sibs), c2, 1))
    if len(cap) > 1:
        c3 = [list(h) for h in cap]
        c3[(key >> m.depth) ^ 1][0] = bump(c3[(key >> m.depth) ^ 1][0])
        out.append(("another cap entry changed", key, (present, value, sibs), c3, 0))
        c4 = [list(h) for h in cap]
        c4[(key >> m.depth) ^ 1][0] = P + 1
        out.append(("another cap entry not canonical", key, (present, value, sibs), c4, 2))
    return out


class MapCircuit:
    """One gadget on a map of key_bits bits: kind in lookup, update, insert, remove.  The cap (and the claimed new cap) are
    public inputs with public = True; lookup also publishes `present`."""

    def __init__(self, pkg, kind, key_bits, cap_height, value_len, public=True, **kw):
        b = pkg.CircuitBuilder(**kw)
        depth = key_bits - cap_height
        self.bits = b.add_virtual_target_arr(key_bits)
        self.cap = b.add_virtual_cap(cap_height)
        self.sibs = [b.add_virtual_hash() for _ in range(depth)]
        self.value = b.add_virtual_target_arr(value_len)
        self.present = self.new_present = None
        self.new_value, self.claimed = [], []
        pub = [t for h in self.cap for t in h]
        if kind == "lookup":
            self.present = b.add_virtual_target()
            b.merkle_map_lookup_to_cap(self.bits, self.value, self.present, self.cap, self.sibs)
            pub.append(self.present)
        else:
            if kind == "update":
                self.present, self.new_present, self.new_value = b.add_virtual_target(), b.add_virtual_target(), b.add_virtual_target_arr(value_len)
                new_cap = b.merkle_map_update_to_cap(self.bits, self.present, self.value, self.new_present, self.new_value, self.cap, self.sibs)
            else:
                new_cap = getattr(b, "merkle_map_%s_to_cap" % kind)(self.bits, self.value, self.cap, self.sibs)
            self.claimed = b.add_virtual_cap(cap_height)
            for x, y in zip(new_cap, self.claimed):
                b.connect_hashes(x, y)
            pub += [t for h in self.claimed for t in h]
        if public:
            b.register_public_inputs(pub)
        self.pkg, self.kind, self.gates = pkg, kind, b.num_gates()
        self.data = b.build()

    def witness(self, key, proof, cap, new=None, new_cap=None):
        """proof = (present, value, siblings) of the key under `cap`; new = (new_present, new_value) for update"""
        pw = self.pkg.PartialWitness()
        pw.set_cap_target(self.cap, cap)
        pw.set_merkle_map_proof_target((self.bits, self.present, self.value, self.sibs), key, proof)
        if self.kind == "update":
            pw.set_target(self.new_present, new[0])
            pw.set_target_arr(self.new_value, new[1])
        if self.claimed:
            pw.set_cap_target(self.claimed, new_cap)
        return pw.map
