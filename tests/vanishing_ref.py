"""The vanishing identity at zeta in plain Python: Plonky2's `eval_vanishing_poly` on an opening set, written down from the
algorithm (upstream plonk/vanishing_poly.rs, gates/*.rs as recalled), in `int` arithmetic mod p and
GF(p^2) = F[x]/(x^2 - 7) as tests/proof_ref.py.  It shares no code with the product: the circuit comes from the blob
(tests/blob_reader.py), Poseidon's constants from poseidon_rc.inc and the MDS definition (tests/partial_rounds_ref.py), the
EcStepGate's formulas from tests/ec_circuits.py lifted to GF(p^2).

    vanishing(zeta) = sum_k term_k alpha^k = Z_H(zeta) sum_c t_c zeta^(n c),         once per challenge (alpha, t)

The term list, in order:
  * L_0(zeta) (Z_i - 1)                                                           for challenge i = 0, 1
  * per challenge, ten chunks of eight routed wires:  prev prod(w_j + beta k_j zeta + gamma) - next prod(w_j + beta sigma_j + gamma)
    with prev = Z, pp_0 .. pp_8 and next = pp_0 .. pp_8, Z(g zeta)
  * with lookup tables, per challenge (deltas a, b, alpha, delta):  LastLdc SLDC_last | InitSre SLDC_0 | InitSre RE |
    per table: its end selector (RE - the table's combos folded in delta, each row padded to 26 slots with zero) |
    TransSre (RE - fold of RE(g zeta) and the row's 26 combos) | per partial polynomial the looked (TransSre) and the looking
    (TransLdc) relation
  * num_gate_constraints slots: every gate's constraints under its filter, added slot by slot.
The filter of gate j in a selector group [lo, hi) with selector value s is prod_{k in group, k != j} (k - s), times (UNUSED - s)
when the circuit has more than one selector column."""
import numpy as np

import blob_reader
import ec_circuits
import partial_rounds_ref
import proof_ref
from proof_ref import GENERATOR, NUM_CHALLENGES, P, QDF, ROUTED, xadd, xinv, xmul, xsub

G_LOOKUP, G_LOOKUP_TABLE, G_NOOP, G_CONSTANT, G_PUBLIC_INPUT, G_ARITHMETIC, G_POSEIDON, G_ECSTEP = range(8)
NUM_CONSTRAINTS = {G_LOOKUP: 0, G_LOOKUP_TABLE: 0, G_NOOP: 0, G_CONSTANT: 2, G_PUBLIC_INPUT: 4, G_ARITHMETIC: 20, G_POSEIDON: 123,
                   G_ECSTEP: 40}
UNUSED_SELECTOR = (1 << 32) - 1
LU_SLOTS, LUT_SLOTS = ROUTED // 2, ROUTED // 3      # LookupGate: (input, output) pairs; LookupTableGate: (input, output, multiplicity)
NPP = (ROUTED + QDF - 1) // QDF - 1                 # partial products per challenge
NSLDC = (LU_SLOTS + QDF - 2) // (QDF - 1)           # partial lookup polynomials: QDF - 1 looking slots each
LUT_DEG = (LUT_SLOTS + NSLDC - 1) // NSLDC          # table slots per partial polynomial
NLP = NSLDC + 1                                     # RE, then the partial polynomials
SEL_TRANS_SRE, SEL_TRANS_LDC, SEL_INIT_SRE, SEL_LAST_LDC, SEL_START_END = range(5)
OPEN = ("constants", "sigmas", "wires", "zs", "zs_next", "lookup_zs", "lookup_zs_next", "partial_products", "quotient")
HOLDS, FAILS, IN_SUBGROUP = "holds", "fails", "opening point is in the subgroup"
ONE, ZERO = (1, 0), (0, 0)
EXT = ec_circuits.Quintic(xadd, xsub, xmul, lambda k: (k % P, 0))


def xscale(a, k):
    return (a[0] * k % P, a[1] * k % P)


def xpow(a, e):
    r = ONE
    while e:
        if e & 1:
            r = xmul(r, a)
        a = xmul(a, a)
        e >>= 1
    return r


def xprod(factors):
    r = ONE
    for f in factors:
        r = xmul(r, f)
    return r


class Circuit:
    """What the identity needs of a circuit, from its blob, and what depends on the blob and the deltas alone: the table sums."""

    def __init__(self, blob, info):
        b = blob_reader.Blob(blob)
        self.n, self.degree_bits = b.n, b.degree_bits
        self.gates = [int(g) for g in b.gates]
        self.selector_index = [int(s) for s in b.selector_index]
        self.groups = [(int(lo), int(hi)) for lo, hi in b.groups]
        self.nsel, self.nls, self.ngc = len(self.groups), int(b.num_lookup_selectors), int(b.num_gate_constraints)
        self.k_is = [int(k) for k in b.k_is]
        self.luts = [(t[:, 0].astype(object), t[:, 1].astype(object)) for t in b.luts]
        self.lookups = len(b.luts) > 0
        # the coset shifts are upstream's get_unique_coset_shifts: the powers of the field's multiplicative generator
        assert self.k_is == [pow(GENERATOR, i, P) for i in range(ROUTED)]
        assert self.nls == (SEL_START_END + len(self.luts) if self.lookups else 0)
        assert self.ngc == max([NUM_CONSTRAINTS[g] for g in self.gates] + [0])
        assert info["num_zs_cols"] == NUM_CHALLENGES * (1 + NPP + (NLP if self.lookups else 0))
        assert info["num_constants_cols"] == self.nsel + self.nls + 2 and info["num_quotient_cols"] == NUM_CHALLENGES * QDF
        self.counts = dict(constants=self.nsel + self.nls + 2, sigmas=ROUTED, wires=info["num_wires"], zs=NUM_CHALLENGES,
                           zs_next=NUM_CHALLENGES, lookup_zs=NUM_CHALLENGES * NLP if self.lookups else 0,
                           lookup_zs_next=NUM_CHALLENGES * NLP if self.lookups else 0, partial_products=NUM_CHALLENGES * NPP,
                           quotient=NUM_CHALLENGES * QDF)
        self._sums = {}

    def table_sums(self, b, delta):
        """per table sum_j (in_j + b out_j) delta^(26 rows - 1 - j): the table's combos as the coefficients of a polynomial of
        degree 26 rows - 1, highest first, zero on the padding of the last row, at delta"""
        key = (b, delta)
        if key not in self._sums:
            out = []
            for ins, outs in self.luts:
                size = len(ins)
                total = -(-size // LUT_SLOTS) * LUT_SLOTS
                combos = (ins + b * outs) % P
                acc, pw = 0, pow(delta, total - size, P)       # the last entry's power: the padding lies below it
                for j in range(size - 1, -1, -1):
                    acc += int(combos[j]) * pw
                    pw = pw * delta % P
                out.append(acc % P)
            self._sums[key] = out
        return self._sums[key]


_rc = []


def _poseidon_constraints(w):
    """PoseidonGate (gates/poseidon.rs): swap is boolean; delta_i = swap (in_{i+4} - in_i); the permutation of the swapped input
    by textbook rounds (constants, S-box x^7, MDS = circulant + diag(8, 0, ..)), every S-box input but the first full round's
    re-based on its wire; outputs.  Wires: 12 in | 12 out | swap | 4 delta | 3x12 | 22 | 4x12."""
    if not _rc:
        _rc.extend(partial_rounds_ref.round_constants())
    IN, OUT, SWAP, DELTA, FULL0, PARTIAL, FULL1 = 0, 12, 24, 25, 29, 65, 87
    out = []
    swap = w[SWAP]
    out.append(xmul(swap, xsub(swap, ONE)))
    st = [None] * 12
    for i in range(4):
        lhs, rhs, d = w[IN + i], w[IN + 4 + i], w[DELTA + i]
        out.append(xsub(xmul(swap, xsub(rhs, lhs)), d))
        st[i], st[i + 4] = xadd(lhs, d), xsub(rhs, d)
    st[8:] = w[IN + 8:IN + 12]

    def sbox(x):
        x2 = xmul(x, x)
        x4 = xmul(x2, x2)
        return xmul(xmul(x4, x2), x)

    def mds(v):
        return [(sum(partial_rounds_ref.mds_entry(r, c) * v[c][0] for c in range(12)) % P,
                 sum(partial_rounds_ref.mds_entry(r, c) * v[c][1] for c in range(12)) % P) for r in range(12)]

    for rnd in range(30):
        st = [((x[0] + _rc[12 * rnd + i]) % P, x[1]) for i, x in enumerate(st)]
        if rnd < 4 or rnd >= 26:
            if rnd:
                first = FULL0 + 12 * (rnd - 1) if rnd < 4 else FULL1 + 12 * (rnd - 26)
                for i in range(12):
                    out.append(xsub(st[i], w[first + i]))
                    st[i] = w[first + i]
            st = [sbox(x) for x in st]
        else:
            sin = w[PARTIAL + rnd - 4]
            out.append(xsub(st[0], sin))
            st[0] = sbox(sin)
        st = mds(st)
    out += [xsub(st[i], w[OUT + i]) for i in range(12)]
    assert len(out) == 123
    return out


def gate_constraints(kind, w, consts, pi_hash):
    """the unfiltered constraints of one gate on the wires w (extension elements) and its two constants"""
    if kind == G_ARITHMETIC:        # 20 ops: out = c0 m0 m1 + c1 addend
        return [xsub(w[4 * i + 3], xadd(xmul(xmul(w[4 * i], w[4 * i + 1]), consts[0]), xmul(w[4 * i + 2], consts[1]))) for i in range(20)]
    if kind == G_CONSTANT:
        return [xsub(consts[i], w[i]) for i in range(2)]
    if kind == G_PUBLIC_INPUT:
        return [xsub(w[i], (pi_hash[i] % P, 0)) for i in range(4)]
    if kind == G_POSEIDON:
        return _poseidon_constraints(w)
    if kind == G_ECSTEP:
        return ec_circuits.constraints(w, EXT)
    return []


def lookup_terms(circ, o, d, i):
    """the lookup terms of challenge i; d = (a, b, alpha, delta)"""
    w = o["wires"]
    sel = o["constants"][circ.nsel:circ.nsel + circ.nls]
    z, zn = o["lookup_zs"][i * NLP:(i + 1) * NLP], o["lookup_zs_next"][i * NLP:(i + 1) * NLP]
    re, sldc, sldc_next = z[0], z[1:], zn[1:]
    a, b, alpha, delta = d
    looked = [xadd(w[3 * s], xscale(w[3 * s + 1], a)) for s in range(LUT_SLOTS)]
    table = [xadd(w[3 * s], xscale(w[3 * s + 1], b)) for s in range(LUT_SLOTS)]
    looking = [xadd(w[2 * s], xscale(w[2 * s + 1], a)) for s in range(LU_SLOTS)]
    terms = [xmul(sel[SEL_LAST_LDC], sldc[NSLDC - 1]), xmul(sel[SEL_INIT_SRE], sldc[0]), xmul(sel[SEL_INIT_SRE], re)]
    for t, total in enumerate(circ.table_sums(b, delta)):
        terms.append(xmul(sel[SEL_START_END + t], xsub(re, (total, 0))))
    cur = zn[0]
    for c in table:
        cur = xadd(xscale(cur, delta), c)
    terms.append(xmul(sel[SEL_TRANS_SRE], xsub(re, cur)))
    al = (alpha, 0)
    for k in range(NSLDC):
        lut = [xsub(al, c) for c in looked[k * LUT_DEG:(k + 1) * LUT_DEG]]
        mult = [w[3 * s + 2] for s in range(k * LUT_DEG, min((k + 1) * LUT_DEG, LUT_SLOTS))]
        lu = [xsub(al, c) for c in looking[k * (QDF - 1):(k + 1) * (QDF - 1)]]
        # Sum: sldc_k - prev = sum_s mult_s / (alpha - looked_s);  LDC: sldc_k - prev = - sum_s 1 / (alpha - looking_s); cleared
        # of denominators; the first partial polynomial continues the last one of the next row
        diff = xsub(sldc[k], sldc_next[NSLDC - 1] if k == 0 else sldc[k - 1])
        mult_sum, inv_sum = ZERO, ZERO
        for s in range(len(lut)):
            mult_sum = xadd(mult_sum, xmul(mult[s], xprod(lut[:s] + lut[s + 1:])))
        for s in range(len(lu)):
            inv_sum = xadd(inv_sum, xprod(lu[:s] + lu[s + 1:]))
        terms.append(xmul(sel[SEL_TRANS_SRE], xsub(xmul(xprod(lut), diff), mult_sum)))
        terms.append(xmul(sel[SEL_TRANS_LDC], xadd(xmul(xprod(lu), diff), inv_sum)))
    return terms


def terms(circ, o, ch, pi_hash):
    """the flat term list; o: {section name without "open_": [extension elements]}, ch: betas, gammas, deltas, alphas, zeta"""
    for name in OPEN:
        assert len(o[name]) == circ.counts[name], name
    zeta, w, sig = tuple(ch["zeta"]), o["wires"], o["sigmas"]
    zh = xsub(xpow(zeta, circ.n), ONE)
    l0 = xmul(zh, xinv(xscale(xsub(zeta, ONE), circ.n)))       # L_0(x) = (x^n - 1) / (n (x - 1))
    out = [xmul(l0, xsub(o["zs"][i], ONE)) for i in range(NUM_CHALLENGES)]
    for i in range(NUM_CHALLENGES):
        beta, gamma = ch["betas"][i], (ch["gammas"][i], 0)
        pp = o["partial_products"][i * NPP:(i + 1) * NPP]
        acc = [o["zs"][i]] + pp + [o["zs_next"][i]]
        for c in range(NPP + 1):
            cols = range(QDF * c, QDF * (c + 1))
            num = xprod([xadd(xadd(w[j], xscale(zeta, beta * circ.k_is[j] % P)), gamma) for j in cols])
            den = xprod([xadd(xadd(w[j], xscale(sig[j], beta)), gamma) for j in cols])
            out.append(xsub(xmul(acc[c], num), xmul(acc[c + 1], den)))
    if circ.lookups:
        for i in range(NUM_CHALLENGES):
            out += lookup_terms(circ, o, ch["deltas"][4 * i:4 * i + 4], i)
    slots = [ZERO] * circ.ngc
    consts = o["constants"][circ.nsel + circ.nls:]
    for j, kind in enumerate(circ.gates):
        if not NUM_CONSTRAINTS[kind]:
            continue
        lo, hi = circ.groups[circ.selector_index[j]]
        s = o["constants"][circ.selector_index[j]]
        f = xprod([xsub((k, 0), s) for k in range(lo, hi) if k != j])
        if circ.nsel > 1:
            f = xmul(f, xsub((UNUSED_SELECTOR, 0), s))
        for k, c in enumerate(gate_constraints(kind, w, consts, pi_hash)):
            slots[k] = xadd(slots[k], xmul(f, c))
    return out + slots


def sides(circ, o, ch, term_list=None, pi_hash=(0, 0, 0, 0)):
    """[(left, right)] per challenge: sum_k term_k alpha^k and Z_H(zeta) sum_c t_c zeta^(n c)"""
    if term_list is None:
        term_list = terms(circ, o, ch, pi_hash)
    zeta = tuple(ch["zeta"])
    zn = xpow(zeta, circ.n)
    zh = xsub(zn, ONE)
    out = []
    for i in range(NUM_CHALLENGES):
        left = ZERO
        for t in reversed(term_list):
            left = xadd(xscale(left, ch["alphas"][i]), t)
        t_zeta = ZERO
        for c in reversed(o["quotient"][i * QDF:(i + 1) * QDF]):
            t_zeta = xadd(xmul(t_zeta, zn), c)
        out.append((left, xmul(zh, t_zeta)))
    return out


def in_subgroup(circ, ch):
    return xpow(tuple(ch["zeta"]), circ.n) == ONE


def verdict(circ, o, ch, pi_hash=(0, 0, 0, 0)):
    """HOLDS, FAILS or IN_SUBGROUP (checked first, as the verifier does: L_0 has a pole there)"""
    if in_subgroup(circ, ch):
        return IN_SUBGROUP
    return HOLDS if all(l == r for l, r in sides(circ, o, ch, None, pi_hash)) else FAILS


def solve_quotient(circ, o, ch, pi_hash=(0, 0, 0, 0)):
    """sets chunk 0 of each challenge's quotient openings so that the identity holds with the other openings as they are"""
    left = [l for l, _ in sides(circ, o, ch, None, pi_hash)]
    zeta = tuple(ch["zeta"])
    zn = xpow(zeta, circ.n)
    zh_inv = xinv(xsub(zn, ONE))
    for i in range(NUM_CHALLENGES):
        rest = ZERO
        for c in reversed(o["quotient"][i * QDF + 1:(i + 1) * QDF]):
            rest = xadd(xmul(rest, zn), c)
        o["quotient"][i * QDF] = xsub(xmul(left[i], zh_inv), xmul(rest, zn))


def openings_of(info, proof):
    S = proof_ref.sections(info)
    return {name: proof_ref.ext_words(proof, S, "open_" + name) for name in OPEN}


def put_openings(info, o, buf=None):
    """a proof-sized buffer (zeros, or a copy of buf) with the open_* sections written from o"""
    S = proof_ref.sections(info)
    out = np.zeros(info["proof_bytes"], dtype=np.uint8) if buf is None else np.frombuffer(bytes(buf), dtype=np.uint8).copy()
    for name in OPEN:
        off, nbytes, _ = S["open_" + name]
        out[off:off + nbytes] = np.array([v for e in o[name] for v in e], dtype="<u8").view(np.uint8)
    return out.tobytes()


_circuits = {}


def check_vanishing(info, blob, proof, transcript):
    """None, or a string naming the first challenge whose identity fails (or that zeta lies in the subgroup)"""
    key = bytes(blob)
    if key not in _circuits:
        _circuits[key] = Circuit(blob, info)
    circ = _circuits[key]
    if in_subgroup(circ, transcript):
        return "zeta: the opening point is in the subgroup"
    pi_hash = proof_ref.hash_public_inputs(proof_ref.trailer_values(info, proof))
    for i, (l, r) in enumerate(sides(circ, openings_of(info, proof), transcript, None, pi_hash)):
        if l != r:
            return "open_quotient: the vanishing identity of challenge %d does not hold at zeta" % i
    return None
