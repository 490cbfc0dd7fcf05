"""An independent replay of a serialised proof: the Fiat-Shamir transcript, the Merkle paths and the FRI checks of the Plonky2
verifier, written down from the algorithm as DESIGN.md section 8 and oracle/oracle_prover.h describe it, in Python `int`
arithmetic mod p = 2^64 - 2^32 + 1 (numpy only moves bytes).  It shares no code with the product: byte offsets come from
verify_layout.sections, the challenger's permutation is the CPU oracle's Poseidon (oracle_lib), and the tree hasher is passed
in as a pair of functions (hash_no_pad(words [..., n]) -> [..., 4], two_to_one(l [..., 4], r [..., 4]) -> [..., 4]):
`keccak_hasher()` (tests/keccak_ref.py) or `poseidon_hasher()` (the oracle's).

What the replay restates: the transcript (challenges, proof-of-work response, query indices), every Merkle path against its
cap, canonical encoding, the reduced composition value of each query from the opened leaves and the opening set, every
arity-16 fold and the final polynomial.  The vanishing identity at zeta (the gate, permutation and lookup constraints evaluated
on the opening set) is restated in tests/vanishing_ref.py, which needs the circuit's blob: `replay(..., blob=...)` runs it
between the proof-of-work test and the Merkle checks, the host verifier's order; without a blob the replay leaves it out.

Every check returns None when it holds and otherwise a string naming the first thing that failed (section, query, round)."""
import ctypes as C
import re

import numpy as np

import keccak_ref
import oracle_lib
import verify_layout

P = (1 << 64) - (1 << 32) + 1
W_EXT = 7                                   # GF(p^2) = F[x] / (x^2 - 7)
GENERATOR = 14293326489335486720            # the field's multiplicative generator = the coset shift of every LDE
ROOT_2_32 = pow(GENERATOR, (P - 1) >> 32, P)  # of order 2^32; root_of_unity(bits) is its 2^(32 - bits)-th power
assert ROOT_2_32 == 7277203076849721926 and pow(ROOT_2_32, 1 << 31, P) == P - 1
ROUTED, NUM_CHALLENGES, QDF, RATE_BITS, CAP_HEIGHT, POW_BITS, NUM_QUERIES, ARITY_BITS = 80, 2, 8, 3, 4, 16, 28, 4
ARITY = 1 << ARITY_BITS


# ------------------------------------------------------------------------------------------------ field
def root_of_unity(bits):
    return pow(ROOT_2_32, 1 << (32 - bits), P)


def rev_bits(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def xmul(a, b):
    return ((a[0] * b[0] + W_EXT * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def xadd(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def xsub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def xinv(a):
    ni = pow((a[0] * a[0] - W_EXT * a[1] * a[1]) % P, P - 2, P)
    return (a[0] * ni % P, -a[1] * ni % P)


def xpowers(z, count):
    """[z^0 .. z^(count-1)] as two lists (first and second coordinate)"""
    pa, pb, cur = [], [], (1, 0)
    for _ in range(count):
        pa.append(cur[0])
        pb.append(cur[1])
        cur = xmul(cur, z)
    return pa, pb


def _dot(xs, ys):
    return sum(map(int.__mul__, xs, ys))


# ------------------------------------------------------------------------------------------------ hashers, challenger
def _rows(fn):
    """a function of one row of words -> the [..., n] -> [..., 4] form the replay calls"""
    def wrapped(*arrays):
        arrays = [np.asarray(a, dtype=np.uint64) for a in arrays]
        lead = arrays[0].shape[:-1]
        flat = [a.reshape(-1, a.shape[-1]) for a in arrays]
        out = np.array([fn(*[[int(w) for w in a[i]] for a in flat]) for i in range(flat[0].shape[0])], dtype=np.uint64)
        return out.reshape(lead + (4,))
    return wrapped


def _orc_hash_no_pad(words):
    out = (C.c_uint64 * 4)()
    oracle_lib.lib().orc_hash_no_pad((C.c_uint64 * len(words))(*words), len(words), out)
    return list(out)


def _orc_two_to_one(l, r):
    out = (C.c_uint64 * 4)()
    oracle_lib.lib().orc_two_to_one((C.c_uint64 * 4)(*l), (C.c_uint64 * 4)(*r), out)
    return list(out)


def poseidon_hasher():
    return _rows(_orc_hash_no_pad), _rows(_orc_two_to_one)


def keccak_hasher():
    return keccak_ref.hash_no_pad, keccak_ref.two_to_one


def hash_public_inputs(values):
    """hash_no_pad of the public inputs: Poseidon under either tree hasher, four zeros when there are none"""
    return _orc_hash_no_pad(list(values)) if len(values) else [0, 0, 0, 0]


class Challenger:
    """The duplex challenger: inputs overwrite the rate part of the state eight at a time, challenges pop from the back of the
    eight outputs, an observation discards what is left of them."""

    def __init__(self):
        self.state, self.inputs, self.outputs = [0] * 12, [], []

    def _duplex(self):
        self.state[:len(self.inputs)] = self.inputs
        self.inputs = []
        st = (C.c_uint64 * 12)(*self.state)
        oracle_lib.lib().orc_poseidon(st)
        self.state = list(st)
        self.outputs = self.state[:8]

    def observe(self, words):
        for w in words:
            self.outputs = []
            self.inputs.append(int(w))
            if len(self.inputs) == 8:
                self._duplex()

    def challenge(self):
        if self.inputs or not self.outputs:
            self._duplex()
        return self.outputs.pop()

    def challenges(self, count):
        return [self.challenge() for _ in range(count)]


# ------------------------------------------------------------------------------------------------ the proof's bytes
def shape(info):
    """the counts the protocol needs, from the circuit's info dict alone"""
    npp = (ROUTED + QDF - 1) // QDF - 1
    nzpp = NUM_CHALLENGES * (1 + npp)
    zc = info["num_zs_cols"]
    return dict(n=1 << info["degree_bits"], lde_bits=info["degree_bits"] + RATE_BITS, rounds=info["num_fri_rounds"],
                pre=info["num_constants_cols"] + ROUTED, wires=info["num_wires"], zc=zc, nzpp=nzpp, lookups=zc > nzpp,
                qc=info["num_quotient_cols"], keccak=info.get("hasher", "poseidon") == "keccak")


def sections(info):
    """verify_layout.sections of the proof body, plus the public-input trailer (count word, values) where there is one"""
    k = info["num_public_inputs"]
    body = info["proof_bytes"] - (8 + 8 * k if k else 0)
    S = dict(verify_layout.sections(dict(info, proof_bytes=body)))
    if k:
        S["pi_count"] = (body, 8, "words")
        S["pi_values"] = (body + 8, 8 * k, "words")
    return S


def words(proof, S, name):
    off, nbytes, _ = S[name]
    return [int(w) for w in np.frombuffer(proof, dtype="<u8", count=nbytes // 8, offset=off)]


def ext_words(proof, S, name):
    w = words(proof, S, name)
    return list(zip(w[0::2], w[1::2]))


def trailer_values(info, proof):
    """the public-input values of the trailer (registration order); [] for a circuit without public inputs"""
    return words(proof, sections(info), "pi_values") if info["num_public_inputs"] else []


BATCH0 = ("constants", "sigmas", "wires", "zs", "partial_products", "quotient", "lookup_zs")  # opened at zeta, observed order
BATCH1 = ("zs_next", "lookup_zs_next")                                                         # opened at g zeta


# ------------------------------------------------------------------------------------------------ transcript
def replay_transcript(info, verifier_data, proof, public_inputs_hash):
    """The challenger over circuit digest, public-inputs hash, wires cap -> betas, gammas (and, with lookups, four more:
    deltas = betas | gammas | those) -> Z cap -> alphas -> quotient cap -> zeta -> openings in batch order -> fri_alpha ->
    per round cap -> beta -> final polynomial -> PoW witness -> response -> 28 indices.  Returns a dict; "pow_ok" says whether
    the response has the 16 leading zeros."""
    sh, S = shape(info), sections(info)
    ch = Challenger()
    ch.observe(verifier_data[4 << CAP_HEIGHT:])
    ch.observe(public_inputs_hash)
    ch.observe(words(proof, S, "wires_cap"))
    t = {"betas": ch.challenges(NUM_CHALLENGES), "gammas": ch.challenges(NUM_CHALLENGES), "deltas": []}
    if sh["lookups"]:
        t["deltas"] = t["betas"] + t["gammas"] + ch.challenges(2 * NUM_CHALLENGES)
    ch.observe(words(proof, S, "zs_cap"))
    t["alphas"] = ch.challenges(NUM_CHALLENGES)
    ch.observe(words(proof, S, "quotient_cap"))
    t["zeta"] = ch.challenges(2)
    for name in BATCH0 + BATCH1:
        ch.observe(words(proof, S, "open_" + name))
    t["fri_alpha"] = ch.challenges(2)
    t["fri_betas"] = []
    for r in range(sh["rounds"]):
        ch.observe(words(proof, S, "fri_cap%d" % r))
        t["fri_betas"] += ch.challenges(2)
    ch.observe(words(proof, S, "final_poly"))
    t["pow_witness"] = words(proof, S, "pow_witness")
    ch.observe(t["pow_witness"])
    t["pow_response"] = ch.challenge()
    t["pow_ok"] = t["pow_response"] >> (64 - POW_BITS) == 0
    t["query_indices"] = [ch.challenge() % (1 << sh["lde_bits"]) for _ in range(NUM_QUERIES)]
    return t


# ------------------------------------------------------------------------------------------------ Merkle paths
def check_canonical(info, proof):
    """every u64 word of the proof below p; under Keccak every word of a cap entry or sibling below 2^56 (the fourth 2^32)"""
    sh, S = shape(info), sections(info)
    if len(proof) != info["proof_bytes"]:
        return "proof: %d bytes, the circuit's proofs have %d" % (len(proof), info["proof_bytes"])
    for name, (off, nbytes, kind) in S.items():
        if kind != "words":
            continue
        w = np.frombuffer(proof, dtype="<u8", count=nbytes // 8, offset=off)
        if (w >= np.uint64(P)).any():
            return "%s: word %d is not below p" % (name, int(np.argmax(w >= np.uint64(P))))
        if sh["keccak"] and (name.endswith("_cap") or name.endswith("_siblings") or "fri_cap" in name):
            limit = np.tile(np.array([1 << 56] * 3 + [1 << 32], dtype=np.uint64), w.size // 4)
            if (w >= limit).any():
                return "%s: hash word %d out of range" % (name, int(np.argmax(w >= limit)))
    if info["num_public_inputs"] and words(proof, S, "pi_count") != [info["num_public_inputs"]]:
        return "pi_count: wrong number of public inputs"
    return None


def _walk(leaf_digests, siblings, positions, two_to_one):
    """leaf_digests [m, 4], siblings [m, depth, 4], positions [m] -> (roots [m, 4], what is left of each position)"""
    h, pos = np.asarray(leaf_digests, dtype=np.uint64), np.array(positions, dtype=np.int64)
    for lvl in range(siblings.shape[1]):
        sib, right = siblings[:, lvl, :], (pos & 1).astype(bool)[:, None]
        h = np.asarray(two_to_one(np.where(right, sib, h), np.where(right, h, sib)), dtype=np.uint64)
        pos >>= 1
    return h, pos


def check_merkle(info, verifier_data, proof, indices, hasher):
    """Canonical words, sibling counts, then for every query the four initial-tree paths (constants|sigmas against the cap of
    the verifier data, wires / Z / quotient against the proof's caps) and the path of each round's 16-evaluation leaf against
    that round's cap.  A leaf at position x hashes with hash_no_pad; going up, the node is the left operand when its position
    is even; after `depth` levels what is left of the position picks the cap entry."""
    bad = check_canonical(info, proof)
    if bad:
        return bad
    hash_no_pad, two_to_one = hasher
    sh, S = shape(info), sections(info)
    Q = len(indices)

    def block(fmt, per):
        return np.array([words(proof, S, fmt % q) for q in range(Q)], dtype=np.uint64).reshape(Q, -1, per)

    trees = [("init%d" % o, "leaf", 0, sh["lde_bits"] - CAP_HEIGHT) for o in range(4)]
    trees += [("round%d" % r, "evals", ARITY_BITS * (r + 1), sh["lde_bits"] - ARITY_BITS * (r + 1) - CAP_HEIGHT) for r in range(sh["rounds"])]
    for tree, _, _, depth in trees:
        for q in range(Q):
            if proof[S["q%d_%s_count" % (q, tree)][0]] != depth:
                return "q%d_%s_count: %d siblings, the tree has %d levels below its cap" % (q, tree, proof[S["q%d_%s_count" % (q, tree)][0]], depth)
    caps = [np.array(verifier_data[:4 << CAP_HEIGHT], dtype=np.uint64).reshape(-1, 4)]
    caps += [np.array(words(proof, S, c), dtype=np.uint64).reshape(-1, 4) for c in ("wires_cap", "zs_cap", "quotient_cap")]
    caps += [np.array(words(proof, S, "fri_cap%d" % r), dtype=np.uint64).reshape(-1, 4) for r in range(sh["rounds"])]
    verdicts = {}
    for (tree, leaf, shift, depth), cap in zip(trees, caps):
        leaves = block("q%%d_%s_%s" % (tree, leaf), 1)[:, :, 0]
        sibs = block("q%%d_%s_siblings" % tree, 4) if depth else np.zeros((Q, 0, 4), dtype=np.uint64)
        roots, top = _walk(hash_no_pad(leaves), sibs, [x >> shift for x in indices], two_to_one)
        for q in range(Q):
            if [int(w) for w in roots[q]] != [int(w) for w in cap[int(top[q])]]:
                verdicts[(q, tree)] = "q%d_%s: Merkle path does not end in cap entry %d" % (q, tree, int(top[q]))
    for q in range(Q):
        for tree, _, _, _ in trees:
            if (q, tree) in verdicts:
                return verdicts[(q, tree)]
    return None


# ------------------------------------------------------------------------------------------------ FRI
def _interpolate(points, values, at):
    """the polynomial of degree < len(points) through (points[k] in the base field, values[k] in the extension), at `at`"""
    total = (0, 0)
    for k, (xk, vk) in enumerate(zip(points, values)):
        num, den = (1, 0), 1
        for j, xj in enumerate(points):
            if j != k:
                num = xmul(num, xsub(at, (xj, 0)))
                den = den * (xk - xj) % P
        di = pow(den, P - 2, P)
        total = xadd(total, xmul(xmul(num, vk), (di, 0)))
    return total


def check_fri(info, proof, challenges, indices):
    """Query x (a leaf position: the domain point is g w^rev(x)): the reduced composition value from the opened leaves,
    sum0 alpha^|batch1| + sum1 with sum_b = (sum_j alpha^j f_j(point) - sum_j alpha^j opening_j) / (point - z_b), z_0 = zeta,
    z_1 = g_n zeta, salt columns left out, against element x & 15 of the round-0 leaf; each round's leaf interpolated over its
    coset {y w16^rev(k)} at beta against element (x >> 4(r+1)) & 15 of the next leaf; the last against the final polynomial."""
    sh, S = shape(info), sections(info)
    n, lde_bits, rounds, nzpp, zc = sh["n"], sh["lde_bits"], sh["rounds"], sh["nzpp"], sh["zc"]
    zeta, alpha = tuple(challenges["zeta"]), tuple(challenges["fri_alpha"])
    g_zeta = xmul(zeta, (root_of_unity(info["degree_bits"]), 0))
    open0 = [e for name in BATCH0 for e in ext_words(proof, S, "open_" + name)]
    open1 = [e for name in BATCH1 for e in ext_words(proof, S, "open_" + name)]
    pa, pb = xpowers(alpha, len(open0) + 1)
    reduced = []
    for op in (open0, open1):
        reduced.append(((_dot(pa, [e[0] for e in op]) + W_EXT * _dot(pb, [e[1] for e in op])) % P,
                        (_dot(pa, [e[1] for e in op]) + _dot(pb, [e[0] for e in op])) % P))
    shift1 = (pa[len(open1)], pb[len(open1)])
    betas = list(zip(challenges["fri_betas"][0::2], challenges["fri_betas"][1::2]))
    final = ext_words(proof, S, "final_poly")
    if len(final) != n >> (ARITY_BITS * rounds) or len(betas) != rounds:
        return "final_poly: %d coefficients, %d betas for %d rounds" % (len(final), len(betas), rounds)
    w_lde, w16 = root_of_unity(lde_bits), root_of_unity(ARITY_BITS)
    for q, x_index in enumerate(indices):
        pre, wires, zs, quot = (words(proof, S, "q%d_init%d_leaf" % (q, o)) for o in range(4))
        f0 = pre[:sh["pre"]] + wires[:sh["wires"]] + zs[:nzpp] + quot[:sh["qc"]] + zs[nzpp:zc]
        f1 = zs[:NUM_CHALLENGES] + zs[nzpp:zc]
        if len(f0) != len(open0) or len(f1) != len(open1):
            return "q%d: %d + %d leaf columns for %d + %d openings" % (q, len(f0), len(f1), len(open0), len(open1))
        point = GENERATOR * pow(w_lde, rev_bits(x_index, lde_bits), P) % P
        value = (0, 0)
        for f, red, z in ((f0, reduced[0], zeta), (f1, reduced[1], g_zeta)):
            comp = (_dot(pa, f) % P, _dot(pb, f) % P)
            term = xmul(xsub(comp, red), xinv(xsub((point, 0), z)))
            value = xadd(xmul(value, shift1), term) if f is f1 else term
        bits, pos, shift = lde_bits, x_index, GENERATOR
        for r in range(rounds):
            evals = ext_words(proof, S, "q%d_round%d_evals" % (q, r))
            if evals[pos & (ARITY - 1)] != value:
                return "q%d_round%d_evals: element %d is not %s" % (q, r, pos & (ARITY - 1),
                                                                    "the composition value of the leaves" if r == 0 else "the fold of round %d" % (r - 1))
            coset = pos >> ARITY_BITS
            y = shift * pow(root_of_unity(bits), rev_bits(coset, bits - ARITY_BITS), P) % P
            value = _interpolate([y * pow(w16, rev_bits(k, ARITY_BITS), P) % P for k in range(ARITY)], evals, betas[r])
            bits, pos, shift = bits - ARITY_BITS, coset, pow(shift, ARITY, P)
        point = shift * pow(root_of_unity(bits), rev_bits(pos, bits), P) % P
        acc = (0, 0)
        for c in reversed(final):
            acc = ((acc[0] * point + c[0]) % P, (acc[1] * point + c[1]) % P)
        if acc != value:
            return "q%d final_poly: its value at the query point is not %s" % (q, "the fold of round %d" % (rounds - 1) if rounds else
                                                                                "the composition value of the leaves")
    return None


def replay(info, verifier_data, proof, hasher, blob=None):
    """All of it on the proof alone (public-inputs hash from the trailer): None, or the first failure.  With the circuit's
    blob also the vanishing identity at zeta (vanishing_ref.check_vanishing)."""
    bad = check_canonical(info, proof)
    if bad:
        return bad
    t = replay_transcript(info, verifier_data, proof, hash_public_inputs(trailer_values(info, proof)))
    if not t["pow_ok"]:
        return "pow_witness: the response %#x has fewer than %d leading zeros" % (t["pow_response"], POW_BITS)
    if blob is not None:
        import vanishing_ref   # it imports this module
        bad = vanishing_ref.check_vanishing(info, blob, proof, t)
        if bad:
            return bad
    return check_merkle(info, verifier_data, proof, t["query_indices"], hasher) or check_fri(info, proof, t, t["query_indices"])


# ------------------------------------------------------------------------------------------------ openings
def eval_openings(cols_coeffs, n, zeta):
    """Base-field coefficient columns ([cols][n], flat or not) at the extension point zeta: [(c0, c1)] per column.  The n powers
    of zeta are computed once; a column is two integer dot products, reduced mod p at the end."""
    cols = np.asarray(cols_coeffs, dtype=np.uint64).reshape(-1, n)
    pa, pb = xpowers(tuple(zeta), n)
    out = []
    for col in cols:
        c = col.tolist()
        out.append((_dot(c, pa) % P, _dot(c, pb) % P))
    return out


def fold_coefficients(coeffs, betas):
    """The commit phase on coefficients: folded[k] = sum_i beta^i coeffs[16 k + i], once per beta."""
    for beta in betas:
        out = []
        for k in range(len(coeffs) // ARITY):
            acc = (0, 0)
            for c in reversed(coeffs[ARITY * k: ARITY * k + ARITY]):
                acc = xadd(xmul(acc, beta), c)
            out.append(acc)
        coeffs = out
    return coeffs


# ------------------------------------------------------------------------------------------------ tampering
TAMPER_QUERIES = (0, 13, 27)


def tamper_cases(info, proof):
    """[(label, proof bytes)]: one single-bit flip in every section before the queries and after them (caps, each open_*, each
    FRI cap, final polynomial, PoW witness, the public-input values where there are some) and, for queries 0, 13 and 27, in
    every leaf, count byte, sibling block and evaluation block.  The bit is the lowest one of the section's middle word (of
    the count byte), so the changed word stays canonical and, under Keccak, in range."""
    S = sections(info)
    out = []
    for name, (off, nbytes, kind) in S.items():
        m = re.match(r"q(\d+)_", name)
        if m and int(m.group(1)) not in TAMPER_QUERIES:
            continue
        if nbytes == 0 or name == "pi_count":
            continue
        b = bytearray(proof)
        b[off + (8 * (nbytes // 16) if kind == "words" else 0)] ^= 1
        out.append((name, bytes(b)))
    return out


def memoised(hasher):
    """The same pair of functions, each remembering the rows it has hashed: a tampered proof differs from the honest one in
    one place, so replaying many of them recomputes one Merkle path each (the numpy Keccak costs milliseconds per call)."""
    def wrap(fn):
        memo = {}

        def call(*arrays):
            arrays = [np.ascontiguousarray(a, dtype=np.uint64) for a in arrays]
            lead = arrays[0].shape[:-1]
            flat = [a.reshape(-1, a.shape[-1]) for a in arrays]
            keys = [b"".join(a[i].tobytes() for a in flat) for i in range(flat[0].shape[0])]
            miss = sorted({k: i for i, k in enumerate(keys) if k not in memo}.values())
            if miss:
                for i, row in zip(miss, np.asarray(fn(*[a[miss] for a in flat]), dtype=np.uint64)):
                    memo[keys[i]] = row
            return np.stack([memo[k] for k in keys]).reshape(lead + (4,))
        return call
    return tuple(wrap(f) for f in hasher)
