"""Compressed proofs, the cases: an independent compressor written from the layout of DESIGN.md section 8a, and the directed
inputs built from it.  Shared by tests/test_compress_host.py and tests/test_compress_cases_host.py (no GPU) and
tests/test_gpu_compress_directed.py.  Nothing here calls the library: a case is bytes plus the host reason strings that the
verdict order of section 8a allows for it, known from how the bytes were made.

  py_compress        (compressed bytes, {name: byte offset}) of a full proof at given query indices
  index_sweep        full proofs that differ in pow_witness only: other drawn indices, so other layouts, with the index check passing
  index_predicates   which of the layout code's branches a set of indices reaches
  malformed          (label, bytes, acceptable reasons) for malformed compressed proofs of one proof"""
import struct

import verify_layout

P = 0xFFFFFFFF00000001
ARITY_BITS, CAP_HEIGHT, Q = 4, 4, 28

TRUNCATED, TRAILING = "proof truncated", "trailing bytes in proof"
INDEX_RANGE, COUNT, INDICES = "query index out of range", "wrong sibling count in compressed proof", "query indices differ from the transcript"
PI_COUNT, NON_CANONICAL, HASH_RANGE = "wrong number of public inputs", "non-canonical field element", "hash word out of range"
POW, MERKLE_INITIAL, MERKLE_FRI = "Invalid proof-of-work witness.", "Invalid Merkle proof (initial tree).", "Invalid Merkle proof (FRI round)."


# ------------------------------------------------------------------------------------------------ independent compressor
def _body_info(info):
    k = info["num_public_inputs"]
    return dict(info, proof_bytes=info["proof_bytes"] - (8 + 8 * k if k else 0))


def kept_levels(leaves, q, depth):
    """The levels at which query q stores its sibling: the sibling is on no query's path, and no earlier query shares q's
    node at that level (which would have stored it already).  (A closed form of upstream's walk over a set of known nodes.)"""
    out = []
    for lvl in range(depth):
        node = leaves[q] >> lvl
        if any((x >> lvl) == node ^ 1 for x in leaves):
            continue
        if any((leaves[e] >> lvl) == node for e in range(q)):
            continue
        out.append(lvl)
    return out


def py_compress(info, proof, idx):
    """(compressed bytes, {name: byte offset}) for a full proof and its drawn query indices."""
    S = verify_layout.sections(_body_info(info))
    lde_bits, rounds, Q = info["degree_bits"] + 3, info["num_fri_rounds"], len(idx)
    prefix_end, tail_start = S["q0_init0_leaf"][0], S["final_poly"][0]
    out = bytearray(proof[:prefix_end])
    at = {"indices": len(out)}
    out += struct.pack("<%dI" % Q, *idx)

    def firsts(leaves):
        seen = {}
        for q, v in enumerate(leaves):
            seen.setdefault(v, q)
        return [seen[v] for v in sorted(seen)]

    def sib(name, lvl):
        off = S[name][0]
        return proof[off + 32 * lvl: off + 32 * lvl + 32]

    depth0 = lde_bits - CAP_HEIGHT
    for q in firsts(idx):
        kept = kept_levels(idx, q, depth0)
        for o in range(4):
            off, n, _ = S["q%d_init%d_leaf" % (q, o)]
            at["init_leaf_%d_%d" % (q, o)] = len(out)
            out += proof[off:off + n]
            at["init_count_%d_%d" % (q, o)] = len(out)
            out.append(len(kept))
            if kept:
                at["init_sib_%d_%d" % (q, o)] = len(out)
            for lvl in kept:
                out += sib("q%d_init%d_siblings" % (q, o), lvl)
    for r in range(rounds):
        leaves = [x >> (ARITY_BITS * (r + 1)) for x in idx]
        depth = lde_bits - ARITY_BITS * (r + 1) - CAP_HEIGHT
        for q in firsts(leaves):
            left_out = (idx[q] >> (ARITY_BITS * r)) & 15
            off = S["q%d_round%d_evals" % (q, r)][0]
            at["evals_%d_%d" % (r, q)] = len(out)
            for k in range(16):
                if k != left_out:
                    out += proof[off + 16 * k: off + 16 * k + 16]
            kept = kept_levels(leaves, q, depth)
            at["round_count_%d_%d" % (r, q)] = len(out)
            out.append(len(kept))
            if kept:
                at["round_sib_%d_%d" % (r, q)] = len(out)
            for lvl in kept:
                out += sib("q%d_round%d_siblings" % (q, r), lvl)
    at["final_poly"] = len(out)
    at["pow_witness"] = len(out) + (S["pow_witness"][0] - tail_start)
    if info["num_public_inputs"]:
        at["pi_values"] = at["pow_witness"] + 16
    out += proof[tail_start:]
    return bytes(out), at


def coset_collision(info, idx):
    """A pair of queries in the same coset of the last FRI round, at different positions within it."""
    r = info["num_fri_rounds"] - 1
    if r < 0:
        return None
    for a in range(len(idx)):
        for b in range(a + 1, len(idx)):
            if idx[a] >> (4 * r + 4) == idx[b] >> (4 * r + 4) and (idx[a] >> 4 * r) & 15 != (idx[b] >> 4 * r) & 15:
                return a, b
    return None


def _flip(word_bytes):
    v = struct.unpack("<Q", word_bytes)[0]
    w = v ^ 1 if v ^ 1 < P else v ^ 2
    return struct.pack("<Q", w)


def _put(c, off, b):
    return c[:off] + b + c[off + len(b):]


def written_indices(info, c):
    """the index table of a compressed proof"""
    return list(struct.unpack_from("<%dI" % Q, c, verify_layout.sections(_body_info(info))["q0_init0_leaf"][0]))


# ------------------------------------------------------------------------------------------------ index sets
def index_sweep(proof, info, n):
    """`n` full proofs that differ from `proof` in pow_witness alone (honest ^ k for k = 1, 2, ..., the values >= p left
    out).  The transcript draws other indices for each, and compression, which does not check the proof-of-work, lays each out
    at the indices it draws: well-formed compressed proofs whose written indices pass the index check."""
    off = verify_layout.sections(_body_info(info))["pow_witness"][0]
    honest = struct.unpack_from("<Q", proof, off)[0]
    out, k = [], 0
    while len(out) < n:
        k += 1
        if honest ^ k < P:
            out.append(_put(proof, off, struct.pack("<Q", honest ^ k)))
    return out


def index_predicates(idx, info):
    """{name: bool}: the branches of the layout code (CompressLayout / k_cmp_plan) that these query indices reach.
      a      a duplicate tree-0 index
      b      a twin (a later query with an earlier one's index) whose first occurrence is not the preceding query
      c, d   a tree-0 block that keeps no sibling / all `depth` siblings
    and per FRI round r
      e<r>   a coset reached at two different positions
      f<r>, g<r>   a coset block that keeps no sibling / all of the round tree's depth
      h<r>   (r >= 1) two distinct round-(r-1) cosets that fall in one round-r coset and were reached at the same position
             within their own cosets.  (Within the round-r coset two distinct round-(r-1) cosets ARE two different positions, so
             "the same position" can only be the position one round below.)"""
    lde_bits, rounds, n = info["degree_bits"] + 3, info["num_fri_rounds"], len(idx)
    depth0 = lde_bits - CAP_HEIGHT
    first = [idx.index(v) for v in idx]
    kept0 = [len(kept_levels(idx, q, depth0)) for q in range(n) if first[q] == q]
    out = {"a": len(set(idx)) < n, "b": any(first[q] < q - 1 for q in range(n)), "c": 0 in kept0, "d": depth0 in kept0}
    for r in range(rounds):
        leaves = [x >> (ARITY_BITS * (r + 1)) for x in idx]
        pos = [(x >> (ARITY_BITS * r)) & 15 for x in idx]
        depth = lde_bits - ARITY_BITS * (r + 1) - CAP_HEIGHT
        kept = [len(kept_levels(leaves, q, depth)) for q in range(n) if leaves.index(leaves[q]) == q]
        pairs = [(a, b) for a in range(n) for b in range(a + 1, n) if leaves[a] == leaves[b]]
        out["e%d" % r] = any(pos[a] != pos[b] for a, b in pairs)
        out["f%d" % r] = 0 in kept
        out["g%d" % r] = depth in kept
        if r >= 1:
            below = [(x >> (ARITY_BITS * (r - 1))) & 15 for x in idx]
            out["h%d" % r] = any(pos[a] != pos[b] and below[a] == below[b] for a, b in pairs)
    return out


def twin_read(info, idx, r):
    """(first query of a round-r coset, the position a later query of that coset is at) where the two differ, or None: the
    stored evaluation that the twin's fold check reads"""
    leaves = [x >> (ARITY_BITS * (r + 1)) for x in idx]
    pos = [(x >> (ARITY_BITS * r)) & 15 for x in idx]
    for b in range(len(idx)):
        a = leaves.index(leaves[b])
        if a != b and pos[a] != pos[b]:
            return a, pos[b]
    return None


# ------------------------------------------------------------------------------------------------ the layout, read back
class Layout:
    """The blocks of a compressed proof from py_compress's offset map, in byte order: per initial tree o the list of
    (leaf offset, leaf bytes, count offset, kept) and per FRI round the same with the 15 stored evaluations as the leaf."""

    def __init__(self, info, c, at):
        self.rounds = info["num_fri_rounds"]
        self.init = [[] for _ in range(4)]
        self.round = [[] for _ in range(self.rounds)]
        self.query = {}
        for key, off in sorted(at.items(), key=lambda kv: kv[1]):
            if key.startswith("init_leaf_"):
                q, o = map(int, key.split("_")[2:])
                cnt = at["init_count_%d_%d" % (q, o)]
                self.init[o].append((off, cnt - off, cnt, c[cnt]))
            elif key.startswith("evals_"):
                r, q = map(int, key.split("_")[1:])
                cnt = at["round_count_%d_%d" % (r, q)]
                self.round[r].append((off, cnt - off, cnt, c[cnt]))
                self.query[(r, q)] = off

    def trees(self):
        """[(name, blocks)] for the four initial trees and every round tree"""
        return [("init%d" % o, b) for o, b in enumerate(self.init)] + [("round%d" % r, b) for r, b in enumerate(self.round)]

    def count_offsets(self):
        """every count byte, in byte order"""
        return sorted(b[2] for _, blocks in self.trees() for b in blocks)

    def block_counts(self):
        """the count offsets of each block in byte order: four per initial block, one per round block"""
        out = [[self.init[o][i][2] for o in range(4)] for i in range(len(self.init[0]))]
        return out + [[b[2]] for blocks in self.round for b in blocks]

    @staticmethod
    def siblings(blocks):
        """byte offsets of the kept siblings of a tree's blocks, in byte order"""
        return [cnt + 1 + 32 * i for _, _, cnt, kept in blocks for i in range(kept)]


def layout_reason(info, b, idx):
    """What the shape and canonicality checks of section 8a say about the bytes `b` read as a compressed proof with the index
    table `idx` (which `b` holds): a reason string, or None where they pass.  Only what depends on the layout is restated:
    length, count bytes, public-input count, canonical words."""
    N = 1 << (info["degree_bits"] + 3)
    if any(x >= N for x in idx):
        return INDEX_RANGE
    k = info["num_public_inputs"]
    body = bytes(_body_info(info)["proof_bytes"]) + (struct.pack("<Q", k) + bytes(8 * k) if k else b"")
    ref, at = py_compress(info, body, idx)       # (the layout alone: a zero proof, the honest public-input count)
    if len(b) != len(ref):
        return TRUNCATED if len(b) < len(ref) else TRAILING
    L = Layout(info, ref, at)
    if any(b[o] != ref[o] for o in L.count_offsets()):
        return COUNT
    if k and b[at["pow_witness"] + 8: at["pow_witness"] + 16] != struct.pack("<Q", k):
        return PI_COUNT
    skip = set(L.count_offsets())
    spans, pos = [], 0          # the word runs: everything but the index table, the count bytes and the public-input count
    cuts = sorted(list(skip) + [at["indices"] + i for i in range(4 * len(idx))] + ([at["pow_witness"] + 8 + i for i in range(8)] if k else []))
    for cpos in cuts:
        if cpos > pos:
            spans.append((pos, cpos))
        pos = cpos + 1
    spans.append((pos, len(b)))
    for lo, hi in spans:
        assert (hi - lo) % 8 == 0
        if any(w >= P for w in struct.unpack_from("<%dQ" % ((hi - lo) // 8), b, lo)):
            return NON_CANONICAL
    return None


class Slot(bytes):
    """The content of a whole batch slot with a length of its own: the bytes past `length` are there to be ignored."""
    length = 0


def case_bytes(b):
    """(buffer, length) of a case's bytes"""
    return bytes(b), getattr(b, "length", len(b))


# ------------------------------------------------------------------------------------------------ malformed compressed proofs
def relaid_index_sets(info, idx):
    """[(label, idx')]: fixed index sets whose layouts the honest sets do not reach"""
    lde_bits = info["degree_bits"] + 3
    N, depth0 = 1 << lde_bits, lde_bits - CAP_HEIGHT
    a = idx[0]
    b = next(x for x in idx if x != a)
    base = (a >> 4) << 4
    pairs = [2 * (j * (N // 2) // 14) for j in range(14)]
    sets = [("all 0", [0] * Q), ("all N-1", [N - 1] * Q), ("0..27", list(range(Q))), ("27..0", list(range(Q))[::-1]),
            ("14 sibling pairs", [v for e in pairs for v in (e, e + 1)]), ("[a, b] * 14", [a, b] * 14),
            ("one round-0 coset", [base + (k & 15) for k in range(Q)]), ("one per cap subtree", [(k & 15) << depth0 for k in range(Q)]),
            ("reversed", list(idx)[::-1])]
    assert all(len(s) == Q and max(s) < N for _, s in sets)
    return [(lbl, s) for lbl, s in sets if s != list(idx)]


def malformed(info, proof, idx, base=None, pow_fails=None):
    """[(label, bytes, want)]: malformed compressed proofs of the full proof `proof` with drawn indices `idx`; `want` is the set
    of host reasons section 8a's order allows, by construction.  `bytes` is a Slot where the case has a length of its own.
    `base`: the reason an untouched compressed proof of this proof gets where that is not "" (the oracle's public-input proofs
    fail the proof-of-work): it stands in for every verdict behind canonicality.  `pow_fails(bytes) -> bool` says whether the
    proof-of-work check of these compressed bytes fails: with it, the case that needs such a witness is searched and included."""
    idx = list(idx)
    c, at = py_compress(info, proof, idx)
    L = Layout(info, c, at)
    N, stride, prefix, k = 1 << (info["degree_bits"] + 3), info["proof_bytes"], at["indices"], info["num_public_inputs"]
    keccak = info.get("hasher", "poseidon") == "keccak"
    assert len(c) + 1 <= stride
    bad_words = (("p", struct.pack("<Q", P)), ("2^64-1", struct.pack("<Q", 2 ** 64 - 1)))
    out = []

    def late(*reasons):
        return {base} if base else set(reasons)

    def add(label, b, *want):
        out.append((label, b, set(want)))

    def table(ix):
        return _put(c, prefix, struct.pack("<%dI" % Q, *ix))

    def slot(content, length):
        s = Slot(content)
        s.length = length
        return s

    # ---- lengths
    add("length 0", b"", TRUNCATED)
    add("prefix + 4Q - 1", c[:prefix + 4 * Q - 1], TRUNCATED)
    add("prefix + 4Q", c[:prefix + 4 * Q], TRUNCATED)
    add("len - 1", c[:-1], TRUNCATED)
    add("len + 1", c + b"\0", TRAILING)
    filled = c + b"\xff" * (stride - len(c))
    out.append(("0xFF past the honest length", slot(filled, len(c)), late("")))
    add("0xFF up to a length of the stride", slot(filled, stride), TRAILING)

    # ---- index table, the rest left as it is
    for lbl, q, v in (("index 0 = N", 0, N), ("index 27 = N", Q - 1, N), ("index 13 = 0xFFFFFFFF", 13, 0xFFFFFFFF)):
        ix = list(idx)
        ix[q] = v
        add(lbl, table(ix), INDEX_RANGE)
    qa, qb = next((x, y) for x in range(Q) for y in range(Q) if idx[x] != idx[y])
    sw = list(idx)
    sw[qa], sw[qb] = sw[qb], sw[qa]
    x1 = list(idx)
    x1[5] ^= 1
    for lbl, ix in (("indices %d and %d swapped" % (qa, qb), sw), ("index 5 ^ 1", x1)):
        b = table(ix)
        r = layout_reason(info, b, ix)
        out.append((lbl, b, {r} if r else late(INDICES)))

    # ---- re-laid-out index sets: shape-valid for idx', which the transcript does not draw
    relaid = relaid_index_sets(info, idx)
    for lbl, ix in relaid:
        b, _ = py_compress(info, proof, ix)
        assert len(b) <= stride and layout_reason(info, b, ix) is None, lbl
        out.append(("re-laid-out: " + lbl, b, late(INDICES)))

    # ---- count bytes
    blocks = L.block_counts()
    for o in L.count_offsets():
        add("count byte @%d + 1" % o, _put(c, o, bytes([(c[o] + 1) & 255])), COUNT)
    for name, blk in (("first", blocks[0]), ("last", blocks[-1])):
        for o in blk:
            for v in (0, 255):
                if c[o] != v:
                    add("count byte @%d of the %s block = %d" % (o, name, v), _put(c, o, bytes([v])), COUNT)

    # ---- non-canonical words
    words = [("prefix first", 0), ("prefix last", prefix - 8), ("final_poly[0]", at["final_poly"]), ("pow_witness", at["pow_witness"])]
    if k:
        words += [("pi value first", at["pi_values"]), ("pi value last", at["pi_values"] + 8 * (k - 1))]
    for name, blks in L.trees():
        for which, (off, n, cnt, kept) in (("first", blks[0]), ("last", blks[-1])):
            words += [("%s %s block first word" % (name, which), off), ("%s %s block last word" % (name, which), off + n - 8)]
        sibs = Layout.siblings(blks)
        if sibs:
            for which, s in (("first", sibs[0]), ("last", sibs[-1])):
                words += [("%s %s kept sibling first word" % (name, which), s), ("%s %s kept sibling last word" % (name, which), s + 24)]
    seen = set()
    for name, off in words:
        if off in seen:
            continue
        seen.add(off)
        for vn, v in bad_words:
            add("%s = %s" % (name, vn), _put(c, off, v), NON_CANONICAL)

    # ---- public-input count
    if k:
        o = at["pow_witness"] + 8
        for v in (k - 1, k + 1, 0):
            if v != k:
                add("public-input count %d" % v, _put(c, o, struct.pack("<Q", v)), PI_COUNT)

    # ---- canonical flips: the class each must get
    def flipped(off, src=None):
        src = c if src is None else src
        return _put(src, off, _flip(src[off:off + 8]))

    for o in range(4):
        first, last = L.init[o][0], L.init[o][-1]
        out.append(("init%d leaf flip, first block first word" % o, flipped(first[0]), late(MERKLE_INITIAL)))
        out.append(("init%d leaf flip, last block last word" % o, flipped(last[0] + last[1] - 8), late(MERKLE_INITIAL)))
        sibs = Layout.siblings(L.init[o])
        if sibs:
            out.append(("init%d kept sibling flip" % o, flipped(sibs[0]), late(MERKLE_INITIAL)))
            out.append(("init%d last kept sibling flip" % o, flipped(sibs[-1] + 16), late(MERKLE_INITIAL)))
    for r in range(L.rounds):
        first, last = L.round[r][0], L.round[r][-1]
        out.append(("round%d evaluation flip, first block" % r, flipped(first[0]), late(MERKLE_FRI)))
        out.append(("round%d evaluation flip, last block last word" % r, flipped(last[0] + last[1] - 8), late(MERKLE_FRI)))
        tw = twin_read(info, idx, r)
        if tw:   # the first query of the coset fails its tree before the twin fails its fold
            q, pos = tw
            left_out = (idx[q] >> (ARITY_BITS * r)) & 15
            off = L.query[(r, q)] + 16 * (pos if pos < left_out else pos - 1)
            out.append(("round%d evaluation flip where a twin reads it" % r, flipped(off), late(MERKLE_FRI)))
        sibs = Layout.siblings(L.round[r])
        if sibs:
            out.append(("round%d kept sibling flip" % r, flipped(sibs[0] + 8), late(MERKLE_FRI)))
    out.append(("final_poly flip", flipped(at["final_poly"] + 8), {POW, INDICES}))
    out.append(("pow_witness flip", flipped(at["pow_witness"]), {POW, INDICES}))

    # ---- two faults at once: the verdict of section 8a's order
    o = L.count_offsets()[-1]
    two = _put(c, o, bytes([(c[o] + 1) & 255]))
    add("count byte and non-canonical leaf", _put(two, L.init[1][0][0], bad_words[0][1]), COUNT)
    add("len + 1 and non-canonical prefix word", _put(c, 8, bad_words[1][1]) + b"\0", TRAILING)
    all_sibs = [s for _, blks in L.trees() for s in Layout.siblings(blks)]
    if all_sibs:
        add("non-canonical kept sibling and flipped pow_witness", flipped(at["pow_witness"], _put(c, all_sibs[-1], bad_words[0][1])), NON_CANONICAL)
    rl, rat = py_compress(info, proof, relaid[-1][1])
    if L.rounds:
        ev = next(v for key, v in rat.items() if key.startswith("evals_"))
        add("non-canonical stored evaluation, re-laid-out", _put(rl, ev + 8, bad_words[0][1]), NON_CANONICAL)
    if pow_fails:
        honest = struct.unpack_from("<Q", c, at["pow_witness"])[0]
        for v in range(1, 200):
            if honest ^ v < P:
                b = _put(rl, rat["pow_witness"], struct.pack("<Q", honest ^ v))
                if pow_fails(b):
                    add("failing pow_witness, re-laid-out", b, POW)
                    break
        else:
            raise AssertionError("no pow_witness within 200 fails the proof-of-work check")
    if k:
        two = _put(c, at["pow_witness"] + 8, struct.pack("<Q", k + 1))
        add("public-input count and non-canonical public-input value", _put(two, at["pi_values"], bad_words[0][1]), PI_COUNT)

    # ---- Keccak: a hash word out of its range, with the precedence of canonicality
    if keccak:
        assert all_sibs

        def top(src, off):
            assert src[off + 7] == 0
            return _put(src, off + 7, b"\x80")     # >= 2^56 and below p

        sib, cap = all_sibs[0], 32 * 5
        add("kept sibling word out of range", top(c, sib), HASH_RANGE)
        add("cap word out of range", top(c, cap), HASH_RANGE)
        add("kept sibling word = p", _put(c, sib, bad_words[0][1]), NON_CANONICAL)
        add("cap word = p", _put(c, cap, bad_words[0][1]), NON_CANONICAL)
        add("kept sibling word = p and cap word out of range", top(_put(c, sib, bad_words[0][1]), cap), NON_CANONICAL)
        add("cap word = p and kept sibling word out of range", top(_put(c, cap, bad_words[0][1]), sib), NON_CANONICAL)
    assert len({lbl for lbl, _, _ in out}) == len(out)
    return out
