"""Circuits at the edges of the lookup argument and of the row count, and the one checker every whole proof of them is held
to.  Shared by tests/test_lookup_edges_host.py (no GPU), tests/test_gpu_lookup_edges.py and tests/test_gpu_degree_ladder.py.

Makers return (data, pws, ...).  A maker fixes nothing about the shape it produces: the tests assert degree_bits, num_luts,
num_fri_rounds and the row counts, so that a change in the builder that moves a case off its edge fails the case."""
import random

import blob_reader
import proof_ref
import verify_layout

P = 0xFFFFFFFF00000001
LU_SLOTS, LUT_SLOTS = 40, 26      # looking slots of a LookupGate row, table slots of a LookupTableGate row


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------- arithmetic chain
def chain_ops(b, x, y, n_ops):
    """A dependent chain of arithmetic operations: one row's worth of padding per operation or so (the sizes are asserted)."""
    acc = x
    for k in range(n_ops):
        acc = b.mul_const_add(k + 3, acc, y) if k & 1 else b.mul(acc, y)
    return acc


def chain_value(xv, yv, n_ops):
    acc = xv
    for k in range(n_ops):
        acc = ((k + 3) * acc + yv) % P if k & 1 else acc * yv % P
    return acc


def chain_witness(pkg, pw, targets, n_ops, r):
    x, y, out = targets
    xv, yv = r.randrange(P), r.randrange(P)
    pw.set_target(x, xv)
    pw.set_target(y, yv)
    pw.set_target(out, chain_value(xv, yv, n_ops))


def chain(pkg, n_ops, seeds, hasher="poseidon"):
    """No lookup table, routed wires only: the chain sets the number of rows, its end value is asserted in the witness."""
    b = pkg.CircuitBuilder(hasher=hasher)
    x, y = b.add_virtual_target(), b.add_virtual_target()
    out = chain_ops(b, x, y, n_ops)
    data = b.build()
    pws = []
    for seed in seeds:
        pw = pkg.PartialWitness()
        chain_witness(pkg, pw, (x, y, out), n_ops, random.Random(seed))
        pws.append(pw)
    return data, pws


# ---------------------------------------------------------------------------------------------- custom tables
def first_match(table):
    """input -> output as the witness generator resolves it: the first pair with that input wins"""
    out = {}
    for i, o in table:
        out.setdefault(i, o)
    return out


class TableShape:
    """What a table case needs to recompute values and to assert its shape: per table the input and output targets, the
    expected outputs per witness (first match), and the number of gates before build() (the rows that belong to no table and
    precede the first LookupGate row)."""

    def __init__(self):
        self.ins, self.outs, self.want, self.gates_before = [], [], [], 0

    def out_targets(self):
        return [t for outs in self.outs for t in outs]

    def want_values(self, w):
        return [v for per_table in self.want[w] for v in per_table]


def table_circuit(pkg, tables, picks, n_ops=0, seed=0):
    """`tables`: a list of pair lists.  picks[w][k]: the inputs witness w looks up in table k (the count per table is the
    circuit's: every witness gives as many).  The outputs are left to the generator.  n_ops > 0 puts an arithmetic chain in
    front of the lookup rows.  Returns (data, pws, TableShape)."""
    counts = [len(p) for p in picks[0]]
    assert all([len(p) for p in w] == counts for w in picks) and len(counts) == len(tables)
    b = pkg.CircuitBuilder()
    sh = TableShape()
    ch = None
    if n_ops:
        x, y = b.add_virtual_target(), b.add_virtual_target()
        ch = (x, y, chain_ops(b, x, y, n_ops))
    for table, cnt in zip(tables, counts):
        lut = b.add_lookup_table_from_pairs(table)
        ins = [b.add_virtual_target() for _ in range(cnt)]
        sh.ins.append(ins)
        sh.outs.append([b.add_lookup_from_index(t, lut) for t in ins])
    sh.gates_before = b.num_gates()
    data = b.build()
    maps = [first_match(t) for t in tables]
    pws = []
    for w, per_table in enumerate(picks):
        pw = pkg.PartialWitness()
        if ch:
            chain_witness(pkg, pw, ch, n_ops, random.Random(1000 * seed + w))
        for ins, vals in zip(sh.ins, per_table):
            for t, v in zip(ins, vals):
                pw.set_target(t, v)
        sh.want.append([[m[v] for v in vals] for m, vals in zip(maps, per_table)])
        pws.append(pw)
    return data, pws, sh


def lookup_rows(data):
    """[(LookupGate rows, LookupTableGate rows, first LookupGate row, last LookupTableGate row)] per table, from the blob"""
    B = blob_reader.Blob(data.blob)
    return [(int(last_lut - last_lu), int(first_lut - last_lut + 1), int(last_lu), int(first_lut)) for last_lu, last_lut, first_lut in B.lookup_rows]


def assert_table_shape(data, sh, tables, counts):
    """The rows that make the case the edge it claims to be: per table ceil(lookups / 40) LookupGate rows and ceil(entries / 26)
    LookupTableGate rows, laid out behind one another from the row after the gates the builder held before build() (the
    PublicInputGate takes that row); between two tables one NoopGate."""
    rows = lookup_rows(data)
    assert len(rows) == len(tables) == data.info["num_luts"]
    at = sh.gates_before + 1
    for (lu, lut, first_lu, last_lut_row), table, cnt in zip(rows, tables, counts):
        assert lu == ceil_div(cnt, LU_SLOTS), (lu, cnt)
        assert lut == ceil_div(len(table), LUT_SLOTS), (lut, len(table))
        assert first_lu == at, (first_lu, at)
        assert last_lut_row == at + lu + lut - 1
        at += lu + lut + 1
    assert at < 1 << data.info["degree_bits"]
    return rows


# ---------------------------------------------------------------------------------------------- PoseidonGate rows
def hash_rows(pkg, n_perm, seeds):
    """A chain of hash_n_to_m_no_pad calls of 8 inputs and 8 outputs: one PoseidonGate row each, all 135 wire columns live, the
    two-walk quotient.  The end of the chain is asserted in the witness from the native hash."""
    b = pkg.CircuitBuilder()
    first = b.add_virtual_target_arr(8)
    h = first
    for _ in range(n_perm):
        h = b.hash_n_to_m_no_pad(h, 8)
    gates = b.num_gates()
    data = b.build()
    pws = []
    for seed in seeds:
        r = random.Random(seed)
        v = [r.randrange(P) for _ in range(8)]
        pw = pkg.PartialWitness()
        pw.set_target_arr(first, v)
        for _ in range(n_perm):
            v = pkg.poseidon_native.hash_n_to_m_no_pad(v, 8)
        pw.set_target_arr(h, v)
        pws.append(pw)
    return data, pws, gates


# ---------------------------------------------------------------------------------------------- the checker
def host_code(pkg, data, proof, vd):
    """the VERIFY_* code of the host verifier's reason for this proof"""
    try:
        data.verify(proof, vd)
        return pkg.VERIFY_OK
    except pkg.P2Error as e:
        return pkg.VERIFY_REASONS[str(e).split("verify failed: ", 1)[1]]


def flipped_column_byte(info, proof, which=0):
    """The proof with one byte changed inside an opened lookup column (open_lookup_zs) where the circuit has one, else inside
    an opened Z column (open_zs): the lowest byte of the section's middle word, so the word stays canonical."""
    S = verify_layout.sections(info)
    off, nbytes, _ = S["open_lookup_zs"] if S["open_lookup_zs"][1] else S["open_zs"]
    b = bytearray(proof)
    b[off + 8 * (nbytes // 16)] ^= 1 << which
    return bytes(b)


def reference_holds(pkg, data, vd, proof, hasher=None):
    """host verifier and the Python replay (with the vanishing identity) on one proof"""
    data.verify(proof, vd)
    bad = proof_ref.replay(dict(data.info), vd, proof, hasher or proof_ref.poseidon_hasher(), blob=data.blob)
    assert bad is None, bad


def gpu_proofs_hold(gpu, orc, data, pws, oracle=True, hasher=None):
    """prove_batch(pws): all statuses 0, pairwise different proofs; with `oracle` each equal to the CPU oracle's proof byte for
    byte and the verifier data equal to the oracle's; every proof accepted by the host verifier, the GPU verifier and the
    Python replay (vanishing identity included); compress_batch equal to the host's compress and decompress_batch back to the
    proof; and one proof with a byte flipped inside an opened lookup or Z column judged alike by host and GPU verifier.
    `hasher`: the replay's tree hasher (default Poseidon).  Returns the proofs."""
    info = dict(data.info)
    proofs, status = data.prove_batch(pws)
    assert status == [0] * len(pws), status
    assert len({bytes(p) for p in proofs}) == len(pws)     # a batch stride of zero could not pass
    vd = data.verifier_data()
    if oracle:
        oc = orc.OracleCircuit(data.blob)
        assert vd == oc.verifier_data()
        for i, (pw, proof) in enumerate(zip(pws, proofs)):
            ost, ref = oc.prove(pw.map)
            assert ost == 0
            assert proof == ref, "proof %d differs from the oracle's" % i
    hasher = proof_ref.memoised(hasher or proof_ref.poseidon_hasher())
    for i, proof in enumerate(proofs):
        data.verify(proof)
        bad = proof_ref.replay(info, vd, proof, hasher, blob=data.blob)
        assert bad is None, (i, bad)
    assert data.verify_batch(proofs) == [gpu.VERIFY_OK] * len(proofs)
    packed, cst = data.compress_batch(proofs)
    assert cst == [gpu.VERIFY_OK] * len(proofs)
    assert packed == [data.compress(p) for p in proofs]
    back, dst = data.decompress_batch(packed)
    assert dst == [gpu.VERIFY_OK] * len(proofs) and back == proofs
    bad = flipped_column_byte(info, proofs[-1])
    want = host_code(gpu, data, bad, vd)
    assert want != gpu.VERIFY_OK
    assert data.verify_batch([proofs[0], bad]) == [gpu.VERIFY_OK, want]
    return proofs


# ---------------------------------------------------------------------------------------------- the lookup cases
def spread_table(entries, mul):
    """`entries` pairs with distinct inputs 3 i + 1 (holes in between) and outputs mul i + 1; tables of different `mul` differ"""
    return [((3 * i + 1) & 0xFFFF, (mul * i + 1) & 0xFFFF) for i in range(entries)]


def random_picks(tables, counts, seed):
    r = random.Random(seed)
    return [[r.choice(t)[0] for _ in range(c)] for t, c in zip(tables, counts)]


def _one_table(entries, lookups, degree_bits, rounds=0, n_ops=0):
    t = [spread_table(entries, 7)]
    return dict(tables=t, picks=[random_picks(t, [lookups], 10 * entries + w) for w in range(3)], n_ops=n_ops, degree_bits=degree_bits, rounds=rounds)


def _hot():
    t = spread_table(26, 7)
    return dict(tables=[t], picks=[[[t[-1][0]] * 2000], [[t[0][0]] * 2000], random_picks([t], [2000], 5)], n_ops=0, degree_bits=6, rounds=1)


SIX_ENTRIES, SIX_LOOKUPS = (1, 5, 26, 27, 256, 300), (1, 40, 41, 79, 80, 121)


def _six(n_ops, degree_bits, rounds):
    t = [spread_table(e, 5 + 2 * k) for k, e in enumerate(SIX_ENTRIES)]
    return dict(tables=t, picks=[random_picks(t, SIX_LOOKUPS, 60 + w) for w in range(3)], n_ops=n_ops, degree_bits=degree_bits, rounds=rounds)


def _dense():
    t = [(i, (5 * i + 3) & 0xFFFF) for i in range(1025 * LUT_SLOTS - LUT_SLOTS + 1)]
    return dict(tables=[t], picks=[[[0, 26624, 13000]], [[26624, 1, 2]], [[26623, 26, 25]]], n_ops=0, degree_bits=11, rounds=2)


# name -> tables, picks of three witnesses, n_ops, and the shape the case must have.  "one" has a single possible pick, so one
# arithmetic operation (n_ops = 1) tells its three witnesses apart.
LOOKUP_CASES = {
    "one": lambda: _one_table(1, 1, 3, n_ops=1),
    "slots_minus_1": lambda: _one_table(25, 39, 3),
    "slots_exact": lambda: _one_table(26, 40, 3),
    "slots_plus_1": lambda: _one_table(27, 41, 3),
    "two_rows": lambda: _one_table(52, 80, 3),
    "two_rows_plus_1": lambda: _one_table(53, 81, 4),
    "hot": _hot,
    "scan_1024": lambda: _one_table(26, 40920, 11, rounds=2),
    "scan_1025": lambda: _one_table(26, 40921, 11, rounds=2),
    "table_scan": _dense,
    "extremes": lambda: dict(tables=[[(0, 0), (0xFFFF, 0xFFFF)]], picks=[[[0, 0xFFFF, 0]], [[0xFFFF, 0xFFFF, 0]], [[0, 0, 0]]], n_ops=0,
                             degree_bits=3, rounds=0),
    "sparse_repeated": lambda: dict(tables=[[(1, 2), (1, 3), (4, 5), (4, 5)]], picks=[[[1, 4, 1]], [[4, 1, 4]], [[4, 4, 1]]], n_ops=0,
                                    degree_bits=3, rounds=0),
    "six": lambda: _six(0, 6, 1),
    "six_with_rows_around": lambda: _six(300, 8, 1),
    "slots_plus_1_with_rows_around": lambda: _one_table(27, 41, 6, rounds=1, n_ops=90),
}


def lookup_case(pkg, name):
    """(data, pws, TableShape, case dict) of a LOOKUP_CASES entry, its shape asserted"""
    case = LOOKUP_CASES[name]()
    data, pws, sh = table_circuit(pkg, case["tables"], case["picks"], case["n_ops"], seed=len(name))
    counts = [len(p) for p in case["picks"][0]]
    assert data.info["degree_bits"] == case["degree_bits"], data.info
    assert data.info["num_fri_rounds"] == case["rounds"], data.info
    assert data.info["num_luts"] == len(case["tables"])
    case["rows"] = assert_table_shape(data, sh, case["tables"], counts)
    case["counts"] = counts
    return data, pws, sh, case


MISS_TABLE = [(1, 2), (4, 5), (7, 8)]
MISS_VALUES = (2, 65537, P - 1)     # a hole; 65537 = 1 mod 2^16 and p - 1 = 0 mod 2^16: neither may alias a 16-bit entry


def miss_circuit(pkg, value):
    """One lookup on MISS_TABLE and three witnesses: 1, `value` (not in the table), 7."""
    data, pws, sh = table_circuit(pkg, [MISS_TABLE], [[[1]], [[4]], [[7]]])
    assert (data.info["degree_bits"], data.info["num_luts"], data.info["num_fri_rounds"]) == (3, 1, 0)
    assert_table_shape(data, sh, [MISS_TABLE], [1])
    pws[1].map[sh.ins[0][0]] = value
    return data, pws, sh


def build_refusal(pkg, which):
    """The builder with "seventh": seven tables, each looked up once; "unused": two tables, the second never looked up.
    build() on it must raise."""
    b = pkg.CircuitBuilder()
    n = 7 if which == "seventh" else 2
    for k in range(n):
        lut = b.add_lookup_table_from_pairs([(k, k + 1)])
        if which == "seventh" or k == 0:
            b.add_lookup_from_index(b.add_virtual_target(), lut)
    return b


# ---------------------------------------------------------------------------------------------- the vanishing identity alone
VANISHING_CASES = ("slots_plus_1", "extremes", "sparse_repeated", "six", "table_scan")


def vanishing_lookup_sweep(data):
    """(info, vanishing_ref.Circuit, cases, Python's verdict on each) for the hooks behind tests/vanishing_cases.py: an opening
    set that tests/vanishing_ref.py alone makes valid for this circuit, then every single-coordinate perturbation of the
    opened lookup polynomials (at zeta and at g zeta) and of the constants (the lookup selectors among them) with the valid set
    again after every eighth, so that no kernel can read one buffer for the whole batch."""
    import vanishing_cases as VC
    import vanishing_ref as V
    info = dict(data.info)
    circ = V.Circuit(data.blob, info)
    base = VC.solved("", circ, "random", 100)
    cases = [base, VC.solved("", circ, P - 1, 7)]
    for k, c in enumerate(c for c in VC.sweep(circ, base) if c.label.startswith(("lookup_zs", "constants"))):
        cases.append(c)
        if k % 8 == 7:
            cases.append(base)
    want = [VC.python_verdict(circ, c) for c in cases]
    assert want[:2] == [V.HOLDS] * 2 and want.count(V.FAILS) >= 28, want
    return info, circ, cases, want
