"""TEST INFRASTRUCTURE (oracle): an independent restatement, in plain Python, of (1) the slice of plonky2's `CircuitBuilder`
that the reference's AES gadgets call, (2) those gadgets themselves, and (3) witness generation for the resulting circuit.

Nothing here reads the product's circuit blob or shares code with `plonky2-aes_amd/csrc/` (builder.h, aes_gadgets.h): the
product's builder compiles `AesGcmTarget::build` into gate rows, a constants matrix, a sigma permutation and a witness
program; this file derives the same four things again, straight from the reference's Rust (file:line cited per function)
and from plonky2's published builder algorithm, so that tests/test_independent_builder.py can hold the product to them.
plonky2 itself (git dependency of /root/reference/Cargo.toml:12, un-vendored) is absent: the builder half restates its
published algorithm (plonk/circuit_builder.rs, gadgets/arithmetic.rs, gadgets/lookup.rs, gates/selectors.rs,
plonk/permutation_argument.rs, gates/lookup.rs, gates/lookup_table.rs) -- parity with real plonky2 stays unpinned.

Only tests/ may import this module.
"""
P = 0xFFFFFFFF00000001
NUM_WIRES, NUM_ROUTED, NUM_CONSTANTS, MAX_QUOTIENT_DEGREE_FACTOR = 135, 80, 2, 8   # standard_recursion_config
UNUSED = 0xFFFFFFFF
MULTIPLICATIVE_GROUP_GENERATOR = 14293326489335486720      # GoldilocksField
POWER_OF_TWO_GENERATOR = pow(MULTIPLICATIVE_GROUP_GENERATOR, (P - 1) >> 32, P)   # = 7277203076849721926, order 2^32


# --------------------------------------------------------------------------------------------------- Keccak-256
def keccak256(data: bytes) -> bytes:
    """Original Keccak (pad 0x01), rate 136: what `keccak_hash::keccak` computes for LookupGate::lut_hash."""
    RC, R = [], 1
    for _ in range(24):
        c = 0
        for j in range(7):
            R = ((R << 1) ^ ((R >> 7) * 0x71)) & 0xFF
            if R & 2:
                c ^= 1 << ((1 << j) - 1)
        RC.append(c)
    rot = [[0] * 5 for _ in range(5)]
    x, y = 1, 0
    for t in range(24):
        rot[x][y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    M = (1 << 64) - 1
    rol = lambda v, s: ((v << s) | (v >> (64 - s))) & M if s else v
    st = [[0] * 5 for _ in range(5)]
    msg = bytearray(data) + b"\x01"
    while len(msg) % 136:
        msg.append(0)
    msg[-1] |= 0x80
    for off in range(0, len(msg), 136):
        for i in range(17):
            st[i % 5][i // 5] ^= int.from_bytes(msg[off + 8 * i: off + 8 * i + 8], "little")
        for rnd in range(24):
            C = [st[x][0] ^ st[x][1] ^ st[x][2] ^ st[x][3] ^ st[x][4] for x in range(5)]
            D = [C[(x - 1) % 5] ^ rol(C[(x + 1) % 5], 1) for x in range(5)]
            st = [[st[x][y] ^ D[x] for y in range(5)] for x in range(5)]
            B = [[0] * 5 for _ in range(5)]
            for x in range(5):
                for y in range(5):
                    B[y][(2 * x + 3 * y) % 5] = rol(st[x][y], rot[x][y])
            st = [[B[x][y] ^ ((~B[(x + 1) % 5][y]) & B[(x + 2) % 5][y]) for y in range(5)] for x in range(5)]
            st[0][0] ^= RC[rnd]
    return b"".join(st[i % 5][i // 5].to_bytes(8, "little") for i in range(4))


# --------------------------------------------------------------------------------------------------- targets
# virtual target v -> v (>= 0); routed or advice wire (row, column) -> -(row * NUM_WIRES + column) - 1
def wire(row, col):
    return -(row * NUM_WIRES + col) - 1


def is_wire(t):
    return t < 0


def wire_rc(t):
    return divmod(-t - 1, NUM_WIRES)


class GateType:
    """A gate *type* as plonky2's GateRef sees it: equal ids are one gate; `gates` is sorted by (degree, id)."""

    def __init__(self, name, ident, degree, num_constraints):
        self.name, self.id, self.degree, self.num_constraints = name, ident, degree, num_constraints


def lut_hash(table):
    # gates/lookup.rs `new_from_table`: keccak over the pairs, each as (input u16 LE, output u16 LE)
    return keccak256(b"".join(i.to_bytes(2, "little") + o.to_bytes(2, "little") for i, o in table))


def debug_bytes(h):
    return "[" + ", ".join(str(b) for b in h) + "]"            # Rust `{:?}` of [u8; 32]


NOOP = GateType("noop", "NoopGate", 0, 0)
CONSTANT = GateType("constant", "ConstantGate { num_consts: 2 }", 1, 2)
PUBLIC_INPUT = GateType("public_input", "PublicInputGate", 1, 4)
ARITHMETIC = GateType("arithmetic", "ArithmeticGate { num_ops: 20 }", 3, 20)
POSEIDON = GateType("poseidon", "PoseidonGate(PhantomData<plonky2_field::goldilocks_field::GoldilocksField>)<WIDTH=12>", 7, 123)
LU_SLOTS, LUT_SLOTS, ARITH_OPS = NUM_ROUTED // 2, NUM_ROUTED // 3, NUM_ROUTED // 4
# PoseidonGate wires (gates/poseidon.rs): 12 inputs | 12 outputs | swap | 4 deltas | S-box inputs of full rounds 1..3 | of the
# 22 partial rounds | of the last 4 full rounds
PG_IN, PG_OUT, PG_SWAP, PG_DELTA, PG_FULL0, PG_PARTIAL, PG_FULL1 = 0, 12, 24, 25, 29, 65, 87


class Builder:
    def __init__(self):
        self.num_virtual = 0
        self.rows = []                 # [GateType, [constants]]
        self.copies = []               # (target, target)
        self.const_to_target, self.target_to_const = {}, {}
        self.arith_results = {}        # BaseArithmeticOperation -> result
        self.free_slots = {}           # (gate id, params) -> (row, next slot)        `current_slots`
        self.luts, self.lut_lookups, self.lookup_rows = [], [], []
        self.constant_generators = []  # (row, index) of ConstantGate cells not yet bound to a constant
        self.generators = []           # witness generators, tuples tagged by kind

    # ---- plonk/circuit_builder.rs
    def add_virtual_target(self):
        self.num_virtual += 1
        return self.num_virtual - 1

    def constant(self, c):
        c %= P
        t = self.const_to_target.get(c)
        if t is None:
            t = self.add_virtual_target()
            self.const_to_target[c] = t
            self.target_to_const[t] = c
        return t

    def zero(self): return self.constant(0)
    def one(self): return self.constant(1)
    def connect(self, x, y): self.copies.append((x, y))
    def num_gates(self): return len(self.rows)

    def add_gate(self, gtype, constants=()):
        self.rows.append([gtype, list(constants)])
        row = len(self.rows) - 1
        if gtype is CONSTANT:          # `extra_constant_wires`: (constant index i, wire i)
            self.constant_generators += [(row, 0), (row, 1)]
        return row

    def find_slot(self, gtype, num_slots, params, constants):
        key = (gtype.id, tuple(params))
        got = self.free_slots.get(key)
        row, slot = got if got else (self.add_gate(gtype, constants), 0)
        if slot == num_slots - 1:
            self.free_slots.pop(key, None)
        else:
            self.free_slots[key] = (row, slot + 1)
        return row, slot

    # ---- gadgets/arithmetic.rs
    def arithmetic(self, c0, c1, m0, m1, addend):
        c0 %= P
        c1 %= P
        special = self._arithmetic_special_cases(c0, c1, m0, m1, addend)
        if special is not None:
            return special
        op = (c0, c1, m0, m1, addend)
        if op in self.arith_results:
            return self.arith_results[op]
        row, i = self.find_slot(ARITHMETIC, ARITH_OPS, (c0, c1), (c0, c1))
        w = [wire(row, 4 * i + k) for k in range(4)]          # multiplicand_0, multiplicand_1, addend, output
        self.connect(m0, w[0])
        self.connect(m1, w[1])
        self.connect(addend, w[2])
        self.generators.append(("arith", c0, c1, w[0], w[1], w[2], w[3]))
        self.arith_results[op] = w[3]
        return w[3]

    def _arithmetic_special_cases(self, c0, c1, m0, m1, addend):
        zero = self.zero()
        k0, k1, ka = self.target_to_const.get(m0), self.target_to_const.get(m1), self.target_to_const.get(addend)
        first_zero = c0 == 0 or m0 == zero or m1 == zero
        second_zero = c1 == 0 or addend == zero
        first_const = 0 if first_zero else (k0 * k1 * c0 % P if k0 is not None and k1 is not None else None)
        second_const = 0 if second_zero else (ka * c1 % P if ka is not None else None)
        if first_const is not None and second_const is not None:
            return self.constant(first_const + second_const)
        if first_zero and c1 == 1:
            return addend
        if second_zero:
            if k0 is not None and k0 * c0 % P == 1:
                return m1
            if k1 is not None and k1 * c0 % P == 1:
                return m0
        return None

    def mul_const_add(self, c, x, y): return self.arithmetic(c, 1, self.one(), x, y)      # c * 1 * x + y
    def add(self, x, y): return self.arithmetic(1, 1, x, self.one(), y)                   # 1 * x * 1 + y
    def sub(self, x, y): return self.arithmetic(1, P - 1, x, self.one(), y)
    def mul(self, x, y): return self.arithmetic(1, 0, x, y, x)
    def mul_sub(self, x, y, z): return self.arithmetic(1, P - 1, x, y, z)

    def select(self, b, x, y):           # gadgets/select.rs: b*x - (b*y - y)
        tmp = self.mul_sub(b, y, y)
        return self.mul_sub(b, x, tmp)

    def is_equal(self, x, y):            # gadgets/arithmetic.rs `is_equal`
        zero = self.zero()
        equal = self.add_virtual_target()
        not_equal = self.sub(self.one(), equal)
        inv = self.add_virtual_target()
        self.generators.append(("equality", x, y, equal, inv))
        diff = self.sub(x, y)
        not_equal_check = self.mul(equal, diff)
        diff_normalized = self.mul(diff, inv)
        self.connect(not_equal, diff_normalized)
        self.connect(not_equal_check, zero)
        return equal

    # ---- gadgets/hash.rs, hash/poseidon.rs `permute_swapped` (swap = false), hash/hashing.rs `hash_n_to_m_no_pad`
    def permute(self, state):
        row = self.add_gate(POSEIDON)
        self.connect(self.zero(), wire(row, PG_SWAP))
        for i in range(12):
            self.connect(state[i], wire(row, PG_IN + i))
        self.generators.append(("poseidon", row))
        return [wire(row, PG_OUT + i) for i in range(12)]

    def hash_n_to_m_no_pad(self, inputs, num_outputs):
        state = [self.zero()] * 12
        for off in range(0, len(inputs), 8):
            chunk = inputs[off:off + 8]
            state = self.permute(chunk + state[len(chunk):])
        out = []
        while True:
            for t in state[:8]:
                out.append(t)
                if len(out) == num_outputs:
                    return out
            state = self.permute(state)

    # ---- gadgets/lookup.rs
    def add_lookup_table_from_pairs(self, table):
        table = [tuple(p) for p in table]
        if not table:
            raise ValueError("lookup table is empty")
        if table in self.luts:
            return self.luts.index(table)
        self.luts.append(table)
        self.lut_lookups.append([])
        return len(self.luts) - 1

    def add_lookup_from_index(self, looking_in, lut_index):
        assert lut_index < len(self.luts)
        out = self.add_virtual_target()
        self.lut_lookups[lut_index].append((looking_in, out))
        return out

    def _add_all_lookups(self):
        for li, table in enumerate(self.luts):
            lookups = self.lut_lookups[li]
            assert lookups, "LUT %d is unused" % li
            h = debug_bytes(lut_hash(table))
            lu_type = GateType("lookup", "LookupGate {num_slots: %d, lut_hash: %s}" % (LU_SLOTS, h), 0, 0)
            lu_type.lut = li
            last_lu_gate = self.num_gates()
            for looking_in, looking_out in lookups:
                row, i = self.find_slot(lu_type, LU_SLOTS, (li,), ())
                gin, gout = wire(row, 2 * i), wire(row, 2 * i + 1)
                self.connect(gin, looking_in)
                self.connect(gout, looking_out)
                self.generators.append(("lookup", li, gin, gout))
            last_lut_gate = self.num_gates()
            lut_type = GateType("lookup_table", "LookupTableGate {num_slots: %d, lut_hash: %s, last_lut_row: %d}" % (LUT_SLOTS, h, last_lut_gate), 0, 0)
            lut_type.lut = li
            num_lut_rows = (len(table) - 1) // LUT_SLOTS + 1
            for _ in range(LUT_SLOTS * num_lut_rows):
                self.find_slot(lut_type, LUT_SLOTS, (), ())
            first_lut_gate = self.num_gates() - 1
            self.add_gate(NOOP)
            self.lookup_rows.append((last_lu_gate, last_lut_gate, first_lut_gate))

    # ---- plonk/circuit_builder.rs `build`
    def build(self):
        zero = self.zero()                         # hash_n_to_hash_no_pad([]) = four copies of the zero target
        pi_row = self.add_gate(PUBLIC_INPUT)
        for i in range(4):
            self.connect(zero, wire(pi_row, i))
        self._add_all_lookups()
        while len(self.const_to_target) > len(self.constant_generators):
            self.add_gate(CONSTANT, (0, 0))
        for (c, t), (row, idx) in zip(sorted(self.const_to_target.items()), self.constant_generators):
            self.rows[row][1][idx] = c
            self.connect(wire(row, idx), t)
            self.generators.append(("constant", wire(row, idx), c))
        while len(self.rows) < 4 or len(self.rows) & (len(self.rows) - 1):     # blind_and_pad, non-zk
            self.add_gate(NOOP)
        return Shape(self)


class Shape:
    """What preprocessing needs, derived from a finished Builder: sorted gate types, selector groups, the constants
    matrix, and sigma as a permutation of column * n + row indices."""

    def __init__(self, b):
        self.b = b
        n = self.n = len(b.rows)
        types = {}
        for g, _ in b.rows:
            types.setdefault(g.id, g)
        self.gates = sorted(types.values(), key=lambda g: (g.degree, g.id))
        index = {g.id: i for i, g in enumerate(self.gates)}
        self.row_gate = [index[g.id] for g, _ in b.rows]
        # gates/selectors.rs `selector_polynomials`
        max_degree, num = MAX_QUOTIENT_DEGREE_FACTOR + 1, len(self.gates)
        if self.gates[-1].degree + num - 1 <= max_degree:
            self.groups = [(0, num)]
        else:
            self.groups, start = [], 0
            while start < num:
                size = 0
                while start + size < num and size + self.gates[start + size].degree < max_degree:
                    size += 1
                self.groups.append((start, start + size))
                start += size
        single = len(self.groups) == 1
        self.selectors = [[gi if (single or lo <= gi < hi) else UNUSED for gi in self.row_gate] for lo, hi in self.groups]
        # selectors_lookup / selector_ends_lookups
        self.lookup_selectors = []
        if b.luts:
            sel = [[0] * n for _ in range(4 + len(b.luts))]
            for li, (last_lu, last_lut, first_lut) in enumerate(b.lookup_rows):
                for r in range(last_lut, first_lut + 1):
                    sel[0][r] = 1                                  # TransSre
                for r in range(last_lu, last_lut):
                    sel[1][r] = 1                                  # TransLdc
                sel[2][first_lut + 1] = 1                          # InitSre
                sel[3][last_lu] = 1                                # LastLdc
                sel[4 + li][last_lut] = 1                          # StartEnd
            self.lookup_selectors = sel
        self.gate_constants = [[(c[k] if k < len(c) else 0) for _, c in b.rows] for k in range(NUM_CONSTANTS)]
        self.constants = self.selectors + self.lookup_selectors + self.gate_constants
        self._partitions()

    def _node(self, t):
        if is_wire(t):
            row, col = wire_rc(t)
            assert col < NUM_ROUTED, "copy constraint on an advice wire"
            return self.b.num_virtual + row * NUM_ROUTED + col
        return t

    def _partitions(self):
        b, n = self.b, self.n
        V = b.num_virtual
        parent = list(range(V + n * NUM_ROUTED))

        def find(x):
            r = x
            while parent[r] != r:
                r = parent[r]
            while parent[x] != r:
                parent[x], x = r, parent[x]
            return r
        for x, y in b.copies:
            rx, ry = find(self._node(x)), find(self._node(y))
            if rx != ry:
                parent[rx] = ry
        self.find, self.V = find, V
        # plonk/permutation_argument.rs: `wire_partition` collects each class's wires in (row, column) order;
        # `get_sigma_map` sends every wire to the next of its class, the last to the first
        members = {}
        for row in range(n):
            for col in range(NUM_ROUTED):
                members.setdefault(find(V + row * NUM_ROUTED + col), []).append((row, col))
        sigma = [0] * (NUM_ROUTED * n)
        for ws in members.values():
            for k, (row, col) in enumerate(ws):
                nr, nc = ws[(k + 1) % len(ws)]
                sigma[col * n + row] = nc * n + nr
        self.sigma = sigma

    def sigma_values(self):
        """sigma as field elements k_{col} * omega^{row}, column-major, as plonky2's `sigma_vecs`."""
        n = self.n
        bits = n.bit_length() - 1
        omega = pow(POWER_OF_TWO_GENERATOR, 1 << (32 - bits), P)       # primitive_root_of_unity(bits)
        sub, x = [], 1
        for _ in range(n):
            sub.append(x)
            x = x * omega % P
        ks, k = [], 1
        for _ in range(NUM_ROUTED):
            ks.append(k)
            k = k * MULTIPLICATIVE_GROUP_GENERATOR % P                  # get_unique_coset_shifts: g^i
        return [ks[s // n] * sub[s % n] % P for s in self.sigma]

    # ------------------------------------------------------------------------------------------- witness
    def witness(self, inputs):
        """inputs: {virtual target: value}.  Returns wires[col][row]: the 80 routed columns, or all 135 when the circuit has
        PoseidonGate rows (the only gate here with advice wires).  Raises ValueError the way plonky2's generators / its
        copy-constraint check would fail."""
        b, n, find, V = self.b, self.n, self.find, self.V
        val = {}

        def setv(t, v):
            r = find(self._node(t))
            if val.setdefault(r, v) != v:
                raise ValueError("conflicting values in one copy class")
        for t, v in inputs.items():
            setv(t, v % P)
        def outs(g):
            if g[0] == "poseidon":         # every routed wire of the row except its inputs and swap
                return [wire(g[1], c) for c in range(PG_OUT, NUM_ROUTED) if c != PG_SWAP]
            return {"arith": g[6:7], "equality": g[3:5], "lookup": g[3:4], "constant": g[1:2]}[g[0]]

        def ins(g):
            if g[0] == "poseidon":
                return [wire(g[1], PG_IN + i) for i in range(12)] + [wire(g[1], PG_SWAP)]
            return {"arith": g[3:6], "equality": g[1:3], "lookup": g[2:3], "constant": ()}[g[0]]
        advice = {}                        # row -> the 135 wire values of a PoseidonGate row
        tables = [dict(t) for t in b.luts]

        def run(g):
            v = [val[find(self._node(t))] for t in ins(g)]
            if g[0] == "arith":
                setv(g[6], (g[1] * v[0] * v[1] + g[2] * v[2]) % P)
            elif g[0] == "poseidon":
                full = poseidon_gate_row(v[:12], v[12])
                for c in range(PG_OUT, NUM_ROUTED):
                    if c != PG_SWAP:
                        setv(wire(g[1], c), full[c])
                advice[g[1]] = full
            elif g[0] == "constant":
                setv(g[1], g[2])
            elif g[0] == "equality":
                d = (v[0] - v[1]) % P
                setv(g[3], 1 if d == 0 else 0)
                setv(g[4], 0 if d == 0 else pow(d, P - 2, P))
            else:
                if v[0] not in tables[g[1]]:
                    raise ValueError("lookup input is not in the table")
                setv(g[3], tables[g[1]][v[0]])
        # iop/generator.rs `generate_partial_witness`: a generator runs once everything it watches is set (whichever
        # generator or input set it); what it writes may wake others; whatever never runs leaves the witness incomplete
        watchers, missing, ready = {}, [], []
        for k, g in enumerate(b.generators):
            unset = {find(self._node(t)) for t in ins(g)} - val.keys()
            missing.append(len(unset))
            for r in unset:
                watchers.setdefault(r, []).append(k)
            if not unset:
                ready.append(k)
        ran = 0
        while ready:
            g = b.generators[ready.pop()]
            before = [find(self._node(o)) for o in outs(g)]
            fresh = [r for r in before if r not in val]
            run(g)
            ran += 1
            for r in dict.fromkeys(fresh):
                for k in watchers.pop(r, ()):
                    missing[k] -= 1
                    if missing[k] == 0:
                        ready.append(k)
        if ran != len(b.generators):
            raise ValueError("some generators never ran: the witness is incomplete")
        wires = [[0] * n for _ in range(NUM_WIRES if advice else NUM_ROUTED)]
        for row, full in advice.items():
            for c in range(NUM_ROUTED, NUM_WIRES):
                wires[c][row] = full[c]
        for row in range(n):
            for col in range(NUM_ROUTED):
                v = val.get(find(V + row * NUM_ROUTED + col))
                if v:
                    wires[col][row] = v
        # prover.rs `set_lookup_wires` + LookupTableGenerator: table rows upside down, multiplicities, padding of the
        # last LookupGate row with the table's first pair
        for li, (last_lu, last_lut, first_lut) in enumerate(b.lookup_rows):
            table = b.luts[li]
            pos = {inp: i for i, (inp, _) in enumerate(table)}
            mult = [0] * len(table)
            for looking_in, _ in b.lut_lookups[li]:
                mult[pos[val[find(self._node(looking_in))]]] += 1
            remaining = (LU_SLOTS - len(b.lut_lookups[li]) % LU_SLOTS) % LU_SLOTS
            for slot in range(LU_SLOTS - remaining, LU_SLOTS):
                wires[2 * slot][last_lut - 1], wires[2 * slot + 1][last_lut - 1] = table[0]
                mult[0] += 1
            for e, (inp, out) in enumerate(table):
                row, s = first_lut - e // LUT_SLOTS, e % LUT_SLOTS
                wires[3 * s][row], wires[3 * s + 1][row], wires[3 * s + 2][row] = inp, out, mult[e]
        return wires


# ===================================================================================================== Poseidon
def _round_constants():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "poseidon_rc.inc")).read()
    rc = [int(h, 16) for h in re.findall(r"0x([0-9a-fA-F]{16})ULL", text)]
    assert len(rc) == 360 and rc[0] == 0xB585F766F2144405            # upstream's first published constant
    return rc


MDS_CIRC, MDS_DIAG = [17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20], [8] + [0] * 11   # hash/poseidon_goldilocks.rs
_RC = None


def poseidon_gate_row(inputs, swap):
    """PoseidonGenerator::run_once (gates/poseidon.rs): the 135 wires of one PoseidonGate row from its 12 inputs and swap."""
    global _RC
    _RC = _RC or _round_constants()
    row = [0] * NUM_WIRES
    row[PG_IN:PG_IN + 12], row[PG_SWAP] = inputs, swap
    st = list(inputs)
    for i in range(4):
        row[PG_DELTA + i] = d = swap * (inputs[4 + i] - inputs[i]) % P
        st[i], st[4 + i] = (inputs[i] + d) % P, (inputs[4 + i] - d) % P
    for rnd in range(30):
        st = [(x + _RC[12 * rnd + i]) % P for i, x in enumerate(st)]
        if rnd < 4 or rnd >= 26:                                   # full rounds; the very first S-box layer is not witnessed
            if rnd > 0:
                base = PG_FULL0 + 12 * (rnd - 1) if rnd < 4 else PG_FULL1 + 12 * (rnd - 26)
                row[base:base + 12] = st
            st = [pow(x, 7, P) for x in st]
        else:
            row[PG_PARTIAL + rnd - 4] = st[0]
            st[0] = pow(st[0], 7, P)
        st = [(sum(st[(i + r) % 12] * MDS_CIRC[i] for i in range(12)) + st[r] * MDS_DIAG[r]) % P for r in range(12)]
    row[PG_OUT:PG_OUT + 12] = st
    return row


def feistel_cipher(b, state, key_schedule, half=4):      # feistel/src/circuit.rs:42-70, f = hash_n_to_hash_no_pad (:126-131)
    for k in key_schedule:
        left, right = state[:half], state[half:]
        offset = b.hash_n_to_m_no_pad(right + list(k), 4)
        state = right + [b.add(left[i], offset[i]) for i in range(half)]
    return state


# ===================================================================================================== AES gadgets
def _gmul(a, b):                       # native_aes.rs:82-98
    r = 0
    for _ in range(8):
        if b & 1:
            r ^= a
        a = ((a << 1) ^ (0x1B if a & 0x80 else 0)) & 0xFF
        b >>= 1
    return r


def _sbox():                           # FIPS-197 5.1.1: multiplicative inverse, then the affine map (constants.rs:10-28 tabulates it)
    out = []
    for x in range(256):
        inv = next((y for y in range(256) if _gmul(x, y) == 1), 0)
        s = inv
        for k in range(1, 5):
            s ^= ((inv << k) | (inv >> (8 - k))) & 0xFF
        out.append(s ^ 0x63)
    return out


SBOX = _sbox()
RCON = [0x00, 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80, 0x1B, 0x36]     # constants.rs:31-34


def sbox_lut(b): return b.add_lookup_table_from_pairs([(i, o) for i, o in enumerate(SBOX)])                              # circuit_aes.rs:291-298
def byte_xor_lut(b): return b.add_lookup_table_from_pairs([((x << 8) + y, x ^ y) for x in range(256) for y in range(256)])  # :301-310
def gf_2_8_mul_lut(b): return b.add_lookup_table_from_pairs([((x << 8) + y, _gmul(x, y)) for x in range(256) for y in range(256)])  # :313-328
def u8_unit_right_shift_lut(b): return b.add_lookup_table_from_pairs([(x, x >> 1) for x in range(256)])                  # circuit_gcm.rs:390-395
def u8_bitref_lut(b): return b.add_lookup_table_from_pairs([((x << 3) + i, (x >> i) & 1) for x in range(256) for i in range(8)])   # :405-414


def add_virtual_byte_target(b, u8_lut):          # circuit_aes.rs:47-51, 181-183
    t = b.add_virtual_target()
    b.add_lookup_from_index(t, u8_lut)
    return t


def byte_xor(b, xor_lut, x, y):                  # circuit_aes.rs:350-358
    return b.add_lookup_from_index(b.mul_const_add(1 << 8, x, y), xor_lut)


def gf_2_8_mul(b, mul_lut, x, y):                # circuit_aes.rs:243-251
    return b.add_lookup_from_index(b.mul_const_add(1 << 8, x, y), mul_lut)


def state_mix_matrix(b):                         # circuit_aes.rs:330-341
    one, two, three = b.constant(1), b.constant(2), b.constant(3)
    return [[two, three, one, one], [one, two, three, one], [one, one, two, three], [three, one, one, two]]


def sub_word(b, sbox, word):                     # circuit_aes.rs:189-195
    return [b.add_lookup_from_index(t, sbox) for t in word]


def key_expansion(b, xor_lut, sbox, key, nk, nr):   # circuit_aes.rs:197-237
    rcon = [b.constant(c) for c in RCON]
    st = [[key[4 * i + j] for j in range(4)] for i in range(nk)]
    for i in range(nk, 4 * (nr + 1)):
        if i % nk == 0:
            prev = st[i - 1]
            term = sub_word(b, sbox, [prev[(j + 1) % 4] for j in range(4)])
            offset = [byte_xor(b, xor_lut, term[0], rcon[i // nk])] + term[1:]
        elif nk > 6 and i % nk == 4:
            offset = sub_word(b, sbox, st[i - 1])
        else:
            offset = st[i - 1]
        st.append([byte_xor(b, xor_lut, st[i - nk][j], offset[j]) for j in range(4)])
    return st


def add_round_key(b, xor_lut, round_key, s):     # circuit_aes.rs:129-139
    return [[byte_xor(b, xor_lut, s[i][j], round_key[j][i]) for j in range(4)] for i in range(4)]


def sub_bytes(b, sbox, s):                       # circuit_aes.rs:98-103
    return [sub_word(b, sbox, s[i]) for i in range(4)]


def shift_rows(s):                               # native_aes.rs:66-68
    return [[s[i][(i + j) % 4] for j in range(4)] for i in range(4)]


def bytearray_ip(b, xor_lut, mul_lut, x, y):     # circuit_aes.rs:253-265
    acc = b.zero()
    for u, v in zip(x, y):
        acc = byte_xor(b, xor_lut, acc, gf_2_8_mul(b, mul_lut, u, v))
    return acc


def mix_columns(b, xor_lut, mul_lut, mix, s):    # circuit_aes.rs:108-126, 160-168
    cols = [[s[j][i] for j in range(4)] for i in range(4)]
    out_cols = [[bytearray_ip(b, xor_lut, mul_lut, mix[r], cols[i]) for r in range(4)] for i in range(4)]
    return [[out_cols[j][i] for j in range(4)] for i in range(4)]


def encrypt_block(b, luts, mix, s, w, nr):       # circuit_aes.rs:76-95
    xor_lut, mul_lut, sbox = luts
    s = add_round_key(b, xor_lut, w[0:4], s)
    for i in range(1, nr):
        s = sub_bytes(b, sbox, s)
        s = shift_rows(s)
        s = mix_columns(b, xor_lut, mul_lut, mix, s)
        s = add_round_key(b, xor_lut, w[4 * i:4 * i + 4], s)
    s = sub_bytes(b, sbox, s)
    s = shift_rows(s)
    return add_round_key(b, xor_lut, w[4 * nr:4 * nr + 4], s)


def flatten(s): return [s[i % 4][i // 4] for i in range(16)]                    # circuit_aes.rs:29-31
def from_flat(f): return [[f[j * 4 + i] for j in range(4)] for i in range(4)]    # circuit_aes.rs:33-35


def inc32(b, block):                             # circuit_gcm.rs:350-368
    r = list(block)
    zero, u8_max = b.zero(), b.constant(255)
    carry = b.one()
    for k in (15, 14, 13, 12):
        a = block[k]
        total = b.add(a, carry)
        a_is_max = b.is_equal(a, u8_max)
        carry_out = b.mul(carry, a_is_max)
        r[k] = b.select(a_is_max, zero, total)
        carry = carry_out
    return r


def xor_blocks(b, xor_lut, x, y): return [byte_xor(b, xor_lut, x[i], y[i]) for i in range(16)]   # circuit_gcm.rs:370-377


def gctr(b, luts, mix, key, icb, x, nr):         # circuit_gcm.rs:212-260
    L = len(x)
    nblocks = -(-L * 8 // 128)
    y, cb = list(x), list(icb)
    zero = b.zero()
    for i in range(0, -(-L // 16)):
        raw = x[16 * i:16 * i + 16]
        if i > 0:
            cb = inc32(b, cb)
        xi = raw + [zero] * (16 - len(raw))
        ciph = flatten(encrypt_block(b, luts, mix, from_flat(cb), key, nr))
        if i < nblocks and len(raw) == 16:
            yi, nbytes = xor_blocks(b, luts[0], xi, ciph), 16
        else:
            msb = ciph[:L % 16]
            yi, nbytes = xor_blocks(b, luts[0], xi, msb + [zero] * (16 - len(msb))), len(msb)
        y[16 * i:16 * i + nbytes] = yi[:nbytes]
    return y


def u8_bitref(b, bitref_lut, x, i):              # circuit_gcm.rs:417-425
    return b.add_lookup_from_index(b.mul_const_add(8, x, i), bitref_lut)


def right_shift_one(b, shift_lut, v):            # circuit_gcm.rs:327-348
    r, carry = list(v), b.zero()
    for i in range(16):
        cur = v[i]
        shifted = b.add_lookup_from_index(cur, shift_lut)
        next_carry = b.mul_const_add(2 * (P - 1), shifted, cur)
        r[i] = b.mul_const_add(1 << 7, carry, shifted)
        carry = next_carry
    return r


def gf_2_128_mul(b, xor_lut, shift_lut, bitref_lut, x, y):    # circuit_gcm.rs:290-326
    zero = b.zero()
    r_first = b.constant(225)
    z, v = [zero] * 16, list(y)
    for i in range(128):
        xi = u8_bitref(b, bitref_lut, x[i // 8], b.constant(7 - i % 8))
        for k in range(16):
            z[k] = b.select(xi, byte_xor(b, xor_lut, z[k], v[k]), z[k])
        lsb = u8_bitref(b, bitref_lut, v[15], zero)
        v = right_shift_one(b, shift_lut, v)
        v[0] = b.select(lsb, byte_xor(b, xor_lut, v[0], r_first), v[0])
    return z


def ghash(b, xor_lut, shift_lut, bitref_lut, h, x):           # circuit_gcm.rs:262-289
    assert len(x) % 16 == 0
    y = [b.zero()] * 16
    for i in range(len(x) // 16):
        y = gf_2_128_mul(b, xor_lut, shift_lut, bitref_lut, xor_blocks(b, xor_lut, y, x[16 * i:16 * i + 16]), h)
    return y


class AesGcmTarget:
    """circuit_gcm.rs:49-172 (`build`) and :174-208 (`set_targets`)."""

    def __init__(self, b, nk, nr, L, tag):
        self.L, self.with_tag = L, tag
        sbox, xor_lut, mul_lut = sbox_lut(b), byte_xor_lut(b), gf_2_8_mul_lut(b)
        self.key = [add_virtual_byte_target(b, sbox) for _ in range(4 * nk)]
        self.nonce = [add_virtual_byte_target(b, sbox) for _ in range(12)]
        self.pt = [add_virtual_byte_target(b, sbox) for _ in range(L)]
        self.tag = [add_virtual_byte_target(b, sbox) for _ in range(16)]
        mix = state_mix_matrix(b)
        luts = (xor_lut, mul_lut, sbox)
        expanded = key_expansion(b, xor_lut, sbox, self.key, nk, nr)
        zero = b.zero()
        h = flatten(encrypt_block(b, luts, mix, [[zero] * 4 for _ in range(4)], expanded, nr))
        j0 = self.nonce + [zero, zero, zero, b.constant(1)]
        self.ct = gctr(b, luts, mix, expanded, inc32(b, j0), self.pt, nr)
        if not tag:
            return
        u = 16 * -(-L // 16) - L
        a_len = [b.constant(c) for c in (0).to_bytes(8, "big")]
        c_len = [b.constant(c) for c in (L * 8).to_bytes(8, "big")]
        ghash_input = self.ct + [zero] * u + a_len + c_len
        shift_lut, bitref_lut = u8_unit_right_shift_lut(b), u8_bitref_lut(b)
        s = ghash(b, xor_lut, shift_lut, bitref_lut, h, ghash_input)
        t = gctr(b, luts, mix, expanded, j0, s, nr)[:16]
        for x, y in zip(self.tag, t):
            b.connect(x, y)

    def inputs(self, key, nonce, pt, ct, tag):
        assert len(pt) == self.L and len(ct) == self.L        # `copy_from_slice` panics on any other length
        m = {}
        for ts, vs in ((self.key, key), (self.nonce, nonce), (self.pt, pt), (self.ct, ct)):
            m.update(zip(ts, vs))
        m.update(zip(self.tag, tag if self.with_tag else bytes(16)))
        return m
