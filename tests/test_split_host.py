"""Bit and byte decomposition in circuits, on the host: split_le, range_check, le_sum, split_bytes_le, le_bytes_sum,
is_less_than and the witness op behind them (OP_LIMB), through p2_host_witness -- no device.

What is compared: bits and bytes with Python's own, statuses, fault records; all exact.  The soundness cases build the same
constraints WITHOUT the hints (virtual targets the test sets itself) so that a wrong spelling is refused by the constraints,
not by a generator that would never have produced it."""
import pytest

import device_build as device
import split_circuits as sc

P = sc.P


def host(pkg, data, m, outs=()):
    vals, st, f = pkg.host_witness(data.blob, m, outs)
    assert f.status == st and (f.kind == "NONE") == (st == 0), f
    return vals, st, f


# ------------------------------------------------------------------ values
def test_split_le_gives_pythons_bits(pkg):
    data, xs, bits, maps, want = sc.split_le(pkg)
    flat = [t for bs in bits for t in bs]
    assert [len(bs) for bs in bits] == list(sc.WIDTHS)
    seen = set()
    for m, w in zip(maps, want):
        vals, st, _ = host(pkg, data, m, flat)
        assert st == 0 and vals == w, m
        seen |= set(m.values())
    assert {0, 1, (1 << 32) - 1, 1 << 32, 0xFFFFFFFF00000000, P - 1, (1 << 63) - 1, 255} <= seen


@pytest.mark.parametrize("k", (1, 8, 32, 63))
def test_range_check_refuses_two_to_the_k(pkg, k):
    b = pkg.CircuitBuilder()
    x = b.add_virtual_target()
    b.range_check(x, k)
    data = b.build()
    for v in (0, (1 << k) - 1):
        assert host(pkg, data, {x: v})[1] == 0
    _, st, f = host(pkg, data, {x: 1 << k})
    assert st == 1 and f.kind == "GENERATOR_CONFLICT"


def test_split_bytes_le_gives_pythons_bytes(pkg):
    data, xs, parts, maps, want = sc.split_bytes_le(pkg)
    flat = [t for p in parts for t in p]
    assert [len(p) for p in parts] == list(sc.BYTE_COUNTS)
    for m, w in zip(maps, want):
        vals, st, _ = host(pkg, data, m, flat)
        assert st == 0 and vals == w, m
    m = dict(maps[0])
    m[xs[1]] = 1 << 56   # the 7-byte input
    assert host(pkg, data, m)[1] == 1


@pytest.mark.parametrize("n", sc.LT_WIDTHS)
def test_is_less_than(pkg, n):
    data, x, y, lt = sc.is_less_than(pkg, n)
    for a, c in sc.lt_pairs(n):
        vals, st, _ = host(pkg, data, {x: a, y: c}, [lt])
        assert st == 0 and vals == [int(a < c)], (a, c)
    assert host(pkg, data, {x: 1 << n, y: 0})[1] == 1
    assert host(pkg, data, {x: 0, y: 1 << n})[1] == 1


# ------------------------------------------------------------------ soundness without the hints
@pytest.fixture(scope="module")
def by_hand(pkg):
    """64 bit targets and 8 byte targets the test sets itself, constrained by the public pieces only"""
    b = pkg.CircuitBuilder()
    bits = [b.add_virtual_target() for _ in range(64)]
    for t in bits:
        b.assert_bool(t)
    total = b.le_sum(bits)
    bit_data = b.build()
    b = pkg.CircuitBuilder()
    lut = b.sbox_lut()
    byts = [b.add_virtual_target() for _ in range(8)]
    for t in byts:
        b.add_lookup_from_index(t, lut)   # assert_byte
    btotal = b.le_bytes_sum(byts)
    return bit_data, bits, total, b.build(), byts, btotal


@pytest.mark.parametrize("v", (0, 1, (1 << 32) - 2))
def test_sixty_four_bits_have_one_spelling(pkg, by_hand, v):
    data, bits, total = by_hand[:3]
    vals, st, _ = host(pkg, data, dict(zip(bits, sc.bits_of(v, 64))), [total])
    assert st == 0 and vals == [v]
    assert v + P < 1 << 64
    _, st, f = host(pkg, data, dict(zip(bits, sc.bits_of(v + P, 64))))
    assert st == 1 and f.kind == "GENERATOR_CONFLICT"


def test_a_bit_of_two_is_refused(pkg, by_hand):
    data, bits, total = by_hand[:3]
    m = dict(zip(bits, sc.bits_of(5, 64)))
    m[bits[1]] = 2
    _, st, f = host(pkg, data, m)
    assert st == 1 and f.kind == "GENERATOR_CONFLICT"


@pytest.mark.parametrize("v", (0, 1, (1 << 32) - 2))
def test_eight_bytes_have_one_spelling(pkg, by_hand, v):
    data, byts, total = by_hand[3:]
    vals, st, _ = host(pkg, data, dict(zip(byts, v.to_bytes(8, "little"))), [total])
    assert st == 0 and vals == [v]
    _, st, f = host(pkg, data, dict(zip(byts, (v + P).to_bytes(8, "little"))))
    assert st == 1 and f.kind == "GENERATOR_CONFLICT"


def test_a_byte_of_256_is_refused(pkg, by_hand):
    data, byts, total = by_hand[3:]
    m = dict(zip(byts, (77).to_bytes(8, "little")))
    m[byts[2]] = 256
    _, st, f = host(pkg, data, m)
    assert st == 1 and f.kind == "LOOKUP_MISS" and f.found == 256 and f.target == byts[2]


def test_short_sums_are_plain_horner_chains(pkg):
    """63 bits and 7 bytes, the widest sums that need no canonicity condition: the largest values come out as they are"""
    b = pkg.CircuitBuilder()
    bits = [b.add_virtual_target() for _ in range(63)]
    total = b.le_sum(bits)
    data = b.build()
    v = (1 << 63) - 12345
    assert host(pkg, data, dict(zip(bits, sc.bits_of(v, 63))), [total])[0] == [v]
    b = pkg.CircuitBuilder()
    lut = b.sbox_lut()
    byts = [b.add_virtual_byte_target(lut) for _ in range(7)]
    total = b.le_bytes_sum(byts)
    data = b.build()
    v = (1 << 56) - 3
    assert host(pkg, data, dict(zip(byts, v.to_bytes(7, "little"))), [total])[0] == [v]


# ------------------------------------------------------------------ faults with the hints present
def test_a_wrong_bit_loses_against_its_hint(pkg):
    data, xs, bits, maps, _ = sc.split_le(pkg)
    m = dict(maps[1])
    t = bits[2][5]                       # bit 5 of the 32-bit input
    right = (m[xs[2]] >> 5) & 1
    m[t] = 1 - right
    _, st, f = host(pkg, data, m)
    assert (st, f.kind, f.op_kind, f.target, f.computed, f.found) == (1, "GENERATOR_CONFLICT", "LIMB", t, right, 1 - right)
    assert f.input_index == list(m).index(t)


def test_an_unset_input_is_named(pkg):
    data, xs, bits, maps, _ = sc.split_le(pkg)
    m = dict(maps[0])
    del m[xs[3]]
    _, st, f = host(pkg, data, m)
    assert (st, f.kind, f.target) == (2, "NOT_SET", xs[3])
    bdata, bxs, _, bmaps, _ = sc.split_bytes_le(pkg)
    m = dict(bmaps[0])
    del m[bxs[0]]
    _, st, f = host(pkg, bdata, m)
    assert (st, f.kind, f.target) == (2, "NOT_SET", bxs[0])


# ------------------------------------------------------------------ schedule, arguments, code generation
def test_wide_circuit_on_the_host(pkg):
    data, xs, bits = sc.wide(pkg)
    assert data.info["degree_bits"] <= 10
    vals = sc.wide_values(0)
    got, st, _ = host(pkg, data, dict(zip(xs, vals)), bits)
    assert st == 0 and got == [bit for v in vals for bit in sc.bits_of(v, sc.WIDE_BITS)]


def test_bridge_circuit_on_the_host(pkg):
    data, secret, block, ct = sc.bridge(pkg)
    maps, want = sc.bridge_cases(pkg, 1)
    got, st, _ = host(pkg, data, maps[0], ct)
    assert st == 0 and bytes(got) == want[0]


@pytest.mark.parametrize("which", ("wide", "bridge"))
def test_witness_schedule_holds_for_every_fuse(pkg, which):
    data = (sc.wide if which == "wide" else sc.bridge)(pkg)[0]
    plain = data.witness_schedule(1)
    assert plain["chains"] == 0
    for fuse in range(2, 9):
        s = data.witness_schedule(fuse)
        assert s["max_chain"] <= fuse and s["levels"] <= plain["levels"]


def test_widths_out_of_range_are_errors(pkg):
    b = pkg.CircuitBuilder()
    x, y = b.add_virtual_target(), b.add_virtual_target()
    lut = b.sbox_lut()
    for call in (lambda: b.split_le(x, 0), lambda: b.split_le(x, 65), lambda: b.range_check(x, 0), lambda: b.range_check(x, 64),
                 lambda: b.split_bytes_le(x, 0, lut), lambda: b.split_bytes_le(x, 9, lut), lambda: b.split_bytes_le(x, 4, lut + 5),
                 lambda: b.is_less_than(x, y, 0), lambda: b.is_less_than(x, y, 63), lambda: b.le_sum([]), lambda: b.le_sum([x] * 65),
                 lambda: b.le_bytes_sum([]), lambda: b.le_bytes_sum([x] * 9)):
        with pytest.raises(pkg.P2Error):
            call()
    assert len(b.split_le(x, 64)) == 64 and len(b.split_bytes_le(y, 8, lut)) == 8   # the builder is still usable
    b.build()


# k_witness<HAS_POSEIDON, CHAINS> before OP_LIMB: (VGPRs, ScratchSize); the Poseidon instantiations carried their scratch
# before (witness_poseidon_op keeps its 135-word row in memory)
BEFORE = {"ILb0ELb0E": (126, 0), "ILb0ELb1E": (252, 0), "ILb1ELb0E": (209, 1216), "ILb1ELb1E": (256, 1232)}


def test_the_new_op_spills_nothing(pkg):
    assert "LIMB" in pkg.OP_KINDS   # the figures below are about a build that has the op
    remarks = device.cross_compile()[0]
    for fragment in ("k_witness_check", "k_witness_report"):
        found = [v for name, v in remarks.items() if fragment in name]
        assert found, fragment
        for k in found:
            assert k["ScratchSize"] == 0, (fragment, k)
    for inst, (vgprs, scratch) in BEFORE.items():
        found = [v for name, v in remarks.items() if "k_witness" + inst in name]
        assert len(found) == 1, inst
        print("k_witness%s: VGPRs %d (before %d), ScratchSize %d (before %d)" % (inst, found[0]["VGPRs"], vgprs, found[0]["ScratchSize"], scratch))
        assert found[0]["ScratchSize"] <= scratch, (inst, found[0])
