"""GHASH from carry-less multiply tables on the host (CPU): the two tables, the multiplication gadget, the GHASH gadget with
lanes, AesGcmTarget under CircuitBuilder(ghash_tables=lanes) and the sizes of what they build, all through the host witness
twin.  Values come from the native cipher (the bit-serial algorithm), the known answers of tests/golden/aes_kat.json and the
plain-Python restatement tests/ghash_ref.py.  Everything compared is a byte, a count or a status: exact."""
import json
import os
import random

import numpy as np
import pytest

import blob_reader
import ghash_circuits as K
import ghash_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "aes_kat.json")))
GCM_VECTORS = GOLD["cavp_gcm128"] + GOLD["derived_by_pinned_oracle"]   # every one has a tag; the first has an empty plaintext
LANES_BY_VECTOR = (1, 2, 3, 8, 1, 2, 1, 4, 16)


def rnd_block(r):
    return bytes(r.randrange(256) for _ in range(16))


# ------------------------------------------------------------------------------------------ 1. tables
def test_both_tables_in_a_built_blob_equal_the_restatement(pkg):
    data, _, _, _, (lo, hi) = K.mul(pkg)
    luts = blob_reader.Blob(data.blob).luts
    index = np.arange(65536)
    for lut, want in ((lo, G.LO), (hi, G.HI)):
        assert luts[lut].shape == (65536, 2)
        assert np.array_equal(luts[lut][:, 0], index)
        assert np.array_equal(luts[lut][:, 1], np.array(want))
    assert not any(v & 1 for v in G.HI)                     # a 15-bit product: x^15 never appears
    assert lo != hi and data.info["num_luts"] == 4


def test_restated_table_multiply_equals_bit_serial_and_native(pkg):
    r = random.Random(2)
    y = rnd_block(r)
    pairs = [(bytes(16), bytes(16)), (b"\xff" * 16, b"\xff" * 16)] + [(x, y) for x in K.single_bit_blocks()]
    pairs += [(rnd_block(r), rnd_block(r)) for _ in range(200)]
    assert K.single_bit_blocks()[0] == b"\x80" + bytes(15)      # the unit of GF(2^128)
    assert G.gf_mul_tables(K.single_bit_blocks()[0], y) == y
    for x, y in pairs:
        z = G.gf_mul_tables(x, y)
        assert z == G.gf_mul_bit_serial(x, y) == pkg.native.gf_2_128_mul(x, y), (x.hex(), y.hex())


# ------------------------------------------------------------------------------------------ 2. one multiplication as a circuit
def test_multiplication_circuit_computes_the_native_product(pkg):
    data, x_t, y_t, z_t, _ = K.mul(pkg)
    assert data.info["degree_bits"] == 13
    r = random.Random(3)
    y = rnd_block(r)
    for x, yy in K.edge_pairs(count=4) + [(x, y) for x in K.single_bit_blocks()[::9]] + [(y, x) for x in K.single_bit_blocks()[::13]]:
        vals, st, fault = pkg.host_witness(data.blob, K.mul_inputs(x_t, y_t, x, yy), z_t)
        assert st == 0 and fault.kind == "NONE"
        assert bytes(vals) == pkg.native.gf_2_128_mul(x, yy), (x.hex(), yy.hex())


def test_multiplication_circuit_refuses_a_wrong_product_and_a_missing_operand(pkg):
    data, x_t, y_t, z_t, _ = K.mul(pkg)
    x, y = K.edge_pairs()[2]
    z = pkg.native.gf_2_128_mul(x, y)
    honest = K.mul_inputs(x_t, y_t, x, y)
    honest.update(zip(z_t, z))
    assert pkg.host_witness(data.blob, honest)[1] == 0
    wrong = dict(honest)
    wrong[z_t[5]] = (z[5] + 1) % 256
    _, st, fault = pkg.host_witness(data.blob, wrong)
    assert st == 1 and fault.kind == "GENERATOR_CONFLICT" and fault.target == z_t[5]
    missing = dict(honest)
    del missing[y_t[9]]
    _, st, fault = pkg.host_witness(data.blob, missing)
    assert st == 2 and fault.kind == "NOT_SET" and fault.target == y_t[9]


# ------------------------------------------------------------------------------------------ 3. the GHASH gadget
BLOCK_COUNTS = (1, 2, 3, 5, 8, 9)


@pytest.mark.parametrize("lanes", (1, 2, 3, 8))
def test_ghash_gadget_equals_native_ghash(pkg, lanes):
    data, h_t, xs_t, outs_t = K.ghash(pkg, lanes, BLOCK_COUNTS)
    r = random.Random(40 + lanes)
    for h in (rnd_block(r), b"\xff" * 16):
        xs = [bytes(r.randrange(256) for _ in range(16 * n)) for n in BLOCK_COUNTS]
        m = dict(zip(h_t, h))
        for x_t, x in zip(xs_t, xs):
            m.update(zip(x_t, x))
        vals, st, fault = pkg.host_witness(data.blob, m, [t for o in outs_t for t in o])
        assert st == 0 and fault.kind == "NONE"
        for i, x in enumerate(xs):
            want = pkg.native.ghash(h, x)
            assert want == G.ghash_lanes(h, x, lanes)
            assert bytes(vals[16 * i:16 * i + 16]) == want, (lanes, BLOCK_COUNTS[i])


@pytest.mark.parametrize("lanes", (0, 17, -1))
def test_lanes_out_of_range_are_refused_with_a_message(pkg, lanes):
    b = pkg.CircuitBuilder()
    sb, xl, lo, hi = b.sbox_lut(), b.byte_xor_lut(), b.clmul_lo_lut(), b.clmul_hi_lut()
    h = [b.add_virtual_byte_target(sb) for _ in range(16)]
    with pytest.raises(pkg.P2Error):
        b.ghash_tables(xl, lo, hi, h, h, lanes)
    assert b"lanes" in pkg.lib().p2_last_error()
    if lanes:
        with pytest.raises(pkg.P2Error) as e:
            pkg.CircuitBuilder(ghash_tables=lanes)
        assert "lanes" in str(e.value) and b"lanes" in pkg.lib().p2_last_error()
    with pytest.raises(pkg.P2Error):
        b.ghash_tables(xl, lo, hi, h, h[:15], 1)             # not a multiple of 16 bytes


# ------------------------------------------------------------------------------------------ 4. AesGcmTarget with the switch
@pytest.mark.parametrize("i", range(len(GCM_VECTORS)))
def test_aes_gcm_known_answers_with_the_switch(pkg, i):
    v = GCM_VECTORS[i]
    key, iv, pt, ct, tag = (bytes.fromhex(v[k]) for k in ("key", "iv", "pt", "ct", "tag"))
    data, t = K.gcm(pkg, len(key) // 4, len(pt), LANES_BY_VECTOR[i])
    assert data.info["num_luts"] == 5
    # from the inputs alone
    vals, st, fault = pkg.host_witness(data.blob, K.gcm_inputs(t, key, iv, pt), t.ct + t.tag)
    assert st == 0 and fault.kind == "NONE"
    assert bytes(vals[:len(pt)]) == ct and bytes(vals[len(pt):]) == tag
    # the witness with the right ciphertext and tag is taken, one with a tag bit flipped is not
    honest = K.gcm_inputs(t, key, iv, pt, tag)
    honest.update(zip(t.ct, ct))
    assert pkg.host_witness(data.blob, honest)[1] == 0
    for byte, bit in ((0, 0), (15, 7)):
        bad = dict(honest)
        bad[t.tag[byte]] ^= 1 << bit
        assert pkg.host_witness(data.blob, bad)[1] == 1


def test_both_key_sizes_are_among_the_vectors():
    assert {len(v["key"]) // 2 for v in GCM_VECTORS} == {16, 32}


@pytest.mark.parametrize("nk,L,lanes", [(4, 13, 1), (4, 32, 1), (4, 32, 2), (8, 13, 1), (8, 32, 3)])
def test_reference_shapes_against_the_native_cipher(pkg, nk, L, lanes):
    key, iv, pt = bytes([42] * (4 * nk)), bytes([111] * 12), bytes([42] * L)   # circuit_gcm.rs:695 test_encrypt
    ct, tag = pkg.native.gcm_encrypt(key, iv, pt)
    data, t = K.gcm(pkg, nk, L, lanes)
    vals, st, _ = pkg.host_witness(data.blob, K.gcm_inputs(t, key, iv, pt), t.ct + t.tag)
    assert st == 0 and bytes(vals) == ct + tag


# ------------------------------------------------------------------------------------------ 5. sizes
def built(pkg, L, tag, lanes):
    """(rows in use before padding, info): ArithmeticGate rows as the builder counts them, plus LookupGate rows"""
    b = pkg.CircuitBuilder(ghash_tables=lanes)
    pkg.AesGcmTarget.build(b, 4, 10, L, tag)
    rows = b.num_gates()
    data = b.build()
    rows += sum((int(n) + 39) // 40 for n in blob_reader.Blob(data.blob).num_lookups)
    return rows, data.info


def test_one_more_block_costs_at_most_70_rows_and_32_levels(pkg):
    """Per 16-byte block the gadget has 800 arithmetic ops (20 to a row) and 1072 lookups (40 to a row): 66.8 rows.  Levels:
    y ^ x, index and lookup are 4; the deepest position has 31 pieces, five XORs deep, 10; the fold 8.  A running sum over the 31
    pieces would be 30 XORs, 60 levels, on its own."""
    r48, i48 = built(pkg, 48, True, 1)
    r32, i32 = built(pkg, 32, True, 1)
    p48, j48 = built(pkg, 48, False, 1)
    p32, j32 = built(pkg, 32, False, 1)
    rows = (r48 - r32) - (p48 - p32)
    levels = (i48["num_levels"] - i32["num_levels"]) - (j48["num_levels"] - j32["num_levels"])
    ops = (i48["num_ops"] - i32["num_ops"]) - (j48["num_ops"] - j32["num_ops"])
    print("one more GHASH block at lanes = 1: %d rows, %d ops, %d levels" % (rows, ops, levels))
    assert 0 < rows <= 70
    assert 0 < levels <= 32
    assert ops == 800 + 1072


def test_degree_bits_with_and_without_the_switch(pkg):
    table = []
    for L, off_bits, on_bits in ((16, 13, 14), (64, None, None), (1024, 16, 15)):
        for lanes in (0, 1, 8):
            rows, info = built(pkg, L, True, lanes)
            table.append((L, lanes, rows, info["degree_bits"], info["num_ops"], info["num_levels"]))
            if off_bits is not None:
                assert info["degree_bits"] == (on_bits if lanes else off_bits), (L, lanes)
    print("AES-GCM-128 with the tag (DESIGN.md 9e):\n     L lanes    rows bits      ops  levels")
    for row in table:
        print("%6d %5d %7d %4d %8d %7d" % row)


def test_lanes_shorten_the_chain(pkg):
    def levels(lanes, blocks):
        return K.ghash(pkg, lanes, (blocks,))[0].info["num_levels"]

    one_block = levels(1, 2) - levels(1, 1)
    four_more = levels(4, 8) - levels(4, 4)
    print("levels: one block at lanes = 1: %d; blocks 5..8 at lanes = 4: %d" % (one_block, four_more))
    assert 0 < four_more < 4 * one_block
    assert four_more <= one_block + 2        # one group: the same chain, and one XOR (two levels) to join the other three products


# ------------------------------------------------------------------------------------------ 6. switch off
def test_switch_off_is_the_builder_that_never_heard_of_it(pkg):
    def blob(**kw):
        b = pkg.CircuitBuilder(**kw)
        pkg.AesGcmTarget.build(b, 4, 10, 13, True)
        return b.build().blob

    plain = blob()
    assert blob(ghash_tables=0) == plain
    b = pkg.CircuitBuilder()
    assert pkg.lib().p2_builder_set_ghash_tables(b._h, 3) == 0 and pkg.lib().p2_builder_set_ghash_tables(b._h, 0) == 0   # on, then off again
    pkg.AesGcmTarget.build(b, 4, 10, 13, True)
    assert b.build().blob == plain
    assert blob(ghash_tables=1) != plain
    # without a tag there is no GHASH: the switch changes nothing
    b0, b1 = pkg.CircuitBuilder(), pkg.CircuitBuilder(ghash_tables=2)
    pkg.AesGcmTarget.build(b0, 4, 10, 13, False)
    pkg.AesGcmTarget.build(b1, 4, 10, 13, False)
    assert b0.build().blob == b1.build().blob
