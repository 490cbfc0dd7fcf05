"""Host-side mirror of the reference's operator interface over the C ABI (include/p2aes.h).

Same names and argument meaning as the Rust call sites so the parity tests read like the reference's tests:

    builder = CircuitBuilder()                                  # CircuitBuilder::<F, D>::new(config)
    t = AesGcmTarget.build(builder, nk=4, nr=10, L=13, tag=False)   # aes-gcm/src/circuit_gcm.rs:49
    data = builder.build()                                      # builder.build::<PoseidonGoldilocksConfig>()
    pw = PartialWitness()                                       # PartialWitness::<F>::new()
    t.set_targets(pw, key, nonce, pt, ct, tag)                  # circuit_gcm.rs:174
    proof = data.prove(pw)                                      # data.prove(pw)?   (GPU; raises ProveError)
    data.verify(proof)                                          # data.verify(proof)

PyTorch is not needed here; `prove_batch_device` accepts raw device pointers (e.g. torch tensors' data_ptr()).
"""
import ctypes as C
import os
import struct

P = 0xFFFFFFFF00000001


class P2Error(RuntimeError):
    pass


class ProveError(P2Error):
    """`data.prove(pw)` returned Err (witness conflict, lookup miss, missing input)."""

    def __init__(self, status):
        self.status = status
        super().__init__({1: "witness conflict or lookup input not in table", 2: "a generator never ran (missing input)",
                          3: "opening point is in the subgroup",
                          4: "no proof-of-work witness found"}.get(status, "prove failed (%d)" % status))


# p2_verify_batch verdicts (include/p2aes.h P2_VERIFY_*): the reason class verify_proof would return first
VERIFY_OK, VERIFY_SHAPE, VERIFY_NON_CANONICAL, VERIFY_POW, VERIFY_ZETA_IN_SUBGROUP, VERIFY_VANISHING = 0, 1, 2, 3, 4, 5
VERIFY_MERKLE_INITIAL, VERIFY_FRI_FOLD, VERIFY_MERKLE_FRI, VERIFY_FINAL_POLY = 6, 7, 8, 9
# every reason string of csrc/verifier.h -> its verdict code
VERIFY_REASONS = {
    "": VERIFY_OK,
    "proof truncated": VERIFY_SHAPE,
    "trailing bytes in proof": VERIFY_SHAPE,
    "Merkle path of the wrong depth (initial tree).": VERIFY_SHAPE,
    "Merkle path of the wrong depth (FRI round).": VERIFY_SHAPE,
    "non-canonical field element": VERIFY_NON_CANONICAL,
    "hash word out of range": VERIFY_NON_CANONICAL,  # Keccak circuits: a hash word >= 2^56 (the fourth >= 2^32)
    "Invalid proof-of-work witness.": VERIFY_POW,
    "Opening point is in the subgroup.": VERIFY_ZETA_IN_SUBGROUP,
    "vanishing polynomial identity does not hold at zeta": VERIFY_VANISHING,
    "Invalid Merkle proof (initial tree).": VERIFY_MERKLE_INITIAL,
    "FRI fold consistency check failed.": VERIFY_FRI_FOLD,
    "Invalid Merkle proof (FRI round).": VERIFY_MERKLE_FRI,
    "Final polynomial evaluation is invalid.": VERIFY_FINAL_POLY,
    "wrong number of public inputs": VERIFY_SHAPE,
    # compressed proofs (csrc/compress.h): their layout follows from the written query indices
    "query index out of range": VERIFY_SHAPE,
    "wrong sibling count in compressed proof": VERIFY_SHAPE,
    "query indices differ from the transcript": VERIFY_SHAPE,
}

# p2_witness_explain / p2_host_witness fault kinds (include/p2aes.h P2_FAULT_*), by code
FAULT_KINDS = ("NONE", "INPUT_NOT_CANONICAL", "INPUT_CONFLICT", "LOOKUP_MISS", "GENERATOR_CONFLICT", "NOT_SET")
# witness generator kinds (csrc/circuit.h OP_*), by code
OP_KINDS = ("ARITH", "CONST", "LOOKUP", "EQ", "EQINV", "POSEIDON", "LIMB", "ECSTEP")
VALUE_UNSET = 0xFFFFFFFFFFFFFFFF   # P2_VALUE_UNSET: "not assigned" on input, "the run did not determine it" on output

u32p = C.POINTER(C.c_uint32)


def lib_path():
    return os.environ.get("P2AES_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libp2aes.so")


_lib = None
u64, u8p, u64p, u16p, sz = C.c_uint64, C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_uint16), C.c_size_t


class _Info(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("degree_bits", "num_wires", "num_routed_wires", "num_constants_cols", "num_zs_cols",
                                           "num_quotient_cols", "num_luts", "num_ops", "num_levels", "num_slots",
                                           "num_virtual_targets", "num_fri_rounds")] + [("proof_bytes", C.c_uint64), ("zero_knowledge", C.c_uint32),
                                                                                      ("num_gate_kinds", C.c_uint32),
                                                                                      ("num_public_inputs", C.c_uint32),
                                                                                      ("hasher", C.c_uint32)]


# the tree hasher of a circuit (include/p2aes.h P2_HASHER_*): PoseidonGoldilocksConfig / KeccakGoldilocksConfig
HASHERS = {"poseidon": 0, "keccak": 1}


class _Assignment(C.Structure):
    _fields_ = [("targets", u64p), ("values", u64p), ("count", sz)]


class _Fault(C.Structure):
    _fields_ = [("kind", C.c_int32), ("op_kind", C.c_int32), ("input_index", C.c_int64), ("target", C.c_uint64), ("gate_row", C.c_uint32),
                ("computed", C.c_uint64), ("found", C.c_uint64)]


class WitnessFault:
    """p2_witness_fault as a record: kind (a FAULT_KINDS name), op_kind (an OP_KINDS name or None), input_index, target and
    gate_row (None where the C struct says "none"), computed, found."""

    def __init__(self, f, status):
        self.status = status
        self.kind = FAULT_KINDS[f.kind]
        self.op_kind = OP_KINDS[f.op_kind] if f.op_kind >= 0 else None
        self.input_index = f.input_index if f.input_index >= 0 else None
        self.target = f.target if f.target != VALUE_UNSET else None
        self.gate_row = f.gate_row if f.gate_row != 0xFFFFFFFF else None
        self.computed, self.found = f.computed, f.found

    def _key(self):
        return (self.status, self.kind, self.op_kind, self.input_index, self.target, self.gate_row, self.computed, self.found)

    def __eq__(self, other): return isinstance(other, WitnessFault) and self._key() == other._key()
    def __hash__(self): return hash(self._key())

    def __repr__(self):
        return "WitnessFault(status=%d, kind=%s, op_kind=%s, input_index=%s, target=%s, gate_row=%s, computed=%d, found=%d)" % self._key()

    def __str__(self):
        if self.kind == "NONE":
            return "no fault"
        where = "target %s" % ("none" if self.target is None else "%#x" % self.target)
        if self.input_index is not None:
            where += " (entry %d of the assignment)" % self.input_index
        return {"INPUT_NOT_CANONICAL": "value %d of %s is not a canonical field element" % (self.found, where),
                "INPUT_CONFLICT": "%s is set to %d but an earlier entry of its slot sets %d" % (where, self.found, self.computed),
                "LOOKUP_MISS": "lookup input %d at %s is not in its table" % (self.found, where),
                "GENERATOR_CONFLICT": "%s generator computes %d for %s, which holds %d" % (self.op_kind, self.computed, where, self.found),
                "NOT_SET": "%s is needed and was never set" % where}[self.kind]


def _assignment(pw_or_map):
    """(struct, keep-alive) of one PartialWitness or target -> value mapping; values are passed as they are."""
    m = pw_or_map.map if hasattr(pw_or_map, "map") else pw_or_map
    ts, vs = _arr(list(m.keys())), _arr(list(m.values()))
    a = _Assignment()
    a.targets, a.values, a.count = C.cast(ts, u64p), C.cast(vs, u64p), len(m)
    return a, (ts, vs)


def host_witness(blob, pw, outputs=(), explain=True):
    """p2_host_witness: the host twin of generate_witness / explain for one witness, from the blob alone (no device).
    Returns (values of `outputs`, status, WitnessFault or None)."""
    a, keep = _assignment(pw)
    outs = list(outputs)
    vals = (u64 * max(len(outs), 1))()
    st, f = C.c_int(), _Fault()
    if lib().p2_host_witness(blob, len(blob), C.byref(a), _arr(outs) if outs else None, len(outs), vals, C.byref(st), C.byref(f) if explain else None):
        raise P2Error("p2_host_witness failed: " + _err())
    return list(vals[: len(outs)]), st.value, (WitnessFault(f, st.value) if explain else None)


class _KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("ms", C.c_float), ("count", C.c_uint32)]


def lib():
    """Load the shared library; fails loudly if the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise P2Error("native library %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`" % path)
    L = C.CDLL(path)
    vp = C.c_void_p
    sig = {
        "p2_last_error": (C.c_char_p, []),
        "p2_builder_new": (vp, []), "p2_builder_new_zk": (vp, []), "p2_builder_free": (None, [vp]),
        "p2_builder_new_config": (vp, [C.c_int, C.c_int]), "p2_builder_set_hasher": (C.c_int, [vp, C.c_int]),
        "p2_native_keccak_hash_no_pad": (None, [u64p, sz, u64p]), "p2_native_keccak_two_to_one": (None, [u64p, u64p, u64p]),
        "p2_native_keccak256": (None, [C.c_char_p, sz, C.c_char_p]),
        "p2_gpu_merkle_cap_hasher": (C.c_int, [u64p, sz, sz, C.c_int, C.c_int, u64p, C.c_int]),
        "p2_circuit_set_zk_seed": (C.c_int, [vp, u64]),
        "p2_circuit_set_zk_key": (C.c_int, [vp, C.POINTER(u64)]),
        "p2_circuit_set_option": (C.c_int, [vp, C.c_char_p, C.c_long]),
        "p2_prove_batch_multi": (C.c_int, [C.POINTER(vp), sz, sz, C.POINTER(_Assignment), C.c_char_p, C.POINTER(C.c_int)]),
        "p2_builder_add_virtual_target": (u64, [vp]), "p2_builder_constant": (u64, [vp, u64]),
        "p2_builder_zero": (u64, [vp]), "p2_builder_one": (u64, [vp]),
        "p2_builder_arithmetic": (u64, [vp, u64, u64, u64, u64, u64]),
        "p2_builder_mul_const_add": (u64, [vp, u64, u64, u64]),
        "p2_builder_add": (u64, [vp, u64, u64]), "p2_builder_sub": (u64, [vp, u64, u64]), "p2_builder_mul": (u64, [vp, u64, u64]),
        "p2_builder_select": (u64, [vp, u64, u64, u64]), "p2_builder_is_equal": (u64, [vp, u64, u64]),
        "p2_builder_connect": (None, [vp, u64, u64]),
        "p2_builder_assert_bool": (C.c_int, [vp, u64]), "p2_builder_range_check": (C.c_int, [vp, u64, sz]),
        "p2_builder_le_sum": (C.c_int, [vp, u64p, sz, u64p]), "p2_builder_le_bytes_sum": (C.c_int, [vp, u64p, sz, u64p]),
        "p2_builder_split_le": (C.c_int, [vp, u64, sz, u64p]), "p2_builder_split_bytes_le": (C.c_int, [vp, u64, sz, sz, u64p]),
        "p2_builder_is_less_than": (C.c_int, [vp, u64, u64, sz, u64p]),
        "p2_builder_register_public_input": (C.c_int, [vp, u64]),
        "p2_proof_public_inputs": (C.c_int, [C.c_char_p, sz, C.c_char_p, sz, u64p, sz, C.POINTER(sz)]),
        "p2_builder_add_lookup_table_from_pairs": (sz, [vp, u16p, sz]),
        "p2_builder_add_lookup_from_index": (u64, [vp, u64, sz]),
        "p2_builder_num_gates": (sz, [vp]),
        "p2_builder_build": (C.c_int, [vp, C.POINTER(u8p), C.POINTER(sz)]), "p2_blob_free": (None, [u8p]),
        "p2_aes_sbox_lut": (sz, [vp]), "p2_aes_byte_xor_lut": (sz, [vp]), "p2_aes_gf_2_8_mul_lut": (sz, [vp]),
        "p2_gcm_u8_unit_right_shift_lut": (sz, [vp]), "p2_gcm_u8_bitref_lut": (sz, [vp]),
        "p2_aes_add_virtual_byte_target": (u64, [vp, sz]), "p2_aes_add_virtual_byte_target_unsafe": (u64, [vp]),
        "p2_aes_state_sub_bytes": (None, [vp, sz, u64p, u64p]),
        "p2_aes_state_mix_columns": (None, [vp, sz, sz, u64p, u64p]),
        "p2_aes_gf_2_8_mul": (u64, [vp, sz, u64, u64]), "p2_aes_gf_2_8_add": (u64, [vp, sz, u64, u64]),
        "p2_aes_key_expansion": (None, [vp, C.c_int, C.c_int, sz, sz, u64p, u64p]),
        "p2_aes_encrypt_block": (None, [vp, C.c_int, sz, sz, sz, u64p, u64p, u64p]),
        "p2_gcm_gctr": (None, [vp, C.c_int, sz, sz, sz, u64p, u64p, u64p, sz, u64p]),
        "p2_gcm_right_shift_one": (None, [vp, sz, u64p, u64p]), "p2_gcm_inc32": (None, [vp, u64p, u64p]),
        "p2_gcm_gf_2_128_mul": (None, [vp, sz, sz, sz, u64p, u64p, u64p]),
        "p2_gcm_ghash": (C.c_int, [vp, sz, sz, sz, u64p, u64p, sz, u64p]),
        "p2_gcm_clmul_lo_lut": (sz, [vp]), "p2_gcm_clmul_hi_lut": (sz, [vp]),
        "p2_gcm_gf_2_128_mul_tables": (C.c_int, [vp, sz, sz, sz, u64p, u64p, u64p]),
        "p2_gcm_ghash_tables": (C.c_int, [vp, sz, sz, sz, u64p, u64p, sz, u64p, C.c_int]),
        "p2_builder_set_ghash_tables": (C.c_int, [vp, C.c_int]),
        "p2_aes_gcm_build": (C.c_int, [vp, C.c_int, C.c_int, sz, C.c_int, u64p, u64p, u64p, u64p, u64p]),
        "p2_builder_hash_n_to_m_no_pad": (C.c_int, [vp, u64p, sz, u64p, sz]),
        "p2_poseidon_cipher_build": (C.c_int, [vp, sz, u64p, u64p, u64p, u64p]),
        "p2_native_hash_n_to_m_no_pad": (None, [u64p, sz, u64p, sz]),
        "p2_native_poseidon_encrypt": (None, [u64p, u64p, sz, u64p, u64p]),
        "p2_native_poseidon_decrypt": (C.c_int, [u64p, u64p, sz, u64p, sz, u64p]),
        "p2_ecgfp5_group_order": (None, [u64p]), "p2_ecgfp5_generator": (None, [u64p]),
        "p2_ecgfp5_mul": (None, [u64p, u64p, u64p]), "p2_ecgfp5_add": (None, [u64p, u64p, u64p]), "p2_ecgfp5_neg": (None, [u64p, u64p]),
        "p2_ecgfp5_is_in_subgroup": (C.c_int, [u64p]),
        "p2_ecgfp5_compress": (None, [u64p, u64p]), "p2_ecgfp5_decompress": (C.c_int, [u64p, u64p]),
        "p2_ecgfp5_random_scalar": (C.c_int, [u64p]), "p2_ecgfp5_random_point": (C.c_int, [u64p]),
        "p2_ecgfp5_encode_binary": (C.c_int, [u32p, u64p]),
        "p2_ecgfp5_random_scalar_seeded": (None, [u64, u64p]), "p2_ecgfp5_random_point_seeded": (None, [u64, u64p]),
        "p2_ecgfp5_encode_binary_seeded": (None, [u32p, u64, u64p]), "p2_ecgfp5_decode_binary": (None, [u64p, u32p]),
        "p2_elgamal_encrypt": (C.c_int, [u64p, u64p, u64p, u64p, u64p]), "p2_elgamal_decrypt": (C.c_int, [u64p, u64p, u64p, u64p]),
        "p2_hashed_elgamal_encrypt": (C.c_int, [u64p, u64p, u64p, u64p, u64p]),
        "p2_hashed_elgamal_decrypt": (C.c_int, [u64p, u64p, u64p, u64p]),
        "p2_builder_add_virtual_point_target": (None, [vp, u64p]), "p2_builder_constant_point": (None, [vp, u64p, u64p]),
        "p2_builder_add_virtual_biguint320_target": (None, [vp, u64p]),
        "p2_builder_multiply_point": (C.c_int, [vp, u64p, u64p, u64p]), "p2_builder_add_point": (None, [vp, u64p, u64p, u64p]),
        "p2_builder_public_key": (C.c_int, [vp, u64p, u64p]),
        "p2_builder_set_ec_gate": (C.c_int, [vp, C.c_int]), "p2_builder_ec_step": (C.c_int, [vp, u64p, u64p, u64, C.c_int, u64p, u64p]),
        "p2_builder_elgamal_encrypt": (C.c_int, [vp, u64p, u64p, u64p, u64p, u64p]),
        "p2_builder_hashed_elgamal_encrypt": (C.c_int, [vp, u64p, u64p, u64p, u64p, u64p]),
        "p2_selftest_host": (C.c_int, [u64, sz, sz]), "p2_selftest_device": (C.c_int, [u64, sz, C.c_int]),
        "p2_selftest_lazy_device": (C.c_int, [u64, sz, C.c_int]),
        "p2_selftest_ntt_device": (C.c_int, [u64, sz, C.c_int]),
        "p2_native_gf_2_8_mul": (C.c_uint8, [C.c_uint8, C.c_uint8]),
        "p2_native_aes_key_expansion": (None, [C.c_char_p, C.c_int, C.c_int, C.c_char_p]),
        "p2_native_aes_encrypt_block": (None, [C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_char_p]),
        "p2_native_gf_2_128_mul": (None, [C.c_char_p, C.c_char_p, C.c_char_p]),
        "p2_native_ghash": (None, [C.c_char_p, C.c_char_p, sz, C.c_char_p]),
        "p2_native_gctr": (None, [C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_char_p, sz, C.c_char_p]),
        "p2_native_aes_gcm_encrypt": (None, [C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_char_p, sz, C.c_char_p, C.c_char_p]),
        "p2_native_aes_gcm_encrypt_aad": (None, [C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_char_p, sz, C.c_char_p, sz, C.c_char_p, C.c_char_p]),
        "p2_native_aes_gcm_decrypt": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_char_p, sz, C.c_char_p, sz, C.c_char_p, C.c_char_p]),
        "p2_aes_gcm_build_aad": (C.c_int, [vp, C.c_int, C.c_int, sz, C.c_int, sz, u64p, u64p, u64p, u64p, u64p, u64p]),
        "p2_blob_info": (C.c_int, [C.c_char_p, sz, C.POINTER(_Info)]),
        "p2_witness_schedule_check": (C.c_int, [C.c_char_p, sz, C.c_uint32, u32p]),
        "p2_verify": (C.c_int, [C.c_char_p, sz, u64p, sz, C.c_char_p, sz]),
        "p2_vanishing_terms": (C.c_int, [C.c_char_p, sz, C.c_char_p, sz, u64p, u64p, u64p, sz, C.POINTER(sz), u64p, C.POINTER(C.c_int)]),
        "p2_gpu_vanishing_flags": (C.c_int, [vp, sz, C.c_char_p, u64p, u64p, u32p]),
        "p2_proof_compress": (C.c_int, [C.c_char_p, sz, u64p, sz, C.c_char_p, sz, C.c_char_p, sz, C.POINTER(sz)]),
        "p2_proof_decompress": (C.c_int, [C.c_char_p, sz, u64p, sz, C.c_char_p, sz, C.c_char_p, sz, C.POINTER(sz)]),
        "p2_verify_compressed": (C.c_int, [C.c_char_p, sz, u64p, sz, C.c_char_p, sz]),
        "p2_circuit_load": (vp, [C.c_char_p, sz, C.c_int]), "p2_circuit_free": (None, [vp]),
        "p2_circuit_verifier_data": (C.c_int, [vp, u64p, sz, C.POINTER(sz)]),
        "p2_circuit_proof_bytes": (sz, [vp]),
        "p2_circuit_num_public_inputs": (sz, [vp]),
        "p2_circuit_public_inputs": (C.c_int, [vp, C.c_char_p, sz, u64p, sz, C.POINTER(sz)]),
        "p2_circuit_chunk_proofs": (sz, [vp]),
        "p2_prove_batch": (C.c_int, [vp, sz, C.POINTER(_Assignment), C.c_char_p, C.POINTER(C.c_int)]),
        "p2_prove_batch_device": (C.c_int, [vp, sz, u64p, sz, vp, vp, vp, vp]),
        "p2_circuit_synchronize": (C.c_int, [vp]),
        "p2_prove_batch_outputs": (C.c_int, [vp, sz, C.POINTER(_Assignment), u64p, sz, u64p, C.c_char_p, C.POINTER(C.c_int)]),
        "p2_prove_batch_outputs_device": (C.c_int, [vp, sz, u64p, sz, vp, u64p, sz, vp, vp, vp, vp]),
        "p2_witness_batch": (C.c_int, [vp, sz, C.POINTER(_Assignment), u64p, sz, u64p, C.POINTER(C.c_int)]),
        "p2_witness_batch_device": (C.c_int, [vp, sz, u64p, sz, vp, u64p, sz, vp, vp, vp]),
        "p2_witness_explain": (C.c_int, [vp, C.POINTER(_Assignment), C.POINTER(C.c_int), vp]),
        "p2_host_witness": (C.c_int, [C.c_char_p, sz, C.POINTER(_Assignment), u64p, sz, u64p, C.POINTER(C.c_int), vp]),
        "p2_verify_batch": (C.c_int, [vp, sz, C.c_char_p, u64p, sz, C.POINTER(C.c_int)]),
        "p2_verify_batch_device": (C.c_int, [vp, sz, vp, u64p, sz, vp, vp]),
        "p2_compress_batch": (C.c_int, [vp, sz, C.c_char_p, u64p, sz, C.c_char_p, u32p, C.POINTER(C.c_int)]),
        "p2_compress_batch_device": (C.c_int, [vp, sz, vp, u64p, sz, vp, vp, vp, vp]),
        "p2_decompress_batch": (C.c_int, [vp, sz, C.c_char_p, u32p, u64p, sz, C.c_char_p, C.POINTER(C.c_int)]),
        "p2_decompress_batch_device": (C.c_int, [vp, sz, vp, vp, u64p, sz, vp, vp, vp]),
        "p2_verify_compressed_batch": (C.c_int, [vp, sz, C.c_char_p, u32p, u64p, sz, C.POINTER(C.c_int)]),
        "p2_verify_compressed_batch_device": (C.c_int, [vp, sz, vp, vp, u64p, sz, vp, vp]),
        "p2_circuit_set_timing": (C.c_int, [vp, C.c_int]),
        "p2_circuit_get_timing": (sz, [vp, C.POINTER(_KernelTime), sz]),
        "p2_gpu_device_count": (C.c_int, []),
        "p2_gpu_poseidon": (C.c_int, [u64p, sz, C.c_int]),
        "p2_host_partial_rounds": (C.c_int, [u64p, sz]),
        "p2_gpu_partial_rounds": (C.c_int, [u64p, sz, C.c_int]),
        "p2_host_merged_middle": (C.c_int, [u64p, sz]),
        "p2_gpu_merged_middle": (C.c_int, [u64p, sz, C.c_int]),
        "p2_host_ecstep_constraints": (C.c_int, [u64p, sz, u64p]), "p2_host_ecstep_constraints_ext": (C.c_int, [u64p, sz, u64p]),
        "p2_gpu_ecstep_constraints": (C.c_int, [u64p, sz, u64p, C.c_int]),
        "p2_gpu_lde": (C.c_int, [u64p, sz, C.c_int, C.c_int, u64p, C.c_int]),
        "p2_gpu_intt": (C.c_int, [u64p, sz, C.c_int, u64p, C.c_int]),
        "p2_gpu_lde_round": (C.c_int, [u64p, sz, C.c_int, u32p, sz, sz, sz, sz, u64p, sz, C.c_int]),
        "p2_gpu_quotient_chunks": (C.c_int, [u64p, sz, C.c_int, sz, u64p, C.c_int]),
        "p2_gpu_merkle_cap": (C.c_int, [u64p, sz, sz, C.c_int, u64p, C.c_int]),
        "p2_gpu_zeta_pows": (C.c_int, [u64p, sz, u64p, C.c_int]),
        "p2_circuit_debug_read": (C.c_int, [vp, C.c_char_p, sz, u64p, sz, C.POINTER(sz)]),
        "p2_debug_live_resources": (sz, []),
        "p2_builder_permute_swapped": (C.c_int, [vp, u64p, u64, u64p]), "p2_builder_hash_or_noop": (C.c_int, [vp, u64p, sz, u64p]),
        "p2_builder_add_virtual_hash": (C.c_int, [vp, u64p]), "p2_builder_add_virtual_cap": (C.c_int, [vp, C.c_int, u64p]),
        "p2_builder_connect_hashes": (C.c_int, [vp, u64p, u64p]),
        "p2_builder_verify_merkle_proof_to_cap": (C.c_int, [vp, u64p, sz, u64p, sz, u64p, C.c_int, u64p, sz]),
        "p2_builder_verify_merkle_proof": (C.c_int, [vp, u64p, sz, u64p, sz, u64p, u64p, sz]),
        "p2_native_merkle_cap": (C.c_int, [u64p, sz, sz, C.c_int, u64p]),
        "p2_native_merkle_prove": (C.c_int, [u64p, sz, sz, C.c_int, sz, u64p]),
        "p2_native_merkle_verify": (C.c_int, [u64p, sz, sz, u64p, sz, u64p, C.c_int, C.POINTER(C.c_int)]),
        "p2_merkle_tree_new": (C.c_int, [u64p, sz, sz, C.c_int, C.c_int, C.POINTER(vp)]),
        "p2_merkle_tree_new_device": (C.c_int, [vp, sz, sz, C.c_int, C.c_int, vp, C.POINTER(vp)]),
        "p2_merkle_tree_free": (None, [vp]), "p2_merkle_tree_cap": (C.c_int, [vp, u64p, sz]),
        "p2_merkle_tree_prove_batch": (C.c_int, [vp, u64p, sz, u64p]),
        "p2_merkle_tree_prove_batch_device": (C.c_int, [vp, vp, sz, vp, sz, vp, vp]),
        "p2_merkle_verify_batch": (C.c_int, [u64p, sz, u64p, u64p, sz, u64p, C.c_int, sz, C.POINTER(C.c_int), C.c_int]),
        "p2_merkle_verify_batch_device": (C.c_int, [vp, sz, vp, vp, sz, vp, C.c_int, sz, vp, C.c_int, vp]),
        "p2_gpu_merkle_build_device": (C.c_int, [vp, sz, sz, C.c_int, C.c_int, vp, vp, C.c_int, vp]),
        "p2_native_merkle_update": (C.c_int, [u64p, sz, sz, C.c_int, u64p, u64p, sz, u64p, u64p]),
        "p2_merkle_tree_update": (C.c_int, [vp, u64p, u64p, sz, u64p, u64p]),
        "p2_merkle_tree_update_device": (C.c_int, [vp, vp, vp, sz, vp, sz, vp, sz, vp, vp]),
        "p2_merkle_tree_last_update_hashes": (C.c_int, [vp, u64p]),
        "p2_builder_merkle_update_to_cap": (C.c_int, [vp, u64p, u64p, sz, u64p, sz, u64p, C.c_int, u64p, sz, u64p]),
        "p2_builder_merkle_update": (C.c_int, [vp, u64p, u64p, sz, u64p, sz, u64p, u64p, sz, u64p]),
        "p2_builder_merkle_map_lookup_to_cap": (C.c_int, [vp, u64p, sz, u64p, sz, u64, u64p, C.c_int, u64p, sz]),
        "p2_builder_merkle_map_lookup": (C.c_int, [vp, u64p, sz, u64p, sz, u64, u64p, u64p, sz]),
        "p2_builder_merkle_map_update_to_cap": (C.c_int, [vp, u64p, sz, u64, u64p, u64, u64p, sz, u64p, C.c_int, u64p, sz, u64p]),
        "p2_builder_merkle_map_update": (C.c_int, [vp, u64p, sz, u64, u64p, u64, u64p, sz, u64p, u64p, sz, u64p]),
        "p2_builder_merkle_map_insert_to_cap": (C.c_int, [vp, u64p, sz, u64p, sz, u64p, C.c_int, u64p, sz, u64p]),
        "p2_builder_merkle_map_insert": (C.c_int, [vp, u64p, sz, u64p, sz, u64p, u64p, sz, u64p]),
        "p2_builder_merkle_map_remove_to_cap": (C.c_int, [vp, u64p, sz, u64p, sz, u64p, C.c_int, u64p, sz, u64p]),
        "p2_builder_merkle_map_remove": (C.c_int, [vp, u64p, sz, u64p, sz, u64p, u64p, sz, u64p]),
        "p2_native_merkle_map_cap": (C.c_int, [u64p, u64p, sz, sz, C.c_int, C.c_int, u64p]),
        "p2_native_merkle_map_get": (C.c_int, [u64p, u64p, sz, sz, C.c_int, C.c_int, u64, C.POINTER(C.c_int), u64p, u64p]),
        "p2_native_merkle_map_verify": (C.c_int, [u64, C.c_int, u64, u64p, sz, u64p, u64p, C.c_int, C.POINTER(C.c_int)]),
        "p2_merkle_map_new": (C.c_int, [u64p, u64p, sz, sz, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
        "p2_merkle_map_new_device": (C.c_int, [vp, vp, sz, sz, C.c_int, C.c_int, C.c_int, vp, C.POINTER(vp)]),
        "p2_merkle_map_free": (None, [vp]), "p2_merkle_map_cap": (C.c_int, [vp, u64p, sz]),
        "p2_merkle_map_len": (C.c_int, [vp, C.POINTER(sz)]), "p2_merkle_map_hashes": (C.c_int, [vp, u64p]),
        "p2_merkle_map_get_batch": (C.c_int, [vp, u64p, sz, u64p, u64p, u64p]),
        "p2_merkle_map_get_batch_device": (C.c_int, [vp, vp, sz, vp, sz, sz, sz, sz, vp, vp]),
        "p2_merkle_map_verify_batch": (C.c_int, [u64p, C.c_int, u64p, u64p, sz, u64p, u64p, C.c_int, sz, C.POINTER(C.c_int), C.c_int]),
        "p2_merkle_map_verify_batch_device": (C.c_int, [vp, C.c_int, vp, vp, sz, vp, vp, C.c_int, sz, vp, C.c_int, vp]),
        "p2_ecgfp5_scalar_muladd": (None, [u64p, u64p, u64p, u64p]),
        "p2_gpu_ecgfp5_scalar_muladd": (C.c_int, [u64p, u64p, u64p, sz, u64p, C.c_int]),
        "p2_schnorr_challenge": (C.c_int, [u64p, u64p, u64p, sz, u64p]),
        "p2_schnorr_sign": (C.c_int, [u64p, u64p, u64p, sz, u64p, u64p, C.POINTER(C.c_int)]),
        "p2_schnorr_verify": (C.c_int, [u64p, u64p, sz, u64p, C.POINTER(C.c_int)]),
        "p2_builder_add_virtual_schnorr_signature": (C.c_int, [vp, u64p, u64p]),
        "p2_builder_verify_schnorr_signature": (C.c_int, [vp, u64p, u64p, sz, u64p, u64p, u64p]),
        "p2_ecgfp5_mul_batch": (C.c_int, [u64p, u64p, sz, u64p, C.POINTER(C.c_int), C.c_int]),
        "p2_ecgfp5_mul_batch_device": (C.c_int, [vp, vp, sz, vp, vp, C.c_int, vp]),
        "p2_schnorr_sign_batch": (C.c_int, [u64p, u64p, u64p, sz, sz, u64p, u64p, C.POINTER(C.c_int), C.c_int]),
        "p2_schnorr_sign_batch_device": (C.c_int, [vp, vp, vp, sz, sz, vp, vp, vp, C.c_int, vp]),
        "p2_schnorr_verify_batch": (C.c_int, [u64p, u64p, sz, u64p, sz, C.POINTER(C.c_int), C.c_int]),
        "p2_schnorr_verify_batch_device": (C.c_int, [vp, vp, sz, vp, sz, vp, C.c_int, vp]),
        "p2_ecgfp5_encode_binary_padded": (C.c_int, [u32p, u32p, sz, u64p, u32p]),
        "p2_builder_neg_point": (C.c_int, [vp, u64p, u64p]),
        "p2_builder_elgamal_decrypt": (C.c_int, [vp, u64p, u64p, u64p, u64p]),
        "p2_builder_hashed_elgamal_decrypt": (C.c_int, [vp, u64p, u64p, u64p, u64p]),
        "p2_ecgfp5_decompress_batch": (C.c_int, [u64p, sz, u64p, C.POINTER(C.c_int), C.c_int]),
        "p2_ecgfp5_decompress_batch_device": (C.c_int, [vp, sz, vp, vp, C.c_int, vp]),
        "p2_ecgfp5_encode_binary_batch": (C.c_int, [u32p, u32p, sz, sz, u64p, u32p, C.POINTER(C.c_int), C.c_int]),
        "p2_ecgfp5_encode_binary_batch_device": (C.c_int, [vp, vp, sz, sz, vp, vp, vp, C.c_int, vp]),
        "p2_elgamal_encrypt_batch": (C.c_int, [u64p, u64p, u64p, sz, u64p, u64p, C.POINTER(C.c_int), C.c_int]),
        "p2_elgamal_encrypt_batch_device": (C.c_int, [vp, vp, vp, sz, vp, vp, vp, C.c_int, vp]),
        "p2_elgamal_decrypt_batch": (C.c_int, [u64p, u64p, u64p, sz, u64p, C.POINTER(C.c_int), C.c_int]),
        "p2_elgamal_decrypt_batch_device": (C.c_int, [vp, vp, vp, sz, vp, vp, C.c_int, vp]),
        "p2_hashed_elgamal_encrypt_batch": (C.c_int, [u64p, u64p, u64p, sz, u64p, u64p, C.POINTER(C.c_int), C.c_int]),
        "p2_hashed_elgamal_encrypt_batch_device": (C.c_int, [vp, vp, vp, sz, vp, vp, vp, C.c_int, vp]),
        "p2_hashed_elgamal_decrypt_batch": (C.c_int, [u64p, u64p, u64p, sz, u64p, C.POINTER(C.c_int), C.c_int]),
        "p2_hashed_elgamal_decrypt_batch_device": (C.c_int, [vp, vp, vp, sz, vp, vp, C.c_int, vp]),
        "p2_ecgfp5_scalar_bits_device": (C.c_int, [vp, sz, vp, sz, C.c_int, vp]),
        "p2_host_pcipher_hash_state": (C.c_int, [u64p, C.c_int, u64p]),
        "p2_builder_poseidon_encrypt": (C.c_int, [vp, u64p, u64p, u64p, sz, u64p]),
        "p2_builder_poseidon_decrypt": (C.c_int, [vp, u64p, u64p, u64p, sz, u64p]),
        "p2_poseidon_encrypt_batch": (C.c_int, [u64p, u64p, u64p, sz, sz, u64p, C.POINTER(C.c_int), C.c_int]),
        "p2_poseidon_encrypt_batch_device": (C.c_int, [vp, vp, vp, sz, sz, vp, vp, C.c_int, vp]),
        "p2_poseidon_decrypt_batch": (C.c_int, [u64p, u64p, u64p, sz, sz, u64p, C.POINTER(C.c_int), C.c_int]),
        "p2_poseidon_decrypt_batch_device": (C.c_int, [vp, vp, vp, sz, sz, vp, vp, C.c_int, vp]),
        "p2_aes_gcm_batch_workspace": (sz, [C.c_int, sz, sz, sz]),
        "p2_aes_gcm_encrypt_batch": (C.c_int, [C.c_char_p, C.c_int, C.c_char_p, C.c_char_p, sz, C.c_char_p, sz, sz, C.c_char_p, C.c_char_p, C.POINTER(C.c_int), C.c_int]),
        "p2_aes_gcm_decrypt_batch": (C.c_int, [C.c_char_p, C.c_int, C.c_char_p, C.c_char_p, sz, C.c_char_p, C.c_char_p, sz, sz, C.c_char_p, C.POINTER(C.c_int), C.c_int]),
        "p2_aes_gcm_encrypt_batch_device": (C.c_int, [vp, C.c_int, vp, vp, sz, vp, sz, sz, sz, vp, vp, vp, vp, C.c_int, vp]),
        "p2_aes_gcm_decrypt_batch_device": (C.c_int, [vp, C.c_int, vp, vp, sz, vp, vp, sz, sz, sz, vp, vp, vp, C.c_int, vp]),
        "p2_bytes_to_words_device": (C.c_int, [vp, sz, sz, sz, vp, sz, C.c_int, vp]),
        "p2_gpu_gcm_ghash": (C.c_int, [C.c_char_p, C.c_char_p, sz, sz, C.c_int, C.c_char_p, C.c_int]),
        "p2_gpu_aes_encrypt_blocks": (C.c_int, [C.c_char_p, C.c_int, C.c_char_p, sz, C.c_char_p, C.c_int]),
        "p2_gpu_gcm_kernel_times": (C.c_int, [C.c_int, sz, sz, sz, C.c_int, sz, u64p, C.c_int]),
    }
    missing = []
    for name, (res, args) in sig.items():
        try:
            f = getattr(L, name)
        except AttributeError:
            missing.append(name)
            continue
        f.restype, f.argtypes = res, args
    L._p2_missing = missing
    L._p2_signatures = sig
    _lib = L
    return L


def _err():
    return lib().p2_last_error().decode()


def _arr(vals):
    return (u64 * len(vals))(*vals)


class CircuitBuilder:
    def __init__(self, zero_knowledge=False, hasher="poseidon", ec_gate=False, ghash_tables=0):
        """CircuitBuilder::<F, D>::new(standard_recursion_config()) or, with zero_knowledge, standard_recursion_zk_config().
        hasher: "poseidon" (build::<PoseidonGoldilocksConfig>()) or "keccak" (build::<KeccakGoldilocksConfig>(): Keccak-256
        Merkle trees and circuit digest); everything made from the circuit afterwards takes the hasher from it.
        ec_gate: multiply_point (and public_key, elgamal_encrypt, hashed_elgamal_encrypt) as 320 EcStepGate rows.
        ghash_tables: 0, or 1 to 16 lanes: AesGcmTarget.build with a tag computes GHASH from carry-less multiply tables."""
        if hasher not in HASHERS:
            raise P2Error("unknown hasher %r (known: %s)" % (hasher, ", ".join(sorted(HASHERS))))
        if hasher == "poseidon":
            self._h = lib().p2_builder_new_zk() if zero_knowledge else lib().p2_builder_new()
        else:
            self._h = lib().p2_builder_new_config(1 if zero_knowledge else 0, HASHERS[hasher])
        if not self._h:
            raise P2Error(_err())
        if ec_gate and lib().p2_builder_set_ec_gate(self._h, 1):
            raise P2Error(_err())
        if ghash_tables != 0 and lib().p2_builder_set_ghash_tables(self._h, ghash_tables):
            raise P2Error(_err())

    def __del__(self):
        if getattr(self, "_h", None):
            lib().p2_builder_free(self._h)
            self._h = None

    def add_virtual_target(self): return lib().p2_builder_add_virtual_target(self._h)
    def add_virtual_target_arr(self, n): return [self.add_virtual_target() for _ in range(n)]
    def constant(self, c): return lib().p2_builder_constant(self._h, c % P)
    def zero(self): return lib().p2_builder_zero(self._h)
    def one(self): return lib().p2_builder_one(self._h)
    def arithmetic(self, c0, c1, m0, m1, addend): return lib().p2_builder_arithmetic(self._h, c0 % P, c1 % P, m0, m1, addend)
    def mul_const_add(self, c, x, y): return lib().p2_builder_mul_const_add(self._h, c % P, x, y)
    def add(self, x, y): return lib().p2_builder_add(self._h, x, y)
    def sub(self, x, y): return lib().p2_builder_sub(self._h, x, y)
    def mul(self, x, y): return lib().p2_builder_mul(self._h, x, y)
    def select(self, b, x, y): return lib().p2_builder_select(self._h, b, x, y)
    def is_equal(self, x, y): return lib().p2_builder_is_equal(self._h, x, y)
    def connect(self, x, y): lib().p2_builder_connect(self._h, x, y)

    # ---- bits and bytes of a field element (little-endian; include/p2aes.h has the rules)
    def assert_bool(self, t):
        if lib().p2_builder_assert_bool(self._h, t):
            raise P2Error(_err())

    def _sum(self, fn, limbs):
        out = (u64 * 1)()
        if fn(self._h, _arr(limbs), len(limbs), out):
            raise P2Error(_err())
        return out[0]

    def le_sum(self, bits): return self._sum(lib().p2_builder_le_sum, bits)
    def le_bytes_sum(self, byte_targets): return self._sum(lib().p2_builder_le_bytes_sum, byte_targets)

    def split_le(self, x, num_bits):
        out = (u64 * max(min(int(num_bits), 64), 1))()
        if lib().p2_builder_split_le(self._h, x, num_bits, out):
            raise P2Error(_err())
        return list(out)

    def range_check(self, x, num_bits):
        if lib().p2_builder_range_check(self._h, x, num_bits):
            raise P2Error(_err())

    def split_bytes_le(self, x, num_bytes, u8_table_idx):
        out = (u64 * max(min(int(num_bytes), 8), 1))()
        if lib().p2_builder_split_bytes_le(self._h, x, num_bytes, u8_table_idx, out):
            raise P2Error(_err())
        return list(out)

    def is_less_than(self, a, b, num_bits):
        out = (u64 * 1)()
        if lib().p2_builder_is_less_than(self._h, a, b, num_bits, out):
            raise P2Error(_err())
        return out[0]

    def register_public_input(self, t):
        """CircuitBuilder::register_public_input: every proof carries the target's value (in registration order)."""
        if lib().p2_builder_register_public_input(self._h, t):
            raise P2Error(_err())

    def register_public_inputs(self, ts):
        for t in ts:
            self.register_public_input(t)

    def add_lookup_table_from_pairs(self, pairs):
        flat = (C.c_uint16 * (2 * len(pairs)))(*[v for p in pairs for v in p])
        i = lib().p2_builder_add_lookup_table_from_pairs(self._h, flat, len(pairs))
        if i == C.c_size_t(-1).value:
            raise P2Error(_err())
        return i

    def add_lookup_from_index(self, looking_in, lut_index):
        t = lib().p2_builder_add_lookup_from_index(self._h, looking_in, lut_index)
        if t == 0xFFFFFFFFFFFFFFFF:
            raise P2Error(_err())
        return t

    def num_gates(self): return lib().p2_builder_num_gates(self._h)

    # ---- CircuitBuilderAESState (aes-gcm/src/circuit_aes.rs:41-174) and the GCM helpers (circuit_gcm.rs)
    def sbox_lut(self): return lib().p2_aes_sbox_lut(self._h)
    def byte_xor_lut(self): return lib().p2_aes_byte_xor_lut(self._h)
    def gf_2_8_mul_lut(self): return lib().p2_aes_gf_2_8_mul_lut(self._h)
    def u8_unit_right_shift_lut(self): return lib().p2_gcm_u8_unit_right_shift_lut(self._h)
    def u8_bitref_lut(self): return lib().p2_gcm_u8_bitref_lut(self._h)
    def add_virtual_byte_target(self, u8_table_idx): return lib().p2_aes_add_virtual_byte_target(self._h, u8_table_idx)
    def add_virtual_byte_target_unsafe(self): return lib().p2_aes_add_virtual_byte_target_unsafe(self._h)
    def add_virtual_state_target_unsafe(self): return [self.add_virtual_byte_target_unsafe() for _ in range(16)]
    def add_virtual_state_target(self, lut): return [self.add_virtual_byte_target(lut) for _ in range(16)]

    def state_sub_bytes(self, sbox_lut, s):
        out = (u64 * 16)()
        lib().p2_aes_state_sub_bytes(self._h, sbox_lut, _arr(s), out)
        return list(out)

    def state_mix_columns(self, xor_lut, mul_lut, s):
        out = (u64 * 16)()
        lib().p2_aes_state_mix_columns(self._h, xor_lut, mul_lut, _arr(s), out)
        return list(out)

    def gf_2_8_mul(self, mul_lut, x, y): return lib().p2_aes_gf_2_8_mul(self._h, mul_lut, x, y)
    def gf_2_8_add(self, xor_lut, x, y): return lib().p2_aes_gf_2_8_add(self._h, xor_lut, x, y)

    def key_expansion(self, nk, nr, xor_lut, sbox_lut, key):
        out = (u64 * (16 * (nr + 1)))()
        lib().p2_aes_key_expansion(self._h, nk, nr, xor_lut, sbox_lut, _arr(key), out)
        return list(out)

    def encrypt_block(self, nr, xor_lut, mul_lut, sbox_lut, state, expanded_key):
        out = (u64 * 16)()
        lib().p2_aes_encrypt_block(self._h, nr, xor_lut, mul_lut, sbox_lut, _arr(state), _arr(expanded_key), out)
        return list(out)

    def gctr(self, nr, xor_lut, mul_lut, sbox_lut, expanded_key, icb, x):
        out = (u64 * len(x))()
        lib().p2_gcm_gctr(self._h, nr, xor_lut, mul_lut, sbox_lut, _arr(expanded_key), _arr(icb), _arr(x), len(x), out)
        return list(out)

    def right_shift_one(self, shift_lut, v):
        out = (u64 * 16)()
        lib().p2_gcm_right_shift_one(self._h, shift_lut, _arr(v), out)
        return list(out)

    def inc32(self, block):
        out = (u64 * 16)()
        lib().p2_gcm_inc32(self._h, _arr(block), out)
        return list(out)

    def gf_2_128_mul(self, xor_lut, shift_lut, bitref_lut, x, y):
        out = (u64 * 16)()
        lib().p2_gcm_gf_2_128_mul(self._h, xor_lut, shift_lut, bitref_lut, _arr(x), _arr(y), out)
        return list(out)

    def ghash(self, xor_lut, shift_lut, bitref_lut, h, x):
        out = (u64 * 16)()
        if lib().p2_gcm_ghash(self._h, xor_lut, shift_lut, bitref_lut, _arr(h), _arr(x), len(x), out):
            raise P2Error(_err())
        return list(out)

    def clmul_lo_lut(self): return lib().p2_gcm_clmul_lo_lut(self._h)
    def clmul_hi_lut(self): return lib().p2_gcm_clmul_hi_lut(self._h)

    def gf_2_128_mul_tables(self, xor_lut, lo_lut, hi_lut, x, y):
        """x * y in GF(2^128) from the clmul tables; x and y are 16 range-checked byte targets each."""
        if len(x) != 16 or len(y) != 16:
            raise P2Error("gf_2_128_mul_tables takes two blocks of 16 byte targets")
        out = (u64 * 16)()
        if lib().p2_gcm_gf_2_128_mul_tables(self._h, xor_lut, lo_lut, hi_lut, _arr(x), _arr(y), out):
            raise P2Error(_err())
        return list(out)

    def ghash_tables(self, xor_lut, lo_lut, hi_lut, h, x, lanes=1):
        """GHASH_h(x) from the clmul tables, `lanes` (1 to 16) blocks per reduction."""
        if len(h) != 16:
            raise P2Error("ghash_tables takes h as 16 byte targets")
        out = (u64 * 16)()
        if lib().p2_gcm_ghash_tables(self._h, xor_lut, lo_lut, hi_lut, _arr(h), _arr(x), len(x), out, lanes):
            raise P2Error(_err())
        return list(out)

    def hash_n_to_m_no_pad(self, inputs, num_outputs):
        out = (u64 * num_outputs)()
        if lib().p2_builder_hash_n_to_m_no_pad(self._h, _arr(inputs), len(inputs), out, num_outputs):
            raise P2Error(_err())
        return list(out)

    # ---- Merkle membership (plonky2 hash/merkle_proofs.rs, gadgets/hash.rs).  A hash is a list of four targets, a cap a list of
    # 2^cap_height hashes; include/p2aes.h has the rules.
    def permute_swapped(self, inputs, swap):
        """One PoseidonGate row: the permutation of `inputs` (12 targets) with its first two quarters exchanged where swap = 1."""
        if len(inputs) != 12:
            raise P2Error("permute_swapped takes 12 input targets")
        out = (u64 * 12)()
        if lib().p2_builder_permute_swapped(self._h, _arr(inputs), swap, out):
            raise P2Error(_err())
        return list(out)

    def hash_or_noop(self, targets):
        out = (u64 * 4)()
        if lib().p2_builder_hash_or_noop(self._h, _arr(targets) if targets else None, len(targets), out):
            raise P2Error(_err())
        return list(out)

    def add_virtual_hash(self):
        out = (u64 * 4)()
        if lib().p2_builder_add_virtual_hash(self._h, out):
            raise P2Error(_err())
        return list(out)

    def add_virtual_cap(self, cap_height):
        if not 0 <= cap_height <= 16:
            raise P2Error("add_virtual_cap: cap_height must be 0 to 16")
        out = (u64 * (4 << cap_height))()
        if lib().p2_builder_add_virtual_cap(self._h, cap_height, out):
            raise P2Error(_err())
        return [list(out[4 * i:4 * i + 4]) for i in range(1 << cap_height)]

    def connect_hashes(self, x, y):
        if len(x) != 4 or len(y) != 4 or lib().p2_builder_connect_hashes(self._h, _arr(x), _arr(y)):
            raise P2Error("connect_hashes takes two hashes of four targets" if len(x) != 4 or len(y) != 4 else _err())

    def verify_merkle_proof_to_cap(self, leaf_data, index_bits, cap, siblings):
        """leaf_data is the leaf at index sum index_bits[i] 2^i of the tree with this cap (a list of 2^h hashes); siblings: one
        hash per path level, the lowest first; len(index_bits) must be len(siblings) + h."""
        n_cap = len(cap)
        if n_cap == 0 or n_cap & (n_cap - 1) or n_cap > 1 << 16 or any(len(h) != 4 for h in list(cap) + list(siblings)):
            raise P2Error("verify_merkle_proof_to_cap: the cap is 2^h hashes (h <= 16) and every hash four targets")
        flat = lambda hs: _arr([t for h in hs for t in h]) if hs else None  # noqa: E731
        if lib().p2_builder_verify_merkle_proof_to_cap(self._h, _arr(leaf_data) if leaf_data else None, len(leaf_data), _arr(index_bits) if index_bits else None,
                                                       len(index_bits), flat(cap), n_cap.bit_length() - 1, flat(siblings), len(siblings)):
            raise P2Error(_err())

    def verify_merkle_proof(self, leaf_data, index_bits, root, siblings):
        self.verify_merkle_proof_to_cap(leaf_data, index_bits, [root], siblings)

    def merkle_update_to_cap(self, old_leaf, new_leaf, index_bits, old_cap, siblings):
        """The tree with cap old_cap holds old_leaf at the index; returns the cap (a list of 2^h hashes) of the same tree with
        new_leaf there.  siblings: one hash per path level as MerkleTree.update_batch(..., trace=True) records them."""
        n_cap = len(old_cap)
        if n_cap == 0 or n_cap & (n_cap - 1) or n_cap > 1 << 16 or any(len(h) != 4 for h in list(old_cap) + list(siblings)):
            raise P2Error("merkle_update_to_cap: the cap is 2^h hashes (h <= 16) and every hash four targets")
        if len(old_leaf) != len(new_leaf):
            raise P2Error("merkle_update_to_cap: the old leaf has %d targets, the new one %d" % (len(old_leaf), len(new_leaf)))
        flat = lambda hs: _arr([t for h in hs for t in h]) if hs else None  # noqa: E731
        out = (u64 * (4 * n_cap))()
        if lib().p2_builder_merkle_update_to_cap(self._h, _arr(old_leaf) if old_leaf else None, _arr(new_leaf) if new_leaf else None, len(old_leaf),
                                                 _arr(index_bits) if index_bits else None, len(index_bits), flat(old_cap), n_cap.bit_length() - 1, flat(siblings),
                                                 len(siblings), out):
            raise P2Error(_err())
        return [list(out[4 * i:4 * i + 4]) for i in range(n_cap)]

    def merkle_update(self, old_leaf, new_leaf, index_bits, old_root, siblings):
        return self.merkle_update_to_cap(old_leaf, new_leaf, index_bits, [old_root], siblings)[0]

    # ---- sparse keyed trees (MerkleMap; include/p2aes.h has the definition and the gadgets' costs).  key_bits: the D
    # little-endian bits of the key (split_le), the low len(siblings) walk the path, the rest choose the cap entry.
    @staticmethod
    def _map_args(who, key_bits, cap, siblings):
        n_cap = len(cap)
        if n_cap == 0 or n_cap & (n_cap - 1) or n_cap > 1 << 16 or any(len(h) != 4 for h in list(cap) + list(siblings)):
            raise P2Error("%s: the cap is 2^h hashes (h <= 16) and every hash four targets" % who)
        flat = lambda hs: _arr([t for h in hs for t in h]) if hs else None  # noqa: E731
        return (_arr(key_bits) if key_bits else None, len(key_bits)), flat(cap), n_cap.bit_length() - 1, (flat(siblings), len(siblings))

    def merkle_map_lookup_to_cap(self, key_bits, value, present, cap, siblings):
        """The map with this cap holds `value` at the key (present = 1) or nothing (present = 0; the value targets are then
        unconstrained).  `present` is made boolean here."""
        (kb, nb), capw, h, (sb, ns) = self._map_args("merkle_map_lookup_to_cap", key_bits, cap, siblings)
        if lib().p2_builder_merkle_map_lookup_to_cap(self._h, kb, nb, _arr(value) if value else None, len(value), present, capw, h, sb, ns):
            raise P2Error(_err())

    def merkle_map_lookup(self, key_bits, value, present, root, siblings):
        self.merkle_map_lookup_to_cap(key_bits, value, present, [root], siblings)

    def merkle_map_update_to_cap(self, key_bits, old_present, old_value, new_present, new_value, old_cap, siblings):
        """(old_present, old_value) at the key under old_cap; returns the cap with (new_present, new_value) there.  siblings: the
        proof of the key as the map stood before the change (MerkleMap.get)."""
        (kb, nb), capw, h, (sb, ns) = self._map_args("merkle_map_update_to_cap", key_bits, old_cap, siblings)
        if len(old_value) != len(new_value):
            raise P2Error("merkle_map_update_to_cap: the old value has %d targets, the new one %d" % (len(old_value), len(new_value)))
        out = (u64 * (4 * len(old_cap)))()
        if lib().p2_builder_merkle_map_update_to_cap(self._h, kb, nb, old_present, _arr(old_value) if old_value else None, new_present,
                                                     _arr(new_value) if new_value else None, len(old_value), capw, h, sb, ns, out):
            raise P2Error(_err())
        return [list(out[4 * i:4 * i + 4]) for i in range(len(old_cap))]

    def merkle_map_update(self, key_bits, old_present, old_value, new_present, new_value, old_root, siblings):
        return self.merkle_map_update_to_cap(key_bits, old_present, old_value, new_present, new_value, [old_root], siblings)[0]

    def _map_fixed(self, name, key_bits, value, old_cap, siblings):
        (kb, nb), capw, h, (sb, ns) = self._map_args(name, key_bits, old_cap, siblings)
        out = (u64 * (4 * len(old_cap)))()
        if getattr(lib(), "p2_builder_" + name)(self._h, kb, nb, _arr(value) if value else None, len(value), capw, h, sb, ns, out):
            raise P2Error(_err())
        return [list(out[4 * i:4 * i + 4]) for i in range(len(old_cap))]

    def merkle_map_insert_to_cap(self, key_bits, value, old_cap, siblings):
        """The key is absent under old_cap; returns the cap of the map with `value` at it."""
        return self._map_fixed("merkle_map_insert_to_cap", key_bits, value, old_cap, siblings)

    def merkle_map_insert(self, key_bits, value, old_root, siblings):
        return self.merkle_map_insert_to_cap(key_bits, value, [old_root], siblings)[0]

    def merkle_map_remove_to_cap(self, key_bits, value, old_cap, siblings):
        """The key holds `value` under old_cap; returns the cap of the map without it."""
        return self._map_fixed("merkle_map_remove_to_cap", key_bits, value, old_cap, siblings)

    def merkle_map_remove(self, key_bits, value, old_root, siblings):
        return self.merkle_map_remove_to_cap(key_bits, value, [old_root], siblings)[0]

    # ---- pod2 CircuitBuilderElliptic / CircuitBuilderBits and the ecgfp5 crate's builder traits.  A PointTarget is its ten
    # targets (x then u), a BigUInt320Target its 320 little-endian bit targets.
    def add_virtual_point_target(self):
        out = (u64 * 10)()
        lib().p2_builder_add_virtual_point_target(self._h, out)
        return list(out)

    def constant_point(self, point):
        out = (u64 * 10)()
        lib().p2_builder_constant_point(self._h, _pt(point), out)
        return list(out)

    def add_virtual_biguint320_target(self):
        out = (u64 * 320)()
        lib().p2_builder_add_virtual_biguint320_target(self._h, out)
        return list(out)

    def multiply_point(self, bits, point_target):
        out = (u64 * 10)()
        if lib().p2_builder_multiply_point(self._h, _arr(bits), _arr(point_target), out):
            raise P2Error(_err())
        return list(out)

    def ec_step(self, acc, q, bit, hinted=True):
        """One EcStepGate row: (mid, out) = (2 acc, 2 acc + bit q), acc / mid / out as X | Z | U | T (20 targets), q as x | u
        (10).  hinted=False leaves mid and out to the caller's witness."""
        if len(acc) != 20 or len(q) != 10:
            raise P2Error("ec_step takes 20 accumulator targets and 10 point targets")
        mid, out = (u64 * 20)(), (u64 * 20)()
        if lib().p2_builder_ec_step(self._h, _arr(acc), _arr(q), bit, 1 if hinted else 0, mid, out):
            raise P2Error(_err())
        return list(mid), list(out)

    def add_point(self, p, q):
        out = (u64 * 10)()
        lib().p2_builder_add_point(self._h, _arr(p), _arr(q), out)
        return list(out)

    def add_secret_key(self): return self.add_virtual_biguint320_target()   # ecgfp5/src/circuit.rs:31

    def public_key(self, sk_target):                                         # ecgfp5/src/circuit.rs:35
        out = (u64 * 10)()
        if lib().p2_builder_public_key(self._h, _arr(sk_target), out):
            raise P2Error(_err())
        return list(out)

    def elgamal_encrypt(self, pk, nonce, msg):                               # elgamal/circuit.rs:28
        c0, c1 = (u64 * 10)(), (u64 * 10)()
        if lib().p2_builder_elgamal_encrypt(self._h, _arr(pk), _arr(nonce), _arr(msg), c0, c1):
            raise P2Error(_err())
        return list(c0), list(c1)

    def hashed_elgamal_encrypt(self, pk, nonce, msg):                        # hashed_elgamal/circuit.rs:33
        c0, ct = (u64 * 10)(), (u64 * 5)()
        if lib().p2_builder_hashed_elgamal_encrypt(self._h, _arr(pk), _arr(nonce), _arr(msg), c0, ct):
            raise P2Error(_err())
        return list(c0), list(ct)

    # ---- verifiable decryption (not in the reference, whose circuits only encrypt).  The caller ties the key with
    # connect(public_key(sk_bits), pk) target by target.  Not checked in the circuit: c0 and c1 in the group, sk below the order.
    @staticmethod
    def _decrypt_args(sk_bits, c0, second, n_second):
        if len(sk_bits) != 320 or len(c0) != 10 or len(second) != n_second:
            raise P2Error("a decryption takes 320 key bits, a point of 10 targets and %d ciphertext targets" % n_second)

    def neg_point(self, p):
        if len(p) != 10:
            raise P2Error("neg_point takes a point of 10 targets")
        out = (u64 * 10)()
        if lib().p2_builder_neg_point(self._h, _arr(p), out):
            raise P2Error(_err())
        return list(out)

    def elgamal_decrypt(self, sk_bits, c0, c1):
        """msg = c1 - sk c0 (elgamal.rs:19) as ten targets"""
        self._decrypt_args(sk_bits, c0, c1, 10)
        out = (u64 * 10)()
        if lib().p2_builder_elgamal_decrypt(self._h, _arr(sk_bits), _arr(c0), _arr(c1), out):
            raise P2Error(_err())
        return list(out)

    def hashed_elgamal_decrypt(self, sk_bits, c0, ct):
        """msg[i] = ct[i] - hash_n_to_m_no_pad(as_fields(sk c0), 5)[i] (hashed_elgamal.rs:28) as five targets"""
        self._decrypt_args(sk_bits, c0, ct, 5)
        out = (u64 * 5)()
        if lib().p2_builder_hashed_elgamal_decrypt(self._h, _arr(sk_bits), _arr(c0), _arr(ct), out):
            raise P2Error(_err())
        return list(out)

    # ---- the Poseidon cipher on targets the caller supplies (csrc/poseidon_cipher.h): ks a point of 10 targets, nonce 2, a message
    # 5 L targets with L a multiple of 3, a ciphertext 5 (L + 1), the last five the tag.  The sealed-message statement is
    # ks = multiply_point(sk_bits, R); connect(public_key(sk_bits), pk); m = poseidon_decrypt(ks, nonce, ct).  Not checked in the
    # circuit: ks or R in the group, sk below the order.
    @staticmethod
    def _pcipher_args(ks, nonce, rows, extra):
        if len(ks) != 10 or len(nonce) != 2 or len(rows) % 5 or (len(rows) // 5 - extra) % 3 or len(rows) // 5 < extra:
            raise P2Error("the cipher takes a key of 10 targets, a nonce of 2 and 5 targets per element, L a multiple of 3")
        return len(rows) // 5 - extra

    def poseidon_encrypt(self, ks, nonce, m):
        """ct = encrypt(ks, m, nonce) (lib.rs:41): the loop of PoseidonEncryptTarget::build, as 5 (L + 1) targets"""
        L = self._pcipher_args(ks, nonce, m, 0)
        out = (u64 * (5 * (L + 1)))()
        if lib().p2_builder_poseidon_encrypt(self._h, _arr(ks), _arr(nonce), _arr(m) if L else (u64 * 1)(), L, out):
            raise P2Error(_err())
        return list(out)

    def poseidon_decrypt(self, ks, nonce, ct):
        """m = decrypt(ks, ct, nonce) (lib.rs:75) as 5 L targets; the tag is connected to the closing state, so a wrong one is an
        unsatisfiable witness"""
        L = self._pcipher_args(ks, nonce, ct, 1)
        out = (u64 * max(5 * L, 1))()
        if lib().p2_builder_poseidon_decrypt(self._h, _arr(ks), _arr(nonce), _arr(ct), L, out):
            raise P2Error(_err())
        return list(out)[:5 * L]

    # ---- Schnorr signatures on ecGFp5 (csrc/schnorr.h).  A signature target is (s_bits, e): 320 bit targets and a hash.
    def add_virtual_schnorr_signature_target(self):
        bits, e = (u64 * 320)(), (u64 * 4)()
        if lib().p2_builder_add_virtual_schnorr_signature(self._h, bits, e):
            raise P2Error(_err())
        return list(bits), list(e)

    def verify_schnorr_signature(self, pk, msg, sig):
        """Constrains hash(R' | pk | msg) = e for R' = s G + e (-pk) and returns R' (ten targets).  pk: any point target; msg: a
        list of targets; sig: what add_virtual_schnorr_signature_target gave.  Not checked in the circuit: s below the group
        order, pk in the group (see include/p2aes.h)."""
        bits, e = sig
        if len(pk) != 10 or len(bits) != 320 or len(e) != 4:
            raise P2Error("verify_schnorr_signature takes a point of 10 targets and a signature of 320 bits and 4 words")
        r = (u64 * 10)()
        if lib().p2_builder_verify_schnorr_signature(self._h, _arr(pk), _arr(msg) if msg else None, len(msg), _arr(bits), _arr(e), r):
            raise P2Error(_err())
        return list(r)

    def build(self):
        blob, n = u8p(), sz()
        if lib().p2_builder_build(self._h, C.byref(blob), C.byref(n)):
            raise P2Error(_err())
        # (ctypes.string_at takes a C int: blobs of 2^21-row circuits are larger than 2 GiB)
        data = bytes((C.c_char * n.value).from_address(C.cast(blob, C.c_void_p).value))
        lib().p2_blob_free(blob)
        return CircuitData(data)


class PartialWitness:
    """plonky2 iop::witness::PartialWitness: a target -> value map; set_target errors on a conflicting re-set."""

    def __init__(self):
        self.map = {}

    def set_target(self, target, value):
        value = int(value)
        if not 0 <= value < P:
            raise P2Error("value is not a canonical field element")
        old = self.map.get(target)
        if old is not None and old != value:
            raise P2Error("target was set twice with different values")
        self.map[target] = value

    def set_target_arr(self, targets, values):
        for t, v in zip(targets, values):
            self.set_target(t, v)

    # PartialWitnessByteArray / PartialWitnessAESState (circuit_aes.rs:277-297)
    def set_point_target(self, target, point):            # pod2 WitnessWriteCurve (elgamal/circuit.rs:88-92)
        self.set_target_arr(target, list(point[0]) + list(point[1]))

    def set_biguint320_target(self, target, value):       # pod2 bits (elgamal/circuit.rs:90)
        assert 0 <= value < 1 << 320
        self.set_target_arr(target, [(value >> i) & 1 for i in range(320)])

    def set_secret_key_target(self, target, sk):          # ecgfp5/src/circuit.rs:52
        self.set_biguint320_target(target, sk.value)

    def set_hash_target(self, target, words):
        self.set_target_arr(target, _hash4(words))

    def set_schnorr_signature_target(self, target, sig):
        """target = (s_bits, e) of add_virtual_schnorr_signature_target; sig = (s, e_words) as schnorr.sign returns it"""
        s, e = sig
        self.set_biguint320_target(target[0], s)
        self.set_hash_target(target[1], e)

    def set_cap_target(self, targets, cap):               # plonky2 WitnessHashes::set_cap_target
        if len(targets) != len(cap):
            raise P2Error("the cap has %d hashes, its target %d" % (len(cap), len(targets)))
        for t, h in zip(targets, cap):
            self.set_hash_target(t, h)

    def set_merkle_proof_target(self, targets, index, siblings):
        """targets = (index_bits, sibling hashes) as verify_merkle_proof_to_cap took them: the little-endian bits of `index`
        and one hash per level."""
        bits, sibs = targets
        if len(sibs) != len(siblings) or not 0 <= index < 1 << len(bits):
            raise P2Error("the path has %d siblings and the index %d bits" % (len(sibs), len(bits)))
        self.set_target_arr(bits, [(index >> i) & 1 for i in range(len(bits))])
        for t, h in zip(sibs, siblings):
            self.set_hash_target(t, h)

    def set_merkle_map_proof_target(self, targets, key, proof):
        """targets = (key_bits or None, present target or None, value targets, sibling hashes) as a merkle_map_* gadget took them;
        proof = (present, value, siblings) as MerkleMap.get(key) returns it.  None: the circuit derives the bits (split_le) or
        fixes the flag (insert, remove)."""
        bits, present_t, value_t, sibs = targets
        present, value, siblings = proof
        if len(sibs) != len(siblings) or len(value_t) != len(value) or (bits is not None and not 0 <= key < 1 << len(bits)):
            raise P2Error("the proof has %d siblings and %d value words, its targets %d and %d" % (len(siblings), len(value), len(sibs), len(value_t)))
        if bits is not None:
            self.set_target_arr(bits, [(key >> i) & 1 for i in range(len(bits))])
        if present_t is not None:
            self.set_target(present_t, int(present))
        self.set_target_arr(value_t, value)
        for t, h in zip(sibs, siblings):
            self.set_hash_target(t, h)

    def set_byte_target(self, target, value): self.set_target(target, value & 0xFF if isinstance(value, int) else int(value))
    def set_state_target(self, targets, state16):
        for t, v in zip(targets, state16):
            self.set_byte_target(t, v)


class CircuitData:
    """builder.build::<PoseidonGoldilocksConfig>() result.  prove() runs on the GPU (no CPU fallback)."""

    def __init__(self, blob, device=0):
        self.blob = blob
        self.device = device
        self._gpu = None
        self._vd = None
        info = _Info()
        if lib().p2_blob_info(blob, len(blob), C.byref(info)):
            raise P2Error(_err())
        self.info = {n: getattr(info, n) for n, _ in _Info._fields_}
        self.info["hasher"] = {v: k for k, v in HASHERS.items()}[info.hasher]

    def __del__(self):
        if getattr(self, "_gpu", None):
            lib().p2_circuit_free(self._gpu)
            self._gpu = None

    def gpu(self):
        if self._gpu is None:
            h = lib().p2_circuit_load(self.blob, len(self.blob), self.device)
            if not h:
                raise P2Error("p2_circuit_load failed: " + _err())
            self._gpu = h
        return self._gpu

    @property
    def proof_bytes(self): return self.info["proof_bytes"]

    @property
    def num_public_inputs(self): return self.info["num_public_inputs"]

    def public_inputs(self, proof):
        """ProofWithPublicInputs::public_inputs: the values of the proof's public-input trailer, u64 k || k values (parsing
        only; verify() checks that they are the ones the proof is about).  Reads the trailer alone: O(k) per proof."""
        k, pb = self.num_public_inputs, self.proof_bytes
        if len(proof) != pb:
            raise P2Error("proof length differs from the circuit's proof size")
        if k == 0:
            return []
        words = struct.unpack_from("<%dQ" % (k + 1), proof, pb - 8 * (k + 1))
        if words[0] != k:
            raise P2Error("wrong number of public inputs")
        return list(words[1:])

    def witness_schedule(self, fuse=8):
        """Host-side check of the device's witness schedule for macro size `fuse` (csrc/witness_schedule.h):
        {levels, chains, max_chain, fused_ops}; raises if an operand would not be ready when its op runs."""
        out = (C.c_uint32 * 4)()
        if lib().p2_witness_schedule_check(self.blob, len(self.blob), fuse, out):
            raise P2Error(_err())
        return dict(zip(("levels", "chains", "max_chain", "fused_ops"), out))

    def verifier_data(self):
        """constants_sigmas_cap || circuit_digest.  Computed on the device when the circuit is loaded (the reference's
        build() computes it); cached here, so verify() of later proofs needs no device."""
        if self._vd is None:
            out = (u64 * 80)()
            n = sz()
            if lib().p2_circuit_verifier_data(self.gpu(), out, 80, C.byref(n)):
                raise P2Error(_err())
            self._vd = list(out[: n.value])
        return list(self._vd)

    def set_option(self, name, value):
        """Tuning knobs of the GPU handle: "chunk", "streams", "debug_timing", "verify_chunk", "witness_chunk" (include/p2aes.h)."""
        if lib().p2_circuit_set_option(self.gpu(), name.encode(), int(value)):
            raise P2Error(_err())

    @staticmethod
    def _assignments(pws):
        B = len(pws)
        asg = (_Assignment * max(B, 1))()
        keep = []
        for i, pw in enumerate(pws):
            m = pw.map if hasattr(pw, "map") else pw
            ts, vs = _arr(list(m.keys())), _arr(list(m.values()))
            keep.append((ts, vs))
            asg[i].targets, asg[i].values, asg[i].count = C.cast(ts, u64p), C.cast(vs, u64p), len(m)
        return asg, keep

    def prove_batch(self, pws, outputs=None):
        """Returns (proofs: list[bytes|None], status: list[int]); with `outputs` (a list of targets to read back from the
        witness run each proof is made from: p2_prove_batch_outputs) also their values, one list per witness, VALUE_UNSET
        where the run did not determine one."""
        B = len(pws)
        asg, keep = self._assignments(pws)
        buf = C.create_string_buffer(max(B * self.proof_bytes, 1))
        status = (C.c_int * max(B, 1))()
        if outputs is None:
            if lib().p2_prove_batch(self.gpu(), B, asg, buf, status):
                raise P2Error("p2_prove_batch failed: " + _err())
        else:
            outs = list(outputs)
            vals = (u64 * max(B * len(outs), 1))()
            if lib().p2_prove_batch_outputs(self.gpu(), B, asg, _arr(outs) if outs else None, len(outs), vals, buf, status):
                raise P2Error("p2_prove_batch_outputs failed: " + _err())
        pb, base = self.proof_bytes, C.addressof(buf)   # (buf.raw would copy the whole buffer once per proof)
        res = [C.string_at(base + i * pb, pb) if status[i] == 0 else None for i in range(B)], list(status[:B])
        if outputs is None:
            return res
        return res + ([list(vals[i * len(outs):(i + 1) * len(outs)]) for i in range(B)],)

    def generate_witness(self, pws, outputs):
        """Witness generation only (p2_witness_batch; upstream: generate_partial_witness, then get_target): set the inputs,
        name the targets to read.  Returns (values: one list per witness, VALUE_UNSET where the run did not determine a target;
        statuses: 0, 1 or 2 as prove_batch reports them).  No proof is made."""
        B, outs = len(pws), list(outputs)
        asg, keep = self._assignments(pws)
        vals = (u64 * max(B * len(outs), 1))()
        status = (C.c_int * max(B, 1))()
        if lib().p2_witness_batch(self.gpu(), B, asg, _arr(outs) if outs else None, len(outs), vals, status):
            raise P2Error("p2_witness_batch failed: " + _err())
        return [list(vals[i * len(outs):(i + 1) * len(outs)]) for i in range(B)], list(status[:B])

    def explain(self, pw):
        """Why a witness fails (p2_witness_explain): a WitnessFault; kind "NONE" for a witness that generates."""
        a, keep = _assignment(pw)
        st, f = C.c_int(), _Fault()
        if lib().p2_witness_explain(self.gpu(), C.byref(a), C.byref(st), C.byref(f)):
            raise P2Error("p2_witness_explain failed: " + _err())
        return WitnessFault(f, st.value)

    def witness_batch_device(self, targets, d_values, outputs, d_out, d_status, batch, stream=None):
        """Device-resident witness generation: `d_values` [batch][len(targets)] u64 in, `d_out` [batch][len(outputs)] u64 and
        `d_status` int32[batch] out (raw device pointers); runs on `stream` (a raw hipStream_t or None), asynchronously."""
        outs = list(outputs)
        if lib().p2_witness_batch_device(self.gpu(), batch, _arr(list(targets)), len(targets), d_values, _arr(outs) if outs else None, len(outs), d_out, d_status,
                                         stream):
            raise P2Error("p2_witness_batch_device failed: " + _err())

    def prove_batch_outputs_device(self, targets, d_values, outputs, d_out, d_proofs, d_status, batch, stream=None):
        """prove_batch_device that also leaves the values of `outputs` in `d_out` [batch][len(outputs)]."""
        outs = list(outputs)
        if lib().p2_prove_batch_outputs_device(self.gpu(), batch, _arr(list(targets)), len(targets), d_values, _arr(outs) if outs else None, len(outs), d_out,
                                               d_proofs, d_status, stream):
            raise P2Error("p2_prove_batch_outputs_device failed: " + _err())

    @staticmethod
    def prove_batch_multi(datas, pws):
        """One batch sharded over several CircuitData loads of the same blob (one per HIP device): p2_prove_batch_multi."""
        B = len(pws)
        asg = (_Assignment * B)()
        keep = []
        for i, pw in enumerate(pws):
            ts, vs = _arr(list(pw.map.keys())), _arr(list(pw.map.values()))
            keep.append((ts, vs))
            asg[i].targets, asg[i].values, asg[i].count = ts, vs, len(pw.map)
        pb = datas[0].proof_bytes
        buf = C.create_string_buffer(B * pb)
        status = (C.c_int * B)()
        hs = (C.c_void_p * len(datas))(*[d.gpu() for d in datas])
        if lib().p2_prove_batch_multi(hs, len(datas), B, asg, buf, status):
            raise P2Error("p2_prove_batch_multi failed: " + _err())
        base = C.addressof(buf)
        return [C.string_at(base + i * pb, pb) if status[i] == 0 else None for i in range(B)], list(status)

    def prove_batch_device(self, targets, d_values, d_proofs, d_status, batch, stream=None):
        """Device-resident path: `d_values` [batch][len(targets)] u64, `d_proofs` batch*proof_bytes bytes and `d_status`
        int32[batch] are raw device pointers (e.g. torch tensors' data_ptr()); `stream` a raw hipStream_t or None."""
        tarr = _arr(list(targets))
        if lib().p2_prove_batch_device(self.gpu(), batch, tarr, len(targets), d_values, d_proofs, d_status, stream):
            raise P2Error("p2_prove_batch_device failed: " + _err())

    def set_zk_seed(self, seed):
        """TEST ONLY (reproducible zk proofs): blinding key = (seed, 0, 0, 0).  The default key comes from the OS CSPRNG."""
        if lib().p2_circuit_set_zk_seed(self.gpu(), seed):
            raise P2Error(_err())

    def set_zk_key(self, key4):
        """TEST ONLY: fix the full 256-bit blinding key (four field elements) and reset the proof counter."""
        if lib().p2_circuit_set_zk_key(self.gpu(), (C.c_uint64 * 4)(*key4)):
            raise P2Error(_err())

    def synchronize(self):
        if lib().p2_circuit_synchronize(self.gpu()):
            raise P2Error(_err())

    def prove(self, pw):
        proofs, status = self.prove_batch([pw])
        if status[0]:
            raise ProveError(status[0])
        return proofs[0]

    def verify(self, proof, verifier_data=None):
        vd = verifier_data if verifier_data is not None else self.verifier_data()
        if lib().p2_verify(self.blob, len(self.blob), _arr(vd), len(vd), proof, len(proof)):
            raise P2Error("verify failed: " + _err())

    def _vd_arg(self, verifier_data):
        if verifier_data is None:
            return None, 0
        return _arr(verifier_data), len(verifier_data)

    def verify_batch(self, proofs, verifier_data=None):
        """GPU verification of a batch (p2_verify_batch): one VERIFY_* code per proof, the reason class data.verify(proof)
        would report first.  `proofs`: a sequence of proof_bytes-long byte strings (None = a failed slot), or their
        concatenation."""
        pb = self.proof_bytes
        if isinstance(proofs, (bytes, bytearray)):
            if len(proofs) % pb:
                raise P2Error("verify_batch: %d bytes is not a whole number of %d-byte proofs" % (len(proofs), pb))
            blob = bytes(proofs)
        else:
            parts = [bytes(pb) if p is None else bytes(p) for p in proofs]
            if any(len(p) != pb for p in parts):
                raise P2Error("verify_batch: every proof must be %d bytes" % pb)
            blob = b"".join(parts)
        B = len(blob) // pb
        status = (C.c_int * max(B, 1))()
        vd, n = self._vd_arg(verifier_data)
        if lib().p2_verify_batch(self.gpu(), B, blob, vd, n, status):
            raise P2Error("p2_verify_batch failed: " + _err())
        return list(status[:B])

    def verify_batch_device(self, d_proofs, d_status, batch, verifier_data=None, stream=None):
        """Device-resident form: `d_proofs` (batch * proof_bytes bytes) and `d_status` (int32[batch]) are raw device pointers,
        `stream` a raw hipStream_t or None; asynchronous like prove_batch_device."""
        vd, n = self._vd_arg(verifier_data)
        if lib().p2_verify_batch_device(self.gpu(), batch, d_proofs, vd, n, d_status, stream):
            raise P2Error("p2_verify_batch_device failed: " + _err())

    # ---- compressed proofs: upstream's ProofWithPublicInputs::compress,
    # CompressedProofWithPublicInputs::decompress and CircuitData::verify_compressed on the host, batches on the GPU
    def _convert(self, fn, name, proof, verifier_data):
        vd = verifier_data if verifier_data is not None else self.verifier_data()
        proof = bytes(proof)
        out = C.create_string_buffer(max(self.proof_bytes, 1))
        n = sz()
        if fn(self.blob, len(self.blob), _arr(vd), len(vd), proof, len(proof), out, self.proof_bytes, C.byref(n)):
            raise P2Error(name + " failed: " + _err())
        return out.raw[: n.value]

    def compress(self, proof, verifier_data=None):
        """ProofWithPublicInputs::compress (host): the compressed bytes of a full proof of this circuit."""
        return self._convert(lib().p2_proof_compress, "compress", proof, verifier_data)

    def decompress(self, cproof, verifier_data=None):
        """CompressedProofWithPublicInputs::decompress (host): the full proof back."""
        return self._convert(lib().p2_proof_decompress, "decompress", cproof, verifier_data)

    def verify_compressed(self, cproof, verifier_data=None):
        """CircuitData::verify_compressed (host): verify() of the decompressed proof, behind the checks of decompression."""
        vd = verifier_data if verifier_data is not None else self.verifier_data()
        cproof = bytes(cproof)
        if lib().p2_verify_compressed(self.blob, len(self.blob), _arr(vd), len(vd), cproof, len(cproof)):
            raise P2Error("verify_compressed failed: " + _err())

    def _slots(self, items, name):
        """A batch of at most proof_bytes-long byte strings (None = an empty slot) as one fixed-stride buffer and lengths."""
        pb = self.proof_bytes
        parts = [b"" if p is None else bytes(p) for p in items]
        if any(len(p) > pb for p in parts):
            raise P2Error("%s: a proof is longer than %d bytes" % (name, pb))
        B = len(parts)
        buf = C.create_string_buffer(max(B * pb, 1))
        base = C.addressof(buf)
        for i, p in enumerate(parts):
            C.memmove(base + i * pb, p, len(p))
        return B, buf, (C.c_uint32 * max(B, 1))(*[len(p) for p in parts])

    def compress_batch(self, proofs, verifier_data=None):
        """GPU compression (p2_compress_batch): (list of compressed proofs, list of VERIFY_* codes); a failed slot is None."""
        B, buf, _ = self._slots(proofs, "compress_batch")
        pb = self.proof_bytes
        out = C.create_string_buffer(max(B * pb, 1))
        lengths = (C.c_uint32 * max(B, 1))()
        status = (C.c_int * max(B, 1))()
        vd, n = self._vd_arg(verifier_data)
        if lib().p2_compress_batch(self.gpu(), B, buf, vd, n, out, lengths, status):
            raise P2Error("p2_compress_batch failed: " + _err())
        base = C.addressof(out)
        return [C.string_at(base + i * pb, lengths[i]) if status[i] == 0 else None for i in range(B)], list(status[:B])

    def decompress_batch(self, cproofs, verifier_data=None):
        """GPU decompression (p2_decompress_batch): (list of full proofs, list of VERIFY_* codes); a failed slot is None."""
        B, buf, lengths = self._slots(cproofs, "decompress_batch")
        pb = self.proof_bytes
        out = C.create_string_buffer(max(B * pb, 1))
        status = (C.c_int * max(B, 1))()
        vd, n = self._vd_arg(verifier_data)
        if lib().p2_decompress_batch(self.gpu(), B, buf, lengths, vd, n, out, status):
            raise P2Error("p2_decompress_batch failed: " + _err())
        base = C.addressof(out)
        return [C.string_at(base + i * pb, pb) if status[i] == 0 else None for i in range(B)], list(status[:B])

    def verify_compressed_batch(self, cproofs, verifier_data=None, lengths=None):
        """GPU verification of compressed proofs (p2_verify_compressed_batch): one VERIFY_* code per proof, the reason class
        verify_compressed(cproof) would report.  `lengths` overrides the byte strings' own lengths (tests)."""
        B, buf, own = self._slots(cproofs, "verify_compressed_batch")
        if lengths is not None:
            own = (C.c_uint32 * max(B, 1))(*lengths)
        status = (C.c_int * max(B, 1))()
        vd, n = self._vd_arg(verifier_data)
        if lib().p2_verify_compressed_batch(self.gpu(), B, buf, own, vd, n, status):
            raise P2Error("p2_verify_compressed_batch failed: " + _err())
        return list(status[:B])

    def compress_batch_device(self, d_proofs, d_out, d_lengths, d_status, batch, verifier_data=None, stream=None):
        """Device-resident form: full proofs in, compressed proofs at a stride of proof_bytes, uint32 lengths and int32 statuses
        out (raw device pointers, e.g. torch tensors' data_ptr()); asynchronous on `stream` like verify_batch_device."""
        vd, n = self._vd_arg(verifier_data)
        if lib().p2_compress_batch_device(self.gpu(), batch, d_proofs, vd, n, d_out, d_lengths, d_status, stream):
            raise P2Error("p2_compress_batch_device failed: " + _err())

    def decompress_batch_device(self, d_cproofs, d_lengths, d_out, d_status, batch, verifier_data=None, stream=None):
        vd, n = self._vd_arg(verifier_data)
        if lib().p2_decompress_batch_device(self.gpu(), batch, d_cproofs, d_lengths, vd, n, d_out, d_status, stream):
            raise P2Error("p2_decompress_batch_device failed: " + _err())

    def verify_compressed_batch_device(self, d_cproofs, d_lengths, d_status, batch, verifier_data=None, stream=None):
        vd, n = self._vd_arg(verifier_data)
        if lib().p2_verify_compressed_batch_device(self.gpu(), batch, d_cproofs, d_lengths, vd, n, d_status, stream):
            raise P2Error("p2_verify_compressed_batch_device failed: " + _err())

    def debug_read(self, name, index=0, cap=1 << 26):
        out = (u64 * cap)()
        n = sz()
        if lib().p2_circuit_debug_read(self.gpu(), name.encode(), index, out, cap, C.byref(n)):
            raise P2Error(_err())
        return list(out[: n.value])

    def debug_read_bytes(self, name, index=0, cap=1 << 26):
        """The same buffer as little-endian u64 bytes (10^8-word buffers of the 2^19-row circuits: hash, do not list)."""
        out = (u64 * cap)()
        n = sz()
        if lib().p2_circuit_debug_read(self.gpu(), name.encode(), index, out, cap, C.byref(n)):
            raise P2Error(_err())
        return bytes(memoryview(out).cast("B")[: 8 * n.value])


class AesGcmTarget:
    """AesGcmTarget<NK, 4, NR, L, TAG> (aes-gcm/src/circuit_gcm.rs:24-209).  aad_len > 0 (not in the reference, whose a = []):
    that many byte targets `aad` of additional authenticated data, hashed in front of the ciphertext; it needs the tag."""

    @staticmethod
    def build(builder, nk=4, nr=10, L=16, tag=False, aad_len=0):
        t = AesGcmTarget()
        t.nk, t.nr, t.L, t.TAG, t.aad_len = nk, nr, L, tag, aad_len
        key, nonce, pt, ct, tg = (u64 * (4 * nk))(), (u64 * 12)(), (u64 * max(L, 1))(), (u64 * max(L, 1))(), (u64 * 16)()
        aad = (u64 * max(aad_len, 1))()
        if lib().p2_aes_gcm_build_aad(builder._h, nk, nr, L, int(tag), aad_len, key, nonce, pt, ct, tg, aad):
            raise P2Error(_err())
        t.key, t.nonce, t.pt, t.ct, t.tag, t.aad = list(key), list(nonce), list(pt)[:L], list(ct)[:L], list(tg), list(aad)[:aad_len]
        return t

    def set_targets(self, pw, key, nonce, pt, ct, tag, aad=b""):
        # effective contract of circuit_gcm.rs:183-193: len(pt) == len(ct) == L (copy_from_slice panics otherwise)
        assert len(pt) == self.L and len(ct) == self.L and len(key) == 4 * self.nk and len(nonce) == 12 and len(aad) == self.aad_len
        for t, v in zip(self.aad, aad): pw.set_byte_target(t, v)
        for t, v in zip(self.key, key): pw.set_byte_target(t, v)
        for t, v in zip(self.nonce, nonce): pw.set_byte_target(t, v)
        for t, v in zip(self.pt, pt): pw.set_byte_target(t, v)
        for t, v in zip(self.ct, ct): pw.set_byte_target(t, v)
        if self.TAG:
            assert len(tag) == 16
            for t, v in zip(self.tag, tag): pw.set_byte_target(t, v)
        else:
            for t in self.tag: pw.set_byte_target(t, 0)


class PoseidonEncryptTarget:
    """PoseidonEncryptTarget<L> (poseidon-cipher/src/circuit.rs:35-118).  Fq elements are 5-tuples of field elements;
    the key point `ks` is its two coordinates (x, u)."""

    @staticmethod
    def build(builder, L):
        t = PoseidonEncryptTarget()
        t.L = L
        ks, m, nonce, ct = (u64 * 10)(), (u64 * (5 * L))(), (u64 * 2)(), (u64 * (5 * (L + 1)))()
        if lib().p2_poseidon_cipher_build(builder._h, L, ks, m, nonce, ct):
            raise P2Error(_err())
        t.ks, t.m, t.nonce, t.ct = list(ks), list(m), list(nonce), list(ct)
        return t

    def set_targets(self, pw, ks, m, nonce, ct):
        assert len(m) == self.L and len(ct) == self.L + 1 and len(ks) == 2   # circuit.rs:99-100
        pw.set_target_arr(self.ks, [v for fq in ks for v in fq])
        pw.set_target_arr(self.m, [v for fq in m for v in fq])
        pw.set_target_arr(self.nonce, nonce)
        pw.set_target_arr(self.ct, [v for fq in ct for v in fq])


def _hash4(words):
    words = [int(w) for w in words]
    if len(words) != 4:
        raise P2Error("a hash is four field elements")
    return words


def _rows(rows, what):
    """[n][k] as (flat u64 array or None, n, k); every row of one length"""
    rows = [list(r) for r in rows]
    k = len(rows[0]) if rows else 0
    if any(len(r) != k for r in rows):
        raise P2Error("%s must all have one length" % what)
    flat = [int(v) for r in rows for v in r]
    if any(not 0 <= v < 1 << 64 for v in flat):
        raise P2Error("%s hold 64-bit words" % what)
    return (_arr(flat) if flat else None), len(rows), k


def _device_call(name, *args):
    """a _device form: every buffer a raw device pointer, asynchronous on the stream"""
    if getattr(lib(), name)(*args):
        raise P2Error("%s failed: %s" % (name, _err()))


def _batch_call(name, counts, mismatch, outs, device, host, call):
    """One per-item batch call.  counts: the lengths of the input lists, which agree or `mismatch` is raised; outs: one (ctype,
    elements per item) per output array.  -> (flat output arrays, statuses), all empty for an empty batch.  device=None: the host
    loop, host(i, outs, status) per item; otherwise call(fn, n, outs, status) makes the library call fn = `name`."""
    n = counts[0]
    if any(m != n for m in counts):
        raise P2Error(mismatch)
    if n == 0:
        return [[] for _ in outs], []
    outs, status = [(t * max(w * n, 1))() for t, w in outs], (C.c_int * n)()
    if device is None:
        for i in range(n):
            host(i, outs, status)
    elif call(getattr(lib(), name), n, outs, status):
        raise P2Error("%s failed: %s" % (name, _err()))
    return outs, list(status)


class MerkleTree:
    """plonky2 MerkleTree::new(leaves, cap_height) with PoseidonHash.  leaves: a list of equally long lists of canonical field
    elements, a power of two of them.  device = an index: the tree is built and kept on that GPU (p2_merkle_tree_*; .cap,
    .prove, .prove_batch and the device forms); device = None: the host twin (p2_native_merkle_*), which keeps the leaves and
    rebuilds the tree on every call -- for hosts without a device.  Only caps and paths are interface."""

    def __init__(self, leaves, cap_height=0, device=0):
        self._h = None
        self.device, self.cap_height = device, cap_height
        flat, self.num_leaves, self.leaf_len = _rows(leaves, "leaves")
        if self.num_leaves == 0 or self.num_leaves & (self.num_leaves - 1):
            raise P2Error("num_leaves must be a power of two, at least 1")
        self.depth = self.num_leaves.bit_length() - 1 - cap_height
        if device is None:
            self._leaves = flat
            self.cap     # validates the shape and the words
        else:
            h = C.c_void_p()
            if lib().p2_merkle_tree_new(flat, self.num_leaves, self.leaf_len, cap_height, device, C.byref(h)):
                raise P2Error("p2_merkle_tree_new failed: " + _err())
            self._h = h

    @classmethod
    def from_device(cls, d_leaves, num_leaves, leaf_len, cap_height=0, device=0, stream=None):
        """p2_merkle_tree_new_device: `d_leaves` a raw device pointer to [num_leaves][leaf_len] u64 (e.g. a torch tensor's
        data_ptr()), read by kernels enqueued on `stream`; keep the buffer untouched until they have run."""
        t = cls.__new__(cls)
        t._h = None
        t.device, t.cap_height, t.num_leaves, t.leaf_len = device, cap_height, num_leaves, leaf_len
        h = C.c_void_p()
        if lib().p2_merkle_tree_new_device(d_leaves, num_leaves, leaf_len, cap_height, device, stream, C.byref(h)):
            raise P2Error("p2_merkle_tree_new_device failed: " + _err())
        t._h = h
        t.depth = num_leaves.bit_length() - 1 - cap_height
        return t

    def __del__(self):
        if getattr(self, "_h", None):
            lib().p2_merkle_tree_free(self._h)
            self._h = None

    @property
    def cap(self):
        """2^cap_height hashes, each a list of four field elements"""
        n = 4 << max(self.cap_height, 0)
        out = (u64 * n)()
        if self._h is None:
            if lib().p2_native_merkle_cap(self._leaves, self.num_leaves, self.leaf_len, self.cap_height, out):
                raise P2Error("p2_native_merkle_cap failed: " + _err())
        elif lib().p2_merkle_tree_cap(self._h, out, n):
            raise P2Error("p2_merkle_tree_cap failed: " + _err())
        return [list(out[4 * i:4 * i + 4]) for i in range(n // 4)]

    def prove_batch(self, indices):
        """tree.prove(i) for every index: one list of sibling hashes (lowest level first) per index"""
        idx = [int(i) for i in indices]
        d = self.depth
        if self._h is None:
            out = []
            buf = (u64 * max(4 * d, 1))()
            for i in idx:
                if not 0 <= i < 1 << 64 or lib().p2_native_merkle_prove(self._leaves, self.num_leaves, self.leaf_len, self.cap_height, i, buf):
                    raise P2Error("p2_native_merkle_prove failed: " + (_err() if 0 <= i < 1 << 64 else "index out of range"))
                out.append([list(buf[4 * l:4 * l + 4]) for l in range(d)])
            return out
        if any(not 0 <= i < 1 << 64 for i in idx):
            raise P2Error("index out of range")
        buf = (u64 * max(len(idx) * 4 * d, 1))()
        if lib().p2_merkle_tree_prove_batch(self._h, _arr(idx) if idx else None, len(idx), buf):
            raise P2Error("p2_merkle_tree_prove_batch failed: " + _err())
        return [[list(buf[(k * d + l) * 4:(k * d + l) * 4 + 4]) for l in range(d)] for k in range(len(idx))]

    def prove(self, index):
        return self.prove_batch([index])[0]

    def update_batch(self, indices, leaves, trace=False):
        """The writes leaf indices[j] <- leaves[j] in order: item j acts on the tree left by the items before it, duplicates are
        legal and the last write wins.  All or nothing: an index that names no leaf or a word not below p raises and changes
        nothing.  trace=True returns a MerkleUpdateTrace (the siblings each item saw, the cap entry it left), else None."""
        idx = [int(i) for i in indices]
        flat, k, leaf_len = _rows(leaves, "leaves")
        if k != len(idx) or any(not 0 <= i < 1 << 64 for i in idx):
            raise P2Error("update_batch: one leaf per index, indices of 64 bits")
        if k == 0:
            return MerkleUpdateTrace(self, [], [], []) if trace else None
        if leaf_len != self.leaf_len:
            raise P2Error("update_batch: the tree's leaves have %d words, these %d" % (self.leaf_len, leaf_len))
        d = self.depth
        sib, roots = ((u64 * max(k * 4 * d, 1))(), (u64 * (4 * k))()) if trace else (None, None)
        if self._h is None:
            if lib().p2_native_merkle_update(self._leaves, self.num_leaves, self.leaf_len, self.cap_height, _arr(idx), flat, k, sib, roots):
                raise P2Error("p2_native_merkle_update failed: " + _err())
        elif lib().p2_merkle_tree_update(self._h, _arr(idx), flat, k, sib, roots):
            raise P2Error("p2_merkle_tree_update failed: " + _err())
        if not trace:
            return None
        return MerkleUpdateTrace(self, idx, [[list(sib[(j * d + l) * 4:(j * d + l) * 4 + 4]) for l in range(d)] for j in range(k)],
                                 [list(roots[4 * j:4 * j + 4]) for j in range(k)])

    def update(self, index, leaf, trace=False):
        return self.update_batch([index], [leaf], trace)

    def update_batch_device(self, d_indices, d_leaves, k, d_siblings, sib_stride_words, d_root_after, root_stride_words, d_status, stream=None):
        """Device-resident updates (p2_merkle_tree_update_device): `d_indices` u64[k], `d_leaves` u64[k][leaf_len], `d_status` int32[k]
        and, for a trace, `d_siblings` (item j at d_siblings + 8 * j * sib_stride_words bytes) and `d_root_after` are raw device
        pointers; d_siblings = None: no trace.  Asynchronous on `stream`."""
        if self._h is None:
            raise P2Error("a host tree has no device forms")
        if lib().p2_merkle_tree_update_device(self._h, d_indices, d_leaves, k, d_siblings, sib_stride_words, d_root_after, root_stride_words, d_status, stream):
            raise P2Error("p2_merkle_tree_update_device failed: " + _err())

    @property
    def last_update_hashes(self):
        """two_to_one calls of the last update on the device (0 before the first; a host tree does not count)"""
        if self._h is None:
            raise P2Error("a host tree does not count its hashes")
        out = u64()
        if lib().p2_merkle_tree_last_update_hashes(self._h, C.byref(out)):
            raise P2Error("p2_merkle_tree_last_update_hashes failed: " + _err())
        return out.value

    def prove_batch_device(self, d_indices, n, d_out, out_stride_words, d_status, stream=None):
        """Device-resident openings: `d_indices` u64[n], `d_out` (path i at d_out + 8 * i * out_stride_words bytes: 4 * depth words) and
        `d_status` int32[n] are raw device pointers; asynchronous on `stream` like prove_batch_device of a circuit."""
        if self._h is None:
            raise P2Error("a host tree has no device forms")
        if lib().p2_merkle_tree_prove_batch_device(self._h, d_indices, n, d_out, out_stride_words, d_status, stream):
            raise P2Error("p2_merkle_tree_prove_batch_device failed: " + _err())


class MerkleUpdateTrace:
    """What MerkleTree.update_batch(indices, leaves, trace=True) recorded: siblings[j] the path of indices[j] (one hash per level,
    the lowest first) in the tree BEFORE item j, roots_after[j] cap entry indices[j] >> depth right AFTER it."""

    def __init__(self, tree, indices, siblings, roots_after):
        self.indices, self.siblings, self.roots_after, self._depth = indices, siblings, roots_after, tree.depth

    def caps(self, initial_cap):
        """the k + 1 caps: initial_cap, then the cap after every item"""
        out = [[list(h) for h in initial_cap]]
        for i, root in zip(self.indices, self.roots_after):
            cap = [list(h) for h in out[-1]]
            cap[i >> self._depth] = list(root)
            out.append(cap)
        return out


class merkle:
    """verify_merkle_proof_to_cap outside a circuit: statuses 0 accepted, 1 rejected, 2 a word that is not below p."""

    @staticmethod
    def verify_batch(leaves, indices, siblings, cap, device=0):
        """leaves [n][leaf_len], indices [n], siblings [n][depth] hashes, cap 2^h hashes -> n statuses.  device = an index: on
        that GPU (p2_merkle_verify_batch); None: a host loop over p2_native_merkle_verify."""
        lf, n, leaf_len = _rows(leaves, "leaves")
        idx = [int(i) for i in indices]
        sibs = [[w for h in path for w in _hash4(h)] for path in siblings]
        sb, n_s, sib_words = _rows(sibs, "paths")
        capw, n_cap, _ = _rows([_hash4(h) for h in cap], "cap hashes")
        if len(idx) != n or (n_s != n) or n_cap == 0 or n_cap & (n_cap - 1) or any(not 0 <= i < 1 << 64 for i in idx):
            raise P2Error("verify_batch: one index and one path per leaf, a cap of 2^h hashes")
        if n == 0:
            return []
        if leaf_len == 0:
            raise P2Error("verify_batch: empty leaves")
        depth, cap_height = sib_words // 4, n_cap.bit_length() - 1
        status = (C.c_int * n)()
        if device is None:
            st = C.c_int()
            for i in range(n):
                leaf = C.cast(C.byref(lf, 8 * i * leaf_len), u64p)
                path = C.cast(C.byref(sb, 8 * i * sib_words), u64p) if depth else None
                if lib().p2_native_merkle_verify(leaf, leaf_len, idx[i], path, depth, capw, cap_height, C.byref(st)):
                    raise P2Error("p2_native_merkle_verify failed: " + _err())
                status[i] = st.value
        elif lib().p2_merkle_verify_batch(lf, leaf_len, _arr(idx), sb, depth, capw, cap_height, n, status, device):
            raise P2Error("p2_merkle_verify_batch failed: " + _err())
        return list(status)

    @staticmethod
    def verify(leaf, index, siblings, cap, device=0):
        return merkle.verify_batch([leaf], [index], [siblings], cap, device)[0]

    @staticmethod
    def verify_batch_device(d_leaves, leaf_len, d_indices, d_siblings, depth, d_cap, cap_height, n, d_status, device=0, stream=None):
        """Every buffer a raw device pointer (p2_merkle_verify_batch_device); asynchronous on `stream`."""
        _device_call("p2_merkle_verify_batch_device", d_leaves, leaf_len, d_indices, d_siblings, depth, d_cap, cap_height, n, d_status, device, stream)


class MerkleMap:
    """A sparse keyed Merkle tree, MerkleMap(key_bits = D, value_len = V, cap_height = h): the complete tree of depth D with the
    entry of key k at leaf k, of which only the non-empty nodes exist (include/p2aes.h has the definition).  keys: distinct
    integers below 2^D and p; values: one list of V canonical words per key (V = 0: a set).  device = an index: built and kept
    on that GPU (p2_merkle_map_*); value_len: V of a map without entries; device = None: the host twin (p2_native_merkle_map_*), which keeps the entries and rebuilds
    what it needs on every call.  Immutable: a changed set is a new MerkleMap."""

    def __init__(self, keys, values, key_bits, cap_height=0, device=0, value_len=None):
        self._h = None
        keys = [int(k) for k in keys]
        if any(not 0 <= k < 1 << 64 for k in keys):
            raise P2Error("keys are 64-bit words")
        vals, n, self.value_len = _rows(values, "values")
        if n != len(keys):
            raise P2Error("MerkleMap: one value per key")
        if value_len is not None:                          # an empty map cannot tell from its values
            if n and value_len != self.value_len:
                raise P2Error("MerkleMap: the values have %d words, value_len says %d" % (self.value_len, value_len))
            self.value_len = value_len
        self.device, self.key_bits, self.cap_height, self._n = device, key_bits, cap_height, n
        self.depth = key_bits - cap_height
        self._keys, self._vals = (_arr(keys) if keys else None), vals
        if device is None:
            self.cap     # validates the shape and the entries
        else:
            h = C.c_void_p()
            if lib().p2_merkle_map_new(self._keys, vals, n, self.value_len, key_bits, cap_height, device, C.byref(h)):
                raise P2Error("p2_merkle_map_new failed: " + _err())
            self._h = h
            self._keys = self._vals = None

    @classmethod
    def from_device(cls, d_keys, d_values, n, value_len, key_bits, cap_height=0, device=0, stream=None):
        """p2_merkle_map_new_device: raw device pointers to u64[n] and u64[n][value_len], read by kernels on `stream`; the call
        synchronises that stream once and the buffers are free again when it returns."""
        m = cls.__new__(cls)
        m._h = None
        m.device, m.key_bits, m.cap_height, m.value_len, m._n, m.depth = device, key_bits, cap_height, value_len, n, key_bits - cap_height
        h = C.c_void_p()
        if lib().p2_merkle_map_new_device(d_keys, d_values, n, value_len, key_bits, cap_height, device, stream, C.byref(h)):
            raise P2Error("p2_merkle_map_new_device failed: " + _err())
        m._h = h
        return m

    def __del__(self):
        if getattr(self, "_h", None):
            lib().p2_merkle_map_free(self._h)
            self._h = None

    def __len__(self):
        if self._h is None:
            return self._n
        n = sz()
        if lib().p2_merkle_map_len(self._h, C.byref(n)):
            raise P2Error("p2_merkle_map_len failed: " + _err())
        return n.value

    @property
    def cap(self):
        """2^cap_height hashes, each a list of four field elements"""
        n = 4 << min(max(self.cap_height, 0), 16)
        out = (u64 * n)()
        if self._h is None:
            if lib().p2_native_merkle_map_cap(self._keys, self._vals, self._n, self.value_len, self.key_bits, self.cap_height, out):
                raise P2Error("p2_native_merkle_map_cap failed: " + _err())
        elif lib().p2_merkle_map_cap(self._h, out, n):
            raise P2Error("p2_merkle_map_cap failed: " + _err())
        return [list(out[4 * i:4 * i + 4]) for i in range(n // 4)]

    @property
    def hashes(self):
        """two_to_one calls of the build on the device: the non-empty nodes above the leaves (a host map does not count)"""
        if self._h is None:
            raise P2Error("a host map does not count its hashes")
        out = u64()
        if lib().p2_merkle_map_hashes(self._h, C.byref(out)):
            raise P2Error("p2_merkle_map_hashes failed: " + _err())
        return out.value

    def get_batch(self, keys):
        """-> one (present, value, siblings) per key: present 0 or 1, value V words (zeros when absent), siblings one hash per
        level, the lowest first"""
        keys = [int(k) for k in keys]
        if any(not 0 <= k < 1 << 64 for k in keys):
            raise P2Error("keys are 64-bit words")
        V, d = self.value_len, self.depth

        def host(i, outs, status):
            present = C.c_int()
            value, sib = C.cast(C.byref(outs[1], 8 * i * V), u64p), C.cast(C.byref(outs[2], 32 * i * d), u64p)
            if lib().p2_native_merkle_map_get(self._keys, self._vals, self._n, V, self.key_bits, self.cap_height, keys[i], C.byref(present), value, sib):
                raise P2Error("p2_native_merkle_map_get failed: " + _err())
            outs[0][i] = present.value

        ka = _arr(keys) if keys else None
        (present, value, sib), _ = _batch_call("p2_merkle_map_get_batch", [len(keys)], None, [(u64, 1), (u64, V), (u64, 4 * d)], self.device if self._h else None, host,
                                               lambda fn, n, outs, status: fn(self._h, ka, n, outs[0], outs[1], outs[2]))
        return [(int(present[i]), list(value[i * V:(i + 1) * V]), [list(sib[(i * d + l) * 4:(i * d + l) * 4 + 4]) for l in range(d)]) for i in range(len(keys))]

    def get(self, key):
        return self.get_batch([key])[0]

    def get_batch_device(self, d_keys, n, d_out, out_stride_words, present_off, value_off, siblings_off, d_status, stream=None):
        """Device-resident lookups (p2_merkle_map_get_batch_device): `d_keys` u64[n], `d_status` int32[n] and `d_out` are raw device
        pointers; row j is at d_out + 8 * j * out_stride_words bytes and takes presence, the value and the siblings at the given
        word offsets.  Asynchronous on `stream`."""
        if self._h is None:
            raise P2Error("a host map has no device forms")
        _device_call("p2_merkle_map_get_batch_device", self._h, d_keys, n, d_out, out_stride_words, present_off, value_off, siblings_off, d_status, stream)


class merkle_map:
    """MerkleMap proofs checked outside a circuit: statuses 0 the walk reaches its cap entry, 1 it does not, 2 malformed (a key
    out of range, a word not below p, present other than 0 or 1)."""

    @staticmethod
    def verify_batch(keys, key_bits, proofs, cap, device=0):
        """keys [n], proofs [n] of (present, value, siblings) as MerkleMap.get returns them, cap 2^h hashes -> n statuses.  device =
        an index: on that GPU (p2_merkle_map_verify_batch); None: a host loop over p2_native_merkle_map_verify."""
        keys = [int(k) for k in keys]
        proofs = list(proofs)
        flags = [int(p[0]) for p in proofs]
        vals, n_v, V = _rows([p[1] for p in proofs], "values")
        sb, n_s, sib_words = _rows([[w for h in p[2] for w in _hash4(h)] for p in proofs], "paths")
        capw, n_cap, _ = _rows([_hash4(h) for h in cap], "cap hashes")
        if n_cap == 0 or n_cap & (n_cap - 1) or any(not 0 <= v < 1 << 64 for v in keys + flags):
            raise P2Error("verify_batch: keys and flags of 64 bits, a cap of 2^h hashes")
        cap_height = n_cap.bit_length() - 1
        if proofs and sib_words != 4 * (key_bits - cap_height):
            raise P2Error("verify_batch: a proof has key_bits - cap_height siblings")
        st = C.c_int()

        def host(i, outs, status):
            value = C.cast(C.byref(vals, 8 * i * V), u64p) if V else None
            path = C.cast(C.byref(sb, 8 * i * sib_words), u64p) if sib_words else None
            if lib().p2_native_merkle_map_verify(keys[i], key_bits, flags[i], value, V, path, capw, cap_height, C.byref(st)):
                raise P2Error("p2_native_merkle_map_verify failed: " + _err())
            status[i] = st.value

        ka, fa = (_arr(keys), _arr(flags)) if keys else (None, None)
        _, status = _batch_call("p2_merkle_map_verify_batch", [len(keys), len(proofs)], "verify_batch: one proof per key", [], device, host,
                                lambda fn, n, outs, status: fn(ka, key_bits, fa, vals, V, sb, capw, cap_height, n, status, device))
        return status

    @staticmethod
    def verify(key, key_bits, proof, cap, device=0):
        return merkle_map.verify_batch([key], key_bits, [proof], cap, device)[0]

    @staticmethod
    def verify_batch_device(d_keys, key_bits, d_present, d_values, value_len, d_siblings, d_cap, cap_height, n, d_status, device=0, stream=None):
        """Every buffer a raw device pointer (p2_merkle_map_verify_batch_device); asynchronous on `stream`."""
        _device_call("p2_merkle_map_verify_batch_device", d_keys, key_bits, d_present, d_values, value_len, d_siblings, d_cap, cap_height, n, d_status, device, stream)


class keccak_native:
    """The tree hasher of hasher="keccak" on the host (csrc/keccak_hash.h): digests in the four-word form (bytes 0-6, 7-13,
    14-20, 21-24 of the 25-byte Keccak-256 prefix)."""

    @staticmethod
    def hash_no_pad(words):
        out = (u64 * 4)()
        lib().p2_native_keccak_hash_no_pad(_arr(words), len(words), out)
        return list(out)

    @staticmethod
    def two_to_one(l, r):
        out = (u64 * 4)()
        lib().p2_native_keccak_two_to_one(_arr(l), _arr(r), out)
        return list(out)

    @staticmethod
    def keccak256(data):
        out = C.create_string_buffer(32)
        lib().p2_native_keccak256(bytes(data), len(data), out)
        return out.raw


class poseidon_native:
    """poseidon-cipher/src/lib.rs through the C ABI."""

    @staticmethod
    def hash_n_to_m_no_pad(inputs, m):
        out = (u64 * m)()
        lib().p2_native_hash_n_to_m_no_pad(_arr(inputs), len(inputs), out, m)
        return list(out)

    @staticmethod
    def new_key(seed=None):                                # lib.rs:31 (OS randomness, as upstream's OsRng; seed = tests only)
        k = ecgfp5.random_scalar(seed)
        return k, ecgfp5.mul(k, ecgfp5.generator())

    @staticmethod
    def expanded_key(K, seed=None):                        # lib.rs:36
        return ecgfp5.mul(ecgfp5.random_scalar(seed), K)

    @staticmethod
    def encrypt(ks, msg, nonce):
        n = len(msg)
        nct = (n + 2) // 3 * 3 + 1
        ct = (u64 * (5 * nct))()
        lib().p2_native_poseidon_encrypt(_arr([v for fq in ks for v in fq]), _arr([v for fq in msg for v in fq]) if n else (u64 * 1)(), n, _arr(nonce), ct)
        return [tuple(ct[5 * i:5 * i + 5]) for i in range(nct)]

    @staticmethod
    def decrypt(ks, ct, nonce, l):
        msg = (u64 * (5 * max(l, 1)))()
        if lib().p2_native_poseidon_decrypt(_arr([v for fq in ks for v in fq]), _arr([v for fq in ct for v in fq]), len(ct), _arr(nonce), l, msg):
            raise P2Error(_err())
        return [tuple(msg[5 * i:5 * i + 5]) for i in range(l)]

    # ---- the cipher in GPU batches (csrc/kernels_pcipher.h).  Every list is per item; a key is the shared point ks = r K = k R
    # (new_key / expanded_key), used as its ten words; a nonce two words; a message l Fq elements of five words, l one value per
    # call and at most 3072; a ciphertext pad3(l) + 1 elements.  Statuses: 0 done, 1 (decrypt) the tag or the padding is wrong,
    # 2 a word not below p; a row whose status is not 0 holds zeros.  device=None: a host loop over encrypt / decrypt's entry
    # points with the same checks.
    DONE, REJECTED, MALFORMED = 0, 1, 2
    MAX_LEN = 3072

    @staticmethod
    def _batch_args(name, kss, nonces, rows, elems):
        """-> (ks, nonce, flat rows or a one-word dummy, the three list lengths); rows: per item `elems` Fq elements"""
        ks, n, k = _rows([list(p[0]) + list(p[1]) for p in kss], "keys")
        nn, n_n, k_n = _rows(nonces, "nonces")
        flat, n_r, k_r = _rows([[v for fq in row for v in fq] for row in rows], "messages and ciphertexts")
        if n == n_n == n_r != 0 and (k != 10 or k_n != 2 or k_r != 5 * elems):
            raise P2Error("%s: keys are points of ten words, nonces two words, rows %d elements of five words" % (name, elems))
        return ks, nn, flat if flat is not None else (u64 * 1)(), [n, n_n, n_r]

    @staticmethod
    def _pad3(l):
        return (l + 2) // 3 * 3

    @staticmethod
    def _elements(buf, n, elems):
        return [[tuple(buf[5 * (elems * i + j):5 * (elems * i + j) + 5]) for j in range(elems)] for i in range(n)]

    @staticmethod
    def _check_len(l):
        if not 0 <= l <= poseidon_native.MAX_LEN:
            raise P2Error("l is at most 3072 elements")

    @staticmethod
    def encrypt_batch(kss, nonces, msgs, device=0):
        """-> (cts, statuses): cts[i] = encrypt(kss[i], msgs[i], nonces[i]) (lib.rs:41), every message of one length"""
        msgs = [list(m) for m in msgs]
        l = len(msgs[0]) if msgs else 0
        ks, nn, m, counts = poseidon_native._batch_args("encrypt_batch", kss, nonces, msgs, l)
        nct = poseidon_native._pad3(l) + 1

        def host(i, outs, status):
            poseidon_native._check_len(l)
            if any(w >= P for w in ks[10 * i:10 * i + 10]) or any(w >= P for w in nn[2 * i:2 * i + 2]) or any(w >= P for w in m[5 * l * i:5 * l * (i + 1)]):
                status[i] = poseidon_native.MALFORMED
            else:
                lib().p2_native_poseidon_encrypt(_at(ks, 10 * i), _at(m, 5 * l * i), l, _at(nn, 2 * i), _at(outs[0], 5 * nct * i))
        (ct,), st = _batch_call("p2_poseidon_encrypt_batch", counts, "encrypt_batch: every list has one entry per item", [(u64, 5 * nct)], device, host,
                                lambda fn, n, outs, status: fn(ks, nn, m, l, n, outs[0], status, device))
        return poseidon_native._elements(ct, len(st), nct), st

    @staticmethod
    def decrypt_batch(kss, nonces, cts, l, device=0):
        """-> (msgs, statuses): msgs[i] = decrypt(kss[i], cts[i], nonces[i], l) (lib.rs:75); status 1 and l zero elements where the
        reference's asserts fail.  Its rule for the padding elements holds: they are looked at only when l > 3."""
        nct = poseidon_native._pad3(l) + 1
        ks, nn, ct, counts = poseidon_native._batch_args("decrypt_batch", kss, nonces, cts, nct)

        def host(i, outs, status):
            poseidon_native._check_len(l)
            one = (u64 * max(5 * l, 1))()
            if any(w >= P for w in ks[10 * i:10 * i + 10]) or any(w >= P for w in nn[2 * i:2 * i + 2]) or any(w >= P for w in ct[5 * nct * i:5 * nct * (i + 1)]):
                status[i] = poseidon_native.MALFORMED
            elif lib().p2_native_poseidon_decrypt(_at(ks, 10 * i), _at(ct, 5 * nct * i), nct, _at(nn, 2 * i), l, one):
                status[i] = poseidon_native.REJECTED
            else:
                outs[0][5 * l * i:5 * l * (i + 1)] = one[:5 * l]
        (msg,), st = _batch_call("p2_poseidon_decrypt_batch", counts, "decrypt_batch: every list has one entry per item", [(u64, 5 * l)], device, host,
                                 lambda fn, n, outs, status: fn(ks, nn, ct, l, n, outs[0], status, device))
        return poseidon_native._elements(msg, len(st), l), st

    @staticmethod
    def encrypt_batch_device(d_ks, d_nonce, d_msg, l, count, d_ct, d_status, device=0, stream=None):
        """Every buffer a raw device pointer (p2_poseidon_encrypt_batch_device); asynchronous on `stream`."""
        _device_call("p2_poseidon_encrypt_batch_device", d_ks, d_nonce, d_msg, l, count, d_ct, d_status, device, stream)

    @staticmethod
    def decrypt_batch_device(d_ks, d_nonce, d_ct, l, count, d_msg, d_status, device=0, stream=None):
        _device_call("p2_poseidon_decrypt_batch_device", d_ks, d_nonce, d_ct, l, count, d_msg, d_status, device, stream)

    @staticmethod
    def seal_batch(pks, rs, nonces, msgs, device=0):
        """A message of any length to the holder of a public key: R = r G, ks = r pk (two ecgfp5.mul_batch), ct = encrypt(ks, msg,
        nonce).  -> (Rs, cts, statuses); a mul_batch status other than 0 (a pk outside the group: 2) is the item's, its rows zeros."""
        msgs = [list(m) for m in msgs]
        n, l = len(msgs), len(msgs[0]) if msgs else 0
        Rs, st_r = ecgfp5.mul_batch(rs, [ecgfp5.generator()] * n, device)
        kss, st_k = ecgfp5.mul_batch(rs, pks, device)
        cts, st = poseidon_native.encrypt_batch(kss, nonces, msgs, device)
        zero_ct = [(0,) * 5] * (poseidon_native._pad3(l) + 1)
        for i in range(n):
            if st_r[i] or st_k[i]:
                st[i], cts[i], Rs[i] = st_r[i] or st_k[i], list(zero_ct), ((0,) * 5, (0,) * 5)
        return Rs, cts, st

    @staticmethod
    def open_batch(sks, Rs, nonces, cts, l, device=0):
        """The receiving side of seal_batch: ks = sk R (one mul_batch), msg = decrypt(ks, ct, nonce, l).  -> (msgs, statuses)"""
        kss, st_k = ecgfp5.mul_batch(sks, Rs, device)
        msgs, st = poseidon_native.decrypt_batch(kss, nonces, cts, l, device)
        for i in range(len(st)):
            if st_k[i]:
                st[i], msgs[i] = st_k[i], [(0,) * 5] * l
        return msgs, st


def _pt(point):
    return _arr(list(point[0]) + list(point[1]))


def _pt_out(buf):
    return (tuple(buf[0:5]), tuple(buf[5:10]))


def _sc(k):
    return _arr([(k >> (64 * i)) & (2**64 - 1) for i in range(5)])


class ecgfp5:
    """The ecgfp5 crate's native side (ecgfp5/src/lib.rs, elgamal.rs, hashed_elgamal.rs) through the C ABI.  A Point is
    ((x0..x4), (u0..u4)); scalars are Python ints.  Randomness comes from the OS CSPRNG as upstream's OsRng; an explicit seed (tests only) makes it reproducible."""

    @staticmethod
    def group_order():
        out = (u64 * 5)()
        lib().p2_ecgfp5_group_order(out)
        return sum(int(out[i]) << (64 * i) for i in range(5))

    @staticmethod
    def generator():
        out = (u64 * 10)()
        lib().p2_ecgfp5_generator(out)
        return _pt_out(out)

    @staticmethod
    def mul(k, point):
        out = (u64 * 10)()
        lib().p2_ecgfp5_mul(_sc(k), _pt(point), out)
        return _pt_out(out)

    @staticmethod
    def add(p, q):
        out = (u64 * 10)()
        lib().p2_ecgfp5_add(_pt(p), _pt(q), out)
        return _pt_out(out)

    @staticmethod
    def neg(p):
        out = (u64 * 10)()
        lib().p2_ecgfp5_neg(_pt(p), out)
        return _pt_out(out)

    @staticmethod
    def is_in_subgroup(p): return bool(lib().p2_ecgfp5_is_in_subgroup(_pt(p)))

    @staticmethod
    def compress_from_subgroup(p):
        out = (u64 * 5)()
        lib().p2_ecgfp5_compress(_pt(p), out)
        return tuple(out)

    @staticmethod
    def decompress_into_subgroup(w):
        out = (u64 * 10)()
        if lib().p2_ecgfp5_decompress(_arr(list(w)), out):
            raise P2Error(_err())
        return _pt_out(out)

    @staticmethod
    def random_scalar(seed=None):
        """Uniform scalar below the group order from the OS CSPRNG; a `seed` (tests / benchmarks only) makes it reproducible
        and is NOT a source of key material."""
        out = (u64 * 5)()
        if seed is None:
            if lib().p2_ecgfp5_random_scalar(out):
                raise P2Error(_err())
        else:
            lib().p2_ecgfp5_random_scalar_seeded(seed, out)
        return sum(int(out[i]) << (64 * i) for i in range(5))

    @staticmethod
    def new_rand_from_subgroup(seed=None):
        out = (u64 * 10)()
        if seed is None:
            if lib().p2_ecgfp5_random_point(out):
                raise P2Error(_err())
        else:
            lib().p2_ecgfp5_random_point_seeded(seed, out)
        return _pt_out(out)

    @staticmethod
    def encode_binary(x, seed=None):                       # lib.rs:48
        assert 0 <= x < 1 << 160
        out = (u64 * 10)()
        limbs = (C.c_uint32 * 5)(*[(x >> (32 * i)) & 0xFFFFFFFF for i in range(5)])
        if seed is None:
            if lib().p2_ecgfp5_encode_binary(limbs, out):
                raise P2Error(_err())
        else:
            lib().p2_ecgfp5_encode_binary_seeded(limbs, seed, out)
        return _pt_out(out)

    @staticmethod
    def decode_binary(p):                                  # lib.rs:80
        out = (C.c_uint32 * 5)()
        lib().p2_ecgfp5_decode_binary(_pt(p), out)
        return sum(int(out[i]) << (32 * i) for i in range(5))

    @staticmethod
    def elgamal_encrypt(pk, nonce, msg):                   # elgamal.rs:11
        c0, c1 = (u64 * 10)(), (u64 * 10)()
        if lib().p2_elgamal_encrypt(_pt(pk), _sc(nonce), _pt(msg), c0, c1):
            raise P2Error(_err())
        return _pt_out(c0), _pt_out(c1)

    @staticmethod
    def elgamal_decrypt(sk, ct):                           # elgamal.rs:19
        out = (u64 * 10)()
        if lib().p2_elgamal_decrypt(_sc(sk.value), _pt(ct[0]), _pt(ct[1]), out):
            raise P2Error(_err())
        return _pt_out(out)

    @staticmethod
    def hashed_elgamal_encrypt(pk, nonce, msg):            # hashed_elgamal.rs:19
        c0, ct = (u64 * 10)(), (u64 * 5)()
        if lib().p2_hashed_elgamal_encrypt(_pt(pk), _sc(nonce), _arr(list(msg)), c0, ct):
            raise P2Error(_err())
        return _pt_out(c0), tuple(ct)

    @staticmethod
    def hashed_elgamal_decrypt(sk, ct):                    # hashed_elgamal.rs:28
        out = (u64 * 5)()
        if lib().p2_hashed_elgamal_decrypt(_sc(sk.value), _pt(ct[0]), _arr(list(ct[1])), out):
            raise P2Error(_err())
        return tuple(out)

    @staticmethod
    def scalar_muladd(a, b, c):
        """(a b + c) mod the group order for any a, b, c below 2^320"""
        out = (u64 * 5)()
        lib().p2_ecgfp5_scalar_muladd(_sc(a), _sc(b), _sc(c), out)
        return _int5(out)

    @staticmethod
    def mul_batch(scalars, points, device=0):
        """[k P for k, P in zip(scalars, points)] on a GPU (p2_ecgfp5_mul_batch), with one status per item: 0, or 2 (and the
        neutral as output) for a point with a word not below p or outside the group.  device=None: a host loop."""
        ks, n, _ = _rows([_sc_words(k) for k in scalars], "scalars")
        ps, n_p, _ = _rows([list(p[0]) + list(p[1]) for p in points], "points")

        def host(i, outs, status):
            pt = _pt_out(ps[10 * i:10 * i + 10])
            ok = all(w < P for w in pt[0] + pt[1]) and ecgfp5.is_in_subgroup(pt)
            status[i] = 0 if ok else 2
            if ok:
                outs[0][10 * i:10 * i + 10] = list(sum(ecgfp5.mul(_int5(ks[5 * i:5 * i + 5]), pt), ()))
        (out,), st = _batch_call("p2_ecgfp5_mul_batch", [n, n_p], "mul_batch: one point per scalar", [(u64, 10)], device, host,
                                 lambda fn, n, outs, status: fn(ks, ps, n, outs[0], status, device))
        return _points_out(out, len(st)), st

    @staticmethod
    def mul_batch_device(d_k, d_p, count, d_out, d_status, device=0, stream=None):
        """Every buffer a raw device pointer (p2_ecgfp5_mul_batch_device); asynchronous on `stream`."""
        _device_call("p2_ecgfp5_mul_batch_device", d_k, d_p, count, d_out, d_status, device, stream)

    # ---- ElGamal in GPU batches (csrc/kernels_elgamal.h).  Every list is per item; a caller with one key repeats it.  Statuses:
    # 0 done, 1 no result, 2 malformed (a word not below p, a scalar not below n, a point outside the group); a row whose status
    # is not 0 holds zeros.  device=None: a host loop over the single-item entry points with the same checks.
    DONE, NO_RESULT, MALFORMED = 0, 1, 2

    @staticmethod
    def _point_rows(points, what):
        arr, n, k = _rows([list(p[0]) + list(p[1]) for p in points], what)
        if n and k != 10:
            raise P2Error("%s are points of ten words" % what)
        return arr, n

    @staticmethod
    def _word_rows(rows, what):
        arr, n, k = _rows(rows, what)
        if n and k != 5:
            raise P2Error("%s are rows of five words" % what)
        return arr, n

    @staticmethod
    def _point_ok(arr, i):
        return all(w < P for w in arr[10 * i:10 * i + 10]) and bool(lib().p2_ecgfp5_is_in_subgroup(_at(arr, 10 * i)))

    @staticmethod
    def _scalar_ok(arr, i):
        return _int5(arr[5 * i:5 * i + 5]) < ecgfp5.group_order()

    @staticmethod
    def _elgamal_call(name, ins, out_widths, device, ok, twin):
        """What the four ciphers hand to _batch_call.  ins: three (array, n); -> ([flat output arrays], statuses).  The host loop
        calls the single-item entry point twin(i, outs) where ok(i)."""
        def host(i, outs, status):
            if not ok(i):
                status[i] = ecgfp5.MALFORMED
            elif twin(i, outs):
                raise P2Error(name + " (host) failed: " + _err())
        return _batch_call("p2_" + name, [m for _, m in ins], name + ": every list has one entry per item", [(u64, w) for w in out_widths], device, host,
                           lambda fn, n, outs, status: fn(*[a for a, _ in ins], n, *outs, status, device))

    @staticmethod
    def decompress_batch(ws, device=0):
        """-> (points, statuses): decompress_into_subgroup per item; status 1 where w encodes no group element"""
        w, n = ecgfp5._word_rows(ws, "compressed points")

        def host(i, outs, status):
            if any(v >= P for v in w[5 * i:5 * i + 5]):
                status[i] = ecgfp5.MALFORMED
            else:
                status[i] = ecgfp5.NO_RESULT if lib().p2_ecgfp5_decompress(_at(w, 5 * i), _at(outs[0], 10 * i)) else ecgfp5.DONE
        (out,), st = _batch_call("p2_ecgfp5_decompress_batch", [n], None, [(u64, 10)], device, host, lambda fn, n, outs, status: fn(w, n, outs[0], status, device))
        return _points_out(out, len(st)), st

    @staticmethod
    def _encode_args(xs, pads):
        xs, pads = [int(x) for x in xs], [[list(a) for a in p] for p in pads]
        n, attempts = len(xs), len(pads[0]) if pads else 0
        if len(pads) != n or any(len(p) != attempts or any(len(a) != 5 for a in p) for p in pads):
            raise P2Error("encode_binary_batch: per item one message and one list of `attempts` rows of five 32-bit pad words")
        flat = [int(v) for p in pads for a in p for v in a]
        if any(not 0 <= x < 1 << 160 for x in xs) or any(not 0 <= v < 1 << 32 for v in flat):
            raise P2Error("encode_binary_batch: messages are below 2^160, pad words below 2^32")
        limbs = (C.c_uint32 * (5 * n))(*[(x >> (32 * j)) & 0xFFFFFFFF for x in xs for j in range(5)])
        return limbs, (C.c_uint32 * max(len(flat), 1))(*flat), n, attempts

    @staticmethod
    def encode_binary_batch(xs, pads, device=0):
        """encode_binary (lib.rs:48) with the random high halves supplied: xs are messages below 2^160, pads[i] a list of `attempts`
        rows of five 32-bit words (draw them from a CSPRNG: they hide nothing, but a fixed list makes encodings recognisable).
        -> (points, used, statuses): used[i] the number of the attempt taken; status 1 and used = attempts where none decodes."""
        limbs, pad, n, attempts = ecgfp5._encode_args(xs, pads)

        def host(i, outs, status):
            if not 1 <= attempts <= 256:
                raise P2Error("attempts is between 1 and 256")
            u = C.c_uint32()
            rc = lib().p2_ecgfp5_encode_binary_padded(C.cast(C.byref(limbs, 20 * i), u32p), C.cast(C.byref(pad, 20 * attempts * i), u32p), attempts, _at(outs[0], 10 * i),
                                                     C.byref(u))
            outs[1][i], status[i] = u.value, ecgfp5.NO_RESULT if rc else ecgfp5.DONE
        (out, used), st = _batch_call("p2_ecgfp5_encode_binary_batch", [n], None, [(u64, 10), (C.c_uint32, 1)], device, host,
                                      lambda fn, n, outs, status: fn(limbs, pad, attempts, n, *outs, status, device))
        return _points_out(out, len(st)), list(used), st

    @staticmethod
    def decode_binary_batch(points):
        """decode_binary (lib.rs:80) per point, on the host: the low halves of u"""
        return [sum((int(p[1][j]) & 0xFFFFFFFF) << (32 * j) for j in range(5)) for p in points]

    @staticmethod
    def elgamal_encrypt_batch(pks, nonces, msgs, device=0):
        """-> (c0s, c1s, statuses): c0 = nonce G, c1 = msg + nonce pk (elgamal.rs:11)"""
        pk, k, m = ecgfp5._point_rows(pks, "public keys"), _rows([_sc_words(x) for x in nonces], "nonces")[:2], ecgfp5._point_rows(msgs, "messages")
        outs, st = ecgfp5._elgamal_call(
            "elgamal_encrypt_batch", [pk, k, m], (10, 10), device, lambda i: ecgfp5._scalar_ok(k[0], i) and ecgfp5._point_ok(pk[0], i) and ecgfp5._point_ok(m[0], i),
            lambda i, o: lib().p2_elgamal_encrypt(_at(pk[0], 10 * i), _at(k[0], 5 * i), _at(m[0], 10 * i), _at(o[0], 10 * i), _at(o[1], 10 * i)))
        return _points_out(outs[0], len(st)), _points_out(outs[1], len(st)), st

    @staticmethod
    def elgamal_decrypt_batch(sks, c0s, c1s, device=0):
        """-> (msgs, statuses): msg = c1 - sk c0 (elgamal.rs:19); sks are Python ints"""
        k, a, b = _rows([_sc_words(x) for x in sks], "secret keys")[:2], ecgfp5._point_rows(c0s, "c0"), ecgfp5._point_rows(c1s, "c1")
        outs, st = ecgfp5._elgamal_call(
            "elgamal_decrypt_batch", [k, a, b], (10,), device, lambda i: ecgfp5._scalar_ok(k[0], i) and ecgfp5._point_ok(a[0], i) and ecgfp5._point_ok(b[0], i),
            lambda i, o: lib().p2_elgamal_decrypt(_at(k[0], 5 * i), _at(a[0], 10 * i), _at(b[0], 10 * i), _at(o[0], 10 * i)))
        return _points_out(outs[0], len(st)), st

    @staticmethod
    def hashed_elgamal_encrypt_batch(pks, nonces, msgs, device=0):
        """-> (c0s, cts, statuses): messages and ciphertexts are five field elements (hashed_elgamal.rs:19)"""
        pk, k, m = ecgfp5._point_rows(pks, "public keys"), _rows([_sc_words(x) for x in nonces], "nonces")[:2], ecgfp5._word_rows(msgs, "messages")
        outs, st = ecgfp5._elgamal_call(
            "hashed_elgamal_encrypt_batch", [pk, k, m], (10, 5), device,
            lambda i: ecgfp5._scalar_ok(k[0], i) and all(w < P for w in m[0][5 * i:5 * i + 5]) and ecgfp5._point_ok(pk[0], i),
            lambda i, o: lib().p2_hashed_elgamal_encrypt(_at(pk[0], 10 * i), _at(k[0], 5 * i), _at(m[0], 5 * i), _at(o[0], 10 * i), _at(o[1], 5 * i)))
        return _points_out(outs[0], len(st)), [tuple(outs[1][5 * i:5 * i + 5]) for i in range(len(st))], st

    @staticmethod
    def hashed_elgamal_decrypt_batch(sks, c0s, cts, device=0):
        """-> (msgs, statuses) (hashed_elgamal.rs:28)"""
        k, a, c = _rows([_sc_words(x) for x in sks], "secret keys")[:2], ecgfp5._point_rows(c0s, "c0"), ecgfp5._word_rows(cts, "ciphertexts")
        outs, st = ecgfp5._elgamal_call(
            "hashed_elgamal_decrypt_batch", [k, a, c], (5,), device,
            lambda i: ecgfp5._scalar_ok(k[0], i) and all(w < P for w in c[0][5 * i:5 * i + 5]) and ecgfp5._point_ok(a[0], i),
            lambda i, o: lib().p2_hashed_elgamal_decrypt(_at(k[0], 5 * i), _at(a[0], 10 * i), _at(c[0], 5 * i), _at(o[0], 5 * i)))
        return [tuple(outs[0][5 * i:5 * i + 5]) for i in range(len(st))], st

    # the _device forms: every buffer a raw device pointer, asynchronous on `stream`; keys and nonces stay in device memory
    @staticmethod
    def decompress_batch_device(d_w, count, d_out, d_status, device=0, stream=None):
        _device_call("p2_ecgfp5_decompress_batch_device", d_w, count, d_out, d_status, device, stream)

    @staticmethod
    def encode_binary_batch_device(d_limbs, d_pad, attempts, count, d_out, d_used, d_status, device=0, stream=None):
        _device_call("p2_ecgfp5_encode_binary_batch_device", d_limbs, d_pad, attempts, count, d_out, d_used, d_status, device, stream)

    @staticmethod
    def elgamal_encrypt_batch_device(d_pk, d_nonce, d_msg, count, d_c0, d_c1, d_status, device=0, stream=None):
        _device_call("p2_elgamal_encrypt_batch_device", d_pk, d_nonce, d_msg, count, d_c0, d_c1, d_status, device, stream)

    @staticmethod
    def elgamal_decrypt_batch_device(d_sk, d_c0, d_c1, count, d_msg, d_status, device=0, stream=None):
        _device_call("p2_elgamal_decrypt_batch_device", d_sk, d_c0, d_c1, count, d_msg, d_status, device, stream)

    @staticmethod
    def hashed_elgamal_encrypt_batch_device(d_pk, d_nonce, d_msg, count, d_c0, d_ct, d_status, device=0, stream=None):
        _device_call("p2_hashed_elgamal_encrypt_batch_device", d_pk, d_nonce, d_msg, count, d_c0, d_ct, d_status, device, stream)

    @staticmethod
    def hashed_elgamal_decrypt_batch_device(d_sk, d_c0, d_ct, count, d_msg, d_status, device=0, stream=None):
        _device_call("p2_hashed_elgamal_decrypt_batch_device", d_sk, d_c0, d_ct, count, d_msg, d_status, device, stream)

    @staticmethod
    def scalar_bits_device(d_k, count, d_out, stride, device=0, stream=None):
        """d_out[i stride + j] = bit j of scalar i (j < 320 <= stride, in words): a scalar's 320 bit targets in a row of the value
        matrix that prove_batch_device reads, without the host spelling the bits"""
        _device_call("p2_ecgfp5_scalar_bits_device", d_k, count, d_out, stride, device, stream)


def _at(arr, words):
    """pointer to word `words` of a u64 array"""
    return C.cast(C.byref(arr, 8 * words), u64p)


def _points_out(buf, n):
    return [_pt_out(buf[10 * i:10 * i + 10]) for i in range(n)]


def _int5(words):
    return sum(int(words[i]) << (64 * i) for i in range(5))


def _sc_words(k):
    k = int(k)
    if not 0 <= k < 1 << 320:
        raise P2Error("a scalar is below 2^320")
    return [(k >> (64 * i)) & (2**64 - 1) for i in range(5)]


class schnorr:
    """Schnorr signatures on ecGFp5 with a Poseidon challenge (csrc/schnorr.h; UNPINNED against pod2).
    A secret key and a nonce are Python ints in [1, n); a public key is a Point; a message a list of canonical field elements
    (at most 1024); a signature is (s, (e0, e1, e2, e3)).  Statuses: 0 accepted, 1 rejected, 2 malformed."""

    ACCEPTED, REJECTED, MALFORMED = 0, 1, 2

    @staticmethod
    def _sig_words(sig):
        s, e = sig
        return _sc_words(s) + [int(w) for w in _hash4(e)]

    @staticmethod
    def _sig_out(buf):
        return _int5(buf), tuple(int(w) for w in buf[5:9])

    @staticmethod
    def challenge(r, pk, msg):
        msg = [int(w) for w in msg]
        e = (u64 * 4)()
        if lib().p2_schnorr_challenge(_pt(r), _pt(pk), _arr(msg) if msg else None, len(msg), e):
            raise P2Error(_err())
        return tuple(e)

    @staticmethod
    def sign(sk, msg, nonce=None):
        """nonce=None draws one from ecgfp5.random_scalar() (the OS CSPRNG); a nonce must never sign two messages"""
        if nonce is None:
            nonce = ecgfp5.random_scalar()
            while nonce == 0:
                nonce = ecgfp5.random_scalar()
        msg = [int(w) for w in msg]
        sig, st = (u64 * 9)(), C.c_int()
        if lib().p2_schnorr_sign(_arr(_sc_words(sk)), _arr(_sc_words(nonce)), _arr(msg) if msg else None, len(msg), sig, None, C.byref(st)):
            raise P2Error(_err())
        if st.value:
            raise P2Error("schnorr.sign: the secret key and the nonce must be in [1, n), message words below p")
        return schnorr._sig_out(sig)

    @staticmethod
    def verify(pk, msg, sig):
        return schnorr.verify_batch([pk], [msg], [sig], device=None)[0]

    @staticmethod
    def sign_batch(sks, msgs, nonces, device=0):
        """-> (signatures, public keys, statuses); a row with status 2 holds zeros.  device=None: the host twin."""
        sk, n, _ = _rows([_sc_words(k) for k in sks], "secret keys")
        ks, n_k, _ = _rows([_sc_words(k) for k in nonces], "nonces")
        mg, n_m, msg_len = _rows(msgs, "messages")

        def host(i, outs, status):
            st = C.c_int()
            if lib().p2_schnorr_sign(_at(sk, 5 * i), _at(ks, 5 * i), _at(mg, i * msg_len) if msg_len else None, msg_len, _at(outs[0], 9 * i), _at(outs[1], 10 * i), C.byref(st)):
                raise P2Error("p2_schnorr_sign failed: " + _err())
            status[i] = st.value
        (sig, pk), st = _batch_call("p2_schnorr_sign_batch", [n, n_k, n_m], "sign_batch: one nonce and one message per secret key", [(u64, 9), (u64, 10)], device, host,
                                    lambda fn, n, outs, status: fn(sk, ks, mg, msg_len, n, *outs, status, device))
        return [schnorr._sig_out(sig[9 * i:9 * i + 9]) for i in range(len(st))], _points_out(pk, len(st)), st

    @staticmethod
    def verify_batch(pks, msgs, sigs, device=0):
        """-> statuses.  Words of pk, msg and e may be any 64-bit value (such rows are malformed); s any value below 2^320.
        device=None: the host twin."""
        pk, n, _ = _rows([list(p[0]) + list(p[1]) for p in pks], "public keys")
        mg, n_m, msg_len = _rows(msgs, "messages")
        sg, n_s, _ = _rows([_sc_words(s[0]) + [int(w) for w in s[1]] for s in sigs], "signatures")

        def host(i, outs, status):
            st = C.c_int()
            if lib().p2_schnorr_verify(_at(pk, 10 * i), _at(mg, i * msg_len) if msg_len else None, msg_len, _at(sg, 9 * i), C.byref(st)):
                raise P2Error("p2_schnorr_verify failed: " + _err())
            status[i] = st.value
        return _batch_call("p2_schnorr_verify_batch", [n, n_m, n_s], "verify_batch: one message and one signature per public key", [], device, host,
                           lambda fn, n, outs, status: fn(pk, mg, msg_len, sg, n, status, device))[1]

    @staticmethod
    def sign_batch_device(d_sk, d_nonce, d_msg, msg_len, count, d_sig, d_pk, d_status, device=0, stream=None):
        """Every buffer a raw device pointer (p2_schnorr_sign_batch_device; d_pk may be None); asynchronous on `stream`.  The
        secret keys and nonces stay in device memory the caller owns."""
        _device_call("p2_schnorr_sign_batch_device", d_sk, d_nonce, d_msg, msg_len, count, d_sig, d_pk, d_status, device, stream)

    @staticmethod
    def verify_batch_device(d_pk, d_msg, msg_len, d_sig, count, d_status, device=0, stream=None):
        _device_call("p2_schnorr_verify_batch_device", d_pk, d_msg, msg_len, d_sig, count, d_status, device, stream)


class ECGFP5SecretKey:
    """ecgfp5/src/lib.rs:23-42."""

    def __init__(self, s):
        assert 0 <= s < ecgfp5.group_order()
        self.value = s

    @staticmethod
    def rand(seed=None): return ECGFP5SecretKey(ecgfp5.random_scalar(seed))   # lib.rs:35 OsRng; seed = tests only

    def public_key(self): return ecgfp5.mul(self.value, ecgfp5.generator())


class native:
    """aes-gcm/src/native_aes.rs / native_gcm.rs through the C ABI."""

    @staticmethod
    def gf_2_8_mul(a, b): return lib().p2_native_gf_2_8_mul(a, b)

    @staticmethod
    def key_expansion(key):
        nk = len(key) // 4
        out = C.create_string_buffer(16 * (nk + 7))
        lib().p2_native_aes_key_expansion(bytes(key), nk, nk + 6, out)
        return out.raw

    @staticmethod
    def encrypt_block(key, block):
        nk = len(key) // 4
        out = C.create_string_buffer(16)
        lib().p2_native_aes_encrypt_block(bytes(key), nk, nk + 6, bytes(block), out)
        return out.raw

    @staticmethod
    def gf_2_128_mul(x, y):
        out = C.create_string_buffer(16)
        lib().p2_native_gf_2_128_mul(bytes(x), bytes(y), out)
        return out.raw

    @staticmethod
    def ghash(h, x):
        out = C.create_string_buffer(16)
        lib().p2_native_ghash(bytes(h), bytes(x), len(x), out)
        return out.raw

    @staticmethod
    def gctr(key, icb, x):
        nk = len(key) // 4
        out = C.create_string_buffer(max(len(x), 1))
        lib().p2_native_gctr(bytes(key), nk, nk + 6, bytes(icb), bytes(x), len(x), out)
        return out.raw[: len(x)]

    @staticmethod
    def gcm_encrypt(key, nonce, pt, aad=b""):
        """aad: additional authenticated data (SP 800-38D), which the reference leaves out; b"" is native_gcm::encrypt"""
        nk = len(key) // 4
        ct, tag = C.create_string_buffer(max(len(pt), 1)), C.create_string_buffer(16)
        lib().p2_native_aes_gcm_encrypt_aad(bytes(key), nk, nk + 6, bytes(nonce), bytes(aad), len(aad), bytes(pt), len(pt), ct, tag)
        return ct.raw[: len(pt)], tag.raw

    @staticmethod
    def gcm_decrypt(key, nonce, ct, tag, aad=b""):
        """-> the plaintext; P2Error when the tag over (aad, ct) does not match"""
        nk = native._nk(key)
        if len(nonce) != 12 or len(tag) != 16:
            raise P2Error("gcm_decrypt: a nonce is 12 bytes, a tag 16")
        pt = C.create_string_buffer(max(len(ct), 1))
        if lib().p2_native_aes_gcm_decrypt(bytes(key), nk, nk + 6, bytes(nonce), bytes(aad), len(aad), bytes(ct), len(ct), bytes(tag), pt):
            raise P2Error(_err())
        return pt.raw[: len(ct)]

    # ---- AES-GCM in GPU batches (csrc/kernels_gcm.h).  Every list is per item and holds bytes: keys of
    # 16, 24 or 32 bytes, nonces of 12, tags of 16; within a call all keys have one length, all messages one length (at most
    # 2^24) and all aads one length (at most 2^16; aads=None is no aad).  Statuses: 0 done, 1 (decrypt) the tag does not match
    # and the plaintext row holds zeros.  device=None: a host loop over gcm_encrypt / gcm_decrypt's entry points.
    DONE, REJECTED = 0, 1
    MAX_LEN, MAX_AAD = 1 << 24, 1 << 16

    @staticmethod
    def _nk(key):
        if len(key) not in (16, 24, 32):
            raise P2Error("a key is 16, 24 or 32 bytes (nk is 4, 6 or 8)")
        return len(key) // 4

    @staticmethod
    def _byte_rows(rows, what):
        """[n] byte strings of one length -> (their concatenation, n, that length)"""
        rows = [bytes(r) for r in rows]
        k = len(rows[0]) if rows else 0
        if any(len(r) != k for r in rows):
            raise P2Error("%s must all have one length" % what)
        return b"".join(rows), len(rows), k

    @staticmethod
    def _gcm_args(name, keys, nonces, rows, aads, tags=None):
        """-> (key, nonce, rows, aad, tag or None, nk, len, aad_len, list lengths)"""
        key, n, kl = native._byte_rows(keys, "keys")
        nn, n_n, nl = native._byte_rows(nonces, "nonces")
        data, n_r, l = native._byte_rows(rows, "messages and ciphertexts")
        aad, n_a, al = native._byte_rows(aads if aads is not None else [b""] * n, "aads")
        tag, n_t, tl = native._byte_rows(tags, "tags") if tags is not None else (None, n, 16)
        counts = [n, n_n, n_r, n_a, n_t]
        nk = native._nk(key[:kl]) if n else 4
        if n and all(m == n for m in counts):
            if nl != 12 or tl != 16:
                raise P2Error("%s: nonces are 12 bytes, tags 16" % name)
            if l > native.MAX_LEN or al > native.MAX_AAD:
                raise P2Error("%s: a message is at most 2^24 bytes, an aad at most 2^16" % name)
        return key, nn, data, aad, tag, nk, l, al, counts

    @staticmethod
    def gcm_batch_workspace(nk, length, aad_len, count):
        """bytes of the d_work that the _device forms take"""
        if nk not in (4, 6, 8):
            raise P2Error("nk is 4, 6 or 8")
        return lib().p2_aes_gcm_batch_workspace(nk, length, aad_len, count)

    @staticmethod
    def gcm_encrypt_batch(keys, nonces, pts, aads=None, device=0):
        """-> (cts, tags, statuses): (cts[i], tags[i]) = gcm_encrypt(keys[i], nonces[i], pts[i], aads[i])"""
        key, nn, pt, aad, _, nk, l, al, counts = native._gcm_args("gcm_encrypt_batch", keys, nonces, pts, aads)
        kl = 4 * nk

        def host(i, outs, status):
            ct, tag = native.gcm_encrypt(key[kl * i:kl * (i + 1)], nn[12 * i:12 * (i + 1)], pt[l * i:l * (i + 1)], aad[al * i:al * (i + 1)])
            outs[0][l * i:l * (i + 1)] = ct
            outs[1][16 * i:16 * (i + 1)] = tag
        (ct, tag), st = _batch_call("p2_aes_gcm_encrypt_batch", counts, "gcm_encrypt_batch: every list has one entry per item", [(C.c_char, l), (C.c_char, 16)], device, host,
                                    lambda fn, n, outs, status: fn(key, nk, nn, aad, al, pt, l, n, outs[0], outs[1], status, device))
        n = len(st)
        ct, tag = (ct.raw, tag.raw) if n else (b"", b"")
        return [ct[l * i:l * (i + 1)] for i in range(n)], [tag[16 * i:16 * (i + 1)] for i in range(n)], st

    @staticmethod
    def gcm_decrypt_batch(keys, nonces, cts, tags, aads=None, device=0):
        """-> (pts, statuses): pts[i] = gcm_decrypt(keys[i], nonces[i], cts[i], tags[i], aads[i]); status 1 and zeros where it raises"""
        key, nn, ct, aad, tag, nk, l, al, counts = native._gcm_args("gcm_decrypt_batch", keys, nonces, cts, aads, tags)
        kl = 4 * nk

        def host(i, outs, status):
            try:
                outs[0][l * i:l * (i + 1)] = native.gcm_decrypt(key[kl * i:kl * (i + 1)], nn[12 * i:12 * (i + 1)], ct[l * i:l * (i + 1)], tag[16 * i:16 * (i + 1)],
                                                                aad[al * i:al * (i + 1)])
            except P2Error:
                status[i] = native.REJECTED
        (pt,), st = _batch_call("p2_aes_gcm_decrypt_batch", counts, "gcm_decrypt_batch: every list has one entry per item", [(C.c_char, l)], device, host,
                                lambda fn, n, outs, status: fn(key, nk, nn, aad, al, ct, tag, l, n, outs[0], status, device))
        n = len(st)
        pt = pt.raw if n else b""
        return [pt[l * i:l * (i + 1)] for i in range(n)], st

    @staticmethod
    def gcm_encrypt_batch_device(d_key, nk, d_nonce, d_aad, aad_len, d_pt, length, row_stride, count, d_ct, d_tag, d_status, d_work, device=0, stream=None):
        """Every buffer a raw device pointer (p2_aes_gcm_encrypt_batch_device); asynchronous on `stream`.  pt and ct rows are
        row_stride >= length bytes apart; d_work: gcm_batch_workspace(...) bytes, 16-byte aligned."""
        _device_call("p2_aes_gcm_encrypt_batch_device", d_key, nk, d_nonce, d_aad, aad_len, d_pt, length, row_stride, count, d_ct, d_tag, d_status, d_work, device, stream)

    @staticmethod
    def gcm_decrypt_batch_device(d_key, nk, d_nonce, d_aad, aad_len, d_ct, d_tag, length, row_stride, count, d_pt, d_status, d_work, device=0, stream=None):
        _device_call("p2_aes_gcm_decrypt_batch_device", d_key, nk, d_nonce, d_aad, aad_len, d_ct, d_tag, length, row_stride, count, d_pt, d_status, d_work, device, stream)

    @staticmethod
    def bytes_to_words_device(d_bytes, row_bytes, byte_stride, count, d_out, stride_words, device=0, stream=None):
        """d_out[i stride_words + j] = d_bytes[i byte_stride + j] (j < row_bytes <= stride_words): a byte row as the ByteTarget
        segment of a row of the value matrix that prove_batch_device reads, without a host round trip"""
        _device_call("p2_bytes_to_words_device", d_bytes, row_bytes, byte_stride, count, d_out, stride_words, device, stream)
