/* p2aes.h -- C ABI of the MI355X-native Plonky2 proving backend for the 0xPARC/plonky2-aes gadget circuits.
 *
 * This is the drop-in boundary.  The reference calls the third-party `plonky2` crate
 * through five kinds of call sites; each group of entry points below replaces one of them:
 *
 *   reference call site (file:line)                                          entry points here
 *   ---------------------------------------------------------------------    --------------------------------
 *   CircuitBuilder::<F,D>::new(config) + builder methods                     p2_builder_*
 *     aes-gcm/src/circuit_aes.rs:178,182,186,193,249,250,300,317,334,356,357
 *     aes-gcm/src/circuit_gcm.rs:163,314,323,339,342,356,361-364,396,403,415,423,424
 *   gadget constructors (AesGcmTarget::build etc.)                           p2_aes_*, p2_gcm_*
 *     aes-gcm/src/circuit_gcm.rs:49-172, aes-gcm/src/circuit_aes.rs:76-275
 *   builder.build::<PoseidonGoldilocksConfig>()                              p2_builder_build -> blob,
 *     aes-gcm/src/circuit_gcm.rs:771, examples/aes_gcm_128.rs:46 (19 sites)  p2_circuit_load (GPU preprocessing)
 *   PartialWitness::new / pw.set_target / data.prove(pw)   ** HOT PATH **    p2_prove_batch
 *     aes-gcm/src/circuit_aes.rs:283, circuit_gcm.rs:779-781 (20 sites)
 *   data.verify(proof)                                                       p2_verify (host),
 *     aes-gcm/src/circuit_gcm.rs:782 (19 sites)                              p2_verify_batch (GPU, batched)
 *   native_gcm::encrypt (witness values)  aes-gcm/src/native_gcm.rs:16       p2_native_aes_gcm_encrypt(_aad), in GPU batches
 *                                                                            p2_aes_gcm_encrypt_batch, p2_aes_gcm_decrypt_batch
 *   MerkleTree::new / prove, verify_merkle_proof_to_cap (upstream plonky2;   p2_merkle_tree_*, p2_merkle_verify_batch,
 *     not called by the reference: committed sets for pod2-style users)      p2_builder_verify_merkle_proof_to_cap
 *   MerkleMap: sparse keyed trees with non-membership proofs (this project's  p2_merkle_map_*, p2_native_merkle_map_*,
 *     own scheme, UNPINNED against pod2: revocation lists, nullifier sets)   p2_builder_merkle_map_*
 *
 * Conventions: plain pointers and sizes only; every function that can fail returns 0 on success and a
 * non-zero code otherwise, with a thread-local message available from p2_last_error().  The caller owns
 * every buffer it passes in; the library owns handles and all device memory.  Nothing here touches the CPU
 * oracle under oracle/: proving runs on the GPU or fails with P2_ERR_NO_DEVICE.
 */
#ifndef P2AES_H
#define P2AES_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    P2_OK = 0,
    P2_ERR_INVALID = 1,   /* bad argument / malformed blob or proof */
    P2_ERR_NO_DEVICE = 2, /* no usable HIP device: proving has no CPU fallback */
    P2_ERR_HIP = 3,       /* a HIP runtime call failed */
    P2_ERR_VERIFY = 4     /* proof rejected (reason in p2_last_error) */
};
/* per-proof status written by p2_prove_batch (mirrors `data.prove(pw)` returning Err, circuit_aes.rs:403-405) */
enum {
    P2_PROOF_OK = 0,
    P2_PROOF_WITNESS_CONFLICT = 1, /* generator output conflicts with a pre-set target, or lookup input not in table */
    P2_PROOF_MISSING_INPUT = 2,    /* some generator never ran: an input target was not set */
    P2_PROOF_ZETA_IN_SUBGROUP = 3, /* "Opening point is in the subgroup." */
    P2_PROOF_POW_NOT_FOUND = 4     /* no proof-of-work witness among the 2^21 candidates searched (probability ~e^-32) */
};
/* per-proof verdict written by p2_verify_batch: the reason class verify_proof (csrc/verifier.h) would return first */
enum {
    P2_VERIFY_OK = 0,
    P2_VERIFY_SHAPE = 1,             /* "proof truncated", "trailing bytes in proof", "Merkle path of the wrong depth (...)" */
    P2_VERIFY_NON_CANONICAL = 2,     /* "non-canonical field element", "hash word out of range" (Keccak circuits) */
    P2_VERIFY_POW = 3,               /* "Invalid proof-of-work witness." */
    P2_VERIFY_ZETA_IN_SUBGROUP = 4,  /* "Opening point is in the subgroup." */
    P2_VERIFY_VANISHING = 5,         /* "vanishing polynomial identity does not hold at zeta" */
    P2_VERIFY_MERKLE_INITIAL = 6,    /* "Invalid Merkle proof (initial tree)." */
    P2_VERIFY_FRI_FOLD = 7,          /* "FRI fold consistency check failed." */
    P2_VERIFY_MERKLE_FRI = 8,        /* "Invalid Merkle proof (FRI round)." */
    P2_VERIFY_FINAL_POLY = 9         /* "Final polynomial evaluation is invalid." */
};

const char* p2_last_error(void);

/* ------------------------------------------------------------------ CircuitBuilder (host) */
typedef struct p2_builder p2_builder;
/* Targets are opaque 64-bit handles (virtual target index, or a routed wire). */
typedef uint64_t p2_target;

p2_builder* p2_builder_new(void);    /* CircuitConfig::standard_recursion_config() */
p2_builder* p2_builder_new_zk(void); /* CircuitConfig::standard_recursion_zk_config() (examples/aes_gcm_128.rs:36) */
/* The hash configuration of a circuit.  P2_HASHER_POSEIDON is PoseidonGoldilocksConfig (what p2_builder_new / _new_zk build).
 * P2_HASHER_KECCAK is KeccakGoldilocksConfig: Merkle trees and circuit digest hashed with Keccak-256 truncated to 25 bytes
 * (KeccakHash<25>); the Fiat-Shamir challenger, the proof-of-work and the public-input hash stay Poseidon.  A 25-byte digest
 * is carried everywhere as four field elements holding bytes 0-6, 7-13, 14-20 and 21-24, so proof size
 * and layout do not depend on the hasher; a proof whose hash words leave these ranges is P2_VERIFY_NON_CANONICAL.  Every
 * call that takes a blob or a handle reads the hasher from it. */
enum { P2_HASHER_POSEIDON = 0, P2_HASHER_KECCAK = 1 };
/* standard_recursion_config() (zero_knowledge == 0) or standard_recursion_zk_config() with the given hasher; NULL for an
 * unknown hasher.  (0, P2_HASHER_POSEIDON) is p2_builder_new(). */
p2_builder* p2_builder_new_config(int zero_knowledge, int hasher);
/* The hasher of an existing builder, any time before p2_builder_build (upstream chooses it there: build::<C>()); the gates
 * and targets added so far do not depend on it. */
int p2_builder_set_hasher(p2_builder*, int hasher);
void p2_builder_free(p2_builder*);
p2_target p2_builder_add_virtual_target(p2_builder*);
p2_target p2_builder_constant(p2_builder*, uint64_t c);
p2_target p2_builder_zero(p2_builder*);
p2_target p2_builder_one(p2_builder*);
/* c0*m0*m1 + c1*addend */
p2_target p2_builder_arithmetic(p2_builder*, uint64_t c0, uint64_t c1, p2_target m0, p2_target m1, p2_target addend);
p2_target p2_builder_mul_const_add(p2_builder*, uint64_t c, p2_target x, p2_target y); /* c*x + y */
p2_target p2_builder_add(p2_builder*, p2_target x, p2_target y);
p2_target p2_builder_sub(p2_builder*, p2_target x, p2_target y);
p2_target p2_builder_mul(p2_builder*, p2_target x, p2_target y);
p2_target p2_builder_select(p2_builder*, p2_target b, p2_target x, p2_target y); /* if b {x} else {y} */
p2_target p2_builder_is_equal(p2_builder*, p2_target x, p2_target y);
void p2_builder_connect(p2_builder*, p2_target x, p2_target y);
/* Bits and bytes of a field element (CircuitBuilder::assert_bool, le_sum, split_le, range_check; byte forms for the AES
 * gadgets).  Built from ArithmeticGate ops, the byte lookup and one hint per limb; no BaseSumGate, so gate counts differ
 * from upstream's.  All little-endian.  P2_ERR_INVALID with a message if a width is out of range.
 *   assert_bool      t * t - t = 0
 *   le_sum           1..64 boolean targets -> sum of bits[i] * 2^i.  Unlike upstream's, with exactly 64 bits it also refuses
 *                    the spelling of value + p: the result always denotes the integer the bits spell
 *   split_le         x -> num_bits (1..64) boolean targets, with le_sum(bits) == x enforced; no witness if x >= 2^num_bits
 *   range_check      x < 2^num_bits, num_bits 1..63
 *   le_bytes_sum     1..8 range-checked byte targets -> sum of bytes[i] * 256^i; canonical with 8 bytes, as le_sum
 *   split_bytes_le   x -> num_bytes (1..8) byte targets, each looked up in byte table u8_table_idx (p2_aes_sbox_lut) as
 *                    p2_aes_add_virtual_byte_target does
 *   is_less_than     *out = (x < y) for x, y < 2^num_bits, num_bits 1..62; both operands are range-checked */
int p2_builder_assert_bool(p2_builder*, p2_target t);
int p2_builder_le_sum(p2_builder*, const p2_target* bits, size_t n, p2_target* out);
int p2_builder_split_le(p2_builder*, p2_target x, size_t num_bits, p2_target* bits);
int p2_builder_range_check(p2_builder*, p2_target x, size_t num_bits);
int p2_builder_le_bytes_sum(p2_builder*, const p2_target* bytes, size_t n, p2_target* out);
int p2_builder_split_bytes_le(p2_builder*, p2_target x, size_t num_bytes, size_t u8_table_idx, p2_target* bytes);
int p2_builder_is_less_than(p2_builder*, p2_target x, p2_target y, size_t num_bits, p2_target* out);
/* CircuitBuilder::register_public_input: the target's value becomes public input number (calls so far); duplicates allowed.
 * build() hashes the public inputs in the circuit (hash_n_to_hash_no_pad) into the PublicInputGate, and every proof of the
 * circuit ends with the trailer u64 k || k x u64 value.  A circuit with none is built exactly as before.  P2_ERR_INVALID
 * for a target the builder never handed out. */
int p2_builder_register_public_input(p2_builder*, p2_target t);
/* pairs = n_pairs * (input u16, output u16); returns the LUT index (an identical table is re-used);
 * an empty table (n_pairs = 0) is refused: (size_t)-1, p2_last_error set */
size_t p2_builder_add_lookup_table_from_pairs(p2_builder*, const uint16_t* pairs, size_t n_pairs);
/* returns the looked-up output target; (size_t)-1 lut index is an error -> returns UINT64_MAX */
p2_target p2_builder_add_lookup_from_index(p2_builder*, p2_target looking_in, size_t lut_index);
size_t p2_builder_num_gates(const p2_builder*);
/* Compile the circuit.  On success *blob points to a library-owned buffer (release with p2_blob_free). */
int p2_builder_build(p2_builder*, uint8_t** blob, size_t* blob_len);
void p2_blob_free(uint8_t* blob);

/* ------------------------------------------------------------------ AES / GCM gadgets (host) */
size_t p2_aes_sbox_lut(p2_builder*);
size_t p2_aes_byte_xor_lut(p2_builder*);
size_t p2_aes_gf_2_8_mul_lut(p2_builder*);
size_t p2_gcm_u8_unit_right_shift_lut(p2_builder*);
size_t p2_gcm_u8_bitref_lut(p2_builder*);
/* Carry-less byte products in GCM's bit order (a byte B stands for the polynomial rev8(B), the bit-reversed byte): with
 * c = clmul(rev8(a), rev8(b)), (a << 8) + b -> rev8(c & 0xff) and -> rev8(c >> 8).  65 536 entries each; not in the reference. */
size_t p2_gcm_clmul_lo_lut(p2_builder*);
size_t p2_gcm_clmul_hi_lut(p2_builder*);
p2_target p2_aes_add_virtual_byte_target(p2_builder*, size_t u8_table_idx);
p2_target p2_aes_add_virtual_byte_target_unsafe(p2_builder*);
/* States are 16 targets, element [4*i + j] = row i, column j (StateTarget.0[i][j]). */
void p2_aes_state_sub_bytes(p2_builder*, size_t sbox_lut, const p2_target* s, p2_target* out);
void p2_aes_state_mix_columns(p2_builder*, size_t xor_lut, size_t mul_lut, const p2_target* s, p2_target* out);
p2_target p2_aes_gf_2_8_mul(p2_builder*, size_t mul_lut, p2_target x, p2_target y);
p2_target p2_aes_gf_2_8_add(p2_builder*, size_t xor_lut, p2_target x, p2_target y);
/* key: 4*nk bytes targets; out: 4*(nr+1) words * 4 targets, word-major */
void p2_aes_key_expansion(p2_builder*, int nk, int nr, size_t xor_lut, size_t sbox_lut, const p2_target* key, p2_target* out);
void p2_aes_encrypt_block(p2_builder*, int nr, size_t xor_lut, size_t mul_lut, size_t sbox_lut, const p2_target* state,
                          const p2_target* expanded_key, p2_target* out_state);
void p2_gcm_gctr(p2_builder*, int nr, size_t xor_lut, size_t mul_lut, size_t sbox_lut, const p2_target* expanded_key,
                 const p2_target* icb, const p2_target* x, size_t len, p2_target* y);
void p2_gcm_right_shift_one(p2_builder*, size_t shift_lut, const p2_target* v, p2_target* out);
void p2_gcm_inc32(p2_builder*, const p2_target* block, p2_target* out);
void p2_gcm_gf_2_128_mul(p2_builder*, size_t xor_lut, size_t shift_lut, size_t bitref_lut, const p2_target* x,
                         const p2_target* y, p2_target* out);
int p2_gcm_ghash(p2_builder*, size_t xor_lut, size_t shift_lut, size_t bitref_lut, const p2_target* h, const p2_target* x,
                 size_t len, p2_target* out);
/* The same two functions from the carry-less multiply tables (csrc/aes_gadgets.h; not the reference's circuit, only its
 * function): 16 x 16 table products per multiplication, summed by byte position in balanced XOR trees and folded with
 * x^128 = 1 + x + x^2 + x^7 -- 800 arithmetic ops and 1072 lookups per GHASH block instead of 10 880 and 4 480.  Every input
 * byte must be a range-checked byte target (a lookup output, p2_aes_add_virtual_byte_target, a byte constant).  lanes, 1 to 16:
 * blocks taken per reduction, y <- (y ^ x_1) h^k ^ x_2 h^(k-1) ^ .. ^ x_k h; 1 is the plain chain. */
int p2_gcm_gf_2_128_mul_tables(p2_builder*, size_t xor_lut, size_t clmul_lo_lut, size_t clmul_hi_lut, const p2_target* x,
                               const p2_target* y, p2_target* out);
int p2_gcm_ghash_tables(p2_builder*, size_t xor_lut, size_t clmul_lo_lut, size_t clmul_hi_lut, const p2_target* h,
                        const p2_target* x, size_t len, p2_target* out, int lanes);
/* lanes = 0 (the default): p2_aes_gcm_build with a tag builds the reference's bit-serial GHASH.  1 to 16: it builds
 * p2_gcm_ghash_tables with that many lanes, and the two clmul tables instead of the shift and bit tables.  Anything else is an
 * error.  The switch is a property of the builder, not of the blob: the circuit is gates either way. */
int p2_builder_set_ghash_tables(p2_builder*, int lanes);
/* AesGcmTarget<NK,4,NR,L,TAG>::build.  Outputs: key[4*nk], nonce[12], pt[L], ct[L], tag[16]. */
int p2_aes_gcm_build(p2_builder*, int nk, int nr, size_t L, int with_tag, p2_target* key, p2_target* nonce, p2_target* pt,
                     p2_target* ct, p2_target* tag);
/* The same with aad_len range-checked byte targets of additional authenticated data (not in the reference, whose a = []), out in
 * aad[aad_len] (NULL allowed for 0): hashed in front of the ciphertext, aad || 0^v || ct || 0^u || [8 aad_len]_64 || [8 L]_64.
 * They are created after the tag targets, so aad_len = 0 is p2_aes_gcm_build target for target.  aad_len > 0 needs with_tag. */
int p2_aes_gcm_build_aad(p2_builder*, int nk, int nr, size_t L, int with_tag, size_t aad_len, p2_target* key, p2_target* nonce,
                         p2_target* pt, p2_target* ct, p2_target* tag, p2_target* aad);

/* ------------------------------------------------------------------ Poseidon hashing / poseidon-cipher (host) */
/* builder.hash_n_to_m_no_pad::<PoseidonHash>(inputs, m)  (poseidon-cipher/src/circuit.rs:123): PoseidonGate rows */
int p2_builder_hash_n_to_m_no_pad(p2_builder*, const p2_target* inputs, size_t n, p2_target* outputs, size_t m);
/* Merkle membership in a circuit (plonky2 hash/merkle_proofs.rs verify_merkle_proof_to_cap; gadgets/hash.rs permute_swapped;
 * hash/hash_types.rs add_virtual_hash / add_virtual_cap / connect_hashes; hashing.rs hash_or_noop).  A hash is four targets,
 * a cap of height h is 2^h hashes = 4 * 2^h targets.  Poseidon by construction, whatever the circuit's tree hasher.
 *   permute_swapped   one PoseidonGate row: the permutation of inputs[4..8] | inputs[0..4] | inputs[8..12] where swap = 1, of
 *                     `inputs` where swap = 0.  The gate itself constrains swap (swap - 1) = 0.  hash_n_to_m_no_pad's rows are
 *                     this with swap = zero(), gate for gate what they were
 *   hash_or_noop      n <= 4 targets: themselves, zero-padded; more: hash_n_to_m_no_pad(inputs, 4)
 *   verify_merkle_proof_to_cap   leaf[leaf_len] is the leaf at index sum index_bits[i] 2^i of a tree with this cap:
 *                     state = hash_or_noop(leaf), then per sibling state = permute_swapped(state | sibling | 0^4, bit)[0..4], then
 *                     state = cap[the remaining cap_height bits].  n_bits must be n_siblings + cap_height (P2_ERR_INVALID otherwise).
 *                     The path bits are made boolean by the gate; the cap-index bits select through a mux tree of `select`
 *                     ((2^cap_height - 1) * 4 of them, where upstream uses a RandomAccessGate) and are made boolean here with
 *                     assert_bool.  Gate counts differ from upstream's by construction
 *   verify_merkle_proof   the same against a root (cap_height 0) */
int p2_builder_permute_swapped(p2_builder*, const p2_target inputs[12], p2_target swap, p2_target out[12]);
int p2_builder_hash_or_noop(p2_builder*, const p2_target* inputs, size_t n, p2_target out[4]);
int p2_builder_add_virtual_hash(p2_builder*, p2_target out[4]);
int p2_builder_add_virtual_cap(p2_builder*, int cap_height, p2_target* out); /* 0 <= cap_height <= 16 */
int p2_builder_connect_hashes(p2_builder*, const p2_target x[4], const p2_target y[4]);
int p2_builder_verify_merkle_proof_to_cap(p2_builder*, const p2_target* leaf, size_t leaf_len, const p2_target* index_bits, size_t n_bits,
                                          const p2_target* cap, int cap_height, const p2_target* siblings, size_t n_siblings);
int p2_builder_verify_merkle_proof(p2_builder*, const p2_target* leaf, size_t leaf_len, const p2_target* index_bits, size_t n_bits,
                                   const p2_target root[4], const p2_target* siblings, size_t n_siblings);
/* A leaf update as a state transition (not upstream's): the tree with cap old_cap holds old_leaf at the index, and new_cap
 * (4 * 2^cap_height targets, out) is the cap of the same tree with new_leaf there.  No new gate, witness op or kernel: the old walk
 * is verify_merkle_proof_to_cap (cap-index bits made boolean with assert_bool), the new walk climbs from hash_or_noop(new_leaf)
 * over the SAME siblings and index bits (one more PoseidonGate row per level), and new_cap[i] = select(i == cap index, new root,
 * old_cap[i]) with indicators from a demux tree over the cap-index bits: 2 (2^h - 1) + 8 * 2^h more arithmetic ops for cap
 * height h >= 1, none for a root.  Both leaves have leaf_len targets; the other lengths follow verify_merkle_proof_to_cap's rule
 * (P2_ERR_INVALID otherwise, with nothing added).  The siblings a witness sets are item j's of p2_merkle_tree_update's trace.
 *   merkle_update   the same from root to root */
int p2_builder_merkle_update_to_cap(p2_builder*, const p2_target* old_leaf, const p2_target* new_leaf, size_t leaf_len, const p2_target* index_bits,
                                    size_t n_bits, const p2_target* old_cap, int cap_height, const p2_target* siblings, size_t n_siblings, p2_target* new_cap);
int p2_builder_merkle_update(p2_builder*, const p2_target* old_leaf, const p2_target* new_leaf, size_t leaf_len, const p2_target* index_bits, size_t n_bits,
                             const p2_target old_root[4], const p2_target* siblings, size_t n_siblings, p2_target new_root[4]);
/* Native Poseidon Merkle trees on the host (MerkleTree::new(leaves, cap_height).cap, tree.prove(i), verify_merkle_proof_to_cap):
 * the twin of the p2_merkle_tree_* calls below, for hosts without a device.  leaves: [num_leaves][leaf_len] canonical words,
 * row-major; the shape rules are p2_merkle_tree_new's.  cap: 4 * 2^cap_height words; siblings: 4 * (log2(num_leaves) -
 * cap_height) words, the lowest level first.  _cap and _prove build the whole tree on every call.  _verify: *status <- 0
 * accepted, 1 rejected, 2 a leaf, sibling or cap word that is not below p; cap_height 0 to 16, depth + cap_height at most 32. */
int p2_native_merkle_cap(const uint64_t* leaves, size_t num_leaves, size_t leaf_len, int cap_height, uint64_t* cap);
int p2_native_merkle_prove(const uint64_t* leaves, size_t num_leaves, size_t leaf_len, int cap_height, size_t index, uint64_t* siblings);
int p2_native_merkle_verify(const uint64_t* leaf, size_t leaf_len, size_t index, const uint64_t* siblings, size_t depth, const uint64_t* cap,
                            int cap_height, int* status);
/* MerkleTree.update_batch on the host, and the DEFINITION of an update: the k writes leaves[indices[j]] <- new_leaves[j] one after
 * the other, item j on the tree left by the items before it (duplicate indices are legal, the last write wins).  `leaves` is
 * the whole set as p2_native_merkle_cap takes it and is updated in place; the tree is rebuilt from it on every call.  With
 * siblings != NULL item j records [depth][4] words, the path siblings of indices[j] BEFORE its write (p2_native_merkle_prove at that
 * moment), with root_after != NULL four words, cap entry indices[j] >> depth right AFTER it: cap j + 1 is cap j with that one
 * entry replaced.  All or nothing: an index >= num_leaves or a word >= p is P2_ERR_INVALID, names the entry and changes
 * nothing.  k = 0 is a no-op. */
int p2_native_merkle_update(uint64_t* leaves, size_t num_leaves, size_t leaf_len, int cap_height, const uint64_t* indices, const uint64_t* new_leaves,
                            size_t k, uint64_t* siblings, uint64_t* root_after);
/* Sparse keyed Merkle trees: MerkleMap(key_bits = D, value_len = V, cap_height = h), 1 <= D <= 64, 0 <= h <= min(D, 16),
 * 0 <= V <= 134.  This project's own scheme: pod2's tree is not in the reference tree, so it is UNPINNED against pod2.
 *   entries   (key, value[V]): key a u64 below 2^D and below p, value words canonical, keys distinct.
 *   shape     the complete binary tree of depth D; the entry with key k sits at leaf k.
 *   leaves    occupied: hash_or_noop(value | [1]) -- the padded words themselves for V <= 3, (1,0,0,0) for a set (V = 0), hashed
 *             for V >= 4.  Empty: E_0 = (0,0,0,0); no occupied leaf equals it but by a Poseidon collision with zero.
 *   nodes     two_to_one(left, right); an empty subtree of height l is E_l = two_to_one(E_{l-1}, E_{l-1}).
 *   cap       the 2^h nodes of level D - h in index order, dense; an empty map's is 2^h copies of E_{D-h}.
 *   proof     (present, value, siblings[D - h][4]) for key k: siblings[l] is node (k >> l) ^ 1 of level l.  Membership: the walk
 *             from the leaf digest with the bits of k as swap bits reaches cap entry k >> (D - h).  Non-membership: the same walk
 *             from (0,0,0,0).  The position binds the key, so the key is not hashed into the leaf.
 * A map is immutable: a changed set is a new map.
 * Gadgets (no new gate, witness op or kernel).  key_bits: the D little-endian bits of the key, as split_le gives them; n_bits =
 * n_siblings + cap_height or P2_ERR_INVALID with nothing added, as for verify_merkle_proof_to_cap.
 *   lookup   assert_bool(present); start = select(present, hash_or_noop(value | one), 0^4) word by word; then the walk and cap mux
 *            of verify_merkle_proof_to_cap.  One statement serves either answer, so `present` can be a public output.  With
 *            present = 0 the value targets are UNCONSTRAINED.
 *   update   the old walk from (old_present, old_value), the new walk from (new_present, new_value) over the same siblings and
 *            bits, new_cap (4 * 2^cap_height targets, out) from merkle_update_to_cap's demux tree.
 *   insert, remove   update with the flags fixed at (0, 1) and (1, 0): no select and no assert_bool for them, the empty side
 *            starts from zero() targets.
 * Cost: a leaf digest is no row for V <= 3, ceil((V + 1) / 8) PoseidonGate rows above.  lookup: one digest, one row per level,
 * at most 9 ops and the h + 8 (2^h - 1) ops of the cap mux.  update: two digests, two rows per level, at most 18 ops, the mux and the demux's
 * 2 (2^h - 1) - 1 + 8 * 2^h ops (h >= 1).  insert / remove: one digest, two rows per level, mux and demux only.
 * The forms without _to_cap are cap_height 0: root to root. */
int p2_builder_merkle_map_lookup_to_cap(p2_builder*, const p2_target* key_bits, size_t n_bits, const p2_target* value, size_t value_len, p2_target present,
                                        const p2_target* cap, int cap_height, const p2_target* siblings, size_t n_siblings);
int p2_builder_merkle_map_lookup(p2_builder*, const p2_target* key_bits, size_t n_bits, const p2_target* value, size_t value_len, p2_target present,
                                 const p2_target root[4], const p2_target* siblings, size_t n_siblings);
int p2_builder_merkle_map_update_to_cap(p2_builder*, const p2_target* key_bits, size_t n_bits, p2_target old_present, const p2_target* old_value,
                                        p2_target new_present, const p2_target* new_value, size_t value_len, const p2_target* old_cap, int cap_height,
                                        const p2_target* siblings, size_t n_siblings, p2_target* new_cap);
int p2_builder_merkle_map_update(p2_builder*, const p2_target* key_bits, size_t n_bits, p2_target old_present, const p2_target* old_value, p2_target new_present,
                                 const p2_target* new_value, size_t value_len, const p2_target old_root[4], const p2_target* siblings, size_t n_siblings,
                                 p2_target new_root[4]);
int p2_builder_merkle_map_insert_to_cap(p2_builder*, const p2_target* key_bits, size_t n_bits, const p2_target* value, size_t value_len, const p2_target* old_cap,
                                        int cap_height, const p2_target* siblings, size_t n_siblings, p2_target* new_cap);
int p2_builder_merkle_map_insert(p2_builder*, const p2_target* key_bits, size_t n_bits, const p2_target* value, size_t value_len, const p2_target old_root[4],
                                 const p2_target* siblings, size_t n_siblings, p2_target new_root[4]);
int p2_builder_merkle_map_remove_to_cap(p2_builder*, const p2_target* key_bits, size_t n_bits, const p2_target* value, size_t value_len, const p2_target* old_cap,
                                        int cap_height, const p2_target* siblings, size_t n_siblings, p2_target* new_cap);
int p2_builder_merkle_map_remove(p2_builder*, const p2_target* key_bits, size_t n_bits, const p2_target* value, size_t value_len, const p2_target old_root[4],
                                 const p2_target* siblings, size_t n_siblings, p2_target new_root[4]);
/* The map on the host: the definition in code, and the twin of the p2_merkle_map_* calls below.  keys [n], values [n][value_len];
 * it works on the sorted entries and never materialises 2^D nodes; every call builds what it needs again.  A duplicate key, a key
 * not below 2^key_bits and p, a value word not below p, or D, h, V out of range: P2_ERR_INVALID naming the entry, nothing built.
 * _get: *present, value[value_len] (zeros when absent) and siblings[D - h][4] for `key`.  _verify: *status <- 0 the walk reaches
 * its cap entry, 1 it does not, 2 the item is malformed (key out of range, a word not below p, present other than 0 or 1). */
int p2_native_merkle_map_cap(const uint64_t* keys, const uint64_t* values, size_t n, size_t value_len, int key_bits, int cap_height, uint64_t* cap);
int p2_native_merkle_map_get(const uint64_t* keys, const uint64_t* values, size_t n, size_t value_len, int key_bits, int cap_height, uint64_t key, int* present,
                             uint64_t* value, uint64_t* siblings);
int p2_native_merkle_map_verify(uint64_t key, int key_bits, uint64_t present, const uint64_t* value, size_t value_len, const uint64_t* siblings,
                                const uint64_t* cap, int cap_height, int* status);
/* PoseidonEncryptTarget::<L>::build (poseidon-cipher/src/circuit.rs:49).  ks: 10 targets (x then u), m: 5*L,
 * nonce: 2, ct: 5*(L+1) */
int p2_poseidon_cipher_build(p2_builder*, size_t L, p2_target* ks, p2_target* m, p2_target* nonce, p2_target* ct);
/* The cipher on targets the caller supplies, so that the key can come out of another gadget: ks = multiply_point(sk_bits, R),
 * connect(public_key(sk_bits), pk), m = poseidon_decrypt(ks, nonce, ct) states "this ciphertext decrypts, under the secret key of
 * this public key, to that message".  L a multiple of 3 (P2_ERR_INVALID otherwise); m: 5*L targets, ct: 5*(L+1), the last five
 * the tag.  No new gate.
 *   poseidon_encrypt  the loop of PoseidonEncryptTarget::build (circuit.rs:66-86); p2_poseidon_cipher_build is built on it
 *   poseidon_decrypt  per block hash_state, m = ct - s[1..3], s[1..3] = ct; then the closing hash_state and connect(tag, s[1]) word
 *                     by word: a wrong tag is an unsatisfiable witness
 * Not constrained: ks on the curve. */
int p2_builder_poseidon_encrypt(p2_builder*, const p2_target ks[10], const p2_target nonce[2], const p2_target* m, size_t L, p2_target* ct);
int p2_builder_poseidon_decrypt(p2_builder*, const p2_target ks[10], const p2_target nonce[2], const p2_target* ct, size_t L, p2_target* m);
/* native hash / cipher (poseidon-cipher/src/lib.rs:41,75,113).  msg: 5*n_msg words; ct: 5*(ceil3(n_msg)+1) words.  decrypt: n_ct
 * is 3 k + 1 and l <= n_ct - 1 (P2_ERR_INVALID otherwise; the reference panics); P2_ERR_VERIFY where the reference's asserts fail */
void p2_native_hash_n_to_m_no_pad(const uint64_t* in, size_t n, uint64_t* out, size_t m);
void p2_native_poseidon_encrypt(const uint64_t* ks10, const uint64_t* msg, size_t n_msg, const uint64_t* nonce2, uint64_t* ct);
int p2_native_poseidon_decrypt(const uint64_t* ks10, const uint64_t* ct, size_t n_ct, const uint64_t* nonce2, size_t l, uint64_t* msg);

/* ------------------------------------------------------------------ ecGFp5 / ElGamal (host) */
/* The curve is pod2's (not in the reference tree; see csrc/ecgfp5.h).  A point is its affine (x, u) coordinates, ten
 * words, x then u -- pod2 `Point::as_fields` (hashed_elgamal.rs:23); a scalar is five little-endian 64-bit limbs. */
#define P2_POINT_WORDS 10
#define P2_SCALAR_LIMBS 5
#define P2_SCALAR_BITS 320
void p2_ecgfp5_group_order(uint64_t out[5]);                     /* GROUP_ORDER (lib.rs:12) */
void p2_ecgfp5_generator(uint64_t out[10]);                      /* Point::generator() */
void p2_ecgfp5_mul(const uint64_t k[5], const uint64_t p[10], uint64_t out[10]); /* &k * P */
void p2_ecgfp5_add(const uint64_t p[10], const uint64_t q[10], uint64_t out[10]);
void p2_ecgfp5_neg(const uint64_t p[10], uint64_t out[10]);      /* Point::inverse (elgamal.rs:21) */
int p2_ecgfp5_is_in_subgroup(const uint64_t p[10]);              /* 1 / 0 */
void p2_ecgfp5_compress(const uint64_t p[10], uint64_t w[5]);    /* compress_from_subgroup (lib.rs:82) */
int p2_ecgfp5_decompress(const uint64_t w[5], uint64_t out[10]); /* decompress_into_subgroup (lib.rs:74); P2_ERR_INVALID if none */
/* Randomness comes from the operating system's CSPRNG, as the reference's OsRng (lib.rs:35,64): */
int p2_ecgfp5_random_scalar(uint64_t out[5]);                    /* gen_biguint_below(&GROUP_ORDER) (lib.rs:35) */
int p2_ecgfp5_random_point(uint64_t out[10]);                    /* Point::new_rand_from_subgroup */
/* encode_binary / decode_binary (lib.rs:48, :80): 160 message bits as five 32-bit limbs, random padding above them */
int p2_ecgfp5_encode_binary(const uint32_t limbs[5], uint64_t out[10]);
/* TEST / BENCHMARK ONLY: the same three from a 64-bit seed (SplitMix64, not cryptographic) so that inputs are
 * reproducible.  A scalar drawn this way carries at most 64 bits of entropy: never a real key or nonce. */
void p2_ecgfp5_random_scalar_seeded(uint64_t seed, uint64_t out[5]);
void p2_ecgfp5_random_point_seeded(uint64_t seed, uint64_t out[10]);
void p2_ecgfp5_encode_binary_seeded(const uint32_t limbs[5], uint64_t seed, uint64_t out[10]);
void p2_ecgfp5_decode_binary(const uint64_t p[10], uint32_t limbs[5]);
/* elgamal.rs:11, :19; hashed_elgamal.rs:19, :28.  Scalars must be below the group order (P2_ERR_INVALID otherwise). */
int p2_elgamal_encrypt(const uint64_t pk[10], const uint64_t nonce[5], const uint64_t msg[10], uint64_t c0[10], uint64_t c1[10]);
int p2_elgamal_decrypt(const uint64_t sk[5], const uint64_t c0[10], const uint64_t c1[10], uint64_t msg[10]);
int p2_hashed_elgamal_encrypt(const uint64_t pk[10], const uint64_t nonce[5], const uint64_t msg[5], uint64_t c0[10], uint64_t ct[5]);
int p2_hashed_elgamal_decrypt(const uint64_t sk[5], const uint64_t c0[10], const uint64_t ct[5], uint64_t msg[5]);
/* pod2 CircuitBuilderElliptic / CircuitBuilderBits as the reference calls them (ecgfp5/src/circuit.rs:33-38,
 * elgamal/circuit.rs:34-37,70-72): points are 10 targets, a BigUInt320Target is its 320 little-endian bit targets. */
void p2_builder_add_virtual_point_target(p2_builder*, p2_target out[10]);
void p2_builder_constant_point(p2_builder*, const uint64_t p[10], p2_target out[10]);
void p2_builder_add_virtual_biguint320_target(p2_builder*, p2_target bits[320]);
int p2_builder_multiply_point(p2_builder*, const p2_target bits[320], const p2_target p[10], p2_target out[10]);
void p2_builder_add_point(p2_builder*, const p2_target p[10], const p2_target q[10], p2_target out[10]);
/* EcStepGate (csrc/ecstep_gate.h; not an upstream gate): one row holds one double-and-add step of a scalar multiplication,
 *     mid = 2 acc,  out = mid + bit q,
 * in (X:Z:U:T) coordinates, acc / mid / out = X | Z | U | T (4 x 5 elements), q = x | u (2 x 5).  `bit` is not made boolean.
 *   set_ec_gate  on != 0: multiply_point -- and public_key, elgamal_encrypt, hashed_elgamal_encrypt through it -- emits 320 such
 *                rows instead of arithmetic gates.  Off by default; a builder that leaves it off builds what it always built.
 *   ec_step      one row; hinted != 0 attaches the generator that fills mid and out (witness op ECSTEP), hinted == 0 leaves
 *                them to the caller, who sets the returned targets. */
int p2_builder_set_ec_gate(p2_builder*, int on);
int p2_builder_ec_step(p2_builder*, const p2_target acc[20], const p2_target q[10], p2_target bit, int hinted, p2_target mid[20], p2_target out[20]);
/* CircuitBuilderECGFP5PublicKey::public_key (ecgfp5/src/circuit.rs:35) */
int p2_builder_public_key(p2_builder*, const p2_target sk_bits[320], p2_target pk[10]);
/* CircuitBuilderElGamal::elgamal_encrypt (elgamal/circuit.rs:28) */
int p2_builder_elgamal_encrypt(p2_builder*, const p2_target pk[10], const p2_target nonce_bits[320], const p2_target msg[10],
                               p2_target c0[10], p2_target c1[10]);
/* CircuitBuilderHashedElGamal::hashed_elgamal_encrypt (hashed_elgamal/circuit.rs:33) */
int p2_builder_hashed_elgamal_encrypt(p2_builder*, const p2_target pk[10], const p2_target nonce_bits[320], const p2_target msg[5],
                                      p2_target c0[10], p2_target ct[5]);
/* encode_binary (lib.rs:48) with the random high halves supplied by the caller, hence deterministic: attempt a tries
 * w[i] = limbs[i] + (pad[5 a + i] << 32), an attempt with a word not below p is skipped, the first that decodes gives out and
 * *used.  P2_ERR_INVALID (*used = attempts, out untouched) when none does.  The reference draws r < p - limb and keeps r >> 32;
 * uniform 32-bit halves differ from that by less than 2^-32.  The host twin of p2_ecgfp5_encode_binary_batch. */
int p2_ecgfp5_encode_binary_padded(const uint32_t limbs[5], const uint32_t* pad, size_t attempts, uint64_t out[10], uint32_t* used);
/* Verifiable decryption (not in the reference, whose circuits only encrypt): no new gate.
 *   neg_point               negates the five u targets
 *   elgamal_decrypt         msg = c1 - sk c0: add_point(c1, neg_point(multiply_point(sk_bits, c0)))
 *   hashed_elgamal_decrypt  msg[i] = ct[i] - hash_n_to_m_no_pad(multiply_point(sk_bits, c0), 5)[i]
 * The caller ties the key to a public key with connect(public_key(sk_bits), pk).  Works with set_ec_gate on and off.  NOT checked
 * in the circuit: that c0 and c1 are in the group (add_virtual_point_target checks the curve equation only) and that sk < n. */
int p2_builder_neg_point(p2_builder*, const p2_target p[10], p2_target out[10]);
int p2_builder_elgamal_decrypt(p2_builder*, const p2_target sk_bits[320], const p2_target c0[10], const p2_target c1[10], p2_target msg[10]);
int p2_builder_hashed_elgamal_decrypt(p2_builder*, const p2_target sk_bits[320], const p2_target c0[10], const p2_target ct[5], p2_target msg[5]);

/* ------------------------------------------------------------------ Schnorr signatures on ecGFp5 (host) */
/* The scheme (csrc/schnorr.h; this project's own, UNPINNED against pod2's signature bytes):
 *   keys       sk in [1, n), pk = sk G
 *   challenge  e_words[4] = hash_n_to_hash_no_pad(R.x | R.u | pk.x | pk.u | msg), e = sum e_words[i] 2^(64 i)
 *   sign       R = nonce G for a caller-supplied nonce in [1, n), s = (nonce + e sk) mod n; sig[9] = s (5 limbs) | e_words
 *   verify     status 2 (malformed): s >= n, a word of e_words, msg or pk not below p, pk outside the group, pk neutral;
 *              otherwise R' = s G + e (-pk): status 0 (accepted) iff the challenge of R' is e_words, else 1 (rejected).
 * msg: msg_len canonical field elements, 0 <= msg_len <= 1024 (P2_ERR_INVALID above that).  The return value tells whether the
 * call could run; *status is the scheme's answer.
 *   scalar_muladd  out = (a b + c) mod n for arbitrary 320-bit a, b, c (five little-endian limbs each)
 *   sign           *status 0, or 2 with sig (and pk) zeroed: sk or nonce outside [1, n), a message word not below p.  pk: NULL, or
 *                  receives sk G. */
void p2_ecgfp5_scalar_muladd(const uint64_t a[5], const uint64_t b[5], const uint64_t c[5], uint64_t out[5]);
int p2_schnorr_challenge(const uint64_t r[10], const uint64_t pk[10], const uint64_t* msg, size_t msg_len, uint64_t e[4]);
int p2_schnorr_sign(const uint64_t sk[5], const uint64_t nonce[5], const uint64_t* msg, size_t msg_len, uint64_t sig[9], uint64_t pk[10], int* status);
int p2_schnorr_verify(const uint64_t pk[10], const uint64_t* msg, size_t msg_len, const uint64_t sig[9], int* status);
/* The gadget: no new gate.  add_virtual_schnorr_signature: s as 320 boolean bit targets (add_virtual_biguint320_target) and the
 * four challenge words.  verify_schnorr_signature constrains hash(R' | pk | msg) = e for R' = s G + e (-pk), with e's bits from
 * the canonical 64-bit split_le of every word; r: NULL, or receives the targets of R'.  Works with set_ec_gate on and off; pk is
 * any point target.  NOT checked in the circuit: s < n, and that pk is in the group (add_virtual_point_target checks the curve
 * equation only) -- a circuit that takes pk as a public input relies on p2_schnorr_verify's checks outside. */
int p2_builder_add_virtual_schnorr_signature(p2_builder*, p2_target s_bits[320], p2_target e[4]);
int p2_builder_verify_schnorr_signature(p2_builder*, const p2_target pk[10], const p2_target* msg, size_t msg_len, const p2_target s_bits[320],
                                        const p2_target e[4], p2_target r[10]);

/* ------------------------------------------------------------------ self-test (host) */
/* Checks the host build of the arithmetic the kernels share with it: the carry-chain reduction against 128-bit
 * arithmetic (random and extreme inputs), and the restructured Poseidon (poseidon_fast.h: lazy reduction, sparse partial
 * rounds, accumulator fold) against the plain 30-round permutation.  0 = all agree; otherwise the number of mismatches. */
int p2_selftest_host(uint64_t seed, size_t n_reductions, size_t n_permutations);
/* The same comparison compiled for the device and run there (threads x 64 reductions and threads x 1 permutation,
 * textbook forms as the reference): guards against code-generation regressions such as the add-with-carry fold described
 * in DESIGN.md.  Returns the number of mismatches, or a negative P2_ERR_* code. */
int p2_selftest_device(uint64_t seed, size_t threads, int device);
/* The lazy compositions of the polynomial-side kernels (permutation term and product step, the table-slot and looking-slot steps
 * of the one-walk quotient, exact dot products, the table-power multiply) and the operand contracts of gl.h against the textbook canonical forms, on operands drawn from the extremes
 * (0, 1, 2^32 - 1, 2^32, p - 1, p, p + 1, 2^64 - 1, zero limbs, random) and NOT reduced where a contract allows any u64; with one
 * planted violation per contract that must show.  Returns the number of mismatches, or a negative P2_ERR_* code. */
int p2_selftest_lazy_device(uint64_t seed, size_t threads, int device);
/* The transform arithmetic: gl::mul_nb -- the NTT kernels' multiply, whose two-sided correction no other code uses -- on unreduced
 * extremes, on the operand pairs (2^j, m 2^(96 - j)), j = 33, 36, .., 63, that take the reduction's borrow-only path (even lanes; odd
 * lanes draw at random), the butterfly, and the four register stages of a radix-16 step in both forms, against the textbook
 * operations; with one planted violation that must show.  threads x 16 rounds.  Returns the number of mismatches, or a negative
 * P2_ERR_* code. */
int p2_selftest_ntt_device(uint64_t seed, size_t threads, int device);
/* The host build of the hash kernels' permutation: kind 0 = twelve unknown words, 1 = words 8..11 enter as 0, 2 = words 0..7 enter
 * as 0 (the words declared zero are not read); rows bit r = output word r is kept (canonical), the others are unspecified;
 * parts 0 = the round loops as the kernels run them, 1 = first round, middle and last round as separate functions. */
int p2_host_poseidon_known(uint64_t* states, size_t n_perm, int kind, uint32_t rows, int parts);
/* The host build of the cipher kernels' sponge step (csrc/kernels_pcipher.h): out = hash_state(in) = hash_n_to_m_no_pad(in, 20) on
 * twenty canonical words.  last != 0: the closing form, which computes only out[5..10), the tag; the other words come back as 0. */
int p2_host_pcipher_hash_state(const uint64_t in[20], int last, uint64_t out[20]);
/* The partial-round section of that permutation alone, in place on count x 12 words that may be ANY u64: from "the state carries
 * round 4's constants" to "the state carries round 26's" (some representative of each word, not canonical).  After four full
 * rounds a test cannot steer what reaches the folds of the section; through this entry point, and p2_gpu_partial_rounds, it can. */
int p2_host_partial_rounds(uint64_t* states, size_t count);
/* The section the hash kernels run in its place (glf::merged_middle): round 3's MDS and the 22 partial rounds as one chain, in
 * place on count x 12 words that may be ANY u64: from "round 3's twelve S-box outputs" to "the state carries round 26's constants"
 * (some representative of each word, not canonical).  p2_gpu_merged_middle is the same on the device. */
int p2_host_merged_middle(uint64_t* states, size_t count);
/* EcStepGate's 40 constraints on count rows of 80 canonical wires -> out [count][40]; the _ext form over GF(p^2): wires
 * [count][80][2] (c0, c1) -> out [count][40][2].  The evaluator the verifiers and the quotient-side kernel share. */
int p2_host_ecstep_constraints(const uint64_t* wires, size_t count, uint64_t* out);
int p2_host_ecstep_constraints_ext(const uint64_t* wires, size_t count, uint64_t* out);
/* k_hash_leaves' sponge on the host: data [min(active_cols, cols)][num_leaves] -> digests [num_leaves][4] */
int p2_host_hash_leaves(const uint64_t* data, size_t cols, size_t active_cols, size_t num_leaves, uint64_t* digests);

/* ------------------------------------------------------------------ native cipher (host; witness values) */
uint8_t p2_native_gf_2_8_mul(uint8_t a, uint8_t b);
void p2_native_aes_key_expansion(const uint8_t* key, int nk, int nr, uint8_t* out /* 16*(nr+1) */);
void p2_native_aes_encrypt_block(const uint8_t* key, int nk, int nr, const uint8_t* in16, uint8_t* out16);
void p2_native_gf_2_128_mul(const uint8_t* x16, const uint8_t* y16, uint8_t* out16);
void p2_native_ghash(const uint8_t* h16, const uint8_t* x, size_t len, uint8_t* out16);
void p2_native_gctr(const uint8_t* key, int nk, int nr, const uint8_t* icb16, const uint8_t* x, size_t len, uint8_t* y);
/* with additional authenticated data, which the reference leaves out (its a = []): the tag is over aad || 0^v || ct || 0^u ||
 * [8 aad_len]_64 || [8 len]_64 (SP 800-38D section 7.1); aad_len = 0 is p2_native_aes_gcm_encrypt */
void p2_native_aes_gcm_encrypt_aad(const uint8_t* key, int nk, int nr, const uint8_t* nonce12, const uint8_t* aad, size_t aad_len, const uint8_t* pt,
                                   size_t len, uint8_t* ct, uint8_t* tag16);
/* authenticated decryption: 0 and the plaintext when the tag over (aad, ct) matches in all 16 bytes; 1 and pt zeroed when not */
int p2_native_aes_gcm_decrypt(const uint8_t* key, int nk, int nr, const uint8_t* nonce12, const uint8_t* aad, size_t aad_len, const uint8_t* ct, size_t len,
                              const uint8_t* tag16, uint8_t* pt);
void p2_native_aes_gcm_encrypt(const uint8_t* key, int nk, int nr, const uint8_t* nonce12, const uint8_t* pt, size_t len,
                               uint8_t* ct, uint8_t* tag16);

/* The tree hasher of P2_HASHER_KECCAK on the host (csrc/keccak_hash.h): hash_no_pad of n words, and two_to_one of two digests
 * in the four-word form (each word in its range).  out4 is in the four-word form. */
void p2_native_keccak_hash_no_pad(const uint64_t* in, size_t n, uint64_t out4[4]);
void p2_native_keccak_two_to_one(const uint64_t l4[4], const uint64_t r4[4], uint64_t out4[4]);
/* Keccak-256 (original padding) of a byte string, on the same permutation: the hash in a lookup gate's id. */
void p2_native_keccak256(const uint8_t* data, size_t len, uint8_t out32[32]);

/* ------------------------------------------------------------------ circuit info / verification (host) */
/* Shape of a compiled circuit without touching a device. */
typedef struct {
    uint32_t degree_bits, num_wires, num_routed_wires, num_constants_cols, num_zs_cols, num_quotient_cols, num_luts,
        num_ops, num_levels, num_slots, num_virtual_targets, num_fri_rounds;
    uint64_t proof_bytes; /* exact serialised proof size, public-input trailer included */
    uint32_t zero_knowledge, num_gate_kinds; /* standard_recursion_zk_config(); distinct gate types in the circuit */
    uint32_t num_public_inputs; /* targets registered with p2_builder_register_public_input */
    uint32_t hasher;            /* P2_HASHER_* */
} p2_circuit_info;
int p2_blob_info(const uint8_t* blob, size_t len, p2_circuit_info* out);
/* The device-side schedule of a compiled circuit's witness program for macro size `fuse` (csrc/witness_schedule.h; the prover
 * builds it at p2_circuit_load; P2AES_WITNESS_FUSE = longest chain, 1..8, default 1 = none), computed AND checked on the host:
 * every op is kept, every slot keeps its first producer, and every operand of every op is produced in an earlier level
 * or earlier in the op's own chain.  out = {levels, chains, longest chain, ops fused into chains}.  P2_ERR_INVALID if a
 * check fails. */
int p2_witness_schedule_check(const uint8_t* blob, size_t len, uint32_t fuse, uint32_t out[4]);
/* verifier_data = constants_sigmas_cap (16 digests) || circuit_digest, 68 u64 -- from p2_circuit_verifier_data */
int p2_verify(const uint8_t* blob, size_t blob_len, const uint64_t* verifier_data, size_t verifier_data_len,
              const uint8_t* proof, size_t proof_len);
/* Test hook: the vanishing identity at zeta, the check p2_verify makes after the proof-of-work test, on openings and
 * challenges the caller supplies.  openings: a buffer of the circuit's proof size of which only the opening set is read;
 * challenges: betas[2] gammas[2] deltas[8] alphas[2] zeta[2] (the deltas are ignored without lookup tables); pi_hash: the
 * public-inputs hash (taken as zero for a circuit without public inputs).  No transcript, proof-of-work response, Merkle path
 * or FRI check is involved.  terms <- the flat term list, *n_terms extension elements of two words (cap: room in elements);
 * sides[4 i ..] <- for challenge i the sum of term_k alpha_i^k and Z_H(zeta) t_i(zeta), two words each; *verdict <- P2_VERIFY_OK,
 * P2_VERIFY_VANISHING, or P2_VERIFY_ZETA_IN_SUBGROUP (then *n_terms = 0 and the sides are zero).  P2_ERR_INVALID for a word
 * that is not below p.  tests/vanishing_ref.py restates what it computes. */
int p2_vanishing_terms(const uint8_t* blob, size_t blob_len, const uint8_t* openings, size_t len, const uint64_t challenges[16],
                       const uint64_t pi_hash[4], uint64_t* terms, size_t cap, size_t* n_terms, uint64_t sides[8], int* verdict);
/* Compressed proofs: ProofWithPublicInputs::compress, CompressedProofWithPublicInputs::decompress and
 * CircuitData::verify_compressed, on the host.  Same argument conventions as p2_verify; a compressed proof is never longer
 * than the full one (p2_blob_info's proof_bytes), so cap = proof_bytes always suffices.  *n_written receives the output's
 * length (also when cap is too small: P2_ERR_INVALID).  A proof that cannot be converted is P2_ERR_VERIFY with the reason in
 * p2_last_error: compress checks the full proof's shape and canonicality and takes the query indices from the transcript;
 * decompress checks, in this order, the shape (indices below the LDE size, exact length, sibling counts, public-input count),
 * the canonicality of every word, and that the written indices are the ones the transcript draws.  verify_compressed is
 * verify_proof of the decompressed proof and checks the proof-of-work between canonicality and the indices. */
int p2_proof_compress(const uint8_t* blob, size_t blob_len, const uint64_t* verifier_data, size_t verifier_data_len, const uint8_t* proof,
                      size_t proof_len, uint8_t* out, size_t cap, size_t* n_written);
int p2_proof_decompress(const uint8_t* blob, size_t blob_len, const uint64_t* verifier_data, size_t verifier_data_len, const uint8_t* cproof,
                        size_t cproof_len, uint8_t* out, size_t cap, size_t* n_written);
int p2_verify_compressed(const uint8_t* blob, size_t blob_len, const uint64_t* verifier_data, size_t verifier_data_len,
                         const uint8_t* cproof, size_t cproof_len);
/* ProofWithPublicInputs::public_inputs: the k values of the proof's public-input trailer (k = num_public_inputs of the
 * circuit; *n_written = k, 0 for a circuit without public inputs).  P2_ERR_INVALID if proof_len is not the circuit's
 * proof size, the count word is not k, or cap < k.  Parsing only: p2_verify checks that the values are the proven ones.
 * Parses the whole blob on every call; with a loaded handle, p2_circuit_public_inputs reads the trailer alone. */
int p2_proof_public_inputs(const uint8_t* blob, size_t blob_len, const uint8_t* proof, size_t proof_len, uint64_t* out, size_t cap,
                           size_t* n_written);

/* ------------------------------------------------------------------ GPU prover */
typedef struct p2_circuit p2_circuit;
/* Uploads the compiled circuit to HIP device `device` and commits constants+sigmas there (one-time). */
p2_circuit* p2_circuit_load(const uint8_t* blob, size_t len, int device);
void p2_circuit_free(p2_circuit*);
int p2_circuit_verifier_data(const p2_circuit*, uint64_t* out, size_t cap, size_t* n_written);
/* Proofs per chunk of the workspaces the handle holds now (0 before the first proof): a batch is cut into equal chunks of
 * at most this many proofs, dealt round-robin to the proving streams; the size is the "chunk" option capped by free HBM. */
size_t p2_circuit_chunk_proofs(p2_circuit*);
/* zk circuits only.  Blinding values are the output of a Poseidon-based PRF under a 256-bit key (four field elements)
 * and a per-handle proof counter that advances with every proof attempted.  The key is drawn from the operating system's
 * CSPRNG at load time (upstream: OS randomness per proof) -- that is the production path and needs no call here.
 * TEST ONLY: p2_circuit_set_zk_key fixes the key (words are reduced mod p) and, when the key differs from the one the handle
 * holds, restarts the counter -- which makes proofs reproducible so the CPU oracle can check them byte for byte;
 * p2_circuit_set_zk_seed(s) is set_zk_key({s, 0, 0, 0}).  Both return P2_ERR_INVALID unless the environment holds
 * P2AES_ALLOW_FIXED_ZK_KEY=1 (the test suite sets it).  A fixed key is not secret, and one key on two handles (or set again
 * after proofs were made under another) blinds different witnesses with the same values: never outside tests. */
int p2_circuit_set_zk_key(p2_circuit*, const uint64_t key[4]);
int p2_circuit_set_zk_seed(p2_circuit*, uint64_t seed);
size_t p2_circuit_proof_bytes(const p2_circuit*);
/* Public inputs of a loaded circuit: their number, and p2_proof_public_inputs on the handle -- it reads only the proof's
 * trailer (O(k)), so it is the form to call once per proof of a batch. */
size_t p2_circuit_num_public_inputs(const p2_circuit*);
int p2_circuit_public_inputs(const p2_circuit*, const uint8_t* proof, size_t proof_len, uint64_t* out, size_t cap, size_t* n_written);
/* One PartialWitness: (target, value) pairs, values canonical (< p). */
typedef struct {
    const p2_target* targets;
    const uint64_t* values;
    size_t count;
} p2_assignment;
/* Proves `batch` independent witnesses of one circuit.  proofs: batch * p2_circuit_proof_bytes() bytes.
 * status[i] receives a P2_PROOF_* code; a failed proof leaves its slot zeroed (a value >= p fails its witness with
 * P2_PROOF_WITNESS_CONFLICT, like a conflicting set_target).  The call returns after the proofs are in host memory.
 * Inputs and proofs travel through persistent pinned staging buffers owned by the handle.
 * Thread safety: `prove(&self)` in the reference takes a shared reference, and so does this: any number of host threads
 * may call p2_prove_batch / p2_prove_batch_device concurrently on the SAME handle (enqueueing is serialised inside; each
 * caller gets its own staging set) as well as on different handles. */
int p2_prove_batch(p2_circuit*, size_t batch, const p2_assignment* inputs, uint8_t* proofs, int* status);
/* The same call sharded over several handles of ONE compiled circuit, normally one handle per HIP device of the node
 * (p2_circuit_load(blob, len, d) for d = 0..N-1): witness i goes to the handle that owns its contiguous, balanced range of
 * the batch (the partition of SURVEY.md 8e: independent proofs, no data crosses devices), one host thread per handle.
 * proofs / status are indexed like the inputs.  P2_ERR_INVALID if the handles are not loads of the same circuit. */
int p2_prove_batch_multi(p2_circuit* const* handles, size_t n_handles, size_t batch, const p2_assignment* inputs,
                         uint8_t* proofs, int* status);
/* Same pipeline with inputs already resident on the device and proofs left on the device:
 * d_values: [batch][n_targets] u64 (device pointer), targets shared by the whole batch (host pointer); the value
 * 2^64-1 (not a field element) marks "this witness does not assign the target".
 * d_proofs: device buffer of batch * proof_bytes; d_status: device int[batch].  Asynchronous: kernels are enqueued on
 * the circuit's own streams.  `stream` (a hipStream_t passed as void*, NULL = the default stream) orders the call with
 * the caller: the proving streams wait for the work already enqueued on it and it then waits for the proofs, so work
 * the caller enqueues on `stream` afterwards sees them.  d_values must stay untouched until then.  Host code calls
 * p2_circuit_synchronize() (or synchronises `stream`) before reading the outputs. */
int p2_prove_batch_device(p2_circuit*, size_t batch, const p2_target* targets, size_t n_targets, const uint64_t* d_values,
                          uint8_t* d_proofs, int* d_status, void* stream);
int p2_circuit_synchronize(p2_circuit*);

/* ------------------------------------------------------------------ witness outputs, dry runs, fault diagnosis */
/* What the circuit computed (upstream: generate_partial_witness, then witness.get_target).  `connect` merges targets into
 * slots and a slot takes its first producer, so a computed target that the assignment leaves out is simply computed: set the
 * inputs, name the targets to read.  (Trap: an AesGcmTarget built with TAG = false still has its 16 range-checked tag targets,
 * which nothing computes: set them, to zero, or the witness is P2_PROOF_MISSING_INPUT.)
 * On input P2_VALUE_UNSET means "this witness does not assign the target" (device forms); on output it means "the witness run
 * did not determine this target" (its generator never ran, or lost a lookup).
 * Out-target lists follow the rules of input target lists: shared by the batch, host pointers, virtual targets and routed
 * wires in the encoding p2_prove_batch_device accepts, duplicates allowed, n_out == 0 legal; a target without a slot in this
 * circuit is P2_ERR_INVALID ("output target is not a target of this circuit"), checked before anything is enqueued. */
#define P2_VALUE_UNSET UINT64_MAX
/* p2_prove_batch(_device) with read-back: d_out / out_values [batch][n_out] come from the witness run the proof is made from
 * and are written for every proof whatever its status; proofs and statuses are exactly those of p2_prove_batch(_device), which
 * are these calls with n_out = 0.  Host form: a witness rejected on the host (a value >= p, one target assigned two values)
 * never runs as given, and all its outputs are P2_VALUE_UNSET. */
int p2_prove_batch_outputs_device(p2_circuit*, size_t batch, const p2_target* targets, size_t n_targets, const uint64_t* d_values,
                                  const p2_target* out_targets, size_t n_out, uint64_t* d_out, uint8_t* d_proofs, int* d_status, void* stream);
int p2_prove_batch_outputs(p2_circuit*, size_t batch, const p2_assignment* inputs, const p2_target* out_targets, size_t n_out,
                           uint64_t* out_values, uint8_t* proofs, int* status);
/* Witness generation only: no proof is made and the zk proof counter does not advance.  status[i] is 0, 1 or 2 and equals
 * what p2_prove_batch reports for that witness whenever that is 0, 1 or 2.  A failed witness still gets its outputs: a value
 * >= p or a conflicting entry of the assignment is skipped and the run goes on (after two conflicting entries of one slot the
 * slot holds one of the two values).  Device form: the kernels run on `stream` (NULL = the default stream) behind the work
 * already enqueued there, so p2_witness_batch_device -> (copy d_out into the prover's d_values) -> p2_prove_batch_device on one
 * stream needs no host synchronisation; asynchronous, synchronise `stream` before reading.  Thread safety as p2_verify_batch:
 * own workspaces (option "witness_chunk" witnesses each), never waits for the proving streams. */
int p2_witness_batch_device(p2_circuit*, size_t batch, const p2_target* targets, size_t n_targets, const uint64_t* d_values,
                            const p2_target* out_targets, size_t n_out, uint64_t* d_out, int* d_status, void* stream);
int p2_witness_batch(p2_circuit*, size_t batch, const p2_assignment* inputs, const p2_target* out_targets, size_t n_out,
                     uint64_t* out_values, int* status);
/* Why one witness failed.  The run is followed by a data-parallel check of the final slot values (csrc/witness_check.h; exact
 * after the fact because a slot never changes once set).  One fault is reported, the first of:
 *   INPUT_NOT_CANONICAL  an entry whose value is >= p: the lowest index; found = the value
 *   INPUT_CONFLICT       two entries of one slot with different values: the lowest index of a later entry; found = its value,
 *                        computed = the earlier entry's
 *   LOOKUP_MISS / GENERATOR_CONFLICT   the generator with the lowest index in the blob's op order: its operands are set and
 *                        its input is not in its table (found = the input), or its recomputed output (computed) differs from what
 *                        the slot holds (found); input_index = the entry that set that slot, if one did
 *   NOT_SET              a slot no generator produces, that a generator or a routed wire needs, and that is unset: the lowest target
 * kind == P2_FAULT_NONE iff *status == 0, kinds 1-4 iff *status == 1, kind 5 iff *status == 2. */
typedef struct {
    int32_t kind;        /* P2_FAULT_* */
    int32_t op_kind;     /* generator kind (csrc/circuit.h OP_*: 0 ARITH .. 5 POSEIDON, 7 ECSTEP, 6 LIMB = a bit or byte hint of split_le /
                          * split_bytes_le) at fault, -1 if none */
    int64_t input_index; /* entry of the assignment involved, -1 if none */
    p2_target target;    /* a target of the slot at fault: its lowest virtual target, else its lowest routed wire; UINT64_MAX if none */
    uint32_t gate_row;   /* a row holding a routed wire of that slot (the PoseidonGate row for OP_POSEIDON), UINT32_MAX if none */
    uint64_t computed, found;
} p2_witness_fault;
enum {
    P2_FAULT_NONE = 0,
    P2_FAULT_INPUT_NOT_CANONICAL = 1,
    P2_FAULT_INPUT_CONFLICT = 2,
    P2_FAULT_LOOKUP_MISS = 3,
    P2_FAULT_GENERATOR_CONFLICT = 4,
    P2_FAULT_NOT_SET = 5
};
/* out: a p2_witness_fault*, passed as void* like the streams -- the foreign-function declarations generated from this header
 * (tools/gen_rust_ffi.py) carry scalar and handle types only. */
int p2_witness_explain(p2_circuit*, const p2_assignment* input, int* status, void* out);
/* The host twin of the three calls above for one witness, from the blob (no device; like p2_host_hash_leaves it exists for the
 * CPU test suite and the prover never calls it): a sequential interpreter of the scheduled op program and the check function the
 * device kernels use.  fault: a p2_witness_fault* as above, or NULL. */
int p2_host_witness(const uint8_t* blob, size_t len, const p2_assignment* input, const p2_target* out_targets, size_t n_out,
                    uint64_t* out_values, int* status, void* fault);

/* Batched verification on the GPU: the verdict of verify_proof for each proof, as a P2_VERIFY_* code.
 * proofs: batch * p2_circuit_proof_bytes() bytes (the fixed layout of DESIGN.md section 8; every Merkle path has the depth the
 * circuit implies, so a sibling-count byte that differs is P2_VERIFY_SHAPE -- also where the host reader, misled by two count
 * bytes whose errors cancel, would first meet a non-canonical word).  verifier_data: 4*2^cap_height + 4 u64
 * (cap || circuit_digest, host memory) or NULL for the handle's own (vd_len is then ignored).  status[i] <- P2_VERIFY_*.
 * Returns P2_OK when every verdict was produced (rejections are verdicts, not errors), P2_ERR_INVALID / _NO_DEVICE / _HIP
 * otherwise; batch == 0 is a no-op.  A zeroed slot (a proof p2_prove_batch failed) is P2_VERIFY_SHAPE.  Large batches run in
 * chunks (option "verify_chunk", default: ~256 MiB of workspace, at most 512 proofs).  Thread safety as p2_prove_batch: any
 * number of host threads may prove and verify on one handle; verification has its own workspaces and never waits for the
 * proving streams. */
int p2_verify_batch(p2_circuit*, size_t batch, const uint8_t* proofs, const uint64_t* verifier_data, size_t vd_len, int* status);
/* Same with proofs and statuses in device memory, ordered with `stream` (NULL = the default stream) like
 * p2_prove_batch_device: the kernels run on `stream` behind the work already enqueued there, so prove_batch_device ->
 * verify_batch_device on one stream needs no host round trip.  Asynchronous: synchronise `stream` before reading d_status. */
int p2_verify_batch_device(p2_circuit*, size_t batch, const uint8_t* d_proofs, const uint64_t* verifier_data, size_t vd_len,
                           int* d_status, void* stream);
/* Test hook: p2_vanishing_terms' verdict from the device verifier.  buffers [batch][proof size], challenges [batch][16] and
 * pi_hashes [batch][4] as p2_vanishing_terms takes them, all in host memory.  Per chunk it unpacks the buffers, puts the
 * caller's challenges and hashes where the transcript kernel would, and launches the vanishing kernel verify_batch launches
 * for the circuit; flags[i] <- 8 if zeta is in the subgroup (the kernel goes on and may add 16), 16 if the identity fails, 0 if
 * it holds.  Workspaces, chunks and thread safety are p2_verify_batch's. */
int p2_gpu_vanishing_flags(p2_circuit*, size_t batch, const uint8_t* buffers, const uint64_t* challenges, const uint64_t* pi_hashes,
                           uint32_t* flags);
/* Compressed proofs in GPU batches (the conversions of p2_proof_compress / p2_proof_decompress / p2_verify_compressed; layout
 * and verdict order in DESIGN.md section 8).  Compressed proofs sit at a stride of p2_circuit_proof_bytes() (a compressed
 * proof is never longer than the full one) with lengths[i] their actual lengths; the bytes of a slot past its length are
 * zero in compress's output and ignored on input.  status[i] <- P2_VERIFY_*: compress gives OK, SHAPE or NON_CANONICAL (the
 * full proof's shape and canonicality) and a zeroed slot of length 0 for a proof it rejects; decompress gives OK, SHAPE (the
 * compressed shape, or written indices that differ from the drawn ones) or NON_CANONICAL and a zeroed slot for a proof it
 * rejects; verify_compressed gives the verdict of p2_verify_compressed.  A zeroed slot or a zero length is SHAPE.  A length
 * above the stride is P2_ERR_INVALID in the host forms and a SHAPE verdict in the device forms.  verifier_data as
 * p2_verify_batch.  The workspaces, chunks and thread safety are p2_verify_batch's. */
int p2_compress_batch(p2_circuit*, size_t batch, const uint8_t* proofs, const uint64_t* verifier_data, size_t vd_len, uint8_t* out,
                      uint32_t* lengths, int* status);
int p2_decompress_batch(p2_circuit*, size_t batch, const uint8_t* cproofs, const uint32_t* lengths, const uint64_t* verifier_data,
                        size_t vd_len, uint8_t* out, int* status);
int p2_verify_compressed_batch(p2_circuit*, size_t batch, const uint8_t* cproofs, const uint32_t* lengths, const uint64_t* verifier_data,
                               size_t vd_len, int* status);
/* The same with every buffer but verifier_data in device memory, ordered with `stream` like p2_verify_batch_device:
 * prove_batch_device -> compress_batch_device -> verify_compressed_batch_device on one stream needs no host round trip. */
int p2_compress_batch_device(p2_circuit*, size_t batch, const uint8_t* d_proofs, const uint64_t* verifier_data, size_t vd_len,
                             uint8_t* d_out, uint32_t* d_lengths, int* d_status, void* stream);
int p2_decompress_batch_device(p2_circuit*, size_t batch, const uint8_t* d_cproofs, const uint32_t* d_lengths,
                               const uint64_t* verifier_data, size_t vd_len, uint8_t* d_out, int* d_status, void* stream);
int p2_verify_compressed_batch_device(p2_circuit*, size_t batch, const uint8_t* d_cproofs, const uint32_t* d_lengths,
                                      const uint64_t* verifier_data, size_t vd_len, int* d_status, void* stream);
/* Tuning knobs of a handle: "chunk" (proofs per workspace, default 128), "streams" (proving streams, default 2),
 * "debug_timing" (host-path phase times on stderr), "verify_chunk" (proofs per p2_verify_batch chunk), "witness_chunk"
 * (witnesses per chunk of the witness-only calls, default 256: one workgroup per compute unit; capped so that a workspace fits
 * in 80 % of the free HBM).  The environment variables P2AES_CHUNK / P2AES_STREAMS / P2AES_DEBUG_TIMING / P2AES_VERIFY_CHUNK /
 * P2AES_WITNESS_CHUNK set the defaults and are read once, in p2_circuit_load. */
int p2_circuit_set_option(p2_circuit*, const char* name, long value);
/* Per-kernel timing of the most recent batch (HIP events on the proving stream). */
typedef struct {
    char name[48];
    float ms;       /* total over launches */
    uint32_t count; /* launches */
} p2_kernel_time;
int p2_circuit_set_timing(p2_circuit*, int enable);
size_t p2_circuit_get_timing(p2_circuit*, p2_kernel_time* out, size_t cap);

/* ------------------------------------------------------------------ Merkle trees on the GPU (independent of any circuit) */
/* MerkleTree::new(leaves, cap_height) with PoseidonHash: commits a set.  leaves: [num_leaves][leaf_len] canonical words,
 * row-major (a Vec<Vec<F>> of equal lengths); num_leaves a power of two >= 1, 0 <= cap_height <= log2(num_leaves), leaf_len >= 1.
 * A leaf of at most four words is its own digest, zero-padded (hash_or_noop); a longer one is hash_no_pad of it.  Anything
 * else is P2_ERR_INVALID with a message: a bad shape, a null pointer, a word >= p (host form; the device form takes the words
 * as canonical), a tree that does not fit in the free device memory.  *tree <- the handle, passed as void* like the streams
 * (see p2_witness_explain); it holds every digest level on the device, 64 * num_leaves bytes, and not the leaves (while it
 * is being built also a column-major copy of them).  num_leaves at most 2^32, leaf_len at most 2^20.
 * _new returns with the tree built.  _new_device reads d_leaves (a device pointer) in kernels enqueued on `stream` (NULL = the
 * default stream) behind the work already there and returns at once: d_leaves must stay untouched until they have run; every
 * later call on the handle orders itself behind them.  Only caps and paths are interface, not the digests' order in memory. */
int p2_merkle_tree_new(const uint64_t* leaves, size_t num_leaves, size_t leaf_len, int cap_height, int device, void** tree);
int p2_merkle_tree_new_device(const uint64_t* d_leaves, size_t num_leaves, size_t leaf_len, int cap_height, int device, void* stream,
                              void** tree);
void p2_merkle_tree_free(void* tree);
/* tree.cap: 4 * 2^cap_height words to host memory (cap_words: room in words); waits for the build */
int p2_merkle_tree_cap(void* tree, uint64_t* cap, size_t cap_words);
/* tree.prove(i) for n indices: siblings [n][log2(num_leaves) - cap_height][4], the lowest level first.  Host form: an index
 * >= num_leaves is P2_ERR_INVALID and nothing is written.  Device form: path i goes to d_out[i * out_stride_words ..], so a
 * caller can write paths straight into the [batch][n_targets] matrix of p2_prove_batch_device (d_out = the matrix plus the
 * column of the first sibling target, out_stride_words = n_targets); the words between paths are left alone.  d_status[i] <- 0,
 * or 1 for an index >= num_leaves, whose row is left untouched.  Asynchronous on `stream`, like p2_prove_batch_device. */
int p2_merkle_tree_prove_batch(void* tree, const uint64_t* indices, size_t n, uint64_t* siblings);
int p2_merkle_tree_prove_batch_device(void* tree, const uint64_t* d_indices, size_t n, uint64_t* d_out, size_t out_stride_words, int* d_status,
                                      void* stream);
/* tree.update: k ordered writes, leaf indices[j] <- leaves[j] ([k][leaf_len] words), with p2_native_merkle_update's semantics word
 * for word; the shape of the tree does not change.  The trace (siblings [k][depth][4] as the path of indices[j] was before item j,
 * root_after [k][4], cap entry indices[j] >> depth right after it) costs k * depth hashes, all of one level independent of each
 * other; without it every changed node is hashed once.  All or nothing.  Host form: the trace is on iff siblings or root_after is
 * non-null; a bad item is P2_ERR_INVALID, names the entry and is found on the host before anything is enqueued; returns with
 * the update applied.  Device form: the trace is on iff d_siblings is non-null; item j's siblings go to d_siblings[j *
 * sib_stride_words ..] and its root to d_root_after[j * root_stride_words ..] (may be NULL) with the strides of
 * p2_merkle_tree_prove_batch_device, so a trace lands in the [batch][n_targets] matrix of p2_prove_batch_device; d_status[j] <- 0, 1
 * (the index names no leaf; looked at first) or 2 (a word not below p), and where any is not 0 the tree and the trace buffers stay
 * as they were -- a device flag turns the later kernels of the call into no-ops, the host does not synchronise.  Asynchronous on
 * `stream`, behind the build and earlier updates; later _cap, _prove* and _update* calls order themselves behind it.  k < 2^32;
 * k = 0 is a no-op.  Temporaries live in a block on the handle that only grows (growing it waits for the last update).
 * Concurrent calls on ONE handle from several host threads are not supported.
 * _last_update_hashes: the two_to_one calls of the last update (0 before the first), counted on the device; waits for it. */
int p2_merkle_tree_update(void* tree, const uint64_t* indices, const uint64_t* leaves, size_t k, uint64_t* siblings, uint64_t* root_after);
int p2_merkle_tree_update_device(void* tree, const uint64_t* d_indices, const uint64_t* d_leaves, size_t k, uint64_t* d_siblings, size_t sib_stride_words,
                                 uint64_t* d_root_after, size_t root_stride_words, int* d_status, void* stream);
int p2_merkle_tree_last_update_hashes(void* tree, uint64_t* hashes);
/* verify_merkle_proof_to_cap for n paths against one cap: leaves [n][leaf_len], indices [n], siblings [n][depth][4], cap
 * 4 * 2^cap_height words.  status[i] <- 0 accepted, 1 rejected (also an index that names no leaf), 2 a leaf, sibling or cap word
 * that is not below p -- what p2_native_merkle_verify gives path for path.  cap_height 0 to 16, depth + cap_height at most 32.
 * Device form: every buffer in device memory, asynchronous on `stream`. */
int p2_merkle_verify_batch(const uint64_t* leaves, size_t leaf_len, const uint64_t* indices, const uint64_t* siblings, size_t depth,
                           const uint64_t* cap, int cap_height, size_t n, int* status, int device);
int p2_merkle_verify_batch_device(const uint64_t* d_leaves, size_t leaf_len, const uint64_t* d_indices, const uint64_t* d_siblings, size_t depth,
                                  const uint64_t* d_cap, int cap_height, size_t n, int* d_status, int device, void* stream);
/* Benchmark hook (tools/gpu_merkle_bench.py): one tree build on buffers the caller owns.  d_dig: 8 * num_leaves words (the
 * digest levels); with_transpose == 0: the column-major build of p2_gpu_merkle_cap on d_scratch [leaf_len][num_leaves];
 * otherwise the transpose kernel from the row-major d_leaves into d_scratch in front of it, the build of p2_merkle_tree_new.
 * Asynchronous on `stream`. */
int p2_gpu_merkle_build_device(const uint64_t* d_leaves, size_t num_leaves, size_t leaf_len, int cap_height, int with_transpose,
                               uint64_t* d_scratch, uint64_t* d_dig, int device, void* stream);
/* MerkleMap on the GPU (the definition is with p2_native_merkle_map_* above): built once, immutable.  keys [n], values
 * [n][value_len], fewer than 2^32 entries in any order.  The build validates the entries, sorts them, hashes every non-empty node
 * exactly once (p2_merkle_map_hashes: the nodes above the leaves) and keeps, per level, the ascending ids of the non-empty nodes
 * and their digests.  A bad entry is found on the device in both forms: P2_ERR_INVALID naming the first one (the lowest entry
 * index; its key before its words before a duplicate), no handle.  Too little device memory is refused with a message.
 * _new_device: the entries in device memory, read by kernels on `stream`; the call synchronises that stream once (for the level
 * sizes and the bad-entry flag) and returns with the rest of the build enqueued; the buffers may be reused when it returns.
 * Every later call on the handle waits on one event recorded behind the build, on whatever stream it runs.
 * _get_batch: present[n] (0 / 1), values [n][value_len] (zeros when absent), siblings [n][D - h][4]; a key out of range is
 * P2_ERR_INVALID naming it.  _get_batch_device: row j at d_out + j * out_stride_words words, with presence (one word), the value
 * and the siblings at the given word offsets within the row, so proofs land in the [batch][n_targets] matrix of
 * p2_prove_batch_device; d_status[j] <- 0, or 2 for a key out of range, whose row is left untouched.  Asynchronous on `stream`.
 * _verify_batch: n proofs against one cap, keys [n], present [n] words, values [n][value_len], siblings [n][D - h][4]; status[i] as
 * p2_native_merkle_map_verify gives it, proof for proof.  (p2_merkle_verify_batch's 32 index bits are unchanged.) */
int p2_merkle_map_new(const uint64_t* keys, const uint64_t* values, size_t n, size_t value_len, int key_bits, int cap_height, int device, void** map);
int p2_merkle_map_new_device(const uint64_t* d_keys, const uint64_t* d_values, size_t n, size_t value_len, int key_bits, int cap_height, int device, void* stream,
                             void** map);
void p2_merkle_map_free(void* map);
int p2_merkle_map_cap(void* map, uint64_t* cap, size_t cap_words);
int p2_merkle_map_len(void* map, size_t* n);
int p2_merkle_map_hashes(void* map, uint64_t* hashes);
int p2_merkle_map_get_batch(void* map, const uint64_t* keys, size_t n, uint64_t* present, uint64_t* values, uint64_t* siblings);
int p2_merkle_map_get_batch_device(void* map, const uint64_t* d_keys, size_t n, uint64_t* d_out, size_t out_stride_words, size_t present_off, size_t value_off,
                                   size_t siblings_off, int* d_status, void* stream);
int p2_merkle_map_verify_batch(const uint64_t* keys, int key_bits, const uint64_t* present, const uint64_t* values, size_t value_len, const uint64_t* siblings,
                               const uint64_t* cap, int cap_height, size_t n, int* status, int device);
int p2_merkle_map_verify_batch_device(const uint64_t* d_keys, int key_bits, const uint64_t* d_present, const uint64_t* d_values, size_t value_len,
                                      const uint64_t* d_siblings, const uint64_t* d_cap, int cap_height, size_t n, int* d_status, int device, void* stream);

/* ------------------------------------------------------------------ native ecGFp5 and Schnorr signatures in GPU batches */
/* One thread per item (csrc/kernels_schnorr.h); rows are contiguous: scalars [count][5], points [count][10], messages
 * [count][msg_len] (one msg_len per call, at most 1024), signatures [count][9]; status int[count].  The host-pointer forms copy
 * in and out and return when done; the _device forms take raw device pointers and are asynchronous on `stream` (NULL: the
 * default stream).  Secret keys and nonces given to p2_schnorr_sign_batch_device live in device memory the caller owns;
 * zeroising it is the caller's business.
 *   mul_batch     out[i] = k[i] P[i] for any 320-bit k[i]; status 2 (row zeroed) for a P[i] with a word not below p or outside
 *                 the group, else 0 -- p2_ecgfp5_mul item for item
 *   sign_batch    p2_schnorr_sign item for item; pk: NULL, or receives the public keys
 *   verify_batch  p2_schnorr_verify item for item */
int p2_ecgfp5_mul_batch(const uint64_t* k, const uint64_t* p, size_t count, uint64_t* out, int* status, int device);
int p2_ecgfp5_mul_batch_device(const uint64_t* d_k, const uint64_t* d_p, size_t count, uint64_t* d_out, int* d_status, int device, void* stream);
int p2_schnorr_sign_batch(const uint64_t* sk, const uint64_t* nonce, const uint64_t* msg, size_t msg_len, size_t count, uint64_t* sig, uint64_t* pk,
                          int* status, int device);
int p2_schnorr_sign_batch_device(const uint64_t* d_sk, const uint64_t* d_nonce, const uint64_t* d_msg, size_t msg_len, size_t count, uint64_t* d_sig,
                                 uint64_t* d_pk, int* d_status, int device, void* stream);
int p2_schnorr_verify_batch(const uint64_t* pk, const uint64_t* msg, size_t msg_len, const uint64_t* sig, size_t count, int* status, int device);
int p2_schnorr_verify_batch_device(const uint64_t* d_pk, const uint64_t* d_msg, size_t msg_len, const uint64_t* d_sig, size_t count, int* d_status,
                                   int device, void* stream);
/* test entry: out[i] = (a[i] b[i] + c[i]) mod n on the device, one thread per triple */
int p2_gpu_ecgfp5_scalar_muladd(const uint64_t* a, const uint64_t* b, const uint64_t* c, size_t count, uint64_t* out, int device);

/* ------------------------------------------------------------------ ElGamal on ecGFp5 in GPU batches */
/* One thread per item (csrc/kernels_elgamal.h), the call shape of the section above: contiguous rows, every array per item (a
 * caller with one key repeats it), host-pointer forms that copy in and out, _device forms that take raw device pointers and are
 * asynchronous on `stream`.  Compressed points and hashed messages are [count][5] words.  status[i]:
 *   0  done
 *   1  no result: the row is zeroed (decompress: w[i] encodes no group element; encode_binary: no attempt decodes)
 *   2  malformed, every output row of the item zeroed: a word not below p, a scalar not below n, a point outside the group (the
 *      neutral is inside)
 * Outputs are the host's word for word (p2_ecgfp5_decompress, p2_ecgfp5_encode_binary_padded, p2_elgamal_*, p2_hashed_elgamal_*).
 *   decompress_batch      out[i] = decompress_into_subgroup(w[i])
 *   encode_binary_batch   limbs uint32 [count][5], pad uint32 [count][attempts][5], 1 <= attempts <= 256; used[i]: the number of
 *                         the attempt taken, `attempts` with status 1
 *   elgamal_encrypt       c0[i] = nonce[i] G, c1[i] = msg[i] + nonce[i] pk[i]
 *   elgamal_decrypt       msg[i] = c1[i] - sk[i] c0[i]
 *   hashed_elgamal_*      the same with the message five field elements under hash_n_to_m_no_pad(as_fields(nonce pk), 5)
 *   scalar_bits_device    d_out[i stride + j] = bit j of d_k[i], j < 320 <= stride (words): a scalar's row segment of the prover's
 *                         value matrix.  Secret keys and nonces stay in device memory the caller owns. */
int p2_ecgfp5_decompress_batch(const uint64_t* w, size_t count, uint64_t* out, int* status, int device);
int p2_ecgfp5_decompress_batch_device(const uint64_t* d_w, size_t count, uint64_t* d_out, int* d_status, int device, void* stream);
int p2_ecgfp5_encode_binary_batch(const uint32_t* limbs, const uint32_t* pad, size_t attempts, size_t count, uint64_t* out, uint32_t* used, int* status,
                                  int device);
int p2_ecgfp5_encode_binary_batch_device(const uint32_t* d_limbs, const uint32_t* d_pad, size_t attempts, size_t count, uint64_t* d_out, uint32_t* d_used,
                                         int* d_status, int device, void* stream);
int p2_elgamal_encrypt_batch(const uint64_t* pk, const uint64_t* nonce, const uint64_t* msg, size_t count, uint64_t* c0, uint64_t* c1, int* status,
                             int device);
int p2_elgamal_encrypt_batch_device(const uint64_t* d_pk, const uint64_t* d_nonce, const uint64_t* d_msg, size_t count, uint64_t* d_c0, uint64_t* d_c1,
                                    int* d_status, int device, void* stream);
int p2_elgamal_decrypt_batch(const uint64_t* sk, const uint64_t* c0, const uint64_t* c1, size_t count, uint64_t* msg, int* status, int device);
int p2_elgamal_decrypt_batch_device(const uint64_t* d_sk, const uint64_t* d_c0, const uint64_t* d_c1, size_t count, uint64_t* d_msg, int* d_status,
                                    int device, void* stream);
int p2_hashed_elgamal_encrypt_batch(const uint64_t* pk, const uint64_t* nonce, const uint64_t* msg, size_t count, uint64_t* c0, uint64_t* ct, int* status,
                                    int device);
int p2_hashed_elgamal_encrypt_batch_device(const uint64_t* d_pk, const uint64_t* d_nonce, const uint64_t* d_msg, size_t count, uint64_t* d_c0,
                                           uint64_t* d_ct, int* d_status, int device, void* stream);
int p2_hashed_elgamal_decrypt_batch(const uint64_t* sk, const uint64_t* c0, const uint64_t* ct, size_t count, uint64_t* msg, int* status, int device);
int p2_hashed_elgamal_decrypt_batch_device(const uint64_t* d_sk, const uint64_t* d_c0, const uint64_t* d_ct, size_t count, uint64_t* d_msg,
                                           int* d_status, int device, void* stream);
int p2_ecgfp5_scalar_bits_device(const uint64_t* d_k, size_t count, uint64_t* d_out, size_t stride, int device, void* stream);

/* ------------------------------------------------------------------ Poseidon cipher in GPU batches */
/* One thread per message (csrc/kernels_pcipher.h), the call shape of the sections above.  l, the number of Fq elements of a message,
 * is one value per call, 0 <= l <= 3072 (P2_ERR_INVALID beyond, before any launch).  Rows: ks [count][10] (x then u of the shared
 * point, used as words only: no group test, as the host twin), nonce [count][2], msg [count][l][5], ct [count][pad3(l)+1][5] with
 * pad3(l) = l rounded up to a multiple of 3.  status[i]:
 *   0  done
 *   1  decrypt only, the row zeroed: the tag does not match, or a padding element is not zero where the reference asserts it (l > 3)
 *   2  the row zeroed: a word of ks, nonce, msg or ct not below p
 * Outputs are p2_native_poseidon_encrypt's and _decrypt's word for word. */
int p2_poseidon_encrypt_batch(const uint64_t* ks, const uint64_t* nonce, const uint64_t* msg, size_t l, size_t count, uint64_t* ct, int* status, int device);
int p2_poseidon_encrypt_batch_device(const uint64_t* d_ks, const uint64_t* d_nonce, const uint64_t* d_msg, size_t l, size_t count, uint64_t* d_ct, int* d_status,
                                     int device, void* stream);
int p2_poseidon_decrypt_batch(const uint64_t* ks, const uint64_t* nonce, const uint64_t* ct, size_t l, size_t count, uint64_t* msg, int* status, int device);
int p2_poseidon_decrypt_batch_device(const uint64_t* d_ks, const uint64_t* d_nonce, const uint64_t* d_ct, size_t l, size_t count, uint64_t* d_msg, int* d_status,
                                     int device, void* stream);

/* ------------------------------------------------------------------ AES-GCM in GPU batches */
/* Encryption and authenticated decryption with additional authenticated data (SP 800-38D; 96-bit nonces, 16-byte tags), the call
 * shape of the sections above (csrc/kernels_gcm.h).  Rows are bytes and contiguous per item: key
 * [count][4 nk], nonce [count][12], aad [count][aad_len], pt and ct [count][len], tag [count][16]; nk, len and aad_len are one value
 * per call, and a caller with one key repeats it.  The _device forms take `row_stride` >= len, the distance in bytes between pt
 * rows and between ct rows (the host forms pass len): with both bases and the stride multiples of 16 whole blocks move as 128
 * bits, otherwise byte by byte.  They also take d_work, 16-byte aligned device memory of p2_aes_gcm_batch_workspace bytes that
 * the call uses as scratch (round keys, H and its multiplier table per item); the host forms allocate it.  Limits: nk 4, 6 or 8,
 * len <= 2^24, aad_len <= 2^16, row_stride >= len; anything else is P2_ERR_INVALID before any launch.  status[i]:
 *   0  done
 *   1  decrypt only, the pt row zeroed: the tag does not match
 * There is no malformed status: every byte string is a valid input.  Outputs are p2_native_aes_gcm_encrypt_aad's and
 * p2_native_aes_gcm_decrypt's byte for byte.
 *   bytes_to_words_device  d_out[i stride_words + j] = d_bytes[i byte_stride + j], j < row_bytes <= stride_words: a byte row as
 *                          the ByteTarget segment of a row of the prover's value matrix, so keys, plaintexts and computed
 *                          ciphertexts and tags go from device memory into p2_prove_batch_device without a host round trip */
size_t p2_aes_gcm_batch_workspace(int nk, size_t len, size_t aad_len, size_t count); /* bytes of d_work; 0 for an nk that is refused */
int p2_aes_gcm_encrypt_batch(const uint8_t* key, int nk, const uint8_t* nonce, const uint8_t* aad, size_t aad_len, const uint8_t* pt, size_t len, size_t count,
                             uint8_t* ct, uint8_t* tag, int* status, int device);
int p2_aes_gcm_decrypt_batch(const uint8_t* key, int nk, const uint8_t* nonce, const uint8_t* aad, size_t aad_len, const uint8_t* ct, const uint8_t* tag,
                             size_t len, size_t count, uint8_t* pt, int* status, int device);
int p2_aes_gcm_encrypt_batch_device(const uint8_t* d_key, int nk, const uint8_t* d_nonce, const uint8_t* d_aad, size_t aad_len, const uint8_t* d_pt, size_t len,
                                    size_t row_stride, size_t count, uint8_t* d_ct, uint8_t* d_tag, int* d_status, void* d_work, int device, void* stream);
int p2_aes_gcm_decrypt_batch_device(const uint8_t* d_key, int nk, const uint8_t* d_nonce, const uint8_t* d_aad, size_t aad_len, const uint8_t* d_ct,
                                    const uint8_t* d_tag, size_t len, size_t row_stride, size_t count, uint8_t* d_pt, int* d_status, void* d_work,
                                    int device, void* stream);
int p2_bytes_to_words_device(const uint8_t* d_bytes, size_t row_bytes, size_t byte_stride, size_t count, uint64_t* d_out, size_t stride_words, int device,
                             void* stream);
/* test entries (tests/test_gpu_gcm.py): the GHASH kernel alone with lanes = 1 (one thread per item) or 64 (one wave per item),
 * h [count][16], x [count][16 blocks] -> out [count][16] = p2_native_ghash(h[i], x[i]); the block cipher alone, in and out
 * [count][16], out[i] = p2_native_aes_encrypt_block(key[i], in[i]) */
int p2_gpu_gcm_ghash(const uint8_t* h, const uint8_t* x, size_t blocks, size_t count, int lanes, uint8_t* out, int device);
int p2_gpu_aes_encrypt_blocks(const uint8_t* key, int nk, const uint8_t* in, size_t count, uint8_t* out, int device);
/* bench entry (tools/gpu_gcm_bench.py): encryptions of `count` items on device buffers that the call fills with random bytes
 * (rows 16 ceil(len / 16) bytes apart, 128-bit path), one warm-up and then `repeats` runs with an event between the kernels:
 * ns[3 r + 0 .. 2] = k_gcm_setup, k_gcm_ctr, k_gcm_ghash of run r in nanoseconds.  lanes 1 or 64 forces that GHASH kernel, 0 is
 * the public calls' choice. */
int p2_gpu_gcm_kernel_times(int nk, size_t len, size_t aad_len, size_t count, int lanes, size_t repeats, uint64_t* ns, int device);

/* ------------------------------------------------------------------ GPU primitives (parity tests / microbench) */
int p2_gpu_device_count(void);
/* data: n_perm * 12 u64 on host; permuted in place on the device */
int p2_gpu_poseidon(uint64_t* states, size_t n_perm, int device);
/* columns: [cols][n] coefficients (host) -> lde [cols][n<<rate_bits], bit-reversed index order (host) */
int p2_gpu_lde(const uint64_t* coeffs, size_t cols, int degree_bits, int rate_bits, uint64_t* lde, int device);
/* values [cols][n] -> coefficients [cols][n]; degree_bits 1..22 (above 14: two-pass transform) */
int p2_gpu_intt(const uint64_t* values, size_t cols, int degree_bits, uint64_t* coeffs, int device);
/* The LDE of FRI round `round` as the prover's commit phase runs it, on the tables of a circuit of 2^degree_bits rows whose FRI
 * schedule is arities[0..n_rounds): n_r = n >> (arities[0] + .. + arities[round - 1]) coefficients per column, coset shift
 * g^(2^(arities[0] + ..)).  coeffs: batch x in_batch_stride words, [cols][n_r] at the start of each; out: batch x out_batch_stride
 * words, [cols][8 n_r] in bit-reversed order written at the start of each, the words between left as they came in.  round = 0 (any
 * n_rounds) is the main LDE; otherwise round < n_rounds. */
int p2_gpu_lde_round(const uint64_t* coeffs, size_t cols, int degree_bits, const uint32_t* arities, size_t n_rounds, size_t round, size_t batch,
                     size_t in_batch_stride, uint64_t* out, size_t out_batch_stride, int device);
/* The prover's quotient inverse: qvals [batch][chunks][8 n], the values of `chunks` polynomials of degree < 8 n on the LDE coset in
 * bit-reversed order -> out [batch][chunks * 8][n], their coefficients, n per row.  degree_bits 2..22. */
int p2_gpu_quotient_chunks(const uint64_t* qvals, size_t chunks, int degree_bits, size_t batch, uint64_t* out, int device);
/* column-major leaves [cols][num_leaves] -> cap digests (2^cap_height * 4 u64) */
int p2_gpu_merkle_cap(const uint64_t* cols_major, size_t cols, size_t num_leaves, int cap_height, uint64_t* cap, int device);
/* the same with the tree hasher chosen (P2_HASHER_*); Keccak needs cols >= 4 (every leaf is hashed, there is no no-op case) */
int p2_gpu_merkle_cap_hasher(const uint64_t* cols_major, size_t cols, size_t num_leaves, int cap_height, int hasher, uint64_t* cap, int device);
/* the tree kernels on their own, one launch each (tests/test_gpu_sponge.py):
 * data [batch][min(active_cols, cols)][num_leaves], columns >= active_cols are zero and not stored -> digests [batch][num_leaves][4] */
int p2_gpu_hash_leaves(const uint64_t* data, size_t cols, size_t active_cols, size_t num_leaves, size_t batch, uint64_t* digests, int device);
/* p2_host_partial_rounds on the device: one thread per state, at the hash kernels' occupancy (tests/test_gpu_partial_rounds.py) */
int p2_gpu_partial_rounds(uint64_t* states, size_t count, int device);
/* p2_host_merged_middle on the device, the same way (tests/test_gpu_merged_middle.py) */
int p2_gpu_merged_middle(uint64_t* states, size_t count, int device);
/* p2_host_ecstep_constraints on the device: the base-field instantiation, one row per thread (tests/test_gpu_ecstep.py) */
int p2_gpu_ecstep_constraints(const uint64_t* wires, size_t count, uint64_t* out, int device);
/* child [batch][2 * num_parents][4] -> parent [batch][num_parents][4] */
int p2_gpu_merkle_level(const uint64_t* child, size_t num_parents, size_t batch, uint64_t* parent, int device);
/* vals [batch][2][len] -> digests [batch][len / arity][4] */
int p2_gpu_hash_fri_leaves(const uint64_t* vals, size_t len, int arity, size_t batch, uint64_t* digests, int device);
/* the opening-point power tables on their own (tests/test_gpu_side_kernels.py): z = (c0, c1) canonical, n a power of two up to 2^22
 * -> pows [4][2][n]: point k = 0: z, 1: g z, 2: 1 / z, 3: 1 / (g z), g the primitive n-th root of unity; row [k][0] holds c0 */
int p2_gpu_zeta_pows(const uint64_t* z, size_t n, uint64_t* pows, int device);
/* debug: copy a named intermediate buffer of proof `index` of the last batch to the host
 * ("wires", "wires_cap", "zs", "zs_cap", "quotient_coeffs", "quotient_cap", "challenges", "openings",
 * "public_inputs_hash", ...) */
int p2_circuit_debug_read(p2_circuit*, const char* name, size_t index, uint64_t* out, size_t cap, size_t* n_written);
/* debug: how many device allocations, pinned host allocations, streams and events the library holds right now, over all
 * handles, trees and running calls of the process; a handle or tree that is freed takes all of its own with it */
size_t p2_debug_live_resources(void);

#ifdef __cplusplus
}
#endif
#endif
