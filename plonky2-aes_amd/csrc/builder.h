// Host-side mirror of the slice of plonky2's CircuitBuilder API that the reference's gadget crates call
// (SURVEY.md Appendix A.1): add_virtual_target, constant/zero/one, arithmetic (mul_const_add, add, mul, sub,
// mul_sub), select, is_equal, connect, add_lookup_table_from_pairs, add_lookup_from_index, num_gates, build.
// Same names, argument meaning and constant-folding / op-caching / slot-packing behaviour as upstream, so the
// gate rows a gadget produces here are the rows it produces there.  Gate TYPES follow upstream's GateRef identity: every
// lookup table has its own LookupGate and LookupTableGate type (their id() carries the table's Keccak hash), which decides
// the number of selector polynomials; sigma sends each routed wire to the next wire of its copy class in (row, column)
// order, as `wire_partition` / `get_sigma_map` do.  oracle/oracle_builder.py derives all of this a second time,
// independently, and tests/test_independent_builder.py compares.
//
// Call sites mirrored: aes-gcm/src/circuit_aes.rs:176-358, aes-gcm/src/circuit_gcm.rs:49-425.
#pragma once
#include <algorithm>
#include <array>
#include <map>
#include <memory>
#include <unordered_map>

#include "circuit.h"
#include "gl.h"
#include "keccak_hash.h"

namespace p2 {

// Target: virtual target (index) or routed wire (row, column).  plonky2 iop::target::Target.
typedef u64 Target;
static const u64 T_WIRE_BIT = 1ull << 63;
static inline Target wire_target(u32 row, u32 col) { return T_WIRE_BIT | ((u64)row << 8) | col; }
static inline bool is_wire(Target t) { return (t & T_WIRE_BIT) != 0; }
static inline u32 wire_row(Target t) { return (u32)((t & ~T_WIRE_BIT) >> 8); }
static inline u32 wire_col(Target t) { return (u32)(t & 0xFF); }

struct BoolTarget {
    Target target;
};

struct GateInstance {
    u32 kind;
    u64 constants[2];
};

class CircuitBuilder {
   public:
    explicit CircuitBuilder(const Config& cfg = Config()) : cfg_(cfg) {}
    void set_hasher(u32 hasher) { cfg_.hasher = hasher; }  // the tree hasher is a property of build::<C>(), not of the gates

    // ---- targets ------------------------------------------------------------------------------------
    Target add_virtual_target() { return (Target)num_virtual_++; }
    BoolTarget add_virtual_bool_target_unsafe() { return BoolTarget{add_virtual_target()}; }

    Target constant(u64 c) {
        c %= gl::P;
        auto it = constants_to_targets_.find(c);
        if (it != constants_to_targets_.end()) return it->second;
        Target t = add_virtual_target();
        constants_to_targets_[c] = t;
        targets_to_constants_[t] = c;
        return t;
    }
    Target zero() { return constant(0); }
    Target one() { return constant(1); }
    Target neg_one() { return constant(gl::P - 1); }

    bool target_as_constant(Target t, u64* out) const {
        auto it = targets_to_constants_.find(t);
        if (it == targets_to_constants_.end()) return false;
        *out = it->second;
        return true;
    }

    void connect(Target x, Target y) { copy_constraints_.push_back({x, y}); }

    // plonky2 CircuitBuilder::register_public_input: the proof carries the target's value, in registration order
    void register_public_input(Target t) {
        const bool known = is_wire(t) ? (wire_row(t) < gate_instances_.size() && wire_col(t) < cfg_.num_routed_wires) : t < num_virtual_;
        if (!known) throw std::runtime_error("register_public_input: no such target (or a wire that is not routed)");
        public_inputs_.push_back(t);
    }
    size_t num_public_inputs() const { return public_inputs_.size(); }

    size_t num_gates() const { return gate_instances_.size(); }

    // ---- arithmetic (plonky2 gadgets/arithmetic.rs) -----------------------------------------------
    // const_0 * multiplicand_0 * multiplicand_1 + const_1 * addend
    Target arithmetic(u64 c0, u64 c1, Target m0, Target m1, Target addend) {
        Target special;
        if (arithmetic_special_cases(c0, c1, m0, m1, addend, &special)) return special;
        ArithKey key{c0, c1, m0, m1, addend};
        auto it = base_arithmetic_results_.find(key);
        if (it != base_arithmetic_results_.end()) return it->second;
        // find_slot(ArithmeticGate, params = [c0, c1])
        auto sl = arith_slots_.find({c0, c1});
        u32 row, i;
        if (sl == arith_slots_.end()) {
            row = add_gate(G_ARITHMETIC, c0, c1);
            i = 0;
        } else {
            row = sl->second.first;
            i = sl->second.second;
        }
        if (i == ARITH_OPS - 1)
            arith_slots_.erase({c0, c1});
        else
            arith_slots_[{c0, c1}] = {row, i + 1};
        connect(m0, wire_target(row, 4 * i));
        connect(m1, wire_target(row, 4 * i + 1));
        connect(addend, wire_target(row, 4 * i + 2));
        Target out = wire_target(row, 4 * i + 3);
        gens_.push_back(Gen{OP_ARITH, out, wire_target(row, 4 * i), wire_target(row, 4 * i + 1), wire_target(row, 4 * i + 2), 0, c0, c1});
        base_arithmetic_results_[key] = out;
        return out;
    }
    // c*x + y.  Upstream passes the constant one as the FIRST multiplicand here (`self.arithmetic(c, F::ONE, one, x, y)`), unlike
    // add / sub where it is the second: which of the two multiplicand wires carries x is part of the circuit.
    Target mul_const_add(u64 c, Target x, Target y) { return arithmetic(c, 1, one(), x, y); }
    Target add(Target x, Target y) { return arithmetic(1, 1, x, one(), y); }
    Target sub(Target x, Target y) { return arithmetic(1, gl::P - 1, x, one(), y); }
    Target mul(Target x, Target y) { return arithmetic(1, 0, x, y, x); }
    Target mul_sub(Target x, Target y, Target z) { return arithmetic(1, gl::P - 1, x, y, z); }  // x*y - z
    Target mul_const(u64 c, Target x) { return mul_const_add(c, x, zero()); }
    // if b { x } else { y }
    Target select(BoolTarget b, Target x, Target y) {
        Target tmp = mul_sub(b.target, y, y);
        return mul_sub(b.target, x, tmp);
    }
    BoolTarget not_(BoolTarget b) { return BoolTarget{sub(one(), b.target)}; }
    BoolTarget is_equal(Target x, Target y) {
        Target z = zero();
        BoolTarget equal = add_virtual_bool_target_unsafe();
        BoolTarget not_equal = not_(equal);
        Target inv = add_virtual_target();
        gens_.push_back(Gen{OP_EQ, equal.target, x, y, 0, 0, 0, 0});
        gens_.push_back(Gen{OP_EQINV, inv, x, y, 0, 0, 0, 0});
        Target diff = sub(x, y);
        Target not_equal_check = mul(equal.target, diff);
        Target diff_normalized = mul(diff, inv);
        connect(not_equal.target, diff_normalized);
        connect(not_equal_check, z);
        return equal;
    }

    // 1/x (plonky2 gadgets/arithmetic.rs `inverse`): a hinted value checked by x * inv = 1; x = 0 has no witness
    Target inverse(Target x) {
        Target inv = add_virtual_target();
        gens_.push_back(Gen{OP_EQINV, inv, x, zero(), 0, 0, 0, 0});
        connect(mul(x, inv), one());
        return inv;
    }

    // ---- bits and bytes of a field element (plonky2 gadgets/split_base.rs, split_join.rs, range_check.rs) ----------
    // Same names and meaning as upstream; the gates differ by construction (no BaseSumGate: booleanity is an ArithmeticGate
    // op, the sum a Horner chain, the limbs come from OP_LIMB hints), as they already do for the ecgfp5 circuits.
    // Arithmetic ops: assert_bool 1; le_sum n - 1 (64 bits: 68); split_le 2n (64 bits: 2n + 5); le_bytes_sum n - 1 (8 bytes:
    // 12); split_bytes_le n (8 bytes: 13) and one lookup per byte; is_less_than 6n + 5.
    void assert_bool(Target t) { connect(mul_sub(t, t, t), zero()); }

    // sum of bits[i] * 2^i.  The bits must be boolean already (assert_bool, or the result of a gadget).  With exactly 64 bits
    // the sum could pass p and wrap, so two spellings would denote the same field element; here the non-canonical one is
    // refused -- the result always denotes the integer the bits spell.  Upstream's le_sum does NOT do this: there the caller
    // has to know that 64 bits of a Goldilocks element are ambiguous.
    Target le_sum(const std::vector<BoolTarget>& bits) {
        if (bits.empty() || bits.size() > 64) throw std::runtime_error("le_sum: 1 to 64 bits");
        std::vector<Target> limbs;
        for (BoolTarget b : bits) limbs.push_back(b.target);
        return le_limbs_sum(limbs, 1);
    }
    // The little-endian bits of x, as upstream's split_le -- but sound for 64 bits too (see le_sum).  x must be below
    // 2^num_bits, or no witness exists.
    std::vector<BoolTarget> split_le(Target x, size_t num_bits) {
        if (num_bits < 1 || num_bits > 64) throw std::runtime_error("split_le: num_bits must be 1 to 64");
        std::vector<BoolTarget> bits(num_bits);
        for (size_t i = 0; i < num_bits; i++) {
            bits[i] = add_virtual_bool_target_unsafe();
            gens_.push_back(Gen{OP_LIMB, bits[i].target, x, 0, 0, 0, (u64)i, 1});
            assert_bool(bits[i].target);
        }
        assert_equal_to_input(le_sum(bits), x);
        return bits;
    }
    void range_check(Target x, size_t num_bits) {
        if (num_bits < 1 || num_bits > 63) throw std::runtime_error("range_check: num_bits must be 1 to 63");
        (void)split_le(x, num_bits);
    }
    // sum of bytes[i] * 256^i of range-checked bytes (ByteTargets); with exactly 8 bytes canonical, as le_sum with 64 bits
    Target le_bytes_sum(const std::vector<Target>& bytes) {
        if (bytes.empty() || bytes.size() > 8) throw std::runtime_error("le_bytes_sum: 1 to 8 bytes");
        return le_limbs_sum(bytes, 8);
    }
    // The little-endian bytes of x, each range-checked by a lookup into the byte table `u8_table_idx` the way
    // aes::add_virtual_byte_target does it, so they are ByteTargets of the AES gadgets.
    std::vector<Target> split_bytes_le(Target x, size_t num_bytes, size_t u8_table_idx) {
        if (num_bytes < 1 || num_bytes > 8) throw std::runtime_error("split_bytes_le: num_bytes must be 1 to 8");
        if (u8_table_idx >= luts_.size()) throw std::runtime_error("lut index not in luts");
        std::vector<Target> bytes(num_bytes);
        for (size_t i = 0; i < num_bytes; i++) {
            bytes[i] = add_virtual_target();
            gens_.push_back(Gen{OP_LIMB, bytes[i], x, 0, 0, 0, (u64)(8 * i), 8});
            add_lookup_from_index(bytes[i], u8_table_idx);  // aes::assert_byte
        }
        assert_equal_to_input(le_bytes_sum(bytes), x);
        return bytes;
    }
    // a < b for a, b below 2^num_bits (both are range-checked here): the top bit of a - b + 2^num_bits is clear
    BoolTarget is_less_than(Target a, Target b, size_t num_bits) {
        if (num_bits < 1 || num_bits > 62) throw std::runtime_error("is_less_than: num_bits must be 1 to 62");
        range_check(a, num_bits);
        range_check(b, num_bits);
        Target d = add(sub(a, b), constant(1ull << num_bits));
        return not_(split_le(d, num_bits + 1)[num_bits]);
    }

    // ---- lookups (plonky2 gadgets/lookup.rs) ------------------------------------------------------
    size_t add_lookup_table_from_pairs(const std::vector<std::pair<u16, u16>>& table) {
        // an empty table has no LookupTableGate row to stand on: (size() - 1) / LUT_SLOTS + 1 in add_all_lookups would wrap
        if (table.empty()) throw std::runtime_error("lookup table is empty");
        for (size_t i = 0; i < luts_.size(); i++)
            if (luts_[i] == table) return i;
        luts_.push_back(table);
        lut_to_lookups_.emplace_back();
        return luts_.size() - 1;
    }
    Target add_lookup_from_index(Target looking_in, size_t lut_index) {
        if (lut_index >= luts_.size()) throw std::runtime_error("lut index not in luts");
        Target looking_out = add_virtual_target();
        lut_to_lookups_[lut_index].push_back({looking_in, looking_out});
        return looking_out;
    }
    size_t num_luts() const { return luts_.size(); }

    // ---- hashing (plonky2 gadgets/hash.rs, hash/poseidon.rs AlgebraicHasher::permute_swapped) --------
    // One PoseidonGate row; swap = false.
    std::array<Target, 12> permute(const std::array<Target, 12>& inputs) { return permute_swapped(inputs, BoolTarget{zero()}); }
    // One PoseidonGate row that permutes inputs[4..8] | inputs[0..4] | inputs[8..12] where swap = 1 and `inputs` where swap = 0.
    // The gate's own constraint swap (swap - 1) = 0 makes `swap` boolean: no assert_bool is needed for it.
    std::array<Target, 12> permute_swapped(const std::array<Target, 12>& inputs, BoolTarget swap) {
        u32 row = add_gate(G_POSEIDON);
        connect(swap.target, wire_target(row, PG_SWAP));
        for (u32 i = 0; i < 12; i++) connect(inputs[i], wire_target(row, PG_IN + i));
        gens_.push_back(Gen{OP_POSEIDON, wire_target(row, PG_OUT), (Target)row, 0, 0, 0, 0, 0});
        std::array<Target, 12> out;
        for (u32 i = 0; i < 12; i++) out[i] = wire_target(row, PG_OUT + i);
        return out;
    }
    // Overwrite-mode sponge, rate 8 (poseidon-cipher/src/circuit.rs:123, hashed_elgamal/circuit.rs:42)
    std::vector<Target> hash_n_to_m_no_pad(const std::vector<Target>& inputs, size_t num_outputs) {
        std::array<Target, 12> state;
        state.fill(zero());
        for (size_t off = 0; off < inputs.size(); off += 8) {
            for (size_t i = 0; i < 8 && off + i < inputs.size(); i++) state[i] = inputs[off + i];
            state = permute(state);
        }
        std::vector<Target> outputs;
        for (;;) {
            for (size_t i = 0; i < 8; i++) {
                outputs.push_back(state[i]);
                if (outputs.size() == num_outputs) return outputs;
            }
            state = permute(state);
        }
    }

    // ---- Merkle membership (plonky2 hash/merkle_proofs.rs, gadgets/hash.rs) ---------------------------------------
    // Same names and meaning as upstream; the cap entry is chosen by a mux tree of `select` instead of a RandomAccessGate, so
    // gate counts differ by construction.  Per path level: one PoseidonGate row.  Per proof with cap height h: h assert_bool
    // ops and (2^h - 1) * 4 selects (two ArithmeticGate ops each), then four copy constraints.
    typedef std::array<Target, 4> HashOutTarget;
    HashOutTarget add_virtual_hash() { return HashOutTarget{add_virtual_target(), add_virtual_target(), add_virtual_target(), add_virtual_target()}; }
    std::vector<HashOutTarget> add_virtual_cap(u32 cap_height) {
        if (cap_height > 16) throw std::runtime_error("add_virtual_cap: cap_height must be 0 to 16");
        std::vector<HashOutTarget> cap((size_t)1 << cap_height);
        for (auto& h : cap) h = add_virtual_hash();
        return cap;
    }
    void connect_hashes(const HashOutTarget& x, const HashOutTarget& y) {
        for (u32 i = 0; i < 4; i++) connect(x[i], y[i]);
    }
    // The digest of a leaf: up to four elements zero-padded as they are, more through hash_n_to_hash_no_pad.
    HashOutTarget hash_or_noop(const std::vector<Target>& inputs) {
        HashOutTarget h;
        if (inputs.size() <= 4) {
            for (u32 i = 0; i < 4; i++) h[i] = i < inputs.size() ? inputs[i] : zero();
            return h;
        }
        std::vector<Target> o = hash_n_to_m_no_pad(inputs, 4);
        for (u32 i = 0; i < 4; i++) h[i] = o[i];
        return h;
    }
    // The walk from a digest: one PoseidonGate row per sibling, bit l the row's swap.  Returns the digest reached.
    HashOutTarget merkle_walk(HashOutTarget state, const std::vector<BoolTarget>& index_bits, const std::vector<HashOutTarget>& siblings) {
        for (size_t l = 0; l < siblings.size(); l++) {
            std::array<Target, 12> in;
            for (u32 i = 0; i < 4; i++) in[i] = state[i], in[4 + i] = siblings[l][i], in[8 + i] = zero();
            std::array<Target, 12> out = permute_swapped(in, index_bits[l]);
            for (u32 i = 0; i < 4; i++) state[i] = out[i];
        }
        return state;
    }
    // log2 of the cap's size; throws unless the cap holds a power of two of hashes and the bits are one per sibling and cap level
    u32 merkle_check_lengths(const char* who, const std::vector<BoolTarget>& index_bits, const std::vector<HashOutTarget>& cap, const std::vector<HashOutTarget>& siblings) {
        u32 cap_height = 0;
        while (((size_t)1 << cap_height) < cap.size()) cap_height++;
        if (cap.empty() || ((size_t)1 << cap_height) != cap.size()) throw std::runtime_error(std::string(who) + ": the cap must hold a power of two of hashes");
        if (index_bits.size() != siblings.size() + cap_height)
            throw std::runtime_error(std::string(who) + ": " + std::to_string(index_bits.size()) + " index bits for " + std::to_string(siblings.size()) +
                                     " siblings and cap height " + std::to_string(cap_height));
        return cap_height;
    }
    // The walk from `start` and the mux tree over the cap-index bits (made boolean here), then four copy constraints: what
    // verify_merkle_proof_to_cap does behind its leaf digest, and the map lookups behind theirs.
    void verify_merkle_walk_to_cap(const HashOutTarget& start, const std::vector<BoolTarget>& index_bits, const std::vector<HashOutTarget>& cap,
                                   const std::vector<HashOutTarget>& siblings) {
        HashOutTarget state = merkle_walk(start, index_bits, siblings);
        std::vector<HashOutTarget> entries = cap;
        for (size_t j = siblings.size(); j < index_bits.size(); j++) {
            BoolTarget bit = index_bits[j];
            assert_bool(bit.target);
            std::vector<HashOutTarget> half(entries.size() / 2);
            for (size_t i = 0; i < half.size(); i++)
                for (u32 w = 0; w < 4; w++) half[i][w] = select(bit, entries[2 * i + 1][w], entries[2 * i][w]);
            entries.swap(half);
        }
        connect_hashes(state, entries[0]);
    }
    // new_cap[i] = select(i == cap index, new_root, old_cap[i]) by the demux tree over the cap-index bits (merkle_update_to_cap's
    // comment has the counts); a cap of one is the new root itself.
    std::vector<HashOutTarget> merkle_demux_cap(const HashOutTarget& new_root, const std::vector<BoolTarget>& index_bits, size_t n_siblings,
                                                const std::vector<HashOutTarget>& old_cap) {
        if (old_cap.size() == 1) return {new_root};
        std::vector<Target> ind{one()};
        for (size_t j = index_bits.size(); j-- > n_siblings;) {
            std::vector<Target> next(2 * ind.size());
            for (size_t i = 0; i < ind.size(); i++) {
                next[2 * i + 1] = mul_sub(ind[i], index_bits[j].target, zero());  // the selects' constants: the ops share their gates
                next[2 * i] = sub(ind[i], next[2 * i + 1]);
            }
            ind.swap(next);
        }
        std::vector<HashOutTarget> new_cap(old_cap.size());
        for (size_t i = 0; i < old_cap.size(); i++)
            for (u32 w = 0; w < 4; w++) new_cap[i][w] = select(BoolTarget{ind[i]}, new_root[w], old_cap[i][w]);
        return new_cap;
    }
    // leaf_data is the leaf at index sum index_bits[i] 2^i of a tree with the given cap: the low siblings.size() bits walk the
    // path, the bits above them (log2 of the cap's size of them) choose the cap entry.  The path bits are made boolean by the
    // PoseidonGate's swap constraint; the cap-index bits reach only `select`, which constrains nothing, so they are made
    // boolean here with assert_bool.
    void verify_merkle_proof_to_cap(const std::vector<Target>& leaf_data, const std::vector<BoolTarget>& index_bits, const std::vector<HashOutTarget>& cap,
                                    const std::vector<HashOutTarget>& siblings) {
        if (cap.empty() || (cap.size() & (cap.size() - 1))) throw std::runtime_error("verify_merkle_proof_to_cap: the cap must hold a power of two of hashes");
        if (leaf_data.empty()) throw std::runtime_error("verify_merkle_proof_to_cap: empty leaf");
        merkle_check_lengths("verify_merkle_proof_to_cap", index_bits, cap, siblings);
        verify_merkle_walk_to_cap(hash_or_noop(leaf_data), index_bits, cap, siblings);
    }
    void verify_merkle_proof(const std::vector<Target>& leaf_data, const std::vector<BoolTarget>& index_bits, const HashOutTarget& root,
                             const std::vector<HashOutTarget>& siblings) {
        verify_merkle_proof_to_cap(leaf_data, index_bits, {root}, siblings);
    }
    // The tree with cap old_cap holds old_leaf at the index; the returned cap is that of the same tree with new_leaf there: the
    // state transition of one item of MerkleTree.update_batch, whose trace gives `siblings` (not an upstream gadget).  The old walk
    // is verify_merkle_proof_to_cap itself, assert_bool of the cap-index bits included; the new walk climbs from
    // hash_or_noop(new_leaf) over the SAME siblings and bits, one more PoseidonGate row per level.  new_cap[i] = select(i == cap
    // index, new root, old_cap[i]): the indicators come from a demux tree over the cap-index bits, the highest first
    // (2 (2^h - 1) ops: t = ind * bit - 0, ind - t), boolean because the bits are; then 4 * 2^h selects.  A cap of one is the new root.
    std::vector<HashOutTarget> merkle_update_to_cap(const std::vector<Target>& old_leaf, const std::vector<Target>& new_leaf, const std::vector<BoolTarget>& index_bits,
                                                    const std::vector<HashOutTarget>& old_cap, const std::vector<HashOutTarget>& siblings) {
        if (new_leaf.empty()) throw std::runtime_error("merkle_update_to_cap: empty leaf");
        if (new_leaf.size() != old_leaf.size()) throw std::runtime_error("merkle_update_to_cap: the old leaf has " + std::to_string(old_leaf.size()) + " targets, the new one " + std::to_string(new_leaf.size()));
        verify_merkle_proof_to_cap(old_leaf, index_bits, old_cap, siblings);  // throws on every other length mismatch, before anything is added
        return merkle_demux_cap(merkle_walk(hash_or_noop(new_leaf), index_bits, siblings), index_bits, siblings.size(), old_cap);
    }
    HashOutTarget merkle_update(const std::vector<Target>& old_leaf, const std::vector<Target>& new_leaf, const std::vector<BoolTarget>& index_bits,
                                const HashOutTarget& old_root, const std::vector<HashOutTarget>& siblings) {
        return merkle_update_to_cap(old_leaf, new_leaf, index_bits, {old_root}, siblings)[0];
    }

    // ---- sparse keyed trees (merkle_host.h: MerkleMap; not upstream gadgets) ------------------------------------------
    // key_bits are the D little-endian bits of the key: the low siblings.size() walk the path, the rest choose the cap entry, as
    // in verify_merkle_proof_to_cap.  An occupied leaf is hash_or_noop(value | one), an empty one four zero() targets.
    //   lookup   assert_bool(present) -- the selects alone constrain nothing about it --, start = select(present, occupied, 0^4)
    //            word by word, then verify_merkle_walk_to_cap.  One statement serves both answers, so `present` may be a public
    //            output.  With present = 0 the value targets are UNCONSTRAINED: a caller that reads them must gate on present.
    //   update   the old walk as lookup's from (old_present, old_value); the new walk from (new_present, new_value) over the same
    //            siblings and bits; the new cap from merkle_demux_cap.
    //   insert / remove   update with the flags fixed at (0, 1) / (1, 0): no select and no assert_bool for them, the empty side
    //            starts from zero() targets.
    // Cost: a leaf digest is no row for value_len <= 3 and ceil((value_len + 1) / 8) PoseidonGate rows above.  lookup: one digest,
    // one row per level, at most 9 ops (assert_bool, four selects; ops on the constant zero fold) and verify_merkle_proof_to_cap's h assert_bool + 8 (2^h - 1) mux ops.
    // update: two digests, two rows per level, at most 18 ops, the mux ops and merkle_update_to_cap's demux ops (2 (2^h - 1) - 1 + 8 * 2^h
    // for h >= 1).  insert / remove: one digest, two rows per level, the mux and demux ops only.
    void merkle_map_check(const char* who, const std::vector<BoolTarget>& key_bits, size_t value_len, const std::vector<HashOutTarget>& cap,
                          const std::vector<HashOutTarget>& siblings) {
        if (key_bits.empty() || key_bits.size() > 64) throw std::runtime_error(std::string(who) + ": 1 to 64 key bits");
        if (value_len > 134) throw std::runtime_error(std::string(who) + ": a value has at most 134 targets");
        if (merkle_check_lengths(who, key_bits, cap, siblings) > 16) throw std::runtime_error(std::string(who) + ": cap_height must be 0 to 16");
    }
    HashOutTarget merkle_map_leaf(std::vector<Target> value) {
        value.push_back(one());
        return hash_or_noop(value);
    }
    HashOutTarget merkle_map_start(BoolTarget present, const std::vector<Target>& value) {
        assert_bool(present.target);
        HashOutTarget occupied = merkle_map_leaf(value), start;
        for (u32 w = 0; w < 4; w++) start[w] = select(present, occupied[w], zero());
        return start;
    }
    HashOutTarget merkle_map_empty() { return HashOutTarget{zero(), zero(), zero(), zero()}; }
    void merkle_map_lookup_to_cap(const std::vector<BoolTarget>& key_bits, const std::vector<Target>& value, BoolTarget present, const std::vector<HashOutTarget>& cap,
                                  const std::vector<HashOutTarget>& siblings) {
        merkle_map_check("merkle_map_lookup_to_cap", key_bits, value.size(), cap, siblings);
        verify_merkle_walk_to_cap(merkle_map_start(present, value), key_bits, cap, siblings);
    }
    // old_start under old_cap; the returned cap has new_start at the key
    std::vector<HashOutTarget> merkle_map_transition(const HashOutTarget& old_start, const HashOutTarget& new_start, const std::vector<BoolTarget>& key_bits,
                                                     const std::vector<HashOutTarget>& old_cap, const std::vector<HashOutTarget>& siblings) {
        verify_merkle_walk_to_cap(old_start, key_bits, old_cap, siblings);
        return merkle_demux_cap(merkle_walk(new_start, key_bits, siblings), key_bits, siblings.size(), old_cap);
    }
    std::vector<HashOutTarget> merkle_map_update_to_cap(const std::vector<BoolTarget>& key_bits, BoolTarget old_present, const std::vector<Target>& old_value,
                                                        BoolTarget new_present, const std::vector<Target>& new_value, const std::vector<HashOutTarget>& old_cap,
                                                        const std::vector<HashOutTarget>& siblings) {
        if (old_value.size() != new_value.size())
            throw std::runtime_error("merkle_map_update_to_cap: the old value has " + std::to_string(old_value.size()) + " targets, the new one " + std::to_string(new_value.size()));
        merkle_map_check("merkle_map_update_to_cap", key_bits, old_value.size(), old_cap, siblings);
        const HashOutTarget old_start = merkle_map_start(old_present, old_value);
        const HashOutTarget new_start = merkle_map_start(new_present, new_value);
        return merkle_map_transition(old_start, new_start, key_bits, old_cap, siblings);
    }
    std::vector<HashOutTarget> merkle_map_insert_to_cap(const std::vector<BoolTarget>& key_bits, const std::vector<Target>& value, const std::vector<HashOutTarget>& old_cap,
                                                        const std::vector<HashOutTarget>& siblings) {
        merkle_map_check("merkle_map_insert_to_cap", key_bits, value.size(), old_cap, siblings);
        const HashOutTarget leaf = merkle_map_leaf(value);
        return merkle_map_transition(merkle_map_empty(), leaf, key_bits, old_cap, siblings);
    }
    std::vector<HashOutTarget> merkle_map_remove_to_cap(const std::vector<BoolTarget>& key_bits, const std::vector<Target>& value, const std::vector<HashOutTarget>& old_cap,
                                                        const std::vector<HashOutTarget>& siblings) {
        merkle_map_check("merkle_map_remove_to_cap", key_bits, value.size(), old_cap, siblings);
        const HashOutTarget leaf = merkle_map_leaf(value);
        return merkle_map_transition(leaf, merkle_map_empty(), key_bits, old_cap, siblings);
    }

    // ---- ecGFp5 scalar-multiplication step (ecstep_gate.h; not an upstream gate) ---------------------
    // One EcStepGate row: mid = 2 acc, out = mid + bit Q in (X:Z:U:T) coordinates, acc = X | Z | U | T and Q = x | u.  `bit` is
    // not made boolean here.  hinted = false leaves the row without a generator: the caller sets mid and out.
    struct EcStep {
        std::array<Target, 20> mid, out;
    };
    EcStep ec_step(const std::array<Target, 20>& acc, const std::array<Target, 10>& q, Target bit, bool hinted = true) {
        u32 row = add_gate(G_ECSTEP);
        for (u32 i = 0; i < 20; i++) connect(acc[i], wire_target(row, EG_ACC + i));
        for (u32 i = 0; i < 10; i++) connect(q[i], wire_target(row, EG_Q + i));
        connect(bit, wire_target(row, EG_BIT));
        if (hinted) gens_.push_back(Gen{OP_ECSTEP, wire_target(row, EG_MID), (Target)row, 0, 0, 0, 0, 0});
        EcStep r;
        for (u32 i = 0; i < 20; i++) r.mid[i] = wire_target(row, EG_MID + i), r.out[i] = wire_target(row, EG_OUT + i);
        return r;
    }
    // multiply_point (ecgfp5.h) as 320 EcStepGate rows instead of arithmetic gates; off by default
    void set_ec_gate(bool on) { ec_gate_ = on; }
    bool ec_gate() const { return ec_gate_; }
    // AesGcmTarget's GHASH from carry-less multiply tables (aes_gadgets.h ghash_tables_target) with `lanes` blocks per
    // reduction, 1 to 16; 0, the default, is the reference's bit-serial circuit
    void set_ghash_tables(int lanes) {
        if (lanes < 0 || lanes > 16) throw std::runtime_error("set_ghash_tables: lanes must be 0 (off) or 1 to 16");
        ghash_tables_ = lanes;
    }
    int ghash_tables() const { return ghash_tables_; }

    // ---- build (plonky2 CircuitBuilder::build) ----------------------------------------------------
    Circuit build();

   private:
    struct ArithKey {
        u64 c0, c1;
        Target m0, m1, a;
        bool operator==(const ArithKey& o) const { return c0 == o.c0 && c1 == o.c1 && m0 == o.m0 && m1 == o.m1 && a == o.a; }
    };
    struct ArithKeyHash {
        size_t operator()(const ArithKey& k) const {
            u64 h = k.c0 * 0x9E3779B97F4A7C15ull;
            h = (h ^ k.c1) * 0xC2B2AE3D27D4EB4Full;
            h = (h ^ k.m0) * 0x9E3779B97F4A7C15ull;
            h = (h ^ k.m1) * 0xC2B2AE3D27D4EB4Full;
            h = (h ^ k.a) * 0x9E3779B97F4A7C15ull;
            return (size_t)(h ^ (h >> 29));
        }
    };
    struct Gen {
        u32 kind;
        Target out, a, b, c;
        u32 aux;
        u64 k0, k1;
    };

    bool arithmetic_special_cases(u64 c0, u64 c1, Target m0, Target m1, Target addend, Target* out) {
        Target z = zero();
        u64 m0c = 0, m1c = 0, ac = 0;
        bool m0k = target_as_constant(m0, &m0c), m1k = target_as_constant(m1, &m1c), ak = target_as_constant(addend, &ac);
        bool first_zero = c0 == 0 || m0 == z || m1 == z;
        bool second_zero = c1 == 0 || addend == z;
        bool fk = false, sk = false;
        u64 fv = 0, sv = 0;
        if (first_zero) {
            fk = true;
        } else if (m0k && m1k) {
            fk = true;
            fv = gl::mul(gl::mul(m0c, m1c), c0);
        }
        if (second_zero) {
            sk = true;
        } else if (ak) {
            sk = true;
            sv = gl::mul(ac, c1);
        }
        if (fk && sk) {
            *out = constant(gl::add(fv, sv));
            return true;
        }
        if (first_zero && c1 == 1) {
            *out = addend;
            return true;
        }
        if (second_zero) {
            if (m0k && gl::mul(m0c, c0) == 1) {
                *out = m1;
                return true;
            }
            if (m1k && gl::mul(m1c, c0) == 1) {
                *out = m0;
                return true;
            }
        }
        return false;
    }

    // Horner chain over limbs [lo, hi) of `width` bits each, most significant first: hi - lo - 1 ops on one ArithmeticGate shape
    Target horner(const std::vector<Target>& limbs, size_t lo, size_t hi, u32 width) {
        Target acc = limbs[hi - 1];
        for (size_t i = hi - 1; i-- > lo;) acc = mul_const_add(1ull << width, acc, limbs[i]);
        return acc;
    }
    // le_sum / le_bytes_sum.  64 bits in all: the integer must be below p = 2^64 - 2^32 + 1, that is, NOT (high half all
    // ones and low half non-zero): is_equal(hi, 2^32 - 1) * lo = 0.
    Target le_limbs_sum(const std::vector<Target>& limbs, u32 width) {
        const size_t n = limbs.size();
        if (n * width < 64) return horner(limbs, 0, n, width);
        Target lo = horner(limbs, 0, n / 2, width), hi = horner(limbs, n / 2, n, width);
        BoolTarget top = is_equal(hi, constant(0xFFFFFFFFull));
        connect(mul(top.target, lo), zero());
        return mul_const_add(1ull << 32, hi, lo);
    }
    // sum == x for the x a split started from.  Not connect(sum, x): that would make the sum's generator a producer of x's
    // slot, which the limb hints read -- a witness program that waits on itself whenever x is a plain input.
    void assert_equal_to_input(Target sum, Target x) { connect(sub(sum, x), zero()); }

    u32 add_gate(u32 kind, u64 c0 = 0, u64 c1 = 0) {
        u32 row = (u32)gate_instances_.size();
        gate_instances_.push_back(GateInstance{kind, {c0, c1}});
        if (kind == G_CONSTANT) {
            constant_generators_.push_back({row, 0});
            constant_generators_.push_back({row, 1});
        }
        return row;
    }
    void add_all_lookups();

    Config cfg_;
    bool ec_gate_ = false;
    int ghash_tables_ = 0;
    u64 num_virtual_ = 0;
    std::vector<GateInstance> gate_instances_;
    std::vector<std::pair<Target, Target>> copy_constraints_;
    std::map<u64, Target> constants_to_targets_;  // ordered by canonical value, as upstream's sorted_by_key
    std::unordered_map<Target, u64> targets_to_constants_;
    std::unordered_map<ArithKey, Target, ArithKeyHash> base_arithmetic_results_;
    std::map<std::pair<u64, u64>, std::pair<u32, u32>> arith_slots_;
    std::vector<std::vector<std::pair<u16, u16>>> luts_;
    std::vector<std::vector<std::pair<Target, Target>>> lut_to_lookups_;
    std::vector<LookupRows> lookup_rows_;
    std::vector<std::pair<u32, u32>> constant_generators_;  // (row, index)
    std::vector<Gen> gens_;
    std::vector<Target> public_inputs_;
};

// Adds, per LUT: LookupGate rows for the looking pairs, then the LookupTableGate rows (stored upside down),
// then one NoopGate.  plonky2 CircuitBuilder::add_all_lookups.
inline void CircuitBuilder::add_all_lookups() {
    for (size_t lut = 0; lut < luts_.size(); lut++) {
        auto& lookups = lut_to_lookups_[lut];
        if (lookups.empty()) throw std::runtime_error("LUT is unused");
        u32 last_lu_gate = (u32)num_gates();
        u32 row = 0, slot = LU_SLOTS;
        for (auto& pr : lookups) {
            if (slot == LU_SLOTS) {
                row = add_gate(G_LOOKUP, (u64)lut, 0);
                slot = 0;
            }
            Target gin = wire_target(row, 2 * slot), gout = wire_target(row, 2 * slot + 1);
            connect(gin, pr.first);
            connect(gout, pr.second);
            gens_.push_back(Gen{OP_LOOKUP, gout, gin, 0, 0, (u32)lut, 0, 0});
            slot++;
        }
        u32 last_lut_gate = (u32)num_gates();
        u32 num_lut_rows = (u32)((luts_[lut].size() - 1) / LUT_SLOTS + 1);
        for (u32 i = 0; i < num_lut_rows; i++) add_gate(G_LOOKUP_TABLE, (u64)lut, 0);
        u32 first_lut_gate = (u32)num_gates() - 1;
        add_gate(G_NOOP);
        lookup_rows_.push_back(LookupRows{last_lu_gate, last_lut_gate, first_lut_gate});
    }
}

inline Circuit CircuitBuilder::build() {
    Circuit c;
    c.cfg = cfg_;
    const u32 R = cfg_.num_routed_wires;

    // Public inputs.  Without any (the reference registers none) the public-input hash is hash_no_pad([]) = 0^4 and needs
    // no PoseidonGate: four zero constants go to the PublicInputGate, and the circuit is what it was before public inputs
    // existed.  With some, as upstream: public_inputs_hash = hash_n_to_hash_no_pad(public_inputs) in the circuit (one
    // PoseidonGate row per 8 inputs), its four elements connected to the gate's wires 0..3.
    // Upstream also attaches RandomValueGenerators to the gate's unused wires (randomize_unused_pi_wires);
    // here those wires stay 0 so that proofs are reproducible.
    if (public_inputs_.empty()) {
        Target z = zero();
        u32 pi_gate = add_gate(G_PUBLIC_INPUT);
        for (u32 i = 0; i < 4; i++) connect(z, wire_target(pi_gate, i));
    } else {
        std::vector<Target> h = hash_n_to_m_no_pad(public_inputs_, 4);
        u32 pi_gate = add_gate(G_PUBLIC_INPUT);
        for (u32 i = 0; i < 4; i++) connect(h[i], wire_target(pi_gate, i));
    }
    add_all_lookups();
    while (constants_to_targets_.size() > constant_generators_.size()) add_gate(G_CONSTANT);
    {
        size_t k = 0;
        for (auto& kv : constants_to_targets_) {
            auto cg = constant_generators_[k++];
            gate_instances_[cg.first].constants[cg.second] = kv.first;
            Target w = wire_target(cg.first, cg.second);
            connect(w, kv.second);
            gens_.push_back(Gen{OP_CONST, w, 0, 0, 0, 0, kv.first, 0});
        }
    }
    // blind_and_pad.  zk: blinding_counts() rows of random wires for the regular polynomials, and pairs of rows with
    // equal (copy-constrained) random routed wires for the Z polynomials; then pad with NoopGates to a power of two.
    if (cfg_.zero_knowledge) {
        const size_t D = 2, num_gates_now = gate_instances_.size();
        size_t degree_estimate = 1;
        while (degree_estimate < num_gates_now) degree_estimate <<= 1;
        size_t regular = 0, zopen = 0;
        for (;;) {
            u32 db_est = 0;
            while (((size_t)1 << db_est) < degree_estimate) db_est++;
            Circuit tmp;
            tmp.cfg = cfg_;
            tmp.degree_bits = db_est;
            size_t folding = 0, prod = 1;
            for (u32 a : tmp.reduction_arity_bits()) {
                folding += ((size_t)1 << a) - 1;
                prod <<= a;
            }
            size_t final_coeffs = degree_estimate / prod;
            size_t fri_openings = cfg_.num_query_rounds * (1 + D * folding + D * final_coeffs);
            regular = D + fri_openings;
            zopen = 2 * D + fri_openings;
            if (num_gates_now + regular + 2 * zopen <= degree_estimate) break;
            degree_estimate <<= 1;
        }
        for (size_t i = 0; i < regular; i++) c.blind_rows.push_back(add_gate(G_NOOP));
        for (size_t i = 0; i < zopen; i++) {
            u32 g1 = add_gate(G_NOOP), g2 = add_gate(G_NOOP);
            for (u32 w = 0; w < R; w++) connect(wire_target(g1, w), wire_target(g2, w));
            c.blind_zrows.push_back({g1, g2});
        }
    }
    while (gate_instances_.size() < 4 || (gate_instances_.size() & (gate_instances_.size() - 1)) != 0) add_gate(G_NOOP);
    const size_t n = gate_instances_.size();
    u32 db = 0;
    while ((1ull << db) < n) db++;
    c.degree_bits = db;

    // ---- gate types, sorted by (degree, id) as `gates.sort_unstable_by_key(|g| (g.0.degree(), g.0.id()))`; selector
    // polynomials (plonky2 gates/selectors.rs).  A LookupGate's id is "LookupGate {num_slots: 40, lut_hash: [..]}" and a
    // LookupTableGate's "LookupTableGate {num_slots: 26, lut_hash: [..], last_lut_row: R}" with the table's Keccak-256 as a
    // Rust {:?} byte list, so each table contributes two gate types of its own.
    struct GateType {
        u32 kind, lut;
        std::string id;
    };
    std::vector<GateType> types;
    {
        bool present[G_NUM_KINDS] = {false};
        for (auto& g : gate_instances_) present[g.kind] = true;
        for (size_t l = 0; l < luts_.size(); l++) {
            std::vector<uint8_t> bytes;
            for (auto& pr : luts_[l])
                for (u16 v : {pr.first, pr.second}) {
                    bytes.push_back((uint8_t)(v & 0xFF));
                    bytes.push_back((uint8_t)(v >> 8));
                }
            auto h = kc::keccak256(bytes.data(), bytes.size());
            std::string hs = "[";
            for (size_t i = 0; i < h.size(); i++) hs += (i ? ", " : "") + std::to_string((unsigned)h[i]);
            hs += "]";
            types.push_back({G_LOOKUP, (u32)l, "LookupGate {num_slots: " + std::to_string(LU_SLOTS) + ", lut_hash: " + hs + "}"});
            types.push_back({G_LOOKUP_TABLE, (u32)l,
                             "LookupTableGate {num_slots: " + std::to_string(LUT_SLOTS) + ", lut_hash: " + hs + ", last_lut_row: " + std::to_string(lookup_rows_[l].last_lut) + "}"});
        }
        if (present[G_NOOP]) types.push_back({G_NOOP, 0, "NoopGate"});
        if (present[G_CONSTANT]) types.push_back({G_CONSTANT, 0, "ConstantGate { num_consts: 2 }"});
        if (present[G_PUBLIC_INPUT]) types.push_back({G_PUBLIC_INPUT, 0, "PublicInputGate"});
        if (present[G_ARITHMETIC]) types.push_back({G_ARITHMETIC, 0, "ArithmeticGate { num_ops: 20 }"});
        if (present[G_ECSTEP]) types.push_back({G_ECSTEP, 0, "EcStepGate"});
        if (present[G_POSEIDON]) types.push_back({G_POSEIDON, 0, "PoseidonGate(PhantomData<plonky2_field::goldilocks_field::GoldilocksField>)<WIDTH=12>"});
        std::sort(types.begin(), types.end(), [](const GateType& a, const GateType& b) {
            u32 da = gate_degree(a.kind), db = gate_degree(b.kind);
            return da != db ? da < db : a.id < b.id;
        });
    }
    for (auto& t : types) c.gates.push_back(t.kind);
    const u32 num_gates_kinds = (u32)c.gates.size();
    auto type_index = [&](const GateInstance& g) -> u32 {
        for (u32 i = 0; i < num_gates_kinds; i++)
            if (types[i].kind == g.kind && ((g.kind != G_LOOKUP && g.kind != G_LOOKUP_TABLE) || types[i].lut == (u32)g.constants[0])) return i;
        throw std::runtime_error("gate instance without a gate type");
    };
    const u32 max_degree = cfg_.quotient_degree_factor + 1;
    const u32 max_gate_degree = gate_degree(c.gates.back());
    if (max_gate_degree + num_gates_kinds - 1 <= max_degree) {
        c.groups.push_back({0, num_gates_kinds});
        c.selector_index.assign(num_gates_kinds, 0);
    } else {
        u32 start = 0;
        while (start < num_gates_kinds) {
            u32 size = 0;
            while (start + size < num_gates_kinds && size + gate_degree(c.gates[start + size]) < max_degree) size++;
            c.groups.push_back({start, start + size});
            start += size;
        }
        c.selector_index.resize(num_gates_kinds);
        for (u32 g = 0; g < c.groups.size(); g++)
            for (u32 i = c.groups[g].first; i < c.groups[g].second; i++) c.selector_index[i] = g;
    }
    c.num_gate_constraints = 0;
    for (u32 k : c.gates) c.num_gate_constraints = std::max(c.num_gate_constraints, gate_num_constraints(k));
    c.luts = luts_;
    c.lookup_rows = lookup_rows_;
    for (auto& l : lut_to_lookups_) c.num_lookups.push_back((u32)l.size());
    c.num_lookup_selectors = luts_.empty() ? 0 : 4 + (u32)luts_.size();

    const u32 nsel = c.num_selectors();
    const u32 ncc = c.num_constants_cols();
    c.constants.assign((size_t)ncc * n, 0);
    for (size_t row = 0; row < n; row++) {
        u32 gi = type_index(gate_instances_[row]);
        for (u32 s = 0; s < nsel; s++)
            c.constants[(size_t)s * n + row] = (nsel == 1 || c.selector_index[gi] == s) ? gi : UNUSED_SELECTOR;
        for (u32 k = 0; k < cfg_.num_constants; k++)
            c.constants[(size_t)(nsel + c.num_lookup_selectors + k) * n + row] =
                (gate_instances_[row].kind == G_ARITHMETIC || gate_instances_[row].kind == G_CONSTANT) ? gate_instances_[row].constants[k] : 0;
    }
    // lookup selectors: TransSre, TransLdc, InitSre, LastLdc, then one StartEnd per LUT (selectors_lookup,
    // selector_ends_lookups).
    for (size_t l = 0; l < lookup_rows_.size(); l++) {
        auto lr = lookup_rows_[l];
        u64* col = &c.constants[(size_t)nsel * n];
        for (u32 r = lr.last_lut; r <= lr.first_lut; r++) col[0 * n + r] = 1;
        for (u32 r = lr.last_lu; r < lr.last_lut; r++) col[1 * n + r] = 1;
        col[2 * n + lr.first_lut + 1] = 1;
        col[3 * n + lr.last_lu] = 1;
        col[(4 + l) * n + lr.last_lut] = 1;
    }

    // ---- copy constraints -> partitions (union-find over virtual targets and routed wires) ----
    const u64 V = num_virtual_;
    const u64 N = V + (u64)n * R;
    if (N >= 0xFFFFFFF0ull) throw std::runtime_error("circuit too large for 32-bit node ids");
    auto node = [&](Target t) -> u32 {
        if (is_wire(t)) {
            if (wire_col(t) >= R) throw std::runtime_error("copy constraint on non-routed wire");
            return (u32)(V + (u64)wire_row(t) * R + wire_col(t));
        }
        return (u32)t;
    };
    std::vector<u32> parent(N);
    for (u64 i = 0; i < N; i++) parent[i] = (u32)i;
    auto find = [&](u32 x) {
        u32 r = x;
        while (parent[r] != r) r = parent[r];
        while (parent[x] != r) {
            u32 nx = parent[x];
            parent[x] = r;
            x = nx;
        }
        return r;
    };
    for (auto& cc : copy_constraints_) {
        u32 a = find(node(cc.first)), b = find(node(cc.second));
        if (a != b) parent[std::max(a, b)] = std::min(a, b);
    }

    // ---- sigma: every routed wire goes to the next wire of its partition in (row, column) order, the last to the first
    // (plonk/permutation_argument.rs: `wire_partition` fills each class `for row { for column {..} }`, `get_sigma_map` links
    // neighbours cyclically) ----
    c.k_is.resize(R);
    {
        u64 k = 1;
        for (u32 i = 0; i < R; i++) {
            c.k_is[i] = k;
            k = gl::mul(k, gl::MULT_GEN);
        }
    }
    std::vector<u64> subgroup(n);
    {
        u64 w = gl::root_of_unity((int)db), x = 1;
        for (size_t i = 0; i < n; i++) {
            subgroup[i] = x;
            x = gl::mul(x, w);
        }
    }
    c.sigmas.resize((size_t)R * n);
    {
        const u32 NONE = 0xFFFFFFFFu;
        std::vector<u32> first(N, NONE), last(N, NONE);  // per class: column * n + row of its first / latest wire
        auto sig = [&](u64 from, u64 to) { c.sigmas[from] = gl::mul(c.k_is[to / n], subgroup[to % n]); };
        for (u32 row = 0; row < n; row++)
            for (u32 col = 0; col < R; col++) {
                const u32 idx = (u32)((u64)col * n + row);
                u32 r = find((u32)(V + (u64)row * R + col));
                if (first[r] == NONE)
                    first[r] = idx;
                else
                    sig(last[r], idx);
                last[r] = idx;
            }
        for (u64 r = 0; r < N; r++)
            if (first[r] != NONE) sig(last[r], first[r]);
    }

    // ---- witness program over slots ----
    std::vector<int32_t> slot_of(N, -1);
    u32 num_slots = 0;
    auto slot = [&](Target t) -> u32 {
        u32 r = find(node(t));
        if (slot_of[r] < 0) slot_of[r] = (int32_t)num_slots++;
        return (u32)slot_of[r];
    };
    std::vector<Op> ops(gens_.size());
    for (size_t i = 0; i < gens_.size(); i++) {
        const Gen& g = gens_[i];
        Op o{g.kind, slot(g.out), 0, 0, 0, g.aux, g.k0, g.k1};
        if (g.kind == OP_ARITH) {
            o.a = slot(g.a);
            o.b = slot(g.b);
            o.c = slot(g.c);
        } else if (g.kind == OP_LOOKUP || g.kind == OP_LIMB) {
            o.a = slot(g.a);
        } else if (g.kind == OP_EQ || g.kind == OP_EQINV) {
            o.a = slot(g.a);
            o.b = slot(g.b);
        } else if (g.kind == OP_POSEIDON) {
            u32 row = (u32)g.a;
            o.a = row;
            o.aux = (u32)c.poseidon_rows.size();
            c.poseidon_rows.push_back(row);
            for (u32 col = 0; col < R; col++) slot(wire_target(row, col));  // every routed wire of the row carries a value
        } else if (g.kind == OP_ECSTEP) {
            o.a = (u32)g.a;
        }
        ops[i] = o;
    }
    // wires 0..70 of an EcStepGate row carry a value whether or not the row has a generator (an unhinted row's are set by the caller)
    for (size_t row = 0; row < n; row++)
        if (gate_instances_[row].kind == G_ECSTEP)
            for (u32 col = 0; col < EG_WIRES; col++) slot(wire_target((u32)row, col));
    c.vt_slot.resize(V);
    for (u64 v = 0; v < V; v++) c.vt_slot[v] = (int32_t)slot((Target)v);
    for (Target t : public_inputs_) c.pi_slots.push_back(slot(t));  // routed PoseidonGate inputs: every one has a slot already
    c.num_slots = num_slots;
    c.wire_slot.resize((size_t)R * n);
    for (u64 idx = 0; idx < (u64)R * n; idx++) {
        u32 col = (u32)(idx / n), row = (u32)(idx % n);
        c.wire_slot[idx] = slot_of[find((u32)(V + (u64)row * R + col))];
    }
    // levelise (Kahn).  A slot becomes available when its FIRST producer (in this order) has run -- exactly
    // plonky2's "generator fires once its watch list is set"; any further producer of the same slot (two
    // computed values tied by `connect`) runs at a strictly later level and only checks equality.
    {
        const size_t M = ops.size();
        std::vector<u32> num_producers(num_slots, 0);
        std::vector<std::vector<u32>> consumers(num_slots);
        auto wslot = [&](u32 row, u32 col) -> u32 { return (u32)slot_of[find((u32)(V + (u64)row * R + col))]; };
        auto inputs = [&](const Op& o, u32* in) -> int {
            if (o.kind == OP_ARITH) { in[0] = o.a; in[1] = o.b; in[2] = o.c; return 3; }
            if (o.kind == OP_LOOKUP || o.kind == OP_LIMB) { in[0] = o.a; return 1; }
            if (o.kind == OP_EQ || o.kind == OP_EQINV) { in[0] = o.a; in[1] = o.b; return 2; }
            if (o.kind == OP_POSEIDON) {
                for (u32 k = 0; k < 12; k++) in[k] = wslot(o.a, PG_IN + k);
                in[12] = wslot(o.a, PG_SWAP);
                return 13;
            }
            if (o.kind == OP_ECSTEP) {
                for (u32 k = 0; k < EG_MID; k++) in[k] = wslot(o.a, k);
                return (int)EG_MID;
            }
            return 0;
        };
        auto outputs = [&](const Op& o, u32* out) -> int {
            if (o.kind == OP_ECSTEP) {
                for (u32 col = EG_MID; col < EG_WIRES; col++) out[col - EG_MID] = wslot(o.a, col);
                return (int)(EG_WIRES - EG_MID);
            }
            if (o.kind != OP_POSEIDON) { out[0] = o.out; return 1; }
            int k = 0;
            for (u32 col = PG_OUT; col < R; col++)
                if (col != PG_SWAP) out[k++] = wslot(o.a, col);
            return k;
        };
        for (size_t i = 0; i < M; i++) {
            u32 outs[80];
            int k = outputs(ops[i], outs);
            for (int j = 0; j < k; j++) num_producers[outs[j]]++;
        }
        std::vector<u32> pending(M, 0), level(M, 0), slot_level(num_slots, 0);
        std::vector<uint8_t> slot_ready(num_slots, 0);
        for (size_t i = 0; i < M; i++) {
            u32 in[32];
            int k = inputs(ops[i], in);
            for (int j = 0; j < k; j++) {
                bool dup = false;
                for (int j2 = 0; j2 < j; j2++) dup |= in[j2] == in[j];
                if (dup) continue;
                if (num_producers[in[j]] > 0) {
                    pending[i]++;
                    consumers[in[j]].push_back((u32)i);
                }
            }
        }
        // The inverse hints (OP_EQINV: a 96-multiplication Fermat inversion on one lane) feed only equality checks,
        // never the values a circuit computes with.  Left at their natural level they put an inversion into every
        // level of a sequential chain (inc32's carry chain: four per AES-CTR block); instead they are held back until
        // everything else is scheduled and then run side by side in one level, their checks in the levels after.
        std::vector<u32> queue, deferred;
        auto ready = [&](u32 i) { (ops[i].kind == OP_EQINV ? deferred : queue).push_back(i); };
        for (size_t i = 0; i < M; i++)
            if (pending[i] == 0) ready((u32)i);
        size_t done = 0;
        u32 max_level = 0, floor_level = 0;
        for (;;) {
            while (done < queue.size()) {
                u32 i = queue[done++];
                u32 in[32], outs[80];
                int k = inputs(ops[i], in);
                int ko = outputs(ops[i], outs);
                u32 lv = ops[i].kind == OP_EQINV ? floor_level : 0;
                for (int j = 0; j < k; j++) lv = std::max(lv, slot_level[in[j]]);
                for (int j = 0; j < ko; j++) lv = std::max(lv, slot_level[outs[j]]);
                level[i] = lv;  // ops with only user-set inputs are level 0
                max_level = std::max(max_level, lv);
                for (int j = 0; j < ko; j++) {
                    u32 s = outs[j];
                    slot_level[s] = lv + 1;
                    if (!slot_ready[s]) {
                        slot_ready[s] = 1;
                        for (u32 cns : consumers[s])
                            if (--pending[cns] == 0) ready(cns);
                    }
                }
            }
            if (deferred.empty()) break;
            floor_level = max_level + 1;
            queue.insert(queue.end(), deferred.begin(), deferred.end());
            deferred.clear();
        }
        if (done != M) throw std::runtime_error("witness program has a dependency cycle");
        c.level_offsets.assign(max_level + 2, 0);
        for (size_t i = 0; i < M; i++) c.level_offsets[level[i] + 1]++;
        for (u32 l = 0; l <= max_level; l++) c.level_offsets[l + 1] += c.level_offsets[l];
        std::vector<u32> cursor(c.level_offsets.begin(), c.level_offsets.end() - 1);
        c.ops.resize(M);
        for (size_t i = 0; i < M; i++) c.ops[cursor[level[i]]++] = ops[i];
        if (M == 0) c.level_offsets = {0, 0};
    }
    return c;
}

}  // namespace p2
