// Shared by capi_host.cpp and prover_gpu.hip: error slot and circuit-shape helpers.
#pragma once
#include <string>

#include "../../include/p2aes.h"
#include "circuit.h"
#include "proof_layout.h"

namespace p2 {
extern thread_local std::string g_last_error;
inline void set_error(const std::string& s) { g_last_error = s; }

// exact proof size in bytes for the layout written by the prover (proof_layout.h; DESIGN.md "Proof layout")
inline size_t proof_bytes(const Circuit& c) { return make_proof_layout(c).bytes; }
// ProofWithPublicInputs::public_inputs: the trailer of one proof with layout `L`.  O(k): reads the last 8 (k + 1) bytes only.
// *n_written = k (0 without public inputs).
inline int read_public_inputs(const ProofLayout& L, const uint8_t* proof, size_t proof_len, uint64_t* out, size_t cap, size_t* n_written) {
    const size_t k = L.num_pi;
    if (n_written) *n_written = k;
    if (!proof || proof_len != L.bytes) return set_error("proof length differs from the circuit's proof size"), P2_ERR_INVALID;
    if (k == 0) return P2_OK;
    u64 cnt;
    memcpy(&cnt, proof + L.pi_cnt_off, 8);
    if (cnt != k) return set_error("wrong number of public inputs"), P2_ERR_INVALID;
    if (!out || cap < k) return set_error("output buffer holds fewer than " + std::to_string(k) + " public inputs"), P2_ERR_INVALID;
    memcpy(out, proof + L.pi_off, 8 * k);
    return P2_OK;
}
inline void fill_info(const Circuit& c, p2_circuit_info* o) {
    o->degree_bits = c.degree_bits;
    o->num_wires = c.cfg.num_wires;
    o->num_routed_wires = c.cfg.num_routed_wires;
    o->num_constants_cols = c.num_constants_cols();
    o->num_zs_cols = c.num_zs_cols();
    o->num_quotient_cols = c.num_quotient_cols();
    o->num_luts = (uint32_t)c.luts.size();
    o->num_ops = (uint32_t)c.ops.size();
    o->num_levels = (uint32_t)c.level_offsets.size() - 1;
    o->num_slots = c.num_slots;
    o->num_virtual_targets = (uint32_t)c.vt_slot.size();
    o->num_fri_rounds = (uint32_t)c.reduction_arity_bits().size();
    o->proof_bytes = proof_bytes(c);
    o->zero_knowledge = c.cfg.zero_knowledge;
    o->num_gate_kinds = (uint32_t)c.gates.size();
    o->num_public_inputs = (uint32_t)c.pi_slots.size();
    o->hasher = c.cfg.hasher;
}
}  // namespace p2
