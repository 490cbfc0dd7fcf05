// The byte layout of a serialised proof and the order of its opening set, each defined once.
// Host only.  Read by the prover's proof assembly, the GPU verifier's and compressor's table builders (prover_gpu.hip),
// the size / public-input accessors of capi_common.h and the host compressor (compress.h).  Deliberately NOT read by
// verifier.h (parse_proof), compress.h's serialize_proof and the Python restatements under tests/: they pin it from outside.
#pragma once
#include <vector>

#include "circuit.h"

namespace p2 {

// ---- the opening set
// The prover evaluates into five slot blocks: preprocessed | wires | Z(zeta) | Z(g zeta) | quotient, each as wide as its
// oracle (the Z oracle's columns: NC zs, the partial products, the lookup polynomials).
enum OpenSlot { OS_PRE, OS_WIRES, OS_Z, OS_Z_NEXT, OS_QUOT, OS_SLOTS };
// The nine opening vectors, numbered in the order they are serialised.  write_opening_set puts lookup_zs / lookup_zs_next
// between plonk_zs_next and the partial products (the OpeningSet struct itself lists them last).
enum OpenGroup { OG_CONSTANTS, OG_SIGMAS, OG_WIRES, OG_ZS, OG_ZS_NEXT, OG_LOOKUP_ZS, OG_LOOKUP_ZS_NEXT, OG_PARTIAL_PRODUCTS, OG_QUOTIENT, OG_GROUPS };
// The order they are observed by the transcript and reduced by FRI: the batch opened at zeta, then the one at g zeta.
static const OpenGroup OPEN_OBSERVED[OG_GROUPS] = {OG_CONSTANTS, OG_SIGMAS,    OG_WIRES,   OG_ZS,           OG_PARTIAL_PRODUCTS,
                                                   OG_QUOTIENT,  OG_LOOKUP_ZS, OG_ZS_NEXT, OG_LOOKUP_ZS_NEXT};
static const u32 OPEN_BATCH0 = 7;  // OPEN_OBSERVED[0..7) are opened at zeta

struct OpeningSet {
    struct Group {
        OpenSlot slot;
        u32 lo, hi;  // columns [lo, hi) of the slot's oracle
        u32 len() const { return hi - lo; }
    } g[OG_GROUPS];
    u32 slot_base[OS_SLOTS], slots;  // first evaluation slot of each block, and their total
    u32 n_b0 = 0, n_b1 = 0;          // extension elements in the two observed batches
    u32 slot_of(OpenGroup k, u32 i) const { return slot_base[g[k].slot] + g[k].lo + i; }
    // evaluation slots in observed / serialised order (the prover's gather maps)
    std::vector<u32> slots_in(bool observed) const {
        std::vector<u32> v;
        for (u32 k = 0; k < OG_GROUPS; k++) {
            const OpenGroup gk = observed ? OPEN_OBSERVED[k] : (OpenGroup)k;
            for (u32 i = 0; i < g[gk].len(); i++) v.push_back(slot_of(gk, i));
        }
        return v;
    }
};
inline OpeningSet make_opening_set(const Circuit& c) {
    const u32 np = c.num_preprocessed(), W = c.cfg.num_wires, zc = c.num_zs_cols(), qc = c.num_quotient_cols(), NC = c.cfg.num_challenges;
    const u32 ncc = c.num_constants_cols(), nzpp = c.num_zs_pp();
    OpeningSet s{};
    s.g[OG_CONSTANTS] = {OS_PRE, 0, ncc};
    s.g[OG_SIGMAS] = {OS_PRE, ncc, np};
    s.g[OG_WIRES] = {OS_WIRES, 0, W};
    s.g[OG_ZS] = {OS_Z, 0, NC};
    s.g[OG_ZS_NEXT] = {OS_Z_NEXT, 0, NC};
    s.g[OG_LOOKUP_ZS] = {OS_Z, nzpp, zc};
    s.g[OG_LOOKUP_ZS_NEXT] = {OS_Z_NEXT, nzpp, zc};
    s.g[OG_PARTIAL_PRODUCTS] = {OS_Z, NC, nzpp};
    s.g[OG_QUOTIENT] = {OS_QUOT, 0, qc};
    const u32 width[OS_SLOTS] = {np, W, zc, zc, qc};
    for (u32 b = 0; b < OS_SLOTS; b++) {
        s.slot_base[b] = s.slots;
        s.slots += width[b];
    }
    for (u32 k = 0; k < OG_GROUPS; k++) (k < OPEN_BATCH0 ? s.n_b0 : s.n_b1) += s.g[OPEN_OBSERVED[k]].len();
    return s;
}

// ---- the proof
// Byte offsets and counts in one full proof.  Everything is a little-endian u64 word except the u8 sibling count in front of
// each Merkle path.  After the PoW witness, only for a circuit with k >= 1 public inputs, comes the trailer u64 k || k x u64
// value (plonky2 writes the public inputs as a field vector after the proof); zero-PI proofs have none.
struct ProofLayout {
    struct Vec {
        size_t off;
        u32 len;  // extension elements
    };
    // One Merkle opening inside a query, offsets relative to the query's start: the leaf, the count byte, the siblings.
    struct Path {
        size_t leaf_off, cnt_off, sib_off;
        u32 width;  // words of the leaf: an initial tree's row with its salt, or a FRI coset's 2 * arity
        u32 depth;  // siblings below the cap
        u32 shift;  // leaf index = query index >> shift
    };
    OpeningSet set{};
    size_t cap_bytes = 0, caps_off[3] = {0, 0, 0};  // wires, zs / partial products, quotient
    Vec open[OG_GROUPS] = {};
    size_t fri_caps_off = 0;
    size_t queries_off = 0, query_bytes = 0;
    u32 num_queries = 0;
    Path init[4] = {};       // constants + sigmas, wires, zs / partial products, quotient
    std::vector<Path> step;  // per FRI round
    size_t final_off = 0, pow_off = 0;
    u32 final_len = 0;
    u32 num_pi = 0;
    size_t pi_cnt_off = 0, pi_off = 0;  // the count word and the values (both = body_bytes without public inputs)
    size_t body_bytes = 0;  // up to and including the PoW witness: where the trailer starts
    size_t bytes = 0;
    u32 cap_height = 0, lde_bits = 0;
    size_t tail_bytes() const { return bytes - final_off; }  // final polynomial, PoW witness, trailer
    // tree 0 = the initial trees (one depth for all four), tree 1 + r = FRI round r
    size_t num_trees() const { return 1 + step.size(); }
    const Path& tree(size_t t) const { return t == 0 ? init[0] : step[t - 1]; }
    u32 arity_bits(size_t r) const { return step[r].shift - tree(r).shift; }
};
inline ProofLayout make_proof_layout(const Circuit& c) {
    const u32 cap_h = c.cfg.cap_height, lde_bits = c.degree_bits + c.cfg.rate_bits;
    const std::vector<u32> ar = c.reduction_arity_bits();
    ProofLayout L;
    L.set = make_opening_set(c);
    const OpeningSet& os = L.set;
    size_t off = 0;
    auto take = [&off](size_t bytes) {
        const size_t at = off;
        off += bytes;
        return at;
    };
    L.cap_height = cap_h, L.lde_bits = lde_bits;
    L.cap_bytes = (size_t)32 << cap_h;
    for (size_t& o : L.caps_off) o = take(L.cap_bytes);
    for (u32 k = 0; k < OG_GROUPS; k++) L.open[k] = {take(16 * (size_t)os.g[k].len()), os.g[k].len()};
    L.fri_caps_off = take(ar.size() * L.cap_bytes);
    L.queries_off = off;
    L.num_queries = c.cfg.num_query_rounds;
    size_t q = 0;
    auto path = [&q](u32 width, u32 depth, u32 shift) {
        ProofLayout::Path p{q, q + 8 * (size_t)width, q + 8 * (size_t)width + 1, width, depth, shift};
        q = p.sib_off + 32 * (size_t)depth;
        return p;
    };
    const u32 cols[4] = {c.num_preprocessed(), c.cfg.num_wires + c.salt(), c.num_zs_cols() + c.salt(), c.num_quotient_cols() + c.salt()};
    for (int o = 0; o < 4; o++) L.init[o] = path(cols[o], lde_bits - cap_h, 0);
    u32 bits = lde_bits;
    for (u32 a : ar) {
        bits -= a;
        L.step.push_back(path(2u << a, bits - cap_h, lde_bits - bits));
    }
    L.query_bytes = q;
    take(q * L.num_queries);
    L.final_len = (u32)((size_t)1 << (bits - c.cfg.rate_bits));
    L.final_off = take(16 * (size_t)L.final_len);
    L.pow_off = take(8);
    L.body_bytes = off;
    L.num_pi = (u32)c.pi_slots.size();
    L.pi_cnt_off = take(L.num_pi ? 8 : 0);
    L.pi_off = take(8 * (size_t)L.num_pi);
    L.bytes = off;
    return L;
}
}  // namespace p2
