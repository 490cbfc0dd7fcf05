// Compressed proofs on the host: ProofWithPublicInputs::compress, CompressedProofWithPublicInputs::decompress and
// CircuitData::verify_compressed (upstream plonky2 hash/path_compression.rs and fri/proof.rs, restated; DESIGN.md section 8
// gives the byte layout and the verdict order).  The reference for the GPU path of kernels_compress.h.
//
// A compressed proof keeps the full layout's prefix (caps, openings, FRI caps) and tail (final_poly, pow_witness, public-input
// trailer) and replaces the 28 query blocks with
//   query indices                                28 x u32, in the order the transcript draws them
//   initial trees   for each DISTINCT index:     4 x (leaf row, u8 sibling count, kept siblings)
//   FRI round r     for each distinct coset:     15 extension evals, u8 sibling count, kept siblings
// every list in ascending order of its index.  Which siblings are kept, and which evaluation is left out, depends on the
// indices alone, so the layout of a compressed proof is a function of (circuit, indices).
#pragma once
#include <algorithm>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "capi_common.h"
#include "verifier.h"

namespace p2 {

// The layout of one compressed proof, from its query indices.
struct CompressLayout {
    std::vector<std::vector<size_t>> leaf, rep, off;  // [tree][query]: leaf index, first query with that leaf, byte offset of its block
    std::vector<std::vector<std::vector<bool>>> kept; // [tree][query][level]: the sibling is stored in this query's block
    size_t len = 0;
};
inline size_t popcount(const std::vector<bool>& v) { return (size_t)std::count(v.begin(), v.end(), true); }
// One stored opening of tree t: the leaf words (initial tree o's row, or a FRI coset without the evaluation left out), the
// count byte, the kept siblings; an initial-tree block holds four of them.
inline size_t leaf_bytes(const ProofLayout& s, size_t t, int o) { return t == 0 ? 8 * (size_t)s.init[o].width : 8 * (size_t)s.step[t - 1].width - 16; }
inline size_t block_bytes(const ProofLayout& s, size_t t, size_t kept) {
    size_t b = 0;
    for (int o = 0; o < (t == 0 ? 4 : 1); o++) b += leaf_bytes(s, t, o) + 1 + 32 * kept;
    return b;
}
inline CompressLayout compress_layout(const ProofLayout& s, const std::vector<size_t>& idx) {
    CompressLayout L;
    const size_t T = s.num_trees(), Q = s.num_queries;
    L.leaf.assign(T, std::vector<size_t>(Q));
    L.rep = L.off = L.leaf;
    L.kept.resize(T);
    size_t pos = s.queries_off + 4 * Q;
    for (size_t t = 0; t < T; t++) {
        const size_t depth = s.tree(t).depth, nl = (size_t)1 << (depth + s.cap_height);
        for (size_t q = 0; q < Q; q++) {
            L.leaf[t][q] = idx[q] >> s.tree(t).shift;
            L.rep[t][q] = q;
            for (size_t e = 0; e < q; e++)
                if (L.leaf[t][e] == L.leaf[t][q]) {
                    L.rep[t][q] = e;
                    break;
                }
        }
        // compress_merkle_proofs: every node on a query's path below the cap is known; walking the queries in order, a
        // sibling that is not yet known is kept and becomes known
        std::set<size_t> known;
        for (size_t q = 0; q < Q; q++)
            for (size_t j = 0; j < depth; j++) known.insert((L.leaf[t][q] + nl) >> j);
        L.kept[t].assign(Q, std::vector<bool>(depth, false));
        for (size_t q = 0; q < Q; q++) {
            size_t node = L.leaf[t][q] + nl;
            for (size_t l = 0; l < depth; l++, node >>= 1)
                if (known.insert(node ^ 1).second) L.kept[t][q][l] = true;
        }
        std::vector<size_t> order;
        for (size_t q = 0; q < Q; q++)
            if (L.rep[t][q] == q) order.push_back(q);
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return L.leaf[t][a] < L.leaf[t][b]; });
        for (size_t q : order) {
            L.off[t][q] = pos;
            pos += block_bytes(s, t, popcount(L.kept[t][q]));
        }
        for (size_t q = 0; q < Q; q++) L.off[t][q] = L.off[t][L.rep[t][q]];
    }
    L.len = pos + s.tail_bytes();
    return L;
}

struct ByteWriter {
    std::vector<uint8_t>& b;
    size_t pos;
    void u64w(u64 v) {
        memcpy(&b[pos], &v, 8);
        pos += 8;
    }
    void u8w(uint8_t v) { b[pos++] = v; }
    void hash(const Hash4& h) {
        for (int i = 0; i < 4; i++) u64w(h.e[i]);
    }
    void ext(gl::E2 e) {
        u64w(e.a);
        u64w(e.b);
    }
};

// The full layout of DESIGN.md section 8 from a parsed proof (the inverse of parse_proof).
inline std::vector<uint8_t> serialize_proof(const Circuit& c, const ParsedProof& pp) {
    std::vector<uint8_t> out(proof_bytes(c));
    ByteWriter w{out, 0};
    for (auto* cap : {&pp.wires_cap, &pp.zs_cap, &pp.quot_cap})
        for (auto& h : *cap) w.hash(h);
    for (auto* v : {&pp.o_constants, &pp.o_sigmas, &pp.o_wires, &pp.o_zs, &pp.o_zs_next, &pp.o_lk, &pp.o_lk_next, &pp.o_pp, &pp.o_quot})
        for (auto& e : *v) w.ext(e);
    for (auto& cap : pp.fri_caps)
        for (auto& h : cap) w.hash(h);
    for (auto& q : pp.queries) {
        for (int o = 0; o < 4; o++) {
            for (u64 v : q.init_evals[o]) w.u64w(v);
            w.u8w((uint8_t)q.init_proofs[o].size());
            for (auto& h : q.init_proofs[o]) w.hash(h);
        }
        for (size_t k = 0; k < q.step_evals.size(); k++) {
            for (auto& e : q.step_evals[k]) w.ext(e);
            w.u8w((uint8_t)q.step_proofs[k].size());
            for (auto& h : q.step_proofs[k]) w.hash(h);
        }
    }
    for (auto& e : pp.final_poly) w.ext(e);
    w.u64w(pp.pow_witness);
    if (!pp.pis.empty()) {
        w.u64w(pp.pis.size());
        for (u64 v : pp.pis) w.u64w(v);
    }
    return out;
}

// ProofWithPublicInputs::compress.  Shape and canonicality are checked as verify_proof checks them; the proof-of-work and
// everything after it are not (a compressed proof is verified by verify_compressed).
inline std::string compress_proof(const Circuit& c, const VerifierData& vd, const uint8_t* bytes, size_t len, std::vector<uint8_t>& out) {
    ParsedProof pp;
    std::string err = parse_proof(c, bytes, len, pp);
    if (!err.empty()) return err;
    const Transcript T = fiat_shamir(c, vd, pp);
    const ProofLayout s = make_proof_layout(c);
    const size_t Q = s.num_queries, prefix = s.queries_off, tail_len = s.tail_bytes();
    const CompressLayout L = compress_layout(s, T.query_idx);
    out.assign(L.len, 0);
    memcpy(out.data(), bytes, prefix);
    memcpy(out.data() + L.len - tail_len, bytes + s.final_off, tail_len);
    for (size_t q = 0; q < Q; q++) {
        const u32 v = (u32)T.query_idx[q];
        memcpy(&out[prefix + 4 * q], &v, 4);
    }
    for (size_t t = 0; t < L.leaf.size(); t++)
        for (size_t q = 0; q < Q; q++) {
            if (L.rep[t][q] != q) continue;
            const ProofQuery& pq = pp.queries[q];
            ByteWriter w{out, L.off[t][q]};
            auto siblings = [&](const std::vector<Hash4>& path) {
                w.u8w((uint8_t)popcount(L.kept[t][q]));
                for (size_t l = 0; l < path.size(); l++)
                    if (L.kept[t][q][l]) w.hash(path[l]);
            };
            if (t == 0) {
                for (int o = 0; o < 4; o++) {
                    for (u64 v : pq.init_evals[o]) w.u64w(v);
                    siblings(pq.init_proofs[o]);
                }
            } else {
                const size_t r = t - 1, arity = s.step[r].width / 2;
                const size_t left_out = (T.query_idx[q] >> s.tree(r).shift) & (arity - 1);  // what the fold check recomputes
                for (size_t k = 0; k < arity; k++)
                    if (k != left_out) w.ext(pq.step_evals[r][k]);
                siblings(pq.step_proofs[r]);
            }
        }
    return "";
}

// decompress_merkle_proofs: the leaves' digests, then level by level every query's parent, taking a sibling from the query's
// own block where the layout keeps one and from the nodes already seen otherwise.  siblings[q] receives the full path.
inline bool decompress_paths(const CompressLayout& L, size_t t, size_t depth, size_t cap_h, const std::vector<Hash4>& leaf_hash,
                             const std::vector<std::vector<Hash4>>& stored, std::vector<std::vector<Hash4>>& siblings, u32 hasher) {
    const size_t Q = leaf_hash.size(), nl = (size_t)1 << (depth + cap_h);
    std::map<size_t, Hash4> seen;
    for (size_t q = 0; q < Q; q++) seen[L.leaf[t][q] + nl] = leaf_hash[q];
    std::vector<size_t> cursor(Q, 0);
    for (size_t l = 0; l < depth; l++)
        for (size_t q = 0; q < Q; q++) {
            const size_t node = (L.leaf[t][q] + nl) >> l;
            if (L.kept[t][q][l]) seen[node ^ 1] = stored[q][cursor[q]++];
            auto s = seen.find(node ^ 1);
            if (s == seen.end()) return false;
            const Hash4& cur = seen[node];
            seen[node >> 1] = (node & 1) ? h_two_to_one(s->second, cur, hasher) : h_two_to_one(cur, s->second, hasher);
        }
    siblings.assign(Q, std::vector<Hash4>(depth));
    for (size_t q = 0; q < Q; q++)
        for (size_t l = 0; l < depth; l++) siblings[q][l] = seen[((L.leaf[t][q] + nl) >> l) ^ 1];
    return true;
}

// CompressedProofWithPublicInputs::decompress.  Verdict order: the shape -- indices readable and below
// the LDE size, exact length, sibling counts, public-input count -- then canonicality of every word, then (check_pow, for
// verify_compressed) the proof-of-work, then the written indices against the drawn ones.
inline std::string decompress_proof(const Circuit& c, const VerifierData& vd, const uint8_t* cb, size_t clen, std::vector<uint8_t>& out,
                                    bool check_pow) {
    using namespace gl;
    const ProofLayout s = make_proof_layout(c);
    const size_t Q = s.num_queries, prefix = s.queries_off, tail_len = s.tail_bytes();
    if (clen < prefix + 4 * Q) return "proof truncated";
    std::vector<size_t> idx(Q);
    for (size_t q = 0; q < Q; q++) {
        u32 v;
        memcpy(&v, cb + prefix + 4 * q, 4);
        if ((v >> s.lde_bits) != 0) return compressed_shape_reason(CS_INDEX_RANGE);
        idx[q] = v;
    }
    const CompressLayout L = compress_layout(s, idx);
    if (clen < L.len) return "proof truncated";
    if (clen > L.len) return "trailing bytes in proof";
    const size_t T = L.leaf.size();
    for (size_t t = 0; t < T; t++)
        for (size_t q = 0; q < Q; q++) {
            if (L.rep[t][q] != q) continue;
            const size_t k = popcount(L.kept[t][q]);
            size_t at = L.off[t][q];
            for (int o = 0; o < (t == 0 ? 4 : 1); o++) {
                at += leaf_bytes(s, t, o);
                if (cb[at] != k) return compressed_shape_reason(CS_SIBLING_COUNT);
                at += 1 + 32 * k;
            }
        }
    const size_t tail = L.len - tail_len, pi_cnt = tail + (s.pi_cnt_off - s.final_off);
    if (!c.pi_slots.empty()) {
        u64 k;
        memcpy(&k, cb + pi_cnt, 8);
        if (k != c.pi_slots.size()) return "wrong number of public inputs";
    }
    // canonicality of every word: the prefix, each block's words (not its count byte), the tail (not the public-input count)
    auto canon = [&](size_t at, size_t words) {
        for (size_t i = 0; i < words; i++) {
            u64 v;
            memcpy(&v, cb + at + 8 * i, 8);
            if (v >= P) return false;
        }
        return true;
    };
    if (!canon(0, prefix / 8) || !canon(tail, 2 * s.final_len + 1) || !canon(pi_cnt + 8, c.pi_slots.size())) return "non-canonical field element";
    for (size_t t = 0; t < T; t++)
        for (size_t q = 0; q < Q; q++) {
            if (L.rep[t][q] != q) continue;
            const size_t k = popcount(L.kept[t][q]);
            size_t at = L.off[t][q];
            for (int o = 0; o < (t == 0 ? 4 : 1); o++) {
                const size_t ev = leaf_bytes(s, t, o) / 8;
                if (!canon(at, ev) || !canon(at + 8 * ev + 1, 4 * k)) return "non-canonical field element";
                at += 8 * ev + 1 + 32 * k;
            }
        }
    // Keccak circuits: the range of every hash word (caps of the prefix, kept siblings), with the precedence of canonicality
    if (c.cfg.hasher == HASHER_KECCAK) {
        auto ranged = [&](size_t at, size_t hashes) {
            for (size_t i = 0; i < hashes; i++) {
                u64 h[4];
                memcpy(h, cb + at + 32 * i, 32);
                if (!kc::in_range(h)) return false;
            }
            return true;
        };
        const size_t cap_hashes = s.cap_bytes / 32;
        bool ok = ranged(s.caps_off[0], 3 * cap_hashes) && ranged(s.fri_caps_off, s.step.size() * cap_hashes);
        for (size_t t = 0; t < T && ok; t++)
            for (size_t q = 0; q < Q && ok; q++) {
                if (L.rep[t][q] != q) continue;
                const size_t k = popcount(L.kept[t][q]);
                size_t at = L.off[t][q];
                for (int o = 0; o < (t == 0 ? 4 : 1); o++) {
                    ok = ok && ranged(at + leaf_bytes(s, t, o) + 1, k);
                    at += leaf_bytes(s, t, o) + 1 + 32 * k;
                }
            }
        if (!ok) return "hash word out of range";
    }
    // the transcript reads the prefix and the tail only: parse them as a full proof with empty query blocks
    std::vector<uint8_t> full(s.bytes, 0);
    memcpy(full.data(), cb, prefix);
    memcpy(full.data() + s.final_off, cb + tail, tail_len);
    for (size_t q = 0; q < Q; q++) {
        uint8_t* qb = &full[s.queries_off + q * s.query_bytes];
        for (auto& p : s.init) qb[p.cnt_off] = (uint8_t)p.depth;
        for (auto& p : s.step) qb[p.cnt_off] = (uint8_t)p.depth;
    }
    ParsedProof pp;
    std::string err = parse_proof(c, full.data(), full.size(), pp);
    if (!err.empty()) return "internal: " + err;
    const Transcript Tr = fiat_shamir(c, vd, pp);
    if (check_pow && (Tr.pow_response >> (64 - c.cfg.pow_bits)) != 0) return "Invalid proof-of-work witness.";
    if (Tr.query_idx != idx) return compressed_shape_reason(CS_INDICES);

    auto rd64 = [&](size_t at) {
        u64 v;
        memcpy(&v, cb + at, 8);
        return v;
    };
    auto rdhash = [&](size_t at) {
        Hash4 h;
        for (int i = 0; i < 4; i++) h.e[i] = rd64(at + 8 * i);
        return h;
    };
    // initial trees: the leaf rows, then each tree's paths
    for (size_t q = 0; q < Q; q++) {
        size_t at = L.off[0][q];
        const size_t k = popcount(L.kept[0][L.rep[0][q]]);
        for (int o = 0; o < 4; o++) {
            auto& ev = pp.queries[q].init_evals[o];
            for (size_t i = 0; i < s.init[o].width; i++) ev[i] = rd64(at + 8 * i);
            at += leaf_bytes(s, 0, o) + 1 + 32 * k;
        }
    }
    auto rebuild = [&](size_t t, const std::vector<Hash4>& leaf_hash, const std::vector<size_t>& stored_at, std::vector<std::vector<Hash4>>& paths) {
        std::vector<std::vector<Hash4>> stored(Q);
        for (size_t q = 0; q < Q; q++)
            for (size_t i = 0; i < popcount(L.kept[t][q]); i++) stored[q].push_back(rdhash(stored_at[q] + 32 * i));
        return decompress_paths(L, t, s.tree(t).depth, s.cap_height, leaf_hash, stored, paths, c.cfg.hasher);
    };
    for (int o = 0; o < 4; o++) {
        std::vector<Hash4> lh(Q);
        std::vector<size_t> stored_at(Q);
        for (size_t q = 0; q < Q; q++) {
            const auto& ev = pp.queries[q].init_evals[o];
            lh[q] = h_hash_or_noop(ev.data(), ev.size(), c.cfg.hasher);
            size_t at = L.off[0][q];
            const size_t k = popcount(L.kept[0][L.rep[0][q]]);
            for (int o2 = 0; o2 < o; o2++) at += leaf_bytes(s, 0, o2) + 1 + 32 * k;
            stored_at[q] = at + leaf_bytes(s, 0, o) + 1;
        }
        std::vector<std::vector<Hash4>> paths;
        if (!rebuild(0, lh, stored_at, paths)) return "internal: Merkle path reconstruction";
        for (size_t q = 0; q < Q; q++) pp.queries[q].init_proofs[o] = paths[q];
    }
    // FRI rounds: the evaluation the first query of a coset leaves out is the value its fold check expects
    const E2 g_zeta = mul(Tr.zeta, root_of_unity((int)c.degree_bits));
    auto reduce = [&](const std::vector<E2>& v) {
        E2 acc = e2(0);
        for (size_t k = v.size(); k-- > 0;) acc = add(mul(acc, Tr.fri_alpha), v[k]);
        return acc;
    };
    const E2 red0 = reduce(Tr.batch0), red1 = reduce(Tr.batch1);
    const u64 w_lde = root_of_unity((int)s.lde_bits);
    std::vector<u64> sx0(Q);
    for (size_t q = 0; q < Q; q++) sx0[q] = mul(MULT_GEN, pow(w_lde, bitrev((u32)idx[q], (int)s.lde_bits)));
    for (size_t r = 0; r < s.step.size(); r++) {
        const size_t t = 1 + r, arity = s.step[r].width / 2;
        std::vector<Hash4> lh(Q);
        std::vector<size_t> stored_at(Q);
        for (size_t q = 0; q < Q; q++) {
            auto& ev = pp.queries[q].step_evals[r];
            const size_t rq = L.rep[t][q];
            if (rq == q) {
                const size_t left_out = (idx[q] >> s.tree(r).shift) & (arity - 1);
                const E2 v = r == 0 ? fri_combine_initial(c, pp.queries[q], sx0[q], Tr, red0, red1, g_zeta)
                                    : fri_compute_evaluation(pp.queries[q].step_evals[r - 1], idx[q] >> s.tree(r - 1).shift,
                                                             exp_pow2(sx0[q], (int)s.tree(r - 1).shift), s.arity_bits(r - 1), Tr.fri_betas[r - 1]);
                for (size_t k = 0, i = 0; k < arity; k++) {
                    if (k == left_out) {
                        ev[k] = v;
                        continue;
                    }
                    const size_t at = L.off[t][q] + 16 * i++;
                    ev[k] = e2(rd64(at), rd64(at + 8));
                }
            } else {
                ev = pp.queries[rq].step_evals[r];  // (rq < q: complete already)
            }
            std::vector<u64> flat;
            for (auto& e : ev) flat.push_back(e.a), flat.push_back(e.b);
            lh[q] = h_hash_or_noop(flat.data(), flat.size(), c.cfg.hasher);
            stored_at[q] = L.off[t][q] + leaf_bytes(s, t, 0) + 1;
        }
        std::vector<std::vector<Hash4>> paths;
        if (!rebuild(t, lh, stored_at, paths)) return "internal: Merkle path reconstruction";
        for (size_t q = 0; q < Q; q++) pp.queries[q].step_proofs[r] = paths[q];
    }
    out = serialize_proof(c, pp);
    return "";
}

// CircuitData::verify_compressed: verify_proof of the decompressed proof, behind the checks of decompression.
inline std::string verify_compressed_proof(const Circuit& c, const VerifierData& vd, const uint8_t* cb, size_t clen) {
    std::vector<uint8_t> full;
    std::string err = decompress_proof(c, vd, cb, clen, full, true);
    if (!err.empty()) return err;
    return verify_proof(c, vd, full.data(), full.size());
}

}  // namespace p2
