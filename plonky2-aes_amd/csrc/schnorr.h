// Schnorr signatures on ecGFp5 with a Poseidon challenge: the native scheme on the host (the twin of kernels_schnorr.h) and the
// circuit gadget.  pod2 is not in the reference tree, so the scheme is this project's own and UNPINNED against pod2's signature
// bytes:
//     keys       sk in [1, n),  pk = sk G                                            (ecgfp5::public_key)
//     challenge  e_words = hash_n_to_hash_no_pad(R.x | R.u | pk.x | pk.u | msg),  e = sum e_words[i] 2^(64 i)  (< 2^256 < n)
//     sign       R = k G for a caller-supplied nonce k in [1, n),  s = (k + e sk) mod n;  the signature is s (5 limbs) | e_words
//     verify     malformed (2): s >= n; a word of e_words, msg or pk not below p; pk outside the group; pk neutral.
//                R' = s G + e (-pk);  accepted (0) iff the challenge of R' is e_words, else rejected (1).
// R' = neutral is not special: the k = 0 signature (s = e sk, e = H((0,0) | pk | msg)) verifies; sign refuses k = 0.
#pragma once
#include "ecgfp5.h"
#include "ecgfp5_scalar.h"

namespace p2 {
namespace schnorr {

using ecgfp5::Affine;
using ecgfp5::U320;

static const size_t SIG_WORDS = 9;
static const size_t MAX_MSG_LEN = 1024;
enum { ST_ACCEPTED = 0, ST_REJECTED = 1, ST_MALFORMED = 2 };

inline bool fq_canonical(const ecgfp5::Fq& a) {
    for (u64 w : a)
        if (w >= gl::P) return false;
    return true;
}
inline bool words_canonical(const u64* w, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (w[i] >= gl::P) return false;
    return true;
}
inline bool scalar_in_range(const U320& k) { return !ecsc::sc_is_zero(k.w) && ecsc::sc_below_order(k.w); }  // [1, n)
// a public key a verifier takes: canonical words, in the group, not the neutral
inline bool pk_valid(const Affine& pk) {
    if (!fq_canonical(pk.x) || !fq_canonical(pk.u)) return false;
    if (pk.x == ecgfp5::fq_zero() && pk.u == ecgfp5::fq_zero()) return false;
    return ecgfp5::is_in_subgroup(pk);
}
inline void challenge(const Affine& r, const Affine& pk, const u64* msg, size_t msg_len, u64 e[4]) {
    std::vector<u64> in = ecgfp5::as_fields(r);
    const std::vector<u64> p = ecgfp5::as_fields(pk);
    in.insert(in.end(), p.begin(), p.end());
    in.insert(in.end(), msg, msg + msg_len);
    const std::vector<u64> h = pcipher::hash_n_to_m_no_pad(in, 4);
    std::copy(h.begin(), h.end(), e);
}
// status 0 and sig (and pk, if asked for) written, or 2 and sig (and pk) zeroed: sk or k not in [1, n), a message word not below p
inline int sign(const U320& sk, const U320& k, const u64* msg, size_t msg_len, u64 sig[SIG_WORDS], Affine* pk_out) {
    std::fill(sig, sig + SIG_WORDS, 0);
    if (pk_out) *pk_out = Affine{ecgfp5::fq_zero(), ecgfp5::fq_zero()};
    if (!scalar_in_range(sk) || !scalar_in_range(k) || !words_canonical(msg, msg_len)) return ST_MALFORMED;
    const Affine pk = ecgfp5::public_key(sk), r = ecgfp5::scalar_mul(k, ecgfp5::generator());
    challenge(r, pk, msg, msg_len, sig + 5);
    const u64 e[5] = {sig[5], sig[6], sig[7], sig[8], 0};
    ecsc::sc_muladd(e, sk.w, k.w, sig);
    if (pk_out) *pk_out = pk;
    return ST_ACCEPTED;
}
inline int verify(const Affine& pk, const u64* msg, size_t msg_len, const u64 sig[SIG_WORDS]) {
    if (!ecsc::sc_below_order(sig) || !words_canonical(sig + 5, 4) || !words_canonical(msg, msg_len) || !pk_valid(pk)) return ST_MALFORMED;
    U320 s, e;
    memcpy(s.w, sig, 40);
    memcpy(e.w, sig + 5, 32);
    e.w[4] = 0;
    const Affine r = ecgfp5::point_add(ecgfp5::scalar_mul(s, ecgfp5::generator()), ecgfp5::scalar_mul(e, ecgfp5::point_neg(pk)));
    u64 h[4];
    challenge(r, pk, msg, msg_len, h);
    return memcmp(h, sig + 5, 32) == 0 ? ST_ACCEPTED : ST_REJECTED;
}

// ------------------------------------------------------------------------------------------ the gadget
// A signature in a circuit: s as 320 little-endian bit targets (each constrained to {0, 1}) and the four challenge words.
struct SignatureTarget {
    std::vector<BoolTarget> s_bits;
    CircuitBuilder::HashOutTarget e;
};
inline SignatureTarget add_virtual_signature_target(CircuitBuilder& b) {
    return SignatureTarget{ecgfp5::add_virtual_biguint320_target(b), b.add_virtual_hash()};
}
// Constrains H(R' | pk | msg) = e for R' = s G + e (-pk).  The canonical 64-bit split_le of every challenge word is what makes
// e one integer: a 64-bit decomposition that only summed to the word modulo p would admit two bit strings for small words, and
// with them two different points e (-pk).  No new gate: two multiply_point (EcStepGate rows with ec_gate, arithmetic gates
// without), one add_point, one sponge.  NOT checked here: s < n (s and s + n, where it fits in 320 bits, give the same R': the
// native verifier refuses the second) and that pk is in the group (add_virtual_point_target checks the curve equation only): a
// circuit that takes pk as a public input relies on the native check outside.
// Returns R' (for tests and for callers that bind it).
inline ecgfp5::PointTarget verify_signature_target(CircuitBuilder& b, const ecgfp5::PointTarget& pk, const std::vector<Target>& msg, const SignatureTarget& sig) {
    if (sig.s_bits.size() != ecgfp5::SCALAR_BITS) throw std::runtime_error("verify_schnorr_signature takes 320 bits of s");
    if (msg.size() > MAX_MSG_LEN) throw std::runtime_error("verify_schnorr_signature: at most 1024 message words");
    std::vector<BoolTarget> e_bits;
    for (int i = 0; i < 4; i++) {
        const std::vector<BoolTarget> w = b.split_le(sig.e[i], 64);
        e_bits.insert(e_bits.end(), w.begin(), w.end());
    }
    const BoolTarget zero{b.zero()};
    e_bits.resize(ecgfp5::SCALAR_BITS, zero);
    ecgfp5::PointTarget npk = pk;
    for (auto& t : npk.u) t = b.mul_const(ecgfp5::NEG1, t);
    const ecgfp5::PointTarget sg = ecgfp5::multiply_point(b, sig.s_bits, ecgfp5::constant_point(b, ecgfp5::generator()));
    const ecgfp5::PointTarget r = ecgfp5::add_point(b, sg, ecgfp5::multiply_point(b, e_bits, npk));
    std::vector<Target> in(r.x.begin(), r.x.end());
    in.insert(in.end(), r.u.begin(), r.u.end());
    in.insert(in.end(), pk.x.begin(), pk.x.end());
    in.insert(in.end(), pk.u.begin(), pk.u.end());
    in.insert(in.end(), msg.begin(), msg.end());
    const std::vector<Target> h = b.hash_n_to_m_no_pad(in, 4);
    // h == e word by word as connect(h - e, 0), not connect_hashes(h, e): that would make the sponge a producer of e's slots, which
    // the bit hints of split_le read -- a witness program that waits on itself (builder.h assert_equal_to_input has the same reason)
    for (int i = 0; i < 4; i++) b.connect(b.sub(h[i], sig.e[i]), b.zero());
    return r;
}

}  // namespace schnorr
}  // namespace p2
