// Host half of the C ABI declared in include/p2aes.h: CircuitBuilder mirror, AES/GCM gadgets, native cipher,
// blob info and the verifier.  No device code here; the GPU prover lives in prover_gpu.hip.
#include <stdlib.h>

#include "../../include/p2aes.h"
#include "aes_gadgets.h"
#include "capi_common.h"
#include "compress.h"
#include "ecgfp5.h"
#include "merkle_host.h"
#define P2_PCIPHER_SPONGE_ONLY
#include "kernels_pcipher.h"
#include "poseidon_cipher.h"
#include "poseidon_fast.h"
#include "schnorr.h"
#include "verifier.h"
#include "witness_check.h"
#include "witness_schedule.h"

using namespace p2;

namespace p2 {
thread_local std::string g_last_error;
}

struct p2_builder {
    CircuitBuilder b;
};


// No exception may cross the C boundary: every entry point that runs builder / gadget code goes through one of these.
// The message lands in p2_last_error(); the return value is the function's error value (an error code, UINT64_MAX for a
// target, (size_t)-1 for an index; a void function leaves its outputs untouched).
template <class F>
static int guarded(F f) {
    try {
        f();
        return P2_OK;
    } catch (std::exception& e) {
        return set_error(e.what()), P2_ERR_INVALID;
    } catch (...) {
        return set_error("unknown C++ exception"), P2_ERR_INVALID;
    }
}
template <class F>
static p2_target guarded_t(F f) {
    p2_target r = UINT64_MAX;
    (void)guarded([&] { r = f(); });
    return r;
}
template <class F>
static size_t guarded_sz(F f) {
    size_t r = (size_t)-1;
    (void)guarded([&] { r = f(); });
    return r;
}

// verifier_data = constants_sigmas_cap || circuit_digest; false if vd_len does not fit the circuit
static bool read_verifier_data(const Circuit& c, const uint64_t* vd, size_t vd_len, VerifierData& v) {
    size_t cap_n = (size_t)1 << c.cfg.cap_height;
    if (!vd || vd_len != 4 * cap_n + 4) return false;
    v.constants_sigmas_cap.resize(cap_n);
    for (size_t i = 0; i < cap_n; i++) memcpy(v.constants_sigmas_cap[i].e, vd + 4 * i, 32);
    memcpy(v.circuit_digest.e, vd + 4 * cap_n, 32);
    return true;
}
// p2_proof_compress / p2_proof_decompress: one conversion of compress.h, its output copied to `out` when it fits
template <class F>
static int convert_proof(const uint8_t* blob, size_t blob_len, const uint64_t* vd, size_t vd_len, const uint8_t* in, size_t in_len, uint8_t* out,
                         size_t cap, size_t* n_written, F&& f) {
    try {
        if (n_written) *n_written = 0;
        Circuit c = deserialize(blob, blob_len);
        VerifierData v;
        if (!read_verifier_data(c, vd, vd_len, v)) return set_error("verifier_data must be cap || circuit_digest"), P2_ERR_INVALID;
        if (!in) return set_error("null proof"), P2_ERR_INVALID;
        std::vector<uint8_t> res;
        std::string err = f(c, v, in, in_len, res);
        if (!err.empty()) return set_error(err), P2_ERR_VERIFY;
        if (n_written) *n_written = res.size();
        if (!out || cap < res.size()) return set_error("output buffer holds fewer than " + std::to_string(res.size()) + " bytes"), P2_ERR_INVALID;
        memcpy(out, res.data(), res.size());
        return P2_OK;
    } catch (std::exception& e) {
        return set_error(e.what()), P2_ERR_INVALID;
    }
}
extern "C" {

const char* p2_last_error(void) { return p2::g_last_error.c_str(); }

p2_builder* p2_builder_new(void) { return new p2_builder(); }
p2_builder* p2_builder_new_zk(void) {
    Config cfg;
    cfg.zero_knowledge = 1;
    return new p2_builder{CircuitBuilder(cfg)};
}
p2_builder* p2_builder_new_config(int zero_knowledge, int hasher) {
    if (hasher != P2_HASHER_POSEIDON && hasher != P2_HASHER_KECCAK) return set_error("p2_builder_new_config: unknown hasher"), nullptr;
    Config cfg;
    cfg.zero_knowledge = zero_knowledge ? 1 : 0;
    cfg.hasher = (u32)hasher;
    return new p2_builder{CircuitBuilder(cfg)};
}
int p2_builder_set_hasher(p2_builder* b, int hasher) {
    if (!b || (hasher != P2_HASHER_POSEIDON && hasher != P2_HASHER_KECCAK)) return set_error("p2_builder_set_hasher: unknown hasher"), P2_ERR_INVALID;
    b->b.set_hasher((u32)hasher);
    return P2_OK;
}
void p2_builder_free(p2_builder* b) { delete b; }
p2_target p2_builder_add_virtual_target(p2_builder* b) { return guarded_t([&]() -> p2_target { return b->b.add_virtual_target(); }); }
p2_target p2_builder_constant(p2_builder* b, uint64_t c) { return guarded_t([&]() -> p2_target { return b->b.constant(c); }); }
p2_target p2_builder_zero(p2_builder* b) { return guarded_t([&]() -> p2_target { return b->b.zero(); }); }
p2_target p2_builder_one(p2_builder* b) { return guarded_t([&]() -> p2_target { return b->b.one(); }); }
p2_target p2_builder_arithmetic(p2_builder* b, uint64_t c0, uint64_t c1, p2_target m0, p2_target m1, p2_target a) { return guarded_t([&]() -> p2_target {    return b->b.arithmetic(c0 % gl::P, c1 % gl::P, m0, m1, a);}); }
p2_target p2_builder_mul_const_add(p2_builder* b, uint64_t c, p2_target x, p2_target y) { return guarded_t([&]() -> p2_target { return b->b.mul_const_add(c % gl::P, x, y); }); }
p2_target p2_builder_add(p2_builder* b, p2_target x, p2_target y) { return guarded_t([&]() -> p2_target { return b->b.add(x, y); }); }
p2_target p2_builder_sub(p2_builder* b, p2_target x, p2_target y) { return guarded_t([&]() -> p2_target { return b->b.sub(x, y); }); }
p2_target p2_builder_mul(p2_builder* b, p2_target x, p2_target y) { return guarded_t([&]() -> p2_target { return b->b.mul(x, y); }); }
p2_target p2_builder_select(p2_builder* b, p2_target c, p2_target x, p2_target y) { return guarded_t([&]() -> p2_target { return b->b.select(BoolTarget{c}, x, y); }); }
p2_target p2_builder_is_equal(p2_builder* b, p2_target x, p2_target y) { return guarded_t([&]() -> p2_target { return b->b.is_equal(x, y).target; }); }
void p2_builder_connect(p2_builder* b, p2_target x, p2_target y) { (void)guarded([&] { b->b.connect(x, y); }); }
int p2_builder_register_public_input(p2_builder* b, p2_target t) { return guarded([&] { b->b.register_public_input(t); }); }
size_t p2_builder_add_lookup_table_from_pairs(p2_builder* b, const uint16_t* pairs, size_t n) {
    return guarded_sz([&]() -> size_t {
        std::vector<std::pair<u16, u16>> t(n);
        for (size_t i = 0; i < n; i++) t[i] = {pairs[2 * i], pairs[2 * i + 1]};
        return b->b.add_lookup_table_from_pairs(t);
    });
}
p2_target p2_builder_add_lookup_from_index(p2_builder* b, p2_target in, size_t lut) {
    try {
        return b->b.add_lookup_from_index(in, lut);
    } catch (std::exception& e) {
        set_error(e.what());
        return UINT64_MAX;
    }
}
int p2_builder_assert_bool(p2_builder* b, p2_target t) { return guarded([&] { b->b.assert_bool(t); }); }
int p2_builder_le_sum(p2_builder* b, const p2_target* bits, size_t n, p2_target* out) {
    return guarded([&] {
        std::vector<BoolTarget> v(n);
        for (size_t i = 0; i < n; i++) v[i] = BoolTarget{bits[i]};
        *out = b->b.le_sum(v);
    });
}
int p2_builder_split_le(p2_builder* b, p2_target x, size_t num_bits, p2_target* bits) {
    return guarded([&] {
        auto v = b->b.split_le(x, num_bits);
        for (size_t i = 0; i < v.size(); i++) bits[i] = v[i].target;
    });
}
int p2_builder_range_check(p2_builder* b, p2_target x, size_t num_bits) { return guarded([&] { b->b.range_check(x, num_bits); }); }
int p2_builder_le_bytes_sum(p2_builder* b, const p2_target* bytes, size_t n, p2_target* out) {
    return guarded([&] { *out = b->b.le_bytes_sum(std::vector<Target>(bytes, bytes + n)); });
}
int p2_builder_split_bytes_le(p2_builder* b, p2_target x, size_t num_bytes, size_t u8_table_idx, p2_target* bytes) {
    return guarded([&] {
        auto v = b->b.split_bytes_le(x, num_bytes, u8_table_idx);
        std::copy(v.begin(), v.end(), bytes);
    });
}
int p2_builder_is_less_than(p2_builder* b, p2_target x, p2_target y, size_t num_bits, p2_target* out) {
    return guarded([&] { *out = b->b.is_less_than(x, y, num_bits).target; });
}
int p2_builder_set_ec_gate(p2_builder* b, int on) {
    if (!b) return set_error("p2_builder_set_ec_gate: null builder"), P2_ERR_INVALID;
    b->b.set_ec_gate(on != 0);
    return P2_OK;
}
int p2_builder_ec_step(p2_builder* b, const p2_target acc[20], const p2_target q[10], p2_target bit, int hinted, p2_target mid[20], p2_target out[20]) {
    if (!b || !acc || !q || !mid || !out) return set_error("p2_builder_ec_step: null argument"), P2_ERR_INVALID;
    return guarded([&] {
        std::array<Target, 20> a;
        std::array<Target, 10> qq;
        std::copy(acc, acc + 20, a.begin());
        std::copy(q, q + 10, qq.begin());
        const CircuitBuilder::EcStep st = b->b.ec_step(a, qq, bit, hinted != 0);
        std::copy(st.mid.begin(), st.mid.end(), mid);
        std::copy(st.out.begin(), st.out.end(), out);
    });
}
int p2_builder_set_ghash_tables(p2_builder* b, int lanes) {
    if (!b) return set_error("p2_builder_set_ghash_tables: null builder"), P2_ERR_INVALID;
    return guarded([&] { b->b.set_ghash_tables(lanes); });
}
size_t p2_builder_num_gates(const p2_builder* b) { return guarded_sz([&]() -> size_t { return b->b.num_gates(); }); }
int p2_builder_build(p2_builder* b, uint8_t** blob, size_t* len) {
    try {
        Circuit c = b->b.build();
        std::vector<uint8_t> v = serialize(c);
        uint8_t* out = (uint8_t*)malloc(v.size());
        if (!out) return set_error("out of memory"), P2_ERR_INVALID;
        memcpy(out, v.data(), v.size());
        *blob = out;
        *len = v.size();
        return P2_OK;
    } catch (std::exception& e) {
        return set_error(e.what()), P2_ERR_INVALID;
    }
}
void p2_blob_free(uint8_t* blob) { free(blob); }

// ---- gadgets
static aes::StateTarget state_in(const p2_target* s) {
    aes::StateTarget st;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) st[i][j] = s[4 * i + j];
    return st;
}
static void state_out(const aes::StateTarget& st, p2_target* o) {
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) o[4 * i + j] = st[i][j];
}
static std::vector<aes::WordTarget> words_in(const p2_target* w, size_t n) {
    std::vector<aes::WordTarget> v(n);
    for (size_t i = 0; i < n; i++)
        for (int j = 0; j < 4; j++) v[i][j] = w[4 * i + j];
    return v;
}
static aes::BlockTarget block_in(const p2_target* b) {
    aes::BlockTarget r;
    for (int i = 0; i < 16; i++) r[i] = b[i];
    return r;
}
size_t p2_aes_sbox_lut(p2_builder* b) { return guarded_sz([&]() -> size_t { return aes::sbox_lut(b->b); }); }
size_t p2_aes_byte_xor_lut(p2_builder* b) { return guarded_sz([&]() -> size_t { return aes::byte_xor_lut(b->b); }); }
size_t p2_aes_gf_2_8_mul_lut(p2_builder* b) { return guarded_sz([&]() -> size_t { return aes::gf_2_8_mul_lut(b->b); }); }
size_t p2_gcm_u8_unit_right_shift_lut(p2_builder* b) { return guarded_sz([&]() -> size_t { return aes::u8_unit_right_shift_lut(b->b); }); }
size_t p2_gcm_u8_bitref_lut(p2_builder* b) { return guarded_sz([&]() -> size_t { return aes::u8_bitref_lut(b->b); }); }
size_t p2_gcm_clmul_lo_lut(p2_builder* b) { return guarded_sz([&]() -> size_t { return aes::gcm_clmul_lo_lut(b->b); }); }
size_t p2_gcm_clmul_hi_lut(p2_builder* b) { return guarded_sz([&]() -> size_t { return aes::gcm_clmul_hi_lut(b->b); }); }
p2_target p2_aes_add_virtual_byte_target(p2_builder* b, size_t t) {
    try {
        return aes::add_virtual_byte_target(b->b, t);
    } catch (std::exception& e) {
        set_error(e.what());
        return UINT64_MAX;
    }
}
p2_target p2_aes_add_virtual_byte_target_unsafe(p2_builder* b) { return guarded_t([&]() -> p2_target { return aes::add_virtual_byte_target_unsafe(b->b); }); }
void p2_aes_state_sub_bytes(p2_builder* b, size_t sbox, const p2_target* s, p2_target* out) { (void)guarded([&] { state_out(aes::state_sub_bytes(b->b, sbox, state_in(s)), out); }); }
void p2_aes_state_mix_columns(p2_builder* b, size_t xl, size_t ml, const p2_target* s, p2_target* out) {
    (void)guarded([&] {
        aes::StateTarget mix = aes::state_mix_matrix(b->b);
        state_out(aes::state_mix_columns(b->b, xl, ml, mix, state_in(s)), out);
    });
}
p2_target p2_aes_gf_2_8_mul(p2_builder* b, size_t ml, p2_target x, p2_target y) { return guarded_t([&]() -> p2_target { return aes::gf_2_8_mul_t(b->b, ml, x, y); }); }
p2_target p2_aes_gf_2_8_add(p2_builder* b, size_t xl, p2_target x, p2_target y) { return guarded_t([&]() -> p2_target { return aes::gf_2_8_add(b->b, xl, x, y); }); }
void p2_aes_key_expansion(p2_builder* b, int nk, int nr, size_t xl, size_t sl, const p2_target* key, p2_target* out) {
    (void)guarded([&] {
        std::vector<aes::ByteTarget> k(key, key + 4 * nk);
        auto w = aes::key_expansion_t(b->b, nk, nr, xl, sl, k);
        for (size_t i = 0; i < w.size(); i++)
            for (int j = 0; j < 4; j++) out[4 * i + j] = w[i][j];
    });
}
void p2_aes_encrypt_block(p2_builder* b, int nr, size_t xl, size_t ml, size_t sl, const p2_target* state, const p2_target* ek, p2_target* out) {
    (void)guarded([&] {
        aes::StateTarget mix = aes::state_mix_matrix(b->b);
        state_out(aes::encrypt_block_t(b->b, nr, xl, ml, sl, mix, state_in(state), words_in(ek, 4 * (nr + 1))), out);
    });
}
void p2_gcm_gctr(p2_builder* b, int nr, size_t xl, size_t ml, size_t sl, const p2_target* ek, const p2_target* icb, const p2_target* x, size_t len, p2_target* y) {
    (void)guarded([&] {
        aes::StateTarget mix = aes::state_mix_matrix(b->b);
        std::vector<aes::ByteTarget> xv(x, x + len);
        auto r = aes::gctr_target(b->b, nr, xl, ml, sl, mix, words_in(ek, 4 * (nr + 1)), block_in(icb), xv);
        for (size_t i = 0; i < len; i++) y[i] = r[i];
    });
}
void p2_gcm_right_shift_one(p2_builder* b, size_t shl, const p2_target* v, p2_target* out) {
    (void)guarded([&] {
        auto r = aes::right_shift_one_target(b->b, shl, block_in(v));
        for (int i = 0; i < 16; i++) out[i] = r[i];
    });
}
void p2_gcm_inc32(p2_builder* b, const p2_target* blk, p2_target* out) {
    (void)guarded([&] {
        auto r = aes::inc32_target(b->b, block_in(blk));
        for (int i = 0; i < 16; i++) out[i] = r[i];
    });
}
void p2_gcm_gf_2_128_mul(p2_builder* b, size_t xl, size_t shl, size_t brl, const p2_target* x, const p2_target* y, p2_target* out) {
    (void)guarded([&] {
        auto r = aes::gf_2_128_mul_target(b->b, xl, shl, brl, block_in(x), block_in(y));
        for (int i = 0; i < 16; i++) out[i] = r[i];
    });
}
int p2_gcm_ghash(p2_builder* b, size_t xl, size_t shl, size_t brl, const p2_target* h, const p2_target* x, size_t len, p2_target* out) {
    try {
        std::vector<aes::ByteTarget> xv(x, x + len);
        auto r = aes::ghash_target(b->b, xl, shl, brl, block_in(h), xv);
        for (int i = 0; i < 16; i++) out[i] = r[i];
        return P2_OK;
    } catch (std::exception& e) {
        return set_error(e.what()), P2_ERR_INVALID;
    }
}
int p2_gcm_gf_2_128_mul_tables(p2_builder* b, size_t xl, size_t lol, size_t hil, const p2_target* x, const p2_target* y, p2_target* out) {
    if (!b || !x || !y || !out) return set_error("p2_gcm_gf_2_128_mul_tables: null argument"), P2_ERR_INVALID;
    return guarded([&] {
        auto r = aes::gf_2_128_mul_tables_target(b->b, xl, lol, hil, block_in(x), block_in(y));
        for (int i = 0; i < 16; i++) out[i] = r[i];
    });
}
int p2_gcm_ghash_tables(p2_builder* b, size_t xl, size_t lol, size_t hil, const p2_target* h, const p2_target* x, size_t len, p2_target* out, int lanes) {
    if (!b || !h || (len && !x) || !out) return set_error("p2_gcm_ghash_tables: null argument"), P2_ERR_INVALID;
    return guarded([&] {
        std::vector<aes::ByteTarget> xv(x, x + len);
        auto r = aes::ghash_tables_target(b->b, xl, lol, hil, block_in(h), xv, lanes);
        for (int i = 0; i < 16; i++) out[i] = r[i];
    });
}
int p2_aes_gcm_build(p2_builder* b, int nk, int nr, size_t L, int with_tag, p2_target* key, p2_target* nonce, p2_target* pt, p2_target* ct, p2_target* tag) {
    return p2_aes_gcm_build_aad(b, nk, nr, L, with_tag, 0, key, nonce, pt, ct, tag, nullptr);
}
int p2_aes_gcm_build_aad(p2_builder* b, int nk, int nr, size_t L, int with_tag, size_t aad_len, p2_target* key, p2_target* nonce, p2_target* pt, p2_target* ct,
                         p2_target* tag, p2_target* aad) {
    if (!((nk == 4 && nr == 10) || (nk == 6 && nr == 12) || (nk == 8 && nr == 14))) return set_error("unsupported (NK, NR)"), P2_ERR_INVALID;
    if (aad_len && !with_tag) return set_error("aad needs the tag"), P2_ERR_INVALID;
    if (aad_len && !aad) return set_error("p2_aes_gcm_build_aad: null argument"), P2_ERR_INVALID;
    try {
        auto t = aes::AesGcmTarget::build(b->b, nk, nr, L, with_tag != 0, aad_len);
        std::copy(t.aad.begin(), t.aad.end(), aad);
        std::copy(t.key.begin(), t.key.end(), key);
        std::copy(t.nonce.begin(), t.nonce.end(), nonce);
        std::copy(t.pt.begin(), t.pt.end(), pt);
        std::copy(t.ct.begin(), t.ct.end(), ct);
        std::copy(t.tag.begin(), t.tag.end(), tag);
        return P2_OK;
    } catch (std::exception& e) {
        return set_error(e.what()), P2_ERR_INVALID;
    }
}

// ---- Poseidon hashing / poseidon-cipher
int p2_builder_hash_n_to_m_no_pad(p2_builder* b, const p2_target* inputs, size_t n, p2_target* outputs, size_t m) {
    try {
        auto o = b->b.hash_n_to_m_no_pad(std::vector<Target>(inputs, inputs + n), m);
        std::copy(o.begin(), o.end(), outputs);
        return P2_OK;
    } catch (std::exception& e) {
        return set_error(e.what()), P2_ERR_INVALID;
    }
}
// ---- Merkle membership
static CircuitBuilder::HashOutTarget hash_at(const p2_target* h) { return CircuitBuilder::HashOutTarget{h[0], h[1], h[2], h[3]}; }
static std::vector<CircuitBuilder::HashOutTarget> hashes_at(const p2_target* h, size_t n) {
    std::vector<CircuitBuilder::HashOutTarget> v(n);
    for (size_t i = 0; i < n; i++) v[i] = hash_at(h + 4 * i);
    return v;
}
int p2_builder_permute_swapped(p2_builder* b, const p2_target inputs[12], p2_target swap, p2_target out[12]) {
    return guarded([&] {
        std::array<Target, 12> in;
        std::copy(inputs, inputs + 12, in.begin());
        auto o = b->b.permute_swapped(in, BoolTarget{swap});
        std::copy(o.begin(), o.end(), out);
    });
}
int p2_builder_hash_or_noop(p2_builder* b, const p2_target* inputs, size_t n, p2_target out[4]) {
    return guarded([&] {
        auto h = b->b.hash_or_noop(std::vector<Target>(inputs, inputs + n));
        std::copy(h.begin(), h.end(), out);
    });
}
int p2_builder_add_virtual_hash(p2_builder* b, p2_target out[4]) {
    return guarded([&] {
        auto h = b->b.add_virtual_hash();
        std::copy(h.begin(), h.end(), out);
    });
}
int p2_builder_add_virtual_cap(p2_builder* b, int cap_height, p2_target* out) {
    return guarded([&] {
        if (cap_height < 0) throw std::runtime_error("add_virtual_cap: cap_height must be 0 to 16");
        auto cap = b->b.add_virtual_cap((u32)cap_height);
        for (size_t i = 0; i < cap.size(); i++) std::copy(cap[i].begin(), cap[i].end(), out + 4 * i);
    });
}
int p2_builder_connect_hashes(p2_builder* b, const p2_target x[4], const p2_target y[4]) {
    return guarded([&] { b->b.connect_hashes(hash_at(x), hash_at(y)); });
}
int p2_builder_verify_merkle_proof_to_cap(p2_builder* b, const p2_target* leaf, size_t leaf_len, const p2_target* index_bits, size_t n_bits, const p2_target* cap,
                                          int cap_height, const p2_target* siblings, size_t n_siblings) {
    return guarded([&] {
        if (cap_height < 0 || cap_height > 16) throw std::runtime_error("verify_merkle_proof_to_cap: cap_height must be 0 to 16");
        std::vector<BoolTarget> bits(n_bits);
        for (size_t i = 0; i < n_bits; i++) bits[i] = BoolTarget{index_bits[i]};
        b->b.verify_merkle_proof_to_cap(std::vector<Target>(leaf, leaf + leaf_len), bits, hashes_at(cap, (size_t)1 << cap_height), hashes_at(siblings, n_siblings));
    });
}
int p2_builder_verify_merkle_proof(p2_builder* b, const p2_target* leaf, size_t leaf_len, const p2_target* index_bits, size_t n_bits, const p2_target root[4],
                                   const p2_target* siblings, size_t n_siblings) {
    return p2_builder_verify_merkle_proof_to_cap(b, leaf, leaf_len, index_bits, n_bits, root, 0, siblings, n_siblings);
}
int p2_builder_merkle_update_to_cap(p2_builder* b, const p2_target* old_leaf, const p2_target* new_leaf, size_t leaf_len, const p2_target* index_bits, size_t n_bits,
                                    const p2_target* old_cap, int cap_height, const p2_target* siblings, size_t n_siblings, p2_target* new_cap) {
    return guarded([&] {
        if (cap_height < 0 || cap_height > 16) throw std::runtime_error("merkle_update_to_cap: cap_height must be 0 to 16");
        std::vector<BoolTarget> bits(n_bits);
        for (size_t i = 0; i < n_bits; i++) bits[i] = BoolTarget{index_bits[i]};
        auto cap = b->b.merkle_update_to_cap(std::vector<Target>(old_leaf, old_leaf + leaf_len), std::vector<Target>(new_leaf, new_leaf + leaf_len), bits,
                                             hashes_at(old_cap, (size_t)1 << cap_height), hashes_at(siblings, n_siblings));
        for (size_t i = 0; i < cap.size(); i++) std::copy(cap[i].begin(), cap[i].end(), new_cap + 4 * i);
    });
}
int p2_builder_merkle_update(p2_builder* b, const p2_target* old_leaf, const p2_target* new_leaf, size_t leaf_len, const p2_target* index_bits, size_t n_bits,
                             const p2_target old_root[4], const p2_target* siblings, size_t n_siblings, p2_target new_root[4]) {
    return p2_builder_merkle_update_to_cap(b, old_leaf, new_leaf, leaf_len, index_bits, n_bits, old_root, 0, siblings, n_siblings, new_root);
}
// Native trees on the host (merkle_host.h): the twin of the p2_merkle_tree_* calls for the CPU suite
int p2_native_merkle_cap(const uint64_t* leaves, size_t num_leaves, size_t leaf_len, int cap_height, uint64_t* cap) {
    return guarded([&] {
        mt::HostTree t(leaves, num_leaves, leaf_len, cap_height);
        const auto& top = t.levels[t.bits - t.cap_height];
        memcpy(cap, top.data(), top.size() * sizeof(Hash4));
    });
}
int p2_native_merkle_prove(const uint64_t* leaves, size_t num_leaves, size_t leaf_len, int cap_height, size_t index, uint64_t* siblings) {
    return guarded([&] {
        mt::HostTree t(leaves, num_leaves, leaf_len, cap_height);
        if (index >= num_leaves) throw std::runtime_error("leaf index " + std::to_string(index) + " is not below num_leaves");
        for (u32 l = 0; l < t.bits - t.cap_height; l++) memcpy(siblings + 4 * l, t.levels[l][(index >> l) ^ 1].e, 32);
    });
}
int p2_native_merkle_update(uint64_t* leaves, size_t num_leaves, size_t leaf_len, int cap_height, const uint64_t* indices, const uint64_t* new_leaves, size_t k,
                            uint64_t* siblings, uint64_t* root_after) {
    return guarded([&] {
        mt::HostTree t(leaves, num_leaves, leaf_len, cap_height);
        if (k == 0) return;
        if (!indices || !new_leaves) throw std::runtime_error("null argument");
        const std::string bad = mt::first_bad_item(indices, new_leaves, k, num_leaves, leaf_len);
        if (!bad.empty()) throw std::runtime_error(bad);
        mt::host_update(t, leaf_len, indices, new_leaves, k, siblings, root_after);
        for (size_t j = 0; j < k; j++) memcpy(leaves + indices[j] * leaf_len, new_leaves + j * leaf_len, 8 * leaf_len);
    });
}
int p2_native_merkle_verify(const uint64_t* leaf, size_t leaf_len, size_t index, const uint64_t* siblings, size_t depth, const uint64_t* cap, int cap_height,
                            int* status) {
    return guarded([&] {
        if (!leaf || !cap || !status || (depth && !siblings)) throw std::runtime_error("null argument");
        if (leaf_len < 1 || leaf_len > 0xFFFFFFFFull || cap_height < 0 || cap_height > 16 || depth + (size_t)cap_height > 32)
            throw std::runtime_error("leaf_len >= 1, cap_height 0 to 16, siblings + cap_height at most 32");
        *status = mt::host_verify(leaf, leaf_len, index, siblings, depth, cap, (u32)cap_height);
    });
}
// ---- sparse keyed trees: the gadgets (builder.h) and the host twin (merkle_host.h)
static std::vector<BoolTarget> bools_at(const p2_target* t, size_t n) {
    std::vector<BoolTarget> v(n);
    for (size_t i = 0; i < n; i++) v[i] = BoolTarget{t[i]};
    return v;
}
static std::vector<Target> targets_at(const p2_target* t, size_t n) { return n ? std::vector<Target>(t, t + n) : std::vector<Target>(); }
static void map_cap_height(const char* who, int cap_height) {
    if (cap_height < 0 || cap_height > 16) throw std::runtime_error(std::string(who) + ": cap_height must be 0 to 16");
}
static void cap_out(const std::vector<CircuitBuilder::HashOutTarget>& cap, p2_target* out) {
    for (size_t i = 0; i < cap.size(); i++) std::copy(cap[i].begin(), cap[i].end(), out + 4 * i);
}
int p2_builder_merkle_map_lookup_to_cap(p2_builder* b, const p2_target* key_bits, size_t n_bits, const p2_target* value, size_t value_len, p2_target present,
                                        const p2_target* cap, int cap_height, const p2_target* siblings, size_t n_siblings) {
    return guarded([&] {
        map_cap_height("merkle_map_lookup_to_cap", cap_height);
        b->b.merkle_map_lookup_to_cap(bools_at(key_bits, n_bits), targets_at(value, value_len), BoolTarget{present}, hashes_at(cap, (size_t)1 << cap_height),
                                      hashes_at(siblings, n_siblings));
    });
}
int p2_builder_merkle_map_lookup(p2_builder* b, const p2_target* key_bits, size_t n_bits, const p2_target* value, size_t value_len, p2_target present,
                                 const p2_target root[4], const p2_target* siblings, size_t n_siblings) {
    return p2_builder_merkle_map_lookup_to_cap(b, key_bits, n_bits, value, value_len, present, root, 0, siblings, n_siblings);
}
int p2_builder_merkle_map_update_to_cap(p2_builder* b, const p2_target* key_bits, size_t n_bits, p2_target old_present, const p2_target* old_value, p2_target new_present,
                                        const p2_target* new_value, size_t value_len, const p2_target* old_cap, int cap_height, const p2_target* siblings,
                                        size_t n_siblings, p2_target* new_cap) {
    return guarded([&] {
        map_cap_height("merkle_map_update_to_cap", cap_height);
        cap_out(b->b.merkle_map_update_to_cap(bools_at(key_bits, n_bits), BoolTarget{old_present}, targets_at(old_value, value_len), BoolTarget{new_present},
                                              targets_at(new_value, value_len), hashes_at(old_cap, (size_t)1 << cap_height), hashes_at(siblings, n_siblings)),
                new_cap);
    });
}
int p2_builder_merkle_map_update(p2_builder* b, const p2_target* key_bits, size_t n_bits, p2_target old_present, const p2_target* old_value, p2_target new_present,
                                 const p2_target* new_value, size_t value_len, const p2_target old_root[4], const p2_target* siblings, size_t n_siblings,
                                 p2_target new_root[4]) {
    return p2_builder_merkle_map_update_to_cap(b, key_bits, n_bits, old_present, old_value, new_present, new_value, value_len, old_root, 0, siblings, n_siblings, new_root);
}
int p2_builder_merkle_map_insert_to_cap(p2_builder* b, const p2_target* key_bits, size_t n_bits, const p2_target* value, size_t value_len, const p2_target* old_cap,
                                        int cap_height, const p2_target* siblings, size_t n_siblings, p2_target* new_cap) {
    return guarded([&] {
        map_cap_height("merkle_map_insert_to_cap", cap_height);
        cap_out(b->b.merkle_map_insert_to_cap(bools_at(key_bits, n_bits), targets_at(value, value_len), hashes_at(old_cap, (size_t)1 << cap_height),
                                              hashes_at(siblings, n_siblings)),
                new_cap);
    });
}
int p2_builder_merkle_map_insert(p2_builder* b, const p2_target* key_bits, size_t n_bits, const p2_target* value, size_t value_len, const p2_target old_root[4],
                                 const p2_target* siblings, size_t n_siblings, p2_target new_root[4]) {
    return p2_builder_merkle_map_insert_to_cap(b, key_bits, n_bits, value, value_len, old_root, 0, siblings, n_siblings, new_root);
}
int p2_builder_merkle_map_remove_to_cap(p2_builder* b, const p2_target* key_bits, size_t n_bits, const p2_target* value, size_t value_len, const p2_target* old_cap,
                                        int cap_height, const p2_target* siblings, size_t n_siblings, p2_target* new_cap) {
    return guarded([&] {
        map_cap_height("merkle_map_remove_to_cap", cap_height);
        cap_out(b->b.merkle_map_remove_to_cap(bools_at(key_bits, n_bits), targets_at(value, value_len), hashes_at(old_cap, (size_t)1 << cap_height),
                                              hashes_at(siblings, n_siblings)),
                new_cap);
    });
}
int p2_builder_merkle_map_remove(p2_builder* b, const p2_target* key_bits, size_t n_bits, const p2_target* value, size_t value_len, const p2_target old_root[4],
                                 const p2_target* siblings, size_t n_siblings, p2_target new_root[4]) {
    return p2_builder_merkle_map_remove_to_cap(b, key_bits, n_bits, value, value_len, old_root, 0, siblings, n_siblings, new_root);
}
int p2_native_merkle_map_cap(const uint64_t* keys, const uint64_t* values, size_t n, size_t value_len, int key_bits, int cap_height, uint64_t* cap) {
    return guarded([&] {
        mt::HostMap m(keys, values, n, value_len, key_bits, cap_height);
        if (!cap) throw std::runtime_error("null argument");
        m.cap(cap);
    });
}
int p2_native_merkle_map_get(const uint64_t* keys, const uint64_t* values, size_t n, size_t value_len, int key_bits, int cap_height, uint64_t key, int* present,
                             uint64_t* value, uint64_t* siblings) {
    return guarded([&] {
        mt::HostMap m(keys, values, n, value_len, key_bits, cap_height);
        if (!present || (value_len && !value) || (m.depth() && !siblings)) throw std::runtime_error("null argument");
        if (!mt::map_key_ok(key, m.D)) throw std::runtime_error("the key is not below 2^key_bits and p");
        const ptrdiff_t at = m.find(key);
        *present = at >= 0;
        for (size_t w = 0; w < value_len; w++) value[w] = at >= 0 ? values[m.pos[(size_t)at] * value_len + w] : 0;
        m.siblings(key, siblings);
    });
}
int p2_native_merkle_map_verify(uint64_t key, int key_bits, uint64_t present, const uint64_t* value, size_t value_len, const uint64_t* siblings, const uint64_t* cap,
                                int cap_height, int* status) {
    return guarded([&] {
        mt::map_check_shape(key_bits, cap_height, value_len);
        if (!cap || !status || (value_len && !value) || (key_bits > cap_height && !siblings)) throw std::runtime_error("null argument");
        *status = mt::host_map_verify(key, (u32)key_bits, present, value, value_len, siblings, cap, (u32)cap_height);
    });
}
int p2_poseidon_cipher_build(p2_builder* b, size_t L, p2_target* ks, p2_target* m, p2_target* nonce, p2_target* ct) {
    try {
        auto t = pcipher::PoseidonEncryptTarget::build(b->b, L);
        for (int i = 0; i < 5; i++) {
            ks[i] = t.ks_x[i];
            ks[5 + i] = t.ks_u[i];
        }
        for (size_t i = 0; i < L; i++)
            for (int j = 0; j < 5; j++) m[5 * i + j] = t.m[i][j];
        nonce[0] = t.nonce[0];
        nonce[1] = t.nonce[1];
        for (size_t i = 0; i <= L; i++)
            for (int j = 0; j < 5; j++) ct[5 * i + j] = t.ct[i][j];
        return P2_OK;
    } catch (std::exception& e) {
        return set_error(e.what()), P2_ERR_INVALID;
    }
}
static pcipher::FqT fqt_at(const p2_target* p) { return pcipher::FqT{(Target)p[0], (Target)p[1], (Target)p[2], (Target)p[3], (Target)p[4]}; }
// the two cipher gadgets share one call shape: `in` and `out` are the message and the ciphertext, in this or the other order
static int pcipher_gadget(p2_builder* b, bool decrypt, const p2_target* ks, const p2_target* nonce, const p2_target* in, size_t L, p2_target* out) {
    try {
        if (!b || !ks || !nonce || !in || !out) throw std::runtime_error("null argument");
        if (L % 3 != 0) throw std::runtime_error("L must be a multiple of 3");
        const Target n[2] = {(Target)nonce[0], (Target)nonce[1]};
        std::vector<pcipher::FqT> v(decrypt ? L + 1 : L);
        for (size_t i = 0; i < v.size(); i++) v[i] = fqt_at(in + 5 * i);
        const auto o = decrypt ? pcipher::poseidon_decrypt(b->b, fqt_at(ks), fqt_at(ks + 5), n, v) : pcipher::poseidon_encrypt(b->b, fqt_at(ks), fqt_at(ks + 5), n, v);
        for (size_t i = 0; i < o.size(); i++)
            for (int j = 0; j < 5; j++) out[5 * i + j] = o[i][j];
        return P2_OK;
    } catch (std::exception& e) {
        return set_error(e.what()), P2_ERR_INVALID;
    }
}
int p2_builder_poseidon_encrypt(p2_builder* b, const p2_target ks[10], const p2_target nonce[2], const p2_target* m, size_t L, p2_target* ct) {
    return pcipher_gadget(b, false, ks, nonce, m, L, ct);
}
int p2_builder_poseidon_decrypt(p2_builder* b, const p2_target ks[10], const p2_target nonce[2], const p2_target* ct, size_t L, p2_target* m) {
    return pcipher_gadget(b, true, ks, nonce, ct, L, m);
}
void p2_native_hash_n_to_m_no_pad(const uint64_t* in, size_t n, uint64_t* out, size_t m) {
    (void)guarded([&] {
        auto o = pcipher::hash_n_to_m_no_pad(std::vector<u64>(in, in + n), m);
        std::copy(o.begin(), o.end(), out);
    });
}
void p2_native_keccak_hash_no_pad(const uint64_t* in, size_t n, uint64_t out[4]) { kc::hash_no_pad(in, (u32)n, out); }
void p2_native_keccak_two_to_one(const uint64_t l[4], const uint64_t r[4], uint64_t out[4]) { kc::two_to_one(l, r, out); }
void p2_native_keccak256(const uint8_t* data, size_t len, uint8_t out[32]) { memcpy(out, kc::keccak256(data, len).data(), 32); }
static pcipher::Fq fq_at(const uint64_t* p) { return pcipher::Fq{p[0], p[1], p[2], p[3], p[4]}; }
void p2_native_poseidon_encrypt(const uint64_t* ks, const uint64_t* msg, size_t n_msg, const uint64_t* nonce, uint64_t* ct) {
    (void)guarded([&] {
        std::vector<pcipher::Fq> m(n_msg);
        for (size_t i = 0; i < n_msg; i++) m[i] = fq_at(msg + 5 * i);
        auto c = pcipher::encrypt(fq_at(ks), fq_at(ks + 5), m, nonce);
        for (size_t i = 0; i < c.size(); i++) memcpy(ct + 5 * i, c[i].data(), 40);
    });
}
int p2_native_poseidon_decrypt(const uint64_t* ks, const uint64_t* ct, size_t n_ct, const uint64_t* nonce, size_t l, uint64_t* msg) {
    // pcipher::decrypt walks whole blocks of three: any other shape would write past m, and the reference panics there
    if (n_ct % 3 != 1) return set_error("poseidon decrypt: a ciphertext has 3 k + 1 elements"), P2_ERR_INVALID;
    std::vector<pcipher::Fq> c(n_ct), m;
    for (size_t i = 0; i < n_ct; i++) c[i] = fq_at(ct + 5 * i);
    if ( l > n_ct - 1 || !pcipher::decrypt(fq_at(ks), fq_at(ks + 5), c, nonce, l, &m)) return set_error("poseidon decrypt: authentication failed"), P2_ERR_VERIFY;
    for (size_t i = 0; i < m.size(); i++) memcpy(msg + 5 * i, m[i].data(), 40);
    return P2_OK;
}

// ---- ecGFp5
static ecgfp5::Affine pt_at(const uint64_t* p) { return ecgfp5::Affine{fq_at(p), fq_at(p + 5)}; }
static void pt_put(const ecgfp5::Affine& a, uint64_t* out) {
    memcpy(out, a.x.data(), 40);
    memcpy(out + 5, a.u.data(), 40);
}
static ecgfp5::U320 sc_at(const uint64_t* k) {
    ecgfp5::U320 s;
    memcpy(s.w, k, 40);
    return s;
}
static void ptt_put(const ecgfp5::PointTarget& p, p2_target* out) {
    for (int i = 0; i < 5; i++) out[i] = p.x[i], out[5 + i] = p.u[i];
}
static ecgfp5::PointTarget ptt_at(const p2_target* p) {
    ecgfp5::PointTarget t;
    for (int i = 0; i < 5; i++) t.x[i] = p[i], t.u[i] = p[5 + i];
    return t;
}
static std::vector<BoolTarget> bits_at(const p2_target* bits) {
    std::vector<BoolTarget> v(ecgfp5::SCALAR_BITS);
    for (size_t i = 0; i < v.size(); i++) v[i] = BoolTarget{bits[i]};
    return v;
}
static int scalar_ok(const uint64_t* k) {
    if (!ecgfp5::u320_lt(sc_at(k), ecgfp5::GROUP_ORDER)) return set_error("scalar is not below the group order"), P2_ERR_INVALID;
    return P2_OK;
}
void p2_ecgfp5_group_order(uint64_t out[5]) { (void)guarded([&] { memcpy(out, ecgfp5::GROUP_ORDER.w, 40); }); }
void p2_ecgfp5_generator(uint64_t out[10]) { (void)guarded([&] { pt_put(ecgfp5::generator(), out); }); }
void p2_ecgfp5_mul(const uint64_t k[5], const uint64_t p[10], uint64_t out[10]) { (void)guarded([&] { pt_put(ecgfp5::scalar_mul(sc_at(k), pt_at(p)), out); }); }
void p2_ecgfp5_add(const uint64_t p[10], const uint64_t q[10], uint64_t out[10]) { (void)guarded([&] { pt_put(ecgfp5::point_add(pt_at(p), pt_at(q)), out); }); }
void p2_ecgfp5_neg(const uint64_t p[10], uint64_t out[10]) { (void)guarded([&] { pt_put(ecgfp5::point_neg(pt_at(p)), out); }); }
int p2_ecgfp5_is_in_subgroup(const uint64_t p[10]) { return ecgfp5::is_in_subgroup(pt_at(p)) ? 1 : 0; }
void p2_ecgfp5_compress(const uint64_t p[10], uint64_t w[5]) { (void)guarded([&] { memcpy(w, ecgfp5::compress_from_subgroup(pt_at(p)).data(), 40); }); }
int p2_ecgfp5_decompress(const uint64_t w[5], uint64_t out[10]) {
    ecgfp5::Affine a;
    if (!ecgfp5::decompress_into_subgroup(fq_at(w), &a)) return set_error("not the encoding of a group element"), P2_ERR_INVALID;
    pt_put(a, out);
    return P2_OK;
}
int p2_ecgfp5_random_scalar(uint64_t out[5]) {
    return guarded([&] {
        ecgfp5::Rng rng = ecgfp5::Rng::os();
        memcpy(out, ecgfp5::random_scalar(rng).w, 40);
    });
}
int p2_ecgfp5_random_point(uint64_t out[10]) {
    return guarded([&] {
        ecgfp5::Rng rng = ecgfp5::Rng::os();
        pt_put(ecgfp5::random_point(rng), out);
    });
}
int p2_ecgfp5_encode_binary(const uint32_t limbs[5], uint64_t out[10]) {
    return guarded([&] {
        ecgfp5::Rng rng = ecgfp5::Rng::os();
        pt_put(ecgfp5::encode_binary(limbs, rng), out);
    });
}
void p2_ecgfp5_random_scalar_seeded(uint64_t seed, uint64_t out[5]) {
    (void)guarded([&] {
        ecgfp5::Rng rng = ecgfp5::Rng::from_seed(seed);
        memcpy(out, ecgfp5::random_scalar(rng).w, 40);
    });
}
void p2_ecgfp5_random_point_seeded(uint64_t seed, uint64_t out[10]) {
    (void)guarded([&] {
        ecgfp5::Rng rng = ecgfp5::Rng::from_seed(seed);
        pt_put(ecgfp5::random_point(rng), out);
    });
}
void p2_ecgfp5_encode_binary_seeded(const uint32_t limbs[5], uint64_t seed, uint64_t out[10]) {
    (void)guarded([&] {
        ecgfp5::Rng rng = ecgfp5::Rng::from_seed(seed);
        pt_put(ecgfp5::encode_binary(limbs, rng), out);
    });
}
void p2_ecgfp5_decode_binary(const uint64_t p[10], uint32_t limbs[5]) { (void)guarded([&] { ecgfp5::decode_binary(pt_at(p), limbs); }); }
int p2_elgamal_encrypt(const uint64_t pk[10], const uint64_t nonce[5], const uint64_t msg[10], uint64_t c0[10], uint64_t c1[10]) {
    if (scalar_ok(nonce)) return P2_ERR_INVALID;
    ecgfp5::Affine a, b;
    ecgfp5::elgamal_encrypt(pt_at(pk), sc_at(nonce), pt_at(msg), &a, &b);
    pt_put(a, c0);
    pt_put(b, c1);
    return P2_OK;
}
int p2_elgamal_decrypt(const uint64_t sk[5], const uint64_t c0[10], const uint64_t c1[10], uint64_t msg[10]) {
    if (scalar_ok(sk)) return P2_ERR_INVALID;
    pt_put(ecgfp5::elgamal_decrypt(sc_at(sk), pt_at(c0), pt_at(c1)), msg);
    return P2_OK;
}
int p2_hashed_elgamal_encrypt(const uint64_t pk[10], const uint64_t nonce[5], const uint64_t msg[5], uint64_t c0[10], uint64_t ct[5]) {
    if (scalar_ok(nonce)) return P2_ERR_INVALID;
    ecgfp5::Affine a;
    ecgfp5::hashed_elgamal_encrypt(pt_at(pk), sc_at(nonce), msg, &a, ct);
    pt_put(a, c0);
    return P2_OK;
}
int p2_hashed_elgamal_decrypt(const uint64_t sk[5], const uint64_t c0[10], const uint64_t ct[5], uint64_t msg[5]) {
    if (scalar_ok(sk)) return P2_ERR_INVALID;
    ecgfp5::hashed_elgamal_decrypt(sc_at(sk), pt_at(c0), ct, msg);
    return P2_OK;
}
void p2_builder_add_virtual_point_target(p2_builder* b, p2_target out[10]) { (void)guarded([&] { ptt_put(ecgfp5::add_virtual_point_target(b->b), out); }); }
void p2_builder_constant_point(p2_builder* b, const uint64_t p[10], p2_target out[10]) { (void)guarded([&] { ptt_put(ecgfp5::constant_point(b->b, pt_at(p)), out); }); }
void p2_builder_add_virtual_biguint320_target(p2_builder* b, p2_target bits[320]) {
    (void)guarded([&] {
        auto v = ecgfp5::add_virtual_biguint320_target(b->b);
        for (size_t i = 0; i < v.size(); i++) bits[i] = v[i].target;
    });
}
int p2_builder_multiply_point(p2_builder* b, const p2_target bits[320], const p2_target p[10], p2_target out[10]) {
    try {
        ptt_put(ecgfp5::multiply_point(b->b, bits_at(bits), ptt_at(p)), out);
        return P2_OK;
    } catch (std::exception& e) {
        return set_error(e.what()), P2_ERR_INVALID;
    }
}
void p2_builder_add_point(p2_builder* b, const p2_target p[10], const p2_target q[10], p2_target out[10]) { (void)guarded([&] {    ptt_put(ecgfp5::add_point(b->b, ptt_at(p), ptt_at(q)), out);}); }
int p2_builder_public_key(p2_builder* b, const p2_target sk_bits[320], p2_target pk[10]) {
    try {
        ptt_put(ecgfp5::public_key_target(b->b, bits_at(sk_bits)), pk);
        return P2_OK;
    } catch (std::exception& e) {
        return set_error(e.what()), P2_ERR_INVALID;
    }
}
int p2_builder_elgamal_encrypt(p2_builder* b, const p2_target pk[10], const p2_target nonce_bits[320], const p2_target msg[10], p2_target c0[10],
                               p2_target c1[10]) {
    try {
        ecgfp5::PointTarget a, c;
        ecgfp5::elgamal_encrypt_target(b->b, ptt_at(pk), bits_at(nonce_bits), ptt_at(msg), &a, &c);
        ptt_put(a, c0);
        ptt_put(c, c1);
        return P2_OK;
    } catch (std::exception& e) {
        return set_error(e.what()), P2_ERR_INVALID;
    }
}
int p2_builder_hashed_elgamal_encrypt(p2_builder* b, const p2_target pk[10], const p2_target nonce_bits[320], const p2_target msg[5],
                                      p2_target c0[10], p2_target ct[5]) {
    try {
        ecgfp5::PointTarget a;
        ecgfp5::hashed_elgamal_encrypt_target(b->b, ptt_at(pk), bits_at(nonce_bits), msg, &a, ct);
        ptt_put(a, c0);
        return P2_OK;
    } catch (std::exception& e) {
        return set_error(e.what()), P2_ERR_INVALID;
    }
}
// the host twin of p2_ecgfp5_encode_binary_batch, and the decryption gadgets (ecgfp5.h)
int p2_ecgfp5_encode_binary_padded(const uint32_t limbs[5], const uint32_t* pad, size_t attempts, uint64_t out[10], uint32_t* used) {
    if (!limbs || !out || !used || (attempts && !pad)) return set_error("null argument"), P2_ERR_INVALID;
    ecgfp5::Affine a;
    const size_t n = ecgfp5::encode_binary_padded(limbs, pad, attempts, &a);
    *used = (uint32_t)n;
    if (n == attempts) return set_error("no attempt decodes to a group element"), P2_ERR_INVALID;
    pt_put(a, out);
    return P2_OK;
}
int p2_builder_neg_point(p2_builder* b, const p2_target p[10], p2_target out[10]) {
    return guarded([&] { ptt_put(ecgfp5::neg_point(b->b, ptt_at(p)), out); });
}
int p2_builder_elgamal_decrypt(p2_builder* b, const p2_target sk_bits[320], const p2_target c0[10], const p2_target c1[10], p2_target msg[10]) {
    try {
        ptt_put(ecgfp5::elgamal_decrypt_target(b->b, bits_at(sk_bits), ptt_at(c0), ptt_at(c1)), msg);
        return P2_OK;
    } catch (std::exception& e) {
        return set_error(e.what()), P2_ERR_INVALID;
    }
}
int p2_builder_hashed_elgamal_decrypt(p2_builder* b, const p2_target sk_bits[320], const p2_target c0[10], const p2_target ct[5], p2_target msg[5]) {
    try {
        ecgfp5::hashed_elgamal_decrypt_target(b->b, bits_at(sk_bits), ptt_at(c0), ct, msg);
        return P2_OK;
    } catch (std::exception& e) {
        return set_error(e.what()), P2_ERR_INVALID;
    }
}

// ---- Schnorr signatures on ecGFp5 (schnorr.h): the host twins of p2_schnorr_*_batch, and the gadget
void p2_ecgfp5_scalar_muladd(const uint64_t a[5], const uint64_t b[5], const uint64_t c[5], uint64_t out[5]) { ecsc::sc_muladd(a, b, c, out); }
int p2_schnorr_challenge(const uint64_t r[10], const uint64_t pk[10], const uint64_t* msg, size_t msg_len, uint64_t e[4]) {
    return guarded([&] {
        if (msg_len > schnorr::MAX_MSG_LEN || (msg_len && !msg)) throw std::runtime_error("msg_len is at most 1024 words");
        schnorr::challenge(pt_at(r), pt_at(pk), msg, msg_len, e);
    });
}
int p2_schnorr_sign(const uint64_t sk[5], const uint64_t nonce[5], const uint64_t* msg, size_t msg_len, uint64_t sig[9], uint64_t pk[10], int* status) {
    return guarded([&] {
        if (!status || msg_len > schnorr::MAX_MSG_LEN || (msg_len && !msg)) throw std::runtime_error("msg_len is at most 1024 words, status not null");
        ecgfp5::Affine pub;
        *status = schnorr::sign(sc_at(sk), sc_at(nonce), msg, msg_len, sig, pk ? &pub : nullptr);
        if (pk) pt_put(pub, pk);
    });
}
int p2_schnorr_verify(const uint64_t pk[10], const uint64_t* msg, size_t msg_len, const uint64_t sig[9], int* status) {
    return guarded([&] {
        if (!status || msg_len > schnorr::MAX_MSG_LEN || (msg_len && !msg)) throw std::runtime_error("msg_len is at most 1024 words, status not null");
        *status = schnorr::verify(pt_at(pk), msg, msg_len, sig);
    });
}
int p2_builder_add_virtual_schnorr_signature(p2_builder* b, p2_target s_bits[320], p2_target e[4]) {
    return guarded([&] {
        const schnorr::SignatureTarget t = schnorr::add_virtual_signature_target(b->b);
        for (size_t i = 0; i < t.s_bits.size(); i++) s_bits[i] = t.s_bits[i].target;
        std::copy(t.e.begin(), t.e.end(), e);
    });
}
int p2_builder_verify_schnorr_signature(p2_builder* b, const p2_target pk[10], const p2_target* msg, size_t msg_len, const p2_target s_bits[320], const p2_target e[4],
                                        p2_target r[10]) {
    return guarded([&] {
        if (msg_len && !msg) throw std::runtime_error("null message");
        const schnorr::SignatureTarget t{bits_at(s_bits), hash_at(e)};
        const ecgfp5::PointTarget rp = schnorr::verify_signature_target(b->b, ptt_at(pk), std::vector<Target>(msg, msg + msg_len), t);
        if (r) ptt_put(rp, r);
    });
}

// ---- self-test
int p2_selftest_host(uint64_t seed, size_t n_reductions, size_t n_permutations) {
    u64 x = seed | 1;
    auto rnd = [&]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    size_t bad = 0;
    for (size_t i = 0; i < n_reductions; i++) {
        u64 hi = rnd(), lo = rnd();
        switch (i & 15) {
            case 0: hi &= gl::EPS; break;
            case 1: lo &= gl::EPS; break;
            case 2: hi |= ~gl::EPS; break;
            case 3: lo |= ~gl::EPS; break;
            case 4: hi = 0; break;
            case 5: lo = 0; break;
            case 6: hi = ~0ull; lo = ~0ull - (x & 3); break;
            case 7: hi &= ~gl::EPS; lo &= gl::EPS; break;
            default: break;
        }
        unsigned __int128 v = ((unsigned __int128)hi << 64) | lo;
        u64 want = (u64)(v % gl::P);
        if (glf::canon(glf::red128(hi, lo)) != want) bad++;
        if (gl::reduce128(hi, lo) != want) bad++;
        glf::Acc a;
        a.init();
        a.fma(hi, lo);
        a.fma(lo, lo);
        unsigned __int128 w = ((unsigned __int128)hi * lo) % gl::P + ((unsigned __int128)lo * lo) % gl::P;
        if (glf::canon(a.reduce()) != (u64)(w % gl::P)) bad++;
    }
    for (size_t i = 0; i < n_permutations; i++) {
        u64 s0[12], s1[12];
        for (int k = 0; k < 12; k++) s0[k] = s1[k] = (i & 3) == 3 ? rnd() : rnd() % gl::P;  // canonical or arbitrary words
        for (int k = 0; k < 12; k++) s0[k] %= gl::P;
        gl::poseidon(s0);
        glf::poseidon(s1);
        for (int k = 0; k < 12; k++) bad += s0[k] != s1[k];
    }
    return (int)std::min<size_t>(bad, 0x7FFFFFFF);
}

// The host build of the permutation with known-zero inputs and a mask of output words (poseidon_fast.h): FR_* kind, rows bit r =
// word r is kept.  parts = 0: the two round loops the kernels run; 1: first_round / middle / last_round one after the other.
int p2_host_poseidon_known(uint64_t* states, size_t n_perm, int kind, uint32_t rows, int parts) {
    if (kind < 0 || kind > (int)glf::FR_ZERO_RATE || rows == 0 || rows > glf::ROWS_ALL) return set_error("kind must be 0..2 and rows a mask of words 0..11"), P2_ERR_INVALID;
    for (size_t i = 0; i < n_perm; i++) {
        u64* s = states + 12 * i;
        if (parts) {
            glf::first_round_any(s, (u32)kind);
            glf::middle(s);
            glf::last_round_any(s, rows);
        } else {
            glf::permute_known_any(s, (u32)kind, rows);
        }
    }
    return P2_OK;
}
// pcipher::hash_state as the cipher kernels run it (p2k::pcipher_hash_state, kernels_pcipher.h).  last != 0: only out[5..10) is
// defined, the other words come back as 0.
int p2_host_pcipher_hash_state(const uint64_t in[20], int last, uint64_t out[20]) {
    if (!in || !out) return set_error("p2_host_pcipher_hash_state: null argument"), P2_ERR_INVALID;
    for (int i = 0; i < 20; i++)
        if (in[i] >= gl::P) return set_error("p2_host_pcipher_hash_state: non-canonical word"), P2_ERR_INVALID;
    u64 s[20];
    memcpy(s, in, sizeof s);
    p2k::pcipher_hash_state(s, last != 0);
    for (int i = 0; i < 20; i++) out[i] = (last && (i < 5 || i >= 10)) ? 0 : s[i];
    return P2_OK;
}
// The 22 partial rounds alone (glf::partial_block), on arbitrary u64 words: what reaches its folds is the caller's choice.
int p2_host_partial_rounds(uint64_t* states, size_t count) {
    for (size_t i = 0; i < count; i++) glf::partial_block(states + 12 * i);
    return P2_OK;
}
// Round 3's MDS and the partial rounds as one chain (glf::merged_middle), on arbitrary u64 words: round 3's S-box outputs in.
int p2_host_merged_middle(uint64_t* states, size_t count) {
    for (size_t i = 0; i < count; i++) glf::merged_middle(states + 12 * i);
    return P2_OK;
}
// EcStepGate's 40 constraints (ecstep_gate_constraints<FBase>) of `count` rows of 80 wires, on arbitrary canonical words; the
// _ext form is the <FExt> instantiation on (c0, c1) pairs.
int p2_host_ecstep_constraints(const uint64_t* wires, size_t count, uint64_t* out) {
    if (count && (!wires || !out)) return set_error("p2_host_ecstep_constraints: null argument"), P2_ERR_INVALID;
    for (size_t i = 0; i < 80 * count; i++)
        if (wires[i] >= gl::P) return set_error("p2_host_ecstep_constraints: non-canonical wire"), P2_ERR_INVALID;
    for (size_t r = 0; r < count; r++)
        ecstep_gate_constraints<FBase>([&](u32 i) { return wires[80 * r + i]; }, [&](int k, u64 c) { out[40 * r + k] = c; });
    return P2_OK;
}
int p2_host_ecstep_constraints_ext(const uint64_t* wires, size_t count, uint64_t* out) {
    if (count && (!wires || !out)) return set_error("p2_host_ecstep_constraints_ext: null argument"), P2_ERR_INVALID;
    for (size_t i = 0; i < 160 * count; i++)
        if (wires[i] >= gl::P) return set_error("p2_host_ecstep_constraints_ext: non-canonical wire"), P2_ERR_INVALID;
    for (size_t r = 0; r < count; r++)
        ecstep_gate_constraints<FExt>([&](u32 i) { return gl::e2(wires[160 * r + 2 * i], wires[160 * r + 2 * i + 1]); },
                                      [&](int k, gl::E2 c) { out[80 * r + 2 * k] = c.a, out[80 * r + 2 * k + 1] = c.b; });
    return P2_OK;
}
// k_hash_leaves on the host, with the same sponge steps (glf::sponge_permute): data [active][num_leaves] column-major, columns
// >= active_cols are zero and not stored; digests [num_leaves][4].
int p2_host_hash_leaves(const uint64_t* data, size_t cols, size_t active_cols, size_t num_leaves, uint64_t* digests) {
    if (cols == 0 || cols > (1u << 20)) return set_error("cols out of range"), P2_ERR_INVALID;
    for (size_t leaf = 0; leaf < num_leaves; leaf++) {
        u64 st[12] = {0};
        u64* out = digests + 4 * leaf;
        if (cols <= 4) {
            for (size_t c = 0; c < 4; c++) out[c] = (c < cols && c < active_cols) ? data[c * num_leaves + leaf] : 0;
            continue;
        }
        for (size_t c0 = 0; c0 < cols; c0 += 8) {
            for (size_t k = 0; k < 8 && c0 + k < cols; k++) st[k] = c0 + k < active_cols ? data[(c0 + k) * num_leaves + leaf] : 0;
            glf::sponge_permute(st, (int)c0, (int)cols, (int)std::min(active_cols, cols));
        }
        for (int i = 0; i < 4; i++) out[i] = st[i];
    }
    return P2_OK;
}

// ---- native cipher
uint8_t p2_native_gf_2_8_mul(uint8_t a, uint8_t b) { return aes::gf_2_8_mul(a, b); }
void p2_native_aes_key_expansion(const uint8_t* key, int nk, int nr, uint8_t* out) {
    (void)guarded([&] {
        auto w = aes::key_expansion(nk, nr, key);
        for (size_t i = 0; i < w.size(); i++) memcpy(out + 4 * i, w[i].data(), 4);
    });
}
void p2_native_aes_encrypt_block(const uint8_t* key, int nk, int nr, const uint8_t* in, uint8_t* out) {
    (void)guarded([&] {
        auto w = aes::key_expansion(nk, nr, key);
        auto s = aes::flatten_state(aes::encrypt_block(nr, in, w));
        memcpy(out, s.data(), 16);
    });
}
void p2_native_gf_2_128_mul(const uint8_t* x, const uint8_t* y, uint8_t* out) {
    (void)guarded([&] {
        auto r = aes::gf_2_128_mul(x, y);
        memcpy(out, r.data(), 16);
    });
}
void p2_native_ghash(const uint8_t* h, const uint8_t* x, size_t len, uint8_t* out) {
    (void)guarded([&] {
        auto r = aes::ghash(h, x, len);
        memcpy(out, r.data(), 16);
    });
}
void p2_native_gctr(const uint8_t* key, int nk, int nr, const uint8_t* icb, const uint8_t* x, size_t len, uint8_t* y) {
    (void)guarded([&] {
        auto w = aes::key_expansion(nk, nr, key);
        auto r = aes::gctr(nr, w, icb, x, len);
        if (len) memcpy(y, r.data(), len);
    });
}
void p2_native_aes_gcm_encrypt(const uint8_t* key, int nk, int nr, const uint8_t* nonce, const uint8_t* pt, size_t len, uint8_t* ct, uint8_t* tag) { (void)guarded([&] {    aes::gcm_encrypt(nk, nr, key, nonce, pt, len, ct, tag);}); }
void p2_native_aes_gcm_encrypt_aad(const uint8_t* key, int nk, int nr, const uint8_t* nonce, const uint8_t* aad, size_t aad_len, const uint8_t* pt, size_t len,
                                   uint8_t* ct, uint8_t* tag) {
    (void)guarded([&] { aes::gcm_encrypt_aad(nk, nr, key, nonce, aad, aad_len, pt, len, ct, tag); });
}
int p2_native_aes_gcm_decrypt(const uint8_t* key, int nk, int nr, const uint8_t* nonce, const uint8_t* aad, size_t aad_len, const uint8_t* ct, size_t len,
                              const uint8_t* tag, uint8_t* pt) {
    bool ok = false;
    if (guarded([&] { ok = aes::gcm_decrypt(nk, nr, key, nonce, aad, aad_len, ct, len, tag, pt); })) return P2_ERR_INVALID;
    if (!ok) set_error("aes-gcm decrypt: authentication failed");
    return ok ? 0 : 1;
}

// ---- info / verify
int p2_blob_info(const uint8_t* blob, size_t len, p2_circuit_info* out) {
    try {
        Circuit c = deserialize(blob, len);
        fill_info(c, out);
        return P2_OK;
    } catch (std::exception& e) {
        return set_error(e.what()), P2_ERR_INVALID;
    }
}
int p2_witness_schedule_check(const uint8_t* blob, size_t len, uint32_t fuse, uint32_t out[4]) {
    try {
        Circuit c = deserialize(blob, len);
        WitnessSchedule s = schedule_witness(c, fuse);
        const size_t M = c.ops.size(), n = (size_t)1 << c.degree_bits;
        const u32 R = c.cfg.num_routed_wires;
        auto same = [](const Op& x, const Op& y) { return x.kind == y.kind && x.out == y.out && x.a == y.a && x.b == y.b && x.c == y.c && x.aux == y.aux && x.k0 == y.k0 && x.k1 == y.k1; };
        auto slots_of = [&](const Op& o, u32* d, int& first_out) {
            int nd = 0;
            if (o.kind == OP_ARITH) d[nd++] = o.a, d[nd++] = o.b, d[nd++] = o.c;
            else if (o.kind == OP_LOOKUP || o.kind == OP_LIMB) d[nd++] = o.a;
            else if (o.kind == OP_EQ || o.kind == OP_EQINV) d[nd++] = o.a, d[nd++] = o.b;
            else if (o.kind == OP_POSEIDON) {
                for (u32 k = 0; k < 12; k++) d[nd++] = (u32)c.wire_slot[(size_t)(PG_IN + k) * n + o.a];
                d[nd++] = (u32)c.wire_slot[(size_t)PG_SWAP * n + o.a];
            } else if (o.kind == OP_ECSTEP) {
                for (u32 col = 0; col < EG_MID; col++) d[nd++] = (u32)c.wire_slot[(size_t)col * n + o.a];
            }
            first_out = nd;
            if (o.kind == OP_ECSTEP) {
                for (u32 col = EG_MID; col < EG_WIRES; col++) d[nd++] = (u32)c.wire_slot[(size_t)col * n + o.a];
            } else if (o.kind == OP_POSEIDON) {
                for (u32 col = PG_OUT; col < R; col++)
                    if (col != PG_SWAP) d[nd++] = (u32)c.wire_slot[(size_t)col * n + o.a];
            } else {
                d[nd++] = o.out;
            }
            return nd;
        };
        if (s.ops.size() != M || s.levels.empty()) return set_error("witness schedule: shape"), P2_ERR_INVALID;
        // every op belongs to exactly one unit (a chain or a single) of exactly one level, and the levels tile the op array
        const u32 NONE = ~0u;
        std::vector<u32> unit_of(M, NONE), level_of(M, NONE);
        u32 cursor = 0, unit = 0, chain_cursor = 0;
        for (size_t l = 0; l < s.levels.size(); l++) {
            const WLevel& L = s.levels[l];
            if (L.chain_begin != chain_cursor || (size_t)L.chain_begin + L.chain_count > s.chains.size()) return set_error("witness schedule: chain ranges"), P2_ERR_INVALID;
            for (u32 ci = 0; ci < L.chain_count; ci++) {
                const WChain& ch = s.chains[L.chain_begin + ci];
                if (ch.start != cursor || ch.count < 2 || ch.count > std::max<u32>(fuse, 1) || (size_t)ch.start + ch.count > M) return set_error("witness schedule: chain shape"), P2_ERR_INVALID;
                for (u32 k = 0; k < ch.count; k++) {
                    const u32 kind = s.ops[ch.start + k].kind;
                    if (kind != OP_ARITH && kind != OP_CONST && kind != OP_EQ) return set_error("witness schedule: a chain holds an op the chain executor does not run"), P2_ERR_INVALID;
                    unit_of[ch.start + k] = unit, level_of[ch.start + k] = (u32)l;
                }
                unit++;
                cursor += ch.count;
            }
            chain_cursor += L.chain_count;
            if (L.single_begin != cursor || L.single_end < L.single_begin || L.single_end > M) return set_error("witness schedule: single ranges"), P2_ERR_INVALID;
            for (u32 k = L.single_begin; k < L.single_end; k++) unit_of[k] = unit++, level_of[k] = (u32)l;
            cursor = L.single_end;
        }
        if (cursor != M || chain_cursor != s.chains.size()) return set_error("witness schedule: the levels do not tile the program"), P2_ERR_INVALID;
        // first producer of every slot, in the builder's order and in the scheduled order
        std::vector<int64_t> first_orig(c.num_slots, -1), first_sched(c.num_slots, -1);
        u32 d[96];
        int fo;
        for (size_t i = 0; i < M; i++) {
            int nd = slots_of(c.ops[i], d, fo);
            for (int j = fo; j < nd; j++)
                if (first_orig[d[j]] < 0) first_orig[d[j]] = (int64_t)i;
        }
        for (size_t i = 0; i < M; i++) {
            int nd = slots_of(s.ops[i], d, fo);
            for (int j = fo; j < nd; j++)
                if (first_sched[d[j]] < 0) first_sched[d[j]] = (int64_t)i;
        }
        for (u32 sl = 0; sl < c.num_slots; sl++) {
            if ((first_orig[sl] < 0) != (first_sched[sl] < 0)) return set_error("witness schedule: a slot lost or gained a producer"), P2_ERR_INVALID;
            if (first_orig[sl] >= 0 && !same(c.ops[first_orig[sl]], s.ops[first_sched[sl]])) return set_error("witness schedule: a slot changed its first producer"), P2_ERR_INVALID;
        }
        for (size_t i = 0; i < M; i++) {
            int nd = slots_of(s.ops[i], d, fo);
            for (int j = 0; j < nd; j++) {
                const int64_t p = first_sched[d[j]];
                if (p < 0 || p == (int64_t)i) continue;   // a user input, or this op is the producer
                const bool earlier_level = level_of[p] < level_of[i];
                const bool same_unit_before = unit_of[p] == unit_of[i] && p < (int64_t)i;
                if (!earlier_level && !same_unit_before) return set_error("witness schedule: an operand is not ready when its op runs"), P2_ERR_INVALID;
            }
        }
        // multiset of ops preserved: compare sorted fingerprints
        auto fp = [](const Op& o) { return ((u64)o.kind * 0x9E3779B97F4A7C15ull) ^ ((u64)o.out << 32 | o.a) ^ (((u64)o.b << 32 | o.c) * 0xBF58476D1CE4E5B9ull) ^ (o.k0 * 3 + o.k1 * 5 + o.aux); };
        std::vector<u64> fa(M), fb(M);
        for (size_t i = 0; i < M; i++) fa[i] = fp(c.ops[i]), fb[i] = fp(s.ops[i]);
        std::sort(fa.begin(), fa.end());
        std::sort(fb.begin(), fb.end());
        if (fa != fb) return set_error("witness schedule: ops changed"), P2_ERR_INVALID;
        out[0] = (u32)s.levels.size();
        out[1] = (u32)s.chains.size();
        out[2] = s.max_chain;
        out[3] = (u32)s.fused_ops;
        return P2_OK;
    } catch (std::exception& e) {
        return set_error(e.what()), P2_ERR_INVALID;
    }
}
// The host twin of the device's witness run (k_witness, k_witness_wired_unset, k_gather_slots, k_witness_check/_report): the
// scheduled op program interpreted one op after the other, with the kernel's rules -- an op with an unset operand does not run
// (2), a conflict or a lookup miss (1) outranks it, nothing stops the run -- and then the shared check of witness_check.h.
int p2_host_witness(const uint8_t* blob, size_t len, const p2_assignment* input, const p2_target* out_targets, size_t n_out, uint64_t* out_values, int* status,
                    void* fault_out) {
    p2_witness_fault* fault = (p2_witness_fault*)fault_out;
    try {
        if (!blob || !input || !status || (n_out && (!out_targets || !out_values)) || (input->count && (!input->targets || !input->values)))
            return set_error("p2_host_witness: null argument"), P2_ERR_INVALID;
        const Circuit c = deserialize(blob, len);
        std::vector<u32> in_slots(input->count), out_slots(n_out);
        for (size_t i = 0; i < input->count; i++) {
            const int32_t s = target_slot(c, input->targets[i]);
            if (s < 0) return set_error("input target is not a target of this circuit"), P2_ERR_INVALID;
            in_slots[i] = (u32)s;
        }
        for (size_t i = 0; i < n_out; i++) {
            const int32_t s = target_slot(c, out_targets[i]);
            if (s < 0) return set_error("output target is not a target of this circuit"), P2_ERR_INVALID;
            out_slots[i] = (u32)s;
        }
        const WitnessTables T = witness_tables(c);
        const WitnessSchedule sched = schedule_witness(c, 1);
        const size_t n = c.n();
        std::vector<u64> val(c.num_slots, W_UNSET);
        int worst = 0;  // 0 ok, 2 missing input, 3 conflict: the encoding of k_witness's s_status
        auto put = [&](u32 slot, u64 v) {
            if (val[slot] == W_UNSET) val[slot] = v;
            else if (val[slot] != v) worst = 3;
        };
        for (size_t i = 0; i < input->count; i++) {
            if (input->values[i] >= gl::P) worst = 3;  // an assignment has no "absent" marker: 2^64-1 is a non-canonical value like any other
            else put(in_slots[i], input->values[i]);
        }
        for (const Op& o : sched.ops) {
            if (o.kind == OP_POSEIDON) {
                u64 w[135];
                bool ready = true;
                for (u32 col = 0; col < 12; col++) ready &= (w[col] = val[c.wire_slot[(size_t)col * n + o.a]]) != W_UNSET;
                ready &= (w[PG_SWAP] = val[c.wire_slot[(size_t)PG_SWAP * n + o.a]]) != W_UNSET;
                if (!ready) {
                    worst = std::max(worst, 2);
                    continue;
                }
                poseidon_gate_witness(w);
                for (u32 col = PG_OUT; col < c.cfg.num_routed_wires; col++)
                    if (col != PG_SWAP) put((u32)c.wire_slot[(size_t)col * n + o.a], w[col]);
                continue;
            }
            if (o.kind == OP_ECSTEP) {
                u64 w[EG_WIRES];
                bool ready = true;
                for (u32 col = 0; col < EG_MID; col++) ready &= (w[col] = val[c.wire_slot[(size_t)col * n + o.a]]) != W_UNSET;
                if (!ready) {
                    worst = std::max(worst, 2);
                    continue;
                }
                ecstep_gate_witness(w);
                for (u32 col = EG_MID; col < EG_WIRES; col++) put((u32)c.wire_slot[(size_t)col * n + o.a], w[col]);
                continue;
            }
            u64 x = 0, y = 0, z = 0, r = 0;
            if (o.kind != OP_CONST) x = val[o.a];
            if (o.kind == OP_ARITH || o.kind == OP_EQ || o.kind == OP_EQINV) y = val[o.b];
            if (o.kind == OP_ARITH) z = val[o.c];
            if (x == W_UNSET || y == W_UNSET || z == W_UNSET) {
                worst = std::max(worst, 2);
                continue;
            }
            if (o.kind == OP_ARITH) {
                r = gl::add(gl::mul(gl::mul(x, y), o.k0), gl::mul(z, o.k1));
            } else if (o.kind == OP_CONST) {
                r = o.k0;
            } else if (o.kind == OP_LOOKUP) {
                const u64 ent = x < 65536 ? T.lut_ent[(size_t)o.aux * 65536 + x] : ~0ull;
                if (ent == ~0ull) {
                    worst = 3;
                    continue;
                }
                r = ent & 0xFFFF;
            } else if (o.kind == OP_EQ) {
                r = x == y ? 1 : 0;
            } else if (o.kind == OP_LIMB) {
                r = limb_of(x, o.k0, o.k1);
            } else {
                r = x == y ? 0 : gl::inv(gl::sub(x, y));
            }
            put(o.out, r);
        }
        int st = worst == 3 ? 1 : worst;
        if (st == 0)  // k_fill_wires' rule, as k_witness_wired_unset keeps it
            for (u32 s : T.wired_slots)
                if (val[s] == W_UNSET) {
                    st = 2;
                    break;
                }
        *status = st;
        for (size_t i = 0; i < n_out; i++) out_values[i] = val[out_slots[i]];
        if (!fault) return P2_OK;
        const std::vector<u32> prev = input_prev_links(in_slots, c.num_slots);
        WCheckCtx x{};
        x.ops = c.ops.data(), x.num_ops = (u32)c.ops.size(), x.num_slots = c.num_slots, x.n = (u32)n;
        x.val = val.data(), x.lut_ent = T.lut_ent.data(), x.wire_slot = c.wire_slot.data();
        x.free_slots = T.free_slots.data(), x.num_free = (u32)T.free_slots.size(), x.slot_target = T.slot_target.data(), x.slot_row = T.slot_row.data();
        x.input_slots = in_slots.data(), x.input_values = input->values, x.n_inputs = (u32)input->count, x.absent_marker = 0;
        u32 bad_input = W_NO_INDEX, conflict_input = W_NO_INDEX, bad_op = W_NO_INDEX, unset_free = W_NO_INDEX, slot = W_NO_INDEX;
        for (u32 i = x.n_inputs; i-- > 0;) {
            u64 earlier;
            const int k = wcheck_input(x, prev.data(), i, &earlier);
            if (k == P2_FAULT_INPUT_NOT_CANONICAL) bad_input = i;
            if (k == P2_FAULT_INPUT_CONFLICT) conflict_input = i;
        }
        for (u32 i = 0; i < x.num_ops && bad_op == W_NO_INDEX; i++)
            if (wcheck_op(x, i).kind) bad_op = i;
        for (u32 j = 0; j < x.num_free && unset_free == W_NO_INDEX; j++)
            if (val[T.free_slots[j]] == W_UNSET) unset_free = j;
        wfault_report(x, prev.data(), st, bad_input, conflict_input, bad_op, unset_free, fault, &slot);
        for (u32 i = 0; slot != W_NO_INDEX && i < x.n_inputs; i++)
            if (in_slots[i] == slot && winput_sets(x, i)) {
                fault->input_index = i;
                break;
            }
        return P2_OK;
    } catch (std::exception& e) {
        return set_error(e.what()), P2_ERR_INVALID;
    }
}
int p2_verify(const uint8_t* blob, size_t blob_len, const uint64_t* vd, size_t vd_len, const uint8_t* proof, size_t proof_len) {
    try {
        Circuit c = deserialize(blob, blob_len);
        VerifierData v;
        if (!read_verifier_data(c, vd, vd_len, v)) return set_error("verifier_data must be cap || circuit_digest"), P2_ERR_INVALID;
        std::string err = verify_proof(c, v, proof, proof_len);
        if (!err.empty()) return set_error(err), P2_ERR_VERIFY;
        return P2_OK;
    } catch (std::exception& e) {
        return set_error(e.what()), P2_ERR_INVALID;
    }
}
// eval_vanishing (verifier.h) on openings and challenges the caller supplies; see include/p2aes.h.
int p2_vanishing_terms(const uint8_t* blob, size_t blob_len, const uint8_t* openings, size_t len, const uint64_t challenges[16],
                       const uint64_t pi_hash[4], uint64_t* terms, size_t cap, size_t* n_terms, uint64_t* sides, int* verdict) {
    try {
        if (!openings || !challenges || !pi_hash || !n_terms || !sides || !verdict || (cap && !terms))
            return set_error("p2_vanishing_terms: null argument"), P2_ERR_INVALID;
        Circuit c = deserialize(blob, blob_len);
        const ProofLayout L = make_proof_layout(c);
        const size_t NC = c.cfg.num_challenges;
        if (len != L.bytes) return set_error("p2_vanishing_terms: the buffer must have the size of a proof of the circuit"), P2_ERR_INVALID;
        if (NC != 2) return set_error("p2_vanishing_terms: num_challenges != 2"), P2_ERR_INVALID;
        ParsedProof pp;
        std::vector<gl::E2>* groups[OG_GROUPS];
        groups[OG_CONSTANTS] = &pp.o_constants, groups[OG_SIGMAS] = &pp.o_sigmas, groups[OG_WIRES] = &pp.o_wires, groups[OG_ZS] = &pp.o_zs;
        groups[OG_ZS_NEXT] = &pp.o_zs_next, groups[OG_LOOKUP_ZS] = &pp.o_lk, groups[OG_LOOKUP_ZS_NEXT] = &pp.o_lk_next;
        groups[OG_PARTIAL_PRODUCTS] = &pp.o_pp, groups[OG_QUOTIENT] = &pp.o_quot;
        bool canonical = true;
        for (u32 g = 0; g < OG_GROUPS; g++)
            for (size_t i = 0; i < L.open[g].len; i++) {
                u64 w[2];
                memcpy(w, openings + L.open[g].off + 16 * i, 16);
                canonical = canonical && w[0] < gl::P && w[1] < gl::P;
                groups[g]->push_back(gl::e2(w[0], w[1]));
            }
        for (int i = 0; i < 16; i++) canonical = canonical && challenges[i] < gl::P;
        for (int i = 0; i < 4; i++) canonical = canonical && pi_hash[i] < gl::P;
        if (!canonical) return set_error("p2_vanishing_terms: non-canonical field element"), P2_ERR_INVALID;
        Transcript T;
        T.betas.assign(challenges, challenges + 2);
        T.gammas.assign(challenges + 2, challenges + 4);
        T.deltas.assign(challenges + 4, challenges + 12);
        T.alphas.assign(challenges + 12, challenges + 14);
        T.zeta = gl::e2(challenges[14], challenges[15]);
        for (int i = 0; i < 4; i++) T.pi_hash.e[i] = c.pi_slots.empty() ? 0 : pi_hash[i];
        VanishingEval ev;
        const std::string reason = eval_vanishing(c, pp, T, &ev);
        *n_terms = ev.terms.size();
        memset(sides, 0, 8 * sizeof(uint64_t));
        if (reason == "Opening point is in the subgroup.") return *verdict = P2_VERIFY_ZETA_IN_SUBGROUP, P2_OK;
        if (ev.terms.size() > cap) return set_error("p2_vanishing_terms: " + std::to_string(ev.terms.size()) + " terms, room for fewer"), P2_ERR_INVALID;
        for (size_t k = 0; k < ev.terms.size(); k++) terms[2 * k] = ev.terms[k].a, terms[2 * k + 1] = ev.terms[k].b;
        for (size_t i = 0; i < NC; i++) sides[4 * i] = ev.lhs[i].a, sides[4 * i + 1] = ev.lhs[i].b, sides[4 * i + 2] = ev.rhs[i].a, sides[4 * i + 3] = ev.rhs[i].b;
        *verdict = reason.empty() ? P2_VERIFY_OK : P2_VERIFY_VANISHING;
        return P2_OK;
    } catch (std::exception& e) {
        return set_error(e.what()), P2_ERR_INVALID;
    }
}
int p2_proof_compress(const uint8_t* blob, size_t blob_len, const uint64_t* vd, size_t vd_len, const uint8_t* proof, size_t proof_len, uint8_t* out,
                      size_t cap, size_t* n_written) {
    return convert_proof(blob, blob_len, vd, vd_len, proof, proof_len, out, cap, n_written,
                         [](const Circuit& c, const VerifierData& v, const uint8_t* p, size_t n, std::vector<uint8_t>& r) { return compress_proof(c, v, p, n, r); });
}
int p2_proof_decompress(const uint8_t* blob, size_t blob_len, const uint64_t* vd, size_t vd_len, const uint8_t* cproof, size_t cproof_len,
                        uint8_t* out, size_t cap, size_t* n_written) {
    return convert_proof(blob, blob_len, vd, vd_len, cproof, cproof_len, out, cap, n_written,
                         [](const Circuit& c, const VerifierData& v, const uint8_t* p, size_t n, std::vector<uint8_t>& r) {
                             return decompress_proof(c, v, p, n, r, false);
                         });
}
int p2_verify_compressed(const uint8_t* blob, size_t blob_len, const uint64_t* vd, size_t vd_len, const uint8_t* cproof, size_t cproof_len) {
    try {
        Circuit c = deserialize(blob, blob_len);
        VerifierData v;
        if (!read_verifier_data(c, vd, vd_len, v)) return set_error("verifier_data must be cap || circuit_digest"), P2_ERR_INVALID;
        if (!cproof) return set_error("null proof"), P2_ERR_INVALID;
        std::string err = verify_compressed_proof(c, v, cproof, cproof_len);
        if (!err.empty()) return set_error(err), P2_ERR_VERIFY;
        return P2_OK;
    } catch (std::exception& e) {
        return set_error(e.what()), P2_ERR_INVALID;
    }
}
int p2_proof_public_inputs(const uint8_t* blob, size_t blob_len, const uint8_t* proof, size_t proof_len, uint64_t* out, size_t cap, size_t* n_written) {
    try {
        Circuit c = deserialize(blob, blob_len);  // the whole blob: p2_circuit_public_inputs is the per-proof form
        return read_public_inputs(make_proof_layout(c), proof, proof_len, out, cap, n_written);
    } catch (std::exception& e) {
        return set_error(e.what()), P2_ERR_INVALID;
    }
}
}
