// ElGamal on ecGFp5 in GPU batches (ecgfp5.h has the schemes and the host twins; include/p2aes.h the entry points): square roots
// in GF(p^5), point decompression, encode_binary with caller-supplied padding, the plain and the hashed cipher, and a scalar's
// bits for the prover's value matrix.  One thread per item, 64 threads per block, on the helpers of kernels_schnorr.h: an item is
// one or two 320-step ladders, one inversion per affine point and, for the hashed cipher, two permutations of the overwrite-mode
// sponge.  Every value stays canonical, so outputs are the host's word for word -- including which square root ecq_sqrt returns
// and which candidate ec_decompress takes, since both walk the host's steps in the host's order.  The Tonelli-Shanks loops
// diverge across lanes; they are bounded by the field's 2-adicity (32 rounds of at most 32 squarings) and small beside a ladder.
#pragma once
#include "kernels_schnorr.h"

namespace p2k {

// ecgfp5::gl_sqrt: Tonelli-Shanks in GF(p), p - 1 = 2^32 odd, POW2_GEN of order 2^32.  false: a is not a square.
GL_D bool gl_sqrt_dev(u64 a, u64& out) {
    out = 0;
    if (a == 0) return true;
    if (gl::pow(a, (gl::P - 1) / 2) != 1) return false;
    const u64 q = (gl::P - 1) >> 32;
    u64 c = gl::POW2_GEN, x = gl::pow(a, (q + 1) / 2), t = gl::pow(a, q);
    int m = 32;
#pragma nounroll
    for (int round = 0; round < 32 && t != 1; round++) {  // m falls every round: at most 32
        int i = 0;
#pragma nounroll
        for (u64 t2 = t; t2 != 1 && i < m; i++) t2 = gl::sqr(t2);
        const u64 b = gl::exp_pow2(c, m - i - 1);
        x = gl::mul(x, b);
        c = gl::sqr(b);
        t = gl::mul(t, c);
        m = i;
    }
    out = x;
    return true;
}
// ecgfp5::fq_sqrt: sqrt(a) = sqrt((a v^2)_0) / v with v = a^((r-1)/2) up to the norm, y = a^((p+1)/2), v = frob_1(y frob_2(y)).
// false: a is not a square.
GL_D bool ecq_sqrt(const EcFq& a, EcFq& out) {
    out = ecq_zero();
    if (ecq_is_zero(a)) return true;
    EcFq y = ecq_one(), base = a;
#pragma nounroll
    for (u64 e = (gl::P + 1) / 2; e; e >>= 1) {
        if (e & 1) y = p2::q5_mul<p2::FBase>(y, base);
        base = p2::q5_mul<p2::FBase>(base, base);
    }
    const EcFq v = ecq_frob<1>(p2::q5_mul<p2::FBase>(y, ecq_frob<2>(y)));
    u64 s;
    if (!gl_sqrt_dev(ecq_mul_c0(a, p2::q5_mul<p2::FBase>(v, v)), s)) return false;
    out = p2::q5_scale<p2::FBase>(ecq_inv(v), s);
    return true;
}
// ecgfp5::decompress_into_subgroup: the group element with compressed form u, x a root of x^2 + (2 - 1/u^2) x + 263 z that is
// not a square.  The candidates (r - bc)/2 and (-r - bc)/2 are tried in this order.  false: no group element has this u.
GL_D bool ec_decompress(const EcFq& u, EcAffine& out) {
    out.x = ecq_zero(), out.u = ecq_zero();
    if (ecq_is_zero(u)) return true;
    EcFq bc = ecq_neg(ecq_inv(p2::q5_mul<p2::FBase>(u, u)));
    bc.c[0] = gl::add(bc.c[0], 2);
    EcFq disc = p2::q5_mul<p2::FBase>(bc, bc);
    disc.c[1] = gl::sub(disc.c[1], 4 * p2::EG_B1);
    EcFq r;
    if (!ecq_sqrt(disc, r)) return false;
    bool found = false;
#pragma nounroll
    for (int s = 0; s < 2 && !found; s++) {
        EcAffine cand;
        cand.x = p2::q5_scale<p2::FBase>(p2::q5_sub<p2::FBase>(r, bc), (gl::P + 1) / 2);
        cand.u = u;
        if (ec_in_subgroup(cand)) out = cand, found = true;
        r = ecq_neg(r);
    }
    return found;
}
GL_D void zero_words(u64* __restrict__ o, int n) {
    for (int w = 0; w < n; w++) o[w] = 0;
}
// a point as the kernels take one: canonical words, inside the group (the neutral is)
GL_D bool ec_point_ok(const EcAffine& q) { return ecq_canonical(q.x) && ecq_canonical(q.u) && ec_in_subgroup(q); }
GL_D bool sc_ok(const u64* __restrict__ k) {
    u64 a[5];
#pragma unroll
    for (int w = 0; w < 5; w++) a[w] = k[w];
    return p2::ecsc::sc_below_order(a);
}
// the first five words of hash_n_to_m_no_pad(a.x | a.u, 5): eight words, a permutation, two words, a permutation
GL_D void elgamal_pad(const EcAffine& a, u64 h[5]) {
    u64 st[12];
#pragma unroll
    for (int i = 0; i < 5; i++) st[i] = a.x.c[i];
#pragma unroll
    for (int i = 0; i < 3; i++) st[5 + i] = a.u.c[i];
#pragma unroll
    for (int i = 8; i < 12; i++) st[i] = 0;
    glf::poseidon_sparse(st);
    st[0] = a.u.c[3], st[1] = a.u.c[4];
    glf::poseidon_sparse(st);
#pragma unroll
    for (int i = 0; i < 5; i++) h[i] = st[i];
}

// out[i] = the group element with compressed form w[i].  status 0; 1 (row zeroed) when w[i] encodes no group element; 2 (row
// zeroed) for a word not below p.
__global__ __launch_bounds__(64) void k_ec_decompress_batch(const u64* __restrict__ w, size_t count, u64* __restrict__ out, int* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const EcFq u = ecq_load(w + 5 * i);
    u64* o = out + 10 * i;
    EcAffine a;
    const int st = !ecq_canonical(u) ? 2 : ec_decompress(u, a) ? 0 : 1;
    if (st)
        zero_words(o, 10);
    else
        ec_store_affine(o, a);
    status[i] = st;
}

// ecgfp5::encode_binary with the random high halves supplied: attempt a decompresses w[j] = limbs[j] + (pad[a][j] << 32), an
// attempt with a word not below p is skipped, the first that decodes gives out[i] and used[i].  status 0, or 1 (row zeroed,
// used[i] = attempts) when none decodes.
__global__ __launch_bounds__(64) void k_ec_encode_binary(const u32* __restrict__ limbs, const u32* __restrict__ pad, u32 attempts, size_t count, u64* __restrict__ out,
                                                         u32* __restrict__ used, int* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const u32* lo = limbs + 5 * i;
    const u32* hi = pad + 5 * i * (size_t)attempts;
    u64* o = out + 10 * i;
    u32 a = 0;
    bool found = false;
    EcAffine pt;
#pragma nounroll
    for (; a < attempts; a++) {
        EcFq w;
#pragma unroll
        for (int j = 0; j < 5; j++) w.c[j] = (u64)lo[j] + ((u64)hi[5 * (size_t)a + j] << 32);
        if (!ecq_canonical(w)) continue;
        if (ec_decompress(w, pt)) {
            found = true;
            break;
        }
    }
    if (found)
        ec_store_affine(o, pt);
    else
        zero_words(o, 10);
    used[i] = a;
    status[i] = found ? 0 : 1;
}

// c0[i] = nonce[i] G, c1[i] = msg[i] + nonce[i] pk[i] (elgamal.rs:11).  status 0, or 2 (rows zeroed) for a nonce not below n or a
// pk or msg that k_ec_mul_batch would refuse.
__global__ __launch_bounds__(64) void k_elgamal_encrypt(const u64* __restrict__ pk, const u64* __restrict__ nonce, const u64* __restrict__ msg, size_t count, EcWords gen,
                                                        u64* __restrict__ c0, u64* __restrict__ c1, int* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const u64* k = nonce + 5 * i;
    if (!sc_ok(k) || !ec_point_ok(ec_load_affine(pk + 10 * i)) || !ec_point_ok(ec_load_affine(msg + 10 * i))) {
        zero_words(c0 + 10 * i, 10);
        zero_words(c1 + 10 * i, 10);
        status[i] = 2;
        return;
    }
    ec_store_affine(c0 + 10 * i, ec_affine(ec_ladder(k, ec_from_words(gen))));
    const EcProj s = ec_ladder(k, ec_load_affine(pk + 10 * i));
    const EcAffine m = ec_load_affine(msg + 10 * i);
    ec_store_affine(c1 + 10 * i, ec_affine(p2::ec_add_mixed<p2::FBase>(s, m.x, m.u)));
    status[i] = 0;
}

// msg[i] = c1[i] - sk[i] c0[i] (elgamal.rs:19).  status 0, or 2 (row zeroed) for sk not below n or a c0 or c1 outside the group.
__global__ __launch_bounds__(64) void k_elgamal_decrypt(const u64* __restrict__ sk, const u64* __restrict__ c0, const u64* __restrict__ c1, size_t count, u64* __restrict__ msg,
                                                        int* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const u64* k = sk + 5 * i;
    if (!sc_ok(k) || !ec_point_ok(ec_load_affine(c0 + 10 * i)) || !ec_point_ok(ec_load_affine(c1 + 10 * i))) {
        zero_words(msg + 10 * i, 10);
        status[i] = 2;
        return;
    }
    EcProj s = ec_ladder(k, ec_load_affine(c0 + 10 * i));
    s.U = ecq_neg(s.U);
    const EcAffine c = ec_load_affine(c1 + 10 * i);
    ec_store_affine(msg + 10 * i, ec_affine(p2::ec_add_mixed<p2::FBase>(s, c.x, c.u)));
    status[i] = 0;
}

// c0[i] = nonce[i] G, ct[i][j] = msg[i][j] + h[j] with h = hash_n_to_m_no_pad(as_fields(nonce[i] pk[i]), 5) (hashed_elgamal.rs:19).
// status 0, or 2 (rows zeroed) for a nonce not below n, a pk outside the group or a message word not below p.
__global__ __launch_bounds__(64) void k_hashed_elgamal_encrypt(const u64* __restrict__ pk, const u64* __restrict__ nonce, const u64* __restrict__ msg, size_t count,
                                                               EcWords gen, u64* __restrict__ c0, u64* __restrict__ ct, int* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const u64* k = nonce + 5 * i;
    if (!sc_ok(k) || !words_canonical(msg + 5 * i, 5) || !ec_point_ok(ec_load_affine(pk + 10 * i))) {
        zero_words(c0 + 10 * i, 10);
        zero_words(ct + 5 * i, 5);
        status[i] = 2;
        return;
    }
    ec_store_affine(c0 + 10 * i, ec_affine(ec_ladder(k, ec_from_words(gen))));
    u64 h[5];
    elgamal_pad(ec_affine(ec_ladder(k, ec_load_affine(pk + 10 * i))), h);
#pragma unroll
    for (int j = 0; j < 5; j++) ct[5 * i + j] = gl::add(msg[5 * i + j], h[j]);
    status[i] = 0;
}

// msg[i][j] = ct[i][j] - h[j] with h from sk[i] c0[i] (hashed_elgamal.rs:28).  status 0, or 2 (row zeroed) for sk not below n, a c0
// outside the group or a ciphertext word not below p.
__global__ __launch_bounds__(64) void k_hashed_elgamal_decrypt(const u64* __restrict__ sk, const u64* __restrict__ c0, const u64* __restrict__ ct, size_t count,
                                                               u64* __restrict__ msg, int* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const u64* k = sk + 5 * i;
    if (!sc_ok(k) || !words_canonical(ct + 5 * i, 5) || !ec_point_ok(ec_load_affine(c0 + 10 * i))) {
        zero_words(msg + 5 * i, 5);
        status[i] = 2;
        return;
    }
    u64 h[5];
    elgamal_pad(ec_affine(ec_ladder(k, ec_load_affine(c0 + 10 * i))), h);
#pragma unroll
    for (int j = 0; j < 5; j++) msg[5 * i + j] = gl::sub(ct[5 * i + j], h[j]);
    status[i] = 0;
}

// out[i stride + j] = bit j of the scalar k[i], j < 320, least significant first: a row of the prover's value matrix
__global__ __launch_bounds__(64) void k_ec_scalar_bits(const u64* __restrict__ k, size_t count, u64* __restrict__ out, size_t stride) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    u64* o = out + i * stride;
#pragma nounroll
    for (int limb = 0; limb < 5; limb++) {
        const u64 w = k[5 * i + limb];
#pragma nounroll
        for (int j = 0; j < 64; j++) o[64 * limb + j] = (w >> j) & 1;
    }
}

}  // namespace p2k
