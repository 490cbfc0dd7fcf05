// Native ecGFp5 in GPU batches: scalar multiplication, Schnorr signing and Schnorr verification (schnorr.h has the scheme and the
// host twins; include/p2aes.h the entry points).  One thread per item, 64 threads per block: an item is a 320-step ladder of
// ec_double<FBase> / ec_add_mixed<FBase> (ecstep_gate.h, the formulas of the EcStepGate and of k_ecwitness), then one inversion
// in GF(p^5) for the affine form and, for signatures, the overwrite-mode Poseidon sponge (glf::poseidon_sparse, as
// PoseidonTree::hash_or_noop walks it) and one (a b + c) mod n (ecgfp5_scalar.h).  Every value stays canonical, so outputs are
// the host's word for word.  Scalars are read from global memory one limb per 64 steps, points and accumulators live in
// registers; the generator arrives as a kernel argument (uniform: scalar registers).
#pragma once
#include "ecgfp5_scalar.h"
#include "ecstep_gate.h"
#include "poseidon_fast.h"

namespace p2k {

typedef p2::Q5<p2::FBase> EcFq;
typedef p2::EcPoint<p2::FBase> EcProj;
struct EcAffine {
    EcFq x, u;
};
struct EcWords {  // a point as its ten words x | u, by value in a kernel's arguments
    u64 w[10];
};

// ---- compile-time Frobenius constants: z^p = gamma z with gamma = 3^((p-1)/5), so a^(p^k) scales coefficient i by gamma^(i k)
namespace ecfrob {
constexpr u64 cmul(u64 a, u64 b) { return (u64)(((unsigned __int128)a * b) % gl::P); }
constexpr u64 cpow(u64 b, u64 e) {
    u64 r = 1;
    for (; e; e >>= 1) {
        if (e & 1) r = cmul(r, b);
        b = cmul(b, b);
    }
    return r;
}
constexpr u64 GAMMA = cpow(3, (gl::P - 1) / 5);
static_assert(GAMMA != 1 && cpow(GAMMA, 5) == 1, "gamma is a primitive fifth root of unity");
// coefficient i of a^(p^K)
template <int K>
GL_D u64 scale(int i) {
    constexpr u64 s1 = cpow(GAMMA, K), s2 = cpow(GAMMA, 2 * K), s3 = cpow(GAMMA, 3 * K), s4 = cpow(GAMMA, 4 * K);
    return i == 0 ? 1 : i == 1 ? s1 : i == 2 ? s2 : i == 3 ? s3 : s4;
}
}  // namespace ecfrob

GL_D EcFq ecq_zero() {
    EcFq r;
#pragma unroll
    for (int i = 0; i < 5; i++) r.c[i] = 0;
    return r;
}
GL_D EcFq ecq_one() {
    EcFq r = ecq_zero();
    r.c[0] = 1;
    return r;
}
GL_D EcFq ecq_load(const u64* p) {
    EcFq r;
#pragma unroll
    for (int i = 0; i < 5; i++) r.c[i] = p[i];
    return r;
}
GL_D bool ecq_is_zero(const EcFq& a) { return (a.c[0] | a.c[1] | a.c[2] | a.c[3] | a.c[4]) == 0; }
GL_D bool ecq_eq(const EcFq& a, const EcFq& b) {
    bool e = true;
#pragma unroll
    for (int i = 0; i < 5; i++) e &= a.c[i] == b.c[i];
    return e;
}
GL_D bool ecq_canonical(const EcFq& a) {
    bool c = true;
#pragma unroll
    for (int i = 0; i < 5; i++) c &= a.c[i] < gl::P;
    return c;
}
GL_D EcFq ecq_neg(const EcFq& a) {
    EcFq r;
#pragma unroll
    for (int i = 0; i < 5; i++) r.c[i] = gl::neg(a.c[i]);
    return r;
}
// a where bit = 1, zero where bit = 0
GL_D EcFq ecq_masked(const EcFq& a, u64 bit) {
    EcFq r;
#pragma unroll
    for (int i = 0; i < 5; i++) r.c[i] = a.c[i] & (0 - bit);
    return r;
}
template <int K>
GL_D EcFq ecq_frob(const EcFq& a) {
    EcFq r;
    r.c[0] = a.c[0];
#pragma unroll
    for (int i = 1; i < 5; i++) r.c[i] = gl::mul(a.c[i], ecfrob::scale<K>(i));
    return r;
}
// a^(p + p^2 + p^3 + p^4): a times it is the norm, an element of GF(p) (ecgfp5::fq_conj_product)
GL_D EcFq ecq_conj_product(const EcFq& a) {
    const EcFq t = p2::q5_mul<p2::FBase>(ecq_frob<1>(a), ecq_frob<2>(a));
    return p2::q5_mul<p2::FBase>(t, ecq_frob<2>(t));
}
// coefficient 0 of a b
GL_D u64 ecq_mul_c0(const EcFq& a, const EcFq& b) {
    u64 hi = gl::mul(a.c[1], b.c[4]);
#pragma unroll
    for (int i = 2; i < 5; i++) hi = gl::add(hi, gl::mul(a.c[i], b.c[5 - i]));
    return gl::add(gl::mul(a.c[0], b.c[0]), gl::mul(hi, 3));
}
GL_D u64 ecq_norm(const EcFq& a) { return ecq_mul_c0(a, ecq_conj_product(a)); }
GL_D EcFq ecq_inv(const EcFq& a) {  // 0 -> 0, as ecgfp5::fq_inv
    const EcFq t = ecq_conj_product(a);
    const u64 nrm = ecq_mul_c0(a, t);
    return p2::q5_scale<p2::FBase>(t, nrm ? gl::inv(nrm) : 0);
}
// (X / Z, U / T) with one inversion, of Z T
GL_D EcAffine ec_affine(const EcProj& p) {
    const EcFq i = ecq_inv(p2::q5_mul<p2::FBase>(p.Z, p.T));
    EcAffine a;
    a.x = p2::q5_mul<p2::FBase>(p.X, p2::q5_mul<p2::FBase>(i, p.T));
    a.u = p2::q5_mul<p2::FBase>(p.U, p2::q5_mul<p2::FBase>(i, p.Z));
    return a;
}
GL_D EcProj ec_neutral() { return EcProj{ecq_zero(), ecq_one(), ecq_zero(), ecq_one()}; }
// ecgfp5::is_in_subgroup for canonical words: the neutral, or on the curve x = u^2 (x^2 + 2 x + 263 z) with x not a square
GL_D bool ec_in_subgroup(const EcAffine& a) {
    const bool x0 = ecq_is_zero(a.x), u0 = ecq_is_zero(a.u);
    if (x0 || u0) return x0 && u0;
    EcFq w = p2::q5_add<p2::FBase>(p2::q5_mul<p2::FBase>(a.x, a.x), p2::q5_dbl<p2::FBase>(a.x));
    w.c[1] = gl::add(w.c[1], p2::EG_B1);
    if (!ecq_eq(p2::q5_mul<p2::FBase>(p2::q5_mul<p2::FBase>(a.u, a.u), w), a.x)) return false;
    const u64 nrm = ecq_norm(a.x);  // not 0: x is not 0
    return gl::pow(nrm, (gl::P - 1) / 2) != 1;
}
GL_D EcAffine ec_load_affine(const u64* p) { return EcAffine{ecq_load(p), ecq_load(p + 5)}; }
GL_D EcAffine ec_from_words(const EcWords& g) {
    EcAffine a;
#pragma unroll
    for (int i = 0; i < 5; i++) a.x.c[i] = g.w[i], a.u.c[i] = g.w[5 + i];
    return a;
}
GL_D void ec_store_affine(u64* out, const EcAffine& a) {
#pragma unroll
    for (int i = 0; i < 5; i++) out[i] = a.x.c[i], out[5 + i] = a.u.c[i];
}
// k q for the 320-bit scalar at k[0..5) (global memory), as Point::mul: most significant bit first, acc <- 2 acc + bit q
GL_D EcProj ec_ladder(const u64* __restrict__ k, const EcAffine& q) {
    EcProj acc = ec_neutral();
#pragma nounroll
    for (int limb = 4; limb >= 0; limb--) {
        const u64 w = k[limb];
#pragma nounroll
        for (int j = 63; j >= 0; j--) {
            const u64 bit = (w >> j) & 1;
            acc = p2::ec_add_mixed<p2::FBase>(p2::ec_double<p2::FBase>(acc), ecq_masked(q.x, bit), ecq_masked(q.u, bit));
        }
    }
    return acc;
}
// hash_n_to_hash_no_pad(r.x | r.u | pk.x | pk.u | msg): the sponge of PoseidonTree::hash_or_noop over 20 + msg_len words (always
// more than four).  r and pk are in registers: their words are blocks 0, 1 and half of block 2, picked with constant indices
// once the block loop's body is unrolled over a block's eight words; the message comes from global memory.
GL_D void schnorr_challenge(const EcAffine& r, const EcAffine& pk, const u64* __restrict__ msg, u32 msg_len, u64 e[4]) {
    u64 rw[24];
#pragma unroll
    for (int i = 0; i < 5; i++) rw[i] = r.x.c[i], rw[5 + i] = r.u.c[i], rw[10 + i] = pk.x.c[i], rw[15 + i] = pk.u.c[i];
#pragma unroll
    for (int i = 20; i < 24; i++) rw[i] = 0;
    u64 st[12];
#pragma unroll
    for (int i = 0; i < 12; i++) st[i] = 0;
    const u32 len = 20 + msg_len;
#pragma nounroll
    for (u32 off = 0; off < len; off += 8) {
        const u32 n = min(8u, len - off);
#pragma unroll
        for (u32 i = 0; i < 8; i++) {
            if (i >= n) continue;  // overwrite mode: a short last chunk keeps the state's other rate words
            u64 v;
            if (off == 0) v = rw[i];
            else if (off == 8) v = rw[8 + i];
            else if (off == 16 && i < 4) v = rw[16 + i];
            else v = msg[off + i - 20];
            st[i] = v;
        }
        glf::poseidon_sparse(st);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) e[i] = st[i];
}
GL_D bool words_canonical(const u64* __restrict__ w, u32 n) {
    bool c = true;
    for (u32 i = 0; i < n; i++) c &= w[i] < gl::P;
    return c;
}

// out[i] = k[i] P[i], affine.  status 0, or 2 (output zeroed) for a P[i] with a word not below p or outside the group.
__global__ __launch_bounds__(64) void k_ec_mul_batch(const u64* __restrict__ k, const u64* __restrict__ p, size_t count, u64* __restrict__ out, int* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const EcAffine q = ec_load_affine(p + 10 * i);
    u64* o = out + 10 * i;
    if (!ecq_canonical(q.x) || !ecq_canonical(q.u) || !ec_in_subgroup(q)) {
#pragma unroll
        for (int w = 0; w < 10; w++) o[w] = 0;
        status[i] = 2;
        return;
    }
    ec_store_affine(o, ec_affine(ec_ladder(k + 5 * i, q)));
    status[i] = 0;
}

// sig[i] = Sign(sk[i], msg[i], nonce[i]); pk[i] = sk[i] G where pk is not null.  status 0, or 2 (sig and pk rows zeroed) for a
// secret key or nonce outside [1, n) or a message word not below p.
__global__ __launch_bounds__(64) void k_schnorr_sign(const u64* __restrict__ sk, const u64* __restrict__ nonce, const u64* __restrict__ msg, u32 msg_len, size_t count,
                                                     EcWords gen, u64* __restrict__ sig, u64* __restrict__ pk, int* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    u64 a[5], k[5];
#pragma unroll
    for (int w = 0; w < 5; w++) a[w] = sk[5 * i + w], k[w] = nonce[5 * i + w];
    const u64* m = msg + i * (size_t)msg_len;
    u64* o = sig + 9 * i;
    const bool ok = !p2::ecsc::sc_is_zero(a) && p2::ecsc::sc_below_order(a) && !p2::ecsc::sc_is_zero(k) && p2::ecsc::sc_below_order(k) && words_canonical(m, msg_len);
    if (!ok) {
#pragma unroll
        for (int w = 0; w < 9; w++) o[w] = 0;
        if (pk) {
#pragma unroll
            for (int w = 0; w < 10; w++) pk[10 * i + w] = 0;
        }
        status[i] = 2;
        return;
    }
    const EcAffine g = ec_from_words(gen);
    const EcAffine pub = ec_affine(ec_ladder(sk + 5 * i, g));
    if (pk) ec_store_affine(pk + 10 * i, pub);
    const EcAffine r = ec_affine(ec_ladder(nonce + 5 * i, g));
    u64 e[5];
    schnorr_challenge(r, pub, m, msg_len, e);
    e[4] = 0;
    u64 s[5];
    p2::ecsc::sc_muladd(e, a, k, s);
#pragma unroll
    for (int w = 0; w < 5; w++) o[w] = s[w];
#pragma unroll
    for (int w = 0; w < 4; w++) o[5 + w] = e[w];
    status[i] = 0;
}

// status[i] = Verify(pk[i], msg[i], sig[i]): 0 accepted, 1 rejected, 2 malformed.  s G + e (-pk) is one joint ladder: per bit one
// doubling and the mixed additions of bit_s G and bit_e (-pk), the second only for the low 256 bits, where e has bits.
__global__ __launch_bounds__(64) void k_schnorr_verify(const u64* __restrict__ pk, const u64* __restrict__ msg, u32 msg_len, const u64* __restrict__ sig, size_t count,
                                                       EcWords gen, int* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const u64* sg = sig + 9 * i;
    const u64* m = msg + i * (size_t)msg_len;
    const u64* pkw = pk + 10 * i;
    u64 s[5];
#pragma unroll
    for (int w = 0; w < 5; w++) s[w] = sg[w];
    EcAffine q = ec_load_affine(pkw);
    bool ok = p2::ecsc::sc_below_order(s) && words_canonical(sg + 5, 4) && words_canonical(m, msg_len) && ecq_canonical(q.x) && ecq_canonical(q.u);
    ok = ok && !(ecq_is_zero(q.x) && ecq_is_zero(q.u)) && ec_in_subgroup(q);
    if (!ok) {
        status[i] = 2;
        return;
    }
    const EcAffine pub = q;
    q.u = ecq_neg(q.u);
    const EcAffine g = ec_from_words(gen);
    EcProj acc = ec_neutral();
#pragma nounroll
    for (int limb = 4; limb >= 0; limb--) {
        const u64 ws = sg[limb], we = limb < 4 ? sg[5 + limb] : 0;
#pragma nounroll
        for (int j = 63; j >= 0; j--) {
            const u64 bs = (ws >> j) & 1, be = (we >> j) & 1;
            acc = p2::ec_add_mixed<p2::FBase>(p2::ec_double<p2::FBase>(acc), ecq_masked(g.x, bs), ecq_masked(g.u, bs));
            if (limb < 4) acc = p2::ec_add_mixed<p2::FBase>(acc, ecq_masked(q.x, be), ecq_masked(q.u, be));
        }
    }
    u64 e[4];
    schnorr_challenge(ec_affine(acc), pub, m, msg_len, e);
    bool same = true;
#pragma unroll
    for (int w = 0; w < 4; w++) same &= e[w] == sg[5 + w];
    status[i] = same ? 0 : 1;
}

// test entry: out[i] = (a[i] b[i] + c[i]) mod n
__global__ __launch_bounds__(64) void k_ec_scalar_muladd(const u64* __restrict__ a, const u64* __restrict__ b, const u64* __restrict__ c, size_t count, u64* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    u64 x[5], y[5], z[5], r[5];
#pragma unroll
    for (int w = 0; w < 5; w++) x[w] = a[5 * i + w], y[w] = b[5 * i + w], z[w] = c[5 * i + w];
    p2::ecsc::sc_muladd(x, y, z, r);
#pragma unroll
    for (int w = 0; w < 5; w++) out[5 * i + w] = r[w];
}

}  // namespace p2k
