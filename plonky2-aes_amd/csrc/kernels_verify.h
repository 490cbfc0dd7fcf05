// Batched proof verification on the device (p2_verify_batch, include/p2aes.h): the checks of verifier.h::verify_proof for a
// chunk of proofs of one circuit, in five launches.
//
//   k_vfy_unpack      every word and every sibling-count byte of every proof, one coalesced pass: the byte offsets come from a
//                     per-circuit table (the fixed layout of DESIGN.md section 8), so no address depends on proof contents.
//                     Writes the words 8-byte aligned ([proof][W]) and flags SHAPE (a count byte that differs from the depth
//                     the circuit implies) and NON_CANONICAL (a word >= p).
//   k_vfy_transcript  Fiat-Shamir, a 16-lane group per proof (DevChallenger / glf::poseidon_coop, as the prover's k_challenger),
//                     observing straight from the unpacked proof; checks the proof-of-work response against pow_bits (the
//                     prover discards it) and reduces the query indices mod the LDE size.
//   k_vfy_vanishing   one workgroup per proof: the vanishing identity at zeta in GF(p^2), term for term as the host verifier
//                     (Z(1), partial-product chunks, lookup terms, gate constraints with selector filters); each LUT's
//                     delta-folded accumulation is split over the workgroup.  Also the opening reductions the queries need.
//   k_vfy_queries     a thread per (proof, query, slot), slot = one of the four initial trees | one FRI round | the final
//                     polynomial, so that every Poseidon chain of a query runs at once.  A round slot re-derives the value its
//                     fold check expects from the previous round's evaluations (or fri_combine_initial for round 0); the
//                     first failing check is kept per proof with an atomic min over (query, slot, check).
//   k_vfy_finish      one status per proof in the host verifier's order.
#pragma once
#include "../../include/p2aes.h"
#include "kernels.h"

namespace p2k {

// VF_INDICES: a compressed proof's written query indices differ from the drawn ones (kernels_compress.h), SHAPE after POW
enum VerifyFlag : u32 { VF_SHAPE = 1, VF_NONCANON = 2, VF_POW = 4, VF_ZETA = 8, VF_VANISH = 16, VF_INDICES = 32 };
static const u32 VQ_WORDS = 8;        // per proof: red0, red1, g*zeta, fri_alpha^|e1| (extension elements)
static const u32 VFY_MAX_ROUNDS = 8;  // as CH_FRI_BETAS
static const u32 VFY_ARITY_BITS = 4;  // FriReductionStrategy::ConstantArityBits(4, 5): checked on the host
static const u32 VFY_ARITY = 1u << VFY_ARITY_BITS;
static const u32 VFY_MAX_GC = 123;    // PoseidonGate, the most constraints of any gate

struct VerifyArgs {
    const uint8_t* proofs;  // [batch][proof_bytes]
    size_t proof_bytes;
    u64* words;             // [batch][W] unpacked words
    u32 W, n_cnt, batch;
    const u32* word_off;    // [W] byte offset of word i
    const u32* cnt_off;     // [n_cnt] byte offset of each sibling-count byte
    const uint8_t* cnt_exp; // [n_cnt] the depth the circuit implies
    u32* flags;             // [batch] VF_* bits
    u32* qfail;             // [batch] smallest failing (query, slot, check) key, ~0 if none
    u64* chal;              // [batch][CH_WORDS]
    u64* vq;                // [batch][VQ_WORDS]
    const u64* vd;          // constants_sigmas cap (4 * 2^cap_height) || circuit digest (4)
    int* status;            // [batch] P2_VERIFY_*
    // layout (word indices into one unpacked proof)
    u32 cap_words, fri_caps_off, final_off, final_len, pow_off;
    u32 o_const, o_sig, o_wires, o_zs, o_zsn, o_lk, o_lkn, o_pp, o_quot;
    u32 q_off, q_stride;
    u32 init_eval_off[4], init_width[4], init_sib_off[4], init_depth;
    u32 step_eval_off[VFY_MAX_ROUNDS], step_sib_off[VFY_MAX_ROUNDS], step_depth[VFY_MAX_ROUNDS];
    const u32* obs_map;     // word index of every extension element of the opening batches, batch 0 then batch 1
    u32 n_b0, n_b1;
    // circuit
    u32 degree_bits, lde_bits, cap_height, pow_bits, num_queries, num_rounds, has_lookup;
    u32 R, num_wires, NC, npp, qdf, nlp, nsldc, lut_deg, nsel, nls, ngc, nzpp, zc;
    u32 num_gates, gate_kind[p2::MAX_GATE_TYPES], gate_sel[p2::MAX_GATE_TYPES], group_lo[p2::MAX_GATE_TYPES], group_hi[p2::MAX_GATE_TYPES];
    u32 num_luts;
    const u32* lut_pairs;    // input | output << 16, LUT after LUT
    const u32* lut_offsets;  // [num_luts + 1]
    const u64* k_is;         // [R]
    // public inputs (k >= 1 only): the count word's byte offset (compared with num_pi, never unpacked: it is not a field
    // element) and the values' word index; the transcript leaves hash_no_pad(values) in pi_hash for the vanishing check
    u32 num_pi, pi_cnt_byte, pi_off;
    u64* pi_hash;            // [batch][4]
};

__device__ __forceinline__ u64 vfy_ld_bytes(const uint8_t* p) {
    u64 v = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) v |= (u64)p[i] << (8 * i);
    return v;
}
__device__ __forceinline__ E2 vfy_e2(const u64* w, u32 idx) { return gl::e2(w[idx], w[idx + 1]); }

// ------------------------------------------------------------------------------------------- 1. shape and canonicality
__global__ __launch_bounds__(256) void k_vfy_unpack(VerifyArgs a) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x, p = blockIdx.y;
    const uint8_t* pr = a.proofs + (size_t)p * a.proof_bytes;
    if (i < a.W) {
        const u64 v = vfy_ld_bytes(pr + a.word_off[i]);
        a.words[(size_t)p * a.W + i] = v;
        if (v >= gl::P) atomicOr(&a.flags[p], (u32)VF_NONCANON);
    }
    if (i < a.n_cnt && pr[a.cnt_off[i]] != a.cnt_exp[i]) atomicOr(&a.flags[p], (u32)VF_SHAPE);
    if (i == 0 && a.num_pi && vfy_ld_bytes(pr + a.pi_cnt_byte) != (u64)a.num_pi) atomicOr(&a.flags[p], (u32)VF_SHAPE);  // "wrong number of public inputs"
}

// ------------------------------------------------------------------------------------------- 2. transcript
__global__ __launch_bounds__(64) void k_vfy_transcript(VerifyArgs a) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    const bool real = (t >> 4) < a.batch;
    const u32 p = real ? (t >> 4) : a.batch - 1;  // a group past the end replays the last proof without storing
    DevChallenger c;
    c.i = t & 15;
    c.gbase = (int)(threadIdx.x & 63) & ~15;
    c.w = c.inb = c.outb = 0;
    c.in_len = c.out_len = 0;
    const bool writer = real && c.i == 0;
    const u64* w = a.words + (size_t)p * a.W;
    u64* ch = a.chal + (size_t)p * CH_WORDS;
    for (int i = 0; i < 4; i++) c.observe(a.vd[a.cap_words + i]);  // circuit digest
    if (a.num_pi) {
        // public_inputs_hash = hash_no_pad(values) on the group's sponge (overwrite mode, rate 8), then observed
        u64 s = 0;
        for (u32 off = 0; off < a.num_pi; off += 8) {
            if (c.i < 8 && off + c.i < a.num_pi) s = w[a.pi_off + off + c.i];
            s = glf::poseidon_coop(s, c.i);
        }
        for (int i = 0; i < 4; i++) {
            const u64 h = glf::shfl64(s, c.gbase + i);
            c.observe(h);
            if (writer) a.pi_hash[(size_t)p * 4 + i] = h;
        }
    } else {
        for (int i = 0; i < 4; i++) c.observe(0);  // hash of zero public inputs
    }
    for (u32 i = 0; i < a.cap_words; i++) c.observe(w[i]);          // wires cap
    u64 bg[4], dl[4];
    for (int i = 0; i < 4; i++) bg[i] = c.challenge();  // betas, gammas
    if (a.has_lookup)
        for (int i = 0; i < 4; i++) dl[i] = c.challenge();
    for (u32 i = 0; i < a.cap_words; i++) c.observe(w[a.cap_words + i]);  // zs cap
    const u64 al0 = c.challenge(), al1 = c.challenge();
    for (u32 i = 0; i < a.cap_words; i++) c.observe(w[2 * a.cap_words + i]);  // quotient cap
    const u64 z0 = c.challenge(), z1 = c.challenge();
    for (u32 e = 0; e < a.n_b0 + a.n_b1; e++) {
        const u32 k = a.obs_map[e];
        c.observe(w[k]);
        c.observe(w[k + 1]);
    }
    const u64 fa0 = c.challenge(), fa1 = c.challenge();
    if (writer) {
        for (int i = 0; i < 2; i++) ch[CH_BETAS + i] = bg[i], ch[CH_GAMMAS + i] = bg[2 + i];
        if (a.has_lookup)
            for (int i = 0; i < 4; i++) ch[CH_DELTAS + i] = bg[i], ch[CH_DELTAS + 4 + i] = dl[i];
        ch[CH_ALPHAS] = al0, ch[CH_ALPHAS + 1] = al1;
        ch[CH_ZETA] = z0, ch[CH_ZETA + 1] = z1;
        ch[CH_FRI_ALPHA] = fa0, ch[CH_FRI_ALPHA + 1] = fa1;
    }
    for (u32 r = 0; r < a.num_rounds; r++) {
        const u64* cap = w + a.fri_caps_off + (size_t)r * a.cap_words;
        for (u32 i = 0; i < a.cap_words; i++) c.observe(cap[i]);
        const u64 b0 = c.challenge(), b1 = c.challenge();
        if (writer) ch[CH_FRI_BETAS + 2 * r] = b0, ch[CH_FRI_BETAS + 2 * r + 1] = b1;
    }
    for (u32 i = 0; i < 2 * a.final_len; i++) c.observe(w[a.final_off + i]);
    c.observe(w[a.pow_off]);
    const u64 resp = c.challenge();
    if (writer && (resp >> (64 - a.pow_bits)) != 0) atomicOr(&a.flags[p], (u32)VF_POW);
    const u64 N = (u64)1 << a.lde_bits;
    for (u32 q = 0; q < a.num_queries; q++) {
        const u64 v = c.challenge() % N;
        if (writer) ch[CH_QUERY + q] = v;
    }
}

// ------------------------------------------------------------------------------------------- 3. vanishing identity at zeta
// The vanishing polynomial of challenge i is sum_k term_k alpha_i^k over ONE term list (Z(1) terms, partial-product chunks,
// lookup terms, gate constraints -- each group for both challenges in turn), accumulated as the terms are produced.
// (num_challenges = 2 is checked on the host; two named accumulators keep everything in registers)
struct VanAcc {
    E2 acc0, acc1;
    u64 apow0, apow1, alpha0, alpha1;
    __device__ __forceinline__ void push(E2 t) {
        acc0 = gl::add(acc0, gl::mul(t, apow0));
        acc1 = gl::add(acc1, gl::mul(t, apow1));
        apow0 = gl::mul(apow0, alpha0);
        apow1 = gl::mul(apow1, alpha1);
    }
};

// PoseidonGate's 123 constraints in GF(p^2) for the one working lane of k_vfy_vanishing: the constraint sequence of
// poseidon_gate_constraints<FExt> (poseidon_gate.h), with the permutation state and the MDS output in LDS (`st`, `tmp`,
// twelve elements each) instead of private arrays -- the MDS gathers st[(i + r) % 12], an index the compiler keeps dynamic,
// which would put 24-word private arrays in scratch memory.
__device__ __constant__ static const u32 VFY_MDS_CIRC[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
template <class WireFn, class EmitFn>
__device__ __forceinline__ void vfy_poseidon_gate(WireFn wire, EmitFn emit, E2* st, E2* tmp) {
    auto constants = [&](int round) {
        for (int i = 0; i < 12; i++) st[i] = gl::add(st[i], gl::e2(gl::poseidon_rc(12 * round + i)));
    };
    auto sbox = [](E2 x) {
        const E2 x2 = gl::mul(x, x), x3 = gl::mul(x2, x), x4 = gl::mul(x2, x2);
        return gl::mul(x3, x4);
    };
    auto mds = [&]() {
        for (int r = 0; r < 12; r++) {
            E2 acc = gl::e2(0);
            for (int i = 0; i < 12; i++) {
                const int j = i + r < 12 ? i + r : i + r - 12;
                acc = gl::add(acc, gl::mul(st[j], (u64)VFY_MDS_CIRC[i]));
            }
            if (r == 0) acc = gl::add(acc, gl::mul(st[0], (u64)8));
            tmp[r] = acc;
        }
        for (int i = 0; i < 12; i++) st[i] = tmp[i];
    };
    int k = 0;
    const E2 swap = wire(p2::PG_SWAP);
    emit(k++, gl::mul(swap, gl::sub(swap, gl::e2(1))));
    for (int i = 0; i < 4; i++) {
        const E2 lhs = wire(p2::PG_IN + i), rhs = wire(p2::PG_IN + i + 4), d = wire(p2::PG_DELTA + i);
        emit(k++, gl::sub(gl::mul(swap, gl::sub(rhs, lhs)), d));
        st[i] = gl::add(lhs, d);
        st[i + 4] = gl::sub(rhs, d);
    }
    for (int i = 8; i < 12; i++) st[i] = wire(p2::PG_IN + i);
    int round = 0;
    for (int r = 0; r < 4; r++, round++) {
        constants(round);
        if (r != 0)
            for (int i = 0; i < 12; i++) {
                const E2 sin = wire(p2::PG_FULL0 + 12 * (r - 1) + i);
                emit(k++, gl::sub(st[i], sin));
                st[i] = sin;
            }
        for (int i = 0; i < 12; i++) st[i] = sbox(st[i]);
        mds();
    }
    for (int r = 0; r < 22; r++, round++) {
        constants(round);
        const E2 sin = wire(p2::PG_PARTIAL + r);
        emit(k++, gl::sub(st[0], sin));
        st[0] = sbox(sin);
        mds();
    }
    for (int r = 0; r < 4; r++, round++) {
        constants(round);
        for (int i = 0; i < 12; i++) {
            const E2 sin = wire(p2::PG_FULL1 + 12 * r + i);
            emit(k++, gl::sub(st[i], sin));
            st[i] = sin;
        }
        for (int i = 0; i < 12; i++) st[i] = sbox(st[i]);
        mds();
    }
    for (int i = 0; i < 12; i++) emit(k++, gl::sub(st[i], wire(p2::PG_OUT + i)));
}

// The opening reductions fri_combine_initial needs: red0, red1, g*zeta, fri_alpha^|e1| into vq (also k_cmp_reductions)
__device__ __forceinline__ void vfy_opening_reductions(const VerifyArgs& a, u32 p, const u64* w, const u64* ch, E2 zeta) {
    const E2 fa = gl::e2(ch[CH_FRI_ALPHA], ch[CH_FRI_ALPHA + 1]);
    E2 r0 = gl::e2(0), r1 = gl::e2(0);
    for (u32 e = a.n_b0; e-- > 0;) r0 = gl::add(gl::mul(r0, fa), vfy_e2(w, a.obs_map[e]));
    for (u32 e = a.n_b1; e-- > 0;) r1 = gl::add(gl::mul(r1, fa), vfy_e2(w, a.obs_map[a.n_b0 + e]));
    const E2 gz = gl::mul(zeta, gl::root_of_unity((int)a.degree_bits));
    const E2 ap = gl::pow(fa, (u64)(a.NC + a.zc - a.nzpp));
    u64* o = a.vq + (size_t)p * VQ_WORDS;
    o[0] = r0.a, o[1] = r0.b, o[2] = r1.a, o[3] = r1.b, o[4] = gz.a, o[5] = gz.b, o[6] = ap.a, o[7] = ap.b;
}

// HAS_EC: the gate list may hold an EcStepGate (k_vfy_ecvanishing below); k_vfy_vanishing is the body without that branch.
template <bool HAS_EC>
__device__ __forceinline__ void vfy_vanishing_body(const VerifyArgs& a) {
    __shared__ u64 red[256];
    __shared__ u64 lutacc[2][p2::MAX_LUTS];
    __shared__ E2 gate[VFY_MAX_GC];
    __shared__ E2 pg_st[12], pg_tmp[12];
    const u32 p = blockIdx.x, tid = threadIdx.x;
    const u64* w = a.words + (size_t)p * a.W;
    const u64* ch = a.chal + (size_t)p * CH_WORDS;
    // each LUT's accumulation acc = sum_k e_k d3^(total-1-k), e_k = in_k + d1 out_k (0 on the padding of the last row):
    // contiguous blocks per thread, each Horner-folded and shifted by d3^(entries after the block)
    if (a.has_lookup) {
        for (u32 i = 0; i < a.NC; i++) {
            const u64 d1 = ch[CH_DELTAS + 4 * i + 1], d3 = ch[CH_DELTAS + 4 * i + 3];
            for (u32 l = 0; l < a.num_luts; l++) {
                const u32 lo = a.lut_offsets[l], size = a.lut_offsets[l + 1] - lo;
                const u32 total = (size + p2::LUT_SLOTS - 1) / p2::LUT_SLOTS * p2::LUT_SLOTS;
                const u32 per = (total + blockDim.x - 1) / blockDim.x;
                const u32 b0 = min(tid * per, total), b1 = min(b0 + per, total);
                u64 h = 0;
                for (u32 k = b0; k < b1; k++) {
                    u64 e = 0;
                    if (k < size) {
                        const u32 pr = a.lut_pairs[lo + k];
                        e = gl::add((u64)(pr & 0xFFFF), gl::mul(d1, (u64)(pr >> 16)));
                    }
                    h = gl::add(gl::mul(h, d3), e);
                }
                red[tid] = gl::mul(h, gl::pow(d3, total - b1));
                __syncthreads();
                for (u32 s = blockDim.x / 2; s > 0; s >>= 1) {
                    if (tid < s) red[tid] = gl::add(red[tid], red[tid + s]);
                    __syncthreads();
                }
                if (tid == 0) lutacc[i][l] = red[0];
                __syncthreads();
            }
        }
    }
    for (u32 k = tid; k < a.ngc; k += blockDim.x) gate[k] = gl::e2(0);
    __syncthreads();
    const E2 zeta = gl::e2(ch[CH_ZETA], ch[CH_ZETA + 1]);
    if (tid == 64) vfy_opening_reductions(a, p, w, ch, zeta);  // a second wave: what fri_combine_initial needs (k_vfy_queries)
    if (tid != 0) return;
    const u32 NC = a.NC, R = a.R, npp = a.npp, qdf = a.qdf, nlp = a.nlp, nsldc = a.nsldc;
    const E2 zpn = gl::exp_pow2(zeta, (int)a.degree_bits);
    const E2 zh = gl::sub(zpn, gl::e2(1));
    if (gl::eq(zpn, gl::e2(1))) atomicOr(&a.flags[p], (u32)VF_ZETA);
    const u64 n = (u64)1 << a.degree_bits;
    const E2 l0 = gl::mul(zh, gl::inv(gl::mul(gl::sub(zeta, gl::e2(1)), n % gl::P)));
    VanAcc V;
    V.acc0 = V.acc1 = gl::e2(0);
    V.apow0 = V.apow1 = 1;
    V.alpha0 = ch[CH_ALPHAS], V.alpha1 = ch[CH_ALPHAS + 1];
    auto wire = [&](u32 k) { return vfy_e2(w, a.o_wires + 2 * k); };
    // Z(1) = 1
    for (u32 i = 0; i < NC; i++) V.push(gl::mul(l0, gl::sub(vfy_e2(w, a.o_zs + 2 * i), gl::e2(1))));
    // partial-product chunks
    for (u32 i = 0; i < NC; i++) {
        const u64 beta = ch[CH_BETAS + i], gamma = ch[CH_GAMMAS + i];
        for (u32 chunk = 0; chunk * qdf < R; chunk++) {
            E2 num = gl::e2(1), den = gl::e2(1);
            for (u32 j = chunk * qdf; j < min(R, (chunk + 1) * qdf); j++) {
                const E2 wj = wire(j);
                num = gl::mul(num, gl::add(gl::add(wj, gl::mul(zeta, gl::mul(beta, a.k_is[j]))), gl::e2(gamma)));
                den = gl::mul(den, gl::add(gl::add(wj, gl::mul(vfy_e2(w, a.o_sig + 2 * j), beta)), gl::e2(gamma)));
            }
            const E2 prev = chunk == 0 ? vfy_e2(w, a.o_zs + 2 * i) : vfy_e2(w, a.o_pp + 2 * (i * npp + chunk - 1));
            const E2 next = chunk == npp ? vfy_e2(w, a.o_zsn + 2 * i) : vfy_e2(w, a.o_pp + 2 * (i * npp + chunk));
            V.push(gl::sub(gl::mul(prev, num), gl::mul(next, den)));
        }
    }
    // lookup terms
    if (nlp) {
        for (u32 i = 0; i < NC; i++) {
            const u64* d = ch + CH_DELTAS + 4 * i;
            const u32 lz = a.o_lk + 2 * i * nlp, lzn = a.o_lkn + 2 * i * nlp, sel = a.o_const + 2 * a.nsel;
            auto SEL = [&](u32 k) { return vfy_e2(w, sel + 2 * k); };
            auto SL = [&](u32 k) { return vfy_e2(w, lz + 2 * (1 + k)); };
            auto SLN = [&](u32 k) { return vfy_e2(w, lzn + 2 * (1 + k)); };
            auto looked = [&](u32 s) { return gl::add(wire(3 * s), gl::mul(wire(3 * s + 1), d[0])); };
            auto lookup = [&](u32 s) { return gl::add(wire(3 * s), gl::mul(wire(3 * s + 1), d[1])); };
            auto looking = [&](u32 s) { return gl::add(wire(2 * s), gl::mul(wire(2 * s + 1), d[0])); };
            const E2 LZ = vfy_e2(w, lz), LZN = vfy_e2(w, lzn);
            const u32 lu_deg = qdf - 1, lut_deg = a.lut_deg;
            V.push(gl::mul(SEL(3), SL(nsldc - 1)));
            V.push(gl::mul(SEL(2), SL(0)));
            V.push(gl::mul(SEL(2), LZ));
            for (u32 l = 0; l < a.num_luts; l++) V.push(gl::mul(SEL(4 + l), gl::sub(LZ, gl::e2(lutacc[i][l]))));
            E2 cur = LZN;
            for (u32 s = 0; s < p2::LUT_SLOTS; s++) cur = gl::add(gl::mul(cur, d[3]), lookup(s));
            V.push(gl::mul(SEL(0), gl::sub(LZ, cur)));
            const E2 alpha_e = gl::e2(d[2]);
            for (u32 poly = 0; poly < nsldc; poly++) {
                const u32 a0 = poly * lut_deg, a1 = min((poly + 1) * lut_deg, p2::LUT_SLOTS);
                const u32 b0 = poly * lu_deg, b1 = min((poly + 1) * lu_deg, p2::LU_SLOTS);
                E2 lut_prod = gl::e2(1), lu_prod = gl::e2(1), lu_sum = gl::e2(0), lut_sum_mul = gl::e2(0);
                for (u32 k = a0; k < a1; k++) lut_prod = gl::mul(lut_prod, gl::sub(alpha_e, looked(k)));
                for (u32 k = b0; k < b1; k++) lu_prod = gl::mul(lu_prod, gl::sub(alpha_e, looking(k)));
                for (u32 k = b0; k < b1; k++) {
                    E2 pr = gl::e2(1);
                    for (u32 m = b0; m < b1; m++)
                        if (m != k) pr = gl::mul(pr, gl::sub(alpha_e, looking(m)));
                    lu_sum = gl::add(lu_sum, pr);
                }
                for (u32 k = a0; k < a1; k++) {
                    E2 pr = gl::e2(1);
                    for (u32 m = a0; m < a1; m++)
                        if (m != k) pr = gl::mul(pr, gl::sub(alpha_e, looked(m)));
                    lut_sum_mul = gl::add(lut_sum_mul, gl::mul(wire(3 * k + 2), pr));
                }
                const E2 prev = poly == 0 ? SLN(nsldc - 1) : SL(poly - 1);
                const E2 diff = gl::sub(SL(poly), prev);
                V.push(gl::mul(SEL(0), gl::sub(gl::mul(lut_prod, diff), lut_sum_mul)));
                V.push(gl::mul(SEL(1), gl::add(gl::mul(lu_prod, diff), lu_sum)));
            }
        }
    }
    // gate constraints, filtered by their selector
    const u32 gc = a.o_const + 2 * (a.nsel + a.nls);
    for (u32 gi = 0; gi < a.num_gates; gi++) {
        const u32 kind = a.gate_kind[gi];
        if (kind != p2::G_ARITHMETIC && kind != p2::G_CONSTANT && kind != p2::G_PUBLIC_INPUT && kind != p2::G_POSEIDON && !(HAS_EC && kind == p2::G_ECSTEP)) continue;  // no constraints
        const E2 s = vfy_e2(w, a.o_const + 2 * a.gate_sel[gi]);
        E2 filter = gl::e2(1);
        for (u32 j = a.group_lo[gi]; j < a.group_hi[gi]; j++)
            if (j != gi) filter = gl::mul(filter, gl::sub(gl::e2(j), s));
        if (a.nsel > 1) filter = gl::mul(filter, gl::sub(gl::e2(p2::UNUSED_SELECTOR), s));
        if (kind == p2::G_ARITHMETIC) {
            const E2 c0 = vfy_e2(w, gc), c1 = vfy_e2(w, gc + 2);
            for (u32 op = 0; op < p2::ARITH_OPS; op++) {
                const E2 c = gl::sub(wire(4 * op + 3), gl::add(gl::mul(gl::mul(wire(4 * op), wire(4 * op + 1)), c0), gl::mul(wire(4 * op + 2), c1)));
                gate[op] = gl::add(gate[op], gl::mul(filter, c));
            }
        } else if (kind == p2::G_CONSTANT) {
            for (u32 k = 0; k < 2; k++) gate[k] = gl::add(gate[k], gl::mul(filter, gl::sub(vfy_e2(w, gc + 2 * k), wire(k))));
        } else if (kind == p2::G_PUBLIC_INPUT) {
            for (u32 k = 0; k < 4; k++) {
                const E2 h = gl::e2(a.num_pi ? a.pi_hash[(size_t)p * 4 + k] : 0);
                gate[k] = gl::add(gate[k], gl::mul(filter, gl::sub(wire(k), h)));
            }
        } else if (kind == p2::G_POSEIDON) {
            vfy_poseidon_gate(wire, [&](int k, E2 cst) { gate[k] = gl::add(gate[k], gl::mul(filter, cst)); }, pg_st, pg_tmp);
        } else if (HAS_EC && kind == p2::G_ECSTEP) {
            p2::ecstep_gate_constraints<p2::FExt>(wire, [&](int k, E2 cst) { gate[k] = gl::add(gate[k], gl::mul(filter, cst)); });
        }
    }
    for (u32 k = 0; k < a.ngc; k++) V.push(gate[k]);
    for (u32 i = 0; i < NC; i++) {
        E2 t = gl::e2(0);
        for (u32 c = qdf; c-- > 0;) t = gl::add(gl::mul(t, zpn), vfy_e2(w, a.o_quot + 2 * (i * qdf + c)));
        if (!gl::eq(i == 0 ? V.acc0 : V.acc1, gl::mul(zh, t))) atomicOr(&a.flags[p], (u32)VF_VANISH);
    }
}
__global__ __launch_bounds__(256) void k_vfy_vanishing(VerifyArgs a) { vfy_vanishing_body<false>(a); }
// the same kernel for circuits with EcStepGate rows
__global__ __launch_bounds__(256) void k_vfy_ecvanishing(VerifyArgs a) { vfy_vanishing_body<true>(a); }

// ------------------------------------------------------------------------------------------- 4. queries
// The tree hasher of the circuit's configuration, as the path walks of the verifier (vfy_merkle) and of the compressor
// (cmp_merkle, kernels_compress.h) use it: a policy type per hasher, KeccakTree (kernels_keccak.h) with the same members.
// (glf::poseidon_sparse: the permutation with the sparse partial rounds -- k_vfy_queries' register count is held to that form.)
struct PoseidonTree {
    // the digest of a leaf: the leaf itself if it fits in a digest, else the overwrite-mode sponge
    static __device__ __forceinline__ void hash_or_noop(const u64* in, u32 len, u64* out) {
        if (len <= 4) {
#pragma unroll
            for (int i = 0; i < 4; i++) out[i] = (u32)i < len ? in[i] : 0;
            return;
        }
        u64 st[12];
#pragma unroll
        for (int i = 0; i < 12; i++) st[i] = 0;
        for (u32 off = 0; off < len; off += 8) {
            const u32 k = min(8u, len - off);
#pragma unroll
            for (u32 i = 0; i < 8; i++)
                if (i < k) st[i] = in[off + i];  // overwrite mode: a short last chunk keeps the state's other rate words
            glf::poseidon_sparse(st);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) out[i] = st[i];
    }
    // cur = two_to_one(cur, sib), or two_to_one(sib, cur) for a right child
    static __device__ __forceinline__ void compress(u64* cur, const u64* sib, bool right) {
        u64 st[12];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            st[i] = right ? sib[i] : cur[i];
            st[4 + i] = right ? cur[i] : sib[i];
            st[8 + i] = 0;
        }
        glf::poseidon_sparse(st);
#pragma unroll
        for (int i = 0; i < 4; i++) cur[i] = st[i];
    }
    // whether a stored hash is an accepted encoding: four canonical field elements
    static __device__ __forceinline__ bool valid(const u64* h) { return h[0] < gl::P && h[1] < gl::P && h[2] < gl::P && h[3] < gl::P; }
};

// verify_merkle_to_cap: the leaf's digest climbed with `depth` siblings and compared with cap entry index >> depth
// (vfy_merkle_walk: the same from a digest, with the index type of the caller's tree -- the sparse maps walk 64 bits)
template <class H, class Index>
__device__ __forceinline__ bool vfy_merkle_walk(u64* cur, Index index, const u64* cap, u32 cap_n, const u64* sib, u32 depth) {
    for (u32 l = 0; l < depth; l++) {
        H::compress(cur, sib + 4 * (size_t)l, index & 1);
        index >>= 1;
    }
    const u64* c = cap + 4 * (size_t)(index & (cap_n - 1));
    return index < cap_n && cur[0] == c[0] && cur[1] == c[1] && cur[2] == c[2] && cur[3] == c[3];
}
template <class H>
__device__ __forceinline__ bool vfy_merkle(const u64* leaf, u32 width, u32 index, const u64* cap, u32 cap_n, const u64* sib, u32 depth) {
    u64 cur[4];
    H::hash_or_noop(leaf, width, cur);
    return vfy_merkle_walk<H, u32>(cur, index, cap, cap_n, sib, depth);
}
// compute_evaluation: interpolate the arity-16 coset {(x_t, evals[bitrev t])} containing subgroup_x and evaluate at beta, as the
// host's Lagrange sum.  The nodes are x_t = c g^t (c = coset start, g of order 16), so every denominator has a closed form:
// prod_{m != t} (x_t - x_m) = x_t^15 prod_{k=1..15} (1 - g^k) = 16 x_t^15 = 16 c^16 / x_t -- one inversion for all sixteen.  No
// arrays: x_m is rebuilt by a running product in the inner loop, y_t is read from the proof.
__device__ __forceinline__ E2 vfy_interpolate(const u64* evals, u32 within, u64 subgroup_x, E2 beta) {
    const u64 g = gl::root_of_unity((int)VFY_ARITY_BITS);
    const u32 rev_within = gl::bitrev(within, (int)VFY_ARITY_BITS);
    const u64 coset_start = gl::mul(subgroup_x, gl::pow(g, VFY_ARITY - rev_within));
    const u64 inv_d = gl::inv(gl::mul(VFY_ARITY, gl::exp_pow2(coset_start, (int)VFY_ARITY_BITS)));  // 1 / (16 c^16)
    E2 acc = gl::e2(0);
    u64 xt = coset_start;
    for (u32 t = 0; t < VFY_ARITY; t++) {
        E2 num = gl::e2(1);
        u64 xm = coset_start;
        for (u32 m = 0; m < VFY_ARITY; m++) {
            if (m != t) num = gl::mul(num, gl::sub(beta, gl::e2(xm)));
            xm = gl::mul(xm, g);
        }
        const u32 bt = ((t & 1) << 3) | ((t & 2) << 1) | ((t & 4) >> 1) | ((t & 8) >> 3);  // bitrev(t, 4)
        acc = gl::add(acc, gl::mul(gl::mul(vfy_e2(evals, 2 * bt), num), gl::mul(xt, inv_d)));
        xt = gl::mul(xt, g);
    }
    return acc;
}
// fri_combine_initial: the opening batches at zeta and g*zeta against the initial trees' leaves at subgroup_x
__device__ __forceinline__ E2 vfy_combine_initial(const VerifyArgs& a, const u64* qw, u64 subgroup_x, const u64* ch, const u64* vq) {
    const E2 fa = gl::e2(ch[CH_FRI_ALPHA], ch[CH_FRI_ALPHA + 1]), zeta = gl::e2(ch[CH_ZETA], ch[CH_ZETA + 1]);
    const u64 *e_pre = qw + a.init_eval_off[0], *e_w = qw + a.init_eval_off[1], *e_z = qw + a.init_eval_off[2], *e_q = qw + a.init_eval_off[3];
    // e0 = pre | wires | zs[0, nzpp) | quotient | zs[nzpp, zc);  e1 = zs[0, NC) | zs[nzpp, zc); Horner from the last element
    E2 r0 = gl::e2(0), r1 = gl::e2(0);
    auto fold = [&](E2& r, const u64* v, u32 len) {
        for (u32 k = len; k-- > 0;) r = gl::add(gl::mul(r, fa), gl::e2(v[k]));
    };
    fold(r0, e_z + a.nzpp, a.zc - a.nzpp);
    fold(r0, e_q, a.NC * a.qdf);
    fold(r0, e_z, a.nzpp);
    fold(r0, e_w, a.num_wires);
    fold(r0, e_pre, a.init_width[0]);
    fold(r1, e_z + a.nzpp, a.zc - a.nzpp);
    fold(r1, e_z, a.NC);
    const E2 red0 = gl::e2(vq[0], vq[1]), red1 = gl::e2(vq[2], vq[3]), gz = gl::e2(vq[4], vq[5]), ap = gl::e2(vq[6], vq[7]);
    E2 sum = gl::mul(gl::sub(r0, red0), gl::inv(gl::sub(gl::e2(subgroup_x), zeta)));
    sum = gl::mul(sum, ap);
    return gl::add(sum, gl::mul(gl::sub(r1, red1), gl::inv(gl::sub(gl::e2(subgroup_x), gz))));
}
// The value the fold check of round k expects: fri_combine_initial for k = 0, else round k-1's coset interpolated at its beta.
__device__ __forceinline__ E2 vfy_expected(const VerifyArgs& a, const u64* w, const u64* qw, u32 k, u32 x_index, u64 subgroup_x0, const u64* ch, const u64* vq) {
    if (k == 0) return vfy_combine_initial(a, qw, subgroup_x0, ch, vq);
    const u32 shift = VFY_ARITY_BITS * (k - 1);
    const u64 sx = gl::exp_pow2(subgroup_x0, (int)shift);
    const E2 beta = gl::e2(ch[CH_FRI_BETAS + 2 * (k - 1)], ch[CH_FRI_BETAS + 2 * (k - 1) + 1]);
    return vfy_interpolate(qw + a.step_eval_off[k - 1], (x_index >> shift) & (VFY_ARITY - 1), sx, beta);
}

// slot s of query q: s < 4 initial tree s; 4 <= s < 4 + rounds: FRI round s - 4 (fold check, then Merkle); the last: final poly.
// Failure key ((q * slots + s) << 1 | check): the smallest key is the check verify_proof reports first.
template <class H>
__device__ __forceinline__ void vfy_queries(const VerifyArgs& a) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x, slot = blockIdx.y, slots = gridDim.y;
    if (t >= a.batch * a.num_queries) return;
    const u32 p = t / a.num_queries, q = t % a.num_queries;
    const u64* w = a.words + (size_t)p * a.W;
    const u64* ch = a.chal + (size_t)p * CH_WORDS;
    const u64* vq = a.vq + (size_t)p * VQ_WORDS;
    const u64* qw = w + a.q_off + (size_t)q * a.q_stride;
    const u32 cap_n = 1u << a.cap_height;
    const u32 x_index = (u32)(ch[CH_QUERY + q] & (((u64)1 << a.lde_bits) - 1));
    const u32 key = (q * slots + slot) << 1;
    // the Merkle climb of this slot (an initial tree, or a FRI round after its fold check): one call site, inlined
    const u64 *leaf = nullptr, *cap = nullptr, *sib = nullptr;
    u32 width = 0, index = 0, depth = 0, mkey = key;
    if (slot < 4) {
        cap = slot == 0 ? a.vd : w + (size_t)(slot - 1) * a.cap_words;
        leaf = qw + a.init_eval_off[slot], width = a.init_width[slot], index = x_index, sib = qw + a.init_sib_off[slot], depth = a.init_depth;
    } else {
        const u64 subgroup_x0 = gl::mul(gl::MULT_GEN, gl::pow(gl::root_of_unity((int)a.lde_bits), gl::bitrev(x_index, (int)a.lde_bits)));
        const u32 k = slot - 4;
        const E2 expect = vfy_expected(a, w, qw, k, x_index, subgroup_x0, ch, vq);
        if (k == a.num_rounds) {
            const u64 sx = gl::exp_pow2(subgroup_x0, (int)(VFY_ARITY_BITS * a.num_rounds));
            E2 fe = gl::e2(0);
            for (u32 i = a.final_len; i-- > 0;) fe = gl::add(gl::mul(fe, sx), vfy_e2(w, a.final_off + 2 * i));
            if (!gl::eq(fe, expect)) atomicMin(&a.qfail[p], key);
            return;
        }
        const u32 xk = x_index >> (VFY_ARITY_BITS * k), within = xk & (VFY_ARITY - 1);
        leaf = qw + a.step_eval_off[k];
        if (!gl::eq(vfy_e2(leaf, 2 * within), expect)) {
            atomicMin(&a.qfail[p], key);
            return;
        }
        cap = w + a.fri_caps_off + (size_t)k * a.cap_words, width = 2 * VFY_ARITY, index = xk >> VFY_ARITY_BITS;
        sib = qw + a.step_sib_off[k], depth = a.step_depth[k], mkey = key | 1;
    }
    if (!vfy_merkle<H>(leaf, width, index, cap, cap_n, sib, depth)) atomicMin(&a.qfail[p], mkey);
}
__global__ __launch_bounds__(64) void k_vfy_queries(VerifyArgs a) { vfy_queries<PoseidonTree>(a); }

// ------------------------------------------------------------------------------------------- 5. one status per proof
__global__ void k_vfy_finish(VerifyArgs a, u32 slots) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.batch) return;
    const u32 f = a.flags[p], key = a.qfail[p];
    int st = P2_VERIFY_OK;
    if (f & VF_SHAPE) st = P2_VERIFY_SHAPE;
    else if (f & VF_NONCANON) st = P2_VERIFY_NON_CANONICAL;
    else if (f & VF_POW) st = P2_VERIFY_POW;
    else if (f & VF_INDICES) st = P2_VERIFY_SHAPE;
    else if (f & VF_ZETA) st = P2_VERIFY_ZETA_IN_SUBGROUP;
    else if (f & VF_VANISH) st = P2_VERIFY_VANISHING;
    else if (key != ~0u) {
        const u32 slot = (key >> 1) % slots;
        if (slot < 4) st = P2_VERIFY_MERKLE_INITIAL;
        else if (slot < slots - 1) st = (key & 1) ? P2_VERIFY_MERKLE_FRI : P2_VERIFY_FRI_FOLD;
        else st = P2_VERIFY_FINAL_POLY;
    }
    a.status[p] = st;
}

}  // namespace p2k
