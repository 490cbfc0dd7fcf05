// Compressed proofs on the device (p2_compress_batch, p2_decompress_batch, p2_verify_compressed_batch; include/p2aes.h): the
// conversions of compress.h for a chunk of proofs of one circuit, composed with the verifier kernels of kernels_verify.h.
// Compressed proofs sit at a stride of the full proof size, with a length per proof; the layout is DESIGN.md section 8.
//
//   k_cmp_plan        a workgroup per proof: the layout of its compressed form from its query indices (the written ones, or
//                     the drawn ones when compressing).  A thread per (tree, query) finds the first query with its leaf and
//                     the levels at which the query stores a sibling; the blocks' byte offsets follow by ranking the distinct
//                     leaves.  Checks the length and, reading only below it, every sibling count (SHAPE).
//   k_cmp_scatter     a thread per word of the full layout (a per-circuit table names its source): prefix, leaves, stored
//                     evaluations and tail into the unpacked words of k_vfy_unpack, each checked < p.
//   k_cmp_reductions  the opening reductions of k_vfy_vanishing, for the inferred evaluations
//   k_cmp_infer       a workgroup per proof, a thread per query, round after round: the first query of each coset computes the
//                     evaluation its fold check expects and writes it where the compressed form left it out; the other
//                     queries of the coset copy it.  Also compares the written indices with the drawn ones.
//   k_cmp_merkle      a workgroup per (proof, tree), a thread per query: the leaf digests, then level by level every query's
//                     parent, its sibling taken from its own block where the layout stores one, else from the node of the
//                     query that has it on its path or stored it first (LDS).
//   k_cmp_pack        the unpacked words back to the full byte layout (decompression's output)
//   k_cmp_emit        compression: every word of an unpacked full proof to its place in the compressed layout
//   k_cmp_finish      one status (and length) per proof
// Every read of a compressed proof is at an offset computed from its indices alone, below its checked length.
#pragma once
#include "kernels_verify.h"

namespace p2k {

static const u32 CMP_MAXQ = 32;                     // queries per proof (a workgroup of k_cmp_infer / k_cmp_merkle)
static const u32 CMP_MAXT = 1 + VFY_MAX_ROUNDS;     // trees: 0 = the initial trees (one index set), 1 + r = FRI round r
enum CmpWord : u32 { CW_PREFIX = 0, CW_TAIL = 1, CW_LEAF = 2, CW_EVAL = 3, CW_SIB = 4 };
// per-circuit word table: kind << 28 | query << 22 | slot << 18 | element  (slot: initial tree 0..3, FRI round 4 + r;
// element: leaf word, evaluation word (0..31), or sibling level << 2 | word)
__host__ __device__ __forceinline__ u32 cmp_code(u32 kind, u32 q, u32 slot, u32 e) { return kind << 28 | q << 22 | slot << 18 | e; }

struct CmpPlan {
    u32 idx[CMP_MAXQ];             // query indices
    u32 off[CMP_MAXT][CMP_MAXQ];   // byte offset of the block of the query's first twin (the first query with its leaf)
    u32 mask[CMP_MAXT][CMP_MAXQ];  // levels at which the query stores its sibling (0 for a twin)
    uint8_t rep[CMP_MAXT][CMP_MAXQ];
    u32 len;                       // length of the compressed proof; 0: no layout (SHAPE)
};

struct CmpArgs {
    VerifyArgs v;
    const uint8_t* cproofs;  // [batch][v.proof_bytes] compressed proofs (decompress / verify), or the output (compress)
    uint8_t* cout;           // compress: [batch][v.proof_bytes] compressed; decompress: [batch][v.proof_bytes] full proofs
    const u32* lengths;      // [batch] lengths of the compressed proofs (decompress / verify)
    u32* lengths_out;        // [batch] (compress)
    CmpPlan* plan;           // [batch]
    const u32* wmap;         // [v.W] cmp_code of every word of the full layout
    u32 prefix, tail, cols[4], from_chal;
};

__device__ __forceinline__ u32 cmp_shift(u32 t) { return VFY_ARITY_BITS * t; }
__device__ __forceinline__ u32 cmp_depth(const VerifyArgs& a, u32 t) { return t == 0 ? a.init_depth : a.step_depth[t - 1]; }
__device__ __forceinline__ u32 cmp_block_bytes(const CmpArgs& a, u32 t, u32 kept) {
    if (t == 0) return 8 * (a.cols[0] + a.cols[1] + a.cols[2] + a.cols[3]) + 4 * (1 + 32 * kept);
    return 16 * (VFY_ARITY - 1) + 1 + 32 * kept;
}
// byte offset, within an initial-tree block whose queries store `kept` siblings, of tree o's leaf row
__device__ __forceinline__ u32 cmp_leaf_at(const CmpArgs& a, u32 o, u32 kept) {
    u32 at = 0;
    for (u32 i = 0; i < o; i++) at += 8 * a.cols[i] + 1 + 32 * kept;
    return at;
}
// byte offset, within the block, of the first stored sibling of tree slot s (initial tree s < 4, FRI round s - 4)
__device__ __forceinline__ u32 cmp_sib_at(const CmpArgs& a, u32 s, u32 kept) {
    return s < 4 ? cmp_leaf_at(a, s, kept) + 8 * a.cols[s] + 1 : 16 * (VFY_ARITY - 1) + 1;
}
__device__ __forceinline__ void cmp_st_bytes(uint8_t* p, u64 v) {
#pragma unroll
    for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i));
}

// ------------------------------------------------------------------------------------------- 1. layout
__global__ __launch_bounds__(256) void k_cmp_plan(CmpArgs a) {
    __shared__ u32 s_idx[CMP_MAXQ], s_size[CMP_MAXT][CMP_MAXQ], s_base[CMP_MAXT + 1];
    __shared__ uint8_t s_rep[CMP_MAXT][CMP_MAXQ];
    __shared__ u32 s_ok;
    const VerifyArgs& v = a.v;
    const u32 p = blockIdx.x, tid = threadIdx.x, Q = v.num_queries, T = 1 + v.num_rounds;
    const uint8_t* cp = a.cproofs + (size_t)p * v.proof_bytes;
    CmpPlan& pl = a.plan[p];
    u32 clen = 0;
    if (tid == 0) {
        s_ok = 1;
        if (a.from_chal) {
            s_ok = (v.flags[p] & (VF_SHAPE | VF_NONCANON)) == 0;  // a full proof that cannot be compressed
        } else {
            clen = a.lengths[p];
            s_ok = clen <= v.proof_bytes && clen >= a.prefix + 4 * Q;
        }
    }
    __syncthreads();
    if (tid < Q) {
        u32 x = 0;
        if (a.from_chal) {
            x = (u32)v.chal[(size_t)p * CH_WORDS + CH_QUERY + tid];
        } else if (s_ok) {
            const uint8_t* b = cp + a.prefix + 4 * tid;
            x = (u32)b[0] | (u32)b[1] << 8 | (u32)b[2] << 16 | (u32)b[3] << 24;
        }
        if ((x >> v.lde_bits) != 0) s_ok = 0;  // (a benign race: every writer stores 0)
        s_idx[tid] = x & ((1u << v.lde_bits) - 1);
    }
    __syncthreads();
    const u32 t = tid / CMP_MAXQ, q = tid % CMP_MAXQ;
    const bool mine = t < T && q < Q;
    u32 mask = 0, rep = q, leaf = 0;
    if (mine) {
        const u32 sh = cmp_shift(t), depth = cmp_depth(v, t);
        leaf = s_idx[q] >> sh;
        for (u32 e = 0; e < q; e++)
            if ((s_idx[e] >> sh) == leaf) {
                rep = e;
                break;
            }
        // compress_merkle_proofs: the sibling at level l is stored by q unless some query has it on its path, or an earlier
        // query shares q's node at level l (and so stored it, or had it on its path, first)
        for (u32 l = 0; l < depth; l++) {
            const u32 node = leaf >> l;
            bool known = false;
            for (u32 e = 0; e < Q && !known; e++) {
                const u32 other = (s_idx[e] >> sh) >> l;
                known = other == (node ^ 1) || (e < q && other == node);
            }
            if (!known) mask |= 1u << l;
        }
        s_rep[t][q] = (uint8_t)rep;
        s_size[t][q] = rep == q ? cmp_block_bytes(a, t, __popc(mask)) : 0;
    }
    __syncthreads();
    if (tid == 0) {
        u32 pos = a.prefix + 4 * Q;
        for (u32 tt = 0; tt < T; tt++) {
            s_base[tt] = pos;
            for (u32 e = 0; e < Q; e++) pos += s_size[tt][e];
        }
        s_base[T] = pos + a.tail;
        if (s_base[T] > v.proof_bytes) {  // never longer than the stride (cannot happen with 28 queries under a cap of 16)
            if (s_ok) atomicOr(&v.flags[p], (u32)VF_SHAPE);
            s_ok = 0;
        }
        if (!a.from_chal && s_base[T] != clen) s_ok = 0;
    }
    __syncthreads();
    const u32 len = s_base[T];
    if (mine) {
        const u32 sh = cmp_shift(t);
        u32 off = s_base[t];
        for (u32 e = 0; e < Q; e++)
            if (s_rep[t][e] == e && (s_idx[e] >> sh) < leaf) off += s_size[t][e];
        pl.off[t][q] = off;
        pl.mask[t][q] = mask;
        pl.rep[t][q] = (uint8_t)rep;
        // the sibling counts (below the checked length: every block lies in [prefix, len - tail))
        if (!a.from_chal && s_ok && rep == q) {
            const u32 k = __popc(mask);
            for (u32 o = 0; o < (t == 0 ? 4u : 1u); o++)
                if (cp[off + (t == 0 ? cmp_leaf_at(a, o, k) + 8 * a.cols[o] : 16 * (VFY_ARITY - 1))] != k) atomicOr(&v.flags[p], (u32)VF_SHAPE);
        }
    }
    if (tid < Q) pl.idx[tid] = s_idx[tid];
    if (tid == 0) {
        pl.len = s_ok ? len : 0;
        if (!a.from_chal) {
            if (!s_ok) atomicOr(&v.flags[p], (u32)VF_SHAPE);
            else if (v.num_pi && vfy_ld_bytes(cp + len - a.tail + (v.pi_cnt_byte - (u32)(v.proof_bytes - a.tail))) != (u64)v.num_pi)
                atomicOr(&v.flags[p], (u32)VF_SHAPE);  // "wrong number of public inputs"
        }
    }
}

// ------------------------------------------------------------------------------------------- 2. decompression: words in place
__global__ __launch_bounds__(256) void k_cmp_scatter(CmpArgs a) {
    const VerifyArgs& v = a.v;
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x, p = blockIdx.y;
    const CmpPlan& pl = a.plan[p];
    if (i >= v.W || pl.len == 0) return;
    const u32 code = a.wmap[i], kind = code >> 28, q = (code >> 22) & 63, slot = (code >> 18) & 15, e = code & 0x3FFFF;
    u32 src;
    if (kind == CW_PREFIX) {
        src = v.word_off[i];
    } else if (kind == CW_TAIL) {
        src = pl.len - (u32)(v.proof_bytes - v.word_off[i]);
    } else if (kind == CW_LEAF) {
        src = pl.off[0][q] + cmp_leaf_at(a, slot, __popc(pl.mask[0][pl.rep[0][q]])) + 8 * e;
    } else if (kind == CW_EVAL) {
        const u32 r = slot - 4, rq = pl.rep[1 + r][q], left_out = (pl.idx[rq] >> cmp_shift(r)) & (VFY_ARITY - 1), k = e >> 1;
        if (k == left_out) return;  // k_cmp_infer
        src = pl.off[1 + r][q] + 16 * (k < left_out ? k : k - 1) + 8 * (e & 1);
    } else {
        return;  // siblings: k_cmp_merkle
    }
    const u64 x = vfy_ld_bytes(a.cproofs + (size_t)p * v.proof_bytes + src);
    v.words[(size_t)p * v.W + i] = x;
    if (x >= gl::P) atomicOr(&v.flags[p], (u32)VF_NONCANON);
}

// ------------------------------------------------------------------------------------------- 3. opening reductions
__global__ void k_cmp_reductions(CmpArgs a) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.v.batch) return;
    const u64* ch = a.v.chal + (size_t)p * CH_WORDS;
    vfy_opening_reductions(a.v, p, a.v.words + (size_t)p * a.v.W, ch, gl::e2(ch[CH_ZETA], ch[CH_ZETA + 1]));
}

// ------------------------------------------------------------------------------------------- 4. inferred evaluations
__global__ __launch_bounds__(CMP_MAXQ) void k_cmp_infer(CmpArgs a) {
    const VerifyArgs& v = a.v;
    const u32 p = blockIdx.x, q = threadIdx.x;
    const CmpPlan& pl = a.plan[p];
    if (pl.len == 0) return;  // (uniform over the workgroup)
    const bool mine = q < v.num_queries;
    u64* w = v.words + (size_t)p * v.W;
    const u64* ch = v.chal + (size_t)p * CH_WORDS;
    const u64* vq = v.vq + (size_t)p * VQ_WORDS;
    const u32 x = mine ? pl.idx[q] : 0;
    if (mine && ch[CH_QUERY + q] != x) atomicOr(&v.flags[p], (u32)VF_INDICES);
    u64* qw = w + v.q_off + (size_t)(mine ? q : 0) * v.q_stride;
    const u64 sx0 = gl::mul(gl::MULT_GEN, gl::pow(gl::root_of_unity((int)v.lde_bits), gl::bitrev(x, (int)v.lde_bits)));
    for (u32 r = 0; r < v.num_rounds; r++) {
        const u32 rq = mine ? pl.rep[1 + r][q] : 0;
        if (mine && rq == q) {
            const E2 val = vfy_expected(v, w, qw, r, x, sx0, ch, vq);
            u64* d = qw + v.step_eval_off[r] + 2 * ((x >> cmp_shift(r)) & (VFY_ARITY - 1));
            d[0] = val.a, d[1] = val.b;
        }
        __syncthreads();
        if (mine && rq != q) {
            const u32 k = (pl.idx[rq] >> cmp_shift(r)) & (VFY_ARITY - 1);
            const u64* s = w + v.q_off + (size_t)rq * v.q_stride + v.step_eval_off[r] + 2 * k;
            u64* d = qw + v.step_eval_off[r] + 2 * k;
            d[0] = s[0], d[1] = s[1];
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------- 5. Merkle paths
// H: the tree hasher (PoseidonTree, KeccakTree).  A stored sibling that is not an accepted encoding of a hash is NON_CANONICAL.
template <class H>
__device__ __forceinline__ void cmp_merkle(const CmpArgs& a) {
    __shared__ u32 s_node[CMP_MAXQ], s_mask[CMP_MAXQ];
    __shared__ u64 s_cur[CMP_MAXQ][4], s_sib[CMP_MAXQ][4];
    const VerifyArgs& v = a.v;
    const u32 p = blockIdx.x, slot = blockIdx.y, q = threadIdx.x, Q = v.num_queries;
    const CmpPlan& pl = a.plan[p];
    if (pl.len == 0) return;  // (uniform over the workgroup)
    const bool mine = q < Q;
    const u32 t = slot < 4 ? 0 : slot - 3, depth = cmp_depth(v, t);
    u64* qw = v.words + (size_t)p * v.W + v.q_off + (size_t)(mine ? q : 0) * v.q_stride;
    u64* sib_out = qw + (slot < 4 ? v.init_sib_off[slot] : v.step_sib_off[slot - 4]);
    const u32 mask = mine ? pl.mask[t][q] : 0;
    const u32 leaf = mine ? pl.idx[q] >> cmp_shift(t) : 0xFFFFFFFFu;
    const uint8_t* stored = a.cproofs + (size_t)p * v.proof_bytes + (mine ? pl.off[t][q] + cmp_sib_at(a, slot, __popc(mask)) : 0);
    u64 cur[4];
    if (slot < 4) H::hash_or_noop(qw + v.init_eval_off[slot], v.init_width[slot], cur);
    else H::hash_or_noop(qw + v.step_eval_off[slot - 4], 2 * VFY_ARITY, cur);
    s_mask[q] = mask;
    for (u32 l = 0; l < depth; l++) {
        const u32 node = leaf >> l;
        s_node[q] = mine ? node : 0xFFFFFFFFu;
        for (int i = 0; i < 4; i++) s_cur[q][i] = cur[i];
        if ((mask >> l) & 1) {
            const uint8_t* b = stored + 32 * __popc(mask & ((1u << l) - 1));
            u64 y[4];
            for (int i = 0; i < 4; i++) {
                y[i] = vfy_ld_bytes(b + 8 * i);
                s_sib[q][i] = y[i];
            }
            if (!H::valid(y)) atomicOr(&v.flags[p], (u32)VF_NONCANON);
        }
        __syncthreads();
        u64 sb[4] = {0, 0, 0, 0};
        if (mine) {
            if ((mask >> l) & 1) {
                for (int i = 0; i < 4; i++) sb[i] = s_sib[q][i];
            } else {
                u32 from = CMP_MAXQ;
                bool on_path = false;
                for (u32 e = 0; e < Q && from == CMP_MAXQ; e++)
                    if (s_node[e] == (node ^ 1)) from = e, on_path = true;
                for (u32 e = 0; e < q && from == CMP_MAXQ; e++)
                    if (s_node[e] == node && ((s_mask[e] >> l) & 1)) from = e;
                if (from < CMP_MAXQ)
                    for (int i = 0; i < 4; i++) sb[i] = on_path ? s_cur[from][i] : s_sib[from][i];
            }
            for (int i = 0; i < 4; i++) sib_out[4 * l + i] = sb[i];
            H::compress(cur, sb, node & 1);
        }
        __syncthreads();
    }
}
__global__ __launch_bounds__(CMP_MAXQ) void k_cmp_merkle(CmpArgs a) { cmp_merkle<PoseidonTree>(a); }

// ------------------------------------------------------------------------------------------- 6. outputs
// decompression: the full byte layout of every proof whose status is OK, zeros otherwise
__global__ __launch_bounds__(256) void k_cmp_pack(CmpArgs a) {
    const VerifyArgs& v = a.v;
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x, p = blockIdx.y;
    uint8_t* o = a.cout + (size_t)p * v.proof_bytes;
    const bool ok = v.status[p] == P2_VERIFY_OK;
    if (i < v.W) cmp_st_bytes(o + v.word_off[i], ok ? v.words[(size_t)p * v.W + i] : 0);
    if (i < v.n_cnt) o[v.cnt_off[i]] = ok ? v.cnt_exp[i] : 0;
    if (i == 0 && v.num_pi) cmp_st_bytes(o + v.pi_cnt_byte, ok ? v.num_pi : 0);
}

// compression: every word of an unpacked full proof to its place (the slot was zeroed before), for the proofs that compress
__global__ __launch_bounds__(256) void k_cmp_emit(CmpArgs a) {
    const VerifyArgs& v = a.v;
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x, p = blockIdx.y;
    const CmpPlan& pl = a.plan[p];
    if (pl.len == 0) return;
    uint8_t* o = a.cout + (size_t)p * v.proof_bytes;
    const u32 Q = v.num_queries, T = 1 + v.num_rounds;
    if (i < Q) {
        const u32 x = pl.idx[i];
        for (int k = 0; k < 4; k++) o[a.prefix + 4 * i + k] = (uint8_t)(x >> (8 * k));
    }
    if (i < T * Q) {  // sibling counts
        const u32 t = i / Q, q = i % Q;
        if (pl.rep[t][q] == q) {
            const u32 k = __popc(pl.mask[t][q]);
            for (u32 s = 0; s < (t == 0 ? 4u : 1u); s++) o[pl.off[t][q] + cmp_sib_at(a, t == 0 ? s : 4, k) - 1] = (uint8_t)k;
        }
    }
    if (i == 0 && v.num_pi) cmp_st_bytes(o + pl.len - a.tail + (v.pi_cnt_byte - (u32)(v.proof_bytes - a.tail)), v.num_pi);
    if (i >= v.W) return;
    const u32 code = a.wmap[i], kind = code >> 28, q = (code >> 22) & 63, slot = (code >> 18) & 15, e = code & 0x3FFFF;
    u32 dst;
    if (kind == CW_PREFIX) {
        dst = v.word_off[i];
    } else if (kind == CW_TAIL) {
        dst = pl.len - (u32)(v.proof_bytes - v.word_off[i]);
    } else if (kind == CW_LEAF) {
        if (pl.rep[0][q] != q) return;
        dst = pl.off[0][q] + cmp_leaf_at(a, slot, __popc(pl.mask[0][q])) + 8 * e;
    } else if (kind == CW_EVAL) {
        const u32 r = slot - 4, left_out = (pl.idx[q] >> cmp_shift(r)) & (VFY_ARITY - 1), k = e >> 1;
        if (pl.rep[1 + r][q] != q || k == left_out) return;
        dst = pl.off[1 + r][q] + 16 * (k < left_out ? k : k - 1) + 8 * (e & 1);
    } else {
        const u32 t = slot < 4 ? 0 : slot - 3, l = e >> 2, mask = pl.mask[t][q];
        if (!((mask >> l) & 1)) return;
        dst = pl.off[t][q] + cmp_sib_at(a, slot, __popc(mask)) + 32 * __popc(mask & ((1u << l) - 1)) + 8 * (e & 3);
    }
    cmp_st_bytes(o + dst, v.words[(size_t)p * v.W + i]);
}

// one status per proof: compress SHAPE | NON_CANONICAL of the full proof; decompress SHAPE, NON_CANONICAL, then the indices
__global__ void k_cmp_finish(CmpArgs a) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.v.batch) return;
    const u32 f = a.v.flags[p];
    int st = P2_VERIFY_OK;
    if (f & VF_SHAPE) st = P2_VERIFY_SHAPE;
    else if (f & VF_NONCANON) st = P2_VERIFY_NON_CANONICAL;
    else if (!a.from_chal && (f & VF_INDICES)) st = P2_VERIFY_SHAPE;
    a.v.status[p] = st;
    if (a.from_chal) a.lengths_out[p] = st == P2_VERIFY_OK ? a.plan[p].len : 0;
}

}  // namespace p2k
