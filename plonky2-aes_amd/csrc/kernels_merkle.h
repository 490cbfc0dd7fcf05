// Stand-alone Merkle trees on the device (p2_merkle_tree_*, p2_merkle_verify_batch; include/p2aes.h): the transpose that puts
// ROW-MAJOR leaves in front of the column-major tree kernels (k_hash_leaves, k_merkle_level, k_merkle_top, k_merkle_top_coop:
// kernels.h, merkle_build's level layout), openings gathered from the digest levels, and batched path checks with the proof
// verifier's vfy_merkle<PoseidonTree> (kernels_verify.h).  Poseidon only.
// A leaf kernel of its own that staged row-major sponge blocks through an LDS tile was measured against transpose + k_hash_leaves
// and did not pay (1.1 % of a 2^20 x 8-word build; DESIGN.md section 9f, profiles/merkle_bench.jsonl): the transpose stays.
#pragma once
#include "kernels.h"
#include "kernels_verify.h"

namespace p2k {

// k_mt_transpose: row-major leaves [rows][cols] -> column-major [cols][rows], the layout k_hash_leaves reads with coalesced
// loads, through a 32 x 32 LDS tile; both global sides move 256 contiguous bytes per 32 lanes.  The row stride of 33 words makes
// the transposed read (lane tx reads tile[tx][y]: ds_read_b64, bank (2 (33 tx + y)) mod 64, conflict group a 32-lane half) hit
// 32 distinct bank pairs, since 33 is odd; a stride of 32 would put all 32 lanes on one pair.
__global__ __launch_bounds__(256) void k_mt_transpose(const u64* __restrict__ in, size_t rows, u32 cols, u64* __restrict__ out) {
    __shared__ u64 tile[32][33];
    const size_t r0 = (size_t)blockIdx.x * 32;
    const u32 c0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (u32 y = ty; y < 32; y += 8)
        if (r0 + y < rows && c0 + tx < cols) tile[y][tx] = in[(r0 + y) * cols + c0 + tx];
    __syncthreads();
    for (u32 y = ty; y < 32; y += 8)
        if (c0 + y < cols && r0 + tx < rows) out[(size_t)(c0 + y) * rows + r0 + tx] = tile[tx][y];
}

// k_mt_paths: thread (path i, level l) copies the sibling of leaf indices[i] at level l, node (index >> l) ^ 1, to
// out[i * out_stride + 4 l ..].  dig: the levels as merkle_build lays them out.  An index that is no leaf: status 1, row untouched.
__global__ __launch_bounds__(256) void k_mt_paths(const u64* __restrict__ dig, u32 bits, u32 depth, const u64* __restrict__ indices, size_t n, u64* __restrict__ out,
                                                  size_t out_stride, int* __restrict__ status) {
    const u32 per = depth ? depth : 1;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * per) return;
    const size_t i = t / per;
    const u32 l = (u32)(t - i * per);
    const u64 index = indices[i];
    const bool ok = index < ((u64)1 << bits);
    if (l == 0 && status) status[i] = ok ? 0 : 1;
    if (!ok || depth == 0) return;
    const u64* s = dig + 4 * (((size_t)2 << bits) - ((size_t)2 << (bits - l))) + 4 * ((index >> l) ^ 1);
    u64* o = out + i * out_stride + 4 * l;
#pragma unroll
    for (int w = 0; w < 4; w++) o[w] = s[w];
}

// k_mt_verify: one thread per path.  0 accepted, 1 rejected, 2 a leaf, sibling or cap word that is not below p.
__global__ __launch_bounds__(64) void k_mt_verify(const u64* __restrict__ leaves, u32 leaf_len, const u64* __restrict__ indices, const u64* __restrict__ siblings,
                                                  u32 depth, const u64* __restrict__ cap, u32 cap_height, size_t n, int* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64* leaf = leaves + i * leaf_len;
    const u64* sib = siblings + i * 4 * (size_t)depth;
    const u32 cap_n = 1u << cap_height;
    bool canonical = true;
    for (u32 w = 0; w < leaf_len; w++) canonical &= leaf[w] < gl::P;
    for (u32 w = 0; w < 4 * depth; w++) canonical &= sib[w] < gl::P;
    for (u32 w = 0; w < 4 * cap_n; w++) canonical &= cap[w] < gl::P;
    if (!canonical) {
        status[i] = 2;
        return;
    }
    const u64 index = indices[i];
    // vfy_merkle walks a 32-bit index; one that does not fit names no leaf of a tree these entry points accept
    const bool ok = (index >> 32) == 0 && vfy_merkle<PoseidonTree>(leaf, leaf_len, (u32)index, cap, cap_n, sib, depth);
    status[i] = ok ? 0 : 1;
}

}  // namespace p2k
