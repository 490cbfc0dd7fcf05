// Kernels that run AFTER k_witness, on the final slot values of a chunk of witnesses: reading targets back, the missing-input
// rule of k_fill_wires for a run that builds no wire matrix, and the fault diagnosis of witness_check.h.  k_witness itself
// and every other kernel of the proving pipeline are used as they are.
#pragma once
#include "kernels.h"
#include "witness_check.h"

namespace p2k {

// out[p][j] = values[p][out_slots[j]].  Grid (ceil(n_out / 256), batch).  The index loads and the stores are coalesced; the
// value loads go wherever the slots are -- element-granular reads through L2.  That is what reading n_out scattered words
// out of num_slots is; there is nothing to tile.
__global__ __launch_bounds__(256) void k_gather_slots(const u64* __restrict__ values, u32 num_slots, const u32* __restrict__ out_slots, u32 n_out,
                                                      u64* __restrict__ out) {
    const u32 j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_out) return;
    out[(size_t)blockIdx.y * n_out + j] = values[(size_t)blockIdx.y * num_slots + out_slots[j]];
}

// k_fill_wires' status rule without the wire matrix: a witness whose status is still 0 and that left a slot of a routed wire
// unset is a missing input (2); a conflict (1) already recorded wins.  `wired` is the ascending list of the distinct wired
// slots (p2_circuit_load), so the scan reads `values` nearly in order instead of through the 80 n wire-to-slot indirection.
// Grid (blocks, batch), any number of blocks.
__global__ __launch_bounds__(256) void k_witness_wired_unset(const u64* __restrict__ values, u32 num_slots, const u32* __restrict__ wired, u32 n_wired,
                                                             int* __restrict__ status) {
    const u64* val = values + (size_t)blockIdx.y * num_slots;
    bool unset = false;
    for (u32 j = blockIdx.x * 256 + threadIdx.x; j < n_wired; j += gridDim.x * 256) unset |= val[wired[j]] == UNSET;
    if (unset) atomicCAS(&status[blockIdx.y], 0, 2);
}

// Fault candidates of ONE witness (witness_check.h).  Thread t < num_ops recomputes generator t of the blob's op order from the
// final values -- a PoseidonGate row is one thread, as in witness_poseidon_op; thread num_ops + j looks at free slot j.  Two
// keys, each reduced with a 64-bit atomicMin: keys[0] = lowest faulting generator, keys[1] = first unset free slot (the report
// takes one or the other by the run's status, so they never compete).  The caller presets both to W_NO_KEY.
__global__ __launch_bounds__(256) void k_witness_check(p2::WCheckCtx c, unsigned long long* __restrict__ keys) {
    const u32 t = blockIdx.x * 256 + threadIdx.x;
    if (t < c.num_ops) {
        if (p2::wcheck_op(c, t).kind != P2_FAULT_NONE) atomicMin(&keys[0], (unsigned long long)t);
    } else if (t - c.num_ops < c.num_free) {
        if (c.val[c.free_slots[t - c.num_ops]] == UNSET) atomicMin(&keys[1], (unsigned long long)(t - c.num_ops));
    }
}

// The second, small pass: the input steps (non-canonical value, conflicting entries) over the assignment, then the record.
// One workgroup.  force_status != 0 replaces the run's status (an assignment form whose 2^64-1 is a value, not a marker).
__global__ __launch_bounds__(256) void k_witness_report(p2::WCheckCtx c, const u32* __restrict__ prev, int* __restrict__ status, int force_status,
                                                        const unsigned long long* __restrict__ keys, p2_witness_fault* __restrict__ out) {
    __shared__ u32 s_bad, s_conflict, s_slot, s_setter;
    __shared__ p2_witness_fault s_fault;
    if (threadIdx.x == 0) s_bad = s_conflict = s_slot = s_setter = p2::W_NO_INDEX;
    __syncthreads();
    for (u32 i = threadIdx.x; i < c.n_inputs; i += 256) {
        u64 earlier;
        const int k = p2::wcheck_input(c, prev, i, &earlier);
        if (k == P2_FAULT_INPUT_NOT_CANONICAL) atomicMin(&s_bad, i);
        if (k == P2_FAULT_INPUT_CONFLICT) atomicMin(&s_conflict, i);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int st = force_status ? force_status : status[0];
        status[0] = st;
        const u32 bad_op = keys[0] == p2::W_NO_KEY ? p2::W_NO_INDEX : (u32)keys[0], unset_free = keys[1] == p2::W_NO_KEY ? p2::W_NO_INDEX : (u32)keys[1];
        u32 slot;
        p2::wfault_report(c, prev, st, s_bad, s_conflict, bad_op, unset_free, &s_fault, &slot);
        s_slot = slot;
    }
    __syncthreads();
    if (s_slot != p2::W_NO_INDEX)
        for (u32 i = threadIdx.x; i < c.n_inputs; i += 256)
            if (c.input_slots[i] == s_slot && p2::winput_sets(c, i)) atomicMin(&s_setter, i);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_setter != p2::W_NO_INDEX) s_fault.input_index = s_setter;
        *out = s_fault;
    }
}

}  // namespace p2k
