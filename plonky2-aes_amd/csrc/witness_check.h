// After-the-fact diagnosis of one witness run, written once for the host (p2_host_witness) and the device (k_witness_check,
// k_witness_report in kernels_witness_io.h), the way verifier.h is shared.
//
// Why it can be done afterwards: a slot never changes once it is set.  A generator that conflicted while the program ran had
// every operand set and lost against a value that was already there; both are still there when the program has finished, so
// recomputing the generator from the FINAL slot values finds the same conflict -- and nothing else, because a generator that
// won its slot recomputes to what the slot holds.  The same holds for a lookup whose input is not in its table.
//
// One fault is reported (p2_witness_fault, include/p2aes.h), chosen in this order:
//   1. INPUT_NOT_CANONICAL  lowest entry of the assignment whose value is >= p (and is not the "absent" marker where the
//                           caller's form has one);
//   2. INPUT_CONFLICT       lowest entry whose value differs from that of an earlier entry of the same slot;
//   3./4. LOOKUP_MISS / GENERATOR_CONFLICT   the generator with the lowest index in the BLOB's op order;
//   5. NOT_SET              the lowest target among the unset slots that no generator produces and that a generator or a
//                           routed wire needs.
// 1-4 are looked for when the run ended with status 1, 5 when it ended with status 2, nothing with status 0: kind and status
// cannot disagree.
#pragma once
#include <algorithm>
#include <vector>

#include "../../include/p2aes.h"
#include "circuit.h"
#include "gl.h"
#include "ecstep_gate.h"
#include "poseidon_gate.h"

#if defined(__HIPCC__)
#define WC_HD __host__ __device__
#else
#define WC_HD
#endif
// wcheck_op and wfault_report in device code: always inlined, a call would pass the context through scratch memory
#if defined(__HIP_DEVICE_COMPILE__)
#define WC_HD_INLINE __host__ __device__ __forceinline__
#else
#define WC_HD_INLINE WC_HD inline
#endif
// Device: no global load written below may be issued before `v` is computed (an empty asm that takes v and clobbers memory).
// The loads of a check do not depend on the values they are compared with, and the compiler otherwise issues all of them first.
#if defined(__HIP_DEVICE_COMPILE__)
#define WC_LOADS_AFTER(v) asm volatile("" : "+v"(v) : : "memory")
#else
#define WC_LOADS_AFTER(v) (void)0
#endif

namespace p2 {

static const u64 W_UNSET = ~0ull;       // P2_VALUE_UNSET
static const u64 W_NO_KEY = ~0ull;      // "no candidate" of the two reduction keys
static const u32 W_NO_INDEX = ~0u;

// ------------------------------------------------------------------ tables, built once per circuit on the host
// slot -> its reported target and row; the wired slots (k_witness_wired_unset) and the free slots (NOT_SET candidates).
struct WitnessTables {
    std::vector<u32> wired_slots;   // distinct slots some routed wire refers to, ascending
    std::vector<u64> slot_target;   // per slot: its lowest virtual target, else its lowest routed wire (1<<63 | row<<8 | col), else ~0
    std::vector<u32> slot_row;      // per slot: the row of its lowest routed wire (lowest row, then column), else UINT32_MAX
    std::vector<u32> free_slots;    // slots without a producer that an op or a routed wire needs, ascending by slot_target
    std::vector<u64> lut_ent;       // [num_luts][65536] input -> (flat entry index << 16) | output, or ~0 (as the prover's table)
};

// operands of an op (Poseidon: the row's 12 inputs and its swap wire; EcStep: the row's wires 0..30); returns their number
inline int op_operands(const Circuit& c, const Op& o, u32* d) {
    const size_t n = c.n();
    int nd = 0;
    if (o.kind == OP_ARITH) {
        d[nd++] = o.a, d[nd++] = o.b, d[nd++] = o.c;
    } else if (o.kind == OP_LOOKUP || o.kind == OP_LIMB) {
        d[nd++] = o.a;
    } else if (o.kind == OP_EQ || o.kind == OP_EQINV) {
        d[nd++] = o.a, d[nd++] = o.b;
    } else if (o.kind == OP_POSEIDON) {
        for (u32 k = 0; k < 12; k++) d[nd++] = (u32)c.wire_slot[(size_t)(PG_IN + k) * n + o.a];
        d[nd++] = (u32)c.wire_slot[(size_t)PG_SWAP * n + o.a];
    } else if (o.kind == OP_ECSTEP) {
        for (u32 k = 0; k < EG_MID; k++) d[nd++] = (u32)c.wire_slot[(size_t)k * n + o.a];
    }
    return nd;
}

inline std::vector<u64> witness_lut_entries(const Circuit& c) {
    std::vector<u64> ent(c.luts.size() * 65536, ~0ull);
    size_t flat = 0;
    for (size_t l = 0; l < c.luts.size(); l++)
        for (size_t i = 0; i < c.luts[l].size(); i++, flat++) {
            auto pr = c.luts[l][i];
            if (ent[l * 65536 + pr.first] == ~0ull) ent[l * 65536 + pr.first] = ((u64)flat << 16) | pr.second;
        }
    return ent;
}

// the distinct slots some routed wire refers to, ascending (all the prover needs of the tables at load)
inline std::vector<u32> wired_slot_list(const Circuit& c) {
    std::vector<uint8_t> wired(c.num_slots, 0);
    for (int32_t s : c.wire_slot)
        if (s >= 0) wired[s] = 1;
    std::vector<u32> out;
    for (u32 s = 0; s < c.num_slots; s++)
        if (wired[s]) out.push_back(s);
    return out;
}

inline WitnessTables witness_tables(const Circuit& c, bool with_lut = true) {
    const size_t n = c.n();
    const u32 R = c.cfg.num_routed_wires;
    WitnessTables t;
    t.slot_target.assign(c.num_slots, ~0ull);
    t.slot_row.assign(c.num_slots, ~0u);
    std::vector<uint8_t> produced(c.num_slots, 0), needed(c.num_slots, 0);
    t.wired_slots = wired_slot_list(c);
    for (size_t v = c.vt_slot.size(); v-- > 0;)
        if (c.vt_slot[v] >= 0) t.slot_target[c.vt_slot[v]] = (u64)v;
    for (size_t row = n; row-- > 0;)
        for (u32 col = R; col-- > 0;) {
            const int32_t s = c.wire_slot[(size_t)col * n + row];
            if (s < 0) continue;
            needed[s] = 1;
            t.slot_row[s] = (u32)row;
            if (t.slot_target[s] >> 63) t.slot_target[s] = (1ull << 63) | ((u64)row << 8) | col;  // no virtual target: lowest wire so far
        }
    u32 d[32];
    for (const Op& o : c.ops) {
        const int nd = op_operands(c, o, d);
        for (int j = 0; j < nd; j++) needed[d[j]] = 1;
        if (o.kind == OP_POSEIDON) {
            for (u32 col = PG_OUT; col < R; col++)
                if (col != PG_SWAP) produced[c.wire_slot[(size_t)col * n + o.a]] = 1;
        } else if (o.kind == OP_ECSTEP) {
            for (u32 col = EG_MID; col < EG_WIRES; col++) produced[c.wire_slot[(size_t)col * n + o.a]] = 1;
        } else {
            produced[o.out] = 1;
        }
    }
    for (u32 s = 0; s < c.num_slots; s++)
        if (!produced[s] && needed[s]) t.free_slots.push_back(s);
    std::sort(t.free_slots.begin(), t.free_slots.end(), [&](u32 x, u32 y) { return t.slot_target[x] != t.slot_target[y] ? t.slot_target[x] < t.slot_target[y] : x < y; });
    if (with_lut) t.lut_ent = witness_lut_entries(c);
    return t;
}

// p2_target -> slot, or -1 (the encoding p2_prove_batch_device accepts: a virtual target index, or 1<<63 | row<<8 | column)
inline int32_t target_slot(const Circuit& c, u64 t) {
    if (t >> 63) {
        const u64 row = (t & ~(1ull << 63)) >> 8, col = t & 0xFF;
        return (row < c.n() && col < c.cfg.num_routed_wires) ? c.wire_slot[col * c.n() + row] : -1;
    }
    return t < c.vt_slot.size() ? c.vt_slot[t] : -1;
}

// ------------------------------------------------------------------ the check, host and device
struct WCheckCtx {
    const Op* ops;             // BLOB order (Circuit::ops), not the schedule's
    u32 num_ops, num_slots, n;
    const u64* val;            // [num_slots] final values of one witness
    const u64* lut_ent;        // [num_luts][65536]
    const int32_t* wire_slot;  // [80][n]
    const u32* free_slots;     // NOT_SET candidates in report order
    u32 num_free;
    const u64* slot_target;    // [num_slots]
    const u32* slot_row;       // [num_slots]
    // the assignment that was run
    const u32* input_slots;    // [n_inputs]
    const u64* input_values;   // [n_inputs]
    u32 n_inputs;
    int absent_marker;         // 1: a value of 2^64-1 means "not assigned" (device forms); 0: it is a non-canonical value
};

// PoseidonGenerator of one row, its written routed wires (columns 12..79 but the swap wire) handed to emit(col, value) in
// the order the generator computes them.  Twelve state words and nothing else live: no row buffer.
template <class Emit>
WC_HD inline void poseidon_row_walk(const u64* in, u64 swap, Emit emit) {
    typedef FBase F;
    u64 st[12];
    for (int i = 0; i < 4; i++) {
        const u64 d = gl::mul(swap, gl::sub(in[i + 4], in[i]));
        emit(PG_DELTA + i, d);
        st[i] = gl::add(in[i], d);
        st[i + 4] = gl::sub(in[i + 4], d);
    }
    for (int i = 8; i < 12; i++) st[i] = in[i];
    int round = 0;
    for (int r = 0; r < 4; r++, round++) {
        pg_constants<F>(st, round);
        if (r != 0)
            for (int i = 0; i < 12; i++) emit(PG_FULL0 + 12 * (r - 1) + i, st[i]);
        pg_sbox_layer<F>(st);
        pg_mds<F>(st);
    }
    for (int r = 0; r < 22; r++, round++) {
        pg_constants<F>(st, round);
        if (PG_PARTIAL + r < 80) emit(PG_PARTIAL + r, st[0]);
        st[0] = pg_sbox<F>(st[0]);
        pg_mds<F>(st);
    }
    for (int r = 0; r < 4; r++, round++) {
        pg_constants<F>(st, round);
        pg_sbox_layer<F>(st);
        pg_mds<F>(st);
    }
    for (int i = 0; i < 12; i++) emit(PG_OUT + i, st[i]);
}

// OP_LIMB: bits [k0, k0 + k1) of a canonical value (load-time validation keeps 1 <= k1 <= 16 and k0 + k1 <= 64)
WC_HD inline u64 limb_of(u64 x, u64 k0, u64 k1) { return (x >> k0) & ((1ull << k1) - 1); }

struct WOpFault {
    int kind;  // P2_FAULT_NONE, P2_FAULT_LOOKUP_MISS or P2_FAULT_GENERATOR_CONFLICT
    u32 slot;  // the slot at fault: the lookup's input, or the output the generator lost
    u64 computed, found;
};

// Generator `i` (blob order) against the final values.  A generator with an unset operand never ran and is no fault here;
// neither is one whose output slot is unset (it can only be unset if the generator never ran when it was scheduled).
WC_HD_INLINE WOpFault wcheck_op(const WCheckCtx& c, u32 i) {
    const Op o = c.ops[i];
    WOpFault f{P2_FAULT_NONE, 0, 0, 0};
    if (o.kind == OP_POSEIDON) {
        u64 in[12];
        for (u32 k = 0; k < 12; k++) {
            in[k] = c.val[c.wire_slot[(size_t)k * c.n + o.a]];
            if (in[k] == W_UNSET) return f;
        }
        const u64 swap = c.val[c.wire_slot[(size_t)PG_SWAP * c.n + o.a]];
        if (swap == W_UNSET) return f;
        u32 best_col = W_NO_INDEX;  // the conflict of the lowest column, whatever order the walk visits them in
        poseidon_row_walk(in, swap, [&](u32 col, u64 v) {
            const u32 sl = (u32)c.wire_slot[(size_t)col * c.n + o.a];
            const u64 cur = c.val[sl];
            if (cur != W_UNSET && cur != v && col < best_col) {
                best_col = col;
                f.kind = P2_FAULT_GENERATOR_CONFLICT, f.slot = sl, f.computed = v, f.found = cur;
            }
        });
        return f;
    }
    if (o.kind == OP_ECSTEP) {
        for (u32 k = 0; k < EG_MID; k++)
            if (c.val[c.wire_slot[(size_t)k * c.n + o.a]] == W_UNSET) return f;
        // the walk reads each operand when it needs it, and visits the columns in ascending order: the first conflict is the
        // one of the lowest column
        // (the present values of the 20 mid slots are fetched once mid is computed, those of the out slots once out is: fetched
        // up front, 40 slots and their indices would sit in registers beside the 18 products and spill)
        ecstep_row_walk([&](u32 k) { return c.val[c.wire_slot[(size_t)k * c.n + o.a]]; }, [&](u32 col, u64 v) {
            if (col == EG_MID || col == EG_OUT) WC_LOADS_AFTER(v);
            const u32 sl = (u32)c.wire_slot[(size_t)col * c.n + o.a];
            const u64 cur = c.val[sl];
            if (cur != W_UNSET && cur != v && f.kind == P2_FAULT_NONE) f.kind = P2_FAULT_GENERATOR_CONFLICT, f.slot = sl, f.computed = v, f.found = cur;
        });
        return f;
    }
    u64 x = 0, y = 0, z = 0, r = 0;
    if (o.kind != OP_CONST) x = c.val[o.a];
    if (o.kind == OP_ARITH || o.kind == OP_EQ || o.kind == OP_EQINV) y = c.val[o.b];
    if (o.kind == OP_ARITH) z = c.val[o.c];
    if (x == W_UNSET || y == W_UNSET || z == W_UNSET) return f;
    if (o.kind == OP_ARITH) {
        r = gl::add(gl::mul(gl::mul(x, y), o.k0), gl::mul(z, o.k1));
    } else if (o.kind == OP_CONST) {
        r = o.k0;
    } else if (o.kind == OP_LOOKUP) {
        const u64 ent = x < 65536 ? c.lut_ent[(size_t)o.aux * 65536 + x] : ~0ull;
        if (ent == ~0ull) {
            f.kind = P2_FAULT_LOOKUP_MISS, f.slot = o.a, f.found = x;
            return f;
        }
        r = ent & 0xFFFF;
    } else if (o.kind == OP_EQ) {
        r = x == y ? 1 : 0;
    } else if (o.kind == OP_LIMB) {
        r = limb_of(x, o.k0, o.k1);
    } else {
        r = x == y ? 0 : gl::inv(gl::sub(x, y));
    }
    const u64 cur = c.val[o.out];
    if (cur != W_UNSET && cur != r) f.kind = P2_FAULT_GENERATOR_CONFLICT, f.slot = o.out, f.computed = r, f.found = cur;
    return f;
}

// does entry i of the assignment set a slot (a canonical value that is not the absent marker)?
WC_HD inline bool winput_sets(const WCheckCtx& c, u32 i) { return c.input_values[i] < gl::P; }
// steps 1 and 2 for entry i: P2_FAULT_NONE, _INPUT_NOT_CANONICAL or _INPUT_CONFLICT (then *earlier = the earlier entry's value).
// prev[i] = the latest earlier entry of the same slot, or W_NO_INDEX.
WC_HD inline int wcheck_input(const WCheckCtx& c, const u32* prev, u32 i, u64* earlier) {
    const u64 v = c.input_values[i];
    if (v >= gl::P) return (v == W_UNSET && c.absent_marker) ? P2_FAULT_NONE : P2_FAULT_INPUT_NOT_CANONICAL;
    for (u32 j = prev[i]; j != W_NO_INDEX; j = prev[j])
        if (winput_sets(c, j)) {
            *earlier = c.input_values[j];
            return c.input_values[j] != v ? P2_FAULT_INPUT_CONFLICT : P2_FAULT_NONE;
        }
    return P2_FAULT_NONE;
}
inline std::vector<u32> input_prev_links(const std::vector<u32>& slots, u32 num_slots) {
    std::vector<u32> last(num_slots, W_NO_INDEX), prev(slots.size(), W_NO_INDEX);
    for (size_t i = 0; i < slots.size(); i++) prev[i] = last[slots[i]], last[slots[i]] = (u32)i;
    return prev;
}

// The record, from the run's status and the four minima: lowest non-canonical entry, lowest conflicting entry, lowest
// faulting generator, first unset free slot (positions in free_slots); W_NO_INDEX = none.  *slot receives the slot at fault
// (W_NO_INDEX if none): the caller fills input_index with the lowest entry that sets it (winput_sets), which for the input
// kinds is already in place.
WC_HD_INLINE void wfault_report(const WCheckCtx& c, const u32* prev, int status, u32 bad_input, u32 conflict_input, u32 bad_op, u32 unset_free,
                                p2_witness_fault* out, u32* slot) {
    p2_witness_fault f;
    f.kind = P2_FAULT_NONE, f.op_kind = -1, f.input_index = -1, f.target = ~0ull, f.gate_row = ~0u, f.computed = 0, f.found = 0;
    *slot = W_NO_INDEX;
    u32 s = W_NO_INDEX;
    if (status == 1 && bad_input != W_NO_INDEX) {
        f.kind = P2_FAULT_INPUT_NOT_CANONICAL, f.input_index = bad_input, f.found = c.input_values[bad_input];
        s = c.input_slots[bad_input];
    } else if (status == 1 && conflict_input != W_NO_INDEX) {
        f.kind = P2_FAULT_INPUT_CONFLICT, f.input_index = conflict_input, f.found = c.input_values[conflict_input];
        (void)wcheck_input(c, prev, conflict_input, &f.computed);
        s = c.input_slots[conflict_input];
    } else if (status == 1 && bad_op != W_NO_INDEX) {
        const WOpFault of = wcheck_op(c, bad_op);
        f.kind = of.kind, f.op_kind = (int32_t)c.ops[bad_op].kind, f.computed = of.computed, f.found = of.found;
        s = *slot = of.slot;
    } else if (status == 2 && unset_free != W_NO_INDEX) {
        f.kind = P2_FAULT_NOT_SET;
        s = c.free_slots[unset_free];
    } else if (status) {
        // not reachable for a status k_witness produced (every status 1 leaves one of the first three, every status 2 an unset
        // free slot); kept so that kind and status agree whatever the caller passes
        f.kind = status == 1 ? P2_FAULT_GENERATOR_CONFLICT : P2_FAULT_NOT_SET;
    }
    if (s != W_NO_INDEX) {
        f.target = c.slot_target[s];
        f.gate_row = c.slot_row[s];
        if (f.op_kind == (int32_t)OP_POSEIDON || f.op_kind == (int32_t)OP_ECSTEP) f.gate_row = c.ops[bad_op].a;
    }
    *out = f;
}

}  // namespace p2
