// GPU half of the C ABI (include/p2aes.h): p2_circuit_load, p2_prove_batch(_device), debug reads, primitives.
// Replaces `CircuitData::prove(pw)` (reference call sites: SURVEY.md A.2) with a sequence of HIP kernels on one
// stream per circuit handle; no host synchronisation between stages (Fiat-Shamir runs in a device kernel).
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <random>
#include <string>
#include <thread>

#include "capi_common.h"
#include "hip_owners.h"
#include "os_random.h"
#include "kernels.h"
#include "kernels2.h"
#include "kernels_compress.h"
#include "kernels_keccak.h"
#include "kernels_merkle.h"
#include "kernels_merkle_update.h"
#include "kernels_merkle_map.h"
#include "kernels_elgamal.h"
#include "kernels_gcm.h"
#include "kernels_pcipher.h"
#include "kernels_schnorr.h"
#include "kernels_witness_io.h"
#include "merkle_host.h"
#include "pool.h"
#include "verifier.h"

using namespace p2;
using namespace p2k;

// HIPCHECK_AS: the error names `text`, the HIP call an owner's method makes, where the expression itself would name the method
#define HIPCHECK(expr) HIPCHECK_AS(#expr, expr)
#define HIPCHECK_AS(text, expr)                                                                 \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess) {                                                                 \
            set_error(std::string(text) + ": " + hipGetErrorString(_e));                        \
            return P2_ERR_HIP;                                                                  \
        }                                                                                       \
    } while (0)

struct Tree {
    u64* dig = nullptr;  // [batch][4 * 2^(bits+1)]
    u32 bits = 0;        // log2(#leaves)
    size_t stride() const { return (size_t)8 << bits; }
};
// first word of level l of a tree's digest buffer (level 0: the 2^bits leaf digests)
static size_t level_off(u32 bits, u32 l) { return 4 * (((size_t)2 << bits) - ((size_t)2 << (bits - l))); }
static size_t cap_off(const Tree& t, u32 cap_height) { return level_off(t.bits, t.bits - cap_height); }

// Device allocations with one owner -- a handle, a workspace, a PrimCtx, one call of a primitive -- freed when it goes, on every
// path out.
class Allocs {
    std::vector<void*> v;

public:
    Allocs() = default;
    Allocs(const Allocs&) = delete;
    ~Allocs() { clear(); }
    bool empty() const { return v.empty(); }
    hipError_t alloc(void** p, size_t bytes) {
        const hipError_t e = hipMalloc(p, bytes);
        if (e == hipSuccess) v.push_back(*p), g_live_resources++;
        return e;
    }
    void clear() {
        for (void* p : v) (void)hipFree(p);
        g_live_resources -= v.size();
        v.clear();
    }
};
template <class T>
static int dalloc(Allocs& mem, T** p, size_t count) {
    void* q = nullptr;
    HIPCHECK_AS("hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T))", mem.alloc(&q, std::max<size_t>(count, 1) * sizeof(T)));
    *p = (T*)q;
    return 0;
}
template <class T>
static int upload(Allocs& mem, T** p, const T* host, size_t count) {
    if (dalloc(mem, p, count)) return P2_ERR_HIP;
    if (count) HIPCHECK(hipMemcpy(*p, host, count * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

// What a launch needs: its stream and, while per-kernel timing is on, the event pairs that collect_timing has yet to read.
struct Lane {
    hipStream_t stream = nullptr;  // where the launches go: `own` (open), or a caller's stream (mt_build)
    Stream own;
    bool timing = false;  // follows p2_circuit::timing_on (p2_circuit_set_timing, build_workspace)
    std::vector<std::pair<std::string, std::pair<Event, Event>>> pending;
    hipError_t open(unsigned flags) { const hipError_t e = own.create(flags); return stream = own, e; }
};
// Launch on a lane, with optional per-kernel event timing under `name`.
#define LAUNCH(lane, name, kernel, grid, block, shmem, ...)                                  \
    do {                                                                                     \
        Lane& _l = (lane);                                                                   \
        Event _e0, _e1;                                                                      \
        if (_l.timing) {                                                                     \
            (void)_e0.create(hipEventDefault);                                               \
            (void)_e1.create(hipEventDefault);                                               \
            (void)hipEventRecord(_e0, _l.stream);                                            \
        }                                                                                    \
        hipLaunchKernelGGL(kernel, grid, block, shmem, _l.stream, __VA_ARGS__);              \
        if (_l.timing) {                                                                     \
            (void)hipEventRecord(_e1, _l.stream);                                            \
            _l.pending.emplace_back(name, std::make_pair(std::move(_e0), std::move(_e1)));   \
        }                                                                                    \
        HIPCHECK(hipGetLastError());                                                         \
    } while (0)

// What the transform and tree building blocks read: the size, the twiddle and shift tables and three words of the config.
struct Domain {
    u32 logn = 0;
    std::vector<u32> arities;
    u64 *d_tw_fwd = nullptr, *d_tw_inv = nullptr;  // w^k / w^-k for k < n_max/2, n_max = n
    u64 *d_tw_fwd_full = nullptr, *d_tw_inv_full = nullptr;  // w^k / w^-k for k < n (two-pass NTT, n > 2^14)
    u64* d_tw_fwd_round[9] = {nullptr};                       // order n_r tables for FRI rounds that still need two passes
    u64* d_shift_pows[9] = {nullptr};              // per FRI round r (0 = main LDE): [8][n_r] (s_r w^j)^i
    u64* d_shift_tw = nullptr;                     // main LDE, 2^13 <= n <= 2^14: [8][n/2] d_shift_pows[0][j][i] * w^i
    std::map<const u64*, u64*> pass1_out_tw;       // two-pass NTT: output-twiddle table per full twiddle table (ensure_pass1_table)
    u32 rate_bits = 3, cap_height = 0, hasher = HASHER_POSEIDON;
    size_t n() const { return (size_t)1 << logn; }
};

// One committed oracle: column values -> coefficients -> LDE (the salt columns of a zk circuit last) -> Merkle tree.
struct Oracle {
    u64* vals = nullptr;  // [cols][n] per proof; null where the values never exist in this form (the quotient)
    u64 *coef = nullptr, *lde = nullptr;  // [cols][n], [cols + salt][8 n]
    Tree tree;
    u32 cols = 0;       // materialised columns
    u32 tree_cols = 0;  // columns of a leaf before the salt: more than `cols` where the rest are identically zero (wires)
    u32 salt = 0;
    size_t coef_stride = 0, lde_stride = 0;  // per proof; 0 for the preprocessed oracle, which every proof shares
    size_t dig_stride() const { return lde_stride ? tree.stride() : 0; }
};

struct Workspace {
    Allocs mem;  // everything below that build_workspace allocates; declared first: freed after the lane has gone
    Lane lane;   // the proving stream
    Event done;  // recorded after the last kernel of a call; the caller's stream waits on it
    u32* d_input_slots = nullptr;      // slot of every input target, as last uploaded to this workspace
    std::vector<u32> h_input_slots;    // host copy: re-uploaded only when a call brings a different target list
    u64* d_input_values = nullptr;
    u64* d_values = nullptr;
    u32* d_mult = nullptr;
    int* d_status = nullptr;
    u64* d_advice = nullptr;
    u64* d_pi_hash = nullptr;          // [chunk][4] public-input hash per proof (k_pi_hash; circuits with public inputs)
    DevBuf<u32> d_out_slots;           // slot of every out-target (p2_prove_batch_outputs*), as last uploaded; grown on demand
    std::vector<u32> h_out_slots;
    Oracle wires, zs, quot;
    u64 *d_permq = nullptr, *d_perm_seg = nullptr, *d_fri_seg = nullptr, *d_lktmp = nullptr;
    u64 *d_qvals = nullptr, *d_qres = nullptr;
    ChalState* d_chal_state = nullptr;
    u64* d_chal = nullptr;
    u64 *d_pows = nullptr, *d_ev = nullptr, *d_obs = nullptr, *d_comp = nullptr, *d_apow = nullptr;
    u64 *d_ztab = nullptr, *d_fripow = nullptr;  // per proof: the two-level tables of k_zeta_tabs, the FRI alpha powers
    u64* d_fri_coef[9] = {nullptr};  // [2][n_r]
    u64* d_fri_vals[9] = {nullptr};  // [2][8 n_r]
    Tree fri_tree[9];
    unsigned long long* d_pow_best = nullptr;
    u32* d_pow_list = nullptr;  // [chunk] unsolved proofs + [1] their count (proof-of-work phases)
    uint8_t* d_proofs = nullptr;
    PolyRef* d_polyrefs = nullptr;
    EvalRef* d_evalrefs = nullptr;
    ~Workspace() { if (lane.stream) (void)hipStreamSynchronize(lane.stream); }
};

// Members go in reverse order: the pools and the proving workspaces (each waits for its own stream first), then the setup lane,
// and `allocs` -- the tables all of them read -- last.
struct p2_circuit {
    Circuit c;
    int device = 0;
    Allocs allocs;
    Lane setup;  // load-time work (preprocessing); the proving lanes are the workspaces'
    Domain dom;
    size_t n = 0, N = 0;
    u32 lde_bits = 0, active_wires = 0;
    ProofLayout layout;  // where every field of a proof sits (proof_layout.h), built at load
    size_t pbytes = 0;   // = layout.bytes
    // ---- static device data
    Op* d_ops = nullptr;
    WLevel* d_wlevels = nullptr;
    WChain* d_wchains = nullptr;
    u32 witness_levels = 0, witness_chains = 0;
    int32_t* d_wire_slot = nullptr;
    u32* d_pi_slots = nullptr;  // witness slot of every public input (circuits with public inputs)
    u64* d_lut_ent = nullptr;
    u32 *d_lut_pairs = nullptr, *d_lut_offsets = nullptr, *d_num_lookups = nullptr;
    LookupRows* d_lookup_rows = nullptr;
    int32_t* d_pos_index = nullptr;  // [n] advice block of a PoseidonGate row, else -1
    u32 *d_blind_rows = nullptr, *d_blind_zrows = nullptr;
    ZkKey zk_key{};      // blinding PRF key (zk circuits): OS randomness at load, or p2_circuit_set_zk_key
    u64 zk_counter = 0;  // proofs attempted under this key; never reused, also when a batch fails
    size_t total_lut_entries = 0;
    u64 *d_sigmas = nullptr, *d_k_is = nullptr, *d_subgroup = nullptr;
    u64* d_shift_inv_pows = nullptr;               // [8][n] (g w^j)^-i / n   (quotient inverse)
    u64 *d_xs = nullptr, *d_l0 = nullptr, *d_zh_inv = nullptr, *d_w8inv = nullptr, *d_qscale = nullptr;
    Oracle pre;               // constants | sigmas, committed at load
    u64* d_digest = nullptr;  // circuit digest (4)
    std::vector<u64> verifier_data;
    u32 n_b0 = 0, n_b1 = 0, n_evalrefs = 0;
    u32 *d_map_obs = nullptr, *d_map_ser = nullptr;
    u32 n_obs = 0, n_ser = 0, ev_count = 0;
    // ---- per-stream workspaces: chunks are dealt round-robin to streams so that the latency-bound stages of one
    // chunk (witness levels, Fiat-Shamir, PoW tail) overlap with the Poseidon-heavy stages of another
    std::vector<std::unique_ptr<Workspace>> ws;
    Event ev_witness;  // end of the latest witness kernel on any proving stream
    bool witness_recorded = false;
    u32 ws_inputs = 0;
    size_t chunk = 0;
    // tuning options (p2_circuit_set_option; the environment is read ONCE, at load): proofs per chunk, proving streams,
    // phase timing of the host path on stderr
    size_t opt_chunk = 128, opt_streams = 2;
    // Longest chain of the witness schedule (P2AES_WITNESS_FUSE at load, 1..8).  Default 1 = no chains: measured on the 64 KiB
    // circuit, chains of 8 cut the levels from 12.4 k to 2.6 k and change nothing (73 vs 66 ms per 16 witnesses, 17.4 vs 17.6
    // proofs/s) -- the kernel is bound by one compute unit's address path, not by its depth -- and the chain executor costs
    // 252 VGPRs against 126.  The contraction is what a several-CUs-per-witness kernel would need; it stays selectable.
    u32 opt_witness_fuse = 1;
    bool opt_debug_timing = false;
    // host-path staging (p2_prove_batch): persistent device buffers + pinned host buffers, one set per concurrent caller
    Pool<struct Staging, NoKey> staging;
    // batched verification (p2_verify_batch): layout tables built at load, workspaces leased per call like the staging sets
    std::string vfy_error;  // non-empty: a precondition of the verifier kernels does not hold for this circuit
    VerifyArgs vfy_args{};  // layout and circuit fields; the per-call pointers are filled in by proof_run
    Pool<struct VerifyWs> vfy;     // keyed by the option "verify_chunk"
    // compressed proofs (kernels_compress.h): the source of every word of the full layout
    u32* d_cmp_wmap = nullptr;
    // Keccak circuits: the word index of every hash of the unpacked proof, the caps first (k_kcv_range)
    u32* d_kc_hash_idx = nullptr;
    u32 kc_cap_hashes = 0, kc_hashes = 0;
    // witness-only calls and witness outputs (kernels_witness_io.h): the distinct wired slots (built at load), workspaces
    // leased per call like the verification ones, and the tables of the fault check, uploaded by the first p2_witness_explain
    u32* d_wired_slots = nullptr;
    u32 n_wired = 0;
    Pool<struct WitnessWs> wit{256};  // keyed by the option "witness_chunk"
    std::unique_ptr<struct ExplainTables> explain;
    std::mutex explain_mu;
    long fail_alloc_after = -1;            // test hook, see dalloc_ws
    // timing
    bool timing_on = false;
    std::map<std::string, std::pair<float, u32>> times;
    std::mutex mu;
    p2_circuit();  // both defined below the leased workspaces, whose types they need complete
    ~p2_circuit();
};

// Launch outside the timing map (the verification / compression driver, whose kernels run on a caller's or a workspace's stream).
#define LAUNCH_ON(st, kernel, grid, block, ...)                          \
    do {                                                                 \
        hipLaunchKernelGGL(kernel, grid, block, 0, st, __VA_ARGS__);     \
        HIPCHECK(hipGetLastError());                                     \
    } while (0)

// The gate table of QuotientArgs and VerifyArgs: kind, selector column and selector group of every gate type.
template <class Args>
static void fill_gate_table(const Circuit& c, Args& a) {
    for (u32 g = 0; g < c.gates.size(); g++) {
        a.gate_kind[g] = c.gates[g];
        a.gate_sel[g] = c.selector_index[g];
        a.group_lo[g] = c.groups[c.selector_index[g]].first;
        a.group_hi[g] = c.groups[c.selector_index[g]].second;
    }
}

// index of the EcStepGate in the circuit's gate list, or -1: such circuits take k_ecwitness, k_ecstep_post and k_vfy_ecvanishing
static int ecstep_gate_index(const Circuit& c) {
    for (size_t g = 0; g < c.gates.size(); g++)
        if (c.gates[g] == p2::G_ECSTEP) return (int)g;
    return -1;
}

static inline dim3 g1(size_t work, u32 block, u32 y = 1, u32 z = 1) { return dim3((u32)((work + block - 1) / block), y, z); }

// ---------------------------------------------------------------------------------- building blocks
static const u32 R16_MIN_BITS = 8;  // the register-blocked kernel needs n / 16 threads >= a few waves; smaller transforms keep k_ntt_lds
static size_t r16_lds_bytes(int logn) { return 8 * (((size_t)1 << logn) + ((size_t)1 << (logn - 4))); }
static int run_ntt(Lane& L, const Domain& D, const char* name, NttArgs a, u32 cols, u32 batch) {
    a.log_nmax = (int)D.logn;
    if ((u32)a.logn >= 13 && !a.bitrev_in && !a.bitrev_out && !a.post) {
        // half a column per workgroup: two (or more) workgroups per compute unit overlap each other's memory phases
        LAUNCH(L, name, k_ntt_r16<true>, dim3(2 * cols * a.cosets, batch), dim3(1u << (a.logn - 5)), r16_lds_bytes(a.logn - 1), a);
        return 0;
    }
    if ((u32)a.logn >= R16_MIN_BITS) {
        LAUNCH(L, name, k_ntt_r16<false>, dim3(cols * a.cosets, batch), dim3(1u << (a.logn - 4)), r16_lds_bytes(a.logn), a);
        return 0;
    }
    size_t shmem = (size_t)8 << a.logn;
    LAUNCH(L, name, k_ntt_lds, dim3(cols * a.cosets, batch), dim3(1024), shmem, a);
    return 0;
}
static const u32 LDS_NTT_MAX_BITS = 14;  // whole transform in one workgroup's LDS up to 2^14 points
// The NTT kernels are launched with more dynamic LDS than the default limit allows (p2_circuit_load, PrimCtx::init).
static hipError_t raise_ntt_lds_limits() {
    const std::pair<const void*, int> limits[] = {{(const void*)k_ntt_lds, 128 * 1024},
                                                  {(const void*)k_ntt_r16<false>, (int)r16_lds_bytes(LDS_NTT_MAX_BITS)},
                                                  {(const void*)k_ntt_r16<true>, (int)r16_lds_bytes(LDS_NTT_MAX_BITS - 1)},
                                                  {(const void*)k_ntt_pass1_r16, 64 * 1024}};
    for (const auto& l : limits)
        if (hipError_t e = hipFuncSetAttribute(l.first, hipFuncAttributeMaxDynamicSharedMemorySize, l.second)) return e;
    return hipSuccess;
}
// The output twiddles of pass 1 for the order-2^logn table `tw_full`, in output order (k_pass1_out_tw); built at load, never
// while workspaces are open (allocations made then belong to the workspaces).
static int ensure_pass1_table(Lane& L, Domain& D, Allocs& mem, const u64* tw_full, u32 logn) {
    if (logn <= LDS_NTT_MAX_BITS || D.pass1_out_tw.count(tw_full)) return 0;
    u64* t = nullptr;
    if (dalloc(mem, &t, (size_t)1 << logn)) return P2_ERR_HIP;
    hipLaunchKernelGGL(k_pass1_out_tw, g1((size_t)1 << logn, 256), dim3(256), 0, L.stream, tw_full, t, (int)logn, (int)(logn - 12));
    HIPCHECK(hipGetLastError());
    D.pass1_out_tw[tw_full] = t;
    return 0;
}
// two-pass transform of `cols*cosets` blocks: natural order in `in`, bit-reversed order in `out`
static int ntt_big(Lane& L, const Domain& D, const char* name, const u64* in, u64* out, const u64* tw_full, const u64* pre, u32 logn, u32 cols, u32 cosets,
                   const u32* block_of_coset, int in_coset_blocks, size_t in_col_stride, size_t out_col_stride, size_t in_batch_stride,
                   size_t out_batch_stride, u64 post_scalar, u32 batch) {
    const u32 log_n2 = 12, log_n1 = logn - log_n2;
    u32 log_T = 12 - log_n1;  // tile of n1 x T = 4096 elements (32 KiB LDS)
    if (log_T < 2) return set_error("transform too large for the two-pass NTT"), P2_ERR_INVALID;
    Pass1Args a{};
    a.in = in;
    a.out = out;
    a.tw = tw_full;
    a.pre = pre;
    a.in_col_stride = in_col_stride;
    a.out_col_stride = out_col_stride;
    a.in_batch_stride = in_batch_stride;
    a.out_batch_stride = out_batch_stride;
    a.logn = (int)logn;
    a.log_n1 = (int)log_n1;
    a.log_T = (int)log_T;
    a.cosets = (int)cosets;
    a.in_coset_blocks = in_coset_blocks;
    for (u32 j = 0; j < 8; j++) a.block_of_coset[j] = block_of_coset ? block_of_coset[j] : 0;
    u32 tiles = (1u << log_n2) >> log_T;
    auto it = D.pass1_out_tw.find(tw_full);
    if (it == D.pass1_out_tw.end()) return set_error("internal: no pass-1 twiddle table for this transform"), P2_ERR_INVALID;
    a.out_tw = it->second;
    a.xcd_swizzle = (cosets > 1 && !in_coset_blocks) ? 1 : 0;  // only where workgroups share their input
    const std::string name1 = std::string(name) + "_pass1";  // the two passes are timed apart
    LAUNCH(L, name1, k_ntt_pass1_r16, dim3(tiles * cols * cosets, batch), dim3(256), r16_lds_bytes(12), a);
    // pass 2: every row of n2 contiguous points, in place
    if (out_col_stride != ((size_t)cosets << logn)) return set_error("internal: two-pass NTT needs densely packed output blocks"), P2_ERR_INVALID;
    NttArgs b{};
    b.in = out;
    b.out = out;
    b.tw = tw_full;
    b.post_scalar = post_scalar;
    b.in_col_stride = b.out_col_stride = (size_t)1 << log_n2;
    b.in_batch_stride = b.out_batch_stride = out_batch_stride;
    b.logn = (int)log_n2;
    b.log_nmax = (int)logn;
    b.cosets = 1;
    size_t rows = ((size_t)cols * cosets) << log_n1;
    // grid.x is limited to 2^31-1; rows*1 fits for every supported size
    LAUNCH(L, name, k_ntt_r16<false>, dim3((u32)rows, batch), dim3(1u << (log_n2 - 4)), r16_lds_bytes((int)log_n2), b);
    return 0;
}
// The transform tables of a domain: D.logn, D.rate_bits and D.arities in; the twiddles of both directions, the order-n_r tables
// of the FRI rounds that still take two passes, every pass-1 output table, the coset shift powers of every round, the folded
// table of the half-column kernel and (where `shift_inv_pows` is given) the quotient inverse's [8][n] (g w^j)^-i / n out.  The
// loader and the primitives' PrimCtx both call it: one copy, so that a hook runs on the tables the prover runs on.
static int build_transform_tables(Lane& L, Domain& D, Allocs& mem, u64** shift_inv_pows) {
    const size_t n = D.n();
    {
        std::vector<u64> sub(n), twi(n);
        u64 w = gl::root_of_unity((int)D.logn), wi = gl::inv(w), x = 1, xi = 1;
        for (size_t i = 0; i < n; i++) {
            sub[i] = x;
            twi[i] = xi;
            x = gl::mul(x, w);
            xi = gl::mul(xi, wi);
        }
        if (upload(mem, &D.d_tw_fwd_full, sub.data(), n)) return P2_ERR_HIP;  // w^k, k < n
        if (upload(mem, &D.d_tw_inv_full, twi.data(), n)) return P2_ERR_HIP;
        D.d_tw_fwd = D.d_tw_fwd_full;    // the single-pass kernel only indexes k < n/2
        D.d_tw_inv = D.d_tw_inv_full;
        if (ensure_pass1_table(L, D, mem, D.d_tw_fwd_full, D.logn) || ensure_pass1_table(L, D, mem, D.d_tw_inv_full, D.logn)) return P2_ERR_HIP;
        // FRI rounds whose polynomial is still > 2^14 need their own order-n_r table
        u32 logn_r = D.logn;
        for (u32 r = 0; r < D.arities.size(); r++) {
            logn_r -= D.arities[r];
            if (logn_r > LDS_NTT_MAX_BITS) {
                size_t n_r = (size_t)1 << logn_r;
                std::vector<u64> t(n_r);
                for (size_t i = 0; i < n_r; i++) t[i] = sub[i << (D.logn - logn_r)];
                if (upload(mem, &D.d_tw_fwd_round[r + 1], t.data(), n_r)) return P2_ERR_HIP;
                if (ensure_pass1_table(L, D, mem, D.d_tw_fwd_round[r + 1], logn_r)) return P2_ERR_HIP;
            }
        }
    }
    {
        // LDE shift tables for round r: bases s_{r,j} = g^(16^r) * w_{8 n_r}^j
        u32 logn_r = D.logn;
        u64 shift = gl::MULT_GEN;
        for (u32 r = 0; r <= D.arities.size(); r++) {
            size_t n_r = (size_t)1 << logn_r;
            std::vector<u64> bases(8);
            u64 wl = gl::root_of_unity((int)(logn_r + D.rate_bits));
            for (u32 j = 0; j < 8; j++) bases[j] = gl::mul(shift, gl::pow(wl, j));
            u64* d_b;
            if (upload(mem, &d_b, bases.data(), 8)) return P2_ERR_HIP;
            if (dalloc(mem, &D.d_shift_pows[r], 8 * n_r)) return P2_ERR_HIP;
            hipLaunchKernelGGL(k_pow_table, g1(n_r, 256, 8), dim3(256), 0, L.stream, D.d_shift_pows[r], d_b, (u32)n_r, (u64)1);
            if (r == 0 && D.logn >= 13 && D.logn <= LDS_NTT_MAX_BITS) {
                if (dalloc(mem, &D.d_shift_tw, 8 * (n_r / 2))) return P2_ERR_HIP;
                hipLaunchKernelGGL(k_mul_tables, g1(n_r / 2, 256, 8), dim3(256), 0, L.stream, D.d_shift_tw, D.d_shift_pows[0], n_r, D.d_tw_fwd, 0, (u32)(n_r / 2));
            }
            if (r == 0 && shift_inv_pows) {
                std::vector<u64> ib(8);
                for (u32 j = 0; j < 8; j++) ib[j] = gl::inv(bases[j]);
                u64* d_ib;
                if (upload(mem, &d_ib, ib.data(), 8)) return P2_ERR_HIP;
                if (dalloc(mem, shift_inv_pows, 8 * n_r)) return P2_ERR_HIP;
                hipLaunchKernelGGL(k_pow_table, g1(n_r, 256, 8), dim3(256), 0, L.stream, *shift_inv_pows, d_ib, (u32)n_r, gl::inv((u64)n % gl::P));
            }
            if (r < D.arities.size()) {
                shift = gl::pow(shift, (u64)1 << D.arities[r]);
                logn_r -= D.arities[r];
            }
        }
        HIPCHECK(hipGetLastError());
    }
    return 0;
}
// values [cols][n] -> coeffs [cols][n].  `scratch` ([cols][n] per proof, same batch stride) is needed when n > 2^14.
static int intt_cols(Lane& L, const Domain& D, const u64* vals, u64* coeffs, u32 cols, size_t batch_stride, u32 batch, u64* scratch = nullptr,
                     size_t scratch_batch_stride = 0) {
    const size_t n = D.n();
    if (D.logn > LDS_NTT_MAX_BITS) {
        if (!scratch) return set_error("internal: large iNTT needs scratch"), P2_ERR_INVALID;
        if (ntt_big(L, D, "intt", vals, scratch, D.d_tw_inv_full, nullptr, D.logn, cols, 1, nullptr, 0, n, n, batch_stride, scratch_batch_stride,
                    gl::inv((u64)n % gl::P), batch))
            return P2_ERR_HIP;
        LAUNCH(L, "bitrev_copy", k_bitrev_copy, g1(n, 256, batch, cols), dim3(256), 0, scratch, n, scratch_batch_stride, coeffs, n, batch_stride,
               (int)D.logn, 1u, (const u64*)nullptr, 0u);
        return 0;
    }
    NttArgs a{};
    a.in = vals;
    a.out = coeffs;
    a.tw = D.d_tw_inv;
    a.post_scalar = gl::inv((u64)n % gl::P);
    a.in_col_stride = a.out_col_stride = n;
    a.in_batch_stride = a.out_batch_stride = batch_stride;
    a.logn = (int)D.logn;
    a.cosets = 1;
    a.bitrev_out = 1;
    return run_ntt(L, D, "intt", a, cols, batch);
}
// coeffs [cols][n_r] -> lde [cols][8 n_r] (bit-reversed order)
static int lde_cols(Lane& L, const Domain& D, const u64* coeffs, size_t in_batch_stride, u64* lde, size_t out_batch_stride, u32 cols, u32 round, u32 batch) {
    u32 logn_r = D.logn;
    for (u32 r = 0; r < round; r++) logn_r -= D.arities[r];
    u32 blocks[8];
    for (u32 j = 0; j < 8; j++) blocks[j] = gl::bitrev(j, (int)D.rate_bits);
    if (logn_r > LDS_NTT_MAX_BITS) {
        // twiddles of order n_r are a stride of the order-n table
        if (round != 0 && D.d_tw_fwd_round[round] == nullptr) return set_error("internal: missing round twiddles"), P2_ERR_INVALID;
        const u64* tw = round == 0 ? D.d_tw_fwd_full : D.d_tw_fwd_round[round];
        return ntt_big(L, D, "lde", coeffs, lde, tw, D.d_shift_pows[round], logn_r, cols, 8, blocks, 0, (size_t)1 << logn_r, (size_t)8 << logn_r,
                       in_batch_stride, out_batch_stride, 1, batch);
    }
    NttArgs a{};
    a.in = coeffs;
    a.out = lde;
    a.tw = D.d_tw_fwd;
    a.pre = D.d_shift_pows[round];
    a.pre_tw = round == 0 ? D.d_shift_tw : nullptr;
    a.post_scalar = 1;
    a.in_col_stride = (size_t)1 << logn_r;
    a.out_col_stride = (size_t)8 << logn_r;
    a.in_batch_stride = in_batch_stride;
    a.out_batch_stride = out_batch_stride;
    a.logn = (int)logn_r;
    a.cosets = 1 << D.rate_bits;
    for (u32 j = 0; j < 8; j++) a.block_of_coset[j] = blocks[j];
    return run_ntt(L, D, "lde", a, cols, batch);
}
// Quotient values on the LDE coset -> coefficient chunks.  qvals: [B][chunks][8 n] in the LDE's bit-reversed order (block
// rev3(j) = coset j), overwritten; qres: scratch of the same shape; coef: [B] x coef_batch_stride, [chunks * 8][n].
// Coset-wise inverse transform (residues r_j, scaled by (g w^j)^-i / n), then the 8-point cross-coset DFT.
static int quotient_chunks(Lane& L, const Domain& D, u64* qvals, u64* qres, u64* coef, u32 chunks, size_t coef_batch_stride, u32 B, const u64* shift_inv_pows,
                           const u64* w8inv, const u64* qscale) {
    const size_t n = D.n(), N = n << D.rate_bits, qs = (size_t)chunks * N;
    if (D.logn > LDS_NTT_MAX_BITS) {
        u32 ident[8] = {0, 1, 2, 3, 4, 5, 6, 7};
        LAUNCH(L, "bitrev_copy", k_bitrev_copy, g1(n, 256, B, chunks * 8), dim3(256), 0, qvals, N, qs, qres, N, qs, (int)D.logn, 8u, (const u64*)nullptr, 0u);
        if (ntt_big(L, D, "quotient_intt", qres, qvals, D.d_tw_inv_full, nullptr, D.logn, chunks, 8, ident, 1, N, N, qs, qs, 1, B)) return P2_ERR_HIP;
        LAUNCH(L, "bitrev_copy", k_bitrev_copy, g1(n, 256, B, chunks * 8), dim3(256), 0, qvals, N, qs, qres, N, qs, (int)D.logn, 8u, shift_inv_pows, 1u);
    } else {
        NttArgs t{};
        t.in = qvals;
        t.out = qres;
        t.tw = D.d_tw_inv;
        t.post = shift_inv_pows;
        t.post_scalar = 1;
        t.in_col_stride = t.out_col_stride = N;
        t.in_batch_stride = t.out_batch_stride = qs;
        t.logn = (int)D.logn;
        t.cosets = 8;
        t.bitrev_in = 1;
        t.bitrev_out = 1;
        t.in_coset_blocks = 1;
        // input block rev3(j) holds coset j; residue r_j is written to the same block
        for (u32 j = 0; j < 8; j++) t.block_of_coset[j] = gl::bitrev(j, 3);
        if (run_ntt(L, D, "quotient_intt", t, chunks, B)) return P2_ERR_HIP;
    }
    LAUNCH(L, "quotient_chunks", k_quotient_chunks_rev, g1(n, 256, B, chunks), dim3(256), 0, qres, coef, (u32)n, qs, coef_batch_stride, w8inv, qscale);
    return 0;
}
// The two 8-entry tables of k_quotient_chunks_rev: w8^-j, and s^-c / 8 with s = g^n.
static void quotient_chunk_scales(u32 logn, u64* w8inv, u64* qscale) {
    const u64 gn = gl::pow(gl::MULT_GEN, (u64)1 << logn), w8 = gl::root_of_unity(3);
    for (u32 j = 0; j < 8; j++) {
        w8inv[j] = gl::inv(gl::pow(w8, j));
        qscale[j] = gl::mul(gl::inv(gl::pow(gn, j)), gl::inv(8));
    }
}
// The three tree kernels of a hasher (one parameter list each for both hashers), and whether the top of a tree may be fused.
struct TreeKernels {
    decltype(&k_hash_leaves) leaves;
    decltype(&k_hash_fri_leaves) fri_leaves;
    decltype(&k_merkle_level) level;
    // Keccak: one launch per level for every batch size: a Keccak level is one permutation of 24 short rounds, and the fused top of
    // the Poseidon path exists for the latency of a single proof only
    bool fused_top;
};
static TreeKernels tree_kernels(u32 hasher) {
    if (hasher == HASHER_KECCAK) return {k_kc_leaves, k_kc_fri_leaves, k_kc_level, false};
    return {k_hash_leaves, k_hash_fri_leaves, k_merkle_level, true};
}
// The levels above the leaf digests, up to the cap: wide levels one launch each, the top (at most 256 parents per cap
// subtree, up to nine levels) in one launch of a workgroup per cap node.
static int merkle_levels(Lane& L, const Domain& D, Tree& t, u32 batch) {
    const u32 cap_h = D.cap_height;
    if (t.bits <= cap_h) return 0;
    const u32 levels = t.bits - cap_h;                       // level l: 2^(bits-l-1) parents
    const TreeKernels k = tree_kernels(D.hasher);
    // The last `fused` levels (parents per cap subtree 2^(fused-1) .. 1) run as ONE launch of a workgroup per cap node -- for
    // SMALL batches only.  These levels are latency bound either way (a level is one permutation deep whatever its width), so
    // what the fusion buys is launches: 54 -> 18 per chunk, 118 -> 70 for the whole pipeline.  For a full chunk it costs time:
    // the waves of a fused walk stay resident for all its levels and slow each other down, where separately launched levels
    // shrink to one wave per SIMD as they narrow (measured per 128-proof chunk: nine levels in 256-thread workgroups + 3.3 ms,
    // seven levels in one wave + 1.3 ms against 21.1 ms).  Launch count does not matter there: the chip is busy throughout.
    const u32 fused = k.fused_top && batch <= 16 ? std::min<u32>(levels, 9) : 0;
    const u32 top_threads = 256;
    for (u32 l = 0; l < levels - fused; l++) {
        size_t parents = ((size_t)1 << t.bits) >> (l + 1);
        LAUNCH(L, "merkle_level", k.level, g1(parents, 256, batch), dim3(256), 0, t.dig + level_off(t.bits, l), t.dig + level_off(t.bits, l + 1), parents, t.stride());
    }
    if (fused) {
        // parents per cap subtree at the fused levels: 2^(fused-1) .. 1; those with more than 32 one thread per node, the rest cooperative
        const u32 direct = fused > 6 ? fused - 6 : 0;
        if (direct) LAUNCH(L, "merkle_top", k_merkle_top, dim3(1u << cap_h, batch), dim3(top_threads), 0, t.dig, t.stride(), t.bits, levels - fused, direct);
        LAUNCH(L, "merkle_top", k_merkle_top_coop, dim3(1u << cap_h, batch), dim3(256), 0, t.dig, t.stride(), t.bits, levels - fused + direct, fused - direct);
    }
    return 0;
}
static int merkle_build(Lane& L, const Domain& D, const u64* data, u32 cols, u32 active, size_t col_stride, size_t batch_stride, Tree& t, u32 batch) {
    size_t leaves = (size_t)1 << t.bits;
    LAUNCH(L, "hash_leaves", tree_kernels(D.hasher).leaves, g1(leaves, 256, batch), dim3(256), 0, data, (int)cols, (int)active, col_stride, batch_stride, leaves, t.dig,
           t.stride());
    return merkle_levels(L, D, t, batch);
}
static int challenger(p2_circuit* C, Workspace& W, u32 stage, const u64* observe, size_t stride, u32 len, u32 aux, u64 mod, u32 batch) {
    ChalArgs a{};
    a.st = W.d_chal_state;
    a.chal = W.d_chal;
    a.observe = observe;
    a.observe_stride = stride;
    a.observe_len = len;
    a.batch = batch;
    a.stage = stage;
    a.aux = aux;
    a.mod = mod;
    a.digest = C->d_digest;
    a.pi_hash = C->c.pi_slots.empty() ? nullptr : W.d_pi_hash;
    a.status = W.d_status;
    LAUNCH(W.lane, "challenger", k_challenger, g1((size_t)batch * 16, 64), dim3(64), 0, a);  // a 16-lane group per proof
    return 0;
}

// ---------------------------------------------------------------------------------- load / preprocess
static int circuit_setup(p2_circuit* C) {
    const Circuit& c = C->c;
    Domain& D = C->dom;
    const size_t n = C->n, N = C->N;
    const u32 R = c.cfg.num_routed_wires, ncc = c.num_constants_cols(), np = c.num_preprocessed();
    if (c.cfg.num_challenges > 2) return set_error("k_perm_chunks handles at most two challenges"), P2_ERR_INVALID;
    if (c.num_partial_products() + 1 > PERM_MAX_CHUNKS) return set_error("more partial-product chunks than k_perm_scan holds in registers"), P2_ERR_INVALID;
    {
        // the witness program, rescheduled for the device: contracted critical chains + single ops per level (witness_schedule.h)
        WitnessSchedule ws = schedule_witness(c, std::min<u32>(C->opt_witness_fuse, WITNESS_KMAX));
        if (ws.max_chain > (u32)WITNESS_KMAX) return set_error("internal: witness chain longer than the kernel is unrolled for"), P2_ERR_INVALID;
        C->witness_levels = (u32)ws.levels.size();
        C->witness_chains = (u32)ws.chains.size();
        if (upload(C->allocs, &C->d_ops, ws.ops.data(), ws.ops.size())) return P2_ERR_HIP;
        if (upload(C->allocs, &C->d_wlevels, ws.levels.data(), ws.levels.size())) return P2_ERR_HIP;
        if (upload(C->allocs, &C->d_wchains, ws.chains.data(), ws.chains.size())) return P2_ERR_HIP;
    }
    if (upload(C->allocs, &C->d_wire_slot, c.wire_slot.data(), c.wire_slot.size())) return P2_ERR_HIP;
    {
        const std::vector<u32> wired = wired_slot_list(c);
        C->n_wired = (u32)wired.size();
        if (upload(C->allocs, &C->d_wired_slots, wired.data(), wired.size())) return P2_ERR_HIP;
    }
    if (!c.pi_slots.empty() && upload(C->allocs, &C->d_pi_slots, c.pi_slots.data(), c.pi_slots.size())) return P2_ERR_HIP;
    {
        // witness generation resolves a lookup with ONE load: input value -> (flat entry index << 16) | output
        std::vector<u64> ent(c.luts.size() * 65536, ~0ull);
        std::vector<u32> pairs, offs(1, 0);
        for (size_t l = 0; l < c.luts.size(); l++) {
            for (size_t i = 0; i < c.luts[l].size(); i++) {
                auto pr = c.luts[l][i];
                if (ent[l * 65536 + pr.first] == ~0ull) ent[l * 65536 + pr.first] = ((u64)pairs.size() << 16) | pr.second;
                pairs.push_back((u32)pr.first | ((u32)pr.second << 16));
            }
            offs.push_back((u32)pairs.size());
        }
        C->total_lut_entries = pairs.size();
        if (upload(C->allocs, &C->d_lut_ent, ent.data(), ent.size())) return P2_ERR_HIP;
        if (upload(C->allocs, &C->d_lut_pairs, pairs.data(), pairs.size())) return P2_ERR_HIP;
        if (upload(C->allocs, &C->d_lut_offsets, offs.data(), offs.size())) return P2_ERR_HIP;
        if (upload(C->allocs, &C->d_num_lookups, c.num_lookups.data(), c.num_lookups.size())) return P2_ERR_HIP;
        if (upload(C->allocs, &C->d_lookup_rows, c.lookup_rows.data(), c.lookup_rows.size())) return P2_ERR_HIP;
    }
    {
        std::vector<int32_t> pi(n, -1);
        for (size_t k = 0; k < c.poseidon_rows.size(); k++) pi[c.poseidon_rows[k]] = (int32_t)k;
        if (upload(C->allocs, &C->d_pos_index, pi.data(), n)) return P2_ERR_HIP;
    }
    if (upload(C->allocs, &C->d_blind_rows, c.blind_rows.data(), c.blind_rows.size())) return P2_ERR_HIP;
    if (upload(C->allocs, &C->d_blind_zrows, (const u32*)c.blind_zrows.data(), 2 * c.blind_zrows.size())) return P2_ERR_HIP;
    if (upload(C->allocs, &C->d_sigmas, c.sigmas.data(), c.sigmas.size())) return P2_ERR_HIP;
    if (upload(C->allocs, &C->d_k_is, c.k_is.data(), c.k_is.size())) return P2_ERR_HIP;
    // twiddles, subgroup, coset tables (host-computed once; O(n) field ops)
    if (int rc = build_transform_tables(C->setup, D, C->allocs, &C->d_shift_inv_pows)) return rc;
    C->d_subgroup = D.d_tw_fwd_full;  // w^k, k < n
    {
        // per-point tables on the LDE coset (position p <-> natural index rev(p))
        std::vector<u64> xs(N), l0(N), zh_inv(8), w8inv(8), qscale(8);
        u64 wl = gl::root_of_unity((int)C->lde_bits);
        std::vector<u64> nat(N);
        u64 x = gl::MULT_GEN;
        for (size_t i = 0; i < N; i++) {
            nat[i] = x;
            x = gl::mul(x, wl);
        }
        u64 gn = gl::pow(gl::MULT_GEN, n), w8 = gl::root_of_unity((int)c.cfg.rate_bits);
        std::vector<u64> zh(8);
        for (u32 j = 0; j < 8; j++) {
            zh[j] = gl::sub(gl::mul(gn, gl::pow(w8, j)), 1);
            zh_inv[j] = gl::inv(zh[j]);
        }
        quotient_chunk_scales(D.logn, w8inv.data(), qscale.data());
        // batch inversion of n*(x-1)
        std::vector<u64> den(N), pref(N);
        u64 acc = 1;
        for (size_t i = 0; i < N; i++) {
            den[i] = gl::mul((u64)n % gl::P, gl::sub(nat[i], 1));
            pref[i] = acc;
            acc = gl::mul(acc, den[i]);
        }
        u64 inv_all = gl::inv(acc);
        for (size_t i = N; i-- > 0;) {
            u64 di = gl::mul(inv_all, pref[i]);
            inv_all = gl::mul(inv_all, den[i]);
            size_t p = gl::bitrev((u32)i, (int)C->lde_bits);
            xs[p] = nat[i];
            l0[p] = gl::mul(zh[i & 7], di);
        }
        if (upload(C->allocs, &C->d_xs, xs.data(), N)) return P2_ERR_HIP;
        if (upload(C->allocs, &C->d_l0, l0.data(), N)) return P2_ERR_HIP;
        if (upload(C->allocs, &C->d_zh_inv, zh_inv.data(), 8)) return P2_ERR_HIP;
        if (upload(C->allocs, &C->d_w8inv, w8inv.data(), 8)) return P2_ERR_HIP;
        if (upload(C->allocs, &C->d_qscale, qscale.data(), 8)) return P2_ERR_HIP;
    }
    // constants | sigmas commitment on the device
    {
        Oracle& o = C->pre;
        o.cols = o.tree_cols = np;
        o.tree.bits = C->lde_bits;
        if (dalloc(C->allocs, &o.vals, (size_t)np * n) || dalloc(C->allocs, &o.coef, (size_t)np * n) || dalloc(C->allocs, &o.lde, (size_t)np * N) ||
            dalloc(C->allocs, &o.tree.dig, o.tree.stride()))
            return P2_ERR_HIP;
        HIPCHECK(hipMemcpy(o.vals, c.constants.data(), (size_t)ncc * n * 8, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(o.vals + (size_t)ncc * n, c.sigmas.data(), (size_t)R * n * 8, hipMemcpyHostToDevice));
        if (intt_cols(C->setup, D, o.vals, o.coef, np, 0, 1, o.lde, 0)) return P2_ERR_HIP;
        if (lde_cols(C->setup, D, o.coef, 0, o.lde, 0, np, 0, 1)) return P2_ERR_HIP;
        if (merkle_build(C->setup, D, o.lde, np, np, N, 0, o.tree, 1)) return P2_ERR_HIP;
        HIPCHECK(hipStreamSynchronize(C->setup.stream));
        size_t cap_n = (size_t)1 << c.cfg.cap_height;
        std::vector<u64> cap(4 * cap_n);
        HIPCHECK(hipMemcpy(cap.data(), o.tree.dig + cap_off(o.tree, c.cfg.cap_height), cap.size() * 8, hipMemcpyDeviceToHost));
        // circuit digest = hash_no_pad(cap || hash_pad([]) || degree_bits), both hashes by the tree hasher (upstream C::Hasher)
        const u64 padded[12] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};  // hash_pad of the empty domain separator
        const Hash4 dom_sep = h_hash_or_noop(padded, 12, c.cfg.hasher);
        std::vector<u64> parts(cap);
        parts.insert(parts.end(), dom_sep.e, dom_sep.e + 4);
        parts.push_back(c.degree_bits);
        const Hash4 digest = h_hash_or_noop(parts.data(), parts.size(), c.cfg.hasher);
        C->verifier_data = cap;
        C->verifier_data.insert(C->verifier_data.end(), digest.e, digest.e + 4);
        if (upload(C->allocs, &C->d_digest, digest.e, 4)) return P2_ERR_HIP;
    }
    return 0;
}

// Reads the event pairs of every lane into the timing map (waits for the launches they bracket).
static void collect_timing(p2_circuit* C) {
    std::vector<Lane*> lanes{&C->setup};
    for (auto& W : C->ws) lanes.push_back(&W->lane);
    for (Lane* L : lanes) {
        for (auto& pe : L->pending) {
            float ms = 0;
            (void)hipEventSynchronize(pe.second.second);
            (void)hipEventElapsedTime(&ms, pe.second.first, pe.second.second);
            auto& t = C->times[pe.first];
            t.first += ms;
            t.second++;
        }
        L->pending.clear();  // (destroys the events)
    }
}
// Drains and releases every per-stream workspace; the handle is left with none (chunk == 0), ready to allocate again.
static void release_workspaces(p2_circuit* C) {
    for (auto& W : C->ws)
        if (W->lane.stream) (void)hipStreamSynchronize(W->lane.stream);
    C->ws.clear();
    C->chunk = 0;
    C->ws_inputs = 0;
    C->witness_recorded = false;
}
// The reference tables of a workspace: the coefficient column behind every opening (the two FRI batches, in observed order)
// and the opening set itself.
static int setup_polyrefs(p2_circuit* C, Workspace& W) {
    const OpeningSet& os = C->layout.set;
    const Oracle* oracle[OS_SLOTS] = {&C->pre, &W.wires, &W.zs, &W.zs, &W.quot};
    std::vector<PolyRef> v;
    for (OpenGroup k : OPEN_OBSERVED)
        for (u32 i = os.g[k].lo; i < os.g[k].hi; i++) {
            const Oracle& o = *oracle[os.g[k].slot];
            v.push_back({i < o.cols ? o.coef : nullptr, o.coef_stride, i, 0});  // past `cols`: identically zero, never materialised
        }
    C->n_b0 = os.n_b0;
    C->n_b1 = os.n_b1;
    // the opening set: every materialised column of every oracle at zeta, the Z columns at g zeta as well
    std::vector<EvalRef> e;
    for (u32 b = 0; b < OS_SLOTS; b++)
        for (u32 i = 0; i < oracle[b]->cols; i++) e.push_back({oracle[b]->coef, oracle[b]->coef_stride, i, b == OS_Z_NEXT, os.slot_base[b] + i, 0});
    C->n_evalrefs = (u32)e.size();
    if (upload(W.mem, &W.d_evalrefs, e.data(), e.size())) return P2_ERR_HIP;
    return upload(W.mem, &W.d_polyrefs, v.data(), v.size());
}
// Test hook (P2AES_TEST_FAIL_ALLOC_AFTER=k in the environment when the handle is loaded): the k-th workspace allocation
// fails as if the device were out of memory.  Exercises the roll-back below without needing a full HBM.
static int dalloc_ws(p2_circuit* C, Allocs& mem, size_t& counter, void** p, size_t bytes) {
    if (C->fail_alloc_after >= 0 && (long)counter++ == C->fail_alloc_after) {
        C->fail_alloc_after = -1;  // one shot: the retry must succeed
        return set_error("hipMalloc: injected allocation failure (test hook)"), P2_ERR_HIP;
    }
    HIPCHECK_AS("hipMalloc(&q, std::max<size_t>(bytes, 8))", mem.alloc(p, std::max<size_t>(bytes, 8)));
    return 0;
}
// entries of the per-proof table of FRI alpha powers: the longer of the two batches.  From the layout, which the handle has from
// load on -- C->n_b0 / n_b1 are set by setup_polyrefs, at the END of the first build_workspace.
static u32 fri_pow_count(const p2_circuit* C) { return std::max<u32>(std::max(C->layout.set.n_b0, C->layout.set.n_b1), 1); }
static int build_workspace(p2_circuit* C, Workspace* W, size_t chunk, u32 ws_inputs, size_t& counter) {
    const Circuit& c = C->c;
    const size_t n = C->n, N = C->N;
    const u32 NC = c.cfg.num_challenges;
    W->lane.timing = C->timing_on;
    if (W->lane.open(hipStreamNonBlocking) != hipSuccess) return set_error("hipStreamCreate failed"), P2_ERR_HIP;
    if (W->done.create(hipEventDisableTiming) != hipSuccess) return set_error("hipEventCreate failed"), P2_ERR_HIP;
#define WS_ALLOC(field, count)                                                                       \
    if (dalloc_ws(C, W->mem, counter, (void**)&(field), (size_t)(count) * sizeof(*(field)))) return P2_ERR_HIP
    WS_ALLOC(W->d_input_slots, ws_inputs);
    WS_ALLOC(W->d_input_values, chunk * ws_inputs);
    WS_ALLOC(W->d_values, chunk * c.num_slots);
    WS_ALLOC(W->d_mult, chunk * std::max<size_t>(C->total_lut_entries, 1));
    WS_ALLOC(W->d_status, chunk);
    WS_ALLOC(W->d_advice, chunk * std::max<size_t>(c.poseidon_rows.size(), 1) * 55);
    WS_ALLOC(W->d_pi_hash, chunk * 4);
    W->wires.cols = C->active_wires, W->wires.tree_cols = c.cfg.num_wires;
    W->zs.cols = W->zs.tree_cols = c.num_zs_cols();
    W->quot.cols = W->quot.tree_cols = c.num_quotient_cols();
    for (Oracle* o : {&W->wires, &W->zs, &W->quot}) {
        o->salt = c.salt();
        o->coef_stride = (size_t)o->cols * n;
        o->lde_stride = (size_t)(o->cols + o->salt) * N;
        o->tree.bits = C->lde_bits;
        if (o != &W->quot) WS_ALLOC(o->vals, chunk * o->coef_stride);  // the quotient is evaluated on the LDE domain: d_qvals
        WS_ALLOC(o->coef, chunk * o->coef_stride);
        WS_ALLOC(o->lde, chunk * o->lde_stride);
        WS_ALLOC(o->tree.dig, chunk * o->tree.stride());
    }
    WS_ALLOC(W->d_permq, chunk * NC * (c.num_partial_products() + 1) * n);
    WS_ALLOC(W->d_perm_seg, chunk * NC * PERM_MAX_SEGS);
    WS_ALLOC(W->d_fri_seg, chunk * 4 * FRI_MAX_SEGS);
    WS_ALLOC(W->d_lktmp, chunk * NC * (c.num_sldc_polys() + 1) * n);
    WS_ALLOC(W->d_qvals, chunk * NC * N);
    WS_ALLOC(W->d_qres, chunk * NC * N);
    WS_ALLOC(W->d_chal_state, chunk);
    WS_ALLOC(W->d_chal, chunk * CH_WORDS);
    WS_ALLOC(W->d_pows, chunk * 8 * n);
    WS_ALLOC(W->d_ev, chunk * 2 * C->ev_count);
    WS_ALLOC(W->d_obs, chunk * 2 * C->n_obs);
    WS_ALLOC(W->d_comp, chunk * 4 * n);
    WS_ALLOC(W->d_apow, chunk * 2 * APOW_STRIDE);
    WS_ALLOC(W->d_ztab, chunk * 4 * zeta_tab_words((u32)n));
    WS_ALLOC(W->d_fripow, chunk * 2 * fri_pow_count(C));
    u32 logn_r = C->dom.logn;
    for (u32 r = 0; r <= C->dom.arities.size(); r++) {
        size_t n_r = (size_t)1 << logn_r;
        WS_ALLOC(W->d_fri_coef[r], chunk * 2 * n_r);
        if (r < C->dom.arities.size()) {
            WS_ALLOC(W->d_fri_vals[r], chunk * 2 * 8 * n_r);
            W->fri_tree[r].bits = logn_r + c.cfg.rate_bits - C->dom.arities[r];
            WS_ALLOC(W->fri_tree[r].dig, chunk * W->fri_tree[r].stride());
            logn_r -= C->dom.arities[r];
        }
    }
    WS_ALLOC(W->d_pow_best, chunk);
    WS_ALLOC(W->d_pow_list, chunk + 1);
    WS_ALLOC(W->d_proofs, chunk * C->pbytes);
#undef WS_ALLOC
    return setup_polyrefs(C, *W);
}
// Makes sure `nstreams` workspaces of `chunk` proofs and `n_inputs` input targets exist.  All-or-nothing: the new shape
// (C->chunk, C->ws_inputs, C->ws) is published only after every allocation has succeeded; on failure whatever was
// allocated is released and the handle is left without workspaces, so that a retry (with a smaller batch) allocates
// afresh instead of launching kernels on null pointers.
static int alloc_workspace(p2_circuit* C, size_t chunk, u32 n_inputs, size_t nstreams) {
    if (C->chunk >= chunk && C->ws_inputs >= n_inputs && C->ws.size() >= nstreams) return 0;
    if (C->chunk != 0) {
        // a later call wants a bigger shape (a first prove(pw) sizes the workspace for one proof; a batch follows):
        // drain the proving streams, release the old workspaces and allocate the larger ones
        if (C->timing_on) collect_timing(C);
        chunk = std::max(chunk, C->chunk);
        n_inputs = std::max(n_inputs, C->ws_inputs);
        nstreams = std::max(nstreams, C->ws.size());
        release_workspaces(C);
    }
    const u32 ws_inputs = std::max<u32>(n_inputs, 1);
    size_t counter = 0;
    for (size_t wi = 0; wi < nstreams; wi++) {
        C->ws.push_back(std::make_unique<Workspace>());  // owned by the handle from here on: release_workspaces() frees a half-built one too
        if (build_workspace(C, C->ws.back().get(), chunk, ws_inputs, counter)) {
            std::string why = g_last_error;
            release_workspaces(C);
            set_error("workspace allocation failed (" + why + "); the handle holds no workspace now, a smaller batch may fit");
            return P2_ERR_HIP;
        }
    }
    C->chunk = chunk;
    C->ws_inputs = ws_inputs;
    return 0;
}

// ---------------------------------------------------------------------------------- the pipeline
// Commits one oracle and feeds its cap to the transcript: inverse transform of the values (where the oracle has them: the
// quotient arrives as coefficients), LDE, salt columns (zk), Merkle tree, challenger stage `stage` (0, 1, 2 = wires, Z, quotient).
static int commit_oracle(p2_circuit* C, Workspace& W, Oracle& o, u32 stage, u32 aux, u64 proof_base, u32 B) {
    const size_t N = C->N;
    const u32 cap_h = C->dom.cap_height;
    if (o.vals && intt_cols(W.lane, C->dom, o.vals, o.coef, o.cols, o.coef_stride, B, o.lde, o.lde_stride)) return P2_ERR_HIP;
    if (lde_cols(W.lane, C->dom, o.coef, o.coef_stride, o.lde, o.lde_stride, o.cols, 0, B)) return P2_ERR_HIP;
    if (o.salt)
        LAUNCH(W.lane, "fill_salt", k_fill_salt, g1((size_t)o.salt * N / 8, 256, B), dim3(256), 0, o.lde + (size_t)o.cols * N, o.lde_stride, N, C->zk_key, proof_base,
               (u64)ZK_SALT + 1 + stage);
    if (merkle_build(W.lane, C->dom, o.lde, o.tree_cols + o.salt, o.cols + o.salt, N, o.lde_stride, o.tree, B)) return P2_ERR_HIP;
    return challenger(C, W, stage, o.tree.dig + cap_off(o.tree, cap_h), o.tree.stride(), 4u << cap_h, aux, 0, B);
}
// the target slots are already in the workspace (d_input_slots); d_values: [batch][n_inputs] device; proofs/status: device.
// n_out > 0: the values of W.d_out_slots are read back into d_out [B][n_out] right behind the witness.
static int prove_chunk(p2_circuit* C, Workspace& W, u32 B, u32 n_inputs, const u64* d_values, u32 n_out, u64* d_out, uint8_t* d_proofs, int* d_status_out,
                       u64 proof_base) {
    const Circuit& c = C->c;
    const size_t n = C->n, N = C->N;
    const u32 R = c.cfg.num_routed_wires, NC = c.cfg.num_challenges, npp = c.num_partial_products(), nlp = c.num_lookup_polys();
    const u32 qc = c.num_quotient_cols(), act = C->active_wires, ncc = c.num_constants_cols();
    const u32 cap_h = c.cfg.cap_height, cap_words = 4u << cap_h, nsldc = c.num_sldc_polys();
    const size_t ws = W.wires.coef_stride, wls = W.wires.lde_stride, zs_s = W.zs.coef_stride, zl_s = W.zs.lde_stride;
    hipStream_t st = W.lane.stream;
    // 1. witness
    HIPCHECK(hipMemsetAsync(W.d_mult, 0, (size_t)B * std::max<size_t>(C->total_lut_entries, 1) * 4, st));
    {
        WitnessArgs a{};
        a.ops = C->d_ops;
        a.levels = C->d_wlevels;
        a.chains = C->d_wchains;
        a.num_levels = C->witness_levels;
        a.num_slots = c.num_slots;
        a.n_inputs = n_inputs;
        a.input_slots = W.d_input_slots;
        a.input_values = d_values;
        a.values = W.d_values;
        a.lut_ent = C->d_lut_ent;
        a.mult = W.d_mult;
        a.total_lut_entries = C->total_lut_entries;
        a.status = W.d_status;
        a.wire_slot = C->d_wire_slot;
        a.advice = W.d_advice;
        a.n = (u32)n;
        a.num_poseidon_rows = (u32)c.poseidon_rows.size();
        // 512 threads (8 waves, <= 128 VGPRs each) leave room on the compute unit: a 1024-thread workgroup needs a
        // completely empty unit and waits for the tail of whatever wide kernel the other stream is running.
        const u32 WITNESS_THREADS = 512;
        // Witness kernels of successive chunks run one after the other (each occupies only B compute units): without
        // this the two proving streams stay in lockstep -- both in witness generation with the chip idle, then both in
        // the wide kernels -- and a deep circuit's witness time is never hidden.  Chained, chunk k+1's witness runs
        // under chunk k's commitments.
        if (C->witness_recorded) HIPCHECK(hipStreamWaitEvent(W.lane.stream, C->ev_witness, 0));
        if (ecstep_gate_index(c) >= 0) {
            const bool pos = !c.poseidon_rows.empty();
            if (!pos && C->witness_chains) LAUNCH(W.lane, "witness", (k_ecwitness<false, true>), dim3(B), dim3(WITNESS_THREADS), 0, a);
            if (!pos && !C->witness_chains) LAUNCH(W.lane, "witness", (k_ecwitness<false, false>), dim3(B), dim3(WITNESS_THREADS), 0, a);
            if (pos && C->witness_chains) LAUNCH(W.lane, "witness", (k_ecwitness<true, true>), dim3(B), dim3(WITNESS_THREADS), 0, a);
            if (pos && !C->witness_chains) LAUNCH(W.lane, "witness", (k_ecwitness<true, false>), dim3(B), dim3(WITNESS_THREADS), 0, a);
        } else if (c.poseidon_rows.empty()) {
            if (C->witness_chains)
                LAUNCH(W.lane, "witness", (k_witness<false, true>), dim3(B), dim3(WITNESS_THREADS), 0, a);
            else
                LAUNCH(W.lane, "witness", (k_witness<false, false>), dim3(B), dim3(WITNESS_THREADS), 0, a);
        } else {
            if (C->witness_chains)
                LAUNCH(W.lane, "witness", (k_witness<true, true>), dim3(B), dim3(WITNESS_THREADS), 0, a);
            else
                LAUNCH(W.lane, "witness", (k_witness<true, false>), dim3(B), dim3(WITNESS_THREADS), 0, a);
        }
        HIPCHECK(hipEventRecord(C->ev_witness, W.lane.stream));
        C->witness_recorded = true;
    }
    if (!c.pi_slots.empty())
        LAUNCH(W.lane, "pi_hash", k_pi_hash, g1((size_t)B * 16, 64), dim3(64), 0, W.d_values, c.num_slots, C->d_pi_slots, (u32)c.pi_slots.size(), B,
               W.d_pi_hash, d_proofs, C->pbytes, C->layout.body_bytes);  // a 16-lane group per proof
    if (n_out) LAUNCH(W.lane, "gather_slots", k_gather_slots, g1(n_out, 256, B), dim3(256), 0, W.d_values, c.num_slots, W.d_out_slots, n_out, d_out);
    LAUNCH(W.lane, "fill_wires", k_fill_wires, g1((size_t)R * n, 256, B), dim3(256), 0, C->d_wire_slot, W.d_values, W.wires.vals, (size_t)R * n, c.num_slots, ws,
           W.d_status);
    if (act > R)
        LAUNCH(W.lane, "fill_advice", k_fill_advice, g1((size_t)55 * n, 256, B), dim3(256), 0, C->d_pos_index, W.d_advice, W.wires.vals, (u32)n,
               (u32)c.poseidon_rows.size(), ws);
    if (c.cfg.zero_knowledge) {
        size_t cnt = (c.blind_rows.size() * 135 + 7) / 8 + (c.blind_zrows.size() * 80 + 7) / 8;  // PRF blocks of eight elements
        LAUNCH(W.lane, "fill_blind", k_fill_blind, g1(std::max<size_t>(cnt, 1), 256, B), dim3(256), 0, C->d_blind_rows, (u32)c.blind_rows.size(), C->d_blind_zrows,
               (u32)c.blind_zrows.size(), W.wires.vals, ws, (u32)n, C->zk_key, proof_base);
    }
    if (!c.luts.empty()) {
        LutRowsArgs a{};
        a.lut_pairs = C->d_lut_pairs;
        a.lut_offsets = C->d_lut_offsets;
        a.rows = C->d_lookup_rows;
        a.num_lookups = C->d_num_lookups;
        a.mult = W.d_mult;
        a.total_lut_entries = C->total_lut_entries;
        a.wires = W.wires.vals;
        a.wires_batch_stride = ws;
        a.n = (u32)n;
        a.num_luts = (u32)c.luts.size();
        LAUNCH(W.lane, "lut_rows", k_lut_rows, g1(std::max<size_t>(C->total_lut_entries, 256), 256, B), dim3(256), 0, a);
    }
    // 2. wires commitment; 3. betas, gammas, deltas
    if (commit_oracle(C, W, W.wires, 0, nlp ? 1 : 0, proof_base, B)) return P2_ERR_HIP;
    // 4. partial products and Z
    HIPCHECK(hipMemsetAsync(W.zs.vals, 0, (size_t)B * zs_s * 8, st));
    LAUNCH(W.lane, "perm_chunks", k_perm_chunks, g1(n, 256, B), dim3(256), 0, W.wires.vals, ws, C->d_sigmas, C->d_k_is, C->d_subgroup, W.d_chal,
           W.d_permq, (size_t)NC * (npp + 1) * n, (u32)n, R, c.cfg.quotient_degree_factor, npp + 1, NC);
    {
        // columns longer than 2^14 rows in segments of 2^14 (at most PERM_MAX_SEGS), a workgroup per segment
        const u32 segs = (u32)std::min<size_t>(std::max<size_t>(n >> 14, 1), PERM_MAX_SEGS);
        if (segs > 1)
            LAUNCH(W.lane, "perm_scan", k_perm_seg_products, dim3(NC, B, segs), dim3(1024), 0, W.d_permq, (size_t)NC * (npp + 1) * n, W.d_perm_seg, (u32)n, npp + 1);
        LAUNCH(W.lane, "perm_scan", k_perm_scan, dim3(NC, B, segs), dim3(1024), 0, W.d_permq, (size_t)NC * (npp + 1) * n, W.zs.vals, zs_s, (u32)n, npp + 1, NC,
               segs > 1 ? W.d_perm_seg : nullptr);
    }
    // 5. lookup polynomials
    if (nlp) {
        LookupArgs a{};
        a.wires = W.wires.vals;
        a.wires_batch_stride = ws;
        a.chal = W.d_chal;
        a.zs = W.zs.vals;
        a.zs_batch_stride = zs_s;
        a.tmp = W.d_lktmp;
        a.tmp_batch_stride = (size_t)NC * (nsldc + 1) * n;
        a.rows = C->d_lookup_rows;
        a.n = (u32)n;
        a.num_luts = (u32)c.luts.size();
        a.num_sldc = nsldc;
        a.lut_deg = c.lut_degree();
        a.lu_deg = c.cfg.quotient_degree_factor - 1;
        a.num_challenges = NC;
        a.zs_lookup_col0 = c.num_zs_pp();
        LAUNCH(W.lane, "lookup_terms", k_lookup_terms, g1(n, 256, B, NC * (nsldc + 1)), dim3(256), 0, a);
        LAUNCH(W.lane, "lookup_scan", k_lookup_scan, dim3((u32)c.luts.size(), B, NC), dim3(1024), 0, a);
    }
    // 6. zs commitment, alphas
    if (commit_oracle(C, W, W.zs, 1, 0, proof_base, B)) return P2_ERR_HIP;
    // 7. quotient
    {
        QuotientArgs a{};
        a.pre_lde = C->pre.lde;
        a.wires_lde = W.wires.lde;
        a.zs_lde = W.zs.lde;
        a.wires_batch_stride = wls;
        a.zs_batch_stride = zl_s;
        a.chal = W.d_chal;
        a.xs = C->d_xs;
        a.l0 = C->d_l0;
        a.zh_inv = C->d_zh_inv;
        a.k_is = C->d_k_is;
        a.out = W.d_qvals;
        a.out_batch_stride = (size_t)NC * N;
        a.n = (u32)n;
        a.logn = C->dom.logn;
        a.rate_bits = c.cfg.rate_bits;
        a.R = R;
        a.ncc = ncc;
        a.nsel = c.num_selectors();
        a.nls = c.num_lookup_selectors;
        a.NC = NC;
        a.npp = npp;
        a.qdf = c.cfg.quotient_degree_factor;
        a.num_luts = (u32)c.luts.size();
        a.nsldc = nsldc;
        a.lut_deg = nlp ? c.lut_degree() : 0;
        a.nlp = nlp;
        a.num_gates = (u32)c.gates.size();
        a.num_gate_constraints = c.num_gate_constraints;
        fill_gate_table(c, a);
        for (u32 l = 0; l < c.luts.size(); l++) a.lut_last_row[l] = c.lookup_rows[l].last_lut;
        a.zs_values = W.zs.vals;
        a.zs_values_batch_stride = zs_s;
        a.pi_hash = c.pi_slots.empty() ? nullptr : W.d_pi_hash;
        a.apow = W.d_apow;
        {
            u32 nlk = nlp ? 4 + (u32)c.luts.size() + 2 * nsldc : 0;
            u32 nterms = NC + NC * (npp + 1) + NC * nlk + c.num_gate_constraints;
            if (nterms > APOW_STRIDE) return set_error("internal: too many vanishing terms for the alpha-power table"), P2_ERR_INVALID;
            LAUNCH(W.lane, "alpha_pows", k_alpha_pows, g1(2 * B, 64), dim3(64), 0, W.d_chal, W.d_apow, B, nterms);
        }
        if (c.poseidon_rows.empty())
            LAUNCH(W.lane, "quotient", (k_quotient<false, true>), g1(N, 256, B), dim3(256), 0, a);  // the wire columns read once
        else
            LAUNCH(W.lane, "quotient", k_quotient<true>, g1(N, 256, B), dim3(256), 0, a);
        const int eg = ecstep_gate_index(c);
        if (eg >= 0) {  // k_quotient skips the kind: its terms are added behind it (the stage's time is the sum of the two)
            EcQuotientArgs e{};
            e.pre_lde = a.pre_lde, e.wires_lde = a.wires_lde, e.wires_batch_stride = a.wires_batch_stride, e.zh_inv = a.zh_inv, e.apow = a.apow;
            e.out = a.out, e.out_batch_stride = a.out_batch_stride;
            e.n = a.n, e.logn = a.logn, e.rate_bits = a.rate_bits, e.nsel = a.nsel;
            e.idx_gate = NC + NC * (npp + 1) + NC * (nlp ? 4 + (u32)c.luts.size() + 2 * nsldc : 0);
            e.gate = (u32)eg, e.gate_sel = a.gate_sel[eg], e.group_lo = a.group_lo[eg], e.group_hi = a.group_hi[eg];
            LAUNCH(W.lane, "quotient", k_ecstep_post, g1(N, 256, B), dim3(256), 0, e);
        }
        if (quotient_chunks(W.lane, C->dom, W.d_qvals, W.d_qres, W.quot.coef, NC, (size_t)qc * n, B, C->d_shift_inv_pows, C->d_w8inv, C->d_qscale)) return P2_ERR_HIP;
    }
    if (commit_oracle(C, W, W.quot, 2, c.degree_bits, proof_base, B)) return P2_ERR_HIP;
    // 8. openings
    // (the table launch goes under the same name: the stage's time is the sum of the two)
    LAUNCH(W.lane, "zeta_pows", k_zeta_tabs, g1(ZT_LO + zeta_tab_hi((u32)n), 256, B, 4), dim3(256), 0, W.d_chal, W.d_ztab, (u32)n, gl::root_of_unity((int)C->dom.logn));
    LAUNCH(W.lane, "zeta_pows", k_zeta_pows, g1(n, 256, B, 4), dim3(256), 0, W.d_ztab, W.d_pows, (size_t)8 * n, (u32)n);
    HIPCHECK(hipMemsetAsync(W.d_ev, 0, (size_t)B * 2 * C->ev_count * 8, st));
    {
        const size_t evs = 2 * (size_t)C->ev_count;
        u64* ev = W.d_ev;
        LAUNCH(W.lane, "eval_polys", k_eval_polys_refs, dim3(C->n_evalrefs, B), dim3(256), 0, W.d_evalrefs, W.d_pows, (size_t)8 * n, (u32)n, ev, evs);
        LAUNCH(W.lane, "gather_ext", k_gather_ext, g1(C->n_obs, 256, B), dim3(256), 0, W.d_ev, evs, C->d_map_obs, C->n_obs, W.d_obs, (size_t)2 * C->n_obs);
    }
    if (challenger(C, W, 3, W.d_obs, (size_t)2 * C->n_obs, 2 * C->n_obs, 0, 0, B)) return P2_ERR_HIP;
    // 9. FRI: compose, divide, commit phase
    {
        const u32 npow = fri_pow_count(C);
        LAUNCH(W.lane, "fri_compose", k_fri_alpha_pows, g1(npow, 64, B), dim3(64), 0, W.d_chal, W.d_fripow, npow);
        LAUNCH(W.lane, "fri_compose", k_fri_compose, g1(n, 256, B), dim3(256), 0, W.d_polyrefs, C->n_b0, C->n_b1, W.d_fripow, npow, (u32)n, W.d_comp, (size_t)4 * n);
    }
    {
        const u32 segs = (u32)std::min<size_t>(std::max<size_t>(n >> 14, 1), FRI_MAX_SEGS);  // as in the permutation scan
        if (segs > 1)
            LAUNCH(W.lane, "fri_divide", k_fri_seg_sums, dim3(B, segs), dim3(1024), 0, W.d_comp, (size_t)4 * n, W.d_pows, (size_t)8 * n, (u32)n, W.d_fri_seg);
        LAUNCH(W.lane, "fri_divide", k_fri_divide, dim3(B, segs), dim3(1024), 0, W.d_comp, (size_t)4 * n, W.d_pows, (size_t)8 * n, W.d_chal, (u32)n, C->n_b1,
               W.d_fri_coef[0], (size_t)2 * n, segs > 1 ? W.d_fri_seg : nullptr);
    }
    {
        u32 logn_r = C->dom.logn;
        for (u32 r = 0; r < C->dom.arities.size(); r++) {
            size_t n_r = (size_t)1 << logn_r, len = 8 * n_r;
            u32 arity = 1u << C->dom.arities[r];
            if (lde_cols(W.lane, C->dom, W.d_fri_coef[r], 2 * n_r, W.d_fri_vals[r], 2 * len, 2, r, B)) return P2_ERR_HIP;
            Tree& t = W.fri_tree[r];
            size_t leaves = len / arity;
            LAUNCH(W.lane, "hash_fri_leaves", tree_kernels(C->dom.hasher).fri_leaves, g1(leaves, 256, B), dim3(256), 0, W.d_fri_vals[r], len, 2 * len, (int)arity, t.dig,
                   t.stride());
            if (merkle_levels(W.lane, C->dom, t, B)) return P2_ERR_HIP;
            if (challenger(C, W, 4, t.dig + cap_off(t, cap_h), t.stride(), cap_words, r, 0, B)) return P2_ERR_HIP;
            size_t n_next = n_r >> C->dom.arities[r];
            LAUNCH(W.lane, "fri_fold", k_fri_fold, g1(n_next, 256, B), dim3(256), 0, W.d_fri_coef[r], n_r, 2 * n_r, W.d_fri_coef[r + 1], n_next, 2 * n_next, W.d_chal, r,
                   arity);
            logn_r -= C->dom.arities[r];
        }
        // final polynomial (interleave components for observation)
        size_t fl = (size_t)1 << logn_r;
        u32 R_ = (u32)C->dom.arities.size();
        LAUNCH(W.lane, "interleave", k_interleave_ext, g1(fl, 256, B), dim3(256), 0, W.d_fri_coef[R_], fl, 2 * fl, W.d_obs, (size_t)2 * C->n_obs);
        if (challenger(C, W, 5, W.d_obs, (size_t)2 * C->n_obs, (u32)(2 * fl), 0, 0, B)) return P2_ERR_HIP;
        // proof of work
        HIPCHECK(hipMemsetAsync(W.d_pow_best, 0xFF, (size_t)B * 8, st));
        {
            u32 block0 = 0;
            for (int ph = 0; ph < 3; ph++) {
                u32* list = ph ? W.d_pow_list : nullptr;
                if (ph) LAUNCH(W.lane, "pow", k_pow_compact, dim3(1), dim3(256), 0, W.d_pow_best, B, W.d_pow_list, W.d_pow_list + C->chunk);
                const u32 slots = ph ? std::min<u32>(B, POW_PHASE_SLOTS[ph]) : B;
                LAUNCH(W.lane, "pow", k_pow, dim3(slots, POW_PHASE_BLOCKS[ph]), dim3(256), 0, W.d_chal_state, W.d_chal, (int)c.cfg.pow_bits, W.d_pow_best,
                       block0, (const u32*)list, (const u32*)(list ? list + C->chunk : nullptr));
                block0 += POW_PHASE_BLOCKS[ph];
            }
        }
        LAUNCH(W.lane, "pow_finish", k_pow_finish, g1(B, 64), dim3(64), 0, W.d_chal, W.d_pow_best, B, W.d_status);
        if (challenger(C, W, 6, W.d_obs, 0, 0, c.cfg.num_query_rounds, (u64)N, B)) return P2_ERR_HIP;
        // 10. proof assembly
        const ProofLayout& L = C->layout;
        ProofSegs segs{};
        u32 nseg = 0;
        segs.proofs = d_proofs;
        segs.proof_bytes = L.bytes;
        const Oracle* oracles[4] = {&C->pre, &W.wires, &W.zs, &W.quot};
        for (int o = 1; o < 4; o++) {
            const Tree& t = oracles[o]->tree;
            segs.s[nseg++] = ProofSeg{t.dig + cap_off(t, cap_h), nullptr, t.stride(), 0, L.caps_off[o - 1], cap_words, 0};
        }
        segs.s[nseg++] = ProofSeg{W.d_ev, C->d_map_ser, 2 * (size_t)C->ev_count, 0, L.open[0].off, C->n_ser, 2};
        if (R_ + 6 > 12) return set_error("internal: more FRI rounds than proof segments"), P2_ERR_INVALID;
        for (u32 r = 0; r < R_; r++) {
            Tree& t = W.fri_tree[r];
            segs.s[nseg++] = ProofSeg{t.dig + cap_off(t, cap_h), nullptr, t.stride(), 0, L.fri_caps_off + r * L.cap_bytes, cap_words, 0};
        }
        QueryArgs q{};
        for (int o = 0; o < 4; o++) {
            const Oracle& from = *oracles[o];
            q.oracles[o].lde = from.lde;
            q.oracles[o].lde_batch_stride = from.lde_stride;
            q.oracles[o].digests = from.tree.dig;
            q.oracles[o].dig_batch_stride = from.dig_stride();
            q.oracles[o].cols = from.tree_cols + from.salt;  // blinded leaves end with the salt
            q.oracles[o].active_cols = from.cols + from.salt;
        }
        q.lde_bits = C->lde_bits;
        q.cap_height = cap_h;
        q.num_queries = c.cfg.num_query_rounds;
        q.num_rounds = R_;
        u32 lb = C->lde_bits;
        for (u32 r = 0; r < R_; r++) {
            q.arity_bits[r] = C->dom.arities[r];
            q.fri_vals[r] = W.d_fri_vals[r];
            q.fri_vals_batch_stride[r] = (size_t)2 << lb;
            q.fri_bits[r] = lb;
            q.fri_digests[r] = W.fri_tree[r].dig;
            q.fri_dig_batch_stride[r] = W.fri_tree[r].stride();
            lb -= C->dom.arities[r];
        }
        q.chal = W.d_chal;
        q.proofs = d_proofs;
        q.proof_bytes = L.bytes;
        q.queries_off = L.queries_off;
        q.query_bytes = L.query_bytes;
        LAUNCH(W.lane, "write_queries", k_write_queries, dim3(c.cfg.num_query_rounds, B), dim3(256), 0, q);
        segs.s[nseg++] = ProofSeg{W.d_fri_coef[R_], nullptr, 2 * fl, fl, L.final_off, (u32)fl, 1};
        segs.s[nseg++] = ProofSeg{W.d_chal + CH_POW, nullptr, (size_t)CH_WORDS, 0, L.pow_off, 1u, 0};  // the trailer: k_pi_hash
        LAUNCH(W.lane, "proof_segments", k_proof_segments, dim3(2, B, nseg), dim3(256), 0, segs);
    }
    LAUNCH(W.lane, "finish", k_finish, g1(C->pbytes, 256, B), dim3(256), 0, W.d_status, d_status_out, d_proofs, C->pbytes, B);
    return 0;
}

// The leased workspaces (pool.h) have a stream of their own, and those whose calls may return before their kernels have run an
// event `done` behind the last of them.  After a failed call the lease drains the workspace; a destructor first waits for the
// last user, then the members free themselves.
static void ws_drain(hipStream_t own, bool has_caller = false, void* caller = nullptr) {
    if (has_caller) (void)hipStreamSynchronize((hipStream_t)caller);
    if (own) (void)hipStreamSynchronize(own);
}
// Host-path staging: device buffers, pinned host mirrors and a stream, kept across p2_prove_batch calls (they only grow).
// A caller leases one set for the duration of its call; concurrent callers on one handle each get their own.
struct Staging {
    NoKey key;
    Staged<u64> vals, out;  // out: witness outputs (p2_prove_batch_outputs); never allocated by p2_prove_batch
    Staged<uint8_t> proofs;
    Staged<int> stat;
    Stream stream;  // (after the memory, as in every workspace: the stream goes first)
    void drain(bool has_caller, void* caller) { ws_drain(stream, has_caller, caller); }
    ~Staging() { ws_drain(stream); }
    bool fit(size_t vals_bytes, size_t proofs_bytes, size_t batch, size_t out_bytes) {
        return (stream || stream.create(hipStreamNonBlocking) == hipSuccess) && vals.grow(vals_bytes) && proofs.grow(proofs_bytes) &&
               stat.grow(batch * sizeof(int)) && out.grow(out_bytes);
    }
};

// Every entry point that allocates (std::vector, std::map, std::thread) runs behind this guard: an exception becomes
// P2_ERR_* + p2_last_error(), never std::terminate -- also on the worker threads of p2_prove_batch_multi.
template <class F>
static int guarded_rc(F&& f) {
    try {
        return f();
    } catch (std::bad_alloc&) {
        return set_error("out of host memory"), P2_ERR_HIP;
    } catch (std::exception& e) {
        return set_error(e.what()), P2_ERR_INVALID;
    } catch (...) {
        return set_error("unknown exception"), P2_ERR_INVALID;
    }
}
// ---------------------------------------------------------------------------------- batched verification and compressed proofs
// (kernels_verify.h, kernels_compress.h): the layout tables built at load, the leased workspaces and one driver for the four operations
// Per-call workspace: device buffers for one chunk of proofs, a stream for the host path and an event that orders the next
// user of the workspace behind the last kernel that read it (the device path returns before its kernels have run).
struct VerifyWs {
    size_t key = 0, chunk = 0;  // the "verify_chunk" option it was made under = the proofs it holds
    DevBuf<u64> d_words, d_chal, d_vq, d_vd, d_pi_hash;
    DevBuf<u32> d_flags, d_qfail;
    DevBuf<uint8_t> d_proofs;
    DevBuf<int> d_status;
    PinBuf<int> h_status;
    // compressed proofs, allocated by their first use (cmp_ensure); never by plain verification
    DevBuf<CmpPlan> d_plan;
    DevBuf<uint8_t> d_cout;
    DevBuf<u32> d_len;
    PinBuf<u32> h_len;
    Stream stream;
    Event done;
    void drain(bool has_caller, void* caller) { ws_drain(stream, has_caller, caller); }
    ~VerifyWs() { if (done) (void)hipEventSynchronize(done); }
};
struct VdArg {
    u64 w[4 * 16 + 4];
};
__global__ void k_vfy_set_vd(VdArg v, u64* out, u32 count) {
    if (threadIdx.x < count) out[threadIdx.x] = v.w[threadIdx.x];
}

// Layout tables of the proof (the reader of verifier.h with every count taken from the circuit) and the host-side checks of
// what the verifier kernels assume.  Called once from p2_circuit_load.
static int verify_setup(p2_circuit* C) {
    const Circuit& c = C->c;
    const u32 NC = c.cfg.num_challenges, R = c.cfg.num_routed_wires, NW = c.cfg.num_wires, qdf = c.cfg.quotient_degree_factor;
    const u32 nlp = c.num_lookup_polys(), npp = c.num_partial_products(), zc = c.num_zs_cols(), lde_bits = C->lde_bits;
    // preconditions of k_vfy_vanishing / k_vfy_queries: fixed shapes they index with (cf. the host verifier's fixed arrays)
    std::string why;
    if (NC != 2) why = "num_challenges != 2";
    else if (R != 80 || NW != 135) why = "the lookup, arithmetic and Poseidon terms need 80 routed wires of 135";
    else if (qdf != 8 || c.cfg.num_constants != 2) why = "quotient_degree_factor / num_constants differ from standard_recursion_config";
    else if (c.cfg.cap_height != 4) why = "cap_height != 4";
    else if (c.k_is.size() != R) why = "k_is shape";
    else if (c.num_gate_constraints > VFY_MAX_GC || c.gates.size() > p2::MAX_GATE_TYPES || c.luts.size() > p2::MAX_LUTS) why = "gate / lookup table count";
    else if (c.cfg.num_query_rounds > CH_WORDS - CH_QUERY || C->dom.arities.size() > VFY_MAX_ROUNDS) why = "query rounds / FRI rounds";
    else if (c.cfg.pow_bits == 0 || c.cfg.pow_bits > 32) why = "pow_bits";
    else if (C->pbytes >= (size_t)UINT32_MAX) why = "proof too large";
    for (u32 ab : C->dom.arities)
        if (ab != VFY_ARITY_BITS) why = "FRI arity other than 16";
    if (!why.empty()) {
        C->vfy_error = "p2_verify_batch does not support this circuit: " + why;
        return 0;
    }
    // the unpacked words and the count bytes, in the order of the layout
    const ProofLayout& L = C->layout;
    std::vector<u32> woff, coff, obs;
    std::vector<uint8_t> cexp;
    auto words = [&](size_t at, size_t k) {
        u32 first = (u32)woff.size();
        for (size_t i = 0; i < k; i++) woff.push_back((u32)(at + 8 * i));
        return first;
    };
    VerifyArgs& a = C->vfy_args;
    a.cap_words = (u32)(L.cap_bytes / 8);
    words(L.caps_off[0], 3 * a.cap_words);
    u32 open_word[OG_GROUPS];
    for (u32 k = 0; k < OG_GROUPS; k++) open_word[k] = words(L.open[k].off, 2 * L.open[k].len);
    a.o_const = open_word[OG_CONSTANTS], a.o_sig = open_word[OG_SIGMAS], a.o_wires = open_word[OG_WIRES];
    a.o_zs = open_word[OG_ZS], a.o_zsn = open_word[OG_ZS_NEXT], a.o_lk = open_word[OG_LOOKUP_ZS], a.o_lkn = open_word[OG_LOOKUP_ZS_NEXT];
    a.o_pp = open_word[OG_PARTIAL_PRODUCTS], a.o_quot = open_word[OG_QUOTIENT];
    a.fri_caps_off = words(L.fri_caps_off, L.step.size() * a.cap_words);
    a.init_depth = L.init[0].depth;
    a.q_off = (u32)woff.size();
    for (u32 q = 0; q < L.num_queries; q++) {
        const size_t at = L.queries_off + q * L.query_bytes;
        const u32 base = (u32)woff.size();
        auto path = [&](const ProofLayout::Path& p, u32& eval_off, u32& sib_off) {
            eval_off = words(at + p.leaf_off, p.width) - base;
            coff.push_back((u32)(at + p.cnt_off));
            cexp.push_back((uint8_t)p.depth);
            sib_off = words(at + p.sib_off, 4 * p.depth) - base;
        };
        for (int o = 0; o < 4; o++) {
            path(L.init[o], a.init_eval_off[o], a.init_sib_off[o]);
            a.init_width[o] = L.init[o].width;
        }
        for (u32 k = 0; k < L.step.size(); k++) {
            path(L.step[k], a.step_eval_off[k], a.step_sib_off[k]);
            a.step_depth[k] = L.step[k].depth;
        }
        a.q_stride = (u32)woff.size() - base;
    }
    a.final_len = L.final_len;
    a.final_off = words(L.final_off, 2 * L.final_len);
    a.pow_off = words(L.pow_off, 1);
    a.num_pi = L.num_pi;
    if (a.num_pi) {
        a.pi_cnt_byte = (u32)L.pi_cnt_off;  // the count word: compared with num_pi by k_vfy_unpack, not unpacked
        a.pi_off = words(L.pi_off, a.num_pi);
    }
    // the opening batches in the order they are observed and reduced
    for (OpenGroup g : OPEN_OBSERVED)
        for (u32 i = 0; i < L.open[g].len; i++) obs.push_back(open_word[g] + 2 * i);
    a.n_b0 = L.set.n_b0;
    a.n_b1 = L.set.n_b1;
    a.W = (u32)woff.size();
    a.n_cnt = (u32)coff.size();
    if (upload(C->allocs, (u32**)&a.word_off, woff.data(), woff.size()) || upload(C->allocs, (u32**)&a.cnt_off, coff.data(), coff.size()) ||
        upload(C->allocs, (uint8_t**)&a.cnt_exp, cexp.data(), cexp.size()) || upload(C->allocs, (u32**)&a.obs_map, obs.data(), obs.size()))
        return P2_ERR_HIP;
    if (c.cfg.hasher == HASHER_KECCAK) {
        std::vector<u32> hidx;
        for (u32 i = 0; i < 3 * a.cap_words; i += 4) hidx.push_back(i);
        for (u32 i = 0; i < L.step.size() * a.cap_words; i += 4) hidx.push_back(a.fri_caps_off + i);
        C->kc_cap_hashes = (u32)hidx.size();
        for (u32 q = 0; q < L.num_queries; q++) {
            const u32 base = a.q_off + q * a.q_stride;
            for (int o = 0; o < 4; o++)
                for (u32 l = 0; l < a.init_depth; l++) hidx.push_back(base + a.init_sib_off[o] + 4 * l);
            for (u32 k = 0; k < L.step.size(); k++)
                for (u32 l = 0; l < a.step_depth[k]; l++) hidx.push_back(base + a.step_sib_off[k] + 4 * l);
        }
        C->kc_hashes = (u32)hidx.size();
        if (upload(C->allocs, &C->d_kc_hash_idx, hidx.data(), hidx.size())) return P2_ERR_HIP;
    }
    a.proof_bytes = C->pbytes;
    a.degree_bits = c.degree_bits;
    a.lde_bits = lde_bits;
    a.cap_height = c.cfg.cap_height;
    a.pow_bits = c.cfg.pow_bits;
    a.num_queries = c.cfg.num_query_rounds;
    a.num_rounds = (u32)C->dom.arities.size();
    a.has_lookup = nlp ? 1 : 0;
    a.R = R, a.num_wires = NW, a.NC = NC, a.npp = npp, a.qdf = qdf, a.nlp = nlp, a.nsldc = c.num_sldc_polys();
    a.lut_deg = nlp ? c.lut_degree() : 0;
    a.nsel = c.num_selectors(), a.nls = c.num_lookup_selectors, a.ngc = c.num_gate_constraints, a.nzpp = c.num_zs_pp(), a.zc = zc;
    a.num_gates = (u32)c.gates.size();
    fill_gate_table(c, a);
    a.num_luts = (u32)c.luts.size();
    a.lut_pairs = C->d_lut_pairs;
    a.lut_offsets = C->d_lut_offsets;
    a.k_is = C->d_k_is;
    // chunk: the unpacked words and the staged proofs of a chunk within ~256 MiB, at most 512 proofs
    const size_t per_proof = 8 * (size_t)a.W + C->pbytes + 8 * (CH_WORDS + VQ_WORDS) + 16;
    C->vfy.set_key(std::max<size_t>(1, std::min<size_t>(512, ((size_t)256 << 20) / per_proof)));
    if (const char* e = getenv("P2AES_VERIFY_CHUNK")) C->vfy.set_key((size_t)std::min(4096, std::max(1, atoi(e))));
    return 0;
}

// The compressed layout's per-circuit table: where each word of the full layout comes from.
static int cmp_setup(p2_circuit* C) {
    if (!C->vfy_error.empty()) return 0;
    const Circuit& c = C->c;
    const VerifyArgs& a = C->vfy_args;
    if (c.cfg.num_query_rounds > CMP_MAXQ || a.init_depth > 31) {
        C->vfy_error = "compressed proofs: more than 32 queries or an initial tree deeper than 31 levels";
        return 0;
    }
    std::vector<u32> wmap(a.W, cmp_code(CW_PREFIX, 0, 0, 0));
    for (u32 i = a.final_off; i < a.W; i++) wmap[i] = cmp_code(CW_TAIL, 0, 0, 0);
    for (u32 q = 0; q < c.cfg.num_query_rounds; q++) {
        const u32 base = a.q_off + q * a.q_stride;
        for (u32 o = 0; o < 4; o++) {
            for (u32 e = 0; e < a.init_width[o]; e++) wmap[base + a.init_eval_off[o] + e] = cmp_code(CW_LEAF, q, o, e);
            for (u32 e = 0; e < 4 * a.init_depth; e++) wmap[base + a.init_sib_off[o] + e] = cmp_code(CW_SIB, q, o, e);
        }
        for (u32 r = 0; r < a.num_rounds; r++) {
            for (u32 e = 0; e < 2 * VFY_ARITY; e++) wmap[base + a.step_eval_off[r] + e] = cmp_code(CW_EVAL, q, 4 + r, e);
            for (u32 e = 0; e < 4 * a.step_depth[r]; e++) wmap[base + a.step_sib_off[r] + e] = cmp_code(CW_SIB, q, 4 + r, e);
        }
    }
    return upload(C->allocs, &C->d_cmp_wmap, wmap.data(), wmap.size());
}

static std::unique_ptr<VerifyWs> verify_make(const p2_circuit* C, size_t chunk) {
    auto W = std::make_unique<VerifyWs>();
    const VerifyArgs& a = C->vfy_args;
    W->key = W->chunk = chunk;
    const bool ok = W->stream.create(hipStreamNonBlocking) == hipSuccess && W->done.create(hipEventDisableTiming) == hipSuccess &&
                    W->d_words.alloc(chunk * a.W) == hipSuccess && W->d_chal.alloc(chunk * CH_WORDS) == hipSuccess && W->d_vq.alloc(chunk * VQ_WORDS) == hipSuccess &&
                    W->d_vd.alloc(sizeof(VdArg) / 8) == hipSuccess && W->d_pi_hash.alloc(chunk * 4) == hipSuccess && W->d_flags.alloc(chunk) == hipSuccess &&
                    W->d_qfail.alloc(chunk) == hipSuccess && W->d_proofs.alloc(chunk * C->pbytes) == hipSuccess && W->d_status.alloc(chunk) == hipSuccess &&
                    W->h_status.alloc(chunk) == hipSuccess;
    if (!ok) return set_error("verification workspace could not be allocated"), nullptr;
    return W;
}
struct VerifyLease : Lease<VerifyWs> {
    explicit VerifyLease(p2_circuit* C) : Lease(C->vfy, [C](size_t chunk) { return verify_make(C, chunk); }) {}
};

// ---- the driver: verify, compress, decompress, verify compressed
enum ProofOp { OP_VERIFY, OP_COMPRESS, OP_DECOMPRESS, OP_VERIFY_COMPRESSED };
static int cmp_ensure(p2_circuit* C, VerifyWs* W) {
    if (W->d_plan) return P2_OK;
    const size_t n = W->chunk;
    if (W->d_plan.alloc(n) != hipSuccess || W->d_cout.alloc(n * C->pbytes) != hipSuccess || W->d_len.alloc(n) != hipSuccess || W->h_len.alloc(n) != hipSuccess)
        return set_error("compression workspace could not be allocated"), P2_ERR_HIP;
    return P2_OK;
}

// Enqueues one operation on `batch` proofs on `st`, a chunk of the workspace at a time.  host: every buffer is host memory
// (staged through the workspace, and the call waits for the results); otherwise all are device memory and the call returns
// once everything is enqueued.  in: full proofs (verify, compress) or compressed ones at the same stride with `lengths`;
// out: compressed proofs (compress, with lengths_out) or full ones (decompress).
static int proof_run(p2_circuit* C, VerifyWs* W, ProofOp op, size_t batch, const uint8_t* in, const u32* lengths, uint8_t* out, u32* lengths_out,
                     const VdArg& vd, int* status, hipStream_t st, bool host) {
    const ProofLayout& L = C->layout;
    const size_t pb = L.bytes;
    const bool full_in = op == OP_VERIFY || op == OP_COMPRESS, verdict = op == OP_VERIFY || op == OP_VERIFY_COMPRESSED;
    const bool keccak = C->c.cfg.hasher == HASHER_KECCAK;
    HIPCHECK(hipStreamWaitEvent(st, W->done, 0));  // the workspace's previous user
    LAUNCH_ON(st, k_vfy_set_vd, dim3(1), dim3(128), vd, W->d_vd, C->vfy_args.cap_words + 4);
    for (size_t done = 0; done < batch; done += W->chunk) {
        const u32 B = (u32)std::min(W->chunk, batch - done);
        CmpArgs a{};
        a.v = C->vfy_args;
        VerifyArgs& v = a.v;
        v.batch = B;
        v.words = W->d_words;
        v.flags = W->d_flags;
        v.qfail = W->d_qfail;
        v.chal = W->d_chal;
        v.vq = W->d_vq;
        v.vd = W->d_vd;
        v.pi_hash = W->d_pi_hash;
        a.plan = W->d_plan;
        a.wmap = C->d_cmp_wmap;
        a.prefix = (u32)L.queries_off;
        a.tail = (u32)L.tail_bytes();
        for (int o = 0; o < 4; o++) a.cols[o] = L.init[o].width;
        a.from_chal = op == OP_COMPRESS;
        if (host) {
            HIPCHECK(hipMemcpyAsync(W->d_proofs, in + done * pb, B * pb, hipMemcpyHostToDevice, st));
            if (lengths) HIPCHECK(hipMemcpyAsync(W->d_len, lengths + done, B * 4, hipMemcpyHostToDevice, st));
            v.status = W->d_status;
            a.cout = W->d_cout;
            a.lengths = W->d_len;
            a.lengths_out = W->d_len;
            v.proofs = a.cproofs = W->d_proofs;
        } else {
            v.status = status + done;
            a.cout = out ? out + done * pb : nullptr;
            a.lengths = lengths ? lengths + done : nullptr;
            a.lengths_out = lengths_out ? lengths_out + done : nullptr;
            v.proofs = a.cproofs = in + done * pb;
        }
        HIPCHECK(hipMemsetAsync(W->d_flags, 0, (size_t)B * 4, st));
        HIPCHECK(hipMemsetAsync(W->d_qfail, 0xFF, (size_t)B * 4, st));
        const dim3 words_grid((v.W + 255) / 256, B), proofs_grid = g1(B, 64), transcript_grid = g1((size_t)B * 16, 64);
        if (full_in) {  // the words of a full proof and its challenges
            LAUNCH_ON(st, k_vfy_unpack, words_grid, dim3(256), v);
            if (keccak) LAUNCH_ON(st, k_kcv_range, g1(C->kc_hashes, 256, B), dim3(256), v, (const u32*)C->d_kc_hash_idx, C->kc_hashes);
            LAUNCH_ON(st, k_vfy_transcript, transcript_grid, dim3(64), v);
        } else {  // the same from a compressed proof: what it stores, then what its Merkle caps and fold checks imply
            LAUNCH_ON(st, k_cmp_plan, dim3(B), dim3(256), a);
            LAUNCH_ON(st, k_cmp_scatter, words_grid, dim3(256), a);
            // (the caps of the prefix; a proof without a layout keeps its SHAPE flag, which comes first.  Stored siblings: k_kcc_merkle)
            if (keccak) LAUNCH_ON(st, k_kcv_range, g1(C->kc_cap_hashes, 256, B), dim3(256), v, (const u32*)C->d_kc_hash_idx, C->kc_cap_hashes);
            LAUNCH_ON(st, k_vfy_transcript, transcript_grid, dim3(64), v);
            LAUNCH_ON(st, k_cmp_reductions, proofs_grid, dim3(64), a);
            LAUNCH_ON(st, k_cmp_infer, dim3(B), dim3(CMP_MAXQ), a);
            if (keccak) LAUNCH_ON(st, k_kcc_merkle, dim3(B, 4 + v.num_rounds), dim3(CMP_MAXQ), a);
            else LAUNCH_ON(st, k_cmp_merkle, dim3(B, 4 + v.num_rounds), dim3(CMP_MAXQ), a);
        }
        if (op == OP_COMPRESS) {
            LAUNCH_ON(st, k_cmp_plan, dim3(B), dim3(256), a);
            HIPCHECK(hipMemsetAsync(a.cout, 0, (size_t)B * pb, st));
            LAUNCH_ON(st, k_cmp_emit, words_grid, dim3(256), a);
            LAUNCH_ON(st, k_cmp_finish, proofs_grid, dim3(64), a);
        } else if (op == OP_DECOMPRESS) {
            LAUNCH_ON(st, k_cmp_finish, proofs_grid, dim3(64), a);
            LAUNCH_ON(st, k_cmp_pack, words_grid, dim3(256), a);
        } else {
            const u32 slots = 4 + v.num_rounds + 1;
            if (ecstep_gate_index(C->c) >= 0) LAUNCH_ON(st, k_vfy_ecvanishing, dim3(B), dim3(256), v);
            else LAUNCH_ON(st, k_vfy_vanishing, dim3(B), dim3(256), v);
            const dim3 queries_grid((u32)(((size_t)B * v.num_queries + 63) / 64), slots);
            if (keccak) LAUNCH_ON(st, k_kcv_queries, queries_grid, dim3(64), v);
            else LAUNCH_ON(st, k_vfy_queries, queries_grid, dim3(64), v);
            LAUNCH_ON(st, k_vfy_finish, proofs_grid, dim3(64), v, slots);
        }
        if (host) {
            HIPCHECK(hipMemcpyAsync(W->h_status, W->d_status, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
            if (op == OP_COMPRESS) HIPCHECK(hipMemcpyAsync(W->h_len, W->d_len, (size_t)B * 4, hipMemcpyDeviceToHost, st));
            if (!verdict) HIPCHECK(hipMemcpyAsync(out + done * pb, W->d_cout, (size_t)B * pb, hipMemcpyDeviceToHost, st));
            HIPCHECK(hipStreamSynchronize(st));
            memcpy(status + done, W->h_status, (size_t)B * sizeof(int));
            if (op == OP_COMPRESS) memcpy(lengths_out + done, W->h_len, (size_t)B * 4);
        }
    }
    HIPCHECK(hipEventRecord(W->done, st));
    return P2_OK;
}

static int proof_batch_impl(p2_circuit* C, ProofOp op, size_t batch, const uint8_t* in, const u32* lengths, const uint64_t* verifier_data, size_t vd_len,
                            uint8_t* out, u32* lengths_out, int* status, hipStream_t st, bool host) {
    static const char* names[4] = {"p2_verify_batch", "p2_compress_batch", "p2_decompress_batch", "p2_verify_compressed_batch"};
    const std::string name = names[op];
    const bool full_in = op == OP_VERIFY || op == OP_COMPRESS, verdict = op == OP_VERIFY || op == OP_VERIFY_COMPRESSED;
    if (!C) return set_error(name + ": null circuit handle"), P2_ERR_INVALID;
    const size_t vd_words = (size_t)C->vfy_args.cap_words + 4;
    if (verifier_data && vd_len != vd_words) return set_error("verifier_data must be cap || circuit_digest (" + std::to_string(vd_words) + " words)"), P2_ERR_INVALID;
    if (!C->vfy_error.empty()) return set_error(C->vfy_error), P2_ERR_INVALID;
    if (batch == 0) return P2_OK;
    if (!in || !status || (!verdict && !out) || (op == OP_COMPRESS && !lengths_out) || (!full_in && !lengths))
        return set_error(name + (op == OP_VERIFY ? ": null proofs or status" : ": null buffer")), P2_ERR_INVALID;
    if (host && !full_in)
        for (size_t i = 0; i < batch; i++)
            if (lengths[i] > C->pbytes)
                return set_error(name + ": length " + std::to_string(lengths[i]) + " of proof " + std::to_string(i) + " exceeds the stride " + std::to_string(C->pbytes)),
                       P2_ERR_INVALID;
    VdArg vd{};
    if (vd_words > sizeof(vd.w) / 8) return set_error("internal: verifier data larger than the kernel argument"), P2_ERR_INVALID;
    memcpy(vd.w, verifier_data ? verifier_data : C->verifier_data.data(), vd_words * 8);
    HIPCHECK(hipSetDevice(C->device));
    VerifyLease lease(C);
    VerifyWs* W = lease.ws.get();
    if (!W) return P2_ERR_HIP;
    if (!host) lease.on_stream(st);
    int rc = op == OP_VERIFY ? P2_OK : cmp_ensure(C, W);  // plain verification never allocates the compression buffers
    if (rc == P2_OK) rc = proof_run(C, W, op, batch, in, lengths, out, lengths_out, vd, status, host ? (hipStream_t)W->stream : st, host);
    lease.failed = rc != P2_OK;
    return rc;
}

// p2_gpu_vanishing_flags: the vanishing kernel of OP_VERIFY on the caller's openings, challenges and public-input hashes.  Per
// chunk: k_vfy_unpack, the challenge rows and hashes copied to where k_vfy_transcript leaves them (the rest of a row zero: the
// opening reductions of the kernel's second wave read fri_alpha and write vq, which nothing here reads), the kernel, the flags.
static int vanishing_flags_run(p2_circuit* C, VerifyWs* W, size_t batch, const uint8_t* buffers, const uint64_t* challenges, const uint64_t* pi_hashes,
                               uint32_t* flags) {
    const size_t pb = C->layout.bytes;
    hipStream_t st = W->stream;
    HIPCHECK(hipStreamWaitEvent(st, W->done, 0));  // the workspace's previous user
    std::vector<u64> rows;
    for (size_t done = 0; done < batch; done += W->chunk) {
        const u32 B = (u32)std::min(W->chunk, batch - done);
        VerifyArgs v = C->vfy_args;
        v.batch = B;
        v.words = W->d_words;
        v.flags = W->d_flags;
        v.qfail = W->d_qfail;
        v.chal = W->d_chal;
        v.vq = W->d_vq;
        v.vd = W->d_vd;
        v.pi_hash = W->d_pi_hash;
        v.status = W->d_status;
        v.proofs = W->d_proofs;
        rows.assign((size_t)B * CH_WORDS, 0);
        for (u32 p = 0; p < B; p++) memcpy(&rows[(size_t)p * CH_WORDS], challenges + (done + p) * 16, 16 * sizeof(u64));  // CH_BETAS .. CH_ZETA
        HIPCHECK(hipMemcpyAsync(W->d_proofs, buffers + done * pb, B * pb, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(W->d_chal, rows.data(), rows.size() * sizeof(u64), hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(W->d_pi_hash, pi_hashes + done * 4, (size_t)B * 4 * sizeof(u64), hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemsetAsync(W->d_flags, 0, (size_t)B * 4, st));
        LAUNCH_ON(st, k_vfy_unpack, dim3((v.W + 255) / 256, B), dim3(256), v);
        if (ecstep_gate_index(C->c) >= 0) LAUNCH_ON(st, k_vfy_ecvanishing, dim3(B), dim3(256), v);
        else LAUNCH_ON(st, k_vfy_vanishing, dim3(B), dim3(256), v);
        HIPCHECK(hipMemcpyAsync(flags + done, W->d_flags, (size_t)B * 4, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipStreamSynchronize(st));  // `rows` is refilled by the next chunk
        for (u32 p = 0; p < B; p++) flags[done + p] &= (u32)(VF_ZETA | VF_VANISH);
    }
    HIPCHECK(hipEventRecord(W->done, st));
    return P2_OK;
}
static int vanishing_flags_impl(p2_circuit* C, size_t batch, const uint8_t* buffers, const uint64_t* challenges, const uint64_t* pi_hashes, uint32_t* flags) {
    if (!C) return set_error("p2_gpu_vanishing_flags: null circuit handle"), P2_ERR_INVALID;
    if (!C->vfy_error.empty()) return set_error(C->vfy_error), P2_ERR_INVALID;
    if (batch == 0) return P2_OK;
    if (!buffers || !challenges || !pi_hashes || !flags) return set_error("p2_gpu_vanishing_flags: null buffer"), P2_ERR_INVALID;
    static_assert(CH_BETAS == 0 && CH_GAMMAS == 2 && CH_DELTAS == 4 && CH_ALPHAS == 12 && CH_ZETA == 14, "the caller's 16 words are the head of a challenge row");
    for (size_t i = 0; i < batch * 16; i++)
        if (challenges[i] >= gl::P) return set_error("p2_gpu_vanishing_flags: non-canonical challenge"), P2_ERR_INVALID;
    for (size_t i = 0; i < batch * 4; i++)
        if (pi_hashes[i] >= gl::P) return set_error("p2_gpu_vanishing_flags: non-canonical public-inputs hash"), P2_ERR_INVALID;
    HIPCHECK(hipSetDevice(C->device));
    VerifyLease lease(C);
    if (!lease) return P2_ERR_HIP;
    const int rc = vanishing_flags_run(C, lease.ws.get(), batch, buffers, challenges, pi_hashes, flags);
    lease.failed = rc != P2_OK;
    return rc;
}

// ---------------------------------------------------------------------------------- witness-only runs, fault diagnosis
// (kernels_witness_io.h)  A lean workspace, leased per call like the verification ones: per witness the slot values, the
// multiplicity counters and the PoseidonGate advice block that k_witness writes -- megabytes where a proving workspace holds
// the oracles of DESIGN.md section 4.  The witness-only path launches the k_witness instantiations the prover launches and
// does not join the prover's ev_witness chain.
struct WitnessWs {
    size_t key = 0, chunk = 0;  // the "witness_chunk" option it was made under; the witnesses it holds (that, capped by free HBM)
    DevBuf<u64> d_values, d_advice;
    DevBuf<u32> d_mult;
    // the target lists as last uploaded (re-uploaded only when a call brings other ones), grown on demand
    DevBuf<u32> d_input_slots, d_out_slots;
    std::vector<u32> h_input_slots, h_out_slots;
    // host forms: staging of inputs, outputs and statuses, grown on demand
    Staged<u64> in, out;
    Staged<int> status;
    // p2_witness_explain
    DevBuf<u64> d_ex_in;
    DevBuf<u32> d_prev;
    DevBuf<unsigned long long> d_keys;  // the two reduction keys, then the run's status word
    DevBuf<p2_witness_fault> d_fault;
    PinBuf<p2_witness_fault> h_fault;  // and the status word behind it
    Stream stream;                     // the host forms' stream
    Event done;                        // behind the last kernel that used the workspace
    void drain(bool has_caller, void* caller) { ws_drain(stream, has_caller, caller); }
    ~WitnessWs() { if (done) (void)hipEventSynchronize(done); }
};
// the tables of the fault check on the device (witness_check.h), uploaded by the first p2_witness_explain of a handle: the
// ops in blob order are as large as the scheduled copy, so a handle that never explains does not carry them
struct ExplainTables {
    Allocs mem;
    Op* d_ops = nullptr;
    u32 *d_free_slots = nullptr, *d_slot_row = nullptr;
    u64* d_slot_target = nullptr;
    u32 n_free = 0;
};
// device bytes one witness takes in a WitnessWs
static size_t witness_ws_bytes(const p2_circuit* C) {
    return 8 * (size_t)C->c.num_slots + 4 * std::max<size_t>(C->total_lut_entries, 1) + 8 * 55 * std::max<size_t>(C->c.poseidon_rows.size(), 1);
}
static std::unique_ptr<WitnessWs> witness_make(const p2_circuit* C, size_t chunk) {
    auto W = std::make_unique<WitnessWs>();
    W->key = chunk;
    // the same cap as the prover's: a workspace takes at most 80 % of the HBM that is free
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) chunk = std::max<size_t>(1, std::min(chunk, (size_t)(0.8 * (double)free_b) / witness_ws_bytes(C)));
    W->chunk = chunk;
    const bool ok = W->stream.create(hipStreamNonBlocking) == hipSuccess && W->done.create(hipEventDisableTiming) == hipSuccess &&
                    W->d_values.alloc(chunk * (size_t)C->c.num_slots) == hipSuccess && W->d_mult.alloc(chunk * std::max<size_t>(C->total_lut_entries, 1)) == hipSuccess &&
                    W->d_advice.alloc(chunk * 55 * std::max<size_t>(C->c.poseidon_rows.size(), 1)) == hipSuccess;
    if (!ok) return set_error("witness workspace could not be allocated"), nullptr;
    return W;
}
struct WitnessLease : Lease<WitnessWs> {
    explicit WitnessLease(p2_circuit* C) : Lease(C->wit, [C](size_t chunk) { return witness_make(C, chunk); }) {}
};
// targets -> slots; `what` names the list in the error ("input" / "output")
static int target_slots(const p2_circuit* C, const p2_target* targets, size_t n, const char* what, std::vector<u32>& slots) {
    slots.resize(n);
    for (size_t i = 0; i < n; i++) {
        const int32_t slot = target_slot(C->c, targets[i]);
        if (slot < 0) return set_error(std::string(what) + " target is not a target of this circuit"), P2_ERR_INVALID;
        slots[i] = (u32)slot;
    }
    return P2_OK;
}
// A slot list of a workspace: uploaded only when it differs from the one the workspace holds, and then behind everything that
// still reads the old one.
static int witness_put_slots(WitnessWs* W, DevBuf<u32>& d, std::vector<u32>& held, const std::vector<u32>& slots) {
    if (held == slots && d) return P2_OK;
    HIPCHECK(hipEventSynchronize(W->done));
    if (!d.grow(std::max<size_t>(slots.size(), 1))) return set_error("witness workspace could not be allocated"), P2_ERR_HIP;
    if (!slots.empty()) HIPCHECK(hipMemcpy(d, slots.data(), slots.size() * 4, hipMemcpyHostToDevice));
    held = slots;
    return P2_OK;
}
static int launch_witness(p2_circuit* C, hipStream_t st, u32 B, const WitnessArgs& a) {
    const bool pos = !C->c.poseidon_rows.empty();
    const bool ec = ecstep_gate_index(C->c) >= 0;
    if (!ec && !pos && C->witness_chains) LAUNCH_ON(st, (k_witness<false, true>), dim3(B), dim3(512), a);
    if (!ec && !pos && !C->witness_chains) LAUNCH_ON(st, (k_witness<false, false>), dim3(B), dim3(512), a);
    if (!ec && pos && C->witness_chains) LAUNCH_ON(st, (k_witness<true, true>), dim3(B), dim3(512), a);
    if (!ec && pos && !C->witness_chains) LAUNCH_ON(st, (k_witness<true, false>), dim3(B), dim3(512), a);
    if (ec && !pos && C->witness_chains) LAUNCH_ON(st, (k_ecwitness<false, true>), dim3(B), dim3(512), a);
    if (ec && !pos && !C->witness_chains) LAUNCH_ON(st, (k_ecwitness<false, false>), dim3(B), dim3(512), a);
    if (ec && pos && C->witness_chains) LAUNCH_ON(st, (k_ecwitness<true, true>), dim3(B), dim3(512), a);
    if (ec && pos && !C->witness_chains) LAUNCH_ON(st, (k_ecwitness<true, false>), dim3(B), dim3(512), a);
    return P2_OK;
}
// Enqueues witness generation of `batch` witnesses on `st`, a chunk of the workspace at a time: k_witness, the wired-slot
// rule, the gather.  Every pointer is device memory; the slot lists are in the workspace.
static int witness_run(p2_circuit* C, WitnessWs* W, size_t batch, u32 n_inputs, const u64* d_values, u32 n_out, u64* d_out, int* d_status, hipStream_t st) {
    const Circuit& c = C->c;
    HIPCHECK(hipStreamWaitEvent(st, W->done, 0));  // the workspace's previous user
    for (size_t done = 0; done < batch; done += W->chunk) {
        const u32 B = (u32)std::min(W->chunk, batch - done);
        HIPCHECK(hipMemsetAsync(W->d_mult, 0, (size_t)B * std::max<size_t>(C->total_lut_entries, 1) * 4, st));
        WitnessArgs a{};
        a.ops = C->d_ops, a.levels = C->d_wlevels, a.chains = C->d_wchains;
        a.num_levels = C->witness_levels, a.num_slots = c.num_slots, a.n_inputs = n_inputs;
        a.input_slots = W->d_input_slots, a.input_values = d_values + done * n_inputs;
        a.values = W->d_values, a.lut_ent = C->d_lut_ent, a.mult = W->d_mult, a.total_lut_entries = C->total_lut_entries;
        a.status = d_status + done, a.wire_slot = C->d_wire_slot, a.advice = W->d_advice;
        a.n = (u32)C->n, a.num_poseidon_rows = (u32)c.poseidon_rows.size();
        if (int rc = launch_witness(C, st, B, a)) return rc;
        if (C->n_wired)
            LAUNCH_ON(st, k_witness_wired_unset, dim3((u32)std::min<size_t>((C->n_wired + 255) / 256, 64), B), dim3(256), W->d_values, c.num_slots, C->d_wired_slots,
                      C->n_wired, d_status + done);
        if (n_out) LAUNCH_ON(st, k_gather_slots, g1(n_out, 256, B), dim3(256), W->d_values, c.num_slots, W->d_out_slots, n_out, d_out + done * n_out);
    }
    HIPCHECK(hipEventRecord(W->done, st));
    return P2_OK;
}
static int witness_null_handle(const char* name) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return set_error("no HIP device available: witness generation on a handle has no CPU fallback"), P2_ERR_NO_DEVICE;
    return set_error(std::string(name) + ": null circuit handle"), P2_ERR_INVALID;
}
static int witness_batch_device_impl(p2_circuit* C, size_t batch, const p2_target* targets, size_t n_targets, const uint64_t* d_values, const p2_target* out_targets,
                                     size_t n_out, uint64_t* d_out, int* d_status, void* stream) {
    if (!C) return witness_null_handle("p2_witness_batch_device");
    if ((n_targets && !targets) || (n_out && (!out_targets || !d_out)) || (batch && (!d_status || (n_targets && !d_values))))
        return set_error("p2_witness_batch_device: null buffer"), P2_ERR_INVALID;
    std::vector<u32> in_slots, out_slots;
    if (int rc = target_slots(C, targets, n_targets, "input", in_slots)) return rc;
    if (int rc = target_slots(C, out_targets, n_out, "output", out_slots)) return rc;
    if (batch == 0) return P2_OK;
    HIPCHECK(hipSetDevice(C->device));
    WitnessLease lease(C);
    WitnessWs* W = lease.ws.get();
    if (!W) return P2_ERR_HIP;
    lease.on_stream(stream);
    if (int rc = witness_put_slots(W, W->d_input_slots, W->h_input_slots, in_slots)) return rc;
    if (int rc = witness_put_slots(W, W->d_out_slots, W->h_out_slots, out_slots)) return rc;
    if (int rc = witness_run(C, W, batch, (u32)n_targets, d_values, (u32)n_out, d_out, d_status, (hipStream_t)stream)) return rc;
    lease.failed = false;
    return P2_OK;
}

// One layout of a batch of assignments for the device: [batch][nt] values on a shared target list.  Fast path: every
// PartialWitness assigns the same target list in the same order.  Otherwise the batch is put on the union of the targets, a
// witness that does not assign a target gets the "absent" marker (2^64-1, not a field element), and a witness that assigns
// one target two different values fails on the host like set_target does.  Either way a value that is not a canonical field
// element fails that witness here, on the host (host_status).  zero_rejected: such a value goes to the device as 0 (the
// prover: the witness is rejected whatever runs); otherwise it goes as it is and k_witness skips it.
struct PackedInputs {
    size_t nt = 0;
    const p2_target* targets = nullptr;
    std::vector<u64> union_targets;
    std::map<u64, size_t> col;
    bool same = true;
    std::vector<int> host_status;
    size_t nvals(size_t batch) const { return batch * std::max<size_t>(nt, 1); }
    void plan(size_t batch, const p2_assignment* inputs) {
        nt = inputs[0].count;
        for (size_t i = 1; i < batch && same; i++) same = inputs[i].count == nt && memcmp(inputs[i].targets, inputs[0].targets, nt * 8) == 0;
        host_status.assign(batch, 0);
        targets = inputs[0].targets;
        if (!same) {
            for (size_t i = 0; i < batch; i++)
                for (size_t k = 0; k < inputs[i].count; k++)
                    if (col.emplace(inputs[i].targets[k], union_targets.size()).second) union_targets.push_back(inputs[i].targets[k]);
            nt = union_targets.size();
            targets = union_targets.data();
        }
    }
    void fill(size_t batch, const p2_assignment* inputs, u64* hv, bool zero_rejected) {
        if (same) {
            for (size_t i = 0; i < batch; i++)
                for (size_t k = 0; k < nt; k++) {
                    u64 v = inputs[i].values[k];
                    if (v >= gl::P) {
                        host_status[i] = P2_PROOF_WITNESS_CONFLICT;
                        if (zero_rejected) v = 0;
                    }
                    hv[i * nt + k] = v;
                }
        } else {
            std::fill(hv, hv + nvals(batch), ~0ull);
            for (size_t i = 0; i < batch; i++)
                for (size_t k = 0; k < inputs[i].count; k++) {
                    u64& cell = hv[i * nt + col[inputs[i].targets[k]]];
                    u64 v = inputs[i].values[k];
                    const bool rejected = v >= gl::P || (cell != ~0ull && cell != v);
                    if (rejected) host_status[i] = P2_PROOF_WITNESS_CONFLICT;
                    if (rejected && zero_rejected) v = 0;
                    if (zero_rejected || cell == ~0ull) cell = v;  // (witness-only: the first value of a target stays, as in the slot)
                }
        }
    }
};

static int witness_batch_impl(p2_circuit* C, size_t batch, const p2_assignment* inputs, const p2_target* out_targets, size_t n_out, uint64_t* out_values, int* status) {
    if (!C) return witness_null_handle("p2_witness_batch");
    if (n_out && (!out_targets || (batch && !out_values))) return set_error("p2_witness_batch: null output buffer"), P2_ERR_INVALID;
    std::vector<u32> in_slots, out_slots;
    if (int rc = target_slots(C, out_targets, n_out, "output", out_slots)) return rc;
    if (batch == 0) return P2_OK;
    if (!inputs || !status) return set_error("p2_witness_batch: null inputs or status"), P2_ERR_INVALID;
    for (size_t i = 0; i < batch; i++)
        if (inputs[i].count && (!inputs[i].targets || !inputs[i].values)) return set_error("p2_witness_batch: null assignment"), P2_ERR_INVALID;
    PackedInputs pk;
    pk.plan(batch, inputs);
    if (int rc = target_slots(C, pk.targets, pk.nt, "input", in_slots)) return rc;
    HIPCHECK(hipSetDevice(C->device));
    WitnessLease lease(C);
    WitnessWs* W = lease.ws.get();
    if (!W) return P2_ERR_HIP;
    const size_t nvals = pk.nvals(batch), nouts = batch * std::max<size_t>(n_out, 1);
    HIPCHECK(hipEventSynchronize(W->done));  // the staging buffers may be replaced below
    if (!W->in.grow(nvals * 8) || !W->out.grow(nouts * 8) || !W->status.grow(batch * sizeof(int)))
        return set_error("staging buffers for p2_witness_batch could not be allocated"), P2_ERR_HIP;
    pk.fill(batch, inputs, W->in.h, false);
    if (int rc = witness_put_slots(W, W->d_input_slots, W->h_input_slots, in_slots)) return rc;
    if (int rc = witness_put_slots(W, W->d_out_slots, W->h_out_slots, out_slots)) return rc;
    HIPCHECK(hipMemcpyAsync(W->in.d, W->in.h, nvals * 8, hipMemcpyHostToDevice, W->stream));
    if (int rc = witness_run(C, W, batch, (u32)pk.nt, W->in.d, (u32)n_out, W->out.d, W->status.d, W->stream)) return rc;
    if (n_out) HIPCHECK(hipMemcpyAsync(W->out.h, W->out.d, batch * n_out * 8, hipMemcpyDeviceToHost, W->stream));
    HIPCHECK(hipMemcpyAsync(W->status.h, W->status.d, batch * sizeof(int), hipMemcpyDeviceToHost, W->stream));
    HIPCHECK(hipStreamSynchronize(W->stream));
    if (n_out) memcpy(out_values, W->out.h, batch * n_out * 8);
    for (size_t i = 0; i < batch; i++) status[i] = pk.host_status[i] ? pk.host_status[i] : W->status.h[i];
    lease.failed = false;
    return P2_OK;
}

static int explain_tables(p2_circuit* C) {
    std::lock_guard<std::mutex> lock(C->explain_mu);
    if (C->explain) return P2_OK;
    const WitnessTables T = witness_tables(C->c, false);
    auto E = std::make_unique<ExplainTables>();
    E->n_free = (u32)T.free_slots.size();
    if (upload(E->mem, &E->d_ops, C->c.ops.data(), C->c.ops.size()) || upload(E->mem, &E->d_free_slots, T.free_slots.data(), T.free_slots.size()) ||
        upload(E->mem, &E->d_slot_row, T.slot_row.data(), T.slot_row.size()) || upload(E->mem, &E->d_slot_target, T.slot_target.data(), T.slot_target.size()))
        return P2_ERR_HIP;
    C->explain = std::move(E);
    return P2_OK;
}
static int witness_explain_impl(p2_circuit* C, const p2_assignment* input, int* status, p2_witness_fault* out) {
    if (!C) return witness_null_handle("p2_witness_explain");
    if (!input || !status || !out || (input->count && (!input->targets || !input->values))) return set_error("p2_witness_explain: null argument"), P2_ERR_INVALID;
    std::vector<u32> in_slots;
    if (int rc = target_slots(C, input->targets, input->count, "input", in_slots)) return rc;
    HIPCHECK(hipSetDevice(C->device));
    if (int rc = explain_tables(C)) return rc;
    const ExplainTables& E = *C->explain;
    WitnessLease lease(C);
    WitnessWs* W = lease.ws.get();
    if (!W) return P2_ERR_HIP;
    const u32 ni = (u32)input->count;
    const std::vector<u32> prev = input_prev_links(in_slots, C->c.num_slots);
    int force_status = 0;  // an assignment has no "absent" marker: any value >= p is non-canonical, also the one k_witness takes for the marker
    for (u32 i = 0; i < ni; i++)
        if (input->values[i] >= gl::P) force_status = 1;
    HIPCHECK(hipEventSynchronize(W->done));
    if (!W->d_ex_in.grow(std::max<size_t>(ni, 1)) || !W->d_prev.grow(std::max<size_t>(ni, 1))) return set_error("witness workspace could not be allocated"), P2_ERR_HIP;
    if (!W->d_keys && (W->d_keys.alloc(3) != hipSuccess || W->d_fault.alloc(1) != hipSuccess || W->h_fault.alloc_bytes(sizeof(p2_witness_fault) + sizeof(int)) != hipSuccess))
        return set_error("witness workspace could not be allocated"), P2_ERR_HIP;
    int* d_status = (int*)(W->d_keys + 2);
    if (int rc = witness_put_slots(W, W->d_input_slots, W->h_input_slots, in_slots)) return rc;
    hipStream_t st = W->stream;
    if (ni) {
        HIPCHECK(hipMemcpy(W->d_ex_in, input->values, (size_t)ni * 8, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(W->d_prev, prev.data(), (size_t)ni * 4, hipMemcpyHostToDevice));
    }
    HIPCHECK(hipMemsetAsync(W->d_keys, 0xFF, 16, st));
    if (int rc = witness_run(C, W, 1, ni, W->d_ex_in, 0, nullptr, d_status, st)) return rc;
    WCheckCtx x{};
    x.ops = E.d_ops, x.num_ops = (u32)C->c.ops.size(), x.num_slots = C->c.num_slots, x.n = (u32)C->n;
    x.val = W->d_values, x.lut_ent = C->d_lut_ent, x.wire_slot = C->d_wire_slot;
    x.free_slots = E.d_free_slots, x.num_free = E.n_free, x.slot_target = E.d_slot_target, x.slot_row = E.d_slot_row;
    x.input_slots = W->d_input_slots, x.input_values = W->d_ex_in, x.n_inputs = ni, x.absent_marker = 0;
    LAUNCH_ON(st, k_witness_check, g1(std::max<size_t>((size_t)x.num_ops + x.num_free, 1), 256), dim3(256), x, W->d_keys);
    LAUNCH_ON(st, k_witness_report, dim3(1), dim3(256), x, (const u32*)W->d_prev, d_status, force_status, (const unsigned long long*)W->d_keys, W->d_fault);
    HIPCHECK(hipEventRecord(W->done, st));
    int* h_status = (int*)(W->h_fault + 1);
    HIPCHECK(hipMemcpyAsync(W->h_fault, W->d_fault, sizeof(p2_witness_fault), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(h_status, d_status, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    *out = *W->h_fault;
    *status = *h_status;
    lease.failed = false;
    return P2_OK;
}

// ---------------------------------------------------------------------------------- the device of a call, the one-launch runner
static int pick_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return set_error("no HIP device available"), P2_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return set_error("device index out of range"), P2_ERR_INVALID;
    HIPCHECK(hipSetDevice(device));
    return 0;
}
// ---- one runner for the calls that are one launch over buffers the caller sizes: the per-item batch calls in their host and
// _device forms, and the single-launch test primitives.  A call states its shape check, count, where it runs, its buffers in the
// order the launch takes them, and the launch.  run_batch does the rest, in this order (callers see it): the shape error;
// count == 0 is P2_OK; a buffer that is NULL although it has elements and is not optional is "null argument"; pick_device; then
// host buffers are staged (ins uploaded, outs allocated), the launch goes on the stream -- the null stream for host buffers --
// and the outs are copied back in list order, so the call returns with the results in host memory.  For device buffers nothing
// but the launch is enqueued.  The launch gets NULL for a buffer of zero elements and for an optional buffer the caller left
// out, in both forms; every other buffer is the staged copy or the caller's device pointer.  A scratch buffer is working memory
// of the launch, never copied: host forms pass no pointer and get an allocation for the call, device forms pass the caller's.
// The launch may enqueue more than one kernel on the stream.
enum BufDir { BUF_IN, BUF_OUT, BUF_INOUT, BUF_SCRATCH };
struct Buf {
    void* p;
    size_t n, elem;  // total elements, bytes per element
    BufDir dir;
    bool optional;  // may be NULL although n > 0: the launch gets NULL and nothing is copied
};
template <class T>
static Buf buf_in(const T* p, size_t n) { return {(void*)p, n, sizeof(T), BUF_IN, false}; }
template <class T>
static Buf buf_out(T* p, size_t n, bool optional = false) { return {p, n, sizeof(T), BUF_OUT, optional}; }
template <class T>
static Buf buf_inout(T* p, size_t n) { return {p, n, sizeof(T), BUF_INOUT, false}; }
template <class T>
static Buf buf_scratch(T* p, size_t n) { return {p, n, sizeof(T), BUF_SCRATCH, false}; }
struct DevPtr {  // a device pointer as the launch takes it: it converts to the kernel's parameter type
    void* p = nullptr;
    template <class T>
    operator T*() const { return (T*)p; }
};
struct Where {
    int device;
    bool on_device;  // the buffers are device memory: nothing is staged and the launch goes on `stream`
    hipStream_t stream;
};
static Where on_host(int device) { return {device, false, nullptr}; }
static Where on_device(int device, void* stream) { return {device, true, (hipStream_t)stream}; }
template <size_t N, class Launch>
static int run_batch(const char* bad_shape, size_t count, Where w, const Buf (&bufs)[N], Launch&& launch) {
    return guarded_rc([&]() -> int {
        if (bad_shape) return set_error(bad_shape), P2_ERR_INVALID;
        if (count == 0) return (int)P2_OK;
        for (const Buf& b : bufs)
            if (b.n && !b.p && !b.optional && (b.dir != BUF_SCRATCH || w.on_device)) return set_error("null argument"), P2_ERR_INVALID;
        if (int rc = pick_device(w.device)) return rc;
        Allocs tmp;
        DevPtr d[N];
        for (size_t i = 0; i < N; i++) {
            const Buf& b = bufs[i];
            if (!b.n || (!b.p && b.dir != BUF_SCRATCH)) continue;
            if (w.on_device) {
                d[i].p = b.p;
                continue;
            }
            char* q;
            if (dalloc(tmp, &q, b.n * b.elem)) return P2_ERR_HIP;
            d[i].p = q;
            if (b.dir == BUF_IN || b.dir == BUF_INOUT) HIPCHECK(hipMemcpy(q, b.p, b.n * b.elem, hipMemcpyHostToDevice));
        }
        launch(d, w.stream);
        HIPCHECK(hipGetLastError());
        if (w.on_device) return (int)P2_OK;
        for (size_t i = 0; i < N; i++)
            if (d[i].p && (bufs[i].dir == BUF_OUT || bufs[i].dir == BUF_INOUT)) HIPCHECK(hipMemcpy(bufs[i].p, d[i].p, bufs[i].n * bufs[i].elem, hipMemcpyDeviceToHost));
        return (int)P2_OK;
    });
}

extern "C" {

int p2_gpu_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

p2_circuit* p2_circuit_load(const uint8_t* blob, size_t len, int device) {
    try {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
            set_error("no HIP device available: the prover has no CPU fallback");
            return nullptr;
        }
        if (device < 0 || device >= ndev) {
            set_error("device index out of range");
            return nullptr;
        }
        std::unique_ptr<p2_circuit, void (*)(p2_circuit*)> owner(new p2_circuit(), p2_circuit_free);  // until the load has succeeded
        p2_circuit* C = owner.get();
        C->c = deserialize(blob, len);
        const Circuit& c = C->c;
        if (c.cfg.rate_bits != 3 || c.cfg.num_challenges != 2 || c.cfg.quotient_degree_factor != 8 || c.cfg.num_routed_wires != 80 || c.cfg.arity_bits != 4 ||
            c.cfg.num_query_rounds > 64 || c.gates.size() > p2::MAX_GATE_TYPES || c.luts.size() > p2::MAX_LUTS)
            throw std::runtime_error("only CircuitConfig::standard_recursion_config() is supported");
        if (c.degree_bits > 22) throw std::runtime_error("degree_bits > 22 is not supported");
        C->device = device;
        C->dom.logn = c.degree_bits;
        C->dom.rate_bits = c.cfg.rate_bits, C->dom.cap_height = c.cfg.cap_height, C->dom.hasher = c.cfg.hasher;
        C->n = c.n();
        C->lde_bits = c.degree_bits + c.cfg.rate_bits;
        C->N = C->n << c.cfg.rate_bits;
        C->dom.arities = c.reduction_arity_bits();
        // routed-only gates leave wires 80..134 identically zero (never materialised); PoseidonGate rows use all 135
        C->active_wires = (c.poseidon_rows.empty() && !c.cfg.zero_knowledge) ? c.cfg.num_routed_wires : c.cfg.num_wires;
        for (int i = 0; i < 4; i++) C->zk_key.k[i] = os_random_field();
        // environment defaults for the options, read once here (never per call)
        if (const char* e = getenv("P2AES_CHUNK")) C->opt_chunk = (size_t)std::max(1, atoi(e));
        if (const char* e = getenv("P2AES_STREAMS")) C->opt_streams = (size_t)std::min(8, std::max(1, atoi(e)));
        if (const char* e = getenv("P2AES_WITNESS_FUSE")) C->opt_witness_fuse = (u32)std::min(1024, std::max(1, atoi(e)));
        C->opt_debug_timing = getenv("P2AES_DEBUG_TIMING") != nullptr;
        if (const char* e = getenv("P2AES_WITNESS_CHUNK")) C->wit.set_key((size_t)std::min(4096, std::max(1, atoi(e))));
        if (const char* e = getenv("P2AES_TEST_FAIL_ALLOC_AFTER")) C->fail_alloc_after = atol(e);
        C->layout = make_proof_layout(c);
        C->pbytes = C->layout.bytes;
        if (hipSetDevice(device) != hipSuccess) throw std::runtime_error("hipSetDevice failed");
        if (C->setup.open(hipStreamDefault) != hipSuccess) throw std::runtime_error("hipStreamCreate failed");
        if (C->ev_witness.create(hipEventDisableTiming) != hipSuccess) throw std::runtime_error("hipEventCreate failed");
        if (raise_ntt_lds_limits() != hipSuccess) throw std::runtime_error("cannot raise the dynamic LDS limit for the NTT kernels");
        // opening maps: the evaluation slots in observed and in serialised order
        const std::vector<u32> obs = C->layout.set.slots_in(true), ser = C->layout.set.slots_in(false);
        C->ev_count = C->layout.set.slots;
        C->n_obs = (u32)obs.size();
        C->n_ser = (u32)ser.size();
        if (C->layout.final_len > C->n_obs) throw std::runtime_error("final polynomial larger than the observation buffer");
        if (upload(C->allocs, &C->d_map_obs, obs.data(), obs.size()) || upload(C->allocs, &C->d_map_ser, ser.data(), ser.size())) throw std::runtime_error(g_last_error);
        if (circuit_setup(C)) throw std::runtime_error(g_last_error);
        if (verify_setup(C) || cmp_setup(C)) throw std::runtime_error(g_last_error);
        return owner.release();
    } catch (std::exception& e) {
        return set_error(e.what()), nullptr;
    }
}
p2_circuit::p2_circuit() = default;
p2_circuit::~p2_circuit() {
    if (setup.stream) (void)hipStreamSynchronize(setup.stream);
    release_workspaces(this);
}
size_t p2_debug_live_resources(void) { return g_live_resources.load(); }

void p2_circuit_free(p2_circuit* C) {
    if (!C) return;
    (void)hipSetDevice(C->device);
    (void)hipDeviceSynchronize();
    delete C;
}

int p2_circuit_verifier_data(const p2_circuit* C, uint64_t* out, size_t cap, size_t* n_written) {
    if (cap < C->verifier_data.size()) return set_error("buffer too small"), P2_ERR_INVALID;
    memcpy(out, C->verifier_data.data(), C->verifier_data.size() * 8);
    *n_written = C->verifier_data.size();
    return P2_OK;
}
size_t p2_circuit_proof_bytes(const p2_circuit* C) { return C->pbytes; }
size_t p2_circuit_num_public_inputs(const p2_circuit* C) { return C ? C->c.pi_slots.size() : 0; }
int p2_circuit_public_inputs(const p2_circuit* C, const uint8_t* proof, size_t proof_len, uint64_t* out, size_t cap, size_t* n_written) {
    if (!C) return set_error("p2_circuit_public_inputs: null circuit handle"), P2_ERR_INVALID;
    return read_public_inputs(C->layout, proof, proof_len, out, cap, n_written);
}
size_t p2_circuit_chunk_proofs(p2_circuit* C) {
    std::lock_guard<std::mutex> lock(C->mu);
    return C->chunk;
}
int p2_circuit_set_zk_key(p2_circuit* C, const uint64_t key[4]) {
    // TEST ONLY, and refused unless the process opted in: a fixed key is not secret, and a (key, proof index) pair that is used
    // for two different witnesses breaks zero-knowledge.
    const char* allow = getenv("P2AES_ALLOW_FIXED_ZK_KEY");
    if (!allow || strcmp(allow, "1") != 0)
        return set_error("p2_circuit_set_zk_key is a test hook: set P2AES_ALLOW_FIXED_ZK_KEY=1 to fix the blinding key (never in production)"), P2_ERR_INVALID;
    std::lock_guard<std::mutex> lock(C->mu);
    bool same = true;
    for (int i = 0; i < 4; i++) same = same && C->zk_key.k[i] == key[i] % gl::P;
    if (same) return P2_OK;  // the proof counter keeps running: setting the key a handle already holds never replays an index
    for (int i = 0; i < 4; i++) C->zk_key.k[i] = key[i] % gl::P;
    C->zk_counter = 0;
    return P2_OK;
}
int p2_circuit_set_zk_seed(p2_circuit* C, uint64_t seed) {
    const uint64_t key[4] = {seed, 0, 0, 0};
    return p2_circuit_set_zk_key(C, key);
}

// out_targets / n_out / d_out: the targets read back from every witness ([batch][n_out]); n_out = 0 is p2_prove_batch_device
static int prove_batch_device_impl(p2_circuit* C, size_t batch, const p2_target* targets, size_t n_targets, const uint64_t* d_values, const p2_target* out_targets,
                                   size_t n_out, uint64_t* d_out, uint8_t* d_proofs, int* d_status, void* stream) {
    if (!C) return witness_null_handle("p2_prove_batch_outputs_device");
    if (n_out && (!out_targets || !d_out)) return set_error("p2_prove_batch_outputs_device: null output buffer"), P2_ERR_INVALID;
    std::lock_guard<std::mutex> lock(C->mu);
    hipStream_t caller = (hipStream_t)stream;
    HIPCHECK(hipSetDevice(C->device));
    std::vector<u32> slots, out_slots;
    if (int rc = target_slots(C, targets, n_targets, "input", slots)) return rc;
    if (int rc = target_slots(C, out_targets, n_out, "output", out_slots)) return rc;
    // Chunk size / stream count: options "chunk" (default 128 proofs per chunk) and "streams" (default 2).  A batch smaller
    // than chunk x streams is split evenly over the streams, so that the serial stages of one chunk (witness levels,
    // the Fiat-Shamir chain, proof-of-work) overlap the wide kernels of the other.  A later, larger batch regrows the
    // workspaces (alloc_workspace); a smaller one runs in the existing ones.
    size_t want_chunk = C->opt_chunk, want_streams = C->opt_streams;
    {
        // cap the chunk so that all workspaces fit in ~80% of the HBM that is free (plus what the workspaces hold now); chunks of
        // a batch are then made EQUAL (a 32-proof batch under a cap of 14 is 3 x 11, not 14 + 14 + 4)
        const Circuit& c = C->c;
        size_t n = C->n, N = C->N, zc = c.num_zs_cols(), qc = c.num_quotient_cols(), act = C->active_wires, NC = c.cfg.num_challenges;
        size_t words = c.num_slots + (act + zc) * 2 * n + qc * n + (act + zc + qc) * N + NC * (c.num_partial_products() + c.num_sldc_polys() + 2) * n +
                       2 * NC * N + 3 * 8 * N + 16 * n + 4 * N;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            free_b += 8 * words * C->chunk * C->ws.size();
            size_t fit = (size_t)(0.8 * (double)free_b) / (8 * words * want_streams);
            want_chunk = std::max<size_t>(1, std::min(want_chunk, fit));
        }
    }
    size_t nstreams = std::min(want_streams, std::max<size_t>(batch, 1));
    size_t chunk = std::min(want_chunk, (std::max<size_t>(batch, 1) + nstreams - 1) / nstreams);
    {
        const size_t nchunks = (std::max<size_t>(batch, 1) + chunk - 1) / chunk;
        chunk = (std::max<size_t>(batch, 1) + nchunks - 1) / nchunks;
    }
    if (C->chunk >= chunk && C->ws.size() >= nstreams) chunk = C->chunk, nstreams = C->ws.size();
    if (alloc_workspace(C, chunk, (u32)n_targets, nstreams)) return P2_ERR_HIP;
    // Ordering with the caller: the proving streams wait for everything already enqueued on the caller's stream (its
    // inputs) and the caller's stream then waits for the proofs.  NULL means the legacy default stream, which is
    // ordered the same way (an event recorded on stream 0) -- no device-wide synchronisation, so consecutive calls
    // pipeline into each other.
    Event ev_in;
    HIPCHECK_AS("hipEventCreateWithFlags(&ev_guard.e, hipEventDisableTiming)", ev_in.create(hipEventDisableTiming));
    HIPCHECK(hipEventRecord(ev_in, caller));
    for (auto& W : C->ws) HIPCHECK(hipStreamWaitEvent(W->lane.stream, ev_in, 0));
    // the blinding counter advances before anything is enqueued: a batch that fails half-way must not leave its proof
    // indices to be used again under the same key
    const u64 proof_base0 = C->zk_counter;
    C->zk_counter += batch;
    size_t k = 0;
    for (size_t done = 0; done < batch; done += C->chunk, k++) {
        u32 B = (u32)std::min(C->chunk, batch - done);
        Workspace& W = *C->ws[k % C->ws.size()];
        if (W.h_input_slots != slots) {  // a new target list: wait for the workspace's earlier chunks, then upload
            HIPCHECK(hipStreamSynchronize(W.lane.stream));
            HIPCHECK(hipMemcpy(W.d_input_slots, slots.data(), n_targets * 4, hipMemcpyHostToDevice));
            W.h_input_slots = slots;
        }
        if (n_out && (W.h_out_slots != out_slots || !W.d_out_slots)) {  // likewise the out-target list
            HIPCHECK(hipStreamSynchronize(W.lane.stream));
            if (!W.d_out_slots.grow(n_out)) return set_error("out-target list could not be allocated"), P2_ERR_HIP;
            HIPCHECK(hipMemcpy(W.d_out_slots, out_slots.data(), n_out * 4, hipMemcpyHostToDevice));
            W.h_out_slots = out_slots;
        }
        int rc = prove_chunk(C, W, B, (u32)n_targets, d_values + done * n_targets, (u32)n_out, n_out ? d_out + done * n_out : nullptr, d_proofs + done * C->pbytes,
                             d_status + done, proof_base0 + done);
        if (rc) return rc;
    }
    for (auto& W : C->ws) {
        HIPCHECK(hipEventRecord(W->done, W->lane.stream));
        HIPCHECK(hipStreamWaitEvent(caller, W->done, 0));
    }
    return P2_OK;
}
int p2_prove_batch_device(p2_circuit* C, size_t batch, const p2_target* targets, size_t n_targets, const uint64_t* d_values, uint8_t* d_proofs, int* d_status,
                          void* stream) {
    return guarded_rc([&] { return prove_batch_device_impl(C, batch, targets, n_targets, d_values, nullptr, 0, nullptr, d_proofs, d_status, stream); });
}
int p2_prove_batch_outputs_device(p2_circuit* C, size_t batch, const p2_target* targets, size_t n_targets, const uint64_t* d_values, const p2_target* out_targets,
                                  size_t n_out, uint64_t* d_out, uint8_t* d_proofs, int* d_status, void* stream) {
    return guarded_rc([&] { return prove_batch_device_impl(C, batch, targets, n_targets, d_values, out_targets, n_out, d_out, d_proofs, d_status, stream); });
}
int p2_witness_batch_device(p2_circuit* C, size_t batch, const p2_target* targets, size_t n_targets, const uint64_t* d_values, const p2_target* out_targets, size_t n_out,
                            uint64_t* d_out, int* d_status, void* stream) {
    return guarded_rc([&] { return witness_batch_device_impl(C, batch, targets, n_targets, d_values, out_targets, n_out, d_out, d_status, stream); });
}
int p2_witness_batch(p2_circuit* C, size_t batch, const p2_assignment* inputs, const p2_target* out_targets, size_t n_out, uint64_t* out_values, int* status) {
    return guarded_rc([&] { return witness_batch_impl(C, batch, inputs, out_targets, n_out, out_values, status); });
}
int p2_witness_explain(p2_circuit* C, const p2_assignment* input, int* status, void* out) {
    return guarded_rc([&] { return witness_explain_impl(C, input, status, (p2_witness_fault*)out); });
}

int p2_circuit_synchronize(p2_circuit* C) {
    std::lock_guard<std::mutex> lock(C->mu);
    HIPCHECK(hipSetDevice(C->device));
    HIPCHECK(hipStreamSynchronize(C->setup.stream));
    for (auto& W : C->ws) HIPCHECK(hipStreamSynchronize(W->lane.stream));
    if (C->timing_on) collect_timing(C);
    return P2_OK;
}

static int prove_batch_impl(p2_circuit* C, size_t batch, const p2_assignment* inputs, const p2_target* out_targets, size_t n_out, uint64_t* out_values,
                            uint8_t* proofs, int* status) {
    if (!C) return witness_null_handle("p2_prove_batch_outputs");
    if (n_out && (!out_targets || (batch && !out_values))) return set_error("p2_prove_batch_outputs: null output buffer"), P2_ERR_INVALID;
    if (n_out) {  // an out-target outside the circuit is an error of the call, whatever the batch
        std::vector<u32> out_slots;
        if (int rc = target_slots(C, out_targets, n_out, "output", out_slots)) return rc;
    }
    if (batch == 0) return P2_OK;
    HIPCHECK(hipSetDevice(C->device));
    PackedInputs pk;  // the layout of the batch on one target list, and the witnesses the host rejects
    pk.plan(batch, inputs);
    const size_t nt = pk.nt, nvals = pk.nvals(batch);
    Lease<Staging, NoKey> S(C->staging, [](NoKey) { return std::make_unique<Staging>(); });
    if (!S->fit(nvals * 8, batch * C->pbytes, batch, batch * n_out * 8)) {
        S.ws.reset();  // dropped, not returned to the pool
        return set_error("staging buffers for p2_prove_batch could not be allocated"), P2_ERR_HIP;
    }
    const auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const bool dbg = C->opt_debug_timing;
    double t_a = now();
    pk.fill(batch, inputs, S->vals.h, true);  // pinned: the values are laid out straight into the buffer the DMA engine reads
    double t_b = now();
    // one stream carries upload -> prove -> download; p2_prove_batch_device orders the proving streams with it
    HIPCHECK(hipMemcpyAsync(S->vals.d, S->vals.h, nvals * 8, hipMemcpyHostToDevice, S->stream));
    int rc = p2_prove_batch_outputs_device(C, batch, pk.targets, nt, S->vals.d, out_targets, n_out, S->out.d, S->proofs.d, S->stat.d, (void*)S->stream);
    if (rc != P2_OK) return rc;  // (the lease drains S->stream)
    HIPCHECK(hipMemcpyAsync(S->proofs.h, S->proofs.d, batch * C->pbytes, hipMemcpyDeviceToHost, S->stream));
    HIPCHECK(hipMemcpyAsync(S->stat.h, S->stat.d, batch * sizeof(int), hipMemcpyDeviceToHost, S->stream));
    if (n_out) HIPCHECK(hipMemcpyAsync(S->out.h, S->out.d, batch * n_out * 8, hipMemcpyDeviceToHost, S->stream));
    double t_c = now();
    HIPCHECK(hipStreamSynchronize(S->stream));
    double t_d = now();
    memcpy(proofs, S->proofs.h, batch * C->pbytes);
    memcpy(status, S->stat.h, batch * sizeof(int));
    if (n_out) memcpy(out_values, S->out.h, batch * n_out * 8);
    for (size_t i = 0; i < batch; i++)
        if (pk.host_status[i]) {
            status[i] = pk.host_status[i];
            memset(proofs + i * C->pbytes, 0, C->pbytes);
            std::fill(out_values + i * n_out, out_values + (i + 1) * n_out, P2_VALUE_UNSET);  // what ran was not this witness
        }
    S.failed = false;
    if (dbg) fprintf(stderr, "[p2aes] pack %.3f enqueue %.3f wait %.3f unpack %.3f s\n", t_b - t_a, t_c - t_b, t_d - t_c, now() - t_d);
    return P2_OK;
}
int p2_prove_batch_outputs(p2_circuit* C, size_t batch, const p2_assignment* inputs, const p2_target* out_targets, size_t n_out, uint64_t* out_values, uint8_t* proofs,
                           int* status) {
    return guarded_rc([&] { return prove_batch_impl(C, batch, inputs, out_targets, n_out, out_values, proofs, status); });
}
int p2_prove_batch(p2_circuit* C, size_t batch, const p2_assignment* inputs, uint8_t* proofs, int* status) {
    return guarded_rc([&] { return prove_batch_impl(C, batch, inputs, nullptr, 0, nullptr, proofs, status); });
}

// In-process multi-device form of p2_prove_batch: contiguous balanced ranges of the batch, one host thread per handle.
// zk circuits: every handle blinds with ITS OWN key (drawn from the OS at load) and its own proof counter; handles that were
// given one fixed key by the test hook would blind different witnesses with the same (key, index) values.
static int prove_batch_multi_impl(p2_circuit* const* handles, size_t n_handles, size_t batch, const p2_assignment* inputs, uint8_t* proofs, int* status) {
    if (n_handles == 0 || !handles) return set_error("p2_prove_batch_multi needs at least one handle"), P2_ERR_INVALID;
    for (size_t h = 0; h < n_handles; h++)
        if (!handles[h] || handles[h]->pbytes != handles[0]->pbytes || handles[h]->verifier_data != handles[0]->verifier_data)
            return set_error("p2_prove_batch_multi: the handles are not loads of one compiled circuit"), P2_ERR_INVALID;
    if (batch == 0) return P2_OK;
    const size_t pb = handles[0]->pbytes, base = batch / n_handles, extra = batch % n_handles;
    std::vector<int> rc(n_handles, P2_OK);
    std::vector<std::string> err(n_handles);
    std::vector<std::thread> workers;
    size_t lo = 0;
    for (size_t h = 0; h < n_handles; h++) {
        const size_t cnt = base + (h < extra ? 1 : 0), first = lo;
        lo += cnt;
        if (cnt == 0) continue;
        workers.emplace_back([=, &rc, &err] {
            rc[h] = p2_prove_batch(handles[h], cnt, inputs + first, proofs + first * pb, status + first);
            if (rc[h] != P2_OK) err[h] = g_last_error;  // the error slot is thread-local: carry it to the caller's thread
        });
    }
    for (auto& w : workers) w.join();
    for (size_t h = 0; h < n_handles; h++)
        if (rc[h] != P2_OK) return set_error("handle " + std::to_string(h) + " (device " + std::to_string(handles[h]->device) + "): " + err[h]), rc[h];
    return P2_OK;
}
int p2_prove_batch_multi(p2_circuit* const* handles, size_t n_handles, size_t batch, const p2_assignment* inputs, uint8_t* proofs, int* status) {
    return guarded_rc([&] { return prove_batch_multi_impl(handles, n_handles, batch, inputs, proofs, status); });
}

int p2_circuit_set_option(p2_circuit* C, const char* name, long value) {
    std::lock_guard<std::mutex> lock(C->mu);
    std::string k(name ? name : "");
    if (k == "chunk") {
        if (value < 1 || value > 4096) return set_error("option chunk: 1..4096 proofs"), P2_ERR_INVALID;
        C->opt_chunk = (size_t)value;
    } else if (k == "streams") {
        if (value < 1 || value > 8) return set_error("option streams: 1..8"), P2_ERR_INVALID;
        C->opt_streams = (size_t)value;
    } else if (k == "debug_timing") {
        C->opt_debug_timing = value != 0;
    } else if (k == "verify_chunk") {
        if (value < 1 || value > 4096) return set_error("option verify_chunk: 1..4096 proofs"), P2_ERR_INVALID;
        C->vfy.set_key((size_t)value);
    } else if (k == "witness_chunk") {
        if (value < 1 || value > 4096) return set_error("option witness_chunk: 1..4096 witnesses"), P2_ERR_INVALID;
        C->wit.set_key((size_t)value);
    } else {
        return set_error("unknown option (known: chunk, streams, debug_timing, verify_chunk, witness_chunk)"), P2_ERR_INVALID;
    }
    return P2_OK;
}

int p2_circuit_set_timing(p2_circuit* C, int enable) {
    std::lock_guard<std::mutex> lock(C->mu);
    C->timing_on = C->setup.timing = enable != 0;
    for (auto& W : C->ws) W->lane.timing = C->timing_on;
    C->times.clear();
    return P2_OK;
}
size_t p2_circuit_get_timing(p2_circuit* C, p2_kernel_time* out, size_t cap) {
    std::lock_guard<std::mutex> lock(C->mu);
    size_t k = 0;
    for (auto& kv : C->times) {
        if (k < cap) {
            memset(&out[k], 0, sizeof(out[k]));
            strncpy(out[k].name, kv.first.c_str(), sizeof(out[k].name) - 1);
            out[k].ms = kv.second.first;
            out[k].count = kv.second.second;
        }
        k++;
    }
    return k;
}

int p2_circuit_debug_read(p2_circuit* C, const char* name_c, size_t index, uint64_t* out, size_t cap, size_t* n_written) {
    std::lock_guard<std::mutex> lock(C->mu);
    HIPCHECK(hipSetDevice(C->device));
    HIPCHECK(hipDeviceSynchronize());
    const Circuit& c = C->c;
    std::string name(name_c);
    // `index` addresses proof (index % chunk) of the workspace that handled chunk (index / chunk) of the last call
    Workspace* W = C->ws.empty() ? nullptr : C->ws[(index / C->chunk) % C->ws.size()].get();
    if (W) index %= C->chunk;
    const size_t n = C->n, N = C->N;
    const u64* src = nullptr;
    size_t count = 0;
    // NAME (values), NAME_coeffs, NAME_lde and NAME_cap of every committed oracle
    const std::pair<std::string, const Oracle*> oracles[] = {{"pre", &C->pre}, {"wires", W ? &W->wires : nullptr}, {"zs", W ? &W->zs : nullptr}, {"quotient", W ? &W->quot : nullptr}};
    for (const auto& [prefix, o] : oracles) {
        if (!o) continue;
        if (name == prefix && o->vals) { src = o->vals + index * o->coef_stride; count = (size_t)o->cols * n; }
        else if (name == prefix + "_coeffs") { src = o->coef + index * o->coef_stride; count = (size_t)o->cols * n; }
        else if (name == prefix + "_lde") { src = o->lde + index * o->lde_stride; count = (size_t)(o->cols + o->salt) * N; }
        else if (name == prefix + "_cap") { src = o->tree.dig + index * o->dig_stride() + cap_off(o->tree, c.cfg.cap_height); count = 4u << c.cfg.cap_height; }
    }
    if (src) {}  // one of the oracles' buffers
    else if (!W) return set_error("nothing has been proven yet"), P2_ERR_INVALID;
    else if (name == "values") { src = W->d_values + index * c.num_slots; count = c.num_slots; }
    else if (name == "quotient_values") { src = W->d_qvals + index * 2 * N; count = 2 * N; }
    else if (name == "public_inputs_hash" && c.pi_slots.empty()) {
        if (cap < 4) return set_error("debug buffer too small"), P2_ERR_INVALID;
        for (int i = 0; i < 4; i++) out[i] = 0;  // hash_no_pad of zero public inputs
        *n_written = 4;
        return P2_OK;
    }
    else if (name == "public_inputs_hash") { src = W->d_pi_hash + index * 4; count = 4; }
    else if (name == "challenges") { src = W->d_chal + index * CH_WORDS; count = CH_WORDS; }
    else if (name == "openings") { src = W->d_ev + index * 2 * C->ev_count; count = 2 * (size_t)C->ev_count; }
    else if (name == "fri_final_poly_in") { src = W->d_fri_coef[0] + index * 2 * n; count = 2 * n; }
    else return set_error("unknown debug buffer"), P2_ERR_INVALID;
    if (count > cap) return set_error("debug buffer too small"), P2_ERR_INVALID;
    HIPCHECK(hipMemcpy(out, src, count * 8, hipMemcpyDeviceToHost));
    *n_written = count;
    return P2_OK;
}

// ---------------------------------------------------------------------------------- primitives (parity tests)
// ---- device self-test
namespace p2k {
__global__ void k_selftest(unsigned long long* bad, u64 seed, size_t threads) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= threads) return;
    u64 x = (seed | 1) + 0x9E3779B97F4A7C15ull * (t + 1);
    auto rnd = [&]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    unsigned long long b = 0;
    for (int i = 0; i < 64; i++) {
        u64 hi = rnd(), lo = rnd();
        const int m = i & 15;
        if (m == 0) hi &= gl::EPS;
        if (m == 1) lo &= gl::EPS;
        if (m == 2) hi |= ~gl::EPS;
        if (m == 3) lo |= ~gl::EPS;
        if (m == 4) hi = 0;
        if (m == 5) lo = 0;
        if (m == 6) {
            hi = ~0ull;
            lo = ~0ull - (x & 3);
        }
        if (m == 7) {
            hi &= ~gl::EPS;
            lo &= gl::EPS;
        }
        const u64 want = gl::reduce128(hi, lo);  // textbook form
        if (glf::canon(glf::red128(hi, lo)) != want) b++;
        glf::Acc a;
        a.init();
        a.fma(hi, lo);
        a.fma(lo, lo);
        if (glf::canon(a.reduce()) != gl::add(gl::mul(hi % gl::P, lo % gl::P), gl::mul(lo % gl::P, lo % gl::P))) b++;
        // a carry-consuming chain right after a reduction: the pattern the backend used to break
        const u64 r = glf::red128(hi, lo);
        u32 k, K;
        const u32 c0 = __builtin_addc((u32)r, 0xFFFFFFFFu, 0u, &k);
        const u32 c1 = __builtin_addc((u32)(r >> 32), 0u, k, &K);
        if ((K ? (((u64)c1 << 32) | c0) : r) != want) b++;
        // the mad-based field operations every kernel uses (gl.h) against the textbook forms
        const u64 x = hi % gl::P, y = lo % gl::P, z = rnd() % gl::P;
        if (gl::mul(x, y) != gl::mul_ref(x, y)) b++;
        if (gl::mul(hi, lo) != gl::mul_ref(x, y)) b++;  // non-canonical inputs are fine for mul
        if (gl::sub(x, y) != gl::sub_ref(x, y) || gl::sub(y, x) != gl::sub_ref(y, x)) b++;
        if (gl::mul_add(x, y, z) != gl::add_ref(gl::mul_ref(x, y), z)) b++;
        if (gl::add(x, y) != gl::add_ref(x, y) || gl::add(x, gl::P - 1) != gl::add_ref(x, gl::P - 1) || gl::add(y, gl::P - 1 - (y & 1)) != gl::add_ref(y, gl::P - 1 - (y & 1))) b++;
        if (glf::canon(hi) != hi % gl::P) b++;
        // the reduction's borrow case (R < H.hi + k), which random inputs never reach: 2^48 * (m 2^48) = m 2^96 = -m, and
        // 2^32 * (m 2^32) = m 2^64 with a zero low limb.  Odd threads keep random operands, so that one wave holds lanes that
        // borrow next to lanes that carry (the correction is chosen per wave, then applied per lane).
        {
            const u64 mm = ((t * 64 + i) & 0xFFFE) + 1;
            const u64 p48 = 1ull << 48, q = (t & 1) ? y : (mm << 48), pa = (t & 1) ? x : p48;
            if (gl::mul(pa, q) != gl::mul_ref(pa, q)) b++;
            if (glf::canon(glf::mulr(pa, q)) != gl::mul_ref(pa, q)) b++;
            if (gl::mul_add(pa, q, z) != gl::add_ref(gl::mul_ref(pa, q), z)) b++;
            const u64 e = (t & 2) ? (mm << 32) : (gl::P - mm), f = (t & 2) ? (1ull << 32) : (1ull << 48);
            if (gl::mul(e, f) != gl::mul_ref(e, f)) b++;
        }
    }
    u64 s0[12], s1[12];
    for (int k = 0; k < 12; k++) {
        s1[k] = (t & 3) == 3 ? rnd() : rnd() % gl::P;
        s0[k] = s1[k] % gl::P;
    }
    gl::poseidon(s0);
    glf::poseidon(s1);
    for (int k = 0; k < 12; k++) b += s0[k] != s1[k];
    if (b) atomicAdd(bad, b);
}
// the cooperative permutation (16 lanes per state) against the plain one: every group draws its own state
__global__ __launch_bounds__(64) void k_selftest_coop(unsigned long long* bad, u64 seed) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x, grp = t >> 4, i = t & 15;
    u64 st[12];
    u64 x = (seed | 1) + 0x9E3779B97F4A7C15ull * (grp + 1);
    for (int k = 0; k < 12; k++) {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        st[k] = (grp & 7) == 0 ? (k & 1 ? gl::P - 1 : 0) : x % gl::P;
    }
    u64 mine = 0;
    for (int k = 0; k < 12; k++)
        if ((u32)k == i) mine = st[k];
    const u64 got = glf::poseidon_coop(mine, i);
    gl::poseidon(st);  // every lane redundantly, the textbook form
    u64 want = 0;
    for (int k = 0; k < 12; k++)
        if ((u32)k == i) want = st[k];
    if (got != want) atomicAdd(bad, 1ull);
}
}  // namespace p2k

int p2_selftest_device(uint64_t seed, size_t threads, int device) {
    if (hipSetDevice(device) != hipSuccess) return set_error("no such HIP device"), -P2_ERR_HIP;
    Allocs mem;
    unsigned long long* d = nullptr;
    if (dalloc(mem, &d, 1) || hipMemset(d, 0, 8) != hipSuccess) return set_error("hipMalloc failed"), -P2_ERR_HIP;
    hipLaunchKernelGGL(p2k::k_selftest, dim3((u32)((threads + 255) / 256)), dim3(256), 0, 0, d, (u64)seed, threads);
    hipLaunchKernelGGL(p2k::k_selftest_coop, dim3((u32)std::min<size_t>(std::max<size_t>(threads / 64, 1), 4096)), dim3(64), 0, 0, d, (u64)seed);
    unsigned long long h = 0;
    if (hipError_t e = hipMemcpy(&h, d, 8, hipMemcpyDeviceToHost)) return set_error(hipGetErrorString(e)), -P2_ERR_HIP;
    return (int)std::min<unsigned long long>(h, 0x7FFFFFFF);
}

// ---- self-test of the lazy compositions of the polynomial-side kernels (gl.h, operand contracts)
namespace p2k {
// What a non-canonical intermediate does to these compositions shows only for values in [p, 2^64), which random data reaches with
// probability 2^-32: the operands are therefore drawn from the extremes, and wherever a contract says "any u64" they are not
// reduced first.  `r` is the random word the draw may use, `sel` chooses.
__device__ __forceinline__ u64 lazy_draw(u64 r, u32 sel) {
    switch (sel % 12) {
        case 0: return 0;
        case 1: return 1;
        case 2: return gl::EPS;
        case 3: return 1ull << 32;
        case 4: return gl::P - 1;
        case 5: return gl::P;
        case 6: return gl::P + 1;
        case 7: return ~0ull;
        case 8: return ((r & 0xFFFF) | 1) << 48;  // zero low limbs: the reduction's borrow case
        case 9: return (r & gl::EPS) << 32;
        default: return r;
    }
}
__global__ void k_selftest_lazy(unsigned long long* bad, u64 seed, size_t threads) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= threads) return;
    u64 x = (seed | 1) + 0x9E3779B97F4A7C15ull * (t + 1), xu = (seed | 1) ^ 0xD1B54A32D192ED03ull;  // xu: the same in every thread
    auto step = [](u64& v) {
        v ^= v << 13;
        v ^= v >> 7;
        v ^= v << 17;
        return v;
    };
    auto rnd = [&]() {
        const u64 r = step(x);
        return lazy_draw(r, (u32)(r >> 40));
    };
    auto rnd_uniform = [&]() {  // for the operands that the kernels read from SGPRs: a lane-dependent value may not go there
        const u64 r = step(xu);
        return lazy_draw(r, (u32)(r >> 40));
    };
    auto M = [](u64 a, u64 b) { return gl::mul_ref(a % gl::P, b % gl::P); };
    unsigned long long b = 0;
    for (int i = 0; i < 16; i++) {
        // permutation term and product step: w and gamma canonical as loaded, everything else any u64; two terms multiplied
        // without a canonical value in between, then the running product continued
        const u64 w = rnd() % gl::P, g = rnd() % gl::P, beta = rnd(), f0 = rnd(), f1 = rnd(), prod = rnd();
        const u64 tt = gl::add(w, g);
        if (tt != gl::add_ref(w, g)) b++;
        const u64 t0 = perm_term(beta, f0, tt), t1 = perm_term(beta, f1, tt);
        const u64 r0 = gl::add_ref(M(beta, f0), tt), r1 = gl::add_ref(M(beta, f1), tt);
        if (glf::canon(t0) != r0 || glf::canon(t1) != r1) b++;
        if (glf::canon(perm_step(perm_step(prod, t0), t1)) != M(M(prod, r0), r1)) b++;
        if (gl::mul(perm_step(t0, t1), prod) != M(M(r0, r1), prod)) b++;  // what is stored: canonical
        const u64 any = rnd();
        if (glf::canon(perm_term(beta, f0, any)) != gl::add_ref(M(beta, f0), any % gl::P)) b++;  // the addend may be any u64 too
        // Acc dot product: five terms, any u64, the extension factor uniform
        {
            glf::Acc ka, kb;
            ka.init(), kb.init();
            u64 wka = 0, wkb = 0;
            for (int j = 0; j < 5; j++) {
                const u64 v = rnd(), ua = rnd_uniform(), ub = rnd_uniform();
                acc_dot2_k(ka, kb, v, ua, ub);
                wka = gl::add_ref(wka, M(v, ua));
                wkb = gl::add_ref(wkb, M(v, ub));
            }
            if (acc_value(ka) != wka || acc_value(kb) != wkb) b++;
        }
        // table-power multiply: the high factor (and its 7-fold second word, an operand of its own here) uniform
        {
            const u64 l0 = rnd(), l1 = rnd(), h0 = rnd_uniform(), h1 = rnd_uniform(), h1w = rnd_uniform();
            const E2 got = tabpow_mul(gl::e2(l0, l1), h0, h1, h1w);
            if (got.a != gl::add_ref(M(l0, h0), M(l1, h1w)) || got.b != gl::add_ref(M(l0, h1), M(l1, h0))) b++;
            const u64 c = rnd_uniform() % gl::P, d = rnd_uniform() % gl::P;  // and as the table holds it: h1w = 7 h1, canonical
            const E2 lo = gl::e2(l0 % gl::P, l1 % gl::P), want = gl::mul(lo, gl::e2(c, d)), have = tabpow_mul(lo, c, d, gl::mul(d, gl::W_EXT));
            if (have.a != want.a || have.b != want.b) b++;
        }
        // table-slot and looking-slot steps of the one-walk quotient: challenges and wire values canonical as loaded, the
        // running values any u64; three steps, each on what the one before left (never canonicalised in between), then the
        // closing terms; and the plain forms on canonical values
        {
            const u64 dA = rnd_uniform() % gl::P, dB = rnd_uniform() % gl::P, dAl = rnd_uniform() % gl::P, dD = rnd_uniform() % gl::P;
            u64 cur = rnd(), tsum = rnd(), tprod = rnd(), lsum = rnd(), lprod = rnd();
            u64 rcur = cur % gl::P, rtsum = tsum % gl::P, rtprod = tprod % gl::P, rlsum = lsum % gl::P, rlprod = lprod % gl::P;
            for (int st = 0; st < 3; st++) {
                const u64 win = rnd() % gl::P, wout = rnd() % gl::P, wm = rnd() % gl::P;
                const u64 f = gl::sub_ref(dAl, gl::add_ref(gl::mul_ref(dA, wout), win));
                const u64 ncur = gl::add_ref(gl::mul_ref(rcur, dD), gl::add_ref(gl::mul_ref(dB, wout), win));
                const u64 nts = gl::add_ref(gl::mul_ref(rtsum, f), gl::mul_ref(wm, rtprod)), ntp = gl::mul_ref(rtprod, f);
                const u64 nls = gl::add_ref(gl::mul_ref(rlsum, f), rlprod), nlp = gl::mul_ref(rlprod, f);
                {  // the plain forms from the same canonical state: canonical results
                    u64 c2 = rcur, s2 = rtsum, p2_ = rtprod;
                    lut_step<false>(c2, s2, p2_, dA, dB, dAl, dD, win, wout, wm);
                    if (c2 != ncur || s2 != nts || p2_ != ntp) b++;
                }
                lut_step<true>(cur, tsum, tprod, dA, dB, dAl, dD, win, wout, wm);
                lu_step(lsum, lprod, dA, dAl, win, wout);  // canonical from the second step on, whatever it started from
                rcur = ncur, rtsum = nts, rtprod = ntp, rlsum = nls, rlprod = nlp;
                if (glf::canon(cur) != rcur || glf::canon(tsum) != rtsum || glf::canon(tprod) != rtprod) b++;
                if (lsum != rlsum || lprod != rlprod) b++;
            }
            const u64 diff = rnd() % gl::P;
            if (glf::canon(lut_close<true>(tprod, tsum, diff)) != gl::sub_ref(gl::mul_ref(rtprod, diff), rtsum)) b++;
            if (glf::canon(lu_close(lprod, lsum, diff)) != gl::add_ref(gl::mul_ref(rlprod, diff), rlsum)) b++;
            if (gl::sub(dAl, glf::canon(cur)) != gl::sub_ref(dAl, rcur)) b++;  // the RE term's subtrahend, canonicalised once
        }
        // sub: canonical subtrahend, any minuend; add: one canonical operand
        {
            const u64 a = rnd(), c = rnd() % gl::P;
            if (glf::canon(gl::sub(a, c)) != gl::sub_ref(a % gl::P, c)) b++;
            if (glf::canon(gl::add(a, c)) != gl::add_ref(a % gl::P, c) || glf::canon(gl::add(c, a)) != gl::add_ref(a % gl::P, c)) b++;
            if (glf::canon(gl::mul_nc(gl::sub(a, c), f0)) != M(gl::sub_ref(a % gl::P, c), f0)) b++;
        }
    }
    // Planted violations, one per contract that can be broken: the comparison above must SEE them.  A non-canonical subtrahend
    // (p + 1 for 1) and two non-canonical summands must give something other than the field result; if they do not, the checks
    // above prove nothing, and that counts as a mismatch.
    {
        const u64 one_nc = gl::P + 1 + (x & 0), top = ~0ull - (x & 0);
        if (glf::canon(gl::sub(0, one_nc)) == gl::sub_ref(0, one_nc % gl::P)) b++;
        if (glf::canon(gl::add(top, top)) == gl::add_ref(top % gl::P, top % gl::P)) b++;
    }
    if (b) atomicAdd(bad, b);
}
}  // namespace p2k

int p2_selftest_lazy_device(uint64_t seed, size_t threads, int device) {
    if (hipSetDevice(device) != hipSuccess) return set_error("no such HIP device"), -P2_ERR_HIP;
    if (threads == 0 || threads > ((size_t)1 << 30)) return set_error("thread count out of range"), -P2_ERR_INVALID;
    Allocs mem;
    unsigned long long* d = nullptr;
    if (dalloc(mem, &d, 1) || hipMemset(d, 0, 8) != hipSuccess) return set_error("hipMalloc failed"), -P2_ERR_HIP;
    hipLaunchKernelGGL(p2k::k_selftest_lazy, dim3((u32)((threads + 255) / 256)), dim3(256), 0, 0, d, (u64)seed, threads);
    unsigned long long h = 0;
    if (hipError_t e = hipMemcpy(&h, d, 8, hipMemcpyDeviceToHost)) return set_error(hipGetErrorString(e)), -P2_ERR_HIP;
    return (int)std::min<unsigned long long>(h, 0x7FFFFFFF);
}
// ---- self-test of the transform arithmetic: gl::mul_nb (the branch-free two-sided correction, which only the NTT kernels use) and
// the register butterflies of kernels.h built on it
namespace p2k {
// 2^j for j = 33, 36, .., 63 -- the forward twiddles w_64^k = 8^k, k = 11..21 -- and m 2^(96 - j) with 1 <= m < 2^(j - 32): the
// product m 2^96 has zero low limbs and no carry, so the reduction borrows and does nothing else
__device__ __forceinline__ void borrow_pair(u64 r, u64& pw, u64& q) {
    const int j = 33 + 3 * (int)((r >> 56) % 11);
    const u64 m = 1 + (r & 0xFFFFFFFFFFFFull) % (((u64)1 << (j - 32)) - 1);
    pw = (u64)1 << j;
    q = m << (96 - j);
}
// stage A of ntt_r16_stage, written out with the textbook operations
__device__ void ref_r16_stage(u64* x, const u64* w, int A) {
    const int half = 8 >> A, base = 16 - 2 * half;
    for (int r = 0; r < 16; r++) {
        if (r & half) continue;
        const u64 u = x[r], v = x[r + half];
        x[r] = gl::add_ref(u, v);
        x[r + half] = gl::mul_ref(gl::sub_ref(u, v), w[base + r % half]);
    }
}
__global__ void k_selftest_ntt(unsigned long long* bad, u64 seed, size_t threads) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= threads) return;
    u64 x = (seed | 1) + 0x9E3779B97F4A7C15ull * (t + 1);
    auto step = [&]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    auto rnd = [&]() {  // lazy_draw's extremes, unreduced
        const u64 r = step();
        return lazy_draw(r, (u32)(r >> 40));
    };
    auto C = [](u64 v) { return v >= gl::P ? v - gl::P : v; };  // v mod p
    auto rndc = [&]() { return C(rnd()); };
    auto M = [&](u64 a, u64 b) { return gl::mul_ref(C(a), C(b)); };
    const bool odd = t & 1;
    unsigned long long b = 0;
    for (int i = 0; i < 16; i++) {
        // any u64 in, canonical out
        {
            const u64 a = rnd(), c = rnd();
            if (gl::mul_nb(a, c) != M(a, c)) b++;
        }
        // the borrow-only correction, in both operand orders: even lanes borrow, odd lanes draw at random, so that one wave holds
        // borrowing, carrying and plain lanes (the correction is built from two lane masks)
        u64 pw, q;
        borrow_pair(step(), pw, q);
        {
            const u64 ea = odd ? step() : pw, eb = odd ? step() : q, want = M(ea, eb);
            if (gl::mul_nb(ea, eb) != want || gl::mul_nb(eb, ea) != want) b++;
        }
        // the butterfly on canonical values, and with u - v a borrow operand against a power-of-two twiddle
        {
            const u64 u = rndc(), v = rndc(), w = rndc();
            if (gl::add(u, v) != gl::add_ref(u, v)) b++;
            if (gl::mul_nb(gl::sub(u, v), w) != gl::mul_ref(gl::sub_ref(u, v), w)) b++;
            const u64 ub = gl::add_ref(v, q), wb = odd ? w : pw;
            if (gl::add(ub, v) != gl::add_ref(ub, v)) b++;
            if (gl::mul_nb(gl::sub(ub, v), wb) != gl::mul_ref(q, wb)) b++;
        }
        // a 16-point register block through the four stages of a step: extremes, and in even lanes a borrow operand at one pair
        // of the first stage
        u64 xs[16], tw[15], got[16], want[16];
        for (int k = 0; k < 16; k++) xs[k] = rndc();
        for (int k = 0; k < 15; k++) tw[k] = rndc();
        if (!odd) {
            const int r = i & 7;
            tw[r] = pw;
            xs[r] = gl::add_ref(xs[r + 8], q);
        }
        for (int k = 0; k < 16; k++) got[k] = want[k] = xs[k];
        ntt_r16_stage<0>(got, tw);
        ntt_r16_stage<1>(got, tw);
        ntt_r16_stage<2>(got, tw);
        ntt_r16_stage<3>(got, tw);
        for (int A = 0; A < 4; A++) ref_r16_stage(want, tw, A);
        for (int k = 0; k < 16; k++) b += got[k] != want[k];
        // the last step's form skips the products by the first twiddle of every stage: equal to the plain form where those are 1
        tw[0] = tw[8] = tw[12] = tw[14] = 1;
        for (int k = 0; k < 16; k++) got[k] = want[k] = xs[k];
        ntt_r16_stage_m0<0>(got, tw);
        ntt_r16_stage_m0<1>(got, tw);
        ntt_r16_stage_m0<2>(got, tw);
        ntt_r16_stage_m0<3>(got, tw);
        for (int A = 0; A < 4; A++) ref_r16_stage(want, tw, A);
        for (int k = 0; k < 16; k++) b += got[k] != want[k];
        for (int k = 0; k < 16; k++) got[k] = xs[k];
        ntt_r16_stage<0>(got, tw);
        ntt_r16_stage<1>(got, tw);
        ntt_r16_stage<2>(got, tw);
        ntt_r16_stage<3>(got, tw);
        for (int k = 0; k < 16; k++) b += got[k] != want[k];
        // a later stage on its own, with the borrow operand at one of ITS pairs (stage A pairs r and r + (8 >> A))
        {
            const int A = 1 + i % 3, half = 8 >> A, base = 16 - 2 * half, r = ((i >> 2) & 1) * 2 * half + (i % half);
            for (int k = 0; k < 16; k++) got[k] = want[k];  // canonical values: what the stages above left
            if (!odd) {
                tw[base + r % half] = pw;
                got[r] = gl::add_ref(got[r + half], q);
            }
            for (int k = 0; k < 16; k++) want[k] = got[k];
            if (A == 1) ntt_r16_stage<1>(got, tw);
            if (A == 2) ntt_r16_stage<2>(got, tw);
            if (A == 3) ntt_r16_stage<3>(got, tw);
            ref_r16_stage(want, tw, A);
            for (int k = 0; k < 16; k++) b += got[k] != want[k];
        }
    }
    // The planted violation: a non-canonical subtrahend (p + 1 for 1) in the butterfly must give something other than the field
    // result; if it does not, the comparisons above prove nothing, and that counts as a mismatch.
    {
        const u64 one_nc = gl::P + 1 + (x & 0), w = (u64)1 << 33;
        if (gl::mul_nb(gl::sub(0, one_nc), w) == gl::mul_ref(gl::sub_ref(0, C(one_nc)), w)) b++;
    }
    if (b) atomicAdd(bad, b);
}
}  // namespace p2k

int p2_selftest_ntt_device(uint64_t seed, size_t threads, int device) {
    if (hipSetDevice(device) != hipSuccess) return set_error("no such HIP device"), -P2_ERR_HIP;
    if (threads == 0 || threads > ((size_t)1 << 30)) return set_error("thread count out of range"), -P2_ERR_INVALID;
    Allocs mem;
    unsigned long long* d = nullptr;
    if (dalloc(mem, &d, 1) || hipMemset(d, 0, 8) != hipSuccess) return set_error("hipMalloc failed"), -P2_ERR_HIP;
    hipLaunchKernelGGL(p2k::k_selftest_ntt, dim3((u32)((threads + 255) / 256)), dim3(256), 0, 0, d, (u64)seed, threads);
    unsigned long long h = 0;
    if (hipError_t e = hipMemcpy(&h, d, 8, hipMemcpyDeviceToHost)) return set_error(hipGetErrorString(e)), -P2_ERR_HIP;
    return (int)std::min<unsigned long long>(h, 0x7FFFFFFF);
}
// k_zeta_tabs and k_zeta_pows on their own: z = (z[0], z[1]) -> pows [4][2][n], the powers of z, g z, 1/z and 1/(g z) with g the
// primitive n-th root of unity (n a power of two up to 2^22)
int p2_gpu_zeta_pows(const uint64_t* z, size_t n, uint64_t* pows, int device) {
    if (n == 0 || n > ((size_t)1 << 22) || (n & (n - 1))) return set_error("n must be a power of two up to 2^22"), P2_ERR_INVALID;
    if (z[0] >= gl::P || z[1] >= gl::P) return set_error("z is not canonical"), P2_ERR_INVALID;
    if (int rc = pick_device(device)) return rc;
    int logn = 0;
    while (((size_t)1 << logn) < n) logn++;
    std::vector<u64> chal(CH_WORDS, 0);
    chal[CH_ZETA] = z[0];
    chal[CH_ZETA + 1] = z[1];
    Allocs mem;
    u64 *d_chal, *d_tab, *d_pows;
    if (upload(mem, &d_chal, chal.data(), chal.size()) || dalloc(mem, &d_tab, 4 * zeta_tab_words((u32)n)) || dalloc(mem, &d_pows, 8 * n)) return P2_ERR_HIP;
    hipLaunchKernelGGL(k_zeta_tabs, g1(ZT_LO + zeta_tab_hi((u32)n), 256, 1, 4), dim3(256), 0, 0, d_chal, d_tab, (u32)n, gl::root_of_unity(logn));
    HIPCHECK(hipGetLastError());
    hipLaunchKernelGGL(k_zeta_pows, g1(n, 256, 1, 4), dim3(256), 0, 0, d_tab, d_pows, (size_t)8 * n, (u32)n);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpy(pows, d_pows, 8 * n * 8, hipMemcpyDeviceToHost));
    return P2_OK;
}

// k_poseidon_states, k_partial_rounds and k_merged_middle on their own (tests): `count` states of 12 words, in place
static int states_in_place(void (*kernel)(u64*, size_t), const char* bad_shape, uint64_t* states, size_t count, int device) {
    return run_batch(bad_shape, count, on_host(device), {buf_inout(states, 12 * count)},
                     [&](const DevPtr* d, hipStream_t s) { hipLaunchKernelGGL(kernel, g1(count, 256), dim3(256), 0, s, d[0], count); });
}
static const char* states_count_shape(size_t count) { return count == 0 || count > (1u << 24) ? "count out of range" : nullptr; }
int p2_gpu_poseidon(uint64_t* states, size_t n_perm, int device) { return states_in_place(k_poseidon_states, nullptr, states, n_perm, device); }
int p2_gpu_partial_rounds(uint64_t* states, size_t count, int device) { return states_in_place(k_partial_rounds, states_count_shape(count), states, count, device); }
int p2_gpu_merged_middle(uint64_t* states, size_t count, int device) { return states_in_place(k_merged_middle, states_count_shape(count), states, count, device); }
// The three tree kernels on their own (tests): host arrays in, host arrays out, one launch each.
//   data [batch][min(active_cols, cols)][num_leaves] -> digests [batch][num_leaves][4]
int p2_gpu_hash_leaves(const uint64_t* data, size_t cols, size_t active_cols, size_t num_leaves, size_t batch, uint64_t* digests, int device) {
    if (cols == 0 || cols > (1u << 20) || num_leaves == 0 || batch == 0 || batch > 65535) return set_error("shape out of range"), P2_ERR_INVALID;
    if (int rc = pick_device(device)) return rc;
    const size_t stored = std::min(active_cols, cols), in_words = std::max<size_t>(stored, 1) * num_leaves;
    Allocs mem;
    u64 *d_in, *d_out;
    if (dalloc(mem, &d_in, batch * in_words) || dalloc(mem, &d_out, batch * num_leaves * 4)) return P2_ERR_HIP;
    HIPCHECK(hipMemcpy(d_in, data, batch * stored * num_leaves * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_hash_leaves, g1(num_leaves, 256, (u32)batch), dim3(256), 0, 0, d_in, (int)cols, (int)active_cols, num_leaves, stored * num_leaves, num_leaves,
                       d_out, num_leaves * 4);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpy(digests, d_out, batch * num_leaves * 32, hipMemcpyDeviceToHost));
    return P2_OK;
}
// p2_host_ecstep_constraints on the device: the <FBase> instantiation the quotient-side kernel runs
int p2_gpu_ecstep_constraints(const uint64_t* wires, size_t count, uint64_t* out, int device) {
    const char* bad = count == 0 || count > (1u << 20) || !wires || !out ? "count out of range" : nullptr;
    for (size_t i = 0; !bad && i < 80 * count; i++)
        if (wires[i] >= gl::P) bad = "p2_gpu_ecstep_constraints: non-canonical wire";
    return run_batch(bad, count, on_host(device), {buf_in(wires, 80 * count), buf_out(out, 40 * count)},
                     [&](const DevPtr* d, hipStream_t s) { hipLaunchKernelGGL(k_ecstep_selftest, g1(count, 256), dim3(256), 0, s, d[0], count, d[1]); });
}
//   child [batch][2 * num_parents][4] -> parent [batch][num_parents][4]
int p2_gpu_merkle_level(const uint64_t* child, size_t num_parents, size_t batch, uint64_t* parent, int device) {
    if (num_parents == 0 || batch == 0 || batch > 65535) return set_error("shape out of range"), P2_ERR_INVALID;
    if (int rc = pick_device(device)) return rc;
    const size_t stride = 8 * num_parents;  // the kernel strides children and parents alike (levels of one digest buffer)
    Allocs mem;
    u64 *d_in, *d_out;
    if (upload(mem, &d_in, (const u64*)child, batch * stride) || dalloc(mem, &d_out, batch * stride)) return P2_ERR_HIP;
    hipLaunchKernelGGL(k_merkle_level, g1(num_parents, 256, (u32)batch), dim3(256), 0, 0, d_in, d_out, num_parents, stride);
    HIPCHECK(hipGetLastError());
    for (size_t b = 0; b < batch; b++) HIPCHECK(hipMemcpy(parent + b * 4 * num_parents, d_out + b * stride, num_parents * 32, hipMemcpyDeviceToHost));
    return P2_OK;
}
//   vals [batch][2][len] (the two components of len extension values) -> digests [batch][len / arity][4]
int p2_gpu_hash_fri_leaves(const uint64_t* vals, size_t len, int arity, size_t batch, uint64_t* digests, int device) {
    const bool bad = arity < 1 || arity > 64 || len == 0 || len % (size_t)arity || batch == 0 || batch > 65535;
    const size_t leaves = bad ? 0 : len / (size_t)arity;
    return run_batch(bad ? "shape out of range" : nullptr, batch, on_host(device), {buf_in(vals, batch * 2 * len), buf_out(digests, batch * leaves * 4)},
                     [&](const DevPtr* d, hipStream_t s) {
                         hipLaunchKernelGGL(k_hash_fri_leaves, g1(leaves, 256, (u32)batch), dim3(256), 0, s, d[0], len, 2 * len, arity, d[1], leaves * 4);
                     });
}
// What the NTT / Merkle primitives need of a handle: a lane, the transform tables of one size and the allocations behind them.
struct PrimCtx {
    Allocs mem;  // declared first: freed after the lane's stream has gone
    Lane lane;
    Domain dom;
    u64* d_shift_inv_pows = nullptr;  // with_quotient: [8][n] (g w^j)^-i / n
    // the tables come from the loader's own builder (build_transform_tables); `arities` as the circuit's FRI schedule
    int init(int device, int degree_bits, const std::vector<u32>& arities = {}, bool with_quotient = false) {
        if (int rc = pick_device(device)) return rc;
        dom.logn = (u32)degree_bits;
        dom.arities = arities;
        HIPCHECK_AS("hipStreamCreate(&lane.stream)", lane.open(hipStreamDefault));
        HIPCHECK(raise_ntt_lds_limits());
        return build_transform_tables(lane, dom, mem, with_quotient ? &d_shift_inv_pows : nullptr);
    }
    ~PrimCtx() { if (lane.stream) (void)hipStreamSynchronize(lane.stream); }
};
int p2_gpu_intt(const uint64_t* values, size_t cols, int degree_bits, uint64_t* coeffs, int device) {
    if (degree_bits < 1 || degree_bits > 22) return set_error("degree_bits must be in 1..22"), P2_ERR_INVALID;
    PrimCtx ctx;
    if (int rc = ctx.init(device, degree_bits)) return rc;
    const size_t n = ctx.dom.n();
    u64 *d_in, *d_out, *d_scratch;
    if (upload(ctx.mem, &d_in, (const u64*)values, cols * n) || dalloc(ctx.mem, &d_out, cols * n) || dalloc(ctx.mem, &d_scratch, cols * n)) return P2_ERR_HIP;
    if (intt_cols(ctx.lane, ctx.dom, d_in, d_out, (u32)cols, 0, 1, d_scratch, 0)) return P2_ERR_HIP;
    HIPCHECK(hipStreamSynchronize(ctx.lane.stream));
    HIPCHECK(hipMemcpy(coeffs, d_out, cols * n * 8, hipMemcpyDeviceToHost));
    return P2_OK;
}
int p2_gpu_lde(const uint64_t* coeffs, size_t cols, int degree_bits, int rate_bits, uint64_t* lde, int device) {
    if (degree_bits < 1 || degree_bits > 22 || rate_bits != 3) return set_error("degree_bits must be in 1..22 and rate_bits 3"), P2_ERR_INVALID;
    PrimCtx ctx;
    if (int rc = ctx.init(device, degree_bits)) return rc;
    const size_t n = ctx.dom.n();
    u64 *d_in, *d_out;
    if (upload(ctx.mem, &d_in, (const u64*)coeffs, cols * n) || dalloc(ctx.mem, &d_out, cols * 8 * n)) return P2_ERR_HIP;
    if (lde_cols(ctx.lane, ctx.dom, d_in, 0, d_out, 0, (u32)cols, 0, 1)) return P2_ERR_HIP;
    HIPCHECK(hipStreamSynchronize(ctx.lane.stream));
    HIPCHECK(hipMemcpy(lde, d_out, cols * 8 * n * 8, hipMemcpyDeviceToHost));
    return P2_OK;
}
// lde_cols as step 9 of the prover calls it: the polynomials of FRI round `round` (n_r = n >> sum of arities[0..round)), `batch`
// proofs with their own strides.  coeffs: [batch] x in_batch_stride words holding [cols][n_r]; out: [batch] x out_batch_stride
// words, [cols][8 n_r] in bit-reversed order written (words between the proofs are left as they came in).
int p2_gpu_lde_round(const uint64_t* coeffs, size_t cols, int degree_bits, const uint32_t* arities, size_t n_rounds, size_t round, size_t batch,
                     size_t in_batch_stride, uint64_t* out, size_t out_batch_stride, int device) {
    if (degree_bits < 1 || degree_bits > 22 || cols == 0 || cols > 4096 || batch == 0 || batch > 65535 || n_rounds > 8 || (round && round >= n_rounds))
        return set_error("shape out of range"), P2_ERR_INVALID;
    u32 logn_r = (u32)degree_bits, left = (u32)degree_bits;
    std::vector<u32> ar(arities, arities + n_rounds);
    for (size_t r = 0; r < n_rounds; r++) {
        if (ar[r] == 0 || ar[r] >= left) return set_error("arities reduce the degree to nothing"), P2_ERR_INVALID;
        left -= ar[r];
        if (r < round) logn_r = left;
    }
    const size_t n_r = (size_t)1 << logn_r;
    if (in_batch_stride < cols * n_r || out_batch_stride < 8 * cols * n_r) return set_error("batch stride smaller than a proof's columns"), P2_ERR_INVALID;
    PrimCtx ctx;
    if (int rc = ctx.init(device, degree_bits, ar)) return rc;
    u64 *d_in, *d_out;
    if (upload(ctx.mem, &d_in, (const u64*)coeffs, batch * in_batch_stride) || upload(ctx.mem, &d_out, (const u64*)out, batch * out_batch_stride)) return P2_ERR_HIP;
    if (lde_cols(ctx.lane, ctx.dom, d_in, in_batch_stride, d_out, out_batch_stride, (u32)cols, (u32)round, (u32)batch)) return P2_ERR_HIP;
    HIPCHECK(hipStreamSynchronize(ctx.lane.stream));
    HIPCHECK(hipMemcpy(out, d_out, batch * out_batch_stride * 8, hipMemcpyDeviceToHost));
    return P2_OK;
}
// The prover's quotient inverse on its own (quotient_chunks): qvals [batch][chunks][8 n], the values of `chunks` polynomials of
// degree < 8 n on the LDE coset in bit-reversed order -> out [batch][chunks * 8][n], their coefficients n at a time.
int p2_gpu_quotient_chunks(const uint64_t* qvals, size_t chunks, int degree_bits, size_t batch, uint64_t* out, int device) {
    if (degree_bits < 2 || degree_bits > 22 || chunks == 0 || chunks > 64 || batch == 0 || batch > 65535) return set_error("shape out of range"), P2_ERR_INVALID;
    PrimCtx ctx;
    if (int rc = ctx.init(device, degree_bits, {}, true)) return rc;
    const size_t words = batch * chunks * (ctx.dom.n() << ctx.dom.rate_bits);
    u64 w8inv[8], qscale[8];
    quotient_chunk_scales(ctx.dom.logn, w8inv, qscale);
    u64 *d_q, *d_res, *d_coef, *d_w8inv, *d_qscale;
    if (upload(ctx.mem, &d_q, (const u64*)qvals, words) || dalloc(ctx.mem, &d_res, words) || dalloc(ctx.mem, &d_coef, words) ||
        upload(ctx.mem, &d_w8inv, w8inv, 8) || upload(ctx.mem, &d_qscale, qscale, 8))
        return P2_ERR_HIP;
    if (quotient_chunks(ctx.lane, ctx.dom, d_q, d_res, d_coef, (u32)chunks, words / batch, (u32)batch, ctx.d_shift_inv_pows, d_w8inv, d_qscale)) return P2_ERR_HIP;
    HIPCHECK(hipStreamSynchronize(ctx.lane.stream));
    HIPCHECK(hipMemcpy(out, d_coef, words * 8, hipMemcpyDeviceToHost));
    return P2_OK;
}
int p2_gpu_merkle_cap(const uint64_t* cols_major, size_t cols, size_t num_leaves, int cap_height, uint64_t* cap, int device) {
    return p2_gpu_merkle_cap_hasher(cols_major, cols, num_leaves, cap_height, P2_HASHER_POSEIDON, cap, device);
}
int p2_gpu_merkle_cap_hasher(const uint64_t* cols_major, size_t cols, size_t num_leaves, int cap_height, int hasher, uint64_t* cap, int device) {
    if (hasher != P2_HASHER_POSEIDON && hasher != P2_HASHER_KECCAK) return set_error("unknown hasher"), P2_ERR_INVALID;
    if (hasher == P2_HASHER_KECCAK && cols < 4) return set_error("Keccak trees hash every leaf: at least 4 columns"), P2_ERR_INVALID;
    u32 bits = 0;
    while (((size_t)1 << bits) < num_leaves) bits++;
    if (((size_t)1 << bits) != num_leaves || (int)bits < cap_height) return set_error("num_leaves must be a power of two >= 2^cap_height"), P2_ERR_INVALID;
    PrimCtx ctx;
    if (int rc = ctx.init(device, 4)) return rc;
    ctx.dom.cap_height = (u32)cap_height;
    ctx.dom.hasher = (u32)hasher;
    u64* d_in;
    Tree t;
    t.bits = bits;
    if (upload(ctx.mem, &d_in, (const u64*)cols_major, cols * num_leaves) || dalloc(ctx.mem, &t.dig, t.stride())) return P2_ERR_HIP;
    if (merkle_build(ctx.lane, ctx.dom, d_in, (u32)cols, (u32)cols, num_leaves, 0, t, 1)) return P2_ERR_HIP;
    HIPCHECK(hipStreamSynchronize(ctx.lane.stream));
    HIPCHECK(hipMemcpy(cap, t.dig + cap_off(t, (u32)cap_height), ((size_t)4 << cap_height) * 8, hipMemcpyDeviceToHost));
    return P2_OK;
}

// ---- stand-alone Merkle trees (kernels_merkle.h, merkle_host.h)
// A tree independent of any circuit: every digest level on the device in merkle_build's layout; the leaves are not kept.
struct MerkleTreeHandle {
    int device = 0;
    u32 leaf_len = 0, cap_height = 0;
    Tree t;
    Allocs mem;      // (the memory first: freed after the stream and the event have gone)
    Allocs scratch;  // the column-major copy of the leaves: needed until the build has run
    // updates (mt_update): a grow-only block for keys, node versions and the sort, never freed under a running kernel, and the
    // hash counter and the bad-item flag of the last update
    DevBuf<u64> upd;
    u64* upd_ctl = nullptr;  // [0] the counter, [1] the flag (its low word)
    Lane lane;               // the stream of the host forms
    Event built;             // recorded behind the last kernel of the build and of every update, on whichever stream ran it
    void drop_scratch(bool wait) {
        if (scratch.empty() || (wait ? hipEventSynchronize(built) : hipEventQuery(built)) != hipSuccess) return;
        scratch.clear();
    }
    ~MerkleTreeHandle() {
        if (built) (void)hipEventSynchronize(built);
        if (lane.stream) (void)hipStreamSynchronize(lane.stream);
    }
    u32 depth() const { return t.bits - cap_height; }
};
// row-major leaves -> column-major, then merkle_build (leaf digests and the levels up to the cap), on `stream`; records `built`
static int mt_transpose(Lane& L, const u64* d_leaves, size_t num_leaves, u32 leaf_len, u64* d_cols) {
    LAUNCH(L, "mt_transpose", k_mt_transpose, dim3((u32)((num_leaves + 31) / 32), (leaf_len + 31) / 32), dim3(256), 0, d_leaves, num_leaves, leaf_len, d_cols);
    return 0;
}
static int mt_build(MerkleTreeHandle& T, const u64* d_leaves, hipStream_t stream) {
    Lane L;
    L.stream = stream;
    Domain D;
    D.cap_height = T.cap_height;
    const size_t leaves = (size_t)1 << T.t.bits;
    u64* d_cols;
    if (dalloc(T.scratch, &d_cols, leaves * T.leaf_len) || mt_transpose(L, d_leaves, leaves, T.leaf_len, d_cols)) return P2_ERR_HIP;
    if (merkle_build(L, D, d_cols, T.leaf_len, T.leaf_len, leaves, 0, T.t, 1)) return P2_ERR_HIP;
    HIPCHECK(hipEventRecord(T.built, stream));
    return P2_OK;
}
static int mt_new(const u64* leaves, bool on_device, size_t num_leaves, size_t leaf_len, int cap_height, int device, hipStream_t stream, void** tree) {
    if (!tree) return set_error("null tree pointer"), P2_ERR_INVALID;
    *tree = nullptr;
    const u32 bits = mt::check_shape(num_leaves, leaf_len, cap_height);  // throws: P2_ERR_INVALID
    if (!leaves) return set_error("null leaves"), P2_ERR_INVALID;
    const size_t words = num_leaves * leaf_len;
    if (!on_device) {
        const size_t bad = mt::first_non_canonical(leaves, words);
        if (bad != words) return set_error("word " + std::to_string(bad % leaf_len) + " of leaf " + std::to_string(bad / leaf_len) + " is not below p"), P2_ERR_INVALID;
    }
    if (int rc = pick_device(device)) return rc;
    std::unique_ptr<MerkleTreeHandle> T(new MerkleTreeHandle());
    T->device = device;
    T->leaf_len = (u32)leaf_len;
    T->cap_height = (u32)cap_height;
    T->t.bits = bits;
    size_t free_b = 0, total_b = 0;
    HIPCHECK(hipMemGetInfo(&free_b, &total_b));
    const size_t need = 8 * T->t.stride() + 8 * words + (on_device ? 0 : 8 * words);  // digests, the column-major copy, the upload
    if (need > free_b) return set_error("the tree needs " + std::to_string(need) + " bytes of device memory, " + std::to_string(free_b) + " are free"), P2_ERR_INVALID;
    HIPCHECK_AS("hipStreamCreateWithFlags(&T->lane.stream, hipStreamNonBlocking)", T->lane.open(hipStreamNonBlocking));
    HIPCHECK_AS("hipEventCreateWithFlags(&T->built, hipEventDisableTiming)", T->built.create(hipEventDisableTiming));
    if (dalloc(T->mem, &T->t.dig, T->t.stride())) return P2_ERR_HIP;
    if (on_device) {
        if (int rc = mt_build(*T, leaves, stream)) return rc;
    } else {
        Allocs tmp;  // the uploaded leaves go when the build has run
        u64* d_leaves;
        if (upload(tmp, &d_leaves, leaves, words)) return P2_ERR_HIP;
        if (int rc = mt_build(*T, d_leaves, T->lane.stream)) return rc;
        HIPCHECK(hipStreamSynchronize(T->lane.stream));
        T->drop_scratch(true);
    }
    *tree = T.release();
    return P2_OK;
}
static int mt_handle(void* tree, MerkleTreeHandle** T) {
    if (!tree) return set_error("null tree handle"), P2_ERR_INVALID;
    *T = (MerkleTreeHandle*)tree;
    HIPCHECK(hipSetDevice((*T)->device));
    (*T)->drop_scratch(false);
    return P2_OK;
}
static int mt_paths(MerkleTreeHandle& T, const u64* d_indices, size_t n, u64* d_out, size_t out_stride, int* d_status, hipStream_t stream) {
    if (n == 0) return P2_OK;
    if (!d_indices || !d_status || (T.depth() && !d_out)) return set_error("null argument"), P2_ERR_INVALID;
    if (out_stride < 4 * (size_t)T.depth()) return set_error("out_stride_words is smaller than a path (" + std::to_string(4 * T.depth()) + " words)"), P2_ERR_INVALID;
    HIPCHECK(hipStreamWaitEvent(stream, T.built, 0));
    const size_t threads = n * std::max<u32>(T.depth(), 1);
    hipLaunchKernelGGL(k_mt_paths, g1(threads, 256), dim3(256), 0, stream, T.t.dig, T.t.bits, T.depth(), d_indices, n, d_out, out_stride, d_status);
    HIPCHECK(hipGetLastError());
    return P2_OK;
}
// ---- ordered leaf updates (kernels_merkle_update.h): validate and hash the leaves, sort the keys, then one launch per level.
// trace = d_sib != nullptr.  Everything is enqueued on `stream` behind the handle's event, which is recorded again at the end.
static int mt_update_launch(MerkleTreeHandle& T, const u64* d_indices, const u64* d_leaves, size_t k, u64* d_sib, size_t sib_stride, u64* d_root, size_t root_stride,
                            int* d_status, hipStream_t stream, u64* keys_a, u64* keys_b, u64* v_a, u64* v_b, void* sort_tmp, size_t sort_bytes) {
    const u32 bits = T.t.bits, depth = T.depth();
    u64* counter = T.upd_ctl;
    u32* flag = (u32*)(T.upd_ctl + 1);
    const dim3 grid = g1(k, 256), block(256);
    HIPCHECK(hipMemsetAsync(T.upd_ctl, 0, 16, stream));
    hipLaunchKernelGGL(k_mu_leaves, grid, block, 0, stream, d_indices, d_leaves, T.leaf_len, bits, k, keys_a, v_a, d_status, flag);
    HIPCHECK(hipGetLastError());
    HIPCHECK(rocprim::radix_sort_keys(sort_tmp, sort_bytes, keys_a, keys_b, k, 0u, 32u + bits, stream));
    if (!d_sib || depth == 0) {
        hipLaunchKernelGGL(k_mu_fast_leaf, grid, block, 0, stream, keys_b, v_a, k, T.t.dig, flag);
        for (u32 l = 1; l <= depth; l++)
            hipLaunchKernelGGL(k_mu_fast_level, grid, block, 0, stream, keys_b, k, l, T.t.dig + level_off(bits, l - 1), T.t.dig + level_off(bits, l), flag, counter);
        if (d_sib && d_root) hipLaunchKernelGGL(k_mu_roots, grid, block, 0, stream, v_a, k, d_root, root_stride, flag);
    } else {
        hipLaunchKernelGGL(k_mu_gather, g1(k * depth, 256), block, 0, stream, T.t.dig, bits, depth, d_indices, k, d_sib, sib_stride, flag);
        u64 *a_in = keys_b, *a_out = keys_a, *v_in = v_a, *v_out = v_b;
        for (u32 l = 0; l < depth; l++) {
            hipLaunchKernelGGL(k_mu_step, grid, block, 0, stream, a_in, v_in, k, l, l == 0 ? 1u : 0u, l + 1 == depth ? 1u : 0u, a_out, v_out, T.t.dig, bits, d_sib, sib_stride,
                               d_root, root_stride, flag, counter);
            std::swap(a_in, a_out);
            if (l == 0) v_in = v_b, v_out = v_a;
            else std::swap(v_in, v_out);
        }
    }
    HIPCHECK(hipGetLastError());
    return P2_OK;
}
static int mt_update(MerkleTreeHandle& T, const u64* d_indices, const u64* d_leaves, size_t k, u64* d_sib, size_t sib_stride, u64* d_root, size_t root_stride, int* d_status,
                     hipStream_t stream) {
    if (k == 0) return P2_OK;
    if (!d_indices || !d_leaves || !d_status) return set_error("null argument"), P2_ERR_INVALID;
    if (k >> 32) return set_error("an update takes fewer than 2^32 items"), P2_ERR_INVALID;
    if (d_sib && sib_stride < 4 * (size_t)T.depth()) return set_error("sib_stride_words is smaller than a path (" + std::to_string(4 * T.depth()) + " words)"), P2_ERR_INVALID;
    if (d_sib && d_root && root_stride < 4) return set_error("root_stride_words is smaller than a hash (4 words)"), P2_ERR_INVALID;
    size_t sort_bytes = 0;
    HIPCHECK(rocprim::radix_sort_keys(nullptr, sort_bytes, (u64*)nullptr, (u64*)nullptr, k, 0u, 32u + T.t.bits, stream));
    const size_t sort_off = (10 * k + 31) & ~(size_t)31;  // keys A | keys B | v A | v B, then the sort's block on a 256-byte boundary
    const size_t need = sort_off + (sort_bytes + 7) / 8;
    if (!T.upd_ctl && dalloc(T.mem, &T.upd_ctl, 2)) return P2_ERR_HIP;
    if (need * 8 > T.upd.bytes()) {  // grow: the last update may still be reading the old block
        HIPCHECK(hipEventSynchronize(T.built));
        HIPCHECK_AS("hipMalloc((void**)&T.upd, need * 8)", T.upd.alloc(need));  // exactly `need` words, the old block freed first
    }
    HIPCHECK(hipStreamWaitEvent(stream, T.built, 0));
    const int rc = mt_update_launch(T, d_indices, d_leaves, k, d_sib, sib_stride, d_root, root_stride, d_status, stream, T.upd, T.upd + k, T.upd + 2 * k, T.upd + 6 * k,
                                    T.upd + sort_off, sort_bytes);
    HIPCHECK(hipEventRecord(T.built, stream));  // also behind a launch that failed half-way: what was enqueued still runs
    return rc;
}
static int mt_verify(const uint64_t* leaves, size_t leaf_len, const uint64_t* indices, const uint64_t* siblings, size_t depth, const uint64_t* cap, int cap_height, size_t n,
                     int* status, Where w) {
    const bool bad = leaf_len < 1 || leaf_len > 0xFFFFFFFFull || cap_height < 0 || cap_height > 16 || depth + (size_t)cap_height > 32;
    return run_batch(bad ? "leaf_len >= 1, cap_height 0 to 16, siblings + cap_height at most 32" : nullptr, n, w,
                     {buf_in(leaves, n * leaf_len), buf_in(indices, n), buf_in(siblings, n * 4 * depth), buf_in(cap, bad ? 0 : (size_t)4 << cap_height), buf_out(status, n)},
                     [&](const DevPtr* d, hipStream_t s) {
                         hipLaunchKernelGGL(k_mt_verify, g1(n, 64), dim3(64), 0, s, d[0], (u32)leaf_len, d[1], d[2], (u32)depth, d[3], (u32)cap_height, n, d[4]);
                     });
}

int p2_merkle_tree_new(const uint64_t* leaves, size_t num_leaves, size_t leaf_len, int cap_height, int device, void** tree) {
    return guarded_rc([&] { return mt_new((const u64*)leaves, false, num_leaves, leaf_len, cap_height, device, nullptr, tree); });
}
int p2_merkle_tree_new_device(const uint64_t* d_leaves, size_t num_leaves, size_t leaf_len, int cap_height, int device, void* stream, void** tree) {
    return guarded_rc([&] { return mt_new((const u64*)d_leaves, true, num_leaves, leaf_len, cap_height, device, (hipStream_t)stream, tree); });
}
void p2_merkle_tree_free(void* tree) {
    if (!tree) return;
    (void)hipSetDevice(((MerkleTreeHandle*)tree)->device);
    delete (MerkleTreeHandle*)tree;
}
int p2_merkle_tree_cap(void* tree, uint64_t* cap, size_t cap_words) {
    return guarded_rc([&]() -> int {
        MerkleTreeHandle* T;
        if (int rc = mt_handle(tree, &T)) return rc;
        const size_t words = (size_t)4 << T->cap_height;
        if (!cap || cap_words < words) return set_error("the cap holds " + std::to_string(words) + " words"), P2_ERR_INVALID;
        HIPCHECK(hipEventSynchronize(T->built));
        T->drop_scratch(true);
        HIPCHECK(hipMemcpy(cap, T->t.dig + cap_off(T->t, T->cap_height), words * 8, hipMemcpyDeviceToHost));
        return (int)P2_OK;
    });
}
int p2_merkle_tree_prove_batch(void* tree, const uint64_t* indices, size_t n, uint64_t* siblings) {
    return guarded_rc([&]() -> int {
        MerkleTreeHandle* T;
        if (int rc = mt_handle(tree, &T)) return rc;
        if (n == 0) return (int)P2_OK;
        if (!indices || (T->depth() && !siblings)) return set_error("null argument"), P2_ERR_INVALID;
        for (size_t i = 0; i < n; i++)
            if (indices[i] >> T->t.bits) return set_error("leaf index " + std::to_string(indices[i]) + " (entry " + std::to_string(i) + ") is not below num_leaves"), P2_ERR_INVALID;
        const size_t stride = 4 * (size_t)T->depth();
        Allocs tmp;
        u64 *d_idx, *d_out;
        int* d_st;
        if (upload(tmp, &d_idx, (const u64*)indices, n) || dalloc(tmp, &d_out, n * stride) || dalloc(tmp, &d_st, n)) return P2_ERR_HIP;
        if (int rc = mt_paths(*T, d_idx, n, d_out, stride, d_st, T->lane.stream)) return rc;
        HIPCHECK(hipStreamSynchronize(T->lane.stream));
        if (stride) HIPCHECK(hipMemcpy(siblings, d_out, n * stride * 8, hipMemcpyDeviceToHost));
        return (int)P2_OK;
    });
}
int p2_merkle_tree_prove_batch_device(void* tree, const uint64_t* d_indices, size_t n, uint64_t* d_out, size_t out_stride_words, int* d_status, void* stream) {
    return guarded_rc([&]() -> int {
        MerkleTreeHandle* T;
        if (int rc = mt_handle(tree, &T)) return rc;
        return mt_paths(*T, (const u64*)d_indices, n, (u64*)d_out, out_stride_words, d_status, (hipStream_t)stream);
    });
}
int p2_merkle_tree_update(void* tree, const uint64_t* indices, const uint64_t* leaves, size_t k, uint64_t* siblings, uint64_t* root_after) {
    return guarded_rc([&]() -> int {
        MerkleTreeHandle* T;
        if (int rc = mt_handle(tree, &T)) return rc;
        if (k == 0) return (int)P2_OK;
        if (!indices || !leaves) return set_error("null argument"), P2_ERR_INVALID;
        const std::string bad = mt::first_bad_item((const u64*)indices, (const u64*)leaves, k, (size_t)1 << T->t.bits, T->leaf_len);
        if (!bad.empty()) return set_error(bad), P2_ERR_INVALID;
        const bool trace = siblings || root_after;
        const size_t stride = 4 * (size_t)T->depth();
        Allocs tmp;
        u64 *d_idx, *d_leaves, *d_sib = nullptr, *d_root = nullptr;
        int* d_st;
        if (upload(tmp, &d_idx, (const u64*)indices, k) || upload(tmp, &d_leaves, (const u64*)leaves, k * T->leaf_len) || dalloc(tmp, &d_st, k)) return P2_ERR_HIP;
        if (trace && (dalloc(tmp, &d_sib, k * stride) || dalloc(tmp, &d_root, 4 * k))) return P2_ERR_HIP;
        const int rc = mt_update(*T, d_idx, d_leaves, k, d_sib, stride, d_root, 4, d_st, T->lane.stream);
        HIPCHECK(hipStreamSynchronize(T->lane.stream));  // before tmp goes, whatever rc says
        if (rc) return rc;
        if (siblings && stride) HIPCHECK(hipMemcpy(siblings, d_sib, k * stride * 8, hipMemcpyDeviceToHost));
        if (root_after) HIPCHECK(hipMemcpy(root_after, d_root, k * 32, hipMemcpyDeviceToHost));
        return (int)P2_OK;
    });
}
int p2_merkle_tree_update_device(void* tree, const uint64_t* d_indices, const uint64_t* d_leaves, size_t k, uint64_t* d_siblings, size_t sib_stride_words,
                                 uint64_t* d_root_after, size_t root_stride_words, int* d_status, void* stream) {
    return guarded_rc([&]() -> int {
        MerkleTreeHandle* T;
        if (int rc = mt_handle(tree, &T)) return rc;
        return mt_update(*T, (const u64*)d_indices, (const u64*)d_leaves, k, (u64*)d_siblings, sib_stride_words, (u64*)d_root_after, root_stride_words, d_status,
                         (hipStream_t)stream);
    });
}
int p2_merkle_tree_last_update_hashes(void* tree, uint64_t* hashes) {
    return guarded_rc([&]() -> int {
        MerkleTreeHandle* T;
        if (int rc = mt_handle(tree, &T)) return rc;
        if (!hashes) return set_error("null argument"), P2_ERR_INVALID;
        *hashes = 0;
        if (!T->upd_ctl) return (int)P2_OK;
        HIPCHECK(hipEventSynchronize(T->built));
        HIPCHECK(hipMemcpy(hashes, T->upd_ctl, 8, hipMemcpyDeviceToHost));
        return (int)P2_OK;
    });
}
int p2_merkle_verify_batch(const uint64_t* leaves, size_t leaf_len, const uint64_t* indices, const uint64_t* siblings, size_t depth, const uint64_t* cap, int cap_height,
                           size_t n, int* status, int device) {
    return mt_verify(leaves, leaf_len, indices, siblings, depth, cap, cap_height, n, status, on_host(device));
}
int p2_merkle_verify_batch_device(const uint64_t* d_leaves, size_t leaf_len, const uint64_t* d_indices, const uint64_t* d_siblings, size_t depth, const uint64_t* d_cap,
                                  int cap_height, size_t n, int* d_status, int device, void* stream) {
    return mt_verify(d_leaves, leaf_len, d_indices, d_siblings, depth, d_cap, cap_height, n, d_status, on_device(device, stream));
}
// Bench hook (tools/gpu_merkle_bench.py): one tree build on buffers the caller owns.  d_dig: 8 * num_leaves words, the level
// layout.  with_transpose = 0: merkle_build on d_scratch, column-major [leaf_len][num_leaves] (the build of p2_gpu_merkle_cap);
// otherwise k_mt_transpose of the row-major d_leaves into d_scratch first (the build of p2_merkle_tree_new).
int p2_gpu_merkle_build_device(const uint64_t* d_leaves, size_t num_leaves, size_t leaf_len, int cap_height, int with_transpose, uint64_t* d_scratch, uint64_t* d_dig,
                               int device, void* stream) {
    return guarded_rc([&]() -> int {
        const u32 bits = mt::check_shape(num_leaves, leaf_len, cap_height);
        if ((with_transpose && !d_leaves) || !d_scratch || !d_dig) return set_error("null argument"), P2_ERR_INVALID;
        if (int rc = pick_device(device)) return rc;
        Lane L;
        L.stream = (hipStream_t)stream;
        Domain D;
        D.cap_height = (u32)cap_height;
        Tree t;
        t.bits = bits;
        t.dig = (u64*)d_dig;
        if (with_transpose && mt_transpose(L, (const u64*)d_leaves, num_leaves, (u32)leaf_len, (u64*)d_scratch)) return P2_ERR_HIP;
        return merkle_build(L, D, (const u64*)d_scratch, (u32)leaf_len, (u32)leaf_len, num_leaves, 0, t, 1);
    });
}

// ---- sparse keyed Merkle trees (kernels_merkle_map.h; the definition and the host twin are mt::HostMap, merkle_host.h)
// An immutable map on the device: per level the ascending ids of the non-empty nodes and their digests, the E_l table, the
// dense cap, and the keys and values in key order.  The rules are MerkleTreeHandle's: owned resources, one event behind the
// build that every later call waits on, a memory check in front of the allocations.
struct MerkleMapHandle {
    int device = 0;
    u32 D = 0, h = 0, V = 0;
    size_t n = 0;
    std::vector<size_t> level_n;  // [depth + 1]: the non-empty nodes of every level
    Allocs mem;                   // (the memory first: freed after the stream and the event have gone)
    Allocs scratch;               // positions, the b sort, the (entry, child) ping-pong: needed until the build has run
    u64 *keys = nullptr, *vals = nullptr, *ids = nullptr, *dig = nullptr, *empties = nullptr, *cap = nullptr;
    u64* ctl = nullptr;  // [0] the lowest bad (entry, kind), [1] the hash counter, then the 65-bin histogram (u32)
    MapLevel* levels = nullptr;
    Lane lane;    // the stream of the host forms
    Event built;  // recorded behind the last kernel of the build, on whichever stream ran it
    void drop_scratch(bool wait) {
        if (scratch.empty() || (wait ? hipEventSynchronize(built) : hipEventQuery(built)) != hipSuccess) return;
        scratch.clear();
    }
    ~MerkleMapHandle() {
        if (built) (void)hipEventSynchronize(built);
        if (lane.stream) (void)hipStreamSynchronize(lane.stream);
    }
    u32 depth() const { return D - h; }
};
static const size_t MM_CTL_WORDS = 2 + 33;
static int mm_refuse(const std::string& what, size_t need, size_t free_b) {
    return set_error(what + " needs " + std::to_string(need) + " bytes of device memory, " + std::to_string(free_b) + " are free"), P2_ERR_INVALID;
}
// Everything on `st`.  One synchronisation: the histogram (every level's size) and the bad-entry flag come back together.
static int mm_build(MerkleMapHandle& T, const u64* d_keys, const u64* d_values, hipStream_t st) {
    const size_t n = T.n;
    const u32 depth = T.depth();
    const dim3 block(256);
    Hash4 E[65];
    mt::map_empty_digests(E);
    std::vector<u64> ctl0(MM_CTL_WORDS, 0);
    ctl0[0] = ~0ull;
    if (dalloc(T.mem, &T.empties, 65 * 4) || dalloc(T.mem, &T.ctl, MM_CTL_WORDS) || dalloc(T.mem, &T.cap, (size_t)4 << T.h) || dalloc(T.mem, &T.levels, depth + 1))
        return P2_ERR_HIP;
    HIPCHECK(hipMemcpy(T.empties, E, sizeof(E), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(T.ctl, ctl0.data(), MM_CTL_WORDS * 8, hipMemcpyHostToDevice));
    unsigned long long* bad = (unsigned long long*)T.ctl;
    u64* counter = T.ctl + 1;
    u32* hist = (u32*)(T.ctl + 2);
    T.level_n.assign(depth + 1, 0);
    std::vector<MapLevel> levels(depth + 1, MapLevel{nullptr, nullptr, 0});
    if (n) {
        size_t free_b = 0, total_b = 0, sort_a = 0, sort_b = 0;
        HIPCHECK(rocprim::radix_sort_pairs(nullptr, sort_a, (const u64*)nullptr, (u64*)nullptr, (const u32*)nullptr, (u32*)nullptr, n, 0u, T.D, st));
        HIPCHECK(rocprim::radix_sort_pairs(nullptr, sort_b, (const u32*)nullptr, (u32*)nullptr, (const u32*)nullptr, (u32*)nullptr, n, 0u, 7u, st));
        const size_t sort_bytes = std::max(sort_a, sort_b);
        HIPCHECK(hipMemGetInfo(&free_b, &total_b));
        const size_t need1 = 8 * n * (1 + T.V) + 10 * 4 * n + sort_bytes;  // keys and values in key order; ten u32 arrays; the sorts' block
        if (need1 > free_b) return mm_refuse("sorting the map", need1, free_b);
        u32 *pos_a, *pos_b, *bkey, *bkey_s, *idx, *order, *ent[2], *child[2];
        char* sort_tmp;
        if (dalloc(T.mem, &T.keys, n) || dalloc(T.mem, &T.vals, n * T.V) || dalloc(T.scratch, &pos_a, n) || dalloc(T.scratch, &pos_b, n) || dalloc(T.scratch, &bkey, n) ||
            dalloc(T.scratch, &bkey_s, n) || dalloc(T.scratch, &idx, n) || dalloc(T.scratch, &order, n) || dalloc(T.scratch, &ent[0], n) || dalloc(T.scratch, &ent[1], n) ||
            dalloc(T.scratch, &child[0], n) || dalloc(T.scratch, &child[1], n) || dalloc(T.scratch, &sort_tmp, sort_bytes))
            return P2_ERR_HIP;
        const dim3 grid = g1(n, 256);
        hipLaunchKernelGGL(k_mm_check, grid, block, 0, st, d_keys, d_values, n, T.D, T.V, pos_a, bad);
        HIPCHECK(hipGetLastError());
        HIPCHECK(rocprim::radix_sort_pairs((void*)sort_tmp, sort_a, d_keys, T.keys, (const u32*)pos_a, pos_b, n, 0u, T.D, st));
        hipLaunchKernelGGL(k_mm_diff, grid, block, 0, st, T.keys, pos_b, n, bkey, idx, hist, bad);
        HIPCHECK(hipGetLastError());
        HIPCHECK(rocprim::radix_sort_pairs((void*)sort_tmp, sort_b, (const u32*)bkey, bkey_s, (const u32*)idx, order, n, 0u, 7u, st));
        if (T.V) hipLaunchKernelGGL(k_mm_gather, g1(n * T.V, 256), block, 0, st, d_values, pos_b, n, T.V, T.vals);
        HIPCHECK(hipGetLastError());
        std::vector<u64> ctl(MM_CTL_WORDS);
        HIPCHECK(hipMemcpyAsync(ctl.data(), T.ctl, MM_CTL_WORDS * 8, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipStreamSynchronize(st));
        if (ctl[0] != ~0ull) return set_error(mt::map_bad_message((size_t)(ctl[0] >> 2), (int)(ctl[0] & 3))), P2_ERR_INVALID;
        const u32* h_hist = (const u32*)(ctl.data() + 2);
        size_t above = 0, total = 0;
        for (u32 l = 65; l-- > 0;) {  // n_l = #{i : b_i >= l}
            above += h_hist[l];
            if (l <= depth) T.level_n[l] = above, total += above;
        }
        if (T.level_n[0] != n) return set_error("the level histogram does not add up to the entries"), P2_ERR_HIP;
        HIPCHECK(hipMemGetInfo(&free_b, &total_b));
        const size_t need2 = 8 * (total - n) + 32 * total;  // the ids above the leaves, every digest
        if (need2 > free_b) return mm_refuse("the map's " + std::to_string(total) + " nodes", need2, free_b);
        if (dalloc(T.mem, &T.ids, total - n) || dalloc(T.mem, &T.dig, 4 * total)) return P2_ERR_HIP;
        size_t off = 0;
        for (u32 l = 0; l <= depth; l++) {
            levels[l] = MapLevel{l ? T.ids + (off - n) : T.keys, T.dig + 4 * off, T.level_n[l]};
            off += T.level_n[l];
        }
        auto group = [&](u32 l) { return l + 1 <= depth ? order + T.level_n[l + 1] : order; };  // the entries with b == l (used for l < depth only)
        auto group_n = [&](u32 l) { return l + 1 <= depth ? T.level_n[l] - T.level_n[l + 1] : (size_t)0; };
        hipLaunchKernelGGL(k_mm_leaves, grid, block, 0, st, T.vals, n, T.V, (u64*)levels[0].dig, depth >= 1 ? 1u : 0u, bkey, group(0), group_n(0), ent[0], child[0]);
        HIPCHECK(hipGetLastError());
        for (u32 l = 0; l < depth; l++) {
            const u32 in = l & 1, place = l + 2 <= depth ? 1u : 0u;
            hipLaunchKernelGGL(k_mm_level, g1(T.level_n[l + 1], 256), block, 0, st, l, levels[l].ids, levels[l].dig, levels[l].n, ent[in], child[in], T.level_n[l + 1],
                               T.empties + 4 * l, (u64*)levels[l + 1].ids, (u64*)levels[l + 1].dig, place, bkey, group(l + 1), group_n(l + 1), ent[in ^ 1], child[in ^ 1],
                               counter);
        }
        HIPCHECK(hipGetLastError());
    }
    HIPCHECK(hipMemcpy(T.levels, levels.data(), levels.size() * sizeof(MapLevel), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_mm_cap, g1((size_t)1 << T.h, 256), block, 0, st, levels[depth].ids, levels[depth].dig, levels[depth].n, T.empties + 4 * depth, 1u << T.h, T.cap);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(T.built, st));
    return P2_OK;
}
static int mm_new(const u64* keys, const u64* values, bool on_device, size_t n, size_t value_len, int key_bits, int cap_height, int device, hipStream_t stream, void** map) {
    if (!map) return set_error("null map pointer"), P2_ERR_INVALID;
    *map = nullptr;
    mt::map_check_shape(key_bits, cap_height, value_len);  // throws: P2_ERR_INVALID
    if (n && (!keys || (value_len && !values))) return set_error("null argument"), P2_ERR_INVALID;
    if (n >> 32) return set_error("a map takes fewer than 2^32 entries"), P2_ERR_INVALID;
    if (int rc = pick_device(device)) return rc;
    std::unique_ptr<MerkleMapHandle> T(new MerkleMapHandle());
    T->device = device;
    T->D = (u32)key_bits, T->h = (u32)cap_height, T->V = (u32)value_len, T->n = n;
    HIPCHECK_AS("hipStreamCreateWithFlags(&T->lane.stream, hipStreamNonBlocking)", T->lane.open(hipStreamNonBlocking));
    HIPCHECK_AS("hipEventCreateWithFlags(&T->built, hipEventDisableTiming)", T->built.create(hipEventDisableTiming));
    if (on_device) {
        if (int rc = mm_build(*T, keys, values, stream)) return (void)hipStreamSynchronize(stream), rc;  // what was enqueued has run before the handle goes
    } else {
        size_t free_b = 0, total_b = 0;
        HIPCHECK(hipMemGetInfo(&free_b, &total_b));
        if (8 * n * (1 + value_len) > free_b) return mm_refuse("uploading the entries", 8 * n * (1 + value_len), free_b);
        Allocs tmp;  // the uploaded entries go when the build has run
        u64 *d_keys, *d_values;
        if (upload(tmp, &d_keys, keys, n) || upload(tmp, &d_values, values, n * value_len)) return P2_ERR_HIP;
        const int rc = mm_build(*T, d_keys, d_values, T->lane.stream);
        HIPCHECK(hipStreamSynchronize(T->lane.stream));  // before tmp goes, whatever rc says
        if (rc) return rc;
        T->drop_scratch(true);
    }
    *map = T.release();
    return P2_OK;
}
static int mm_handle(void* map, MerkleMapHandle** T) {
    if (!map) return set_error("null map handle"), P2_ERR_INVALID;
    *T = (MerkleMapHandle*)map;
    HIPCHECK(hipSetDevice((*T)->device));
    (*T)->drop_scratch(false);
    return P2_OK;
}
static int mm_get(MerkleMapHandle& T, const u64* d_keys, size_t nq, u64* d_out, size_t stride, size_t present_off, size_t value_off, size_t sib_off, int* d_status,
                  hipStream_t stream) {
    if (nq == 0) return P2_OK;
    if (!d_keys || !d_out || !d_status) return set_error("null argument"), P2_ERR_INVALID;
    const size_t sib_words = 4 * (size_t)T.depth();
    if (present_off >= stride || value_off > stride || T.V > stride - value_off || sib_off > stride || sib_words > stride - sib_off)
        return set_error("a row of out_stride_words words does not hold presence, " + std::to_string(T.V) + " value words and " + std::to_string(sib_words) +
                         " sibling words at these offsets"),
               P2_ERR_INVALID;
    HIPCHECK(hipStreamWaitEvent(stream, T.built, 0));
    hipLaunchKernelGGL(k_mm_get, g1(nq * (T.depth() + 1), 256), dim3(256), 0, stream, T.levels, T.vals, T.empties, T.D, T.depth(), T.V, d_keys, nq, d_out, stride, present_off,
                       value_off, sib_off, d_status);
    HIPCHECK(hipGetLastError());
    return P2_OK;
}
static int mm_verify(const uint64_t* keys, int key_bits, const uint64_t* present, const uint64_t* values, size_t value_len, const uint64_t* siblings, const uint64_t* cap,
                     int cap_height, size_t n, int* status, Where w) {
    const bool bad = key_bits < 1 || key_bits > 64 || cap_height < 0 || cap_height > 16 || cap_height > key_bits || value_len > mt::MAP_MAX_VALUE_LEN;
    const size_t depth = bad ? 0 : (size_t)(key_bits - cap_height);
    return run_batch(bad ? "key_bits 1 to 64, cap_height 0 to min(key_bits, 16), value_len at most 134" : nullptr, n, w,
                     {buf_in(keys, n), buf_in(present, n), buf_in(values, n * value_len), buf_in(siblings, n * 4 * depth), buf_in(cap, bad ? 0 : (size_t)4 << cap_height),
                      buf_out(status, n)},
                     [&](const DevPtr* d, hipStream_t s) {
                         hipLaunchKernelGGL(k_mm_verify, g1(n, 64), dim3(64), 0, s, d[0], (u32)key_bits, d[1], d[2], (u32)value_len, d[3], d[4], (u32)cap_height, n, d[5]);
                     });
}

int p2_merkle_map_new(const uint64_t* keys, const uint64_t* values, size_t n, size_t value_len, int key_bits, int cap_height, int device, void** map) {
    return guarded_rc([&] { return mm_new((const u64*)keys, (const u64*)values, false, n, value_len, key_bits, cap_height, device, nullptr, map); });
}
int p2_merkle_map_new_device(const uint64_t* d_keys, const uint64_t* d_values, size_t n, size_t value_len, int key_bits, int cap_height, int device, void* stream,
                             void** map) {
    return guarded_rc([&] { return mm_new((const u64*)d_keys, (const u64*)d_values, true, n, value_len, key_bits, cap_height, device, (hipStream_t)stream, map); });
}
void p2_merkle_map_free(void* map) {
    if (!map) return;
    (void)hipSetDevice(((MerkleMapHandle*)map)->device);
    delete (MerkleMapHandle*)map;
}
int p2_merkle_map_cap(void* map, uint64_t* cap, size_t cap_words) {
    return guarded_rc([&]() -> int {
        MerkleMapHandle* T;
        if (int rc = mm_handle(map, &T)) return rc;
        const size_t words = (size_t)4 << T->h;
        if (!cap || cap_words < words) return set_error("the cap holds " + std::to_string(words) + " words"), P2_ERR_INVALID;
        HIPCHECK(hipEventSynchronize(T->built));
        T->drop_scratch(true);
        HIPCHECK(hipMemcpy(cap, T->cap, words * 8, hipMemcpyDeviceToHost));
        return (int)P2_OK;
    });
}
int p2_merkle_map_len(void* map, size_t* n) {
    return guarded_rc([&]() -> int {
        MerkleMapHandle* T;
        if (int rc = mm_handle(map, &T)) return rc;
        if (!n) return set_error("null argument"), P2_ERR_INVALID;
        *n = T->n;
        return (int)P2_OK;
    });
}
int p2_merkle_map_hashes(void* map, uint64_t* hashes) {
    return guarded_rc([&]() -> int {
        MerkleMapHandle* T;
        if (int rc = mm_handle(map, &T)) return rc;
        if (!hashes) return set_error("null argument"), P2_ERR_INVALID;
        HIPCHECK(hipEventSynchronize(T->built));
        HIPCHECK(hipMemcpy(hashes, T->ctl + 1, 8, hipMemcpyDeviceToHost));
        return (int)P2_OK;
    });
}
int p2_merkle_map_get_batch(void* map, const uint64_t* keys, size_t n, uint64_t* present, uint64_t* values, uint64_t* siblings) {
    return guarded_rc([&]() -> int {
        MerkleMapHandle* T;
        if (int rc = mm_handle(map, &T)) return rc;
        if (n == 0) return (int)P2_OK;
        const size_t sib_words = 4 * (size_t)T->depth(), stride = 1 + T->V + sib_words;
        if (!keys || !present || (T->V && !values) || (sib_words && !siblings)) return set_error("null argument"), P2_ERR_INVALID;
        for (size_t i = 0; i < n; i++)
            if (!mt::map_key_ok(keys[i], T->D)) return set_error("key " + std::to_string(keys[i]) + " (entry " + std::to_string(i) + ") is not below 2^key_bits and p"), P2_ERR_INVALID;
        Allocs tmp;
        u64 *d_keys, *d_out;
        int* d_st;
        if (upload(tmp, &d_keys, (const u64*)keys, n) || dalloc(tmp, &d_out, n * stride) || dalloc(tmp, &d_st, n)) return P2_ERR_HIP;
        const int rc = mm_get(*T, d_keys, n, d_out, stride, 0, 1, 1 + T->V, d_st, T->lane.stream);
        HIPCHECK(hipStreamSynchronize(T->lane.stream));  // before tmp goes, whatever rc says
        if (rc) return rc;
        std::vector<u64> rows(n * stride);
        HIPCHECK(hipMemcpy(rows.data(), d_out, n * stride * 8, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; i++) {
            const u64* row = rows.data() + i * stride;
            present[i] = row[0];
            if (T->V) memcpy(values + i * T->V, row + 1, 8 * (size_t)T->V);
            if (sib_words) memcpy(siblings + i * sib_words, row + 1 + T->V, 8 * sib_words);
        }
        return (int)P2_OK;
    });
}
int p2_merkle_map_get_batch_device(void* map, const uint64_t* d_keys, size_t n, uint64_t* d_out, size_t out_stride_words, size_t present_off, size_t value_off,
                                   size_t siblings_off, int* d_status, void* stream) {
    return guarded_rc([&]() -> int {
        MerkleMapHandle* T;
        if (int rc = mm_handle(map, &T)) return rc;
        return mm_get(*T, (const u64*)d_keys, n, (u64*)d_out, out_stride_words, present_off, value_off, siblings_off, d_status, (hipStream_t)stream);
    });
}
int p2_merkle_map_verify_batch(const uint64_t* keys, int key_bits, const uint64_t* present, const uint64_t* values, size_t value_len, const uint64_t* siblings,
                               const uint64_t* cap, int cap_height, size_t n, int* status, int device) {
    return mm_verify(keys, key_bits, present, values, value_len, siblings, cap, cap_height, n, status, on_host(device));
}
int p2_merkle_map_verify_batch_device(const uint64_t* d_keys, int key_bits, const uint64_t* d_present, const uint64_t* d_values, size_t value_len,
                                      const uint64_t* d_siblings, const uint64_t* d_cap, int cap_height, size_t n, int* d_status, int device, void* stream) {
    return mm_verify(d_keys, key_bits, d_present, d_values, value_len, d_siblings, d_cap, cap_height, n, d_status, on_device(device, stream));
}

// ---- native ecGFp5 in batches: scalar multiplication and Schnorr signatures (kernels_schnorr.h; the host twins are in schnorr.h)
static const size_t SCHNORR_MAX_MSG_LEN = 1024;  // schnorr::MAX_MSG_LEN
static EcWords ec_generator_words() {
    EcWords g;
    p2_ecgfp5_generator(g.w);
    return g;
}
static const char* schnorr_shape(size_t msg_len) { return msg_len > SCHNORR_MAX_MSG_LEN ? "msg_len is at most 1024 words" : nullptr; }
// Each pair of entry points below is one function that states the buffers and the launch (run_batch), called by the host form
// with on_host(device) and by the _device form with on_device(device, stream).
static int ec_mul_batch(const uint64_t* k, const uint64_t* p, size_t count, uint64_t* out, int* status, Where w) {
    return run_batch(nullptr, count, w, {buf_in(k, 5 * count), buf_in(p, 10 * count), buf_out(out, 10 * count), buf_out(status, count)},
                     [&](const DevPtr* d, hipStream_t s) { hipLaunchKernelGGL(k_ec_mul_batch, g1(count, 64), dim3(64), 0, s, d[0], d[1], count, d[2], d[3]); });
}
int p2_ecgfp5_mul_batch(const uint64_t* k, const uint64_t* p, size_t count, uint64_t* out, int* status, int device) {
    return ec_mul_batch(k, p, count, out, status, on_host(device));
}
int p2_ecgfp5_mul_batch_device(const uint64_t* d_k, const uint64_t* d_p, size_t count, uint64_t* d_out, int* d_status, int device, void* stream) {
    return ec_mul_batch(d_k, d_p, count, d_out, d_status, on_device(device, stream));
}
// pk may be NULL: the kernel then writes no public keys
static int schnorr_sign_batch(const uint64_t* sk, const uint64_t* nonce, const uint64_t* msg, size_t msg_len, size_t count, uint64_t* sig, uint64_t* pk, int* status, Where w) {
    return run_batch(schnorr_shape(msg_len), count, w,
                     {buf_in(sk, 5 * count), buf_in(nonce, 5 * count), buf_in(msg, msg_len * count), buf_out(sig, 9 * count), buf_out(pk, 10 * count, true), buf_out(status, count)},
                     [&](const DevPtr* d, hipStream_t s) {
                         hipLaunchKernelGGL(k_schnorr_sign, g1(count, 64), dim3(64), 0, s, d[0], d[1], d[2], (u32)msg_len, count, ec_generator_words(), d[3], d[4], d[5]);
                     });
}
int p2_schnorr_sign_batch(const uint64_t* sk, const uint64_t* nonce, const uint64_t* msg, size_t msg_len, size_t count, uint64_t* sig, uint64_t* pk, int* status, int device) {
    return schnorr_sign_batch(sk, nonce, msg, msg_len, count, sig, pk, status, on_host(device));
}
int p2_schnorr_sign_batch_device(const uint64_t* d_sk, const uint64_t* d_nonce, const uint64_t* d_msg, size_t msg_len, size_t count, uint64_t* d_sig, uint64_t* d_pk,
                                 int* d_status, int device, void* stream) {
    return schnorr_sign_batch(d_sk, d_nonce, d_msg, msg_len, count, d_sig, d_pk, d_status, on_device(device, stream));
}
static int schnorr_verify_batch(const uint64_t* pk, const uint64_t* msg, size_t msg_len, const uint64_t* sig, size_t count, int* status, Where w) {
    return run_batch(schnorr_shape(msg_len), count, w, {buf_in(pk, 10 * count), buf_in(msg, msg_len * count), buf_in(sig, 9 * count), buf_out(status, count)},
                     [&](const DevPtr* d, hipStream_t s) {
                         hipLaunchKernelGGL(k_schnorr_verify, g1(count, 64), dim3(64), 0, s, d[0], d[1], (u32)msg_len, d[2], count, ec_generator_words(), d[3]);
                     });
}
int p2_schnorr_verify_batch(const uint64_t* pk, const uint64_t* msg, size_t msg_len, const uint64_t* sig, size_t count, int* status, int device) {
    return schnorr_verify_batch(pk, msg, msg_len, sig, count, status, on_host(device));
}
int p2_schnorr_verify_batch_device(const uint64_t* d_pk, const uint64_t* d_msg, size_t msg_len, const uint64_t* d_sig, size_t count, int* d_status, int device, void* stream) {
    return schnorr_verify_batch(d_pk, d_msg, msg_len, d_sig, count, d_status, on_device(device, stream));
}
// test entry: out[i] = (a[i] b[i] + c[i]) mod n, one thread per triple
int p2_gpu_ecgfp5_scalar_muladd(const uint64_t* a, const uint64_t* b, const uint64_t* c, size_t count, uint64_t* out, int device) {
    return run_batch(nullptr, count, on_host(device), {buf_in(a, 5 * count), buf_in(b, 5 * count), buf_in(c, 5 * count), buf_out(out, 5 * count)},
                     [&](const DevPtr* d, hipStream_t s) { hipLaunchKernelGGL(k_ec_scalar_muladd, g1(count, 64), dim3(64), 0, s, d[0], d[1], d[2], count, d[3]); });
}

// ---- ElGamal on ecGFp5 in batches (kernels_elgamal.h; the host twins are in ecgfp5.h)
static const size_t ENCODE_MAX_ATTEMPTS = 256;
static int ec_decompress_batch(const uint64_t* w5, size_t count, uint64_t* out, int* status, Where w) {
    return run_batch(nullptr, count, w, {buf_in(w5, 5 * count), buf_out(out, 10 * count), buf_out(status, count)},
                     [&](const DevPtr* d, hipStream_t s) { hipLaunchKernelGGL(k_ec_decompress_batch, g1(count, 64), dim3(64), 0, s, d[0], count, d[1], d[2]); });
}
int p2_ecgfp5_decompress_batch(const uint64_t* w, size_t count, uint64_t* out, int* status, int device) {
    return ec_decompress_batch(w, count, out, status, on_host(device));
}
int p2_ecgfp5_decompress_batch_device(const uint64_t* d_w, size_t count, uint64_t* d_out, int* d_status, int device, void* stream) {
    return ec_decompress_batch(d_w, count, d_out, d_status, on_device(device, stream));
}
static int ec_encode_batch(const uint32_t* limbs, const uint32_t* pad, size_t attempts, size_t count, uint64_t* out, uint32_t* used, int* status, Where w) {
    const bool bad = attempts == 0 || attempts > ENCODE_MAX_ATTEMPTS;
    return run_batch(bad ? "attempts is between 1 and 256" : nullptr, count, w,
                     {buf_in(limbs, 5 * count), buf_in(pad, 5 * attempts * count), buf_out(out, 10 * count), buf_out(used, count), buf_out(status, count)},
                     [&](const DevPtr* d, hipStream_t s) {
                         hipLaunchKernelGGL(k_ec_encode_binary, g1(count, 64), dim3(64), 0, s, d[0], d[1], (u32)attempts, count, d[2], d[3], d[4]);
                     });
}
int p2_ecgfp5_encode_binary_batch(const uint32_t* limbs, const uint32_t* pad, size_t attempts, size_t count, uint64_t* out, uint32_t* used, int* status, int device) {
    return ec_encode_batch(limbs, pad, attempts, count, out, used, status, on_host(device));
}
int p2_ecgfp5_encode_binary_batch_device(const uint32_t* d_limbs, const uint32_t* d_pad, size_t attempts, size_t count, uint64_t* d_out, uint32_t* d_used, int* d_status,
                                         int device, void* stream) {
    return ec_encode_batch(d_limbs, d_pad, attempts, count, d_out, d_used, d_status, on_device(device, stream));
}
// The two encryptions share one call shape, the two decryptions another; `words` is the row width of a message and of the
// second ciphertext half: 10 (a point) for ElGamal, 5 for the hashed form.
using EgEncryptKernel = void (*)(const u64*, const u64*, const u64*, size_t, EcWords, u64*, u64*, int*);
using EgDecryptKernel = void (*)(const u64*, const u64*, const u64*, size_t, u64*, int*);
static int eg_encrypt(EgEncryptKernel kernel, size_t words, const uint64_t* pk, const uint64_t* nonce, const uint64_t* msg, size_t count, uint64_t* c0, uint64_t* c1,
                      int* status, Where w) {
    return run_batch(nullptr, count, w,
                     {buf_in(pk, 10 * count), buf_in(nonce, 5 * count), buf_in(msg, words * count), buf_out(c0, 10 * count), buf_out(c1, words * count), buf_out(status, count)},
                     [&](const DevPtr* d, hipStream_t s) {
                         hipLaunchKernelGGL(kernel, g1(count, 64), dim3(64), 0, s, d[0], d[1], d[2], count, ec_generator_words(), d[3], d[4], d[5]);
                     });
}
static int eg_decrypt(EgDecryptKernel kernel, size_t words, const uint64_t* sk, const uint64_t* c0, const uint64_t* c1, size_t count, uint64_t* msg, int* status, Where w) {
    return run_batch(nullptr, count, w, {buf_in(sk, 5 * count), buf_in(c0, 10 * count), buf_in(c1, words * count), buf_out(msg, words * count), buf_out(status, count)},
                     [&](const DevPtr* d, hipStream_t s) { hipLaunchKernelGGL(kernel, g1(count, 64), dim3(64), 0, s, d[0], d[1], d[2], count, d[3], d[4]); });
}
int p2_elgamal_encrypt_batch(const uint64_t* pk, const uint64_t* nonce, const uint64_t* msg, size_t count, uint64_t* c0, uint64_t* c1, int* status, int device) {
    return eg_encrypt(k_elgamal_encrypt, 10, pk, nonce, msg, count, c0, c1, status, on_host(device));
}
int p2_elgamal_encrypt_batch_device(const uint64_t* d_pk, const uint64_t* d_nonce, const uint64_t* d_msg, size_t count, uint64_t* d_c0, uint64_t* d_c1, int* d_status,
                                    int device, void* stream) {
    return eg_encrypt(k_elgamal_encrypt, 10, d_pk, d_nonce, d_msg, count, d_c0, d_c1, d_status, on_device(device, stream));
}
int p2_elgamal_decrypt_batch(const uint64_t* sk, const uint64_t* c0, const uint64_t* c1, size_t count, uint64_t* msg, int* status, int device) {
    return eg_decrypt(k_elgamal_decrypt, 10, sk, c0, c1, count, msg, status, on_host(device));
}
int p2_elgamal_decrypt_batch_device(const uint64_t* d_sk, const uint64_t* d_c0, const uint64_t* d_c1, size_t count, uint64_t* d_msg, int* d_status, int device, void* stream) {
    return eg_decrypt(k_elgamal_decrypt, 10, d_sk, d_c0, d_c1, count, d_msg, d_status, on_device(device, stream));
}
int p2_hashed_elgamal_encrypt_batch(const uint64_t* pk, const uint64_t* nonce, const uint64_t* msg, size_t count, uint64_t* c0, uint64_t* ct, int* status, int device) {
    return eg_encrypt(k_hashed_elgamal_encrypt, 5, pk, nonce, msg, count, c0, ct, status, on_host(device));
}
int p2_hashed_elgamal_encrypt_batch_device(const uint64_t* d_pk, const uint64_t* d_nonce, const uint64_t* d_msg, size_t count, uint64_t* d_c0, uint64_t* d_ct,
                                           int* d_status, int device, void* stream) {
    return eg_encrypt(k_hashed_elgamal_encrypt, 5, d_pk, d_nonce, d_msg, count, d_c0, d_ct, d_status, on_device(device, stream));
}
int p2_hashed_elgamal_decrypt_batch(const uint64_t* sk, const uint64_t* c0, const uint64_t* ct, size_t count, uint64_t* msg, int* status, int device) {
    return eg_decrypt(k_hashed_elgamal_decrypt, 5, sk, c0, ct, count, msg, status, on_host(device));
}
int p2_hashed_elgamal_decrypt_batch_device(const uint64_t* d_sk, const uint64_t* d_c0, const uint64_t* d_ct, size_t count, uint64_t* d_msg, int* d_status, int device,
                                           void* stream) {
    return eg_decrypt(k_hashed_elgamal_decrypt, 5, d_sk, d_c0, d_ct, count, d_msg, d_status, on_device(device, stream));
}
int p2_ecgfp5_scalar_bits_device(const uint64_t* d_k, size_t count, uint64_t* d_out, size_t stride, int device, void* stream) {
    return run_batch(stride < 320 ? "stride is at least 320 words" : nullptr, count, on_device(device, stream), {buf_in(d_k, 5 * count), buf_out(d_out, stride * count)},
                     [&](const DevPtr* d, hipStream_t s) { hipLaunchKernelGGL(k_ec_scalar_bits, g1(count, 64), dim3(64), 0, s, d[0], count, d[1], stride); });
}

// ---- the Poseidon cipher in batches (kernels_pcipher.h; the host twins are in poseidon_cipher.h).  Encryption and decryption
// share one call shape: ks, nonce, one input row and one output row per item, of 5 l and 5 (pad3(l) + 1) words in this or the
// other order.
static const size_t PCIPHER_MAX_LEN = 3072;
static int pcipher_run(bool decrypt, const uint64_t* ks, const uint64_t* nonce, const uint64_t* in, size_t l, size_t count, uint64_t* out, int* status, Where w) {
    const bool bad = l > PCIPHER_MAX_LEN;
    const size_t msg_words = bad ? 0 : 5 * l, ct_words = bad ? 0 : 5 * ((l + 2) / 3 * 3 + 1);
    const auto kernel = decrypt ? k_pcipher_decrypt : k_pcipher_encrypt;
    return run_batch(bad ? "l is at most 3072 elements" : nullptr, count, w,
                     {buf_in(ks, 10 * count), buf_in(nonce, 2 * count), buf_in(in, (decrypt ? ct_words : msg_words) * count),
                      buf_out(out, (decrypt ? msg_words : ct_words) * count), buf_out(status, count)},
                     [&](const DevPtr* d, hipStream_t s) { hipLaunchKernelGGL(kernel, g1(count, 64), dim3(64), 0, s, d[0], d[1], d[2], (u32)l, count, d[3], d[4]); });
}
int p2_poseidon_encrypt_batch(const uint64_t* ks, const uint64_t* nonce, const uint64_t* msg, size_t l, size_t count, uint64_t* ct, int* status, int device) {
    return pcipher_run(false, ks, nonce, msg, l, count, ct, status, on_host(device));
}
int p2_poseidon_encrypt_batch_device(const uint64_t* d_ks, const uint64_t* d_nonce, const uint64_t* d_msg, size_t l, size_t count, uint64_t* d_ct, int* d_status, int device,
                                     void* stream) {
    return pcipher_run(false, d_ks, d_nonce, d_msg, l, count, d_ct, d_status, on_device(device, stream));
}
int p2_poseidon_decrypt_batch(const uint64_t* ks, const uint64_t* nonce, const uint64_t* ct, size_t l, size_t count, uint64_t* msg, int* status, int device) {
    return pcipher_run(true, ks, nonce, ct, l, count, msg, status, on_host(device));
}
int p2_poseidon_decrypt_batch_device(const uint64_t* d_ks, const uint64_t* d_nonce, const uint64_t* d_ct, size_t l, size_t count, uint64_t* d_msg, int* d_status, int device,
                                     void* stream) {
    return pcipher_run(true, d_ks, d_nonce, d_ct, l, count, d_msg, d_status, on_device(device, stream));
}

// ---- AES-GCM in batches (kernels_gcm.h; the host twins are aes::gcm_encrypt_aad and aes::gcm_decrypt).  Encryption and
// decryption share one call shape: key, nonce and aad rows, one input row and one output row per item `stride` bytes apart, and
// the tag, which encryption writes and decryption reads.  Three launches over the scratch workspace: setup, then counter mode and
// GHASH in the order the direction needs.
static const size_t GCM_MAX_LEN = (size_t)1 << 24, GCM_MAX_AAD = (size_t)1 << 16;
// From this many GHASH blocks per item the one-wave-per-item kernel runs, below it the one-thread-per-item kernel: the smallest
// measured block count from which the wide form is faster (profiles/gcm_bench.jsonl).
static const size_t GCM_WIDE_MIN_BLOCKS = 128;
static bool gcm_nk_ok(int nk) { return nk == 4 || nk == 6 || nk == 8; }
static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static void gcm_ghash_launch(int lanes, hipStream_t s, const u32* ws, int nk, const GhashIn& in, size_t count, const uint8_t* given, uint8_t* out, int* status) {
    if (lanes == 64)
        hipLaunchKernelGGL(k_gcm_ghash<64>, dim3((u32)count), dim3(64), 0, s, ws, nk, in, count, given, out, status);
    else
        hipLaunchKernelGGL(k_gcm_ghash<1>, g1(count, 64), dim3(64), 0, s, ws, nk, in, count, given, out, status);
}
// One call on device pointers, and its three steps.  tag is written by an encryption and read by a decryption; lanes 0 is the
// choice by GCM_WIDE_MIN_BLOCKS.
struct GcmCall {
    bool decrypt;
    int nk;
    size_t aad_len, len, stride, count;
    const uint8_t *key, *nonce, *aad, *in;
    uint8_t *tag, *out;
    int* status;
    u32* ws;
    int lanes;
    size_t blocks() const { return (len + 15) / 16; }
    bool aligned() const { return aligned16(in) && aligned16(out) && stride % 16 == 0; }
};
static void gcm_setup_step(const GcmCall& c, hipStream_t s) {
    hipLaunchKernelGGL(k_gcm_setup, g1(c.count, 64), dim3(64), 0, s, c.key, c.nk, c.nonce, (const uint8_t*)nullptr, c.count, c.ws);
}
static void gcm_ctr_step(const GcmCall& c, hipStream_t s) {
    if (!c.blocks()) return;
    const int* gate = c.decrypt ? c.status : nullptr;
    if (c.aligned())
        hipLaunchKernelGGL(k_gcm_ctr<true>, g1(c.count * c.blocks(), 256), dim3(256), 0, s, c.ws, c.nk, c.in, c.len, c.stride, c.count, gate, c.out);
    else
        hipLaunchKernelGGL(k_gcm_ctr<false>, g1(c.count * c.blocks(), 256), dim3(256), 0, s, c.ws, c.nk, c.in, c.len, c.stride, c.count, gate, c.out);
}
static void gcm_ghash_step(const GcmCall& c, hipStream_t s) {
    const uint8_t* ct = c.decrypt ? c.in : c.out;
    const GhashIn g{c.aad, ct, c.aad_len, c.len, c.stride, false, aligned16(ct) && c.stride % 16 == 0};
    const int lanes = c.lanes ? c.lanes : (c.aad_len + 15) / 16 + c.blocks() + 1 >= GCM_WIDE_MIN_BLOCKS ? 64 : 1;
    gcm_ghash_launch(lanes, s, c.ws, c.nk, g, c.count, c.decrypt ? c.tag : nullptr, c.decrypt ? nullptr : c.tag, c.status);
}
static int gcm_run(bool decrypt, const uint8_t* key, int nk, const uint8_t* nonce, const uint8_t* aad, size_t aad_len, const uint8_t* in, uint8_t* tag, size_t len,
                   size_t stride, size_t count, uint8_t* out, int* status, void* work, Where w) {
    const char* bad = nullptr;
    if (!gcm_nk_ok(nk)) bad = "nk is 4, 6 or 8";
    else if (len > GCM_MAX_LEN) bad = "len is at most 2^24 bytes";
    else if (aad_len > GCM_MAX_AAD) bad = "aad_len is at most 2^16 bytes";
    else if (stride < len) bad = "row_stride is at least len";
    else if (count >> 31 || (count * ((len + 15) / 16) / 256) >> 31) bad = "count is too large for one launch";
    else if (w.on_device && !aligned16(work)) bad = "d_work is 16-byte aligned";
    if (bad) nk = 4, len = aad_len = stride = 0;
    return run_batch(bad, count, w,
                     {buf_in(key, (size_t)4 * nk * count), buf_in(nonce, 12 * count), buf_in(aad, aad_len * count), buf_in(in, stride * count),
                      decrypt ? buf_in(tag, 16 * count) : buf_out(tag, 16 * count), buf_out(out, stride * count), buf_out(status, count),
                      buf_scratch((u32*)work, (size_t)gcm_ws_words(nk + 6) * count)},
                     [&](const DevPtr* d, hipStream_t s) {
                         const GcmCall c{decrypt, nk, aad_len, len, stride, count, d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], 0};
                         gcm_setup_step(c, s);
                         if (decrypt) gcm_ghash_step(c, s), gcm_ctr_step(c, s);  // the status first: it gates the counter mode
                         else gcm_ctr_step(c, s), gcm_ghash_step(c, s);
                     });
}
size_t p2_aes_gcm_batch_workspace(int nk, size_t len, size_t aad_len, size_t count) {
    (void)len, (void)aad_len;  // the workspace holds per-item key material only
    return gcm_nk_ok(nk) ? (size_t)gcm_ws_words(nk + 6) * 4 * count : 0;
}
int p2_aes_gcm_encrypt_batch(const uint8_t* key, int nk, const uint8_t* nonce, const uint8_t* aad, size_t aad_len, const uint8_t* pt, size_t len, size_t count,
                             uint8_t* ct, uint8_t* tag, int* status, int device) {
    return gcm_run(false, key, nk, nonce, aad, aad_len, pt, tag, len, len, count, ct, status, nullptr, on_host(device));
}
int p2_aes_gcm_decrypt_batch(const uint8_t* key, int nk, const uint8_t* nonce, const uint8_t* aad, size_t aad_len, const uint8_t* ct, const uint8_t* tag, size_t len,
                             size_t count, uint8_t* pt, int* status, int device) {
    return gcm_run(true, key, nk, nonce, aad, aad_len, ct, (uint8_t*)tag, len, len, count, pt, status, nullptr, on_host(device));
}
int p2_aes_gcm_encrypt_batch_device(const uint8_t* d_key, int nk, const uint8_t* d_nonce, const uint8_t* d_aad, size_t aad_len, const uint8_t* d_pt, size_t len,
                                    size_t row_stride, size_t count, uint8_t* d_ct, uint8_t* d_tag, int* d_status, void* d_work, int device, void* stream) {
    return gcm_run(false, d_key, nk, d_nonce, d_aad, aad_len, d_pt, d_tag, len, row_stride, count, d_ct, d_status, d_work, on_device(device, stream));
}
int p2_aes_gcm_decrypt_batch_device(const uint8_t* d_key, int nk, const uint8_t* d_nonce, const uint8_t* d_aad, size_t aad_len, const uint8_t* d_ct,
                                    const uint8_t* d_tag, size_t len, size_t row_stride, size_t count, uint8_t* d_pt, int* d_status, void* d_work, int device,
                                    void* stream) {
    return gcm_run(true, d_key, nk, d_nonce, d_aad, aad_len, d_ct, (uint8_t*)d_tag, len, row_stride, count, d_pt, d_status, d_work, on_device(device, stream));
}
int p2_bytes_to_words_device(const uint8_t* d_bytes, size_t row_bytes, size_t byte_stride, size_t count, uint64_t* d_out, size_t stride_words, int device,
                             void* stream) {
    const char* bad = row_bytes > stride_words ? "stride_words is at least row_bytes" : nullptr;
    return run_batch(bad, row_bytes ? count : 0, on_device(device, stream), {buf_in(d_bytes, row_bytes * count), buf_out(d_out, stride_words * count)},
                     [&](const DevPtr* d, hipStream_t s) {
                         hipLaunchKernelGGL(k_bytes_to_words, g1(count * row_bytes, 256), dim3(256), 0, s, d[0], row_bytes, byte_stride, count, d[1], stride_words);
                     });
}
// test entries: the GHASH kernel alone with the lane count chosen, against p2_native_ghash; the block cipher alone, against
// p2_native_aes_encrypt_block
int p2_gpu_gcm_ghash(const uint8_t* h, const uint8_t* x, size_t blocks, size_t count, int lanes, uint8_t* out, int device) {
    const char* bad = lanes != 1 && lanes != 64 ? "lanes is 1 or 64" : blocks > GCM_MAX_LEN / 16 ? "at most 2^20 blocks" : nullptr;
    return run_batch(bad, count, on_host(device),
                     {buf_in(h, 16 * count), buf_in(x, 16 * blocks * count), buf_out(out, 16 * count), buf_scratch((u32*)nullptr, (size_t)gcm_ws_words(10) * count)},
                     [&](const DevPtr* d, hipStream_t s) {
                         hipLaunchKernelGGL(k_gcm_setup, g1(count, 64), dim3(64), 0, s, (const uint8_t*)nullptr, 4, (const uint8_t*)nullptr, d[0], count, d[3]);
                         GhashIn g{nullptr, d[1], 0, 16 * blocks, 16 * blocks, true, true};
                         gcm_ghash_launch(lanes, s, d[3], 4, g, count, nullptr, d[2], nullptr);
                     });
}
int p2_gpu_aes_encrypt_blocks(const uint8_t* key, int nk, const uint8_t* in, size_t count, uint8_t* out, int device) {
    const bool bad = !gcm_nk_ok(nk);
    if (bad) nk = 4;
    return run_batch(bad ? "nk is 4, 6 or 8" : nullptr, count, on_host(device),
                     {buf_in(key, (size_t)4 * nk * count), buf_in(in, 16 * count), buf_out(out, 16 * count), buf_scratch((u32*)nullptr, (size_t)gcm_ws_words(nk + 6) * count)},
                     [&](const DevPtr* d, hipStream_t s) {
                         hipLaunchKernelGGL(k_gcm_setup, g1(count, 64), dim3(64), 0, s, d[0], nk, (const uint8_t*)nullptr, (const uint8_t*)nullptr, count, d[3]);
                         hipLaunchKernelGGL(k_aes_encrypt_blocks, g1(count, 64), dim3(64), 0, s, d[3], nk, d[1], count, d[2]);
                     });
}
// bench entry (tools/gpu_gcm_bench.py): encryptions of `count` items on device buffers filled here with random bytes, one
// warm-up and then `repeats` runs with an event between the kernels: ns[3 r + 0 .. 2] = k_gcm_setup, k_gcm_ctr, k_gcm_ghash of
// run r, in nanoseconds.  lanes 1 or 64 forces the GHASH kernel, 0 leaves the public calls' choice.
int p2_gpu_gcm_kernel_times(int nk, size_t len, size_t aad_len, size_t count, int lanes, size_t repeats, uint64_t* ns, int device) {
    return guarded_rc([&]() -> int {
        if (!gcm_nk_ok(nk) || len > GCM_MAX_LEN || aad_len > GCM_MAX_AAD || !count || count >> 31 || (lanes != 0 && lanes != 1 && lanes != 64) || !repeats || !ns)
            return set_error("p2_gpu_gcm_kernel_times: argument out of range"), P2_ERR_INVALID;
        if (int rc = pick_device(device)) return rc;
        Allocs tmp;
        const size_t stride = (len + 15) / 16 * 16, sizes[4] = {(size_t)4 * nk * count, 12 * count, aad_len * count, stride * count};
        uint8_t* in[4];
        std::mt19937_64 gen(1);
        for (int k = 0; k < 4; k++) {
            std::vector<uint64_t> host(sizes[k] / 8 + 1);
            for (auto& v : host) v = gen();
            if (upload(tmp, &in[k], (const uint8_t*)host.data(), sizes[k])) return P2_ERR_HIP;
        }
        uint8_t *out, *tag;
        int* status;
        u32* ws;
        if (dalloc(tmp, &out, stride * count) || dalloc(tmp, &tag, 16 * count) || dalloc(tmp, &status, count) || dalloc(tmp, &ws, (size_t)gcm_ws_words(nk + 6) * count))
            return P2_ERR_HIP;
        const GcmCall c{false, nk, aad_len, len, stride, count, in[0], in[1], in[2], in[3], tag, out, status, ws, lanes};
        Event ev[4];
        for (Event& e : ev) HIPCHECK(e.create(hipEventDefault));
        for (size_t r = 0; r <= repeats; r++) {
            HIPCHECK(hipEventRecord(ev[0], nullptr));
            gcm_setup_step(c, nullptr);
            HIPCHECK(hipEventRecord(ev[1], nullptr));
            gcm_ctr_step(c, nullptr);
            HIPCHECK(hipEventRecord(ev[2], nullptr));
            gcm_ghash_step(c, nullptr);
            HIPCHECK(hipEventRecord(ev[3], nullptr));
            HIPCHECK(hipEventSynchronize(ev[3]));
            HIPCHECK(hipGetLastError());
            if (r)
                for (int k = 0; k < 3; k++) {
                    float ms = 0;
                    HIPCHECK(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
                    ns[3 * (r - 1) + k] = (uint64_t)((double)ms * 1e6);
                }
        }
        return (int)P2_OK;
    });
}

// ---- batched verification
int p2_verify_batch(p2_circuit* C, size_t batch, const uint8_t* proofs, const uint64_t* verifier_data, size_t vd_len, int* status) {
    return guarded_rc([&] { return proof_batch_impl(C, OP_VERIFY, batch, proofs, nullptr, verifier_data, vd_len, nullptr, nullptr, status, nullptr, true); });
}
int p2_verify_batch_device(p2_circuit* C, size_t batch, const uint8_t* d_proofs, const uint64_t* verifier_data, size_t vd_len, int* d_status, void* stream) {
    return guarded_rc([&] { return proof_batch_impl(C, OP_VERIFY, batch, d_proofs, nullptr, verifier_data, vd_len, nullptr, nullptr, d_status, (hipStream_t)stream, false); });
}
int p2_gpu_vanishing_flags(p2_circuit* C, size_t batch, const uint8_t* buffers, const uint64_t* challenges, const uint64_t* pi_hashes, uint32_t* flags) {
    return guarded_rc([&] { return vanishing_flags_impl(C, batch, buffers, challenges, pi_hashes, flags); });
}
int p2_compress_batch(p2_circuit* C, size_t batch, const uint8_t* proofs, const uint64_t* vd, size_t vd_len, uint8_t* out, uint32_t* lengths, int* status) {
    return guarded_rc([&] { return proof_batch_impl(C, OP_COMPRESS, batch, proofs, nullptr, vd, vd_len, out, lengths, status, nullptr, true); });
}
int p2_compress_batch_device(p2_circuit* C, size_t batch, const uint8_t* d_proofs, const uint64_t* vd, size_t vd_len, uint8_t* d_out, uint32_t* d_lengths,
                             int* d_status, void* stream) {
    return guarded_rc([&] { return proof_batch_impl(C, OP_COMPRESS, batch, d_proofs, nullptr, vd, vd_len, d_out, d_lengths, d_status, (hipStream_t)stream, false); });
}
int p2_decompress_batch(p2_circuit* C, size_t batch, const uint8_t* cproofs, const uint32_t* lengths, const uint64_t* vd, size_t vd_len, uint8_t* out, int* status) {
    return guarded_rc([&] { return proof_batch_impl(C, OP_DECOMPRESS, batch, cproofs, lengths, vd, vd_len, out, nullptr, status, nullptr, true); });
}
int p2_decompress_batch_device(p2_circuit* C, size_t batch, const uint8_t* d_cproofs, const uint32_t* d_lengths, const uint64_t* vd, size_t vd_len, uint8_t* d_out,
                               int* d_status, void* stream) {
    return guarded_rc([&] { return proof_batch_impl(C, OP_DECOMPRESS, batch, d_cproofs, d_lengths, vd, vd_len, d_out, nullptr, d_status, (hipStream_t)stream, false); });
}
int p2_verify_compressed_batch(p2_circuit* C, size_t batch, const uint8_t* cproofs, const uint32_t* lengths, const uint64_t* vd, size_t vd_len, int* status) {
    return guarded_rc([&] { return proof_batch_impl(C, OP_VERIFY_COMPRESSED, batch, cproofs, lengths, vd, vd_len, nullptr, nullptr, status, nullptr, true); });
}
int p2_verify_compressed_batch_device(p2_circuit* C, size_t batch, const uint8_t* d_cproofs, const uint32_t* d_lengths, const uint64_t* vd, size_t vd_len,
                                      int* d_status, void* stream) {
    return guarded_rc([&] { return proof_batch_impl(C, OP_VERIFY_COMPRESSED, batch, d_cproofs, d_lengths, vd, vd_len, nullptr, nullptr, d_status, (hipStream_t)stream, false); });
}
}
