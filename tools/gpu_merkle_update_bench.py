#!/usr/bin/env python3
"""Ordered leaf updates against a full rebuild on one GPU: a 2^20 x 8-word tree with cap height 4 (the tree of
profiles/merkle_bench.jsonl), k = 2^8, 2^12, 2^16, 2^20 random indices.  Three forms alternate in one process on the same
buffers, medians of MERKLE_UPDATE_BENCH_REPEATS (5) with the range, after a warm-up round:

  update           p2_merkle_tree_update_device without a trace: every changed node hashed once
  update+trace     the same with siblings and root_after: k * depth hashes
  rebuild          p2_gpu_merkle_build_device with the transpose, the build of p2_merkle_tree_new (unchanged by updates)

and the host twin p2_native_merkle_update on the same tree for 0, 2^8 and 2^12 items with their traces: it rebuilds the tree on
every call (k = 0 is that alone), then loops over the items; loop_ms is the difference.  Every timed call ends with a stream synchronisation.
Appends one JSON line to profiles/merkle_update_bench.jsonl."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("MERKLE_UPDATE_BENCH_OUT", os.path.join(ROOT, "profiles", "merkle_update_bench.jsonl"))
REPEATS = int(os.environ.get("MERKLE_UPDATE_BENCH_REPEATS", "5"))
BITS, LEAF_LEN, CAP_HEIGHT = int(os.environ.get("MERKLE_UPDATE_BENCH_BITS", "20")), 8, 4
KS = [1 << b for b in (8, 12, 16, 20) if b <= BITS]
HOST_KS = (1 << 8, 1 << 12)
P = 0xFFFFFFFF00000001


def field(rng, shape):
    return (rng.integers(0, 1 << 63, size=shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=shape, dtype=np.uint64)) % np.uint64(P)


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    pkg = g.load_package()
    L = pkg.lib()
    assert L.p2_gpu_device_count() > 0, "no HIP device"
    n, depth = 1 << BITS, BITS - CAP_HEIGHT
    rng = np.random.default_rng(7)
    leaves = field(rng, (n, LEAF_LEN))
    u64p, vp = C.POINTER(C.c_uint64), C.c_void_p

    H = C.CDLL(next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln))
    H.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
    H.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
    H.hipStreamCreate.argtypes = [C.POINTER(vp)]
    H.hipStreamSynchronize.argtypes = [vp]

    def dalloc(nbytes, host=None):
        p = vp()
        assert H.hipMalloc(C.byref(p), nbytes) == 0
        if host is not None:
            assert H.hipMemcpy(p, host.ctypes.data_as(vp), nbytes, 1) == 0
        return p

    s = vp()
    assert H.hipStreamCreate(C.byref(s)) == 0
    d_leaves, d_scratch, d_dig = dalloc(leaves.nbytes, leaves), dalloc(leaves.nbytes), dalloc(64 * n)
    tree = vp()
    assert L.p2_merkle_tree_new_device(d_leaves, n, LEAF_LEN, CAP_HEIGHT, 0, s, C.byref(tree)) == 0, L.p2_last_error()
    kmax = max(KS)
    idx_all, new_all = rng.integers(0, n, size=kmax, dtype=np.uint64), field(rng, (kmax, LEAF_LEN))
    d_idx, d_new = dalloc(idx_all.nbytes, idx_all), dalloc(new_all.nbytes, new_all)
    d_sib, d_root, d_st = dalloc(32 * depth * kmax), dalloc(32 * kmax), dalloc(4 * kmax)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        assert H.hipStreamSynchronize(s) == 0
        return 1e3 * (time.perf_counter() - t0)

    def update(k, trace):
        assert L.p2_merkle_tree_update_device(tree, d_idx, d_new, k, d_sib if trace else None, 4 * depth, d_root if trace else None, 4, d_st, s) == 0, L.p2_last_error()

    def rebuild():
        assert L.p2_gpu_merkle_build_device(d_leaves, n, LEAF_LEN, CAP_HEIGHT, 1, d_scratch, d_dig, 0, s) == 0, L.p2_last_error()

    res = {"num_leaves": n, "leaf_len": LEAF_LEN, "cap_height": CAP_HEIGHT, "repeats": REPEATS, "k": {}}
    hashes = C.c_uint64()
    for k in KS:
        forms = {"update": lambda: update(k, False), "update+trace": lambda: update(k, True), "rebuild": rebuild}
        runs, counted = {name: [] for name in forms}, {}
        for rep in range(REPEATS + 1):          # the first round warms up (and grows the handle's scratch block)
            for name, fn in forms.items():      # alternated: every round runs every form once
                t = timed(fn)
                if rep:
                    runs[name].append(t)
                if name != "rebuild":
                    assert L.p2_merkle_tree_last_update_hashes(tree, C.byref(hashes)) == 0
                    counted[name] = hashes.value
        row = {name: {"ms": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for name, v in runs.items()}
        assert counted["update+trace"] == k * depth, counted
        row["hashes"] = counted
        row["traced_perm_per_s"] = round(k * depth / row["update+trace"]["ms"] * 1e3)
        res["k"][str(k)] = row
        print(k, row, flush=True)
    st = np.empty(kmax, dtype=np.int32)
    assert H.hipMemcpy(st.ctypes.data_as(vp), d_st, st.nbytes, 2) == 0 and not st.any()
    L.p2_merkle_tree_free(tree)

    # ---- the host twin: one call per k on the whole tree; k = 0 is the rebuild every call starts with
    sib, root = np.empty(4 * depth * max(HOST_KS), dtype=np.uint64), np.empty(4 * max(HOST_KS), dtype=np.uint64)
    res["host"] = {}
    for k in (0,) + HOST_KS:
        t0 = time.perf_counter()
        assert L.p2_native_merkle_update(leaves.ctypes.data_as(u64p), n, LEAF_LEN, CAP_HEIGHT, idx_all.ctypes.data_as(u64p), new_all.ctypes.data_as(u64p), k,
                                         sib.ctypes.data_as(u64p), root.ctypes.data_as(u64p)) == 0, L.p2_last_error()
        res["host"][str(k)] = {"ms": round(1e3 * (time.perf_counter() - t0), 1)}
        print("host", k, res["host"][str(k)], flush=True)
    for k in HOST_KS:
        res["host"][str(k)]["loop_ms"] = round(res["host"][str(k)]["ms"] - res["host"]["0"]["ms"], 1)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
