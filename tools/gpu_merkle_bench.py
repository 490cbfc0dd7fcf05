#!/usr/bin/env python3
"""Stand-alone Merkle trees on one GPU, everything alternated in one process, medians of MERKLE_BENCH_REPEATS (5) after a warm-up.

  build      a 2^20 x 8-word tree (cap height 4) on the same buffers (p2_gpu_merkle_build_device):
               colmajor             k_hash_leaves on the data laid out column-major, then the levels: p2_gpu_merkle_cap's build
               transpose+colmajor   the transpose kernel from the row-major leaves in front of it: the build of p2_merkle_tree_new
             and p2_merkle_tree_new_device itself, which also allocates the digests and the column-major copy (64 MiB each).
             (The first line of profiles/merkle_bench.jsonl also has "rowmajor": a leaf kernel that staged row-major sponge blocks
             through an LDS tile, measured once against the transpose and then dropped -- DESIGN.md section 9f.)
  openings   p2_merkle_tree_prove_batch_device for 2^16 random indices of that tree
  verify     p2_merkle_verify_batch (host pointers: transfers included), its device form, and a host loop over
             p2_native_merkle_verify on 2^12 of the paths

Appends one JSON line to profiles/merkle_bench.jsonl."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("MERKLE_BENCH_OUT", os.path.join(ROOT, "profiles", "merkle_bench.jsonl"))
REPEATS = int(os.environ.get("MERKLE_BENCH_REPEATS", "5"))
BITS, LEAF_LEN, CAP_HEIGHT, N_OPEN, N_HOST = int(os.environ.get("MERKLE_BENCH_BITS", "20")), 8, 4, 1 << 16, 1 << 12
P = 0xFFFFFFFF00000001


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    pkg = g.load_package()
    L = pkg.lib()
    assert L.p2_gpu_device_count() > 0, "no HIP device"
    n, depth = 1 << BITS, BITS - CAP_HEIGHT
    rng = np.random.default_rng(7)
    leaves = (rng.integers(0, 1 << 63, size=(n, LEAF_LEN), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, LEAF_LEN), dtype=np.uint64)) % np.uint64(P)
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

    def read(p, count, dtype=np.uint64):
        out = np.empty(count, dtype=dtype)
        assert H.hipMemcpy(out.ctypes.data_as(vp), p, out.nbytes, 2) == 0
        return out

    s = vp()
    assert H.hipStreamCreate(C.byref(s)) == 0
    d_leaves, d_cols = dalloc(leaves.nbytes, leaves), dalloc(leaves.nbytes, np.ascontiguousarray(leaves.T))
    d_scratch, d_dig = dalloc(leaves.nbytes), [dalloc(64 * n) for _ in range(2)]
    cap_off = 4 * (2 * n - (2 << CAP_HEIGHT))   # level_off(bits, bits - cap_height)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        assert H.hipStreamSynchronize(s) == 0
        return 1e3 * (time.perf_counter() - t0)

    def build(with_transpose, scratch, dig):
        assert L.p2_gpu_merkle_build_device(d_leaves, n, LEAF_LEN, CAP_HEIGHT, with_transpose, scratch, dig, 0, s) == 0, L.p2_last_error()

    forms = {"colmajor": lambda: build(0, d_cols, d_dig[0]), "transpose+colmajor": lambda: build(1, d_scratch, d_dig[1])}
    trees = []

    def new_device():
        h = vp()
        assert L.p2_merkle_tree_new_device(d_leaves, n, LEAF_LEN, CAP_HEIGHT, 0, s, C.byref(h)) == 0, L.p2_last_error()
        trees.append(h)

    forms["p2_merkle_tree_new_device"] = new_device
    runs = {k: [] for k in forms}
    for rep in range(REPEATS + 1):          # the first round warms up
        for name, fn in forms.items():      # alternated: every round runs every form once
            t = timed(fn)
            if rep:
                runs[name].append(t)
        while len(trees) > 1:
            L.p2_merkle_tree_free(trees.pop(0))
    caps = [read(vp(d.value + 8 * cap_off), 4 << CAP_HEIGHT) for d in d_dig]
    tree = trees[0]
    cap = np.empty(4 << CAP_HEIGHT, dtype=np.uint64)
    assert L.p2_merkle_tree_cap(tree, cap.ctypes.data_as(u64p), cap.size) == 0
    assert all((c == cap).all() for c in caps), "the builds disagree"
    res = {"num_leaves": n, "leaf_len": LEAF_LEN, "cap_height": CAP_HEIGHT, "repeats": REPEATS,
           "build_ms": {k: round(statistics.median(v), 3) for k, v in runs.items()}, "build_ms_runs": {k: [round(t, 3) for t in v] for k, v in runs.items()}}
    b = res["build_ms"]
    res["transpose_share"] = round(1 - b["colmajor"] / b["transpose+colmajor"], 4)

    # ---- openings
    idx = rng.integers(0, n, size=N_OPEN, dtype=np.uint64)
    d_idx, d_paths, d_st = dalloc(idx.nbytes, idx), dalloc(32 * depth * N_OPEN), dalloc(4 * N_OPEN)

    def open_paths():
        assert L.p2_merkle_tree_prove_batch_device(tree, d_idx, N_OPEN, d_paths, 4 * depth, d_st, s) == 0, L.p2_last_error()

    timed(open_paths)
    t_open = statistics.median(timed(open_paths) for _ in range(REPEATS))
    assert not read(d_st, N_OPEN, np.int32).any()
    res["openings"] = {"n": N_OPEN, "depth": depth, "ms": round(t_open, 3), "per_s": round(N_OPEN / t_open * 1e3)}

    # ---- verification
    opened = np.ascontiguousarray(leaves[idx.astype(np.int64)])
    paths = read(d_paths, 4 * depth * N_OPEN)
    d_opened, d_cap, d_vst = dalloc(opened.nbytes, opened), dalloc(cap.nbytes, cap), dalloc(4 * N_OPEN)
    status = np.full(N_OPEN, -1, dtype=np.int32)
    ip = C.POINTER(C.c_int)

    def verify_host_pointers():
        assert L.p2_merkle_verify_batch(opened.ctypes.data_as(u64p), LEAF_LEN, idx.ctypes.data_as(u64p), paths.ctypes.data_as(u64p), depth, cap.ctypes.data_as(u64p),
                                        CAP_HEIGHT, N_OPEN, status.ctypes.data_as(ip), 0) == 0, L.p2_last_error()

    def verify_device():
        assert L.p2_merkle_verify_batch_device(d_opened, LEAF_LEN, d_idx, d_paths, depth, d_cap, CAP_HEIGHT, N_OPEN, d_vst, 0, s) == 0, L.p2_last_error()

    timed(verify_host_pointers)
    assert not status.any()
    timed(verify_device)
    assert not read(d_vst, N_OPEN, np.int32).any()
    t_vh = statistics.median(timed(verify_host_pointers) for _ in range(REPEATS))
    t_vd = statistics.median(timed(verify_device) for _ in range(REPEATS))

    def host_loop():
        st = C.c_int()
        for i in range(N_HOST):
            assert L.p2_native_merkle_verify(opened[i].ctypes.data_as(u64p), LEAF_LEN, int(idx[i]), paths[4 * depth * i:].ctypes.data_as(u64p), depth,
                                             cap.ctypes.data_as(u64p), CAP_HEIGHT, C.byref(st)) == 0 and st.value == 0

    t_host = statistics.median(timed(host_loop) for _ in range(3))
    res["verify"] = {"n": N_OPEN, "gpu_host_pointers_ms": round(t_vh, 3), "gpu_device_ms": round(t_vd, 3), "gpu_device_paths_per_s": round(N_OPEN / t_vd * 1e3),
                     "host_loop_n": N_HOST, "host_loop_ms": round(t_host, 3), "host_loop_paths_per_s": round(N_HOST / t_host * 1e3)}
    L.p2_merkle_tree_free(tree)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
