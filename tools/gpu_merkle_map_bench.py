#!/usr/bin/env python3
"""MerkleMap on one GPU, one process, every timed call ended by a stream synchronisation, medians of MERKLE_MAP_BENCH_REPEATS (5)
with the range after a warm-up round, the forms alternated (every round runs every form once):

  build            p2_merkle_map_new_device (validation, both sorts, the one read-back, allocation, leaves, one launch per
                   level, the cap) for N = 2^12, 2^16, 2^20 random keys at D = 64 and D = 24, values of 4 words (one
                   permutation per leaf); permutations/s counts the leaves and p2_merkle_map_hashes
  dense            D = 20, N = 2^20: the same tree as MerkleTree over value | 1, built beside it by p2_gpu_merkle_build_device
                   with the transpose -- the price of keeping ids and searching
  get, verify      p2_merkle_map_get_batch_device and p2_merkle_map_verify_batch_device, 2^16 queries against the D = 64,
                   N = 2^20 map, half of them present
  host             p2_native_merkle_map_cap on one core, N = 2^12, D = 64

Appends one JSON line to profiles/merkle_map_bench.jsonl."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("MERKLE_MAP_BENCH_OUT", os.path.join(ROOT, "profiles", "merkle_map_bench.jsonl"))
REPEATS = int(os.environ.get("MERKLE_MAP_BENCH_REPEATS", "5"))
MAX_BITS = int(os.environ.get("MERKLE_MAP_BENCH_BITS", "20"))
V, QUERIES = 4, 1 << 16
P = 0xFFFFFFFF00000001


def field(rng, shape):
    return (rng.integers(0, 1 << 63, size=shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=shape, dtype=np.uint64)) % np.uint64(P)


def distinct_keys(rng, key_bits, n):
    if key_bits < 64:
        return rng.choice(1 << key_bits, size=n, replace=False).astype(np.uint64)
    keys = np.unique(field(rng, 2 * n))
    rng.shuffle(keys)
    return keys[:n].copy()


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    pkg = g.load_package()
    L = pkg.lib()
    assert L.p2_gpu_device_count() > 0, "no HIP device"
    rng = np.random.default_rng(11)
    u64p, vp = C.POINTER(C.c_uint64), C.c_void_p

    H = C.CDLL(next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln))
    H.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
    H.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
    H.hipStreamCreate.argtypes = [C.POINTER(vp)]
    H.hipStreamSynchronize.argtypes = [vp]

    def dalloc(nbytes, host=None):
        p = vp()
        assert H.hipMalloc(C.byref(p), max(nbytes, 8)) == 0
        if host is not None:
            assert H.hipMemcpy(p, host.ctypes.data_as(vp), host.nbytes, 1) == 0
        return p

    s = vp()
    assert H.hipStreamCreate(C.byref(s)) == 0

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        assert H.hipStreamSynchronize(s) == 0
        return 1e3 * (time.perf_counter() - t0)

    sizes = [b for b in (12, 16, 20) if b <= MAX_BITS]
    configs = [(64, b) for b in sizes] + [(24, b) for b in sizes] + [(MAX_BITS, MAX_BITS)]
    data = {}
    for D, b in configs:
        keys = distinct_keys(rng, D, 1 << b)
        vals = field(rng, (1 << b, V))
        data[(D, b)] = (keys, vals, dalloc(keys.nbytes, keys), dalloc(vals.nbytes, vals))

    def build(D, b):
        keys, vals, d_keys, d_vals = data[(D, b)]
        h = vp()
        assert L.p2_merkle_map_new_device(d_keys, d_vals, 1 << b, V, D, 0, 0, s, C.byref(h)) == 0, L.p2_last_error()
        return h

    # the dense tree beside the dense map: leaves value | 1 in key order
    dk, dv = data[(MAX_BITS, MAX_BITS)][:2]
    n_dense = 1 << MAX_BITS
    leaves = np.ones((n_dense, V + 1), dtype=np.uint64)
    leaves[dk.astype(np.int64), :V] = dv
    d_leaves, d_scratch, d_dig = dalloc(leaves.nbytes, leaves), dalloc(leaves.nbytes), dalloc(64 * n_dense)

    def tree():
        assert L.p2_gpu_merkle_build_device(d_leaves, n_dense, V + 1, 0, 1, d_scratch, d_dig, 0, s) == 0, L.p2_last_error()

    res = {"value_len": V, "repeats": REPEATS, "build": {}}
    runs, hashes = {c: [] for c in configs}, {}
    runs["tree"] = []
    handle = [None]
    for rep in range(REPEATS + 1):                  # the first round warms up
        for c in configs:
            t = timed(lambda: handle.__setitem__(0, build(*c)))
            if rep:
                runs[c].append(t)
            hv = C.c_uint64()
            assert L.p2_merkle_map_hashes(handle[0], C.byref(hv)) == 0
            hashes[c] = hv.value
            L.p2_merkle_map_free(handle[0])
        t = timed(tree)
        if rep:
            runs["tree"].append(t)

    def stats(v):
        return {"ms": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

    for c in configs:
        D, b = c
        row = stats(runs[c])
        row["hashes"] = hashes[c]
        row["perm_per_s"] = round(((1 << b) + hashes[c]) / row["ms"] * 1e3)
        row["levels"] = D
        res["build"]["D%d N2^%d" % c] = row
        print(c, row, flush=True)
    res["dense_tree"] = stats(runs["tree"])
    res["dense_tree"]["perm_per_s"] = round((2 * n_dense - 1) / res["dense_tree"]["ms"] * 1e3)
    print("tree", res["dense_tree"], flush=True)

    # ---- lookups and path checks on the largest D = 64 map
    D, b = 64, max(sizes)
    keys = data[(D, b)][0]
    m = build(D, b)
    q = np.concatenate([keys[:QUERIES // 2], distinct_keys(rng, 64, QUERIES // 2)])
    rng.shuffle(q)
    stride = 1 + V + 4 * D
    d_q, d_rows, d_st = dalloc(q.nbytes, q), dalloc(8 * stride * QUERIES), dalloc(4 * QUERIES)
    cap = np.zeros(4, dtype=np.uint64)
    assert L.p2_merkle_map_cap(m, cap.ctypes.data_as(u64p), 4) == 0

    def get():
        assert L.p2_merkle_map_get_batch_device(m, d_q, QUERIES, d_rows, stride, 0, 1, 1 + V, d_st, s) == 0, L.p2_last_error()

    get()
    assert H.hipStreamSynchronize(s) == 0
    rows = np.empty((QUERIES, stride), dtype=np.uint64)
    assert H.hipMemcpy(rows.ctypes.data_as(vp), d_rows, rows.nbytes, 2) == 0
    present = np.ascontiguousarray(rows[:, 0])
    d_f, d_v, d_s, d_c = dalloc(present.nbytes, present), dalloc(8 * V * QUERIES, np.ascontiguousarray(rows[:, 1:1 + V])), \
        dalloc(32 * D * QUERIES, np.ascontiguousarray(rows[:, 1 + V:])), dalloc(32, cap)

    def verify():
        assert L.p2_merkle_map_verify_batch_device(d_q, D, d_f, d_v, V, d_s, d_c, 0, QUERIES, d_st, 0, s) == 0, L.p2_last_error()

    runs = {"get": [], "verify": []}
    for rep in range(REPEATS + 1):
        for name, fn in (("get", get), ("verify", verify)):
            t = timed(fn)
            if rep:
                runs[name].append(t)
    st = np.empty(QUERIES, dtype=np.int32)
    assert H.hipMemcpy(st.ctypes.data_as(vp), d_st, st.nbytes, 2) == 0 and not st.any()
    res["queries"] = {"count": QUERIES, "present": int(present.sum()), "map": "D%d N2^%d" % (D, b), "get": stats(runs["get"]), "verify": stats(runs["verify"])}
    res["queries"]["verify"]["perm_per_s"] = round(QUERIES * D / res["queries"]["verify"]["ms"] * 1e3)
    print(res["queries"], flush=True)
    L.p2_merkle_map_free(m)

    # ---- the host twin on one core
    keys, vals = data[(64, 12)][:2]
    t0 = time.perf_counter()
    assert L.p2_native_merkle_map_cap(keys.ctypes.data_as(u64p), vals.ctypes.data_as(u64p), len(keys), V, 64, 0, cap.ctypes.data_as(u64p)) == 0, L.p2_last_error()
    ms = 1e3 * (time.perf_counter() - t0)
    res["host"] = {"map": "D64 N2^12", "ms": round(ms, 1), "us_per_perm": round(1e3 * ms / (len(keys) + hashes[(64, 12)]), 2)}
    print("host", res["host"], flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
