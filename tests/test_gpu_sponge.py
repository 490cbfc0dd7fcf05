"""GPU tests (pytest -m gpu) of the tree kernels' sponge steps: k_hash_leaves, k_merkle_level and k_hash_fri_leaves, one launch
each, against the textbook overwrite-mode sponge over the CPU oracle's permutation, bit for bit.

The kernels leave out the S-boxes and MDS terms of words known to be zero (the capacity in front of a first chunk, a whole chunk
of columns >= active_cols) and the MDS rows of outputs the next chunk overwrites, so the shapes are the ones at which that
choice changes: a single chunk, a full second chunk, partial last chunks of 1, 2 and 7 words, `active_cols` inside a chunk, on a
chunk boundary, whole zero chunks, and a zero chunk in front of a partial last chunk; 300 leaves (two workgroups, the second
partly idle) and two proofs per launch."""
import ctypes as C
import random

import pytest

import sponge_ref as S

pytestmark = pytest.mark.gpu
P = S.P
LEAVES, BATCH = 300, 2


@pytest.fixture(scope="module")
def lib(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.fail("-m gpu tests need a GPU: the HIP path has no CPU fallback")
    return S.bind(pkg.lib())


def _words(r, n):
    return [r.choice(S.EXTREMES) if r.random() < 0.1 else r.randrange(P) for _ in range(n)]


def _leaf_cases():
    for cols in (5, 8, 9, 15, 16, 17, 34, 135):
        for active in [cols] + [a for a in (3, 8, 9, 16) + ((80,) if cols == 135 else ()) if a < cols]:
            yield cols, active


@pytest.mark.parametrize("cols,active", list(_leaf_cases()))
def test_hash_leaves(lib, orc, cols, active):
    r = random.Random(cols * 1000 + active)
    data = _words(r, BATCH * active * LEAVES)                      # [batch][active][leaves]: the zero columns are not stored
    out = (C.c_uint64 * (BATCH * LEAVES * 4))()
    assert lib.p2_gpu_hash_leaves((C.c_uint64 * len(data))(*data), cols, active, LEAVES, BATCH, out, 0) == 0, lib.p2_last_error()
    for b in range(BATCH):
        for leaf in range(LEAVES):
            row = [data[(b * active + c) * LEAVES + leaf] for c in range(active)] + [0] * (cols - active)
            o = 4 * (b * LEAVES + leaf)
            assert list(out[o:o + 4]) == S.hash_no_pad(orc, row), (cols, active, b, leaf)


def test_two_level_tree(lib, orc):
    """k_merkle_level twice: 1200 leaf digests -> 600 -> 300 nodes per proof, the second launch on the first one's output."""
    r = random.Random(7)
    level = [_words(r, 4 * 4 * LEAVES) for _ in range(BATCH)]
    for parents in (2 * LEAVES, LEAVES):
        flat = [w for lv in level for w in lv]
        out = (C.c_uint64 * (BATCH * parents * 4))()
        assert lib.p2_gpu_merkle_level((C.c_uint64 * len(flat))(*flat), parents, BATCH, out, 0) == 0, lib.p2_last_error()
        nxt = []
        for b in range(BATCH):
            got = list(out[b * parents * 4:(b + 1) * parents * 4])
            for i in range(parents):
                assert got[4 * i:4 * i + 4] == S.two_to_one(orc, level[b][8 * i:8 * i + 4], level[b][8 * i + 4:8 * i + 8]), (parents, b, i)
            nxt.append(got)
        level = nxt


@pytest.mark.parametrize("arity", [16, 8, 4])
def test_hash_fri_leaves(lib, orc, arity):
    """A leaf is `arity` consecutive extension values flattened (c0, c1): 32 words = four full chunks at the prover's arity 16."""
    r = random.Random(arity)
    n = LEAVES * arity
    vals = _words(r, BATCH * 2 * n)                                # [batch][2][len]
    out = (C.c_uint64 * (BATCH * LEAVES * 4))()
    assert lib.p2_gpu_hash_fri_leaves((C.c_uint64 * len(vals))(*vals), n, arity, BATCH, out, 0) == 0, lib.p2_last_error()
    for b in range(BATCH):
        for leaf in range(LEAVES):
            row = [vals[(2 * b + (e & 1)) * n + leaf * arity + (e >> 1)] for e in range(2 * arity)]
            o = 4 * (b * LEAVES + leaf)
            assert list(out[o:o + 4]) == S.hash_no_pad(orc, row), (arity, b, leaf)
