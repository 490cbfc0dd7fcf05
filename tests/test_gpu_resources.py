"""Who frees what: p2_debug_live_resources() -- the device allocations, pinned allocations, streams and events the library's
owners hold -- returns to where it started when a circuit handle, a stand-alone Merkle tree or a primitive call goes, whatever ran
in between: every host entry point, a change of the chunk options (workspaces made under the old value are replaced, not added
to), an injected allocation failure, two threads on one handle.  The counter is the library's own, so other jobs on the device
do not show in it.  Circuit: gf_2_8_mul, the smallest the suite has; batches of 2 and 3."""
import ctypes as C
import gc
import threading

import pytest

import circuits

pytestmark = pytest.mark.gpu

TRIPLES = [(0x57, 0x13, 0xFE), (0x57, 0x83, 0xC1), (1, 1, 1)]


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.skip("no HIP device")
    return pkg


def live(gpu):
    gc.collect()  # a handle of an earlier test that is only now collected must not be freed between two readings
    return gpu.lib().p2_debug_live_resources()


def free(gpu, data):
    gpu.lib().p2_circuit_free(data._gpu)
    data._gpu = None


def verify_and_witness(data, pws, proofs, outs):
    assert data.verify_batch(proofs) == [0] * len(proofs)
    vals, st = data.generate_witness(pws, outs)
    assert st == [0] * len(pws) and [v[-1] for v in vals] == [t[2] for t in TRIPLES[:len(pws)]]


def test_everything_goes_when_the_handle_goes(gpu):
    L = gpu.lib()
    base = live(gpu)
    data, pws = circuits.gf_2_8_mul(gpu, TRIPLES)
    outs = list(pws[0].map)  # x, y, xy
    data.gpu()
    assert live(gpu) > base
    proofs, st = data.prove_batch(pws)
    assert st == [0, 0, 0]
    again, st, vals = data.prove_batch(pws[:2], outputs=outs)
    assert st == [0, 0] and again == proofs[:2] and vals == [list(t) for t in TRIPLES[:2]]
    verify_and_witness(data, pws, proofs, outs)
    cps, st = data.compress_batch(proofs)
    assert st == [0, 0, 0] and cps == [data.compress(p) for p in proofs]
    assert data.decompress_batch(cps) == (proofs, [0, 0, 0])
    assert data.verify_compressed_batch(cps) == [0, 0, 0]
    flags = (C.c_uint32 * 3)(*([0xFFFFFFFF] * 3))
    assert L.p2_gpu_vanishing_flags(data.gpu(), 3, b"".join(proofs), (C.c_uint64 * 48)(), (C.c_uint64 * 12)(), flags) == 0, L.p2_last_error()
    assert data.explain(pws[0]).kind == "NONE"
    data.set_option("verify_chunk", 2)   # the workspaces in the pools are stale now: the next calls replace them
    data.set_option("witness_chunk", 2)
    verify_and_witness(data, pws, proofs, outs)
    assert live(gpu) > base
    free(gpu, data)
    assert live(gpu) == base


def test_a_tree_and_a_primitive_call_take_their_own_with_them(gpu):
    L = gpu.lib()
    base = live(gpu)
    leaves = [[(5 * i + j) % 251 for j in range(3)] for i in range(8)]
    tree = gpu.MerkleTree(leaves, cap_height=1, device=0)
    assert live(gpu) > base
    trace = tree.update(5, [7, 8, 9], trace=True)
    assert trace is not None
    leaves[5] = [7, 8, 9]
    assert tree.prove(5) == gpu.MerkleTree(leaves, cap_height=1, device=None).prove(5)
    L.p2_merkle_tree_free(tree._h)
    tree._h = None
    assert live(gpu) == base
    vals, out = (C.c_uint64 * 16)(*range(16)), (C.c_uint64 * 16)()
    assert L.p2_gpu_intt(vals, 2, 3, out, 0) == 0, L.p2_last_error()
    assert live(gpu) == base


def test_a_stale_workspace_is_replaced_not_added(gpu):
    data, pws = circuits.gf_2_8_mul(gpu, TRIPLES)
    outs = list(pws[0].map)
    proofs, st = data.prove_batch(pws)
    assert st == [0, 0, 0]
    counts = {}
    for opt, values, call in (("verify_chunk", (3, 7), lambda: data.verify_batch(proofs)), ("witness_chunk", (2, 5), lambda: data.generate_witness(pws, outs)[1])):
        for v in values:
            data.set_option(opt, v)
            assert call() == [0, 0, 0]
            counts[opt, v] = live(gpu)
    assert counts["verify_chunk", 3] == counts["verify_chunk", 7]
    assert counts["witness_chunk", 2] == counts["witness_chunk", 5]
    free(gpu, data)


def test_nothing_is_left_after_an_injected_allocation_failure(gpu, monkeypatch):
    base = live(gpu)
    monkeypatch.setenv("P2AES_TEST_FAIL_ALLOC_AFTER", "17")
    data, pws = circuits.gf_2_8_mul(gpu, TRIPLES[:2])
    data.gpu()                                      # the hook is read when the handle is loaded
    monkeypatch.delenv("P2AES_TEST_FAIL_ALLOC_AFTER")
    loaded = live(gpu)
    with pytest.raises(gpu.P2Error, match="workspace allocation failed .*injected allocation failure"):
        data.prove_batch(pws)
    # the half-built workspaces went, with the 17 allocations that had succeeded; what the call leaves is its staging set, back in
    # the pool: a stream and three device/pinned pairs (values, proofs, statuses; no outputs were asked for)
    assert live(gpu) == loaded + 7
    proofs, st = data.prove_batch(pws)              # one-shot hook: the retry allocates every buffer again
    assert st == [0, 0]
    for p in proofs:
        data.verify(p)
    free(gpu, data)
    assert live(gpu) == base


def test_two_threads_on_one_handle(gpu):
    base = live(gpu)
    data, pws = circuits.gf_2_8_mul(gpu, TRIPLES)
    outs = list(pws[0].map)
    proofs, st = data.prove_batch(pws)
    assert st == [0, 0, 0]
    errors = []

    def work():
        try:
            for _ in range(10):
                verify_and_witness(data, pws, proofs, outs)
        except BaseException as e:  # noqa: B902 -- carried to the test's thread
            errors.append(e)

    threads = [threading.Thread(target=work) for _ in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    free(gpu, data)
    assert live(gpu) == base
