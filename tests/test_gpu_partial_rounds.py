"""GPU test (pytest -m gpu) of the block form of Poseidon's partial rounds: ONE launch of 256 states through
p2_gpu_partial_rounds (k_partial_rounds: partial_block as the hash kernels compile it, five waves per SIMD), against the 22 naive
rounds.  The kernel's outputs are some representative of each word; they are compared as field elements, all of them.

The second step of every fold sits behind a wave-uniform branch, so the four waves are chosen with the halves model of
partial_rounds_ref.py:
  wave 0   lanes that carry at some fold and lanes that carry nowhere, alternating: the branch runs with a partial mask;
  wave 1   every lane carries at some fold, and every fold site (row 0 at depths 1 and 2, the twelve end rows) is among them;
  wave 2   no lane carries anywhere: the branch is never taken;
  wave 3   random and extreme words."""
import ctypes as C
import random

import pytest

import partial_rounds_ref as R
import sponge_ref as S

pytestmark = pytest.mark.gpu
P = R.P


def _waves(tab):
    rnd = random.Random(9107)
    solved = [R.carrying_row0_d1(tab, rnd) for _ in range(4)] + [R.carrying_row0_d2(tab, rnd) for _ in range(4)]
    by_row, carriers, plain = {}, [], []   # one carrying state per end row, further carrying states, states that carry nowhere
    while len(by_row) < 12 or len(carriers) < 76 or len(plain) < 96:
        st = R.random_states(rnd, 1)[0]
        sites = R.carried_sites(R.halves(st, tab)[1])
        new = sorted(r for kind, r in sites if kind == "end" and r not in by_row)
        if not sites:
            plain.append(st)
        elif new:
            by_row[new[0]] = st
        else:
            carriers.append(st)
    w0 = [carriers[44 + i // 2] if i % 2 else plain[i // 2] for i in range(64)]
    w1 = solved + [by_row[r] for r in range(12)] + carriers[:44]
    w2 = plain[32:96]
    w3 = [[e] * 12 for e in S.EXTREMES + [R.M64, P, R.M64 - R.M32]] + [[rnd.choice(S.EXTREMES + [R.M64]) for _ in range(12)] for _ in range(20)]
    w3 += R.random_states(rnd, 64 - len(w3))
    return w0, w1, w2, w3


def test_partial_rounds_one_launch_four_waves(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.fail("-m gpu tests need a GPU: the HIP path has no CPU fallback")
    rc, tab = R.round_constants(), R.emitted_tables()
    w0, w1, w2, w3 = _waves(tab)
    assert [len(w) for w in (w0, w1, w2, w3)] == [64] * 4
    # what the waves are for, from the model: a silent loss of coverage fails here
    c0 = [bool(R.carried_sites(R.halves(st, tab)[1])) for st in w0]
    assert c0 == [bool(i % 2) for i in range(64)]
    s1 = [R.carried_sites(R.halves(st, tab)[1]) for st in w1]
    assert all(s1) and set().union(*s1) == set(R.SITES)
    assert not any(R.carried_sites(R.halves(st, tab)[1]) for st in w2)
    states = w0 + w1 + w2 + w3
    buf = (C.c_uint64 * (12 * 256))(*[w for st in states for w in st])
    assert pkg.lib().p2_gpu_partial_rounds(buf, 256, 0) == 0, pkg.lib().p2_last_error()
    for i, st in enumerate(states):
        assert [w % P for w in buf[12 * i:12 * i + 12]] == R.naive(st, rc), (i // 64, i % 64)
