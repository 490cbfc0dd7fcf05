"""GPU test (pytest -m gpu) of the merged middle of Poseidon: ONE launch of 256 states through p2_gpu_merged_middle
(k_merged_middle: merged_middle as the hash kernels compile it, five waves per SIMD), against round 3's MDS and the 22 naive rounds.
The kernel's outputs are some representative of each word; they are compared as field elements, all of them.

The second step of a rare fold (row 0 at depths 1, 2 and 3) sits behind a wave-uniform branch, so the four waves are chosen with the
halves model of merged_middle_ref.py:
  wave 0   lanes that take some rare fold and lanes that take none, alternating: the branch runs with a partial mask;
  wave 1   every lane takes some rare fold, and every rare site is among them;
  wave 2   no lane takes any rare fold: the branch is never taken;
  wave 3   extreme and random words.
The end rows fold branch-free, with the second step on every lane; waves 0..2 between them run every end row of both tables with
and without the carry of its first step."""
import ctypes as C
import random

import pytest

import merged_middle_ref as MM
import partial_rounds_ref as R
import sponge_ref as S

pytestmark = pytest.mark.gpu
P = R.P


def _rare(tab, st, rare):
    return MM.carried_sites(MM.halves(st, tab)[1]) & rare


def _waves(tab):
    rnd = random.Random(9206)
    rare = set(MM.rare_sites(tab))
    solved = [MM.carrying_row0_d1(tab, rnd) for _ in range(32)] + [MM.carrying_row0_d2(tab, rnd) for _ in range(32)]
    d3, plain = [], []   # row 0 at depth 3 carries once in some six hundred folds: found by trying
    while len(d3) < 2 or len(plain) < 96:
        st = R.random_states(rnd, 1)[0]
        got = _rare(tab, st, rare)
        if not got:
            plain.append(st)
        elif ("row0", 3) in got:
            d3.append(st)
        else:
            solved.append(st)
    carriers = d3 + solved
    w0 = [carriers[-1 - i // 2] if i % 2 else plain[i // 2] for i in range(64)]
    w1 = carriers[:64]
    w2 = plain[32:96]
    w3 = [[e] * 12 for e in S.EXTREMES + [R.M64, P, R.M64 - R.M32]] + [[rnd.choice(S.EXTREMES + [R.M64]) for _ in range(12)] for _ in range(20)]
    w3 += R.random_states(rnd, 64 - len(w3))
    return rare, w0, w1, w2, w3


def test_merged_middle_one_launch_four_waves(pkg):
    if pkg.lib().p2_gpu_device_count() <= 0:
        pytest.fail("-m gpu tests need a GPU: the HIP path has no CPU fallback")
    rc, tab = R.round_constants(), MM.emitted_tables()
    rare, w0, w1, w2, w3 = _waves(tab)
    assert [len(w) for w in (w0, w1, w2, w3)] == [64] * 4
    # what the waves are for, from the model: a silent loss of coverage fails here
    assert rare == {("row0", 1), ("row0", 2), ("row0", 3)}
    assert [bool(_rare(tab, st, rare)) for st in w0] == [bool(i % 2) for i in range(64)]
    s1 = [_rare(tab, st, rare) for st in w1]
    assert all(s1) and set().union(*s1) == rare
    assert not any(_rare(tab, st, rare) for st in w2)
    ends = {(s, c) for st in w0 + w1 + w2 for _, s, c in MM.halves(st, tab)[1] if s[0] == "end4"}
    assert ends == {(("end4", r), c) for r in range(12) for c in (False, True)}
    states = w0 + w1 + w2 + w3
    buf = (C.c_uint64 * (12 * 256))(*[w for st in states for w in st])
    assert pkg.lib().p2_gpu_merged_middle(buf, 256, 0) == 0, pkg.lib().p2_last_error()
    for i, st in enumerate(states):
        assert [w % P for w in buf[12 * i:12 * i + 12]] == MM.naive(st, rc), (i // 64, i % 64)
