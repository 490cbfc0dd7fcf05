"""CPU tests of the block form of Poseidon's 22 partial rounds (poseidon_fast.h: partial_block; tools/gen_poseidon_fast.py):
the emitted tables against a derivation of their own, the accumulator and fold bounds of every row, and the host build of
partial_block (p2_host_partial_rounds) against the naive rounds -- on inputs chosen so that every fold of the loop body is
reached with and without its carry."""
import ctypes as C
import random

import pytest

import partial_rounds_ref as R
import sponge_ref as S

P = R.P


@pytest.fixture(scope="module")
def rc():
    return R.round_constants()


@pytest.fixture(scope="module")
def tab():
    return R.emitted_tables()


@pytest.fixture(scope="module")
def inputs(tab):
    """(states, per state the model's fold events): random and extreme states, and states searched with the halves model until
    every fold site has an input that carries.  Computed once."""
    rnd = random.Random(2205)
    states = [[0] * 12, [P - 1] * 12, [R.M64] * 12] + [[e] * 12 for e in S.EXTREMES]
    states += [[rnd.choice(S.EXTREMES + [R.M64, P, R.M64 - R.M32]) for _ in range(12)] for _ in range(16)]
    states += R.random_states(rnd, 400)    # a block-end row carries once in ~250 folds: 400 x 7 folds a row
    states += [R.carrying_row0_d1(tab, rnd) for _ in range(2)] + [R.carrying_row0_d2(tab, rnd) for _ in range(2)]
    return states, [R.halves(st, tab)[1] for st in states]


def test_emitted_tables_recomputed_from_the_round_constants(rc, tab):
    """(a) every table poseidon_fast.inc emits for the block form, recomputed from poseidon_rc.inc and the MDS definition by
    pushing unit vectors and constants through the naive linear steps: not with the generator's code."""
    want = R.derive(rc)
    assert len(tab["PB_ROW0_D2"]) == 12 and len(tab["PB_END"]) == 2 * 12 * 13 and len(tab["PB_K"]) == 8 * 14
    for name in want:
        assert tab[name] == want[name], name
    assert all(k < P for k in tab["PB_K"])
    assert tab["PB_K"][14 * 7 + 2:] == rc[12 * 26:12 * 27]   # the last block leaves round 26's constants
    # the coefficients the kernels hold as inline constants are what the derivation gives for them
    for r in range(12):
        assert R._linear_rounds([1] + [0] * 11, 1)[r] == R.mds_entry(r, 0) <= 64
    assert sorted(R.BLOCKS) == [1] + [3] * 7 and sum(R.BLOCKS) == 22


def test_every_row_keeps_its_accumulators_and_its_fold_in_64_bits(tab):
    """(b) worst case on arbitrary 32-bit halves: (sum of a row's coefficients, t-columns included) (2^32 - 1) + (2^32 - 1), the
    constant's half, stays below 2^64 -- and so do the fold's ah + (al >> 32) and its second step."""
    rows = [("row0", 1, [R.mds_entry(0, j) for j in range(12)]), ("row0", 2, tab["PB_ROW0_D2"] + [R.mds_entry(0, 0)])]
    for kind, size in ((0, 3), (1, 1)):
        for r in range(12):
            e = tab["PB_END"][13 * (12 * kind + r):13 * (12 * kind + r + 1)]
            rows.append(("end%d" % size, r, e + ([R.mds_entry(r, 0)] if size == 3 else [])))
    assert len(rows) == 26
    for name, r, coef in rows:
        assert all(0 <= c <= R.M32 for c in coef)
        acc = sum(coef) * R.M32 + R.M32
        assert acc < 1 << 64, (name, r)
        ah2 = acc + (acc >> 32)
        assert ah2 < 1 << 64, (name, r)
        assert (ah2 >> 32) * R.M32 + R.M32 < 1 << 64, (name, r)   # after a wrap the sum is < x2 (2^32 - 1): + (2^32 - 1) fits
        assert acc < 1 << 57, (name, r)                              # what poseidon_fast.h states for its fold


def test_the_inputs_reach_every_fold_with_and_without_a_carry(inputs):
    """The condition of (c), from the model alone: every fold site of the loop body -- row 0 at depth 1, at depth 2, the twelve
    rows of a block's end -- runs on at least one input that carries and on one that does not."""
    _, events = inputs
    for site in R.SITES:
        assert any(c for ev in events for _, s, c in ev if s == site), ("no carrying input", site)
        assert any(not c for ev in events for _, s, c in ev if s == site), ("no input without a carry", site)
    assert any(not R.carried_sites(ev) for ev in events)   # and a state that carries nowhere


def test_host_partial_rounds_against_the_naive_rounds(pkg, rc, tab, inputs):
    """(c) p2_host_partial_rounds, the host build of partial_block on the same tables, against the 22 naive rounds."""
    states, _ = inputs
    flat = [w for st in states for w in st]
    buf = (C.c_uint64 * len(flat))(*flat)
    assert pkg.lib().p2_host_partial_rounds(buf, len(states)) == 0
    for i, st in enumerate(states):
        got = [w % P for w in buf[12 * i:12 * i + 12]]
        assert got == R.naive(st, rc), i
        assert got == [w % P for w in R.halves(st, tab)[0]], i


def test_the_whole_permutation_still_matches_the_oracle(pkg, orc):
    rnd = random.Random(7)
    lib = S.bind(pkg.lib())
    states = [[rnd.randrange(P) for _ in range(12)] for _ in range(8)]
    buf = (C.c_uint64 * 96)(*[w for st in states for w in st])
    assert lib.p2_host_poseidon_known(buf, 8, 0, 0xFFF, 0) == 0
    for i, st in enumerate(states):
        assert list(buf[12 * i:12 * i + 12]) == S.permute(orc, st)
