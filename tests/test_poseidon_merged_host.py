"""CPU tests of the merged middle of Poseidon (poseidon_fast.h: merged_middle; tools/gen_poseidon_fast.py): round 3's MDS and the 22
partial rounds as one chain of 23 linear layers in blocks of up to four.  The emitted tables against a derivation of their own, the
three 64-bit bounds and the choice of fold of every emitted row, the host build (p2_host_merged_middle) against the naive rounds on
inputs that reach every fold of the loop body with and without its carry, and the whole permutation against the oracle."""
import ctypes as C
import random

import pytest

import merged_middle_ref as MM
import partial_rounds_ref as R
import sponge_ref as S

P = R.P


@pytest.fixture(scope="module")
def rc():
    return R.round_constants()


@pytest.fixture(scope="module")
def tab():
    return MM.emitted_tables()


@pytest.fixture(scope="module")
def inputs(tab):
    """(states, per state the model's fold events): extreme and random states, states solved for a carry at row 0 of depths 1 and 2,
    and random states tried until row 0 at depth 3 and every end row of the depth-3 table (a carry in some hundreds of folds each)
    have carried.  Computed once."""
    rnd = random.Random(2306)
    states = [[0] * 12, [P - 1] * 12, [R.M64] * 12] + [[e] * 12 for e in S.EXTREMES]
    states += [[rnd.choice(S.EXTREMES + [R.M64, P, R.M64 - R.M32]) for _ in range(12)] for _ in range(16)]
    states += R.random_states(rnd, 64)
    states += [MM.carrying_row0_d1(tab, rnd) for _ in range(2)] + [MM.carrying_row0_d2(tab, rnd) for _ in range(2)]
    events = [MM.halves(st, tab)[1] for st in states]
    missing = set(MM.SITES) - set().union(*(MM.carried_sites(ev) for ev in events))
    for _ in range(40000):   # expected: about three thousand
        if not missing:
            break
        st = R.random_states(rnd, 1)[0]
        ev = MM.halves(st, tab)[1]
        if MM.carried_sites(ev) & missing:
            missing -= MM.carried_sites(ev)
            states.append(st)
            events.append(ev)
    return states, events


def test_emitted_tables_recomputed_from_the_round_constants(rc, tab):
    """(a) the partition and every table poseidon_fast.inc emits for the merged middle, recomputed from poseidon_rc.inc and the MDS
    definition by pushing unit vectors and constants through the naive linear steps: not with the generator's code."""
    depths = tab["PM_DEPTH"]
    assert sum(depths) == 23 and max(depths) <= 4 and min(depths) >= 1
    assert depths == [4] * 5 + [3]   # what the loop body assumes: a trip that is not four deep is three deep, and comes last
    want = MM.derive(rc, depths)
    assert len(tab["PM_ROW0_D3"]) == 13 and len(tab["PM_END"]) == 2 * 12 * 14 and len(tab["PM_K"]) == 6 * 15
    for name in want:
        assert tab[name] == want[name], name
    assert all(k < P for k in tab["PM_K"])
    assert tab["PM_K"][0] == rc[48]   # the first block's K_1 is round 4's constant: what mds_full(.., RC + 48) added
    # the last block's end carries round 26's constants on top of the earlier ones pushed through
    last = tab["PM_K"][15 * 5:]
    x = [0] * 12
    for i in (1, 2):
        x = [(a + rc[12 * (23 + i) + k]) % P for k, a in enumerate(R.mds_apply([0] + x[1:], P))]
    assert last[3:] == [(a + rc[12 * 26 + k]) % P for k, a in enumerate(R.mds_apply([0] + x[1:], P))]
    # the coefficients the kernels hold as inline constants are what the derivation gives for them
    e0 = [1] + [0] * 11
    for r in range(12):
        assert R._linear_rounds(e0, 1)[r] == R.mds_entry(r, 0) <= 64
        assert tab["PM_END"][14 * (12 + r) + 1] == R.mds_entry(r, 0)   # depth 3: the slot of t_2, the last real t
    # the figures the depth was chosen by
    end4 = [c for s, c in MM.emitted_rows(tab) if s[0] == "end4"]
    assert max(max(c) for c in end4) == 317240928
    assert max(sum(c[2:14]) for c in end4) == 3534187520 and max(sum(c) for c in end4) == 3535450306


def test_every_row_keeps_its_bounds_and_gets_the_right_fold(tab):
    """(b) worst case on arbitrary 32-bit halves: (sum of a row's coefficients, t-columns included) (2^32 - 1) + (2^32 - 1), the
    constant's half, stays below 2^64; so do the fold's ah + (al >> 32) and, after a wrap, + (2^32 - 1).  The generator's choice of
    fold: the rare-carry branch only where x2 < 2^26 (what fold_al_ah states for it), the always-on second step elsewhere."""
    rows = MM.emitted_rows(tab)
    assert [s for s, _ in rows] == MM.SITES and len(rows) == 27
    for site, coef in rows:
        assert all(0 <= c <= R.M32 for c in coef), site
        acc = sum(coef) * R.M32 + R.M32
        assert acc < 1 << 64, site
        ah2 = acc + (acc >> 32)
        assert ah2 < 1 << 64, site
        x2 = ah2 >> 32
        assert x2 * R.M32 + R.M32 < 1 << 64, site   # after a wrap the sum is < x2 (2^32 - 1): + (2^32 - 1) fits
        assert MM.always_flag(tab, site) == (x2 >= 1 << 26), site
    # as the generator reports it: every end row at depth 4 always, nothing else
    assert (tab["PM_ALWAYS_ROW0"], tab["PM_ALWAYS_END4"], tab["PM_ALWAYS_END3"]) == (0, 0xFFF, 0)
    assert MM.rare_sites(tab) == MM.SITES[:3]   # the end rows are one copy for both tables and run the always form


def test_the_inputs_reach_every_fold_with_and_without_a_carry(inputs):
    """The condition of (c), from the model alone: every fold site of the loop body -- row 0 at depths 1, 2 and 3, the twelve end
    rows on the depth-4 table and on the depth-3 table -- runs on at least one input that carries and on one that does not."""
    _, events = inputs
    for site in MM.SITES:
        assert any(c for ev in events for _, s, c in ev if s == site), ("no carrying input", site)
        assert any(not c for ev in events for _, s, c in ev if s == site), ("no input without a carry", site)
    assert {s for ev in events for _, s, _ in ev} == set(MM.SITES)


def test_host_merged_middle_against_the_naive_rounds(pkg, rc, tab, inputs):
    """(c) p2_host_merged_middle, the host build of merged_middle on the same tables, against M z + c4 and the 22 naive rounds."""
    states, _ = inputs
    flat = [w for st in states for w in st]
    buf = (C.c_uint64 * len(flat))(*flat)
    assert pkg.lib().p2_host_merged_middle(buf, len(states)) == 0
    for i, st in enumerate(states):
        got = [w % P for w in buf[12 * i:12 * i + 12]]
        assert got == MM.naive(st, rc), i
        assert got == [w % P for w in MM.halves(st, tab)[0]], i


def test_the_whole_permutation_still_matches_the_oracle(pkg, orc):
    """(d) general kind, all rows, through both arrangements of the round loops."""
    rnd = random.Random(8)
    lib = S.bind(pkg.lib())
    states = [[rnd.randrange(P) for _ in range(12)] for _ in range(8)]
    for parts in (0, 1):
        buf = (C.c_uint64 * 96)(*[w for st in states for w in st])
        assert lib.p2_host_poseidon_known(buf, 8, 0, 0xFFF, parts) == 0
        for i, st in enumerate(states):
            assert list(buf[12 * i:12 * i + 12]) == S.permute(orc, st), (parts, i)
