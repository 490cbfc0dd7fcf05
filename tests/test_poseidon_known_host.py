"""CPU tests of the permutation with known-zero inputs and masked outputs (poseidon_fast.h: first_round / middle / last_round,
permute_known, sponge_permute) through the host build of the same functions, against the CPU oracle's plain permutation."""
import ctypes as C
import os
import random
import re

import pytest

import sponge_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plonky2-aes_amd", "csrc")
P = S.P
KNOWN = {0: [], 1: [8, 9, 10, 11], 2: list(range(8))}   # FR_GENERAL, FR_ZERO_CAP, FR_ZERO_RATE: the words that enter as 0
# all; the digest; the capacity (a full chunk follows); a chunk of m < 8 words follows; k_pow's word 7
MASKS = [0xFFF, 0x00F, 0xF00] + [(0xFF & ~((1 << m) - 1)) | 0xF00 for m in range(1, 8)] + [1 << 7]


@pytest.fixture(scope="module")
def lib(pkg):
    return S.bind(pkg.lib())


def _states(seed, n):
    """Random canonical states, states of extreme words, and a few non-canonical representatives (>= p)."""
    r = random.Random(seed)
    out = [[e] * 12 for e in S.EXTREMES]
    out += [[r.choice(S.EXTREMES) for _ in range(12)] for _ in range(n // 4)]
    out += [[r.randrange(P) for _ in range(12)] for _ in range(n)]
    out += [[r.randrange(P, 1 << 64) if k % 3 == 0 else r.randrange(P) for k in range(12)] for _ in range(8)]
    return out


@pytest.fixture(scope="module")
def reference(orc):
    """kind -> (states with the known words at 0, their plain permutations): computed once."""
    ref = {}
    for kind, known in KNOWN.items():
        states = [[0 if k in known else w for k, w in enumerate(st)] for st in _states(100 + kind, 48)]
        ref[kind] = (states, [S.permute(orc, [w % P for w in st]) for st in states])
    return ref


@pytest.mark.parametrize("parts", [0, 1])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_every_mask_and_first_round_variant_on_the_kept_words(lib, reference, kind, parts):
    states, want = reference[kind]
    r = random.Random(kind)
    for rows in MASKS:
        # the words declared zero are not read: hand them garbage
        flat = [r.randrange(1 << 64) if k in KNOWN[kind] else w for st in states for k, w in enumerate(st)]
        buf = (C.c_uint64 * len(flat))(*flat)
        assert lib.p2_host_poseidon_known(buf, len(states), kind, rows, parts) == 0
        for i, w in enumerate(want):
            got = list(buf[12 * i:12 * i + 12])
            kept = [k for k in range(12) if (rows >> k) & 1]
            assert [got[k] for k in kept] == [w[k] for k in kept], (kind, hex(rows), parts, i)


def test_known_answer_and_argument_checks(lib):
    buf = (C.c_uint64 * 12)()
    assert lib.p2_host_poseidon_known(buf, 1, 1, 0xFFF, 0) == 0
    assert buf[0] == 0x3C18A9786CB0B359   # upstream test vector, all-zero input (a zero capacity in particular)
    assert lib.p2_host_poseidon_known(buf, 1, 3, 0xFFF, 0) != 0
    assert lib.p2_host_poseidon_known(buf, 1, 0, 0, 0) != 0
    assert lib.p2_host_poseidon_known(buf, 1, 0, 0x1000, 0) != 0


def _cases():
    for cols in (1, 4, 5, 8, 9, 15, 16, 17, 24, 34, 135):
        for active in sorted({cols, 0, 3, 8, 9, 16, 80} - {a for a in (3, 8, 9, 16, 80) if a > cols}):
            yield cols, active


@pytest.mark.parametrize("cols,active", list(_cases()))
def test_sponge_steps_against_the_textbook_sponge(lib, orc, pkg, cols, active):
    """hash_or_noop of rows whose columns >= active are zero: chunk 0 on a zero capacity, whole zero chunks as a zero rate, a
    chunk straddling `active` and a zero chunk in front of a partial last chunk, every kept-row mask."""
    r = random.Random(cols * 1000 + active)
    leaves = 5
    data = [r.choice(S.EXTREMES) if r.random() < 0.2 else r.randrange(P) for _ in range(max(active, 1) * leaves)]
    out = (C.c_uint64 * (4 * leaves))()
    assert lib.p2_host_hash_leaves((C.c_uint64 * len(data))(*data), cols, active, leaves, out) == 0
    for leaf in range(leaves):
        row = [data[c * leaves + leaf] if c < active else 0 for c in range(cols)]
        want = S.hash_or_noop(orc, row)
        assert list(out[4 * leaf:4 * leaf + 4]) == want, (cols, active, leaf)
        if cols > 4:   # and the product's own textbook sponge over gl::poseidon
            o = (C.c_uint64 * 4)()
            pkg.lib().p2_native_hash_n_to_m_no_pad((C.c_uint64 * cols)(*row), cols, o, 4)
            assert list(o) == want


def _table(text, name):
    m = re.search(r"%s\[[^\]]*\]\s*=\s*\{(.*?)\};" % name, text, flags=re.S)
    return [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]+)ULL", m.group(1))]


def test_generated_addend_tables_recomputed_from_the_round_constants():
    """RC1_ZCAP[r] = RC[12 + r] + sum_{k in 8..11} M[r][k] RC[k]^7 and RC1_ZRATE likewise over k in 0..7, canonical: recomputed
    here from poseidon_rc.inc and the MDS definition, not with the generator's code."""
    rc = [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]+)ULL", open(os.path.join(CSRC, "poseidon_rc.inc")).read())]
    assert len(rc) == 360 and rc[0] == 0xB585F766F2144405
    inc = open(os.path.join(CSRC, "poseidon_fast.inc")).read()
    circ = [17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20]
    for name, known in (("RC1_ZCAP", range(8, 12)), ("RC1_ZRATE", range(0, 8))):
        tab = _table(inc, name)
        assert len(tab) == 12 and all(x < P for x in tab)
        for r in range(12):
            acc = rc[12 + r]
            for k in known:
                m_rk = circ[(k - r) % 12] + (8 if r == k == 0 else 0)
                acc += m_rk * pow(rc[k], 7, P)
            assert tab[r] == acc % P, (name, r)
