#!/usr/bin/env python3
"""Derive the constants of two rewritten forms of Poseidon's 22 partial rounds and check both against the naive permutation.

1. The sparse-matrix form (fewest multiplications; every constant a full field element).  It serves poseidon_coop, the
   one-word-per-lane Fiat-Shamir chain, where a multiplication costs the same whatever its constant.

Naive partial round i:   s += c_i ; s0 = s0^7 ; s = M s        (M = 12x12 MDS)
Rewritten (exactly equivalent):
    s[1..] = D0 s[1..]                       dense 11x11, once
    for i in 0..22:  s0 = (s0 + a_i)^7
                     (s0, s[1..]) = (25 s0 + what_i . s[1..],  s[1..] + v_i s0)
    s += L                                   folded into the next full round's constants
Derivation: (A) the non-S-box parts of each round constant commute with the S-box and are pushed forward through M;
(B) M = [[m00, w],[v, Mh]] factors as [[m00, w Mh^-1],[v, I]] . diag(1, Mh); diag(1, Mh) commutes with the partial S-box
and is merged into the previous round's matrix, recursively, from the last round backwards.

2. The block form (derive_blocks): blocks of up to three rounds evaluated on 32-bit halves with small integer coefficients,
   for the thread-per-sponge kernels, where a term with a 64-bit constant costs 8 issue slots (12 with its reduction) and a
   term with a small coefficient 2.  With M the MDS matrix, Z = diag(0, 1, .., 1) and a state x that carries round r's
   constants, let y = (x_0^7, x_1, .., x_11).  Then, over the integers apart from the constants K_i,
       x(1) = M y + K_1
       x(2) = MZM y + (M e0) t_1 + K_2                      t_i = (x(i)_0)^7
       x(3) = MZMZM y + (MZM e0) t_1 + (M e0) t_2 + K_3     K_i = MZ K_(i-1) + c_(r+i) mod p,  K_0 = 0
   Only row 0 of the depths inside a block is needed (it feeds the next S-box); all twelve rows are evaluated once, at the
   block's end.  The matrices are the same for every block, only the K_i differ, and the last block's K carries round 26's
   constants.  Every coefficient is a small non-negative integer: a row's two half-accumulators stay far below 2^64 for
   arbitrary u64 state words (block_bounds proves it, and the bound of the fold that follows, for every row emitted).

3. The merged middle (MERGED, merged_tables): the block form again, over 23 linear layers instead of 22.  The MDS of the last
   full round in front of the partial rounds (round 3) is one more M in front of the chain [S-box on word 0, M] x 22, with
   y = round 3's twelve S-box outputs and round 4's constants as its K_1, so it opens the first block instead of running on its
   own.  The blocks are up to four layers deep:
       x(4) = MZMZMZM y + (MZMZM e0) t_1 + (MZM e0) t_2 + (M e0) t_3 + K_4
   whose coefficients stay below 2^29 and whose rows sum to less than 2^32: a half-accumulator still fits 64 bits (depth 5
   does not: its coefficients need 37 bits), but the fold's x2 is no longer small, so its second step runs on every lane
   instead of behind a rare branch (row_fold decides that per emitted row, and proves the bounds either way).
"""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_poseidon_constants import MDS_CIRC, MDS_DIAG, P, constants, permute  # noqa: E402

W = 12


def matmul(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(len(B))) % P for j in range(len(B[0]))] for i in range(len(A))]


def matvec(A, v):
    return [sum(A[i][k] * v[k] for k in range(len(v))) % P for i in range(len(A))]


def inverse(A):
    n = len(A)
    a = [row[:] + [int(i == j) for j in range(n)] for i, row in enumerate(A)]
    for c in range(n):
        piv = next(r for r in range(c, n) if a[r][c])
        a[c], a[piv] = a[piv], a[c]
        inv = pow(a[c][c], P - 2, P)
        a[c] = [x * inv % P for x in a[c]]
        for r in range(n):
            if r != c and a[r][c]:
                f = a[r][c]
                a[r] = [(x - f * y) % P for x, y in zip(a[r], a[c])]
    return [row[n:] for row in a]


def derive():
    rc = constants()
    M = [[(MDS_CIRC[(c - r) % W] + (MDS_DIAG[r] if r == c else 0)) % P for c in range(W)] for r in range(W)]
    # (A) scalar constants
    e = [0] * W
    a = []
    for i in range(22):
        t = [(rc[12 * (4 + i) + k] + e[k]) % P for k in range(W)]
        a.append(t[0])
        rest = [0] + t[1:]
        e = matvec(M, rest)
    L = e
    # (B) sparse factors, backwards
    Q = M
    what, v = [None] * 22, [None] * 22
    for i in reversed(range(22)):
        Qh = [row[1:] for row in Q[1:]]
        Qhi = inverse(Qh)
        w = [Q[0][1:]]
        what[i] = matmul(w, Qhi)[0]
        v[i] = [Q[r][0] for r in range(1, W)]
        assert Q[0][0] == 25
        D = [[1] + [0] * 11] + [[0] + Qh[r] for r in range(11)]
        Q = matmul(D, M)
    D0 = [row[1:] for row in D[1:]]
    # E = D0 . M[1.., :]: the dense layer merged into the linear layer of the fourth full round (rows 1..11 of its output)
    E = matmul(D0, [M[r] for r in range(1, W)])
    return rc, a, what, v, D0, L, E


def first_round_addends(rc, known):
    """Addends of the first full round's MDS rows when the state words in `known` enter the permutation as 0: such a word
    leaves the S-box as the constant rc[k]^7, and its MDS terms join the row's own constant (the second round's rc[12 + r]):
        addend[r] = rc[12 + r] + sum_{k in known} M[r][k] * rc[k]^7      (canonical)."""
    M = [[(MDS_CIRC[(c - r) % W] + (MDS_DIAG[r] if r == c else 0)) % P for c in range(W)] for r in range(W)]
    z = {k: pow(rc[k], 7, P) for k in known}
    return [(rc[12 + r] + sum(M[r][k] * z[k] for k in known)) % P for r in range(W)]


def permute_fast(state, rc, a, what, v, D0, L, E=None):
    s = list(state)

    def full(s, r, extra=None):
        s = [(s[i] + rc[12 * r + i] + (extra[i] if extra else 0)) % P for i in range(W)]
        s = [pow(x, 7, P) for x in s]
        return [(sum(s[(i + k) % W] * MDS_CIRC[i] for i in range(W)) + s[k] * MDS_DIAG[k]) % P for k in range(W)]

    for r in range(3):
        s = full(s, r)
    if E is None:
        s = full(s, 3)
        s = [s[0]] + matvec(D0, s[1:])
    else:   # fourth full round with the dense layer merged in: row 0 by the MDS, rows 1.. by E
        z = [pow((s[i] + rc[12 * 3 + i]) % P, 7, P) for i in range(W)]
        s0 = (sum(z[i % W] * MDS_CIRC[i] for i in range(W)) + z[0] * MDS_DIAG[0]) % P
        s = [s0] + matvec(E, z)
    for i in range(22):
        s0 = pow((s[0] + a[i]) % P, 7, P)
        n0 = (25 * s0 + sum(x * y for x, y in zip(what[i], s[1:]))) % P
        s = [n0] + [(s[j + 1] + v[i][j] * s0) % P for j in range(11)]
    s = full(s, 26, extra=L)
    for r in range(27, 30):
        s = full(s, r)
    return s


# ---- block form
BLOCKS = [3, 3, 3, 3, 3, 3, 3, 1]   # what poseidon_fast.h evaluates: one loop body of three rounds, whose last trip runs one
MASK32 = (1 << 32) - 1


def mds_int():
    return [[MDS_CIRC[(c - r) % W] + (MDS_DIAG[r] if r == c else 0) for c in range(W)] for r in range(W)]


def imatmul(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(W)) for j in range(W)] for i in range(W)]


def depth_matrices(depth):
    """[M, MZM, MZMZM, ..] over the integers."""
    M = mds_int()
    MZ = [[0 if c == 0 else M[r][c] for c in range(W)] for r in range(W)]
    out = [M]
    for _ in range(depth - 1):
        out.append(imatmul(MZ, out[-1]))
    return out


def block_rows(size):
    """size -> the coefficient rows the block evaluates: ('row0', depth d) for d < size and ('end', r) for the twelve rows
    at depth `size`; each row is (coefficients of y_0..y_11, coefficients of t_1..t_(d-1))."""
    A = depth_matrices(size)
    rows = {}
    for d in range(1, size + 1):
        for r in (range(W) if d == size else [0]):
            tcols = [A[d - 1 - i][r][0] for i in range(1, d)]   # t_i enters through M e0 and then d - 1 - i more rounds
            rows[("end", r) if d == size else ("row0", d)] = (A[d - 1][r], tcols)
    return rows


def row_fold(coef, tcols, key=None):
    """The three 64-bit bounds of one row on arbitrary 32-bit halves, and which fold it gets: 'rare' (x2 < 2^26: the carry of
    the fold's first step is rare, its second step sits behind a wave-uniform branch, fold_al_ah) or 'always' (the second
    step runs branch-free on every lane).  -> (worst accumulator, fold)."""
    acc = (sum(coef) + sum(tcols)) * MASK32 + MASK32
    assert all(0 <= c <= MASK32 for c in list(coef) + list(tcols)), key
    assert acc < 1 << 64, key
    ah2 = acc + (acc >> 32)
    assert ah2 < 1 << 64, key
    x2 = ah2 >> 32
    assert x2 * MASK32 + MASK32 < 1 << 64, key
    return acc, ("rare" if x2 < 1 << 26 else "always")


def block_bounds(size):
    """Worst case of a row's half-accumulators on arbitrary 32-bit halves, with a 32-bit half of K on top, and of the fold
    that follows (poseidon_fast.h, fold_al_ah): ah' = ah + (al >> 32) must fit 64 bits, and with x2 = ah' >> 32 the sum
    base + x2 (2^32 - 1) may wrap once; the wrapped sum is below x2 (2^32 - 1), so adding 2^32 - 1 again must not wrap."""
    worst = 0
    for key, (coef, tcols) in block_rows(size).items():
        acc = (sum(coef) + sum(tcols)) * MASK32 + MASK32
        assert acc < 1 << 64, (size, key)
        ah2 = acc + (acc >> 32)
        assert ah2 < 1 << 64, (size, key)
        x2 = ah2 >> 32
        assert x2 * MASK32 + MASK32 < 1 << 64, (size, key)
        worst = max(worst, acc)
    return worst


def block_constants(rc, sizes, first=4):
    """Per block: [K of row 0 at depth 1, .., size - 1] and the twelve K of the block's end, canonical.  first = 4: the 22
    layers of the partial rounds; first = 3: the 23 layers that begin with round 3's own MDS."""
    assert sum(sizes) == 26 - first
    M = mds_int()
    out, r = [], first
    for size in sizes:
        K, row0 = [0] * W, []
        for i in range(1, size + 1):
            K = [(sum(M[a][c] * K[c] for c in range(1, W)) + rc[12 * (r + i) + a]) % P for a in range(W)]
            if i < size:
                row0.append(K[0])
        out.append((row0, K))
        r += size
    assert r == 26
    return out


def fold_halves(al, ah):
    """The fold as the kernels run it: 64-bit registers, one conditional second step."""
    assert al < 1 << 64 and ah < 1 << 64
    ah2 = ah + (al >> 32)
    assert ah2 < 1 << 64
    x2, base = ah2 >> 32, ((ah2 & MASK32) << 32) | (al & MASK32)
    t = base + x2 * MASK32
    if t >> 64:
        t = (t & ((1 << 64) - 1)) + MASK32
        assert t < 1 << 64
    return t


def partial_rounds_blocks(x, rc, sizes, first=4):
    """The 22 partial rounds in block form on halves, as poseidon_fast.h evaluates them.  x: twelve arbitrary u64 carrying
    round 4's constants; out: twelve u64 carrying round 26's.  first = 3: the merged middle -- x is round 3's S-box layer
    (arbitrary u64), and the first block has no S-box of its own in front."""
    def sbox(v):
        return pow(v % P, 7, P)

    def row(coef, tcols, y, t, k):
        al, ah = k & MASK32, k >> 32
        for c, v in list(zip(coef, y)) + list(zip(tcols, t)):
            al += c * (v & MASK32)
            ah += c * (v >> 32)
        return fold_halves(al, ah)

    x = list(x)
    for b, (size, (k_row0, k_end)) in enumerate(zip(sizes, block_constants(rc, sizes, first))):
        rows = block_rows(size)
        y, t = [x[0] if first == 3 and b == 0 else sbox(x[0])] + x[1:], []
        for d in range(1, size):
            t.append(sbox(row(*rows[("row0", d)], y, t, k_row0[d - 1])))
        x = [row(*rows[("end", r)], y, t, k_end[r]) for r in range(W)]
    return x


def partial_rounds_naive(x, rc):
    M = mds_int()
    x = [v % P for v in x]
    for r in range(4, 26):
        y = [pow(x[0], 7, P)] + x[1:]
        x = [(sum(M[a][c] * y[c] for c in range(W)) + rc[12 * (r + 1) + a]) % P for a in range(W)]
    return x


def check_blocks(rc, rnd):
    for size in (1, 2, 3):
        assert block_bounds(size) < 1 << 57
    for sizes in (BLOCKS, [3] * 6 + [2, 2], [2] * 11, [1] * 22):
        assert all(n <= 3 for n in sizes)   # a larger block needs block_bounds(n) first
        for t in range(12):
            st = [[0] * 12, [P - 1] * 12, [(1 << 64) - 1] * 12][t] if t < 3 else \
                [rnd.randrange(1 << 64) if (t + k) % 3 else rnd.randrange(P) for k in range(12)]
            got = partial_rounds_blocks(st, rc, sizes)
            assert [v % P for v in got] == partial_rounds_naive(st, rc), (sizes, t)
    # and inside the whole permutation
    for t in range(4):
        st = [rnd.randrange(P) for _ in range(12)]
        s = st
        for r in range(4):
            s = [pow((s[i] + rc[12 * r + i]) % P, 7, P) for i in range(W)]
            s = [(sum(s[(i + k) % W] * MDS_CIRC[i] for i in range(W)) + s[k] * MDS_DIAG[k]) % P for k in range(W)]
        s = [(s[i] + rc[48 + i]) % P for i in range(W)]
        s = [v % P for v in partial_rounds_blocks(s, rc, BLOCKS)]
        for r in range(26, 30):
            s = [pow(v, 7, P) for v in s]
            s = [(sum(s[(i + k) % W] * MDS_CIRC[i] for i in range(W)) + s[k] * MDS_DIAG[k] + (rc[12 * (r + 1) + k] if r < 29 else 0)) % P
                 for k in range(W)]
        assert s == permute(st, rc)


def block_tables(rc):
    """The tables poseidon_fast.h reads for BLOCKS (sizes 3 and 1 only: one loop body).
      PB_ROW0_D2[12]     row 0 of MZM: the y-coefficients of the third S-box's input (its t_1 coefficient, M[0][0], and the
                         whole of depth 1's row 0 are MDS entries, which the kernels hold as inline constants)
      PB_END[2][12][13]  per block size (3, then 1) and output row: the t_1 coefficient, then the twelve y-coefficients; the
                         t_2 coefficient of a block of three is M[r][0], an inline constant again.  A block of one has t = 0.
      PB_K[8][14]        per block: K of row 0 at depths 1 and 2 (0 for the block of one), then the twelve K of its end."""
    assert BLOCKS == [3] * 7 + [1]
    r3, r1 = block_rows(3), block_rows(1)
    M = mds_int()
    assert r3[("row0", 1)] == (M[0], []) and r3[("row0", 2)][1] == [M[0][0]]
    assert all(r3[("end", r)][1][1] == M[r][0] for r in range(W))
    end = [[r3[("end", r)][1][0]] + r3[("end", r)][0] for r in range(W)] + [[0] + r1[("end", r)][0] for r in range(W)]
    assert all(0 <= c <= MASK32 for row in end for c in row)
    K = [(k0 + [0, 0])[:2] + kend for k0, kend in block_constants(rc, BLOCKS)]
    return r3[("row0", 2)][0], end, K


# ---- merged middle
MERGED = [4, 4, 4, 4, 4, 3]        # what poseidon_fast.h evaluates: one loop body of depth four, whose last trip skips a stage
MERGED_FALLBACK = [3] * 7 + [2]    # the same 23 layers within the bounds of the blocks of three


def merged_naive(z, rc):
    """z: round 3's twelve S-box outputs.  M z + round 4's constants, then rounds 4..25; out: carries round 26's constants."""
    M = mds_int()
    z = [v % P for v in z]
    return partial_rounds_naive([(sum(M[a][c] * z[c] for c in range(W)) + rc[48 + a]) % P for a in range(W)], rc)


def check_merged(rc, rnd):
    assert sum(MERGED) == 23 and max(MERGED) <= 4
    folds = {}
    for size in sorted(set(MERGED)):
        for key, (coef, tcols) in block_rows(size).items():
            folds[(size,) + key] = row_fold(coef, tcols, (size, key))
    assert all(f == "always" for (size, kind, _), (_, f) in folds.items() if size == 4 and kind == "end")
    assert all(f == "rare" for (size, kind, _), (_, f) in folds.items() if size < 4 or kind == "row0")
    try:   # depth 5 does not fit: some row's accumulator passes 2^64
        for coef, tcols in block_rows(5).values():
            row_fold(coef, tcols)
        raise SystemExit("a block of five fits after all?")
    except AssertionError:
        pass
    for sizes in (MERGED, MERGED_FALLBACK, [4] * 5 + [2, 1], [1] * 23):
        for t in range(12):
            st = [[0] * 12, [P - 1] * 12, [(1 << 64) - 1] * 12][t] if t < 3 else \
                [rnd.randrange(1 << 64) if (t + k) % 3 else rnd.randrange(P) for k in range(12)]
            got = partial_rounds_blocks(st, rc, sizes, first=3)
            assert [v % P for v in got] == merged_naive(st, rc), (sizes, t)
    for t in range(4):   # and inside the whole permutation
        st = [rnd.randrange(P) for _ in range(12)]
        s = st
        for r in range(4):
            s = [pow((s[i] + rc[12 * r + i]) % P, 7, P) for i in range(W)]
            if r < 3:
                s = [(sum(s[(i + k) % W] * MDS_CIRC[i] for i in range(W)) + s[k] * MDS_DIAG[k]) % P for k in range(W)]
        s = [v % P for v in partial_rounds_blocks(s, rc, MERGED, first=3)]
        for r in range(26, 30):
            s = [pow(v, 7, P) for v in s]
            s = [(sum(s[(i + k) % W] * MDS_CIRC[i] for i in range(W)) + s[k] * MDS_DIAG[k] + (rc[12 * (r + 1) + k] if r < 29 else 0)) % P
                 for k in range(W)]
        assert s == permute(st, rc)
    return max(acc for acc, _ in folds.values())


def merged_tables(rc):
    """The tables poseidon_fast.h reads for MERGED (one loop body of depth four; the trip of depth three skips its third stage).
      PM_DEPTH[6]        the partition
      PM_ROW0_D3[13]     row 0 at depth 3: the t_1 coefficient, then the twelve y-coefficients (t_2's is M[0][0], inline; depths
                         1 and 2 are mds_row0 and PB_ROW0_D2, as in the blocks of three)
      PM_END[2][12][14]  per depth (4, then 3) and output row: the coefficients of t_1 and t_2, then the twelve of y.  At depth 4
                         t_3 keeps M[r][0], an inline constant; at depth 3 the loop body runs with t_3 = 0 and the slot of t_2,
                         the last real t, holds M[r][0].
      PM_K[6][15]        per block: K of row 0 at depths 1, 2, 3 (0 where the block is shallower), then the twelve K of its end.
      PM_ALWAYS_*        bit per row: the fold's second step runs always (row_fold); ROW0: bit d - 1 for depth d."""
    assert MERGED == [4] * 5 + [3]
    r4, r3 = block_rows(4), block_rows(3)
    M = mds_int()
    assert r4[("row0", 1)] == (M[0], []) and r4[("row0", 2)] == (r3[("row0", 2)][0], [M[0][0]]) and r4[("row0", 3)][1][1] == M[0][0]
    assert all(r4[("end", r)][1][2] == M[r][0] and r3[("end", r)][1][1] == M[r][0] for r in range(W))
    row0_d3 = [r4[("row0", 3)][1][0]] + r4[("row0", 3)][0]
    end = [r4[("end", r)][1][:2] + r4[("end", r)][0] for r in range(W)] + [r3[("end", r)][1] + r3[("end", r)][0] for r in range(W)]
    K = [(k0 + [0, 0, 0])[:3] + kend for k0, kend in block_constants(rc, MERGED, first=3)]
    assert K[0][0] == rc[48]   # the first block's K_1 is round 4's constants
    always = {
        "ROW0": sum((row_fold(*r4[("row0", d)])[1] == "always") << (d - 1) for d in (1, 2, 3)),
        "END4": sum((row_fold(*r4[("end", r)])[1] == "always") << r for r in range(W)),
        "END3": sum((row_fold(*r3[("end", r)])[1] == "always") << r for r in range(W)),
    }
    return row0_d3, end, K, always


if __name__ == "__main__":
    rc, a, what, v, D0, L, E = derive()
    rnd = random.Random(1)
    for t in range(20):
        st = [0] * 12 if t == 0 else [rnd.randrange(P) for _ in range(12)]
        assert permute(st, rc) == permute_fast(st, rc, a, what, v, D0, L)
        assert permute(st, rc) == permute_fast(st, rc, a, what, v, D0, L, E)
    print("sparse partial rounds == naive permutation on 20 states")
    zcap, zrate = first_round_addends(rc, range(8, 12)), first_round_addends(rc, range(0, 8))
    for t in range(20):   # the two addend tables against a plain first round on states with the known words at 0
        for known, tab in ((range(8, 12), zcap), (range(0, 8), zrate)):
            st = [0 if k in known else rnd.randrange(P) for k in range(12)]
            z = [pow((st[k] + rc[k]) % P, 7, P) for k in range(12)]
            plain = [(sum(z[(i + r) % W] * MDS_CIRC[i] for i in range(W)) + z[r] * MDS_DIAG[r] + rc[12 + r]) % P for r in range(W)]
            live = [(tab[r] + sum((MDS_CIRC[(k - r) % W] + (MDS_DIAG[r] if k == r else 0)) * z[k] for k in range(W) if k not in known)) % P
                    for r in range(W)]
            assert plain == live
    print("first-round addends for known-zero capacity / rate == plain first round on 20 states each")
    check_blocks(rc, rnd)
    print("block form of the partial rounds == naive rounds, accumulator and fold bounds hold for blocks of 1, 2, 3 rounds")
    row0_d2, end, K = block_tables(rc)
    worst = check_merged(rc, rnd)
    print("merged middle (23 layers as %s) == round 3's MDS + naive rounds; accumulators below 2^%.2f, fold bounds hold per row"
          % (MERGED, __import__("math").log2(worst)))
    m_row0_d3, m_end, m_K, m_always = merged_tables(rc)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("// Generated by tools/gen_poseidon_fast.py; equivalence with the naive permutation checked at generation time.\n")

            def arr(name, vals, dims):
                f.write("P2F_DECL const unsigned long long %s%s = {\n" % (name, dims))
                for i in range(0, len(vals), 4):
                    f.write("    " + ", ".join("0x%016xULL" % x for x in vals[i:i + 4]) + ",\n")
                f.write("};\n")
            arr("PF_A", a, "[22]")
            arr("PF_WHAT", [x for row in what for x in row], "[22 * 11]")
            arr("PF_V", [x for row in v for x in row], "[22 * 11]")
            arr("PF_E", [x for row in E for x in row], "[11 * 12]")
            arr("PF_RC26", [(rc[12 * 26 + k] + L[k]) % P for k in range(12)], "[12]")
            arr("RC1_ZCAP", zcap, "[12]")
            arr("RC1_ZRATE", zrate, "[12]")

            def arr32(name, vals, dims, per_line):
                f.write("P2F_DECL const unsigned int %s%s = {\n" % (name, dims))
                for i in range(0, len(vals), per_line):
                    f.write("    " + ", ".join("%uu" % x for x in vals[i:i + per_line]) + ",\n")
                f.write("};\n")
            arr32("PB_ROW0_D2", row0_d2, "[12]", 12)
            arr32("PB_END", [x for row in end for x in row], "[2 * 12 * 13]", 13)
            arr("PB_K", [x for row in K for x in row], "[8 * 14]")
            arr32("PM_DEPTH", MERGED, "[6]", 6)
            arr32("PM_ROW0_D3", m_row0_d3, "[13]", 13)
            arr32("PM_END", [x for row in m_end for x in row], "[2 * 12 * 14]", 14)
            arr("PM_K", [x for row in m_K for x in row], "[6 * 15]")
            for name in ("ROW0", "END4", "END3"):
                f.write("static constexpr unsigned int PM_ALWAYS_%s = 0x%03xu;\n" % (name, m_always[name]))
        print("wrote", sys.argv[1])
