"""Python models of Poseidon's 22 partial rounds for the tests of their block form (poseidon_fast.h: partial_block):

  * naive()        the rounds as defined: S-box on word 0, MDS, next constants -- on field elements;
  * derive()       the block tables recomputed from poseidon_rc.inc and the MDS definition by pushing unit vectors and the round
                   constants through the naive linear steps (no matrix products: not the generator's code);
  * halves()       the block form on 32-bit halves with 64-bit accumulators and the one-or-two-step fold, from the tables
                   poseidon_fast.inc holds, recording for every fold which code site ran it and whether its carry branch was taken;
  * carrying_*()   searches for inputs that take the carry branch of a given fold site.

A fold SITE is a copy of the fold in the kernels' loop body: row 0 at depth 1, row 0 at depth 2 and the twelve rows of a block's
end (the block of one round runs the same end stage)."""
import os
import random
import re

P = 0xFFFFFFFF00000001
M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
CIRC = [17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20]
BLOCKS = [3] * 7 + [1]
SITES = [("row0", 1), ("row0", 2)] + [("end", r) for r in range(12)]
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "plonky2-aes_amd", "csrc")


def mds_entry(r, c):
    return CIRC[(c - r) % 12] + (8 if r == c == 0 else 0)


def mds_apply(v, mod=None):
    out = [sum(mds_entry(r, c) * v[c] for c in range(12)) for r in range(12)]
    return [x % mod for x in out] if mod else out


def round_constants():
    rc = [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]+)ULL", open(os.path.join(CSRC, "poseidon_rc.inc")).read())]
    assert len(rc) == 360 and rc[0] == 0xB585F766F2144405
    return rc


def emitted_tables():
    """{name: list of ints} for the block tables of poseidon_fast.inc."""
    text = open(os.path.join(CSRC, "poseidon_fast.inc")).read()
    out = {}
    for name in ("PB_ROW0_D2", "PB_END", "PB_K"):
        body = re.search(r"\b%s\[[^\]]*\]\s*=\s*\{(.*?)\};" % name, text, flags=re.S).group(1)
        out[name] = [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]+)ULL", body)] or [int(x) for x in re.findall(r"\b(\d+)u\b", body)]
    return out


def naive(x, rc):
    """Rounds 4..25 on a state that carries round 4's constants; out: carries round 26's.  Canonical."""
    x = [v % P for v in x]
    for r in range(4, 26):
        x[0] = pow(x[0], 7, P)
        x = [(a + rc[12 * (r + 1) + k]) % P for k, a in enumerate(mds_apply(x, P))]
    return x


def _linear_rounds(v, depth):
    """v through `depth` linear steps of partial rounds with every S-box output taken as 0: M, then (zero word 0, M) ..."""
    v = mds_apply(v)
    for _ in range(depth - 1):
        v = mds_apply([0] + v[1:])
    return v


def derive(rc):
    """The tables as poseidon_fast.inc lays them out, from first principles.  Coefficient of y_j in row r at depth d: word r of
    e_j after d linear steps.  Coefficient of t_i (the S-box output that replaces word 0 after step i): word r of e_0 after the
    remaining d - i steps."""
    unit = [[int(i == j) for i in range(12)] for j in range(12)]
    row0_d2 = [_linear_rounds(unit[j], 2)[0] for j in range(12)]
    end = []
    for size in (3, 1):
        cols = [_linear_rounds(unit[j], size) for j in range(12)]
        t1 = _linear_rounds(unit[0], size - 1) if size == 3 else [0] * 12
        end += [[t1[r]] + [cols[j][r] for j in range(12)] for r in range(12)]
    K, r = [], 4
    for size in BLOCKS:
        x, row0 = [0] * 12, []
        for i in range(1, size + 1):
            x = [(a + rc[12 * (r + i) + k]) % P for k, a in enumerate(mds_apply([0] + x[1:], P))]
            if i < size:
                row0.append(x[0])
        K.append((row0 + [0, 0])[:2] + x)
        r += size
    return {"PB_ROW0_D2": row0_d2, "PB_END": [c for row in end for c in row], "PB_K": [k for row in K for k in row]}


def fold(al, ah):
    """-> (u64 congruent to al + 2^32 ah, carry branch taken)"""
    assert al <= M64 and ah <= M64
    ah2 = ah + (al >> 32)
    assert ah2 <= M64
    x2, base = ah2 >> 32, ((ah2 & M32) << 32) | (al & M32)
    t = base + x2 * M32
    if t > M64:
        t = (t & M64) + M32
        assert t <= M64   # the second step cannot wrap
        return t, True
    return t, False


def _row(k, terms):
    al, ah = k & M32, k >> 32
    for c, v in terms:
        al += c * (v & M32)
        ah += c * (v >> 32)
    return fold(al, ah)


def halves(x, tab, blocks=8):
    """The block form as the kernels evaluate it.  -> (twelve u64, [(block, site, carried)])."""
    x, ev = list(x), []
    d2, end, K = tab["PB_ROW0_D2"], tab["PB_END"], tab["PB_K"]
    for b in range(blocks):
        k, three = K[14 * b:14 * b + 14], BLOCKS[b] == 3
        y = [pow(x[0] % P, 7, P)] + x[1:]
        t1 = t2 = 0
        if three:
            v, c = _row(k[0], [(mds_entry(0, j), y[j]) for j in range(12)])
            ev.append((b, ("row0", 1), c))
            t1 = pow(v % P, 7, P)
            v, c = _row(k[1], [(mds_entry(0, 0), t1)] + [(d2[j], y[j]) for j in range(12)])
            ev.append((b, ("row0", 2), c))
            t2 = pow(v % P, 7, P)
        e = end[0 if three else 156:]
        x = []
        for r in range(12):
            v, c = _row(k[2 + r], [(mds_entry(r, 0), t2), (e[13 * r], t1)] + [(e[13 * r + 1 + j], y[j]) for j in range(12)])
            ev.append((b, ("end", r), c))
            x.append(v)
    return x, ev


def carried_sites(ev):
    return {s for _, s, c in ev if c}


# ---- inputs that reach a fold's carry branch.  On random data a block-end row carries about once in 250 folds, row 0 at depth 2
# once in 2^17 and row 0 at depth 1 once in 2^24, so only the first is found by trying; the other two are solved for in the first
# block, whose inputs words 1..11 the caller sets freely.
def carrying_row0_d1(tab, rnd):
    """Row 0 at depth 1 is linear in the halves of y: solve for one high half (coefficient 13, odd) so that the low word of
    ah' = ah + (al >> 32) lands just under 2^32."""
    while True:
        x = [rnd.randrange(1 << 64) for _ in range(12)]
        y = [pow(x[0] % P, 7, P)] + x[1:]
        j = 6   # M[0][6] = 13
        al = (tab["PB_K"][0] & M32) + sum(mds_entry(0, i) * (y[i] & M32) for i in range(12))
        rest = (tab["PB_K"][0] >> 32) + sum(mds_entry(0, i) * (y[i] >> 32) for i in range(12) if i != j) + (al >> 32)
        h = ((M32 - 1 - rest) * pow(13, -1, 1 << 32)) & M32   # 13 h + rest = 2^32 - 2 (mod 2^32); x2 is some tens
        x[j] = (h << 32) | (x[j] & M32)
        if ("row0", 1) in carried_sites(halves(x, tab, 1)[1]):
            return x


def carrying_row0_d2(tab, rnd):
    """Row 0 at depth 2 also sees t_1, the S-box of depth 1's row.  Moving the high halves of two words a, b by +c_b k and -c_a k
    (c: depth 1's coefficients) leaves depth 1's row, and with it t_1, unchanged, and moves depth 2's ah' by D k with
    D = C_a c_b - C_b c_a: solve D k = (a value just under 2^32) - ah' (mod 2^32) for a k small enough that neither half wraps."""
    d2 = tab["PB_ROW0_D2"]

    def det(a, b):
        return d2[a] * mds_entry(0, b) - d2[b] * mds_entry(0, a)

    def twos(n):
        return (n & -n).bit_length() - 1

    a, b = min(((a, b) for a in range(1, 12) for b in range(1, 12) if det(a, b)), key=lambda ab: twos(det(*ab)))
    ca, cb, D = mds_entry(0, a), mds_entry(0, b), det(a, b)
    e = twos(D)                                    # D = 2^e D', D' odd: D k = T needs 2^e | T, and fixes k mod 2^(32 - e)
    m = 1 << (32 - e)
    Dinv = pow((D >> e) % m, -1, m)
    while True:
        x = [rnd.randrange(1 << 64) for _ in range(12)]
        x[a] &= (1 << 62) - 1          # room to grow
        x[b] |= 3 << 62                # room to shrink
        kmax = min((M32 - (x[a] >> 32)) // cb, (x[b] >> 32) // ca)
        y = [pow(x[0] % P, 7, P)] + x[1:]
        v, _ = _row(tab["PB_K"][0], [(mds_entry(0, j), y[j]) for j in range(12)])
        t1 = pow(v % P, 7, P)
        terms = [(mds_entry(0, 0), t1)] + [(d2[j], y[j]) for j in range(12)]
        al = (tab["PB_K"][1] & M32) + sum(c * (w & M32) for c, w in terms)
        ah2 = (tab["PB_K"][1] >> 32) + sum(c * (w >> 32) for c, w in terms) + (al >> 32)
        for w in range(2, 4096):   # the window under 2^32 is x2 wide, some ten thousands
            T = (-w - ah2) & M32
            if T & ((1 << e) - 1):
                continue
            k = ((T >> e) * Dinv) % m
            if k <= kmax:
                z = list(x)
                z[a] += (cb * k) << 32
                z[b] -= (ca * k) << 32
                if ("row0", 2) in carried_sites(halves(z, tab, 1)[1]):
                    return z


def random_states(rnd, n):
    return [[rnd.randrange(1 << 64) if (i + k) % 4 else rnd.randrange(P) for k in range(12)] for i in range(n)]
