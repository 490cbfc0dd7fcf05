"""Python models of the merged middle of Poseidon (poseidon_fast.h: merged_middle) for its tests: round 3's MDS and the 22 partial
rounds as one chain of 23 linear layers, in blocks of up to four.  Built on partial_rounds_ref.py, which stays as it is:

  * naive()        M z + round 4's constants, then rounds 4..25 as partial_rounds_ref.naive does them -- on field elements;
  * derive()       the PM_* tables recomputed from poseidon_rc.inc and the MDS definition by pushing unit vectors and the round
                   constants through the naive linear steps (not the generator's code);
  * halves()       the merged form on 32-bit halves with 64-bit accumulators and the two-step fold, from the tables
                   poseidon_fast.inc holds, recording for every fold which code site ran it and whether its first step carried;
  * carrying_*()   inputs that carry at row 0 of depth 1 / depth 2 in the first block, solved for.

A fold SITE is a copy of the fold in the loop body, per table it runs on: row 0 at depths 1, 2, 3 and the twelve end rows on the
depth-4 table ("end4") and on the depth-3 table ("end3").  A site is RARE when its second step sits behind the wave-uniform branch
(PM_ALWAYS_* clear for every table the copy serves); the end rows are one copy for both tables, so they all run the always form."""
import os
import re

import partial_rounds_ref as R

P, M32, M64 = R.P, R.M32, R.M64
SITES = [("row0", d) for d in (1, 2, 3)] + [("end4", r) for r in range(12)] + [("end3", r) for r in range(12)]
NAMES = ("PB_ROW0_D2", "PM_DEPTH", "PM_ROW0_D3", "PM_END", "PM_K")


def emitted_tables():
    """{name: list of ints} for the tables merged_middle reads, and the PM_ALWAYS_* masks."""
    text = open(os.path.join(R.CSRC, "poseidon_fast.inc")).read()
    out = {}
    for name in NAMES:
        body = re.search(r"\b%s\[[^\]]*\]\s*=\s*\{(.*?)\};" % name, text, flags=re.S).group(1)
        out[name] = [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]+)ULL", body)] or [int(x) for x in re.findall(r"\b(\d+)u\b", body)]
    for name in ("ROW0", "END4", "END3"):
        out["PM_ALWAYS_" + name] = int(re.search(r"\bPM_ALWAYS_%s\s*=\s*0x([0-9a-fA-F]+)u;" % name, text).group(1), 16)
    return out


def naive(z, rc):
    """z: round 3's twelve S-box outputs (any u64).  Out: the state that carries round 26's constants, canonical."""
    x = [(a + rc[48 + k]) % P for k, a in enumerate(R.mds_apply([v % P for v in z], P))]
    return R.naive(x, rc)


def derive(rc, depths):
    """The tables as poseidon_fast.inc lays them out, from first principles, for a partition `depths` of the 23 layers whose blocks
    are four deep except a last one of three.  Coefficient of y_j in row r at depth d: word r of e_j after d linear steps; of t_i:
    word r of e_0 after the remaining d - i steps."""
    unit = [[int(i == j) for i in range(12)] for j in range(12)]
    e0 = unit[0]
    row0_d3 = [R._linear_rounds(e0, 2)[0]] + [R._linear_rounds(unit[j], 3)[0] for j in range(12)]
    end = []
    for size in (4, 3):
        cols = [R._linear_rounds(unit[j], size) for j in range(12)]
        t1, t2 = R._linear_rounds(e0, size - 1), R._linear_rounds(e0, size - 2)
        end += [[t1[r], t2[r]] + [cols[j][r] for j in range(12)] for r in range(12)]
    K, r = [], 3
    for size in depths:
        x, row0 = [0] * 12, []
        for i in range(1, size + 1):
            x = [(a + rc[12 * (r + i) + k]) % P for k, a in enumerate(R.mds_apply([0] + x[1:], P))]
            if i < size:
                row0.append(x[0])
        K.append((row0 + [0, 0, 0])[:3] + x)
        r += size
    assert r == 26
    return {"PM_ROW0_D3": row0_d3, "PM_END": [c for row in end for c in row], "PM_K": [k for row in K for k in row],
            "PB_ROW0_D2": [R._linear_rounds(unit[j], 2)[0] for j in range(12)]}


def emitted_rows(tab):
    """[(site, coefficients of every term of the row)] for each row the loop body evaluates, per table."""
    m00 = R.mds_entry(0, 0)
    rows = [(("row0", 1), [R.mds_entry(0, j) for j in range(12)]), (("row0", 2), tab["PB_ROW0_D2"] + [m00]), (("row0", 3), tab["PM_ROW0_D3"] + [m00])]
    for r in range(12):
        rows.append((("end4", r), tab["PM_END"][14 * r:14 * r + 14] + [R.mds_entry(r, 0)]))
    for r in range(12):
        rows.append((("end3", r), tab["PM_END"][14 * (12 + r):14 * (12 + r) + 14]))   # t_3 = 0: no inline term
    return rows


def always_flag(tab, site):
    """What the generator emitted for the row of `site`."""
    kind, i = site
    return bool((tab["PM_ALWAYS_ROW0"] >> (i - 1)) & 1) if kind == "row0" else bool((tab["PM_ALWAYS_" + kind.upper()] >> i) & 1)


def rare_sites(tab):
    """The sites whose second step is behind the branch: row 0 where its flag is clear; an end row (one copy for both tables) only
    if neither table asks for the always form."""
    out = [s for s in SITES[:3] if not always_flag(tab, s)]
    for kind in ("end4", "end3"):
        out += [(kind, r) for r in range(12) if not always_flag(tab, ("end4", r)) and not always_flag(tab, ("end3", r))]
    return out


def halves(z, tab, blocks=6):
    """The merged form as the kernels evaluate it.  -> (twelve u64, [(block, site, carried)])."""
    x, ev = list(z), []
    d2, d3, end, K = tab["PB_ROW0_D2"], tab["PM_ROW0_D3"], tab["PM_END"], tab["PM_K"]
    m0 = [R.mds_entry(0, j) for j in range(12)]
    for b in range(blocks):
        k, four = K[15 * b:15 * b + 15], tab["PM_DEPTH"][b] == 4
        y = ([pow(x[0] % P, 7, P)] if b else [x[0]]) + x[1:]
        yl, yh = [v & M32 for v in y], [v >> 32 for v in y]

        def row(kk, coef, extra):
            al = (kk & M32) + sum(map(int.__mul__, coef, yl))
            ah = (kk >> 32) + sum(map(int.__mul__, coef, yh))
            for c, v in extra:
                al += c * (v & M32)
                ah += c * (v >> 32)
            return R.fold(al, ah)

        v, c = row(k[0], m0, [])
        ev.append((b, ("row0", 1), c))
        t1 = pow(v % P, 7, P)
        v, c = row(k[1], d2, [(m0[0], t1)])
        ev.append((b, ("row0", 2), c))
        t2 = pow(v % P, 7, P)
        t3 = 0
        if four:
            v, c = row(k[2], d3[1:], [(d3[0], t1), (m0[0], t2)])
            ev.append((b, ("row0", 3), c))
            t3 = pow(v % P, 7, P)
        e = end[0 if four else 12 * 14:]
        x = []
        for r in range(12):
            v, c = row(k[3 + r], e[14 * r + 2:14 * r + 14], [(e[14 * r], t1), (e[14 * r + 1], t2), (R.mds_entry(r, 0), t3)])
            ev.append((b, ("end4" if four else "end3", r), c))
            x.append(v)
    return x, ev


def carried_sites(ev):
    return {s for _, s, c in ev if c}


# ---- inputs that carry at a rare fold.  On random data row 0 carries once in 2^24 folds at depth 1 and once in 2^17 at depth 2, so
# those two are solved for in the first block, all of whose inputs are the caller's; row 0 at depth 3 and an end row on the depth-3
# table (x2 < 2^24) carry once in some hundreds of folds and are found by trying.
def carrying_row0_d1(tab, rnd):
    """Row 0 at depth 1 is linear in the halves of y = z: solve for one high half (coefficient 13, odd) so that the low word of
    ah' = ah + (al >> 32) lands just under 2^32 (partial_rounds_ref.carrying_row0_d1, on this form's K and with y_0 = z_0)."""
    while True:
        x = [rnd.randrange(1 << 64) for _ in range(12)]
        j = 6   # M[0][6] = 13
        al = (tab["PM_K"][0] & M32) + sum(R.mds_entry(0, i) * (x[i] & M32) for i in range(12))
        rest = (tab["PM_K"][0] >> 32) + sum(R.mds_entry(0, i) * (x[i] >> 32) for i in range(12) if i != j) + (al >> 32)
        h = ((M32 - 1 - rest) * pow(13, -1, 1 << 32)) & M32
        x[j] = (h << 32) | (x[j] & M32)
        if ("row0", 1) in carried_sites(halves(x, tab, 1)[1]):
            return x


def carrying_row0_d2(tab, rnd):
    """Moving the high halves of two words a, b by +c_b k and -c_a k (c: depth 1's coefficients) leaves depth 1's row, and t_1,
    unchanged and moves depth 2's ah' by D k, D = C_a c_b - C_b c_a (partial_rounds_ref.carrying_row0_d2, on this form)."""
    d2 = tab["PB_ROW0_D2"]

    def det(a, b):
        return d2[a] * R.mds_entry(0, b) - d2[b] * R.mds_entry(0, a)

    def twos(n):
        return (n & -n).bit_length() - 1

    a, b = min(((a, b) for a in range(1, 12) for b in range(1, 12) if det(a, b)), key=lambda ab: twos(det(*ab)))
    ca, cb, D = R.mds_entry(0, a), R.mds_entry(0, b), det(a, b)
    e = twos(D)
    m = 1 << (32 - e)
    Dinv = pow((D >> e) % m, -1, m)
    while True:
        x = [rnd.randrange(1 << 64) for _ in range(12)]
        x[a] &= (1 << 62) - 1          # room to grow
        x[b] |= 3 << 62                # room to shrink
        kmax = min((M32 - (x[a] >> 32)) // cb, (x[b] >> 32) // ca)
        v, _ = R._row(tab["PM_K"][0], [(R.mds_entry(0, j), x[j]) for j in range(12)])
        t1 = pow(v % P, 7, P)
        terms = [(R.mds_entry(0, 0), t1)] + [(d2[j], x[j]) for j in range(12)]
        al = (tab["PM_K"][1] & M32) + sum(c * (w & M32) for c, w in terms)
        ah2 = (tab["PM_K"][1] >> 32) + sum(c * (w >> 32) for c, w in terms) + (al >> 32)
        for w in range(2, 4096):
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
