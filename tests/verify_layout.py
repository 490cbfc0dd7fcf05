"""Byte layout of a serialised proof (the reader of csrc/verifier.h), from p2_blob_info alone: the sections
the batched-verifier tests tamper with."""


def sections(info, num_queries=28):
    """{name: (byte offset, length in bytes, kind)}; kind "words" (u64 words) or "count" (one sibling-count byte)."""
    R, W, NC, qdf, cap = 80, info["num_wires"], 2, 8, 4
    ncc, zc, qc = info["num_constants_cols"], info["num_zs_cols"], info["num_quotient_cols"]
    npp = (R + qdf - 1) // qdf - 1
    nlp = (zc - NC * (1 + npp)) // NC
    salt = 4 if info["zero_knowledge"] else 0
    lde_bits = info["degree_bits"] + 3
    rounds = info["num_fri_rounds"]
    out, pos = {}, 0

    def put(name, nbytes, kind="words"):
        nonlocal pos
        out[name] = (pos, nbytes, kind)
        pos += nbytes

    for c in ("wires_cap", "zs_cap", "quotient_cap"):
        put(c, 8 * 4 * 16)
    for name, k in (("constants", ncc), ("sigmas", R), ("wires", W), ("zs", NC), ("zs_next", NC), ("lookup_zs", NC * nlp),
                    ("lookup_zs_next", NC * nlp), ("partial_products", NC * npp), ("quotient", NC * qdf)):
        put("open_" + name, 16 * k)
    for r in range(rounds):
        put("fri_cap%d" % r, 8 * 4 * 16)
    cols = [ncc + R, W + salt, zc + salt, qc + salt]
    for q in range(num_queries):
        for o in range(4):
            depth = lde_bits - cap
            put("q%d_init%d_leaf" % (q, o), 8 * cols[o])
            put("q%d_init%d_count" % (q, o), 1, "count")
            put("q%d_init%d_siblings" % (q, o), 32 * depth)
        bits = lde_bits
        for r in range(rounds):
            depth = bits - cap - 4
            put("q%d_round%d_evals" % (q, r), 16 * 16)
            put("q%d_round%d_count" % (q, r), 1, "count")
            put("q%d_round%d_siblings" % (q, r), 32 * depth)
            bits -= 4
    put("final_poly", 16 * ((1 << info["degree_bits"]) >> (4 * rounds)))
    put("pow_witness", 8)
    assert pos == info["proof_bytes"], (pos, info["proof_bytes"])
    return out
