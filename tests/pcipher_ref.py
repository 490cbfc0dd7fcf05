"""poseidon-cipher/src/lib.rs in Python, for the cipher tests: hash_state (:113), encrypt (:41) and decrypt (:75) on
sponge_ref.permute over the CPU oracle's Poseidon.  It calls nothing of the library under test.  An Fq element is a tuple of five
words, a key the point (x, u), a nonce two words.  encrypt_padded takes the padded message and the length apart, so that a
ciphertext whose padding elements are not zero can be made."""
import oracle_lib
import sponge_ref

P = sponge_ref.P
ZERO = (0,) * 5


def hash_n_to_m_no_pad(words, m):
    st = [0] * 12
    for c0 in range(0, len(words), 8):
        chunk = [int(w) for w in words[c0:c0 + 8]]
        st[:len(chunk)] = chunk
        st = sponge_ref.permute(oracle_lib, st)
    out = []
    while True:
        for w in st[:8]:
            out.append(w)
            if len(out) == m:
                return out
        st = sponge_ref.permute(oracle_lib, st)


def hash_state(s):
    """s: four Fq elements -> four Fq elements"""
    h = hash_n_to_m_no_pad([w for e in s for w in e], 20)
    return [tuple(h[5 * i:5 * i + 5]) for i in range(4)]


def pad3(l):
    return (l + 2) // 3 * 3


def fq_add(a, b):
    return tuple((x + y) % P for x, y in zip(a, b))


def fq_sub(a, b):
    return tuple((x - y) % P for x, y in zip(a, b))


def encrypt_padded(ks, m_padded, nonce, l):
    """lib.rs:41 after its padding step: m_padded has a multiple of three elements, l is the length the state opens with"""
    assert len(m_padded) % 3 == 0
    s = [ZERO, tuple(ks[0]), tuple(ks[1]), (nonce[0], nonce[1], l, 0, 0)]
    ct = []
    for i in range(len(m_padded) // 3):
        s = hash_state(s)
        for k in range(3):
            s[1 + k] = fq_add(s[1 + k], m_padded[3 * i + k])
            ct.append(s[1 + k])
    return ct + [hash_state(s)[1]]


def encrypt(ks, msg, nonce):
    msg = [tuple(e) for e in msg]
    return encrypt_padded(ks, msg + [ZERO] * (pad3(len(msg)) - len(msg)), nonce, len(msg))


def decrypt(ks, ct, nonce, l):
    """lib.rs:75; None where one of its asserts fails.  The padding elements are looked at only when l > 3."""
    s = [ZERO, tuple(ks[0]), tuple(ks[1]), (nonce[0], nonce[1], l, 0, 0)]
    m = []
    for i in range(len(ct) // 3):
        s = hash_state(s)
        for k in range(3):
            m.append(fq_sub(ct[3 * i + k], s[1 + k]))
            s[1 + k] = tuple(ct[3 * i + k])
    if l > 3:
        if l % 3 == 2 and m[-1] != ZERO:
            return None
        if l % 3 == 1 and (m[-1] != ZERO or m[-2] != ZERO):
            return None
    if tuple(ct[-1]) != hash_state(s)[1]:
        return None
    return m[:l]
