// The AES-GCM host twins (csrc/aes_gadgets.h: gcm_encrypt_aad, gcm_decrypt, gcm_encrypt) at the edge lengths, as a stand-alone
// program for the sanitizers: every buffer is a heap allocation of exactly its length, so one byte read or written past an end
// is reported.  It checks what can be checked without a second implementation: aad_len = 0 equals gcm_encrypt, decryption
// inverts encryption, a flipped bit in the ciphertext, tag or aad is refused with the plaintext zeroed, and McGrew-Viega's
// test case 4.  tests/test_gcm_sanitize_host.py builds and runs it.
#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

#include "aes_gadgets.h"

using namespace p2;

static int failures = 0;
#define CHECK(c)                                              \
    do {                                                      \
        if (!(c)) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c), failures++; \
    } while (0)

// a heap buffer of exactly n bytes (n = 0: a one-byte allocation nobody may touch is not needed: nullptr)
static std::unique_ptr<uint8_t[]> buf(size_t n, unsigned seed) {
    std::unique_ptr<uint8_t[]> p(n ? new uint8_t[n] : nullptr);
    for (size_t i = 0; i < n; i++) p[i] = (uint8_t)(seed = seed * 1103515245u + 12345u) >> 3;
    return p;
}
static std::vector<uint8_t> unhex(const char* s) {
    std::vector<uint8_t> v;
    for (; s[0] && s[1]; s += 2) {
        unsigned b;
        sscanf(s, "%2x", &b);
        v.push_back((uint8_t)b);
    }
    return v;
}

int main() {
    const size_t lens[] = {0, 1, 13, 15, 16, 17, 31, 32, 33}, aad_lens[] = {0, 1, 5, 13, 16, 17, 20};
    size_t cases = 0;
    for (int nk = 4; nk <= 8; nk += 2)
        for (size_t len : lens)
            for (size_t al : aad_lens) {
                const int nr = nk + 6;
                auto key = buf(4 * nk, 1 + nk), nonce = buf(12, 2 + len), pt = buf(len, 3 + al), aad = buf(al, 4 + len);
                auto ct = buf(len, 0), tag = buf(16, 0), back = buf(len, 0);
                aes::gcm_encrypt_aad(nk, nr, key.get(), nonce.get(), aad.get(), al, pt.get(), len, ct.get(), tag.get());
                if (al == 0) {
                    auto ct0 = buf(len, 0), tag0 = buf(16, 0);
                    aes::gcm_encrypt(nk, nr, key.get(), nonce.get(), pt.get(), len, ct0.get(), tag0.get());
                    CHECK(!memcmp(tag0.get(), tag.get(), 16) && (!len || !memcmp(ct0.get(), ct.get(), len)));
                }
                CHECK(aes::gcm_decrypt(nk, nr, key.get(), nonce.get(), aad.get(), al, ct.get(), len, tag.get(), back.get()));
                CHECK(!len || !memcmp(back.get(), pt.get(), len));
                // one flipped bit in each of ct, tag and aad: refused, and the plaintext buffer zeroed
                for (int which = 0; which < 3; which++) {
                    uint8_t* p = which == 0 ? ct.get() : which == 1 ? tag.get() : aad.get();
                    const size_t n = which == 0 ? len : which == 1 ? 16 : al;
                    if (!n) continue;
                    p[n - 1] ^= 0x80;
                    if (len) memset(back.get(), 0xAA, len);
                    CHECK(!aes::gcm_decrypt(nk, nr, key.get(), nonce.get(), aad.get(), al, ct.get(), len, tag.get(), back.get()));
                    for (size_t i = 0; i < len; i++) CHECK(back[i] == 0);
                    p[n - 1] ^= 0x80;
                }
                cases++;
            }
    {
        auto key = unhex("feffe9928665731c6d6a8f9467308308"), iv = unhex("cafebabefacedbaddecaf888"), aad = unhex("feedfacedeadbeeffeedfacedeadbeefabaddad2");
        auto pt = unhex("d9313225f88406e5a55909c5aff5269a86a7a9531534f7da2e4c303d8a318a721c3c0c95956809532fcf0e2449a6b525b16aedf5aa0de657ba637b39");
        auto want = unhex("5bc94fbc3221a5db94fae95ae7121a47");
        auto ct = buf(pt.size(), 0), tag = buf(16, 0);
        aes::gcm_encrypt_aad(4, 10, key.data(), iv.data(), aad.data(), aad.size(), pt.data(), pt.size(), ct.get(), tag.get());
        CHECK(pt.size() == 60 && !memcmp(tag.get(), want.data(), 16) && ct[0] == 0x42 && ct[1] == 0x83);
    }
    if (failures) return printf("gcm check: %d failures\n", failures), 1;
    printf("gcm ok: %zu shapes\n", cases);
    return 0;
}
