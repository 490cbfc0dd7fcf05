// The MerkleMap host twin (csrc/merkle_host.h: mt::HostMap, mt::host_map_verify) as a stand-alone program for the sanitizers:
// every buffer is a heap allocation of exactly its length, so one word read or written past an end is reported.  Without a
// second implementation it checks what the definition promises: every proof the map gives, for present and absent keys, walks
// to the map's cap (status 0) and stops doing so with the flag flipped (1); a flag of 2 and a word of p are malformed (2); bad
// entries throw and name themselves.  tests/test_merkle_map_sanitize_host.py builds and runs it.
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "merkle_host.h"

using namespace p2;

static int failures = 0;
#define CHECK(c)                                              \
    do {                                                      \
        if (!(c)) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c), failures++; \
    } while (0)

static std::unique_ptr<u64[]> words(size_t n) { return std::unique_ptr<u64[]>(n ? new u64[n]() : nullptr); }

static std::string refused(const std::vector<u64>& keys, const std::vector<u64>& values, size_t V, int D, int h) {
    auto k = words(keys.size()), v = words(values.size());
    if (!keys.empty()) memcpy(k.get(), keys.data(), 8 * keys.size());
    if (!values.empty()) memcpy(v.get(), values.data(), 8 * values.size());
    try {
        mt::HostMap m(k.get(), v.get(), keys.size(), V, D, h);
    } catch (std::exception& e) {
        return e.what();
    }
    return "";
}

int main() {
    const struct {
        int D, h;
    } shapes[] = {{1, 0}, {1, 1}, {3, 0}, {3, 1}, {8, 4}, {13, 0}, {64, 0}, {64, 4}, {64, 16}};
    const size_t value_lens[] = {0, 1, 3, 4, 7, 8, 134}, counts[] = {0, 1, 2, 5};
    size_t cases = 0;
    for (auto s : shapes)
        for (size_t V : value_lens)
            for (size_t n : counts) {
                const u64 space = s.D == 64 ? gl::P : (u64)1 << s.D;
                if (n > space) continue;
                auto keys = words(n), values = words(n * V);
                // keys spread over the space, its last one among them, given in descending order
                for (size_t i = 0; i < n; i++) keys[i] = i == 0 ? space - 1 : (space / (n + 1)) * (n - i);
                for (size_t i = 0; i < n * V; i++) values[i] = (0x9E3779B97F4A7C15ull * (i + 1)) % gl::P;
                mt::HostMap m(keys.get(), values.get(), n, V, s.D, s.h);
                const size_t depth = (size_t)(s.D - s.h), cap_n = (size_t)1 << s.h;
                auto cap = words(4 * cap_n), sib = words(4 * depth), zeros = words(V);
                m.cap(cap.get());
                std::vector<u64> queries = {0, space - 1, space / 2};
                for (size_t i = 0; i < n; i++) queries.push_back(keys[i]), queries.push_back(keys[i] ^ 1);
                for (u64 q : queries) {
                    if (!mt::map_key_ok(q, (u32)s.D)) continue;
                    const ptrdiff_t at = m.find(q);
                    m.siblings(q, sib.get());
                    const u64* value = at >= 0 ? values.get() + m.pos[(size_t)at] * V : zeros.get();
                    CHECK(mt::host_map_verify(q, (u32)s.D, at >= 0, value, V, sib.get(), cap.get(), (u32)s.h) == 0);
                    CHECK(mt::host_map_verify(q, (u32)s.D, at < 0, value, V, sib.get(), cap.get(), (u32)s.h) == 1);
                    CHECK(mt::host_map_verify(q, (u32)s.D, 2, value, V, sib.get(), cap.get(), (u32)s.h) == 2);
                    const size_t entry = 4 * (size_t)mt::map_shr(q, (u32)depth);
                    cap[entry] ^= 1;
                    CHECK(mt::host_map_verify(q, (u32)s.D, at >= 0, value, V, sib.get(), cap.get(), (u32)s.h) == 1);
                    cap[entry] ^= 1;
                    if (depth) {
                        sib[4 * depth - 1] = gl::P;
                        CHECK(mt::host_map_verify(q, (u32)s.D, at >= 0, value, V, sib.get(), cap.get(), (u32)s.h) == 2);
                    }
                }
                cases++;
            }
    CHECK(refused({3, gl::P}, {1, 2}, 1, 64, 0).find("entry 1") != std::string::npos);
    CHECK(refused({3, 5, 256}, {}, 0, 8, 0).find("entry 2") != std::string::npos);
    CHECK(refused({7, 3, 9, 3}, {}, 0, 8, 2).find("entry 3") != std::string::npos);
    CHECK(refused({7, 3}, {1, 2, gl::P, 0}, 2, 8, 0).find("entry 1") != std::string::npos);
    CHECK(!refused({1}, {}, 0, 0, 0).empty() && !refused({1}, {}, 0, 65, 0).empty() && !refused({1}, {}, 0, 3, 4).empty() && !refused({1}, {}, 135, 8, 0).empty());
    CHECK(refused({1, 0}, {}, 0, 1, 1).empty());
    if (failures) return printf("merkle map check: %d failures\n", failures), 1;
    printf("merkle map ok: %zu maps\n", cases);
    return 0;
}
