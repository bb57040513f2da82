// The host logic of the engine's logit rules (csrc/rules_host.h) as a stand-alone program:
// tests/test_rules_host_asan.py compiles it with -fsanitize=address,undefined and runs it, so
// every read of a caller's array and every write of a result is checked. The arrays are heap
// allocations of exactly the stated size, which puts a read past their end into a redzone.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "rules_host.h"

namespace rh = llmi::rules_host;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

template <typename T>
static std::unique_ptr<T[]> exact(std::initializer_list<T> v) {
    std::unique_ptr<T[]> p(new T[v.size()]);
    size_t i = 0;
    for (T x : v) p[i++] = x;
    return p;
}

static void bitmap_cases() {
    for (int vocab : {1, 31, 32, 33, 100, 4096, 32000, 32001}) {
        std::vector<uint32_t> w(3, 0xDEADBEEFu);
        // empty list: the all-clear bitmap of the right size
        CHECK(rh::ids_to_bitmap(nullptr, 0, vocab, &w) == rh::kOk);
        CHECK(w.size() == rh::bitmap_words(vocab));
        for (uint32_t x : w) CHECK(x == 0u);
        // id 0 and id vocab - 1 (a vocab that is no multiple of 32 ends inside a word)
        auto ids = exact<int32_t>({0, vocab - 1});
        CHECK(rh::ids_to_bitmap(ids.get(), 2, vocab, &w) == rh::kOk);
        CHECK(w.size() == (size_t)(vocab + 31) / 32);
        for (int i = 0; i < (int)w.size() * 32; ++i) {
            const bool bit = (w[i >> 5] >> (i & 31)) & 1u;
            CHECK(bit == (i == 0 || i == vocab - 1));  // nothing past vocab is set
        }
        // ids at and above vocab, and below 0, are refused and leave the result alone
        std::vector<uint32_t> before = w;
        auto at = exact<int32_t>({0, vocab});
        CHECK(rh::ids_to_bitmap(at.get(), 2, vocab, &w) == rh::kIdRange);
        auto above = exact<int32_t>({vocab + 31});
        CHECK(rh::ids_to_bitmap(above.get(), 1, vocab, &w) == rh::kIdRange);
        auto huge = exact<int32_t>({std::numeric_limits<int32_t>::max()});
        CHECK(rh::ids_to_bitmap(huge.get(), 1, vocab, &w) == rh::kIdRange);
        auto neg = exact<int32_t>({-1});
        CHECK(rh::ids_to_bitmap(neg.get(), 1, vocab, &w) == rh::kIdRange);
        CHECK(w == before);
        // a repeated id is harmless in a set
        auto dup = exact<int32_t>({vocab - 1, vocab - 1});
        CHECK(rh::ids_to_bitmap(dup.get(), 2, vocab, &w) == rh::kOk);
        CHECK(((w[(vocab - 1) >> 5] >> ((vocab - 1) & 31)) & 1u) == 1u);
    }
    std::vector<uint32_t> w;
    auto one = exact<int32_t>({0});
    CHECK(rh::ids_to_bitmap(one.get(), 1, 0, &w) == rh::kBadVocab);
    CHECK(rh::ids_to_bitmap(one.get(), -1, 8, &w) == rh::kBadCount);
    CHECK(rh::ids_to_bitmap(nullptr, 1, 8, &w) == rh::kNullArray);
    CHECK(w.empty());
}

static void bias_cases() {
    const float inf = std::numeric_limits<float>::infinity();
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (int vocab : {1, 33, 100, 32000}) {
        std::vector<float> d(5, 1.f);
        // empty list: the all-zero row
        CHECK(rh::bias_to_dense(nullptr, nullptr, 0, vocab, &d) == rh::kOk);
        CHECK(d.size() == (size_t)vocab);
        for (float x : d) CHECK(x == 0.f && !std::signbit(x));
        if (vocab < 2) continue;
        // id 0, id vocab - 1, a ban
        auto ids = exact<int32_t>({0, vocab - 1, 1});
        auto vals = exact<float>({2.5f, -3.f, -inf});
        CHECK(rh::bias_to_dense(ids.get(), vals.get(), 3, vocab, &d) == rh::kOk);
        CHECK(d.size() == (size_t)vocab && d[0] == 2.5f && d[vocab - 1] == -3.f && d[1] == -inf);
        for (int i = 2; i < vocab - 1; ++i) CHECK(d[i] == 0.f);
        const std::vector<float> before = d;
        // refused: ids at / above vocab, duplicates, NaN, +inf; the result is left alone
        auto at = exact<int32_t>({vocab});
        auto v1 = exact<float>({1.f});
        CHECK(rh::bias_to_dense(at.get(), v1.get(), 1, vocab, &d) == rh::kIdRange);
        auto above = exact<int32_t>({0, vocab + 1000});
        auto v2 = exact<float>({1.f, 1.f});
        CHECK(rh::bias_to_dense(above.get(), v2.get(), 2, vocab, &d) == rh::kIdRange);
        auto dup = exact<int32_t>({vocab - 1, 0, vocab - 1});
        auto v3 = exact<float>({1.f, 2.f, 3.f});
        CHECK(rh::bias_to_dense(dup.get(), v3.get(), 3, vocab, &d) == rh::kDuplicateId);
        auto two = exact<int32_t>({0, 1});
        auto vnan = exact<float>({1.f, nan});
        CHECK(rh::bias_to_dense(two.get(), vnan.get(), 2, vocab, &d) == rh::kBadValue);
        auto vinf = exact<float>({inf, 1.f});
        CHECK(rh::bias_to_dense(two.get(), vinf.get(), 2, vocab, &d) == rh::kBadValue);
        CHECK(rh::bias_to_dense(two.get(), nullptr, 2, vocab, &d) == rh::kNullArray);
        CHECK(rh::bias_to_dense(nullptr, v2.get(), 2, vocab, &d) == rh::kNullArray);
        CHECK(rh::bias_to_dense(two.get(), v2.get(), -2, vocab, &d) == rh::kBadCount);
        CHECK(d.size() == before.size() && std::memcmp(d.data(), before.data(), d.size() * 4) == 0);
    }
    CHECK(rh::bias_value_ok(0.f) && rh::bias_value_ok(-inf) && rh::bias_value_ok(-1e38f));
    CHECK(!rh::bias_value_ok(inf) && !rh::bias_value_ok(nan));
    CHECK(rh::penalty_ok(0.f) && rh::penalty_ok(-2.f));
    CHECK(!rh::penalty_ok(inf) && !rh::penalty_ok(-inf) && !rh::penalty_ok(nan));
    for (int s = rh::kOk; s <= rh::kBadValue; ++s) CHECK(std::strlen(rh::message(s)) > 0);
}

int main() {
    bitmap_cases();
    bias_cases();
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("rules_host: all checks passed\n");
    return 0;
}
