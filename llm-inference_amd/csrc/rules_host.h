// Host side of the engine's logit rules (llmi_engine_set_logit_rules / llmi_engine_set_allowed):
// everything that reads a caller's arrays -- the size and value checks, sparse (id, value) bias
// pairs to a dense row, an id list to allowed-bitmap words. Plain C++ with no HIP dependency, so
// tests/cpp/test_rules_host.cpp runs it under the address and undefined-behaviour sanitizers.
// Every function checks all of its input before it writes, and writes only into its own
// result (which replaces *out on success and leaves it alone on a refusal); no caller pointer
// is kept.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace llmi {
namespace rules_host {

enum Status {
    kOk = 0,
    kBadVocab,    // vocab <= 0
    kBadCount,    // n < 0
    kNullArray,   // n > 0 with a null array
    kIdRange,     // an id outside [0, vocab)
    kDuplicateId, // a bias id given twice
    kBadValue,    // a bias value that is NaN or +inf
};

inline const char* message(int status) {
    switch (status) {
        case kOk: return "ok";
        case kBadVocab: return "vocab must be positive";
        case kBadCount: return "the element count must be >= 0";
        case kNullArray: return "a null array with a positive element count";
        case kIdRange: return "token ids must be in [0, vocab)";
        case kDuplicateId: return "a bias id is given twice";
        case kBadValue: return "bias values must be finite or -inf (a ban)";
        default: return "unknown status";
    }
}

inline size_t bitmap_words(int vocab) { return ((size_t)vocab + 31) / 32; }

// a bias value: finite, or -inf (a ban); NaN and +inf are refused
inline bool bias_value_ok(float v) { return std::isfinite(v) || (std::isinf(v) && v < 0.f); }
inline bool penalty_ok(float v) { return std::isfinite(v); }

inline int check_ids(const int32_t* ids, int n, int vocab) {
    if (vocab <= 0) return kBadVocab;
    if (n < 0) return kBadCount;
    if (n > 0 && !ids) return kNullArray;
    for (int i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= vocab) return kIdRange;
    return kOk;
}

// ids [n] -> the allowed bitmap, uint32 [(vocab + 31) / 32]: bit id & 31 of word id >> 5 set for
// every id of the list, every other bit (the last word's bits past vocab too) clear. A repeated
// id is harmless here. n = 0 gives the all-clear bitmap (the caller decides what that means).
inline int ids_to_bitmap(const int32_t* ids, int n, int vocab, std::vector<uint32_t>* out) {
    const int rc = check_ids(ids, n, vocab);
    if (rc != kOk) return rc;
    std::vector<uint32_t> w(bitmap_words(vocab), 0u);
    for (int i = 0; i < n; ++i) w[(size_t)ids[i] >> 5] |= 1u << (ids[i] & 31);
    out->swap(w);
    return kOk;
}

// sparse pairs (ids [n], values [n]) -> the dense bias row fp32 [vocab], 0 where no pair names
// the id. n = 0 gives the all-zero row.
inline int bias_to_dense(const int32_t* ids, const float* values, int n, int vocab, std::vector<float>* out) {
    int rc = check_ids(ids, n, vocab);
    if (rc != kOk) return rc;
    if (n > 0 && !values) return kNullArray;
    std::vector<uint32_t> seen(bitmap_words(vocab), 0u);
    for (int i = 0; i < n; ++i) {
        if (!bias_value_ok(values[i])) return kBadValue;
        uint32_t& w = seen[(size_t)ids[i] >> 5];
        const uint32_t bit = 1u << (ids[i] & 31);
        if (w & bit) return kDuplicateId;
        w |= bit;
    }
    std::vector<float> d((size_t)vocab, 0.f);
    for (int i = 0; i < n; ++i) d[(size_t)ids[i]] = values[i];
    out->swap(d);
    return kOk;
}

}  // namespace rules_host
}  // namespace llmi
