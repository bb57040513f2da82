// LlamaModel("tiny", LLMI_F16, LLMI_I8) (include/llmi/model.h): the int8 KV cache through the C++
// model class. Synthetic weights of seed argv[1], argv[2] greedy tokens after the prompt ids
// argv[3..]; also reads slot (layer 0, position 0) of K through llmi_engine_kv_slot_q8 on a second
// engine stepped through the C ABI, against llmi_engine_kv_slot (q * s, exact in fp32).
//   -> {"tokens": [...], "slot_ok": true}
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "llmi/model.h"

static float half_bits_to_float(uint16_t h) {
    const uint32_t s = (uint32_t)(h >> 15) << 31, e = (h >> 10) & 31, m = h & 1023;
    uint32_t b;
    if (e == 0) {
        if (m == 0) {
            b = s;
        } else {  // subnormal: m * 2^-24
            const float v = (float)m * 5.9604644775390625e-8f;
            std::memcpy(&b, &v, 4);
            b |= s;
        }
    } else if (e == 31) {
        b = s | 0x7F800000u | (m << 13);
    } else {
        b = s | ((e + 112) << 23) | (m << 13);
    }
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: test_kv8 <seed> <n_new> <prompt ids...>\n");
        return 2;
    }
    const uint64_t seed = std::strtoull(argv[1], nullptr, 10);
    const int n_new = std::atoi(argv[2]);
    std::vector<int> prompt;
    for (int i = 3; i < argc; ++i) prompt.push_back(std::atoi(argv[i]));
    try {
        llm::LlamaModel model("tiny", LLMI_F16, LLMI_I8);
        model.loadWeightsFromDummy(seed);
        const std::vector<int> toks = model.Response(prompt, n_new, nullptr, /*eos_token_id=*/-1);

        llmi_config cfg;
        LLMI_CALL(llmi_config_preset("tiny", &cfg));
        cfg.kv_dtype = LLMI_I8;
        llmi_engine* e = nullptr;
        LLMI_CALL(llmi_engine_create(&cfg, 0, nullptr, &e));
        LLMI_CALL(llmi_engine_load_synthetic(e, seed));
        LLMI_CALL(llmi_engine_set_prompt(e, prompt.data(), (int)prompt.size()));
        LLMI_CALL(llmi_engine_decode(e, 1, 0));
        std::vector<int8_t> q((size_t)cfg.kv_heads * cfg.head_dim);
        std::vector<uint16_t> sb(cfg.kv_heads);
        std::vector<float> deq(q.size());
        LLMI_CALL(llmi_engine_kv_slot_q8(e, 0, 0, 0, q.data(), sb.data()));
        LLMI_CALL(llmi_engine_kv_slot(e, 0, 0, 0, deq.data()));
        bool ok = true, any = false;
        for (int h = 0; h < cfg.kv_heads; ++h)
            for (int d = 0; d < cfg.head_dim; ++d) {
                const size_t i = (size_t)h * cfg.head_dim + d;
                ok = ok && deq[i] == (float)q[i] * half_bits_to_float(sb[h]);
                any = any || q[i] != 0;
            }
        llmi_engine_destroy(e);

        std::printf("{\"tokens\": [");
        for (size_t i = 0; i < toks.size(); ++i) std::printf(i ? ", %d" : "%d", toks[i]);
        std::printf("], \"slot_ok\": %s}\n", ok && any ? "true" : "false");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
