// LlamaModel("tiny", LLMI_I4) (include/llmi/model.h): the fp32 .bin files under argv[1] (a prefix
// with its trailing separator) go through loadWeightsQuantized -- q/k/v, gate_up and down to 4-bit
// groups, o_proj to W8A16, on the device -- and the model greedy-decodes argv[2] tokens after the
// prompt ids argv[3..]. Also runs CreateRealLLMModel(path, preset, LLMI_I4, true) (fp16 KV cache:
// its ids are printed, not compared) and checks that the plain loadWeights refuses an int4 model.
//   -> {"tokens": [...], "factory_tokens": [...], "plain_refused": true}
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "llmi/model.h"

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: test_i4_load <prefix> <n_new> <prompt ids...>\n");
        return 2;
    }
    const std::string dir = argv[1];
    const int n_new = std::atoi(argv[2]);
    std::vector<int> prompt;
    for (int i = 3; i < argc; ++i) prompt.push_back(std::atoi(argv[i]));
    try {
        llm::LlamaModel model("tiny", LLMI_I4, LLMI_F32);
        bool refused = false;
        try {
            model.loadWeights(dir);
        } catch (const std::exception&) {
            refused = true;
        }
        model.loadWeightsQuantized(dir);
        const std::vector<int> toks = model.Response(prompt, n_new, nullptr, /*eos_token_id=*/-1);
        auto made = llm::CreateRealLLMModel(dir, "tiny", LLMI_I4, true);
        const std::vector<int> toks2 = made->Response(prompt, n_new, nullptr, -1);
        std::printf("{\"tokens\": [");
        for (size_t i = 0; i < toks.size(); ++i) std::printf(i ? ", %d" : "%d", toks[i]);
        std::printf("], \"factory_tokens\": [");
        for (size_t i = 0; i < toks2.size(); ++i) std::printf(i ? ", %d" : "%d", toks2[i]);
        std::printf("], \"plain_refused\": %s}\n", refused ? "true" : "false");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
