// LlamaModel::setLogprobs + Response + lastLogprobs through the C++ model API: prints the
// generated ids and their log-probabilities (raw bits), which tests/test_cpp_logprobs.py
// compares with the Python engine's. Without arguments it only has to compile and link (no
// device work).
//   test_logprobs weight_seed n_new n_top id...
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "llmi/model.h"

static unsigned bits(float v) {
    unsigned u;
    std::memcpy(&u, &v, 4);
    return u;
}

int main(int argc, char** argv) {
    if (argc < 5) {
        // both model classes carry the entry points
        void (Llama<float>::*set)(int) = &Llama<float>::setLogprobs;
        llm::TokenLogprobs (Llama<half_t>::*get)() = &Llama<half_t>::lastLogprobs;
        return (set && get) ? 0 : 1;
    }
    try {
        const uint64_t weight_seed = std::strtoull(argv[1], nullptr, 10);
        const int n_new = std::atoi(argv[2]);
        std::vector<int> prompt;
        for (int i = 4; i < argc; ++i) prompt.push_back(std::atoi(argv[i]));
        llm::LlamaModel m("tiny", LLMI_F16, LLMI_F32);
        m.loadWeightsFromDummy(weight_seed);
        m.setLogprobs(std::atoi(argv[3]));
        const std::vector<int> toks = m.Response(prompt, n_new, nullptr, /*eos*/ -1);
        const llm::TokenLogprobs lp = m.lastLogprobs();
        std::printf("{\"n_top\": %d, \"tokens\": [", lp.n_top);
        for (size_t i = 0; i < toks.size(); ++i) std::printf("%s%d", i ? ", " : "", toks[i]);
        std::printf("], \"logprob_bits\": [");
        for (size_t i = 0; i < lp.token.size(); ++i) std::printf("%s%u", i ? ", " : "", bits(lp.token[i]));
        std::printf("], \"top_ids\": [");
        for (size_t i = 0; i < lp.top_ids.size(); ++i) std::printf("%s%d", i ? ", " : "", lp.top_ids[i]);
        std::printf("], \"top_logprob_bits\": [");
        for (size_t i = 0; i < lp.top_logprobs.size(); ++i) std::printf("%s%u", i ? ", " : "", bits(lp.top_logprobs[i]));
        std::printf("]}\n");
        // off again: Response still answers, and there is nothing to read
        m.setLogprobs(-1);
        const std::vector<int> again = m.Response(prompt, n_new, nullptr, -1);
        bool refused = false;
        try {
            (void)m.lastLogprobs();
        } catch (const std::exception&) {
            refused = true;
        }
        std::printf("{\"off_same_tokens\": %s, \"off_refused\": %s}\n", again == toks ? "true" : "false",
                    refused ? "true" : "false");
    } catch (const std::exception& e) {
        std::printf("{\"exception\": \"%s\"}\n", e.what());
        return 2;
    }
    return 0;
}
