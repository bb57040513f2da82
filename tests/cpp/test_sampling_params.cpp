// LlamaModel::setSamplingParams + Response through the C++ model API: prints the generated
// ids, which tests/test_cpp_sampling_params.py compares with the Python engine's for the same
// parameters. Without arguments it only has to compile and link (no device work).
//   test_sampling_params weight_seed n_new top_k top_p temperature repetition_penalty seed id...
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "llmi/model.h"

int main(int argc, char** argv) {
    if (argc < 9) return 0;
    try {
        const uint64_t weight_seed = std::strtoull(argv[1], nullptr, 10);
        const int n_new = std::atoi(argv[2]);
        std::vector<int> prompt;
        for (int i = 8; i < argc; ++i) prompt.push_back(std::atoi(argv[i]));
        llm::LlamaModel m("tiny", LLMI_F16, LLMI_F32);
        m.loadWeightsFromDummy(weight_seed);
        m.setSamplingParams(std::atoi(argv[3]), (float)std::atof(argv[4]), (float)std::atof(argv[5]),
                            (float)std::atof(argv[6]), std::strtoull(argv[7], nullptr, 10));
        const std::vector<int> toks = m.Response(prompt, n_new, nullptr, /*eos*/ -1);
        std::printf("{\"tokens\": [");
        for (size_t i = 0; i < toks.size(); ++i) std::printf("%s%d", i ? ", " : "", toks[i]);
        std::printf("]}\n");
        // setSampling replaces the sampler: k = 0 is greedy again
        m.setSampling(0);
        const std::vector<int> greedy = m.Response(prompt, n_new, nullptr, -1);
        std::printf("{\"greedy\": [");
        for (size_t i = 0; i < greedy.size(); ++i) std::printf("%s%d", i ? ", " : "", greedy[i]);
        std::printf("]}\n");
    } catch (const std::exception& e) {
        std::printf("{\"exception\": \"%s\"}\n", e.what());
        return 2;
    }
    return 0;
}
